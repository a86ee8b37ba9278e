"""NumPy restatement of sslam_seg_map_cloud, written from its contract in include/sslam.h, and the cases of the map-cloud tests.

The contract: R, t of a cloud are cast from double to float once; x' = ((r00 x + r01 y) + r02 z) + tx in float32 (NumPy has no fused
multiply-add); a point takes part when its coordinates and its transformed coordinates are finite; cell = floor(x' * inv) in float32 with
inv = float32(1) / float32(resolution); brick = cell >> 3, local = cell & 7; per voxel the count and the sums of rint(float64(x') * 2^20)
as int64; centroid = float32((sum / 2^20) / count) in float64; voxels with count >= max(min_points, 1), ordered by (bz, by, bx, lz, ly, lx).
"""
import math

import numpy as np

INVALID, NO_DEVICE, UNSUPPORTED = -1, -2, -6


def pose12(T):
    T = np.asarray(T, np.float64)
    if T.shape in ((4, 4), (3, 4)):
        T = np.concatenate([T[:3, :3].reshape(-1), T[:3, 3]])
    return T.reshape(12)


def transform_f32(xyz, T):
    """[n, 3] float32 -> ([n, 3] float32 transformed, [n] bool: takes part)"""
    P = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    T = pose12(T).astype(np.float32)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(all="ignore"):
        out = np.stack([((T[3 * r] * x + T[3 * r + 1] * y) + T[3 * r + 2] * z) + T[9 + r] for r in range(3)], 1)
    assert out.dtype == np.float32
    ok = np.isfinite(P).all(1) & np.isfinite(out).all(1)
    return out, ok


def transform_f64(xyz, T):
    """the same with the doubles of T and float64 arithmetic, rounded to float32 at the end: NOT the contract (the cpu test shows they differ)"""
    P = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    T = pose12(T)
    with np.errstate(all="ignore"):
        out = (P @ T[:9].reshape(3, 3).T + T[9:]).astype(np.float32)
    ok = np.isfinite(P).all(1) & np.isfinite(out).all(1)
    return out, ok


def map_ref(clouds, poses, resolution, min_points=1, transform=transform_f32):
    """-> (xyz [m, 3] float32, counts [m] int32, cells [m, 3] int32, stats dict)"""
    parts = []
    n_points = 0
    for c, T in zip(clouds, poses):
        c = np.ascontiguousarray(c, np.float32).reshape(-1, 3)
        n_points += len(c)
        t, ok = transform(c, T)
        parts.append(t[ok])
    P = np.concatenate(parts, 0) if parts else np.zeros((0, 3), np.float32)
    stats = dict(n_clouds=len(clouds), n_points=n_points, n_used=len(P), n_bricks=0, n_voxels=0)
    empty = (np.zeros((0, 3), np.float32), np.zeros(0, np.int32), np.zeros((0, 3), np.int32), stats)
    if len(P) == 0:
        return empty
    inv = np.float32(1.0) / np.float32(resolution)
    cell = np.floor(P * inv).astype(np.int64)
    assert np.abs(cell).max() < 2 ** 31
    brick, local = cell >> 3, cell & 7
    fixed = np.rint(P.astype(np.float64) * 1048576.0).astype(np.int64)
    order = np.lexsort((local[:, 0], local[:, 1], local[:, 2], brick[:, 0], brick[:, 1], brick[:, 2]))
    cell, fixed = cell[order], fixed[order]
    first = np.ones(len(cell), bool)
    first[1:] = (cell[1:] != cell[:-1]).any(1)
    at = np.flatnonzero(first)
    counts = np.diff(np.append(at, len(cell)))
    sums = np.add.reduceat(fixed, at, axis=0)
    cells = cell[at]
    stats["n_voxels"] = len(at)
    stats["n_bricks"] = len(np.unique(cells >> 3, axis=0))
    keep = counts >= max(int(min_points), 1)
    cent = ((sums[keep].astype(np.float64) / 1048576.0) / counts[keep].astype(np.float64)[:, None]).astype(np.float32)
    return cent, counts[keep].astype(np.int32), cells[keep].astype(np.int32), stats


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
def _rot90(axis, quarter_turns):
    c, s = [(1, 0), (0, 1), (-1, 0), (0, -1)][quarter_turns % 4]
    R = np.eye(3)
    a, b = [(1, 2), (2, 0), (0, 1)][axis]
    R[a, a], R[a, b], R[b, a], R[b, b] = c, -s, s, c
    return R


LATTICE_RESOLUTION = 0.25                                  # inv = 4 exactly
LATTICE_SIZES = (0, 1, 63, 64, 65, 255, 256, 0, 257, 1000, 130)   # an empty cloud between two full ones; the last is all NaN / inf
LATTICE_SHARED = np.array([5.0, -7.0, 9.0]) / 16.0         # a map point every cloud with points sends one point to


def lattice_case(seed=0):
    """(clouds, poses): coordinates multiples of 1/16 in [-3, 3), poses rotations by multiples of 90 degrees about each axis in turn with
    translations multiples of 1/8 in [-1, 1].  Every arithmetic step is exact in float32, so float32 and float64 agree here: this case tests
    the cells, the order and the layout, not the rounding.  NaN / inf rows sit at rows 63 and 64 of the 257- and 1000-point clouds (the
    boundary of the first wave), and the last cloud has no usable row at all."""
    rng = np.random.default_rng(seed)
    clouds, poses = [], []
    for k, n in enumerate(LATTICE_SIZES):
        R = _rot90(k % 3, 1 + k // 3) @ _rot90((k + 1) % 3, k)
        t = rng.integers(-8, 9, 3) / 8.0
        if k == 2:
            t = np.array([-1.0, -0.625, -0.125])
        P = rng.integers(-48, 48, (n, 3)) / 16.0
        if n:
            P[n // 2] = R.T @ (LATTICE_SHARED - t)         # exact: R is a signed permutation
        P = P.astype(np.float32)
        if n in (257, 1000):
            P[63] = (np.nan, 0.0, 0.0)
            P[64] = (0.0, np.inf, 0.0)
        if k == len(LATTICE_SIZES) - 1:
            P[:] = 0.5
            P[0::3, 0] = np.nan; P[1::3, 1] = -np.inf; P[2::3, 2] = np.inf
        clouds.append(P)
        poses.append(np.concatenate([R.reshape(-1), t]))
    return clouds, poses


def random_rotation(rng):
    q = rng.normal(size=4)
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def box_points(rng, n, size=(8.0, 6.0, 3.0)):
    """n points on the six faces of a box centred on the origin"""
    P = (rng.random((n, 3)) - 0.5) * np.asarray(size)
    face = rng.integers(0, 6, n)
    P[np.arange(n), face % 3] = np.where(face < 3, -0.5, 0.5) * np.asarray(size)[face % 3]
    return P.astype(np.float32)


def generic_case(seed=1, n_clouds=40):
    """(clouds, poses): 300 .. 3000 points on the planes of a box, random rigid poses with translations up to 50 m"""
    rng = np.random.default_rng(seed)
    clouds, poses = [], []
    for k in range(n_clouds):
        clouds.append(box_points(rng, int(rng.integers(300, 3001))))
        poses.append(np.concatenate([random_rotation(rng).reshape(-1), rng.uniform(-50.0, 50.0, 3)]))
    return clouds, poses


SHARED_RESOLUTION = 0.1
SHARED_CELL = (12, -7, 3)


def shared_voxel_case(seed=2, n_clouds=8, per_cloud=7500):
    """(clouds, poses): every point of every cloud lands in the one voxel SHARED_CELL at SHARED_RESOLUTION (a margin of a fifth of the voxel
    covers the float32 rounding of the way there and back)"""
    rng = np.random.default_rng(seed)
    clouds, poses = [], []
    for k in range(n_clouds):
        R, t = random_rotation(rng), rng.uniform(-5.0, 5.0, 3)
        q = (np.asarray(SHARED_CELL) + 0.2 + 0.6 * rng.random((per_cloud, 3))) * SHARED_RESOLUTION
        clouds.append(((q - t) @ R).astype(np.float32))    # R^T (q - t)
        poses.append(np.concatenate([R.reshape(-1), t]))
    return clouds, poses


def far_case():
    """two points 3 km apart along the diagonal: 216 507 bricks per axis at resolution 0.001, far more than 2^26 in the box"""
    d = 3000.0 / math.sqrt(3.0)
    return [np.array([[0.0, 0.0, 0.0], [d, d, d]], np.float32)], [np.concatenate([np.eye(3).reshape(-1), np.zeros(3)])]
