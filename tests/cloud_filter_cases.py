"""Inputs and plain float64 references for the cloud filters (voxel grid, statistical outlier removal, k-means) -- test helper, not
collected.  tests/test_cloud_filters_cpu.py and tests/test_cloud_filters_gpu.py share it.

The references do not come from oracle/np_filters.py: they are the textbook form of each operation in float64,

    voxel_reference     group the finite points by floor(float32(x) * float32(1 / leaf)), float64 mean per group, groups in (z, y, x) order
    sor_reference       brute-force k nearest neighbours among the finite points, float64 mean of the k distances
    kmeans_reference    float64 mean of the points that carry each label

and the bars are derived from the number formats, not from what the kernels give:

    centroid_bar(m) = 2 * (2^-21 + 2^-24 |m|)   one 2^-20 fixed-point rounding (<= 2^-21) per point, carried through the mean, plus half a
                                                float32 ulp of the final cast; a margin of two over that
    SOR_REL = 8 * 2^-24                         five float32 roundings in the squared distance, halved by the root, the root's own rounding
                                                and the final cast; order statistics are 1-Lipschitz, a swapped near-tie costs nothing more

Every case is built once (lru_cache) and handed out read-only.
"""
from __future__ import annotations

import functools

import numpy as np

F = np.float32
NAN = np.nan
SOR_REL = 8.0 * 2.0 ** -24
SSLAM_ERR_INVALID = -1
SSLAM_ERR_UNSUPPORTED = -6
MAX_CELLS = 1 << 26


def centroid_bar(m):
    return 2.0 * (2.0 ** -21 + 2.0 ** -24 * np.abs(m))


def _ro(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


# ---- references -------------------------------------------------------------------------------------------------------------------
def voxel_keys(xyz, leaf):
    """(finite mask, int64 cell key [m, 3] of every finite point): floor(float32(x) * float32(1 / leaf)), the rule of pcl::VoxelGrid"""
    p = np.asarray(xyz, F).reshape(-1, 3)
    fin = np.isfinite(p).all(1)
    inv = F(1.0) / F(leaf)
    return fin, np.floor((p[fin] * inv).astype(F)).astype(np.int64)


def voxel_geometry(xyz, leaf):
    """(minb[3], div[3]) of the grid over the finite points, from the keys alone"""
    _, key = voxel_keys(xyz, leaf)
    return key.min(0), key.max(0) - key.min(0) + 1


def voxel_reference(xyz, leaf):
    """(float64 mean [m, 3], count [m]) per occupied voxel, voxels in ascending (z, y, x) key"""
    p = np.asarray(xyz, F).reshape(-1, 3)
    fin, key = voxel_keys(p, leaf)
    if not len(key):
        return np.zeros((0, 3)), np.zeros(0, np.int64)
    q = p[fin].astype(np.float64)
    order = np.lexsort((key[:, 0], key[:, 1], key[:, 2]))
    ks, qs = key[order], q[order]
    first = np.r_[True, (ks[1:] != ks[:-1]).any(1)]
    start = np.flatnonzero(first)
    count = np.diff(np.r_[start, len(ks)])
    return np.add.reduceat(qs, start, axis=0) / count[:, None], count


def sor_reference(xyz, mean_k):
    """float64 mean distance of every finite point to its mean_k nearest finite neighbours (itself excluded); -1 for the other rows"""
    p = np.asarray(xyz, F).reshape(-1, 3)
    fin = np.isfinite(p).all(1)
    q = p[fin].astype(np.float64)
    d = np.sqrt(((q[:, None, :] - q[None, :, :]) ** 2).sum(2))
    d.sort(axis=1)
    out = np.full(len(p), -1.0)
    out[fin] = d[:, 1:mean_k + 1].mean(1)
    return out


def kmeans_reference(pts, labels, k):
    """(float64 mean [k, dim] of the points carrying each label, NaN rows for empty clusters; counts [k])"""
    p = np.asarray(pts, F)
    p = p.reshape(len(p), -1).astype(np.float64)
    mean = np.full((k, p.shape[1]), NAN)
    cnt = np.bincount(labels, minlength=k)
    for j in range(k):
        if cnt[j]:
            mean[j] = p[labels == j].mean(0)
    return mean, cnt


# ---- voxel grid cases: name -> (xyz float32 [n, 3], leaf) -------------------------------------------------------------------------------
VOXEL_SIZES = (1, 63, 64, 65, 255, 256, 257)
VOXEL_BIG = 65793                   # 257 blocks of 256: one past the 256-block cap of k_voxel_minmax, whose grid-stride loop then runs
VOXEL_LEAVES = (0.04, 0.1, 0.125, 1.0)
FACE_LEAVES = (0.1, 0.04, 0.125)
FACE_K = np.arange(-400, 401)
SPARSE_NCELL = (1 << 22, 1 << 23)
SPARSE_MAX_OCCUPIED = 100


def _uniform_cloud(n, seed):
    """n points in a 3 x 2 x 1.8 m box; the LAST point sits alone outside it, so it moves the bounding box and owns a voxel: a kernel that
    drops the tail of a wave or of a block loses both"""
    rng = np.random.default_rng(seed)
    p = rng.uniform((-1.5, -1.0, 0.2), (1.5, 1.0, 2.0), (n, 3)).astype(F)
    p[n - 1] = (2.05, 1.55, 2.55)
    return p


def face_lattice(leaf):
    """float32(k) * float32(leaf) for k = -400 .. 400 with -0.0 next to 0.0: every value sits (in exact arithmetic) on a voxel face"""
    v = (FACE_K.astype(F) * F(leaf)).astype(F)
    return np.concatenate([v, np.array([-0.0], F)])


def _face_cloud(leaf, axis):
    """the lattice along `axis`; the two other coordinates take lattice values of k = -2 .. 2, so the grid stays 801 x 5 x 5"""
    rng = np.random.default_rng(1000 + axis)
    v = face_lattice(leaf)
    p = (rng.integers(-2, 3, (len(v), 3)).astype(F) * F(leaf)).astype(F)
    p[:, axis] = v
    return p[rng.permutation(len(p))]


def _nonfinite(name):
    rng = np.random.default_rng(77)
    if name == "interleaved":
        p = rng.uniform(-1, 1, (600, 3)).astype(F)
        for i in range(600):
            if i % 3 == 1:
                p[i, i % 2] = NAN
            elif i % 7 == 3:
                p[i, (i // 7) % 3] = np.inf if i % 2 else -np.inf
        return p
    n, a, b = {"wave": (300, 64, 128), "block": (700, 256, 512), "first_block": (700, 0, 256), "all": (130, 0, 130)}[name]
    p = rng.uniform(-1, 1, (n, 3)).astype(F)
    bad = np.array([NAN, np.inf, -np.inf], F)
    for i in range(a, b):
        p[i, i % 3] = bad[(i // 3) % 3]
    return p


def _two_clusters(offset):
    rng = np.random.default_rng(5)
    a = rng.uniform(0.01, 0.14, (30, 3))
    b = rng.uniform(0.01, 0.14, (30, 3)) + np.asarray(offset)
    p = np.vstack([a, b]).astype(F)
    return p[rng.permutation(len(p))]


@functools.lru_cache(maxsize=None)
def voxel_case(name):
    kind, _, arg = name.partition(":")
    if kind == "size":
        n, leaf = arg.split("@")
        return _ro(_uniform_cloud(int(n), int(n))), float(leaf)
    if kind == "one_voxel":            # 60 000 points in one cell: every atomic of k_voxel_accumulate lands on the same three sums
        rng = np.random.default_rng(3)
        return _ro(rng.uniform(0.31, 0.39, (60000, 3)).astype(F)), 0.1
    if kind == "lattice":              # the exact centres of a 16 x 12 x 7 block of cells at a binary leaf, one point each, shuffled
        g = np.stack(np.meshgrid(np.arange(16), np.arange(12), np.arange(7), indexing="ij"), -1).reshape(-1, 3)
        p = ((g + 0.5) * 0.125 - np.array([1.0, 0.5, 0.25])).astype(F)
        return _ro(p[np.random.default_rng(4).permutation(len(p))]), 0.125
    if kind == "negative":
        return _ro(np.random.default_rng(6).uniform(-3.0, -0.5, (3000, 3)).astype(F)), 0.1
    if kind == "face":
        leaf, axis = arg.split("@")
        return _ro(_face_cloud(float(leaf), int(axis))), float(leaf)
    if kind == "nonfinite":
        return _ro(_nonfinite(arg)), 0.1
    if kind == "sparse":               # two clusters 16.5 m apart on every axis: 4.8e6 cells, a few dozen of them occupied
        return _ro(_two_clusters((16.5, 16.5, 16.5))), 0.1
    if kind == "sparse_flat":          # a flat grid whose z stride (div[0] * div[1]) is beyond 2^16
        return _ro(_two_clusters((30.0, 25.0, 0.5))), 0.1
    raise KeyError(name)


VOXEL_CASES = ([f"size:{n}@{leaf}" for n in VOXEL_SIZES for leaf in VOXEL_LEAVES] + [f"size:{VOXEL_BIG}@0.1", "one_voxel", "lattice", "negative"]
               + [f"face:{leaf}@{axis}" for leaf in FACE_LEAVES for axis in range(3)]
               + [f"nonfinite:{k}" for k in ("interleaved", "wave", "block", "first_block", "all")] + ["sparse", "sparse_flat"])
CAPACITY_VOXEL_CASE = "size:257@0.1"
# ordinary coordinates, a grid of 501^3 > 2^26 cells at leaf 0.1: refused with SSLAM_ERR_UNSUPPORTED
TOO_MANY_CELLS = (_ro(np.array([[0, 0, 0], [50, 50, 50], [1, 2, 3]], F)), 0.1)


# ---- outlier removal cases: name -> (xyz, mean_k, stddev_mul) ---------------------------------------------------------------------------
SOR_MEAN_K = (1, 8, 50, 63)
SOR_MULS = (0.0, 1.0, 2.0)


def sor_sizes(mean_k):
    return sorted({n for n in (mean_k + 1, 127, 128, 129, 257, 700) if n >= mean_k + 1})


def _blob(n, seed):
    """a Gaussian blob with a twelfth of the points scattered far around it; the last point is a stray"""
    rng = np.random.default_rng(seed)
    p = rng.normal(0, 0.3, (n, 3))
    stray = rng.choice(n, max(n // 12, 1), replace=False)
    p[stray] += rng.uniform(-3, 3, (len(stray), 3))
    p[n - 1] = (4.0, -4.0, 4.0)
    return p.astype(F)


@functools.lru_cache(maxsize=None)
def sor_case(name):
    kind, _, arg = name.partition(":")
    if kind == "size":
        k, n, mul = arg.split("@")
        return _ro(_blob(int(n), 100 * int(k) + int(n))), int(k), float(mul)
    if kind == "offset":               # far from the origin: the differences stay exact, the squares do not cancel
        rng = np.random.default_rng(8)
        return _ro((np.array([100.0, -50.0, 30.0]) + rng.normal(0, 0.01, (300, 3))).astype(F)), 8, float(arg)
    if kind == "duplicates":           # every distance 0: mean 0, deviation 0, nothing above the threshold
        return _ro(np.tile(np.array([[0.7, -1.3, 2.1]], F), (130, 1))), 8, float(arg)
    if kind == "nan_rows":             # exactly mean_k + 1 finite points among NaN rows
        rng = np.random.default_rng(9)
        p = rng.normal(0, 0.3, (20, 3)).astype(F)
        p[[0, 2, 3, 5, 8, 9, 11, 13, 14, 17, 19], 1] = NAN
        return _ro(p), 8, 1.0
    if kind == "overflow":             # 38 ordinary points and two at +-3e19: a squared distance to either is past FLT_MAX = 3.4e38
        rng = np.random.default_rng(10)
        p = rng.normal(0, 0.3, (40, 3)).astype(F)
        p[7] = (3e19, 0, 0); p[31] = (-3e19, 0, 0)
        return _ro(p), 39, 1.0
    raise KeyError(name)


def _sor_size_names():
    out, i = [], 0
    for k in SOR_MEAN_K:
        for n in sor_sizes(k):
            out.append(f"size:{k}@{n}@{SOR_MULS[i % 3]}"); i += 1
    return out


SOR_CASES = (_sor_size_names() + [f"size:50@257@{m}" for m in SOR_MULS] + [f"offset:{m}" for m in SOR_MULS] + ["duplicates:0.0", "duplicates:1.0"]
             + ["nan_rows", "overflow"])
CAPACITY_SOR_CASE = "size:8@257@1.0"


def sor_too_few_finite():
    """the nan_rows cloud with one more row lost: mean_k finite points, refused"""
    p, k, mul = sor_case("nan_rows")
    q = p.copy()
    q[np.flatnonzero(np.isfinite(p).all(1))[0], 2] = np.inf
    assert np.isfinite(q).all(1).sum() == k
    return q, k, mul


# ---- k-means cases: name -> (points float32 [n, dim], k, expected number of empty clusters or None) ------------------------------------
KM_SIZES = (1, 5, 65, 255, 256, 257, 513)
KM_K = (1, 2, 4, 16)
KM_DIMS = (1, 3)
KM_SEEDS = (0, 5, 11)


@functools.lru_cache(maxsize=None)
def kmeans_points(n, dim):
    """three blobs (two in 1-D are closer than the third), the last point apart from all of them"""
    rng = np.random.default_rng(10 * n + dim)
    cen = np.array([[0.0, 0.0, 1.0], [1.0, 0.2, 0.0], [-2.0, 1.0, 0.5]])[:, :dim]
    p = cen[rng.integers(0, 3, n)] + rng.normal(0, 0.05, (n, dim))
    p[n - 1] = np.array([3.0, -1.0, 2.0])[:dim]
    return _ro(p.astype(F))


@functools.lru_cache(maxsize=None)
def kmeans_special(name):
    rng = np.random.default_rng(12)
    if name == "one_point":
        return _ro(np.array([[0.3, -0.2, 0.9]], F)), 2, 1
    if name == "identical":            # all distances tie: the lowest centre takes every point, three clusters stay empty
        return _ro(np.tile(np.array([[0.25, 0.5, -0.75]], F), (300, 1))), 4, 3
    if name == "five_points":
        return kmeans_points(5, 3), 16, None          # at least 11 clusters are empty
    if name == "two_blobs":            # 5 apart along x, 0.01 wide: the outermost centres take a blob each, the two between them nothing
        p = np.vstack([rng.normal(0, 0.01, (150, 3)), rng.normal(0, 0.01, (150, 3)) + (5.0, 0, 0)])
        return _ro(p[rng.permutation(300)].astype(F)), 4, 2
    if name == "two_blobs_1d":
        p = np.concatenate([rng.normal(-1.0, 0.01, 150), rng.normal(4.0, 0.01, 150)])
        return _ro(p[rng.permutation(300)].astype(F).reshape(-1, 1)), 4, 2
    if name == "constant_coordinate":  # the bounding box has no extent in y: every random centre shares that coordinate
        p = kmeans_points(257, 3).copy(); p[:, 1] = F(0.375)
        return _ro(p), 4, None
    raise KeyError(name)


KM_SPECIAL = ("one_point", "identical", "five_points", "two_blobs", "two_blobs_1d", "constant_coordinate")


# ---- the comparisons with the references, shared by both files -------------------------------------------------------------------------
def check_voxel_against_reference(cent, cnt, xyz, leaf):
    """the invariants the GPU file asserts on the kernels' output, here for any (centroids, counts)"""
    mean, count = voxel_reference(xyz, leaf)
    assert np.array_equal(cnt, count) and int(np.sum(cnt)) == int(np.isfinite(xyz).all(1).sum())
    if len(cnt) == 0:
        return 0.0
    # ascending cell order: the cell of every centroid's own group, recomputed from the reference's key order
    fin, key = voxel_keys(xyz, leaf)
    ks = key[np.lexsort((key[:, 0], key[:, 1], key[:, 2]))]
    first = np.r_[True, (ks[1:] != ks[:-1]).any(1)]
    minb, div = voxel_geometry(xyz, leaf)
    cell = ((ks[first] - minb) * np.array([1, div[0], div[0] * div[1]])).sum(1)
    assert (np.diff(cell) > 0).all()
    err = np.abs(cent.astype(np.float64) - mean)
    bar = centroid_bar(mean)
    assert (err <= bar).all(), f"centroid off its float64 mean by {float((err / bar).max()):.3f} of the bar"
    return float((err / bar).max())


def check_sor_against_reference(md, xyz, mean_k):
    """every mean distance within SOR_REL of the float64 one (not for the overflow case, whose means are asserted to be +inf); returns
    the worst error in units of 2^-24 relative"""
    ref = sor_reference(xyz, mean_k)
    fin = np.isfinite(xyz).all(1)
    assert np.array_equal(md[~fin], np.full((~fin).sum(), -1.0, F))
    err = np.abs(md[fin].astype(np.float64) - ref[fin])
    assert (err <= SOR_REL * ref[fin]).all(), f"mean distance off by {float((err / np.maximum(ref[fin], 1e-300)).max() / 2.0 ** -24):.2f} x 2^-24"
    return float((err / np.maximum(ref[fin], 1e-300)).max() / 2.0 ** -24)


def check_kmeans_against_reference(pts, lab, cen, k):
    """a non-empty cluster's centre within the centroid bar of the float64 mean of its points, an empty one's inside the bounding box"""
    mean, cnt = kmeans_reference(pts, lab, k)
    p = pts.reshape(len(pts), -1)
    lo, hi = p.min(0), p.max(0)
    for j in range(k):
        if cnt[j]:
            err = np.abs(cen[j].astype(np.float64) - mean[j])
            assert (err <= centroid_bar(mean[j])).all(), (j, err, mean[j])
        else:
            assert (cen[j] >= lo).all() and (cen[j] <= hi).all(), (j, cen[j], lo, hi)
    return cnt
