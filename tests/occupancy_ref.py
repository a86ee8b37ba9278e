"""Restatement of sslam_seg_occupancy_map, written from its contract in include/sslam.h, a second reference for the traversal that does not
come from that contract, and the cases of the occupancy tests.  Shares no code with the library.

The contract, per ray: the end point and the sensor origin are transformed in float32 without fused multiply-add,
x' = ((r00 x + r01 y) + r02 z) + tx.  Position of a coordinate p: u = p * inv (float32, inv = 1 / resolution), c = floor(u),
f = u - floor(u), q = min(int(f * 1024), 1023), Q = c * 1024 + q (an integer in 1/1024 cell).  D = Qe - Qo; a ray with |D|^2 > R^2,
R = floor(max_range * inv * 1024) in double, is cut: D_a = trunc(D_a * R / L) with L = ceil(sqrt(|D|^2)), exact.  The walk makes
|ce_a - co_a| steps per axis (cell = Q >> 10), each time on the axis, among those with steps left, whose next face has the smallest
parameter num_a / |D_a| (num_a = 1024 - qo_a going up, qo_a going down, + 1024 per step); exact ties go to the lowest axis.  Every cell but
the last gets a miss; the last a hit, or a miss when the ray was cut.  Log-odds = clamp(float32(hits) * l_hit + float32(misses) * l_miss).

Three implementations: occupancy_ref (Python ints, one ray at a time: the restatement the tests compare with), occupancy_ref_vec (NumPy
int64 over all rays at once, a dense table of counts, for tools/occupancy_timing.py's millions of rays; the cpu test holds it equal to the first), and
segment_cells_exact (fractions.Fraction: which cells does the exact segment Qo -> Qe meet -- no walk at all).
"""
import math
from fractions import Fraction

import numpy as np

INVALID, NO_DEVICE, UNSUPPORTED = -1, -2, -6
FAR = 524288.0                                             # |u| at or beyond 2^19 cells: the call is refused
F32 = np.float32


class Unsupported(Exception):
    pass


def logodds(p):
    return F32(math.log(p / (1.0 - p)))


def default_params(**kw):
    """the defaults of sslam_occ_default_params; every float a numpy float32, as the kernels see them"""
    P = dict(resolution=F32(0.05), max_range=F32(10.0), z_min=F32(-1.0), z_max=F32(5.0), sensor_origin=np.zeros(3, F32),
             l_hit=logodds(0.7), l_miss=logodds(0.4), l_min=logodds(0.1192), l_max=logodds(0.971), l_occ=logodds(0.5), emit=0)
    for k, v in kw.items():
        assert k in P, k
        P[k] = np.asarray(v, F32).reshape(3) if k == "sensor_origin" else (int(v) if k == "emit" else F32(v))
    return P


def pose12(T):
    T = np.asarray(T, np.float64)
    if T.shape in ((4, 4), (3, 4)):
        T = np.concatenate([T[:3, :3].reshape(-1), T[:3, 3]])
    return T.reshape(12)


def transform(xyz, T):
    """[n, 3] float32 at the pose T (12 doubles, cast to float32 once): ([n, 3] float32, [n] bool: finite before and after)"""
    P = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    T = pose12(T).astype(F32)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(all="ignore"):
        out = np.stack([((T[3 * r] * x + T[3 * r + 1] * y) + T[3 * r + 2] * z) + T[9 + r] for r in range(3)], 1)
    assert out.dtype == F32
    return out, np.isfinite(P).all(1) & np.isfinite(out).all(1)


def range_units(P):
    inv = F32(1.0) / P["resolution"]
    return int(math.floor(float(P["max_range"]) * float(inv) * 1024.0))


def position(p, inv):
    """one float32 coordinate -> Q, a Python int; Unsupported beyond 2^19 cells"""
    u = F32(p) * inv
    if not abs(float(u)) < FAR:
        raise Unsupported("cell %g" % float(u))
    fl = np.floor(u)
    f = u - fl
    assert f.dtype == F32
    return int(fl) * 1024 + min(int(f * F32(1024.0)), 1023)


def cut(Qo, Qe, R):
    """-> (Qe after the range rule, truncated)"""
    D = [e - o for o, e in zip(Qo, Qe)]
    len2 = sum(d * d for d in D)
    if len2 <= R * R:
        return list(Qe), False
    L = math.isqrt(len2)
    if L * L < len2:
        L += 1
    D = [(abs(d) * R // L) * (1 if d >= 0 else -1) for d in D]     # C division: towards zero
    return [o + d for o, d in zip(Qo, D)], True


def walk(Qo, Qe):
    """the cells of the walk from Qo to Qe (after cut), in order; the last one is the end cell"""
    D = [e - o for o, e in zip(Qo, Qe)]
    cell = [o >> 10 for o in Qo]
    left = [abs((e >> 10) - (o >> 10)) for o, e in zip(Qo, Qe)]
    num = [(1024 - (o & 1023)) if d > 0 else (o & 1023) for o, d in zip(Qo, D)]
    out = [tuple(cell)]
    while sum(left):
        best = None
        for a in range(3):
            if left[a] and (best is None or num[a] * abs(D[best]) < num[best] * abs(D[a])):   # strictly smaller: a tie stays with the lower axis
                best = a
        cell[best] += 1 if D[best] > 0 else -1
        num[best] += 1024
        left[best] -= 1
        out.append(tuple(cell))
    assert out[-1] == tuple(e >> 10 for e in Qe)
    return out


def rays_of(clouds, poses, P):
    """every ray that takes part: (Qo, Qe, truncated) in cloud and point order, and the counters of pass 0"""
    inv = F32(1.0) / P["resolution"]
    R = range_units(P)
    assert 1 <= R <= 1 << 20
    st = dict(n_clouds=len(clouds), n_points=0, n_rays=0, n_truncated=0, n_clipped_z=0)
    rays = []
    for c, T in zip(clouds, poses):
        c = np.ascontiguousarray(c, F32).reshape(-1, 3)
        st["n_points"] += len(c)
        o, o_ok = transform(P["sensor_origin"].reshape(1, 3), T)
        if not o_ok[0] or len(c) == 0:
            continue
        t, ok = transform(c, T)
        Qo = None
        for p in t[ok]:
            if not (P["z_min"] <= p[2] <= P["z_max"]):
                st["n_clipped_z"] += 1
                continue
            if Qo is None:
                Qo = [position(v, inv) for v in o[0]]
            Qe, tr = cut(Qo, [position(v, inv) for v in p], R)
            rays.append((Qo, Qe, tr))
            st["n_rays"] += 1
            st["n_truncated"] += tr
    return rays, st


def cell_logodds(hits, misses, P):
    t = hits.astype(F32) * P["l_hit"] + misses.astype(F32) * P["l_miss"]
    assert t.dtype == F32
    return np.fmin(np.fmax(t, P["l_min"]), P["l_max"])


def _records(cells, hits, misses, P, st):
    """cells [m, 3] int64 (unique), hits, misses -> the ordered, emit-filtered records and the stats"""
    st = dict(st, n_steps=int(hits.sum() + misses.sum()), n_cells=len(cells), n_bricks=0)
    if len(cells):
        b = (cells >> 3) - (cells >> 3).min(0)
        nb = b.max(0) + 1
        brick = (b[:, 2] * nb[1] + b[:, 1]) * nb[0] + b[:, 0]                  # bricks ascending with x fastest ...
        l = cells & 7
        order = np.argsort(brick * 512 + ((l[:, 2] << 6) | (l[:, 1] << 3) | l[:, 0]), kind="stable")   # ... then the local index, x fastest
        st["n_bricks"] = len(np.unique(brick))
        cells, hits, misses = cells[order], hits[order], misses[order]
    lo = cell_logodds(hits, misses, P)
    keep = np.ones(len(cells), bool) if P["emit"] == 0 else (lo >= P["l_occ"]) if P["emit"] == 1 else (lo < P["l_occ"])
    return cells[keep].astype(np.int32).reshape(-1, 3), hits[keep].astype(np.int32), misses[keep].astype(np.int32), lo[keep], st


def occupancy_ref(clouds, poses, P):
    """-> (cells [m, 3] int32, hits [m] int32, misses [m] int32, logodds [m] float32, stats dict); raises Unsupported"""
    rays, st = rays_of(clouds, poses, P)
    table = {}
    for Qo, Qe, tr in rays:
        path = walk(Qo, Qe)
        for c in path[:-1]:
            table.setdefault(c, [0, 0])[1] += 1
        table.setdefault(path[-1], [0, 0])[1 if tr else 0] += 1
    cells = np.array(sorted(table), np.int64).reshape(-1, 3)
    hm = np.array([table[tuple(c)] for c in cells.tolist()], np.int64).reshape(-1, 2)
    return _records(cells, hm[:, 0], hm[:, 1], P, st)


# ---- the same over all rays at once (NumPy int64) --------------------------------------------------------------------------------------
def _positions_vec(p, inv):
    u = p * inv
    assert u.dtype == F32
    if not (np.abs(u) < F32(FAR)).all():
        raise Unsupported("cell beyond 2^19")
    fl = np.floor(u)
    return fl.astype(np.int64) * 1024 + np.minimum(((u - fl) * F32(1024.0)).astype(np.int64), 1023)


def occupancy_ref_vec(clouds, poses, P):
    """occupancy_ref over all rays at once; the counts live in a dense table over the box of the cells (at most 2^29 of them)"""
    inv = F32(1.0) / P["resolution"]
    R = range_units(P)
    st = dict(n_clouds=len(clouds), n_points=0, n_rays=0, n_truncated=0, n_clipped_z=0)
    Qo_l, Qe_l = [], []
    for c, T in zip(clouds, poses):
        c = np.ascontiguousarray(c, F32).reshape(-1, 3)
        st["n_points"] += len(c)
        o, o_ok = transform(P["sensor_origin"].reshape(1, 3), T)
        if not o_ok[0] or len(c) == 0:
            continue
        t, ok = transform(c, T)
        t = t[ok]
        inz = (t[:, 2] >= P["z_min"]) & (t[:, 2] <= P["z_max"])
        st["n_clipped_z"] += int((~inz).sum())
        t = t[inz]
        if len(t) == 0:
            continue
        Qe_l.append(_positions_vec(t, inv))
        Qo_l.append(np.broadcast_to(_positions_vec(o, inv), Qe_l[-1].shape))
    if not Qe_l:
        z = np.zeros(0, np.int64)
        return _records(z.reshape(0, 3), z, z, P, st)
    Qo, Qe = np.concatenate(Qo_l), np.concatenate(Qe_l)
    D = Qe - Qo
    len2 = (D * D).sum(1)
    tr = len2 > R * R
    L = np.ceil(np.sqrt(len2.astype(np.float64))).astype(np.int64)
    L += L * L < len2
    L -= (L - 1) * (L - 1) >= len2
    assert ((L * L >= len2) & ((L - 1) * (L - 1) < len2) | (len2 == 0)).all()
    Dc = np.sign(D) * (np.abs(D) * R // np.maximum(L, 1)[:, None])
    D = np.where(tr[:, None], Dc, D)
    Qe = Qo + D
    st["n_rays"], st["n_truncated"] = len(D), int(tr.sum())
    cell, ce = Qo >> 10, Qe >> 10
    lo3 = np.minimum(cell.min(0), ce.min(0))
    ext = np.maximum(cell.max(0), ce.max(0)) - lo3 + 1
    key = lambda c: ((c[:, 2] - lo3[2]) * ext[1] + (c[:, 1] - lo3[1])) * ext[0] + (c[:, 0] - lo3[0])
    left = np.abs(ce - cell)
    num = np.where(D > 0, 1024 - (Qo & 1023), Qo & 1023)
    aD, step = np.abs(D), np.sign(D)
    assert int(ext[0]) * int(ext[1]) * int(ext[2]) <= 1 << 29, "the box of the cells is too large for the dense table"
    hits_d, misses_d = np.zeros(int(ext.prod()), np.int32), np.zeros(int(ext.prod()), np.int32)
    while len(cell):
        done = left.sum(1) == 0
        if done.any():
            k = key(cell[done])
            np.add.at(hits_d, k[~tr[done]], 1); np.add.at(misses_d, k[tr[done]], 1)
            go = ~done
            cell, left, num, aD, step, tr = cell[go], left[go], num[go], aD[go], step[go], tr[go]
            if not len(cell):
                break
        np.add.at(misses_d, key(cell), 1)
        ok = left > 0
        nx, ny, nz = num[:, 0], num[:, 1], num[:, 2]
        dx, dy, dz = aD[:, 0], aD[:, 1], aD[:, 2]
        xy = ok[:, 0] & (~ok[:, 1] | (nx * dy <= ny * dx))
        xz = ~ok[:, 2] | (nx * dz <= nz * dx)
        yz = ~ok[:, 2] | (ny * dz <= nz * dy)
        a = np.where(xy, np.where(xz, 0, 2), np.where(ok[:, 1], np.where(yz, 1, 2), 2))
        r = np.arange(len(a))
        cell[r, a] += step[r, a]; num[r, a] += 1024; left[r, a] -= 1
    keys = np.flatnonzero(hits_d | misses_d)
    hits, misses = hits_d[keys].astype(np.int64), misses_d[keys].astype(np.int64)
    cells = np.stack([keys % ext[0] + lo3[0], keys // ext[0] % ext[1] + lo3[1], keys // (ext[0] * ext[1]) + lo3[2]], 1)
    return _records(cells, hits, misses, P, st)


# ---- the second reference: the exact segment against the cubes, no walk ----------------------------------------------------------------
def segment_cells_exact(Qo, Qe):
    """-> (touched, crossed): the cells whose CLOSED cube [1024 c, 1024 (c + 1)]^3 the segment Qo + t (Qe - Qo), t in [0, 1], meets, and
    those whose OPEN cube it meets.  Per cell and axis the parameter interval is computed in fractions.Fraction."""
    D = [e - o for o, e in zip(Qo, Qe)]
    rng = [range(min(o, e) // 1024 - 1, max(o, e) // 1024 + 2) for o, e in zip(Qo, Qe)]
    touched, crossed = set(), set()
    for cx in rng[0]:
        for cy in rng[1]:
            for cz in rng[2]:
                lo, hi = Fraction(0), Fraction(1)          # closed interval of t inside the closed cube
                olo, ohi = Fraction(-1), Fraction(2)       # open interval of t inside the open cube (before [0, 1])
                inside = strictly = True
                for c, o, d in zip((cx, cy, cz), Qo, D):
                    a, b = 1024 * c, 1024 * (c + 1)
                    if d == 0:
                        inside &= a <= o <= b
                        strictly &= a < o < b
                    else:
                        t0, t1 = sorted((Fraction(a - o, d), Fraction(b - o, d)))
                        lo, hi = max(lo, t0), min(hi, t1)
                        olo, ohi = max(olo, t0), min(ohi, t1)
                if inside and lo <= hi:
                    touched.add((cx, cy, cz))
                if strictly and olo < ohi and olo < 1 and ohi > 0:
                    crossed.add((cx, cy, cz))
    return touched, crossed


def ties_of(Qo, Qe):
    """the largest number of axes (1, 2 or 3) whose next faces had exactly equal parameters at some step of the walk"""
    D = [e - o for o, e in zip(Qo, Qe)]
    left = [abs((e >> 10) - (o >> 10)) for o, e in zip(Qo, Qe)]
    num = [(1024 - (o & 1023)) if d > 0 else (o & 1023) for o, d in zip(Qo, D)]
    worst = 1 if sum(left) else 0
    while sum(left):
        t = {a: Fraction(num[a], abs(D[a])) for a in range(3) if left[a]}
        best = min(t, key=lambda a: (t[a], a))
        worst = max(worst, sum(v == t[best] for v in t.values()))
        num[best] += 1024
        left[best] -= 1
    return worst


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
LATTICE_SIZES = (63, 64, 65, 255, 256, 257)


def identity_pose(t=(0.0, 0.0, 0.0)):
    return np.concatenate([np.eye(3).reshape(-1), np.asarray(t, np.float64)])


def lattice_params(**kw):
    return default_params(resolution=0.125, max_range=2.5, z_min=-1.0, z_max=1.75, sensor_origin=(0.25, -0.125, 0.5), **kw)


def lattice_case(seed=0):
    """(clouds, poses): six clouds of LATTICE_SIZES points.  Every coordinate, the sensor origin and every translation is a multiple of
    1/64 and the resolution is 1/8, so every float32 step is exact, positions are multiples of 128 / 1024 of a cell, and rays through
    cell edges and corners are exact ties.  The first rows of every cloud are made by hand, relative to the ray origin g of the cloud:
    diagonals in two and three axes (ties), ends on cell faces reached going down, ends inside the origin's cell (zero steps), four
    copies of one map point and six more map points in every cloud (shared cells, the clamp at l_max), far ends (cut) and ends above and below the z range."""
    rng = np.random.default_rng(seed)
    org = np.array([0.25, -0.125, 0.5])
    trans = np.array([[0, 0, 0], [-24, 40, 8], [16, -72, -8], [-128, -64, 0], [1, 3, 5], [-35, 9, -3]]) / 64.0   # the first four keep the origin on a cell corner
    clouds, poses = [], []
    for k, n in enumerate(LATTICE_SIZES):
        g = org + trans[k]                                 # the ray origin in the map
        rows = []
        for a in (3, 5, 8, 11):                            # two- and three-axis diagonals, in cells
            for sx, sy in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
                rows.append(g + np.array([sx * a, sy * a, 0]) / 8.0)
                rows.append(g + np.array([sx * a, 0, sy * min(a, 5)]) / 8.0)
            rows.append(g + np.array([a, a, a]) * (1 if a < 8 else -1) / 8.0 * (0.5 if a >= 8 else 1))
        for j in range(6):                                 # going down on x and y, ending exactly on faces (multiples of 1/8)
            rows.append(np.floor((g - np.array([0.4 + 0.3 * j, 0.2 * j + 0.13, 0.0])) * 8.0) / 8.0 + np.array([0, 0, 1 / 64.0]))
        for j in range(3):                                 # inside the origin's cell: zero steps
            rows.append(np.floor(g * 8.0) / 8.0 + np.array([1 + j, 2, 3 + j]) / 64.0)
        rows += [np.array([1.0 + 3 / 64.0, 0.5 + 5 / 64.0, 0.75 + 1 / 64.0])] * 4    # the same map point four times, in every cloud
        for j in range(6):                                 # six more map points that every cloud sees: shared end cells
            rows.append(np.array([1.5 + 9 * j / 64.0, 0.75 + 1 / 64.0, 0.25 + (j % 3) / 8.0 + 3 / 64.0]))
        for j in range(4):                                 # beyond max_range
            rows.append(g + np.array([2.0 + 0.25 * j, -1.75, 0.25]) * (1 if j % 2 else -1))
        for j in range(4):                                 # outside the z range (the last two exactly ON its bounds: they stay)
            rows.append(np.array([g[0] + 0.5, g[1] - 0.25 * j, (2.0, -1.25, 1.75, -1.0)[j]]))
        rows = np.array(rows[:n])
        rest = np.stack([rng.integers(-160, 160, n - len(rows)), rng.integers(-160, 160, n - len(rows)), rng.integers(-96, 144, n - len(rows))], 1) / 64.0
        world = np.concatenate([rows, rest + np.round(g * 64.0) / 64.0 * np.array([1, 1, 0])])
        clouds.append((world - trans[k]).astype(F32))     # exact: multiples of 1/64 below 2^24 / 64
        poses.append(identity_pose(trans[k]))
    return clouds, poses


def random_rotation(rng):
    q = rng.normal(size=4)
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


GENERIC_ORIGIN = (0.1, -0.05, 0.3)


def generic_case(seed=1, n_clouds=4, n_points=300):
    """(clouds, poses, max_range): points on the faces of an 8 x 6 x 3 m room seen from n_clouds rigid poses inside it, in each pose's own
    frame; max_range is the 80th percentile of the ray lengths, so about a fifth of the rays are cut"""
    rng = np.random.default_rng(seed)
    size = np.array([8.0, 6.0, 3.0])
    clouds, poses, lengths = [], [], []
    for k in range(n_clouds):
        n = n_points + int(rng.integers(-20, 21))
        W = (rng.random((n, 3)) - 0.5) * size
        face = rng.integers(0, 6, n)
        W[np.arange(n), face % 3] = np.where(face < 3, -0.5, 0.5) * size[face % 3]
        W += np.array([0.3, -0.2, 1.5])
        R, t = random_rotation(rng), rng.uniform(-1.5, 1.5, 3) + np.array([0.3, -0.2, 1.5])
        clouds.append(((W - t) @ R).astype(F32))           # R^T (W - t)
        poses.append(np.concatenate([R.reshape(-1), t]))
        lengths.append(np.linalg.norm(W - (R @ np.array(GENERIC_ORIGIN) + t), axis=1))
    return clouds, poses, float(np.percentile(np.concatenate(lengths), 80))


def far_case():
    """two clouds of one point each whose poses lie 3000 m apart along the xy diagonal: 26 517 bricks per axis at resolution 0.01"""
    d = 3000.0 / math.sqrt(2.0)
    one = np.array([[1.0, 0.5, 0.25]], F32)
    return [one, one], [identity_pose(), identity_pose((d, d, 0.0))]
