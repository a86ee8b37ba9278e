"""Restatement of sslam_seg_occupancy_map_scans, written from its contract in include/sslam.h: OctoMap's per-scan update over the rays of
tests/occupancy_ref.py.  Shares no code with the library; the rays, the cut, the walk, the parameters and the cases come from occupancy_ref.

The contract: a scan is one cloud; scans are applied in the order given.  Per scan H = the last cells of its rays that were not cut, M = every
other cell its walks visit (the last cell of a cut ray included) minus H.  Every cell of H or M gets one update,
lo = fmin(fmax(float32(lo + l), l_min), l_max) from lo = 0, l = l_hit for H and l_miss for M.  hits / misses count the scans with the cell in
H / M; the log-odds are lo after the last scan; n_steps is the number of (scan, cell) updates.

Two implementations: scan_ref (Python sets and dicts, one cloud and one ray at a time: the restatement the tests compare with) and
scan_ref_vec (per cloud the unique cell keys by np.unique over a vectorised walk, then the ordered update over dense tables; the cpu test
holds the two equal, and tools/occupancy_timing.py --scans uses it for its millions of rays)."""
import numpy as np

import occupancy_ref as OR

F32 = np.float32
_COUNTERS = ("n_points", "n_rays", "n_truncated", "n_clipped_z")


def scan_sets(cloud, T, P):
    """one scan -> (H, V, counters): the last cells of its uncut rays; every cell visited as anything else (V - H is the contract's M)"""
    rays, st = OR.rays_of([cloud], [T], P)
    H, V = set(), set()
    for Qo, Qe, tr in rays:
        path = OR.walk(Qo, Qe)
        V.update(path[:-1])
        (V if tr else H).add(path[-1])
    return H, V, st


def update(lo, l, P):
    t = F32(lo) + F32(l)
    assert t.dtype == F32
    return np.fmin(np.fmax(t, P["l_min"]), P["l_max"])


def _ordered(cells, hits, misses, lo, P, st):
    """the records in the order of occupancy_ref._records, with the sequential log-odds in place of its clamp of the sum, then `emit`"""
    n = len(cells)
    oc, perm, _, _, rs = OR._records(cells, np.arange(n, dtype=np.int64), np.zeros(n, np.int64), dict(P, emit=0), st)
    perm = perm.astype(np.int64)
    hits, misses, lo = hits[perm], misses[perm], lo[perm].astype(F32)
    st = dict(rs, n_steps=int(hits.sum() + misses.sum()))
    keep = np.ones(n, bool) if P["emit"] == 0 else (lo >= P["l_occ"]) if P["emit"] == 1 else (lo < P["l_occ"])
    return oc[keep], hits[keep].astype(np.int32), misses[keep].astype(np.int32), lo[keep], st


def scan_ref(clouds, poses, P):
    """-> (cells [m, 3] int32, hits [m] int32, misses [m] int32, logodds [m] float32, stats dict), as occupancy_ref; raises OR.Unsupported"""
    st = dict(n_clouds=len(clouds), **{k: 0 for k in _COUNTERS})
    table = {}                                             # cell -> [hits, misses, lo]
    for c, T in zip(clouds, poses):
        H, V, one = scan_sets(c, T, P)
        for k in _COUNTERS:
            st[k] += one[k]
        for cells, col, l in ((H, 0, P["l_hit"]), (V - H, 1, P["l_miss"])):
            for cell in cells:
                e = table.setdefault(cell, [0, 0, F32(0.0)])
                e[col] += 1
                e[2] = update(e[2], l, P)
    cells = np.array(sorted(table), np.int64).reshape(-1, 3)
    rows = [table[tuple(c)] for c in cells.tolist()]
    hits = np.array([r[0] for r in rows], np.int64)
    misses = np.array([r[1] for r in rows], np.int64)
    lo = np.array([r[2] for r in rows], F32)
    return _ordered(cells, hits, misses, lo, P, st)


# ---- the second formulation: unique keys per cloud, dense tables ------------------------------------------------------------------------
def _cloud_cells_vec(c, T, P, st):
    """one cloud -> (cells [k, 3] int64, is_hit [k] bool), every visited cell once; None when no ray takes part"""
    inv = F32(1.0) / P["resolution"]
    R = OR.range_units(P)
    c = np.ascontiguousarray(c, F32).reshape(-1, 3)
    st["n_points"] += len(c)
    o, o_ok = OR.transform(P["sensor_origin"].reshape(1, 3), T)
    if not o_ok[0] or len(c) == 0:
        return None
    t, ok = OR.transform(c, T)
    t = t[ok]
    inz = (t[:, 2] >= P["z_min"]) & (t[:, 2] <= P["z_max"])
    st["n_clipped_z"] += int((~inz).sum())
    t = t[inz]
    if len(t) == 0:
        return None
    Qe = OR._positions_vec(t, inv)
    Qo = np.broadcast_to(OR._positions_vec(o, inv), Qe.shape).copy()
    D = Qe - Qo
    len2 = (D * D).sum(1)
    tr = len2 > R * R
    L = np.floor(np.sqrt(len2.astype(np.float64))).astype(np.int64)            # floor of the root, the double corrected in integers ...
    L -= L * L > len2
    L += (L + 1) * (L + 1) <= len2
    L += L * L < len2                                                          # ... then the smallest L with L^2 >= len2
    Dc = np.sign(D) * (np.abs(D) * R // np.maximum(L, 1)[:, None])
    D = np.where(tr[:, None], Dc, D)
    Qe = Qo + D
    st["n_rays"] += len(D)
    st["n_truncated"] += int(tr.sum())
    cell, ce = Qo >> 10, Qe >> 10
    left = np.abs(ce - cell)
    num = np.where(D > 0, 1024 - (Qo & 1023), Qo & 1023)
    aD, step = np.abs(D), np.sign(D)
    seen, flag = [], []
    while len(cell):
        done = left.sum(1) == 0
        seen.append(cell.copy()); flag.append(done & ~tr)
        go = ~done
        cell, left, num, aD, step, tr = cell[go], left[go], num[go], aD[go], step[go], tr[go]
        if not len(cell):
            break
        # the axis with steps left whose next face comes first; ties to the lower axis: compare the fractions num / aD by cross-multiplication
        best = np.full(len(cell), -1)
        for a in range(3):
            b = np.maximum(best, 0)
            r = np.arange(len(cell))
            better = (left[:, a] > 0) & ((best < 0) | (num[:, a] * aD[r, b] < num[r, b] * aD[:, a]))
            best = np.where(better, a, best)
        r = np.arange(len(cell))
        cell[r, best] += step[r, best]; num[r, best] += 1024; left[r, best] -= 1
    seen, flag = np.concatenate(seen), np.concatenate(flag)
    lo3 = seen.min(0)
    ext = seen.max(0) - lo3 + 1
    key = ((seen[:, 2] - lo3[2]) * ext[1] + (seen[:, 1] - lo3[1])) * ext[0] + (seen[:, 0] - lo3[0])
    hit_keys = np.unique(key[flag])
    miss_keys = np.setdiff1d(np.unique(key), hit_keys)
    keys = np.concatenate([hit_keys, miss_keys])
    cells = np.stack([keys % ext[0] + lo3[0], keys // ext[0] % ext[1] + lo3[1], keys // (ext[0] * ext[1]) + lo3[2]], 1)
    return cells, np.arange(len(keys)) < len(hit_keys)


def scan_ref_vec(clouds, poses, P):
    st = dict(n_clouds=len(clouds), **{k: 0 for k in _COUNTERS})
    scans = [s for s in (_cloud_cells_vec(c, T, P, st) for c, T in zip(clouds, poses)) if s is not None]
    if not scans:
        z = np.zeros(0, np.int64)
        return _ordered(z.reshape(0, 3), z, z, z.astype(F32), P, st)
    lo3 = np.min([s[0].min(0) for s in scans], 0)
    ext = np.max([s[0].max(0) for s in scans], 0) - lo3 + 1
    size = int(ext[0]) * int(ext[1]) * int(ext[2])
    assert size <= 1 << 29, "the box of the cells is too large for the dense tables"
    hits_d, misses_d, lo_d = np.zeros(size, np.int32), np.zeros(size, np.int32), np.zeros(size, F32)
    for cells, is_hit in scans:
        key = ((cells[:, 2] - lo3[2]) * ext[1] + (cells[:, 1] - lo3[1])) * ext[0] + (cells[:, 0] - lo3[0])   # unique inside a scan
        hits_d[key[is_hit]] += 1
        misses_d[key[~is_hit]] += 1
        t = lo_d[key] + np.where(is_hit, P["l_hit"], P["l_miss"]).astype(F32)
        assert t.dtype == F32
        lo_d[key] = np.fmin(np.fmax(t, P["l_min"]), P["l_max"])
    keys = np.flatnonzero(hits_d | misses_d)
    cells = np.stack([keys % ext[0] + lo3[0], keys // ext[0] % ext[1] + lo3[1], keys // (ext[0] * ext[1]) + lo3[2]], 1)
    return _ordered(cells, hits_d[keys].astype(np.int64), misses_d[keys].astype(np.int64), lo_d[keys], P, st)


# ---- the case in which the order of the scans matters -----------------------------------------------------------------------------------
def moved_params(**kw):
    return OR.default_params(resolution=0.1, **kw)


def moved_case(n_clouds=130, n_first=70, seed=7):
    """(clouds, poses): an object that has gone.  Every cloud has a pose with a yaw in +-0.2 rad and a translation of (+-0.1, +-0.3,
    0.5 +- 0.05); the sensor sits at the pose.  16 rays go through a 4 x 4 grid (jitter +-0.04) on the patch y in [-0.45, 0.45],
    z in [0.15, 0.85] of the plane x = 2, 8 rays go to the wall x = 4 beside it.  The first n_first clouds end their 16 rays on the patch;
    the later ones end them on the wall along the same directions.  With clamp-of-sum the patch stays occupied for ever (70 hits against
    60 misses); with OctoMap's clamp after every update it is free after a dozen scans."""
    rng = np.random.default_rng(seed)
    gy = -0.45 + 0.9 * (np.arange(4) + 0.5) / 4
    gz = 0.15 + 0.7 * (np.arange(4) + 0.5) / 4
    clouds, poses = [], []
    for k in range(n_clouds):
        yaw = rng.uniform(-0.2, 0.2)
        t = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.3, 0.3), 0.5 + rng.uniform(-0.05, 0.05)])
        R = np.array([[np.cos(yaw), -np.sin(yaw), 0.0], [np.sin(yaw), np.cos(yaw), 0.0], [0.0, 0.0, 1.0]])
        Y, Z = np.meshgrid(gy, gz, indexing="ij")
        patch = np.stack([np.full(16, 2.0), Y.reshape(-1) + rng.uniform(-0.04, 0.04, 16), Z.reshape(-1) + rng.uniform(-0.04, 0.04, 16)], 1)
        if k >= n_first:                                   # the object has gone: the same directions, on to the wall
            patch = t + (patch - t) * ((4.0 - t[0]) / (patch[:, 0] - t[0]))[:, None]
        side = np.where(np.arange(8) % 2 == 0, 1.0, -1.0)
        wall = np.stack([np.full(8, 4.0), side * rng.uniform(1.2, 2.0, 8), rng.uniform(0.15, 0.85, 8)], 1)
        W = np.concatenate([patch, wall])
        clouds.append(((W - t) @ R).astype(F32))           # R^T (W - t)
        poses.append(np.concatenate([R.reshape(-1), t]))
    return clouds, poses
