"""The inputs of the cloud-filter tests (tests/cloud_filter_cases.py) do what they claim, the oracle holds the bars the GPU file sets, and
the voxel geometry guard refuses what it must: oracle and host code alone, no GPU.

tests/test_cloud_filters_gpu.py holds the kernels to oracle/np_filters.py bit for bit and to float64 references within derived bars.
That says something only while the face lattices really separate the float32 product rule from its neighbours, the sparse grid is
sparse, the k-means cases really empty their clusters, and the oracle itself is inside the bars.  The guard of the voxel index
(sslam_debug_voxel_geometry, the driver's own rule) is host code, so out-of-range coordinates are tested here and never fed to a kernel."""
import ctypes as C

import numpy as np
import pytest

from oracle import np_filters as NF
from tests import cloud_filter_cases as CF

F = np.float32


# ---- the cases bite -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaf", CF.FACE_LEAVES)
def test_face_lattice_separates_the_product_rule(leaf):
    """lattice values (of k = -400 .. 400) whose cell under floor(float32(x) * float32(1 / leaf)) differs from the cell under
    floor(float64(x) / leaf) and under float32 division.  Leaves 0.1 and 0.04 are not binary fractions: hundreds of values differ
    (267 / 0 and 299 / 82 measured).  Leaf 0.125 is exact in binary: it is the control on which all three rules give cell k."""
    v = CF.face_lattice(leaf)[:len(CF.FACE_K)]
    prod = np.floor((v * (F(1.0) / F(leaf))).astype(F)).astype(np.int64)
    dbl = np.floor(v.astype(np.float64) / leaf).astype(np.int64)
    div32 = np.floor((v / F(leaf)).astype(F)).astype(np.int64)
    n_dbl, n_div = int((prod != dbl).sum()), int((prod != div32).sum())
    print(f"leaf {leaf}: {n_dbl} of {len(v)} cells differ from float64 division, {n_div} from float32 division")
    if leaf == 0.125:
        assert n_dbl == 0 and n_div == 0 and np.array_equal(prod, CF.FACE_K)
    else:
        assert n_dbl >= 50
    if leaf == 0.04:
        assert n_div >= 50
    for axis in range(3):
        xyz, lf = CF.voxel_case(f"face:{leaf}@{axis}")
        assert lf == leaf and set(v.tolist()) <= set(xyz[:, axis].tolist())
        z = xyz[xyz[:, axis] == 0, axis]
        assert np.signbit(z).any() and not np.signbit(z).all()          # -0.0 and 0.0 both present
        _, div = CF.voxel_geometry(xyz, leaf)
        assert div[axis] >= 800 and int(np.prod(div)) <= 802 * 25


def test_sparse_grids_are_sparse():
    xyz, leaf = CF.voxel_case("sparse")
    _, div = CF.voxel_geometry(xyz, leaf)
    ncell = int(np.prod(div))
    _, cnt = CF.voxel_reference(xyz, leaf)
    print(f"sparse: div {div.tolist()}, {ncell} cells, {len(cnt)} occupied")
    assert CF.SPARSE_NCELL[0] < ncell < CF.SPARSE_NCELL[1] and 2 <= len(cnt) < CF.SPARSE_MAX_OCCUPIED
    xyz, leaf = CF.voxel_case("sparse_flat")
    _, div = CF.voxel_geometry(xyz, leaf)
    assert int(div[0] * div[1]) > 65536 and len(CF.voxel_reference(xyz, leaf)[1]) < CF.SPARSE_MAX_OCCUPIED


def test_voxel_cases_have_the_shape_they_claim():
    xyz, leaf = CF.voxel_case("one_voxel")
    assert len(xyz) == 60000 and len(CF.voxel_reference(xyz, leaf)[1]) == 1
    xyz, leaf = CF.voxel_case("lattice")
    _, cnt = CF.voxel_reference(xyz, leaf)
    assert len(cnt) == len(xyz) == 16 * 12 * 7 and (cnt == 1).all() and np.array_equal(CF.voxel_geometry(xyz, leaf)[1], [16, 12, 7])
    xyz, leaf = CF.voxel_case("negative")
    assert (xyz < 0).all()
    assert len(CF.voxel_case(f"size:{CF.VOXEL_BIG}@0.1")[0]) > 256 * 256
    fin = np.isfinite(CF.voxel_case("nonfinite:wave")[0]).all(1)
    assert not fin[64:128].any() and fin[:64].all() and fin[128:].all()
    fin = np.isfinite(CF.voxel_case("nonfinite:block")[0]).all(1)
    assert not fin[256:512].any() and fin[:256].all() and fin[512:].all()
    assert not np.isfinite(CF.voxel_case("nonfinite:first_block")[0]).all(1)[:256].any()
    assert not np.isfinite(CF.voxel_case("nonfinite:all")[0]).all(1).any()
    p = CF.voxel_case("nonfinite:interleaved")[0]
    assert np.isnan(p).any() and (p == np.inf).any() and (p == -np.inf).any() and 200 < np.isfinite(p).all(1).sum() < 400
    for n in CF.VOXEL_SIZES:              # the last point of every size case owns a voxel and moves the bounding box
        xyz, leaf = CF.voxel_case(f"size:{n}@0.1")
        assert len(xyz) == n and (n == 1 or (xyz[-1] > xyz[:-1].max(0)).all())


@pytest.mark.parametrize("name", CF.KM_SPECIAL)
@pytest.mark.parametrize("seed", CF.KM_SEEDS)
def test_kmeans_cases_empty_their_clusters_in_the_winning_attempt(name, seed):
    pts, k, want_empty = CF.kmeans_special(name)
    lab, cen, _ = NF.kmeans(pts, k, seed)
    empty = k - len(np.unique(lab))
    if name == "five_points":
        assert empty >= 11
    elif want_empty is not None:
        assert empty == want_empty, (name, seed, np.bincount(lab, minlength=k))
    if name == "identical":
        assert (lab == 0).all()
    if name == "constant_coordinate":
        assert (pts[:, 1] == pts[0, 1]).all() and (cen[:, 1] == pts[0, 1]).all()


# ---- the oracle against the float64 references ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CF.VOXEL_CASES)
def test_oracle_voxel_grid_within_the_bar(name):
    xyz, leaf = CF.voxel_case(name)
    cent, cnt = NF.voxel_grid(xyz, leaf)
    worst = CF.check_voxel_against_reference(cent, cnt, xyz, leaf)
    print(f"{name}: {len(cnt)} voxels, worst centroid at {worst:.3f} of the bar")
    if name == "nonfinite:all":
        assert len(cnt) == 0


@pytest.mark.parametrize("name", [c for c in CF.SOR_CASES if c != "overflow"])
def test_oracle_outlier_removal_within_the_bar(name):
    xyz, k, mul = CF.sor_case(name)
    keep, md = NF.statistical_outlier_removal(xyz, k, mul)
    worst = CF.check_sor_against_reference(md, xyz, k)
    print(f"{name}: {len(keep)} of {len(xyz)} kept, worst mean distance {worst:.2f} x 2^-24 relative")
    fin = np.isfinite(xyz).all(1)
    assert set(keep.tolist()) <= set(np.flatnonzero(fin).tolist())
    if name.startswith("duplicates"):
        assert len(keep) == len(xyz) and (md == 0).all()
    if name == "nan_rows":
        assert fin.sum() == k + 1
    if name.startswith("size") and mul > 0 and len(xyz) >= 127:
        assert len(xyz) - 1 not in keep and 0 < len(keep) < len(xyz)      # the last point is a stray


def test_oracle_outlier_removal_overflow_and_refusal():
    """two points at +-3e19: every point has a neighbour whose squared distance is past FLT_MAX (the float64 one is 9e38 or more), so the
    float32 pipeline must carry +inf into every mean; the threshold is NaN and all 40 stay.  One finite point too few is refused."""
    xyz, k, mul = CF.sor_case("overflow")
    q = xyz.astype(np.float64)
    d2 = ((q[:, None] - q[None]) ** 2).sum(2)
    assert (np.sort(d2, axis=1)[:, k] > float(np.finfo(F).max)).all()
    keep, md = NF.statistical_outlier_removal(xyz, k, mul)
    assert np.isposinf(md).all() and np.array_equal(keep, np.arange(40))
    xyz, k, mul = CF.sor_too_few_finite()
    with pytest.raises(ValueError):
        NF.statistical_outlier_removal(xyz, k, mul)


@pytest.mark.parametrize("dim", CF.KM_DIMS)
@pytest.mark.parametrize("n", CF.KM_SIZES)
def test_oracle_kmeans_within_the_bar(n, dim):
    pts = CF.kmeans_points(n, dim)
    for k in CF.KM_K:
        for seed in CF.KM_SEEDS:
            lab, cen, comp = NF.kmeans(pts, k, seed)
            assert lab.min() >= 0 and lab.max() < k and cen.shape == (k, dim) and comp >= 0
            CF.check_kmeans_against_reference(pts, lab, cen, k)


@pytest.mark.parametrize("name", CF.KM_SPECIAL)
def test_oracle_kmeans_special_cases_within_the_bar(name):
    pts, k, _ = CF.kmeans_special(name)
    for seed in CF.KM_SEEDS:
        lab, cen, _ = NF.kmeans(pts, k, seed)
        CF.check_kmeans_against_reference(pts, lab, cen, k)


# ---- sslam_debug_voxel_geometry: the driver's rule, on the host ------------------------------------------------------------------------------
def _geometry(lib, lo, hi, leaf):
    lo = np.ascontiguousarray(lo, F); hi = np.ascontiguousarray(hi, F)
    minb = np.full(3, 123456789, np.int32); div = np.full(3, -987654321, np.int64)
    rc = lib.sslam_debug_voxel_geometry(lo.ctypes.data, hi.ctypes.data, C.c_float(leaf), minb.ctypes.data, div.ctypes.data)
    if rc:
        assert (minb == 123456789).all() and (div == -987654321).all(), "outputs written on an error"
    return rc, minb, div


@pytest.mark.parametrize("name", [c for c in CF.VOXEL_CASES if c != "nonfinite:all"])
def test_voxel_geometry_equals_the_oracle(hip_lib, name):
    xyz, leaf = CF.voxel_case(name)
    q = xyz[np.isfinite(xyz).all(1)]
    rc, minb, div = _geometry(hip_lib, q.min(0), q.max(0), leaf)
    _, ominb, odiv = NF.voxel_geometry(q.min(0), q.max(0), leaf)
    assert rc == 0 and np.array_equal(minb, ominb) and np.array_equal(div, odiv)
    kminb, kdiv = CF.voxel_geometry(xyz, leaf)             # and both equal the extent of the per-point keys
    assert np.array_equal(minb, kminb) and np.array_equal(div, kdiv)


REFUSED = {
    "lo -1e10": ((-1e10, 0, 0), (0, 0, 0), 0.1),
    "lo = hi = -1e10": ((0, -1e10, 0), (0, -1e10, 0), 0.1),
    "hi 1e10 alone": ((0, 0, 1e10), (0, 0, 1e10), 0.1),
    "hi 1e10, small lo": ((-1, -1, -1), (1, 1e10, 1), 0.1),
    "lo -1e10, hi 1e10": ((-1e10, 0, 0), (1e10, 0, 0), 0.1),
    "hi 2.2e8 at leaf 0.1": ((0, 0, 0), (2.2e8, 0, 0), 0.1),
    "hi 2^31 at leaf 1": ((0, 0, 0), (2.0 ** 31, 0, 0), 1.0),
    "lo below -2^31 at leaf 1": ((-2.0 ** 31 - 256, 0, 0), (-2.0 ** 31, 0, 0), 1.0),
    "FLT_MAX": ((0, 0, 0), (3.4e38, 0, 0), 0.1),
    "leaf 1e-45": ((0, 0, 0), (1, 1, 1), 1e-45),
    "2^26 + 1 cells in a row": ((0, 0, 0), (2.0 ** 26, 0, 0), 1.0),
    "2^26 + 1 cells, 5 x 13421773": ((0, 0, 0), (4, 13421772, 0), 1.0),
    "2^32 x 2^32 x 2^32 would wrap": ((-2.0 ** 31, -2.0 ** 31, -2.0 ** 31), (2.0 ** 31 - 128, 2.0 ** 31 - 128, 2.0 ** 31 - 128), 1.0),
    "501^3 cells": ((0, 0, 0), (50, 50, 50), 0.1),
    "upper below lower": ((1, 0, 0), (0, 0, 0), 0.1),
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_voxel_geometry_refuses(hip_lib, what):
    lo, hi, leaf = REFUSED[what]
    rc, _, _ = _geometry(hip_lib, lo, hi, leaf)
    assert rc == CF.SSLAM_ERR_UNSUPPORTED, hip_lib.sslam_last_error().decode()
    with pytest.raises(ValueError):
        NF.voxel_geometry(np.array(lo, F), np.array(hi, F), leaf)


def test_voxel_geometry_accepts_the_last_valid_grids(hip_lib):
    rc, minb, div = _geometry(hip_lib, (0, 0, 0), (511, 511, 255), 1.0)                     # exactly 2^26 cells
    assert rc == 0 and np.array_equal(div, [512, 512, 256]) and np.array_equal(minb, [0, 0, 0])
    rc, minb, div = _geometry(hip_lib, (-2.0 ** 31, 0, 0), (-2.0 ** 31 + 256, 0, 0), 1.0)   # floor(lo * inv) = -2^31 fits
    assert rc == 0 and minb[0] == -2 ** 31 and np.array_equal(div, [257, 1, 1])
    rc, minb, div = _geometry(hip_lib, (2.0 ** 31 - 384, 0, 0), (2.0 ** 31 - 128, 0, 0), 1.0)   # the largest float below 2^31
    assert rc == 0 and minb[0] == 2 ** 31 - 384 and np.array_equal(div, [257, 1, 1])
    for lo, hi, leaf in (((0, 0, 0), (511, 511, 255), 1.0), ((-2.0 ** 31, 0, 0), (-2.0 ** 31 + 256, 0, 0), 1.0)):
        _, ominb, odiv = NF.voxel_geometry(np.array(lo, F), np.array(hi, F), leaf)
        rc, minb, div = _geometry(hip_lib, lo, hi, leaf)
        assert np.array_equal(minb, ominb) and np.array_equal(div, odiv)
    # a leaf that is not positive, or a missing array, is a bad argument, not an unsupported grid
    assert _geometry(hip_lib, (0, 0, 0), (1, 1, 1), 0.0)[0] == CF.SSLAM_ERR_INVALID
    assert _geometry(hip_lib, (0, 0, 0), (1, 1, 1), float("nan"))[0] == CF.SSLAM_ERR_INVALID
    assert hip_lib.sslam_debug_voxel_geometry(None, None, C.c_float(0.1), None, None) == CF.SSLAM_ERR_INVALID
