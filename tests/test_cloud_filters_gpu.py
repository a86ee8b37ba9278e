"""The cloud filters of the legacy path on the GPU -- k_voxel_minmax / accumulate / flag / centroids, k_sor_mean_distance, k_kmeans_assign
and their host drivers -- at the edges of a wave, of a block and of their parameters (cases and references: tests/cloud_filter_cases.py).

Every case is held to oracle/np_filters.py bit for bit (index sets, counts, centroids, mean distances, labels, centres, compactness), as
tests/test_seg_gpu.py holds the one synthetic frame, and to a float64 reference that does not come from the oracle, within bars derived
from the number formats.  No test here feeds the library an out-of-range coordinate: that guard is host code and is tested in
tests/test_cloud_filters_cpu.py through sslam_debug_voxel_geometry."""
import ctypes as C

import numpy as np
import pytest

from oracle import np_filters as NF
from tests import cloud_filter_cases as CF
from tests import seg_params as SP

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def seg(gpu_lib):
    from semantic_slam_amd.segmentation import PointCloudSegmentation
    return PointCloudSegmentation()


def _refused(seg, code, call):
    from semantic_slam_amd.graph_slam import SslamError
    with pytest.raises(SslamError) as e:
        call()
    assert e.value.code == code, e.value.args


# ---- voxel grid -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CF.VOXEL_CASES)
def test_voxel_grid(seg, name):
    xyz, leaf = CF.voxel_case(name)
    cent, cnt = seg.downsamplePointcloud(xyz, leaf)
    co, no = NF.voxel_grid(xyz, leaf)
    print(f"{name}: {len(cnt)} voxels on the device, {len(no)} in the oracle")
    assert np.array_equal(cnt, no)
    assert np.array_equal(cent, co)
    worst = CF.check_voxel_against_reference(cent, cnt, xyz, leaf)      # counts, their sum, cell order, centroids within the bar
    print(f"{name}: worst centroid at {worst:.3f} of the bar")
    if name == "nonfinite:all":
        assert len(cnt) == 0
    if name == "one_voxel":
        assert cnt.tolist() == [len(xyz)]
    if name == "lattice":
        assert (cnt == 1).all() and len(cnt) == len(xyz)


@pytest.mark.parametrize("max_out", [0, 1, 100])
def test_voxel_grid_capacity(seg, max_out):
    """max_out below the number of occupied voxels, counts_out NULL as the tick passes it: the return value is the full count, the
    first max_out centroids are written and nothing after them"""
    xyz, leaf = CF.voxel_case(CF.CAPACITY_VOXEL_CASE)
    co, no = NF.voxel_grid(xyz, leaf)
    assert max_out < len(no)
    out = np.full((len(no) + 8, 3), -777.0, F)
    m = seg._lib.sslam_seg_voxel_grid(seg._h, xyz.ctypes.data, len(xyz), C.c_float(leaf), out.ctypes.data, None, max_out)
    assert m == len(no)
    assert np.array_equal(out[:max_out], co[:max_out]) and (out[max_out:] == -777.0).all()
    cnt = np.full(len(no) + 8, -777, np.int32)                   # and with counts
    out[:] = -777.0
    m = seg._lib.sslam_seg_voxel_grid(seg._h, xyz.ctypes.data, len(xyz), C.c_float(leaf), out.ctypes.data, cnt.ctypes.data, max_out)
    assert m == len(no) and np.array_equal(cnt[:max_out], no[:max_out]) and (cnt[max_out:] == -777).all()
    assert np.array_equal(out[:max_out], co[:max_out]) and (out[max_out:] == -777.0).all()


def test_voxel_grid_refuses_too_many_cells(seg):
    """ordinary coordinates, 501^3 cells: refused before anything is sized by the cell count; the handle works afterwards"""
    xyz, leaf = CF.TOO_MANY_CELLS
    _refused(seg, CF.SSLAM_ERR_UNSUPPORTED, lambda: seg.downsamplePointcloud(xyz, leaf))
    with pytest.raises(ValueError):
        NF.voxel_grid(xyz, leaf)
    cent, cnt = seg.downsamplePointcloud(xyz, 1.0)
    co, no = NF.voxel_grid(xyz, 1.0)
    assert np.array_equal(cnt, no) and np.array_equal(cent, co) and len(no) == 3


# ---- statistical outlier removal --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c for c in CF.SOR_CASES if c != "overflow"])
def test_outlier_removal(seg, name):
    xyz, k, mul = CF.sor_case(name)
    keep, md = seg.removeOutliers(xyz, k, mul)
    ko, mo = NF.statistical_outlier_removal(xyz, k, mul)
    worst = CF.check_sor_against_reference(md, xyz, k)
    print(f"{name}: {len(keep)} kept on the device, {len(ko)} in the oracle; worst mean distance {worst:.2f} x 2^-24 relative")
    assert np.array_equal(md, mo)
    assert np.array_equal(keep, ko)
    if name.startswith("duplicates"):
        assert len(keep) == len(xyz) and (md == 0).all()


def test_outlier_removal_overflowed_distances_are_infinite(seg):
    """38 ordinary points and two at +-3e19 with mean_k = 39: every point's k nearest include a squared distance past FLT_MAX, which is
    +inf in float32 and has to stand as +inf (a FLT_MAX sentinel would give sqrtf(FLT_MAX) = 1.8e19 instead); all 40 stay"""
    xyz, k, mul = CF.sor_case("overflow")
    keep, md = seg.removeOutliers(xyz, k, mul)
    ko, mo = NF.statistical_outlier_removal(xyz, k, mul)
    print("overflow: mean distances", md[:4], "...; kept", len(keep))
    assert np.isposinf(mo).all() and np.isposinf(md).all()
    assert np.array_equal(keep, ko) and np.array_equal(keep, np.arange(40))


def test_outlier_removal_refuses_too_few_finite_points(seg):
    """mean_k + 1 finite points among NaN rows pass (test_outlier_removal[nan_rows]); one fewer is SSLAM_ERR_INVALID, whatever n is, and
    the outputs stay untouched"""
    xyz, k, mul = CF.sor_too_few_finite()
    assert len(xyz) > k + 1
    keep = np.full(len(xyz), -777, np.int32); md = np.full(len(xyz), -777.0, F)
    rc = seg._lib.sslam_seg_statistical_outlier_removal(seg._h, xyz.ctypes.data, len(xyz), k, mul, keep.ctypes.data, len(xyz), md.ctypes.data)
    print("too few finite points: return value", rc, md[:4])
    assert rc == CF.SSLAM_ERR_INVALID
    assert (keep == -777).all() and (md == -777.0).all()
    _refused(seg, CF.SSLAM_ERR_INVALID, lambda: seg.removeOutliers(xyz, k, mul))
    with pytest.raises(ValueError):
        NF.statistical_outlier_removal(xyz, k, mul)


@pytest.mark.parametrize("max_out", [0, 1, 100])
def test_outlier_removal_capacity(seg, max_out):
    xyz, k, mul = CF.sor_case(CF.CAPACITY_SOR_CASE)
    ko, mo = NF.statistical_outlier_removal(xyz, k, mul)
    assert max_out < len(ko)
    keep = np.full(len(xyz), -777, np.int32)
    m = seg._lib.sslam_seg_statistical_outlier_removal(seg._h, xyz.ctypes.data, len(xyz), k, mul, keep.ctypes.data, max_out, None)
    assert m == len(ko)
    assert np.array_equal(keep[:max_out], ko[:max_out]) and (keep[max_out:] == -777).all()


# ---- k-means --------------------------------------------------------------------------------------------------------------------------
def _check_kmeans(seg, pts, k, seed):
    lab, cen, comp = seg.computeKmeans(pts, k, seed)
    lo, Co, compo = NF.kmeans(pts, k, seed)
    assert np.array_equal(lab, lo), f"k {k} seed {seed}: {(lab != lo).sum()} labels differ"
    assert np.array_equal(cen, Co) and comp == compo
    return lab, cen, CF.check_kmeans_against_reference(pts, lab, cen, k)


@pytest.mark.parametrize("dim", CF.KM_DIMS)
@pytest.mark.parametrize("n", CF.KM_SIZES)
def test_kmeans(seg, n, dim):
    pts = CF.kmeans_points(n, dim)
    for k in CF.KM_K:
        for seed in CF.KM_SEEDS:
            _check_kmeans(seg, pts, k, seed)


@pytest.mark.parametrize("name", CF.KM_SPECIAL)
def test_kmeans_empty_clusters_and_degenerate_boxes(seg, name):
    pts, k, want_empty = CF.kmeans_special(name)
    for seed in CF.KM_SEEDS:
        lab, cen, cnt = _check_kmeans(seg, pts, k, seed)
        empty = int((cnt == 0).sum())
        print(f"{name} seed {seed}: cluster sizes {cnt.tolist()}")
        if want_empty is not None:
            assert empty == want_empty
        if name == "five_points":
            assert empty >= 11
        if name == "identical":
            assert (lab == 0).all()


# ---- one handle for everything -----------------------------------------------------------------------------------------------------------
def test_one_handle_runs_all_three_filters_and_then_segments_a_frame(gpu_lib):
    from semantic_slam_amd.segmentation import PointCloudSegmentation
    h = PointCloudSegmentation(params=SP.make_params())
    xyz, leaf = CF.voxel_case("nonfinite:interleaved")
    cent, cnt = h.downsamplePointcloud(xyz, leaf)
    co, no = NF.voxel_grid(xyz, leaf)
    assert np.array_equal(cnt, no) and np.array_equal(cent, co)
    pts, k, mul = CF.sor_case("size:50@257@1.0")
    keep, md = h.removeOutliers(pts, k, mul)
    ko, mo = NF.statistical_outlier_removal(pts, k, mul)
    assert np.array_equal(keep, ko) and np.array_equal(md, mo)
    _check_kmeans(h, CF.kmeans_points(257, 3), 4, 0)
    SP.check_frames(h, [dict(seed=1, n_boxes=12)], {}, batched=True)
    cent, cnt = h.downsamplePointcloud(xyz, leaf)                 # and the filters after a frame
    assert np.array_equal(cnt, no) and np.array_equal(cent, co)
