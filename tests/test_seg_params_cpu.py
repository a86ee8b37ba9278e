"""The inputs of the segmentation parameter sweep (tests/seg_params.py) make every parameter bite: oracle alone, no GPU.

test_seg_params_gpu.py holds the HIP frontend to the oracle at non-default parameters and with full 64-entry tables.  That says
something only while the non-default run differs from the default one and the tables really fill; a later edit of synth.py could
silently turn either into a no-op.  These tests pin that down on the oracle's own output."""
import numpy as np
import pytest

from tests import seg_params as SP


def _changed_normals(a, b):
    both_nan = np.isnan(a) & np.isnan(b)
    return int(((a != b) & ~both_nan).any(1).sum())


@pytest.mark.parametrize("case", list(SP.ALL_CASES))
def test_case_differs_from_the_default_run(case):
    over = SP.ALL_CASES[case]
    _, nrm0, lab0 = SP.oracle_run(SP.LDS_FRAME, {})
    planes, nrm, lab = SP.oracle_run(SP.LDS_FRAME, over)
    px = int((lab != lab0).sum())
    npx = _changed_normals(nrm, nrm0)
    print(f"{case}: {len(planes)} planes, {px} label pixels and {npx} normals differ from the default run")
    if set(over) == {"max_depth_change_factor"}:
        # the factor moves few labels (31 and 6 pixels) but thousands of normals, through the distance map that sizes the smoothing window
        assert npx >= 1000
    else:
        assert px >= 100
    if case == "combined":
        assert npx >= 1000 and len(planes) >= 1


def test_every_parameter_has_a_case_with_planes():
    with_planes = {param for name, (param, over) in SP.KERNEL_CASES.items() if len(SP.oracle_run(SP.LDS_FRAME, over)[0]) >= 1}
    assert with_planes == {"max_depth_change_factor", "angular_threshold", "distance_threshold", "maximum_curvature", "num_point_seg"}
    assert len(SP.oracle_run(SP.LDS_FRAME, {})[0]) >= 2          # the host-filter cases drop one plane and keep another
    assert len(SP.oracle_run(SP.HBM_FRAME, SP.COMBINED)[0]) >= 1
    for s in SP.MANY_BOX_SEEDS:
        assert 1 <= len(SP.oracle_run(dict(seed=s, n_boxes=32), SP.COMBINED)[0]) < 512


def test_host_filter_thresholds_sit_on_a_plane():
    """min_contour_points is a strict '>' on the contour length, planar_area a '>=' in double, norm_point_thres an 'n < thres'"""
    ref = SP.oracle_run(SP.LDS_FRAME, {})[0]
    p = ref[1]
    rest = [(q.box_index, q.inlier_count) for q in ref if q is not p]
    ids = lambda planes: [(q.box_index, q.inlier_count) for q in planes]
    assert p.num_points == int(p.num_points) and len({q.num_points for q in ref}) == len(ref) and len({q.area for q in ref}) == len(ref)
    assert ids(SP.oracle_run(SP.LDS_FRAME, dict(min_contour_points=int(p.num_points)))[0]) == rest
    assert ids(SP.oracle_run(SP.LDS_FRAME, dict(min_contour_points=int(p.num_points) - 1))[0]) == ids(ref)
    area = sorted(q.area for q in ref)[1]                         # one plane below it, one on it, the rest above
    above = float(np.nextafter(np.float32(area), np.float32(np.inf)))
    assert ids(SP.oracle_run(SP.LDS_FRAME, dict(planar_area=float(area)))[0]) == ids([q for q in ref if q.area >= area])
    assert ids(SP.oracle_run(SP.LDS_FRAME, dict(planar_area=above))[0]) == ids([q for q in ref if q.area > area])
    assert ids(SP.oracle_run(SP.LDS_FRAME, dict(norm_point_thres=12288))[0]) == ids(ref)
    assert SP.oracle_run(SP.LDS_FRAME, dict(norm_point_thres=12289))[0] == []


def test_reference_quirks_shows_in_the_world_pose_of_a_tilted_robot():
    tilted = dict(SP.LDS_FRAME, rpy=SP.TILTED_POSE)
    q1 = SP.oracle_run(tilted, dict(reference_quirks=1))[0]
    q0 = SP.oracle_run(tilted, dict(reference_quirks=0))[0]
    assert len(q0) == len(q1) >= 1
    for a, b in zip(q0, q1):
        assert list(a.world_pose) != list(b.world_pose)
    # with roll = pitch = 0, as make_frame leaves them, the quirk is invisible
    f0 = SP.oracle_run(SP.LDS_FRAME, dict(reference_quirks=0))[0]
    f1 = SP.oracle_run(SP.LDS_FRAME, dict(reference_quirks=1))[0]
    assert [list(a.world_pose) for a in f0] == [list(a.world_pose) for a in f1]


@pytest.mark.parametrize("box_w,box_h,cands", [(128, 96, (93, 1, 95, 2, 1, 70)), (168, 100, (110, 1, 145, 3, 2, 112))])
def test_full_table_frames_fill_the_tables(box_w, box_h, cands):
    """num_point_seg = 5 on the noisy frame: three boxes have more than 64 candidate components, the oracle accepts exactly 64 regions
    in each (maximum_curvature = 1.0 accepts every candidate), and without post-filters all of them become planes"""
    fk = SP.full_table_frame(box_w, box_h)
    per_box = SP.candidates_per_box(fk, SP.FULL_TABLE)
    assert tuple(c for c, _ in per_box) == cands
    assert tuple(r for _, r in per_box) == tuple(min(c, 64) for c in cands)
    assert sum(c > 64 for c in cands) == 3
    assert 1 <= len(SP.oracle_run(fk, SP.FULL_TABLE)[0]) < 512
    planes = SP.oracle_run(fk, {**SP.FULL_TABLE, **SP.NO_POST_FILTER})[0]
    assert 3 * 64 - 32 <= len(planes) < 512                       # a few regions have no boundary or face neither way
    lab = SP.oracle_run(fk, SP.FULL_TABLE)[2]
    assert lab.max() == 63                                         # label code 63 is in the images the refinement kernels sweep


def test_curvature_gated_case_overflows_without_filling_the_region_table():
    per_box = SP.candidates_per_box(SP.full_table_frame(168, 100), SP.CURVATURE_GATED)
    assert sum(c > 64 for c, _ in per_box) == 1 and (76, 31) in per_box


def test_full_table_frames_of_the_many_box_call_stay_below_the_oracle_limit():
    full = 0
    for s in SP.FULL_TABLE_MANY_SEEDS:
        fk = SP.full_table_frame(128, 96, seed=s, n_boxes=32)
        assert len(SP.oracle_run(fk, SP.FULL_TABLE)[0]) < 512
        full += sum(c > 64 for c, _ in SP.candidates_per_box(fk, SP.FULL_TABLE))
    assert full >= 9                                               # a full candidate table per frame on average
