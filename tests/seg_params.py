"""Case tables and the comparison helper of the segmentation parameter sweep (test_seg_params_cpu.py, test_seg_params_gpu.py).

The frontend is compared bit for bit with oracle/oracle_seg.c.  The tables here move every field of ``sslam_seg_params`` that the
kernels read from their ``View`` (and the host post-filters of ``seg_finish``) away from its default, on frames where the CPU test
shows that the move changes the result.  Oracle runs are cached per (frame, params): a reference is computed once and shared."""
import dataclasses
import functools

import numpy as np

from semantic_slam_amd.synth import make_frame

# ---- frames ---------------------------------------------------------------------------------------------------------------------
LDS_FRAME = dict(seed=0)                                        # 32 boxes of 128 x 96: connected components and refinement out of LDS
HBM_FRAME = dict(seed=5, n_boxes=12, box_w=168, box_h=100)      # 16800 px per box: above the LDS limit, the HBM forms
MANY_BOX_SEEDS = tuple(range(40, 49))                           # nine 32-box frames = 288 boxes in one call: k_regions<256>
TILTED_POSE = (0.05, -0.1, 2.1)                                 # roll, pitch, yaw: reference_quirks only shows with roll != pitch


def full_table_frame(box_w, box_h, seed=5, n_boxes=6):
    """noisy frame on which num_point_seg = 5 leaves more than 64 candidate components in some boxes"""
    return dict(seed=seed, n_boxes=n_boxes, box_w=box_w, box_h=box_h, noise=4e-3)


FULL_TABLE = dict(num_point_seg=5, maximum_curvature=1.0)       # curvature is at most 1/3: every candidate is accepted
NO_POST_FILTER = dict(min_contour_points=0, planar_area=0.0)    # every region reaches k_contour / k_area's output
CURVATURE_GATED = dict(num_point_seg=10, maximum_curvature=0.02)
FULL_TABLE_MANY_SEEDS = tuple(range(5, 14))                     # nine 32-box frames of full_table_frame(128, 96)

# ---- parameter cases ------------------------------------------------------------------------------------------------------------
# name -> (the parameter the case is about, overrides)
KERNEL_CASES = {
    "mdcf_0.01": ("max_depth_change_factor", dict(max_depth_change_factor=0.01)),
    "mdcf_0.1": ("max_depth_change_factor", dict(max_depth_change_factor=0.1)),
    "angular_0.01": ("angular_threshold", dict(angular_threshold=0.01)),
    "angular_0.1": ("angular_threshold", dict(angular_threshold=0.1)),
    "distance_0.005": ("distance_threshold", dict(distance_threshold=0.005)),
    "distance_0.05": ("distance_threshold", dict(distance_threshold=0.05)),
    "curvature_0.0005": ("maximum_curvature", dict(maximum_curvature=0.0005)),
    "curvature_0.01": ("maximum_curvature", dict(maximum_curvature=0.01)),
    "num_point_seg_50": ("num_point_seg", dict(num_point_seg=50)),
    "num_point_seg_1500": ("num_point_seg", dict(num_point_seg=1500)),
}
COMBINED = dict(max_depth_change_factor=0.05, angular_threshold=0.02, distance_threshold=0.01, maximum_curvature=0.005, num_point_seg=100)
ALL_CASES = {**{k: v[1] for k, v in KERNEL_CASES.items()}, "combined": COMBINED}


def make_params(**over):
    from semantic_slam_amd.segmentation import default_params
    p = default_params()
    for k, v in over.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def _key(d):
    return tuple(sorted(d.items()))


@functools.lru_cache(maxsize=None)
def _frame(key):
    kw = dict(key)
    pose = kw.pop("rpy", None)
    f = make_frame(**kw)
    if pose is not None:
        rp = f.robot_pose.copy(); rp[3:6] = pose
        f = dataclasses.replace(f, robot_pose=rp)
    f.cloud.setflags(write=False)
    return f


def frame(**kw):
    """make_frame(**kw), cached and read-only; ``rpy=(roll, pitch, yaw)`` replaces the attitude of the robot pose"""
    return _frame(_key(kw))


@functools.lru_cache(maxsize=None)
def _oracle(fkey, pkey):
    from oracle.oracle import segment_frame
    planes, nrm, lab = segment_frame(_frame(fkey), make_params(**dict(pkey)), want_products=True)
    assert len(planes) < 512, "the oracle's plane table is full: the case says nothing beyond it"
    nrm.setflags(write=False); lab.setflags(write=False)
    return planes, nrm, lab


def oracle_run(frame_kw, over):
    """(plane records, normals [npix, 4], label image [npix]) of the oracle, boxes packed back to back; cached"""
    return _oracle(_key(frame_kw), _key(over))


def box_crops(f):
    xyz = f.xyz()
    for b in f.boxes:
        w, h = int(b["width"]), int(b["height"])
        yield np.ascontiguousarray(xyz[b["tl_y"]:b["tl_y"] + h, b["tl_x"]:b["tl_x"] + w]).reshape(-1, 3), w, h


@functools.lru_cache(maxsize=None)
def _candidates(fkey, pkey):
    from oracle.oracle import box_normals, box_multi_plane
    p = make_params(**dict(pkey))
    out = []
    for pts, w, h in box_crops(_frame(fkey)):
        nrm, _ = box_normals(pts, w, h, p.max_depth_change_factor, p.normal_smoothing_size)
        regs, _, cc = box_multi_plane(pts, nrm, w, h, int(p.num_point_seg), p.angular_threshold, p.distance_threshold, p.maximum_curvature)
        sizes = np.bincount(cc[cc >= 0])
        out.append((int((sizes > int(p.num_point_seg)).sum()), len(regs)))
    return tuple(out)


def candidates_per_box(frame_kw, over):
    """per box: (connected components with more than num_point_seg pixels, regions the oracle accepts), from the oracle's
    pre-refinement component labels"""
    return _candidates(_key(frame_kw), _key(over))


def accepted_boxes(f, params):
    """indices of the boxes the host-side filter lets through (make_frame's boxes are whitelisted and inside the image)"""
    return [bi for bi, b in enumerate(f.boxes) if int(b["width"]) * int(b["height"]) >= params.norm_point_thres]


# ---- the comparison: the full bar of test_frame_matches_oracle_bit_exact ----------------------------------------------------------
def assert_planes_match_oracle(got, ref, what=""):
    assert len(got) == len(ref), f"{what}: {len(got)} planes, the oracle has {len(ref)}"
    for k, (a, r) in enumerate(zip(got, ref)):
        w = f"{what} plane {k}"
        assert a.box_index == r.box_index, w
        assert a.inlier_count == r.inlier_count, (w, a.inlier_count, r.inlier_count)
        assert a.num_points == r.num_points, (w, a.num_points, r.num_points)
        assert a.area == r.area, (w, a.area, r.area)
        assert a.plane_type == ("horizontal" if r.plane_type == 0 else "vertical"), w
        assert np.array_equal(a.pose, np.array(r.centroid_cam, np.float32)), w
        assert np.array_equal(a.normal_orientation, np.array(r.normal_d, np.float32)), w
        assert np.array_equal(a.world_pose, np.array(r.world_pose, np.float32)), w


def assert_images_match_oracle(seg, f, nrm, lab, what=""):
    """normals (NaN pattern, then values) and label image of every accepted box of frame 0 of the handle's last call"""
    off = 0
    for bi in accepted_boxes(f, seg.params):
        n = int(f.boxes[bi]["width"]) * int(f.boxes[bi]["height"])
        gn = seg.normals(bi).reshape(n, 4)
        on = nrm[off:off + n]
        assert np.array_equal(np.isnan(gn), np.isnan(on)), f"{what} box {bi}: NaN pattern of the normals differs"
        m = ~np.isnan(on)
        assert np.array_equal(gn[m], on[m]), f"{what} box {bi}: normals differ in {(gn[m] != on[m]).sum()} components"
        gl = seg.labels(bi).reshape(n)
        assert np.array_equal(gl, lab[off:off + n]), f"{what} box {bi}: label image differs in {(gl != lab[off:off + n]).sum()} px"
        off += n


def check_frames(seg, frames_kw, over, batched=False, check_drop=True):
    """Run the frames through `seg` (created with make_params(**over)) -- frame by frame, or all of them in one segment_frames call --
    and hold every product to the oracle's: normals, label images (of every frame, or of frame 0 of a batched call, which is what the
    parity hooks address) and every field of the plane records.  Returns the planes per frame."""
    frames = [frame(**kw) for kw in frames_kw]
    refs = [oracle_run(kw, over) for kw in frames_kw]
    if batched:
        got = seg.segment_frames(frames)
        if check_drop:
            assert seg.last_overflow()[0] == 0
        assert_images_match_oracle(seg, frames[0], refs[0][1], refs[0][2], "frame 0")
    else:
        got = []
        for k, (f, ref) in enumerate(zip(frames, refs)):
            got.append(seg.segmentallPointCloudData(f.robot_pose, f.cam_angle, f.boxes, f))
            if check_drop:
                assert seg.last_overflow()[0] == 0
            assert_images_match_oracle(seg, f, ref[1], ref[2], f"frame {k}")
    for k, (g, ref) in enumerate(zip(got, refs)):
        assert_planes_match_oracle(g, ref[0], f"frame {k}")
    return got


def assert_same_planes(a_list, b_list):
    """two results of the HIP path are the same records, bit for bit"""
    assert len(a_list) == len(b_list)
    for a, b in zip(a_list, b_list):
        assert (a.box_index, a.inlier_count, a.num_points, a.area, a.plane_type, a.type, a.prob) == \
               (b.box_index, b.inlier_count, b.num_points, b.area, b.plane_type, b.type, b.prob)
        assert np.array_equal(a.pose, b.pose) and np.array_equal(a.normal_orientation, b.normal_orientation)
        assert np.array_equal(a.world_pose, b.world_pose)
