"""Detections for find_matches that take the landmark table past two strides of k_associate's 256 threads and make equal-distance
ties between landmarks 256 or more indices apart -- test helper, not collected.

A detection at the camera origin (pose 0, 0, 0) lands on the robot's position exactly: the rotation part of the world transform
multiplies zeros.  So a landmark mapped from the robot at c + d, one of the same kind mapped much later from c - d (too far from the
first to match it: a new landmark), and a detection from c have float-equal distances, z and -z, in the Euclidean mode and -- all
covariances being the same multiple of the identity -- in the Mahalanobis mode too.  c, d and c +- d are exact in float32.  (An exact
twin of a mapped landmark is never mapped as new without quirk B5: its distance is 0.)

Four kinds (class, plane type) carry one tie pair each, at table indices chosen by the place of their detections in the frames:
    kind (1, 0): 0 and 256   the same thread, one stride apart
    kind (2, 1): 1 and 257   likewise
    kind (3, 0): 2 and 279   two lanes of the first wave (shuffle arg-min)
    kind (3, 1): 3 and 330   the first and the second wave (the arg-min across waves)
With quirk B5 (distance_min carried from detection to detection inside a call) only the first detection of a frame sees a fresh
minimum, so a tie frame then holds one tie detection, and the kinds take turns.
"""
from __future__ import annotations

import numpy as np

TIE_KINDS = [(1, 0), (2, 1), (3, 0), (3, 1)]
TIE_INDICES = [(0, 256), (1, 257), (2, 279), (3, 330)]
C0 = np.array([-64.0, -32.0, 0.5], np.float32)
RPY = np.array([0.02, -0.03, 0.7], np.float32)
N_TIE_FRAMES = 6


def _grid(rng, n, depth):
    """n detections on a 3 m grid in the camera frame, `depth` metres out, with 0.3 m of jitter: at least 2.4 m apart"""
    out = []
    for k in range(n):
        p = np.array([3.0 * (k % 8) - 10.0, 3.0 * (k // 8) - 6.0, depth], np.float32) + rng.uniform(-0.3, 0.3, 3).astype(np.float32)
        out.append(dict(pose=p, normal=rng.normal(size=4).astype(np.float32), class_id=int(rng.integers(1, 4)), plane_type=int(rng.integers(0, 2))))
    return out


def _origin(rng, kind):
    return dict(pose=np.zeros(3, np.float32), normal=rng.normal(size=4).astype(np.float32), class_id=kind[0], plane_type=kind[1])


def schedule(use_eq: bool, quirk: bool, seed: int = 7):
    """-> list of (robot pose [6] float32, detections, tie kinds expected at the head of this frame's detections)"""
    rng = np.random.default_rng(seed)
    d = np.array([1.0 if use_eq else 0.5, 0.0, 0.0], np.float32)      # |2d| is beyond the match threshold (1.21 / 0.5 squared), |d| inside it
    pose = lambda t: np.concatenate([np.asarray(t, np.float32), RPY]).astype(np.float32)
    far = lambda k: pose([100.0 * k, 7.0, 0.1])
    frames = []
    visit = 0                                                        # visits of the region around C0 look at grids 2 m further out each time

    def near(t, heads, places=None):
        nonlocal visit
        objs = _grid(rng, 40, 5.0 + 2.0 * visit)
        visit += 1
        if places is None:
            objs = [_origin(rng, k) for k in heads] + objs[len(heads):]
        else:
            for k, p in zip(heads, places):
                objs[p] = _origin(rng, k)
        return (pose(t), objs)
    frames.append(near(C0 + d, TIE_KINDS) + ([],))                   # landmarks 0..3: the four first twins
    for k in range(1, 6):
        frames.append((far(k), _grid(rng, 40, 5.0), []))             # .. 239
    frames.append(near(C0 - d, TIE_KINDS[:3], [16, 17, 39]) + ([],))  # 256, 257, 279
    frames.append((far(7), _grid(rng, 40, 5.0), []))                 # .. 319
    frames.append(near(C0 - d, TIE_KINDS[3:], [10]) + ([],))         # 330
    for r in range(N_TIE_FRAMES):
        heads = [TIE_KINDS[r % 4]] if quirk else TIE_KINDS[r % 4:] + TIE_KINDS[:r % 4]
        frames.append(near(C0, heads) + (heads,))
    frames.append((far(20), _grid(rng, 40, 5.0), []))               # past 600 landmarks: 616 without quirk B5, 634 with it
    return frames
