"""Organised clouds in other PointCloud2 layouts, and detection boxes on the image border -- test helper, not collected.

synth.make_frame and synth.repack_xyz always give row_step == width * point_step and x, y, z at offsets 0, 4, 8; with such frames a
reader that takes row_step for width * point_step, or a field offset for 4 * k, reads the right bytes.  ``relayout`` moves x, y, z to
arbitrary offsets inside a point of any size, pads every row, and fills every byte that is not a coordinate with the float 7.5e8: a
reader that strays lands on a finite, absurd coordinate (which changes plane records, label images and normals) and not on a NaN,
which the pipeline would quietly drop.
"""
from __future__ import annotations

import copy
import dataclasses

import numpy as np

FILL = 7.5e8

# (point_step, (off_x, off_y, off_z), bytes of padding after every row)
LAYOUTS = [
    (20, (8, 0, 12), 28),      # permuted fields, a point that is no power of two, padded rows
    (12, (0, 4, 8), 64),       # packed xyz, padded rows only
    (32, (16, 20, 4), 0),      # the registered cloud's size with the fields elsewhere
    (24, (4, 12, 20), 4),      # gaps between the fields, the last one ending with the point
]


def read_xyz(frame) -> np.ndarray:
    """[height, width, 3] float32 by the frame's own layout"""
    h, w, ps = frame.height, frame.width, frame.point_step
    rows = np.ascontiguousarray(frame.cloud, np.uint8).reshape(h, frame.row_step)[:, :w * ps].reshape(h, w, ps)
    return np.stack([np.ascontiguousarray(rows[:, :, o:o + 4]).view(np.float32)[:, :, 0] for o in frame.offsets], axis=-1)


def relayout(frame, point_step, offsets, row_pad, fill=FILL):
    """the same frame with x, y, z at `offsets` of a `point_step`-byte point and `row_pad` bytes after every row (the last one included:
    the cloud holds height * row_step bytes); every other byte belongs to a float32 `fill`"""
    assert point_step % 4 == 0 and row_pad % 4 == 0 and all(o % 4 == 0 and 0 <= o <= point_step - 4 for o in offsets) and len(set(offsets)) == 3
    xyz = read_xyz(frame)
    h, w = frame.height, frame.width
    row_step = w * point_step + row_pad
    buf = np.full((h, row_step // 4), fill, np.float32)
    pts = buf[:, :w * point_step // 4].reshape(h, w, point_step // 4)      # a view: the padding keeps the fill
    for k, o in enumerate(offsets):
        pts[:, :, o // 4] = xyz[:, :, k]
    new = dict(cloud=buf.reshape(-1).view(np.uint8).copy(), point_step=point_step, row_step=row_step, offsets=tuple(offsets))
    if dataclasses.is_dataclass(frame):
        out = dataclasses.replace(frame, **new)
    else:
        out = copy.copy(frame)
        for k, v in new.items():
            setattr(out, k, v)
    assert np.array_equal(read_xyz(out), xyz, equal_nan=True) and out.cloud.nbytes == h * row_step
    return out


def border_boxes(frame, box_w, box_h):
    """`frame` with eight boxes flush against the image border -- the four corners (0-3: top left, top right, bottom left, bottom right)
    and the middles of the four edges (4: top, 5: bottom, 6: left, 7: right) -- followed by three boxes that stick out by one pixel (8:
    over the right edge, 9: over the bottom edge, 10: tl_x = -1), which both the reference and the product drop
    (plane_segmentation.cpp:34-38)"""
    W, H = frame.width, frame.height
    r, b, mx, my = W - box_w, H - box_h, (W - box_w) // 2, (H - box_h) // 2
    tl = [(0, 0), (r, 0), (0, b), (r, b), (mx, 0), (mx, b), (0, my), (r, my), (r + 1, my), (mx, b + 1), (-1, my)]
    boxes = np.zeros(len(tl), frame.boxes.dtype)
    boxes["tl_x"] = [t[0] for t in tl]; boxes["tl_y"] = [t[1] for t in tl]
    boxes["width"] = box_w; boxes["height"] = box_h
    boxes["class_id"] = frame.boxes["class_id"][0]; boxes["prob"] = 0.9
    return dataclasses.replace(frame, boxes=boxes)


RIGHT_EDGE, BOTTOM_EDGE, OUTSIDE = (1, 3, 7), (2, 3, 5), (8, 9, 10)

# Frames chosen by what the CPU oracle alone finds in them (the tests assert these counts; they are properties of synth.make_frame):
LAYOUT_FRAME = dict(seed=4, n_boxes=32)                    # 8 planes (seed 0 with its 32 boxes has 4, seed 1 with 10 boxes 3)
LAYOUT_BATCH = (dict(seed=4, n_boxes=32), dict(seed=7, n_boxes=32), dict(seed=9, n_boxes=32))    # 8, 7 and 6 planes
# The bottom of the image sees the floor from 1.5 m: with 128 x 96 boxes no seed of 0..7 gives a plane on the bottom edge.
BORDER_FRAMES = [(13, 200, 150),                           # planes in boxes 1, 3, 4, 7: the bottom right corner and the right edge
                 (3, 256, 192)]                            # planes in boxes 0, 1, 2, 4, 5, 6, 7: every edge, three corners
WIDE_FRAME = dict(seed=3, width=800, height=600, n_boxes=1, box_w=800, box_h=150)   # one box as wide as the image: 6 planes
