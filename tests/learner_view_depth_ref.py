"""The learner view's depth plane (include/rcw.h "the learner view", formats RCW_VIEW_DEPTH8 / RGBD8 / GRAYD8) restated in numpy —
test infrastructure, beside learner_view_ref.py.

With Hc = height_camera_view_pu, hl a column's height_line_pu and pad = column_padding(Hc, hl), row y of the column holds
    u = min(max(hl, 0), Hc)           where pad <= y < Hc - pad (the colour's rows),
    u = Hc - 2 min(y, Hc - 1 - y)     on the ceiling and floor rows,
and D = (255 u + Hc // 2) // Hc; at reduced sizes D is averaged over the colour channels' boxes with their rounding.

Two independent readings of it:
  depth_frames        the full (B, Hc, N) byte image pixel by pixel (a Python loop over rows and columns' regions), and from_depth_frames,
                      which box-averages such an image with prefix sums;
  from_descriptors    counts, per image column and box, the ceiling / colour / floor rows and takes the ceiling and floor sums from a
                      prefix table of the edge value.
view() puts the colour planes of learner_view_ref.from_descriptors and the depth plane together for a format and a layout; full_size() is
the whole view at (Hc, N) alone, selected pixel by pixel in bytes."""
import numpy as np

import learner_view_ref as LV

CHANNELS = {"rgb": 3, "gray": 1, "depth": 1, "rgbd": 4, "grayd": 2}
COLOUR_OF = {"rgb": "rgb", "gray": "gray", "depth": None, "rgbd": "rgb", "grayd": "gray"}
HAS_DEPTH = {"rgb": False, "gray": False, "depth": True, "rgbd": True, "grayd": True}


def depth_byte(u, Hc):
    return (255 * np.asarray(u, dtype=np.int64) + Hc // 2) // Hc


def depth_frames(col_h, Hc):
    """(B, Hc, N) uint8: D of every camera pixel, written row by row from the rule."""
    col_h = np.asarray(col_h, dtype=np.int64)
    B, N = col_h.shape
    out = np.empty((B, Hc, N), dtype=np.uint8)
    y = np.arange(Hc, dtype=np.int64)
    edge = Hc - 2 * np.minimum(y, Hc - 1 - y)                              # u of a ceiling or floor pixel of row y
    for b in range(B):
        for k in range(N):
            hl = int(col_h[b, k])
            pad = 0 if hl >= Hc - 1 else min((Hc - hl) // 2, Hc)
            u = np.where((pad <= y) & (y < Hc - pad), min(max(hl, 0), Hc), edge)     # every pixel of the column
            out[b, :, k] = (255 * u + Hc // 2) // Hc
    return out


def from_depth_frames(D, size):
    """(B, h, w) uint8: the box averages of a (B, Hc, N) depth image."""
    D = np.asarray(D, dtype=np.int64)
    B, H, N = D.shape
    h, w = size
    rb, cb = LV.row_bounds(H, h), LV.row_bounds(N, w)
    P = np.zeros((B, H + 1, N + 1), dtype=np.int64)
    P[:, 1:, 1:] = D.cumsum(axis=1).cumsum(axis=2)
    S = P[:, rb[1:]][:, :, cb[1:]] - P[:, rb[:-1]][:, :, cb[1:]] - P[:, rb[1:]][:, :, cb[:-1]] + P[:, rb[:-1]][:, :, cb[:-1]]
    n = np.diff(rb)[:, None] * np.diff(cb)[None, :]
    return ((S + n[None] // 2) // n[None]).astype(np.uint8)


def from_descriptors(col_h, Hc, size):
    """(B, h, w) uint8: the same from the descriptors, by counting rows."""
    col_h = np.asarray(col_h, dtype=np.int64)
    B, N = col_h.shape
    h, w = size
    assert 1 <= h <= Hc and 1 <= w <= N
    pad = LV.padding(Hc, col_h)                                            # (B, N)
    fs = np.maximum(pad, Hc - pad)
    y = np.arange(Hc, dtype=np.int64)
    E = np.concatenate([[0], depth_byte(Hc - 2 * np.minimum(y, Hc - 1 - y), Hc).cumsum()])   # prefix sums of the edge value
    Dw = depth_byte(np.clip(col_h, 0, Hc), Hc)                             # (B, N)
    rb, cb = LV.row_bounds(Hc, h), LV.row_bounds(N, w)
    r0, r1 = rb[:-1][None, :, None], rb[1:][None, :, None]                # (1, h, 1) against (B, 1, N)
    c_end = np.maximum(r0, np.minimum(r1, pad[:, None, :]))                # ceiling rows [r0, c_end)
    f_beg = np.minimum(r1, np.maximum(r0, fs[:, None, :]))                 # floor rows [f_beg, r1)
    nm = np.maximum(0, f_beg - c_end)
    per_col = (E[c_end] - E[r0]) + nm * Dw[:, None, :] + (E[r1] - E[f_beg])   # (B, h, N)
    P = np.zeros((B, h, N + 1), dtype=np.int64)
    P[:, :, 1:] = per_col.cumsum(axis=2)
    S = P[:, :, cb[1:]] - P[:, :, cb[:-1]]
    n = np.diff(rb)[:, None] * np.diff(cb)[None, :]
    return ((S + n[None] // 2) // n[None]).astype(np.uint8)


def assemble(colour, depth, layout):
    """colour: (B, C, h, w) uint8 or None; depth: (B, h, w) uint8 or None -> the view in `layout`."""
    planes = ([] if colour is None else [colour]) + ([] if depth is None else [depth[:, None]])
    chw = np.concatenate(planes, axis=1)
    return np.ascontiguousarray(chw if layout == "chw" else chw.transpose(0, 2, 3, 1))


def view(col_h, col_c, cfg, Hc, fmt, size, layout="chw", depth=from_descriptors):
    """The learner view of format `fmt` ("rgb", "gray", "depth", "rgbd", "grayd") from the descriptors: uint8 (B, C, h, w) or (B, h, w, C).
    `depth`: the reading of the depth plane, from_descriptors or `lambda col_h, Hc, size: from_depth_frames(depth_frames(col_h, Hc), size)`."""
    colour = None if COLOUR_OF[fmt] is None else LV.from_descriptors(col_h, col_c, cfg, Hc, COLOUR_OF[fmt], size, "chw")
    d = depth(col_h, Hc, size) if HAS_DEPTH[fmt] else None
    return assemble(colour, d, layout)


def by_frames(col_h, Hc, size):
    return from_depth_frames(depth_frames(col_h, Hc), size)


def full_size(col_h, col_c, cfg, Hc, fmt, layout="chw"):
    """view() at size (Hc, N), where a box is one pixel and nothing is averaged: every plane selected per pixel from the column rule, in
    bytes — for batches at which view()'s int64 box sums take seconds (a thousand agents).  tests/test_learner_view_depth_spec.py holds it
    against view() byte for byte."""
    col_h = np.asarray(col_h, dtype=np.int64)
    B, N = col_h.shape
    pad = LV.padding(Hc, col_h)
    fs = np.maximum(pad, Hc - pad).astype(np.int32)[:, None, :]
    y = np.arange(Hc, dtype=np.int32)[None, :, None]
    ceiling, floor = y < pad.astype(np.int32)[:, None, :], y >= fs
    planes = []
    if COLOUR_OF[fmt] is not None:
        ceil_c, floor_c, ids = LV.colours(cfg)
        vc, vf = LV.channels_of(ceil_c, COLOUR_OF[fmt]), LV.channels_of(floor_c, COLOUR_OF[fmt])
        vm = LV.channels_of(np.array(ids, dtype=np.int64), COLOUR_OF[fmt])[np.asarray(col_c, dtype=np.int64) & 3].astype(np.uint8)   # (B, N, C)
        for k in range(len(vc)):
            planes.append(np.where(ceiling, np.uint8(vc[k]), np.where(floor, np.uint8(vf[k]), vm[:, None, :, k])))
    if HAS_DEPTH[fmt]:
        rows = np.arange(Hc, dtype=np.int64)
        edge = depth_byte(Hc - 2 * np.minimum(rows, Hc - 1 - rows), Hc).astype(np.uint8)[None, :, None]
        wall = depth_byte(np.clip(col_h, 0, Hc), Hc).astype(np.uint8)[:, None, :]
        planes.append(np.where(ceiling | floor, edge, wall))
    chw = np.stack(planes, axis=1)
    return np.ascontiguousarray(chw if layout == "chw" else chw.transpose(0, 2, 3, 1))
