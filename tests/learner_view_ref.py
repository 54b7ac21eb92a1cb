"""The learner view's pixel contract (include/rcw.h, DESIGN.md "learner view") restated in numpy — test infrastructure.

from_frames       reduces UInt32 camera views (B, N, H) — the engine's or the oracle's — pixel by pixel;
from_descriptors  computes the same from the column descriptors (height_line_pu, colour id) and the configuration by counting, per
                  image column, the box rows that are ceiling, colour and floor.
Both return uint8 (B, C, h, w) for layout "chw" and (B, h, w, C) for "hwc"; C = 3 for "rgb", 1 for "gray"."""
import numpy as np


def row_bounds(H, h):
    return (np.arange(h + 1, dtype=np.int64) * H) // h


def gray_of(p):
    p = np.asarray(p, dtype=np.int64)
    return (77 * ((p >> 16) & 0xFF) + 150 * ((p >> 8) & 0xFF) + 29 * (p & 0xFF) + 128) >> 8


def channels_of(p, fmt):
    """(..., C) int64 channel values of packed 0x00RRGGBB pixels."""
    p = np.asarray(p, dtype=np.int64)
    if fmt == "gray":
        return gray_of(p)[..., None]
    return np.stack([(p >> 16) & 0xFF, (p >> 8) & 0xFF, p & 0xFF], axis=-1)


def _finish(S, n, layout):
    out = ((S + n[None, :, :, None] // 2) // n[None, :, :, None]).astype(np.uint8)     # (B, h, w, C)
    return np.ascontiguousarray(out.transpose(0, 3, 1, 2)) if layout == "chw" else np.ascontiguousarray(out)


def from_frames(frames, fmt, size, layout="chw"):
    frames = np.asarray(frames, dtype=np.uint32)
    B, N, H = frames.shape
    h, w = size
    assert 1 <= h <= H and 1 <= w <= N
    img = channels_of(frames.transpose(0, 2, 1), fmt)                      # (B, H, N, C): row first
    rb, cb = row_bounds(H, h), row_bounds(N, w)
    # box sums through prefix sums over rows, then columns (int64: a box can be the whole image)
    P = np.zeros((B, H + 1, N + 1, img.shape[-1]), dtype=np.int64)
    P[:, 1:, 1:] = img.cumsum(axis=1).cumsum(axis=2)
    S = P[:, rb[1:]][:, :, cb[1:]] - P[:, rb[:-1]][:, :, cb[1:]] - P[:, rb[1:]][:, :, cb[:-1]] + P[:, rb[:-1]][:, :, cb[:-1]]
    n = np.diff(rb)[:, None] * np.diff(cb)[None, :]
    return _finish(S, n, layout)


def padding(H, hl):
    """column_padding (SR:433-436): rows of ceiling at the top of a column of height_line_pu hl."""
    hl = np.asarray(hl, dtype=np.int64)
    pad = np.minimum((H - hl) // 2, H)
    return np.where(hl >= H - 1, 0, pad)


def colours(cfg):
    c = lambda name: cfg[name] if isinstance(cfg, dict) else getattr(cfg, name)
    return (c("ceiling_color"), c("floor_color"),
            [c("wall_dim_1_color"), c("wall_dim_2_color"), c("goal_dim_1_color"), c("goal_dim_2_color")])


def from_descriptors(col_h, col_c, cfg, H, fmt, size, layout="chw"):
    col_h = np.asarray(col_h, dtype=np.int64)
    col_c = np.asarray(col_c, dtype=np.int64) & 3
    B, N = col_h.shape
    h, w = size
    assert 1 <= h <= H and 1 <= w <= N
    ceil_c, floor_c, ids = colours(cfg)
    vc, vf = channels_of(ceil_c, fmt), channels_of(floor_c, fmt)          # (C,)
    vm = channels_of(np.array(ids, dtype=np.int64), fmt)[col_c]            # (B, N, C)
    pad = padding(H, col_h)                                                # (B, N)
    fs = np.maximum(pad, H - pad)
    rb, cb = row_bounds(H, h), row_bounds(N, w)
    r0, r1 = rb[:-1][None, :, None], rb[1:][None, :, None]                # (1, h, 1) against (B, 1, N)
    nc = np.maximum(0, np.minimum(r1, pad[:, None, :]) - r0)
    nf = np.maximum(0, r1 - np.maximum(r0, fs[:, None, :]))
    nm = (r1 - r0) - nc - nf                                               # (B, h, N)
    per_col = nc[..., None] * vc + nm[..., None] * vm[:, None, :, :] + nf[..., None] * vf   # (B, h, N, C)
    P = np.zeros((B, h, N + 1, per_col.shape[-1]), dtype=np.int64)
    P[:, :, 1:] = per_col.cumsum(axis=2)
    S = P[:, :, cb[1:]] - P[:, :, cb[:-1]]
    n = np.diff(rb)[:, None] * np.diff(cb)[None, :]
    return _finish(S, n, layout)
