"""The local map (include/rcw.h, rcw_set_local_map) restated in Python — test infrastructure, not a test.

  offsets         the offset table off[k] = T(2k + 1 - S) / T(2r): one division of two exactly representable integers in T.
  local_map_one   ONE agent's (S, S) image in numpy SCALARS of type T, a cell at a time, operation for operation as the header states them.
  local_map       the same for a batch at once in numpy ARRAYS of dtype T (the same IEEE operation per element, in the same order), which is
                  what makes comparing 64 agents after every call affordable; tests/test_local_map_spec.py holds it to local_map_one.
  Tracked         an engine with the feature on; after every call it reads the engine's OWN state — position, heading, the direction table
                  the handle holds, the tile map, the seen map — and compares every byte of every agent's image with local_map of it.  State
                  parity with the oracle, and the seen map itself, are the existing suite's job.
"""
import numpy as np

WORLD, SEEN = "world", "seen"


def offsets(S, r, T):
    return np.array([T(2 * k + 1 - S) / T(2 * r) for k in range(S)], dtype=T)


def linear(plane):
    """An (H, W) plane in the tile map's own linear order: tile (i, j), 1-based, at (i - 1) + H (j - 1)."""
    return np.ascontiguousarray(np.asarray(plane).T).reshape(-1)


def local_map_one(values, pos, d, S, r, T):
    """values: uint8 (H, W), what a cell over tile (i, j) shows: values[i-1, j-1] (1 + the tile's bits, or the seen map); pos (px, py);
    d (d1, d2) the heading vector.  uint8 (S, S)."""
    values = np.asarray(values)
    H, W = values.shape
    lin = linear(values)
    off = offsets(S, r, T)
    px, py, d1, d2 = T(pos[0]), T(pos[1]), T(d[0]), T(d[1])
    out = np.zeros((S, S), np.uint8)
    with np.errstate(all="ignore"):
        for q in range(S):
            for c in range(S):
                a, l = off[S - 1 - q], off[S - 1 - c]
                wx = T(T(px + T(a * d1)) + T(l * d2))
                wy = T(T(py + T(a * d2)) - T(l * d1))
                fx, fy = np.floor(wx), np.floor(wy)
                if fx >= 0 and fx < T(H) and fy >= 0 and fy < T(W):          # (a NaN fails every comparison)
                    out[q, c] = lin[int(fx) + H * int(fy)]
    return out


def local_map(values, pos, heading, dir_table, S, r, T):
    """values uint8 (B, H, W); pos (B, 2); heading int (B,); dir_table (nd, 2) of dtype T.  uint8 (B, S, S)."""
    values = np.asarray(values)
    B, H, W = values.shape
    dir_table = np.asarray(dir_table)
    assert dir_table.dtype == T
    lin = np.ascontiguousarray(values.transpose(0, 2, 1)).reshape(B, H * W)
    off = offsets(S, r, T)
    pos = np.asarray(pos).astype(T)
    d = dir_table[np.asarray(heading).astype(np.int64)]
    px, py, d1, d2 = (v.reshape(B, 1, 1) for v in (pos[:, 0], pos[:, 1], d[:, 0], d[:, 1]))
    a = off[::-1].reshape(1, S, 1)                                          # row q: off[S - 1 - q]
    l = off[::-1].reshape(1, 1, S)                                          # column c: off[S - 1 - c]
    with np.errstate(all="ignore"):
        wx = (px + a * d1) + l * d2
        wy = (py + a * d2) - l * d1
        assert wx.dtype == T and wy.dtype == T
        fx, fy = np.floor(wx), np.floor(wy)
        inside = (fx >= 0) & (fx < T(H)) & (fy >= 0) & (fy < T(W))
        t = np.where(inside, fx, 0).astype(np.int64) + H * np.where(inside, fy, 0).astype(np.int64)
    got = np.take_along_axis(lin, t.reshape(B, S * S), axis=1).reshape(B, S, S)
    return np.where(inside, got, 0).astype(np.uint8)


def tile_values(tile_map):
    """uint8 (B, H, W) from the engine's bool (B, 2, H, W) tile map: 1 + (WALL bit | GOAL bit << 1)."""
    tm = np.asarray(tile_map)
    return (1 + (tm[:, 0].astype(np.uint8) | (tm[:, 1].astype(np.uint8) << 1))).astype(np.uint8)


class Tracked:
    """An engine and the specification beside it: `check` reads the engine's state and compares every byte of every image."""

    def __init__(self, rcw, env, size, cells_per_tile=1, source=WORLD, enable=True):
        self.rcw, self.env = rcw, env
        if enable:
            env.set_local_map(size, cells_per_tile, source)
        self.S, self.r, self.source = size, cells_per_tile, source
        assert env.local_map_info == {"source": source, "size": size, "cells_per_tile": cells_per_tile}
        self.outside = self.inside = 0
        self.check("enabled")

    def want(self):
        env, w = self.env, self.env.world
        values = env.seen_map if self.source == SEEN else tile_values(w.tile_map)
        table = w.directions_wu
        assert table.dtype == env.T
        return local_map(values, w.player_position_wu, w.player_direction_au, table, self.S, self.r, env.T)

    def check(self, where):
        got, want = self.env.local_map_host(), self.want()
        assert got.dtype == np.uint8 and got.shape == (self.env.batch, self.S, self.S)
        np.testing.assert_array_equal(got, want, err_msg=f"local map {where}")
        self.outside += int((want == 0).sum())
        self.inside += int((want != 0).sum())
        return got

    def step(self, actions, where):
        self.rcw.act_(self.env, actions)
        return self.check(where)

    def rollout(self, steps, seed, where):
        from walls_ref import draw_actions

        rng = np.random.default_rng(seed)
        for t in range(steps):
            self.step(draw_actions(rng, self.env.batch), f"{where}: step {t}")
