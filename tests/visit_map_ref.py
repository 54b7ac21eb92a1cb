"""The visit map (include/rcw.h, rcw_set_visit_map) restated in numpy — test infrastructure, not a test.

  cell          the cell rule for a batch: (sector, i, j) per agent from positions in the world-unit type and 0-based direction indices;
                has[b] False where an agent has no cell (a position that is not finite, a tile off the map).  cell_index: the same as the
                linear index s*H*W + i + H*j the library uses, -1 for no cell.
  Tracked       an engine with the visit map on, and the definition applied beside it: after every call the test tells it what the call was
                (`stepped`, `refilled(mask)`, `untouched`), it reads the engine's OWN positions, direction indices, episode counters and
                layout words, applies COUNT / BEGIN and the table's adds, and holds the engine's map, four words and table to the result
                EXACTLY — everything is an integer.  `seen` counts what the run contained.
"""
import numpy as np

SATURATED = 65535


def cell(H, W, nd, sectors, pos, dirs):
    """pos (B, 2) in T, dirs (B,) 0-based.  Returns (has bool (B,), s, i, j int64 (B,)); s, i, j are 0 where has is False."""
    pos = np.asarray(pos)
    x, y = pos[:, 0], pos[:, 1]
    finite = np.isfinite(x) & np.isfinite(y)
    with np.errstate(invalid="ignore"):
        fx, fy = np.floor(x), np.floor(y)                                         # in the array's own type
        has = finite & (fx >= 0) & (fx < H) & (fy >= 0) & (fy < W)
    i = np.where(has, fx, 0).astype(np.int64)
    j = np.where(has, fy, 0).astype(np.int64)
    s = np.where(has, (np.asarray(dirs, np.int64) * sectors) // nd, 0)
    return has, s, i, j


def cell_index(H, W, nd, sectors, pos, dirs):
    has, s, i, j = cell(H, W, nd, sectors, pos, dirs)
    return np.where(has, s * H * W + i + H * j, -1)


class Tracked:
    def __init__(self, env, sectors=1, table=False, enable=True):
        self.env = env
        if enable:
            env.set_visit_map(sectors=sectors, table=table)
        info = env.visit_map_info
        assert info["enabled"]
        self.sectors, self.has_table, self.rows, self.first_level = info["sectors"], info["table"], info["rows"], info["first"]
        cfg = env.cfg
        self.H, self.W, self.nd, self.B = cfg.height_tile_map_tu, cfg.width_tile_map_tu, cfg.num_directions, env.batch
        B, S, H, W = self.B, self.sectors, self.H, self.W
        self.map = np.zeros((B, S, H, W), np.uint16)
        self.here, self.visited, self.first = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
        self.level_here = np.zeros(B, np.uint32)
        self.table = np.zeros((1 + self.rows, S, H, W), np.uint32)
        self.episode = np.zeros(B, np.uint32)
        self.counts = 0                                                           # COUNTs of agents with a cell since the table was zeroed
        self.seen = dict(checks=0, restarts=0, begun=0, kept=0, first1=0, first0=0, most=0, shared=0)
        if enable:
            self._apply(np.ones(B, bool), np.ones(B, bool))
            self.check("enabled")

    # ---- the definition ------------------------------------------------------------------------------------------------------------------
    def _state(self):
        w = self.env.world
        layout = np.asarray(self.env.wall_layout) if self.rows else None
        return w.player_position_wu, w.player_direction_au, w.episode.astype(np.uint32), layout

    def _rows_of(self, layout):
        """the table's row of every agent: 1 + (layout - first_level) where that is in range, else 0"""
        if layout is None:
            return np.zeros(self.B, np.int64)
        k = layout.astype(np.int64) - self.first_level
        return np.where((k >= 0) & (k < self.rows), 1 + k, 0)

    def _apply(self, touched, begin):
        """COUNT for the agents of `touched`, with BEGIN in front for those of `begin` (a subset); then level_here for every agent"""
        pos, dirs, episode, layout = self._state()
        has, s, i, j = cell(self.H, self.W, self.nd, self.sectors, pos, dirs)
        rows = self._rows_of(layout)
        added = set()
        for b in np.flatnonzero(touched):
            if begin[b]:
                self.map[b] = 0
                self.visited[b] = 0
            if has[b]:
                at = (b, s[b], i[b], j[b])
                v = int(self.map[at])
                self.first[b] = int(v == 0)
                self.map[at] = min(v + 1, SATURATED)
                self.visited[b] += self.first[b]
                self.here[b] = self.map[at]
                if self.has_table:
                    self.table[0, s[b], i[b], j[b]] += np.uint32(1)
                    if rows[b]:
                        self.table[rows[b], s[b], i[b], j[b]] += np.uint32(1)
                    key = (int(rows[b]), int(s[b]), int(i[b]), int(j[b]))
                    self.seen["shared"] += key in added
                    added.add(key)
                    self.counts += 1
            else:
                self.here[b] = self.first[b] = 0
            if begin[b]:
                self.first[b] = 0
                self.episode[b] = episode[b]
            else:
                self.seen["first1"] += int(self.first[b] == 1)
                self.seen["first0"] += int(self.first[b] == 0)
        if self.has_table:
            self.level_here = np.where(has, self.table[rows, s, i, j], 0).astype(np.uint32)

    # ---- what the test tells it -----------------------------------------------------------------------------------------------------------
    def stepped(self, where):
        """behind rcw_step / rcw_step_device: the counter decides who begins"""
        stale = self.env.world.episode.astype(np.uint32) != self.episode
        self.seen["restarts"] += int(stale.sum())
        self._apply(np.ones(self.B, bool), stale)
        return self.check(where)

    def refilled(self, mask, where):
        """behind reset_ / set_state / set_walls (mask None: every agent): the mask decides, the others keep every byte"""
        m = np.ones(self.B, bool) if mask is None else np.asarray(mask).astype(bool)
        self.seen["kept"] += int(((~m) & (self.map.reshape(self.B, -1).sum(axis=1) > 1)).sum())   # (kept a map worth keeping)
        self.seen["begun"] += int(m.sum())
        self._apply(m, m)
        return self.check(where)

    def untouched(self, where):
        """behind a call that must change nothing (a new direction table, a restore of nothing, ...)"""
        return self.check(where)

    def table_cleared(self):
        self.table[:] = 0
        self.counts = 0

    def check(self, where, env=None):
        """env: another engine that was given the same calls without a readout in between (the twin of a queued or replayed run)"""
        env = env or self.env
        got = dict(map=env.visit_map, here=env.visits_here.numpy(), visited=env.visited_cells.numpy(), first=env.visit_first.numpy(),
                   level_here=env.level_visits_here.numpy())
        exp = dict(map=self.map, here=self.here, visited=self.visited, first=self.first, level_here=self.level_here)
        for name, dtype in (("map", np.uint16), ("here", np.int32), ("visited", np.int32), ("first", np.int32), ("level_here", np.uint32)):
            assert got[name].dtype == dtype and got[name].shape == exp[name].shape, (name, got[name].dtype, got[name].shape)
            np.testing.assert_array_equal(got[name], exp[name], err_msg=f"{name} {where}")
        np.testing.assert_array_equal(exp["visited"], (self.map.reshape(self.B, -1) != 0).sum(axis=1))     # (the reference holds its own invariant)
        if self.has_table:
            t = env.visit_table()
            assert t["first"] == self.first_level and t["total"].dtype == np.uint32 and t["levels"].shape == self.table[1:].shape
            np.testing.assert_array_equal(t["total"], self.table[0], err_msg=f"table row 0 {where}")
            np.testing.assert_array_equal(t["levels"], self.table[1:], err_msg=f"table level rows {where}")
            assert int(t["total"].astype(np.int64).sum()) == self.counts, where
        self.seen["checks"] += 1
        self.seen["most"] = max(self.seen["most"], int(self.map.max()))
        return {k: v.copy() for k, v in exp.items()}
