"""The seen map (include/rcw.h, rcw_set_seen_map) restated in Python — test infrastructure, not a test.

  visited_tiles   RayCaster.cast_ray's march of ONE ray restated in numpy scalars of type T, with the ray table's own |1/dx|, |1/dy|: the
                  tiles the ray is on, in order, from the player's tile through the stop tile.
  marked_tiles    the same march for every ray of every agent at once (numpy arrays of dtype T: the same IEEE operation per element, in the
                  same order), which is what makes a rollout of 64 agents affordable; tests/test_seen_map_spec.py holds it to visited_tiles.
  SeenMapRef      is fed the engine's OWN state after every call — the tile map's two layers, goal, position, heading, episode counter —,
                  the engine's own ray table (rcw_ray_table / rcw_ray_table64: the floats are the device's) and which agents an explicit
                  call masked, and keeps map, seen_count, newly_seen and goal_seen by the header's table.  State parity with the oracle is
                  the existing suite's job: this checks the new arrays against the state the engine reports.
  ring, crossed   the layouts the tests share.
  Tracked         an engine with the feature on and a SeenMapRef beside it: the one comparer of the GPU tests; it counts the events it saw.
"""
import numpy as np


def ring(H, W):
    """the wall ring alone: the reference's empty room"""
    w = np.zeros((H, W), bool)
    w[[0, -1], :] = True
    w[:, [0, -1]] = True
    return w


def crossed(size=9):
    """the ring plus a wall cross through the centre with a gap in each arm: rays stop on interior walls, and see through the gaps"""
    w = ring(size, size)
    c = size // 2
    w[c, 1:-1] = True
    w[1:-1, c] = True
    for i, j in ((c, 2), (c, size - 3), (2, c), (size - 3, c)):
        w[i, j] = False
    return w


def tile_bits(tile_map):
    """uint8 (B, H, W) from the engine's bool (B, 2, H, W) tile map: WALL bit | GOAL bit << 1."""
    tm = np.asarray(tile_map)
    return (tm[:, 0].astype(np.uint8) | (tm[:, 1].astype(np.uint8) << 1)).astype(np.uint8)


def linear(plane):
    """An (H, W) plane in the tile map's own linear order: tile (i, j), 1-based, at (i - 1) + H (j - 1)."""
    return np.ascontiguousarray(np.asarray(plane).T).reshape(-1)


def visited_tiles(obstacles, x, y, dx, dy, ddx, ddy, tie_le, T):
    """obstacles: bool (H, W), obstacles[i-1, j-1] (WALL or GOAL); the ray (dx, dy) with ddx = |1 / dx|, ddy = |1 / dy| from (x, y), all
    taken as T.  The 1-based tiles (i, j) the march is on, in order; the last one is the stop tile.  A start off the map (or NaN): [].
    A ray that leaves the map ends with the last tile it was on inside it (every map the library accepts stops it before)."""
    obstacles = np.asarray(obstacles) != 0
    H, W = obstacles.shape
    x, y, dx, dy, ddx, ddy = (T(v) for v in (x, y, dx, dy, ddx, ddy))
    if not (np.isfinite(x) and np.isfinite(y)):
        return []
    i, j = int(np.floor(x)) + 1, int(np.floor(y)) + 1                      # wu_to_tu UT:5
    if not (1 <= i <= H and 1 <= j <= W):
        return []
    with np.errstate(all="ignore"):
        si = -1 if dx < 0 else 1
        sj = -1 if dy < 0 else 1
        sx = ((x - T(i - 1)) if dx < 0 else (T(i) - x)) * ddx
        sy = ((y - T(j - 1)) if dy < 0 else (T(j) - y)) * ddy
        out = [(i, j)]
        while not obstacles[i - 1, j - 1]:
            if (sx <= sy) if tie_le else (sx < sy):
                sx = sx + ddx
                i += si
            else:
                sy = sy + ddy
                j += sj
            if not (1 <= i <= H and 1 <= j <= W):
                break
            out.append((i, j))
    return out


def marked_tiles(bits, pos, heading, table, tie_le, T):
    """bits uint8 (n, H, W), pos (n, 2), heading (n,), table (nd, 5, N) of dtype T: bool (n, H, W), the tiles the n agents' N rays visit."""
    bits = np.asarray(bits)
    n, H, W = bits.shape
    HW = H * W
    table = np.asarray(table)
    assert table.dtype == T
    obst = (bits != 0).transpose(0, 2, 1).reshape(n, HW)
    pos = np.asarray(pos).astype(T)
    x, y = pos[:, 0:1], pos[:, 1:2]                                        # (n, 1): broadcast over the rays
    rows = table[np.asarray(heading).astype(np.int64)]                     # (n, 5, N)
    dx, dy, ddx, ddy = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]
    with np.errstate(all="ignore"):
        fx, fy = np.floor(x), np.floor(y)
        on = np.isfinite(x) & np.isfinite(y) & (fx >= 0) & (fx < H) & (fy >= 0) & (fy < W)
        i0 = np.where(on, fx, 0).astype(np.int64) + 1
        j0 = np.where(on, fy, 0).astype(np.int64) + 1
        neg_x, neg_y = dx < 0, dy < 0
        si = np.where(neg_x, -1, 1)
        tj = np.where(neg_y, -H, H)
        sx = (np.where(neg_x, x - (i0 - 1).astype(T), i0.astype(T) - x) * ddx).astype(T)
        sy = (np.where(neg_y, y - (j0 - 1).astype(T), j0.astype(T) - y) * ddy).astype(T)
        assert sx.dtype == T and sy.dtype == T
        t = np.broadcast_to((i0 - 1) + H * (j0 - 1), dx.shape).copy()
        active = np.broadcast_to(on, dx.shape).copy()
        who = np.broadcast_to(np.arange(n)[:, None], dx.shape)
        marked = np.zeros((n, HW), bool)
        while active.any():
            inside = active & (t >= 0) & (t < HW)
            marked[who[inside], t[inside]] = True
            active = inside & ~obst[who, np.clip(t, 0, HW - 1)]
            xf = (sx <= sy) if tie_le else (sx < sy)
            sx = np.where(active & xf, sx + ddx, sx)
            sy = np.where(active & ~xf, sy + ddy, sy)
            t = t + np.where(active, np.where(xf, si, tj), 0)
    return np.ascontiguousarray(marked.reshape(n, W, H).transpose(0, 2, 1))


class SeenMapRef:
    def __init__(self, table, tie_le, bits, goal, pos, heading, episode):
        """The state as of rcw_set_seen_map(h, 1): every agent cleared and marked from its pose, newly_seen = 0."""
        bits = np.asarray(bits)
        self.B, self.H, self.W = bits.shape
        self.table, self.tie_le, self.T = np.asarray(table), bool(tie_le), np.asarray(table).dtype.type
        self.map = np.zeros((self.B, self.H, self.W), np.uint8)
        self.seen_count = np.zeros(self.B, np.int32)
        self.newly_seen = np.zeros(self.B, np.int32)
        self.goal_seen = np.zeros(self.B, np.int32)
        self.recorded = np.zeros(self.B, np.uint32)
        self.masked(bits, goal, pos, heading, episode, None)

    def set_table(self, table):
        """rcw_set_direction_table*: nothing is marked by the call; the next marking uses the new rays."""
        assert np.asarray(table).dtype == self.table.dtype
        self.table = np.asarray(table)

    def _mark(self, who, clear, bits, goal, pos, heading):
        who = np.flatnonzero(who)
        if len(who) == 0:
            return
        bits, goal = np.asarray(bits), np.asarray(goal)
        marked = marked_tiles(bits[who], np.asarray(pos)[who], np.asarray(heading)[who], self.table, self.tie_le, self.T)
        for k, b in enumerate(who):
            if clear:
                self.map[b] = 0
            fresh = marked[k] & (self.map[b] == 0)
            self.map[b][fresh] = 1 + bits[b][fresh]
            self.newly_seen[b] = 0 if clear else int(fresh.sum())
            self.seen_count[b] = int((self.map[b] != 0).sum())
            gi, gj = int(goal[b][0]), int(goal[b][1])
            on_map = 1 <= gi <= self.H and 1 <= gj <= self.W
            self.goal_seen[b] = int(on_map and self.map[b, gi - 1, gj - 1] != 0)

    def masked(self, bits, goal, pos, heading, episode, mask):
        """rcw_reset / rcw_set_state / rcw_set_walls (and enabling): the mask decides, not the counter; the others keep everything.  The
        counter of a cleared agent is recorded, so the step behind a reset does not clear it once more."""
        who = np.ones(self.B, bool) if mask is None else np.asarray(mask).reshape(self.B) != 0
        self._mark(who, True, bits, goal, pos, heading)
        self.recorded[who] = np.asarray(episode)[who]

    def stepped(self, bits, goal, pos, heading, episode):
        """rcw_step / rcw_step_device: an agent whose episode counter moved is cleared and marked from its new pose; every other one is
        marked on top of what it has."""
        moved = np.asarray(episode) != self.recorded
        self._mark(moved, True, bits, goal, pos, heading)
        self._mark(~moved, False, bits, goal, pos, heading)
        self.recorded[moved] = np.asarray(episode)[moved]
        return moved

    @property
    def maps_linear(self):
        """uint8 (B, H*W): the export's own order"""
        return np.stack([linear(m) for m in self.map])


EVENTS = ("new_after_turn", "new_after_move", "no_new_blocked", "goal_seen_flipped", "restart_after_done", "restart_after_truncation")


def account(events, ref, moved, goal_seen_before, done_before, truncated_before, pose_before, pose_after, actions, table_changed, where):
    """What a step that `ref` has just taken showed, added to `events` — and what no step may show: new tiles for a restarted agent or from
    an unchanged pose (unless the ray table changed in between), goal_seen going back within an episode.  actions: None if unknown."""
    events["restart_after_done"] += int((moved & done_before).sum())
    events["restart_after_truncation"] += int((moved & truncated_before & ~done_before).sum())
    assert (ref.newly_seen[moved] == 0).all(), where
    stay, new = ~moved, ref.newly_seen > 0
    events["goal_seen_flipped"] += int((stay & (goal_seen_before == 0) & (ref.goal_seen == 1)).sum())
    assert not (stay & (goal_seen_before == 1) & (ref.goal_seen == 0)).any(), f"goal_seen went back within an episode, {where}"
    same_pose = (np.asarray(pose_after[0]) == np.asarray(pose_before[0])).all(axis=1) & (np.asarray(pose_after[1]) == np.asarray(pose_before[1]))
    if not table_changed:
        assert not (stay & same_pose & new).any(), f"new tiles from an unchanged pose, {where}"
    if actions is not None:
        a = np.asarray(actions)
        events["new_after_turn"] += int((stay & (a >= 3) & (a <= 4) & new).sum())
        events["new_after_move"] += int((stay & (a >= 1) & (a <= 2) & ~same_pose & new).sum())
        events["no_new_blocked"] += int((stay & (a >= 1) & (a <= 2) & same_pose).sum())


class Tracked:
    """An engine with the feature on and the reference beside it; every method makes the call on the engine, tells the reference what the
    header's table says the call does, and compares everything.  `raising`: the handle was made with out_of_bounds = 0, so a step may leave
    an IndexError for the next sync — taken there and cleared before the state is read."""

    def __init__(self, rcw, env, enable=True, raising=False):
        self.rcw, self.env, self.raising, self.steps_that_raised = rcw, env, raising, 0
        self.events = dict.fromkeys(EVENTS, 0)
        self.table_changed = False
        if enable:
            env.set_seen_map(True)
            assert env.seen_map_enabled
        self.ref = SeenMapRef(env.ray_table(), env.cfg.dda_tie_break != 0, *self.state())
        self._remember()
        self.check("enabled")

    def state(self):
        w = self.env.world
        return tile_bits(w.tile_map), w.goal_position, w.player_position_wu, w.player_direction_au, w.episode

    def _remember(self):
        w = self.env.world
        self.done, self.truncated = w.done.astype(bool), w.truncated.astype(bool)
        self.pos, self.heading = w.player_position_wu.copy(), w.player_direction_au.copy()

    def check(self, where):
        env, ref = self.env, self.ref
        np.testing.assert_array_equal(env.seen_count.numpy(), ref.seen_count, err_msg=f"seen_count {where}")
        np.testing.assert_array_equal(env.seen_new.numpy(), ref.newly_seen, err_msg=f"newly_seen {where}")
        np.testing.assert_array_equal(env.goal_seen.numpy(), ref.goal_seen, err_msg=f"goal_seen {where}")
        got = env.seen_map
        assert got.dtype == np.uint8 and got.shape == ref.map.shape
        np.testing.assert_array_equal(got, ref.map, err_msg=f"map {where}")

    def stepped(self, actions, where):
        """behind a step the caller has just made (actions: what it passed, None if the test does not know)"""
        if self.raising:
            try:
                self.env.sync()
            except IndexError:
                assert (self.env.world.status != 0).any(), f"an IndexError without a status word, {where}"
                self.env.clear_error()
                self.steps_that_raised += 1
        seen0 = self.ref.goal_seen.copy()
        moved = self.ref.stepped(*self.state())
        w = self.env.world
        account(self.events, self.ref, moved, seen0, self.done, self.truncated, (self.pos, self.heading),
                (w.player_position_wu, w.player_direction_au), actions, self.table_changed, where)
        self.table_changed = False
        self._remember()
        self.check(where)

    def set_direction_table(self, directions):
        """the call marks nothing; the next step marks with the new rays"""
        self.env.set_direction_table(directions)
        self.ref.set_table(self.env.ray_table())
        self.table_changed = True
        self.check("behind set_direction_table")

    def step(self, actions, where):
        self.rcw.act_(self.env, actions)
        self.stepped(actions, where)

    def masked(self, mask, where):
        """behind a reset_ / set_state / set_walls the caller has just made with `mask`"""
        self.ref.masked(*self.state(), mask)
        m = np.ones(self.env.batch, bool) if mask is None else np.asarray(mask) != 0
        self._remember()
        self.check(where)
        assert (self.ref.newly_seen[m] == 0).all()

    def rollout(self, steps, seed, where):
        from walls_ref import draw_actions

        rng = np.random.default_rng(seed)
        for t in range(steps):
            self.step(draw_actions(rng, self.env.batch), f"{where}: step {t}")
