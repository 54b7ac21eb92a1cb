"""The goal distance (include/rcw.h, rcw_set_goal_distance) restated in Python — test infrastructure, not a test.

  bfs_field       a deque breadth-first search over ONE (H, W) layout and goal: the uint16 field, 0xFFFF for walls and tiles without a path.
  GoalDistanceRef is fed the engine's OWN state after every call — walls, goal, position, episode counter — plus which agents an explicit
                  call masked, and keeps field, distance, start_distance and progress by the header's table.  State parity with the oracle is
                  the existing suite's job: this checks the new words against the state the engine reports.
  pocket, serpentine, pillars   the layouts the tests share; level_sizes and middle_free_tile say how wide a field's levels are and where
                  the wide-level cases put their goals.
  Tracked         an engine with the feature on and a GoalDistanceRef beside it: the one comparer of the GPU tests and of
                  tools/fuzz_parity.py goal.
"""
from collections import deque

import numpy as np

UNREACHED = 0xFFFF


def bfs_field(walls, goal):
    """walls: bool (H, W), walls[i-1, j-1]; goal: 1-based (i, j).  Distances in tiles between edge neighbours whose WALL bit is clear;
    the GOAL bit plays no part.  A goal inside a wall: every entry 0xFFFF.
    (Plain lists over the map with a closed border round it: the loop needs no range check, and numpy's scalar indexing was most of the
    time of a Python flood — the large maps of the GPU tests flood in tens of milliseconds.)"""
    w = np.asarray(walls) != 0
    H, W = w.shape
    gi, gj = int(goal[0]) - 1, int(goal[1]) - 1
    if not (0 <= gi < H and 0 <= gj < W) or w[gi, gj]:
        return np.full((H, W), UNREACHED, np.uint16)
    S = W + 2                                                              # the bordered map's row length
    closed = np.ones((H + 2, S), bool)
    closed[1:-1, 1:-1] = w
    closed = closed.reshape(-1).tolist()                                   # walls, the border, and what the flood has reached
    dist = [UNREACHED] * len(closed)
    start = (gi + 1) * S + gj + 1
    closed[start], dist[start] = True, 0
    q = deque([start])
    while q:
        t = q.popleft()
        d = dist[t] + 1
        for n in (t - S, t + S, t - 1, t + 1):
            if not closed[n]:
                closed[n], dist[n] = True, d
                q.append(n)
    return np.array(dist, np.uint16).reshape(H + 2, S)[1:-1, 1:-1].copy()


def linear(field):
    """The (H, W) field in the tile map's own linear order: tile (i, j), 1-based, at (i - 1) + H (j - 1)."""
    return np.ascontiguousarray(np.asarray(field).T).reshape(-1)


def lookup(field, pos):
    """field[t] for t = wu_to_tu(pos) (utils.jl:5: floor(x) + 1, floor(y) + 1), -1 where that is 0xFFFF or t is off the map."""
    H, W = field.shape
    x, y = float(pos[0]), float(pos[1])
    if not (np.isfinite(x) and np.isfinite(y)):
        return -1
    i, j = int(np.floor(x)), int(np.floor(y))
    if not (0 <= i < H and 0 <= j < W):
        return -1
    v = int(field[i, j])
    return -1 if v == UNREACHED else v


def pocket():
    """7 x 7: the ring plus a closed box of walls around (4, 4), 1-based — a free tile no other free tile reaches."""
    w = np.zeros((7, 7), bool)
    w[[0, -1], :] = True
    w[:, [0, -1]] = True
    for i, j in ((3, 3), (3, 4), (3, 5), (4, 3), (4, 5), (5, 3), (5, 4), (5, 5)):
        w[i - 1, j - 1] = True
    return w


def serpentine(H, W):
    """One corridor that snakes through the whole map: wall rows at every second interior row, each open at alternating ends.  The longest
    distance is about H W / 2 tiles and every breadth-first level holds one tile."""
    w = np.zeros((H, W), bool)
    w[[0, -1], :] = True
    w[:, [0, -1]] = True
    for k, i in enumerate(range(2, H - 2, 2)):                             # 0-based wall rows 2, 4, ...: free rows 1, 3, ...
        w[i, 1:W - 1] = True
        w[i, W - 2 if k % 2 == 0 else 1] = False
    return w


def pillars(H, W, density, rng):
    """The ring plus independent random interior walls: every interior tile is a wall with probability `density`.  Levels as wide as an
    open room's, ragged at every pillar; pockets without a path happen and are welcome (0xFFFF in the kernel and here alike).  A caller
    that hands the layout to set_walls checks that two tiles stayed free."""
    w = np.zeros((H, W), bool)
    w[[0, -1], :] = True
    w[:, [0, -1]] = True
    w[1:-1, 1:-1] |= rng.random((H - 2, W - 2)) < density
    return w


PILLAR_SEEDS = (0, 1, 2, 3, 5, 8, 9, 10)       # pillars(132, 134, 0.2, default_rng(seed)): the widest level from the middle free tile passes 128 tiles


def level_sizes(field):
    """The count of tiles at each distance of one field: level_sizes(f)[d] tiles are d steps from the goal ([] where nothing is reached).
    A breadth-first level of the kernel's queue holds exactly these tiles."""
    f = np.asarray(field)
    return np.bincount(f[f != UNREACHED].astype(np.int64))


def widest_level(field):
    s = level_sizes(field)
    return int(s.max()) if len(s) else 0


def middle_free_tile(walls):
    """1-based (i, j) of the middle one of a layout's free tiles in row-major order: a free tile of the middle row (near the middle)."""
    free = np.argwhere(~(np.asarray(walls) != 0))
    return tuple(int(v) + 1 for v in free[len(free) // 2])


class GoalDistanceRef:
    def __init__(self, walls, goal, pos, episode):
        """The state as of rcw_set_goal_distance(h, 1): every agent flooded, start_distance = distance, progress = 0."""
        self.B = len(goal)
        self.field = [None] * self.B
        self.distance = np.zeros(self.B, np.int32)
        self.start_distance = np.zeros(self.B, np.int32)
        self.progress = np.zeros(self.B, np.int32)
        self.recorded = np.zeros(self.B, np.uint32)
        self.masked(walls, goal, pos, episode, None)

    def _refresh(self, b, walls, goal, pos, episode):
        self.field[b] = bfs_field(walls[b], goal[b])
        self.distance[b] = self.start_distance[b] = lookup(self.field[b], pos[b])
        self.progress[b] = 0
        self.recorded[b] = episode[b]

    def masked(self, walls, goal, pos, episode, mask):
        """rcw_reset / rcw_set_state / rcw_set_walls (and enabling): the mask decides, not the counter; the others keep everything."""
        who = np.ones(self.B, bool) if mask is None else np.asarray(mask).reshape(self.B) != 0
        for b in np.flatnonzero(who):
            self._refresh(b, walls, goal, pos, episode)

    def stepped(self, walls, goal, pos, episode):
        """rcw_step / rcw_step_device: an agent whose episode counter moved is restarted; every other one takes progress = old - new where
        both are >= 0, else 0, and keeps start_distance."""
        for b in range(self.B):
            if int(episode[b]) != int(self.recorded[b]):
                self._refresh(b, walls, goal, pos, episode)
                continue
            old, new = int(self.distance[b]), lookup(self.field[b], pos[b])
            self.progress[b] = old - new if old >= 0 and new >= 0 else 0
            self.distance[b] = new

    @property
    def fields(self):
        return np.stack(self.field)


class Tracked:
    """An engine with the feature on and the reference beside it; every method makes the call on the engine, tells the reference what the
    header's table says the call does, and compares everything.  `raising`: the handle was made with out_of_bounds = 0, so a step may leave
    an IndexError for the next sync — taken there and cleared, the way tests/test_gpu_time_limit.py's raising cases do, before the state is
    read.  `floods` and `widest` say what the calls made the kernel flood: behind a step (its own stale path) or behind a masked call and
    enabling (the refill launch)."""

    def __init__(self, rcw, env, enable=True, raising=False):
        self.rcw, self.env, self.raising, self.steps_that_raised = rcw, env, raising, 0
        self.events = dict(unreachable=0, restart_after_done=0, restart_after_truncation=0, progress_up=0, progress_down=0)
        self.floods = dict(step=0, refill=0)
        self.widest = dict(step=0, refill=0)
        self._walls = None
        if enable:
            env.set_goal_distance(True)
            assert env.goal_distance_enabled
        self.ref = GoalDistanceRef(*self.state())
        self._flooded("refill", np.ones(env.batch, bool))
        self._flags()
        self.check("enabled")

    def state(self, walls_changed=True):
        w = self.env.world
        if walls_changed or self._walls is None:
            self._walls = w.walls
        return self._walls, w.goal_position, w.player_position_wu, w.episode

    def _flags(self):
        w = self.env.world
        self.done, self.truncated = w.done.astype(bool), w.truncated.astype(bool)

    def _flooded(self, how, who):
        self.floods[how] += int(who.sum())
        self.widest[how] = max([self.widest[how]] + [widest_level(self.ref.field[b]) for b in np.flatnonzero(who)])

    def check(self, where):
        env, ref = self.env, self.ref
        np.testing.assert_array_equal(env.goal_distance.numpy(), ref.distance, err_msg=f"distance {where}")
        np.testing.assert_array_equal(env.goal_start_distance.numpy(), ref.start_distance, err_msg=f"start_distance {where}")
        np.testing.assert_array_equal(env.goal_progress.numpy(), ref.progress, err_msg=f"progress {where}")
        field = env.goal_distance_field
        assert field.dtype == np.uint16 and field.shape == ref.fields.shape
        np.testing.assert_array_equal(field, ref.fields, err_msg=f"field {where}")

    def step(self, actions, where):
        ep0 = self.ref.recorded.copy()
        self.rcw.act_(self.env, actions)
        if self.raising:
            try:
                self.env.sync()
            except IndexError:
                assert (self.env.world.status != 0).any(), f"an IndexError without a status word, {where}"
                self.env.clear_error()
                self.steps_that_raised += 1
        self.ref.stepped(*self.state(walls_changed=False))
        moved = self.env.world.episode != ep0
        self._flooded("step", moved)
        ev = self.events
        ev["restart_after_done"] += int((moved & self.done).sum())
        ev["restart_after_truncation"] += int((moved & self.truncated & ~self.done).sum())
        ev["unreachable"] += int((self.ref.distance < 0).sum())
        ev["progress_up"] += int((self.ref.progress > 0).sum())
        ev["progress_down"] += int((self.ref.progress < 0).sum())
        self._flags()
        self.check(where)

    def masked(self, mask, where):
        """behind a reset_ / set_state / set_walls the caller has just made with `mask`"""
        self.ref.masked(*self.state(), mask)
        m = np.ones(self.env.batch, bool) if mask is None else np.asarray(mask) != 0
        self._flooded("refill", m)
        self._flags()
        self.check(where)
        np.testing.assert_array_equal(self.ref.start_distance[m], self.ref.distance[m])
        assert (self.ref.progress[m] == 0).all()

    def rollout(self, steps, seed, where):
        from walls_ref import draw_actions

        rng = np.random.default_rng(seed)
        for t in range(steps):
            self.step(draw_actions(rng, self.env.batch), f"{where}: step {t}")
