"""The wall bank's scenarios, written ONCE and run twice — test infrastructure, not a test.

A scenario is a function of a driver: it builds banks, draws actions from a seeded generator and makes calls (set_wall_bank, step, reset,
set_state, set_weights, ...).  Two drivers take the same calls:

    Recorder   the reference alone (tests/wall_bank_ref.py, under tests/time_limit_ref.py where the scenario sets a limit): every call
               is followed by a snapshot.  tests/test_wall_bank_spec.py runs it with render=False and asserts from the reference's own
               counts that the scenario reaches what it claims; `recorded(name)` runs it once with frames and keeps the snapshots.
    Player     an engine: every call is made on it and compared with the next snapshot, byte for byte — walls_ref.assert_equal plus
               wall_layout, and the time limit's two words where a limit is set — and then handed to the feature trackers the test
               attached (goal distance, seen map, local map), which compare their own arrays against the engine's state.

Every scenario: 8 headings, a quarter tile a move, a player radius of 0.3, auto_reset, forward-heavy actions (walls_ref.draw_actions).
"""
import functools

import numpy as np

import time_limit_ref as TL
import wall_bank_ref as WB
import walls_ref as WR


def _layouts():
    import raycastworlds_jl_amd as RCW

    return RCW.layouts


def three_layouts(H, W):
    """ring only | two pillars | four rooms"""
    L = _layouts()
    pillars = L.ring(H, W)
    pillars[2, 2] = pillars[2, 4] = True
    return np.stack([L.ring(H, W), pillars, L.four_rooms(H, W)])


def mazes(H, W, n, seed):
    L = _layouts()
    return np.stack([L.maze(H, W, np.random.default_rng(seed + k)) for k in range(n)])


def pillars_and_mazes(H, W, n, seed):
    """every other layout a maze, the rest a grid of pillars with one of them (by k) taken out: n distinct layouts"""
    L = _layouts()
    out = mazes(H, W, n, seed)
    for k in range(0, n, 2):
        w = L.ring(H, W)
        w[2:-2:2, 2:-2:2] = True
        rows = (H - 3) // 2                                                   # pillars along an axis
        w[2 + 2 * ((k // 2) % rows), 2 + 2 * ((k // 2) // rows)] = False
        out[k] = w
    return out


def ragged_weights(n):
    """1, 0, 7, 2, 0, 0, 3, 1000, ... : zeros, repeats and one heavy entry, far from a power of two in sum"""
    base = [1, 0, 7, 2, 0, 0, 3, 1000, 5, 1, 0, 41, 2]
    return np.array([base[k % len(base)] + (k // len(base)) for k in range(n)], np.uint32)


# ---- the shapes -------------------------------------------------------------------------------------------------------------------
SMALL = dict(H=5, W=7, N=320, Hc=64, B=67, seed=4)                  # 35 tiles: 3 words, the last one padded; 67 agents: no multiple of 64
SQUARE = dict(H=8, W=8, N=33, Hc=24, B=9, seed=11)                  # 64 tiles: 4 full words
BIG = dict(H=33, W=33, N=64, Hc=64, B=16, seed=21)                  # 1089 tiles: 69 words, more than a wavefront
F64 = dict(H=9, W=9, N=96, Hc=40, B=10, seed=5, T="Float64")
CALLS = dict(H=6, W=6, N=64, Hc=64, B=16, seed=7)
EDGE = dict(H=255, W=254, N=8, Hc=16, B=3, seed=51)                 # 64770 tiles, the most rcw_create takes (H W + 2 H = 65280): 4050 words,
                                                                    # 64 passes of the lane + 64 i loops, 15.8 KiB of LDS under reset_agent
SHAPES = dict(SMALL=SMALL, SQUARE=SQUARE, BIG=BIG, F64=F64, CALLS=CALLS, EDGE=EDGE)


def make_ref(c, render=True, **kw):
    return WB.WallBankRef(c["B"], c["seed"], c["H"], c["W"], c["N"], c["Hc"], T=np.float64 if c.get("T") == "Float64" else np.float32,
                          render=render, **kw)


def make_env(rcw, c, form=None, **kw):
    env = rcw.SingleRoomModule.SingleRoom(batch=c["B"], seed=c["seed"], T=c.get("T", "Float32"), auto_reset=True, num_directions=8,
                                          position_increment_wu=0.25, player_radius_wu=0.3, height_tile_map_tu=c["H"], width_tile_map_tu=c["W"],
                                          num_rays=c["N"], height_camera_view_pu=c["Hc"], **kw)
    if form is not None:
        env.set_step_form(form)
        assert env.step_form() == form
    return env


# ---- the two drivers --------------------------------------------------------------------------------------------------------------
class Recorder:
    def __init__(self, c, render=True, **kw):
        self.c, self.ref, self.lim, self.snaps = c, make_ref(c, render, **kw), None, []
        self.B = c["B"]
        self._snap()

    def _snap(self):
        s = self.ref.snapshot()
        if self.lim is not None:
            s.update(episode_steps=self.lim.episode_steps.copy(), truncated=self.lim.truncated.copy())
        s["bank"] = self.ref.bank is not None
        self.snaps.append(s)

    @property
    def events(self):
        return dict(self.ref.events, **(self.lim.events if self.lim is not None else {}), layouts_drawn=set(self.ref.layouts_drawn))

    def set_time_limit(self, L):
        self.lim = TL.TimeLimitRef(self.ref, L, self.ref.seed, True)
        self._snap()

    def set_wall_bank(self, walls, weights=None):
        self.ref.set_wall_bank(walls, weights)
        if self.lim is not None and walls is not None:
            self.lim.clear()
        self._snap()

    def set_weights(self, weights):
        self.ref.set_weights(weights)
        self._snap()

    def set_walls(self, walls, index=None, mask=None):
        self.ref.set_walls(walls, index, mask)
        if self.lim is not None:
            self.lim.clear(mask)
        self._snap()

    def step(self, actions):
        (self.lim or self.ref).step(actions)
        self._snap()

    def reset(self, mask=None, seed=None):
        self.ref.reset(mask, seed)
        if self.lim is not None:
            self.lim.seed = self.ref.seed
            self.lim.clear(mask)
        self._snap()

    def set_state(self, goal, pos, heading, mask=None):
        self.ref.set_state(goal, pos, heading, mask)
        if self.lim is not None:
            self.lim.clear(mask)
        self._snap()

    def state(self):
        """(walls (B, H, W), goal, position, heading) as they stand: what a scenario builds a set_state from"""
        s = self.snaps[-1]
        return np.stack([self.ref.walls_of(b) for b in range(self.B)]), s["goal"].copy(), s["position"].copy(), s["direction"].copy()


class Player:
    """the same calls on an engine, each compared with the recorded snapshot; trackers: objects with stepped(actions, where) and
    masked(mask, where), told after the comparison what the call was"""

    def __init__(self, rcw, env, snaps, name):
        self.rcw, self.env, self.snaps, self.name, self.k, self.trackers = rcw, env, snaps, name, 0, []
        self.B = env.batch
        self._check("fresh")

    def _check(self, where):
        s = self.snaps[self.k]
        where = f"{self.name}, call {self.k}: {where}"
        self.k += 1
        assert bool(self.env.wall_bank_info["layouts"]) == s["bank"], where
        WB.assert_equal(self.env, s, where)
        if "episode_steps" in s:
            np.testing.assert_array_equal(self.env.world.episode_steps, s["episode_steps"], err_msg=f"episode_steps {where}")
            np.testing.assert_array_equal(self.env.world.truncated.astype(np.uint8), s["truncated"], err_msg=f"truncated {where}")
        return where

    def finished(self):
        assert self.k == len(self.snaps), (self.k, len(self.snaps))

    def _masked(self, mask, where):
        where = self._check(where)
        for t in self.trackers:
            t.masked(mask, where)

    def set_time_limit(self, L):
        self.env.set_time_limit(L)
        self._check(f"set_time_limit({L})")

    def set_wall_bank(self, walls, weights=None):
        self.env.set_wall_bank(walls, weights)
        if walls is None:
            self._check("bank off")
        else:
            self._masked(None, "set_wall_bank")

    def set_weights(self, weights):
        self.env.set_wall_bank_weights(weights)
        self._check("set_wall_bank_weights")

    def set_walls(self, walls, index=None, mask=None):
        self.env.set_walls(walls, index, mask)
        self._masked(mask, "set_walls")

    def step(self, actions):
        self.rcw.act_(self.env, actions)
        where = self._check("step")
        for t in self.trackers:
            t.stepped(actions, where)

    def reset(self, mask=None, seed=None):
        self.rcw.reset_(self.env, mask, seed)
        self._masked(mask, "reset")

    def set_state(self, goal, pos, heading, mask=None):
        self.env.set_state(goal, pos, heading, mask)
        self._masked(mask, "set_state")

    def state(self):
        """the engine's own state, which the call before found equal to the reference's"""
        w = self.env.world
        return w.walls, w.goal_position.copy(), w.player_position_wu.copy(), w.player_direction_au.copy()


# ---- the scenarios ----------------------------------------------------------------------------------------------------------------
def rollout(d, bank, weights, limit, steps, seed):
    d.set_wall_bank(bank, weights)
    if limit:
        d.set_time_limit(limit)
    rng = np.random.default_rng(seed)
    for _ in range(steps):
        d.step(WR.draw_actions(rng, d.B))


def walk_into_the_goal(d, mask):
    """the masked agents are put on the first free tile of their map whose neighbour one row down is free too, facing it (heading 0 is
    +i), the goal on that neighbour; then everybody steps forward once: a quarter tile brings the player's radius of 0.3 over the goal
    tile's edge, the masked agents are done, and the next step restarts them.  On a large map under a short limit nobody arrives
    otherwise."""
    walls, goal, pos, heading = d.state()
    for b in np.flatnonzero(mask):
        free = ~walls[b]
        i, j = np.argwhere(free[:-1] & free[1:])[0]                          # 0-based; the goal on (i + 1, j)
        goal[b], pos[b], heading[b] = (i + 2, j + 1), (i + 0.5, j + 0.5), 0
    d.set_state(goal, pos, heading, mask)
    d.step(np.ones(d.B, np.uint8))


def small(d):
    """5 x 7, three layouts, limit 4, 30 steps: restarts every few steps"""
    rollout(d, three_layouts(5, 7), None, 4, 30, 5)


def square_one(d):
    """a bank of one layout: every draw is layout 0"""
    rollout(d, three_layouts(8, 8)[2:], None, 3, 10, 12)


def square_zero_weight(d):
    """two layouts, weights (0, 5): layout 0 is never drawn"""
    rollout(d, three_layouts(8, 8)[1:], np.array([0, 5], np.uint32), 3, 10, 13)


def big(d):
    """33 x 33, 130 layouts with ragged weights: the copy loop past 64 lanes, the binary search past 64 entries"""
    rollout(d, pillars_and_mazes(33, 33, 130, 300), ragged_weights(130), 3, 5, 22)
    two = np.zeros(130, np.uint32); two[64], two[129] = 1, 2                 # from here two layouts, both past entry 63: some are kept
    d.set_weights(two)
    rng = np.random.default_rng(23)
    for _ in range(7):
        d.step(WR.draw_actions(rng, d.B))


def edge(d):
    """255 x 254, the largest map a handle takes: three layouts (pillars, a maze, pillars), weights (1, 0, 3), limit 2, five steps — two
    agents walk into their goals — and a step that restarts them"""
    rollout(d, pillars_and_mazes(255, 254, 3, 500), np.array([1, 0, 3], np.uint32), 2, 5, 52)
    walk_into_the_goal(d, np.array([1, 0, 1], np.uint8))
    d.step(np.array([1, 2, 3], np.uint8))


def f64(d):
    """a Float64 handle, nine 9 x 9 mazes"""
    rollout(d, mazes(9, 9, 9, 40), None, 4, 14, 6)


def features(d):
    """what the feature tests play beside their trackers: 6 x 6, three layouts, limit 4"""
    rollout(d, three_layouts(6, 6), np.array([2, 1, 3], np.uint32), 4, 14, 9)


def calls(d):
    """the call rules: masked reset_ (new seed and same seed), masked set_state (layout and counter kept), new weights between steps, the
    bank off (walls kept, set_walls works again), the bank on again"""
    B, c = d.B, CALLS
    bank = three_layouts(6, 6)
    rng = np.random.default_rng(17)
    step = lambda n: [d.step(WR.draw_actions(rng, B)) for _ in range(n)]
    d.set_time_limit(5)
    d.set_wall_bank(bank, np.array([1, 1, 2], np.uint32))
    step(4)
    mask = np.zeros(B, np.uint8); mask[[0, 3, 4, 9, 15]] = 1
    d.reset(mask, seed=99)                                                   # a new seed: the masked agents draw layouts under it
    step(3)
    d.reset(mask[::-1].copy(), seed=99)                                      # the same seed, other agents
    step(2)
    # set_state: a goal and a pose on tiles free in all three layouts ((2,2) and (5,5) are), for every third agent
    m3 = np.zeros(B, np.uint8); m3[::3] = 1
    goal = np.tile(np.array([[5, 5]], np.int32), (B, 1))
    pos = np.tile(np.array([[1.5, 1.5]], np.float32), (B, 1))
    heading = (np.arange(B) % 8).astype(np.int32)
    d.set_state(goal, pos, heading, m3)
    step(2)
    d.set_weights(np.array([0, 0, 7], np.uint32))                            # from here every new episode is layout 2
    step(6)
    d.set_weights(None)
    step(3)
    d.set_wall_bank(None)                                                    # off: the walls stay, restarts keep them
    step(4)
    d.set_walls(bank[1], None, mask)                                         # ... and set_walls works again
    step(3)
    d.set_wall_bank(bank[:2], np.array([3, 1], np.uint32))                   # on again, another bank
    step(5)


SCENARIOS = dict(small=(small, SMALL), square_one=(square_one, SQUARE), square_zero_weight=(square_zero_weight, SQUARE), big=(big, BIG),
                 f64=(f64, F64), features=(features, CALLS), calls=(calls, CALLS), edge=(edge, EDGE))


@functools.lru_cache(maxsize=None)
def recorded(name, render=True, offset=0, batch=None):
    """the reference's run of a scenario, computed once: (snapshots, events)"""
    fn, c = SCENARIOS[name]
    c = dict(c, B=batch) if batch is not None else c
    rec = Recorder(c, render, agent_id_offset=offset)
    fn(rec)
    return rec.snaps, rec.events


def play(rcw, name, env, trackers=(), wrap=None):
    """the scenario on `env` against its recording; trackers(player) -> the feature trackers, made once the player has checked the fresh state"""
    fn, _ = SCENARIOS[name]
    snaps, events = recorded(name)
    p = Player(rcw, env, snaps, name)
    p.trackers = list(trackers)
    fn(p if wrap is None else wrap(p))                                       # (wrap: tests/deferred.py takes a note behind every call)
    p.finished()
    return events
