"""The caves' scenarios, written ONCE and run twice — test infrastructure, not a test.

The drivers and the shapes are tests/wall_bank_cases.py's and tests/wall_generator_cases.py's, by import: a Recorder (the reference alone,
tests/wall_caves_ref.py, under tests/time_limit_ref.py where the scenario sets a limit; a snapshot after every call) and a Player (an
engine: every call made on it and compared with the next snapshot byte for byte, then handed to the feature trackers).  What changes is the
reference they drive, the call `set_wall_caves`, and the comparison of wall_layout, which the engine serves while the CAVES are on.

Every scenario: 8 headings, a quarter tile a move, a player radius of 0.3, auto_reset, forward-heavy actions (walls_ref.draw_actions).
"""
import functools

import numpy as np

import wall_bank_cases as BC
import wall_caves_ref as WC
import wall_generator_cases as GC
import walls_ref as WR

# ---- the shapes ---------------------------------------------------------------------------------------------------------------------------
SQUARE = dict(H=8, W=8, N=32, Hc=64, B=67, seed=11)                 # 36 interior tiles; 67 agents: no multiple of 64; 32 x 64 pixels: both step forms
TIE = dict(H=7, W=9, N=32, Hc=24, B=5, seed=13)                     # 35 interior tiles; the level is chosen for its tie
TIE64 = dict(TIE, T="Float64")
MID = dict(H=16, W=16, N=32, Hc=24, B=8, seed=21)                   # 196 interior tiles: four a lane (the last: 4 lanes)
WIDE = dict(H=21, W=45, N=32, Hc=24, B=6, seed=31)                  # non-square: 19 x 43 = 817 tiles, t = i + H j and the planes' stride 19 differ
TINY = dict(H=5, W=5, N=16, Hc=16, B=3, seed=2)                     # 9 interior tiles: fewer than a wavefront has lanes
LEVELS = dict(H=9, W=12, N=32, Hc=24, B=67, seed=13)                # 67 agents on three levels
CALLS = dict(BC.CALLS, H=8, W=8)                                    # 16 agents x 64 rays
EDGE = dict(H=66, W=66, N=8, Hc=16, B=33, seed=41)                  # the bound: 4096 interior tiles, 64 a lane, rows wider than a wavefront
SHAPES = dict(SQUARE=SQUARE, TIE=TIE, TIE64=TIE64, MID=MID, WIDE=WIDE, TINY=TINY, LEVELS=LEVELS, CALLS=CALLS, EDGE=EDGE)
# what tests/test_wall_caves_spec.py finds, with the restatement, and pins: a level of 0 .. 1499 under level seed 9 at 7 x 9, fill 0.35,
# smooth 0, whose two largest regions tie at or above `need` (the first such level), and per shape the level of 0 .. 149 under level seed 9
# whose cave at the defaults takes the labelling restatement the most rounds, with that count
HARD_LEVEL_SEED = 9
TIE_FILL, TIE_SMOOTH = 0.35, 0
TIE_LEVEL = 97
ALL_SHAPES = [(5, 7), (8, 8), (9, 12), (16, 16), (21, 45), (32, 32), (66, 66)]
HARD_LEVELS = {(5, 7): (9, 2), (8, 8): (0, 2), (9, 12): (58, 3), (16, 16): (0, 3), (21, 45): (140, 4), (32, 32): (0, 4), (66, 66): (0, 4)}   # (level, rounds)


def make_ref(c, render=True, **kw):
    return WC.WallCavesRef(c["B"], c["seed"], c["H"], c["W"], c["N"], c["Hc"], T=np.float64 if c.get("T") == "Float64" else np.float32,
                           render=render, **kw)


make_env = BC.make_env


# ---- the two drivers ----------------------------------------------------------------------------------------------------------------------
class Recorder(GC.Recorder):
    def __init__(self, c, render=True, **kw):
        self.c, self.ref, self.lim, self.snaps, self.render = c, make_ref(c, render, **kw), None, [], render
        self.B = c["B"]
        self._snap()

    def _snap(self):
        s = self.ref.snapshot()
        if self.lim is not None:
            s.update(episode_steps=self.lim.episode_steps.copy(), truncated=self.lim.truncated.copy())
        s["caves"], s["rendered"] = self.ref.gen is not None, self.render
        self.snaps.append(s)

    @property
    def events(self):
        return dict(self.ref.events, **(self.lim.events if self.lim is not None else {}), keys_made=set(self.ref.keys_made))

    def set_wall_caves(self, fill=WC.DEFAULT_FILL, smooth=WC.DEFAULT_SMOOTH, levels=0, first_level=0, level_seed=0):
        self.ref.set_wall_caves(fill, smooth, levels, first_level, level_seed)
        if self.lim is not None and fill is not None:
            self.lim.clear()
        self._snap()


class Player(GC.Player):
    def _check(self, where):
        s = self.snaps[self.k]
        where = f"{self.name}, call {self.k}: {where}"
        self.k += 1
        assert self.env.wall_caves_info["enabled"] == s["caves"] and not self.env.wall_bank_info["layouts"], where
        assert self.env.wall_generator_info["enabled"] == s["caves"] and self.env.wall_generator_info["loops"] == 0, where
        if s["rendered"]:
            WC.assert_equal(self.env, s, where)
        else:
            GC.assert_state_equal(self.env, s, where)
            if s["caves"]:
                np.testing.assert_array_equal(self.env.wall_layout.numpy(), s["wall_layout"], err_msg=f"wall_layout {where}")
        if "episode_steps" in s:
            np.testing.assert_array_equal(self.env.world.episode_steps, s["episode_steps"], err_msg=f"episode_steps {where}")
            np.testing.assert_array_equal(self.env.world.truncated.astype(np.uint8), s["truncated"], err_msg=f"truncated {where}")
        return where

    def set_wall_caves(self, fill=WC.DEFAULT_FILL, smooth=WC.DEFAULT_SMOOTH, levels=0, first_level=0, level_seed=0):
        self.env.set_wall_caves(fill, smooth, levels, first_level, level_seed)
        if fill is None:
            self._check("caves off")
        else:
            self._masked(None, "set_wall_caves")


# ---- the scenarios ------------------------------------------------------------------------------------------------------------------------
def rollout(d, caves, limit, steps, seed):
    d.set_wall_caves(**caves)
    if limit:
        d.set_time_limit(limit)
    rng = np.random.default_rng(seed)
    for _ in range(steps):
        d.step(WR.draw_actions(rng, d.B))


walk_into_the_goal = BC.walk_into_the_goal


def walk_and_step(d, every, seed, steps=3):
    walk_into_the_goal(d, (np.arange(d.B) % every == 0).astype(np.uint8))
    rng = np.random.default_rng(seed)
    for _ in range(steps):
        d.step(WR.draw_actions(rng, d.B))


def square(d):
    """8 x 8, 67 agents, limit 4, the defaults: about a quarter of the layouts are the fallback's mazes"""
    rollout(d, dict(), 4, 10, 12)
    walk_and_step(d, 3, 13)


def tie(d):
    """7 x 9, one level for every agent: a cave whose two largest regions tie"""
    rollout(d, dict(fill=TIE_FILL, smooth=TIE_SMOOTH, levels=1, first_level=TIE_LEVEL, level_seed=HARD_LEVEL_SEED), 3, 5, 14)
    walk_and_step(d, 2, 15)


def mid(d):
    """16 x 16 at the defaults"""
    rollout(d, dict(), 3, 5, 22)
    walk_and_step(d, 2, 23)


def wide(d):
    """21 x 45, smoothed eight times"""
    rollout(d, dict(smooth=8), 3, 4, 32)
    walk_and_step(d, 3, 33)


def empty(d):
    """5 x 5, fill 0: the empty room, 9 free tiles, never a fallback"""
    rollout(d, dict(fill=0, smooth=0), 3, 6, 42)
    walk_and_step(d, 2, 44)


def full(d):
    """5 x 5, fill 2^32 - 1: all wall, always the fallback's maze"""
    rollout(d, dict(fill=0xFFFFFFFF, smooth=1), 3, 6, 43)
    walk_and_step(d, 2, 45)


def levels(d):
    """three levels 43, 44, 45 under level seed 9: 67 agents share three layouts — 43 and 45 fall back to their mazes at 9 x 12, 44 is a cave"""
    rollout(d, dict(levels=3, first_level=43, level_seed=9), 4, 8, 14)


def features(d):
    """what the feature tests play beside their trackers: 8 x 8, 16 agents, limit 4"""
    rollout(d, dict(), 4, 10, 9)
    walk_and_step(d, 3, 10, 2)


def calls(d):
    """the call rules: masked reset_ (new seed and same seed), masked set_state (cave and counter kept), caves off (walls kept, set_walls
    works again), on again with levels, and with other parameters over the running ones"""
    B = d.B
    rng = np.random.default_rng(17)
    step = lambda n: [d.step(WR.draw_actions(rng, B)) for _ in range(n)]
    d.set_time_limit(5)
    d.set_wall_caves()
    step(3)
    mask = np.zeros(B, np.uint8); mask[[0, 3, 4, 9, 15]] = 1
    d.reset(mask, seed=99)                                                   # a new seed: the masked agents make caves under it
    step(2)
    d.reset(mask[::-1].copy(), seed=99)                                      # the same seed, other agents
    step(2)
    walk_into_the_goal(d, (np.arange(B) % 3 == 0).astype(np.uint8))          # a masked set_state: the layouts and the counters stay
    step(4)
    d.set_wall_caves(None)                                                   # off: the walls stay, restarts keep them
    step(3)
    ring = np.ones((8, 8), bool); ring[1:-1, 1:-1] = False
    d.set_walls(ring, None, mask)                                            # ... and set_walls works again
    step(2)
    d.set_wall_caves(fill=0.45, smooth=1, levels=2, first_level=5, level_seed=3)   # on again: two levels
    step(3)
    d.set_wall_caves(fill=0.2, smooth=0)                                     # other parameters over the running caves
    step(3)


SCENARIOS = dict(square=(square, SQUARE), tie=(tie, TIE), tie64=(tie, TIE64), mid=(mid, MID), wide=(wide, WIDE), empty=(empty, TINY), full=(full, TINY),
                 levels=(levels, LEVELS), features=(features, CALLS), calls=(calls, CALLS))
MIXED = ("square", "levels", "features", "calls")                            # scenarios that must reach caves AND fallbacks


@functools.lru_cache(maxsize=None)
def recorded(name, render=True, offset=0, batch=None):
    """the reference's run of a scenario, computed once: (snapshots, events)"""
    fn, c = SCENARIOS[name]
    c = dict(c, B=batch) if batch is not None else c
    rec = Recorder(c, render, agent_id_offset=offset)
    fn(rec)
    return rec.snaps, rec.events


def play(rcw, name, env, trackers=(), wrap=None):
    """the scenario on `env` against its recording; trackers: the feature trackers, made once the engine exists"""
    fn, _ = SCENARIOS[name]
    snaps, events = recorded(name)
    p = Player(rcw, env, snaps, name)
    p.trackers = list(trackers)
    fn(p if wrap is None else wrap(p))                                       # (wrap: tests/deferred.py takes a note behind every call)
    p.finished()
    return events
