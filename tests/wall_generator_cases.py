"""The wall generator's scenarios, written ONCE and run twice — test infrastructure, not a test.

The drivers and the shapes are tests/wall_bank_cases.py's, by import: a Recorder (the reference alone, tests/wall_generator_ref.py, under
tests/time_limit_ref.py where the scenario sets a limit; a snapshot after every call) and a Player (an engine: every call made on it and
compared with the next snapshot byte for byte, then handed to the feature trackers).  What changes is the reference they drive, the call
`set_wall_generator`, and the comparison of wall_layout, which the engine serves while the GENERATOR is on.  A Recorder made with
render=False records no frames; its Player compares everything but the column descriptors and the camera view (`huge`: 65 x 65).

Every scenario: 8 headings, a quarter tile a move, a player radius of 0.3, auto_reset, forward-heavy actions (walls_ref.draw_actions).
"""
import functools

import numpy as np

import wall_bank_cases as BC
import wall_generator_ref as WG
import walls_ref as WR

# ---- the shapes: the bank's, and three of the generator's own ---------------------------------------------------------------------------
SMALL, SQUARE, BIG, F64, CALLS = BC.SMALL, BC.SQUARE, BC.BIG, BC.F64, BC.CALLS
WIDE = dict(H=21, W=45, N=32, Hc=24, B=8, seed=31)                  # non-square: 10 x 22 = 220 cells, four cells a lane (the last: 28 lanes)
HUGE = dict(H=65, W=65, N=16, Hc=24, B=4, seed=41)                  # 1024 cells: 16 a lane, 265 words
LEVELS = dict(H=7, W=9, N=32, Hc=24, B=67, seed=13)                 # 3 x 4 cells; 67 agents on three levels
# the size bound, 4096 cells (64 a lane, 48 KiB of slots and labels), on every kind of map that reaches it
EDGE = dict(HUGE, H=129, W=129)                                     # 64 x 64 cells, 1042 words
EDGE_ROWS64 = dict(EDGE, Hc=64)                                     # ... with the fewest camera rows the one-launch step takes (24 rows: refused)
EDGE_EVEN = dict(HUGE, H=130, W=130)                                # 64 x 64 still: the last interior row and column stay wall; 1058 words
THIN = dict(HUGE, H=5, W=4097)                                      # 2 x 2048 cells, 1282 words
TALL = dict(HUGE, H=4097, W=5)                                      # 2048 x 2 cells: nj == 2
THIN_EVEN = dict(HUGE, H=6, W=4098)                                 # 2 x 2048 still; 1538 words: the largest LDS request the launch makes
SHAPES = dict(BC.SHAPES, WIDE=WIDE, HUGE=HUGE, LEVELS=LEVELS, EDGE=EDGE, EDGE_ROWS64=EDGE_ROWS64, EDGE_EVEN=EDGE_EVEN, THIN=THIN, TALL=TALL, THIN_EVEN=THIN_EVEN)
# the level of 0 .. 149 under HARD_LEVEL_SEED whose maze takes the kernel's algorithm the most rounds, then the deepest hook chain
# (wall_generator_ref.boruvka; tests/test_wall_generator_spec.py makes the search), and the rounds the GPU test demands of it from the model
HARD_LEVEL_SEED = 9
HARD_LEVELS = {(129, 129): 32, (5, 4097): 31, (4097, 5): 141, (33, 33): 1}
HARD_ROUNDS = {(129, 129): 7, (5, 4097): 8, (4097, 5): 8, (33, 33): 5}
WORDS = dict(edge=1042, edge_rows64=1042, edge_even=1058, thin=1282, tall=1282, thin_even=1538)      # 2 (ceil(H W / 16) rounded up to even)


def make_ref(c, render=True, **kw):
    return WG.WallGeneratorRef(c["B"], c["seed"], c["H"], c["W"], c["N"], c["Hc"], T=np.float64 if c.get("T") == "Float64" else np.float32,
                               render=render, **kw)


make_env = BC.make_env


# ---- the two drivers ----------------------------------------------------------------------------------------------------------------------
class Recorder(BC.Recorder):
    def __init__(self, c, render=True, **kw):
        self.c, self.ref, self.lim, self.snaps, self.render = c, make_ref(c, render, **kw), None, [], render
        self.B = c["B"]
        self._snap()

    def _snap(self):
        s = self.ref.snapshot()
        if self.lim is not None:
            s.update(episode_steps=self.lim.episode_steps.copy(), truncated=self.lim.truncated.copy())
        s["generator"], s["rendered"] = self.ref.gen is not None, self.render
        self.snaps.append(s)

    @property
    def events(self):
        return dict(self.ref.events, **(self.lim.events if self.lim is not None else {}), mazes_made=set(self.ref.mazes_made))

    def state(self):
        """(walls (B, H, W), goal, position, heading) as they stand: what a scenario builds a set_state from"""
        s = self.snaps[-1]
        return np.stack([self.ref.walls_of(b) for b in range(self.B)]), s["goal"].copy(), s["position"].copy(), s["direction"].copy()

    def set_wall_generator(self, loops=0.0, levels=0, first_level=0, level_seed=0):
        self.ref.set_wall_generator(loops, levels, first_level, level_seed)
        if self.lim is not None and loops is not None:
            self.lim.clear()
        self._snap()


def assert_state_equal(env, r, where):
    """walls_ref.assert_equal without the frames (a recording made with render=False has none)"""
    w = env.world
    pos = w.player_position_wu
    bits = np.uint64 if pos.dtype == np.float64 else np.uint32
    assert pos.dtype == r["position"].dtype
    for got, key in ((w.status, "status"), (w.episode, "episode"), (w.goal_position, "goal"), (pos.view(bits), None), (w.player_direction_au, "direction"),
                     (w.reward, "reward"), (w.done.astype(np.uint8), "done"), (w.tile_map_chunks, "tile_map_chunks")):
        want = r["position"].view(bits) if key is None else r[key]
        np.testing.assert_array_equal(got, want, err_msg=f"{key or 'position'} {where}")


class Player(BC.Player):
    def _check(self, where):
        s = self.snaps[self.k]
        where = f"{self.name}, call {self.k}: {where}"
        self.k += 1
        assert self.env.wall_generator_info["enabled"] == s["generator"] and not self.env.wall_bank_info["layouts"], where
        if s["rendered"]:
            WG.assert_equal(self.env, s, where)
        else:
            assert_state_equal(self.env, s, where)
            if s["generator"]:
                np.testing.assert_array_equal(self.env.wall_layout.numpy(), s["wall_layout"], err_msg=f"wall_layout {where}")
        if "episode_steps" in s:
            np.testing.assert_array_equal(self.env.world.episode_steps, s["episode_steps"], err_msg=f"episode_steps {where}")
            np.testing.assert_array_equal(self.env.world.truncated.astype(np.uint8), s["truncated"], err_msg=f"truncated {where}")
        return where

    def state(self):
        """the engine's own state, which the call before found equal to the reference's"""
        w = self.env.world
        return w.walls, w.goal_position.copy(), w.player_position_wu.copy(), w.player_direction_au.copy()

    def set_wall_generator(self, loops=0.0, levels=0, first_level=0, level_seed=0):
        self.env.set_wall_generator(loops, levels, first_level, level_seed)
        if loops is None:
            self._check("generator off")
        else:
            self._masked(None, "set_wall_generator")


# ---- the scenarios ------------------------------------------------------------------------------------------------------------------------
def rollout(d, gen, limit, steps, seed):
    d.set_wall_generator(**gen)
    if limit:
        d.set_time_limit(limit)
    rng = np.random.default_rng(seed)
    for _ in range(steps):
        d.step(WR.draw_actions(rng, d.B))


walk_into_the_goal = BC.walk_into_the_goal


def small(d):
    """5 x 7 (2 x 3 cells, 15 spanning trees), limit 4, 30 steps: restarts every few steps"""
    rollout(d, dict(), 4, 30, 5)


def square(d):
    """8 x 8: even sizes, 9 cells, the last interior row and column stay wall; a quarter of the non-tree edges opened"""
    rollout(d, dict(loops=0.25), 3, 12, 12)


def big(d):
    """33 x 33: 256 cells, four a lane, 69 words"""
    rollout(d, dict(loops=0.05), 3, 4, 22)
    walk_into_the_goal(d, (np.arange(d.B) % 2).astype(np.uint8))
    rng = np.random.default_rng(23)
    for _ in range(4):
        d.step(WR.draw_actions(rng, d.B))


def wide(d):
    """21 x 45: non-square, 220 cells"""
    rollout(d, dict(), 3, 4, 32)
    walk_into_the_goal(d, (np.arange(d.B) % 3 == 0).astype(np.uint8))
    rng = np.random.default_rng(33)
    for _ in range(4):
        d.step(WR.draw_actions(rng, d.B))


def huge(d):
    """65 x 65: 1024 cells; the install, four steps under limit 2 — two agents walk into their goals — and a reset with a new seed (recorded
    without frames)"""
    rollout(d, dict(loops=0.1), 2, 2, 42)
    walk_into_the_goal(d, np.array([1, 0, 1, 0], np.uint8))
    d.step(np.array([1, 2, 3, 4], np.uint8))
    d.reset(None, 77)


def f64(d):
    """a Float64 handle, 9 x 9"""
    rollout(d, dict(loops=0.5), 4, 14, 6)


def levels(d):
    """three levels 40, 41, 42 under level seed 9: 67 agents share three mazes"""
    rollout(d, dict(levels=3, first_level=40, level_seed=9), 4, 10, 14)


def features(d):
    """what the feature tests play beside their trackers: 6 x 6 (4 cells), limit 4"""
    rollout(d, dict(loops=0.5), 4, 14, 9)


def calls(d):
    """the call rules: masked reset_ (new seed and same seed), masked set_state (maze and counter kept), the generator off (walls kept,
    set_walls works again), on again with levels, and with other parameters over the running one"""
    B = d.B
    rng = np.random.default_rng(17)
    step = lambda n: [d.step(WR.draw_actions(rng, B)) for _ in range(n)]
    d.set_time_limit(5)
    d.set_wall_generator()
    step(4)
    mask = np.zeros(B, np.uint8); mask[[0, 3, 4, 9, 15]] = 1
    d.reset(mask, seed=99)                                                   # a new seed: the masked agents make mazes under it
    step(3)
    d.reset(mask[::-1].copy(), seed=99)                                      # the same seed, other agents
    step(2)
    # set_state: a goal and a pose on cells (free in every 6 x 6 maze: tiles (2,2), (4,4) 1-based), for every third agent
    m3 = np.zeros(B, np.uint8); m3[::3] = 1
    goal = np.tile(np.array([[4, 4]], np.int32), (B, 1))
    pos = np.tile(np.array([[1.5, 1.5]], np.float32), (B, 1))
    heading = (np.arange(B) % 8).astype(np.int32)
    d.set_state(goal, pos, heading, m3)
    step(6)
    d.set_wall_generator(None)                                               # off: the walls stay, restarts keep them
    step(4)
    ring = np.ones((6, 6), bool); ring[1:-1, 1:-1] = False
    d.set_walls(ring, None, mask)                                            # ... and set_walls works again
    step(3)
    d.set_wall_generator(loops=1.0, levels=2, first_level=5, level_seed=3)   # on again: two levels, every edge open
    step(4)
    d.set_wall_generator(loops=0.0)                                          # other parameters over the running generator
    step(4)


SCENARIOS = dict(small=(small, SMALL), square=(square, SQUARE), big=(big, BIG), wide=(wide, WIDE), huge=(huge, HUGE), f64=(f64, F64),
                 levels=(levels, LEVELS), features=(features, CALLS), calls=(calls, CALLS),
                 edge=(huge, EDGE), edge_rows64=(huge, EDGE_ROWS64), edge_even=(huge, EDGE_EVEN), thin=(huge, THIN), tall=(huge, TALL), thin_even=(huge, THIN_EVEN))
AT_THE_BOUND = ("edge", "edge_rows64", "edge_even", "thin", "tall", "thin_even")            # `huge`'s script at 4096 cells
UNRENDERED = ("huge",)


@functools.lru_cache(maxsize=None)
def recorded(name, render=True, offset=0, batch=None):
    """the reference's run of a scenario, computed once: (snapshots, events)"""
    fn, c = SCENARIOS[name]
    c = dict(c, B=batch) if batch is not None else c
    rec = Recorder(c, render and name not in UNRENDERED, agent_id_offset=offset)
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
