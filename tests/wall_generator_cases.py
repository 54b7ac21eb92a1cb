"""The wall generator's scenarios, written ONCE and run twice — test infrastructure, not a test.

The drivers are tests/wall_family.py's, by its row `generator`: a Recorder (the reference alone: wall_family.WallFamilyRef over
wall_generator_ref.maze) and a Player (an engine against the recording), with `set_wall_generator` as their own call; the bank's shapes by
import.  This module is the generator's shapes, its pinned levels and its scenarios.  A Recorder made with render=False records no frames;
its Player compares everything but the column descriptors and the camera view (`huge`, 65 x 65, is never rendered: UNRENDERED).

Every scenario: 8 headings, a quarter tile a move, a player radius of 0.3, auto_reset, forward-heavy actions (walls_ref.draw_actions).
"""
import functools

import numpy as np

import wall_bank_cases as BC
import wall_family as WF
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


make_ref = functools.partial(WF.make_ref, "generator")
make_env = WF.make_env
Recorder, Player = WF.drivers("generator")                                       # the shared drivers with `set_wall_generator` as their own call


# ---- the scenarios ------------------------------------------------------------------------------------------------------------------------
rollout = functools.partial(WF.rollout, "generator")
walk_into_the_goal = WF.walk_into_the_goal


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


recorded = functools.partial(WF.recorded, "generator")                                  # (name, render=True, offset=0, batch=None) -> (snapshots, events), cached
play = functools.partial(WF.play, "generator")                                          # (rcw, name, env, trackers=(), wrap=None) -> events


# ---- what tests/test_gpu_wall_families.py plays of this family: the arguments of the tests every family has ------------------------------------
ROLLOUTS = [("small", "two-launches"), ("small", "one-launch"), ("square", None), ("big", "two-launches"), ("big", "one-launch"), ("wide", None),
            ("huge", None), ("f64", None), ("levels", None), ("calls", "two-launches"), ("calls", "one-launch"),
            ("edge", "two-launches"), ("edge_rows64", "one-launch"), ("edge_even", None), ("thin", None), ("tall", None), ("thin_even", None)]
REPLAYED = (dict(LEVELS, B=21, H=9, W=11), (dict(loops=0.25), dict(loops=0.25, levels=5, first_level=3, level_seed=8)))
BESIDE_A_PLAIN_HANDLE = dict(loops=0.5)
UNTOUCHED = dict(levels=3, first_level=1, level_seed=2)
CAPTURED = (dict(CALLS, B=12, H=7, W=9), dict(loops=0.25, levels=0))
SHARDED = (9, dict(loops=0.25, levels=6, first_level=10, level_seed=4), (0.0,))     # (the map's width, the install, other parameters without levels)
REFUSED_MAPS = [(4, 9, ValueError, "at least 5 x 5"), (9, 4, ValueError, "at least 5 x 5"), (131, 129, "unsupported", "at most 4096 cells")]
NAMED = {(131, 129): ("129 x 129",)}                                            # 65 x 64 = 4160 cells: the message names the bound
FUZZ = ("gen", "wall generator:", ("step", "reset", "masked_reset", "set_state", "off_and_on", "episode_starts", "goal_redraws", "restarts_after_done",
                                   "restarts_after_truncation", "one_launch_steps", "two_launch_steps", "even_sizes", "with_levels", "with_loops", "cells_past_64"))


def reached(events, name=None):
    """what the reference's counts must show of a run (of scenario `name`) beyond restarts: nothing of the generator's own"""


def check_rollout(rcw, env, name):
    """what holds of the engine behind scenario `name`"""
    c = SCENARIOS[name][1]
    if name == "f64":
        assert env.world.player_position_wu.dtype == np.float64
    if name == "big":
        assert env.world.tile_map_chunks.shape[1] * 2 > 64                    # more tile-map words than a wavefront has lanes
    if name == "huge":
        assert WG.grid(c["H"], c["W"])[2] == 1024
    if name in AT_THE_BOUND:
        assert WG.grid(c["H"], c["W"])[2] == 4096 == WG.MAX_CELLS            # the bound itself, not 4095
        assert env.world.tile_map_chunks.shape[1] * 2 == WORDS[name]          # (a chunk is two words)
    if name == "levels":
        layout, walls = env.wall_layout.numpy(), env.world.walls
        assert set(layout.tolist()) == {40, 41, 42} and min(np.bincount(layout - 40)) > 5
        for level in (40, 41, 42):                                            # every level held by several agents, one maze a level
            held = walls[layout == level]
            assert (held == held[0]).all()
            np.testing.assert_array_equal(held[0], rcw.layouts.generated_maze(rcw.layouts.generated_maze_key(0, 0, 0, 1, level, 9)[0], c["H"], c["W"]))
    else:
        assert (env.wall_layout.numpy() == -1).all()
