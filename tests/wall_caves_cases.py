"""The caves' scenarios, written ONCE and run twice — test infrastructure, not a test.

The drivers are tests/wall_family.py's, by its row `caves`: a Recorder (the reference alone: wall_family.WallFamilyRef over
wall_caves_ref.cave) and a Player (an engine against the recording), with `set_wall_caves` as their own call.  This module is the caves'
shapes, their pinned levels and their scenarios.

Every scenario: 8 headings, a quarter tile a move, a player radius of 0.3, auto_reset, forward-heavy actions (walls_ref.draw_actions).
"""
import functools

import numpy as np

import wall_bank_cases as BC
import wall_caves_ref as WC
import wall_family as WF
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


make_ref = functools.partial(WF.make_ref, "caves")
make_env = WF.make_env
Recorder, Player = WF.drivers("caves")                                       # the shared drivers with `set_wall_caves` as their own call


# ---- the scenarios ------------------------------------------------------------------------------------------------------------------------
rollout = functools.partial(WF.rollout, "caves")
walk_into_the_goal = WF.walk_into_the_goal
walk_and_step = WF.walk_and_step


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


recorded = functools.partial(WF.recorded, "caves")                                  # (name, render=True, offset=0, batch=None) -> (snapshots, events), cached
play = functools.partial(WF.play, "caves")                                          # (rcw, name, env, trackers=(), wrap=None) -> events


# ---- what tests/test_gpu_wall_families.py plays of this family: the arguments of the tests every family has ------------------------------------
ROLLOUTS = [("square", "two-launches"), ("square", "one-launch"), ("tie", None), ("tie64", None), ("mid", None), ("wide", None), ("empty", None),
            ("full", None), ("levels", None), ("calls", "two-launches"), ("calls", "one-launch")]
REPLAYED = (dict(LEVELS, B=21), (dict(fill=0.42, smooth=1), dict(levels=5, first_level=3, level_seed=8)))
BESIDE_A_PLAIN_HANDLE = dict()
UNTOUCHED = dict(levels=3, first_level=1, level_seed=2)
CAPTURED = (dict(CALLS, B=12), dict(fill=0.40, smooth=2))
SHARDED = (12, dict(fill=0.42, smooth=2, levels=6, first_level=40, level_seed=9), (0.3, 1))    # (the map's width, the install, other parameters without levels)
REFUSED_MAPS = [(4, 9, ValueError, "at least 5 x 5"), (9, 4, ValueError, "at least 5 x 5"), (67, 66, "unsupported", "at most 4096 interior tiles")]
NAMED = {(67, 66): ("66 x 66",)}                                                # 65 x 64 = 4160 interior tiles: the message names the bound
FUZZ = ("caves", "wall caves:", ("step", "reset", "masked_reset", "set_state", "arrive", "off_and_on", "episode_starts", "fallbacks", "caves_kept", "goal_redraws",
                                 "restarts_after_done", "restarts_after_truncation", "one_launch_steps", "two_launch_steps", "non_square", "with_levels", "smoothed",
                                 "tiles_past_64"))


def reached(events, name=None):
    """what the reference's counts must show of a run (of scenario `name`) beyond restarts: caves AND fallbacks, by the reference's own count"""
    if name is None or name in MIXED:
        assert 0 < events["fallbacks"] < events["episode_starts"]


def check_rollout(rcw, env, name):
    """what holds of the engine behind scenario `name`"""
    c = SCENARIOS[name][1]
    walls, layout = env.world.walls, env.wall_layout.numpy()
    if name == "tie64":
        assert env.world.player_position_wu.dtype == np.float64
    if name in ("tie", "tie64"):
        # the two largest regions of generation 0 tie: every agent holds the cave of the one with the smaller tile index
        g = WC.smoothed(WF.level_key(HARD_LEVEL_SEED, TIE_LEVEL), 7, 9, WC.fill_word(TIE_FILL), TIE_SMOOTH)
        first, second = sorted(WC.regions(g), key=lambda r: (-len(r), r[0]))[:2]
        assert len(first) == len(second) >= WC.need(7, 9) and first[0] < second[0]
        for a in range(env.batch):
            assert sorted(int(i + 7 * j) for i, j in np.argwhere(~walls[a])) == first
        assert (layout == TIE_LEVEL).all()
    elif name == "levels":
        assert set(layout.tolist()) == {43, 44, 45} and min(np.bincount(layout - 43)) > 5
        fell = {}
        for level in (43, 44, 45):                                            # every level held by several agents, one layout a level
            held = walls[layout == level]
            assert (held == held[0]).all()
            want, fell[level] = rcw.layouts.generated_cave(rcw.layouts.generated_maze_key(0, 0, 0, 1, level, 9)[0], c["H"], c["W"], return_fell_back=True)
            np.testing.assert_array_equal(held[0], want)
        assert fell == {43: True, 44: False, 45: True}
    elif name == "empty":
        assert (layout == -1).all() and ((~walls).sum(axis=(1, 2)) == 9).all()
    elif name == "full":
        assert (layout == -1).all() and ((~walls).sum(axis=(1, 2)) == 7).all()
    else:
        assert (layout == -1).all()
