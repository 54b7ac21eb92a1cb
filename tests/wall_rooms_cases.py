"""The rooms' scenarios, written ONCE and run twice — test infrastructure, not a test.

The drivers are tests/wall_family.py's, by its row `rooms`: a Recorder (the reference alone: wall_family.WallFamilyRef over
wall_rooms_ref.rooms) and a Player (an engine against the recording), with `set_wall_rooms` as their own call.  This module is the rooms'
shapes, their pinned levels and their scenarios.

Every scenario: 8 headings, a quarter tile a move, a player radius of 0.3, auto_reset, forward-heavy actions (walls_ref.draw_actions).
"""
import functools

import numpy as np

import wall_bank_cases as BC
import wall_family as WF
import walls_ref as WR

ALL = 0xFFFFFFFF
# ---- the shapes ---------------------------------------------------------------------------------------------------------------------------
TINY = dict(H=5, W=5, N=32, Hc=64, B=67, seed=2)                    # 9 interior tiles, four layouts at room 1; 67 agents: no multiple of 64; both step forms
SQUARE = dict(H=8, W=8, N=32, Hc=24, B=9, seed=11)                  # an even side: the last interior line is even
SQUARE64 = dict(SQUARE, T="Float64")
DOORS = dict(H=9, W=12, N=32, Hc=24, B=8, seed=13)                  # two doors a wall
WIDE = dict(H=21, W=45, N=32, Hc=24, B=6, seed=31)                  # non-square: t = i + H j; more chambers than a few lanes hold
LEVELS = dict(H=9, W=12, N=32, Hc=24, B=67, seed=13)                # 67 agents on three levels
CALLS = dict(BC.CALLS, H=8, W=8)                                    # 16 agents x 64 rays
EDGE = dict(H=66, W=66, N=8, Hc=16, B=33, seed=41)                  # rounds wider than a wavefront: a lane takes several chambers
SHAPES = dict(TINY=TINY, SQUARE=SQUARE, SQUARE64=SQUARE64, DOORS=DOORS, WIDE=WIDE, LEVELS=LEVELS, CALLS=CALLS, EDGE=EDGE)
# what tests/test_wall_rooms_spec.py finds, with the restatement, and pins: of the levels 0 .. 149 under level seed 9 at 66 x 66 with
# room 1, stop 0, doors 0, the one whose widest round handles the most chambers (level, chambers) and the one with the most rounds
# (level, rounds); the first of equals
HARD_LEVEL_SEED = 9
ALL_SHAPES = [(5, 7), (8, 8), (9, 12), (16, 16), (21, 45), (32, 32), (66, 66)]
PARAMETERS = [(1, 0.0, 0.0), (2, 0.0, 0.0), (2, 0.25, 0.5), (3, 0.5, 0.0)]     # (room, stop, doors)
WIDEST_LEVEL = (111, 166)                                           # (level, the chambers of its widest round)
DEEPEST_LEVEL = (48, 25)                                            # (level, rounds)


make_ref = functools.partial(WF.make_ref, "rooms")
make_env = WF.make_env
Recorder, Player = WF.drivers("rooms")                                       # the shared drivers with `set_wall_rooms` as their own call


# ---- the scenarios ------------------------------------------------------------------------------------------------------------------------
rollout = functools.partial(WF.rollout, "rooms")
walk_into_the_goal = WF.walk_into_the_goal
walk_and_step = WF.walk_and_step


def tiny(d):
    """5 x 5, room 1, 67 agents, limit 4: one wall with one door, the four layouts"""
    rollout(d, dict(room=1, stop=0, doors=0), 4, 10, 12)
    walk_and_step(d, 3, 13)


def square(d):
    """8 x 8 at the defaults"""
    rollout(d, dict(), 3, 6, 22)
    walk_and_step(d, 2, 23)


def doors(d):
    """9 x 12, room 1, never a stop, a second door drawn for every wall"""
    rollout(d, dict(room=1, stop=0, doors=ALL), 3, 5, 14)
    walk_and_step(d, 2, 15)


def wide(d):
    """21 x 45, room 2, stop 1/4, doors 1/2"""
    rollout(d, dict(room=2, stop=0.25, doors=0.5), 3, 4, 32)
    walk_and_step(d, 3, 33)


def levels(d):
    """three levels 43, 44, 45 under level seed 9: 67 agents share three layouts"""
    rollout(d, dict(room=1, levels=3, first_level=43, level_seed=9), 4, 8, 14)


def features(d):
    """what the feature tests play beside their trackers: 8 x 8, 16 agents, limit 4"""
    rollout(d, dict(room=1), 4, 10, 9)
    walk_and_step(d, 3, 10, 2)


def calls(d):
    """the call rules: masked reset_ (new seed and same seed), masked set_state (rooms and counter kept), rooms off (walls kept, set_walls
    works again), on again with levels, and with other parameters over the running ones"""
    B = d.B
    rng = np.random.default_rng(17)
    step = lambda n: [d.step(WR.draw_actions(rng, B)) for _ in range(n)]
    d.set_time_limit(5)
    d.set_wall_rooms()
    step(3)
    mask = np.zeros(B, np.uint8); mask[[0, 3, 4, 9, 15]] = 1
    d.reset(mask, seed=99)                                                   # a new seed: the masked agents make rooms under it
    step(2)
    d.reset(mask[::-1].copy(), seed=99)                                      # the same seed, other agents
    step(2)
    walk_into_the_goal(d, (np.arange(B) % 3 == 0).astype(np.uint8))          # a masked set_state: the layouts and the counters stay
    step(4)
    d.set_wall_rooms(None)                                                   # off: the walls stay, restarts keep them
    step(3)
    ring = np.ones((8, 8), bool); ring[1:-1, 1:-1] = False
    d.set_walls(ring, None, mask)                                            # ... and set_walls works again
    step(2)
    d.set_wall_rooms(room=1, stop=0.1, doors=0.5, levels=2, first_level=5, level_seed=3)   # on again: two levels
    step(3)
    d.set_wall_rooms(room=3, stop=0, doors=0)                                # other parameters over the running rooms
    step(3)


SCENARIOS = dict(tiny=(tiny, TINY), square=(square, SQUARE), square64=(square, SQUARE64), doors=(doors, DOORS), wide=(wide, WIDE), levels=(levels, LEVELS),
                 features=(features, CALLS), calls=(calls, CALLS))


recorded = functools.partial(WF.recorded, "rooms")                                  # (name, render=True, offset=0, batch=None) -> (snapshots, events), cached
play = functools.partial(WF.play, "rooms")                                          # (rcw, name, env, trackers=(), wrap=None) -> events


# ---- what tests/test_gpu_wall_families.py plays of this family: the arguments of the tests every family has ------------------------------------
ROLLOUTS = [("tiny", "two-launches"), ("tiny", "one-launch"), ("square", None), ("square64", None), ("doors", None), ("wide", None), ("levels", None),
            ("calls", "two-launches"), ("calls", "one-launch")]
REPLAYED = (dict(LEVELS, B=21), (dict(room=1, stop=0.1, doors=0.6), dict(levels=5, first_level=3, level_seed=8)))
BESIDE_A_PLAIN_HANDLE = dict(room=1)
UNTOUCHED = dict(room=1, levels=3, first_level=1, level_seed=2)
CAPTURED = (dict(CALLS, B=12), dict(room=1, stop=0.25, doors=0.5))
SHARDED = (12, dict(room=1, stop=0.2, doors=0.5, levels=6, first_level=40, level_seed=9), (2, 0.5, 0))    # (the map's width, the install, other parameters without levels)
REFUSED_MAPS = [(4, 9, ValueError, "at least 5 x 5"), (9, 4, ValueError, "at least 5 x 5"),
                (131, 131, "unsupported", "at most 4096"), (130, 131, "unsupported", "at most 4096")]
NAMED = {(131, 131): ("130 x 130", "4225"), (130, 131): ("130 x 130", "4160")}  # Q past the bound: the message names the bound and Q
FUZZ = ("rooms", "wall rooms:", ("step", "reset", "masked_reset", "set_state", "arrive", "off_and_on", "episode_starts", "rooms_made", "second_doors", "goal_redraws",
                                 "restarts_after_done", "restarts_after_truncation", "one_launch_steps", "two_launch_steps", "non_square", "with_levels", "stopped",
                                 "rooms_past_64"))


def reached(events, name=None):
    """what the reference's counts must show of a run (of scenario `name`) beyond restarts: the root is always cut, so more rooms than layouts"""
    assert events["rooms_made"] > events["episode_starts"]
    if name == "doors":
        assert events["second_doors"] > events["episode_starts"]


def check_rollout(rcw, env, name):
    """what holds of the engine behind scenario `name`"""
    c = SCENARIOS[name][1]
    walls, layout = env.world.walls, env.wall_layout.numpy()
    if name == "square64":
        assert env.world.player_position_wu.dtype == np.float64
    if name == "tiny":
        assert (layout == -1).all() and ((~walls).sum(axis=(1, 2)) == 7).all() and len({w.tobytes() for w in walls}) == 4   # the four layouts
    elif name == "levels":
        assert set(layout.tolist()) == {43, 44, 45} and min(np.bincount(layout - 43)) > 5
        for level in (43, 44, 45):                                            # every level held by several agents, one layout a level
            held = walls[layout == level]
            assert (held == held[0]).all()
            want = rcw.layouts.generated_rooms(rcw.layouts.generated_maze_key(0, 0, 0, 1, level, 9)[0], c["H"], c["W"], 1)
            np.testing.assert_array_equal(held[0], want)
    else:
        assert (layout == -1).all()
