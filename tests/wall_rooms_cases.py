"""The rooms' scenarios, written ONCE and run twice — test infrastructure, not a test.

The drivers and the shapes are tests/wall_bank_cases.py's and tests/wall_generator_cases.py's, by import, as the caves' are: a Recorder (the
reference alone, tests/wall_rooms_ref.py, under tests/time_limit_ref.py where the scenario sets a limit; a snapshot after every call) and a
Player (an engine: every call made on it and compared with the next snapshot byte for byte, then handed to the feature trackers).  What
changes is the reference they drive, the call `set_wall_rooms`, and the comparison of wall_layout, which the engine serves while the ROOMS
are on.

Every scenario: 8 headings, a quarter tile a move, a player radius of 0.3, auto_reset, forward-heavy actions (walls_ref.draw_actions).
"""
import functools

import numpy as np

import wall_bank_cases as BC
import wall_generator_cases as GC
import wall_rooms_ref as RR
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


def make_ref(c, render=True, **kw):
    return RR.WallRoomsRef(c["B"], c["seed"], c["H"], c["W"], c["N"], c["Hc"], T=np.float64 if c.get("T") == "Float64" else np.float32,
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
        s["rooms"], s["rendered"] = self.ref.gen is not None, self.render
        self.snaps.append(s)

    @property
    def events(self):
        return dict(self.ref.events, **(self.lim.events if self.lim is not None else {}), keys_made=set(self.ref.keys_made))

    def set_wall_rooms(self, room=RR.DEFAULT_ROOM, stop=RR.DEFAULT_STOP, doors=RR.DEFAULT_DOORS, levels=0, first_level=0, level_seed=0):
        self.ref.set_wall_rooms(room, stop, doors, levels, first_level, level_seed)
        if self.lim is not None and room is not None:
            self.lim.clear()
        self._snap()


class Player(GC.Player):
    def _check(self, where):
        s = self.snaps[self.k]
        where = f"{self.name}, call {self.k}: {where}"
        self.k += 1
        assert self.env.wall_rooms_info["enabled"] == s["rooms"] and not self.env.wall_bank_info["layouts"], where
        assert not self.env.wall_caves_info["enabled"], where
        assert self.env.wall_generator_info["enabled"] == s["rooms"] and self.env.wall_generator_info["loops"] == 0, where
        if s["rendered"]:
            RR.assert_equal(self.env, s, where)
        else:
            GC.assert_state_equal(self.env, s, where)
            if s["rooms"]:
                np.testing.assert_array_equal(self.env.wall_layout.numpy(), s["wall_layout"], err_msg=f"wall_layout {where}")
        if "episode_steps" in s:
            np.testing.assert_array_equal(self.env.world.episode_steps, s["episode_steps"], err_msg=f"episode_steps {where}")
            np.testing.assert_array_equal(self.env.world.truncated.astype(np.uint8), s["truncated"], err_msg=f"truncated {where}")
        return where

    def set_wall_rooms(self, room=RR.DEFAULT_ROOM, stop=RR.DEFAULT_STOP, doors=RR.DEFAULT_DOORS, levels=0, first_level=0, level_seed=0):
        self.env.set_wall_rooms(room, stop, doors, levels, first_level, level_seed)
        if room is None:
            self._check("rooms off")
        else:
            self._masked(None, "set_wall_rooms")


# ---- the scenarios ------------------------------------------------------------------------------------------------------------------------
def rollout(d, rooms, limit, steps, seed):
    d.set_wall_rooms(**rooms)
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
