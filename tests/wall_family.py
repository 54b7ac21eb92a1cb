"""The wall generator's layout families — mazes, caves, rooms — described ONCE: test infrastructure, not a test.

A family is a row of FAMILIES: the name of its setter and of its info property, its own parameters in order (name, default, whether a
probability word: a float is scaled, an int is taken as the word), its maker (m, H, W, *params) -> (walls, counts), the event counters
`counts` feeds, the host export of raycastworlds_jl_amd.layouts that replays it, its install_refusal, and what the OTHER families' infos
read while it is on.  The makers themselves stay where they are: wall_generator_ref.maze, wall_caves_ref.cave, wall_rooms_ref.rooms.

On that table, once, what the families share:

    WallFamilyRef   WallsRef with one override of _reset_agent.  THE KEY OF AN EPISODE, with g the global agent id and e the counter
                    before the increment: key = episode_key(seed, g, e), u = draw(key, 2^63) (wall_generator_ref.maze_key);
                    levels == 0: m = u, wall_layout = -1; levels >= 1: l = first_level + below(u, levels), m = episode_key(level_seed, l, 0),
                    wall_layout = l.  After that the rule is the bank's: WALL := the family's layout of m, GOAL cleared, the reset of
                    walls_ref.py against the new walls under `key` from draw 0, counter = e + 1 (once).  An install restarts every agent
                    under the current seed; switching off keeps the walls; set_walls is refused while the family is on.  `events` also
                    counts episode_starts and the family's counters, `keys_made` is the set of keys m used so far.
    assert_equal    walls_ref.assert_equal plus wall_layout, which the engine serves while a family is on.
    Recorder        the reference alone, under tests/time_limit_ref.py where the scenario sets a limit: a snapshot after every call.
    Player          an engine: every call made on it and compared with the next snapshot byte for byte, then handed to the feature trackers.
    drivers(key)    the two with the family's setter as their one own method — what a cases module exports as Recorder and Player.
    rollout, walk_and_step, recorded, play      the scenarios' common moves and the two entry points, keyed by family and scenario.
    engine_state, infos, unchanged, level_key   what the GPU tests of every family read of a handle.

The shapes, the pinned hard levels and the scenarios are each family's own: tests/wall_generator_cases.py, wall_caves_cases.py,
wall_rooms_cases.py.
"""
import functools
import importlib
from collections import namedtuple

import numpy as np

import wall_bank_cases as BC
import wall_caves_ref as WC
import wall_generator_ref as WG
import wall_rooms_ref as RR
import walls_ref as WR
from oracle import pyref

word = WG.loops_word                                                           # a probability as the UInt32 the rules compare with
LEVELS = (("levels", 0), ("first_level", 0), ("level_seed", 0))               # every family's setter ends with these three

Family = namedtuple("Family", "key setter info params make counters made replay install_refusal others cases_module")


def _maze(m, H, W, loops):
    return WG.maze(m, H, W, loops), ()


def _cave(m, H, W, fill, smooth):
    walls, fell = WC.cave(m, H, W, fill, smooth, return_fell_back=True)
    return walls, (int(fell),)


def _rooms(m, H, W, room, stop, doors):
    walls, leaves, cuts, _ = RR.rooms(m, H, W, room, stop, doors, details=True)
    return walls, (len(leaves), sum(len(c[2]) == 2 and c[2][0] != c[2][1] for c in cuts))


# `others`: info property -> what it reads while the family is on.  wall_generator_info reports `enabled` and loops == 0 under caves and rooms.
_BESIDE = dict(enabled=True, loops=0)
FAMILIES = dict(
    generator=Family("generator", "set_wall_generator", "wall_generator_info", (("loops", 0.0, True),), _maze, (), "mazes_made", "generated_maze",
                     lambda H, W, p, levels, first: WG.install_refusal(H, W, levels, first),
                     dict(wall_caves_info=dict(enabled=False), wall_rooms_info=dict(enabled=False)), "wall_generator_cases"),
    caves=Family("caves", "set_wall_caves", "wall_caves_info", (("fill", WC.DEFAULT_FILL, True), ("smooth", WC.DEFAULT_SMOOTH, False)), _cave,
                 ("fallbacks",), "keys_made", "generated_cave",
                 lambda H, W, p, levels, first: WC.install_refusal(H, W, p[1], levels, first),
                 dict(wall_generator_info=_BESIDE, wall_rooms_info=dict(enabled=False)), "wall_caves_cases"),
    rooms=Family("rooms", "set_wall_rooms", "wall_rooms_info",
                 (("room", RR.DEFAULT_ROOM, False), ("stop", RR.DEFAULT_STOP, True), ("doors", RR.DEFAULT_DOORS, True)), _rooms,
                 ("rooms_made", "second_doors"), "keys_made", "generated_rooms",
                 lambda H, W, p, levels, first: RR.install_refusal(H, W, p[0], levels, first),
                 dict(wall_generator_info=_BESIDE, wall_caves_info=dict(enabled=False)), "wall_rooms_cases"),
)


def cases_of(key):
    """the family's cases module (imported late: the cases modules import this one)"""
    return importlib.import_module(FAMILIES[key].cases_module)


def arguments(f, args, kw):
    """a setter's arguments in order, defaults filled in: the family's own, then levels, first_level, level_seed"""
    names = [p[0] for p in f.params] + [n for n, _ in LEVELS]
    vals = dict(zip(names, [p[1] for p in f.params] + [d for _, d in LEVELS]))
    assert len(args) <= len(names) and set(kw) <= set(names) and not set(kw) & set(names[:len(args)]), (f.setter, args, kw)
    vals.update(zip(names, args))
    vals.update(kw)
    return [vals[n] for n in names]


def parameters(f, own):
    """the family's own parameters as the engine holds them: probabilities as words, the rest as ints"""
    return tuple((int(p) if isinstance(p, (int, np.integer)) else word(p)) if is_word else int(p) for (_, _, is_word), p in zip(f.params, own))


# ---- the reference --------------------------------------------------------------------------------------------------------------------------
class WallFamilyRef(WR.WallsRef):
    def __init__(self, family, *args, **kw):
        self.family = FAMILIES[family] if isinstance(family, str) else family
        self.gen = None                                                         # (own parameters, levels, first_level, level_seed) while on
        setattr(self, self.family.setter, self.set_family)
        super().__init__(*args, **kw)
        self.wall_layout = np.zeros(self.B, np.int32)
        self.events.update(dict.fromkeys(("episode_starts",) + self.family.counters, 0))
        self.keys_made = set()
        self._cache = {}

    # ---- the rule ------------------------------------------------------------------------------------------------------------------
    def _reset_agent(self, b):
        if self.gen is not None:
            own, levels, first_level, level_seed = self.gen
            m, level = WG.maze_key(self.seed, self.offset + b, int(self.episode[b]), levels, first_level, level_seed)
            if m not in self._cache:
                self._cache[m] = self.family.make(m, self.H, self.W, *own)
            walls, counts = self._cache[m]
            tm = self.worlds[b].tile_map
            for i in range(1, self.H + 1):
                for j in range(1, self.W + 1):
                    tm[pyref.WALL][i][j] = bool(walls[i - 1, j - 1])
                    tm[pyref.GOAL][i][j] = False
            self.events["episode_starts"] += 1
            for name, n in zip(self.family.counters, counts):
                self.events[name] += n
            self.keys_made.add(m)
            self.wall_layout[b] = level
        super()._reset_agent(b)

    # ---- the calls -----------------------------------------------------------------------------------------------------------------
    def set_family(self, *args, **kw):
        """the family's setter (bound under its own name too): install — every agent restarts under the rule with the current seed — or,
        the first parameter None, switch off (walls kept).  A probability: a float, or the UInt32 word as an int."""
        f = self.family
        *own, levels, first_level, level_seed = arguments(f, args, kw)
        if own[0] is None:
            self.gen = None
            return
        own = parameters(f, own)
        assert f.install_refusal(self.H, self.W, own, levels, first_level) is None
        self.gen = (own, int(levels), int(first_level), int(level_seed))
        self._cache = {}
        self.reset()

    def set_walls(self, walls, index=None, mask=None):
        if self.gen is not None:
            raise RuntimeError(f"rcw_set_walls is refused while the handle's {self.family.key} is on")
        super().set_walls(walls, index, mask)

    def snapshot(self):
        return dict(super().snapshot(), wall_layout=self.wall_layout.copy())


def make_ref(family, c, render=True, **kw):
    return WallFamilyRef(family, c["B"], c["seed"], c["H"], c["W"], c["N"], c["Hc"], T=np.float64 if c.get("T") == "Float64" else np.float32,
                         render=render, **kw)


make_env = BC.make_env


def assert_equal(env, ref, where=""):
    """walls_ref.assert_equal plus wall_layout (while a family is on: without a source of layouts the engine refuses the getter)"""
    r = ref if isinstance(ref, dict) else ref.snapshot()
    WR.assert_equal(env, r, where)
    if any(getattr(env, f.info)["enabled"] for f in FAMILIES.values()):
        got = env.wall_layout.numpy()
        assert got.dtype == np.int32
        np.testing.assert_array_equal(got, r["wall_layout"], err_msg=f"wall_layout {where}")


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


# ---- the two drivers ----------------------------------------------------------------------------------------------------------------------
class Recorder(BC.Recorder):
    """wall_bank_cases.Recorder on a WallFamilyRef.  A Recorder made with render=False records no frames."""
    family = None

    def __init__(self, c, render=True, **kw):
        self.c, self.ref, self.lim, self.snaps, self.render = c, make_ref(self.family, c, render, **kw), None, [], render
        self.B = c["B"]
        self._snap()

    def _snap(self):
        s = self.ref.snapshot()
        if self.lim is not None:
            s.update(episode_steps=self.lim.episode_steps.copy(), truncated=self.lim.truncated.copy())
        s[self.family.key], s["rendered"] = self.ref.gen is not None, self.render
        self.snaps.append(s)

    @property
    def events(self):
        return dict(self.ref.events, **(self.lim.events if self.lim is not None else {}), **{self.family.made: set(self.ref.keys_made)})

    def _set_family(self, *args, **kw):
        self.ref.set_family(*args, **kw)
        if self.lim is not None and self.ref.gen is not None:
            self.lim.clear()
        self._snap()


class Player(BC.Player):
    """wall_bank_cases.Player against a family's recording: without frames it compares everything but the column descriptors and the
    camera view"""
    family = None

    def _check(self, where):
        f, s = self.family, self.snaps[self.k]
        where = f"{self.name}, call {self.k}: {where}"
        self.k += 1
        on = s[f.key]
        assert getattr(self.env, f.info)["enabled"] == on and not self.env.wall_bank_info["layouts"], where
        for info, reads in f.others.items():                                  # the other families' infos: on with this one, or never
            got = getattr(self.env, info)
            want = dict(reads, enabled=reads["enabled"] and on)
            assert {k: got[k] for k in want} == want, f"{info} {where}"
        if s["rendered"]:
            assert_equal(self.env, s, where)
        else:
            assert_state_equal(self.env, s, where)
            if on:
                np.testing.assert_array_equal(self.env.wall_layout.numpy(), s["wall_layout"], err_msg=f"wall_layout {where}")
        if "episode_steps" in s:
            np.testing.assert_array_equal(self.env.world.episode_steps, s["episode_steps"], err_msg=f"episode_steps {where}")
            np.testing.assert_array_equal(self.env.world.truncated.astype(np.uint8), s["truncated"], err_msg=f"truncated {where}")
        return where

    def _set_family(self, *args, **kw):
        vals = arguments(self.family, args, kw)
        getattr(self.env, self.family.setter)(*vals)
        if vals[0] is None:
            self._check(f"{self.family.key} off")
        else:
            self._masked(None, self.family.setter)


@functools.lru_cache(maxsize=None)
def drivers(key):
    """(Recorder, Player) of a family: the shared classes with the family's setter as their one own public method"""
    f = FAMILIES[key]
    return tuple(type(base.__name__, (base,), {"family": f, f.setter: base._set_family, "__doc__": base.__doc__}) for base in (Recorder, Player))


# ---- what the scenarios share -------------------------------------------------------------------------------------------------------------
walk_into_the_goal = BC.walk_into_the_goal


def rollout(key, d, params, limit, steps, seed):
    """the family's install with `params`, a limit (0: none), `steps` steps of forward-heavy actions"""
    getattr(d, FAMILIES[key].setter)(**params)
    if limit:
        d.set_time_limit(limit)
    rng = np.random.default_rng(seed)
    for _ in range(steps):
        d.step(WR.draw_actions(rng, d.B))


def walk_and_step(d, every, seed, steps=3):
    walk_into_the_goal(d, (np.arange(d.B) % every == 0).astype(np.uint8))
    rng = np.random.default_rng(seed)
    for _ in range(steps):
        d.step(WR.draw_actions(rng, d.B))


@functools.lru_cache(maxsize=None)
def recorded(key, name, render=True, offset=0, batch=None):
    """the reference's run of a family's scenario, computed once: (snapshots, events)"""
    cases = cases_of(key)
    fn, c = cases.SCENARIOS[name]
    c = dict(c, B=batch) if batch is not None else c
    rec = drivers(key)[0](c, render and name not in getattr(cases, "UNRENDERED", ()), agent_id_offset=offset)
    fn(rec)
    return rec.snaps, rec.events


def play(key, rcw, name, env, trackers=(), wrap=None):
    """the scenario on `env` against its recording; trackers: the feature trackers, made once the engine exists"""
    fn, _ = cases_of(key).SCENARIOS[name]
    snaps, events = recorded(key, name)
    p = drivers(key)[1](rcw, env, snaps, name)
    p.trackers = list(trackers)
    fn(p if wrap is None else wrap(p))                                       # (wrap: tests/deferred.py takes a note behind every call)
    p.finished()
    return events


# ---- what the GPU tests read of a handle --------------------------------------------------------------------------------------------------
def level_key(level_seed, level):
    """the key of every agent's layout under levels=1, first_level=level, level_seed"""
    return WR.episode_key(level_seed, level, 0)


def engine_state(env):
    w = env.world
    h, c = env.columns()
    s = dict(frame=env.camera_view_host(), col_h=h, col_c=c, tile_map=w.tile_map_chunks, goal=w.goal_position, position=w.player_position_wu,
             heading=w.player_direction_au, reward=w.reward, done=w.done, episode=w.episode, status=w.status, episode_steps=w.episode_steps,
             truncated=w.truncated)
    if env.wall_generator_info["enabled"] or env.wall_bank_info["layouts"]:
        s["wall_layout"] = env.wall_layout.numpy()
    return s


def infos(env):
    return env.wall_rooms_info, env.wall_caves_info, env.wall_generator_info, env.wall_bank_info


def unchanged(env, before, info, what):
    after = engine_state(env)
    assert set(after) == set(before), what
    for k in before:
        np.testing.assert_array_equal(after[k], before[k], err_msg=f"{k} behind {what}")
    assert infos(env) == info, what
