"""The walled worlds on the C oracle — test infrastructure, not a test.

WalledOracle is oracle.OracleBatch (oracle/rcw_oracle.c, which carries interior walls: orc_set_walls, the goal redraw of reset!(world))
with the interface of tests/walls_ref.py's WallsRef on it — reset, set_walls, set_state, step, step_lenient, clear_status, snapshot,
walls_of, events — and ONE rule on top, the rule of the wall bank and of the wall generator's families (include/rcw.h):

    a handle with a SOURCE of layouts gives an agent another layout whenever its episode counter moves.  With g the global agent id and e
    the counter before the increment, the agent takes the source's layout of (seed, g, e), is reset against it under episode_key(seed, g, e)
    — what orc_set_walls does for the masked agents — and its counter is e + 1, once.  An agent a step restarts (done under auto_reset
    here; truncated: tests/time_limit_ref.py resets it through `reset(mask, seed)` in front of the step) is not moved by that step's
    action: the step leaves it alone (the oracle's `moved` mask).  An install restarts everybody under the current seed.

The sources are built from the makers that exist, not restated: wall_bank_ref.layout_draw over the bank's cumulative weights;
wall_generator_ref.maze_key and wall_family.FAMILIES[...].make for mazes, caves and rooms.  Layouts are cached per key: with levels >= 1 a
rollout of a thousand agents on large maps runs the Python makers a handful of times.

What ties this reference to the reviewed ones: tests/test_oracle_walls.py holds the C against WallsRef byte for byte, and
tests/test_walled_oracle_spec.py holds FastRecorder — the scenarios' Recorder on this class — against the Python Recorders' snapshots of
a bank, a maze, a cave and a rooms scenario.  TimeLimitRef wraps a WalledOracle exactly as it wraps a WallsRef.

`events`: interior_wall_ray_hits (rays of rendered frames that stopped on a wall tile inside the ring, counted in numpy behind every
call for the agents it rendered), goal_redraws and blocked_next_to_interior_wall (the oracle's own per-agent counters), restarts_after_done,
episode_starts (under a source).
"""
import functools

import numpy as np

import wall_bank_cases as BC
import wall_bank_ref as WB
import wall_family as WF
import wall_generator_ref as WG
from oracle import oracle as O


# ---- the sources of layouts ---------------------------------------------------------------------------------------------------------
class BankSource:
    """rcw_set_wall_bank: layout k of the bank, k drawn by wall_bank_ref.layout_draw"""

    def __init__(self, walls, weights=None):
        walls = np.asarray(walls) != 0
        self.bank = walls[None] if walls.ndim == 2 else walls
        assert all(WB.valid_layout(w) for w in self.bank)
        self.set_weights(weights)

    def set_weights(self, weights):
        self.cum = WB.cumulative(weights, len(self.bank))

    def layout(self, seed, g, e):
        """(a key to cache the layout under, the layout, the agent's wall_layout word)"""
        k = WB.layout_draw(seed, g, e, self.cum)
        return k, self.bank[k], k


class FamilySource:
    """rcw_set_wall_generator / _caves / _rooms: the family's maker on wall_generator_ref.maze_key's key"""

    def __init__(self, family, H, W, own, levels, first_level, level_seed):
        self.family, self.H, self.W = family, H, W
        self.own, self.levels, self.first_level, self.level_seed = own, int(levels), int(first_level), int(level_seed)
        self._made = {}

    def layout(self, seed, g, e):
        m, level = WG.maze_key(seed, g, e, self.levels, self.first_level, self.level_seed)
        if m not in self._made:
            self._made[m] = np.asarray(self.family.make(m, self.H, self.W, *self.own)[0]) != 0
        return m, self._made[m], level


# ---- the reference --------------------------------------------------------------------------------------------------------------------
class WalledOracle(O.OracleBatch):
    def __init__(self, batch, seed=0, render=True, config=None, **overrides):
        super().__init__(batch, seed=seed, render=render, config=config, **overrides)
        self.seed, self.offset, self.auto_reset = int(seed), int(self.cfg.agent_id_offset), bool(self.cfg.auto_reset)
        self.source = None
        self.wall_layout = np.zeros(self.B, np.int32)
        self.keys_made, self.layouts_drawn = set(), set()
        self._counts = dict(interior_wall_ray_hits=0, restarts_after_done=0, episode_starts=0)
        self._account(None)                                                      # (orc_create renders the first reset's frames)

    # ---- bookkeeping ---------------------------------------------------------------------------------------------------------------
    @property
    def events(self):
        return dict(self._counts, goal_redraws=int(self.goal_redraws.sum()), blocked_next_to_interior_wall=int(self.blocked_inner.sum()))

    def _who(self, mask):
        return np.ones(self.B, bool) if mask is None else np.asarray(mask).reshape(self.B) != 0

    def _account(self, mask):
        who = self._who(mask)
        stop = self.ray_stop
        i, j = stop[..., 0], stop[..., 1]
        inner = (i > 1) & (i < self.H) & (j > 1) & (j < self.W) & who[:, None]
        b = np.broadcast_to(np.arange(self.B)[:, None], i.shape)
        self._counts["interior_wall_ray_hits"] += int(self.walls[b[inner], i[inner] - 1, j[inner] - 1].sum())

    def walls_of(self, b):
        return self.walls[b].copy()

    # ---- the rule ------------------------------------------------------------------------------------------------------------------
    def _begin_episodes(self, who):
        """the agents in `who` take their source's layout of (seed, g, counter) and are reset against it: one orc_set_walls"""
        agents = np.flatnonzero(who)
        if not agents.size:
            return
        stack, place, index = [], {}, np.zeros(self.B, np.int32)
        episode = self.episode
        for a in agents:
            key, walls, word = self.source.layout(self.seed, self.offset + int(a), int(episode[a]))
            if key not in place:
                place[key] = len(stack)
                stack.append(walls)
            index[a] = place[key]
            self.wall_layout[a] = word
            (self.layouts_drawn if isinstance(self.source, BankSource) else self.keys_made).add(key)
        O.OracleBatch.set_walls(self, np.stack(stack), index, who.astype(np.uint8))
        self._counts["episode_starts"] += int(agents.size)

    def _install(self, source):
        self.source = source
        self.reset()

    # ---- the calls -----------------------------------------------------------------------------------------------------------------
    def reset(self, mask=None, seed=None):
        if seed is not None:
            self.seed = int(seed)
        if self.source is None:
            super().reset(mask, self.seed)
        else:
            super().reset(np.zeros(self.B, np.uint8), self.seed)                 # (the batch's seed alone: nobody is in the mask)
            self._begin_episodes(self._who(mask))
        self._account(mask)

    def set_walls(self, walls, index=None, mask=None):
        if self.source is not None:
            raise RuntimeError("rcw_set_walls is refused while the handle has a source of layouts")
        super().set_walls(walls, index, mask)
        self._account(mask)

    def set_state(self, goal, pos, heading, mask=None):
        super().set_state(goal, pos, heading, mask)
        self._account(mask)

    def _step(self, actions, lenient, moved):
        a = np.ascontiguousarray(actions, dtype=np.uint8).reshape(self.B)
        valid = (a >= 1) & (a <= 4)
        moved = self._who(moved)
        if not lenient and not valid[moved].all():
            return super().step(a, moved.astype(np.uint8))                       # (the refusal: nothing is touched)
        restart = valid & moved & (self.done != 0) & self.auto_reset
        self._counts["restarts_after_done"] += int(restart.sum())
        if self.source is not None and restart.any():
            self._begin_episodes(restart)
            moved = moved & ~restart
        rc = (super().step_lenient if lenient else super().step)(a, moved.astype(np.uint8))
        self._account(valid & (moved | restart))
        return rc

    def step(self, actions, moved=None):
        return self._step(actions, False, moved)

    def step_lenient(self, actions, moved=None):
        return self._step(actions, True, moved)

    # ---- the sources' setters, under the engine's names ------------------------------------------------------------------------------
    @property
    def bank(self):
        return self.source.bank if isinstance(self.source, BankSource) else None

    @property
    def gen(self):
        s = self.source
        return (s.own, s.levels, s.first_level, s.level_seed) if isinstance(s, FamilySource) else None

    def set_wall_bank(self, walls, weights=None):
        """install (every agent restarts under the rule with the current seed) or, walls None, switch off (walls kept)"""
        if walls is None:
            self.source = None
        else:
            self._install(BankSource(walls, weights))

    def set_weights(self, weights):
        self.source.set_weights(weights)

    def set_wall_family(self, key, *args, **kw):
        """a family's setter (wall_family.arguments: its own parameters, then levels, first_level, level_seed); the first None: off"""
        f = WF.FAMILIES[key]
        *own, levels, first_level, level_seed = WF.arguments(f, args, kw)
        if own[0] is None:
            self.source = None
            return
        own = WF.parameters(f, own)
        assert f.install_refusal(self.H, self.W, own, levels, first_level) is None
        self._install(FamilySource(f, self.H, self.W, own, levels, first_level, level_seed))

    def set_wall_generator(self, *args, **kw):
        self.set_wall_family("generator", *args, **kw)

    def set_wall_caves(self, *args, **kw):
        self.set_wall_family("caves", *args, **kw)

    def set_wall_rooms(self, *args, **kw):
        self.set_wall_family("rooms", *args, **kw)

    # ---- the compared arrays ---------------------------------------------------------------------------------------------------------
    def snapshot(self):
        """walls_ref.WallsRef.snapshot's arrays, copied, plus wall_layout"""
        s = dict(reward=self.reward, done=self.done, goal=self.goal, position=self.position, direction=self.direction, episode=self.episode,
                 col_height=self.col_height, col_colour=self.col_colour, status=self.status)
        s = {k: v.copy() for k, v in s.items()}
        s.update(tile_map_chunks=self.tile_map_chunks(), wall_layout=self.wall_layout.copy())
        if self.render:
            s["camera_view"] = self.camera_view.copy()
        return s


def case_overrides(c, auto_reset=True, agent_id_offset=0, **more):
    """the config of the wall tests' shapes (walls_ref.WallsRef's defaults): 8 headings, a quarter tile a move, a player radius of 0.3"""
    kw = dict(height_tile_map_tu=c["H"], width_tile_map_tu=c["W"], num_rays=c["N"], height_camera_view_pu=c["Hc"], num_directions=c.get("nd", 8),
              position_increment_wu=0.25, position_increment_wu_f64=0.25, player_radius_wu=np.float32(0.3), player_radius_wu_f64=0.3,
              auto_reset=1 if auto_reset else 0, agent_id_offset=agent_id_offset, world_unit_bits=64 if c.get("T") == "Float64" else 32)
    kw.update(more)
    return kw


def from_case(c, render=True, **kw):
    return WalledOracle(c["B"], seed=c["seed"], render=render, **case_overrides(c, **kw))


# ---- the scenarios' Recorder on this reference ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def FastRecorder(kind):
    """kind "bank": wall_bank_cases.Recorder, else wall_family.drivers(kind)'s — the same methods, the snapshots of a WalledOracle"""
    base = BC.Recorder if kind == "bank" else WF.drivers(kind)[0]

    def init(self, c, render=True, **kw):
        self.c, self.ref, self.lim, self.snaps, self.render, self.B = c, from_case(c, render, **kw), None, [], render, c["B"]
        if kind != "bank":
            self.ref.set_family = functools.partial(self.ref.set_wall_family, kind)
        self._snap()

    return type("FastRecorder_" + kind, (base,), {"__init__": init})


def recorded(kind, name, **kw):
    """the scenario `name` of the bank's or a family's cases on this reference: (snapshots, events)"""
    fn, c = (BC.SCENARIOS if kind == "bank" else WF.cases_of(kind).SCENARIOS)[name]
    rec = FastRecorder(kind)(c, **kw)
    fn(rec)
    return rec.snaps, rec.events
