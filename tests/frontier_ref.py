"""The frontier (include/rcw.h, rcw_set_frontier) restated in Python — test infrastructure, not a test.

  flood         the definition for one agent in numpy: the sources — unseen tiles with a seen passable edge neighbour, taken by shifting
                the (H, W) plane, so nothing wraps from one column into the next —, then a breadth-first dilation a level at a time
                through passable tiles.  Returns (field uint16 (H, W), tiles).  level_sizes(field): how many tiles each level holds.
  expected      field, distance and tiles of a whole batch from the engine's OWN seen map and positions, and the action words through
                guide_ref.rule on that field with the engine's own headings and table.  A kept agent's map has not changed since its last
                flood, so the flood of the map as it is now is what every agent must hold, kept or flooded again.
  Tracked       an engine with the frontier on; `check` compares all five arrays with `expected` after whatever call the test just made and
                counts what the comparisons saw: behind a step the agents kept (newly_seen == 0, the same episode) and flooded again,
                agents with distance == -1, restarts, the widest flood.
  explore       the closed loop on the CPU, a batch in lock-step: seen_map_ref's march marks the map, the flood and guide_ref's rule give
                the action, a small act! with guide_ref's collision test moves the agent — until distance == -1 or the goal is touched.
"""
import numpy as np

import guide_ref as GR
import seen_map_ref as SM
from oracle import pyref

UNREACHED = 0xFFFF


def _around(a):
    """bool (H, W): the tiles with an edge neighbour in `a` — shifted planes, zero beyond the map's edge"""
    out = np.zeros_like(a)
    out[1:] |= a[:-1]
    out[:-1] |= a[1:]
    out[:, 1:] |= a[:, :-1]
    out[:, :-1] |= a[:, 1:]
    return out


def flood(seen_map):
    """seen_map: uint8 (H, W), 0 unseen, 1 free, 2 wall, 3 goal, 4 and above wall.  (field, tiles)."""
    m = np.asarray(seen_map)
    passable = (m == 1) | (m == 3)
    front = (m == 0) & _around(passable)
    field = np.full(m.shape, UNREACHED, np.uint16)
    field[front] = 0
    tiles = int(front.sum())
    reached = front.copy()
    level = 0
    while front.any():
        level += 1
        front = _around(front) & passable & ~reached
        field[front] = level
        reached |= front
    return field, tiles


def level_sizes(field):
    f = np.asarray(field).reshape(-1)
    return np.bincount(f[f != UNREACHED].astype(np.int64))


def lookup(field, pos):
    """distance: the field at the player's tile, -1 where that is 0xFFFF, off the map or not finite"""
    x, y = float(pos[0]), float(pos[1])
    if not (np.isfinite(x) and np.isfinite(y)):
        return -1
    i, j = int(np.floor(x)), int(np.floor(y))
    H, W = field.shape
    if not (0 <= i < H and 0 <= j < W):
        return -1
    f = int(field[i, j])
    return -1 if f == UNREACHED else f


def expected(env):
    """dict(field (B, H, W), distance, tiles, action, heading) from the engine's own seen map, positions, headings and table"""
    maps, w = env.seen_map, env.world
    pos, dirs = w.player_position_wu, w.player_direction_au
    inc = env.cfg.position_increment_wu_f64 if env.T is np.float64 else env.cfg.position_increment_wu
    floods = [flood(m) for m in maps]
    fields = np.stack([f for f, _ in floods])
    action, heading = GR.expected(fields, pos, dirs, w.directions_wu, inc, env.T)
    return dict(field=fields, distance=np.array([lookup(fields[b], pos[b]) for b in range(len(maps))], np.int32),
                tiles=np.array([t for _, t in floods], np.int32), action=action, heading=heading)


class Tracked:
    """An engine with the frontier on.  Every `check` reads the engine's state and holds all five arrays to `expected`; `seen` counts, over
    the checks behind a step, the agents kept and flooded again, and over all checks distance == -1, restarts and the widest flood."""

    def __init__(self, env, enable=True):
        self.env = env
        self.seen = dict(checks=0, kept=0, flooded=0, nothing_left=0, restarts=0, most_sources=0, widest_level=0, forward=0)
        if enable:
            env.set_frontier(True)
        assert env.frontier_enabled and env.seen_map_enabled
        self.episode = env.world.episode.copy()
        self.check("enabled")

    def check(self, where, stepped=False):
        env = self.env
        exp = expected(env)
        got = dict(field=env.frontier_field, distance=env.frontier_distance.numpy(), tiles=env.frontier_tiles.numpy(),
                   action=env.explore_action.numpy(), heading=env.explore_heading.numpy())
        for name, dtype in (("field", np.uint16), ("distance", np.int32), ("tiles", np.int32), ("heading", np.int32), ("action", np.uint8)):
            assert got[name].dtype == dtype and got[name].shape == exp[name].shape, (name, got[name].dtype, got[name].shape)
            np.testing.assert_array_equal(got[name], exp[name], err_msg=f"{name} {where}")
        assert ((exp["action"] >= 1) & (exp["action"] <= 4)).all() and (exp["heading"][exp["distance"] < 0] == -1).all()
        s, episode = self.seen, env.world.episode
        restarted = episode != self.episode
        if stepped:
            kept = (env.seen_new.numpy() == 0) & ~restarted
            s["kept"] += int(kept.sum())
            s["flooded"] += int((~kept).sum())
        s["checks"] += 1
        s["restarts"] += int(restarted.sum())
        s["nothing_left"] += int((exp["distance"] < 0).sum())
        s["forward"] += int((exp["action"] == 1).sum())
        s["most_sources"] = max(s["most_sources"], int(exp["tiles"].max()))
        s["widest_level"] = max(s["widest_level"], max(int(level_sizes(f).max(initial=0)) for f in exp["field"]))
        self.episode = episode.copy()
        return exp


# ---- the closed loop on the CPU --------------------------------------------------------------------------------------------------------
def ray_table(nd, N, T, fov=2 / 3):
    """(nd, 5, N) as rcw_ray_table lays it out, from pyref.World.ray_fan: [dx | dy | |1/dx| | |1/dy| | 0]"""
    w = pyref.World(H=4, W=4, nd=nd, num_rays=N, fov=fov, T=T)
    out = np.zeros((nd, 5, N), T)
    with np.errstate(divide="ignore"):
        for d in range(nd):
            w.dir = d
            for k, (dx, dy) in enumerate(w.ray_fan()):
                out[d, :4, k] = (dx, dy, abs(T(1) / T(dx)), abs(T(1) / T(dy)))
    return out


def explore(walls, goals, pos, dirs, nd, rays, inc, radius, T, limit):
    """walls bool (n, H, W); goals (n, 2) 1-based; pos (n, 2); dirs (n,).  Every agent marks what its rays cross, floods, takes the rule's
    action, until its distance is -1 or it touches its goal.  Returns (steps (n,) — the actions taken, -1: not finished within `limit` —,
    how (n,) — 'explored' / 'goal' / None)."""
    walls = np.asarray(walls, bool)
    n, H, W = walls.shape
    bits = walls.astype(np.uint8)
    for a in range(n):
        bits[a, goals[a][0] - 1, goals[a][1] - 1] |= 2
    table, dtab = ray_table(nd, rays, T), GR.direction_table(nd, T)
    wm = [GR._map(walls[a]) for a in range(n)]
    gm = [GR._map((bits[a] & 2) != 0) for a in range(n)]
    inc, radius = T(inc), T(radius)
    pos, dirs = np.array(pos, T), np.array(dirs, np.int64)
    seen = np.zeros((n, H, W), np.uint8)
    fields = [None] * n
    steps, how = np.full(n, -1), [None] * n
    live = np.ones(n, bool)
    for step in range(limit + 1):
        idx = np.flatnonzero(live)
        if not len(idx):
            break
        marked = SM.marked_tiles(bits[idx], pos[idx], dirs[idx], table, False, T)
        for k, a in enumerate(idx):
            fresh = marked[k] & (seen[a] == 0)
            if fresh.any() or fields[a] is None:
                seen[a][fresh] = 1 + bits[a][fresh]
                fields[a] = flood(seen[a])[0]
            if lookup(fields[a], pos[a]) < 0:
                steps[a], how[a], live[a] = step, "explored", False
                continue
            if step == limit:
                continue
            act, _ = GR.rule(fields[a], pos[a][0], pos[a][1], dirs[a], dtab, inc, T)
            if act == 1:
                x, y = pos[a]
                new = (x + inc * dtab[dirs[a]][0], y + inc * dtab[dirs[a]][1])
                g, w = GR.collides(wm[a], gm[a], new, radius, T)
                if g:
                    steps[a], how[a], live[a] = step + 1, "goal", False
                elif not w:
                    pos[a] = new
            elif act == 3:
                dirs[a] = (dirs[a] + 1) % nd
            else:
                assert act == 4
                dirs[a] = (dirs[a] - 1) % nd
    return steps, how
