"""The guide (include/rcw.h, rcw_set_guide) restated in Python — test infrastructure, not a test.

  rule          the rule for one agent in numpy scalars of the handle's world-unit type, a rounding per operation: the tile and the
                no-advice cases, the next tile, the target (re-centre first), the argmax over the direction table AS IT IS (a NaN
                product sum never wins, an all-NaN table gives 0), the action from delta = (heading - d) mod nd.
  expected      the words of a whole batch from the engine's OWN state: its goal-distance field, positions, headings and table.
  Tracked       an engine with the guide on; `check` compares both words with `expected` after whatever call the test just made, and
                counts what the comparisons saw (agents without advice, each action).
  follow        a small act! (SR:139-191 through oracle.pyref's collision test) that walks ONE agent by the rule until it is done: the
                closed-loop property on the CPU.  bound(l, nd, inc): the promise's step count.
"""
import math

import numpy as np

from oracle import pyref

UNREACHED = 0xFFFF


def rule(field, x, y, d, table, inc, T=np.float32):
    """field: uint16 (H, W), field[i, j] 0-based; (x, y): the position; d: the 0-based heading; table: (nd, 2), row k = (D1, D2); inc:
    position_increment.  Returns (action, heading)."""
    field = np.asarray(field)
    H, W = field.shape
    table = np.asarray(table, dtype=T).reshape(-1, 2)
    nd = len(table)
    x, y, inc = T(x), T(y), T(inc)
    none = (3, -1)
    if not (np.isfinite(x) and np.isfinite(y)):
        return none
    i, j = int(np.floor(x)), int(np.floor(y))
    if not (0 <= i < H and 0 <= j < W):
        return none
    f = int(field[i, j])
    if f == UNREACHED or f == 0:
        return none
    nxt = None
    for a, b in ((i - 1, j), (i + 1, j), (i, j - 1), (i, j + 1)):
        if 0 <= a < H and 0 <= b < W and int(field[a, b]) == f - 1:
            nxt = (a, b)
            break
    if nxt is None:                                                        # (no flood's field: the header gives it the no-advice words)
        return none
    half = T(0.5)
    ct = (T(i) + half, T(j) + half)
    cn = (T(nxt[0]) + half, T(nxt[1]) + half)
    e = y - ct[1] if nxt[0] != i else x - ct[0]
    p = cn if abs(e) <= inc else ct
    vx, vy = T(p[0] - x), T(p[1] - y)
    with np.errstate(all="ignore"):
        s = table[:, 0] * vx + table[:, 1] * vy                            # (elementwise in T: a rounding per operation)
    assert s.dtype == T
    ok = np.flatnonzero(~np.isnan(s))
    heading = int(ok[np.argmax(s[ok])]) if len(ok) else 0                  # (argmax: the first of the greatest)
    delta = (heading - int(d)) % nd
    return (1 if delta == 0 else (3 if delta <= nd // 2 else 4)), heading


def expected(fields, pos, dirs, table, inc, T):
    """(action uint8 (B), heading int32 (B)) of a batch: fields (B, H, W), pos (B, 2), dirs (B)."""
    out = [rule(fields[b], pos[b][0], pos[b][1], dirs[b], table, inc, T) for b in range(len(dirs))]
    return np.array([a for a, _ in out], np.uint8), np.array([h for _, h in out], np.int32)


class Tracked:
    """An engine with the guide on.  Every `check` reads the engine's state — field, position, heading, table — and holds both words to
    the rule; `seen` counts the agents without advice and each action over all checks, so a test can insist on what it reached."""

    def __init__(self, env, enable=True):
        self.env = env
        self.seen = {"no_advice": 0, 1: 0, 3: 0, 4: 0, "checks": 0}
        if enable:
            env.set_guide(True)
        assert env.guide_enabled and env.goal_distance_enabled
        self.inc = env.cfg.position_increment_wu_f64 if env.T is np.float64 else env.cfg.position_increment_wu
        self.check("enabled")

    def check(self, where):
        env, w = self.env, self.env.world
        action, heading = expected(env.goal_distance_field, w.player_position_wu, w.player_direction_au, w.directions_wu, self.inc, env.T)
        got_a, got_h = env.guide_action.numpy(), env.guide_heading.numpy()
        assert got_a.dtype == np.uint8 and got_h.dtype == np.int32 and got_a.shape == got_h.shape == (env.batch,)
        np.testing.assert_array_equal(got_h, heading, err_msg=f"heading {where}")
        np.testing.assert_array_equal(got_a, action, err_msg=f"action {where}")
        self.seen["checks"] += 1
        self.seen["no_advice"] += int((heading < 0).sum())
        for a in (1, 3, 4):
            self.seen[a] += int((action == a).sum())
        return action, heading


# ---- the closed loop on the CPU ------------------------------------------------------------------------------------------------------
def bound(l, nd, inc):
    """the promise: an agent l tiles from its goal arrives within this many steps"""
    return (l + 1) * (nd // 2 + 2 * math.ceil(1 / inc))


def direction_table(nd, T):
    """directions_wu SR:65-69: (cos, sin) of (k - 1) 2 pi / nd computed in Float64 and converted"""
    return np.array([(T(math.cos(k * 2 * math.pi / nd)), T(math.sin(k * 2 * math.pi / nd))) for k in range(nd)], T)


def _map(layer):
    """bool (H, W) -> the 1-based nested lists oracle.pyref's collision test takes"""
    H, W = layer.shape
    m = [[False] * (W + 1) for _ in range(H + 1)]
    for i in range(H):
        for j in range(W):
            m[i + 1][j + 1] = bool(layer[i, j])
    return m


def collides(walls_map, goal_map, pos, radius, T):
    return pyref.is_player_colliding(goal_map, pos, radius, T), pyref.is_player_colliding(walls_map, pos, radius, T)


def follow(walls, field, goal, pos, d, table, inc, radius, T, limit):
    """act!(world, rule's action) until done or `limit` steps: the steps taken, or None where the agent did not arrive.  goal: 1-based."""
    H, W = walls.shape
    goal_layer = np.zeros((H, W), bool)
    goal_layer[goal[0] - 1, goal[1] - 1] = True
    wm, gm = _map(walls), _map(goal_layer)
    inc, radius = T(inc), T(radius)
    nd = len(table)
    x, y, d = T(pos[0]), T(pos[1]), int(d)
    for step in range(1, limit + 1):
        a, _ = rule(field, x, y, d, table, inc, T)
        if a == 1:                                                         # UT:16, SR:162-174
            new = (x + inc * table[d][0], y + inc * table[d][1])
            g, w = collides(wm, gm, new, radius, T)
            if g:
                return step
            if not w:
                x, y = new
        elif a == 3:
            d = (d + 1) % nd
        else:
            assert a == 4
            d = (d - 1) % nd
    return None
