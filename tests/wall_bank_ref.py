"""The wall bank (include/rcw.h, rcw_set_wall_bank) restated on the CPU — the specification, test infrastructure, not a test.

A handle with a bank holds L layouts, each valid as rcw_set_walls wants one (ring present, two free interior tiles), and UInt32 weights
w[0..L-1] (None: all 1) with 1 <= sum <= 2^32 - 1; cum[k] = w[0] + ... + w[k].  An agent BEGINS AN EPISODE whenever its episode counter
moves: a reset, a done or truncated restart under auto_reset, and the call that installs the bank.  With g = agent_id_offset + a and e the
counter before the increment:

    key = episode_key(seed, g, e)                  the key the reset of that episode already uses (walls_ref.py, from csrc/rcw_rng.h)
    u   = draw(key, 2^63)                          the reset's own draw indices count from 0 and stay below 4 + 3 * 1024 * H * W
    k   = the smallest index with cum[k] > below(u, sum)
    WALL layer := layout k, GOAL layer cleared, wall_layout[a] := k
    then the reset of walls_ref.py against the new walls: the same key, draw indices from 0, counter = e + 1 (once)

WallBankRef is WallsRef with that one override of _reset_agent; everything else — the step under auto_reset, set_state, the snapshot, the
composition TimeLimitRef(WallBankRef(...), L, seed, True) — is inherited.  `events` also counts
    episode_starts   agents that began an episode under the bank
    layout_changed   ... and drew another layout than the one they had
    layout_kept      ... and drew the one they had again
and `layouts_drawn` is the set of layouts drawn so far.  The install itself counts as episode_starts only: the agents had no layout before.
"""
import numpy as np

import walls_ref as WR
from oracle import pyref

LAYOUT_DRAW = 1 << 63


def cumulative(weights, layouts):
    """cum[k] = w[0] + ... + w[k] in Python integers (weights None: all 1); the sum must lie in 1 .. 2^32 - 1"""
    w = [1] * layouts if weights is None else [int(x) for x in weights]
    assert len(w) == layouts and all(0 <= x <= 0xFFFFFFFF for x in w)
    cum, s = [], 0
    for x in w:
        s += x
        cum.append(s)
    if not 1 <= s <= 0xFFFFFFFF:
        raise ValueError(f"weights sum to {s}: outside 1 .. 2^32 - 1")
    return cum


def index_of(r, cum):
    """the smallest k with cum[k] > r, for 0 <= r < cum[-1] — a plain scan: the engine's binary search must agree with it"""
    for k, c in enumerate(cum):
        if c > r:
            return k
    raise AssertionError((r, cum))


def layout_draw(seed, global_agent, episode, cum):
    """the layout an agent's episode `episode` (the counter before the increment) is given"""
    key = WR.episode_key(seed, global_agent, episode)
    return index_of(WR.below(WR.draw(key, LAYOUT_DRAW), cum[-1]), cum)


def valid_layout(walls):
    """rcw_set_walls' two conditions on one layout (bool (H, W))"""
    w = np.asarray(walls) != 0
    ring = w[0, :].all() and w[-1, :].all() and w[:, 0].all() and w[:, -1].all()
    return bool(ring) and int((~w[1:-1, 1:-1]).sum()) >= 2


class WallBankRef(WR.WallsRef):
    def __init__(self, *args, **kw):
        self.bank = self.cum = None
        super().__init__(*args, **kw)
        self.wall_layout = np.zeros(self.B, np.int32)
        self.events.update(episode_starts=0, layout_changed=0, layout_kept=0)
        self.layouts_drawn = set()

    # ---- the rule ------------------------------------------------------------------------------------------------------------------
    def _reset_agent(self, b):
        if self.bank is not None:
            k = layout_draw(self.seed, self.offset + b, int(self.episode[b]), self.cum)
            tm = self.worlds[b].tile_map
            for i in range(1, self.H + 1):
                for j in range(1, self.W + 1):
                    tm[pyref.WALL][i][j] = bool(self.bank[k, i - 1, j - 1])
                    tm[pyref.GOAL][i][j] = False
            self.events["episode_starts"] += 1
            if not self._installing:
                self.events["layout_kept" if k == self.wall_layout[b] else "layout_changed"] += 1
            self.layouts_drawn.add(k)
            self.wall_layout[b] = k
        super()._reset_agent(b)

    # ---- the calls -----------------------------------------------------------------------------------------------------------------
    def set_wall_bank(self, walls, weights=None):
        """rcw_set_wall_bank: install (every agent restarts under the rule with the current seed) or, walls None, switch off (walls kept)"""
        if walls is None:
            self.bank = self.cum = None
            return
        walls = np.asarray(walls) != 0
        walls = walls[None] if walls.ndim == 2 else walls
        assert walls.shape[1:] == (self.H, self.W) and all(valid_layout(w) for w in walls)
        self.cum = cumulative(weights, len(walls))
        self.bank = walls
        self._installing = True
        try:
            self.reset()
        finally:
            self._installing = False

    _installing = False

    def set_weights(self, weights):
        """rcw_set_wall_bank_weights: they hold from each agent's next episode start; no agent is touched"""
        assert self.bank is not None
        self.cum = cumulative(weights, len(self.bank))

    def set_walls(self, walls, index=None, mask=None):
        if self.bank is not None:
            raise RuntimeError("rcw_set_walls is refused while the handle has a bank")
        super().set_walls(walls, index, mask)

    def snapshot(self):
        return dict(super().snapshot(), wall_layout=self.wall_layout.copy())


def assert_equal(env, ref, where=""):
    """walls_ref.assert_equal plus wall_layout (while the reference has a bank: without one the engine refuses the getter)"""
    r = ref if isinstance(ref, dict) else ref.snapshot()
    WR.assert_equal(env, r, where)
    if env.wall_bank_info["layouts"]:
        got = env.wall_layout.numpy()
        assert got.dtype == np.int32
        np.testing.assert_array_equal(got, r["wall_layout"], err_msg=f"wall_layout {where}")
