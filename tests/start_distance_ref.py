"""The start rule (include/rcw.h, "the start rule") restated on the CPU — test infrastructure, not a test.

Independent of the library: the generator is tests/walls_ref.py's Python integers (episode_key, draw, below), the flood a plain queue.

  field(walls, goal)            step 1: int array (H, W), -1 on walls and on what the goal does not reach
  start_rule(...)               steps 1 to 4 for one agent: ((i, j) 1-based or None, outcome)
  StartRef                      tests/walls_ref.py's WallsRef with the rule applied behind every reset!(world) of an agent — reset, set_walls
                                and the restart of a done agent under auto_reset (and, through tests/time_limit_ref.py's TimeLimitRef, of a
                                truncated one).  `placed` is the UInt8 word; `band` may be changed between calls; band None: the rule is off
                                and the reference is WallsRef.  `unruled_start` keeps, per agent, the distance of the tile reset! drew — what
                                the start would have been without the rule.
"""
import collections

import numpy as np

import walls_ref as WR

START_DRAW = (1 << 63) + (1 << 62)
MAX = 65534
NOT_YET, IN_BAND, CLAMPED, KEPT = 0, 1, 2, 3


def valid_band(lo, hi):
    return 1 <= lo <= hi <= MAX


def field(walls, goal):
    """the breadth-first field from the 1-based goal (gi, gj) through `walls` (bool (H, W)), 4-neighbour; -1: a wall, or not reached"""
    w = np.asarray(walls) != 0
    H, W = w.shape
    F = np.full((H, W), -1, np.int64)
    gi, gj = int(goal[0]) - 1, int(goal[1]) - 1
    if not (0 <= gi < H and 0 <= gj < W) or w[gi, gj]:
        return F
    F[gi, gj] = 0
    todo = collections.deque([(gi, gj)])
    while todo:
        i, j = todo.popleft()
        for a, b in ((i - 1, j), (i + 1, j), (i, j - 1), (i, j + 1)):
            if 0 <= a < H and 0 <= b < W and not w[a, b] and F[a, b] < 0:
                F[a, b] = F[i, j] + 1
                todo.append((a, b))
    return F


def start_rule(walls, goal, key, lo, hi):
    """((i, j) 1-based | None, outcome) — steps 1 to 4 of the rule"""
    assert valid_band(lo, hi)
    F = field(walls, goal)
    H, W = F.shape
    lin = F.T.reshape(-1)                                                       # tile (i, j) at t = (i - 1) + H (j - 1)
    E = np.flatnonzero((lin >= lo) & (lin <= hi))
    outcome = IN_BAND
    if E.size == 0:
        D = int(lin.max())
        if D < 1:
            return None, KEPT
        E, outcome = np.flatnonzero(lin == D), CLAMPED
    t = int(E[WR.below(WR.draw(key, START_DRAW), int(E.size))])
    return (t % H + 1, t // H + 1), outcome


class StartRef(WR.WallsRef):
    def __init__(self, *args, band=None, **kw):
        self.band = band
        batch = args[0] if args else kw["batch"]
        self.placed = np.zeros(batch, np.uint8)
        self.unruled_start = np.full(batch, -2, np.int64)
        self.outcomes = collections.Counter()
        super().__init__(*args, **kw)

    def _reset_agent(self, b):
        e = int(self.episode[b])                                                # the counter before the increment
        super()._reset_agent(b)
        w = self.worlds[b]
        F = field(self.walls_of(b), w.goal)
        self.unruled_start[b] = F[int(np.floor(w.pos[0])), int(np.floor(w.pos[1]))]
        if self.band is None:
            return
        tile, outcome = start_rule(self.walls_of(b), w.goal, WR.episode_key(self.seed, self.offset + b, e), *self.band)
        self.placed[b] = outcome
        self.outcomes[outcome] += 1
        if tile is not None:
            w.set_state(w.goal, (self.T(tile[0] - 0.5), self.T(tile[1] - 0.5)), w.dir)
            self._account_rays(b)

    def distance(self):
        """each agent's distance to its goal now (-1: none): what goal_distance reports"""
        out = np.empty(self.B, np.int64)
        for b, w in enumerate(self.worlds):
            out[b] = field(self.walls_of(b), w.goal)[int(np.floor(w.pos[0])), int(np.floor(w.pos[1]))]
        return out


# ---- the hand-made maps of the issue ------------------------------------------------------------------------------------------------
def ring(H, W):
    w = np.zeros((H, W), bool)
    w[[0, -1], :] = True
    w[:, [0, -1]] = True
    return w


def corridor():
    """5 x 70, walls on rows 2 and 4: a one-tile corridor of 68 tiles, wider than a wavefront"""
    w = ring(5, 70)
    w[1, :] = True
    w[3, :] = True
    return w


def islands():
    """7 x 7 whose free interior tiles are all isolated single cells"""
    w = np.ones((7, 7), bool)
    for i in (1, 3, 5):
        for j in (1, 3, 5):
            w[i, j] = False
    return w


def two_rooms():
    """9 x 12, two sealed rooms of different sizes: columns 2..4 and columns 6..11"""
    w = ring(9, 12)
    w[:, 4] = True
    return w


def four_rooms():
    import raycastworlds_jl_amd as RCW

    return np.asarray(RCW.layouts.four_rooms(8, 8)) != 0


# name: (walls, band, seed)
MAPS = dict(CORRIDOR=(corridor, (60, 65), 11), ISLANDS=(islands, (1, 2), 5), TWO_ROOMS=(two_rooms, (1, MAX), 3), FOUR_ROOMS=(four_rooms, (3, 4), 9))
