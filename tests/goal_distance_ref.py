"""The goal distance (include/rcw.h, rcw_set_goal_distance) restated in Python — test infrastructure, not a test.

  bfs_field       a deque breadth-first search over ONE (H, W) layout and goal: the uint16 field, 0xFFFF for walls and tiles without a path.
  GoalDistanceRef is fed the engine's OWN state after every call — walls, goal, position, episode counter — plus which agents an explicit
                  call masked, and keeps field, distance, start_distance and progress by the header's table.  State parity with the oracle is
                  the existing suite's job: this checks the new words against the state the engine reports.
  pocket, serpentine   the two layouts the tests share.
"""
from collections import deque

import numpy as np

UNREACHED = 0xFFFF


def bfs_field(walls, goal):
    """walls: bool (H, W), walls[i-1, j-1]; goal: 1-based (i, j).  Distances in tiles between edge neighbours whose WALL bit is clear;
    the GOAL bit plays no part.  A goal inside a wall: every entry 0xFFFF."""
    w = np.asarray(walls) != 0
    H, W = w.shape
    f = np.full((H, W), UNREACHED, np.uint16)
    gi, gj = int(goal[0]) - 1, int(goal[1]) - 1
    if not (0 <= gi < H and 0 <= gj < W) or w[gi, gj]:
        return f
    f[gi, gj] = 0
    q = deque([(gi, gj)])
    while q:
        i, j = q.popleft()
        for ni, nj in ((i - 1, j), (i + 1, j), (i, j - 1), (i, j + 1)):
            if 0 <= ni < H and 0 <= nj < W and not w[ni, nj] and f[ni, nj] == UNREACHED:
                f[ni, nj] = f[i, j] + 1
                q.append((ni, nj))
    return f


def linear(field):
    """The (H, W) field in the tile map's own linear order: tile (i, j), 1-based, at (i - 1) + H (j - 1)."""
    return np.ascontiguousarray(np.asarray(field).T).reshape(-1)


def lookup(field, pos):
    """field[t] for t = wu_to_tu(pos) (utils.jl:5: floor(x) + 1, floor(y) + 1), -1 where that is 0xFFFF or t is off the map."""
    H, W = field.shape
    x, y = float(pos[0]), float(pos[1])
    if not (np.isfinite(x) and np.isfinite(y)):
        return -1
    i, j = int(np.floor(x)), int(np.floor(y))
    if not (0 <= i < H and 0 <= j < W):
        return -1
    v = int(field[i, j])
    return -1 if v == UNREACHED else v


def pocket():
    """7 x 7: the ring plus a closed box of walls around (4, 4), 1-based — a free tile no other free tile reaches."""
    w = np.zeros((7, 7), bool)
    w[[0, -1], :] = True
    w[:, [0, -1]] = True
    for i, j in ((3, 3), (3, 4), (3, 5), (4, 3), (4, 5), (5, 3), (5, 4), (5, 5)):
        w[i - 1, j - 1] = True
    return w


def serpentine(H, W):
    """One corridor that snakes through the whole map: wall rows at every second interior row, each open at alternating ends.  The longest
    distance is about H W / 2 tiles and every breadth-first level holds one tile."""
    w = np.zeros((H, W), bool)
    w[[0, -1], :] = True
    w[:, [0, -1]] = True
    for k, i in enumerate(range(2, H - 2, 2)):                             # 0-based wall rows 2, 4, ...: free rows 1, 3, ...
        w[i, 1:W - 1] = True
        w[i, W - 2 if k % 2 == 0 else 1] = False
    return w


class GoalDistanceRef:
    def __init__(self, walls, goal, pos, episode):
        """The state as of rcw_set_goal_distance(h, 1): every agent flooded, start_distance = distance, progress = 0."""
        self.B = len(goal)
        self.field = [None] * self.B
        self.distance = np.zeros(self.B, np.int32)
        self.start_distance = np.zeros(self.B, np.int32)
        self.progress = np.zeros(self.B, np.int32)
        self.recorded = np.zeros(self.B, np.uint32)
        self.masked(walls, goal, pos, episode, None)

    def _refresh(self, b, walls, goal, pos, episode):
        self.field[b] = bfs_field(walls[b], goal[b])
        self.distance[b] = self.start_distance[b] = lookup(self.field[b], pos[b])
        self.progress[b] = 0
        self.recorded[b] = episode[b]

    def masked(self, walls, goal, pos, episode, mask):
        """rcw_reset / rcw_set_state / rcw_set_walls (and enabling): the mask decides, not the counter; the others keep everything."""
        who = np.ones(self.B, bool) if mask is None else np.asarray(mask).reshape(self.B) != 0
        for b in np.flatnonzero(who):
            self._refresh(b, walls, goal, pos, episode)

    def stepped(self, walls, goal, pos, episode):
        """rcw_step / rcw_step_device: an agent whose episode counter moved is restarted; every other one takes progress = old - new where
        both are >= 0, else 0, and keeps start_distance."""
        for b in range(self.B):
            if int(episode[b]) != int(self.recorded[b]):
                self._refresh(b, walls, goal, pos, episode)
                continue
            old, new = int(self.distance[b]), lookup(self.field[b], pos[b])
            self.progress[b] = old - new if old >= 0 and new >= 0 else 0
            self.distance[b] = new

    @property
    def fields(self):
        return np.stack(self.field)
