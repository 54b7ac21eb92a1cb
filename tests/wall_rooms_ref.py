"""The wall generator's rooms (include/rcw.h, rcw_set_wall_rooms) restated on the CPU — the specification, test infrastructure, not a test.

ROOMS FROM ONE 64-BIT KEY, rooms(m, H, W, room, stop, doors) for H, W >= 5, with draw(m, n) and below(u, r) of walls_ref.py
(csrc/rcw_rng.h); tiles are 0-based (i, j) with index t = i + H j.  The ring is WALL, the interior starts free.  A chamber is a rectangle
of interior tiles [i0..i1] x [j0..j1], bounds inclusive; the root is [1..H-2] x [1..W-2].  A chamber's draws have the indices n + k,
n = 2^61 + 8 ((t0 << 16) | t1), t0 = i0 + H j0, t1 = i1 + H j1:

    walls     row walls R = {even i: i0 + room <= i <= i1 - room}, empty unless j1 > j0; column walls C = {even j: j0 + room <= j <=
              j1 - room}, empty unless i1 > i0; both empty: a room
    stop      a chamber other than the root is a room where (draw(m, n + 1) >> 32) < stop
    side      the non-empty one of R, C; of two a row wall where i1 - i0 > j1 - j0, a column wall where it is shorter, on a tie a row wall
              where bit 63 of draw(m, n) is set
    line      s = the below(draw(m, n + 2), |S|)-th element of the chosen set, ascending
    doors     the span lo .. hi on line s (j0 .. j1 for a row wall, i0 .. i1 for a column wall); cnt = (hi - lo) // 2 + 1 candidates lo,
              lo + 2, ...; the first door at lo + 2 below(draw(m, n + 3), cnt), and where (draw(m, n + 4) >> 32) < doors a second at
              lo + 2 below(draw(m, n + 5), cnt); every other tile of the span is WALL
    children  the rectangles on either side of line s

THE KEY OF AN EPISODE is the generator's (wall_generator_ref.maze_key), and after it the rule is the bank's.

`rooms` is the rule by recursion.  `rounds` restates the kernel's traversal (csrc/rcw_wall_bank.hip, rcw_wall_rooms_kernel's header): a
list of chambers, every live one cut once a round, one child in its place and the other appended; it returns the layout, the number of
rounds and the most chambers a round handled.  The reference that applies the rule is wall_family.WallFamilyRef; its `events` count
rooms_made and second_doors (walls with two distinct doors).
"""
import numpy as np

import wall_generator_ref as WG
import walls_ref as WR

ROOMS_DRAW = 1 << 61
MAX_ROOMS = 4096
MAX_TILES = 65536
DEFAULT_ROOM, DEFAULT_STOP, DEFAULT_DOORS = 2, 0.25, 0.25

word = WG.loops_word                                                           # a probability as the UInt32 the rule compares with


def bound(H, W):
    """Q: every room holds an (odd, odd) tile"""
    return -(-(H - 2) // 2) * -(-(W - 2) // 2)


def draw_index(H, c):
    i0, i1, j0, j1 = c
    return ROOMS_DRAW + 8 * (((i0 + H * j0) << 16) | (i1 + H * j1))


def cut(m, H, W, c, room, stop, doors):
    """One chamber (i0, i1, j0, j1): None where it is a room, else (row, s, doors, wall tiles, the two children)."""
    i0, i1, j0, j1 = c
    R = [i for i in range(i0 + room, i1 - room + 1) if i % 2 == 0] if j1 > j0 else []
    C = [j for j in range(j0 + room, j1 - room + 1) if j % 2 == 0] if i1 > i0 else []
    if not R and not C:
        return None
    n = draw_index(H, c)
    if c != (1, H - 2, 1, W - 2) and (WR.draw(m, n + 1) >> 32) < stop:
        return None
    if R and C:
        row = i1 - i0 > j1 - j0 if i1 - i0 != j1 - j0 else bool(WR.draw(m, n) >> 63)
    else:
        row = bool(R)
    S = R if row else C
    s = S[WR.below(WR.draw(m, n + 2), len(S))]
    lo, hi = (j0, j1) if row else (i0, i1)
    cnt = (hi - lo) // 2 + 1
    gaps = [lo + 2 * WR.below(WR.draw(m, n + 3), cnt)]
    if (WR.draw(m, n + 4) >> 32) < doors:
        gaps.append(lo + 2 * WR.below(WR.draw(m, n + 5), cnt))
    tiles = [(s, x) if row else (x, s) for x in range(lo, hi + 1) if x not in gaps]
    kids = ((i0, s - 1, j0, j1), (s + 1, i1, j0, j1)) if row else ((i0, i1, j0, s - 1), (i0, i1, s + 1, j1))
    return row, s, gaps, tiles, kids


def _defaults(room, stop, doors):
    return (DEFAULT_ROOM if room is None else room, word(DEFAULT_STOP) if stop is None else stop, word(DEFAULT_DOORS) if doors is None else doors)


def rooms(m, H, W, room=None, stop=None, doors=None, details=False):
    """bool (H, W), walls[i, j] 0-based = tile (i + 1, j + 1) is a WALL; stop and doors are the UInt32 words (None: the defaults').
    details: (walls, the rooms as (i0, i1, j0, j1), the walls as (row, s, doors, chamber), the deepest recursion)."""
    room, stop, doors = _defaults(room, stop, doors)
    assert H >= 5 and W >= 5 and room >= 1 and 0 <= stop <= 0xFFFFFFFF and 0 <= doors <= 0xFFFFFFFF and H * W <= MAX_TILES
    w = np.ones((H, W), bool)
    w[1:-1, 1:-1] = False
    leaves, cuts, deepest = [], [], [0]

    def split(c, depth):
        deepest[0] = max(deepest[0], depth)
        r = cut(m, H, W, c, room, stop, doors)
        if r is None:
            leaves.append(c)
            return
        row, s, gaps, tiles, kids = r
        for i, j in tiles:
            assert not w[i, j], "a wall over a wall"
            w[i, j] = True
        cuts.append((row, s, tuple(gaps), c))
        for k in kids:
            split(k, depth + 1)

    import sys
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 10000))
    try:
        split((1, H - 2, 1, W - 2), 0)
    finally:
        sys.setrecursionlimit(old)
    return (w, leaves, cuts, deepest[0]) if details else w


def rounds(m, H, W, room=None, stop=None, doors=None):
    """The kernel's rounds: (walls, rounds, widest, entries).  A round takes every live chamber of the list as it found it: a room is flagged,
    a cut chamber is overwritten by the child in front of the line and the other is appended.  `rounds` counts the rounds that handled a live
    chamber (the deepest recursion + 1), `widest` the most live chambers a round found, `entries` the list's final length (<= Q)."""
    room, stop, doors = _defaults(room, stop, doors)
    w = np.ones((H, W), bool)
    w[1:-1, 1:-1] = False
    chambers, live = [(1, H - 2, 1, W - 2)], [True]
    count = widest = 0
    while True:
        n = len(chambers)
        todo = [e for e in range(n) if live[e]]
        if not todo:
            break
        count += 1
        widest = max(widest, len(todo))
        for e in todo:
            r = cut(m, H, W, chambers[e], room, stop, doors)
            if r is None:
                live[e] = False
                continue
            for i, j in r[3]:
                w[i, j] = True
            chambers[e] = r[4][0]
            chambers.append(r[4][1])
            live.append(True)
        assert len(chambers) <= bound(H, W)
    return w, count, widest, len(chambers)


def install_refusal(H, W, room, levels, first_level):
    """what rcw_set_wall_rooms says of a geometry, a room side and a level range: None, "invalid" or "unsupported" """
    if H < 5 or W < 5 or room < 1 or levels < 0 or first_level < 0 or first_level + levels > 2 ** 31 - 1:
        return "invalid"
    return "unsupported" if bound(H, W) > MAX_ROOMS or H * W > MAX_TILES else None
