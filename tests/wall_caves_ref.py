"""The wall generator's caves (include/rcw.h, rcw_set_wall_caves) restated on the CPU — the specification, test infrastructure, not a test.

A CAVE FROM ONE 64-BIT KEY, cave(m, H, W, fill, smooth) for H, W >= 5, with draw(m, n) of walls_ref.py (csrc/rcw_rng.h); tiles are 0-based
(i, j) with index t = i + H j:

    ring      every tile with i in {0, H-1} or j in {0, W-1} is WALL, at every stage
    gen 0     an interior tile t is WALL where (draw(m, 2^62 + t) >> 32) < fill (UInt32: 0 an empty room, 2^32 - 1 all wall)
    smooth    `smooth` times (0 .. 8), synchronously: WALL in g + 1 where at least 5 of the 3 x 3 around the tile, itself included, are WALL in g
    regions   the 4-connected components of free tiles; the largest is kept, of several largest the one with the smallest tile index t;
              every other free tile becomes WALL
    fallback  need = max(7, (H-2)(W-2) // 4); a kept region of fewer tiles (or none): the layout is maze(m, H, W, 0) of wall_generator_ref.py

THE KEY OF AN EPISODE is the generator's (wall_generator_ref.maze_key), and after it the rule is the bank's.

The reference that applies the rule is wall_family.WallFamilyRef; its `events` count fallbacks (episode starts whose layout is the maze).

`labelling` restates the kernel's rounds (csrc/rcw_wall_bank.hip, rcw_wall_caves_kernel's header), as wall_generator_ref.boruvka restates
the maze's.
"""
import numpy as np

import wall_generator_ref as WG
import walls_ref as WR

CAVE_DRAW = 1 << 62
MAX_TILES = 4096
MAX_SMOOTH = 8
DEFAULT_FILL, DEFAULT_SMOOTH = 0.40, 2

fill_word = WG.loops_word                                                      # a probability as the UInt32 the rule compares with


def need(H, W):
    return max(7, ((H - 2) * (W - 2)) // 4)


def generation0(m, H, W, fill):
    """bool (H, W): True = WALL"""
    g = np.ones((H, W), bool)
    for j in range(1, W - 1):
        for i in range(1, H - 1):
            g[i, j] = (WR.draw(m, CAVE_DRAW + i + H * j) >> 32) < fill
    return g


def smooth_once(g):
    """one synchronous step of the automaton on a bool (H, W) whose ring is WALL"""
    H, W = g.shape
    n = np.zeros((H, W), np.int32)
    gi = g.astype(np.int32)
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            n[1:-1, 1:-1] += gi[1 + di:H - 1 + di, 1 + dj:W - 1 + dj]
    out = np.ones((H, W), bool)
    out[1:-1, 1:-1] = n[1:-1, 1:-1] >= 5
    return out


def smoothed(m, H, W, fill, smooth):
    g = generation0(m, H, W, fill)
    for _ in range(smooth):
        g = smooth_once(g)
    return g


def regions(g):
    """the 4-connected regions of free tiles of a bool (H, W), by a stack flood fill: a list of sorted lists of tile indices t = i + H j, in
    the order of their smallest tile"""
    H, W = g.shape
    seen = g.copy()
    out = []
    for j in range(W):
        for i in range(H):
            if seen[i, j]:
                continue
            seen[i, j] = True
            stack, tiles = [(i, j)], []
            while stack:
                a, b = stack.pop()
                tiles.append(a + H * b)
                for c, d in ((a - 1, b), (a + 1, b), (a, b - 1), (a, b + 1)):
                    if not seen[c, d]:                                         # (a free tile is interior: all four exist)
                        seen[c, d] = True
                        stack.append((c, d))
            out.append(sorted(tiles))
    return out


def kept_region(g):
    """the tiles of the region rule 4 keeps (sorted), or [] where there is no free tile"""
    best = []
    for r in regions(g):                                                       # (in the order of their smallest tile: a later one must be strictly larger)
        if len(r) > len(best):
            best = r
    return best


def cave(m, H, W, fill=None, smooth=DEFAULT_SMOOTH, return_fell_back=False):
    """bool (H, W), walls[i, j] 0-based = tile (i + 1, j + 1) is a WALL; fill is the UInt32 word (None: the default's)"""
    fill = fill_word(DEFAULT_FILL) if fill is None else fill
    assert H >= 5 and W >= 5 and 0 <= fill <= 0xFFFFFFFF and 0 <= smooth <= MAX_SMOOTH
    kept = kept_region(smoothed(m, H, W, fill, smooth))
    if len(kept) < need(H, W):
        w = WG.maze(m, H, W, 0)
        return (w, True) if return_fell_back else w
    w = np.ones((H, W), bool)
    for t in kept:
        w[t % H, t // H] = False
    return (w, False) if return_fell_back else w


def labelling(g):
    """The kernel's labelling rounds on a bool (H, W) (True = WALL), over the interior tiles q = (i - 1) + (H - 2)(j - 1): (labels, rounds).
    labels[q] is -1 on a wall, else the smallest q of the tile's region.  A round — hook: every free tile takes the smallest label among
    itself and its free 4-neighbours (read as the round found them) and the tile its label named is lowered to that one too; jump: every
    tile takes its label's label until nothing moves.  Rounds run until a hook moves nothing; that last, idle hook is not counted.  The
    kernel's lanes may read labels a neighbour lowered in the same round, so its count can be smaller, never its result different."""
    H, W = g.shape
    h, w = H - 2, W - 2
    free = ~g[1:-1, 1:-1]
    big = h * w
    lab = np.where(free, np.arange(big).reshape(w, h).T, big).astype(np.int64)      # lab[ii, jj], q = ii + h jj; `big` on walls
    rounds = 0
    while True:
        least = lab.copy()
        least[1:, :] = np.minimum(least[1:, :], lab[:-1, :])
        least[:-1, :] = np.minimum(least[:-1, :], lab[1:, :])
        least[:, 1:] = np.minimum(least[:, 1:], lab[:, :-1])
        least[:, :-1] = np.minimum(least[:, :-1], lab[:, 1:])
        moved = free & (least < lab)
        if not moved.any():
            break
        rounds += 1
        flat = lab.T.reshape(-1).copy()                                              # flat[q]
        lq = least.T.reshape(-1)
        idx = np.flatnonzero(moved.T.reshape(-1))
        np.minimum.at(flat, flat[idx], lq[idx])                                      # the tile the label named ...
        np.minimum.at(flat, idx, lq[idx])                                            # ... and the tile itself
        while True:                                                                  # jump
            ok = flat < big
            nxt = flat.copy()
            nxt[ok] = flat[flat[ok]]
            if (nxt == flat).all():
                break
            flat = nxt
        lab = flat.reshape(w, h).T
    out = lab.T.reshape(-1).copy()
    out[out == big] = -1
    return out, rounds


def kept_by_labels(g):
    """rule 4 from `labelling`, the kernel's way: sizes per root, the largest (size << 16) | (0xFFFF - root) wins; the kept tiles t, sorted"""
    H, W = g.shape
    h = H - 2
    labels, _ = labelling(g)
    roots, sizes = np.unique(labels[labels >= 0], return_counts=True)
    if len(roots) == 0:
        return []
    word = max((int(s) << 16) | (0xFFFF - int(r)) for r, s in zip(roots, sizes))
    root = 0xFFFF - (word & 0xFFFF)
    return sorted(int((q % h + 1) + H * (q // h + 1)) for q in np.flatnonzero(labels == root))


def install_refusal(H, W, smooth, levels, first_level):
    """what rcw_set_wall_caves says of a geometry, a smoothing count and a level range: None, "invalid" or "unsupported" """
    if H < 5 or W < 5 or not 0 <= smooth <= MAX_SMOOTH or levels < 0 or first_level < 0 or first_level + levels > 2 ** 31 - 1:
        return "invalid"
    return "unsupported" if (H - 2) * (W - 2) > MAX_TILES else None
