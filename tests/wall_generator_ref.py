"""The wall generator (include/rcw.h, rcw_set_wall_generator) restated on the CPU — the specification, test infrastructure, not a test.

A MAZE FROM ONE 64-BIT KEY, maze(m, H, W, loops) for H, W >= 5, with draw(m, n) of walls_ref.py (csrc/rcw_rng.h):

    cells   the tiles with odd 0-based (i, j) inside the ring: ni = (H-1)//2, nj = (W-1)//2, C = ni nj, cell c = ci nj + cj on tile
            (2ci+1, 2cj+1) — layouts.maze's grid; with an even H or W the last interior row or column stays wall
    edges   east of c: id 2c, where cj+1 < nj, passage tile (2ci+1, 2cj+2); south of c: id 2c+1, where ci+1 < ni, passage (2ci+2, 2cj+1)
    order   w(id) = (draw(m, id) & 0xFFFFFFFFFFF00000) | id — ids stay below 2^20, so the words are distinct
    tree    the minimum spanning tree of the cell grid under w (unique); here: Kruskal by sorting w
    loops   a non-tree edge is opened too where (draw(m, 2C + id) >> 32) < loops (UInt32; 0: a perfect maze)
    every tile is WALL except the cells and the passage tiles of tree edges and opened edges

THE KEY OF AN EPISODE, with g the global agent id and e the counter before the increment: key = episode_key(seed, g, e),
u = draw(key, 2^63) — the bank's draw index.  levels == 0: m = u, wall_layout = -1.  levels >= 1: l = first_level + below(u, levels),
m = episode_key(level_seed, l, 0), wall_layout = l.  After that the rule is the bank's: WALL := the maze, GOAL cleared, the reset of
walls_ref.py against the new walls under `key` from draw 0, counter = e + 1 (once).

The reference that applies the rule, wall_family.WallFamilyRef, is WallsRef with that one override of _reset_agent, as WallBankRef is; this
module is the maze, its key and the restatement of the kernel's rounds.
"""
import numpy as np

import walls_ref as WR

LAYOUT_DRAW = 1 << 63
ORDER_MASK = 0xFFFFFFFFFFF00000
MAX_CELLS = 4096


def loops_word(p):
    """a probability in [0, 1] as the UInt32 the rule compares with"""
    return min(int(float(p) * 2.0 ** 32), 0xFFFFFFFF)


def grid(H, W):
    ni, nj = (H - 1) // 2, (W - 1) // 2
    return ni, nj, ni * nj


def edges(H, W):
    """every edge of the cell grid: (id, cell, other cell, passage tile (i, j) 0-based)"""
    ni, nj, _ = grid(H, W)
    out = []
    for ci in range(ni):
        for cj in range(nj):
            c = ci * nj + cj
            if cj + 1 < nj:
                out.append((2 * c, c, c + 1, (2 * ci + 1, 2 * cj + 2)))
            if ci + 1 < ni:
                out.append((2 * c + 1, c, c + nj, (2 * ci + 2, 2 * cj + 1)))
    return out


def order_word(m, eid):
    return (WR.draw(m, eid) & ORDER_MASK) | eid


def tree_edges(m, H, W):
    """the ids of the minimum spanning tree's edges: Kruskal, the edges sorted by their order words, a plain union-find"""
    _, _, C = grid(H, W)
    parent = list(range(C))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    took = []
    for _, eid, a, b in sorted((order_word(m, e[0]), e[0], e[1], e[2]) for e in edges(H, W)):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
            took.append(eid)
    return took


def boruvka(m, H, W):
    """the kernel's rounds (csrc/rcw_wall_bank.hip, rcw_wall_generator_kernel's header) restated: (the tree's edge ids sorted, the rounds, the
    longest hook chain).  A round — offer: every edge that joins two labels offers its order word to both labels' slots, the smallest stays;
    pick: every root with an offer takes the winning edge into the tree and notes the label across it; hook: the root hangs itself under
    that label, but of two roots that picked each other the smaller stays a root; jump: every cell takes its root's root until nothing
    moves.  The chain of a round is the largest number of hooks between a root of the round and the root it ends under — what the
    pointer jumping has to shorten; the third value is the largest chain of any round.  Rounds run until one label is left: the model has
    no cap (the kernel's is 13)."""
    _, nj, C = grid(H, W)
    offers = [(order_word(m, e[0]), e[1], e[2]) for e in edges(H, W)]
    label = list(range(C))
    tree, rounds, deepest = set(), 0, 0
    while any(l != label[0] for l in label):
        rounds += 1
        slot = {}                                                              # offer
        for w, a, b in offers:
            la, lb = label[a], label[b]
            if la != lb:
                if w < slot.get(la, 1 << 64):
                    slot[la] = w
                if w < slot.get(lb, 1 << 64):
                    slot[lb] = w
        across = {}                                                            # pick
        for root, w in slot.items():
            eid = w & 0xFFFFF
            a = eid >> 1
            b = a + (nj if eid & 1 else 1)
            tree.add(eid)
            la, lb = label[a], label[b]
            assert root in (la, lb) and la != lb
            across[root] = lb if la == root else la
        up = {}                                                                # hook
        for root, other in across.items():
            if not (across.get(other) == root and root < other):
                up[root] = other
        top, depth = {}, {}                                                    # jump
        for r in up:
            path = []
            while r in up and r not in top:
                path.append(r)
                r = up[r]
                assert len(path) <= C                                          # (a cycle: the words were not distinct)
            end, d = (top[r], depth[r]) if r in top else (r, 0)
            for q in reversed(path):
                d += 1
                top[q], depth[q] = end, d
        deepest = max(deepest, max(depth.values()))
        label = [top.get(l, l) for l in label]
    return sorted(tree), rounds, deepest


def maze(m, H, W, loops=0):
    """bool (H, W), walls[i, j] 0-based = tile (i + 1, j + 1) is a WALL; loops is the UInt32 word"""
    assert H >= 5 and W >= 5 and 0 <= loops <= 0xFFFFFFFF
    ni, nj, C = grid(H, W)
    assert 2 * C < (1 << 20)
    w = np.ones((H, W), bool)
    w[1:2 * ni:2, 1:2 * nj:2] = False
    tree = set(tree_edges(m, H, W))
    for eid, _, _, (i, j) in edges(H, W):
        if eid in tree or (WR.draw(m, 2 * C + eid) >> 32) < loops:
            w[i, j] = False
    return w


def maze_key(seed, global_agent, episode, levels=0, first_level=0, level_seed=0):
    """(m, wall_layout) of the episode `episode` (the counter before the increment) of a global agent"""
    assert levels >= 0 and first_level >= 0 and first_level + levels <= 2 ** 31 - 1
    u = WR.draw(WR.episode_key(seed, global_agent, episode), LAYOUT_DRAW)
    if levels == 0:
        return u, -1
    level = first_level + WR.below(u, levels)
    return WR.episode_key(level_seed, level, 0), level


def install_refusal(H, W, levels, first_level):
    """what rcw_set_wall_generator says of a geometry and a level range: None, "invalid" or "unsupported" """
    if H < 5 or W < 5 or levels < 0 or first_level < 0 or first_level + levels > 2 ** 31 - 1:
        return "invalid"
    return "unsupported" if grid(H, W)[2] > MAX_CELLS else None
