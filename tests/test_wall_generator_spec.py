"""The wall generator's specification (tests/wall_generator_ref.py) anchored on the CPU: the maze rule by hand at 5 x 5 and 5 x 7, the
tree's size, connectivity and ring at every shape of the suite, loops as a subset, the level rule, the library's two host exports
(rcw_wall_generator_key, rcw_wall_generator_layout: Kruskal in C++, no device) against the reference byte for byte, sharding — and a
rehearsal, without frames, of every scenario the GPU tests play (tests/wall_generator_cases.py), asserting from the reference's own counts
that each reaches restarts of both kinds and goal redraws:

    scenario   episode_starts  goal_redraws  restarts_after_done  restarts_after_truncation  mazes
    small      470             167           22                   381                        470
    square      36              45            3                    24                         36
    big         48              25            8                    24                         48   (eight agents are walked into their goals)
    wide        24              13            3                    13                         24   (three are)
    huge        12               9            2                     2                         12   (two are)
    f64         31              11            2                    19                         31
    levels     201             121            6                   128                          3   (three levels: three mazes)
    features    51              66            5                    30                         51
    calls       97             123           17                    34                         80
    edge        12              16            2                     2                         12   (`huge`'s script at 4096 cells: 129 x 129)
    edge_rows64 12              16            2                     2                         12   (the same with 64 camera rows, for the one-launch step)
    edge_even   12               4            2                     2                         12   (130 x 130)
    thin        12               6            2                     2                         12   (5 x 4097)
    tall        12               8            2                     2                         12   (4097 x 5)
    thin_even   12               9            2                     2                         12   (6 x 4098)

THE KERNEL'S ALGORITHM, wall_generator_ref.boruvka: the rounds of offer, pick, hook and jump as the kernel's header describes them, in plain
Python, against Kruskal — the same tree at every shape of the suite (200 keys a shape up to 9 x 9, 36 at the larger ones: some 14 s on
this CPU, both trees of every key).  It also counts the rounds and the longest hook chain, which lets the GPU tests choose their mazes: with levels=1 every agent's
maze key is episode_key(level_seed, first_level, 0).  Levels 0 .. 149 under level seed 9 (33 x 33: 0 .. 299), some 13 s on this CPU, 4 to 5 s a large shape:

    shape        rounds: levels           hook chain: levels                       the hardest (most rounds, then the deepest chain)
    129 x 129    6: 99, 7: 51             5: 10, 6: 96, 7: 38, 8: 6                level 32 (7 rounds, chain 8)
    5 x 4097     7: 78, 8: 72             5: 39, 6: 94, 7: 16, 8: 1                level 31 (8, 7)
    4097 x 5     7: 78, 8: 72             5: 30, 6: 96, 7: 23, 8: 1                level 141 (8, 8)
    33 x 33      4: 209, 5: 91            3: 6, 4: 101, 5: 152, 6: 39, 7: 2        level 1 (5, 6; the first of its kind)

Random keys come nowhere near the kernel's cap of 13 rounds (ceil(log2 4096) = 12 is the worst case of any order): eight is what a search
of this size finds, and the GPU tests claim no more.

The exports are missing from the build before this feature: the tests that call them fail there.
"""
import numpy as np
import pytest

import wall_generator_cases as C
import wall_generator_ref as WG
import walls_ref as WR

COLUMNS = ("episode_starts", "goal_redraws", "restarts_after_done", "restarts_after_truncation")
REHEARSED = dict(small=(470, 167, 22, 381), square=(36, 45, 3, 24), big=(48, 25, 8, 24), wide=(24, 13, 3, 13), huge=(12, 9, 2, 2),
                 f64=(31, 11, 2, 19), levels=(201, 121, 6, 128), features=(51, 66, 5, 30), calls=(97, 123, 17, 34),
                 edge=(12, 16, 2, 2), edge_rows64=(12, 16, 2, 2), edge_even=(12, 4, 2, 2), thin=(12, 6, 2, 2), tall=(12, 8, 2, 2), thin_even=(12, 9, 2, 2))
AT_THE_BOUND = [(129, 129), (130, 130), (5, 4097), (4097, 5), (6, 4098)]     # 4096 cells each
SHAPES = [(5, 7), (6, 6), (8, 8), (9, 9), (21, 45), (33, 33), (65, 65)] + AT_THE_BOUND
LOOPS = [0, 1, 1 << 30, (1 << 32) - 1]
KEYS = [0, 1, 0x0123456789ABCDEF, (1 << 64) - 1]


def layouts():
    from raycastworlds_jl_amd import layouts as L

    return L


# ---- the maze rule by hand ------------------------------------------------------------------------------------------------------------------
def test_5_by_5_drops_the_edge_with_the_largest_order_word():
    """4 cells in a square, 4 edges — ids 0 (east of cell 0), 1 (south of 0), 3 (south of 1), 4 (east of 2) —: a spanning tree takes three,
    and the minimum one leaves out the largest word"""
    assert WG.grid(5, 5) == (2, 2, 4)
    assert [(e[0], e[3]) for e in WG.edges(5, 5)] == [(0, (1, 2)), (1, (2, 1)), (3, (2, 3)), (4, (3, 2))]
    dropped = set()
    for m in range(40):
        words = {eid: WG.order_word(m, eid) for eid in (0, 1, 3, 4)}
        assert all(w & 0xFFFFF == eid and w >> 20 == WR.draw(m, eid) >> 20 for eid, w in words.items())
        worst = max(words, key=words.get)
        assert sorted(WG.tree_edges(m, 5, 5)) == sorted(set(words) - {worst})
        w = WG.maze(m, 5, 5)
        passages = {0: (1, 2), 1: (2, 1), 3: (2, 3), 4: (3, 2)}
        for eid, (i, j) in passages.items():
            assert bool(w[i, j]) == (eid == worst)
        assert not w[1, 1] and not w[1, 3] and not w[3, 1] and not w[3, 3] and w[2, 2] and int((~w).sum()) == 7
        dropped.add(worst)
    assert dropped == {0, 1, 3, 4}


def test_5_by_7_shows_exactly_its_15_spanning_trees():
    """a 2 x 3 grid of cells has 15 spanning trees (Kirchhoff); 400 keys show every one and nothing else"""
    seen = set()
    for m in range(400):
        tree = tuple(sorted(WG.tree_edges(WR.draw(77, m), 5, 7)))
        assert len(tree) == 5
        seen.add(tree)
    assert len(seen) == 15


def test_400_keys_give_400_mazes_at_9_by_9_but_for_birthdays():
    """a 4 x 4 grid of cells has 100352 spanning trees: 400 uniform draws would hold 400 * 399 / 2 / 100352 = 0.8 equal pairs on average, and
    random minimum spanning trees are not quite uniform — a few times that.  Ten equal pairs would be a broken order word."""
    assert len({WG.maze(WR.draw(78, m), 9, 9).tobytes() for m in range(400)}) >= 390


@pytest.mark.parametrize("H,W", SHAPES)
def test_a_tree_of_c_minus_1_edges_connected_and_ring_closed(H, W):
    ni, nj, C_ = WG.grid(H, W)
    L = layouts()
    for m in KEYS[:3 if H < 65 else 1]:
        assert len(WG.tree_edges(m, H, W)) == C_ - 1
        w = WG.maze(m, H, W)
        assert int((~w).sum()) == 2 * C_ - 1                                  # the cells and one passage a tree edge
        assert L.is_connected(w)
        assert w[0].all() and w[-1].all() and w[:, 0].all() and w[:, -1].all()
        assert w[2 * ni:].all() and w[:, 2 * nj:].all()                       # an even size: the last interior row or column stays wall
        assert WG.maze(m, H, W).tobytes() == w.tobytes()


@pytest.mark.parametrize("H,W", [(5, 7), (8, 8), (9, 9), (33, 33)])
def test_loops_only_open_walls_of_the_perfect_maze(H, W):
    _, _, C_ = WG.grid(H, W)
    edges = len(WG.edges(H, W))
    for m in KEYS[:3]:
        perfect = WG.maze(m, H, W)
        previous = perfect
        for loops in (1 << 28, 1 << 30, 1 << 31, (1 << 32) - 1):
            w = WG.maze(m, H, W, loops)
            assert not (w & ~previous).any()                                  # a subset of the walls at the smaller word
            assert layouts().is_connected(w)
            previous = w
        assert int((~previous).sum()) >= C_ + edges - 1                       # 2^32 - 1: every edge open but a draw of exactly 2^32 - 1
    if (H, W) == (33, 33):
        opened = int((perfect & ~WG.maze(KEYS[2], H, W, 1 << 30)).sum())
        assert 0.15 < opened / (edges - (C_ - 1)) < 0.35                      # about a quarter of the 225 non-tree edges


# ---- the kernel's algorithm against Kruskal -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(5, 5)] + SHAPES)
def test_the_rounds_of_the_kernel_find_kruskals_tree(H, W):
    """offer, pick, hook, jump until one label is left: the tree Kruskal finds, C - 1 edges, in at most ceil(log2 C) rounds, no chain longer
    than the roots a round can have"""
    _, _, C_ = WG.grid(H, W)
    for k in range(200 if H * W <= 81 else 36):
        m = WR.draw(79, k)
        tree, rounds, chain = WG.boruvka(m, H, W)
        assert tree == sorted(WG.tree_edges(m, H, W)), f"{H} x {W}, key {m:#x}"
        assert len(tree) == C_ - 1 and 1 <= rounds <= (C_ - 1).bit_length() and 1 <= chain < C_


def test_two_roots_that_picked_each_other_keep_the_smaller():
    """5 x 5: four cells, every round-one root picks its smaller edge.  Over 40 keys some pair always picks each other (the smallest edge of
    all is the pick of both its ends), the model ends on one label — a cycle would trip its assertion — and both one round and two occur"""
    rounds = {WG.boruvka(m, 5, 5)[1] for m in range(40)}
    assert rounds == {1, 2}


SEARCHED = {(129, 129): ({6: 99, 7: 51}, (7, 8)), (5, 4097): ({7: 78, 8: 72}, (8, 7)), (4097, 5): ({7: 78, 8: 72}, (8, 8)),
            (33, 33): ({4: 209, 5: 91}, (5, 6))}


@pytest.mark.parametrize("H,W", sorted(SEARCHED))
def test_the_hard_levels_are_the_hardest_of_their_search(H, W):
    """wall_generator_cases.HARD_LEVELS, which the GPU tests install, from the model alone: the level of 0 .. 149 under level seed 9 with the
    most rounds, then the deepest chain, then the smallest number; and the distribution of the docstring"""
    found = [WG.boruvka(WR.episode_key(C.HARD_LEVEL_SEED, level, 0), H, W)[1:] for level in range(300 if H == 33 else 150)]
    counts, hardest = SEARCHED[(H, W)]
    assert {r: [f[0] for f in found].count(r) for r in {f[0] for f in found}} == counts
    level = max(range(150), key=lambda l: (found[l], -l))
    assert level == C.HARD_LEVELS[(H, W)] and found[level] == hardest
    assert hardest[0] >= C.HARD_ROUNDS[(H, W)] == max(counts)                # the most rounds the search shows


# ---- the level rule -----------------------------------------------------------------------------------------------------------------------
def test_levels_stay_in_their_range_and_all_are_reached():
    seen = set()
    for g in range(40):
        for e in range(10):
            m, level = WG.maze_key(5, g, e, 4, 1000, 17)
            assert 1000 <= level < 1004 and m == WR.episode_key(17, level, 0)
            seen.add(level)
    assert seen == {1000, 1001, 1002, 1003}
    top = 2 ** 31 - 1
    assert WG.maze_key(5, 0, 0, 1, top - 1, 3)[1] == top - 1
    m, level = WG.maze_key(5, 3, 2)
    assert level == -1 and m == WR.draw(WR.episode_key(5, 3, 2), 1 << 63)


def test_two_agents_on_one_level_hold_one_maze():
    c = dict(C.CALLS, B=12, H=7, W=9)
    ref = C.make_ref(c, render=False)
    ref.set_wall_generator(0.25, levels=2, first_level=7, level_seed=1)
    by_level = {}
    for b in range(12):
        by_level.setdefault(int(ref.wall_layout[b]), []).append(ref.walls_of(b))
    assert set(by_level) == {7, 8} and all(len(v) > 1 for v in by_level.values())
    for level, walls in by_level.items():
        for w in walls:
            np.testing.assert_array_equal(w, WG.maze(WR.episode_key(1, level, 0), 7, 9, WG.loops_word(0.25)))
    assert not (by_level[7][0] == by_level[8][0]).all()


def test_what_an_install_is_refused_for():
    assert WG.install_refusal(4, 9, 0, 0) == "invalid" and WG.install_refusal(9, 4, 0, 0) == "invalid"
    assert WG.install_refusal(9, 9, -1, 0) == "invalid" and WG.install_refusal(9, 9, 1, -1) == "invalid"
    assert WG.install_refusal(9, 9, 2, 2 ** 31 - 2) == "invalid" and WG.install_refusal(9, 9, 1, 2 ** 31 - 2) is None
    assert WG.install_refusal(129, 129, 0, 0) is None and WG.install_refusal(130, 130, 0, 0) is None      # 64 x 64 cells still
    assert WG.install_refusal(131, 129, 0, 0) == "unsupported"


# ---- the library's host exports -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(5, 5)] + SHAPES)
def test_the_host_export_equals_the_reference_byte_for_byte(H, W):
    L = layouts()
    for m in KEYS[:2] if H >= 65 else KEYS:
        for loops in LOOPS:
            got = L.generated_maze(m, H, W, loops)
            assert got.dtype == bool and got.shape == (H, W)
            np.testing.assert_array_equal(got, WG.maze(m, H, W, loops), err_msg=f"{H} x {W}, key {m:#x}, loops {loops}")
    np.testing.assert_array_equal(L.generated_maze(KEYS[2], H, W, 0.25), WG.maze(KEYS[2], H, W, 1 << 30))


def test_the_key_export_equals_the_reference():
    L = layouts()
    for seed, g, e in ((0, 0, 0), (5, 66, 3), ((1 << 64) - 1, 2 ** 31 - 1, 2 ** 32 - 1)):
        assert L.generated_maze_key(seed, g, e) == WG.maze_key(seed, g, e)
        for levels, first, ls in ((1, 0, 0), (3, 40, 9), (2 ** 31 - 1, 0, 1 << 63), (1, 2 ** 31 - 2, 5)):
            assert L.generated_maze_key(seed, g, e, levels, first, ls) == WG.maze_key(seed, g, e, levels, first, ls)


def test_the_host_exports_refuse_what_the_rule_excludes():
    import ctypes as Ct

    from raycastworlds_jl_amd import _capi

    L, lib = layouts(), _capi.load()
    for H, W in ((4, 9), (9, 4), (0, 0), (-5, 7)):
        with pytest.raises(ValueError, match="at least 5 x 5"):
            L.generated_maze(1, H, W)
    with pytest.raises(ValueError, match="2\\^20"):
        L.generated_maze(1, 1500, 1500)
    assert lib.rcw_wall_generator_layout(9, 9, 1, 0, None) == _capi.RCW_ERR_INVALID_ARGUMENT
    for bad in ((3, 0, 0, -1, 0, 0), (3, 0, 0, 1, -1, 0), (3, 0, 0, 2, 2 ** 31 - 2, 0), (3, -1, 0, 0, 0, 0)):
        with pytest.raises(ValueError, match="first_level"):
            L.generated_maze_key(*bad)
    assert lib.rcw_wall_generator_key(3, 0, 0, 0, 0, 0, None, None) == _capi.RCW_OK          # either pointer may be NULL
    level = Ct.c_int32(5)
    assert lib.rcw_wall_generator_key(3, 0, 0, 0, 0, 0, None, Ct.byref(level)) == _capi.RCW_OK and level.value == -1
    for p, word in ((0.0, 0), (0.25, 1 << 30), (1.0, (1 << 32) - 1), (1e-10, 0), (7, 7)):
        assert L.loops_word(p) == word
    for bad in (-0.1, 1.5, -1, 1 << 32):
        with pytest.raises(ValueError):
            L.loops_word(bad)


# ---- the reference as a whole ---------------------------------------------------------------------------------------------------------------------
def test_two_shards_equal_the_halves_of_one():
    c = dict(C.CALLS, B=12, H=5, W=7)
    whole = C.make_ref(c, render=False)
    halves = [C.make_ref(dict(c, B=6), render=False, agent_id_offset=o) for o in (0, 6)]
    for r in [whole] + halves:
        r.set_wall_generator(0.1)
    rng = np.random.default_rng(8)
    for t in range(30):
        a = WR.draw_actions(rng, 12)
        whole.step(a); halves[0].step(a[:6]); halves[1].step(a[6:])
        w = whole.snapshot()
        for h, sl in zip(halves, (slice(0, 6), slice(6, 12))):
            s = h.snapshot()
            for k in ("wall_layout", "episode", "goal", "position", "direction", "done", "tile_map_chunks"):
                np.testing.assert_array_equal(s[k], w[k][sl], err_msg=f"{k}, step {t}")
    assert whole.events["restarts_after_done"] > 0 and whole.events["episode_starts"] > 12


def test_the_walls_of_an_episode_are_the_maze_of_its_key():
    """after the install and after restarts: every agent's walls are maze(maze_key(seed, g, counter - 1)), the counter moves once a call"""
    c = dict(C.CALLS, B=8, H=5, W=7)
    ref = C.make_ref(c, render=False, agent_id_offset=100)
    ref.set_wall_generator(0.25)
    rng = np.random.default_rng(2)
    for _ in range(40):
        ep0 = ref.episode.copy()
        ref.step(WR.draw_actions(rng, 8))
        assert set((ref.episode - ep0).tolist()) <= {0, 1}
        for b in range(8):
            m, level = WG.maze_key(c["seed"], 100 + b, int(ref.episode[b]) - 1)
            assert level == -1 == ref.wall_layout[b]
            np.testing.assert_array_equal(ref.walls_of(b), WG.maze(m, 5, 7, 1 << 30))
    assert ref.events["restarts_after_done"] > 0
    with pytest.raises(RuntimeError):
        ref.set_walls(np.ones((5, 7), bool))
    before = ref.tile_map_chunks.copy()
    ref.set_wall_generator(None)
    np.testing.assert_array_equal(ref.tile_map_chunks, before)


@pytest.mark.parametrize("name", sorted(C.SCENARIOS))
def test_every_gpu_scenario_reaches_what_it_claims(name):
    snaps, ev = C.recorded(name, False)
    assert tuple(ev[k] for k in COLUMNS) == REHEARSED[name], {k: ev[k] for k in COLUMNS}
    assert all(ev[k] > 0 for k in COLUMNS), ev                               # restarts of both kinds and goal redraws, in every scenario
    if name == "levels":
        assert len(ev["mazes_made"]) == 3
        last = snaps[-1]["wall_layout"]
        assert set(last.tolist()) == {40, 41, 42} and min(np.bincount(last - 40)) > 5
    elif name != "calls":
        assert len(ev["mazes_made"]) == ev["episode_starts"]                 # a maze of its own every episode
    if name == "calls":
        assert [s["generator"] for s in snaps].count(False) > 5 and snaps[-1]["generator"]
    ep = np.stack([s["episode"] for s in snaps]).astype(np.int64)
    assert set(np.diff(ep, axis=0).ravel().tolist()) <= {0, 1}              # the counter moves once a call at most
