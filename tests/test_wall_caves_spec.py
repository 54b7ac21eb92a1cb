"""The caves' specification (tests/wall_caves_ref.py) anchored on the CPU: the rule by hand at 5 x 5 and on a 7 x 9 generation written out
here, ties between largest regions, what holds of every layout at every shape of the suite, how often the fallback is taken, the library's
host export (rcw_wall_caves_layout: a queue flood fill in C++, no device) against the reference byte for byte, sharding — and a rehearsal,
without frames, of every scenario the GPU tests play (tests/wall_caves_cases.py), asserting from the reference's own counts what each
reaches.  Every scenario reaches restarts of both kinds and — but `empty`, whose room has no wall to redraw a goal for — goal redraws; the
four that mix the families (`square`, `levels`, `features`, `calls`) reach caves and fallbacks, the others are all caves or — `full` — all
fallbacks by construction:

    scenario   episode_starts  fallbacks  goal_redraws  restarts_after_done  restarts_after_truncation
    square     227              68        369           31                   129
    tie(64)     15               0         30            3                     7    (one level: the cave with the tie)
    mid         24               0         17            4                    12
    wide        18               0          8            2                    10
    empty        9               0          0            2                     4    (5 x 5, fill 0)
    full         9               9          2            2                     4    (5 x 5, all wall: always the maze)
    levels     134              91        124            1                    66    (three levels, two of them mazes)
    features    56              19         75            8                    32
    calls       83              26        131           10                    26

THE KERNEL'S LABELLING, wall_caves_ref.labelling: hook and jump as the kernel's header describes them, synchronously, against the stack
flood fill — the same kept region at every shape.  Its round count lets the GPU tests choose their caves: with levels=1 every agent's key
is episode_key(level_seed, first_level, 0).  Levels 0 .. 149 under level seed 9 at the defaults (rounds: levels):

    shape      rounds: levels               the level with the most (the smallest such)
    5 x 7      0: 99, 1: 45, 2: 6           9
    8 x 8      0: 8, 1: 44, 2: 98           0
    9 x 12     1: 27, 2: 122, 3: 1          58
    16 x 16    1: 2, 2: 101, 3: 47          0
    21 x 45    2: 34, 3: 115, 4: 1          140
    32 x 32    2: 8, 3: 131, 4: 11          0
    66 x 66    3: 78, 4: 72                 0

Pointer jumping shortens every chain a hook makes before the next hook, so the counts stay this small; the kernel's loop has no cap and
needs none.  Nothing here claims a worst case.

The exports are missing from the build before this feature: the tests that call them fail there.
"""
import numpy as np
import pytest

import wall_caves_cases as C
import wall_caves_ref as WC
import wall_generator_ref as WG
import walls_ref as WR

COLUMNS = ("episode_starts", "fallbacks", "goal_redraws", "restarts_after_done", "restarts_after_truncation")
REHEARSED = dict(calls=(83, 26, 131, 10, 26), empty=(9, 0, 0, 2, 4), features=(56, 19, 75, 8, 32), full=(9, 9, 2, 2, 4), levels=(134, 91, 124, 1, 66),
                 mid=(24, 0, 17, 4, 12), square=(227, 68, 369, 31, 129), tie=(15, 0, 30, 3, 7), tie64=(15, 0, 30, 3, 7), wide=(18, 0, 8, 2, 10))
SHAPES = C.ALL_SHAPES
DEFAULT = WC.fill_word(WC.DEFAULT_FILL)
FILLS = [0, DEFAULT, WC.fill_word(0.5), (1 << 32) - 1]
SMOOTHS = [0, 2, 8]
KEYS = [0, 1, 0x0123456789ABCDEF, (1 << 64) - 1]
SEARCHED = {(5, 7): {0: 99, 1: 45, 2: 6}, (8, 8): {0: 8, 1: 44, 2: 98}, (9, 12): {1: 27, 2: 122, 3: 1}, (16, 16): {1: 2, 2: 101, 3: 47},
            (21, 45): {2: 34, 3: 115, 4: 1}, (32, 32): {2: 8, 3: 131, 4: 11}, (66, 66): {3: 78, 4: 72}}


def layouts():
    from raycastworlds_jl_amd import layouts as L

    return L


def level_key(level):
    return WR.episode_key(C.HARD_LEVEL_SEED, level, 0)


# ---- the rule by hand ---------------------------------------------------------------------------------------------------------------------
def test_5_by_5_without_fill_is_the_empty_room():
    ring = np.ones((5, 5), bool); ring[1:-1, 1:-1] = False
    for m in KEYS:
        w, fell = WC.cave(m, 5, 5, 0, 0, return_fell_back=True)
        assert not fell and int((~w).sum()) == 9 and w.tobytes() == ring.tobytes()
        # a smoothing step walls up the four interior corners (five of their nine are ring): a plus of 5 tiles, below need = 7 — the maze
        once = WC.smoothed(m, 5, 5, 0, 1)
        assert int((~once).sum()) == 5 and once[1, 1] and once[1, 3] and once[3, 1] and once[3, 3] and not once[2, 2]
        w, fell = WC.cave(m, 5, 5, 0, 1, return_fell_back=True)
        assert fell and w.tobytes() == WG.maze(m, 5, 5, 0).tobytes()


def test_5_by_5_all_wall_is_the_maze_of_the_key():
    for m in KEYS:
        for smooth in SMOOTHS:
            w, fell = WC.cave(m, 5, 5, (1 << 32) - 1, smooth, return_fell_back=True)
            assert fell and w.tobytes() == WG.maze(m, 5, 5, 0).tobytes() and int((~w).sum()) == 7


def test_generation_0_draws_tile_t_at_index_2_to_the_62_plus_t():
    m, H, W = KEYS[2], 7, 9
    g = WC.generation0(m, H, W, DEFAULT)
    assert g[0].all() and g[-1].all() and g[:, 0].all() and g[:, -1].all()
    for i in range(1, H - 1):
        for j in range(1, W - 1):
            assert bool(g[i, j]) == ((WR.draw(m, (1 << 62) + i + H * j) >> 32) < DEFAULT)
    assert 0 < int(g[1:-1, 1:-1].sum()) < 35


# a 7 x 9 generation 0, '#' = WALL, and by hand the number of walls in the 3 x 3 around every interior tile (the ring counts)
GEN0 = ["#########",
        "#.#...#.#",
        "#..#....#",
        "##...##.#",
        "#.#..#..#",
        "#...#..##",
        "#########"]
COUNT = [[6, 5, 5, 4, 4, 4, 6],
         [5, 3, 2, 2, 3, 3, 5],
         [5, 3, 2, 3, 3, 3, 4],
         [5, 2, 2, 3, 4, 4, 5],
         [6, 4, 5, 5, 5, 5, 6]]
GEN1 = ["#########",
        "####...##",
        "##.....##",
        "##......#",
        "##.....##",
        "##.######",
        "#########"]


def test_one_smoothing_step_of_a_generation_written_out_here():
    g0 = np.array([[ch == "#" for ch in row] for row in GEN0])
    assert g0.shape == (7, 9)
    for i in range(1, 6):
        for j in range(1, 8):
            assert int(g0[i - 1:i + 2, j - 1:j + 2].sum()) == COUNT[i - 1][j - 1], (i, j)     # the hand count against the picture
    g1 = WC.smooth_once(g0)
    for i in range(7):
        for j in range(9):
            ring = i in (0, 6) or j in (0, 8)
            assert bool(g1[i, j]) == (ring or COUNT[i - 1][j - 1] >= 5), (i, j)
            assert bool(g1[i, j]) == (GEN1[i][j] == "#"), (i, j)
    # synchronous: the step read generation 0 alone, so doing it in place, tile by tile, gives another picture
    inplace = g0.copy()
    for j in range(1, 8):
        for i in range(1, 6):
            inplace[i, j] = inplace[i - 1:i + 2, j - 1:j + 2].sum() >= 5
    assert inplace.tobytes() != g1.tobytes()
    # generation 0 is one region of 25 tiles from (1, 1), generation 1 one of 20 from (2, 2)
    assert [(len(r), r[0]) for r in WC.regions(g0)] == [(25, 1 + 7 * 1)]
    assert [(len(r), r[0]) for r in WC.regions(g1)] == [(20, 2 + 7 * 2)] and len(WC.kept_region(g1)) == 20


# ---- ties -----------------------------------------------------------------------------------------------------------------------------------
def two_largest(g):
    rs = sorted(WC.regions(g), key=lambda r: (-len(r), r[0]))
    return rs[:2]


def test_of_two_largest_regions_the_one_with_the_smaller_tile_index_survives():
    """levels 0 .. 1499 under level seed 9 at 7 x 9, fill 0.35, no smoothing: those whose two largest regions tie at or above `need`"""
    H, W, fill = 7, 9, WC.fill_word(C.TIE_FILL)
    ties = []
    for level in range(1500):
        g = WC.smoothed(level_key(level), H, W, fill, C.TIE_SMOOTH)
        top = two_largest(g)
        if len(top) == 2 and len(top[0]) == len(top[1]) >= WC.need(H, W):
            ties.append(level)
            first, second = top
            assert first[0] < second[0]
            w, fell = WC.cave(level_key(level), H, W, fill, C.TIE_SMOOTH, return_fell_back=True)
            assert not fell
            free = sorted(int(i + H * j) for i, j in np.argwhere(~w))
            assert free == first and not set(second) & set(free)
            assert WC.kept_by_labels(g) == first                               # the kernel's word (size << 16) | (0xFFFF - root) agrees
    assert len(ties) == 14 and ties[:3] == [97, 114, 519] and C.TIE_LEVEL == ties[0]


# ---- what holds of every layout ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SHAPES)
def test_ring_connectivity_need_and_the_labelling_at_every_shape(H, W):
    """levels 0 .. 149 at the defaults: the invariants of rule 5, the labelling restatement against the flood fill, and the search for the
    level with the most labelling rounds (wall_caves_cases.HARD_LEVELS, which the GPU tests install)"""
    L = layouts()
    rounds = []
    for level in range(150):
        m = level_key(level)
        g = WC.smoothed(m, H, W, DEFAULT, WC.DEFAULT_SMOOTH)
        labels, r = WC.labelling(g)
        rounds.append(r)
        kept = WC.kept_region(g)
        assert WC.kept_by_labels(g) == kept, f"level {level}"
        h = H - 2
        for q in np.flatnonzero(labels >= 0)[:: max(1, h)]:                    # a label is the smallest q of its region
            assert labels[q] <= q and labels[labels[q]] == labels[q]
        if level % (1 if H * W <= 256 else 10) == 0:
            w, fell = WC.cave(m, H, W, DEFAULT, WC.DEFAULT_SMOOTH, return_fell_back=True)
            assert w[0].all() and w[-1].all() and w[:, 0].all() and w[:, -1].all()
            assert L.is_connected(w)
            assert fell == (len(kept) < WC.need(H, W))
            if fell:
                assert w.tobytes() == WG.maze(m, H, W, 0).tobytes()
            else:
                assert int((~w).sum()) == len(kept) >= WC.need(H, W) >= 7
    assert {r: rounds.count(r) for r in set(rounds)} == SEARCHED[(H, W)]
    level = max(range(150), key=lambda l: (rounds[l], -l))
    assert (level, rounds[level]) == C.HARD_LEVELS[(H, W)]


def test_labels_on_a_spiral_end_on_its_outer_end():
    """a one-tile corridor wound into a 21 x 21 map, 200 tiles long: one region whose smallest tile is its outer end.  Every tile that is
    smaller than both its neighbours on the corridor is a root after the first hook; the jumps flatten the trees and the second hook joins
    them: two rounds, where a propagation without pointer jumping would take 200"""
    H = W = 21
    g = np.ones((H, W), bool)
    i, j, di, dj = 1, 1, 0, 1
    g[i, j] = False
    for _ in range(400):
        ni, nj = i + di, j + dj
        ahead2 = (ni + di, nj + dj)
        if not (1 <= ni < H - 1 and 1 <= nj < W - 1) or not g[ni, nj] or (1 <= ahead2[0] < H - 1 and 1 <= ahead2[1] < W - 1 and not g[ahead2]):
            di, dj = dj, -di
            ni, nj = i + di, j + dj
            ahead2 = (ni + di, nj + dj)
            if not (1 <= ni < H - 1 and 1 <= nj < W - 1) or not g[ni, nj] or (1 <= ahead2[0] < H - 1 and 1 <= ahead2[1] < W - 1 and not g[ahead2]):
                break
        i, j = ni, nj
        g[i, j] = False
    assert len(WC.regions(g)) == 1 and int((~g).sum()) > 100
    labels, rounds = WC.labelling(g)
    assert set(labels[labels >= 0].tolist()) == {0} and 1 <= rounds <= 8
    assert WC.kept_by_labels(g) == WC.kept_region(g)


# ---- both paths taken -------------------------------------------------------------------------------------------------------------------------
def fallbacks(H, W, levels=200):
    return sum(WC.cave(level_key(l), H, W, DEFAULT, WC.DEFAULT_SMOOTH, return_fell_back=True)[1] for l in range(levels))


def test_how_often_the_defaults_fall_back():
    """levels 0 .. 199 of level seed 9 at the defaults: 1 at 16 x 16, none at 32 x 32, 192 at 5 x 7 (23 at 9 x 12, 57 at 8 x 8)"""
    found = {shape: fallbacks(*shape) for shape in ((16, 16), (32, 32), (5, 7), (9, 12), (8, 8))}
    assert found[(16, 16)] <= 20                                               # at most 10 %
    assert found[(32, 32)] == 0
    assert found[(5, 7)] >= 160                                                # at least 80 %
    assert found == {(16, 16): 1, (32, 32): 0, (5, 7): 192, (9, 12): 23, (8, 8): 57}


# ---- the library's host export ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(5, 5)] + SHAPES)
def test_the_host_export_equals_the_reference_byte_for_byte(H, W):
    L = layouts()
    both = set()
    for m in [level_key(C.HARD_LEVELS.get((H, W), (0, 0))[0])] + (KEYS[:1] if H >= 32 else KEYS):
        for fill in FILLS:
            for smooth in SMOOTHS:
                got, fell = L.generated_cave(m, H, W, fill, smooth, return_fell_back=True)
                want, wfell = WC.cave(m, H, W, fill, smooth, return_fell_back=True)
                assert got.dtype == bool and got.shape == (H, W) and fell == wfell
                np.testing.assert_array_equal(got, want, err_msg=f"{H} x {W}, key {m:#x}, fill {fill}, smooth {smooth}")
                both.add(fell)
    assert both == {False, True}                                              # fill 0 without smoothing never falls back, fill 2^32 - 1 always does
    np.testing.assert_array_equal(L.generated_cave(KEYS[2], H, W), WC.cave(KEYS[2], H, W, DEFAULT, 2))
    np.testing.assert_array_equal(L.generated_cave(KEYS[2], H, W, 0.5, 1), WC.cave(KEYS[2], H, W, 1 << 31, 1))


def test_the_host_export_at_the_tie_levels():
    L = layouts()
    for level in (97, 114, 519):
        got = L.generated_cave(level_key(level), 7, 9, C.TIE_FILL, C.TIE_SMOOTH)
        np.testing.assert_array_equal(got, WC.cave(level_key(level), 7, 9, WC.fill_word(C.TIE_FILL), C.TIE_SMOOTH))


def test_the_host_export_refuses_what_the_rule_excludes():
    import ctypes as Ct

    from raycastworlds_jl_amd import _capi

    L, lib = layouts(), _capi.load()
    for H, W in ((4, 9), (9, 4), (0, 0), (-5, 7)):
        with pytest.raises(ValueError, match="at least 5 x 5"):
            L.generated_cave(1, H, W)
    for smooth in (9, -1):
        with pytest.raises(ValueError, match="0 .. 8"):
            L.generated_cave(1, 9, 9, 0.4, smooth)
    with pytest.raises(ValueError, match="4096 interior tiles"):
        L.generated_cave(1, 67, 66)
    L.generated_cave(1, 66, 66)
    L.generated_cave(1, 5, 1367)                                              # 3 x 1365 = 4095 interior tiles
    out = np.zeros(81, np.uint8)
    assert lib.rcw_wall_caves_layout(9, 9, 1, 0, 0, None, None) == _capi.RCW_ERR_INVALID_ARGUMENT
    assert lib.rcw_wall_caves_layout(9, 9, 1, 0, 0, out.ctypes.data_as(Ct.c_void_p), None) == _capi.RCW_OK   # fell_back may be NULL
    assert int((out == 0).sum()) == 49
    assert lib.rcw_wall_caves_layout(67, 66, 1, 0, 0, out.ctypes.data_as(Ct.c_void_p), None) == _capi.RCW_ERR_UNSUPPORTED
    assert lib.rcw_wall_caves_layout(9, 9, 1, 0, 9, out.ctypes.data_as(Ct.c_void_p), None) == _capi.RCW_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        L.generated_cave(1, 9, 9, 1.5)


def test_what_an_install_is_refused_for():
    assert WC.install_refusal(4, 9, 2, 0, 0) == "invalid" and WC.install_refusal(9, 4, 2, 0, 0) == "invalid"
    assert WC.install_refusal(9, 9, 9, 0, 0) == "invalid" and WC.install_refusal(9, 9, -1, 0, 0) == "invalid"
    assert WC.install_refusal(9, 9, 2, -1, 0) == "invalid" and WC.install_refusal(9, 9, 2, 1, -1) == "invalid"
    assert WC.install_refusal(9, 9, 2, 2, 2 ** 31 - 2) == "invalid" and WC.install_refusal(9, 9, 8, 1, 2 ** 31 - 2) is None
    assert WC.install_refusal(66, 66, 0, 0, 0) is None and WC.install_refusal(67, 66, 0, 0, 0) == "unsupported"


# ---- the reference as a whole ---------------------------------------------------------------------------------------------------------------------
def test_two_shards_equal_the_halves_of_one():
    c = dict(C.CALLS, B=12)
    whole = C.make_ref(c, render=False)
    halves = [C.make_ref(dict(c, B=6), render=False, agent_id_offset=o) for o in (0, 6)]
    for r in [whole] + halves:
        r.set_wall_caves()
    rng = np.random.default_rng(8)
    for t in range(150):
        a = WR.draw_actions(rng, 12)
        whole.step(a); halves[0].step(a[:6]); halves[1].step(a[6:])
        w = whole.snapshot()
        for h, sl in zip(halves, (slice(0, 6), slice(6, 12))):
            s = h.snapshot()
            for k in ("wall_layout", "episode", "goal", "position", "direction", "done", "tile_map_chunks"):
                np.testing.assert_array_equal(s[k], w[k][sl], err_msg=f"{k}, step {t}")
    assert whole.events["restarts_after_done"] > 0 and whole.events["episode_starts"] > 12
    assert 0 < whole.events["fallbacks"] < whole.events["episode_starts"]
    assert whole.events["fallbacks"] == halves[0].events["fallbacks"] + halves[1].events["fallbacks"]


def test_the_walls_of_an_episode_are_the_cave_of_its_key():
    c = dict(C.CALLS, B=8)
    ref = C.make_ref(c, render=False, agent_id_offset=100)
    ref.set_wall_caves(0.4, 2)
    rng = np.random.default_rng(2)
    for _ in range(40):
        ep0 = ref.episode.copy()
        ref.step(WR.draw_actions(rng, 8))
        assert set((ref.episode - ep0).tolist()) <= {0, 1}
        for b in range(8):
            m, level = WG.maze_key(c["seed"], 100 + b, int(ref.episode[b]) - 1)
            assert level == -1 == ref.wall_layout[b]
            np.testing.assert_array_equal(ref.walls_of(b), WC.cave(m, 8, 8, DEFAULT, 2))
    assert ref.events["restarts_after_done"] > 0
    with pytest.raises(RuntimeError):
        ref.set_walls(np.ones((8, 8), bool))
    before = ref.tile_map_chunks.copy()
    ref.set_wall_caves(None)
    np.testing.assert_array_equal(ref.tile_map_chunks, before)


@pytest.mark.parametrize("name", sorted(C.SCENARIOS))
def test_every_gpu_scenario_reaches_what_it_claims(name):
    snaps, ev = C.recorded(name, False)
    assert tuple(ev[k] for k in COLUMNS) == REHEARSED[name], {k: ev[k] for k in COLUMNS}
    assert all(ev[k] > 0 for k in COLUMNS if k != "fallbacks" and (k, name) != ("goal_redraws", "empty")), ev   # restarts of both kinds and goal redraws
    if name in C.MIXED:
        assert 0 < ev["fallbacks"] < ev["episode_starts"]                      # at least one fallback and at least one cave
    elif name == "full":
        assert ev["fallbacks"] == ev["episode_starts"]
    else:
        assert ev["fallbacks"] == 0
    if name == "levels":
        assert len(ev["keys_made"]) == 3
        last = snaps[-1]["wall_layout"]
        assert set(last.tolist()) == {43, 44, 45} and min(np.bincount(last - 43)) > 5
    elif name in ("tie", "tie64"):
        assert len(ev["keys_made"]) == 1 and (snaps[-1]["wall_layout"] == C.TIE_LEVEL).all()
    elif name != "calls":
        assert len(ev["keys_made"]) == ev["episode_starts"]                   # a layout of its own every episode
    if name == "calls":
        assert [s["caves"] for s in snaps].count(False) > 5 and snaps[-1]["caves"]
    ep = np.stack([s["episode"] for s in snaps]).astype(np.int64)
    assert set(np.diff(ep, axis=0).ravel().tolist()) <= {0, 1}              # the counter moves once a call at most
