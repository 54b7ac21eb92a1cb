"""The rooms' specification (tests/wall_rooms_ref.py) anchored on the CPU: the rule by hand at 5 x 5 and 8 x 8 and on a 9 x 12 layout written
out here from its draws, what holds of every layout at every shape of the suite, the kernel's round-by-round traversal against the
recursion, the library's host export (rcw_wall_rooms_layout: depth first off a stack in C++, no device) against the reference byte for byte
up to the size bound, the draw indices against the other families', sharding — and a rehearsal, without frames, of every scenario the GPU
tests play (tests/wall_rooms_cases.py), asserting from the reference's own counts what each reaches:

    scenario   episode_starts  rooms_made  second_doors  goal_redraws  restarts_after_done  restarts_after_truncation
    tiny       233             466           0           67            43                   123    (5 x 5, room 1: two rooms each)
    square(64)  27              89          10            5             5                    13
    doors       24             256         103           16             4                    12    (a second door drawn for every wall)
    wide        18             292          95            3             2                    10
    levels     135             939         142           53             1                    67    (three levels)
    features    54             258          18           19             6                    32
    calls       83             233          24           25             8                    26

THE KERNEL'S ROUNDS, wall_rooms_ref.rounds: the chambers one cut below each other share a round, so the rounds are the deepest recursion
+ 1 and the widest round is the most chambers at one depth.  Levels 0 .. 149 under level seed 9 with room 1, stop 0, doors 0:

    shape      most rooms  deepest recursion  most chambers at one depth
    8 x 8        7          4                   6
    16 x 16     31         11                  22
    33 x 33    119         18                  54
    66 x 66    492         24                 166     (level 111: 166 chambers in one round; level 48: 25 rounds)

and over levels 0 .. 9 at the bound: 130 x 130 1808 rooms, depth 28, 468 a round; 5 x 4097 2048 rooms, depth 31, 516 a round.  With
levels=1 every agent's key is episode_key(level_seed, first_level, 0): the GPU tests install levels 111 and 48 at 66 x 66.

The exports are missing from the build before this feature: the tests that call them fail there.
"""
import numpy as np
import pytest

import wall_caves_ref as WC
import wall_generator_ref as WG
import wall_rooms_cases as C
import wall_rooms_ref as RR
import walls_ref as WR

ALL = 0xFFFFFFFF
COLUMNS = ("episode_starts", "rooms_made", "second_doors", "goal_redraws", "restarts_after_done", "restarts_after_truncation")
REHEARSED = dict(tiny=(233, 466, 0, 67, 43, 123), square=(27, 89, 10, 5, 5, 13), square64=(27, 89, 10, 5, 5, 13), doors=(24, 256, 103, 16, 4, 12),
                 wide=(18, 292, 95, 3, 2, 10), levels=(135, 939, 142, 53, 1, 67), features=(54, 258, 18, 19, 6, 32), calls=(83, 233, 24, 25, 8, 26))
SHAPES = C.ALL_SHAPES
PARAMETERS = [(room, RR.word(stop), RR.word(doors)) for room, stop, doors in C.PARAMETERS]
KEYS = [0, 1, 0x0123456789ABCDEF, (1 << 64) - 1]
SEARCHED = {(8, 8): (7, 4, 6), (16, 16): (31, 11, 22), (33, 33): (119, 18, 54), (66, 66): (492, 24, 166)}   # most rooms, deepest, widest


def layouts():
    from raycastworlds_jl_amd import layouts as L

    return L


def level_key(level):
    return WR.episode_key(C.HARD_LEVEL_SEED, level, 0)


def picture(w):
    return ["".join("#" if x else "." for x in row) for row in w]


# ---- the rule by hand ---------------------------------------------------------------------------------------------------------------------
FOUR = [["#####", "#...#", "#.###", "#...#", "#####"], ["#####", "#...#", "###.#", "#...#", "#####"],      # the centre row, the door at either end
        ["#####", "#.#.#", "#.#.#", "#...#", "#####"], ["#####", "#...#", "#.#.#", "#.#.#", "#####"]]      # the centre column


def test_5_by_5_with_room_1_and_one_door_has_exactly_four_layouts():
    """the root [1..3] x [1..3]: R = C = {2}, a tie, so bit 63 of draw n picks the side; the wall covers 3 tiles, the door is at 1 or 3"""
    seen = set()
    for level in range(200):
        m = level_key(level)
        w, leaves, cuts, deep = RR.rooms(m, 5, 5, 1, 0, 0, details=True)
        p = picture(w)
        assert p in FOUR and int((~w).sum()) == 7 and len(leaves) == 2 and deep == 1
        n = RR.ROOMS_DRAW + 8 * (((1 + 5 * 1) << 16) | (3 + 5 * 3))
        assert RR.draw_index(5, (1, 3, 1, 3)) == n
        row, door = bool(WR.draw(m, n) >> 63), 1 + 2 * WR.below(WR.draw(m, n + 3), 2)
        assert p == FOUR[(0 if row else 2) + (door == 3 if row else door == 1)]
        seen.add(tuple(p))
    assert len(seen) == 4


def test_5_by_5_with_a_second_door_has_never_more_than_six_layouts():
    seen = {tuple(picture(RR.rooms(level_key(level), 5, 5, 1, 0, ALL))) for level in range(200)}
    assert 4 < len(seen) <= 6                                                  # per side: a door at 1, at 3, or at both
    assert all(sum(row.count(".") for row in p) in (7, 8) for p in seen)


def test_5_by_5_with_room_2_is_the_empty_room():
    ring = np.ones((5, 5), bool); ring[1:-1, 1:-1] = False
    for m in KEYS:
        for stop, doors in ((0, 0), (ALL, ALL)):
            w, leaves, cuts, deep = RR.rooms(m, 5, 5, 2, stop, doors, details=True)
            assert w.tobytes() == ring.tobytes() and leaves == [(1, 3, 1, 3)] and not cuts


def test_8_by_8_with_room_2_admits_line_4_alone_in_each_direction():
    """[1..6]: even lines 1 + 2 <= s <= 6 - 2; the halves [1..3] and [5..6] admit none (3 <= s <= 1; 7 <= s <= 4)"""
    sides = set()
    for level in range(100):
        w, leaves, cuts, deep = RR.rooms(level_key(level), 8, 8, 2, 0, 0, details=True)
        assert all(s == 4 for _, s, _, _ in cuts) and 2 <= len(cuts) <= 3 and len(leaves) == len(cuts) + 1
        assert cuts[0][3] == (1, 6, 1, 6)
        sides.add(cuts[0][0])
        for i in range(1, 7):
            for j in range(1, 7):
                assert not w[i, j] or i == 4 or j == 4
    assert sides == {False, True}


# A 9 x 12 layout from its draws: level 3 of level seed 9, room 1, stop 0, doors 1/2 (the word 2^31).  Per cut chamber, in the order of the
# recursion: the chamber, its admissible row and column lines, the side and why, then the picks — below(draw(m, n + 2), |S|), the first
# door's below(draw(m, n + 3), cnt), whether draw n + 4 (high word below 2^31) grants a second door and that one's below(draw(m, n + 5), cnt).
HAND_KEY = 0xF37559193240E5F1
HAND = [  # chamber          R          C             side      why        pick  cnt  door  second  its pick
    ((1, 7, 1, 10), [2, 4, 6], [2, 4, 6, 8], "column", "shorter", 2, 4, 2, True, 2),      # line 6; doors 5 and 5
    ((1, 7, 1, 5), [2, 4, 6], [2, 4], "row", "longer", 1, 3, 0, True, 0),                 # line 4; doors 1 and 1
    ((1, 3, 1, 5), [2], [2, 4], "column", "shorter", 0, 2, 1, True, 0),                   # line 2; doors 3 and 1: no wall tile but (2, 2)
    ((1, 3, 3, 5), [2], [4], "column", "tie", 0, 2, 0, False, None),                      # line 4; door 1
    ((5, 7, 1, 5), [6], [2, 4], "column", "shorter", 1, 2, 1, True, 0),                   # line 4; doors 7 and 5
    ((5, 7, 1, 3), [6], [2], "column", "tie", 0, 2, 0, True, 1),                          # line 2; doors 5 and 7
    ((1, 7, 7, 10), [2, 4, 6], [8], "row", "longer", 0, 2, 1, False, None),               # line 2; door 9
    ((3, 7, 7, 10), [4, 6], [8], "row", "longer", 1, 2, 0, True, 1),                      # line 6; doors 7 and 9
    ((3, 5, 7, 10), [4], [8], "column", "shorter", 0, 2, 1, True, 1),                     # line 8; doors 5 and 5
    ((3, 5, 9, 10), [4], [], "row", "only", 0, 1, 0, False, None),                        # line 4; door 9
]
HAND_PICTURE = ["############",
                "#.....#....#",
                "#.#.#.###.##",
                "#...#.#.#..#",
                "#.#####.#.##",
                "#..........#",
                "#.#.#.#.#.##",
                "#.....#....#",
                "############"]
HAND_ROOMS = [(1, 3, 1, 1), (1, 3, 3, 3), (1, 3, 5, 5), (5, 7, 1, 1), (5, 7, 3, 3), (5, 7, 5, 5), (1, 1, 7, 10), (3, 5, 7, 7), (3, 3, 9, 10), (5, 5, 9, 10), (7, 7, 7, 10)]


def test_a_9_by_12_layout_written_out_tile_by_tile_from_its_draws():
    H, W, m, doors = 9, 12, HAND_KEY, 1 << 31
    assert level_key(3) == m
    w = np.array([[ch == "#" for ch in "############"]] + [[ch == "#" for ch in "#..........#"]] * 7 + [[ch == "#" for ch in "############"]])
    for (i0, i1, j0, j1), R, Cs, side, why, pick, cnt, door, second, pick2 in HAND:
        assert R == [i for i in range(i0 + 1, i1) if i % 2 == 0] and Cs == [j for j in range(j0 + 1, j1) if j % 2 == 0]
        di, dj = i1 - i0, j1 - j0
        n = (1 << 61) + 8 * (((i0 + H * j0) << 16) | (i1 + H * j1))
        if why == "only":
            assert (side == "row") == (not Cs) and bool(R) != bool(Cs)
        elif why == "tie":
            assert R and Cs and di == dj and (side == "row") == bool(WR.draw(m, n) >> 63)
        else:
            assert R and Cs and (side == "row") == (di > dj) and why == ("longer" if di > dj else "shorter")
        S = R if side == "row" else Cs
        assert WR.below(WR.draw(m, n + 2), len(S)) == pick
        s = S[pick]
        lo, hi = (j0, j1) if side == "row" else (i0, i1)
        assert cnt == (hi - lo) // 2 + 1 and WR.below(WR.draw(m, n + 3), cnt) == door
        assert ((WR.draw(m, n + 4) >> 32) < doors) == second
        gaps = {lo + 2 * door}
        if second:
            assert WR.below(WR.draw(m, n + 5), cnt) == pick2
            gaps.add(lo + 2 * pick2)
        for x in range(lo, hi + 1):
            if x not in gaps:
                tile = (s, x) if side == "row" else (x, s)
                assert not w[tile]
                w[tile] = True
    assert picture(w) == HAND_PICTURE
    got, leaves, cuts, deep = RR.rooms(m, H, W, 1, 0, doors, details=True)
    assert picture(got) == HAND_PICTURE and sorted(leaves) == sorted(HAND_ROOMS) and [c[3] for c in cuts] == [h[0] for h in HAND] and deep == 5
    for i0, i1, j0, j1 in HAND_ROOMS:                                         # the rooms are free rectangles
        assert not w[i0:i1 + 1, j0:j1 + 1].any()
    assert int((~w).sum()) == sum((i1 - i0 + 1) * (j1 - j0 + 1) for i0, i1, j0, j1 in HAND_ROOMS) + 14   # ... and 14 door tiles (4 of the 10 walls have two)
    assert picture(RR.rounds(m, H, W, 1, 0, doors)[0]) == HAND_PICTURE
    assert picture(layouts().generated_rooms(m, H, W, 1, 0, 0.5)) == HAND_PICTURE


def test_stop_everywhere_leaves_exactly_two_rooms():
    for H, W in SHAPES:
        for level in range(10):
            w, leaves, cuts, deep = RR.rooms(level_key(level), H, W, 1, ALL, 0, details=True)
            assert len(leaves) == 2 and len(cuts) == 1 and deep == 1 and cuts[0][3] == (1, H - 2, 1, W - 2)   # the root is never left whole


def test_without_second_doors_every_wall_has_one_door_and_walls_are_rooms_less_one():
    for H, W in SHAPES:
        for level in range(10 if H * W <= 1024 else 3):
            w, leaves, cuts, deep = RR.rooms(level_key(level), H, W, 1, RR.word(0.1), 0, details=True)
            assert len(cuts) == len(leaves) - 1
            for row, s, gaps, (i0, i1, j0, j1) in cuts:
                line = w[s, j0:j1 + 1] if row else w[i0:i1 + 1, s]
                assert len(gaps) == 1 and int((~line).sum()) == 1


# ---- what holds of every layout ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SHAPES)
def test_ring_connectivity_parity_room_sides_and_the_rounds_at_every_shape(H, W):
    """levels 0 .. 149 (0 .. 29 at 32 x 32, 0 .. 9 at 66 x 66) under the four parameter sets: the invariants of the rule, and the kernel's
    round-by-round traversal against the recursion"""
    L = layouts()
    Q = RR.bound(H, W)
    assert Q == ((H - 1) // 2) * ((W - 1) // 2)
    odd = np.zeros((H, W), bool); odd[1:H - 1:2, 1:W - 1:2] = True      # the interior's (odd, odd) tiles
    for level in range(150 if H * W <= 1000 else 30 if H * W <= 1024 else 10):
        m = level_key(level)
        for room, stop, doors in PARAMETERS:
            where = f"{H} x {W}, level {level}, room {room}, stop {stop}, doors {doors}"
            w, leaves, cuts, deep = RR.rooms(m, H, W, room, stop, doors, details=True)
            assert w[0].all() and w[-1].all() and w[:, 0].all() and w[:, -1].all(), where
            assert L.is_connected(w), where
            assert int((~w).sum()) >= 7, where
            assert not (w & odd).any(), where
            assert 1 <= len(leaves) <= Q and len(cuts) == len(leaves) - 1, where
            for i0, i1, j0, j1 in leaves:
                assert i0 % 2 == 1 and j0 % 2 == 1 and not w[i0:i1 + 1, j0:j1 + 1].any(), where
                assert (i1 - i0 + 1 >= room and j1 - j0 + 1 >= room) or (i0, i1, j0, j1) == (1, H - 2, 1, W - 2), where
            for row, s, gaps, c in cuts:
                assert s % 2 == 0 and all(g % 2 == 1 for g in gaps), where
            by_rounds, count, widest, entries = RR.rounds(m, H, W, room, stop, doors)
            assert by_rounds.tobytes() == w.tobytes() and count == deep + 1 and entries == len(leaves) and widest <= entries, where


@pytest.mark.parametrize("H,W", sorted(SEARCHED))
def test_the_search_for_the_widest_round_and_the_deepest_recursion(H, W):
    """levels 0 .. 149, room 1, stop 0, doors 0: the table of this file's header, and at 66 x 66 the two levels the GPU tests install
    (wall_rooms_cases.WIDEST_LEVEL, DEEPEST_LEVEL): a round of more chambers than a wavefront has lanes, and the most rounds"""
    found = [RR.rounds(level_key(level), H, W, 1, 0, 0)[1:] for level in range(150)]     # (rounds, widest, entries)
    assert (max(f[2] for f in found), max(f[0] for f in found) - 1, max(f[1] for f in found)) == SEARCHED[(H, W)]
    if (H, W) == (66, 66):
        widest = max(range(150), key=lambda l: (found[l][1], -l))
        deepest = max(range(150), key=lambda l: (found[l][0], -l))
        assert (widest, found[widest][1]) == C.WIDEST_LEVEL and found[widest][1] > 64
        assert (deepest, found[deepest][0]) == C.DEEPEST_LEVEL
        assert max(f[2] for f in found) <= RR.bound(H, W) == 1024


# ---- the library's host export ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(5, 5)] + SHAPES + [(130, 130), (5, 4097)])
def test_the_host_export_equals_the_reference_byte_for_byte(H, W):
    L = layouts()
    counts = set()
    for m in [level_key(0)] + (KEYS[:1] if H * W >= 1024 else KEYS):
        for room, stop, doors in PARAMETERS + [(1, ALL, ALL)]:
            got, n = L.generated_rooms(m, H, W, room, stop, doors, return_rooms=True)
            want, leaves, _, _ = RR.rooms(m, H, W, room, stop, doors, details=True)
            assert got.dtype == bool and got.shape == (H, W) and n == len(leaves)
            np.testing.assert_array_equal(got, want, err_msg=f"{H} x {W}, key {m:#x}, room {room}, stop {stop}, doors {doors}")
            counts.add(n)
    assert len(counts) > 1 or (H, W) == (5, 5)
    np.testing.assert_array_equal(L.generated_rooms(KEYS[2], H, W), RR.rooms(KEYS[2], H, W))          # the defaults: room 2, 1/4, 1/4
    np.testing.assert_array_equal(L.generated_rooms(KEYS[2], H, W, 1, 0.5, 1.0), RR.rooms(KEYS[2], H, W, 1, 1 << 31, ALL))
    if H * W > 16000:                                                        # the bound: as many rooms as there are (odd, odd) tiles or nearly
        got, n = L.generated_rooms(level_key(1), H, W, 1, 0, 0, return_rooms=True)
        np.testing.assert_array_equal(got, RR.rooms(level_key(1), H, W, 1, 0, 0))
        assert RR.bound(H, W) == 4096 and 1500 < n <= 4096


def test_the_host_export_refuses_what_the_rule_excludes():
    import ctypes as Ct

    from raycastworlds_jl_amd import _capi

    L, lib = layouts(), _capi.load()
    for H, W in ((4, 9), (9, 4), (0, 0), (-5, 7)):
        with pytest.raises(ValueError, match="at least 5 x 5"):
            L.generated_rooms(1, H, W)
    for room in (0, -1):
        with pytest.raises(ValueError, match="at least 1 tile"):
            L.generated_rooms(1, 9, 9, room)
    for H, W in ((131, 131), (130, 131), (5, 4099), (7, 2733)):
        with pytest.raises(ValueError, match="at most 4096"):
            L.generated_rooms(1, H, W)
    L.generated_rooms(1, 130, 130)
    L.generated_rooms(1, 5, 4097)
    L.generated_rooms(1, 6, 4098)
    L.generated_rooms(1, 9, 9, 2 ** 31 - 1)                                   # a room nothing fits twice into: the empty room
    out = np.zeros(81, np.uint8)
    assert lib.rcw_wall_rooms_layout(9, 9, 1, 1, 0, 0, None, None) == _capi.RCW_ERR_INVALID_ARGUMENT
    assert lib.rcw_wall_rooms_layout(9, 9, 1, 9, 0, 0, out.ctypes.data_as(Ct.c_void_p), None) == _capi.RCW_OK   # rooms may be NULL
    assert int((out == 0).sum()) == 49
    assert lib.rcw_wall_rooms_layout(131, 131, 1, 1, 0, 0, out.ctypes.data_as(Ct.c_void_p), None) == _capi.RCW_ERR_UNSUPPORTED
    assert "130 x 130" in _capi.last_error(lib) and "4096" in _capi.last_error(lib)
    assert lib.rcw_wall_rooms_layout(9, 9, 1, 0, 0, 0, out.ctypes.data_as(Ct.c_void_p), None) == _capi.RCW_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        L.generated_rooms(1, 9, 9, 2, 1.5)


def test_what_an_install_is_refused_for():
    assert RR.install_refusal(4, 9, 2, 0, 0) == "invalid" and RR.install_refusal(9, 4, 2, 0, 0) == "invalid"
    assert RR.install_refusal(9, 9, 0, 0, 0) == "invalid" and RR.install_refusal(9, 9, -1, 0, 0) == "invalid"
    assert RR.install_refusal(9, 9, 2, -1, 0) == "invalid" and RR.install_refusal(9, 9, 2, 1, -1) == "invalid"
    assert RR.install_refusal(9, 9, 2, 2, 2 ** 31 - 2) == "invalid" and RR.install_refusal(9, 9, 8, 1, 2 ** 31 - 2) is None
    assert RR.install_refusal(130, 130, 1, 0, 0) is None and RR.install_refusal(5, 4097, 1, 0, 0) is None
    assert RR.install_refusal(131, 131, 1, 0, 0) == "unsupported" and RR.install_refusal(130, 131, 1, 0, 0) == "unsupported"
    assert RR.bound(130, 130) == RR.bound(5, 4097) == RR.bound(6, 4098) == 4096 and RR.bound(131, 131) == 4225 and RR.bound(130, 131) == 4160


def test_the_draw_indices_meet_no_other_familys():
    """a chamber's six indices lie in [2^61, 2^61 + 2^35): above the maze's (below 2^21) and reset_agent's (from 0), below the caves' (from
    2^62) and the layout draw (2^63); distinct chambers have distinct indices, eight apart at least"""
    assert RR.ROOMS_DRAW == 1 << 61 and WC.CAVE_DRAW == 1 << 62 and WG.LAYOUT_DRAW == 1 << 63
    for H, W in ((5, 5), (66, 66), (130, 130), (5, 4097), (16, 4096)):
        assert H * W <= RR.MAX_TILES
        top = RR.draw_index(H, (H - 2, H - 2, W - 2, W - 2)) + 5
        assert RR.ROOMS_DRAW <= RR.draw_index(H, (1, 1, 1, 1)) and top < RR.ROOMS_DRAW + (1 << 35) < WC.CAVE_DRAW
    assert 2 * 2 * WG.MAX_CELLS * 2 < 1 << 21 < RR.ROOMS_DRAW                 # the maze: edge ids and loop draws
    w, leaves, cuts, _ = RR.rooms(level_key(0), 66, 66, 1, 0, 0, details=True)
    used = sorted(RR.draw_index(66, c) for c in leaves + [c[3] for c in cuts])
    assert len(set(used)) == len(used) and min(b - a for a, b in zip(used, used[1:])) >= 8


# ---- the reference as a whole ---------------------------------------------------------------------------------------------------------------------
def test_the_level_rule_is_the_generators():
    """levels >= 1: the key is the episode key of (level_seed, level, 0), the level drawn from the episode's own draw 2^63"""
    c = dict(C.CALLS, B=8)
    ref = C.make_ref(c, render=False, agent_id_offset=100)
    ref.set_wall_rooms(1, 0.1, 0.5, levels=3, first_level=7, level_seed=5)
    rng = np.random.default_rng(2)
    seen = set()
    for _ in range(150):
        ep0 = ref.episode.copy()
        ref.step(WR.draw_actions(rng, 8))
        assert set((ref.episode - ep0).tolist()) <= {0, 1}
        for b in range(8):
            m, level = WG.maze_key(c["seed"], 100 + b, int(ref.episode[b]) - 1, 3, 7, 5)
            u = WR.draw(WR.episode_key(c["seed"], 100 + b, int(ref.episode[b]) - 1), 1 << 63)
            assert level == 7 + WR.below(u, 3) == ref.wall_layout[b] and m == WR.episode_key(5, level, 0)
            np.testing.assert_array_equal(ref.walls_of(b), RR.rooms(m, 8, 8, 1, RR.word(0.1), RR.word(0.5)))
            seen.add(level)
    assert seen == {7, 8, 9} and ref.events["restarts_after_done"] > 0
    with pytest.raises(RuntimeError):
        ref.set_walls(np.ones((8, 8), bool))
    before = ref.tile_map_chunks.copy()
    ref.set_wall_rooms(None)
    np.testing.assert_array_equal(ref.tile_map_chunks, before)
    ref.set_wall_rooms()                                                      # no levels: a layout per (global agent, episode), wall_layout -1
    for b in range(8):
        m, level = WG.maze_key(c["seed"], 100 + b, int(ref.episode[b]) - 1)
        assert level == -1 == ref.wall_layout[b]
        np.testing.assert_array_equal(ref.walls_of(b), RR.rooms(m, 8, 8))


def test_two_shards_equal_the_halves_of_one():
    c = dict(C.CALLS, B=12)
    whole = C.make_ref(c, render=False)
    halves = [C.make_ref(dict(c, B=6), render=False, agent_id_offset=o) for o in (0, 6)]
    for r in [whole] + halves:
        r.set_wall_rooms(room=1)
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
    assert whole.events["rooms_made"] == halves[0].events["rooms_made"] + halves[1].events["rooms_made"] > whole.events["episode_starts"]


@pytest.mark.parametrize("name", sorted(C.SCENARIOS))
def test_every_gpu_scenario_reaches_what_it_claims(name):
    snaps, ev = C.recorded(name, False)
    assert tuple(ev[k] for k in COLUMNS) == REHEARSED[name], {k: ev[k] for k in COLUMNS}
    assert all(ev[k] > 0 for k in COLUMNS if (k, name) != ("second_doors", "tiny")), ev   # restarts of both kinds, goal redraws, several rooms
    assert ev["rooms_made"] > ev["episode_starts"]
    if name == "levels":
        assert len(ev["keys_made"]) == 3
        last = snaps[-1]["wall_layout"]
        assert set(last.tolist()) == {43, 44, 45} and min(np.bincount(last - 43)) > 5
    elif name != "calls":
        assert len(ev["keys_made"]) == ev["episode_starts"]                   # a layout of its own every episode
    if name == "calls":
        assert [s["rooms"] for s in snaps].count(False) > 5 and snaps[-1]["rooms"]
    ep = np.stack([s["episode"] for s in snaps]).astype(np.int64)
    assert set(np.diff(ep, axis=0).ravel().tolist()) <= {0, 1}              # the counter moves once a call at most
