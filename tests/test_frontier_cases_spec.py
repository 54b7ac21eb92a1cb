"""The hand-made seen maps of tests/frontier_cases.py, on the CPU:

  * the conditions each family is built for, asserted on the maps and on the reference (tests/frontier_ref.py), never on an engine;
  * the library's host export (rcw_frontier_rule, through layouts.frontier_rule) against the numpy flood on every map of every family;
  * that the maps discriminate: nine deliberately wrong floods, written out below, each differ from the true one on at least one map of
    every family meant to catch it.  This stands in for running broken kernels, several of which would index out of bounds.

CPU only."""
import numpy as np
import pytest

import frontier_cases as FC
import frontier_ref as FR

X = FC.X


def levels(field):
    """(how many levels the flood has, its widest level)"""
    sizes = FR.level_sizes(field)
    return len(sizes), int(sizes.max(initial=0))


# ---- the conditions ---------------------------------------------------------------------------------------------------------------------
def test_bytes_wide_every_byte_at_every_index_mod_16_and_every_map_on_the_wide_path():
    (case,) = FC.bytes_wide()
    assert (case.H, case.W, len(case.maps)) == (16, 16, 256) and all(FC.wide_path(a, 16, 16) for a in range(256))
    pairs, classes = set(), dict(passable=0, source=0, wall=0)
    for m in case.maps:
        field, _ = FR.flood(m)
        for v, t, (i, cols), want in FC.gadget_fields(m):
            pairs.add((v, t % 16))
            assert tuple(int(field[i, j]) for j in cols) == want, (v, t)      # the class of v alone decides its gadget
            classes["passable" if want[0] == 2 else "source" if want[0] == 1 else "wall"] += 1
    assert len(pairs) == 256 * 16
    assert classes == dict(passable=2 * 32, source=32, wall=253 * 32)


def test_bytes_narrow_every_byte_off_the_wide_path_and_five_maps_on_it_with_a_tail():
    (case,) = FC.bytes_narrow()
    H, W, B = case.H, case.W, len(case.maps)
    assert (H, W, B) == (17, 15, 67) and H * W == 255
    wide = [a for a in range(B) if FC.wide_path(a, H, W)]
    assert wide == [0, 16, 32, 48, 64] and all((a * 255) % 16 != 0 for a in range(B) if a not in wide)
    narrow, tail = set(), set()
    for a, m in enumerate(case.maps):
        field, _ = FR.flood(m)
        for v, t, (i, cols), want in FC.gadget_fields(m):
            assert tuple(int(field[i, j]) for j in cols) == want, (a, v, t)
            if a not in wide:
                narrow.add(v)
            else:
                tail |= {i + H * j for j in cols if i + H * j >= 240}         # gadget tiles among the map's last 15 bytes
    assert narrow == set(range(256))
    assert tail                                                               # the wide path's byte loop decides gadgets too


def test_border_and_wrap_the_literal_maps_and_random_maps_on_the_bitmap_edges():
    assert FC.WRAP_SHAPES == [(4, 4), (5, 3), (3, 6), (3, 85), (85, 3)]
    for H, W in FC.WRAP_SHAPES:
        maps, want = FC.wrap_maps(H, W)
        assert len(maps) == 2 * (W - 1) + 3
        for m, (tiles, cells) in zip(maps, want):
            field, got = FR.flood(m)
            exp = np.full((H, W), X, np.uint16)
            for (i, j), v in cells.items():
                exp[i, j] = v
            np.testing.assert_array_equal(field, exp)
            assert got == tiles
    random = [c for c in FC.border_and_wrap() if c.name.startswith("random")]
    assert [c.H * c.W for c in random] == [9, 32, 64, 33, 65, 255, 256] and all(len(c.maps) == 67 for c in random)
    for c in random:
        edge = np.ones((c.H, c.W), bool)
        edge[1:-1, 1:-1] = False
        on_edge = c.maps[:, edge]
        assert set(np.unique(c.maps)) == {0, 1, 2, 3} and {0, 1, 3} <= set(np.unique(on_edge))   # unseen and passable tiles on the border
        assert c.maps.dtype == np.uint8


def test_full_queue_sources_and_passable_tiles_fill_the_queue():
    cases = FC.full_queue()
    assert [(c.H, c.W) for c in cases] == [(17, 15), (16, 16), (3, 85), (85, 3)]
    for c in cases:
        HW, counts = c.H * c.W, []
        for m in c.maps:
            field, tiles = FR.flood(m)
            passable = int(((m == 1) | (m == 3)).sum())
            assert tiles + passable == HW and levels(field) == (2, max(tiles, passable)) and max(tiles, passable) > 64
            counts.append((tiles, passable))
        assert sorted(counts) == ([(128, 128)] * 2 if HW == 256 else [(127, 128), (128, 127)])


def test_deep_floods_are_500_levels_deep_and_the_poses_meet_0_minus_1_and_more_than_255():
    cases = FC.deep_floods()
    assert [(c.H, c.W) for c in cases] == [(33, 33), (251, 3), (3, 251)]
    for c, deep in zip(cases, (577, 503, 503)):
        fields = [FR.flood(m) for m in c.maps]
        assert [t for _, t in fields] == [1, 1]                               # one unseen tile at the corridor's end
        assert levels(fields[0][0]) == (deep, 1) and deep >= 500
        assert levels(fields[1][0])[0] > 255
        d = {}
        for name, (k, (i, j)) in c.poses.items():
            assert 1 <= i <= c.H - 2 and 1 <= j <= c.W - 2, name              # interior: all the archive's validation admits
            d[name] = FR.lookup(fields[k][0], (i + 0.5, j + 0.5))
        assert d["source"] == 0 and d["wall"] == -1 and d["pocket"] == -1 and d["deep"] > 255 and d["deep_short"] > 255, d
        k, (i, j) = c.poses["pocket"]
        assert c.maps[k][i, j] == FC.FREE and fields[k][0][i, j] == X         # passable, and no source reaches it


def test_wide_levels_on_the_non_square_map():
    (case,) = FC.wide_levels()
    assert (case.H, case.W) == (40, 120)
    room, cross = [FR.flood(m) for m in case.maps]
    assert room[1] == 1 and levels(room[0]) == (81, 80)
    assert cross[1] > 64 and levels(cross[0])[1] > 64


# ---- the export against the numpy flood -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", sorted(FC.FAMILIES))
def test_the_export_equals_the_numpy_flood_on_every_map(rcw, family):
    from raycastworlds_jl_amd import layouts

    n = 0
    for case in FC.FAMILIES[family]():
        assert case.maps.dtype == np.uint8 and case.maps.shape[1:] == (case.H, case.W) and case.H * case.W <= 40 * 120
        for m in case.maps:
            field, tiles = layouts.frontier_rule(m)
            ref, ref_tiles = FR.flood(m)
            np.testing.assert_array_equal(field, ref, err_msg=case.name)
            assert tiles == ref_tiles
            n += 1
    assert n > 0


# ---- the maps discriminate --------------------------------------------------------------------------------------------------------------
def wrong_flood(m, kind):
    """The flood with ONE mistake, in the device's linear order (tile (i, j) at t = i + H j); kind 0: none.
      1  neighbours t - 1, t + 1, t - H, t + H wherever 0 <= n < H W: no row test
      2  passable = v & 1                      3  passable = (v & 3) in (1, 3)            4  unseen = (v & 0x7F) == 0
      5  the last H W % 16 tiles read as wall  6  the last H W % 32 tiles read as wall
      7  only the first 64 sources kept        8  a level truncated to its first 64 tiles  9  field values mod 256"""
    H, W = m.shape
    HW = H * W
    v = np.ascontiguousarray(np.asarray(m).T).reshape(-1).astype(np.int64)
    if kind in (5, 6) and HW % (16 if kind == 5 else 32):
        v[HW - HW % (16 if kind == 5 else 32):] = FC.WALL
    passable = (v & 1) == 1 if kind == 2 else ((v & 3) == 1) | ((v & 3) == 3) if kind == 3 else (v == 1) | (v == 3)
    unseen = (v & 0x7F) == 0 if kind == 4 else v == 0

    def around(a):
        out = np.zeros_like(a)
        if kind == 1:
            for s in (1, H):
                out[s:] |= a[:-s]
                out[:-s] |= a[s:]
            return out
        return np.ascontiguousarray(FR._around(a.reshape(W, H).T).T).reshape(-1)

    def first64(a):
        keep = np.zeros_like(a)
        keep[np.flatnonzero(a)[:64]] = True
        return keep

    front = unseen & ~passable & around(passable)
    if kind == 7:
        front = first64(front)
    field = np.full(HW, X, np.uint16)
    field[front] = 0
    reached = front.copy()
    level = 0
    while front.any():
        level += 1
        front = around(front) & passable & ~reached
        if kind == 8:
            front = first64(front)
        field[front] = level % 256 if kind == 9 else level
        reached |= front
    return np.ascontiguousarray(field.reshape(W, H).T)


# which families are meant to catch which mistake
CATCHES = {1: ("border_and_wrap",), 2: ("bytes_wide", "bytes_narrow"), 3: ("bytes_wide", "bytes_narrow"), 4: ("bytes_wide", "bytes_narrow"),
           5: ("bytes_narrow", "border_and_wrap"), 6: ("bytes_narrow", "border_and_wrap"), 7: ("full_queue", "wide_levels"),
           8: ("full_queue", "wide_levels"), 9: ("deep_floods",)}


@pytest.mark.parametrize("family", sorted(FC.FAMILIES))
def test_the_flood_without_a_mistake_is_the_reference(family):
    for case in FC.FAMILIES[family]():
        for m in case.maps[::7]:
            np.testing.assert_array_equal(wrong_flood(m, 0), FR.flood(m)[0])


@pytest.mark.parametrize("kind", sorted(CATCHES))
def test_every_wrong_flood_is_told_from_the_true_one_by_its_families(kind):
    for family in CATCHES[kind]:
        caught = sum(int((wrong_flood(m, kind) != FR.flood(m)[0]).any()) for case in FC.FAMILIES[family]() for m in case.maps)
        print(f"mistake {kind}: {caught} maps of {family} tell it")
        assert caught > 0, (kind, family)
