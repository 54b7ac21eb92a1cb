"""The local map's specification (tests/local_map_ref.py) against cases worked out by hand — no GPU.  What the GPU tests compare the engine
with is this function; here it is held to the header's words: the agent at the centre, row 0 the farthest ahead, column 0 on the +cam side
(cam = rotate_minus_90 of the heading, the side of ray 0), r cells a tile, 0 outside the map."""
import numpy as np
import pytest

import local_map_ref as LM


def ring_values(H, W):
    """1 + bits of the reference's empty room: wall ring 2, interior 1"""
    v = np.full((H, W), 1, np.uint8)
    v[[0, -1], :] = 2
    v[:, [0, -1]] = 2
    return v


def numbered(H, W):
    """every tile its own value: 1 + its linear index (i - 1) + H (j - 1), so an image names the tiles it shows (H * W < 255)"""
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return (1 + i + H * j).astype(np.uint8)


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_offset_table(T):
    np.testing.assert_array_equal(LM.offsets(1, 1, T), [0])
    np.testing.assert_array_equal(LM.offsets(3, 1, T), [-1, 0, 1])
    np.testing.assert_array_equal(LM.offsets(4, 2, T), [-0.75, -0.25, 0.25, 0.75])
    off = LM.offsets(5, 3, T)
    assert off.dtype == T and off[0] == T(-4) / T(6) and off[4] == T(4) / T(6) and off[2] == 0      # one division, rounded once in T
    assert T(2) / T(3) != np.float64(2) / np.float64(3) or T is np.float64


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_size_one_is_the_agents_own_tile(T):
    v = numbered(5, 7)
    for i, j in ((1, 1), (3, 4), (5, 7)):
        for d in ((1, 0), (0, 1), (-1, 0), (0.6, -0.8)):
            img = LM.local_map_one(v, (i - 0.5, j - 0.25), d, 1, 1, T)
            assert img.shape == (1, 1) and img[0, 0] == v[i - 1, j - 1]
    assert LM.local_map_one(v, (5.5, 3.5), (1, 0), 1, 1, T)[0, 0] == 0      # off the map
    assert LM.local_map_one(v, (np.nan, 3.5), (1, 0), 1, 1, T)[0, 0] == 0   # NaN
    assert LM.local_map_one(v, (2.5, np.inf), (1, 0), 1, 1, T)[0, 0] == 0
    assert LM.local_map_one(v, (-0.25, 3.5), (1, 0), 1, 1, T)[0, 0] == 0    # floor(-0.25) = -1: outside, not tile 1


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_heading_along_i(T):
    """5 x 7, the agent at the centre of tile (i, j) = (3, 4), heading (1, 0): row 0 is the tile ahead, i + 1.  Column 0 is on the +cam
    side, cam = rotate_minus_90(dir) = (d2, -d1) = (0, -1): the tile at j - 1, by the header's formula wy = (py + a d2) - l d1 with
    l = off[S-1-0] = +1.  (The feature's request names the formula AND, for this case, "column 0 the tile at j + 1"; the two cannot both
    hold, and the formula — stated with the lateral axis and the side of ray 0 = dir + fov cam — is the contract.  Ray 0 fills the camera
    view's LAST image column (SR:431 mirrors), so the local map's columns run against the camera view's; `[:, :, ::-1]` turns them.)"""
    v = numbered(5, 7)
    H = 5
    i, j = 3, 4
    img = LM.local_map_one(v, (i - 0.5, j - 0.5), (1, 0), 3, 1, T)

    def tile(ii, jj):
        return 1 + (ii - 1) + H * (jj - 1)

    # row 0: ahead = off[2] = +1 -> wx = px + 1: tile i + 1.  column 0: lateral = off[2] = +1 -> wy = py - 1 * d1 = py - 1: tile j - 1 —
    # and +cam = (d2, -d1) = (0, -1) points to smaller j: column 0 is on the +cam side, where ray 0 = dir + fov cam looks.
    want = np.array([[tile(i + 1, j - 1), tile(i + 1, j), tile(i + 1, j + 1)],
                     [tile(i, j - 1), tile(i, j), tile(i, j + 1)],
                     [tile(i - 1, j - 1), tile(i - 1, j), tile(i - 1, j + 1)]], np.uint8)
    np.testing.assert_array_equal(img, want)
    # on the ring map itself: from (4, 4) the row ahead is the ring
    ring = LM.local_map_one(ring_values(5, 7), (3.5, 3.5), (1, 0), 3, 1, T)
    np.testing.assert_array_equal(ring, [[2, 2, 2], [1, 1, 1], [1, 1, 1]])


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_heading_along_j(T):
    """heading (0, 1): ahead is j + 1; cam = (d2, -d1) = (1, 0): column 0 shows i + 1"""
    v = numbered(5, 7)
    H = 5
    i, j = 3, 4
    img = LM.local_map_one(v, (i - 0.5, j - 0.5), (0, 1), 3, 1, T)

    def tile(ii, jj):
        return 1 + (ii - 1) + H * (jj - 1)

    want = np.array([[tile(i + 1, j + 1), tile(i, j + 1), tile(i - 1, j + 1)],
                     [tile(i + 1, j), tile(i, j), tile(i - 1, j)],
                     [tile(i + 1, j - 1), tile(i, j - 1), tile(i - 1, j - 1)]], np.uint8)
    np.testing.assert_array_equal(img, want)


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_a_window_larger_than_the_map(T):
    v = ring_values(4, 4)
    img = LM.local_map_one(v, (1.5, 2.5), (1, 0), 9, 1, T)                  # the agent in tile (2, 3); cells 4 tiles to every side
    assert img[4, 4] == 1
    # row q shows i = 2 + (4 - q), column c shows j = 3 - (4 - c): the map is rows 2..5 (i = 4..1), columns 2..5 (j = 1..4)
    inside = np.zeros((9, 9), bool)
    inside[2:6, 2:6] = True
    assert (img[~inside] == 0).all() and (img[inside] != 0).all()
    np.testing.assert_array_equal(img[2:6, 2:6], [[2, 2, 2, 2], [2, 1, 1, 2], [2, 1, 1, 2], [2, 2, 2, 2]])
    far = LM.local_map_one(v, (1.5, 2.5), (1e6, 0), 9, 1, T)                # a non-unit heading vector scales the window
    assert far[4, 4] == 1 and (far[np.arange(9) != 4] == 0).all()


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_two_cells_a_tile_doubles_every_tile(T):
    v = numbered(5, 7)
    for d in ((1, 0), (0, 1), (-1, 0), (0, -1)):
        one = LM.local_map_one(v, (2.5, 3.5), d, 3, 1, T)
        two = LM.local_map_one(v, (2.5, 3.5), d, 6, 2, T)
        np.testing.assert_array_equal(two, np.repeat(np.repeat(one, 2, axis=0), 2, axis=1))


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_a_diagonal_heading_by_hand(T):
    """heading (h, h), h = sqrt(1/2) in T, the agent at (3.5, 3.5) on a 7 x 7 map, S = 3, r = 1: the formula cell by cell, written out"""
    v = numbered(7, 7)
    h = T(np.sqrt(T(0.5)))
    px = py = T(3.5)
    img = LM.local_map_one(v, (px, py), (h, h), 3, 1, T)
    off = [T(-1), T(0), T(1)]
    for q in range(3):
        for c in range(3):
            a, l = off[2 - q], off[2 - c]
            wx = T(T(px + T(a * h)) + T(l * h))
            wy = T(T(py + T(a * h)) - T(l * h))
            assert img[q, c] == 1 + int(np.floor(wx)) + 7 * int(np.floor(wy)), (q, c)
    # and the picture: straight ahead is (+h, +h): tile (5, 5); column 0 (+cam = (h, -h)) of the middle row is (+h, -h): tile (5, 3)
    t = lambda i, j: 1 + (i - 1) + 7 * (j - 1)                              # noqa: E731
    assert img[1, 1] == t(4, 4) and img[0, 1] == t(5, 5) and img[2, 1] == t(3, 3) and img[1, 0] == t(5, 3) and img[1, 2] == t(3, 5)
    # the corners lie 2h = 1.414 along one axis: ahead + cam side = (2h, 0) -> tile (5, 4) — 3.5 + 1.414 = 4.914, still tile 5
    assert img[0, 0] == t(5, 4) and img[0, 2] == t(4, 5) and img[2, 0] == t(4, 3) and img[2, 2] == t(3, 4)


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_batched_form_equals_the_scalar_form(T):
    rng = np.random.default_rng(3)
    B, H, W, nd = 12, 5, 7, 16
    values = rng.integers(1, 5, (B, H, W)).astype(np.uint8)
    pos = (rng.random((B, 2)) * [H + 2, W + 2] - 1).astype(T)              # some off the map
    pos[3] = (np.nan, 2.5)
    pos[4] = (2.5, -np.inf)
    pos[5] = (1e30, 1e30)
    theta = 2 * np.pi * np.arange(nd) / nd + 0.1
    table = np.stack([np.cos(theta), np.sin(theta)], axis=1).astype(T)
    table[7] = (3.0, -0.5)                                                  # neither unit nor on an axis
    table[8] = (T(2e38) if T is np.float32 else T(1e308), T(2e38) if T is np.float32 else T(1e308))   # products overflow: Inf, and Inf - Inf = NaN
    heading = rng.integers(0, nd, B)
    heading[:3] = (7, 8, 8)
    for S, r in ((1, 1), (3, 1), (6, 2), (5, 3), (9, 16)):
        got = LM.local_map(values, pos, heading, table, S, r, T)
        assert got.dtype == np.uint8 and got.shape == (B, S, S)
        for b in range(B):
            np.testing.assert_array_equal(got[b], LM.local_map_one(values[b], pos[b], table[heading[b]], S, r, T), err_msg=f"agent {b}, S {S}, r {r}")
        assert (got[3] == 0).all() and (got[4] == 0).all() and (got[5] == 0).all()
    assert (LM.local_map(values, pos, heading, table, 9, 1, T) != 0).any()


def test_exactly_four_instantiations_ship():
    """(needs the compiler, no GPU) rcw_local_map_kernel<T, SEEN>: two types, two sources"""
    from test_kernel_instantiations import shipped_kernels

    names = sorted(n for n in shipped_kernels() if n.startswith("rcw_local_map_kernel<"))
    assert names == ["rcw_local_map_kernel<double, false>", "rcw_local_map_kernel<double, true>",
                     "rcw_local_map_kernel<float, false>", "rcw_local_map_kernel<float, true>"], names
