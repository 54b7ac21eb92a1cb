"""The seen map's contract (include/rcw.h, rcw_set_seen_map) without a GPU: tests/seen_map_ref.py — what the GPU tests hold the engine to —
against oracle/pyref.py's cast_ray and against cases derived by hand, the call table on a rollout of the Python reference of the dynamics,
and the declarations.  The rollout is also the rehearsal of tests/test_gpu_seen_map.py: the events those tests assert happen here first."""
import numpy as np
import pytest

import seen_map_ref as SM
import walls_ref as WR
from oracle import pyref


ring, crossed = SM.ring, SM.crossed


def one_based(obstacles):
    """pyref's obstacle_map[i][j], 1-based lists"""
    H, W = obstacles.shape
    return [[False] * (W + 1)] + [[False] + [bool(obstacles[i, j]) for j in range(W)] for i in range(H)]


def python_table(nd, N, T, fov=2 / 3):
    """(nd, 5, N) as rcw_ray_table lays it out, from pyref.World.ray_fan: [dx | dy | |1/dx| | |1/dy| | 0]"""
    w = pyref.World(H=4, W=4, nd=nd, num_rays=N, fov=fov, T=T)
    out = np.zeros((nd, 5, N), T)
    with np.errstate(divide="ignore"):
        for d in range(nd):
            w.dir = d
            for k, (dx, dy) in enumerate(w.ray_fan()):
                out[d, :4, k] = (dx, dy, abs(T(1) / T(dx)), abs(T(1) / T(dy)))
    return out


def straight_table(T):
    """one ray, for heading 0 only: straight ahead, (dx, dy) = (1, 0), |1/dx| = 1, |1/dy| = Inf (the fan's only ray would be its first edge)"""
    out = np.zeros((8, 5, 1), T)
    out[0, :, 0] = (1, 0, 1, np.inf, 1)
    return out


RAY_CASES = [(np.float32, False), (np.float32, True), (np.float64, False), (np.float64, True)]


@pytest.mark.parametrize("T,tie_le", RAY_CASES)
def test_the_last_visited_tile_is_cast_rays_stop_tile(T, tie_le):
    """every heading of 16, 33 rays each, from three positions of a crossed 9 x 9 map and a 5 x 13 room"""
    table = python_table(16, 33, T)
    for obstacles, starts in ((crossed(), [(1.5, 1.5), (6.25, 2.75), (3.999, 7.001)]), (ring(5, 13), [(2.5, 6.5), (1.125, 11.875)])):
        obstacles = obstacles.copy()
        obstacles[2, 2] |= True                                             # (a goal tile is an obstacle like a wall)
        om = one_based(obstacles)
        for x, y in starts:
            for d in range(16):
                for k in range(33):
                    dx, dy, ddx, ddy = table[d, :4, k]
                    tiles = SM.visited_tiles(obstacles, x, y, dx, dy, ddx, ddy, tie_le, T)
                    i, j, _, _ = pyref.cast_ray(om, x, y, dx, dy, tie_le=tie_le, T=T)
                    assert tiles[-1] == (i, j), (x, y, d, k)
                    assert tiles[0] == (pyref.wu_to_tu(x), pyref.wu_to_tu(y))
                    assert all(abs(a[0] - b[0]) + abs(a[1] - b[1]) == 1 for a, b in zip(tiles, tiles[1:]))     # a step moves one tile along one axis
                    assert not any(obstacles[i - 1, j - 1] for i, j in tiles[:-1]) and obstacles[tiles[-1][0] - 1, tiles[-1][1] - 1]


@pytest.mark.parametrize("T,tie_le", RAY_CASES)
def test_a_ray_through_a_tile_corner(T, tie_le):
    """From the centre of tile (2, 2) along the diagonal (dx = dy, so |1/dx| = |1/dy| and both side distances are equal at every corner): with
    dda_tie_break = x first on <= the march steps in x at each tie, otherwise in y.  A pillar on (3, 2) stops the first at once and lets the second
    run its staircase to the ring at (5, 6); one on (2, 3) the other way round, to (6, 5); pyref's cast_ray says the same."""
    s = T(np.sqrt(0.5))
    dd = abs(T(1) / s)
    for pillar, stops_le, stops_lt in (((3, 2), (3, 2), (5, 6)), ((2, 3), (6, 5), (2, 3))):
        obstacles = ring(6, 6)
        obstacles[pillar[0] - 1, pillar[1] - 1] = True
        tiles = SM.visited_tiles(obstacles, 1.5, 1.5, s, s, dd, dd, tie_le, T)
        want = stops_le if tie_le else stops_lt
        assert tiles[-1] == want, tiles
        assert tiles[1] == ((3, 2) if tie_le else (2, 3))
        assert pyref.cast_ray(one_based(obstacles), 1.5, 1.5, s, s, tie_le=tie_le, T=T)[:2] == want
    open_room = SM.visited_tiles(ring(6, 6), 1.5, 1.5, s, s, dd, dd, tie_le, T)
    stair = [(2, 2), (3, 2), (3, 3), (4, 3), (4, 4), (5, 4), (5, 5), (6, 5)] if tie_le else [(2, 2), (2, 3), (3, 3), (3, 4), (4, 4), (4, 5), (5, 5), (5, 6)]
    assert open_room == stair


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_one_ray_straight_ahead_marks_the_row_to_the_wall(T):
    """heading 0 is (1, 0): i grows.  From the centre of (2, 4) in a 7 x 9 room the one ray of a one-ray table marks (2, 4) .. (7, 4)."""
    table = straight_table(T)
    bits = ring(7, 9).astype(np.uint8)[None]
    marked = SM.marked_tiles(bits, np.array([[1.5, 3.5]], T), np.array([0]), table, False, T)[0]
    want = np.zeros((7, 9), bool)
    want[1:7, 3] = True
    np.testing.assert_array_equal(marked, want)
    ref = SM.SeenMapRef(table, False, bits, np.array([[5, 4]]), np.array([[1.5, 3.5]], T), np.array([0]), np.array([1], np.uint32))
    assert ref.seen_count[0] == 6 and ref.newly_seen[0] == 0 and ref.goal_seen[0] == 1
    assert ref.map[0, 1:6, 3].tolist() == [1] * 5 and ref.map[0, 6, 3] == 2                     # free tiles, then the ring
    assert SM.linear(ref.map[0])[1 + 7 * 3] == 1 and SM.linear(ref.map[0])[6 + 7 * 3] == 2       # tile (i, j) at (i - 1) + H (j - 1)


def test_edge_cases_of_the_marking_rule():
    T = np.float32
    table = python_table(8, 9, T)
    bits = ring(6, 6).astype(np.uint8)
    bits[3, 3] = 2                                                          # the goal
    stack = np.stack([bits] * 4)
    pos = np.array([[np.nan, 2.5], [-0.5, 2.5], [0.5, 2.5], [3.5, 3.5]], T)   # NaN, off the map, on a ring tile, on the goal tile
    marked = SM.marked_tiles(stack, pos, np.zeros(4, int), table, False, T)
    assert not marked[0].any() and not marked[1].any()
    assert marked[2].sum() == 1 and marked[2][0, 2] and marked[3].sum() == 1 and marked[3][3, 3]
    assert SM.visited_tiles(bits != 0, np.nan, 2.5, 1, 0, 1, np.inf, False, T) == []
    assert SM.visited_tiles(bits != 0, 0.5, 2.5, 1, 0, 1, np.inf, False, T) == [(1, 3)]


@pytest.mark.parametrize("T,tie_le", RAY_CASES)
def test_the_batched_march_marks_what_the_scalar_march_visits(T, tie_le):
    rng = np.random.default_rng(3)
    table = python_table(16, 17, T)
    walls = crossed()
    n = 24
    bits = np.stack([walls.astype(np.uint8)] * n)
    free = np.argwhere(~walls)
    tiles = free[rng.integers(0, len(free), n)]
    pos = (tiles + rng.choice([0.125, 0.5, 0.875, 0.0], (n, 2))).astype(T)  # (0.0: on a tile edge — ties)
    heading = rng.integers(0, 16, n)
    marked = SM.marked_tiles(bits, pos, heading, table, tie_le, T)
    for b in range(n):
        want = np.zeros_like(walls)
        for k in range(17):
            dx, dy, ddx, ddy = table[heading[b], :4, k]
            for i, j in SM.visited_tiles(walls, pos[b, 0], pos[b, 1], dx, dy, ddx, ddy, tie_le, T):
                want[i - 1, j - 1] = True
        np.testing.assert_array_equal(marked[b], want, err_msg=f"agent {b}")


# ---- the call table on a rollout of the Python reference of the dynamics -------------------------------------------------------------
def ref_bits(ref):
    return np.stack([ref.walls_of(b).astype(np.uint8) | (ref.goals_of(b).astype(np.uint8) << 1) for b in range(ref.B)])


def ref_state(ref):
    return ref_bits(ref), ref.goal, ref.position, ref.direction, ref.episode.copy()


def rehearse(walls, B, steps, limit, seed, action_seed, N=33, nd=16):
    """WallsRef (the dynamics, no frames) under a time limit kept here, a SeenMapRef fed its state: the events of seen_map_ref.account"""
    H, W = walls.shape[-2:]
    ref = WR.WallsRef(B, seed, H, W, N, 24, nd=nd, render=False)
    ref.set_walls(walls)
    seen = SM.SeenMapRef(python_table(nd, N, np.float32), False, *ref_state(ref))
    events = dict.fromkeys(SM.EVENTS, 0)
    steps_taken = np.zeros(B, int)
    rng = np.random.default_rng(action_seed)
    for t in range(steps):
        a = WR.draw_actions(rng, B)
        done = ref.done.astype(bool)
        truncated = (steps_taken >= limit) & ~done if limit else np.zeros(B, bool)
        pose, before, counts = (ref.position, ref.direction), seen.goal_seen.copy(), seen.seen_count.copy()
        for b in np.flatnonzero(truncated):                                 # the limit's restart: the action is ignored, as for a done agent
            ref.worlds[b].done = True
        ref.step(a)
        restarted = done | truncated
        steps_taken = np.where(restarted, 0, steps_taken + 1)
        moved = seen.stepped(*ref_state(ref))
        np.testing.assert_array_equal(moved, restarted)
        SM.account(events, seen, moved, before, done, truncated, pose, (ref.position, ref.direction), a, False, f"step {t}")
        np.testing.assert_array_equal(seen.seen_count[~moved], counts[~moved] + seen.newly_seen[~moved])
        np.testing.assert_array_equal(seen.seen_count, (seen.map != 0).reshape(B, -1).sum(axis=1))
    return ref, seen, events


def test_the_call_table_on_a_rollout():
    ref, seen, events = rehearse(crossed(), 64, 40, 12, 5, 6)
    assert all(v > 0 for v in events.values()), events
    # a masked call: the agents of the mask are cleared and marked, newly_seen = 0; the others keep every byte and their words
    mask = (np.arange(64) % 3 == 0).astype(np.uint8)
    before = (seen.map.copy(), seen.seen_count.copy(), seen.newly_seen.copy(), seen.goal_seen.copy())
    ref.reset(mask)
    seen.masked(*ref_state(ref), mask)
    m = mask != 0
    assert (seen.newly_seen[m] == 0).all() and (seen.recorded[m] == ref.episode[m]).all()
    for now, was in zip((seen.map, seen.seen_count, seen.newly_seen, seen.goal_seen), before):
        np.testing.assert_array_equal(now[~m], was[~m])
    fresh = SM.SeenMapRef(seen.table, False, *ref_state(ref))
    np.testing.assert_array_equal(seen.map[m], fresh.map[m])               # cleared: exactly what the new pose sees
    # the step behind it clears nobody again: the counter was recorded
    ref.step(np.full(64, 3, np.uint8))
    moved = seen.stepped(*ref_state(ref))
    assert not moved[m].any()
    # a goal put into a wall reads 4 once seen
    bits = ring(6, 6).astype(np.uint8)[None].copy()
    bits[0, 5, 2] |= 2
    r = SM.SeenMapRef(straight_table(np.float32), False, bits, np.array([[6, 3]]), np.array([[1.5, 2.5]], np.float32), np.array([0]), np.array([1], np.uint32))
    assert r.map[0, 5, 2] == 4 and r.goal_seen[0] == 1 and r.seen_count[0] == 5
    # a goal off the map: goal_seen = 0
    r = SM.SeenMapRef(straight_table(np.float32), False, ring(6, 6).astype(np.uint8)[None], np.array([[0, 3]]), np.array([[1.5, 2.5]], np.float32), np.array([0]), np.array([1], np.uint32))
    assert r.goal_seen[0] == 0


def test_the_gpu_rollouts_reach_their_events():
    """what tests/test_gpu_seen_map.py asserts of its rollouts happens with the Python dynamics too: the same layouts, rays, seeds and
    lengths.  (The engine's ray table may differ from python_table in a rounding, so its counts may differ by a few — not by their sign:
    the rarest event below happens 11 times.)"""
    from raycastworlds_jl_amd import layouts

    rng = np.random.default_rng(9)
    mazes = np.stack([layouts.maze(9, 9, rng) for _ in range(64)])
    for walls, N in ((ring(4, 4), 1), (ring(7, 9), 33), (ring(5, 13), 257), (crossed(), 33), (crossed(), 64), (mazes, 33)):
        _, _, events = rehearse(walls, 64, 40, 12, 5, 6, N=N)
        assert all(v >= 11 for v in events.values()), (walls.shape, N, events)


# ---- the declarations ------------------------------------------------------------------------------------------------------------------
EXPORTS = ("rcw_set_seen_map", "rcw_seen_map_enabled", "rcw_seen_words", "rcw_seen_words_device_ptr", "rcw_seen_map", "rcw_seen_map_device_ptr")


def test_the_header_declares_the_six_exports():
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "rcw.h")).read()
    for name in EXPORTS:
        assert re.search(r"RCW_API int %s\(rcw_handle\* h[,)]" % name, header), name
    assert "#define RCW_ABI_VERSION 4" in header                            # additive: the version stays
    assert header.index("the goal distance") < header.index("the seen map")


def test_the_six_exports_are_bound_and_refuse_a_null_handle(rcw):
    import ctypes as C

    from raycastworlds_jl_amd import _capi

    lib = _capi.load()
    for name in EXPORTS:
        assert name in _capi.SIGNATURES and hasattr(lib, name), name
    n, p = C.c_int32(7), C.c_void_p()
    word = (C.c_int32 * 1)()
    calls = [lib.rcw_set_seen_map(None, 1), lib.rcw_seen_map_enabled(None, C.byref(n)), lib.rcw_seen_words(None, word, None, None),
             lib.rcw_seen_words_device_ptr(None, C.byref(p), None, None), lib.rcw_seen_map(None, 0, 1, word), lib.rcw_seen_map_device_ptr(None, C.byref(p))]
    assert calls == [_capi.RCW_ERR_INVALID_ARGUMENT] * 6, calls
    assert _capi.last_error(lib)


def test_the_python_mirror_has_the_feature(rcw):
    import inspect

    SR = rcw.SingleRoomModule.SingleRoom
    assert inspect.signature(SR.__init__).parameters["seen_map"].default is False
    assert inspect.signature(SR.set_seen_map).parameters["on"].default is True
    for name in ("seen_count", "seen_new", "goal_seen", "seen_map", "seen_map_device", "seen_map_enabled"):
        assert isinstance(getattr(SR, name), property), name
