"""The frontier's definition (include/rcw.h, "the frontier") anchored on the CPU:

  * literal cases, held by the library's handle-less export (rcw_frontier_rule, through layouts.frontier_rule) AND by the reference of the
    GPU tests (tests/frontier_ref.py): a fully seen room, an unseen map, one seen tile, a wall in between, which bytes pass, sources on
    the map's first row and column, and the column-wrap pair — tiles (H-1, j) and (0, j+1), adjacent in linear order, no neighbours;
  * 200 seen maps made by seen_map_ref's march from random poses on pillars and mazes at 5 x 5, 9 x 9, 17 x 13 and 40 x 40: the export
    against the numpy flood;
  * the refused arguments;
  * the frontier's per-agent arrays, none of them archived: a shape with the frontier plans the record, and the key, it plans without;
  * the closed loop on the reference: 16 agents on 13 x 13 generated mazes explore everything, or reach their goal, within 2,000 steps;
  * the export under ASan and UBSan as a program of its own (tests/san_frontier_main.cpp).

The export is missing from the build before this feature: every test that calls it fails there.  CPU only."""
import ctypes as C
import os

import numpy as np
import pytest

import frontier_ref as FR
import goal_distance_ref as GD
import seen_map_ref as SM
from test_snapshot_spec import ALL_ON, F64_5X5, devlib, plan, shape  # noqa: F401  (devlib: the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X = 0xFFFF


def both(rcw, seen_map):
    """(field, tiles) by the library's export and by the reference: they must agree before either is held to a literal"""
    from raycastworlds_jl_amd import layouts

    m = np.asarray(seen_map, np.uint8)
    field, tiles = layouts.frontier_rule(m)
    ref, ref_tiles = FR.flood(m)
    assert field.dtype == np.uint16 and field.shape == m.shape
    np.testing.assert_array_equal(field, ref)
    assert tiles == ref_tiles == int((field == 0).sum())
    return field, tiles


def seen_ring(n=5):
    """a fully seen n x n room: the ring 2, the interior 1"""
    m = np.full((n, n), 2, np.uint8)
    m[1:-1, 1:-1] = 1
    return m


def test_nothing_is_left_in_a_fully_seen_room_and_nothing_starts_on_an_unseen_map(rcw):
    field, tiles = both(rcw, seen_ring())
    assert tiles == 0 and (field == X).all()
    field, tiles = both(rcw, np.zeros((5, 5), np.uint8))
    assert tiles == 0 and (field == X).all()


def test_one_seen_tile_has_its_four_neighbours_for_sources(rcw):
    m = np.zeros((5, 5), np.uint8)
    m[2, 2] = 1
    field, tiles = both(rcw, m)
    want = np.full((5, 5), X, np.uint16)
    want[2, 2] = 1
    want[1, 2] = want[3, 2] = want[2, 1] = want[2, 3] = 0
    np.testing.assert_array_equal(field, want)
    assert tiles == 4


def test_a_seen_wall_between_a_passable_and_an_unseen_tile_makes_no_source(rcw):
    m = np.full((3, 5), 2, np.uint8)
    m[1] = (2, 1, 2, 0, 2)                                                    # free | wall | unseen: the unseen tile touches walls only
    field, tiles = both(rcw, m)
    assert tiles == 0 and (field == X).all()
    m[1] = (2, 1, 1, 0, 2)                                                    # free | free | unseen
    field, tiles = both(rcw, m)
    assert tiles == 1 and list(field[1]) == [X, 2, 1, 0, X]


def test_which_bytes_pass(rcw):
    for value, passes in ((1, True), (3, True), (2, False), (4, False), (5, False), (7, False), (129, False), (255, False)):
        m = np.full((3, 5), 2, np.uint8)
        m[1] = (2, 1, value, 0, 2)                                            # the flood must cross `value` to reach the source's other side
        field, tiles = both(rcw, m)
        if passes:
            assert tiles == 1 and list(field[1]) == [X, 2, 1, 0, X], value
        else:
            assert tiles == 0 and (field == X).all(), value


def test_an_unseen_tile_in_the_first_row_or_column_beside_a_passable_one_is_a_source(rcw):
    m = np.full((4, 4), 2, np.uint8)
    m[1, 1] = 1
    m[0, 1] = 0                                                               # row 0
    m[1, 0] = 0                                                               # column 0
    field, tiles = both(rcw, m)
    assert tiles == 2 and field[0, 1] == 0 and field[1, 0] == 0 and field[1, 1] == 1
    m = np.full((4, 4), 2, np.uint8)
    m[2, 2] = 3
    m[3, 2] = 0                                                               # the last row
    m[2, 3] = 0                                                               # the last column
    field, tiles = both(rcw, m)
    assert tiles == 2 and field[3, 2] == 0 and field[2, 3] == 0 and field[2, 2] == 1


@pytest.mark.parametrize("H,W", [(4, 4), (5, 3), (3, 6)])
def test_the_last_tile_of_a_column_and_the_first_of_the_next_are_no_neighbours(rcw, H, W):
    """tile (H-1, j) and tile (0, j+1) are one apart in linear order; with no other contact neither makes the other a source"""
    for j in range(W - 1):
        m = np.full((H, W), 2, np.uint8)
        m[H - 1, j] = 1                                                       # passable, its on-map neighbours are walls
        m[0, j + 1] = 0                                                       # unseen
        field, tiles = both(rcw, m)
        assert tiles == 0 and (field == X).all(), j
        m = np.full((H, W), 2, np.uint8)                                      # ... and the other way round
        m[0, j + 1] = 1
        m[H - 1, j] = 0
        field, tiles = both(rcw, m)
        assert tiles == 0 and (field == X).all(), j
    # a source in row 0 does not flood into the passable tile in front of it in linear order
    m = np.full((H, W), 2, np.uint8)
    m[0, 1] = 0
    m[1, 1] = 1
    m[H - 1, 0] = 1
    field, tiles = both(rcw, m)
    assert tiles == 1 and field[1, 1] == 1 and field[H - 1, 0] == X


def seen_maps(H, W, count, rng):
    """`count` seen maps of H x W: pillars or a maze, a goal, one to twelve poses whose rays (16 of nd 16) mark the map"""
    from raycastworlds_jl_amd import layouts

    table = FR.ray_table(16, 16, np.float32)
    out = []
    while len(out) < count:
        walls = GD.pillars(H, W, 0.25, rng) if len(out) % 2 == 0 or min(H, W) < 5 else layouts.maze(H, W, rng)
        free = np.argwhere(~walls)
        if len(free) < 2:
            continue
        bits = walls.astype(np.uint8)
        g = free[rng.integers(len(free))]
        bits[g[0], g[1]] |= 2
        m = np.zeros((H, W), np.uint8)
        for _ in range(int(rng.integers(1, 13))):
            p = free[rng.integers(len(free))] + rng.random(2)
            marked = SM.marked_tiles(bits[None], p[None].astype(np.float32), np.array([rng.integers(16)]), table, False, np.float32)[0]
            m[marked] = 1 + bits[marked]
        out.append(m)
    return out


def test_the_export_equals_the_numpy_flood_on_200_marched_maps(rcw):
    rng = np.random.default_rng(19)
    seen = dict(maps=0, sources=0, unreachable=0, far=0)
    for H, W in ((5, 5), (9, 9), (17, 13), (40, 40)):
        for m in seen_maps(H, W, 50, rng):
            field, tiles = both(rcw, m)
            passable = (m == 1) | (m == 3)
            assert ((field != X) & (field > 0) == passable & (field != X)).all() and (field[~passable & (field != 0)] == X).all()
            seen["maps"] += 1
            seen["sources"] += tiles
            seen["unreachable"] += int((passable & (field == X)).sum())
            seen["far"] = max(seen["far"], int(field[field != X].max(initial=0)))
    print(seen)
    assert seen["maps"] == 200 and seen["sources"] > 200 and seen["far"] >= 5, seen       # (floods of several levels were among them)


def test_refused_arguments(rcw):
    from raycastworlds_jl_amd import _capi, layouts

    lib = _capi.load()
    m = np.zeros(25, np.uint8)
    f = np.zeros(25, np.uint16)
    n = C.c_int32()
    bad = _capi.RCW_ERR_INVALID_ARGUMENT
    assert lib.rcw_frontier_rule(5, 5, m.ctypes.data, f.ctypes.data, C.byref(n)) == _capi.RCW_OK
    assert lib.rcw_frontier_rule(5, 5, None, f.ctypes.data, C.byref(n)) == bad
    assert lib.rcw_frontier_rule(5, 5, m.ctypes.data, None, C.byref(n)) == bad
    assert lib.rcw_frontier_rule(5, 5, m.ctypes.data, f.ctypes.data, None) == bad
    for H, W in ((0, 5), (5, 0), (-1, 5), (5, -5), (256, 256), (65536, 1), (1, 65536), (65536, 65536), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert lib.rcw_frontier_rule(H, W, m.ctypes.data, f.ctypes.data, C.byref(n)) == bad, (H, W)
    with pytest.raises(ValueError):
        layouts.frontier_rule(np.zeros((2, 3, 3), np.uint8))
    big, tiles = layouts.frontier_rule(np.ones((255, 257), np.uint8))         # H*W == 65535: the largest map
    assert tiles == 0 and (big == X).all()


def test_the_frontiers_arrays_are_never_archived_and_leave_every_record_and_key_alone(devlib):
    devlib.rcw_dev_frontier_plan.argtypes = [C.POINTER(C.c_int32), C.c_char_p, C.c_int32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8),
                                             C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    for kw in (ALL_ON, F64_5X5, dict(H=17, W=13, nd=16, N=8, Hc=8, seen=1)):
        names, sizes, kept = C.create_string_buffer(4096), (C.c_uint32 * 16)(), (C.c_uint8 * 16)()
        segments, row_bytes, key = C.c_int32(), C.c_uint64(), C.c_uint64()
        n = devlib.rcw_dev_frontier_plan(shape(**kw), names, 4096, sizes, kept, C.byref(segments), C.byref(row_bytes), C.byref(key))
        HW = kw["H"] * kw["W"]
        assert n == 6 and names.value.decode().split("\n")[:n] == ["frontier.distance", "frontier.tiles", "frontier.action", "frontier.heading",
                                                                   "frontier.last_episode", "frontier.field"]
        assert list(sizes[:n]) == [4, 4, 1, 4, 4, 2 * HW] and not any(kept[:n])
        without = plan(devlib, **kw)                                          # the same 23 words, the frontier off
        assert (segments.value, row_bytes.value, key.value) == (len(without[0]), without[1], without[2])
    assert devlib.rcw_dev_frontier_plan(None, None, 0, None, None, None, None, None) < 0


# ---- the closed loop on the reference -------------------------------------------------------------------------------------------------
LOOP = dict(agents=16, H=13, W=13, loops=0.1, nd=16, rays=8, inc=0.25, radius=0.25, limit=2000)


def loop_worlds(rng):
    from raycastworlds_jl_amd import layouts

    c = LOOP
    walls, goals, pos = [], [], []
    for a in range(c["agents"]):
        w = layouts.generated_maze(int(rng.integers(1, 2 ** 62)), c["H"], c["W"], loops=c["loops"])
        free = np.argwhere(~w)
        g, p = free[rng.choice(len(free), 2, replace=False)]
        walls.append(w)
        goals.append(g + 1)
        pos.append(p + 0.5)
    return np.stack(walls), np.array(goals), np.array(pos), rng.integers(0, c["nd"], c["agents"])


def test_agents_that_follow_the_rule_explore_everything_or_reach_their_goal_within_2000_steps(rcw):
    c = LOOP
    walls, goals, pos, dirs = loop_worlds(np.random.default_rng(7))
    steps, how = FR.explore(walls, goals, pos, dirs, c["nd"], c["rays"], c["inc"], c["radius"], np.float32, c["limit"])
    print("steps", list(steps), how)
    assert (steps >= 0).all(), (list(steps), how)
    assert steps.max() <= c["limit"] and set(how) <= {"explored", "goal"}
    assert steps.max() > 20                                                   # (they did walk)


def test_the_rule_under_asan_and_ubsan_as_a_program_of_its_own(tmp_path):
    """tests/san_frontier_main.cpp with csrc/rcw_rules.hip in one translation unit, host side only, under -fsanitize=address,undefined:
    rcw_frontier_rule on hostile maps, each map and field in a heap block of exactly its size.  A stand-alone program on the CPU: no
    sanitizer's runtime is loaded into Python."""
    import shutil
    import subprocess

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "san_frontier")
    build = subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
                            "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-o", exe,
                            os.path.join(ROOT, "tests", "san_frontier_main.cpp")], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    assert run.returncode == 0 and "san_frontier_main: ok" in run.stdout, run.stdout[-2000:] + run.stderr[-3000:]
    assert "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
