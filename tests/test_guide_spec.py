"""The guide's rule (include/rcw.h, "the guide") anchored on the CPU:

  * hand-derived cases, held by the library's handle-less export (rcw_guide_rule, through layouts.guide_rule) AND by the reference of the
    GPU tests (tests/guide_ref.py): the next tile on each of the four sides and their order of preference, every heading against it, the
    `<=` of the re-centring at exactly inc and at the next float beyond, delta == nd / 2, an odd nd, the no-advice cases, ties and NaNs
    in the table;
  * the export against the reference on random states, both world-unit types, shuffled tables with duplicates;
  * THE PROMISE on the reference alone, with a small act! beside it: for nd in {4, 16, 128} and (inc, r) in {(1/8, 1/8), (1/4, 1/4),
    (0.2, 0.3)}, on a maze, pillars, four rooms and the serpentine, every start l tiles from the goal arrives within
    (l + 1) (nd / 2 + 2 ceil(1 / inc)) steps — from tile centres and from anywhere in the tile the circle fits;
  * `promised` for those three and for r = 0.45, inc = 1/8 (where it is 0), through the development build;
  * the export under ASan and UBSan as a program of its own (tests/san_guide_main.cpp).

The export is missing from the build before this feature: every test that calls it fails there.  CPU only."""
import ctypes as C
import os

import numpy as np
import pytest

import goal_distance_ref as GD
import guide_ref as GR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = [np.float32, np.float64]
COMPASS = [(1, 0), (0, 1), (-1, 0), (0, -1)]                                  # +i, +j, -i, -j: exact in both types
INC = 0.125


def both(rcw, field, x, y, d, table, inc, T):
    """(action, heading) by the library's export and by the reference: they must agree before either is held to a literal"""
    from raycastworlds_jl_amd import layouts

    lib = layouts.guide_rule(field, (x, y), d, table, inc, T="Float64" if T is np.float64 else "Float32")
    ref = GR.rule(field, x, y, d, table, inc, T)
    assert lib == ref, (lib, ref)
    return lib


def around(side, f=5):
    """5 x 5, everything 0xFFFF but the middle tile (2, 2) = f, the neighbour on `side` = f - 1 and the other three = f + 1"""
    field = np.full((5, 5), 0xFFFF, np.uint16)
    field[2, 2] = f
    for s, (a, b) in enumerate(((1, 2), (3, 2), (2, 1), (2, 3))):
        field[a, b] = (f - 1) & 0xFFFF if s in (side if isinstance(side, tuple) else (side,)) else f + 1
    return field


@pytest.mark.parametrize("T", TYPES, ids=["f32", "f64"])
def test_at_a_tile_centre_the_next_tile_on_each_side_against_every_heading(rcw, T):
    wanted = {0: 2, 1: 0, 2: 3, 3: 1}                                        # (i-1, j): -i is entry 2; (i+1, j): 0; (i, j-1): 3; (i, j+1): 1
    for side, heading in wanted.items():
        for d in range(4):
            delta = (heading - d) % 4
            action = {0: 1, 1: 3, 2: 3, 3: 4}[delta]                           # delta == nd / 2 turns LEFT
            assert both(rcw, around(side), 2.5, 2.5, d, COMPASS, INC, T) == (action, heading), (side, d)
    # two nearer neighbours: the first in the order (i-1, j), (i+1, j), (i, j-1), (i, j+1)
    assert both(rcw, around((0, 3)), 2.5, 2.5, 2, COMPASS, INC, T) == (1, 2)
    assert both(rcw, around((1, 2)), 2.5, 2.5, 0, COMPASS, INC, T) == (1, 0)
    assert both(rcw, around((2, 3)), 2.5, 2.5, 3, COMPASS, INC, T) == (1, 3)
    # a goal next door (f = 1, the neighbour holds 0)
    assert both(rcw, around(1, f=1), 2.5, 2.5, 0, COMPASS, INC, T) == (1, 0)


@pytest.mark.parametrize("T", TYPES, ids=["f32", "f64"])
def test_the_recentring_boundary_is_less_or_equal_at_exactly_inc(rcw, T):
    up = lambda v: float(np.nextafter(T(v), T(np.inf)))
    down = lambda v: float(np.nextafter(T(v), T(-np.inf)))
    # travel along i (the next tile is (3, 2)): the offset is y - 2.5
    assert both(rcw, around(1), 2.5, 2.5 + INC, 0, COMPASS, INC, T) == (1, 0)             # |e| == inc: go
    assert both(rcw, around(1), 2.5, up(2.5 + INC), 0, COMPASS, INC, T) == (4, 3)         # one float beyond: back to the axis, -j
    assert both(rcw, around(1), 2.5, 2.5 - INC, 0, COMPASS, INC, T) == (1, 0)
    assert both(rcw, around(1), 2.5, down(2.5 - INC), 0, COMPASS, INC, T) == (3, 1)       # +j
    # travel along j (the next tile is (2, 1)): the offset is x - 2.5
    assert both(rcw, around(2), 2.5 + INC, 2.5, 3, COMPASS, INC, T) == (1, 3)
    assert both(rcw, around(2), up(2.5 + INC), 2.5, 3, COMPASS, INC, T) == (4, 2)         # -i
    assert both(rcw, around(2), down(2.5 - INC), 2.5, 3, COMPASS, INC, T) == (3, 0)       # +i
    # off the axis ALONG the travel does not matter
    assert both(rcw, around(1), 2.9, 2.5, 0, COMPASS, INC, T) == (1, 0)
    assert both(rcw, around(1), 2.01, 2.5 + INC, 0, COMPASS, INC, T) == (1, 0)


@pytest.mark.parametrize("T", TYPES, ids=["f32", "f64"])
def test_half_a_turn_goes_left_and_an_odd_table(rcw, T):
    t8 = GR.direction_table(8, T)
    assert both(rcw, around(1), 2.5, 2.5, 4, t8, INC, T) == (3, 0)            # delta 4 == nd / 2
    assert both(rcw, around(1), 2.5, 2.5, 3, t8, INC, T) == (4, 0)            # delta 5
    assert both(rcw, around(1), 2.5, 2.5, 5, t8, INC, T) == (3, 0)            # delta 3
    t7 = GR.direction_table(7, T)                                             # cos(2 pi k / 7): the greatest at k = 0
    assert both(rcw, around(1), 2.5, 2.5, 0, t7, INC, T) == (1, 0)
    assert both(rcw, around(1), 2.5, 2.5, 4, t7, INC, T) == (3, 0)            # delta 3 == 7 // 2: left (5, 6, 0)
    assert both(rcw, around(1), 2.5, 2.5, 3, t7, INC, T) == (4, 0)            # delta 4: right (2, 1, 0)
    assert both(rcw, around(0), 2.5, 2.5, 0, t7, INC, T)[1] in (3, 4)         # towards -i: cos is least at k = 3 and 4
    assert both(rcw, around(1), 2.5, 2.5, 0, [(1, 0)], INC, T) == (1, 0)      # nd = 1: always forward
    assert both(rcw, around(0), 2.5, 2.5, 0, [(1, 0)], INC, T) == (1, 0)


@pytest.mark.parametrize("T", TYPES, ids=["f32", "f64"])
def test_where_there_is_no_advice_the_agent_turns_on_the_spot(rcw, T):
    none = (3, -1)
    assert both(rcw, around(1, f=0), 2.5, 2.5, 0, COMPASS, INC, T) == none                  # on the goal tile
    field = around(1)
    field[2, 2] = 0xFFFF
    assert both(rcw, field, 2.5, 2.5, 0, COMPASS, INC, T) == none                           # no path
    assert both(rcw, around(1), 0.5, 2.5, 0, COMPASS, INC, T) == none                       # a tile of the ring
    for x, y in ((np.nan, 2.5), (2.5, np.nan), (np.inf, 2.5), (2.5, -np.inf), (-0.5, 2.5), (2.5, 5.0), (5.0, 2.5), (2.5, -1e-3), (1e30, 2.5), (3e9, 3e9)):
        assert both(rcw, around(1), x, y, 0, COMPASS, INC, T) == none, (x, y)
    assert both(rcw, np.full((5, 5), 7, np.uint16), 2.5, 2.5, 0, COMPASS, INC, T) == none   # no flood's field: nothing is nearer
    corner = np.full((5, 5), 0xFFFF, np.uint16)
    corner[0, 0], corner[4, 4] = 3, 3                                                       # (the neighbours off the map are not looked at)
    assert both(rcw, corner, 0.5, 0.5, 0, COMPASS, INC, T) == none
    assert both(rcw, corner, 4.5, 4.5, 0, COMPASS, INC, T) == none


@pytest.mark.parametrize("T", TYPES, ids=["f32", "f64"])
def test_of_equal_entries_the_smaller_index_wins_and_a_nan_never(rcw, T):
    nan = np.nan
    assert both(rcw, around(1), 2.5, 2.5, 0, [(1, 0), (1, 0), (0, 1), (-1, 0)], INC, T) == (1, 0)
    assert both(rcw, around(1), 2.5, 2.5, 0, [(0, 1), (1, 0), (1, 0), (1, 0)], INC, T) == (3, 1)
    assert both(rcw, around(1), 2.5, 2.5, 0, [(nan, 0), (0, nan), (1, 0), (1, 0)], INC, T) == (3, 2)
    assert both(rcw, around(1), 2.5, 2.5, 0, [(np.inf, np.inf), (-1, 0), (-2, 0)], INC, T) == (3, 1)   # inf * 1 + inf * 0 is NaN
    assert both(rcw, around(1), 2.5, 2.5, 2, [(nan, nan)] * 5, INC, T) == (4, 0)                      # all NaN: heading 0, delta 3 of 5
    assert both(rcw, around(1), 2.5, 2.5, 0, [(0.0, 1), (-0.0, 1), (0, -1)], INC, T) == (1, 0)        # +0 and -0 compare equal


ND = [1, 2, 3, 4, 7, 64, 65, 128, 130, 1000]


@pytest.mark.parametrize("T", TYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("nd", ND)
def test_the_export_equals_the_reference_on_random_states(rcw, nd, T):
    from raycastworlds_jl_amd import layouts

    rng = np.random.default_rng(1000 * nd + (T is np.float64))
    base = GR.direction_table(nd, T)
    seen = {1: 0, 3: 0, 4: 0, -1: 0}
    for trial in range(12):
        H, W = (int(v) for v in rng.integers(5, 18, 2))
        walls = GD.pillars(H, W, 0.2, rng)
        free = np.argwhere(~walls)
        goal = free[rng.integers(len(free))] + 1
        field = GD.bfs_field(walls, goal)
        table = base[rng.integers(0, nd, nd)] if trial % 3 == 1 else rng.permutation(base)   # shuffled; every third with duplicates
        inc = [0.125, 0.25, 0.2, 0.37][trial % 4]
        for _ in range(40):
            if rng.random() < 0.9:                                           # inside a free tile, anywhere in it (the tile's edges included)
                i, j = free[rng.integers(len(free))]
                x, y = i + rng.choice([0.0, 0.5, 0.5 - inc, 0.5 + inc, rng.random()]), j + rng.choice([0.0, 0.5, 0.5 - inc, 0.5 + inc, rng.random()])
            else:                                                            # anywhere, the walls and beyond the map included
                x, y = rng.uniform(-1, H + 1), rng.uniform(-1, W + 1)
            d = int(rng.integers(nd))
            got = layouts.guide_rule(field, (x, y), d, table, inc, T="Float64" if T is np.float64 else "Float32")
            assert got == GR.rule(field, x, y, d, table, inc, T), (H, W, x, y, d, inc)
            seen[got[0]] += 1
            seen[-1] += got[1] < 0
    assert seen[1] + seen[3] + seen[4] == 480 and seen[-1] >= 10
    assert nd == 1 or (seen[3] > seen[-1] and (seen[4] > 0 or nd == 2))               # (nd = 2: delta 1 == nd / 2 turns left)


# ---- the promise ---------------------------------------------------------------------------------------------------------------------
PARAMS = [(1 / 8, 1 / 8), (1 / 4, 1 / 4), (0.2, 0.3)]


def layout(name, rng):
    from raycastworlds_jl_amd import layouts

    if name == "maze":
        return layouts.maze(11, 13, rng)
    if name == "pillars":
        return GD.pillars(11, 11, 0.3, rng)
    if name == "four_rooms":
        return layouts.four_rooms(11, 12)
    return GD.serpentine(9, 8)


@pytest.mark.parametrize("name", ["maze", "pillars", "four_rooms", "serpentine"])
@pytest.mark.parametrize("inc,radius", PARAMS, ids=["eighth", "quarter", "fifth-0.3"])
@pytest.mark.parametrize("nd", [4, 16, 128])
def test_an_agent_that_follows_the_guide_arrives_within_the_bound(rcw, nd, inc, radius, name):
    """On the reference alone.  Eight starts a case — the farthest tile, three more tile centres, four poses anywhere in the tile the
    circle fits — alternating between the two world-unit types; every one with a path (l >= 1) must arrive."""
    rng = np.random.default_rng([nd, int(1000 * inc), int(1000 * radius), len(name)])
    walls = layout(name, rng)
    free = np.argwhere(~walls)
    goal = free[rng.integers(len(free))] + 1
    field = GD.bfs_field(walls, goal)
    reach = np.argwhere((field != GD.UNREACHED) & (field > 0))
    assert len(reach) >= 4
    far = reach[np.argmax(field[reach[:, 0], reach[:, 1]])]
    starts = [far] + [reach[rng.integers(len(reach))] for _ in range(7)]
    wm, gm = GR._map(walls), GR._map(field == 0)
    worst = 0.0
    for n, (i, j) in enumerate(starts):
        T = TYPES[n % 2]
        table = GR.direction_table(nd, T)
        pos = (i + 0.5, j + 0.5)
        if n >= 4:
            for _ in range(1000):
                q = (i + rng.random(), j + rng.random())
                if not any(GR.collides(wm, gm, q, T(radius), T)):
                    pos = q
                    break
        l = int(field[i, j])
        limit = GR.bound(l, nd, inc)
        steps = GR.follow(walls, field, goal, pos, int(rng.integers(nd)), table, inc, radius, T, limit)
        assert steps is not None, f"{name}, nd {nd}, inc {inc}, r {radius}, {T.__name__}: the agent at {pos}, {l} tiles out, did not arrive in {limit} steps"
        worst = max(worst, steps / limit)
    assert 0 < worst <= 1


def config(rcw, T, inc, radius):
    from raycastworlds_jl_amd import _capi

    cfg = _capi.default_config()
    cfg.world_unit_bits = 64 if T is np.float64 else 32
    cfg.position_increment_wu, cfg.player_radius_wu = inc, radius
    cfg.position_increment_wu_f64, cfg.player_radius_wu_f64 = inc, radius
    return cfg


@pytest.mark.parametrize("T", TYPES, ids=["f32", "f64"])
def test_promised_says_which_case_a_configuration_is_in(rcw, T):
    from raycastworlds_jl_amd import _capi

    if not os.path.exists(_capi.DEV_LIB_PATH):
        from raycastworlds_jl_amd import build as _build

        _build.build()
    lib = _capi.load("dev")
    promised = lambda inc, r: lib.rcw_dev_guide_promised(C.byref(config(rcw, T, inc, r)))
    assert promised(1 / 8, 0.45) == 0                                        # the setting at which the prototype's agents got stuck
    for inc, r in PARAMS:
        assert promised(inc, r) == 1
    assert promised(0.25, 0.25) == 1 and promised(0.25, 0.26) == 0 and promised(0.5, 1e-3) == 0
    assert lib.rcw_dev_guide_promised(None) < 0


def test_the_rule_under_asan_and_ubsan_as_a_program_of_its_own(tmp_path):
    """tests/san_guide_main.cpp with csrc/rcw_rules.hip in one translation unit, host side only, under -fsanitize=address,undefined:
    rcw_guide_rule on hostile positions, fields and tables, each in a heap block of exactly its size.  A stand-alone program on the CPU:
    no sanitizer's runtime is loaded into Python."""
    import shutil
    import subprocess

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "san_guide")
    build = subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
                            "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-o", exe,
                            os.path.join(ROOT, "tests", "san_guide_main.cpp")], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    assert run.returncode == 0 and "san_guide_main: ok" in run.stdout, run.stdout[-2000:] + run.stderr[-3000:]
    assert "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
