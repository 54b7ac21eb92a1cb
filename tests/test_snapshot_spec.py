"""The state archive without a device (include/rcw.h, "the state archive"), through the development build:

  * rcw_dev_snapshot_plan            the record's segment table for a shape — names, bytes, row_bytes, shape key;
  * rcw_dev_step_facts, event 9      what a restore does to the facts of the step (StepFacts::restored);
  * rcw_dev_snapshot_validate_row    rcw_snapshot_rows_load's host check of one exported row.

The expected tables are written out by hand from the list in include/rcw.h.  CPU only."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from test_step_state import ACT, MASK, ONE, PRIME, Handle, row

SHAPE_FIELDS = ("H", "W", "nd", "N", "Hc", "real64", "reward_type", "goal", "seen", "stats", "view_fmt", "view_layout", "view_C", "view_h",
                "view_w", "view_frames", "local_source", "local_size", "local_cells", "source_kind", "layouts", "levels", "first_level")
GRAY8, BANK, MAZES = 2, 1, 2

BASE = dict(H=8, W=8, nd=128, N=64, Hc=64)
# every feature on, on a 4 x 4 map: gray 7 x 9 with k = 3, a 5 x 5 local map of the seen map, a bank of three layouts
ALL_ON = dict(H=4, W=4, nd=128, N=64, Hc=64, goal=1, seen=1, stats=1, view_fmt=GRAY8, view_C=1, view_h=7, view_w=9, view_frames=3,
              local_source=2, local_size=5, local_cells=1, source_kind=BANK, layouts=3)
F64_5X5 = dict(H=5, W=5, nd=128, N=64, Hc=64, real64=1, goal=1, seen=1, stats=1)

EXPECTED = {
    "none": (BASE, [("pos", 8), ("dir", 4), ("goal", 8), ("reward", 4), ("done", 1), ("episode", 4), ("tile_map", 16), ("episode_steps", 4),
                    ("truncated", 1)], 50),
    "all": (ALL_ON, [("pos", 8), ("dir", 4), ("goal", 8), ("reward", 4), ("done", 1), ("episode", 4), ("tile_map", 8), ("episode_steps", 4),
                     ("truncated", 1),
                     ("goal_distance.field", 32), ("goal_distance.distance", 4), ("goal_distance.start_distance", 4),
                     ("goal_distance.progress", 4), ("goal_distance.last_episode", 4),
                     ("seen_map.seen_count", 4), ("seen_map.newly_seen", 4), ("seen_map.goal_seen", 4), ("seen_map.last_episode", 4),
                     ("seen_map.bits", 4), ("seen_map.map", 16),
                     ("learner_view.stack", 189), ("learner_view.last_episode", 4),
                     ("local_map.image", 25),
                     ("layout_source.last_episode", 4), ("layout_source.layout", 4),
                     ("episode_stats.finished", 1), ("episode_stats.outcome", 1), ("episode_stats.length", 4), ("episode_stats.moves", 4),
                     ("episode_stats.level", 4), ("episode_stats.spl_q16", 4), ("episode_stats.episodes", 4), ("episode_stats.prev_x", 4),
                     ("episode_stats.prev_y", 4), ("episode_stats.last_episode", 4)], 386),
    "f64_5x5": (F64_5X5, [("pos64", 16), ("dir", 4), ("goal", 8), ("reward", 4), ("done", 1), ("episode", 4), ("tile_map", 8),
                          ("episode_steps", 4), ("truncated", 1),
                          ("goal_distance.field", 50), ("goal_distance.distance", 4), ("goal_distance.start_distance", 4),
                          ("goal_distance.progress", 4), ("goal_distance.last_episode", 4),
                          ("seen_map.seen_count", 4), ("seen_map.newly_seen", 4), ("seen_map.goal_seen", 4), ("seen_map.last_episode", 4),
                          ("seen_map.bits", 4), ("seen_map.map", 25),
                          ("episode_stats.finished", 1), ("episode_stats.outcome", 1), ("episode_stats.length", 4), ("episode_stats.moves", 4),
                          ("episode_stats.level", 4), ("episode_stats.spl_q16", 4), ("episode_stats.episodes", 4), ("episode_stats.prev_x", 8),
                          ("episode_stats.prev_y", 8), ("episode_stats.last_episode", 4)], 203),
}


@pytest.fixture(scope="module")
def devlib(rcw):
    from raycastworlds_jl_amd import _capi

    if not os.path.exists(_capi.DEV_LIB_PATH):
        from raycastworlds_jl_amd import build as _build

        _build.build()
    lib = C.CDLL(_capi.DEV_LIB_PATH)
    lib.rcw_dev_step_facts.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32)]
    lib.rcw_dev_snapshot_plan.argtypes = [C.POINTER(C.c_int32), C.c_char_p, C.c_int32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.rcw_dev_snapshot_validate_row.argtypes = [C.POINTER(C.c_int32), C.c_char_p, C.c_char_p, C.c_int32]
    return lib


def shape(**kw):
    assert not set(kw) - set(SHAPE_FIELDS)
    return (C.c_int32 * len(SHAPE_FIELDS))(*[kw.get(f, 0) for f in SHAPE_FIELDS])


def plan(lib, **kw):
    names, sizes = C.create_string_buffer(4096), (C.c_uint32 * 64)()
    row_bytes, key = C.c_uint64(), C.c_uint64()
    n = lib.rcw_dev_snapshot_plan(shape(**kw), names, 4096, sizes, C.byref(row_bytes), C.byref(key))
    assert n > 0
    return list(zip(names.value.decode().split("\n")[:n], sizes[:n])), row_bytes.value, key.value


@pytest.mark.parametrize("case", sorted(EXPECTED))
def test_the_segment_table_is_the_one_written_out_by_hand(devlib, case):
    kw, table, total = EXPECTED[case]
    segments, row_bytes, _ = plan(devlib, **kw)
    assert segments == table
    assert row_bytes == sum(b for _, b in table) == total
    assert len(segments) <= 36


def test_the_shape_key_tells_every_feature_dimension_and_kind_apart(devlib):
    base = plan(devlib, **ALL_ON)[2]
    assert base == plan(devlib, **ALL_ON)[2] and base != 0
    others = {
        "goal distance off": dict(ALL_ON, goal=0),
        "seen map off": dict(ALL_ON, seen=0, local_source=1),
        "statistics off": dict(ALL_ON, stats=0),
        "learner view off": dict(ALL_ON, view_fmt=0, view_C=0, view_h=0, view_w=0, view_frames=0),
        "local map off": dict(ALL_ON, local_source=0, local_size=0, local_cells=0),
        "layout source off": dict(ALL_ON, source_kind=0, layouts=0),
        "view 9 x 7, the same bytes": dict(ALL_ON, view_h=9, view_w=7),
        "k = 1": dict(ALL_ON, view_frames=1),
        "k = 4": dict(ALL_ON, view_frames=4),
        "local map 7": dict(ALL_ON, local_size=7),
        "local map of the world": dict(ALL_ON, local_source=1),
        "mazes, the same bytes": dict(ALL_ON, source_kind=MAZES, layouts=0),
        "Float64": dict(ALL_ON, real64=1),
        "Int32 rewards, the same bytes": dict(ALL_ON, reward_type=2),
        "another map": dict(ALL_ON, H=5),
        "more directions": dict(ALL_ON, nd=64),
    }
    keys = {name: plan(devlib, **kw)[2] for name, kw in others.items()}
    assert base not in keys.values()
    assert len(set(keys.values())) == len(keys)
    # the source's RANGE is a setting of the handle, not part of the shape
    assert plan(devlib, **dict(ALL_ON, layouts=7))[2] == base


def test_a_restore_forgets_the_slots_and_the_next_step_primes(devlib):
    """restored = forget + obs_unknown.  Unmasked: the restore's own render is the prime, the step behind it one launch that may keep.
    Masked: the render rewrites the masked agents' slots only, so the next step primes — every agent's successors are cast again, the
    unmasked agents' may have been previews of the state the masked agents left — and only the one behind it is one launch with keep."""
    h = Handle(devlib)
    h.create()
    assert h.step() == row(on=1, primed=1, obs_current=1, cur=1, cols_stale=1, path=ONE, keep=1)
    assert h.event(9) == row(on=1, primed=0, obs_current=0, cur=1, cols_stale=1)
    assert h.camera(0) == row(on=1, primed=1, obs_current=1, cur=1, cols_stale=0, path=PRIME)
    assert h.step() == row(on=1, primed=1, obs_current=1, cur=0, cols_stale=1, path=ONE, keep=1)

    m = Handle(devlib)
    m.create()
    m.step()
    assert m.event(9) == row(on=1, primed=0, obs_current=0, cur=1, cols_stale=1)
    assert m.camera(MASK) == row(on=1, primed=0, obs_current=0, cur=1, cols_stale=1, path=PRIME)
    assert m.step() == row(on=1, primed=1, obs_current=1, cur=1, cols_stale=0, path=PRIME)
    assert m.step() == row(on=1, primed=1, obs_current=1, cur=0, cols_stale=1, path=ONE, keep=1)

    # the two-launch form has no slots to forget: a restore changes no fact
    t = Handle(devlib, eligible=0)
    t.create()
    before = t.step()
    assert t.event(9) == before._replace(path=-1, keep=0)
    assert t.camera(MASK).path == 0 and t.step(0).path == 0
    assert ACT == 1


def valid_row(lib, kw):
    segments, row_bytes, _ = plan(lib, **kw)
    offset, at = 0, {}
    for name, b in segments:
        at[name] = offset
        offset += b
    H, W = kw["H"], kw["W"]
    r = bytearray(row_bytes)
    if kw.get("real64"):
        struct.pack_into("<dd", r, at["pos64"], 1.5, 2.25)
    else:
        struct.pack_into("<ff", r, at["pos"], 1.5, 2.25)
    struct.pack_into("<i", r, at["dir"], kw["nd"] - 1)
    struct.pack_into("<ii", r, at["goal"], 2, W - 1)
    bits = np.zeros(8 * dict(segments)["tile_map"], dtype=np.uint8)
    for j in range(W):
        for i in range(H):
            if i in (0, H - 1) or j in (0, W - 1):
                bits[2 * (i + H * j)] = 1
    bits[2 * (1 + H * (W - 2)) + 1] = 1                                   # the goal layer's bit of the goal tile
    r[at["tile_map"]:at["tile_map"] + len(bits) // 8] = np.packbits(bits, bitorder="little").tobytes()
    if kw.get("source_kind"):
        struct.pack_into("<i", r, at["layout_source.layout"], kw["layouts"] - 1)
    return r, at


def validate(lib, kw, r):
    msg = C.create_string_buffer(256)
    rc = lib.rcw_dev_snapshot_validate_row(shape(**kw), bytes(r), msg, 256)
    return rc, msg.value.decode()


@pytest.mark.parametrize("case", ["all", "f64_5x5"])
def test_a_row_is_refused_for_each_field_a_kernel_indexes_with(devlib, case):
    from raycastworlds_jl_amd import _capi

    kw = EXPECTED[case][0]
    good, at = valid_row(devlib, kw)
    assert validate(devlib, kw, good) == (0, "")
    H, W = kw["H"], kw["W"]
    pos = "pos64" if kw.get("real64") else "pos"
    nan = struct.pack("<d", float("nan")) if kw.get("real64") else struct.pack("<f", float("nan"))

    def flip(bit):
        def f(r):
            r[at["tile_map"] + bit // 8] ^= 1 << (bit % 8)
        return f

    corruptions = [
        ("goal", lambda r: struct.pack_into("<ii", r, at["goal"], 1, 2)),                      # on the border
        ("goal", lambda r: struct.pack_into("<ii", r, at["goal"], 2, W)),
        ("dir", lambda r: struct.pack_into("<i", r, at["dir"], kw["nd"])),
        ("dir", lambda r: struct.pack_into("<i", r, at["dir"], -1)),
        (pos, lambda r: r.__setitem__(slice(at[pos], at[pos] + len(nan)), nan)),
        (pos, lambda r: r.__setitem__(slice(at[pos], at[pos] + len(nan)), struct.pack("<d" if kw.get("real64") else "<f", H - 1.0))),
        ("tile_map", flip(0)),                                                                 # the corner's WALL bit
        ("tile_map", flip(2 * ((H - 1) + H * (W - 1)))),
        ("tile_map", flip(2 * H * W)),                                                         # the first padding bit
        ("tile_map", flip(63)),
    ]
    if kw.get("source_kind"):
        corruptions += [("layout_source.layout", lambda r: struct.pack_into("<i", r, at["layout_source.layout"], kw["layouts"])),
                        ("layout_source.layout", lambda r: struct.pack_into("<i", r, at["layout_source.layout"], -1))]
    for field, corrupt in corruptions:
        r = bytearray(good)
        corrupt(r)
        assert r != good
        rc, msg = validate(devlib, kw, r)
        assert rc == _capi.RCW_ERR_INVALID_ARGUMENT and msg.startswith(field + ":"), (field, rc, msg)
    # what no kernel indexes with is the caller's word
    r = bytearray(good)
    struct.pack_into("<i", r, at["episode"], -5)
    r[at["seen_map.map"]] = 200
    assert validate(devlib, kw, r) == (0, "")


def test_a_family_without_levels_takes_minus_one_and_a_level_range_its_levels(devlib):
    kw = dict(ALL_ON, source_kind=MAZES, layouts=0, levels=0)
    r, at = valid_row(devlib, dict(kw, layouts=0))
    for value, ok in ((-1, True), (0, False)):
        struct.pack_into("<i", r, at["layout_source.layout"], value)
        assert (validate(devlib, kw, r)[0] == 0) == ok
    kw = dict(kw, levels=4, first_level=10)
    for value, ok in ((9, False), (10, True), (13, True), (14, False), (-1, False)):
        struct.pack_into("<i", r, at["layout_source.layout"], value)
        assert (validate(devlib, kw, r)[0] == 0) == ok


def test_the_rewinds_windows_hold_what_the_gpu_test_claims():
    """tests/snapshot_cases.py's rewinds rehearsed on the CPU — tests/wall_bank_ref.py under tests/time_limit_ref.py, every feature that moves
    the dynamics (bank, weights, limit, auto_reset) as the engine has it: each window behind the save holds at least one restart behind a
    goal, one truncation and one turn-only step, the lone agent's included, and exactly the counts of REHEARSED"""
    import snapshot_cases as SC

    for (B, c, _, T, _, seed, action_seed), want in zip(SC.REWINDS, SC.REHEARSED):
        ev = SC.rehearse(B, c, T, SC.actions(B, SC.T1 + SC.T2, seed=action_seed), SC.T1, seed=seed)
        assert tuple(ev[k] for k in SC.EVENTS) == want, (B, ev)
        assert min(want[:3]) >= 1


def test_the_host_rules_under_asan_and_ubsan_as_a_program_of_their_own(tmp_path):
    """tests/san_snapshot_main.cpp with csrc/rcw_rules.hip in one translation unit, host side only, under -fsanitize=address,undefined: the
    record's plan and the row check on rows that end exactly where the heap block ends.  A stand-alone program on the CPU, as
    oracle/san_walls_main.c is for the oracle's walls: no sanitizer's runtime is loaded into Python."""
    import shutil
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "san_snapshot")
    build = subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
                            "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-o", exe,
                            os.path.join(root, "tests", "san_snapshot_main.cpp")], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    assert run.returncode == 0 and "san_snapshot_main: ok" in run.stdout, run.stdout[-2000:] + run.stderr[-3000:]
    assert "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
