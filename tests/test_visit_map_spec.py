"""The visit map's definition (include/rcw.h, "the visit map") anchored on the CPU:

  * the cell rule, held by the library's handle-less export (rcw_visit_cell, through layouts.visit_cell) AND by the reference of the GPU
    tests (tests/visit_map_ref.py), in both world-unit types: literal cases — x or y exactly an integer, -0.0, just below H, negative,
    >= H, NaN, +-inf —, sectors 1, 3 and 8 against nd 8, 16 and 130 with d = nd - 1 among them, and 2,000 random poses;
  * the refused arguments;
  * the plan: parts, bytes, `archived` and carve of kFeatVisits, the table's rows rule and the byte cap, and that a shape with the feature
    off plans exactly the segments, and the key, it planned before;
  * the rules under ASan and UBSan as a program of its own (tests/san_visit_main.cpp).

The exports are missing from the build before this feature: every test here fails there.  CPU only."""
import ctypes as C
import os

import numpy as np
import pytest

import visit_map_ref as VR
from test_snapshot_spec import ALL_ON, F64_5X5, SHAPE_FIELDS, devlib, plan  # noqa: F401  (devlib: the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = [np.float32, np.float64]
BANK, MAZES = 1, 2
CAP = 256 << 20


def both(H, W, nd, sectors, x, y, d, T):
    """the cell by the library's export and by the reference: they must agree before either is held to a literal"""
    from raycastworlds_jl_amd import layouts

    got = layouts.visit_cell(H, W, nd, sectors, (x, y), d, T)
    ref = int(VR.cell_index(H, W, nd, sectors, np.array([[x, y]], T), np.array([d]))[0])
    assert got == ref, (H, W, nd, sectors, x, y, d, T, got, ref)
    return got


@pytest.mark.parametrize("T", TYPES)
def test_the_tile_of_literal_positions(rcw, T):
    H, W = 5, 7
    inf, nan = float("inf"), float("nan")
    below = float(np.nextafter(T(H), T(0)))                                       # the largest T below H
    for (x, y), want in [((1.5, 2.5), 1 + H * 2), ((3.0, 2.0), 3 + H * 2), ((3.0, 2.75), 3 + H * 2), ((1.25, 6.0), 1 + H * 6),
                         ((0.0, 0.0), 0), ((-0.0, 0.5), 0), ((0.5, -0.0), 0), ((-0.0, -0.0), 0),
                         ((below, 0.5), 4), ((0.5, float(np.nextafter(T(W), T(0)))), H * 6), ((below, float(np.nextafter(T(W), T(0)))), H * W - 1),
                         ((-0.25, 1.5), -1), ((1.5, -1.0), -1), ((-1e-30, 1.5), -1), ((-3.0, -3.0), -1),
                         ((5.0, 1.5), -1), ((1.5, 7.0), -1), ((6.5, 1.5), -1), ((1.5, 1e9), -1), ((1e30, 1e30), -1),
                         ((nan, 1.5), -1), ((1.5, nan), -1), ((nan, nan), -1),
                         ((inf, 1.5), -1), ((-inf, 1.5), -1), ((1.5, inf), -1), ((1.5, -inf), -1)]:
        assert both(H, W, 8, 1, x, y, 0, T) == want, (x, y)
    # the floor is taken in T: the Float64 just below 5 is 5 in Float32
    x = float(np.nextafter(np.float64(H), 0.0))
    assert both(H, W, 8, 1, x, 0.5, 0, np.float64) == 4 and both(H, W, 8, 1, x, 0.5, 0, np.float32) == -1


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("nd", [8, 16, 130])
@pytest.mark.parametrize("sectors", [1, 3, 8])
def test_the_sector_is_the_index_scaled_by_integer_division(rcw, T, nd, sectors):
    H, W = 5, 7
    t = 2 + H * 3
    seen = set()
    for d in range(nd):
        c = both(H, W, nd, sectors, 2.5, 3.25, d, T)
        assert c == ((d * sectors) // nd) * H * W + t, d
        seen.add(c // (H * W))
    assert seen == set(range(sectors))                                            # every sector is somebody's
    assert both(H, W, nd, sectors, 2.5, 3.25, nd - 1, T) == (sectors - 1) * H * W + t
    assert both(H, W, nd, sectors, 2.5, 3.25, 0, T) == t
    assert both(H, W, nd, sectors, 9.5, 3.25, nd - 1, T) == -1                    # no cell in any sector


@pytest.mark.parametrize("T", TYPES)
def test_the_export_equals_the_numpy_rule_on_2000_random_poses(rcw, T):
    rng = np.random.default_rng(5)
    n = dict(on=0, off=0)
    for _ in range(2000):
        H, W = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        nd = int(rng.choice([1, 3, 8, 16, 130]))
        sectors = int(rng.integers(1, min(8, nd) + 1))
        x, y = (rng.random(2) * 1.4 - 0.2) * (H, W)
        if rng.random() < 0.3:
            x = float(np.round(x))                                                # exactly on an edge
        c = both(H, W, nd, sectors, x, y, int(rng.integers(0, nd)), T)
        n["on" if c >= 0 else "off"] += 1
        assert -1 <= c < sectors * H * W
    assert n["on"] > 500 and n["off"] > 300, n


def test_refused_arguments(rcw):
    from raycastworlds_jl_amd import _capi, layouts

    lib = _capi.load()
    c = C.c_int32(-7)
    bad = _capi.RCW_ERR_INVALID_ARGUMENT
    assert lib.rcw_visit_cell(5, 5, 8, 1, 1.5, 1.5, 32, 0, C.byref(c)) == _capi.RCW_OK and c.value == 6
    assert lib.rcw_visit_cell(5, 5, 8, 1, 1.5, 1.5, 32, 0, None) == bad
    for H, W, nd, sectors, bits, d in [(0, 5, 8, 1, 32, 0), (5, 0, 8, 1, 32, 0), (-1, 5, 8, 1, 32, 0), (5, -5, 8, 1, 32, 0),
                                       (5, 5, 0, 1, 32, 0), (5, 5, -8, 1, 32, 0),
                                       (5, 5, 8, 0, 32, 0), (5, 5, 8, -1, 32, 0), (5, 5, 8, 9, 32, 0), (5, 5, 130, 9, 32, 0), (5, 5, 4, 5, 32, 0), (5, 5, 1, 2, 32, 0),
                                       (5, 5, 8, 1, 16, 0), (5, 5, 8, 1, 0, 0), (5, 5, 8, 1, 33, 0),
                                       (5, 5, 8, 1, 32, -1), (5, 5, 8, 1, 32, 8), (5, 5, 8, 1, 32, 2 ** 31 - 1),
                                       (16384, 16384, 8, 1, 32, 0), (2 ** 31 - 1, 2 ** 31 - 1, 8, 1, 64, 0), (2 ** 31 - 1, 2, 8, 1, 64, 0)]:
        c.value = -7
        assert lib.rcw_visit_cell(H, W, nd, sectors, 1.5, 1.5, bits, d, C.byref(c)) == bad and c.value == -7, (H, W, nd, sectors, bits, d)
    with pytest.raises(ValueError):
        layouts.visit_cell(5, 5, 8, 9, (1.5, 1.5), 0)
    assert layouts.visit_cell(16384, 16383, 8, 8, (16383.5, 16382.5), 7, np.float64) == 8 * 16384 * 16383 - 1   # the largest map the export takes


# ---- the plan ------------------------------------------------------------------------------------------------------------------------------
WHOLE = SHAPE_FIELDS + ("guide", "frontier", "visit_sectors", "visit_flags")
PARTS = ["visit_map.here", "visit_map.visited", "visit_map.first", "visit_map.level_here", "visit_map.last_episode", "visit_map.map"]


def visit_plan(lib, batch=1, **kw):
    """rcw_dev_visit_plan of the WHOLE shape: dict(names, bytes, archived, offsets, head, total, rows, first, segments, row_bytes, key)"""
    assert not set(kw) - set(WHOLE)
    shape = (C.c_int32 * len(WHOLE))(*[kw.get(f, 0) for f in WHOLE])
    names, sizes, kept, offs = C.create_string_buffer(4096), (C.c_uint32 * 16)(), (C.c_uint8 * 16)(), (C.c_uint64 * 16)()
    head, total, row_bytes, key = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    rows, first, segments = C.c_int32(), C.c_int32(), C.c_int32()
    lib.rcw_dev_visit_plan.argtypes = [C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_char_p, C.c_int32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8),
                                       C.POINTER(C.c_uint64)] + [C.POINTER(C.c_uint64)] * 2 + [C.POINTER(C.c_int32)] * 3 + [C.POINTER(C.c_uint64)] * 2
    n = lib.rcw_dev_visit_plan(shape, len(WHOLE), batch, names, 4096, sizes, kept, offs, C.byref(head), C.byref(total), C.byref(rows), C.byref(first),
                               C.byref(segments), C.byref(row_bytes), C.byref(key))
    assert n >= 0, n
    return dict(names=names.value.decode().split("\n")[:n], bytes=list(sizes[:n]), archived=list(kept[:n]), offsets=list(offs[:n]), head=head.value,
                total=total.value, rows=rows.value, first=first.value, segments=segments.value, row_bytes=row_bytes.value, key=key.value)


def test_a_shape_with_the_feature_off_plans_exactly_what_it_planned(devlib):
    for kw in (ALL_ON, F64_5X5, dict(H=17, W=13, nd=16, N=8, Hc=8, seen=1)):
        before = plan(devlib, **kw)                                               # the 23-word export: the feature cannot be on there
        p = visit_plan(devlib, **kw)
        assert p["names"] == [] and p["head"] == 0 and p["rows"] == 0
        assert (p["segments"], p["row_bytes"], p["key"]) == (len(before[0]), before[1], before[2])
        q = visit_plan(devlib, **dict(kw, guide=1, frontier=1))                   # ... nor do the two that are never archived change it
        assert (q["segments"], q["row_bytes"], q["key"]) == (len(before[0]), before[1], before[2])


@pytest.mark.parametrize("sectors", [1, 3, 8])
def test_every_part_is_archived_and_lies_last_in_the_record(devlib, sectors):
    for kw in (dict(H=5, W=7, nd=8, N=8, Hc=8), ALL_ON, F64_5X5):
        HW = kw["H"] * kw["W"]
        cells = sectors * HW
        before = plan(devlib, **kw)
        p = visit_plan(devlib, batch=67, **dict(kw, visit_sectors=sectors))
        assert p["names"] == PARTS and p["bytes"] == [4, 4, 4, 4, 4, 2 * cells] and all(p["archived"])
        assert p["head"] == 0 and p["rows"] == 0 and p["first"] == 0              # no table without the flag, whatever the source
        # the carve: each part on a multiple of 16 bytes, in list order
        off, want = 0, []
        for b in p["bytes"]:
            want.append(off)
            off = (off + 67 * b + 15) // 16 * 16
        assert p["offsets"] == want and p["total"] == off
        # the record: the six segments behind everything the shape had
        assert p["segments"] == len(before[0]) + 6 and p["row_bytes"] == before[1] + 20 + 2 * cells and p["key"] != before[2]
        keys = {visit_plan(devlib, **dict(kw, visit_sectors=s))["key"] for s in (1, 2, 3, 8)}
        assert len(keys) == 4
        # the table is the head, not a part: the flag changes neither record nor key
        t = visit_plan(devlib, batch=67, **dict(kw, visit_sectors=sectors, visit_flags=1))
        assert (t["segments"], t["row_bytes"], t["key"]) == (p["segments"], p["row_bytes"], p["key"])
        assert t["offsets"] == [o + (t["head"] + 15) // 16 * 16 for o in p["offsets"]]


def test_the_tables_rows_follow_the_statistics_rule_under_the_byte_cap(devlib):
    base = dict(H=5, W=7, nd=8, N=8, Hc=8, visit_sectors=3, visit_flags=1)
    cells = 3 * 35
    for kw, rows, first in [(dict(), 0, 0),
                            (dict(source_kind=BANK, layouts=3), 3, 0),
                            (dict(source_kind=BANK, layouts=65536), 65536, 0),
                            (dict(source_kind=BANK, layouts=65537), 0, 0),            # the statistics' own bound
                            (dict(source_kind=MAZES, levels=5, first_level=3), 5, 3),
                            (dict(source_kind=MAZES, levels=0, first_level=3), 0, 0),
                            (dict(source_kind=3, levels=7, first_level=-2), 7, -2),
                            (dict(source_kind=4, levels=2, first_level=2 ** 31 - 2), 2, 2 ** 31 - 2)]:
        p = visit_plan(devlib, **dict(base, **kw))
        assert (p["rows"], p["first"]) == (rows, first), kw
        assert p["head"] == 4 * cells * (1 + rows)
    # the cap: 8 sectors of 64 x 64 are 131,072 bytes a row — 2,047 level rows fit in 256 MiB beside row 0, 2,048 do not
    big = dict(H=64, W=64, nd=8, N=8, Hc=8, visit_sectors=8, visit_flags=1, source_kind=BANK)
    assert 4 * 8 * 64 * 64 * 2048 == CAP
    p = visit_plan(devlib, **dict(big, layouts=2047))
    assert p["rows"] == 2047 and p["head"] == CAP
    p = visit_plan(devlib, **dict(big, layouts=2048))
    assert p["rows"] == 0 and p["first"] == 0 and p["head"] == 4 * 8 * 64 * 64                         # not an error: row 0 always works
    p = visit_plan(devlib, **dict(big, source_kind=MAZES, layouts=0, levels=65536, first_level=9))
    assert p["rows"] == 0 and p["first"] == 0                                                           # (4 * cells * 65537 passes 32 bits)
    # refused shapes of the export itself
    assert devlib.rcw_dev_visit_plan(None, len(WHOLE), 1, None, 0, None, None, None, None, None, None, None, None, None, None) < 0
    shape = (C.c_int32 * len(WHOLE))(*([5, 5, 8, 8, 8] + [0] * (len(WHOLE) - 5)))
    names = C.create_string_buffer(64)
    assert devlib.rcw_dev_visit_plan(shape, len(WHOLE) - 1, 1, names, 64, None, None, None, None, None, None, None, None, None, None) < 0


# ---- the sanitizers ----------------------------------------------------------------------------------------------------------------------
def test_the_rules_under_asan_and_ubsan_as_a_program_of_their_own(tmp_path):
    """tests/san_visit_main.cpp with csrc/rcw_rules.hip in one translation unit, host side only, under -fsanitize=address,undefined:
    rcw_visit_cell and the plan on hostile inputs.  A stand-alone program on the CPU: no sanitizer's runtime is loaded into Python."""
    import shutil
    import subprocess

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "san_visit")
    build = subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
                            "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-o", exe,
                            os.path.join(ROOT, "tests", "san_visit_main.cpp")], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    assert run.returncode == 0 and "san_visit_main: ok" in run.stdout, run.stdout[-2000:] + run.stderr[-3000:]
    assert "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
