"""The learner view's depth plane on the CPU (include/rcw.h "the learner view"): cases worked by hand, the two numpy readings of the
contract (tests/learner_view_depth_ref.py: pixel by pixel, and by counting rows per column) against each other on hand-made descriptors
and on the oracle's, the three constants in the header and the bindings, a rehearsal of the GPU tests' rollouts on the oracle alone, and the
hand-made descriptors of tests/learner_view_depth_cases.py: what each builder holds, and both readings on every case the GPU renders."""
import os
import re

import numpy as np
import pytest

import learner_view_depth_cases as K
import learner_view_depth_ref as LD
import learner_view_depth_rollout as G
import learner_view_ref as LV
from helpers import CFG1, CFG2, CFG3, CFG4, CFG5, REFERENCE_DEFAULT
from test_learner_view_spec import REF_COLOURS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONSTANTS = {"RCW_VIEW_DEPTH8": 4, "RCW_VIEW_RGBD8": 5, "RCW_VIEW_GRAYD8": 6}
FORMATS = ("depth", "rgbd", "grayd")


def test_a_column_of_eight_rows_by_hand():
    # Hc = 8, hl = 4: pad = 2; rows 0, 1, 6, 7 are ceiling / floor with u = 8, 6, 6, 8, rows 2 .. 5 the wall with u = 4
    # D = (255 u + 4) // 8: 2044 // 8 = 255, 1534 // 8 = 191, 1024 // 8 = 128
    hl = np.array([[4]])
    assert int(LV.padding(8, 4)) == 2
    rows = [255, 191, 128, 128, 128, 128, 191, 255]
    assert LD.depth_frames(hl, 8)[0, :, 0].tolist() == rows
    assert LD.from_descriptors(hl, 8, (8, 1))[0, :, 0].tolist() == rows
    # size (2, 1): rows [0, 4) and [4, 8), each 255 + 191 + 128 + 128 = 702 over 4 pixels
    assert sum(rows[:4]) == sum(rows[4:]) == 702
    assert LD.from_descriptors(hl, 8, (2, 1))[0, :, 0].tolist() == [(702 + 2) // 4] * 2 == [176, 176]
    assert LD.by_frames(hl, 8, (2, 1))[0, :, 0].tolist() == [176, 176]
    # one pixel: 1404 over 8
    assert LD.from_descriptors(hl, 8, (1, 1))[0, 0, 0] == LD.by_frames(hl, 8, (1, 1))[0, 0, 0] == (1404 + 4) // 8 == 176


def test_a_column_of_nine_rows_by_hand():
    # Hc = 9, hl = 4: pad = (9 - 4) // 2 = 2, the wall on rows [2, 7), floor from max(2, 7) = 7; Hc // 2 = 4
    # ceiling / floor rows 0, 1, 7, 8: u = 9, 7, 7, 9 -> (2295 + 4) // 9 = 255, (1785 + 4) // 9 = 198; wall u = 4 -> (1020 + 4) // 9 = 113
    hl = np.array([[4]])
    assert int(LV.padding(9, 4)) == 2
    rows = [255, 198, 113, 113, 113, 113, 113, 198, 255]
    assert LD.depth_frames(hl, 9)[0, :, 0].tolist() == rows
    assert LD.from_descriptors(hl, 9, (9, 1))[0, :, 0].tolist() == rows
    # size (2, 1): rows [0, 4) = 255 + 198 + 113 + 113 = 679 over 4, rows [4, 9) = 113 * 3 + 198 + 255 = 792 over 5
    want = [(679 + 2) // 4, (792 + 2) // 5]
    assert want == [170, 158]
    assert LD.from_descriptors(hl, 9, (2, 1))[0, :, 0].tolist() == want
    assert LD.by_frames(hl, 9, (2, 1))[0, :, 0].tolist() == want
    # the middle row of an odd column is its own mirror: u = 9 - 2 * 4 = 1 where it is ceiling (hl far below zero: pad = Hc)
    far = np.array([[-100]])
    assert int(LV.padding(9, -100)) == 9
    assert LD.depth_frames(far, 9)[0, :, 0].tolist() == [(255 * u + 4) // 9 for u in (9, 7, 5, 3, 1, 3, 5, 7, 9)]
    assert LD.from_descriptors(far, 9, (9, 1))[0, :, 0].tolist() == LD.depth_frames(far, 9)[0, :, 0].tolist()


def test_descriptors_at_the_edges_of_the_column_rule():
    H = 9
    cfg = dict(REF_COLOURS)
    hl = np.array([[0, 1, H - 2, H - 1, H, 2 ** 31 - 1, -(2 ** 31), 4]], dtype=np.int64)
    cid = np.array([[0, 1, 2, 3, 0, 1, 2, 3]], dtype=np.uint8)
    full = LD.depth_frames(hl, H)[0]                                           # (H, 8)
    pad = LV.padding(H, hl[0])
    assert pad.tolist() == [4, 4, 1, 0, 0, 0, 9, 2]
    for k in range(8):
        if pad[k] <= H // 2:
            assert full[:, k].tolist() == full[::-1, k].tolist(), k            # D(y) = D(Hc - 1 - y)
        if pad[k] == 0:
            assert len(set(full[:, k].tolist())) == 1, k                        # a wall that fills the column: one value
    assert full[:, 3].tolist() == [(255 * 8 + 4) // 9] * 9 and full[:, 4].tolist() == [255] * 9 and full[:, 5].tolist() == [255] * 9
    for fmt in FORMATS:
        for size in ((H, 8), (1, 1), (4, 3), (H, 1), (2, 8)):
            for layout in ("chw", "hwc"):
                a = LD.view(hl, cid, cfg, H, fmt, size, layout)
                b = LD.view(hl, cid, cfg, H, fmt, size, layout, depth=LD.by_frames)
                np.testing.assert_array_equal(a, b, err_msg=f"{fmt} {size} {layout}")
                c = LD.CHANNELS[fmt]
                assert a.shape == ((1, c) + size if layout == "chw" else (1,) + size + (c,))
                if fmt != "depth":                                              # the colour planes are the colour view, byte for byte
                    colour = LV.from_descriptors(hl, cid, cfg, H, LD.COLOUR_OF[fmt], size, layout)
                    np.testing.assert_array_equal(a[:, :c - 1] if layout == "chw" else a[..., :c - 1], colour)
    np.testing.assert_array_equal(LD.view(hl, cid, cfg, H, "depth", (4, 3), "chw").ravel(), LD.view(hl, cid, cfg, H, "depth", (4, 3), "hwc").ravel())


@pytest.mark.parametrize("name,cfg", [("cfg1", CFG1), ("cfg2", CFG2), ("cfg3", CFG3), ("cfg4", CFG4), ("cfg5", CFG5),
                                      ("reference_default", REFERENCE_DEFAULT)])
def test_the_two_readings_agree_on_the_oracle(oracle, name, cfg):
    orc = oracle.OracleBatch(3, seed=11, **cfg)
    rng = np.random.default_rng(5)
    for _ in range(4):
        orc.step(rng.integers(1, 5, 3).astype(np.uint8))
    frames, H, N = orc.camera_view.copy(), orc.Hc, orc.N
    D = LD.depth_frames(orc.col_height, H)
    sizes = [(1, 1), (H, 1), (1, N), (37, 53), (84, 84), (H, N), (H // 2, N // 3)]
    for size in sizes:
        size = (min(size[0], H), min(size[1], N))
        layout = "hwc" if size[0] % 2 else "chw"
        np.testing.assert_array_equal(LD.from_descriptors(orc.col_height, H, size), LD.from_depth_frames(D, size), err_msg=f"{name} {size}")
        for fmt in ("rgbd", "grayd"):
            v = LD.view(orc.col_height, orc.col_colour, orc.cfg, H, fmt, size, layout)
            c = LD.CHANNELS[fmt]
            np.testing.assert_array_equal(v[:, :c - 1] if layout == "chw" else v[..., :c - 1],
                                          LV.from_frames(frames, LD.COLOUR_OF[fmt], size, layout), err_msg=f"{name} {fmt} {size}")
            np.testing.assert_array_equal(v[:, c - 1] if layout == "chw" else v[..., c - 1], LD.from_depth_frames(D, size))
    orc.close()


def test_the_header_and_the_bindings_carry_the_constants():
    from raycastworlds_jl_amd import _capi

    text = open(os.path.join(ROOT, "include", "rcw.h")).read()
    jl = open(os.path.join(ROOT, "julia", "BatchedSingleRoom.jl")).read()
    for name, value in CONSTANTS.items():
        m = re.search(r"#define\s+" + name + r"\s+(\d+)", text)
        assert m and int(m.group(1)) == value, name
        assert getattr(_capi, name) == value, name
        m = re.search(r"const\s+" + name + r"\s*=\s*Int32\((\d+)\)", jl)
        assert m and int(m.group(1)) == value, name
    assert re.search(r"#define\s+RCW_ABI_VERSION\s+4\b", text)
    for sym in (":depth", ":rgbd", ":grayd"):
        assert sym in jl, sym
    assert _capi.RCW_VIEW_RGBD8 == _capi.RCW_VIEW_RGB8 | _capi.RCW_VIEW_DEPTH8 and _capi.RCW_VIEW_GRAYD8 == _capi.RCW_VIEW_GRAY8 | _capi.RCW_VIEW_DEPTH8


@pytest.mark.parametrize("name", sorted(G.ROLLOUTS))
def test_rehearsal_of_the_gpu_rollouts(oracle, name):
    """every rollout of tests/test_gpu_learner_view_depth.py (tests/learner_view_depth_rollout.py), its seeds and actions, on the oracle alone: the descriptors it compares hold a
    column a wall fills (pad = 0), a column with ceiling and floor (pad > 0) and at least 8 distinct D among wall pixels"""
    d = G.DepthRollout(None, oracle, name).run()
    Hc = d.orc.Hc
    hl = np.concatenate(d.seen).astype(np.int64)
    assert len(d.seen) == 9                                                     # the view set, 4 steps, the masked reset, 3 steps
    pad = LV.padding(Hc, hl)
    assert (pad == 0).any(), "no column a wall fills"
    assert (pad > 0).any(), "no column with ceiling and floor"
    wall = pad < Hc - pad                                                       # columns with at least one wall pixel
    values = np.unique(LD.depth_byte(np.clip(hl[wall], 0, Hc), Hc))
    assert len(values) >= 8, values.tolist()
    d.close()


# ---- the hand-made descriptors of tests/test_gpu_learner_view_depth_descriptors.py (tests/learner_view_depth_cases.py) ------------------
PARENT_ROLLOUTS = ("cfg1", "odd", "many rays", "depth table", "huge box", "cfg2 near the goal", "cfg1 near the goal",
                   "many rays near the goal", "cfg2", "cfg2 x 64")
LIMITS = (K.largest_agent_Hc(K.LIMIT_RAYS, (1, 1)), K.largest_agent_Hc(K.LIMIT_RAYS, (1, 1)) + 1, K.FULL_KERNEL_LAST, K.FULL_KERNEL_LAST + 1,
          K.CREATE_LIMIT)


def test_the_rollouts_never_reach_a_height_at_or_below_zero(oracle):
    """why the hand-made descriptors exist: over every rollout the depth plane had before them, height_line_pu stays above zero — max(hl, 0),
    u = 0 and pad > Hc / 2 are out of a rollout's reach in the 8 x 8 room.  Should a later rollout change this, it fails here."""
    assert set(PARENT_ROLLOUTS) <= set(G.ROLLOUTS) and set(G.ROLLOUTS) - set(PARENT_ROLLOUTS) == {"cfg1 x 1100"}
    for name in PARENT_ROLLOUTS:
        d = G.DepthRollout(None, oracle, name).run()
        hl = np.concatenate(d.seen).astype(np.int64)
        assert hl.min() > 0, (name, int(hl.min()))
        assert not (2 * LV.padding(d.orc.Hc, hl) > d.orc.Hc).any(), name
        d.close()


@pytest.mark.parametrize("Hc,N", [(1021, 16), (257, 256), (37, 33), (16, 5600), (1500, 5000), (2048, 4096), (9, 4)])
def test_every_u_holds_what_it_claims(Hc, N):
    hl, cid = K.every_u(Hc, N)
    values = list(range(-2, Hc + 3)) + [2 ** 31 - 1, -(2 ** 31), 2 ** 30, -(2 ** 30), -Hc - 1, -Hc, -Hc + 1, 2 * Hc]
    n = -(-len(values) // N)
    assert hl.shape == cid.shape == (n, N) and hl.dtype == np.int32 and cid.dtype == np.uint8
    flat = hl.ravel().astype(np.int64)
    assert flat[:len(values)].tolist() == values
    assert flat[len(values):].tolist() == [values[i % len(values)] for i in range(len(values), n * N)]     # the tail repeats from the start
    assert set(range(-2, Hc + 3)) <= set(flat.tolist())
    assert cid[0, :4].tolist() == [0, 1, 2, 3] and (n == 1 or cid[1, :4].tolist() == [1, 2, 3, 0]) and cid.max() == 3
    held = K.holds(hl, Hc)
    assert held == {"hl < 0": True, "u == 0": True, "pad == Hc": True, "pad > Hc / 2": True, "pad == 0 with u == Hc - 1": True,
                    "distinct u": Hc + 1}


def test_a_height_below_zero_has_no_colour_row():
    """What the lower clamp of u = min(max(hl, 0), Hc) can show: nothing.  hl < 0 gives pad = min((Hc - hl) // 2, Hc) >= (Hc + 1) // 2, so
    Hc - pad <= pad and the column has no colour row for Dw to appear on; u = 0 is seen on one row alone, the middle one of an odd column of
    hl = 0.  (A kernel without the max() renders the same bytes: DESIGN.md 4.6.)  A padding that wrapped at hl = INT_MIN would show on that
    row only where depth_byte(1) > 0, i.e. at an odd Hc below 510: the 256 x 257 case of K.EVERY_U."""
    for Hc in (9, 16, 37, 256, 257, 1021, 2048, 32767, 2 ** 20):
        hl = np.concatenate([np.arange(-2 * Hc - 3, 1), [-(2 ** 31), -(2 ** 30)]]).astype(np.int64)
        pad = LV.padding(Hc, hl)
        rows = np.maximum(0, (Hc - pad) - pad)                                   # colour rows of each column
        assert (rows[hl < 0] == 0).all() and rows[hl == 0].tolist() == [Hc % 2]
    assert int(LD.depth_byte(1, 257)) == 1 and int(LD.depth_byte(1, 1021)) == 0 and K.SWEEP["height_camera_view_pu"] == 257
    assert [Hc for Hc in range(1, 4096, 2) if int(LD.depth_byte(1, Hc)) > 0][-1] == 509
    mid = LD.depth_frames(np.array([[-(2 ** 31), 0]]), 257)[0, 128]
    assert mid.tolist() == [1, 0]                                                # De(128) on the padded column, Dw = D(0) on the wall's one row


@pytest.mark.parametrize("Hc", LIMITS + (255, 256, 1021))
def test_thresholds_holds_both_sides_of_255_steps(Hc):
    assert LIMITS == (16331, 16332, 32767, 32768, 2 ** 20)
    values = K.threshold_values(Hc)
    assert len(values) == 510
    D = LD.depth_byte(np.array(values), Hc)
    assert D[0::2].tolist() == list(range(1, 256)) and D[1::2].tolist() == list(range(0, 255))
    for d, u in zip(range(1, 256), values[0::2]):                               # the smallest u of its D: a search, not the formula
        assert u == next(x for x in range(max(0, u - 3), Hc + 1) if (255 * x + Hc // 2) // Hc == d)
    hl, cid = K.thresholds(Hc, 16)
    assert hl.shape == (33, 16) and hl.ravel()[:510].tolist() == values
    assert hl.ravel()[510:520].tolist() == [0, 1, Hc - 2, Hc - 1, Hc, Hc + 1, -1, -Hc, -(2 ** 31), 2 ** 31 - 1]
    held = K.holds(hl, Hc)
    assert all(held[k] for k in ("hl < 0", "u == 0", "pad == Hc", "pad > Hc / 2", "pad == 0 with u == Hc - 1"))


def test_random_rows_are_pairwise_different():
    """the descriptor sets of the sweep and the alignment tests, at an MI355X's 256 CUs and at a quarter of them"""
    for cus in (256, 64):
        for CT in (1, 2, 4):
            n = K.sweep_rows(CT, cus)
            assert n * CT * 3 >= 10 * cus > (n - 1) * CT * 3
            hl, cid = K.random_rows(n, 257, 256, seed=CT)
            assert hl.shape == cid.shape == (n, 256) and len({r.tobytes() for r in hl}) == n
            assert hl.min() >= -257 and hl.max() <= 514 and (hl == -257).any() and (hl == 514).any() and cid.max() == 3
            assert n * CT * 257 * 256 < 128 << 20
    assert K.full_kernel_blocks(256, 257) == (3, 128) and 257 - 2 * 128 == 1     # three row blocks a plane, the last of one row
    hl, _ = K.random_rows(3, 256, 64, seed=3)
    assert len({r.tobytes() for r in hl}) == 3


@pytest.mark.parametrize("name", sorted(K.EVERY_U))
def test_the_two_readings_agree_on_every_u(name):
    cfg, sizes = K.EVERY_U[name]
    Hc, N = cfg.get("height_camera_view_pu", 256), cfg["num_rays"]
    hl, cid = K.every_u(Hc, N)
    frames = LD.depth_frames(hl, Hc)
    colours = dict(REF_COLOURS)
    for size, formats in sizes:
        size = size or (Hc, N)
        count = LD.from_descriptors(hl, Hc, size)
        msg = K.first_difference(LD.from_depth_frames(frames, size)[:, None], count[:, None], hl, Hc, size, "chw", name)
        assert msg is None, msg
        for fmt, layout in formats:                                             # view() is these planes, and at full size full_size() is view()
            v = LD.view(hl, cid, colours, Hc, fmt, size, layout)
            np.testing.assert_array_equal(v[:, -1] if layout == "chw" else v[..., -1], count)
            if size == (Hc, N):
                np.testing.assert_array_equal(LD.full_size(hl, cid, colours, Hc, fmt, layout), v)


@pytest.mark.parametrize("Hc", LIMITS)
def test_the_two_readings_agree_at_the_limits_of_Hc(Hc):
    """thresholds at the heights of the GPU test; at 2^20 the pixel reading takes one descriptor row (it walks 16 columns of a million rows
    each).  The middle row of the (255, 16) view is the wall's byte itself."""
    hl, cid = K.thresholds(Hc, K.LIMIT_RAYS)
    part = hl[:1] if Hc == K.CREATE_LIMIT else hl
    sizes = K.LIMIT_SIZES + (((Hc, K.LIMIT_RAYS),) if Hc == K.FULL_KERNEL_LAST else ())
    frames = LD.depth_frames(part, Hc)
    for size in sizes:
        count = K.view_in_chunks(hl, cid, dict(REF_COLOURS), Hc, "depth", size, rows=8)[:, 0]
        msg = K.first_difference(LD.from_depth_frames(frames, size)[:, None], count[:len(part), None], part, Hc, size, "chw", f"Hc = {Hc}")
        assert msg is None, msg
        if size == (255, 16):
            columns, D = K.middle_row(hl, Hc)
            assert columns.sum() >= 2 * 254 and set(range(1, 256)) <= set(D[columns].tolist())     # both sides of every step from D = 2 up
            np.testing.assert_array_equal(count[:, 127, :][columns], D[columns])


def test_full_size_is_view_on_the_oracle(oracle):
    orc = oracle.OracleBatch(4, seed=3, **CFG1)
    rng = np.random.default_rng(2)
    for _ in range(3):
        orc.step(rng.integers(1, 5, 4).astype(np.uint8))
    hl = orc.col_height.astype(np.int64)
    hl[0, :8] = [0, 1, -1, orc.Hc - 2, orc.Hc - 1, orc.Hc, -orc.Hc, 2 ** 31 - 1]
    for fmt in ("rgb", "gray") + FORMATS:
        for layout in ("chw", "hwc"):
            np.testing.assert_array_equal(LD.full_size(hl, orc.col_colour, orc.cfg, orc.Hc, fmt, layout),
                                          LD.view(hl, orc.col_colour, orc.cfg, orc.Hc, fmt, (orc.Hc, orc.N), layout), err_msg=f"{fmt} {layout}")
    orc.close()
