"""The learner view's depth plane on the CPU (include/rcw.h "the learner view"): cases worked by hand, the two numpy readings of the
contract (tests/learner_view_depth_ref.py: pixel by pixel, and by counting rows per column) against each other on hand-made descriptors
and on the oracle's, the three constants in the header and the bindings, and a rehearsal of the GPU tests' rollouts on the oracle alone."""
import os
import re

import numpy as np
import pytest

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
