"""The learner view's pixel contract on the CPU (include/rcw.h "the learner view"): hand-derived cases, the two numpy readings of it
(tests/learner_view_ref.py: from the UInt32 frames, from the column descriptors) against each other on the oracle's frames, and
the declarations and bindings of its five exports."""
import os
import re

import numpy as np
import pytest

import learner_view_ref as LV
from helpers import CFG1, CFG2, CFG3, CFG4, CFG5, REFERENCE_DEFAULT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("rcw_set_learner_view", "rcw_learner_view_info", "rcw_learner_view_device_ptr", "rcw_learner_view_copy",
           "rcw_expand_columns_view")
CONSTANTS = {"RCW_VIEW_OFF": 0, "RCW_VIEW_RGB8": 1, "RCW_VIEW_GRAY8": 2, "RCW_VIEW_CHW": 0, "RCW_VIEW_HWC": 1, "RCW_VIEW_ONLY": 1}
REF_COLOURS = dict(ceiling_color=0x00FFFFFF, floor_color=0x00404040, wall_dim_1_color=0x00808080, wall_dim_2_color=0x00C0C0C0,
                   goal_dim_1_color=0x00800000, goal_dim_2_color=0x00C00000)


def test_an_uneven_five_to_two_box_by_hand():
    # one column of 5 rows, values 0, 10, 20, 30, 41 in blue: rows [0, 2) and [2, 5)
    frame = np.array([[0, 10, 20, 30, 41]], dtype=np.uint32)[None]            # (B, N, H) = (1, 1, 5)
    out = LV.from_frames(frame, "rgb", (2, 1))
    assert out.shape == (1, 3, 2, 1)
    assert out[0, 2, :, 0].tolist() == [5, 30]                                 # (0 + 10 + 1) // 2, (20 + 30 + 41 + 1) // 3
    assert out[0, 0].sum() == 0 and out[0, 1].sum() == 0
    assert LV.row_bounds(5, 2).tolist() == [0, 2, 5]


def test_an_exact_half_rounds_up():
    frame = np.array([[[0, 1]]], dtype=np.uint32)                              # blue 0 and 1 in one 2-row box: 0.5 -> 1
    assert LV.from_frames(frame, "rgb", (1, 1))[0, 2, 0, 0] == 1
    frame = np.array([[[2, 5]]], dtype=np.uint32)                              # 3.5 -> 4
    assert LV.from_frames(frame, "rgb", (1, 1), layout="hwc")[0, 0, 0, 2] == 4


def test_the_gray_values_of_the_reference_palette():
    vals = [int(LV.gray_of(REF_COLOURS[k])) for k in ("ceiling_color", "floor_color", "wall_dim_1_color", "wall_dim_2_color",
                                                       "goal_dim_1_color", "goal_dim_2_color")]
    assert vals == [255, 64, 128, 192, 39, 58]


def test_full_size_rgb_is_the_frame_transposed_and_unpacked():
    from raycastworlds_jl_amd.viewer import frame_to_rgb

    rng = np.random.default_rng(1)
    frames = rng.integers(0, 2 ** 32, (2, 7, 5), dtype=np.uint64).astype(np.uint32)
    chw = LV.from_frames(frames, "rgb", (5, 7))
    hwc = LV.from_frames(frames, "rgb", (5, 7), layout="hwc")
    for b in range(2):
        np.testing.assert_array_equal(hwc[b], frame_to_rgb(frames[b]))
        np.testing.assert_array_equal(chw[b], frame_to_rgb(frames[b]).transpose(2, 0, 1))
    g = LV.from_frames(frames, "gray", (5, 7))
    np.testing.assert_array_equal(g[:, 0], LV.gray_of(frames.transpose(0, 2, 1)))
    np.testing.assert_array_equal(g, LV.from_frames(frames, "gray", (5, 7), layout="hwc").transpose(0, 3, 1, 2))


def test_descriptors_at_the_edges_of_the_column_rule():
    H = 9
    cfg = dict(REF_COLOURS)
    hl = np.array([[0, 1, H - 2, H - 1, H, 2 ** 31 - 1, -(2 ** 31), 4]], dtype=np.int64)
    cid = np.array([[0, 1, 2, 3, 0, 1, 2, 3]], dtype=np.uint8)
    frames = np.empty((1, hl.shape[1], H), dtype=np.uint32)
    for k in range(hl.shape[1]):                                               # pixel(): rows < pad ceiling, < H - pad colour, floor
        pad = int(LV.padding(H, hl[0, k]))
        colour = [cfg["wall_dim_1_color"], cfg["wall_dim_2_color"], cfg["goal_dim_1_color"], cfg["goal_dim_2_color"]][cid[0, k]]
        frames[0, k] = [cfg["ceiling_color"] if y < pad else (colour if y < H - pad else cfg["floor_color"]) for y in range(H)]
    for fmt in ("rgb", "gray"):
        for size in ((H, 8), (1, 1), (4, 3), (H, 1), (2, 8)):
            for layout in ("chw", "hwc"):
                np.testing.assert_array_equal(LV.from_descriptors(hl, cid, cfg, H, fmt, size, layout),
                                              LV.from_frames(frames, fmt, size, layout), err_msg=f"{fmt} {size} {layout}")


@pytest.mark.parametrize("name,cfg", [("cfg1", CFG1), ("cfg2", CFG2), ("cfg3", CFG3), ("cfg4", CFG4), ("cfg5", CFG5),
                                      ("reference_default", REFERENCE_DEFAULT)])
def test_frames_and_descriptors_agree_on_the_oracle(oracle, name, cfg):
    orc = oracle.OracleBatch(3, seed=11, **cfg)
    rng = np.random.default_rng(5)
    for _ in range(4):
        orc.step(rng.integers(1, 5, 3).astype(np.uint8))
    frames, H, N = orc.camera_view.copy(), orc.Hc, orc.N
    sizes = [(1, 1), (H, 1), (1, N), (37, 53), (84, 84), (H, N), (H // 2, N // 3)]
    for fmt in ("rgb", "gray"):
        for size in sizes:
            size = (min(size[0], H), min(size[1], N))
            layout = "hwc" if size[0] % 2 else "chw"
            np.testing.assert_array_equal(LV.from_descriptors(orc.col_height, orc.col_colour, orc.cfg, H, fmt, size, layout),
                                          LV.from_frames(frames, fmt, size, layout), err_msg=f"{name} {fmt} {size}")
    orc.close()


def test_the_header_declares_the_exports_and_the_constants():
    text = open(os.path.join(ROOT, "include", "rcw.h")).read()
    for name in EXPORTS:
        assert re.search(r"RCW_API\s+int\s+" + name + r"\s*\(", text), name
    for name, value in CONSTANTS.items():
        m = re.search(r"#define\s+" + name + r"\s+(\d+)", text)
        assert m and int(m.group(1)) == value, name
    assert re.search(r"#define\s+RCW_ABI_VERSION\s+4\b", text)


def test_the_python_and_julia_bindings_carry_them(rcw):
    from raycastworlds_jl_amd import _capi

    for name in EXPORTS:
        assert name in _capi.SIGNATURES, name
    for name, value in CONSTANTS.items():
        assert getattr(_capi, name) == value, name
    jl = open(os.path.join(ROOT, "julia", "BatchedSingleRoom.jl")).read()
    for name in EXPORTS:
        assert re.search(r"ccall\(\(:" + name + r",\s*librcw\)", jl), name
    assert "function set_learner_view!" in jl and "function learner_view(" in jl
    lib = _capi.load()
    for name in EXPORTS:
        assert hasattr(lib, name), name
    for name in ("set_learner_view", "learner_view_host", "expand_columns_view"):
        assert callable(getattr(rcw.SingleRoomModule.SingleRoom, name)), name
