"""The learner view's k-frame stack on the CPU (include/rcw.h "the frame stack"): the declarations and bindings of its two exports, and
the numpy model of it (tests/learner_view_stack_ref.py) against a brute-force restatement over an oracle rollout in which every agent
restarts under auto_reset."""
import os
import re

import numpy as np
import pytest

import learner_view_ref as LV
import learner_view_stack_ref as LS
from helpers import CFG2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("rcw_set_learner_view_stack", "rcw_learner_view_stack")


def near_the_goal(oracle, batch):
    """the rollout of tests/test_gpu_unchanged_skip.py's rollout_episodes on the oracle alone: the 8 x 8 room, every agent four forward
    moves from its goal, auto_reset, then steps that are forward with probability 0.7"""
    from test_gpu_unchanged_skip import Rollout

    r = Rollout(None, oracle, batch, 3, 8, auto_reset=True, out_of_bounds=1, **CFG2)
    r.set_state_near_the_goal()
    return r


def draw_actions(rng, batch, p_forward=0.7):
    a = rng.integers(1, 5, batch).astype(np.uint8)
    return np.where(rng.random(batch) < p_forward, 1, a).astype(np.uint8)


def test_the_header_the_bindings_and_the_library_carry_the_two_exports(rcw):
    from raycastworlds_jl_amd import _capi

    text = open(os.path.join(ROOT, "include", "rcw.h")).read()
    assert re.search(r"RCW_API\s+int\s+rcw_set_learner_view_stack\s*\(\s*rcw_handle\*\s*h\s*,(\s*int32_t\s+\w+\s*,){5}\s*int32_t\s+frames\s*\)", text)
    assert re.search(r"RCW_API\s+int\s+rcw_learner_view_stack\s*\(\s*rcw_handle\*\s*h\s*,\s*int32_t\*\s*frames\s*\)", text)
    m = re.search(r"#define\s+RCW_VIEW_MAX_FRAMES\s+(\d+)", text)
    assert m and int(m.group(1)) == 16 == _capi.RCW_VIEW_MAX_FRAMES
    assert re.search(r"#define\s+RCW_ABI_VERSION\s+4\b", text)                 # additive: the version stays
    jl = open(os.path.join(ROOT, "julia", "BatchedSingleRoom.jl")).read()
    lib = _capi.load()
    for name in EXPORTS:
        assert name in _capi.SIGNATURES, name
        assert re.search(r"ccall\(\(:" + name + r",\s*librcw\)", jl), name
        assert hasattr(lib, name), name
    assert len(_capi.SIGNATURES["rcw_set_learner_view_stack"]) == 7 and len(_capi.SIGNATURES["rcw_learner_view_stack"]) == 2
    assert re.search(r"function set_learner_view!\(env::BatchedSingleRoom;[^\n]*(\n +[^\n]*){0,3}\bstack::Integer = 1\)\n", jl)
    assert isinstance(rcw.SingleRoomModule.SingleRoom.learner_view_stack, property)


def test_the_model_by_hand():
    v = lambda *x: np.array(x, np.uint8).reshape(len(x), 1, 1, 1)
    m = LS.StackModel(3, v(1, 2), [0, 0])
    assert m.stack[:, :, 0, 0].tolist() == [[1, 1, 1], [2, 2, 2]]
    assert not m.push(v(3, 4), [0, 0]).any()
    assert m.stack[:, :, 0, 0].tolist() == [[1, 1, 3], [2, 2, 4]]
    assert m.push(v(5, 6), [0, 1]).tolist() == [False, True]                   # agent 1 was re-sampled in this step
    assert m.stack[:, :, 0, 0].tolist() == [[1, 3, 5], [6, 6, 6]]
    m.push(v(7, 8), [0, 1])
    assert m.stack[:, :, 0, 0].tolist() == [[3, 5, 7], [6, 6, 8]]
    m.refill(v(9, 10), mask=[1, 0], episode=[0, 0])                            # a masked reset with a seed: counter 0, as before — the mask decides
    assert m.stack[:, :, 0, 0].tolist() == [[9, 9, 9], [6, 6, 8]]
    assert m.episode.tolist() == [0, 1]                                        # (the untouched agent keeps its recorded counter too)
    m.push(v(11, 12), [0, 1])
    assert m.stack[:, :, 0, 0].tolist() == [[9, 9, 11], [6, 8, 12]]
    rgb = LS.StackModel(2, np.arange(6, dtype=np.uint8).reshape(1, 3, 1, 2), [4])
    rgb.push(np.arange(6, 12, dtype=np.uint8).reshape(1, 3, 1, 2), [4])
    assert rgb.stack.shape == (1, 6, 1, 2) and rgb.stack.ravel().tolist() == list(range(12))   # channel s C + c: slot s, channel c


@pytest.mark.parametrize("k,fmt,size", [(4, "gray", (84, 84)), (3, "rgb", (37, 53)), (1, "gray", (20, 20)), (16, "gray", (5, 7))])
def test_the_model_against_the_brute_force_restatement(oracle, k, fmt, size):
    B = 64
    r = near_the_goal(oracle, B)
    orc = r.orc
    views = [LV.from_frames(orc.camera_view, fmt, size)]
    model = LS.StackModel(k, views[0], orc.episode)
    first = [np.zeros(B, np.int64)]
    restarts = np.zeros(B, np.int64)
    quiet = 0
    for t in range(1, 25):
        ep = orc.episode.copy()
        assert orc.step(draw_actions(r.rng, B)) == 0
        moved = orc.episode != ep
        restarts += (orc.episode - ep).astype(np.int64)
        first.append(np.where(moved, t, first[-1]))
        quiet += int((t - first[-1] >= 3).sum())                               # all four slots of a k = 4 stack are different steps' frames
        views.append(LV.from_frames(orc.camera_view, fmt, size))
        np.testing.assert_array_equal(model.push(views[-1], orc.episode), moved)
        want = LS.brute_force(views, first, k)
        assert model.stack.shape == want.shape == (B, k * views[0].shape[1]) + size
        np.testing.assert_array_equal(model.stack, want, err_msg=f"step {t}")
        if k == 1:
            np.testing.assert_array_equal(model.stack, views[-1])
    # from the oracle's own counters: the rollout restarts every agent, and most agent-steps shift a full stack
    assert restarts.sum() >= B and (restarts >= 1).all(), (int(restarts.sum()), int((restarts >= 1).sum()))
    assert quiet >= B, quiet
    orc.close()
