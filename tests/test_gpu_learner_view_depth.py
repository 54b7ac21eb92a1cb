"""The learner view's depth plane on the GPU (include/rcw.h "the learner view": RCW_VIEW_DEPTH8 / RGBD8 / GRAYD8): every byte of the view
against the numpy restatement (tests/learner_view_depth_ref.py, with tests/learner_view_ref.py for the colour planes) over the CPU
oracle's column descriptors, after every call of a short rollout — set the view, four steps under auto_reset, a masked reset (the agents
outside the mask keep every byte), three more steps.  The engine's own descriptors (env.columns()) are compared with the oracle's at each
of those points as well.  The shapes are the smallest that reach each kernel of rcw_view.hip and each rule of its launchers.

The rollouts are tests/learner_view_depth_rollout.py's; tests/test_learner_view_depth_spec.py runs every one of them on the oracle alone and asserts that its descriptors
hold a column a wall fills (pad = 0), a column with ceiling and floor (pad > 0) and at least 8 distinct wall depths."""
import ctypes as C

import numpy as np
import pytest

import learner_view_depth_ref as LD
from helpers import CFG1
from learner_view_depth_rollout import AGENT_LDS, ROLLOUTS, DepthRollout

pytestmark = pytest.mark.gpu

def rollout(rcw, oracle, name, **kw):
    d = DepthRollout(rcw, oracle, name, **kw).run()
    d.close()


FULL = [("depth", "chw"), ("rgbd", "chw"), ("grayd", "chw"), ("depth", "hwc")]


@pytest.mark.parametrize("fmt,layout", FULL, ids=[f"{f} {l}" for f, l in FULL])
def test_the_full_size_kernel(rcw, oracle, fmt, layout):
    """64 columns x 256 rows at full size: rcw_view_full_kernel, the depth plane one more plane item"""
    rollout(rcw, oracle, "cfg1", fmt=fmt, size=None, layout=layout)


ALL = [(f, l) for f in ("depth", "rgbd", "grayd") for l in ("chw", "hwc")]
AGENT = [("cfg1", (84, 64)), ("cfg1", (37, 53)), ("cfg1", (1, 1)), ("cfg1", (256, 1)), ("cfg1", (1, 64)),
         ("odd", (37, 33)), ("odd", (37, 33 - 1)), ("odd", (1, 1)), ("odd", (37, 1)), ("odd", (1, 33)), ("odd", (20, 17))]


@pytest.mark.parametrize("name,size", AGENT, ids=[f"{n} {s[0]}x{s[1]}" for n, s in AGENT])
def test_the_agent_kernel(rcw, oracle, name, size):
    """rcw_view_agent_kernel: (84, 84) and (37, 53) clipped to the view, one pixel, one column, one row, and — at 33 columns, which the full
    kernel does not take — full size; all three formats in both layouts (HWC RGB-D: the 4-byte store)"""
    for fmt, layout in ALL:
        rollout(rcw, oracle, name, fmt=fmt, size=size, layout=layout)


BOX = [("many rays", "depth", (8, 700), "chw"), ("many rays", "rgbd", (5, 33), "hwc"), ("depth table", "grayd", (7, 300), "chw")]


@pytest.mark.parametrize("name,fmt,size,layout", BOX, ids=[f"{b[0]} {b[1]}" for b in BOX])
def test_the_box_kernel(rcw, oracle, name, fmt, size, layout):
    """rcw_view_box_kernel: the column tables beyond 64 KiB of LDS — at 5000 rays x 1500 rows only because of the depth table's 1501 words"""
    cfg = ROLLOUTS[name][0]
    if name == "depth table":
        assert AGENT_LDS(cfg, size) <= 64 * 1024 < AGENT_LDS(cfg, size) + (cfg["height_camera_view_pu"] + 1) * 4
    else:
        assert AGENT_LDS(cfg, size) > 64 * 1024
    rollout(rcw, oracle, name, fmt=fmt, size=size, layout=layout)


def test_sums_of_64_bits(rcw, oracle):
    """one box of 2048 x 4096 = 8,388,608 pixels: 257 n >= 2^31, rcw_view_box_kernel's 64-bit instantiation"""
    assert 257 * 2048 * 4096 >= 2 ** 31
    rollout(rcw, oracle, "huge box", fmt="grayd", size=(1, 1), layout="chw")


STACK = [("the fused kernel, frames of 2 x 84 x 84", "cfg2 near the goal", "grayd", (84, 84), 3),
         ("the fused kernel, frames of 7844 bytes", "cfg2 near the goal", "rgbd", (37, 53), 3),
         ("the full kernel, then the push", "cfg1 near the goal", "rgbd", None, 2),
         ("the box kernel, then the push", "many rays near the goal", "depth", (8, 700), 3),
         ("the fused kernel, six slots", "cfg2 near the goal", "grayd", (20, 30), 6)]


@pytest.mark.parametrize("what,name,fmt,size,k", STACK, ids=[s[0] for s in STACK])
def test_the_stack(rcw, oracle, what, name, fmt, size, k):
    """the k-frame stack with C = 2 and C = 4: rcw_view_agent_push_kernel (per = 14112: 16-byte chunks; 7844: bytes) and the staged frame
    with rcw_view_push_kernel behind the full and the box kernel; the slot rule (tests/learner_view_stack_ref.py) across an auto_reset
    restart and the masked reset; six slots: shift_chunk moves four a trip, its second trip inside a depth instantiation of the fused kernel"""
    assert (4 * 37 * 53) % 16 != 0 and (2 * 84 * 84) % 16 == 0
    rollout(rcw, oracle, name, fmt=fmt, size=size, layout="chw", k=k)


def test_view_only_steps(rcw, oracle):
    d = DepthRollout(rcw, oracle, "cfg2", fmt="grayd", size=(84, 84), layout="chw", camera_view=False)
    assert d.env.step_form() == "two-launches"
    frozen = d.env.camera_view_host()
    d.run()
    assert d.env.step_form() == "two-launches"
    np.testing.assert_array_equal(d.env.camera_view_host(), frozen)            # the steps left the camera view alone
    assert d.env._lib.rcw_update_camera_view(d.env._h) == 0
    np.testing.assert_array_equal(d.env.camera_view_host(), d.orc.camera_view)  # on demand
    d.close()


def test_the_one_launch_step_at_64_agents(rcw, oracle):
    d = DepthRollout(rcw, oracle, "cfg2 x 64", fmt="rgbd", size=(84, 84), layout="hwc", form="one-launch")
    assert d.env.step_form() == "one-launch"
    d.run()
    assert d.env.step_form() == "one-launch"
    d.close()


def test_expand_columns_view_of_the_handles_own_descriptors(rcw, oracle):
    torch = pytest.importorskip("torch")
    for fmt, size, layout, k in (("rgbd", (37, 53), "hwc", 1), ("depth", (84, 64), "chw", 1), ("rgbd", None, "chw", 1), ("depth", (37, 53), "chw", 3)):
        d = DepthRollout(rcw, oracle, "cfg1", fmt=fmt, size=size, layout=layout, k=k)
        for t in range(3):
            d.step(t, f"step {t}")
        hl, cid = d.env.columns()
        one = d.env.expand_columns_view(torch.from_numpy(hl).cuda(), torch.from_numpy(cid).cuda())
        torch.cuda.synchronize()
        assert tuple(one.shape) == d.single().shape                                # single-frame, whatever the stack
        np.testing.assert_array_equal(one.cpu().numpy(), d.single())
        if k == 1:
            np.testing.assert_array_equal(one.cpu().numpy(), d.env.learner_view_host())
        d.check("after expand_columns_view")
        d.close()


def test_refusals_leave_the_previous_view(rcw, oracle):
    from raycastworlds_jl_amd import _capi

    env = rcw.SingleRoomModule.SingleRoom(batch=4, seed=2, **CFG1)
    lib, h = env._lib, env._h
    assert (_capi.RCW_VIEW_DEPTH8, _capi.RCW_VIEW_RGBD8, _capi.RCW_VIEW_GRAYD8) == (4, 5, 6)
    env.set_learner_view("grayd", (20, 30), "chw", stack=2)
    p0, bytes0 = env.learner_view.ptr, env.learner_view_host()
    info0 = env.learner_view_info()
    assert info0 == {"format": "grayd", "layout": "chw", "size": (20, 30), "camera_view": True}
    raw = [C.c_int32() for _ in range(5)]
    assert lib.rcw_learner_view_info(h, *[C.byref(x) for x in raw]) == 0 and raw[0].value == _capi.RCW_VIEW_GRAYD8
    refused = [((f, _capi.RCW_VIEW_CHW, 20, 30, 0, 1), _capi.RCW_ERR_INVALID_ARGUMENT) for f in (3, 7, 8, -1)]
    refused.append(((_capi.RCW_VIEW_GRAYD8, _capi.RCW_VIEW_HWC, 20, 30, 0, 2), _capi.RCW_ERR_UNSUPPORTED))
    for args, code in refused:
        assert lib.rcw_set_learner_view_stack(h, *args) == code, args
        if args[5] == 1:
            assert lib.rcw_set_learner_view(h, *args[:5]) == code, args
        assert env.learner_view.ptr == p0 and env.learner_view_stack == 2 and env.learner_view_info() == info0, args
        np.testing.assert_array_equal(env.learner_view_host(), bytes0)
    with pytest.raises(ValueError):
        env.set_learner_view("depthd", (20, 30))
    for fmt, c in (("depth", 1), ("rgbd", 4), ("grayd", 2)):
        env.set_learner_view(fmt, (20, 30), "hwc")
        assert env.learner_view.shape == (4, 20, 30, c) and env.learner_view_info()["format"] == fmt
        env.set_learner_view(fmt, (20, 30), "chw", stack=3)
        assert env.learner_view.shape == (4, 3 * c, 20, 30)
    env.close()


def test_gray_to_gray_with_depth_and_back(rcw, oracle):
    """a handle that had a depth plane for a while holds the gray bytes of one that never had; the colour planes of RGB-D / gray-D are the
    RGB / gray view"""
    mk = lambda: rcw.SingleRoomModule.SingleRoom(batch=6, seed=5, auto_reset=True, out_of_bounds=1, **CFG1)
    a, b = mk(), mk()
    rng = np.random.default_rng(1)

    def both():
        act = rng.integers(1, 5, 6).astype(np.uint8)
        rcw.act_(a, act); rcw.act_(b, act)

    for size in ((84, 64), None):
        full = size or (256, 64)
        a.set_learner_view("gray", size); b.set_learner_view("gray", size)
        both()
        np.testing.assert_array_equal(a.learner_view_host(), b.learner_view_host())
        a.set_learner_view("grayd", size)
        both()
        got = a.learner_view_host()
        assert got.shape == (6, 2) + full
        np.testing.assert_array_equal(got[:, :1], b.learner_view_host())
        a.set_learner_view("rgbd", size, "hwc"); b.set_learner_view("rgb", size, "hwc")
        both()
        np.testing.assert_array_equal(a.learner_view_host()[..., :3], b.learner_view_host())
        a.set_learner_view("gray", size); b.set_learner_view("gray", size)
        both()
        np.testing.assert_array_equal(a.learner_view_host(), b.learner_view_host())
        hl, cid = a.columns()
        np.testing.assert_array_equal(a.learner_view_host(), LD.view(hl, cid, a.cfg, 256, "gray", full))
    a.close(); b.close()
