"""The learner view's k-frame stack on the GPU (include/rcw.h "the frame stack"): every byte of the stack against the numpy model
(tests/learner_view_stack_ref.py) fed with the contract's single-frame views (tests/learner_view_ref.py) of the CPU oracle's frames and
with the oracle's episode counters, after every step.

The rollout is tests/test_gpu_unchanged_skip.py's near-the-goal one (the 8 x 8 room, every agent four forward moves from its goal,
auto_reset, forward with probability 0.7): each run asserts from the oracle's counters that at least as many episodes restarted as there
are agents and that every agent restarted, so the refill on an episode change and the shift are both exercised.  cfg-1 has 64 rays and the
view does not up-sample, so its gray k = 4 case is 84 x 64 where cfg-2's is 84 x 84."""
import ctypes as C

import numpy as np
import pytest

import learner_view_ref as LV
import learner_view_stack_ref as LS
from helpers import CFG1, CFG2
from test_gpu_unchanged_skip import Rollout
from test_learner_view_stack_spec import draw_actions

pytestmark = pytest.mark.gpu


def single(orc, fmt, size, chunk=512):
    """the single-frame learner view of the oracle's frames (in chunks of agents: the prefix sums are int64)"""
    f = orc.camera_view
    return np.concatenate([LV.from_frames(f[i:i + chunk], fmt, size) for i in range(0, len(f), chunk)])


class Stacked:
    """engine, oracle and model side by side"""

    def __init__(self, rcw, oracle, batch, k, fmt, size, camera_view=True, form=None, near_the_goal=True, seed=3, rng_seed=8, **kw):
        self.r = r = Rollout(rcw, oracle, batch, seed, rng_seed, auto_reset=True, out_of_bounds=1, **kw)
        self.rcw, self.env, self.orc, self.B, self.k, self.fmt = rcw, r.env, r.orc, batch, k, fmt
        if form is not None:
            self.env.set_step_form(form)
        self.size = size or (self.env.cfg.height_camera_view_pu, self.env.cfg.num_rays)
        if near_the_goal:
            r.set_state_near_the_goal()
        self.env.set_learner_view(fmt, size, "chw", camera_view=camera_view, stack=k)
        r.frames_checked = camera_view
        self.model = LS.StackModel(k, self.view(), self.orc.episode)
        self.restarts = np.zeros(batch, np.int64)
        self.check("after set_learner_view")

    def view(self):
        return single(self.orc, self.fmt, self.size)

    def check(self, where, state=True):
        got = self.env.learner_view_host()
        c = 3 if self.fmt == "rgb" else 1
        assert got.shape == self.model.stack.shape == (self.B, self.k * c) + tuple(self.size), (got.shape, where)
        if not np.array_equal(got, self.model.stack):
            bad = np.argwhere((got != self.model.stack).reshape(self.B, self.k, -1).any(axis=2))
            raise AssertionError(f"the stack {where}: {len(bad)} (agent, slot) pairs differ, first {bad[:8].tolist()}")
        if state:
            self.r.check(where)

    def step(self, where, device=False, a=None, check=True):
        a = draw_actions(self.r.rng, self.B) if a is None else a
        ep = self.orc.episode.copy()
        if device:
            import torch

            self.rcw.act_(self.env, torch.from_numpy(a).cuda())
        else:
            self.rcw.act_(self.env, a)
        assert self.orc.step(a) == 0
        self.pushed(ep)
        if check:
            self.check(where)

    def pushed(self, ep):
        self.restarts += (self.orc.episode - ep).astype(np.int64)
        self.model.push(self.view(), self.orc.episode)

    def assert_every_agent_restarted(self):
        assert self.restarts.sum() >= self.B and (self.restarts >= 1).all(), (int(self.restarts.sum()), int((self.restarts >= 1).sum()))

    def close(self):
        self.env.close(); self.orc.close()


CASES = [("cfg2 gray 84x84 k4", CFG2, 4, "gray", (84, 84)), ("cfg1 gray 84x64 k4", CFG1, 4, "gray", (84, 64)),
         ("cfg2 rgb 37x53 k3", CFG2, 3, "rgb", (37, 53)), ("cfg1 rgb 37x53 k3", CFG1, 3, "rgb", (37, 53))]


@pytest.mark.parametrize("camera_view", [True, False], ids=["with the camera view", "RCW_VIEW_ONLY"])
@pytest.mark.parametrize("form", ["two-launches", "one-launch"])
@pytest.mark.parametrize("name,cfg,k,fmt,size", CASES, ids=[c[0] for c in CASES])
def test_the_near_the_goal_rollout(rcw, oracle, name, cfg, k, fmt, size, form, camera_view):
    pytest.importorskip("torch")
    s = Stacked(rcw, oracle, 64, k, fmt, size, camera_view=camera_view, form=form, **cfg)
    assert s.env.learner_view_stack == k
    assert s.env.step_form() == (form if camera_view else "two-launches")      # (RCW_VIEW_ONLY: the one-launch request gives way)
    for t in range(24):
        s.step(f"{name} {form} step {t}", device=t % 3 == 0)
        np.testing.assert_array_equal(s.env.world.episode, s.orc.episode)
    s.assert_every_agent_restarted()
    s.close()


# 5600 rays: the per-column tables of rcw_view_agent_kernel (3 words a ray + the box bounds) pass 64 KiB of LDS, so every reduced size
# takes rcw_view_box_kernel — into the staging frame, with rcw_view_push_kernel behind it
MANY_RAYS = dict(height_tile_map_tu=8, width_tile_map_tu=8, num_rays=5600, height_camera_view_pu=16)
KERNELS = [("rcw_view_full_kernel gray, then the push", CFG2, "gray", None, 2),
           ("rcw_view_full_kernel rgb, then the push", CFG2, "rgb", None, 2),
           ("rcw_view_box_kernel, then the push in 16-byte chunks", MANY_RAYS, "gray", (8, 700), 3),
           ("rcw_view_box_kernel, then the push in bytes", MANY_RAYS, "rgb", (5, 33), 4),
           ("the fused kernel, a column of 256 rows", CFG2, "gray", (256, 1), 3),
           ("the fused kernel, frames of 37 x 53 bytes", CFG2, "gray", (37, 53), 4),
           ("the fused kernel, frames of 3 bytes and 16 slots", CFG2, "rgb", (1, 1), 16),
           ("the fused kernel, frames of one 16-byte chunk", CFG2, "gray", (2, 8), 5)]


@pytest.mark.parametrize("name,cfg,fmt,size,k", KERNELS, ids=[c[0] for c in KERNELS])
def test_every_kernel_that_writes_the_stack(rcw, oracle, name, cfg, fmt, size, k):
    """which kernel a case takes follows from rcw_launch_view_stack's rule: full size (256 x 256 at cfg-2) is rcw_view_full_kernel, tables
    beyond 64 KiB of LDS are rcw_view_box_kernel — both write the staging frame and rcw_view_push_kernel follows, in 16-byte chunks where
    C h w is a multiple of 16 (5600) and in bytes where it is not (495) —, everything else is rcw_view_agent_push_kernel, whose shift
    has the same two paths"""
    s = Stacked(rcw, oracle, 24, k, fmt, size, **cfg)
    if cfg is MANY_RAYS:
        assert (3 * s.env.cfg.num_rays + s.size[0] + s.size[1] + 2) * 4 > 64 * 1024
    for t in range(12):
        s.step(f"{name} step {t}", device=t % 2 == 1)
    assert s.restarts.sum() >= 12, int(s.restarts.sum())
    s.close()


@pytest.mark.parametrize("form", ["two-launches", "one-launch"])
def test_masked_reset_and_set_state_refill_by_the_mask(rcw, oracle, form):
    s = Stacked(rcw, oracle, 48, 4, "gray", (84, 84), form=form, **CFG2)
    env, orc, m = s.env, s.orc, s.model
    for t in range(5):
        s.step(f"step {t}")
    # a masked reset with a NEW seed: the counters of the masked agents go to 0 — which some of them held already
    before = env.learner_view_host()
    mask = np.zeros(48, np.uint8); mask[::3] = 1
    s.rcw.reset_(env, mask=mask, seed=99); orc.reset(mask=mask, seed=99)
    m.refill(s.view(), mask, orc.episode)
    s.check("after a masked reset")
    after = env.learner_view_host()
    np.testing.assert_array_equal(after[mask == 0], before[mask == 0])
    one = s.view()
    for slot in range(4):
        np.testing.assert_array_equal(after[mask == 1, slot], one[mask == 1, 0])
    for t in range(3):
        s.step(f"after the masked reset, step {t}")
    # a masked set_state
    w = env.world
    goal, pos, dirs = w.goal_position.copy(), w.player_position_wu.copy(), (w.player_direction_au + 5) % env.cfg.num_directions
    m2 = np.zeros(48, np.uint8); m2[1::2] = 1
    before = env.learner_view_host()
    env.set_state(goal, pos, dirs, mask=m2); orc.set_state(goal, pos, dirs, mask=m2)
    m.refill(s.view(), m2, orc.episode)
    s.check("after a masked set_state")
    after = env.learner_view_host()
    np.testing.assert_array_equal(after[m2 == 0], before[m2 == 0])
    for slot in range(4):
        np.testing.assert_array_equal(after[m2 == 1, slot], s.view()[m2 == 1, 0])
    for t in range(3):
        s.step(f"after the masked set_state, step {t}")
    # unmasked ones
    s.rcw.reset_(env, seed=5); orc.reset(seed=5)
    m.refill(s.view(), None, orc.episode)
    s.check("after a reset")
    s.step("after the reset")
    s.r.set_state_near_the_goal()
    m.refill(s.view(), None, orc.episode)
    s.check("after set_state")
    for t in range(6):
        s.step(f"after set_state, step {t}")
    s.close()


def test_a_new_direction_table_refills_every_agent(rcw, oracle):
    s = Stacked(rcw, oracle, 16, 3, "gray", (84, 84), **CFG2)
    for t in range(4):
        s.step(f"step {t}")
    th = (np.arange(s.env.cfg.num_directions) * 2 * np.pi / s.env.cfg.num_directions) + 0.01
    dirs = np.stack([np.cos(th), np.sin(th)], axis=1).astype(np.float32)
    s.env.set_direction_table(dirs); s.orc.set_direction_table(dirs)
    s.model.refill(s.view(), None, s.orc.episode)
    s.check("after set_direction_table")
    got = s.env.learner_view_host()
    for slot in range(3):
        np.testing.assert_array_equal(got[:, slot], s.view()[:, 0])
    for t in range(3):
        s.step(f"after set_direction_table, step {t}")
    s.close()


def test_what_does_not_touch_the_stack(rcw, oracle):
    """the getters, cast_rays, update_camera_view, expand_columns_view and a change of the step form there and back"""
    torch = pytest.importorskip("torch")
    s = Stacked(rcw, oracle, 32, 4, "gray", (84, 84), **CFG2)
    env = s.env
    for t in range(4):
        s.step(f"step {t}")
    ptr = env.learner_view.ptr
    lib, h = env._lib, env._h
    assert lib.rcw_cast_rays(h) == 0 and lib.rcw_update_camera_view(h) == 0
    hl, cid = env.columns()
    one = env.expand_columns_view(torch.from_numpy(hl).cuda(), torch.from_numpy(cid).cuda())
    torch.cuda.synchronize()
    assert tuple(one.shape) == (32, 1, 84, 84)                                 # single-frame, whatever the stack
    np.testing.assert_array_equal(one.cpu().numpy(), s.view())
    _ = env.world.episode, env.world.reward, env.camera_view_host()
    s.check("after the calls that leave the stack alone")
    for form in ("one-launch", "two-launches", None):
        env.set_step_form(form)
        s.check(f"after set_step_form({form!r})")
        s.step(f"a step in form {form!r}")
    assert env.learner_view.ptr == ptr
    s.close()


def test_invalid_device_actions_still_push(rcw, oracle):
    torch = pytest.importorskip("torch")
    s = Stacked(rcw, oracle, 40, 4, "gray", (84, 84), **CFG2)
    env, orc = s.env, s.orc
    for t in range(4):
        s.step(f"step {t}")
    bad_agents = [3, 20, 39]
    for rep in range(2):
        a = draw_actions(s.r.rng, 40)
        a[bad_agents] = [0, 9, 255]
        ep = orc.episode.copy()
        frame_before = s.view()
        s.rcw.act_(env, torch.from_numpy(a).cuda()); orc.step_lenient(a)
        with pytest.raises(AssertionError):
            env.sync()
        np.testing.assert_array_equal(env.world.status, orc.status)
        env.clear_error(); orc.clear_status()
        np.testing.assert_array_equal(s.view()[bad_agents], frame_before[bad_agents])   # not stepped ...
        s.pushed(ep)
        s.check(f"invalid device actions {rep}")                                        # ... yet pushed
    got = env.learner_view_host()
    np.testing.assert_array_equal(got[bad_agents, 3], got[bad_agents, 1])
    for t in range(3):
        s.step(f"after the invalid actions, step {t}")
    s.close()


def test_a_stack_of_one_is_the_plain_learner_view(rcw, oracle):
    a_ = Rollout(rcw, oracle, 32, 3, 8, auto_reset=True, out_of_bounds=1, **CFG2)
    b_ = rcw.SingleRoomModule.SingleRoom(batch=32, seed=3, auto_reset=True, out_of_bounds=1, **CFG2)
    a_.set_state_near_the_goal()
    b_.set_state(np.tile(np.array([[4, 6]], np.int32), (32, 1)), np.tile(np.array([[3.5, 4.5]], np.float32), (32, 1)), np.full(32, 32, np.int32))
    for fmt, size, layout in (("gray", (84, 84), "chw"), ("rgb", (37, 53), "hwc"), ("rgb", None, "chw")):
        a_.env.set_learner_view(fmt, size, layout, stack=1)
        b_.set_learner_view(fmt, size, layout)
        assert a_.env.learner_view_stack == b_.learner_view_stack == 1
        assert a_.env.learner_view.shape == b_.learner_view.shape
        for t in range(8):
            a = draw_actions(a_.rng, 32)
            rcw.act_(a_.env, a); rcw.act_(b_, a); a_.orc.step(a)
            got = a_.env.learner_view_host()
            np.testing.assert_array_equal(got, b_.learner_view_host())
            np.testing.assert_array_equal(got, LV.from_frames(a_.orc.camera_view, fmt, size or (256, 256), layout))
    a_.env.close(); b_.close(); a_.orc.close()


def test_a_captured_step_pushes_on_every_replay(rcw, oracle):
    torch = pytest.importorskip("torch")
    s = Stacked(rcw, oracle, 64, 4, "gray", (84, 84), form="one-launch", **CFG2)
    env, orc = s.env, s.orc
    stream = torch.cuda.Stream()
    env.sync()
    env.set_stream(stream.cuda_stream)
    a_host = np.ones(64, np.uint8)                                             # forward: every agent reaches its goal and restarts
    a_host[::4] = draw_actions(s.r.rng, 16)
    with torch.cuda.stream(stream):
        actions = torch.from_numpy(a_host).cuda()
        stream.synchronize()
        ptr = env.learner_view.ptr
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            rcw.act_(env, actions)
        assert env.step_form() == "two-launches"
        for k in range(10):
            ep = orc.episode.copy()
            g.replay(); assert orc.step(a_host) == 0
            stream.synchronize()
            s.pushed(ep)
            s.check(f"replay {k}")
        assert env.learner_view.ptr == ptr
        for t in range(3):
            s.step(f"behind the replays, step {t}")
        stream.synchronize()
    assert s.restarts.sum() >= 32, int(s.restarts.sum())
    del g
    s.close()


def test_refusals(rcw, oracle):
    from raycastworlds_jl_amd import _capi
    from raycastworlds_jl_amd._capi import RcwError

    env = rcw.SingleRoomModule.SingleRoom(batch=6, seed=2, **CFG2)
    lib, h = env._lib, env._h
    k = C.c_int32(-1)
    assert lib.rcw_learner_view_stack(h, C.byref(k)) == 0 and k.value == 0     # no view: 0
    assert env.learner_view_stack == 0
    assert lib.rcw_learner_view_stack(h, None) == _capi.RCW_ERR_INVALID_ARGUMENT
    assert lib.rcw_learner_view_stack(None, C.byref(k)) == _capi.RCW_ERR_INVALID_ARGUMENT
    with pytest.raises(RuntimeError):
        env.learner_view
    G, CHW, HWC = _capi.RCW_VIEW_GRAY8, _capi.RCW_VIEW_CHW, _capi.RCW_VIEW_HWC
    assert lib.rcw_set_learner_view_stack(h, G, CHW, 20, 30, 0, 3) == 0
    p0 = env.learner_view.ptr
    refused = [((G, HWC, 20, 30, 0, 2), _capi.RCW_ERR_UNSUPPORTED), ((_capi.RCW_VIEW_RGB8, HWC, 20, 30, 0, 16), _capi.RCW_ERR_UNSUPPORTED),
               ((G, CHW, 20, 30, 0, 0), _capi.RCW_ERR_INVALID_ARGUMENT), ((G, CHW, 20, 30, 0, 17), _capi.RCW_ERR_INVALID_ARGUMENT),
               ((G, CHW, 20, 30, 0, -1), _capi.RCW_ERR_INVALID_ARGUMENT), ((G, CHW, 0, 30, 0, 2), _capi.RCW_ERR_INVALID_ARGUMENT),
               ((G, CHW, 20, 257, 0, 2), _capi.RCW_ERR_INVALID_ARGUMENT), ((G, CHW, 20, 30, 2, 2), _capi.RCW_ERR_INVALID_ARGUMENT),
               ((3, CHW, 20, 30, 0, 2), _capi.RCW_ERR_INVALID_ARGUMENT), ((G, 2, 20, 30, 0, 2), _capi.RCW_ERR_INVALID_ARGUMENT)]
    for args, code in refused:
        assert lib.rcw_set_learner_view_stack(h, *args) == code, args
        assert env.learner_view_stack == 3 and env.learner_view.ptr == p0      # the previous view stays as it was
        assert env.learner_view_info() == {"format": "gray", "layout": "chw", "size": (20, 30), "camera_view": True}
    with pytest.raises(RcwError) as e:
        env.set_learner_view("gray", (20, 30), layout="hwc", stack=2)
    assert e.value.code == _capi.RCW_ERR_UNSUPPORTED
    for k in (0, 17):
        with pytest.raises(ValueError):                                        # (RCW_ERR_INVALID_ARGUMENT, as the binding raises it)
            env.set_learner_view("gray", (20, 30), stack=k)
    assert env.learner_view_stack == 3 and env.learner_view.ptr == p0
    env.set_learner_view("gray", (20, 30), "hwc", stack=1)                      # HWC with one frame: as ever
    assert env.learner_view_stack == 1 and env.learner_view.shape == (6, 20, 30, 1)
    assert lib.rcw_set_learner_view_stack(h, G, CHW, 20, 30, 0, 16) == 0
    assert env.learner_view_stack == 16 and env.learner_view.shape == (6, 16, 20, 30)
    env.set_learner_view(None)
    assert env.learner_view_stack == 0
    env.close()


def test_copies_and_the_rlbase_state(rcw, oracle):
    s = Stacked(rcw, oracle, 20, 3, "rgb", (37, 53), **CFG2)
    env = s.env
    for t in range(5):
        s.step(f"step {t}")
    want = s.model.stack
    np.testing.assert_array_equal(env.learner_view_host(first=7, count=5), want[7:12])
    np.testing.assert_array_equal(env.learner_view_host(first=19), want[19:])
    out = np.full((4, 9, 37, 53), 7, np.uint8)
    assert env._lib.rcw_learner_view_copy(env._h, out.ctypes.data_as(C.c_void_p), 2, 3) == 0
    np.testing.assert_array_equal(out[:3], want[2:5])
    assert (out[3] == 7).all()                                                 # count * k * C * h * w bytes, not one more
    assert env._lib.rcw_learner_view_copy(env._h, out.ctypes.data_as(C.c_void_p), 18, 3) != 0
    v = env.learner_view
    assert v.shape == (20, 9, 37, 53) and v.dtype == np.uint8
    np.testing.assert_array_equal(np.asarray(v), want)
    np.testing.assert_array_equal(v.torch(sync=True).cpu().numpy(), want)
    rl = rcw.RLBaseEnv(env, observation="learner_view")
    st = rcw.RLBase.state(rl)
    assert st.shape == (20, 9, 37, 53) and st.ptr == v.ptr
    s.step("after the copies")
    np.testing.assert_array_equal(np.asarray(rcw.RLBase.state(rl)), s.model.stack)
    s.close()


class StackedByDescriptors(Stacked):
    """the single-frame views from the oracle's column descriptors — the contract's other numpy reading, several times cheaper at 4096
    agents (tests/test_learner_view_spec.py holds the two readings against each other) — and from its frames for the first 128 agents"""

    def view(self):
        o = self.orc
        v = np.concatenate([LV.from_descriptors(o.col_height[i:i + 256], o.col_colour[i:i + 256], o.cfg, o.Hc, self.fmt, self.size)
                            for i in range(0, self.B, 256)])
        np.testing.assert_array_equal(v[:128], LV.from_frames(o.camera_view[:128], self.fmt, self.size))
        return v


def test_baseline_cfg2_at_its_full_batch(rcw, oracle):
    s = StackedByDescriptors(rcw, oracle, 4096, 4, "gray", (84, 84), **CFG2)
    s.r.frames_checked = False                                                  # (the camera view of 4096 agents is tests/test_gpu_unchanged_skip.py's)
    for t in range(12):
        s.step(f"cfg-2 x 4096, step {t}", device=t % 2 == 0)
    assert s.restarts.sum() >= 4096 // 2, int(s.restarts.sum())
    s.close()
