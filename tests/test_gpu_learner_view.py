"""The learner view on the GPU (include/rcw.h "the learner view"): every byte against the contract's numpy restatement
(tests/learner_view_ref.py) applied to the engine's own frames and to the CPU oracle's, through rollouts in both step forms, the
view-only step, the five exports' refusals, hand-made descriptors, a captured step and BASELINE cfg-2 at its full size."""
import ctypes as C

import numpy as np
import pytest

import learner_view_ref as LV
from helpers import CFG1, CFG2, CFG3, CFG5, REFERENCE_DEFAULT, assert_state_equal

pytestmark = pytest.mark.gpu


def _make(rcw, oracle, batch, seed=0, **kw):
    env = rcw.SingleRoomModule.SingleRoom(batch=batch, seed=seed, **kw)
    okw = {k: v for k, v in kw.items() if k not in ("auto_reset", "T")}
    if kw.get("auto_reset"):
        okw["auto_reset"] = 1
    if kw.get("T") == "Float64":
        okw["world_unit_bits"] = 64
    orc = oracle.OracleBatch(batch, seed=seed, **okw)
    return env, orc


def _check_view(env, frames, fmt, size, layout, where=""):
    got = env.learner_view_host()
    want = LV.from_frames(frames, fmt, size, layout)
    assert got.shape == want.shape, (got.shape, want.shape, where)
    np.testing.assert_array_equal(got, want, err_msg=f"learner view {fmt} {size} {layout} {where}")


def test_full_size_is_the_camera_view_unpacked(rcw, oracle):
    from raycastworlds_jl_amd.viewer import frame_to_rgb

    for cfg in (CFG1, CFG2, REFERENCE_DEFAULT, dict(CFG1, height_camera_view_pu=100), dict(CFG1, num_rays=50)):
        env, orc = _make(rcw, oracle, 5, seed=3, **cfg)
        H, N = env.cfg.height_camera_view_pu, env.cfg.num_rays
        for fmt, layout in (("rgb", "chw"), ("rgb", "hwc"), ("gray", "chw"), ("gray", "hwc")):
            env.set_learner_view(fmt, None, layout)
            frames = env.camera_view_host()
            got = env.learner_view_host()
            if fmt == "rgb":
                want = np.stack([frame_to_rgb(f) for f in frames])
                np.testing.assert_array_equal(got, want.transpose(0, 3, 1, 2) if layout == "chw" else want, err_msg=f"{cfg} {layout}")
            else:
                np.testing.assert_array_equal(got.reshape(5, H, N), LV.from_frames(frames, "gray", (H, N))[:, 0], err_msg=f"{cfg}")
            np.testing.assert_array_equal(frames, orc.camera_view)
        env.close(); orc.close()


def test_downsampled_sizes_against_the_engines_and_the_oracles_frames(rcw, oracle):
    for cfg in (CFG1, CFG2, CFG3, CFG5, dict(CFG1, height_camera_view_pu=100)):
        env, orc = _make(rcw, oracle, 4, seed=8, **cfg)
        rng = np.random.default_rng(3)
        for _ in range(5):
            a = rng.integers(1, 5, 4).astype(np.uint8)
            rcw.act_(env, a); orc.step(a)
        H, N = env.cfg.height_camera_view_pu, env.cfg.num_rays
        for size in ((1, 1), (H, 1), (1, N), (37, 53), (84, 84), (H // 2, N // 2), (H, N // 3)):
            size = (min(size[0], H), min(size[1], N))
            for fmt in ("rgb", "gray"):
                for layout in ("chw", "hwc"):
                    env.set_learner_view(fmt, size, layout)
                    _check_view(env, env.camera_view_host(), fmt, size, layout, f"{cfg} engine")
                    _check_view(env, orc.camera_view, fmt, size, layout, f"{cfg} oracle")
        env.close(); orc.close()


ROLLOUTS = [("cfg2 84", dict(CFG2), "gray", (84, 84), "chw"),
            ("cfg2 full rgb", dict(CFG2), "rgb", None, "chw"),
            ("cfg1 37x53 hwc", dict(CFG1), "rgb", (37, 53), "hwc"),
            ("cfg2 full gray", dict(CFG2), "gray", None, "hwc")]


@pytest.mark.parametrize("form", ["two-launches", "one-launch"])
@pytest.mark.parametrize("name,cfg,fmt,size,layout", ROLLOUTS, ids=[r[0] for r in ROLLOUTS])
def test_rollouts_against_the_oracle(rcw, oracle, form, name, cfg, fmt, size, layout):
    torch = pytest.importorskip("torch")
    env, orc = _make(rcw, oracle, 24, seed=21, auto_reset=True, out_of_bounds=1, **cfg)
    env.set_step_form(form)
    env.set_learner_view(fmt, size, layout)
    size = size or (env.cfg.height_camera_view_pu, env.cfg.num_rays)
    rng = np.random.default_rng(7)
    for s in range(24):
        a = rng.integers(1, 5, env.batch).astype(np.uint8)
        if s % 3 == 0:
            rcw.act_(env, torch.from_numpy(a).cuda())
        else:
            rcw.act_(env, a)
        orc.step(a)
        if s % 6 == 5:
            _check_view(env, orc.camera_view, fmt, size, layout, f"{form} step {s}")
    # invalid device actions: those agents are not stepped
    bad = rng.integers(1, 5, env.batch).astype(np.uint8)
    bad[5] = 0; bad[11] = 7
    rcw.act_(env, torch.from_numpy(bad).cuda()); orc.step_lenient(bad)
    with pytest.raises(AssertionError):
        env.sync()
    env.clear_error(); orc.clear_status()
    _check_view(env, orc.camera_view, fmt, size, layout, "after invalid device actions")
    # a masked reset with a new seed: the masked agents only
    before = env.learner_view_host()
    mask = np.zeros(env.batch, np.uint8); mask[::3] = 1
    rcw.reset_(env, mask=mask, seed=99); orc.reset(mask=mask, seed=99)
    after = env.learner_view_host()
    _check_view(env, orc.camera_view, fmt, size, layout, "after a masked reset")
    np.testing.assert_array_equal(after[mask == 0], before[mask == 0])
    # a masked set_state
    w = env.world
    goal, pos, dirs = w.goal_position.copy(), w.player_position_wu.copy(), (w.player_direction_au + 5) % env.cfg.num_directions
    m2 = np.zeros(env.batch, np.uint8); m2[1::2] = 1
    env.set_state(goal, pos, dirs, mask=m2); orc.set_state(goal, pos, dirs, mask=m2)
    _check_view(env, orc.camera_view, fmt, size, layout, "after a masked set_state")
    for s in range(6):
        a = rng.integers(1, 5, env.batch).astype(np.uint8)
        rcw.act_(env, a); orc.step(a)
    assert_state_equal(env, orc, where=f"{form} end")
    _check_view(env, orc.camera_view, fmt, size, layout, f"{form} end")
    env.close(); orc.close()


def test_float64_worlds_and_a_handle_with_the_top_view(rcw, oracle):
    for kw, size in ((dict(T="Float64", **CFG2), (84, 84)), (dict(render_top_view=1, pu_per_tu=16, **CFG1), (64, 64)),
                     (dict(render_top_view=1, pu_per_tu=16, **CFG1), (30, 17))):
        env, orc = _make(rcw, oracle, 9, seed=5, **kw)
        env.set_learner_view("rgb", size, "chw")
        rng = np.random.default_rng(2)
        for s in range(15):
            a = rng.integers(1, 5, env.batch).astype(np.uint8)
            rcw.act_(env, a); orc.step(a)
            try:
                env.sync()
            except IndexError:
                env.clear_error(); orc.clear_status()
        _check_view(env, orc.camera_view, "rgb", size, "chw", f"{kw}")
        if kw.get("render_top_view"):
            np.testing.assert_array_equal(env.top_view_host(), orc.top_view)
        env.close(); orc.close()


def test_view_only_steps(rcw, oracle):
    from raycastworlds_jl_amd._capi import RcwError

    for kw in (dict(CFG2), dict(render_top_view=1, pu_per_tu=16, **CFG1)):
        env, orc = _make(rcw, oracle, 16, seed=6, out_of_bounds=1, **kw)
        lib, h = env._lib, env._h
        if not kw.get("render_top_view"):
            env.set_step_form("one-launch")
            assert env.step_form() == "one-launch"
        env.set_learner_view("gray", (84, 84) if env.cfg.num_rays >= 84 else (50, 50), "chw", camera_view=False)
        size = env.learner_view_info()["size"]
        assert env.learner_view_info()["camera_view"] is False
        assert env.step_form() == "two-launches"
        with pytest.raises(RcwError) as e:
            env.set_step_form("one-launch")
        assert e.value.code == -7
        env.set_step_form(None)
        assert env.step_form() == "two-launches"
        assert env.fill_kernel_name().startswith("rcw_fill")
        frozen = env.camera_view_host()
        rl = rcw.RLBaseEnv(env)
        with pytest.raises(RuntimeError):
            rcw.RLBase.state(rl)
        rl2 = rcw.RLBaseEnv(env, observation="learner_view")
        assert rcw.RLBase.state(rl2).shape == (16, 1) + size
        rng = np.random.default_rng(1)
        for s in range(12):
            a = rng.integers(1, 5, env.batch).astype(np.uint8)
            rcw.act_(env, a); orc.step(a)
        env.sync()
        np.testing.assert_array_equal(env.camera_view_host(), frozen)          # steps leave the camera view alone
        _check_view(env, orc.camera_view, "gray", size, "chw", "view only")
        assert_state_equal(env, orc, frames=False, where="view only")
        if kw.get("render_top_view"):
            np.testing.assert_array_equal(env.top_view_host(), orc.top_view)
        assert lib.rcw_update_camera_view(h) == 0
        np.testing.assert_array_equal(env.camera_view_host(), orc.camera_view)  # on demand
        # back to the camera view in the step: rendered at once, and the rule's step form again
        env.set_learner_view("gray", size, "chw")
        np.testing.assert_array_equal(env.camera_view_host(), orc.camera_view)
        a = rng.integers(1, 5, env.batch).astype(np.uint8)
        rcw.act_(env, a); orc.step(a)
        np.testing.assert_array_equal(env.camera_view_host(), orc.camera_view)
        _check_view(env, orc.camera_view, "gray", size, "chw", "after view only")
        env.close(); orc.close()


def test_set_learner_view_renders_reconfigures_refuses_and_frees(rcw, oracle):
    from raycastworlds_jl_amd import _capi

    env, orc = _make(rcw, oracle, 6, seed=2, **CFG1)
    lib, h = env._lib, env._h
    H, N = env.cfg.height_camera_view_pu, env.cfg.num_rays
    p = C.c_void_p()
    assert lib.rcw_learner_view_device_ptr(h, C.byref(p)) == _capi.RCW_ERR_UNSUPPORTED      # none yet
    out = np.empty(16, np.uint8)
    assert lib.rcw_learner_view_copy(h, out.ctypes.data_as(C.c_void_p), 0, 1) == _capi.RCW_ERR_UNSUPPORTED
    assert env.learner_view_info() == {"format": None, "layout": "chw", "size": (0, 0), "camera_view": True}
    env.set_learner_view("rgb", (20, 30), "hwc")                               # rendered at once
    _check_view(env, orc.camera_view, "rgb", (20, 30), "hwc", "at once")
    v1 = env.learner_view
    assert v1.shape == (6, 20, 30, 3) and v1.dtype == np.uint8
    np.testing.assert_array_equal(np.asarray(v1), env.learner_view_host())
    t = v1.torch(sync=True)
    np.testing.assert_array_equal(t.cpu().numpy(), env.learner_view_host())
    bad = [(3, 0, 20, 30, 0), (1, 2, 20, 30, 0), (1, 0, 0, 30, 0), (1, 0, 20, 0, 0), (1, 0, H + 1, 30, 0), (1, 0, 20, N + 1, 0),
           (1, 0, 20, 30, 2), (0, 0, 0, 0, 1), (-1, 0, 20, 30, 0)]
    for args in bad:
        assert lib.rcw_set_learner_view(h, *args) == _capi.RCW_ERR_INVALID_ARGUMENT, args
        assert env.learner_view_info()["size"] == (20, 30)
        assert lib.rcw_learner_view_device_ptr(h, C.byref(p)) == 0 and p.value == v1.ptr
    with pytest.raises(ValueError):
        env.set_learner_view("gray", (H + 1, 2))
    rng = np.random.default_rng(0)
    a = rng.integers(1, 5, 6).astype(np.uint8)
    rcw.act_(env, a); orc.step(a)
    _check_view(env, orc.camera_view, "rgb", (20, 30), "hwc", "old view still works")
    env.set_learner_view("gray", (7, 9), "chw")
    v2 = env.learner_view
    assert v2.shape == (6, 1, 7, 9) and v2.ptr != 0
    _check_view(env, orc.camera_view, "gray", (7, 9), "chw", "reconfigured")
    fmt, lay, hh, ww, fl = (C.c_int32() for _ in range(5))
    assert lib.rcw_learner_view_info(h, C.byref(fmt), C.byref(lay), C.byref(hh), C.byref(ww), C.byref(fl)) == 0
    assert (fmt.value, lay.value, hh.value, ww.value, fl.value) == (_capi.RCW_VIEW_GRAY8, _capi.RCW_VIEW_CHW, 7, 9, 0)
    env.set_learner_view(None)
    assert env.learner_view_info()["format"] is None
    assert lib.rcw_learner_view_device_ptr(h, C.byref(p)) == _capi.RCW_ERR_UNSUPPORTED
    rcw.act_(env, a); orc.step(a)                                              # a handle without a view steps as before
    assert_state_equal(env, orc, where="view off")
    env.close(); orc.close()


def test_expand_columns_view_on_hand_made_descriptors(rcw, oracle):
    torch = pytest.importorskip("torch")
    env = rcw.SingleRoomModule.SingleRoom(batch=3, seed=1, **CFG2)
    H, N = env.cfg.height_camera_view_pu, env.cfg.num_rays
    rng = np.random.default_rng(4)
    n = 5
    hl = rng.integers(0, 2 * H, (n, N)).astype(np.int64)
    hl[0, :8] = [0, 1, H - 2, H - 1, H, 2 ** 31 - 1, -(2 ** 31), 2 ** 30]
    hl[1] = 0
    hl[2] = H - 1
    hl = hl.astype(np.int32)
    cid = rng.integers(0, 4, (n, N)).astype(np.uint8)
    cid[3] = np.arange(N) % 4
    cfg = env.cfg
    th, tc = torch.from_numpy(hl).cuda(), torch.from_numpy(cid).cuda()
    for fmt, size, layout in (("rgb", None, "chw"), ("gray", None, "chw"), ("rgb", (84, 84), "hwc"), ("gray", (37, 53), "chw"),
                              ("rgb", (H, N), "hwc"), ("gray", (1, 1), "chw")):
        env.set_learner_view(fmt, size, layout)
        size = size or (H, N)
        got = env.expand_columns_view(th, tc)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(got.cpu().numpy(), LV.from_descriptors(hl, cid, cfg, H, fmt, size, layout), err_msg=f"{fmt} {size}")
    env.close()


def test_a_captured_step_updates_the_view_on_replay(rcw, oracle):
    torch = pytest.importorskip("torch")
    env, orc = _make(rcw, oracle, 48, seed=31, out_of_bounds=1, auto_reset=True, **CFG2)
    env.set_step_form("one-launch")
    env.set_learner_view("gray", (84, 84))
    stream = torch.cuda.Stream()
    env.set_stream(stream.cuda_stream)
    a_host = np.random.default_rng(2).integers(1, 5, env.batch).astype(np.uint8)
    with torch.cuda.stream(stream):
        actions = torch.from_numpy(a_host).cuda()
        for _ in range(3):
            rcw.act_(env, actions); orc.step(a_host)
        stream.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            rcw.act_(env, actions)
        assert env.step_form() == "two-launches"
        for k in range(6):
            g.replay(); orc.step(a_host)
            if k % 2 == 1:
                stream.synchronize()
                _check_view(env, orc.camera_view, "gray", (84, 84), "chw", f"replay {k}")
        stream.synchronize()
    assert_state_equal(env, orc, where="after 6 replays")
    env.close(); orc.close()


def test_baseline_cfg2_full_size(rcw, oracle):
    env, orc = _make(rcw, oracle, 4096, seed=0, **CFG2)
    a = np.random.default_rng(0).integers(1, 5, 4096).astype(np.uint8)
    env.set_learner_view("gray", (84, 84))
    rcw.act_(env, a); orc.step(a)
    _check_view(env, orc.camera_view, "gray", (84, 84), "chw", "cfg-2 gray 84")
    env.set_learner_view("rgb", None, "chw")
    rcw.act_(env, a); orc.step(a)
    _check_view(env, orc.camera_view, "rgb", (256, 256), "chw", "cfg-2 rgb full")
    env.close(); orc.close()
