"""The wall bank on the GPU (include/rcw.h, rcw_set_wall_bank): the scenarios of tests/wall_bank_cases.py played on an engine against
tests/wall_bank_ref.py — after EVERY call the whole state of walls_ref.assert_equal (status, episode, goal, pose, reward, done, tile-map
chunks, column descriptors, camera view), wall_layout, and the time limit's two words; where they are on, the goal distance's words and
fields, the seen map, the local map and the frame stack as well.  tests/test_wall_bank_spec.py rehearses every scenario on the CPU and
asserts from the reference's counts that it reaches restarts of both kinds, kept and changed layouts and goal redraws.

The `small` scenario is the issue's own (67 agents x 320 rays, 30 steps): its reference takes some ten seconds of Python ray casting, once,
shared by the two step forms.  Every export is missing from the build before this feature: each test here fails there.
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import goal_distance_ref as GD
import learner_view_ref as LV
import learner_view_stack_ref as LS
import local_map_ref as LM
import seen_map_ref as SM
import wall_bank_cases as BC
import wall_bank_ref as WB
import walls_ref as WR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the rollouts -----------------------------------------------------------------------------------------------------------------
ROLLOUTS = [("small", "two-launches"), ("small", "one-launch"), ("square_one", None), ("square_zero_weight", None), ("big", "two-launches"),
            ("big", "one-launch"), ("f64", None), ("calls", "two-launches"), ("calls", "one-launch"), ("edge", None)]


@pytest.mark.parametrize("name,form", ROLLOUTS, ids=[f"{n}-{f or 'auto'}" for n, f in ROLLOUTS])
def test_a_scenario_against_the_reference_after_every_call(rcw, name, form):
    env = BC.make_env(rcw, BC.SCENARIOS[name][1], form)
    events = BC.play(rcw, name, env)
    assert events["episode_starts"] > env.batch
    if form is not None:
        assert env.step_form() == form
    if name == "f64":
        assert env.world.player_position_wu.dtype == np.float64
    if name == "big":
        assert env.world.tile_map_chunks.shape[1] * 2 > 64                    # more tile-map words than a wavefront has lanes
        assert max(events["layouts_drawn"]) >= 64
    if name == "edge":                                                        # the largest map a handle takes: 64 passes of the copy loops, 15.8 KiB of LDS
        assert env.world.tile_map_chunks.shape[1] * 2 == 4050 == 64 * 64 - 46
        assert events["layouts_drawn"] == {0, 2} and events["restarts_after_done"] > 0 and events["restarts_after_truncation"] > 0
    env.close()


# ---- the features beside a bank -----------------------------------------------------------------------------------------------------
class GoalTracker:
    """goal_distance_ref.Tracked told by the player what happened; the walls are read afresh after every call (a restart changes them)"""

    def __init__(self, rcw, env):
        self.t = GD.Tracked(rcw, env)

    def stepped(self, actions, where):
        self.t.ref.stepped(*self.t.state())
        self.t.check(where)

    def masked(self, mask, where):
        self.t.masked(mask, where)


class SeenTracker:
    def __init__(self, rcw, env):
        self.t = SM.Tracked(rcw, env)

    def stepped(self, actions, where):
        self.t.stepped(actions, where)

    def masked(self, mask, where):
        self.t.masked(mask, where)


class LocalTracker:
    def __init__(self, rcw, env, size, cells, source):
        self.t = LM.Tracked(rcw, env, size, cells, source)

    def stepped(self, actions, where):
        self.t.check(where)

    def masked(self, mask, where):
        self.t.check(where)


class StackTracker:
    """the k-frame learner view: learner_view_ref fed with the engine's own descriptors, learner_view_stack_ref's model of the slots"""

    def __init__(self, env, k, fmt, size):
        self.env, self.fmt, self.size = env, fmt, size
        env.set_learner_view(fmt, size, "chw", stack=k)
        self.model = LS.StackModel(k, self.view(), env.world.episode)
        self.check("enabled")
        self.refills = 0

    def view(self):
        h, c = self.env.columns()
        return LV.from_descriptors(h, c, self.env.cfg, self.env.cfg.height_camera_view_pu, self.fmt, self.size)

    def check(self, where):
        np.testing.assert_array_equal(self.env.learner_view_host(), self.model.stack, err_msg=f"the frame stack {where}")

    def stepped(self, actions, where):
        self.model.push(self.view(), self.env.world.episode)
        self.check(where)

    def masked(self, mask, where):
        self.model.refill(self.view(), np.ones(self.env.batch, np.uint8) if mask is None else mask, self.env.world.episode)
        self.check(where)


FEATURES = ["goal_distance", "seen_map", "local_seen", "stack", "everything"]


@pytest.mark.parametrize("form", ["two-launches", "one-launch"])
@pytest.mark.parametrize("feature", FEATURES)
def test_the_features_follow_the_new_maze_in_one_pass(rcw, feature, form):
    """each feature beside a bank (and all of them at once): the camera view against the reference, the feature against its own reference fed
    with the engine's state, after every call of the `features` scenario"""
    env = BC.make_env(rcw, BC.CALLS, form)
    trackers = []
    if feature in ("goal_distance", "everything"):
        trackers.append(GoalTracker(rcw, env))
    if feature in ("seen_map", "local_seen", "everything"):
        trackers.append(SeenTracker(rcw, env))
    if feature in ("local_seen", "everything"):
        trackers.append(LocalTracker(rcw, env, 9, 2, LM.SEEN))
    if feature in ("stack", "everything"):
        trackers.append(StackTracker(env, 4, "gray", (21, 21)))
    events = BC.play(rcw, "features", env, trackers)
    assert events["layout_changed"] > 0 and events["restarts_after_done"] > 0 and events["restarts_after_truncation"] > 0
    assert env.step_form() == form
    env.close()


def test_view_only_and_the_top_view_beside_a_plain_bank_handle(rcw):
    """RCW_VIEW_ONLY (the step paints no camera view: the bank's kernel sits between the cast and the view kernel) and a handle with a top
    view, each stepped beside a plain handle with the same bank: the state equal after every call, the learner view the reference's of the
    plain handle's descriptors, the top view the reference worlds'"""
    c, pu = dict(BC.CALLS, B=6), 8
    bank, weights = BC.three_layouts(6, 6), np.array([1, 2, 1], np.uint32)
    plain = BC.make_env(rcw, c)
    only = BC.make_env(rcw, c)
    top = BC.make_env(rcw, c, render_top_view=True, pu_per_tu=pu)
    ref = BC.make_ref(c)
    only.set_learner_view("rgb", (16, 16), "chw", camera_view=False)
    for e in (plain, only, top):
        e.set_wall_bank(bank, weights)
        e.set_time_limit(4)
    ref.set_wall_bank(bank, weights)

    def compare(where):
        for k in ("episode", "goal_position", "player_position_wu", "player_direction_au", "done", "tile_map_chunks", "episode_steps", "truncated"):
            for e, who in ((only, "view only"), (top, "top view")):
                np.testing.assert_array_equal(getattr(e.world, k), getattr(plain.world, k), err_msg=f"{k} of the {who} handle, {where}")
        for e in (only, top):
            np.testing.assert_array_equal(e.wall_layout.numpy(), plain.wall_layout.numpy(), err_msg=f"wall_layout {where}")
        h, cc = plain.columns()
        np.testing.assert_array_equal(only.learner_view_host(), LV.from_descriptors(h, cc, plain.cfg, c["Hc"], "rgb", (16, 16)), err_msg=f"view {where}")
        np.testing.assert_array_equal(top.camera_view_host(), plain.camera_view_host(), err_msg=f"camera view {where}")

    import time_limit_ref as TL
    lim = TL.TimeLimitRef(ref, 4, c["seed"], True)
    compare("behind set_wall_bank")
    np.testing.assert_array_equal(top.top_view_host(), ref.top_view(pu), err_msg="top view behind set_wall_bank")
    rng = np.random.default_rng(6)
    for t in range(14):
        a = WR.draw_actions(rng, c["B"])
        for e in (plain, only, top):
            rcw.act_(e, a)
        lim.step(a)
        compare(f"step {t}")
        np.testing.assert_array_equal(top.top_view_host(), ref.top_view(pu), err_msg=f"top view, step {t}")
    WB.assert_equal(plain, ref, "the plain handle behind the rollout")
    assert ref.events["layout_changed"] > 0 and lim.events["restarts_after_truncation"] > 0
    for e in (plain, only, top):
        e.close()


# ---- the call rules and hostile arguments ------------------------------------------------------------------------------------------------
def engine_state(env):
    w = env.world
    h, c = env.columns()
    s = dict(frame=env.camera_view_host(), col_h=h, col_c=c, tile_map=w.tile_map_chunks, goal=w.goal_position, position=w.player_position_wu,
             heading=w.player_direction_au, reward=w.reward, done=w.done, episode=w.episode, status=w.status, episode_steps=w.episode_steps,
             truncated=w.truncated)
    if env.wall_bank_info["layouts"]:
        s["wall_layout"] = env.wall_layout.numpy()
    return s


def test_refusals_leave_the_handle_byte_identical(rcw):
    from raycastworlds_jl_amd import _capi

    c = BC.CALLS
    env = BC.make_env(rcw, c)
    bank = BC.three_layouts(6, 6)
    lib, h = env._lib, env._h
    # without a bank: the getters and the weights are refused, switching off is fine
    out = np.zeros(c["B"], np.int32)
    p = C.c_void_p()
    assert lib.rcw_wall_layout(h, out.ctypes.data_as(C.c_void_p)) == _capi.RCW_ERR_UNSUPPORTED
    assert lib.rcw_wall_layout_device_ptr(h, C.byref(p)) == _capi.RCW_ERR_UNSUPPORTED
    assert lib.rcw_set_wall_bank_weights(h, None) == _capi.RCW_ERR_UNSUPPORTED
    assert env.wall_bank_info == {"layouts": 0, "total_weight": 0}
    env.set_wall_bank(None)
    env.set_wall_bank(bank, [1, 0, 3])
    assert env.wall_bank_info == {"layouts": 3, "total_weight": 4}
    rcw.act_(env, np.ones(c["B"], np.uint8))
    before, info, ptr = engine_state(env), env.wall_bank_info, env.wall_layout.ptr
    open_ring = bank.copy(); open_ring[1, 0, 3] = False
    full = bank.copy(); full[2, 1:-1, 1:-1] = True; full[2, 1, 1] = False
    flat = np.ascontiguousarray(bank.transpose(0, 2, 1), dtype=np.uint8)
    for bad, exc, message in (
            (lambda: env.set_wall_bank(open_ring), ValueError, r"layout 1: ring tile \(1,4\)"),
            (lambda: env.set_wall_bank(full), ValueError, "layout 2: 1 free interior tile"),
            (lambda: env.set_wall_bank(bank, [0, 0, 0]), ValueError, "sum to zero"),
            (lambda: env.set_wall_bank(bank, [0xFFFFFFFF, 0, 1]), ValueError, "more than 2\\^32 - 1"),
            (lambda: env.set_wall_bank_weights([0, 0, 0]), ValueError, "sum to zero"),
            (lambda: env.set_wall_bank_weights([0xFFFFFFFF, 1, 0]), ValueError, "more than 2\\^32 - 1"),
            (lambda: env.set_wall_bank_weights([1, 2]), ValueError, "3 integers"),
            (lambda: env.set_wall_bank(bank, [1, -1, 1]), ValueError, "3 integers"),
            (lambda: env._check(lib.rcw_set_wall_bank(h, flat.ctypes.data_as(C.c_void_p), -1, None)), ValueError, "layouts must be >= 0"),
            (lambda: env.set_walls(bank[0]), _capi.RcwError, "switch the bank off first"),
            (lambda: rcw.reset_(env, rng=np.random.default_rng(1)), ValueError, "wall bank")):
        with pytest.raises(exc, match=message) as ei:
            bad()
        if exc is _capi.RcwError:
            assert ei.value.code == _capi.RCW_ERR_UNSUPPORTED
        after = engine_state(env)
        for k in before:
            np.testing.assert_array_equal(after[k], before[k], err_msg=f"{k} behind {message}")
        assert env.wall_bank_info == info and env.wall_layout.ptr == ptr
    # ... and the refused weights did not replace the old ones: a full reset still never draws layout 1
    rcw.reset_(env, seed=3)
    assert set(env.wall_layout.numpy().tolist()) <= {0, 2}
    # an environment built with rng takes no bank
    with pytest.raises(ValueError, match="rng"):
        BC.make_env(rcw, dict(c, B=2), rng=np.random.default_rng(0), wall_bank=bank)
    with pytest.raises(ValueError, match="needs wall_bank"):
        BC.make_env(rcw, dict(c, B=2), wall_bank_weights=[1, 2, 3])
    env.close()


def test_calls_that_do_nothing_to_the_bank(rcw):
    """set_direction_table, set_time_limit, set_step_form, the feature switches and the getters: layouts, counters and walls stay; the weights
    call moves nothing either, and `walls` reads the bank's layouts back"""
    c = BC.CALLS
    bank = BC.three_layouts(6, 6)
    env = BC.make_env(rcw, c, wall_bank=bank, wall_bank_weights=[1, 1, 1])
    keep = lambda: (env.wall_layout.numpy().copy(), env.world.episode.copy(), env.world.tile_map_chunks.copy())
    before = keep()
    np.testing.assert_array_equal(env.world.walls, bank[before[0]])
    t = env.wall_layout.torch(sync=False)
    assert t.dtype.is_floating_point is False and tuple(t.shape) == (c["B"],)
    env.sync()
    np.testing.assert_array_equal(t.cpu().numpy(), before[0])
    for call in (lambda: env.set_direction_table(env.world.directions_wu[::-1].copy()), lambda: env.set_time_limit(7), lambda: env.set_step_form("one-launch"),
                 lambda: env.set_step_form("two-launches"), lambda: env.set_goal_distance(True), lambda: env.set_seen_map(True),
                 lambda: env.set_local_map(5), lambda: env.set_learner_view("gray", (8, 8)), lambda: env.set_wall_bank_weights([5, 0, 0]),
                 lambda: env.clear_error(), lambda: rcw.cast_rays_(env), lambda: rcw.update_camera_view_(env)):
        call()
        for got, want in zip(keep(), before):
            np.testing.assert_array_equal(got, want)
    rcw.reset_(env)                                                          # the new weights hold from the next episode start
    assert not env.wall_layout.numpy().any() and (env.world.episode == before[1] + 1).all()
    env.close()


# ---- the graph, the shards, the fuzzer ---------------------------------------------------------------------------------------------------
def test_a_captured_step_replayed_12_times_under_limit_3(rcw):
    torch = pytest.importorskip("torch")
    c = dict(BC.CALLS, B=12)
    bank, weights = BC.three_layouts(6, 6), np.array([1, 2, 1], np.uint32)
    env = BC.make_env(rcw, c, wall_bank=bank, wall_bank_weights=weights, max_episode_steps=3, goal_distance=True)
    ref = BC.make_ref(c)
    import time_limit_ref as TL
    ref.set_wall_bank(bank, weights)
    lim = TL.TimeLimitRef(ref, 3, c["seed"], True)
    gd = GoalTracker(rcw, env)
    stream = torch.cuda.Stream()
    env.sync()
    env.set_stream(stream.cuda_stream)
    a_host = np.ones(c["B"], np.uint8)                                       # forward: the same action in every replay
    with torch.cuda.stream(stream):
        actions = torch.from_numpy(a_host).cuda()
        stream.synchronize()
        ptr = env.wall_layout.ptr
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            rcw.act_(env, actions)                                           # (captured, not run)
        for k in range(12):
            g.replay()
            stream.synchronize()
            lim.step(a_host)
            WB.assert_equal(env, ref, f"replay {k}")
            np.testing.assert_array_equal(env.world.episode_steps, lim.episode_steps, err_msg=f"episode_steps, replay {k}")
            gd.stepped(a_host, f"replay {k}")
        assert env.wall_layout.ptr == ptr
        stream.synchronize()
    assert ref.events["layout_changed"] > 0 and ref.events["layout_kept"] > 0 and lim.events["restarts_after_truncation"] >= 2 * c["B"]
    del g
    env.close()


def test_two_shards_equal_their_slices_of_the_whole_batch(rcw):
    G, WORLD = 16, 2
    kw = dict(seed=5, auto_reset=True, height_tile_map_tu=9, width_tile_map_tu=9, num_rays=33, height_camera_view_pu=24, num_directions=8,
              position_increment_wu=0.25, player_radius_wu=0.3)
    bank, weights = BC.mazes(9, 9, 5, 60), np.array([1, 3, 0, 2, 2], np.uint32)
    whole = rcw.SingleRoomModule.SingleRoom(batch=G, wall_bank=bank, wall_bank_weights=weights, max_episode_steps=4, **kw)
    shards = [rcw.ShardedSingleRoom(G, rank=r, world=WORLD, device=0, **kw) for r in range(WORLD)]
    for sh in shards:
        sh.set_wall_bank(bank, weights)
        sh.env.set_time_limit(4)

    def compare(where):
        for sh in shards:
            sl = slice(sh.first, sh.first + sh.count)
            np.testing.assert_array_equal(sh.env.wall_layout.numpy(), whole.wall_layout.numpy()[sl], err_msg=f"wall_layout {where}")
            for k in ("episode", "goal_position", "player_position_wu", "player_direction_au", "done", "tile_map_chunks", "truncated"):
                np.testing.assert_array_equal(getattr(sh.env.world, k), getattr(whole.world, k)[sl], err_msg=f"{k} {where}")
            np.testing.assert_array_equal(sh.env.camera_view_host(), whole.camera_view_host()[sl], err_msg=f"camera view {where}")

    compare("installed")
    rng = np.random.default_rng(3)
    moved = whole.world.episode.copy()
    for k in range(12):
        a = WR.draw_actions(rng, G)
        rcw.act_(whole, a)
        for sh in shards:
            sh.act_(sh.local_slice(a))
        compare(f"step {k}")
    assert (whole.world.episode > moved).all() and len(set(whole.wall_layout.numpy().tolist())) > 1
    shards[0].set_wall_bank_weights([0, 0, 0, 0, 1]); shards[1].set_wall_bank_weights([0, 0, 0, 0, 1]); whole.set_wall_bank_weights([0, 0, 0, 0, 1])
    rcw.reset_(whole, seed=8)
    for sh in shards:
        sh.reset_(seed=8)
    compare("behind new weights and a reset")
    assert (whole.wall_layout.numpy() == 4).all()
    for sh in shards:
        sh.env.close()
    whole.close()


def test_random_banks_and_call_sequences_stay_in_parity():
    """tools/fuzz_parity.py bank: maps of 3 x 4 to 40 x 40, banks of 1 to 70 layouts, 30 random calls each, totals printed"""
    res = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tools", "fuzz_parity.py"), "16", "71", "bank"],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert "16 random configurations" in res.stdout and ", 0 mismatches" in res.stdout
    closing = res.stdout.strip().splitlines()[-1]
    print(closing)
    totals = {k: int(v) for v, k in re.findall(r"(\d+) ([a-z_0-9]+)\b", closing[closing.index("wall bank:"):closing.rindex(")")])}
    for k in ("step", "reset", "masked_reset", "set_state", "weights", "off_and_on", "episode_starts", "layout_changed", "layout_kept", "goal_redraws",
              "restarts_after_done", "restarts_after_truncation", "one_launch_steps", "two_launch_steps", "words_not_multiple_of_4", "banks_past_64"):
        assert totals[k] > 0, closing
