"""Queued calls that nobody reads between (tests/deferred.py): the scenarios of the wall bank, the generator and the caves, the action ring,
the weights' staging buffer and the top view's side stream, each replayed on an engine that is read ONCE, behind the last call, with a
backlog of queued device work in front so that the host really runs ahead of the device.

Expected values: an observed twin — a second handle played through the cases' own Player and the feature trackers, held after every call
to the plain references as tests/test_gpu_wall_bank.py holds it — whose host copies behind every call the unread handle must equal byte for
byte; the reference's own snapshots where they carry everything that is watched (the weights' staging); oracle.OracleBatch for the top view.

Every test also asserts rows of the table of calls that wait (deferred.WAITS; INTEGRATION.md "Streams"): in front of the first call of the
script that may wait — or behind the last call — the backlog's closing event has not completed.  The rows held this way are
deferred.ASSERTED_ON_DEVICE (tests/test_deferred_spec.py derives the set from the scripts run here): the scenarios reach rcw_step_device,
rcw_step two calls ahead, rcw_set_time_limit and rcw_set_wall_bank_weights one call ahead; test_the_other_calls_of_a_rollout_do_not_wait
adds the unmasked rcw_reset, rcw_bind_obs, rcw_update_camera_view, rcw_update_top_view, rcw_cast_rays, rcw_columns_device_ptr and
rcw_expand_columns.  Every other row is read from the code.  Measured margins: profiles/deferred_backlog.txt.
"""
import functools

import numpy as np
import pytest

import deferred as D
import local_map_ref as LM
import wall_bank_cases as BC
import wall_caves_cases as CC
import wall_generator_cases as GC

pytestmark = pytest.mark.gpu
CASES = dict(bank=BC, generator=GC, caves=CC)
EVERYTHING = ("goal_distance", "seen_map", "local_map", "learner_view")
NO_VIEW = ("goal_distance", "seen_map", "local_map")
STACK = dict(k=4, fmt="gray", size=(21, 21))


@pytest.fixture(scope="module", autouse=True)
def _give_the_backlog_buffer_back():
    """the 1 GiB the backlog fills goes back to the device behind this file: later tests measure what is free"""
    yield
    D.release_backlog()


# (family, scenario, action mode) of every scenario the file plays unread: what tests/test_deferred_spec.py derives the rows held on the device from
SCENARIO_RUNS = [("bank", "features", "host"), ("bank", "features", "device"), ("bank", "calls", "host"), ("bank", "big", "host"), ("bank", "big", "device"),
                 ("generator", "features", "device"), ("generator", "calls", "host"), ("caves", "features", "device"), ("bank", "small", "host")]


def check_report(report):
    """what every unread run ends on: the backlog was still running at the check, and it ended by itself in under a second (Deferred.run
    asserts BACKLOG_LIMIT_MS times the number of backlogs: the one rerun on a slow host queues four)"""
    print(report)
    assert report["pending"] is True and report["backlog_ms"] < D.BACKLOG_LIMIT_MS * report["backlogs"] and report["backlogs"] in (1, 4)


def enable(env, features):
    """the features on an engine nobody tracks, in the order and with the arguments the trackers switch them on"""
    if "goal_distance" in features:
        env.set_goal_distance(True)
    if "seen_map" in features:
        env.set_seen_map(True)
    if "local_map" in features:
        env.set_local_map(9, 2, LM.SEEN)
    if "learner_view" in features:
        env.set_learner_view(STACK["fmt"], STACK["size"], "chw", stack=STACK["k"])
    return env


def trackers_of(rcw, env, features):
    from test_gpu_wall_bank import GoalTracker, LocalTracker, SeenTracker, StackTracker

    t = []
    if "goal_distance" in features:
        t.append(GoalTracker(rcw, env))
    if "seen_map" in features:
        t.append(SeenTracker(rcw, env))
    if "local_map" in features:
        t.append(LocalTracker(rcw, env, 9, 2, LM.SEEN))
    if "learner_view" in features:
        t.append(StackTracker(env, STACK["k"], STACK["fmt"], STACK["size"]))
    return t


@functools.lru_cache(maxsize=None)
def twin(rcw, family, name, form, features):
    """the observed twin's records of a scenario, made once for every (form, features): (records, host state behind the last call, events)"""
    cases = CASES[family]
    env = cases.make_env(rcw, cases.SCENARIOS[name][1], form)
    try:
        return D.observed_twin(cases, rcw, name, env, trackers_of(rcw, env, features), features)
    finally:
        env.close()


def unread(rcw, family, name, form, features, mode, spy=None):
    cases = CASES[family]
    want, final, events = twin(rcw, family, name, form, features)
    script = D.script_of(cases, name)
    assert len(want) == len(script.calls)

    def make():
        env = enable(cases.make_env(rcw, cases.SCENARIOS[name][1], form), features)
        assert form is None or env.step_form() == form
        if spy is not None:                                                   # the mirror's two ways to StepFacts::columns_wanted, noted from here on
            for method in ("columns_device", "set_learner_view"):
                setattr(env, method, lambda *a, _m=method, _f=getattr(env, method), **k: (spy.append(_m), _f(*a, **k))[1])
            assert env.learner_view_info()["format"] is None
        return env

    report = D.run_unread(make, rcw, script, want, final, features, mode, name=f"{family} {name}, {form or 'auto'}")
    check_report(report)
    return report, events, script


# ---- the bank -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("form", ["two-launches", "one-launch"])
def test_the_bank_with_every_feature_on(rcw, form, mode):
    report, events, script = unread(rcw, "bank", "features", form, EVERYTHING, mode)
    assert events["layout_changed"] > 0 and events["restarts_after_done"] > 0 and events["restarts_after_truncation"] > 0
    assert report["checked_at"] == (len(script.calls) if mode == "device" else 4)      # host: in front of the third rcw_step


@pytest.mark.parametrize("form", ["two-launches", "one-launch"])
def test_the_banks_call_rules_with_host_actions(rcw, form):
    """waiting and non-waiting calls mixed: masked resets, set_state, new weights, the bank off, set_walls, the bank on again"""
    report, events, script = unread(rcw, "bank", "calls", form, (), "host")
    assert report["backlog_at"] == 2 and report["checked_at"] == 4


@pytest.mark.parametrize("mode", ["host", "device"])
def test_130_layouts_and_new_weights_between_the_steps(rcw, mode):
    report, events, script = unread(rcw, "bank", "big", None, (), mode)
    assert max(events["layouts_drawn"]) >= 64 and [m for m, _, _ in script.calls].count("set_weights") == 1
    assert report["checked_at"] == (len(script.calls) if mode == "device" else 4)      # device: across set_wall_bank_weights, one call ahead


# ---- the generator and the caves ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["two-launches", "one-launch"])
def test_the_generator_with_every_feature_on(rcw, form):
    report, events, script = unread(rcw, "generator", "features", form, EVERYTHING, "device")
    assert events["restarts_after_done"] > 0 and events["restarts_after_truncation"] > 0 and events["goal_redraws"] > 0
    assert report["checked_at"] == len(script.calls)


def test_the_generators_call_rules_in_the_one_launch_form(rcw):
    report, events, script = unread(rcw, "generator", "calls", "one-launch", (), "host")
    assert report["backlog_at"] == 2 and report["checked_at"] == 4


@pytest.mark.parametrize("form", ["two-launches", "one-launch"])
def test_the_caves_with_every_feature_on(rcw, form):
    report, events, script = unread(rcw, "caves", "features", form, EVERYTHING, "device")
    assert events["restarts_after_done"] > 0 and events["restarts_after_truncation"] > 0
    assert script.calls[report["checked_at"]][0] == "set_state"                         # (walk_into_the_goal: the first call that waits)


# ---- columns nobody wanted ----------------------------------------------------------------------------------------------------------------
def test_columns_nobody_wanted(rcw):
    """the one-launch step on a handle that never handed out its descriptors and has no learner view: every step leaves them stale, the bank
    rewrites tile maps behind it, the features follow — and the ONE rcw_columns at the very end recasts what the reference's last call left"""
    asked = []
    report, events, script = unread(rcw, "bank", "features", "one-launch", NO_VIEW, "device", spy=asked)
    assert asked == [], asked                                                 # nobody reached rcw_columns_device_ptr or switched a learner view on
    want, final, _ = twin(rcw, "bank", "features", "one-launch", NO_VIEW)
    last = BC.recorded("features")[0][-1]
    np.testing.assert_array_equal(final["col_height"], last["col_height"])
    np.testing.assert_array_equal(final["col_colour"], last["col_colour"])
    assert events["layout_changed"] > 0


# ---- the action ring ----------------------------------------------------------------------------------------------------------------------
def test_thirty_host_action_steps_through_the_ring_of_two(rcw):
    """67 agents, 30 steps, every step's actions its own: were a pinned buffer rewritten before its copy ran — the backlog holds the first
    two copies back while the host queues on —, an earlier step would move by a later step's actions"""
    report, events, script = unread(rcw, "bank", "small", None, (), "host")
    assert script.actions.shape == (30, 67) and len({row.tobytes() for row in script.actions}) == 30
    assert report["backlog_at"] == 1 and report["checked_at"] == 4 and events["episode_starts"] > 67


# ---- the weights' staging -----------------------------------------------------------------------------------------------------------------
def final_of_snapshot(s):
    pos = s["position"]
    return dict(status=s["status"], episode=s["episode"], goal=s["goal"], position_bits=pos.view(np.uint64 if pos.dtype == np.float64 else np.uint32),
                heading=s["direction"], tile_map_chunks=s["tile_map_chunks"], col_height=s["col_height"], col_colour=s["col_colour"])


@pytest.mark.parametrize("mode", ["host", "device"])
def test_twelve_weight_vectors_through_one_pinned_buffer(rcw, mode):
    """against WallBankRef under TimeLimitRef alone: every restart draws under the vector queued in front of its step"""
    script, snaps, events = D.weights_recording(True)
    by = D.restarts_by_vector(script.calls, snaps)
    for layout, vector in enumerate(D.WEIGHT_VECTORS):                        # (rehearsed in tests/test_deferred_spec.py)
        assert by[vector][0] > 0 and by[vector][1] == {layout}
    want = D.records_of_snapshots(snaps)
    assert all("wall_layout" in r and "camera_view" in r for r in want) and all("truncated" in r for r in want[1:])   # (the limit: from call 1)
    report = D.run_unread(lambda: BC.make_env(rcw, BC.CALLS), rcw, script, want, final_of_snapshot(snaps[-1]), (), mode, name="the weights' staging")
    check_report(report)
    assert (report["backlog_at"], report["checked_at"]) == (1, 4)


# ---- the top view's side stream, and the calls of a rollout that no scenario makes ---------------------------------------------------------
TOP = dict(height_tile_map_tu=8, width_tile_map_tu=8, num_rays=40, height_camera_view_pu=32, render_top_view=True, pu_per_tu=12, out_of_bounds=1)
PLAIN = dict(height_tile_map_tu=8, width_tile_map_tu=8, num_rays=64, height_camera_view_pu=64, out_of_bounds=1)      # takes the one-launch step


def oracle_records(oracle, calls, batch, seed, kw):
    """the oracle's own records of a script of steps, unmasked resets and RENDER_METHODS (which move nothing: the record before stands;
    `expanded`: the descriptors' frames are the camera view's), and its state behind the last call"""
    orc = oracle.OracleBatch(batch, seed=seed, auto_reset=1, **kw)
    try:
        want = []
        for method, args, kwargs in calls:
            if method == "step":
                assert orc.step(args[0]) == 0
            elif method == "reset":
                orc.reset(mask=None, seed=kwargs["seed"])
            else:
                assert method in D.RENDER_METHODS
            r = dict(camera_view=orc.camera_view.copy(), reward=orc.reward.copy(), done=orc.done.copy())
            if kw.get("render_top_view"):
                r["top_view"] = orc.top_view.copy()
            if method == "expand_columns":
                r["expanded"] = r["camera_view"]
            want.append(r)
        final = dict(status=orc.status.copy(), episode=orc.episode.copy(), goal=orc.goal.copy(), position_bits=orc.position.view(np.uint32).copy(),
                     heading=orc.direction.copy(), tile_map_chunks=orc.tile_map_chunks(), col_height=orc.col_height.copy(), col_colour=orc.col_colour.copy())
        return want, final
    finally:
        orc.close()


@pytest.mark.parametrize("runs", [1, 8])
@pytest.mark.parametrize("batch", [5, 64])
def test_the_two_kernel_top_view_behind_a_backlog(rcw, oracle, batch, runs):
    """20 device-action steps, fork and join with the side stream in every one of them, none read: top view and camera view of every step
    against the oracle's"""
    actions = np.random.default_rng(7).integers(1, 5, (20, batch)).astype(np.uint8)
    script = D.Steps(actions)
    want, final = oracle_records(oracle, script.calls, batch, 12, TOP)
    assert len({r["top_view"].tobytes() for r in want}) > 10

    def make():
        env = rcw.SingleRoomModule.SingleRoom(batch=batch, seed=12, auto_reset=True, **TOP)
        env.set_top_view_form("two-kernels", runs)
        assert env.top_view_form() == "two-kernels" and env.fill_kernel_name() != "rcw_fill256_draw_kernel"     # (not the fused launch: a fork every step)
        return env

    report = D.run_unread(make, rcw, script, want, final, ("top_view",), "device", name=f"top view, {batch} agents, {runs} runs")
    check_report(report)
    assert report["checked_at"] == 20


def render_calls(batch, top):
    """steps with, between them, the calls of a rollout that no scenario makes — all of them rows the table marks as not waiting: an unmasked
    reset with a new seed, rcw_update_camera_view, rcw_cast_rays, rcw_bind_obs, and with a top view rcw_update_top_view; without one (the
    one-launch step: the descriptors are stale from the second step on) rcw_columns_device_ptr and rcw_expand_columns of what it hands out"""
    rng = np.random.default_rng(8)
    step = lambda: ("step", (rng.integers(1, 5, batch).astype(np.uint8),), {})
    call = lambda m: (m, (), {})
    calls = [step(), step(), step(), call("update_camera_view"), step(), ("reset", (None,), dict(seed=21)), step(), call("cast_rays"), step(),
             call("bind_obs"), step(), step()]
    if top:
        calls += [call("update_top_view"), step(), call("cast_rays"), call("update_top_view"), call("update_camera_view")]
    else:
        calls += [call("columns_device"), call("expand_columns"), step(), call("expand_columns"), ("reset", (None,), dict(seed=22)), call("expand_columns")]
    return calls + [step(), step()]


@pytest.mark.parametrize("top", [True, False], ids=["top view", "one-launch"])
def test_the_other_calls_of_a_rollout_do_not_wait(rcw, oracle, top):
    """every call of render_calls behind the backlog, device actions, the closing event pending behind the last one; every copy against
    the oracle, which these calls — the resets apart — leave where it is"""
    batch, kw = (5, TOP) if top else (67, PLAIN)
    script = D.Calls(render_calls(batch, top), batch)
    want, final = oracle_records(oracle, script.calls, batch, 12, kw)
    assert D.plan_backlog(script.calls, "device") == (0, len(script.calls))

    def make():
        env = rcw.SingleRoomModule.SingleRoom(batch=batch, seed=12, auto_reset=True, **kw)
        if top:
            env.set_top_view_form("two-kernels", 1)
            assert env.top_view_form() == "two-kernels"
        else:
            env.set_step_form("one-launch")
            assert env.step_form() == "one-launch"
        return env

    report = D.run_unread(make, rcw, script, want, final, ("top_view",) if top else (), "device", name=f"the other calls, {'top view' if top else 'one-launch'}")
    check_report(report)
    assert report["checked_at"] == len(script.calls)
