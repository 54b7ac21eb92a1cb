"""tests/deferred.py on the CPU: the Script driver records a scenario faithfully, the comparison names the first difference, the weights
scenario reaches what tests/test_gpu_deferred.py claims of it — from the reference alone —, and the table of waiting calls covers every
export the drivers' methods reach in single_room.py."""
import inspect
import os
import re

import numpy as np
import pytest

import deferred as D
import wall_bank_cases as BC
import wall_caves_cases as CC
import wall_generator_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = dict(bank=BC, generator=GC, caves=CC)
EVERY_SCENARIO = [(family, name) for family, cases in CASES.items() for name in cases.SCENARIOS]


@pytest.mark.parametrize("family,name", EVERY_SCENARIO, ids=[f"{f}-{n}" for f, n in EVERY_SCENARIO])
def test_a_replayed_script_reproduces_the_recording(family, name):
    """the calls a Script kept, made again on a fresh Recorder, leave the snapshots of `recorded(name)` (dynamics, walls, layouts, counters;
    the rehearsal's recordings carry no frames), and the steps' actions come out as one array"""
    cases = CASES[family]
    fn, c = cases.SCENARIOS[name]
    script = D.script_of(cases, name)
    want, _ = cases.recorded(name, False)
    fresh = cases.Recorder(c, False)
    script.replay(fresh)
    assert len(fresh.snaps) == len(want) == len(script.calls) + 1
    for k, (g, w) in enumerate(zip(fresh.snaps, want)):
        assert g.keys() == w.keys()
        for key in w:
            np.testing.assert_array_equal(g[key], w[key], err_msg=f"{name}, snapshot {k}: {key}")
    steps = [args[0] for m, args, _ in script.calls if m == "step"]
    assert script.actions.shape == (len(steps), c["B"]) and script.actions.dtype == np.uint8
    for row, a in zip(script.actions, steps):
        np.testing.assert_array_equal(row, a)
    assert len(steps) > 0 and ((script.actions >= 1) & (script.actions <= 4)).all()


def test_a_script_keeps_its_own_copy_of_every_argument():
    class Quiet:
        B = 3

        def step(self, a):
            pass

    s = D.Script(Quiet())
    a = np.array([1, 2, 3], np.uint8)
    s.step(a)
    a[:] = 4
    s.step(a)
    np.testing.assert_array_equal(s.actions, [[1, 2, 3], [4, 4, 4]])
    with pytest.raises(AttributeError):
        s.numpy


def _records(n):
    rng = np.random.default_rng(3)
    return [dict(camera_view=rng.integers(0, 2 ** 32, (3, 4, 5), dtype=np.uint32), reward=rng.random(3, np.float32), done=np.zeros(3, np.uint8),
                 wall_layout=rng.integers(0, 3, 3).astype(np.int32)) for _ in range(n)]


@pytest.mark.parametrize("k,name", [(0, "camera_view"), (3, "reward"), (6, "wall_layout"), (6, "done")])
def test_one_changed_byte_is_reported_with_its_call_and_array(k, name):
    calls = [("step", (np.ones(3, np.uint8),), {})] * 3 + [("set_weights", (np.array([1, 2], np.uint32),), {})] + [("reset", (None,), dict(seed=9))] * 3
    want = _records(7)
    got = [{key: v.copy() for key, v in r.items()} for r in want]
    assert D.first_difference(got, want, calls) is None
    D.assert_records_equal(got, want, calls, "equal")
    got[k][name].view(np.uint8).reshape(-1)[-1] ^= 1
    for later in range(k + 1, 7):                                             # a later difference does not hide the first
        got[later]["reward"][0] += 1
    at, call, array = D.first_difference(got, want, calls)
    assert (at, array) == (k, name) and call.startswith(calls[k][0] + "(")
    with pytest.raises(AssertionError, match=rf"call {k}, {re.escape(call)}: {name} \(1 of"):
        D.assert_records_equal(got, want, calls, "changed")


def test_a_missing_copy_a_shape_and_a_type_are_differences():
    calls = [("step", (np.ones(3, np.uint8),), {})] * 2
    want = _records(2)
    for spoil in (lambda r: r.pop("done"), lambda r: r.update(done=r["done"][:2]), lambda r: r.update(done=r["done"].astype(np.int8))):
        got = [{key: v.copy() for key, v in r.items()} for r in want]
        spoil(got[1])
        d = D.first_difference(got, want, calls)
        assert d is not None and d[0] == 1 and d[2].startswith("done")


def test_every_weight_vector_sees_restarts_in_the_weights_scenario():
    """limit 1: a step cuts every episode and the next one restarts it, so every second step starts B episodes — under the vector queued in
    front of THAT step: vectors 1, 3, 5, ... of the twelve, each of the three twice, and each draws its own layout alone"""
    script, snaps, events = D.weights_recording(False)
    assert [m for m, _, _ in script.calls] == ["set_wall_bank", "set_time_limit"] + ["set_weights", "step"] * D.WEIGHT_STEPS
    by = D.restarts_by_vector(script.calls, snaps)
    assert set(by) == set(D.WEIGHT_VECTORS)
    B = script.B
    for layout, vector in enumerate(D.WEIGHT_VECTORS):
        starts, drew = by[vector]
        assert starts == 2 * B and drew == {layout}, (vector, starts, drew)
    assert events["restarts_after_truncation"] + events["restarts_after_done"] == 6 * B and events["layout_changed"] > 0
    # ... and the plan: the backlog in front of the first set_weights, the pending check in front of the second (one pinned buffer)
    assert D.plan_backlog(script.calls, "host") == (1, 4) and D.plan_backlog(script.calls, "device") == (1, 4)


def test_the_backlog_plan_of_the_scenarios():
    """where the backlog goes and where its event must still be pending: behind the waiting call that installs bank, generator or caves; in
    front of the third host-action step (the ring is two deep), or behind the last call where actions stay on the device"""
    for cases in (BC, GC, CC):
        calls = D.script_of(cases, "features").calls
        assert calls[0][0] in ("set_wall_bank", "set_wall_generator", "set_wall_caves") and calls[1][0] == "set_time_limit"
        start, check = D.plan_backlog(calls, "host")
        assert start == 1 and [m for m, _, _ in calls[start:check]] == ["set_time_limit", "step", "step"] and calls[check][0] == "step"
        start, check = D.plan_backlog(calls, "device")
        waits = [k for k, call in enumerate(calls) if call[0] in ("set_state", "set_walls")]
        assert start == 1 and check == (waits[0] if waits else len(calls))
    calls = D.script_of(BC, "big").calls                                      # ... set_weights once between the steps: one call ahead, no wait
    assert [m for m, _, _ in calls].count("set_weights") == 1 and D.plan_backlog(calls, "device") == (1, len(calls))
    calls = D.script_of(BC, "calls").calls                                    # set_time_limit | set_wall_bank (waits) | steps ...
    assert D.plan_backlog(calls, "host") == (2, 4) and calls[6][0] == "reset" and D.plan_backlog(calls, "device") == (2, 6)
    assert D.plan_backlog([("set_state", (), {}), ("set_time_limit", (3,), {})], "host") == (None, None)
    assert not D.may_wait("reset", (None, 77), {}, "host", ()) and D.may_wait("reset", (np.ones(2, np.uint8),), dict(seed=1), "host", ())


def test_the_waits_table_names_every_export_the_drivers_reach():
    import raycastworlds_jl_amd.single_room as SR

    reached = {}
    for method, names in D.DRIVER_METHODS.items():
        reached[method] = D.exports_reached(SR, names)
        assert reached[method], method
        silent = sorted(e for e in reached[method] if D.waits(e) is None)
        assert not silent, f"{method} reaches {silent}: tests/deferred.py and INTEGRATION.md \"Streams\" do not say whether they wait"
    assert {"rcw_step", "rcw_step_device"} <= reached["step"] and "rcw_reset" in reached["reset"]
    assert "rcw_set_wall_bank_weights" in reached["set_weights"] and "rcw_set_wall_caves" in reached["set_wall_caves"]
    # the drivers' methods are the Player's: every one of them exists there, and the Player has no other call
    for cases in (BC, GC, CC):
        public = {n for n, f in inspect.getmembers(cases.Player, inspect.isfunction) if not n.startswith("_")} - {"finished", "state"}
        assert public <= set(D.DRIVER_METHODS), public - set(D.DRIVER_METHODS)
    assert set(D.RENDER_METHODS.values()) <= set(D.WAITS) and not set(D.RENDER_METHODS) & set(D.DRIVER_METHODS)


def test_the_document_carries_the_table_word_for_word():
    """every row of WAITS with its own words for the rule (a `yes` where the ring's rule belongs is a difference) and with who holds it, the
    two classes a row each, and every export that is named exists"""
    header = open(os.path.join(ROOT, "include", "rcw.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    doc = doc[doc.index("## 4. Streams"):doc.index("## 5. Multi-GPU")]
    rows = dict((m.group(1), (m.group(2), m.group(3))) for m in re.finditer(r"^\s*\| `(rcw_\w+)` \| (.+?) \| (.+?) \|", doc, re.M))
    assert set(rows) == set(D.WAITS), set(rows) ^ set(D.WAITS)
    assert D.ASSERTED_ON_DEVICE <= set(D.WAITS) and len(set(D.CELL.values())) == len(D.CELL) == 5
    for export, rule in D.WAITS.items():
        assert rows[export] == (D.CELL[rule], "device" if export in D.ASSERTED_ON_DEVICE else "code"), (export, rule, rows[export])
    assert re.search(r"^\s*\| every copy-out \| yes \| code \|", doc, re.M)
    assert re.search(r"^\s*\| every `\*_device_ptr` and `\*_info` getter, `rcw_get_stream`, `rcw_time_limit`, `rcw_learner_view_stack` \| no \| code \|", doc, re.M)
    for export in set(D.WAITS) | D.HOST_ANSWERS | D.COPY_OUTS:
        assert re.search(rf"\b{export}\s*\(", header), export
    assert all(D.waits(e) == D.NEVER for e in D.HOST_ANSWERS | {"rcw_wall_bank_info", "rcw_obs_device_ptr"}) and all(D.waits(e) == D.ALWAYS for e in D.COPY_OUTS)
    assert D.waits("rcw_set_learner_view") is None


def test_the_device_rows_are_behind_the_backlog_in_some_script():
    """ASSERTED_ON_DEVICE, from the scripts tests/test_gpu_deferred.py runs: each of its exports is made between the backlog and the pending
    check of at least one of them"""
    import test_gpu_deferred as T

    held = set()
    scripts = [(D.script_of(cases, name).calls, mode) for family, name, mode in T.SCENARIO_RUNS for cases in [CASES[family]]]
    scripts += [(D.weights_recording(False)[0].calls, "host"), (T.render_calls(5, True), "device"), (T.render_calls(5, False), "device")]
    for calls, mode in scripts:
        start, check = D.plan_backlog(calls, mode)
        for method, args, kwargs in calls[start:check]:
            if method == "step":
                held.add("rcw_step" if mode == "host" else "rcw_step_device")
            elif method in D.RENDER_METHODS:
                held.add(D.RENDER_METHODS[method])
            else:
                held.add(dict(reset="rcw_reset", set_time_limit="rcw_set_time_limit", set_weights="rcw_set_wall_bank_weights")[method])
    assert held == D.ASSERTED_ON_DEVICE, held ^ D.ASSERTED_ON_DEVICE
