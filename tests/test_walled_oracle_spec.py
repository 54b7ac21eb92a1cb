"""The fast walled reference (tests/walled_oracle.py: the C oracle plus the layout-source rule) anchored to the reviewed Python ones, on
the CPU: for a scenario each of the wall bank, the mazes, the caves and the rooms — at their own small shapes, with a time limit on in
all four, the bank's and the families' `calls` scenarios with every call the rule has a clause for (masked reset_ under a new seed,
masked set_state, new weights, the source off and on again, set_walls in between), one in Float64 — the scenarios' Recorder on a
WalledOracle reproduces the Python Recorder's snapshots byte for byte, call by call: every array WallsRef compares, wall_layout, and the
time limit's two words.  With tests/test_oracle_walls.py (the C against WallsRef) this is what ties the GPU tests at the real frame
shapes (tests/test_gpu_walls_full_shapes.py) to the references that were reviewed line by line.
"""
import numpy as np
import pytest

import time_limit_ref as TL
import wall_bank_cases as BC
import wall_family as WF
import walled_oracle as WO
from test_oracle_walls import ARRAYS, assert_snapshots_equal

ANCHORS = [("bank", "calls"), ("generator", "calls"), ("caves", "tie64"), ("caves", "calls"), ("rooms", "calls"), ("rooms", "square")]


@pytest.mark.parametrize("kind,name", ANCHORS, ids=[f"{k}-{n}" for k, n in ANCHORS])
def test_the_scenario_on_the_fast_reference_is_the_python_recording(rcw, oracle, kind, name):
    want, events = BC.recorded(name) if kind == "bank" else WF.recorded(kind, name)
    got, fast_events = WO.recorded(kind, name)
    assert len(got) == len(want)
    limited = 0
    for k, (g, w) in enumerate(zip(got, want)):
        where = f"{kind} / {name}, call {k}"
        assert w.get("rendered", True)
        assert_snapshots_equal(g, w, where, ARRAYS + ("wall_layout",))
        flag = "bank" if kind == "bank" else kind
        assert g[flag] == w[flag], where
        assert ("episode_steps" in g) == ("episode_steps" in w), where
        if "episode_steps" in w:
            limited += 1
            assert_snapshots_equal(g, w, where, ("episode_steps", "truncated"))
    assert limited > 0 and events["truncations"] > 0 and events["restarts_after_truncation"] > 0 and events["restarts_after_done"] + events["terminations"] > 0, events
    shared = ("interior_wall_ray_hits", "blocked_next_to_interior_wall", "goal_redraws", "restarts_after_done", "episode_starts", "truncations",
              "restarts_after_truncation", "terminations")
    assert {k: fast_events[k] for k in shared} == {k: events[k] for k in shared}
    made = "layouts_drawn" if kind == "bank" else WF.FAMILIES[kind].made
    assert fast_events[made] == events[made] and len(events[made]) >= 1


def test_the_time_limit_wraps_it_as_it_wraps_the_reference_worlds(rcw, oracle):
    """no source: TimeLimitRef(WalledOracle) against TimeLimitRef(WallsRef) on the 6 x 6 layouts, limit 3, invalid actions in between"""
    import test_gpu_walls as GW

    c = dict(GW.ROOMS, N=24, Hc=20, B=12)
    walls, index = GW.three_layouts(6, 6), (np.arange(12) % 3).astype(np.int32)
    ref, orc = GW.make_ref(c), WO.from_case(c)
    ref.set_walls(walls, index); orc.set_walls(walls, index)
    a, b = TL.TimeLimitRef(ref, 3, c["seed"], True), TL.TimeLimitRef(orc, 3, c["seed"], True)
    rng = np.random.default_rng(1)
    for t in range(30):
        act = TL.draw_actions(rng, 12, t, bad_every=4)
        a.step(act); b.step(act)
        assert_snapshots_equal(orc.snapshot(), ref.snapshot(), f"step {t}")
        np.testing.assert_array_equal(a.episode_steps, b.episode_steps); np.testing.assert_array_equal(a.truncated, b.truncated)
        ref.clear_status(); orc.clear_status()
    assert a.events == b.events and a.events["restarts_after_truncation"] > 0 and a.events["invalid_while_truncated"] + a.events["truncations"] > 0
    assert {k: orc.events[k] for k in ref.events} == ref.events
