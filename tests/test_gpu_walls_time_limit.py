"""Interior walls under the episode time limit on the GPU ("an unreachable goal is what the time limit is for"): set_walls, then
set_time_limit(L), then every step of a rollout against tests/time_limit_ref.py composed over tests/walls_ref.py — TimeLimitRef(WallsRef), no
second reference; tests/test_walls_spec.py anchors that composition to the C oracle on a ring-only map — byte for byte: everything
tests/test_gpu_walls.py compares, and episode_steps and truncated.

The cases, layouts and engines are test_gpu_walls.py's.  What the limit adds on a walled map is the goal redraw loop inside a restart that a
TRUNCATION asked for — reset_agent under `resample`, and in the one-launch form reset_preview under `reborn`, both in the *_limit_kernel
twins — counted here as goal_redraws_on_truncation_restarts: the growth of the reference's goal_redraws over the steps in which agents
restarted after a truncation and none after `done`.  Rehearsed on the CPU (rollout(name, render=False)):

    rollout   L   steps   forms        truncations   restarts_after_truncation   restarts_after_done   goal_redraws_on_truncation_restarts
    ROOMS     5   30      both         72            72                          11                    12
    WIDE      4   30      one-launch   86            86                          12                     4
    MAZE      3   12      auto         24            24                           0                    20
    F64       5   30      flat fill    73            73                           7                    16
"""
import functools

import numpy as np
import pytest

import time_limit_ref as TL
import walls_ref as WR
from test_gpu_walls import CASES, make_env, make_ref, walls_of

pytestmark = pytest.mark.gpu

LIMITS = dict(ROOMS=(5, 30), WIDE=(4, 30), MAZE=(3, 12), F64=(5, 30))       # (L, steps)
REHEARSED = dict(ROOMS=(72, 72, 11, 12), WIDE=(86, 86, 12, 4), MAZE=(24, 24, 0, 20), F64=(73, 73, 7, 16))
COLUMNS = ("truncations", "restarts_after_truncation", "restarts_after_done", "goal_redraws_on_truncation_restarts")


def snapshot(ref, lim):
    return dict(ref.snapshot(), episode_steps=lim.episode_steps.copy(), truncated=lim.truncated.copy())


@functools.lru_cache(maxsize=None)
def rollout(name, render=True):
    """the reference's rollout, computed once and shared by the forms of the engine: (a snapshot behind set_walls and behind every step,
    the actions, the event counts of both helpers and the redraws on truncation restarts)"""
    c = CASES[name]
    L, steps = LIMITS[name]
    walls, index = walls_of(name)
    ref = make_ref(c, render=render)
    ref.set_walls(walls, index)
    lim = TL.TimeLimitRef(ref, L, c["seed"], True)
    rng = np.random.default_rng(c["seed"] + 1)
    snaps, actions, on_truncation = [snapshot(ref, lim)], [], 0
    for _ in range(steps):
        a = WR.draw_actions(rng, c["B"])
        redraws, after_t, after_d = ref.events["goal_redraws"], lim.events["restarts_after_truncation"], lim.events["restarts_after_done"]
        lim.step(a)
        if lim.events["restarts_after_truncation"] > after_t and lim.events["restarts_after_done"] == after_d:
            on_truncation += ref.events["goal_redraws"] - redraws
        actions.append(a); snaps.append(snapshot(ref, lim))
    assert ref.events["restarts_after_done"] == lim.events["restarts_after_done"]
    return snaps, actions, dict(ref.events, **lim.events, goal_redraws_on_truncation_restarts=on_truncation)


def assert_equal(env, snap, where):
    WR.assert_equal(env, snap, where)
    np.testing.assert_array_equal(env.world.episode_steps, snap["episode_steps"], err_msg=f"episode_steps {where}")
    np.testing.assert_array_equal(env.world.truncated.astype(np.uint8), snap["truncated"], err_msg=f"truncated {where}")


ROLLOUTS = [("ROOMS", "two-launches"), ("ROOMS", "one-launch"), ("WIDE", "one-launch"), ("MAZE", None), ("F64", None)]


@pytest.mark.parametrize("name,form", ROLLOUTS, ids=[f"{n}-{f or 'auto'}" for n, f in ROLLOUTS])
def test_a_limited_rollout_on_a_walled_map(rcw, name, form):
    c = CASES[name]
    L, _ = LIMITS[name]
    snaps, actions, events = rollout(name)
    assert tuple(events[k] for k in COLUMNS) == REHEARSED[name], events
    assert all(events[k] > 0 for k in COLUMNS if not (name == "MAZE" and k == "restarts_after_done")), events
    walls, index = walls_of(name)
    env = make_env(rcw, c, form)
    if name == "F64":
        assert env.step_form() == "two-launches" and env.fill_kernel_name() == "rcw_fill_flat_kernel"
    env.set_walls(walls, index)
    env.set_time_limit(L)
    assert env.time_limit == L
    assert_equal(env, snaps[0], f"{name}: behind set_walls and set_time_limit")
    for t, a in enumerate(actions):
        rcw.act_(env, a)
        assert_equal(env, snaps[t + 1], f"{name} ({form}): step {t}")
    if form is not None:
        assert env.step_form() == form
    env.close()
