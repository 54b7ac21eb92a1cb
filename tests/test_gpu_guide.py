"""The guide on the GPU (include/rcw.h, rcw_set_guide): both words of every agent byte for byte against tests/guide_ref.py — the rule in
numpy scalars, fed the engine's own field, positions, headings and table — after enabling and after every call of a rollout; the closed
loop on the device, plain and as a replayed graph; the life cycle; snapshots; and that a handle without the guide launches what it did.

Frames are 8 rays by 8 rows: nothing here reads a pixel.  The nd values are the kernel's boundaries — 1: one lane has work; 63, 64, 65: a
partial, a full and a wrapped pass of the wavefront over the table; 128; 130: a tail pass; 1000."""
import ctypes as C

import numpy as np
import pytest

import goal_distance_ref as GD
import guide_ref as GR

pytestmark = pytest.mark.gpu

B = 67
MAPS = [(5, 5), (9, 9), (17, 13)]
ND = [1, 63, 64, 65, 128, 130, 1000]
# every nd in both types; the maps and the out-of-bounds modes go round, so that each map and each mode meets both types
ROLLOUTS = [(nd, T, MAPS[(k + t) % 3], (k + t) % 2) for t, T in enumerate(["Float32", "Float64"]) for k, nd in enumerate(ND)]


def make(rcw, batch, H, W, nd=8, T="Float32", oob=1, inc=0.25, radius=0.25, seed=11, **kw):
    return rcw.SingleRoomModule.SingleRoom(batch=batch, seed=seed, T=T, auto_reset=True, num_directions=nd, position_increment_wu=inc,
                                           player_radius_wu=radius, height_tile_map_tu=H, width_tile_map_tu=W, num_rays=8,
                                           height_camera_view_pu=8, out_of_bounds=oob, **kw)


def pillar_layouts(H, W, rng, count=8):
    """pillars with pockets (a third of the interior at most); two free tiles are what set_walls asks for"""
    out = []
    while len(out) < count:
        w = GD.pillars(H, W, 0.3 if min(H, W) > 5 else 0.2, rng)
        if (~w).sum() >= 2:
            out.append(w)
    return np.stack(out)


def settle(env, raising):
    """out_of_bounds = 0: a step may leave an IndexError for the next sync — taken here and cleared before the state is read"""
    if raising:
        try:
            env.sync()
        except IndexError:
            env.clear_error()


@pytest.mark.parametrize("nd,T,hw,oob", ROLLOUTS, ids=[f"nd{nd}-{T}-{h}x{w}-oob{o}" for nd, T, (h, w), o in ROLLOUTS])
def test_both_words_after_every_call_of_a_rollout(rcw, nd, T, hw, oob):
    """sixty steps — half the agents follow the guide, half draw —, and every sixth call a masked reset_, set_state (onto walls, goals and
    anywhere in a tile), set_walls or a shuffled direction table with duplicates"""
    H, W = hw
    rng = np.random.default_rng([nd, H, W, oob, T == "Float64"])
    env = make(rcw, B, H, W, nd=nd, T=T, oob=oob)
    env.set_walls(pillar_layouts(H, W, rng), index=rng.integers(0, 8, B))
    env.set_goal_distance(True)
    t = GR.Tracked(env)
    base = env.world.directions_wu.copy()
    for step in range(60):
        kind = (step // 6) % 4 if step % 6 == 5 else -1
        mask = rng.random(B) < 0.4
        if kind == 0:
            rcw.reset_(env, mask=mask)
        elif kind == 1:
            goal = np.stack([rng.integers(2, H, B), rng.integers(2, W, B)], axis=1)
            cell = np.stack([rng.integers(1, H - 1, B), rng.integers(1, W - 1, B)], axis=1)
            onto_goal = rng.random(B) < 0.2
            cell[onto_goal] = goal[onto_goal] - 1                                 # (0-based tile of the 1-based goal)
            off = np.where(rng.random((B, 2)) < 0.5, 0.5, rng.random((B, 2)) * 0.999)
            env.set_state(goal, cell + off, rng.integers(0, nd, B), mask=mask)
        elif kind == 2:
            env.set_walls(pillar_layouts(H, W, rng), index=rng.integers(0, 8, B), mask=mask)
        elif kind == 3:
            table = base[rng.integers(0, nd, nd)] if step % 12 == 5 else rng.permutation(base)
            env.set_direction_table(table)
        if kind >= 0:
            settle(env, oob == 0)
            t.check(f"call {kind} before step {step}")
        follow = rng.random(B) < 0.5
        a = np.where(follow, env.guide_action.numpy(), rng.integers(1, 5, B)).astype(np.uint8)
        rcw.act_(env, a)
        settle(env, oob == 0)
        t.check(f"step {step}")
    s = t.seen
    assert s["checks"] == 71 and s["no_advice"] > 0 and (nd == 1 or s[3] > s["no_advice"]), s
    assert s[1] > 0 and (nd <= 2 or s[4] > 0), s
    assert int(env.world.episode.max()) >= 3                                      # agents arrived and restarted on the way
    env.close()


# ---- the closed loop on the device ----------------------------------------------------------------------------------------------------
LOOP = dict(batch=256, H=13, W=13, nd=16, inc=0.25, radius=0.25, steps=900)
_largest = {}


def loop_env(rcw, limit):
    c = LOOP
    env = make(rcw, c["batch"], c["H"], c["W"], nd=c["nd"], inc=c["inc"], radius=c["radius"], seed=4, wall_generator=dict(loops=0.1))
    if limit:
        env.set_time_limit(limit)
    env.set_guide(True)
    env.set_episode_stats(True)
    return env


def largest_start_distance(rcw):
    """The same loop without a limit, once: the largest l of any episode it starts (a running maximum kept on the device), and that
    `steps` calls are enough for every agent to close an episode.  The engine is deterministic: with a limit no episode reaches, the
    limited loop sees the very same episodes."""
    if "l" not in _largest:
        import torch

        env = loop_env(rcw, 0)
        assert env.guide_info == dict(enabled=True, promised=True)
        actions, start = env.guide_action.torch(sync=False), env.goal_start_distance.torch(sync=False)
        with torch.cuda.stream(env.torch_stream()):
            seen = start.clone()
            for _ in range(LOOP["steps"]):
                rcw.act_(env, actions)
                seen = torch.maximum(seen, start)
        _largest["l"] = int(seen.max().item())
        tab = env.episode_stats_table()["totals"]
        assert int(np.asarray(env.episode_stats.episodes).min()) >= 1 and tab["successes"] == tab["episodes"] >= LOOP["batch"], tab
        assert 10 <= _largest["l"] < 121
        env.close()
    return _largest["l"]


def assert_everyone_arrived(env, l):
    tab = env.episode_stats_table()["totals"]
    assert tab["truncations"] == 0 and tab["successes"] == tab["episodes"] >= LOOP["batch"], (tab, l)
    assert int(np.asarray(env.episode_stats.episodes).min()) >= 1
    # (an episode starts at a tile centre and the guide walks from centre to centre: the path is l tiles but for the last move, which
    # touches the goal and is not made — SPL is 1 up to that; half of it is asked)
    assert env.episode_stats_table()["spl"]["totals"] > 0.5


def test_agents_fed_their_own_guide_all_arrive_inside_the_bound(rcw):
    """256 agents on generated mazes with loops, auto_reset, the time limit the promise's bound for the largest l the loop sees; the
    actions go from guide_action into the step with no host copy"""
    pytest.importorskip("torch")
    l = largest_start_distance(rcw)
    env = loop_env(rcw, GR.bound(l, LOOP["nd"], LOOP["inc"]))
    actions = env.guide_action.torch(sync=False)
    syncs = env.host_syncs
    for _ in range(LOOP["steps"]):
        rcw.act_(env, actions)
    assert env.host_syncs == syncs
    assert_everyone_arrived(env, l)
    env.close()


def test_the_same_under_a_captured_and_replayed_graph_of_the_step(rcw):
    """one captured step whose actions are the guide's own array, replayed: the guide's kernel rewrites what the next replay reads"""
    torch = pytest.importorskip("torch")
    l = largest_start_distance(rcw)
    env = loop_env(rcw, GR.bound(l, LOOP["nd"], LOOP["inc"]))
    stream = torch.cuda.Stream()
    env.sync()
    env.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        actions = env.guide_action.torch(sync=False)
        for _ in range(2):
            rcw.act_(env, actions)
        stream.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            rcw.act_(env, actions)
        for _ in range(LOOP["steps"] - 2):
            g.replay()
        stream.synchronize()
    assert_everyone_arrived(env, l)
    GR.Tracked(env, enable=False)                                                 # ... and the words are the rule's of the final state
    del g
    env.close()


# ---- the life cycle --------------------------------------------------------------------------------------------------------------------
def test_enabling_disabling_and_what_a_handle_without_the_guide_launches(rcw):
    from raycastworlds_jl_amd import _capi, layouts

    UNSUPPORTED = _capi.RCW_ERR_UNSUPPORTED
    env = make(rcw, B, 9, 9, nd=8)
    lib, h = env._lib, env._h
    p, q = C.c_void_p(), C.c_void_p()
    kernels = (env.fill_kernel_name(), env.step_form())
    assert env.guide_info == dict(enabled=False, promised=True) and not env.guide_enabled
    assert lib.rcw_set_guide(h, 1) == UNSUPPORTED and "goal distance" in _capi.last_error(lib)   # no field to follow
    assert lib.rcw_set_guide(h, 0) == 0                                            # RCW_OK also where there was none
    assert lib.rcw_guide(h, None, None) == UNSUPPORTED
    assert lib.rcw_guide_device_ptr(h, C.byref(p), C.byref(q)) == UNSUPPORTED and not p.value and not q.value
    env.set_guide(True)                                                            # (the wrapper enables the goal distance first)
    assert env.goal_distance_enabled and env.guide_info == dict(enabled=True, promised=True)
    t = GR.Tracked(env, enable=False)
    assert lib.rcw_guide(h, None, None) == 0                                       # either pointer may be NULL
    assert lib.rcw_guide_device_ptr(h, C.byref(p), None) == 0 and lib.rcw_guide_device_ptr(h, None, C.byref(q)) == 0
    assert (p.value, q.value) == (env.guide_action.ptr, env.guide_heading.ptr) and p.value % 16 == 0 and q.value % 16 == 0
    rng = np.random.default_rng(3)
    for k in range(6):
        rcw.act_(env, rng.integers(1, 5, B).astype(np.uint8))
        action, heading = t.check(f"step {k}")
    # the handle-less export on the engine's own state
    field, w = env.goal_distance_field, env.world
    for b in range(0, B, 7):
        assert layouts.guide_rule(field[b], w.player_position_wu[b], w.player_direction_au[b], w.directions_wu, 0.25) == (action[b], heading[b])
    # stable pointers: steps, a reset, the goal distance enabled again (a new field, the same words, computed again)
    env.set_goal_distance(True)
    rcw.reset_(env)
    assert lib.rcw_guide_device_ptr(h, C.byref(p), C.byref(q)) == 0 and (p.value, q.value) == (env.guide_action.ptr, env.guide_heading.ptr)
    t.check("behind set_goal_distance(True) again and a reset")
    env.set_guide(True)                                                            # again: recomputed
    GR.Tracked(env, enable=False)
    assert (env.fill_kernel_name(), env.step_form()) == kernels
    # the goal distance goes: so does the guide
    env.set_goal_distance(False)
    assert env.guide_info["enabled"] is False and lib.rcw_guide(h, None, None) == UNSUPPORTED
    assert (env.fill_kernel_name(), env.step_form()) == kernels                   # off -> on -> off: the handle launches what it did
    rcw.act_(env, rng.integers(1, 5, B).astype(np.uint8))
    env.sync()
    env.set_guide(True)
    env.set_guide(False)
    assert env.goal_distance_enabled and not env.guide_enabled                     # (switching the guide off leaves the goal distance)
    env.close()
    # the promise's condition
    for inc, radius, promised in ((0.125, 0.45, False), (0.2, 0.3, True), (0.25, 0.26, False)):
        for T in ("Float32", "Float64"):
            e = make(rcw, 2, 5, 5, T=T, inc=inc, radius=radius)
            assert e.guide_info == dict(enabled=False, promised=promised), (inc, radius, T)
            e.close()


def test_the_one_launch_step_with_the_guide_behind_it(rcw):
    """the guide is queued behind either form of the step; a handle that takes the one-launch form keeps it with the guide on"""
    env = rcw.SingleRoomModule.SingleRoom(batch=64, seed=2, auto_reset=True, num_directions=8, position_increment_wu=0.25, player_radius_wu=0.25,
                                          height_tile_map_tu=9, width_tile_map_tu=9, num_rays=64, height_camera_view_pu=64, out_of_bounds=1)
    env.set_step_form("one-launch")
    env.set_guide(True)
    t = GR.Tracked(env, enable=False)
    rng = np.random.default_rng(5)
    for k in range(12):
        rcw.act_(env, np.where(rng.random(64) < 0.7, env.guide_action.numpy(), rng.integers(1, 5, 64)).astype(np.uint8))
        t.check(f"one-launch step {k}")
    assert env.step_form() == "one-launch"
    env.close()


# ---- snapshots ---------------------------------------------------------------------------------------------------------------------------
def test_a_restore_computes_the_restored_agents_words_and_rows_fit_a_handle_without_the_guide(rcw):
    rng = np.random.default_rng(9)
    walls = pillar_layouts(9, 9, rng)
    index = rng.integers(0, 8, B)

    def build(guide):
        env = make(rcw, B, 9, 9, nd=8)
        env.set_walls(walls, index=index)
        env.set_goal_distance(True)
        if guide:
            env.set_guide(True)
        env.set_snapshots(B)
        return env

    one, two = build(True), build(False)
    assert one.snapshot_info["shape_key"] == two.snapshot_info["shape_key"] and one.snapshot_info["row_bytes"] == two.snapshot_info["row_bytes"]
    t = GR.Tracked(one, enable=False)
    for k in range(5):
        rcw.act_(one, rng.integers(1, 5, B).astype(np.uint8))
    saved = t.check("at the save")
    pose = (one.world.player_position_wu.copy(), one.world.player_direction_au.copy())
    one.snapshot_save()
    for k in range(9):
        rcw.act_(one, rng.integers(1, 5, B).astype(np.uint8))
    t.check("moved on")
    mask = rng.random(B) < 0.5
    one.snapshot_restore(mask=mask)
    action, heading = t.check("behind the masked restore")
    np.testing.assert_array_equal(one.world.player_position_wu[mask], pose[0][mask])
    np.testing.assert_array_equal(action[mask], saved[0][mask])                    # the words of the restored state
    np.testing.assert_array_equal(heading[mask], saved[1][mask])
    assert (one.world.player_direction_au[~mask] != pose[1][~mask]).any() or (one.world.player_position_wu[~mask] != pose[0][~mask]).any()
    # ... under another table the restored agents' words follow the table as it is NOW
    one.set_direction_table(np.roll(one.world.directions_wu, 3, axis=0))
    one.snapshot_restore()
    t.check("behind a restore under a rolled table")
    # rows go to a handle without the guide, and come back
    two.snapshot_import(one.snapshot_export())
    two.snapshot_restore()
    np.testing.assert_array_equal(two.world.player_position_wu, pose[0])
    np.testing.assert_array_equal(two.goal_distance_field, one.goal_distance_field)
    rcw.act_(two, 3)
    two.snapshot_save()
    one.snapshot_import(two.snapshot_export())
    one.snapshot_restore()
    t.check("behind a restore of rows saved without the guide")
    np.testing.assert_array_equal(one.world.player_direction_au, two.world.player_direction_au)
    one.close()
    two.close()


# ---- the example -------------------------------------------------------------------------------------------------------------------------
def test_the_example_follows_the_guide_to_every_goal():
    """examples/follow_the_guide.py as a user would run it, in a process of its own: 128 agents, 500 steps, 4 levels, no exploration"""
    import os
    import re
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "examples/follow_the_guide.py", "128", "500", "4"], cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"128 agents x 500 steps following the guide \(promised: True, epsilon 0 %\): (\d+) episodes, success rate ([\d.]+), (\d+) truncated, mean SPL ([\d.]+)", r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) >= 128 and float(m.group(2)) == 1.0 and int(m.group(3)) == 0 and float(m.group(4)) > 0.5, r.stdout
    assert len(re.findall(r"^  level \d: \d+ episodes", r.stdout, re.M)) == 4, r.stdout
