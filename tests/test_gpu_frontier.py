"""The frontier on the GPU (include/rcw.h, rcw_set_frontier): the field — all B * H * W entries — and the four words of every agent byte
for byte against tests/frontier_ref.py — the flood in numpy, fed the engine's own seen map, and the guide's rule in numpy scalars, fed the
engine's own positions, headings and table — after enabling and after every call of a rollout; floods wider than a wavefront; the map size
that needs the raised LDS limit; queued calls; the closed loop on the device, plain and as a replayed graph; the life cycle; snapshots; the
example.

Frames are 8 rays by 8 rows except where stated: nothing here reads a pixel."""
import ctypes as C

import numpy as np
import pytest

import frontier_ref as FR
import goal_distance_ref as GD

pytestmark = pytest.mark.gpu

B = 67
MAPS = [(5, 5), (9, 9), (17, 13)]
ND = [8, 64, 130]
# every nd in both types; the maps and the out-of-bounds modes go round, so that each map and each mode meets both types
ROLLOUTS = [(nd, T, MAPS[(k + t) % 3], (k + t) % 2) for t, T in enumerate(["Float32", "Float64"]) for k, nd in enumerate(ND)]


def make(rcw, batch, H, W, nd=8, T="Float32", oob=1, inc=0.25, radius=0.25, seed=11, rays=8, **kw):
    return rcw.SingleRoomModule.SingleRoom(batch=batch, seed=seed, T=T, auto_reset=True, num_directions=nd, position_increment_wu=inc,
                                           player_radius_wu=radius, height_tile_map_tu=H, width_tile_map_tu=W, num_rays=rays,
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
def test_field_and_words_after_every_call_of_a_rollout(rcw, nd, T, hw, oob):
    """sixty steps under a time limit of 25 — half the agents follow explore_action, half draw —, and every sixth call a masked reset_,
    set_state (onto walls, goals and anywhere in a tile), set_walls or a shuffled direction table with duplicates"""
    H, W = hw
    rng = np.random.default_rng([nd, H, W, oob, T == "Float64"])
    env = make(rcw, B, H, W, nd=nd, T=T, oob=oob, max_episode_steps=25)
    env.set_walls(pillar_layouts(H, W, rng), index=rng.integers(0, 8, B))
    env.set_seen_map(True)
    t = FR.Tracked(env)
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
        a = np.where(follow, env.explore_action.numpy(), rng.integers(1, 5, B)).astype(np.uint8)
        rcw.act_(env, a)
        settle(env, oob == 0)
        t.check(f"step {step}", stepped=True)
    s = t.seen
    print(s)
    assert s["checks"] == 71 and s["kept"] > 0 and s["flooded"] > 0 and s["nothing_left"] > 0 and s["restarts"] > 0 and s["forward"] > 0, s
    env.close()


def test_floods_wider_than_a_wavefront(rcw):
    """an empty 40 x 40 room, 64 rays: a fan's rim is more than 64 sources, and a level of the flood more than 64 tiles — several passes of
    the wavefront over the seeds and over a level, whose appends go behind a ballot prefix"""
    env = make(rcw, 3, 40, 40, nd=16, rays=64, seed=5)
    # two agents in opposite corners looking along the diagonal, one at the middle of an edge looking across: the longest fans the room has
    # (the goals sit in corners no fan crosses early: a goal tile stops a ray)
    env.set_state(np.array([[2, 39], [2, 39], [39, 39]]), np.array([[1.5, 1.5], [38.5, 38.5], [20.5, 1.5]]), np.array([2, 10, 4]))
    env.set_seen_map(True)
    t = FR.Tracked(env)
    for k in range(6):
        rcw.act_(env, np.array([3, 3, 1], np.uint8))                              # the fans sweep the room, the third agent walks
        t.check(f"step {k}", stepped=True)
    print(t.seen)
    assert t.seen["most_sources"] > 64 and t.seen["widest_level"] > 64, t.seen
    env.close()


def test_the_map_size_that_needs_the_raised_lds_limit(rcw):
    """182 x 182: the flood needs 76.8 KiB of LDS there, more than a launch gets without the raised limit (this kernel needs it from
    167 x 167, the goal distance's from 176 x 176)"""
    env = make(rcw, 2, 182, 182, nd=16, seed=3)
    env.set_seen_map(True)
    t = FR.Tracked(env)
    for k in range(3):
        rcw.act_(env, np.array([3, 1], np.uint8))
        t.check(f"step {k}", stepped=True)
    assert t.seen["most_sources"] > 0
    env.close()


def test_queued_calls_that_nobody_reads_between(rcw):
    """three steps, a masked reset and two steps queued without a readout: the field is the final map's"""
    rng = np.random.default_rng(8)
    env = make(rcw, B, 9, 9, nd=8)
    env.set_walls(pillar_layouts(9, 9, rng), index=rng.integers(0, 8, B))
    env.set_frontier(True)                                                        # (the wrapper enables the seen map first)
    actions = [rng.integers(1, 5, B).astype(np.uint8) for _ in range(5)]
    mask = rng.random(B) < 0.5
    syncs = env.host_syncs
    for a in actions[:3]:
        rcw.act_(env, a)
    rcw.reset_(env, mask=mask)
    for a in actions[3:]:
        rcw.act_(env, a)
    assert env.host_syncs == syncs
    FR.Tracked(env, enable=False)
    env.close()


# ---- the closed loop on the device ----------------------------------------------------------------------------------------------------
LOOP = dict(batch=256, H=13, W=13, nd=16, inc=0.25, radius=0.25, rays=8, cap=4000)


def loop_env(rcw):
    c = LOOP
    env = make(rcw, c["batch"], c["H"], c["W"], nd=c["nd"], inc=c["inc"], radius=c["radius"], rays=c["rays"], seed=4, wall_generator=dict(loops=0.1))
    env.set_frontier(True)
    return env


def test_agents_fed_their_own_explore_action_finish_within_4000_steps(rcw):
    """256 agents on generated mazes, the CPU loop's parameters; the actions go from explore_action into the step with no host copy.  An
    agent is finished once it has reported distance == -1 or has restarted (it touched its goal); the flag lives on the device and is read
    every 500 steps"""
    torch = pytest.importorskip("torch")
    env = loop_env(rcw)
    with torch.cuda.stream(env.torch_stream()):
        actions, distance, done = env.explore_action.torch(sync=False), env.frontier_distance.torch(sync=False), env.done_device().torch(sync=False)
        finished = distance < 0
        episode0 = env.world.episode.copy()
        steps = 0
        while steps < LOOP["cap"]:
            syncs = env.host_syncs
            for _ in range(500):
                rcw.act_(env, actions)
                finished |= (distance < 0) | (done != 0)
            assert env.host_syncs == syncs
            steps += 500
            left = int((~finished).sum().item())
            print(f"after {steps} steps: {left} agents still exploring")
            if left == 0:
                break
    assert left == 0, f"{left} of {LOOP['batch']} agents neither explored everything nor reached their goal within {LOOP['cap']} steps"
    assert (env.world.episode > episode0).any()                                   # (some did reach their goal and restarted)
    FR.Tracked(env, enable=False)
    env.close()


def test_the_same_under_a_captured_and_replayed_graph_of_the_step(rcw):
    """one captured step whose actions are the frontier's own array, replayed 30 times: the kernels rewrite what the next replay reads, and
    the recorded episode counter lives on the device"""
    torch = pytest.importorskip("torch")
    env = loop_env(rcw)
    stream = torch.cuda.Stream()
    env.sync()
    env.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        actions = env.explore_action.torch(sync=False)
        for _ in range(2):
            rcw.act_(env, actions)
        stream.synchronize()
        before = env.world.player_position_wu.copy(), env.world.player_direction_au.copy()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            rcw.act_(env, actions)
        for _ in range(30):
            g.replay()
        stream.synchronize()
    assert (env.world.player_position_wu != before[0]).any() and (env.world.player_direction_au != before[1]).any()
    FR.Tracked(env, enable=False)                                                 # ... and everything is the flood's and the rule's of the final state
    del g
    env.close()


# ---- the life cycle --------------------------------------------------------------------------------------------------------------------
def test_enabling_disabling_and_what_a_handle_without_the_frontier_launches(rcw):
    from raycastworlds_jl_amd import _capi, layouts

    UNSUPPORTED = _capi.RCW_ERR_UNSUPPORTED
    env = make(rcw, B, 9, 9, nd=8)
    lib, h = env._lib, env._h
    p = [C.c_void_p() for _ in range(4)]
    q = C.c_void_p()
    out = np.zeros((B, 81), np.uint16)
    kernels = (env.fill_kernel_name(), env.step_form())
    assert env.frontier_info == dict(enabled=False) and not env.frontier_enabled
    assert lib.rcw_set_frontier(h, 1) == UNSUPPORTED and "seen map" in _capi.last_error(lib)   # no map to flood over
    assert lib.rcw_set_frontier(h, 0) == 0                                         # RCW_OK also where there was none
    assert lib.rcw_frontier(h, None, None, None, None) == UNSUPPORTED
    assert lib.rcw_frontier_device_ptr(h, *[C.byref(v) for v in p]) == UNSUPPORTED and not any(v.value for v in p)
    assert lib.rcw_frontier_field(h, 0, B, out.ctypes.data) == UNSUPPORTED
    assert lib.rcw_frontier_field_device_ptr(h, C.byref(q)) == UNSUPPORTED and not q.value
    env.set_frontier(True)                                                         # (the wrapper enables the seen map first)
    assert env.seen_map_enabled and env.frontier_info == dict(enabled=True)
    t = FR.Tracked(env, enable=False)
    assert lib.rcw_frontier(h, None, None, None, None) == 0                        # any pointer may be NULL
    assert lib.rcw_frontier_device_ptr(h, C.byref(p[0]), None, None, None) == 0 and lib.rcw_frontier_device_ptr(h, None, C.byref(p[1]), C.byref(p[2]), C.byref(p[3])) == 0
    words = (env.frontier_distance, env.frontier_tiles, env.explore_action, env.explore_heading)
    assert [v.value for v in p] == [w.ptr for w in words] and all(v.value % 16 == 0 for v in p)
    assert lib.rcw_frontier_field_device_ptr(h, C.byref(q)) == 0 and q.value == env.frontier_field_device.ptr and q.value % 16 == 0
    assert lib.rcw_frontier_field_device_ptr(h, None) == _capi.RCW_ERR_INVALID_ARGUMENT
    rng = np.random.default_rng(3)
    for k in range(6):
        rcw.act_(env, rng.integers(1, 5, B).astype(np.uint8))
        exp = t.check(f"step {k}", stepped=True)
    # a range of the field, and the refused ranges
    part = np.zeros((5, 9, 9), np.uint16)
    assert lib.rcw_frontier_field(h, 7, 5, part.ctypes.data) == 0
    np.testing.assert_array_equal(part.transpose(0, 2, 1), exp["field"][7:12])
    assert lib.rcw_frontier_field(h, B - 2, 3, part.ctypes.data) == _capi.RCW_ERR_INVALID_ARGUMENT
    assert lib.rcw_frontier_field(h, 0, 5, None) == _capi.RCW_ERR_INVALID_ARGUMENT
    np.testing.assert_array_equal(env.frontier_field_device.numpy().transpose(0, 2, 1), exp["field"])
    # the handle-less export on the engine's own maps
    maps = env.seen_map
    for b in range(0, B, 7):
        field, tiles = layouts.frontier_rule(maps[b])
        np.testing.assert_array_equal(field, exp["field"][b])
        assert tiles == exp["tiles"][b]
    # the seen map cannot go while the frontier floods over it; nothing changes
    assert lib.rcw_set_seen_map(h, 0) == UNSUPPORTED and "frontier" in _capi.last_error(lib)
    assert env.seen_map_enabled and env.frontier_enabled
    t.check("behind the refused set_seen_map(False)")
    # the seen map again: every agent's map starts afresh, every agent is flooded again
    env.set_seen_map(True)
    exp = t.check("behind set_seen_map(True) again")
    assert lib.rcw_frontier_device_ptr(h, *[C.byref(v) for v in p]) == 0 and [v.value for v in p] == [w.ptr for w in words]   # (stable pointers)
    rcw.act_(env, rng.integers(1, 5, B).astype(np.uint8))
    t.check("a step behind it", stepped=True)
    env.set_frontier(True)                                                         # again: recomputed
    FR.Tracked(env, enable=False)
    assert (env.fill_kernel_name(), env.step_form()) == kernels
    # off, and on again
    env.set_frontier(False)
    assert env.frontier_info == dict(enabled=False) and env.seen_map_enabled
    assert lib.rcw_frontier(h, None, None, None, None) == UNSUPPORTED and lib.rcw_frontier_field(h, 0, B, out.ctypes.data) == UNSUPPORTED
    assert lib.rcw_frontier_device_ptr(h, *[C.byref(v) for v in p]) == UNSUPPORTED and lib.rcw_frontier_field_device_ptr(h, C.byref(q)) == UNSUPPORTED
    assert (env.fill_kernel_name(), env.step_form()) == kernels                   # off -> on -> off: the handle launches what it did
    rcw.act_(env, rng.integers(1, 5, B).astype(np.uint8))
    env.sync()
    env.set_frontier(True)
    t = FR.Tracked(env, enable=False)
    rcw.act_(env, rng.integers(1, 5, B).astype(np.uint8))
    t.check("a step behind off and on again", stepped=True)
    env.set_frontier(False)
    env.set_seen_map(False)                                                        # ... and now the seen map may go
    assert not env.seen_map_enabled
    env.close()


def test_the_one_launch_step_with_the_frontier_behind_it(rcw):
    """the frontier is queued behind either form of the step; a handle that takes the one-launch form keeps it with the frontier on"""
    env = rcw.SingleRoomModule.SingleRoom(batch=64, seed=2, auto_reset=True, num_directions=8, position_increment_wu=0.25, player_radius_wu=0.25,
                                          height_tile_map_tu=9, width_tile_map_tu=9, num_rays=64, height_camera_view_pu=64, out_of_bounds=1)
    env.set_step_form("one-launch")
    env.set_frontier(True)
    t = FR.Tracked(env, enable=False)
    rng = np.random.default_rng(5)
    for k in range(12):
        rcw.act_(env, np.where(rng.random(64) < 0.7, env.explore_action.numpy(), rng.integers(1, 5, 64)).astype(np.uint8))
        t.check(f"one-launch step {k}", stepped=True)
    assert env.step_form() == "one-launch"
    env.close()


# ---- snapshots ---------------------------------------------------------------------------------------------------------------------------
def test_a_restore_floods_the_restored_agents_again_and_rows_fit_a_handle_without_the_frontier(rcw):
    rng = np.random.default_rng(9)
    walls = pillar_layouts(9, 9, rng)
    index = rng.integers(0, 8, B)

    def build(frontier):
        env = make(rcw, B, 9, 9, nd=8)
        env.set_walls(walls, index=index)
        env.set_seen_map(True)
        if frontier:
            env.set_frontier(True)
        env.set_snapshots(B)
        return env

    one, two = build(True), build(False)
    assert one.snapshot_info["shape_key"] == two.snapshot_info["shape_key"] and one.snapshot_info["row_bytes"] == two.snapshot_info["row_bytes"]
    t = FR.Tracked(one, enable=False)
    for k in range(5):
        rcw.act_(one, rng.integers(1, 5, B).astype(np.uint8))
    saved = t.check("at the save")
    saved_maps = one.seen_map
    one.snapshot_save()
    for k in range(10):
        rcw.act_(one, rng.integers(1, 5, B).astype(np.uint8))
    moved = t.check("moved on")
    assert (moved["field"] != saved["field"]).any()
    mask = rng.random(B) < 0.5
    one.snapshot_restore(mask=mask)
    back = t.check("behind the masked restore")
    for name in ("field", "distance", "tiles", "action", "heading"):
        np.testing.assert_array_equal(back[name][mask], saved[name][mask], err_msg=name)        # the restored agents: as of the save
        np.testing.assert_array_equal(back[name][~mask], moved[name][~mask], err_msg=name)      # the others: kept
    # rows go to a handle without the frontier, and come back
    two.snapshot_import(one.snapshot_export())
    two.snapshot_restore()
    np.testing.assert_array_equal(two.seen_map, saved_maps)
    rcw.act_(two, 3)
    two.snapshot_save()
    one.snapshot_import(two.snapshot_export())
    one.snapshot_restore()
    t.check("behind a restore of rows saved without the frontier")
    np.testing.assert_array_equal(one.seen_map, two.seen_map)
    one.close()
    two.close()


# ---- the example -------------------------------------------------------------------------------------------------------------------------
def test_the_example_explores_then_goes():
    """examples/explore_then_go.py as a user would run it, in a process of its own: 128 agents, 1200 steps, 4 levels"""
    import os
    import re
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "examples/explore_then_go.py", "128", "1200", "4"], cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = r"%s: 128 agents x 1200 steps: (\d+) episodes, success rate ([\d.]+), (\d+) truncated, mean length ([\d.]+), mean SPL ([\d.]+)"
    explore, oracle = re.search(line % "explore, then go", r.stdout), re.search(line % "the guide alone", r.stdout)
    assert explore and oracle, r.stdout
    assert int(oracle.group(1)) >= 128 and float(oracle.group(2)) == 1.0, r.stdout
    # the explorer reaches goals too, and no faster than the oracle that knows where they are
    assert int(explore.group(1)) >= 128 and float(explore.group(2)) > 0.9 and float(explore.group(4)) >= float(oracle.group(4)), r.stdout
