"""The visit map on the GPU (include/rcw.h, rcw_set_visit_map): the map — all B * sectors * H * W entries —, the four words of every agent
and the table, held EXACTLY (everything is an integer) to tests/visit_map_ref.py, which applies the definition to the engine's own
positions, direction indices, episode counters and layout words after every call: rollouts with restarts and masked calls at odd sizes
(the clear's narrow head and tail), the table with several agents on one entry in one call, saturation, the state archive, queued and
replayed steps, the life cycle, the example.

Frames are 8 rays by 8 rows: nothing here reads a pixel."""
import ctypes as C

import numpy as np
import pytest

import visit_map_ref as VR
from test_gpu_frontier import make, pillar_layouts, settle

pytestmark = pytest.mark.gpu

B = 67
MAPS = [(5, 5), (5, 7), (17, 13)]
SECTORS = [1, 3, 8]
ND = [8, 16, 130]
# every nd in both types; maps, sectors and the out-of-bounds modes go round, so that each meets both types
ROLLOUTS = [(nd, T, MAPS[(k + t) % 3], SECTORS[(k + 2 * t + 1) % 3], (k + t) % 2) for t, T in enumerate(["Float32", "Float64"]) for k, nd in enumerate(ND)]


def random_actions(rng, n=B):
    return rng.integers(1, 5, n).astype(np.uint8)


@pytest.mark.parametrize("nd,T,hw,sectors,oob", ROLLOUTS, ids=[f"nd{nd}-{T}-{h}x{w}-s{s}-oob{o}" for nd, T, (h, w), s, o in ROLLOUTS])
def test_map_and_words_after_every_call_of_a_rollout(rcw, nd, T, hw, sectors, oob):
    """sixty random steps under a time limit of 7 with auto_reset, and every sixth call a masked reset_, set_state (onto walls and anywhere
    in a tile), set_walls or a shuffled direction table.  67 agents of an odd number of cells: most maps begin off a multiple of 16 bytes"""
    H, W = hw
    rng = np.random.default_rng([nd, H, W, sectors, oob, T == "Float64"])
    env = make(rcw, B, H, W, nd=nd, T=T, oob=oob, max_episode_steps=7)
    env.set_walls(pillar_layouts(H, W, rng), index=rng.integers(0, 8, B))
    t = VR.Tracked(env, sectors=sectors)
    assert env.visit_map_info == dict(enabled=True, sectors=sectors, table=False, rows=0, first=0)
    base = env.world.directions_wu.copy()
    for step in range(60):
        kind = (step // 6) % 4 if step % 6 == 5 else -1
        mask = rng.random(B) < 0.4
        if kind == 0:
            rcw.reset_(env, mask=mask)
        elif kind == 1:
            goal = np.stack([rng.integers(2, H, B), rng.integers(2, W, B)], axis=1)
            tile = np.stack([rng.integers(1, H - 1, B), rng.integers(1, W - 1, B)], axis=1)
            off = np.where(rng.random((B, 2)) < 0.5, 0.5, rng.random((B, 2)) * 0.999)
            env.set_state(goal, tile + off, rng.integers(0, nd, B), mask=mask)
        elif kind == 2:
            env.set_walls(pillar_layouts(H, W, rng), index=rng.integers(0, 8, B), mask=mask)
        elif kind == 3:
            env.set_direction_table(rng.permutation(base))
        if kind >= 0:
            settle(env, oob == 0)
            if kind == 3:
                t.untouched(f"a new direction table before step {step}")
            else:
                t.refilled(mask, f"call {kind} before step {step}")
        rcw.act_(env, random_actions(rng))
        settle(env, oob == 0)
        t.stepped(f"step {step}")
    s = t.seen
    print(s)
    # the run contained what the comparisons are about — asserted on the reference
    # (a mask costs an agent at most one restart under the limit and begins it once: 60 steps under a limit of 7 begin every agent 8 times)
    assert s["checks"] == 71 and s["restarts"] > B and s["restarts"] + s["begun"] >= 8 * B and s["kept"] > 0 and s["first1"] > 0 and s["first0"] > 0 and s["most"] >= 3, s
    env.close()


# ---- the table -----------------------------------------------------------------------------------------------------------------------------
def bank_env(rcw, rng, **kw):
    return make(rcw, B, 5, 5, max_episode_steps=7, wall_bank=pillar_layouts(5, 5, rng, count=3), **kw)


def test_the_table_and_level_here_with_many_agents_on_one_entry(rcw):
    """a bank of three layouts on 5 x 5: nine interior tiles for 67 agents, so every call adds to one (row, cell) from several agents"""
    rng = np.random.default_rng(31)
    env = bank_env(rcw, rng)
    t = VR.Tracked(env, sectors=1, table=True)
    assert env.visit_map_info == dict(enabled=True, sectors=1, table=True, rows=3, first=0)
    for step in range(40):
        rcw.act_(env, random_actions(rng))
        t.stepped(f"step {step}")                                                 # (also: table[0].sum() == the number of counts)
        np.testing.assert_array_equal(t.table[1:].sum(axis=0), t.table[0])        # every layout of a bank has its row
    assert t.seen["shared"] > 40 and t.seen["restarts"] >= 5 * B, t.seen
    assert t.counts == 41 * B                                                     # every agent has a cell in every call
    np.testing.assert_array_equal(env.visit_table(device=True).numpy().transpose(0, 1, 3, 2), t.table)
    env.close()


def test_a_clear_queued_between_two_steps_without_a_sync(rcw):
    """two engines, the same seed and the same calls: one is read after every call and held to the reference, the other queues step, clear
    and step with no readout in between and must end where the reference is"""
    rngs = [np.random.default_rng(32), np.random.default_rng(32)]
    envs = [bank_env(rcw, r) for r in rngs]
    t = VR.Tracked(envs[0], sectors=1, table=True)
    envs[1].set_visit_map(sectors=1, table=True)
    a1, a2 = random_actions(rngs[0]), random_actions(rngs[0])
    rcw.act_(envs[0], a1)
    t.stepped("step 1")
    envs[0].visit_table_clear()
    t.table_cleared()
    words = t.untouched("behind the clear")                                      # the table is zero, no per-agent word has moved
    assert words["level_here"].any()
    rcw.act_(envs[0], a2)
    t.stepped("step 2")
    syncs = envs[1].host_syncs
    rcw.act_(envs[1], a1)
    envs[1].visit_table_clear()
    rcw.act_(envs[1], a2)
    assert envs[1].host_syncs == syncs
    t.check("the queued twin", env=envs[1])
    assert t.counts == B
    for e in envs:
        e.close()


def test_a_generators_level_range_and_a_handle_without_a_source(rcw):
    rng = np.random.default_rng(33)
    env = make(rcw, B, 5, 5, max_episode_steps=7, wall_generator=dict(loops=0.1, levels=5, first_level=3))
    t = VR.Tracked(env, sectors=1, table=True)
    assert (t.rows, t.first_level) == (5, 3)
    for step in range(20):
        rcw.act_(env, random_actions(rng))
        t.stepped(f"generator, step {step}")
    np.testing.assert_array_equal(t.table[1:].sum(axis=0), t.table[0])
    assert (t.table[1:].reshape(5, -1).sum(axis=1) > 0).all()                     # every level was played
    env.close()
    env = make(rcw, B, 5, 5, max_episode_steps=7)
    t = VR.Tracked(env, sectors=3, table=True)
    assert (t.rows, t.first_level) == (0, 0) and env.visit_table()["levels"].shape == (0, 3, 5, 5)
    for step in range(10):
        rcw.act_(env, random_actions(rng))
        t.stepped(f"no source, step {step}")
    assert t.level_here.max() > 1
    env.close()


def test_the_layout_source_setters_are_refused_while_the_table_is_on(rcw):
    from raycastworlds_jl_amd import _capi

    rng = np.random.default_rng(34)
    layouts = pillar_layouts(9, 9, rng, count=3)
    setters = [lambda e: e.set_wall_bank(layouts), lambda e: e.set_wall_generator(loops=0.1), lambda e: e.set_wall_caves(), lambda e: e.set_wall_rooms(),
               lambda e: e.set_wall_bank(None), lambda e: e.set_wall_generator(None), lambda e: e.set_wall_caves(None), lambda e: e.set_wall_rooms(None)]
    env = make(rcw, B, 9, 9, max_episode_steps=7)
    t = VR.Tracked(env, sectors=2, table=True)
    rcw.act_(env, random_actions(rng))
    t.stepped("a step")
    for k, setter in enumerate(setters):
        with pytest.raises(_capi.RcwError) as e:
            setter(env)
        assert e.value.code == _capi.RCW_ERR_UNSUPPORTED and "visit table" in str(e.value), (k, e.value)
        t.untouched(f"behind refused setter {k}")                                 # nothing changes
    # without the table: an install restarts every agent — BEGIN for all —, a removal does nothing
    env.set_visit_map(sectors=2, table=False)
    t = VR.Tracked(env, enable=False)
    t.refilled(None, "enabled again without the table")
    layouts9 = pillar_layouts(9, 9, rng, count=3)
    for k, (install, remove) in enumerate([(lambda: env.set_wall_bank(layouts9), lambda: env.set_wall_bank(None)),
                                           (lambda: env.set_wall_generator(loops=0.1), lambda: env.set_wall_generator(None)),
                                           (lambda: env.set_wall_caves(), lambda: env.set_wall_caves(None)),
                                           (lambda: env.set_wall_rooms(), lambda: env.set_wall_rooms(None))]):
        install()
        t.refilled(None, f"behind install {k}")
        rcw.act_(env, random_actions(rng))
        t.stepped(f"a step under source {k}")
        remove()
        t.untouched(f"behind removal {k}")
    env.close()


# ---- saturation ----------------------------------------------------------------------------------------------------------------------------
def test_an_entry_saturates_at_65535_and_the_table_still_grows(rcw):
    """the visit map's parts are the last segments of an exported row — here, visited, first, level_here, the counter, the map —: the entry
    of the agent's cell is set to 65534 in the row, the row imported and restored, and the agent turns on the spot three times"""
    env = make(rcw, 2, 5, 5, nd=8, max_episode_steps=0, visit_map=dict(sectors=1, table=True), snapshots=2)
    cells = 25
    rcw.act_(env, np.array([3, 4], np.uint8))                                     # (a turn: the cell is counted a second time)
    assert list(env.visits_here.numpy()) == [2, 2]
    cell = VR.cell_index(5, 5, 8, 1, env.world.player_position_wu, env.world.player_direction_au)
    env.snapshot_save()
    d = env.snapshot_export()
    rows = d["rows"]
    maps = rows[:, -2 * cells:].view(np.uint16)
    assert maps.shape == (2, cells) and [maps[a, cell[a]] for a in range(2)] == [2, 2] and (maps != 0).sum() == 2
    maps[0, cell[0]] = 65534
    env.snapshot_import(d)
    env.snapshot_restore()
    assert env.visit_map.reshape(2, -1).max(axis=1).tolist() == [65534, 2] and list(env.visits_here.numpy()) == [2, 2]   # a restore counts nothing
    total = int(env.visit_table()["total"].sum())
    assert total == 4
    for k in range(3):
        rcw.act_(env, np.array([3, 4], np.uint8))
        assert list(env.visits_here.numpy()) == [65535, 3 + k], k
        assert env.visit_map.reshape(2, -1).max(axis=1).tolist() == [65535, 3 + k]
        assert list(env.visit_first.numpy()) == [0, 0] and list(env.visited_cells.numpy()) == [1, 1]
        assert int(env.visit_table()["total"].sum()) == total + 2 * (k + 1)       # the table grows by one an agent a step, saturated or not
    env.close()


# ---- the state archive ---------------------------------------------------------------------------------------------------------------------
def test_a_restore_puts_the_record_back_counts_nothing_and_leaves_the_table(rcw):
    rng = np.random.default_rng(35)
    env = bank_env(rcw, rng)
    t = VR.Tracked(env, sectors=2, table=True)
    env.set_snapshots(B)
    for k in range(5):
        rcw.act_(env, random_actions(rng))
        saved = t.stepped(f"step {k}")
    saved_table, saved_counts = t.table.copy(), t.counts
    env.snapshot_save()
    t.untouched("behind the save")
    for k in range(20):
        rcw.act_(env, random_actions(rng))
        moved = t.stepped(f"moved on, step {k}")
    assert (moved["map"] != saved["map"]).any() and t.counts == saved_counts + 20 * B
    mask = rng.random(B) < 0.5
    env.snapshot_restore(mask=mask)
    # the reference takes the record back for the restored agents — the table is NOT rolled back
    for name, arr in (("map", t.map), ("here", t.here), ("visited", t.visited), ("first", t.first), ("level_here", t.level_here)):
        arr[mask] = saved[name][mask]
    t.episode = np.where(mask, env.world.episode.astype(np.uint32), t.episode)    # (the private counter is the record's: the restored episode's)
    back = t.untouched("behind the masked restore")
    assert (t.table != saved_table).any()
    for name in ("map", "here", "visited", "first", "level_here"):
        np.testing.assert_array_equal(back[name][~mask], moved[name][~mask], err_msg=name)
    rcw.act_(env, random_actions(rng))
    t.stepped("a step behind the restore")                                        # the restored counter matches the restored episode: nobody begins for it
    env.close()


def test_rows_of_another_sector_count_are_refused_and_a_handle_without_the_feature_keeps_its_key(rcw):
    from raycastworlds_jl_amd import _capi

    plain = make(rcw, 4, 5, 5, snapshots=4)
    key = plain.snapshot_info["shape_key"]
    plain.close()
    one, two = make(rcw, 4, 5, 5, visit_map=dict(sectors=1), snapshots=4), make(rcw, 4, 5, 5, visit_map=dict(sectors=2), snapshots=4)
    with_table = make(rcw, 4, 5, 5, visit_map=dict(sectors=1, table=True), snapshots=4)
    assert one.snapshot_info["shape_key"] not in (key, two.snapshot_info["shape_key"]) and two.snapshot_info["shape_key"] != key
    assert one.snapshot_info["row_bytes"] + 50 == two.snapshot_info["row_bytes"]
    assert with_table.snapshot_info["shape_key"] == one.snapshot_info["shape_key"]          # the table is no part of a record
    two.snapshot_save()
    with pytest.raises(ValueError):
        one.snapshot_import(two.snapshot_export())                                           # another shape key, another row size
    # a handle whose sectors changed behind the binding: the save names the segment
    one.set_visit_map(sectors=2)
    with pytest.raises(_capi.RcwError) as e:
        one.snapshot_save()
    assert e.value.code == _capi.RCW_ERR_UNSUPPORTED and "visit_map.map" in str(e.value), e.value
    one.set_visit_map(None)
    with pytest.raises(_capi.RcwError) as e:
        one.snapshot_save()
    assert "visit_map.here" in str(e.value), e.value
    one.set_snapshots(4)
    assert one.snapshot_info["shape_key"] == key                                             # off again: the key it had without the feature
    for e_ in (one, two, with_table):
        e_.close()


# ---- queued and captured ---------------------------------------------------------------------------------------------------------------------
def twins(rcw, rng_seed, **kw):
    out = []
    for _ in range(2):
        rng = np.random.default_rng(rng_seed)
        out.append(bank_env(rcw, rng, **kw))
    return out


def test_thirty_steps_queued_with_device_actions_and_no_sync(rcw):
    torch = pytest.importorskip("torch")
    read, queued = twins(rcw, 36)
    t = VR.Tracked(read, sectors=3, table=True)
    queued.set_visit_map(sectors=3, table=True)
    rng = np.random.default_rng(37)
    actions = [random_actions(rng) for _ in range(30)]
    for k, a in enumerate(actions):
        rcw.act_(read, a)
        t.stepped(f"step {k}")
    with torch.cuda.stream(queued.torch_stream()):
        device_actions = [torch.as_tensor(a).to("cuda", non_blocking=False) for a in actions]
        queued.sync()
        syncs = queued.host_syncs
        for a in device_actions:
            rcw.act_(queued, a)
        assert queued.host_syncs == syncs
    t.check("the queued twin", env=queued)
    assert t.seen["restarts"] >= 3 * B
    read.close()
    queued.close()


def test_a_captured_step_replayed_thirty_times(rcw):
    """one captured step with a fixed action array, replayed 30 times, against its twin stepped and read 30 times: the recorded episode
    counter lives on the device, so the restarts under the time limit begin the agents' maps inside the replays"""
    torch = pytest.importorskip("torch")
    read, replayed = twins(rcw, 38)
    t = VR.Tracked(read, sectors=1, table=True)
    replayed.set_visit_map(sectors=1, table=True)
    a = random_actions(np.random.default_rng(39))
    for k in range(32):
        rcw.act_(read, a)
        t.stepped(f"step {k}")
    stream = torch.cuda.Stream()
    replayed.sync()
    replayed.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        actions = torch.as_tensor(a).to("cuda")
        for _ in range(2):
            rcw.act_(replayed, actions)
        stream.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            rcw.act_(replayed, actions)
        for _ in range(30):
            g.replay()
        stream.synchronize()
    t.check("the replayed twin", env=replayed)
    assert t.seen["restarts"] >= 4 * B
    del g
    read.close()
    replayed.close()


# ---- the life cycle --------------------------------------------------------------------------------------------------------------------------
def test_enabling_disabling_and_what_a_handle_without_the_visit_map_launches(rcw):
    from raycastworlds_jl_amd import _capi, layouts

    UNSUPPORTED, BAD = _capi.RCW_ERR_UNSUPPORTED, _capi.RCW_ERR_INVALID_ARGUMENT
    env = make(rcw, B, 5, 7, nd=16, max_episode_steps=7)
    lib, h = env._lib, env._h
    p = [C.c_void_p() for _ in range(4)]
    q = C.c_void_p()
    out = np.zeros((B, 8 * 35), np.uint16)
    tab = np.zeros(8 * 35, np.uint32)
    kernels = (env.fill_kernel_name(), env.step_form())
    off = dict(enabled=False, sectors=0, table=False, rows=0, first=0)

    def getters_refuse():
        assert env.visit_map_info == off
        assert lib.rcw_visit_words(h, None, None, None, None) == UNSUPPORTED
        assert lib.rcw_visit_words_device_ptr(h, *[C.byref(v) for v in p]) == UNSUPPORTED
        assert lib.rcw_visit_map(h, 0, B, out.ctypes.data) == UNSUPPORTED and lib.rcw_visit_map_device_ptr(h, C.byref(q)) == UNSUPPORTED
        assert lib.rcw_visit_table(h, tab.ctypes.data) == UNSUPPORTED and lib.rcw_visit_table_device_ptr(h, C.byref(q)) == UNSUPPORTED
        assert lib.rcw_visit_table_clear(h) == UNSUPPORTED

    getters_refuse()
    assert not any(v.value for v in p) and not q.value
    assert lib.rcw_set_visit_map(h, 0, 0, 0) == 0                                  # RCW_OK also where there was none
    for sectors, flags in ((0, 0), (-1, 0), (9, 0), (17, 0), (1, 2), (1, -1)):
        assert lib.rcw_set_visit_map(h, 1, sectors, flags) == BAD, (sectors, flags)
    getters_refuse()
    rng = np.random.default_rng(40)
    t = VR.Tracked(env, sectors=3)
    assert lib.rcw_visit_table(h, tab.ctypes.data) == UNSUPPORTED and "table" in _capi.last_error(lib)   # on, without the table
    assert lib.rcw_visit_table_device_ptr(h, C.byref(q)) == UNSUPPORTED and lib.rcw_visit_table_clear(h) == UNSUPPORTED
    assert lib.rcw_visit_words(h, None, None, None, None) == 0                     # any pointer may be NULL
    assert lib.rcw_visit_words_device_ptr(h, C.byref(p[0]), None, None, None) == 0 and lib.rcw_visit_words_device_ptr(h, None, C.byref(p[1]), C.byref(p[2]), C.byref(p[3])) == 0
    words = (env.visits_here, env.visited_cells, env.visit_first, env.level_visits_here)
    assert [v.value for v in p] == [w.ptr for w in words] and all(v.value % 16 == 0 for v in p)
    assert lib.rcw_visit_map_device_ptr(h, C.byref(q)) == 0 and q.value == env.visit_map_device.ptr and q.value % 16 == 0
    assert lib.rcw_visit_map_device_ptr(h, None) == BAD
    for k in range(6):
        rcw.act_(env, random_actions(rng))
        exp = t.stepped(f"step {k}")
    # a range of the map, the refused ranges, the map where it lives
    part = np.zeros((5, 3, 7, 5), np.uint16)
    assert lib.rcw_visit_map(h, 7, 5, part.ctypes.data) == 0
    np.testing.assert_array_equal(part.transpose(0, 1, 3, 2), exp["map"][7:12])
    assert lib.rcw_visit_map(h, B - 2, 3, part.ctypes.data) == BAD and lib.rcw_visit_map(h, 0, 5, None) == BAD
    np.testing.assert_array_equal(env.visit_map_device.numpy().transpose(0, 1, 3, 2), exp["map"])
    # the handle-less export on the engine's own poses: the counted cell is the one entry `here` names
    pos, dirs = env.world.player_position_wu, env.world.player_direction_au
    flat = env.visit_map_device.numpy().reshape(B, -1)
    for b in range(0, B, 5):
        c = layouts.visit_cell(5, 7, 16, 3, pos[b], dirs[b], env.T)
        assert c >= 0 and flat[b, c] == exp["here"][b]
    # again with other parameters: everything begins afresh; and the table
    t = VR.Tracked(env, sectors=8, table=True)
    assert env.visit_map_info == dict(enabled=True, sectors=8, table=True, rows=0, first=0)
    assert lib.rcw_visit_table(h, None) == BAD and lib.rcw_visit_table_device_ptr(h, None) == BAD
    assert lib.rcw_visit_table(h, tab.ctypes.data) == 0 and int(tab.sum()) == B
    assert lib.rcw_visit_table_device_ptr(h, C.byref(q)) == 0 and q.value == env.visit_table(device=True).ptr and q.value % 16 == 0
    rcw.act_(env, random_actions(rng))
    t.stepped("a step with eight sectors and the table")
    assert (env.fill_kernel_name(), env.step_form()) == kernels
    # off, and on again
    env.set_visit_map(None)
    getters_refuse()
    assert (env.fill_kernel_name(), env.step_form()) == kernels                   # off -> on -> off: the handle launches what it did
    rcw.act_(env, random_actions(rng))
    env.sync()
    t = VR.Tracked(env, sectors=1)
    rcw.act_(env, random_actions(rng))
    t.stepped("a step behind off and on again")
    env.close()


def test_the_constructor_keyword(rcw):
    env = make(rcw, 5, 5, 5, visit_map=True)
    assert env.visit_map_info == dict(enabled=True, sectors=1, table=False, rows=0, first=0) and list(env.visits_here.numpy()) == [1] * 5
    env.close()
    env = make(rcw, 5, 5, 5, visit_map=dict(sectors=4, table=True))
    assert env.visit_map_info == dict(enabled=True, sectors=4, table=True, rows=0, first=0) and env.visit_map.shape == (5, 4, 5, 5)
    env.close()


# ---- the example -----------------------------------------------------------------------------------------------------------------------------
def test_the_example_prints_the_bonus_and_the_coverage():
    """examples/count_bonus.py as a user would run it, in a process of its own: 128 agents, 150 steps"""
    import os
    import re
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "examples/count_bonus.py", "128", "150"], cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"128 agents x 150 random steps: mean episodic bonus ([\d.]+) a step \(beta 0.1\), ([\d.]+) of the steps entered a new cell", r.stdout)
    assert m and 0.0 < float(m.group(1)) <= 0.1 and 0.0 < float(m.group(2)) < 1.0, r.stdout
    levels = re.findall(r"level (\d+): (\d+) visits, (\d+) of (\d+) free tiles covered", r.stdout)
    assert [int(v[0]) for v in levels] == [0, 1, 2] and sum(int(v[1]) for v in levels) == 128 * 151, r.stdout
    assert all(0 < int(v[2]) <= int(v[3]) for v in levels), r.stdout
