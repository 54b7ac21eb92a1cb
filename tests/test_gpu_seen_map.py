"""The seen map on the GPU (include/rcw.h, rcw_set_seen_map): after EVERY call the three words and the whole map of every agent are compared
for equality with tests/seen_map_ref.py, which is fed the state the engine itself reports (both layers of the tile map, goal, position,
heading, episode counter), the engine's own ray table and which agents an explicit call masked.  State parity with the oracle is the rest of
the suite's job.

The kernel has ONE path for every map size (a byte per tile and the bitmap of marked tiles in LDS): maps up to 58,239 tiles launch with the
default dynamic-LDS limit, larger ones after the limit is raised — the 254 x 254 case takes that branch of the launcher, every other case
the first.  The shapes are the smallest at which it can go wrong: one ray (one live lane), 63 tiles (one partial bitmap word), 65 tiles (a
second word holding one bit), 33 and 257 rays (a partial wavefront, one ray past the workgroup), interior walls, a maze per agent.

tests/test_seen_map_spec.py rehearses the rollouts below with the Python dynamics: every event asserted here happens there."""
import ctypes as C

import numpy as np
import pytest

import seen_map_ref as SM
import walls_ref as WR

pytestmark = pytest.mark.gpu

FAST = dict(num_directions=16, position_increment_wu=0.25, player_radius_wu=0.3)    # a tile in four moves, sixteen headings: new tiles at most steps
Tracked = SM.Tracked


def make_env(rcw, B, H, W, N=33, Hc=24, seed=5, form=None, **kw):
    env = rcw.SingleRoomModule.SingleRoom(batch=B, seed=seed, auto_reset=kw.pop("auto_reset", True), height_tile_map_tu=H, width_tile_map_tu=W,
                                          num_rays=N, height_camera_view_pu=Hc, **{**FAST, **kw})
    if form is not None:
        env.set_step_form(form)
        assert env.step_form() == form
    return env


def all_events(t, but=()):
    assert all(v > 0 for k, v in t.events.items() if k not in but), t.events


# ---- 1  the shapes ------------------------------------------------------------------------------------------------------------------
def mazes(n, seed=9):
    from raycastworlds_jl_amd import layouts

    rng = np.random.default_rng(seed)
    return np.stack([layouts.maze(9, 9, rng) for _ in range(n)])


SHAPES = {
    "4x4-1ray": (lambda: SM.ring(4, 4), 1, ()),
    "7x9-63tiles": (lambda: SM.ring(7, 9), 33, ()),
    "5x13-65tiles-257rays": (lambda: SM.ring(5, 13), 257, ()),
    "crossed": (SM.crossed, 33, ()),
    "mazes": (lambda: mazes(64), 33, ()),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes(rcw, name):
    layout, N, rare = SHAPES[name]
    walls = layout()
    H, W = walls.shape[-2:]
    env = make_env(rcw, 64, H, W, N=N)
    env.set_walls(walls)
    env.set_time_limit(12)
    t = Tracked(rcw, env)
    if walls.ndim == 3:
        assert len({m.tobytes() for m in t.ref.map}) > 32                   # (the maps are the agents' own)
    raw = np.zeros((64, H * W), np.uint8)                                   # the export itself: tile (i, j) at (i - 1) + H (j - 1)
    assert env._lib.rcw_seen_map(env._h, 0, 64, raw.ctypes.data) == 0
    np.testing.assert_array_equal(raw, t.ref.maps_linear)
    t.rollout(40, 6, name)
    all_events(t, but=rare)
    assert (t.ref.map == 2).any() and (t.ref.map == 3).any() and t.ref.map.max() == 3
    env.close()


def test_the_largest_map(rcw):
    """254 x 254: the largest square map rcw_create accepts, 71 KiB of LDS — the raised limit.  A reset, a set_state that puts one player
    next to the last interior tile (the largest tile indices there are), five steps."""
    H = W = 254
    env = make_env(rcw, 2, H, W, N=64)
    t = Tracked(rcw, env)
    goal = np.array([(2, 2), (H - 1, W - 1)], np.int32)
    pos = np.array([(H - 1.5, W - 2.5), (1.5, 1.5)], np.float32)
    env.set_state(goal, pos, np.array([4, 2], np.int32))                   # heading 4 of 16: (0, 1), towards the ring at j = W
    t.masked(None, "254 x 254: set_state")
    assert t.ref.map[0, H - 2, W - 1] == 2 and np.flatnonzero(SM.linear(t.ref.map[0])).max() > 64000
    assert t.ref.seen_count[1] > 100                                        # (the fan from the first interior corner crosses the room)
    rcw.reset_(env)
    t.masked(None, "254 x 254: reset")
    t.rollout(5, 1, "254 x 254")
    env.close()


# ---- 2  the rollouts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("auto_reset", [True, False])
@pytest.mark.parametrize("form,N,Hc", [("two-launches", 33, 24), ("one-launch", 64, 256)])
def test_both_step_forms(rcw, form, N, Hc, auto_reset):
    env = make_env(rcw, 64, 9, 9, N=N, Hc=Hc, form=form, auto_reset=auto_reset)
    env.set_walls(SM.crossed())
    env.set_time_limit(12)
    t = Tracked(rcw, env)
    t.rollout(40, 6, f"crossed ({form}, auto_reset {auto_reset})")
    assert env.step_form() == form
    if auto_reset:
        all_events(t)
    else:
        all_events(t, but=("restart_after_done", "restart_after_truncation"))
        assert t.events["restart_after_done"] == 0 and t.events["restart_after_truncation"] == 0 and env.world.truncated.any()
    env.close()


@pytest.mark.parametrize("T,tie", [("Float32", 1), ("Float64", 0), ("Float64", 1)])       # (Float32, tie 0: every other test)
def test_the_other_instantiations(rcw, T, tie):
    env = make_env(rcw, 64, 9, 9, T=T, dda_tie_break=tie)
    env.set_walls(SM.crossed())
    env.set_time_limit(12)
    t = Tracked(rcw, env)
    assert env.world.player_position_wu.dtype == (np.float64 if T == "Float64" else np.float32) and t.ref.tie_le == bool(tie) and t.ref.table.dtype == env.T
    t.rollout(40, 6, f"{T}, tie {tie}")
    all_events(t)
    env.close()


# ---- 3  masked calls ------------------------------------------------------------------------------------------------------------------
def test_masked_calls(rcw):
    B, H, W = 12, 9, 9
    env = make_env(rcw, B, H, W)
    env.set_walls(SM.crossed())
    t = Tracked(rcw, env)
    t.rollout(6, 2, "before the masked calls")

    def words():
        return env.seen_map, env.seen_count.numpy(), env.seen_new.numpy(), env.goal_seen.numpy()

    def kept(before, mask, where):
        for now, was in zip(words(), before):
            np.testing.assert_array_equal(now[mask == 0], was[mask == 0], err_msg=where)

    mask = (np.arange(B) % 3 == 0).astype(np.uint8)
    before = words()
    rcw.reset_(env, mask)
    t.masked(mask, "masked reset_")
    kept(before, mask, "masked reset_")
    t.rollout(3, 3, "between")
    # set_state: the goal of the masked agents into an interior wall, the player looking at it along i; the episode counter stays
    ep = env.world.episode.copy()
    goal, pos, head = env.world.goal_position.copy(), env.world.player_position_wu.copy(), env.world.player_direction_au.copy()
    mask2 = (np.arange(B) % 4 == 1).astype(np.uint8)
    goal[mask2 != 0] = (5, 4)                                               # a tile of the cross
    pos[mask2 != 0] = (2.5, 3.5)
    head[mask2 != 0] = 0                                                    # (1, 0): i grows
    before = words()
    env.set_state(goal, pos, head, mask=mask2)
    np.testing.assert_array_equal(env.world.episode, ep)
    t.masked(mask2, "masked set_state: a goal in a wall")
    kept(before, mask2, "masked set_state")
    assert (env.seen_map[mask2 != 0][:, 4, 3] == 4).all() and (env.goal_seen.numpy()[mask2 != 0] == 1).all()
    t.rollout(3, 4, "between")
    # a player put on an obstacle tile marks that tile alone
    mask3 = (np.arange(B) % 4 == 2).astype(np.uint8)
    goal, pos, head = env.world.goal_position.copy(), env.world.player_position_wu.copy(), env.world.player_direction_au.copy()
    pos[mask3 != 0] = (4.5, 3.5)                                            # tile (5, 4) of the cross
    before = words()
    env.set_state(goal, pos, head, mask=mask3)
    t.masked(mask3, "masked set_state: a player on a wall tile")
    kept(before, mask3, "masked set_state (2)")
    assert (env.seen_count.numpy()[mask3 != 0] == 1).all() and (env.seen_map[mask3 != 0][:, 4, 3] == 2).all()
    mask4 = (np.arange(B) % 2 == 0).astype(np.uint8)
    before = words()
    env.set_walls(SM.ring(H, W), mask=mask4)
    t.masked(mask4, "masked set_walls")
    kept(before, mask4, "masked set_walls")
    t.rollout(6, 5, "behind the masked calls")
    env.close()


# ---- 4  calls that must do nothing -------------------------------------------------------------------------------------------------------
def test_calls_that_do_nothing(rcw):
    env = make_env(rcw, 16, 9, 9, N=64, Hc=64)
    env.set_walls(SM.crossed())
    t = Tracked(rcw, env)
    t.rollout(5, 1, "before")
    assert t.ref.newly_seen.any()
    rcw.cast_rays_(env)
    t.check("behind cast_rays")
    rcw.update_camera_view_(env)
    t.check("behind update_camera_view")
    env.set_step_form("one-launch")
    t.check("behind set_step_form")
    env.set_step_form("two-launches")
    env.set_time_limit(7)
    t.check("behind set_time_limit")
    env.set_learner_view("gray", (16, 16))
    t.check("behind set_learner_view")
    env.set_goal_distance(True)
    t.check("behind set_goal_distance")
    nd = env.cfg.num_directions
    theta = 2 * np.pi * np.arange(nd) / nd + 0.3                            # every heading turned by 0.3 rad
    t.set_direction_table(np.stack([np.cos(theta), np.sin(theta)], axis=1))
    before = t.ref.seen_count.copy()
    t.step(np.full(16, 1, np.uint8), "the step behind set_direction_table")
    assert (t.ref.seen_count > before).any()                                # ... marks with the new rays
    t.rollout(5, 2, "behind")
    env.close()


# ---- 5  error paths -------------------------------------------------------------------------------------------------------------------
def test_an_invalid_device_action(rcw):
    torch = pytest.importorskip("torch")
    B = 32
    env = make_env(rcw, B, 9, 9)
    env.set_walls(SM.crossed())
    t = Tracked(rcw, env)
    t.rollout(4, 1, "before")
    a = WR.draw_actions(np.random.default_rng(2), B)
    bad = np.arange(B) % 5 == 0
    a[bad] = np.array([0, 5, 255, 9, 77, 200, 6], np.uint8)[: bad.sum()]
    pose = env.world.player_position_wu.copy(), env.world.player_direction_au.copy()
    rcw.act_(env, torch.from_numpy(a).cuda())
    with pytest.raises(AssertionError, match="invalid action"):
        env.sync()
    env.clear_error()
    t.stepped(a, "an invalid device action")
    assert (env.seen_new.numpy()[bad] == 0).all() and (env.seen_new.numpy()[~bad] > 0).any()
    np.testing.assert_array_equal(env.world.player_position_wu[bad], pose[0][bad])
    t.rollout(4, 3, "behind")
    env.close()


@pytest.mark.parametrize("form", ["two-launches", "one-launch"])
def test_a_raising_move_with_the_feature_on(rcw, form):
    """out_of_bounds = 0 in the 4 x 4 room of tests/test_gpu_time_limit.py (a quarter-tile move next to the ring tests a neighbourhood that
    leaves the map: 19 of its 24 steps raise there): the step leaves an IndexError for the next sync.  The kernel behind that step ran all
    the same: after each raise, cleared the way those tests clear it, words and maps equal the reference fed from the state the engine
    reports — an agent the raise left where it was has newly_seen 0 — and the steps behind it go on."""
    import time_limit_ref as TL

    B = 64
    env = rcw.SingleRoomModule.SingleRoom(batch=B, seed=7, auto_reset=True, height_tile_map_tu=4, width_tile_map_tu=4, num_rays=64,
                                          height_camera_view_pu=64, num_directions=8, position_increment_wu=0.25, out_of_bounds=0)
    env.set_step_form(form)
    env.set_time_limit(4)
    t = Tracked(rcw, env, raising=True)
    rng = np.random.default_rng(8)
    for k in range(24):
        t.step(TL.draw_actions(rng, B, k, 0), f"raising ({form}): step {k}")
    assert env.step_form() == form
    assert t.steps_that_raised == 19, t.steps_that_raised                  # (that module's rehearsal of rollout A: the same seed and actions)
    assert t.events["restart_after_truncation"] > 0 and t.events["no_new_blocked"] > 0, t.events
    env.sync()
    env.close()


# ---- 6  off and on ---------------------------------------------------------------------------------------------------------------------
def test_off_and_on(rcw, oracle):
    from raycastworlds_jl_amd import _capi

    cfg = dict(height_tile_map_tu=8, width_tile_map_tu=8, num_rays=64)
    env = rcw.SingleRoomModule.SingleRoom(batch=32, seed=3, **cfg)
    orc = oracle.OracleBatch(32, seed=3, **cfg)
    lib, h = env._lib, env._h
    p, n = C.c_void_p(), C.c_int32(-1)
    words = np.zeros(32, np.int32)
    maps = np.zeros((32, 64), np.uint8)

    def readers():
        return (lib.rcw_seen_words(h, words.ctypes.data, None, None), lib.rcw_seen_words_device_ptr(h, C.byref(p), None, None),
                lib.rcw_seen_map(h, 0, 32, maps.ctypes.data), lib.rcw_seen_map_device_ptr(h, C.byref(p)))

    assert readers() == (_capi.RCW_ERR_UNSUPPORTED,) * 4
    assert lib.rcw_seen_map_enabled(h, C.byref(n)) == 0 and n.value == 0 and not env.seen_map_enabled
    assert lib.rcw_set_seen_map(h, 0) == 0
    with pytest.raises(_capi.RcwError):
        env.seen_count
    rng = np.random.default_rng(0)

    def steps(k):
        for _ in range(k):
            a = rng.integers(1, 5, 32).astype(np.uint8)
            rcw.act_(env, a)
            orc.step(a)

    steps(10)
    t = Tracked(rcw, env)                                                  # enabled mid-episode: what the current pose sees, newly_seen 0
    assert not env.seen_new.numpy().any() and (env.seen_count.numpy() > 0).all()
    assert readers() == (0,) * 4 and p.value == env.seen_map_device.ptr
    assert env.seen_map_device.shape == (32, 8, 8) and env.seen_map_device.dtype == np.uint8
    for k in range(10):
        a = rng.integers(1, 5, 32).astype(np.uint8)
        t.step(a, f"on: step {k}")
        orc.step(a)
    grown = env.seen_count.numpy().copy()
    env.set_seen_map(True)                                                 # again: afresh, from the current state
    t.masked(None, "enabled again")
    assert (env.seen_count.numpy() <= grown).all() and (env.seen_count.numpy() < grown).any()
    env.set_seen_map(False)
    assert readers() == (_capi.RCW_ERR_UNSUPPORTED,) * 4 and not env.seen_map_enabled
    steps(10)
    np.testing.assert_array_equal(env.camera_view_host(), orc.camera_view)   # a handle without it equals the oracle as before
    np.testing.assert_array_equal(env.world.player_position_wu, orc.position)
    env.close()
    orc.close()


def test_constructor_keyword_and_torch_alias(rcw):
    """SingleRoom(seen_map=True), and the bonus expression of the README on the device"""
    torch = pytest.importorskip("torch")
    env = make_env(rcw, 8, 7, 9, seen_map=True)
    assert env.seen_map_enabled
    t = Tracked(rcw, env, enable=False)
    t.rollout(5, 1, "constructor keyword")
    bonus = torch.as_tensor(env.world.reward, device="cuda") + 0.01 * env.seen_new.torch(sync=True)
    np.testing.assert_allclose(bonus.cpu().numpy(), env.world.reward + np.float32(0.01) * t.ref.newly_seen.astype(np.float32), rtol=0, atol=1e-7)
    assert env.seen_count.torch(sync=False).dtype == torch.int32 and env.goal_seen.torch(sync=True).cpu().numpy().tolist() == t.ref.goal_seen.tolist()
    dev = env.seen_map_device.torch(sync=True)
    assert dev.dtype == torch.uint8 and tuple(dev.shape) == (8, 9, 7)
    np.testing.assert_array_equal(dev.cpu().numpy().transpose(0, 2, 1), t.ref.map)
    env.close()


def test_map_export_sub_ranges(rcw):
    """rcw_seen_map(h, first, count, out) with a maze per agent, so that every row differs: each sub-range holds the reference's rows and
    nothing is written in front of or behind them; a count of zero is an empty copy, a range past the batch is refused."""
    from raycastworlds_jl_amd import _capi

    B, size = 9, 9
    env = make_env(rcw, B, size, size)
    env.set_walls(mazes(B, seed=13))
    t = Tracked(rcw, env)
    t.rollout(3, 2, "sub-ranges")
    want = t.ref.maps_linear
    assert len({w.tobytes() for w in want}) == B
    lib, h, HW, canary = env._lib, env._h, size * size, 0xA5

    def read(first, count):
        buf = np.full((max(count, 0) + 2, HW), canary, np.uint8)          # a canary row in front of the output and one behind it
        rc = lib.rcw_seen_map(h, first, count, buf[1:].ctypes.data)
        return rc, buf

    for first, count in ((3, 5), (B - 1, 1), (0, 1), (0, B), (4, 0)):
        rc, buf = read(first, count)
        assert rc == 0, (first, count, _capi.last_error(lib))
        np.testing.assert_array_equal(buf[1:1 + count], want[first:first + count], err_msg=f"rows [{first}, {first + count})")
        assert (buf[0] == canary).all() and (buf[-1] == canary).all(), (first, count)
    for first, count in ((-1, 2), (0, -1), (B - 1, 2), (B, 1), (0, B + 1)):
        rc, buf = read(first, count)
        assert rc == _capi.RCW_ERR_INVALID_ARGUMENT, (first, count, rc)
        assert (buf == canary).all(), (first, count)
    assert lib.rcw_seen_map(h, 0, 1, None) == _capi.RCW_ERR_INVALID_ARGUMENT
    t.check("behind the refusals")
    env.close()


# ---- 7  a captured step ---------------------------------------------------------------------------------------------------------------
def test_a_captured_step_replays(rcw):
    torch = pytest.importorskip("torch")
    B = 32
    env = make_env(rcw, B, 9, 9)
    env.set_walls(SM.crossed())
    env.set_time_limit(3)
    t = Tracked(rcw, env)
    stream = torch.cuda.Stream()
    env.sync()
    env.set_stream(stream.cuda_stream)
    a_host = WR.draw_actions(np.random.default_rng(4), B)
    with torch.cuda.stream(stream):
        actions = torch.from_numpy(a_host).cuda()
        stream.synchronize()
        ptr = env.seen_count.ptr
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            rcw.act_(env, actions)                                         # (captured, not run)
        for k in range(6):
            g.replay()
            stream.synchronize()
            t.stepped(a_host, f"replay {k}")
        assert env.seen_count.ptr == ptr
        stream.synchronize()
    assert t.events["restart_after_truncation"] > 0 and t.events["new_after_turn"] + t.events["new_after_move"] > 0, t.events
    del g
    env.close()


# ---- 8  sharding --------------------------------------------------------------------------------------------------------------------------
def test_two_shards_equal_their_slices_of_the_whole_batch(rcw):
    G, WORLD = 16, 2
    kw = dict(seed=5, auto_reset=True, height_tile_map_tu=9, width_tile_map_tu=9, num_rays=33, height_camera_view_pu=24, **FAST)
    whole = rcw.SingleRoomModule.SingleRoom(batch=G, **kw)
    shards = [rcw.ShardedSingleRoom(G, rank=r, world=WORLD, device=0, **kw) for r in range(WORLD)]
    walls = mazes(G, seed=21)
    whole.set_walls(walls)
    whole.set_time_limit(6)
    t = Tracked(rcw, whole)
    for sh in shards:
        sh.set_walls(walls)
        sh.env.set_time_limit(6)
        sh.env.set_seen_map()
        assert sh.env.seen_map_enabled

    def compare(where):
        for sh in shards:
            rows = slice(sh.first, sh.first + sh.count)
            np.testing.assert_array_equal(sh.env.world.episode, whole.world.episode[rows], err_msg=where)
            np.testing.assert_array_equal(sh.env.seen_map, t.ref.map[rows], err_msg=f"map, {where}")
            for name, want in (("seen_count", t.ref.seen_count), ("seen_new", t.ref.newly_seen), ("goal_seen", t.ref.goal_seen)):
                np.testing.assert_array_equal(getattr(sh.env, name).numpy(), want[rows], err_msg=f"{name}, {where}")

    compare("switched on")
    rng = np.random.default_rng(3)
    for k in range(20):
        a = WR.draw_actions(rng, G)
        t.step(a, f"whole batch: step {k}")
        for sh in shards:
            sh.act_(sh.local_slice(a))
        compare(f"step {k}")
    assert t.events["restart_after_truncation"] > 0 and t.events["new_after_move"] > 0, t.events
    for sh in shards:
        sh.close()
    whole.close()
