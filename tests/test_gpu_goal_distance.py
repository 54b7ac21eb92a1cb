"""The goal distance on the GPU (include/rcw.h, rcw_set_goal_distance): after EVERY call the three words and the whole field of every agent
are compared for equality with tests/goal_distance_ref.py, which is fed the state the engine itself reports (walls, goal, position, episode
counter) and which agents an explicit call masked.  State parity with the oracle is the rest of the suite's job.

The kernel has ONE path for every map size (walls and visited bits plus the queue in LDS, the field written to HBM and never read by the
flood): maps up to 180 x 180 launch with the default dynamic-LDS limit, larger ones after the limit is raised — the 200 x 300 case takes
that branch of the launcher, every other case the first.

The pocket rollout rehearsed on the CPU with TimeLimitRef(WallsRef(render=False)) and GoalDistanceRef over the same seed and actions (B = 64,
limit 20, 200 steps, engine seed 5, actions from seed 6): 1656 agent-steps at distance -1, 54 restarts after done, 559 after a truncation,
261 agent-steps with positive progress and 280 with negative.  The engine's own counts must be these."""
import ctypes as C

import numpy as np
import pytest

import goal_distance_ref as GD
import walls_ref as WR

pytestmark = pytest.mark.gpu

FAST = dict(num_directions=8, position_increment_wu=0.25, player_radius_wu=0.3)     # a tile in four moves: rollouts that get somewhere


def make_env(rcw, B, H, W, N=8, Hc=24, seed=5, form=None, **kw):
    env = rcw.SingleRoomModule.SingleRoom(batch=B, seed=seed, auto_reset=kw.pop("auto_reset", True), height_tile_map_tu=H, width_tile_map_tu=W,
                                          num_rays=N, height_camera_view_pu=Hc, **FAST, **kw)
    if form is not None:
        env.set_step_form(form)
        assert env.step_form() == form
    return env


class Tracked:
    """An engine with the feature on and the reference beside it; every method makes the call on the engine, tells the reference what the
    header's table says the call does, and compares everything."""

    def __init__(self, rcw, env, enable=True):
        self.rcw, self.env = rcw, env
        self.events = dict(unreachable=0, restart_after_done=0, restart_after_truncation=0, progress_up=0, progress_down=0)
        self._walls = None
        if enable:
            env.set_goal_distance(True)
            assert env.goal_distance_enabled
        self.ref = GD.GoalDistanceRef(*self.state())
        self._flags()
        self.check("enabled")

    def state(self, walls_changed=True):
        w = self.env.world
        if walls_changed or self._walls is None:
            self._walls = w.walls
        return self._walls, w.goal_position, w.player_position_wu, w.episode

    def _flags(self):
        w = self.env.world
        self.done, self.truncated = w.done.astype(bool), w.truncated.astype(bool)

    def check(self, where):
        env, ref = self.env, self.ref
        np.testing.assert_array_equal(env.goal_distance.numpy(), ref.distance, err_msg=f"distance {where}")
        np.testing.assert_array_equal(env.goal_start_distance.numpy(), ref.start_distance, err_msg=f"start_distance {where}")
        np.testing.assert_array_equal(env.goal_progress.numpy(), ref.progress, err_msg=f"progress {where}")
        field = env.goal_distance_field
        assert field.dtype == np.uint16 and field.shape == ref.fields.shape
        np.testing.assert_array_equal(field, ref.fields, err_msg=f"field {where}")

    def step(self, actions, where):
        ep0 = self.ref.recorded.copy()
        self.rcw.act_(self.env, actions)
        self.ref.stepped(*self.state(walls_changed=False))
        moved = self.env.world.episode != ep0
        ev = self.events
        ev["restart_after_done"] += int((moved & self.done).sum())
        ev["restart_after_truncation"] += int((moved & self.truncated & ~self.done).sum())
        ev["unreachable"] += int((self.ref.distance < 0).sum())
        ev["progress_up"] += int((self.ref.progress > 0).sum())
        ev["progress_down"] += int((self.ref.progress < 0).sum())
        self._flags()
        self.check(where)

    def masked(self, mask, where):
        """behind a reset_ / set_state / set_walls the caller has just made with `mask`"""
        self.ref.masked(*self.state(), mask)
        self._flags()
        self.check(where)
        m = np.ones(self.env.batch, bool) if mask is None else np.asarray(mask) != 0
        np.testing.assert_array_equal(self.ref.start_distance[m], self.ref.distance[m])
        assert (self.ref.progress[m] == 0).all()

    def rollout(self, steps, seed, where):
        rng = np.random.default_rng(seed)
        for t in range(steps):
            self.step(WR.draw_actions(rng, self.env.batch), f"{where}: step {t}")


# ---- 1  the pocket rollout ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,N,Hc", [("two-launches", 8, 24), ("one-launch", 64, 256)])
def test_pocket_rollout(rcw, form, N, Hc):
    env = make_env(rcw, 64, 7, 7, N=N, Hc=Hc, form=form)
    env.set_walls(GD.pocket())
    env.set_time_limit(20)
    t = Tracked(rcw, env)
    t.rollout(200, 6, f"pocket ({form})")
    assert env.step_form() == form
    assert all(v > 0 for v in t.events.values()), t.events
    assert t.events == dict(unreachable=1656, restart_after_done=54, restart_after_truncation=559, progress_up=261, progress_down=280), t.events
    env.close()


# ---- 2  a non-square map: the transposition trap -------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,Hc", [("two-launches", 24), ("one-launch", 256)])
def test_non_square_map(rcw, form, Hc):
    H, W = 5, 7
    walls = np.zeros((H, W), bool)
    walls[[0, -1], :] = True
    walls[:, [0, -1]] = True
    walls[2, 2] = True                                                     # (3, 3): off-centre in both axes
    env = make_env(rcw, 16, H, W, N=320, Hc=Hc, form=form)
    env.set_walls(walls)
    env.set_time_limit(10)
    t = Tracked(rcw, env)
    raw = np.zeros((16, H * W), np.uint16)                                  # the export itself: tile (i, j) at (i - 1) + H (j - 1)
    assert env._lib.rcw_goal_distance_field(env._h, 0, 16, raw.ctypes.data) == 0
    for k in range(16):
        np.testing.assert_array_equal(raw[k], GD.linear(t.ref.field[k]))
    assert any((raw[k] != np.ascontiguousarray(t.ref.field[k]).reshape(-1)).any() for k in range(16))      # (and not its transpose)
    t.rollout(40, 3, f"5 x 7 ({form})")
    assert t.events["progress_up"] > 0 and t.events["restart_after_truncation"] > 0, t.events
    env.close()


# ---- 3  a maze per agent -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [9, 32])
def test_per_agent_mazes(rcw, size):
    from raycastworlds_jl_amd import layouts

    rng = np.random.default_rng(size)
    mazes = np.stack([layouts.maze(size, size, rng) for _ in range(32)])
    env = make_env(rcw, 32, size, size, N=64, Hc=64)
    env.set_walls(mazes)
    env.set_time_limit(30)
    t = Tracked(rcw, env)
    assert len({f.tobytes() for f in t.ref.field}) == 32                   # (the fields are the agents' own)
    t.rollout(100, size + 1, f"mazes {size}")
    assert t.events["restart_after_truncation"] > 0 and t.events["progress_up"] > 0 and t.events["progress_down"] > 0, t.events
    env.close()


# ---- 4  the largest map class -------------------------------------------------------------------------------------------------------
def test_largest_map_serpentine(rcw):
    """200 x 300, one corridor of about 30,000 tiles: the flood's levels hold one tile each, and the launch needs the raised LDS limit."""
    H, W = 200, 300
    env = make_env(rcw, 2, H, W, N=8, Hc=24)
    env.set_walls(GD.serpentine(H, W))
    t = Tracked(rcw, env)
    reach = t.ref.fields[t.ref.fields != GD.UNREACHED]
    assert int(reach.max()) > 10000, int(reach.max())
    rcw.reset_(env)
    t.masked(None, "serpentine: reset")
    t.rollout(5, 1, "serpentine")
    env.close()


# ---- 5  masked calls ------------------------------------------------------------------------------------------------------------------
def test_masked_calls(rcw):
    from raycastworlds_jl_amd import layouts

    B, H, W = 12, 9, 11
    env = make_env(rcw, B, H, W, N=16, Hc=24)
    env.set_walls(layouts.four_rooms(H, W))
    t = Tracked(rcw, env)
    t.rollout(6, 2, "before the masked calls")
    mask = (np.arange(B) % 3 == 0).astype(np.uint8)
    before = env.goal_distance_field
    rcw.reset_(env, mask)
    t.masked(mask, "masked reset_")
    np.testing.assert_array_equal(env.goal_distance_field[mask == 0], before[mask == 0])
    # set_state moves the goal of the masked agents; the episode counter stays: the mask decides
    t.rollout(3, 3, "between")
    ep = env.world.episode.copy()
    goal = env.world.goal_position.copy()
    pos = env.world.player_position_wu.copy()
    head = env.world.player_direction_au.copy()
    mask2 = (np.arange(B) % 4 == 1).astype(np.uint8)
    goal[mask2 != 0] = (2, 2)
    pos[mask2 != 0] = (H - 1.5, W - 1.5)
    before = env.goal_distance_field
    env.set_state(goal, pos, head, mask=mask2)
    np.testing.assert_array_equal(env.world.episode, ep)
    t.masked(mask2, "masked set_state")
    after = env.goal_distance_field
    np.testing.assert_array_equal(after[mask2 == 0], before[mask2 == 0])
    assert (after[mask2 != 0][:, 1, 1] == 0).all() and (env.goal_distance.numpy()[mask2 != 0] == (H - 3) + (W - 3)).all()
    t.rollout(3, 4, "between")
    mask3 = (np.arange(B) % 2 == 0).astype(np.uint8)
    before = env.goal_distance_field
    env.set_walls(GD.serpentine(H, W), mask=mask3)
    t.masked(mask3, "masked set_walls")
    np.testing.assert_array_equal(env.goal_distance_field[mask3 == 0], before[mask3 == 0])
    t.rollout(6, 5, "behind the masked calls")
    env.close()


# ---- 6  the goal in a wall ------------------------------------------------------------------------------------------------------------
def test_goal_in_a_wall(rcw):
    B = 4
    env = make_env(rcw, B, 7, 7, auto_reset=False)
    env.set_walls(GD.pocket())
    t = Tracked(rcw, env)
    goal = np.tile(np.array([3, 3], np.int32), (B, 1))                     # an interior WALL tile of the pocket layout
    pos = np.tile(np.array([1.5, 1.5], np.float32), (B, 1))
    env.set_state(goal, pos, np.zeros(B, np.int32))
    t.masked(None, "goal in a wall")
    assert (env.goal_distance_field == GD.UNREACHED).all()
    assert (env.goal_distance.numpy() == -1).all() and (env.goal_start_distance.numpy() == -1).all()
    t.rollout(4, 1, "goal in a wall")
    env.sync()
    env.close()


# ---- 7  Float64 -----------------------------------------------------------------------------------------------------------------------
def test_float64_world(rcw):
    from raycastworlds_jl_amd import layouts

    env = make_env(rcw, 16, 9, 9, N=16, Hc=24, T="Float64")
    env.set_walls(layouts.four_rooms(9, 9))
    env.set_time_limit(12)
    t = Tracked(rcw, env)
    assert env.world.player_position_wu.dtype == np.float64
    t.rollout(40, 8, "Float64")
    assert t.events["progress_up"] > 0 and t.events["restart_after_truncation"] > 0, t.events
    env.close()


# ---- 8  views ---------------------------------------------------------------------------------------------------------------------------
def test_views_do_not_change_the_words(rcw):
    """a frame stack, RCW_VIEW_ONLY and the top view beside a plain handle: same seed, same actions, the same words"""
    from raycastworlds_jl_amd import layouts

    def make(**kw):
        env = make_env(rcw, 16, 9, 9, N=32, Hc=32, **kw)
        env.set_walls(layouts.four_rooms(9, 9))
        env.set_time_limit(8)
        return env

    plain, stacked, only, top = make(), make(), make(), make(render_top_view=True, pu_per_tu=8)
    stacked.set_learner_view("gray", (16, 16), stack=3)
    only.set_learner_view("gray", (16, 16), camera_view=False)
    ts = [Tracked(rcw, e) for e in (plain, stacked, only, top)]
    rng = np.random.default_rng(9)
    for k in range(30):
        a = WR.draw_actions(rng, 16)
        for t in ts:
            t.step(a, f"views: step {k}")
        for t in ts[1:]:
            np.testing.assert_array_equal(t.ref.distance, ts[0].ref.distance)
            np.testing.assert_array_equal(t.ref.progress, ts[0].ref.progress)
            np.testing.assert_array_equal(t.ref.start_distance, ts[0].ref.start_distance)
    assert ts[0].events["restart_after_truncation"] > 0
    assert only.step_form() == "two-launches"
    for e in (plain, stacked, only, top):
        e.close()


# ---- 9  a captured step ---------------------------------------------------------------------------------------------------------------
def test_a_captured_step_replays(rcw):
    torch = pytest.importorskip("torch")
    B = 32
    env = make_env(rcw, B, 7, 7, N=16, Hc=24)
    env.set_walls(GD.pocket())
    env.set_time_limit(3)
    t = Tracked(rcw, env)
    stream = torch.cuda.Stream()
    env.sync()
    env.set_stream(stream.cuda_stream)
    a_host = WR.draw_actions(np.random.default_rng(4), B)
    with torch.cuda.stream(stream):
        actions = torch.from_numpy(a_host).cuda()
        stream.synchronize()
        ptr = env.goal_distance.ptr
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            rcw.act_(env, actions)                                         # (captured, not run)
        for k in range(6):
            ep0 = t.ref.recorded.copy()
            g.replay()
            stream.synchronize()
            t.ref.stepped(*t.state(walls_changed=False))
            t.events["restart_after_truncation"] += int((env.world.episode != ep0).sum())
            t.check(f"replay {k}")
        assert env.goal_distance.ptr == ptr
        stream.synchronize()
    assert t.events["restart_after_truncation"] > 0
    del g
    env.close()


# ---- 10  off and on ---------------------------------------------------------------------------------------------------------------------
def test_off_and_on(rcw, oracle):
    from raycastworlds_jl_amd import _capi

    cfg = dict(height_tile_map_tu=8, width_tile_map_tu=8, num_rays=64)
    env = rcw.SingleRoomModule.SingleRoom(batch=32, seed=3, **cfg)
    orc = oracle.OracleBatch(32, seed=3, **cfg)
    lib, h = env._lib, env._h
    p, n = C.c_void_p(), C.c_int32(-1)
    words = np.zeros(32, np.int32)
    field = np.zeros((32, 64), np.uint16)

    def readers():
        return (lib.rcw_goal_distance(h, words.ctypes.data, None, None), lib.rcw_goal_distance_device_ptr(h, C.byref(p), None, None),
                lib.rcw_goal_distance_field(h, 0, 32, field.ctypes.data), lib.rcw_goal_distance_field_device_ptr(h, C.byref(p)))

    assert readers() == (_capi.RCW_ERR_UNSUPPORTED,) * 4
    assert lib.rcw_goal_distance_enabled(h, C.byref(n)) == 0 and n.value == 0 and not env.goal_distance_enabled
    assert lib.rcw_set_goal_distance(h, 0) == 0
    with pytest.raises(_capi.RcwError):
        env.goal_distance
    rng = np.random.default_rng(0)

    def steps(k):
        for _ in range(k):
            a = rng.integers(1, 5, 32).astype(np.uint8)
            rcw.act_(env, a)
            orc.step(a)

    steps(10)
    t = Tracked(rcw, env)                                                  # enabled mid-episode: start_distance == distance
    np.testing.assert_array_equal(env.goal_start_distance.numpy(), env.goal_distance.numpy())
    assert readers() == (0,) * 4 and p.value == env.goal_distance_field_device().ptr
    assert env.goal_distance_field_device().shape == (32, 8, 8)
    for k in range(10):
        a = rng.integers(1, 5, 32).astype(np.uint8)
        t.step(a, f"on: step {k}")
        orc.step(a)
    assert (env.goal_distance.numpy() >= 0).all()                          # an empty room: every tile reaches the goal
    env.set_goal_distance(True)                                            # again: the same, from the current state
    t.masked(None, "enabled again")
    env.set_goal_distance(False)
    assert readers() == (_capi.RCW_ERR_UNSUPPORTED,) * 4 and not env.goal_distance_enabled
    steps(10)
    np.testing.assert_array_equal(env.camera_view_host(), orc.camera_view)
    np.testing.assert_array_equal(env.world.player_position_wu, orc.position)
    env.close()
    orc.close()


def test_constructor_keyword_and_torch_alias(rcw):
    """SingleRoom(goal_distance=True), and the shaping expression of the README on the device"""
    torch = pytest.importorskip("torch")
    env = make_env(rcw, 8, 7, 7, goal_distance=True)
    assert env.goal_distance_enabled
    t = Tracked(rcw, env, enable=False)
    t.rollout(5, 1, "constructor keyword")
    shaped = torch.as_tensor(env.world.reward, device="cuda") + 0.1 * env.goal_progress.torch(sync=True)
    np.testing.assert_allclose(shaped.cpu().numpy(), env.world.reward + np.float32(0.1) * t.ref.progress.astype(np.float32), rtol=0, atol=1e-7)
    assert env.goal_distance.torch(sync=False).dtype == torch.int32
    env.close()
