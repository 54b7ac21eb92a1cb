"""The goal distance on the GPU (include/rcw.h, rcw_set_goal_distance): after EVERY call the three words and the whole field of every agent
are compared for equality with tests/goal_distance_ref.py, which is fed the state the engine itself reports (walls, goal, position, episode
counter) and which agents an explicit call masked.  State parity with the oracle is the rest of the suite's job.

The kernel has ONE path for every map size (walls and visited bits plus the queue in LDS, the field written to HBM and never read by the
flood): maps up to 180 x 180 launch with the default dynamic-LDS limit, larger ones after the limit is raised — the 200 x 300 case takes
that branch of the launcher, every other case the first.

The pocket rollout rehearsed on the CPU with TimeLimitRef(WallsRef(render=False)) and GoalDistanceRef over the same seed and actions (B = 64,
limit 20, 200 steps, engine seed 5, actions from seed 6): 1656 agent-steps at distance -1, 54 restarts after done, 559 after a truncation,
261 agent-steps with positive progress and 280 with negative.  The engine's own counts must be these.

Levels wider than the wavefront (sections 11 to 14).  A level of the flood is the queue segment [head, level_end), taken 64 tiles at a time;
the layouts above never hold more than 12 tiles at one distance, whichever free tile is the goal (tests/test_goal_distance_spec.py), so they run the chunk
loop once a level, with a dozen live lanes at most and the upper half of the ballot empty.  The cases below flood open and pillared rooms of
132 x 134 tiles (37.6 KiB of LDS: the default launch) and the largest maps rcw_create accepts (the raised limit): every level width from 1
to 130 once, levels of 259 and 503 tiles, ragged ones — behind a masked set_state (the refill launch) and behind the restarts of a short
rollout under a time limit (the step's own stale path).  What each layout's levels hold is asserted of the REFERENCE's field before the
engine is believed, and rehearsed without a GPU in tests/test_goal_distance_spec.py."""
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


Tracked = GD.Tracked                                                       # the one comparer, shared with tools/fuzz_parity.py goal


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


# ---- 11  levels wider than the wavefront ----------------------------------------------------------------------------------------------
WIDE_H, WIDE_W = 132, 134        # the smallest map whose levels pass 128 tiles along either axis; not square: the transposition trap again


def centres(tiles, T=np.float32):
    """the centre of each 1-based tile in world units"""
    return (np.asarray(tiles, np.float64) - 0.5).astype(T)


def free_tiles(walls, which):
    """per agent one free tile, 1-based: number `which(n)` of the layout's n free tiles in row-major order"""
    out = []
    for w in walls:
        free = np.argwhere(~w)
        out.append(free[which(len(free))] + 1)
    return np.array(out, np.int32)


def wide_levels_case(rcw, env, goals, name, precondition, open_room=True):
    """What every wide-level case does, on a handle that has its walls: every goal placed by a full set_state and `precondition` asserted
    of the reference's fields; a masked set_state that hands each masked agent its neighbour's goal, after which the agents outside the mask
    hold every byte they held; twelve steps under a limit of five, so that the step's own stale path floods the re-sampled goals of two
    rounds of restarts.  Returns the Tracked."""
    B = env.batch
    T = env.world.player_position_wu.dtype
    t = Tracked(rcw, env)
    walls = t._walls
    goals = np.asarray(goals, np.int32).reshape(B, 2)
    players = free_tiles(walls, lambda n: n // 7)                           # a free tile of an early row: off the goal
    env.set_state(goals, centres(players, T), np.zeros(B, np.int32))
    t.masked(None, f"{name}: the goals placed")
    np.testing.assert_array_equal(env.world.goal_position, goals)
    precondition([GD.level_sizes(f) for f in t.ref.field], t.ref)
    mask = (np.arange(B) % 2 == 0).astype(np.uint8)
    before = env.goal_distance_field
    swapped = np.roll(goals, 1, axis=0)
    env.set_state(swapped, centres(players, T), np.ones(B, np.int32), mask=mask)
    t.masked(mask, f"{name}: masked set_state")
    after = env.goal_distance_field
    np.testing.assert_array_equal(after[mask == 0], before[mask == 0])
    if len({tuple(g) for g in goals}) == B:
        assert all((after[b] != before[b]).any() for b in np.flatnonzero(mask))
    assert t.widest["refill"] > 128, t.widest
    env.set_time_limit(5)
    t.rollout(12, 7, name)
    assert t.events["restart_after_truncation"] > 0, t.events
    assert t.floods["step"] >= B, t.floods                                  # (every agent is restarted at least once)
    if open_room:                                                          # wherever a restart puts the goal, an open 130 x 132 room has such a level;
        assert t.widest["step"] > 64, t.widest                              # between pillars the goal may fall into a pocket: compared all the same, not asserted
    return t


@pytest.mark.parametrize("form,N,Hc", [("two-launches", 8, 24), ("one-launch", 64, 256)])
def test_every_level_width_once(rcw, form, N, Hc):
    """The ring alone, goals at the four interior corners: from (2, 2) the levels hold exactly 1, 2, ..., 130 tiles and shrink again
    (largest distance 260), so level_end - base passes 63, 64, 65, 127, 128 and 129 — the chunk loop's second and third iteration with
    one live lane, with all, and the ballot's upper half from empty to full."""
    H, W = WIDE_H, WIDE_W
    env = make_env(rcw, 4, H, W, N=N, Hc=Hc, form=form)

    def precondition(sizes, ref):
        for s in sizes:
            assert set(range(1, 131)) <= set(s.tolist()) and len(s) - 1 == 260

    wide_levels_case(rcw, env, [(2, 2), (2, W - 1), (H - 1, 2), (H - 1, W - 1)], f"every width ({form})", precondition)
    assert env.step_form() == form
    env.close()


def test_more_than_four_chunks_a_level(rcw):
    """The goal at the centre of the ring: the widest level holds 259 tiles (five chunks), the largest distance is 131."""
    env = make_env(rcw, 2, WIDE_H, WIDE_W)

    def precondition(sizes, ref):
        for s in sizes:
            assert s.max() > 256 and (int(s.max()), len(s) - 1) == (259, 131)

    wide_levels_case(rcw, env, [(66, 67), (66, 67)], "five chunks", precondition)
    env.close()


@pytest.mark.parametrize("T", ["Float32", "Float64"])
def test_ragged_levels_between_pillars(rcw, T):
    """pillars(132, 134, 0.2, default_rng(seed)) per agent, the goal on the middle free tile: levels of up to 217 tiles with holes at every
    pillar, so that the winners of a ballot are scattered over the lanes, and free tiles without a path in every layout.  (The seeds: the
    first eight whose widest level passes 128 tiles; tests/test_goal_distance_spec.py holds each one's figures.)"""
    B = len(GD.PILLAR_SEEDS)
    walls = np.stack([GD.pillars(WIDE_H, WIDE_W, 0.2, np.random.default_rng(seed)) for seed in GD.PILLAR_SEEDS])
    env = make_env(rcw, B, WIDE_H, WIDE_W, T=T)
    env.set_walls(walls)
    assert env.world.player_position_wu.dtype == (np.float64 if T == "Float64" else np.float32)

    def precondition(sizes, ref):
        assert all(s.max() > 128 for s in sizes), [int(s.max()) for s in sizes]
        assert any(((ref.field[b] == GD.UNREACHED) & ~walls[b]).any() for b in range(B))

    t = wide_levels_case(rcw, env, [GD.middle_free_tile(w) for w in walls], f"pillars ({T})", precondition, open_room=False)
    np.testing.assert_array_equal(t._walls, walls)
    env.close()


# ---- 12  the largest maps the library accepts ------------------------------------------------------------------------------------------
# rcw_create takes H W + 2 H <= 65280 (the cast kernel stages a byte a tile and two guard bands of H bytes in 64 KiB of LDS), so a map of
# 255 x 256 = 65,280 tiles is refused: the squarest map it takes is 254 x 255, the squarest whose last interior tile has a linear index
# above 65,000 is 86 x 757, and the largest index of any is 65,269 in a corridor of 3 x 21,758.  All three need the raised LDS limit.
LARGEST = [(254, 255, 503, 0), (86, 757, 168, 65000), (3, 21758, 2, 65250)]


@pytest.mark.parametrize("H,W,widest,index", LARGEST, ids=[f"{c[0]}x{c[1]}" for c in LARGEST])
def test_largest_maps_open_room(rcw, H, W, widest, index):
    """The ring alone on the largest maps, one goal at the centre and one on the last interior tile — its index and its neighbours' are the
    largest UInt16 queue entries there are, next to the 0xFFFF sentinel.  Then a reset and five steps."""
    assert H * W + 2 * H <= 65280 < H * (W + 1) + 2 * H                     # (one more column is refused)
    env = make_env(rcw, 2, H, W, N=8, Hc=24)
    t = Tracked(rcw, env)
    goals = np.array([((H + 1) // 2, (W + 1) // 2), (H - 1, W - 1)], np.int32)
    env.set_state(goals, centres([(2, 2), (2, 2)]), np.zeros(2, np.int32))
    t.masked(None, f"{H} x {W}: the goals placed")
    sizes = [GD.level_sizes(f) for f in t.ref.field]
    assert int(sizes[0].max()) == widest and t.widest["refill"] >= widest
    assert (int(sizes[1].max()), len(sizes[1]) - 1) == (min(H, W) - 2, H + W - 6)      # the corner: 1, 2, ... up to the short side, H + W - 6 steps
    top = int(np.flatnonzero(GD.linear(t.ref.field[1]) != GD.UNREACHED).max())
    assert top == H * W - H - 2 and top > index, top
    assert (env.goal_distance.numpy() == [(H + 1) // 2 - 2 + (W + 1) // 2 - 2, H + W - 6]).all()
    rcw.reset_(env)
    t.masked(None, f"{H} x {W}: reset")
    t.rollout(5, 1, f"{H} x {W}")
    env.close()


def test_a_map_of_65280_tiles_is_refused(rcw):
    from raycastworlds_jl_amd import _capi

    with pytest.raises(_capi.RcwError):
        make_env(rcw, 1, 255, 256)


# ---- 13  the field export's sub-range ---------------------------------------------------------------------------------------------------
def test_field_export_sub_ranges(rcw):
    """rcw_goal_distance_field(h, first, count, out) with a maze per agent, so that every row differs: each sub-range holds the reference's
    rows first .. first + count - 1 and nothing is written in front of or behind them.  check_range (csrc/rcw_api.hip) takes
    first >= 0, count >= 0 and first + count <= B: a count of zero is an empty copy, not an error."""
    from raycastworlds_jl_amd import _capi, layouts

    B, size = 9, 9
    rng = np.random.default_rng(13)
    env = make_env(rcw, B, size, size)
    env.set_walls(np.stack([layouts.maze(size, size, rng) for _ in range(B)]))
    t = Tracked(rcw, env)
    t.rollout(3, 2, "sub-ranges")
    want = np.stack([GD.linear(f) for f in t.ref.field])
    assert len({w.tobytes() for w in want}) == B
    lib, h, HW, canary = env._lib, env._h, size * size, 0xA5C3

    def read(first, count):
        buf = np.full((max(count, 0) + 2, HW), canary, np.uint16)         # a canary row in front of the output and one behind it
        rc = lib.rcw_goal_distance_field(h, first, count, buf[1:].ctypes.data)
        return rc, buf

    for first, count in ((3, 5), (B - 1, 1), (0, 1), (0, B), (4, 0)):
        rc, buf = read(first, count)
        assert rc == 0, (first, count, _capi.last_error(lib))
        np.testing.assert_array_equal(buf[1:1 + count], want[first:first + count], err_msg=f"rows [{first}, {first + count})")
        assert (buf[0] == canary).all() and (buf[-1] == canary).all(), (first, count)
    for first, count in ((-1, 2), (0, -1), (3, -2), (B - 1, 2), (B, 1), (0, B + 1)):
        rc, buf = read(first, count)
        assert rc == _capi.RCW_ERR_INVALID_ARGUMENT, (first, count, rc)
        assert "bad agent range" in _capi.last_error(lib)
        assert (buf == canary).all(), (first, count)
    assert lib.rcw_goal_distance_field(h, 0, 1, None) == _capi.RCW_ERR_INVALID_ARGUMENT
    t.check("behind the refusals")                                          # nothing was queued by them
    t.rollout(2, 3, "behind the refusals")
    env.close()


# ---- 14  a raising move with the feature on ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["two-launches", "one-launch"])
def test_a_raising_move_with_the_feature_on(rcw, form):
    """out_of_bounds = 0 in the 4 x 4 room of tests/test_gpu_time_limit.py (a quarter-tile move next to the ring tests a neighbourhood that
    leaves the map: 19 of its 24 steps raise there): the step leaves an IndexError for the next sync.  The kernel behind that step ran all
    the same: after each raise, cleared the way those tests clear it, the words and fields equal the reference fed from the state the engine
    reports — an agent the raise left where it was has progress 0 — and the steps behind it go on."""
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
    assert t.events["restart_after_truncation"] > 0, t.events
    assert not env.world.status.any()
    env.sync()
    env.close()
