"""The local map on the GPU (include/rcw.h, rcw_set_local_map): after EVERY call every byte of every agent's image is compared for equality
with tests/local_map_ref.py, which is fed the state the engine itself reports — position, heading, the direction table the handle holds,
the tile map or the seen map.  State parity with the oracle and the seen map itself are the rest of the suite's job.

The kernel has one path a source and a type (four instantiations); what varies is the store: a lane owns an aligned 32-bit word of the
batch's byte array, and with S*S not a multiple of four an agent's image begins and ends inside a word — S in {1, 3, 5, 31} makes every
lead 0..3 occur within four agents, S in {2, 8, 64, 128} none.  S = 128 is the one size at which a lane loops (4096 words on 256 lanes).
(That exactly four instantiations ship is asserted in tests/test_local_map_spec.py: it needs the compiler, not a GPU.)"""
import ctypes as C

import numpy as np
import pytest

import local_map_ref as LM
import walls_ref as WR

pytestmark = pytest.mark.gpu

FAST = dict(num_directions=16, position_increment_wu=0.25, player_radius_wu=0.3)
Tracked = LM.Tracked
OFF = {"source": None, "size": 0, "cells_per_tile": 0}


def make_env(rcw, B, H, W, N=33, Hc=24, seed=5, form=None, **kw):
    env = rcw.SingleRoomModule.SingleRoom(batch=B, seed=seed, auto_reset=kw.pop("auto_reset", True), height_tile_map_tu=H, width_tile_map_tu=W,
                                          num_rays=N, height_camera_view_pu=Hc, **{**FAST, **kw})
    if form is not None:
        env.set_step_form(form)
        assert env.step_form() == form
    return env


def ring(H, W):
    w = np.zeros((H, W), bool)
    w[[0, -1], :] = True
    w[:, [0, -1]] = True
    return w


def mazes(n, size=9, seed=9):
    from raycastworlds_jl_amd import layouts

    rng = np.random.default_rng(seed)
    return np.stack([layouts.maze(size, size, rng) for _ in range(n)])


# ---- 1  the shapes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 3, 5, 8, 31, 64, 128])
def test_sizes(rcw, S):
    """every size on a 7 x 9 room (H != W), r = 1 and one other r; 13 agents, so that with S*S = 1 mod 4 every lead occurs three times"""
    env = make_env(rcw, 13, 7, 9)
    t = Tracked(rcw, env, S, 1)
    t.rollout(4, S, f"S {S}")
    assert t.inside > 0 and (S < 3 or t.outside > 0)
    r = {1: 2, 2: 3, 3: 16, 5: 3, 8: 2, 31: 3, 64: 16, 128: 16}[S]
    env.set_local_map(S, r)
    t2 = Tracked(rcw, env, S, r, enable=False)
    t2.rollout(3, S + 1, f"S {S}, r {r}")
    env.close()


@pytest.mark.parametrize("name,H,W", [("4x4", 4, 4), ("7x9", 7, 9), ("5x13", 5, 13), ("13x5", 13, 5)])
@pytest.mark.parametrize("r", [1, 2, 3, 16])
def test_maps_and_cells_per_tile(rcw, name, H, W, r):
    env = make_env(rcw, 16, H, W)
    env.set_time_limit(6)
    t = Tracked(rcw, env, 5 * r + 1, r)                                     # five tiles and a cell across
    t.rollout(10, r, f"{name}, r {r}")
    assert t.inside > 0 and t.outside > 0
    env.close()


def test_a_maze_per_agent(rcw):
    """32 x 32 mazes, one per agent (the images differ from agent to agent), 64 agents, restarts under a time limit"""
    env = make_env(rcw, 64, 32, 32)
    env.set_walls(mazes(64, 32))
    env.set_time_limit(5)
    t = Tracked(rcw, env, 31, 2)
    t.rollout(12, 2, "mazes")
    got = env.local_map_host()
    assert len({g.tobytes() for g in got}) > 32 and (got == 2).any() and (got == 1).any()
    env.close()


def test_the_largest_map(rcw):
    """254 x 254: the largest square map rcw_create accepts — 4033 tile words in LDS —, S = 128, r = 1, one player next to the last
    interior tile (the largest tile indices there are); then the same size over the seen map"""
    H = W = 254
    env = make_env(rcw, 2, H, W, N=64)
    t = Tracked(rcw, env, 128, 1)
    goal = np.array([(2, 2), (H - 1, W - 1)], np.int32)
    pos = np.array([(H - 1.5, W - 2.5), (1.5, 1.5)], np.float32)
    env.set_state(goal, pos, np.array([4, 2], np.int32))
    got = t.check("254 x 254: set_state")
    assert (got[0] == 0).any() and (got[0] == 2).any() and (got[0] == 1).any()    # (outside, the ring, the room)
    t.rollout(3, 1, "254 x 254")
    env.set_seen_map(True)
    env.set_local_map(128, 1, "seen")
    t3 = Tracked(rcw, env, 128, 1, LM.SEEN, enable=False)
    t3.rollout(2, 2, "254 x 254, seen")
    env.close()


# ---- 2  headings ----------------------------------------------------------------------------------------------------------------------
def test_every_heading_of_eight(rcw):
    B, nd = 16, 8
    env = make_env(rcw, B, 7, 9, num_directions=nd)
    t = Tracked(rcw, env, 7, 2)
    goal, pos = env.world.goal_position.copy(), env.world.player_position_wu.copy()
    seen = set()
    for k in range(4):
        head = ((np.arange(B) + k) % nd).astype(np.int32)
        env.set_state(goal, pos, head)
        t.check(f"headings, round {k}")
        seen |= set(head.tolist())
    assert seen == set(range(nd))
    # the same place, turned: eight different pictures on a map without symmetry
    walls = ring(7, 9)
    walls[1, 2] = walls[4, 6] = walls[5, 1] = walls[2, 5] = True
    env.set_walls(walls)
    goal[:] = (4, 4)
    pos[:] = (2.5, 3.25)
    env.set_state(goal, pos, (np.arange(B) % nd).astype(np.int32))
    got = t.check("one place, eight headings")
    assert len({g.tobytes() for g in got[:nd]}) == nd
    env.close()


def test_128_directions_on_a_random_rollout(rcw):
    env = make_env(rcw, 32, 9, 9, num_directions=128)
    env.set_walls(mazes(32))
    t = Tracked(rcw, env, 9, 3)
    t.rollout(24, 7, "128 directions")
    assert len(set(env.world.player_direction_au.tolist())) > 8
    env.close()


def test_a_custom_direction_table(rcw):
    """non-unit, non-axis vectors: the image follows AT the call (a re-render), and the steps behind it"""
    B, nd = 16, 16
    env = make_env(rcw, B, 9, 9)
    t = Tracked(rcw, env, 9, 2)
    before = env.local_map_host()
    rng = np.random.default_rng(5)
    table = (rng.random((nd, 2)) * 3 - 1.5).astype(np.float32)
    table[np.abs(table) < 0.2] = 0.7
    env.set_direction_table(table)
    np.testing.assert_array_equal(env.world.directions_wu, table)
    got = t.check("behind set_direction_table")
    assert (got != before).any()
    t.rollout(6, 3, "behind set_direction_table")
    env.close()


# ---- 3  types ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", [LM.WORLD, LM.SEEN])
def test_float64_handles(rcw, source):
    env = make_env(rcw, 16, 7, 9, T="Float64", seen_map=source == LM.SEEN)
    assert env.world.player_position_wu.dtype == np.float64 and env.world.directions_wu.dtype == np.float64
    env.set_time_limit(6)
    t = Tracked(rcw, env, 11, 3, source)
    t.rollout(12, 4, f"Float64, {source}")
    theta = 2 * np.pi * np.arange(16) / 16 + 0.3
    env.set_direction_table(np.stack([1.25 * np.cos(theta), 0.75 * np.sin(theta)], axis=1))
    t.check("Float64: behind set_direction_table")
    t.rollout(4, 5, "Float64: behind set_direction_table")
    env.close()


# ---- 4  the seen map as the source --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,N,Hc", [("two-launches", 33, 24), ("one-launch", 64, 256)])
def test_seen_rollouts_in_both_step_forms(rcw, form, N, Hc):
    """auto_reset and a time limit of a few steps: agents restart, their seen maps are cleared, and the image shows the cleared map in the
    same call (the local map's launch is behind the seen map's)"""
    B = 32
    env = make_env(rcw, B, 9, 9, N=N, Hc=Hc, form=form, seen_map=True)
    env.set_walls(mazes(B))
    env.set_time_limit(4)
    t = Tracked(rcw, env, 13, 2, LM.SEEN)
    episodes = env.world.episode.copy()
    t.rollout(14, 6, f"seen ({form})")
    assert env.step_form() == form and (env.world.episode > episodes).any()
    assert t.inside > 0 and t.outside > 0
    env.close()


def test_seen_masked_calls_and_enabling_again(rcw):
    B, H, W = 12, 9, 9
    env = make_env(rcw, B, H, W, seen_map=True)
    env.set_walls(mazes(B))
    t = Tracked(rcw, env, 9, 1, LM.SEEN)
    t.rollout(6, 2, "before the masked calls")
    mask = (np.arange(B) % 3 == 0).astype(np.uint8)
    before = env.local_map_host()
    rcw.reset_(env, mask)
    got = t.check("masked reset_")
    np.testing.assert_array_equal(got[mask == 0], before[mask == 0])       # the same bytes again
    t.rollout(3, 3, "between")
    goal, pos, head = env.world.goal_position.copy(), env.world.player_position_wu.copy(), env.world.player_direction_au.copy()
    mask2 = (np.arange(B) % 4 == 1).astype(np.uint8)
    pos[mask2 != 0] = (2.5, 3.5)
    head[mask2 != 0] = 3
    before = env.local_map_host()
    env.set_state(goal, pos, head, mask=mask2)
    got = t.check("masked set_state")
    np.testing.assert_array_equal(got[mask2 == 0], before[mask2 == 0])
    t.rollout(3, 4, "between")
    mask3 = (np.arange(B) % 2 == 0).astype(np.uint8)
    before = env.local_map_host()
    env.set_walls(ring(H, W), mask=mask3)
    got = t.check("masked set_walls")
    np.testing.assert_array_equal(got[mask3 == 0], before[mask3 == 0])
    t.rollout(4, 5, "behind the masked calls")
    count = env.seen_count.numpy().copy()
    env.set_seen_map(True)                                                  # again: the seen maps afresh (in a new buffer), the images with them
    t.check("set_seen_map(True) again")
    assert (env.seen_count.numpy() < count).any()
    t.rollout(3, 6, "behind set_seen_map(True)")
    env.close()


def test_world_masked_calls(rcw):
    B, H, W = 12, 9, 9
    env = make_env(rcw, B, H, W)
    t = Tracked(rcw, env, 10, 2)
    mask = (np.arange(B) % 3 == 0).astype(np.uint8)
    env.set_walls(mazes(B), mask=mask)
    t.check("masked set_walls")
    rcw.reset_(env, mask)
    t.check("masked reset_")
    rcw.reset_(env)
    t.check("reset_")
    t.rollout(5, 1, "behind")
    env.close()


# ---- 5  refusals and switching ----------------------------------------------------------------------------------------------------------
def test_refusals_and_switching(rcw):
    from raycastworlds_jl_amd import _capi

    env = make_env(rcw, 8, 7, 9)
    lib, h = env._lib, env._h
    assert lib.rcw_set_local_map(h, 0, 0, 0) == 0                           # off where there was none
    with pytest.raises(_capi.RcwError):                                     # SEEN without a seen map
        env.set_local_map(8, 1, "seen")
    assert lib.rcw_set_local_map(h, _capi.RCW_LOCAL_SEEN, 8, 1) == _capi.RCW_ERR_UNSUPPORTED
    assert env.local_map_info == OFF
    t = Tracked(rcw, env, 8, 2)
    ptr = env.local_map.ptr
    for source, size, r in ((1, 0, 1), (1, 129, 1), (1, -1, 1), (1, 8, 0), (1, 8, 17), (3, 8, 1), (-1, 8, 1), (2, 0, 0)):
        assert lib.rcw_set_local_map(h, source, size, r) == _capi.RCW_ERR_INVALID_ARGUMENT, (source, size, r)
        assert env.local_map_info == {"source": "world", "size": 8, "cells_per_tile": 2}
        p = C.c_void_p()
        assert lib.rcw_local_map_device_ptr(h, C.byref(p)) == 0 and p.value == ptr
    with pytest.raises(ValueError):
        env.set_local_map(8, 1, "top")
    t.check("behind the refusals")
    env.set_seen_map(True)
    env.set_seen_map(False)                                                 # the source is the world: the seen map comes and goes freely
    t.check("the seen map on and off beside a world source")
    env.set_seen_map(True)
    env.set_local_map(12, 3, "seen")                                        # on with other parameters
    t = Tracked(rcw, env, 12, 3, LM.SEEN, enable=False)
    t.rollout(3, 1, "seen")
    with pytest.raises(_capi.RcwError, match="switch the local map off first"):
        env.set_seen_map(False)
    assert lib.rcw_set_seen_map(h, 0) == _capi.RCW_ERR_UNSUPPORTED and env.seen_map_enabled
    t.check("behind the refused set_seen_map(False)")
    t.rollout(2, 2, "behind the refusal")
    env.set_local_map(0)
    assert env.local_map_info == OFF
    env.set_seen_map(False)
    assert not env.seen_map_enabled
    env.set_local_map(None)
    t = Tracked(rcw, env, 5, 1)                                             # and on again
    t.rollout(3, 3, "on again")
    env.close()


def test_a_handle_without_the_feature(rcw, oracle):
    from raycastworlds_jl_amd import _capi

    cfg = dict(height_tile_map_tu=8, width_tile_map_tu=8, num_rays=64)
    env = rcw.SingleRoomModule.SingleRoom(batch=32, seed=3, **cfg)
    orc = oracle.OracleBatch(32, seed=3, **cfg)
    lib, h = env._lib, env._h
    v = [C.c_int32(-1) for _ in range(3)]
    assert lib.rcw_local_map_info(h, *[C.byref(x) for x in v]) == 0 and [x.value for x in v] == [0, 0, 0]
    assert lib.rcw_local_map_info(h, None, None, None) == 0 and env.local_map_info == OFF
    p, buf = C.c_void_p(), np.zeros((32, 16), np.uint8)
    assert lib.rcw_local_map_device_ptr(h, C.byref(p)) == _capi.RCW_ERR_UNSUPPORTED
    assert lib.rcw_local_map_copy(h, buf.ctypes.data, 0, 32) == _capi.RCW_ERR_UNSUPPORTED
    with pytest.raises(_capi.RcwError):
        env.local_map
    rng = np.random.default_rng(0)
    for _ in range(10):
        a = rng.integers(1, 5, 32).astype(np.uint8)
        rcw.act_(env, a)
        orc.step(a)
    np.testing.assert_array_equal(env.camera_view_host(), orc.camera_view)   # a handle without it equals the oracle as before
    env.close()
    orc.close()


def test_calls_that_do_nothing(rcw):
    env = make_env(rcw, 16, 9, 9, N=64, Hc=64)
    t = Tracked(rcw, env, 9, 2)
    t.rollout(3, 1, "before")
    rcw.cast_rays_(env)
    t.check("behind cast_rays")
    rcw.update_camera_view_(env)
    t.check("behind update_camera_view")
    env.set_step_form("one-launch")
    t.check("behind set_step_form")
    env.set_time_limit(7)
    t.check("behind set_time_limit")
    env.set_learner_view("gray", (16, 16))
    t.check("behind set_learner_view")
    env.set_goal_distance(True)
    t.check("behind set_goal_distance")
    t.rollout(5, 2, "behind")
    env.close()


# ---- 6  cells far off the map, Inf and NaN ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", ["Float32", "Float64"])
def test_cells_far_off_the_map_inf_and_nan(rcw, T):
    """Inputs the contract defines: 'for any position, including NaN, +-Inf and positions far off the map' the cell is 0 and nothing outside
    the agent's tiles is read.  rcw_set_state refuses a position outside the room under either out_of_bounds mode (asserted below, with the
    images unchanged), so the world coordinates are driven there through the other input the contract names, the direction table — 'whatever
    rcw_set_direction_table last put there': finite entries of 1e6 (cells a million tiles off), of (3, 0.5) (a partial image), and of
    the type's largest magnitudes, whose products with the offsets overflow to +-Inf and whose sums are Inf - Inf = NaN."""
    B = 16
    env = make_env(rcw, B, 7, 9, T=T, out_of_bounds=1)
    big = 2e38 if T == "Float32" else 1e308
    t = Tracked(rcw, env, 9, 1)
    goal, pos, head = env.world.goal_position.copy(), env.world.player_position_wu.copy(), env.world.player_direction_au.copy()
    before = env.local_map_host()
    for bad in ((-3.5, 2.5), (2.5, 40.0), (np.nan, 2.5), (2.5, np.inf)):
        p = pos.copy()
        p[0] = bad
        with pytest.raises(ValueError, match="not inside the room"):
            env.set_state(goal, p, head)
        np.testing.assert_array_equal(env.local_map_host(), before)
    table = env.world.directions_wu.copy()
    table[0] = (1e6, 0)
    table[1] = (0, -1e6)
    table[2] = (3, 0.5)
    table[3] = (big, big)
    table[4] = (-big, big)
    table[5] = (big, 0)
    env.set_direction_table(table)
    env.set_state(goal, pos, (np.arange(B) % 8).astype(np.int32))
    got = t.check("huge direction vectors")
    c = 4
    for a in range(6):
        assert got[a, c, c] != 0                                            # the centre cell: offsets 0, the agent's own tile
    for a in (0, 1, 3, 4, 5):
        assert (got[a] != 0).sum() == 1, a                                  # every other cell is at least 10^6 tiles off, Inf or NaN
    assert (got[2] != 0).sum() > 1 and (got[2] == 0).any()                  # cells three tiles apart: some on the 7 x 9 map, most off it
    with np.errstate(all="ignore"):
        Tn = env.T
        off = LM.offsets(9, 1, Tn)
        assert np.isinf(off[8] * Tn(big)) and np.isnan(off[8] * Tn(big) + off[0] * Tn(big))     # (the arithmetic does produce them)
    env.set_state(goal, pos, ((np.arange(B) + 3) % 8).astype(np.int32))   # the vectors on other agents, other positions
    t.check("huge direction vectors, turned")
    env.close()


# ---- 7  the exports -----------------------------------------------------------------------------------------------------------------------
def test_copy_sub_ranges(rcw):
    from raycastworlds_jl_amd import _capi

    B, S = 9, 5                                                             # 25 bytes an agent: every sub-range starts at another lead
    env = make_env(rcw, B, 9, 9)
    env.set_walls(mazes(B, seed=13))
    t = Tracked(rcw, env, S, 1)
    t.rollout(3, 2, "sub-ranges")
    want = t.want().reshape(B, S * S)
    assert len({w.tobytes() for w in want}) > B // 2
    lib, h, canary = env._lib, env._h, 0xA5

    def read(first, count):
        buf = np.full((max(count, 0) + 2, S * S), canary, np.uint8)
        rc = lib.rcw_local_map_copy(h, buf[1:].ctypes.data, first, count)
        return rc, buf

    for first, count in ((3, 5), (B - 1, 1), (0, 1), (0, B), (4, 0)):
        rc, buf = read(first, count)
        assert rc == 0, (first, count, _capi.last_error(lib))
        np.testing.assert_array_equal(buf[1:1 + count], want[first:first + count], err_msg=f"agents [{first}, {first + count})")
        assert (buf[0] == canary).all() and (buf[-1] == canary).all(), (first, count)
    for first, count in ((-1, 2), (0, -1), (B - 1, 2), (B, 1), (0, B + 1)):
        rc, buf = read(first, count)
        assert rc == _capi.RCW_ERR_INVALID_ARGUMENT and (buf == canary).all(), (first, count, rc)
    assert lib.rcw_local_map_copy(h, None, 0, 1) == _capi.RCW_ERR_INVALID_ARGUMENT
    np.testing.assert_array_equal(env.local_map_host(2, 3), want[2:5].reshape(3, S, S))
    env.close()


def test_constructor_keyword_and_torch_alias(rcw):
    torch = pytest.importorskip("torch")
    env = make_env(rcw, 8, 7, 9, local_map=7)
    assert env.local_map_info == {"source": "world", "size": 7, "cells_per_tile": 1}
    env.close()
    env = make_env(rcw, 8, 7, 9, seen_map=True, local_map=dict(size=10, cells_per_tile=2, source="seen"))
    t = Tracked(rcw, env, 10, 2, LM.SEEN, enable=False)
    dev = env.local_map
    assert dev.shape == (8, 10, 10) and dev.dtype == np.uint8 and env.local_map is dev
    alias = dev.torch(sync=False)
    assert alias.dtype == torch.uint8 and tuple(alias.shape) == (8, 10, 10) and alias.data_ptr() == dev.ptr
    for k in range(4):
        want = t.step(WR.draw_actions(np.random.default_rng(k), 8), f"alias: step {k}")
        np.testing.assert_array_equal(alias.cpu().numpy(), want)           # the same tensor, rewritten in place
        np.testing.assert_array_equal(np.asarray(dev), want)
    env.set_local_map(6)
    assert env.local_map is not dev and env.local_map.shape == (8, 6, 6)
    env.close()


def test_a_captured_step_replays(rcw):
    torch = pytest.importorskip("torch")
    B = 32
    env = make_env(rcw, B, 9, 9, seen_map=True)
    env.set_walls(mazes(B))
    env.set_time_limit(3)
    t = Tracked(rcw, env, 11, 2, LM.SEEN)
    stream = torch.cuda.Stream()
    env.sync()
    env.set_stream(stream.cuda_stream)
    a_host = WR.draw_actions(np.random.default_rng(4), B)
    with torch.cuda.stream(stream):
        actions = torch.from_numpy(a_host).cuda()
        stream.synchronize()
        ptr = env.local_map.ptr
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            rcw.act_(env, actions)                                         # (captured, not run)
        images = set()
        for k in range(6):
            g.replay()
            stream.synchronize()
            images.add(t.check(f"replay {k}").tobytes())
        assert env.local_map.ptr == ptr and len(images) > 1
        stream.synchronize()
    del g
    env.close()


def test_two_shards_equal_their_slices_of_the_whole_batch(rcw):
    G, WORLD = 16, 2
    kw = dict(seed=5, auto_reset=True, height_tile_map_tu=9, width_tile_map_tu=9, num_rays=33, height_camera_view_pu=24, **FAST)
    whole = rcw.SingleRoomModule.SingleRoom(batch=G, **kw)
    shards = [rcw.ShardedSingleRoom(G, rank=r, world=WORLD, device=0, **kw) for r in range(WORLD)]
    walls = mazes(G, seed=21)
    whole.set_walls(walls)
    whole.set_time_limit(6)
    t = Tracked(rcw, whole, 7, 1)                                           # 49 bytes an agent
    for sh in shards:
        sh.set_walls(walls)
        sh.env.set_time_limit(6)
        sh.env.set_local_map(7, 1)

    def compare(where):
        want = whole.local_map_host()
        for sh in shards:
            np.testing.assert_array_equal(sh.env.local_map_host(), want[sh.first:sh.first + sh.count], err_msg=where)

    compare("switched on")
    rng = np.random.default_rng(3)
    for k in range(12):
        a = WR.draw_actions(rng, G)
        t.step(a, f"whole batch: step {k}")
        for sh in shards:
            sh.act_(sh.local_slice(a))
        compare(f"step {k}")
    for sh in shards:
        sh.close()
    whole.close()
