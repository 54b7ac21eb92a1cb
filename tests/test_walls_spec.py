"""Interior walls on the CPU (include/rcw.h, rcw_set_walls): the export in the header, the bindings and the library; the generator of
tests/walls_ref.py against the unchanged C oracle on ring-only maps, alone and under the time limit's composition; the development build's device-less validation; the host-rng
draws with and without walls; the layout generators."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import time_limit_ref as TL
import walls_ref as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_header_the_bindings_and_the_library_carry_rcw_set_walls(rcw):
    from raycastworlds_jl_amd import _capi

    text = open(os.path.join(ROOT, "include", "rcw.h")).read()
    assert re.search(r"RCW_API\s+int\s+rcw_set_walls\s*\(\s*rcw_handle\*\s*h\s*,\s*const\s+uint8_t\*\s*walls_host\s*,\s*int32_t\s+layouts\s*,"
                     r"\s*const\s+int32_t\*\s*layout_index_host\s*,\s*const\s+uint8_t\*\s*mask_host\s*\)\s*;", text)
    assert re.search(r"#define\s+RCW_ABI_VERSION\s+4\b", text) and _capi.RCW_ABI_VERSION == 4      # additive: the version stays
    assert _capi.SIGNATURES["rcw_set_walls"] == [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    jl = open(os.path.join(ROOT, "julia", "BatchedSingleRoom.jl")).read()
    assert re.search(r"ccall\(\(:rcw_set_walls,\s*librcw\)", jl) and "function set_walls!" in jl
    lib = _capi.load()
    assert hasattr(lib, "rcw_set_walls") and lib.rcw_abi_version() == 4
    assert lib.rcw_set_walls(None, None, 1, None, None) == _capi.RCW_ERR_INVALID_ARGUMENT and _capi.last_error(lib)
    SR = rcw.SingleRoomModule
    assert callable(SR.SingleRoom.set_walls) and isinstance(SR.SingleRoomWorld.walls, property) and callable(rcw.ShardedSingleRoom.set_walls)
    assert all(callable(getattr(rcw.layouts, n)) for n in ("ring", "four_rooms", "maze", "is_connected"))


@pytest.mark.parametrize("H,W", [(8, 8), (5, 7), (32, 32), (3, 3)])
def test_the_restated_generator_is_the_oracles_on_a_ring_only_map(rcw, oracle, H, W):
    """64 agents, three consecutive resets.  3 x 3: the one interior tile is the goal, the sampler gives up after 1024 H W tries"""
    ring = rcw.layouts.ring(H, W)
    orc = oracle.OracleBatch(64, seed=11, render=False, height_tile_map_tu=H, width_tile_map_tu=W, num_rays=8, height_camera_view_pu=8, num_directions=8)
    counts = {}
    for episode in range(3):                                                 # (the key is the counter BEFORE the increment)
        if episode:
            orc.reset(seed=11)
        assert (orc.episode == episode + 1).all()
        for a in range(64):
            gi, gj, ti, tj, d, gave_up = WR.reset_draws(11, a, episode, H, W, 8, ring, counts)
            assert (gi, gj) == tuple(orc.goal[a]) and (ti - 0.5, tj - 0.5) == tuple(orc.position[a]) and d == orc.direction[a], (episode, a)
            assert gave_up == (orc.status[a] == WR.RCW_WARN_SAMPLER_GAVE_UP) == ((H, W) == (3, 3))
    assert counts["goal_redraws"] == 0                                       # no interior tile of a ring is a wall: the draw indices did not move
    orc.close()


def test_the_time_limit_over_the_reference_worlds_is_the_time_limit_over_the_oracle_on_a_ring_only_map(oracle):
    """TimeLimitRef(WallsRef) — what tests/test_gpu_walls_time_limit.py compares the engine with — beside TimeLimitRef(OracleBatch), the
    composition tests/test_gpu_time_limit.py uses, on a 6 x 6 map without interior walls: 16 agents, a limit of 5, 30 steps.  Position bits,
    heading, goal, done, reward, episode counter and the limit's two words after every step; the restarts after a truncation go through
    WallsRef.reset(mask, seed) and the generator restated in Python, those after `done` through step_lenient."""
    B, L, seed = 16, 5, 7
    walled = WR.WallsRef(B, seed, 6, 6, 8, 8, nd=8, inc=0.25, radius=0.3, render=False)
    orc = oracle.OracleBatch(B, seed=seed, render=False, height_tile_map_tu=6, width_tile_map_tu=6, num_rays=8, height_camera_view_pu=8, num_directions=8,
                             auto_reset=1, position_increment_wu=0.25, player_radius_wu=0.3)
    a, b = TL.TimeLimitRef(walled, L, seed, True), TL.TimeLimitRef(orc, L, seed, True)
    rng = np.random.default_rng(seed + 1)
    for t in range(30):
        actions = TL.draw_actions(rng, B, t)
        a.step(actions); b.step(actions)
        np.testing.assert_array_equal(walled.position.view(np.uint32), orc.position.view(np.uint32), err_msg=f"position, step {t}")
        np.testing.assert_array_equal(walled.direction, orc.direction, err_msg=f"heading, step {t}")
        np.testing.assert_array_equal(walled.goal, orc.goal, err_msg=f"goal, step {t}")
        np.testing.assert_array_equal(walled.done, orc.done, err_msg=f"done, step {t}")
        np.testing.assert_array_equal(walled.reward, orc.reward, err_msg=f"reward, step {t}")
        np.testing.assert_array_equal(walled.episode, orc.episode, err_msg=f"episode, step {t}")
        np.testing.assert_array_equal(a.episode_steps, b.episode_steps, err_msg=f"episode_steps, step {t}")
        np.testing.assert_array_equal(a.truncated, b.truncated, err_msg=f"truncated, step {t}")
    assert a.events == b.events and all(a.events[k] > 0 for k in ("truncations", "terminations", "restarts_after_truncation", "restarts_after_done")), a.events
    assert walled.events["restarts_after_done"] == a.events["restarts_after_done"] and walled.events["goal_redraws"] == 0
    assert not walled.status.any() and not orc.status.any()
    orc.close()


@pytest.mark.parametrize("name", ["ROOMS", "WIDE", "MAZE", "F64"])
def test_the_limited_rollouts_on_walled_maps_reach_what_they_claim(rcw, name):
    """the rehearsal of tests/test_gpu_walls_time_limit.py without the frames: the dynamics alone give the counts its docstring quotes"""
    import test_gpu_walls_time_limit as G

    events = G.rollout(name, render=False)[2]
    assert tuple(events[k] for k in G.COLUMNS) == G.REHEARSED[name], events
    assert events["goal_redraws_on_truncation_restarts"] > 0 and events["restarts_after_truncation"] == events["truncations"] > 0
    assert (events["restarts_after_done"] > 0) == (name != "MAZE")


def test_the_numpy_blocks_of_the_generator_are_its_python_integers(rcw):
    rng = np.random.default_rng(0)
    redrawn = 0
    for k in range(24):
        H, W = int(rng.integers(3, 7)), int(rng.integers(3, 7))
        walls = rcw.layouts.ring(H, W)
        walls[1:-1, 1:-1] |= rng.random((H - 2, W - 2)) < 0.6
        counts = {}
        assert WR.reset_draws(5, k, k % 3, H, W, 8, walls, counts) == WR.reset_draws_scalar(5, k, k % 3, H, W, 8, walls)
        redrawn += counts["goal_redraws"]
    assert redrawn > 0
    assert WR._draws_below(123, 4, 3, 49).tolist() == [WR.below(WR.draw(123, n), 49) for n in (4, 5, 6)]


@pytest.fixture(scope="module")
def validate(rcw):
    from raycastworlds_jl_amd import _capi

    if not os.path.exists(_capi.DEV_LIB_PATH):
        from raycastworlds_jl_amd import build as _build

        _build.build()
    lib = C.CDLL(_capi.DEV_LIB_PATH)
    lib.rcw_dev_validate_walls.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int32]
    lib.rcw_dev_validate_walls.restype = C.c_int

    def call(H, W, B, walls, index=None, mask=None):
        """walls: bool (M, H, W) or None -> (return code, message)"""
        msg = C.create_string_buffer(256)
        flat = None if walls is None else np.ascontiguousarray(np.asarray(walls).transpose(0, 2, 1), dtype=np.uint8)
        ix = None if index is None else np.ascontiguousarray(index, dtype=np.int32)
        mk = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        rc = lib.rcw_dev_validate_walls(H, W, B, ptr(flat), 0 if walls is None else len(walls), ptr(ix), ptr(mk), msg, 256)
        return rc, msg.value.decode()

    return call


def test_the_device_less_validation(rcw, validate):
    L = rcw.layouts
    ring, rooms = L.ring(6, 7), L.four_rooms(6, 7)
    assert validate(6, 7, 4, ring[None]) == (0, "")
    assert validate(6, 7, 4, np.stack([ring, rooms]), index=[0, 1, 1, 0]) == (0, "")
    assert validate(6, 7, 2, np.stack([ring, rooms])) == (0, "")             # layouts == B, a NULL index
    for i, j in ((0, 3), (5, 0), (2, 6), (5, 6)):                            # a missing ring tile, named 1-based
        bad = rooms.copy(); bad[i, j] = False
        rc, msg = validate(6, 7, 4, np.stack([ring, bad]), index=[0, 0, 0, 0])   # (also a layout nobody takes)
        assert rc == -1 and "layout 1" in msg and f"({i + 1},{j + 1})" in msg and "ring" in msg, msg
    full = np.ones((6, 7), bool); full[2, 2] = False                        # fewer than two free interior tiles
    rc, msg = validate(6, 7, 4, full[None])
    assert rc == -1 and "layout 0" in msg and "1 free interior tile" in msg, msg
    full[3, 4] = False
    assert validate(6, 7, 4, full[None])[0] == 0
    for index in ([0, 2, 1, 0], [0, -1, 1, 0]):                              # an index out of range
        rc, msg = validate(6, 7, 4, np.stack([ring, rooms]), index=index)
        assert rc == -1 and "agent 1" in msg and "0..1" in msg, msg
    assert validate(6, 7, 4, np.stack([ring, rooms]), index=[0, 2, 1, 0], mask=[1, 0, 1, 1])[0] == 0   # (a masked-out agent's entry is not read)
    rc, msg = validate(6, 7, 4, np.stack([ring, rooms, ring]))               # layouts not in {1, B} with a NULL index
    assert rc == -1 and "3 layouts" in msg, msg
    assert validate(6, 7, 4, None)[0] == -1
    rc, msg = validate(3, 3, 1, L.ring(3, 3)[None])                          # one interior tile: no room for a goal and a player
    assert rc == -1 and "1 free interior tile" in msg


def test_the_host_draws_without_walls_are_what_they_were(rcw):
    """walls=None: the same generator state in, the same values and the same state out as the function had before the keyword existed
    (restated here from its text); walls = the ring: the same again"""
    SR = rcw.SingleRoomModule

    def before(rng, H, W, nd):
        gi, gj = int(rng.integers(2, H)), int(rng.integers(2, W))
        occupied = lambda lin: lin % H in (0, H - 1) or lin // H in (0, W - 1) or (lin % H + 1, lin // H + 1) == (gi, gj)
        lin = int(rng.integers(0, H * W))
        for _ in range(1024 * H * W):
            if not occupied(lin):
                break
            lin = int(rng.integers(0, H * W))
        return gi, gj, lin % H + 1, lin // H + 1, int(rng.integers(0, nd))

    for H, W in ((8, 8), (5, 7), (4, 4)):
        a, b, c = (np.random.default_rng(21) for _ in range(3))
        for _ in range(50):
            want = before(a, H, W, 16)
            assert SR.reference_reset_draws(b, H, W, 16) == want == SR.reference_reset_draws(c, H, W, 16, walls=rcw.layouts.ring(H, W))
            assert a.bit_generator.state == b.bit_generator.state == c.bit_generator.state


def test_the_host_draws_keep_goal_and_player_off_the_walls(rcw):
    SR = rcw.SingleRoomModule
    walls = rcw.layouts.ring(8, 8)
    walls[1:-1, 1:-1] = (np.arange(36) % 2 == 0).reshape(6, 6)               # half of the 36 interior tiles
    assert walls[1:-1, 1:-1].sum() == 18
    rng, shadow = np.random.default_rng(4), np.random.default_rng(4)
    redrawn = 0
    for _ in range(200):
        first = (int(shadow.integers(2, 8)), int(shadow.integers(2, 8)))     # the pair a reset draws first
        gi, gj, ti, tj, d = SR.reference_reset_draws(rng, 8, 8, 8, walls=walls)
        assert not walls[gi - 1, gj - 1] and not walls[ti - 1, tj - 1] and (ti, tj) != (gi, gj) and 0 <= d < 8
        redrawn += int(walls[first[0] - 1, first[1] - 1])
        assert (first == (gi, gj)) == (not walls[first[0] - 1, first[1] - 1])
        shadow.bit_generator.state = rng.bit_generator.state
    assert redrawn >= 1, redrawn                                             # (about half of them)


@pytest.mark.parametrize("H,W", [(5, 5), (8, 8), (9, 12), (32, 32)])
def test_the_layout_generators(rcw, H, W):
    L = rcw.layouts
    maze = L.maze(H, W, np.random.default_rng(3))
    for walls in (L.ring(H, W), L.four_rooms(H, W), maze):
        assert walls.dtype == np.bool_ and walls.shape == (H, W)
        assert walls[0].all() and walls[-1].all() and walls[:, 0].all() and walls[:, -1].all()
        assert (~walls[1:-1, 1:-1]).sum() >= 2 and L.is_connected(walls)
    np.testing.assert_array_equal(maze, L.maze(H, W, np.random.default_rng(3)))      # a pure function of its rng
    assert (maze != L.maze(H, W, np.random.default_rng(4))).any() or (H, W) == (5, 5)
    assert not (~L.ring(H, W))[0].any() and (~L.ring(H, W))[1:-1, 1:-1].all()
    split = L.ring(H, W); split[:, W // 2] = True
    assert not L.is_connected(split) and not L.is_connected(np.ones((H, W), bool))
