"""The rooms on the GPU (include/rcw.h, rcw_set_wall_rooms): what exists because of the ROOMS' kernel.  What the rooms share with the
generator and the caves is written once in tests/test_gpu_wall_families.py: the host replay, the graph, the shards, the fuzzer and more
run there, a case a family; the scenarios of tests/wall_rooms_cases.py after every call, the features and the maps the rooms do not take
are its bodies, run HERE under the rooms' own cases.

WIDER THAN A WAVEFRONT AND AT THE SIZE BOUND: at 66 x 66 with room 1 the level of 0 .. 149 whose widest round cuts 166 chambers (a lane
takes three) and the one with the most rounds (25), installed through levels=1 on 33 agents and compared with both CPU makers; 1031
agents, more workgroups than the device holds at once, each against the host export; 130 x 130 and 5 x 4097, Q = 4096, without frames;
and which calls the rooms refuse and which refuse them.  Every comparison is exact.
"""
import ctypes as C

import numpy as np
import pytest

import test_gpu_wall_families as shared
import wall_rooms_cases as RC
import wall_rooms_ref as RR
from wall_family import engine_state, infos, level_key, unchanged

pytestmark = pytest.mark.gpu
QUARTER = RR.word(0.25)
DEFAULTS = dict(enabled=True, room=2, stop=QUARTER, doors=QUARTER)


# ---- what every family has, under this family's own cases: the bodies are tests/test_gpu_wall_families.py's --------------------------------
@pytest.mark.parametrize("name,form", RC.ROLLOUTS, ids=shared.rollout_ids(RC.ROLLOUTS))
def test_a_scenario_against_the_reference_after_every_call(rcw, name, form):
    shared.a_scenario_against_the_reference_after_every_call(rcw, "rooms", name, form)


@pytest.mark.parametrize("form", shared.FORMS)
@pytest.mark.parametrize("feature", shared.FEATURES)
def test_the_features_follow_the_new_layout_in_one_pass(rcw, feature, form):
    shared.the_features_follow_the_new_layout_in_one_pass(rcw, "rooms", feature, form)


@pytest.mark.parametrize("H,W,exc,message", RC.REFUSED_MAPS)
def test_a_map_the_rooms_do_not_take(rcw, H, W, exc, message):
    shared.a_map_the_family_does_not_take(rcw, "rooms", H, W, exc, message)


# ---- wider than a wavefront, and at the size bound ------------------------------------------------------------------------------------------
def assert_rooms_of_the_rule(L, walls, H, W, m, room, stop, doors, where):
    """one agent's walls against both CPU makers of the rooms of key m, and what holds of every layout"""
    assert walls.tobytes() == RR.rooms(m, H, W, room, stop, doors).tobytes(), f"the reference's rooms, {where}"
    assert walls.tobytes() == L.generated_rooms(m, H, W, room, stop, doors).tobytes(), f"the host export's rooms, {where}"
    assert L.is_connected(walls), where
    assert walls[0].all() and walls[-1].all() and walls[:, 0].all() and walls[:, -1].all(), f"the ring, {where}"


@pytest.mark.parametrize("which", ["widest", "deepest"])
def test_the_widest_round_and_the_most_rounds_at_66_by_66(rcw, which):
    """levels=1: every agent's key is episode_key(level_seed, first_level, 0), so the test chooses its layout — of the levels 0 .. 149 under
    level seed 9 with room 1, stop 0, doors 0 the one whose widest round cuts 166 chambers, three to a lane, and the one that takes 25
    rounds (the search: tests/test_wall_rooms_spec.py).  33 agents, no frames compared; the walls byte for byte against the Python
    reference and the host export, after the install and after a step that restarts everybody under limit 1; then other parameters over
    the same key."""
    L, (H, W) = rcw.layouts, (66, 66)
    level, figure = RC.WIDEST_LEVEL if which == "widest" else RC.DEEPEST_LEVEL
    m = level_key(RC.HARD_LEVEL_SEED, level)
    _, rounds, widest, entries = RR.rounds(m, H, W, 1, 0, 0)
    assert (widest if which == "widest" else rounds) == figure and widest > 64 and entries > 400
    assert L.generated_maze_key(0, 0, 0, 1, level, RC.HARD_LEVEL_SEED) == (m, level)
    env = RC.make_env(rcw, dict(RC.EDGE, T="Float64" if which == "deepest" else "Float32"))
    B = env.batch
    for room, stop, doors in ((1, 0, 0), (1, 0, RC.ALL), (2, QUARTER, QUARTER), (5, 0, 1 << 31)):
        env.set_time_limit(0)
        env.set_wall_rooms(room, stop, doors, levels=1, first_level=level, level_seed=RC.HARD_LEVEL_SEED)
        for when in ("installed", "restarted"):
            walls = env.world.walls
            assert (env.wall_layout.numpy() == level).all()
            assert (walls == walls[0]).all()
            assert_rooms_of_the_rule(L, walls[0], H, W, m, room, stop, doors, f"room {room}, stop {stop}, doors {doors}, {when}")
            if when == "installed":
                episode = env.world.episode.copy()
                env.set_time_limit(1)
                for _ in range(2):                                           # the first step ends every episode (done or truncated), the second restarts it
                    rcw.act_(env, np.ones(B, np.uint8))
                np.testing.assert_array_equal(env.world.episode, episode + 1)
    assert env.world.player_position_wu.dtype == (np.float64 if which == "deepest" else np.float32)
    env.close()


def test_1031_layouts_at_66_by_66_and_a_masked_reset_beside_them(rcw):
    """1031 agents — a prime, more workgroups than the device holds at once — make a later workgroup reuse the LDS of an earlier one
    uncleared, where a word, a list entry or the tail left uninitialised would first show.  No levels, room 1 and no stop: 1031 distinct
    layouts of several hundred rooms, each against the host export (tests/test_wall_rooms_spec.py pins the export to the Python reference
    at this shape).  Then a masked reset_ of every other agent under a new seed: the masked agents hold the rooms of their new keys, the
    others are byte-identical."""
    L = rcw.layouts
    H = W = 66
    B, seed = 1031, 17
    env = RC.make_env(rcw, dict(H=H, W=W, N=8, Hc=16, B=B, seed=seed))
    env.set_wall_rooms(1, 0, 0.25)

    def check(seeds, where):
        walls, episode = env.world.walls, env.world.episode
        assert (env.wall_layout.numpy() == -1).all(), where
        for a in range(B):
            key, level = L.generated_maze_key(int(seeds[a]), a, int(episode[a]) - 1)
            assert level == -1
            assert walls[a].tobytes() == L.generated_rooms(key, H, W, 1, 0, 0.25).tobytes(), f"agent {a} {where}"
        return walls

    walls = check(np.full(B, seed), "installed")
    assert len({w.tobytes() for w in walls}) == B                             # 1031 distinct layouts
    w = env.world
    before = dict(tile_map=w.tile_map_chunks.copy(), goal=w.goal_position.copy(), position=w.player_position_wu.copy(),
                  heading=w.player_direction_au.copy(), episode=w.episode.copy())
    mask = (np.arange(B) % 2).astype(np.uint8)
    rcw.reset_(env, mask, 18)
    check(np.where(mask != 0, 18, seed), "behind the masked reset")
    w, kept = env.world, mask == 0
    after = dict(tile_map=w.tile_map_chunks, goal=w.goal_position, position=w.player_position_wu, heading=w.player_direction_au, episode=w.episode)
    for k in before:
        np.testing.assert_array_equal(after[k][kept], before[k][kept], err_msg=f"{k} of the agents outside the mask")
    np.testing.assert_array_equal(after["episode"][~kept], before["episode"][~kept] + 1)
    assert (after["tile_map"][~kept] != before["tile_map"][~kept]).any(axis=1).all()    # new rooms for every masked agent
    env.close()


@pytest.mark.parametrize("H,W", [(130, 130), (5, 4097)])
def test_the_two_maps_at_the_bound(rcw, H, W):
    """Q = 4096 on both: the 32 KiB chamber list whole, beside 1057 words at 130 x 130 and 1281 at 5 x 4097, where every wall is three tiles
    and two of every three interior columns end up a room of their own.  Room 1, never a stop: some 1800 and 2048 rooms an agent, the
    count from the host export; each agent against the export, one against the Python rule; then the defaults after a restart.  No frames."""
    L, B = rcw.layouts, 5
    assert RR.bound(H, W) == 4096 == RR.MAX_ROOMS
    env = RC.make_env(rcw, dict(H=H, W=W, N=8, Hc=16, B=B, seed=23))
    for room, stop, doors in ((1, 0, 0), (2, QUARTER, QUARTER)):
        env.set_wall_rooms(room, stop, doors)
        for when in ("installed", "reset"):
            walls, most = env.world.walls, 0
            for a in range(B):
                key, _ = L.generated_maze_key(23, a, int(env.world.episode[a]) - 1)
                want, n = L.generated_rooms(key, H, W, room, stop, doors, return_rooms=True)
                assert walls[a].tobytes() == want.tobytes(), f"agent {a}, room {room}, {when}"
                most = max(most, n)
            assert most > 1500 if room == 1 else most >= 2
            rcw.reset_(env)
    key, _ = L.generated_maze_key(23, 0, int(env.world.episode[0]) - 1)
    assert env.world.walls[0].tobytes() == RR.rooms(key, H, W, 2, QUARTER, QUARTER).tobytes()    # ... and one of them against the Python rule
    rcw.act_(env, np.ones(B, np.uint8))                                      # ... and it still steps
    env.close()


# ---- the call rules and hostile arguments ------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_byte_identical(rcw):
    from raycastworlds_jl_amd import _capi

    c = RC.CALLS
    env = RC.make_env(rcw, c, max_episode_steps=5)
    lib, h = env._lib, env._h
    off, gen_off = dict(enabled=False, room=0, stop=0, doors=0), dict(enabled=False, loops=0, levels=0, first_level=0, level_seed=0)
    caves_off = dict(enabled=False, fill=0, smooth=0)
    out, p = np.zeros(c["B"], np.int32), C.c_void_p()
    # with no source of layouts on, the getters are refused; switching off is fine
    assert lib.rcw_wall_layout(h, out.ctypes.data_as(C.c_void_p)) == _capi.RCW_ERR_UNSUPPORTED
    assert lib.rcw_wall_layout_device_ptr(h, C.byref(p)) == _capi.RCW_ERR_UNSUPPORTED
    assert env.wall_rooms_info == off and env.wall_generator_info == gen_off
    assert lib.rcw_wall_rooms_info(h, None, None, None, None) == _capi.RCW_OK     # any pointer may be NULL
    assert lib.rcw_wall_rooms_info(None, None, None, None, None) == _capi.RCW_ERR_INVALID_ARGUMENT
    env.set_wall_rooms(None)
    bank = np.stack([rcw.layouts.ring(8, 8), rcw.layouts.four_rooms(8, 8)])

    def refused(call, exc, message, code=None):
        before, info = engine_state(env), infos(env)
        with pytest.raises(exc, match=message) as ei:
            call()
        if code is not None:
            assert ei.value.code == code
        unchanged(env, before, info, message)

    def nothing(call, what):
        before, info = engine_state(env), infos(env)
        call()
        unchanged(env, before, info, what)

    # rooms on: a bank, the generator, caves and set_walls are refused; bad arguments are, and the running rooms stay
    env.set_wall_rooms(1, 0.25, 0.5, levels=4, first_level=2, level_seed=6)
    assert env.wall_rooms_info == dict(enabled=True, room=1, stop=1 << 30, doors=1 << 31) and env.wall_caves_info == caves_off
    assert env.wall_generator_info == dict(enabled=True, loops=0, levels=4, first_level=2, level_seed=6)
    rcw.act_(env, np.ones(c["B"], np.uint8))
    ptr = env.wall_layout.ptr
    refused(lambda: env.set_wall_bank(bank), _capi.RcwError, "rcw_set_wall_rooms\\(h, 0", _capi.RCW_ERR_UNSUPPORTED)
    refused(lambda: env.set_walls(bank[0]), _capi.RcwError, "rcw_set_wall_rooms\\(h, 0", _capi.RCW_ERR_UNSUPPORTED)
    refused(lambda: env.set_wall_generator(0.25), _capi.RcwError, "rcw_set_wall_rooms\\(h, 0", _capi.RCW_ERR_UNSUPPORTED)
    refused(lambda: env.set_wall_caves(), _capi.RcwError, "rcw_set_wall_rooms\\(h, 0", _capi.RCW_ERR_UNSUPPORTED)
    nothing(lambda: env.set_wall_generator(None), "set_wall_generator(None)")   # the other families' switches do not end the rooms
    nothing(lambda: env.set_wall_caves(None), "set_wall_caves(None)")
    refused(lambda: env._check(lib.rcw_set_wall_rooms(h, 1, 0, 0, 0, 0, 0, 0)), ValueError, "at least 1 tile")
    refused(lambda: env._check(lib.rcw_set_wall_rooms(h, 1, -3, 0, 0, 0, 0, 0)), ValueError, "at least 1 tile")
    refused(lambda: env.set_wall_rooms(0), ValueError, "at least 1 tile")
    refused(lambda: env._check(lib.rcw_set_wall_rooms(h, 1, 2, 0, 0, -1, 0, 0)), ValueError, "level range")
    refused(lambda: env._check(lib.rcw_set_wall_rooms(h, 1, 2, 0, 0, 1, -1, 0)), ValueError, "level range")
    refused(lambda: env._check(lib.rcw_set_wall_rooms(h, 1, 2, 0, 0, 2, 2 ** 31 - 2, 0)), ValueError, "level range")
    refused(lambda: env.set_wall_rooms(2, 1.5), ValueError, "probability")
    refused(lambda: env.set_wall_rooms(2, 0.5, -0.5), ValueError, "probability")
    refused(lambda: env.set_wall_rooms(2.5), ValueError, "room")
    refused(lambda: env.set_wall_rooms(2, levels=-1), ValueError, "levels")
    refused(lambda: env.set_wall_rooms(2, level_seed=2 ** 64), ValueError, "level_seed")
    refused(lambda: rcw.reset_(env, rng=np.random.default_rng(1)), ValueError, "wall generator")
    assert env.wall_layout.ptr == ptr
    env.set_wall_rooms(3, 0, 0, levels=1, first_level=2 ** 31 - 2)           # the last level there is
    assert (env.wall_layout.numpy() == 2 ** 31 - 2).all()
    # switching off keeps the walls; then each other source on in turn: rooms are refused, and their switch ends none of them
    walls, episode = env.world.walls, env.world.episode
    env.set_wall_rooms(None)
    assert env.wall_rooms_info == off and env.wall_generator_info == gen_off
    np.testing.assert_array_equal(env.world.walls, walls)
    np.testing.assert_array_equal(env.world.episode, episode)
    assert lib.rcw_wall_layout(h, out.ctypes.data_as(C.c_void_p)) == _capi.RCW_ERR_UNSUPPORTED
    env.set_wall_bank(bank)
    rcw.act_(env, np.ones(c["B"], np.uint8))
    refused(lambda: env.set_wall_rooms(), _capi.RcwError, "switch the bank off first", _capi.RCW_ERR_UNSUPPORTED)
    nothing(lambda: env.set_wall_rooms(None), "set_wall_rooms(None) beside a bank")
    env.set_wall_bank(None)
    env.set_wall_generator(0.25, levels=2)
    refused(lambda: env.set_wall_rooms(), _capi.RcwError, "switch the generator off first", _capi.RCW_ERR_UNSUPPORTED)
    nothing(lambda: env.set_wall_rooms(None), "set_wall_rooms(None) beside the generator")
    assert env.wall_generator_info["loops"] == 1 << 30 and not env.wall_rooms_info["enabled"]
    env.set_wall_generator(None)
    env.set_wall_caves(levels=2)
    refused(lambda: env.set_wall_rooms(), _capi.RcwError, "rcw_set_wall_caves\\(h, 0", _capi.RCW_ERR_UNSUPPORTED)
    nothing(lambda: env.set_wall_rooms(None), "set_wall_rooms(None) beside caves")
    assert env.wall_caves_info["enabled"] and not env.wall_rooms_info["enabled"]
    env.set_wall_caves(None)
    env.set_walls(bank[1])                                                   # set_walls works again
    env.set_wall_rooms()                                                     # ... and rooms are fine once everything else is off
    assert env.wall_rooms_info == DEFAULTS and all(rcw.layouts.is_connected(w) for w in env.world.walls)
    env.close()
    # an environment built with rng takes no rooms; rooms and another source in one constructor
    with pytest.raises(ValueError, match="rng"):
        RC.make_env(rcw, dict(c, B=2), rng=np.random.default_rng(0), wall_rooms={})
    with pytest.raises(ValueError, match="rng"):
        rcw.ShardedSingleRoom(4, rank=0, world=2, device=0, rng=np.random.default_rng(0), wall_rooms={})
    with pytest.raises(_capi.RcwError, match="switch the generator off first"):
        RC.make_env(rcw, dict(c, B=2), wall_generator={}, wall_rooms={})
    with pytest.raises(_capi.RcwError, match="rcw_set_wall_caves\\(h, 0"):
        RC.make_env(rcw, dict(c, B=2), wall_caves={}, wall_rooms={})
    with pytest.raises(_capi.RcwError, match="switch the bank off first"):
        RC.make_env(rcw, dict(c, B=2), wall_bank=bank, wall_rooms={})
