"""The caves on the GPU (include/rcw.h, rcw_set_wall_caves): what exists because of the CAVES' kernel.  What the caves share with the
generator and the rooms is written once in tests/test_gpu_wall_families.py: the host replay, the graph, the shards, the fuzzer and more
run there, a case a family; the scenarios of tests/wall_caves_cases.py after every call, the features and the maps the caves do not take
are its bodies, run HERE under the caves' own cases.

AT THE SIZE BOUND (66 x 66: 4096 interior tiles, 64 a lane, rows wider than a wavefront, 41.9 KiB of LDS): the level of 0 .. 149 that
takes the labelling restatement the most rounds, installed through levels=1 on 33 agents and compared with both CPU makers; and 1031
agents, more workgroups than the device holds at once, each against the host export; 5 x 1367, the thinnest map at the bound; and which
calls the caves refuse and which refuse them.
"""
import ctypes as C

import numpy as np
import pytest

import test_gpu_wall_families as shared
import wall_caves_cases as CC
import wall_caves_ref as WC
from wall_family import engine_state, infos, level_key, unchanged

pytestmark = pytest.mark.gpu
DEFAULT = WC.fill_word(WC.DEFAULT_FILL)


# ---- what every family has, under this family's own cases: the bodies are tests/test_gpu_wall_families.py's --------------------------------
@pytest.mark.parametrize("name,form", CC.ROLLOUTS, ids=shared.rollout_ids(CC.ROLLOUTS))
def test_a_scenario_against_the_reference_after_every_call(rcw, name, form):
    shared.a_scenario_against_the_reference_after_every_call(rcw, "caves", name, form)


@pytest.mark.parametrize("form", shared.FORMS)
@pytest.mark.parametrize("feature", shared.FEATURES)
def test_the_features_follow_the_new_layout_in_one_pass(rcw, feature, form):
    shared.the_features_follow_the_new_layout_in_one_pass(rcw, "caves", feature, form)


@pytest.mark.parametrize("H,W,exc,message", CC.REFUSED_MAPS)
def test_a_map_the_caves_do_not_take(rcw, H, W, exc, message):
    shared.a_map_the_family_does_not_take(rcw, "caves", H, W, exc, message)


# ---- at the size bound ------------------------------------------------------------------------------------------------------------------
def assert_a_cave_of_the_rule(L, walls, H, W, m, fill, smooth, where):
    """one agent's walls against both CPU makers of the cave of key m, and what holds of every layout"""
    assert walls.tobytes() == WC.cave(m, H, W, fill, smooth).tobytes(), f"the reference's cave, {where}"
    assert walls.tobytes() == L.generated_cave(m, H, W, fill, smooth).tobytes(), f"the host export's cave, {where}"
    assert L.is_connected(walls), where
    assert walls[0].all() and walls[-1].all() and walls[:, 0].all() and walls[:, -1].all(), f"the ring, {where}"


@pytest.mark.parametrize("T", ["Float32", "Float64"])
def test_the_cave_that_takes_the_most_labelling_rounds_at_66_by_66(rcw, T):
    """levels=1: every agent's key is episode_key(level_seed, first_level, 0), so the test chooses its cave — the level of 0 .. 149 under
    level seed 9 that takes the labelling restatement the most rounds (the search: tests/test_wall_caves_spec.py).  33 agents, no frames
    compared; the walls byte for byte against the Python reference and the host export, after the install and after a step that restarts
    everybody under limit 1; then other parameters over the same key: unsmoothed (fill 0.30 keeps its cave, the default fill falls back: its
    free tiles do not percolate), smoothed eight times, and fill 0.55, which falls back smoothed."""
    L, (H, W) = rcw.layouts, (66, 66)
    level, rounds = CC.HARD_LEVELS[(H, W)]
    m = level_key(CC.HARD_LEVEL_SEED, level)
    g = WC.smoothed(m, H, W, DEFAULT, WC.DEFAULT_SMOOTH)
    assert WC.labelling(g)[1] == rounds == 4 and (H - 2) * (W - 2) == 4096 == WC.MAX_TILES
    assert L.generated_maze_key(0, 0, 0, 1, level, CC.HARD_LEVEL_SEED) == (m, level)
    env = CC.make_env(rcw, dict(CC.EDGE, T=T))
    B = env.batch
    for fill, smooth, falls in ((DEFAULT, 2, False), (WC.fill_word(0.30), 0, False), (DEFAULT, 0, True), (DEFAULT, 8, False), (WC.fill_word(0.55), 2, True)):
        env.set_time_limit(0)
        env.set_wall_caves(fill, smooth, levels=1, first_level=level, level_seed=CC.HARD_LEVEL_SEED)
        assert L.generated_cave(m, H, W, fill, smooth, return_fell_back=True)[1] == falls
        for when in ("installed", "restarted"):
            walls = env.world.walls
            assert (env.wall_layout.numpy() == level).all()
            assert (walls == walls[0]).all()
            assert_a_cave_of_the_rule(L, walls[0], H, W, m, fill, smooth, f"fill {fill}, smooth {smooth}, {when}")
            if when == "installed":
                episode = env.world.episode.copy()
                env.set_time_limit(1)
                for _ in range(2):                                           # the first step ends every episode (done or truncated), the second restarts it
                    rcw.act_(env, np.ones(B, np.uint8))
                np.testing.assert_array_equal(env.world.episode, episode + 1)
    assert env.world.player_position_wu.dtype == (np.float64 if T == "Float64" else np.float32)
    env.close()


def test_1031_caves_of_4096_tiles_and_a_masked_reset_beside_them(rcw):
    """66 x 66 asks for 41.9 KiB of LDS a workgroup: with 160 KiB a compute unit three workgroups fit, 768 on 256 compute units (from the
    documented LDS size; the residency itself has not been measured).  1031 agents — a prime past that — make a later workgroup reuse the
    LDS of an earlier one uncleared, where a label, a counter or a plane left uninitialised would first show.  No levels: 1031 distinct
    caves, each against the host export (tests/test_wall_caves_spec.py pins the export to the Python reference at this shape).  Then a
    masked reset_ of every other agent under a new seed: the masked agents hold the caves of their new keys, the others are
    byte-identical."""
    L = rcw.layouts
    H = W = 66
    B, seed = 1031, 17
    env = CC.make_env(rcw, dict(H=H, W=W, N=8, Hc=16, B=B, seed=seed))
    env.set_wall_caves()

    def check(seeds, where):
        walls, episode = env.world.walls, env.world.episode
        assert (env.wall_layout.numpy() == -1).all(), where
        for a in range(B):
            key, level = L.generated_maze_key(int(seeds[a]), a, int(episode[a]) - 1)
            assert level == -1
            assert walls[a].tobytes() == L.generated_cave(key, H, W).tobytes(), f"agent {a} {where}"
        return walls

    walls = check(np.full(B, seed), "installed")
    assert len({w.tobytes() for w in walls}) == B                             # 1031 distinct caves
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
    assert (after["tile_map"][~kept] != before["tile_map"][~kept]).any(axis=1).all()    # a new cave for every masked agent
    env.close()


def test_the_thinnest_map_at_the_bound(rcw):
    """5 x 1367: 3 x 1365 = 4095 interior tiles on the map with the most words (428) the bound admits — the largest LDS request the launch
    makes — and a cell grid of 2 x 683 for the fallback.  A corridor three tiles wide: at fill 0.10 without smoothing some agents keep
    a cave and some fall back, at the defaults every one falls back; each agent against the host export."""
    L, H, W, B = rcw.layouts, 5, 1367, 5
    env = CC.make_env(rcw, dict(H=H, W=W, N=8, Hc=16, B=B, seed=23))
    for fill, smooth in ((0.10, 0), (0.40, 2)):
        env.set_wall_caves(fill, smooth)
        walls, fell = env.world.walls, 0
        for a in range(B):
            key, _ = L.generated_maze_key(23, a, int(env.world.episode[a]) - 1)
            want, f = L.generated_cave(key, H, W, fill, smooth, return_fell_back=True)
            assert walls[a].tobytes() == want.tobytes(), f"agent {a}, fill {fill}"
            fell += f
        assert 0 < fell < B if smooth == 0 else fell == B
    key, _ = L.generated_maze_key(23, 0, int(env.world.episode[0]) - 1)
    assert walls[0].tobytes() == WC.cave(key, H, W, DEFAULT, 2).tobytes()    # ... and one of them against the Python rule
    env.close()


# ---- the call rules and hostile arguments ------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_byte_identical(rcw):
    from raycastworlds_jl_amd import _capi

    c = CC.CALLS
    env = CC.make_env(rcw, c, max_episode_steps=5)
    lib, h = env._lib, env._h
    off, gen_off = dict(enabled=False, fill=0, smooth=0), dict(enabled=False, loops=0, levels=0, first_level=0, level_seed=0)
    out, p = np.zeros(c["B"], np.int32), C.c_void_p()
    # with neither a bank nor a generator nor caves the getters are refused; switching off is fine
    assert lib.rcw_wall_layout(h, out.ctypes.data_as(C.c_void_p)) == _capi.RCW_ERR_UNSUPPORTED
    assert lib.rcw_wall_layout_device_ptr(h, C.byref(p)) == _capi.RCW_ERR_UNSUPPORTED
    assert env.wall_caves_info == off and env.wall_generator_info == gen_off
    assert lib.rcw_wall_caves_info(h, None, None, None) == _capi.RCW_OK           # any pointer may be NULL
    assert lib.rcw_wall_caves_info(None, None, None, None) == _capi.RCW_ERR_INVALID_ARGUMENT
    env.set_wall_caves(None)
    bank = np.stack([rcw.layouts.ring(8, 8), rcw.layouts.four_rooms(8, 8)])

    def refused(call, exc, message, code=None):
        before, info = engine_state(env), infos(env)
        with pytest.raises(exc, match=message) as ei:
            call()
        if code is not None:
            assert ei.value.code == code
        unchanged(env, before, info, message)

    # caves on: a bank, the generator and set_walls are refused; bad arguments are, and the running caves stay
    env.set_wall_caves(0.25, 3, levels=4, first_level=2, level_seed=6)
    assert env.wall_caves_info == dict(enabled=True, fill=1 << 30, smooth=3)
    assert env.wall_generator_info == dict(enabled=True, loops=0, levels=4, first_level=2, level_seed=6)
    rcw.act_(env, np.ones(c["B"], np.uint8))
    ptr = env.wall_layout.ptr
    refused(lambda: env.set_wall_bank(bank), _capi.RcwError, "switch them off first", _capi.RCW_ERR_UNSUPPORTED)
    refused(lambda: env.set_walls(bank[0]), _capi.RcwError, "switch them off first", _capi.RCW_ERR_UNSUPPORTED)
    refused(lambda: env.set_wall_generator(0.25), _capi.RcwError, "switch them off first", _capi.RCW_ERR_UNSUPPORTED)
    before, info = engine_state(env), infos(env)
    env.set_wall_generator(None)                                             # the generator's switch does not end the caves
    unchanged(env, before, info, "set_wall_generator(None)")
    refused(lambda: env._check(lib.rcw_set_wall_caves(h, 1, 0, -1, 0, 0, 0)), ValueError, "0 .. 8")
    refused(lambda: env._check(lib.rcw_set_wall_caves(h, 1, 0, 9, 0, 0, 0)), ValueError, "0 .. 8")
    refused(lambda: env.set_wall_caves(0.4, 9), ValueError, "0 .. 8")
    refused(lambda: env._check(lib.rcw_set_wall_caves(h, 1, 0, 2, -1, 0, 0)), ValueError, "level range")
    refused(lambda: env._check(lib.rcw_set_wall_caves(h, 1, 0, 2, 1, -1, 0)), ValueError, "level range")
    refused(lambda: env._check(lib.rcw_set_wall_caves(h, 1, 0, 2, 2, 2 ** 31 - 2, 0)), ValueError, "level range")
    refused(lambda: env.set_wall_caves(1.5), ValueError, "probability")
    refused(lambda: env.set_wall_caves(0.5, levels=-1), ValueError, "levels")
    refused(lambda: env.set_wall_caves(0.5, level_seed=2 ** 64), ValueError, "level_seed")
    refused(lambda: rcw.reset_(env, rng=np.random.default_rng(1)), ValueError, "wall generator")
    assert env.wall_layout.ptr == ptr
    env.set_wall_caves(0.3, 8, levels=1, first_level=2 ** 31 - 2)            # the last level there is
    assert (env.wall_layout.numpy() == 2 ** 31 - 2).all()
    # switching off keeps the walls; then the bank on: caves are refused; then the generator on: caves are refused
    walls, episode = env.world.walls, env.world.episode
    env.set_wall_caves(None)
    assert env.wall_caves_info == off and env.wall_generator_info == gen_off
    np.testing.assert_array_equal(env.world.walls, walls)
    np.testing.assert_array_equal(env.world.episode, episode)
    assert lib.rcw_wall_layout(h, out.ctypes.data_as(C.c_void_p)) == _capi.RCW_ERR_UNSUPPORTED
    env.set_wall_bank(bank)
    rcw.act_(env, np.ones(c["B"], np.uint8))
    refused(lambda: env.set_wall_caves(), _capi.RcwError, "switch the bank off first", _capi.RCW_ERR_UNSUPPORTED)
    env.set_wall_bank(None)
    env.set_wall_generator(0.25, levels=2)
    refused(lambda: env.set_wall_caves(), _capi.RcwError, "switch the generator off first", _capi.RCW_ERR_UNSUPPORTED)
    before, info = engine_state(env), infos(env)
    env.set_wall_caves(None)                                                 # ... and the caves' switch does not end the generator
    unchanged(env, before, info, "set_wall_caves(None)")
    assert env.wall_generator_info["loops"] == 1 << 30 and not env.wall_caves_info["enabled"]
    env.set_wall_generator(None)
    env.set_walls(bank[1])                                                   # set_walls works again
    env.set_wall_caves()                                                     # ... and caves are fine once everything else is off
    assert env.wall_caves_info == dict(enabled=True, fill=DEFAULT, smooth=2) and all(rcw.layouts.is_connected(w) for w in env.world.walls)
    env.close()
    # an environment built with rng takes no caves; caves and another source in one constructor
    with pytest.raises(ValueError, match="rng"):
        CC.make_env(rcw, dict(c, B=2), rng=np.random.default_rng(0), wall_caves={})
    with pytest.raises(ValueError, match="rng"):
        rcw.ShardedSingleRoom(4, rank=0, world=2, device=0, rng=np.random.default_rng(0), wall_caves={})
    with pytest.raises(_capi.RcwError, match="switch the generator off first"):
        CC.make_env(rcw, dict(c, B=2), wall_generator={}, wall_caves={})
    with pytest.raises(_capi.RcwError, match="switch the bank off first"):
        CC.make_env(rcw, dict(c, B=2), wall_bank=bank, wall_caves={})
