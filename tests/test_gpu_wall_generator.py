"""The wall generator on the GPU (include/rcw.h, rcw_set_wall_generator): what exists because of the MAZE kernel.  What the generator shares
with the caves and the rooms is written once in tests/test_gpu_wall_families.py: the host replay, the graph, the shards, the fuzzer and
more run there, a case a family; the scenarios of tests/wall_generator_cases.py after every call (at the size bound too: `edge`, `thin`,
`tall`, ...), the features and the maps the generator does not take are its bodies, run HERE under the generator's own cases.

Here: the hardest mazes a search with the model of the kernel's rounds finds (wall_generator_ref.boruvka), installed through levels=1, at
the size bound of 4096 cells (64 cells a lane, 48 KiB of slots and labels beside the words) and below it; 1031 agents, more workgroups than
the device holds at once; which calls the generator refuses and which refuse it; and NeverLost, the tracker every family's tests hold
beside the goal distance.
"""
import ctypes as C

import numpy as np
import pytest

import test_gpu_wall_families as shared
import wall_generator_cases as GC
import wall_generator_ref as WG
from wall_family import engine_state, infos, level_key, unchanged

pytestmark = pytest.mark.gpu


class NeverLost:
    """with the goal distance on, no agent ever reads -1: the generator's mazes are connected"""

    def __init__(self, env):
        self.env, self.checked = env, 0

    def _check(self, where):
        d = self.env.goal_distance.numpy()
        assert (d >= 0).all(), f"an agent without a path to its goal, {where}: {d}"
        assert (self.env.goal_distance_field[~self.env.world.walls] != 0xFFFF).all(), f"a free tile without a path, {where}"
        self.checked += 1

    def stepped(self, actions, where):
        self._check(where)

    def masked(self, mask, where):
        self._check(where)


# ---- what every family has, under this family's own cases: the bodies are tests/test_gpu_wall_families.py's --------------------------------
@pytest.mark.parametrize("name,form", GC.ROLLOUTS, ids=shared.rollout_ids(GC.ROLLOUTS))
def test_a_scenario_against_the_reference_after_every_call(rcw, name, form):
    shared.a_scenario_against_the_reference_after_every_call(rcw, "generator", name, form)


@pytest.mark.parametrize("form", shared.FORMS)
@pytest.mark.parametrize("feature", shared.FEATURES)
def test_the_features_follow_the_new_maze_in_one_pass(rcw, feature, form):
    shared.the_features_follow_the_new_layout_in_one_pass(rcw, "generator", feature, form)


@pytest.mark.parametrize("H,W,exc,message", GC.REFUSED_MAPS)
def test_a_map_the_generator_does_not_take(rcw, H, W, exc, message):
    shared.a_map_the_family_does_not_take(rcw, "generator", H, W, exc, message)


# ---- mazes chosen for the rounds they take ------------------------------------------------------------------------------------------------
def assert_a_maze_of_the_rule(L, walls, H, W, m, word, where):
    """one agent's walls against both CPU makers of the maze of key m, and what holds of every maze"""
    assert walls.tobytes() == WG.maze(m, H, W, word).tobytes(), f"the reference's maze, {where}"
    assert walls.tobytes() == L.generated_maze(m, H, W, word).tobytes(), f"the host export's maze, {where}"
    assert L.is_connected(walls), where
    assert walls[0].all() and walls[-1].all() and walls[:, 0].all() and walls[:, -1].all(), f"the ring, {where}"


@pytest.mark.parametrize("T", ["Float32", "Float64"])
@pytest.mark.parametrize("H,W", sorted(GC.HARD_LEVELS))
def test_the_maze_that_takes_the_most_rounds(rcw, H, W, T):
    """levels=1: every agent's maze key is episode_key(level_seed, first_level, 0), so the test chooses its maze — the level of 0 .. 149
    under level seed 9 that takes the model of the kernel's rounds the most rounds, then the deepest hook chain (the search and its
    distribution: tests/test_wall_generator_spec.py).  Seven rounds at 129 x 129 and eight on the thin maps are the most that search
    shows; random keys come nowhere near the kernel's cap of 13, and nothing here claims to.  The rounds are asserted from the model,
    never from the engine.  Three agents, a perfect maze and loops 0.25: the walls byte for byte against the Python reference and the
    host export, after the install and after a step that restarts everybody under limit 1."""
    L, level = rcw.layouts, GC.HARD_LEVELS[(H, W)]
    m = level_key(GC.HARD_LEVEL_SEED, level)
    tree, rounds, chain = WG.boruvka(m, H, W)
    assert tree == sorted(WG.tree_edges(m, H, W))
    assert rounds >= {(129, 129): 7, (5, 4097): 8, (4097, 5): 8, (33, 33): 5}[(H, W)] == GC.HARD_ROUNDS[(H, W)] and chain >= 6
    assert L.generated_maze_key(0, 0, 0, 1, level, GC.HARD_LEVEL_SEED) == (m, level)
    env = GC.make_env(rcw, dict(H=H, W=W, N=8, Hc=16, B=3, seed=3, T=T))
    for loops in (0.0, 0.25):
        word = WG.loops_word(loops)
        env.set_time_limit(0)
        env.set_wall_generator(loops, levels=1, first_level=level, level_seed=GC.HARD_LEVEL_SEED)
        for when in ("installed", "restarted"):
            walls = env.world.walls
            assert (env.wall_layout.numpy() == level).all()
            for a in range(3):
                assert_a_maze_of_the_rule(L, walls[a], H, W, m, word, f"agent {a}, loops {loops}, {when}")
            if loops == 0.0:
                assert int((~walls[0]).sum()) == 2 * WG.grid(H, W)[2] - 1    # a perfect maze: the cells and a passage a tree edge
            if when == "installed":
                episode = env.world.episode.copy()
                env.set_time_limit(1)
                for _ in range(2):                                           # the first step ends every episode (done or truncated), the second restarts it
                    rcw.act_(env, np.ones(3, np.uint8))
                np.testing.assert_array_equal(env.world.episode, episode + 1)
    assert env.world.player_position_wu.dtype == (np.float64 if T == "Float64" else np.float32)
    env.close()


# ---- more agents than the device holds workgroups ----------------------------------------------------------------------------------------------
def test_1031_mazes_of_4096_cells_and_a_masked_reset_beside_them(rcw):
    """129 x 129 asks for 1042 words + 48 KiB = 52.1 KiB of LDS a workgroup: with 160 KiB a compute unit three workgroups fit, 768 on 256
    compute units (from the documented LDS size; the residency itself has not been measured).  1031 agents — a prime past that — make a
    later workgroup reuse the LDS of an earlier one uncleared, where a slot, a label or a word left uninitialised would first show.  No
    levels: 1031 distinct mazes, each against the host export (tests/test_wall_generator_spec.py pins the export to the Python reference
    at this shape; 1031 Python mazes would take a minute).  Then a masked reset_ of every other agent under a new seed — the masked agents
    hold the mazes of their new keys, the others are byte-identical: the two-loads-and-out path beside workgroups that rebuilt their
    LDS — and five levels shared by all."""
    L = rcw.layouts
    H = W = 129
    B, seed, loops = 1031, 17, 0.1
    env = GC.make_env(rcw, dict(H=H, W=W, N=8, Hc=16, B=B, seed=seed))
    env.set_wall_generator(loops)

    def check(seeds, where):
        walls, episode = env.world.walls, env.world.episode
        assert (env.wall_layout.numpy() == -1).all(), where
        for a in range(B):
            key, level = L.generated_maze_key(int(seeds[a]), a, int(episode[a]) - 1)
            assert level == -1
            assert walls[a].tobytes() == L.generated_maze(key, H, W, loops).tobytes(), f"agent {a} {where}"
        return walls

    walls = check(np.full(B, seed), "installed")
    assert len({w.tobytes() for w in walls}) == B                             # 1031 distinct mazes
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
    assert (after["tile_map"][~kept] != before["tile_map"][~kept]).any(axis=1).all()    # a new maze for every masked agent
    # five levels: five mazes shared by 1031 agents
    env.set_wall_generator(loops, levels=5, first_level=60, level_seed=4)
    layout, walls = env.wall_layout.numpy(), env.world.walls
    assert set(layout.tolist()) == {60, 61, 62, 63, 64}
    for level in range(60, 65):
        held = walls[layout == level]
        assert len(held) > 100 and (held == held[0]).all()
        assert held[0].tobytes() == L.generated_maze(L.generated_maze_key(0, 0, 0, 1, level, 4)[0], H, W, loops).tobytes()
    for a in range(B):
        assert L.generated_maze_key(18, a, int(env.world.episode[a]) - 1, 5, 60, 4)[1] == layout[a]
    env.close()


# ---- the call rules and hostile arguments ------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_byte_identical(rcw):
    from raycastworlds_jl_amd import _capi

    c = GC.CALLS
    env = GC.make_env(rcw, c, max_episode_steps=5)
    lib, h = env._lib, env._h
    off = dict(enabled=False, loops=0, levels=0, first_level=0, level_seed=0)
    out, p = np.zeros(c["B"], np.int32), C.c_void_p()
    # with neither a bank nor a generator the getters are refused; switching off is fine
    assert lib.rcw_wall_layout(h, out.ctypes.data_as(C.c_void_p)) == _capi.RCW_ERR_UNSUPPORTED
    assert lib.rcw_wall_layout_device_ptr(h, C.byref(p)) == _capi.RCW_ERR_UNSUPPORTED
    assert env.wall_generator_info == off
    assert lib.rcw_wall_generator_info(h, None, None, None, None, None) == _capi.RCW_OK      # any pointer may be NULL
    env.set_wall_generator(None)
    bank = np.stack([rcw.layouts.ring(6, 6), rcw.layouts.four_rooms(6, 6)])

    def refused(call, exc, message, code=None):
        before, info = engine_state(env), infos(env)
        with pytest.raises(exc, match=message) as ei:
            call()
        if code is not None:
            assert ei.value.code == code
        unchanged(env, before, info, message)

    # the generator on: a bank and set_walls are refused; a bad level range is, and the running generator stays
    env.set_wall_generator(0.25, levels=4, first_level=2, level_seed=6)
    assert env.wall_generator_info == dict(enabled=True, loops=1 << 30, levels=4, first_level=2, level_seed=6)
    rcw.act_(env, np.ones(c["B"], np.uint8))
    ptr = env.wall_layout.ptr
    refused(lambda: env.set_wall_bank(bank), _capi.RcwError, "switch the generator off first", _capi.RCW_ERR_UNSUPPORTED)
    refused(lambda: env.set_walls(bank[0]), _capi.RcwError, "switch the generator off first", _capi.RCW_ERR_UNSUPPORTED)
    refused(lambda: env._check(lib.rcw_set_wall_generator(h, 1, 0, -1, 0, 0)), ValueError, "level range")
    refused(lambda: env._check(lib.rcw_set_wall_generator(h, 1, 0, 1, -1, 0)), ValueError, "level range")
    refused(lambda: env._check(lib.rcw_set_wall_generator(h, 1, 0, 2, 2 ** 31 - 2, 0)), ValueError, "level range")
    refused(lambda: env.set_wall_generator(1.5), ValueError, "probability")
    refused(lambda: env.set_wall_generator(0.5, levels=-1), ValueError, "levels")
    refused(lambda: env.set_wall_generator(0.5, level_seed=2 ** 64), ValueError, "level_seed")
    refused(lambda: rcw.reset_(env, rng=np.random.default_rng(1)), ValueError, "wall generator")
    assert env.wall_layout.ptr == ptr
    env.set_wall_generator(0.0, levels=1, first_level=2 ** 31 - 2)           # the last level there is
    assert (env.wall_layout.numpy() == 2 ** 31 - 2).all()
    # switching off keeps the walls; then the bank on: the generator is refused
    walls, episode = env.world.walls, env.world.episode
    env.set_wall_generator(None)
    assert env.wall_generator_info == off
    np.testing.assert_array_equal(env.world.walls, walls)
    np.testing.assert_array_equal(env.world.episode, episode)
    assert lib.rcw_wall_layout(h, out.ctypes.data_as(C.c_void_p)) == _capi.RCW_ERR_UNSUPPORTED
    env.set_wall_bank(bank)
    rcw.act_(env, np.ones(c["B"], np.uint8))
    refused(lambda: env.set_wall_generator(), _capi.RcwError, "switch the bank off first", _capi.RCW_ERR_UNSUPPORTED)
    env.set_wall_bank(None)
    env.set_wall_generator()                                                 # ... and fine once the bank is off
    assert env.wall_generator_info["enabled"] and all(rcw.layouts.is_connected(w) for w in env.world.walls)
    env.close()
    # an environment built with rng takes no generator
    with pytest.raises(ValueError, match="rng"):
        GC.make_env(rcw, dict(c, B=2), rng=np.random.default_rng(0), wall_generator={})
    with pytest.raises(ValueError, match="rng"):
        rcw.ShardedSingleRoom(4, rank=0, world=2, device=0, rng=np.random.default_rng(0), wall_generator={})
