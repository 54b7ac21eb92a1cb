"""The wall generator on the GPU (include/rcw.h, rcw_set_wall_generator): the scenarios of tests/wall_generator_cases.py played on an engine
against tests/wall_generator_ref.py — after EVERY call the whole state of walls_ref.assert_equal (status, episode, goal, pose, reward, done,
tile-map chunks, column descriptors, camera view), wall_layout, and the time limit's two words; and the bank tests' feature trackers beside
them: the goal distance's words and fields (which never read -1: every maze is connected) in every rollout, the seen map, the local map
from the seen map and the 4-frame stack in the `features` scenario.  tests/test_wall_generator_spec.py rehearses every scenario on the CPU
and asserts from the reference's counts that it reaches restarts of both kinds and goal redraws.

AT THE SIZE BOUND (4096 cells: 64 cells a lane, 48 KiB of slots and labels beside the words): the `huge` script at 129 x 129, 130 x 130,
5 x 4097, 4097 x 5 and 6 x 4098 — all recorded WITH frames, the reference takes a second or two each; 129 x 129 in both step forms, the
one-launch step with 64 camera rows (`edge_rows64`: it does not take the 24 of the others) —; the hardest mazes a search with
the model of the kernel's rounds finds (wall_generator_ref.boruvka), installed through levels=1; and 1031 agents, more workgroups than the
device holds at once.

The `small` scenario is the issue's own (67 agents x 320 rays, 30 steps): its reference takes some ten seconds of Python ray casting, once,
shared by the two step forms.  Every export is missing from the build before this feature: each test here fails there.
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import learner_view_ref as LV
import local_map_ref as LM
import time_limit_ref as TL
import wall_generator_cases as GC
import wall_generator_ref as WG
import walls_ref as WR
from test_gpu_wall_bank import GoalTracker, LocalTracker, SeenTracker, StackTracker

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


# ---- the rollouts -----------------------------------------------------------------------------------------------------------------
ROLLOUTS = [("small", "two-launches"), ("small", "one-launch"), ("square", None), ("big", "two-launches"), ("big", "one-launch"), ("wide", None),
            ("huge", None), ("f64", None), ("levels", None), ("calls", "two-launches"), ("calls", "one-launch"),
            ("edge", "two-launches"), ("edge_rows64", "one-launch"), ("edge_even", None), ("thin", None), ("tall", None), ("thin_even", None)]


@pytest.mark.parametrize("name,form", ROLLOUTS, ids=[f"{n}-{f or 'auto'}" for n, f in ROLLOUTS])
def test_a_scenario_against_the_reference_after_every_call(rcw, name, form):
    c = GC.SCENARIOS[name][1]
    env = GC.make_env(rcw, c, form)
    trackers = [] if name == "calls" else [GoalTracker(rcw, env), NeverLost(env)]   # (`calls` switches the generator off and sets walls by hand)
    events = GC.play(rcw, name, env, trackers)
    assert events["episode_starts"] > env.batch and events["restarts_after_done"] > 0 and events["restarts_after_truncation"] > 0
    if trackers:
        assert trackers[1].checked > 5
    if form is not None:
        assert env.step_form() == form
    if name == "f64":
        assert env.world.player_position_wu.dtype == np.float64
    if name == "big":
        assert env.world.tile_map_chunks.shape[1] * 2 > 64                    # more tile-map words than a wavefront has lanes
    if name == "huge":
        assert WG.grid(c["H"], c["W"])[2] == 1024
    if name in GC.AT_THE_BOUND:
        assert WG.grid(c["H"], c["W"])[2] == 4096 == WG.MAX_CELLS            # the bound itself, not 4095
        assert env.world.tile_map_chunks.shape[1] * 2 == GC.WORDS[name]       # (a chunk is two words)
    if name == "levels":
        layout, walls = env.wall_layout.numpy(), env.world.walls
        assert set(layout.tolist()) == {40, 41, 42} and min(np.bincount(layout - 40)) > 5
        for level in (40, 41, 42):                                            # every level held by several agents, one maze a level
            held = walls[layout == level]
            assert (held == held[0]).all()
            np.testing.assert_array_equal(held[0], rcw.layouts.generated_maze(rcw.layouts.generated_maze_key(0, 0, 0, 1, level, 9)[0], c["H"], c["W"]))
    else:
        assert (env.wall_layout.numpy() == -1).all()
    env.close()


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
    m = WR.episode_key(GC.HARD_LEVEL_SEED, level, 0)
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


FEATURES = ["goal_distance", "seen_map", "local_seen", "stack", "everything"]


@pytest.mark.parametrize("form", ["two-launches", "one-launch"])
@pytest.mark.parametrize("feature", FEATURES)
def test_the_features_follow_the_new_maze_in_one_pass(rcw, feature, form):
    """each feature beside the generator (and all of them at once): the camera view against the reference, the feature against its own
    reference fed with the engine's state, after every call of the `features` scenario"""
    env = GC.make_env(rcw, GC.CALLS, form)
    trackers = []
    if feature in ("goal_distance", "everything"):
        trackers += [GoalTracker(rcw, env), NeverLost(env)]
    if feature in ("seen_map", "local_seen", "everything"):
        trackers.append(SeenTracker(rcw, env))
    if feature in ("local_seen", "everything"):
        trackers.append(LocalTracker(rcw, env, 9, 2, LM.SEEN))
    if feature in ("stack", "everything"):
        trackers.append(StackTracker(env, 4, "gray", (21, 21)))
    events = GC.play(rcw, "features", env, trackers)
    assert events["restarts_after_done"] > 0 and events["restarts_after_truncation"] > 0 and events["goal_redraws"] > 0
    assert env.step_form() == form
    env.close()


def test_the_host_replay_equals_every_agents_walls(rcw):
    """layouts.generated_maze(generated_maze_key(...)) equals env.world.walls[a] for every agent — a shard with an agent_id_offset — after
    the install and after restarts, without levels and with them"""
    L = rcw.layouts
    c = dict(GC.LEVELS, B=21, H=9, W=11)
    for gen in (dict(loops=0.25), dict(loops=0.25, levels=5, first_level=3, level_seed=8)):
        env = GC.make_env(rcw, c, agent_id_offset=1000, max_episode_steps=3, wall_generator=gen)
        info = env.wall_generator_info
        assert info == dict(enabled=True, loops=1 << 30, levels=gen.get("levels", 0), first_level=gen.get("first_level", 0), level_seed=gen.get("level_seed", 0))
        rng = np.random.default_rng(4)
        first = env.world.episode.copy()
        for t in range(8):
            walls, episode, layout = env.world.walls, env.world.episode, env.wall_layout.numpy()
            for a in range(c["B"]):
                key, level = L.generated_maze_key(c["seed"], 1000 + a, int(episode[a]) - 1, info["levels"], info["first_level"], info["level_seed"])
                assert level == layout[a]
                np.testing.assert_array_equal(walls[a], L.generated_maze(key, c["H"], c["W"], 0.25), err_msg=f"agent {a}, step {t}")
                assert L.is_connected(walls[a])
            rcw.act_(env, WR.draw_actions(rng, c["B"]))
        assert (env.world.episode >= first + 2).all()                        # limit 3: everybody restarted at least twice
        env.close()


def test_view_only_and_the_top_view_beside_a_plain_generator_handle(rcw):
    """RCW_VIEW_ONLY (the step paints no camera view: the generator's kernel sits between the cast and the view kernel) and a handle with a
    top view, each stepped beside a plain handle with the same generator: the state equal after every call, the learner view the reference's
    of the plain handle's descriptors, the top view the reference worlds'"""
    c, pu = dict(GC.CALLS, B=6), 8
    plain = GC.make_env(rcw, c)
    only = GC.make_env(rcw, c)
    top = GC.make_env(rcw, c, render_top_view=True, pu_per_tu=pu)
    ref = GC.make_ref(c)
    only.set_learner_view("rgb", (16, 16), "chw", camera_view=False)
    for e in (plain, only, top):
        e.set_wall_generator(0.5)
        e.set_time_limit(4)
    ref.set_wall_generator(0.5)

    def compare(where):
        for k in ("episode", "goal_position", "player_position_wu", "player_direction_au", "done", "tile_map_chunks", "episode_steps", "truncated"):
            for e, who in ((only, "view only"), (top, "top view")):
                np.testing.assert_array_equal(getattr(e.world, k), getattr(plain.world, k), err_msg=f"{k} of the {who} handle, {where}")
        h, cc = plain.columns()
        np.testing.assert_array_equal(only.learner_view_host(), LV.from_descriptors(h, cc, plain.cfg, c["Hc"], "rgb", (16, 16)), err_msg=f"view {where}")
        np.testing.assert_array_equal(top.camera_view_host(), plain.camera_view_host(), err_msg=f"camera view {where}")

    lim = TL.TimeLimitRef(ref, 4, c["seed"], True)
    compare("behind set_wall_generator")
    np.testing.assert_array_equal(top.top_view_host(), ref.top_view(pu), err_msg="top view behind set_wall_generator")
    rng = np.random.default_rng(6)
    for t in range(14):
        a = WR.draw_actions(rng, c["B"])
        for e in (plain, only, top):
            rcw.act_(e, a)
        lim.step(a)
        compare(f"step {t}")
        np.testing.assert_array_equal(top.top_view_host(), ref.top_view(pu), err_msg=f"top view, step {t}")
    WG.assert_equal(plain, ref, "the plain handle behind the rollout")
    assert ref.events["episode_starts"] > c["B"] and lim.events["restarts_after_truncation"] > 0    # (the install is B of them)
    for e in (plain, only, top):
        e.close()


# ---- the call rules and hostile arguments ------------------------------------------------------------------------------------------------
def engine_state(env):
    w = env.world
    h, c = env.columns()
    s = dict(frame=env.camera_view_host(), col_h=h, col_c=c, tile_map=w.tile_map_chunks, goal=w.goal_position, position=w.player_position_wu,
             heading=w.player_direction_au, reward=w.reward, done=w.done, episode=w.episode, status=w.status, episode_steps=w.episode_steps,
             truncated=w.truncated)
    if env.wall_generator_info["enabled"] or env.wall_bank_info["layouts"]:
        s["wall_layout"] = env.wall_layout.numpy()
    return s


def unchanged(env, before, info, what):
    after = engine_state(env)
    assert set(after) == set(before), what
    for k in before:
        np.testing.assert_array_equal(after[k], before[k], err_msg=f"{k} behind {what}")
    assert (env.wall_generator_info, env.wall_bank_info) == info, what


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
        before, info = engine_state(env), (env.wall_generator_info, env.wall_bank_info)
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


@pytest.mark.parametrize("H,W,exc,message", [(4, 9, ValueError, "at least 5 x 5"), (9, 4, ValueError, "at least 5 x 5"),
                                             (131, 129, "unsupported", "at most 4096 cells")])
def test_a_map_the_generator_does_not_take(rcw, H, W, exc, message):
    """4 x 9 and 9 x 4: invalid; 131 x 129 (65 x 64 = 4160 cells): unsupported, the message names the bound; the handle stays as it was"""
    from raycastworlds_jl_amd import _capi

    assert WG.install_refusal(H, W, 0, 0) == ("invalid" if exc is ValueError else "unsupported")
    env = GC.make_env(rcw, dict(H=H, W=W, N=8, Hc=16, B=2, seed=1))
    before, info = engine_state(env), (env.wall_generator_info, env.wall_bank_info)
    with pytest.raises(ValueError if exc is ValueError else _capi.RcwError, match=message) as ei:
        env.set_wall_generator()
    if exc == "unsupported":
        assert ei.value.code == _capi.RCW_ERR_UNSUPPORTED and "129 x 129" in ei.value.message
    unchanged(env, before, info, message)
    rcw.act_(env, np.ones(2, np.uint8))                                      # ... and still steps
    env.close()


def test_calls_that_do_nothing_to_the_generator(rcw):
    """set_direction_table, set_time_limit, set_step_form, the feature switches and the getters: mazes, counters and levels stay"""
    c = GC.CALLS
    env = GC.make_env(rcw, c, wall_generator=dict(levels=3, first_level=1, level_seed=2))
    keep = lambda: (env.wall_layout.numpy().copy(), env.world.episode.copy(), env.world.tile_map_chunks.copy())
    before = keep()
    t = env.wall_layout.torch(sync=False)
    assert t.dtype.is_floating_point is False and tuple(t.shape) == (c["B"],)
    env.sync()
    np.testing.assert_array_equal(t.cpu().numpy(), before[0])
    for call in (lambda: env.set_direction_table(env.world.directions_wu[::-1].copy()), lambda: env.set_time_limit(7), lambda: env.set_step_form("one-launch"),
                 lambda: env.set_step_form("two-launches"), lambda: env.set_goal_distance(True), lambda: env.set_seen_map(True),
                 lambda: env.set_local_map(5), lambda: env.set_learner_view("gray", (8, 8)), lambda: env.clear_error(), lambda: rcw.cast_rays_(env),
                 lambda: rcw.update_camera_view_(env)):
        call()
        for got, want in zip(keep(), before):
            np.testing.assert_array_equal(got, want)
    rcw.reset_(env)
    assert (env.world.episode == before[1] + 1).all() and set(env.wall_layout.numpy().tolist()) <= {1, 2, 3}
    env.close()


# ---- the graph, the shards, the fuzzer ---------------------------------------------------------------------------------------------------
def test_a_captured_step_replayed_12_times_under_limit_3(rcw):
    torch = pytest.importorskip("torch")
    c = dict(GC.CALLS, B=12, H=7, W=9)
    gen = dict(loops=0.25, levels=0)
    env = GC.make_env(rcw, c, wall_generator=gen, max_episode_steps=3, goal_distance=True)
    ref = GC.make_ref(c)
    ref.set_wall_generator(**gen)
    lim = TL.TimeLimitRef(ref, 3, c["seed"], True)
    gd, lost = GoalTracker(rcw, env), NeverLost(env)
    stream = torch.cuda.Stream()
    env.sync()
    env.set_stream(stream.cuda_stream)
    a_host = np.ones(c["B"], np.uint8)                                       # forward: the same action in every replay
    with torch.cuda.stream(stream):
        actions = torch.from_numpy(a_host).cuda()
        stream.synchronize()
        ptr = env.wall_layout.ptr
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            rcw.act_(env, actions)                                           # (captured, not run)
        for k in range(12):
            g.replay()
            stream.synchronize()
            lim.step(a_host)
            WG.assert_equal(env, ref, f"replay {k}")
            np.testing.assert_array_equal(env.world.episode_steps, lim.episode_steps, err_msg=f"episode_steps, replay {k}")
            gd.stepped(a_host, f"replay {k}")
            lost.stepped(a_host, f"replay {k}")
        assert env.wall_layout.ptr == ptr
        stream.synchronize()
    assert len(ref.mazes_made) > 3 * c["B"] and lim.events["restarts_after_truncation"] >= 2 * c["B"]
    del g
    env.close()


def test_two_shards_equal_their_slices_of_the_whole_batch(rcw):
    G, WORLD = 16, 2
    kw = dict(seed=5, auto_reset=True, height_tile_map_tu=9, width_tile_map_tu=9, num_rays=33, height_camera_view_pu=24, num_directions=8,
              position_increment_wu=0.25, player_radius_wu=0.3)
    gen = dict(loops=0.25, levels=6, first_level=10, level_seed=4)
    whole = rcw.SingleRoomModule.SingleRoom(batch=G, wall_generator=gen, max_episode_steps=4, **kw)
    shards = [rcw.ShardedSingleRoom(G, rank=r, world=WORLD, device=0, **kw) for r in range(WORLD)]
    for sh in shards:
        sh.set_wall_generator(**gen)
        sh.env.set_time_limit(4)

    def compare(where):
        for sh in shards:
            sl = slice(sh.first, sh.first + sh.count)
            np.testing.assert_array_equal(sh.env.wall_layout.numpy(), whole.wall_layout.numpy()[sl], err_msg=f"wall_layout {where}")
            for k in ("episode", "goal_position", "player_position_wu", "player_direction_au", "done", "tile_map_chunks", "truncated"):
                np.testing.assert_array_equal(getattr(sh.env.world, k), getattr(whole.world, k)[sl], err_msg=f"{k} {where}")
            np.testing.assert_array_equal(sh.env.camera_view_host(), whole.camera_view_host()[sl], err_msg=f"camera view {where}")

    compare("installed")
    rng = np.random.default_rng(3)
    moved = whole.world.episode.copy()
    for k in range(12):
        a = WR.draw_actions(rng, G)
        rcw.act_(whole, a)
        for sh in shards:
            sh.act_(sh.local_slice(a))
        compare(f"step {k}")
    assert (whole.world.episode > moved).all() and len(set(whole.wall_layout.numpy().tolist())) > 1
    for e in [whole] + [sh.env for sh in shards]:
        e.set_wall_generator(0.0)                                            # no levels from here: a maze per (global agent, episode)
    for sh in shards:
        sh.reset_(seed=8)
    rcw.reset_(whole, seed=8)
    compare("behind other parameters and a reset")
    assert (whole.wall_layout.numpy() == -1).all()
    for sh in shards:
        sh.env.close()
    whole.close()


def test_random_generators_and_call_sequences_stay_in_parity():
    """tools/fuzz_parity.py gen: maps of 5 x 5 to 40 x 40, loops, levels, 30 random calls each, totals printed"""
    res = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tools", "fuzz_parity.py"), "16", "71", "gen"],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert "16 random configurations" in res.stdout and ", 0 mismatches" in res.stdout
    closing = res.stdout.strip().splitlines()[-1]
    print(closing)
    totals = {k: int(v) for v, k in re.findall(r"(\d+) ([a-z_0-9]+)\b", closing[closing.index("wall generator:"):closing.rindex(")")])}
    for k in ("step", "reset", "masked_reset", "set_state", "off_and_on", "episode_starts", "goal_redraws", "restarts_after_done",
              "restarts_after_truncation", "one_launch_steps", "two_launch_steps", "even_sizes", "with_levels", "with_loops", "cells_past_64"):
        assert totals[k] > 0, closing
