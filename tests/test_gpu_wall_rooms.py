"""The rooms on the GPU (include/rcw.h, rcw_set_wall_rooms): the scenarios of tests/wall_rooms_cases.py played on an engine against
tests/wall_rooms_ref.py — after EVERY call the whole state of walls_ref.assert_equal (status, episode, goal, pose, reward, done, tile-map
chunks, column descriptors, camera view), wall_layout, and the time limit's two words; and the bank tests' feature trackers beside them:
the goal distance's words and fields (which never read -1: every layout is connected) in every rollout, the seen map, the local map from
the seen map and the 4-frame stack in the `features` scenario.  tests/test_wall_rooms_spec.py rehearses every scenario on the CPU and
asserts from the reference's counts what it reaches.

WIDER THAN A WAVEFRONT AND AT THE SIZE BOUND: at 66 x 66 with room 1 the level of 0 .. 149 whose widest round cuts 166 chambers (a lane
takes three) and the one with the most rounds (25), installed through levels=1 on 33 agents and compared with both CPU makers; 1031
agents, more workgroups than the device holds at once, each against the host export; 130 x 130 and 5 x 4097, Q = 4096, without frames.

Every comparison is exact.  Every export is missing from the build before this feature: each test here fails there.
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
import wall_rooms_cases as RC
import wall_rooms_ref as RR
import walls_ref as WR
from test_gpu_wall_bank import GoalTracker, LocalTracker, SeenTracker, StackTracker
from test_gpu_wall_generator import NeverLost

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUARTER = RR.word(0.25)
DEFAULTS = dict(enabled=True, room=2, stop=QUARTER, doors=QUARTER)


def level_key(level):
    return WR.episode_key(RC.HARD_LEVEL_SEED, level, 0)


# ---- the rollouts -----------------------------------------------------------------------------------------------------------------
ROLLOUTS = [("tiny", "two-launches"), ("tiny", "one-launch"), ("square", None), ("square64", None), ("doors", None), ("wide", None), ("levels", None),
            ("calls", "two-launches"), ("calls", "one-launch")]


@pytest.mark.parametrize("name,form", ROLLOUTS, ids=[f"{n}-{f or 'auto'}" for n, f in ROLLOUTS])
def test_a_scenario_against_the_reference_after_every_call(rcw, name, form):
    c = RC.SCENARIOS[name][1]
    env = RC.make_env(rcw, c, form)
    trackers = [] if name == "calls" else [GoalTracker(rcw, env), NeverLost(env)]   # (`calls` switches the rooms off and sets walls by hand)
    events = RC.play(rcw, name, env, trackers)
    assert events["episode_starts"] > env.batch and events["restarts_after_done"] > 0 and events["restarts_after_truncation"] > 0
    assert events["rooms_made"] > events["episode_starts"]
    if trackers:
        assert trackers[1].checked > 5
    if form is not None:
        assert env.step_form() == form
    walls, layout = env.world.walls, env.wall_layout.numpy()
    if name == "square64":
        assert env.world.player_position_wu.dtype == np.float64
    if name == "tiny":
        assert (layout == -1).all() and ((~walls).sum(axis=(1, 2)) == 7).all() and len({w.tobytes() for w in walls}) == 4   # the four layouts
    elif name == "levels":
        assert set(layout.tolist()) == {43, 44, 45} and min(np.bincount(layout - 43)) > 5
        for level in (43, 44, 45):                                            # every level held by several agents, one layout a level
            held = walls[layout == level]
            assert (held == held[0]).all()
            want = rcw.layouts.generated_rooms(rcw.layouts.generated_maze_key(0, 0, 0, 1, level, 9)[0], c["H"], c["W"], 1)
            np.testing.assert_array_equal(held[0], want)
    elif name == "doors":
        assert (layout == -1).all() and events["second_doors"] > events["episode_starts"]
    else:
        assert (layout == -1).all()
    assert all(rcw.layouts.is_connected(w) for w in walls[:16])
    env.close()


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
    m = level_key(level)
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


# ---- the features -------------------------------------------------------------------------------------------------------------------------
FEATURES = ["goal_distance", "seen_map", "local_seen", "stack", "everything"]


@pytest.mark.parametrize("form", ["two-launches", "one-launch"])
@pytest.mark.parametrize("feature", FEATURES)
def test_the_features_follow_the_new_layout_in_one_pass(rcw, feature, form):
    """each feature beside the rooms (and all of them at once): the camera view against the reference, the feature against its own
    reference fed with the engine's state, after every call of the `features` scenario; the goal distance never reads -1"""
    env = RC.make_env(rcw, RC.CALLS, form)
    trackers = []
    if feature in ("goal_distance", "everything"):
        trackers += [GoalTracker(rcw, env), NeverLost(env)]
    if feature in ("seen_map", "local_seen", "everything"):
        trackers.append(SeenTracker(rcw, env))
    if feature in ("local_seen", "everything"):
        trackers.append(LocalTracker(rcw, env, 9, 2, LM.SEEN))
    if feature in ("stack", "everything"):
        trackers.append(StackTracker(env, 4, "gray", (21, 21)))
    events = RC.play(rcw, "features", env, trackers)
    assert events["restarts_after_done"] > 0 and events["restarts_after_truncation"] > 0 and events["goal_redraws"] > 0
    assert events["rooms_made"] > events["episode_starts"]
    assert env.step_form() == form
    env.close()


def test_the_host_replay_equals_every_agents_walls(rcw):
    """layouts.generated_rooms(generated_maze_key(...)) equals env.world.walls[a] for every agent — a shard with an agent_id_offset — after
    the install and after restarts, without levels and with them; the constructor's keyword and its defaults"""
    L = rcw.layouts
    c = dict(RC.LEVELS, B=21)
    for rooms in (dict(room=1, stop=0.1, doors=0.6), dict(levels=5, first_level=3, level_seed=8)):
        env = RC.make_env(rcw, c, agent_id_offset=1000, max_episode_steps=3, wall_rooms=rooms)
        room, stop, doors = rooms.get("room", 2), rooms.get("stop", 0.25), rooms.get("doors", 0.25)
        assert env.wall_rooms_info == dict(enabled=True, room=room, stop=RR.word(stop), doors=RR.word(doors))
        info = env.wall_generator_info
        assert info == dict(enabled=True, loops=0, levels=rooms.get("levels", 0), first_level=rooms.get("first_level", 0), level_seed=rooms.get("level_seed", 0))
        rng = np.random.default_rng(4)
        first = env.world.episode.copy()
        for t in range(8):
            walls, episode, layout = env.world.walls, env.world.episode, env.wall_layout.numpy()
            for a in range(c["B"]):
                key, level = L.generated_maze_key(c["seed"], 1000 + a, int(episode[a]) - 1, info["levels"], info["first_level"], info["level_seed"])
                assert level == layout[a]
                np.testing.assert_array_equal(walls[a], L.generated_rooms(key, c["H"], c["W"], room, stop, doors), err_msg=f"agent {a}, step {t}")
                assert L.is_connected(walls[a])
            rcw.act_(env, WR.draw_actions(rng, c["B"]))
        assert (env.world.episode >= first + 2).all()                        # limit 3: everybody restarted at least twice
        env.close()
    env = RC.make_env(rcw, dict(c, B=2), wall_rooms={})
    assert env.wall_rooms_info == DEFAULTS
    env.close()


def test_view_only_and_the_top_view_beside_a_plain_rooms_handle(rcw):
    """RCW_VIEW_ONLY (the step paints no camera view: the rooms' kernel sits between the cast and the view kernel) and a handle with a top
    view, each stepped beside a plain handle with the same rooms: the state equal after every call, the learner view the reference's of the
    plain handle's descriptors, the top view the reference worlds'"""
    c, pu = dict(RC.CALLS, B=6), 8
    plain = RC.make_env(rcw, c)
    only = RC.make_env(rcw, c)
    top = RC.make_env(rcw, c, render_top_view=True, pu_per_tu=pu)
    ref = RC.make_ref(c)
    only.set_learner_view("rgb", (16, 16), "chw", camera_view=False)
    for e in (plain, only, top):
        e.set_wall_rooms(room=1)
        e.set_time_limit(4)
    ref.set_wall_rooms(room=1)

    def compare(where):
        for k in ("episode", "goal_position", "player_position_wu", "player_direction_au", "done", "tile_map_chunks", "episode_steps", "truncated"):
            for e, who in ((only, "view only"), (top, "top view")):
                np.testing.assert_array_equal(getattr(e.world, k), getattr(plain.world, k), err_msg=f"{k} of the {who} handle, {where}")
        h, cc = plain.columns()
        np.testing.assert_array_equal(only.learner_view_host(), LV.from_descriptors(h, cc, plain.cfg, c["Hc"], "rgb", (16, 16)), err_msg=f"view {where}")
        np.testing.assert_array_equal(top.camera_view_host(), plain.camera_view_host(), err_msg=f"camera view {where}")

    lim = TL.TimeLimitRef(ref, 4, c["seed"], True)
    compare("behind set_wall_rooms")
    np.testing.assert_array_equal(top.top_view_host(), ref.top_view(pu), err_msg="top view behind set_wall_rooms")
    rng = np.random.default_rng(6)
    for t in range(14):
        a = WR.draw_actions(rng, c["B"])
        for e in (plain, only, top):
            rcw.act_(e, a)
        lim.step(a)
        compare(f"step {t}")
        np.testing.assert_array_equal(top.top_view_host(), ref.top_view(pu), err_msg=f"top view, step {t}")
    RR.assert_equal(plain, ref, "the plain handle behind the rollout")
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


def infos(env):
    return env.wall_rooms_info, env.wall_caves_info, env.wall_generator_info, env.wall_bank_info


def unchanged(env, before, info, what):
    after = engine_state(env)
    assert set(after) == set(before), what
    for k in before:
        np.testing.assert_array_equal(after[k], before[k], err_msg=f"{k} behind {what}")
    assert infos(env) == info, what


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


@pytest.mark.parametrize("H,W,exc,message", [(4, 9, ValueError, "at least 5 x 5"), (9, 4, ValueError, "at least 5 x 5"),
                                             (131, 131, "unsupported", "at most 4096"), (130, 131, "unsupported", "at most 4096")])
def test_a_map_the_rooms_do_not_take(rcw, H, W, exc, message):
    """4 x 9 and 9 x 4: invalid; 131 x 131 (Q = 4225) and 130 x 131 (4160): unsupported, the message names the bound; the handle stays as it was"""
    from raycastworlds_jl_amd import _capi

    assert RR.install_refusal(H, W, 2, 0, 0) == ("invalid" if exc is ValueError else "unsupported")
    env = RC.make_env(rcw, dict(H=H, W=W, N=8, Hc=16, B=2, seed=1))
    before, info = engine_state(env), infos(env)
    with pytest.raises(ValueError if exc is ValueError else _capi.RcwError, match=message) as ei:
        env.set_wall_rooms()
    if exc == "unsupported":
        assert ei.value.code == _capi.RCW_ERR_UNSUPPORTED and "130 x 130" in ei.value.message and str(RR.bound(H, W)) in ei.value.message
    unchanged(env, before, info, message)
    rcw.act_(env, np.ones(2, np.uint8))                                      # ... and still steps
    env.close()


def test_calls_that_do_nothing_to_the_rooms(rcw):
    """set_direction_table, set_time_limit, set_step_form, the feature switches and the getters: layouts, counters and levels stay"""
    c = RC.CALLS
    env = RC.make_env(rcw, c, wall_rooms=dict(room=1, levels=3, first_level=1, level_seed=2))
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
    c = dict(RC.CALLS, B=12)
    rooms = dict(room=1, stop=0.25, doors=0.5)
    env = RC.make_env(rcw, c, wall_rooms=rooms, max_episode_steps=3, goal_distance=True)
    ref = RC.make_ref(c)
    ref.set_wall_rooms(**rooms)
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
            RR.assert_equal(env, ref, f"replay {k}")
            np.testing.assert_array_equal(env.world.episode_steps, lim.episode_steps, err_msg=f"episode_steps, replay {k}")
            gd.stepped(a_host, f"replay {k}")
            lost.stepped(a_host, f"replay {k}")
        assert env.wall_layout.ptr == ptr
        stream.synchronize()
    assert len(ref.keys_made) > 3 * c["B"] and lim.events["restarts_after_truncation"] >= 2 * c["B"]
    assert ref.events["rooms_made"] > ref.events["episode_starts"]
    del g
    env.close()


def test_two_shards_equal_their_slices_of_the_whole_batch(rcw):
    G, WORLD = 16, 2
    kw = dict(seed=5, auto_reset=True, height_tile_map_tu=9, width_tile_map_tu=12, num_rays=33, height_camera_view_pu=24, num_directions=8,
              position_increment_wu=0.25, player_radius_wu=0.3)
    rooms = dict(room=1, stop=0.2, doors=0.5, levels=6, first_level=40, level_seed=9)
    whole = rcw.SingleRoomModule.SingleRoom(batch=G, wall_rooms=rooms, max_episode_steps=4, **kw)
    shards = [rcw.ShardedSingleRoom(G, rank=r, world=WORLD, device=0, **kw) for r in range(WORLD)]
    for sh in shards:
        sh.set_wall_rooms(**rooms)
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
        e.set_wall_rooms(2, 0.5, 0)                                          # no levels from here: rooms per (global agent, episode)
    for sh in shards:
        sh.reset_(seed=8)
    rcw.reset_(whole, seed=8)
    compare("behind other parameters and a reset")
    assert (whole.wall_layout.numpy() == -1).all()
    for sh in shards:
        sh.set_wall_rooms(None)
        assert not sh.env.wall_rooms_info["enabled"]
        sh.env.close()
    whole.close()


def test_random_rooms_and_call_sequences_stay_in_parity():
    """tools/fuzz_parity.py rooms: maps of 5 x 5 to 40 x 40, room sides, stop and door probabilities, levels, 30 random calls each (some walk agents into their goals), totals printed"""
    res = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tools", "fuzz_parity.py"), "16", "71", "rooms"],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert "16 random configurations" in res.stdout and ", 0 mismatches" in res.stdout
    closing = res.stdout.strip().splitlines()[-1]
    print(closing)
    totals = {k: int(v) for v, k in re.findall(r"(\d+) ([a-z_0-9]+)\b", closing[closing.index("wall rooms:"):closing.rindex(")")])}
    for k in ("step", "reset", "masked_reset", "set_state", "arrive", "off_and_on", "episode_starts", "rooms_made", "second_doors", "goal_redraws", "restarts_after_done",
              "restarts_after_truncation", "one_launch_steps", "two_launch_steps", "non_square", "with_levels", "stopped", "rooms_past_64"):
        assert totals[k] > 0, closing
