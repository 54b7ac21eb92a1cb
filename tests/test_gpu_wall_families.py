"""What the wall generator's families share on the GPU (include/rcw.h, rcw_set_wall_generator / rcw_set_wall_caves / rcw_set_wall_rooms),
written once over tests/wall_family.py's table.  Six tests run here, a case a family.  Three bodies with many cases a family — the
rollouts, the features, the refused maps — are written here too and run in the family's own module, under its own parametrisation, where
their cases keep the ids they have had.  The scenarios of the family's cases module are played on an
engine against wall_family.WallFamilyRef — after EVERY call the whole state of walls_ref.assert_equal (status, episode, goal, pose, reward,
done, tile-map chunks, column descriptors, camera view), wall_layout, the infos of the other families and the time limit's two words — with
the bank tests' feature trackers beside them: the goal distance's words and fields (which never read -1: every layout is connected) in
every rollout, the seen map, the local map from the seen map and the 4-frame stack in the `features` scenario.  Then the host replay, a
view-only and a top-view handle beside a plain one, the maps a family does not take, the calls that leave it alone, a captured step, two
shards against the whole batch, and the fuzzer.

Each test's arguments — shapes, parameters, seeds, batch sizes — are the family's own, from its cases module (ROLLOUTS, REPLAYED, CAPTURED,
SHARDED, REFUSED_MAPS, ...), and so is what a scenario must have reached (`reached`, `check_rollout`).  What exists because of ONE family's kernel stays
in that family's module: tests/test_gpu_wall_generator.py, test_gpu_wall_caves.py, test_gpu_wall_rooms.py, where the refusals are too —
which sources refuse which differs by more than a name.  Every comparison is exact.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import learner_view_ref as LV
import local_map_ref as LM
import time_limit_ref as TL
import wall_family as WF
import walls_ref as WR
from test_gpu_wall_bank import GoalTracker, LocalTracker, SeenTracker, StackTracker

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = list(WF.FAMILIES)
per_family = pytest.mark.parametrize("family", FAMILIES)


def never_lost(env):
    """the generator module's NeverLost (imported late: the three family modules import this one for the bodies below)"""
    from test_gpu_wall_generator import NeverLost

    return NeverLost(env)


def own_parameters(f, params):
    """the family's own parameters of a setter's keywords, defaults filled in, as the caller gave them"""
    return WF.arguments(f, (), params)[:len(f.params)]


def expected_infos(f, params):
    """{info property: what it reads} behind an install with the keywords `params`"""
    *own, levels, first_level, level_seed = WF.arguments(f, (), params)
    words = dict(zip((p[0] for p in f.params), WF.parameters(f, own)))
    out = {f.info: dict(enabled=True, **words)}
    out.setdefault("wall_generator_info", {}).update(enabled=True, loops=words.get("loops", 0), levels=levels, first_level=first_level, level_seed=level_seed)
    return out


# ---- three bodies whose cases keep their ids in the family's own module: written here, called there under the family's parametrisation ----
def rollout_ids(rollouts):
    return [f"{n}-{f or 'auto'}" for n, f in rollouts]


def a_scenario_against_the_reference_after_every_call(rcw, family, name, form):
    """a case of the family's ROLLOUTS"""
    cases = WF.cases_of(family)
    c = cases.SCENARIOS[name][1]
    env = WF.make_env(rcw, c, form)
    trackers = [] if name == "calls" else [GoalTracker(rcw, env), never_lost(env)]   # (`calls` switches the family off and sets walls by hand)
    events = WF.play(family, rcw, name, env, trackers)
    assert events["episode_starts"] > env.batch and events["restarts_after_done"] > 0 and events["restarts_after_truncation"] > 0
    cases.reached(events, name)
    if trackers:
        assert trackers[1].checked > 5
    if form is not None:
        assert env.step_form() == form
    cases.check_rollout(rcw, env, name)
    assert all(rcw.layouts.is_connected(w) for w in env.world.walls[:16])
    env.close()


FEATURES = ["goal_distance", "seen_map", "local_seen", "stack", "everything"]


FORMS = ["two-launches", "one-launch"]


def the_features_follow_the_new_layout_in_one_pass(rcw, family, feature, form):
    """each feature beside the family (and all of them at once): the camera view against the reference, the feature against its own
    reference fed with the engine's state, after every call of the `features` scenario; the goal distance never reads -1"""
    cases = WF.cases_of(family)
    env = WF.make_env(rcw, cases.CALLS, form)
    trackers = []
    if feature in ("goal_distance", "everything"):
        trackers += [GoalTracker(rcw, env), never_lost(env)]
    if feature in ("seen_map", "local_seen", "everything"):
        trackers.append(SeenTracker(rcw, env))
    if feature in ("local_seen", "everything"):
        trackers.append(LocalTracker(rcw, env, 9, 2, LM.SEEN))
    if feature in ("stack", "everything"):
        trackers.append(StackTracker(env, 4, "gray", (21, 21)))
    events = WF.play(family, rcw, "features", env, trackers)
    assert events["restarts_after_done"] > 0 and events["restarts_after_truncation"] > 0 and events["goal_redraws"] > 0
    cases.reached(events, "features")
    assert env.step_form() == form
    env.close()


def a_map_the_family_does_not_take(rcw, family, H, W, exc, message):
    """a case of the family's REFUSED_MAPS — too small: invalid; past the family's bound: unsupported, the message names the bound (NAMED);
    the handle stays as it was"""
    from raycastworlds_jl_amd import _capi

    f, cases = WF.FAMILIES[family], WF.cases_of(family)
    assert f.install_refusal(H, W, WF.parameters(f, own_parameters(f, {})), 0, 0) == ("invalid" if exc is ValueError else "unsupported")
    env = WF.make_env(rcw, dict(H=H, W=W, N=8, Hc=16, B=2, seed=1))
    before, info = WF.engine_state(env), WF.infos(env)
    with pytest.raises(ValueError if exc is ValueError else _capi.RcwError, match=message) as ei:
        getattr(env, f.setter)()
    if exc == "unsupported":
        assert ei.value.code == _capi.RCW_ERR_UNSUPPORTED and all(n in ei.value.message for n in cases.NAMED[(H, W)])
    WF.unchanged(env, before, info, message)
    rcw.act_(env, np.ones(2, np.uint8))                                      # ... and still steps
    env.close()


# ---- the tests every family has, a case a family -------------------------------------------------------------------------------------------
@per_family
def test_the_host_replay_equals_every_agents_walls(rcw, family):
    """the family's export of `layouts` on generated_maze_key(...) equals env.world.walls[a] for every agent — a shard with an
    agent_id_offset — after the install and after restarts, without levels and with them; the constructor's keyword and its defaults"""
    L, f = rcw.layouts, WF.FAMILIES[family]
    replay, keyword = getattr(L, f.replay), f.setter[len("set_"):]
    c, installs = WF.cases_of(family).REPLAYED
    for params in installs:
        env = WF.make_env(rcw, c, agent_id_offset=1000, max_episode_steps=3, **{keyword: params})
        for info, reads in expected_infos(f, params).items():
            assert getattr(env, info) == reads, info
        own, info = own_parameters(f, params), env.wall_generator_info
        rng = np.random.default_rng(4)
        first = env.world.episode.copy()
        for t in range(8):
            walls, episode, layout = env.world.walls, env.world.episode, env.wall_layout.numpy()
            for a in range(c["B"]):
                key, level = L.generated_maze_key(c["seed"], 1000 + a, int(episode[a]) - 1, info["levels"], info["first_level"], info["level_seed"])
                assert level == layout[a]
                np.testing.assert_array_equal(walls[a], replay(key, c["H"], c["W"], *own), err_msg=f"agent {a}, step {t}")
                assert L.is_connected(walls[a])
            rcw.act_(env, WR.draw_actions(rng, c["B"]))
        assert (env.world.episode >= first + 2).all()                        # limit 3: everybody restarted at least twice
        env.close()
    env = WF.make_env(rcw, dict(c, B=2), **{keyword: {}})
    assert getattr(env, f.info) == expected_infos(f, {})[f.info]
    env.close()


@per_family
def test_view_only_and_the_top_view_beside_a_plain_handle(rcw, family):
    """RCW_VIEW_ONLY (the step paints no camera view: the family's kernel sits between the cast and the view kernel) and a handle with a top
    view, each stepped beside a plain handle with the same family: the state equal after every call, the learner view the reference's of the
    plain handle's descriptors, the top view the reference worlds'"""
    f, cases = WF.FAMILIES[family], WF.cases_of(family)
    c, pu, params = dict(cases.CALLS, B=6), 8, cases.BESIDE_A_PLAIN_HANDLE
    plain = WF.make_env(rcw, c)
    only = WF.make_env(rcw, c)
    top = WF.make_env(rcw, c, render_top_view=True, pu_per_tu=pu)
    ref = WF.make_ref(family, c)
    only.set_learner_view("rgb", (16, 16), "chw", camera_view=False)
    for e in (plain, only, top):
        getattr(e, f.setter)(**params)
        e.set_time_limit(4)
    ref.set_family(**params)

    def compare(where):
        for k in ("episode", "goal_position", "player_position_wu", "player_direction_au", "done", "tile_map_chunks", "episode_steps", "truncated"):
            for e, who in ((only, "view only"), (top, "top view")):
                np.testing.assert_array_equal(getattr(e.world, k), getattr(plain.world, k), err_msg=f"{k} of the {who} handle, {where}")
        h, cc = plain.columns()
        np.testing.assert_array_equal(only.learner_view_host(), LV.from_descriptors(h, cc, plain.cfg, c["Hc"], "rgb", (16, 16)), err_msg=f"view {where}")
        np.testing.assert_array_equal(top.camera_view_host(), plain.camera_view_host(), err_msg=f"camera view {where}")

    lim = TL.TimeLimitRef(ref, 4, c["seed"], True)
    compare(f"behind {f.setter}")
    np.testing.assert_array_equal(top.top_view_host(), ref.top_view(pu), err_msg=f"top view behind {f.setter}")
    rng = np.random.default_rng(6)
    for t in range(14):
        a = WR.draw_actions(rng, c["B"])
        for e in (plain, only, top):
            rcw.act_(e, a)
        lim.step(a)
        compare(f"step {t}")
        np.testing.assert_array_equal(top.top_view_host(), ref.top_view(pu), err_msg=f"top view, step {t}")
    WF.assert_equal(plain, ref, "the plain handle behind the rollout")
    assert ref.events["episode_starts"] > c["B"] and lim.events["restarts_after_truncation"] > 0    # (the install is B of them)
    cases.reached(ref.events)
    for e in (plain, only, top):
        e.close()


@per_family
def test_calls_that_do_nothing_to_the_family(rcw, family):
    """set_direction_table, set_time_limit, set_step_form, the feature switches and the getters: layouts, counters and levels stay"""
    f, cases = WF.FAMILIES[family], WF.cases_of(family)
    c = cases.CALLS
    env = WF.make_env(rcw, c, **{f.setter[len("set_"):]: cases.UNTOUCHED})
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
@per_family
def test_a_captured_step_replayed_12_times_under_limit_3(rcw, family):
    torch = pytest.importorskip("torch")
    f, cases = WF.FAMILIES[family], WF.cases_of(family)
    c, params = cases.CAPTURED
    env = WF.make_env(rcw, c, max_episode_steps=3, goal_distance=True, **{f.setter[len("set_"):]: params})
    ref = WF.make_ref(family, c)
    ref.set_family(**params)
    lim = TL.TimeLimitRef(ref, 3, c["seed"], True)
    gd, lost = GoalTracker(rcw, env), never_lost(env)
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
            WF.assert_equal(env, ref, f"replay {k}")
            np.testing.assert_array_equal(env.world.episode_steps, lim.episode_steps, err_msg=f"episode_steps, replay {k}")
            gd.stepped(a_host, f"replay {k}")
            lost.stepped(a_host, f"replay {k}")
        assert env.wall_layout.ptr == ptr
        stream.synchronize()
    assert len(ref.keys_made) > 3 * c["B"] and lim.events["restarts_after_truncation"] >= 2 * c["B"]
    cases.reached(ref.events)
    del g
    env.close()


@per_family
def test_two_shards_equal_their_slices_of_the_whole_batch(rcw, family):
    f = WF.FAMILIES[family]
    width, params, later = WF.cases_of(family).SHARDED
    G, WORLD = 16, 2
    kw = dict(seed=5, auto_reset=True, height_tile_map_tu=9, width_tile_map_tu=width, num_rays=33, height_camera_view_pu=24, num_directions=8,
              position_increment_wu=0.25, player_radius_wu=0.3)
    whole = rcw.SingleRoomModule.SingleRoom(batch=G, max_episode_steps=4, **{f.setter[len("set_"):]: params}, **kw)
    shards = [rcw.ShardedSingleRoom(G, rank=r, world=WORLD, device=0, **kw) for r in range(WORLD)]
    for sh in shards:
        getattr(sh, f.setter)(**params)
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
        getattr(e, f.setter)(*later)                                          # no levels from here: a layout per (global agent, episode)
    for sh in shards:
        sh.reset_(seed=8)
    rcw.reset_(whole, seed=8)
    compare("behind other parameters and a reset")
    assert (whole.wall_layout.numpy() == -1).all()
    for sh in shards:
        getattr(sh, f.setter)(None)
        assert not getattr(sh.env, f.info)["enabled"]
        sh.env.close()
    whole.close()


@per_family
def test_random_parameters_and_call_sequences_stay_in_parity(family):
    """tools/fuzz_parity.py gen | caves | rooms: maps of 5 x 5 to 40 x 40, the family's parameters, levels, 30 random calls each (some walk
    agents into their goals), totals printed"""
    mode, label, reached = WF.cases_of(family).FUZZ
    res = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tools", "fuzz_parity.py"), "16", "71", mode],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert "16 random configurations" in res.stdout and ", 0 mismatches" in res.stdout
    closing = res.stdout.strip().splitlines()[-1]
    print(closing)
    totals = {k: int(v) for v, k in re.findall(r"(\d+) ([a-z_0-9]+)\b", closing[closing.index(label):closing.rindex(")")])}
    for k in reached:
        assert totals[k] > 0, closing
