"""Interior walls on the GPU (include/rcw.h, rcw_set_walls): every step of a rollout against tests/walls_ref.py — B `pyref.World`s with
their layouts written into tile_map[WALL], reset by the generator restated in Python — byte for byte: camera view, reward, done, goal,
position, heading, episode, tile-map chunks, column descriptors and status == 0.

Every rollout: 8 headings, a quarter tile a move, a player radius of 0.3 (with a quarter-tile move the default 1/8 reaches the reference's
BoundsError, CD:35; 0.3 cannot: an IndexError out of the reference means wrong inputs), auto_reset, forward-heavy actions from a seeded
generator.  The seeds and step counts were rehearsed on the CPU (WallsRef alone) so that each rollout sees all four kinds of event; the
counts of the reference's own bookkeeping, asserted below to be non-zero (and restarts_after_done >= 3 for the 6 x 6 rollout, which the
one-launch form needs: a disagreement between reset_preview and reset_agent shows as a wrong frame on the step after a restart):

    rollout   interior_wall_ray_hits   blocked_next_to_interior_wall   goal_redraws   restarts_after_done
    ROOMS      9546                     40                              6              7
    WIDE      35470                     53                              2              8
    F64       11866                     48                              3             10
    MAZE       6095                     27                              5              1
"""
import functools

import numpy as np
import pytest

import learner_view_ref as LV
import learner_view_stack_ref as LS
import walls_ref as WR
from helpers import assert_state_equal

pytestmark = pytest.mark.gpu

ALL = ("interior_wall_ray_hits", "blocked_next_to_interior_wall", "goal_redraws", "restarts_after_done")


def _layouts():
    import raycastworlds_jl_amd as RCW

    return RCW.layouts


def three_layouts(H, W):
    """ring only | a bar and a pillar | four rooms"""
    L = _layouts()
    bar = L.ring(H, W)
    if (H, W) == (6, 6):
        bar[2, 1:4] = True
        bar[4, 3] = True
    else:                                                                    # 5 x 7: two pillars in the middle row
        bar[2, 2] = True
        bar[2, 4] = True
    return np.stack([L.ring(H, W), bar, L.four_rooms(H, W)])


def mazes(H, W, n, seed):
    L = _layouts()
    return np.stack([L.maze(H, W, np.random.default_rng(seed + k)) for k in range(n)])


ROOMS = dict(H=6, W=6, N=64, Hc=64, B=16, steps=48, seed=7)          # a wavefront per agent in the one-launch form
WIDE = dict(H=5, W=7, N=320, Hc=64, B=16, steps=40, seed=4)          # a workgroup per agent; H = 5: the 2-bit fields run across the word boundaries
F64 = dict(H=6, W=6, N=96, Hc=40, B=16, steps=40, seed=5, T="Float64")   # 40 rows: the flat fill, two launches
MAZE = dict(H=32, W=32, N=64, Hc=64, B=8, steps=12, seed=154)        # 64 tile-map words an agent, marches that end on interior walls between the guard bands
CASES = dict(ROOMS=ROOMS, WIDE=WIDE, F64=F64, MAZE=MAZE)


def walls_of(name):
    c = CASES[name]
    if name == "MAZE":
        return mazes(c["H"], c["W"], c["B"], 100), None                      # B distinct layouts, layouts == B, a NULL index
    return three_layouts(c["H"], c["W"]), (np.arange(c["B"]) % 3).astype(np.int32)


def make_ref(c, **kw):
    return WR.WallsRef(c["B"], c["seed"], c["H"], c["W"], c["N"], c["Hc"], T=np.float64 if c.get("T") == "Float64" else np.float32, **kw)


def make_env(rcw, c, form=None, **kw):
    env = rcw.SingleRoomModule.SingleRoom(batch=c["B"], seed=c["seed"], T=c.get("T", "Float32"), auto_reset=True, num_directions=8,
                                          position_increment_wu=0.25, player_radius_wu=0.3, height_tile_map_tu=c["H"], width_tile_map_tu=c["W"],
                                          num_rays=c["N"], height_camera_view_pu=c["Hc"], **kw)
    if form is not None:
        env.set_step_form(form)
        assert env.step_form() == form
    return env


@functools.lru_cache(maxsize=None)
def rollout(name, render=True):
    """the reference's rollout, computed once and shared by the forms of the engine: (a snapshot behind set_walls and behind every step,
    the actions, the event counts)"""
    c = CASES[name]
    walls, index = walls_of(name)
    ref = make_ref(c, render=render)
    ref.set_walls(walls, index)
    rng = np.random.default_rng(c["seed"] + 1)
    snaps, actions = [ref.snapshot()], []
    for _ in range(c["steps"]):
        a = WR.draw_actions(rng, c["B"])
        ref.step(a)
        actions.append(a); snaps.append(ref.snapshot())
    return snaps, actions, dict(ref.events)


def covered(events, least_restarts=1):
    assert all(events[k] > 0 for k in ALL) and events["restarts_after_done"] >= least_restarts, events


ROLLOUTS = [("ROOMS", "two-launches"), ("ROOMS", "one-launch"), ("WIDE", "two-launches"), ("WIDE", "one-launch"), ("F64", None), ("MAZE", None)]


@pytest.mark.parametrize("name,form", ROLLOUTS, ids=[f"{n}-{f or 'auto'}" for n, f in ROLLOUTS])
def test_step_by_step_against_the_reference_worlds(rcw, name, form):
    c = CASES[name]
    snaps, actions, events = rollout(name)
    covered(events, 3 if name == "ROOMS" else 1)
    walls, index = walls_of(name)
    env = make_env(rcw, c, form)
    if name == "F64":
        assert env.step_form() == "two-launches" and env.fill_kernel_name() == "rcw_fill_flat_kernel"
    env.set_walls(walls, index)
    np.testing.assert_array_equal(env.world.walls, walls[index] if index is not None else walls)
    WR.assert_equal(env, snaps[0], f"{name}: behind set_walls")
    for t, a in enumerate(actions):
        rcw.act_(env, a)
        WR.assert_equal(env, snaps[t + 1], f"{name} ({form}): step {t}")
    if form is not None:
        assert env.step_form() == form
    env.close()


def top_forms(env):
    """the forms set_top_view_form accepts for the environment's shape"""
    from raycastworlds_jl_amd import _capi

    out = []
    for form in ("in-place", "one-kernel", "two-kernels"):
        try:
            env.set_top_view_form(form)
        except _capi.RcwError as e:
            assert e.code == _capi.RCW_ERR_UNSUPPORTED
            continue
        assert env.top_view_form() == form
        out.append(form)
    return out


@pytest.mark.parametrize("pu,Hc", [(8, 64), (32, 256)])
def test_the_top_view_draws_the_interior_walls_in_every_form(rcw, pu, Hc):
    c = dict(ROOMS, B=6, Hc=Hc)
    walls, index = three_layouts(6, 6), (np.arange(6) % 3).astype(np.int32)
    probe = make_env(rcw, c, render_top_view=True, pu_per_tu=pu)
    forms = top_forms(probe)
    probe.close()
    assert "one-kernel" in forms or "in-place" in forms
    ref = make_ref(c)
    ref.set_walls(walls, index)
    rng = np.random.default_rng(3)
    tops, actions = [ref.top_view(pu)], []
    for _ in range(6):
        actions.append(WR.draw_actions(rng, 6)); ref.step(actions[-1])
    tops.append(ref.top_view(pu))
    assert ref.events["interior_wall_ray_hits"] > 0
    for form in forms:
        env = make_env(rcw, c, render_top_view=True, pu_per_tu=pu)
        env.set_top_view_form(form)
        env.set_walls(walls, index)
        np.testing.assert_array_equal(env.top_view_host(), tops[0], err_msg=f"top view behind set_walls, {form}, {pu} px a tile")
        for a in actions:
            rcw.act_(env, a)
        np.testing.assert_array_equal(env.top_view_host(), tops[1], err_msg=f"top view behind 6 steps, {form}, {pu} px a tile")
        WR.assert_equal(env, ref, f"behind 6 steps, {form}")
        rcw.update_top_view_(env)                                            # (the stand-alone form)
        np.testing.assert_array_equal(env.top_view_host(), tops[1], err_msg=f"update_top_view_, {form}, {pu} px a tile")
        env.close()


def test_the_learner_view_and_its_stack_follow_the_walls(rcw):
    """gray 21 x 21, two frame slots, the bar-and-pillar layout for every agent: the view against tests/learner_view_ref.py fed with the
    reference's descriptors, the stack against tests/learner_view_stack_ref.py; a masked set_walls refills the touched agents' slots"""
    c = dict(ROOMS, steps=24)
    bar = three_layouts(6, 6)[1]
    env = make_env(rcw, c)
    ref = make_ref(c)
    env.set_learner_view("gray", (21, 21), "chw", stack=2)
    env.set_walls(bar); ref.set_walls(bar)
    view = lambda: LV.from_descriptors(ref.col_height, ref.col_colour, env.cfg, c["Hc"], "gray", (21, 21))
    model = LS.StackModel(2, view(), ref.episode)
    np.testing.assert_array_equal(env.learner_view_host(), model.stack, err_msg="the stack behind set_walls")
    rng = np.random.default_rng(c["seed"] + 1)
    for t in range(c["steps"]):
        a = WR.draw_actions(rng, c["B"])
        rcw.act_(env, a); ref.step(a)
        model.push(view(), ref.episode)
        np.testing.assert_array_equal(env.learner_view_host(), model.stack, err_msg=f"the stack behind step {t}")
        if t == 11:
            mask = np.zeros(c["B"], np.uint8); mask[::4] = 1
            rooms = _layouts().four_rooms(6, 6)
            env.set_walls(rooms, mask=mask); ref.set_walls(rooms, mask=mask)
            model.refill(view(), mask, ref.episode)
            got = env.learner_view_host()
            np.testing.assert_array_equal(got, model.stack, err_msg="the stack behind the masked set_walls")
            assert (got[mask != 0, 0] == got[mask != 0, 1]).all() and (got[mask == 0, 0] != got[mask == 0, 1]).any()
    WR.assert_equal(env, ref, "behind the rollout")
    assert ref.events["interior_wall_ray_hits"] > 0
    env.close()


def engine_state(env):
    w = env.world
    h, c = env.columns()
    return dict(frame=env.camera_view_host(), col_h=h, col_c=c, tile_map=w.tile_map_chunks, goal=w.goal_position, position=w.player_position_wu,
                heading=w.player_direction_au, reward=w.reward, done=w.done, episode=w.episode, status=w.status, episode_steps=w.episode_steps,
                truncated=w.truncated)


def test_a_masked_set_walls_in_the_one_launch_form(rcw):
    """after 5 steps, 5 of 16 agents get other walls: the others keep every byte (and their primed slots: the next steps are right for all 16)"""
    c = ROOMS
    walls, index = walls_of("ROOMS")
    env = make_env(rcw, c, "one-launch")
    ref = make_ref(c)
    env.set_walls(walls, index); ref.set_walls(walls, index)
    rng = np.random.default_rng(c["seed"] + 1)
    for t in range(5):
        a = WR.draw_actions(rng, c["B"])
        rcw.act_(env, a); ref.step(a)
    WR.assert_equal(env, ref, "behind 5 steps")
    mask = np.zeros(c["B"], np.uint8); mask[[1, 4, 6, 11, 15]] = 1
    other = ((index + 1) % 3).astype(np.int32)
    before = engine_state(env)
    env.set_walls(walls, other, mask); ref.set_walls(walls, other, mask)
    after = engine_state(env)
    keep = mask == 0
    for k in before:
        np.testing.assert_array_equal(after[k][keep], before[k][keep], err_msg=f"{k} of the untouched agents")
    assert (after["episode"][~keep] == before["episode"][~keep] + 1).all()
    WR.assert_equal(env, ref, "behind the masked set_walls")
    assert env.step_form() == "one-launch"
    for t in range(10):
        a = WR.draw_actions(rng, c["B"])
        rcw.act_(env, a); ref.step(a)
        WR.assert_equal(env, ref, f"step {t} behind the masked set_walls")
    env.close()


def test_the_ring_through_set_walls_is_one_more_reset(rcw, oracle):
    """set_walls(layouts.ring(H, W)) on a fresh 8 x 8 environment changes no bit of the map and resets every agent once more: the state, then
    and 20 steps on, is the unchanged C oracle's that was reset(seed) once more than a plain environment would be"""
    cfg = dict(height_tile_map_tu=8, width_tile_map_tu=8, num_rays=64, out_of_bounds=1)
    env = rcw.SingleRoomModule.SingleRoom(batch=32, seed=9, auto_reset=True, **cfg)
    orc = oracle.OracleBatch(32, seed=9, auto_reset=1, **cfg)
    assert_state_equal(env, orc, where="fresh")
    env.set_walls(_layouts().ring(8, 8)); orc.reset(seed=9)
    assert_state_equal(env, orc, where="behind set_walls(ring)")
    np.testing.assert_array_equal(env.world.episode, orc.episode)
    rng = np.random.default_rng(2)
    for t in range(20):
        a = WR.draw_actions(rng, 32)
        rcw.act_(env, a); orc.step(a)
    assert_state_equal(env, orc, where="20 steps behind set_walls(ring)")
    np.testing.assert_array_equal(env.world.episode, orc.episode)
    assert not env.world.status.any()
    env.close(); orc.close()


def test_a_masked_set_walls_zeroes_the_touched_agents_time_limit_words(rcw):
    c = ROOMS
    walls, index = walls_of("ROOMS")
    env = make_env(rcw, c)
    env.set_walls(walls, index)
    env.set_time_limit(4)
    rng = np.random.default_rng(1)
    for _ in range(4):
        rcw.act_(env, np.where(rng.random(c["B"]) < 0.5, 3, 4).astype(np.uint8))   # (turns: nobody reaches a goal, every agent is truncated)
    steps, truncated = env.world.episode_steps, env.world.truncated
    assert (steps == 4).all() and truncated.all()
    mask = np.zeros(c["B"], np.uint8); mask[::3] = 1
    env.set_walls(walls, index, mask)
    touched = mask != 0
    assert not env.world.episode_steps[touched].any() and not env.world.truncated[touched].any()
    np.testing.assert_array_equal(env.world.episode_steps[~touched], steps[~touched])
    np.testing.assert_array_equal(env.world.truncated[~touched], truncated[~touched])
    env.close()


def test_an_rng_environment_draws_its_reset_on_the_host_against_the_walls(rcw):
    """SingleRoom(rng=...): behind set_walls goal and pose are reference_reset_draws(..., walls=...) from a generator in the same state; the
    frames and the top view are the reference worlds' with those draws injected"""
    SR = rcw.SingleRoomModule
    c = dict(ROOMS, B=6)
    walls, index = three_layouts(6, 6), np.array([2, 1, 0, 1, 2, 1], np.int32)
    env = make_env(rcw, c, rng=np.random.default_rng(5), render_top_view=True, pu_per_tu=8)
    twin = np.random.default_rng(5)
    for _ in range(2 * c["B"]):                                              # the constructor's two resets an agent (SR:62-74, SR:105)
        SR.reference_reset_draws(twin, 6, 6, 8)
    env.set_walls(walls, index)
    draws = [SR.reference_reset_draws(twin, 6, 6, 8, walls=walls[index[b]]) for b in range(c["B"])]
    goal = np.array([d[:2] for d in draws], np.int32)
    pos = np.array([(d[2] - 0.5, d[3] - 0.5) for d in draws], np.float32)
    heading = np.array([d[4] for d in draws], np.int32)
    np.testing.assert_array_equal(env.world.goal_position, goal)
    np.testing.assert_array_equal(env.world.player_position_wu, pos)
    np.testing.assert_array_equal(env.world.player_direction_au, heading)
    assert not walls[index][np.arange(c["B"]), goal[:, 0] - 1, goal[:, 1] - 1].any()
    ref = make_ref(c)
    ref.set_walls(walls, index)
    ref.set_state(goal, pos, heading)
    want = ref.snapshot()
    np.testing.assert_array_equal(env.camera_view_host(), want["camera_view"])
    np.testing.assert_array_equal(env.world.tile_map_chunks, want["tile_map_chunks"])
    h, cc = env.columns()
    np.testing.assert_array_equal(h, want["col_height"]); np.testing.assert_array_equal(cc, want["col_colour"])
    np.testing.assert_array_equal(env.top_view_host(), ref.top_view(8))
    assert env.rng.bit_generator.state == twin.bit_generator.state           # (the same draws, no more)
    env.close()


def test_refusals_leave_the_environment_untouched(rcw):
    c = ROOMS
    walls, index = walls_of("ROOMS")
    env = make_env(rcw, c)
    env.set_walls(walls, index)
    rcw.act_(env, np.ones(c["B"], np.uint8))
    before = engine_state(env)
    open_ring = walls.copy(); open_ring[1, 0, 3] = False
    for bad, message in ((lambda: env.set_walls(open_ring, index), "ring tile"),
                         (lambda: env.set_walls(walls), "layout index"),          # 3 layouts, 16 agents, no index
                         (lambda: env.set_walls(walls, np.where(np.arange(c["B"]) == 7, 3, index)), "not in 0..2")):
        with pytest.raises(ValueError, match=message):
            bad()
        after = engine_state(env)
        for k in before:
            np.testing.assert_array_equal(after[k], before[k], err_msg=k)
    env.close()
