"""Walled worlds at the frame shapes the step was tuned for, against the C oracle with interior walls (tests/walled_oracle.py).

tests/test_gpu_walls.py and the wall sources' tests compare with references that render in Python, so their frames are small (64 rows or
fewer, 320 columns at the most, 67 agents).  Here the same byte-for-byte comparison — the full state and EVERY pixel after EVERY step —
runs where the kernels bench.py times do their work: 256 rows by the rule at 1024 agents (rcw_fill256_cast_kernel, `keep` on), the
window kernel at 128 and 512 rows, 64 rows at 100 and 1500 columns (more than kCastCols columns a lane), cfg-3's 16 x 16 map at 512
columns, the flat fill at 100, 37 and 65 rows, all of it again under a time limit of 3 (the _limit twins), the top view at 13, 20 and 32
pixels a tile in every form, and the four layout sources — the bank, mazes, caves, rooms — restarting agents on new maps behind the
one-launch step (rcw_wall_bank_paint_kernel past one trip of its row loop, ragged at 100 and 65 rows, and with 1 and 3 columns).

The reference is WalledOracle: oracle/rcw_oracle.c held to WallsRef by tests/test_oracle_walls.py, its layout-source rule held to the
Python Recorders by tests/test_walled_oracle_spec.py.  The rollouts are tests/test_gpu_unchanged_skip.py's Rollout — imported, given the
walled reference in the oracle's place — with the moves between steps that may make the observation buffer differ from what the primed
slots describe.  Every case counts, FROM THE REFERENCE ALONE, what it must have exercised and fails if it did not.

Rehearsed on the CPU (walled_rollout(None, ...): the reference alone), `unchanged / agent-steps` and the reference's events beside each
case below.
"""
import types

import numpy as np
import pytest

import deferred as D
import goal_distance_ref as GD
import time_limit_ref as TL
import wall_bank_cases as BC
import wall_bank_ref as WB
import wall_family as WF
import walled_oracle as WO
import walls_ref as WR
from helpers import CFG2, CFG3
from test_gpu_unchanged_skip import SENTINEL, SMALL, Rollout, _one_launch

pytestmark = pytest.mark.gpu


class Limited(WO.WalledOracle):
    """WalledOracle whose `step` goes through a TimeLimitRef once `limit(L)` was called: what Rollout.act steps"""
    lim = None

    def limit(self, L):
        self.lim = TL.TimeLimitRef(self, L, self.seed, True)

    def step(self, actions, moved=None):
        if self.lim is None:
            return super().step(actions, moved)
        self.lim.step(actions)
        return 0

    def cleared(self, mask=None, seed=None):
        """behind a reset / set_state / set_walls of the test's: the masked agents' two words"""
        if self.lim is not None:
            if seed is not None:
                self.lim.seed = int(seed)
            self.lim.clear(mask)


FAST = types.SimpleNamespace(OracleBatch=Limited)                              # what Rollout takes for the `oracle` module


def layouts_for(H, W, batch, seed=0):
    """(walls (8, H, W), index (batch)): four rooms, mazes and pillars in turn, a different layout for neighbouring agents"""
    import raycastworlds_jl_amd as RCW

    L, out = RCW.layouts, []
    for k in range(8):
        rng = np.random.default_rng(seed + k)
        w = (L.four_rooms(H, W), L.maze(H, W, rng), GD.pillars(H, W, 0.2, rng), GD.pillars(H, W, 0.35, rng))[k % 4]
        out.append(w if WB.valid_layout(w) else L.four_rooms(H, W))
    return np.stack(out), (np.arange(batch) % 8).astype(np.int32)


# ---- the moves between steps, on the engine (None: the reference alone) and the reference alike --------------------------------------------
def set_walls(r, walls, index=None, mask=None, where="set_walls"):
    if r.env is not None:
        r.env.set_walls(walls, index, mask)
    r.orc.set_walls(walls, index, mask)
    r.orc.cleared(mask)
    full_check(r, where)


def place(r, mask, at, where):
    """set_state onto free tiles, heading +i (0): `at` "wall": half a move short of touching the wall tile one row down — the forward move is
    refused, the frame stays —; "goal": the same distance from a free tile that gets the goal — the forward move ends the episode.  An
    agent whose map has no such pair of tiles keeps its state."""
    o = r.orc
    walls, goal, pos, heading = o.walls, o.goal.copy(), o.position.copy(), o.direction.copy()
    short = float(o.cfg.player_radius_wu_f64 + o.cfg.position_increment_wu_f64 / 2)
    mask = np.asarray(mask, np.uint8).copy()
    for b in np.flatnonzero(mask):
        free = ~walls[b]
        pairs = np.argwhere(free[:-1] & (walls[b][1:] if at == "wall" else free[1:]))      # 0-based (i, j): the tile, its neighbour one row down
        inner = pairs[pairs[:, 0] + 1 < o.H - 1] if at == "wall" else pairs                # (an interior wall where the map has one)
        pairs = inner if len(inner) else pairs
        if not len(pairs):
            mask[b] = 0
            continue
        i, j = pairs[(3 * b) % len(pairs)]
        others = [t for t in np.argwhere(free) if tuple(t) != (i, j)]
        goal[b] = (i + 2, j + 1) if at == "goal" else (others[-1][0] + 1, others[-1][1] + 1)
        pos[b], heading[b] = (i + 1 - short, j + 0.5), 0
    pos = pos.astype(r.real)
    if r.env is not None:
        r.env.set_state(goal, pos, heading, mask=mask)
    o.set_state(goal, pos, heading, mask=mask)
    o.cleared(mask)
    full_check(r, where)
    return mask


def reset(r, mask, seed, where):
    if r.env is not None:
        r.rcw.reset_(r.env, mask=mask, seed=seed)
    r.orc.reset(mask=mask, seed=seed)
    r.orc.cleared(mask, seed)
    full_check(r, where)


def full_check(r, where):
    """Rollout.check (state, descriptors, every pixel) plus what it leaves out: episode, status, the walls, the time limit's two words"""
    r.check(where)
    if r.env is None:
        return
    w, o = r.env.world, r.orc
    np.testing.assert_array_equal(w.episode, o.episode, err_msg=f"episode {where}")
    np.testing.assert_array_equal(w.status, o.status, err_msg=f"status {where}")
    if o.lim is not None:
        np.testing.assert_array_equal(w.episode_steps, o.lim.episode_steps, err_msg=f"episode_steps {where}")
        np.testing.assert_array_equal(w.truncated.astype(np.uint8), o.lim.truncated, err_msg=f"truncated {where}")


def steps(r, n, where, forward=None, p_forward=0.5):
    """n steps, each compared in full; forward: agents that are given action 1 whatever is drawn"""
    for s in range(n):
        a = r.rng.integers(1, 5, r.B).astype(np.uint8)
        a = np.where(r.rng.random(r.B) < p_forward, 1, a).astype(np.uint8)
        if forward is not None:
            a[np.asarray(forward) != 0] = 1
        before = r.orc.episode.copy()
        r.act(a, f"{where}, step {s}")
        full_check(r, f"{where}, step {s}")
        moved = r.orc.episode != before
        r.restart_steps += int(moved.any())
        r.partial_restart_steps += int(moved.any() and not moved.all())


def walled_rollout(rcw, kw, batch, form="one-launch", by_rule=False, one_in=None, limit=0, seed=21, rng_seed=5, buffers=True):
    """The rollout of every shape: per-agent layouts, random steps, agents put in front of walls and of goals, a masked and a full set_walls,
    a masked reset_ under a new seed, a sentinel buffer bound and taken away, a change of form there and back.  Returns
    (unchanged, agent-steps, the reference's events)."""
    kw = dict(kw, out_of_bounds=1, auto_reset=True)
    r = Rollout(rcw, FAST, batch, seed, rng_seed, **kw)
    r.restart_steps = r.partial_restart_steps = 0
    one = form == "one-launch"
    if one:
        _one_launch(r, by_rule)
    elif r.env is not None:
        r.env.set_step_form(form)
    H, W = r.orc.H, r.orc.W
    walls, index = layouts_for(H, W, batch)
    full_check(r, "fresh")
    set_walls(r, walls, index)
    if limit:
        if r.env is not None:
            r.env.set_time_limit(limit)
        r.orc.limit(limit)
    n = 2 if by_rule else 3                                                    # (steps a phase: the by-rule batch compares 268 MB a step)
    steps(r, n + 1, "first")
    third = (np.arange(batch) % 3 == 0).astype(np.uint8)
    at = place(r, third, "wall", "set_state in front of walls")
    steps(r, n, "in front of walls", forward=at)
    at = place(r, 1 - third, "goal", "set_state in front of goals")
    steps(r, n, "in front of goals", forward=at)                               # (done on the first, restarted by the second)
    half = (r.rng.random(batch) < 0.5).astype(np.uint8); half[0] = 1; half[-1] = 0
    set_walls(r, walls, ((index + 3) % 8).astype(np.int32), half, "the masked set_walls")
    steps(r, n, "after the masked set_walls")
    reset(r, 1 - half, 77, "the masked reset_ under a new seed")
    steps(r, n, "after the masked reset_")
    if r.env is not None and buffers and one:
        r.bind(r.new_buffer())
    steps(r, n, "a bound buffer that held a sentinel")
    at = place(r, third, "wall", "set_state in front of walls, the bound buffer")
    steps(r, 2, "in front of walls, the bound buffer", forward=at)
    if r.env is not None and buffers and one:
        r.bind(None)
    steps(r, 2, "the library's buffer again")
    if one:
        if r.env is not None:
            r.env.set_step_form("two-launches")
        steps(r, 2, "two launches")
        if r.env is not None:
            r.env.set_step_form(None if by_rule else "one-launch")
            assert r.env.step_form() == "one-launch"
    set_walls(r, walls[1:2], None, None, "one layout for everybody")
    at = place(r, third, "goal", "set_state in front of goals, one layout")
    steps(r, n + 1, "one layout for everybody", forward=at)
    events = dict(r.orc.events, restart_steps=r.restart_steps, partial_restart_steps=r.partial_restart_steps, **(r.orc.lim.events if limit else {}))
    if one:
        unchanged, agent_steps = r.finish(one_in)
    else:
        if r.env is not None:
            assert r.env.step_form() == form
            r.env.close()
        unchanged, agent_steps = r.unchanged, r.agent_steps
    assert events["interior_wall_ray_hits"] > 0 and events["blocked_next_to_interior_wall"] > 0 and events["goal_redraws"] > 0, events
    assert events["restarts_after_done"] > 0 and events["partial_restart_steps"] > 0, events
    if limit:
        assert events["truncations"] > 0 and events["restarts_after_truncation"] > 0, events
    print(f"{unchanged} of {agent_steps} agent-steps left the frame unchanged; {events}")
    return unchanged, agent_steps, events


# ---- (a) the flagship shape by the rule; (b), (c), (d) the other one-launch kernels on request; (f) all of them under a limit of 3 ----------
# name -> (the engine's keywords, batch, the form by the rule, one unchanged frame in how many agent-steps).  Beside each case, rehearsed on
# the reference alone (walled_rollout(None, ...)): unchanged / agent-steps; interior_wall_ray_hits, blocked_next_to_interior_wall,
# goal_redraws, restarts_after_done; steps on which some but not all agents restarted.  Under the limit of 3 (seed 22): the same, then
# truncations, restarts_after_truncation.
HC64 = dict(height_camera_view_pu=64, num_directions=64)
SHAPES = {
    # 9001 / 22528 (704 needed); 4014245, 3498, 2932, 1039; 11        limit, 36 agents: 254 / 1044; 169344, 67, 208, 36; 13; 228, 195
    "a: 8 x 8, 256 x 256, 1024 agents by the rule": (dict(**CFG2), 1024, True, 32),
    # 461 / 1044; 183392, 158, 140, 36; 2                             limit: 324 / 1044; 169344, 67, 208, 36; 13; 228, 195
    "b: 128 rows, 256 columns": (SMALL[1][1], SMALL[1][2], False, None),
    # 203 / 580; 117971, 96, 18, 20; 2                                limit: 77 / 580; 103026, 40, 80, 20; 13; 126, 109
    "b: 512 rows, 300 columns, a workgroup per agent": (SMALL[2][1], SMALL[2][2], False, None),
    # 599 / 1276; 82435, 189, 81, 44; 2                               limit: 357 / 1276; 74799, 84, 180, 44; 13; 278, 236
    "c: 64 rows, 100 columns": (dict(HC64, height_tile_map_tu=7, width_tile_map_tu=11, num_rays=100), SMALL[0][2], False, None),
    # 143 / 348; 355485, 48, 30, 12; 2                                limit: 123 / 348; 289573, 23, 62, 12; 13; 76, 62
    "c: 64 rows, 1500 columns: the reloaded slot-0 words": (dict(HC64, height_tile_map_tu=9, width_tile_map_tu=8, num_rays=1500), SMALL[5][2], False, None),
    # 303 / 696; 295868, 109, 43, 24; 2
    "d: cfg3, 16 x 16, 512 columns": (dict(**CFG3), SMALL[6][2], False, None),
    # 137 / 348; 148132, 50, 17, 12; 2
    "d: cfg3, Float64": (dict(T="Float64", **CFG3), 12, False, None),
}
# (e), two launches at 100 / 37 / 65 rows, 20 agents: 204, 255, 227 / 540; 35358, 83, 36, 20; 2
# the sources' scenario at 12 agents (source_recording): 28 or 29 restarts behind a step, 5 steps on which some but not all restart, 4 or 5 of
# them after done, 24 after truncation, 17 to 53 unchanged frames (112 to 125 at one column); at 1024 agents in the short form, bank / caves:
# 1383 / 1422 restarts behind a step, 7 / 7 partial steps, 1559 / 1499 unchanged frames, 1016 / 1001 restarts after truncation, 367 / 421 after done
LIMITED = [k for k in SHAPES if k[0] in "abc"]


@pytest.mark.parametrize("name", list(SHAPES))
def test_one_launch_on_walled_maps_matches_the_reference_after_every_step(rcw, name):
    pytest.importorskip("torch")
    kw, batch, by_rule, one_in = SHAPES[name]
    walled_rollout(rcw, kw, batch, by_rule=by_rule, one_in=one_in)


@pytest.mark.parametrize("name", LIMITED, ids=[k.replace("1024 agents by the rule", "36 agents on request") for k in LIMITED])
def test_the_limit_twins_on_walled_maps(rcw, name):
    """(f): the same rollouts under a time limit of 3 — rcw_fill256_cast_limit_kernel and the window kernel's _limit forms; the small batch
    for (a) too: the by-rule batch is the test above's"""
    pytest.importorskip("torch")
    kw, batch, by_rule, one_in = SHAPES[name]
    walled_rollout(rcw, kw, 36 if by_rule else batch, one_in=None, limit=3, seed=22, rng_seed=6)


# ---- (e) two launches: the flat and the frame fill ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hc", [100, 37, 65])
def test_two_launches_at_rows_no_window_takes(rcw, Hc):
    kw = dict(height_camera_view_pu=Hc, height_tile_map_tu=7, width_tile_map_tu=11, num_rays=100)
    env = rcw.SingleRoomModule.SingleRoom(batch=2, **kw)
    name = env.fill_kernel_name()
    env.close()
    assert "window" not in name and "256" not in name, name
    walled_rollout(rcw, kw, 20, form="two-launches", buffers=False)


# ---- the white box: which frames the one-launch step does not store, on a walled map ---------------------------------------------------------------
def test_the_skip_on_a_walled_map_is_taken_and_is_as_written(rcw):
    """tests/test_gpu_unchanged_skip.py's sentinel test with interior walls: behind a primed step the frames are overwritten with a
    sentinel through the torch alias and a step follows — every agent holds the reference's frame or the sentinel in every pixel, the
    sentinel only where the reference's frame is the same before and after the step, at least one agent in 32 does; with bind_obs called
    after the overwriting no sentinel survives"""
    torch = pytest.importorskip("torch")
    B = 96
    for tell in (False, True):
        r = Rollout(rcw, FAST, B, 11, 12, out_of_bounds=1, auto_reset=True, **CFG2)
        r.restart_steps = r.partial_restart_steps = 0
        _one_launch(r, False)
        walls, index = layouts_for(8, 8, B)
        set_walls(r, walls, index)
        at = place(r, (np.arange(B) % 4 == 0).astype(np.uint8), "wall", "in front of walls")
        steps(r, 2, "first", forward=at)
        alias = r.env.camera_view.torch().view(torch.int32)
        alias.fill_(SENTINEL - (1 << 32))
        torch.cuda.synchronize()
        if tell:
            r.env.bind_obs(None)
        before = r.orc.camera_view.copy()
        a = r.rng.integers(1, 5, B).astype(np.uint8); a[at != 0] = 1
        rcw.act_(r.env, a); assert r.orc.step(a) == 0
        got, want = r.env.camera_view_host(), r.orc.camera_view
        same = (want == before).reshape(B, -1).all(axis=1)
        right = (got == want).reshape(B, -1).all(axis=1)
        kept = (got == SENTINEL).reshape(B, -1).all(axis=1)
        print(f"bind_obs in between: {tell}; {int(same.sum())} agents unchanged in the reference, {int(kept.sum())} frames not stored")
        assert (right | kept).all(), "an agent holds neither the reference's frame nor the sentinel in every pixel"
        assert not (kept & ~same).any(), "a frame was left alone that the step changed"
        if tell:
            assert not kept.any() and right.all()
        else:
            assert int(kept.sum()) * 32 >= B and kept[at != 0].all(), f"{int(kept.sum())} of {B} frames skipped"
            rcw.update_camera_view_(r.env)
            np.testing.assert_array_equal(r.env.camera_view_host(), want)
        steps(r, 3, "further steps")
        assert r.orc.events["blocked_next_to_interior_wall"] > 0
        r.env.close()


# ---- the top view over walls at real pixel scales -----------------------------------------------------------------------------------------------
def top_forms(env):
    from raycastworlds_jl_amd import _capi

    out = []
    for form in ("in-place", "one-kernel", "two-kernels"):
        try:
            env.set_top_view_form(form)
        except _capi.RcwError as e:
            assert e.code == _capi.RCW_ERR_UNSUPPORTED
            continue
        out.append(form)
    return out


@pytest.mark.parametrize("pu", [13, 20, 32])
def test_the_top_view_over_walls_at_real_scales(rcw, pu):
    """8 x 8 at 13 and 20 pixels a tile (104 and 160 rows: the flat store) and at 32 (256 rows: the 256-row store), every form the
    geometry takes — the two-kernel form among them —, per-agent layouts, a masked set_walls in between; the top view and the whole
    state against the reference after every call"""
    B = 8
    kw = dict(out_of_bounds=1, auto_reset=True, render_top_view=True, pu_per_tu=pu, **CFG2)
    okw = dict(out_of_bounds=1, auto_reset=1, render_top_view=1, pu_per_tu=pu, **CFG2)
    make = lambda: rcw.SingleRoomModule.SingleRoom(batch=B, seed=5, **kw)
    probe = make(); forms = top_forms(probe); probe.close()
    assert "two-kernels" in forms and len(forms) >= 2, forms
    walls, index = layouts_for(8, 8, B, seed=3)
    mask = np.array([1, 0, 0, 1, 1, 0, 1, 0], np.uint8)
    for form in forms:
        env, orc = make(), Limited(B, seed=5, **okw)
        env.set_top_view_form(form)
        assert env.top_view_form() == form
        r = types.SimpleNamespace(env=env, orc=orc, rcw=rcw, B=B, real=np.float32, rng=np.random.default_rng(pu), check=None)

        def check(where, env=env, orc=orc):
            from helpers import assert_state_equal

            assert_state_equal(env, orc, where=where)
            np.testing.assert_array_equal(env.top_view_host(), orc.top_view, err_msg=f"top view {where}, {form}, {pu} px a tile")
        r.check = check
        set_walls(r, walls, index, None, "set_walls")
        for t in range(4):
            a = WR.draw_actions(r.rng, B)
            rcw.act_(env, a); assert orc.step(a) == 0
            full_check(r, f"step {t}")
        set_walls(r, walls, ((index + 1) % 8).astype(np.int32), mask, "the masked set_walls")
        place(r, mask, "goal", "in front of goals")
        for t in range(4):
            a = np.where(mask != 0, 1, WR.draw_actions(r.rng, B)).astype(np.uint8)
            rcw.act_(env, a); assert orc.step(a) == 0
            full_check(r, f"step {t} behind the masked set_walls")
        rcw.update_top_view_(env)
        check("update_top_view_")
        assert orc.events["interior_wall_ray_hits"] > 0 and orc.events["restarts_after_done"] > 0
        env.close(); orc.close()


# ---- the four layout sources at these shapes ----------------------------------------------------------------------------------------------------
SOURCES = ("bank", "generator", "caves", "rooms")
FAMILY_PARAMS = dict(generator=dict(loops=0.3, levels=3, first_level=5, level_seed=9), caves=dict(levels=3, first_level=2, level_seed=9),
                     rooms=dict(room=1, levels=3, first_level=4, level_seed=9))


def source_scenario(kind, short=False):
    """install; random steps; every third agent walks into its goal (a restart behind the next step, for some but not all); a time limit of 3
    from there: every agent is cut and restarted within four steps, not all of them on the same one"""
    def fn(d):
        if kind == "bank":
            d.set_wall_bank(layouts_for(8, 8, 1)[0], np.array([3, 1, 2, 0, 1, 1, 2, 1], np.uint32))
        else:
            getattr(d, WF.FAMILIES[kind].setter)(**FAMILY_PARAMS[kind])
        rng = np.random.default_rng(7)
        for _ in range(1 if short else 3):
            d.step(WR.draw_actions(rng, d.B))
        BC.walk_into_the_goal(d, (np.arange(d.B) % 3 == 0).astype(np.uint8))
        for _ in range(1 if short else 2):
            d.step(WR.draw_actions(rng, d.B))
        mask = (np.arange(d.B) % 2 == 0).astype(np.uint8)
        d.set_time_limit(3)
        d.step(WR.draw_actions(rng, d.B))
        d.reset(mask, seed=31)                                               # (the agents' episode clocks now differ by a step)
        for _ in range(4 if short else 8):
            d.step(np.where(rng.random(d.B) < 0.5, 3, WR.draw_actions(rng, d.B)).astype(np.uint8))
    return fn


class Noted:
    """a driver that passes every call on to a Recorder and keeps (method, args, kwargs), as deferred.Script does for the methods it knows"""

    def __init__(self, recorder):
        self.rec, self.B, self.calls = recorder, recorder.B, []

    def state(self):
        return self.rec.state()

    def __getattr__(self, method):
        def call(*args, **kwargs):
            self.calls.append((method, args, kwargs))
            getattr(self.rec, method)(*args, **kwargs)
        return call


def source_recording(kind, c, script=Noted):
    """(the script, the reference's snapshots, what they say happened)"""
    script = script(WO.FastRecorder(kind)(c))
    source_scenario(kind)(script)
    snaps, events = script.rec.snaps, dict(script.rec.events)
    some = part = same = 0
    for k, (method, _, _) in enumerate(script.calls):
        if method == "step":
            moved = snaps[k + 1]["episode"] != snaps[k]["episode"]
            some += int(moved.sum()); part += int(moved.any() and not moved.all())
            same += int((snaps[k + 1]["camera_view"] == snaps[k]["camera_view"]).reshape(c["B"], -1).all(axis=1).sum())
    events.update(restarts_behind_a_step=some, partial_restart_steps=part, unchanged=same, done_restarts=script.rec.ref.events["restarts_after_done"])
    return script, snaps, events


class Lockstep:
    """a Recorder and a Player side by side, call by call, the Player reading the Recorder's list of snapshots — of which only the last two
    are kept: at 1024 agents a snapshot is 268 MB.  Counts, from the reference's snapshots, what source_recording counts."""

    def __init__(self, rec, make_player):
        self.rec, self.B = rec, rec.B
        self.player = make_player(rec.snaps)
        self.restarts = self.partial = self.unchanged = 0

    def state(self):
        return self.rec.state()

    def __getattr__(self, method):
        def call(*args, **kwargs):
            getattr(self.rec, method)(*args, **kwargs)
            before, after = self.rec.snaps[-2], self.rec.snaps[-1]
            if method == "step":
                moved = after["episode"] != before["episode"]
                self.restarts += int(moved.sum()); self.partial += int(moved.any() and not moved.all())
                self.unchanged += int((after["camera_view"] == before["camera_view"]).reshape(self.B, -1).all(axis=1).sum())
            self.rec.snaps[-2] = None
            getattr(self.player, method)(*args, **kwargs)
        return call


def source_case(c, form):
    return dict(dict(H=8, W=8, N=256, Hc=256, B=12, seed=3), **c), form


SOURCE_SHAPES = {
    "8 x 8, 256 x 256, one launch": source_case({}, "one-launch"),
    "128 rows": source_case(dict(Hc=128), "one-launch"),
    "512 rows": source_case(dict(Hc=512, N=300), "one-launch"),
    "100 rows, two launches": source_case(dict(Hc=100, N=100), "two-launches"),
    "65 rows, two launches": source_case(dict(Hc=65, N=100), "two-launches"),
    "1 column, 256 rows": source_case(dict(N=1), "one-launch"),
    "3 columns, 256 rows": source_case(dict(N=3), "one-launch"),
}


def play_source(rcw, kind, c, form, name):
    script, snaps, events = source_recording(kind, c)
    assert events["restarts_behind_a_step"] > 0 and events["partial_restart_steps"] > 0, events
    assert events["done_restarts"] > 0 and events["restarts_after_truncation"] > 0 and events["interior_wall_ray_hits"] > 0, events
    if form == "one-launch":
        assert events["unchanged"] > 0, events
    env = BC.make_env(rcw, c, form)
    player = (BC.Player if kind == "bank" else WF.drivers(kind)[1])(rcw, env, snaps, f"{kind}, {name}")
    source_scenario(kind)(player)
    player.finished()
    assert env.step_form() == form
    env.close()
    return events


@pytest.mark.parametrize("kind", SOURCES)
@pytest.mark.parametrize("name", list(SOURCE_SHAPES))
def test_a_layout_source_restarts_agents_on_new_maps(rcw, kind, name):
    c, form = SOURCE_SHAPES[name]
    print(play_source(rcw, kind, c, form, name))


@pytest.mark.parametrize("kind", ["bank", "caves"])
def test_a_layout_source_at_1024_agents_by_the_rule(rcw, kind):
    """the bank and one family once at the batch that takes the one-launch form by the rule (the scenario's short form, in lockstep)"""
    c = dict(H=8, W=8, N=256, Hc=256, B=1024, seed=3)
    env = BC.make_env(rcw, c)
    assert env.step_form() == "one-launch"                                    # (by the rule)
    Player = BC.Player if kind == "bank" else WF.drivers(kind)[1]
    d = Lockstep(WO.FastRecorder(kind)(c), lambda snaps: Player(rcw, env, snaps, f"{kind} at 1024 agents"))
    source_scenario(kind, short=True)(d)
    d.player.finished()
    events = d.rec.events
    assert d.restarts > 0 and d.partial > 0 and d.unchanged > 0 and events["restarts_after_truncation"] > 0 and d.rec.ref.events["restarts_after_done"] > 0, events
    assert env.step_form() == "one-launch"
    env.close()


@pytest.mark.parametrize("kind", ["bank", "generator"])
def test_a_layout_source_at_256_rows_with_nobody_reading_between(rcw, kind):
    """the 256-row case through tests/deferred.py's Deferred: every call queued, the outputs copied on the stream, one wait at the end"""
    pytest.importorskip("torch")
    c, form = SOURCE_SHAPES["8 x 8, 256 x 256, one launch"]
    script, snaps, events = source_recording(kind, c, D.Script)
    want = D.records_of_snapshots(snaps)
    last = snaps[-1]
    pos = last["position"]
    final = dict(status=last["status"], episode=last["episode"], goal=last["goal"], position_bits=pos.view(np.uint32), heading=last["direction"],
                 tile_map_chunks=last["tile_map_chunks"], col_height=last["col_height"], col_colour=last["col_colour"])
    D.run_unread(lambda: BC.make_env(rcw, c, form), rcw, script, want, final, (), "host", name=f"{kind} at 256 rows, unread")
