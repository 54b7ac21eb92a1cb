"""The start rule on the GPU (include/rcw.h, "the start rule"; csrc/rcw_start_distance.hip) against tests/start_distance_ref.py.

  parity      the four hand-made maps of tests/test_start_distance_spec.py at B = 67, 64 rays: set_walls, the rule on, time limit 5, reset_,
              24 random steps under auto_reset — after EVERY call the whole tests/walls_ref.py state (pose, goal, tile map, descriptors,
              camera view, counters, status), the limit's two words and `placed`, byte for byte; in both step forms in Float32, once in Float64.
  dynamic LDS 200 x 200, a ring of walls only, B = 3: more than 64 KiB of LDS and hundreds of levels.
  features    beside every other feature, in learner-view-only mode and with a top view, after every call: the whole state is StartRef's,
              every start is the rule's tile and lies in the band, and each feature's own reference (goal distance, guide, seen map,
              frontier, visit map, local map, episode statistics, learner view, frame stack, top view) holds its words, maps and frames.
  and         stream order without reads between (the pose copied on the stream), enabling moves nothing, refusals, the archive, a
              captured step.
"""
import functools

import numpy as np
import pytest

import start_distance_ref as SR
import time_limit_ref as TL
import walls_ref as WR

pytestmark = pytest.mark.gpu

B, STEPS, LIMIT = 67, 24, 5


def make_env(rcw, H, W, seed, batch=B, T="Float32", form=None, **kw):
    env = rcw.SingleRoomModule.SingleRoom(batch=batch, seed=seed, T=T, auto_reset=True, num_directions=8, position_increment_wu=0.25,
                                          player_radius_wu=0.3, height_tile_map_tu=H, width_tile_map_tu=W,
                                          num_rays=kw.pop("num_rays", 64), height_camera_view_pu=kw.pop("height_camera_view_pu", 64), **kw)
    if form is not None:
        env.set_step_form(form)
        assert env.step_form() == form
    return env


def snapshot(ref, lim):
    return dict(ref.snapshot(), episode_steps=lim.episode_steps.copy(), truncated=lim.truncated.copy(), placed=ref.placed.copy())


@functools.lru_cache(maxsize=None)
def rollout(name, T="Float32"):
    """the reference's rollout, computed once and shared by the forms: snapshots behind set_walls (rule on, nobody placed), behind reset_
    and behind every step; the actions; the outcome counts"""
    make_walls, band, seed = SR.MAPS[name]
    walls = make_walls()
    H, W = walls.shape
    ref = SR.StartRef(B, seed, H, W, 64, 64, T=np.float64 if T == "Float64" else np.float32)
    ref.set_walls(walls)
    ref.band = band
    lim = TL.TimeLimitRef(ref, LIMIT, seed, True)
    snaps, actions = [snapshot(ref, lim)], []
    ref.reset()
    lim.clear()
    snaps.append(snapshot(ref, lim))
    rng = np.random.default_rng(seed + 1)
    for _ in range(STEPS):
        a = rng.integers(1, 5, B).astype(np.uint8)
        lim.step(a)
        actions.append(a); snaps.append(snapshot(ref, lim))
    return snaps, actions, dict(ref.outcomes), dict(lim.events)


def assert_equal(env, snap, where):
    WR.assert_equal(env, snap, where)
    np.testing.assert_array_equal(env.world.episode_steps, snap["episode_steps"], err_msg=f"episode_steps {where}")
    np.testing.assert_array_equal(env.world.truncated.astype(np.uint8), snap["truncated"], err_msg=f"truncated {where}")
    np.testing.assert_array_equal(env.start_placed.numpy(), snap["placed"], err_msg=f"placed {where}")


PARITY = [(n, f, "Float32") for n in SR.MAPS for f in ("two-launches", "one-launch")] + [("FOUR_ROOMS", None, "Float64")]


@pytest.mark.parametrize("name,form,T", PARITY, ids=[f"{n}-{f or 'auto'}-{t}" for n, f, t in PARITY])
def test_every_call_of_a_rollout_equals_the_reference(rcw, name, form, T):
    snaps, actions, outcomes, events = rollout(name, T)
    assert events["restarts_after_truncation"] + events["restarts_after_done"] >= 2 * B, events
    make_walls, band, seed = SR.MAPS[name]
    walls = make_walls()
    env = make_env(rcw, *walls.shape, seed, T=T, form=form)
    env.set_walls(walls)
    env.set_start_distance(*band)
    assert env.start_distance_info == dict(enabled=True, lo=band[0], hi=band[1])
    env.set_time_limit(LIMIT)
    assert_equal(env, snaps[0], f"{name}: the rule switched on")
    rcw.reset_(env)
    assert_equal(env, snaps[1], f"{name}: reset_")
    for t, a in enumerate(actions):
        rcw.act_(env, a)
        assert_equal(env, snaps[t + 2], f"{name} ({form}, {T}): step {t}")
    if form is not None:
        assert env.step_form() == form
    env.close()


def test_the_parity_scenarios_reach_every_outcome():
    total = {}
    for name in SR.MAPS:
        for k, v in rollout(name)[2].items():
            total[k] = total.get(k, 0) + v
    assert all(total.get(k, 0) > 0 for k in (SR.IN_BAND, SR.CLAMPED, SR.KEPT)), total


def test_a_map_whose_flood_needs_more_than_64_kib_of_lds(rcw):
    H = W = 200
    seed, band = 21, (150, 260)
    walls = SR.ring(H, W)
    env = make_env(rcw, H, W, seed, batch=3, num_rays=8, height_camera_view_pu=8, start_distance=band)
    ref = SR.StartRef(3, seed, H, W, 8, 8, render=False)
    ref.band = band

    def compare(where):
        np.testing.assert_array_equal(env.world.goal_position, ref.goal, err_msg=where)
        np.testing.assert_array_equal(env.world.player_position_wu, ref.position, err_msg=where)
        np.testing.assert_array_equal(env.world.player_direction_au, ref.direction, err_msg=where)
        np.testing.assert_array_equal(env.world.episode, ref.episode, err_msg=where)
        np.testing.assert_array_equal(env.start_placed.numpy(), ref.placed, err_msg=where)
        assert (env.world.status == 0).all()

    rcw.reset_(env)
    ref.reset()
    compare("reset_")
    d = ref.distance()
    assert ((d >= band[0]) & (d <= band[1])).all() and (ref.placed == SR.IN_BAND).all()
    rcw.reset_(env, np.array([0, 1, 0], np.uint8))
    ref.reset(np.array([0, 1, 0], np.uint8))
    compare("a masked reset_")
    env.set_start_distance(390, 395)                                              # the farthest tile of a 198 x 198 room is at most 394 away
    rcw.reset_(env)
    ref.band = (390, 395)
    ref.reset()
    compare("a band at the far corner")
    assert set(ref.placed.tolist()) <= {SR.IN_BAND, SR.CLAMPED}
    rng = np.random.default_rng(2)
    for t in range(2):
        a = rng.integers(1, 5, 3).astype(np.uint8)
        rcw.act_(env, a)
        ref.step(a)
        compare(f"step {t}")
    env.close()


# ---- beside every feature ---------------------------------------------------------------------------------------------------------------
# One scenario — four_rooms(9, 9), 33 agents, band (3, 5), time limit 4: reset_, ten random steps — whose expected state is StartRef's
# (rendered: frames, descriptors, top view), computed once and shared.  After EVERY call the engine's whole state is held to that
# snapshot first; each feature's own reference (tests/*_ref.py) then holds the feature's words, maps and frames.  Those references read
# pose, goal, walls and counters from the engine — which the line before has just held to StartRef's placed state, so they are driven
# from it — and the frames' references (the learner view, the frame stack, the top view) take the snapshot's own descriptors and images.
# The layout sources give the walls themselves: there the start is held to the rule on the engine's walls and goal, and the goal
# distance's reference runs beside it.
N_BESIDE, BAND_BESIDE, SEED_BESIDE, LIMIT_BESIDE, STEPS_BESIDE = 33, (3, 5), 17, 4, 10


def _family(rcw):
    L = rcw.layouts
    return np.stack([L.four_rooms(9, 9), L.ring(9, 9), L.maze(9, 9, np.random.default_rng(4))])


FEATURES = {
    "goal+guide": lambda rcw: dict(guide=True),
    "seen+frontier": lambda rcw: dict(frontier=True),
    "visit_map": lambda rcw: dict(visit_map=dict(sectors=2)),
    "local_map": lambda rcw: dict(local_map=5),
    "episode_stats": lambda rcw: dict(episode_stats=True),
    "wall_bank": lambda rcw: dict(wall_bank=_family(rcw)),
    "mazes": lambda rcw: dict(wall_generator={}),
    "caves": lambda rcw: dict(wall_caves={}),
    "rooms": lambda rcw: dict(wall_rooms={}),
    "top_view": lambda rcw: dict(render_top_view=True, pu_per_tu=8),
    "frame_stack": lambda rcw: dict(),
    "view_only": lambda rcw: dict(),
}
SOURCES = ("wall_bank", "mazes", "caves", "rooms")

# (a handle with a top view, or one whose learner view is set with camera_view=False, takes the two-launch step only)
BESIDE = [(f, form) for f in FEATURES for form in ("two-launches", "one-launch") if form == "two-launches" or f not in ("top_view", "view_only")]


@functools.lru_cache(maxsize=None)
def beside_rollout():
    """StartRef's rollout of the scenario: snapshots (with the top view at 8 px a tile) behind the rule's enabling, reset_ and every step"""
    import raycastworlds_jl_amd as RCW

    walls = np.asarray(RCW.layouts.four_rooms(9, 9)) != 0
    ref = SR.StartRef(N_BESIDE, SEED_BESIDE, 9, 9, 64, 64)
    ref.set_walls(walls)
    ref.band = BAND_BESIDE
    lim = TL.TimeLimitRef(ref, LIMIT_BESIDE, SEED_BESIDE, True)
    shot = lambda: dict(snapshot(ref, lim), top_view=ref.top_view(8))
    snaps, actions = [shot()], []
    ref.reset()
    lim.clear()
    snaps.append(shot())
    rng = np.random.default_rng(8)
    for _ in range(STEPS_BESIDE):
        a = rng.integers(1, 5, N_BESIDE).astype(np.uint8)
        lim.step(a)
        actions.append(a); snaps.append(shot())
    return walls, snaps, actions, dict(ref.outcomes)


def assert_state(env, snap, where, camera):
    """assert_equal above; without the camera view where the handle does not paint it (RCW_VIEW_ONLY)"""
    if camera:
        return assert_equal(env, snap, where)
    w = env.world
    for name, got in (("status", w.status), ("episode", w.episode), ("goal", w.goal_position), ("position", w.player_position_wu),
                      ("direction", w.player_direction_au), ("reward", w.reward), ("done", w.done.astype(np.uint8)), ("tile_map_chunks", w.tile_map_chunks),
                      ("episode_steps", w.episode_steps), ("truncated", w.truncated.astype(np.uint8)), ("placed", env.start_placed.numpy())):
        np.testing.assert_array_equal(got, snap[name], err_msg=f"{name} {where}")
    h, c = env.columns()
    np.testing.assert_array_equal(h, snap["col_height"], err_msg=f"height_line_pu {where}")
    np.testing.assert_array_equal(c, snap["col_colour"], err_msg=f"colour id {where}")


class Trackers:
    """the existing per-feature references of every feature the handle has on, told of every call"""

    def __init__(self, rcw, env, feature):
        import episode_stats_ref as ES
        import frontier_ref as FR
        import goal_distance_ref as GD
        import guide_ref as GR
        import local_map_ref as LM
        import seen_map_ref as SM
        import visit_map_ref as VM

        self.env, self.ES = env, ES
        self.goal = GD.Tracked(rcw, env, enable=False)
        self.guide = GR.Tracked(env, enable=False) if feature == "goal+guide" else None
        self.seen = SM.Tracked(rcw, env, enable=False) if feature == "seen+frontier" else None
        self.frontier = FR.Tracked(env, enable=False) if feature == "seen+frontier" else None
        self.visits = VM.Tracked(env, enable=False) if feature == "visit_map" else None
        if self.visits:
            assert self.visits.sectors == 2
            self.visits.refilled(None, "the rule switched on")            # (the last call in front was set_walls: BEGIN for every agent)
        self.local = LM.Tracked(rcw, env, 5, enable=False) if feature == "local_map" else None
        self.stats = None
        if feature == "episode_stats":
            info = env.episode_stats_info
            self.stats = ES.EpisodeStatsRef(env.batch, info["rows"], info["first"], env.cfg.position_increment_wu)
            self.stats.begin(None, env.world.player_position_wu, env.world.episode)
            ES.assert_equal(env, self.stats, "the rule switched on")

    def reset(self, where):
        env = self.env
        self.goal.masked(None, where)
        if self.guide: self.guide.check(where)
        if self.seen: self.seen.masked(None, where)
        if self.frontier: self.frontier.check(where)
        if self.visits: self.visits.refilled(None, where)
        if self.local: self.local.check(where)
        if self.stats:
            self.stats.begin(None, env.world.player_position_wu, env.world.episode)
            self.ES.assert_equal(env, self.stats, where)

    def stepped(self, actions, where):
        env, w = self.env, self.env.world
        self.goal.ref.stepped(*self.goal.state(walls_changed=True))
        self.goal.check(where)
        if self.guide: self.guide.check(where)
        if self.seen: self.seen.stepped(actions, where)
        if self.frontier: self.frontier.check(where, stepped=True)
        if self.visits: self.visits.stepped(where)
        if self.local: self.local.check(where)
        if self.stats:
            self.stats.step(w.player_position_wu, w.done, w.truncated, w.episode, None, self.goal.ref.start_distance)
            self.ES.assert_equal(env, self.stats, where)


@pytest.mark.parametrize("feature,form", BESIDE, ids=[f"{f}-{form}" for f, form in BESIDE])
def test_beside_every_feature_an_episode_starts_in_the_band(rcw, feature, form):
    import learner_view_ref as LV
    import learner_view_stack_ref as LS

    band, n = BAND_BESIDE, N_BESIDE
    walls4, snaps, actions, outcomes = beside_rollout()
    assert outcomes.get(SR.IN_BAND, 0) >= 3 * n, outcomes
    source = feature in SOURCES
    env = make_env(rcw, 9, 9, SEED_BESIDE, batch=n, max_episode_steps=LIMIT_BESIDE, goal_distance=True, **FEATURES[feature](rcw))
    if feature == "frame_stack":
        env.set_learner_view("gray", (16, 16), stack=4)
    if feature == "view_only":
        env.set_learner_view("gray", (16, 16), camera_view=False)
    else:
        env.set_step_form(form)
    if not source:
        env.set_walls(walls4)
    env.set_start_distance(*band)
    view = lambda s: LV.from_descriptors(s["col_height"], s["col_colour"], env.cfg, 64, "gray", (16, 16))
    stack = LS.StackModel(4, view(snaps[0]), snaps[0]["episode"]) if feature == "frame_stack" else None
    track = Trackers(rcw, env, feature)
    episode = env.world.episode
    began_total = 0

    def check(k, where):
        nonlocal episode, began_total
        now = env.world.episode
        began, episode = now != episode, now
        began_total += int(began.sum())
        if not source:                                                            # the whole state, frames included, is StartRef's
            assert_state(env, snaps[k], where, camera=feature != "view_only")
            if feature == "top_view":
                np.testing.assert_array_equal(env.top_view_host(), snaps[k]["top_view"], err_msg=f"top view {where}")
            if feature == "view_only":
                np.testing.assert_array_equal(env.learner_view_host(), view(snaps[k]), err_msg=f"learner view {where}")
            if stack is not None:
                if k > 0:
                    stack.push(view(snaps[k]), snaps[k]["episode"])
                np.testing.assert_array_equal(env.learner_view_host(), stack.stack, err_msg=f"the frame stack {where}")
        pos, goal, walls = env.world.player_position_wu, env.world.goal_position, env.world.walls
        placed, start = env.start_placed.numpy(), env.goal_start_distance.numpy()
        for b in map(int, np.flatnonzero(began)):                                 # the start is the rule's, on the walls and the goal the agent has
            F = SR.field(walls[b], goal[b])
            i, j = int(np.floor(pos[b, 0])), int(np.floor(pos[b, 1]))
            assert placed[b] in (SR.IN_BAND, SR.CLAMPED, SR.KEPT), (where, b, placed[b])
            assert start[b] == F[i, j] and tuple(pos[b]) == (i + 0.5, j + 0.5), (where, b)
            if placed[b] == SR.IN_BAND:
                assert band[0] <= start[b] <= band[1], (where, b, start[b])
            if placed[b] == SR.CLAMPED:
                assert start[b] == F.max() < band[0], (where, b, start[b])
            key = WR.episode_key(SEED_BESIDE, b, int(now[b]) - 1)
            assert SR.start_rule(walls[b], goal[b], key, *band) == ((i + 1, j + 1) if placed[b] != SR.KEPT else None, placed[b]), (where, b)
        assert (env.world.status == 0).all(), where

    check(0, f"{feature}: the rule switched on")
    rcw.reset_(env)
    check(1, f"{feature}: reset_")
    track.reset(f"{feature}: reset_")
    assert began_total == n
    for t, a in enumerate(actions):
        rcw.act_(env, a)
        check(t + 2, f"{feature} ({form}): step {t}")
        track.stepped(a, f"{feature} ({form}): step {t}")
    assert began_total >= 3 * n
    if feature == "visit_map":
        assert track.visits.seen["restarts"] >= 2 * n
    env.close()


# ---- the life cycle ---------------------------------------------------------------------------------------------------------------------
def state_bytes(env):
    w = env.world
    h, c = env.columns()
    return dict(pos=w.player_position_wu.tobytes(), dir=w.player_direction_au.tobytes(), goal=w.goal_position.tobytes(), reward=w.reward.tobytes(),
                done=w.done.tobytes(), episode=w.episode.tobytes(), steps=w.episode_steps.tobytes(), truncated=w.truncated.tobytes(),
                status=w.status.tobytes(), tile_map=w.tile_map_chunks.tobytes(), col_h=h.tobytes(), col_c=c.tobytes(), obs=env.camera_view_host().tobytes())


def test_enabling_moves_nothing_and_refusals_change_nothing(rcw):
    from raycastworlds_jl_amd import _capi

    walls = SR.two_rooms()
    env = make_env(rcw, 9, 12, 3, max_episode_steps=LIMIT)
    env.set_walls(walls)
    rng = np.random.default_rng(1)
    for _ in range(3):
        rcw.act_(env, rng.integers(1, 5, B).astype(np.uint8))
    assert env.start_distance_info == dict(enabled=False, lo=0, hi=0)
    for getter in (lambda: env.start_placed, lambda: env.start_placed.numpy()):
        with pytest.raises(_capi.RcwError) as ei:
            getter()
        assert ei.value.code == _capi.RCW_ERR_UNSUPPORTED
    out = np.zeros(B, np.uint8)
    assert env._lib.rcw_start_distance(env._h, out.ctypes.data) == _capi.RCW_ERR_UNSUPPORTED
    env.set_start_distance(None)                                                  # off where there was none: fine
    before = state_bytes(env)
    key = env.snapshot_info["shape_key"]
    for lo, hi in ((0, 3), (4, 3), (1, 65535), (-1, -1)):
        with pytest.raises(ValueError, match="band"):                             # (RCW_ERR_INVALID_ARGUMENT)
            env.set_start_distance(lo, hi)
        assert env.start_distance_info == dict(enabled=False, lo=0, hi=0) and state_bytes(env) == before
    env.set_start_distance(1)
    assert env.start_distance_info == dict(enabled=True, lo=1, hi=SR.MAX)
    assert state_bytes(env) == before, "switching the rule on moved something"
    assert (env.start_placed.numpy() == 0).all()
    assert env.snapshot_info["shape_key"] != key                                  # a shape key of its own
    placed = env.start_placed
    for lo, hi in ((0, 3), (7, 6), (1, 65535)):                                   # refused on a handle that has it: the band stays
        with pytest.raises(ValueError, match="band"):
            env.set_start_distance(lo, hi)
        assert env.start_distance_info == dict(enabled=True, lo=1, hi=SR.MAX) and state_bytes(env) == before
    env.set_start_distance(2, 9)                                                  # only the band changes: the array stays where it is
    assert env.start_placed.ptr == placed.ptr and state_bytes(env) == before
    env.set_start_distance(None)
    assert env.snapshot_info["shape_key"] == key and state_bytes(env) == before
    env.set_start_distance(1, None)                                               # off and on again: the next reset is under the rule
    rcw.reset_(env)
    assert (env.start_placed.numpy() == SR.IN_BAND).all()
    pos, goal = env.world.player_position_wu, env.world.goal_position
    for b in range(B):
        assert SR.field(walls, goal[b])[int(pos[b, 0]), int(pos[b, 1])] >= 1
    env.close()


def test_queued_bands_each_hold_for_the_reset_behind_them(rcw):
    """set(1, 2), reset_, a copy of the pose, set(6, 9), reset_, a copy, set(1, 1), reset_, a copy — all queued, nothing read between.
    The pose has no device pointer of its own: its stream-ordered copy is the state archive's device save (rows given as a device tensor:
    no host wait), whose record begins with the position; goal_start_distance is cloned beside it."""
    torch = pytest.importorskip("torch")
    walls = SR.corridor()
    env = make_env(rcw, 5, 70, 11, goal_distance=True)
    env.set_walls(walls)
    env.set_start_distance(1, 2)
    env.set_snapshots(3 * B)
    start = env.goal_start_distance
    bands = ((1, 2), (6, 9), (1, 1))
    with torch.cuda.stream(env.torch_stream()):
        rows = [torch.arange(k * B, (k + 1) * B, dtype=torch.int32, device=f"cuda:{env.device}") for k in range(3)]
        env.sync()
        syncs, copies = env.host_syncs, []
        for k, band in enumerate(bands):
            env.set_start_distance(*band)
            rcw.reset_(env)
            env.snapshot_save(rows[k])
            copies.append(start.torch(sync=False).clone())
        assert env.host_syncs == syncs, "a call between the resets waited for the stream"
        env.sync()
    records = env.snapshot_export()["rows"]
    assert env.snapshot_filled.all()
    for k, band in enumerate(bands):
        rec = records[k * B:(k + 1) * B]
        pos = np.ascontiguousarray(rec[:, 0:8]).view(np.float32)                 # the record's first segments: pos (2 x Float32), dir, goal (2 x Int32)
        goal = np.ascontiguousarray(rec[:, 12:20]).view(np.int32)
        got = copies[k].cpu().numpy()
        for b in range(B):
            i, j = int(pos[b, 0]), int(pos[b, 1])
            assert tuple(pos[b]) == (i + 0.5, j + 0.5), (k, b, pos[b])
            d = SR.field(walls, goal[b])[i, j]
            assert band[0] <= d <= band[1] and got[b] == d, (k, band, b, d, got[b])
    np.testing.assert_array_equal(env.world.player_position_wu, np.ascontiguousarray(records[2 * B:, 0:8]).view(np.float32))
    env.close()


def test_a_restore_into_a_running_episode_does_not_place_again(rcw):
    walls, band, seed = SR.four_rooms(), (3, 4), 9

    def fresh():
        env = make_env(rcw, 8, 8, seed, max_episode_steps=LIMIT, goal_distance=True)
        env.set_walls(walls)
        env.set_start_distance(*band)
        env.set_snapshots(B)
        rcw.reset_(env)
        return env

    rng = np.random.default_rng(5)
    acts = [rng.integers(1, 5, B).astype(np.uint8) for _ in range(16)]
    plain, env, other = fresh(), fresh(), fresh()
    trace = []
    for t, a in enumerate(acts):
        rcw.act_(plain, a)
        trace.append((state_bytes(plain), plain.start_placed.numpy().copy()))
    for a in acts[:3]:
        rcw.act_(env, a)
    env.snapshot_save()
    saved = state_bytes(env)
    for a in acts[3:9]:                                                           # past the limit: every agent restarts at least once
        rcw.act_(env, a)
    env.snapshot_restore()
    assert state_bytes(env) == saved == trace[2][0], "the restored agents were placed again"
    for t in range(3, 16):
        rcw.act_(env, acts[t])
        assert state_bytes(env) == trace[t][0] and (env.start_placed.numpy() == trace[t][1]).all(), f"step {t} behind the restore"
    # rows move between two handles of the same key
    assert other.snapshot_info["shape_key"] == env.snapshot_info["shape_key"]
    other.snapshot_import(env.snapshot_export())
    other.snapshot_restore()
    assert state_bytes(other) == saved
    for t in range(3, 8):
        rcw.act_(other, acts[t])
        assert state_bytes(other) == trace[t][0], f"step {t} on the other handle"
    for e in (plain, env, other):
        e.close()


def test_a_captured_step_replayed_equals_the_same_steps_uncaptured(rcw):
    torch = pytest.importorskip("torch")
    walls, band, seed = SR.four_rooms(), (3, 4), 9

    def fresh():
        env = make_env(rcw, 8, 8, seed, max_episode_steps=3, form="two-launches")
        env.set_walls(walls)
        env.set_start_distance(*band)
        rcw.reset_(env)
        return env

    plain, env = fresh(), fresh()
    a = np.random.default_rng(6).integers(1, 5, B).astype(np.uint8)
    for _ in range(2 + 8):
        rcw.act_(plain, a)
    stream = torch.cuda.Stream()
    env.sync()
    env.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        actions = torch.from_numpy(a).to(f"cuda:{env.device}")
        for _ in range(2):
            rcw.act_(env, actions)
        stream.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            rcw.act_(env, actions)
        for _ in range(8):
            g.replay()
        stream.synchronize()
    assert state_bytes(env) == state_bytes(plain)
    assert (env.start_placed.numpy() == plain.start_placed.numpy()).all() and (plain.world.episode >= 3).all()
    del g
    env.close()
    plain.close()


def test_an_environment_with_rng_takes_no_start_rule(rcw):
    env = rcw.SingleRoomModule.SingleRoom(batch=2, rng=np.random.default_rng(0), height_tile_map_tu=6, width_tile_map_tu=6, num_rays=8, height_camera_view_pu=8)
    with pytest.raises(ValueError, match="rng"):
        env.set_start_distance(1, 2)
    env.set_start_distance(None)
    env.close()


def test_the_example_widens_the_band_and_the_starts_follow():
    import importlib.util
    import os

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "start_curriculum.py")
    spec = importlib.util.spec_from_file_location("start_curriculum", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    means = mod.main(batch=256, steps=30, phases=4)
    assert len(means) == 4 and all(a < b for a, b in zip(means, means[1:])), means
    assert 1.0 <= means[0] <= 2.0, means
