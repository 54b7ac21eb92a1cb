"""The state archive's GPU scenarios — test infrastructure, not a test: an engine with EVERY feature on, and the host copy of everything it
hands out per agent.  tests/test_gpu_snapshot.py and tests/test_gpu_snapshot_sharded.py play them.

The configuration is tests/episode_stats_cases.py's — 8 headings, a quarter tile a move, a player radius of 0.3, 64 rays, a camera view of 64
rows, forward-heavy actions, a wall bank with weights [1, 0, 3], a limit of 8 steps — with the goal distance, the seen map, a 5 x 5 local
map of the seen map, a k-frame learner view and the statistics on top.  Two shapes:

  ODD   5 x 5 map (a 50-byte field, a 25-byte seen map: byte copies with unaligned records), gray 7 x 9 with k = 3 (189 bytes, odd)
  WIDE  4 x 4 map (a 32-byte field: the 16-byte path), gray 8 x 8 with k = 4 (256 bytes: the 16-byte path)"""
import numpy as np

import walls_ref as WR

ODD = dict(H=5, W=5, view=(7, 9), k=3)
WIDE = dict(H=4, W=4, view=(8, 8), k=4)
LIMIT = 8
WEIGHTS = (1, 0, 3)


def bank_layouts(H, W):
    """the empty room, a pillar, and (5 x 5: tests/episode_stats_cases.py's) a wall across with a door / (4 x 4) another pillar"""
    w = np.zeros((3, H, W), bool)
    w[:, [0, -1], :] = True
    w[:, :, [0, -1]] = True
    w[1, 2, 2] = True
    if H >= 5:
        w[2, 2, 1:3] = True
    else:
        w[2, 1, 2] = True
    return w


def configure(env, c, form=None, local_source="seen", rows=None):
    """every feature on a fresh engine, in the order the archive wants them: the archive is bound last"""
    env.set_wall_bank(bank_layouts(c["H"], c["W"]), WEIGHTS)
    env.set_time_limit(LIMIT)
    env.set_goal_distance(True)
    env.set_seen_map(True)
    env.set_local_map(5, source=local_source)
    env.set_learner_view("gray", size=c["view"], stack=c["k"])
    env.set_episode_stats(True)
    if form is not None:
        env.set_step_form(form)
        assert env.step_form() == form
    if rows is not None:
        env.set_snapshots(rows)
    return env


def keywords(c, seed=5, T="Float32", auto_reset=True):
    return dict(seed=seed, T=T, auto_reset=auto_reset, num_directions=8, position_increment_wu=0.25, player_radius_wu=0.3,
                height_tile_map_tu=c["H"], width_tile_map_tu=c["W"], num_rays=64, height_camera_view_pu=64)


def make(rcw, B, c=ODD, form=None, rows=None, local_source="seen", **kw):
    env = rcw.SingleRoomModule.SingleRoom(batch=B, **keywords(c, **kw))
    return configure(env, c, form, local_source, rows)


PER_AGENT = ("position", "direction", "goal", "reward", "done", "episode", "episode_steps", "truncated", "tile_map", "camera_view",
             "goal_distance", "goal_start_distance", "goal_progress", "goal_distance_field", "seen_count", "seen_new", "goal_seen", "seen_map",
             "local_map", "learner_view", "wall_layout", "finished", "outcome", "length", "moves", "level", "spl_q16", "episodes")


def record(env):
    """every per-agent output of the engine and its camera frames, host copies, and the statistics' table"""
    w, s = env.world, env.episode_stats
    r = dict(position=w.player_position_wu, direction=w.player_direction_au, goal=w.goal_position, reward=w.reward, done=w.done,
             episode=w.episode, episode_steps=w.episode_steps, truncated=w.truncated, tile_map=w.tile_map_chunks,
             camera_view=env.camera_view_host(), goal_distance=np.asarray(env.goal_distance), goal_start_distance=np.asarray(env.goal_start_distance),
             goal_progress=np.asarray(env.goal_progress), goal_distance_field=env.goal_distance_field, seen_count=np.asarray(env.seen_count),
             seen_new=np.asarray(env.seen_new), goal_seen=np.asarray(env.goal_seen), seen_map=env.seen_map, local_map=env.local_map_host(),
             learner_view=env.learner_view_host(), wall_layout=np.asarray(env.wall_layout))
    r.update({name: np.asarray(getattr(s, name)) for name in ("finished", "outcome", "length", "moves", "level", "spl_q16", "episodes")})
    r = {k: np.array(v) for k, v in r.items()}
    assert set(r) == set(PER_AGENT) and all(v.shape[0] == env.batch for v in r.values())
    r["table"] = np.array(np.asarray(env.episode_stats_table(device=True)))
    return r


def assert_same(got, want, where, agents=None, source=None, table=False):
    """`got`'s agents `agents` (None: all) equal `want`'s agents `source` (None: the same ones), byte for byte, in every per-agent output"""
    for key in PER_AGENT:
        g = got[key] if agents is None else got[key][agents]
        w = want[key] if agents is None and source is None else want[key][agents if source is None else source]
        assert g.dtype == w.dtype and g.shape == w.shape, (where, key)
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero((g.reshape(g.shape[0], -1) != w.reshape(w.shape[0], -1)).any(axis=1))
            raise AssertionError(f"{where}: {key} differs for {bad.size} of {g.shape[0]} agents (first: {bad[:8]})")
    if table:
        np.testing.assert_array_equal(got["table"], want["table"], err_msg=f"{where}: table")


# The rewinds of tests/test_gpu_snapshot.py: B, shape, step form, T, rows, the engine's seed, the actions' seed — 11 steps, the save, a
# window of 14.  REHEARSED: what `rehearse` counts in each window on the CPU (tests/test_snapshot_spec.py runs it and holds it to this
# table; the GPU test holds the engine's own counts to the same table): restarts behind a goal, truncations, turn-only steps, restarts onto
# another layout.  The lone agent's seeds (2, 23) were searched on the CPU for a window that holds all of them.
T1, T2 = 11, 14
REWINDS = [(1, ODD, None, "Float32", 1, 2, 23), (63, ODD, "two-launches", "Float32", 63, 5, 63), (64, WIDE, "one-launch", "Float32", 67, 5, 64),
           (65, ODD, "one-launch", "Float64", 68, 5, 65), (257, WIDE, "two-launches", "Float64", 260, 5, 257), (257, ODD, "one-launch", "Float32", 257, 5, 257)]
REHEARSED = [(1, 1, 4, 1), (17, 65, 276, 33), (36, 73, 238, 43), (18, 65, 297, 29), (173, 256, 1002, 145), (78, 258, 1047, 111)]
EVENTS = ("goal_restarts", "truncations", "turn_only", "layout_changes")


def rehearse(B, c, T, acts, t1, seed=5):
    """the rewind's window on the CPU: tests/wall_bank_ref.py under tests/time_limit_ref.py (the composition tests/episode_stats_cases.py
    rehearses its bank with) plays `acts`; what the steps behind the first t1 held, counted as window_events counts them on an engine"""
    import time_limit_ref as TL
    import wall_bank_ref as WB

    ref = WB.WallBankRef(B, seed, c["H"], c["W"], 64, 64, T=np.float64 if T == "Float64" else np.float32, render=False)
    ref.set_wall_bank(bank_layouts(c["H"], c["W"]), WEIGHTS)
    lim = TL.TimeLimitRef(ref, LIMIT, seed, True)
    ev = dict(goal_restarts=0, truncations=0, turn_only=0, layout_changes=0)
    for k, a in enumerate(acts):
        before = dict(episode=ref.episode.copy(), done=ref.done.astype(bool).copy(), direction=ref.direction.copy(), position=ref.position.copy(),
                      layout=ref.wall_layout.copy())
        lim.step(a)
        if k < t1:
            continue
        same = ref.episode == before["episode"]
        ev["goal_restarts"] += int((before["done"] & ~same).sum())
        ev["truncations"] += int(((lim.truncated != 0) & same).sum())
        ev["turn_only"] += int((same & (ref.direction != before["direction"]) & (ref.position == before["position"]).all(axis=1)).sum())
        ev["layout_changes"] += int((~same & (ref.wall_layout != before["layout"])).sum())
    return ev


def actions(B, steps, seed):
    rng = np.random.default_rng(seed)
    return [WR.draw_actions(rng, B) for _ in range(steps)]


def play(rcw, env, acts, select=None):
    """step through `acts` (agent i takes acts[k][select[i]]), a record behind every call, the table as its change over the call"""
    out, before = [], record(env)["table"]
    for a in acts:
        rcw.act_(env, a if select is None else np.ascontiguousarray(a[select]))
        r = record(env)
        r["table"], before = r["table"] - before, r["table"]
        out.append(r)
    return out


def window_events(recs, start):
    """what a recorded window held, from the engine's own outputs: restarts behind a goal, truncations, turn-only steps"""
    ev = dict(goal_restarts=0, truncations=0, turn_only=0, layout_changes=0)
    prev = start
    for r in recs:
        same = r["episode"] == prev["episode"]
        ev["goal_restarts"] += int((prev["done"].astype(bool) & ~same).sum())
        ev["truncations"] += int((r["truncated"].astype(bool) & same).sum())
        ev["turn_only"] += int((same & (r["direction"] != prev["direction"]) & (r["position"] == prev["position"]).all(axis=1)).sum())
        ev["layout_changes"] += int((~same & (r["wall_layout"] != prev["wall_layout"])).sum())
        prev = r
    return ev
