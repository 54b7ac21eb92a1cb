"""Episode statistics on the GPU (include/rcw.h, rcw_set_episode_stats): after EVERY call all seven per-agent words and the whole table
against tests/episode_stats_ref.py, and from the reference's own event counts the assertion that the run exercised what it claims.

The rollouts on the time-limit scenario feed the reference from the ORACLE (tests/test_gpu_time_limit.py's harness: engine, oracle and
tests/time_limit_ref.py side by side, the engine's state held to the oracle's behind every step).  Every other test feeds it the engine's
own state behind the call — position, done, truncated, episode counter, wall_layout, goal_start_distance — as the goal distance's and the
seen map's references are fed: state parity with the oracles is the existing suite's job.

The wall-bank scenario (tests/episode_stats_cases.py: three layouts on 5 x 5, weights [1, 0, 3], a limit of 8, goal distance first, 65
agents, 40 steps) was rehearsed on the CPU — tests/wall_bank_ref.py under tests/time_limit_ref.py, tests/test_episode_stats_spec.py runs the
rehearsal —: 288 closes, 65 in row 1, none in row 2, 223 in row 3; 46 successes and 242 truncations, every one with SPL defined; row 1 holds
11 successes and 54 truncations, row 3 holds 35 and 188.

Shapes: B in {1, 63, 64, 65, 257} — a lone lane, a wave tail on either side, a second workgroup with one lane —, 4 x 4 and 5 x 5 rooms, 64
rays, a camera view of 64 rows.  Every export is missing from the build before this feature: each test here fails there.
"""
import ctypes as C
import types

import numpy as np
import pytest

import deferred as D
import episode_stats_cases as EC
import episode_stats_ref as ES
import time_limit_ref as TL
import walls_ref as WR
from test_gpu_time_limit import A, Limited

pytestmark = pytest.mark.gpu
UNSUPPORTED = -7                                                             # RCW_ERR_UNSUPPORTED


# ---- the two harnesses ---------------------------------------------------------------------------------------------------------------
class Recorded(Limited):
    """the time-limit harness with the statistics on: the reference is fed from the oracle and the composed limit"""

    def __init__(self, rcw, oracle, **kw):
        super().__init__(rcw, oracle, **kw)
        self.env.set_episode_stats(True)
        assert self.env.episode_stats_enabled and self.env.episode_stats_info == dict(enabled=True, rows=0, first=0)
        self.stats = ES.EpisodeStatsRef(self.B, 0, 0, 0.25)
        self.stats.begin(None, self.orc.position, self.orc.episode)
        self.faulted = np.zeros(self.B, bool)                                  # an invalid action since the agent's record began
        self.closes_compared = 0

    def feed(self, a):
        before = self.stats.last_episode.copy()
        closing = self.stats.step(self.orc.position, self.orc.done, self.ref.truncated, self.orc.episode)
        self.faulted[self.orc.episode != before] = False
        self.faulted |= ~((a >= 1) & (a <= 4))
        # on a handle with a limit the length at the close is the episode's steps, for every agent that did not fault
        clean = closing & ~self.faulted
        np.testing.assert_array_equal(self.stats.length[clean], self.ref.episode_steps[clean])
        self.closes_compared += int(clean.sum())

    def check(self, where):
        super().check(where)
        ES.assert_equal(self.env, self.stats, where)

    def step(self, where, device=None, a=None, check=True):
        a = TL.draw_actions(self.rng, self.B, self.t, self.bad_every) if a is None else a
        super().step(where, device=device, a=a, check=False)
        self.feed(a)
        if check:
            self.check(where)


class Tracked:
    """an engine with the statistics on and the reference beside it, fed the engine's own state behind every call"""

    def __init__(self, env, inc=0.25):
        self.env = env
        info = env.episode_stats_info
        assert info["enabled"]
        self.ref = ES.EpisodeStatsRef(env.batch, info["rows"], info["first"], inc)
        self.ref.begin(None, env.world.player_position_wu, env.world.episode)
        self.check("enabled")

    def inputs(self):
        env, w = self.env, self.env.world
        drawn = env.wall_bank_info["layouts"] > 0 or env.wall_generator_info["enabled"]
        return dict(pos=w.player_position_wu, done=w.done, truncated=w.truncated, episode=w.episode,
                    layout=np.asarray(env.wall_layout) if drawn else None,
                    start_distance=np.asarray(env.goal_start_distance) if env.goal_distance_enabled else None)

    def check(self, where):
        ES.assert_equal(self.env, self.ref, where)

    def stepped(self, where):
        closing = self.ref.step(**self.inputs())
        self.check(where)
        return closing

    def masked(self, mask, where):
        self.ref.begin(mask, self.env.world.player_position_wu, self.env.world.episode)
        self.check(where)


def make(rcw, B, H=5, W=5, seed=5, T="Float32", auto_reset=True, limit=0, **kw):
    env = rcw.SingleRoomModule.SingleRoom(batch=B, seed=seed, T=T, auto_reset=auto_reset, num_directions=8, position_increment_wu=0.25,
                                          player_radius_wu=0.3, height_tile_map_tu=H, width_tile_map_tu=W, num_rays=64, height_camera_view_pu=64, **kw)
    if limit:
        env.set_time_limit(limit)
    return env


def run(rcw, env, t, steps, seed, name):
    rng = np.random.default_rng(seed)
    for k in range(steps):
        rcw.act_(env, WR.draw_actions(rng, env.batch))
        t.stepped(f"{name} step {k}")
    return t.ref.events


# ---- 1: rollouts on the time-limit scenario, the rule's inputs from the oracle -----------------------------------------------------------
@pytest.mark.parametrize("batch", [65, 257])
@pytest.mark.parametrize("T", ["Float32", "Float64"])
@pytest.mark.parametrize("form", ["two-launches", "one-launch"])
def test_rollouts_on_the_time_limit_scenario(rcw, oracle, form, T, batch):
    """4 x 4, 8 headings, quarter-tile moves, L = 4, 48 steps, every fifth step with invalid device actions, auto_reset (the scenario's
    docstring: 258 truncations and 27 terminations on the oracle alone at B = 64 over 24 steps)"""
    pytest.importorskip("torch")
    s = Recorded(rcw, oracle, form=form, batch=batch, T=T, **A)
    s.check("before the first step")
    s.run(f"{form} {T} B={batch}")
    ev = s.stats.events
    assert ev["successes"] > 0 and ev["truncations"] > 0 and ev["restarts_after_success"] > 0 and ev["restarts_after_truncation"] > 0, ev
    assert ev["frozen_calls"] > 0 and s.ref.events["invalid_while_truncated"] > 0, (ev, s.ref.events)   # a frozen record under an invalid action
    assert ev["successes"] == s.ref.events["terminations"] and ev["truncations"] == s.ref.events["truncations"]
    assert 0 < s.closes_compared < ev["successes"] + ev["truncations"]            # (the rest: agents an invalid action left unstepped)
    assert int(s.stats.table[0, 0]) == ev["successes"] + ev["truncations"] == int(s.stats.episodes.sum())
    assert s.env.step_form() == form
    s.close()


# ---- 2: without auto_reset -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 63, 64])
def test_without_auto_reset_a_record_closes_once(rcw, batch):
    """no limit, goal distance on: an agent that reaches the goal closes its record once — SPL below 1 where it wandered —, walks on with
    frozen words, and `finished` is 1 for exactly one call"""
    env = make(rcw, batch, H=4, W=4, seed=17, auto_reset=False)                # (rehearsed on the oracle: the lone agent arrives after 30 calls and 13 moves)
    env.set_goal_distance(True)
    env.set_episode_stats(True)
    t = Tracked(env)
    finished_calls = np.zeros(batch, int)
    rng = np.random.default_rng(2)
    for k in range(60):
        rcw.act_(env, WR.draw_actions(rng, batch))
        t.stepped(f"step {k}")
        finished_calls += t.ref.finished
    ev = t.ref.events
    assert ev["successes"] > 0 and ev["truncations"] == 0 and ev["frozen_calls"] > 0 and ev["spl_defined"] == ev["successes"], ev
    closed = t.ref.outcome != 0
    assert (finished_calls[closed] == 1).all() and (finished_calls[~closed] == 0).all() and (t.ref.episodes <= 1).all()
    q = t.ref.spl_q16[closed]
    assert ((q > 0) & (q < 65536)).any(), q                                  # a path longer than the tile distance: the division decides
    env.close()


# ---- 3: rows on a wall bank ----------------------------------------------------------------------------------------------------------
def bank_env(rcw, B=EC.BANK["B"], limit=EC.BANK["L"], **kw):
    env = make(rcw, B, seed=EC.BANK["seed"], **kw)
    env.set_wall_bank(EC.bank_layouts(), EC.BANK["weights"])
    env.set_time_limit(limit)
    env.set_goal_distance(True)
    env.set_episode_stats(True)
    return env


def test_rows_on_a_wall_bank(rcw):
    """the rehearsed scenario: the counts of the module docstring; row 2 (weight 0) stays zero, row 0 is the sum of the level rows, and
    `level` at a close is the layout of the episode that finished — the one the agent had BEFORE the call, not the next one's"""
    env = bank_env(rcw)
    assert env.episode_stats_info == dict(enabled=True, rows=3, first=0)
    t = Tracked(env)
    for k, a in enumerate(EC.bank_actions()):
        layout_before = np.asarray(env.wall_layout).copy()
        rcw.act_(env, a)
        closing = t.stepped(f"bank step {k}")
        level = np.asarray(env.episode_stats.level)
        np.testing.assert_array_equal(level[closing], layout_before[closing])
        table = np.asarray(env.episode_stats_table(device=True))
        assert not table[2].any() and (table[0] == table[1:].sum(axis=0)).all()
    ev = t.ref.events
    assert tuple(int(v) for v in ev["closes_per_row"]) == EC.BANK_REHEARSED["closes_per_row"]
    assert (ev["successes"], ev["truncations"], ev["spl_defined"]) == EC.BANK_REHEARSED["successes_truncations_spl"]
    tab = env.episode_stats_table()
    assert tab["first"] == 0 and tab["totals"]["episodes"] == 288 and tab["levels"]["episodes"].tolist() == [65, 0, 223]
    assert tab["levels"]["successes"].tolist() == [11, 0, 35] and tab["levels"]["truncations"].tolist() == [54, 0, 188]
    assert np.isnan(tab["spl"]["levels"][1]) and tab["spl"]["totals"] == tab["totals"]["sum_spl_q16"] / 65536 / 288
    env.close()


# ---- 4: rows on a generator ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels,first,rows", [(3, 7, 3), (300, 2, 300), (0, 0, 0), (65537, 5, 0)])
def test_rows_on_a_generator(rcw, levels, first, rows):
    """mazes on 5 x 5 under a limit of 6: a row per level from first_level; more rows than agents; no level range, or one past
    RCW_EPISODE_STATS_MAX_ROWS: no level rows, and row 0 still right"""
    env = make(rcw, 65, limit=6, wall_generator=dict(levels=levels, first_level=first, level_seed=3), episode_stats=True)
    assert env.episode_stats_info == dict(enabled=True, rows=rows, first=first if rows else 0)
    t = Tracked(env)
    ev = run(rcw, env, t, 20, 4, f"levels {levels}")
    closes = ev["successes"] + ev["truncations"]
    assert closes > 65 and int(t.ref.table[0, 0]) == closes
    if rows:
        assert ev["closes_outside_the_rows"] == 0 and int(t.ref.table[1:, 0].sum()) == closes and (t.ref.table[1:, 0] > 0).sum() >= min(rows, 3)
        assert t.ref.level[t.ref.outcome != 0].min() >= first
    else:
        assert ev["closes_outside_the_rows"] == closes and t.ref.table.shape == (1, 8)
        assert (t.ref.level[t.ref.outcome != 0] >= first).all() if levels else (t.ref.level == -1).all()
    env.close()


# ---- 5: every agent closes in one call into one row ----------------------------------------------------------------------------------
def test_all_agents_close_in_one_call_into_one_row(rcw):
    """B = 257, L = 1, a bank of one layout: every other call closes all 257 records — five wavefronts adding to the same two rows"""
    env = make(rcw, 257)
    env.set_wall_bank(EC.bank_layouts()[:1])
    env.set_time_limit(1)
    env.set_episode_stats(True)
    t = Tracked(env)
    closing_calls = 0
    for k in range(8):
        before = t.ref.table.copy()
        rcw.act_(env, np.full(257, 3, np.uint8))                             # a turn: nobody reaches a goal
        closing = t.stepped(f"step {k}")
        if closing.any():
            assert closing.all() and (t.ref.table[:, 0] - before[:, 0]).tolist() == [257, 257] and (t.ref.table[:, 2] - before[:, 2]).tolist() == [257, 257]
            closing_calls += 1
        else:
            assert (t.ref.table == before).all()
    assert closing_calls == 4 and np.asarray(env.episode_stats_table(device=True))[:, 0].tolist() == [4 * 257, 4 * 257]
    env.close()


# ---- 6: masked calls in the middle of episodes -----------------------------------------------------------------------------------------
def test_masked_reset_set_state_and_set_walls_in_the_middle_of_episodes(rcw):
    B = 65
    env = make(rcw, B, limit=12, episode_stats=True)                         # (4 + 3 + 3 steps: nobody is truncated before the last masked call)
    t = Tracked(env)
    run(rcw, env, t, 4, 11, "warm-up")
    keep = lambda: {w: getattr(t.ref, w).copy() for w in ES.WORDS if w != "finished"}
    for call, k in (("reset", 0), ("set_state", 1), ("set_walls", 2)):
        mask = np.zeros(B, np.uint8); mask[k::3] = 1
        open_before = int(((t.ref.outcome == 0) & (t.ref.length > 0) & (mask != 0)).sum())
        before, dropped, table, episodes = keep(), t.ref.events["dropped_by_mask"], t.ref.table.copy(), t.ref.episodes.copy()
        if call == "reset":
            rcw.reset_(env, mask=mask, seed=5)
        elif call == "set_state":
            goal = np.tile(np.array([[3, 3]], np.int32), (B, 1)); pos = np.full((B, 2), 1.5, np.float32); heading = np.arange(B, dtype=np.int32) % 8
            env.set_state(goal, pos, heading, mask=mask)
        else:
            env.set_walls(EC.bank_layouts()[1:2], mask=mask)
        t.masked(mask, f"after the masked {call}")
        assert open_before > 0 and t.ref.events["dropped_by_mask"] - dropped == open_before      # records abandoned in the middle: dropped
        assert (t.ref.table == table).all() and (t.ref.episodes == episodes).all() and not t.ref.finished.any()
        for w, v in before.items():
            np.testing.assert_array_equal(getattr(t.ref, w)[mask == 0], v[mask == 0], err_msg=w)
        assert (t.ref.length[mask != 0] == 0).all() and (t.ref.outcome[mask != 0] == 0).all()
        run(rcw, env, t, 3, 20 + k, f"behind {call}")
    env.close()


# ---- 7: clear, queued between steps that nobody reads between ------------------------------------------------------------------------------
def test_clear_queued_between_two_steps_without_a_read(rcw):
    """step, clear, step behind a backlog of queued device work, read once at the end (the style of tests/test_gpu_deferred.py): the table
    behind the second step holds that step's closes alone, the words are untouched by the clear, and no call waited for the stream.  Expected
    values: a twin played with a read behind every call.  L = 2, and a masked reset in the warm-up puts the two halves of the batch a step
    apart: one half closes behind the first step, the other behind the second."""
    torch = pytest.importorskip("torch")
    B = 65
    mask = np.zeros(B, np.uint8); mask[::2] = 1
    rng = np.random.default_rng(3)
    acts = [WR.draw_actions(rng, B) for _ in range(5)]

    def warm():
        env = make(rcw, B, limit=2)
        rcw.act_(env, acts[0])
        rcw.act_(env, acts[1])                                                # everybody is truncated
        rcw.reset_(env, mask=mask, seed=5)
        rcw.act_(env, acts[2])                                                # the others restart: a step behind the masked ones
        env.set_episode_stats(True)
        return env

    twin = warm()
    t = Tracked(twin)
    rcw.act_(twin, acts[3]); first = t.stepped("twin, first step").copy()
    want1 = (t.ref.table.copy(), {w: getattr(t.ref, w).copy() for w in ES.WORDS})
    twin.episode_stats_clear(); t.ref.clear(); t.check("twin, cleared")
    rcw.act_(twin, acts[4]); second = t.stepped("twin, second step").copy()
    want2 = (t.ref.table.copy(), {w: getattr(t.ref, w).copy() for w in ES.WORDS})
    assert first.any() and second.any() and want2[0][0, 0] == second.sum() and want1[0][0, 0] == first.sum()
    twin.close()

    env = warm()
    stream = env.torch_stream()
    try:
        with torch.cuda.stream(stream):
            dev = [torch.from_numpy(a).to(f"cuda:{env.device}") for a in acts[3:]]
            words = {w: getattr(env.episode_stats, w).torch(sync=False) for w in ES.WORDS}
            raw = env.episode_stats_table(device=True)
            table = rcw.SingleRoomModule.DeviceArray(raw.ptr, raw.shape, np.int64, env, env._sync).torch(sync=False)   # (the same bytes, a type every torch copies)
            stream.synchronize()
            syncs = env.host_syncs
            events = D.Deferred._backlog(types.SimpleNamespace(env=env, scale=1), torch)
            rcw.act_(env, dev[0])
            got1 = (table.clone(), {w: x.clone() for w, x in words.items()})
            env.episode_stats_clear()
            rcw.act_(env, dev[1])
            got2 = (table.clone(), {w: x.clone() for w, x in words.items()})
            pending = not events[1].query()
            assert env.host_syncs == syncs
            env.sync()
        for (gt, gw), (wt, ww), where in ((got1, want1, "behind the first step"), (got2, want2, "behind clear and the second step")):
            np.testing.assert_array_equal(gt.cpu().numpy().view(np.uint64), wt, err_msg=f"the table {where}")
            for w in ES.WORDS:
                np.testing.assert_array_equal(gw[w].cpu().numpy(), ww[w], err_msg=f"{w} {where}")
        assert pending, "a call waited for the stream: the backlog had ended before the last call was queued"
    finally:
        D.release_backlog()
        env.close()


# ---- 8: the source setters while the statistics are on ---------------------------------------------------------------------------------
def test_the_source_setters_are_refused_while_on(rcw):
    from raycastworlds_jl_amd import _capi

    env = bank_env(rcw, B=63)
    t = Tracked(env)
    run(rcw, env, t, 3, 1, "before")
    lib, h = env._lib, env._h
    walls = np.ascontiguousarray(EC.bank_layouts()[:1].transpose(0, 2, 1).astype(np.uint8))
    state = lambda: (env.world.episode.copy(), np.asarray(env.wall_layout).copy(), env.world.tile_map_chunks.copy(), env.wall_bank_info, env.wall_generator_info)
    before = state()
    calls = [lambda: lib.rcw_set_wall_bank(h, walls.ctypes.data_as(C.c_void_p), 1, None), lambda: lib.rcw_set_wall_bank(h, None, 0, None),
             lambda: lib.rcw_set_wall_generator(h, 1, 0, 0, 0, 0), lambda: lib.rcw_set_wall_generator(h, 0, 0, 0, 0, 0),
             lambda: lib.rcw_set_wall_caves(h, 1, 1 << 30, 2, 0, 0, 0), lambda: lib.rcw_set_wall_rooms(h, 1, 1, 0, 0, 0, 0, 0)]
    for k, call in enumerate(calls):
        assert call() == UNSUPPORTED, k
        assert "rcw_set_episode_stats" in _capi.last_error(lib)
        after = state()
        assert all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(before, after)), k
        t.check(f"behind refusal {k}")
    run(rcw, env, t, 2, 2, "behind the refusals")
    env.set_episode_stats(False)
    assert not env.episode_stats_enabled
    env.set_wall_bank(None)                                                  # ... and then they work
    env.set_wall_generator(levels=4, first_level=1)
    env.set_episode_stats(True)
    assert env.episode_stats_info == dict(enabled=True, rows=4, first=1)
    t = Tracked(env)
    ev = run(rcw, env, t, 12, 3, "on the generator")
    assert ev["truncations"] > 0 and ev["closes_outside_the_rows"] == 0
    env.close()


# ---- 9: a handle that has not enabled it; enabling twice -------------------------------------------------------------------------------
def test_getters_on_a_disabled_handle_and_enabling_twice(rcw):
    env = make(rcw, 64, H=4, W=4, limit=3)
    lib, h = env._lib, env._h
    p = [C.c_void_p() for _ in range(7)]
    buf = np.zeros(64 * 8, np.uint64)
    assert env.episode_stats_info == dict(enabled=False, rows=0, first=0) and not env.episode_stats_enabled
    assert lib.rcw_episode_stats(h, *[None] * 7) == UNSUPPORTED
    assert lib.rcw_episode_stats_device_ptr(h, *[C.byref(x) for x in p]) == UNSUPPORTED and not any(x.value for x in p)
    assert lib.rcw_episode_stats_table(h, buf.ctypes.data_as(C.c_void_p)) == UNSUPPORTED
    assert lib.rcw_episode_stats_table_device_ptr(h, C.byref(p[0])) == UNSUPPORTED
    assert lib.rcw_episode_stats_clear(h) == UNSUPPORTED
    assert lib.rcw_set_episode_stats(h, 0) == 0                              # RCW_OK also where there was none
    rng = np.random.default_rng(0)
    for _ in range(4):                                                       # a handle that never enabled it steps as ever
        rcw.act_(env, WR.draw_actions(rng, 64))
    env.set_episode_stats(True)
    t = Tracked(env)                                                         # in the middle of episodes: every record begins here
    ev = run(rcw, env, t, 9, 1, "first enabling")
    assert ev["truncations"] > 0 and t.ref.episodes.any() and t.ref.table.any()
    env.set_episode_stats(True)                                              # again: from zero
    t = Tracked(env)
    assert not np.asarray(env.episode_stats.episodes).any() and not np.asarray(env.episode_stats_table(device=True)).any()
    assert env.episode_stats_table()["totals"]["episodes"] == 0 and np.isnan(env.episode_stats_table()["spl"]["totals"])
    run(rcw, env, t, 5, 2, "second enabling")
    env.set_episode_stats(False)
    assert lib.rcw_episode_stats_clear(h) == UNSUPPORTED
    env.close()


# ---- 10: a replayed graph of a step -----------------------------------------------------------------------------------------------------
def test_a_replayed_graph_records_like_any_step(rcw, oracle):
    """one captured step (two launches, one stream, no top view: no parallel branch), replayed 2 L + 2 times with the same device actions"""
    torch = pytest.importorskip("torch")
    s = Recorded(rcw, oracle, form="two-launches", **dict(A, bad_every=0))
    stream = torch.cuda.Stream()
    s.env.sync()
    s.env.set_stream(stream.cuda_stream)
    a_host = TL.draw_actions(s.rng, s.B, 0)
    with torch.cuda.stream(stream):
        actions = torch.from_numpy(a_host).cuda()
        for _ in range(2):
            s.step("warm-up", a=a_host, device=True)
        stream.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            s.rcw.act_(s.env, actions)
        for k in range(2 * A["L"] + 2):
            g.replay(); s.ref.step(a_host); s.feed(a_host)
            stream.synchronize()
            s.check(f"replay {k}")
    ev = s.stats.events
    assert ev["truncations"] > 0 and ev["restarts_after_truncation"] > 0 and int(s.stats.episodes.max()) >= 2, ev
    del g
    s.close()


# ---- 11: two shards against the whole batch ------------------------------------------------------------------------------------------------
def test_two_shards_sum_to_the_whole_batch(rcw):
    """handles of 32 and 33 agents with agent_id_offset 0 and 32 against one of 65 on the bank scenario: the per-agent words are the slices,
    and the table is additive over shards"""
    whole = bank_env(rcw)
    parts = [bank_env(rcw, B=32, agent_id_offset=0), bank_env(rcw, B=33, agent_id_offset=32)]
    tw, tp = Tracked(whole), [Tracked(e) for e in parts]
    cut = [slice(0, 32), slice(32, 65)]
    for k, a in enumerate(EC.bank_actions()[:24]):
        rcw.act_(whole, a); tw.stepped(f"whole step {k}")
        for e, t, sl in zip(parts, tp, cut):
            rcw.act_(e, a[sl]); t.stepped(f"shard {sl.start} step {k}")
        for w in ES.WORDS:
            np.testing.assert_array_equal(np.concatenate([getattr(t.ref, w) for t in tp]), getattr(tw.ref, w), err_msg=f"{w} step {k}")
        tables = [np.asarray(e.episode_stats_table(device=True)) for e in parts]
        np.testing.assert_array_equal(tables[0] + tables[1], np.asarray(whole.episode_stats_table(device=True)), err_msg=f"the table, step {k}")
    ev = tw.ref.events
    assert ev["successes"] > 0 and ev["truncations"] > 0 and all(t.ref.table[0, 0] > 0 for t in tp)
    for e in parts + [whole]:
        e.close()
