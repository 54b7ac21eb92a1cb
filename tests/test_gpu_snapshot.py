"""The state archive on the GPU (include/rcw.h, "the state archive"): save and restore of agent records, with EVERY feature on
(tests/snapshot_cases.py: a wall bank, a limit of 8, the goal distance, the seen map, a local map of it, a k-frame learner view, the
statistics, auto_reset).

The yardstick is the engine's own UNRESTORED continuation, which the existing suite holds to the oracles: after a restore the same actions
must leave the same bytes in every per-agent output, the camera frames and the table's changes, call by call.  test_rewind_beside_the_oracle
holds the restored state to the C oracle and the limit's reference as well, on the time limit's harness.

Shapes: B in {1, 63, 64, 65, 257} — a lone lane, a wave tail on either side, a second workgroup of the resolve kernel with one lane —, the
5 x 5 map with gray 7 x 9, k = 3 (50-, 25- and 189-byte segments: the byte path) and the 4 x 4 map with gray 8 x 8, k = 4 (32- and 256-byte
segments: the 16-byte path), rows in {1, B, B + 3}, both step forms, both world-unit types.

Every export is missing from the build before this feature: each test here fails there."""
import numpy as np
import pytest

import deferred as D
import snapshot_cases as SC

pytestmark = pytest.mark.gpu
UNSUPPORTED, INVALID_ARGUMENT = -7, -1

T1, T2 = SC.T1, SC.T2


def rows_for(B, rows, seed=3):
    """distinct rows for the B agents out of `rows` >= B, not the identity where there is room"""
    return np.random.default_rng(seed).permutation(rows)[:B].astype(np.int32)


@pytest.mark.parametrize("case", range(len(SC.REWINDS)), ids=[f"B{b}-{'odd' if c is SC.ODD else 'wide'}-{f or 'auto'}-{t}-rows{r}" for b, c, f, t, r, _, _ in SC.REWINDS])
def test_rewind(rcw, case):
    """Step 11 times, save, step 14 more with a record behind every call; restore and replay: every record byte for byte, the table's
    changes included, and the episodes that restart behind the restore draw the same layouts.  Every window holds a restart behind a
    goal, a truncation and a turn-only step: seeds and length were rehearsed on the CPU (tests/snapshot_cases.py `rehearse`:
    tests/wall_bank_ref.py under tests/time_limit_ref.py; tests/test_snapshot_spec.py runs it), and the engine's own recorded counters
    must be the rehearsal's, case by case — restarts behind a goal, truncations, turn-only steps, restarts onto another layout:
    B = 1: 1, 1, 4, 1; B = 63: 17, 65, 276, 33; B = 64: 36, 73, 238, 43; B = 65: 18, 65, 297, 29; B = 257 (4 x 4): 173, 256, 1002,
    145; B = 257 (5 x 5): 78, 258, 1047, 111."""
    B, c, form, T, rows, seed, action_seed = SC.REWINDS[case]
    env = SC.make(rcw, B, c, form=form, T=T, rows=rows, seed=seed)
    acts = SC.actions(B, T1 + T2, seed=action_seed)
    which = rows_for(B, rows) if rows > 1 else None
    for a in acts[:T1]:
        rcw.act_(env, a)
    env.snapshot_save(which)
    assert env.snapshot_filled.sum() == B
    at_save = SC.record(env)
    first = SC.play(rcw, env, acts[T1:])
    ev = SC.window_events(first, at_save)
    assert ev["goal_restarts"] > 0 and ev["truncations"] > 0 and ev["turn_only"] > 0, ev
    assert tuple(ev[k] for k in SC.EVENTS) == SC.REHEARSED[case], ev
    env.snapshot_restore(which)
    SC.assert_same(SC.record(env), at_save, "behind the restore")
    second = SC.play(rcw, env, acts[T1:])
    for k, (g, w) in enumerate(zip(second, first)):
        SC.assert_same(g, w, f"replayed step {k}", table=True)
    assert tuple(SC.window_events(second, at_save)[k] for k in SC.EVENTS) == SC.REHEARSED[case]
    if form is not None:
        assert env.step_form() == form
    env.close()


@pytest.mark.parametrize("B,c,form", [(65, SC.ODD, "one-launch"), (257, SC.WIDE, "two-launches"), (64, SC.ODD, "two-launches")])
def test_masked_restore(rcw, B, c, form):
    """unmasked agents: every output, frames included, as just before the call; masked agents: their rows.  Then both go on as their
    own unrestored continuations would: the masked agents' from the save, the others' from where they were."""
    env = SC.make(rcw, B, c, form=form, rows=B + 3)
    acts = SC.actions(B, 16, seed=40 + B)
    which = rows_for(B, B + 3)
    for a in acts[:6]:
        rcw.act_(env, a)
    env.snapshot_save(which)
    at_save = SC.record(env)
    from_save = SC.play(rcw, env, acts[6:10])
    before = SC.record(env)
    mask = (np.random.default_rng(B).random(B) < 0.5).astype(np.uint8)
    mask[0], mask[-1] = 1, 0
    m, u = np.flatnonzero(mask), np.flatnonzero(mask == 0)
    env.snapshot_restore(which, mask)
    after = SC.record(env)
    SC.assert_same(after, before, "unmasked agents", agents=u)
    SC.assert_same(after, at_save, "masked agents", agents=m)
    np.testing.assert_array_equal(after["table"], before["table"])
    # the masked agents replay the four steps behind the save
    got = SC.play(rcw, env, acts[6:10])
    for k, (g, w) in enumerate(zip(got, from_save)):
        SC.assert_same(g, w, f"masked agents, replayed step {k}", agents=m)
    env.close()


@pytest.mark.parametrize("B,c,form,T", [(65, SC.ODD, "two-launches", "Float32"), (64, SC.WIDE, "one-launch", "Float64")])
def test_gather(rcw, B, c, form, T):
    """without auto_reset: agent i restored from agent p[i]'s row and fed p[i]'s actions puts out what p[i] put out, step by step — for a
    permutation, and for every agent from row 0 — and the reset behind it counts the SOURCE's episode on"""
    env = SC.make(rcw, B, c, form=form, T=T, rows=B, auto_reset=False)
    acts = SC.actions(B, 14, seed=70 + B)
    for a in acts[:5]:
        rcw.act_(env, a)
    env.snapshot_save()
    at_save = SC.record(env)
    first = SC.play(rcw, env, acts[5:])
    for name, p in (("a permutation", np.random.default_rng(1).permutation(B).astype(np.int32)), ("row 0", np.zeros(B, np.int32))):
        env.snapshot_restore(p)
        everyone = np.arange(B)
        SC.assert_same(SC.record(env), at_save, f"{name}: behind the restore", agents=everyone, source=p)
        got = SC.play(rcw, env, acts[5:], select=p)
        for k, (g, w) in enumerate(zip(got, first)):
            SC.assert_same(g, w, f"{name}: step {k}", agents=everyone, source=p)
        rcw.reset_(env)
        np.testing.assert_array_equal(env.world.episode, first[-1]["episode"][p] + 1)
    env.close()


@pytest.mark.parametrize("B,pair", [(65, (3, 64)), (257, (5, 200))])
def test_two_agents_saving_into_one_row_on_the_device_leave_the_higher_one(rcw, B, pair):
    """the device path alone takes two agents into one row: the row holds the WHOLE record of the higher-numbered one (proved by restoring
    it into a third agent), on both the byte path's and the 16-byte path's segments; the host path refuses the pair"""
    torch = pytest.importorskip("torch")
    for c in (SC.ODD, SC.WIDE):
        env = SC.make(rcw, B, c, rows=2)
        for a in SC.actions(B, 7, seed=B):
            rcw.act_(env, a)
        lo, hi = pair
        rows, mask = np.zeros(B, np.int32), np.zeros(B, np.uint8)
        mask[[lo, hi]] = 1
        with pytest.raises(ValueError, match=rf"agent {hi}: row 0 is also agent {lo}'s"):
            env.snapshot_save(rows, mask)
        assert not env.snapshot_filled.any()
        before = SC.record(env)
        dev = f"cuda:{env.device}"
        env.snapshot_save(torch.from_numpy(rows).to(dev), torch.from_numpy(mask).to(dev))
        env.sync()
        assert env.snapshot_filled.tolist() == [True, False]
        third = np.zeros(B, np.uint8)
        third[0] = 1
        env.snapshot_restore(rows, third)
        after = SC.record(env)
        SC.assert_same(after, before, "the third agent holds the higher agent's record", agents=np.array([0]), source=np.array([hi]))
        assert any(before[k][lo].tobytes() != before[k][hi].tobytes() for k in SC.PER_AGENT)
        SC.assert_same(after, before, "everyone else", agents=np.arange(1, B))
        env.close()


def digest(env):
    return SC.record(env), env.snapshot_export()["rows"].tobytes(), env.snapshot_filled.tolist()


def test_bad_indices(rcw):
    """-1, `rows` and an unfilled row.  Host variants: refused with the agent named, nothing changes (every output, the archive's bytes and
    its filled flags).  Device variants: that agent is left as it was, its status word and the handle's error word are
    RCW_ERR_INVALID_ARGUMENT, the others are served, clear_error clears it."""
    torch = pytest.importorskip("torch")
    B, R = 65, 70
    env = SC.make(rcw, B, SC.ODD, rows=R)
    acts = SC.actions(B, 9, seed=8)
    for a in acts[:4]:
        rcw.act_(env, a)
    good = np.arange(B, dtype=np.int32)                                        # rows 65 .. 69 stay unfilled
    env.snapshot_save(good)
    at_save = SC.record(env)
    for a in acts[4:]:
        rcw.act_(env, a)
    dev = f"cuda:{env.device}"
    for bad, restore_only in ((-1, False), (R, False), (B + 2, True)):
        rows = good.copy()
        rows[7] = bad
        before = digest(env)
        for what in ("restore",) if restore_only else ("save", "restore"):
            with pytest.raises(ValueError, match=r"agent 7: row"):
                getattr(env, f"snapshot_{what}")(rows)
            after = digest(env)
            SC.assert_same(after[0], before[0], f"host {what} with row {bad}", table=True)
            assert after[1:] == before[1:]
        # the device variant: a restore serves the 64 others and leaves agent 7
        env.snapshot_restore(torch.from_numpy(rows).to(dev))
        with pytest.raises(ValueError, match="rcw_snapshot_restore_device"):
            env.sync()
        status = env.world.status
        assert status[7] == INVALID_ARGUMENT and not np.delete(status, 7).any()
        env.clear_error()
        env.sync()
        assert not env.world.status.any()
        after = SC.record(env)
        others = np.delete(np.arange(B), 7)
        SC.assert_same(after, before[0], f"device restore with row {bad}: the agent itself", agents=np.array([7]))
        SC.assert_same(after, at_save, f"device restore with row {bad}: the others", agents=others)
        for a in acts[4:]:
            rcw.act_(env, a)
    # ... and a device save: the bad agent's row is not written, the others' are
    rows = good.copy()
    rows[7] = R
    env.set_snapshots(R)
    env.snapshot_save(torch.from_numpy(rows).to(dev))
    with pytest.raises(ValueError):
        env.sync()
    assert env.world.status[7] == INVALID_ARGUMENT
    env.clear_error()
    filled = env.snapshot_filled
    assert not filled[7] and filled[others].all() and not filled[B:].any()
    env.close()


def test_shape_binding(rcw):
    """a feature toggled, another view size or k, another local-map size, another source kind: save and restore are refused with the
    segment named and nothing changes; binding again makes them work, with every row unfilled"""
    from raycastworlds_jl_amd import _capi

    B = 5
    env = SC.make(rcw, B, SC.ODD, rows=B, local_source="world")
    env.snapshot_save()
    c = SC.ODD
    toggles = [
        ("goal_distance.field", lambda: env.set_goal_distance(False)),
        ("goal_distance.field", lambda: env.set_goal_distance(True)),
        ("seen_map.seen_count", lambda: env.set_seen_map(False)),
        ("episode_stats.finished", lambda: env.set_episode_stats(False)),
        ("learner_view.stack", lambda: env.set_learner_view("gray", size=c["view"], stack=c["k"] + 1)),
        ("learner_view.stack", lambda: env.set_learner_view("gray", size=c["view"][::-1], stack=c["k"] + 1)),     # the same bytes
        ("learner_view.frame", lambda: env.set_learner_view("gray", size=c["view"], stack=1)),
        ("learner_view.frame", lambda: env.set_learner_view(None)),
        ("local_map.image", lambda: env.set_local_map(7)),
        ("local_map.image", lambda: env.set_local_map(0)),
        ("layout_source.last_episode", lambda: env.set_wall_bank(None)),
        ("layout_source.last_episode", lambda: env.set_wall_generator(levels=3)),
        ("layout_source.last_episode", lambda: (env.set_wall_generator(None), env.set_wall_caves(levels=3))),    # another kind, the same bytes
    ]
    for segment, toggle in toggles:
        info = env.snapshot_info
        assert env.snapshot_filled.all()
        toggle()
        assert env.snapshot_info == info                                       # (the archive's: bound to the old shape)
        for call in (env.snapshot_save, env.snapshot_restore):
            with pytest.raises(_capi.RcwError, match=rf"segment {segment};") as e:
                call()
            assert e.value.code == UNSUPPORTED
        assert env.snapshot_filled.all()
        env.set_snapshots(B)
        assert env.snapshot_info["shape_key"] != info["shape_key"] and not env.snapshot_filled.any()
        with pytest.raises(ValueError, match="row 0 has not been filled"):
            env.snapshot_restore()
        env.snapshot_save()
        env.snapshot_restore()
    env.set_snapshots(0)
    assert env.snapshot_info["rows"] == 0
    with pytest.raises(_capi.RcwError, match="no state archive"):
        env.snapshot_save()
    with pytest.raises(ValueError, match="rows must be in"):
        env.set_snapshots(_capi.RCW_SNAPSHOT_MAX_ROWS + 1)
    env.close()


@pytest.mark.parametrize("B,c,T", [(65, SC.ODD, "Float32"), (64, SC.WIDE, "Float64")])
def test_export_and_import(rcw, B, c, T):
    """rows exported from one handle and imported into another of the same configuration and seed but another history: restored there,
    its continuation is the first handle's.  A wrong shape key and a corrupted row are refused, and nothing is loaded."""
    import struct

    from raycastworlds_jl_amd import _capi

    one = SC.make(rcw, B, c, T=T, rows=B)
    acts = SC.actions(B, 15, seed=90 + B)
    for a in acts[:7]:
        rcw.act_(one, a)
    one.snapshot_save()
    at_save = SC.record(one)
    d = one.snapshot_export()
    assert d["rows"].shape == (B, one.snapshot_info["row_bytes"]) and d["shape_key"] == one.snapshot_info["shape_key"]
    want = SC.play(rcw, one, acts[7:])
    one.close()

    two = SC.make(rcw, B, c, T=T, rows=B + 3)
    for a in SC.actions(B, 4, seed=1):
        rcw.act_(two, a)
    assert two.snapshot_info["shape_key"] == d["shape_key"]
    with pytest.raises(_capi.RcwError, match="shape key") as e:
        two.snapshot_import(dict(d, shape_key=d["shape_key"] ^ 1), first=3)
    assert e.value.code == UNSUPPORTED
    spoiled = d["rows"].copy()
    dir_at = 16 if T == "Float64" else 8                                       # behind pos
    spoiled[B - 1, dir_at:dir_at + 4] = np.frombuffer(struct.pack("<i", 8), np.uint8)   # direction == num_directions
    with pytest.raises(ValueError, match=rf"row {B + 2}: dir:"):
        two.snapshot_import(dict(d, rows=spoiled), first=3)
    assert not two.snapshot_filled.any()
    two.snapshot_import(d, first=3)
    assert two.snapshot_filled.tolist() == [False] * 3 + [True] * B
    assert two.snapshot_export(first=3)["rows"].tobytes() == d["rows"].tobytes()
    two.snapshot_restore(np.arange(3, B + 3, dtype=np.int32))
    SC.assert_same(SC.record(two), at_save, "behind the restore of imported rows")
    got = SC.play(rcw, two, acts[7:])
    for k, (g, w) in enumerate(zip(got, want)):
        SC.assert_same(g, w, f"continuation step {k}", table=True)
    two.close()


def test_the_device_variants_wait_for_nothing(rcw):
    """behind tests/deferred.py's backlog (its driver's own, unedited): device steps, a device save, more steps, a device restore, a step —
    and the backlog's closing event is still pending when the host has queued them all.  The host variants are the ones that wait:
    INTEGRATION.md "Streams" lists them so."""
    torch = pytest.importorskip("torch")
    B = 65
    env = SC.make(rcw, B, SC.ODD, rows=B)
    acts = SC.actions(B, 6, seed=2)
    driver = D.Deferred(rcw, env, D.Steps(np.stack(acts)), mode="device", name="snapshots")
    stream = env.torch_stream()
    try:
        with torch.cuda.stream(stream):
            dev = f"cuda:{env.device}"
            device_actions = torch.from_numpy(np.stack(acts)).to(dev)
            rows = torch.arange(B, dtype=torch.int32, device=dev)
            mask = torch.ones(B, dtype=torch.uint8, device=dev)
            stream.synchronize()
            # the host variants are the ones that wait: the mirror counts a host synchronisation for each
            syncs = env.host_syncs
            env.snapshot_save(np.arange(B, dtype=np.int32))
            env.snapshot_restore(np.arange(B, dtype=np.int32), np.ones(B, np.uint8))
            assert env.host_syncs == syncs + 2
            syncs = env.host_syncs
            first, last = driver._backlog(torch)
            for k in range(3):
                rcw.act_(env, device_actions[k])
            env.snapshot_save(rows, mask)
            saved = {k: getattr(env, k).torch(sync=False).clone() for k in ("learner_view", "seen_count", "camera_view")}
            for k in range(3, 6):
                rcw.act_(env, device_actions[k])
            env.snapshot_restore(rows, mask)
            restored = {k: getattr(env, k).torch(sync=False).clone() for k in saved}
            rcw.act_(env, device_actions[3])
            pending = not last.query()
            assert env.host_syncs == syncs
            env.sync()
        assert first.elapsed_time(last) < D.BACKLOG_LIMIT_MS
        assert pending, "a device variant of the state archive waited for the stream: the backlog had ended behind the last call"
        for k in saved:
            assert torch.equal(saved[k], restored[k]), k
    finally:
        env.close()
        D.release_backlog()


def test_the_return_to_state_example_runs():
    """examples/return_to_state.py as a user would run it, in a process of its own: it archives, returns agents and says so"""
    import os
    import re
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "examples/return_to_state.py", "96", "60", "10"], cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"96 agents x 60 steps: the archived agent had seen (\d+) tiles, (\d+) returns to it", r.stdout)
    assert m and int(m.group(1)) > 0 and int(m.group(2)) > 0, r.stdout


# ---- beside the oracle: tests/test_gpu_time_limit.py's harness keeps engine, C oracle and tests/time_limit_ref.py in lockstep -----------------
def frozen(s):
    """what the harness' oracle and limit reference hold NOW, as `assert_state_equal` reads an oracle"""
    import types

    o = s.orc
    chunks = np.array(o.tile_map_chunks())
    return types.SimpleNamespace(direction=np.array(o.direction), goal=np.array(o.goal), position=np.array(o.position), reward=np.array(o.reward),
                                 done=np.array(o.done), tile_map_chunks=lambda: chunks, col_height=np.array(o.col_height), col_colour=np.array(o.col_colour),
                                 camera_view=np.array(o.camera_view), episode=np.array(o.episode), episode_steps=s.ref.episode_steps.copy(),
                                 truncated=s.ref.truncated.copy())


def held_to(env, f, where):
    from helpers import assert_state_equal

    assert_state_equal(env, f, where=where)                                    # pose, goal, reward, done, tile map, column descriptors, camera frames
    np.testing.assert_array_equal(env.world.episode, f.episode, err_msg=f"episode {where}")
    np.testing.assert_array_equal(env.world.episode_steps, f.episode_steps, err_msg=f"episode_steps {where}")
    np.testing.assert_array_equal(env.world.truncated.astype(np.uint8), f.truncated, err_msg=f"truncated {where}")


@pytest.mark.parametrize("name,form,batch", [("A", "two-launches", 65), ("A", "one-launch", 64), ("F64", None, 65)])
def test_rewind_beside_the_oracle(rcw, oracle, name, form, batch):
    """The time limit's harness (engine, C oracle and the limit's reference side by side, compared behind every step): 8 steps, a save, 12
    more with what the ORACLE holds behind each kept; then a restore, and the engine alone replays the 12 — behind the restore and behind
    every replayed step it must hold what the oracle held there: pose, goal, reward, done, episode, tile map, column descriptors, camera
    frames and the limit's two words.  The gather and the render behind it are thereby held to a reference that is not the engine.  The
    window's events are the reference's own counts."""
    import time_limit_ref as TL
    import test_gpu_time_limit as GT

    torch = pytest.importorskip("torch")
    case = dict(getattr(GT, name), bad_every=0)
    s = GT.Limited(rcw, oracle, form=form, batch=batch, **case)
    s.env.set_snapshots(batch + 3)
    rows = rows_for(batch, batch + 3)
    rng = np.random.default_rng(31)
    acts = [TL.draw_actions(rng, batch, 0) for _ in range(20)]
    for k, a in enumerate(acts[:8]):
        s.step(f"step {k}", a=a)
    s.env.snapshot_save(rows)
    at_save, before = frozen(s), dict(s.ref.events)
    kept = []
    for k, a in enumerate(acts[8:]):
        s.step(f"window step {k}", a=a)
        kept.append(frozen(s))
    ev = {k: s.ref.events[k] - before[k] for k in before}
    assert ev["truncations"] > 0 and ev["terminations"] > 0 and ev["restarts_after_done"] > 0 and ev["restarts_after_truncation"] > 0, ev
    assert (kept[-1].episode != at_save.episode).any()
    s.env.snapshot_restore(rows)
    held_to(s.env, at_save, "behind the restore")
    for k, a in enumerate(acts[8:]):
        rcw.act_(s.env, torch.from_numpy(a).cuda() if k % 2 else a)
        held_to(s.env, kept[k], f"replayed step {k}")
    # ... and a masked restore: the masked agents hold the oracle's state at the save, the others the oracle's at the end
    mask = (np.arange(batch) % 3 == 0).astype(np.uint8)
    s.env.snapshot_restore(rows, mask)
    w = s.env.world
    for key, got in (("position", w.player_position_wu), ("direction", w.player_direction_au), ("goal", w.goal_position), ("episode", w.episode),
                     ("camera_view", s.env.camera_view_host())):
        want = np.where(mask.astype(bool).reshape((-1,) + (1,) * (got.ndim - 1)), getattr(at_save, key), getattr(kept[-1], key))
        np.testing.assert_array_equal(got, want, err_msg=f"masked restore: {key}")
    if form is not None:
        assert s.env.step_form() == form
    s.close()
