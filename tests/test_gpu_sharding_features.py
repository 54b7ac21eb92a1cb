"""Four shards of a global batch of 16 on the GPU with every feature on: ShardedSingleRoom(16, rank=r, world=4) engines — 4 agents at
agent_id_offset = 4 r, all four handles alive in one process and stepped in turn — against the [4 r, 4 r + 4) slice of the WHOLE batch's
reference, never against another engine.  sharded.py: "agent_id_offset keys the reset generator by GLOBAL id, so the states do not depend
on how the batch is sharded"; what draws from that generator or indexes per-agent state since walls, the time limit, the goal distance and
the frame stack came — reset_agent's goal redraw loop, reset_preview in the one-launch step, the *_limit_kernel twins, rcw_set_walls'
layout index, the flood behind a restart, the stack's refill — runs here at a non-zero offset.

The expected values are tests/test_gpu_walls_time_limit.py's rollouts (TimeLimitRef over WallsRef, the rollouts the unsharded engine is
held to).  tests/test_sharded_walls_spec.py anchors them: a reference shard at offset 4 r is that slice, and every shard of ROOMS, WIDE and
F64 sees >= 1 restart after done, >= 17 after a truncation and >= 1 goal redraw inside a truncation restart (its table, asserted there).

A rollout compares every rank after every step and names the ranks that differ at the end, each with its first difference.
"""
import numpy as np
import pytest

import goal_distance_ref as GD
import learner_view_ref as LV
import learner_view_stack_ref as LS
import time_limit_ref as TL
import walls_ref as WR
from test_gpu_walls import CASES, ROOMS, engine_state, make_ref, three_layouts, walls_of
from test_gpu_walls_time_limit import LIMITS, REHEARSED, COLUMNS
from test_gpu_walls_time_limit import assert_equal as assert_limited_equal
from test_gpu_walls_time_limit import rollout as whole_rollout

pytestmark = pytest.mark.gpu

G, WORLD, PER = 16, 4, 4
TOUCHED = [1, 4, 6, 11, 15]                                                  # one or two agents of every shard


def make_shards(rcw, c, form=None, make_rng=None):
    """the four engines of the global batch (test_gpu_walls.make_env's keywords), the step's form forced: four agents would take two
    launches.  make_rng: every rank's own generator, in the same state (the ranks of a job are processes; here they share one)."""
    assert c["B"] == G
    shards = [rcw.ShardedSingleRoom(G, rank=r, world=WORLD, device=0, seed=c["seed"], T=c.get("T", "Float32"), auto_reset=True, num_directions=8,
                                    position_increment_wu=0.25, player_radius_wu=0.3, height_tile_map_tu=c["H"], width_tile_map_tu=c["W"],
                                    num_rays=c["N"], height_camera_view_pu=c["Hc"], **({"rng": make_rng()} if make_rng else {}))
              for r in range(WORLD)]
    for r, sh in enumerate(shards):
        assert (sh.first, sh.count, sh.env.batch, sh.env.cfg.agent_id_offset) == (PER * r, PER, PER, PER * r)
        if form is not None:
            sh.env.set_step_form(form)
            assert sh.env.step_form() == form
    return shards


def close(shards):
    for sh in shards:
        sh.close()


def shard_of(whole, r):
    """rank r's rows of a snapshot (a dict of arrays indexed by global agent) or of one such array"""
    if isinstance(whole, dict):
        return {k: v[PER * r:PER * (r + 1)] for k, v in whole.items()}
    return whole[PER * r:PER * (r + 1)]


class Ranks:
    """the first difference of every rank: a rank that differed is compared no further, the others go on"""

    def __init__(self):
        self.first = {}

    def check(self, r, compare):
        if r in self.first:
            return
        try:
            compare()
        except AssertionError as e:
            self.first[r] = str(e).strip()

    def settle(self):
        if self.first:
            pytest.fail(f"ranks {sorted(self.first)} differ from their slice of the whole batch; ranks {sorted(set(range(WORLD)) - set(self.first))} do not\n" +
                        "\n".join(f"--- rank {r}: {m}" for r, m in sorted(self.first.items())), pytrace=False)


def set_walls_and_limit(shards, name):
    walls, index = walls_of(name)
    L, _ = LIMITS[name]
    for sh in shards:
        sh.set_walls(walls, index)                                           # the GLOBAL index, through the wrapper
        np.testing.assert_array_equal(sh.env.world.walls, walls[index][sh.first:sh.first + PER])
        sh.env.set_time_limit(L)
        assert sh.env.time_limit == L


def whole(name):
    snaps, actions, events = whole_rollout(name)
    assert tuple(events[k] for k in COLUMNS) == REHEARSED[name], events       # (the rollout tests/test_sharded_walls_spec.py's table is about)
    return snaps, actions


ROLLOUTS = [("ROOMS", "two-launches"), ("ROOMS", "one-launch"), ("WIDE", "one-launch"), ("F64", None)]


@pytest.mark.parametrize("name,form", ROLLOUTS, ids=[f"{n}-{f or 'auto'}" for n, f in ROLLOUTS])
def test_every_shard_is_its_slice_of_the_limited_rollout_on_a_walled_map(rcw, name, form):
    """ROOMS: a wavefront per agent (one-launch: reset_preview and reset_agent have to agree under the offset); WIDE: a workgroup per
    agent; F64: the flat fill in two launches"""
    snaps, actions = whole(name)
    shards = make_shards(rcw, CASES[name], form)
    if name == "F64":
        assert all(sh.env.step_form() == "two-launches" and sh.env.fill_kernel_name() == "rcw_fill_flat_kernel" for sh in shards)
    set_walls_and_limit(shards, name)
    ranks = Ranks()
    for r, sh in enumerate(shards):
        ranks.check(r, lambda: assert_limited_equal(sh.env, shard_of(snaps[0], r), f"{name}, rank {r}: behind set_walls and set_time_limit"))
    for t, a in enumerate(actions):
        for sh in shards:
            sh.act_(sh.local_slice(a))
        for r, sh in enumerate(shards):
            ranks.check(r, lambda: assert_limited_equal(sh.env, shard_of(snaps[t + 1], r), f"{name} ({form}), rank {r}: step {t}"))
    if form is not None:
        assert all(sh.env.step_form() == form for sh in shards)
    close(shards)
    ranks.settle()


def goal_distance_words(env):
    return dict(goal_distance=env.goal_distance.numpy(), goal_start_distance=env.goal_start_distance.numpy(), goal_progress=env.goal_progress.numpy(),
                goal_distance_field=env.goal_distance_field)


@pytest.mark.parametrize("form", ["two-launches", "one-launch"])
def test_every_shard_with_everything_on_at_once(rcw, form):
    """the ROOMS rollout again with the goal distance and a stacked learner view on every shard.  Both are expected from the REFERENCE's
    state of the whole batch — GoalDistanceRef fed the reference's walls, goals, positions and episode counters, StackModel pushed with
    learner_view_ref.from_descriptors of the reference's descriptors and its counters (a truncation restart moves the counter: a
    refill) — and sliced; the shard's own state is held to the same snapshot first."""
    name, c = "ROOMS", ROOMS
    snaps, actions = whole(name)
    walls, index = walls_of(name)
    shards = make_shards(rcw, c, form)
    for sh in shards:
        sh.env.set_learner_view("gray", (21, 21), "chw", stack=2)
    set_walls_and_limit(shards, name)
    for sh in shards:
        sh.env.set_goal_distance()
        assert sh.env.goal_distance_enabled
    view = lambda s: LV.from_descriptors(s["col_height"], s["col_colour"], shards[0].env.cfg, c["Hc"], "gray", (21, 21))
    state = lambda s: (walls[index], s["goal"], s["position"], s["episode"])
    stack = LS.StackModel(2, view(snaps[0]), snaps[0]["episode"])
    dist = GD.GoalDistanceRef(*state(snaps[0]))
    restarted, progress = np.zeros(G, int), 0

    def compare(r, sh, snap, where):
        assert_limited_equal(sh.env, shard_of(snap, r), where)
        got = goal_distance_words(sh.env)
        want = dict(goal_distance=dist.distance, goal_start_distance=dist.start_distance, goal_progress=dist.progress, goal_distance_field=dist.fields)
        for k in want:
            assert got[k].dtype == want[k].dtype
            np.testing.assert_array_equal(got[k], shard_of(want[k], r), err_msg=f"{k} {where}")
        np.testing.assert_array_equal(sh.env.learner_view_host(), shard_of(stack.stack, r), err_msg=f"the stack {where}")

    ranks = Ranks()
    for r, sh in enumerate(shards):
        ranks.check(r, lambda: compare(r, sh, snaps[0], f"rank {r}: everything switched on"))
    for t, a in enumerate(actions):
        for sh in shards:
            sh.act_(sh.local_slice(a))
        restarted += stack.push(view(snaps[t + 1]), snaps[t + 1]["episode"])
        dist.stepped(*state(snaps[t + 1]))
        progress += int((dist.progress != 0).sum())
        for r, sh in enumerate(shards):
            ranks.check(r, lambda: compare(r, sh, snaps[t + 1], f"({form}) rank {r}: step {t}"))
    assert (restarted.reshape(WORLD, PER).sum(axis=1) >= 18).all() and progress > 0, (restarted, progress)   # (>= 17 + 1 restarts a shard: the spec file's table)
    assert all(sh.env.step_form() == form for sh in shards)
    close(shards)
    ranks.settle()


def test_a_masked_global_set_walls_in_the_one_launch_form(rcw):
    """5 steps, set_walls(walls, (index + 1) % 3, global mask) on every rank — one or two agents of every shard —, 10 more steps: each
    shard against its slice of a 16-agent WallsRef given the same calls; the untouched agents of each shard keep every byte across the call"""
    c = ROOMS
    walls, index = walls_of("ROOMS")
    shards, ref = make_shards(rcw, c, "one-launch"), make_ref(c)
    for sh in shards:
        sh.set_walls(walls, index)
    ref.set_walls(walls, index)
    rng = np.random.default_rng(c["seed"] + 1)
    ranks = Ranks()

    def steps(n, where):
        for t in range(n):
            a = WR.draw_actions(rng, G)
            for sh in shards:
                sh.act_(sh.local_slice(a))
            ref.step(a)
            snap = ref.snapshot()
            for r, sh in enumerate(shards):
                ranks.check(r, lambda: WR.assert_equal(sh.env, shard_of(snap, r), f"rank {r}: step {t} {where}"))

    steps(5, "behind set_walls")
    mask = np.zeros(G, np.uint8); mask[TOUCHED] = 1
    other = ((index + 1) % 3).astype(np.int32)
    assert all(1 <= shard_of(mask, r).sum() <= 2 for r in range(WORLD))
    ref.set_walls(walls, other, mask)
    snap = ref.snapshot()
    for r, sh in enumerate(shards):
        before = engine_state(sh.env)
        sh.set_walls(walls, other, mask)                                     # the GLOBAL index and mask
        after = engine_state(sh.env)
        keep = shard_of(mask, r) == 0

        def compare():
            for k in before:
                np.testing.assert_array_equal(after[k][keep], before[k][keep], err_msg=f"rank {r}: {k} of the untouched agents")
            np.testing.assert_array_equal(after["episode"][~keep], before["episode"][~keep] + 1, err_msg=f"rank {r}: the touched agents' episode")
            WR.assert_equal(sh.env, shard_of(snap, r), f"rank {r}: behind the masked set_walls")

        ranks.check(r, compare)
        assert sh.env.step_form() == "one-launch"
    steps(10, "behind the masked set_walls")
    assert ref.events["restarts_after_done"] > 0 and ref.events["goal_redraws"] > 0, ref.events
    close(shards)
    ranks.settle()


@pytest.mark.parametrize("form", ["two-launches", "one-launch"])
def test_device_resets_through_the_wrapper_on_a_walled_map(rcw, form):
    """reset_(seed=31), then reset_(local_mask=the shard's slice of a global mask, seed=77), then 5 steps under a time limit of 2: each
    shard against its slice of WallsRef.reset(None, 31) / reset(mask, 77).  The limit makes every agent that did not reach its goal
    restart on step 3 — the agents the masked reset did not touch among them, with the seed it brought."""
    c, L = ROOMS, 2
    walls, index = walls_of("ROOMS")
    shards, ref = make_shards(rcw, c, form), make_ref(c)
    for sh in shards:
        sh.set_walls(walls, index)
        sh.env.set_time_limit(L)
    ref.set_walls(walls, index)
    lim = TL.TimeLimitRef(ref, L, c["seed"], True)
    snapshot = lambda: dict(ref.snapshot(), episode_steps=lim.episode_steps.copy(), truncated=lim.truncated.copy())
    ranks = Ranks()

    def compare_all(where):
        snap = snapshot()
        for r, sh in enumerate(shards):
            ranks.check(r, lambda: assert_limited_equal(sh.env, shard_of(snap, r), f"({form}) rank {r}: {where}"))

    compare_all("behind set_walls")
    for sh in shards:
        sh.reset_(seed=31)
    ref.reset(None, 31); lim.clear(); lim.seed = 31
    compare_all("behind reset_(seed=31)")
    mask = np.zeros(G, np.uint8); mask[TOUCHED] = 1
    for sh in shards:
        sh.reset_(local_mask=sh.local_slice(mask), seed=77)
    ref.reset(mask, 77); lim.clear(mask); lim.seed = 77
    compare_all("behind the masked reset_(seed=77)")
    episode = ref.episode.copy()
    rng = np.random.default_rng(c["seed"] + 1)
    for t in range(5):
        a = WR.draw_actions(rng, G)
        for sh in shards:
            sh.act_(sh.local_slice(a))
        lim.step(a)
        compare_all(f"step {t} behind the resets")
    untouched_restarts = ((ref.episode - episode) * (mask == 0)).reshape(WORLD, PER).sum(axis=1)
    assert (untouched_restarts >= 2).all(), untouched_restarts               # in every shard, agents outside the mask restarted with the new seed
    assert all(sh.env.step_form() == form for sh in shards)
    close(shards)
    ranks.settle()


def test_the_rng_keyword_on_the_device(rcw):
    """ShardedSingleRoom(rng=default_rng(5)) on every rank, then set_walls(three_layouts, index): each shard's goal, pose and heading are the
    twin generator's draws for ITS global agents — behind the two construction resets an agent —, and frames, descriptors and tile map
    are the reference worlds' with those draws injected"""
    SR = rcw.SingleRoomModule
    c = ROOMS
    walls, index = three_layouts(6, 6), (np.arange(G) % 3).astype(np.int32)
    shards = make_shards(rcw, c, make_rng=lambda: np.random.default_rng(5))
    twin = np.random.default_rng(5)
    for _ in range(2 * G):                                                   # the constructor's two resets an agent (SR:62-74, SR:105)
        SR.reference_reset_draws(twin, 6, 6, 8)
    for sh in shards:
        sh.set_walls(walls, index)
    draws = [SR.reference_reset_draws(twin, 6, 6, 8, walls=walls[index[b]]) for b in range(G)]
    goal = np.array([d[:2] for d in draws], np.int32)
    pos = np.array([(d[2] - 0.5, d[3] - 0.5) for d in draws], np.float32)
    heading = np.array([d[4] for d in draws], np.int32)
    assert not walls[index][np.arange(G), goal[:, 0] - 1, goal[:, 1] - 1].any()
    ref = make_ref(c)
    ref.set_walls(walls, index)
    ref.set_state(goal, pos, heading)
    want = ref.snapshot()
    ranks = Ranks()
    for r, sh in enumerate(shards):
        def compare():
            w = sh.env.world
            np.testing.assert_array_equal(w.goal_position, shard_of(goal, r), err_msg=f"rank {r}: goal")
            np.testing.assert_array_equal(w.player_position_wu.view(np.uint32), shard_of(pos, r).view(np.uint32), err_msg=f"rank {r}: position")
            np.testing.assert_array_equal(w.player_direction_au, shard_of(heading, r), err_msg=f"rank {r}: heading")
            np.testing.assert_array_equal(sh.env.camera_view_host(), shard_of(want["camera_view"], r), err_msg=f"rank {r}: camera view")
            np.testing.assert_array_equal(w.tile_map_chunks, shard_of(want["tile_map_chunks"], r), err_msg=f"rank {r}: tile map")
            h, cc = sh.env.columns()
            np.testing.assert_array_equal(h, shard_of(want["col_height"], r), err_msg=f"rank {r}: height_line_pu")
            np.testing.assert_array_equal(cc, shard_of(want["col_colour"], r), err_msg=f"rank {r}: colour id")
            assert sh.rng.bit_generator.state == twin.bit_generator.state, f"rank {r}: every global agent's draws, no more"

        ranks.check(r, compare)
    close(shards)
    ranks.settle()
