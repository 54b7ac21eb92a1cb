"""ShardedSingleRoom.set_walls and the sharded references, without a device: four (and two) shards of a global batch of 16 against the
one 16-agent batch — sharded.py: "agent_id_offset keys the reset generator by GLOBAL id, so the states do not depend on how the batch is
sharded" — with walls, the time limit and the `rng` keyword on.

  (a) the references   tests/walls_ref.py's WallsRef at agent_id_offset = 4 r under tests/time_limit_ref.py's TimeLimitRef, fed its slice
                       of the whole rollout's actions, is the slice of tests/test_gpu_walls_time_limit.py's 16-agent rollout after every
                       step — the oracle tests/test_gpu_sharding_features.py slices — and every shard reaches every kind of restart:

      rollout (L, steps)   rank            restarts_after_truncation   restarts_after_done   goal_redraws    goal_redraws_on_truncation_restarts
      ROOMS (5, 30)        0 / 1 / 2 / 3   17 / 18 / 19 / 18           4 / 2 / 1 / 4         4 / 9 / 5 / 5   4 / 8 / 5 / 2
      WIDE (4, 30)         0 / 1 / 2 / 3   23 / 21 / 19 / 23           1 / 4 / 6 / 1         3 / 2 / 8 / 2   3 / 2 / 4 / 1
      F64 (5, 30)          0 / 1 / 2 / 3   18 / 18 / 19 / 18           2 / 2 / 1 / 2         6 / 5 / 6 / 5   4 / 5 / 6 / 4

                       (goal_redraws_on_truncation_restarts per shard as test_gpu_walls_time_limit.rollout counts it for the batch: the
                       growth of goal_redraws over the steps in which the shard restarted agents after a truncation and none after done.)
                       A change of a reference that moves a number: rehearse again and update the table; ">= 1 in every shard" stays.
  (b), (c), (d)        ShardedSingleRoom over an engine double — a WallsRef without frames behind the calls the wrapper and
                       _reset_from_rng make of an engine — with every rank given the same GLOBAL arguments: the slicing of index, mask and
                       the per-agent rows, the refusals every rank makes alike, and the global layouts remembered for the `rng` keyword.
"""
import types

import numpy as np
import pytest

import time_limit_ref as TL
import walls_ref as WR
from test_gpu_walls import CASES, ROOMS, make_ref, three_layouts, walls_of
from test_gpu_walls_time_limit import COLUMNS, LIMITS, REHEARSED
from test_gpu_walls_time_limit import rollout as whole_rollout

G = 16
H = W = 6
ND = 8
TOUCHED = [1, 4, 6, 11, 15]                                                  # one or two agents of every shard of four

SHARD_COLUMNS = ("restarts_after_truncation", "restarts_after_done", "goal_redraws", "goal_redraws_on_truncation_restarts")
SHARD_EVENTS = dict(ROOMS=((17, 18, 19, 18), (4, 2, 1, 4), (4, 9, 5, 5), (4, 8, 5, 2)),
                    WIDE=((23, 21, 19, 23), (1, 4, 6, 1), (3, 2, 8, 2), (3, 2, 4, 1)),
                    F64=((18, 18, 19, 18), (2, 2, 1, 2), (6, 5, 6, 5), (4, 5, 6, 4)))


def global_mask(agents=TOUCHED):
    m = np.zeros(G, np.uint8)
    m[list(agents)] = 1
    return m


# ---- (a) the references ---------------------------------------------------------------------------------------------------------
def shard_rollout(name, world, rank, check):
    """rank's shard of the rollout of tests/test_gpu_walls_time_limit.py: check(step, ref, lim) behind set_walls (step -1) and behind
    every step; returns the shard's own event counts"""
    c = CASES[name]
    L, steps = LIMITS[name]
    per = G // world
    lo, hi = rank * per, (rank + 1) * per
    walls, index = walls_of(name)
    ref = make_ref(dict(c, B=per), agent_id_offset=lo, render=False)
    ref.set_walls(walls, index[lo:hi])
    lim = TL.TimeLimitRef(ref, L, c["seed"], True)
    rng = np.random.default_rng(c["seed"] + 1)
    check(-1, ref, lim)
    on_truncation = 0
    for t in range(steps):
        a = WR.draw_actions(rng, G)                                          # the whole batch's draws: the shard takes its columns
        redraws, after_t, after_d = ref.events["goal_redraws"], lim.events["restarts_after_truncation"], lim.events["restarts_after_done"]
        lim.step(a[lo:hi])
        if lim.events["restarts_after_truncation"] > after_t and lim.events["restarts_after_done"] == after_d:
            on_truncation += ref.events["goal_redraws"] - redraws
        check(t, ref, lim)
    return dict(ref.events, **lim.events, goal_redraws_on_truncation_restarts=on_truncation)


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("name", ["ROOMS", "WIDE", "F64"])
def test_a_shard_of_the_references_is_its_slice_of_the_whole_rollout(name, world):
    assert CASES[name]["B"] == G
    snaps, actions, events = whole_rollout(name, render=False)
    assert tuple(events[k] for k in COLUMNS) == REHEARSED[name], events
    per = G // world
    counts = []
    for rank in range(world):
        lo, hi = rank * per, (rank + 1) * per

        def check(t, ref, lim):
            want, where = snaps[t + 1], f"{name}, rank {rank} of {world}, step {t}"
            bits = np.uint64 if want["position"].dtype == np.float64 else np.uint32
            assert ref.position.dtype == want["position"].dtype
            np.testing.assert_array_equal(ref.goal, want["goal"][lo:hi], err_msg=f"goal {where}")
            np.testing.assert_array_equal(ref.position.view(bits), want["position"][lo:hi].view(bits), err_msg=f"position {where}")
            np.testing.assert_array_equal(ref.direction, want["direction"][lo:hi], err_msg=f"heading {where}")
            np.testing.assert_array_equal(ref.episode, want["episode"][lo:hi], err_msg=f"episode {where}")
            np.testing.assert_array_equal(lim.episode_steps, want["episode_steps"][lo:hi], err_msg=f"episode_steps {where}")
            np.testing.assert_array_equal(lim.truncated, want["truncated"][lo:hi], err_msg=f"truncated {where}")

        counts.append(shard_rollout(name, world, rank, check))
    for k in ("restarts_after_truncation", "restarts_after_done", "goal_redraws", "truncations"):
        assert sum(c[k] for c in counts) == events[k], (k, counts, events)   # (per agent: they add up; the fourth column is per STEP and need not)
    if world == 4:
        got = tuple(tuple(c[k] for c in counts) for k in SHARD_COLUMNS)
        assert got == SHARD_EVENTS[name], got
        for c in counts:                                                     # what tests/test_gpu_sharding_features.py relies on, every offset included
            assert c["restarts_after_done"] >= 1 and c["restarts_after_truncation"] >= 17 and c["goal_redraws_on_truncation_restarts"] >= 1, c


# ---- the engine double ----------------------------------------------------------------------------------------------------------
class Double:
    """What ShardedSingleRoom and _reset_from_rng touch of an engine, over a WallsRef without frames.  The arguments are taken the way
    SingleRoom takes them (one entry per LOCAL agent, reshape and all), and every call is recorded."""

    def __init__(self, batch, agent_id_offset, device, seed=0, height_tile_map_tu=H, width_tile_map_tu=W, num_directions=ND, num_rays=64,
                 height_camera_view_pu=64, position_increment_wu=0.25, player_radius_wu=0.3, auto_reset=True):
        self.batch, self.T = batch, np.float32
        self.cfg = types.SimpleNamespace(height_tile_map_tu=height_tile_map_tu, width_tile_map_tu=width_tile_map_tu, num_directions=num_directions)
        self.ref = WR.WallsRef(batch, seed, height_tile_map_tu, width_tile_map_tu, num_rays, height_camera_view_pu, nd=num_directions,
                               inc=position_increment_wu, radius=player_radius_wu, auto_reset=auto_reset, agent_id_offset=agent_id_offset,
                               render=False)
        self.calls, self.closed = [], False

    def set_walls(self, walls, index=None, mask=None):
        self.calls.append("set_walls")
        w = np.asarray(walls)
        w = w[None] if w.ndim == 2 else w
        ix = None if index is None else np.ascontiguousarray(index, dtype=np.int32).reshape(self.batch)
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8).reshape(self.batch)
        if ix is None and len(w) not in (1, self.batch):
            raise ValueError(f"a NULL layout index needs 1 layout or one per agent ({self.batch}); got {len(w)} layouts")
        if ix is not None and ((ix < 0) | (ix >= len(w)))[np.ones(self.batch, bool) if m is None else m != 0].any():
            raise ValueError("layout index out of range")
        self.ref.set_walls(w, ix, m)

    def set_state(self, goal, pos, head, mask=None):
        self.calls.append("set_state")
        self.ref.set_state(np.asarray(goal).reshape(self.batch, 2), np.asarray(pos, self.T).reshape(self.batch, 2),
                           np.asarray(head).reshape(self.batch), mask)

    def close(self):
        self.closed = True


CFG = dict(seed=ROOMS["seed"], height_tile_map_tu=H, width_tile_map_tu=W, num_directions=ND, num_rays=ROOMS["N"],
           height_camera_view_pu=ROOMS["Hc"], position_increment_wu=0.25, player_radius_wu=0.3, auto_reset=True)


@pytest.fixture
def sharded(rcw, monkeypatch):
    """make(world): the `world` ShardedSingleRoom of a global batch of 16 over engine doubles, in one process; act_ and reset_ of
    single_room routed to the doubles until the test ends"""
    from raycastworlds_jl_amd import single_room

    monkeypatch.setattr(single_room, "act_", lambda env, a: env.ref.step(np.asarray(a, dtype=np.uint8)))
    monkeypatch.setattr(single_room, "reset_", lambda env, mask=None, seed=None: env.ref.reset(mask, seed))
    made = []

    def make(world, make_rng=None):
        """make_rng: every rank's own generator(s), in the same state (the ranks of a job are processes; here they share one)"""
        shards = [rcw.ShardedSingleRoom(G, rank=r, world=world, env_factory=Double, **dict(CFG, **({"rng": make_rng()} if make_rng else {})))
                  for r in range(world)]
        assert [(s.first, s.count) for s in shards] == [(r * G // world, G // world) for r in range(world)]
        assert [s.env.ref.offset for s in shards] == [s.first for s in shards]
        made.extend(shards)
        return shards

    yield make
    for s in made:
        s.close()
        assert s.env.closed


def whole_ref():
    return make_ref(ROOMS, render=False)


def ref_state(*refs):
    return dict(goal=np.concatenate([r.goal for r in refs]), position=np.concatenate([r.position for r in refs]).view(np.uint32),
                heading=np.concatenate([r.direction for r in refs]), episode=np.concatenate([r.episode for r in refs]),
                tile_map=np.concatenate([r.tile_map_chunks for r in refs]))


def assert_shards_equal(shards, whole, where):
    got, want = ref_state(*(s.env.ref for s in shards)), ref_state(whole)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{k} {where}")


def step_all(shards, whole, rng, steps, where):
    for t in range(steps):
        a = WR.draw_actions(rng, G)
        for s in shards:
            s.act_(s.local_slice(a))
        whole.step(a)
        assert_shards_equal(shards, whole, f"{where}: step {t}")


def sixteen_layouts(rcw):
    """16 DISTINCT layouts (layouts.maze has 3 on a 6 x 6 map): layout k has a pillar for every set bit of k, so a wrong slice shows"""
    out = np.stack([rcw.layouts.ring(H, W) for _ in range(G)])
    for k in range(G):
        for bit, (i, j) in enumerate(((1, 1), (1, 3), (3, 1), (3, 3))):
            out[k, i, j] = bool(k >> bit & 1)
    assert len({m.tobytes() for m in out}) == G
    return out


# ---- (b) set_walls on the device-generator path ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["one-layout", "three-layouts-and-an-index", "a-layout-per-global-agent"])
def test_set_walls_with_global_arguments_on_every_rank(rcw, sharded, shape):
    walls3, index = three_layouts(H, W), (np.arange(G) % 3).astype(np.int32)
    args = {"one-layout": (walls3[2],), "three-layouts-and-an-index": (walls3, index), "a-layout-per-global-agent": (sixteen_layouts(rcw),)}[shape]
    shards, whole = sharded(4), whole_ref()
    assert_shards_equal(shards, whole, "fresh")
    for s in shards:
        s.set_walls(*args)
        assert s.env.calls == ["set_walls"]
    whole.set_walls(*args)
    assert_shards_equal(shards, whole, f"behind set_walls, {shape}")
    per_agent = np.stack([whole.walls_of(b) for b in range(G)])
    want = {"one-layout": walls3[[2] * G], "three-layouts-and-an-index": walls3[index], "a-layout-per-global-agent": args[0]}[shape]
    np.testing.assert_array_equal(per_agent, want)                           # (the whole took what the call says, so the shards did)
    step_all(shards, whole, np.random.default_rng(ROOMS["seed"] + 1), 10, shape)
    assert whole.events["restarts_after_done"] + whole.events["goal_redraws"] > 0


@pytest.mark.parametrize("strays", [False, True], ids=["index-in-range", "strays-outside-the-mask"])
def test_a_masked_set_walls_with_the_global_mask(sharded, strays):
    """5 steps, then 5 of the 16 agents — one or two of every shard — get another layout: the others keep every compared word, the touched
    ones are one episode further, and 10 steps on the shards are still the whole.  `strays`: index entries outside 0..2 where the mask
    is zero, in three ranks' slices: nobody reads them, every rank accepts the call."""
    walls, index = three_layouts(H, W), (np.arange(G) % 3).astype(np.int32)
    shards, whole = sharded(4), whole_ref()
    for s in shards:
        s.set_walls(walls, index)
    whole.set_walls(walls, index)
    rng = np.random.default_rng(ROOMS["seed"] + 1)
    step_all(shards, whole, rng, 5, "behind set_walls")
    mask, other = global_mask(), ((index + 1) % 3).astype(np.int32)
    if strays:
        other[[0, 2]], other[9], other[[12, 14]] = 99, -1, (-1, 99)
        assert not mask[[0, 2, 9, 12, 14]].any()
    assert all(1 <= mask[s.first:s.first + s.count].sum() <= 2 for s in shards)
    before = ref_state(*(s.env.ref for s in shards))
    for s in shards:
        s.set_walls(walls, other, mask)
    whole.set_walls(walls, np.where(mask != 0, other, 0), mask)
    after = ref_state(*(s.env.ref for s in shards))
    keep = mask == 0
    for k in before:
        np.testing.assert_array_equal(after[k][keep], before[k][keep], err_msg=f"{k} of the untouched agents")
    np.testing.assert_array_equal(after["episode"][~keep], before["episode"][~keep] + 1)
    assert (after["tile_map"][~keep] != before["tile_map"][~keep]).any(axis=1).all()
    assert_shards_equal(shards, whole, "behind the masked set_walls")
    step_all(shards, whole, rng, 10, "behind the masked set_walls")


# ---- (c) refusals ---------------------------------------------------------------------------------------------------------------
def test_every_rank_refuses_alike_and_touches_no_engine(sharded):
    walls, index = three_layouts(H, W), (np.arange(G) % 3).astype(np.int32)
    shards = sharded(4)
    for s in shards:
        s.set_walls(walls, index)
        s.env.calls.clear()
    before = ref_state(*(s.env.ref for s in shards))
    in_rank_3 = index.copy()
    in_rank_3[15] = 3                                                        # under a set mask bit, in the last rank's slice
    bad = {"an index outside 0..2 under the mask, in rank 3's slice": (walls, in_rank_3, global_mask()),
           "the same without a mask": (walls, in_rank_3),
           "three layouts without an index": (walls,),
           "walls with four dimensions": (walls[None], index),
           "an index of 15 entries": (walls, index[:15]),
           "an index of 4 entries (a local one)": (walls, index[:4])}
    for what, args in bad.items():
        for s in shards:
            with pytest.raises(ValueError):
                s.set_walls(*args)
            assert s.env.calls == [], f"rank {s.rank} reached its engine: {what}"
    after = ref_state(*(s.env.ref for s in shards))
    for k in before:
        np.testing.assert_array_equal(after[k], before[k], err_msg=k)


# ---- (d) the rng keyword ----------------------------------------------------------------------------------------------------------
def rng_state(shards):
    refs = [s.env.ref for s in shards]
    return (np.concatenate([r.goal for r in refs]), np.concatenate([r.position for r in refs]).view(np.uint32),
            np.concatenate([r.direction for r in refs]))


@pytest.mark.parametrize("generators", ["one-global-generator", "a-generator-per-global-agent"])
def test_the_rng_keyword_remembers_the_global_layouts(rcw, sharded, generators):
    """set_walls((3, H, W), index), set_walls(four_rooms, mask), reset_(global_mask) on batches built with `rng`, at world 1, 2 and 4 from
    generators in the same state: after each call the shards' goal, pose and heading are world 1's and are reference_reset_draws from a
    twin against each GLOBAL agent's current layout, in global agent order — the layouts of the first call persist where the second did
    not touch them."""
    SR = rcw.SingleRoomModule
    one = generators == "one-global-generator"
    make_rng = (lambda: np.random.default_rng(5)) if one else (lambda: [np.random.default_rng(50 + a) for a in range(G)])
    worlds = {w: sharded(w, make_rng) for w in (1, 2, 4)}
    twin = make_rng()
    of = lambda a: twin if one else twin[a]
    want = (np.zeros((G, 2), np.int32), np.zeros((G, 2), np.float32), np.zeros(G, np.int32))

    def expect(touched, layout, construction=False):
        for a in np.flatnonzero(touched):
            if construction:
                SR.reference_reset_draws(of(a), H, W, ND)                    # SR:62-74: drawn, then overwritten by reset!(world) SR:105
            gi, gj, ti, tj, d = SR.reference_reset_draws(of(a), H, W, ND, walls=None if layout is None else layout[a])
            want[0][a], want[1][a], want[2][a] = (gi, gj), (np.float32(ti - 0.5), np.float32(tj - 0.5)), d

    def check(where, layout):
        for w, shards in worlds.items():
            got = rng_state(shards)
            for x, y, what in zip(got, rng_state(worlds[1]), ("goal", "position", "heading")):
                np.testing.assert_array_equal(x, y, err_msg=f"{what} {where}: world {w} against world 1")
            for x, y, what in zip(got, (want[0], want[1].view(np.uint32), want[2]), ("goal", "position", "heading")):
                np.testing.assert_array_equal(x, y, err_msg=f"{what} {where}: world {w} against the twin's draws")
            if layout is not None:
                assert not layout[np.arange(G), got[0][:, 0] - 1, got[0][:, 1] - 1].any(), f"a goal on a wall {where}, world {w}"
            for s in shards:
                if one:                                                      # every rank made every global agent's draws and no more
                    assert s.rng.bit_generator.state == twin.bit_generator.state, f"{where}: rank {s.rank} of {w}"
                else:                                                        # its own agents' draws and nobody else's
                    fresh = make_rng()
                    for a in range(G):
                        mine = s.first <= a < s.first + s.count
                        assert s.rng[a].bit_generator.state == (twin if mine else fresh)[a].bit_generator.state, f"{where}: rank {s.rank} of {w}, agent {a}"

    everyone = np.ones(G, bool)
    expect(everyone, None, construction=True)
    check("behind the construction", None)

    walls3, index = three_layouts(H, W), (np.arange(G) % 3).astype(np.int32)
    layout = walls3[index].copy()
    for shards in worlds.values():
        for s in shards:
            s.set_walls(walls3, index)
    expect(everyone, layout)
    check("behind set_walls with an index", layout)

    rooms, mask = rcw.layouts.four_rooms(H, W), global_mask()
    assert (walls3[index[mask != 0]] != rooms).any(axis=(1, 2)).sum() >= 3   # (the second call changes the layout of at least 3 of its 5 agents)
    layout[mask != 0] = rooms
    for shards in worlds.values():
        for s in shards:
            s.set_walls(rooms, mask=mask)
    expect(mask != 0, layout)
    check("behind the masked set_walls", layout)

    g = global_mask([0, 1, 4, 5, 10, 11, 14])                               # 1, 4, 11 took the second call's layout; 0, 5, 10, 14 kept the first's
    kept = [a for a in np.flatnonzero(g) if not mask[a]]
    assert {int(index[a]) for a in kept} == {0, 1, 2} and any(mask[a] for a in np.flatnonzero(g))
    for shards in worlds.values():
        for s in shards:
            s.reset_(global_mask=g)
    expect(g != 0, layout)
    check("behind the masked reset", layout)
