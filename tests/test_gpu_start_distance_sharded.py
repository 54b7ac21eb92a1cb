"""Shards of a global batch with the start rule on, all alive in one process on one GPU and stepped in turn, against ONE engine of the
whole batch: the rule is a function of (seed, GLOBAL agent id, episode, walls, goal, band), so a shard's poses, goals, counters, frames and
`placed` are its slice of the batch's.  Two sealed rooms, auto_reset, a time limit of 4, the band changed half-way.

  * two UNEVEN shards of 67 agents (40 + 27): engines at their agent_id_offset;
  * ShardedSingleRoom(66, rank=r, world=2): the mirror's own setter and word.
"""
import numpy as np
import pytest

import start_distance_ref as SR

pytestmark = pytest.mark.gpu

CFG = dict(seed=31, auto_reset=True, num_directions=8, position_increment_wu=0.25, player_radius_wu=0.3, height_tile_map_tu=9,
           width_tile_map_tu=12, num_rays=16, height_camera_view_pu=16, max_episode_steps=4, walls=SR.two_rooms(), start_distance=(2, 3))


def run(rcw, whole, shards, step_shard, set_band, steps=14):
    """shards: (first, count, engine-like with start_placed, its SingleRoom)"""
    G = whole.batch
    rng = np.random.default_rng(7)

    def compare(where):
        for k, (first, count, sh, env) in enumerate(shards):
            part = slice(first, first + count)
            for name, got, want in (("placed", sh.start_placed.numpy(), whole.start_placed.numpy()), ("position", env.world.player_position_wu, whole.world.player_position_wu),
                                    ("goal", env.world.goal_position, whole.world.goal_position), ("episode", env.world.episode, whole.world.episode),
                                    ("heading", env.world.player_direction_au, whole.world.player_direction_au), ("camera view", env.camera_view_host(), whole.camera_view_host())):
                np.testing.assert_array_equal(got, want[part], err_msg=f"{name}, shard {k}, {where}")

    for e in [whole] + [s[3] for s in shards]:
        rcw.reset_(e)
    compare("reset_")
    assert (whole.start_placed.numpy() == SR.IN_BAND).all()
    for step in range(steps):
        if step == steps // 2:
            whole.set_start_distance(40, 50)                                      # beyond both rooms: clamped
            set_band(40, 50)
        a = rng.integers(1, 5, G).astype(np.uint8)
        rcw.act_(whole, a)
        for k in range(len(shards)):
            step_shard(k, a)
        compare(f"step {step}")
    assert (whole.world.episode >= 4).all() and (whole.start_placed.numpy() == SR.CLAMPED).all()


def test_uneven_shards_are_slices_of_the_batch(rcw):
    counts = (40, 27)
    whole = rcw.SingleRoomModule.SingleRoom(batch=sum(counts), **CFG)
    firsts = (0, 40)
    engines = [rcw.SingleRoomModule.SingleRoom(batch=c, agent_id_offset=f, **CFG) for f, c in zip(firsts, counts)]
    shards = [(f, c, e, e) for f, c, e in zip(firsts, counts, engines)]
    run(rcw, whole, shards, lambda k, a: rcw.act_(engines[k], a[shards[k][0]:shards[k][0] + shards[k][1]]),
        lambda lo, hi: [e.set_start_distance(lo, hi) for e in engines])
    for e in [whole] + engines:
        e.close()


def test_the_sharded_mirror(rcw):
    whole = rcw.SingleRoomModule.SingleRoom(batch=66, **CFG)
    mirrors = [rcw.ShardedSingleRoom(66, rank=r, world=2, device=0, **CFG) for r in range(2)]
    assert all(m.start_distance_info == dict(enabled=True, lo=2, hi=3) for m in mirrors)
    shards = [(sh.first, sh.count, sh, sh.env) for sh in mirrors]
    run(rcw, whole, shards, lambda k, a: mirrors[k].act_(mirrors[k].local_slice(a)), lambda lo, hi: [m.set_start_distance(lo, hi) for m in mirrors])
    mirrors[1].set_start_distance(None)
    assert not mirrors[1].start_distance_info["enabled"] and mirrors[0].start_distance_info["enabled"]
    for e in [whole] + mirrors:
        e.close()
    with pytest.raises(ValueError, match="rng"):
        rcw.ShardedSingleRoom(4, rank=0, world=2, device=0, rng=np.random.default_rng(0), start_distance=(1, 2))
