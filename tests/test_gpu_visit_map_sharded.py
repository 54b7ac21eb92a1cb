"""Shards of a global batch with the visit map and its table on, all alive in one process on one GPU and stepped in turn, against ONE
engine of the whole batch, which tests/visit_map_ref.py holds to the definition: a wall bank of three layouts (drawn by the GLOBAL agent
id), auto_reset, a time limit of 7.

  * two and three UNEVEN shards of 67 agents (40 + 27, 30 + 20 + 17): engines at their agent_id_offset, what a shard is —
    ShardedSingleRoom itself cuts equal shards only;
  * ShardedSingleRoom(66, rank=r, world=2): the mirror's own methods.

The map and here / visited / first count each agent's own poses, so a shard's are its slice of the batch's.  The table is per handle:
every shard's is held to the definition on its own agents (level_here comes from the shard's OWN table and is no slice of the batch's),
and the shards' tables sum to the batch's."""
import numpy as np
import pytest

import visit_map_ref as VR
from test_gpu_frontier import pillar_layouts

pytestmark = pytest.mark.gpu


def config(rng):
    return dict(seed=23, auto_reset=True, num_directions=16, position_increment_wu=0.25, player_radius_wu=0.25, height_tile_map_tu=5,
                width_tile_map_tu=7, num_rays=8, height_camera_view_pu=8, out_of_bounds=1, max_episode_steps=7,
                wall_bank=pillar_layouts(5, 7, rng, count=3), visit_map=dict(sectors=3, table=True))


def run(rcw, rng, whole, shards, step_shard, steps=30):
    """shards: (first, count, engine-like with the visit map's properties, its SingleRoom); step_shard(k, global actions)"""
    G = whole.batch
    tracked = [VR.Tracked(e, enable=False) for e in [whole] + [s[3] for s in shards]]
    for t in tracked:
        assert (t.sectors, t.has_table, t.rows) == (3, True, 3)
        t.refilled(None, "constructed")

    def compare(where):
        total = np.zeros_like(tracked[0].table)
        for k, (first, count, sh, _) in enumerate(shards):
            part = slice(first, first + count)
            for name, got in (("map", sh.visit_map), ("here", sh.visits_here.numpy()), ("visited", sh.visited_cells.numpy()), ("first", sh.visit_first.numpy())):
                np.testing.assert_array_equal(got, getattr(tracked[0], name)[part], err_msg=f"{name}, shard {k}, {where}")
            tab = sh.visit_table()
            total += np.concatenate([tab["total"][None], tab["levels"]])
        np.testing.assert_array_equal(total, tracked[0].table, err_msg=f"the shards' tables, summed, {where}")

    compare("constructed")
    for step in range(steps):
        a = rng.integers(1, 5, G).astype(np.uint8)
        rcw.act_(whole, a)
        for k in range(len(shards)):
            step_shard(k, a)
        for t in tracked:
            t.stepped(f"step {step}")
        compare(f"step {step}")
    assert tracked[0].seen["restarts"] >= 3 * G and tracked[0].seen["shared"] > 0
    # level_here is the shard's own table's: somewhere it is less than the batch's
    own = np.concatenate([t.level_here for t in tracked[1:]])
    assert (own <= tracked[0].level_here).all() and (own < tracked[0].level_here).any()


@pytest.mark.parametrize("counts", [(40, 27), (30, 20, 17)], ids=["40+27", "30+20+17"])
def test_uneven_shards_are_slices_and_their_tables_sum_to_the_batchs(rcw, counts):
    rng = np.random.default_rng(50 + len(counts))
    cfg = config(rng)
    G = sum(counts)
    whole = rcw.SingleRoomModule.SingleRoom(batch=G, **cfg)
    firsts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    engines = [rcw.SingleRoomModule.SingleRoom(batch=int(c), agent_id_offset=int(f), **cfg) for f, c in zip(firsts, counts)]
    shards = [(int(f), int(c), e, e) for f, c, e in zip(firsts, counts, engines)]
    run(rcw, rng, whole, shards, lambda k, a: rcw.act_(engines[k], a[shards[k][0]:shards[k][0] + shards[k][1]]))
    for e in [whole] + engines:
        e.close()


def test_the_sharded_mirror(rcw):
    rng = np.random.default_rng(60)
    cfg = config(rng)
    whole = rcw.SingleRoomModule.SingleRoom(batch=66, **cfg)
    mirrors = [rcw.ShardedSingleRoom(66, rank=r, world=2, device=0, **cfg) for r in range(2)]
    shards = [(sh.first, sh.count, sh, sh.env) for sh in mirrors]
    run(rcw, rng, whole, shards, lambda k, a: mirrors[k].act_(mirrors[k].local_slice(a)))
    mirrors[0].visit_table_clear()
    assert int(mirrors[0].visit_table()["total"].sum()) == 0 and int(mirrors[1].visit_table()["total"].sum()) > 0
    assert mirrors[0].level_visits_here.numpy().any()                             # (the clear touches no per-agent word)
    mirrors[1].set_visit_map(None)
    assert not mirrors[1].env.visit_map_info["enabled"] and mirrors[0].env.visit_map_info["enabled"]
    mirrors[1].set_visit_map(sectors=2)
    assert mirrors[1].env.visit_map_info == dict(enabled=True, sectors=2, table=False, rows=0, first=0)
    for e in [whole] + mirrors:
        e.close()
