"""Two shards of a global batch of 66 with the frontier on — ShardedSingleRoom(66, rank=r, world=2) engines, 33 agents each at
agent_id_offset = 33 r, both alive in one process and stepped in turn — against the [33 r, 33 r + 33) slice of ONE engine of 66 agents,
which tests/frontier_ref.py holds to the flood and the rule: generated mazes (keyed by the GLOBAL agent id), auto_reset, most of the agents
following explore_action.  The frontier is a function of each agent's own seen map and pose, so a shard's arrays are its slice of the
batch's."""
import numpy as np
import pytest

import frontier_ref as FR

pytestmark = pytest.mark.gpu

G, WORLD, PER = 66, 2, 33
CFG = dict(seed=21, auto_reset=True, num_directions=16, position_increment_wu=0.25, player_radius_wu=0.25, height_tile_map_tu=9,
           width_tile_map_tu=11, num_rays=8, height_camera_view_pu=8, wall_generator=dict(loops=0.2), frontier=True)


@pytest.mark.parametrize("T", ["Float32", "Float64"])
def test_every_shards_arrays_are_their_slice_of_the_batch(rcw, T):
    whole = rcw.SingleRoomModule.SingleRoom(batch=G, T=T, **CFG)
    shards = [rcw.ShardedSingleRoom(G, rank=r, world=WORLD, device=0, T=T, **CFG) for r in range(WORLD)]
    t = FR.Tracked(whole, enable=False)
    rng = np.random.default_rng(6)
    arrived = 0

    def compare(where, stepped):
        exp = t.check(where, stepped=stepped)
        for r, sh in enumerate(shards):
            assert (sh.first, sh.count, sh.env.frontier_enabled) == (PER * r, PER, True)
            part = slice(PER * r, PER * (r + 1))
            for name, got in (("distance", sh.frontier_distance.numpy()), ("tiles", sh.frontier_tiles.numpy()), ("action", sh.explore_action.numpy()),
                              ("heading", sh.explore_heading.numpy()), ("field", sh.frontier_field)):
                np.testing.assert_array_equal(got, exp[name][part], err_msg=f"{name}, rank {r}, {where}")
        return exp["action"]

    action = compare("constructed", False)
    for step in range(60):
        a = np.where(rng.random(G) < 0.8, action, rng.integers(1, 5, G)).astype(np.uint8)
        rcw.act_(whole, a)
        for sh in shards:
            sh.act_(sh.local_slice(a))
        arrived += int(whole.world.done.sum())
        action = compare(f"step {step}", True)
    assert t.seen["kept"] > 0 and t.seen["flooded"] > 0 and t.seen["forward"] > 0, t.seen
    shards[1].set_frontier(False)
    assert not shards[1].env.frontier_enabled and shards[0].env.frontier_enabled
    for e in [whole] + shards:
        e.close()
