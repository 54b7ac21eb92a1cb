"""Two shards of a global batch of 66 with the guide on — ShardedSingleRoom(66, rank=r, world=2) engines, 33 agents each at
agent_id_offset = 33 r, both alive in one process and stepped in turn — against the [33 r, 33 r + 33) slice of ONE engine of 66 agents,
which tests/guide_ref.py holds to the rule: generated mazes (keyed by the GLOBAL agent id), auto_reset, half the agents following the
guide.  The guide is a function of each agent's own state, so a shard's words are its slice of the batch's."""
import numpy as np
import pytest

import guide_ref as GR

pytestmark = pytest.mark.gpu

G, WORLD, PER = 66, 2, 33
CFG = dict(seed=21, auto_reset=True, num_directions=16, position_increment_wu=0.25, player_radius_wu=0.25, height_tile_map_tu=9,
           width_tile_map_tu=11, num_rays=8, height_camera_view_pu=8, wall_generator=dict(loops=0.2), guide=True)


@pytest.mark.parametrize("T", ["Float32", "Float64"])
def test_every_shards_words_are_its_slice_of_the_batch(rcw, T):
    whole = rcw.SingleRoomModule.SingleRoom(batch=G, T=T, **CFG)
    shards = [rcw.ShardedSingleRoom(G, rank=r, world=WORLD, device=0, T=T, **CFG) for r in range(WORLD)]
    t = GR.Tracked(whole, enable=False)
    rng = np.random.default_rng(6)
    arrived = 0

    def compare(where):
        action, heading = t.check(where)
        for r, sh in enumerate(shards):
            assert (sh.first, sh.count, sh.env.guide_enabled) == (PER * r, PER, True)
            np.testing.assert_array_equal(sh.guide_action.numpy(), action[PER * r:PER * (r + 1)], err_msg=f"action, rank {r}, {where}")
            np.testing.assert_array_equal(sh.guide_heading.numpy(), heading[PER * r:PER * (r + 1)], err_msg=f"heading, rank {r}, {where}")
        return action

    action = compare("constructed")
    for step in range(80):
        a = np.where(rng.random(G) < 0.8, action, rng.integers(1, 5, G)).astype(np.uint8)
        rcw.act_(whole, a)
        for sh in shards:
            sh.act_(sh.local_slice(a))
        arrived += int(whole.world.done.sum())
        action = compare(f"step {step}")
    assert arrived > 0 and t.seen[1] > 0 and t.seen[4] > 0                     # agents reached goals and restarted on new mazes
    shards[1].set_guide(False)
    assert not shards[1].env.guide_enabled and shards[0].env.guide_enabled
    for e in [whole] + shards:
        e.close()
