"""The state archive of a sharded batch (raycastworlds.jl_amd/sharded.py): every shard has its own archive and rows are local.  Two shards of
a global batch of 66 — ShardedSingleRoom(66, rank=r, world=2), both handles alive in one process and stepped in turn — rewind with every
feature on (tests/snapshot_cases.py), and each shard's records are the [33 r, 33 r + 33) slice of the unsharded engine's rewind: the layouts
the restarted episodes draw are keyed by the GLOBAL agent id and the restored episode counter."""
import numpy as np
import pytest

import snapshot_cases as SC

pytestmark = pytest.mark.gpu

G, WORLD, PER = 66, 2, 33
T1, T2 = 9, 12


def rewind(rcw, env, acts, save, restore):
    for a in acts[:T1]:
        rcw.act_(env, a)
    save()
    at_save = SC.record(env)
    first = SC.play(rcw, env, acts[T1:])
    restore()
    return at_save, first, SC.record(env), SC.play(rcw, env, acts[T1:])


@pytest.mark.parametrize("form", ["two-launches", "one-launch"])
def test_two_shards_rewind_as_their_slices_of_the_whole_batch(rcw, form):
    c = SC.ODD
    acts = SC.actions(G, T1 + T2, seed=21)
    rows = np.random.default_rng(4).permutation(PER + 3)[:PER].astype(np.int32)       # LOCAL rows, the same on both shards
    whole = SC.make(rcw, G, c, form=form, rows=G)
    w_save, w_first, w_back, w_second = rewind(rcw, whole, acts, whole.snapshot_save, whole.snapshot_restore)
    ev = SC.window_events(w_first, w_save)
    assert ev["goal_restarts"] > 0 and ev["truncations"] > 0 and ev["layout_changes"] > 0, ev
    SC.assert_same(w_back, w_save, "the whole batch behind its restore")
    whole.close()
    for r in range(WORLD):
        sh = rcw.ShardedSingleRoom(G, rank=r, world=WORLD, device=0, **SC.keywords(c))
        assert (sh.first, sh.count, sh.env.cfg.agent_id_offset) == (PER * r, PER, PER * r)
        SC.configure(sh.env, c, form)
        sh.set_snapshots(PER + 3)
        mine = [np.ascontiguousarray(a[sh.first:sh.first + PER]) for a in acts]
        s_save, s_first, s_back, s_second = rewind(rcw, sh.env, mine, lambda: sh.snapshot_save(rows), lambda: sh.snapshot_restore(rows))
        agents = np.arange(PER)
        source = agents + PER * r
        SC.assert_same(s_save, w_save, f"rank {r} at the save", agents=agents, source=source)
        SC.assert_same(s_back, w_save, f"rank {r} behind the restore", agents=agents, source=source)
        for k in range(T2):
            SC.assert_same(s_first[k], w_first[k], f"rank {r}, step {k}", agents=agents, source=source)
            SC.assert_same(s_second[k], w_second[k], f"rank {r}, replayed step {k}", agents=agents, source=source)
            np.testing.assert_array_equal(s_second[k]["table"], s_first[k]["table"], err_msg=f"rank {r}, replayed step {k}: the table's change")
        sh.close()
