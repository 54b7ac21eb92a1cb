"""The wall bank's specification (tests/wall_bank_ref.py) anchored on the CPU: the index rule by hand, a zero weight, the draw at index 2^63
beside the reset's own draws, sharding, the composition with the time limit — and a rehearsal, without frames, of every scenario the GPU
tests play (tests/wall_bank_cases.py), asserting from the reference's own counts that each reaches what it claims:

    scenario             episode_starts  layout_changed  layout_kept  goal_redraws  restarts_after_done  restarts_after_truncation
    small                472             265             140          64            31                   374
    square_one            27               0              18           3             0                    18     (one layout: nothing to change)
    square_zero_weight    27               0              18           3             0                    18     (one layout of weight > 0)
    big                   64              40               8          43             0                    48     (33 x 33, limit 3: nobody arrives)
    f64                   30              18               2          18             1                    19
    features              50              18              16          10             2                    32
    calls                 81              29              20          26             5                    52
    edge                   9               3               3           6             2                     4     (255 x 254, the largest map: two agents are
                                                                                                                  walked into their goals)
"""
import numpy as np
import pytest

import time_limit_ref as TL
import wall_bank_cases as C
import wall_bank_ref as WB
import walls_ref as WR

COLUMNS = ("episode_starts", "layout_changed", "layout_kept", "goal_redraws", "restarts_after_done", "restarts_after_truncation")
REHEARSED = dict(small=(472, 265, 140, 64, 31, 374), square_one=(27, 0, 18, 3, 0, 18), square_zero_weight=(27, 0, 18, 3, 0, 18),
                 big=(64, 40, 8, 43, 0, 48), f64=(30, 18, 2, 18, 1, 19), features=(50, 18, 16, 10, 2, 32), calls=(81, 29, 20, 26, 5, 52),
                 edge=(9, 3, 3, 6, 2, 4))
ALL_FOUR = ("small", "f64", "features", "calls", "edge")    # at least one layout_changed, layout_kept, goal_redraws, and restarts of both kinds


def test_the_index_rule_by_hand():
    """weights (2, 0, 3): cum = (2, 2, 5).  r = 0, 1 -> 0; r = 2, 3, 4 -> 2; layout 1 (cum[1] = cum[0]) is never the SMALLEST index"""
    cum = WB.cumulative([2, 0, 3], 3)
    assert cum == [2, 2, 5]
    assert [WB.index_of(r, cum) for r in range(5)] == [0, 0, 2, 2, 2]
    for k in (0, 2):                                                         # the boundaries r = cum[k] - 1 and r = cum[k]
        assert WB.index_of(cum[k] - 1, cum) == k
        if cum[k] < cum[-1]:
            assert WB.index_of(cum[k], cum) > k
    assert WB.cumulative(None, 4) == [1, 2, 3, 4]
    assert WB.cumulative([0xFFFFFFFF, 0], 2)[-1] == 0xFFFFFFFF
    for bad in ([0, 0], [0xFFFFFFFF, 1]):
        with pytest.raises(ValueError):
            WB.cumulative(bad, 2)


def test_the_scaled_draw_covers_the_range_and_nothing_else():
    """below(u, s) for the extreme draws: u = 0 -> 0, u = 2^64 - 1 -> s - 1, also at s = 2^32 - 1"""
    for s in (1, 5, 0xFFFFFFFF):
        assert WR.below(0, s) == 0 and WR.below((1 << 64) - 1, s) == s - 1


def test_a_zero_weight_layout_is_never_drawn():
    """4,000 (agent, episode) keys under seed 31, weights (1, 0, 3): layout 1 never, layout 2 in 2,990 of them (0.75 +- 0.03)"""
    cum = WB.cumulative([1, 0, 3], 3)
    counts = [0, 0, 0]
    for g in range(200):
        for e in range(20):
            counts[WB.layout_draw(31, g, e, cum)] += 1
    assert counts[1] == 0 and sum(counts) == 4000
    assert abs(counts[2] / 4000 - 0.75) < 0.03
    assert counts == [1010, 0, 2990], counts


def test_a_bank_of_the_ring_is_the_plain_reference():
    """L = 1 on a ring bank: the draw at index 2^63 leaves every draw of the reset alone — WallBankRef equals WallsRef reset once more, byte
    for byte, over a rollout (the install is one more reset with the same seed)"""
    c = dict(C.CALLS, B=8)
    bank, plain = C.make_ref(c), WR.WallsRef(c["B"], c["seed"], c["H"], c["W"], c["N"], c["Hc"])
    ring = C.three_layouts(6, 6)[:1]
    bank.set_wall_bank(ring)
    plain.reset()
    rng = np.random.default_rng(3)
    for t in range(25):
        a = WR.draw_actions(rng, c["B"])
        bank.step(a); plain.step(a)
        sb, sp = bank.snapshot(), plain.snapshot()
        assert not sb.pop("wall_layout").any()
        for k in sp:
            np.testing.assert_array_equal(sb[k], sp[k], err_msg=f"{k}, step {t}")
    assert bank.events["restarts_after_done"] >= 1 and bank.events["episode_starts"] > c["B"]


def test_two_shards_equal_the_halves_of_one():
    c = dict(C.CALLS, B=12)
    bank, weights = C.three_layouts(6, 6), np.array([1, 2, 1], np.uint32)
    whole = C.make_ref(c, render=False)
    halves = [C.make_ref(dict(c, B=6), render=False, agent_id_offset=o) for o in (0, 6)]
    for r in [whole] + halves:
        r.set_wall_bank(bank, weights)
    rng = np.random.default_rng(8)
    for t in range(30):
        a = WR.draw_actions(rng, 12)
        whole.step(a); halves[0].step(a[:6]); halves[1].step(a[6:])
        w = whole.snapshot()
        for h, sl in zip(halves, (slice(0, 6), slice(6, 12))):
            s = h.snapshot()
            for k in ("wall_layout", "episode", "goal", "position", "direction", "done", "tile_map_chunks"):
                np.testing.assert_array_equal(s[k], w[k][sl], err_msg=f"{k}, step {t}")
    assert whole.events["layout_changed"] > 0 and whole.events["restarts_after_done"] > 0


def test_the_time_limit_composes_over_the_bank():
    """TimeLimitRef(WallBankRef(...), L, seed, True): a truncated agent restarts through reset(mask, seed) — the same override, the same key —
    and the counter moves once a restart"""
    c = dict(C.CALLS, B=8)
    ref = C.make_ref(c, render=False)
    ref.set_wall_bank(C.three_layouts(6, 6))
    lim = TL.TimeLimitRef(ref, 3, c["seed"], True)
    rng = np.random.default_rng(2)
    for _ in range(12):
        ep0, starts0 = ref.episode.copy(), ref.events["episode_starts"]
        lim.step(WR.draw_actions(rng, c["B"]))
        moved = ref.episode - ep0
        assert set(moved.tolist()) <= {0, 1} and int(moved.sum()) == ref.events["episode_starts"] - starts0
        for b in np.flatnonzero(moved):
            k = WB.layout_draw(c["seed"], int(b), int(ep0[b]), ref.cum)
            assert ref.wall_layout[b] == k
            np.testing.assert_array_equal(ref.walls_of(b), ref.bank[k])
    assert lim.events["restarts_after_truncation"] > 0


def test_set_state_and_new_weights_touch_no_layout():
    c = dict(C.CALLS, B=6)
    ref = C.make_ref(c, render=False)
    ref.set_wall_bank(C.three_layouts(6, 6))
    before = (ref.wall_layout.copy(), ref.episode.copy(), ref.tile_map_chunks.copy())
    ref.set_weights([0, 0, 1])
    for got, want in zip((ref.wall_layout, ref.episode, ref.tile_map_chunks), before):
        np.testing.assert_array_equal(got, want)
    ref.reset()
    assert (ref.wall_layout == 2).all()
    with pytest.raises(RuntimeError):
        ref.set_walls(C.three_layouts(6, 6)[0])
    ref.set_wall_bank(None)
    ref.set_walls(C.three_layouts(6, 6)[0])


@pytest.mark.parametrize("name", sorted(C.SCENARIOS))
def test_every_gpu_scenario_reaches_what_it_claims(name):
    snaps, ev = C.recorded(name, False)
    assert tuple(ev[k] for k in COLUMNS) == REHEARSED[name], {k: ev[k] for k in COLUMNS}
    if name in ALL_FOUR:
        assert all(ev[k] > 0 for k in COLUMNS), ev
    if name == "square_one":
        assert ev["layouts_drawn"] == {0}
    if name == "square_zero_weight":
        assert ev["layouts_drawn"] == {1}                                    # (layout 0 has weight 0)
    if name == "big":
        assert max(ev["layouts_drawn"]) >= 64 and len(ev["layouts_drawn"]) >= 10 and ev["layout_kept"] > 0
    if name == "edge":
        c = C.EDGE
        assert c["H"] * c["W"] + 2 * c["H"] == 65280 and snaps[0]["tile_map_chunks"].shape[1] * 2 == 4050     # no larger map is accepted
        assert ev["layouts_drawn"] == {0, 2}                                 # (layout 1 has weight 0)
    if name == "calls":
        assert [s["bank"] for s in snaps].count(False) > 5 and snaps[-1]["bank"]
    ep = np.stack([s["episode"] for s in snaps]).astype(np.int64)
    assert set(np.diff(ep, axis=0).ravel().tolist()) <= {0, 1}              # the counter moves once a call at most
