"""The start rule on the CPU (include/rcw.h, "the start rule"): tests/start_distance_ref.py — the rule restated in Python integers and a
plain queue flood — on hand-made maps, and layouts.start_rule (rcw_start_rule, host arithmetic) against it.  No device.

  (a) CORRIDOR     5 x 70, walls on rows 2 and 4: one corridor of 68 tiles.  Band (60, 65): a goal near an end has tiles in the band, a goal
                   near the middle has none and is clamped to the farthest tile.
  (b) ISLANDS      7 x 7 of isolated single cells: nothing but the goal is reached, the drawn pose stays.
  (c) TWO_ROOMS    two sealed rooms on 9 x 12, band (1, max): every start has a real distance — and WITHOUT the rule, same seeds, some have none.
  (d) FOUR_ROOMS   four_rooms(8, 8), band (3, 4).
  (e) the band's edges and every invalid band.
The last test holds, from the reference's counts, that the scenarios tests/test_gpu_start_distance.py runs reach outcomes 1, 2 and 3.
"""
import numpy as np
import pytest

import start_distance_ref as SR
import walls_ref as WR


def both(rcw, walls, goal, key, lo, hi):
    """the reference's answer, held to layouts.start_rule's"""
    want = SR.start_rule(walls, goal, key, lo, hi)
    got = rcw.layouts.start_rule(walls, goal, key, lo, None if hi == SR.MAX and key % 2 else hi)
    assert got == want, (goal, key, lo, hi, got, want)
    return want


def test_the_draw_index_meets_no_other_draw_of_the_episode_key():
    # reset!'s indices count from 0: two for the goal, two more per redraw (at most 1024 H W), one per tile try (at most 1024 H W + 1), one heading
    HW = 65280
    assert 2 + 2 * 1024 * HW + 1024 * HW + 2 < 1 << 31 < 1 << 63 < SR.START_DRAW < 1 << 64
    assert SR.START_DRAW == 0xC000000000000000 and SR.START_DRAW != 1 << 63        # the layout sources' draw


def test_corridor_band_and_clamp(rcw):
    walls = SR.corridor()
    F = SR.field(walls, (3, 2))
    assert (F >= 0).sum() == 68 and F.max() == 67 and F[2, 68] == 67 and F[0, 0] == -1
    seen = set()
    for key in range(40):
        for gj in (2, 3, 68, 69):                                               # near an end: tiles 60..65 away exist
            (i, j), outcome = both(rcw, walls, (3, gj), key, 60, 65)
            assert outcome == SR.IN_BAND and i == 3 and 60 <= abs(j - gj) <= 65
            seen.add(abs(j - gj))
        for gj in (30, 35, 40):                                                 # near the middle: the farthest tile is under 60 away
            (i, j), outcome = both(rcw, walls, (3, gj), key, 60, 65)
            D = max(gj - 2, 69 - gj)
            assert outcome == SR.CLAMPED and i == 3 and abs(j - gj) == D < 60
        (i, j), outcome = both(rcw, walls, (3, 35), key, 60, 65)                # 33 tiles to one end, 34 to the other: one farthest tile
        assert (i, j) == (3, 69)
    assert seen == set(range(60, 66))                                           # the draw reaches every distance of the band
    # ... and from (3, 36) the other end is the farthest
    assert {SR.start_rule(walls, (3, 36), k, 60, 65)[0] for k in range(20)} == {(3, 2)}


def test_isolated_cells_keep_the_drawn_pose(rcw):
    walls = SR.islands()
    for key in range(10):
        for goal in ((2, 2), (4, 6), (6, 4)):
            assert both(rcw, walls, goal, key, 1, 2) == (None, SR.KEPT)
    assert both(rcw, walls, (3, 3), 1, 1, SR.MAX) == (None, SR.KEPT)            # a goal inside a wall reaches nothing
    # the whole reference: the pose is reset_draws's
    _, band, seed = SR.MAPS["ISLANDS"]
    ref = SR.StartRef(6, seed, 7, 7, 8, 8, fresh=False, render=False)
    ref.band = band
    ref.set_walls(walls)
    for b in range(6):
        gi, gj, ti, tj, d, _ = WR.reset_draws(seed, b, 0, 7, 7, 8, walls)
        assert ref.worlds[b].goal == (gi, gj) and ref.worlds[b].pos == (np.float32(ti - 0.5), np.float32(tj - 0.5)) and ref.worlds[b].dir == d
    assert (ref.placed == SR.KEPT).all()


def test_two_sealed_rooms_every_start_reaches_the_goal(rcw):
    walls = SR.two_rooms()
    _, band, seed = SR.MAPS["TWO_ROOMS"]
    B = 67
    ruled = SR.StartRef(B, seed, 9, 12, 8, 8, fresh=False, render=False)
    ruled.band = band
    ruled.set_walls(walls)
    plain = SR.StartRef(B, seed, 9, 12, 8, 8, fresh=False, render=False)
    plain.set_walls(walls)
    assert (ruled.goal == plain.goal).all()
    assert (ruled.distance() >= 1).all() and (ruled.placed == SR.IN_BAND).all()
    assert (plain.distance() == -1).sum() >= 5, "the guarantee would be vacuous: without the rule nobody starts in the other room"
    assert (ruled.unruled_start == plain.distance()).all()
    for b in range(B):
        w = ruled.worlds[b]
        tile, outcome = both(rcw, walls, w.goal, WR.episode_key(seed, b, 0), *band)
        assert outcome == SR.IN_BAND and w.pos == (np.float32(tile[0] - 0.5), np.float32(tile[1] - 0.5))


def test_four_rooms_band(rcw):
    walls = SR.four_rooms()
    free = np.argwhere(~walls) + 1
    counts = {}
    for gi, gj in free:
        F = SR.field(walls, (gi, gj))
        for key in range(6):
            tile, outcome = both(rcw, walls, (gi, gj), key, 3, 4)
            want = SR.IN_BAND if F.max() >= 3 else SR.CLAMPED
            assert outcome == want
            d = F[tile[0] - 1, tile[1] - 1]
            assert (3 <= d <= 4) if outcome == SR.IN_BAND else d == F.max()
            counts[outcome] = counts.get(outcome, 0) + 1
    assert counts.get(SR.IN_BAND, 0) > 0


def test_the_drawn_tile_is_uniform_over_the_band_in_tile_order(rcw):
    walls = SR.ring(6, 9)
    F = SR.field(walls, (3, 4))
    lin = F.T.reshape(-1)
    E = np.flatnonzero((lin >= 2) & (lin <= 3))
    hits = np.zeros(E.size, int)
    for key in range(60 * E.size):
        (i, j), outcome = both(rcw, walls, (3, 4), WR.mix64(key), 2, 3)
        hits[np.searchsorted(E, (i - 1) + 6 * (j - 1))] += 1
    assert hits.min() > 30 and hits.max() < 95


def test_band_edges_and_invalid_bands(rcw):
    walls = SR.corridor()
    for lo, hi in ((5, 5), (1, 1), (1, 3), (67, 67), (67, SR.MAX), (1, SR.MAX), (SR.MAX, SR.MAX)):
        (i, j), outcome = both(rcw, walls, (3, 2), 7, lo, hi)
        d = j - 2
        assert (outcome == SR.IN_BAND and lo <= d <= hi) if lo <= 67 else (outcome == SR.CLAMPED and d == 67)
    assert rcw.layouts.start_rule(walls, (3, 2), 7, 1, None) == SR.start_rule(walls, (3, 2), 7, 1, SR.MAX)
    for lo, hi in ((0, 3), (-1, 3), (4, 3), (1, SR.MAX + 1), (1, 65535), (0, 0), (2 ** 31 - 1, 2 ** 31 - 1), (3, -1)):
        assert not SR.valid_band(lo, hi)
        with pytest.raises(ValueError, match="band"):
            rcw.layouts.start_rule(walls, (3, 2), 7, lo, hi)
    with pytest.raises(ValueError):
        rcw.layouts.start_rule(np.zeros((300, 300), bool), (3, 2), 7, 1, 2)     # H W > 65535
    with pytest.raises(ValueError):
        rcw.layouts.start_rule(walls[None], (3, 2), 7, 1, 2)


def scenario(name, render=False, B=67, steps=24, limit=5):
    """the rollout tests/test_gpu_start_distance.py holds the engine to: set_walls, the rule on, the limit, reset_, `steps` random steps"""
    import time_limit_ref as TL

    make_walls, band, seed = SR.MAPS[name]
    walls = make_walls()
    H, W = walls.shape
    ref = SR.StartRef(B, seed, H, W, 64, 64, render=render)
    ref.set_walls(walls)
    ref.band = band
    lim = TL.TimeLimitRef(ref, limit, seed, True)
    return ref, lim, walls


def test_the_gpu_scenarios_reach_every_outcome():
    total = {}
    for name in SR.MAPS:
        ref, lim, _ = scenario(name)
        rng = np.random.default_rng(SR.MAPS[name][2] + 1)
        ref.reset()
        lim.clear()
        for _ in range(24):
            lim.step(rng.integers(1, 5, ref.B).astype(np.uint8))
        assert lim.events["restarts_after_truncation"] + lim.events["restarts_after_done"] >= 2 * ref.B, (name, lim.events)
        total[name] = dict(ref.outcomes)
    assert total["CORRIDOR"].get(SR.IN_BAND, 0) > 0 and total["CORRIDOR"].get(SR.CLAMPED, 0) > 0, total
    assert set(total["ISLANDS"]) == {SR.KEPT}, total
    assert set(total["TWO_ROOMS"]) == {SR.IN_BAND}, total
    assert total["FOUR_ROOMS"].get(SR.IN_BAND, 0) > 0, total
