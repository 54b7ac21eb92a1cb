"""Episode statistics (include/rcw.h, "episode statistics") on the CPU: hand-written traces through tests/episode_stats_ref.py with LITERAL
expected words and table entries, the SPL arithmetic on literal cases, the rehearsal of the GPU tests' wall-bank scenario on
tests/wall_bank_ref.py — whose counts tests/test_gpu_episode_stats.py quotes —, and the exports: the header declares the seven, the
library refuses a NULL handle in each.  The export checks fail on a build without the feature.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import episode_stats_ref as ES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("rcw_set_episode_stats", "rcw_episode_stats_info", "rcw_episode_stats", "rcw_episode_stats_device_ptr", "rcw_episode_stats_table",
           "rcw_episode_stats_table_device_ptr", "rcw_episode_stats_clear")


def P(*xy):
    """positions (B, 2) in Float32 from x0, y0, x1, y1, ..."""
    return np.array(xy, np.float32).reshape(-1, 2)


def one(rows=0, first=0, inc=0.125, pos=(1.5, 1.5), episode=1):
    r = ES.EpisodeStatsRef(1, rows, first, inc)
    r.begin(None, P(*pos), [episode])
    return r


def words(r, a=0):
    return tuple(int(getattr(r, w)[a]) for w in ES.WORDS)


# ---- hand-written traces ---------------------------------------------------------------------------------------------------------------
def test_an_agent_that_succeeds():
    """three calls: a move, a turn (the position keeps its bits), the move that reaches the goal; l = 1"""
    r = one()
    assert words(r) == (0, 0, 0, 0, -1, -1, 0)
    r.step(P(1.625, 1.5), [0], [0], [1], start_distance=[1])
    assert words(r) == (0, 0, 1, 1, -1, -1, 0)
    r.step(P(1.625, 1.5), [0], [0], [1], start_distance=[1])
    assert words(r) == (0, 0, 2, 1, -1, -1, 0)
    r.step(P(1.75, 1.5), [1], [0], [1], start_distance=[1])
    # finished, success, length 3, moves 2, no layout source, p = 2 / 8 < l = 1: SPL 1.0, the first episode
    assert words(r) == (1, 1, 3, 2, -1, 65536, 1)
    assert r.table.tolist() == [[1, 1, 0, 3, 2, 1, 65536, 0]]


def test_one_that_truncates_and_is_restarted():
    """a limit of 2: the second call truncates; the third restarts (the counter moved) and does not count; then the new record lives"""
    r = one(rows=2, first=0)
    r.step(P(1.5, 1.5), [0], [0], [1], layout=[1], start_distance=[4])       # blocked: no move
    r.step(P(1.5, 1.625), [0], [1], [1], layout=[1], start_distance=[4])
    assert words(r) == (1, 2, 2, 1, 1, 0, 1)                                 # truncated with SPL defined: 0
    assert r.table.tolist() == [[1, 0, 1, 2, 1, 1, 0, 0], [0] * 8, [1, 0, 1, 2, 1, 1, 0, 0]]
    r.step(P(2.5, 2.5), [0], [0], [2], layout=[0], start_distance=[2])       # the restarting call: BEGIN, and the next episode's layout
    assert words(r) == (0, 0, 0, 0, -1, -1, 1)
    r.step(P(2.625, 2.5), [0], [0], [2], layout=[0], start_distance=[2])
    assert words(r) == (0, 0, 1, 1, -1, -1, 1)
    r.step(P(2.75, 2.5), [1], [1], [2], layout=[0], start_distance=[2])      # done wins where both are set
    assert words(r) == (1, 1, 2, 2, 0, 65536, 2)
    assert r.table.tolist() == [[2, 1, 1, 4, 3, 2, 65536, 0], [1, 1, 0, 2, 2, 1, 65536, 0], [1, 0, 1, 2, 1, 1, 0, 0]]
    assert r.events["restarts_after_truncation"] == 1 and r.events["closes_per_row"].tolist() == [2, 1, 1]


def test_one_frozen_without_auto_reset_walks_on():
    r = one()
    r.step(P(1.625, 1.5), [1], [0], [1])
    assert words(r) == (1, 1, 1, 1, -1, -1, 1)                               # goal distance off: SPL undefined, not counted
    assert r.table.tolist() == [[1, 1, 0, 1, 1, 0, 0, 0]]
    for k in range(3):                                                       # done stays set, the agent walks: nothing is recorded again
        r.step(P(1.75 + k / 8, 1.5), [1], [0], [1])
        assert words(r) == (0, 1, 1, 1, -1, -1, 1)
    assert r.table.tolist() == [[1, 1, 0, 1, 1, 0, 0, 0]] and r.events["frozen_calls"] == 3
    r.begin([1], P(1.5, 1.5), [2])                                           # a reset: a new record
    assert words(r) == (0, 0, 0, 0, -1, -1, 1)


def test_one_reset_by_mask_in_the_middle_of_an_episode_is_dropped():
    """two agents; the mask takes the first in the middle of its episode: its record is dropped, `episodes` and the table do not move; the
    second keeps every word but `finished`"""
    r = ES.EpisodeStatsRef(2, 0, 0, 0.125)
    r.begin(None, P(1.5, 1.5, 2.5, 2.5), [1, 1])
    r.step(P(1.625, 1.5, 2.625, 2.5), [0, 1], [0, 0], [1, 1])
    assert words(r, 0) == (0, 0, 1, 1, -1, -1, 0) and words(r, 1) == (1, 1, 1, 1, -1, -1, 1)
    r.begin([1, 0], P(3.5, 3.5, 2.625, 2.5), [2, 1])
    assert words(r, 0) == (0, 0, 0, 0, -1, -1, 0) and words(r, 1) == (0, 1, 1, 1, -1, -1, 1)
    assert r.table.tolist() == [[1, 1, 0, 1, 1, 0, 0, 0]] and r.events["dropped_by_mask"] == 1
    r.step(P(3.5, 3.5, 2.75, 2.5), [0, 1], [0, 0], [2, 1])                   # the first counts from the reset's position: no move
    assert words(r, 0) == (0, 0, 1, 0, -1, -1, 0) and words(r, 1) == (0, 1, 1, 1, -1, -1, 1)


def test_a_level_outside_the_rows_reaches_row_0_alone():
    r = one(rows=3, first=7)
    r.step(P(1.625, 1.5), [1], [0], [1], layout=[10], start_distance=[1])     # k = 3: one past the last row
    assert words(r) == (1, 1, 1, 1, 10, 65536, 1)
    assert r.table.tolist() == [[1, 1, 0, 1, 1, 1, 65536, 0]] + [[0] * 8] * 3
    r.begin(None, P(1.5, 1.5), [2])
    r.step(P(1.5, 1.5), [0], [1], [2], layout=[9], start_distance=[-1])       # k = 2: the last row; unreachable goal: SPL undefined
    assert words(r) == (1, 2, 1, 0, 9, -1, 2)
    assert r.table.tolist() == [[2, 1, 1, 2, 1, 1, 65536, 0], [0] * 8, [0] * 8, [1, 0, 1, 1, 0, 0, 0, 0]]
    r.begin(None, P(1.5, 1.5), [3])
    r.step(P(1.5, 1.5), [0], [1], [3], layout=[6])                           # k = -1: below the first
    assert r.table[1:, 0].tolist() == [0, 0, 1] and int(r.table[0, 0]) == 3 and r.events["closes_outside_the_rows"] == 2
    r.clear()
    assert not r.table.any() and words(r) == (1, 2, 1, 0, 6, -1, 3)           # clear touches no per-agent word


def test_a_negative_zero_is_a_move_and_a_nan_is_not():
    """the position is compared as a bit pattern"""
    r = one(pos=(0.0, 1.5))
    r.step(np.array([[-0.0, 1.5]], np.float32), [0], [0], [1])
    assert words(r)[2:4] == (1, 1)
    nan = np.array([[np.nan, 1.5]], np.float32)
    r.step(nan, [0], [0], [1])
    r.step(nan.copy(), [0], [0], [1])
    assert words(r)[2:4] == (3, 2)


# ---- the SPL word --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l,moves,inc,want", [(3, 24, 0.125, 65536), (3, 32, 0.125, 49152), (3, 20, 0.125, 65536),
                                              (3, 30, float(np.float32(0.1)), 65535), (1, 0, 0.125, 65536), (2, 2 ** 32 - 1, 0.25, 0)])
def test_the_spl_word_on_literal_cases(l, moves, inc, want):
    """l 3 over 24 moves of 1/8: the shortest path, 65536; 32 moves: 3/4; 20 moves: p < l, 65536.  inc = 0.1f widens to
    13421773 / 134217728: 30 moves are p = 3.0000000447..., just over l, and 196608 / p = 65535.99902...: 65535.  The longest path a
    UInt32 counts: 131072 / 1073741823.75 floors to 0."""
    assert ES.spl_q16(moves, inc, l) == want


def test_spl_is_undefined_without_a_distance_and_not_counted():
    for sd in ([-1], [0], None):                                             # unreachable, on the goal at the start, goal distance off
        r = one()
        r.step(P(1.625, 1.5), [1], [0], [1], start_distance=sd)
        assert words(r)[5] == -1 and r.table[0].tolist() == [1, 1, 0, 1, 1, 0, 0, 0] and r.events["spl_defined"] == 0
    r = one(inc=float(np.float32(0.1)))
    for k in range(29):
        r.step(P(1.5 + (k + 1) / 8, 1.5), [0], [0], [1], start_distance=[3])
    r.step(P(9.0, 1.5), [1], [0], [1], start_distance=[3])
    assert words(r) == (1, 1, 30, 30, -1, 65535, 1) and r.table[0].tolist() == [1, 1, 0, 30, 30, 1, 65535, 0]


# ---- the GPU tests' wall-bank scenario, rehearsed ----------------------------------------------------------------------------------------
def test_the_bank_scenario_reaches_what_the_gpu_test_claims():
    import episode_stats_cases as EC

    ref, events = EC.rehearse_bank()
    assert tuple(int(v) for v in events["closes_per_row"]) == EC.BANK_REHEARSED["closes_per_row"]
    assert (events["successes"], events["truncations"], events["spl_defined"]) == EC.BANK_REHEARSED["successes_truncations_spl"]
    t = ref.table
    assert not t[2].any() and (t[0] == t[1:].sum(axis=0)).all()
    for row in (1, 3):
        assert t[row, 1] >= 1 and t[row, 2] >= 1 and t[row, 6] > 0              # a success with SPL defined and a truncation


# ---- the exports ---------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_seven_exports_and_the_constants():
    text = open(os.path.join(ROOT, "include", "rcw.h")).read()
    declared = set(re.findall(r"RCW_API\s+int\s+(rcw_\w+)\s*\(", text))
    assert set(EXPORTS) <= declared, sorted(set(EXPORTS) - declared)
    for name, value in (("RCW_EPISODE_OPEN", 0), ("RCW_EPISODE_SUCCESS", 1), ("RCW_EPISODE_TRUNCATED", 2), ("RCW_EPISODE_STATS_ROW_WORDS", 8),
                        ("RCW_EPISODE_STATS_MAX_ROWS", 65536)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", text), name


def test_each_export_refuses_a_null_handle(rcw):
    from raycastworlds_jl_amd import _capi

    lib = _capi.load()
    for name in EXPORTS:
        sig = _capi.SIGNATURES[name]
        args = [None] + [None if (t is C.c_void_p or hasattr(t, "contents")) else t(1) for t in sig[1:]]
        rc = getattr(lib, name)(*args)
        assert rc == _capi.RCW_ERR_INVALID_ARGUMENT, (name, rc)
        assert _capi.last_error(lib), name
