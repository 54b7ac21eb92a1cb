"""Differential fuzzing in the suite: tools/fuzz_parity.py over 120 random configurations with a
fixed seed (map size, columns, headings, field of view, radius, step, camera/image heights, Float32
and Float64 world units, the unpinned switches, both BoundsError policies, auto-reset, top view)."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_random_configurations_stay_in_parity():
    res = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tools", "fuzz_parity.py"), "120", "2025"],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert "120 random configurations" in res.stdout and ", 0 mismatches" in res.stdout


def test_random_flat_kernel_geometries_stay_in_parity():
    """The same over the geometries only the flat kernels take: top views at 9..60 pixels a tile (two-kernel form asked
    for) and camera heights anywhere from 24 rows."""
    res = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tools", "fuzz_parity.py"), "80", "77", "flat"],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert "80 random configurations" in res.stdout and ", 0 mismatches" in res.stdout


def test_random_time_limits_stay_in_parity():
    """tools/fuzz_parity.py limit: the geometries of the one-launch step (asked for in every case; maps of 3 x 3 to 40 x 40 tiles, 1 to 1,500
    view columns, 64 to 512 rows, 1 to 17 agents) with a time limit of 1, 2, 3, 7 or 20 steps, with and without auto_reset, under both
    BoundsError policies: the *_limit_kernel twins against tests/time_limit_ref.py over the oracle, episode_steps and truncated included.
    (Seed 31: 21 of the 24 take the one-launch step; 1660 truncations, 358 restarts after a truncation, 3 moves that raised with a counter.)"""
    res = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tools", "fuzz_parity.py"), "24", "31", "limit"],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert "24 random configurations" in res.stdout and ", 0 mismatches" in res.stdout
    closing = res.stdout.strip().splitlines()[-1]
    events = {k: int(v) for v, k in re.findall(r"(\d+) (truncations|restarts_after_truncation)\b", closing)}
    assert events["truncations"] > 0 and events["restarts_after_truncation"] > 0, closing


def test_random_goal_distances_stay_in_parity():
    """tools/fuzz_parity.py goal: maps of 3 x 4 to 48 x 48 tiles and one in six of 64 to 140 on a side, the ring / four rooms / a maze /
    pillars / the serpentine per agent or shared, 1 to 17 agents (1 to 4 on the maps of 64 and more on a side: the reference's Python floods
    are the cost, and agents are cut before the map size), Float32 and Float64, both forms of the step, auto_reset on and off, a
    time limit of 0, 2, 5 or 20; 30 random calls each (steps, masked and full resets, masked set_state and set_walls, the feature off and
    on), the three words and every agent's field against tests/goal_distance_ref.py after every call.
    (Seed 54: 88 floods behind a step, 63 agent-steps at distance -1, 336 steps, 70 full and 86 masked resets, 72 set_state, 81 set_walls, 75 times off
    and on, the widest level 177 tiles, 4 of the 24 maps with H W a multiple of 32, 8 configurations with the one-launch step.)"""
    res = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tools", "fuzz_parity.py"), "24", "54", "goal"],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert "24 random configurations" in res.stdout and ", 0 mismatches" in res.stdout
    closing = res.stdout.strip().splitlines()[-1]
    print(closing)
    totals = {k: int(v) for v, k in re.findall(r"(\d+) ([a-z_0-9]+)\b", closing[closing.index("goal distance:"):closing.rindex(")")])}
    assert set(totals) == {"floods_behind_a_step", "agent_steps_at_distance_minus_1", "step", "reset", "masked_reset", "set_state", "set_walls", "off_and_on",
                           "widest_level", "tiles_multiple_of_32", "tiles_not_multiple_of_32", "one_launch_steps", "two_launch_steps"}, closing
    assert all(v > 0 for v in totals.values()), closing
    assert totals["widest_level"] > 64, closing


def test_random_sequences_of_api_calls_stay_in_parity():
    """tools/api_fuzz.py: 12 handles x 50 random calls — steps with host / device / scalar actions, masked and full resets,
    injected states, rejected actions, another stream, another output buffer, another top-view form, another form of the step (one launch / two), stand-alone
    re-renders, rays, descriptor expansion, profiling — every observable compared with the oracle after every call."""
    res = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tools", "api_fuzz.py"), "12", "5", "50"],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert "12 runs x 50 calls, every observable equal" in res.stdout


def test_random_sequences_with_the_rccl_gather_stay_in_parity():
    """The same behind ShardedSingleRoom in a one-rank "nccl" group with the collective forced: the observation gather —
    torch.distributed and the library's own ncclAllGather, columns + expansion and frames — between the other calls
    (another stream, another output buffer, resets ...)."""
    res = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tools", "api_fuzz.py"), "8", "9", "40", "sharded"],
                         capture_output=True, text=True, timeout=600, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert "8 runs x 40 calls, every observable equal" in res.stdout and "gather_obs_abi" in res.stdout
