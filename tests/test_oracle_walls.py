"""The C oracle's interior walls (oracle/rcw_oracle.c: orc_set_walls, the goal redraw of reset!(world), the masked steps) pinned to the
reference that the walled GPU tests already trust: tests/walls_ref.py's WallsRef — B `pyref.World`s, the generator in Python integers.

The C-side run equals WallsRef BYTE FOR BYTE after every call — tile-map chunks, goal, position (as bits), heading, reward, done, episode,
status, the column descriptors, the camera view, the top view — in the four rollouts of tests/test_gpu_walls.py at their own shapes
(their snapshots are computed once, by that module's `rollout`), in a masked-set_walls sequence on a 5 x 7 map (2-bit fields across the
word boundaries) and on the 6 x 6 one, in Float32 and Float64, auto_reset on and off.  Each of the four rollouts reaches a goal redraw,
a ray that ends on an interior wall, a move blocked beside one and a restart — asserted from WallsRef.events alone — and the fast
reference's own bookkeeping (tests/walled_oracle.py) counts the same numbers.

The refusals of rcw_dev_validate_walls are the oracle's, and leave it untouched.  The sanitizer run is a stand-alone program
(oracle/san_walls_main.c, `make -C oracle san-walls`): nothing here loads a sanitizer's runtime into Python.
"""
import os
import subprocess

import numpy as np
import pytest

import test_gpu_walls as GW
import walled_oracle as WO
import walls_ref as WR
from test_walls_spec import validate  # noqa: F401  (the fixture: rcw_dev_validate_walls of the development build)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS = ("tile_map_chunks", "goal", "position", "direction", "reward", "done", "episode", "status", "col_height", "col_colour", "camera_view")


def assert_snapshots_equal(got, want, where, keys=ARRAYS):
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape, where)
        if g.dtype.kind == "f":
            bits = np.uint64 if g.dtype == np.float64 else np.uint32
            g, w = g.view(bits), w.view(bits)
        np.testing.assert_array_equal(g, w, err_msg=f"{k} {where}")


@pytest.mark.parametrize("name", list(GW.CASES))
def test_the_four_rollouts_equal_the_reference_worlds_after_every_call(rcw, oracle, name):
    c = GW.CASES[name]
    snaps, actions, events = GW.rollout(name)
    assert all(events[k] > 0 for k in GW.ALL), events                        # (WallsRef's counts alone)
    walls, index = GW.walls_of(name)
    orc = WO.from_case(c)
    orc.set_walls(walls, index)
    np.testing.assert_array_equal(orc.walls, walls[index] if index is not None else walls)
    assert_snapshots_equal(orc.snapshot(), snaps[0], f"{name}: behind set_walls")
    for t, a in enumerate(actions):
        assert orc.step(a) == 0
        assert_snapshots_equal(orc.snapshot(), snaps[t + 1], f"{name}: step {t}")
    assert {k: orc.events[k] for k in GW.ALL} == events                      # (the fast reference's bookkeeping counts what WallsRef counts)
    orc.close()


def masked_sequence(c, walls, index, auto_reset):
    """set_walls for all, steps, a masked set_walls with other layouts, steps, a masked reset under another seed, one layout for a few,
    steps: (the call, its arguments) in order"""
    B = c["B"]
    rng = np.random.default_rng(c["seed"] + 3)
    steps = lambda n: [("step", (WR.draw_actions(rng, B),)) for _ in range(n)]
    m1 = np.zeros(B, np.uint8); m1[[1, 4, 6]] = 1
    m2 = np.zeros(B, np.uint8); m2[::3] = 1
    other = ((index + 1) % len(walls)).astype(np.int32)
    return ([("set_walls", (walls, index))] + steps(8) + [("set_walls", (walls, other, m1))] + steps(8) + [("reset", (m2, 91))] + steps(5)
            + [("set_walls", (walls[-1], None, m2[::-1].copy()))] + steps(8 if auto_reset else 4))


@pytest.mark.parametrize("auto_reset", [True, False], ids=["auto_reset", "no_auto_reset"])
@pytest.mark.parametrize("T", ["Float32", "Float64"])
@pytest.mark.parametrize("H,W", [(5, 7), (6, 6)])
def test_a_masked_set_walls_sequence(rcw, oracle, H, W, T, auto_reset):
    c = dict(H=H, W=W, N=24, Hc=20, B=8, seed=13, T=T)
    walls, index = GW.three_layouts(H, W), (np.arange(8) % 3).astype(np.int32)
    ref = GW.make_ref(c, auto_reset=auto_reset)
    orc = WO.from_case(c, auto_reset=auto_reset, render_top_view=1, pu_per_tu=6)
    assert_snapshots_equal(orc.snapshot(), ref.snapshot(), "fresh")
    for k, (call, args) in enumerate(masked_sequence(c, walls, index, auto_reset)):
        getattr(ref, call)(*args)
        assert getattr(orc, call)(*args) in (None, 0)
        where = f"{H} x {W}, {T}, call {k}: {call}"
        assert_snapshots_equal(orc.snapshot(), ref.snapshot(), where)
        if k % 6 == 0:
            np.testing.assert_array_equal(orc.top_view, ref.top_view(6), err_msg=f"top view {where}")
        for b in range(8):
            np.testing.assert_array_equal(orc.walls_of(b), ref.walls_of(b))
    assert orc.events == {k: ref.events[k] for k in orc.events if k != "episode_starts"} | dict(episode_starts=0), (orc.events, ref.events)
    assert ref.events["goal_redraws"] > 0 and ref.events["interior_wall_ray_hits"] > 0
    orc.close()


def test_a_ring_only_map_draws_what_it_drew(oracle):
    """set_walls(ring) is one more reset: the draw indices of a map without interior walls are unchanged"""
    kw = dict(height_tile_map_tu=8, width_tile_map_tu=8, num_rays=32, auto_reset=1)
    a, b = WO.WalledOracle(16, seed=9, **kw), oracle.OracleBatch(16, seed=9, **kw)
    ring = np.zeros((8, 8), bool); ring[[0, -1]] = True; ring[:, [0, -1]] = True
    a.set_walls(ring); b.reset(seed=9)
    rng = np.random.default_rng(2)
    for _ in range(30):
        act = WR.draw_actions(rng, 16)
        assert a.step(act) == 0 and b.step(act) == 0
    for k in ("goal", "position", "direction", "episode", "camera_view", "done"):
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=k)
    assert not a.goal_redraws.any() and a.events["interior_wall_ray_hits"] == 0


def test_the_goal_redraw_is_the_scalar_restatement(oracle):
    """half of the interior walled, 24 agents, three episodes each: goal, tile and heading are walls_ref.reset_draws_scalar's — the
    restatement in Python integers the header's text was written beside — and the oracle's counter saw pairs drawn again.  (The cap of
    1024 H W redraws is out of reach of a layout set_walls accepts: two free interior tiles are all a goal needs.)"""
    walls = np.zeros((8, 8), bool); walls[[0, -1]] = True; walls[:, [0, -1]] = True
    walls[1:-1, 1:-1] = (np.arange(36) % 2 == 0).reshape(6, 6)
    orc = WO.WalledOracle(24, seed=5, height_tile_map_tu=8, width_tile_map_tu=8, num_rays=8, height_camera_view_pu=8, num_directions=8,
                          agent_id_offset=1000)
    for episode in (1, 2, 3):
        orc.set_walls(walls) if episode == 1 else orc.reset(seed=5)
        for b in range(24):
            gi, gj, ti, tj, d, gave_up = WR.reset_draws_scalar(5, 1000 + b, episode, 8, 8, 8, walls)
            assert (orc.goal[b].tolist(), orc.position[b].tolist(), int(orc.direction[b])) == ([gi, gj], [ti - 0.5, tj - 0.5], d) and not gave_up
    assert orc.goal_redraws.sum() > 0 and not orc.status.any() and (orc.episode == 4).all()
    orc.close()


def test_the_refusals_are_those_of_the_engine_and_leave_the_oracle_untouched(rcw, oracle, validate):  # noqa: F811
    L = rcw.layouts
    H, W, B = 6, 7, 4
    ring, rooms = L.ring(H, W), L.four_rooms(H, W)
    orc = WO.from_case(dict(H=H, W=W, N=16, Hc=16, B=B, seed=2))
    orc.set_walls(np.stack([ring, rooms]), [0, 1, 1, 0])
    assert orc.step(np.ones(B, np.uint8)) == 0
    before = orc.snapshot()
    cases = []
    for i, j in ((0, 3), (5, 0), (2, 6), (5, 6)):                            # a missing ring tile, also of a layout nobody takes
        bad = rooms.copy(); bad[i, j] = False
        cases.append((np.stack([ring, bad]), [0, 0, 0, 0], None))
    full = np.ones((H, W), bool); full[2, 2] = False
    cases.append((full[None], None, None))                                   # fewer than two free interior tiles
    cases += [(np.stack([ring, rooms]), ix, None) for ix in ([0, 2, 1, 0], [0, -1, 1, 0])]   # an index out of range
    cases.append((np.stack([ring, rooms, ring]), None, None))                # a NULL index with another layout count
    cases.append((np.zeros((0, H, W), bool), None, None))                    # no layout at all
    for walls, index, mask in cases:
        if len(walls):
            assert validate(H, W, B, walls, index, mask)[0] == -1
        with pytest.raises(ValueError):
            orc.set_walls(walls, index, mask)
        assert_snapshots_equal(orc.snapshot(), before, "behind a refusal")
    with pytest.raises(ValueError):
        orc.set_walls(np.ones((H + 1, W), bool))
    full[3, 4] = False
    for walls, index, mask in ((full[None], None, None), (np.stack([ring, rooms]), [0, 2, 1, 0], [1, 0, 1, 1])):   # (what the engine takes, the oracle takes)
        assert validate(H, W, B, walls, index, mask)[0] == 0
        orc.set_walls(walls, index, mask)
    assert (orc.episode == before["episode"] + np.array([2, 1, 2, 2], np.uint32)).all()
    orc.close()


def test_a_step_leaves_the_unmoved_agents_as_they_are(oracle):
    kw = dict(height_tile_map_tu=8, width_tile_map_tu=8, num_rays=32, auto_reset=1, out_of_bounds=1)
    a, b = oracle.OracleBatch(12, seed=4, **kw), oracle.OracleBatch(12, seed=4, **kw)
    rng = np.random.default_rng(0)
    g = np.tile(np.array([[4, 6]], np.int32), (12, 1)); p = np.tile(np.array([[3.5, 4.5]], np.float32), (12, 1)); d = np.full(12, 32, np.int32)
    a.set_state(g, p, d); b.set_state(g, p, d)                               # (four forward moves from the goal: episodes end and restart)
    restarted = 0
    for t in range(40):
        act = np.where(rng.random(12) < 0.7, 1, rng.integers(1, 5, 12)).astype(np.uint8)
        moved = (rng.random(12) < 0.6).astype(np.uint8)
        keep = {k: getattr(a, k).copy() for k in ("goal", "position", "direction", "episode", "camera_view", "done", "reward", "status")}
        bad = act.copy(); bad[moved == 0] = 77                               # (an unmoved agent's action is not read)
        lenient = t % 2 == 1
        if lenient:
            bad[np.flatnonzero(moved)[:1]] = 0
            act = np.where(moved != 0, bad, act).astype(np.uint8)
        assert (a.step_lenient if lenient else a.step)(bad, moved) == 0
        for k, v in keep.items():
            np.testing.assert_array_equal(getattr(a, k)[moved == 0], v[moved == 0], err_msg=f"{k} of the unmoved, step {t}")
        restarted += int((a.episode != keep["episode"]).sum())
        # the twin, unmasked: the same agents moved one at a time are what a mask of one gives
        for k in np.flatnonzero(moved):
            one = np.zeros(12, np.uint8); one[k] = 1
            assert b.step_lenient(act, one) == 0
        for k in keep:
            np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=f"{k}, step {t}")
        a.clear_status(); b.clear_status()
    assert restarted > 0
    assert a.step(np.zeros(12, np.uint8), np.zeros(12, np.uint8)) == 0 and a.step(np.zeros(12, np.uint8)) != 0
    a.close(); b.close()


def test_the_stand_alone_program_runs_clean_under_the_sanitizers():
    """oracle/san_walls_main.c with rcw_oracle.c under -fsanitize=address,undefined, both widths, on the CPU"""
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("gcc has no libasan.so here")                           # (as tests/test_oracle_sanitizers.py)
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "-B", "san-walls"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "clean (T = Float32)" in r.stdout and "clean (T = Float64)" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
