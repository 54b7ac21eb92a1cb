"""The goal distance's specification (tests/goal_distance_ref.py) against cases derived by hand and against layouts.is_connected.
CPU only: what the GPU tests compare the engine with must itself be right."""
import numpy as np

from goal_distance_ref import (PILLAR_SEEDS, UNREACHED, GoalDistanceRef, bfs_field, level_sizes, linear, lookup, middle_free_tile, pillars, pocket,
                               serpentine, widest_level)

X = UNREACHED


def test_pocket_field_by_hand():
    """7 x 7 pocket layout, goal (2, 2): the ring corridor's distances read off the drawing; walls and the enclosed (4, 4) hold 0xFFFF."""
    f = bfs_field(pocket(), (2, 2))
    want = np.array([[X, X, X, X, X, X, X],
                     [X, 0, 1, 2, 3, 4, X],
                     [X, 1, X, X, X, 5, X],
                     [X, 2, X, X, X, 6, X],
                     [X, 3, X, X, X, 7, X],
                     [X, 4, 5, 6, 7, 8, X],
                     [X, X, X, X, X, X, X]], np.uint16)
    assert f.dtype == np.uint16
    np.testing.assert_array_equal(f, want)


def test_goal_in_the_pocket_reaches_nothing_else():
    f = bfs_field(pocket(), (4, 4))
    assert f[3, 3] == 0
    f[3, 3] = X
    assert (f == X).all()


def test_goal_in_a_wall_reaches_nothing():
    assert (bfs_field(pocket(), (3, 3)) == X).all()
    assert (bfs_field(pocket(), (1, 1)) == X).all()


def test_agrees_with_is_connected():
    """No 0xFFFF on a free tile exactly when the layout is connected: 50 random mazes (connected by construction), the pocket (not), and
    mazes with one more tile walled in."""
    from raycastworlds_jl_amd import layouts

    rng = np.random.default_rng(11)
    cases = [(pocket(), (2, 2))]
    for k in range(50):
        H, W = int(rng.integers(5, 20)), int(rng.integers(5, 20))
        m = layouts.maze(H, W, rng)
        free = np.argwhere(~m)
        g = free[int(rng.integers(len(free)))]
        cases.append((m, (g[0] + 1, g[1] + 1)))
        if k % 5 == 0 and H >= 7 and W >= 7:                               # close a box around (4, 4): a pocket inside a maze
            p = m.copy()
            p[2:5, 2:5] = True
            p[3, 3] = False
            q = np.argwhere(~p)
            q = q[(q != (3, 3)).any(axis=1)]
            if len(q):
                cases.append((p, tuple(q[0] + 1)))
    seen = set()
    for walls, goal in cases:
        f = bfs_field(walls, goal)
        all_reached = not (f[~walls] == X).any()
        assert all_reached == layouts.is_connected(walls)
        assert (f[walls] == X).all()
        seen.add(all_reached)
    assert seen == {True, False}


def test_linear_order_on_a_non_square_map():
    """5 x 7: tile (i, j) at (i - 1) + H (j - 1), the order rcw_set_walls takes — not its transpose."""
    H, W = 5, 7
    walls = np.zeros((H, W), bool)
    walls[[0, -1], :] = True
    walls[:, [0, -1]] = True
    walls[2, 2] = True                                                     # (3, 3): off-centre
    f = bfs_field(walls, (2, 2))
    lin = linear(f)
    assert lin.shape == (H * W,)
    for i in range(1, H + 1):
        for j in range(1, W + 1):
            assert lin[(i - 1) + H * (j - 1)] == f[i - 1, j - 1]
    assert lin[(2 - 1) + H * (6 - 1)] == 4 and lin[(4 - 1) + H * (2 - 1)] == 2      # (2, 6) is four tiles along the row, (4, 2) two down
    assert f[3, 2] == 3 and f[2, 3] == 3                                   # round the wall at (3, 3) either way: (4, 3) and (3, 4)


def test_lookup_is_wu_to_tu():
    f = bfs_field(pocket(), (2, 2))
    assert lookup(f, (1.5, 1.5)) == 0 and lookup(f, (1.999, 2.0)) == 1 and lookup(f, (5.5, 5.5)) == 8
    assert lookup(f, (3.5, 3.5)) == -1                                     # the pocket
    assert lookup(f, (2.5, 2.5)) == -1                                     # a wall
    assert lookup(f, (-0.5, 1.5)) == -1 and lookup(f, (1.5, 7.0)) == -1 and lookup(f, (float("nan"), 1.0)) == -1


def test_serpentine_is_one_long_corridor():
    w = serpentine(12, 9)
    f = bfs_field(w, (2, 2))
    free = ~w
    assert not (f[free] == X).any()
    assert int(f[free].max()) >= free.sum() - 9                            # (all but the last double row lies along one path)
    big = bfs_field(serpentine(254, 254), (2, 2))
    assert int(big[big != X].max()) > 31000                                # tens of thousands of levels of one tile


def test_word_rules():
    """restart (the counter moved), mask (the counter did not), and either side -1."""
    walls = np.stack([pocket()] * 4)
    goal = np.array([[2, 2]] * 4, np.int32)
    pos = np.array([[5.5, 5.5], [1.5, 2.5], [3.5, 3.5], [1.5, 1.5]], np.float32)
    ep = np.array([1, 1, 1, 1], np.uint32)
    r = GoalDistanceRef(walls, goal, pos, ep)
    np.testing.assert_array_equal(r.distance, [8, 1, -1, 0])
    np.testing.assert_array_equal(r.start_distance, r.distance)
    np.testing.assert_array_equal(r.progress, 0)
    # a step: agent 0 one tile closer, agent 1 one farther, agent 2 still in the pocket, agent 3 restarted with a new goal
    pos2 = np.array([[5.5, 4.5], [1.5, 3.5], [3.5, 3.5], [5.5, 5.5]], np.float32)
    goal2 = goal.copy(); goal2[3] = (2, 6)
    ep2 = np.array([1, 1, 1, 2], np.uint32)
    r.stepped(walls, goal2, pos2, ep2)
    np.testing.assert_array_equal(r.distance, [7, 2, -1, 4])
    np.testing.assert_array_equal(r.progress, [1, -1, 0, 0])
    np.testing.assert_array_equal(r.start_distance, [8, 1, -1, 4])
    assert r.field[3][1, 5] == 0 and r.field[0][1, 1] == 0
    # a step that changes agent 0's goal WITHOUT the counter moving is not seen (set_state's business); one that leaves the map gives 0
    pos3 = pos2.copy(); pos3[1] = (-1.0, 3.5)
    r.stepped(walls, goal2, pos3, ep2)
    np.testing.assert_array_equal(r.distance, [7, -1, -1, 4])
    np.testing.assert_array_equal(r.progress, [0, 0, 0, 0])
    r.stepped(walls, goal2, pos2, ep2)                                     # and back: -1 on the old side
    np.testing.assert_array_equal(r.progress, [0, 0, 0, 0])
    np.testing.assert_array_equal(r.distance, [7, 2, -1, 4])
    # a masked set_state that moves agent 0's goal: counter unchanged, the field changes; agent 1 outside the mask keeps every byte
    before = r.field[1].copy()
    goal3 = goal2.copy(); goal3[0] = (6, 6)
    r.masked(walls, goal3, pos2, ep2, np.array([1, 0, 0, 0], np.uint8))
    assert r.field[0][5, 5] == 0 and r.distance[0] == 1 and r.start_distance[0] == 1 and r.progress[0] == 0
    np.testing.assert_array_equal(r.field[1], before)
    assert r.start_distance[1] == 1 and r.distance[1] == 2


def textbook_bfs(walls, goal):
    """the flood as a textbook writes it — a queue of (i, j), every neighbour range-checked, the distances read from the array being
    filled: slow, and what bfs_field's border-and-lists loop must equal"""
    from collections import deque

    w = np.asarray(walls) != 0
    H, W = w.shape
    f = np.full((H, W), X, np.uint16)
    gi, gj = int(goal[0]) - 1, int(goal[1]) - 1
    if not (0 <= gi < H and 0 <= gj < W) or w[gi, gj]:
        return f
    f[gi, gj] = 0
    q = deque([(gi, gj)])
    while q:
        i, j = q.popleft()
        for ni, nj in ((i - 1, j), (i + 1, j), (i, j - 1), (i, j + 1)):
            if 0 <= ni < H and 0 <= nj < W and not w[ni, nj] and f[ni, nj] == X:
                f[ni, nj] = f[i, j] + 1
                q.append((ni, nj))
    return f


def test_bfs_field_is_the_textbook_flood():
    """300 random maps of 1 x 1 to 39 x 39 — noise without a ring (free tiles on the border: the range checks), pillars, mazes, serpentines,
    empty maps — with three goals each, on the map, in walls and off the map: the same array, type and shape."""
    from raycastworlds_jl_amd import layouts

    rng = np.random.default_rng(0)
    compared = reached_border = off_map = 0
    for k in range(300):
        H, W = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        kind = k % 4
        if kind == 0:
            w = rng.random((H, W)) < rng.uniform(0, 0.6)
        elif kind == 1 and H >= 3 and W >= 3:
            w = pillars(H, W, rng.uniform(0, 0.5), rng)
        elif kind == 2 and H >= 5 and W >= 5:
            w = layouts.maze(H, W, rng)
        elif H >= 3 and W >= 3:
            w = serpentine(H, W)
        else:
            w = np.zeros((H, W), bool)
        for _ in range(3):
            g = (int(rng.integers(-1, H + 2)), int(rng.integers(-1, W + 2)))
            got, want = bfs_field(w, g), textbook_bfs(w, g)
            assert got.dtype == want.dtype == np.uint16 and got.shape == want.shape == (H, W)
            np.testing.assert_array_equal(got, want, err_msg=f"{H} x {W}, goal {g}")
            compared += 1
            off_map += not (1 <= g[0] <= H and 1 <= g[1] <= W)
            reached_border += bool((got[[0, -1], :] != X).any() or (got[:, [0, -1]] != X).any())
    assert compared == 900 and off_map > 50 and reached_border > 100, (compared, off_map, reached_border)
    big = pillars(132, 134, 0.2, np.random.default_rng(0))
    np.testing.assert_array_equal(bfs_field(big, (67, 75)), textbook_bfs(big, (67, 75)))


# ---- how wide the levels are: the preconditions of the GPU tests' wide-level cases, rehearsed where no kernel can satisfy them --------
def ring(H, W):
    w = np.zeros((H, W), bool)
    w[[0, -1], :] = True
    w[:, [0, -1]] = True
    return w


def test_level_sizes_by_hand():
    f = bfs_field(pocket(), (2, 2))                                        # the ring corridor: two ways round, one tile where they meet
    assert level_sizes(f).tolist() == [1, 2, 2, 2, 2, 2, 2, 2, 1] and widest_level(f) == 2
    assert level_sizes(bfs_field(pocket(), (3, 3))).tolist() == [] and widest_level(bfs_field(pocket(), (3, 3))) == 0
    assert level_sizes(bfs_field(ring(5, 5), (3, 3))).tolist() == [1, 4, 4]
    assert int(level_sizes(f).sum()) == int((f != X).sum())


def test_pillars_layout():
    w = pillars(30, 40, 0.25, np.random.default_rng(1))
    assert w.dtype == bool and w.shape == (30, 40) and w[[0, -1], :].all() and w[:, [0, -1]].all()
    assert 0.15 < w[1:-1, 1:-1].mean() < 0.35
    np.testing.assert_array_equal(w, pillars(30, 40, 0.25, np.random.default_rng(1)))
    np.testing.assert_array_equal(pillars(6, 7, 0.0, np.random.default_rng(0)), ring(6, 7))
    assert pillars(6, 7, 1.0, np.random.default_rng(0)).all()
    g = middle_free_tile(w)
    assert not w[g[0] - 1, g[1] - 1] and abs(g[0] - 15) <= 1


def test_open_room_132_x_134_has_every_level_width():
    """From an interior corner the levels hold 1, 2, ..., 130 tiles, every value present, and the largest distance is 260; from the centre
    the widest level holds 259 tiles and the largest distance is 131."""
    H, W = 132, 134
    for goal in ((2, 2), (2, W - 1), (H - 1, 2), (H - 1, W - 1)):
        s = level_sizes(bfs_field(ring(H, W), goal))
        assert set(range(1, 131)) <= set(s.tolist()) and int(s.max()) == 130 and len(s) - 1 == 260
    s = level_sizes(bfs_field(ring(H, W), (66, 67)))
    assert int(s.max()) == 259 and len(s) - 1 == 131


PILLAR_FIGURES = {0: (217, 88, 39), 1: (184, 91, 66), 2: (131, 119, 27), 3: (151, 119, 39), 5: (168, 104, 35), 8: (201, 87, 23), 9: (182, 100, 27),
                  10: (194, 95, 31)}      # seed: (widest level, levels of more than 64 tiles, free tiles without a path)


def test_pillared_rooms_have_ragged_wide_levels():
    assert tuple(PILLAR_FIGURES) == PILLAR_SEEDS
    for seed, figures in PILLAR_FIGURES.items():
        w = pillars(132, 134, 0.2, np.random.default_rng(seed))
        f = bfs_field(w, middle_free_tile(w))
        s = level_sizes(f)
        assert (int(s.max()), int((s > 64).sum()), int(((f == X) & ~w).sum())) == figures, seed
        assert s.max() > 128
    for seed, widest in ((4, 122), (6, 120), (7, 117)):                    # (the seeds in between: their middle free tile lies by the long wall)
        w = pillars(132, 134, 0.2, np.random.default_rng(seed))
        assert widest_level(bfs_field(w, middle_free_tile(w))) == widest


def test_the_largest_maps_the_library_accepts():
    """rcw_create takes H W + 2 H <= 65280.  254 x 255, the squarest: 503 tiles in the widest level from the centre; 86 x 757, the squarest
    whose last interior tile lies above index 65,000: 168; 3 x 21758 holds the largest index of all, 65,269, in a corridor one tile wide.
    From the last interior tile the levels grow to the short side's interior and the largest distance is H + W - 6."""
    for H, W, widest in ((254, 255, 503), (86, 757, 168), (3, 21758, 2)):
        assert H * W + 2 * H <= 65280 < H * (W + 1) + 2 * H
        assert widest_level(bfs_field(ring(H, W), ((H + 1) // 2, (W + 1) // 2))) == widest
        f = bfs_field(ring(H, W), (H - 1, W - 1))
        s = level_sizes(f)
        assert (int(s.max()), len(s) - 1) == (min(H, W) - 2, H + W - 6)
        assert int(np.flatnonzero(linear(f) != X).max()) == H * W - H - 2
    assert 255 * 256 + 2 * 255 > 65280                                     # (65,280 tiles in 255 x 256 do not fit beside the guard bands)
    assert 86 * 757 - 86 - 2 == 65014 and 3 * 21758 - 3 - 2 == 65269


def test_the_layouts_of_the_older_gpu_tests_have_narrow_levels():
    """Why the wide-level cases exist: every layout tests/test_gpu_goal_distance.py flooded before them keeps its levels far below the 64
    lanes of a wavefront, whatever the goal — the chunk loop ran once a level and the ballot's upper half stayed empty."""
    from raycastworlds_jl_amd import layouts

    def widest_over_goals(walls, every=1):
        return max(widest_level(bfs_field(walls, (i + 1, j + 1))) for i, j in np.argwhere(~walls)[::every])

    found = {"7 x 7 pocket": widest_over_goals(pocket()), "8 x 8 room": widest_over_goals(ring(8, 8)), "5 x 7 room": widest_over_goals(ring(5, 7)),
             "9 x 11 four_rooms": widest_over_goals(layouts.four_rooms(9, 11)), "9 x 9 four_rooms": widest_over_goals(layouts.four_rooms(9, 9)),
             "9 x 11 serpentine": widest_over_goals(serpentine(9, 11)), "200 x 300 serpentine": widest_over_goals(serpentine(200, 300), every=3001)}
    for size in (9, 32):
        rng = np.random.default_rng(size)                                  # test_per_agent_mazes' own layouts
        found[f"{size} x {size} mazes"] = max(widest_over_goals(layouts.maze(size, size, rng), every=1 if size == 9 else 11) for _ in range(32))
    assert all(v < 64 for v in found.values()), found
    # (over EVERY goal the 32 x 32 mazes reach 12 — four seconds of floods, recomputed once; the sample of every 11th free tile cannot pass it)
    assert max(found.values()) <= 12 and found["7 x 7 pocket"] == 2 and found["8 x 8 room"] == 10 and found["200 x 300 serpentine"] <= 3, found


# ---- the boundary, without a GPU: what the parent commit does not have --------------------------------------------------------------
EXPORTS = ("rcw_set_goal_distance", "rcw_goal_distance_enabled", "rcw_goal_distance", "rcw_goal_distance_device_ptr",
           "rcw_goal_distance_field", "rcw_goal_distance_field_device_ptr")


def test_the_six_exports_are_declared_bound_and_refuse_a_null_handle(rcw):
    """The header declares them, the binding lists them, the built library exports them, and none dereferences a NULL handle."""
    import ctypes as C
    import re

    from raycastworlds_jl_amd import _capi

    header = open(_capi.HEADER_PATH).read()
    lib = _capi.load()
    for name in EXPORTS:
        assert re.search(r"RCW_API int %s\(rcw_handle\* h[,)]" % name, header), name
        assert name in _capi.SIGNATURES, name
        assert hasattr(lib, name), name
    assert "#define RCW_ABI_VERSION 4" in header                            # additive: the version stays
    n, p = C.c_int32(7), C.c_void_p()
    word = (C.c_int32 * 1)()
    calls = [lib.rcw_set_goal_distance(None, 1), lib.rcw_goal_distance_enabled(None, C.byref(n)), lib.rcw_goal_distance(None, word, None, None),
             lib.rcw_goal_distance_device_ptr(None, C.byref(p), None, None), lib.rcw_goal_distance_field(None, 0, 1, word),
             lib.rcw_goal_distance_field_device_ptr(None, C.byref(p))]
    assert calls == [_capi.RCW_ERR_INVALID_ARGUMENT] * 6, calls
    assert _capi.last_error(lib)


def test_the_python_mirror_has_the_feature(rcw):
    import inspect

    SR = rcw.SingleRoomModule.SingleRoom
    assert inspect.signature(SR.__init__).parameters["goal_distance"].default is False
    assert inspect.signature(SR.set_goal_distance).parameters["on"].default is True
    for name in ("goal_distance", "goal_start_distance", "goal_progress", "goal_distance_field", "goal_distance_enabled"):
        assert isinstance(getattr(SR, name), property), name


def test_one_kernel_family_in_the_shipped_isa():
    """`make asm`: the listing holds the kernels of csrc/rcw_goal_distance.hip under the names the contract reserves — rcw_goal_distance*,
    none that the kernel counts of the other tests go by — and the one-wavefront kernel needs no workgroup barrier."""
    import os
    import re
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "raycastworlds.jl_amd", "csrc")
    res = subprocess.run(["make", "-C", csrc, "asm"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    text = open(os.path.join(root, "raycastworlds.jl_amd", "lib", "asm", "rcw_goal_distance.s")).read()
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    assert kernels and all("rcw_goal_distance" in k for k in kernels), kernels
    assert not [k for k in kernels if "_limit_kernel" in k or "rcw_cast" in k or "rcw_fill" in k], kernels
    assert "s_barrier" not in text
    whole = open(os.path.join(root, "raycastworlds.jl_amd", "lib", "asm", "rcw_kernels.s")).read()
    assert all(k in whole for k in kernels)                                # (the concatenated listing the ISA checks read carries it)
