"""The goal distance's specification (tests/goal_distance_ref.py) against cases derived by hand and against layouts.is_connected.
CPU only: what the GPU tests compare the engine with must itself be right."""
import numpy as np

from goal_distance_ref import UNREACHED, GoalDistanceRef, bfs_field, linear, lookup, pocket, serpentine

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
