"""The episode time limit on the GPU (include/rcw.h, rcw_set_time_limit): every step of a rollout against the unchanged oracle composed by
tests/time_limit_ref.py, byte for byte — camera view, reward, done, episode counter, position, heading, goal, tile map, column descriptors
and the limit's own two words — in every form a step takes.

The scenarios (4 x 4 / 4 x 5 rooms, 8 headings, a quarter tile a move, forward-heavy actions, limits of 3 and 4 steps) were rehearsed on
the oracle alone: each truncates hundreds of times, reaches the goal dozens of times — some of them on the very step the limit is
reached —, and restarts after either.  Each test asserts from the helper's own event counts that its run did exercise what it claims.

Under RCW_OOB_ERROR (out_of_bounds = 0) the same rooms raise: a quarter-tile move next to the ring tests a neighbourhood that leaves the map.
The rehearsal of the raising rollouts (24 steps, 64 agents, no invalid actions; the same counts in Float32 and Float64):

    rollout   raised_with_words_kept   steps of the 24 that raise   truncations   terminations   on_the_limit_step   restarts after truncation / done
    A          84                       19                           258           27             6                   240 / 25
    WIDE       34                       20                           357           18             8                   350 / 18
    F64        79                       23                           255           34             7                   234 / 31
"""
import numpy as np
import pytest

import learner_view_ref as LV
import learner_view_stack_ref as LS
import time_limit_ref as TL
from helpers import assert_state_equal

pytestmark = pytest.mark.gpu

B = 64
A = dict(H=4, W=4, N=64, Hc=64, L=4, steps=48, seed=7, bad_every=5)          # a wavefront per agent in the one-launch form
WIDE = dict(H=4, W=5, N=320, Hc=64, L=3, steps=40, seed=11)                 # a workgroup per agent
F64 = dict(H=4, W=4, N=96, Hc=40, L=4, steps=40, seed=3, T="Float64")       # 40 rows: the flat fill, two launches
ALL = ("truncations", "terminations", "on_the_limit_step", "restarts_after_truncation", "restarts_after_done")


class Limited:
    """engine, oracle and the helper side by side"""

    def __init__(self, rcw, oracle, H, W, N, Hc, L, seed, steps=0, bad_every=0, T="Float32", auto_reset=True, form=None, limit_by="call", batch=B,
                 out_of_bounds=1, **kw):
        geometry = dict(height_tile_map_tu=H, width_tile_map_tu=W, num_rays=N, height_camera_view_pu=Hc, num_directions=8, out_of_bounds=out_of_bounds, **kw)
        ctor = dict(max_episode_steps=L) if limit_by == "constructor" else {}
        self.env = rcw.SingleRoomModule.SingleRoom(batch=batch, seed=seed, T=T, auto_reset=auto_reset, position_increment_wu=0.25, **geometry, **ctor)
        self.orc = oracle.OracleBatch(batch, seed=seed, auto_reset=1 if auto_reset else 0, position_increment_wu=0.25, position_increment_wu_f64=0.25,
                                      world_unit_bits=64 if T == "Float64" else 32, **geometry)
        self.rcw, self.steps_planned, self.bad_every, self.top = rcw, steps, bad_every, bool(kw.get("render_top_view"))
        self.B, self.may_raise, self.steps_that_raised = batch, out_of_bounds == 0, 0
        self.rng = np.random.default_rng(seed + 1)
        self.t = 0
        if form is not None:
            self.env.set_step_form(form)
            assert self.env.step_form() == form
        if limit_by == "call":
            self.env.set_time_limit(L)
        self.ref = TL.TimeLimitRef(self.orc, L, seed, auto_reset)
        assert self.env.time_limit == L

    def check(self, where):
        env, orc, ref = self.env, self.orc, self.ref
        assert_state_equal(env, orc, where=where)
        np.testing.assert_array_equal(env.world.episode, orc.episode, err_msg=f"episode {where}")
        np.testing.assert_array_equal(env.world.episode_steps, ref.episode_steps, err_msg=f"episode_steps {where}")
        np.testing.assert_array_equal(env.world.truncated.astype(np.uint8), ref.truncated, err_msg=f"truncated {where}")
        if self.top:
            np.testing.assert_array_equal(env.top_view_host(), orc.top_view, err_msg=f"top view {where}")

    def step(self, where, device=None, a=None, check=True):
        a = TL.draw_actions(self.rng, self.B, self.t, self.bad_every) if a is None else a
        valid = bool(((a >= 1) & (a <= 4)).all())
        if device is None:
            device = not valid or self.t % 2 == 1                          # (rcw_step refuses the whole batch: the invalid rows take the device path)
        if device:
            import torch

            self.rcw.act_(self.env, torch.from_numpy(a).cuda())
        else:
            self.rcw.act_(self.env, a)
        self.ref.step(a)
        self.t += 1
        if not valid:
            with pytest.raises(AssertionError, match="invalid action"):
                self.env.sync()
            self.env.clear_error()
        elif self.may_raise:
            # RCW_OOB_ERROR: a move that tested a tile outside the map raised in the reference.  The engine says so at the next sync, once for
            # the batch (IndexError), and per agent in the sticky status words: the oracle's, agent for agent.
            try:
                self.env.sync()
            except IndexError:
                np.testing.assert_array_equal(self.env.world.status, self.orc.status, err_msg=f"status {where}")
                self.env.clear_error(); self.orc.clear_status()
                self.steps_that_raised += 1
            else:
                assert not (self.orc.status == TL.RCW_ERR_OUT_OF_BOUNDS).any(), f"the oracle raised and the engine did not, {where}: {self.orc.status}"
        if check:
            self.check(where)

    def run(self, name, steps=None):
        for _ in range(self.steps_planned if steps is None else steps):
            self.step(f"{name} step {self.t}")
        return self.ref.events

    def close(self):
        self.env.close(); self.orc.close()


def covered(events, columns):
    assert all(events[c] > 0 for c in columns), events


ROLLOUTS = [("two launches, a wavefront of columns", A, "two-launches", ALL + ("invalid_while_truncated",)),
            ("one launch, a wavefront per agent", A, "one-launch", ALL + ("invalid_while_truncated",)),
            ("two launches, 320 columns", WIDE, "two-launches", ALL),
            ("one launch, a workgroup per agent", WIDE, "one-launch", ALL),
            ("Float64, the flat fill", F64, None, ALL)]


@pytest.mark.parametrize("name,case,form,columns", ROLLOUTS, ids=[r[0] for r in ROLLOUTS])
def test_step_by_step_against_the_composed_oracle(rcw, oracle, name, case, form, columns):
    pytest.importorskip("torch")
    s = Limited(rcw, oracle, form=form, **case)
    if form is None:
        assert s.env.step_form() == "two-launches" and s.env.fill_kernel_name() == "rcw_fill_flat_kernel"
    s.check(f"{name}: before the first step")
    covered(s.run(name), columns)
    assert s.orc.episode.max() >= 5
    s.close()


RAISED = {"A": (84, 19), "WIDE": (34, 20), "Float64": (79, 23)}             # (raised_with_words_kept, steps of the 24 that raise)
RAISING = [("A, two launches", A, "two-launches"), ("A, one launch", A, "one-launch"), ("WIDE, two launches", WIDE, "two-launches"),
           ("WIDE, one launch", WIDE, "one-launch"), ("Float64, the flat fill", F64, None)]


@pytest.mark.parametrize("name,case,form", RAISING, ids=[r[0] for r in RAISING])
def test_a_raising_move_leaves_the_agent_and_keeps_both_words(rcw, oracle, name, case, form):
    """The "raised in act!" row of DESIGN 4.7 under RCW_OOB_ERROR: the agent is left as it was and episode_steps / truncated are kept (the
    `LIMIT && !oob` arm of cast_body).  Every step syncs: an IndexError there must come with the oracle's status words, no IndexError with
    none.  In the one-launch form the forward (or backward) slot of a move that would raise is the current frame: the frames are compared
    behind every step, the raising ones included.  (The two-launch kernels store the words only where the move did not raise, so the guard
    decides nothing there that reaches memory: a build without it fails the two one-launch cases alone, through `reborn` and the frames.)"""
    pytest.importorskip("torch")
    s = Limited(rcw, oracle, form=form, out_of_bounds=0, **dict(case, steps=24, bad_every=0))
    if form is None:
        assert s.env.step_form() == "two-launches" and s.env.fill_kernel_name() == "rcw_fill_flat_kernel"
    ev = s.run(name)
    covered(ev, ALL + ("raised_with_words_kept",))
    assert (ev["raised_with_words_kept"], s.steps_that_raised) == RAISED[name.split(",")[0]]          # (the rehearsal's)
    if form is not None:
        assert s.env.step_form() == form
    s.close()


@pytest.mark.parametrize("form", ["two-launches", "one-launch"])
def test_without_auto_reset_the_counter_keeps_counting(rcw, oracle, form):
    pytest.importorskip("torch")
    s = Limited(rcw, oracle, form=form, auto_reset=False, **dict(A, bad_every=0))
    ev = s.run(f"no auto_reset, {form}")
    covered(ev, ("truncations", "terminations", "on_the_limit_step"))      # (the counter passes L once an agent: the coincidence is rare — 2 here)
    assert ev["restarts_after_truncation"] == 0 and ev["restarts_after_done"] == 0
    assert int(s.ref.episode_steps.max()) > 2 * A["L"] and (s.orc.episode == s.orc.episode[0]).all()   # nobody restarted
    s.close()


def test_with_the_top_view_in_the_camera_fills_launch(rcw, oracle):
    """render_top_view: the cast kernel, then the camera fill and the top view's drawing in one launch, then the store kernel — the limit is
    the cast kernel's; both images follow the restarts"""
    pytest.importorskip("torch")
    s = Limited(rcw, oracle, **dict(A, Hc=256, steps=24), render_top_view=1, pu_per_tu=64, limit_by="constructor")
    assert s.env.fill_kernel_name() == "rcw_fill256_draw_kernel" and s.env.top_view_form() == "two-kernels"
    covered(s.run("top view"), ALL)
    s.close()


def test_the_frame_stack_refills_on_a_truncation_restart(rcw, oracle):
    """set_learner_view("gray", (16, 16), camera_view=False, stack=3): the cast kernel, then the view kernel.  The stack's bytes against the
    numpy model fed with the oracle's frames and episode counters: a restart after a truncation moved the counter, so all three slots of that
    agent hold the new episode's first frame."""
    pytest.importorskip("torch")
    s = Limited(rcw, oracle, **A)
    s.env.set_learner_view("gray", (16, 16), "chw", camera_view=False, stack=3)
    view = lambda: LV.from_frames(s.orc.camera_view, "gray", (16, 16))
    model = LS.StackModel(3, view(), s.orc.episode)
    refilled_after_truncation = 0
    for t in range(A["steps"]):
        was_truncated = s.ref.truncated != 0
        s.step(f"stack step {t}", check=False)
        restarted = model.push(view(), s.orc.episode)
        refilled_after_truncation += int((restarted & was_truncated).sum())
        got = s.env.learner_view_host()
        np.testing.assert_array_equal(got, model.stack, err_msg=f"the stack after step {t}")
        assert (got[restarted, 0] == got[restarted, 2]).all()
        np.testing.assert_array_equal(s.env.world.episode_steps, s.ref.episode_steps)
        np.testing.assert_array_equal(s.env.world.truncated.astype(np.uint8), s.ref.truncated)
        np.testing.assert_array_equal(s.env.world.done.astype(np.uint8), s.orc.done)
    covered(s.ref.events, ALL)
    assert refilled_after_truncation == s.ref.events["restarts_after_truncation"] > 0
    s.close()


def test_a_new_limit_in_the_middle_of_a_one_launch_run(rcw, oracle):
    """L 4 -> 2 -> 0 between one-launch steps.  The slots hold successors cast under the old limit — the re-sampled world's for every agent
    it had truncated —, and the call zeroes the counters: the very next step must show the current world's successor for those agents.  With
    L = 0 the run is the plain oracle's and both arrays read zero."""
    pytest.importorskip("torch")
    s = Limited(rcw, oracle, form="one-launch", **dict(A, bad_every=0))
    s.run("L = 4", 9)
    assert (s.ref.truncated != 0).sum() >= B // 2, "too few agents are truncated at the moment the limit changes"
    for limit, steps in ((2, 9), (0, 8), (3, 7)):
        s.env.set_time_limit(limit); s.ref.set_time_limit(limit)
        assert s.env.time_limit == limit and s.env.step_form() == "one-launch"
        s.check(f"right after set_time_limit({limit})")                     # zeroed words, every other byte as it was
        before = dict(s.ref.events)
        s.run(f"L = {limit}", steps)
        if limit == 0:
            assert s.ref.events["truncations"] == before["truncations"] and not s.env.world.episode_steps.any() and not s.env.world.truncated.any()
        else:
            assert s.ref.events["restarts_after_truncation"] > before["restarts_after_truncation"]
    with pytest.raises(ValueError):
        s.env.set_time_limit(-1)
    assert s.env.time_limit == 3
    s.close()


@pytest.mark.parametrize("form", ["two-launches", "one-launch"])
def test_masked_reset_and_set_state_zero_the_masked_agents_words(rcw, oracle, form):
    pytest.importorskip("torch")
    s = Limited(rcw, oracle, form=form, **dict(A, bad_every=0))
    s.run("warm-up", 9)
    mask = np.zeros(B, np.uint8); mask[::3] = 1
    assert (s.ref.episode_steps[mask != 0] > 0).any() and (s.ref.truncated[mask == 0] != 0).any()
    s.rcw.reset_(s.env, mask=mask, seed=99); s.orc.reset(mask=mask, seed=99); s.ref.clear(mask); s.ref.seed = 99   # (the handle's seed from here on)
    s.check("after the masked reset")
    assert not s.env.world.episode_steps[mask != 0].any() and s.env.world.episode_steps[mask == 0].any()
    s.run("behind the reset", 6)
    mask = np.zeros(B, np.uint8); mask[1::4] = 1
    goal = np.tile(np.array([[3, 3]], np.int32), (B, 1)); pos = np.full((B, 2), 1.5, np.float32); heading = np.arange(B, dtype=np.int32) % 8
    assert (s.ref.episode_steps[mask != 0] > 0).any()
    s.env.set_state(goal, pos, heading, mask=mask); s.orc.set_state(goal, pos, heading, mask=mask); s.ref.clear(mask)
    s.check("after the masked set_state")
    s.run("behind set_state", 6)
    s.rcw.reset_(s.env, seed=99); s.orc.reset(seed=99); s.ref.clear()
    s.check("after a reset of every agent")
    assert not s.env.world.episode_steps.any() and not s.env.world.truncated.any()
    s.close()


def test_a_replayed_graph_counts_and_truncates(rcw, oracle):
    """one captured step (two launches, one stream), replayed L + 2 times with the same device actions: nothing about the limit lives on the
    host but L, which the captured kernels carry as an argument"""
    torch = pytest.importorskip("torch")
    s = Limited(rcw, oracle, form="two-launches", **dict(A, bad_every=0))
    stream = torch.cuda.Stream()
    s.env.sync()
    s.env.set_stream(stream.cuda_stream)
    a_host = TL.draw_actions(s.rng, B, 0)
    with torch.cuda.stream(stream):
        actions = torch.from_numpy(a_host).cuda()
        for _ in range(2):                                                   # (warm-up outside the capture)
            s.step("warm-up", a=a_host, device=True)
        stream.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            s.rcw.act_(s.env, actions)
        for k in range(A["L"] + 2):
            g.replay(); s.ref.step(a_host)
            stream.synchronize()
            s.check(f"replay {k}")
    covered(s.ref.events, ("truncations", "restarts_after_truncation"))
    del g
    s.close()


def test_a_handle_without_a_limit_runs_what_it_ran(rcw, oracle):
    """a handle that never set a limit, one after set_time_limit(0) and the plain oracle, step by step in both forms; the two arrays stay
    zero, and the device arrays and the RLBase verb read what the host copies read"""
    pytest.importorskip("torch")
    for form in ("one-launch", "two-launches"):
        plain = Limited(rcw, oracle, form=form, limit_by="nobody", **dict(A, L=0))
        off = Limited(rcw, oracle, form=form, **dict(A, L=0))
        assert plain.env.fill_kernel_name() == off.env.fill_kernel_name()
        for t in range(12):
            a = TL.draw_actions(plain.rng, B, t, 5)
            plain.step(f"no limit, {form}, step {t}", a=a); off.step(f"set_time_limit(0), {form}, step {t}", a=a)
            np.testing.assert_array_equal(plain.env.camera_view_host(), off.env.camera_view_host())
        for s in (plain, off):
            assert not s.env.world.episode_steps.any() and not s.env.world.truncated.any()
            s.close()
    s = Limited(rcw, oracle, **A)
    s.run("device arrays", 9)
    rl = rcw.RLBaseEnv(s.env)
    assert s.ref.truncated.any()
    np.testing.assert_array_equal(np.asarray(s.env.truncated_device()), s.ref.truncated)
    np.testing.assert_array_equal(np.asarray(rcw.RLBase.is_truncated(rl)), s.ref.truncated != 0)
    np.testing.assert_array_equal(np.asarray(s.env.episode_steps_device()), s.ref.episode_steps)
    np.testing.assert_array_equal(s.env.truncated_device(as_bool=True).torch().cpu().numpy(), s.ref.truncated != 0)
    assert s.env.episode_steps_device() is s.env.episode_steps_device()
    s.close()
