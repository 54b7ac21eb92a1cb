"""The one-launch step leaves the frames of agents whose view it does not change as they are (include/rcw.h, rcw_camera_view).

The casting half of a launch leaves one byte per agent beside the slots it writes: bit s set when the frame the action s selects is the
very frame of the current state (a blocked / goal / raising move SR:162-176, an invalid action SR:140, or a move or turn so close to a wall
that every column stays saturated SR:433).  The fill half of the NEXT launch does not store the chunks of such an agent — if the handle
knows that the bound observation buffer holds the current frames (rcw_handle.h, StepFacts::obs_current).  What must hold whatever was skipped: after
every step the buffer equals the reference's camera_view for EVERY agent.

Every rollout here compares every pixel of every agent with the CPU oracle after every step, and does between steps whatever may make
the buffer differ from what the slots describe — each followed by further steps.  Every rollout also counts, from the ORACLE's frames
alone, the agent-steps whose frame is bit-identical before and after the step, and FAILS if there were too few for the skip to have been
exercised: at least one in 32 agent-steps for the 8 x 8 room at 512 agents or more (the bench's policy leaves 7.5 % of cfg-2's frames
unchanged, 6.0 % on the worst single step of 1024 agents), at least one in the rollout for the other geometries.  The seeds are fixed;
the counts of the cfg-2 rollouts on the CPU oracle alone (Rollout(env=None)) stand beside each case, the small batches' smallest is 14 of
480 agent-steps (512 rows, the buffers rollout).
"""
import numpy as np
import pytest

from helpers import CFG2, CFG3, assert_state_equal

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEF


class Rollout:
    """env (None: the oracle alone, to count a rollout's unchanged frames on the CPU) and oracle side by side."""

    def __init__(self, rcw, oracle, batch, seed, rng_seed, **kw):
        self.rcw, self.B, self.kw = rcw, batch, kw
        okw = {k: v for k, v in kw.items() if k not in ("auto_reset", "T")}
        if kw.get("auto_reset"):
            okw["auto_reset"] = 1
        if kw.get("T") == "Float64":
            okw["world_unit_bits"] = 64
        self.orc = oracle.OracleBatch(batch, seed=seed, **okw)
        self.env = rcw.SingleRoomModule.SingleRoom(batch=batch, seed=seed, **kw) if rcw is not None else None
        self.rng = np.random.default_rng(rng_seed)
        self.real = np.float64 if kw.get("T") == "Float64" else np.float32
        self.buf = None                     # the caller's buffer bound at the moment (a torch tensor), None: the library's
        self.frames_checked = True          # False while the camera view is not rendered (RCW_VIEW_ONLY)
        self.unchanged = self.agent_steps = 0

    def frames(self):
        if self.buf is None:
            return self.env.camera_view_host()
        self.env.sync()
        return self.buf.cpu().numpy().view(np.uint32)

    def check(self, where):
        if self.env is None:
            return
        assert_state_equal(self.env, self.orc, frames=False, where=where)
        if self.frames_checked:
            got, want = self.frames(), self.orc.camera_view
            if not np.array_equal(got, want):
                bad = np.flatnonzero((got != want).reshape(self.B, -1).any(axis=1))
                stale = [int(a) for a in bad if (got[a] == SENTINEL).all()]
                raise AssertionError(f"camera_view {where}: {bad.size} agents differ (first {bad[:8].tolist()}), {len(stale)} of them still hold the sentinel")

    def act(self, a, where, lenient=False):
        before = self.orc.camera_view.copy()
        if self.env is not None:
            self.rcw.act_(self.env, a)
        if lenient:
            self.orc.step_lenient(a if isinstance(a, np.ndarray) else a.cpu().numpy())
        else:
            assert self.orc.step(a) == 0
        self.unchanged += int((self.orc.camera_view == before).reshape(self.B, -1).all(axis=1).sum())
        self.agent_steps += self.B
        if not lenient:
            self.check(where)

    def steps(self, n, where, p_forward=None):
        for s in range(n):
            a = self.rng.integers(1, 5, self.B).astype(np.uint8)
            if p_forward is not None:
                a = np.where(self.rng.random(self.B) < p_forward, 1, a).astype(np.uint8)
            self.act(a, f"{where}, step {s}")

    # ---- what happens between steps ----------------------------------------------------------------------------------------
    def reset(self, masked, seed):
        mask = None
        if masked:
            mask = (self.rng.random(self.B) < 0.5).astype(np.uint8); mask[0] = 1; mask[-1] = 0
        if self.env is not None:
            self.rcw.reset_(self.env, mask=mask, seed=seed)
        self.orc.reset(mask=mask, seed=seed)
        self.check(f"after reset (masked: {masked})")

    def set_state_at_the_wall(self, masked):
        """(every other agent, or all:) right in front of a wall, looking at it — forward moves are blocked: the frame stays"""
        H, W = self.orc.H, self.orc.W
        goal = np.tile(np.array([[2, 2]], np.int32), (self.B, 1))
        pos = np.tile(np.array([[H - 1 - 0.25, 1.5 + (W - 3) / 2]], self.real), (self.B, 1))
        d = np.zeros(self.B, np.int32)
        mask = None
        if masked:
            mask = np.zeros(self.B, np.uint8); mask[::2] = 1
        if self.env is not None:
            self.env.set_state(goal, pos, d, mask=mask)
        self.orc.set_state(goal, pos, d, mask=mask)
        self.check(f"after set_state (masked: {masked})")

    def set_state_near_the_goal(self):
        """every agent four forward moves from its goal (the 8 x 8 room): episodes end there and, under auto_reset, restart"""
        B = self.B
        g = np.tile(np.array([[4, 6]], np.int32), (B, 1)); p = np.tile(np.array([[3.5, 4.5]], self.real), (B, 1)); d = np.full(B, 32, np.int32)
        if self.env is not None:
            self.env.set_state(g, p, d)
        self.orc.set_state(g, p, d)
        self.check("after set_state near the goal")

    def invalid_device_actions(self, where):
        import torch

        a = self.rng.integers(1, 5, self.B).astype(np.uint8)
        a[[3, self.B // 2, self.B - 1]] = [0, 9, 255]
        self.act(torch.from_numpy(a).cuda() if self.env is not None else a, where, lenient=True)
        if self.env is not None:
            with pytest.raises(AssertionError):
                self.env.sync()
            np.testing.assert_array_equal(self.env.world.status, self.orc.status)
            self.env.clear_error()
        self.orc.clear_status()
        self.check(where)

    def new_buffer(self):
        import torch

        cfg = self.env.cfg
        t = torch.empty((self.B, cfg.num_rays, cfg.height_camera_view_pu), dtype=torch.int32, device="cuda")
        t.fill_(SENTINEL - (1 << 32))
        torch.cuda.synchronize()
        return t

    def bind(self, buf):
        self.env.sync()
        self.env.bind_obs(buf.data_ptr() if buf is not None else None)
        self.buf = buf

    def finish(self, one_in=None):
        if self.env is not None:
            assert self.env.step_form() == "one-launch"
            self.env.close()
        need = 1 if one_in is None else -(-self.agent_steps // one_in)
        assert self.unchanged >= need, (f"{self.unchanged} unchanged frames in {self.agent_steps} agent-steps of the oracle's rollout, {need} needed: "
                                        "the rollout does not exercise the skip")
        return self.unchanged, self.agent_steps


def _one_launch(r, by_rule):
    if r.env is None:
        return
    if not by_rule:
        r.env.set_step_form("one-launch")
    assert r.env.step_form() == "one-launch"


def rollout_resets_and_states(rcw, oracle, batch=1024, by_rule=True, one_in=32, **kw):
    """masked and unmasked reset_ / set_state, invalid device actions, update_camera_view_, a change of form there and back, profiling"""
    r = Rollout(rcw, oracle, batch, 21, 5, **kw)
    _one_launch(r, by_rule)
    r.check("after create")
    r.steps(6, "first")
    r.reset(True, 77); r.steps(4, "after the masked reset")
    r.reset(False, 78); r.steps(4, "after the reset")
    r.set_state_at_the_wall(True); r.steps(4, "after the masked set_state")
    r.set_state_at_the_wall(False); r.steps(4, "after set_state")
    r.invalid_device_actions("invalid device actions"); r.steps(3, "after the invalid actions")
    if r.env is not None:
        rcw.update_camera_view_(r.env)
    r.check("after update_camera_view_"); r.steps(3, "after update_camera_view_")
    if r.env is not None:
        r.env.set_step_form("two-launches")
    r.steps(2, "two launches")
    if r.env is not None:
        r.env.set_step_form(None if by_rule else "one-launch")
    _one_launch(r, True); r.steps(4, "one launch again")
    if r.env is not None:
        r.env.profile(True)
    r.steps(3, "profiling")
    if r.env is not None:
        assert r.env.profile_read()[3] == 3
        r.env.profile(False)
    r.steps(3, "profiling off")
    return r.finish(one_in)


def rollout_buffers(rcw, oracle, batch=1024, by_rule=True, one_in=32, **kw):
    """bind_obs to a buffer full of a sentinel and back, two buffers alternating every step, RCW_VIEW_ONLY for a few steps"""
    r = Rollout(rcw, oracle, batch, 6, 1, **kw)
    _one_launch(r, by_rule)
    r.steps(4, "first")
    if r.env is not None:
        r.bind(r.new_buffer())
    r.steps(4, "a bound buffer that held a sentinel")
    if r.env is not None:
        r.buf.fill_(SENTINEL - (1 << 32)); __import__("torch").cuda.synchronize()   # the caller refills its buffer, and says so: the same pointer again
        r.bind(r.buf)
    r.steps(3, "the same buffer, refilled and bound again")
    if r.env is not None:
        r.bind(None)
    r.steps(4, "the library's buffer again")
    bufs = [r.new_buffer(), r.new_buffer()] if r.env is not None else [None, None]
    for s in range(6):
        if r.env is not None:
            r.bind(bufs[s & 1])
        r.steps(1, f"two buffers alternating, {s}")
    if r.env is not None:
        r.bind(None)
    r.steps(3, "the library's buffer after the two")
    if by_rule:                                              # (a one-launch REQUEST gives way to RCW_VIEW_ONLY and does not come back by itself)
        if r.env is not None:
            r.env.set_learner_view("gray", size=(64, 64), camera_view=False)
        r.frames_checked = False
        r.steps(3, "RCW_VIEW_ONLY")
        if r.env is not None:
            r.env.set_learner_view("gray", size=(64, 64), camera_view=True)
        r.frames_checked = True
        r.check("the camera view back in the step")
        _one_launch(r, True)
        r.steps(4, "after RCW_VIEW_ONLY")
        if r.env is not None:
            r.env.set_learner_view(None)
        r.steps(3, "the learner view off")
    return r.finish(one_in)


def rollout_episodes(rcw, oracle, batch=1024, by_rule=True, one_in=32, **kw):
    """episodes that end on the goal and restart under auto_reset (the re-sampled world's frame was cast one launch ahead)"""
    r = Rollout(rcw, oracle, batch, 3, 8, auto_reset=True, **kw)
    _one_launch(r, by_rule)
    r.set_state_near_the_goal()
    ep0 = int(r.orc.episode.sum())
    for s in range(24):
        r.steps(1, f"restart rollout {s}", p_forward=0.7)
        if r.env is not None:
            np.testing.assert_array_equal(r.env.world.episode, r.orc.episode)
    assert int(r.orc.episode.sum()) - ep0 > batch // 2, "too few episodes restarted for the test to mean anything"
    return r.finish(one_in)


def rollout_captured_step(rcw, oracle, batch=1024, one_in=32, **kw):
    """a captured step (the handle keeps two launches from then on), replays, and the one-launch form asked for again"""
    import torch

    r = Rollout(rcw, oracle, batch, 31, 2, auto_reset=True, **kw)
    _one_launch(r, True)
    env = r.env
    r.steps(4, "first")
    if env is None:
        r.steps(4 + 5, "(replays, after)")
        return r.finish(one_in)
    stream = torch.cuda.Stream()
    env.sync()
    env.set_stream(stream.cuda_stream)
    a_host = r.rng.integers(1, 5, batch).astype(np.uint8)
    with torch.cuda.stream(stream):
        actions = torch.from_numpy(a_host).cuda()
        stream.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            rcw.act_(env, actions)
        assert env.step_form() == "two-launches"
        for k in range(4):
            before = r.orc.camera_view.copy()
            g.replay(); assert r.orc.step(a_host) == 0
            r.unchanged += int((r.orc.camera_view == before).reshape(batch, -1).all(axis=1).sum()); r.agent_steps += batch
            stream.synchronize()
            r.check(f"replay {k}")
        env.set_step_form("one-launch")
        r.steps(5, "one launch again, behind the replays")
        stream.synchronize()
    del g
    return r.finish(one_in)


# (in the comments: unchanged / agent-steps of the oracle's rollout, counted on the CPU with Rollout(env=None), and the one in 32 needed;
# the states set in front of a wall and near the goal make the first and third far richer in unchanged frames than a random walk)
BIG = [
    ("resets, states, invalid actions, forms, profiling", rollout_resets_and_states, dict(out_of_bounds=1, **CFG2)),   # 24798 / 41984, 1312 needed
    ("bound buffers, RCW_VIEW_ONLY", rollout_buffers, dict(out_of_bounds=1, **CFG2)),                                    # 2682 / 34816 (7.7 %), 1088 needed
    ("episodes restart", rollout_episodes, dict(out_of_bounds=1, **CFG2)),                                               # 10001 / 24576, 768 needed
    ("a captured step", rollout_captured_step, dict(out_of_bounds=1, **CFG2)),                                           # 1110 / 13312 (8.3 %), 416 needed
]


@pytest.mark.parametrize("name,fn,kw", BIG, ids=[b[0] for b in BIG])
def test_cfg2_at_1024_agents_matches_the_oracle_after_every_step(rcw, oracle, name, fn, kw):
    """cfg-2, 1024 agents: the one-launch form by the rule, rcw_fill256_cast_kernel, a wavefront per agent."""
    pytest.importorskip("torch")
    unchanged, agent_steps = fn(rcw, oracle, **kw)
    print(f"{name}: {unchanged} of {agent_steps} agent-steps left the frame unchanged")


SMALL = [
    ("64 rows (four columns a chunk), 100 columns", dict(height_camera_view_pu=64, height_tile_map_tu=7, width_tile_map_tu=11, num_rays=100), 44),
    ("128 rows (two columns a chunk)", dict(height_camera_view_pu=128, **CFG2), 36),
    ("512 rows, a workgroup per agent", dict(height_camera_view_pu=512, height_tile_map_tu=9, width_tile_map_tu=9, num_rays=300), 20),
    ("Float64", dict(T="Float64", **CFG2), 28),
    ("Float64, 600 columns, a workgroup per agent", dict(T="Float64", height_tile_map_tu=8, width_tile_map_tu=8, num_rays=600), 12),
    ("1500 columns: the reloaded slot-0 words", dict(height_tile_map_tu=9, width_tile_map_tu=8, num_rays=1500, num_directions=64), 12),
    ("cfg3, a workgroup per agent", dict(**CFG3), 24),
]


@pytest.mark.parametrize("fn", [rollout_resets_and_states, rollout_buffers], ids=["resets", "buffers"])
@pytest.mark.parametrize("name,kw,batch", SMALL, ids=[s[0] for s in SMALL])
def test_small_batches_on_request(rcw, oracle, name, kw, batch, fn):
    """The other camera heights (rcw_fill_window_cast_kernel, M = 4, 2, 1), Float64, both casting shapes, more than 1024 view columns:
    small batches that take the one-launch form on request."""
    pytest.importorskip("torch")
    unchanged, agent_steps = fn(rcw, oracle, batch=batch, by_rule=False, one_in=None, out_of_bounds=1, **kw)
    print(f"{name}: {unchanged} of {agent_steps} agent-steps left the frame unchanged")


@pytest.mark.parametrize("name,kw,batch", SMALL[:3], ids=[s[0] for s in SMALL[:3]])
def test_small_batches_episodes_restart(rcw, oracle, name, kw, batch):
    pytest.importorskip("torch")
    if kw["height_tile_map_tu"] != 8:                          # (set_state_near_the_goal is laid out for the 8 x 8 room)
        kw = dict(kw, height_tile_map_tu=8, width_tile_map_tu=8)
    rollout_episodes(rcw, oracle, batch=batch, by_rule=False, one_in=None, out_of_bounds=1, **kw)


def test_the_skip_is_taken_and_the_contract_is_as_written(rcw, oracle):
    """White box.  Behind a primed step the frames are overwritten with a sentinel through the torch alias — which the contract forbids
    without telling the library — and a step follows: every agent then holds either the oracle's frame or the sentinel in EVERY pixel,
    the sentinel only where the oracle's frame is the same before and after that step, and at least one agent in 32 does.
    update_camera_view_ repairs all of them; with bind_obs called after the overwriting no sentinel survives."""
    torch = pytest.importorskip("torch")
    B = 1024
    for tell in (False, True):
        r = Rollout(rcw, oracle, B, 11, 12, out_of_bounds=1, **CFG2)
        _one_launch(r, True)
        r.steps(3, "first")
        alias = r.env.camera_view.torch().view(torch.int32)
        alias.fill_(SENTINEL - (1 << 32))
        torch.cuda.synchronize()
        if tell:
            r.env.bind_obs(None)
        before = r.orc.camera_view.copy()
        a = r.rng.integers(1, 5, B).astype(np.uint8)
        rcw.act_(r.env, a); assert r.orc.step(a) == 0
        got, want = r.env.camera_view_host(), r.orc.camera_view
        same = (want == before).reshape(B, -1).all(axis=1)
        right = (got == want).reshape(B, -1).all(axis=1)
        kept = (got == SENTINEL).reshape(B, -1).all(axis=1)
        print(f"bind_obs in between: {tell}; {int(same.sum())} agents unchanged in the oracle, {int(kept.sum())} frames not stored")
        assert (right | kept).all(), "an agent holds neither the oracle's frame nor the sentinel in every pixel"
        assert not (kept & ~same).any(), "a frame was left alone that the step changed"
        if tell:
            assert not kept.any() and right.all()
        else:
            assert int(kept.sum()) * 32 >= B, f"{int(kept.sum())} of {B} frames skipped: fewer than one in 32"
            rcw.update_camera_view_(r.env)
            np.testing.assert_array_equal(r.env.camera_view_host(), want)
        r.steps(3, "further steps")
        r.env.close()
