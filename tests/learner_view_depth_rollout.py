"""The rollouts of the depth plane's GPU tests (tests/test_gpu_learner_view_depth.py) — test infrastructure, importable without a GPU:
tests/test_learner_view_depth_spec.py rehearses every one of them on the CPU oracle alone.

A rollout sets the view, steps four times under auto_reset, resets the agents of a mask (those outside it keep every byte) and steps
three more times; after every call the engine's state, its column descriptors and every byte of its learner view are compared with the
oracle's state and the numpy restatement of the view over the oracle's descriptors (tests/learner_view_depth_ref.py)."""
import numpy as np

import learner_view_depth_ref as LD
import learner_view_stack_ref as LS
from helpers import CFG1, CFG2, assert_state_equal

ODD = dict(CFG1, num_rays=33, height_camera_view_pu=37)        # 33 columns x 37 rows: neither a power of two
# 5600 columns x 16 rows: the column tables pass 64 KiB of LDS.  height_line_pu is camera_height_tile_wu * num_rays / (2 fov distance) — the
# NUMBER OF RAYS, not of rows, scales it —, so with the default camera height of 1 every wall of the 8 x 8 room would fill its 16 rows
# (4200 / distance); 1/256 brings a column's line to 16.4 / distance rows: ceiling and floor beyond a distance of 1.1
MANY_RAYS = dict(height_tile_map_tu=8, width_tile_map_tu=8, num_rays=5600, height_camera_view_pu=16, camera_height_tile_wu=1.0 / 256)
DEPTH_TABLE = dict(height_tile_map_tu=8, width_tile_map_tu=8, num_rays=5000, height_camera_view_pu=1500)   # ... only with the depth table
HUGE_BOX = dict(height_tile_map_tu=8, width_tile_map_tu=8, num_rays=4096, height_camera_view_pu=2048)
AGENT_LDS = lambda cfg, size: (3 * cfg["num_rays"] + size[0] + size[1] + 2) * 4       # rcw_view_agent_kernel's tables without depth

# (cfg, agents, seed of the worlds, seed of the actions, near the goal): every rollout a test of this file runs
ROLLOUTS = {"cfg1": (CFG1, 5, 5, 8, False), "odd": (ODD, 5, 1, 8, False), "many rays": (MANY_RAYS, 3, 1, 8, False),
            "depth table": (DEPTH_TABLE, 2, 1, 8, False), "huge box": (HUGE_BOX, 2, 1, 8, False),
            "cfg2 near the goal": (CFG2, 7, 1, 8, True), "cfg1 near the goal": (CFG1, 5, 1, 8, True),
            "many rays near the goal": (MANY_RAYS, 3, 1, 8, True), "cfg2": (CFG2, 6, 1, 8, False), "cfg2 x 64": (CFG2, 64, 1, 8, False),
            # more (agent, plane) items than the full kernel's grid of 4 workgroups a CU: its sweep's second trip, the masked reset's
            # `continue` behind the prefetch included
            "cfg1 x 1100": (CFG1, 1100, 5, 8, False)}
FULL_SIZE_PIXELS = 1 << 22                                   # frames of more pixels than this, at full size: LD.full_size for LD.view


class DepthRollout:
    """engine (rcw = None: the oracle alone), oracle and, for k > 1, the stack model side by side"""

    def __init__(self, rcw, oracle, rollout, fmt="depth", size=None, layout="chw", k=1, camera_view=True, form=None):
        cfg, batch, seed, rng_seed, self.near_the_goal = ROLLOUTS[rollout]
        self.orc = oracle.OracleBatch(batch, seed=seed, auto_reset=1, out_of_bounds=1, **cfg)
        self.env = rcw.SingleRoomModule.SingleRoom(batch=batch, seed=seed, auto_reset=True, out_of_bounds=1, **cfg) if rcw is not None else None
        self.rng = np.random.default_rng(rng_seed)
        self.rcw, self.B, self.camera_view = rcw, batch, camera_view
        self.fmt, self.layout, self.k = fmt, layout, k
        self.size = size or (self.orc.Hc, self.orc.N)
        self.seen = []                                       # the oracle's height_line_pu at every point the view is compared
        self.auto_restarts = 0
        if self.env is not None and form is not None:
            self.env.set_step_form(form)
        if self.near_the_goal:                               # every agent four forward moves from its goal (the 8 x 8 room)
            g = np.tile(np.array([[4, 6]], np.int32), (batch, 1)); p = np.tile(np.array([[3.5, 4.5]], np.float32), (batch, 1))
            d = np.full(batch, 32, np.int32)
            if self.env is not None:
                self.env.set_state(g, p, d)
            self.orc.set_state(g, p, d)
        if self.env is not None:
            self.env.set_learner_view(fmt, size, layout, camera_view=camera_view, stack=k)
            info = self.env.learner_view_info()
            assert info == {"format": fmt, "layout": layout, "size": tuple(self.size), "camera_view": camera_view}
        self.model = LS.StackModel(k, self.single("chw"), self.orc.episode) if k > 1 and self.env is not None else None

    def single(self, layout=None):
        o = self.orc
        if tuple(self.size) == (o.Hc, o.N) and self.B * o.Hc * o.N > FULL_SIZE_PIXELS:
            # a thousand agents at full size: the same bytes (tests/test_learner_view_depth_spec.py) without view()'s int64 box sums
            return LD.full_size(o.col_height, o.col_colour, o.cfg, o.Hc, self.fmt, layout or self.layout)
        return LD.view(o.col_height, o.col_colour, o.cfg, o.Hc, self.fmt, self.size, layout or self.layout)

    def check(self, where):
        self.seen.append(self.orc.col_height.copy())
        if self.env is None:
            return None
        assert_state_equal(self.env, self.orc, frames=self.camera_view, where=where)    # (env.columns() against the oracle's among the rest)
        got = self.env.learner_view_host()
        want = self.single() if self.model is None else self.model.stack
        assert got.shape == want.shape, (got.shape, want.shape, where)
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            raise AssertionError(f"{self.fmt} {self.size} {self.layout} k={self.k} {where}: {len(bad)} bytes differ, first at {bad[:6].tolist()}: "
                                 f"got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}")
        return got

    def actions(self, t):
        a = self.rng.integers(1, 5, self.B).astype(np.uint8)
        if self.near_the_goal and t < 4:
            a[::2] = 1                                       # every other agent walks to its goal: auto_reset restarts it in the step after
        return a

    def step(self, t, where):
        a = self.actions(t)
        ep = self.orc.episode.copy()
        if self.env is not None:
            self.rcw.act_(self.env, a)
        assert self.orc.step(a) == 0
        self.auto_restarts += int((self.orc.episode != ep).sum())
        if self.model is not None:
            self.model.push(self.single("chw"), self.orc.episode)
        return self.check(where)

    def run(self):
        self.check("after set_learner_view")
        for t in range(4):
            self.step(t, f"step {t}")
        mask = np.zeros(self.B, np.uint8); mask[::3] = 1
        before = self.env.learner_view_host() if self.env is not None else None
        if self.env is not None:
            self.rcw.reset_(self.env, mask=mask, seed=99)
        self.orc.reset(mask=mask, seed=99)
        if self.model is not None:
            self.model.refill(self.single("chw"), mask, self.orc.episode)
        after = self.check("after a masked reset")
        if self.env is not None:
            np.testing.assert_array_equal(after[mask == 0], before[mask == 0])         # outside the mask: every byte kept
            if self.k > 1:
                one = self.single("chw")
                c = one.shape[1]
                for s in range(self.k):
                    np.testing.assert_array_equal(after[mask == 1, s * c:(s + 1) * c], one[mask == 1])
        for t in range(4, 7):
            self.step(t, f"step {t}")
        if self.near_the_goal:
            assert self.auto_restarts >= 1, "no agent restarted under auto_reset: the slot rule across a restart was not exercised"
        return self

    def close(self):
        if self.env is not None:
            self.env.close()
        self.orc.close()
