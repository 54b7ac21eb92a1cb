"""The learner view's depth plane on the GPU, on hand-made column descriptors (tests/learner_view_depth_cases.py) through
env.expand_columns_view: what no rollout in an 8 x 8 room produces — a height_line_pu at or below zero (max(hl, 0), u = 0, a padding
beyond half the column), every u of 0 .. Hc through each kernel of csrc/rcw_view.hip, both sides of every step of the depth byte at the
heights where a launch rule or an argument about the arithmetic ends (the agent kernels' 64 KiB of LDS, the full kernel's Hc < 32768,
rcw_create's 2^20), the full kernel's sweep past its first trip, and buffers that are not 16-byte aligned.

Every byte is compared with the numpy restatement (tests/learner_view_depth_ref.py): LD.view's counting reading and, where it is quick,
the pixel-by-pixel one; tests/test_learner_view_depth_spec.py holds the two against each other on the same cases without a GPU."""
import numpy as np
import pytest

import learner_view_depth_cases as K
import learner_view_depth_ref as LD
from helpers import CFG1, assert_state_equal
from learner_view_depth_rollout import AGENT_LDS, DEPTH_TABLE, MANY_RAYS, ROLLOUTS, DepthRollout

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


class Pixels:
    """the pixel-by-pixel reading of one descriptor set (LD.view's `depth`): its (n, Hc, N) image is written once, a size's boxes once"""

    def __init__(self, hl, Hc):
        self.hl, self.frames, self.sizes = hl, LD.depth_frames(hl, Hc), {}

    def __call__(self, col_h, Hc, size):
        assert col_h is self.hl
        if size not in self.sizes:
            self.sizes[size] = LD.from_depth_frames(self.frames, size)
        return self.sizes[size]


class Case:
    """a handle of `cfg` and a descriptor set in device memory"""

    def __init__(self, rcw, torch, cfg, hl, cid, batch=1, pixel_rows=None):
        self.env = rcw.SingleRoomModule.SingleRoom(batch=batch, seed=1, **cfg)
        self.torch, self.hl, self.cid = torch, hl, cid
        self.Hc, self.N = self.env.cfg.height_camera_view_pu, self.env.cfg.num_rays
        assert hl.shape == cid.shape and hl.shape[1] == self.N
        self.th, self.tc = torch.from_numpy(hl).cuda(), torch.from_numpy(cid).cuda()
        self.part = hl if pixel_rows is None else hl[:pixel_rows]          # the descriptor rows the pixel reading takes (0: none)
        self.pixels = Pixels(self.part, self.Hc) if len(self.part) else None

    def render(self, fmt, size, layout, camera_view=True, th=None, tc=None, out=None):
        self.env.set_learner_view(fmt, size, layout, camera_view=camera_view)
        got = self.env.expand_columns_view(self.th if th is None else th, self.tc if tc is None else tc, out=out)
        self.torch.cuda.synchronize()
        return got.cpu().numpy()

    def check(self, fmt, size, layout, what, camera_view=True, rows=32):
        full = size or (self.Hc, self.N)
        got = self.render(fmt, size, layout, camera_view)
        want = K.view_in_chunks(self.hl, self.cid, self.env.cfg, self.Hc, fmt, full, layout, rows=rows)
        msg = K.first_difference(got, want, self.hl, self.Hc, full, layout, f"{what}: {fmt}")
        assert msg is None, msg
        if self.pixels is not None:
            n = len(self.part)
            want = LD.view(self.part, self.cid[:n], self.env.cfg, self.Hc, fmt, full, layout, depth=self.pixels)
            msg = K.first_difference(got[:n], want, self.part, self.Hc, full, layout, f"{what}, pixel by pixel: {fmt}")
            assert msg is None, msg
        return got

    def close(self):
        self.env.close()


# ---- (a) every u, through every kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K.EVERY_U))
def test_every_u(rcw, torch, name):
    """hl = -2 .. Hc + 2 and eight extremes (INT_MAX, INT_MIN, +-2^30, -Hc - 1, -Hc, -Hc + 1, 2 Hc): 16 columns x 1021 rows (a prime) at full size
    through rcw_view_full_kernel and at five reduced sizes through rcw_view_agent_kernel; 33 x 37 through the agent kernel at full size;
    5600 x 16 and 5000 x 1500 through rcw_view_box_kernel; 4096 x 2048, where one descriptor row holds every u, at one pixel through its
    64-bit instantiation and at two through the agent kernel's largest 32-bit sums"""
    cfg, sizes = K.EVERY_U[name]
    Hc, N = cfg.get("height_camera_view_pu", 256), cfg["num_rays"]
    if cfg is MANY_RAYS:
        assert all(AGENT_LDS(cfg, size) > 64 * 1024 for size, _ in sizes)
    if cfg is DEPTH_TABLE:
        assert all(AGENT_LDS(cfg, size) <= 64 * 1024 < AGENT_LDS(cfg, size) + (Hc + 1) * 4 for size, _ in sizes)
    if name == "prime, the agent kernel":
        assert all(K.agent_lds(N, Hc, size) <= 64 * 1024 for size, _ in sizes)
    if name == "huge box, sums of 64 bits":                             # (1, 1): 257 n >= 2^31, 64-bit sums; (1, 2): the largest box of 32-bit sums,
        assert 257 * Hc * N >= 2 ** 31 > 257 * Hc * (N // 2)            # which the agent kernel still takes (255 n = 1.07e9 in a uint32)
        assert K.agent_lds(N, Hc, (1, 2)) <= 64 * 1024
    hl, cid = K.every_u(Hc, N)
    assert K.holds(hl, Hc)["distinct u"] == Hc + 1
    case = Case(rcw, torch, cfg, hl, cid, batch=2)
    for size, formats in sizes:
        for fmt, layout in formats:
            case.check(fmt, size, layout, name)
    case.close()


# ---- (b) the limits of Hc ----------------------------------------------------------------------------------------------------------------
AGENT_LAST = K.largest_agent_Hc(K.LIMIT_RAYS, (1, 1))         # the launcher's rule (view_agent_lds), restated in K.agent_lds


def limits_of(rcw, torch, Hc, pixel_rows):
    """both sides of every step of the depth byte, and the column rule's edges, at a height of Hc: (255, 16), (7, 16) and (1, 1) in every
    format and layout; the middle row of the (255, 16) view is the wall's own byte (K.middle_row: no box code)"""
    hl, cid = K.thresholds(Hc, K.LIMIT_RAYS)
    case = Case(rcw, torch, K.limit(Hc), hl, cid, pixel_rows=pixel_rows)
    columns, D = K.middle_row(hl, Hc)
    assert columns.sum() >= 2 * 254
    for size in K.LIMIT_SIZES:
        for fmt, layout in K.ALL:
            got = case.check(fmt, size, layout, f"Hc = {Hc}", camera_view=False)
            if size == (255, 16):
                mid = got[:, -1, 127, :] if layout == "chw" else got[:, 127, :, -1]
                bad = np.argwhere(columns & (mid != D))
                assert len(bad) == 0, (f"Hc = {Hc} {fmt} {layout}: row 127 is not depth_byte(u) in {len(bad)} columns, first (row, column) "
                                       f"{bad[0].tolist()}: hl = {hl[tuple(bad[0])]}, got {mid[tuple(bad[0])]}, want {D[tuple(bad[0])]}")
    return case


@pytest.mark.parametrize("Hc", [AGENT_LAST, AGENT_LAST + 1, K.FULL_KERNEL_LAST, K.FULL_KERNEL_LAST + 1])
def test_the_limits_of_Hc(rcw, torch, Hc):
    """16331: the last height whose depth table the agent kernel takes (at (1, 1); every other size of it, and 16332, go to the box kernel);
    32767: the full kernel's last height, rendered at full size too (depth, CHW: 17 MB); 32768: the first one it refuses"""
    assert (AGENT_LAST, K.FULL_KERNEL_LAST) == (16331, 32767)
    assert K.agent_lds(16, AGENT_LAST, (1, 1)) <= 64 * 1024 < K.agent_lds(16, AGENT_LAST, (7, 16))
    case = limits_of(rcw, torch, Hc, pixel_rows=None if Hc <= AGENT_LAST + 1 else 8)
    if Hc == K.FULL_KERNEL_LAST:
        case.check("depth", None, "chw", f"Hc = {Hc}, the full kernel", camera_view=False, rows=8)
    case.close()


def test_a_height_of_2_to_the_20(rcw, oracle, torch):
    """rcw_create's largest height_camera_view_pu, and the largest depth_byte's Float32 quotient is argued for: a handle of it is created,
    renders the thresholds (the counting reading alone: the pixel one walks a million rows a column) — (1, 1) a box of 2^24 pixels, 64-bit
    sums — and steps under RCW_VIEW_ONLY against the oracle"""
    Hc = K.CREATE_LIMIT
    assert 257 * Hc * K.LIMIT_RAYS >= 2 ** 31 > 255 * Hc + Hc // 2
    case = limits_of(rcw, torch, Hc, pixel_rows=0)
    env = case.env
    orc = oracle.OracleBatch(1, seed=1, **K.limit(Hc))
    env.set_learner_view("depth", (255, 16), "chw", camera_view=False)
    for a in (2, 1, 3):
        act = np.array([a], np.uint8)
        rcw.act_(env, act)
        assert orc.step(act) == 0
        assert_state_equal(env, orc, frames=False, where=f"action {a}")
        want = LD.view(orc.col_height, orc.col_colour, orc.cfg, Hc, "depth", (255, 16))
        msg = K.first_difference(env.learner_view_host(), want, orc.col_height, Hc, (255, 16), "chw", f"after action {a}")
        assert msg is None, msg
    orc.close()
    case.close()


# ---- (c) the full kernel beyond one sweep ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,CT", [("depth", 1), ("grayd", 2), ("rgbd", 4)])
def test_the_full_kernel_beyond_one_sweep(rcw, torch, fmt, CT):
    """256 columns x 257 rows: items of 128 rows, three a plane, the last of one row; rows of random descriptors, no two equal, for at least
    2.5 trips of `it += gridDim.x` (a grid of 4 workgroups a CU) — the item -> (agent, plane, block) mapping by CT and the prefetch of the
    next item's descriptors on the second and third trip"""
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    Hc, N = K.SWEEP["height_camera_view_pu"], K.SWEEP["num_rays"]
    blocks, rows_item = K.full_kernel_blocks(N, Hc)
    assert blocks >= 3 and Hc - (blocks - 1) * rows_item == 1
    n = K.sweep_rows(CT, cus, N, Hc)
    assert n * CT * blocks >= 2.5 * 4 * cus and n * CT * Hc * N < 128 << 20
    hl, cid = K.random_rows(n, Hc, N, seed=CT)
    case = Case(rcw, torch, K.SWEEP, hl, cid, pixel_rows=4)
    got = case.check(fmt, None, "chw", f"{n} rows")
    tail = slice(n - 4, n)                                                   # the pixel reading of the last rows too: the last trip's items
    want = LD.view(hl[tail], cid[tail], case.env.cfg, Hc, fmt, (Hc, N), "chw", depth=LD.by_frames)
    msg = K.first_difference(got[tail], want, hl[tail], Hc, (Hc, N), "chw", f"the last 4 of {n} rows, pixel by pixel")
    assert msg is None, msg
    case.close()


@pytest.mark.parametrize("fmt,CT", [("depth", 1), ("rgbd", 4)])
def test_a_rollout_of_more_agents_than_workgroups(rcw, oracle, torch, fmt, CT):
    """1100 agents of 64 columns x 256 rows at full size, an item a plane: the sweep's second trip in the step and, under the masked reset,
    its `continue` behind the prefetch"""
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    assert ROLLOUTS["cfg1 x 1100"][:2] == (CFG1, 1100) and 1100 * CT > 4 * cus
    assert K.full_kernel_blocks(64, 256)[0] == 1
    d = DepthRollout(rcw, oracle, "cfg1 x 1100", fmt=fmt, size=None, layout="chw").run()
    d.close()


# ---- (d) buffers that are not 16-byte aligned --------------------------------------------------------------------------------------------
GUARD = 64
UNALIGNED = [("gray", None, "chw", (1, 2, 4, 8)), ("rgb", None, "chw", (1, 2, 4, 8)), ("depth", None, "chw", (1, 2, 4, 8)),
             ("rgbd", None, "chw", (1, 2, 4, 8)), ("rgbd", None, "hwc", (1, 2, 4, 8)), ("rgbd", (37, 53), "hwc", (1, 4))]


@pytest.mark.parametrize("fmt,size,layout,offsets", UNALIGNED, ids=[f"{u[0]} {u[2]} {u[1] or 'full'}" for u in UNALIGNED])
def test_buffers_that_are_not_16_byte_aligned(rcw, torch, fmt, size, layout, offsets):
    """64 columns x 256 rows: at full size an unaligned view or descriptor buffer goes to the agent kernel instead of the full kernel, and a
    view that is not 4-byte aligned turns RGB-D HWC's 4-byte store into byte stores (offsets 1 and 2; 4 and 8 keep the word) — the same
    bytes either way, and none outside the view"""
    hl, cid = K.random_rows(3, 256, 64, seed=3)
    hl[0, :10] = [0, -1, 1, 254, 255, 256, -256, -257, 2 ** 31 - 1, -(2 ** 31)]
    case = Case(rcw, torch, CFG1, hl, cid)
    base = case.check(fmt, size, layout, "aligned")
    nbytes = base.size

    def shifted(src, off):                                                   # `src` again, `off` elements behind a 16-byte boundary
        flat = torch.empty(src.numel() + off, dtype=src.dtype, device="cuda")
        assert flat.data_ptr() % 16 == 0
        flat[off:] = src.ravel()
        t = flat[off:].view(src.shape)
        assert t.is_contiguous() and t.data_ptr() % 16 == (off * src.element_size()) % 16 != 0
        return t

    def run(off, th=None, tc=None):
        flat = torch.full((GUARD + off + nbytes + GUARD + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        assert flat.data_ptr() % 16 == 0
        out = flat[GUARD + off:GUARD + off + nbytes].view(base.shape)
        assert out.is_contiguous() and out.data_ptr() % 16 == off
        got = case.render(fmt, size, layout, th=th, tc=tc, out=out)
        where = f"{fmt} {layout} {size}: view at byte offset {off}, hl {'shifted' if th is not None else 'aligned'}, cid {'shifted' if tc is not None else 'aligned'}"
        msg = K.first_difference(got, base, hl, 256, size or (256, 64), layout, where)
        assert msg is None, msg
        host = flat.cpu().numpy()
        assert (host[:GUARD + off] == 0xA5).all() and (host[GUARD + off + nbytes:] == 0xA5).all(), f"{where}: bytes outside the view written"
        np.testing.assert_array_equal(host[GUARD + off:GUARD + off + nbytes], base.ravel())

    run(0)
    for off in offsets:
        run(off)
    th, tc = shifted(case.th, 1), shifted(case.tc, 1)
    assert th.data_ptr() % 16 == 4 and tc.data_ptr() % 16 == 1
    run(0, th=th)
    run(0, tc=tc)
    run(offsets[0], th=th, tc=tc)
    case.close()
