"""Hand-made column descriptors for the depth plane's GPU tests (tests/test_gpu_learner_view_depth_descriptors.py) — test infrastructure,
importable without a GPU, beside learner_view_depth_rollout.py: tests/test_learner_view_depth_spec.py checks on the CPU that every
builder holds what it claims and that the two numpy readings (tests/learner_view_depth_ref.py) agree on every case.

A rollout in an 8 x 8 room never produces a height_line_pu at or below zero, and only some of the Hc + 1 inverse depths u; env.expand_columns_view
renders the handle's view of ANY descriptors in device memory, so these builders lay out the ones the contract (include/rcw.h) has a clause for.
Each returns (hl int32 (n, N), cid uint8 (n, N))."""
import numpy as np

import learner_view_depth_ref as LD
import learner_view_ref as LV
from learner_view_depth_rollout import DEPTH_TABLE, HUGE_BOX, MANY_RAYS, ODD

INT_MAX, INT_MIN = 2 ** 31 - 1, -(2 ** 31)


def _lay(values, N):
    """row-major into ceil(len / N) rows, the tail repeating from the start; cid = (row + column) % 4"""
    values = np.asarray(values, dtype=np.int64)
    assert values.min() >= INT_MIN and values.max() <= INT_MAX
    n = -(-len(values) // N)
    hl = np.resize(values, (n, N)).astype(np.int32)
    cid = ((np.arange(n)[:, None] + np.arange(N)[None, :]) % 4).astype(np.uint8)
    return hl, cid


def extremes(Hc):
    return [INT_MAX, INT_MIN, 2 ** 30, -(2 ** 30), -Hc - 1, -Hc, -Hc + 1, 2 * Hc]


def every_u(Hc, N):
    """every hl in -2 .. Hc + 2 — every u = min(max(hl, 0), Hc) with both clamps, every pad from 0 to Hc / 2 + 1 — and eight extremes"""
    return _lay(list(range(-2, Hc + 3)) + extremes(Hc), N)


def threshold_values(Hc):
    """for D = 1 .. 255 the smallest u with depth_byte(u) = D, and u - 1: 510 values, both sides of every step of D"""
    assert Hc >= 255                                          # (below, D skips values: not every D has a u)
    out = []
    for D in range(1, 256):
        u = -(-(D * Hc - Hc // 2) // 255)                     # ceil((D Hc - Hc // 2) / 255): 255 u + Hc // 2 >= D Hc
        assert 1 <= u <= Hc and int(LD.depth_byte(u, Hc)) == D and int(LD.depth_byte(u - 1, Hc)) == D - 1, (Hc, D, u)
        out += [u, u - 1]
    return out


def thresholds(Hc, N):
    return _lay(threshold_values(Hc) + [0, 1, Hc - 2, Hc - 1, Hc, Hc + 1, -1, -Hc, INT_MIN, INT_MAX], N)


def random_rows(n, Hc, N, seed):
    """hl uniform in [-Hc, 2 Hc], no two rows equal: bytes rendered from another agent's descriptors differ"""
    rng = np.random.default_rng(seed)
    hl = rng.integers(-Hc, 2 * Hc + 1, (n, N)).astype(np.int32)
    cid = rng.integers(0, 4, (n, N)).astype(np.uint8)
    assert len(np.unique(hl, axis=0)) == n
    return hl, cid


def holds(hl, Hc):
    """what a descriptor set exercises of the column rule"""
    hl = np.asarray(hl, dtype=np.int64)
    pad = LV.padding(Hc, hl)
    u = np.clip(hl, 0, Hc)
    return {"hl < 0": bool((hl < 0).any()), "u == 0": bool((u == 0).any()), "pad == Hc": bool((pad == Hc).any()),
            "pad > Hc / 2": bool((2 * pad > Hc).any()), "pad == 0 with u == Hc - 1": bool(((pad == 0) & (u == Hc - 1)).any()),
            "distinct u": len(np.unique(u))}


def middle_row(hl, Hc, h=255, r=127):
    """The third reading of thresholds' cases at a view of (h, N) rows — a box is one column wide —: (columns, D) with `columns` the (n, N)
    mask of the columns whose line covers the whole box of output row r, i.e. hl >= (rows of that box) + 2, and D = depth_byte(clip(hl, 0, Hc))
    the byte such a box averages to, whatever the box code does.  With r0 = r Hc // h and r1 = (r + 1) Hc // h the claim is pad <= r0 and
    r1 <= Hc - pad for those columns; it is asserted here, not assumed."""
    hl = np.asarray(hl, dtype=np.int64)
    rb = LV.row_bounds(Hc, h)
    r0, r1 = int(rb[r]), int(rb[r + 1])
    columns = hl >= (r1 - r0) + 2
    pad = LV.padding(Hc, hl)
    assert (pad[columns] <= r0).all() and (r1 <= Hc - pad[columns]).all(), (Hc, h, r, r0, r1)
    return columns, LD.depth_byte(np.clip(hl, 0, Hc), Hc).astype(np.uint8)


def first_difference(got, want, hl, Hc, size, layout, what=""):
    """None where got == want, else the message of DepthRollout.check with the first differing index's descriptor: the first column of its box,
    that column's hl and pad"""
    if got.shape != want.shape:
        return f"{what}: shape {got.shape}, want {want.shape}"
    if np.array_equal(got, want):
        return None
    bad = np.argwhere(got != want)
    i = tuple(bad[0])
    a, (r, c) = i[0], ((i[2], i[3]) if layout == "chw" else (i[1], i[2]))
    k = int(LV.row_bounds(np.asarray(hl).shape[1], size[1])[c])
    rows = LV.row_bounds(Hc, size[0])[r:r + 2].tolist()
    h0 = int(np.asarray(hl)[a, k])
    return (f"{what} {size} {layout}: {len(bad)} bytes differ, first at {bad[:6].tolist()}: got {got[i]}, want {want[i]}; "
            f"rows {rows} of image column {k} of descriptor row {a}: hl = {h0}, pad = {int(LV.padding(Hc, h0))}, Hc = {Hc}")


def view_in_chunks(hl, cid, cfg, Hc, fmt, size, layout="chw", depth=LD.from_descriptors, rows=32):
    """LD.view over `rows` descriptor rows at a time (its intermediates are int64 (rows, h, N, C))"""
    return np.concatenate([LD.view(hl[i:i + rows], cid[i:i + rows], cfg, Hc, fmt, size, layout, depth=depth) for i in range(0, len(hl), rows)])


# ---- the geometries of the GPU tests, shared with the CPU spec -------------------------------------------------------------------------
PRIME = dict(height_tile_map_tu=8, width_tile_map_tu=8, num_rays=16, height_camera_view_pu=1021)     # 16 columns x 1021 rows (a prime)
SWEEP = dict(height_tile_map_tu=8, width_tile_map_tu=8, num_rays=256, height_camera_view_pu=257)     # the full kernel: 128 rows an item, 3 blocks a plane
LIMIT_RAYS = 16

ALL = [(f, l) for f in ("depth", "rgbd", "grayd") for l in ("chw", "hwc")]
FULL = [("depth", "chw"), ("rgbd", "chw"), ("grayd", "chw"), ("depth", "hwc")]        # what the full-size kernel takes
# every_u through every kernel — name: (configuration, [(size, [(format, layout)])]), size None: full size
EVERY_U = {"prime, the full kernel": (PRIME, [(None, FULL)]),
           # 257 rows: odd and below 510, the one kind of height at which the middle row's De = depth_byte(1) is not the byte of u = 0 — what a
           # column of hl = INT_MIN shows there if its padding wraps (padding32's max(h, -Hc)); 270 values in two rows of 256 columns
           "256 x 257, the full kernel": (SWEEP, [(None, FULL)]),
           "prime, the agent kernel": (PRIME, [((1, 1), ALL), ((37, 5), ALL), ((1021, 1), ALL), ((1, 16), ALL), ((1020, 16), ALL)]),
           "odd, the agent kernel": (ODD, [((37, 33), ALL), ((20, 17), ALL), ((1, 1), ALL)]),
           "many rays, the box kernel": (MANY_RAYS, [((8, 700), ALL), ((16, 5600), ALL), ((5, 33), [("rgbd", "hwc")])]),
           "depth table, the box kernel": (DEPTH_TABLE, [((7, 300), [("grayd", "chw")])]),
           "huge box, sums of 64 bits": (HUGE_BOX, [((1, 1), ALL), ((1, 2), ALL)])}


def limit(Hc):
    return dict(height_tile_map_tu=8, width_tile_map_tu=8, num_rays=LIMIT_RAYS, height_camera_view_pu=Hc)


def agent_lds(N, Hc, size, depth=True):
    """view_agent_lds of csrc/rcw_view.hip: the bytes of the agent kernels' tables"""
    return (3 * N + size[0] + size[1] + 2 + (Hc + 1 if depth else 0)) * 4


def largest_agent_Hc(N, size):
    """the largest Hc whose depth table still fits the agent kernels' 64 KiB at `size`"""
    Hc = (64 * 1024) // 4 - (3 * N + size[0] + size[1] + 2) - 1
    assert agent_lds(N, Hc, size) <= 64 * 1024 < agent_lds(N, Hc + 1, size)
    return Hc


FULL_KERNEL_LAST = 32767                                   # rcw_view_full_eligible: Hc < 32768
CREATE_LIMIT = 2 ** 20                                     # rcw_create's largest height_camera_view_pu
LIMIT_SIZES = ((255, 16), (7, 16), (1, 1))


def full_kernel_blocks(N, Hc):
    """row blocks a plane of rcw_view_full_kernel: a workgroup of 256 lanes, N / 16 lanes a row, 8 passes an item"""
    rows_item = (256 // (N // 16)) * 8
    return -(-Hc // rows_item), rows_item


def sweep_rows(CT, cus, N=256, Hc=257):
    """descriptor rows for at least 2.5 sweeps of the full kernel's grid of 4 workgroups a CU"""
    blocks, _ = full_kernel_blocks(N, Hc)
    n = -(-10 * cus // (CT * blocks))
    assert n * CT * blocks >= 2.5 * 4 * cus
    return n
