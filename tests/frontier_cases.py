"""Hand-made seen maps for the frontier's flood — test infrastructure, not a test.  tests/test_gpu_frontier_handmade.py feeds them to
rcw_frontier_kernel through an edited row of the state archive (tests/snapshot_rows.py); tests/test_frontier_cases_spec.py holds the
conditions each family is built for, the host export against the numpy flood on every map, and that each family tells the wrong flood it
is meant to catch from the true one — all on the CPU.

An engine-made seen map holds the bytes 0 .. 3 inside a wall border.  These hold every byte, passable and unseen tiles in the first and
last row and column, as many sources and passable tiles as the queue has room for, floods hundreds of levels deep and levels wider than a
wavefront.  A family is a list of Case(name, H, W, maps uint8 (B, H, W)); `poses` (deep floods only) are the tiles agents are put on.

The kernel reads an agent's map sixteen bytes a lane where the map starts on a multiple of 16 bytes — agent a's starts at a H W behind
the array's base, itself a multiple of 16 — and a byte a lane elsewhere: `wide_path(a, H, W)`."""
from collections import namedtuple

import numpy as np

FREE, UNSEEN, WALL, GOAL = 1, 0, 2, 3
X = 0xFFFF

Case = namedtuple("Case", "name H W maps poses", defaults=(None,))


def wide_path(a, H, W):
    return (a * H * W) % 16 == 0


# ---- bytes: gadgets passable | v | unseen ---------------------------------------------------------------------------------------------
def gadget_slots(H, W):
    """[(i, j, flip)]: a gadget lies in row i, columns j .. j + 2 — v in the middle — even rows at columns 0 and 8, odd rows at 4 and 12, so
    that no two gadgets share an edge; flip: unseen | v | passable.  W >= 15."""
    assert W >= 15
    return [(i, j, k) for i in range(H) for k, j in enumerate((0, 8) if i % 2 == 0 else (4, 12))]


def gadget_map(H, W, values):
    """walls everywhere but one gadget a slot: values[s] is slot s's v"""
    m = np.full((H, W), WALL, np.uint8)
    for (i, j, flip), v in zip(gadget_slots(H, W), values):
        m[i, j:j + 3] = (UNSEEN, v, FREE) if flip else (FREE, v, UNSEEN)
    return m


def gadget_fields(m):
    """what the class of v makes of each gadget of m: [(v, v's tile index i + H j, (row, the columns of passable | v | unseen), the three
    field values in that order)] — a passable v is crossed, a v of 0 is itself the source, any other v keeps the flood out"""
    H, W = m.shape
    out = []
    for i, j, flip in gadget_slots(H, W):
        v = int(m[i, j + 1])
        want = (2, 1, 0) if v in (1, 3) else (1, 0, X) if v == 0 else (X, X, X)
        out.append((v, i + H * (j + 1), (i, (j + 2, j + 1, j) if flip else (j, j + 1, j + 2)), want))
    return out


def bytes_wide():
    """16 x 16, 256 agents: every map starts on a multiple of 16 bytes and a column is one lane's 16-byte load.  Row i — the tile index
    mod 16 — holds v = a + 37 i (+ 128 in the second gadget) mod 256 in agent a: over the batch every byte at every index mod 16, twice"""
    H = W = 16
    maps = np.stack([gadget_map(H, W, [(a + 37 * i + 128 * k) % 256 for i, _, k in gadget_slots(H, W)]) for a in range(256)])
    return [Case("bytes, 16 x 16, sixteen a lane", H, W, maps)]


def bytes_narrow():
    """17 x 15 (255 bytes a map), 67 agents: all but agents 0, 16, 32, 48, 64 start off a multiple of 16 and go a byte a lane; those five go
    sixteen a lane with a tail of 15 bytes.  34 gadgets a map, v = 34 a + s mod 256: agents 1 .. 8 alone hold every byte"""
    H, W = 17, 15
    maps = np.stack([gadget_map(H, W, [(34 * a + s) % 256 for s in range(len(gadget_slots(H, W)))]) for a in range(67)])
    return [Case("bytes, 17 x 15, a byte a lane", H, W, maps)]


# ---- border and wrap ------------------------------------------------------------------------------------------------------------------
WRAP_SHAPES = [(4, 4), (5, 3), (3, 6), (3, 85), (85, 3)]
RANDOM_SHAPES = [(3, 3), (4, 8), (8, 8), (3, 11), (5, 13), (17, 15), (16, 16)]    # H W = 9, 32, 64, 33, 65, 255, 256


def wrap_maps(H, W):
    """tests/test_frontier_spec.py's literal maps at H x W.  Returns (maps, want): want[k] = (tiles, {tile: field value}) — every other
    tile holds 0xFFFF"""
    maps, want = [], []

    def add(cells, tiles, field):
        m = np.full((H, W), WALL, np.uint8)
        for (i, j), v in cells.items():
            m[i, j] = v
        maps.append(m)
        want.append((tiles, field))

    for j in range(W - 1):                                                        # tile (H-1, j) and tile (0, j+1): one apart in linear order, no neighbours
        add({(H - 1, j): FREE, (0, j + 1): UNSEEN}, 0, {})
        add({(0, j + 1): FREE, (H - 1, j): UNSEEN}, 0, {})
    # a source in row 0 does not flood into the passable tile in front of it in linear order
    add({(0, 1): UNSEEN, (1, 1): FREE, (H - 1, 0): FREE}, 1, {(0, 1): 0, (1, 1): 1})
    # sources in the first row and column, in the last row and column
    add({(1, 1): FREE, (0, 1): UNSEEN, (1, 0): UNSEEN}, 2, {(0, 1): 0, (1, 0): 0, (1, 1): 1})
    add({(H - 2, W - 2): GOAL, (H - 1, W - 2): UNSEEN, (H - 2, W - 1): UNSEEN}, 2, {(H - 1, W - 2): 0, (H - 2, W - 1): 0, (H - 2, W - 2): 1})
    return np.stack(maps), want


def border_and_wrap():
    cases = [Case(f"wrap, {H} x {W}", H, W, wrap_maps(H, W)[0]) for H, W in WRAP_SHAPES]
    for H, W in RANDOM_SHAPES:                                                    # uniform over 0 .. 3 on ALL tiles, the border included
        rng = np.random.default_rng([H, W, 67])
        cases.append(Case(f"random, {H} x {W}", H, W, rng.integers(0, 4, (67, H, W)).astype(np.uint8)))
    return cases


# ---- a full queue ---------------------------------------------------------------------------------------------------------------------
FULL_SHAPES = [(17, 15), (16, 16), (3, 85), (85, 3)]


def full_queue():
    """checkerboards, passable on one parity and unseen on the other: every unseen tile is a source, every tile enters the queue"""
    cases = []
    for H, W in FULL_SHAPES:
        parity = np.add.outer(np.arange(H), np.arange(W)) % 2
        cases.append(Case(f"checkerboards, {H} x {W}", H, W, np.stack([np.where(parity == p, FREE, UNSEEN).astype(np.uint8) for p in (0, 1)])))
    return cases


# ---- deep floods ----------------------------------------------------------------------------------------------------------------------
def serpentine_path(H, W):
    """the tiles of a one-tile corridor down column 0, across at the bottom, up column 2, across at the top, ... in the order walked"""
    path = []
    for k, j in enumerate(range(0, W, 2)):
        rows = range(H) if k % 2 == 0 else range(H - 1, -1, -1)
        path += [(i, j) for i in rows]
        if j + 2 < W:
            path.append((path[-1][0], j + 1))
    return path


def corridor(H, W, path):
    m = np.full((H, W), WALL, np.uint8)
    for i, j in path[:-1]:
        m[i, j] = FREE
    m[path[-1]] = UNSEEN                                                          # the one source, at the corridor's end
    return m


def deep_case(H, W):
    """Two maps.  `whole`: the serpentine through every other column of the map, border included, its last tile unseen — H W deep as far as
    a one-tile corridor can be.  `short`: the same corridor ending in the interior, so that an agent — the archive admits interior poses
    only — can stand on the source, with a passable pocket behind walls further on.  The serpentine runs along the longer side (3 x 251:
    through every other column; 251 x 3: every other row, the transpose).  poses: {name: (map index, tile)}"""
    t = H > W
    h, w = (W, H) if t else (H, W)
    path = serpentine_path(h, w)
    inside = lambda p: 1 <= p[0] <= h - 2 and 1 <= p[1] <= w - 2
    # the short corridor ends in the middle of a column, six columns before the map does
    end = max(k for k, p in enumerate(path) if inside(p) and p[1] <= w - 7 and p[1] % 2 == 0 and p[0] == h // 2)
    short = path[:end + 1]
    pocket = (h // 2, short[-1][1] + 3)
    whole_map, short_map = corridor(h, w, path), corridor(h, w, short)
    short_map[pocket] = FREE
    deep = [p for p in path[:len(path) // 3] if inside(p)][0]                    # in the first third of the corridor: two thirds of it from the source
    poses = dict(deep=(0, deep), deep_short=(1, deep), source=(1, short[-1]), pocket=(1, pocket), wall=(0, (h // 2, 1) if h > 3 else (1, 1)))
    maps = np.stack([whole_map, short_map])
    if t:
        maps = np.ascontiguousarray(maps.transpose(0, 2, 1))
        poses = {k: (n, (p[1], p[0])) for k, (n, p) in poses.items()}
    return Case(f"serpentine, {H} x {W}", H, W, maps, poses)


DEEP_SHAPES = [(33, 33), (251, 3), (3, 251)]


def deep_floods():
    return [deep_case(H, W) for H, W in DEEP_SHAPES]


# ---- wide levels on a non-square map ---------------------------------------------------------------------------------------------------
def wide_levels():
    """40 x 120.  All passable but one unseen tile in the middle: diamonds of up to 80 tiles a level.  Its complement: all unseen but a
    passable cross, whose every neighbour is a source — more than 64, found in several passes over the seeds"""
    H, W = 40, 120
    room = np.full((H, W), FREE, np.uint8)
    room[20, 60] = UNSEEN
    cross = np.full((H, W), UNSEEN, np.uint8)
    cross[20, :] = FREE
    cross[:, 60] = FREE
    return [Case("a room and a cross, 40 x 120", H, W, np.stack([room, cross]))]


FAMILIES = dict(bytes_wide=bytes_wide, bytes_narrow=bytes_narrow, border_and_wrap=border_and_wrap, full_queue=full_queue, deep_floods=deep_floods,
                wide_levels=wide_levels)
