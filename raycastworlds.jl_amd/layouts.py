"""Wall layouts for `SingleRoom.set_walls`: host-side numpy, nothing here touches the device (`generated_maze` and
`generated_maze_key`, `generated_cave`, `generated_rooms`, `guide_rule` and `frontier_rule` call the library's handle-less host functions: no device either).

A layout is bool (H, W) with `walls[i-1, j-1]` = tile (i, j) is a WALL — the index order of `env.world.tile_map[b, 0]`.
Every generator returns the wall ring (SR:57-60) closed, as `rcw_set_walls` requires, and at least two free interior
tiles.  `is_connected` is the host-side answer to reachability, which the engine does not check.
"""
from __future__ import annotations

import numpy as np


def _check_size(H: int, W: int, least: int) -> None:
    if H < least or W < least:
        raise ValueError(f"a {H} x {W} tile map is too small for this layout (at least {least} x {least})")


def ring(H: int, W: int) -> np.ndarray:
    """The reference's map: the wall ring around an empty room (SR:57-60)."""
    _check_size(H, W, 3)
    w = np.zeros((H, W), dtype=bool)
    w[[0, -1], :] = True
    w[:, [0, -1]] = True
    return w


def four_rooms(H: int, W: int) -> np.ndarray:
    """A wall along the middle row and one along the middle column, each with one door in either half: four rooms, every
    one joined to its two neighbours.  Any H, W >= 5."""
    _check_size(H, W, 5)
    w = ring(H, W)
    ci, cj = H // 2, W // 2                       # the dividing row and column (0-based; interior since H, W >= 5)
    w[ci, :] = True
    w[:, cj] = True
    # doors: the middle of each of the four wall segments (segments are 1 .. c-1 and c+1 .. n-2, never empty)
    w[ci, (1 + cj - 1) // 2] = False
    w[ci, (cj + 1 + W - 2) // 2] = False
    w[(1 + ci - 1) // 2, cj] = False
    w[(ci + 1 + H - 2) // 2, cj] = False
    return w


def maze(H: int, W: int, rng) -> np.ndarray:
    """A perfect maze by the recursive backtracker (depth-first, an explicit stack) on the odd sub-grid: cells are the
    tiles with odd 0-based (i, j) inside the ring, a passage is the tile between two cells.  Connected by construction;
    a pure function of `rng` (a `numpy.random.Generator`).  Any H, W >= 5; with an even H or W the last interior row or
    column stays wall."""
    _check_size(H, W, 5)
    w = np.ones((H, W), dtype=bool)
    ni, nj = (H - 1) // 2, (W - 1) // 2           # cells along each axis: 0-based tiles 1, 3, ..., 2 n - 1 <= size - 2
    seen = np.zeros((ni, nj), dtype=bool)
    ci, cj = int(rng.integers(0, ni)), int(rng.integers(0, nj))
    seen[ci, cj] = True
    w[2 * ci + 1, 2 * cj + 1] = False
    stack = [(ci, cj)]
    steps = ((1, 0), (-1, 0), (0, 1), (0, -1))
    while stack:
        ci, cj = stack[-1]
        free = [(di, dj) for di, dj in steps
                if 0 <= ci + di < ni and 0 <= cj + dj < nj and not seen[ci + di, cj + dj]]
        if not free:
            stack.pop()
            continue
        di, dj = free[int(rng.integers(0, len(free)))]
        w[2 * ci + 1 + di, 2 * cj + 1 + dj] = False           # the passage
        ci, cj = ci + di, cj + dj
        w[2 * ci + 1, 2 * cj + 1] = False
        seen[ci, cj] = True
        stack.append((ci, cj))
    return w


def loops_word(loops) -> int:
    """The wall generator's `loops` as the UInt32 the rule compares with: a probability in [0, 1] scaled with
    min(int(p * 2^32), 2^32 - 1) (an int is taken as the word itself)."""
    if isinstance(loops, (int, np.integer)) and not isinstance(loops, bool):
        word = int(loops)
        if not 0 <= word <= 0xFFFFFFFF:
            raise ValueError(f"loops as an integer is the UInt32 word itself: 0 .. 2^32 - 1, got {loops}")
        return word
    p = float(loops)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"loops is a probability in [0, 1], got {loops}")
    return min(int(p * 2.0 ** 32), 0xFFFFFFFF)


def generated_maze_key(seed: int, global_agent: int, episode: int, levels: int = 0, first_level: int = 0, level_seed: int = 0):
    """(maze_key, level) of the wall generator (include/rcw.h, "the wall generator") for episode `episode` — the counter before
    the increment, `env.world.episode - 1` of a running episode — of global agent `global_agent` under `seed`; level is -1
    with `levels == 0`.  rcw_wall_generator_key: host arithmetic, no device."""
    import ctypes as C

    from . import _capi

    lib = _capi.load()
    key, level = C.c_uint64(), C.c_int32()
    rc = lib.rcw_wall_generator_key(int(seed), int(global_agent), int(episode), int(levels), int(first_level), int(level_seed),
                                    C.byref(key), C.byref(level))
    if rc != _capi.RCW_OK:
        raise ValueError(_capi.last_error(lib))
    return key.value, level.value


def generated_maze(maze_key: int, H: int, W: int, loops=0.0) -> np.ndarray:
    """The wall generator's maze of one 64-bit key, bool (H, W): the minimum spanning tree of the cell grid under the key's
    order words, plus the non-tree edges `loops` opens (a probability in [0, 1]; an int: the UInt32 word itself).
    rcw_wall_generator_layout: host arithmetic (Kruskal), no device — what an agent's `env.world.walls[a]` holds."""
    from . import _capi

    lib = _capi.load()
    out = np.empty((max(int(W), 0), max(int(H), 0)), dtype=np.uint8)   # tile (i, j), 0-based, at i + H j
    rc = lib.rcw_wall_generator_layout(int(H), int(W), int(maze_key), loops_word(loops), out.ctypes.data)
    if rc != _capi.RCW_OK:
        raise ValueError(_capi.last_error(lib))
    return np.ascontiguousarray(out.T != 0)


def generated_cave(key: int, H: int, W: int, fill=0.40, smooth: int = 2, return_fell_back: bool = False):
    """The wall generator's cave of one 64-bit key (`generated_maze_key` serves both families), bool (H, W): the interior filled
    with probability `fill` (an int: the UInt32 word itself), smoothed `smooth` times, pruned to its largest region — or, where that
    region is too small, the perfect maze of the key; `return_fell_back=True` returns (walls, fell_back).
    rcw_wall_caves_layout: host arithmetic (a queue flood fill), no device — what an agent's `env.world.walls[a]` holds."""
    import ctypes as C

    from . import _capi

    lib = _capi.load()
    out = np.empty((max(int(W), 0), max(int(H), 0)), dtype=np.uint8)   # tile (i, j), 0-based, at i + H j
    fell = C.c_int32()
    rc = lib.rcw_wall_caves_layout(int(H), int(W), int(key), loops_word(fill), int(smooth), out.ctypes.data, C.byref(fell))
    if rc != _capi.RCW_OK:
        raise ValueError(_capi.last_error(lib))
    walls = np.ascontiguousarray(out.T != 0)
    return (walls, bool(fell.value)) if return_fell_back else walls


def generated_rooms(key: int, H: int, W: int, room: int = 2, stop=0.25, doors=0.25, return_rooms: bool = False):
    """The wall generator's rooms of one 64-bit key (`generated_maze_key` serves every family), bool (H, W): the interior split
    recursively by walls on even lines, each with a door on an odd position and, with probability `doors`, a second one; a chamber
    other than the whole interior is left a room with probability `stop`, and no room side falls below `room` (`stop`, `doors`: an
    int is the UInt32 word itself); `return_rooms=True` returns (walls, number of rooms).
    rcw_wall_rooms_layout: host arithmetic (depth first off a stack), no device — what an agent's `env.world.walls[a]` holds."""
    import ctypes as C

    from . import _capi

    lib = _capi.load()
    out = np.empty((max(int(W), 0), max(int(H), 0)), dtype=np.uint8)   # tile (i, j), 0-based, at i + H j
    rooms = C.c_int32()
    rc = lib.rcw_wall_rooms_layout(int(H), int(W), int(key), int(room), loops_word(stop), loops_word(doors), out.ctypes.data, C.byref(rooms))
    if rc != _capi.RCW_OK:
        raise ValueError(_capi.last_error(lib))
    walls = np.ascontiguousarray(out.T != 0)
    return (walls, int(rooms.value)) if return_rooms else walls


def guide_rule(field, position, direction: int, directions_wu, position_increment: float, T="Float32"):
    """The guide's rule (include/rcw.h, "the guide") for ONE agent on the host: (action, heading) — action in 1..4, heading the 0-based
    direction index the guide wants, -1 where it has no advice.  `field`: uint16 (H, W), one agent's `env.goal_distance_field[b]`;
    `position`: (x, y) in world units; `direction`: the agent's 0-based heading; `directions_wu`: (nd, 2), `env.world.directions_wu`'s layout
    (row k the direction of index k); `T`: the world-unit type the rule computes in.  rcw_guide_rule: host arithmetic, no device."""
    import ctypes as C

    from . import _capi

    lib = _capi.load()
    real = np.float64 if str(T) in ("Float64", "float64", "<class 'numpy.float64'>", "<class 'float'>") else np.float32
    f = np.ascontiguousarray(np.asarray(field, dtype=np.uint16).T)         # tile (i, j), 0-based, at i + H j
    if f.ndim != 2:
        raise ValueError(f"one field (H, W) at a time, got {f.shape}")
    table = np.ascontiguousarray(directions_wu, dtype=real)                # entry k at (2 k, 2 k + 1)
    if table.ndim != 2 or table.shape[1] != 2:
        raise ValueError(f"directions_wu is (nd, 2), got {np.shape(directions_wu)}")
    action, heading = C.c_uint8(), C.c_int32()
    rc = lib.rcw_guide_rule(f.shape[1], f.shape[0], f.ctypes.data, float(position[0]), float(position[1]), 64 if real is np.float64 else 32,
                            int(direction), table.shape[0], table.ctypes.data, float(position_increment), C.byref(action), C.byref(heading))
    if rc != _capi.RCW_OK:
        raise ValueError(_capi.last_error(lib))
    return int(action.value), int(heading.value)


def frontier_rule(seen_map):
    """The frontier's flood (include/rcw.h, "the frontier") for ONE agent on the host: (field, tiles) — `field` uint16 (H, W), 0 on the
    unseen tiles next to a seen free one, on a seen free tile the moves to the nearest of them, 0xFFFF elsewhere; `tiles` how many hold 0.
    `seen_map`: uint8 (H, W), one agent's `env.seen_map[b]` (0 unseen, 1 free, 2 wall, 3 goal, 4 and above wall).  rcw_frontier_rule:
    host arithmetic, no device."""
    import ctypes as C

    from . import _capi

    lib = _capi.load()
    m = np.asarray(seen_map, dtype=np.uint8)
    if m.ndim != 2:
        raise ValueError(f"one seen map (H, W) at a time, got {m.shape}")
    H, W = m.shape
    lin = np.ascontiguousarray(m.T)                                        # tile (i, j), 0-based, at i + H j
    out = np.empty((W, H), dtype=np.uint16)
    tiles = C.c_int32()
    rc = lib.rcw_frontier_rule(H, W, lin.ctypes.data, out.ctypes.data, C.byref(tiles))
    if rc != _capi.RCW_OK:
        raise ValueError(_capi.last_error(lib))
    return np.ascontiguousarray(out.T), int(tiles.value)


def visit_cell(H: int, W: int, num_directions: int, sectors: int, position, direction: int, T=np.float32) -> int:
    """The visit map's cell rule (include/rcw.h, "the visit map") for ONE agent on the host: the 0-based cell `s*H*W + i + H*j` of an agent
    at `position` (x, y) facing the 0-based direction index `direction`, -1 where it has none (a position that is not finite, a tile off
    the map).  `env.visit_map[b].reshape(-1)` is NOT in this order; `env.visit_map_device` is.  rcw_visit_cell: host arithmetic, no device."""
    import ctypes as C

    from . import _capi

    lib = _capi.load()
    cell = C.c_int32()
    bits = 64 if np.dtype(T) == np.float64 else 32
    rc = lib.rcw_visit_cell(int(H), int(W), int(num_directions), int(sectors), float(position[0]), float(position[1]), bits, int(direction), C.byref(cell))
    if rc != _capi.RCW_OK:
        raise ValueError(_capi.last_error(lib))
    return int(cell.value)


def start_rule(walls, goal, key: int, lo: int = 1, hi=None):
    """The start rule (include/rcw.h, "the start rule") for ONE agent on the host: (tile, outcome) — `tile` the 1-based (i, j) the
    player is placed on, None where the drawn pose is kept; `outcome` 1 in the band, 2 clamped to the farthest tiles, 3 kept.  `walls`:
    (H, W), non-zero = wall, one agent's `env.world.walls[b]`; `goal`: its 1-based (i, j); `key`: the episode key of (seed, global agent
    id, episode counter before the start); `lo..hi` the band, `hi=None`: no upper bound.  rcw_start_rule: host arithmetic, no device."""
    import ctypes as C

    from . import _capi

    lib = _capi.load()
    w = np.asarray(walls) != 0
    if w.ndim != 2:
        raise ValueError(f"one layout (H, W) at a time, got {w.shape}")
    H, W = w.shape
    lin = np.ascontiguousarray(w.T, dtype=np.uint8)                        # tile (i, j), 0-based, at i + H j
    tile, outcome = C.c_int32(), C.c_int32()
    rc = lib.rcw_start_rule(lin.ctypes.data, H, W, int(goal[0]), int(goal[1]), int(key) & (2 ** 64 - 1), int(lo),
                            _capi.RCW_START_DISTANCE_MAX if hi is None else int(hi), C.byref(tile), C.byref(outcome))
    if rc != _capi.RCW_OK:
        raise ValueError(_capi.last_error(lib))
    t = int(tile.value)
    return (None if t < 0 else (t % H + 1, t // H + 1)), int(outcome.value)


def is_connected(walls) -> bool:
    """True where every free tile of the layout (bool (H, W)) can be reached from every other through free tiles that
    share an edge — the moves `act!` can make between tile centres.  A layout without a free tile is not connected."""
    w = np.asarray(walls) != 0
    if w.ndim != 2:
        raise ValueError(f"one layout (H, W) at a time, got {w.shape}")
    free = np.argwhere(~w)
    if len(free) == 0:
        return False
    H, W = w.shape
    seen = np.zeros_like(w)
    start = tuple(free[0])
    seen[start] = True
    todo = [start]
    while todo:
        i, j = todo.pop()
        for a, b in ((i + 1, j), (i - 1, j), (i, j + 1), (i, j - 1)):
            if 0 <= a < H and 0 <= b < W and not w[a, b] and not seen[a, b]:
                seen[a, b] = True
                todo.append((a, b))
    return bool(seen.sum() == len(free))
