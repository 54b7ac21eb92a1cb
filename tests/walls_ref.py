"""Interior walls (include/rcw.h, rcw_set_walls) restated on the CPU — test infrastructure, not a test.

Two pieces, both independent of the engine's code:

  the generator   csrc/rcw_rng.h in Python integers (mix64, episode_key, draw, below) and `reset_draws`, reset!(world) SR:110-137 with the
                  one change of rule interior walls bring: the goal pair (SR:120) is drawn AGAIN while its tile's WALL bit is set, at most
                  1024 H W times; then the player's tile by rejection on any bit (UT:23-37) and the heading (SR:128).  The key is
                  (seed, global agent id, episode counter BEFORE the increment).
  WallsRef        B `oracle.pyref.World`s — the second, line-by-line restatement of the reference, which takes whatever its tile map holds —
                  with their layouts written into tile_map[WALL], composed the way the engine composes a step under cfg.auto_reset: an agent
                  that is done is re-sampled by the next step, its action ignored, reward 0, done false.  `events` counts what a rollout
                  exercised, so that a test can insist from the reference's own counts that its scenario reached what it claims:
                    interior_wall_ray_hits          rays of rendered frames that stopped on a wall tile inside the ring
                    blocked_next_to_interior_wall   moves the reference refused because the player would touch a wall tile inside the ring
                    goal_redraws                    goal pairs drawn again because the pair before fell on a wall
                    restarts_after_done             agents re-sampled by a step because they were done
                  step_lenient and clear_status are the two further calls tests/time_limit_ref.py makes of an oracle:
                  TimeLimitRef(WallsRef(...), L, seed, True) is the time limit on a walled map, without a second reference.
"""
import numpy as np

from oracle import pyref

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
RCW_WARN_SAMPLER_GAVE_UP = 1
RCW_ERR_INVALID_ACTION = -2


# ---- csrc/rcw_rng.h ------------------------------------------------------------------------------------------------------------
def mix64(z):
    z &= M64
    z ^= z >> 30; z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27; z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def episode_key(seed, global_agent, episode):
    k = mix64(seed + GOLDEN * (global_agent + 1))
    return mix64(k ^ ((episode * 0xD1B54A32D192ED03) & M64))


def draw(key, n):
    return mix64(key + GOLDEN * (n + 1))


def below(u, rng):
    return (u * rng) >> 64


def _draws_below(key, n0, count, rng):
    """below(draw(key, n), rng) for n = n0 .. n0 + count - 1 in numpy uint64 (the same integers; rng < 2^32): the rejection loop of a map
    without a free tile makes 1024 H W draws, which Python integers take a second an agent for."""
    with np.errstate(over="ignore"):
        z = np.uint64(key) + np.uint64(GOLDEN) * (np.arange(n0, n0 + count, dtype=np.uint64) + np.uint64(1))
        z ^= z >> np.uint64(30); z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27); z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
        hi, lo, r = z >> np.uint64(32), z & np.uint64(0xFFFFFFFF), np.uint64(rng)
        return ((hi * r + ((lo * r) >> np.uint64(32))) >> np.uint64(32)).astype(np.int64)


def reset_draws(seed, global_agent, episode, H, W, nd, walls, counts=None):
    """The draws of one reset!(world) of `global_agent` in episode `episode` (the counter before the increment) on a map whose WALL layer
    is `walls` (bool (H, W), walls[i-1, j-1]; the ring included).  Returns (goal_i, goal_j, tile_i, tile_j, heading, gave_up), 1-based.
    counts (a dict): "goal_redraws" is advanced by the pairs drawn again."""
    walls = np.asarray(walls) != 0
    assert walls.shape == (H, W)
    key, n, HW = episode_key(seed, global_agent, episode), 0, H * W
    cap = 1024 * HW
    gi = 2 + below(draw(key, n), H - 2); n += 1                                 # SR:120
    gj = 2 + below(draw(key, n), W - 2); n += 1
    gave_up, redraws = False, 0
    while walls[gi - 1, gj - 1]:
        if redraws == cap:
            gave_up = True
            break
        gi = 2 + below(draw(key, n), H - 2); n += 1
        gj = 2 + below(draw(key, n), W - 2); n += 1
        redraws += 1
    if counts is not None:
        counts["goal_redraws"] = counts.get("goal_redraws", 0) + redraws
    occupied = walls.T.reshape(-1).copy()                                       # tile (i, j) at lin = (i - 1) + H (j - 1)
    occupied[(gi - 1) + H * (gj - 1)] = True
    lin = below(draw(key, n), HW); n += 1                                       # UT:24
    tries, placed = 0, False
    while tries < cap:                                                          # UT:26: at most `cap` tiles are looked at
        if not occupied[lin]:
            placed = True
            break
        block = min(cap - tries, 4096)
        lins = _draws_below(key, n, block, HW)                                  # the next `block` redraws (UT:28), should all be needed
        free = np.flatnonzero(~occupied[lins[:-1]]) if block > 1 else np.array([], np.int64)
        if free.size:                                                           # redraw number free[0] + 1 lands on a free tile
            lin, n, tries, placed = int(lins[free[0]]), n + int(free[0]) + 1, tries + int(free[0]) + 1, True
            break
        lin, n, tries = int(lins[-1]), n + block, tries + block
    gave_up = gave_up or not placed
    d = below(draw(key, n), nd)                                                 # SR:128
    return gi, gj, lin % H + 1, lin // H + 1, d, gave_up


def reset_draws_scalar(seed, global_agent, episode, H, W, nd, walls):
    """reset_draws in Python integers alone, as csrc/rcw_device.h's reset_agent reads: what the numpy blocks above must equal."""
    walls = np.asarray(walls) != 0
    key, n, HW = episode_key(seed, global_agent, episode), 0, H * W
    cap = 1024 * HW
    gi = 2 + below(draw(key, n), H - 2); n += 1
    gj = 2 + below(draw(key, n), W - 2); n += 1
    gave_up, t = False, 0
    while walls[gi - 1, gj - 1]:
        if t == cap:
            gave_up = True
            break
        gi = 2 + below(draw(key, n), H - 2); n += 1
        gj = 2 + below(draw(key, n), W - 2); n += 1
        t += 1
    lin = below(draw(key, n), HW); n += 1
    placed = False
    for _ in range(cap):
        i, j = lin % H + 1, lin // H + 1
        if walls[i - 1, j - 1] or (i, j) == (gi, gj):
            lin = below(draw(key, n), HW); n += 1
        else:
            placed = True
            break
    d = below(draw(key, n), nd)
    return gi, gj, lin % H + 1, lin // H + 1, d, gave_up or not placed


def draw_actions(rng, batch):
    """forward-heavy actions from a seeded generator (tests/time_limit_ref.py's mix)"""
    return rng.choice(np.array([1, 1, 1, 2, 3, 4], np.uint8), batch)


def pack_tile_map(wall, goal):
    """BitArray{3}(2, H, W).chunks of one agent from its two layers (bool (H, W)): bit (o-1) + 2(i-1) + 2H(j-1), LSB first."""
    H, W = wall.shape
    bits = np.zeros((W, H, 2), np.uint8)
    bits[:, :, 0] = wall.T
    bits[:, :, 1] = goal.T
    nchunks = (2 * H * W + 63) // 64
    flat = np.zeros(nchunks * 64, np.uint8)
    flat[:2 * H * W] = bits.reshape(-1)
    return np.packbits(flat, bitorder="little").view(np.uint64)


class _BlindWorld(pyref.World):
    """the dynamics alone (a rehearsal looking for seeds and step counts does not need the frames)"""

    def cast_rays(self):
        self.ray_dirs, self.ray_hits = [], []

    def update_camera_view(self):
        self.col_height, self.col_colour = [0] * self.N, [0] * self.N


class WallsRef:
    def __init__(self, batch, seed, H, W, num_rays, Hc, nd=8, inc=0.25, radius=0.3, T=np.float32, auto_reset=True, agent_id_offset=0, fresh=True,
                 render=True):
        self.B, self.seed, self.H, self.W, self.N, self.Hc, self.nd, self.T = batch, int(seed), H, W, num_rays, Hc, nd, T
        self.auto_reset, self.offset = bool(auto_reset), int(agent_id_offset)
        world = pyref.World if render else _BlindWorld
        self.worlds = [world(H=H, W=W, nd=nd, radius=radius, inc=inc, num_rays=num_rays, Hc=Hc, T=T) for _ in range(batch)]
        self.episode = np.zeros(batch, np.uint32)
        self.status = np.zeros(batch, np.int32)
        self.events = dict(interior_wall_ray_hits=0, blocked_next_to_interior_wall=0, goal_redraws=0, restarts_after_done=0)
        if fresh:
            self.reset()                                                        # rcw_create: the initial state is rcw_reset(h, NULL, seed)

    # ---- the layers ------------------------------------------------------------------------------------------------------------
    def walls_of(self, b):
        tm = self.worlds[b].tile_map[pyref.WALL]
        return np.array([[tm[i][j] for j in range(1, self.W + 1)] for i in range(1, self.H + 1)], bool)

    def goals_of(self, b):
        tm = self.worlds[b].tile_map[pyref.GOAL]
        return np.array([[tm[i][j] for j in range(1, self.W + 1)] for i in range(1, self.H + 1)], bool)

    def _who(self, mask):
        return range(self.B) if mask is None else [b for b in range(self.B) if np.asarray(mask).reshape(self.B)[b]]

    def _account_rays(self, b):
        w = self.worlds[b]
        wall = w.tile_map[pyref.WALL]
        self.events["interior_wall_ray_hits"] += sum(1 for (i, j, _, _) in w.ray_hits if 1 < i < self.H and 1 < j < self.W and wall[i][j])

    def _reset_agent(self, b):
        w = self.worlds[b]
        gi, gj, ti, tj, d, gave_up = reset_draws(self.seed, self.offset + b, int(self.episode[b]), self.H, self.W, self.nd, self.walls_of(b), self.events)
        w.set_state((gi, gj), (self.T(ti - 0.5), self.T(tj - 0.5)), d)           # SR:118-134 (pose: convert(T, tile - 0.5) SR:125)
        self.episode[b] += 1
        if gave_up and self.status[b] == 0:
            self.status[b] = RCW_WARN_SAMPLER_GAVE_UP
        self._account_rays(b)

    # ---- the calls -------------------------------------------------------------------------------------------------------------
    def reset(self, mask=None, seed=None):
        if seed is not None:
            self.seed = int(seed)
        for b in self._who(mask):
            self._reset_agent(b)

    def set_walls(self, walls, index=None, mask=None):
        walls = np.asarray(walls) != 0
        walls = walls[None] if walls.ndim == 2 else walls
        assert walls.shape[1:] == (self.H, self.W) and (index is not None or len(walls) in (1, self.B))
        for b in self._who(mask):
            m = int(index[b]) if index is not None else (0 if len(walls) == 1 else b)
            tm = self.worlds[b].tile_map
            for i in range(1, self.H + 1):
                for j in range(1, self.W + 1):
                    tm[pyref.WALL][i][j] = bool(walls[m, i - 1, j - 1])
                    tm[pyref.GOAL][i][j] = False
            self._reset_agent(b)

    def set_state(self, goal, pos, heading, mask=None):
        for b in self._who(mask):
            self.worlds[b].set_state(goal[b], pos[b], heading[b])
            self._account_rays(b)

    def _step_agent(self, b, act):
        w = self.worlds[b]
        if self.auto_reset and w.done:
            self.events["restarts_after_done"] += 1
            self._reset_agent(b)
            return
        if act in (1, 2):                                                       # the move act! is about to test (UT:16-17), against the interior walls alone
            d = w.directions[w.dir]
            s = 1 if act == 1 else -1
            new = (w.pos[0] + w.inc * d[0], w.pos[1] + w.inc * d[1]) if s == 1 else (w.pos[0] - w.inc * d[0], w.pos[1] - w.inc * d[1])
            inner = [[1 < i < self.H and 1 < j < self.W and bool(w.tile_map[pyref.WALL][i][j]) for j in range(self.W + 1)] for i in range(self.H + 1)]
            if not pyref.is_player_colliding(w.tile_map[pyref.GOAL], new, w.radius, self.T) and pyref.is_player_colliding(inner, new, w.radius, self.T):
                self.events["blocked_next_to_interior_wall"] += 1
        w.step(act)
        self._account_rays(b)

    def step(self, actions):
        a = np.asarray(actions).reshape(self.B)
        for b in range(self.B):
            self._step_agent(b, int(a[b]))

    def step_lenient(self, actions):
        """rcw_step_device's rule, as the oracle's step_lenient has it: an agent whose action is outside 1..4 is not stepped — not restarted
        either — and its status word says so; every other agent steps as in `step`."""
        a = np.asarray(actions).reshape(self.B)
        for b in range(self.B):
            if 1 <= int(a[b]) <= 4:
                self._step_agent(b, int(a[b]))
            else:
                self.status[b] = RCW_ERR_INVALID_ACTION

    def clear_status(self):
        self.status[...] = 0

    # ---- the batched arrays, in the engine's shapes and types ---------------------------------------------------------------------
    @property
    def camera_view(self):
        return np.stack([w.camera_view for w in self.worlds])

    @property
    def reward(self):
        return np.array([w.reward for w in self.worlds], np.float32)

    @property
    def done(self):
        return np.array([w.done for w in self.worlds], np.uint8)

    @property
    def goal(self):
        return np.array([w.goal for w in self.worlds], np.int32)

    @property
    def position(self):
        return np.array([w.pos for w in self.worlds], self.T)

    @property
    def direction(self):
        return np.array([w.dir for w in self.worlds], np.int32)

    @property
    def col_height(self):
        return np.array([w.col_height for w in self.worlds], np.int64).clip(-2 ** 31, 2 ** 31 - 1).astype(np.int32)

    @property
    def col_colour(self):
        return np.array([w.col_colour for w in self.worlds], np.uint8)

    @property
    def tile_map_chunks(self):
        return np.stack([pack_tile_map(self.walls_of(b), self.goals_of(b)) for b in range(self.B)])

    def top_view(self, pu):
        out = []
        for w in self.worlds:
            w.update_top_view(pu)
            out.append(w.top_view)
        return np.stack(out)

    def snapshot(self):
        """every compared array, copied: a rollout computed once and replayed against several forms of the engine"""
        return dict(camera_view=self.camera_view, reward=self.reward, done=self.done, goal=self.goal, position=self.position, direction=self.direction,
                    episode=self.episode.copy(), col_height=self.col_height, col_colour=self.col_colour, tile_map_chunks=self.tile_map_chunks,
                    status=self.status.copy())


def assert_equal(env, ref, where=""):
    """the engine against a WallsRef (or one of its snapshots), byte for byte"""
    r = ref if isinstance(ref, dict) else ref.snapshot()
    w = env.world
    pos = w.player_position_wu
    assert pos.dtype == r["position"].dtype
    bits = np.uint64 if pos.dtype == np.float64 else np.uint32
    np.testing.assert_array_equal(w.status, r["status"], err_msg=f"status {where}")
    np.testing.assert_array_equal(w.episode, r["episode"], err_msg=f"episode {where}")
    np.testing.assert_array_equal(w.goal_position, r["goal"], err_msg=f"goal {where}")
    np.testing.assert_array_equal(pos.view(bits), r["position"].view(bits), err_msg=f"position {where}")
    np.testing.assert_array_equal(w.player_direction_au, r["direction"], err_msg=f"heading {where}")
    np.testing.assert_array_equal(w.reward, r["reward"], err_msg=f"reward {where}")
    np.testing.assert_array_equal(w.done.astype(np.uint8), r["done"], err_msg=f"done {where}")
    np.testing.assert_array_equal(w.tile_map_chunks, r["tile_map_chunks"], err_msg=f"tile map {where}")
    h, c = env.columns()
    np.testing.assert_array_equal(h, r["col_height"], err_msg=f"height_line_pu {where}")
    np.testing.assert_array_equal(c, r["col_colour"], err_msg=f"colour id {where}")
    np.testing.assert_array_equal(env.camera_view_host(), r["camera_view"], err_msg=f"camera view {where}")

