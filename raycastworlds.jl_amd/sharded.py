"""Multi-GPU: agents shard across ranks, one process per GPU, no data-path collective.

Agents are independent (nothing in SingleRoomWorld, SR:21-40, refers to another world), so a
global batch of B agents on G GPUs is G engines of B/G agents; rank r owns the contiguous
global ids [r*B/G, (r+1)*B/G).  `agent_id_offset` keys the reset generator by GLOBAL id, so
the states do not depend on how the batch is sharded.  Stepping needs no communication.

The only exchange is the optional observation gather BASELINE.json's north_star names.
Over xGMI a full-frame gather costs ~50x what producing the frames costs, so
the default gathers the compact per-column descriptors (5 bytes per column instead of
4*H_cam) with RCCL and expands them to pixels on the receiving GPU (rcw_expand_columns);
`mode="frames"` gathers the pixels themselves for API fidelity.

Two transports, same result:
  * `gather_*`      torch.distributed (backend "nccl" = RCCL on ROCm, "gloo" in the CPU tests); the
                    collective is issued from the engine's stream, so it is ordered behind the step
                    that produced the frames without any host synchronisation;
  * `gather_*_abi`  the library's own entry points (rcw_comm_init / rcw_gather_*), which call RCCL
                    directly on the engine's stream — what a host without torch (the Julia binding)
                    uses; here torch.distributed only carries the 128-byte ncclUniqueId to the ranks.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Callable, Optional, Tuple

import numpy as np


def shard_range(global_batch: int, world: int, rank: int) -> Tuple[int, int]:
    """(first global agent id, count) of `rank`'s contiguous shard; shards must be equal so
    that all_gather needs no padding."""
    if world < 1 or not (0 <= rank < world):
        raise ValueError(f"bad rank {rank} / world {world}")
    if global_batch % world != 0:
        raise ValueError(f"global batch {global_batch} is not divisible by {world} ranks")
    per = global_batch // world
    return rank * per, per


def default_device() -> int:
    """The HIP device of this process: LOCAL_RANK under torch.distributed.run (the global rank is
    not a device index on a multi-node job), else torch's current device."""
    if "LOCAL_RANK" in os.environ:
        return int(os.environ["LOCAL_RANK"])
    try:
        import torch

        if torch.cuda.is_available():
            return int(torch.cuda.current_device())
    except ImportError:
        pass
    return 0


def make_unique_id(library: Optional[str] = None) -> bytes:
    """rcw_comm_unique_id: the 128 bytes ONE rank makes and every rank of the gather group hands to
    `ShardedSingleRoom.comm_init_abi(unique_id=...)` / rcw_comm_init."""
    from . import _capi

    _capi.preload_rccl()
    lib = _capi.load(library)
    uid = (C.c_uint8 * _capi.RCW_UNIQUE_ID_BYTES)()
    _capi.check(lib.rcw_comm_unique_id(uid), lib)
    return bytes(uid)


class ShardedSingleRoom:
    """B agents over `world` ranks.  `env_factory(batch=, agent_id_offset=, device=, **kw)` builds
    the local engine: SingleRoomModule.SingleRoom (HIP) unless a test injects another.

    `collective="auto"` skips the all-gather on a world of one rank (there is nothing to exchange);
    `"always"` issues it regardless — how the RCCL path is exercised on a one-GPU box."""

    def __init__(self, global_batch: int, *, rank: Optional[int] = None, world: Optional[int] = None,
                 group=None, device: Optional[int] = None, env_factory: Optional[Callable] = None,
                 collective: str = "auto", **kwargs):
        if collective not in ("auto", "always"):
            raise ValueError(f"collective must be 'auto' or 'always', not {collective!r}")
        self.group = group
        self.collective = collective
        # torch.distributed is asked only for what the caller did not say: with `rank` and `world` given (and the library
        # transport's unique id brought by the caller, comm_init_abi) a host without torch shards and gathers all the same
        if world is None or rank is None:
            dist = self._dist
            if world is None:
                world = dist.get_world_size(group) if dist.is_initialized() else 1
            if rank is None:
                rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.world, self.rank = int(world), int(rank)
        self.global_batch = int(global_batch)
        self.first, self.count = shard_range(self.global_batch, self.world, self.rank)
        if env_factory is None:
            from .single_room import SingleRoom as env_factory
        # the reference's `rng` keyword (SR:49,265) for a sharded batch: generators are GLOBAL — one per global agent, or one
        # for all, which every rank advances through all global agents' draws (in the same initial state on every rank) —
        # so that the states do not depend on the sharding, as with the device generator (agent_id_offset)
        self.rng = kwargs.pop("rng", None)
        for source in ("wall_bank", "wall_generator", "wall_caves", "wall_rooms"):
            self._refuse_rng(source.replace("_", " "), kwargs.get(source))
        self._refuse_rng("start rule", kwargs.get("start_distance") or None)
        self.env = env_factory(batch=self.count, agent_id_offset=self.first,
                               device=default_device() if device is None else device, **kwargs)
        self._abi_comm = False
        if self.rng is not None:
            from .single_room import _reset_from_rng

            _reset_from_rng(self.env, self.rng, None, construction=True, first=self.first, global_batch=self.global_batch)

    def _refuse_rng(self, what: str, asked) -> None:
        """(a layout source drawn on the device, asked of a batch whose resets are drawn on the host; asked = None switches one off)"""
        if self.rng is not None and asked is not None:
            raise ValueError(f"a batch built with rng draws its resets on the host: it takes no {what}")

    @property
    def _dist(self):
        import torch.distributed as dist                  # (on first use: the torch transport, or a rank / world left to it)

        return dist

    # ---- stepping: purely local ------------------------------------------------------
    def local_slice(self, global_array):
        """This rank's rows of an array indexed by global agent id."""
        return global_array[self.first:self.first + self.count]

    def act_(self, local_actions) -> None:
        from .single_room import act_

        act_(self.env, local_actions)

    def reset_(self, local_mask=None, seed: Optional[int] = None, rng=None, global_mask=None) -> None:
        """`RCW.reset!` of this rank's agents: on the device (`local_mask`, `seed`), or — `rng`, or a batch constructed with
        one — from the caller's GLOBAL generator(s), with the GLOBAL mask (`global_mask`: a single generator's draws for the
        other ranks' unmasked agents have to be made too)."""
        from .single_room import _reset_from_rng, reset_

        if rng is None and seed is None:
            rng = self.rng
        if rng is not None:
            if local_mask is not None and global_mask is None:
                if hasattr(rng, "integers") and self.world > 1:
                    raise ValueError("a masked reset from ONE generator needs the GLOBAL mask (global_mask=...): the other ranks' draws are made too")
                global_mask = np.ones(self.global_batch, dtype=np.uint8)
                global_mask[self.first:self.first + self.count] = np.asarray(local_mask, dtype=np.uint8).reshape(self.count)
            _reset_from_rng(self.env, rng, global_mask, first=self.first, global_batch=self.global_batch)
            return
        reset_(self.env, local_mask, seed)

    def set_walls(self, walls, index=None, mask=None) -> None:
        """`SingleRoom.set_walls` for the sharded batch: `index` and `mask` are GLOBAL (one entry per global agent) and every
        rank passes the same arguments; each rank hands its engine its slice.  `walls` (H, W) or (M, H, W) is replicated —
        or, with M == the global batch and no index (agent a takes layout a), sliced.  A batch built with `rng` resets the
        touched agents from the global generator(s), as `reset_(global_mask=...)` does."""
        G, lo, hi = self.global_batch, self.first, self.first + self.count
        w = np.asarray(walls) != 0
        if w.ndim == 2:
            w = w[None]
        if w.ndim != 3:
            raise ValueError(f"walls must be (H, W) or (M, H, W), got {w.shape}")
        M = w.shape[0]
        if index is None and M not in (1, G):
            raise ValueError(f"without an index, walls holds 1 layout or one per global agent ({G}); got {M}")
        gi = None if index is None else np.ascontiguousarray(index, dtype=np.int32).reshape(G)
        gm = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8).reshape(G)
        if gi is None and M == G and M != 1:
            local_walls, local_index = w[lo:hi], None                 # agent a takes layout a: this shard's rows
        else:
            local_walls, local_index = w, (None if gi is None else gi[lo:hi])
        if gi is not None and ((gi < 0) | (gi >= M))[np.ones(G, bool) if gm is None else gm != 0].any():
            raise ValueError(f"layout index not in 0..{M - 1}")     # (also another rank's: every rank refuses alike)
        self.env.set_walls(local_walls, local_index, None if gm is None else gm[lo:hi])
        if self.rng is not None:
            from .single_room import _reset_from_rng

            took = gi if gi is not None else (np.zeros(G, dtype=np.int32) if M == 1 else np.arange(G, dtype=np.int32))
            if getattr(self.env, "_rng_walls_global", None) is None:
                ring = np.zeros((G,) + w.shape[1:], dtype=bool)
                ring[:, [0, -1], :] = True
                ring[:, :, [0, -1]] = True
                self.env._rng_walls_global = ring
            touched = np.ones(G, dtype=bool) if gm is None else gm != 0
            self.env._rng_walls_global[touched] = w[took[touched]]
            _reset_from_rng(self.env, self.rng, gm, first=self.first, global_batch=self.global_batch)

    def set_wall_bank(self, walls, weights=None) -> None:
        """`SingleRoom.set_wall_bank` for the sharded batch: the bank and its weights are REPLICATED — every rank passes the same
        arguments — and nothing else is needed: the layout an agent draws is keyed by its global id (`agent_id_offset`), so a shard
        equals its slice of the whole batch."""
        self._refuse_rng("wall bank", walls)
        self.env.set_wall_bank(walls, weights)

    def set_wall_generator(self, loops=0.0, levels: int = 0, first_level: int = 0, level_seed: int = 0) -> None:
        """`SingleRoom.set_wall_generator` for the sharded batch: the parameters are REPLICATED — every rank passes the same — and
        nothing else is needed: the maze an agent's episode gets is keyed by its global id (`agent_id_offset`)."""
        self._forward_family("wall generator", self.env.set_wall_generator, loops, levels, first_level, level_seed)

    def set_wall_caves(self, fill=0.40, smooth: int = 2, levels: int = 0, first_level: int = 0, level_seed: int = 0) -> None:
        """`SingleRoom.set_wall_caves` for the sharded batch: the parameters are REPLICATED — every rank passes the same — and
        nothing else is needed: the cave an agent's episode gets is keyed by its global id (`agent_id_offset`)."""
        self._forward_family("wall caves", self.env.set_wall_caves, fill, smooth, levels, first_level, level_seed)

    def set_wall_rooms(self, room=2, stop=0.25, doors=0.25, levels: int = 0, first_level: int = 0, level_seed: int = 0) -> None:
        """`SingleRoom.set_wall_rooms` for the sharded batch: the parameters are REPLICATED — every rank passes the same — and
        nothing else is needed: the rooms an agent's episode gets are keyed by its global id (`agent_id_offset`)."""
        self._forward_family("wall rooms", self.env.set_wall_rooms, room, stop, doors, levels, first_level, level_seed)

    def _forward_family(self, what: str, setter, *args) -> None:
        """a family's replicated parameters on to the shard's environment; the first one None switches the family off"""
        self._refuse_rng(what, args[0])
        setter(*args)

    def set_wall_bank_weights(self, weights) -> None:
        """`SingleRoom.set_wall_bank_weights`, the same weights on every rank."""
        self.env.set_wall_bank_weights(weights)

    # ---- the guide: a function of each agent's own state, so a shard's words are its slice of the batch's ----
    def set_guide(self, on: bool = True) -> None:
        """`SingleRoom.set_guide` of this rank's engine (also the `guide=True` keyword); `guide_action` / `guide_heading` are LOCAL."""
        self.env.set_guide(on)

    # ---- the frontier: a function of each agent's own seen map and pose, so a shard's words are its slice of the batch's ----
    def set_frontier(self, on: bool = True) -> None:
        """`SingleRoom.set_frontier` of this rank's engine (also the `frontier=True` keyword); the arrays below are LOCAL."""
        self.env.set_frontier(on)

    # ---- the start rule: a function of (seed, GLOBAL agent id, episode, walls, goal, band), so a shard's starts are its slice of the batch's ----
    def set_start_distance(self, lo=1, hi=None) -> None:
        """`SingleRoom.set_start_distance` of this rank's engine (also the `start_distance=` keyword); `start_placed` is LOCAL.  Every
        rank sets the same band."""
        self._refuse_rng("start rule", None if lo is None or lo is False else lo)
        self.env.set_start_distance(lo, hi)

    @property
    def start_distance_info(self) -> dict:
        return self.env.start_distance_info

    # ---- the visit map: a count of each agent's own poses, so a shard's map and words are its slice of the batch's ----
    def set_visit_map(self, sectors=1, table: bool = False) -> None:
        """`SingleRoom.set_visit_map` of this rank's engine (also the `visit_map=` keyword).  The map and `visits_here` /
        `visited_cells` / `visit_first` of a shard are its slice of the batch's.  The table is per handle: a shard's table holds its own
        agents' counts, the shards' tables sum to the batch's (nothing here all-reduces them), and `level_visits_here` is taken from
        the shard's OWN table — it is not a slice of the batch's."""
        self.env.set_visit_map(sectors, table)

    def visit_table(self, device: bool = False):
        """`SingleRoom.visit_table` of this rank's engine: this SHARD's counts."""
        return self.env.visit_table(device)

    def visit_table_clear(self) -> None:
        self.env.visit_table_clear()

    # ---- the state archive: every shard has its own, rows are LOCAL ---------------------------
    def set_snapshots(self, rows: int) -> None:
        """`SingleRoom.set_snapshots` of this rank's engine: `rows` records a SHARD.  Rows do not cross shards."""
        self.env.set_snapshots(rows)

    def snapshot_save(self, rows=None, mask=None) -> None:
        """`SingleRoom.snapshot_save` with this rank's LOCAL arrays (one entry per local agent, local row indices)."""
        self.env.snapshot_save(rows, mask)

    def snapshot_restore(self, rows=None, mask=None) -> None:
        """`SingleRoom.snapshot_restore` with this rank's LOCAL arrays."""
        self.env.snapshot_restore(rows, mask)

    # ---- the observation gather over torch.distributed -------------------------------------
    def _as_tensor(self, x):
        import torch

        if hasattr(x, "__cuda_array_interface__"):
            return x.torch(sync=False)   # ordered on the engine's stream below, not by a host sync
        return torch.as_tensor(x)

    def _skip(self) -> bool:
        return self.world == 1 and self.collective == "auto"

    def _engine_stream(self, tensor):
        """Context that makes the engine's stream torch's current stream (device tensors), so the
        collective is enqueued behind the step and its result is ordered on that same stream."""
        import contextlib

        import torch

        if getattr(tensor, "is_cuda", False) and hasattr(self.env, "torch_stream"):
            return torch.cuda.stream(self.env.torch_stream())
        return contextlib.nullcontext()

    def _all_gather(self, local, out):
        """all_gather_into_tensor of `local` (this rank's rows) into `out` (global rows).  uint32 frames go
        through the process group as int32 (same bytes) so nothing depends on unsigned support in the backend."""
        import torch

        a, b = local.contiguous(), out
        if a.dtype == torch.uint32:
            a, b = a.view(torch.int32), b.view(torch.int32)
        self._dist.all_gather_into_tensor(b, a, group=self.group)
        return out

    def gather_columns(self):
        """all_gather of the compact descriptors: (height_line_pu int32 (B, N), colour id uint8 (B, N))
        for the GLOBAL batch, on every rank (device tensors on GPU), ordered on the engine's stream."""
        import torch

        h, c = self.env.columns_device()
        h, c = self._as_tensor(h), self._as_tensor(c)
        if self._skip():
            return h, c
        with self._engine_stream(h):
            gh = torch.empty((self.global_batch,) + tuple(h.shape[1:]), dtype=h.dtype, device=h.device)
            gc = torch.empty((self.global_batch,) + tuple(c.shape[1:]), dtype=c.dtype, device=c.device)
            self._all_gather(h, gh)
            self._all_gather(c, gc)
        return gh, gc

    def gather_observations(self, mode: str = "columns"):
        """The GLOBAL observation batch (B, N, H_cam) on every rank, ordered on the engine's stream
        (a consumer on another stream waits for `env.torch_stream()`; `env.sync()` waits on the host).

        mode="columns": gather descriptors (5 B/column), expand to pixels locally;
        mode="frames":  gather the pixels (4*H_cam B/column) — ~50x the bytes over xGMI."""
        import torch

        if mode == "frames":
            local = self._as_tensor(self.env.camera_view)
            if self._skip():
                return local
            with self._engine_stream(local):
                out = torch.empty((self.global_batch,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
                self._all_gather(local, out)
            return out
        if mode != "columns":
            raise ValueError(f"unknown gather mode {mode!r}")
        gh, gc = self.gather_columns()
        with self._engine_stream(gh):
            return self.env.expand_columns(gh, gc)

    # ---- the same gather through the C ABI (RCCL called by the library) -----------------------
    def comm_init_abi(self, unique_id: Optional[bytes] = None) -> None:
        """rcw_comm_init on this rank's engine.  Rank 0 makes the ncclUniqueId (rcw_comm_unique_id) and
        torch.distributed carries its 128 bytes to the other ranks; a world of one needs no transport.

        `unique_id`: the 128 bytes of `make_unique_id()` brought here by the CALLER's own transport (MPI, a file, a socket:
        what a host without torch.distributed does — and how several ranks can live in one process, one engine each,
        where torch.distributed's ranks are processes).  That path imports no torch."""
        from . import _capi

        if self._abi_comm:
            return
        _capi.preload_rccl()
        lib = self.env._lib
        if unique_id is not None:
            if len(unique_id) != _capi.RCW_UNIQUE_ID_BYTES:
                raise ValueError(f"a unique id is {_capi.RCW_UNIQUE_ID_BYTES} bytes, got {len(unique_id)}")
            uid = (C.c_uint8 * _capi.RCW_UNIQUE_ID_BYTES)(*bytes(unique_id))
            self.env._check(lib.rcw_comm_init(self.env._h, uid, self.rank, self.world))
            self._abi_comm = True
            return
        uid = (C.c_uint8 * _capi.RCW_UNIQUE_ID_BYTES)()
        if self.rank == 0:
            self.env._check(lib.rcw_comm_unique_id(uid))
        if self.world > 1:
            import torch                                  # (only the torch.distributed hand-over needs it)

            t = torch.tensor(list(uid), dtype=torch.uint8)
            backend = self._dist.get_backend(self.group)
            if backend == "nccl":
                t = t.cuda(self.env.device)
            self._dist.broadcast(t, src=0, group=self.group)
            uid = (C.c_uint8 * _capi.RCW_UNIQUE_ID_BYTES)(*t.cpu().tolist())
        self.env._check(lib.rcw_comm_init(self.env._h, uid, self.rank, self.world))
        self._abi_comm = True

    def gather_columns_abi(self):
        """rcw_gather_columns: (height_line_pu int32 (B, N), colour id uint8 (B, N)) of the global batch as
        torch tensors filled on the engine's stream."""
        import torch

        self.comm_init_abi()
        env = self.env
        dev = f"cuda:{env.device}"
        gh = torch.empty((self.global_batch, env.cfg.num_rays), dtype=torch.int32, device=dev)
        gc = torch.empty((self.global_batch, env.cfg.num_rays), dtype=torch.uint8, device=dev)
        cross = env._order_behind_torch()
        from . import _capi

        env._check(env._lib.rcw_gather_columns(env._h, C.c_void_p(gh.data_ptr()), C.c_void_p(gc.data_ptr())))
        if cross:
            env._release_after_use(gh, gc)
        return gh, gc

    def gather_observations_abi(self, mode: str = "columns", out=None):
        """rcw_gather_observations: the global observation batch (B, N, H_cam) uint32, filled on the
        engine's stream by the library (RCCL all-gather + on-device expansion)."""
        import torch

        from . import _capi

        modes = {"columns": _capi.RCW_GATHER_COLUMNS, "frames": _capi.RCW_GATHER_FRAMES}
        if mode not in modes:
            raise ValueError(f"unknown gather mode {mode!r}")
        self.comm_init_abi()
        env = self.env
        if out is None:
            out = torch.empty((self.global_batch, env.cfg.num_rays, env.cfg.height_camera_view_pu), dtype=torch.uint32,
                              device=f"cuda:{env.device}")
        cross = env._order_behind_torch()
        env._check(env._lib.rcw_gather_observations(env._h, modes[mode], C.c_void_p(out.data_ptr())))
        if cross:
            env._release_after_use(out)
        return out

    def close(self):
        if self._abi_comm:
            self.env._lib.rcw_comm_destroy(self.env._h)
            self._abi_comm = False
        self.env.close()


# The per-agent arrays a shard hands out as its engine's, by `SingleRoom`'s names: functions of each agent's own state, so a shard's
# are its slice of the batch's (but `level_visits_here`: `set_visit_map`).  They are LOCAL: one entry per agent of this rank.
_FORWARDED = ("guide_action", "guide_heading",
              "frontier_distance", "frontier_tiles", "explore_action", "explore_heading", "frontier_field",
              "visit_map", "visits_here", "visited_cells", "visit_first", "level_visits_here", "start_placed")
for _name in _FORWARDED:
    setattr(ShardedSingleRoom, _name, property(lambda self, _name=_name: getattr(self.env, _name)))
del _name
