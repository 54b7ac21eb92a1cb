"""Host-side mirror of RayCastWorlds.jl's SingleRoomModule for a BATCH of agents.

The reference is Julia (src/single_room.jl, "SR" below); no Julia toolchain exists in this
pipeline, so this Python layer plays the role of the Julia host code above the C ABI
(include/rcw.h) with the reference's names and argument meanings:

    reference (Julia)                       here (Python)
    SingleRoom(; kwargs...)      SR:258     SingleRoom(batch, **same kwargs)
    RCW.reset!(env)              SR:326     reset_(env)
    RCW.act!(env, action)        SR:333     act_(env, actions)        # one action per agent
    RCW.get_action_names(env)    SR:486     get_action_names(env)
    RCW.RLBaseEnv(env)           rlbase.jl  RLBaseEnv(env)            # see rlbase.py
    env.world.reward / .done ... SR:21-40   env.world.reward / .done ...

All compute happens in librcw_hip.so on the GPU; nothing here falls back to the CPU.
Arrays come back batch-first in numpy C order, which is byte-identical to the Julia
column-major layout with a trailing batch axis: camera_view (B, N, H_cam) == Julia
UInt32 (H_cam, N, B).
"""
from __future__ import annotations

import collections
import ctypes as C
import sys
import types
from typing import Optional, Sequence

import numpy as np

from . import _capi

NUM_OBJECTS = 2   # SR:16
WALL = 1          # SR:17
GOAL = 2          # SR:18
NUM_ACTIONS = 4   # SR:19

NUM_VIEWS = 2     # SR:237
CAMERA_VIEW = 1   # SR:238
TOP_VIEW = 2      # SR:239


class _Handle:
    """Owner of the native `rcw_handle`: whoever holds one keeps the engine's device memory alive.

    It refers to nothing but the library, so it can be held from places Python's collector cannot see (the deleter of a
    torch tensor made over engine memory, `_CudaExport` below) without tying the environment into an uncollectable
    cycle: environment -> DeviceArray -> tensor -> export -> _Handle, and nothing leads back."""

    __slots__ = ("lib", "h")

    def __init__(self, lib):
        self.lib = lib
        self.h = C.c_void_p()

    def close(self):
        if self.h:
            self.lib.rcw_destroy(self.h)         # waits for the handle's stream
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:                        # noqa: BLE001 — interpreter shutdown
            pass


class _CudaExport:
    """What `DeviceArray.torch()` hands to `torch.as_tensor`: pointer, shape and type of the device memory plus the
    `_Handle` that keeps it allocated.  torch takes a reference to the exporting object inside the tensor's storage
    deleter — a reference invisible to Python's collector — so the exporter must not lead back to whoever caches the
    tensor (exporting the DeviceArray itself leaked every environment whose reward / done / state
    tensor had been made)."""

    __slots__ = ("__cuda_array_interface__", "_handle")

    def __init__(self, interface: dict, handle):
        self.__cuda_array_interface__ = interface
        self._handle = handle


class DeviceArray(np.lib.mixins.NDArrayOperatorsMixin):
    """A typed view of library-owned device memory (no copy).

    Exposes `__cuda_array_interface__` (v3), so `torch.as_tensor(x, device="cuda")` and
    friends alias it exactly as `RLBase.state(env)` aliases `camera_view` (SR:576).

    A GPU-resident consumer takes `x.torch(sync=False)` — one cached tensor over the stable device pointer, ordered on
    the engine's stream, no host synchronisation ever.  A host consumer just uses it as an array: `np.asarray(x)`,
    `x == 0`, `x.any()`, `total += x` copy the current contents to the host at that moment (one device-to-host copy
    behind the engine's stream — the explicit request; a sticky device error such as the reference's BoundsError
    surfaces there).
    """

    def __init__(self, ptr: int, shape: Sequence[int], dtype, owner, sync, host_getter=None):
        self.ptr = int(ptr)
        self.shape = tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self._owner = owner   # keeps the handle alive
        self._sync = sync
        self._host_getter = host_getter
        self._torch = None

    @property
    def nbytes(self) -> int:
        return int(np.prod(self.shape)) * self.dtype.itemsize

    @property
    def __cuda_array_interface__(self):
        # One host synchronisation when the alias is made (what a casual `torch.as_tensor(env.camera_view)`
        # needs to read valid data).  After that the alias is NOT re-synchronised: torch work on a stream other
        # than the engine's must `wait_stream(env.torch_stream())` (or share one stream via `env.set_stream`)
        # before reading frames a later step writes — INTEGRATION.md "Streams".
        self._sync()
        return self._interface()

    def _interface(self) -> dict:
        # (device memory behind a Bool view is one byte per element: exported as uint8, viewed as bool by .torch())
        return {
            "shape": self.shape,
            "typestr": "|u1" if self.dtype == np.bool_ else self.dtype.str,
            "data": (self.ptr, False),
            "version": 3,
            "strides": None,
        }

    @staticmethod
    def _tensor_over(export, device: int):
        import torch

        return torch.as_tensor(export, device=f"cuda:{device}")

    def torch(self, sync: bool = True):
        """Zero-copy torch tensor on the handle's device (made once per DeviceArray, the pointer is stable).
        `sync=False` skips the host synchronisation: for callers that order their work on the engine's stream
        themselves (a policy on the shared stream, the observation gather)."""
        if sync:
            self._sync()
        if self._torch is None:
            # exported through a proxy that holds the native handle, not this object: see _CudaExport
            t = self._tensor_over(_CudaExport(self._interface(), getattr(self._owner, "_handle", None)), self._owner.device)
            if self.dtype == np.bool_:
                import torch

                t = t.view(torch.bool)
            self._torch = t
        return self._torch

    # DLPack (the array-API exchange protocol: `jax.dlpack.from_dlpack(x)`, `cupy.from_dlpack(x)`, `torch.from_dlpack(x)`):
    # the same zero-copy alias, handed over by the cached torch tensor.  The consumer's stream is ordered behind the
    # engine's by one host synchronisation at export, as with __cuda_array_interface__.
    def __dlpack__(self, stream=None, **kwargs):
        t = self.torch(sync=True)
        return t.__dlpack__(**kwargs) if stream is None else t.__dlpack__(stream=stream, **kwargs)

    def __dlpack_device__(self):
        return self.torch(sync=False).__dlpack_device__()

    def numpy(self) -> np.ndarray:
        """Copy to host (waits for the engine's stream)."""
        if self._host_getter is not None:
            return self._host_getter()
        return self._owner._copy_device_array(self)

    # ---- host-side use as an array: every operation below starts with one device-to-host copy --------------
    def __array__(self, dtype=None, copy=None):
        a = self.numpy()
        return a if dtype is None else a.astype(dtype, copy=False)

    def __array_ufunc__(self, ufunc, method, *inputs, out=None, **kwargs):
        if out is not None:
            if any(isinstance(o, DeviceArray) for o in out):
                # `x += 1`, `np.add(a, b, out=x)`: engine memory is the engine's to write (the next step overwrites it)
                raise TypeError("a DeviceArray is read-only from the host: operate on np.asarray(x) or x.torch()")
            kwargs["out"] = out
        inputs = tuple(np.asarray(x) if isinstance(x, DeviceArray) else x for x in inputs)
        return getattr(ufunc, method)(*inputs, **kwargs)

    def __bool__(self):
        """As ndarray: the value of a one-element array, ValueError for more (`if is_terminated(env):` with a batch)."""
        return bool(self.numpy())

    def __iter__(self):
        """One device-to-host copy, then the host array's iterator (not one copy per element)."""
        return iter(self.numpy())

    def any(self, *a, **k):
        return self.numpy().any(*a, **k)

    def all(self, *a, **k):
        return self.numpy().all(*a, **k)

    def sum(self, *a, **k):
        return self.numpy().sum(*a, **k)

    def __len__(self):
        return self.shape[0]

    def __getitem__(self, idx):
        return self.numpy()[idx]

    def __repr__(self):
        return f"DeviceArray(ptr=0x{self.ptr:x}, shape={self.shape}, dtype={self.dtype})"


def _torch_owns(stream) -> bool:
    """True for a stream out of torch's own pool (`torch.cuda.Stream()`, the current / default stream): torch never
    destroys those.  `torch.cuda.ExternalStream` is a Stream subclass with the same `.cuda_stream` attribute, but wraps
    a hipStream_t its creator may destroy at any time — anything that is not provably torch's is the caller's."""
    torch = sys.modules.get("torch")
    if torch is None:
        return False
    return isinstance(stream, torch.cuda.Stream) and not isinstance(stream, torch.cuda.ExternalStream)


def _as_ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---- the per-agent words, maps and fields of the features, described ONCE (DESIGN.md "the per-agent arrays in the binding") ----------
# A group of words: the attribute that caches its `DeviceArray`s, the export that copies them to the host (a pointer a word, NULL: not
# this one), the export that hands out their device pointers, and the words in the ABI's order as (public name, dtype).  `namespace`:
# the group is handed out whole, as a SimpleNamespace of its words.
_Words = collections.namedtuple("_Words", "cache host device_ptr words namespace", defaults=(False,))
_WORDS = {
    "goal_distance": _Words("_goal_distance_dev", "rcw_goal_distance", "rcw_goal_distance_device_ptr",
                            (("goal_distance", np.int32), ("goal_start_distance", np.int32), ("goal_progress", np.int32))),
    "guide": _Words("_guide_dev", "rcw_guide", "rcw_guide_device_ptr", (("guide_action", np.uint8), ("guide_heading", np.int32))),
    "seen_map": _Words("_seen_map_dev", "rcw_seen_words", "rcw_seen_words_device_ptr",
                       (("seen_count", np.int32), ("seen_new", np.int32), ("goal_seen", np.int32))),
    "frontier": _Words("_frontier_dev", "rcw_frontier", "rcw_frontier_device_ptr",
                       (("frontier_distance", np.int32), ("frontier_tiles", np.int32), ("explore_action", np.uint8), ("explore_heading", np.int32))),
    "visit_map": _Words("_visit_map_dev", "rcw_visit_words", "rcw_visit_words_device_ptr",
                        (("visits_here", np.int32), ("visited_cells", np.int32), ("visit_first", np.int32), ("level_visits_here", np.uint32))),
    "episode_stats": _Words("_episode_stats_dev", "rcw_episode_stats", "rcw_episode_stats_device_ptr",
                            (("finished", np.uint8), ("outcome", np.uint8), ("length", np.uint32), ("moves", np.uint32), ("level", np.int32),
                             ("spl_q16", np.int32), ("episodes", np.uint32)), namespace=True),
    "wall_layout": _Words("_wall_layout_dev", "rcw_wall_layout", "rcw_wall_layout_device_ptr", (("wall_layout", np.int32),)),
    "start_distance": _Words("_start_distance_dev", "rcw_start_distance", "rcw_start_distance_device_ptr", (("start_placed", np.uint8),)),
}

# An array in the tile map's own order, (B, [sectors,] W, H) on the device: its element type, the export that copies agents
# [first, first + count) to the host, the export that hands out its device pointer, and whether it has the visit map's sector axis.
_Tiles = collections.namedtuple("_Tiles", "dtype host device_ptr sectors")
_TILES = {
    "goal_distance_field": _Tiles(np.uint16, "rcw_goal_distance_field", "rcw_goal_distance_field_device_ptr", False),
    "seen_map": _Tiles(np.uint8, "rcw_seen_map", "rcw_seen_map_device_ptr", False),
    "frontier_field": _Tiles(np.uint16, "rcw_frontier_field", "rcw_frontier_field_device_ptr", False),
    "visit_map": _Tiles(np.uint16, "rcw_visit_map", "rcw_visit_map_device_ptr", True),
}

# Every attribute of a SingleRoom that caches an alias of engine memory, by group: what `close()` drops, and a setter for its groups
# (`SingleRoom._drop`).  An alias cached under a name that is not here outlives `close()`.
_CACHES = {
    "reward": ("_reward_dev",), "done": ("_done_dev", "_done_dev_bool"), "truncated": ("_truncated_dev", "_truncated_dev_bool"),
    "episode_steps": ("_episode_steps_dev",), "local_map": ("_local_map_dev",), "state": ("_state_alias",),
    "constant_actions": ("_constant_action_buffers",), "learner_view": ("_learner_view_alias",),
    **{group: (row.cache,) for group, row in _WORDS.items()},
}


def _word(group: str, k: Optional[int], doc: str) -> property:
    """The property of SingleRoom for word `k` of `_WORDS[group]` (None: the group itself, a namespace).  The cached path is one
    dictionary hit and one index."""
    row = _WORDS[group]
    cache = row.cache

    def get(self):
        words = self.__dict__.get(cache) or self._device_words(row)
        return words if k is None else words[k]

    return property(get, doc=doc)


def _tiles(name: str, doc: str, device: bool = False) -> property:
    """The property of SingleRoom for `_TILES[name]`: the host copy, indexed like `env.world.walls`, or (`device`) the alias."""
    row = _TILES[name]
    return property((lambda self: self._tiles_device(row)) if device else (lambda self: self._tiles_host(row)), doc=doc)


class SingleRoomWorld:
    """Accessors for the batched `SingleRoomWorld` state (SR:21-40). Each property copies
    the current device state to host."""

    def __init__(self, env: "SingleRoom"):
        self._env = env

    def _get(self, fn, dtype, shape):
        out = np.empty(shape, dtype=dtype)
        self._env.host_syncs += 1                      # every host getter waits for the engine's stream
        self._env._check(fn(self._env._h, _as_ptr(out)))
        return out

    @property
    def num_directions(self) -> int:
        return self._env.cfg.num_directions

    @property
    def num_rays(self) -> int:
        return self._env.cfg.num_rays

    @property
    def player_radius_wu(self) -> float:
        return self._env.cfg.player_radius_wu

    @property
    def position_increment_wu(self) -> float:
        return self._env.cfg.position_increment_wu

    @property
    def semi_field_of_view_wu(self) -> float:
        return self._env.cfg.semi_field_of_view_wu

    @property
    def goal_reward(self):                             # SR:34-35, one(R) SR:82
        return self._env.R(1)

    @property
    def reward(self) -> np.ndarray:                    # SR:33, in R
        return self._get(self._env._lib.rcw_reward_typed, self._env.R, (self._env.batch,))

    @property
    def done(self) -> np.ndarray:                      # SR:35
        return self._get(self._env._lib.rcw_done, np.uint8, (self._env.batch,)).astype(bool)

    @property
    def player_position_wu(self) -> np.ndarray:        # SR:24, (B, 2) in T
        if self._env.T is np.float64:
            return self._get(self._env._lib.rcw_position64, np.float64, (self._env.batch, 2))
        return self._get(self._env._lib.rcw_position, np.float32, (self._env.batch, 2))

    @property
    def player_direction_au(self) -> np.ndarray:       # SR:25
        return self._get(self._env._lib.rcw_direction, np.int32, (self._env.batch,))

    @property
    def goal_position(self) -> np.ndarray:             # SR:32, (B, 2) 1-based (i, j)
        return self._get(self._env._lib.rcw_goal, np.int32, (self._env.batch, 2))

    @property
    def status(self) -> np.ndarray:
        """Per-agent sticky status: 0, -5 where the reference would have raised BoundsError, -2 for an invalid device action, or the
        warning 1 (`RCW_WARN_SAMPLER_GAVE_UP`) where `sample_empty_position` found no empty tile and gave up (utils.jl:34)."""
        return self._get(self._env._lib.rcw_status, np.int32, (self._env.batch,))

    @property
    def episode(self) -> np.ndarray:
        return self._get(self._env._lib.rcw_episode, np.uint32, (self._env.batch,))

    @property
    def episode_steps(self) -> np.ndarray:
        """Steps each agent's episode has taken since `set_time_limit` / its last reset (uint32; zero while there is no limit)."""
        return self._get(self._env._lib.rcw_episode_steps, np.uint32, (self._env.batch,))

    @property
    def truncated(self) -> np.ndarray:
        """Which agents' episodes the time limit has cut (bool; `episode_steps >= time_limit and not done`)."""
        return self._get(self._env._lib.rcw_truncated, np.uint8, (self._env.batch,)).astype(bool)

    @property
    def directions_wu(self) -> np.ndarray:             # SR:28, (nd, 2)
        out = np.empty((self.num_directions, 2), dtype=self._env.T)
        fn = self._env._lib.rcw_direction_table64 if self._env.T is np.float64 else self._env._lib.rcw_direction_table
        self._env._check(fn(self._env._h, _as_ptr(out)))
        return out

    @property
    def tile_map_chunks(self) -> np.ndarray:
        """BitArray{3}(2, H, W).chunks per agent: uint64 (B, nchunks)  SR:22."""
        n = C.c_int32()
        self._env._check(self._env._lib.rcw_tile_map_num_chunks(self._env._h, C.byref(n)))
        return self._get(self._env._lib.rcw_tile_map_chunks, np.uint64, (self._env.batch, n.value))

    @property
    def tile_map(self) -> np.ndarray:
        """bool (B, 2, H, W): tile_map[b, o-1, i-1, j-1] == Julia tile_map[o, i, j] of agent b."""
        env = self._env
        return unpack_tile_map(self.tile_map_chunks, env.cfg.height_tile_map_tu, env.cfg.width_tile_map_tu)

    @property
    def walls(self) -> np.ndarray:
        """bool (B, H, W): the WALL layer, `tile_map[:, 0]` — the ring (SR:57-60) and what `set_walls` put inside it."""
        return self.tile_map[:, WALL - 1]

    def rays(self, first: int = 0, count: Optional[int] = None):
        """(ray_stop_position_tu (n, N, 2) int64, ray_hit_dimension (n, N) int64,
        ray_distance_wu (n, N) float32, ray_directions_wu (n, N, 2) float32)  SR:29-31,39."""
        env = self._env
        n = env.batch - first if count is None else count
        N = env.cfg.num_rays
        stop = np.empty((n, N, 2), dtype=np.int64)
        dim = np.empty((n, N), dtype=np.int64)
        dist = np.empty((n, N), dtype=env.T)
        dirs = np.empty((n, N, 2), dtype=env.T)
        fn = env._lib.rcw_rays64 if env.T is np.float64 else env._lib.rcw_rays
        env._check(fn(env._h, first, n, _as_ptr(stop), _as_ptr(dim), _as_ptr(dist), _as_ptr(dirs)))
        return stop, dim, dist, dirs


class SingleRoom:
    """`SingleRoom(; kwargs...)` (SR:258-324) for `batch` independent agents on one MI355X.

    Keyword arguments and defaults are the reference's (SR:258-272). `T` is "Float32" (default)
    or "Float64"; `R` (the reward type, SR:266) is "Float32" (default), "Float64", "Int32" or "Int64";
    `seed` keys the device generator (the default: resets are sampled on the GPU, reproducibly, in the reference's
    distribution).  `rng` (SR:49,265) gives the reference's keyword back: a `numpy.random.Generator` — or one per agent —
    from which construction and every `reset_(env, rng=...)` draw goal, player tile and heading on the HOST in exactly
    the reference's order (`reference_reset_draws`), injected with `rcw_set_state`.  `device` is the HIP device index.
    `max_episode_steps` (this build's addition; 0 = none, the reference's behaviour) is the episode time limit of
    `set_time_limit`.  `walls` / `wall_index` (this build's addition; None = the reference's empty room) are `set_walls`'
    arguments, applied right after construction.  `goal_distance` (this build's addition) is `set_goal_distance(True)` after them,
    `guide` (this build's addition) `set_guide(True)` right behind it (it enables the goal distance where that is off),
    `seen_map` (this build's addition) `set_seen_map(True)` after that, `frontier` (this build's addition) `set_frontier(True)` right
    behind it (it enables the seen map where that is off), `local_map` (this build's addition; an int — the size — or a dict
    of `set_local_map`'s keywords) `set_local_map` after that, `episode_stats` (this build's addition) `set_episode_stats(True)` last of
    all — behind the layout sources below, whose levels count its table's rows —, `visit_map` (this build's addition; True, or a dict of
    `set_visit_map`'s keywords) `set_visit_map` right behind it, for the same reason.  `wall_bank` / `wall_bank_weights` (this build's addition) are `set_wall_bank`'s
    arguments, applied after `walls` and the time limit and before the features: a layout drawn on the device at every episode start.
    `wall_generator` (this build's addition; a dict of `set_wall_generator`'s keywords, `{}` for the defaults) is applied in the same
    place: a new maze made on the device at every episode start.  It and `wall_bank` exclude each other.  `wall_caves` (this build's
    addition; a dict of `set_wall_caves`' keywords, `{}` for the defaults) is applied right behind it: a new cave made on the device at
    every episode start.  It excludes `wall_bank` and `wall_generator`.  `wall_rooms` (this build's addition; a dict of
    `set_wall_rooms`' keywords, `{}` for the defaults) is applied behind that: new rooms and doorways made on the device at every
    episode start.  It excludes the other three.  `start_distance` (this build's addition; a pair `(lo, hi)`, or True for `(1, None)`) is
    `set_start_distance` behind every feature: no agent moves, the rule holds from the next episode start.  `snapshots` (this build's addition; a number of rows) is `set_snapshots` last of all,
    with every feature above already on: the state archive of `snapshot_save` / `snapshot_restore`.  The learner view is set after
    construction: bind the archive behind it (`set_snapshots`) where one is wanted.
    """

    def __init__(
        self,
        batch: int = 1,
        *,
        T="Float32",
        height_tile_map_tu: int = 8,
        width_tile_map_tu: int = 16,
        num_directions: int = 128,
        player_radius_wu: float = 1 / 8,
        position_increment_wu: float = 1 / 8,
        seed: int = 0,
        rng=None,
        R="Float32",
        semi_field_of_view_wu: float = 2 / 3,
        num_rays: int = 512,
        pu_per_tu: int = 32,
        camera_height_tile_wu: float = 1.0,
        height_camera_view_pu: int = 256,
        device: int = 0,
        auto_reset: bool = False,
        agent_id_offset: int = 0,
        dda_tie_break: int = 0,
        dda_distance: int = 0,
        normalize_mode: int = 0,
        out_of_bounds: int = 0,
        render_top_view: bool = False,
        library: Optional[str] = None,
        max_episode_steps: int = 0,
        walls=None,
        wall_index=None,
        goal_distance: bool = False,
        guide: bool = False,
        seen_map: bool = False,
        frontier: bool = False,
        local_map=None,
        wall_bank=None,
        wall_bank_weights=None,
        wall_generator=None,
        wall_caves=None,
        wall_rooms=None,
        episode_stats: bool = False,
        visit_map=None,
        snapshots: int = 0,
        start_distance=None,
    ):
        f32_names = ("Float32", "float32", "<class 'numpy.float32'>")
        f64_names = ("Float64", "float64", "<class 'numpy.float64'>", "<class 'float'>")
        if str(T) not in f32_names + f64_names:
            raise NotImplementedError(f"world-unit type T = {T!r}: only Float32 and Float64 are built")
        r_names = {**{n: (np.float32, _capi.RCW_REWARD_FLOAT32) for n in f32_names},
                   **{n: (np.float64, _capi.RCW_REWARD_FLOAT64) for n in f64_names},
                   **{n: (np.int32, _capi.RCW_REWARD_INT32) for n in ("Int32", "int32", "<class 'numpy.int32'>")},
                   **{n: (np.int64, _capi.RCW_REWARD_INT64) for n in ("Int64", "Int", "int64", "<class 'numpy.int64'>",
                                                                     "<class 'int'>")}}
        if str(R) not in r_names:
            raise NotImplementedError(f"reward type R = {R!r}: Float32, Float64, Int32 and Int64 are built")
        self.T = np.float64 if str(T) in f64_names else np.float32
        self.R, reward_type = r_names[str(R)]
        # `library`: None = the shipped librcw_hip.so; "dev" (or a path) = the development build, which also reads the
        # RCW_* tuning knobs (overrides of what the rules compute; the kernels are the shipped ones: csrc/Makefile `dev`)
        self._lib = _capi.load(library)
        cfg = _capi.RcwConfig()
        _capi.check(self._lib.rcw_config_default(C.byref(cfg)), self._lib)
        cfg.height_tile_map_tu = height_tile_map_tu
        cfg.width_tile_map_tu = width_tile_map_tu
        cfg.num_directions = num_directions
        cfg.player_radius_wu = np.float32(player_radius_wu)          # convert(T, .) SR:263
        cfg.position_increment_wu = np.float32(position_increment_wu)
        cfg.semi_field_of_view_wu = np.float32(semi_field_of_view_wu)
        cfg.num_rays = num_rays
        cfg.pu_per_tu = pu_per_tu
        cfg.camera_height_tile_wu = np.float32(camera_height_tile_wu)
        cfg.height_camera_view_pu = height_camera_view_pu
        cfg.auto_reset = 1 if auto_reset else 0
        cfg.agent_id_offset = agent_id_offset
        cfg.dda_tie_break = dda_tie_break
        cfg.dda_distance = dda_distance
        cfg.normalize_mode = normalize_mode
        cfg.out_of_bounds = out_of_bounds
        cfg.render_top_view = 1 if render_top_view else 0
        cfg.reward_type = reward_type                 # R, with goal_reward = one(R) SR:82
        cfg.goal_reward = 1.0
        cfg.goal_reward_f64 = 1.0
        # convert(T, .) of the caller's values (SR:263-270): for T = Float64 the Float64 value itself
        cfg.world_unit_bits = 64 if self.T is np.float64 else 32
        cfg.player_radius_wu_f64 = float(player_radius_wu)
        cfg.position_increment_wu_f64 = float(position_increment_wu)
        cfg.semi_field_of_view_wu_f64 = float(semi_field_of_view_wu)
        cfg.camera_height_tile_wu_f64 = float(camera_height_tile_wu)
        self.cfg = cfg
        self.batch = int(batch)
        self.device = int(device)
        self.seed = int(seed)
        self._handle = _Handle(self._lib)    # owns the native handle; `self._h` reads it
        self._check(self._lib.rcw_create(C.byref(cfg), self.batch, self.device, self.seed, C.byref(self._handle.h)))
        self.world = SingleRoomWorld(self)
        self._held = []          # (event, tensors): torch tensors a NON-torch stream may still be reading (_release_after_use)
        self._free_events = []
        self._torch_owned_stream = None
        # In a process that already uses torch the engine runs on a stream TORCH owns (never destroyed, so
        # `Tensor.record_stream` on it is safe for tensors that outlive the engine).  A caller that has not imported torch
        # does not get it imported here and keeps the library's own stream (`stream_ptr()`).
        torch = sys.modules.get("torch")
        if torch is not None:
            try:
                if torch.cuda.is_available():
                    self.set_stream(torch.cuda.Stream(device=self.device))
            except BaseException:
                self._handle.close()             # nothing of a half-made environment stays allocated
                raise
        self.host_syncs = 0      # host synchronisations / device-to-host getters issued through this object (bench.py --api rlbase)
        self.rng = rng
        if rng is not None:
            # the reference's constructor consumes its rng TWICE: the draws of SR:62-74, then reset!(world) SR:105 -> SR:120-128
            try:
                _reset_from_rng(self, rng, None, construction=True)
            except BaseException:
                self._handle.close()
                raise
        self._rng_walls = None   # bool (B, H, W): each agent's layout, kept for the host-drawn resets of an `rng` environment only
        if walls is not None:
            try:
                self.set_walls(walls, wall_index)
            except BaseException:
                self._handle.close()
                raise
        elif wall_index is not None:
            self._handle.close()
            raise ValueError("wall_index needs walls")
        if max_episode_steps:
            try:
                self.set_time_limit(max_episode_steps)
            except BaseException:
                self._handle.close()
                raise
        if wall_bank is not None:
            try:
                self.set_wall_bank(wall_bank, wall_bank_weights)
            except BaseException:
                self._handle.close()
                raise
        elif wall_bank_weights is not None:
            self._handle.close()
            raise ValueError("wall_bank_weights needs wall_bank")
        for setter, keywords in ((self.set_wall_generator, wall_generator), (self.set_wall_caves, wall_caves), (self.set_wall_rooms, wall_rooms)):
            if keywords is not None:
                try:
                    setter(**dict(keywords))
                except BaseException:
                    self._handle.close()
                    raise
        if goal_distance:
            try:
                self.set_goal_distance(True)
            except BaseException:
                self._handle.close()
                raise
        if guide:
            try:
                self.set_guide(True)
            except BaseException:
                self._handle.close()
                raise
        if seen_map:
            try:
                self.set_seen_map(True)
            except BaseException:
                self._handle.close()
                raise
        if frontier:
            try:
                self.set_frontier(True)
            except BaseException:
                self._handle.close()
                raise
        if local_map is not None:
            try:
                self.set_local_map(**local_map) if isinstance(local_map, dict) else self.set_local_map(local_map)
            except BaseException:
                self._handle.close()
                raise
        if episode_stats:
            try:
                self.set_episode_stats(True)
            except BaseException:
                self._handle.close()
                raise
        if visit_map is not None and visit_map is not False:
            try:
                self.set_visit_map(**visit_map) if isinstance(visit_map, dict) else self.set_visit_map()
            except BaseException:
                self._handle.close()
                raise
        if start_distance is not None and start_distance is not False:
            try:
                self.set_start_distance(*start_distance) if isinstance(start_distance, (tuple, list)) else self.set_start_distance()
            except BaseException:
                self._handle.close()
                raise
        if snapshots:
            try:
                self.set_snapshots(snapshots)
            except BaseException:
                self._handle.close()
                raise
        # colour fields of the reference struct SR:241-256
        self.floor_color = cfg.floor_color
        self.ceiling_color = cfg.ceiling_color
        self.wall_dim_1_color = cfg.wall_dim_1_color
        self.wall_dim_2_color = cfg.wall_dim_2_color
        self.goal_dim_1_color = cfg.goal_dim_1_color
        self.goal_dim_2_color = cfg.goal_dim_2_color
        self.camera_height_tile_wu = cfg.camera_height_tile_wu
        self.height_camera_view_pu = cfg.height_camera_view_pu

    def _check(self, rc: int) -> None:
        _capi.check(rc, self._lib)

    @property
    def _h(self):
        """The native `rcw_handle*` (NULL once closed)."""
        return self._handle.h

    # ---- lifetime -------------------------------------------------------------------
    def close(self):
        """`rcw_destroy`.  Device aliases made earlier (`camera_view`, `reward(env).torch()`, ...) dangle from here on,
        as any view of freed memory does; without an explicit close the memory lives as long as the last of them."""
        handle = getattr(self, "_handle", None)
        if handle is not None:
            handle.close()
        self._held = []
        self._drop(*_CACHES)

    def _drop(self, *groups: str) -> None:
        """Forget the cached aliases of `groups` (`_CACHES`): the next access asks the library again."""
        for group in groups:
            for name in _CACHES[group]:
                self.__dict__.pop(name, None)

    # (no __del__: an environment that is dropped without close() lets go of its _Handle, and the engine is destroyed
    # when the last holder does — this object, or the last torch tensor made over engine memory, whichever lives longer)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- device views ---------------------------------------------------------------
    def _sync(self):
        self.host_syncs += 1
        self._check(self._lib.rcw_sync(self._h))

    def sync(self):
        self._sync()

    def _copy_device_array(self, arr: DeviceArray) -> np.ndarray:
        if arr.ptr == self._obs_ptr():
            out = np.empty(arr.shape, dtype=arr.dtype)
            self._check(self._lib.rcw_obs_copy(self._h, _as_ptr(out), 0, self.batch))
            return out
        import torch

        return torch.as_tensor(arr, device=f"cuda:{self.device}").cpu().numpy()

    def _obs_ptr(self) -> int:
        p = C.c_void_p()
        self._check(self._lib.rcw_obs_device_ptr(self._h, C.byref(p)))
        return int(p.value)

    @property
    def camera_view(self) -> DeviceArray:
        """The observation batch, aliased (SR:300, SR:576): uint32 (B, N, H_cam) in C order."""
        return DeviceArray(self._obs_ptr(), (self.batch, self.cfg.num_rays, self.cfg.height_camera_view_pu),
                           np.uint32, self, self._sync)

    @property
    def top_view(self) -> DeviceArray:
        """`env.top_view` (SR:302, needs render_top_view=True): uint32 (B, W*pu, H*pu) in C order ==
        Julia (H*pu, W*pu, B)."""
        p = C.c_void_p()
        self._check(self._lib.rcw_top_view_device_ptr(self._h, C.byref(p)))
        pu = self.cfg.pu_per_tu
        return DeviceArray(p.value, (self.batch, self.cfg.width_tile_map_tu * pu, self.cfg.height_tile_map_tu * pu),
                           np.uint32, self, self._sync)

    def top_view_host(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        n = self.batch - first if count is None else count
        pu = self.cfg.pu_per_tu
        out = np.empty((n, self.cfg.width_tile_map_tu * pu, self.cfg.height_tile_map_tu * pu), dtype=np.uint32)
        self._check(self._lib.rcw_top_view_copy(self._h, _as_ptr(out), first, n))
        return out

    def camera_view_host(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        n = self.batch - first if count is None else count
        out = np.empty((n, self.cfg.num_rays, self.cfg.height_camera_view_pu), dtype=np.uint32)
        self._check(self._lib.rcw_obs_copy(self._h, _as_ptr(out), first, n))
        return out

    def columns(self, first: int = 0, count: Optional[int] = None):
        """Compact per-column descriptors (height_line_pu int32 (n, N), colour id uint8 (n, N))."""
        n = self.batch - first if count is None else count
        h = np.empty((n, self.cfg.num_rays), dtype=np.int32)
        c = np.empty((n, self.cfg.num_rays), dtype=np.uint8)
        self._check(self._lib.rcw_columns(self._h, first, n, _as_ptr(h), _as_ptr(c)))
        return h, c

    def columns_device(self):
        hp, cp = C.c_void_p(), C.c_void_p()
        self._check(self._lib.rcw_columns_device_ptr(self._h, C.byref(hp), C.byref(cp)))
        shape = (self.batch, self.cfg.num_rays)
        return (DeviceArray(hp.value, shape, np.int32, self, self._sync),
                DeviceArray(cp.value, shape, np.uint8, self, self._sync))

    def expand_columns(self, height_line_pu, colour_id, out=None):
        """Descriptors (CUDA tensors (n, N) int32 / uint8, e.g. gathered from other GPUs) ->
        frames (n, N, H_cam) as a torch CUDA tensor, with this engine's colours (rcw_expand_columns).
        Stream-ordered on the engine's stream behind the producer of the descriptors (torch's current
        stream); no host synchronisation.  Consumers on another stream wait for `env.torch_stream()`."""
        import torch

        n = int(height_line_pu.shape[0])
        if tuple(height_line_pu.shape) != (n, self.cfg.num_rays) or tuple(colour_id.shape) != (n, self.cfg.num_rays):
            raise ValueError("descriptor shape must be (n, num_rays)")
        if height_line_pu.dtype != torch.int32 or colour_id.dtype != torch.uint8:
            raise ValueError("descriptors must be int32 / uint8")
        h = height_line_pu.contiguous()
        c = colour_id.contiguous()
        if out is None:
            out = torch.empty((n, self.cfg.num_rays, self.cfg.height_camera_view_pu), dtype=torch.uint32,
                              device=f"cuda:{self.device}")
        cross = self._order_behind_torch()
        self._check(self._lib.rcw_expand_columns(self._h, C.c_void_p(h.data_ptr()), C.c_void_p(c.data_ptr()), n,
                                                 C.c_void_p(out.data_ptr())))
        if cross:
            self._release_after_use(h, c, out)
        return out

    # ---- the learner view (rcw_set_learner_view) ------------------------------------------------------------------
    _VIEW_FORMATS = {None: _capi.RCW_VIEW_OFF, "rgb": _capi.RCW_VIEW_RGB8, "gray": _capi.RCW_VIEW_GRAY8,
                     "depth": _capi.RCW_VIEW_DEPTH8, "rgbd": _capi.RCW_VIEW_RGBD8, "grayd": _capi.RCW_VIEW_GRAYD8}
    _VIEW_CHANNELS = {"rgb": 3, "gray": 1, "depth": 1, "rgbd": 4, "grayd": 2}

    def set_learner_view(self, format: Optional[str] = "gray", size=None, layout: str = "chw", camera_view: bool = True,
                         stack: int = 1) -> None:
        """Also render a uint8 observation a learner consumes at every reset / set_state / step: `format` "gray" or "rgb",
        "depth" (one plane of inverse depth: 255 at or nearer than the distance at which a wall fills the column, 0 infinitely
        far — include/rcw.h), "rgbd" (R, G, B, D) or "grayd" (Y, D) (None: off), `size` (h, w) with h <= height_camera_view_pu and w <= num_rays (None: full size; each output pixel is
        the rounded mean of its box of camera pixels), `layout` "chw" (B, C, h, w) or "hwc" (B, h, w, C).
        `camera_view=False` (RCW_VIEW_ONLY): steps skip the uint32 camera view — `camera_view` then holds the last frames
        rendered until `update_camera_view_(env)`.  Renders the current state at once.
        `stack=k` (1..16, "chw" only): the view holds each agent's last k frames, uint8 (B, k C, h, w), slot 0 (channels
        [0, C)) the oldest and slot k - 1 the newest.  The engine keeps it per episode on the device: a step shifts the slots
        and appends the new frame; reset_, set_state and the step in which auto_reset restarts an agent fill all k slots of
        that agent with its new frame, so no frame of a finished episode shows in the next one (include/rcw.h)."""
        formats = self._VIEW_FORMATS
        layouts = {"chw": _capi.RCW_VIEW_CHW, "hwc": _capi.RCW_VIEW_HWC}
        if format not in formats:
            raise ValueError(f"unknown learner view format {format!r} (\"gray\", \"rgb\", \"depth\", \"rgbd\", \"grayd\" or None)")
        if layout not in layouts:
            raise ValueError(f"unknown learner view layout {layout!r} (\"chw\" or \"hwc\")")
        if format is None and not camera_view:
            raise ValueError("camera_view=False needs a learner view format")
        h, w = (self.cfg.height_camera_view_pu, self.cfg.num_rays) if size is None else (int(size[0]), int(size[1]))
        flags = 0 if camera_view else _capi.RCW_VIEW_ONLY
        stack = int(stack)
        if stack == 1:
            self._check(self._lib.rcw_set_learner_view(self._h, formats[format], layouts[layout], h, w, flags))
        else:
            self._check(self._lib.rcw_set_learner_view_stack(self._h, formats[format], layouts[layout], h, w, flags, stack))
        self._view_only = not camera_view                # (RLBase.state refuses the stale camera view of such a handle)
        self._drop("learner_view")

    def learner_view_info(self) -> dict:
        """The current learner view settings (rcw_learner_view_info): format, layout, size, camera_view."""
        v = [C.c_int32() for _ in range(5)]
        self._check(self._lib.rcw_learner_view_info(self._h, *[C.byref(x) for x in v]))
        fmt, lay, h, w, flags = (x.value for x in v)
        return {"format": {value: name for name, value in self._VIEW_FORMATS.items()}[fmt],
                "layout": "hwc" if lay == _capi.RCW_VIEW_HWC else "chw", "size": (h, w),
                "camera_view": not (flags & _capi.RCW_VIEW_ONLY)}

    @property
    def learner_view_stack(self) -> int:
        """The number of frame slots of the learner view (rcw_learner_view_stack): `set_learner_view`'s `stack`, 0 without a view."""
        k = C.c_int32()
        self._check(self._lib.rcw_learner_view_stack(self._h, C.byref(k)))
        return k.value

    def _learner_view_shape(self, n: int, info: Optional[dict] = None, stack: Optional[int] = None):
        info = info or self.learner_view_info()
        if info["format"] is None:
            raise RuntimeError("this environment has no learner view: call set_learner_view first")
        c = self._VIEW_CHANNELS[info["format"]]
        h, w = info["size"]
        k = self.learner_view_stack if stack is None else stack
        return (n, k * c, h, w) if info["layout"] == "chw" else (n, h, w, c)

    @property
    def learner_view(self) -> DeviceArray:
        """The learner view batch, aliased device memory: uint8 (B, stack * C, h, w) or (B, h, w, C), rewritten in place by every
        step in stream order (`.torch(sync=False)` for a consumer on the GPU)."""
        shape = self._learner_view_shape(self.batch)
        p = C.c_void_p()
        self._check(self._lib.rcw_learner_view_device_ptr(self._h, C.byref(p)))
        alias = self.__dict__.get("_learner_view_alias")
        if alias is None or alias.ptr != p.value or alias.shape != shape:
            alias = self._learner_view_alias = DeviceArray(p.value, shape, np.uint8, self, self._sync,
                                                           host_getter=lambda: self.learner_view_host())
        return alias

    def learner_view_host(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """Agents [first, first + count) of the learner view, copied to the host (waits for the engine's stream)."""
        n = self.batch - first if count is None else count
        out = np.empty(self._learner_view_shape(n), dtype=np.uint8)
        self._check(self._lib.rcw_learner_view_copy(self._h, _as_ptr(out), first, n))
        return out

    def expand_columns_view(self, height_line_pu, colour_id, out=None):
        """Descriptors (CUDA tensors (n, N) int32 / uint8) -> this environment's learner view of them, a uint8 torch CUDA
        tensor in the view's shape (rcw_expand_columns_view).  Stream-ordered like `expand_columns`."""
        import torch

        n = int(height_line_pu.shape[0])
        if tuple(height_line_pu.shape) != (n, self.cfg.num_rays) or tuple(colour_id.shape) != (n, self.cfg.num_rays):
            raise ValueError("descriptor shape must be (n, num_rays)")
        if height_line_pu.dtype != torch.int32 or colour_id.dtype != torch.uint8:
            raise ValueError("descriptors must be int32 / uint8")
        shape = self._learner_view_shape(n, stack=1)              # (single-frame, whatever the handle's stack)
        h = height_line_pu.contiguous()
        c = colour_id.contiguous()
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=f"cuda:{self.device}")
        elif tuple(out.shape) != shape or out.dtype != torch.uint8 or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous uint8 tensor of shape {shape}")
        cross = self._order_behind_torch()
        self._check(self._lib.rcw_expand_columns_view(self._h, C.c_void_p(h.data_ptr()), C.c_void_p(c.data_ptr()), n,
                                                      C.c_void_p(out.data_ptr())))
        if cross:
            self._release_after_use(h, c, out)
        return out

    def _constant_actions(self, action: int):
        """A device array holding `action` for every agent (None without torch: the host path is taken)."""
        cache = self.__dict__.setdefault("_constant_action_buffers", {})
        buf = cache.get(action)
        if buf is None and action not in cache:
            try:
                import torch

                buf = torch.full((self.batch,), action, dtype=torch.uint8, device=f"cuda:{self.device}")
                torch.cuda.synchronize(self.device)      # (made on torch's stream, used on the engine's from now on)
            except Exception:                            # noqa: BLE001 — no torch / no CUDA torch: stay on the host path
                buf = None
            cache[action] = buf
        return buf

    def _order_behind_torch(self, *tensors):
        """Make the engine's stream wait for torch's current stream (the producer of `tensors`), and keep the
        tensors alive until the engine has consumed them: `_release_after_use` must follow the launch.  Without
        the hold, a tensor the caller drops right after the call goes back to torch's caching allocator, which
        may hand the block out again — to be overwritten on torch's stream — before the engine has read it."""
        import torch

        producer = torch.cuda.current_stream(self.device)
        if producer.cuda_stream == self.stream_ptr():
            return False
        self.torch_stream().wait_stream(producer)
        return True

    def _release_after_use(self, *tensors):
        """Keep `tensors` (handed to the engine on its stream) from being recycled by torch's caching allocator before the
        engine has used them, although the caller may drop them right after the call.

        On a stream torch owns (the default: see __init__) this is `Tensor.record_stream` — no bookkeeping, never blocks.
        On any other stream (the library's own, a caller's raw hipStream_t) record_stream must NOT be used: the
        allocator records an event on every recorded stream when the tensor is finally freed, which may be long after
        `close()` has destroyed that stream — an event record on a destroyed HIP stream is a use after free inside the
        runtime (the segmentation fault of rounds 2 and 3).  There, references are held instead until an
        event recorded now on the engine's stream has completed (a ring of 16 reusable events; the host only ever blocks
        when it runs 16 launches ahead of the GPU)."""
        import torch

        if self._stream_is_torch_owned():
            ts = self.torch_stream()
            for t in tensors:
                t.record_stream(ts)
            return
        ring, free = self._held, self._free_events
        while ring and ring[0][0].query():
            free.append(ring.pop(0)[0])
        if len(ring) >= 16:
            ev, _ = ring.pop(0)
            ev.synchronize()
            free.append(ev)
        ev = free.pop() if free else torch.cuda.Event()
        ev.record(self.torch_stream())
        ring.append((ev, tensors))

    # ---- the features' per-agent words and tile-order arrays: one readout, one alias for all of `_WORDS` and `_TILES` ----
    def _word_host(self, row: _Words, k: int) -> np.ndarray:
        """Word `k` of a group, copied to the host (waits for the engine's stream)."""
        out = np.empty(self.batch, dtype=row.words[k][1])
        args = [None] * len(row.words)
        args[k] = _as_ptr(out)
        self.host_syncs += 1
        self._check(getattr(self._lib, row.host)(self._h, *args))
        return out

    def _device_words(self, row: _Words):
        """A group's words as `DeviceArray`s (B,), made once and cached under `row.cache` until a setter drops them."""
        p = [C.c_void_p() for _ in row.words]
        self._check(getattr(self._lib, row.device_ptr)(self._h, *[C.byref(q) for q in p]))
        group = tuple(DeviceArray(p[k].value, (self.batch,), dtype, self, self._sync, host_getter=lambda k=k: self._word_host(row, k))
                      for k, (_, dtype) in enumerate(row.words))
        if row.namespace:
            group = types.SimpleNamespace(**{name: x for (name, _), x in zip(row.words, group)})
        self.__dict__[row.cache] = group
        return group

    def _tiles_shape(self, row: _Tiles):
        lead = (self.batch, self.visit_map_info["sectors"]) if row.sectors else (self.batch,)
        return lead + (self.cfg.width_tile_map_tu, self.cfg.height_tile_map_tu)      # tile (i, j) at (i - 1) + H (j - 1)

    def _tiles_host(self, row: _Tiles, device_order: bool = False) -> np.ndarray:
        """A tile-order array copied to the host (waits for the engine's stream): (B, [sectors,] H, W), indexed like
        `env.world.walls` — or (`device_order`) as it lies on the device, (B, [sectors,] W, H)."""
        out = np.empty(self._tiles_shape(row), dtype=row.dtype)
        self.host_syncs += 1
        self._check(getattr(self._lib, row.host)(self._h, 0, self.batch, _as_ptr(out)))
        return out if device_order else np.ascontiguousarray(np.swapaxes(out, -1, -2))

    def _tiles_device(self, row: _Tiles) -> DeviceArray:
        """A tile-order array where it lives; a new alias at every call (the pointer moves with the feature's setter)."""
        p = C.c_void_p()
        self._check(getattr(self._lib, row.device_ptr)(self._h, C.byref(p)))
        return DeviceArray(p.value, self._tiles_shape(row), row.dtype, self, self._sync, host_getter=lambda: self._tiles_host(row, device_order=True))

    def reward_device(self) -> DeviceArray:
        """`world.reward` (SR:33) where it lives: R (B,) in device memory, stable for the handle's lifetime, rewritten
        by every step in stream order.  The same object on every call (its torch alias is made once)."""
        if getattr(self, "_reward_dev", None) is None:
            p = C.c_void_p()
            self._check(self._lib.rcw_reward_device_ptr(self._h, C.byref(p)))
            self._reward_dev = DeviceArray(p.value, (self.batch,), self.R, self, self._sync,
                                           host_getter=lambda: self.world.reward)
        return self._reward_dev

    def done_device(self, as_bool: bool = False) -> DeviceArray:
        """`world.done` (SR:35) in device memory: one byte per agent (`as_bool`: the same bytes viewed as Bool)."""
        name = "_done_dev_bool" if as_bool else "_done_dev"
        if getattr(self, name, None) is None:
            p = C.c_void_p()
            self._check(self._lib.rcw_done_device_ptr(self._h, C.byref(p)))
            getter = (lambda: self.world.done) if as_bool else (lambda: self.world.done.astype(np.uint8))
            setattr(self, name, DeviceArray(p.value, (self.batch,), np.bool_ if as_bool else np.uint8, self, self._sync,
                                            host_getter=getter))
        return getattr(self, name)

    # ---- the episode time limit (include/rcw.h, rcw_set_time_limit) -------------------
    def set_time_limit(self, max_episode_steps: int) -> None:
        """An episode ends after `max_episode_steps` steps without the goal: the step that reaches the limit sets `truncated`, and under
        `auto_reset` the next action restarts the agent as it restarts a done one (the action is ignored, the episode counter moves, the
        frame stack refills).  0 switches the limit off (the default).  Decided on the device by the step's own kernels: no host
        synchronisation.  Every call zeroes `episode_steps` and `truncated` of every agent — the limit counts from the call."""
        self._check(self._lib.rcw_set_time_limit(self._h, int(max_episode_steps)))

    @property
    def time_limit(self) -> int:
        n = C.c_int32()
        self._check(self._lib.rcw_time_limit(self._h, C.byref(n)))
        return int(n.value)

    def truncated_device(self, as_bool: bool = False) -> DeviceArray:
        """`truncated` in device memory: one byte per agent (`as_bool`: the same bytes viewed as Bool), rewritten by every step in
        stream order while a time limit is set.  The same object on every call, like `done_device`."""
        name = "_truncated_dev_bool" if as_bool else "_truncated_dev"
        if getattr(self, name, None) is None:
            p = C.c_void_p()
            self._check(self._lib.rcw_truncated_device_ptr(self._h, C.byref(p)))
            getter = (lambda: self.world.truncated) if as_bool else (lambda: self.world.truncated.astype(np.uint8))
            setattr(self, name, DeviceArray(p.value, (self.batch,), np.bool_ if as_bool else np.uint8, self, self._sync,
                                            host_getter=getter))
        return getattr(self, name)

    def episode_steps_device(self) -> DeviceArray:
        """`episode_steps` in device memory: uint32 (B,); at the step that sets `done` or `truncated` it is the episode's length."""
        if getattr(self, "_episode_steps_dev", None) is None:
            p = C.c_void_p()
            self._check(self._lib.rcw_episode_steps_device_ptr(self._h, C.byref(p)))
            self._episode_steps_dev = DeviceArray(p.value, (self.batch,), np.uint32, self, self._sync,
                                                  host_getter=lambda: self.world.episode_steps)
        return self._episode_steps_dev

    # ---- the goal distance (include/rcw.h, rcw_set_goal_distance) ----------------------
    def set_goal_distance(self, on: bool = True) -> None:
        """Keep each agent's shortest-path distance to its goal on the device: the breadth-first distance in tiles through the agent's
        walls (`goal_distance_field`), looked up at the player's tile after every call (`goal_distance`, -1: unreachable), its value at
        the start of the episode (`goal_start_distance`: SPL's path length) and what the last step gained (`goal_progress`: potential-
        based shaping is `r + c * env.goal_progress.torch(sync=False)`).  Follows resets, `set_state`, `set_walls` and `auto_reset`
        restarts with no host synchronisation.  Switching it on (again) recomputes everything and makes the current state the
        episode's start; the device arrays handed out before are invalid after every call."""
        self._drop("goal_distance")
        if not on:
            self._drop("guide")                                   # (the guide reads the field: it goes with it)
        self._check(self._lib.rcw_set_goal_distance(self._h, 1 if on else 0))

    @property
    def goal_distance_enabled(self) -> bool:
        n = C.c_int32()
        self._check(self._lib.rcw_goal_distance_enabled(self._h, C.byref(n)))
        return bool(n.value)

    goal_distance = _word("goal_distance", 0,
        """int32 (B,) in device memory: tiles from the player's tile to the goal through the walls; -1 where there is no path (or the
        player is off the map).  Rewritten behind every step, reset, `set_state` and `set_walls` in stream order.""")
    goal_start_distance = _word("goal_distance", 1,
        """int32 (B,): `goal_distance` as of the start of each agent's current episode.""")
    goal_progress = _word("goal_distance", 2,
        """int32 (B,): tiles the last step brought each agent closer to its goal (negative: farther); 0 for an agent the call restarted
        or reset, and where either distance is -1.""")
    goal_distance_field = _tiles("goal_distance_field",
        """uint16 (B, H, W), a host copy: `field[b, i-1, j-1]` is the distance of tile (i, j) from agent b's goal, 0xFFFF for walls and
        tiles without a path — indexed like `env.world.walls`.""")

    def goal_distance_field_device(self) -> DeviceArray:
        """The field where it lives: uint16 (B, W, H) in device memory — the tile map's own order, `[b, j-1, i-1]`."""
        return self._tiles_device(_TILES["goal_distance_field"])

    # ---- the guide (include/rcw.h, rcw_set_guide) ----------------------------------------
    def set_guide(self, on: bool = True) -> None:
        """Keep, on the device, the action that follows each agent's shortest path to its goal (`guide_action`, uint8 in 1..4: what `act_`
        takes as it stands) and the direction index it wants the agent to face (`guide_heading`, int32, -1: no advice — no path, or on
        the goal tile; the action is then a turn on the spot), rewritten behind every call that moves an agent, a goal or a wall, a new
        direction table and a `snapshot_restore`.  The label imitation learning and DAgger need, with no host in the loop:
        `torch.where(beta, env.guide_action.torch(sync=False), policy_action)`.  Switching it on enables the goal distance first where
        that is off; `set_goal_distance(False)` switches the guide off too.  The device arrays handed out before are invalid after
        every call."""
        self._drop("guide")
        if on and not self.goal_distance_enabled:
            self.set_goal_distance(True)
        self._check(self._lib.rcw_set_guide(self._h, 1 if on else 0))

    @property
    def guide_info(self) -> dict:
        """`enabled`, and `promised`: whether position_increment + player_radius <= 0.5, for which an agent that follows the guide is
        promised to arrive (rcw_guide_info)."""
        v = [C.c_int32(), C.c_int32()]
        self._check(self._lib.rcw_guide_info(self._h, C.byref(v[0]), C.byref(v[1])))
        return {"enabled": bool(v[0].value), "promised": bool(v[1].value)}

    @property
    def guide_enabled(self) -> bool:
        return self.guide_info["enabled"]

    guide_action = _word("guide", 0,
        """uint8 (B,): the guide's action for every agent, always in 1..4.  `.torch(sync=False)` on the GPU — `act_` takes it as it is —,
        `np.asarray(...)` for a host copy.""")
    guide_heading = _word("guide", 1,
        """int32 (B,): the 0-based direction index the guide wants each agent to face, -1 where it has no advice.""")

    # ---- episode statistics (include/rcw.h, rcw_set_episode_stats) ----------------------
    EPISODE_STATS_COLUMNS = ("episodes", "successes", "truncations", "sum_length", "sum_moves", "spl_episodes", "sum_spl_q16")

    def set_episode_stats(self, on: bool = True) -> None:
        """Keep, on the device, how each agent's episodes end — `episode_stats.finished / outcome / length / moves / level / spl_q16 /
        episodes` — and their sums over the batch and per level of the layout source that is live NOW (`episode_stats_table`): what a
        "record episode statistics" wrapper keeps, with no host synchronisation.  Enable the wall bank or the generator (and the goal
        distance, for SPL) first: while the statistics are on, the layout source cannot be changed.  Switching it on (again) zeroes
        everything and begins every agent's record at its current state; the device arrays handed out before are invalid after every
        call."""
        self._drop("episode_stats")
        self._check(self._lib.rcw_set_episode_stats(self._h, 1 if on else 0))

    @property
    def episode_stats_info(self) -> dict:
        """`enabled`, and the table's level rows: `rows` of them, the first for level `first` (rcw_episode_stats_info)."""
        v = [C.c_int32(), C.c_int32(), C.c_int32()]
        self._check(self._lib.rcw_episode_stats_info(self._h, *[C.byref(x) for x in v]))
        return {"enabled": bool(v[0].value), "rows": v[1].value, "first": v[2].value}

    @property
    def episode_stats_enabled(self) -> bool:
        return self.episode_stats_info["enabled"]

    episode_stats = _word("episode_stats", None,
        """The seven per-agent words as `DeviceArray`s (B,): `finished` (uint8, 1 iff the last step closed the agent's record), `outcome`
        (uint8: 0 open, 1 success, 2 truncated), `length`, `moves` (uint32), `level` (int32, -1 without a layout source), `spl_q16` (int32,
        SPL * 65536, -1 where undefined) and `episodes` (uint32).  The words keep a finished episode until the agent begins another:
        read them where `finished` is set.  `.torch(sync=False)` on the GPU, `np.asarray(...)` for a host copy.""")

    def episode_stats_table(self, device: bool = False):
        """The sums over the records closed since enabling (or the last `episode_stats_clear`).  A dict of numpy arrays: `totals` — the
        seven `EPISODE_STATS_COLUMNS` of the whole batch, by name —, `levels` — the same per level, each an array of `rows` entries, level
        `first + k` at k —, `first`, and `spl`, the mean SPL as floats (`totals`' and per level; NaN where no close had it defined).
        `device=True`: the raw uint64 (1 + rows, 8) `DeviceArray` instead, row 0 the totals."""
        rows = self.episode_stats_info["rows"]
        if device:
            p = C.c_void_p()
            self._check(self._lib.rcw_episode_stats_table_device_ptr(self._h, C.byref(p)))
            return DeviceArray(p.value, (1 + rows, 8), np.uint64, self, self._sync, host_getter=lambda: self._episode_stats_table_host(rows))
        t = self._episode_stats_table_host(rows)
        cols = self.EPISODE_STATS_COLUMNS
        with np.errstate(divide="ignore", invalid="ignore"):
            spl = np.where(t[:, 5] > 0, t[:, 6] / 65536.0 / t[:, 5], np.nan)
        return {"totals": {c: int(t[0, k]) for k, c in enumerate(cols)}, "levels": {c: t[1:, k].copy() for k, c in enumerate(cols)},
                "first": self.episode_stats_info["first"], "spl": {"totals": float(spl[0]), "levels": spl[1:].copy()}}

    def _episode_stats_table_host(self, rows: int) -> np.ndarray:
        out = np.empty((1 + rows, 8), dtype=np.uint64)
        self.host_syncs += 1
        self._check(self._lib.rcw_episode_stats_table(self._h, _as_ptr(out)))
        return out

    def episode_stats_clear(self) -> None:
        """Zero the table, stream-ordered and without waiting for the stream; the per-agent words stay.  What a replay loop calls after
        it has read the table."""
        self._check(self._lib.rcw_episode_stats_clear(self._h))

    # ---- the start rule (include/rcw.h, rcw_set_start_distance) --------------------------
    def set_start_distance(self, lo=1, hi=None) -> None:
        """Place the player of every episode that starts from now on — `reset_`, a done or truncated restart under `auto_reset`, a
        layout source's restart, `set_walls` — on a tile whose shortest-path distance to the goal lies in `lo..hi` (`hi=None`: no upper
        bound), on the device and reproducibly (`layouts.start_rule` replays it).  Where the band lies beyond what the goal's region
        holds, the farthest tiles are taken; `start_placed` says which (1 in the band, 2 clamped, 3 the drawn pose kept: nothing but
        the goal can be reached).  `(1, None)` is the plain guarantee that the goal can be reached.  No agent moves when it is
        switched on; calling it again only changes the band, with no wait — a curriculum moves it between steps.
        `set_start_distance(None)` switches it off.  An environment built with `rng` draws its resets on the host and takes no
        start rule."""
        if lo is None or lo is False:
            self._drop("start_distance")
            self._check(self._lib.rcw_set_start_distance(self._h, 0, 0, 0))
            return
        self._refuse_rng("start rule")
        top = _capi.RCW_START_DISTANCE_MAX
        hi = top if hi is None else hi
        for name, v in (("lo", lo), ("hi", hi)):
            if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not -2 ** 31 <= int(v) < 2 ** 31:
                raise ValueError(f"{name} must be an integer, got {v!r}")
        if not self.start_distance_info["enabled"]:
            self._drop("start_distance")
        self._check(self._lib.rcw_set_start_distance(self._h, 1, int(lo), int(hi)))

    @property
    def start_distance_info(self) -> dict:
        """`enabled`, `lo`, `hi` of the start rule (rcw_start_distance_info); zeros while it is off."""
        v = [C.c_int32() for _ in range(3)]
        self._check(self._lib.rcw_start_distance_info(self._h, *[C.byref(x) for x in v]))
        return {"enabled": bool(v[0].value), "lo": v[1].value, "hi": v[2].value}

    start_placed = _word("start_distance", 0,
        """uint8 (B,) in device memory: how each agent's last episode start went under the start rule — 0 none yet, 1 placed in the
        band, 2 clamped to the farthest tiles, 3 the drawn pose kept.""")

    # ---- the visit map (include/rcw.h, rcw_set_visit_map) --------------------------------
    def set_visit_map(self, sectors=1, table: bool = False) -> None:
        """Keep, on the device, how often each agent has stood in each cell — tile x heading sector (`sectors` of them, 1..8, at most
        `num_directions`) — this episode: `visit_map` (uint16, saturating), `visits_here` (the count of the cell the agent is on: the N of
        `beta / sqrt(N)`), `visited_cells`, `visit_first` (1 where the last step entered a cell for the first time this episode: the
        NovelD gate) and, with `table=True`, the uint32 table of the counts summed over the batch and per level of the layout source that
        is live NOW (`visit_table`, `level_visits_here`; the layout source cannot be changed while it is on).  A restart clears the
        agent's map; with no host in the loop.  `set_visit_map(None)` switches it off.  Switching it on (again) zeroes everything and
        counts every agent's cell once; the device arrays handed out before are invalid after every call."""
        self._drop("visit_map")
        if sectors is None or sectors is False:
            self._check(self._lib.rcw_set_visit_map(self._h, 0, 0, 0))
        else:
            self._check(self._lib.rcw_set_visit_map(self._h, 1, int(sectors), _capi.RCW_VISIT_TABLE if table else 0))

    @property
    def visit_map_info(self) -> dict:
        """`enabled`, `sectors`, `table`, and the table's level rows: `rows` of them, the first for level `first` (rcw_visit_map_info)."""
        v = [C.c_int32() for _ in range(5)]
        self._check(self._lib.rcw_visit_map_info(self._h, *[C.byref(x) for x in v]))
        return {"enabled": bool(v[0].value), "sectors": v[1].value, "table": bool(v[2].value & _capi.RCW_VISIT_TABLE), "rows": v[3].value, "first": v[4].value}

    visits_here = _word("visit_map", 0,
        """int32 (B,) in device memory: how often each agent has stood in the cell it is in, this call included (0: off the map).
        `beta * torch.rsqrt(env.visits_here.torch(sync=False).float().clamp(min=1))` is the count bonus.""")
    visited_cells = _word("visit_map", 1,
        """int32 (B,): the cells each agent has stood in this episode.""")
    visit_first = _word("visit_map", 2,
        """int32 (B,): 1 where the last call counted a cell the agent had not stood in this episode; 0 behind a restart.""")
    level_visits_here = _word("visit_map", 3,
        """uint32 (B,): the table's count of each agent's cell on its level (of the whole batch where it has no level row), every
        agent's adds of the call included; 0 without the table.""")
    visit_map = _tiles("visit_map",
        """uint16 (B, sectors, H, W), a host copy: `visit_map[b, s, i-1, j-1]` of tile (i, j) — indexed like `env.seen_map` per sector.""")
    visit_map_device = _tiles("visit_map",
        """The map where it lives: uint16 (B, sectors, W, H) in device memory — the tile map's own order, `[b, s, j-1, i-1]`.""", device=True)

    def visit_table(self, device: bool = False):
        """The counts summed since enabling (or the last `visit_table_clear`).  A dict: `total` uint32 (sectors, H, W) — every agent's
        counts —, `levels` (rows, sectors, H, W) — the same per level, level `first + k` at k —, and `first`.  `device=True`: the raw
        uint32 (1 + rows, sectors, W, H) `DeviceArray` instead, row 0 the total."""
        info = self.visit_map_info
        H, W, S, rows = self.cfg.height_tile_map_tu, self.cfg.width_tile_map_tu, info["sectors"], info["rows"]
        if device:
            p = C.c_void_p()
            self._check(self._lib.rcw_visit_table_device_ptr(self._h, C.byref(p)))
            return DeviceArray(p.value, (1 + rows, S, W, H), np.uint32, self, self._sync, host_getter=lambda: self._visit_table_host(rows, S))
        t = np.ascontiguousarray(self._visit_table_host(rows, S).transpose(0, 1, 3, 2))
        return {"total": t[0], "levels": t[1:], "first": info["first"]}

    def _visit_table_host(self, rows: int, sectors: int) -> np.ndarray:
        out = np.empty((1 + rows, sectors, self.cfg.width_tile_map_tu, self.cfg.height_tile_map_tu), dtype=np.uint32)
        self.host_syncs += 1
        self._check(self._lib.rcw_visit_table(self._h, _as_ptr(out)))
        return out

    def visit_table_clear(self) -> None:
        """Zero the table, stream-ordered and without waiting for the stream; the per-agent maps and words stay."""
        self._check(self._lib.rcw_visit_table_clear(self._h))

    # ---- the state archive (include/rcw.h, rcw_set_snapshots) ----------------------------
    def set_snapshots(self, rows: int) -> None:
        """Bind the state archive: `rows` agent records kept on the device, none filled, laid out for the features that are on NOW
        (enable the goal distance, the seen map, the learner view, the local map, the layout source and the statistics first: a save or
        restore after any of them changed is refused until the archive is bound again).  0 frees it."""
        self._check(self._lib.rcw_set_snapshots(self._h, int(rows)))

    @property
    def snapshot_info(self) -> dict:
        """`rows`, `row_bytes` (one record, as `snapshot_export` hands it out) and `shape_key` (rcw_snapshot_info)."""
        rows, row_bytes, key = C.c_int32(), C.c_uint64(), C.c_uint64()
        self._check(self._lib.rcw_snapshot_info(self._h, C.byref(rows), C.byref(row_bytes), C.byref(key)))
        return {"rows": rows.value, "row_bytes": row_bytes.value, "shape_key": key.value}

    def _snapshot_call(self, what: str, rows, mask) -> None:
        on_device = [x is not None and (isinstance(x, DeviceArray) or (_is_device_tensor(x) and x.is_cuda)) for x in (rows, mask)]
        if any(on_device):
            if not all(d or x is None for d, x in zip(on_device, (rows, mask))):
                raise ValueError(f"snapshot_{what}: rows and mask must both be on the device or both on the host")
            ptrs, tensors = [], []
            for x, itemsize, name in ((rows, 4, "rows: int32"), (mask, 1, "mask: uint8 or bool")):
                if x is None:
                    ptrs.append(None)
                    continue
                if isinstance(x, DeviceArray):
                    ok, ptr = x.dtype.itemsize == itemsize and x.shape == (self.batch,), x.ptr
                else:
                    ok, ptr = x.element_size() == itemsize and x.numel() == self.batch and x.is_contiguous() and not x.is_floating_point(), x.data_ptr()
                    tensors.append(x)
                if not ok:
                    raise ValueError(f"snapshot_{what}: device {name}, contiguous, of length batch")
                ptrs.append(C.c_void_p(ptr))
            cross = bool(tensors) and self._order_behind_torch()
            self._check(getattr(self._lib, f"rcw_snapshot_{what}_device")(self._h, *ptrs))
            if cross:
                self._release_after_use(*tensors)
            return
        r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        for x, name in ((r, "rows"), (m, "mask")):
            if x is not None and x.shape != (self.batch,):
                raise ValueError(f"snapshot_{what}: {name} must have length batch")
        self.host_syncs += 1
        self._check(getattr(self._lib, f"rcw_snapshot_{what}")(self._h, _as_ptr(r), _as_ptr(m)))

    def snapshot_save(self, rows=None, mask=None) -> None:
        """Save the records of the agents of `mask` (None: all) into the rows `rows` (int32 (B,); None: agent a into row a).  numpy
        arrays or None: checked on the host — a bad index or two agents into one row raise ValueError and change nothing —, and the call
        waits for the stream.  `DeviceArray`s or CUDA torch tensors: stream-ordered, no host wait; a bad index leaves that agent out and
        sets its status word and the error word (`sync()` raises, `clear_error()` clears), and of two agents into one row the higher wins."""
        self._snapshot_call("save", rows, mask)

    def snapshot_restore(self, rows=None, mask=None) -> None:
        """Put the agents of `mask` back as the rows `rows` hold them — several agents may take one row — and render them again.  The
        arguments as for `snapshot_save`; an unfilled row is a bad index."""
        self._snapshot_call("restore", rows, mask)

    @property
    def snapshot_filled(self) -> np.ndarray:
        """bool (rows,): which rows a save or an import has filled (waits for the stream)."""
        out = np.zeros(self.snapshot_info["rows"], dtype=np.uint8)
        self.host_syncs += 1
        self._check(self._lib.rcw_snapshot_filled(self._h, _as_ptr(out)))
        return out.astype(bool)

    def snapshot_export(self, first: int = 0, count: Optional[int] = None) -> dict:
        """Rows [first, first + count) on the host: `dict(shape_key, row_bytes, rows=uint8 (count, row_bytes))` — what
        `snapshot_import` of an environment of the same shape takes, in this process or a later one."""
        info = self.snapshot_info
        count = info["rows"] - first if count is None else int(count)
        out = np.zeros((max(count, 0), info["row_bytes"]), dtype=np.uint8)
        self.host_syncs += 1
        self._check(self._lib.rcw_snapshot_rows_copy(self._h, int(first), count, _as_ptr(out)))
        return {"shape_key": info["shape_key"], "row_bytes": info["row_bytes"], "rows": out}

    def snapshot_import(self, d: dict, first: int = 0) -> None:
        """Load `snapshot_export`'s rows into rows [first, ...) and count them as filled.  Another shape key is refused; so is a row whose
        goal, direction, position, map border or layout index a kernel could not index with (ValueError naming row and field).  Everything
        else in a row is trusted."""
        rows = np.ascontiguousarray(d["rows"], dtype=np.uint8)
        if rows.ndim != 2 or rows.shape[1] != self.snapshot_info["row_bytes"]:
            raise ValueError(f"snapshot_import: rows must be uint8 (count, {self.snapshot_info['row_bytes']})")
        self.host_syncs += 1
        self._check(self._lib.rcw_snapshot_rows_load(self._h, int(first), rows.shape[0], C.c_void_p(rows.ctypes.data), int(d["shape_key"])))

    # ---- the seen map (include/rcw.h, rcw_set_seen_map) ---------------------------------
    def set_seen_map(self, on: bool = True) -> None:
        """Keep, on the device, the tiles each agent's view rays have crossed since its episode began — exactly what the camera saw:
        every tile the march of each of the `num_rays` rays visits, from the player's tile through the stop tile.  `seen_map` holds 0 for
        an unseen tile and otherwise 1 free, 2 wall, 3 goal; `seen_count` counts the seen tiles, `seen_new` those the last step saw for
        the first time (a coverage bonus is `c * env.seen_new.torch(sync=False)`), `goal_seen` says whether the goal tile is among them.
        Follows resets, `set_state`, `set_walls` and `auto_reset` restarts with no host synchronisation.  Switching it on (again) starts
        every agent's map afresh from its current pose; the device arrays handed out before are invalid after every call."""
        self._drop("seen_map", "local_map")
        self._check(self._lib.rcw_set_seen_map(self._h, 1 if on else 0))

    @property
    def seen_map_enabled(self) -> bool:
        n = C.c_int32()
        self._check(self._lib.rcw_seen_map_enabled(self._h, C.byref(n)))
        return bool(n.value)

    seen_count = _word("seen_map", 0,
        """int32 (B,) in device memory: the tiles of each agent's map seen so far in its episode.  Rewritten behind every step, reset,
        `set_state` and `set_walls` in stream order.""")
    seen_new = _word("seen_map", 1,
        """int32 (B,): the tiles the last step saw for the first time; 0 for an agent the call restarted or reset.""")
    goal_seen = _word("seen_map", 2,
        """int32 (B,): 1 once the goal tile is among the seen tiles of the agent's episode, else 0.""")
    seen_map = _tiles("seen_map",
        """uint8 (B, H, W), a host copy: `seen_map[b, i-1, j-1]` is 0 while agent b has not seen tile (i, j) in its episode, else 1 free,
        2 wall, 3 goal (4: a goal `set_state` put into a wall) — indexed like `env.world.walls`.""")
    seen_map_device = _tiles("seen_map",
        """The map where it lives: uint8 (B, W, H) in device memory — the tile map's own order, `[b, j-1, i-1]`.""", device=True)

    # ---- the frontier (include/rcw.h, rcw_set_frontier) ----------------------------------
    def set_frontier(self, on: bool = True) -> None:
        """Keep, on the device, each agent's way to the nearest unseen tile: `frontier_field` (uint16: 0 on the unseen tiles next to a seen
        free one, on a seen free tile the moves to the nearest of them, 0xFFFF elsewhere), `frontier_distance` (the field at the agent's
        tile, -1: nothing left to explore from here), `frontier_tiles` (how many frontier tiles the agent's last flood found),
        `explore_action` (uint8 in 1..4, the guide's rule on this field: what `act_` takes as it stands) and `explore_heading` (-1: no
        advice).  An agent is flooded again only where its seen map changed or its episode began; with no host in the loop.  Explore, then
        go: `torch.where(env.goal_seen.torch(sync=False) > 0, env.guide_action.torch(sync=False), env.explore_action.torch(sync=False))`.
        Switching it on enables the seen map first where that is off; `set_seen_map(False)` is refused while it is on.  The device arrays
        handed out before are invalid after every call."""
        self._drop("frontier")
        if on and not self.seen_map_enabled:
            self.set_seen_map(True)
        self._check(self._lib.rcw_set_frontier(self._h, 1 if on else 0))

    @property
    def frontier_info(self) -> dict:
        """`enabled` (rcw_frontier_info)."""
        v = C.c_int32()
        self._check(self._lib.rcw_frontier_info(self._h, C.byref(v)))
        return {"enabled": bool(v.value)}

    @property
    def frontier_enabled(self) -> bool:
        return self.frontier_info["enabled"]

    frontier_distance = _word("frontier", 0,
        """int32 (B,) in device memory: the moves from each agent's tile to the nearest frontier tile through seen free tiles; -1 where
        there is none — everything the agent can reach has been seen — or the agent is off the map.""")
    frontier_tiles = _word("frontier", 1,
        """int32 (B,): the number of frontier tiles as of each agent's last flood.""")
    explore_action = _word("frontier", 2,
        """uint8 (B,): the action that leads each agent to its nearest frontier tile, always in 1..4.  `.torch(sync=False)` on the GPU —
        `act_` takes it as it is —, `np.asarray(...)` for a host copy.""")
    explore_heading = _word("frontier", 3,
        """int32 (B,): the 0-based direction index the frontier's rule wants each agent to face, -1 where it has no advice.""")
    frontier_field = _tiles("frontier_field",
        """uint16 (B, H, W), a host copy: `field[b, i-1, j-1]` of tile (i, j) — indexed like `env.seen_map`.""")
    frontier_field_device = _tiles("frontier_field",
        """The field where it lives: uint16 (B, W, H) in device memory — the tile map's own order, `[b, j-1, i-1]`.""", device=True)

    # ---- the local map (include/rcw.h, rcw_set_local_map) -------------------------------
    _LOCAL_SOURCES = {"world": _capi.RCW_LOCAL_WORLD, "seen": _capi.RCW_LOCAL_SEEN}
    _local_map_dev = None                                         # (the alias `local_map` caches on the object; `_drop` takes it away)

    def set_local_map(self, size, cells_per_tile: int = 1, source: str = "world") -> None:
        """Keep, on the device, an agent-centred, heading-up crop of each agent's map: `local_map` is uint8 (B, size, size), the agent
        at the centre, row 0 the farthest ahead, column 0 on the side of ray 0 (rotate_minus_90 of the heading), `cells_per_tile` cells to a tile.
        `source="world"` shows the tile map as it is now, `source="seen"` the agent's seen map (`set_seen_map()` first): 0 outside the
        map (or not seen), 1 free, 2 wall, 3 goal.  Computed from the engine's own position, heading and direction table behind every
        step, reset, `set_state`, `set_walls` and `set_direction_table`, with no host synchronisation.  `size=0` or `None` switches it
        off; the device array handed out before is invalid after every call."""
        self._drop("local_map")
        if not size:
            self._check(self._lib.rcw_set_local_map(self._h, 0, 0, 0))
            return
        if source not in self._LOCAL_SOURCES:
            raise ValueError(f"source must be one of {sorted(self._LOCAL_SOURCES)} (got {source!r})")
        self._check(self._lib.rcw_set_local_map(self._h, self._LOCAL_SOURCES[source], int(size), int(cells_per_tile)))

    @property
    def local_map_info(self) -> dict:
        """The local map's settings (rcw_local_map_info): `source` (None while it is off), `size`, `cells_per_tile`."""
        v = [C.c_int32() for _ in range(3)]
        self._check(self._lib.rcw_local_map_info(self._h, *[C.byref(x) for x in v]))
        src, size, cpt = (x.value for x in v)
        return {"source": {value: name for name, value in self._LOCAL_SOURCES.items()}.get(src), "size": size, "cells_per_tile": cpt}

    def local_map_host(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """Agents [first, first + count) of the local map, uint8 (count, size, size), copied to the host (waits for the engine's stream)."""
        n = self.batch - first if count is None else count
        S = self.local_map_info["size"]
        out = np.empty((max(n, 0), S, S), dtype=np.uint8)
        self.host_syncs += 1
        self._check(self._lib.rcw_local_map_copy(self._h, _as_ptr(out), first, n))
        return out

    @property
    def local_map(self) -> DeviceArray:
        """The local map batch, aliased device memory: uint8 (B, size, size), rewritten in place behind every step in stream order
        (`.torch(sync=False)` for a policy on the GPU; `np.asarray(env.local_map)` copies it to the host)."""
        if self._local_map_dev is None:
            p = C.c_void_p()
            self._check(self._lib.rcw_local_map_device_ptr(self._h, C.byref(p)))
            S = self.local_map_info["size"]
            self._local_map_dev = DeviceArray(p.value, (self.batch, S, S), np.uint8, self, self._sync, host_getter=lambda: self.local_map_host())
        return self._local_map_dev

    # ---- wall layouts (include/rcw.h, rcw_set_walls) ----------------------------------
    def set_walls(self, walls, index=None, mask=None) -> None:
        """Interior walls: `walls` is bool / uint8 (H, W) — one layout for every agent — or (M, H, W) with `index` int (B,)
        naming each agent's layout (None: M == 1, or M == B and agent a takes layout a); `walls[m, i-1, j-1]` is tile (i, j),
        the index order of `env.world.tile_map[b, 0]`.  `mask`: the agents the call touches (None: all).  The wall ring must
        be there and two interior tiles free (ValueError otherwise, the environment untouched); `layouts` has generators.
        The touched agents are reset against the new walls — on the device with the environment's seed, or, for an
        environment built with `rng`, from that generator on the host (`reference_reset_draws(..., walls=...)`) —, and
        the walls stay through every later reset, set_state and auto_reset restart until the next call.  Reachability is
        not checked (`layouts.is_connected`); `set_state` does not know the walls."""
        H, W, B = self.cfg.height_tile_map_tu, self.cfg.width_tile_map_tu, self.batch
        w = np.asarray(walls)
        if w.ndim == 2:
            w = w[None]
        if w.ndim != 3 or w.shape[1:] != (H, W):
            raise ValueError(f"walls must be (H, W) = ({H}, {W}) or (M, {H}, {W}), got {np.asarray(walls).shape}")
        w = w != 0
        M = w.shape[0]
        # tile (i, j) of layout m at m H W + (i - 1) + H (j - 1): (M, W, H) in C order
        flat = np.ascontiguousarray(w.transpose(0, 2, 1), dtype=np.uint8)
        ix = None if index is None else np.ascontiguousarray(index, dtype=np.int32).reshape(B)
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8).reshape(B)
        self._check(self._lib.rcw_set_walls(self._h, _as_ptr(flat), M, _as_ptr(ix), _as_ptr(m)))
        if self.rng is not None:
            took = ix if ix is not None else (np.zeros(B, dtype=np.int32) if M == 1 else np.arange(B, dtype=np.int32))
            if self._rng_walls is None:
                self._rng_walls = np.zeros((B, H, W), dtype=bool)
                self._rng_walls[:, [0, -1], :] = True
                self._rng_walls[:, :, [0, -1]] = True
            touched = np.ones(B, dtype=bool) if m is None else m != 0
            self._rng_walls[touched] = w[took[touched]]
            _reset_from_rng(self, self.rng, m)

    # ---- what the setters of the layout sources (bank, generator, caves, rooms) check alike ----
    def _refuse_rng(self, what: str) -> None:
        if self.rng is not None:
            raise ValueError(f"an environment built with rng draws its resets on the host: it takes no {what}")

    @staticmethod
    def _check_family_integers(own: Optional[str] = None, **values) -> None:
        """The integer arguments of a generator family, in the caller's order: `level_seed` a UInt64, the others 0 .. 2^31 - 1 — but for
        `own`, the family's own Int32, whose negative values go on to the library's refusal."""
        for name, v in values.items():
            top = 2 ** 64 - 1 if name == "level_seed" else 2 ** 31 - 1
            if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not (-2 ** 31 if name == own else 0) <= int(v) <= top:
                raise ValueError(f"{name} must be an integer in 0 .. {top}, got {v!r}")

    def _set_wall_family(self, what: str, call, params, own: Optional[str], levels, first_level, level_seed) -> None:
        """What the setters of the generator's families share.  `call` is the family's export; `params` its own parameters in the
        export's order as (name, value, is a probability); `own` is `_check_family_integers`'.  The first value None: the family off."""
        self._drop("wall_layout")
        if params[0][1] is None:
            self._check(call(self._h, 0, *[0] * (len(params) + 3)))
            return
        self._refuse_rng(what)
        from . import layouts as _layouts

        words = {name: _layouts.loops_word(v) for name, v, probability in params if probability}
        self._check_family_integers(own, **{name: v for name, v, probability in params if not probability},
                                    levels=levels, first_level=first_level, level_seed=level_seed)
        self._check(call(self._h, 1, *[words[name] if probability else int(v) for name, v, probability in params],
                         int(levels), int(first_level), int(level_seed)))

    # ---- the wall bank (include/rcw.h, rcw_set_wall_bank) -------------------------------
    def set_wall_bank(self, walls, weights=None) -> None:
        """A bank of wall layouts on the device, one drawn for an agent at every start of an episode — `reset_`, a done or truncated
        restart under `auto_reset`, and this call, which restarts every agent (episode counters + 1).  `walls` is bool / uint8
        (M, H, W) (or (H, W): a bank of one), each layout checked as `set_walls` checks one (ValueError otherwise, the environment
        untouched); `weights` is M non-negative integers whose sum lies in 1 .. 2^32 - 1 (None: uniform): layout k is drawn with
        probability weights[k] / sum, as a pure function of (seed, global agent id, episode, bank) — sharding, the step form and the
        agent's previous walls play no part.  No host synchronisation per step; `wall_layout` says which layout each agent has,
        `env.world.walls` reads the walls back.  `walls=None` switches the bank off: the agents keep the walls they have and
        `set_walls` works again.  An environment built with `rng` draws its resets on the host and takes no bank."""
        if walls is None:
            self._drop("wall_layout")
            self._check(self._lib.rcw_set_wall_bank(self._h, None, 0, None))
            return
        self._refuse_rng("wall bank")
        H, W = self.cfg.height_tile_map_tu, self.cfg.width_tile_map_tu
        w = np.asarray(walls)
        if w.ndim == 2:
            w = w[None]
        if w.ndim != 3 or w.shape[1:] != (H, W) or w.shape[0] < 1:
            raise ValueError(f"wall bank must be (M, H, W) = (M, {H}, {W}) with M >= 1, got {np.asarray(walls).shape}")
        flat = np.ascontiguousarray((w != 0).transpose(0, 2, 1), dtype=np.uint8)   # tile (i, j) of layout m at m H W + (i - 1) + H (j - 1)
        wt = self._wall_bank_weights(weights, w.shape[0])
        self._drop("wall_layout")
        self._check(self._lib.rcw_set_wall_bank(self._h, _as_ptr(flat), w.shape[0], _as_ptr(wt)))

    @staticmethod
    def _wall_bank_weights(weights, layouts: int):
        if weights is None:
            return None
        wt = np.asarray(weights)
        if wt.shape != (layouts,) or not np.issubdtype(wt.dtype, np.integer) or (wt < 0).any() or (wt > 0xFFFFFFFF).any():
            raise ValueError(f"wall bank weights must be {layouts} integers in 0 .. 2^32 - 1")
        return np.ascontiguousarray(wt, dtype=np.uint32)

    def set_wall_bank_weights(self, weights) -> None:
        """New weights for the installed bank (None: uniform), in stream order and without waiting for the device: they hold from each
        agent's next episode start, no agent is touched — what a prioritised-replay caller calls every few updates."""
        wt = self._wall_bank_weights(weights, self.wall_bank_info["layouts"])
        self._check(self._lib.rcw_set_wall_bank_weights(self._h, _as_ptr(wt)))

    @property
    def wall_bank_info(self) -> dict:
        """`layouts` and `total_weight` of the bank (rcw_wall_bank_info); zeros while it is off."""
        n, t = C.c_int32(), C.c_uint64()
        self._check(self._lib.rcw_wall_bank_info(self._h, C.byref(n), C.byref(t)))
        return {"layouts": n.value, "total_weight": t.value}

    # ---- the wall generator (include/rcw.h, rcw_set_wall_generator) ---------------------
    def set_wall_generator(self, loops=0.0, levels: int = 0, first_level: int = 0, level_seed: int = 0) -> None:
        """A new maze made on the device at every start of an episode — `reset_`, a done or truncated restart under `auto_reset`, and
        this call, which restarts every agent (episode counters + 1).  The maze is the minimum spanning tree of the odd sub-grid
        (`layouts.maze`'s cells) under an order drawn from one 64-bit key, plus the non-tree edges `loops` opens — a probability in
        [0, 1], scaled to UInt32 with min(int(p * 2^32), 2^32 - 1); 0 is a perfect maze.  `levels == 0`: the key is the episode's own,
        every episode a maze of its own, `wall_layout` reads -1.  `levels >= 1`: the episode picks level
        first_level + (0 .. levels - 1) and the maze is a function of (level_seed, level, H, W, loops) alone — a seeded range to train
        on and a held-out one to evaluate on; `wall_layout` says which.  `layouts.generated_maze(*layouts.generated_maze_key(...))`
        replays any of them on the host.  Maps of 5 x 5 to 129 x 129 (4096 cells).  `set_walls` and `set_wall_bank` are refused while
        the generator is on; `set_wall_generator(None)` switches it off, the agents keep their walls.  An environment built with
        `rng` draws its resets on the host and takes no generator."""
        self._set_wall_family("wall generator", self._lib.rcw_set_wall_generator, (("loops", loops, True),), None, levels, first_level, level_seed)

    @property
    def wall_generator_info(self) -> dict:
        """`enabled`, `loops` (the UInt32 word), `levels`, `first_level` and `level_seed` of the generator (rcw_wall_generator_info);
        zeros while it is off."""
        on, loops, levels, first, seed = C.c_int32(), C.c_uint32(), C.c_int32(), C.c_int32(), C.c_uint64()
        self._check(self._lib.rcw_wall_generator_info(self._h, C.byref(on), C.byref(loops), C.byref(levels), C.byref(first), C.byref(seed)))
        return {"enabled": bool(on.value), "loops": loops.value, "levels": levels.value, "first_level": first.value, "level_seed": seed.value}

    # ---- the wall generator: caves (include/rcw.h, rcw_set_wall_caves) ------------------
    def set_wall_caves(self, fill=0.40, smooth: int = 2, levels: int = 0, first_level: int = 0, level_seed: int = 0) -> None:
        """A new cave made on the device at every start of an episode, where `set_wall_generator` makes a maze: a random fill of the
        interior (`fill`: the probability of a wall, or the UInt32 word itself as `loops` takes one), smoothed `smooth` times (0 .. 8)
        by the 5-of-9 automaton, pruned to its largest 4-connected region.  A cave whose region has fewer than
        max(7, (H-2)(W-2) // 4) tiles is replaced by the perfect maze of the same key — on small maps that is most of them (nearly
        all at 5 x 7, about a quarter at 8 x 8, none at 32 x 32 at the defaults).  `levels`, `first_level`, `level_seed` and
        `wall_layout` are the generator's; `layouts.generated_cave(layouts.generated_maze_key(...)[0], H, W, fill, smooth)` replays
        any of them on the host.  Maps of 5 x 5 up to 4096 interior tiles (66 x 66).  `set_walls`, `set_wall_bank` and
        `set_wall_generator` are refused while caves are on, and caves while a bank or the generator is; `set_wall_caves(None)`
        switches them off, the agents keep their walls.  An environment built with `rng` draws its resets on the host and takes
        no caves."""
        self._set_wall_family("wall caves", self._lib.rcw_set_wall_caves, (("fill", fill, True), ("smooth", smooth, False)), "smooth",
                              levels, first_level, level_seed)

    @property
    def wall_caves_info(self) -> dict:
        """`enabled`, `fill` (the UInt32 word) and `smooth` of the caves (rcw_wall_caves_info); zeros while they are off.  The level
        parameters read from `wall_generator_info`, which reports `enabled` and `loops == 0` while caves are on."""
        on, fill, smooth = C.c_int32(), C.c_uint32(), C.c_int32()
        self._check(self._lib.rcw_wall_caves_info(self._h, C.byref(on), C.byref(fill), C.byref(smooth)))
        return {"enabled": bool(on.value), "fill": fill.value, "smooth": smooth.value}

    # ---- the wall generator: rooms (include/rcw.h, rcw_set_wall_rooms) ------------------
    def set_wall_rooms(self, room=2, stop=0.25, doors=0.25, levels: int = 0, first_level: int = 0, level_seed: int = 0) -> None:
        """New rooms made on the device at every start of an episode, where `set_wall_generator` makes a maze: rectangular rooms of
        different sizes joined by doorways, `layouts.four_rooms`' topology.  The interior is split recursively by walls on even
        lines; every wall has a door and, with probability `doors`, a second one; a chamber other than the whole interior is left a
        room with probability `stop`; no room side falls below `room` (>= 1).  `stop` and `doors` are probabilities, or the UInt32
        words themselves as `loops` takes one.  Connected by construction on every map from 5 x 5: no fallback.  `levels`,
        `first_level`, `level_seed` and `wall_layout` are the generator's;
        `layouts.generated_rooms(layouts.generated_maze_key(...)[0], H, W, room, stop, doors)` replays any of them on the host.  Maps
        of 5 x 5 up to ceil((H-2)/2) ceil((W-2)/2) = 4096 (130 x 130, 5 x 4097).  `set_walls`, `set_wall_bank`, `set_wall_generator`
        and `set_wall_caves` are refused while rooms are on, and rooms while any of them is; `set_wall_rooms(None)` switches them
        off, the agents keep their walls.  An environment built with `rng` draws its resets on the host and takes no rooms."""
        self._set_wall_family("wall rooms", self._lib.rcw_set_wall_rooms, (("room", room, False), ("stop", stop, True), ("doors", doors, True)), "room",
                              levels, first_level, level_seed)

    @property
    def wall_rooms_info(self) -> dict:
        """`enabled`, `room`, `stop` and `doors` (the UInt32 words) of the rooms (rcw_wall_rooms_info); zeros while they are off.  The
        level parameters read from `wall_generator_info`, which reports `enabled` and `loops == 0` while rooms are on."""
        on, room, stop, doors = C.c_int32(), C.c_int32(), C.c_uint32(), C.c_uint32()
        self._check(self._lib.rcw_wall_rooms_info(self._h, C.byref(on), C.byref(room), C.byref(stop), C.byref(doors)))
        return {"enabled": bool(on.value), "room": room.value, "stop": stop.value, "doors": doors.value}

    wall_layout = _word("wall_layout", 0,
        """int32 (B,) in device memory: the bank layout each agent's current episode was given — with the wall generator its level, or
        -1 — (`.torch(sync=False)` on the GPU, `np.asarray(env.wall_layout)` for a host copy).  Valid until the next `set_wall_bank`
        , `set_wall_generator`, `set_wall_caves` or `set_wall_rooms`.""")

    def ray_table(self) -> np.ndarray:
        """(nd, 5, N) float32: per heading [dx | dy | |1/dx| | |1/dy| | dir·ray]."""
        out = np.empty((self.cfg.num_directions, 5, self.cfg.num_rays), dtype=self.T)
        fn = self._lib.rcw_ray_table64 if self.T is np.float64 else self._lib.rcw_ray_table
        self._check(fn(self._h, _as_ptr(out)))
        return out

    def device_name(self) -> str:
        buf = C.create_string_buffer(256)
        self._check(self._lib.rcw_device_name(self._h, buf, 256))
        return buf.value.decode()

    # ---- state injection (how "identical seeds" is realised) ---------
    def set_state(self, goal_position, player_position_wu, player_direction_au, mask=None):
        g = np.ascontiguousarray(goal_position, dtype=np.int32).reshape(self.batch, 2)
        p = np.ascontiguousarray(player_position_wu, dtype=self.T).reshape(self.batch, 2)
        d = np.ascontiguousarray(player_direction_au, dtype=np.int32).reshape(self.batch)
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8).reshape(self.batch)
        fn = self._lib.rcw_set_state64 if self.T is np.float64 else self._lib.rcw_set_state
        self._check(fn(self._h, _as_ptr(g), _as_ptr(p), _as_ptr(d), _as_ptr(m)))

    def set_direction_table(self, directions_wu):
        d = np.ascontiguousarray(directions_wu, dtype=self.T).reshape(self.cfg.num_directions, 2)
        fn = self._lib.rcw_set_direction_table64 if self.T is np.float64 else self._lib.rcw_set_direction_table
        self._check(fn(self._h, _as_ptr(d)))

    def stream_ptr(self) -> int:
        """The hipStream_t (as an int) the engine's work is ordered on."""
        p = C.c_void_p()
        self._check(self._lib.rcw_get_stream(self._h, C.byref(p)))
        return int(p.value or 0)

    def _stream_is_torch_owned(self) -> bool:
        ts = getattr(self, "_torch_owned_stream", None)
        return ts is not None and ts.cuda_stream == self.stream_ptr()

    def torch_stream(self):
        """The engine's stream as a torch stream object (for wait_stream / wait_event / record_stream): the torch Stream
        itself where torch owns it, else ONE `ExternalStream` wrapper per raw stream, kept for the engine's lifetime."""
        import torch

        if self._stream_is_torch_owned():
            return self._torch_owned_stream
        ptr = self.stream_ptr()
        cached = getattr(self, "_torch_stream", None)
        if cached is None or cached[0] != ptr:
            cached = self._torch_stream = (ptr, torch.cuda.ExternalStream(ptr, device=f"cuda:{self.device}"))
        return cached[1]

    def set_stream(self, stream):
        """Order the engine's work on another stream: a `torch.cuda.Stream` (kept alive here; torch never destroys its
        streams, so tensors may be handed over with record_stream); a `torch.cuda.ExternalStream` or a raw hipStream_t as
        an int — a stream the CALLER owns and keeps alive for as long as the engine, and any tensor it was given, lives
        (tensors are then held by reference until the engine has used them, never `record_stream`ed: torch would record
        an event on that stream whenever the tensor is finally freed, possibly after the caller destroyed it); or None:
        the library's own stream."""
        self._torch_owned_stream = None
        if stream is not None and hasattr(stream, "cuda_stream"):
            if _torch_owns(stream):
                self._torch_owned_stream = stream
            stream = stream.cuda_stream
        self._check(self._lib.rcw_set_stream(self._h, C.c_void_p(stream) if stream else None))

    def bind_obs(self, device_ptr: Optional[int]):
        self._check(self._lib.rcw_bind_obs(self._h, C.c_void_p(device_ptr) if device_ptr else None))

    def clear_error(self):
        self._check(self._lib.rcw_clear_error(self._h))

    def profile(self, enable: bool):
        """Bracket the cast and fill kernels of every step with HIP events (<= 256 steps)."""
        self._check(self._lib.rcw_profile(self._h, 1 if enable else 0))

    def profile_read(self):
        """(mean cast kernel ms, mean top view kernel ms (0 without it), mean fill kernel ms, steps recorded).
        With the two-kernel top view the second is its store kernel; its draw kernel runs beside the fill."""
        c, t, f, n = C.c_float(), C.c_float(), C.c_float(), C.c_int32()
        self._check(self._lib.rcw_profile_read(self._h, C.byref(c), C.byref(t), C.byref(f), C.byref(n)))
        return float(c.value), float(t.value), float(f.value), int(n.value)

    def set_top_view_form(self, form: Optional[str] = None, runs: int = 0) -> None:
        """Choose the form update_top_view! takes instead of the library's rule (rcw_set_top_view_form): None = automatic,
        "in-place", "one-kernel" or "two-kernels"; `runs` = 0 (automatic) or 1..8 runs of agents for the two-kernel form.
        All forms write the same pixels.  Raises RcwError (unsupported) when the geometry cannot take the form."""
        forms = {None: 0, "auto": 0, "in-place": _capi.RCW_TOP_VIEW_IN_PLACE, "one-kernel": _capi.RCW_TOP_VIEW_ONE_KERNEL,
                 "two-kernels": _capi.RCW_TOP_VIEW_TWO_KERNELS}
        if form not in forms:
            raise ValueError(f"unknown top view form {form!r}")
        self._check(self._lib.rcw_set_top_view_form(self._h, forms[form], int(runs)))

    def step_form(self) -> str:
        """How many launches a step of this handle takes (rcw_step_form): "two-launches" (cast kernel, then fill kernel) or
        "one-launch" (the fill picks each frame among the successors the previous launch cast: rcw_fill256_cast_kernel)."""
        f = C.c_int32()
        self._check(self._lib.rcw_step_form(self._h, C.byref(f)))
        return {_capi.RCW_STEP_TWO_LAUNCHES: "two-launches", _capi.RCW_STEP_ONE_LAUNCH: "one-launch"}[f.value]

    def set_step_form(self, form: Optional[str] = None) -> None:
        """Choose the step's form instead of the library's rule (rcw_set_step_form): None = automatic, "two-launches" or
        "one-launch".  Both leave the same state and the same pixels.  Raises RcwError (unsupported) when the geometry cannot
        take the one-launch form (a 256-row camera view without a top view)."""
        forms = {None: 0, "auto": 0, "two-launches": _capi.RCW_STEP_TWO_LAUNCHES, "one-launch": _capi.RCW_STEP_ONE_LAUNCH}
        if form not in forms:
            raise ValueError(f"unknown step form {form!r}")
        self._check(self._lib.rcw_set_step_form(self._h, forms[form]))

    def fill_kernel_name(self) -> str:
        """The kernel update_camera_view! takes for this camera height (rcw_fill_kernel_name)."""
        buf = C.create_string_buffer(64)
        self._check(self._lib.rcw_fill_kernel_name(self._h, buf, 64))
        return buf.value.decode()

    def top_view_form(self) -> str:
        """Which kernel form update_top_view! takes for this geometry: "none", "in-place", "one-kernel", "two-kernels"."""
        f = C.c_int32()
        self._check(self._lib.rcw_top_view_form(self._h, C.byref(f)))
        return ("none", "in-place", "one-kernel", "two-kernels")[f.value]

    def update_top_view_form(self) -> str:
        """The form `update_top_view_(env)` takes when called alone, outside a step (rcw_update_top_view_form)."""
        f = C.c_int32()
        self._check(self._lib.rcw_update_top_view_form(self._h, C.byref(f)))
        return ("none", "in-place", "one-kernel", "two-kernels")[f.value]

    def timer_start(self):
        self._check(self._lib.rcw_timer_start(self._h))

    def timer_stop(self) -> float:
        ms = C.c_float()
        self._check(self._lib.rcw_timer_stop(self._h, C.byref(ms)))
        return float(ms.value)


# ---- the generic functions of RayCastWorlds.jl:7-14 that are on the path ------------------
def reference_reset_draws(rng, H: int, W: int, nd: int, old_goal=None, walls=None):
    """The random draws of ONE `reset!(world)` (SR:110-137) from `rng` (a `numpy.random.Generator`: `integers(lo, hi)`,
    `hi` exclusive), in the reference's order and number:

        rand(rng, 2:H-1), rand(rng, 2:W-1)                     the goal tile                      SR:120
        rand(rng, CartesianIndices((1:H, 1:W)))                the player's tile; drawn AGAIN while the tile is occupied
                                                               (wall ring or the new goal), at most 1024 H W times  UT:23-37
        rand(rng, 0:nd-1)                                      the heading                        SR:128

    A position is ONE draw of a linear index into the column-major region (i = lin mod H + 1, j = lin div H + 1), as
    `rand(rng, ::AbstractArray)` indexes its argument with one `rand(rng, 1:length)`.  Returns (goal_i, goal_j, tile_i,
    tile_j, heading), tiles 1-based.  `old_goal` is not needed: reset! clears the old goal bit before it draws (SR:118).

    `walls` (bool (H, W), `walls[i-1, j-1]`; None: the wall ring alone, the reference's map) — this build's interior walls
    (`SingleRoom.set_walls`): the goal pair is drawn AGAIN while its tile is a wall, at most 1024 H W times (then the last pair
    stays), and the player's tile is occupied where `walls` says so.  On the ring alone no interior tile is a wall: the same
    draws, in number and value."""
    gi = int(rng.integers(2, H))                     # 2 : H - 1
    gj = int(rng.integers(2, W))
    if walls is not None:
        walls = np.asarray(walls) != 0
        if walls.shape != (H, W):
            raise ValueError(f"walls must be (H, W) = ({H}, {W}), got {walls.shape}")
        for _ in range(1024 * H * W):
            if not walls[gi - 1, gj - 1]:
                break
            gi = int(rng.integers(2, H))
            gj = int(rng.integers(2, W))

    def occupied(lin):
        i, j = lin % H + 1, lin // H + 1
        if walls is not None:
            return bool(walls[i - 1, j - 1]) or (i == gi and j == gj)
        return i == 1 or i == H or j == 1 or j == W or (i == gi and j == gj)      # any(@view tile_map[:, position]) UT:27

    lin = int(rng.integers(0, H * W))                # UT:24
    for _ in range(1024 * H * W):                    # UT:26
        if occupied(lin):
            lin = int(rng.integers(0, H * W))        # UT:28
        else:
            break
    else:                                            # UT:34 (@warn, then the occupied tile is returned)
        import warnings

        warnings.warn(f"Could not sample an empty position in max_tries = {1024 * H * W}. "
                      f"Returning non-empty position: ({lin % H + 1}, {lin // H + 1})", RuntimeWarning, stacklevel=2)
    d = int(rng.integers(0, nd))                     # 0 : nd - 1
    return gi, gj, lin % H + 1, lin // H + 1, d


def _reset_from_rng(env: "SingleRoom", rng, mask, construction: bool = False, first: int = 0, global_batch: Optional[int] = None) -> None:
    """reset!(world) for every (unmasked) agent with the caller's generator(s): agent after agent from ONE generator —
    B reference worlds sharing an rng, reset in order — or agent a from `rng[a]` — each agent the reference world built
    with that rng.  The state goes to the engine with one rcw_set_state (tile_map goal bit, pose, heading, reward 0,
    done false, rays cast, views rendered: SR:118-134, SR:328-329).

    `first` / `global_batch` (ShardedSingleRoom): this engine holds the global agents [first, first + batch) of `global_batch`;
    `rng` and `mask` are then the GLOBAL ones — one generator is advanced through every unmasked global agent's draws and this
    shard keeps its own, so that the states do not depend on the sharding (every rank passes generators in the same state)."""
    H, W, nd, B = env.cfg.height_tile_map_tu, env.cfg.width_tile_map_tu, env.cfg.num_directions, env.batch
    G = B if global_batch is None else int(global_batch)
    per_agent = not hasattr(rng, "integers")
    if per_agent and len(rng) != G:
        raise ValueError(f"expected one generator or {G} of them, got {len(rng)}")
    gm = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8).reshape(G)
    goal = np.ones((B, 2), dtype=np.int32)
    pos = np.ones((B, 2), dtype=env.T)
    head = np.zeros(B, dtype=np.int32)
    for ga in (range(first, first + B) if per_agent else range(G)):          # (one generator: the other shards' draws are made and dropped)
        if gm is not None and not gm[ga]:
            continue
        g = rng[ga] if per_agent else rng
        a = ga - first
        layouts = getattr(env, "_rng_walls", None)   # (set_walls on an rng environment: each LOCAL agent's layout; the other shards' agents draw as the caller's global layouts say)
        gw = getattr(env, "_rng_walls_global", None)
        w = gw[ga] if gw is not None else (layouts[a] if layouts is not None and 0 <= a < B else None)
        if construction:
            reference_reset_draws(g, H, W, nd)       # SR:62-74: drawn, then overwritten by reset!(world) SR:105
        gi, gj, ti, tj, d = reference_reset_draws(g, H, W, nd, walls=w)
        if 0 <= a < B:
            goal[a] = (gi, gj)
            pos[a] = (env.T(ti - 0.5), env.T(tj - 0.5))  # convert(T, tile - 0.5) SR:125
            head[a] = d
    # masked-out agents keep their state: rcw_set_state skips them, the placeholders above are never read
    env.set_state(goal, pos, head, mask=None if gm is None else gm[first:first + B])


def reset_(env: SingleRoom, mask=None, seed: Optional[int] = None, rng=None) -> None:
    """`RCW.reset!(env)` SR:326-331 — all agents, or those with a non-zero `mask` byte.

    Default: sampled on the device by the engine's counter-based generator keyed (seed, global agent id, episode).
    `rng` (or an environment constructed with one, SR:49): the reference's own keyword — the draws come from the caller's
    generator on the host, in the reference's order (`reference_reset_draws`)."""
    if rng is None and seed is None:
        rng = getattr(env, "rng", None)
    if rng is not None:
        if env.wall_bank_info["layouts"]:
            raise ValueError("the environment draws its walls from a wall bank on the device: reset it with a seed, not an rng")
        if env.wall_generator_info["enabled"]:
            raise ValueError("the environment makes its walls with the wall generator on the device: reset it with a seed, not an rng")
        _reset_from_rng(env, rng, mask)
        return None
    if seed is not None:
        env.seed = int(seed)
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8).reshape(env.batch)
    env._check(env._lib.rcw_reset(env._h, _as_ptr(m), env.seed))
    return None


def host_actions(batch: int, action) -> np.ndarray:
    """Normalise host-side actions to a contiguous uint8 (batch,) array; anything outside 1..4
    raises AssertionError like `@assert action in Base.OneTo(NUM_ACTIONS)` (SR:140)."""
    if np.isscalar(action):
        a = np.full(batch, action)
    else:
        a = np.asarray(action).reshape(-1)
        if a.size != batch:
            raise ValueError(f"expected {batch} actions, got {a.size}")
        if a.dtype == np.uint8 and a.flags.c_contiguous and a.size:          # the common case: two reductions, no temporaries
            if a.min() >= 1 and a.max() <= NUM_ACTIONS:
                return a
    ok = (a >= 1) & (a <= NUM_ACTIONS)
    if a.dtype.kind == "f":
        ok &= a == np.floor(a)
    if not np.all(ok):
        raise AssertionError(f"Invalid action: {a[~ok][0]}")
    return np.ascontiguousarray(a.astype(np.uint8, copy=False))


def unpack_tile_map(chunks: np.ndarray, H: int, W: int) -> np.ndarray:
    """BitArray{3}(2, H, W).chunks per agent (uint64 (B, nchunks)) -> bool (B, 2, H, W) with
    tile_map[b, o-1, i-1, j-1] == Julia tile_map[o, i, j]; bit index (o-1) + 2(i-1) + 2H(j-1)."""
    chunks = np.ascontiguousarray(chunks, dtype=np.uint64)
    bits = np.unpackbits(chunks.view(np.uint8), axis=1, bitorder="little")[:, : 2 * H * W]
    return bits.reshape(chunks.shape[0], W, H, 2).transpose(0, 3, 2, 1).astype(bool)


def _is_device_tensor(x) -> bool:
    return hasattr(x, "is_cuda") and hasattr(x, "data_ptr")


def act_(env: SingleRoom, action) -> None:
    """`RCW.act!(env, action)` SR:333-340 (without the top view) for every agent.

    `action`: one int in 1..4 applied to all agents, a length-B sequence / numpy array, or
    a CUDA uint8 torch tensor of length B (stays on the device).  Anything outside 1..4
    raises AssertionError and steps no agent (`@assert` SR:140).
    """
    if _is_device_tensor(action):
        if not action.is_cuda:
            action = action.numpy()
        else:
            import torch

            if action.dtype != torch.uint8 or action.numel() != env.batch or not action.is_contiguous():
                raise ValueError("device actions must be a contiguous uint8 tensor of length batch")
            # The actions were produced on torch's current stream; unless the engine runs on that very
            # stream, make the engine's stream wait for them (an event record + wait, no host sync) and
            # hold the tensor until the cast kernel has read it (the caller may drop a temporary at once).
            cross = env._order_behind_torch()
            env._check(env._lib.rcw_step_device(env._h, C.c_void_p(action.data_ptr())))
            if cross:
                env._release_after_use(action)
            return None
    if isinstance(action, (int, np.integer)) and not isinstance(action, bool):
        # one action for every agent (what the reference's own loop passes: env(rand(1:4)), test/runtests.jl:28): a
        # device-resident constant per action, made once — no staging copy, no array to validate
        if not 1 <= int(action) <= NUM_ACTIONS:
            raise AssertionError(f"Invalid action: {action}")
        buf = env._constant_actions(int(action))
        if buf is not None:
            env._check(env._lib.rcw_step_device(env._h, C.c_void_p(buf.data_ptr())))
            return None
    a = host_actions(env.batch, action)
    env._check(env._lib.rcw_step(env._h, _as_ptr(a)))
    return None


def cast_rays_(env: SingleRoom, first: int = 0, count: Optional[int] = None):
    """`RCW.cast_rays!(world)` SR:195-231: recasts every agent's rays from the current state (rcw_cast_rays:
    the compact column descriptors are refreshed, no pixel is written) and returns the ray buffers
    (stop tile, hit dimension, distance, direction) of agents [first, first+count)."""
    env._check(env._lib.rcw_cast_rays(env._h))
    return env.world.rays(first, count)


def update_camera_view_(env: SingleRoom) -> None:
    """`RCW.update_camera_view!(env)` SR:374-444: refills `camera_view` from the stored ray results without
    casting, as the reference's does (rcw_update_camera_view: the fill kernel alone)."""
    env._check(env._lib.rcw_update_camera_view(env._h))


def update_top_view_(env: SingleRoom) -> None:
    """`RCW.update_top_view!(env)` SR:446-483 (env built with render_top_view=True): redraws `top_view`."""
    env._check(env._lib.rcw_update_top_view(env._h))


def get_action_keys(env: SingleRoom):
    """`RCW.get_action_keys(env)` SR:485: the keys of actions 1..4 — MiniFB's KB_KEY_W / S / A / D there, their letters here
    (what `viewer.play_keys` takes)."""
    return ("w", "s", "a", "d")


def get_action_names(env: SingleRoom):
    """`RCW.get_action_names(env)` SR:486."""
    return ("MOVE_FORWARD", "MOVE_BACKWARD", "TURN_LEFT", "TURN_RIGHT")


def wu_to_tu(x_wu) -> int:
    """utils.jl:5: the (1-based) tile of a world-unit coordinate."""
    return int(np.floor(x_wu)) + 1


def wu_to_pu(x_wu, pu_per_wu) -> int:
    """utils.jl:6: the (1-based) pixel of a world-unit coordinate; the product is formed in x_wu's own type, as Julia does."""
    return int(np.floor(x_wu * pu_per_wu)) + 1


def pu_to_tu(i_pu: int, pu_per_tu: int) -> int:
    """utils.jl:7: the (1-based) tile of a (1-based) pixel, `(i_pu - 1) ÷ pu_per_tu + 1`.  Julia's `÷` truncates toward zero
    (Python's `//` floors): for a pixel off the image's low edge, i_pu <= 0, the two differ — pixel 0 at 32 pixels a tile is
    tile 1 in the reference, not tile 0."""
    n, d = int(i_pu) - 1, int(pu_per_tu)
    q = abs(n) // abs(d)
    return (q if (n < 0) == (d < 0) else -q) + 1
