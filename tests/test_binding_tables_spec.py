"""The Python binding's per-agent words, tile-order arrays and alias caches (single_room.py, sharded.py), pinned without a device.

A `SingleRoom` made with `__new__` over a library that records every native call, writes a fresh address into every pointer it is
asked for and fills every host buffer with 0, 1, 2, ...: what each public name calls, what it hands out, what it caches, which setter
drops which cache, what `close()` leaves behind, and what a host copy adds to `host_syncs`.  The map is 5 x 7, so a transpose that
went missing shows in the shapes."""
import ctypes
import types

import numpy as np
import pytest

from helpers import FakeLib, bare_env

B, H, W, S = 4, 5, 7, 2

# (host function, device-pointer function, ((public name, dtype), ...) in the ABI's order)
WORD_GROUPS = {
    "goal distance": ("rcw_goal_distance", "rcw_goal_distance_device_ptr",
                      (("goal_distance", np.int32), ("goal_start_distance", np.int32), ("goal_progress", np.int32))),
    "guide": ("rcw_guide", "rcw_guide_device_ptr", (("guide_action", np.uint8), ("guide_heading", np.int32))),
    "seen words": ("rcw_seen_words", "rcw_seen_words_device_ptr",
                   (("seen_count", np.int32), ("seen_new", np.int32), ("goal_seen", np.int32))),
    "frontier": ("rcw_frontier", "rcw_frontier_device_ptr",
                 (("frontier_distance", np.int32), ("frontier_tiles", np.int32), ("explore_action", np.uint8), ("explore_heading", np.int32))),
    "visit words": ("rcw_visit_words", "rcw_visit_words_device_ptr",
                    (("visits_here", np.int32), ("visited_cells", np.int32), ("visit_first", np.int32), ("level_visits_here", np.uint32))),
    "episode statistics": ("rcw_episode_stats", "rcw_episode_stats_device_ptr",
                           (("finished", np.uint8), ("outcome", np.uint8), ("length", np.uint32), ("moves", np.uint32), ("level", np.int32),
                            ("spl_q16", np.int32), ("episodes", np.uint32))),
    "wall layout": ("rcw_wall_layout", "rcw_wall_layout_device_ptr", (("wall_layout", np.int32),)),
}
WORDS = [(group, k) for group, (_, _, words) in WORD_GROUPS.items() for k in range(len(words))]

# public name -> (dtype, host function, device-pointer function, has the sector axis)
TILE_ARRAYS = {
    "goal_distance_field": (np.uint16, "rcw_goal_distance_field", "rcw_goal_distance_field_device_ptr", False),
    "seen_map": (np.uint8, "rcw_seen_map", "rcw_seen_map_device_ptr", False),
    "frontier_field": (np.uint16, "rcw_frontier_field", "rcw_frontier_field_device_ptr", False),
    "visit_map": (np.uint16, "rcw_visit_map", "rcw_visit_map_device_ptr", True),
}


class RecordingLib(FakeLib):
    """Every `rcw_*` export: returns 0, and records (name, which arguments behind the handle are None) in `calls`.  A
    `byref(c_void_p)` gets an address no earlier call gave out, kept in `address[(name, slot)]`; a `byref(c_int32)` gets 1 (every
    feature reads as enabled) — but `rcw_visit_map_info`, whose second word, `sectors`, is S; a host buffer of a readout
    (`ndarray.ctypes.data_as(c_void_p)`: the pointer keeps its array) is filled with 0, 1, 2, ..."""

    def __init__(self):
        super().__init__()
        self.calls, self.address, self._next = [], {}, 0x10000
        self.goal_distance_enabled = 1

    def __getattr__(self, name):
        if not name.startswith("rcw_"):
            raise AttributeError(name)

        def export(h, *args):
            assert h, f"{name} with a NULL handle"
            self.calls.append((name, tuple(a is None for a in args)))
            for k, a in enumerate(args):
                target = getattr(a, "_obj", None)                        # byref(x)
                if isinstance(target, ctypes.c_void_p):
                    self._next += 0x100
                    target.value = self.address[(name, k)] = self._next
                elif isinstance(target, ctypes.c_int32):
                    target.value = S if (name, k) == ("rcw_visit_map_info", 1) else self.goal_distance_enabled if name == "rcw_goal_distance_enabled" else 1
                elif isinstance(a, ctypes.c_void_p) and hasattr(a, "_arr") and not name.startswith("rcw_set_"):
                    a._arr.reshape(-1)[:] = np.arange(a._arr.size)
            return 0

        return export

    def take(self, ignore=("rcw_visit_map_info",)):
        """The calls since the last `take`, the settings readouts in `ignore` left out."""
        calls, self.calls = [c for c in self.calls if c[0] not in ignore], []
        return calls


class _Cfg:
    height_tile_map_tu, width_tile_map_tu, num_directions, num_rays = H, W, 16, 8


@pytest.fixture()
def env(rcw):
    e = bare_env(rcw, RecordingLib())
    assert e.batch == B
    e.cfg, e.rng = _Cfg(), None
    return e


def _word(env, group, k):
    name = WORD_GROUPS[group][2][k][0]
    return getattr(env.episode_stats, name) if group == "episode statistics" else getattr(env, name)


def _fill(shape, dtype):
    return np.arange(int(np.prod(shape))).astype(dtype).reshape(shape)


@pytest.mark.parametrize("group,k", WORDS, ids=[WORD_GROUPS[g][2][k][0] for g, k in WORDS])
def test_a_word_is_fetched_once_cached_and_copied_alone(rcw, env, group, k):
    SR, lib = rcw.SingleRoomModule, env._lib
    host, device_ptr, words = WORD_GROUPS[group]
    name, dtype = words[k]
    x = _word(env, group, k)
    assert lib.take() == [(device_ptr, (False,) * len(words))]                      # one call, every slot asked for
    assert isinstance(x, SR.DeviceArray)
    assert (x.ptr, x.shape, x.dtype) == (lib.address[(device_ptr, k)], (B,), np.dtype(dtype))
    assert len({lib.address[(device_ptr, j)] for j in range(len(words))}) == len(words)
    assert _word(env, group, k) is x and lib.take() == []                           # the very object, no call
    assert env.host_syncs == 0
    a = np.asarray(x)
    assert lib.take() == [(host, tuple(j != k for j in range(len(words))))]        # one call, this word's slot alone
    assert a.dtype == np.dtype(dtype) and a.shape == (B,)
    np.testing.assert_array_equal(a, np.arange(B))
    assert env.host_syncs == 1
    np.asarray(x)
    assert env.host_syncs == 2 and _word(env, group, k) is x


def test_the_table_of_this_test_names_24_words():
    assert len(WORDS) == 24 and len({WORD_GROUPS[g][2][k][0] for g, k in WORDS}) == 24


@pytest.mark.parametrize("name", TILE_ARRAYS)
def test_a_tile_order_array_comes_back_indexed_like_the_walls(env, name):
    lib = env._lib
    dtype, host, _, sectors = TILE_ARRAYS[name]
    lead = (B, S) if sectors else (B,)
    a = getattr(env, name)
    assert lib.take() == [(host, (False, False, False))] and env.host_syncs == 1   # (h, first, count, out): one call, one wait
    assert isinstance(a, np.ndarray) and a.dtype == np.dtype(dtype) and a.shape == lead + (H, W)
    assert a.flags.c_contiguous
    np.testing.assert_array_equal(a, np.swapaxes(_fill(lead + (W, H), dtype), -1, -2))
    getattr(env, name)
    assert env.host_syncs == 2


@pytest.mark.parametrize("name", TILE_ARRAYS)
def test_a_tile_order_alias_is_made_anew_in_the_maps_own_order(rcw, env, name):
    SR, lib = rcw.SingleRoomModule, env._lib
    dtype, host, device_ptr, sectors = TILE_ARRAYS[name]
    lead = (B, S) if sectors else (B,)
    attribute = getattr(SR.SingleRoom, name + "_device")
    if name == "goal_distance_field":                                               # the one method among them
        assert callable(attribute) and not isinstance(attribute, property)
        get = lambda: env.goal_distance_field_device()                              # noqa: E731
    else:
        assert isinstance(attribute, property) and not callable(attribute)
        get = lambda: getattr(env, name + "_device")                                # noqa: E731
    x = get()
    assert lib.take() == [(device_ptr, (False,))]
    assert isinstance(x, SR.DeviceArray)
    assert (x.ptr, x.shape, x.dtype) == (lib.address[(device_ptr, 0)], lead + (W, H), np.dtype(dtype))
    y = get()
    assert y is not x and lib.take() == [(device_ptr, (False,))]                    # never cached
    assert not any(v is x or v is y for v in env.__dict__.values())
    assert env.host_syncs == 0
    a = x._host_getter()
    assert lib.take() == [(host, (False, False, False))] and env.host_syncs == 1
    assert a.dtype == np.dtype(dtype) and a.flags.c_contiguous
    np.testing.assert_array_equal(a, _fill(lead + (W, H), dtype))
    np.testing.assert_array_equal(np.asarray(x), a)


# ---- which setter drops which cache --------------------------------------------------------------------------------
CACHED = {  # a name of every cached group -> the call its first access makes
    "goal distance": (lambda e: e.goal_distance, "rcw_goal_distance_device_ptr"),
    "guide": (lambda e: e.guide_action, "rcw_guide_device_ptr"),
    "seen words": (lambda e: e.seen_count, "rcw_seen_words_device_ptr"),
    "frontier": (lambda e: e.frontier_distance, "rcw_frontier_device_ptr"),
    "visit words": (lambda e: e.visits_here, "rcw_visit_words_device_ptr"),
    "episode statistics": (lambda e: e.episode_stats, "rcw_episode_stats_device_ptr"),
    "wall layout": (lambda e: e.wall_layout, "rcw_wall_layout_device_ptr"),
    "local map": (lambda e: e.local_map, "rcw_local_map_device_ptr"),
}
_RING = np.ones((1, H, W), dtype=np.uint8)
_RING[:, 1:-1, 1:-1] = 0
SETTERS = [  # (id, call, the groups whose caches it drops, a setup before the caches are filled)
    ("set_goal_distance(True)", lambda e: e.set_goal_distance(True), {"goal distance"}, None),
    ("set_goal_distance(False)", lambda e: e.set_goal_distance(False), {"goal distance", "guide"}, None),
    ("set_guide(True)", lambda e: e.set_guide(True), {"guide"}, None),
    ("set_guide(False)", lambda e: e.set_guide(False), {"guide"}, None),
    ("set_guide(True) without the goal distance", lambda e: e.set_guide(True), {"guide", "goal distance"},
     lambda e: setattr(e._lib, "goal_distance_enabled", 0)),                        # (it switches the goal distance on first)
    ("set_seen_map(True)", lambda e: e.set_seen_map(True), {"seen words", "local map"}, None),
    ("set_seen_map(False)", lambda e: e.set_seen_map(False), {"seen words", "local map"}, None),
    ("set_frontier(True)", lambda e: e.set_frontier(True), {"frontier"}, None),
    ("set_frontier(False)", lambda e: e.set_frontier(False), {"frontier"}, None),
    ("set_local_map(3)", lambda e: e.set_local_map(3), {"local map"}, None),
    ("set_local_map(None)", lambda e: e.set_local_map(None), {"local map"}, None),
    ("set_episode_stats(True)", lambda e: e.set_episode_stats(True), {"episode statistics"}, None),
    ("set_episode_stats(False)", lambda e: e.set_episode_stats(False), {"episode statistics"}, None),
    ("set_visit_map()", lambda e: e.set_visit_map(), {"visit words"}, None),
    ("set_visit_map(None)", lambda e: e.set_visit_map(None), {"visit words"}, None),
    ("set_wall_bank(walls)", lambda e: e.set_wall_bank(_RING, [3]), {"wall layout"}, None),
    ("set_wall_bank(None)", lambda e: e.set_wall_bank(None), {"wall layout"}, None),
    ("set_wall_generator()", lambda e: e.set_wall_generator(levels=2), {"wall layout"}, None),
    ("set_wall_generator(None)", lambda e: e.set_wall_generator(None), {"wall layout"}, None),
    ("set_wall_caves()", lambda e: e.set_wall_caves(), {"wall layout"}, None),
    ("set_wall_caves(None)", lambda e: e.set_wall_caves(None), {"wall layout"}, None),
    ("set_wall_rooms()", lambda e: e.set_wall_rooms(), {"wall layout"}, None),
    ("set_wall_rooms(None)", lambda e: e.set_wall_rooms(None), {"wall layout"}, None),
    ("set_wall_bank_weights", lambda e: e.set_wall_bank_weights(None), set(), None),
    ("set_time_limit", lambda e: e.set_time_limit(5), set(), None),
    ("set_snapshots", lambda e: e.set_snapshots(2), set(), None),
]


@pytest.mark.parametrize("call,dropped,setup", [s[1:] for s in SETTERS], ids=[s[0] for s in SETTERS])
def test_a_setter_drops_its_own_caches_and_no_other(env, call, dropped, setup):
    lib = env._lib
    if setup:
        setup(env)
    before = {group: get(env) for group, (get, _) in CACHED.items()}
    lib.take()
    call(env)
    lib.take()
    for group, (get, device_ptr) in CACHED.items():
        after = get(env)
        fetched = [c[0] for c in lib.take(ignore=("rcw_visit_map_info", "rcw_local_map_info"))]
        if group in dropped:
            assert after is not before[group] and fetched == [device_ptr], group
        else:
            assert after is before[group] and fetched == [], group


def test_a_wall_bank_that_is_refused_on_the_host_keeps_the_layout_alias(env):
    """(the cache goes where the call reaches the library, not before the host's own checks)"""
    x = env.wall_layout
    with pytest.raises(ValueError):
        env.set_wall_bank(np.ones((1, H + 1, W), dtype=np.uint8))
    assert env.wall_layout is x


def test_close_leaves_no_alias_behind(rcw, env):
    SR = rcw.SingleRoomModule
    for group, k in WORDS:
        _word(env, group, k)
    for name in TILE_ARRAYS:
        getattr(env, name)
        x = getattr(env, name + "_device")
        x() if callable(x) else x
    env.local_map, env.reward_device(), env.episode_steps_device()
    for as_bool in (False, True):
        env.done_device(as_bool), env.truncated_device(as_bool)
    env._state_alias = SR.DeviceArray(0x2000, (B, 8, 8), np.uint32, env, lambda: None)      # (what rlbase.state caches)
    env._learner_view_alias = SR.DeviceArray(0x3000, (B, 1, 8, 8), np.uint8, env, lambda: None)
    env._constant_action_buffers = {1: object()}

    def holds_an_alias(v):
        if isinstance(v, types.SimpleNamespace):
            v = tuple(vars(v).values())
        return isinstance(v, SR.DeviceArray) or (isinstance(v, tuple) and any(isinstance(x, SR.DeviceArray) for x in v))

    assert sum(holds_an_alias(v) for v in env.__dict__.values()) == 7 + 1 + 6 + 2           # groups, local map, core, the two set here
    env.close()
    assert [k for k, v in env.__dict__.items() if holds_an_alias(v)] == []
    assert "_constant_action_buffers" not in env.__dict__
    assert env._lib.destroyed == 1 and not env._h


# ---- the docstrings: what help(SingleRoom) shows -------------------------------------------------------------------------
DOCS = {
    "goal_progress": """int32 (B,): tiles the last step brought each agent closer to its goal (negative: farther); 0 for an agent the call restarted
        or reset, and where either distance is -1.""",
    "explore_action": """uint8 (B,): the action that leads each agent to its nearest frontier tile, always in 1..4.  `.torch(sync=False)` on the GPU —
        `act_` takes it as it is —, `np.asarray(...)` for a host copy.""",
    "visit_first": """int32 (B,): 1 where the last call counted a cell the agent had not stood in this episode; 0 behind a restart.""",
    "seen_map_device": """The map where it lives: uint8 (B, W, H) in device memory — the tile map's own order, `[b, j-1, i-1]`.""",
}


def test_every_public_name_keeps_a_docstring(rcw):
    cls = rcw.SingleRoomModule.SingleRoom
    names = [words[k][0] for g, (_, _, words) in WORD_GROUPS.items() if g != "episode statistics" for k in range(len(words))]
    names += ["episode_stats", "local_map"] + list(TILE_ARRAYS) + [n + "_device" for n in TILE_ARRAYS]
    assert len(names) == 17 + 2 + 8
    for name in names:
        doc = getattr(cls, name).__doc__
        assert doc and doc.strip() and len(doc) > 40, name
    for name, doc in DOCS.items():
        assert getattr(cls, name).__doc__ == doc, name


# ---- sharded.py: the arrays a shard forwards ------------------------------------------------------------------------------
FORWARDED = ("guide_action", "guide_heading", "frontier_distance", "frontier_tiles", "explore_action", "explore_heading", "frontier_field",
             "visit_map", "visits_here", "visited_cells", "visit_first", "level_visits_here")


def test_a_shard_forwards_its_engines_arrays(rcw):
    from raycastworlds_jl_amd import sharded

    cls = sharded.ShardedSingleRoom
    batch = cls.__new__(cls)
    batch.env = types.SimpleNamespace(**{name: object() for name in FORWARDED})
    assert len(set(FORWARDED)) == 12
    for name in FORWARDED:
        assert isinstance(getattr(cls, name), property), name
        assert getattr(batch, name) is getattr(batch.env, name), name
    for name in ("goal_distance", "goal_progress", "seen_map", "seen_count", "goal_distance_field", "episode_stats", "wall_layout"):
        assert not hasattr(cls, name), name                                          # (not forwarded today: a feature, not this file's subject)
