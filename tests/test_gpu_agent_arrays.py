"""The table of a handle's live per-agent arrays on the GPU (csrc/rcw_handle.h, rcw_handle::live): for every array that has a `*_device_ptr`
export, the bytes behind that pointer — read with rcw_memcpy_to_host — are the bytes the array's host readout hands out, after every call;
and a save of all agents exports rows whose segments, cut at rcw_dev_snapshot_plan's offsets, are those same readouts.  The readouts, the
pointers and the archive's copy all look an array up in the one table: a part carved at one place and handed out at another shows here.

tests/snapshot_cases.py's engine with every feature on, shape ODD (5 x 5 map, gray 7 x 9, k = 3).  B = 5: 4-byte arrays of 20 bytes, a seen
map of 125 — every part but the first starts behind real padding; B = 67: more than a wavefront, and odd.  Both world-unit types (the
statistics' previous position and the local map's offset table change size).  Through the C ABI itself, not the Python properties."""
import ctypes as C

import numpy as np
import pytest

import snapshot_cases as SC
import snapshot_rows as SR
from test_snapshot_spec import SHAPE_FIELDS

pytestmark = pytest.mark.gpu

WORDS = dict(goal=("goal_distance", "goal_start_distance", "goal_progress"), seen=("seen_count", "seen_new", "goal_seen"),
             stats=("finished", "outcome", "length", "moves", "level", "spl_q16", "episodes"))
# the record's segment of every public array (the core state's five without a device pointer included: host readouts of the same table)
SEGMENT = {"pos": "position", "pos64": "position", "dir": "direction", "goal": "goal", "reward": "reward", "done": "done", "episode": "episode",
           "tile_map": "tile_map", "episode_steps": "episode_steps", "truncated": "truncated",
           "goal_distance.field": "goal_distance_field", "goal_distance.distance": "goal_distance", "goal_distance.start_distance": "goal_start_distance",
           "goal_distance.progress": "goal_progress", "seen_map.seen_count": "seen_count", "seen_map.newly_seen": "seen_new", "seen_map.goal_seen": "goal_seen",
           "seen_map.map": "seen_map", "learner_view.stack": "learner_view", "local_map.image": "local_map", "layout_source.layout": "wall_layout",
           **{"episode_stats." + w: w for w in WORDS["stats"]}}
PRIVATE = {"goal_distance.last_episode", "seen_map.last_episode", "seen_map.bits", "learner_view.last_episode", "layout_source.last_episode",
           "episode_stats.prev_x", "episode_stats.prev_y", "episode_stats.last_episode"}


def spec(env, B, c, T):
    """name -> an empty host array of the array's type and shape"""
    H, W, (vh, vw), k = c["H"], c["W"], c["view"], c["k"]
    rows = C.c_int32()
    env._check(env._lib.rcw_episode_stats_info(env._h, None, C.byref(rows), None))
    nchunks = (2 * H * W + 63) // 64
    s = dict(reward=(np.float32,), done=(np.uint8,), truncated=(np.uint8,), episode_steps=(np.uint32,),
             goal_distance=(np.int32,), goal_start_distance=(np.int32,), goal_progress=(np.int32,), goal_distance_field=(np.uint16, H * W),
             seen_count=(np.int32,), seen_new=(np.int32,), goal_seen=(np.int32,), seen_map=(np.uint8, H * W), local_map=(np.uint8, 25),
             learner_view=(np.uint8, k * vh * vw), wall_layout=(np.int32,), finished=(np.uint8,), outcome=(np.uint8,), length=(np.uint32,),
             moves=(np.uint32,), level=(np.int32,), spl_q16=(np.int32,), episodes=(np.uint32,),
             position=(np.float64 if T == "Float64" else np.float32, 2), direction=(np.int32,), goal=(np.int32, 2), episode=(np.uint32,),
             tile_map=(np.uint64, nchunks))
    out = {name: np.zeros((B,) + tuple(v[1:]), v[0]) for name, v in s.items()}
    out["table"] = np.zeros(8 * (1 + rows.value), np.uint64)
    return out


def ptr(a):
    return C.c_void_p(a.ctypes.data)


def host_readouts(env, B, c, T):
    lib, h, ok, r = env._lib, env._h, env._check, spec(env, B, c, T)
    ok(lib.rcw_reward_typed(h, ptr(r["reward"])))
    for name in ("done", "truncated", "episode_steps", "direction", "goal", "episode"):
        ok(getattr(lib, "rcw_" + name)(h, ptr(r[name])))
    ok((lib.rcw_position64 if T == "Float64" else lib.rcw_position)(h, ptr(r["position"])))
    ok(lib.rcw_tile_map_chunks(h, ptr(r["tile_map"])))
    ok(lib.rcw_goal_distance(h, *[ptr(r[w]) for w in WORDS["goal"]]))
    ok(lib.rcw_goal_distance_field(h, 0, B, ptr(r["goal_distance_field"])))
    ok(lib.rcw_seen_words(h, *[ptr(r[w]) for w in WORDS["seen"]]))
    ok(lib.rcw_seen_map(h, 0, B, ptr(r["seen_map"])))
    ok(lib.rcw_local_map_copy(h, ptr(r["local_map"]), 0, B))
    ok(lib.rcw_learner_view_copy(h, ptr(r["learner_view"]), 0, B))
    ok(lib.rcw_wall_layout(h, ptr(r["wall_layout"])))
    ok(lib.rcw_episode_stats(h, *[ptr(r[w]) for w in WORDS["stats"]]))
    ok(lib.rcw_episode_stats_table(h, ptr(r["table"])))
    return r


def device_pointers(env):
    lib, h, ok, p = env._lib, env._h, env._check, {}

    def ask(fn, *names):
        got = [C.c_void_p() for _ in names]
        ok(fn(h, *[C.byref(g) for g in got]))
        assert all(g.value for g in got), names
        p.update(zip(names, [g.value for g in got]))

    for name in ("reward", "done", "truncated", "episode_steps", "local_map", "learner_view", "wall_layout", "seen_map"):
        ask(getattr(lib, f"rcw_{name}_device_ptr"), name)
    ask(lib.rcw_goal_distance_device_ptr, *WORDS["goal"])
    ask(lib.rcw_goal_distance_field_device_ptr, "goal_distance_field")
    ask(lib.rcw_seen_words_device_ptr, *WORDS["seen"])
    ask(lib.rcw_episode_stats_device_ptr, *WORDS["stats"])
    ask(lib.rcw_episode_stats_table_device_ptr, "table")
    return p


def assert_pointers_hold_the_readouts(env, B, c, T, where):
    want, got, pointers = host_readouts(env, B, c, T), spec(env, B, c, T), device_pointers(env)
    assert len(set(pointers.values())) == len(pointers) == 23
    for name, p in pointers.items():
        env._check(env._lib.rcw_memcpy_to_host(env._h, ptr(got[name]), C.c_void_p(p), got[name].nbytes))
        assert got[name].tobytes() == want[name].tobytes(), (where, name)
    return want


@pytest.mark.parametrize("T", ["Float32", "Float64"])
@pytest.mark.parametrize("B", [5, 67])
def test_every_device_pointer_holds_what_its_readout_hands_out(rcw, B, T):
    c = SC.ODD
    env = SC.make(rcw, B, c, T=T, rows=B)
    acts = SC.actions(B, 8, seed=B)
    assert_pointers_hold_the_readouts(env, B, c, T, "configured")
    for k, a in enumerate(acts[:6]):
        rcw.act_(env, a)
        assert_pointers_hold_the_readouts(env, B, c, T, f"step {k}")
    rcw.reset_(env, mask=(np.arange(B) % 2).astype(np.uint8), seed=9)
    assert_pointers_hold_the_readouts(env, B, c, T, "masked reset")
    for k, a in enumerate(acts[6:]):
        rcw.act_(env, a)
        last = assert_pointers_hold_the_readouts(env, B, c, T, f"step {6 + k}")
    assert last["episode_steps"].any() and last["seen_count"].all() and last["learner_view"].any() and last["length"].any()   # (something to compare)

    # the archive's copy goes through the same table: a save of every agent, exported, cut at the plan's offsets
    env.snapshot_save()
    exported = env.snapshot_export()
    kw = SR.shape_of(env, source_kind=1, layouts=3)
    assert kw == dict(H=c["H"], W=c["W"], nd=8, N=64, Hc=64, real64=int(T == "Float64"), reward_type=0, goal=1, seen=1, stats=1, view_fmt=kw["view_fmt"],
                      view_layout=kw["view_layout"], view_C=1, view_h=c["view"][0], view_w=c["view"][1], view_frames=c["k"], local_source=kw["local_source"],
                      local_size=kw["local_size"], local_cells=kw["local_cells"], source_kind=1, layouts=3) and set(kw) <= set(SHAPE_FIELDS)
    table = SR.segments(exported, **kw)                                           # (the plan's key and row_bytes are the export's)
    assert exported["rows"].shape == (B, exported["row_bytes"])
    end, seen = 0, set()
    for name, offset, size in table:
        assert offset == end
        if name not in PRIVATE:
            want = last[SEGMENT[name]].reshape(B, -1).view(np.uint8)
            assert want.shape[1] == size and exported["rows"][:, offset:offset + size].tobytes() == want.tobytes(), name
            seen.add(SEGMENT[name])
        end = offset + size
    assert end == exported["row_bytes"] and seen == set(last) - {"table"}
