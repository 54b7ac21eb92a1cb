"""The state archive's exported rows, cut at rcw_dev_snapshot_plan's offsets — test infrastructure, not a test.

An exported row is trusted but for goal, direction, position, tile-map border and layout index (validate_snapshot_row), and a restore puts
`seen_map.map` and `goal_distance.field` back as the row holds them without launching the kernels that write them: a test that overwrites
one segment of a row feeds a hand-made input to the kernels that READ it (rcw_frontier_kernel, rcw_guide_kernel).

  shape_of      the 23 words of the engine's shape from its own readouts; the layout source's words do not read back and come as keywords
  plan          the segment table of that shape: [(name, offset, bytes)], row_bytes, shape key
  segments      ... held to an export: the plan's row_bytes and key ARE the export's
  segment       a writable view (rows, bytes) of exported["rows"] for one segment name
  device_order  an (H, W) map or field as the device holds it: tile (i, j) at i + H j
  feed          save every agent, export, overwrite one segment with hand-made per-agent arrays, import, restore (the agents of `mask`)
"""
import ctypes as C

import numpy as np

from test_snapshot_spec import SHAPE_FIELDS


def shape_of(env, **source):
    """source: source_kind, layouts, levels, first_level of a handle with a layout source (0 without)"""
    assert not set(source) - {"source_kind", "layouts", "levels", "first_level"}, source
    cfg = env.cfg
    view = [C.c_int32() for _ in range(5)]
    env._check(env._lib.rcw_learner_view_info(env._h, *[C.byref(v) for v in view]))
    local = [C.c_int32() for _ in range(3)]
    env._check(env._lib.rcw_local_map_info(env._h, *[C.byref(v) for v in local]))
    fmt, layout, vh, vw, _flags = [v.value for v in view]
    kw = dict(H=cfg.height_tile_map_tu, W=cfg.width_tile_map_tu, nd=cfg.num_directions, N=cfg.num_rays, Hc=cfg.height_camera_view_pu,
              real64=int(env.T is np.float64), reward_type=cfg.reward_type, goal=int(env.goal_distance_enabled), seen=int(env.seen_map_enabled),
              stats=int(env.episode_stats_enabled), local_source=local[0].value, local_size=local[1].value, local_cells=local[2].value, **source)
    if fmt:
        kw.update(view_fmt=fmt, view_layout=layout, view_C=env._VIEW_CHANNELS[env.learner_view_info()["format"]], view_h=vh, view_w=vw,
                  view_frames=env.learner_view_stack)
    return kw


def plan(**kw):
    """([(name, offset, bytes)], row_bytes, key) of a shape, from the development build"""
    from raycastworlds_jl_amd import _capi

    assert not set(kw) - set(SHAPE_FIELDS), kw
    dev = C.CDLL(_capi.DEV_LIB_PATH)
    dev.rcw_dev_snapshot_plan.argtypes = [C.POINTER(C.c_int32), C.c_char_p, C.c_int32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    names, sizes, row_bytes, key = C.create_string_buffer(4096), (C.c_uint32 * 64)(), C.c_uint64(), C.c_uint64()
    n = dev.rcw_dev_snapshot_plan((C.c_int32 * len(SHAPE_FIELDS))(*[kw.get(f, 0) for f in SHAPE_FIELDS]), names, 4096, sizes, C.byref(row_bytes), C.byref(key))
    assert n > 0
    table, offset = [], 0
    for name, size in zip(names.value.decode().split("\n")[:n], sizes[:n]):
        table.append((name, offset, size))
        offset += size
    assert offset == row_bytes.value
    return table, row_bytes.value, key.value


def segments(exported, **kw):
    """the plan of shape `kw`, which must be the export's: its key and row_bytes, and rows of that many bytes"""
    table, row_bytes, key = plan(**kw)
    rows = exported["rows"]
    assert key == exported["shape_key"] and row_bytes == exported["row_bytes"] and rows.ndim == 2 and rows.shape[1] == row_bytes, (kw, row_bytes, exported["row_bytes"])
    return table


def segment(env, exported, name, **source):
    """a writable view (rows, bytes) of exported["rows"]: the segment `name` of every row"""
    found = [(offset, size) for n, offset, size in segments(exported, **shape_of(env, **source)) if n == name]
    assert len(found) == 1, name
    offset, size = found[0]
    rows = exported["rows"]
    assert rows.dtype == np.uint8 and rows.flags.writeable
    view = rows[:, offset:offset + size]
    assert np.shares_memory(view, rows)
    return view


def device_order(planes):
    """(B, H, W) -> (B, H * W) in the device's order, tile (i, j) at i + H j: each plane m goes in as m.T.reshape(-1)"""
    p = np.asarray(planes)
    assert p.ndim == 3
    return np.ascontiguousarray(p.transpose(0, 2, 1)).reshape(p.shape[0], -1)


def feed(env, name, planes, mask=None, **source):
    """save every agent into its own row, overwrite segment `name` of every row with planes (B, H, W) — uint8 for "seen_map.map", uint16 for
    "goal_distance.field" —, import the rows and restore the agents of `mask` (None: all).  Returns the edited export."""
    planes = np.asarray(planes)
    assert planes.dtype == dict([("seen_map.map", np.uint8), ("goal_distance.field", np.uint16)])[name]
    assert planes.shape == (env.batch, env.cfg.height_tile_map_tu, env.cfg.width_tile_map_tu), planes.shape
    assert env.snapshot_info["rows"] >= env.batch
    env.snapshot_save()
    exported = env.snapshot_export(0, env.batch)
    view = segment(env, exported, name, **source)
    flat = device_order(planes).view(np.uint8)
    assert flat.shape == view.shape, (flat.shape, view.shape)
    view[:] = flat
    env.snapshot_import(exported)
    env.snapshot_restore(mask=mask)
    return exported
