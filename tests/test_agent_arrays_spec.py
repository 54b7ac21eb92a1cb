"""The per-agent arrays of a handle without a device (csrc/rcw_handle.h, "the per-agent arrays of a handle"), through the development build:

  * rcw_dev_agent_arrays    one feature's parts — id, name, bytes per agent, archived — its head, and the carve of them for a batch;
  * rcw_dev_snapshot_plan   the state archive's record, held to tests/golden/snapshot_plan_keys.json: names, bytes, row_bytes and shape key of
                            every shape of tests/test_snapshot_spec.py as the library planned them before the one description existed.

What a carve must hold follows from its use: a setter allocates `total` bytes, puts the head at the buffer's start and part k's [B] array at
offset[k].  CPU only."""
import ctypes as C
import json
import os

import pytest

from test_snapshot_spec import ALL_ON, F64_5X5, devlib, plan, shape  # noqa: F401  (devlib: the fixture)

FEATURES = ("core", "goal_distance", "seen_map", "learner_view", "local_map", "layout_source", "episode_stats")
MAP_7X9 = dict(ALL_ON, H=7, W=9)                                            # H W = 63: a seen map of 63 bytes, two words of bits
SHAPES = {"all": ALL_ON, "f64_5x5": F64_5X5, "7x9": MAP_7X9}
BATCHES = (1, 3, 5, 63, 64, 65, 257)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "snapshot_plan_keys.json")


def arrays(lib, kw, feature, B):
    lib.rcw_dev_agent_arrays.argtypes = [C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_char_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_uint32),
                                         C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    names, ids, sizes, kept, offsets = C.create_string_buffer(4096), (C.c_int32 * 16)(), (C.c_uint32 * 16)(), (C.c_uint8 * 16)(), (C.c_uint64 * 16)()
    head, total = C.c_uint64(), C.c_uint64()
    n = lib.rcw_dev_agent_arrays(shape(**kw), feature, B, names, 4096, ids, sizes, kept, offsets, C.byref(head), C.byref(total))
    assert 0 <= n <= 10
    parts = [dict(name=name, id=ids[k], bytes=sizes[k], archived=bool(kept[k]), offset=offsets[k]) for k, name in enumerate(names.value.decode().split("\n")[:n])]
    return parts, head.value, total.value


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("case", sorted(SHAPES))
def test_a_carve_keeps_every_part_apart_and_on_16_bytes(devlib, case, B):
    kw = SHAPES[case]
    for feature in range(len(FEATURES)):
        parts, head, total = arrays(devlib, kw, feature, B)
        assert parts or (head == 0 and total == 0), FEATURES[feature]
        end = head                                                         # the head fits in front of the first part
        for p in parts:
            assert p["offset"] % 16 == 0 and p["bytes"] > 0, (FEATURES[feature], p)
            assert end <= p["offset"], (FEATURES[feature], p)              # in list order, disjoint
            end = p["offset"] + p["bytes"] * B
        assert end <= total, FEATURES[feature]                             # the last part ends inside what is allocated
        assert total - end < 16 and all(p["offset"] - q["offset"] - q["bytes"] * B < 16 for q, p in zip(parts, parts[1:]))   # (and nothing but padding between)


@pytest.mark.parametrize("case", sorted(SHAPES))
def test_the_archived_parts_of_every_feature_are_the_archives_record(devlib, case):
    """THE tie between the carve and the record: what a setter allocates for a part and what a save or a restore moves are one number."""
    kw = SHAPES[case]
    segments, row_bytes, _ = plan(devlib, **kw)
    listed, ids = [], []
    for feature in range(len(FEATURES)):
        parts, _, _ = arrays(devlib, kw, feature, 5)
        listed += [(p["name"], p["bytes"]) for p in parts if p["archived"]]
        ids += [p["id"] for p in parts]
    assert listed == segments and sum(b for _, b in listed) == row_bytes
    assert ids == sorted(set(ids))                                         # an id a part, in the order of the lists


def test_what_the_archive_leaves_out_and_the_heads(devlib):
    def left_out(kw, feature):
        return [p["name"] for p in arrays(devlib, kw, feature, 3)[0] if not p["archived"]]

    assert [left_out(ALL_ON, f) for f in range(7)] == [[], [], [], ["learner_view.staging"], [], ["layout_source.status_seen", "layout_source.mask"], []]
    assert left_out(dict(ALL_ON, view_frames=1), 3) == []                  # k = 1: the kernels' frame IS the view
    heads = [arrays(devlib, ALL_ON, f, 3)[1] for f in range(7)]
    # the box tables (7 + 1 rows, 9 + 1 columns), five Float32 offsets, the table's batch row and three level rows of 8 UInt64
    assert heads == [0, 0, 0, 4 * (8 + 10), 4 * 5, 0, 8 * 8 * (1 + 3)]
    assert arrays(devlib, dict(ALL_ON, view_fmt=6, view_C=2), 3, 3)[1] == 4 * (8 + 10 + 64 + 1)   # gray + depth: the depth sums, Hc + 1
    assert arrays(devlib, dict(F64_5X5, local_source=1, local_size=7, local_cells=2), 4, 3)[1] == 8 * 7
    assert arrays(devlib, F64_5X5, 6, 3)[1] == 8 * 8                       # no layout source: the batch row alone
    # a feature that is off has nothing
    assert [arrays(devlib, F64_5X5, f, 3) for f in (3, 4, 5)] == [([], 0, 0)] * 3


def test_the_record_is_the_one_planned_before_the_one_description(devlib):
    golden = json.load(open(GOLDEN))
    assert len(golden) == 19
    for name, want in golden.items():
        segments, row_bytes, key = plan(devlib, **want["shape"])
        assert [s for s, _ in segments] == want["names"], name
        assert [b for _, b in segments] == want["bytes"], name
        assert row_bytes == want["row_bytes"] and "%016x" % key == want["key"], name
