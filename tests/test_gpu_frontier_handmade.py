"""rcw_frontier_kernel on hand-made seen maps (tests/frontier_cases.py; what each family holds is asserted on the CPU in
tests/test_frontier_cases_spec.py).  In every rollout test the kernel floods maps the seen-map kernel wrote: the bytes 0 .. 3 inside a wall
border.  Here an exported row of the state archive is cut at the plan's offsets (tests/snapshot_rows.py), its `seen_map.map` overwritten,
the row imported and restored: the restore puts the map back as the row holds it, launches no seen-map kernel, and floods the restored
agents again.  Directly behind it the engine's own map is held to the hand-made one, and field, distance, tiles and the action words of
every agent to tests/frontier_ref.py on that map — integers, compared exactly.  No step follows a restore: `seen_map.bits` is the row's.

Frames are 8 rays by 8 rows: nothing here reads a pixel."""
import numpy as np
import pytest

import frontier_cases as FC
import frontier_ref as FR
import snapshot_rows as SR

pytestmark = pytest.mark.gpu


def make(rcw, batch, H, W, nd=8, T="Float32", seed=11):
    env = rcw.SingleRoomModule.SingleRoom(batch=batch, seed=seed, T=T, auto_reset=True, num_directions=nd, position_increment_wu=0.25,
                                          player_radius_wu=0.25, height_tile_map_tu=H, width_tile_map_tu=W, num_rays=8,
                                          height_camera_view_pu=8, out_of_bounds=1)
    env.set_seen_map(True)
    env.set_frontier(True)
    env.set_snapshots(batch)
    return env


def flood_handmade(rcw, case, maps=None, T="Float32", state=None):
    """the flow: an engine of the case's shape, poses where the case has them, the maps through an edited row, every check behind the restore.
    Returns (the reference's arrays, what Tracked counted)."""
    maps = case.maps if maps is None else maps
    env = make(rcw, len(maps), case.H, case.W, T=T)
    try:
        if state is not None:
            env.set_state(*state)
        assert env.seen_map_device.ptr % 16 == 0                                  # agent a's map starts a H W bytes behind a multiple of 16: FC.wide_path
        SR.feed(env, "seen_map.map", maps)
        np.testing.assert_array_equal(env.seen_map, maps)                         # the kernel flooded THIS map
        t = FR.Tracked(env, enable=False)                                         # (its first check: all five arrays against the reference)
        return t.check("behind the restore"), t.seen
    finally:
        env.close()


def ids(cases):
    return [c.name for c in cases]


@pytest.mark.parametrize("case", FC.bytes_wide() + FC.bytes_narrow(), ids=ids(FC.bytes_wide() + FC.bytes_narrow()))
def test_every_byte_is_classified_alike_sixteen_a_lane_and_a_byte_a_lane(rcw, case):
    """gadgets passable | v | unseen for every byte v: at 16 x 16 all 256 maps go sixteen bytes a lane, v at every index mod 16; at
    17 x 15 sixty-two of 67 maps go a byte a lane and five sixteen a lane with a tail of 15"""
    exp, _ = flood_handmade(rcw, case)
    crossed = sum(int(exp["field"][a][i, cols[0]] == 2) for a, m in enumerate(case.maps) for _, _, (i, cols), _ in FC.gadget_fields(m))
    assert crossed > 0 and (exp["tiles"] > 0).any()


BORDER = FC.border_and_wrap()


@pytest.mark.parametrize("case", BORDER, ids=ids(BORDER))
def test_passable_and_unseen_tiles_in_the_first_and_last_row_and_column(rcw, case):
    """the column-wrap pairs, sources on the border and random maps without a wall border, at H W on the edges of a bitmap word, the
    wavefront and the 16-byte load"""
    state = None
    if (case.H, case.W) == (3, 3):
        # the one interior tile is the goal: the reset's sampler gives up (RCW_WARN_SAMPLER_GAVE_UP) and leaves the player where the
        # archive's validation admits no pose.  Every agent onto that tile, then.
        B = len(case.maps)
        state = (np.full((B, 2), 2), np.full((B, 2), 1.5), np.arange(B) % 8)
    exp, seen = flood_handmade(rcw, case, state=state)
    if case.name.startswith("wrap"):
        for a, (tiles, cells) in enumerate(FC.wrap_maps(case.H, case.W)[1]):
            assert exp["tiles"][a] == tiles and int((exp["field"][a] != FC.X).sum()) == len(cells)
    else:
        assert seen["most_sources"] > 0


FULL = FC.full_queue()


@pytest.mark.parametrize("case", FULL, ids=ids(FULL))
def test_sources_and_passable_tiles_that_fill_the_queue(rcw, case):
    exp, seen = flood_handmade(rcw, case)
    passable = ((case.maps == 1) | (case.maps == 3)).reshape(2, -1).sum(axis=1)
    assert (exp["tiles"] + passable == case.H * case.W).all() and seen["widest_level"] > 64 and seen["most_sources"] > 64


DEEP = FC.deep_floods()


@pytest.mark.parametrize("T", ["Float32", "Float64"])
@pytest.mark.parametrize("case", DEEP, ids=ids(DEEP))
def test_floods_five_hundred_levels_deep(rcw, case, T):
    """a serpentine with one source at its end; agents on the source, on a wall, in a pocket no source reaches and deep in the corridor,
    at a tile's centre and off it"""
    names = sorted(case.poses) * 2
    B = len(names)
    which = np.array([case.poses[n][0] for n in names])
    tile = np.array([case.poses[n][1] for n in names], np.float64)
    off = np.where(np.arange(B)[:, None] < B // 2, 0.5, np.random.default_rng(B).random((B, 2)) * 0.999)
    goal = np.tile([case.H - 1, case.W - 1], (B, 1))
    exp, _ = flood_handmade(rcw, case, maps=case.maps[which], T=T, state=(goal, tile + off, np.arange(B) % 8))
    d = exp["distance"]
    assert int(FR.level_sizes(exp["field"][names.index("deep")]).size) >= 500
    assert (d == 0).any() and (d == -1).any() and (d > 255).any(), d
    assert dict(zip(names, d))["source"] == 0 and dict(zip(names, d))["pocket"] == -1


@pytest.mark.parametrize("case", FC.wide_levels(), ids=ids(FC.wide_levels()))
def test_levels_and_seeds_wider_than_a_wavefront_on_a_non_square_map(rcw, case):
    """a room with one unseen tile in the middle: 81 levels, the widest of 80 tiles; a passable cross on an unseen map: every neighbour
    of the cross a source"""
    exp, _ = flood_handmade(rcw, case)
    room = FR.level_sizes(exp["field"][0])
    assert (room.size, int(room.max())) == (81, 80) and list(exp["tiles"][:1]) == [1] and exp["tiles"][1] > 64


def test_a_masked_restore_floods_the_agents_of_the_mask_and_keeps_every_byte_of_the_others(rcw):
    """random maps without a border at 17 x 15 go to the agents of a mask; the others keep map, field, distance and tiles, and their
    action words are the rule's on their unchanged field"""
    (case,) = [c for c in FC.border_and_wrap() if c.name == "random, 17 x 15"]
    B = len(case.maps)
    rng = np.random.default_rng(23)
    env = make(rcw, B, case.H, case.W)
    t = FR.Tracked(env, enable=False)
    for k in range(4):
        rcw.act_(env, rng.integers(1, 5, B).astype(np.uint8))
    t.check("before", stepped=True)
    before = dict(map=env.seen_map, field=env.frontier_field, distance=env.frontier_distance.numpy().copy(), tiles=env.frontier_tiles.numpy().copy())
    mask = rng.random(B) < 0.5
    assert mask.any() and not mask.all()
    SR.feed(env, "seen_map.map", case.maps, mask=mask)
    after = dict(map=env.seen_map, field=env.frontier_field, distance=env.frontier_distance.numpy(), tiles=env.frontier_tiles.numpy())
    np.testing.assert_array_equal(after["map"][mask], case.maps[mask])
    for name in before:
        np.testing.assert_array_equal(after[name][~mask], before[name][~mask], err_msg=name)
    assert (after["field"][mask] != before["field"][mask]).any()
    t.check("behind the masked restore")                                          # every agent, on the map it now holds
    env.close()
