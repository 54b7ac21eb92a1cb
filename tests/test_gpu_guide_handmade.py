"""rcw_guide_kernel<float> and <double> on hand-made fields.  The header promises the no-advice words "on a field that has none" — one no
flood wrote —, and in every rollout test the kernel reads fields a flood wrote: an entry's nearer neighbour always exists, and the values
are small.  Here an exported row of the state archive is cut at the plan's offsets (tests/snapshot_rows.py), its `goal_distance.field`
overwritten, the row imported and restored: the restore puts the field back as the row holds it, launches no goal-distance kernel, and
launches the guide's on the restored field.  Directly behind it the engine's own field is held to the hand-made one and both words of
every agent to tests/guide_ref.py's rule on it — integers, compared exactly — and once more behind one step, where the agents whose
episode goes on still hold the hand-made field.

Frames are 8 rays by 8 rows: nothing here reads a pixel."""
import numpy as np
import pytest

import guide_ref as GR
import snapshot_rows as SR

pytestmark = pytest.mark.gpu

B = 67
X = 0xFFFF
VALUES = np.array([0, 1, 2, 3, 4, 0xFFFD, 0xFFFE, 0xFFFF], np.uint16)
CASES = [(nd, T, hw) for T in ("Float32", "Float64") for nd in (8, 130) for hw in ((5, 7), (9, 9))]


def handmade_fields(H, W, tiles, rng):
    """(B, H, W): agents 0 .. 2 constant fields of 0, 1 and 0xFFFF; 3: 0xFFFE under the player, 0xFFFD beside it, 0xFFFF elsewhere; 4: 0
    under the player, 0xFFFF around; 5 .. 8: 3 under the player and 2 at ONE neighbour — up, down, left, right —, 3 elsewhere; the
    others: drawn from VALUES, so that several neighbours hold f - 1, or none does"""
    fields = VALUES[rng.integers(0, len(VALUES), (B, H, W))]
    for a, v in enumerate((0, 1, X)):
        fields[a] = v
    i, j = tiles[3]
    fields[3] = X
    fields[3, i, j] = 0xFFFE
    fields[3, i, j + 1] = 0xFFFD
    i, j = tiles[4]
    fields[4] = X
    fields[4, i, j] = 0
    for k, (di, dj) in enumerate(((-1, 0), (1, 0), (0, -1), (0, 1))):
        i, j = tiles[5 + k]
        fields[5 + k] = 3
        fields[5 + k, i + di, j + dj] = 2
    return fields


def first_match(field, tile):
    """from the inputs alone: (the entry under the player, which of up / down / left / right is the first to hold one less — None: none)"""
    (H, W), (i, j) = field.shape, tile
    f = int(field[i, j])
    if f in (0, X):
        return f, None
    for k, (a, b) in enumerate(((i - 1, j), (i + 1, j), (i, j - 1), (i, j + 1))):
        if 0 <= a < H and 0 <= b < W and int(field[a, b]) == f - 1:
            return f, k
    return f, None


@pytest.mark.parametrize("nd,T,hw", CASES, ids=[f"nd{nd}-{T}-{h}x{w}" for nd, T, (h, w) in CASES])
def test_both_words_on_fields_no_flood_wrote(rcw, nd, T, hw):
    H, W = hw
    rng = np.random.default_rng([nd, H, W, T == "Float64"])
    env = rcw.SingleRoomModule.SingleRoom(batch=B, seed=11, T=T, auto_reset=True, num_directions=nd, position_increment_wu=0.25, player_radius_wu=0.25,
                                          height_tile_map_tu=H, width_tile_map_tu=W, num_rays=8, height_camera_view_pu=8, out_of_bounds=1)
    env.set_guide(True)                                                           # (enables the goal distance first)
    env.set_snapshots(B)
    # interior poses, which is all the archive's validation admits: a tile's centre or anywhere in it
    tiles = np.stack([rng.integers(1, H - 1, B), rng.integers(1, W - 1, B)], axis=1)
    off = np.where(rng.random((B, 2)) < 0.5, 0.5, rng.random((B, 2)) * 0.999)
    goal = np.stack([rng.integers(2, H, B), rng.integers(2, W, B)], axis=1)
    fields = handmade_fields(H, W, tiles, rng)
    # the headings: the rule's own heading (which does not depend on the agent's), one index before and one behind it go round the agents
    # that have advice, so that forward, the left and the right turn all occur at either nd
    pos = (tiles + off).astype(env.T)
    inc = env.cfg.position_increment_wu_f64 if env.T is np.float64 else env.cfg.position_increment_wu
    _, wanted = GR.expected(fields, pos, np.zeros(B, np.int64), env.world.directions_wu, inc, env.T)
    dirs, advised = rng.integers(0, nd, B), np.flatnonzero(wanted >= 0)
    dirs[advised] = (wanted[advised] + np.arange(len(advised)) % 3 - 1) % nd
    env.set_state(goal, pos, dirs)
    SR.feed(env, "goal_distance.field", fields)
    np.testing.assert_array_equal(env.goal_distance_field, fields)                # the kernel read THIS field
    np.testing.assert_array_equal(np.floor(env.world.player_position_wu).astype(np.int64), tiles)
    t = GR.Tracked(env, enable=False)                                             # (its first check: both words against the rule)
    action, heading = t.check("behind the restore")
    # what the batch held, from the inputs and the reference
    own, match = zip(*[first_match(fields[b], tiles[b]) for b in range(B)])
    own, none = np.array(own), np.array([m is None for m in match])
    np.testing.assert_array_equal(heading < 0, none)
    assert (none & (own != 0) & (own != X)).sum() > 0                             # no nearer neighbour on a field with a value: "no flood's field"
    assert none[[0, 2, 4]].all() and none[1] and own[3] == 0xFFFE and match[3] == 3 and list(match[5:9]) == [0, 1, 2, 3]
    assert all(sum(m == k for m in match) > 0 for k in range(4))
    assert (action[none] == 3).all() and all((action == a).sum() > 0 for a in (1, 3, 4)), np.bincount(action)
    # one step: the agents whose episode goes on keep the hand-made field
    episode = env.world.episode.copy()
    rcw.act_(env, rng.integers(1, 5, B).astype(np.uint8))
    t.check("a step behind the restore")
    same = env.world.episode == episode
    assert same.sum() > B // 2
    np.testing.assert_array_equal(env.goal_distance_field[same], fields[same])
    env.close()
