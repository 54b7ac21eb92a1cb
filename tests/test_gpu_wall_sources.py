"""The four sources of wall layouts — the wall bank, and the wall generator's mazes, caves and rooms — beside one another (include/rcw.h:
rcw_set_wall_bank, rcw_set_wall_generator, rcw_set_wall_caves, rcw_set_wall_rooms; rcw_set_walls is the fifth setter).  A handle has at
most one of them live.  One table-driven test, a case per live source, 8 x 8 tiles, 4 agents, a time limit of 5, one step taken so that no
array is all zero:

  * every setter that would install something else is refused: RCW_ERR_UNSUPPORTED, the whole text of rcw_last_error as TEXTS has it,
    and the engine byte for byte what it was (STATE: frames, descriptors, tile map, goals, poses, rewards, counters, status, the time
    limit's words, wall_layout and its device pointer, the four *_info);
  * every other source's off call returns RCW_OK and changes none of that;
  * the live source installed again with other parameters: the counters move by exactly one, *_info shows the new values, every
    agent's layout is connected;
  * the live source switched off: walls and counters stay, rcw_wall_layout is refused, set_walls works again.

TEXTS is a copy of the sixteen refusal texts as the library's source spelt them out, one line a pair, before the refusal became one
function over a table: this test passed unchanged on that build.  It reads no assembly and provokes no fault.
"""
import ctypes as C

import numpy as np
import pytest

import wall_bank_cases as BC

pytestmark = pytest.mark.gpu
CASE = dict(B=4, H=8, W=8, N=16, Hc=24, seed=11)

BANK = "the handle draws its walls from a wall bank; switch the bank off first (rcw_set_wall_bank(h, NULL, 0, NULL))"
TEXTS = {   # (live source, refused setter) -> rcw_last_error
    ("bank", "set_walls"): "rcw_set_walls: " + BANK,
    ("bank", "set_wall_generator"): "rcw_set_wall_generator: " + BANK,
    ("bank", "set_wall_caves"): "rcw_set_wall_caves: " + BANK,
    ("bank", "set_wall_rooms"): "rcw_set_wall_rooms: " + BANK,
    ("mazes", "set_walls"): "rcw_set_walls: the handle makes its walls with the wall generator; switch the generator off first (rcw_set_wall_generator(h, 0, ...))",
    ("mazes", "set_wall_bank"): "rcw_set_wall_bank: the handle makes its walls with the wall generator; switch the generator off first (rcw_set_wall_generator(h, 0, ...))",
    ("mazes", "set_wall_caves"): "rcw_set_wall_caves: the handle makes mazes; switch the generator off first (rcw_set_wall_generator(h, 0, ...))",
    ("mazes", "set_wall_rooms"): "rcw_set_wall_rooms: the handle makes mazes; switch the generator off first (rcw_set_wall_generator(h, 0, ...))",
    ("caves", "set_walls"): "rcw_set_walls: the handle makes its walls with the wall generator's caves; switch them off first (rcw_set_wall_caves(h, 0, ...))",
    ("caves", "set_wall_bank"): "rcw_set_wall_bank: the handle makes its walls with the wall generator's caves; switch them off first (rcw_set_wall_caves(h, 0, ...))",
    ("caves", "set_wall_generator"): "rcw_set_wall_generator: the handle makes caves; switch them off first (rcw_set_wall_caves(h, 0, ...))",
    ("caves", "set_wall_rooms"): "rcw_set_wall_rooms: the handle makes caves; switch them off first (rcw_set_wall_caves(h, 0, ...))",
    ("rooms", "set_walls"): "rcw_set_walls: the handle makes its walls with the wall generator's rooms; switch them off first (rcw_set_wall_rooms(h, 0, ...))",
    ("rooms", "set_wall_bank"): "rcw_set_wall_bank: the handle makes its walls with the wall generator's rooms; switch them off first (rcw_set_wall_rooms(h, 0, ...))",
    ("rooms", "set_wall_generator"): "rcw_set_wall_generator: the handle makes rooms; switch them off first (rcw_set_wall_rooms(h, 0, ...))",
    ("rooms", "set_wall_caves"): "rcw_set_wall_caves: the handle makes rooms; switch them off first (rcw_set_wall_rooms(h, 0, ...))",
}

NO_BANK = dict(layouts=0, total_weight=0)
NO_GEN = dict(enabled=False, loops=0, levels=0, first_level=0, level_seed=0)
NO_CAVES = dict(enabled=False, fill=0, smooth=0)
NO_ROOMS = dict(enabled=False, room=0, stop=0, doors=0)


def word(p):
    return min(int(p * 2 ** 32), 2 ** 32 - 1)


def sources():
    """name -> (its setter, the arguments of the install, the arguments of the second install, the four *_info behind each)"""
    bank = BC.three_layouts(CASE["H"], CASE["W"])
    return {
        "bank": ("set_wall_bank", (bank, [1, 2, 3]), (bank[::-1][:2], [5, 1]),
                 (dict(layouts=3, total_weight=6), NO_GEN, NO_CAVES, NO_ROOMS), (dict(layouts=2, total_weight=6), NO_GEN, NO_CAVES, NO_ROOMS)),
        "mazes": ("set_wall_generator", (0.25, 3, 2, 9), (0.5, 0, 0, 0),
                  (NO_BANK, dict(enabled=True, loops=word(0.25), levels=3, first_level=2, level_seed=9), NO_CAVES, NO_ROOMS),
                  (NO_BANK, dict(enabled=True, loops=word(0.5), levels=0, first_level=0, level_seed=0), NO_CAVES, NO_ROOMS)),
        "caves": ("set_wall_caves", (0.4, 2, 3, 2, 9), (0.3, 1, 0, 0, 0),
                  (NO_BANK, dict(enabled=True, loops=0, levels=3, first_level=2, level_seed=9), dict(enabled=True, fill=word(0.4), smooth=2), NO_ROOMS),
                  (NO_BANK, dict(enabled=True, loops=0, levels=0, first_level=0, level_seed=0), dict(enabled=True, fill=word(0.3), smooth=1), NO_ROOMS)),
        "rooms": ("set_wall_rooms", (2, 0.25, 0.25, 3, 2, 9), (1, 0.0, 0.5, 0, 0, 0),
                  (NO_BANK, dict(enabled=True, loops=0, levels=3, first_level=2, level_seed=9), NO_CAVES, dict(enabled=True, room=2, stop=word(0.25), doors=word(0.25))),
                  (NO_BANK, dict(enabled=True, loops=0, levels=0, first_level=0, level_seed=0), NO_CAVES, dict(enabled=True, room=1, stop=0, doors=word(0.5)))),
    }


def infos(env):
    return env.wall_bank_info, env.wall_generator_info, env.wall_caves_info, env.wall_rooms_info


def state(env):
    w = env.world
    h, c = env.columns()
    return dict(frame=env.camera_view_host(), col_h=h, col_c=c, tile_map=w.tile_map_chunks, goal=w.goal_position, position=w.player_position_wu,
                heading=w.player_direction_au, reward=w.reward, done=w.done, episode=w.episode, status=w.status, episode_steps=w.episode_steps,
                truncated=w.truncated, wall_layout=env.wall_layout.numpy(), wall_layout_ptr=np.array([env.wall_layout.ptr], np.uint64))


def unchanged(env, before, info, what):
    after = state(env)
    assert set(after) == set(before), what
    for k in before:
        np.testing.assert_array_equal(after[k], before[k], err_msg=f"{k} behind {what}")
    assert infos(env) == info, what


@pytest.mark.parametrize("live", ["bank", "mazes", "caves", "rooms"])
def test_one_live_source_and_the_other_setters(rcw, live):
    from raycastworlds_jl_amd import _capi

    L, B = rcw.layouts, CASE["B"]
    table = sources()
    setter, first, second, info_first, info_second = table[live]
    env = BC.make_env(rcw, CASE, max_episode_steps=5)
    assert infos(env) == (NO_BANK, NO_GEN, NO_CAVES, NO_ROOMS)
    getattr(env, setter)(*first)
    rcw.act_(env, np.full(B, 1, np.uint8))
    assert infos(env) == info_first
    before, info = state(env), infos(env)
    assert before["episode"].all() and before["episode_steps"].all() and before["wall_layout_ptr"][0] != 0

    # 1  every setter that would install something else
    ring = L.ring(CASE["H"], CASE["W"])
    others = {"set_walls": (ring,)}
    others.update({table[k][0]: table[k][1] for k in table if k != live})
    assert len(others) == 4
    for name, args in others.items():
        with pytest.raises(_capi.RcwError) as ei:
            getattr(env, name)(*args)
        print(f"{live} live, {name}: {ei.value.code} {ei.value.message!r}")
        assert ei.value.code == _capi.RCW_ERR_UNSUPPORTED, (live, name)
        assert ei.value.message == TEXTS[live, name] and _capi.last_error(env._lib) == TEXTS[live, name]
        unchanged(env, before, info, f"{name} refused beside the {live}")

    # 2  every other source's off call
    for k in table:
        if k != live:
            getattr(env, table[k][0])(None)                                  # (raises on anything but RCW_OK)
            unchanged(env, before, info, f"{table[k][0]}(None) beside the {live}")

    # 3  the live source once more, with other parameters
    getattr(env, setter)(*second)
    np.testing.assert_array_equal(env.world.episode, before["episode"] + 1)
    assert infos(env) == info_second
    walls = env.world.walls
    assert all(L.is_connected(w) for w in walls)
    layout = env.wall_layout.numpy()
    if live == "bank":
        assert set(layout.tolist()) <= {0, 1}
        for a in range(B):
            np.testing.assert_array_equal(walls[a], second[0][layout[a]])
    else:
        assert (layout == -1).all()
    rcw.act_(env, np.full(B, 2, np.uint8))

    # 4  ... and switched off
    walls, episode = env.world.walls, env.world.episode
    getattr(env, setter)(None)
    assert infos(env) == (NO_BANK, NO_GEN, NO_CAVES, NO_ROOMS)
    np.testing.assert_array_equal(env.world.walls, walls)
    np.testing.assert_array_equal(env.world.episode, episode)
    out, p = np.zeros(B, np.int32), C.c_void_p()
    assert env._lib.rcw_wall_layout(env._h, out.ctypes.data_as(C.c_void_p)) == _capi.RCW_ERR_UNSUPPORTED
    assert env._lib.rcw_wall_layout_device_ptr(env._h, C.byref(p)) == _capi.RCW_ERR_UNSUPPORTED
    pillars = table["bank"][1][0][1]
    env.set_walls(pillars)
    np.testing.assert_array_equal(env.world.walls, np.broadcast_to(pillars, (B,) + pillars.shape))
    np.testing.assert_array_equal(env.world.episode, episode + 1)
    rcw.act_(env, np.full(B, 1, np.uint8))
    env.close()
