"""The episode time limit on the CPU (include/rcw.h, rcw_set_time_limit): the reference composition of tests/time_limit_ref.py against
rows written out by hand for one agent, the six exports in the header, the binding and the library, and what rcw_set_time_limit does to
the facts of a step (the development build's StepFacts without a device)."""
import ctypes as C
import os
import re

import numpy as np

import time_limit_ref as TL
from test_step_state import PRIME, ONE, Handle, devlib, row   # noqa: F401  (devlib: the development build, a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = {"rcw_set_time_limit": 2, "rcw_time_limit": 2, "rcw_episode_steps": 2, "rcw_truncated": 2, "rcw_episode_steps_device_ptr": 2,
           "rcw_truncated_device_ptr": 2}
FORWARD, BACKWARD, LEFT, RIGHT = 1, 2, 3, 4


def world(oracle, limit, goal, auto_reset=1, batch=1, out_of_bounds=1, seed=5):
    """`batch` agents of a 4 x 4 room (interior tiles (2..3, 2..3)) at the centre of tile (2, 2), heading 0 = +x, a quarter tile a move:
    forward once is free (x = 1.75); forward twice touches tile (3, 2) — the goal there ends the episode, a free tile lets the agent in."""
    orc = oracle.OracleBatch(batch, seed=seed, render=False, height_tile_map_tu=4, width_tile_map_tu=4, num_rays=8, height_camera_view_pu=8,
                             num_directions=4, auto_reset=auto_reset, out_of_bounds=out_of_bounds, position_increment_wu=0.25,
                             position_increment_wu_f64=0.25)
    orc.set_state(np.tile(np.array(goal, np.int32), (batch, 1)), np.full((batch, 2), 1.5, np.float32), np.zeros(batch, np.int32))
    return orc, TL.TimeLimitRef(orc, limit, seed, auto_reset)


def words(ref):
    return ref.episode_steps.tolist(), ref.truncated.tolist(), ref.orc.done.tolist()


def test_two_steps_reach_a_limit_of_two(oracle):
    orc, ref = world(oracle, 2, goal=(3, 3))
    assert words(ref) == ([0], [0], [0])
    ref.step([FORWARD])
    assert words(ref) == ([1], [0], [0]) and orc.position[0].tolist() == [1.75, 1.5]
    ref.step([FORWARD])
    assert words(ref) == ([2], [1], [0]) and orc.position[0].tolist() == [2.0, 1.5]
    assert ref.events["truncations"] == 1 and ref.events["terminations"] == 0


def test_a_truncated_agent_restarts_with_its_action_ignored(oracle):
    orc, ref = world(oracle, 2, goal=(3, 3))
    ref.step([LEFT]); ref.step([LEFT])                                       # a turn counts like any step
    assert words(ref) == ([2], [1], [0]) and orc.direction.tolist() == [2] and orc.episode.tolist() == [1]
    twin = oracle.OracleBatch(1, seed=5, render=False, config=orc.cfg)       # what reset!(world) draws for (seed, agent 0, episode 1)
    twin.set_state(orc.goal.copy(), orc.position.copy(), orc.direction.copy())
    twin.reset(seed=5)
    ref.step([FORWARD])                                                      # ... is what the restart leaves: nothing moved forward
    assert words(ref) == ([0], [0], [0]) and orc.episode.tolist() == [2] and orc.reward.tolist() == [0.0]
    assert orc.position.tolist() == twin.position.tolist() and orc.direction.tolist() == twin.direction.tolist() and orc.goal.tolist() == twin.goal.tolist()
    assert ref.events["restarts_after_truncation"] == 1
    ref.step([LEFT])                                                         # the new episode counts from zero
    assert words(ref)[:2] == ([1], [0])


def test_the_goal_on_the_limit_step_terminates_and_does_not_truncate(oracle):
    orc, ref = world(oracle, 2, goal=(3, 2))
    ref.step([FORWARD]); ref.step([FORWARD])
    assert words(ref) == ([2], [0], [1]) and orc.reward.tolist() == [1.0] and orc.position[0].tolist() == [1.75, 1.5]
    assert ref.events["on_the_limit_step"] == 1 and ref.events["truncations"] == 0 and ref.events["terminations"] == 1
    ref.step([FORWARD])                                                      # the restart of a done agent clears the words too
    assert words(ref) == ([0], [0], [0]) and ref.events["restarts_after_done"] == 1


def test_an_invalid_action_changes_nothing(oracle):
    orc, ref = world(oracle, 2, goal=(3, 3))
    ref.step([FORWARD])
    for bad in (0, 5, 255):
        ref.step([bad])
        assert words(ref) == ([1], [0], [0]) and orc.position[0].tolist() == [1.75, 1.5]
    ref.step([FORWARD])
    assert words(ref) == ([2], [1], [0])
    ep = orc.episode.tolist()
    ref.step([0])                                                            # not stepped, so not restarted either
    assert words(ref) == ([2], [1], [0]) and orc.episode.tolist() == ep and ref.events["invalid_while_truncated"] == 1


def test_a_raising_move_leaves_the_words(oracle):
    """out_of_bounds = 0 (RCW_OOB_ERROR): from x = 2.875 the forward move tests x = 3.125, whose neighbourhood leaves the 4 x 4 map —
    BoundsError in the reference: the agent is left exactly as it was, the two words with it."""
    orc, ref = world(oracle, 3, goal=(2, 3), out_of_bounds=0)
    orc.set_state(orc.goal.copy(), np.array([[2.875, 1.5]], np.float32), orc.direction.copy())
    ref.step([LEFT]); ref.step([RIGHT])
    assert words(ref) == ([2], [0], [0])
    ref.step([FORWARD])
    assert orc.status.tolist() == [TL.RCW_ERR_OUT_OF_BOUNDS] and orc.position[0].tolist() == [2.875, 1.5]
    assert words(ref) == ([2], [0], [0]) and ref.events["raised_with_words_kept"] == 1
    ref.step([LEFT])
    assert words(ref) == ([3], [1], [0]) and ref.events["raised_with_words_kept"] == 1


def test_a_masked_reset_zeroes_the_masked_agents_words(oracle):
    orc, ref = world(oracle, 2, goal=(3, 3), batch=2)
    ref.step([LEFT, LEFT]); ref.step([LEFT, LEFT])
    assert words(ref)[:2] == ([2, 2], [1, 1])
    mask = np.array([0, 1], np.uint8)
    orc.reset(mask=mask, seed=5); ref.clear(mask)
    assert words(ref)[:2] == ([2, 0], [1, 0])


def test_without_auto_reset_the_counter_keeps_counting(oracle):
    orc, ref = world(oracle, 2, goal=(3, 2), auto_reset=0)
    seen = []
    for a in (LEFT, RIGHT, LEFT, RIGHT, FORWARD, FORWARD, LEFT):
        ref.step([a])
        seen.append(words(ref))
    # nothing restarts: the flag is recomputed by every step, and the goal (step 6) takes it back, as `done` itself is recomputed (step 7)
    assert seen == [([1], [0], [0]), ([2], [1], [0]), ([3], [1], [0]), ([4], [1], [0]), ([5], [1], [0]), ([6], [0], [1]), ([7], [1], [0])]
    assert orc.episode.tolist() == [1] and ref.events["restarts_after_truncation"] == 0 and ref.events["on_the_limit_step"] == 0


def test_no_limit_is_the_oracle_alone(oracle):
    orc, ref = world(oracle, 0, goal=(3, 2))
    plain = oracle.OracleBatch(1, seed=5, render=False, config=orc.cfg)
    plain.set_state(orc.goal.copy(), orc.position.copy(), orc.direction.copy())
    for a in (FORWARD, FORWARD, LEFT, 0, FORWARD):
        ref.step([a]); plain.step_lenient(np.array([a], np.uint8))
        assert words(ref)[:2] == ([0], [0])
        assert orc.position.tolist() == plain.position.tolist() and orc.done.tolist() == plain.done.tolist() and orc.episode.tolist() == plain.episode.tolist()


def test_the_header_the_bindings_and_the_library_carry_the_six_exports(rcw):
    from raycastworlds_jl_amd import _capi

    text = open(os.path.join(ROOT, "include", "rcw.h")).read()
    assert re.search(r"#define\s+RCW_ABI_VERSION\s+4\b", text) and _capi.RCW_ABI_VERSION == 4      # additive: the version stays
    assert re.search(r"RCW_API\s+int\s+rcw_set_time_limit\s*\(\s*rcw_handle\*\s*h\s*,\s*int32_t\s+max_episode_steps\s*\)", text)
    assert re.search(r"RCW_API\s+int\s+rcw_time_limit\s*\(\s*rcw_handle\*\s*h\s*,\s*int32_t\*\s*out\s*\)", text)
    assert re.search(r"RCW_API\s+int\s+rcw_episode_steps\s*\(\s*rcw_handle\*\s*h\s*,\s*uint32_t\*\s*out_host", text)
    assert re.search(r"RCW_API\s+int\s+rcw_truncated\s*\(\s*rcw_handle\*\s*h\s*,\s*uint8_t\*\s*out_host", text)
    assert re.search(r"RCW_API\s+int\s+rcw_episode_steps_device_ptr\s*\(\s*rcw_handle\*\s*h\s*,\s*void\*\*\s*device_ptr\s*\)", text)
    assert re.search(r"RCW_API\s+int\s+rcw_truncated_device_ptr\s*\(\s*rcw_handle\*\s*h\s*,\s*void\*\*\s*device_ptr\s*\)", text)
    jl = open(os.path.join(ROOT, "julia", "BatchedSingleRoom.jl")).read()
    lib = _capi.load()
    for name, arity in EXPORTS.items():
        assert len(_capi.SIGNATURES[name]) == arity, name
        assert re.search(r"ccall\(\(:" + name + r",\s*librcw\)", jl), name
        assert hasattr(lib, name), name
    env = rcw.SingleRoomModule.SingleRoom
    assert callable(env.set_time_limit) and isinstance(env.time_limit, property) and callable(env.truncated_device) and callable(env.episode_steps_device)
    assert callable(rcw.RLBase.is_truncated)


def test_a_null_handle_and_a_null_output_are_refused(rcw):
    from raycastworlds_jl_amd import _capi

    lib = _capi.load()
    out = C.c_int32(7)
    for call in (lambda: lib.rcw_set_time_limit(None, 5), lambda: lib.rcw_time_limit(None, C.byref(out)), lambda: lib.rcw_episode_steps(None, None),
                 lambda: lib.rcw_truncated(None, None), lambda: lib.rcw_episode_steps_device_ptr(None, None), lambda: lib.rcw_truncated_device_ptr(None, None)):
        assert call() == _capi.RCW_ERR_INVALID_ARGUMENT and _capi.last_error(lib)
    assert out.value == 7


def test_setting_the_limit_makes_the_one_launch_step_cast_its_slots_again(devlib):
    """rcw_set_time_limit is event 8 of the development build's StepFacts: the slots were cast under the old limit, so the next step takes the
    priming path (its own casting launch, with the actions), stores every frame, and the one behind it is one launch again.  No fact is
    added, the form does not change, and a two-launch handle notices nothing."""
    h = Handle(devlib)
    h.create()
    assert h.step() == row(on=1, primed=1, obs_current=1, cur=1, cols_stale=1, path=ONE, keep=1)
    assert h.event(8) == row(on=1, primed=0, obs_current=0, cur=1, cols_stale=1)
    assert h.step() == row(on=1, primed=1, obs_current=1, cur=1, path=PRIME)
    assert h.step() == row(on=1, primed=1, obs_current=1, cur=0, cols_stale=1, path=ONE, keep=1)
    g = Handle(devlib, eligible=0)
    g.create()
    before = g.step()
    assert g.event(8) == before._replace(path=-1) and g.step() == before
