"""The facts of a step (csrc/rcw_handle.h, StepFacts): which launches a step of a handle makes, and whether the one-launch step may leave
the frame of an agent whose view it does not change as it is (`keep`).  A wrong fact does not crash: it leaves stale frames in the
observation batch, so the transitions are pinned here, on the CPU.  The development build drives a StepFacts through a list of events
without a device (rcw_dev_step_facts); the helpers below put the events together as the entry points of include/rcw.h do, and every
expected row is written out by hand from those words — nothing here is computed from the library's answers.

A row: on, want, captured, primed, obs_current, cur, cols_live, cols_stale, store_all | path, keep | refused.
"""
import ctypes as C
import os
from collections import namedtuple

import pytest

Row = namedtuple("Row", "on want captured primed obs_current cur cols_live cols_stale store_all path keep refused")
TWO, ONE, PRIME = 0, 1, 2                       # StepFacts::Path
FORM_TWO, FORM_ONE = 1, 2                       # RCW_STEP_TWO_LAUNCHES, RCW_STEP_ONE_LAUNCH
ACT, MASK, CAPTURING, FAILS, FILL_FAILS = 1, 2, 4, 8, 16


def row(on=0, want=0, captured=0, primed=0, obs_current=0, cur=0, cols_live=0, cols_stale=0, store_all=0, path=-1, keep=0, refused=0):
    return Row(on, want, captured, primed, obs_current, cur, cols_live, cols_stale, store_all, path, keep, refused)


@pytest.fixture(scope="module")
def devlib(rcw):
    from raycastworlds_jl_amd import _capi

    if not os.path.exists(_capi.DEV_LIB_PATH):
        from raycastworlds_jl_amd import build as _build

        _build.build()
    lib = C.CDLL(_capi.DEV_LIB_PATH)
    lib.rcw_dev_step_facts.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32)]
    lib.rcw_dev_step_facts.restype = C.c_int
    return lib


class Handle:
    """The events a handle has seen so far; every call replays them all (the export starts from a fresh StepFacts) and returns the
    row behind the last one."""

    def __init__(self, lib, eligible=1, pays=1, store_all=0):
        self.lib, self.args, self.events = lib, (eligible, pays, store_all), []

    def last(self):
        n = len(self.events)
        ev = (C.c_int32 * (3 * n))(*[x for e in self.events for x in e])
        out = (C.c_int32 * (12 * n))()
        assert self.lib.rcw_dev_step_facts(*self.args, ev, n, out) == n
        return Row(*out[12 * (n - 1):12 * n])

    def event(self, kind, a=0, b=0):
        self.events.append((kind, a, b))
        return self.last()

    # the entry points, as include/rcw.h words them
    def plan(self, want, view_only=0):          # plan_step_form alone
        return self.event(0, want, view_only)

    def camera(self, flags=0):                  # launch_step_camera alone
        return self.event(1, flags)

    def create(self):                           # rcw_create: the form by the rule, then rcw_reset of every agent with the handle's seed
        self.plan(0)
        return self.reset()

    def step(self, flags=0):                    # rcw_step / rcw_step_device
        return self.camera(ACT | flags)

    def reset(self, mask=0, new_seed=0, auto_reset=0):   # rcw_reset: the state kernel, then the render without an action
        self.event(4, (1 if mask else 0) | (2 if new_seed else 0) | (4 if auto_reset else 0))
        return self.camera(MASK if mask else 0)

    def set_step_form(self, form):              # rcw_set_step_form: a form that comes on is primed by a render without an action
        was_on = self.last().on
        r = self.plan(form)
        return self.camera() if r.on and not was_on else r

    def view_only_step(self, flags=0):
        return self.event(2, flags)

    def bind_obs(self):
        return self.event(3)

    def read_columns(self):                     # rcw_cast_rays; rcw_columns, the gathers (ensure_columns)
        return self.event(5)

    def columns_device_ptr(self):               # ... and a learner view switched on
        return self.event(6)

    def update_camera_view(self):
        return self.event(7)


def test_a_created_handle_primes_and_then_steps_in_one_launch(devlib):
    h = Handle(devlib)
    assert h.plan(0) == row(on=1)
    # rcw_create's reset is the handle's first camera render: the casting halves alone, then the fill — slots primed, buffer current
    assert h.reset() == row(on=1, primed=1, obs_current=1, path=PRIME)
    # every step from then on is one launch that may skip; the slot buffers alternate; nobody holds the descriptors, so they go stale
    assert h.step() == row(on=1, primed=1, obs_current=1, cur=1, cols_stale=1, path=ONE, keep=1)
    assert h.step() == row(on=1, primed=1, obs_current=1, cur=0, cols_stale=1, path=ONE, keep=1)
    # a first STEP on slots nobody primed takes the priming path with its actions; the one behind it is one launch
    g = Handle(devlib)
    g.plan(0)
    assert g.step() == row(on=1, primed=1, obs_current=1, path=PRIME)
    assert g.step() == row(on=1, primed=1, obs_current=1, cur=1, cols_stale=1, path=ONE, keep=1)


def test_a_masked_reset_keeps_the_buffer_current_only_if_it_was(devlib):
    h = Handle(devlib)
    h.create()
    h.step()
    # same seed: the masked agents' slots are rewritten in place and exactly they are repainted; the others' descriptors stay stale
    assert h.reset(mask=1) == row(on=1, primed=1, obs_current=1, cur=1, cols_stale=1, path=PRIME)
    assert h.step() == row(on=1, primed=1, obs_current=1, cur=0, cols_stale=1, path=ONE, keep=1)
    # ... not current before (the caller rebound the buffer): repainting the masked agents does not make it so
    h.bind_obs()
    assert h.reset(mask=1) == row(on=1, primed=1, obs_current=0, cur=0, cols_stale=1, path=PRIME)
    assert h.step() == row(on=1, primed=1, obs_current=1, cur=1, cols_stale=1, path=ONE, keep=0)


def test_a_masked_reset_with_a_new_seed_under_auto_reset_forgets_the_slots(devlib):
    h = Handle(devlib)
    h.create()
    h.step()
    assert h.reset(mask=1, new_seed=1, auto_reset=1) == row(on=1, primed=0, obs_current=0, cur=1, cols_stale=1, path=PRIME)
    assert h.step() == row(on=1, primed=1, obs_current=1, cur=1, cols_stale=0, path=PRIME)          # every agent's slots cast again
    assert h.step() == row(on=1, primed=1, obs_current=1, cur=0, cols_stale=1, path=ONE, keep=1)
    # without auto_reset nothing was drawn ahead with the old seed; without a mask every slot is cast again anyway
    g = Handle(devlib)
    g.create()
    assert g.reset(mask=1, new_seed=1, auto_reset=0) == row(on=1, primed=1, obs_current=1, path=PRIME)
    assert g.reset(mask=0, new_seed=1, auto_reset=1) == row(on=1, primed=1, obs_current=1, path=PRIME)
    assert g.step() == row(on=1, primed=1, obs_current=1, cur=1, cols_stale=1, path=ONE, keep=1)


def test_bind_obs_makes_the_next_step_store_every_frame(devlib):
    h = Handle(devlib)
    h.create()
    assert h.bind_obs() == row(on=1, primed=1, obs_current=0)
    assert h.step() == row(on=1, primed=1, obs_current=1, cur=1, cols_stale=1, path=ONE, keep=0)
    assert h.step() == row(on=1, primed=1, obs_current=1, cur=0, cols_stale=1, path=ONE, keep=1)


def test_update_camera_view_behind_bind_obs_restores_the_skip(devlib):
    h = Handle(devlib)
    h.create()
    h.step()
    h.bind_obs()
    # it reads the descriptors (recast: no longer stale) and paints every agent's current frame, which is what slot 0 holds
    assert h.update_camera_view() == row(on=1, primed=1, obs_current=1, cur=1, cols_stale=0)
    assert h.step() == row(on=1, primed=1, obs_current=1, cur=0, cols_stale=1, path=ONE, keep=1)
    # on a handle of the two-launch form it paints, and no fact comes back
    g = Handle(devlib, pays=0)
    g.create()
    assert g.update_camera_view() == row()


def test_a_captured_step_keeps_two_launches_until_one_launch_is_asked_for(devlib):
    h = Handle(devlib)
    h.create()
    assert h.step(CAPTURING) == row(on=0, captured=1, path=TWO)
    assert h.step() == row(on=0, captured=1, path=TWO)
    assert h.set_step_form(0) == row(on=0, captured=1)                                   # the rule does not turn it on again
    assert h.plan(FORM_ONE) == row(on=1, want=FORM_ONE)                                  # the caller does, and captured is cleared
    assert h.step() == row(on=1, want=FORM_ONE, primed=1, obs_current=1, path=PRIME)     # the next step primes
    assert h.step() == row(on=1, want=FORM_ONE, primed=1, obs_current=1, cur=1, cols_stale=1, path=ONE, keep=1)
    # a two-launch handle asks nobody whether its stream is capturing: captured stays clear
    g = Handle(devlib, pays=0)
    g.create()
    assert g.step(CAPTURING) == row(path=TWO)


def test_a_change_of_form_forgets_both_ways(devlib):
    h = Handle(devlib)
    h.create()
    h.step()
    assert h.set_step_form(FORM_TWO) == row(on=0, want=FORM_TWO, cur=1, cols_stale=1)
    # (the two-launch step writes the descriptors and still leaves cols_stale: a later reader recasts once more than it must)
    assert h.step() == row(on=0, want=FORM_TWO, cur=1, cols_stale=1, path=TWO)
    assert h.plan(0) == row(on=1, cur=1, cols_stale=1)
    assert h.camera() == row(on=1, primed=1, obs_current=1, cur=1, path=PRIME)           # rcw_set_step_form's priming render
    # the same form asked for again changes nothing
    assert h.set_step_form(0) == row(on=1, primed=1, obs_current=1, cur=1)
    assert h.set_step_form(FORM_ONE) == row(on=1, want=FORM_ONE, primed=1, obs_current=1, cur=1)


def test_the_descriptors_go_stale_unless_a_caller_holds_them(devlib):
    h = Handle(devlib)
    h.create()
    assert h.step().cols_stale == 1
    assert h.read_columns() == row(on=1, primed=1, obs_current=1, cur=1, cols_stale=0)
    assert h.step() == row(on=1, primed=1, obs_current=1, cur=0, cols_stale=1, path=ONE, keep=1)
    assert h.columns_device_ptr() == row(on=1, primed=1, obs_current=1, cur=0, cols_live=1, cols_stale=0)
    assert h.step() == row(on=1, primed=1, obs_current=1, cur=1, cols_live=1, cols_stale=0, path=ONE, keep=1)
    assert h.step() == row(on=1, primed=1, obs_current=1, cur=0, cols_live=1, cols_stale=0, path=ONE, keep=1)


def test_store_all_never_keeps_while_the_buffer_stays_current(devlib):
    h = Handle(devlib, store_all=1)
    assert h.create() == row(on=1, primed=1, obs_current=1, store_all=1, path=PRIME)
    assert h.step() == row(on=1, primed=1, obs_current=1, cur=1, cols_stale=1, store_all=1, path=ONE, keep=0)
    assert h.step() == row(on=1, primed=1, obs_current=1, cur=0, cols_stale=1, store_all=1, path=ONE, keep=0)


def test_view_only_takes_two_launches_and_refuses_one(devlib):
    h = Handle(devlib)
    h.create()
    # rcw_set_learner_view(..., RCW_VIEW_ONLY): the view kernel reads the descriptors, then the step's form is planned again
    h.columns_device_ptr()
    assert h.plan(0, view_only=1) == row(on=0, cols_live=1)
    assert h.plan(FORM_ONE, view_only=1) == row(on=0, cols_live=1, refused=1)            # refused, and nothing changed
    assert h.view_only_step(ACT) == row(on=0, cols_live=1)
    assert h.update_camera_view() == row(on=0, cols_live=1)                              # painted on demand; the form is off: not "current"
    # view-only off again: the form goes by the rule, and nobody has primed it
    assert h.plan(0) == row(on=1, cols_live=1)
    assert h.step() == row(on=1, primed=1, obs_current=1, cols_live=1, path=PRIME)
    # the view-only step paints no camera view, whatever the facts were: obs_current goes; with a mask the descriptors stay as stale as they were
    g = Handle(devlib)
    g.create()
    g.step()
    assert g.view_only_step(ACT | MASK) == row(on=1, primed=1, obs_current=0, cur=1, cols_stale=1)
    assert g.view_only_step(ACT) == row(on=1, primed=1, obs_current=0, cur=1, cols_stale=0)
    # a request for one launch that the view-only handle remembered from before is refused without touching anything either
    k = Handle(devlib)
    k.plan(FORM_ONE)
    assert k.plan(FORM_ONE, view_only=1) == row(on=1, want=FORM_ONE, refused=1)


def test_an_ineligible_handle_keeps_two_launches(devlib):
    h = Handle(devlib, eligible=0)
    assert h.create() == row(path=TWO)
    assert h.set_step_form(FORM_ONE) == row(refused=1)
    assert h.step() == row(path=TWO)
    assert h.set_step_form(FORM_TWO) == row(want=FORM_TWO)
    # eligible, but the batch too small for it to pay: the rule keeps two launches, the caller may still ask for one
    g = Handle(devlib, pays=0)
    assert g.create() == row(path=TWO)
    assert g.plan(FORM_ONE) == row(on=1, want=FORM_ONE)
    assert g.plan(0) == row(on=0)


def test_a_failed_step_leaves_the_buffer_not_current(devlib):
    h = Handle(devlib)
    h.create()
    # the one launch was chosen, with the skip — and did not go out: nothing comes back, the slot buffers keep their places
    assert h.step(FAILS) == row(on=1, primed=1, obs_current=0, cur=0, path=ONE, keep=1)
    assert h.step() == row(on=1, primed=1, obs_current=1, cur=1, cols_stale=1, path=ONE, keep=0)
    # the priming path: a casting launch that failed primes nothing; one whose fill failed has primed the slots, but the buffer is not current
    g = Handle(devlib)
    g.plan(0)
    assert g.camera(FAILS) == row(on=1, path=PRIME)
    assert g.camera(FILL_FAILS) == row(on=1, primed=1, obs_current=0, path=PRIME)
    assert g.step() == row(on=1, primed=1, obs_current=1, cur=1, cols_stale=1, path=ONE, keep=0)


def test_an_unknown_event_is_refused(devlib):
    ev = (C.c_int32 * 3)(99, 0, 0)
    out = (C.c_int32 * 12)()
    assert devlib.rcw_dev_step_facts(1, 1, 0, ev, 1, out) < 0
    assert devlib.rcw_dev_step_facts(1, 1, 0, None, 1, out) < 0
