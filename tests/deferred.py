"""Queued calls that nobody reads between — test infrastructure, not a test.

Every other GPU test of the suite makes one call, reads the state back (rcw_sync, or a copy-out, which waits for the handle's stream) and
makes the next call.  A learner queues hundreds of calls and reads once.  This module plays the scenarios of tests/wall_bank_cases.py,
tests/wall_generator_cases.py and tests/wall_caves_cases.py the learner's way, with two more drivers beside Recorder and Player:

    Script     records the calls a scenario makes as (method, args, kwargs), and answers `state()` from the Recorder that runs beside it —
               the reference alone.  `replay(d)` makes the same calls on any driver; `actions` is every step's actions, (steps, B).
    Deferred   replays a script on an engine and reads NOTHING in between.  Behind every call it queues stream-ordered device copies of the
               handle's device-resident outputs (`x.torch(sync=False).clone()` on the engine's stream); behind the last call it synchronises
               ONCE and compares every copy, call by call, with the expected records, then the state that has no device pointer (status,
               episode, goal, pose, tile map, and last the column descriptors: rcw_columns runs ensure_columns) with the last expected one.

The expected records never come from the deferred handle.  `observed_twin` plays the same scenario on a SECOND handle through the cases'
own Player and the feature trackers — after every call against wall_bank_ref / wall_generator_ref / wall_caves_ref / TimeLimitRef and the
feature references, as tests/test_gpu_wall_bank.py does — and keeps the host copies of the watched outputs behind every call.  Where the
reference renders everything that is watched (`records_of_snapshots`, an oracle.OracleBatch) the records are the reference's own.

THE BACKLOG.  At these batch sizes a step takes the device about as long as its launches take the host, so without help the stream is
drained at nearly every call and a missing wait could not show.  Before the first stretch of the script that holds a step, `Deferred` queues
BACKLOG_FILLS fills of a BACKLOG_BYTES tensor on the engine's stream — plain torch work that ends by itself — between two events.  While
the backlog runs, everything the host queues is pending, deterministically: a later call's bytes in a pinned staging buffer WOULD overwrite a
copy that has not run yet.  WAITS says which exports may wait for the stream (INTEGRATION.md "Streams" carries the same table); where the
script holds none of them between the backlog and some call, the backlog's closing event must still be pending in front of that call.
Only the rows of ASSERTED_ON_DEVICE are held this way, by the scripts of tests/test_gpu_deferred.py; the rest is read from the code.
If it is not, the host's time since the backlog is compared with the backlog's event-measured duration: under half of it, "a call waited
for the stream"; otherwise the host was slow (a busy, shared machine), the run is repeated ONCE with four times the backlog, and the
assertion then holds or fails.  It never skips.

Measured on an MI355X (profiles/deferred_backlog.txt): (a) the host's time to queue the longest script (the bank's `calls`, 42 calls, host
actions) with no backlog is 3.04 - 3.28 ms, every other script's 1.2 - 2.6 ms; (b) the device's time for 400 fills of 1 GiB, by events, is
61.9 - 62.1 ms (0.155 ms a fill).  400 fills give (b) = 19 (a) where 4 (a) is asked, and stay far under a second.  In the tests the host
reached each pending check 0.15 - 2.9 ms behind the backlog's last record.
"""
import inspect
import re
import time

import numpy as np

# ---- the backlog ------------------------------------------------------------------------------------------------------------------------
BACKLOG_BYTES = 1 << 30                 # one fill writes 1 GiB
BACKLOG_FILLS = 400                     # 62 ms on an MI355X (profiles/deferred_backlog.txt)
BACKLOG_LIMIT_MS = 1000                 # the backlog ends by itself in under a second (the one rerun with four of them: in under four)

# ---- which exports may wait for the handle's stream (csrc/rcw_api.hip; INTEGRATION.md "Streams") -----------------------------------------
NEVER, ALWAYS = "never", "always"
RING = "the third call ahead"           # rcw_step: two pinned buffers, each behind the event of the copy that read it last
ONE_AHEAD = "the second call ahead"     # rcw_set_wall_bank_weights: one pinned buffer behind one event
MASKED = "with a mask"                  # upload_mask: the caller's pageable bytes
CELL = {NEVER: "no", ALWAYS: "yes", RING: "from the third call ahead", ONE_AHEAD: "from the second call ahead", MASKED: "with a mask"}   # the document's words
WAITS = {                               # the calls of a rollout, a row each in the document
    "rcw_step_device": NEVER, "rcw_step": RING, "rcw_reset": MASKED, "rcw_set_time_limit": NEVER, "rcw_bind_obs": NEVER,
    "rcw_set_wall_bank_weights": ONE_AHEAD, "rcw_update_camera_view": NEVER, "rcw_update_top_view": NEVER, "rcw_cast_rays": NEVER,
    "rcw_expand_columns": NEVER, "rcw_expand_columns_view": NEVER,
    "rcw_columns_device_ptr": NEVER,                                          # (queues a cast where the descriptors are stale; does not wait for it)
    "rcw_set_walls": ALWAYS, "rcw_set_state": ALWAYS, "rcw_set_state64": ALWAYS, "rcw_set_wall_bank": ALWAYS,
    "rcw_set_wall_generator": ALWAYS, "rcw_set_wall_caves": ALWAYS,           # (replace_buffers: wait_all_streams)
    "rcw_set_direction_table": ALWAYS, "rcw_set_direction_table64": ALWAYS, "rcw_set_stream": ALWAYS, "rcw_sync": ALWAYS,
    "rcw_clear_error": ALWAYS,
}
# ... and two classes, a row each: what answers from the host (no stream is touched), and the copy-outs (copy_out, sync_and_check)
HOST_ANSWERS = {"rcw_get_stream", "rcw_time_limit", "rcw_learner_view_stack"}
COPY_OUTS = {"rcw_obs_copy", "rcw_top_view_copy", "rcw_columns", "rcw_reward_typed", "rcw_done", "rcw_truncated", "rcw_episode_steps", "rcw_status",
             "rcw_episode", "rcw_goal", "rcw_position", "rcw_position64", "rcw_direction", "rcw_tile_map_chunks", "rcw_wall_layout",
             "rcw_goal_distance", "rcw_goal_distance_field", "rcw_seen_words", "rcw_seen_map", "rcw_local_map_copy", "rcw_learner_view_copy",
             "rcw_rays", "rcw_rays64"}
# the rows tests/test_gpu_deferred.py holds on the device, behind the backlog; the others are read from the code
ASSERTED_ON_DEVICE = {"rcw_step_device", "rcw_step", "rcw_reset", "rcw_set_time_limit", "rcw_bind_obs", "rcw_set_wall_bank_weights",
                      "rcw_update_camera_view", "rcw_update_top_view", "rcw_cast_rays", "rcw_expand_columns", "rcw_columns_device_ptr"}


def waits(export):
    """the rule of an export: its row, or its class's (every *_device_ptr and *_info getter answers from the host); None: the table is silent"""
    if export in WAITS:
        return WAITS[export]
    if export in HOST_ANSWERS or export.endswith("_device_ptr") or export.endswith("_info"):
        return NEVER
    return ALWAYS if export in COPY_OUTS else None


# the drivers' methods -> the functions of single_room.py they call on an engine (names: SingleRoom's methods, or the module's functions)
DRIVER_METHODS = dict(step=("act_",), reset=("reset_",), set_state=("set_state",), set_walls=("set_walls",), set_time_limit=("set_time_limit",),
                      set_wall_bank=("set_wall_bank",), set_weights=("set_wall_bank_weights",), set_wall_generator=("set_wall_generator",),
                      set_wall_caves=("set_wall_caves",))
# ... and the calls of a rollout that no scenario makes, which `Calls` scripts hold: method -> the export it is
RENDER_METHODS = dict(update_camera_view="rcw_update_camera_view", update_top_view="rcw_update_top_view", cast_rays="rcw_cast_rays",
                      bind_obs="rcw_bind_obs", columns_device="rcw_columns_device_ptr", expand_columns="rcw_expand_columns")


def exports_reached(module, names, seen=None):
    """the rcw_* exports that the functions `names` of single_room.py reach: those their source names, and those of every method, property
    or function of the module that their source refers to as `self.x`, `env.x` or `x(` — to any depth"""
    seen = set() if seen is None else seen
    out = set()
    for name in names:
        if name in seen:
            continue
        seen.add(name)
        obj = getattr(module.SingleRoom, name, None) or getattr(module, name, None)
        if isinstance(obj, property):
            obj = obj.fget
        if isinstance(obj, staticmethod):
            obj = obj.__func__
        if not inspect.isfunction(obj):
            continue
        src = inspect.getsource(obj)
        out |= set(re.findall(r"_lib\.(rcw_\w+)", src))
        refs = set(re.findall(r"(?:self|env)\.(\w+)", src)) | set(re.findall(r"\b(_?[a-z]\w+)\(", src))
        out |= exports_reached(module, sorted(refs), seen)
    return out


def may_wait(method, args, kwargs, mode, before):
    """whether call (method, args, kwargs) of a script may wait for the stream by WAITS; `before`: the calls queued since the stream was last
    known drained (the backlog), `mode` "host" or "device" actions"""
    if method == "step":
        if mode == "device":
            return WAITS["rcw_step_device"] != NEVER
        return sum(1 for m, _, _ in before if m == "step") >= 2             # RING
    if method == "reset":
        mask = args[0] if args else kwargs.get("mask")
        return mask is not None                                               # MASKED
    if method == "set_weights":
        return any(m == "set_weights" for m, _, _ in before)                   # ONE_AHEAD
    if method == "set_time_limit":
        return WAITS["rcw_set_time_limit"] != NEVER
    if method in RENDER_METHODS:
        return WAITS[RENDER_METHODS[method]] != NEVER
    return True                                                               # set_state, set_walls, set_wall_bank, set_wall_generator, set_wall_caves


def plan_backlog(calls, mode):
    """(start, check): the backlog goes in front of call `start` — the first call of the first stretch of calls that do not wait and hold a
    step — and its event must still be pending in front of call `check` (len(calls): behind the last one), the first that may wait.
    (None, None) for a script without such a stretch."""
    k = 0
    while k < len(calls):
        if may_wait(*calls[k], mode, ()):
            k += 1
            continue
        end = k
        while end < len(calls) and not may_wait(*calls[end], mode, calls[k:end]):
            end += 1
        if any(m == "step" for m, _, _ in calls[k:end]):
            return k, end
        k = end
    return None, None


# ---- the third driver: a script ------------------------------------------------------------------------------------------------------------
def _copied(x):
    return x.copy() if isinstance(x, np.ndarray) else x


class Script:
    """the calls of a scenario, recorded beside a Recorder (which answers `state()`: the reference alone)"""

    def __init__(self, recorder):
        self.rec, self.B, self.calls = recorder, recorder.B, []

    def state(self):
        return self.rec.state()

    def __getattr__(self, method):
        if method not in DRIVER_METHODS:
            raise AttributeError(method)

        def call(*args, **kwargs):
            self.calls.append((method, tuple(_copied(a) for a in args), {k: _copied(v) for k, v in kwargs.items()}))
            getattr(self.rec, method)(*args, **kwargs)
        return call

    @property
    def actions(self):
        """every step's actions, uint8 (steps, B)"""
        rows = [np.asarray(args[0], np.uint8).reshape(self.B) for m, args, _ in self.calls if m == "step"]
        return np.stack(rows) if rows else np.zeros((0, self.B), np.uint8)

    def replay(self, d):
        for method, args, kwargs in self.calls:
            getattr(d, method)(*args, **kwargs)


def script_of(cases, name, render=False):
    """the script of scenario `name` of a cases module (wall_bank_cases, wall_generator_cases, wall_caves_cases)"""
    fn, c = cases.SCENARIOS[name]
    s = Script(cases.Recorder(c, render))
    fn(s)
    return s


class Calls:
    """a script given as a list of (method, args, kwargs) — steps, unmasked resets and RENDER_METHODS — for an engine whose reference is
    not a Recorder (oracle.OracleBatch)"""

    def __init__(self, calls, batch):
        self.B, self.calls = batch, [(m, tuple(_copied(a) for a in args), dict(kw)) for m, args, kw in calls]
        rows = [np.asarray(args[0], np.uint8).reshape(batch) for m, args, _ in self.calls if m == "step"]
        self.actions = np.stack(rows) if rows else np.zeros((0, batch), np.uint8)


class Steps(Calls):
    """a script of steps alone"""

    def __init__(self, actions):
        actions = np.ascontiguousarray(actions, np.uint8)
        super().__init__([("step", (row,), {}) for row in actions], actions.shape[1])


# ---- the weights' staging: a scenario of this module's own, on wall_bank_cases' drivers ------------------------------------------------------
WEIGHT_VECTORS = ((1, 0, 0), (0, 1, 0), (0, 0, 1))
WEIGHT_STEPS = 12


def weights_scenario(d):
    """three layouts under time limit 1 — every agent's episode is cut by one step and restarted by the next —, other weights in front of
    every step: each restart must draw under the vector queued last, and the twelve vectors pass through ONE pinned buffer"""
    import wall_bank_cases as BC
    import walls_ref as WR

    d.set_wall_bank(BC.three_layouts(6, 6))
    d.set_time_limit(1)
    rng = np.random.default_rng(31)
    for t in range(WEIGHT_STEPS):
        d.set_weights(np.array(WEIGHT_VECTORS[t % 3], np.uint32))
        d.step(WR.draw_actions(rng, d.B))


def weights_recording(render):
    """(script, snapshots, events) of weights_scenario on wall_bank_cases.CALLS' shape: the reference alone"""
    import wall_bank_cases as BC

    s = Script(BC.Recorder(BC.CALLS, render))
    weights_scenario(s)
    return s, s.rec.snaps, s.rec.events


def restarts_by_vector(calls, snaps):
    """from the reference's snapshots alone: {weight vector: (episode starts under it, {layouts they drew})}"""
    out, vector = {}, None
    for k, (method, args, _) in enumerate(calls):
        if method == "set_weights":
            vector = tuple(int(x) for x in args[0])
        elif method == "step" and vector is not None:
            moved = snaps[k + 1]["episode"] != snaps[k]["episode"]
            n, drew = out.get(vector, (0, set()))
            out[vector] = (n + int(moved.sum()), drew | set(snaps[k + 1]["wall_layout"][moved].tolist()))
    return out


def describe(call):
    method, args, kwargs = call
    short = lambda v: f"<{'x'.join(map(str, v.shape))}>" if isinstance(v, np.ndarray) else repr(v)
    return f"{method}({', '.join([short(a) for a in args] + [f'{k}={short(v)}' for k, v in kwargs.items()])})"


# ---- the comparison --------------------------------------------------------------------------------------------------------------------
def first_difference(got, want, calls):
    """the first (call index, call, array name) at which the records differ — a missing array, a shape, a type or a byte — or None"""
    assert len(got) == len(want) == len(calls), (len(got), len(want), len(calls))
    for k, (g, w) in enumerate(zip(got, want)):
        for name in w:
            if name not in g:
                return k, describe(calls[k]), f"{name} (not copied)"
            a, b = np.asarray(g[name]), np.asarray(w[name])
            if a.shape != b.shape or a.dtype != b.dtype or a.tobytes() != b.tobytes():
                return k, describe(calls[k]), name
    return None


def assert_records_equal(got, want, calls, where):
    d = first_difference(got, want, calls)
    if d is not None:
        k, call, name = d
        a, b = np.asarray(got[k].get(name, ())), np.asarray(want[k].get(name, ()))
        n = int((a != b).sum()) if a.shape == b.shape else -1
        raise AssertionError(f"{where}: the first difference is at call {k}, {call}: {name} ({n} of {b.size} elements differ)")


def records_of_snapshots(snaps, keys=("camera_view", "reward", "done", "truncated", "episode_steps", "wall_layout")):
    """the reference's own records of a rendered recording: snapshot k + 1 stands behind call k"""
    return [{k: s[k] for k in keys if k in s} for s in snaps[1:]]


# ---- the observed twin ---------------------------------------------------------------------------------------------------------------------
HOST_STATE = ("status", "episode", "goal", "position_bits", "heading", "tile_map_chunks", "col_height", "col_colour")


def host_record(env, watch, drawn):
    """the watched outputs through the ordinary host getters (each waits for the stream)"""
    w = env.world
    r = dict(camera_view=env.camera_view_host(), reward=w.reward, done=w.done.astype(np.uint8), truncated=w.truncated.astype(np.uint8),
             episode_steps=w.episode_steps)
    if drawn:
        r["wall_layout"] = env.wall_layout.numpy()
    if "goal_distance" in watch:
        r.update(goal_distance=env.goal_distance.numpy(), goal_start_distance=env.goal_start_distance.numpy(),
                 goal_progress=env.goal_progress.numpy(), goal_distance_field=env.goal_distance_field_device().numpy())
    if "seen_map" in watch:
        r.update(seen_count=env.seen_count.numpy(), seen_new=env.seen_new.numpy(), goal_seen=env.goal_seen.numpy(), seen_map=env.seen_map_device.numpy())
    if "local_map" in watch:
        r["local_map"] = env.local_map_host()
    if "learner_view" in watch:
        r["learner_view"] = env.learner_view_host()
    if "top_view" in watch:
        r["top_view"] = env.top_view_host()
    return r


def host_state(env):
    """what has no device pointer, and last the column descriptors (rcw_columns: ensure_columns)"""
    w = env.world
    pos = w.player_position_wu
    s = dict(status=w.status, episode=w.episode, goal=w.goal_position, position_bits=pos.view(np.uint64 if pos.dtype == np.float64 else np.uint32),
             heading=w.player_direction_au, tile_map_chunks=w.tile_map_chunks)
    s["col_height"], s["col_colour"] = env.columns()
    return s


def is_drawn(env):
    return bool(env.wall_bank_info["layouts"]) or env.wall_generator_info["enabled"]


class _Noting:
    """a Player whose every call is followed by a note"""

    def __init__(self, player, note):
        self._p, self._note, self.B = player, note, player.B

    def state(self):
        return self._p.state()

    def __getattr__(self, method):
        if method not in DRIVER_METHODS:
            raise AttributeError(method)

        def call(*args, **kwargs):
            getattr(self._p, method)(*args, **kwargs)
            self._note()
        return call


def observed_twin(cases, rcw, name, env, trackers, watch):
    """`cases.play(rcw, name, env, trackers)` — the cases' own Player against the cases' own recording, every tracker told of every call —
    with the host copies of the watched outputs kept behind EVERY call (play's `wrap`: trackers are told of steps and masked calls only):
    (records, the host state behind the last call, events)"""
    records = []
    events = cases.play(rcw, name, env, trackers, wrap=lambda p: _Noting(p, lambda: records.append(host_record(env, watch, is_drawn(env)))))
    return records, host_state(env), events


# ---- the fourth driver: the engine, unread -------------------------------------------------------------------------------------------------
class NotPending(AssertionError):
    def __init__(self, message, host_slow):
        super().__init__(message)
        self.host_slow = host_slow


_backlog_buffers = {}


def release_backlog():
    """drop the backlog's tensors and hand torch's cached blocks back to the device"""
    if _backlog_buffers:
        import torch

        _backlog_buffers.clear()
        torch.cuda.empty_cache()


_SWITCHES = dict(set_wall_bank=("walls", None), set_wall_generator=("loops", 0.0), set_wall_caves=("fill", 0.4))   # first parameter, its default


def switched_on(call):
    """whether a set_wall_bank / set_wall_generator / set_wall_caves call leaves wall_layout served: None as the first argument switches off"""
    method, args, kwargs = call
    keyword, default = _SWITCHES[method]
    return (args[0] if args else kwargs.get(keyword, default)) is not None


class Deferred:
    """`script` on `env`, nothing read before the end.  watch: the features whose outputs are copied beside the ones always copied
    ("goal_distance", "seen_map", "local_map", "learner_view", "top_view"); mode: "host" (each step's numpy row: rcw_step's ring) or "device"
    (rows of one uint8 CUDA tensor uploaded before the script starts: rcw_step_device).  `run(want, final)` raises on the first difference."""

    def __init__(self, rcw, env, script, watch=(), mode="host", name="", backlog=1):
        assert mode in ("host", "device")
        self.rcw, self.env, self.calls, self.watch, self.mode, self.name, self.scale = rcw, env, list(script.calls), tuple(watch), mode, name, backlog
        self.actions = script.actions
        self.report = {}

    # -- what is copied --
    def _arrays(self):
        env, a = self.env, {}
        a.update(camera_view=env.camera_view, reward=env.reward_device(), done=env.done_device(), truncated=env.truncated_device(),
                 episode_steps=env.episode_steps_device())
        if "goal_distance" in self.watch:
            a.update(goal_distance=env.goal_distance, goal_start_distance=env.goal_start_distance, goal_progress=env.goal_progress,
                     goal_distance_field=env.goal_distance_field_device())
        if "seen_map" in self.watch:
            a.update(seen_count=env.seen_count, seen_new=env.seen_new, goal_seen=env.goal_seen, seen_map=env.seen_map_device)
        if "local_map" in self.watch:
            a["local_map"] = env.local_map
        if "learner_view" in self.watch:
            a["learner_view"] = env.learner_view
        if "top_view" in self.watch:
            a["top_view"] = env.top_view
        return a

    def _queue_copies(self, arrays, drawn):
        q = {k: x.torch(sync=False).clone() for k, x in arrays.items()}
        if drawn:
            q["wall_layout"] = self.env.wall_layout.torch(sync=False).clone()      # (the pointer: rcw_wall_layout_device_ptr, from the host)
        return q

    def _backlog(self, torch):
        dev = self.env.device
        buf = _backlog_buffers.get(dev)
        if buf is None:
            buf = _backlog_buffers[dev] = torch.empty(BACKLOG_BYTES // 4, dtype=torch.int32, device=f"cuda:{dev}")
            torch.cuda.synchronize(dev)
        first, last = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        first.record()
        for k in range(BACKLOG_FILLS * self.scale):
            buf.fill_(k)
        last.record()
        return first, last

    def _call(self, k, step_row, device_actions):
        method, args, kwargs = self.calls[k]
        env = self.env
        if method == "step":
            self.rcw.act_(env, device_actions[step_row] if self.mode == "device" else args[0])
        elif method == "reset":
            self.rcw.reset_(env, *args, **kwargs)
        elif method == "set_weights":
            env.set_wall_bank_weights(*args, **kwargs)
        elif method == "update_camera_view":
            self.rcw.update_camera_view_(env)
        elif method == "update_top_view":
            self.rcw.update_top_view_(env)
        elif method == "cast_rays":
            env._check(env._lib.rcw_cast_rays(env._h))                         # (cast_rays_ of the mirror goes on to read the rays)
        elif method == "bind_obs":
            env.bind_obs(None)                                                # the handle's own buffer: the next step stores every frame
        elif method == "columns_device":
            self._columns = env.columns_device()
        elif method == "expand_columns":
            h, c = self._columns
            return dict(expanded=env.expand_columns(h.torch(sync=False), c.torch(sync=False)))
        else:
            getattr(env, method)(*args, **kwargs)

    def run(self, want, final=None):
        import torch

        env, calls = self.env, self.calls
        assert len(want) == len(calls), (len(want), len(calls))
        start, check = plan_backlog(calls, self.mode) if self.scale else (None, None)     # (backlog=0: no backlog, for measuring the host alone)
        stream = env.torch_stream()
        with torch.cuda.stream(stream):
            device_actions = None
            if self.mode == "device":
                device_actions = torch.from_numpy(self.actions).to(f"cuda:{env.device}")
            arrays = self._arrays()
            stream.synchronize()
            syncs, drawn, copies, row = env.host_syncs, is_drawn(env), [], 0
            events = t_backlog = pending = t_check = None
            t0 = time.perf_counter()
            for k, call in enumerate(calls):
                if k == start:
                    events = self._backlog(torch)
                    t_backlog = time.perf_counter()
                if k == check:
                    pending, t_check = not events[1].query(), time.perf_counter()
                extra = self._call(k, row, device_actions)
                row += call[0] == "step"
                if call[0] in _SWITCHES:
                    drawn = switched_on(call)
                copies.append(dict(self._queue_copies(arrays, drawn), **(extra or {})))
            if check == len(calls):
                pending, t_check = not events[1].query(), time.perf_counter()
            t_end = time.perf_counter()
            assert env.host_syncs == syncs, f"{self.name}: the mirror counted a host synchronisation before the end"
            env.sync()                                                        # the one wait
        got = [{k: t.cpu().numpy() for k, t in q.items()} for q in copies]
        self.report = dict(calls=len(calls), enqueue_ms=1e3 * (t_end - t0), backlog_at=start, checked_at=check, pending=pending, backlogs=self.scale)
        if events is not None:
            self.report.update(backlog_ms=events[0].elapsed_time(events[1]), host_ms_to_check=1e3 * (t_check - t_backlog))
            assert self.report["backlog_ms"] < BACKLOG_LIMIT_MS * self.scale, f"{self.name}: the backlog took {self.report['backlog_ms']:.0f} ms"
        assert_records_equal(got, want, calls, f"{self.name}, unread, {self.mode} actions")
        if final is not None:
            have = host_state(env)
            for key in HOST_STATE:
                if key in final:
                    np.testing.assert_array_equal(have[key], final[key], err_msg=f"{self.name}, unread: {key} behind the last call")
        if start is not None and not pending:
            r = self.report
            slow = r["host_ms_to_check"] >= 0.5 * r["backlog_ms"]
            raise NotPending(f"{self.name}: a call waited for the stream — the backlog ({r['backlog_ms']:.1f} ms on the device) had ended in front of "
                             f"call {check} of {len(calls)}, {r['host_ms_to_check']:.1f} ms of host time behind it" if not slow else
                             f"{self.name}: the host took {r['host_ms_to_check']:.1f} ms to queue calls {start} .. {check} behind a backlog of "
                             f"{r['backlog_ms']:.1f} ms", slow)
        return self.report


def run_unread(make, rcw, script, want, final=None, watch=(), mode="host", name=""):
    """Deferred on a fresh engine `make()`; where the backlog had ended although the host was merely slow, once more on another fresh
    engine with four times the backlog — and then the assertion stands"""
    env = make()
    try:
        return Deferred(rcw, env, script, watch, mode, name).run(want, final)
    except NotPending as e:
        if not e.host_slow:
            raise
    finally:
        env.close()
    env = make()
    try:
        return Deferred(rcw, env, script, watch, mode, name, backlog=4).run(want, final)
    finally:
        env.close()
