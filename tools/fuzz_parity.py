#!/usr/bin/env python3
"""Dev tool (GPU box): differential fuzzing of the HIP path against the CPU oracle over random
configurations (map size, columns, headings, field of view, radius, step, camera height, image
height, world-unit type, the three unpinned switches, both BoundsError policies, auto-reset).

    python tools/fuzz_parity.py [configs] [seed] [top|split|flat|step|limit|goal|bank|gen|caves|rooms]
                                                                   # "top": every configuration renders the top view;
                                                                   # "split": ... with a geometry of the unit store kernels;
                                                                   # "flat": ... of the flat store kernel (any pu >= 9), and any
                                                                   #         camera height from 24 rows (the flat fill kernel)
                                                                   # "step": the geometries of the one-launch step, asked for in every case
                                                                   # "limit": ... of at most 17 agents and 512 rows, with an episode time limit of
                                                                   #         1, 2, 3, 7 or 20 steps: the rollout against tests/time_limit_ref.py over
                                                                   #         the oracle, episode_steps and truncated compared with the rest
                                                                   # "goal": the goal distance (rcw_set_goal_distance) — random maps, layouts and
                                                                   #         sequences of calls against tests/goal_distance_ref.py, the three words and
                                                                   #         every agent's whole field compared after every call (goal_mode below)
                                                                   # "bank": the wall bank (rcw_set_wall_bank) — random maps, banks, weights and
                                                                   #         sequences of calls against tests/wall_bank_ref.py, the whole state, the
                                                                   #         frames and wall_layout compared after every call (bank_mode below)
                                                                   # "gen", "caves", "rooms": a family of the wall generator
                                                                   #         (rcw_set_wall_generator, rcw_set_wall_caves, rcw_set_wall_rooms) — random maps,
                                                                   #         the family's parameters, level ranges and sequences of calls against
                                                                   #         tests/wall_family.py's reference, compared the same way (family_mode below)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np

import goal_distance_ref as GD
import raycastworlds_jl_amd as RCW
import time_limit_ref as TL
from helpers import assert_state_equal
from oracle import oracle as O

n_cfg = int(sys.argv[1]) if len(sys.argv) > 1 else 200
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
always_top = len(sys.argv) > 3 and sys.argv[3] in ("top", "split", "flat")
split_geometry = len(sys.argv) > 3 and sys.argv[3] == "split"   # geometries of the unit store kernels (units of 256 / 128 / 64 / 32 rows)
flat_geometry = len(sys.argv) > 3 and sys.argv[3] == "flat"     # geometries of the flat store kernel; the two-kernel form is asked for
step_geometry = len(sys.argv) > 3 and sys.argv[3] == "step"     # what the one-launch step takes (a camera view of 256 k / 128 / 64 rows, no top view), asked for in every case:
                                                                # 1 .. 1,500 view columns (a wavefront per agent, a workgroup per agent, the table's tail), maps of up to 40 x 40 tiles
limit_geometry = len(sys.argv) > 3 and sys.argv[3] == "limit"   # "step"'s draw with a time limit (rcw_set_time_limit): the *_limit_kernel twins of the step's kernels


def goal_mode(n_cfg, seed):
    """Maps of 3 x 4 to 48 x 48 tiles, one in six 64 to 140 on a side (levels wider than a wavefront; at most 4 agents there: the Python
    floods of the reference are the cost); the ring, four rooms, a maze, pillars at 0.05 to 0.35 or the serpentine, one layout per agent
    or one for all; 1 to 17 agents, Float32 and Float64, both forms of the step asked for, auto_reset on and off, a time limit of 0, 2, 5
    or 20.  Then 30 random calls — a step, a masked or full reset_, a masked set_state to random free tiles, a masked set_walls, the
    feature off and on again —, everything compared by GD.Tracked after each.  Every configuration draws from a generator of its own,
    default_rng([seed, c]): what it is does not depend on the ones before it."""
    from raycastworlds_jl_amd import _capi, layouts

    rng = None

    def layout(H, W):
        kind = str(rng.choice(["ring", "four_rooms", "maze", "pillars", "serpentine"]))
        if kind in ("four_rooms", "maze") and min(H, W) < 5:
            kind = "ring"
        w = {"ring": lambda: layouts.ring(H, W), "four_rooms": lambda: layouts.four_rooms(H, W), "maze": lambda: layouts.maze(H, W, rng),
             "pillars": lambda: GD.pillars(H, W, float(rng.uniform(0.05, 0.35)), rng), "serpentine": lambda: GD.serpentine(H, W)}[kind]()
        return w if (~w).sum() >= 2 else layouts.ring(H, W)                  # (rcw_set_walls wants two free tiles)

    def world(B, H, W):
        return np.stack([layout(H, W) for _ in range(B)]) if rng.integers(0, 2) else layout(H, W)

    def some(B):
        mask = (rng.random(B) < 0.5).astype(np.uint8)
        mask[int(rng.integers(0, B))] = 1
        return mask

    totals = dict(floods_behind_a_step=0, agent_steps_at_distance_minus_1=0, step=0, reset=0, masked_reset=0, set_state=0, set_walls=0, off_and_on=0,
                  widest_level=0, tiles_multiple_of_32=0, tiles_not_multiple_of_32=0, one_launch_steps=0, two_launch_steps=0)
    fails = 0
    for c in range(n_cfg):
        rng = np.random.default_rng([seed, c])
        big = rng.integers(0, 6) == 0
        H, W = (int(rng.integers(64, 141)), int(rng.integers(64, 141))) if big else (int(rng.integers(3, 49)), int(rng.integers(4, 49)))
        B = int(rng.integers(1, 5 if big else 18))
        T64, auto_reset, L = bool(rng.integers(0, 2)), bool(rng.integers(0, 2)), int(rng.choice([0, 2, 5, 20]))
        N, Hc = [(8, 24), (16, 64), (64, 256), (7, 128)][int(rng.integers(0, 4))]
        form = str(rng.choice(["one-launch", "two-launches"]))
        engine_seed = int(rng.integers(0, 2**31))
        where = f"config {c}: {H} x {W}, B={B} T64={T64} auto_reset={auto_reset} L={L} N={N} Hc={Hc} {form} seed={engine_seed}"
        try:
            env = RCW.SingleRoomModule.SingleRoom(batch=B, seed=engine_seed, T="Float64" if T64 else "Float32", auto_reset=auto_reset, height_tile_map_tu=H,
                                                  width_tile_map_tu=W, num_rays=N, height_camera_view_pu=Hc, num_directions=8, position_increment_wu=0.25,
                                                  player_radius_wu=0.3)
            try:
                env.set_step_form(form)
            except _capi.RcwError as e:                        # the one refusal there is: this geometry does not take the one-launch step
                assert form == "one-launch" and e.code == _capi.RCW_ERR_UNSUPPORTED and "does not take the one-launch step" in e.message, e
                form = "two-launches"
            assert env.step_form() == form
            totals["one_launch_steps" if form == "one-launch" else "two_launch_steps"] += 1
            totals["tiles_multiple_of_32" if H * W % 32 == 0 else "tiles_not_multiple_of_32"] += 1
            env.set_walls(world(B, H, W))
            env.set_time_limit(L)
            t = GD.Tracked(RCW, env)
            for k in range(30):
                call = str(rng.choice(["step", "step", "step", "step", "reset", "masked_reset", "set_state", "set_walls", "off_and_on"]))
                at = f"{where}, call {k} ({call})"
                totals[call] += 1
                if call == "step":
                    t.step(rng.integers(1, 5, B).astype(np.uint8), at)
                elif call in ("reset", "masked_reset"):
                    mask = some(B) if call == "masked_reset" else None
                    RCW.reset_(env, mask=mask, seed=int(rng.integers(0, 2**31)))
                    t.masked(mask, at)
                elif call == "set_state":
                    mask, w = some(B), env.world
                    goal, pos, heading = w.goal_position, w.player_position_wu, w.player_direction_au
                    for b in np.flatnonzero(mask):
                        free = np.argwhere(~t._walls[b])
                        goal[b] = free[int(rng.integers(0, len(free)))] + 1
                        pos[b] = free[int(rng.integers(0, len(free)))] + 0.5
                        heading[b] = int(rng.integers(0, 8))
                    env.set_state(goal, pos, heading, mask=mask)
                    t.masked(mask, at)
                elif call == "set_walls":
                    mask = some(B)
                    env.set_walls(world(B, H, W), mask=mask)
                    t.masked(mask, at)
                else:
                    env.set_goal_distance(False)
                    assert not env.goal_distance_enabled
                    env.set_goal_distance(True)
                    t.masked(None, at)
            totals["floods_behind_a_step"] += t.floods["step"]
            totals["agent_steps_at_distance_minus_1"] += t.events["unreachable"]
            totals["widest_level"] = max(totals["widest_level"], t.widest["step"], t.widest["refill"])
            env.close()
        except Exception as e:   # noqa: BLE001
            fails += 1
            print(f"{where} FAILED\n   {type(e).__name__}: {str(e)[:400]}")
            if fails >= 5:
                break
    print(f"{n_cfg} random configurations (goal distance: " + ", ".join(f"{v} {k}" for k, v in totals.items()) + f"), {fails} mismatches")
    return 1 if fails else 0


def bank_mode(n_cfg, seed):
    """Maps of 3 x 4 to 40 x 40 tiles; a bank of 1, 2, 3, 7 or 70 layouts — the ring, four rooms, a maze or pillars at 0.05 to 0.35 —,
    uniform or with random weights of 0 to 5; 1 to 9 agents with 8 or 16 view columns (the reference renders in Python), Float32 and
    Float64, both forms of the step asked for, a time limit of 0, 2 or 5, auto_reset.  Then 30 random calls — a step, a masked or full
    reset_ with a new seed, a masked set_state onto free tiles of each agent's current layout, new weights, the bank off and another one
    on —, each made on the reference (tests/wall_bank_cases.py's Recorder) and on the engine (its Player), which compares the whole state,
    the frames, the time limit's words and wall_layout after every call.  Every configuration draws from default_rng([seed, c])."""
    import wall_bank_cases as BC
    from raycastworlds_jl_amd import _capi, layouts

    rng = None

    def layout(H, W):
        kind = str(rng.choice(["ring", "four_rooms", "maze", "pillars"]))
        if kind in ("four_rooms", "maze") and min(H, W) < 5:
            kind = "ring"
        w = {"ring": lambda: layouts.ring(H, W), "four_rooms": lambda: layouts.four_rooms(H, W), "maze": lambda: layouts.maze(H, W, rng),
             "pillars": lambda: GD.pillars(H, W, float(rng.uniform(0.05, 0.35)), rng)}[kind]()
        return w if (~w).sum() >= 2 else layouts.ring(H, W)

    def bank(H, W):
        M = int(rng.choice([1, 2, 3, 7, 70]))
        walls = np.stack([layout(H, W) for _ in range(M)])
        weights = None
        if rng.integers(0, 2):
            weights = rng.integers(0, 6, M).astype(np.uint32)
            weights[int(rng.integers(0, M))] += 1                            # (a sum of zero is refused)
        return walls, weights

    def some(B):
        mask = (rng.random(B) < 0.5).astype(np.uint8)
        mask[int(rng.integers(0, B))] = 1
        return mask

    totals = dict(step=0, reset=0, masked_reset=0, set_state=0, weights=0, off_and_on=0, episode_starts=0, layout_changed=0, layout_kept=0, goal_redraws=0,
                  restarts_after_done=0, restarts_after_truncation=0, one_launch_steps=0, two_launch_steps=0, words_not_multiple_of_4=0, banks_past_64=0)
    fails = 0
    for c in range(n_cfg):
        rng = np.random.default_rng([seed, c])
        H, W = int(rng.integers(3, 41)), int(rng.integers(4, 41))
        B = int(rng.integers(1, 10))
        T64, L = bool(rng.integers(0, 2)), int(rng.choice([0, 2, 5]))
        N, Hc = [(8, 64), (16, 64), (8, 24), (16, 128)][int(rng.integers(0, 4))]
        form = str(rng.choice(["one-launch", "two-launches"]))
        engine_seed = int(rng.integers(0, 2**31))
        shape = dict(H=H, W=W, N=N, Hc=Hc, B=B, seed=engine_seed, T="Float64" if T64 else "Float32")
        where = f"config {c}: {H} x {W}, B={B} T64={T64} L={L} N={N} Hc={Hc} {form} seed={engine_seed}"
        try:
            env = BC.make_env(RCW, shape)
            try:
                env.set_step_form(form)
            except _capi.RcwError as e:
                assert form == "one-launch" and e.code == _capi.RCW_ERR_UNSUPPORTED and "does not take the one-launch step" in e.message, e
                form = "two-launches"
            totals["one_launch_steps" if form == "one-launch" else "two_launch_steps"] += 1
            totals["words_not_multiple_of_4"] += int(((2 * H * W + 63) // 64 * 2) % 4 != 0)
            rec = BC.Recorder(shape)
            play = BC.Player(RCW, env, rec.snaps, where)
            both = lambda call, *a, **k: (getattr(rec, call)(*a, **k), getattr(play, call)(*a, **k))
            if L:
                both("set_time_limit", L)
            walls, weights = bank(H, W)
            totals["banks_past_64"] += int(len(walls) > 64)
            both("set_wall_bank", walls, weights)
            for k in range(30):
                call = str(rng.choice(["step", "step", "step", "step", "step", "reset", "masked_reset", "set_state", "weights", "off_and_on"]))
                play.name = f"{where}, call {k} ({call})"
                totals[call] += 1
                if call == "step":
                    both("step", rng.integers(1, 5, B).astype(np.uint8))
                elif call in ("reset", "masked_reset"):
                    both("reset", some(B) if call == "masked_reset" else None, int(rng.integers(0, 2**31)))
                elif call == "set_state":
                    mask, s = some(B), rec.snaps[-1]
                    goal, pos, heading = s["goal"].copy(), s["position"].copy(), s["direction"].copy()
                    for b in np.flatnonzero(mask):
                        free = np.argwhere(~rec.ref.walls_of(b))
                        goal[b] = free[int(rng.integers(0, len(free)))] + 1
                        pos[b] = free[int(rng.integers(0, len(free)))] + 0.5
                        heading[b] = int(rng.integers(0, 8))
                    both("set_state", goal, pos, heading, mask)
                elif call == "weights":
                    M = len(rec.ref.bank)
                    weights = rng.integers(0, 6, M).astype(np.uint32)
                    weights[int(rng.integers(0, M))] += 1
                    both("set_weights", weights if rng.integers(0, 4) else None)
                else:
                    both("set_wall_bank", None)
                    both("step", rng.integers(1, 5, B).astype(np.uint8))
                    walls, weights = bank(H, W)
                    totals["banks_past_64"] += int(len(walls) > 64)
                    both("set_wall_bank", walls, weights)
            play.finished()
            for k, v in rec.events.items():
                if k in totals:
                    totals[k] += v
            env.close()
        except Exception as e:   # noqa: BLE001
            fails += 1
            print(f"{where} FAILED\n   {type(e).__name__}: {str(e)[:400]}")
            if fails >= 5:
                break
    print(f"{n_cfg} random configurations (wall bank: " + ", ".join(f"{v} {k}" for k, v in totals.items()) + f"), {fails} mismatches")
    return 1 if fails else 0


# ---- the wall generator's families: what each one contributes to family_mode ---------------------------------------------------------------------
def _draw_generator(rng):
    """loops 0, 0.1, 0.5 or 1"""
    return dict(loops=float(rng.choice([0.0, 0.0, 0.1, 0.5, 1.0])))


def _draw_caves(rng):
    """fill 0.2 .. 0.6 (now and then 0 or all wall), smoothed 0 .. 8 times"""
    fill = [0.2, 0.3, 0.4, 0.4, 0.45, 0.5, 0.6, 0.0, 1.0][int(rng.integers(0, 9))]
    return dict(fill=fill, smooth=int(rng.integers(0, 9)))


def _draw_rooms(rng):
    """a least room side of 1 .. 4, stop 0 .. 0.5 (now and then always), a second door with probability 0 .. 1"""
    stop = [0.0, 0.0, 0.1, 0.25, 0.25, 0.5, 1.0][int(rng.integers(0, 7))]
    doors = [0.0, 0.25, 0.25, 0.5, 1.0][int(rng.integers(0, 5))]
    return dict(room=int(rng.integers(1, 5)), stop=stop, doors=doors)


# mode -> the row of tests/wall_family.py, the closing line's label, the parameter draw, the calls beside step / reset / set_state, the totals
# behind the calls' own (the reference's events, then what is counted of a map and of an install), and how those are counted
FUZZ_FAMILIES = dict(
    gen=dict(family="generator", label="wall generator", draw=_draw_generator, calls=("off_and_on",), events=("episode_starts",),
             counts=("even_sizes", "with_levels", "with_loops", "cells_past_64"),
             of_map=lambda H, W: dict(even_sizes=H % 2 == 0 or W % 2 == 0, cells_past_64=((H - 1) // 2) * ((W - 1) // 2) > 64),
             of_install=lambda g: dict(with_loops=g["loops"] > 0), of_events=lambda ev: {}),
    caves=dict(family="caves", label="wall caves", draw=_draw_caves, calls=("arrive", "off_and_on"), events=("episode_starts", "fallbacks", "caves_kept"),
               counts=("non_square", "with_levels", "smoothed", "tiles_past_64"),
               of_map=lambda H, W: dict(non_square=H != W, tiles_past_64=(H - 2) * (W - 2) > 64),
               of_install=lambda g: dict(smoothed=g["smooth"] > 0), of_events=lambda ev: dict(caves_kept=ev["episode_starts"] - ev["fallbacks"])),
    rooms=dict(family="rooms", label="wall rooms", draw=_draw_rooms, calls=("arrive", "off_and_on"), events=("episode_starts", "rooms_made", "second_doors"),
               counts=("non_square", "with_levels", "stopped", "rooms_past_64"),                       # (rooms_past_64: more (odd, odd) tiles than a wavefront has lanes)
               of_map=lambda H, W: dict(non_square=H != W, rooms_past_64=-(-(H - 2) // 2) * -(-(W - 2) // 2) > 64),
               of_install=lambda g: dict(stopped=g["stop"] > 0), of_events=lambda ev: {}),
)


def family_mode(mode, n_cfg, seed):
    """One family of the wall generator (FUZZ_FAMILIES[mode]): maps of 5 x 5 to 40 x 40 tiles, a quarter of them 5 .. 8 on a side; the family's
    own parameters by its draw; no levels, or 1, 2 or 5 levels from a random first level under a random level seed; 1 to 9 agents with 8 or 16
    view columns (the reference renders in Python), Float32 and Float64, both forms of the step asked for, a time limit of 0, 2 or 5,
    auto_reset.  Then 30 random calls — a step, a masked or full reset_ with a new seed, a masked set_state onto free tiles of each agent's
    current layout, for caves and rooms some agents walked into their goals (wall_bank_cases.walk_into_the_goal: in open layouts a random walk
    rarely arrives), the family off and other parameters on —, each made on the reference (tests/wall_family.py's Recorder) and on the
    engine (its Player), which compares the whole state, the frames, the time limit's words and wall_layout after every call.  Every
    configuration draws from default_rng([seed, c])."""
    import wall_family as WF
    from raycastworlds_jl_amd import _capi

    fam = FUZZ_FAMILIES[mode]
    setter = WF.FAMILIES[fam["family"]].setter
    Recorder, Player = WF.drivers(fam["family"])
    rng = None

    def parameters():
        levels = int(rng.choice([0, 0, 1, 2, 5]))
        return dict(fam["draw"](rng), levels=levels, first_level=int(rng.integers(0, 2**31 - 1 - levels)) if levels else 0,
                    level_seed=int(rng.integers(0, 2**63)) if levels else 0)

    def some(B):
        mask = (rng.random(B) < 0.5).astype(np.uint8)
        mask[int(rng.integers(0, B))] = 1
        return mask

    def count(found):
        for k, v in found.items():
            totals[k] += int(v)

    totals = dict.fromkeys(("step", "reset", "masked_reset", "set_state") + fam["calls"] + fam["events"] + ("goal_redraws", "restarts_after_done",
                           "restarts_after_truncation", "one_launch_steps", "two_launch_steps") + fam["counts"], 0)
    fails = 0
    for c in range(n_cfg):
        rng = np.random.default_rng([seed, c])
        H, W = int(rng.integers(5, 41)), int(rng.integers(5, 41))
        if c % 4 == 0:
            H, W = int(rng.integers(5, 9)), int(rng.integers(5, 9))          # (a quarter small: agents arrive, restarts after done)
        B = int(rng.integers(1, 10))
        T64, L = bool(rng.integers(0, 2)), int(rng.choice([0, 2, 5]))
        N, Hc = [(8, 64), (16, 64), (8, 24), (16, 128)][int(rng.integers(0, 4))]
        form = str(rng.choice(["one-launch", "two-launches"]))
        engine_seed = int(rng.integers(0, 2**31))
        shape = dict(H=H, W=W, N=N, Hc=Hc, B=B, seed=engine_seed, T="Float64" if T64 else "Float32")
        where = f"config {c}: {H} x {W}, B={B} T64={T64} L={L} N={N} Hc={Hc} {form} seed={engine_seed}"
        try:
            env = WF.make_env(RCW, shape)
            try:
                env.set_step_form(form)
            except _capi.RcwError as e:
                assert form == "one-launch" and e.code == _capi.RCW_ERR_UNSUPPORTED and "does not take the one-launch step" in e.message, e
                form = "two-launches"
            totals["one_launch_steps" if form == "one-launch" else "two_launch_steps"] += 1
            count(fam["of_map"](H, W))
            rec = Recorder(shape)
            play = Player(RCW, env, rec.snaps, where)
            both = lambda call, *a, **k: (getattr(rec, call)(*a, **k), getattr(play, call)(*a, **k))
            if L:
                both("set_time_limit", L)

            def install():
                g = parameters()
                count(dict(fam["of_install"](g), with_levels=g["levels"] > 0))
                both(setter, **g)

            install()
            for k in range(30):
                call = str(rng.choice(["step", "step", "step", "step", "step", "step", "reset", "masked_reset", "set_state"] + list(fam["calls"])))
                play.name = f"{where}, call {k} ({call})"
                totals[call] += 1
                if call == "step":
                    both("step", rng.integers(1, 5, B).astype(np.uint8))
                elif call in ("reset", "masked_reset"):
                    both("reset", some(B) if call == "masked_reset" else None, int(rng.integers(0, 2**31)))
                elif call == "set_state":
                    mask, s = some(B), rec.snaps[-1]
                    goal, pos, heading = s["goal"].copy(), s["position"].copy(), s["direction"].copy()
                    for b in np.flatnonzero(mask):
                        free = np.argwhere(~rec.ref.walls_of(b))
                        goal[b] = free[int(rng.integers(0, len(free)))] + 1
                        pos[b] = free[int(rng.integers(0, len(free)))] + 0.5
                        heading[b] = int(rng.integers(0, 8))
                    both("set_state", goal, pos, heading, mask)
                elif call == "arrive":
                    mask = some(B)
                    for b in np.flatnonzero(mask):                           # (free tiles in one row have no tile to walk down from)
                        free = ~rec.ref.walls_of(b)
                        mask[b] = int((free[:-1] & free[1:]).any())
                    WF.walk_into_the_goal(rec, mask)
                    WF.walk_into_the_goal(play, mask)
                else:
                    both(setter, None)
                    both("step", rng.integers(1, 5, B).astype(np.uint8))
                    install()
            play.finished()
            events = rec.events
            count({k: v for k, v in dict(events, **fam["of_events"](events)).items() if k in totals})
            env.close()
        except Exception as e:   # noqa: BLE001
            fails += 1
            print(f"{where} FAILED\n   {type(e).__name__}: {str(e)[:400]}")
            if fails >= 5:
                break
    print(f"{n_cfg} random configurations ({fam['label']}: " + ", ".join(f"{v} {k}" for k, v in totals.items()) + f"), {fails} mismatches")
    return 1 if fails else 0


if len(sys.argv) > 3 and sys.argv[3] == "goal":
    sys.exit(goal_mode(n_cfg, int(sys.argv[2])))
if len(sys.argv) > 3 and sys.argv[3] == "bank":
    sys.exit(bank_mode(n_cfg, int(sys.argv[2])))
if len(sys.argv) > 3 and sys.argv[3] in FUZZ_FAMILIES:
    sys.exit(family_mode(sys.argv[3], n_cfg, int(sys.argv[2])))
limit_events = {}
one_launch_steps = 0
two_kernel_forms = 0                                            # (rcw_set_top_view_form: by default it is taken only from 256 MiB a step)
fails = 0
O.set_num_threads(8)
for c in range(n_cfg):
    if c % 10 == 0:
        print(f"config {c} ...", flush=True)
    T64 = bool(rng.integers(0, 2))
    radius = float(rng.choice([1 / 8, 0.05, 0.2, 0.3, 0.49]))
    inc = float(rng.choice([1 / 8, 1 / 16, 0.1, 0.03, radius]))
    kw = dict(height_tile_map_tu=int(rng.integers(4, 24)), width_tile_map_tu=int(rng.integers(4, 24)),
              num_rays=int(rng.choice([1, 2, 7, 64, 100, 256, 333])), num_directions=int(rng.choice([4, 16, 36, 128, 360])),
              player_radius_wu=radius, position_increment_wu=min(inc, radius),
              semi_field_of_view_wu=float(rng.choice([2 / 3, 0.25, 1.0, 1.7])),
              camera_height_tile_wu=float(rng.choice([1.0, 0.5, 2.5])),
              height_camera_view_pu=int(rng.choice([256, 64, 100, 37, 512, 128, 84, 768])),
              dda_tie_break=int(rng.integers(0, 2)), dda_distance=int(rng.integers(0, 2)),
              normalize_mode=int(rng.integers(0, 2)), out_of_bounds=int(rng.integers(0, 2)),
              auto_reset=bool(rng.integers(0, 2)), render_top_view=bool(rng.integers(0, 4) == 0) or always_top,
              pu_per_tu=int(rng.choice([4, 8, 13, 32, 40, 52] if always_top else [4, 8, 13, 32])))
    R = str(rng.choice(["Float32", "Float64", "Int32", "Int64"]))
    B = int(rng.integers(1, 40))
    if limit_geometry:                                      # (draws of its own: the other modes' stay what they were for a given seed)
        kw.update(height_camera_view_pu=int(rng.choice([256, 256, 256, 64, 128, 512])), render_top_view=False, num_rays=int(rng.choice([1, 7, 64, 100, 255, 256, 257, 333, 512, 700, 1024, 1100, 1500])),
                  height_tile_map_tu=int(rng.integers(3, 41)), width_tile_map_tu=int(rng.integers(3, 41)))
        B = int(rng.choice([1, 3, 4, 5, 17]))
        L = int(rng.choice([1, 2, 3, 7, 20]))
    if step_geometry:
        kw.update(height_camera_view_pu=int(rng.choice([256, 256, 256, 64, 128, 512, 768, 1024, 2048])), render_top_view=False, num_rays=int(rng.choice([1, 7, 64, 100, 255, 256, 257, 333, 512, 700, 1024, 1100, 1500])),
                  height_tile_map_tu=int(rng.integers(3, 41)), width_tile_map_tu=int(rng.integers(3, 41)))
        B = int(rng.choice([1, 3, 4, 5, 17, 64, 130]))
    if split_geometry:
        # image heights of 32 m rows with tiles that divide the store kernel's unit (256, 128, 64 or 32 rows)
        pu = int(rng.choice([8, 16, 32, 32, 64, 128]))
        kw["pu_per_tu"] = pu
        m = int(rng.integers(2, 25))
        H = max(4, (32 * m) // pu) if pu <= 64 else int(rng.integers(4, 7)) // 2 * 2
        kw["height_tile_map_tu"] = H
        kw["width_tile_map_tu"] = int(rng.integers(4, 10 if pu >= 64 else 20))
        B = int(rng.integers(1, 12 if pu >= 64 else 40))
    if flat_geometry:
        pu = int(rng.integers(9, 61))
        kw["pu_per_tu"] = pu
        H = int(rng.integers(4, 20))
        if (H * pu) % 4:                                   # image height a multiple of 4
            H += (4 - H % 4) % 4 if pu % 2 else (2 - H % 2) % 2
        kw["height_tile_map_tu"] = max(H, 4)
        kw["width_tile_map_tu"] = int(rng.integers(4, 14))
        kw["height_camera_view_pu"] = int(rng.choice([int(rng.integers(24, 700)), int(rng.integers(24, 48)), 84, 100, 250, 300, 333, 40]))
        B = int(rng.integers(1, 30))
    seed = int(rng.integers(0, 2**31))
    okw = {k: v for k, v in kw.items()}
    okw["auto_reset"] = int(kw["auto_reset"]); okw["render_top_view"] = int(kw["render_top_view"])
    okw["reward_type"] = ["Float32", "Float64", "Int32", "Int64"].index(R)
    if T64:
        okw["world_unit_bits"] = 64
        for k in ("player_radius_wu", "position_increment_wu", "semi_field_of_view_wu", "camera_height_tile_wu"):
            okw[k + "_f64"] = float(kw[k])
    try:
        env = RCW.SingleRoomModule.SingleRoom(batch=B, seed=seed, T="Float64" if T64 else "Float32", R=R, **kw)
        orc = O.OracleBatch(B, seed=seed, **okw)
        assert_state_equal(env, orc, rays=True, where="create")
        ref = None
        if limit_geometry:
            env.set_time_limit(L)
            ref = TL.TimeLimitRef(orc, L, seed, kw["auto_reset"])

        def words(where):
            np.testing.assert_array_equal(env.world.episode_steps, ref.episode_steps, err_msg=f"episode_steps {where}")
            np.testing.assert_array_equal(env.world.truncated.astype(np.uint8), ref.truncated, err_msg=f"truncated {where}")
        if kw["render_top_view"] and (split_geometry or flat_geometry or rng.integers(0, 2)):
            try:
                env.set_top_view_form("two-kernels", runs=int(rng.integers(0, 4)))
                two_kernel_forms += 1
            except Exception:                                  # the geometry does not take it: the automatic form stays
                pass
        if step_geometry or limit_geometry or rng.integers(0, 2):               # the one-launch step (these batches are below where the rule takes it by itself)
            try:
                env.set_step_form("one-launch")
                one_launch_steps += 1
            except Exception:                                  # another camera height / a top view: the two launches stay
                pass
        if rng.integers(0, 2):
            # arbitrary injected poses: uniform, exactly on tile boundaries, a hair off them, tile centres,
            # possibly inside the goal tile (a ray that starts inside an obstacle)
            H, W = kw["height_tile_map_tu"], kw["width_tile_map_tu"]
            real = np.float64 if T64 else np.float32
            def coords(n, hi):
                kind = rng.integers(0, 4, n)
                u = rng.uniform(1.0, hi - 1.0, n)
                k = rng.integers(1, hi - 1, n).astype(np.float64)
                eps = rng.choice([1e-7, -1e-7, 1e-12, 3e-5], n)
                out = np.where(kind == 0, u, np.where(kind == 1, k, np.where(kind == 2, k + eps, k + 0.5)))
                out = np.clip(out, 1.0, np.nextafter(real(hi - 1), real(0))).astype(real)
                return np.where(out < 1, real(1), out)
            pos = np.stack([coords(B, H), coords(B, W)], axis=1).astype(real)
            goal = np.stack([rng.integers(2, H, B), rng.integers(2, W, B)], axis=1).astype(np.int32)
            d = rng.integers(0, kw["num_directions"], B).astype(np.int32)
            env.set_state(goal, pos, d)
            orc.set_state(goal, pos, d)
            if ref is not None:
                ref.clear()
            assert_state_equal(env, orc, rays=True, where="set_state with arbitrary poses")
        for s in range(int(rng.integers(5, 60))):
            if rng.integers(0, 12) == 0:                       # a masked reset with a fresh seed now and then
                mask = (rng.random(B) < 0.4).astype(np.uint8)
                sd = int(rng.integers(0, 2**31))
                RCW.reset_(env, mask=mask, seed=sd)
                orc.reset(mask=mask, seed=sd)
                if ref is not None:
                    ref.clear(mask); ref.seed = sd
                    assert_state_equal(env, orc, rays=True, where=f"masked reset in front of step {s}")
                    np.testing.assert_array_equal(env.world.episode, orc.episode)
                    words(f"masked reset in front of step {s}")
            a = rng.integers(1, 5, B).astype(np.uint8)
            RCW.act_(env, a)
            if ref is not None:
                ref.step(a)                                    # (both BoundsError policies: the helper reads who raised from the status words)
            else:
                assert orc.step(a) == 0
            try:
                env.sync()
            except IndexError:
                np.testing.assert_array_equal(env.world.status, orc.status)
                env.clear_error(); orc.clear_status()
        assert_state_equal(env, orc, rays=True, where="rollout")
        np.testing.assert_array_equal(env.world.episode, orc.episode)
        if ref is not None:
            words("rollout")
            for k, v in ref.events.items():
                limit_events[k] = limit_events.get(k, 0) + v
        if kw["render_top_view"]:
            np.testing.assert_array_equal(env.top_view_host(), orc.top_view)
        env.close(); orc.close()
    except Exception as e:   # noqa: BLE001
        fails += 1
        print(f"config {c} FAILED: T64={T64} R={R} B={B} seed={seed}{f' L={L}' if limit_geometry else ''} {kw}\n   {type(e).__name__}: {str(e)[:300]}")
        if fails >= 5:
            break
limit_words = "; time limit: " + ", ".join(f"{v} {k}" for k, v in limit_events.items()) if limit_geometry else ""
print(f"{n_cfg} random configurations ({two_kernel_forms} with the two-kernel top view asked for and taken, {one_launch_steps} with the one-launch step{limit_words}), {fails} mismatches")
sys.exit(1 if fails else 0)
