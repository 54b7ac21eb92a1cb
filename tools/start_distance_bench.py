"""What the start rule (rcw_set_start_distance) costs a step, timed like tools/guide_bench.py: HIP events on the engine's stream around
`--steps` steps after `--warmup`.  Each case runs `--repeats` times, interleaved; the JSON carries every run, the median and the range, and
the differences of the medians.

    python tools/start_distance_bench.py --steps 200 --warmup 20 --repeats 5 [--out profiles/start_distance_bench.json]

At BASELINE.json's configuration 2 (8x8 map, 256 view columns, 4096 agents) with layouts.four_rooms, auto_reset and a time limit of 50 —
restarts, and with them floods, happen inside the timed steps, the same in every case —, in both step forms:
    off          neither feature: device-resident U{1..4} actions
    start        the start rule on, band (3, 4): its kernel and the masked re-render of whom it placed, three more launches a step
    gd           the goal distance on (the nearest kernel of the same shape: a wavefront per agent, a flood in LDS for a restarted one)
    gd_start     both: a restart floods twice
The cases of a form draw the same actions, but `start` and `gd_start` place the agents elsewhere: the states differ from `off`'s from the
first restart on, the number of restarts a step (one in 51 of the agents) does not.

`bounds_error_word_set`: every case of this configuration, `off` and a ring-only map included, ends with the handle's sticky error word
set.  It is the reference's own BoundsError at its default player_radius_wu = position_increment_wu = 1/8 on a map 8 tiles wide: an agent
at distance 1/8 from the ring (y = 6.875 facing +y) that moves forward would stand ON the ring's edge (y = 7.0, tile 8 = W), whose 3 x 3
collision neighbourhood leaves the map — is_player_colliding indexes the map before it tests, so the reference raises there, and the engine
(out_of_bounds = 0, the default) leaves that agent as it was and sets its status word and the error word.  A handful of 4096 agents in a
run; the step's launches are the same either way, so the timing is of the ordinary step.  The tool clears the word and reports it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH, LIMIT, BAND = 4096, 50, (3, 4)
CFG = dict(height_tile_map_tu=8, width_tile_map_tu=8, num_rays=256)
CASES = ("off", "start", "gd", "gd_start")
FORMS = ("one-launch", "two-launches")


def run_case(RCW, torch, case, form, steps, warmup, actions):
    env = RCW.SingleRoomModule.SingleRoom(batch=BATCH, seed=0, auto_reset=True, max_episode_steps=LIMIT, walls=RCW.layouts.four_rooms(8, 8), **CFG)
    env.set_step_form(form)
    stream = torch.cuda.Stream()
    env.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        if case in ("gd", "gd_start"):
            env.set_goal_distance(True)
        if case in ("start", "gd_start"):
            env.set_start_distance(*BAND)
        for s in range(warmup + LIMIT):                     # (every agent's first truncation lies in the warm-up)
            RCW.act_(env, actions[s % len(actions)])
        stream.synchronize()
        env.timer_start()
        for s in range(steps):
            RCW.act_(env, actions[(warmup + LIMIT + s) % len(actions)])
        ms = env.timer_stop()
        stream.synchronize()
    assert env.step_form() == form
    raised = False
    try:                                                    # (the sticky error word: a step of some agent raised the reference's BoundsError)
        env.sync()
    except IndexError:
        raised = True
        env.clear_error()
    episodes = float(env.world.episode.mean())
    env.close()
    return ms, episodes, raised


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    import numpy as np
    import torch

    import raycastworlds_jl_amd as RCW

    if not torch.cuda.is_available():
        sys.exit("start_distance_bench: no GPU; a timing taken anywhere else says nothing")
    g = torch.Generator().manual_seed(0)
    actions = [torch.randint(1, 5, (BATCH,), dtype=torch.uint8, generator=g).cuda() for _ in range(64)]
    out = {"metric": "us per step (HIP events around `steps` steps)", "steps": args.steps, "warmup": args.warmup + LIMIT, "repeats": args.repeats,
           "time_limit": LIMIT, "walls": "layouts.four_rooms(8, 8)", "band": list(BAND), "batch": BATCH, **CFG, "device": None, "forms": {}}
    for form in FORMS:
        runs, episodes, raised = {n: [] for n in CASES}, {}, {}
        for _ in range(args.repeats):
            for n in CASES:
                ms, episodes[n], raised[n] = run_case(RCW, torch, n, form, args.steps, args.warmup, actions)
                runs[n].append(ms * 1000.0 / args.steps)
        block = {"cases": {}}
        for n in CASES:
            r = np.array(runs[n])
            block["cases"][n] = {"us_per_step_median": float(np.median(r)), "us_per_step_min": float(r.min()), "us_per_step_max": float(r.max()),
                                 "mean_episode_counter_at_the_end": episodes[n], "bounds_error_word_set": raised[n], "us_per_step_runs": [float(x) for x in r]}
        k = block["cases"]
        block["start_added_us_per_step"] = k["start"]["us_per_step_median"] - k["off"]["us_per_step_median"]
        block["goal_distance_added_us_per_step"] = k["gd"]["us_per_step_median"] - k["off"]["us_per_step_median"]
        block["start_added_beside_goal_distance_us_per_step"] = k["gd_start"]["us_per_step_median"] - k["gd"]["us_per_step_median"]
        out["forms"][form] = block
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
