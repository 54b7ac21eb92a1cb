"""What the frontier (rcw_set_frontier) costs a step, timed like tools/guide_bench.py: HIP events on the engine's stream around `--steps`
steps after `--warmup`.  Each case runs `--repeats` times, interleaved; the JSON carries every run, the median and the range, and the
differences of the medians.

    python tools/frontier_bench.py --steps 200 --warmup 20 --repeats 5 [--config cfg1] [--out profiles/frontier_bench.json]

At BASELINE.json's configurations 1 (8x8 map, 64 view columns, 1 agent), 3 (16x16, 512 columns, 16384 agents) and 5 (32x32, 1024
columns, 8192 agents), all under auto_reset, a generated maze per episode (rcw_set_wall_generator, loops 0.1) and a time limit of 200 —
restarts, and with them floods of a fresh map, happen inside the timed steps, the same in every case of a configuration:
    seen            the seen map on: device-resident U{1..4} actions
    seen_frontier   ... and the frontier: two more launches a step (the flood where a map changed, the action words); the same random
                    actions, so the two cases step through the same states
    follow          seen_frontier fed its own explore_action, no host in the loop: what a frontier-following expert costs (other states:
                    the agents keep uncovering tiles, so more of them flood in a step)
`enable_us`: rcw_set_frontier(h, 1) alone — a flood of EVERY agent and all words — between two events, and beside it on the same handle
rcw_set_goal_distance(h, 1) alone, the goal distance's flood of every agent: the yardstick.  Medians of the repeats."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {
    "cfg1": dict(batch=1, cfg=dict(height_tile_map_tu=8, width_tile_map_tu=8, num_rays=64)),
    "cfg3": dict(batch=16384, cfg=dict(height_tile_map_tu=16, width_tile_map_tu=16, num_rays=512)),
    "cfg5": dict(batch=8192, cfg=dict(height_tile_map_tu=32, width_tile_map_tu=32, num_rays=1024)),
}
CASES = ("seen", "seen_frontier", "follow")
LIMIT = 200


def run_case(RCW, torch, case, config, steps, warmup, actions):
    c = CONFIGS[config]
    env = RCW.SingleRoomModule.SingleRoom(batch=c["batch"], seed=0, auto_reset=True, max_episode_steps=LIMIT, wall_generator=dict(loops=0.1),
                                          **c["cfg"])
    stream = torch.cuda.Stream()
    env.set_stream(stream.cuda_stream)
    enable_us = goal_us = None
    with torch.cuda.stream(stream):
        env.set_seen_map(True)
        if case in ("seen_frontier", "follow"):
            for s in range(20):                             # (maps a few steps old, as a flood of every agent finds them in a run)
                RCW.act_(env, actions[s % len(actions)])
            stream.synchronize()
            env.timer_start()
            env.set_frontier(True)
            enable_us = env.timer_stop() * 1000.0
            stream.synchronize()
            env.timer_start()
            env.set_goal_distance(True)
            goal_us = env.timer_stop() * 1000.0
            env.set_goal_distance(False)
        own = env.explore_action.torch(sync=False) if case == "follow" else None

        def step(s):
            RCW.act_(env, own if own is not None else actions[s % len(actions)])

        for s in range(warmup + LIMIT):                     # (every agent's first truncation lies in the warm-up)
            step(s)
        stream.synchronize()
        env.timer_start()
        for s in range(steps):
            step(warmup + LIMIT + s)
        ms = env.timer_stop()
        stream.synchronize()
    form = env.step_form()
    episodes = float(env.world.episode.mean())
    flooded = float((env.seen_new.numpy() != 0).mean())     # (of the last step: the share of agents whose map changed)
    try:
        env.sync()
    except IndexError:
        env.clear_error()
    env.close()
    return ms, form, episodes, flooded, enable_us, goal_us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--config", choices=sorted(CONFIGS), action="append", default=None, help="run these configurations only")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    import numpy as np
    import torch

    import raycastworlds_jl_amd as RCW

    if not torch.cuda.is_available():
        sys.exit("frontier_bench: no GPU; a timing taken anywhere else says nothing")
    g = torch.Generator().manual_seed(0)
    configs = args.config or list(CONFIGS)
    out = {"metric": "us per step (HIP events around `steps` steps), and env-steps/s", "steps": args.steps, "warmup": args.warmup + LIMIT,
           "repeats": args.repeats, "time_limit": LIMIT, "walls": "rcw_set_wall_generator(loops=0.1)", "device": None, "configs": {}}
    for config in configs:
        batch = CONFIGS[config]["batch"]
        actions = [torch.randint(1, 5, (batch,), dtype=torch.uint8, generator=g).cuda() for _ in range(64)]
        runs, enable, goal, forms, episodes, flooded = {n: [] for n in CASES}, {n: [] for n in CASES}, {n: [] for n in CASES}, {}, {}, {}
        for _ in range(args.repeats):
            for n in CASES:
                ms, forms[n], episodes[n], flooded[n], en, gd = run_case(RCW, torch, n, config, args.steps, args.warmup, actions)
                runs[n].append(ms * 1000.0 / args.steps)
                if en is not None:
                    enable[n].append(en)
                    goal[n].append(gd)
        block = {"batch": batch, **CONFIGS[config]["cfg"], "cases": {}}
        for n in CASES:
            r = np.array(runs[n])
            block["cases"][n] = {"us_per_step_median": float(np.median(r)), "us_per_step_min": float(r.min()), "us_per_step_max": float(r.max()),
                                 "env_steps_per_s_median": float(batch / np.median(r) * 1e6), "step_form": forms[n],
                                 "mean_episode_counter_at_the_end": episodes[n], "share_of_agents_whose_map_changed_in_the_last_step": flooded[n],
                                 "us_per_step_runs": [float(x) for x in r]}
            if enable[n]:
                block["cases"][n]["enable_us"] = {"frontier_median": float(np.median(enable[n])), "goal_distance_median": float(np.median(goal[n])),
                                                  "frontier_runs": [float(x) for x in enable[n]], "goal_distance_runs": [float(x) for x in goal[n]]}
        k = block["cases"]
        block["seen_frontier_minus_seen_us_per_step"] = k["seen_frontier"]["us_per_step_median"] - k["seen"]["us_per_step_median"]
        block["follow_minus_seen_us_per_step"] = k["follow"]["us_per_step_median"] - k["seen"]["us_per_step_median"]
        e = k["seen_frontier"]["enable_us"]
        block["flood_of_every_agent_frontier_over_goal_distance"] = e["frontier_median"] / e["goal_distance_median"]
        out["configs"][config] = block
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
