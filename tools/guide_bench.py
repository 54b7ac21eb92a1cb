"""What the guide (rcw_set_guide) costs a step, timed like tools/goal_distance_bench.py: HIP events on the engine's stream around `--steps`
steps after `--warmup`.  Each case runs `--repeats` times, interleaved; the JSON carries every run, the median and the range, and the
differences of the medians.

    python tools/guide_bench.py --steps 200 --warmup 20 --repeats 5 [--parent-tree PATH] [--out profiles/guide_bench.json]

At BASELINE.json's configurations 1 (8x8 map, 64 view columns, 1 agent), 3 (16x16, 512 columns, 16384 agents) and 5 (32x32, 1024
columns, 8192 agents), all under auto_reset, a generated maze per episode (rcw_set_wall_generator, loops 0.1) and a time limit of 200 —
restarts, and with them floods, happen inside the timed steps, the same in every case of a configuration:
    off          neither feature: device-resident U{1..4} actions
    gd           the goal distance on: one more launch a step
    gd_guide     ... and the guide: one more again; the same random actions, so the three cases step through the same states
    follow       gd_guide fed its own guide_action, no host in the loop: what a DAgger expert or a baseline run costs (other states: the
                 agents arrive, and restart, far more often)
    off_parent / off_child   with --parent-tree, a built checkout of the commit before (its binding cannot load this library, nor this one
                 its): `off` in a child process a repeat, this tree's package and the parent's in turn — a handle without the guide must
                 cost what it did.  Compare these two with each other, not with the in-process `off`.
`enable_us`: rcw_set_guide(h, 1) alone — every agent's words once — between two events, median of the repeats."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.environ.get("RCW_BENCH_TREE") or ROOT            # (the child processes of --parent-tree: which checkout's package to import)
sys.path.insert(0, TREE)

CONFIGS = {
    "cfg1": dict(batch=1, cfg=dict(height_tile_map_tu=8, width_tile_map_tu=8, num_rays=64)),
    "cfg3": dict(batch=16384, cfg=dict(height_tile_map_tu=16, width_tile_map_tu=16, num_rays=512)),
    "cfg5": dict(batch=8192, cfg=dict(height_tile_map_tu=32, width_tile_map_tu=32, num_rays=1024)),
}
CASES = ("off", "gd", "gd_guide", "follow")
LIMIT = 200


def run_case(RCW, torch, case, config, steps, warmup, actions):
    c = CONFIGS[config]
    env = RCW.SingleRoomModule.SingleRoom(batch=c["batch"], seed=0, auto_reset=True, max_episode_steps=LIMIT, wall_generator=dict(loops=0.1),
                                          **c["cfg"])
    stream = torch.cuda.Stream()
    env.set_stream(stream.cuda_stream)
    enable_us = None
    with torch.cuda.stream(stream):
        if case in ("gd", "gd_guide", "follow"):
            env.set_goal_distance(True)
        if case in ("gd_guide", "follow"):
            stream.synchronize()
            env.timer_start()
            env.set_guide(True)
            enable_us = env.timer_stop() * 1000.0
        own = env.guide_action.torch(sync=False) if case == "follow" else None

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
    try:
        env.sync()
    except IndexError:
        env.clear_error()
    env.close()
    return ms, form, episodes, enable_us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--config", choices=sorted(CONFIGS), action="append", default=None, help="run these configurations only")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the commit before: adds the off_child / off_parent cases")
    ap.add_argument("--only-off", action="store_true", help="(the child processes) the `off` case of every configuration once, one JSON line")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    import numpy as np
    import torch

    import raycastworlds_jl_amd as RCW

    if not torch.cuda.is_available():
        sys.exit("guide_bench: no GPU; a timing taken anywhere else says nothing")
    g = torch.Generator().manual_seed(0)
    configs = args.config or list(CONFIGS)
    cases = ["off"] if args.only_off else list(CASES)
    children = {"off_child": ROOT, "off_parent": args.parent_tree} if args.parent_tree and not args.only_off else {}
    child_runs = {n: {c: [] for c in configs} for n in children}
    out = {"metric": "us per step (HIP events around `steps` steps), and env-steps/s", "steps": args.steps, "warmup": args.warmup + LIMIT,
           "repeats": args.repeats, "time_limit": LIMIT, "walls": "rcw_set_wall_generator(loops=0.1)", "device": None, "configs": {}}
    for config in configs:
        batch = CONFIGS[config]["batch"]
        actions = [torch.randint(1, 5, (batch,), dtype=torch.uint8, generator=g).cuda() for _ in range(64)]
        runs, enable, forms, episodes = {n: [] for n in cases}, {n: [] for n in cases}, {}, {}
        for _ in range(1 if args.only_off else args.repeats):
            for n in cases:
                ms, forms[n], episodes[n], en = run_case(RCW, torch, n, config, args.steps, args.warmup, actions)
                runs[n].append(ms * 1000.0 / args.steps)
                if en is not None:
                    enable[n].append(en)
        block = {"batch": batch, **CONFIGS[config]["cfg"], "cases": {}}
        for n in cases:
            r = np.array(runs[n])
            block["cases"][n] = {"us_per_step_median": float(np.median(r)), "us_per_step_min": float(r.min()), "us_per_step_max": float(r.max()),
                                 "env_steps_per_s_median": float(batch / np.median(r) * 1e6), "step_form": forms[n],
                                 "mean_episode_counter_at_the_end": episodes[n], "us_per_step_runs": [float(x) for x in r]}
            if enable[n]:
                block["cases"][n]["enable_us"] = {"median": float(np.median(enable[n])), "runs": [float(x) for x in enable[n]]}
        k = block["cases"]
        out["configs"][config] = block
        if args.only_off:
            continue
        block["guide_added_us_per_step"] = k["gd_guide"]["us_per_step_median"] - k["gd"]["us_per_step_median"]
        block["goal_distance_added_us_per_step"] = k["gd"]["us_per_step_median"] - k["off"]["us_per_step_median"]
    import subprocess

    for _ in range(args.repeats if children else 0):        # this tree's package and the parent's in turn, a process each
        for n, tree in children.items():
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only-off", "--steps", str(args.steps), "--warmup", str(args.warmup)]
                               + [x for c in configs for x in ("--config", c)], env=dict(os.environ, RCW_BENCH_TREE=os.path.abspath(tree)),
                               capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.exit(f"guide_bench: the {n} child failed:\n{r.stdout[-1000:]}{r.stderr[-2000:]}")
            d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
            for c in configs:
                child_runs[n][c].append(d["configs"][c]["cases"]["off"]["us_per_step_median"])
    for c in configs if children else []:
        k = out["configs"][c]["cases"]
        for n in children:
            r = np.array(child_runs[n][c])
            k[n] = {"us_per_step_median": float(np.median(r)), "us_per_step_min": float(r.min()), "us_per_step_max": float(r.max()),
                    "us_per_step_runs": [float(x) for x in r]}
        out["configs"][c]["off_child_minus_off_parent_us_per_step"] = k["off_child"]["us_per_step_median"] - k["off_parent"]["us_per_step_median"]
        out["configs"][c]["ranges_overlap"] = bool(k["off_child"]["us_per_step_min"] <= k["off_parent"]["us_per_step_max"]
                                                   and k["off_parent"]["us_per_step_min"] <= k["off_child"]["us_per_step_max"])
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
