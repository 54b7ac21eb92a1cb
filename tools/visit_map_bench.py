"""What the visit map (rcw_set_visit_map) costs a step, timed like tools/frontier_bench.py: HIP events on the engine's stream around `--steps`
steps after `--warmup`.  Each case runs `--repeats` times, interleaved; the JSON carries every run, the median and the range, and the
differences of the medians.

    python tools/visit_map_bench.py --steps 200 --warmup 20 --repeats 5 [--config cfg1] [--out profiles/visit_map_bench.json]

At BASELINE.json's configurations 1 (8x8 map, 64 view columns, 1 agent), 3 (16x16, 512 columns, 16384 agents) and 5 (32x32, 1024
columns, 8192 agents), all under auto_reset and a time limit of 200 — restarts, and with them clears of a whole map, happen inside the
timed steps, the same in every case of a configuration — with device-resident U{1..4} actions, the same in every case:
    off              a generated maze per episode (rcw_set_wall_generator, loops 0.1), no visit map
    visits           ... and the visit map, one sector: one more launch a step
    visits_sectors8  ... with eight sectors: the same launch, eight times the bytes to clear at a restart
    off_bank         a wall bank of 16 mazes instead of the generator, no visit map
    visits_table     ... and the visit map with its table (16 level rows): two more launches a step, two atomic adds an agent
`stale_agents_a_step`: the agents whose episode counter moved, per timed step (the clears).  `enable_us`: rcw_set_visit_map(h, 1, ...)
alone — the allocation, the table's memset, a BEGIN of every agent — between two events.  Medians of the repeats."""
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
CASES = {"off": None, "visits": dict(sectors=1), "visits_sectors8": dict(sectors=8), "off_bank": None, "visits_table": dict(sectors=1, table=True)}
LIMIT = 200
BANK = 16


def run_case(RCW, torch, np, case, config, steps, warmup, actions):
    c = CONFIGS[config]
    H, W = c["cfg"]["height_tile_map_tu"], c["cfg"]["width_tile_map_tu"]
    rng = np.random.default_rng(0)
    walls = dict(wall_bank=[RCW.layouts.maze(H, W, rng) for _ in range(BANK)]) if case in ("off_bank", "visits_table") else dict(wall_generator=dict(loops=0.1))
    env = RCW.SingleRoomModule.SingleRoom(batch=c["batch"], seed=0, auto_reset=True, max_episode_steps=LIMIT, **walls, **c["cfg"])
    stream = torch.cuda.Stream()
    env.set_stream(stream.cuda_stream)
    enable_us = None
    with torch.cuda.stream(stream):
        if CASES[case] is not None:
            stream.synchronize()
            env.timer_start()
            env.set_visit_map(**CASES[case])
            enable_us = env.timer_stop() * 1000.0
        for s in range(warmup + LIMIT):                     # (every agent's first truncation lies in the warm-up)
            RCW.act_(env, actions[s % len(actions)])
        stream.synchronize()
        before = env.world.episode.astype(np.int64)
        env.timer_start()
        for s in range(steps):
            RCW.act_(env, actions[(warmup + LIMIT + s) % len(actions)])
        ms = env.timer_stop()
        stream.synchronize()
    form = env.step_form()
    stale = float((env.world.episode.astype(np.int64) - before).sum()) / steps
    try:
        env.sync()
    except IndexError:
        env.clear_error()
    env.close()
    return ms, form, stale, enable_us


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
        sys.exit("visit_map_bench: no GPU; a timing taken anywhere else says nothing")
    g = torch.Generator().manual_seed(0)
    configs = args.config or list(CONFIGS)
    out = {"metric": "us per step (HIP events around `steps` steps), and env-steps/s", "steps": args.steps, "warmup": args.warmup + LIMIT,
           "repeats": args.repeats, "time_limit": LIMIT, "walls": f"rcw_set_wall_generator(loops=0.1); off_bank / visits_table: a wall bank of {BANK} mazes",
           "device": None, "configs": {}}
    for config in configs:
        batch = CONFIGS[config]["batch"]
        actions = [torch.randint(1, 5, (batch,), dtype=torch.uint8, generator=g).cuda() for _ in range(64)]
        runs, enable, forms, stale = {n: [] for n in CASES}, {n: [] for n in CASES}, {}, {}
        for _ in range(args.repeats):
            for n in CASES:
                ms, forms[n], stale[n], en = run_case(RCW, torch, np, n, config, args.steps, args.warmup, actions)
                runs[n].append(ms * 1000.0 / args.steps)
                if en is not None:
                    enable[n].append(en)
        block = {"batch": batch, **CONFIGS[config]["cfg"], "cases": {}}
        for n in CASES:
            r = np.array(runs[n])
            block["cases"][n] = {"us_per_step_median": float(np.median(r)), "us_per_step_min": float(r.min()), "us_per_step_max": float(r.max()),
                                 "env_steps_per_s_median": float(batch / np.median(r) * 1e6), "step_form": forms[n], "stale_agents_a_step": stale[n],
                                 "us_per_step_runs": [float(x) for x in r]}
            if enable[n]:
                block["cases"][n]["enable_us"] = {"median": float(np.median(enable[n])), "runs": [float(x) for x in enable[n]]}
        k = block["cases"]
        block["visits_minus_off_us_per_step"] = k["visits"]["us_per_step_median"] - k["off"]["us_per_step_median"]
        block["visits_sectors8_minus_off_us_per_step"] = k["visits_sectors8"]["us_per_step_median"] - k["off"]["us_per_step_median"]
        block["visits_table_minus_off_bank_us_per_step"] = k["visits_table"]["us_per_step_median"] - k["off_bank"]["us_per_step_median"]
        out["configs"][config] = block
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
