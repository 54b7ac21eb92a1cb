"""Env-steps/s with a wall bank, timed like bench.py: device-resident U{1..4} actions, HIP events on the engine's stream around `--steps`
steps after `--warmup`.  Each case runs `--repeats` times (interleaved, so drift hits every case alike); the JSON line carries every run,
the median and the range, and the ratios of the medians.

    python tools/wall_bank_bench.py --repeats 5 [--out profiles/wall_bank_bench.json]

Cases, all under auto_reset:
  at BASELINE cfg-2 (8x8 map, 256 view columns, --batch agents)
    four_rooms           layouts.four_rooms for every agent through set_walls: no bank
    four_rooms_bank      a bank of two layouts (four rooms | two pillars), uniform
  at cfg-5's geometry (32x32 map, 1024 view columns, --maze-batch agents) under a time limit of --limit steps, warmed up past it
    maze                 a maze of its own for every agent through set_walls: no bank, every episode on the same maze
    maze_bank            a bank of --maze-batch mazes, uniform: a new maze per episode, drawn on the device
    maze_host_relayout   what a caller does without the bank: after every step read the episode counters (a host synchronisation) and give
                         whoever restarted another maze with a masked set_walls (a host upload; the counter moves a second time)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG2 = dict(height_tile_map_tu=8, width_tile_map_tu=8, num_rays=256)
CFG5 = dict(height_tile_map_tu=32, width_tile_map_tu=32, num_rays=1024)
CASES = {
    "four_rooms": dict(cfg=CFG2, walls="four_rooms"),
    "four_rooms_bank": dict(cfg=CFG2, bank="two"),
    "maze": dict(cfg=CFG5, big=True, walls="maze"),
    "maze_bank": dict(cfg=CFG5, big=True, bank="maze"),
    "maze_host_relayout": dict(cfg=CFG5, big=True, walls="maze", relayout=True),
}


def make_walls(RCW, np, kind, H, W, batch):
    L = RCW.layouts
    if kind == "four_rooms":
        return L.four_rooms(H, W)
    if kind == "two":
        pillars = L.ring(H, W)
        pillars[2, 2] = pillars[H - 3, W - 3] = True
        return np.stack([L.four_rooms(H, W), pillars])
    return np.stack([L.maze(H, W, np.random.default_rng(1000 + a)) for a in range(batch)])


def run_case(RCW, torch, np, name, batch, steps, warmup, limit, actions, cache):
    kw = CASES[name]
    H, W = kw["cfg"]["height_tile_map_tu"], kw["cfg"]["width_tile_map_tu"]
    env = RCW.SingleRoomModule.SingleRoom(batch=batch, seed=0, auto_reset=True, **kw["cfg"])
    kind = kw.get("walls") or kw.get("bank")
    if (kind, batch) not in cache:
        cache[(kind, batch)] = make_walls(RCW, np, kind, H, W, batch)
    walls = cache[(kind, batch)]
    if "bank" in kw:
        env.set_wall_bank(walls)
    else:
        env.set_walls(walls)
    if kw.get("big"):
        env.set_time_limit(limit)
    relayout = kw.get("relayout", False)
    pick = np.random.default_rng(7)

    def counters():
        try:
            return env.world.episode
        except IndexError:                               # (the default radius and increment reach the reference's BoundsError: sticky, harmless here)
            env.clear_error()
            return env.world.episode

    seen = counters()
    stream = torch.cuda.Stream()
    env.set_stream(stream.cuda_stream)

    def step(s):
        nonlocal seen
        RCW.act_(env, actions[s % len(actions)])
        if relayout:
            episode = counters()                                             # the host synchronisation
            moved = episode != seen
            if moved.any():
                env.set_walls(walls, pick.integers(0, len(walls), batch).astype(np.int32), moved.astype(np.uint8))
            seen = episode + moved                                           # (set_walls moves the counter once more)

    with torch.cuda.stream(stream):
        for s in range(warmup):
            step(s)
        stream.synchronize()
        env.timer_start()
        for s in range(steps):
            step(warmup + s)
        ms = env.timer_stop()
        stream.synchronize()
    form = env.step_form()
    episodes = float(counters().mean())
    layouts = int(len(set(env.wall_layout.numpy().tolist()))) if "bank" in kw else None
    env.close()
    return ms, form, episodes, layouts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=220)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--maze-batch", type=int, default=1024, help="agents (and bank layouts) of the three cfg-5 cases")
    ap.add_argument("--limit", type=int, default=200, help="the time limit of the three cfg-5 cases")
    ap.add_argument("--case", choices=sorted(CASES), default=None, help="run this case only (for a profiler)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    import numpy as np
    import torch

    import raycastworlds_jl_amd as RCW

    g = torch.Generator().manual_seed(0)
    batches = {n: (args.maze_batch if CASES[n].get("big") else args.batch) for n in CASES}
    actions = {b: [torch.randint(1, 5, (b,), dtype=torch.uint8, generator=g).cuda() for _ in range(64)] for b in set(batches.values())}
    names = [args.case] if args.case else list(CASES)
    runs = {n: [] for n in names}
    forms, episodes, layouts, cache = {}, {}, {}, {}
    for _ in range(args.repeats):
        for n in names:
            ms, forms[n], episodes[n], layouts[n] = run_case(RCW, torch, np, n, batches[n], args.steps, args.warmup, args.limit, actions[batches[n]], cache)
            runs[n].append(batches[n] * args.steps / (ms / 1000.0))
    out = {"metric": "env-steps/s", "config": "four_rooms*: cfg-2: 8x8 map, 256 view columns, 256 rows; maze*: cfg-5: 32x32 map, 1024 view columns, "
           f"time limit {args.limit}", "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "cases": {}}
    for n in names:
        r = np.array(runs[n])
        out["cases"][n] = {"batch": batches[n], "median": float(np.median(r)), "min": float(r.min()), "max": float(r.max()),
                           "us_per_step_median": float(batches[n] / np.median(r) * 1e6), "us_per_step_range": [float(batches[n] / r.max() * 1e6), float(batches[n] / r.min() * 1e6)],
                           "step_form": forms[n], "mean_episode_counter_at_the_end": episodes[n], "distinct_layouts_at_the_end": layouts[n],
                           "runs": [float(x) for x in r]}
    med = lambda n: out["cases"][n]["median"]
    for a, b in (("four_rooms_bank", "four_rooms"), ("maze_bank", "maze"), ("maze_bank", "maze_host_relayout"), ("maze_host_relayout", "maze")):
        if a in runs and b in runs:
            out[f"{a}_over_{b}"] = med(a) / med(b)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
