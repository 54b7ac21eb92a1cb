"""Env-steps/s with interior walls, timed like bench.py: device-resident U{1..4} actions, HIP events on the engine's stream around
`--steps` steps after `--warmup`.  Each case runs `--repeats` times (interleaved, so drift hits every case alike); the JSON line carries
every run, the median and the range, and the ratios of the medians against `plain`.

    python tools/walls_bench.py --steps 200 --warmup 20 --repeats 5 [--out profiles/walls_bench.json]

Cases, at BASELINE cfg-2 (8x8 map, 256 view columns, 4096 agents) unless said otherwise, all under auto_reset:
    plain                a handle that never called set_walls
    ring_via_set_walls   the same map through the new call (layouts.ring): the same kernels on the same bits — the check of "no cost"
    four_rooms           layouts.four_rooms for every agent
    maze_plain           cfg-5's geometry (32x32 map, 1024 view columns, --maze-batch agents), no walls: what `maze` is compared with
    maze                 cfg-5's geometry, a maze of its own for every agent (layouts.maze, layouts == batch)
four_rooms and maze are informative: shorter rays and more saturated columns, and more goals reached."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG2 = dict(height_tile_map_tu=8, width_tile_map_tu=8, num_rays=256)
CFG5 = dict(height_tile_map_tu=32, width_tile_map_tu=32, num_rays=1024)
CASES = {
    "plain": dict(cfg=CFG2),
    "ring_via_set_walls": dict(cfg=CFG2, walls="ring"),
    "four_rooms": dict(cfg=CFG2, walls="four_rooms"),
    "maze_plain": dict(cfg=CFG5, big=True),
    "maze": dict(cfg=CFG5, big=True, walls="maze"),
}


def make_walls(RCW, np, kind, H, W, batch):
    L = RCW.layouts
    if kind == "ring":
        return L.ring(H, W)
    if kind == "four_rooms":
        return L.four_rooms(H, W)
    return np.stack([L.maze(H, W, np.random.default_rng(1000 + a)) for a in range(batch)])


def run_case(RCW, torch, np, name, batch, steps, warmup, actions, walls_cache):
    kw = CASES[name]
    env = RCW.SingleRoomModule.SingleRoom(batch=batch, seed=0, auto_reset=True, **kw["cfg"])
    if "walls" in kw:
        key = (kw["walls"], batch)
        if key not in walls_cache:
            walls_cache[key] = make_walls(RCW, np, kw["walls"], kw["cfg"]["height_tile_map_tu"], kw["cfg"]["width_tile_map_tu"], batch)
        env.set_walls(walls_cache[key])
    stream = torch.cuda.Stream()
    env.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        for s in range(warmup):
            RCW.act_(env, actions[s % len(actions)])
        stream.synchronize()
        env.timer_start()
        for s in range(steps):
            RCW.act_(env, actions[(warmup + s) % len(actions)])
        ms = env.timer_stop()
        stream.synchronize()
    form = env.step_form()
    episodes = float(env.world.episode.mean())
    try:
        env.sync()
    except IndexError:                                   # (the default radius and increment reach the reference's BoundsError: sticky, harmless here)
        env.clear_error()
    env.close()
    return ms, form, episodes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--maze-batch", type=int, default=1024, help="agents of the two cfg-5 cases")
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
    forms, episodes, walls_cache = {}, {}, {}
    for _ in range(args.repeats):
        for n in names:
            ms, forms[n], episodes[n] = run_case(RCW, torch, np, n, batches[n], args.steps, args.warmup, actions[batches[n]], walls_cache)
            runs[n].append(batches[n] * args.steps / (ms / 1000.0))
    out = {"metric": "env-steps/s", "config": "cfg-2: 8x8 map, 256 view columns, 256 rows; maze*: cfg-5: 32x32 map, 1024 view columns", "steps": args.steps,
           "warmup": args.warmup, "repeats": args.repeats, "cases": {}}
    for n in names:
        r = np.array(runs[n])
        out["cases"][n] = {"batch": batches[n], "median": float(np.median(r)), "min": float(r.min()), "max": float(r.max()),
                           "us_per_step_median": float(batches[n] / np.median(r) * 1e6), "step_form": forms[n],
                           "mean_episode_counter_at_the_end": episodes[n], "runs": [float(x) for x in r]}
    for n in names:                                      # (maze* against plain compares two geometries: see maze_over_maze_plain)
        if n != "plain" and "plain" in runs:
            out[f"{n}_over_plain"] = out["cases"][n]["median"] / out["cases"]["plain"]["median"]
    if "maze" in runs and "maze_plain" in runs:
        out["maze_over_maze_plain"] = out["cases"]["maze"]["median"] / out["cases"]["maze_plain"]["median"]
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
