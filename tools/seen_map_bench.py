"""What the seen map (rcw_set_seen_map) costs a step, timed like tools/goal_distance_bench.py: device-resident U{1..4} actions, HIP events on
the engine's stream around `--steps` steps after `--warmup`.  Each case runs `--repeats` times, interleaved; the JSON carries every run, the
median and the range, and the differences of the medians.

    python tools/seen_map_bench.py --steps 200 --warmup 20 --repeats 5 [--out profiles/seen_map_bench.json]

Cases, all under auto_reset:
  at BASELINE cfg-2 (8x8 map, 256 view columns, 4096 agents)
    plain            the feature off
    plain_seen       the feature on: one more launch a step
    plain_cast       the yardstick: rcw_cast_rays alone, `--steps` times — the project's own cast-only march over the same rays
  at cfg-5's geometry (32x32 map, 1024 view columns, --maze-batch agents), a maze per agent, time limit 200 (the march is deep; restarts,
  and with them clears, happen inside the timed steps)
    maze, maze_seen, maze_cast   the same three
The seen-map kernel does the yardstick's march plus one LDS atomic per tile crossed plus a pass over H*W / 32 words: `*_seen_added_us` is the
step's time with the feature minus without, `*_cast_us` the yardstick's time per call, `*_added_over_cast` their ratio.
`enable_ms`: rcw_set_seen_map(h, 1) alone — every agent cleared and marked at once — between two events, median of the repeats."""
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
    "plain_seen": dict(cfg=CFG2, seen=True),
    "plain_cast": dict(cfg=CFG2, cast_only=True),
    "maze": dict(cfg=CFG5, big=True, walls="maze", limit=200),
    "maze_seen": dict(cfg=CFG5, big=True, walls="maze", limit=200, seen=True),
    "maze_cast": dict(cfg=CFG5, big=True, walls="maze", limit=200, cast_only=True),
}


def make_walls(RCW, np, H, W, batch):
    return np.stack([RCW.layouts.maze(H, W, np.random.default_rng(1000 + a)) for a in range(batch)])


def run_case(RCW, torch, np, name, batch, steps, warmup, actions, walls_cache):
    kw = CASES[name]
    env = RCW.SingleRoomModule.SingleRoom(batch=batch, seed=0, auto_reset=True, **kw["cfg"])
    if "walls" in kw:
        if batch not in walls_cache:
            walls_cache[batch] = make_walls(RCW, np, kw["cfg"]["height_tile_map_tu"], kw["cfg"]["width_tile_map_tu"], batch)
        env.set_walls(walls_cache[batch])
    if kw.get("limit"):
        env.set_time_limit(kw["limit"])
    stream = torch.cuda.Stream()
    env.set_stream(stream.cuda_stream)
    enable_ms = None
    with torch.cuda.stream(stream):
        if kw.get("seen"):
            stream.synchronize()
            env.timer_start()
            env.set_seen_map(True)
            enable_ms = env.timer_stop()
        warmup += kw.get("limit", 0)                        # (every agent's first truncation lies in the warm-up, its restart in the timed steps)
        for s in range(warmup):
            RCW.act_(env, actions[s % len(actions)])
        stream.synchronize()
        env.timer_start()
        if kw.get("cast_only"):                             # the yardstick: the cast kernel alone on the state the warm-up left
            for s in range(steps):
                env._check(env._lib.rcw_cast_rays(env._h))
        else:
            for s in range(steps):
                RCW.act_(env, actions[(warmup + s) % len(actions)])
        ms = env.timer_stop()
        stream.synchronize()
    form = env.step_form()
    seen = float(env.seen_count.numpy().mean()) if kw.get("seen") else None
    try:
        env.sync()
    except IndexError:                                   # (the default radius and increment reach the reference's BoundsError: sticky, harmless here)
        env.clear_error()
    env.close()
    return ms, form, enable_ms, seen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--maze-batch", type=int, default=1024, help="agents of the three cfg-5 cases")
    ap.add_argument("--case", choices=sorted(CASES), action="append", default=None, help="run these cases only")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    import numpy as np
    import torch

    import raycastworlds_jl_amd as RCW

    g = torch.Generator().manual_seed(0)
    batches = {n: (args.maze_batch if CASES[n].get("big") else args.batch) for n in CASES}
    actions = {b: [torch.randint(1, 5, (b,), dtype=torch.uint8, generator=g).cuda() for _ in range(64)] for b in set(batches.values())}
    names = args.case or list(CASES)
    runs, enable = {n: [] for n in names}, {n: [] for n in names}
    forms, seen, walls_cache = {}, {}, {}
    for _ in range(args.repeats):
        for n in names:
            ms, forms[n], en, seen[n] = run_case(RCW, torch, np, n, batches[n], args.steps, args.warmup, actions[batches[n]], walls_cache)
            runs[n].append(ms * 1000.0 / args.steps)
            if en is not None:
                enable[n].append(en)
    out = {"metric": "us per step (per rcw_cast_rays call in the *_cast cases)", "device": torch.cuda.get_device_name(0),
           "config": "plain*: cfg-2: 8x8 map, 256 view columns, 256 rows; maze*: cfg-5: 32x32 map, 1024 view columns, a maze per agent, limit 200",
           "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "cases": {}}
    for n in names:
        r = np.array(runs[n])
        out["cases"][n] = {"batch": batches[n], "us_median": float(np.median(r)), "us_min": float(r.min()), "us_max": float(r.max()),
                           "env_steps_per_s_median": float(batches[n] / np.median(r) * 1e6), "step_form": forms[n], "runs_us": [float(x) for x in r]}
        if enable[n]:
            out["cases"][n]["enable_ms"] = {"median": float(np.median(enable[n])), "runs": [float(x) for x in enable[n]]}
        if seen[n] is not None:
            out["cases"][n]["mean_seen_count_at_the_end"] = seen[n]
    c = out["cases"]
    for base in ("plain", "maze"):
        on, cast = f"{base}_seen", f"{base}_cast"
        if base in c and on in c:
            out[f"{on}_added_us"] = c[on]["us_median"] - c[base]["us_median"]
            if cast in c:
                out[f"{cast}_us"] = c[cast]["us_median"]
                out[f"{base}_added_over_cast"] = out[f"{on}_added_us"] / c[cast]["us_median"]
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
