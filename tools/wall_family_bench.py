"""Env-steps/s with the wall generator's families — mazes, caves, rooms — beside the case without any and beside each other: device-resident
U{1..4} actions, HIP events on the engine's stream around `--steps` steps after `--warmup`.  Each case runs `--repeats` times (interleaved,
so drift hits every case alike); the JSON carries every run, the median and the range; the text file the table DESIGN.md quotes.

    python tools/wall_family_bench.py --family caves rooms --repeats 5 [--out profiles/wall_rooms_bench]      # writes <out>.json and <out>.txt

`--family` (any of generator, caves, rooms; default: all) selects the cases: the two without a family always, then per family its own two
and its yardstick's.  `--family generator`, `--family caves` and `--family caves rooms` write the keys of profiles/wall_generator_bench.json,
wall_caves_bench.json and wall_rooms_bench.json.

Cases, all under auto_reset:
  at cfg-5's geometry (32x32 map, 1024 view columns, --maze-batch agents) under a time limit of --limit steps, warmed up past it
    maze                 a maze of its own for every agent through set_walls: no source of layouts, every episode on the same maze
    maze_bank            (generator) a bank of --maze-batch mazes, uniform: a new maze per episode, drawn on the device from a finite set
    maze_generator       the wall generator: a new maze per episode, made on the device (15 x 15 = 225 cells)
    caves                the caves at the defaults: a new cave per episode (30 x 30 = 900 interior tiles; none falls back)
    rooms                the rooms at the defaults: new rooms per episode (Q = 15 x 15 = 225 chambers at the most)
  at BASELINE cfg-2 (8x8 map, 256 view columns, --batch agents)
    four_rooms           layouts.four_rooms for every agent through set_walls: no source of layouts
    four_rooms_bank      (generator) a bank of two layouts (four rooms | two pillars), uniform
    generator_8x8        the wall generator (3 x 3 = 9 cells)
    caves_8x8            the caves at the defaults (36 interior tiles; about a quarter fall back to the maze)
    rooms_8x8            the rooms at the defaults (room 2: line 4 alone in each direction, two to four rooms)
The yardstick is run on the same box in the same call — the bank for the generator, the generator for caves and rooms: what a family adds
to a step over the case without any, beside what its yardstick adds.  The installing call (every agent restarts: the bank copies a layout
each, a family makes one each) is timed too, HIP events around --install-repeats calls on a warm handle.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG2 = dict(height_tile_map_tu=8, width_tile_map_tu=8, num_rays=256)
CFG5 = dict(height_tile_map_tu=32, width_tile_map_tu=32, num_rays=1024)
CASES = {                                                                       # install: the setter called with its defaults
    "maze": dict(cfg=CFG5, big=True, walls="maze"),
    "maze_bank": dict(cfg=CFG5, big=True, bank="maze"),
    "maze_generator": dict(cfg=CFG5, big=True, install="set_wall_generator"),
    "caves": dict(cfg=CFG5, big=True, install="set_wall_caves"),
    "rooms": dict(cfg=CFG5, big=True, install="set_wall_rooms"),
    "four_rooms": dict(cfg=CFG2, walls="four_rooms"),
    "four_rooms_bank": dict(cfg=CFG2, bank="two"),
    "generator_8x8": dict(cfg=CFG2, install="set_wall_generator"),
    "caves_8x8": dict(cfg=CFG2, install="set_wall_caves"),
    "rooms_8x8": dict(cfg=CFG2, install="set_wall_rooms"),
}
BASE = {"maze_bank": "maze", "maze_generator": "maze", "caves": "maze", "rooms": "maze",
        "four_rooms_bank": "four_rooms", "generator_8x8": "four_rooms", "caves_8x8": "four_rooms", "rooms_8x8": "four_rooms"}
# family -> its two cases, each with its yardstick (run beside it)
FAMILIES = {"generator": (("maze_generator", "maze_bank"), ("generator_8x8", "four_rooms_bank")),
            "caves": (("caves", "maze_generator"), ("caves_8x8", "generator_8x8")),
            "rooms": (("rooms", "maze_generator"), ("rooms_8x8", "generator_8x8"))}


def make_walls(RCW, np, kind, H, W, batch):
    L = RCW.layouts
    if kind == "four_rooms":
        return L.four_rooms(H, W)
    if kind == "two":
        pillars = L.ring(H, W)
        pillars[2, 2] = pillars[H - 3, W - 3] = True
        return np.stack([L.four_rooms(H, W), pillars])
    return np.stack([L.maze(H, W, np.random.default_rng(1000 + a)) for a in range(batch)])


def run_case(RCW, torch, np, name, batch, steps, warmup, limit, actions, cache, install_repeats):
    kw = CASES[name]
    H, W = kw["cfg"]["height_tile_map_tu"], kw["cfg"]["width_tile_map_tu"]
    env = RCW.SingleRoomModule.SingleRoom(batch=batch, seed=0, auto_reset=True, **kw["cfg"])
    kind = kw.get("walls") or kw.get("bank")
    if kind is not None and (kind, batch) not in cache:
        cache[(kind, batch)] = make_walls(RCW, np, kind, H, W, batch)
    walls = cache.get((kind, batch))
    install = getattr(env, kw["install"]) if "install" in kw else (lambda: env.set_wall_bank(walls)) if "bank" in kw else None
    if install is not None:
        install()
    else:
        env.set_walls(walls)
    if kw.get("big"):
        env.set_time_limit(limit)

    def counters():
        try:
            return env.world.episode
        except IndexError:                               # (the default radius and increment reach the reference's BoundsError: sticky, harmless here)
            env.clear_error()
            return env.world.episode

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
        install_ms = None
        if install is not None and install_repeats:
            install()                                                        # (warm: the buffers of the call before are the allocator's)
            stream.synchronize()
            env.timer_start()
            for _ in range(install_repeats):
                install()
            install_ms = env.timer_stop() / install_repeats
            stream.synchronize()
    form = env.step_form()
    episodes = float(counters().mean())
    distinct = None
    if install is not None:
        distinct = int(len({w.tobytes() for w in env.world.walls}))
    env.close()
    return ms, form, episodes, distinct, install_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=220)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--maze-batch", type=int, default=1024, help="agents (and bank layouts) of the cfg-5 cases")
    ap.add_argument("--limit", type=int, default=200, help="the time limit of the cfg-5 cases")
    ap.add_argument("--install-repeats", type=int, default=3, help="installing calls timed per run (0: none)")
    ap.add_argument("--family", nargs="+", choices=sorted(FAMILIES), default=sorted(FAMILIES), help="the families whose cases run (default: all)")
    ap.add_argument("--case", choices=sorted(CASES), default=None, help="run this case only (for a profiler)")
    ap.add_argument("--out", default=None, help="also write <out>.json and <out>.txt")
    args = ap.parse_args()
    import numpy as np
    import torch

    import raycastworlds_jl_amd as RCW

    g = torch.Generator().manual_seed(0)
    batches = {n: (args.maze_batch if CASES[n].get("big") else args.batch) for n in CASES}
    actions = {b: [torch.randint(1, 5, (b,), dtype=torch.uint8, generator=g).cuda() for _ in range(64)] for b in set(batches.values())}
    pairs = [pair for f in FAMILIES if f in args.family for pair in FAMILIES[f]]
    wanted = {"maze", "four_rooms"} | {n for pair in pairs for n in pair}
    names = [args.case] if args.case else [n for n in CASES if n in wanted]
    runs, installs = {n: [] for n in names}, {n: [] for n in names}
    forms, episodes, distinct, cache = {}, {}, {}, {}
    for _ in range(args.repeats):
        for n in names:
            ms, forms[n], episodes[n], distinct[n], ims = run_case(RCW, torch, np, n, batches[n], args.steps, args.warmup, args.limit,
                                                                   actions[batches[n]], cache, args.install_repeats)
            runs[n].append(batches[n] * args.steps / (ms / 1000.0))
            if ims is not None:
                installs[n].append(ims)
    out = {"metric": "env-steps/s", "config": "maze*, caves, rooms: cfg-5: 32x32 map, 1024 view columns, "
           f"time limit {args.limit}; four_rooms*, *_8x8: cfg-2: 8x8 map, 256 view columns, 256 rows", "families": sorted(args.family), "steps": args.steps, "warmup": args.warmup,
           "repeats": args.repeats, "cases": {}}
    for n in names:
        r = np.array(runs[n])
        out["cases"][n] = {"batch": batches[n], "median": float(np.median(r)), "min": float(r.min()), "max": float(r.max()),
                           "us_per_step_median": float(batches[n] / np.median(r) * 1e6), "us_per_step_range": [float(batches[n] / r.max() * 1e6), float(batches[n] / r.min() * 1e6)],
                           "step_form": forms[n], "mean_episode_counter_at_the_end": episodes[n], "distinct_wall_layouts_at_the_end": distinct[n],
                           "install_ms_median": float(np.median(installs[n])) if installs[n] else None, "install_ms_runs": [float(x) for x in installs[n]],
                           "runs": [float(x) for x in r]}
    us = lambda n: out["cases"][n]["us_per_step_median"]
    for n, base in BASE.items():
        if n in runs and base in runs:
            out[f"{n}_adds_us_per_step_over_{base}"] = us(n) - us(base)
            out[f"{n}_over_{base}"] = out["cases"][n]["median"] / out["cases"][base]["median"]
    for own, yardstick in pairs:
        if own in runs and yardstick in runs:
            out[f"{own}_over_{yardstick}"] = out["cases"][own]["median"] / out["cases"][yardstick]["median"]
            if BASE[yardstick] in runs and "bank" not in CASES[yardstick]:      # (the bank's tool never wrote this one)
                out[f"{own}_adds_over_what_{yardstick}_adds"] = out[f"{own}_adds_us_per_step_over_{BASE[own]}"] / out[f"{yardstick}_adds_us_per_step_over_{BASE[yardstick]}"]
    print(json.dumps(out))
    lines = [out["config"], f"{args.steps} steps after {args.warmup}, {args.repeats} interleaved repeats; medians (range)", "",
             f"{'case':<18}{'agents':>7}{'M env-steps/s':>26}{'us a step':>22}{'adds us':>9}{'install ms':>12}{'layouts':>9}"]
    for n in names:
        c = out["cases"][n]
        adds = out.get(f"{n}_adds_us_per_step_over_{BASE.get(n)}")
        lines.append(f"{n:<18}{c['batch']:>7}{c['median'] / 1e6:>10.2f} ({c['min'] / 1e6:.2f}-{c['max'] / 1e6:.2f})"
                     f"{c['us_per_step_median']:>10.1f} ({c['us_per_step_range'][0]:.1f}-{c['us_per_step_range'][1]:.1f})"
                     f"{'' if adds is None else format(adds, '.1f'):>9}{'' if c['install_ms_median'] is None else format(c['install_ms_median'], '.3f'):>12}"
                     f"{'' if c['distinct_wall_layouts_at_the_end'] is None else c['distinct_wall_layouts_at_the_end']:>9}")
    print("\n".join(lines))
    if args.out:
        with open(args.out + ".json", "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
        with open(args.out + ".txt", "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
