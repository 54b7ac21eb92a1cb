"""What episode statistics (rcw_set_episode_stats) add to a step, timed like tools/local_map_bench.py: device-resident U{1..4} actions, HIP
events on the engine's stream around `--steps` steps after `--warmup`.  Each case runs `--repeats` times, interleaved; the JSON carries
every run, the median and the range, and the differences of the medians.

    python tools/episode_stats_bench.py --steps 200 --warmup 40 --repeats 5 [--out profiles/episode_stats_bench.json]

Cases, all at bench.py's geometry (8x8 map, 256 view columns, 4096 agents) under auto_reset, with a time limit of 32 steps, a wall bank and
the goal distance on:
    bank2, bank200               the statistics off, a bank of 2 / of 200 layouts
    bank2_stats, bank200_stats   the statistics on: the table has 2 / 200 level rows
    bank2_torch                  the statistics off and the caller's alternative: the same bookkeeping per step in eager torch on the device
                                 pointers the engine hands out (done, truncated, episode_steps, wall_layout, goal_start_distance) — outcome,
                                 length and level of every close and the table's sums by index_add_.  The engine hands out no device pointer
                                 for the position, so this form has no `moves` and puts the length in SPL's path: it does LESS than the
                                 kernel.
`*_stats_added_us` = *_stats - the base; `bank2_torch_added_us` = bank2_torch - bank2.  `torch_totals` / `stats_totals`: episodes,
successes, truncations, sum_length of the last run of either form (the same seed and actions: they agree where the forms are alike)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG2 = dict(height_tile_map_tu=8, width_tile_map_tu=8, num_rays=256)
LIMIT = 32
CASES = {
    "bank2": dict(layouts=2),
    "bank2_stats": dict(layouts=2, stats=True),
    "bank2_torch": dict(layouts=2, torch_stats=True),
    "bank200": dict(layouts=200),
    "bank200_stats": dict(layouts=200, stats=True),
}


def make_bank(np, H, W, layouts):
    """the ring plus random pillars, every interior tile a wall with probability 0.15"""
    rng = np.random.default_rng(7)
    w = np.zeros((layouts, H, W), bool)
    w[:, [0, -1], :] = True
    w[:, :, [0, -1]] = True
    w[:, 1:-1, 1:-1] |= rng.random((layouts, H - 2, W - 2)) < 0.15
    return w


class TorchStats:
    """The caller's alternative: what the table's first four columns and the per-agent words need, in eager torch behind every step."""

    def __init__(self, RCW, torch, env, rows):
        self.torch = torch
        B = env.batch
        self.done = env.done_device().torch(sync=False)
        self.truncated = env.truncated_device().torch(sync=False)
        steps = env.episode_steps_device()                                     # (UInt32 below 2^31: read as Int32, a type every torch computes with)
        self.steps = RCW.SingleRoomModule.DeviceArray(steps.ptr, steps.shape, "int32", env, env._sync).torch(sync=False)
        self.layout = env.wall_layout.torch(sync=False)
        self.start = env.goal_start_distance.torch(sync=False)
        self.closed = torch.zeros(B, dtype=torch.bool, device=self.done.device)
        self.outcome = torch.zeros(B, dtype=torch.uint8, device=self.done.device)
        self.length = torch.zeros(B, dtype=torch.int64, device=self.done.device)
        self.level = torch.full((B,), -1, dtype=torch.int64, device=self.done.device)
        self.spl = torch.zeros(B, dtype=torch.float64, device=self.done.device)
        self.table = torch.zeros((1 + rows, 7), dtype=torch.int64, device=self.done.device)

    def __call__(self):
        torch = self.torch
        done, over = self.done != 0, (self.done != 0) | (self.truncated != 0)
        closing = over & ~self.closed                                          # (a closed agent restarts with the next call: `over` drops)
        self.closed = over
        length = self.steps.long()
        self.outcome = torch.where(closing, torch.where(done, 1, 2).to(torch.uint8), self.outcome)
        self.length = torch.where(closing, length, self.length)
        self.level = torch.where(closing, self.layout.long(), self.level)
        l = self.start.double()
        defined = closing & (self.start >= 1)
        spl = torch.where(defined & done, torch.floor(65536.0 * l / torch.maximum(length.double() * 0.125, l)), torch.zeros_like(l))
        self.spl = torch.where(closing, spl, self.spl)
        add = torch.stack([closing, closing & done, closing & ~done, closing * length, closing * length, defined, spl.long() * defined], 1).long()
        self.table[0] += add.sum(0)
        self.table.index_add_(0, 1 + self.layout.long(), add)


def run_case(RCW, torch, np, name, batch, steps, warmup, actions, banks):
    kw = CASES[name]
    env = RCW.SingleRoomModule.SingleRoom(batch=batch, seed=0, auto_reset=True, **CFG2)
    env.set_wall_bank(banks[kw["layouts"]])
    env.set_time_limit(LIMIT)
    stream = torch.cuda.Stream()
    env.set_stream(stream.cuda_stream)
    totals = None
    with torch.cuda.stream(stream):
        env.set_goal_distance(True)
        if kw.get("stats"):
            env.set_episode_stats(True)
        book = TorchStats(RCW, torch, env, kw["layouts"]) if kw.get("torch_stats") else None
        for s in range(warmup):
            RCW.act_(env, actions[s % len(actions)])
            if book:
                book()
        stream.synchronize()
        env.timer_start()
        for s in range(steps):
            RCW.act_(env, actions[(warmup + s) % len(actions)])
            if book:
                book()
        ms = env.timer_stop()
        stream.synchronize()
        try:
            env.sync()
        except IndexError:                               # (the default radius and increment reach the reference's BoundsError: sticky, harmless here)
            env.clear_error()
        if book:
            totals = [int(v) for v in book.table[0, :4].tolist()]
        if kw.get("stats"):
            t = env.episode_stats_table()["totals"]
            totals = [t["episodes"], t["successes"], t["truncations"], t["sum_length"]]
    form = env.step_form()
    env.close()
    return ms, form, totals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--case", choices=sorted(CASES), action="append", default=None, help="run these cases only")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    import numpy as np
    import torch

    import raycastworlds_jl_amd as RCW

    g = torch.Generator().manual_seed(0)
    actions = [torch.randint(1, 5, (args.batch,), dtype=torch.uint8, generator=g).cuda() for _ in range(64)]
    banks = {n: make_bank(np, 8, 8, n) for n in (2, 200)}
    names = args.case or list(CASES)
    runs, forms, totals = {n: [] for n in names}, {}, {}
    for _ in range(args.repeats):
        for n in names:
            ms, forms[n], totals[n] = run_case(RCW, torch, np, n, args.batch, args.steps, args.warmup, actions, banks)
            runs[n].append(ms * 1000.0 / args.steps)
    out = {"metric": "us per step", "device": torch.cuda.get_device_name(0),
           "config": f"cfg-2: 8x8 map, 256 view columns, 256 rows, {args.batch} agents; time limit {LIMIT}, a wall bank of 2 / 200 layouts, goal distance on",
           "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "cases": {}}
    for n in names:
        r = np.array(runs[n])
        out["cases"][n] = {"batch": args.batch, "us_median": float(np.median(r)), "us_min": float(r.min()), "us_max": float(r.max()),
                           "env_steps_per_s_median": float(args.batch / np.median(r) * 1e6), "step_form": forms[n], "runs_us": [float(x) for x in r]}
        if totals[n] is not None:
            out["cases"][n]["totals_episodes_successes_truncations_sum_length"] = totals[n]
    c = out["cases"]
    for on, under in (("bank2_stats", "bank2"), ("bank200_stats", "bank200"), ("bank2_torch", "bank2")):
        if on in c and under in c:
            out[f"{on}_added_us"] = c[on]["us_median"] - c[under]["us_median"]
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
