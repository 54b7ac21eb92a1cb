"""Env-steps/s with and without the episode time limit at BASELINE cfg-2 (8x8 map, 256 view columns, 4096 agents), timed like bench.py:
device-resident U{1..4} actions, HIP events on the engine's stream around `--steps` steps after `--warmup`.  Each case runs `--repeats`
times (interleaved, so drift hits every case alike); the JSON line carries every run, the median and the range.

    python tools/time_limit_bench.py --steps 200 --warmup 20 --repeats 5 [--out profiles/time_limit_bench.json]

Cases: plain (a handle that never set a limit), limit_off (after set_time_limit(0): the same kernels), limit_200 (max_episode_steps = 200,
the form the rule picks: one launch), limit_200_two_launches (the same behind set_step_form("two-launches")), and torch_limit_200 — what
a user does without the engine's limit: a counter kept by torch ops on the engine's stream, the mask of the agents past 200 steps copied
to the HOST every step (rcw_reset takes a host mask) and a masked reset_ whenever it is not empty.  That baseline restarts a step early
and without consuming an action, which the engine's auto_reset contract does not; it is there for its cost, not its semantics."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMIT = 200
CASES = {
    "plain": dict(),
    "limit_off": dict(limit=0),
    "limit_200": dict(limit=LIMIT),
    "limit_200_two_launches": dict(limit=LIMIT, form="two-launches"),
    "torch_limit_200": dict(torch_limit=LIMIT),
}


def run_case(RCW, torch, name, batch, steps, warmup, actions):
    env = RCW.SingleRoomModule.SingleRoom(batch=batch, seed=0, auto_reset=True, height_tile_map_tu=8, width_tile_map_tu=8,
                                          num_rays=256)
    kw = CASES[name]
    if "form" in kw:
        env.set_step_form(kw["form"])
    if "limit" in kw:
        env.set_time_limit(kw["limit"])
    k = kw.get("torch_limit", 0)
    stream = torch.cuda.Stream()
    env.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        if k:
            done = env.done_device(as_bool=True).torch(sync=False)
            count = torch.zeros(batch, dtype=torch.int32, device="cuda")

            def act(a):
                RCW.act_(env, a)
                count.add_(1).masked_fill_(done, 0)
                over = (count >= k).cpu().numpy()                   # the host synchronisation the engine's limit does without
                if over.any():
                    RCW.reset_(env, mask=over.astype("uint8"), seed=0)
                    count.masked_fill_(torch.from_numpy(over).cuda(), 0)
        else:
            def act(a):
                RCW.act_(env, a)
        for s in range(warmup):
            act(actions[s % len(actions)])
        stream.synchronize()
        env.timer_start()
        for s in range(steps):
            act(actions[(warmup + s) % len(actions)])
        ms = env.timer_stop()
        stream.synchronize()
    form = env.step_form()
    truncated = int(env.world.truncated.sum())
    try:
        env.sync()
    except IndexError:
        env.clear_error()
    env.close()
    return ms, form, truncated


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--case", choices=sorted(CASES), default=None, help="run this case only (for a profiler)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    import numpy as np
    import torch

    import raycastworlds_jl_amd as RCW

    g = torch.Generator().manual_seed(0)
    actions = [torch.randint(1, 5, (args.batch,), dtype=torch.uint8, generator=g).cuda() for _ in range(64)]
    names = [args.case] if args.case else list(CASES)
    runs = {n: [] for n in names}
    forms, truncated = {}, {}
    for _ in range(args.repeats):
        for n in names:
            ms, forms[n], truncated[n] = run_case(RCW, torch, n, args.batch, args.steps, args.warmup, actions)
            runs[n].append(args.batch * args.steps / (ms / 1000.0))
    out = {"metric": "env-steps/s", "config": "cfg-2: 8x8 map, 256 view columns, 256 rows", "batch": args.batch, "steps": args.steps,
           "warmup": args.warmup, "repeats": args.repeats, "max_episode_steps": LIMIT, "cases": {}}
    for n in names:
        r = np.array(runs[n])
        out["cases"][n] = {"median": float(np.median(r)), "min": float(r.min()), "max": float(r.max()),
                           "us_per_step_median": float(args.batch / np.median(r) * 1e6), "step_form": forms[n],
                           "truncated_at_the_end": truncated[n], "runs": [float(x) for x in r]}
    if "plain" in runs:
        for n in names:
            if n != "plain":
                out[n + "_over_plain"] = out["cases"][n]["median"] / out["cases"]["plain"]["median"]
    if "limit_200" in runs and "torch_limit_200" in runs:
        out["limit_200_over_torch_limit_200"] = out["cases"]["limit_200"]["median"] / out["cases"]["torch_limit_200"]["median"]
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
