"""Env-steps/s of the learner view's cases at BASELINE cfg-2 (8x8 map, 256 view columns, 4096 agents), timed like bench.py:
device-resident U{1..4} actions, HIP events on the engine's stream around `--steps` steps after `--warmup`.  Each case runs
`--repeats` times (interleaved, so drift hits every case alike); the JSON line carries every run, the median and the range.

    python tools/learner_view_bench.py --steps 200 --warmup 20 --repeats 5

Cases: plain (the camera view only), plus_gray84 (camera view + gray 84x84), only_gray84 / only_gray_full / only_rgb_chw_full
(RCW_VIEW_ONLY: the cast kernel and the view kernel); plus_gray84_stack4 / only_gray84_stack4 (the engine's 4-frame stack,
set_learner_view(stack=4)) against plus_gray84_torch_stack4 / only_gray84_torch_stack4: the single-frame view plus a stack kept by torch
ops on the same stream with the same semantics — the done flags of before the step copied, the slots shifted by a cat, all four taken
from the new frame by a where on the agents that were done (those auto_reset re-samples in the step): three launches and two fresh
tensors a step, no host synchronisation.  The depth plane (include/rcw.h): only_depth84 beside only_gray84, only_grayd84_stack4 beside
only_gray84_stack4, and plus_rgbd_full — camera view + RGB-D at full size, CHW —, reported as the bytes of the view over the TIME IT ADDS TO
THE PLAIN STEP (`us_over_plain_step`: the view kernel runs alone on the stream, behind the step's; not the kernel's duration).  The view kernel's own duration comes from a separate rocprofv3 run
(--case NAME runs one case alone, for `rocprofv3 --kernel-trace --stats -- python tools/learner_view_bench.py --case ...`)."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {
    "plain": None,
    "plus_gray84": dict(format="gray", size=(84, 84), layout="chw", camera_view=True),
    "only_gray84": dict(format="gray", size=(84, 84), layout="chw", camera_view=False),
    "only_gray_full": dict(format="gray", size=None, layout="chw", camera_view=False),
    "only_rgb_chw_full": dict(format="rgb", size=None, layout="chw", camera_view=False),
    "plus_gray84_stack4": dict(format="gray", size=(84, 84), layout="chw", camera_view=True, stack=4),
    "only_gray84_stack4": dict(format="gray", size=(84, 84), layout="chw", camera_view=False, stack=4),
    "plus_gray84_torch_stack4": dict(format="gray", size=(84, 84), layout="chw", camera_view=True, torch_stack=4),
    "only_gray84_torch_stack4": dict(format="gray", size=(84, 84), layout="chw", camera_view=False, torch_stack=4),
    "only_depth84": dict(format="depth", size=(84, 84), layout="chw", camera_view=False),
    "only_grayd84_stack4": dict(format="grayd", size=(84, 84), layout="chw", camera_view=False, stack=4),
    "plus_rgbd_full": dict(format="rgbd", size=None, layout="chw", camera_view=True),
}
DEPTH_TWINS = {"only_depth84": "only_gray84", "only_grayd84_stack4": "only_gray84_stack4"}


def run_case(RCW, torch, name, batch, steps, warmup, actions):
    env = RCW.SingleRoomModule.SingleRoom(batch=batch, seed=0, auto_reset=True, height_tile_map_tu=8, width_tile_map_tu=8,
                                          num_rays=256)
    kw = dict(CASES[name] or {})
    k = kw.pop("torch_stack", 0)
    if kw:
        env.set_learner_view(**kw)
    stream = torch.cuda.Stream()
    env.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        if k:                                                   # the stack a user keeps in torch today, on the engine's stream
            view = env.learner_view.torch(sync=False)           # (B, 1, h, w), rewritten in place by every step
            done = env.done_device(as_bool=True).torch(sync=False)
            stack = [view.repeat(1, k, 1, 1)]

            def act(a):
                restarted = done.clone()[:, None, None, None]   # done before the step: re-sampled by it
                RCW.act_(env, a)
                stack[0] = torch.where(restarted, view, torch.cat((stack[0][:, 1:], view), 1))
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
    view_bytes = math.prod(env.learner_view.shape) if kw else 0   # the bytes of the view batch (all its frame slots)
    try:
        env.sync()
    except IndexError:
        env.clear_error()
    env.close()
    return ms, form, view_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--case", choices=sorted(CASES), default=None, help="run this case only (for a profiler)")
    args = ap.parse_args()
    import numpy as np
    import torch

    import raycastworlds_jl_amd as RCW

    g = torch.Generator().manual_seed(0)
    actions = [torch.randint(1, 5, (args.batch,), dtype=torch.uint8, generator=g).cuda() for _ in range(64)]
    names = [args.case] if args.case else list(CASES)
    runs = {n: [] for n in names}
    forms, view_bytes = {}, {}
    for _ in range(args.repeats):
        for n in names:
            ms, forms[n], view_bytes[n] = run_case(RCW, torch, n, args.batch, args.steps, args.warmup, actions)
            runs[n].append(args.batch * args.steps / (ms / 1000.0))
    out = {"metric": "env-steps/s", "config": "cfg-2: 8x8 map, 256 view columns, 256 rows", "batch": args.batch,
           "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "cases": {}}
    for n in names:
        r = np.array(runs[n])
        out["cases"][n] = {"median": float(np.median(r)), "min": float(r.min()), "max": float(r.max()),
                           "us_per_step_median": float(args.batch / np.median(r) * 1e6), "step_form": forms[n], "view_bytes": view_bytes[n],
                           "runs": [float(x) for x in r]}
    for n in names:                                                # the engine's stack against the torch one: faster, and the ranges apart?
        t = n.replace("_stack4", "_torch_stack4")
        if n.endswith("_stack4") and t != n and t in runs:
            e, b = out["cases"][n], out["cases"][t]
            out[n + "_over_torch"] = {"median_ratio": e["median"] / b["median"], "ranges_apart": bool(e["min"] > b["max"])}
    for n, t in DEPTH_TWINS.items():                               # the depth cases beside their colour twins
        if n in runs and t in runs:
            e, b = out["cases"][n], out["cases"][t]
            out[n + "_over_" + t] = {"median_ratio": e["median"] / b["median"],
                                     "us_per_step_more": e["us_per_step_median"] - b["us_per_step_median"]}
    if "plus_rgbd_full" in runs and "plain" in runs:
        us = out["cases"]["plus_rgbd_full"]["us_per_step_median"] - out["cases"]["plain"]["us_per_step_median"]
        nbytes = view_bytes["plus_rgbd_full"]
        out["plus_rgbd_full_view"] = {"bytes": nbytes, "us_over_plain_step": us, "GB_per_s_over_plain_step": nbytes / us / 1e3}
    if "plain" in runs and "only_gray84" in runs:
        out["only_gray84_over_plain"] = out["cases"]["only_gray84"]["median"] / out["cases"]["plain"]["median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
