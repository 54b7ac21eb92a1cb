"""What the state archive's calls cost (rcw_set_snapshots), timed like tools/episode_stats_bench.py: HIP events on the engine's stream around
`--calls` calls of one kind after `--warmup`, every case `--repeats` times, interleaved; the JSON carries every run, the median and the range.

    python tools/snapshot_bench.py --calls 50 --warmup 10 --repeats 5 [--out profiles/snapshot_bench.json]

One handle at bench.py's geometry (8x8 map, 256 view columns, 4096 agents) under auto_reset with a learner view gray 84 x 84, k = 4, the goal
distance, the seen map and a wall bank of 2 layouts; the archive has as many rows as agents.  A record is 28518 bytes in 24 segments
(SEGMENTS below, checked against rcw_snapshot_info), 28224 of them the frame stack.  The device variants throughout:
    save_all             every agent into its own row: the scatter alone
    restore_all          every agent from its own row: the gather AND the render behind it (cast, camera fill, view kernel)
    restore_tenth        a random tenth of the agents (the same mask every call)
    restore_one_row      every agent from row 0
    step                 one step of the same handle, for scale
    plain_copies         THE YARDSTICK: torch's own device-to-device copies of the same 24 segments' bytes for all agents, tensor to tensor, on
                         the engine's stream — a copy, not the kernel under test
    plain_copy_whole     ... and the same bytes as ONE copy
`GB_per_s` counts the bytes read plus the bytes written.  A restore is one call, so the GATHER ALONE comes from the kernel trace: a run of
its own a case,
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/restore_all -- python tools/snapshot_bench.py --case restore_all --repeats 1
(and restore_one_row, restore_tenth, save_all), and `--kernel-stats DIR` then adds, per case found under DIR, the mean time of
rcw_snapshot_copy_kernel and of rcw_snapshot_resolve_kernel to the JSON as `kernel_trace` (calls, mean ns).
`--bench-lines PARENT BRANCH`: two files holding the JSON line of `python bench.py` on the parent and on the branch, copied into the output."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG2 = dict(height_tile_map_tu=8, width_tile_map_tu=8, num_rays=256)
SEGMENTS = [8, 4, 8, 4, 1, 4, 16, 4, 1,                  # pos, dir, goal, reward, done, episode, tile_map, episode_steps, truncated
            128, 4, 4, 4, 4,                             # the goal distance: field, three words, its episode counter
            4, 4, 4, 4, 8, 64,                           # the seen map: three words, its episode counter, bits, map
            4 * 84 * 84, 4,                              # the frame stack and its episode counter
            4, 4]                                        # the layout source: its episode counter, the layout index
CASES = ("save_all", "restore_all", "restore_tenth", "restore_one_row", "step", "plain_copies", "plain_copy_whole")


def kernel_stats(root):
    """per case directory under `root`: rocprofv3's kernel_stats CSV rows of the archive's two kernels — calls and mean ns"""
    import csv
    import glob

    found = {}
    for case in sorted(os.listdir(root)):
        for path in glob.glob(os.path.join(root, case, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row.get("Name", "")
                for kernel in ("rcw_snapshot_copy_kernel", "rcw_snapshot_resolve_kernel"):
                    if kernel in name:
                        found.setdefault(case, {})[kernel] = {"calls": int(row["Calls"]), "mean_ns": float(row["AverageNs"]),
                                                               "min_ns": float(row["MinNs"]), "max_ns": float(row["MaxNs"])}
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--case", choices=CASES, action="append", default=None, help="run these cases only (a kernel trace of one case)")
    ap.add_argument("--kernel-stats", default=None, metavar="DIR", help="rocprofv3 --stats output, a directory a case: merged into the JSON")
    ap.add_argument("--bench-lines", nargs=2, default=None, metavar=("PARENT", "BRANCH"))
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    import numpy as np
    import torch

    import raycastworlds_jl_amd as RCW

    B = args.batch
    env = RCW.SingleRoomModule.SingleRoom(batch=B, seed=0, auto_reset=True, **CFG2)
    walls = np.zeros((2, 8, 8), bool)
    walls[:, [0, -1], :] = True
    walls[:, :, [0, -1]] = True
    walls[1, 3:5, 3:5] = True
    env.set_wall_bank(walls)
    stream = torch.cuda.Stream()
    env.set_stream(stream.cuda_stream)
    out = {"metric": "us per call", "device": torch.cuda.get_device_name(0), "calls": args.calls, "warmup": args.warmup, "repeats": args.repeats,
           "config": f"cfg-2: 8x8 map, 256 view columns, 256 rows, {B} agents; gray 84x84 k=4, goal distance, seen map, a wall bank of 2; {B} rows", "cases": {}}
    with torch.cuda.stream(stream):
        env.set_goal_distance(True)
        env.set_seen_map(True)
        env.set_learner_view("gray", size=(84, 84), stack=4)
        env.set_snapshots(B)
        info = env.snapshot_info
        assert info["row_bytes"] == sum(SEGMENTS), (info, sum(SEGMENTS))
        g = torch.Generator().manual_seed(0)
        actions = [torch.randint(1, 5, (B,), dtype=torch.uint8, generator=g).cuda() for _ in range(16)]
        own = torch.arange(B, dtype=torch.int32).cuda()
        zero = torch.zeros(B, dtype=torch.int32).cuda()
        tenth = (torch.rand(B, generator=g) < 0.1).to(torch.uint8).cuda()
        src = [torch.randint(0, 255, (B * b,), dtype=torch.uint8).cuda() for b in SEGMENTS]
        dst = [torch.empty_like(t) for t in src]
        whole_src, whole_dst = torch.cat(src), torch.empty(B * sum(SEGMENTS), dtype=torch.uint8).cuda()
        for k in range(8):
            RCW.act_(env, actions[k])
        env.snapshot_save(own)
        stream.synchronize()

        def plain():
            for d, s in zip(dst, src):
                d.copy_(s)

        step_k = [0]

        def step():
            step_k[0] += 1
            RCW.act_(env, actions[step_k[0] % len(actions)])

        calls = {"save_all": lambda: env.snapshot_save(own), "restore_all": lambda: env.snapshot_restore(own),
                 "restore_tenth": lambda: env.snapshot_restore(own, tenth), "restore_one_row": lambda: env.snapshot_restore(zero),
                 "step": step, "plain_copies": plain, "plain_copy_whole": lambda: whole_dst.copy_(whole_src)}
        moved = {"save_all": B, "restore_all": B, "restore_tenth": int(tenth.sum().item()), "restore_one_row": B, "plain_copies": B, "plain_copy_whole": B}
        names = args.case or list(CASES)
        runs = {n: [] for n in names}
        for _ in range(args.repeats):
            for n in names:
                for _ in range(args.warmup):
                    calls[n]()
                stream.synchronize()
                env.timer_start()
                for _ in range(args.calls):
                    calls[n]()
                ms = env.timer_stop()
                runs[n].append(ms * 1000.0 / args.calls)
        stream.synchronize()
        try:
            env.sync()
        except IndexError:                               # (the default radius and increment reach the reference's BoundsError: sticky, harmless here)
            env.clear_error()
    out["row_bytes"], out["segments"], out["step_form"] = info["row_bytes"], len(SEGMENTS), env.step_form()
    for n in names:
        r = np.array(runs[n])
        c = out["cases"][n] = {"us_median": float(np.median(r)), "us_min": float(r.min()), "us_max": float(r.max()), "runs_us": [float(x) for x in r]}
        if n in moved:
            c["agents"] = moved[n]
            c["GB_per_s_median"] = float(2 * moved[n] * info["row_bytes"] / np.median(r) / 1e3)
    c = out["cases"]
    if not args.case:
        out["save_all_over_plain_copies"] = c["save_all"]["us_median"] / c["plain_copies"]["us_median"]
        out["save_all_over_plain_copy_whole"] = c["save_all"]["us_median"] / c["plain_copy_whole"]["us_median"]
        out["restore_all_over_step"] = c["restore_all"]["us_median"] / c["step"]["us_median"]
    if args.kernel_stats:
        out["kernel_trace"] = kernel_stats(args.kernel_stats)
    if args.bench_lines:
        for name, path in zip(("bench_parent", "bench_branch"), args.bench_lines):
            with open(path) as f:
                out[name] = json.loads([line for line in f if line.lstrip().startswith("{")][-1])
    env.close()
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
