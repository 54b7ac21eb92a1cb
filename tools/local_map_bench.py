"""What the local map (rcw_set_local_map) costs a step, timed like tools/seen_map_bench.py: device-resident U{1..4} actions, HIP events on the
engine's stream around `--steps` steps after `--warmup`.  Each case runs `--repeats` times, interleaved; the JSON carries every run, the
median and the range, and the differences of the medians.

    python tools/local_map_bench.py --steps 200 --warmup 20 --repeats 5 [--out profiles/local_map_bench.json]

Cases, all under auto_reset:
  at BASELINE cfg-2 (8x8 map, 256 view columns, 4096 agents)
    plain              the feature off
    plain_world        RCW_LOCAL_WORLD, S = 16, r = 1: one more launch a step
    plain_seen         the seen map alone (what the next two stand on)
    plain_seen_local   the seen map and RCW_LOCAL_SEEN, S = 32, r = 2: one more launch behind the seen map's
    plain_seen_torch   the seen map and the caller's alternative: the same S = 32, r = 2 crop built per step in torch from
                       env.seen_map_device, a host copy of position and heading (rcw_position, rcw_direction: the engine hands out no device
                       pointer for either) and a copy of the direction table — eager Float32 arithmetic and one gather
  at cfg-5's geometry (32x32 map, 1024 view columns, --maze-batch agents), a maze per agent, time limit 200
    maze, maze_world, maze_seen, maze_seen_local, maze_seen_torch   the same five
`*_world_added_us` = *_world - the base; `*_seen_local_added_us` = *_seen_local - *_seen; `*_seen_torch_added_us` = *_seen_torch - *_seen.
`torch_cells_differing`: cells in which the torch crop of the last step differs from the engine's image (the torch form promises nothing at
a tile boundary; 0 says the comparison is of like with like)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG2 = dict(height_tile_map_tu=8, width_tile_map_tu=8, num_rays=256)
CFG5 = dict(height_tile_map_tu=32, width_tile_map_tu=32, num_rays=1024)
WORLD, SEEN = dict(size=16, cells_per_tile=1, source="world"), dict(size=32, cells_per_tile=2, source="seen")
MAZE = dict(cfg=CFG5, big=True, walls="maze", limit=200)
CASES = {
    "plain": dict(cfg=CFG2),
    "plain_world": dict(cfg=CFG2, local=WORLD),
    "plain_seen": dict(cfg=CFG2, seen=True),
    "plain_seen_local": dict(cfg=CFG2, seen=True, local=SEEN),
    "plain_seen_torch": dict(cfg=CFG2, seen=True, torch_crop=SEEN),
    "maze": dict(MAZE),
    "maze_world": dict(MAZE, local=WORLD),
    "maze_seen": dict(MAZE, seen=True),
    "maze_seen_local": dict(MAZE, seen=True, local=SEEN),
    "maze_seen_torch": dict(MAZE, seen=True, torch_crop=SEEN),
}


def make_walls(RCW, np, H, W, batch):
    return np.stack([RCW.layouts.maze(H, W, np.random.default_rng(1000 + a)) for a in range(batch)])


class TorchCrop:
    """The caller's alternative: the crop of include/rcw.h's formulas in eager torch, from what the engine hands out today."""

    def __init__(self, torch, env, size, cells_per_tile):
        self.torch, self.env = torch, env
        S, r = size, cells_per_tile
        H, W = env.cfg.height_tile_map_tu, env.cfg.width_tile_map_tu
        self.H, self.W, self.S = H, W, S
        off = torch.tensor([(2 * k + 1 - S) / (2 * r) for k in range(S)], dtype=torch.float32).flip(0).cuda()
        self.a, self.l = off.view(1, S, 1), off.view(1, 1, S)
        self.table = torch.from_numpy(env.world.directions_wu).cuda()
        self.seen = env.seen_map_device.torch(sync=False).view(env.batch, H * W)

    def __call__(self):
        torch, w = self.torch, self.env.world
        pos = torch.from_numpy(w.player_position_wu).cuda(non_blocking=True)        # (host copies: each waits for the engine's stream)
        d = self.table[torch.from_numpy(w.player_direction_au).cuda(non_blocking=True).long()]
        px, py, d1, d2 = (v.view(-1, 1, 1) for v in (pos[:, 0], pos[:, 1], d[:, 0], d[:, 1]))
        wx = (px + self.a * d1) + self.l * d2
        wy = (py + self.a * d2) - self.l * d1
        fx, fy = torch.floor(wx), torch.floor(wy)
        inside = (fx >= 0) & (fx < self.H) & (fy >= 0) & (fy < self.W)
        t = torch.where(inside, fx, torch.zeros_like(fx)).long() + self.H * torch.where(inside, fy, torch.zeros_like(fy)).long()
        got = torch.gather(self.seen, 1, t.view(-1, self.S * self.S)).view(-1, self.S, self.S)
        return torch.where(inside, got, torch.zeros_like(got))


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
    enable_ms, differing = None, None
    with torch.cuda.stream(stream):
        if kw.get("seen"):
            env.set_seen_map(True)
        if kw.get("local"):
            stream.synchronize()
            env.timer_start()
            env.set_local_map(**kw["local"])
            enable_ms = env.timer_stop()
        crop = TorchCrop(torch, env, kw["torch_crop"]["size"], kw["torch_crop"]["cells_per_tile"]) if kw.get("torch_crop") else None
        warmup += kw.get("limit", 0)                        # (every agent's first truncation lies in the warm-up, its restart in the timed steps)
        for s in range(warmup):
            RCW.act_(env, actions[s % len(actions)])
            if crop and s < 8:
                crop()
        stream.synchronize()
        env.timer_start()
        image = None
        for s in range(steps):
            RCW.act_(env, actions[(warmup + s) % len(actions)])
            if crop:
                image = crop()
        ms = env.timer_stop()
        stream.synchronize()
        if crop:                                            # the engine's own image of the same state
            env.set_local_map(**kw["torch_crop"])
            differing = int((image != env.local_map.torch(sync=True)).sum().item())
    form = env.step_form()
    try:
        env.sync()
    except IndexError:                                   # (the default radius and increment reach the reference's BoundsError: sticky, harmless here)
        env.clear_error()
    env.close()
    return ms, form, enable_ms, differing


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--maze-batch", type=int, default=1024, help="agents of the five cfg-5 cases")
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
    forms, differing, walls_cache = {}, {}, {}
    for _ in range(args.repeats):
        for n in names:
            ms, forms[n], en, differing[n] = run_case(RCW, torch, np, n, batches[n], args.steps, args.warmup, actions[batches[n]], walls_cache)
            runs[n].append(ms * 1000.0 / args.steps)
            if en is not None:
                enable[n].append(en)
    out = {"metric": "us per step", "device": torch.cuda.get_device_name(0),
           "config": "plain*: cfg-2: 8x8 map, 256 view columns, 256 rows; maze*: cfg-5: 32x32 map, 1024 view columns, a maze per agent, limit 200; "
                     "*_world: RCW_LOCAL_WORLD S 16 r 1; *_seen_local / *_seen_torch: S 32 r 2 of the seen map",
           "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "cases": {}}
    for n in names:
        r = np.array(runs[n])
        out["cases"][n] = {"batch": batches[n], "us_median": float(np.median(r)), "us_min": float(r.min()), "us_max": float(r.max()),
                           "env_steps_per_s_median": float(batches[n] / np.median(r) * 1e6), "step_form": forms[n], "runs_us": [float(x) for x in r]}
        if enable[n]:
            out["cases"][n]["enable_ms"] = {"median": float(np.median(enable[n])), "runs": [float(x) for x in enable[n]]}
        if differing[n] is not None:
            out["cases"][n]["torch_cells_differing"] = differing[n]
    c = out["cases"]
    for base in ("plain", "maze"):
        for on, under in ((f"{base}_world", base), (f"{base}_seen", base), (f"{base}_seen_local", f"{base}_seen"), (f"{base}_seen_torch", f"{base}_seen")):
            if on in c and under in c:
                out[f"{on}_added_us"] = c[on]["us_median"] - c[under]["us_median"]
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
