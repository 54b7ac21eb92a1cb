"""What the goal distance (rcw_set_goal_distance) costs a step, timed like tools/walls_bench.py: device-resident U{1..4} actions, HIP events
on the engine's stream around `--steps` steps after `--warmup`.  Each case runs `--repeats` times, interleaved; the JSON carries every run,
the median and the range, and the ratios of the medians.

    python tools/goal_distance_bench.py --steps 200 --warmup 20 --repeats 5 [--out profiles/goal_distance_bench.json]

Cases, all under auto_reset:
  at BASELINE cfg-2 (8x8 map, 256 view columns, 4096 agents)
    plain              no walls, the feature off
    four_rooms         layouts.four_rooms, the feature off
    four_rooms_gd      ... with the feature on: one more launch a step, almost every agent on the lookup path
  at cfg-5's geometry (32x32 map, 1024 view columns, --maze-batch agents), a maze per agent, time limit 200 — restarts, and with them
  floods, happen inside the timed steps: these cases warm up for the limit plus `--warmup` steps, so with the default 200 timed steps
  every agent restarts once in them (about one flood per agent per 200 steps, the steady-state rate, though most of them in one step)
    maze               the feature off
    maze_gd            the feature on
    maze_torch_bfs     the feature off and the caller's alternative behind every step: for the agents whose episode counter moved, a batched
                       relaxation of the (B, H, W) field in torch (goal 0, walls 0xFFFF, field = min(field, neighbours + 1) until nothing
                       changes, checked every 16 sweeps), then the lookup at the player's tile and the three words
`enable_ms`: rcw_set_goal_distance(h, 1) alone at both shapes — every agent flooding at once — between two events, median of the repeats."""
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
    "four_rooms": dict(cfg=CFG2, walls="four_rooms"),
    "four_rooms_gd": dict(cfg=CFG2, walls="four_rooms", gd=True),
    "maze": dict(cfg=CFG5, big=True, walls="maze", limit=200),
    "maze_gd": dict(cfg=CFG5, big=True, walls="maze", limit=200, gd=True),
    "maze_torch_bfs": dict(cfg=CFG5, big=True, walls="maze", limit=200, torch_bfs=True),
}
BIG = 0xFFFF


def make_walls(RCW, np, kind, H, W, batch):
    if kind == "four_rooms":
        return RCW.layouts.four_rooms(H, W)
    return np.stack([RCW.layouts.maze(H, W, np.random.default_rng(1000 + a)) for a in range(batch)])


class TorchGoalDistance:
    """The caller's alternative, on the engine's stream: the field kept as int32 (B, H, W) in torch, the state from the library's getters."""

    def __init__(self, env, torch, walls):
        import numpy as np

        self.torch, B = torch, env.batch
        H, W = env.cfg.height_tile_map_tu, env.cfg.width_tile_map_tu
        w = np.broadcast_to(np.asarray(walls), (B, H, W)) if np.asarray(walls).ndim == 2 else np.asarray(walls)
        self.walls = torch.from_numpy(np.ascontiguousarray(w)).cuda()
        self.H, self.W, self.env = H, W, env
        self.field = torch.full((B, H, W), BIG, dtype=torch.int32, device="cuda")
        self.recorded = torch.full((B,), -1, dtype=torch.int64, device="cuda")
        self.distance = torch.zeros(B, dtype=torch.int32, device="cuda")
        self.start = torch.zeros(B, dtype=torch.int32, device="cuda")
        self.progress = torch.zeros(B, dtype=torch.int32, device="cuda")

    def flood(self, who, goal):
        torch = self.torch
        walls = self.walls[who]
        f = torch.full(walls.shape, BIG, dtype=torch.int32, device="cuda")
        k = torch.arange(len(who), device="cuda")
        gi, gj = goal[who, 0].long() - 1, goal[who, 1].long() - 1
        f[k, gi, gj] = torch.where(walls[k, gi, gj], BIG, 0).to(torch.int32)
        while True:
            before = f.clone()
            for _ in range(16):
                n = f.clone()
                n[:, 1:, :] = torch.minimum(n[:, 1:, :], f[:, :-1, :] + 1)
                n[:, :-1, :] = torch.minimum(n[:, :-1, :], f[:, 1:, :] + 1)
                n[:, :, 1:] = torch.minimum(n[:, :, 1:], f[:, :, :-1] + 1)
                n[:, :, :-1] = torch.minimum(n[:, :, :-1], f[:, :, 1:] + 1)
                f = torch.where(walls, BIG, torch.clamp(n, max=BIG))
            if torch.equal(f, before):
                return f

    def update(self, goal, pos, episode):
        torch = self.torch
        moved = episode.long() != self.recorded
        who = torch.nonzero(moved).flatten()                               # (a host synchronisation: the caller has to know how many)
        if len(who):
            self.field[who] = self.flood(who, goal)
            self.recorded[who] = episode[who].long()
        i, j = torch.floor(pos[:, 0]).long(), torch.floor(pos[:, 1]).long()
        inb = (i >= 0) & (i < self.H) & (j >= 0) & (j < self.W)
        v = self.field[torch.arange(len(i), device="cuda"), i.clamp(0, self.H - 1), j.clamp(0, self.W - 1)]
        new = torch.where(inb & (v != BIG), v, -1).to(torch.int32)
        both = (self.distance >= 0) & (new >= 0) & ~moved
        self.progress = torch.where(both, self.distance - new, 0).to(torch.int32)
        self.distance = new
        self.start = torch.where(moved, new, self.start)


def state_tensors(env, torch, np):
    """goal (B, 2) int32, position (B, 2) float32 and the episode counter (B,): the library hands these out as host copies only (there is no
    device pointer for them), so the alternative reads the getters and uploads — what a caller has to do today"""
    w = env.world
    return (torch.from_numpy(w.goal_position).cuda(), torch.from_numpy(np.ascontiguousarray(w.player_position_wu)).cuda(),
            torch.from_numpy(w.episode.astype(np.int64)).cuda())


def run_case(RCW, torch, np, name, batch, steps, warmup, actions, walls_cache):
    kw = CASES[name]
    env = RCW.SingleRoomModule.SingleRoom(batch=batch, seed=0, auto_reset=True, **kw["cfg"])
    walls = None
    if "walls" in kw:
        key = (kw["walls"], batch)
        if key not in walls_cache:
            walls_cache[key] = make_walls(RCW, np, kw["walls"], kw["cfg"]["height_tile_map_tu"], kw["cfg"]["width_tile_map_tu"], batch)
        walls = walls_cache[key]
        env.set_walls(walls)
    if kw.get("limit"):
        env.set_time_limit(kw["limit"])
    stream = torch.cuda.Stream()
    env.set_stream(stream.cuda_stream)
    enable_ms = None
    with torch.cuda.stream(stream):
        if kw.get("gd"):
            stream.synchronize()
            env.timer_start()
            env.set_goal_distance(True)
            enable_ms = env.timer_stop()
        alt = TorchGoalDistance(env, torch, walls) if kw.get("torch_bfs") else None

        def step(s):
            RCW.act_(env, actions[s % len(actions)])
            if alt is not None:
                alt.update(*state_tensors(env, torch, np))

        warmup += kw.get("limit", 0)                        # (every agent's first truncation lies in the warm-up, its restart — and flood — in the timed steps)
        for s in range(warmup):
            step(s)
        stream.synchronize()
        env.timer_start()
        for s in range(steps):
            step(warmup + s)
        ms = env.timer_stop()
        stream.synchronize()
    form = env.step_form()
    episodes = float(env.world.episode.mean())
    try:
        env.sync()
    except IndexError:                                   # (the default radius and increment reach the reference's BoundsError: sticky, harmless here)
        env.clear_error()
    env.close()
    return ms, form, episodes, enable_ms


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
    forms, episodes, walls_cache = {}, {}, {}
    for _ in range(args.repeats):
        for n in names:
            ms, forms[n], episodes[n], en = run_case(RCW, torch, np, n, batches[n], args.steps, args.warmup, actions[batches[n]], walls_cache)
            runs[n].append(batches[n] * args.steps / (ms / 1000.0))
            if en is not None:
                enable[n].append(en)
    out = {"metric": "env-steps/s", "config": "cfg-2: 8x8 map, 256 view columns, 256 rows; maze*: cfg-5: 32x32 map, 1024 view columns, limit 200",
           "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "cases": {}}
    for n in names:
        r = np.array(runs[n])
        out["cases"][n] = {"batch": batches[n], "median": float(np.median(r)), "min": float(r.min()), "max": float(r.max()),
                           "us_per_step_median": float(batches[n] / np.median(r) * 1e6), "step_form": forms[n],
                           "mean_episode_counter_at_the_end": episodes[n], "runs": [float(x) for x in r]}
        if enable[n]:
            out["cases"][n]["enable_ms"] = {"median": float(np.median(enable[n])), "runs": [float(x) for x in enable[n]]}
    c = out["cases"]
    for on, off in (("four_rooms_gd", "four_rooms"), ("maze_gd", "maze")):
        if on in c and off in c:
            out[f"{on}_over_{off}"] = c[on]["median"] / c[off]["median"]
            out[f"{on}_added_us_per_step"] = c[on]["us_per_step_median"] - c[off]["us_per_step_median"]
    if "maze_gd" in c and "maze_torch_bfs" in c:
        out["maze_gd_over_maze_torch_bfs"] = c["maze_gd"]["median"] / c["maze_torch_bfs"]["median"]
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
