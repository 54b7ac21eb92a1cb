"""Explore, then go — the baseline a partially observing agent can match: every agent follows the frontier's action until its rays have
crossed its goal tile (`goal_seen`), and the guide's shortest-path action from then on; on generated mazes with loops drawn from `levels`
levels, auto_reset, a time limit and episode statistics.  Everything stays on the device: the three arrays are mixed with one
`torch.where` and go back into `act_` with no host wait in the loop.  Beside it the oracle — the guide alone, which knows where the goal is
— on the same mazes: what exploring costs.

    python examples/explore_then_go.py [batch] [steps] [levels]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import raycastworlds_jl_amd as RCW


def run(batch, steps, levels, explore):
    env = RCW.SingleRoomModule.SingleRoom(batch=batch, seed=1, height_tile_map_tu=13, width_tile_map_tu=13, num_directions=16,
                                          position_increment_wu=0.25, player_radius_wu=0.25, num_rays=64, height_camera_view_pu=64,
                                          auto_reset=True, max_episode_steps=1000, wall_generator=dict(loops=0.1, levels=levels),
                                          guide=True, frontier=explore, episode_stats=True)
    with torch.cuda.stream(env.torch_stream()):
        go = env.guide_action.torch(sync=False)
        if explore:
            seen, look = env.goal_seen.torch(sync=False), env.explore_action.torch(sync=False)
        for _ in range(steps):
            RCW.act_(env, torch.where(seen > 0, go, look) if explore else go)
        env.sync()
    tab = env.episode_stats_table()
    left = int((env.frontier_distance.numpy() < 0).sum()) if explore else 0
    env.close()
    return tab, left


def main(batch=1024, steps=1500, levels=8):
    for name, explore in (("explore, then go", True), ("the guide alone", False)):
        tab, left = run(batch, steps, levels, explore)
        t = tab["totals"]
        rate = t["successes"] / t["episodes"] if t["episodes"] else float("nan")
        length = t["sum_length"] / t["episodes"] if t["episodes"] else float("nan")
        print(f"{name}: {batch} agents x {steps} steps: {t['episodes']} episodes, success rate {rate:.3f}, {t['truncations']} truncated, "
              f"mean length {length:.1f}, mean SPL {tab['spl']['totals']:.3f}" + (f", {left} agents with nothing left to explore" if explore else ""))


if __name__ == "__main__":
    main(*[int(a) for a in sys.argv[1:4]])
