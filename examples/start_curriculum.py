"""A start-distance curriculum with no host in the loop: the band of the start rule is widened from (1, 2) outwards, phase by phase, while
every agent follows the guide on generated mazes with loops, auto_reset and a time limit.  `set_start_distance` on a handle that has the
rule only changes a kernel argument — no allocation, no wait —, so the loop queues it between steps like any other call.  Per phase the
script prints the mean of `goal_start_distance` over the agents whose episode began in the phase: it follows the band.

    python examples/start_curriculum.py [batch] [steps per phase] [phases]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import raycastworlds_jl_amd as RCW


def main(batch=1024, steps=120, phases=5):
    env = RCW.SingleRoomModule.SingleRoom(batch=batch, seed=1, height_tile_map_tu=13, width_tile_map_tu=13, num_directions=16,
                                          position_increment_wu=0.25, player_radius_wu=0.25, num_rays=64, height_camera_view_pu=64,
                                          auto_reset=True, max_episode_steps=200, wall_generator=dict(loops=0.1),
                                          guide=True, start_distance=(1, 2))
    means = []
    with torch.cuda.stream(env.torch_stream()):
        guide = env.guide_action.torch(sync=False)
        start = env.goal_start_distance.torch(sync=False)
        placed = env.start_placed.torch(sync=False)
        for phase in range(phases):
            lo, hi = 1 + 4 * phase, 2 + 4 * phase
            env.set_start_distance(lo, hi)
            RCW.reset_(env)                                                   # every agent starts the phase inside its band
            total = torch.zeros((), device=start.device)
            for _ in range(steps):
                RCW.act_(env, guide)
                total += start.float().mean()
            means.append((lo, hi, total / steps, (placed == 2).float().mean()))
        env.sync()
    for lo, hi, mean, clamped in means:
        print(f"band ({lo}, {hi}): mean start_distance {float(mean):.2f}, {100 * float(clamped):.1f} % of the agents clamped to their farthest tile")
    env.close()
    return [float(m) for _, _, m, _ in means]


if __name__ == "__main__":
    main(*[int(a) for a in sys.argv[1:4]])
