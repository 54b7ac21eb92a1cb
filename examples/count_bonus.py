"""A count-based exploration bonus with no host in the loop: a random policy on a wall bank of three layouts under a time limit, the visit
map on with its table.  Every step the episodic bonus `beta / sqrt(N_ep)` of each agent's cell is taken from `env.visits_here` on the
device and summed; at the end the batch's mean bonus a step, the share of steps that entered a cell for the first time in the episode
(`env.visit_first`, NovelD's gate), and per level of the bank the coverage — the free tiles some agent has stood on — from `visit_table()`.

    python examples/count_bonus.py [batch] [steps]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import raycastworlds_jl_amd as RCW


def main(batch=1024, steps=400, beta=0.1):
    H = W = 9
    bank = [RCW.layouts.ring(H, W), RCW.layouts.four_rooms(H, W), RCW.layouts.maze(H, W, np.random.default_rng(3))]
    env = RCW.SingleRoomModule.SingleRoom(batch=batch, seed=1, height_tile_map_tu=H, width_tile_map_tu=W, num_directions=16,
                                          position_increment_wu=0.25, player_radius_wu=0.25, num_rays=64, height_camera_view_pu=64,
                                          auto_reset=True, max_episode_steps=100, out_of_bounds=1, wall_bank=bank, visit_map=dict(sectors=1, table=True))
    with torch.cuda.stream(env.torch_stream()):
        here, first = env.visits_here.torch(sync=False), env.visit_first.torch(sync=False)
        bonus = torch.zeros((), device=here.device, dtype=torch.float64)
        firsts = torch.zeros((), device=here.device, dtype=torch.int64)
        generator = torch.Generator(device=here.device).manual_seed(0)
        for _ in range(steps):
            RCW.act_(env, torch.randint(1, 5, (batch,), device=here.device, dtype=torch.uint8, generator=generator))
            bonus += (beta * torch.rsqrt(here.float().clamp(min=1))).sum()
            firsts += (first > 0).sum()
        env.sync()
    table = env.visit_table()
    print(f"{batch} agents x {steps} random steps: mean episodic bonus {bonus.item() / (batch * steps):.4f} a step (beta {beta}), "
          f"{firsts.item() / (batch * steps):.3f} of the steps entered a new cell")
    for k, level in enumerate(table["levels"]):
        free = int((~(bank[k] != 0)).sum())
        print(f"level {table['first'] + k}: {int(level.sum())} visits, {int((level.sum(axis=0) > 0).sum())} of {free} free tiles covered")
    env.close()


if __name__ == "__main__":
    main(*[int(a) for a in sys.argv[1:3]])
