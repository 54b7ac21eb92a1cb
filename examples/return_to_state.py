"""Return-then-explore with the state archive: every `every` steps the agent that has seen the most of its maze is archived, and an agent
whose episode the time limit cuts goes on from that state instead of from a fresh start.  Everything stays on the device: the best agent is
an argmax over `env.seen_count`, the save takes a one-hot mask, the restore takes `truncated` itself as its mask — no host wait in the loop.

    python examples/return_to_state.py [batch] [steps] [every]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import raycastworlds_jl_amd as RCW


def main(batch=256, steps=200, every=10):
    env = RCW.SingleRoomModule.SingleRoom(batch=batch, seed=1, height_tile_map_tu=17, width_tile_map_tu=17, num_rays=128, height_camera_view_pu=64,
                                          auto_reset=True, max_episode_steps=40, wall_generator={}, seen_map=True, snapshots=1)
    dev = f"cuda:{env.device}"
    with torch.cuda.stream(env.torch_stream()):
        seen = env.seen_count.torch(sync=False)
        truncated = env.truncated_device().torch(sync=False)
        row0 = torch.zeros(batch, dtype=torch.int32, device=dev)               # every agent's row: the archive's only one
        best_seen = torch.zeros((), dtype=torch.int32, device=dev)
        returns = torch.zeros((), dtype=torch.int64, device=dev)
        g = torch.Generator(device=dev).manual_seed(0)
        for t in range(steps):
            if t % every == 0:                                                 # archive the agent that has seen the most, if it beats the archive
                top = seen.max()
                better = (seen == top) & (top > best_seen)
                one = torch.zeros(batch, dtype=torch.uint8, device=dev)
                one[better.to(torch.uint8).argmax()] = better.any().to(torch.uint8)
                env.snapshot_save(row0, one)
                best_seen = torch.maximum(best_seen, top)
            RCW.act_(env, torch.randint(1, 5, (batch,), dtype=torch.uint8, device=dev, generator=g))
            cut = truncated.clone()
            returns += cut.sum()
            env.snapshot_restore(row0, cut)                                    # the cut agents go on from the archived state
        env.sync()
        print(f"{batch} agents x {steps} steps: the archived agent had seen {int(best_seen)} tiles, {int(returns)} returns to it, "
              f"the batch now sees {float(seen.float().mean()):.1f} tiles on average")
    env.close()


if __name__ == "__main__":
    main(*[int(a) for a in sys.argv[1:4]])
