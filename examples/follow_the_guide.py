"""The guide as an upper-bound baseline: every agent is fed its own shortest-path action, on generated mazes with loops drawn from `levels`
levels, auto_reset, a time limit and episode statistics — and the statistics' table says how the episodes ended.  Everything stays on the
device: `env.guide_action.torch(sync=False)` goes back into `act_` as it stands, with no host wait in the loop.  A policy is mixed in the
same way: `torch.where(beta_mask, guide, policy_action)` (DAgger's beta), here with `epsilon` of the actions drawn at random.

    python examples/follow_the_guide.py [batch] [steps] [levels] [epsilon percent]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import raycastworlds_jl_amd as RCW


def main(batch=1024, steps=600, levels=8, epsilon=0):
    env = RCW.SingleRoomModule.SingleRoom(batch=batch, seed=1, height_tile_map_tu=13, width_tile_map_tu=13, num_directions=16,
                                          position_increment_wu=0.25, player_radius_wu=0.25, num_rays=64, height_camera_view_pu=64,
                                          auto_reset=True, max_episode_steps=400, wall_generator=dict(loops=0.1, levels=levels),
                                          guide=True, episode_stats=True)
    dev = f"cuda:{env.device}"
    info = env.guide_info
    with torch.cuda.stream(env.torch_stream()):
        guide = env.guide_action.torch(sync=False)
        g = torch.Generator(device=dev).manual_seed(0)
        for _ in range(steps):
            if epsilon:
                explore = torch.randint(0, 100, (batch,), device=dev, generator=g) < epsilon
                action = torch.where(explore, torch.randint(1, 5, (batch,), dtype=torch.uint8, device=dev, generator=g), guide)
            else:
                action = guide
            RCW.act_(env, action)
        env.sync()
    tab = env.episode_stats_table()
    t = tab["totals"]
    rate = t["successes"] / t["episodes"] if t["episodes"] else float("nan")
    print(f"{batch} agents x {steps} steps following the guide (promised: {info['promised']}, epsilon {epsilon} %): {t['episodes']} episodes, "
          f"success rate {rate:.3f}, {t['truncations']} truncated, mean SPL {tab['spl']['totals']:.3f}")
    for k in range(len(tab["levels"]["episodes"])):
        n = int(tab["levels"]["episodes"][k])
        print(f"  level {tab['first'] + k}: {n} episodes, success rate {int(tab['levels']['successes'][k]) / n if n else float('nan'):.3f}, "
              f"mean SPL {float(tab['spl']['levels'][k]):.3f}")
    env.close()


if __name__ == "__main__":
    main(*[int(a) for a in sys.argv[1:5]])
