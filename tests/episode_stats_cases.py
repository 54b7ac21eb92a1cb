"""The wall-bank scenario of the episode statistics' tests — test infrastructure, not a test.  tests/test_episode_stats_spec.py rehearses it
on the CPU (tests/wall_bank_ref.py under tests/time_limit_ref.py, the start distance by tests/goal_distance_ref.py's flood) and
tests/test_gpu_episode_stats.py plays it on an engine; BANK_REHEARSED is what the rehearsal counts, asserted by both.

Three layouts on 5 x 5 — the empty room, a pillar in the middle, a wall across with a door —, weights [1, 0, 3] (layout 1 is never
drawn), a limit of 8 steps, 65 agents, 8 headings, a quarter tile a move, a player radius of 0.3, forward-heavy actions, 40 steps."""
import numpy as np

import episode_stats_ref as ES
import goal_distance_ref as GD
import time_limit_ref as TL
import wall_bank_ref as WB
import walls_ref as WR

BANK = dict(B=65, seed=5, H=5, W=5, N=64, Hc=64, L=8, steps=40, weights=(1, 0, 3), inc=0.25)
BANK_REHEARSED = dict(closes_per_row=(288, 65, 0, 223), successes_truncations_spl=(46, 242, 288))


def bank_layouts():
    w = np.zeros((3, 5, 5), bool)
    w[:, [0, -1], :] = True
    w[:, :, [0, -1]] = True
    w[1, 2, 2] = True                                                          # a pillar in the middle
    w[2, 2, 1:3] = True                                                        # a wall across, its door at the far end
    return w


def bank_actions():
    rng = np.random.default_rng(BANK["seed"] + 1)
    return [WR.draw_actions(rng, BANK["B"]) for _ in range(BANK["steps"])]


class StartDistance:
    """start_distance of rcw_set_goal_distance, from the state behind every call: flooded afresh for an agent whose episode counter moved"""

    def __init__(self, walls, goal, pos, episode):
        self.value = np.array([GD.lookup(GD.bfs_field(walls[b], goal[b]), pos[b]) for b in range(len(goal))], np.int32)
        self.episode = np.array(episode, np.uint32)

    def stepped(self, walls, goal, pos, episode):
        for b in np.flatnonzero(np.asarray(episode) != self.episode):
            self.value[b] = GD.lookup(GD.bfs_field(walls(b), goal[b]), pos[b])
        self.episode = np.array(episode, np.uint32)
        return self.value


def rehearse_bank():
    c = BANK
    ref = WB.WallBankRef(c["B"], c["seed"], c["H"], c["W"], c["N"], c["Hc"], render=False)
    ref.set_wall_bank(bank_layouts(), c["weights"])
    lim = TL.TimeLimitRef(ref, c["L"], c["seed"], True)
    sd = StartDistance([ref.walls_of(b) for b in range(c["B"])], ref.goal, ref.position, ref.episode)
    stats = ES.EpisodeStatsRef(c["B"], 3, 0, c["inc"])
    stats.begin(None, ref.position, ref.episode)
    for a in bank_actions():
        lim.step(a)
        stats.step(ref.position, ref.done, lim.truncated, ref.episode, ref.wall_layout, sd.stepped(ref.walls_of, ref.goal, ref.position, ref.episode))
    return stats, stats.events
