"""Episode statistics (include/rcw.h, rcw_set_episode_stats) restated in numpy — the specification, test infrastructure, not a test.

EpisodeStatsRef(B, rows, first, inc) keeps the seven per-agent words, the two private ones and the UInt64 table (1 + rows, 8) by the
header's rule, and is FED the state behind every call: position (B, 2) in the world-unit type, done, truncated, the episode counter, and
where the handle has them the layout word and the goal's start_distance.
  begin(mask, pos, episode)   rcw_set_episode_stats(h, 1) (mask None, after zero()), rcw_reset / rcw_set_state / rcw_set_walls
  step(pos, done, truncated, episode, layout=None, start_distance=None)   rcw_step / rcw_step_device
  clear()                     rcw_episode_stats_clear
`events` counts what a run exercised — closes by outcome, closes per row, SPL-defined closes, restarts behind either outcome, frozen and
faulted calls, records a masked call dropped —, so that a test can insist that its trace reaches what it claims.
"""
import numpy as np

OPEN, SUCCESS, TRUNCATED = 0, 1, 2
COLUMNS = ("episodes", "successes", "truncations", "sum_length", "sum_moves", "spl_episodes", "sum_spl_q16")
WORDS = ("finished", "outcome", "length", "moves", "level", "spl_q16", "episodes")


def spl_q16(moves, inc, l):
    """The SPL word of a successful close with SPL defined (l >= 1): every operation in IEEE Float64, in the header's order."""
    p = np.float64(moves) * np.float64(inc)
    return int(np.floor((np.float64(65536.0) * np.float64(l)) / max(p, np.float64(l))))


def bits(pos):
    """(B, 2) positions as bit patterns: +0.0 and -0.0 differ, a NaN equals itself"""
    pos = np.ascontiguousarray(pos)
    return pos.view(np.uint64 if pos.dtype == np.float64 else np.uint32).reshape(-1, 2).copy()


class EpisodeStatsRef:
    def __init__(self, B, rows, first, inc):
        self.B, self.rows, self.first, self.inc = int(B), int(rows), int(first), np.float64(inc)
        self.finished = np.zeros(B, np.uint8)
        self.outcome = np.zeros(B, np.uint8)
        self.length = np.zeros(B, np.uint32)
        self.moves = np.zeros(B, np.uint32)
        self.level = np.full(B, -1, np.int32)
        self.spl_q16 = np.full(B, -1, np.int32)
        self.episodes = np.zeros(B, np.uint32)
        self.last_episode = np.zeros(B, np.uint32)
        self.prev = None
        self.table = np.zeros((1 + self.rows, 8), np.uint64)
        self.events = dict(successes=0, truncations=0, spl_defined=0, restarts_after_success=0, restarts_after_truncation=0,
                           restarts_of_open_records=0, frozen_calls=0, dropped_by_mask=0, closes_outside_the_rows=0,
                           closes_per_row=np.zeros(1 + self.rows, np.int64), length_at_close=[])

    def clear(self):
        self.table[...] = 0

    def _begin(self, who, pos, episode):
        self.length[who] = 0; self.moves[who] = 0; self.outcome[who] = OPEN; self.finished[who] = 0
        self.level[who] = -1; self.spl_q16[who] = -1
        self.prev[who] = pos[who]
        self.last_episode[who] = episode[who]

    def begin(self, mask, pos, episode):
        pos, episode = bits(pos), np.asarray(episode, np.uint32)
        if self.prev is None:
            self.prev = pos.copy()
        who = np.ones(self.B, bool) if mask is None else np.asarray(mask).reshape(self.B) != 0
        self.events["dropped_by_mask"] += int((who & (self.outcome == OPEN) & (self.length > 0)).sum())
        self._begin(who, pos, episode)
        self.finished[...] = 0

    def step(self, pos, done, truncated, episode, layout=None, start_distance=None):
        ev = self.events
        pos, episode = bits(pos), np.asarray(episode, np.uint32)
        done, truncated = np.asarray(done).reshape(self.B) != 0, np.asarray(truncated).reshape(self.B) != 0
        restart = episode != self.last_episode
        frozen = ~restart & (self.outcome != OPEN)
        live = ~restart & ~frozen
        ev["restarts_after_success"] += int((restart & (self.outcome == SUCCESS)).sum())
        ev["restarts_after_truncation"] += int((restart & (self.outcome == TRUNCATED)).sum())
        ev["restarts_of_open_records"] += int((restart & (self.outcome == OPEN)).sum())
        ev["frozen_calls"] += int(frozen.sum())
        self._begin(restart, pos, episode)
        self.finished[frozen] = 0
        self.prev[frozen] = pos[frozen]
        self.length[live] += 1
        self.moves[live & (pos != self.prev).any(axis=1)] += 1
        self.prev[live] = pos[live]
        closing = live & (done | truncated)
        self.finished[live] = closing[live]
        for a in np.flatnonzero(closing):
            ok = bool(done[a])
            self.outcome[a] = SUCCESS if ok else TRUNCATED
            self.level[a] = -1 if layout is None else int(layout[a])
            self.episodes[a] += 1
            l = -1 if start_distance is None else int(start_distance[a])
            self.spl_q16[a] = -1 if l < 1 else (spl_q16(int(self.moves[a]), self.inc, l) if ok else 0)
            k = int(self.level[a]) - self.first
            targets = [0] + ([1 + k] if 0 <= k < self.rows else [])
            for r in targets:
                row = self.table[r]
                row[0] += 1; row[1 if ok else 2] += 1; row[3] += self.length[a]; row[4] += self.moves[a]
                if self.spl_q16[a] >= 0:
                    row[5] += 1; row[6] += np.uint64(self.spl_q16[a])
                ev["closes_per_row"][r] += 1
            ev["successes" if ok else "truncations"] += 1
            ev["spl_defined"] += int(self.spl_q16[a] >= 0)
            ev["closes_outside_the_rows"] += int(len(targets) == 1)
            ev["length_at_close"].append((int(a), int(self.length[a])))
        return closing

    def words(self):
        return {w: getattr(self, w) for w in WORDS}


def assert_equal(env, ref, where=""):
    """the engine's seven words and its whole table against the reference"""
    for name in WORDS:
        got = np.asarray(getattr(env.episode_stats, name))
        want = getattr(ref, name)
        assert got.dtype == want.dtype, (name, got.dtype)
        np.testing.assert_array_equal(got, want, err_msg=f"{name} {where}")
    got = np.asarray(env.episode_stats_table(device=True))
    assert got.dtype == np.uint64 and got.shape == ref.table.shape, (got.shape, ref.table.shape)
    np.testing.assert_array_equal(got, ref.table, err_msg=f"the table {where}")
