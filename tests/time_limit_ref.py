"""The episode time limit (include/rcw.h, rcw_set_time_limit) composed from the UNCHANGED oracle — test infrastructure.

TimeLimitRef holds an oracle.OracleBatch and keeps the two words the limit adds, episode_steps and truncated, in numpy.  A step, for
each agent in the header's order:
  1  an action outside 1..4         the agent is not stepped (the oracle's step_lenient skips it); the two words stay
  2  done OR truncated, auto_reset  a restart.  The oracle restarts its done agents itself; the truncated ones are reset here in front
                                    of the step — oracle.reset(mask, seed = the handle's), whose draws are keyed (seed, agent, episode)
                                    and therefore the ones the device's restart makes — and given action 0, so that step_lenient leaves
                                    them alone.  Both words become zero.
  3  otherwise                      the oracle's act!.  An agent whose status word the step set to "out of bounds" raised and keeps the
                                    two words; every other one counts — blocked or not, goal or not — and
                                    truncated = (episode_steps >= L and not done).
With L = 0 the helper is step_lenient and two arrays of zeros.  The status words step_lenient leaves on the agents of rule 2 (their action
0 is "invalid" to the oracle) are the helper's business: it takes them back, so that `orc.status` stays the sticky word the engine keeps
(rcw_status) and a test of RCW_OOB_ERROR can compare the two.  `events` counts what a rollout exercised, so that a test can insist that
its scenario reaches the restart and the coincidence step; raised_with_words_kept: agents whose step raised while episode_steps > 0.

The oracle may be oracle.OracleBatch or anything with its B, done, status, reset(mask, seed), step_lenient and clear_status
(tests/walls_ref.py's WallsRef: the limit on a walled map)."""
import numpy as np

RCW_ERR_OUT_OF_BOUNDS = -5


class TimeLimitRef:
    def __init__(self, orc, limit, seed, auto_reset):
        self.orc, self.seed, self.auto_reset = orc, int(seed), bool(auto_reset)
        self.events = dict(truncations=0, terminations=0, on_the_limit_step=0, restarts_after_truncation=0, restarts_after_done=0,
                           invalid_while_truncated=0, raised_with_words_kept=0)
        self.set_time_limit(limit)

    def set_time_limit(self, limit):
        assert limit >= 0
        self.limit = int(limit)
        self.episode_steps = np.zeros(self.orc.B, np.uint32)
        self.truncated = np.zeros(self.orc.B, np.uint8)

    def clear(self, mask=None):
        """reset_ / set_state: the masked agents' two words (the oracle's own call is the caller's)."""
        who = np.ones(self.orc.B, bool) if mask is None else np.asarray(mask) != 0
        self.episode_steps[who] = 0
        self.truncated[who] = 0

    def step(self, actions):
        orc, ev = self.orc, self.events
        a = np.ascontiguousarray(actions, dtype=np.uint8).reshape(orc.B)
        if self.limit == 0:
            orc.step_lenient(a)
            return
        valid = (a >= 1) & (a <= 4)
        done0 = orc.done.astype(bool).copy()
        trunc0 = self.truncated != 0
        re_t = valid & trunc0 & ~done0 & self.auto_reset
        re_d = valid & done0 & self.auto_reset
        ev["invalid_while_truncated"] += int((~valid & trunc0).sum())
        if re_t.any():
            orc.reset(mask=re_t.astype(np.uint8), seed=self.seed)
        status0 = orc.status.copy()
        orc.clear_status()
        sent = a.copy()
        sent[re_t] = 0
        orc.step_lenient(sent)
        orc.status[re_t] = 0                                                   # (the helper's action 0, not the caller's: nothing was invalid)
        raised = orc.status == RCW_ERR_OUT_OF_BOUNDS                           # (act! raised: "the agent is left exactly as it was")
        orc.status[...] = np.where(orc.status != 0, orc.status, status0)       # (sticky, as the oracle keeps it)
        stepped = valid & ~re_t & ~re_d & ~raised
        self.episode_steps[re_t | re_d] = 0
        self.truncated[re_t | re_d] = 0
        self.episode_steps[stepped] += 1
        done = orc.done.astype(bool)
        reached = stepped & (self.episode_steps >= self.limit)
        self.truncated[stepped] = (reached & ~done)[stepped]
        ev["on_the_limit_step"] += int((reached & done & (self.episode_steps == self.limit)).sum())
        ev["truncations"] += int((stepped & (self.truncated != 0)).sum())
        ev["terminations"] += int((stepped & done).sum())
        ev["restarts_after_truncation"] += int(re_t.sum())
        ev["restarts_after_done"] += int(re_d.sum())
        ev["raised_with_words_kept"] += int((valid & ~re_t & ~re_d & raised & (self.episode_steps > 0)).sum())


def draw_actions(rng, batch, step, bad_every=0):
    """The scenario's actions: forward-heavy draws from [1, 1, 1, 2, 3, 4]; with bad_every, on the steps with step % bad_every == 1 an
    eighth of the agents get one value outside 1..4."""
    a = rng.choice(np.array([1, 1, 1, 2, 3, 4], np.uint8), batch)
    if bad_every and step % bad_every == 1:
        a[rng.integers(0, batch, max(1, batch // 8))] = rng.choice(np.array([0, 5, 255], np.uint8))
    return a
