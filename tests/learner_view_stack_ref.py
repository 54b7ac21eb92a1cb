"""The learner view's k-frame stack (include/rcw.h "the frame stack") restated in numpy — test infrastructure.

StackModel keeps what the engine keeps: the stack, uint8 (B, k C, h, w) with slot 0 (channels [0, C)) the oldest frame and slot k - 1 the
newest, and each agent's episode counter as of its last push.  The single-frame views it is fed come from learner_view_ref.from_frames
applied to the oracle's frames; the episode counters from the oracle's own.

  refill(view, mask=None, episode=None)  setting the view, reset_, set_state: every touched agent's k slots hold its new frame, the others
                                         keep every byte (the MASK decides; the counter is only recorded, for the next push to compare)
  push(view, episode)                    a step: an agent whose counter differs from the recorded one takes the new frame k times, every
                                         other agent's slot s takes slot s + 1 and slot k - 1 the new frame

brute_force restates the same thing without a state: slot s after step t is the single-frame view of step max(t - (k - 1 - s), the first
step of the agent's current episode)."""
import numpy as np


class StackModel:
    def __init__(self, k, view, episode):
        view = np.asarray(view, dtype=np.uint8)
        assert view.ndim == 4 and 1 <= k <= 16
        self.k, self.C = k, view.shape[1]
        self.stack = np.empty((view.shape[0], k * self.C) + view.shape[2:], np.uint8)
        self.episode = np.zeros(view.shape[0], np.uint32)
        self.refill(view, episode=episode)

    def _slot(self, s):
        return self.stack[:, s * self.C:(s + 1) * self.C]

    def _fill(self, view, who):
        for s in range(self.k):
            self._slot(s)[who] = view[who]

    def refill(self, view, mask=None, episode=None):
        view = np.asarray(view, dtype=np.uint8)
        who = np.ones(len(view), bool) if mask is None else np.asarray(mask) != 0
        self._fill(view, who)
        if episode is not None:
            self.episode[who] = np.asarray(episode, np.uint32)[who]

    def push(self, view, episode):
        view, episode = np.asarray(view, dtype=np.uint8), np.asarray(episode, np.uint32)
        restarted = episode != self.episode
        for s in range(self.k - 1):
            self._slot(s)[...] = self._slot(s + 1)
        self._slot(self.k - 1)[...] = view
        self._fill(view, restarted)
        self.episode[...] = episode
        return restarted


def brute_force(views, first_step, k):
    """views[t]: (B, C, h, w) single-frame views after step t (t = 0: the state the stack was set at); first_step[t][b]: the first step of
    the episode agent b is in after step t.  The stack after the last step."""
    t = len(views) - 1
    B, C = views[0].shape[:2]
    out = np.empty((B, k * C) + views[0].shape[2:], np.uint8)
    for b in range(B):
        for s in range(k):
            u = max(t - (k - 1 - s), int(first_step[t][b]))
            out[b, s * C:(s + 1) * C] = views[u][b]
    return out
