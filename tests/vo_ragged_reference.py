"""CPU composition of a ragged batch (tb_vo_reset_seq_dev / tb_vo_step_ragged_dev, include/tb_capi.h): a schedule over the
single-sequence compositions vo_reference.step, vo_desc_reference.step, vo_proj_reference.step and vo_bow_reference.step.

A slot holds one sequence's state with its own frame index (state['t']); a step advances the active slots only. The
compositions decide "keyframe" from t % P.keyframe_every, so the schedule hands them a Params whose keyframe_every is 1 for a
keyframe and larger than any run for a tracking frame (frame 0 is a keyframe either way): a forced keyframe is the same call as a
cadence keyframe, which is what the device loop does.
"""
import copy

import numpy as np

NEVER = 1 << 30   # a keyframe period no run reaches


class Batch:
    def __init__(self, nseq, P, step, initial_state, args=()):
        """step(state, left, right, P, *args) -> (state, info) and initial_state(Tcw0): one of the four compositions"""
        self.S, self.every = int(nseq), int(P.keyframe_every)
        self.P_kf, self.P_track = copy.copy(P), copy.copy(P)
        self.P_kf.keyframe_every, self.P_track.keyframe_every = 1, NEVER
        self._step, self._init, self.args = step, initial_state, tuple(args)
        self.states = [None] * self.S          # None: never reset
        self.infos = [None] * self.S
        self.kf_frames = [-1] * self.S

    def reset(self, which, Tcw0):
        """which: slot indices; Tcw0: one pose per selected slot. The others keep their state."""
        for s, T in zip(which, Tcw0):
            self.states[s], self.infos[s], self.kf_frames[s] = self._init(T), None, -1

    def frames(self):
        return [-1 if st is None else st["t"] - 1 for st in self.states], list(self.kf_frames)

    def keyframes_due(self, active=None, keyframe=()):
        act = range(self.S) if active is None else active
        return [s for s in act if self.states[s] is not None and (self.states[s]["t"] % self.every == 0 or s in keyframe)]

    def step(self, left, right, active=None, keyframe=()):
        """left / right: per-slot images (right may be None where no keyframe is due; idle slots' entries are not looked at).
        Returns the slots that took a keyframe."""
        act = list(range(self.S) if active is None else active)
        for s in act:
            if self.states[s] is None:
                raise RuntimeError("sequence %d is active and was never reset" % s)
        due = self.keyframes_due(act, keyframe)
        for s in act:
            kf = s in due
            t = self.states[s]["t"]
            self.states[s], self.infos[s] = self._step(self.states[s], left[s], right[s] if kf else None,
                                                       self.P_kf if kf else self.P_track, *self.args)
            assert self.infos[s]["keyframe"] == kf
            if kf:
                self.kf_frames[s] = t
        return due


def same(a, b):
    """two states (or anything they are made of) are equal, arrays bit for bit"""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return type(a) == type(b) and a == b
