"""Batched stereo visual odometry on the device: the reference's test_kitti loop (test/test_vo.cpp:674-850).

`StereoVO` runs S independent stereo sequences in lock-step, one `step()` per frame for all of them:

    frame t: LK-track the last frame's keys into this frame (searchByOPFlow, equalised, RANSAC-rejected) -> carry their map
    points over -> pose optimisation from the last pose -> every keyframe_every-th frame: ORB keys + stereo depths -> new
    map points at the optimised pose

`tracker="bf"` or `"violence"` swaps the tracking line for the reference's descriptor trackers (test_vo.cpp:712-713): ORB on
every frame, searchByBF / searchByViolence against the last keyframe, the keyframe's map points carried through the matches.

All state stays in HBM inside the library's tb_vo object (include/tb_capi.h); after the first step a step makes no host
synchronisation and no host <-> device copy. torch supplies the frames and the stream. There is no CPU fallback.
"""
import ctypes as C

import numpy as np
import torch

from . import capi
from .synth_seq import KITTI_BF, KITTI_K


class _DevArray:
    """__cuda_array_interface__ view of a device pointer owned by the library (only read: copied out at once)."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(int(ptr), False), version=2, strides=None)


# The reference's arguments (test_vo.cpp:712-713; the Matcher's fields after setBowParam(50, 100, 30, true, 6) at :709).
# max_level None = nlevels (Frame::GetMaxLevel() returns nLevels).
TRACKER_DEFAULTS = {
    "bf": dict(ratio=10.0, min_th=30.0, min_level=0, max_level=None),
    "violence": dict(min_level=0, max_level=5, radius=50.0, th_low=50, nratio=6.0, histo_len=30, check_orientation=True),
}


def _tracker(kind, nlevels, params):
    if kind not in TRACKER_DEFAULTS:
        raise ValueError("tracker %r: one of 'opflow', 'bf', 'violence'" % (kind,))
    unknown = set(params) - set(TRACKER_DEFAULTS[kind])
    if unknown:
        raise TypeError("tracker %r takes no parameter %s" % (kind, ", ".join(sorted(unknown))))
    q = dict(TRACKER_DEFAULTS[kind], **params)
    t = capi.VOTracker()
    t.min_level = int(q["min_level"])
    if kind == "bf":
        t.kind = capi.TB_VO_BF
        t.bf_ratio, t.bf_min_th = float(q["ratio"]), float(q["min_th"])
        t.max_level = int(nlevels if q["max_level"] is None else q["max_level"])
    else:
        t.kind = capi.TB_VO_VIOLENCE
        t.max_level, t.radius, t.th_low = int(q["max_level"]), float(q["radius"]), int(q["th_low"])
        t.nratio, t.histo_len, t.check_orientation = float(q["nratio"]), int(q["histo_len"]), int(bool(q["check_orientation"]))
    return t


class StereoVO:
    def __init__(self, nseq, width=1241, height=376, K=KITTI_K, bf=KITTI_BF, nlevels=5, scale=0.8, target=2000, init_th=80.0,
                 min_th=30.0, keyframe_every=10, device=0, tracker="opflow", **tracker_params):
        if tracker == "opflow" and tracker_params:
            raise TypeError("the optical-flow tracker takes no parameters")
        self.dev = torch.device("cuda", device)
        torch.cuda.set_device(self.dev)
        self.S, self.width, self.height = int(nseq), int(width), int(height)
        self.keyframe_every = int(keyframe_every)
        # the context runs on a torch stream of its own (pipeline.py: handle 0 would mean "the context's own stream")
        self.stream = torch.cuda.Stream(device=self.dev)
        self.ctx = capi.Context(device, stream=self.stream.cuda_stream)
        prm = capi.VOParams(self.width, self.height, int(nlevels), float(scale), int(target), float(init_th), float(min_th),
                            (C.c_double * 4)(*[float(k) for k in K]), float(bf), self.keyframe_every)
        self.params, self.tracker = prm, tracker
        if tracker == "opflow":
            self.vo = capi.VO(self.ctx, prm, self.S)
        else:
            try:
                self.vo = capi.VO(self.ctx, prm, self.S, _tracker(tracker, nlevels, tracker_params))
            except Exception:
                self.ctx.close()
                self.ctx = None
                raise
        self._Tcw0 = None
        self.frame = -1

    def close(self):
        if getattr(self, "vo", None) is not None:
            self.vo.close()
            self.vo = None
        if getattr(self, "ctx", None) is not None:
            self.ctx.close()
            self.ctx = None

    def _enter(self, *tensors):
        """Order the loop's stream after the caller's work on `tensors` and keep their memory alive until it has read them."""
        self.stream.wait_stream(torch.cuda.current_stream(self.dev))
        for x in tensors:
            if x is not None:
                x.record_stream(self.stream)

    def reset(self, Tcw0):
        """Tcw0: [S, 4, 4] initial poses (array or tensor); the next step is frame 0."""
        T = torch.as_tensor(np.asarray(Tcw0, np.float32) if not torch.is_tensor(Tcw0) else Tcw0, dtype=torch.float32)
        T = T.reshape(self.S, 16).to(self.dev).contiguous()
        self._enter(T)
        self._Tcw0 = T
        self.vo.reset_dev(T.data_ptr())
        self.frame = -1

    def step_rc(self, left, right=None):
        """One frame; returns the library's status code (0 or a negative TB_E* code)."""
        assert left.dtype == torch.uint8 and left.is_cuda and tuple(left.shape) == (self.S, self.height, self.width)
        left = left.contiguous()
        if right is not None:
            assert right.dtype == torch.uint8 and right.is_cuda and tuple(right.shape) == tuple(left.shape)
            right = right.contiguous()
        self._enter(left, right)
        rc = self.vo.step_dev(left.data_ptr(), right.data_ptr() if right is not None else None, self.width,
                              self.width * self.height)
        if rc == 0:
            self.frame += 1
        return rc

    def step(self, left, right=None):
        """left / right: uint8 device tensors [S, H, W]; right may be None unless this frame is a keyframe."""
        self.ctx.check(self.step_rc(left, right))

    # ---- state accessors: copies (on the loop's stream, ordered before the caller's stream)
    def _get(self, key, shape, typestr, dtype):
        ptr = self.vo.state_dev()[key]
        with torch.cuda.stream(self.stream):
            out = torch.as_tensor(_DevArray(ptr, shape, typestr), device=self.dev).view(dtype).clone()
        torch.cuda.current_stream(self.dev).wait_stream(self.stream)
        return out

    @property
    def key_pitch(self):
        return self.vo.state_dev()["key_pitch"]

    def Tcw(self):
        return self._get("Tcw", (self.S, 4, 4), "<f4", torch.float32)

    def keys(self):
        """(xy [S, P, 2] float32, counts [S] int32)"""
        P = self.key_pitch
        return self._get("keys_xy", (self.S, P, 2), "<f4", torch.float32), self._get("key_counts", (self.S,), "<i4", torch.int32)

    def map_points(self):
        """(xyz [S, P, 3] float32, valid [S, P] uint8): entry j belongs to key j"""
        P = self.key_pitch
        return self._get("map_points", (self.S, P, 3), "<f4", torch.float32), self._get("mp_valid", (self.S, P), "|u1", torch.uint8)

    def obs(self):
        """(rows [S, P, 6] float32 = u, v, X, Y, Z, inv_sigma2; counts [S] int32) of the last step's pose optimisation"""
        P = self.key_pitch
        return self._get("obs", (self.S, P, 6), "<f4", torch.float32), self._get("obs_counts", (self.S,), "<i4", torch.int32)

    def n_inliers(self):
        return self._get("n_inliers", (self.S,), "<i4", torch.int32)

    def outlier(self):
        return self._get("outlier", (self.S, self.key_pitch), "|u1", torch.uint8)

    # ---- descriptor trackers (tracker "bf" / "violence")
    def _tget(self, key, shape, typestr, dtype):
        ptr = self.vo.tracker_state_dev()[key]
        with torch.cuda.stream(self.stream):
            out = torch.as_tensor(_DevArray(ptr, shape, typestr), device=self.dev).view(dtype).clone()
        torch.cuda.current_stream(self.dev).wait_stream(self.stream)
        return out

    def orb(self):
        """The current frame's ORB keys: (records [S, P, 7] -- x, y, size, angle, response as float32 and octave, class_id as
        int32, viewed as int32 -- descriptors [S, P, 32] uint8, counts [S] int32)"""
        P = self.key_pitch
        return (self._tget("orb", (self.S, P, 7), "<i4", torch.int32), self._tget("orb_desc", (self.S, P, 32), "|u1", torch.uint8),
                self._tget("orb_counts", (self.S,), "<i4", torch.int32))

    def matches(self):
        """The step's matches: (rows [S, P, 4] int32 = queryIdx, trainIdx, imgIdx, distance bits; counts [S]; matcher flags [S])"""
        P = self.key_pitch
        return (self._tget("matches", (self.S, P, 4), "<i4", torch.int32), self._tget("match_counts", (self.S,), "<i4", torch.int32),
                self._tget("flags", (self.S,), "<i4", torch.int32))

    def keyframe(self):
        """The keyframe: dict(orb [S, P, 7] int32 records, desc [S, P, 32], counts [S], map_points [S, P, 3], mp_valid [S, P],
        frame = the index of its frame, -1 before any)"""
        P = self.key_pitch
        return dict(orb=self._tget("kf_orb", (self.S, P, 7), "<i4", torch.int32),
                    desc=self._tget("kf_desc", (self.S, P, 32), "|u1", torch.uint8),
                    counts=self._tget("kf_counts", (self.S,), "<i4", torch.int32),
                    map_points=self._tget("kf_map_points", (self.S, P, 3), "<f4", torch.float32),
                    mp_valid=self._tget("kf_mp_valid", (self.S, P), "|u1", torch.uint8),
                    frame=self.vo.tracker_state_dev()["kf_frame"])

    def profile_enable(self, on=True, only=None):
        self.ctx.profile_enable(on, only)

    def profile_report(self):
        return self.ctx.profile_report()

    def synchronize(self):
        self.stream.synchronize()
