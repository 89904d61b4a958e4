"""Batched stereo visual odometry on the device: the reference's test_kitti loop (test/test_vo.cpp:674-850).

`StereoVO` runs S independent stereo sequences in lock-step, one `step()` per frame for all of them:

    frame t: LK-track the last frame's keys into this frame (searchByOPFlow, equalised, RANSAC-rejected) -> carry their map
    points over -> pose optimisation from the last pose -> every keyframe_every-th frame: ORB keys + stereo depths -> new
    map points at the optimised pose

`tracker="bf"` or `"violence"` swaps the tracking line for the reference's descriptor trackers (test_vo.cpp:712-713): ORB on
every frame, searchByBF / searchByViolence against the last keyframe, the keyframe's map points carried through the matches.

`tracker="lsh"` runs the line test_vo_1 itself runs (test_vo.cpp:213), searchByNN: the LSH nearest neighbour of
FlannBasedMatcher(LshIndexParams(20, 10, 2)) with searchByBF's filter, restated in include/tb_capi.h; `seed=` or `bits=` fix the
descriptor bits that form the hash keys (the reference leaves them to rand()).

`tracker="projection"` or `"projection_map"` runs the reference's projection loop (test/test_projection.cpp:512-517):
searchByProjection of the keyframe's map points, or of a device-resident map the keyframes add their points to, into the
current frame's lookup grid. The map holds the points of the last `map_keyframes` keyframes.

`tracker="bow", vocab=...` runs the fourth tracking line, searchByBow (test_vo.cpp:711) against the keyframe, with Frame::SetBow
(:705) on the device for every frame: the DBoW2 transform, the FeatureVector keys and the BowVector. `vocab` is a
synth.Vocabulary (uploaded and owned by the loop), a callable `f(context) -> handle` (e.g. one that trains with
`context.vocab_train_dev`; the loop owns the handle), or a handle made on the `context=` the loop was given (borrowed).
`keyframe_db=N` keeps the BowVectors of the last N keyframes of every sequence in a device-resident database that
`query_keyframes` scores the current frame against (TemplatedVocabulary::score), for loop and relocalisation candidates.
`relocalize=M` (with keyframe_db=N) also keeps those keyframes themselves -- keys, descriptors, FeatureVector, map points, pose --
in a device-resident store, and `relocalize()` verifies the best M candidates on the device: searchByBow against each stored
keyframe, PoseOptimization seeded with its pose, the candidate with the most inliers. It is a query: the loop's state stays.
`pnp=True` (or a dict, see PNP_DEFAULTS; with relocalize=M, not with recover= or loop_close=) puts a P3P-RANSAC in front of that
pose stage, so that a candidate seen from metres away or through a mostly wrong match list is still verified: the consensus rows
and the PnP pose go on to PoseOptimization, and `relocalize()` returns the PnP fields as well.
`recover=True` (or a dict, see RECOVER_DEFAULTS; with relocalize=M) makes the loop use it: a sequence whose tracking step keeps
fewer than lost_inliers inliers is relocalised inside the step, adopts the winner's pose, matches and map points, and tracks
against the winning keyframe from then on. Which sequences do is decided on the device; the others are untouched.
`loop_close=True` (or a dict, see LOOP_DEFAULTS; with relocalize=M, keyframe_db <= 63, lock-step, not with recover=) corrects the
trajectory on a revisit: at a keyframe step whose best verified candidate reaches min_inliers, a pose graph of the stored
keyframes and the current frame is optimised on the device (tb_pose_graph_batch_dev), the stored keyframes take their corrected
poses, their map points move rigidly with them, and the frame spawns and is stored at the corrected pose. `loop()` shows it.

The batch need not move in lock-step: `reset(Tcw0, which=)` restarts some sequences in their slots, `step(..., active=, keyframe=)`
advances only the active ones and gives the flagged ones a keyframe off the cadence, `frames()` tells where each one is. A sequence
of such a ragged batch computes what it computes alone (every tracker but "projection_map", and "bow" without keyframe_db=).

`window_ba=True` (or a dict, see WINDOW_BA_DEFAULTS; optical-flow tracker, lock-step only) refines every keyframe segment: the
frames from one keyframe to the next are a local-BA window over the first keyframe's stereo points (key i is the same point in
all of them), and the next keyframe spawns its points at the refined pose. `window()` shows the segment log, the window and the
refined segment. The BA's termination test is the one host synchronisation a keyframe step gains; tracking steps gain none.

`mono=True` (or a dict, see MONO_DEFAULTS; optical-flow tracker, lock-step only, not with window_ba=) grows the map from one
camera: frame 0 is the stereo keyframe that fixes the scale, and every later keyframe takes `right=None`, triangulates the keys
LK has held since the last keyframe from the two known poses (LocalBA::LinearTriangle on the device, gated on depth, parallax
and reprojection error) and merges the keys that have a map point with the frame's ORB keys. `init=True` (or a dict, see
INIT_DEFAULTS; with mono=) starts such a loop without any right image: frame 0 runs ORB only, and the first keyframe whose LK
tracks give the two-view operator (tb_two_view_batch_dev) a pose and at least 50 points initialises the sequence, at the scale
`baseline=` sets; `mono_init()` shows which sequences are initialised and their last attempt. `mono()` shows the keyframe's key
list, the triangulation's flags and the merge's counts.

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
    # test_projection.cpp:512-513 setProjectionParam(30, 50, 30, true, 30); searchByProjection(cur, key_frame)
    "projection": dict(nratio=30.0, th_high=50, histo_len=30, check_orientation=True),
    # :516-517 setProjectionParam(30, 50, 30, true, 20); searchByProjection(map, cur, 0.6); map_keyframes: include/tb_capi.h
    "projection_map": dict(nratio=20.0, radio=0.6, th_high=50, histo_len=30, check_orientation=True, map_keyframes=4),
    # :706 setBowParam(50, 100, 30, true, 6); :711 searchByBow(cur, key_frame, true); Frame.cpp:269 levelsup 4
    "bow": dict(levelsup=4, map_point_only=True, th_low=50, nratio=6.0, histo_len=30, check_orientation=True),
    # test_vo_1 :213 searchByNN(cur, key_frame, 0, 5, 10, 30); matcher.cpp:18 LshIndexParams(20, 10, 2); seed / bits: the bit table
    "lsh": dict(ratio=10.0, min_th=30.0, min_level=0, max_level=None, tables=20, key_size=10, multi_probe_level=2, seed=0, bits=None),
}
# recover=True. ORB-SLAM-style figures, NOT the reference's (it has no relocalisation): tracking counts as lost below 30 inliers
# (ORB-SLAM's local-map tracking asks for 30), a candidate is accepted from 50 inliers on (its relocalisation's figure), the best
# 4 candidates are verified and the keyframe being tracked against is left out of them.
RECOVER_DEFAULTS = dict(lost_inliers=30, topk=4, exclude_newest=1, min_inliers=50)
# loop_close=True. The weights 1 and 1 are the identity information ORB-SLAM's essential graph uses; the reference has no figure
LOOP_DEFAULTS = dict(topk=4, exclude_newest=1, min_inliers=50, iters=10, w_rot=1.0, w_trans=1.0)
# test_vo_1's searchByBow arguments (:207 setBowParam(30, ..., 5), :212 MapPointOnly false)
# window_ba=True: 10 LM iterations, the keyframe held fixed (a second fixed frame is a noisy single-frame estimate and measured
# worse), a point needs 2 inlier observations, a window needs 3 points for its pose to be adopted
WINDOW_BA_DEFAULTS = dict(iters=10, fixed=1, min_obs=2, min_points=3)
# mono=True: ORB-SLAM's triangulation gates (a ray cosine below 0.9998, the 95 % chi-square bound of 2 degrees of freedom) and
# an 8-pixel occupancy cell for the keyframe's merge
MONO_DEFAULTS = dict(cos_parallax_max=0.9998, chi2_max=5.991, cell=8)
# init=True (with mono=): the two-view operator's defaults (capi.two_view_params; baseline sets the scale) and the least number of
# keys LK must still hold at the keyframe
INIT_DEFAULTS = dict(hypotheses=256, chi2_epi=3.841, refit=1, cos_parallax_max=0.9998, chi2_max=5.991, min_good_ratio=0.9,
                     ambiguity_ratio=0.7, min_points=50, baseline=1.0, seed=0, min_tracks=100)
BOW_TEST_VO_1 = dict(th_low=30, nratio=5.0, map_point_only=False)


def _tracker(kind, nlevels, params):
    if kind not in TRACKER_DEFAULTS:
        raise ValueError("tracker %r: one of 'opflow', 'bf', 'violence', 'projection', 'projection_map', 'bow', 'lsh'" % (kind,))
    unknown = set(params) - set(TRACKER_DEFAULTS[kind])
    if unknown:
        raise TypeError("tracker %r takes no parameter %s" % (kind, ", ".join(sorted(unknown))))
    q = dict(TRACKER_DEFAULTS[kind], **params)
    if kind == "bow":
        return capi.VOBow(int(q["levelsup"]), int(bool(q["map_point_only"])), int(q["th_low"]), float(q["nratio"]), int(q["histo_len"]),
                          int(bool(q["check_orientation"])))
    if kind == "lsh":
        t = capi.VOLsh(float(q["ratio"]), float(q["min_th"]), int(q["min_level"]), int(nlevels if q["max_level"] is None else q["max_level"]),
                       int(q["tables"]), int(q["key_size"]), int(q["multi_probe_level"]), int(q["seed"]) & (2 ** 64 - 1), None)
        t._bits = capi._lsh_bits(q["bits"], t.tables, t.key_size)   # kept alive with the struct; read during the create call
        t.bits = t._bits.ctypes.data if t._bits is not None else None
        return t
    t = capi.VOTracker()
    if kind in ("projection", "projection_map"):
        t.kind = capi.TB_VO_PROJECTION if kind == "projection" else capi.TB_VO_PROJECTION_MAP
        t.nratio, t.th_high, t.histo_len = float(q["nratio"]), int(q["th_high"]), int(q["histo_len"])
        t.check_orientation = int(bool(q["check_orientation"]))
        if kind == "projection_map":
            t.radio, t.map_keyframes = float(q["radio"]), int(q["map_keyframes"])
        return t
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


# pnp=True. 256 hypotheses and chi2Mono are this library's defaults, 10 is ORB-SLAM's minInliers for its PnP solver
PNP_DEFAULTS = dict(hypotheses=256, chi2_max=5.991, seed=0, min_consensus=10, expand=1)


class StereoVO:
    def __init__(self, nseq, width=1241, height=376, K=KITTI_K, bf=KITTI_BF, nlevels=5, scale=0.8, target=2000, init_th=80.0,
                 min_th=30.0, keyframe_every=10, device=0, tracker="opflow", vocab=None, context=None, keyframe_db=0, relocalize=0, recover=None, window_ba=None, mono=None, loop_close=None, pnp=None, init=None, **tracker_params):
        if tracker == "opflow" and tracker_params:
            raise TypeError("the optical-flow tracker takes no parameters")
        if mono:
            unknown = set(mono) - set(MONO_DEFAULTS) if isinstance(mono, dict) else ()
            if unknown:
                raise TypeError("mono= takes no parameter %s" % ", ".join(sorted(unknown)))
            mono = dict(MONO_DEFAULTS, **(mono if isinstance(mono, dict) else {}))
        self.mono_params = mono or None
        if init:
            unknown = set(init) - set(INIT_DEFAULTS) if isinstance(init, dict) else ()
            if unknown:
                raise TypeError("init= takes no parameter %s" % ", ".join(sorted(unknown)))
            if not mono:
                raise TypeError("init= starts the mono loop without a right image: it needs mono=")
            init = dict(INIT_DEFAULTS, **(init if isinstance(init, dict) else {}))
        self.init_params = init or None
        if window_ba:
            if tracker != "opflow":
                raise TypeError("window_ba= needs the optical-flow tracker: its key lists are the window's point tracks")
            unknown = set(window_ba) - set(WINDOW_BA_DEFAULTS) if isinstance(window_ba, dict) else ()
            if unknown:
                raise TypeError("window_ba= takes no parameter %s" % ", ".join(sorted(unknown)))
            window_ba = dict(WINDOW_BA_DEFAULTS, **(window_ba if isinstance(window_ba, dict) else {}))
        self.window_ba = window_ba or None
        if keyframe_db and tracker != "bow":
            raise TypeError("keyframe_db= needs tracker 'bow': the database holds the keyframes' BowVectors")
        if relocalize and not keyframe_db:
            raise TypeError("relocalize= needs keyframe_db=N: the candidates come from the keyframe database")
        if recover and not relocalize:
            raise TypeError("recover= needs relocalize=M: a lost sequence adopts the verified candidate's pose")
        if recover:
            unknown = set(recover) - set(RECOVER_DEFAULTS) if isinstance(recover, dict) else ()
            if unknown:
                raise TypeError("recover= takes no parameter %s" % ", ".join(sorted(unknown)))
            recover = dict(RECOVER_DEFAULTS, **(recover if isinstance(recover, dict) else {}))
        self.recover = recover or None
        if loop_close and not relocalize:
            raise TypeError("loop_close= needs relocalize=M: the loop edge is the verified candidate's pose")
        if loop_close and recover:
            raise TypeError("loop_close= and recover= are not combined yet")
        if loop_close:
            unknown = set(loop_close) - set(LOOP_DEFAULTS) if isinstance(loop_close, dict) else ()
            if unknown:
                raise TypeError("loop_close= takes no parameter %s" % ", ".join(sorted(unknown)))
            loop_close = dict(LOOP_DEFAULTS, **(loop_close if isinstance(loop_close, dict) else {}))
        self.loop_close = loop_close or None
        if pnp and not relocalize:
            raise TypeError("pnp= needs relocalize=M: it runs in front of the verification's pose stage")
        if pnp:
            unknown = set(pnp) - set(PNP_DEFAULTS) if isinstance(pnp, dict) else ()
            if unknown:
                raise TypeError("pnp= takes no parameter %s" % ", ".join(sorted(unknown)))
            pnp = dict(PNP_DEFAULTS, **(pnp if isinstance(pnp, dict) else {}))
        self.pnp = pnp or None
        if tracker == "bow" and vocab is None:
            raise ValueError("tracker 'bow' needs vocab=: a synth.Vocabulary, a callable f(context) -> handle, or a handle of context=")
        if tracker != "bow" and vocab is not None:
            raise TypeError("tracker %r takes no vocabulary" % (tracker,))
        self.dev = torch.device("cuda", device)
        torch.cuda.set_device(self.dev)
        self.S, self.width, self.height = int(nseq), int(width), int(height)
        self.keyframe_every = int(keyframe_every)
        # the context runs on a torch stream of its own (pipeline.py: handle 0 would mean "the context's own stream")
        self.stream = torch.cuda.Stream(device=self.dev)
        # context=: the caller's capi.Context (e.g. the one a vocabulary was trained on); it is moved onto the loop's stream and
        # stays the caller's to close
        self._own_ctx = context is None
        self.ctx = capi.Context(device, stream=self.stream.cuda_stream) if context is None else context
        if context is not None:
            context.set_stream(self.stream.cuda_stream)
        self.vocab, self._own_vocab = None, False
        self.db = None          # the keyframe database (keyframe_db=N), borrowed from the loop
        self.store = None       # the keyframe store (relocalize=M), borrowed from the loop
        prm = capi.VOParams(self.width, self.height, int(nlevels), float(scale), int(target), float(init_th), float(min_th),
                            (C.c_double * 4)(*[float(k) for k in K]), float(bf), self.keyframe_every)
        self.params, self.tracker = prm, tracker
        if tracker == "opflow":
            self.vo = capi.VO(self.ctx, prm, self.S)
            if self.window_ba:                # None = off: no call is made
                try:
                    self.ctx.check(self.vo.window_ba_enable(capi.VOWindowBA(*[int(self.window_ba[k]) for k in (
                        "iters", "fixed", "min_obs", "min_points")])))
                except Exception:
                    self.close()
                    raise
        else:
            try:
                trk = _tracker(tracker, nlevels, tracker_params)
                if tracker == "bow":
                    if hasattr(vocab, "c"):           # a synth.Vocabulary: upload it
                        self.vocab, self._own_vocab = self.ctx.vocab_create(vocab), True
                    elif callable(vocab):
                        self.vocab, self._own_vocab = vocab(self.ctx), True
                    elif context is None:
                        raise ValueError("a vocabulary handle belongs to a context: pass that context as context=")
                    else:
                        self.vocab = vocab
                    self.vo = capi.VO(self.ctx, prm, self.S, bow=trk, vocab=self.vocab)
                    if keyframe_db:               # 0 = off: no call is made
                        self.ctx.check(self.vo.bow_db_enable(keyframe_db))
                        self.db = self.vo.bow_db()
                        if relocalize:                # 0 = off: no call is made
                            self.ctx.check(self.vo.reloc_enable(relocalize))
                            self.store = self.vo.kf_store()
                            if pnp:                   # None = off: no call is made. With recover= / loop_close= the library refuses
                                self.ctx.check(self.vo.reloc_pnp_enable(**pnp))
                            if recover:               # None = off: no call is made
                                self.ctx.check(self.vo.recover_enable(capi.VORecover(*[int(recover[k]) for k in (
                                    "lost_inliers", "topk", "exclude_newest", "min_inliers")])))
                            if loop_close:            # None = off: no call is made
                                lc = loop_close
                                self.ctx.check(self.vo.loop_enable(capi.VOLoop(int(lc["topk"]), int(lc["exclude_newest"]), int(lc["min_inliers"]),
                                                                               int(lc["iters"]), float(lc["w_rot"]), float(lc["w_trans"]))))
                elif tracker == "lsh":
                    self.vo = capi.VO(self.ctx, prm, self.S, lsh=trk)
                else:
                    self.vo = capi.VO(self.ctx, prm, self.S, trk)
            except Exception:
                self.vo = None
                self.close()
                raise
        if self.mono_params:                  # None = off: no call is made. The library refuses what the mode does not cover
            try:
                self.ctx.check(self.vo.mono_enable(capi.VOMono(float(self.mono_params["cos_parallax_max"]),
                                                               float(self.mono_params["chi2_max"]), int(self.mono_params["cell"]))))
            except Exception:
                self.close()
                raise
        if self.init_params:
            try:
                tvp = {k: v for k, v in self.init_params.items() if k != "min_tracks"}
                self.ctx.check(self.vo.mono_init_enable(capi.VOMonoInit(capi.two_view_params(**tvp), int(self.init_params["min_tracks"]))))
            except Exception:
                self.close()
                raise
        self._Tcw0 = None
        self._ragged = False
        self.frame = -1

    def close(self):
        self.db = None                       # borrowed: it goes with the loop
        self.store = None
        if getattr(self, "vo", None) is not None:
            self.vo.close()
            self.vo = None
        if getattr(self, "ctx", None) is not None:
            if getattr(self, "vocab", None) is not None and self._own_vocab:   # after the loop that borrowed it
                self.ctx.vocab_destroy(self.vocab)
            self.vocab = None
            if self._own_ctx:
                self.ctx.close()
            self.ctx = None

    def _enter(self, *tensors):
        """Order the loop's stream after the caller's work on `tensors` and keep their memory alive until it has read them."""
        self.stream.wait_stream(torch.cuda.current_stream(self.dev))
        for x in tensors:
            if x is not None:
                x.record_stream(self.stream)

    def _mask(self, m, what):
        """a bool sequence [S] or an index list -> bool [S]; None stays None"""
        if m is None:
            return None
        m = np.asarray(m)
        if m.dtype != np.bool_:
            idx = m.astype(np.int64).reshape(-1)
            if len(idx) and (idx.min() < 0 or idx.max() >= self.S):
                raise ValueError("%s: sequence index out of range" % what)
            m = np.zeros(self.S, bool)
            m[idx] = True
        if m.shape != (self.S,):
            raise ValueError("%s: a bool sequence of length %d or an index list" % (what, self.S))
        return m

    def _ragged_ok(self):
        if getattr(self, "window_ba", None):
            raise TypeError("ragged batches: window_ba= counts the segment's slots for the whole batch")
        if getattr(self, "mono_params", None):
            raise TypeError("ragged batches: mono= keeps one keyframe segment for the whole batch")
        if self.tracker == "projection_map" or self.db is not None:
            raise TypeError("ragged batches: tracker 'projection_map' and keyframe_db= count keyframes for the whole batch")

    def reset(self, Tcw0, which=None):
        """Tcw0: [S, 4, 4] initial poses (array or tensor); the next step is frame 0. which= (a bool sequence [S] or an index
        list) restarts only those sequences -- Tcw0 is then [S, 4, 4] or [len(which), 4, 4] in ascending sequence order -- and the
        others keep their state: the loop is in ragged mode from then on (step() drives it; reset() without which= leaves it)."""
        if which is not None:
            self._ragged_ok()
        self._sim3 = None      # a Sim(3) query belongs to one frame
        T = torch.as_tensor(np.asarray(Tcw0, np.float32) if not torch.is_tensor(Tcw0) else Tcw0, dtype=torch.float32)
        if which is not None:
            w = self._mask(which, "which")
            T = T.reshape(-1, 16).to(self.dev)
            if T.shape[0] != self.S:
                if T.shape[0] != int(w.sum()):
                    raise ValueError("Tcw0: [S, 4, 4] or one pose per selected sequence")
                full = torch.zeros(self.S, 16, dtype=torch.float32, device=self.dev)
                full[torch.from_numpy(np.flatnonzero(w)).to(self.dev)] = T
                T = full
            T = T.contiguous()
            self._enter(T)
            self._Tcw0 = T
            self.ctx.check(self.vo.reset_seq_dev(w, T.data_ptr()))
            self._ragged = True
            self.frame = int(self.vo.frames()[0].max())
            return
        T = T.reshape(self.S, 16).to(self.dev).contiguous()
        self._enter(T)
        self._Tcw0 = T
        self.vo.reset_dev(T.data_ptr())
        self._ragged = False
        self.frame = -1

    def step_rc(self, left, right=None, active=None, keyframe=None):
        """One frame; returns the library's status code (0 or a negative TB_E* code)."""
        self._sim3 = None      # a Sim(3) query belongs to one frame
        if getattr(self, "window_ba", None) and (active is not None or keyframe is not None):
            self._ragged_ok()
        assert left.dtype == torch.uint8 and left.is_cuda and tuple(left.shape) == (self.S, self.height, self.width)
        left = left.contiguous()
        if right is not None:
            assert right.dtype == torch.uint8 and right.is_cuda and tuple(right.shape) == tuple(left.shape)
            right = right.contiguous()
        self._enter(left, right)
        if active is None and keyframe is None and not self._ragged:
            rc = self.vo.step_dev(left.data_ptr(), right.data_ptr() if right is not None else None, self.width,
                                  self.width * self.height)
            if rc == 0:
                self.frame += 1
            return rc
        self._ragged_ok()
        rc = self.vo.step_ragged_dev(left.data_ptr(), right.data_ptr() if right is not None else None, self.width,
                                     self.width * self.height, self._mask(active, "active"), self._mask(keyframe, "keyframe"))
        if rc == 0:
            self._ragged = True   # tb_vo_step_dev may refuse from now on; the ragged entry serves every step
            self.frame = int(self.vo.frames()[0].max())
        return rc

    def step(self, left, right=None, active=None, keyframe=None):
        """left / right: uint8 device tensors [S, H, W]; right may be None unless some sequence has a keyframe in this step.
        active= (bool [S] or an index list): only these sequences take the frame, the others keep their state bit for bit and
        their image slabs are ignored. keyframe=: these sequences take a keyframe now, whatever the cadence says. Either one makes
        the step a ragged one (tb_vo_step_ragged_dev); frames() tells where every sequence is."""
        self.ctx.check(self.step_rc(left, right, active, keyframe))

    def frames(self):
        """(frames [S], kf_frames [S]) int32 numpy arrays: every sequence's frame index (-1 before its first step) and the frame
        index of its keyframe (-1: none)"""
        return self.vo.frames()

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

    @property
    def match_capacity(self):
        """Rows of a sequence's match list: key_pitch, or the map's capacity for tracker "projection_map" (one match per map
        point at most)."""
        return self.vo.map_state_dev()["capacity"] if self.tracker == "projection_map" else self.key_pitch

    def matches(self):
        """The step's matches: (rows [S, M, 4] int32 = queryIdx, trainIdx, imgIdx, distance bits, M = match_capacity; counts [S];
        matcher flags [S])"""
        P = self.match_capacity
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

    # ---- projection trackers (tracker "projection" / "projection_map")
    def _pget(self, ptr, shape, typestr, dtype):
        with torch.cuda.stream(self.stream):
            out = torch.as_tensor(_DevArray(ptr, shape, typestr), device=self.dev).view(dtype).clone()
        torch.cuda.current_stream(self.dev).wait_stream(self.stream)
        return out

    def mp_desc(self):
        """The descriptors that travel with the map points: (current frame's [S, P, 32] uint8, keyframe's [S, P, 32]); entry j
        means something where its map point is valid."""
        d = self.vo.mp_desc_dev()
        P = self.key_pitch
        return (self._pget(d["mp_desc"], (self.S, P, 32), "|u1", torch.uint8),
                self._pget(d["kf_mp_desc"], (self.S, P, 32), "|u1", torch.uint8))

    def map(self):
        """The map of tracker "projection_map": dict(points [S, C, 9] int32 -- tb_mappoint records (pos[3], normal[3], min_dist,
        max_dist as float32, bad as int32), viewed as int32 -- desc [S, C, 32] uint8, counts [S] live points, block_counts
        [S, map_keyframes] points per held keyframe (oldest first), capacity C, map_keyframes, blocks = keyframes held)"""
        m = self.vo.map_state_dev()
        Cp, K = m["capacity"], m["map_keyframes"]
        return dict(points=self._pget(m["points"], (self.S, Cp, 9), "<i4", torch.int32),
                    desc=self._pget(m["desc"], (self.S, Cp, 32), "|u1", torch.uint8),
                    counts=self._pget(m["counts"], (self.S,), "<i4", torch.int32),
                    block_counts=self._pget(m["block_counts"], (self.S, K), "<i4", torch.int32),
                    capacity=Cp, map_keyframes=K, blocks=m["blocks"])

    # ---- searchByBow (tracker "bow"): Frame::SetBow's outputs
    def _bow(self, names):
        d = self.vo.bow_state_dev()
        P = self.key_pitch
        spec = dict(fv_keys=((self.S, P), "<i8", torch.int64), bv_words=((self.S, P), "<i4", torch.int32),
                    bv_values=((self.S, P), "<f8", torch.float64), word_ids=((self.S, P), "<i4", torch.int32),
                    node_ids=((self.S, P), "<i4", torch.int32), fv_counts=((self.S,), "<i4", torch.int32),
                    bv_counts=((self.S,), "<i4", torch.int32))
        out = {}
        for pre in ("", "kf_"):
            out[pre or "cur"] = {n: self._pget(d[pre + n], *spec[n]) for n in names}
        return out["cur"], out["kf_"]

    def feature_vector(self):
        """(current frame, keyframe): each dict(fv_keys [S, P] int64 = node id << 32 | key index, ascending -- the FeatureVector's
        nodes in map order with every node's keys in insertion order --, fv_counts [S], word_ids [S, P], node_ids [S, P] per key)"""
        return self._bow(("fv_keys", "fv_counts", "word_ids", "node_ids"))

    def bow_vector(self):
        """(current frame, keyframe): each dict(bv_words [S, P] int32 ascending, bv_values [S, P] float64, bv_counts [S])"""
        return self._bow(("bv_words", "bv_values", "bv_counts"))

    # ---- the keyframe database (tracker "bow", keyframe_db=N): the last N keyframes' BowVectors per sequence
    def _need_db(self):
        if self.db is None:
            raise capi.TBError(capi.TB_ESTATE, "the keyframe database is off: StereoVO(..., tracker='bow', keyframe_db=N)")
        return self.db

    def keyframe_database(self):
        """dict(words [S, N, P] int32, values [S, N, P] float64, counts [S, N], kf_ids [S, N] int32 with -1 = an empty slot,
        nadded = keyframes added since the last reset): keyframe number a sits in slot a % N; kf_id = its frame index"""
        db = self._need_db()
        with torch.cuda.stream(self.stream):
            out = db.state(self.dev)
        torch.cuda.current_stream(self.dev).wait_stream(self.stream)
        return out

    def query_keyframes(self, topk=4, exclude_newest=1):
        """TemplatedVocabulary::score of the current frame's BowVector (v1) against every keyframe its own sequence's database
        holds, the exclude_newest most recent ones left out (1: the keyframe being tracked against). Device tensors:
        dict(scores [S, N] float64, NaN where a slot is empty or excluded; top_slot / top_kf [S, topk] int32 and top_score
        [S, topk] float64, best first, -1 / NaN past top_count [S]). No host synchronisation."""
        db = self._need_db()
        d = self.vo.bow_state_dev()
        with torch.cuda.stream(self.stream):
            out = db.query_ptr(d["bv_words"], d["bv_values"], d["bv_counts"], self.key_pitch, topk, exclude_newest, self.dev)
        torch.cuda.current_stream(self.dev).wait_stream(self.stream)
        for t in out.values():
            t.record_stream(self.stream)
        return out

    # ---- relocalisation (tracker "bow", keyframe_db=N, relocalize=M): the keyframes themselves and candidate verification
    def _need_store(self):
        if self.store is None:
            raise capi.TBError(capi.TB_ESTATE, "relocalisation is off: StereoVO(..., tracker='bow', keyframe_db=N, relocalize=M)")
        return self.store

    def keyframe_store(self):
        """dict(keys [S, N, P, 7] int32 records, desc [S, N, P, 32], fv_keys [S, N, P] int64, map_points [S, N, P, 3], mp_valid
        [S, N, P], counts / fv_counts / kf_ids [S, N] with kf_id -1 = an empty slot, Tcw [S, N, 4, 4], nadded): slot a % N holds
        keyframe number a as its snapshot was, with the pose its frame was given"""
        st = self._need_store()
        with torch.cuda.stream(self.stream):
            out = st.state(self.dev)
        torch.cuda.current_stream(self.dev).wait_stream(self.stream)
        return out

    def relocalize(self, topk=4, exclude_newest=1, min_inliers=50):
        """Verify the database's best topk candidates for the current frame: searchByBow against each stored keyframe, the rows
        through its map points, PoseOptimization seeded with its pose. Device tensors: query_keyframes' dict plus cand_kf /
        cand_matches / cand_rows / cand_inliers / cand_flags [S, topk] int32, cand_Tcw [S, topk, 4, 4], best_rank / best_kf [S]
        (-1: no candidate reached min_inliers -- ORB-SLAM's figure is 50; the reference has no such step) and best_Tcw [S, 4, 4]
        (the identity when -1). A query: the loop's pose, points and keyframe stay. No host synchronisation.
        With pnp=: also pnp_rows [S, topk] int32 (the rows before the gather), pnp_consensus [S, topk], pnp_winner [S, topk, 2],
        pnp_Tcw [S, topk, 4, 4], pnp_took [S, topk] uint8 (1: the pair went on with its consensus rows and the PnP pose) -- copies."""
        self._need_store()
        self._sim3 = None      # and to one verification: refine_sim3 needs a relocalize_sim3 after this call
        with torch.cuda.stream(self.stream):
            rc, out = self.vo.relocalize_dev(topk, exclude_newest, min_inliers, self.db.capacity, self.dev)
            if rc == 0 and self.pnp:
                st = self.store.pnp_state(self.dev, topk)
                for k, name in (("row_counts", "pnp_rows"), ("consensus", "pnp_consensus"), ("winner", "pnp_winner"), ("Tcw", "pnp_Tcw"),
                                ("took", "pnp_took")):
                    out[name] = st[k].clone().reshape((self.S, int(topk)) + tuple(st[k].shape[1:]))
        self.ctx.check(rc)
        torch.cuda.current_stream(self.dev).wait_stream(self.stream)
        for t in out.values():
            t.record_stream(self.stream)
        return out

    def relocalize_sim3(self, fixed_scale=True, min_consensus=20, **params):
        """After relocalize(topk, ...), on the same topk candidates: the similarity transform between the current frame's own map (its carried points, in its
        camera) and each candidate's stored map (in the stored keyframe's camera), X_current = s R12 X_stored + t12, by Horn's
        closed form in a RANSAC over the verification's matches. Device tensors: S12 [S, 4, 4] float32, srt [S, 8] float64 (the unit
        quaternion w x y z, t12, s), consensus [S] (the winner's, 0 when none), best_rank / best_kf [S] (-1: no candidate reached
        min_consensus -- ORB-SLAM's figure is 20) and the per-candidate cand_rows / cand_consensus / cand_flags [S, topk],
        cand_S12 [S, topk, 4, 4], cand_srt [S, topk, 8]. fixed_scale=True suits a stereo map, whose scale is metric. A query: no
        state tensor changes. No host synchronisation. params: hypotheses, chi2_max, seed."""
        self._need_store()
        with torch.cuda.stream(self.stream):
            rc, out = self.vo.relocalize_sim3_dev(self.dev, min_consensus=min_consensus, fixed_scale=fixed_scale, **params)
            if rc == 0:
                pick = out["best_rank"].clamp(min=0).long().view(-1, 1)
                cons = out["cand_consensus"].gather(1, pick).view(-1)
                out["consensus"] = torch.where(out["best_rank"] >= 0, cons, torch.zeros_like(cons))
                out["S12"], out["srt"] = out["best_S12"], out["best_srt"]
        self.ctx.check(rc)
        torch.cuda.current_stream(self.dev).wait_stream(self.stream)
        for t in out.values():
            t.record_stream(self.stream)
        self._sim3 = out      # refine_sim3 seeds from its cand_srt / cand_consensus
        return out

    def refine_sim3(self, fixed_scale=True, min_inliers=20, use_for_graph=False, **params):
        """After relocalize_sim3(...): ORB-SLAM's OptimizeSim3 on every candidate -- the similarity refined on the reprojection error
        of the matched keys' pixels in both images, from the candidate's cand_srt and its RANSAC inliers. Device tensors: srt [S, 8]
        float64, S12 [S, 4, 4] float32, inliers [S] and stats [S, 8] of the candidate relocalize_sim3 selected (the identity, 0 and
        stats[7] = 2 when none), and cand_srt / cand_S12 / cand_inliers / cand_stats [S, topk, ...]. use_for_graph=True hands the
        refined transform to the next loop_sim3() as its loop edge where the refined inliers reach min_inliers (ORB-SLAM asks for
        20); otherwise no state changes. No host synchronisation. params: th2, iters_first, iters_bad, iters_clean, min_keep."""
        self._need_store()
        if getattr(self, "_sim3", None) is None:
            raise capi.TBError(capi.TB_ESTATE, "refine_sim3 needs a relocalize_sim3 of this frame")
        with torch.cuda.stream(self.stream):
            rc, out = self.vo.refine_sim3_dev(self.dev, self._sim3, min_inliers=min_inliers, use_for_graph=bool(use_for_graph),
                                              fixed_scale=fixed_scale, **params)
            if rc == 0:
                out["srt"], out["S12"], out["inliers"], out["stats"] = out["best_srt"], out["best_S12"], out["best_inliers"], out["best_stats"]
        self.ctx.check(rc)
        torch.cuda.current_stream(self.dev).wait_stream(self.stream)
        for t in out.values():
            t.record_stream(self.stream)
        return out

    def search_sim3(self, th=7.5, th_high=100, use_for_refine=True, srt=None):
        """After relocalize_sim3(...): ORB-SLAM's SearchBySim3 on every candidate -- each frame's points are taken through the
        candidate's similarity into the other frame, a scale-dependent window there is searched by Hamming distance (th: the window in
        level pixels, th_high: the largest distance accepted) and the pairs on which both directions agree join the RANSAC's inliers.
        Device tensors: new [S] and total [S] of the candidate relocalize_sim3 selected (0 when none), cand_new / cand_total [S, topk]
        and cand_stats [S, topk, 8] int32 (tried, searched 1 -> 2; tried, searched 2 -> 1; accepted 1 -> 2, 2 -> 1; new pairs; flag,
        2 = skipped). srt [S, topk, 8]: search under these transforms (a refine_sim3's cand_srt) in place of relocalize_sim3's.
        use_for_refine=True: the next refine_sim3 runs on the widened lists, every row active; otherwise no state changes. A query of
        the loop: it ends in the same bytes whether or not this is called. No host synchronisation."""
        self._need_store()
        if getattr(self, "_sim3", None) is None:
            raise capi.TBError(capi.TB_ESTATE, "search_sim3 needs a relocalize_sim3 of this frame")
        seeds = self._sim3 if srt is None else dict(self._sim3, cand_srt=srt.contiguous())
        with torch.cuda.stream(self.stream):
            rc, out = self.vo.search_sim3_dev(self.dev, seeds, th=th, th_high=th_high, use_for_refine=bool(use_for_refine))
            if rc == 0:
                out["new"], out["total"] = out["best_new"], out["best_total"]
        self.ctx.check(rc)
        torch.cuda.current_stream(self.dev).wait_stream(self.stream)
        for t in out.values():
            t.record_stream(self.stream)
        return out

    def loop_sim3(self, iters=10, fixed_scale=True, w_rot=1.0, w_trans=1.0, w_scale=1.0):
        """After relocalize_sim3(...): the Sim(3) pose graph of the stored keyframes and the current frame, the Sim(3) winner as the
        loop edge (the node of best_kf -> the frame's node, Z = best_srt), optimised by the device solver. Device tensors, copies:
        nnodes [S] = live keyframes + 1, node_kf [S, N + 1] (the frame index for the current frame, -1 unused), before / after
        [S, N + 1, 8] float64 srt nodes (the quaternion w x y z, t, s), edges [S, N + 1, 96] uint8 (capi.PG_SIM3_EDGE records),
        edge_counts [S] (0: no winner, or fewer than 2 stored keyframes), stats [S, 8] float64 (stats[7] = -1: the winner's
        keyframe has left the ring). fixed_scale=True suits a stereo map. A query: no state tensor changes -- adopting the corrected
        nodes is not done here. No host synchronisation."""
        self._need_store()
        with torch.cuda.stream(self.stream):
            rc, out = self.vo.loop_sim3_dev(self.dev, iters, fixed_scale, w_rot, w_trans, w_scale)
        self.ctx.check(rc)
        torch.cuda.current_stream(self.dev).wait_stream(self.stream)
        for t in out.values():
            t.record_stream(self.stream)
        return out

    def recovery(self):
        """The recovery state after the last step (recover=...): dict(lost [S] uint8 and track_inliers [S] int32 -- the tracker's own
        inlier count, before any adoption --, recovered_kf [S] int32 = the frame index of the keyframe the sequence adopted in
        this step or -1, kf_ids [S] int32 = the frame index of the keyframe each sequence tracks against). TB_ESTATE when off."""
        if self.recover is None:
            raise capi.TBError(capi.TB_ESTATE, "recovery is off: StereoVO(..., keyframe_db=N, relocalize=M, recover=True)")
        d = self.vo.recover_state_dev()
        i32 = ((self.S,), "<i4", torch.int32)
        return dict(lost=self._pget(d["lost"], (self.S,), "|u1", torch.uint8), track_inliers=self._pget(d["track_inliers"], *i32),
                    recovered_kf=self._pget(d["recovered_kf"], *i32), kf_ids=self._pget(d["kf_ids"], *i32))

    def loop(self):
        """The loop-correction state of the last keyframe step t > 0 (loop_close=...): dict(closed [S] uint8, loop_kf [S] int32 = the
        kf_id of the keyframe the loop closed with or -1, loop_inliers [S], nnodes [S] = live keyframes + 1, node_kf [S, N + 1] (the
        frame index for the current frame, -1 unused), before / after [S, N + 1, 4, 4], edges [S, N + 1, 80] uint8 (capi.PG_EDGE
        records), edge_counts [S], stats [S, 8] float64). TB_ESTATE when off."""
        if self.loop_close is None:
            raise capi.TBError(capi.TB_ESTATE, "loop correction is off: StereoVO(..., keyframe_db=N, relocalize=M, loop_close=True)")
        d = self.vo.loop_state_dev()
        S, nn = self.S, self.db.capacity + 1
        i32 = ((S,), "<i4", torch.int32)
        return dict(closed=self._pget(d["closed"], (S,), "|u1", torch.uint8), loop_kf=self._pget(d["loop_kf"], *i32),
                    loop_inliers=self._pget(d["loop_inliers"], *i32), nnodes=self._pget(d["nnodes"], *i32),
                    node_kf=self._pget(d["node_kf"], (S, nn), "<i4", torch.int32),
                    before=self._pget(d["before"], (S, nn, 4, 4), "<f4", torch.float32),
                    after=self._pget(d["after"], (S, nn, 4, 4), "<f4", torch.float32),
                    edges=self._pget(d["edges"], (S, nn, capi.PG_EDGE.itemsize), "|u1", torch.uint8),
                    edge_counts=self._pget(d["edge_counts"], *i32), stats=self._pget(d["stats"], (S, 8), "<f8", torch.float64))

    def recovery_rings(self):
        """(word ids, node ids) [S, N, P] int32 of the stored keyframes, slot-aligned with keyframe_store()"""
        if self.recover is None:
            raise capi.TBError(capi.TB_ESTATE, "recovery is off: StereoVO(..., keyframe_db=N, relocalize=M, recover=True)")
        d = self.vo.recover_state_dev()
        sh = ((self.S, self.db.capacity, self.key_pitch), "<i4", torch.int32)
        return self._pget(d["kf_word_ring"], *sh), self._pget(d["kf_node_ring"], *sh)

    # ---- window BA (window_ba=...)
    def window(self):
        """The window-BA state after the last step: dict(keys [S, E + 1, P, 2], ok [S, E + 1, P] uint8, poses [S, E + 1, 4, 4],
        points [S, P, 3], spawned [S, P] uint8 -- the log of the running segment, slot 0 its keyframe, E = keyframe_every; slots
        past `slots` still hold the previous segment's --, obs [S, (E + 1) P, 5] int32 (kf, pt as integers; u, v, inv_sigma2 as
        float32 bits), obs_counts / n_points [S] int32, stats [S, 8] float64, adopted [S] uint8, refined_poses [S, E + 1, 4, 4]
        and refined_points [S, P, 3] -- the last window and the segment as the BA left it --, slots = frames since the segment's
        keyframe, nslots = E + 1). TB_ESTATE when off."""
        if self.window_ba is None:
            raise capi.TBError(capi.TB_ESTATE, "the window BA is off: StereoVO(..., window_ba=True)")
        d = self.vo.window_state_dev()
        S, P, N = self.S, self.key_pitch, d["nslots"]
        f32, u8, i32 = ("<f4", torch.float32), ("|u1", torch.uint8), ("<i4", torch.int32)
        return dict(keys=self._pget(d["seg_keys"], (S, N, P, 2), *f32), ok=self._pget(d["seg_ok"], (S, N, P), *u8),
                    poses=self._pget(d["seg_pose"], (S, N, 4, 4), *f32), points=self._pget(d["seg_pts"], (S, P, 3), *f32),
                    spawned=self._pget(d["seg_spawned"], (S, P), *u8), obs=self._pget(d["obs"], (S, N * P, 5), *i32),
                    obs_counts=self._pget(d["obs_counts"], (S,), *i32), n_points=self._pget(d["n_points"], (S,), *i32),
                    stats=self._pget(d["stats"], (S, 8), "<f8", torch.float64), adopted=self._pget(d["adopted"], (S,), *u8),
                    refined_poses=self._pget(d["ba_pose"], (S, N, 4, 4), *f32), refined_points=self._pget(d["ba_pts"], (S, P, 3), *f32),
                    slots=d["slot"], nslots=N)

    # ---- mono mode (mono=...)
    def mono(self):
        """The mono state after the last step: dict(kf_keys [S, P, 2] and kf_Tcw [S, 4, 4] -- the key list and pose of the keyframe
        the running segment triangulates against --, alive [S, P] uint8 -- LK has held the key since --, tri_points [S, P, 3],
        tri_flags [S, P] uint8 (tb_linear_triangle_batch_dev's codes), tri_tally [S, 6] int32, survivors / added [S] int32 -- the
        last mono keyframe's triangulation, before the merge renumbered the keys, and the merge's counts). TB_ESTATE when off."""
        if self.mono_params is None:
            raise capi.TBError(capi.TB_ESTATE, "the mono mode is off: StereoVO(..., mono=True)")
        d = self.vo.mono_state_dev()
        S, P = self.S, self.key_pitch
        f32, u8, i32 = ("<f4", torch.float32), ("|u1", torch.uint8), ("<i4", torch.int32)
        return dict(kf_keys=self._pget(d["kf_keys_xy"], (S, P, 2), *f32), kf_Tcw=self._pget(d["kf_Tcw"], (S, 4, 4), *f32),
                    alive=self._pget(d["alive"], (S, P), *u8), tri_points=self._pget(d["tri_points"], (S, P, 3), *f32),
                    tri_flags=self._pget(d["tri_flags"], (S, P), *u8), tri_tally=self._pget(d["tri_tally"], (S, 6), *i32),
                    survivors=self._pget(d["survivors"], (S,), *i32), added=self._pget(d["added"], (S,), *i32))

    def mono_init(self):
        """The state of the start without a right image after the last step: dict(initialised [S] uint8, init_frame [S] int32 (-1:
        not yet), attempts [S], and every sequence's last attempt: status, consensus [S], winner [S, 2], good / tri [S, 4], Tcw1
        [S, 4, 4]). TB_ESTATE when off."""
        if self.init_params is None:
            raise capi.TBError(capi.TB_ESTATE, "the start without a right image is off: StereoVO(..., mono=True, init=True)")
        d = self.vo.mono_init_state_dev()
        S = self.S
        f32, u8, i32 = ("<f4", torch.float32), ("|u1", torch.uint8), ("<i4", torch.int32)
        return dict(initialised=self._pget(d["initialised"], (S,), *u8), init_frame=self._pget(d["init_frame"], (S,), *i32),
                    attempts=self._pget(d["attempts"], (S,), *i32), status=self._pget(d["status"], (S,), *i32),
                    consensus=self._pget(d["consensus"], (S,), *i32), winner=self._pget(d["winner"], (S, 2), *i32),
                    good=self._pget(d["good"], (S, 4), *i32), tri=self._pget(d["tri"], (S, 4), *i32),
                    Tcw1=self._pget(d["Tcw1"], (S, 4, 4), *f32))

    def profile_enable(self, on=True, only=None):
        self.ctx.profile_enable(on, only)

    def profile_report(self):
        return self.ctx.profile_report()

    def synchronize(self):
        self.stream.synchronize()
