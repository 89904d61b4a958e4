"""A batched, device-resident depth filter (tb_depth_filter_*, include/tb_capi.h): S sequences with up to `pitch` seeds each.

A seed is a pixel of a keyframe with a Gaussian x Beta belief over the inverse range along its ray. Every later frame with a known
pose narrows it: an epipolar zero-mean-SSD search with the affine-warped reference patch, a 1-D alignment along the line, the
range from the two rays and the Vogiatzis-Hernandez update (the rules: include/tb_capi.h and tests/depth_filter_reference.py).
A seed that converges is a map point (points()). The filter is an operator next to the VO loop; it reads poses and images and
changes nothing of a loop:

    vo = StereoVO(S, mono=True); vo.reset(Tcw0)
    df = DepthFilter(S, vo.width, vo.height, K, context=vo)          # shares the loop's context and stream
    for t, left in enumerate(frames):
        vo.step(left, ...)
        df.update(left, vo.Tcw())                                    # the loop's own pose and left image
        if t % vo.keyframe_every == 0:                               # seed at the loop's keyframes, where it has no map point
            xy, n = vo.keys(); _, has_point = vo.map_points()
            df.add_keyframe(left, vo.Tcw(), xy, n, skip=has_point)
    xyz, ok = df.points()
"""
import numpy as np
import torch

from . import capi
from .vo import _DevArray


class DepthFilter:
    """DepthFilter(S, width, height, K, pitch=2048, context=None, **params). params: depth_mean 15, depth_min 2, conv_div 200,
    px_noise 1, max_steps 1000, zmssd_max 2000, align_iters 10 (capi.depth_filter_params) and ref_slots 4. context=: a capi.Context
    (moved onto the filter's own torch stream) or an object with .ctx and .stream such as a StereoVO (both are shared, so the
    filter's calls are ordered with the loop's); None: a context and a stream of the filter's own on `device`.
    Images are uint8 [S, H, W], poses float32 [S, 4, 4] (world -> camera); device tensors or numpy arrays."""

    def __init__(self, S, width, height, K, pitch=2048, context=None, device=0, ref_slots=4, **params):
        self.S, self.width, self.height, self.pitch, self.ref_slots = int(S), int(width), int(height), int(pitch), int(ref_slots)
        self.K = tuple(float(k) for k in K)
        self.params = capi.depth_filter_params(**params)
        self._own_ctx = context is None
        if context is not None and hasattr(context, "ctx") and hasattr(context, "stream"):
            self.ctx, self.stream = context.ctx, context.stream
            self.dev = self.stream.device
        else:
            self.dev = torch.device("cuda", device)
            torch.cuda.set_device(self.dev)
            self.stream = torch.cuda.Stream(device=self.dev)
            self.ctx = capi.Context(device, stream=self.stream.cuda_stream) if context is None else context
            if context is not None:
                context.set_stream(self.stream.cuda_stream)
        self.df = None
        try:
            self.df = capi.DepthFilter(self.ctx, self.S, self.pitch, self.ref_slots, self.width, self.height, self.K, self.params)
        except Exception:
            self.close()
            raise

    def close(self):
        if getattr(self, "df", None) is not None:
            self.df.close()
            self.df = None
        if getattr(self, "ctx", None) is not None:
            if self._own_ctx:
                self.ctx.close()
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- inputs
    def _t(self, x, dtype, shape, what):
        t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
        t = t.to(device=self.dev, dtype=dtype).contiguous()
        if tuple(t.shape) != tuple(shape):
            raise ValueError("%s: shape %s, expected %s" % (what, tuple(t.shape), tuple(shape)))
        return t

    def _frame(self, images, Tcw):
        img = self._t(images, torch.uint8, (self.S, self.height, self.width), "images")
        T = self._t(Tcw, torch.float32, (self.S, 4, 4), "Tcw")
        return img, T

    def _enter(self, *tensors):
        self.stream.wait_stream(torch.cuda.current_stream(self.dev))
        for x in tensors:
            if x is not None:
                x.record_stream(self.stream)

    def _mask(self, m):
        if m is None:
            return None
        m = np.asarray(m)
        if m.dtype != np.bool_:
            idx = m.astype(np.int64).reshape(-1)
            m = np.zeros(self.S, bool)
            m[idx] = True
        if m.shape != (self.S,):
            raise ValueError("active: a bool sequence of length %d or an index list" % self.S)
        return m

    # ---- the operator
    def add_keyframe(self, images, Tcw, keys, counts, skip=None, active=None):
        """A keyframe for every active sequence: keys float32 [S, P, 2] level-0 pixels of which counts [S] are offered, skip
        [S, P] non-zero where a key is not to become a seed (e.g. it holds a map point). The ring takes the slot after the newest
        one and the seeds bound to it are dropped. Returns the keys that found no free entry, an int32 tensor [S]."""
        img, T = self._frame(images, Tcw)
        k = keys if torch.is_tensor(keys) else torch.from_numpy(np.ascontiguousarray(keys, np.float32))
        k = k.to(device=self.dev, dtype=torch.float32).contiguous()
        if k.dim() != 3 or k.shape[0] != self.S or k.shape[2] != 2 or k.shape[1] < 1:
            raise ValueError("keys: [S, P, 2]")
        P = int(k.shape[1])
        c = self._t(counts, torch.int32, (self.S,), "counts")
        sk = None if skip is None else self._t(skip, torch.uint8, (self.S, P), "skip")
        self._enter(img, T, k, c, sk)
        with torch.cuda.stream(self.stream):
            left = torch.zeros(self.S, dtype=torch.int32, device=self.dev)
        self.ctx.check(self.df.add_keyframe_dev(img.data_ptr(), self.width, self.width * self.height, T.data_ptr(), k.data_ptr(),
                                                c.data_ptr(), P, sk.data_ptr() if sk is not None else 0, self._mask(active),
                                                left.data_ptr()))
        torch.cuda.current_stream(self.dev).wait_stream(self.stream)
        left.record_stream(torch.cuda.current_stream(self.dev))
        return left

    def update(self, images, Tcw, active=None):
        """One update of every active seed of every active sequence against (images, Tcw): no synchronisation, no copy."""
        img, T = self._frame(images, Tcw)
        self._enter(img, T)
        self.ctx.check(self.df.update_dev(img.data_ptr(), self.width, self.width * self.height, T.data_ptr(), self._mask(active)))

    def clear(self, which=None):
        self.ctx.check(self.df.clear(self._mask(which)))

    # ---- outputs: copies (on the filter's stream, ordered before the caller's stream)
    def _get(self, key, shape, typestr, np_dtype):
        ptr = self.df.state_dev()[key]
        with torch.cuda.stream(self.stream):
            raw = torch.as_tensor(_DevArray(ptr, shape, typestr), device=self.dev).clone()
        torch.cuda.current_stream(self.dev).wait_stream(self.stream)
        return raw.cpu().numpy().view(np_dtype).reshape(shape[:2])

    def seeds(self):
        """The entries as a numpy record array [S, pitch] of capi.DF_SEED"""
        return self._get("seeds", (self.S, self.pitch, capi.DF_SEED.itemsize), "|u1", capi.DF_SEED)

    def trace(self):
        """What the last update did with every entry: a numpy record array [S, pitch] of capi.DF_TRACE"""
        return self._get("traces", (self.S, self.pitch, capi.DF_TRACE.itemsize), "|u1", capi.DF_TRACE)

    def slots(self):
        """(slot_Tcw float32 [S, ref_slots, 4, 4] numpy, newest_slot int32 [S])"""
        st = self.df.state_dev()
        with torch.cuda.stream(self.stream):
            T = torch.as_tensor(_DevArray(st["slot_Tcw"], (self.S, self.ref_slots, 4, 4), "<f4"), device=self.dev).view(torch.float32).clone()
        torch.cuda.current_stream(self.dev).wait_stream(self.stream)
        return T.cpu().numpy(), st["newest_slot"]

    def points(self, release=False):
        """(xyz float32 [S, pitch, 3], ok uint8 [S, pitch]) device tensors: the world points of the converged seeds. release=True
        frees those entries for the next keyframe's seeds."""
        with torch.cuda.stream(self.stream):
            xyz = torch.empty((self.S, self.pitch, 3), dtype=torch.float32, device=self.dev)
            ok = torch.empty((self.S, self.pitch), dtype=torch.uint8, device=self.dev)
        self.ctx.check(self.df.points_dev(xyz.data_ptr(), ok.data_ptr(), release))
        torch.cuda.current_stream(self.dev).wait_stream(self.stream)
        xyz.record_stream(torch.cuda.current_stream(self.dev))
        ok.record_stream(torch.cuda.current_stream(self.dev))
        return xyz, ok
