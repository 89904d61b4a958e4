"""Cases at fx != fy for every entry point that takes a camera: shared by tests/test_aniso_references.py (CPU: each reference
recovers the truth its case was built from, and notices fx and fy exchanged) and tests/test_gpu_aniso.py (the kernels against
those references). Every case is one of its operator's smallest existing shapes, rebuilt with K_ANISO (or, for the modules built
on a 640 x 240 image, the same fy / fx ratio on the module's own K) through the generator's optional K."""
import functools

import numpy as np

from trackingbench_slam_amd import synth, synth_seq

import gauge_cases as gc
import pnp_cases as pc
import sim3_cases as sc
import triangulate_cases as trc
import two_view_cases as tc
from ba_cases import K_ANISO

RATIO = K_ANISO[1] / K_ANISO[0]          # ~ 0.907: no power-of-two ratio


def aniso(K):
    """a module's own K with K_ANISO's fy / fx ratio"""
    return (float(K[0]), float(K[0]) * RATIO, float(K[2]), float(K[3]))


def exchanged(K):
    """fx where fy belongs and the reverse"""
    return (K[1], K[0], K[2], K[3])


def exchanged_cam(cam):
    c = cam.copy()
    c["fx"], c["fy"] = cam["fy"], cam["fx"]
    return c


# ------------------------------------------------------------------------------------------------------------ pose solver
POSE = ((1, 9, "id"), (2, 300, "id"), (2, 300, "y180"))      # seed, n, gauge: below the n < 10 round break; the y branch


@functools.lru_cache(maxsize=None)
def pose_case(seed, n, gname, clean=False):
    """(Tcw_true, Tcw_in, obs) under the gauge; clean: no noise, no outliers"""
    Tt, Ti, obs = synth.pose_problem(seed, n, K_ANISO, noise_px=0.0 if clean else 0.5, outlier_frac=0.0 if clean else 0.15)
    G = gc.get(gname)
    Tin, o = gc.gauge_pose_problem(Ti, obs, G)
    return gc.gauge_poses(Tt, G), Tin, o


# -------------------------------------------------------------------------------------------------------------- P3P-RANSAC
K_PNP = aniso(pc.K)
RANSAC_PITCH = 320
RANSAC_SEED = 5
RANSAC_N = (65, pc.CHUNK + 1)


@functools.lru_cache(maxsize=None)
def pnp_case(i, clean=False):
    """(obs [RANSAC_PITCH], good, Tcw) of problem i: RANSAC_N[i] rows, 50 % outliers and 0.5 px noise (clean: neither)"""
    kw = dict(outliers=0.0, noise=0.0) if clean else {}
    return pc.problem(400 + i, RANSAC_N[i], RANSAC_PITCH, K=K_PNP, **kw)


# ------------------------------------------------------------------------------------------------------------------ Sim(3)
SIM3_NOISE = 0.002     # 0.2 % of the depth: rows on both sides of the chi2 gate, so that the gate's pixels matter (at the
#                        module's 0.05 % every good row passes under either focal length and nothing would notice an exchange)


@functools.lru_cache(maxsize=None)
def sim3_case(i, fixed, clean=False):
    """(rows [RANSAC_PITCH], good, (s, R, t)) of problem i; fixed: rows whose true scale is 1"""
    kw = dict(outliers=0.0, noise=0.0) if clean else dict(noise=SIM3_NOISE)
    return sc.problem(400 + i, RANSAC_N[i], RANSAC_PITCH, T=sc.truth(s=1.0) if fixed else None, K=K_ANISO, **kw)


# ---------------------------------------------------------------------------------------------------------------- two-view
TWO_VIEW_SEED = 11
TWO_VIEW = {"initialises": (2.5, 0.1, 0.2), "refused": (0.5, 0.1, 0.0)}     # baseline in metres, pixel noise, outlier fraction


@functools.lru_cache(maxsize=None)
def two_view_case(name, clean=False):
    """(xy0, xy1, good, R, t) of a 256-row forward-motion problem"""
    d, noise, out = TWO_VIEW[name]
    return tc.problem(1, 256, "forward", d, 0.0 if clean else noise, 0.0 if clean else out, K=K_ANISO)


# ----------------------------------------------------------------------------------------------------------- triangulation
@functools.lru_cache(maxsize=None)
def triangulate_case():
    return trc.build(K=K_ANISO)


# -------------------------------------------------------------------------------------------------------------- projection
@functools.lru_cache(maxsize=None)
def projection_case(seed, K=K_ANISO):
    return synth.projection_case(seed, 500, 400, K=K)


def projection_args(c, cam=None):
    return (c["Tcw"], c["cam"] if cam is None else cam, c["width"], c["height"], c["k1"], c["d1"], c["taken1"])


# ---------------------------------------------------------------------------------------------------------- stereo / flow
FLOW_PAIRS = ((7, 96, 64, 40), (9, 333, 211, 300))       # the two smallest synthetic pairs of tests/test_gpu_flow.py
FLOW_BF = 40.0


@functools.lru_cache(maxsize=None)
def flow_case(seed, w, h, n):
    """(left, right, camera, keys): a synthetic stereo pair and the left image's ORB keys"""
    import oracle
    L, R = synth.frame(seed, w, h, stereo=True)
    lv, sf = oracle.pyramid(L, 8, 0.8)
    k, _, _ = oracle.orb_extract(lv, sf, n, 80, 30)
    keys = np.ascontiguousarray(np.stack([k["x"], k["y"]], 1), np.float32)
    return L, R, oracle.camera(*aniso((300.0, 300.0, w / 2, h / 2)), w, h), keys


# ----------------------------------------------------------------------------------------------------------------- VO loop
VO_SEEDS = (0, 1)
VO_FRAMES = 5
VO_KEYFRAME_EVERY = 3


@functools.lru_cache(maxsize=None)
def vo_sequences():
    """(L [T, S, H, W], R, G [T, S, 4, 4]) rendered at K_ANISO, in the layout of tests/test_gpu_vo.py"""
    out = [synth_seq.sequence(s, VO_FRAMES, K=K_ANISO) for s in VO_SEEDS]
    return np.stack([o[0] for o in out], 1), np.stack([o[1] for o in out], 1), np.stack([o[2] for o in out], 1)
