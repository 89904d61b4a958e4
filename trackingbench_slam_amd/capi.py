"""ctypes binding of the C ABI (include/tb_capi.h) exported by libtb_hip.so.

This is plumbing, not the product: every call goes straight into the HIP library.  There is no
CPU fallback -- if the library is missing or no GPU is usable the calls raise.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TB_HIP_LIB") or os.path.join(_HERE, "libtb_hip.so")   # TB_HIP_LIB: experiment builds
_LIB = None

KEYPOINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
MATCH = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])
CORNER = np.dtype([("x", "<i4"), ("y", "<i4"), ("score", "<i4")])
OBS = np.dtype([("u", "<f4"), ("v", "<f4"), ("X", "<f4"), ("Y", "<f4"), ("Z", "<f4"), ("inv_sigma2", "<f4")])
SIM3_ROW = np.dtype([("X1", "<f4"), ("Y1", "<f4"), ("Z1", "<f4"), ("X2", "<f4"), ("Y2", "<f4"), ("Z2", "<f4"), ("inv_sigma2_1", "<f4"),
                     ("inv_sigma2_2", "<f4")])
SIM3_OBS_ROW = np.dtype([("X1", "<f4"), ("Y1", "<f4"), ("Z1", "<f4"), ("X2", "<f4"), ("Y2", "<f4"), ("Z2", "<f4"), ("u1", "<f4"), ("v1", "<f4"),
                         ("u2", "<f4"), ("v2", "<f4"), ("inv_sigma2_1", "<f4"), ("inv_sigma2_2", "<f4")])
BA_OBS = np.dtype([("kf", "<i4"), ("pt", "<i4"), ("u", "<f4"), ("v", "<f4"), ("inv_sigma2", "<f4")])
PG_EDGE = np.dtype([("a", "<i4"), ("b", "<i4"), ("q", "<f8", (4,)), ("t", "<f8", (3,)), ("w_rot", "<f8"), ("w_trans", "<f8")])
PG_SIM3_EDGE = np.dtype([("a", "<i4"), ("b", "<i4"), ("srt", "<f8", (8,)), ("w_rot", "<f8"), ("w_trans", "<f8"), ("w_scale", "<f8")])
CAMERA = np.dtype([("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("width", "<i4"), ("height", "<i4"),
                   ("has_distortion", "<i4"), ("d", "<f4", (5,))])
MAPPOINT = np.dtype([("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_dist", "<f4"), ("max_dist", "<f4"), ("bad", "<i4")])
# tb_df_seed / tb_df_trace of include/tb_types.h (the depth filter)
DF_SEED = np.dtype([("mu", "<f8"), ("sigma2", "<f8"), ("a", "<f8"), ("b", "<f8"), ("z_range", "<f8"), ("u", "<f4"), ("v", "<f4"),
                    ("slot", "<i4"), ("state", "<i4"), ("updates", "<i4"), ("reserved", "<i4")])
DF_TRACE = np.dtype([("score", "<i8"), ("px", "<f8"), ("py", "<f8"), ("z", "<f8"), ("tau", "<f8"), ("flag", "<i4"), ("n", "<i4"),
                     ("win", "<i4"), ("reserved", "<i4")])

TB_OK, TB_EINVAL, TB_ENOMEM, TB_ECAPACITY, TB_EUNSUPPORTED, TB_EDEVICE, TB_ESTATE = 0, -1, -2, -3, -4, -5, -6

# every symbol include/tb_capi.h declares (checked by tests/test_capi_exports.py)
EXPORTS = [
    "tb_create", "tb_destroy", "tb_last_error", "tb_strerror", "tb_version", "tb_set_stream", "tb_synchronize",
    "tb_profile_enable", "tb_profile_only", "tb_profile_report", "tb_debug_force_dense_fast", "tb_debug_ba_plain_obs", "tb_debug_bf_scalar", "tb_measure_copy_seconds", "tb_set_concurrency", "tb_pack_rows_dev",
    "tb_scale_factors", "tb_pyramid_sizes", "tb_orb_quotas",
    "tb_extractor_create", "tb_extractor_destroy", "tb_extractor_set_images_host", "tb_extractor_set_images_dev",
    "tb_extractor_set_levels_host", "tb_extractor_build_pyramid", "tb_extractor_get_level_host", "tb_extractor_orb",
    "tb_extractor_fastgrid", "tb_extractor_counts_host", "tb_extractor_results_host", "tb_extractor_results_dev",
    "tb_extractor_candidates_host", "tb_extractor_copy_results_dev",
    "tb_pyramid", "tb_fast_detect", "tb_orb_extract", "tb_fastgrid_extract",
    "tb_descriptor_distance", "tb_three_maxima", "tb_match_bf", "tb_search_by_bf", "tb_search_by_bf_batch_dev",
    "tb_search_by_violence", "tb_search_by_bow", "tb_search_by_projection", "tb_search_by_projection_map", "tb_frame_grid_batch_dev",
    "tb_search_by_projection_batch_dev", "tb_search_by_projection_map_batch_dev",
    "tb_search_by_violence_batch_dev", "tb_stereo_tracks_to_obs_batch_dev", "tb_vocab_create", "tb_vocab_destroy", "tb_bow_transform",
    "tb_bow_transform_batch_dev", "tb_search_by_bow_batch_dev", "tb_pose_opt", "tb_pose_opt_batch_dev", "tb_local_ba", "tb_local_ba_batch_dev", "tb_ba_obs_stream_positions",
    "tb_clahe", "tb_clahe_dev", "tb_optical_flow_pyr_lk", "tb_optical_flow_pyr_lk_dev", "tb_optical_flow_pyr_lk_batch_dev", "tb_search_by_opflow", "tb_search_by_opflow_batch_dev",
    "tb_find_fundamental_ransac", "tb_reject_with_f", "tb_reject_with_f_batch_dev", "tb_add_map_points_by_stereo", "tb_add_map_points_by_stereo_batch_dev",
    "tb_batch_run", "tb_vo_create", "tb_vo_destroy", "tb_vo_reset_dev", "tb_vo_step_dev", "tb_vo_state_dev",
    "tb_vo_create_ex", "tb_vo_tracker_state_dev", "tb_vo_mp_desc_dev", "tb_vo_map_state_dev",
    "tb_vocab_train", "tb_vocab_train_dev", "tb_vocab_info", "tb_vocab_export",
    "tb_bow_vector_batch_dev", "tb_vo_create_bow", "tb_vo_bow_state_dev",
    "tb_bow_score", "tb_bow_score_batch_dev", "tb_bow_db_create", "tb_bow_db_destroy", "tb_bow_db_clear", "tb_bow_db_add_dev",
    "tb_bow_db_query_dev", "tb_bow_db_state_dev", "tb_vo_bow_db_enable", "tb_vo_bow_db_get",
    "tb_kf_store_create", "tb_kf_store_destroy", "tb_kf_store_clear", "tb_kf_store_add_dev", "tb_kf_store_state_dev",
    "tb_kf_store_work_dev", "tb_relocalize_batch_dev", "tb_reloc_rows_dev", "tb_vo_reloc_enable", "tb_vo_relocalize_dev",
    "tb_vo_kf_store_get", "tb_vo_recover_enable", "tb_vo_recover_state_dev",
    "tb_vo_reset_seq_dev", "tb_vo_step_ragged_dev", "tb_vo_frames",
    "tb_vo_window_ba_enable", "tb_vo_window_state_dev",
    "tb_lsh_draw_bits", "tb_lsh_create", "tb_lsh_destroy", "tb_lsh_info", "tb_match_lsh", "tb_search_by_nn", "tb_search_by_nn_batch_dev",
    "tb_vo_create_lsh",
    "tb_linear_triangle", "tb_linear_triangle_batch_dev", "tb_vo_mono_enable", "tb_vo_mono_state_dev",
    "tb_pose_graph", "tb_pose_graph_batch_dev", "tb_pose_graph_plan", "tb_vo_loop_enable", "tb_vo_loop_state_dev",
    "tb_pnp_ransac", "tb_pnp_ransac_batch_dev", "tb_kf_store_pnp_enable", "tb_kf_store_pnp_state_dev", "tb_vo_reloc_pnp_enable",
    "tb_two_view", "tb_two_view_batch_dev", "tb_vo_mono_init_enable", "tb_vo_mono_init_state_dev",
    "tb_sim3_ransac", "tb_sim3_ransac_batch_dev", "tb_kf_store_sim3_dev", "tb_kf_store_sim3_state_dev", "tb_vo_relocalize_sim3_dev",
    "tb_sim3_optimize", "tb_sim3_optimize_batch_dev", "tb_kf_store_sim3_refine_dev", "tb_kf_store_sim3_refine_state_dev",
    "tb_vo_refine_sim3_dev",
    "tb_search_by_sim3_batch_dev", "tb_kf_store_sim3_search_dev", "tb_kf_store_sim3_search_state_dev", "tb_vo_search_sim3_dev",
    "tb_depth_filter_create", "tb_depth_filter_destroy", "tb_depth_filter_clear", "tb_depth_filter_add_keyframe_dev",
    "tb_depth_filter_update_dev", "tb_depth_filter_points_dev", "tb_depth_filter_state_dev",
    "tb_pose_graph_sim3", "tb_pose_graph_sim3_batch_dev", "tb_pose_graph_sim3_plan", "tb_kf_store_sim3_graph_dev", "tb_vo_loop_sim3_dev",
]

TB_VOC_MAX_L = 8
TB_SCORE_PAIRWISE, TB_SCORE_ALL_PAIRS = 0, 1


class VocabTrainParams(C.Structure):
    """tb_vocab_train_params of include/tb_capi.h"""
    _fields_ = [("k", C.c_int), ("L", C.c_int), ("weighting", C.c_int), ("scoring", C.c_int), ("seed", C.c_uint64), ("max_iters", C.c_int)]


class VocabTrainStats(C.Structure):
    """tb_vocab_train_stats of include/tb_capi.h"""
    _fields_ = [("nnodes", C.c_int), ("nwords", C.c_int), ("capped_nodes", C.c_int), ("empty_clusters", C.c_int),
                ("iters_per_level", C.c_int * TB_VOC_MAX_L)]

    def as_dict(self):
        return dict(nnodes=self.nnodes, nwords=self.nwords, capped_nodes=self.capped_nodes, empty_clusters=self.empty_clusters,
                    iters_per_level=list(self.iters_per_level))


class TBError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("tb error %d: %s" % (code, msg))
        self.code = code


def build(force=False):
    """Compile libtb_hip.so for gfx950 (hipcc cross-compiles without a GPU)."""
    if force or not os.path.exists(LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(_HERE, "csrc"), "-j8"], stdout=subprocess.DEVNULL,
                              stderr=subprocess.DEVNULL)
    return LIB_PATH


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise TBError(TB_EDEVICE, "libtb_hip.so is not built (run __graft_entry__.build())")
        try:
            # One HIP runtime per process: when torch is installed its bundled libamdhip64 must be the one that
            # gets loaded (loading ROCm's copy first makes torch's later initialisation find no GPU).
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        L.tb_last_error.restype = C.c_char_p
        L.tb_strerror.restype = C.c_char_p
        L.tb_version.restype = C.c_char_p
        L.tb_destroy.restype = None
        L.tb_extractor_destroy.restype = None
        L.tb_three_maxima.restype = None
        L.tb_vocab_destroy.restype = None
        L.tb_vocab_destroy.argtypes = [C.c_void_p]
        L.tb_last_error.argtypes = [C.c_void_p]
        L.tb_destroy.argtypes = [C.c_void_p]
        L.tb_extractor_destroy.argtypes = [C.c_void_p]
        L.tb_vo_destroy.restype = None
        L.tb_vo_destroy.argtypes = [C.c_void_p]
        L.tb_bow_db_destroy.restype = None
        L.tb_bow_db_destroy.argtypes = [C.c_void_p]
        L.tb_kf_store_destroy.restype = None
        L.tb_kf_store_destroy.argtypes = [C.c_void_p]
        L.tb_lsh_destroy.restype = None
        L.tb_lsh_destroy.argtypes = [C.c_void_p]
        if hasattr(L, "tb_depth_filter_destroy"):   # TB_HIP_LIB may name an older library (A/B runs)
            L.tb_depth_filter_destroy.restype = None
            L.tb_depth_filter_destroy.argtypes = [C.c_void_p]
        _LIB = L
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _u8img(img):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    assert img.ndim == 2
    return img


def scale_factors(n, scale):
    sf = np.zeros(n, np.float32); isf = np.zeros(n, np.float32)
    s2 = np.zeros(n, np.float32); is2 = np.zeros(n, np.float32)
    rc = lib().tb_scale_factors(n, C.c_float(scale), _p(sf), _p(isf), _p(s2), _p(is2))
    if rc:
        raise TBError(rc, "tb_scale_factors")
    return sf, isf, s2, is2


def pyramid_sizes(w, h, sf):
    sf = np.ascontiguousarray(sf, np.float32)
    ws = np.zeros(len(sf), np.int32); hs = np.zeros(len(sf), np.int32)
    rc = lib().tb_pyramid_sizes(int(w), int(h), len(sf), _p(sf), _p(ws), _p(hs))
    if rc:
        raise TBError(rc, "tb_pyramid_sizes")
    return ws, hs


def orb_quotas(sf, target):
    sf = np.ascontiguousarray(sf, np.float32)
    q = np.zeros(len(sf), np.int32)
    rc = lib().tb_orb_quotas(len(sf), _p(sf), int(target), _p(q))
    if rc:
        raise TBError(rc, "tb_orb_quotas")
    return q


def descriptor_distance(a, b):
    a = np.ascontiguousarray(a, np.uint8); b = np.ascontiguousarray(b, np.uint8)
    return int(lib().tb_descriptor_distance(_p(a), _p(b)))


def three_maxima(sizes):
    sizes = np.ascontiguousarray(sizes, np.int32)
    i1, i2, i3 = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    lib().tb_three_maxima(_p(sizes), len(sizes), C.byref(i1), C.byref(i2), C.byref(i3))
    return i1.value, i2.value, i3.value


def ba_obs_stream_positions(pt_start):
    """tb_ba_obs_stream_positions: where the local BA's observation stream keeps every observation (pt_start: CSR by point)"""
    pt_start = np.ascontiguousarray(pt_start, np.int32)
    pos = np.full(int(pt_start[-1]), -1, np.int32)
    rc = lib().tb_ba_obs_stream_positions(_p(pt_start), len(pt_start) - 1, _p(pos))
    if rc:
        raise TBError(rc, "tb_ba_obs_stream_positions")
    return pos


class BatchParams(C.Structure):
    """tb_batch_params of include/tb_capi.h"""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("nlevels", C.c_int), ("scale", C.c_float), ("target", C.c_int),
                ("init_th", C.c_float), ("min_th", C.c_float), ("bf_ratio", C.c_float), ("bf_min_th", C.c_float)]


def batch_run(contexts, left, right, nlevels=8, scale=0.8, target=2000, init_th=80.0, min_th=30.0, bf_ratio=10.0,
              bf_min_th=30.0, cap=None):
    """tb_batch_run: a batch of stereo frames (uint8 [F, H, W] each side) sharded over `contexts` (one per GPU, or several on
    one), pyramid -> ORB (both sides) -> searchByBF left <-> right per shard, records gathered on the host.
    Returns per frame (kps_left, desc_left, kps_right, desc_right, matches)."""
    left = np.ascontiguousarray(left, np.uint8); right = np.ascontiguousarray(right, np.uint8)
    F, H, W = left.shape
    assert right.shape == left.shape and len(contexts) >= 1
    cap = int(cap or (target + 512))
    prm = BatchParams(W, H, int(nlevels), float(scale), int(target), float(init_th), float(min_th), float(bf_ratio), float(bf_min_th))
    kps = np.zeros((2, F, cap), KEYPOINT); desc = np.zeros((2, F, cap, 32), np.uint8); cnt = np.zeros((2, F), np.int32)
    mt = np.zeros((F, cap), MATCH); mc = np.zeros(F, np.int32)
    hs = (C.c_void_p * len(contexts))(*[c._h for c in contexts])
    rc = lib().tb_batch_run(hs, len(contexts), C.byref(prm), F, _p(left), _p(right), W, C.c_size_t(W * H), cap, _p(kps), _p(desc),
                            _p(cnt), _p(mt), _p(mc))
    if rc != 0:
        msgs = [lib().tb_last_error(c._h).decode() for c in contexts]
        raise TBError(rc, "; ".join(m for m in msgs if m) or lib().tb_strerror(rc).decode())
    return [(kps[0, f, :cnt[0, f]].copy(), desc[0, f, :cnt[0, f]].copy(), kps[1, f, :cnt[1, f]].copy(), desc[1, f, :cnt[1, f]].copy(),
             mt[f, :mc[f]].copy()) for f in range(F)]


class VOParams(C.Structure):
    """tb_vo_params of include/tb_capi.h"""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("nlevels", C.c_int), ("scale", C.c_float), ("target", C.c_int),
                ("init_th", C.c_float), ("min_th", C.c_float), ("K", C.c_double * 4), ("bf", C.c_float), ("keyframe_every", C.c_int)]


TB_VO_OPFLOW, TB_VO_BF, TB_VO_VIOLENCE, TB_VO_PROJECTION, TB_VO_PROJECTION_MAP = 0, 1, 2, 3, 4
TB_VO_BOW = 5
TB_VO_NN = 6


class VOTracker(C.Structure):
    """tb_vo_tracker of include/tb_capi.h"""
    _fields_ = [("kind", C.c_int), ("bf_ratio", C.c_float), ("bf_min_th", C.c_float), ("min_level", C.c_int), ("max_level", C.c_int),
                ("radius", C.c_float), ("th_low", C.c_int), ("nratio", C.c_float), ("histo_len", C.c_int),
                ("check_orientation", C.c_int), ("th_high", C.c_int), ("radio", C.c_float), ("map_keyframes", C.c_int)]


class VOBow(C.Structure):
    """tb_vo_bow of include/tb_capi.h"""
    _fields_ = [("levelsup", C.c_int), ("map_point_only", C.c_int), ("th_low", C.c_int), ("nratio", C.c_float), ("histo_len", C.c_int),
                ("check_orientation", C.c_int)]


class VOLsh(C.Structure):
    """tb_vo_lsh of include/tb_capi.h"""
    _fields_ = [("ratio", C.c_float), ("min_th", C.c_float), ("min_level", C.c_int), ("max_level", C.c_int), ("tables", C.c_int),
                ("key_size", C.c_int), ("multi_probe_level", C.c_int), ("seed", C.c_uint64), ("bits", C.c_void_p)]


def lsh_draw_bits(tables, key_size, seed):
    """tb_lsh_draw_bits: the [tables, key_size] uint16 bit table of `seed` (no context, no GPU)."""
    out = np.zeros((max(int(tables), 0), max(int(key_size), 0)), np.uint16)
    rc = lib().tb_lsh_draw_bits(int(tables), int(key_size), C.c_uint64(int(seed) & (2 ** 64 - 1)), _p(out))
    if rc != TB_OK:
        raise TBError(rc, lib().tb_strerror(rc).decode())
    return out


def _lsh_bits(bits, tables, key_size):
    """an explicit bit table as the contiguous uint16 [tables, key_size] array the library reads (None stays None)"""
    if bits is None:
        return None
    b = np.asarray(bits)
    if b.shape != (int(tables), int(key_size)) or b.min() < 0 or b.max() > 65535:
        raise ValueError("bits: a [tables, key_size] table of bit indices")
    return np.ascontiguousarray(b, np.uint16)


class VORecover(C.Structure):
    """tb_vo_recover of include/tb_capi.h"""
    _fields_ = [("lost_inliers", C.c_int), ("topk", C.c_int), ("exclude_newest", C.c_int), ("min_inliers", C.c_int)]


class VOLoop(C.Structure):
    """tb_vo_loop of include/tb_capi.h"""
    _fields_ = [("topk", C.c_int), ("exclude_newest", C.c_int), ("min_inliers", C.c_int), ("iters", C.c_int), ("w_rot", C.c_double),
                ("w_trans", C.c_double)]


class VOWindowBA(C.Structure):
    """tb_vo_window_ba of include/tb_capi.h"""
    _fields_ = [("iters", C.c_int), ("fixed", C.c_int), ("min_obs", C.c_int), ("min_points", C.c_int)]


class VOMono(C.Structure):
    """tb_vo_mono of include/tb_capi.h"""
    _fields_ = [("cos_parallax_max", C.c_double), ("chi2_max", C.c_double), ("cell", C.c_int)]


class TriangulateParams(C.Structure):
    """tb_triangulate_params of include/tb_capi.h"""
    _fields_ = [("cos_parallax_max", C.c_double), ("chi2_max", C.c_double)]


class PnpParams(C.Structure):
    """tb_pnp_params of include/tb_capi.h"""
    _fields_ = [("hypotheses", C.c_int), ("chi2_max", C.c_double), ("seed", C.c_uint64)]


class Sim3Params(C.Structure):
    """tb_sim3_params of include/tb_capi.h"""
    _fields_ = [("hypotheses", C.c_int), ("fixed_scale", C.c_int), ("chi2_max", C.c_double), ("seed", C.c_uint64)]


def sim3_params(hypotheses=256, fixed_scale=False, chi2_max=9.210, seed=0):
    """a Sim3Params with the defaults of include/tb_capi.h; fixed_scale is passed through as an int, so that the argument check
    can be tested"""
    return Sim3Params(int(hypotheses), int(fixed_scale), float(chi2_max), int(seed) & 0xFFFFFFFFFFFFFFFF)


class Sim3OptParams(C.Structure):
    """tb_sim3_opt_params of include/tb_capi.h"""
    _fields_ = [("th2", C.c_double), ("iters_first", C.c_int), ("iters_bad", C.c_int), ("iters_clean", C.c_int), ("min_keep", C.c_int),
                ("fixed_scale", C.c_int)]


def sim3_opt_params(th2=10.0, iters_first=5, iters_bad=10, iters_clean=5, min_keep=10, fixed_scale=False):
    """a Sim3OptParams with the defaults of include/tb_capi.h; fixed_scale is passed through as an int, so that the argument check
    can be tested"""
    return Sim3OptParams(float(th2), int(iters_first), int(iters_bad), int(iters_clean), int(min_keep), int(fixed_scale))


class Sim3RefineOut(C.Structure):
    """tb_sim3_refine_out of include/tb_capi.h: device pointers, each nullable"""
    _fields_ = [(n, C.c_void_p) for n in ("cand_srt", "cand_S12", "cand_inliers", "cand_stats", "best_srt", "best_S12", "best_inliers",
                                          "best_stats")]


def sim3_refine_out(S, ncand, device):
    """(Sim3RefineOut, dict of the torch tensors it points to): every output of a Sim(3) refinement of S sequences x ncand candidates"""
    import torch
    f64 = lambda *sh: torch.empty(sh, dtype=torch.float64, device=device)
    t = dict(cand_srt=f64(S, ncand, 8), cand_S12=torch.empty((S, ncand, 4, 4), dtype=torch.float32, device=device),
             cand_inliers=torch.empty((S, ncand), dtype=torch.int32, device=device), cand_stats=f64(S, ncand, 8), best_srt=f64(S, 8),
             best_S12=torch.empty((S, 4, 4), dtype=torch.float32, device=device), best_inliers=torch.empty((S,), dtype=torch.int32, device=device),
             best_stats=f64(S, 8))
    ro = Sim3RefineOut(**{k: (v.data_ptr() if v.numel() else None) for k, v in t.items()})
    return ro, t


class Sim3Out(C.Structure):
    """tb_sim3_out of include/tb_capi.h: device pointers, each nullable"""
    _fields_ = [(n, C.c_void_p) for n in ("cand_rows", "cand_consensus", "cand_flags", "cand_S12", "cand_srt", "best_rank", "best_kf",
                                          "best_S12", "best_srt")]


def sim3_out(S, ncand, device):
    """(Sim3Out, dict of the torch tensors it points to): every output of a Sim(3) query of S sequences x ncand candidates"""
    import torch
    i32 = lambda *sh: torch.empty(sh, dtype=torch.int32, device=device)
    t = dict(cand_rows=i32(S, ncand), cand_consensus=i32(S, ncand), cand_flags=i32(S, ncand),
             cand_S12=torch.empty((S, ncand, 4, 4), dtype=torch.float32, device=device),
             cand_srt=torch.empty((S, ncand, 8), dtype=torch.float64, device=device), best_rank=i32(S), best_kf=i32(S),
             best_S12=torch.empty((S, 4, 4), dtype=torch.float32, device=device), best_srt=torch.empty((S, 8), dtype=torch.float64, device=device))
    so = Sim3Out(**{k: (v.data_ptr() if v.numel() else None) for k, v in t.items()})
    return so, t


class Sim3SearchOut(C.Structure):
    """tb_sim3_search_out of include/tb_capi.h: device pointers, each nullable"""
    _fields_ = [(n, C.c_void_p) for n in ("cand_new", "cand_total", "cand_stats", "best_new", "best_total")]


def sim3_search_out(S, ncand, device, best=True):
    """(Sim3SearchOut, dict of the torch tensors it points to): every output of a SearchBySim3 query of S sequences x ncand
    candidates; best=False leaves out best_new / best_total (the Sim(3) query selected nothing)"""
    import torch
    i32 = lambda *sh: torch.empty(sh, dtype=torch.int32, device=device)
    t = dict(cand_new=i32(S, ncand), cand_total=i32(S, ncand), cand_stats=i32(S, ncand, 8))
    if best:
        t.update(best_new=i32(S), best_total=i32(S))
    so = Sim3SearchOut(**{k: (v.data_ptr() if v.numel() else None) for k, v in t.items()})
    return so, t


class Sim3GraphOut(C.Structure):
    """tb_sim3_graph_out of include/tb_types.h: device pointers into the store's buffers"""
    _fields_ = [("nn", C.c_int)] + [(n, C.c_void_p) for n in ("nnodes", "node_kf", "before", "after", "edges", "edge_counts", "stats")]


def sim3_graph_tensors(go, S, device, copy):
    """what a Sim3GraphOut points to, as torch VIEWS of the store's buffers or (copy) as copies made on the current stream:
    dict(nnodes [S] int32, node_kf [S, nn] int32, before / after [S, nn, 8] float64 srt records, edges [S, nn, 96] uint8
    (PG_SIM3_EDGE records), edge_counts [S], stats [S, 8] float64)"""
    import torch
    nn = go.nn
    spec = dict(nnodes=((S,), "<i4", torch.int32), node_kf=((S, nn), "<i4", torch.int32), before=((S, nn, 8), "<f8", torch.float64),
                after=((S, nn, 8), "<f8", torch.float64), edges=((S, nn, PG_SIM3_EDGE.itemsize), "|u1", torch.uint8),
                edge_counts=((S,), "<i4", torch.int32), stats=((S, 8), "<f8", torch.float64))
    out = {k: torch.as_tensor(_DevView(getattr(go, k), sh, ts), device=device).view(dt) for k, (sh, ts, dt) in spec.items()}
    return {k: v.clone() for k, v in out.items()} if copy else out


class TwoViewParams(C.Structure):
    """tb_two_view_params of include/tb_capi.h"""
    _fields_ = [("hypotheses", C.c_int), ("chi2_epi", C.c_double), ("refit", C.c_int), ("tri", TriangulateParams),
                ("min_good_ratio", C.c_double), ("ambiguity_ratio", C.c_double), ("min_points", C.c_int), ("baseline", C.c_double),
                ("seed", C.c_uint64)]


TB_TWO_VIEW_MAX_PITCH = 4096


class VOMonoInit(C.Structure):
    """tb_vo_mono_init of include/tb_capi.h"""
    _fields_ = [("two_view", TwoViewParams), ("min_tracks", C.c_int)]


def two_view_params(hypotheses=256, chi2_epi=3.841, refit=1, cos_parallax_max=0.9998, chi2_max=5.991, min_good_ratio=0.9,
                    ambiguity_ratio=0.7, min_points=50, baseline=1.0, seed=0):
    """a TwoViewParams with the defaults of include/tb_capi.h"""
    return TwoViewParams(int(hypotheses), float(chi2_epi), int(refit), TriangulateParams(float(cos_parallax_max), float(chi2_max)),
                         float(min_good_ratio), float(ambiguity_ratio), int(min_points), float(baseline), int(seed) & 0xFFFFFFFFFFFFFFFF)


class VO:
    """tb_vo: the device-resident stereo VO loop (test_kitti) for nseq sequences on one context. Device pointers in and out.
    tracker None = tb_vo_create (optical flow) unless use_ex; otherwise tb_vo_create_ex with the VOTracker (or NULL).
    bow (a VOBow) = tb_vo_create_bow with the vocabulary handle `vocab` of the same context, which the loop borrows.
    lsh (a VOLsh) = tb_vo_create_lsh."""

    def __init__(self, ctx, params, nseq, tracker=None, use_ex=False, bow=None, vocab=None, lsh=None):
        self.ctx = ctx
        self.nseq = int(nseq)
        self._h = C.c_void_p()
        if lsh is not None:
            ctx.check(lib().tb_vo_create_lsh(ctx._h, C.byref(params), C.byref(lsh), self.nseq, C.byref(self._h)))
        elif bow is not None:
            ctx.check(lib().tb_vo_create_bow(ctx._h, C.byref(params), C.byref(bow), vocab, self.nseq, C.byref(self._h)))
        elif tracker is None and not use_ex:
            ctx.check(lib().tb_vo_create(ctx._h, C.byref(params), self.nseq, C.byref(self._h)))
        else:
            trp = C.byref(tracker) if tracker is not None else None
            ctx.check(lib().tb_vo_create_ex(ctx._h, C.byref(params), trp, self.nseq, C.byref(self._h)))

    def close(self):
        # the loop owns an extractor plan of its context: destroy it while the context is alive
        if self._h and self.ctx._h:
            lib().tb_vo_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset_dev(self, Tcw0_ptr):
        self.ctx.check(lib().tb_vo_reset_dev(self._h, C.c_void_p(Tcw0_ptr)))

    def step_dev(self, left_ptr, right_ptr, stride, pitch):
        """Returns the status code (0 or a negative TB_E* code) instead of raising, so argument checks can be tested."""
        return lib().tb_vo_step_dev(self._h, C.c_void_p(left_ptr), C.c_void_p(right_ptr or None), int(stride), C.c_size_t(pitch))

    def reset_seq_dev(self, which, Tcw0_ptr):
        """tb_vo_reset_seq_dev: `which` a bool sequence [nseq] (host), Tcw0_ptr a device array [nseq][16]. Returns the status code."""
        w = np.ascontiguousarray(np.asarray(which, bool).astype(np.uint8))
        assert w.shape == (self.nseq,)
        return lib().tb_vo_reset_seq_dev(self._h, _p(w), C.c_void_p(Tcw0_ptr))

    def step_ragged_dev(self, left_ptr, right_ptr, stride, pitch, active=None, force_keyframe=None):
        """tb_vo_step_ragged_dev: active / force_keyframe bool sequences [nseq] (host) or None. Returns the status code."""
        m = [None if x is None else np.ascontiguousarray(np.asarray(x, bool).astype(np.uint8)) for x in (active, force_keyframe)]
        assert all(x is None or x.shape == (self.nseq,) for x in m)
        return lib().tb_vo_step_ragged_dev(self._h, C.c_void_p(left_ptr), C.c_void_p(right_ptr or None), int(stride), C.c_size_t(pitch),
                                           _p(m[0]), _p(m[1]))

    def frames(self):
        """tb_vo_frames: (frames [nseq], kf_frames [nseq]) int32 numpy arrays"""
        f, k = np.zeros(self.nseq, np.int32), np.zeros(self.nseq, np.int32)
        self.ctx.check(lib().tb_vo_frames(self._h, _p(f), _p(k)))
        return f, k

    def state_dev(self):
        """dict of device pointers (Tcw, keys_xy, map_points, mp_valid, key_counts, obs, obs_counts, n_inliers, outlier) + key_pitch,
        frame."""
        ptrs = [C.c_void_p() for _ in range(9)]
        pitch, frame = C.c_int(0), C.c_int(0)
        self.ctx.check(lib().tb_vo_state_dev(self._h, *[C.byref(q) for q in ptrs], C.byref(pitch), C.byref(frame)))
        names = ("Tcw", "keys_xy", "map_points", "mp_valid", "key_counts", "obs", "obs_counts", "n_inliers", "outlier")
        out = {k: q.value for k, q in zip(names, ptrs)}
        out["key_pitch"], out["frame"] = pitch.value, frame.value
        return out

    def tracker_state_dev(self):
        """dict of device pointers of a descriptor tracker (orb, orb_desc, orb_counts, matches, match_counts, flags, kf_orb, kf_desc,
        kf_map_points, kf_mp_valid, kf_counts) + kf_frame."""
        ptrs = [C.c_void_p() for _ in range(11)]
        kf_frame = C.c_int(0)
        self.ctx.check(lib().tb_vo_tracker_state_dev(self._h, *[C.byref(q) for q in ptrs], C.byref(kf_frame)))
        names = ("orb", "orb_desc", "orb_counts", "matches", "match_counts", "flags", "kf_orb", "kf_desc", "kf_map_points",
                 "kf_mp_valid", "kf_counts")
        out = {k: q.value for k, q in zip(names, ptrs)}
        out["kf_frame"] = kf_frame.value
        return out

    def bow_state_dev(self):
        """dict of device pointers of a searchByBow loop's SetBow outputs: fv_keys, fv_counts, bv_words, bv_values, bv_counts,
        word_ids, node_ids of the current frame and kf_* of the keyframe."""
        names = ("fv_keys", "fv_counts", "bv_words", "bv_values", "bv_counts", "word_ids", "node_ids")
        names = names + tuple("kf_" + n for n in names)
        ptrs = [C.c_void_p() for _ in names]
        self.ctx.check(lib().tb_vo_bow_state_dev(self._h, *[C.byref(q) for q in ptrs]))
        return {k: q.value for k, q in zip(names, ptrs)}

    def bow_db_enable(self, capacity):
        """tb_vo_bow_db_enable: returns the status code (0 or a negative TB_E* code), so the state checks can be tested."""
        rc = lib().tb_vo_bow_db_enable(self._h, int(capacity))
        if rc == 0:
            self._db_capacity = int(capacity)
        return rc

    def bow_db(self):
        """tb_vo_bow_db_get: the loop's keyframe database as a borrowed BowDatabase (TB_ESTATE when it is not enabled); its pitch
        is the loop's key pitch."""
        h = C.c_void_p()
        self.ctx.check(lib().tb_vo_bow_db_get(self._h, C.byref(h)))
        return BowDatabase(self.ctx, self.nseq, self._db_capacity, self.state_dev()["key_pitch"], None, handle=h)

    def reloc_enable(self, max_candidates):
        """tb_vo_reloc_enable: returns the status code (0 or a negative TB_E* code), so the state checks can be tested."""
        rc = lib().tb_vo_reloc_enable(self._h, int(max_candidates))
        if rc == 0:
            self._max_candidates = int(max_candidates)
        return rc

    def kf_store(self):
        """tb_vo_kf_store_get: the loop's keyframe store as a borrowed KeyframeStore (TB_ESTATE when it is not enabled)."""
        h = C.c_void_p()
        self.ctx.check(lib().tb_vo_kf_store_get(self._h, C.byref(h)))
        return KeyframeStore(self.ctx, self.nseq, self._db_capacity, self.state_dev()["key_pitch"], self._max_candidates, handle=h)

    def relocalize_dev(self, topk, exclude_newest, min_inliers, capacity, device):
        """tb_vo_relocalize_dev: dict of device tensors -- the query's scores / top_* and tb_reloc_out's fields. Returns
        (status code, dict)."""
        import torch
        S, k = self.nseq, max(int(topk), 0)
        q = dict(scores=torch.empty((S, capacity), dtype=torch.float64, device=device),
                 top_slot=torch.empty((S, k), dtype=torch.int32, device=device), top_kf=torch.empty((S, k), dtype=torch.int32, device=device),
                 top_score=torch.empty((S, k), dtype=torch.float64, device=device), top_count=torch.empty(S, dtype=torch.int32, device=device))
        ro, out = reloc_out(S, k, device)
        p = lambda t: C.c_void_p(t.data_ptr()) if t.numel() else None
        rc = lib().tb_vo_relocalize_dev(self._h, int(topk), int(exclude_newest), int(min_inliers), p(q["scores"]), p(q["top_slot"]),
                                        p(q["top_kf"]), p(q["top_score"]), p(q["top_count"]), C.byref(ro))
        if rc == 0:
            self._reloc_topk = int(topk)      # what relocalize_sim3_dev sizes its outputs by
        q.update(out)
        return rc, q

    def relocalize_sim3_dev(self, device, min_consensus=20, topk=None, **params):
        """tb_vo_relocalize_sim3_dev after relocalize_dev: (status code, dict of device tensors with tb_sim3_out's fields
        [nseq, topk, ...]); params as sim3_params. topk None = the topk of this object's last relocalize_dev (1 when there was
        none: the library then answers TB_ESTATE); the library refuses any other count than the verification's with TB_EINVAL
        before it writes, so outputs sized here are never overrun."""
        topk = getattr(self, "_reloc_topk", None) or 1 if topk is None else int(topk)
        so, out = sim3_out(self.nseq, max(topk, 0), device)
        prm = sim3_params(**params)
        return lib().tb_vo_relocalize_sim3_dev(self._h, int(topk), C.byref(prm), int(min_consensus), C.byref(so)), out

    def refine_sim3_dev(self, device, sim3, min_inliers=20, use_for_graph=False, topk=None, **params):
        """tb_vo_refine_sim3_dev after relocalize_sim3_dev: (status code, dict of device tensors with tb_sim3_refine_out's fields
        [nseq, topk, ...]). sim3: the dict relocalize_sim3_dev returned (its cand_srt and cand_consensus seed the refinement);
        params as sim3_opt_params. topk None = the topk of this object's last relocalize_dev; the library refuses any other count.
        use_for_graph is passed through as an int, so that the argument check can be tested."""
        topk = getattr(self, "_reloc_topk", 1) if topk is None else topk
        ro, out = sim3_refine_out(self.nseq, max(int(topk), 0), device)
        prm = sim3_opt_params(**params)
        p = lambda t: C.c_void_p(t.data_ptr() if t is not None and t.numel() else None)
        srt, cons = (sim3 or {}).get("cand_srt"), (sim3 or {}).get("cand_consensus")
        return lib().tb_vo_refine_sim3_dev(self._h, int(topk), p(srt), p(cons), C.byref(prm), int(min_inliers), int(use_for_graph), C.byref(ro)), out

    def search_sim3_dev(self, device, sim3, th=7.5, th_high=100, use_for_refine=True, topk=None, best=True):
        """tb_vo_search_sim3_dev after relocalize_sim3_dev: (status code, dict of device tensors with tb_sim3_search_out's fields
        [nseq, topk, ...]). sim3: a dict with cand_srt and cand_consensus (relocalize_sim3_dev's, or one with a refined cand_srt);
        topk None = the topk of this object's last relocalize_dev; the library refuses any other count. use_for_refine is passed
        through as an int, so that the argument check can be tested."""
        topk = getattr(self, "_reloc_topk", 1) if topk is None else topk
        so, out = sim3_search_out(self.nseq, max(int(topk), 0), device, best)
        p = lambda t: C.c_void_p(t.data_ptr() if t is not None and t.numel() else None)
        srt, cons = (sim3 or {}).get("cand_srt"), (sim3 or {}).get("cand_consensus")
        return lib().tb_vo_search_sim3_dev(self._h, int(topk), p(srt), p(cons), C.c_float(th), int(th_high), int(use_for_refine), C.byref(so)), out

    def loop_sim3_dev(self, device, iters=10, fixed_scale=True, w_rot=1.0, w_trans=1.0, w_scale=1.0):
        """tb_vo_loop_sim3_dev after relocalize_sim3_dev: (status code, sim3_graph_tensors' dict -- copies made on the current
        stream, which the caller makes the loop's -- or None). fixed_scale is passed through as an int, so that the argument check
        can be tested."""
        go = Sim3GraphOut()
        rc = lib().tb_vo_loop_sim3_dev(self._h, int(iters), int(fixed_scale), C.c_double(w_rot), C.c_double(w_trans), C.c_double(w_scale),
                                       C.byref(go))
        return rc, (sim3_graph_tensors(go, self.nseq, device, True) if rc == 0 else None)

    def reloc_pnp_enable(self, hypotheses=256, chi2_max=5.991, seed=0, min_consensus=10, expand=1):
        """tb_vo_reloc_pnp_enable: returns the status code (0 or a negative TB_E* code), so the state checks can be tested."""
        prm = PnpParams(int(hypotheses), float(chi2_max), int(seed) & 0xFFFFFFFFFFFFFFFF)
        return lib().tb_vo_reloc_pnp_enable(self._h, C.byref(prm), int(min_consensus), int(expand))

    def recover_enable(self, prm):
        """tb_vo_recover_enable with a VORecover (None: a null pointer): returns the status code (0 or a negative TB_E* code), so
        the state and argument checks can be tested."""
        return lib().tb_vo_recover_enable(self._h, C.byref(prm) if prm is not None else None)

    def recover_state_dev(self):
        """tb_vo_recover_state_dev: dict of device pointers (lost, track_inliers, recovered_kf, kf_ids, kf_word_ring,
        kf_node_ring); TB_ESTATE when recovery is not enabled."""
        names = ("lost", "track_inliers", "recovered_kf", "kf_ids", "kf_word_ring", "kf_node_ring")
        ptrs = [C.c_void_p() for _ in names]
        self.ctx.check(lib().tb_vo_recover_state_dev(self._h, *[C.byref(q) for q in ptrs]))
        return {k: q.value for k, q in zip(names, ptrs)}

    def loop_enable(self, prm):
        """tb_vo_loop_enable with a VOLoop (None: a null pointer): returns the status code (0 or a negative TB_E* code), so the
        state and argument checks can be tested."""
        return lib().tb_vo_loop_enable(self._h, C.byref(prm) if prm is not None else None)

    def loop_state_dev(self):
        """tb_vo_loop_state_dev: dict of device pointers (closed, loop_kf, loop_inliers, nnodes, node_kf, before, after, edges,
        edge_counts, stats); TB_ESTATE when loop correction is not enabled."""
        names = ("closed", "loop_kf", "loop_inliers", "nnodes", "node_kf", "before", "after", "edges", "edge_counts", "stats")
        ptrs = [C.c_void_p() for _ in names]
        self.ctx.check(lib().tb_vo_loop_state_dev(self._h, *[C.byref(q) for q in ptrs]))
        return {k: q.value for k, q in zip(names, ptrs)}

    def window_ba_enable(self, prm):
        """tb_vo_window_ba_enable with a VOWindowBA (None: a null pointer): returns the status code (0 or a negative TB_E* code),
        so the state and argument checks can be tested."""
        return lib().tb_vo_window_ba_enable(self._h, C.byref(prm) if prm is not None else None)

    def window_state_dev(self):
        """tb_vo_window_state_dev: dict of device pointers (seg_keys, seg_ok, seg_pose, seg_pts, seg_spawned, obs, obs_counts,
        n_points, stats, adopted, ba_pose, ba_pts) + slot, nslots; TB_ESTATE when the window BA is not enabled."""
        names = ("seg_keys", "seg_ok", "seg_pose", "seg_pts", "seg_spawned", "obs", "obs_counts", "n_points", "stats", "adopted",
                 "ba_pose", "ba_pts")
        ptrs = [C.c_void_p() for _ in names]
        slot, nslots = C.c_int(0), C.c_int(0)
        self.ctx.check(lib().tb_vo_window_state_dev(self._h, *[C.byref(q) for q in ptrs], C.byref(slot), C.byref(nslots)))
        out = {k: q.value for k, q in zip(names, ptrs)}
        out["slot"], out["nslots"] = slot.value, nslots.value
        return out

    def mono_enable(self, prm):
        """tb_vo_mono_enable with a VOMono (None: a null pointer): returns the status code (0 or a negative TB_E* code), so the
        state and argument checks can be tested."""
        return lib().tb_vo_mono_enable(self._h, C.byref(prm) if prm is not None else None)

    def mono_init_enable(self, prm):
        """tb_vo_mono_init_enable with a VOMonoInit (None: a null pointer): returns the status code"""
        return lib().tb_vo_mono_init_enable(self._h, C.byref(prm) if prm is not None else None)

    def mono_init_state_dev(self):
        """tb_vo_mono_init_state_dev: dict of device pointers (initialised, init_frame, attempts, status, consensus, winner, good,
        tri, Tcw1); TB_ESTATE when not enabled."""
        names = ("initialised", "init_frame", "attempts", "status", "consensus", "winner", "good", "tri", "Tcw1")
        ptrs = [C.c_void_p() for _ in names]
        self.ctx.check(lib().tb_vo_mono_init_state_dev(self._h, *[C.byref(q) for q in ptrs]))
        return {k: q.value for k, q in zip(names, ptrs)}

    def mono_state_dev(self):
        """tb_vo_mono_state_dev: dict of device pointers (kf_keys_xy, kf_Tcw, alive, tri_points, tri_flags, tri_tally, survivors,
        added); TB_ESTATE when the mono mode is not enabled."""
        names = ("kf_keys_xy", "kf_Tcw", "alive", "tri_points", "tri_flags", "tri_tally", "survivors", "added")
        ptrs = [C.c_void_p() for _ in names]
        self.ctx.check(lib().tb_vo_mono_state_dev(self._h, *[C.byref(q) for q in ptrs]))
        return {k: q.value for k, q in zip(names, ptrs)}

    def mp_desc_dev(self):
        """dict of device pointers of a projection tracker's map-point descriptors (mp_desc, kf_mp_desc)."""
        a, b = C.c_void_p(), C.c_void_p()
        self.ctx.check(lib().tb_vo_mp_desc_dev(self._h, C.byref(a), C.byref(b)))
        return dict(mp_desc=a.value, kf_mp_desc=b.value)

    def map_state_dev(self):
        """dict of device pointers of the map tracker's map (points, desc, counts, block_counts) + capacity, map_keyframes, blocks."""
        ptrs = [C.c_void_p() for _ in range(4)]
        cap, mk, nb = C.c_int(0), C.c_int(0), C.c_int(0)
        self.ctx.check(lib().tb_vo_map_state_dev(self._h, *[C.byref(q) for q in ptrs], C.byref(cap), C.byref(mk), C.byref(nb)))
        out = {k: q.value for k, q in zip(("points", "desc", "counts", "block_counts"), ptrs)}
        out["capacity"], out["map_keyframes"], out["blocks"] = cap.value, mk.value, nb.value
        return out


class Context:
    """tb_ctx: one GPU + one HIP stream."""

    def __init__(self, device=0, stream=None):
        self._h = C.c_void_p()
        self.device = int(device)
        rc = lib().tb_create(int(device), C.byref(self._h))
        if rc:
            raise TBError(rc, "tb_create(device=%d): %s" % (device, lib().tb_strerror(rc).decode()))
        if stream is not None:
            self.set_stream(stream)

    def close(self):
        if self._h:
            lib().tb_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc):
        if rc:
            raise TBError(rc, lib().tb_last_error(self._h).decode() or lib().tb_strerror(rc).decode())

    def set_stream(self, stream_ptr):
        """Run the context on an existing HIP stream. None = the context's own (non-blocking) stream. Handle 0 -- HIP's
        legacy null stream, which is what torch's DEFAULT stream reports -- is refused: the C ABI reads NULL as "own
        stream", so the caller would believe it is ordered against torch's default stream when it is not. Pass a
        torch.cuda.Stream() handle and issue the torch-side work under `with torch.cuda.stream(...)`."""
        if stream_ptr is None:
            self.check(lib().tb_set_stream(self._h, None))
            return
        if int(stream_ptr) == 0:
            raise ValueError("stream handle 0 (the legacy null stream / torch's default stream) is not accepted: "
                             "create a torch.cuda.Stream() and pass its .cuda_stream, or pass None")
        self.check(lib().tb_set_stream(self._h, C.c_void_p(int(stream_ptr))))

    def synchronize(self):
        self.check(lib().tb_synchronize(self._h))

    def profile_enable(self, on=True, only=None):
        """Per-kernel HIP-event timing on the context's stream; `only`: time just that kernel (None: all)."""
        self.check(lib().tb_profile_only(self._h, only.encode() if only else None))
        self.check(lib().tb_profile_enable(self._h, int(on)))

    def measure_copy_seconds(self, src_ptr, dst_ptr, nbytes, reps=10):
        """Average seconds per device-to-device copy of nbytes with the library's 16-byte-per-lane kernel."""
        sec = C.c_double(0)
        self.check(lib().tb_measure_copy_seconds(self._h, C.c_void_p(src_ptr), C.c_void_p(dst_ptr), C.c_size_t(nbytes), int(reps), C.byref(sec)))
        return sec.value

    def set_concurrency(self, peers):
        """tb_set_concurrency: `peers` contexts share this GPU at the same time (launch-shape hint)."""
        self.check(lib().tb_set_concurrency(self._h, int(peers)))

    def ba_plain_obs(self, on=True):
        """test hook (tb_debug_ba_plain_obs): the local BA's point passes walk the array-of-structs observations"""
        self.check(lib().tb_debug_ba_plain_obs(self._h, int(on)))

    def bf_scalar(self, on=True):
        """test hook (tb_debug_bf_scalar): searchByBF's nearest neighbours by the scalar kernel everywhere (same results)"""
        self.check(lib().tb_debug_bf_scalar(self._h, int(on)))

    def force_dense_fast(self, on=True):
        """Test hook: every FAST block takes the any-density path (same results)."""
        self.check(lib().tb_debug_force_dense_fast(self._h, int(on)))

    def profile_report(self):
        """{kernel name: (calls, total_ms)} accumulated since profile_enable(True)."""
        buf = C.create_string_buffer(8192)
        self.check(lib().tb_profile_report(self._h, buf, len(buf)))
        out = {}
        for line in buf.value.decode().splitlines():
            name, calls, ms = line.split()
            out[name] = (int(calls), float(ms))
        return out

    # ---- single-frame operator forms
    def pyramid(self, img, nlevels, scale):
        img = _u8img(img)
        sf = scale_factors(nlevels, scale)[0]
        ws, hs = pyramid_sizes(img.shape[1], img.shape[0], sf)
        levels = [img] + [np.zeros((int(hs[i]), int(ws[i])), np.uint8) for i in range(1, nlevels)]
        ptrs = (C.c_void_p * nlevels)(*[l.ctypes.data for l in levels])
        st = np.array([l.strides[0] for l in levels], np.int32)
        self.check(lib().tb_pyramid(self._h, _p(img), img.shape[1], img.shape[0], img.strides[0], nlevels, _p(sf), ptrs, _p(st)))
        return levels, sf

    def fast_detect(self, img, th, nms=True):
        img = _u8img(img)
        cap = img.size // (4 if nms else 1) + 4096
        out = np.zeros(cap, CORNER)
        n = C.c_int(0)
        self.check(lib().tb_fast_detect(self._h, _p(img), img.shape[1], img.shape[0], img.strides[0], int(th), int(nms),
                                        _p(out), cap, C.byref(n)))
        return out[:n.value].copy()

    @staticmethod
    def _level_args(levels):
        levels = [_u8img(l) for l in levels]
        n = len(levels)
        ptrs = (C.c_void_p * n)(*[l.ctypes.data for l in levels])
        ws = np.array([l.shape[1] for l in levels], np.int32)
        hs = np.array([l.shape[0] for l in levels], np.int32)
        st = np.array([l.strides[0] for l in levels], np.int32)
        return levels, ptrs, ws, hs, st

    def orb_extract(self, levels, sf, target, init_th, min_th, exit_keys=None, quotas=None):
        levels, ptrs, ws, hs, st = self._level_args(levels)
        sf = np.ascontiguousarray(sf, np.float32)
        cap = int(target) + 64 * len(levels) + 64
        if quotas is not None:
            cap = max(cap, int(np.sum(quotas)) + 64 * len(levels) + 64)
        kps = np.zeros(cap, KEYPOINT)
        desc = np.zeros((cap, 32), np.uint8)
        q = np.zeros(len(levels), np.int32) if quotas is None else np.ascontiguousarray(quotas, np.int32).copy()
        ek = None if exit_keys is None else np.ascontiguousarray(exit_keys, KEYPOINT)
        n = C.c_int(0)
        self.check(lib().tb_orb_extract(self._h, ptrs, _p(ws), _p(hs), _p(st), len(levels), _p(sf), int(target),
                                        C.c_float(init_th), C.c_float(min_th), _p(ek), 0 if ek is None else len(ek),
                                        int(quotas is not None), _p(q), _p(kps), _p(desc), cap, C.byref(n)))
        return kps[:n.value].copy(), desc[:n.value].copy(), q

    def fastgrid_extract(self, levels, inv_sf, target, threshold, occupancy=None):
        levels, ptrs, ws, hs, st = self._level_args(levels)
        inv_sf = np.ascontiguousarray(inv_sf, np.float32)
        cap = int(target) * 2 + 4096
        kps = np.zeros(cap, KEYPOINT)
        occ = None if occupancy is None else np.ascontiguousarray(occupancy, np.uint8)
        n = C.c_int(0)
        self.check(lib().tb_fastgrid_extract(self._h, ptrs, _p(ws), _p(hs), _p(st), len(levels), _p(inv_sf), int(target),
                                             C.c_float(threshold), _p(occ), 0 if occ is None else len(occ), _p(kps), cap,
                                             C.byref(n)))
        return kps[:n.value].copy()

    @staticmethod
    def _desc(d):
        d = np.ascontiguousarray(d, np.uint8)
        if d.size == 0:
            d = d.reshape(0, 32)
        assert d.ndim == 2 and d.shape[1] == 32
        return d

    def bf_match(self, d1, d2, crosscheck=True):
        d1, d2 = self._desc(d1), self._desc(d2)
        out = np.zeros(max(len(d1), 1), MATCH)
        n = C.c_int(0)
        self.check(lib().tb_match_bf(self._h, _p(d1), len(d1), _p(d2), len(d2), int(crosscheck), _p(out), len(out), C.byref(n)))
        return out[:n.value].copy()

    def search_by_bf(self, d1, d2, ratio, min_th):
        d1, d2 = self._desc(d1), self._desc(d2)
        out = np.zeros(max(len(d1), 1), MATCH)
        n = C.c_int(0)
        self.check(lib().tb_search_by_bf(self._h, _p(d1), len(d1), _p(d2), len(d2), C.c_float(ratio), C.c_float(min_th),
                                         _p(out), len(out), C.byref(n)))
        return out[:n.value].copy()

    def lsh(self, tables=20, key_size=10, multi_probe_level=2, seed=0, bits=None):
        """tb_lsh_create: the searchByNN matcher's handle (the reference's LshIndexParams(20, 10, 2) by default)."""
        return Lsh(self, tables, key_size, multi_probe_level, seed, bits)

    def match_lsh(self, lsh, d1, d2):
        """tb_match_lsh: the raw list (FlannBasedMatcher.match)."""
        d1, d2 = self._desc(d1), self._desc(d2)
        out = np.zeros(max(len(d1), 1), MATCH)
        n = C.c_int(0)
        self.check(lib().tb_match_lsh(self._h, lsh._h, _p(d1), len(d1), _p(d2), len(d2), _p(out), len(out), C.byref(n)))
        return out[:n.value].copy()

    def search_by_nn(self, lsh, d1, d2, ratio, min_th, cap=None):
        d1, d2 = self._desc(d1), self._desc(d2)
        out = np.zeros(max(len(d1), 1) if cap is None else max(int(cap), 1), MATCH)
        n = C.c_int(0)
        self.check(lib().tb_search_by_nn(self._h, lsh._h, _p(d1), len(d1), _p(d2), len(d2), C.c_float(ratio), C.c_float(min_th), _p(out),
                                         len(out) if cap is None else int(cap), C.byref(n)))
        return out[:n.value].copy()

    def search_by_nn_batch_dev(self, lsh, npairs, desc1_ptr, counts1_ptr, desc2_ptr, counts2_ptr, set_pitch, ratio, min_th, out_ptr, cap,
                               out_counts_ptr):
        """tb_search_by_nn_batch_dev on device pointers; returns the library's status code."""
        return lib().tb_search_by_nn_batch_dev(self._h, lsh._h, int(npairs), C.c_void_p(desc1_ptr), C.c_void_p(counts1_ptr),
                                               C.c_void_p(desc2_ptr), C.c_void_p(counts2_ptr), C.c_size_t(set_pitch), C.c_float(ratio),
                                               C.c_float(min_th), C.c_void_p(out_ptr), int(cap), C.c_void_p(out_counts_ptr))

    def search_by_violence(self, k1, d1, k2, d2, img2_w, img2_h, min_level=0, max_level=1, radius=10.0, th_low=50,
                           nratio=0.0, histo_len=30, check_orientation=True):
        k1 = np.ascontiguousarray(k1, KEYPOINT); k2 = np.ascontiguousarray(k2, KEYPOINT)
        d1, d2 = self._desc(d1), self._desc(d2)
        out = np.zeros(max(len(k1), 1), MATCH)
        n = C.c_int(0)
        self.check(lib().tb_search_by_violence(self._h, _p(k1), _p(d1), len(k1), _p(k2), _p(d2), len(k2), int(img2_w),
                                               int(img2_h), int(min_level), int(max_level), C.c_float(radius), int(th_low),
                                               C.c_float(nratio), int(histo_len), int(check_orientation), _p(out), len(out),
                                               C.byref(n)))
        return out[:n.value].copy()

    @staticmethod
    def _fv(fv):
        nodes = np.array(sorted(fv), np.uint32)
        start = np.zeros(len(nodes) + 1, np.int32)
        items = []
        for i, nd in enumerate(nodes):
            items.extend(int(x) for x in fv[int(nd)])
            start[i + 1] = len(items)
        return nodes, start, np.array(items, np.uint32)

    def search_by_bow(self, k1, d1, fv1, k2, d2, fv2, has_mp2=None, map_point_only=False, th_low=50, nratio=0.0, histo_len=30,
                      check_orientation=True):
        """Matcher::searchByBow(F1, F2, MapPointOnly) (reference matcher.cpp:619-721); fv1 / fv2: the frames' DBoW2 feature
        vectors as dicts {node id: [feature indices]}."""
        k1 = np.ascontiguousarray(k1, KEYPOINT); k2 = np.ascontiguousarray(k2, KEYPOINT)
        d1, d2 = self._desc(d1), self._desc(d2)
        n1a, s1a, i1a = self._fv(fv1)
        n2a, s2a, i2a = self._fv(fv2)
        hm = None if has_mp2 is None else np.ascontiguousarray(has_mp2, np.uint8)
        out = np.zeros(max(len(i1a), 1), MATCH)
        n = C.c_int(0)
        self.check(lib().tb_search_by_bow(self._h, _p(k1), _p(d1), len(k1), _p(n1a), _p(s1a), _p(i1a), len(n1a), _p(k2), _p(d2), len(k2),
                                          _p(hm), _p(n2a), _p(s2a), _p(i2a), len(n2a), int(map_point_only), int(th_low),
                                          C.c_float(nratio), int(histo_len), int(check_orientation), _p(out), len(out), C.byref(n)))
        return out[:n.value].copy()

    def clahe(self, img, clip_limit=3.0, tiles=(8, 8)):
        """Frame::Equalize (reference Frame.cpp:453-458): cv::createCLAHE(3.0, Size(8, 8))->apply."""
        img = np.ascontiguousarray(img, np.uint8)
        assert img.ndim == 2
        h, w = img.shape
        out = np.zeros_like(img)
        self.check(lib().tb_clahe(self._h, _p(img), w, h, w, C.c_double(clip_limit), int(tiles[0]), int(tiles[1]), _p(out), w))
        return out

    def optical_flow_pyr_lk(self, prev, nxt, prev_pts, win=21, max_level=3):
        """cv::calcOpticalFlowPyrLK as Matcher::searchByOPFlow calls it (reference matcher.cpp:744).
        Returns (next_pts [n,2], status [n] u8, err [n], coarsest level used)."""
        prev = np.ascontiguousarray(prev, np.uint8); nxt = np.ascontiguousarray(nxt, np.uint8)
        assert prev.ndim == 2 and prev.shape == nxt.shape
        h, w = prev.shape
        pts = np.ascontiguousarray(prev_pts, np.float32).reshape(-1, 2)
        n = len(pts)
        out = np.zeros((max(n, 1), 2), np.float32)
        status = np.zeros(max(n, 1), np.uint8)
        err = np.zeros(max(n, 1), np.float32)
        top = C.c_int(0)
        self.check(lib().tb_optical_flow_pyr_lk(self._h, _p(prev), _p(nxt), w, h, w, _p(pts), n, int(win), int(max_level),
                                                _p(out), _p(status), _p(err), C.byref(top)))
        return out[:n], status[:n], err[:n], top.value

    def optical_flow_pyr_lk_dev(self, prev_ptr, next_ptr, width, height, stride, pts_ptr, n, out_ptr, status_ptr, err_ptr=0,
                                win=21, max_level=3):
        """Device-resident form (all arguments are device addresses); asynchronous on the context's stream."""
        self.check(lib().tb_optical_flow_pyr_lk_dev(self._h, C.c_void_p(prev_ptr), C.c_void_p(next_ptr), int(width), int(height),
                                                    int(stride), C.c_void_p(pts_ptr), int(n), int(win), int(max_level),
                                                    C.c_void_p(out_ptr), C.c_void_p(status_ptr), C.c_void_p(err_ptr or None)))

    def optical_flow_pyr_lk_batch_dev(self, npairs, prev_ptr, next_ptr, width, height, stride, image_pitch, pts_ptr, counts_ptr,
                                      pts_pitch, out_ptr, status_ptr, err_ptr=0, win=21, max_level=3):
        """Batched device-resident form: one launch per stage for all pairs; asynchronous on the context's stream."""
        self.check(lib().tb_optical_flow_pyr_lk_batch_dev(
            self._h, int(npairs), C.c_void_p(prev_ptr), C.c_void_p(next_ptr), int(width), int(height), int(stride),
            C.c_size_t(image_pitch), C.c_void_p(pts_ptr), C.c_void_p(counts_ptr or None), int(pts_pitch), int(win), int(max_level),
            C.c_void_p(out_ptr), C.c_void_p(status_ptr), C.c_void_p(err_ptr or None)))

    def search_by_opflow_batch_dev(self, npairs, img1_ptr, img2_ptr, width, height, stride, image_pitch, cam1, keys_ptr, counts_ptr,
                                   pts_pitch, cur_ptr, status_ptr, out_ptr, cap, out_counts_ptr, equalized=False, reject=False):
        """Batched device-resident Matcher::searchByOPFlow (cam1: host CAMERA record); asynchronous on the context's stream."""
        cam1 = np.ascontiguousarray(cam1, CAMERA)
        self.check(lib().tb_search_by_opflow_batch_dev(
            self._h, int(npairs), C.c_void_p(img1_ptr), C.c_void_p(img2_ptr), int(width), int(height), int(stride),
            C.c_size_t(image_pitch), _p(cam1), C.c_void_p(keys_ptr), C.c_void_p(counts_ptr or None), int(pts_pitch), int(equalized),
            int(reject), C.c_void_p(cur_ptr), C.c_void_p(status_ptr), C.c_void_p(out_ptr), int(cap), C.c_void_p(out_counts_ptr)))

    def search_by_opflow(self, img1, img2, cam1, keys2_xy, equalized=False, reject=False):
        """Matcher::searchByOPFlow(F1, F2, cur_points, equalized, reject) (reference matcher.cpp:724-768).
        Returns (cur_points [n,2], DMatch records)."""
        img1 = np.ascontiguousarray(img1, np.uint8); img2 = np.ascontiguousarray(img2, np.uint8)
        assert img1.ndim == 2 and img1.shape == img2.shape
        h, w = img1.shape
        cam1 = np.ascontiguousarray(cam1, CAMERA)
        pts = np.ascontiguousarray(keys2_xy, np.float32).reshape(-1, 2)
        n = len(pts)
        cur = np.zeros((max(n, 1), 2), np.float32)
        out = np.zeros(max(n, 1), MATCH)
        cnt = C.c_int(0)
        self.check(lib().tb_search_by_opflow(self._h, _p(img1), _p(img2), w, h, w, _p(cam1), _p(pts), n, int(equalized),
                                             int(reject), _p(cur), _p(out), len(out), C.byref(cnt)))
        return cur[:n], out[:cnt.value].copy()

    def find_fundamental_ransac(self, pts1, pts2, thresh=1.0, conf=0.99):
        """cv::findFundamentalMat(pts1, pts2, FM_RANSAC, thresh, conf, mask) (reference matcher.cpp:872).
        Returns (ok, mask [n] u8, F [3,3] f64, RANSAC iterations run)."""
        p1 = np.ascontiguousarray(pts1, np.float32).reshape(-1, 2)
        p2 = np.ascontiguousarray(pts2, np.float32).reshape(-1, 2)
        assert len(p1) == len(p2)
        n = len(p1)
        mask = np.zeros(max(n, 1), np.uint8)
        F = np.zeros(9, np.float64)
        it, ok = C.c_int(0), C.c_int(0)
        self.check(lib().tb_find_fundamental_ransac(self._h, _p(p1), _p(p2), n, C.c_double(thresh), C.c_double(conf), _p(mask), _p(F),
                                                    C.byref(it), C.byref(ok)))
        return ok.value, mask[:n], F.reshape(3, 3), it.value

    def reject_with_f(self, cur_pts, last_pts, status):
        """Matcher::rejectWithF(cur_pts, last_pts, status) (reference matcher.cpp:853-881). Returns the updated flags."""
        cur = np.ascontiguousarray(cur_pts, np.float32).reshape(-1, 2)
        last = np.ascontiguousarray(last_pts, np.float32).reshape(-1, 2)
        st = np.ascontiguousarray(status, np.uint8).copy()
        assert len(cur) == len(last) == len(st)
        self.check(lib().tb_reject_with_f(self._h, _p(cur), _p(last), len(st), _p(st)))
        return st

    def vocab_create(self, voc):
        """Upload a synth.Vocabulary (tb_vocabulary arrays); returns an opaque handle for bow_transform / vocab_destroy."""
        h = C.c_void_p()
        self.check(lib().tb_vocab_create(self._h, C.byref(voc.c), C.byref(h)))
        return h

    def vocab_destroy(self, h):
        lib().tb_vocab_destroy(h)

    def vocab_export(self, h):
        """tb_vocab_info + tb_vocab_export: the handle's tree as a synth.Vocabulary (host arrays)."""
        from . import synth
        v = [C.c_int() for _ in range(6)]
        self.check(lib().tb_vocab_info(h, *[C.byref(x) for x in v]))
        nn, _, k, L, weighting, scoring = [x.value for x in v]
        cs = np.zeros(nn + 1, np.int32); ci = np.zeros(max(nn - 1, 1), np.int32); desc = np.zeros((nn, 32), np.uint8)
        wid = np.zeros(nn, np.int32); wt = np.zeros(nn, np.float64)
        self.check(lib().tb_vocab_export(h, _p(cs), _p(ci), _p(desc), _p(wid), _p(wt)))
        return synth.Vocabulary(k, L, cs, ci[:cs[nn]], desc, wid, wt, weighting, scoring)

    def vocab_train(self, docs, k=10, L=5, weighting=0, scoring=0, seed=0, max_iters=200):
        """TemplatedVocabulary::create(training_features, k, L, weighting, scoring) on the device (tb_vocab_train). docs: one
        uint8 [n_i, 32] array per training document. Returns (handle, synth.Vocabulary, stats dict); the handle feeds
        bow_transform / tb_search_by_bow_batch_dev and is freed by vocab_destroy; Vocabulary.to_text writes an ORBvoc-style file."""
        docs = [np.ascontiguousarray(d, np.uint8).reshape(-1, 32) for d in docs]
        counts = np.array([len(d) for d in docs] + [0], np.int32)
        flat = np.concatenate(docs) if docs else np.zeros((0, 32), np.uint8)
        P = VocabTrainParams(int(k), int(L), int(weighting), int(scoring), int(seed) & (2 ** 64 - 1), int(max_iters))
        st = VocabTrainStats()
        h = C.c_void_p()
        self.check(lib().tb_vocab_train(self._h, C.byref(P), len(docs), _p(flat) if len(flat) else None, _p(counts), C.byref(h), C.byref(st)))
        return h, self.vocab_export(h), st.as_dict()

    def vocab_train_dev(self, desc, counts, k=10, L=5, weighting=0, scoring=0, seed=0, max_iters=200):
        """tb_vocab_train_dev on torch tensors of this context's device: desc uint8 [ndocs, pitch, 32] (extractor output as it
        is), counts int32 [ndocs]. Returns (handle, synth.Vocabulary, stats dict)."""
        ndocs, pitch = desc.shape[0], desc.shape[1]
        assert desc.is_contiguous() and desc.shape[2] == 32 and counts.is_contiguous() and counts.numel() == ndocs
        P = VocabTrainParams(int(k), int(L), int(weighting), int(scoring), int(seed) & (2 ** 64 - 1), int(max_iters))
        st = VocabTrainStats()
        h = C.c_void_p()
        self.check(lib().tb_vocab_train_dev(self._h, C.byref(P), ndocs, C.c_void_p(desc.data_ptr()), C.c_void_p(counts.data_ptr()), pitch,
                                            C.byref(h), C.byref(st)))
        return h, self.vocab_export(h), st.as_dict()

    def bow_transform(self, vocab_handle, desc, levelsup=4):
        """Frame::SetBow's voc->transform per feature (reference Frame.cpp:267-270): (word_ids, weights, node_ids)."""
        d = self._desc(desc)
        n = len(d)
        wid = np.zeros(max(n, 1), np.int32); wt = np.zeros(max(n, 1), np.float64); nid = np.zeros(max(n, 1), np.int32)
        self.check(lib().tb_bow_transform(self._h, vocab_handle, _p(d), n, int(levelsup), _p(wid), _p(wt), _p(nid)))
        return wid[:n], wt[:n], nid[:n]

    def bow_vector_batch_dev(self, vocab_handle, word_ids, weights, counts):
        """tb_bow_vector_batch_dev on torch tensors of this context's device: word_ids int32 / weights float64 [F, pitch] as
        tb_bow_transform_batch_dev wrote them, counts int32 [F]. Returns (bv_words int32 [F, pitch], bv_values float64 [F, pitch],
        bv_counts int32 [F]): per frame the BowVector as a list sorted by word id. Asynchronous on the context's stream."""
        import torch
        F, pitch = word_ids.shape
        assert word_ids.dtype == torch.int32 and weights.dtype == torch.float64 and counts.dtype == torch.int32
        assert weights.shape == (F, pitch) and counts.numel() == F and word_ids.is_contiguous() and weights.is_contiguous() and counts.is_contiguous()
        bw = torch.zeros_like(word_ids); bv = torch.zeros_like(weights); bc = torch.zeros_like(counts)
        self.check(lib().tb_bow_vector_batch_dev(self._h, vocab_handle, F, C.c_void_p(word_ids.data_ptr()), C.c_void_p(weights.data_ptr()),
                                                 C.c_void_p(counts.data_ptr()), pitch, C.c_void_p(bw.data_ptr()), C.c_void_p(bv.data_ptr()),
                                                 C.c_void_p(bc.data_ptr())))
        return bw, bv, bc

    def bow_score(self, scoring, a_words, a_values, b_words, b_values):
        """tb_bow_score: TemplatedVocabulary::score(v1 = a, v2 = b) of one pair on the host (ScoringObject.cpp:23-311); the
        vectors are sorted lists (words ascending, values beside them). No device is involved."""
        return bow_score(scoring, a_words, a_values, b_words, b_values)

    def bow_score_batch_dev(self, scoring, a_words, a_values, a_counts, b_words, b_values, b_counts, mode=TB_SCORE_ALL_PAIRS):
        """tb_bow_score_batch_dev on torch tensors of this context's device: words int32 / values float64 [n, pitch] as
        tb_bow_vector_batch_dev writes them, counts int32 [n]; a is v1. Returns float64 [na] (TB_SCORE_PAIRWISE) or [na, nb]
        (TB_SCORE_ALL_PAIRS). Asynchronous on the context's stream."""
        import torch
        na, nb = a_words.shape[0], b_words.shape[0]
        for w, v, c in ((a_words, a_values, a_counts), (b_words, b_values, b_counts)):
            assert w.dtype == torch.int32 and v.dtype == torch.float64 and c.dtype == torch.int32 and v.shape == w.shape
            assert c.numel() == w.shape[0] and w.is_contiguous() and v.is_contiguous() and c.is_contiguous()
        out = torch.empty((na,) if mode == TB_SCORE_PAIRWISE else (na, nb), dtype=torch.float64, device=a_words.device)
        p = lambda t: C.c_void_p(t.data_ptr())
        self.check(lib().tb_bow_score_batch_dev(self._h, int(scoring), int(mode), na, p(a_words), p(a_values), p(a_counts), a_words.shape[1],
                                                nb, p(b_words), p(b_values), p(b_counts), b_words.shape[1], p(out)))
        return out

    def reject_with_f_batch(self, cur, last, status, counts=None):
        """tb_reject_with_f_batch_dev on torch tensors of this context's device: cur / last float32 [P, N, 2], status uint8
        [P, N] (updated in place and returned), counts int32 [P] or None. Asynchronous on the context's stream."""
        P, N = status.shape
        assert cur.shape == (P, N, 2) and last.shape == (P, N, 2) and cur.is_contiguous() and last.is_contiguous() and status.is_contiguous()
        self.check(lib().tb_reject_with_f_batch_dev(self._h, P, C.c_void_p(cur.data_ptr()), C.c_void_p(last.data_ptr()),
                                                    C.c_void_p(counts.data_ptr()) if counts is not None else None, N,
                                                    C.c_void_p(status.data_ptr())))
        self.synchronize()
        return status

    def add_map_points_by_stereo(self, img_stereo, img_current, cam_stereo, keys_xy, bf):
        """LocalBA::AddMapPointsByStereo(current_frame, stereo_frame, bf, fx) (reference LocalBA.cpp:46-68): depth per key."""
        a = np.ascontiguousarray(img_stereo, np.uint8); b = np.ascontiguousarray(img_current, np.uint8)
        assert a.ndim == 2 and a.shape == b.shape
        h, w = a.shape
        cam = np.ascontiguousarray(cam_stereo, CAMERA)
        pts = np.ascontiguousarray(keys_xy, np.float32).reshape(-1, 2)
        n = len(pts)
        depth = np.zeros(max(n, 1), np.float32)
        cnt = C.c_int(0)
        self.check(lib().tb_add_map_points_by_stereo(self._h, _p(a), _p(b), w, h, w, _p(cam), _p(pts), n, C.c_float(bf), _p(depth),
                                                     C.byref(cnt)))
        return depth[:n], cnt.value

    def search_by_projection(self, Tcw1, cam1, img1_w, img1_h, k1, d1, taken1, k2, mp2, mp2_desc, scale_factors, nratio,
                             th_high=100, histo_len=30, check_orientation=True):
        """Matcher::searchByProjection(F1, F2) (reference matcher.cpp:406-531); mp2 / mp2_desc aligned with F2's keys."""
        Tcw1 = np.ascontiguousarray(Tcw1, np.float32).reshape(16)
        cam1 = np.ascontiguousarray(cam1, CAMERA)
        k1 = np.ascontiguousarray(k1, KEYPOINT); k2 = np.ascontiguousarray(k2, KEYPOINT)
        d1, mp2_desc = self._desc(d1), self._desc(mp2_desc)
        taken1 = np.ascontiguousarray(taken1, np.uint8)
        mp2 = np.ascontiguousarray(mp2, MAPPOINT)
        sf = np.ascontiguousarray(scale_factors, np.float32)
        out = np.zeros(max(len(k2), 1), MATCH)
        n = C.c_int(0)
        self.check(lib().tb_search_by_projection(self._h, _p(Tcw1), _p(cam1), int(img1_w), int(img1_h), _p(k1), _p(d1), _p(taken1),
                                                 len(k1), _p(k2), _p(mp2), _p(mp2_desc), len(k2), _p(sf), len(sf),
                                                 C.c_float(nratio), int(th_high), int(histo_len), int(check_orientation),
                                                 _p(out), len(out), C.byref(n)))
        return out[:n.value].copy()

    def search_by_projection_map(self, Tcw1, cam1, img1_w, img1_h, k1, d1, taken1, mps, mp_desc, scale_factors, nratio,
                                 radio, th_high=100):
        """Matcher::searchByProjection(map, F1, radio) (reference matcher.cpp:539-617)."""
        Tcw1 = np.ascontiguousarray(Tcw1, np.float32).reshape(16)
        cam1 = np.ascontiguousarray(cam1, CAMERA)
        k1 = np.ascontiguousarray(k1, KEYPOINT)
        d1, mp_desc = self._desc(d1), self._desc(mp_desc)
        taken1 = np.ascontiguousarray(taken1, np.uint8)
        mps = np.ascontiguousarray(mps, MAPPOINT)
        sf = np.ascontiguousarray(scale_factors, np.float32)
        out = np.zeros(max(len(mps), 1), MATCH)
        n = C.c_int(0)
        self.check(lib().tb_search_by_projection_map(self._h, _p(Tcw1), _p(cam1), int(img1_w), int(img1_h), _p(k1), _p(d1),
                                                     _p(taken1), len(k1), _p(mps), _p(mp_desc), len(mps), _p(sf), len(sf),
                                                     C.c_float(nratio), C.c_float(radio), int(th_high), _p(out), len(out),
                                                     C.byref(n)))
        return out[:n.value].copy()

    def pose_opt(self, K, Tcw, obs, outlier=None):
        K = np.ascontiguousarray(K, np.float64)
        Tcw = np.ascontiguousarray(Tcw, np.float32).reshape(16)
        obs = np.ascontiguousarray(obs, OBS)
        outl = np.zeros(len(obs), np.uint8) if outlier is None else np.ascontiguousarray(outlier, np.uint8).copy()
        out = np.zeros(16, np.float32)
        stats = np.zeros(8, np.float64)
        n = C.c_int(0)
        self.check(lib().tb_pose_opt(self._h, _p(K), _p(Tcw), _p(obs), len(obs), _p(outl), _p(out), C.byref(n), _p(stats)))
        return n.value, out.reshape(4, 4), outl, stats

    def linear_triangle(self, xy0, xy1, Tcw0, Tcw1, K, inv_sigma2_0=None, inv_sigma2_1=None, skip=None, cos_parallax_max=0.9998,
                        chi2_max=5.991):
        """tb_linear_triangle: n point pairs (xy0 / xy1 [n][2] pixels) of one pose pair -> (points [n][3] float32, zero where not
        accepted; flags [n] uint8; tally [6] int32)"""
        xy0 = np.ascontiguousarray(xy0, np.float32).reshape(-1, 2)
        xy1 = np.ascontiguousarray(xy1, np.float32).reshape(-1, 2)
        n = len(xy0)
        assert len(xy1) == n
        opt = [None if a is None else np.ascontiguousarray(a, t).reshape(n) for a, t in
               ((inv_sigma2_0, np.float32), (inv_sigma2_1, np.float32), (skip, np.uint8))]
        K = np.ascontiguousarray(K, np.float64)
        T0 = np.ascontiguousarray(Tcw0, np.float32).reshape(16)
        T1 = np.ascontiguousarray(Tcw1, np.float32).reshape(16)
        prm = TriangulateParams(float(cos_parallax_max), float(chi2_max))
        pts, flags, tally = np.zeros((n, 3), np.float32), np.zeros(n, np.uint8), np.zeros(6, np.int32)
        self.check(lib().tb_linear_triangle(self._h, _p(xy0), _p(xy1), n, _p(T0), _p(T1), _p(K), _p(opt[0]), _p(opt[1]), _p(opt[2]),
                                            C.byref(prm), _p(pts), _p(flags), _p(tally)))
        return pts, flags, tally

    def linear_triangle_batch_dev(self, npairs, xy0_ptr, xy1_ptr, counts_ptr, pitch, Tcw0_ptr, Tcw1_ptr, K, inv_sigma2_0_ptr,
                                  inv_sigma2_1_ptr, skip_ptr, points_ptr, flags_ptr, tally_ptr, cos_parallax_max=0.9998, chi2_max=5.991):
        """tb_linear_triangle_batch_dev: device pointers (0 / None for the nullable ones), asynchronous on the context's stream.
        Returns the status code."""
        K = np.ascontiguousarray(K, np.float64)
        prm = TriangulateParams(float(cos_parallax_max), float(chi2_max))
        v = lambda q: C.c_void_p(q or None)
        return lib().tb_linear_triangle_batch_dev(self._h, int(npairs), v(xy0_ptr), v(xy1_ptr), v(counts_ptr), int(pitch), v(Tcw0_ptr),
                                                  v(Tcw1_ptr), _p(K), v(inv_sigma2_0_ptr), v(inv_sigma2_1_ptr), v(skip_ptr),
                                                  C.byref(prm), v(points_ptr), v(flags_ptr), v(tally_ptr))

    def pnp_ransac(self, K, obs, hypotheses=256, chi2_max=5.991, seed=0, prior=None):
        """tb_pnp_ransac: a pose from the rows of one problem (an OBS array) without a prior, or with `prior` (4 x 4) as hypothesis
        -1. Returns a dict: Tcw [4, 4] float32, consensus, inlier uint8 [n], winner (hypothesis, solution), flags."""
        K = np.ascontiguousarray(K, np.float64)
        obs = np.ascontiguousarray(obs, OBS).reshape(-1)
        pr = None if prior is None else np.ascontiguousarray(prior, np.float32).reshape(16)
        prm = PnpParams(int(hypotheses), float(chi2_max), int(seed) & 0xFFFFFFFFFFFFFFFF)
        T, inl, win = np.zeros(16, np.float32), np.zeros(len(obs), np.uint8), np.zeros(2, np.int32)
        cons, flags = C.c_int(0), C.c_int(0)
        self.check(lib().tb_pnp_ransac(self._h, _p(K), _p(obs) if len(obs) else None, len(obs), C.byref(prm), _p(pr), _p(T), C.byref(cons),
                                       _p(inl) if len(obs) else None, _p(win), C.byref(flags)))
        return dict(Tcw=T.reshape(4, 4), consensus=cons.value, inlier=inl, winner=(int(win[0]), int(win[1])), flags=flags.value)

    def pnp_ransac_dev(self, nproblems, K, obs_ptr, counts_ptr, obs_pitch, prior_ptr=0, Tcw_ptr=0, consensus_ptr=0, inlier_ptr=0,
                       winner_ptr=0, flags_ptr=0, hypotheses=256, chi2_max=5.991, seed=0):
        """tb_pnp_ransac_batch_dev: device pointers (0 / None for the nullable ones), asynchronous on the context's stream.
        Returns the status code."""
        K = np.ascontiguousarray(K, np.float64)
        prm = PnpParams(int(hypotheses), float(chi2_max), int(seed) & 0xFFFFFFFFFFFFFFFF)
        v = lambda q: C.c_void_p(q or None)
        return lib().tb_pnp_ransac_batch_dev(self._h, int(nproblems), _p(K), v(obs_ptr), v(counts_ptr), int(obs_pitch), C.byref(prm),
                                             v(prior_ptr), v(Tcw_ptr), v(consensus_ptr), v(inlier_ptr), v(winner_ptr), v(flags_ptr))

    def sim3_ransac(self, rows, K, hypotheses=256, fixed_scale=False, chi2_max=9.210, seed=0):
        """tb_sim3_ransac: the similarity transform X1 = s R12 X2 + t12 from the 3D-3D rows of one problem: a SIM3_ROW array, or the
        tuple (X1 [n][3], X2 [n][3], inv_sigma2_1 [n], inv_sigma2_2 [n]). Returns a dict: S12 [4, 4] float32, srt [8] float64 (the
        unit quaternion w x y z, t12, s), consensus, inlier uint8 [n], winner (hypothesis, refitted), flags."""
        if isinstance(rows, tuple):
            X1, X2 = (np.asarray(a, np.float32).reshape(-1, 3) for a in rows[:2])
            r = np.zeros(len(X1), SIM3_ROW)
            for k, (f1, f2) in enumerate((("X1", "X2"), ("Y1", "Y2"), ("Z1", "Z2"))):
                r[f1], r[f2] = X1[:, k], X2[:, k]
            r["inv_sigma2_1"], r["inv_sigma2_2"] = rows[2], rows[3]
            rows = r
        K = np.ascontiguousarray(K, np.float64)
        rows = np.ascontiguousarray(rows, SIM3_ROW).reshape(-1)
        prm = sim3_params(hypotheses, fixed_scale, chi2_max, seed)
        S, srt, inl, win = np.zeros(16, np.float32), np.zeros(8, np.float64), np.zeros(len(rows), np.uint8), np.zeros(2, np.int32)
        cons, flags = C.c_int(0), C.c_int(0)
        self.check(lib().tb_sim3_ransac(self._h, _p(K), _p(rows) if len(rows) else None, len(rows), C.byref(prm), _p(S), _p(srt), C.byref(cons),
                                        _p(inl) if len(rows) else None, _p(win), C.byref(flags)))
        return dict(S12=S.reshape(4, 4), srt=srt, consensus=cons.value, inlier=inl, winner=(int(win[0]), int(win[1])), flags=flags.value)

    def sim3_ransac_dev(self, nproblems, K, rows_ptr, counts_ptr, pitch, S12_ptr=0, srt_ptr=0, consensus_ptr=0, inlier_ptr=0, winner_ptr=0,
                        flags_ptr=0, hypotheses=256, fixed_scale=False, chi2_max=9.210, seed=0):
        """tb_sim3_ransac_batch_dev: device pointers (0 / None for the nullable ones), asynchronous on the context's stream.
        Returns the status code."""
        K = np.ascontiguousarray(K, np.float64)
        prm = sim3_params(hypotheses, fixed_scale, chi2_max, seed)
        v = lambda q: C.c_void_p(q or None)
        return lib().tb_sim3_ransac_batch_dev(self._h, int(nproblems), _p(K), v(rows_ptr), v(counts_ptr), int(pitch), C.byref(prm), v(S12_ptr),
                                              v(srt_ptr), v(consensus_ptr), v(inlier_ptr), v(winner_ptr), v(flags_ptr))

    def sim3_optimize(self, rows, K, srt0, active=None, **params):
        """tb_sim3_optimize: the similarity srt0 [8] (the unit quaternion w x y z, t12, s: sim3_ransac's srt) refined on the two-image
        reprojection error of one problem's pixel rows (a SIM3_OBS_ROW array); active: the rows that start active (None: all;
        sim3_ransac's inlier mask is the intended input); params as sim3_opt_params. Returns a dict: srt [8] float64, S12 [4, 4]
        float32, inliers, inlier uint8 [n], stats [8] (iterations, initial and final robust chi2, trials, nBad, dropped rows,
        final lambda, flag)."""
        K = np.ascontiguousarray(K, np.float64)
        rows = np.ascontiguousarray(rows, SIM3_OBS_ROW).reshape(-1)
        n = len(rows)
        srt0 = np.ascontiguousarray(srt0, np.float64).reshape(8)
        act = None if active is None else np.ascontiguousarray(np.asarray(active) != 0, np.uint8).reshape(n)
        prm = sim3_opt_params(**params)
        srt, S, inl, st = np.zeros(8, np.float64), np.zeros(16, np.float32), np.zeros(n, np.uint8), np.zeros(8, np.float64)
        cnt = C.c_int(0)
        self.check(lib().tb_sim3_optimize(self._h, _p(K), _p(rows) if n else None, n, _p(act) if (act is not None and n) else None, _p(srt0),
                                          C.byref(prm), _p(srt), _p(S), C.byref(cnt), _p(inl) if n else None, _p(st)))
        return dict(srt=srt, S12=S.reshape(4, 4), inliers=cnt.value, inlier=inl, stats=st)

    def sim3_optimize_dev(self, nproblems, K, rows_ptr, counts_ptr, pitch, srt_in_ptr, mask_ptr, active_ptr=0, srt_out_ptr=0, S12_ptr=0,
                          inliers_ptr=0, stats_ptr=0, **params):
        """tb_sim3_optimize_batch_dev: device pointers (0 / None for the nullable ones: active, srt_out, S12, inliers, stats),
        asynchronous on the context's stream; params as sim3_opt_params. Returns the status code."""
        K = np.ascontiguousarray(K, np.float64)
        prm = sim3_opt_params(**params)
        v = lambda q: C.c_void_p(q or None)
        return lib().tb_sim3_optimize_batch_dev(self._h, int(nproblems), _p(K), v(rows_ptr), v(counts_ptr), int(pitch), v(active_ptr),
                                                v(srt_in_ptr), C.byref(prm), v(srt_out_ptr), v(S12_ptr), v(inliers_ptr), v(mask_ptr),
                                                v(stats_ptr))

    def search_by_sim3_dev(self, npairs, K, width, height, nlevels, scale, side1, side2, srt_ptr, th=7.5, th_high=100, match1_ptr=0,
                           match2_ptr=0, pairs_ptr=0, cap=0, pair_counts_ptr=0, stats_ptr=0):
        """tb_search_by_sim3_batch_dev: side1 / side2 = (keys_ptr, desc_ptr, points_ptr, valid_ptr, matched_ptr, counts_ptr, pitch),
        device pointers (0 / None for the nullable outputs), asynchronous on the context's stream. Returns the status code."""
        K = np.ascontiguousarray(K, np.float64)
        v = lambda q: C.c_void_p(q or None)
        a = []
        for sd in (side1, side2):
            a += [v(q) for q in sd[:6]] + [int(sd[6])]
        return lib().tb_search_by_sim3_batch_dev(self._h, int(npairs), _p(K), int(width), int(height), int(nlevels), C.c_float(scale), *a,
                                                 v(srt_ptr), C.c_float(th), int(th_high), v(match1_ptr), v(match2_ptr), v(pairs_ptr),
                                                 int(cap), v(pair_counts_ptr), v(stats_ptr))

    def search_by_sim3(self, sides1, sides2, srt, K, width, height, nlevels, scale, th=7.5, th_high=100, cap=None):
        """ORB-SLAM's SearchBySim3 on host arrays, one pair or several in one call. A side is a dict(keys = KEYPOINT records [n], desc
        uint8 [n][32], points float32 [n][3] in the side's own camera frame, valid [n], matched [n] (optional)); sides1 / sides2 are one
        such dict each and srt [8] (w x y z, t, s: X1 = s R X2 + t), or lists of them and srt [P][8]. Returns a dict (or a list of
        dicts): match1 [n1] and match2 [n2] int32, pairs (MATCH records, ascending queryIdx, at most cap of them), pair_count (not
        truncated), stats [8] int32 (tried, searched 1 -> 2; tried, searched 2 -> 1; accepted 1 -> 2, 2 -> 1; new pairs; flag)."""
        import torch
        one = isinstance(sides1, dict)
        if one:
            sides1, sides2 = [sides1], [sides2]
        P = len(sides1)
        srt = np.ascontiguousarray(srt, np.float64).reshape(P, 8)
        dev = torch.device("cuda", self.device)
        packed = []
        for sides in (sides1, sides2):
            pitch = max(1, max(len(s["keys"]) for s in sides))
            keys, desc = np.zeros((P, pitch), KEYPOINT), np.zeros((P, pitch, 32), np.uint8)
            pts, val, mat = np.zeros((P, pitch, 3), np.float32), np.zeros((P, pitch), np.uint8), np.zeros((P, pitch), np.uint8)
            cnt = np.zeros(P, np.int32)
            for p, s in enumerate(sides):
                n = cnt[p] = len(s["keys"])
                keys[p, :n], desc[p, :n] = s["keys"], np.asarray(s["desc"], np.uint8).reshape(n, 32)
                pts[p, :n], val[p, :n] = np.asarray(s["points"], np.float32).reshape(n, 3), np.asarray(s["valid"]).reshape(n) != 0
                if s.get("matched") is not None:
                    mat[p, :n] = np.asarray(s["matched"]).reshape(n) != 0
            t = [torch.from_numpy(a.view(np.uint8) if a.dtype == KEYPOINT else a).to(dev) for a in (keys, desc, pts, val, mat, cnt)]
            packed.append((t, pitch))
        (t1, p1), (t2, p2) = packed
        cap = max(1, min(p1, p2) if cap is None else int(cap))
        i32 = lambda *sh: torch.empty(sh, dtype=torch.int32, device=dev)
        m1, m2, pr, pc, st = i32(P, p1), i32(P, p2), i32(P, cap, 4), i32(P), i32(P, 8)
        dsrt = torch.from_numpy(srt).to(dev)
        torch.cuda.current_stream(dev).synchronize()   # the uploads ran on torch's stream, the call runs on the context's
        self.check(self.search_by_sim3_dev(P, K, width, height, nlevels, scale, tuple(x.data_ptr() for x in t1) + (p1,),
                                           tuple(x.data_ptr() for x in t2) + (p2,), dsrt.data_ptr(), th, th_high, m1.data_ptr(), m2.data_ptr(),
                                           pr.data_ptr(), cap, pc.data_ptr(), st.data_ptr()))
        self.synchronize()
        m1, m2, pr, pc, st = (x.cpu().numpy() for x in (m1, m2, pr, pc, st))
        out = []
        for p in range(P):
            n = min(int(pc[p]), cap)
            out.append(dict(match1=m1[p, :len(sides1[p]["keys"])].copy(), match2=m2[p, :len(sides2[p]["keys"])].copy(),
                            pairs=np.ascontiguousarray(pr[p, :n]).view(MATCH).reshape(n), pair_count=int(pc[p]), stats=st[p].copy()))
        return out[0] if one else out

    def two_view(self, xy0, xy1, K, skip=None, inv_sigma2_0=None, inv_sigma2_1=None, Tcw0=None, **params):
        """tb_two_view: a relative pose and first points from the n point pairs (xy0 / xy1 [n][2] pixels) of one problem; params as
        two_view_params. Returns a dict: status, Tcw1 [4, 4] float32, points [n][3] float32 (zero where nothing was written),
        point_flags / inlier uint8 [n], consensus, winner (hypothesis, candidate), good / tri int32 [4]."""
        xy0 = np.ascontiguousarray(xy0, np.float32).reshape(-1, 2)
        xy1 = np.ascontiguousarray(xy1, np.float32).reshape(-1, 2)
        n = len(xy0)
        assert len(xy1) == n
        opt = [None if a is None else np.ascontiguousarray(a, t).reshape(n) for a, t in
               ((skip, np.uint8), (inv_sigma2_0, np.float32), (inv_sigma2_1, np.float32))]
        K = np.ascontiguousarray(K, np.float64)
        T0 = None if Tcw0 is None else np.ascontiguousarray(Tcw0, np.float32).reshape(16)
        prm = two_view_params(**params)
        T1, pts = np.zeros(16, np.float32), np.zeros((n, 3), np.float32)
        pf, inl = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        win, good, tri = np.zeros(2, np.int32), np.zeros(4, np.int32), np.zeros(4, np.int32)
        cons, status = C.c_int(0), C.c_int(0)
        q = lambda a: _p(a) if n else None
        self.check(lib().tb_two_view(self._h, q(xy0), q(xy1), n, _p(opt[0]), _p(opt[1]), _p(opt[2]), _p(K), _p(T0), C.byref(prm), _p(T1),
                                     q(pts), q(pf), q(inl), C.byref(cons), _p(win), _p(good), _p(tri), C.byref(status)))
        return dict(status=status.value, Tcw1=T1.reshape(4, 4), points=pts, point_flags=pf, inlier=inl, consensus=cons.value,
                    winner=(int(win[0]), int(win[1])), good=good, tri=tri)

    def two_view_dev(self, nproblems, xy0_ptr, xy1_ptr, counts_ptr, pitch, K, skip_ptr=0, inv_sigma2_0_ptr=0, inv_sigma2_1_ptr=0,
                     Tcw0_ptr=0, Tcw1_ptr=0, points_ptr=0, point_flags_ptr=0, inlier_ptr=0, consensus_ptr=0, winner_ptr=0, good_ptr=0,
                     tri_ptr=0, status_ptr=0, params=None, **kw):
        """tb_two_view_batch_dev: device pointers (0 / None for the nullable ones), asynchronous on the context's stream; params a
        TwoViewParams, or two_view_params' keywords. Returns the status code."""
        K = np.ascontiguousarray(K, np.float64)
        prm = two_view_params(**kw) if params is None else params
        v = lambda q: C.c_void_p(q or None)
        return lib().tb_two_view_batch_dev(self._h, int(nproblems), v(xy0_ptr), v(xy1_ptr), v(counts_ptr), int(pitch), v(skip_ptr),
                                           v(inv_sigma2_0_ptr), v(inv_sigma2_1_ptr), _p(K), v(Tcw0_ptr), C.byref(prm), v(Tcw1_ptr),
                                           v(points_ptr), v(point_flags_ptr), v(inlier_ptr), v(consensus_ptr), v(winner_ptr), v(good_ptr),
                                           v(tri_ptr), v(status_ptr))

    def local_ba(self, K, poses, nfixed, pts, obs, iters=10):
        K = np.ascontiguousarray(K, np.float64)
        poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 16).copy()
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3).copy()
        obs = np.ascontiguousarray(obs, BA_OBS)
        stats = np.zeros(8, np.float64)
        self.check(lib().tb_local_ba(self._h, _p(K), len(poses), int(nfixed), _p(poses), len(pts), _p(pts), _p(obs), len(obs),
                                     int(iters), _p(stats)))
        return int(stats[0]), poses.reshape(-1, 4, 4), pts, stats

    def pose_graph(self, poses, nfixed, edges, iters=10):
        """tb_pose_graph: one graph from host arrays. poses [nnodes, 4, 4] float32 Tcw, the first nfixed held; edges a PG_EDGE array
        (pose_graph_edges builds one). Returns (iterations, poses, stats [8]); a malformed graph raises."""
        poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 16).copy()
        edges = np.ascontiguousarray(edges, PG_EDGE).reshape(-1)
        stats = np.zeros(8, np.float64)
        self.check(lib().tb_pose_graph(self._h, len(poses), int(nfixed), _p(poses), _p(edges) if len(edges) else None, len(edges),
                                       int(iters), _p(stats)))
        return int(stats[0]), poses.reshape(-1, 4, 4), stats

    def pose_graph_plan(self, ngraphs, nnodes, nfixed, edge_pitch):
        """tb_pose_graph_plan: size the work buffer for this shape ahead of time. Returns the status code."""
        return lib().tb_pose_graph_plan(self._h, int(ngraphs), int(nnodes), int(nfixed), int(edge_pitch))

    def pose_graph_dev(self, ngraphs, nnodes, nfixed, poses_ptr, edges_ptr, counts_ptr, edge_pitch, iters, stats_ptr=0):
        """tb_pose_graph_batch_dev: device pointers (stats nullable), asynchronous on the context's stream. Returns the status code."""
        return lib().tb_pose_graph_batch_dev(self._h, int(ngraphs), int(nnodes), int(nfixed), C.c_void_p(poses_ptr), C.c_void_p(edges_ptr),
                                             C.c_void_p(counts_ptr), int(edge_pitch), int(iters), C.c_void_p(stats_ptr or None))

    def pose_graph_sim3(self, nodes, nfixed, edges, iters=10, fixed_scale=False):
        """tb_pose_graph_sim3: one graph from host arrays. nodes [nnodes, 8] float64 srt records (the quaternion w x y z, t, s), the
        first nfixed held; edges a PG_SIM3_EDGE array (pose_graph_sim3_edges builds one). Returns (nodes, stats [8]); a malformed
        graph raises."""
        nodes = np.ascontiguousarray(nodes, np.float64).reshape(-1, 8).copy()
        edges = np.ascontiguousarray(edges, PG_SIM3_EDGE).reshape(-1)
        stats = np.zeros(8, np.float64)
        self.check(lib().tb_pose_graph_sim3(self._h, len(nodes), int(nfixed), int(bool(fixed_scale)), _p(nodes),
                                            _p(edges) if len(edges) else None, len(edges), int(iters), _p(stats)))
        return nodes, stats

    def pose_graph_sim3_plan(self, ngraphs, nnodes, nfixed, edge_pitch):
        """tb_pose_graph_sim3_plan: size the work buffer for this shape ahead of time. Returns the status code."""
        return lib().tb_pose_graph_sim3_plan(self._h, int(ngraphs), int(nnodes), int(nfixed), int(edge_pitch))

    def pose_graph_sim3_dev(self, ngraphs, nnodes, nfixed, nodes_ptr, edges_ptr, counts_ptr, edge_pitch, iters, stats_ptr=0, fixed_scale=False):
        """tb_pose_graph_sim3_batch_dev: device pointers (stats nullable), asynchronous on the context's stream. fixed_scale: a bool, or
        an int handed through as it is. Returns the status code."""
        return lib().tb_pose_graph_sim3_batch_dev(self._h, int(ngraphs), int(nnodes), int(nfixed), int(fixed_scale), C.c_void_p(nodes_ptr),
                                                  C.c_void_p(edges_ptr), C.c_void_p(counts_ptr), int(edge_pitch), int(iters),
                                                  C.c_void_p(stats_ptr or None))


def pose_graph_edges(pairs, Z, w_rot=1.0, w_trans=1.0):
    """PG_EDGE records of the edges (a, b) in `pairs` with the measured motions Z [n, 4, 4] ~ T_b T_a^-1 (float64 rotation matrices,
    turned into unit quaternions in float64 by the library's own rule) and the weights (scalars or [n])"""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    Z = np.asarray(Z, np.float64).reshape(-1, 4, 4)
    assert len(Z) == len(pairs)
    e = np.zeros(len(pairs), PG_EDGE)
    e["a"], e["b"] = pairs[:, 0], pairs[:, 1]
    e["w_rot"], e["w_trans"] = w_rot, w_trans
    for i, T in enumerate(Z):
        e["q"][i] = _quat_xyzw_from_R(T[:3, :3])
        e["t"][i] = T[:3, 3]
    return e


def _quat_xyzw_from_R(R):
    """the library's own extraction (po_quat_from_R of csrc/tb_se3.h, Eigen's Quaternion(Matrix3)): trace > 0, else the largest
    diagonal entry, ties to the lower index; then w >= 0 and unit norm, as the kernels normalise what they read"""
    q = np.zeros(4)
    t = R[0, 0] + R[1, 1] + R[2, 2]
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t
    else:
        k = 0
        if R[1, 1] > R[0, 0]:
            k = 1
        if R[2, 2] > R[k, k]:
            k = 2
        j, l = (k + 1) % 3, (k + 2) % 3
        t = np.sqrt(R[k, k] - R[j, j] - R[l, l] + 1.0)
        q[k] = 0.5 * t
        t = 0.5 / t
        q[3] = (R[l, j] - R[j, l]) * t
        q[j] = (R[j, k] + R[k, j]) * t
        q[l] = (R[l, k] + R[k, l]) * t
    if q[3] < 0:
        q = -q
    return q / np.sqrt((q * q).sum())


def sim3_from_matrix(S):
    """[n, 4, 4] (or [4, 4]) float64 matrices [[s R, t], [0, 1]] -> srt records [n, 8] (or [8]): the unit quaternion w x y z by the
    kernels' rule (w >= 0), t, s = det(s R)^(1/3)"""
    S = np.asarray(S, np.float64)
    M = S.reshape(-1, 4, 4)
    out = np.zeros((len(M), 8))
    for i, A in enumerate(M):
        s = np.cbrt(np.linalg.det(A[:3, :3]))
        q = _quat_xyzw_from_R(A[:3, :3] / s)
        out[i] = (q[3], q[0], q[1], q[2], A[0, 3], A[1, 3], A[2, 3], s)
    return out.reshape(S.shape[:-2] + (8,))


def sim3_to_matrix(srt):
    """srt records [n, 8] (or [8]) -> float64 matrices [[s R, t], [0, 1]], the quaternion normalised as the kernels normalise it"""
    srt = np.asarray(srt, np.float64)
    V = srt.reshape(-1, 8)
    out = np.zeros((len(V), 4, 4))
    for i, v in enumerate(V):
        w, x, y, z = v[:4] / np.sqrt((v[:4] ** 2).sum()) * (-1.0 if v[0] < 0 else 1.0)
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        out[i, :3, :3], out[i, :3, 3], out[i, 3, 3] = v[7] * R, v[4:7], 1.0
    return out.reshape(srt.shape[:-1] + (4, 4))


def pose_graph_sim3_edges(pairs, Z, w_rot=1.0, w_trans=1.0, w_scale=1.0):
    """PG_SIM3_EDGE records of the edges (a, b) in `pairs` with the measured similarities Z ~ S_b S_a^-1, given as srt records
    [n, 8] (copied as they are: a solver's best_srt stays byte for byte) or as matrices [n, 4, 4] [[s R, t], [0, 1]]
    (sim3_from_matrix), and the weights (scalars or [n])"""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    Z = np.asarray(Z, np.float64)
    Z = Z.reshape(-1, 8) if Z.shape[-1] == 8 else sim3_from_matrix(Z.reshape(-1, 4, 4))
    assert len(Z) == len(pairs)
    e = np.zeros(len(pairs), PG_SIM3_EDGE)
    e["a"], e["b"] = pairs[:, 0], pairs[:, 1]
    e["w_rot"], e["w_trans"], e["w_scale"] = w_rot, w_trans, w_scale
    e["srt"] = Z
    return e


def bow_score(scoring, a_words, a_values, b_words, b_values):
    """tb_bow_score (host, no context): the score of v1 = a against v2 = b under the scoring code of tb_vocabulary."""
    aw = np.ascontiguousarray(a_words, np.int32); av = np.ascontiguousarray(a_values, np.float64)
    bw = np.ascontiguousarray(b_words, np.int32); bv = np.ascontiguousarray(b_values, np.float64)
    assert aw.ndim == 1 and av.shape == aw.shape and bw.ndim == 1 and bv.shape == bw.shape
    out = C.c_double(0.0)
    rc = lib().tb_bow_score(int(scoring), _p(aw) if len(aw) else None, _p(av) if len(aw) else None, len(aw),
                            _p(bw) if len(bw) else None, _p(bv) if len(bw) else None, len(bw), C.byref(out))
    if rc:
        raise TBError(rc, "tb_bow_score: %s" % lib().tb_strerror(rc).decode())
    return out.value


class Lsh:
    """tb_lsh: the parameters and the bit table of the searchByNN matcher on one context."""

    def __init__(self, ctx, tables=20, key_size=10, multi_probe_level=2, seed=0, bits=None):
        self.ctx = ctx
        self._h = C.c_void_p()
        b = _lsh_bits(bits, tables, key_size)
        ctx.check(lib().tb_lsh_create(ctx._h, int(tables), int(key_size), int(multi_probe_level), C.c_uint64(int(seed) & (2 ** 64 - 1)),
                                      _p(b), C.byref(self._h)))

    def close(self):
        if self._h:
            lib().tb_lsh_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        """(tables, key_size, multi_probe_level, bits [tables, key_size] uint16)"""
        T, k, L = C.c_int(0), C.c_int(0), C.c_int(0)
        self.ctx.check(lib().tb_lsh_info(self._h, C.byref(T), C.byref(k), C.byref(L), None))
        bits = np.zeros((T.value, k.value), np.uint16)
        self.ctx.check(lib().tb_lsh_info(self._h, None, None, None, _p(bits)))
        return T.value, k.value, L.value, bits


class BowDatabase:
    """tb_bow_db: per sequence a device-resident ring of the last `capacity` keyframes' BowVectors (include/tb_capi.h). Tensors
    are torch tensors of the context's device; add, query and clear are asynchronous on the context's stream. handle=: wrap a
    database that belongs to someone else (tb_vo_bow_db_get); it is not destroyed here."""

    def __init__(self, ctx, nseq=None, capacity=None, pitch=None, scoring=None, handle=None):
        self.ctx = ctx
        self._own = handle is None
        self.nseq, self.capacity, self.pitch, self.scoring = int(nseq), int(capacity), int(pitch), scoring
        if handle is None:
            self._h = C.c_void_p()
            ctx.check(lib().tb_bow_db_create(ctx._h, self.nseq, self.capacity, self.pitch, self.scoring, C.byref(self._h)))
        else:
            self._h = handle

    def close(self):
        if self._h and self._own and self.ctx._h:
            lib().tb_bow_db_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clear(self):
        self.ctx.check(lib().tb_bow_db_clear(self._h))

    def add_ptr(self, words_ptr, values_ptr, counts_ptr, src_pitch, kf_id):
        """tb_bow_db_add_dev on device pointers; returns the status code."""
        return lib().tb_bow_db_add_dev(self._h, C.c_void_p(words_ptr), C.c_void_p(values_ptr), C.c_void_p(counts_ptr), int(src_pitch),
                                       int(kf_id))

    def add(self, bv_words, bv_values, bv_counts, kf_id):
        """One add for every sequence: bv_words int32 / bv_values float64 [S, src_pitch], bv_counts int32 [S]."""
        assert bv_words.shape[0] == self.nseq and bv_values.shape == bv_words.shape and bv_counts.numel() == self.nseq
        assert bv_words.is_contiguous() and bv_values.is_contiguous() and bv_counts.is_contiguous()
        self.ctx.check(self.add_ptr(bv_words.data_ptr(), bv_values.data_ptr(), bv_counts.data_ptr(), bv_words.shape[1], kf_id))

    def query_ptr(self, words_ptr, values_ptr, counts_ptr, q_pitch, topk, exclude_newest, device):
        """tb_bow_db_query_dev on device pointers: dict(scores [S, capacity], top_slot / top_kf / top_score [S, topk], top_count [S])."""
        import torch
        S, k = self.nseq, int(topk)
        # every element is written by the query's kernels: no fill that could race with them on another stream
        scores = torch.empty((S, self.capacity), dtype=torch.float64, device=device)
        top_slot = torch.empty((S, max(k, 0)), dtype=torch.int32, device=device); top_kf = torch.empty_like(top_slot)
        top_score = torch.empty((S, max(k, 0)), dtype=torch.float64, device=device)
        top_count = torch.empty(S, dtype=torch.int32, device=device)
        p = lambda t: C.c_void_p(t.data_ptr()) if t.numel() else None
        self.ctx.check(lib().tb_bow_db_query_dev(self._h, C.c_void_p(words_ptr), C.c_void_p(values_ptr), C.c_void_p(counts_ptr), int(q_pitch),
                                                 int(exclude_newest), k, p(scores), p(top_slot), p(top_kf), p(top_score), p(top_count)))
        return dict(scores=scores, top_slot=top_slot, top_kf=top_kf, top_score=top_score, top_count=top_count)

    def query(self, q_words, q_values, q_counts, topk=4, exclude_newest=0):
        """Sequence s's query vector (v1) against its own ring: q_words int32 / q_values float64 [S, q_pitch], q_counts int32 [S]."""
        assert q_words.shape[0] == self.nseq and q_values.shape == q_words.shape and q_counts.numel() == self.nseq
        assert q_words.is_contiguous() and q_values.is_contiguous() and q_counts.is_contiguous()
        return self.query_ptr(q_words.data_ptr(), q_values.data_ptr(), q_counts.data_ptr(), q_words.shape[1], topk, exclude_newest,
                              q_words.device)

    def state_dev(self):
        """dict of device pointers (words, values, counts, kf_ids) + nadded."""
        ptrs = [C.c_void_p() for _ in range(4)]
        n = C.c_int(0)
        self.ctx.check(lib().tb_bow_db_state_dev(self._h, *[C.byref(q) for q in ptrs], C.byref(n)))
        out = {k: q.value for k, q in zip(("words", "values", "counts", "kf_ids"), ptrs)}
        out["nadded"] = n.value
        return out

    def state(self, device):
        """Copies of the rings as torch tensors (made on the current stream, so synchronise the context first): dict(words int32 /
        values float64 [S, capacity, pitch], counts / kf_ids int32 [S, capacity] with -1 = empty, nadded)."""
        import torch
        d = self.state_dev()
        S, N, P = self.nseq, self.capacity, self.pitch
        spec = dict(words=((S, N, P), "<i4", torch.int32), values=((S, N, P), "<f8", torch.float64), counts=((S, N), "<i4", torch.int32),
                    kf_ids=((S, N), "<i4", torch.int32))
        out = {k: torch.as_tensor(_DevView(d[k], sh, ts), device=device).view(dt).clone() for k, (sh, ts, dt) in spec.items()}
        out["nadded"] = d["nadded"]
        return out


class DepthFilterParams(C.Structure):
    """tb_depth_filter_params of include/tb_capi.h"""
    _fields_ = [("depth_mean", C.c_double), ("depth_min", C.c_double), ("conv_div", C.c_double), ("px_noise", C.c_double),
                ("max_steps", C.c_int), ("zmssd_max", C.c_int), ("align_iters", C.c_int), ("reserved", C.c_int)]


def depth_filter_params(depth_mean=15.0, depth_min=2.0, conv_div=200.0, px_noise=1.0, max_steps=1000, zmssd_max=2000, align_iters=10):
    return DepthFilterParams(float(depth_mean), float(depth_min), float(conv_div), float(px_noise), int(max_steps), int(zmssd_max),
                             int(align_iters), 0)


class DepthFilter:
    """tb_depth_filter (include/tb_capi.h) on device pointers: per sequence `pitch` seeds and a ring of ref_slots reference images.
    Every call is asynchronous on the context's stream; the methods return the library's status code. Masks are host bool [S]."""

    def __init__(self, ctx, nseq, pitch, ref_slots, width, height, K, params=None):
        self.ctx = ctx
        self.nseq, self.pitch, self.ref_slots, self.width, self.height = int(nseq), int(pitch), int(ref_slots), int(width), int(height)
        self.params = params if params is not None else depth_filter_params()
        self._h = C.c_void_p()
        ctx.check(lib().tb_depth_filter_create(ctx._h, self.nseq, self.pitch, self.ref_slots, self.width, self.height,
                                               (C.c_double * 4)(*[float(k) for k in K]), C.byref(self.params), C.byref(self._h)))

    def close(self):
        if self._h and self.ctx._h:
            lib().tb_depth_filter_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _mask(self, m):
        if m is None:
            return None, None
        a = np.ascontiguousarray(m, np.uint8)
        assert a.shape == (self.nseq,)
        return a, a.ctypes.data_as(C.c_void_p)

    def clear(self, which=None):
        _keep, w = self._mask(which)
        return lib().tb_depth_filter_clear(self._h, w)

    def add_keyframe_dev(self, images_ptr, stride, image_pitch, Tcw_ptr, keys_ptr, counts_ptr, key_pitch, skip_ptr=0, active=None,
                         not_added_ptr=0):
        _keep, a = self._mask(active)
        return lib().tb_depth_filter_add_keyframe_dev(self._h, C.c_void_p(images_ptr), int(stride), C.c_size_t(int(image_pitch)),
                                                      C.c_void_p(Tcw_ptr), C.c_void_p(keys_ptr), C.c_void_p(counts_ptr), int(key_pitch),
                                                      C.c_void_p(skip_ptr or None), a, C.c_void_p(not_added_ptr or None))

    def update_dev(self, images_ptr, stride, image_pitch, Tcw_ptr, active=None):
        _keep, a = self._mask(active)
        return lib().tb_depth_filter_update_dev(self._h, C.c_void_p(images_ptr), int(stride), C.c_size_t(int(image_pitch)),
                                                C.c_void_p(Tcw_ptr), a)

    def points_dev(self, points_ptr, flags_ptr, release=False):
        return lib().tb_depth_filter_points_dev(self._h, C.c_void_p(points_ptr), C.c_void_p(flags_ptr), int(bool(release)))

    def state_dev(self):
        """dict of device pointers (seeds, traces, slot_Tcw) + newest_slot, an int32 array [S] (-1: no keyframe yet)"""
        ptrs = [C.c_void_p() for _ in range(3)]
        newest = np.zeros(self.nseq, np.int32)
        self.ctx.check(lib().tb_depth_filter_state_dev(self._h, *[C.byref(q) for q in ptrs], _p(newest)))
        out = {k: q.value for k, q in zip(("seeds", "traces", "slot_Tcw"), ptrs)}
        out["newest_slot"] = newest
        return out


class _DevView:
    """__cuda_array_interface__ view of a device pointer the library owns (read only: copied out at once)."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(int(ptr), False), version=2, strides=None)


class RelocParams(C.Structure):
    """tb_reloc_params of include/tb_capi.h"""
    _fields_ = [("map_point_only", C.c_int), ("th_low", C.c_int), ("nratio", C.c_float), ("histo_len", C.c_int),
                ("check_orientation", C.c_int), ("min_inliers", C.c_int)]


class RelocOut(C.Structure):
    """tb_reloc_out of include/tb_capi.h: device pointers, each nullable"""
    _fields_ = [(n, C.c_void_p) for n in ("cand_kf", "cand_matches", "cand_rows", "cand_inliers", "cand_flags", "cand_Tcw", "best_rank",
                                          "best_kf", "best_Tcw")]


def reloc_out(S, ncand, device):
    """(RelocOut, dict of the torch tensors it points to): every output of a verification of S sequences x ncand candidates"""
    import torch
    i32 = lambda *sh: torch.empty(sh, dtype=torch.int32, device=device)
    f32 = lambda *sh: torch.empty(sh, dtype=torch.float32, device=device)
    t = dict(cand_kf=i32(S, ncand), cand_matches=i32(S, ncand), cand_rows=i32(S, ncand), cand_inliers=i32(S, ncand), cand_flags=i32(S, ncand),
             cand_Tcw=f32(S, ncand, 4, 4), best_rank=i32(S), best_kf=i32(S), best_Tcw=f32(S, 4, 4))
    ro = RelocOut(**{k: (v.data_ptr() if v.numel() else None) for k, v in t.items()})
    return ro, t


class KeyframeStore:
    """tb_kf_store: per sequence a device-resident ring of the last `capacity` keyframes -- key records, descriptors, FeatureVector
    keys, map points, pose -- ring-aligned with BowDatabase, and the verification of candidates against it (include/tb_capi.h).
    Tensors are torch tensors of the context's device; every call is asynchronous on the context's stream. handle=: wrap a store
    that belongs to someone else (tb_vo_kf_store_get); it is not destroyed here."""

    def __init__(self, ctx, nseq, capacity, pitch, max_candidates, handle=None):
        self.ctx = ctx
        self._own = handle is None
        self.nseq, self.capacity, self.pitch, self.max_candidates = int(nseq), int(capacity), int(pitch), int(max_candidates)
        if handle is None:
            self._h = C.c_void_p()
            ctx.check(lib().tb_kf_store_create(ctx._h, self.nseq, self.capacity, self.pitch, self.max_candidates, C.byref(self._h)))
        else:
            self._h = handle

    def close(self):
        if self._h and self._own and self.ctx._h:
            lib().tb_kf_store_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clear(self):
        self.ctx.check(lib().tb_kf_store_clear(self._h))

    def add_rc(self, keys, desc, counts, fv_keys, fv_counts, map_points, mp_valid, Tcw, kf_id, src_pitch=None):
        """tb_kf_store_add_dev; returns the status code. keys [S, P, 7] int32 records, desc [S, P, 32] uint8, counts [S] int32,
        fv_keys [S, P] int64, fv_counts [S], map_points [S, P, 3] float32, mp_valid [S, P] uint8, Tcw [S, 4, 4] float32."""
        ts = (keys, desc, counts, fv_keys, fv_counts, map_points, mp_valid, Tcw)
        assert all(t.is_contiguous() for t in ts) and keys.shape[0] == self.nseq
        return lib().tb_kf_store_add_dev(self._h, *[C.c_void_p(t.data_ptr()) for t in ts[:7]], int(keys.shape[1] if src_pitch is None else src_pitch),
                                         C.c_void_p(Tcw.data_ptr()), int(kf_id))

    def add(self, *a, **kw):
        self.ctx.check(self.add_rc(*a, **kw))

    def state_dev(self):
        """dict of device pointers (keys, desc, counts, fv_keys, fv_counts, map_points, mp_valid, Tcw, kf_ids) + nadded."""
        names = ("keys", "desc", "counts", "fv_keys", "fv_counts", "map_points", "mp_valid", "Tcw", "kf_ids")
        ptrs = [C.c_void_p() for _ in names]
        n = C.c_int(0)
        self.ctx.check(lib().tb_kf_store_state_dev(self._h, *[C.byref(q) for q in ptrs], C.byref(n)))
        out = {k: q.value for k, q in zip(names, ptrs)}
        out["nadded"] = n.value
        return out

    def state(self, device):
        """Copies of the rings as torch tensors (made on the current stream, so synchronise the context first): dict(keys
        [S, N, P, 7] int32 records, desc [S, N, P, 32] uint8, fv_keys [S, N, P] int64, map_points [S, N, P, 3] float32, mp_valid
        [S, N, P] uint8, counts / fv_counts / kf_ids [S, N] int32 with kf_id -1 = empty, Tcw [S, N, 4, 4] float32, nadded)."""
        import torch
        d = self.state_dev()
        S, N, P = self.nseq, self.capacity, self.pitch
        spec = dict(keys=((S, N, P, 7), "<i4", torch.int32), desc=((S, N, P, 32), "|u1", torch.uint8), fv_keys=((S, N, P), "<i8", torch.int64),
                    map_points=((S, N, P, 3), "<f4", torch.float32), mp_valid=((S, N, P), "|u1", torch.uint8),
                    counts=((S, N), "<i4", torch.int32), fv_counts=((S, N), "<i4", torch.int32), kf_ids=((S, N), "<i4", torch.int32),
                    Tcw=((S, N, 4, 4), "<f4", torch.float32))
        out = {k: torch.as_tensor(_DevView(d[k], sh, ts), device=device).view(dt).clone() for k, (sh, ts, dt) in spec.items()}
        out["nadded"] = d["nadded"]
        return out

    def work(self, device, ncand):
        """tb_kf_store_work_dev: torch VIEWS (not copies) of the last call's work for S x ncand pairs: matches [pairs, P, 4] int32
        (writable: tb_reloc_rows_dev reads them), match_counts [pairs], rows [pairs, P, 6] float32, row_counts [pairs], outlier
        [pairs, P] uint8."""
        import torch
        ptrs = [C.c_void_p() for _ in range(5)]
        pitch = C.c_int(0)
        self.ctx.check(lib().tb_kf_store_work_dev(self._h, *[C.byref(q) for q in ptrs], C.byref(pitch)))
        n, P = self.nseq * int(ncand), pitch.value
        spec = (("matches", (n, P, 4), "<i4", torch.int32), ("match_counts", (n,), "<i4", torch.int32), ("rows", (n, P, 6), "<f4", torch.float32),
                ("row_counts", (n,), "<i4", torch.int32), ("outlier", (n, P), "|u1", torch.uint8))
        return {k: torch.as_tensor(_DevView(q.value, sh, ts), device=device).view(dt) for q, (k, sh, ts, dt) in zip(ptrs, spec)}

    def pnp_enable(self, hypotheses=256, chi2_max=5.991, seed=0, min_consensus=10, expand=1):
        """tb_kf_store_pnp_enable: P3P-RANSAC in front of the pose stage. Returns the status code (0 or a negative TB_E* code), so the
        state and argument checks can be tested."""
        prm = PnpParams(int(hypotheses), float(chi2_max), int(seed) & 0xFFFFFFFFFFFFFFFF)
        return lib().tb_kf_store_pnp_enable(self._h, C.byref(prm), int(min_consensus), int(expand))

    def pnp_state(self, device, ncand):
        """tb_kf_store_pnp_state_dev: torch VIEWS (not copies) of the last call's per-pair PnP outputs for S x ncand pairs: rows
        [pairs, P, 6] float32 (before the gather), row_counts [pairs], consensus [pairs], winner [pairs, 2], Tcw [pairs, 4, 4]
        float32 (the PnP pose), took [pairs] uint8, flags [pairs]."""
        import torch
        ptrs = [C.c_void_p() for _ in range(7)]
        self.ctx.check(lib().tb_kf_store_pnp_state_dev(self._h, *[C.byref(q) for q in ptrs]))
        n, P = self.nseq * int(ncand), self.pitch
        spec = (("rows", (n, P, 6), "<f4", torch.float32), ("row_counts", (n,), "<i4", torch.int32), ("consensus", (n,), "<i4", torch.int32),
                ("winner", (n, 2), "<i4", torch.int32), ("Tcw", (n, 4, 4), "<f4", torch.float32), ("took", (n,), "|u1", torch.uint8),
                ("flags", (n,), "<i4", torch.int32))
        return {k: torch.as_tensor(_DevView(q.value, sh, ts), device=device).view(dt) for q, (k, sh, ts, dt) in zip(ptrs, spec)}

    def sim3_rc(self, K, nlevels, scale, q_keys, q_counts, q_map_points, q_mp_valid, q_Tcw, cand_slot, min_consensus=20, ncand=None,
                q_pitch=None, **params):
        """tb_kf_store_sim3_dev after a relocalize -> (status code, dict of output tensors). q_keys [S, Q, 7] int32 records,
        q_counts [S], q_map_points [S, Q, 3] float32, q_mp_valid [S, Q] uint8, q_Tcw [S, 4, 4] float32, cand_slot [S, ncand] int32
        (what the relocalize took); params as sim3_params."""
        ts = (q_keys, q_counts, q_map_points, q_mp_valid, q_Tcw, cand_slot)
        assert all(t.is_contiguous() for t in ts)
        ncand = int(cand_slot.shape[1] if ncand is None else ncand)
        so, out = sim3_out(self.nseq, max(min(ncand, cand_slot.shape[1]), 0), q_keys.device)
        prm = sim3_params(**params)
        Kd = (C.c_double * 4)(*[float(k) for k in K])
        p = [C.c_void_p(t.data_ptr()) for t in ts]
        rc = lib().tb_kf_store_sim3_dev(self._h, Kd, int(nlevels), C.c_float(scale), p[0], p[1], p[2], p[3],
                                        int(q_keys.shape[1] if q_pitch is None else q_pitch), p[4], p[5], ncand, C.byref(prm), int(min_consensus),
                                        C.byref(so))
        return rc, out

    def sim3(self, *a, **kw):
        rc, out = self.sim3_rc(*a, **kw)
        self.ctx.check(rc)
        return out

    def sim3_refine_rc(self, K, nlevels, scale, q_keys, q_counts, q_map_points, q_mp_valid, q_Tcw, cand_slot, sim3, min_inliers=20,
                       use_for_graph=False, ncand=None, q_pitch=None, **params):
        """tb_kf_store_sim3_refine_dev after a sim3 -> (status code, dict of output tensors with tb_sim3_refine_out's fields). The
        first nine arguments are those the sim3 call took; sim3 is the dict it returned (its cand_srt and cand_consensus seed the
        refinement; None: the store's own buffers); params as sim3_opt_params. use_for_graph is passed through as an int, so that
        the argument check can be tested."""
        ts = (q_keys, q_counts, q_map_points, q_mp_valid, q_Tcw, cand_slot)
        assert all(t.is_contiguous() for t in ts)
        ncand = int(cand_slot.shape[1] if ncand is None else ncand)
        ro, out = sim3_refine_out(self.nseq, max(min(ncand, cand_slot.shape[1]), 0), q_keys.device)
        prm = sim3_opt_params(**params)
        Kd = (C.c_double * 4)(*[float(k) for k in K])
        p = [C.c_void_p(t.data_ptr()) for t in ts]
        v = lambda t: C.c_void_p(t.data_ptr() if t is not None and t.numel() else None)
        srt, cons = (sim3 or {}).get("cand_srt"), (sim3 or {}).get("cand_consensus")
        rc = lib().tb_kf_store_sim3_refine_dev(self._h, Kd, int(nlevels), C.c_float(scale), p[0], p[1], p[2], p[3],
                                               int(q_keys.shape[1] if q_pitch is None else q_pitch), p[4], p[5], ncand, v(srt), v(cons),
                                               C.byref(prm), int(min_inliers), int(use_for_graph), C.byref(ro))
        return rc, out

    def sim3_refine(self, *a, **kw):
        rc, out = self.sim3_refine_rc(*a, **kw)
        self.ctx.check(rc)
        return out

    def sim3_refine_state(self, device, ncand):
        """tb_kf_store_sim3_refine_state_dev: torch VIEWS (not copies) of the last refinement's work for S x ncand pairs: rows
        [pairs, P, 12] float32 (SIM3_OBS_ROW records), row_counts [pairs], active [pairs, P] uint8 (the Sim(3) query's masks, where the
        refinement started; all ones after a sim3_search with use_for_refine), inlier [pairs, P] uint8."""
        import torch
        ptrs = [C.c_void_p() for _ in range(4)]
        self.ctx.check(lib().tb_kf_store_sim3_refine_state_dev(self._h, *[C.byref(q) for q in ptrs]))
        n, P = self.nseq * int(ncand), self.pitch
        spec = (("rows", (n, P, 12), "<f4", torch.float32), ("row_counts", (n,), "<i4", torch.int32), ("active", (n, P), "|u1", torch.uint8),
                ("inlier", (n, P), "|u1", torch.uint8))
        return {k: torch.as_tensor(_DevView(q.value, sh, ts), device=device).view(dt) for q, (k, sh, ts, dt) in zip(ptrs, spec)}

    def sim3_search_rc(self, K, width, height, nlevels, scale, q_keys, q_desc, q_counts, q_map_points, q_mp_valid, q_Tcw, cand_slot, sim3,
                       th=7.5, th_high=100, use_for_refine=True, ncand=None, q_pitch=None, best=True):
        """tb_kf_store_sim3_search_dev after a sim3 -> (status code, dict of output tensors with tb_sim3_search_out's fields): ORB-SLAM's
        SearchBySim3 on every candidate pair. The arguments are those the sim3 call took plus the query's descriptors q_desc [S, Q, 32]
        and the image size; sim3 is the dict it returned (its cand_srt and cand_consensus; a refined cand_srt may stand in; None: the
        store's own buffers). use_for_refine: the next sim3_refine runs on the widened lists; it is passed through as an int, so
        that the argument check can be tested. best=False: no best_* outputs (for a sim3 that selected nothing)."""
        ts = (q_keys, q_desc, q_counts, q_map_points, q_mp_valid, q_Tcw, cand_slot)
        assert all(t.is_contiguous() for t in ts)
        ncand = int(cand_slot.shape[1] if ncand is None else ncand)
        so, out = sim3_search_out(self.nseq, max(min(ncand, cand_slot.shape[1]), 0), q_keys.device, best)
        Kd = (C.c_double * 4)(*[float(k) for k in K])
        p = [C.c_void_p(t.data_ptr()) for t in ts]
        v = lambda t: C.c_void_p(t.data_ptr() if t is not None and t.numel() else None)
        srt, cons = (sim3 or {}).get("cand_srt"), (sim3 or {}).get("cand_consensus")
        rc = lib().tb_kf_store_sim3_search_dev(self._h, Kd, int(width), int(height), int(nlevels), C.c_float(scale), p[0], p[1], p[2], p[3], p[4],
                                               int(q_keys.shape[1] if q_pitch is None else q_pitch), p[5], p[6], ncand, v(srt), v(cons),
                                               C.c_float(th), int(th_high), int(use_for_refine), C.byref(so))
        return rc, out

    def sim3_search(self, *a, **kw):
        rc, out = self.sim3_search_rc(*a, **kw)
        self.ctx.check(rc)
        return out

    def sim3_search_state(self, device, ncand):
        """tb_kf_store_sim3_search_state_dev: torch VIEWS (not copies) of the last search's work for S x ncand pairs: match1 [pairs, Q]
        int32 (Q = that call's query pitch), match2 [pairs, P] int32, pairs [pairs, P, 4] int32 (MATCH records) with pair_counts
        [pairs], widened [pairs, P, 4] int32 with widened_counts [pairs]."""
        import torch
        ptrs = [C.c_void_p() for _ in range(6)]
        qp = C.c_int(0)
        self.ctx.check(lib().tb_kf_store_sim3_search_state_dev(self._h, *[C.byref(q) for q in ptrs], C.byref(qp)))
        n, P, Q = self.nseq * int(ncand), self.pitch, qp.value
        spec = (("match1", (n, Q), "<i4", torch.int32), ("match2", (n, P), "<i4", torch.int32), ("pairs", (n, P, 4), "<i4", torch.int32),
                ("pair_counts", (n,), "<i4", torch.int32), ("widened", (n, P, 4), "<i4", torch.int32), ("widened_counts", (n,), "<i4", torch.int32))
        return {k: torch.as_tensor(_DevView(q.value, sh, ts), device=device).view(dt) for q, (k, sh, ts, dt) in zip(ptrs, spec)}

    def sim3_graph_rc(self, q_Tcw, iters=10, fixed_scale=True, w_rot=1.0, w_trans=1.0, w_scale=1.0):
        """tb_kf_store_sim3_graph_dev after a sim3 -> (status code, dict or None): the Sim(3) pose graph of the live keyframes and the
        query frame q_Tcw [S, 4, 4] float32 with that query's winner as the loop edge, optimised on the device. The dict is
        sim3_graph_tensors': nnodes, node_kf (the frame's node: -2), before, after, edges, edge_counts, stats -- torch VIEWS (not
        copies) of the store's buffers, which the next graph query overwrites; the call is asynchronous on the context's stream,
        so synchronise the context before reading them on another. A query: the store's rings and work do not change.
        fixed_scale is passed through as an int, so that the argument check can be tested."""
        assert q_Tcw is None or q_Tcw.is_contiguous()
        go = Sim3GraphOut()
        rc = lib().tb_kf_store_sim3_graph_dev(self._h, C.c_void_p(q_Tcw.data_ptr() if q_Tcw is not None else None), int(iters), int(fixed_scale),
                                              C.c_double(w_rot), C.c_double(w_trans), C.c_double(w_scale), C.byref(go))
        return rc, (sim3_graph_tensors(go, self.nseq, q_Tcw.device, False) if rc == 0 else None)

    def sim3_graph(self, *a, **kw):
        rc, out = self.sim3_graph_rc(*a, **kw)
        self.ctx.check(rc)
        return out

    def sim3_state(self, device, ncand):
        """tb_kf_store_sim3_state_dev: torch VIEWS (not copies) of the last Sim(3) query's work for S x ncand pairs: rows
        [pairs, P, 8] float32 (SIM3_ROW records), row_counts [pairs], inlier [pairs, P] uint8."""
        import torch
        ptrs = [C.c_void_p() for _ in range(3)]
        self.ctx.check(lib().tb_kf_store_sim3_state_dev(self._h, *[C.byref(q) for q in ptrs]))
        n, P = self.nseq * int(ncand), self.pitch
        spec = (("rows", (n, P, 8), "<f4", torch.float32), ("row_counts", (n,), "<i4", torch.int32), ("inlier", (n, P), "|u1", torch.uint8))
        return {k: torch.as_tensor(_DevView(q.value, sh, ts), device=device).view(dt) for q, (k, sh, ts, dt) in zip(ptrs, spec)}

    def relocalize_rc(self, K, nlevels, scale, q_keys, q_desc, q_counts, q_fv_keys, q_fv_counts, cand_slot, map_point_only=True, th_low=50,
                      nratio=6.0, histo_len=30, check_orientation=True, min_inliers=50, ncand=None, q_pitch=None):
        """tb_relocalize_batch_dev -> (status code, dict of output tensors). q_keys [S, Q, 7] int32 records, q_desc [S, Q, 32],
        q_counts [S], q_fv_keys [S, Q] int64, q_fv_counts [S], cand_slot [S, ncand] int32 (a BowDatabase query's top_slot)."""
        ts = (q_keys, q_desc, q_counts, q_fv_keys, q_fv_counts, cand_slot)
        assert all(t.is_contiguous() for t in ts)
        ncand = int(cand_slot.shape[1] if ncand is None else ncand)
        ro, out = reloc_out(self.nseq, max(min(ncand, cand_slot.shape[1]), 0), q_keys.device)
        prm = RelocParams(int(bool(map_point_only)), int(th_low), float(nratio), int(histo_len), int(bool(check_orientation)), int(min_inliers))
        Kd = (C.c_double * 4)(*[float(k) for k in K])
        p = [C.c_void_p(t.data_ptr()) for t in ts]
        rc = lib().tb_relocalize_batch_dev(self._h, Kd, int(nlevels), C.c_float(scale), p[0], p[1], p[2], p[3], p[4],
                                           int(q_keys.shape[1] if q_pitch is None else q_pitch), p[5], ncand, C.byref(prm), C.byref(ro))
        return rc, out

    def relocalize(self, *a, **kw):
        rc, out = self.relocalize_rc(*a, **kw)
        self.ctx.check(rc)
        return out

    def rows(self, nlevels, scale, q_keys, q_counts, cand_slot, match_counts):
        """tb_reloc_rows_dev: the rows stage alone on the match lists in work()["matches"] with match_counts [S * ncand] int32
        -> cand_rows [S, ncand]; the rows are in work()."""
        import torch
        ts = (q_keys, q_counts, cand_slot, match_counts)
        assert all(t.is_contiguous() for t in ts)
        ncand = int(cand_slot.shape[1])
        rows = torch.empty((self.nseq, ncand), dtype=torch.int32, device=q_keys.device)
        self.ctx.check(lib().tb_reloc_rows_dev(self._h, int(nlevels), C.c_float(scale), C.c_void_p(q_keys.data_ptr()), C.c_void_p(q_counts.data_ptr()),
                                               int(q_keys.shape[1]), C.c_void_p(cand_slot.data_ptr()), ncand, C.c_void_p(match_counts.data_ptr()),
                                               C.c_void_p(rows.data_ptr())))
        return rows


class Extractor:
    """tb_extractor: batched, device-resident pyramid + ORB / FAST-grid extraction plan."""

    def __init__(self, ctx, width, height, nlevels, scale, max_images, max_target):
        self.ctx = ctx
        self.sf, self.inv_sf, self.sigma2, self.inv_sigma2 = scale_factors(nlevels, scale)
        self.width, self.height, self.nlevels = int(width), int(height), int(nlevels)
        self.max_images = int(max_images)
        self.ws, self.hs = pyramid_sizes(width, height, self.sf)
        self._h = C.c_void_p()
        ctx.check(lib().tb_extractor_create(ctx._h, self.width, self.height, self.nlevels, _p(self.sf), None, None,
                                            self.max_images, int(max_target), C.byref(self._h)))
        self._keep = None

    def close(self):
        # tb_destroy() releases every plan of its context; only destroy while the context is alive
        if self._h and self.ctx._h:
            lib().tb_extractor_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_images_host(self, images):
        images = np.ascontiguousarray(images, np.uint8)
        if images.ndim == 2:
            images = images[None]
        assert images.shape[1:] == (self.height, self.width)
        self._keep = images
        self.ctx.check(lib().tb_extractor_set_images_host(self._h, _p(images), images.shape[0], images.strides[1],
                                                          C.c_size_t(images.strides[0])))
        return images.shape[0]

    def set_images_dev(self, dev_ptr, n, stride, pitch):
        self.ctx.check(lib().tb_extractor_set_images_dev(self._h, C.c_void_p(dev_ptr), int(n), int(stride), C.c_size_t(pitch)))

    def build_pyramid(self, n):
        self.ctx.check(lib().tb_extractor_build_pyramid(self._h, int(n)))

    def get_level(self, index, level):
        out = np.zeros((int(self.hs[level]), int(self.ws[level])), np.uint8)
        self.ctx.check(lib().tb_extractor_get_level_host(self._h, int(index), int(level), _p(out), out.strides[0]))
        return out

    def orb(self, n, target, init_th, min_th, quota_mode=0, exit_keys=None):
        ek = None if exit_keys is None else np.ascontiguousarray(exit_keys, KEYPOINT)
        self.ctx.check(lib().tb_extractor_orb(self._h, int(n), int(target), C.c_float(init_th), C.c_float(min_th),
                                              int(quota_mode), _p(ek), 0 if ek is None else len(ek)))

    def fastgrid(self, n, target, threshold, occupancy=None):
        occ = None if occupancy is None else np.ascontiguousarray(occupancy, np.uint8)
        self.ctx.check(lib().tb_extractor_fastgrid(self._h, int(n), _p(self.inv_sf), int(target), C.c_float(threshold),
                                                   _p(occ), 0 if occ is None else len(occ)))

    def counts(self, n):
        c = np.zeros(int(n), np.int32)
        self.ctx.check(lib().tb_extractor_counts_host(self._h, int(n), _p(c)))
        return c

    def results(self, index, cap=None, with_desc=True):
        cap = int(cap or 65536)
        kps = np.zeros(cap, KEYPOINT)
        desc = np.zeros((cap, 32), np.uint8) if with_desc else None
        n = C.c_int(0)
        self.ctx.check(lib().tb_extractor_results_host(self._h, int(index), _p(kps), _p(desc), cap, C.byref(n)))
        return kps[:n.value].copy(), (desc[:n.value].copy() if with_desc else None)

    def results_dev(self):
        kps, desc, counts, cap = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int(0)
        self.ctx.check(lib().tb_extractor_results_dev(self._h, C.byref(kps), C.byref(desc), C.byref(counts), C.byref(cap)))
        return kps.value, desc.value, counts.value, cap.value

    def copy_results_dev(self, n, kps_ptr, desc_ptr, counts_ptr, cap):
        self.ctx.check(lib().tb_extractor_copy_results_dev(self._h, int(n), C.c_void_p(kps_ptr), C.c_void_p(desc_ptr),
                                                           C.c_void_p(counts_ptr), int(cap)))

    def candidates(self, index, level):
        cap = int(self.ws[level]) * int(self.hs[level]) // 4 + 4096
        out = np.zeros(cap, CORNER)
        n = C.c_int(0)
        self.ctx.check(lib().tb_extractor_candidates_host(self._h, int(index), int(level), _p(out), cap, C.byref(n)))
        return out[:n.value].copy()
