/* Internal declarations of libtb_hip.so (not part of the C ABI). */
#ifndef TB_INTERNAL_H
#define TB_INTERNAL_H

#include <cmath>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../include/tb_capi.h"

#define TB_MAX_LEVELS 16
#define TB_BORDER 16          /* EDGE_THRESHOLD - 3, ORBextractor.cpp:749 */
#define TB_NODE_CAP_MAX 2048  /* quadtree list capacity that fits LDS (k_octree.hip) */
#define TB_GRID_CELLS (120 * 36) /* Frame's key lookup grid, FRAME_GRID_COLS x FRAME_GRID_ROWS */
#define TB_GRID_STARTS (TB_GRID_CELLS + 1) /* entries of a grid's cell_start table: cell c holds items [start[c], start[c + 1]) */

/* tb_scratch slots. A slot keeps what a call put there until the next call that takes it, and an entry point that chains
 * others (stereo -> opflow -> LK -> RANSAC, the VO step) must not hand them a slot it still reads. Host forms stage in
 * TB_SLOT_HOST and nothing else does. */
enum {
    TB_SLOT_HOST = 0,           /* host forms: staged inputs and outputs */
    TB_SLOT_BF_TRAIN = 1,       /* tb_search_by_bf_batch_dev: best match per train descriptor */
    TB_SLOT_BF_QUERY = 2,       /* tb_search_by_bf_batch_dev, tb_search_by_nn_batch_dev: best match per query descriptor */
    TB_SLOT_BOW_NODES = 3,      /* tb_bow_transform_batch_dev: node ids */
    TB_SLOT_STEREO_SIGMA = 3,   /*   shared: tb_stereo_tracks_to_obs_batch_dev's sigma table */
    TB_SLOT_BOW_WEIGHTS = 4,    /* tb_bow_transform_batch_dev: weights */
    TB_SLOT_OPFLOW_EQ = 4,      /*   shared: tb_search_by_opflow_batch_dev's equalised images */
    TB_SLOT_WORK = 5,           /* _dev forms: one call's work (matchers' best rows, local BA, CLAHE tables) */
    TB_SLOT_LK = 6,             /* LK pyramids (tbk_lk_work_bytes); tb_pose_opt_batch_dev: residuals */
    TB_SLOT_RANSAC = 7,         /* tbk_ransac_f work */
    TB_SLOT_RANSAC_FLAGS = 8,   /* tbk_ransac_f flags */
    TB_SLOT_STEREO_MATCHES = 9, /* tb_add_map_points_by_stereo_batch_dev: the opflow matches it does not return */
    TB_SLOT_STEREO_COUNTS = 10, /* tb_add_map_points_by_stereo_batch_dev: their counts */
    TB_NSLOTS = 11
};

struct tb_ctx {
    int device = 0;
    int num_cu = 256;   /* compute units of the device (tb_create): launch shapes that aim at one resident round */
    std::vector<std::pair<std::string, hipGraphExec_t>> ba_graphs; /* captured local-BA calls of small batches (k_ba.hip) */
    int peers = 1;      /* tb_set_concurrency: contexts expected to keep this GPU busy at the same time */
    int dbg_fast_dense = 0; /* tb_debug_force_dense_fast: every FAST block takes the any-density path (test hook) */
    int dbg_ba_plain_obs = 0; /* tb_debug_ba_plain_obs: the local-BA point passes walk the array-of-structs observations (test hook) */
    int dbg_bf_scalar = 0; /* tb_debug_bf_scalar: searchByBF's nearest neighbours by the scalar kernel everywhere (test hook) */
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::string err;
    std::map<std::string, tb_extractor*> plans; /* cached single-frame plans */
    std::set<tb_extractor*> live;               /* every plan created on this context */
    /* per-kernel HIP-event timing (tb_profile_*) */
    bool prof = false;
    bool prof_open = false;   /* the last tb_prof_begin recorded its start event */
    std::string prof_only;    /* non-empty: time only this kernel (tb_profile_only) */
    struct ProfRec { const char* name; hipEvent_t a, b; };
    std::vector<ProfRec> prof_recs;
    std::vector<hipEvent_t> prof_pool;
    std::map<std::string, std::pair<long, double>> prof_acc;
    /* grow-only device scratch for the matcher / pose entry points */
    void* scratch[TB_NSLOTS] = {};
    size_t scratch_cap[TB_NSLOTS] = {};
};

int tb_fail(tb_ctx* ctx, int code, const char* fmt, ...);
void tb_prof_begin(tb_ctx* ctx, const char* name);
void tb_prof_end(tb_ctx* ctx);
int tb_scratch(tb_ctx* ctx, int slot, size_t bytes, void** out);
int tb_lds_limit(tb_ctx* ctx, const void* kernel, size_t bytes); /* before a launch with `bytes` of dynamic LDS */

#define TB_HIP(ctx, call)                                                                     \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return tb_fail((ctx), TB_EDEVICE, "%s: %s (%s:%d)", #call, hipGetErrorString(e_), \
                           __FILE__, __LINE__);                                               \
    } while (0)

/* the same for a call that reports through tb_fail itself */
#define TB_TRY(call)            \
    do {                        \
        int rc_ = (call);       \
        if (rc_) return rc_;    \
    } while (0)

/* Every kernel launch of the library: `kernel` on the context's stream, timed as one profile record `name`, and a launch
 * the runtime refused reported through tb_fail. name == nullptr leaves the profile alone: a launch inside an explicit
 * tb_prof_begin / tb_prof_end pair (one record over several launches) or one that is not timed at all. */
template <class... P, class... A>
static int tb_launch(tb_ctx* ctx, const char* name, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, const A&... args) {
    if (name) tb_prof_begin(ctx, name);
    hipLaunchKernelGGL(kernel, grid, block, lds, ctx->stream, args...);
    if (name) tb_prof_end(ctx);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return tb_fail(ctx, TB_EDEVICE, "launch of %s: %s", name ? name : "a kernel", hipGetErrorString(e));
    return TB_OK;
}

/* The device buffers of one handle: every pointer tb_dev_alloc hands out is recorded here, and release() frees them all, so a
 * handle has no free list to keep in step with its allocations and a group that failed half way is not lost track of. */
struct tb_dev_owner {
    std::vector<void*> ptrs;
    void release() {
        for (void* p : ptrs) hipFree(p);
        ptrs.clear();
    }
};

/* `count` elements of T into *out, owned by `own`; fill 0 or 0xff queues that byte fill on the context's stream, -1 leaves
 * the buffer uninitialised. */
template <class T>
static int tb_dev_alloc(tb_ctx* ctx, tb_dev_owner& own, T** out, size_t count, int fill = -1) {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, count * sizeof(T));
    if (e == hipSuccess) {
        own.ptrs.push_back(p);
        *out = static_cast<T*>(p);
        if (fill >= 0) e = hipMemsetAsync(p, fill, count * sizeof(T), ctx->stream);
    }
    if (e != hipSuccess) return tb_fail(ctx, TB_EDEVICE, "device buffer of %zu x %zu bytes: %s", count, sizeof(T), hipGetErrorString(e));
    return TB_OK;
}

/* First statement of every entry point that takes a context or a plan: the HIP "current device" is per host thread and
 * the caller may hold contexts on several GPUs (or drive one context from several threads in turn), so every call binds
 * its thread to the context's device before it launches, copies or allocates. A null context falls through to the
 * function's own argument check. */
#define TB_ENTER(ctx)                                                                          \
    do {                                                                                       \
        tb_ctx* c_ = (ctx);                                                                    \
        if (c_) {                                                                              \
            hipError_t e_ = hipSetDevice(c_->device);                                          \
            if (e_ != hipSuccess) { /* tb_fail itself makes no HIP call and must not come back here */ \
                c_->err = std::string("hipSetDevice: ") + hipGetErrorString(e_);               \
                return TB_EDEVICE;                                                             \
            }                                                                                  \
        }                                                                                      \
    } while (0)

/* Geometry of one pyramid level inside a plan (host and device copies are identical). */
struct LevelGeom {
    int w, h, stride;     /* stride of the slab copy of this level */
    int nCols, nRows;     /* 30-px cell grid, ORBextractor.cpp:757-763 */
    int wCell, hCell;
    int cellBase;         /* index of this level's first entry in the cell table */
    int nCells;           /* valid (not skipped) cells of this level */
    int candCap;          /* capacity of the per-image candidate array of this level */
    int nodeCap;          /* quadtree list capacity = quota + 3 + 4*nIni (this call) */
    int nodeCapAlloc;     /* slots reserved for this level in the selection array */
    int nIni;             /* DistributeOctTree initial nodes, ORBextractor.cpp:498 */
    int quota;            /* mnFeaturesPerLevel[level] of the current call */
    int selBase;          /* first slot of this level in the per-image selection array */
    float hX;             /* (maxX-minX)/nIni as float, ORBextractor.cpp:500 */
    float patchSize;      /* (float)(int)(31*sf[level]), ORBextractor.cpp:812 */
    float sf;             /* mvScaleFactor[level] */
    float inv_sf;         /* FASTExtractor scale argument (fastgrid only) */
    unsigned long long off;     /* byte offset of the level inside one image's slab */
    unsigned long long candOff; /* element offset of the level inside one image's candidate array */
};

struct PlanGeom {
    int nlevels;
    int width, height;
    int selCap;                      /* slots per image in the selection / result arrays */
    unsigned long long slabBytes;    /* bytes per image slab */
    unsigned long long candPerImage; /* candidate records per image */
    /* level-0 source: external frames (dev pointer) or the slab */
    const uint8_t* img0;
    unsigned long long img0_pitch;
    int img0_stride;
    int pad_;
    LevelGeom lv[TB_MAX_LEVELS];
};

/* One FAST work item (k_fast_blocks): a block of ncx x ncy adjacent 30-px cells of one level, staged in LDS once.
 * The ROI is the union of the cells' cv::FAST ROIs (ORBextractor.cpp:765-786): cell (i, j) of the block scans columns
 * [x0 + 3 + j wCell, min(x0 + 3 + (j + 1) wCell, x1 - 3)) and rows likewise -- the cells' scan regions tile the ROI's. */
struct FastBlock {
    int16_t level;
    int16_t ncx, ncy;       /* cells of this block (<= FB_MAX_CX x FB_MAX_CY) */
    int16_t sA;             /* stage-1 lane map, fixed per block (host arithmetic, k_fast.hip): first 16-byte tile segment */
    int16_t x0, y0, x1, y1; /* ROI in absolute level coordinates, [x0,x1) x [y0,y1) */
    int16_t nss, rowsPer;   /*   that holds scanned columns, number of such segments, rows per 64-lane pass = 64 / nss, */
    int16_t nPass;          /*   passes over the scanned rows, */
    uint16_t invNss;        /*   ceil(32768 / nss): lane / nss == (lane * invNss) >> 15 for lane < 64 */
};
#define FB_S 160            /* LDS row stride of a block tile (bytes, 10 x 16) */
#ifndef FB_TH
#define FB_TH 68            /* tile rows */
#endif
#define FB_MAX_CX 4
#ifndef FB_MAX_CY
#define FB_MAX_CY 2
#endif

/* resize tables, built on the host with the oracle-identical double/float arithmetic */
struct ResizeX { int16_t sx, sx1, a0, a1; };
struct ResizeY { int32_t sy0, sy1; int16_t b0, b1; };

struct tb_extractor {
    tb_ctx* ctx = nullptr;
    PlanGeom g;                /* host copy; img0* fields updated per call */
    int max_images = 0, max_target = 0;
    std::vector<float> sf;
    bool have_quotas = false;
    int quotas[TB_MAX_LEVELS];
    int last_n = 0;
    bool last_was_orb = false;
    /* device memory */
    uint8_t* d_slab = nullptr;          /* [max_images][slabBytes] */
    uint8_t* d_img0_copy = nullptr;     /* [max_images][h][stride0] for host-provided frames */
    FastBlock* d_blocks = nullptr; int nBlocksTotal = 0;   /* FAST work items of one image, level-major */
    ResizeX* d_rx[TB_MAX_LEVELS]; ResizeY* d_ry[TB_MAX_LEVELS];
    uint32_t* d_cand = nullptr;         /* [max_images][candPerImage] packed score<<24|y<<12|x */
    int32_t* d_candCount = nullptr;     /* [max_images][TB_MAX_LEVELS] */
    uint32_t* d_knode = nullptr;        /* [max_images][candPerImage] quadtree scratch */
    uint32_t* d_sel = nullptr;          /* [max_images][selCap] selected keypoints, packed */
    int32_t* d_selCount = nullptr;      /* [max_images][TB_MAX_LEVELS] */
    tb_keypoint* d_kps = nullptr;       /* [max_images][selCap] */
    uint8_t* d_desc = nullptr;          /* [max_images][selCap][32] */
    int32_t* d_counts = nullptr;        /* [max_images] */
    float* d_exit = nullptr; int exitCap = 0;   /* exit keys (x,y) */
    int32_t* d_enode = nullptr; size_t enodeCap = 0;
    /* fastgrid scratch */
    unsigned long long* d_gridBest = nullptr; size_t gridBestCap = 0;
    uint8_t* d_occ = nullptr; size_t occCap = 0;
};

/* The handles the VO loop (tb_vo.cpp) reads the fields of; their functions are tb_capi.cpp's. */
struct tb_vocab {
    tb_ctx* ctx = nullptr;
    int nnodes = 0, k = 0, L = 0, weighting = 0, scoring = 0;
    int32_t *d_child_start = nullptr, *d_child_items = nullptr, *d_word_id = nullptr;
    uint8_t* d_desc = nullptr;
    double* d_weight = nullptr;
};

/* the LSH matcher's parameters and its bit table (searchByNN) */
struct tb_lsh {
    tb_ctx* ctx = nullptr;
    int T = 0, k = 0, L = 0;
    std::vector<uint16_t> bits;   /* [T][k] */
    uint8_t* d_bits = nullptr;    /* [T][k] the same on the device */
};

/* the keyframe database: per sequence a ring of BowVectors */
struct tb_bow_db {
    tb_ctx* ctx = nullptr;
    int nseq = 0, cap = 0, pitch = 0, scoring = 0;
    long long nadded = 0;             /* adds since the last clear: the next one goes to slot nadded % cap */
    tb_dev_owner own;
    int32_t* words = nullptr;         /* [nseq][cap][pitch] */
    double* values = nullptr;         /* [nseq][cap][pitch] */
    int32_t* counts = nullptr;        /* [nseq][cap] */
    int32_t* kf_ids = nullptr;        /* [nseq][cap], -1 = empty */
};

/* the keyframe store and the work buffers of candidate verification */
struct tb_kf_store {
    tb_ctx* ctx = nullptr;
    int nseq = 0, cap = 0, pitch = 0, max_cand = 0;
    long long nadded = 0;                 /* adds since the last clear: the next one goes to slot nadded % cap */
    tb_dev_owner own;
    /* the rings, frame index s * cap + slot */
    tb_keypoint* keys = nullptr;          /* [nseq][cap][pitch] */
    uint8_t* desc = nullptr;              /* [nseq][cap][pitch][32] */
    uint64_t* fv = nullptr;               /* [nseq][cap][pitch] */
    float* mp = nullptr;                  /* [nseq][cap][pitch][3] */
    uint8_t* valid = nullptr;             /* [nseq][cap][pitch] */
    float* Tcw = nullptr;                 /* [nseq][cap][16] */
    int32_t *counts = nullptr, *fv_counts = nullptr, *kf_ids = nullptr;   /* [nseq][cap] */
    /* verification work, pairs = nseq * max_cand */
    int32_t *ix1 = nullptr, *ix2 = nullptr;                  /* [pairs] the matcher's frame indices */
    int32_t* best = nullptr;                                 /* [pairs][pitch][4] searchByBow's best rows */
    tb_match* matches = nullptr;                             /* [pairs][pitch] */
    tb_obs* obs = nullptr;                                   /* [pairs][pitch] */
    uint8_t* outlier = nullptr;                              /* [pairs][pitch] */
    double* err = nullptr;                                   /* [pairs][pitch][3] the pose kernel's residuals */
    float *seed = nullptr, *pose = nullptr;                  /* [pairs][16] */
    int32_t *mcounts = nullptr, *flags = nullptr, *ocounts = nullptr, *ninl = nullptr, *ckf = nullptr;   /* [pairs] */
    /* PnP in front of the pose stage (tb_kf_store_pnp_enable): off unless enabled, its buffers allocated at enable */
    bool pnp_on = false;
    tb_pnp_params pnp = {};
    int pnp_min = 0, pnp_expand = 0;
    tb_obs *rows0 = nullptr, *rows2 = nullptr;               /* [pairs][pitch] the rows stage's rows; the expanded rows */
    uint8_t *pmask = nullptr, *outlier2 = nullptr;           /* [pairs][pitch] */
    uint8_t* took = nullptr;                                 /* [pairs] the pair took the PnP path */
    float *ppose = nullptr, *seed2 = nullptr, *pose2 = nullptr;   /* [pairs][16] the PnP pose, the pose stage's seed, the second stage's pose */
    int32_t *cnt0 = nullptr, *cnt2 = nullptr, *pcons = nullptr, *pwin = nullptr, *pflags = nullptr, *ninl2 = nullptr;   /* [pairs], pwin [pairs][2] */
    /* the Sim(3) query (tb_kf_store_sim3_dev): reloc_done = a verification has filled the match lists; the buffers are allocated by
     * the first query */
    bool reloc_done = false, s3_ready = false;
    int reloc_ncand = 0;                                     /* the last verification's candidates per sequence */
    tb_sim3_row* s3_rows = nullptr;                          /* [pairs][pitch] */
    uint8_t* s3_mask = nullptr;                              /* [pairs][pitch] */
    int32_t *s3_cnt = nullptr, *s3_kf = nullptr, *s3_cons = nullptr, *s3_flags = nullptr;   /* [pairs] */
    float* s3_S12 = nullptr;                                 /* [pairs][16] */
    double* s3_srt = nullptr;                                /* [pairs][8] */
    /* the Sim(3) refinement query (tb_kf_store_sim3_refine_dev), allocated by its first call: the pixel rows (row i of a pair is row i
     * of s3_rows), their counts and keyframes as the row kernel writes them, the counts and seeds the optimiser runs on, its mask
     * and its four outputs. s3_done: a tb_kf_store_sim3_dev ran since the store was made or cleared and since the last verification (whose match lists its
     * masks and seeds belong to); s3_own_srt / s3_own_cons: it wrote cand_srt / cand_consensus into the store's own s3_srt / s3_cons; s3_min_cons: its min_consensus (-1: it selected nothing) */
    bool s3_done = false, s3_own_srt = false, s3_own_cons = false, o3_ready = false;
    int s3_min_cons = -1;
    tb_sim3_obs_row* o3_rows = nullptr;                      /* [pairs][pitch] */
    uint8_t* o3_mask = nullptr;                              /* [pairs][pitch] */
    int32_t *o3_cnt = nullptr, *o3_kf = nullptr, *o3_run = nullptr, *o3_inl = nullptr;   /* [pairs] */
    double *o3_seed = nullptr, *o3_srt = nullptr, *o3_stats = nullptr;                   /* [pairs][8] */
    float* o3_S12 = nullptr;                                 /* [pairs][16] */
    /* the SearchBySim3 query (tb_kf_store_sim3_search_dev), allocated by its first call: the operator's inputs the prep forms, its
     * outputs and the widened lists. w3_use: the last search asked for use_for_refine and no verification, Sim(3) query or clear came
     * since: the next refinement builds its rows from w3_wide and starts with every row active (w3_ones, all 1, never written
     * again); w3_qpitch: that search's query pitch, the row pitch of w3_match1. o3_wide: the last refinement did so */
    bool w3_ready = false, w3_use = false, o3_wide = false;
    int w3_qpitch = 0;
    float *w3_pts1 = nullptr, *w3_pts2 = nullptr;            /* [pairs][pitch][3] */
    uint8_t *w3_m1 = nullptr, *w3_m2 = nullptr, *w3_ones = nullptr;   /* [pairs][pitch] */
    int32_t *w3_wink = nullptr, *w3_match1 = nullptr, *w3_match2 = nullptr;   /* [pairs][pitch] */
    tb_match *w3_pairs = nullptr, *w3_wide = nullptr;        /* [pairs][pitch] */
    int32_t *w3_pcnt = nullptr, *w3_wcnt = nullptr, *w3_skip = nullptr, *w3_f1 = nullptr, *w3_f2 = nullptr;   /* [pairs] */
    int32_t* w3_stats = nullptr;                             /* [pairs][8] */
    /* the Sim(3) graph query (tb_kf_store_sim3_graph_dev): the store's own copy of the last Sim(3) query's best_kf / best_srt (the
     * caller's are nullable and may be gone by then; s3_best: that query selected a winner into them), and the graph's buffers,
     * allocated with the solver's plan by the first graph query; nn = cap + 1 */
    bool s3_best = false, g3_ready = false;
    int32_t* s3_best_kf = nullptr;                           /* [nseq] */
    double* s3_best_srt = nullptr;                           /* [nseq][8] */
    int32_t *g3_nnodes = nullptr, *g3_ecount = nullptr;      /* [nseq] */
    int32_t* g3_node_kf = nullptr;                           /* [nseq][nn] */
    double *g3_before = nullptr, *g3_after = nullptr;        /* [nseq][nn][8] */
    tb_pg_sim3_edge* g3_edges = nullptr;                     /* [nseq][nn] */
    double* g3_stats = nullptr;                              /* [nseq][8] */
};

/* tb_kf_store_sim3_graph_dev with the id the query frame's node is given (the public entry: -2; the VO loop: its frame index) */
extern "C" int tb_kf_store_sim3_graph_run(tb_kf_store* st, const char* who, const float* q_Tcw, int frame_id, int iters, int fixed_scale, double w_rot,
                               double w_trans, double w_scale, tb_sim3_graph_out* out);

/* the depth filter (k_depth_filter.hip): per sequence `pitch` entries, a ring of ref_slots reference images with their poses */
struct tb_depth_filter {
    tb_ctx* ctx = nullptr;
    int nseq = 0, pitch = 0, ref_slots = 0, width = 0, height = 0;
    double K[4] = {};
    double px_err = 0.0;                  /* 2 atan(px_noise / (2 sqrt(fx fy))) */
    tb_depth_filter_params prm = {};
    tb_dev_owner own;
    tb_df_seed* seeds = nullptr;          /* [nseq][pitch] */
    tb_df_trace* traces = nullptr;        /* [nseq][pitch] */
    uint8_t* ring = nullptr;              /* [nseq][ref_slots][height][width] */
    float* ring_Tcw = nullptr;            /* [nseq][ref_slots][16] */
    int32_t* newest = nullptr;            /* [nseq] the slot of the last keyframe, -1 before the first */
    int32_t* freelist = nullptr;          /* [nseq][pitch] k_df_add's list of free entries */
    std::vector<int32_t> h_newest;        /* the host's copy of newest: the same rule, no read back */
};
/* one launch over sequences [seq0, seq0 + nseq) */
int tbk_df_update(tb_depth_filter* df, int seq0, int nseq, const uint8_t* images, int stride, size_t image_pitch, const float* Tcw);
int tbk_df_add(tb_depth_filter* df, int seq0, int nseq, const uint8_t* images, int stride, size_t image_pitch, const float* Tcw,
               const float* keys_xy, const int32_t* counts, int key_pitch, const uint8_t* skip, int32_t* not_added);
int tbk_df_points(tb_depth_filter* df, float* points, uint8_t* flags, int release);

/* kernel launchers (k_*.hip) */
int tbk_resize_level(tb_extractor* ex, int level, int n);
int tbk_fast_cells(tb_extractor* ex, int n, int init_th, int min_th);
int tbk_octree(tb_extractor* ex, int n, int n_exit);
int tbk_describe(tb_extractor* ex, int n);
int tbk_fast_image(tb_ctx* ctx, const uint8_t* d_img, int w, int h, int stride, int th, int nms, int arc,
                   uint32_t* d_out, int cap, int32_t* d_count);
int tbk_fastgrid(tb_extractor* ex, int n, int target, float threshold, int n_occ);
int tbk_bf_batch(tb_ctx* ctx, int npairs, const uint8_t* d1, const int32_t* c1, const uint8_t* d2,
                 const int32_t* c2, size_t set_pitch, int max_n, int crosscheck, int filter, float ratio,
                 float min_th, tb_match* out, int cap, int32_t* out_counts, unsigned long long* d_tbest,
                 unsigned long long* d_qbest);
int tbk_lsh_batch(tb_ctx* ctx, int npairs, const uint8_t* d1, const int32_t* c1, const uint8_t* d2, const int32_t* c2, size_t set_pitch,
                  int max_n, const uint8_t* d_bits, int T, int k, int L, int filter, float ratio, float min_th, tb_match* out, int cap,
                  int32_t* out_counts, unsigned long long* d_qbest);
int tbk_violence_batch(tb_ctx* ctx, int npairs, const tb_keypoint* d_k1, const uint8_t* d_d1, const int32_t* d_n1, int pitch1,
                       const tb_keypoint* d_k2, const uint8_t* d_d2, const int32_t* d_n2, int pitch2, const int32_t* d_cellStart,
                       const int32_t* d_cellItems, int img2_w, int img2_h, int min_level, int max_level, float radius, int th_low,
                       float nratio, int histo_len, int check_orientation, int32_t* d_best, tb_match* d_out, int cap,
                       int32_t* d_out_counts, int32_t* d_flags);
/* device-resident lookup grids and the batched searchByProjection(F1, F2) on them */
int tbk_grid_build_batch(tb_ctx* ctx, int nframes, const tb_keypoint* d_keys, const int32_t* d_counts, int key_pitch, int img_w,
                         int img_h, int32_t* d_cellStart, int32_t* d_cellItems);
int tbk_projection_batch(tb_ctx* ctx, int npairs, const float* d_Tcw, const tb_camera* cam, int img_w, int img_h,
                         const tb_keypoint* d_k1, const uint8_t* d_d1, const uint8_t* d_taken1, const int32_t* d_n1, int pitch1,
                         const int32_t* d_cellStart, const int32_t* d_cellItems, const tb_keypoint* d_k2, const tb_mappoint* d_mp2,
                         const uint8_t* d_mp2d, const int32_t* d_n2, int pitch2, const float* sf, int nlevels, float nratio,
                         int th_high, int histo_len, int check_orientation, int32_t* d_best, tb_match* d_out, int cap,
                         int32_t* d_out_counts, int32_t* d_flags, int map_mode, float radio, int max_n2);
int tbk_bow_transform(tb_ctx* ctx, int nnodes, int L, const int32_t* d_child_start, const int32_t* d_child_items, const uint8_t* d_vdesc,
                      const int32_t* d_word_id, const double* d_weight, int nframes, const uint8_t* d_desc, const int32_t* d_counts,
                      int desc_pitch, int levelsup, int32_t* d_word_ids, int32_t* d_node_ids, double* d_weights,
                      unsigned long long* d_fv_keys, int32_t* d_fv_counts);
int tbk_bow_vector(tb_ctx* ctx, int nframes, const int32_t* d_word_ids, const double* d_weights, const int32_t* d_counts, int desc_pitch,
                   int weighting, int scoring, int32_t* d_bv_words, double* d_bv_values, int32_t* d_bv_counts);
int tbk_bow_search_batch(tb_ctx* ctx, int npairs, const tb_keypoint* d_k1, const uint8_t* d_d1, int pitch1, const unsigned long long* d_fv1,
                         const int32_t* d_n1, const tb_keypoint* d_k2, const uint8_t* d_d2, int pitch2, const unsigned long long* d_fv2,
                         const int32_t* d_n2, const uint8_t* d_has_mp2, int map_point_only, int th_low, float nratio, int histo_len,
                         int check_orientation, tb_match* d_out, int cap, int32_t* d_out_counts, int32_t* d_flags, int32_t* d_best,
                         const int32_t* d_ix1 = nullptr, const int32_t* d_ix2 = nullptr);
/* the keyframe store and candidate verification (k_reloc.hip); d_ix1 / d_ix2 above: the frame pair p reads on each side */
int tbk_kf_store_add(tb_ctx* ctx, int nseq, const tb_keypoint* d_keys, const uint8_t* d_desc, const int32_t* d_counts,
                     const unsigned long long* d_fv, const int32_t* d_fv_counts, const float* d_mp, const uint8_t* d_valid, int src_pitch,
                     const float* d_Tcw, int32_t kf_id, int cap, int pitch, int slot, tb_keypoint* s_keys, uint8_t* s_desc,
                     unsigned long long* s_fv, float* s_mp, uint8_t* s_valid, float* s_Tcw, int32_t* s_counts, int32_t* s_fv_counts,
                     int32_t* s_kf_ids);
int tbk_reloc_pairs(tb_ctx* ctx, int nseq, int ncand, int cap, const int32_t* d_cand_slot, const int32_t* d_kf_ids, const float* d_kf_Tcw,
                    int32_t* d_ix1, int32_t* d_ix2, float* d_seed, int32_t* d_cand_kf);
int tbk_reloc_rows(tb_ctx* ctx, int npairs, const tb_keypoint* d_q_keys, const int32_t* d_q_counts, int q_pitch, const int32_t* d_ix1,
                   const int32_t* d_ix2, const tb_match* d_matches, const int32_t* d_match_counts, const float* d_kf_mp,
                   const uint8_t* d_kf_valid, const int32_t* d_kf_counts, int pitch, const float* inv_sigma2, int nlevels, tb_obs* d_obs,
                   int32_t* d_obs_counts, uint8_t* d_outlier, int32_t* d_rows_out);
int tbk_reloc_select(tb_ctx* ctx, int nseq, int ncand, int min_inliers, const int32_t* d_cand_kf, const int32_t* d_cand_inliers,
                     const float* d_cand_Tcw, int32_t* d_best_rank, int32_t* d_best_kf, float* d_best_Tcw);
/* recovery in the VO loop (k_reloc.hip): every array at one pitch, the loop's key pitch. The pick (which pair a sequence adopts),
 * the store's work buffers and rings, the ring-aligned database, the loop's word / node rings, and the loop's state and snapshot. */
struct tb_vo_recover_args {
    int topk, pitch;
    const uint8_t* lost; const int32_t *best_rank, *best_kf, *ix2; const float* best_Tcw;
    const tb_match* w_matches; const tb_obs* w_obs; const uint8_t* w_outlier; const int32_t *w_mcounts, *w_flags, *w_ocounts, *w_ninl;
    const tb_keypoint* s_keys; const uint8_t* s_desc; const unsigned long long* s_fv; const float* s_mp; const uint8_t* s_valid;
    const int32_t *s_counts, *s_fv_counts;
    const int32_t* db_words; const double* db_values; const int32_t* db_counts;
    const int32_t *word_ring, *node_ring;
    const int32_t* orb_counts;
    float *Tcw, *mp; uint8_t* valid; tb_obs* obs; uint8_t* outlier; tb_match* matches;
    int32_t *obs_counts, *n_inliers, *mcounts, *mflags, *recovered_kf;
    tb_keypoint* kf_orb; uint8_t* kf_desc; unsigned long long* kf_fv; float* kf_mp; uint8_t* kf_valid; int32_t *kf_cnt, *kf_fv_cnt;
    int32_t* kf_bv_word; double* kf_bv_val; int32_t* kf_bv_cnt; int32_t *kf_word, *kf_node, *kf_ids;
};
int tbk_vo_recover_mask(tb_ctx* ctx, int nseq, int topk, int lost_inliers, const int32_t* d_n_inliers, const int32_t* d_top_slot,
                        uint8_t* d_lost, int32_t* d_track_inliers, int32_t* d_masked);
int tbk_vo_recover_adopt(tb_ctx* ctx, int nseq, const tb_vo_recover_args* a);
int tbk_vo_recover_switch(tb_ctx* ctx, int nseq, const tb_vo_recover_args* a);
int tbk_vo_recover_ring_add(tb_ctx* ctx, int nseq, const int32_t* d_word, const int32_t* d_node, const int32_t* d_counts, int cap, int pitch,
                            int slot, int32_t* d_word_ring, int32_t* d_node_ring);
/* BowVector scoring and the keyframe database's kernels (k_bow_score.hip): query i of na meets entries i * bq + j, j in [0, nj),
 * out [na][nj]; ring != 0: the entries are ring slots, of which nfilled are in use, the last add went to `newest`, and the
 * `exclude` newest adds are left out (their out is a quiet NaN) */
int tbk_bow_score(tb_ctx* ctx, int scoring, double log_eps, int na, const int32_t* d_aw, const double* d_av, const int32_t* d_ac, int a_pitch,
                  const int32_t* d_bw, const double* d_bv, const int32_t* d_bc, int b_pitch, int nj, int bq, int ring, int nfilled,
                  int newest, int exclude, double* d_out);
int tbk_bow_db_add(tb_ctx* ctx, int nseq, const int32_t* d_src_w, const double* d_src_v, const int32_t* d_src_c, int src_pitch, int cap,
                   int pitch, int slot, int32_t kf_id, int32_t* d_words, double* d_values, int32_t* d_counts, int32_t* d_kf_ids);
int tbk_bow_db_rank(tb_ctx* ctx, int nseq, const double* d_scores, const int32_t* d_kf_ids, int cap, int nfilled, int newest, int exclude,
                    int ascending, int topk, int32_t* d_top_slot, int32_t* d_top_kf, double* d_top_score, int32_t* d_top_count);
/* vocabulary training (k_vocab.hip): the device arrays of a tb_vocab, owned by the caller on success */
struct tb_vocab_arrays {
    int nnodes = 0;
    int32_t *d_child_start = nullptr, *d_child_items = nullptr, *d_word_id = nullptr;
    uint8_t* d_desc = nullptr;
    double* d_weight = nullptr;
};
int tbk_vocab_train(tb_ctx* ctx, const tb_vocab_train_params* P, int ndocs, const uint8_t* d_desc, const int32_t* h_counts,
                    int desc_pitch, tb_vocab_arrays* out, tb_vocab_train_stats* stats);
int tbk_pack_rows(tb_ctx* ctx, const void* d_src, int row_bytes, int cap, const int32_t* d_counts, int nframes, void* d_dst, long long* d_total);
int tbk_copy16(tb_ctx* ctx, const void* d_src, void* d_dst, size_t bytes);
int tbk_stereo_obs(tb_ctx* ctx, int nframes, const tb_keypoint* d_kl, const tb_keypoint* d_kr, int key_pitch, const tb_match* d_matches,
                   const int32_t* d_match_counts, int match_pitch, const float K[4], float bf, const float* d_inv_sigma2, int nlevels,
                   tb_obs* d_obs, int obs_pitch, int32_t* d_obs_counts);
int tbk_pose_batch(tb_ctx* ctx, int nproblems, const double K[4], const float* Tcw_in, const tb_obs* obs,
                   const int32_t* counts, int obs_pitch, uint8_t* outlier, float* Tcw_out, int32_t* n_inliers,
                   double* stats, double* d_err);
int tbk_local_ba_batch(tb_ctx* ctx, int W, const double K[4], int nkf, int nfixed, float* d_poses, int npt, float* d_pts,
                       const tb_ba_obs* d_obs, const int32_t* d_counts, int obs_pitch, int iters, double* d_stats, void* d_work,
                       size_t work_bytes);
size_t tbk_local_ba_work_bytes(const tb_ctx* ctx, int W, int nkf, int nfixed, int npt, int obs_pitch);
/* pose-graph optimisation (k_pgo.hip): one workgroup per graph runs the whole LM loop; d_work: tbk_pose_graph_work_bytes */
size_t tbk_pose_graph_work_bytes(int ngraphs, int nnodes, int nfixed, int edge_pitch);
int tbk_pose_graph_batch(tb_ctx* ctx, int ngraphs, int nnodes, int nfixed, float* d_poses, const tb_pg_edge* d_edges,
                         const int32_t* d_counts, int edge_pitch, int iters, double* d_stats, void* d_work);
/* Sim(3) pose-graph optimisation (k_pgo_sim3.hip): as above on srt nodes [nnodes][8]; d_work: tbk_pose_graph_sim3_work_bytes */
size_t tbk_pose_graph_sim3_work_bytes(int ngraphs, int nnodes, int nfixed, int edge_pitch);
int tbk_pose_graph_sim3_batch(tb_ctx* ctx, int ngraphs, int nnodes, int nfixed, int fixed_scale, double* d_nodes,
                              const tb_pg_sim3_edge* d_edges, const int32_t* d_counts, int edge_pitch, int iters, double* d_stats,
                              void* d_work);
/* the Sim(3) graph of a store's live keyframes and a query frame (k_pgo_sim3.hip): k_vo_loop_graph's rules on srt nodes, the loop
 * edge the kept best_srt byte for byte */
int tbk_sim3_graph(tb_ctx* ctx, int nseq, int cap, int nlive, int oldest, int frame_id, double w_rot, double w_trans, double w_scale,
                   const float* s_Tcw, const int32_t* s_kf_ids, const float* q_Tcw, const int32_t* best_kf, const double* best_srt,
                   double* before, double* after, int32_t* node_kf, int32_t* nnodes, tb_pg_sim3_edge* edges, int32_t* ecount);
/* loop correction in the VO loop (k_pgo.hip): the graph of the stored keyframes (ring slots (oldest + i) % cap, i < nlive) and the
 * current frame, cap + 1 nodes and edge pitch cap + 1 per sequence; and the adoption of the solver's poses */
int tbk_vo_loop_graph(tb_ctx* ctx, int nseq, int cap, int nlive, int oldest, int frame, int topk, double w_rot, double w_trans,
                      const float* s_Tcw, const int32_t* s_kf_ids, const float* cur_Tcw, const int32_t* best_rank, const int32_t* best_kf,
                      const float* best_Tcw, float* before, float* after, int32_t* node_kf, int32_t* nnodes, tb_pg_edge* edges,
                      int32_t* ecount);
int tbk_vo_loop_adopt(tb_ctx* ctx, int nseq, int cap, int nlive, int oldest, int topk, int pitch, const float* before, const float* after,
                      const int32_t* ecount, const double* stats, const int32_t* best_rank, const int32_t* best_kf,
                      const int32_t* cand_inliers, float* s_Tcw, float* s_mp, const uint8_t* s_valid, const int32_t* s_counts, float* kf_mp,
                      const uint8_t* kf_valid, const int32_t* kf_cnt, float* mp, const uint8_t* valid, const int32_t* key_counts, float* Tcw,
                      uint8_t* closed, int32_t* loop_kf, int32_t* loop_inliers);
int tbk_clahe(tb_ctx* ctx, int nimg, const uint8_t* d_src, int w, int h, int stride, size_t spitch, double clip_limit, int tiles_x,
              int tiles_y, uint8_t* d_dst, int dstride, size_t dpitch, uint8_t* d_lut);
int tbk_flow_accept(tb_ctx* ctx, int npairs, const float* d_cur, uint8_t* d_status, const int32_t* d_counts, int pts_pitch, int width,
                    int height, tb_match* d_out, int cap, int32_t* d_out_counts);
/* RANSAC fundamental matrix (k_ransac.hip): mode 0 = Matcher::rejectWithF on the flagged points, 1 = cv::findFundamentalMat on all */
size_t tbk_ransac_work_bytes(int npairs, int pts_pitch);
int tbk_ransac_f(tb_ctx* ctx, int npairs, const float* d_pts1, const float* d_pts2, uint8_t* d_status, const int32_t* d_counts,
                 int pts_pitch, int mode, double thresh, double conf, void* d_work, int32_t* d_flags, double* d_F, int32_t* d_iters);
int tbk_stereo_depth(tb_ctx* ctx, int npairs, const float* d_cur, const float* d_keys, const uint8_t* d_status, const int32_t* d_counts,
                     int pts_pitch, float bf, float* d_depth);
size_t tbk_lk_work_bytes(int w, int h, int max_level, int npairs);
int tbk_lk_track(tb_ctx* ctx, int npairs, const uint8_t* d_prev, const uint8_t* d_next, int w, int h, int stride, size_t image_pitch,
                 const float* d_prev_pts, const int32_t* d_counts, int n, int pts_pitch, int win, int max_level, float* d_next_pts,
                 uint8_t* d_status, float* d_err, void* d_work, int* top_level);

/* device-resident stereo VO loop (k_vo.hip) */
/* d_idx (nullable, here and below): the index list of a ragged step's keyframe block -- row j serves sequence d_idx[j] */
int tbk_vo_copy_image(tb_ctx* ctx, int nimg, const uint8_t* d_src, int w, int h, int stride, size_t pitch, uint8_t* d_dst,
                      const int32_t* d_idx = nullptr);
int tbk_vo_track(tb_ctx* ctx, int nseq, const int32_t* d_prev_counts, const uint8_t* d_status, const float* d_keys, const float* d_prev_mp,
                 const uint8_t* d_prev_valid, int pitch, int32_t* d_key_counts, float* d_mp, uint8_t* d_valid, tb_obs* d_obs,
                 int32_t* d_obs_counts, uint8_t* d_outlier);
int tbk_vo_match_carry(tb_ctx* ctx, int nseq, const tb_keypoint* d_orb, const int32_t* d_orb_counts, const tb_match* d_matches,
                       const int32_t* d_match_counts, const float* d_kf_mp, const uint8_t* d_kf_valid, const int32_t* d_kf_counts, int pitch,
                       const float* inv_sigma2, int nlevels, int32_t* d_win, float* d_keys, int32_t* d_key_counts, float* d_mp,
                       uint8_t* d_valid, tb_obs* d_obs, int32_t* d_obs_counts, uint8_t* d_outlier);
int tbk_vo_kf_pack(tb_ctx* ctx, int nseq, const tb_keypoint* d_orb, const int32_t* d_orb_counts, int orb_pitch, int pitch, float* d_keys,
                   int32_t* d_key_counts, uint8_t* d_valid, const int32_t* d_idx = nullptr);
int tbk_vo_kf_spawn(tb_ctx* ctx, int nseq, const float* d_keys, const int32_t* d_key_counts, const float* d_depth, const float* d_Tcw,
                    const double K[4], int pitch, float* d_mp, uint8_t* d_valid, const int32_t* d_idx = nullptr);

int tbk_vo_proj_carry(tb_ctx* ctx, int nseq, int map_mode, const tb_keypoint* d_orb, const int32_t* d_orb_counts, const tb_match* d_matches,
                      const int32_t* d_match_counts, int match_pitch, const float* d_src_mp, const uint8_t* d_src_valid,
                      const tb_mappoint* d_src_rec, const uint8_t* d_src_desc, const int32_t* d_src_counts, int src_pitch, int pitch,
                      const float* inv_sigma2, int nlevels, int32_t* d_win, float* d_keys, int32_t* d_key_counts, float* d_mp,
                      uint8_t* d_valid, uint8_t* d_mp_desc, tb_obs* d_obs, int32_t* d_obs_counts, uint8_t* d_outlier);
int tbk_vo_kf_append(tb_ctx* ctx, int nseq, const int32_t* d_key_counts, const float* d_depth, const float* d_mp, const uint8_t* d_valid,
                     const uint8_t* d_orb_desc, const float* d_Tcw, int pitch, uint8_t* d_mp_desc, tb_mappoint* d_rec,
                     tb_mappoint* d_map_rec, uint8_t* d_map_desc, int32_t* d_map_n, int32_t* d_map_blocks, int nblk, int slot,
                     int map_pitch, const int32_t* d_idx = nullptr);
int tbk_vo_map_evict(tb_ctx* ctx, int nseq, const tb_mappoint* d_src_rec, const uint8_t* d_src_desc, const int32_t* d_src_n,
                     const int32_t* d_src_blocks, int nblk, int map_pitch, tb_mappoint* d_dst_rec, uint8_t* d_dst_desc, int32_t* d_dst_n,
                     int32_t* d_dst_blocks);
/* Ragged batches (k_vo.hip): the outputs of one frame that are not part of the ping-pong (a ragged step writes a second set and
 * keeps the previous one for the hold) and the keyframe snapshot; nullable members belong to the loops that have them. */
struct tb_vo_frame_out {
    tb_obs* obs = nullptr; int32_t* obs_counts = nullptr; uint8_t* outlier = nullptr; int32_t* n_inliers = nullptr;
    tb_keypoint* orb = nullptr; uint8_t* orb_desc = nullptr; int32_t* orb_cnt = nullptr;
    tb_match* matches = nullptr; int32_t *mcounts = nullptr, *mflags = nullptr;
    uint8_t* mp_desc = nullptr;
    int32_t *bow_word = nullptr, *bow_node = nullptr; uint64_t* fv_keys = nullptr; int32_t* fv_cnt = nullptr;
    int32_t* bv_word = nullptr; double* bv_val = nullptr; int32_t* bv_cnt = nullptr;
};
struct tb_vo_kf_out {
    tb_keypoint* orb = nullptr; uint8_t* desc = nullptr; int32_t* cnt = nullptr; float* mp = nullptr; uint8_t* valid = nullptr;
    uint8_t* mp_desc = nullptr;
    int32_t *bow_word = nullptr, *bow_node = nullptr; uint64_t* fv_keys = nullptr; int32_t* fv_cnt = nullptr;
    int32_t* bv_word = nullptr; double* bv_val = nullptr; int32_t* bv_cnt = nullptr;
};
struct tb_vo_hold_args {
    const int32_t* mask; int pitch, match_pitch; size_t npx;   /* mask [nseq]: 0 idle, 1 active, 2 active on its frame 0 */
    uint8_t* img[2]; float* keys[2]; float* mp[2]; uint8_t* valid[2]; int32_t* kcnt[2]; float* Tcw[2];   /* [0] side a, [1] side b */
    tb_vo_frame_out prev, cur;
};
int tbk_vo_reset_seq(tb_ctx* ctx, int nseq, const int32_t* d_mask, const float* d_Tcw0, float* d_Tcw, int32_t* d_key_counts,
                     int32_t* d_kf_counts, int32_t* d_kf_fv_counts, int32_t* d_kf_bv_counts, int32_t* d_cell_start, int ncell);
int tbk_vo_hold(tb_ctx* ctx, int nseq, const tb_vo_hold_args* a);
int tbk_vo_kf_gather(tb_ctx* ctx, int nkf, const int32_t* d_idx, const float* d_keys, const int32_t* d_key_counts, int pitch,
                     float* d_out_keys, int32_t* d_out_counts);
int tbk_vo_kf_snapshot(tb_ctx* ctx, int nkf, const int32_t* d_idx, int pitch, const tb_vo_frame_out* cur, const float* d_mp,
                       const uint8_t* d_valid, const tb_vo_kf_out* kf);

/* window BA of the optical-flow loop (k_vo.hip): the segment log [nseq][nslot] at the loop's key pitch, the window, the adoption */
int tbk_vo_seg_start(tb_ctx* ctx, int nseq, const float* d_keys, const int32_t* d_key_counts, const float* d_depth, const float* d_mp,
                     const uint8_t* d_valid, const float* d_Tcw, int pitch, int nslot, float* d_seg_keys, uint8_t* d_seg_ok, float* d_seg_pose, float* d_seg_pts,
                     uint8_t* d_seg_spawned);
int tbk_vo_seg_log(tb_ctx* ctx, int nseq, const float* d_keys, const int32_t* d_key_counts, const uint8_t* d_valid, const uint8_t* d_outlier,
                   const int32_t* d_obs_counts, const float* d_Tcw, const uint8_t* d_seg_spawned, int pitch, int nslot, int slot,
                   float* d_seg_keys, uint8_t* d_seg_ok, float* d_seg_pose);
int tbk_vo_seg_window(tb_ctx* ctx, int nseq, const float* d_seg_keys, const uint8_t* d_seg_ok, int pitch, int nslot, int min_obs,
                      tb_ba_obs* d_obs, int32_t* d_obs_counts, int32_t* d_n_points);
int tbk_vo_seg_adopt(tb_ctx* ctx, int nseq, const float* d_win_pose, const int32_t* d_n_points, const double* d_stats, int nslot,
                     int min_points, float* d_Tcw, uint8_t* d_adopted);

/* linear triangulation (k_triangulate.hip); zeroes d_tally first */
int tbk_linear_triangle(tb_ctx* ctx, int npairs, const float* d_xy0, const float* d_xy1, const int32_t* d_counts, int pitch,
                        const float* d_Tcw0, const float* d_Tcw1, const double K[4], const float* d_inv_sigma2_0,
                        const float* d_inv_sigma2_1, const uint8_t* d_skip, double cos_parallax_max, double chi2_max, float* d_points,
                        uint8_t* d_flags, int32_t* d_tally);
/* P3P-RANSAC (k_pnp.hip): one workgroup per problem, no work buffer; every output nullable */
int tbk_pnp_batch(tb_ctx* ctx, int nproblems, const double K[4], const tb_obs* d_obs, const int32_t* d_counts, int obs_pitch, int hypotheses,
                  double chi2_max, unsigned long long seed, const float* d_Tcw_prior, float* d_Tcw_out, int32_t* d_consensus,
                  uint8_t* d_inlier, int32_t* d_winner, int32_t* d_flags);
/* Sim(3) RANSAC (k_sim3.hip): one workgroup per problem, no work buffer; every output nullable. The store's query around it: the
 * 3D-3D rows of every pair through the verification's match lists (cand_kf -1 = no candidate), and the selection */
int tbk_sim3_batch(tb_ctx* ctx, int nproblems, const double K[4], const tb_sim3_row* d_rows, const int32_t* d_counts, int pitch, int hypotheses,
                   int fixed_scale, double chi2_max, unsigned long long seed, float* d_S12, double* d_srt, int32_t* d_consensus,
                   uint8_t* d_inlier, int32_t* d_winner, int32_t* d_flags);
int tbk_sim3_rows(tb_ctx* ctx, int npairs, int ncand, int cap, const int32_t* d_cand_slot, const int32_t* d_kf_ids, const tb_keypoint* d_q_keys,
                  const int32_t* d_q_counts, const float* d_q_mp, const uint8_t* d_q_valid, int q_pitch, const float* d_q_Tcw,
                  const tb_match* d_matches, const int32_t* d_match_counts, const tb_keypoint* d_kf_keys, const float* d_kf_mp,
                  const uint8_t* d_kf_valid, const int32_t* d_kf_counts, const float* d_kf_Tcw, int pitch, const float* inv_sigma2, int nlevels,
                  tb_sim3_row* d_rows, int32_t* d_row_counts, int32_t* d_cand_kf, int32_t* d_rows_out);
/* the same rows with the two keys' pixels (tb_kf_store_sim3_refine_dev), and that query's kernels around the optimiser */
int tbk_sim3_obs_rows(tb_ctx* ctx, int npairs, int ncand, int cap, const int32_t* d_cand_slot, const int32_t* d_kf_ids,
                      const tb_keypoint* d_q_keys, const int32_t* d_q_counts, const float* d_q_mp, const uint8_t* d_q_valid, int q_pitch,
                      const float* d_q_Tcw, const tb_match* d_matches, const int32_t* d_match_counts, const tb_keypoint* d_kf_keys,
                      const float* d_kf_mp, const uint8_t* d_kf_valid, const int32_t* d_kf_counts, const float* d_kf_Tcw, int pitch,
                      const float* inv_sigma2, int nlevels, tb_sim3_obs_row* d_rows, int32_t* d_row_counts, int32_t* d_cand_kf);
int tbk_sim3_refine_prep(tb_ctx* ctx, int npairs, const int32_t* d_cand_kf, const int32_t* d_cand_consensus, const double* d_cand_srt,
                         const int32_t* d_row_counts, int32_t* d_counts, double* d_seed);
int tbk_sim3_refine_select(tb_ctx* ctx, int nseq, int ncand, int min_consensus, int min_inliers, int use_for_graph, const int32_t* d_cand_kf,
                           const int32_t* d_cand_consensus, double* d_srt, float* d_S12, int32_t* d_inl, double* d_stats, double* o_srt,
                           float* o_S12, int32_t* o_inl, double* o_stats, double* b_srt, float* b_S12, int32_t* b_inl, double* b_stats,
                           double* d_keep_srt);
int tbk_sim3_select(tb_ctx* ctx, int nseq, int ncand, int min_consensus, const int32_t* d_cand_kf, const int32_t* d_cand_consensus,
                    const float* d_cand_S12, const double* d_cand_srt, int32_t* d_best_rank, int32_t* d_best_kf, float* d_best_S12,
                    double* d_best_srt, int32_t* d_keep_kf, double* d_keep_srt);
/* Sim(3) refinement on pixel rows (k_sim3_opt.hip): one workgroup per problem, no work buffer; d_active, d_srt_out, d_S12,
 * d_inliers and d_stats nullable, d_mask not (it carries the rows' active flags during the call) */
int tbk_sim3_opt_batch(tb_ctx* ctx, int nproblems, const double K[4], const tb_sim3_obs_row* d_rows, const int32_t* d_counts, int pitch,
                       const uint8_t* d_active, const double* d_srt_in, const tb_sim3_opt_params* prm, double* d_srt_out, float* d_S12,
                       int32_t* d_inliers, uint8_t* d_mask, double* d_stats);
/* tb_sim3_optimize_batch_dev's parameter rules, for the entry points around it */
static inline bool tb_sim3_opt_params_ok(const tb_sim3_opt_params* prm) {
    auto it = [](int v) { return v >= 0 && v <= 99; };
    return prm->th2 >= 0.0 && std::isfinite(prm->th2) && it(prm->iters_first) && it(prm->iters_bad) && it(prm->iters_clean) &&
           prm->min_keep >= 0 && (prm->fixed_scale == 0 || prm->fixed_scale == 1);
}
/* tb_sim3_ransac_batch_dev's parameter rules, for the entry points around it */
static inline bool tb_sim3_params_ok(const tb_sim3_params* prm) {
    return prm->hypotheses >= 1 && prm->hypotheses <= 1024 && (prm->fixed_scale == 0 || prm->fixed_scale == 1) && prm->chi2_max >= 0.0 &&
           std::isfinite(prm->chi2_max);
}
/* SearchBySim3 (k_sim3_search.hip): guided mutual matching of the two sides of every pair under its similarity. A side's keys,
 * descriptors, validity bytes and counts are read at frame[p] (nullptr: p) of their arrays, so a caller that keeps frames in a ring
 * reads them where they lie; its camera points and `already matched` bytes are per pair. d_skip (nullable): a non-zero entry skips
 * the pair (match -1, no pairs, stats flag 2). level_px[l]: the size of a level-l pixel in level-0 pixels (tb_scale_factors'
 * inv_sf). d_match1 / d_match2 are work AND output and not nullable here; d_pairs, d_pair_counts and d_stats are nullable. */
struct tbk_sim3_search_side {
    const tb_keypoint* keys; const uint8_t* desc; const uint8_t* valid; const int32_t* counts; const int32_t* frame;
    const float* points; const uint8_t* matched; int pitch;
};
int tbk_sim3_search_batch(tb_ctx* ctx, int npairs, const double K[4], int width, int height, int nlevels, const float* level_px,
                          const tbk_sim3_search_side* s1, const tbk_sim3_search_side* s2, const double* d_srt, const int32_t* d_skip,
                          float th, int th_high, int32_t* d_match1, int32_t* d_match2, tb_match* d_pairs, int cap, int32_t* d_pair_counts,
                          int32_t* d_stats);
/* the store's query around it (k_sim3.hip, beside the row kernel whose rule they walk): prep = skip flags, frame indices, the camera
 * points of both sides and the `already matched` bytes from the Sim(3) query's masks; merge = the widened match lists, then the
 * per-candidate counts to the caller and those of the selected candidate (min_consensus < 0: none was selected) */
int tbk_sim3_search_prep(tb_ctx* ctx, int npairs, int ncand, int cap, const int32_t* d_cand_slot, const int32_t* d_kf_ids,
                         const int32_t* d_q_counts, const float* d_q_mp, const uint8_t* d_q_valid, int q_pitch, const float* d_q_Tcw,
                         const tb_match* d_matches, const int32_t* d_match_counts, const float* d_kf_mp, const uint8_t* d_kf_valid,
                         const int32_t* d_kf_counts, const float* d_kf_Tcw, int pitch, const int32_t* d_cand_consensus, const uint8_t* d_inlier,
                         float* d_pts1, float* d_pts2, uint8_t* d_m1, uint8_t* d_m2, int32_t* d_wink, int32_t* d_skip, int32_t* d_fr1,
                         int32_t* d_fr2);
int tbk_sim3_search_merge(tb_ctx* ctx, int nseq, int ncand, int min_consensus, const int32_t* d_q_counts, int q_pitch, int pitch,
                          const tb_match* d_matches, const int32_t* d_wink, const int32_t* d_skip, const int32_t* d_match1,
                          const int32_t* d_match2, const tb_match* d_pairs, const int32_t* d_new_counts, const int32_t* d_stats,
                          const int32_t* d_cand_kf, const int32_t* d_cand_consensus, tb_match* d_wide, int32_t* d_wide_counts, int32_t* o_new,
                          int32_t* o_total, int32_t* o_stats, int32_t* b_new, int32_t* b_total);
/* two-view initialisation (k_two_view.hip): one workgroup per problem, no work buffer; every output nullable; pitch <= 2048 */
int tbk_two_view(tb_ctx* ctx, int nproblems, const float* d_xy0, const float* d_xy1, const int32_t* d_counts, const uint8_t* d_skip,
                 const float* d_inv_sigma2_0, const float* d_inv_sigma2_1, int pitch, const double K[4], const float* d_Tcw0,
                 const tb_two_view_params* prm, float* d_Tcw1, float* d_points, uint8_t* d_point_flags, uint8_t* d_inlier,
                 int32_t* d_consensus, int32_t* d_winner, int32_t* d_good, int32_t* d_tri, int32_t* d_status);
/* tb_two_view_batch_dev's parameter rules, for the entry points that store a parameter set */
static inline bool tb_two_view_params_ok(const tb_two_view_params* prm) {
    const bool ratios = prm->min_good_ratio > 0.0 && prm->min_good_ratio <= 1.0 && prm->ambiguity_ratio > 0.0 && prm->ambiguity_ratio <= 1.0;
    return prm->hypotheses >= 1 && prm->hypotheses <= 1024 && prm->chi2_epi >= 0.0 && std::isfinite(prm->chi2_epi) &&
           prm->tri.chi2_max >= 0.0 && std::isfinite(prm->tri.chi2_max) && std::isfinite(prm->tri.cos_parallax_max) && ratios &&
           prm->min_points >= 0 && prm->baseline > 0.0 && std::isfinite(prm->baseline);
}
/* the mono loop without a right image (k_vo.hip): before the keyframe's triangulation, a sequence that is not initialised leaves
 * it (tri_skip = 1) and becomes a two-view problem (tv_skip = !alive), an initialised one the other way round; after the
 * two-view call, the sequences that initialise adopt pose and points, and every attempt's results are kept */
int tbk_vo_init_prep(tb_ctx* ctx, int nseq, const uint8_t* d_initialised, const uint8_t* d_alive, int pitch, uint8_t* d_tri_skip,
                     uint8_t* d_tv_skip);
int tbk_vo_init_adopt(tb_ctx* ctx, int nseq, int t, int min_tracks, const int32_t* d_key_counts, const uint8_t* d_alive, int pitch,
                      const int32_t* d_w_res, const float* d_w_Tcw1, const float* d_points, const uint8_t* d_pflags,
                      uint8_t* d_initialised, int32_t* d_init_frame, int32_t* d_attempts, int32_t* d_res, float* d_Tcw1, float* d_Tcw,
                      float* d_tri_points, uint8_t* d_tri_flags);
/* PnP inside candidate verification (k_pnp.hip): the ordered gather of a pair's rows (stage 0: after the RANSAC, pose_a = the PnP
 * pose, pose_b = the stored seed; stage 1: expand, pose_a = the optimised pose) and the adoption of the second pose stage */
int tbk_pnp_gather(tb_ctx* ctx, int npairs, int stage, const double K[4], double chi2_max, int min_consensus, const tb_obs* d_rows0,
                   const int32_t* d_cnt0, int pitch, const uint8_t* d_mask, const int32_t* d_consensus, const float* d_pose_a,
                   const float* d_pose_b, uint8_t* d_took, tb_obs* d_rows, int32_t* d_cnt, uint8_t* d_outlier, float* d_seed,
                   int32_t* d_rows_out);
int tbk_pnp_adopt(tb_ctx* ctx, int npairs, const uint8_t* d_took, int pitch, const tb_obs* d_rows2, const int32_t* d_cnt2,
                  const uint8_t* d_outlier2, const float* d_pose2, const int32_t* d_ninl2, tb_obs* d_rows, int32_t* d_cnt, uint8_t* d_outlier,
                  float* d_pose, int32_t* d_ninl);
/* mono mode of the optical-flow loop (k_vo.hip): the alive / skip masks after a tracking half, and the keyframe's merge from
 * one side of the ping-pong (src) into the other (dst) */
#define TB_VO_MERGE_BITMAP_MAX 32768 /* bytes of LDS the merge's occupancy bitmap may take */
size_t tbk_vo_merge_bitmap_bytes(int width, int height, int cell);
int tbk_vo_mono_alive(tb_ctx* ctx, int nseq, const int32_t* d_key_counts, const uint8_t* d_status, const uint8_t* d_valid, int pitch,
                      uint8_t* d_alive, uint8_t* d_skip);
int tbk_vo_kf_merge(tb_ctx* ctx, int nseq, const tb_keypoint* d_orb, const int32_t* d_orb_counts, int orb_pitch, int pitch, int width,
                    int height, int cell, const float* d_src_keys, const int32_t* d_src_counts, const float* d_src_mp,
                    const uint8_t* d_src_valid, const float* d_tri_points, const uint8_t* d_tri_flags, float* d_keys,
                    int32_t* d_key_counts, float* d_mp, uint8_t* d_valid, float* d_kf_keys, uint8_t* d_alive, int32_t* d_survivors,
                    int32_t* d_added);


#endif
