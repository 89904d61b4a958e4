/* Host side of the device-resident stereo VO loop (test/test_vo.cpp test_kitti): the tb_vo_* entry points of include/tb_capi.h.
 * A step is launches and device-to-device copies on the context's stream; nothing is allocated per step and nothing is read back.
 * The operators it chains (extractor, matchers, pose optimisation, the keyframe database and store) are tb_capi.cpp's.
 */
#include "tb_internal.h"

#include <string.h>
#include <algorithm>
#include <cmath>
#include <memory>

extern "C" {

struct tb_vo {
    tb_ctx* ctx = nullptr;
    tb_vo_params p;
    int nseq = 0, P = 0;        /* sequences, key capacity (= the extractor's kp_capacity) */
    tb_extractor* ex = nullptr;
    tb_camera cam;              /* width / height: CameraModel::IsInFrame of both frames */
    int next = -1;              /* frame index of the next step (-1: not reset) */
    int cur = 0;                /* which half of the ping-pong buffers holds the last frame */
    tb_dev_owner own;           /* every device buffer below, the lazily allocated groups included */
    /* ping-pong state: the last frame's and the current frame's */
    uint8_t* img[2] = {nullptr, nullptr};    /* [nseq][h][w] left images */
    float* keys[2] = {nullptr, nullptr};     /* [nseq][P][2] */
    int32_t* kcnt[2] = {nullptr, nullptr};   /* [nseq] */
    float* mp[2] = {nullptr, nullptr};       /* [nseq][P][3] */
    uint8_t* valid[2] = {nullptr, nullptr};  /* [nseq][P] */
    float* Tcw[2] = {nullptr, nullptr};      /* [nseq][16] */
    /* The per-frame outputs that are not part of the ping-pong, [nseq] rows at pitch P (matches: Mcap): out[oc] is the set the
     * step writes and the state getters read. The second set is a ragged loop's (vo_ragged_init): a ragged step flips oc and
     * keeps the other set, what the last step left, for the hold. */
    tb_vo_frame_out out[2];
    int oc = 0;
    /* per-step work */
    uint8_t* right = nullptr;                /* [nseq][h][w] */
    uint8_t* status = nullptr;               /* [nseq][P] LK status of the tracking step */
    tb_match* lk_matches = nullptr;          /* [nseq][P] TB_VO_OPFLOW: searchByOPFlow's match list, which the loop does not read */
    int32_t* lk_mcounts = nullptr;           /* [nseq] */
    float* st_pts = nullptr;                 /* [nseq][P][2] stereo tracks */
    uint8_t* st_status = nullptr;            /* [nseq][P] */
    float* depth = nullptr;                  /* [nseq][P] */
    /* descriptor trackers (tr.kind != TB_VO_OPFLOW): the keyframe's snapshot of the current frame's outputs */
    tb_vo_tracker tr;
    float inv_sigma2[TB_MAX_LEVELS];         /* Frame::GetInverseScaleSigmaSquares */
    int32_t* win = nullptr;                  /* [nseq][P] k_vo_match_carry work */
    tb_vo_kf_out kf;
    int32_t* kf_cell_start = nullptr;        /* [nseq][TB_GRID_STARTS] violence: the keyframe's lookup grid */
    int32_t* kf_cell_items = nullptr;        /* [nseq][P] */
    int kf_frame = -1;
    /* projection trackers (TB_VO_PROJECTION, TB_VO_PROJECTION_MAP) */
    int Mcap = 0;                            /* match capacity: P, or the map's capacity */
    float sf[TB_MAX_LEVELS];                 /* Frame::GetScaleFactors */
    int32_t* cell_start = nullptr;           /* [nseq][TB_GRID_STARTS] the current frame's lookup grid */
    int32_t* cell_items = nullptr;           /* [nseq][P] */
    uint8_t* taken = nullptr;                /* [nseq][P] zero: Observations() is 0 throughout the loop */
    tb_mappoint* kf_rec = nullptr;           /* [nseq][P] TB_VO_PROJECTION: the keyframe's map points as the matcher reads them */
    /* the map (TB_VO_PROJECTION_MAP): two sets, eviction moves the survivors from one into the other */
    int mapK = 0, map_cap = 0, map_cur = 0, map_nblk = 0;   /* keyframes held, capacity, live set, blocks in use */
    tb_mappoint* map_rec[2] = {nullptr, nullptr};   /* [nseq][map_cap] */
    uint8_t* map_desc[2] = {nullptr, nullptr};      /* [nseq][map_cap][32] */
    int32_t* map_n[2] = {nullptr, nullptr};         /* [nseq] live counts */
    int32_t* map_blocks[2] = {nullptr, nullptr};    /* [nseq][mapK] points per held keyframe, oldest first */
    /* searchByBow (TB_VO_BOW): the borrowed vocabulary; Frame::SetBow's outputs are members of out[] and kf */
    tb_vo_bow bw;
    const tb_vocab* voc = nullptr;
    double* bow_wt = nullptr;                       /* [nseq][P] word weights of the current frame */
    tb_bow_db* db = nullptr;                        /* the keyframe database (tb_vo_bow_db_enable), owned */
    /* searchByNN (TB_VO_NN): the matcher's parameters and bit table, owned; ratio / minTh are tr.bf_ratio / tr.bf_min_th */
    tb_lsh* lsh = nullptr;
    /* relocalisation (tb_vo_reloc_enable): the keyframe store, owned, and the query's outputs a caller does not take */
    tb_kf_store* store = nullptr;
    double *rl_scores = nullptr, *rl_top_score = nullptr;   /* [nseq][capacity], [nseq][max_candidates] */
    /* rl_top_slot is shared scratch: the recovery and loop stages of a step overwrite it before they read it, and
     * tb_vo_relocalize_dev leaves the top_slot of its query in it (copied in when the caller took the output) for
     * tb_vo_relocalize_sim3_dev, which is why every step clears s3_slot */
    int32_t *rl_top_slot = nullptr, *rl_top_kf = nullptr;   /* [nseq][max_candidates] */
    const int32_t* s3_slot = nullptr;                       /* the top_slot of the tb_vo_relocalize_dev since the last step (null: none), */
    int s3_topk = 0;                                        /* and its topk: what tb_vo_relocalize_sim3_dev runs on */
    bool s3_done = false;                                   /* a tb_vo_relocalize_sim3_dev since the last step: tb_vo_loop_sim3_dev may run */
    /* recovery (tb_vo_recover_enable): the flags and the selection of the last step, the per-sequence tracking keyframe, the
     * masked candidates, and the rings of the keyframes' word / node ids, ring-aligned with the store */
    bool rec_on = false;
    tb_vo_recover rec;
    uint8_t* rc_lost = nullptr;                                          /* [nseq] */
    int32_t *rc_track = nullptr, *rc_kf = nullptr, *rc_kf_ids = nullptr; /* [nseq] */
    int32_t *rc_best_rank = nullptr, *rc_best_kf = nullptr;              /* [nseq] */
    float* rc_best_Tcw = nullptr;                                        /* [nseq][16] */
    int32_t* rc_masked = nullptr;                                        /* [nseq][topk] */
    int32_t *rc_word_ring = nullptr, *rc_node_ring = nullptr;            /* [nseq][capacity][P] */
    /* loop correction (tb_vo_loop_enable): per sequence a graph of cap + 1 nodes -- the stored keyframes, then the current frame
     * -- at edge pitch cap + 1, the solver's statistics and what the last keyframe step t > 0 closed */
    bool lp_on = false;
    tb_vo_loop lp;
    uint8_t* lp_closed = nullptr;                                        /* [nseq] */
    int32_t *lp_kf = nullptr, *lp_inl = nullptr, *lp_nnodes = nullptr, *lp_ecount = nullptr;   /* [nseq] */
    int32_t *lp_best_rank = nullptr, *lp_best_kf = nullptr;              /* [nseq] */
    float* lp_best_Tcw = nullptr;                                        /* [nseq][16] */
    int32_t* lp_node_kf = nullptr;                                       /* [nseq][cap + 1] */
    float *lp_before = nullptr, *lp_after = nullptr;                     /* [nseq][cap + 1][16] */
    tb_pg_edge* lp_edges = nullptr;                                      /* [nseq][cap + 1] */
    double* lp_stats = nullptr;                                          /* [nseq][8] */
    /* ragged batches (tb_vo_reset_seq_dev / tb_vo_step_ragged_dev): the per-sequence frame counters live on the host in both
     * modes; everything else is allocated by the first call that needs it (vo_ragged_init) */
    bool ragged = false;                            /* the sequences no longer share one frame counter */
    std::vector<int32_t> seq_frame, seq_kf_frame;   /* [nseq] last frame, frame of the keyframe (-1: none) */
    std::vector<uint8_t> seq_reset;                 /* [nseq] the sequence has been reset at least once */
    bool rg_ready = false;
    uint8_t* rg_left = nullptr;                     /* [nseq][h][w] the keyframe block's left images, compacted */
    float* rg_keys = nullptr;                       /* [nseq][P][2] its keys */
    int32_t* rg_kcnt = nullptr;                     /* [nseq] */
    int32_t* rg_dev = nullptr;                      /* [2][nseq] the step's mask and its keyframe index list */
    enum { RG_RING = 8 };
    int32_t* rg_pin = nullptr;                      /* [RG_RING][2][nseq] pinned staging; a slot is reused after its copy ran */
    hipEvent_t rg_ev[RG_RING] = {};
    unsigned rg_slot = 0;
    /* window BA (tb_vo_window_ba_enable, TB_VO_OPFLOW): the segment log since the last keyframe -- nslot = keyframe_every + 1
     * slots, slot 0 the keyframe -- the window built from it, and the copy of the segment the BA refines */
    bool wb_on = false;
    tb_vo_window_ba wb;
    int wb_nslot = 0, wb_slot = 0;                  /* slots; the slot the last step wrote (host counter: frames since the keyframe) */
    float* sg_keys = nullptr;                       /* [nseq][nslot][P][2] */
    uint8_t* sg_ok = nullptr;                       /* [nseq][nslot][P] */
    float* sg_pose = nullptr;                       /* [nseq][nslot][16] */
    float* sg_pts = nullptr;                        /* [nseq][P][3] */
    uint8_t* sg_spawned = nullptr;                  /* [nseq][P] */
    tb_ba_obs* wb_obs = nullptr;                    /* [nseq][nslot * P] */
    int32_t *wb_counts = nullptr, *wb_npts = nullptr;   /* [nseq] observations, contributing points */
    double* wb_stats = nullptr;                     /* [nseq][8] */
    float *wb_pose = nullptr, *wb_pts = nullptr;    /* [nseq][nslot][16], [nseq][P][3]: the last window, refined */
    uint8_t* wb_adopted = nullptr;                  /* [nseq] */
    /* mono mode (tb_vo_mono_enable, TB_VO_OPFLOW): the keyframe's key list and pose, which keys LK has held since, and the last
     * mono keyframe's triangulation and merge counts */
    bool mono_on = false;
    tb_vo_mono mono;
    float *mn_kf_keys = nullptr, *mn_kf_Tcw = nullptr;   /* [nseq][P][2], [nseq][16] */
    uint8_t *mn_alive = nullptr, *mn_skip = nullptr;     /* [nseq][P] */
    float* mn_tri_points = nullptr;                      /* [nseq][P][3] */
    uint8_t* mn_tri_flags = nullptr;                     /* [nseq][P] */
    int32_t *mn_tri_tally = nullptr, *mn_survivors = nullptr, *mn_added = nullptr;   /* [nseq][6], [nseq], [nseq] */
    /* the mono loop without a right image (tb_vo_mono_init_enable): which sequences are initialised, the two-view call's
     * outputs of the step (w_: the planes status, consensus, winner[2], good[4], tri[4], 12 ints a sequence) and every sequence's last attempt */
    bool mi_on = false;
    tb_vo_mono_init mi;
    uint8_t *mi_initialised = nullptr, *mi_skip = nullptr, *mi_pflags = nullptr;   /* [nseq], [nseq][P], [nseq][P] */
    int32_t *mi_init_frame = nullptr, *mi_attempts = nullptr;                     /* [nseq] */
    int32_t *mi_w_res = nullptr, *mi_res = nullptr;                               /* [nseq][12] */
    float *mi_w_Tcw1 = nullptr, *mi_Tcw1 = nullptr, *mi_points = nullptr;         /* [nseq][16], [nseq][16], [nseq][P][3] */
};

static bool vo_is_proj(const tb_vo* vo) { return vo->tr.kind == TB_VO_PROJECTION || vo->tr.kind == TB_VO_PROJECTION_MAP; }

void tb_vo_destroy(tb_vo* vo) {
    if (!vo) return;
    hipSetDevice(vo->ctx->device);
    hipStreamSynchronize(vo->ctx->stream);
    if (vo->ex) tb_extractor_destroy(vo->ex);
    tb_bow_db_destroy(vo->db);
    tb_kf_store_destroy(vo->store);
    tb_lsh_destroy(vo->lsh);
    vo->own.release();
    if (vo->rg_pin) hipHostFree(vo->rg_pin);
    for (hipEvent_t e : vo->rg_ev)
        if (e) hipEventDestroy(e);
    delete vo;
}

/* One set of per-frame outputs for the loop's tracker kind; the counts start at zero (and the carried descriptors: the hold
 * and the snapshot copy live entries only). */
static int vo_alloc_frame_out(tb_vo* vo, tb_vo_frame_out& o) {
    tb_ctx* ctx = vo->ctx;
    tb_dev_owner& own = vo->own;
    const size_t S = (size_t)vo->nseq, SP = S * vo->P;
    TB_TRY(tb_dev_alloc(ctx, own, &o.obs, SP));
    TB_TRY(tb_dev_alloc(ctx, own, &o.obs_counts, S, 0));
    TB_TRY(tb_dev_alloc(ctx, own, &o.outlier, SP));
    TB_TRY(tb_dev_alloc(ctx, own, &o.n_inliers, S, 0));
    if (vo->tr.kind == TB_VO_OPFLOW) return TB_OK;
    TB_TRY(tb_dev_alloc(ctx, own, &o.orb, SP));
    TB_TRY(tb_dev_alloc(ctx, own, &o.orb_desc, SP * 32));
    TB_TRY(tb_dev_alloc(ctx, own, &o.orb_cnt, S, 0));
    TB_TRY(tb_dev_alloc(ctx, own, &o.matches, S * (size_t)vo->Mcap));
    TB_TRY(tb_dev_alloc(ctx, own, &o.mcounts, S, 0));
    TB_TRY(tb_dev_alloc(ctx, own, &o.mflags, S, 0));
    if (vo_is_proj(vo)) TB_TRY(tb_dev_alloc(ctx, own, &o.mp_desc, SP * 32, 0));
    if (vo->tr.kind == TB_VO_BOW) {
        TB_TRY(tb_dev_alloc(ctx, own, &o.bow_word, SP));
        TB_TRY(tb_dev_alloc(ctx, own, &o.bow_node, SP));
        TB_TRY(tb_dev_alloc(ctx, own, &o.fv_keys, SP));
        TB_TRY(tb_dev_alloc(ctx, own, &o.fv_cnt, S, 0));
        TB_TRY(tb_dev_alloc(ctx, own, &o.bv_word, SP));
        TB_TRY(tb_dev_alloc(ctx, own, &o.bv_val, SP));
        TB_TRY(tb_dev_alloc(ctx, own, &o.bv_cnt, S, 0));
    }
    return TB_OK;
}

static int vo_create(tb_ctx* ctx, const tb_vo_params* p, const tb_vo_tracker* tr, int nseq, tb_vo** out, const tb_vo_bow* bow = nullptr,
                     const tb_vocab* voc = nullptr, const tb_vo_lsh* lsh = nullptr) {
    if (!ctx || !p || !out) return TB_EINVAL;
    *out = nullptr;
    if (nseq < 1 || p->width < 1 || p->height < 1 || p->nlevels < 2 || p->nlevels > TB_MAX_LEVELS || !(p->scale > 0.f && p->scale < 1.f) ||
        p->target < 1 || p->keyframe_every < 1 || !(p->K[0] > 0.0) || !(p->K[1] > 0.0) || !std::isfinite(p->K[2]) ||
        !std::isfinite(p->K[3]) || !(p->bf > 0.f) || !std::isfinite(p->bf))
        return tb_fail(ctx, TB_EINVAL, "tb_vo_create: bad parameters (nseq %d, %dx%d, %d levels, scale %g, target %d, keyframe_every %d)",
                       nseq, p->width, p->height, p->nlevels, (double)p->scale, p->target, p->keyframe_every);
    std::vector<float> sf(p->nlevels), tmp(p->nlevels);
    tb_scale_factors(p->nlevels, p->scale, sf.data(), tmp.data(), tmp.data(), tmp.data());
    std::unique_ptr<tb_vo, void (*)(tb_vo*)> vu(new tb_vo(), tb_vo_destroy);
    tb_vo* vo = vu.get();
    vo->ctx = ctx;
    vo->p = *p;
    vo->nseq = nseq;
    vo->seq_frame.assign(nseq, -1); vo->seq_kf_frame.assign(nseq, -1); vo->seq_reset.assign(nseq, 0);
    memset(&vo->tr, 0, sizeof vo->tr);
    if (tr) vo->tr = *tr;
    memset(&vo->bw, 0, sizeof vo->bw);
    if (bow) { vo->bw = *bow; vo->voc = voc; }
    int rc = tb_extractor_create(ctx, p->width, p->height, p->nlevels, sf.data(), nullptr, nullptr, nseq, p->target, &vo->ex);
    if (rc) return rc;
    vo->P = vo->ex->g.selCap;
    vo->Mcap = vo->P;
    if (bow && vo->P > 8192)
        return tb_fail(ctx, TB_EUNSUPPORTED, "tb_vo_create_bow: %d keys per frame (the transform sorts at most 8192)", vo->P);
    if (lsh) {
        if (vo->P > 8192) return tb_fail(ctx, TB_EUNSUPPORTED, "tb_vo_create_lsh: %d keys per frame (searchByNN takes sets of at most 8192)", vo->P);
        TB_TRY(tb_lsh_create(ctx, lsh->tables, lsh->key_size, lsh->multi_probe_level, lsh->seed, lsh->bits, &vo->lsh));
    }
    if (vo->tr.kind == TB_VO_PROJECTION_MAP) {
        if ((size_t)vo->tr.map_keyframes * (size_t)vo->P > (size_t)INT32_MAX / 64)
            return tb_fail(ctx, TB_EINVAL, "tb_vo_create_ex: map_keyframes %d x %d keys is too large", vo->tr.map_keyframes, vo->P);
        vo->mapK = vo->tr.map_keyframes;
        vo->map_cap = vo->Mcap = vo->mapK * vo->P;
    }
    memset(&vo->cam, 0, sizeof vo->cam);
    vo->cam.fx = (float)p->K[0]; vo->cam.fy = (float)p->K[1]; vo->cam.cx = (float)p->K[2]; vo->cam.cy = (float)p->K[3];
    vo->cam.width = p->width; vo->cam.height = p->height;
    tb_dev_owner& own = vo->own;
    const size_t S = (size_t)nseq, P = (size_t)vo->P, SP = S * P, img = (size_t)p->width * p->height;
    for (int k = 0; k < 2; k++) {
        TB_TRY(tb_dev_alloc(ctx, own, &vo->img[k], S * img));
        TB_TRY(tb_dev_alloc(ctx, own, &vo->keys[k], SP * 2));
        TB_TRY(tb_dev_alloc(ctx, own, &vo->kcnt[k], S, 0));
        TB_TRY(tb_dev_alloc(ctx, own, &vo->mp[k], SP * 3));
        TB_TRY(tb_dev_alloc(ctx, own, &vo->valid[k], SP, 0));
        TB_TRY(tb_dev_alloc(ctx, own, &vo->Tcw[k], S * 16));
    }
    TB_TRY(vo_alloc_frame_out(vo, vo->out[0]));
    TB_TRY(tb_dev_alloc(ctx, own, &vo->right, S * img));
    TB_TRY(tb_dev_alloc(ctx, own, &vo->status, SP));
    TB_TRY(tb_dev_alloc(ctx, own, &vo->st_pts, SP * 2));
    TB_TRY(tb_dev_alloc(ctx, own, &vo->st_status, SP));
    TB_TRY(tb_dev_alloc(ctx, own, &vo->depth, SP));
    /* every scratch slot the step's operators use, at its largest size now: a step never grows one (growth synchronises) */
    const size_t pitch = img;
    void* d;
    if ((rc = tb_scratch(ctx, TB_SLOT_OPFLOW_EQ, S * pitch, &d)) || (rc = tb_scratch(ctx, TB_SLOT_WORK, S * 8 * 8 * 256, &d)) ||
        (rc = tb_scratch(ctx, TB_SLOT_LK, std::max(tbk_lk_work_bytes(p->width, p->height, 3, nseq), SP * 3 * sizeof(double)), &d)) ||
        (rc = tb_scratch(ctx, TB_SLOT_RANSAC, tbk_ransac_work_bytes(nseq, vo->P), &d)) || (rc = tb_scratch(ctx, TB_SLOT_RANSAC_FLAGS, S * sizeof(int32_t), &d)) ||
        (rc = tb_scratch(ctx, TB_SLOT_STEREO_MATCHES, SP * sizeof(tb_match), &d)) || (rc = tb_scratch(ctx, TB_SLOT_STEREO_COUNTS, S * sizeof(int32_t), &d)))
        return rc;
    if (vo->tr.kind == TB_VO_OPFLOW) {
        TB_TRY(tb_dev_alloc(ctx, own, &vo->lk_matches, SP));
        TB_TRY(tb_dev_alloc(ctx, own, &vo->lk_mcounts, S));
    } else {
        tb_scale_factors(p->nlevels, p->scale, tmp.data(), nullptr, nullptr, vo->inv_sigma2);
        tb_vo_kf_out& kf = vo->kf;
        TB_TRY(tb_dev_alloc(ctx, own, &vo->win, SP));
        TB_TRY(tb_dev_alloc(ctx, own, &kf.orb, SP));
        TB_TRY(tb_dev_alloc(ctx, own, &kf.desc, SP * 32));
        TB_TRY(tb_dev_alloc(ctx, own, &kf.cnt, S, 0));
        TB_TRY(tb_dev_alloc(ctx, own, &kf.mp, SP * 3));
        TB_TRY(tb_dev_alloc(ctx, own, &kf.valid, SP));
        /* an all-zero table is an empty grid: a ragged step runs the matcher for sequences that have no keyframe yet */
        TB_TRY(tb_dev_alloc(ctx, own, &vo->kf_cell_start, S * TB_GRID_STARTS, 0));
        TB_TRY(tb_dev_alloc(ctx, own, &vo->kf_cell_items, SP));
        /* the matcher's slots: searchByBF's best rows per side, searchByViolence's (WORK, shared with CLAHE) */
        if (vo->tr.kind == TB_VO_BF) {
            if ((rc = tb_scratch(ctx, TB_SLOT_BF_TRAIN, SP * 8, &d)) || (rc = tb_scratch(ctx, TB_SLOT_BF_QUERY, SP * 8, &d))) return rc;
        } else if (vo->tr.kind == TB_VO_NN) {
            if ((rc = tb_scratch(ctx, TB_SLOT_BF_QUERY, SP * 8, &d))) return rc;   /* searchByNN's best row per query */
        } else if (vo_is_proj(vo)) {
            /* the projection matchers' best rows: 6 words per map point */
            if ((rc = tb_scratch(ctx, TB_SLOT_WORK, S * (size_t)vo->Mcap * 6 * sizeof(int32_t), &d))) return rc;
        } else if ((rc = tb_scratch(ctx, TB_SLOT_WORK, SP * 16, &d))) {
            return rc;
        }
    }
    if (bow) {
        /* every output of the transform is a buffer of the loop, so tb_bow_transform_batch_dev takes no scratch; the matcher's
         * best rows (WORK) were sized above */
        tb_vo_kf_out& kf = vo->kf;
        TB_TRY(tb_dev_alloc(ctx, own, &vo->bow_wt, SP));
        TB_TRY(tb_dev_alloc(ctx, own, &kf.bow_word, SP));
        TB_TRY(tb_dev_alloc(ctx, own, &kf.bow_node, SP));
        TB_TRY(tb_dev_alloc(ctx, own, &kf.fv_keys, SP));
        TB_TRY(tb_dev_alloc(ctx, own, &kf.fv_cnt, S, 0));
        TB_TRY(tb_dev_alloc(ctx, own, &kf.bv_word, SP));
        TB_TRY(tb_dev_alloc(ctx, own, &kf.bv_val, SP));
        TB_TRY(tb_dev_alloc(ctx, own, &kf.bv_cnt, S, 0));
    }
    if (vo_is_proj(vo)) {
        for (int l = 0; l < p->nlevels; l++) vo->sf[l] = sf[l];
        TB_TRY(tb_dev_alloc(ctx, own, &vo->cell_start, S * TB_GRID_STARTS));
        TB_TRY(tb_dev_alloc(ctx, own, &vo->cell_items, SP));
        TB_TRY(tb_dev_alloc(ctx, own, &vo->taken, SP, 0));
        TB_TRY(tb_dev_alloc(ctx, own, &vo->kf.mp_desc, SP * 32, 0));
        if (vo->tr.kind == TB_VO_PROJECTION) {
            TB_TRY(tb_dev_alloc(ctx, own, &vo->kf_rec, SP));
        } else {
            const size_t C = (size_t)vo->map_cap;
            for (int k = 0; k < 2; k++) {
                TB_TRY(tb_dev_alloc(ctx, own, &vo->map_rec[k], S * C));
                TB_TRY(tb_dev_alloc(ctx, own, &vo->map_desc[k], S * C * 32));
                TB_TRY(tb_dev_alloc(ctx, own, &vo->map_n[k], S, 0));
                TB_TRY(tb_dev_alloc(ctx, own, &vo->map_blocks[k], S * vo->mapK, 0));
            }
        }
    }
    *out = vu.release();
    return TB_OK;
}

int tb_vo_create(tb_ctx* ctx, const tb_vo_params* p, int nseq, tb_vo** out) {
    TB_ENTER(ctx);
    return vo_create(ctx, p, nullptr, nseq, out);
}

int tb_vo_create_ex(tb_ctx* ctx, const tb_vo_params* p, const tb_vo_tracker* tr, int nseq, tb_vo** out) {
    TB_ENTER(ctx);
    if (!ctx || !p || !out) return TB_EINVAL;
    *out = nullptr;
    if (tr && tr->kind != TB_VO_OPFLOW) {
        if (tr->kind == TB_VO_BOW) return tb_fail(ctx, TB_EINVAL, "tb_vo_create_ex: TB_VO_BOW needs a vocabulary, use tb_vo_create_bow");
        if (tr->kind == TB_VO_NN) return tb_fail(ctx, TB_EINVAL, "tb_vo_create_ex: TB_VO_NN needs the LSH parameters, use tb_vo_create_lsh");
        if (tr->kind != TB_VO_BF && tr->kind != TB_VO_VIOLENCE && tr->kind != TB_VO_PROJECTION && tr->kind != TB_VO_PROJECTION_MAP)
            return tb_fail(ctx, TB_EINVAL, "tb_vo_create_ex: unknown tracker kind %d", tr->kind);
        if (tr->kind == TB_VO_PROJECTION || tr->kind == TB_VO_PROJECTION_MAP) {
            const bool map = tr->kind == TB_VO_PROJECTION_MAP;
            if (tr->th_high < 0 || tr->histo_len < 1 || tr->histo_len > 1024 || !std::isfinite(tr->nratio) ||
                (map && (tr->map_keyframes < 1 || !std::isfinite(tr->radio))))
                return tb_fail(ctx, TB_EINVAL, "tb_vo_create_ex: searchByProjection arguments (nratio %g, th_high %d, histo_len %d, radio %g, map_keyframes %d)",
                               (double)tr->nratio, tr->th_high, tr->histo_len, (double)tr->radio, tr->map_keyframes);
        } else if (tr->kind == TB_VO_BF) {
            if (!std::isfinite(tr->bf_ratio) || !std::isfinite(tr->bf_min_th))
                return tb_fail(ctx, TB_EINVAL, "tb_vo_create_ex: searchByBF ratio / minTh must be finite");
            /* matcher.cpp:177: only MinLevel == 0 && MaxLevel == F1->GetMaxLevel() (= nLevels) takes the whole-set branch */
            if (tr->min_level != 0 || tr->max_level != p->nlevels)
                return tb_fail(ctx, TB_EUNSUPPORTED, "tb_vo_create_ex: searchByBF levels (%d, %d): only the whole-set branch (0, %d) exists",
                               tr->min_level, tr->max_level, p->nlevels);
        } else if (tr->histo_len < 1 || tr->histo_len > 1024 || !(tr->radius > 0.f) || !std::isfinite(tr->radius) ||
                   tr->min_level > tr->max_level || !std::isfinite(tr->nratio)) {
            return tb_fail(ctx, TB_EINVAL, "tb_vo_create_ex: searchByViolence arguments (levels %d..%d, radius %g, histo_len %d)",
                           tr->min_level, tr->max_level, (double)tr->radius, tr->histo_len);
        }
    }
    return vo_create(ctx, p, tr && tr->kind != TB_VO_OPFLOW ? tr : nullptr, nseq, out);
}

int tb_vo_create_bow(tb_ctx* ctx, const tb_vo_params* p, const tb_vo_bow* bow, const tb_vocab* voc, int nseq, tb_vo** out) {
    TB_ENTER(ctx);
    if (out) *out = nullptr;
    if (!p || !out || !bow) return TB_EINVAL;
    if (bow->histo_len < 1 || bow->histo_len > 1024 || bow->levelsup < 0 || bow->th_low < 0 || !std::isfinite(bow->nratio)) {
        if (!ctx) return TB_EINVAL;
        return tb_fail(ctx, TB_EINVAL, "tb_vo_create_bow: searchByBow arguments (levelsup %d, th_low %d, nratio %g, histo_len %d)",
                       bow->levelsup, bow->th_low, (double)bow->nratio, bow->histo_len);
    }
    if (!ctx) return TB_EINVAL;
    if (!voc || voc->ctx != ctx) return tb_fail(ctx, TB_EINVAL, "tb_vo_create_bow: a vocabulary of this context is required");
    if (voc->weighting < 0 || voc->weighting > 3 || voc->scoring < 0 || voc->scoring > 5)
        return tb_fail(ctx, TB_EINVAL, "tb_vo_create_bow: the vocabulary's weighting %d / scoring %d", voc->weighting, voc->scoring);
    tb_vo_tracker tr;
    memset(&tr, 0, sizeof tr);
    tr.kind = TB_VO_BOW;
    tr.th_low = bow->th_low; tr.nratio = bow->nratio; tr.histo_len = bow->histo_len; tr.check_orientation = bow->check_orientation;
    return vo_create(ctx, p, &tr, nseq, out, bow, voc);
}

int tb_vo_create_lsh(tb_ctx* ctx, const tb_vo_params* p, const tb_vo_lsh* lsh, int nseq, tb_vo** out) {
    TB_ENTER(ctx);
    if (out) *out = nullptr;
    if (!ctx || !p || !out || !lsh) return TB_EINVAL;
    if (!std::isfinite(lsh->ratio) || !std::isfinite(lsh->min_th))
        return tb_fail(ctx, TB_EINVAL, "tb_vo_create_lsh: searchByNN ratio / minTh must be finite");
    if (lsh->tables < 1 || lsh->tables > 32 || lsh->key_size < 1 || lsh->key_size > 32 || lsh->multi_probe_level < 0 ||
        lsh->multi_probe_level > lsh->key_size)
        return tb_fail(ctx, TB_EINVAL, "tb_vo_create_lsh: tables %d (1..32), key_size %d (1..32), multi_probe_level %d (0..key_size)",
                       lsh->tables, lsh->key_size, lsh->multi_probe_level);
    /* matcher.cpp:45: only MinLevel == 0 && MaxLevel == F1->GetMaxLevel() (= nLevels) takes the whole-set branch */
    if (lsh->min_level != 0 || lsh->max_level != p->nlevels)
        return tb_fail(ctx, TB_EUNSUPPORTED, "tb_vo_create_lsh: searchByNN levels (%d, %d): only the whole-set branch (0, %d) exists",
                       lsh->min_level, lsh->max_level, p->nlevels);
    tb_vo_tracker tr;
    memset(&tr, 0, sizeof tr);
    tr.kind = TB_VO_NN;
    tr.bf_ratio = lsh->ratio; tr.bf_min_th = lsh->min_th; tr.min_level = lsh->min_level; tr.max_level = lsh->max_level;
    return vo_create(ctx, p, &tr, nseq, out, nullptr, nullptr, lsh);
}

static int vo_recover_clear(tb_vo* vo);
static int vo_loop_clear(tb_vo* vo);
static int vo_window_clear(tb_vo* vo);
static int vo_mono_clear(tb_vo* vo);
static int vo_mono_init_clear(tb_vo* vo);
static int vo_extract(tb_vo* vo, const uint8_t* images, int n);

int tb_vo_reset_dev(tb_vo* vo, const float* Tcw0) {
    TB_ENTER((vo ? vo->ctx : nullptr));
    if (!vo || !Tcw0) return TB_EINVAL;
    tb_ctx* ctx = vo->ctx;
    /* frame 0 reads the "last frame": no keys, pose Tcw0 */
    TB_HIP(ctx, hipMemcpyAsync(vo->Tcw[vo->cur], Tcw0, (size_t)vo->nseq * 16 * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->kcnt[vo->cur], 0, (size_t)vo->nseq * sizeof(int32_t), ctx->stream));
    if (vo->tr.kind != TB_VO_OPFLOW) {   /* no keyframe yet */
        TB_HIP(ctx, hipMemsetAsync(vo->kf.cnt, 0, (size_t)vo->nseq * sizeof(int32_t), ctx->stream));
        vo->kf_frame = -1;
    }
    if (vo->tr.kind == TB_VO_BOW) {
        TB_HIP(ctx, hipMemsetAsync(vo->kf.fv_cnt, 0, (size_t)vo->nseq * sizeof(int32_t), ctx->stream));
        TB_HIP(ctx, hipMemsetAsync(vo->kf.bv_cnt, 0, (size_t)vo->nseq * sizeof(int32_t), ctx->stream));
        if (vo->db) TB_TRY(tb_bow_db_clear(vo->db));   /* a new run: no keyframes yet */
        if (vo->store) TB_TRY(tb_kf_store_clear(vo->store));
        if (vo->rec_on) TB_TRY(vo_recover_clear(vo));
        if (vo->lp_on) TB_TRY(vo_loop_clear(vo));
    }
    if (vo->mapK) {   /* an empty map */
        TB_HIP(ctx, hipMemsetAsync(vo->map_n[vo->map_cur], 0, (size_t)vo->nseq * sizeof(int32_t), ctx->stream));
        TB_HIP(ctx, hipMemsetAsync(vo->map_blocks[vo->map_cur], 0, (size_t)vo->nseq * vo->mapK * sizeof(int32_t), ctx->stream));
        vo->map_nblk = 0;
    }
    if (vo->wb_on) TB_TRY(vo_window_clear(vo));
    if (vo->mono_on) TB_TRY(vo_mono_clear(vo));
    if (vo->mi_on) TB_TRY(vo_mono_init_clear(vo));
    vo->next = 0;
    vo->s3_slot = nullptr;
    vo->s3_done = false;
    vo->ragged = false;
    std::fill(vo->seq_frame.begin(), vo->seq_frame.end(), -1);
    std::fill(vo->seq_kf_frame.begin(), vo->seq_kf_frame.end(), -1);
    std::fill(vo->seq_reset.begin(), vo->seq_reset.end(), 1);
    return TB_OK;
}

/* the recovery state of a new run: nothing flagged, nothing adopted, no tracking keyframe */
static int vo_recover_clear(tb_vo* vo) {
    tb_ctx* ctx = vo->ctx;
    const size_t S = (size_t)vo->nseq;
    TB_HIP(ctx, hipMemsetAsync(vo->rc_lost, 0, S, ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->rc_track, 0, S * sizeof(int32_t), ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->rc_kf, 0xff, S * sizeof(int32_t), ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->rc_kf_ids, 0xff, S * sizeof(int32_t), ctx->stream));
    return TB_OK;
}

/* the loop-correction state of a new run: nothing closed, no graph */
static int vo_loop_clear(tb_vo* vo) {
    tb_ctx* ctx = vo->ctx;
    const size_t S = (size_t)vo->nseq, nn = (size_t)vo->store->cap + 1;
    TB_HIP(ctx, hipMemsetAsync(vo->lp_closed, 0, S, ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->lp_kf, 0xff, S * sizeof(int32_t), ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->lp_inl, 0, S * sizeof(int32_t), ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->lp_nnodes, 0, S * sizeof(int32_t), ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->lp_ecount, 0, S * sizeof(int32_t), ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->lp_node_kf, 0xff, S * nn * sizeof(int32_t), ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->lp_before, 0, S * nn * 16 * sizeof(float), ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->lp_after, 0, S * nn * 16 * sizeof(float), ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->lp_edges, 0, S * nn * sizeof(tb_pg_edge), ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->lp_stats, 0, S * 8 * sizeof(double), ctx->stream));
    return TB_OK;
}

/* the window-BA state of a new run: an empty log, an empty window, nothing adopted */
static int vo_window_clear(tb_vo* vo) {
    tb_ctx* ctx = vo->ctx;
    const size_t S = (size_t)vo->nseq, P = (size_t)vo->P, N = (size_t)vo->wb_nslot;
    TB_HIP(ctx, hipMemsetAsync(vo->sg_keys, 0, S * N * P * 2 * sizeof(float), ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->sg_ok, 0, S * N * P, ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->sg_pose, 0, S * N * 16 * sizeof(float), ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->sg_pts, 0, S * P * 3 * sizeof(float), ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->sg_spawned, 0, S * P, ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->wb_obs, 0, S * N * P * sizeof(tb_ba_obs), ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->wb_counts, 0, S * sizeof(int32_t), ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->wb_npts, 0, S * sizeof(int32_t), ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->wb_stats, 0, S * 8 * sizeof(double), ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->wb_pose, 0, S * N * 16 * sizeof(float), ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->wb_pts, 0, S * P * 3 * sizeof(float), ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->wb_adopted, 0, S, ctx->stream));
    vo->wb_slot = 0;
    return TB_OK;
}

/* the mono state of a new run: no keyframe yet, nothing triangulated */
static int vo_mono_clear(tb_vo* vo) {
    tb_ctx* ctx = vo->ctx;
    const size_t S = (size_t)vo->nseq, SP = S * vo->P;
    TB_HIP(ctx, hipMemsetAsync(vo->mn_kf_keys, 0, SP * 2 * sizeof(float), ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->mn_kf_Tcw, 0, S * 16 * sizeof(float), ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->mn_alive, 0, SP, ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->mn_skip, 1, SP, ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->mn_tri_points, 0, SP * 3 * sizeof(float), ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->mn_tri_flags, 0, SP, ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->mn_tri_tally, 0, S * 6 * sizeof(int32_t), ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->mn_survivors, 0, S * sizeof(int32_t), ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->mn_added, 0, S * sizeof(int32_t), ctx->stream));
    return TB_OK;
}

/* the state of a new run without a right image: nothing initialised, no attempt yet */
static int vo_mono_init_clear(tb_vo* vo) {
    tb_ctx* ctx = vo->ctx;
    const size_t S = (size_t)vo->nseq;
    TB_HIP(ctx, hipMemsetAsync(vo->mi_initialised, 0, S, ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->mi_init_frame, 0xff, S * sizeof(int32_t), ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->mi_attempts, 0, S * sizeof(int32_t), ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->mi_res, 0, S * 12 * sizeof(int32_t), ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->mi_Tcw1, 0, S * 16 * sizeof(float), ctx->stream));
    return TB_OK;
}

/* Mono mode, the end of frame 0's stereo keyframe block: the key list and pose the next segment triangulates against. */
static int vo_mono_start(tb_vo* vo, int b) {
    tb_ctx* ctx = vo->ctx;
    const size_t S = (size_t)vo->nseq, SP = S * vo->P;
    TB_HIP(ctx, hipMemcpyAsync(vo->mn_kf_keys, vo->keys[b], SP * 2 * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    TB_HIP(ctx, hipMemcpyAsync(vo->mn_kf_Tcw, vo->Tcw[b], S * 16 * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->mn_alive, 1, SP, ctx->stream));
    return TB_OK;
}

/* Mono mode, the keyframe block of frame t > 0 (include/tb_capi.h, tb_vo_mono): triangulate the segment's tracks at the
 * optimised pose, then merge the keys that have a map point with the frame's ORB keys. The merge reads side b and writes side
 * a, which nothing needs any more; the two sides of the key list, its counts and its map points then change places, so side b
 * is the frame's again. */
static int vo_mono_keyframe(tb_vo* vo, int b, int t) {
    tb_ctx* ctx = vo->ctx;
    const tb_vo_params& p = vo->p;
    const int S = vo->nseq, P = vo->P, a = b ^ 1;
    const tb_triangulate_params tp = {vo->mono.cos_parallax_max, vo->mono.chi2_max};
    if (vo->mi_on) TB_TRY(tbk_vo_init_prep(ctx, S, vo->mi_initialised, vo->mn_alive, P, vo->mn_skip, vo->mi_skip));
    TB_TRY(tb_linear_triangle_batch_dev(ctx, S, vo->mn_kf_keys, vo->keys[b], vo->kcnt[b], P, vo->mn_kf_Tcw, vo->Tcw[b], p.K, nullptr, nullptr,
                                        vo->mn_skip, &tp, vo->mn_tri_points, vo->mn_tri_flags, vo->mn_tri_tally));
    if (vo->mi_on) {   /* the sequences that are not initialised yet: a pose and first points from the segment's tracks alone */
        int32_t* w = vo->mi_w_res;   /* planes: status [S], consensus [S], winner [S][2], good [S][4], tri [S][4] */
        TB_TRY(tbk_two_view(ctx, S, vo->mn_kf_keys, vo->keys[b], vo->kcnt[b], vo->mi_skip, nullptr, nullptr, P, p.K, vo->mn_kf_Tcw,
                            &vo->mi.two_view, vo->mi_w_Tcw1, vo->mi_points, vo->mi_pflags, nullptr, w + (size_t)S, w + 2 * (size_t)S,
                            w + 4 * (size_t)S, w + 8 * (size_t)S, w));
        TB_TRY(tbk_vo_init_adopt(ctx, S, t, vo->mi.min_tracks, vo->kcnt[b], vo->mn_alive, P, w, vo->mi_w_Tcw1, vo->mi_points, vo->mi_pflags,
                                 vo->mi_initialised, vo->mi_init_frame, vo->mi_attempts, vo->mi_res, vo->mi_Tcw1, vo->Tcw[b],
                                 vo->mn_tri_points, vo->mn_tri_flags));
    }
    TB_TRY(vo_extract(vo, vo->img[b], S));
    const tb_keypoint* kps = nullptr; const int32_t* cnt = nullptr; int selCap = 0;
    tb_extractor_results_dev(vo->ex, &kps, nullptr, &cnt, &selCap);
    TB_TRY(tbk_vo_kf_merge(ctx, S, kps, cnt, selCap, P, p.width, p.height, vo->mono.cell, vo->keys[b], vo->kcnt[b], vo->mp[b], vo->valid[b],
                           vo->mn_tri_points, vo->mn_tri_flags, vo->keys[a], vo->kcnt[a], vo->mp[a], vo->valid[a], vo->mn_kf_keys,
                           vo->mn_alive, vo->mn_survivors, vo->mn_added));
    std::swap(vo->keys[a], vo->keys[b]); std::swap(vo->kcnt[a], vo->kcnt[b]);
    std::swap(vo->mp[a], vo->mp[b]); std::swap(vo->valid[a], vo->valid[b]);
    TB_HIP(ctx, hipMemcpyAsync(vo->mn_kf_Tcw, vo->Tcw[b], (size_t)S * 16 * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    return TB_OK;
}

/* The window BA of keyframe step t > 0 (include/tb_capi.h, tb_vo_window_ba), after the step's own slot was logged and before
 * the keyframe block: build the window, refine a copy of the segment, adopt the last slot's pose into side b. The BA call
 * synchronises the stream once -- the one host synchronisation the feature adds, on keyframe steps only. */
static int vo_window_ba(tb_vo* vo, int b) {
    tb_ctx* ctx = vo->ctx;
    const int S = vo->nseq, P = vo->P, N = vo->wb_nslot;
    TB_TRY(tbk_vo_seg_window(ctx, S, vo->sg_keys, vo->sg_ok, P, N, vo->wb.min_obs, vo->wb_obs, vo->wb_counts, vo->wb_npts));
    TB_HIP(ctx, hipMemcpyAsync(vo->wb_pose, vo->sg_pose, (size_t)S * N * 16 * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    TB_HIP(ctx, hipMemcpyAsync(vo->wb_pts, vo->sg_pts, (size_t)S * P * 3 * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    TB_TRY(tb_local_ba_batch_dev(ctx, S, vo->p.K, N, vo->wb.fixed, vo->wb_pose, P, vo->wb_pts, vo->wb_obs, vo->wb_counts, N * P, vo->wb.iters,
                                 vo->wb_stats));
    return tbk_vo_seg_adopt(ctx, S, vo->wb_pose, vo->wb_npts, vo->wb_stats, N, vo->wb.min_points, vo->Tcw[b], vo->wb_adopted);
}

/* searchByBow's arguments as candidate verification takes them */
static tb_reloc_params vo_reloc_params(const tb_vo* vo, int min_inliers) {
    tb_reloc_params prm;
    prm.map_point_only = vo->bw.map_point_only; prm.th_low = vo->bw.th_low; prm.nratio = vo->bw.nratio; prm.histo_len = vo->bw.histo_len;
    prm.check_orientation = vo->bw.check_orientation; prm.min_inliers = min_inliers;
    return prm;
}

/* The recovery stage of frame t > 0 (include/tb_capi.h, tb_vo_recover): flag, query, mask, verify, adopt, switch the tracking
 * keyframe. Every launch is on the context's stream; which sequences adopt is decided on the device. */
static int vo_recover_stage(tb_vo* vo, int b) {
    tb_ctx* ctx = vo->ctx;
    tb_kf_store* st = vo->store;
    tb_bow_db* db = vo->db;
    const tb_vo_recover& r = vo->rec;
    const tb_vo_frame_out& o = vo->out[vo->oc];
    const tb_vo_kf_out& kf = vo->kf;
    if (st->pnp_on) return tb_fail(ctx, TB_ESTATE, "recovery on a store with PnP verification (enabled on the lent store): not combined yet");
    const int S = vo->nseq, P = vo->P;
    TB_TRY(tb_bow_db_query_dev(db, o.bv_word, o.bv_val, o.bv_cnt, P, r.exclude_newest, r.topk, vo->rl_scores, vo->rl_top_slot, vo->rl_top_kf,
                               vo->rl_top_score, nullptr));
    TB_TRY(tbk_vo_recover_mask(ctx, S, r.topk, r.lost_inliers, o.n_inliers, vo->rl_top_slot, vo->rc_lost, vo->rc_track, vo->rc_masked));
    const tb_reloc_params prm = vo_reloc_params(vo, r.min_inliers);
    tb_reloc_out out = {};
    out.best_rank = vo->rc_best_rank; out.best_kf = vo->rc_best_kf; out.best_Tcw = vo->rc_best_Tcw;
    TB_TRY(tb_relocalize_batch_dev(st, vo->p.K, vo->p.nlevels, vo->p.scale, o.orb, o.orb_desc, o.orb_cnt, o.fv_keys, o.fv_cnt, P, vo->rc_masked,
                                   r.topk, &prm, &out));
    tb_vo_recover_args a;
    a.topk = r.topk; a.pitch = P;
    a.lost = vo->rc_lost; a.best_rank = vo->rc_best_rank; a.best_kf = vo->rc_best_kf; a.ix2 = st->ix2; a.best_Tcw = vo->rc_best_Tcw;
    a.w_matches = st->matches; a.w_obs = st->obs; a.w_outlier = st->outlier; a.w_mcounts = st->mcounts; a.w_flags = st->flags;
    a.w_ocounts = st->ocounts; a.w_ninl = st->ninl;
    a.s_keys = st->keys; a.s_desc = st->desc; a.s_fv = (const unsigned long long*)st->fv; a.s_mp = st->mp; a.s_valid = st->valid;
    a.s_counts = st->counts; a.s_fv_counts = st->fv_counts;
    a.db_words = db->words; a.db_values = db->values; a.db_counts = db->counts;
    a.word_ring = vo->rc_word_ring; a.node_ring = vo->rc_node_ring;
    a.orb_counts = o.orb_cnt;
    a.Tcw = vo->Tcw[b]; a.mp = vo->mp[b]; a.valid = vo->valid[b]; a.obs = o.obs; a.outlier = o.outlier; a.matches = o.matches;
    a.obs_counts = o.obs_counts; a.n_inliers = o.n_inliers; a.mcounts = o.mcounts; a.mflags = o.mflags; a.recovered_kf = vo->rc_kf;
    a.kf_orb = kf.orb; a.kf_desc = kf.desc; a.kf_fv = (unsigned long long*)kf.fv_keys; a.kf_mp = kf.mp;
    a.kf_valid = kf.valid; a.kf_cnt = kf.cnt; a.kf_fv_cnt = kf.fv_cnt;
    a.kf_bv_word = kf.bv_word; a.kf_bv_val = kf.bv_val; a.kf_bv_cnt = kf.bv_cnt;
    a.kf_word = kf.bow_word; a.kf_node = kf.bow_node; a.kf_ids = vo->rc_kf_ids;
    TB_TRY(tbk_vo_recover_adopt(ctx, S, &a));
    return tbk_vo_recover_switch(ctx, S, &a);
}

/* The loop-correction stage of a keyframe step t > 0 (include/tb_capi.h, tb_vo_loop), between the tracking step's pose and the
 * keyframe block: query, verify, build the graph, solve, adopt. Every launch is on the context's stream; the ring is counted for
 * the whole batch, so which slots are live is host arithmetic, and which sequences adopt is decided on the device. */
static int vo_loop_stage(tb_vo* vo, int b, int t) {
    tb_ctx* ctx = vo->ctx;
    tb_kf_store* st = vo->store;
    const tb_vo_loop& l = vo->lp;
    const tb_vo_frame_out& o = vo->out[vo->oc];
    const int S = vo->nseq, P = vo->P, cap = st->cap, nn = cap + 1;
    if (st->pnp_on) return tb_fail(ctx, TB_ESTATE, "loop correction on a store with PnP verification (enabled on the lent store): not combined yet");
    const int nlive = (int)std::min<long long>(st->nadded, cap), oldest = st->nadded >= cap ? (int)(st->nadded % cap) : 0;
    TB_TRY(tb_bow_db_query_dev(vo->db, o.bv_word, o.bv_val, o.bv_cnt, P, l.exclude_newest, l.topk, vo->rl_scores, vo->rl_top_slot,
                               vo->rl_top_kf, vo->rl_top_score, nullptr));
    const tb_reloc_params prm = vo_reloc_params(vo, l.min_inliers);
    tb_reloc_out out = {};
    out.best_rank = vo->lp_best_rank; out.best_kf = vo->lp_best_kf; out.best_Tcw = vo->lp_best_Tcw;
    TB_TRY(tb_relocalize_batch_dev(st, vo->p.K, vo->p.nlevels, vo->p.scale, o.orb, o.orb_desc, o.orb_cnt, o.fv_keys, o.fv_cnt, P,
                                   vo->rl_top_slot, l.topk, &prm, &out));
    TB_TRY(tbk_vo_loop_graph(ctx, S, cap, nlive, oldest, t, l.topk, l.w_rot, l.w_trans, st->Tcw, st->kf_ids, vo->Tcw[b], vo->lp_best_rank,
                             vo->lp_best_kf, vo->lp_best_Tcw, vo->lp_before, vo->lp_after, vo->lp_node_kf, vo->lp_nnodes, vo->lp_edges,
                             vo->lp_ecount));
    TB_TRY(tb_pose_graph_batch_dev(ctx, S, nn, 1, vo->lp_after, vo->lp_edges, vo->lp_ecount, nn, l.iters, vo->lp_stats));
    return tbk_vo_loop_adopt(ctx, S, cap, nlive, oldest, l.topk, P, vo->lp_before, vo->lp_after, vo->lp_ecount, vo->lp_stats, vo->lp_best_rank,
                             vo->lp_best_kf, st->ninl, st->Tcw, st->mp, st->valid, st->counts, vo->kf.mp, vo->kf.valid, vo->kf.cnt, vo->mp[b],
                             vo->valid[b], vo->kcnt[b], vo->Tcw[b], vo->lp_closed, vo->lp_kf, vo->lp_inl);
}

/* ORB operator() on n images. The extractor's results do not outlive its next call, so a descriptor tracker copies them into
 * out[oc]; the optical-flow loop extracts for a keyframe only and packs its keys straight from the extractor. */
static int vo_extract(tb_vo* vo, const uint8_t* images, int n) {
    const tb_vo_params& p = vo->p;
    TB_TRY(tb_extractor_set_images_dev(vo->ex, images, n, p.width, (size_t)p.width * p.height));
    TB_TRY(tb_extractor_build_pyramid(vo->ex, n));
    TB_TRY(tb_extractor_orb(vo->ex, n, p.target, p.init_th, p.min_th, 0, nullptr, 0));
    if (vo->tr.kind == TB_VO_OPFLOW) return TB_OK;
    const tb_vo_frame_out& o = vo->out[vo->oc];
    return tb_extractor_copy_results_dev(vo->ex, n, o.orb, o.orb_desc, o.orb_cnt, vo->P);
}

/* The tracking half of frame t after the left images are in img[b]: the frame's keys, the map points they carry over from the
 * last frame (optical flow), the keyframe or the map, and the optimised pose, into side b and out[oc]. Frame 0 tracks nothing
 * and keeps the reset pose. See include/tb_capi.h, tb_vo_tracker. */
static int vo_track(tb_vo* vo, int t) {
    tb_ctx* ctx = vo->ctx;
    const tb_vo_params& p = vo->p;
    const tb_vo_tracker& tr = vo->tr;
    const tb_vo_frame_out& o = vo->out[vo->oc];
    const tb_vo_kf_out& kf = vo->kf;
    const int S = vo->nseq, P = vo->P, W = p.width, H = p.height;
    const size_t ip = (size_t)W * H, cnt_bytes = (size_t)S * sizeof(int32_t);
    const int a = vo->cur, b = a ^ 1;   /* a: last frame, b: this frame */
    if (t == 0) TB_HIP(ctx, hipMemcpyAsync(vo->Tcw[b], vo->Tcw[a], (size_t)S * 16 * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    if (tr.kind == TB_VO_OPFLOW) {
        if (t == 0) {
            TB_HIP(ctx, hipMemsetAsync(vo->kcnt[b], 0, cnt_bytes, ctx->stream));
            TB_HIP(ctx, hipMemsetAsync(o.obs_counts, 0, cnt_bytes, ctx->stream));
            TB_HIP(ctx, hipMemsetAsync(o.n_inliers, 0, cnt_bytes, ctx->stream));
            return TB_OK;
        }
        /* test_vo.cpp:716: searchByOPFlow(cur, last, pts, true, true) -- the tracked points land in this frame's key list */
        TB_TRY(tb_search_by_opflow_batch_dev(ctx, S, vo->img[b], vo->img[a], W, H, W, ip, &vo->cam, vo->keys[a], vo->kcnt[a], P, 1, 1,
                                             vo->keys[b], vo->status, vo->lk_matches, P, vo->lk_mcounts));
        TB_TRY(tbk_vo_track(ctx, S, vo->kcnt[a], vo->status, vo->keys[b], vo->mp[a], vo->valid[a], P, vo->kcnt[b], vo->mp[b], vo->valid[b],
                            o.obs, o.obs_counts, o.outlier));
        /* :761 LocalBA::PoseOptimization, started from the last frame's pose (:688) */
        return tb_pose_opt_batch_dev(ctx, S, p.K, vo->Tcw[a], o.obs, o.obs_counts, P, o.outlier, vo->Tcw[b], o.n_inliers, nullptr);
    }
    const bool proj = vo_is_proj(vo), map = tr.kind == TB_VO_PROJECTION_MAP;
    const int c = vo->map_cur;
    /* ORB operator() on every frame; test_projection.cpp:495-504 adds SetKeys and AssignFeaturesToGrid */
    TB_TRY(vo_extract(vo, vo->img[b], S));
    if (tr.kind == TB_VO_BOW) {
        /* :705 cur_frame_ptr->SetBow(vocabulary) on every frame: voc->transform(descriptors, mBowVec, mFeatVec, levelsup) */
        TB_TRY(tb_bow_transform_batch_dev(ctx, vo->voc, S, o.orb_desc, o.orb_cnt, P, vo->bw.levelsup, o.bow_word, o.bow_node, vo->bow_wt,
                                          o.fv_keys, o.fv_cnt));
        TB_TRY(tb_bow_vector_batch_dev(ctx, vo->voc, S, o.bow_word, vo->bow_wt, o.orb_cnt, P, o.bv_word, o.bv_val, o.bv_cnt));
    }
    if (proj) TB_TRY(tb_frame_grid_batch_dev(ctx, S, o.orb, o.orb_cnt, P, W, H, vo->cell_start, vo->cell_items));
    if (t == 0) {
        TB_HIP(ctx, hipMemsetAsync(o.mcounts, 0, cnt_bytes, ctx->stream));
        TB_HIP(ctx, hipMemsetAsync(o.mflags, 0, cnt_bytes, ctx->stream));
        TB_HIP(ctx, hipMemsetAsync(o.n_inliers, 0, cnt_bytes, ctx->stream));
    } else if (tr.kind == TB_VO_BOW) {
        /* searchByBow(cur, key_frame, MapPointOnly): F1 = the current frame, F2 = the keyframe, whose map points are has_mp2 */
        TB_TRY(tb_search_by_bow_batch_dev(ctx, S, o.orb, o.orb_desc, P, o.fv_keys, o.fv_cnt, kf.orb, kf.desc, P, kf.fv_keys, kf.fv_cnt,
                                          kf.valid, vo->bw.map_point_only, tr.th_low, tr.nratio, tr.histo_len, tr.check_orientation,
                                          o.matches, P, o.mcounts, o.mflags));
    } else if (tr.kind == TB_VO_BF) {
        /* :712 searchByBF(cur, key_frame, 0, nLevels, ratio, minTh): the whole-set branch */
        TB_TRY(tb_search_by_bf_batch_dev(ctx, S, o.orb_desc, o.orb_cnt, kf.desc, kf.cnt, (size_t)P * 32, tr.bf_ratio, tr.bf_min_th, o.matches,
                                         P, o.mcounts));
    } else if (tr.kind == TB_VO_NN) {
        /* test_vo_1 :213 searchByNN(cur, key_frame, 0, nLevels, ratio, minTh): the whole-set branch */
        TB_TRY(tb_search_by_nn_batch_dev(ctx, vo->lsh, S, o.orb_desc, o.orb_cnt, kf.desc, kf.cnt, (size_t)P * 32, tr.bf_ratio, tr.bf_min_th,
                                         o.matches, P, o.mcounts));
    } else if (tr.kind == TB_VO_VIOLENCE) {
        /* :713 searchByViolence(cur, key_frame, min_level, max_level, radius) over the keyframe's lookup grid */
        TB_TRY(tb_search_by_violence_batch_dev(ctx, S, o.orb, o.orb_desc, o.orb_cnt, P, kf.orb, kf.desc, kf.cnt, P, vo->kf_cell_start,
                                               vo->kf_cell_items, W, H, tr.min_level, tr.max_level, tr.radius, tr.th_low, tr.nratio,
                                               tr.histo_len, tr.check_orientation, o.matches, P, o.mcounts, o.mflags));
    } else if (map) {
        /* :516-517 searchByProjection(map_ptr, cur, radio) at the last frame's pose (:510) */
        TB_TRY(tb_search_by_projection_map_batch_dev(ctx, S, vo->Tcw[a], &vo->cam, W, H, o.orb, o.orb_desc, vo->taken, o.orb_cnt, P,
                                                     vo->cell_start, vo->cell_items, vo->map_rec[c], vo->map_desc[c], vo->map_n[c],
                                                     vo->map_cap, vo->map_cap, vo->sf, p.nlevels, tr.nratio, tr.radio, tr.th_high, o.matches,
                                                     vo->Mcap, o.mcounts, o.mflags));
    } else {
        /* :512-513 searchByProjection(cur, key_frame) at the last frame's pose (:510) */
        TB_TRY(tb_search_by_projection_batch_dev(ctx, S, vo->Tcw[a], &vo->cam, W, H, o.orb, o.orb_desc, vo->taken, o.orb_cnt, P,
                                                 vo->cell_start, vo->cell_items, kf.orb, vo->kf_rec, kf.mp_desc, kf.cnt, P, vo->sf,
                                                 p.nlevels, tr.nratio, tr.th_high, tr.histo_len, tr.check_orientation, o.matches, vo->Mcap,
                                                 o.mcounts, o.mflags));
    }
    /* the keys, the map points (projection: and their descriptors, :520-530) the matches carry over and the pose rows (match
     * count 0 at frame 0: a fresh frame) */
    if (map) {
        TB_TRY(tbk_vo_proj_carry(ctx, S, 1, o.orb, o.orb_cnt, o.matches, o.mcounts, vo->Mcap, nullptr, nullptr, vo->map_rec[c],
                                 vo->map_desc[c], vo->map_n[c], vo->map_cap, P, vo->inv_sigma2, p.nlevels, vo->win, vo->keys[b], vo->kcnt[b],
                                 vo->mp[b], vo->valid[b], o.mp_desc, o.obs, o.obs_counts, o.outlier));
    } else if (proj) {
        TB_TRY(tbk_vo_proj_carry(ctx, S, 0, o.orb, o.orb_cnt, o.matches, o.mcounts, vo->Mcap, kf.mp, kf.valid, nullptr, kf.mp_desc, kf.cnt, P,
                                 P, vo->inv_sigma2, p.nlevels, vo->win, vo->keys[b], vo->kcnt[b], vo->mp[b], vo->valid[b], o.mp_desc, o.obs,
                                 o.obs_counts, o.outlier));
    } else {
        TB_TRY(tbk_vo_match_carry(ctx, S, o.orb, o.orb_cnt, o.matches, o.mcounts, kf.mp, kf.valid, kf.cnt, P, vo->inv_sigma2, p.nlevels,
                                  vo->win, vo->keys[b], vo->kcnt[b], vo->mp[b], vo->valid[b], o.obs, o.obs_counts, o.outlier));
    }
    if (t == 0) return TB_OK;
    TB_TRY(tb_pose_opt_batch_dev(ctx, S, p.K, vo->Tcw[a], o.obs, o.obs_counts, P, o.outlier, vo->Tcw[b], o.n_inliers, nullptr));
    return vo->rec_on ? vo_recover_stage(vo, b) : TB_OK;
}

/* The keyframe block of frame t, side b: stereo depths for the frame's keys, the new map points, key_frame = cur_frame_ptr.
 * d_idx == nullptr: the whole batch (nk == nseq), read in place. Otherwise the nk sequences h_idx / d_idx name (ascending, a
 * ragged step): their images and keys are compacted for the stereo operator, and everything else serves row d_idx[j]. What
 * counts keyframes for the whole batch -- the map, the database, the store, the recovery rings -- never meets an index list
 * (vo_ragged_unsupported). */
static int vo_keyframe(tb_vo* vo, int t, int b, int nk, const int32_t* h_idx, const int32_t* d_idx, const uint8_t* right, int stride,
                       size_t pitch) {
    tb_ctx* ctx = vo->ctx;
    const tb_vo_params& p = vo->p;
    const tb_vo_tracker& tr = vo->tr;
    const tb_vo_frame_out& o = vo->out[vo->oc];
    const tb_vo_kf_out& kf = vo->kf;
    const int P = vo->P, W = p.width, H = p.height;
    const size_t ip = (size_t)W * H;
    const uint8_t* left = vo->img[b];
    const float* keys = vo->keys[b];
    const int32_t* kcnt = vo->kcnt[b];
    TB_TRY(tbk_vo_copy_image(ctx, nk, right, W, H, stride, pitch, vo->right, d_idx));
    if (d_idx) {
        TB_TRY(tbk_vo_copy_image(ctx, nk, left, W, H, W, ip, vo->rg_left, d_idx));
        left = vo->rg_left;
    }
    if (tr.kind == TB_VO_OPFLOW) {
        /* :774-785 ORB operator()(pyramid, sf, target, init_th, min_th) + SetKeys. A descriptor tracker's second ORB call on the
         * same pyramid returns the same keys, so SetKeys resizes m to m and keeps every carried map point: nothing to do. */
        TB_TRY(vo_extract(vo, left, nk));
        const tb_keypoint* kps = nullptr; const int32_t* cnt = nullptr; int selCap = 0;
        tb_extractor_results_dev(vo->ex, &kps, nullptr, &cnt, &selCap);
        TB_TRY(tbk_vo_kf_pack(ctx, nk, kps, cnt, selCap, P, vo->keys[b], vo->kcnt[b], vo->valid[b], d_idx));
    }
    if (d_idx) {
        TB_TRY(tbk_vo_kf_gather(ctx, nk, d_idx, keys, kcnt, P, vo->rg_keys, vo->rg_kcnt));
        keys = vo->rg_keys; kcnt = vo->rg_kcnt;
    }
    /* :800 AddMapPointsByStereo(cur, right, d * fx, fx), then the new map points (:802-832) */
    TB_TRY(tb_add_map_points_by_stereo_batch_dev(ctx, nk, vo->right, left, W, H, W, ip, &vo->cam, keys, kcnt, P, p.bf, vo->st_pts,
                                                 vo->st_status, vo->depth));
    TB_TRY(tbk_vo_kf_spawn(ctx, nk, vo->keys[b], vo->kcnt[b], vo->depth, vo->Tcw[b], p.K, P, vo->mp[b], vo->valid[b], d_idx));
    if (tr.kind == TB_VO_OPFLOW) return TB_OK;
    if (vo_is_proj(vo)) {
        const bool map = tr.kind == TB_VO_PROJECTION_MAP;
        int slot = 0;
        if (map) {
            if (vo->map_nblk == vo->mapK) {   /* the oldest keyframe's points leave; the survivors move into the other set */
                const int c = vo->map_cur, d = c ^ 1;
                TB_TRY(tbk_vo_map_evict(ctx, nk, vo->map_rec[c], vo->map_desc[c], vo->map_n[c], vo->map_blocks[c], vo->mapK, vo->map_cap,
                                        vo->map_rec[d], vo->map_desc[d], vo->map_n[d], vo->map_blocks[d]));
                vo->map_cur = d;
                vo->map_nblk = vo->mapK - 1;
            }
            slot = vo->map_nblk++;
        }
        const int c = vo->map_cur;
        TB_TRY(tbk_vo_kf_append(ctx, nk, vo->kcnt[b], vo->depth, vo->mp[b], vo->valid[b], o.orb_desc, vo->Tcw[b], P, o.mp_desc,
                                map ? nullptr : vo->kf_rec, map ? vo->map_rec[c] : nullptr, map ? vo->map_desc[c] : nullptr,
                                map ? vo->map_n[c] : nullptr, map ? vo->map_blocks[c] : nullptr, map ? vo->mapK : 0, slot, vo->map_cap,
                                d_idx));
    }
    /* key_frame = cur_frame_ptr (:836, test_projection.cpp:641), for these sequences */
    TB_TRY(tbk_vo_kf_snapshot(ctx, nk, d_idx, P, &o, vo->mp[b], vo->valid[b], &kf));
    if (tr.kind == TB_VO_VIOLENCE) {
        /* the keyframe's lookup grid, once per keyframe: one call per run of neighbouring sequences (no list: the run [0, nk)) */
        for (int j = 0; j < nk;) {
            int e = h_idx ? j + 1 : nk;
            while (h_idx && e < nk && h_idx[e] == h_idx[e - 1] + 1) e++;
            const size_t s0 = h_idx ? (size_t)h_idx[j] : 0;
            TB_TRY(tb_frame_grid_batch_dev(ctx, e - j, kf.orb + s0 * P, kf.cnt + s0, P, W, H, vo->kf_cell_start + s0 * TB_GRID_STARTS,
                                           vo->kf_cell_items + s0 * P));
            j = e;
        }
    }
    if (tr.kind != TB_VO_BOW || d_idx) return TB_OK;
    /* the keyframe keeps the vectors SetBow gave it: they are not computed again. The keyframe database, when enabled: the
     * snapshot's BowVector into the ring slot of this keyframe */
    if (vo->db) TB_TRY(tb_bow_db_add_dev(vo->db, kf.bv_word, kf.bv_val, kf.bv_cnt, P, t));
    /* the keyframe store, when enabled: the snapshot itself and the frame's optimised pose into the same ring slot */
    if (vo->store) TB_TRY(tb_kf_store_add_dev(vo->store, kf.orb, kf.desc, kf.cnt, kf.fv_keys, kf.fv_cnt, kf.mp, kf.valid, P, vo->Tcw[b], t));
    /* recovery, when enabled: the snapshot's word / node ids into the same ring slot (the store has just counted this add); this
     * keyframe is what every sequence tracks against from now on */
    if (vo->rec_on) {
        TB_TRY(tbk_vo_recover_ring_add(ctx, nk, kf.bow_word, kf.bow_node, kf.cnt, vo->store->cap, P,
                                       (int)((vo->store->nadded - 1) % vo->store->cap), vo->rc_word_ring, vo->rc_node_ring));
        TB_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)vo->rc_kf_ids, t, (size_t)nk, ctx->stream));
    }
    return TB_OK;
}

/* Frame t of every sequence (the arguments are checked): what tb_vo_step_dev launches. */
static int vo_step_lock(tb_vo* vo, int t, bool keyframe, const uint8_t* left, const uint8_t* right, int stride, size_t pitch) {
    const int S = vo->nseq, b = vo->cur ^ 1;
    TB_TRY(tbk_vo_copy_image(vo->ctx, S, left, vo->p.width, vo->p.height, stride, pitch, vo->img[b]));
    TB_TRY(vo_track(vo, t));
    if (vo->lp_on && keyframe && t > 0) TB_TRY(vo_loop_stage(vo, b, t));
    if (vo->wb_on && t > 0) {   /* the frame's slot of the segment log */
        const tb_vo_frame_out& o = vo->out[vo->oc];
        const int slot = t - vo->kf_frame;
        if (slot < 1 || slot >= vo->wb_nslot) return tb_fail(vo->ctx, TB_ESTATE, "window BA: frame %d is %d frames past its keyframe", t, slot);
        TB_TRY(tbk_vo_seg_log(vo->ctx, S, vo->keys[b], vo->kcnt[b], vo->valid[b], o.outlier, o.obs_counts, vo->Tcw[b], vo->sg_spawned, vo->P,
                              vo->wb_nslot, slot, vo->sg_keys, vo->sg_ok, vo->sg_pose));
        vo->wb_slot = slot;
        if (keyframe) TB_TRY(vo_window_ba(vo, b));
    }
    if (vo->mono_on && t > 0)   /* which keys LK still holds, and which of them have no map point yet */
        TB_TRY(tbk_vo_mono_alive(vo->ctx, S, vo->kcnt[b], vo->status, vo->valid[b], vo->P, vo->mn_alive, vo->mn_skip));
    if (keyframe && vo->mono_on && t > 0) {
        TB_TRY(vo_mono_keyframe(vo, b, t));
    } else if (keyframe && vo->mi_on) {   /* frame 0 without a right image: ORB only, no key has a map point */
        TB_TRY(vo_extract(vo, vo->img[b], S));
        const tb_keypoint* kps = nullptr; const int32_t* cnt = nullptr; int selCap = 0;
        tb_extractor_results_dev(vo->ex, &kps, nullptr, &cnt, &selCap);
        TB_TRY(tbk_vo_kf_pack(vo->ctx, S, kps, cnt, selCap, vo->P, vo->keys[b], vo->kcnt[b], vo->valid[b], nullptr));
        TB_TRY(vo_mono_start(vo, b));
    } else if (keyframe) {
        TB_TRY(vo_keyframe(vo, t, b, S, nullptr, nullptr, right, stride, pitch));
        if (vo->mono_on) TB_TRY(vo_mono_start(vo, b));
        if (vo->wb_on) {   /* the next segment starts here */
            TB_TRY(tbk_vo_seg_start(vo->ctx, S, vo->keys[b], vo->kcnt[b], vo->depth, vo->mp[b], vo->valid[b], vo->Tcw[b], vo->P, vo->wb_nslot,
                                    vo->sg_keys,
                                    vo->sg_ok, vo->sg_pose, vo->sg_pts, vo->sg_spawned));
            vo->wb_slot = 0;
        }
    }
    if (keyframe) vo->kf_frame = t;
    vo->cur = b;
    vo->next = t + 1;
    vo->s3_slot = nullptr;   /* a Sim(3) query needs a tb_vo_relocalize_dev of this frame */
    vo->s3_done = false;
    for (int s = 0; s < S; s++) {
        vo->seq_frame[s] = t;
        if (keyframe) vo->seq_kf_frame[s] = t;
    }
    return TB_OK;
}

int tb_vo_step_dev(tb_vo* vo, const uint8_t* left, const uint8_t* right, int stride, size_t pitch) {
    TB_ENTER((vo ? vo->ctx : nullptr));
    if (!vo) return TB_EINVAL;
    tb_ctx* ctx = vo->ctx;
    const tb_vo_params& p = vo->p;
    if (vo->ragged) return tb_fail(ctx, TB_ESTATE, "tb_vo_step_dev: the loop is in ragged mode (tb_vo_step_ragged_dev, or tb_vo_reset_dev)");
    if (vo->next < 0) return tb_fail(ctx, TB_ESTATE, "tb_vo_step_dev before tb_vo_reset_dev");
    const int t = vo->next;
    const bool keyframe = t % p.keyframe_every == 0;
    if (!left || stride < p.width || pitch < (size_t)stride * p.height) return tb_fail(ctx, TB_EINVAL, "tb_vo_step_dev: left images / geometry");
    if (keyframe && !right && !(vo->mono_on && (t > 0 || vo->mi_on)))
        return tb_fail(ctx, TB_EINVAL, "tb_vo_step_dev: frame %d is a keyframe and needs the right images", t);
    return vo_step_lock(vo, t, keyframe, left, right, stride, pitch);
}

/* ---- ragged batches: see include/tb_capi.h, tb_vo_step_ragged_dev */
static const char* vo_ragged_unsupported(const tb_vo* vo) {
    if (vo->tr.kind == TB_VO_PROJECTION_MAP) return "TB_VO_PROJECTION_MAP counts the map's blocks and evicts for the whole batch";
    if (vo->db) return "the keyframe database's ring slot is counted for the whole batch";
    if (vo->wb_on) return "the window BA counts the segment's slots for the whole batch";
    if (vo->mono_on) return "the mono mode keeps one keyframe segment for the whole batch";
    return nullptr;
}

/* Everything ragged mode needs beyond the lock-step loop, allocated once (allocation synchronises; a step never grows it). A
 * failed attempt leaves what it got with the owner, the pinned ring and the events; the next one takes only what is missing
 * of the last two. */
static int vo_ragged_init(tb_vo* vo) {
    if (vo->rg_ready) return TB_OK;
    tb_ctx* ctx = vo->ctx;
    const size_t S = (size_t)vo->nseq, P = (size_t)vo->P, img = (size_t)vo->p.width * vo->p.height;
    TB_TRY(vo_alloc_frame_out(vo, vo->out[vo->oc ^ 1]));
    TB_TRY(tb_dev_alloc(ctx, vo->own, &vo->rg_left, S * img));
    TB_TRY(tb_dev_alloc(ctx, vo->own, &vo->rg_keys, S * P * 2));
    TB_TRY(tb_dev_alloc(ctx, vo->own, &vo->rg_kcnt, S));
    TB_TRY(tb_dev_alloc(ctx, vo->own, &vo->rg_dev, 2 * S));
    if (!vo->rg_pin) TB_HIP(ctx, hipHostMalloc((void**)&vo->rg_pin, (size_t)tb_vo::RG_RING * 2 * S * sizeof(int32_t), hipHostMallocDefault));
    for (hipEvent_t& e : vo->rg_ev)
        if (!e) TB_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    vo->rg_ready = true;
    return TB_OK;
}

/* The one host -> device copy of a ragged call: mask [nseq] and index list [nseq] from a pinned ring slot into rg_dev. The slot
 * is reused RG_RING calls later, after its event says the copy has run. Returns the slot's host pointer through *pin. */
static int vo_ragged_stage(tb_vo* vo, int32_t** pin) {
    tb_ctx* ctx = vo->ctx;
    const int k = (int)(vo->rg_slot % tb_vo::RG_RING);
    TB_HIP(ctx, hipEventSynchronize(vo->rg_ev[k]));
    *pin = vo->rg_pin + (size_t)k * 2 * vo->nseq;
    return TB_OK;
}
static int vo_ragged_upload(tb_vo* vo, const int32_t* pin) {
    tb_ctx* ctx = vo->ctx;
    const int k = (int)(vo->rg_slot++ % tb_vo::RG_RING);
    TB_HIP(ctx, hipMemcpyAsync(vo->rg_dev, pin, (size_t)2 * vo->nseq * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    TB_HIP(ctx, hipEventRecord(vo->rg_ev[k], ctx->stream));
    return TB_OK;
}

int tb_vo_reset_seq_dev(tb_vo* vo, const uint8_t* which, const float* Tcw0) {
    TB_ENTER((vo ? vo->ctx : nullptr));
    if (!vo || !which || !Tcw0) return TB_EINVAL;
    tb_ctx* ctx = vo->ctx;
    if (const char* why = vo_ragged_unsupported(vo)) return tb_fail(ctx, TB_EUNSUPPORTED, "tb_vo_reset_seq_dev: %s", why);
    TB_TRY(vo_ragged_init(vo));
    const int S = vo->nseq;
    int32_t* pin;
    TB_TRY(vo_ragged_stage(vo, &pin));
    for (int s = 0; s < S; s++) { pin[s] = which[s] ? 1 : 0; pin[S + s] = 0; }
    TB_TRY(vo_ragged_upload(vo, pin));
    /* null for the loops that have no such array */
    TB_TRY(tbk_vo_reset_seq(ctx, S, vo->rg_dev, Tcw0, vo->Tcw[vo->cur], vo->kcnt[vo->cur], vo->kf.cnt, vo->kf.fv_cnt, vo->kf.bv_cnt,
                            vo->tr.kind == TB_VO_VIOLENCE ? vo->kf_cell_start : nullptr, TB_GRID_STARTS));
    for (int s = 0; s < S; s++)
        if (which[s]) { vo->seq_frame[s] = -1; vo->seq_kf_frame[s] = -1; vo->seq_reset[s] = 1; }
    vo->ragged = true;
    vo->next = 1 + *std::max_element(vo->seq_frame.begin(), vo->seq_frame.end());
    vo->s3_slot = nullptr;
    vo->s3_done = false;
    vo->kf_frame = *std::max_element(vo->seq_kf_frame.begin(), vo->seq_kf_frame.end());
    return TB_OK;
}

int tb_vo_step_ragged_dev(tb_vo* vo, const uint8_t* left, const uint8_t* right, int stride, size_t pitch, const uint8_t* active,
                          const uint8_t* force_keyframe) {
    TB_ENTER((vo ? vo->ctx : nullptr));
    if (!vo) return TB_EINVAL;
    tb_ctx* ctx = vo->ctx;
    const tb_vo_params& p = vo->p;
    if (const char* why = vo_ragged_unsupported(vo)) return tb_fail(ctx, TB_EUNSUPPORTED, "tb_vo_step_ragged_dev: %s", why);
    if (!vo->ragged && vo->next < 0) return tb_fail(ctx, TB_ESTATE, "tb_vo_step_ragged_dev before tb_vo_reset_dev / tb_vo_reset_seq_dev");
    const int S = vo->nseq;
    int nact = 0, nkf = 0, t0 = -1;
    bool same_t = true;
    for (int s = 0; s < S; s++) {
        if (active && !active[s]) continue;
        if (!vo->seq_reset[s]) return tb_fail(ctx, TB_ESTATE, "tb_vo_step_ragged_dev: sequence %d is active and was never reset", s);
        const int t = vo->seq_frame[s] + 1;
        if (nact++ == 0) t0 = t;
        same_t = same_t && t == t0;
        nkf += t % p.keyframe_every == 0 || (force_keyframe && force_keyframe[s]);
    }
    if (nact == 0) return TB_OK;   /* every sequence idles: nothing changes */
    if (!left || stride < p.width || pitch < (size_t)stride * p.height)
        return tb_fail(ctx, TB_EINVAL, "tb_vo_step_ragged_dev: left images / geometry");
    if (nkf && !right) return tb_fail(ctx, TB_EINVAL, "tb_vo_step_ragged_dev: %d sequences have a keyframe and need the right images", nkf);
    if (nact == S && same_t && (nkf == 0 || nkf == S)) {
        /* every sequence at the same frame with the same decision: this is tb_vo_step_dev's step, launch for launch */
        TB_TRY(vo_step_lock(vo, t0, nkf == S, left, right, stride, pitch));
        if (vo->ragged) vo->kf_frame = *std::max_element(vo->seq_kf_frame.begin(), vo->seq_kf_frame.end());
        return TB_OK;
    }
    TB_TRY(vo_ragged_init(vo));
    /* the masks, known to the host, go up in one copy; nothing is decided on the device and nothing is read back */
    int32_t* pin;
    TB_TRY(vo_ragged_stage(vo, &pin));
    nkf = 0;
    for (int s = 0; s < S; s++) {
        const bool act = !active || active[s];
        const int t = vo->seq_frame[s] + 1;
        pin[s] = act ? (t == 0 ? 2 : 1) : 0;
        if (act && (t % p.keyframe_every == 0 || (force_keyframe && force_keyframe[s]))) pin[S + nkf++] = s;
    }
    for (int j = nkf; j < S; j++) pin[S + j] = 0;
    TB_TRY(vo_ragged_upload(vo, pin));
    const int W = p.width, H = p.height;
    const int a = vo->cur, b = a ^ 1;
    TB_TRY(tbk_vo_copy_image(ctx, S, left, W, H, stride, pitch, vo->img[b]));
    /* the tracking half over all sequences, as frame t > 0 of the lock-step loop, into the other set of per-frame outputs: a
     * sequence without keys or keyframe gets no match, no row and keeps its pose; an idle one is restored below */
    vo->oc ^= 1;
    if (int rc = vo_track(vo, 1)) { vo->oc ^= 1; return rc; }
    tb_vo_hold_args h;
    h.mask = vo->rg_dev; h.pitch = vo->P; h.match_pitch = vo->Mcap; h.npx = (size_t)W * H;
    h.img[0] = vo->img[a]; h.img[1] = vo->img[b]; h.keys[0] = vo->keys[a]; h.keys[1] = vo->keys[b]; h.mp[0] = vo->mp[a]; h.mp[1] = vo->mp[b];
    h.valid[0] = vo->valid[a]; h.valid[1] = vo->valid[b]; h.kcnt[0] = vo->kcnt[a]; h.kcnt[1] = vo->kcnt[b];
    h.Tcw[0] = vo->Tcw[a]; h.Tcw[1] = vo->Tcw[b];
    h.prev = vo->out[vo->oc ^ 1]; h.cur = vo->out[vo->oc];
    TB_TRY(tbk_vo_hold(ctx, S, &h));
    vo->cur = b;
    if (nkf) TB_TRY(vo_keyframe(vo, -1, b, nkf, pin + S, vo->rg_dev + S, right, stride, pitch));
    for (int s = 0; s < S; s++)
        if (pin[s]) vo->seq_frame[s]++;
    for (int j = 0; j < nkf; j++) vo->seq_kf_frame[pin[S + j]] = vo->seq_frame[pin[S + j]];
    vo->ragged = true;
    vo->next = 1 + *std::max_element(vo->seq_frame.begin(), vo->seq_frame.end());
    vo->s3_slot = nullptr;
    vo->s3_done = false;
    vo->kf_frame = *std::max_element(vo->seq_kf_frame.begin(), vo->seq_kf_frame.end());
    return TB_OK;
}

int tb_vo_frames(tb_vo* vo, int32_t* frames, int32_t* kf_frames) {
    TB_ENTER((vo ? vo->ctx : nullptr));
    if (!vo) return TB_EINVAL;
    for (int s = 0; s < vo->nseq; s++) {
        if (frames) frames[s] = vo->seq_frame[s];
        if (kf_frames) kf_frames[s] = vo->seq_kf_frame[s];
    }
    return TB_OK;
}

int tb_vo_state_dev(tb_vo* vo, const float** Tcw, const float** keys_xy, const float** map_points, const uint8_t** mp_valid,
                    const int32_t** key_counts, const tb_obs** obs, const int32_t** obs_counts, const int32_t** n_inliers,
                    const uint8_t** outlier, int* key_pitch, int* frame) {
    TB_ENTER((vo ? vo->ctx : nullptr));
    if (!vo) return TB_EINVAL;
    const int c = vo->cur;
    const tb_vo_frame_out& o = vo->out[vo->oc];
    if (Tcw) *Tcw = vo->Tcw[c];
    if (keys_xy) *keys_xy = vo->keys[c];
    if (map_points) *map_points = vo->mp[c];
    if (mp_valid) *mp_valid = vo->valid[c];
    if (key_counts) *key_counts = vo->kcnt[c];
    if (obs) *obs = o.obs;
    if (obs_counts) *obs_counts = o.obs_counts;
    if (n_inliers) *n_inliers = o.n_inliers;
    if (outlier) *outlier = o.outlier;
    if (key_pitch) *key_pitch = vo->P;
    if (frame) *frame = vo->next - 1 < -1 ? -1 : vo->next - 1;
    return TB_OK;
}

int tb_vo_tracker_state_dev(tb_vo* vo, const tb_keypoint** orb, const uint8_t** orb_desc, const int32_t** orb_counts,
                            const tb_match** matches, const int32_t** match_counts, const int32_t** flags, const tb_keypoint** kf_orb,
                            const uint8_t** kf_desc, const float** kf_map_points, const uint8_t** kf_mp_valid,
                            const int32_t** kf_counts, int* kf_frame) {
    TB_ENTER((vo ? vo->ctx : nullptr));
    if (!vo) return TB_EINVAL;
    if (vo->tr.kind == TB_VO_OPFLOW) return tb_fail(vo->ctx, TB_ESTATE, "tb_vo_tracker_state_dev: the loop tracks by optical flow");
    const tb_vo_frame_out& o = vo->out[vo->oc];
    if (orb) *orb = o.orb;
    if (orb_desc) *orb_desc = o.orb_desc;
    if (orb_counts) *orb_counts = o.orb_cnt;
    if (matches) *matches = o.matches;
    if (match_counts) *match_counts = o.mcounts;
    if (flags) *flags = o.mflags;
    if (kf_orb) *kf_orb = vo->kf.orb;
    if (kf_desc) *kf_desc = vo->kf.desc;
    if (kf_map_points) *kf_map_points = vo->kf.mp;
    if (kf_mp_valid) *kf_mp_valid = vo->kf.valid;
    if (kf_counts) *kf_counts = vo->kf.cnt;
    if (kf_frame) *kf_frame = vo->kf_frame;
    return TB_OK;
}

int tb_vo_bow_state_dev(tb_vo* vo, const uint64_t** fv_keys, const int32_t** fv_counts, const int32_t** bv_words, const double** bv_values,
                        const int32_t** bv_counts, const int32_t** word_ids, const int32_t** node_ids, const uint64_t** kf_fv_keys,
                        const int32_t** kf_fv_counts, const int32_t** kf_bv_words, const double** kf_bv_values, const int32_t** kf_bv_counts,
                        const int32_t** kf_word_ids, const int32_t** kf_node_ids) {
    TB_ENTER((vo ? vo->ctx : nullptr));
    if (!vo) return TB_EINVAL;
    if (vo->tr.kind != TB_VO_BOW) return tb_fail(vo->ctx, TB_ESTATE, "tb_vo_bow_state_dev: the loop does not track by searchByBow");
    const tb_vo_frame_out& o = vo->out[vo->oc];
    const tb_vo_kf_out& kf = vo->kf;
    if (fv_keys) *fv_keys = o.fv_keys;
    if (fv_counts) *fv_counts = o.fv_cnt;
    if (bv_words) *bv_words = o.bv_word;
    if (bv_values) *bv_values = o.bv_val;
    if (bv_counts) *bv_counts = o.bv_cnt;
    if (word_ids) *word_ids = o.bow_word;
    if (node_ids) *node_ids = o.bow_node;
    if (kf_fv_keys) *kf_fv_keys = kf.fv_keys;
    if (kf_fv_counts) *kf_fv_counts = kf.fv_cnt;
    if (kf_bv_words) *kf_bv_words = kf.bv_word;
    if (kf_bv_values) *kf_bv_values = kf.bv_val;
    if (kf_bv_counts) *kf_bv_counts = kf.bv_cnt;
    if (kf_word_ids) *kf_word_ids = kf.bow_word;
    if (kf_node_ids) *kf_node_ids = kf.bow_node;
    return TB_OK;
}

int tb_vo_bow_db_enable(tb_vo* vo, int capacity) {
    TB_ENTER((vo ? vo->ctx : nullptr));
    if (!vo) return TB_EINVAL;
    if (vo->tr.kind != TB_VO_BOW) return tb_fail(vo->ctx, TB_ESTATE, "tb_vo_bow_db_enable: the loop does not track by searchByBow");
    if (vo->next > 0) return tb_fail(vo->ctx, TB_ESTATE, "tb_vo_bow_db_enable after a step (frame %d)", vo->next - 1);
    if (vo->db) return tb_fail(vo->ctx, TB_ESTATE, "tb_vo_bow_db_enable: the database is enabled already");
    return tb_bow_db_create(vo->ctx, vo->nseq, capacity, vo->P, vo->voc->scoring, &vo->db);
}

int tb_vo_bow_db_get(tb_vo* vo, tb_bow_db** out) {
    if (!vo || !out) return TB_EINVAL;
    *out = nullptr;
    if (!vo->db) return tb_fail(vo->ctx, TB_ESTATE, "tb_vo_bow_db_get: the keyframe database is not enabled");
    *out = vo->db;
    return TB_OK;
}

int tb_vo_reloc_enable(tb_vo* vo, int max_candidates) {
    TB_ENTER((vo ? vo->ctx : nullptr));
    if (!vo) return TB_EINVAL;
    tb_ctx* ctx = vo->ctx;
    if (vo->tr.kind != TB_VO_BOW) return tb_fail(ctx, TB_ESTATE, "tb_vo_reloc_enable: the loop does not track by searchByBow");
    if (!vo->db) return tb_fail(ctx, TB_ESTATE, "tb_vo_reloc_enable: the keyframe database is not enabled (tb_vo_bow_db_enable)");
    if (vo->next > 0) return tb_fail(ctx, TB_ESTATE, "tb_vo_reloc_enable after a step (frame %d)", vo->next - 1);
    if (vo->store) return tb_fail(ctx, TB_ESTATE, "tb_vo_reloc_enable: relocalisation is enabled already");
    TB_TRY(tb_kf_store_create(ctx, vo->nseq, vo->db->cap, vo->P, max_candidates, &vo->store));
    const size_t S = (size_t)vo->nseq, SC = S * max_candidates;
    int rc;
    if ((rc = tb_dev_alloc(ctx, vo->own, &vo->rl_scores, S * vo->db->cap)) || (rc = tb_dev_alloc(ctx, vo->own, &vo->rl_top_score, SC)) ||
        (rc = tb_dev_alloc(ctx, vo->own, &vo->rl_top_slot, SC)) || (rc = tb_dev_alloc(ctx, vo->own, &vo->rl_top_kf, SC))) {
        tb_kf_store_destroy(vo->store);   /* the store is what says "enabled": without it the call can be repeated */
        vo->store = nullptr;
    }
    return rc;
}

int tb_vo_relocalize_dev(tb_vo* vo, int topk, int exclude_newest, int min_inliers, double* scores, int32_t* top_slot, int32_t* top_kf,
                         double* top_score, int32_t* top_count, const tb_reloc_out* out) {
    TB_ENTER((vo ? vo->ctx : nullptr));
    if (!vo) return TB_EINVAL;
    tb_ctx* ctx = vo->ctx;
    if (!vo->store) return tb_fail(ctx, TB_ESTATE, "tb_vo_relocalize_dev: relocalisation is not enabled (tb_vo_reloc_enable)");
    if (vo->next < 1) return tb_fail(ctx, TB_ESTATE, "tb_vo_relocalize_dev before the first step");
    if (topk < 1 || topk > vo->store->max_cand || exclude_newest < 0)
        return tb_fail(ctx, TB_EINVAL, "tb_vo_relocalize_dev: topk %d (1..%d), exclude_newest %d", topk, vo->store->max_cand, exclude_newest);
    if (!scores) scores = vo->rl_scores;
    if (!top_slot) top_slot = vo->rl_top_slot;
    if (!top_kf) top_kf = vo->rl_top_kf;
    if (!top_score) top_score = vo->rl_top_score;
    const tb_vo_frame_out& o = vo->out[vo->oc];
    TB_TRY(tb_bow_db_query_dev(vo->db, o.bv_word, o.bv_val, o.bv_cnt, vo->P, exclude_newest, topk, scores, top_slot, top_kf, top_score,
                               top_count));
    const tb_reloc_params prm = vo_reloc_params(vo, min_inliers);
    TB_TRY(tb_relocalize_batch_dev(vo->store, vo->p.K, vo->p.nlevels, vo->p.scale, o.orb, o.orb_desc, o.orb_cnt, o.fv_keys, o.fv_cnt, vo->P,
                                   top_slot, topk, &prm, out));
    if (top_slot != vo->rl_top_slot)   /* tb_vo_relocalize_sim3_dev reads the loop's own copy: the caller's buffer may be gone by then */
        TB_HIP(ctx, hipMemcpyAsync(vo->rl_top_slot, top_slot, (size_t)vo->nseq * topk * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
    vo->s3_slot = vo->rl_top_slot;
    vo->s3_topk = topk;
    return TB_OK;
}

int tb_vo_relocalize_sim3_dev(tb_vo* vo, int topk, const tb_sim3_params* prm, int min_consensus, const tb_sim3_out* out) {
    TB_ENTER((vo ? vo->ctx : nullptr));
    if (!vo) return TB_EINVAL;
    tb_ctx* ctx = vo->ctx;
    if (!vo->store) return tb_fail(ctx, TB_ESTATE, "tb_vo_relocalize_sim3_dev: relocalisation is not enabled (tb_vo_reloc_enable)");
    if (vo->next < 1) return tb_fail(ctx, TB_ESTATE, "tb_vo_relocalize_sim3_dev before the first step");
    if (!vo->s3_slot) return tb_fail(ctx, TB_ESTATE, "tb_vo_relocalize_sim3_dev: no tb_vo_relocalize_dev since the last step");
    if (topk != vo->s3_topk)   /* the outputs are [nseq][topk]: a caller that sized them for another count must not be written to */
        return tb_fail(ctx, TB_EINVAL, "tb_vo_relocalize_sim3_dev: topk %d, but the last tb_vo_relocalize_dev ran with %d", topk, vo->s3_topk);
    const tb_vo_frame_out& o = vo->out[vo->oc];
    const int c = vo->cur;
    vo->s3_done = false;
    TB_TRY(tb_kf_store_sim3_dev(vo->store, vo->p.K, vo->p.nlevels, vo->p.scale, o.orb, o.orb_cnt, vo->mp[c], vo->valid[c], vo->P, vo->Tcw[c],
                                vo->s3_slot, vo->s3_topk, prm, min_consensus, out));
    vo->s3_done = true;
    return TB_OK;
}

int tb_vo_refine_sim3_dev(tb_vo* vo, int topk, const double* cand_srt, const int32_t* cand_consensus, const tb_sim3_opt_params* prm,
                          int min_inliers, int use_for_graph, const tb_sim3_refine_out* out) {
    TB_ENTER((vo ? vo->ctx : nullptr));
    if (!vo) return TB_EINVAL;
    tb_ctx* ctx = vo->ctx;
    if (!vo->store) return tb_fail(ctx, TB_ESTATE, "tb_vo_refine_sim3_dev: relocalisation is not enabled (tb_vo_reloc_enable)");
    if (!vo->s3_done || !vo->s3_slot) return tb_fail(ctx, TB_ESTATE, "tb_vo_refine_sim3_dev: no tb_vo_relocalize_sim3_dev since the last step");
    if (topk != vo->s3_topk)   /* the inputs and outputs are [nseq][topk]: a caller that sized them for another count must not be read or written past */
        return tb_fail(ctx, TB_EINVAL, "tb_vo_refine_sim3_dev: topk %d, but the last tb_vo_relocalize_dev ran with %d", topk, vo->s3_topk);
    const tb_vo_frame_out& o = vo->out[vo->oc];
    const int c = vo->cur;
    return tb_kf_store_sim3_refine_dev(vo->store, vo->p.K, vo->p.nlevels, vo->p.scale, o.orb, o.orb_cnt, vo->mp[c], vo->valid[c], vo->P,
                                       vo->Tcw[c], vo->s3_slot, vo->s3_topk, cand_srt, cand_consensus, prm, min_inliers, use_for_graph, out);
}

int tb_vo_search_sim3_dev(tb_vo* vo, int topk, const double* cand_srt, const int32_t* cand_consensus, float th, int th_high, int use_for_refine,
                          const tb_sim3_search_out* out) {
    TB_ENTER((vo ? vo->ctx : nullptr));
    if (!vo) return TB_EINVAL;
    tb_ctx* ctx = vo->ctx;
    if (!vo->store) return tb_fail(ctx, TB_ESTATE, "tb_vo_search_sim3_dev: relocalisation is not enabled (tb_vo_reloc_enable)");
    if (!vo->s3_done || !vo->s3_slot) return tb_fail(ctx, TB_ESTATE, "tb_vo_search_sim3_dev: no tb_vo_relocalize_sim3_dev since the last step");
    if (topk != vo->s3_topk)   /* the inputs and outputs are [nseq][topk]: a caller that sized them for another count must not be read or written past */
        return tb_fail(ctx, TB_EINVAL, "tb_vo_search_sim3_dev: topk %d, but the last tb_vo_relocalize_dev ran with %d", topk, vo->s3_topk);
    const tb_vo_frame_out& o = vo->out[vo->oc];
    const int c = vo->cur;
    return tb_kf_store_sim3_search_dev(vo->store, vo->p.K, vo->p.width, vo->p.height, vo->p.nlevels, vo->p.scale, o.orb, o.orb_desc, o.orb_cnt,
                                       vo->mp[c], vo->valid[c], vo->P, vo->Tcw[c], vo->s3_slot, vo->s3_topk, cand_srt, cand_consensus, th, th_high,
                                       use_for_refine, out);
}

int tb_vo_loop_sim3_dev(tb_vo* vo, int iters, int fixed_scale, double w_rot, double w_trans, double w_scale, tb_sim3_graph_out* out) {
    TB_ENTER((vo ? vo->ctx : nullptr));
    if (!vo) return TB_EINVAL;
    tb_ctx* ctx = vo->ctx;
    if (!vo->store) return tb_fail(ctx, TB_ESTATE, "tb_vo_loop_sim3_dev: relocalisation is not enabled (tb_vo_reloc_enable)");
    if (!vo->s3_done) return tb_fail(ctx, TB_ESTATE, "tb_vo_loop_sim3_dev: no tb_vo_relocalize_sim3_dev since the last step");
    return tb_kf_store_sim3_graph_run(vo->store, "tb_vo_loop_sim3_dev", vo->Tcw[vo->cur], vo->next - 1, iters, fixed_scale, w_rot, w_trans,
                                      w_scale, out);
}

int tb_vo_reloc_pnp_enable(tb_vo* vo, const tb_pnp_params* prm, int min_consensus, int expand) {
    TB_ENTER((vo ? vo->ctx : nullptr));
    if (!vo) return TB_EINVAL;
    tb_ctx* ctx = vo->ctx;
    if (!vo->store) return tb_fail(ctx, TB_ESTATE, "tb_vo_reloc_pnp_enable: relocalisation is not enabled (tb_vo_reloc_enable)");
    if (vo->next > 0) return tb_fail(ctx, TB_ESTATE, "tb_vo_reloc_pnp_enable after a step (frame %d)", vo->next - 1);
    if (vo->rec_on || vo->lp_on)
        return tb_fail(ctx, TB_ESTATE, "tb_vo_reloc_pnp_enable: recovery or loop correction is enabled; their adoption reads the verification's rows, "
                                       "which PnP compacts: not combined yet");
    return tb_kf_store_pnp_enable(vo->store, prm, min_consensus, expand);   /* TB_ESTATE when enabled already */
}

int tb_vo_recover_enable(tb_vo* vo, const tb_vo_recover* prm) {
    TB_ENTER((vo ? vo->ctx : nullptr));
    if (!vo) return TB_EINVAL;
    tb_ctx* ctx = vo->ctx;
    if (!vo->store) return tb_fail(ctx, TB_ESTATE, "tb_vo_recover_enable: relocalisation is not enabled (tb_vo_reloc_enable)");
    if (vo->store->pnp_on) return tb_fail(ctx, TB_ESTATE, "tb_vo_recover_enable: PnP verification is enabled; the two are not combined yet");
    if (vo->next > 0) return tb_fail(ctx, TB_ESTATE, "tb_vo_recover_enable after a step (frame %d)", vo->next - 1);
    if (vo->rec_on) return tb_fail(ctx, TB_ESTATE, "tb_vo_recover_enable: recovery is enabled already");
    if (vo->lp_on) return tb_fail(ctx, TB_ESTATE, "tb_vo_recover_enable: loop correction is enabled; the two are not combined yet");
    if (!prm) return tb_fail(ctx, TB_EINVAL, "tb_vo_recover_enable: null parameters");
    if (prm->lost_inliers < 0 || prm->min_inliers < 0 || prm->exclude_newest < 0 || prm->topk < 1 || prm->topk > vo->store->max_cand)
        return tb_fail(ctx, TB_EINVAL, "tb_vo_recover_enable: lost_inliers %d, topk %d (1..%d), exclude_newest %d, min_inliers %d",
                       prm->lost_inliers, prm->topk, vo->store->max_cand, prm->exclude_newest, prm->min_inliers);
    const size_t S = (size_t)vo->nseq, ring = S * vo->store->cap * vo->P;
    TB_TRY(tb_dev_alloc(ctx, vo->own, &vo->rc_lost, S));
    TB_TRY(tb_dev_alloc(ctx, vo->own, &vo->rc_track, S));
    TB_TRY(tb_dev_alloc(ctx, vo->own, &vo->rc_kf, S));
    TB_TRY(tb_dev_alloc(ctx, vo->own, &vo->rc_kf_ids, S));
    TB_TRY(tb_dev_alloc(ctx, vo->own, &vo->rc_best_rank, S));
    TB_TRY(tb_dev_alloc(ctx, vo->own, &vo->rc_best_kf, S));
    TB_TRY(tb_dev_alloc(ctx, vo->own, &vo->rc_best_Tcw, S * 16));
    TB_TRY(tb_dev_alloc(ctx, vo->own, &vo->rc_masked, S * prm->topk));
    TB_TRY(tb_dev_alloc(ctx, vo->own, &vo->rc_word_ring, ring));
    TB_TRY(tb_dev_alloc(ctx, vo->own, &vo->rc_node_ring, ring));
    TB_TRY(vo_recover_clear(vo));
    vo->rec = *prm;
    vo->rec_on = true;
    return TB_OK;
}

int tb_vo_recover_state_dev(tb_vo* vo, const uint8_t** lost, const int32_t** track_inliers, const int32_t** recovered_kf,
                            const int32_t** kf_ids, const int32_t** kf_word_ring, const int32_t** kf_node_ring) {
    TB_ENTER((vo ? vo->ctx : nullptr));
    if (!vo) return TB_EINVAL;
    if (!vo->rec_on) return tb_fail(vo->ctx, TB_ESTATE, "tb_vo_recover_state_dev: recovery is not enabled (tb_vo_recover_enable)");
    if (lost) *lost = vo->rc_lost;
    if (track_inliers) *track_inliers = vo->rc_track;
    if (recovered_kf) *recovered_kf = vo->rc_kf;
    if (kf_ids) *kf_ids = vo->rc_kf_ids;
    if (kf_word_ring) *kf_word_ring = vo->rc_word_ring;
    if (kf_node_ring) *kf_node_ring = vo->rc_node_ring;
    return TB_OK;
}

int tb_vo_loop_enable(tb_vo* vo, const tb_vo_loop* prm) {
    TB_ENTER((vo ? vo->ctx : nullptr));
    if (!vo) return TB_EINVAL;
    tb_ctx* ctx = vo->ctx;
    if (!vo->store) return tb_fail(ctx, TB_ESTATE, "tb_vo_loop_enable: relocalisation is not enabled (tb_vo_reloc_enable)");
    if (vo->store->pnp_on) return tb_fail(ctx, TB_ESTATE, "tb_vo_loop_enable: PnP verification is enabled; the two are not combined yet");
    if (vo->next > 0 || vo->ragged) return tb_fail(ctx, TB_ESTATE, "tb_vo_loop_enable after a step, or on a ragged loop");
    if (vo->lp_on) return tb_fail(ctx, TB_ESTATE, "tb_vo_loop_enable: loop correction is enabled already");
    if (vo->rec_on) return tb_fail(ctx, TB_ESTATE, "tb_vo_loop_enable: recovery is enabled; the two are not combined yet");
    if (!prm) return tb_fail(ctx, TB_EINVAL, "tb_vo_loop_enable: null parameters");
    if (vo->store->cap > 63)
        return tb_fail(ctx, TB_EINVAL, "tb_vo_loop_enable: store capacity %d: the graph holds the keyframes and the frame, 64 nodes", vo->store->cap);
    if (prm->topk < 1 || prm->topk > vo->store->max_cand || prm->exclude_newest < 0 || prm->min_inliers < 0 || prm->iters < 0 ||
        prm->iters > 99 || !(prm->w_rot >= 0) || !(prm->w_trans >= 0) || !std::isfinite(prm->w_rot) || !std::isfinite(prm->w_trans))
        return tb_fail(ctx, TB_EINVAL, "tb_vo_loop_enable: topk %d (1..%d), exclude_newest %d, min_inliers %d, iters %d (0..99), weights %g %g",
                       prm->topk, vo->store->max_cand, prm->exclude_newest, prm->min_inliers, prm->iters, prm->w_rot, prm->w_trans);
    const size_t S = (size_t)vo->nseq, nn = (size_t)vo->store->cap + 1;
    TB_TRY(tb_dev_alloc(ctx, vo->own, &vo->lp_closed, S));
    TB_TRY(tb_dev_alloc(ctx, vo->own, &vo->lp_kf, S));
    TB_TRY(tb_dev_alloc(ctx, vo->own, &vo->lp_inl, S));
    TB_TRY(tb_dev_alloc(ctx, vo->own, &vo->lp_nnodes, S));
    TB_TRY(tb_dev_alloc(ctx, vo->own, &vo->lp_ecount, S));
    TB_TRY(tb_dev_alloc(ctx, vo->own, &vo->lp_best_rank, S));
    TB_TRY(tb_dev_alloc(ctx, vo->own, &vo->lp_best_kf, S));
    TB_TRY(tb_dev_alloc(ctx, vo->own, &vo->lp_best_Tcw, S * 16));
    TB_TRY(tb_dev_alloc(ctx, vo->own, &vo->lp_node_kf, S * nn));
    TB_TRY(tb_dev_alloc(ctx, vo->own, &vo->lp_before, S * nn * 16));
    TB_TRY(tb_dev_alloc(ctx, vo->own, &vo->lp_after, S * nn * 16));
    TB_TRY(tb_dev_alloc(ctx, vo->own, &vo->lp_edges, S * nn));
    TB_TRY(tb_dev_alloc(ctx, vo->own, &vo->lp_stats, S * 8));
    /* the solver's work buffer is planned here, so that no step grows it (growing waits for the stream) */
    TB_TRY(tb_pose_graph_plan(ctx, vo->nseq, (int)nn, 1, (int)nn));
    vo->lp = *prm;
    vo->lp_on = true;
    return vo_loop_clear(vo);
}

int tb_vo_loop_state_dev(tb_vo* vo, const uint8_t** closed, const int32_t** loop_kf, const int32_t** loop_inliers, const int32_t** nnodes,
                         const int32_t** node_kf, const float** before, const float** after, const tb_pg_edge** edges,
                         const int32_t** edge_counts, const double** stats) {
    TB_ENTER((vo ? vo->ctx : nullptr));
    if (!vo) return TB_EINVAL;
    if (!vo->lp_on) return tb_fail(vo->ctx, TB_ESTATE, "tb_vo_loop_state_dev: loop correction is not enabled (tb_vo_loop_enable)");
    if (closed) *closed = vo->lp_closed;
    if (loop_kf) *loop_kf = vo->lp_kf;
    if (loop_inliers) *loop_inliers = vo->lp_inl;
    if (nnodes) *nnodes = vo->lp_nnodes;
    if (node_kf) *node_kf = vo->lp_node_kf;
    if (before) *before = vo->lp_before;
    if (after) *after = vo->lp_after;
    if (edges) *edges = vo->lp_edges;
    if (edge_counts) *edge_counts = vo->lp_ecount;
    if (stats) *stats = vo->lp_stats;
    return TB_OK;
}

int tb_vo_window_ba_enable(tb_vo* vo, const tb_vo_window_ba* prm) {
    TB_ENTER((vo ? vo->ctx : nullptr));
    if (!vo) return TB_EINVAL;
    tb_ctx* ctx = vo->ctx;
    const int E = vo->p.keyframe_every;
    if (vo->tr.kind != TB_VO_OPFLOW) return tb_fail(ctx, TB_ESTATE, "tb_vo_window_ba_enable: the loop does not track by optical flow");
    if (vo->mono_on) return tb_fail(ctx, TB_EUNSUPPORTED, "tb_vo_window_ba_enable: the loop is in mono mode (its keyframes spawn no stereo points)");
    if (vo->next > 0 || vo->ragged) return tb_fail(ctx, TB_ESTATE, "tb_vo_window_ba_enable after a step (frame %d)", vo->next - 1);
    if (vo->wb_on) return tb_fail(ctx, TB_ESTATE, "tb_vo_window_ba_enable: the window BA is enabled already");
    if (!prm) return tb_fail(ctx, TB_EINVAL, "tb_vo_window_ba_enable: null parameters");
    if (prm->iters < 1 || prm->iters > 99 || prm->fixed < 1 || prm->fixed > E || prm->min_obs < 2 || prm->min_points < 1)
        return tb_fail(ctx, TB_EINVAL, "tb_vo_window_ba_enable: iters %d (1..99), fixed %d (1..%d), min_obs %d (>= 2), min_points %d (>= 1)",
                       prm->iters, prm->fixed, E, prm->min_obs, prm->min_points);
    /* the local BA's limits: 64 free keyframes, 128 in all */
    if (E + 1 - prm->fixed > 64 || E + 1 > 128)
        return tb_fail(ctx, TB_EUNSUPPORTED, "tb_vo_window_ba_enable: a window of %d frames with %d fixed (the local BA takes 64 free, 128 in all)",
                       E + 1, prm->fixed);
    const size_t S = (size_t)vo->nseq, P = (size_t)vo->P, N = (size_t)E + 1;
    if (N * P > (size_t)INT32_MAX / 64) return tb_fail(ctx, TB_EUNSUPPORTED, "tb_vo_window_ba_enable: %zu x %zu observations per window", N, P);
    vo->wb_nslot = (int)N;
    tb_dev_owner& own = vo->own;
    TB_TRY(tb_dev_alloc(ctx, own, &vo->sg_keys, S * N * P * 2));
    TB_TRY(tb_dev_alloc(ctx, own, &vo->sg_ok, S * N * P));
    TB_TRY(tb_dev_alloc(ctx, own, &vo->sg_pose, S * N * 16));
    TB_TRY(tb_dev_alloc(ctx, own, &vo->sg_pts, S * P * 3));
    TB_TRY(tb_dev_alloc(ctx, own, &vo->sg_spawned, S * P));
    TB_TRY(tb_dev_alloc(ctx, own, &vo->wb_obs, S * N * P));
    TB_TRY(tb_dev_alloc(ctx, own, &vo->wb_counts, S));
    TB_TRY(tb_dev_alloc(ctx, own, &vo->wb_npts, S));
    TB_TRY(tb_dev_alloc(ctx, own, &vo->wb_stats, S * 8));
    TB_TRY(tb_dev_alloc(ctx, own, &vo->wb_pose, S * N * 16));
    TB_TRY(tb_dev_alloc(ctx, own, &vo->wb_pts, S * P * 3));
    TB_TRY(tb_dev_alloc(ctx, own, &vo->wb_adopted, S));
    TB_TRY(vo_window_clear(vo));
    /* the BA's workspace at its size now: a step never grows a scratch slot (growth synchronises) */
    void* d;
    TB_TRY(tb_scratch(ctx, TB_SLOT_WORK, tbk_local_ba_work_bytes(ctx, vo->nseq, (int)N, prm->fixed, vo->P, (int)(N * P)), &d));
    vo->wb = *prm;
    vo->wb_on = true;
    return TB_OK;
}

int tb_vo_window_state_dev(tb_vo* vo, const float** seg_keys, const uint8_t** seg_ok, const float** seg_pose, const float** seg_pts,
                           const uint8_t** seg_spawned, const tb_ba_obs** obs, const int32_t** obs_counts, const int32_t** n_points,
                           const double** stats, const uint8_t** adopted, const float** ba_pose, const float** ba_pts, int* slot,
                           int* nslots) {
    TB_ENTER((vo ? vo->ctx : nullptr));
    if (!vo) return TB_EINVAL;
    if (!vo->wb_on) return tb_fail(vo->ctx, TB_ESTATE, "tb_vo_window_state_dev: the window BA is not enabled (tb_vo_window_ba_enable)");
    if (seg_keys) *seg_keys = vo->sg_keys;
    if (seg_ok) *seg_ok = vo->sg_ok;
    if (seg_pose) *seg_pose = vo->sg_pose;
    if (seg_pts) *seg_pts = vo->sg_pts;
    if (seg_spawned) *seg_spawned = vo->sg_spawned;
    if (obs) *obs = vo->wb_obs;
    if (obs_counts) *obs_counts = vo->wb_counts;
    if (n_points) *n_points = vo->wb_npts;
    if (stats) *stats = vo->wb_stats;
    if (adopted) *adopted = vo->wb_adopted;
    if (ba_pose) *ba_pose = vo->wb_pose;
    if (ba_pts) *ba_pts = vo->wb_pts;
    if (slot) *slot = vo->wb_slot;
    if (nslots) *nslots = vo->wb_nslot;
    return TB_OK;
}

int tb_vo_mono_enable(tb_vo* vo, const tb_vo_mono* prm) {
    TB_ENTER((vo ? vo->ctx : nullptr));
    if (!vo) return TB_EINVAL;
    tb_ctx* ctx = vo->ctx;
    if (vo->tr.kind != TB_VO_OPFLOW)
        return tb_fail(ctx, TB_EUNSUPPORTED, "tb_vo_mono_enable: the loop does not track by optical flow (a later change)");
    if (vo->wb_on) return tb_fail(ctx, TB_EUNSUPPORTED, "tb_vo_mono_enable: the window BA is enabled (a later change)");
    if (vo->next >= 0 || vo->ragged) return tb_fail(ctx, TB_ESTATE, "tb_vo_mono_enable after a reset");
    if (vo->mono_on) return tb_fail(ctx, TB_ESTATE, "tb_vo_mono_enable: the mono mode is enabled already");
    if (!prm) return tb_fail(ctx, TB_EINVAL, "tb_vo_mono_enable: null parameters");
    if (!std::isfinite(prm->cos_parallax_max) || !std::isfinite(prm->chi2_max) || prm->cell <= 0)
        return tb_fail(ctx, TB_EINVAL, "tb_vo_mono_enable: cos_parallax_max %g, chi2_max %g, cell %d (> 0)", prm->cos_parallax_max,
                       prm->chi2_max, prm->cell);
    const size_t bitmap = tbk_vo_merge_bitmap_bytes(vo->p.width, vo->p.height, prm->cell);
    if (bitmap > TB_VO_MERGE_BITMAP_MAX)
        return tb_fail(ctx, TB_EINVAL, "tb_vo_mono_enable: cell %d on %d x %d needs an occupancy bitmap of %zu bytes (at most %d)", prm->cell,
                       vo->p.width, vo->p.height, bitmap, TB_VO_MERGE_BITMAP_MAX);
    const size_t S = (size_t)vo->nseq, SP = S * vo->P;
    tb_dev_owner& own = vo->own;
    TB_TRY(tb_dev_alloc(ctx, own, &vo->mn_kf_keys, SP * 2));
    TB_TRY(tb_dev_alloc(ctx, own, &vo->mn_kf_Tcw, S * 16));
    TB_TRY(tb_dev_alloc(ctx, own, &vo->mn_alive, SP));
    TB_TRY(tb_dev_alloc(ctx, own, &vo->mn_skip, SP));
    TB_TRY(tb_dev_alloc(ctx, own, &vo->mn_tri_points, SP * 3));
    TB_TRY(tb_dev_alloc(ctx, own, &vo->mn_tri_flags, SP));
    TB_TRY(tb_dev_alloc(ctx, own, &vo->mn_tri_tally, S * 6));
    TB_TRY(tb_dev_alloc(ctx, own, &vo->mn_survivors, S));
    TB_TRY(tb_dev_alloc(ctx, own, &vo->mn_added, S));
    vo->mono = *prm;
    TB_TRY(vo_mono_clear(vo));
    vo->mono_on = true;
    return TB_OK;
}

int tb_vo_mono_init_enable(tb_vo* vo, const tb_vo_mono_init* prm) {
    TB_ENTER((vo ? vo->ctx : nullptr));
    if (!vo) return TB_EINVAL;
    tb_ctx* ctx = vo->ctx;
    if (!vo->mono_on) return tb_fail(ctx, TB_ESTATE, "tb_vo_mono_init_enable: the mono mode is not enabled (tb_vo_mono_enable first)");
    if (vo->next >= 0 || vo->ragged) return tb_fail(ctx, TB_ESTATE, "tb_vo_mono_init_enable after a reset");
    if (vo->mi_on) return tb_fail(ctx, TB_ESTATE, "tb_vo_mono_init_enable: enabled already");
    if (!prm) return tb_fail(ctx, TB_EINVAL, "tb_vo_mono_init_enable: null parameters");
    if (prm->min_tracks < 0 || !tb_two_view_params_ok(&prm->two_view))
        return tb_fail(ctx, TB_EINVAL, "tb_vo_mono_init_enable: min_tracks %d (>= 0), or two-view parameters tb_two_view_batch_dev refuses",
                       prm->min_tracks);
    if (vo->P > TB_TWO_VIEW_MAX_PITCH)
        return tb_fail(ctx, TB_EUNSUPPORTED, "tb_vo_mono_init_enable: key pitch %d (the two-view operator stages at most %d rows)", vo->P,
                       TB_TWO_VIEW_MAX_PITCH);
    const size_t S = (size_t)vo->nseq, SP = S * vo->P;
    tb_dev_owner& own = vo->own;
    TB_TRY(tb_dev_alloc(ctx, own, &vo->mi_initialised, S));
    TB_TRY(tb_dev_alloc(ctx, own, &vo->mi_skip, SP));
    TB_TRY(tb_dev_alloc(ctx, own, &vo->mi_pflags, SP));
    TB_TRY(tb_dev_alloc(ctx, own, &vo->mi_init_frame, S));
    TB_TRY(tb_dev_alloc(ctx, own, &vo->mi_attempts, S));
    TB_TRY(tb_dev_alloc(ctx, own, &vo->mi_w_res, S * 12));
    TB_TRY(tb_dev_alloc(ctx, own, &vo->mi_res, S * 12));
    TB_TRY(tb_dev_alloc(ctx, own, &vo->mi_w_Tcw1, S * 16));
    TB_TRY(tb_dev_alloc(ctx, own, &vo->mi_Tcw1, S * 16));
    TB_TRY(tb_dev_alloc(ctx, own, &vo->mi_points, SP * 3));
    vo->mi = *prm;
    TB_TRY(vo_mono_init_clear(vo));
    vo->mi_on = true;
    return TB_OK;
}

int tb_vo_mono_init_state_dev(tb_vo* vo, const uint8_t** initialised, const int32_t** init_frame, const int32_t** attempts,
                              const int32_t** status, const int32_t** consensus, const int32_t** winner, const int32_t** good,
                              const int32_t** tri, const float** Tcw1) {
    TB_ENTER((vo ? vo->ctx : nullptr));
    if (!vo) return TB_EINVAL;
    if (!vo->mi_on) return tb_fail(vo->ctx, TB_ESTATE, "tb_vo_mono_init_state_dev: not enabled (tb_vo_mono_init_enable)");
    const size_t S = (size_t)vo->nseq;
    if (initialised) *initialised = vo->mi_initialised;
    if (init_frame) *init_frame = vo->mi_init_frame;
    if (attempts) *attempts = vo->mi_attempts;
    if (status) *status = vo->mi_res;
    if (consensus) *consensus = vo->mi_res + S;
    if (winner) *winner = vo->mi_res + 2 * S;
    if (good) *good = vo->mi_res + 4 * S;
    if (tri) *tri = vo->mi_res + 8 * S;
    if (Tcw1) *Tcw1 = vo->mi_Tcw1;
    return TB_OK;
}

int tb_vo_mono_state_dev(tb_vo* vo, const float** kf_keys_xy, const float** kf_Tcw, const uint8_t** alive, const float** tri_points,
                         const uint8_t** tri_flags, const int32_t** tri_tally, const int32_t** survivors, const int32_t** added) {
    TB_ENTER((vo ? vo->ctx : nullptr));
    if (!vo) return TB_EINVAL;
    if (!vo->mono_on) return tb_fail(vo->ctx, TB_ESTATE, "tb_vo_mono_state_dev: the mono mode is not enabled (tb_vo_mono_enable)");
    if (kf_keys_xy) *kf_keys_xy = vo->mn_kf_keys;
    if (kf_Tcw) *kf_Tcw = vo->mn_kf_Tcw;
    if (alive) *alive = vo->mn_alive;
    if (tri_points) *tri_points = vo->mn_tri_points;
    if (tri_flags) *tri_flags = vo->mn_tri_flags;
    if (tri_tally) *tri_tally = vo->mn_tri_tally;
    if (survivors) *survivors = vo->mn_survivors;
    if (added) *added = vo->mn_added;
    return TB_OK;
}

int tb_vo_kf_store_get(tb_vo* vo, tb_kf_store** out) {
    if (!vo || !out) return TB_EINVAL;
    *out = nullptr;
    if (!vo->store) return tb_fail(vo->ctx, TB_ESTATE, "tb_vo_kf_store_get: relocalisation is not enabled");
    *out = vo->store;
    return TB_OK;
}

int tb_vo_mp_desc_dev(tb_vo* vo, const uint8_t** mp_desc, const uint8_t** kf_mp_desc) {
    TB_ENTER((vo ? vo->ctx : nullptr));
    if (!vo) return TB_EINVAL;
    if (!vo_is_proj(vo)) return tb_fail(vo->ctx, TB_ESTATE, "tb_vo_mp_desc_dev: the loop's tracker carries no map-point descriptors");
    if (mp_desc) *mp_desc = vo->out[vo->oc].mp_desc;
    if (kf_mp_desc) *kf_mp_desc = vo->kf.mp_desc;
    return TB_OK;
}

int tb_vo_map_state_dev(tb_vo* vo, const tb_mappoint** points, const uint8_t** desc, const int32_t** counts, const int32_t** block_counts,
                        int* capacity, int* map_keyframes, int* blocks) {
    TB_ENTER((vo ? vo->ctx : nullptr));
    if (!vo) return TB_EINVAL;
    if (!vo->mapK) return tb_fail(vo->ctx, TB_ESTATE, "tb_vo_map_state_dev: the loop has no map");
    const int c = vo->map_cur;
    if (points) *points = vo->map_rec[c];
    if (desc) *desc = vo->map_desc[c];
    if (counts) *counts = vo->map_n[c];
    if (block_counts) *block_counts = vo->map_blocks[c];
    if (capacity) *capacity = vo->map_cap;
    if (map_keyframes) *map_keyframes = vo->mapK;
    if (blocks) *blocks = vo->map_nblk;
    return TB_OK;
}

}  // extern "C"
