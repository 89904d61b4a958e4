/* Plain-data types that cross the C ABI of the tracking hot path.
 *
 * Layouts mirror the OpenCV 3.x types the reference's operator API passes
 * (reference: include/extractors/ORBextractor.h:38-52, include/matchers/matcher.h:39-62,
 * include/mapping/LocalBA.h:16-22) so a binding can reinterpret_cast vectors of
 * cv::KeyPoint / cv::DMatch without a copy.
 */
#ifndef TB_TYPES_H
#define TB_TYPES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* == cv::KeyPoint (28 bytes): pt.x, pt.y, size, angle, response, octave, class_id */
typedef struct tb_keypoint {
    float x, y;
    float size;
    float angle;
    float response;
    int32_t octave;
    int32_t class_id;
} tb_keypoint;

/* == cv::DMatch (16 bytes) */
typedef struct tb_match {
    int32_t queryIdx;
    int32_t trainIdx;
    int32_t imgIdx;
    float distance;
} tb_match;

/* One FAST corner: integer pixel position inside the scanned image + score. */
typedef struct tb_corner {
    int32_t x, y, score;
} tb_corner;

/* One motion-only BA observation (reference: src/mapping/LocalBA.cpp:333-363):
 * pixel (Feature::px), world point (MapPoint::GetWorldPos), information scale
 * (Frame::GetInverseScaleSigmaSquares()[octave]). */
typedef struct tb_obs {
    float u, v;
    float X, Y, Z;
    float inv_sigma2;
} tb_obs;

/* One 3D-3D row of the Sim(3) solver (tb_sim3_ransac_batch_dev), 32 bytes: the same physical point in camera-1 coordinates and
 * in camera-2 coordinates, with the invLevelSigma2 of the two keys that observe it. No pixel is stored: a row's observation in
 * image i is the projection of its own point Xi. */
typedef struct tb_sim3_row {
    float X1, Y1, Z1;
    float X2, Y2, Z2;
    float inv_sigma2_1, inv_sigma2_2;
} tb_sim3_row;

/* One pixel row of the Sim(3) optimiser (tb_sim3_optimize_batch_dev), 48 bytes: a tb_sim3_row's two points, then the pixels
 * (u1, v1) and (u2, v2) of the two keys that observe the point, then the two keys' invLevelSigma2. The first six fields and
 * the two weights mean what they mean in tb_sim3_row. */
typedef struct tb_sim3_obs_row {
    float X1, Y1, Z1;
    float X2, Y2, Z2;
    float u1, v1;
    float u2, v2;
    float inv_sigma2_1, inv_sigma2_2;
} tb_sim3_obs_row;

/* Pinhole camera as the projection matchers use it (reference PinholeCamera, CameraModel.cpp:63-93 and
 * CameraModel.h:33-39): focal lengths, principal point, image size for IsInFrame, and the radial-tangential
 * coefficients d[0..4] (k1 k2 p1 p2 k3) applied iff has_distortion. */
typedef struct tb_camera {
    float fx, fy, cx, cy;
    int32_t width, height;
    int32_t has_distortion;
    float d[5];
} tb_camera;

/* A map point as Matcher::searchByProjection / Frame::IsInFrustum read it (reference MapPoint: GetWorldPos,
 * GetNormal, Get{Min,Max}DistanceInvariance, isBad). bad != 0 also stands for "this key has no map point" where
 * the array is aligned with a frame's keys. Descriptors travel separately (32 bytes each). */
typedef struct tb_mappoint {
    float pos[3];
    float normal[3];
    float min_dist, max_dist;
    int32_t bad;
} tb_mappoint;

/* A DBoW2 vocabulary as flat arrays (reference third_part/DBoW2/DBoW2/TemplatedVocabulary.h:297-329, the tree that
 * Frame::SetBow walks, src/types/Frame.cpp:267-270). Node 0 is the root; the children of node n are
 * child_items[child_start[n] .. child_start[n + 1]) in the vocabulary's order (the order decides ties: the first child with
 * the smallest distance wins, TemplatedVocabulary.h:1231-1244); a node without children is a word and carries word_id / weight.
 * desc: 32 bytes per node (FORB::TDescriptor). k / L as in the vocabulary file's first line; weighting: 0 TF_IDF, 1 TF, 2 IDF,
 * 3 BINARY; scoring: 0 L1_NORM, 1 L2_NORM, 2 CHI_SQUARE, 3 KL, 4 BHATTACHARYYA, 5 DOT_PRODUCT (BowVector.h:36-53). */
typedef struct tb_vocabulary {
    int32_t nnodes, k, L;
    int32_t weighting, scoring;
    const int32_t* child_start;   /* nnodes + 1 */
    const int32_t* child_items;   /* child_start[nnodes] node ids */
    const uint8_t* desc;          /* nnodes x 32 */
    const int32_t* word_id;       /* nnodes, read for leaves */
    const double* weight;         /* nnodes, read for leaves (WordValue) */
} tb_vocabulary;

/* One local-BA observation: keyframe index, point index, pixel, information scale. */
typedef struct tb_ba_obs {
    int32_t kf, pt;
    float u, v;
    float inv_sigma2;
} tb_ba_obs;

/* One pose-graph edge: the measured motion Z ~ T_b T_a^-1 between nodes a and b as a unit quaternion (x, y, z, w) and a
 * translation, in FP64 -- an edge built from two stored poses has a residual of rounding size, which a float32 Z would not give --
 * and the weights of its information matrix diag(w_rot I3, w_trans I3). 80 bytes. */
typedef struct tb_pg_edge {
    int32_t a, b;
    double q[4];
    double t[3];
    double w_rot, w_trans;
} tb_pg_edge;

/* One Sim(3) pose-graph edge: the measured similarity Z ~ S_b S_a^-1 between nodes a and b in the FP64 srt layout of
 * tb_sim3_ransac_batch_dev (the quaternion w x y z, then t, then s: X_b = s R X_a + t), and the weights of its information matrix
 * diag(w_rot I3, w_trans I3, w_scale) over the residual (omega, upsilon, sigma). 96 bytes. */
typedef struct tb_pg_sim3_edge {
    int32_t a, b;
    double srt[8];
    double w_rot, w_trans, w_scale;
} tb_pg_sim3_edge;

/* What a Sim(3) graph query (tb_kf_store_sim3_graph_dev, tb_vo_loop_sim3_dev) hands back: device pointers into buffers the store
 * owns, valid until its next graph query; nn = capacity + 1 nodes and edge slots a sequence. */
typedef struct tb_sim3_graph_out {
    int nn;
    const int32_t* nnodes;        /* [nseq] live keyframes + 1 */
    const int32_t* node_kf;       /* [nseq][nn] kf_id; the query frame's node: -2 (store) or the frame index (loop); -1 unused */
    const double* before;         /* [nseq][nn][8] srt */
    const double* after;          /* [nseq][nn][8] srt */
    const tb_pg_sim3_edge* edges; /* [nseq][nn] */
    const int32_t* edge_counts;   /* [nseq] */
    const double* stats;          /* [nseq][8] tb_pose_graph_sim3_batch_dev's */
} tb_sim3_graph_out;

/* One entry of a depth filter (tb_depth_filter_*, include/tb_capi.h): the reference pixel (u, v) at level 0 and the ring slot of
 * its reference image; mu, sigma2: inverse range along the pixel's unit ray and its variance; a, b: the Beta counts of the inlier
 * ratio; z_range = 1 / depth_min; state 0 free, 1 active, 2 converged, 3 dropped; updates: the updates that reached the match
 * stage (success or NO_MATCH). 64 bytes. */
typedef struct tb_df_seed {
    double mu, sigma2, a, b, z_range;
    float u, v;
    int32_t slot, state, updates, reserved;
} tb_df_seed;

/* What the last update did with an entry: flag -1 idle (the entry was not active), 0 updated, 1 BEHIND, 2 OUTSIDE, 3 WARP,
 * 4 DEGENERATE, 5 NO_MATCH, 6 CONVERGED (updated, and the state became 2), 7 NONFINITE; n: the sample count of the epipolar search
 * (0 before step 4), win / score: the winning sample and its score (-1: none), (px, py): the aligned pixel, z: the range the two
 * rays give, tau: its uncertainty (0 where the update did not get there). 56 bytes. */
typedef struct tb_df_trace {
    int64_t score;
    double px, py, z, tau;
    int32_t flag, n, win, reserved;
} tb_df_trace;

/* Error codes (0 = ok). */
enum {
    TB_OK = 0,
    TB_EINVAL = -1,       /* bad argument (null pointer, non-positive size, ...) */
    TB_ENOMEM = -2,       /* host or device allocation failed */
    TB_ECAPACITY = -3,    /* caller-provided output capacity too small */
    TB_EUNSUPPORTED = -4, /* reference behaviour undefined/broken for this input */
    TB_EDEVICE = -5,      /* HIP runtime error; see tb_last_error() */
    TB_ESTATE = -6        /* call sequence error (e.g. AddPoints before operator()) */
};

#ifdef __cplusplus
}
#endif
#endif /* TB_TYPES_H */
