/* C ABI of the MI355X tracking hot path (libtb_hip.so).
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ or torch types.  The reference has no
 * FFI of its own (it is one C++ static library, CMakeLists.txt:30-45); the functions below are what a
 * binding for its hot-path operators would bind, one per operator, each citing the reference interface
 * it replaces.  include/extractors, include/matchers, include/mapping hold the C++ header shims that
 * keep the reference's class signatures on top of this ABI.
 *
 * Conventions: return 0 (TB_OK) or a negative TB_E* code (tb_types.h); tb_last_error(ctx) gives the text.
 * Outputs are caller-allocated with stated capacities.  A tb_ctx owns one GPU and one HIP stream and is
 * not thread-safe; contexts on different GPUs are independent.  "host" pointers are ordinary memory,
 * "dev" pointers are HIP device memory of the context's GPU.  There is NO CPU fallback: every compute
 * entry point fails with TB_EDEVICE when no gfx950 device is usable.
 */
#ifndef TB_CAPI_H
#define TB_CAPI_H

#include "tb_types.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tb_ctx tb_ctx;
typedef struct tb_extractor tb_extractor;

/* ---------------------------------------------------------------- context */
int tb_create(int device, tb_ctx** out);
void tb_destroy(tb_ctx* ctx);
const char* tb_last_error(const tb_ctx* ctx);
const char* tb_strerror(int code);
const char* tb_version(void);
/* Run everything on an existing HIP stream (e.g. torch's current stream); NULL = the context's own. */
int tb_set_stream(tb_ctx* ctx, void* hip_stream);
int tb_synchronize(tb_ctx* ctx);
/* Per-kernel timing with HIP events on the context's stream (measurement aid for bench.py: the roofline
 * figure needs the dominant kernel's average launch duration over the timed region). enable(1) resets the
 * accumulators; report() synchronises and writes one line per kernel: "name calls total_ms\n". */
int tb_profile_enable(tb_ctx* ctx, int on);
/* Time only the named kernel while profiling is enabled (NULL or "": all of them). Two event records per launch cost host
 * time and a queue packet each: with several hundred launches per step, timing every kernel inside a measured region costs
 * ~2 % of the region; timing the one kernel a roofline figure is about does not. */
int tb_profile_only(tb_ctx* ctx, const char* kernel);
/* Exchange helper ("counts first, then the live records"): the first counts[f] rows of every frame of a
 * [nframes][cap][row_bytes] record array, frame after frame, to the front of dst (same total size); *total (nullable, device,
 * int64) = the number of rows written. row_bytes a multiple of 4. Device pointers, asynchronous on the context's stream. */
int tb_pack_rows_dev(tb_ctx* ctx, const void* src, int row_bytes, int cap, const int32_t* counts, int nframes, void* dst,
                     long long* total);
/* A hint for launch shapes: `peers` contexts (this one included) are expected to run their kernels on this GPU at the same time
 * -- e.g. a batch's local-BA windows split over several contexts, each on its own stream and host thread. Kernels whose grid is
 * sized to fill the chip in one resident round (the local-BA Schur kernel) then take 1 / peers of it. Default 1. Results do not
 * depend on it beyond the order of floating-point partial sums (the number of partial systems per window follows the grid). */
int tb_set_concurrency(tb_ctx* ctx, int peers);
/* Measurement helper: copies `bytes` (a multiple of 16, 16-byte aligned device pointers) with a 16-byte-per-lane
 * kernel and returns the average seconds per copy over `reps` (HIP events on the context's stream, one untimed copy first). The
 * streaming bandwidth of the device is 2 * bytes / seconds. */
int tb_measure_copy_seconds(tb_ctx* ctx, const void* d_src, void* d_dst, size_t bytes, int reps, double* seconds);
/* Test hook: on != 0 sends every block of the cell-wise FAST kernel down its any-density path (no candidate lists; the
 * results are the same). A context setting, not an environment variable: nothing outside the caller changes which kernels run. */
int tb_debug_force_dense_fast(tb_ctx* ctx, int on);
/* Test hook: on != 0 makes the point passes of tb_local_ba / tb_local_ba_batch_dev walk the array-of-structs copy of the
 * observations in every window, also where they would read the lane-interleaved stream (tb_ba_obs_stream_positions). The
 * results are the same bit for bit. */
int tb_debug_ba_plain_obs(tb_ctx* ctx, int on);
/* Test hook: on != 0 makes every searchByBF entry point (tb_search_by_bf, tb_match_bf, tb_search_by_bf_batch_dev, the VO loop's
 * bf tracker) find its nearest neighbours with the scalar popcount kernel, also where the matrix-core kernel would run. The
 * results are the same bit for bit. */
int tb_debug_bf_scalar(tb_ctx* ctx, int on);
int tb_profile_report(tb_ctx* ctx, char* buf, int cap);

/* ---------------------------------------------------------------- a1/a2/a3: host-side scalar set-up
 * Frame::Frame scale vectors (src/types/Frame.cpp:18-29), Frame::ComputePyramid sizes (:423-424),
 * ORBExtractor::operator() per-level quota (src/extractors/ORBextractor.cpp:919-930). Pure host math. */
int tb_scale_factors(int nlevels, float scale, float* sf, float* inv_sf, float* sigma2, float* inv_sigma2);
int tb_pyramid_sizes(int width, int height, int nlevels, const float* sf, int* widths, int* heights);
int tb_orb_quotas(int nlevels, const float* sf, int target, int* quotas);

/* ---------------------------------------------------------------- batched extractor (device resident)
 * One plan = one image geometry (width x height, nlevels, scale vector) and up to max_images frames in
 * flight.  Replaces Frame::ComputePyramid (Frame.cpp:414-427) + ORBExtractor::operator()/AddPoints
 * (ORBextractor.cpp:906-978, :840-904) + FASTExtractor::operator() (FASTextractor.cpp:8-80) for a
 * whole batch of frames per call. max_target bounds `target` of later calls. */
int tb_extractor_create(tb_ctx* ctx, int width, int height, int nlevels, const float* sf,
                        const int* widths, const int* heights, /* per-level sizes; NULL = Frame.cpp:423-424 */
                        int max_images, int max_target, tb_extractor** out);
void tb_extractor_destroy(tb_extractor* ex);
/* Level-0 images: n frames, row stride `stride` bytes, frame pitch `pitch` bytes. The host form copies
 * (PCIe); the dev form only records the pointer (frames are read in place, they must stay valid). */
int tb_extractor_set_images_host(tb_extractor* ex, const uint8_t* images, int n, int stride, size_t pitch);
int tb_extractor_set_images_dev(tb_extractor* ex, const uint8_t* dev_images, int n, int stride, size_t pitch);
/* Caller-built pyramid for frame `index` (the reference's extractors take std::vector<cv::Mat>&). */
int tb_extractor_set_levels_host(tb_extractor* ex, int index, const uint8_t* const* levels, const int* strides);
/* a2: levels 1..n-1 of every frame by the cv::resize INTER_LINEAR chain. */
int tb_extractor_build_pyramid(tb_extractor* ex, int n);
int tb_extractor_get_level_host(tb_extractor* ex, int index, int level, uint8_t* out, int out_stride);
/* a3-a10: ORB extraction of frames [0,n). quota_mode 0 = operator() (quotas from target), 1 = AddPoints
 * (reuse the quotas of the last quota_mode-0 call; TB_ESTATE if none). exit keys (host, may be NULL)
 * apply to every frame of the call. Results stay on the device. */
int tb_extractor_orb(tb_extractor* ex, int n, int target, float init_th, float min_th, int quota_mode,
                     const tb_keypoint* exit_keys, int n_exit);
/* a11: FASTExtractor grid extraction (no descriptors). occupancy: host bytes, may be NULL. */
int tb_extractor_fastgrid(tb_extractor* ex, int n, const float* inv_sf, int target, float threshold,
                          const uint8_t* occupancy, int n_occupancy);
/* Results of the last extraction call. counts: n ints (keypoints per frame). */
int tb_extractor_counts_host(tb_extractor* ex, int n, int* counts);
int tb_extractor_results_host(tb_extractor* ex, int index, tb_keypoint* kps, uint8_t* desc, int cap, int* count);
/* Device views (valid until the next extraction call): keypoints [max_images][kp_capacity],
 * descriptors [max_images][kp_capacity][32], counts [max_images]. */
int tb_extractor_results_dev(tb_extractor* ex, const tb_keypoint** kps, const uint8_t** desc,
                             const int32_t** counts, int* kp_capacity);
/* Copy the results of frames [0,n) into caller-owned device buffers (e.g. torch tensors that feed the
 * RCCL gather): kps [n][cap], desc [n][cap][32], counts [n]; cap >= the plan's kp_capacity is not required,
 * rows beyond cap are dropped (counts are clamped). Asynchronous on the context's stream. */
int tb_extractor_copy_results_dev(tb_extractor* ex, int n, tb_keypoint* kps, uint8_t* desc, int32_t* counts, int cap);
/* Stage probes for parity tests: FAST candidates of one level after the cell loop (a4). */
int tb_extractor_candidates_host(tb_extractor* ex, int index, int level, tb_corner* out, int cap, int* count);

/* ---------------------------------------------------------------- single-frame operator forms (host buffers)
 * What the header shims call; each wraps a cached plan. */
/* Frame::ComputePyramid: levels[i] (i>=1) receive widths[i] x heights[i] bytes at strides[i]. */
int tb_pyramid(tb_ctx* ctx, const uint8_t* image, int width, int height, int stride, int nlevels,
               const float* sf, uint8_t* const* levels_out, const int* strides_out);
/* cv::FAST(img, kps, th, nms) TYPE_9_16 on a whole image (the primitive inside a4; raster order). */
int tb_fast_detect(tb_ctx* ctx, const uint8_t* image, int width, int height, int stride, int threshold,
                   int nms, tb_corner* out, int cap, int* count);
/* ORBExtractor::operator() (use_quotas 0) / AddPoints (use_quotas 1), ORBextractor.cpp:906-978,:840-904 */
int tb_orb_extract(tb_ctx* ctx, const uint8_t* const* levels, const int* widths, const int* heights,
                   const int* strides, int nlevels, const float* sf, int target, float init_th, float min_th,
                   const tb_keypoint* exit_keys, int n_exit, int use_quotas, int* quotas_inout,
                   tb_keypoint* kps, uint8_t* desc, int cap, int* count);
/* FASTExtractor::operator(), FASTextractor.cpp:8-80 */
int tb_fastgrid_extract(tb_ctx* ctx, const uint8_t* const* levels, const int* widths, const int* heights,
                        const int* strides, int nlevels, const float* inv_sf, int target, float threshold,
                        const uint8_t* occupancy, int n_occupancy, tb_keypoint* kps, int cap, int* count);

/* ---------------------------------------------------------------- matchers
 * Matcher::DescriptorDistance / ComputeThreeMaxima (matcher.cpp:793-851): host helpers.
 * The matcher host forms (out, cap, *count) list at most cap matches: more is TB_ECAPACITY with the full count in *count
 * and out not written. */
int tb_descriptor_distance(const uint8_t* a, const uint8_t* b);
void tb_three_maxima(const int* bin_sizes, int nbins, int* ind1, int* ind2, int* ind3);
/* cv::BFMatcher(NORM_HAMMING, crossCheck).match (the call inside searchByBF, matcher.cpp:207) */
int tb_match_bf(tb_ctx* ctx, const uint8_t* d1, int n1, const uint8_t* d2, int n2, int crosscheck,
                tb_match* out, int cap, int* count);
/* Matcher::searchByBF whole-set branch, matcher.cpp:168-228 */
int tb_search_by_bf(tb_ctx* ctx, const uint8_t* d1, int n1, const uint8_t* d2, int n2, float ratio,
                    float min_th, tb_match* out, int cap, int* count);
/* Batched device form: npairs descriptor-set pairs, set p of side s at desc_s + p*set_pitch bytes with
 * counts_s[p] rows; matches to out + p*cap, counts to out_counts[p]. All pointers are device memory. */
int tb_search_by_bf_batch_dev(tb_ctx* ctx, int npairs, const uint8_t* desc1, const int32_t* counts1,
                              const uint8_t* desc2, const int32_t* counts2, size_t set_pitch,
                              float ratio, float min_th, tb_match* out, int cap, int32_t* out_counts);

/* Matcher::searchByNN(F1, F2, MinLevel, MaxLevel, ratio, minTh), matcher.cpp:35-95 -- the tracking line test_vo_1 runs
 * (test/test_vo.cpp:213): cv::FlannBasedMatcher(new cv::flann::LshIndexParams(20, 10, 2)).match(d1, d2) (matcher.cpp:17-18)
 * followed by searchByBF's distance filter (:76-85 = :209-218). No cross-check, and the neighbour is approximate: the nearest
 * among the train descriptors that share an LSH bucket with the query. Neither OpenCV nor FLANN is part of the reference tree,
 * so the matcher is restated here and is UNPINNED against genuine OpenCV.
 *
 * The rule. Inputs: d1 [n1][32] (query, F1), d2 [n2][32] (train, F2), tables T, key_size k, multi_probe_level L, and a bit
 * table bits [T][k] of descriptor bit indices 0..255; bit b is bit b % 8 of byte b / 8 (what FLANN's size_t masks address on a
 * little-endian host).
 *   key_t(d)  = the k bits of d at bits[t][0..k). Their order inside the key does not matter: the probe set below is symmetric
 *               under a permutation of the key's bits.
 *   cand(q)   = { j < n2 : there is a t < T with popcount(key_t(d1[q]) ^ key_t(d2[j])) <= L }. This is FLANN's multi-probe walk
 *               (every xor mask with at most L bits set, over every table) stated per pair: buckets, speed levels and the
 *               visiting order cannot change it.
 *   nn(q)     = the j in cand(q) with the smallest (Hamming(d1[q], d2[j]), j) (KNNUniqueResultSet orders by distance, then index).
 * The raw list (tb_match_lsh) is, for q ascending with cand(q) not empty, (queryIdx q, trainIdx nn(q), imgIdx 0 as tb_match_bf
 * writes it, distance = (float)Hamming). A query without a candidate gives no match (convertToDMatches keeps idx >= 0 only).
 * tb_search_by_nn keeps the matches of the raw list with distance < fminf(ratio * min_d, minTh), min_d = the smallest distance
 * of the raw list, in the float expressions of tb_search_by_bf. An empty raw list, n1 == 0 or n2 == 0 give count 0 (the
 * reference would dereference min_element of an empty vector). Only the whole-set branch exists, as for searchByBF (:45-49;
 * the other branch writes rows of an empty cv::Mat): the shim and the VO loop refuse (MinLevel, MaxLevel) != (0, nLevels) and
 * MapPointOnly with TB_EUNSUPPORTED. The Map* overload (:103-157) writes rows of an empty Mat too and is not built.
 *
 * The bit table. FLANN draws it with rand(); here it is an explicit input, drawn by tb_lsh_draw_bits (a restatement of OpenCV
 * 3's LshIndex::buildIndex / LshTable<unsigned char> from memory) from the splitmix64 stream of `seed` (synth.Stream): word i
 * (i = 0, 1, ...) is mix(seed + (i + 1) * 0x9E3779B97F4A7C15). A pool starts empty. Before table t draws, a pool with fewer
 * than k entries is thrown away and refilled: a[i] = i for i < 256, then for i = 255 down to 1 the next word w of the stream
 * gives j = w % (i + 1) and a[i], a[j] are swapped (Fisher-Yates: 255 words per refill, the r-th refill reads words 255 r ..
 * 255 r + 254). Table t takes the first k entries of the pool, in pool order, and they leave the pool. (20, 10) uses 200
 * distinct bits of one pool; (30, 10) refills before table 25.
 * Deviations: the reference rebuilds its index with fresh rand() bits in every match() call, here the bits are fixed per
 * handle; and a caller may pass an explicit table (bits != NULL: seed is ignored) instead of a seed.
 * Limits: T in 1..32, k in 1..32, L in 0..k, descriptor sets of at most 8192 rows (the key pitch limit): TB_EINVAL outside.
 * An explicit table with a value above 255 or a value repeated inside one table is TB_EINVAL.
 *
 * tb_lsh_draw_bits needs no context and no GPU: out [tables][key_size]. tb_lsh_info: each output nullable, bits
 * [tables][key_size]. tb_match_lsh / tb_search_by_nn: host pointers, staged onto the batched form (more than cap matches:
 * TB_ECAPACITY with the full count in *count and out not written). tb_search_by_nn_batch_dev: device pointers laid out as
 * tb_search_by_bf_batch_dev's (set_pitch / 32 rows per set at most, which must be <= 8192); both sides' keys are computed
 * inside the call and nothing of a call survives it; no host synchronisation, no host <-> device copy. */
typedef struct tb_lsh tb_lsh;
int tb_lsh_draw_bits(int tables, int key_size, uint64_t seed, uint16_t* out);
int tb_lsh_create(tb_ctx* ctx, int tables, int key_size, int multi_probe_level, uint64_t seed, const uint16_t* bits,
                  tb_lsh** out);
void tb_lsh_destroy(tb_lsh* lsh);
int tb_lsh_info(const tb_lsh* lsh, int* tables, int* key_size, int* multi_probe_level, uint16_t* bits);
int tb_match_lsh(tb_ctx* ctx, const tb_lsh* lsh, const uint8_t* d1, int n1, const uint8_t* d2, int n2, tb_match* out, int cap,
                 int* count);
int tb_search_by_nn(tb_ctx* ctx, const tb_lsh* lsh, const uint8_t* d1, int n1, const uint8_t* d2, int n2, float ratio,
                    float min_th, tb_match* out, int cap, int* count);
int tb_search_by_nn_batch_dev(tb_ctx* ctx, const tb_lsh* lsh, int npairs, const uint8_t* desc1, const int32_t* counts1,
                              const uint8_t* desc2, const int32_t* counts2, size_t set_pitch, float ratio, float min_th,
                              tb_match* out, int cap, int32_t* out_counts);
/* Matcher::searchByViolence, matcher.cpp:299-395 (+ Frame grid, Frame.cpp:187-265). Host pointers: stages F2's lookup grid
 * and one pair for tb_search_by_violence_batch_dev, so histo_len <= 1024 (the reference uses 30). */
int tb_search_by_violence(tb_ctx* ctx, const tb_keypoint* k1, const uint8_t* d1, int n1,
                          const tb_keypoint* k2, const uint8_t* d2, int n2, int img2_width, int img2_height,
                          int min_level, int max_level, float radius, int th_low, float nratio,
                          int histo_len, int check_orientation, tb_match* out, int cap, int* count);

/* SURVEY 8(f) row 4 -- Matcher::searchByBow(F1, F2, MapPointOnly), matcher.cpp:619-721. The frames' DBoW2 feature vectors
 * (Frame::GetFeatureVector(), a std::map<NodeId, std::vector<unsigned>> filled by voc->transform(.., 4), Frame.cpp:269)
 * are INPUTS: nodesX = node ids in ascending order (the map's order), startX[nnX + 1] / itemsX = the nodes' feature index
 * lists as CSR, in insertion order. DBoW2 and its vocabulary stay outside this library (the reference tree ships no
 * vocabulary file). has_mp2 (nullable, n2 bytes): F2->GetMapPoint(i) != nullptr, read when map_point_only is set.
 * th_low / nratio / histo_len / check_orientation = the Matcher's TH_LOW / nRatio / HISTO_LENGTH / checkOrientation.
 * Matches: queryIdx = F1 key, trainIdx = F2 key, imgIdx = -1, distance = Hamming, in the reference's order. Runs
 * tb_search_by_bow_batch_dev on one pair, so histo_len <= 1024 (the reference uses 30), and a feature vector whose node ids
 * are not strictly ascending or whose offsets are out of order is TB_EINVAL. */
int tb_search_by_bow(tb_ctx* ctx, const tb_keypoint* k1, const uint8_t* d1, int n1, const uint32_t* nodes1, const int32_t* start1,
                     const uint32_t* items1, int nn1, const tb_keypoint* k2, const uint8_t* d2, int n2, const uint8_t* has_mp2,
                     const uint32_t* nodes2, const int32_t* start2, const uint32_t* items2, int nn2, int map_point_only, int th_low,
                     float nratio, int histo_len, int check_orientation, tb_match* out, int cap, int* count);

/* SURVEY 8(f) row 1 -- Matcher::searchByProjection(F1, F2), matcher.cpp:406-531 (+ Frame::GetFeaturesInArea,
 * Frame.cpp:202-255; PinholeCamera::World2Cam, CameraModel.cpp:63-93; CameraModel::IsInFrame, CameraModel.h:33-39).
 * F1 = current frame: pose Tcw1 (row-major 4x4), camera, level-0 image size (lookup-grid factors), keys k1,
 * descriptors d1 (n1 x 32), taken1[i] != 0 iff F1->GetMapPoint(i) has Observations() > 0 (nullable = none).
 * F2 = reference frame: keys k2 (octave, angle) and, aligned with them, its map points mp2 (bad != 0 also for "no
 * map point") with descriptors mp2_desc (n2 x 32). scale_factors = F1->GetScaleFactors() (nlevels entries).
 * Matches: queryIdx = F1 key, trainIdx = i2, imgIdx = -1, distance = Hamming; order as the reference emits them.
 * Runs tb_search_by_projection_batch_dev on one pair: histo_len <= 1024 and nlevels <= 32 (the reference uses 30 and 8). */
int tb_search_by_projection(tb_ctx* ctx, const float Tcw1[16], const tb_camera* cam1, int img1_width, int img1_height,
                            const tb_keypoint* k1, const uint8_t* d1, const uint8_t* taken1, int n1,
                            const tb_keypoint* k2, const tb_mappoint* mp2, const uint8_t* mp2_desc, int n2,
                            const float* scale_factors, int nlevels, float nratio, int th_high, int histo_len,
                            int check_orientation, tb_match* out, int cap, int* count);
/* Matcher::searchByProjection(map, F1, radio), matcher.cpp:539-617 (+ Frame::IsInFrustum, Frame.cpp:370-412, entered
 * with viewingCosLimit 0.5; the predicted level is the reference's constant 0). mps = map->GetAllMapPoints() in
 * order; trainIdx = index into mps. Runs tb_search_by_projection_map_batch_dev on one frame: nlevels <= 32 (the reference
 * uses 8). */
int tb_search_by_projection_map(tb_ctx* ctx, const float Tcw1[16], const tb_camera* cam1, int img1_width, int img1_height,
                                const tb_keypoint* k1, const uint8_t* d1, const uint8_t* taken1, int n1,
                                const tb_mappoint* mps, const uint8_t* mp_desc, int nmp,
                                const float* scale_factors, int nlevels, float nratio, float radio, int th_high,
                                tb_match* out, int cap, int* count);

/* SURVEY 8(f) row 3 -- Frame::AssignFeaturesToGrid (Frame.cpp:187-200, PosInGrid :257-265) for a batch of frames, on
 * the device: frame f has counts[f] keys at keys + f*key_pitch; its 120x36 lookup grid comes back as CSR,
 * cell_start + f*4321 (cell c = posX*36 + posY, last entry = total) and cell_items + f*key_pitch (key indices, inside a
 * cell in insertion = index order). img_* = level-0 image size (grid factors, swapped as in Frame.cpp:30-31).
 * Device pointers, asynchronous on the context's stream. */
int tb_frame_grid_batch_dev(tb_ctx* ctx, int nframes, const tb_keypoint* keys, const int32_t* counts, int key_pitch,
                            int img_width, int img_height, int32_t* cell_start, int32_t* cell_items);
/* Batched, device-resident Matcher::searchByProjection(F1, F2) (matcher.cpp:406-531): pair p reads Tcw1 + 16p, F1's
 * keys / descriptors / taken flags at stride pitch1 (n1[p] valid) with the lookup grid built by
 * tb_frame_grid_batch_dev, F2's keys and key-aligned map points / descriptors at stride pitch2 (n2[p] valid); cam1 and
 * scale_factors are host arrays shared by all pairs. Matches go to out + p*cap in the reference's order, their
 * number to out_counts[p] (if it exceeds cap the list is truncated, the count is not); flags[p] != 0 reports what the
 * host form returns as an error (1: a key octave outside the scale factors, 2: a rotation bin outside the histogram,
 * where the reference asserts). Device pointers, asynchronous, no host synchronisation. histo_len <= 1024. */
int tb_search_by_projection_batch_dev(tb_ctx* ctx, int npairs, const float* Tcw1, const tb_camera* cam1, int img1_width,
                                      int img1_height, const tb_keypoint* k1, const uint8_t* d1, const uint8_t* taken1,
                                      const int32_t* n1, int pitch1, const int32_t* cell_start, const int32_t* cell_items,
                                      const tb_keypoint* k2, const tb_mappoint* mp2, const uint8_t* mp2_desc,
                                      const int32_t* n2, int pitch2, const float* scale_factors, int nlevels, float nratio,
                                      int th_high, int histo_len, int check_orientation, tb_match* out, int cap,
                                      int32_t* out_counts, int32_t* flags);

/* Batched, device-resident Matcher::searchByProjection(map, F1, radio) (matcher.cpp:539-617): pair p = one current
 * frame (pose, keys, descriptors, taken flags, lookup grid as above) against a map of nmp[p] points at
 * mps + p*mp_pitch, mp_desc + p*mp_pitch*32; mp_pitch = 0 matches every frame against ONE shared map. max_nmp bounds
 * nmp[]. Matches (queryIdx = F1 key, trainIdx = map point index) to out + p*cap in map order, counts to
 * out_counts[p] (truncated list, untruncated count). Device pointers, asynchronous. */
int tb_search_by_projection_map_batch_dev(tb_ctx* ctx, int npairs, const float* Tcw1, const tb_camera* cam1, int img1_width,
                                          int img1_height, const tb_keypoint* k1, const uint8_t* d1, const uint8_t* taken1,
                                          const int32_t* n1, int pitch1, const int32_t* cell_start, const int32_t* cell_items,
                                          const tb_mappoint* mps, const uint8_t* mp_desc, const int32_t* nmp, int mp_pitch,
                                          int max_nmp, const float* scale_factors, int nlevels, float nratio, float radio,
                                          int th_high, tb_match* out, int cap, int32_t* out_counts, int32_t* flags);
/* Batched, device-resident Matcher::searchByViolence (matcher.cpp:299-395): pair p matches F1's keys (k1 / d1 at stride
 * pitch1, n1[p] valid) against F2's (stride pitch2, n2[p] valid) through F2's lookup grid from
 * tb_frame_grid_batch_dev (built over k2 with img2_*). Matches (queryIdx = F1 key, trainIdx = F2 key) go to
 * out + p*cap in the reference's order, their number to out_counts[p] (truncated list, untruncated count);
 * flags[p] = 2 reports a rotation bin outside the histogram (the reference asserts). Device pointers, asynchronous. */
int tb_search_by_violence_batch_dev(tb_ctx* ctx, int npairs, const tb_keypoint* k1, const uint8_t* d1, const int32_t* n1,
                                    int pitch1, const tb_keypoint* k2, const uint8_t* d2, const int32_t* n2, int pitch2,
                                    const int32_t* cell_start2, const int32_t* cell_items2, int img2_width, int img2_height,
                                    int min_level, int max_level, float radius, int th_low, float nratio, int histo_len,
                                    int check_orientation, tb_match* out, int cap, int32_t* out_counts, int32_t* flags);

/* SURVEY 8(f) row 4, second half -- the DBoW2 transform behind Frame::SetBow (src/types/Frame.cpp:267-270:
 * voc->transform(descriptors, mBowVec, mFeatVec, 4); third_part/DBoW2/DBoW2/TemplatedVocabulary.h:1124-1260, FORB.cpp:81-101).
 * The reference tree ships no vocabulary file, so the caller supplies the tree (tb_vocabulary: the arrays of an ORBvoc-style
 * text file, TemplatedVocabulary::loadFromTextFile :1338-1420); tb_vocab_create uploads it once per context.
 * tb_bow_transform: per descriptor the word it falls into (word_ids), that word's weight (weights; 0 = a stopped word, which
 * enters neither vector) and its ancestor at level L - levelsup (node_ids: the key of the frame's FeatureVector; the root when
 * L - levelsup <= 0; where a branch ends above that level the reference leaves the id unset -- here it is the leaf).
 * Host pointers. The BowVector / FeatureVector containers are built from these arrays (shim: Frame::SetBow; on the device:
 * the fv_keys of tb_bow_transform_batch_dev and tb_bow_vector_batch_dev). */
typedef struct tb_vocab tb_vocab;
int tb_vocab_create(tb_ctx* ctx, const tb_vocabulary* host, tb_vocab** out);
void tb_vocab_destroy(tb_vocab* v);
int tb_bow_transform(tb_ctx* ctx, const tb_vocab* voc, const uint8_t* desc, int n, int levelsup, int32_t* word_ids,
                     double* weights, int32_t* node_ids);
/* Batched, device-resident: frame f has counts[f] descriptors at desc + f * desc_pitch * 32. Outputs [nframes][desc_pitch]:
 * word_ids / node_ids / weights (each nullable), and fv_keys (nullable, uint64): the frame's FeatureVector as a sorted list --
 * (node id << 32 | feature index) of every feature whose word is not stopped, ascending, i.e. the std::map's node order
 * with every node's features in insertion order; fv_counts[f] entries. Feeds tb_search_by_bow_batch_dev. Device pointers,
 * asynchronous on the context's stream; desc_pitch <= 8192. */
int tb_bow_transform_batch_dev(tb_ctx* ctx, const tb_vocab* voc, int nframes, const uint8_t* desc, const int32_t* counts,
                               int desc_pitch, int levelsup, int32_t* word_ids, int32_t* node_ids, double* weights,
                               uint64_t* fv_keys, int32_t* fv_counts);
/* The other container of that transform, the BowVector (Frame::mBowVec), batched and device-resident: TemplatedVocabulary::
 * transform(features, v, fv, levelsup) (TemplatedVocabulary.h:1124-1188) and BowVector::normalize (BowVector.cpp:57-80) on the
 * arrays tb_bow_transform_batch_dev wrote (word_ids, weights: [nframes][desc_pitch], counts[f] of them valid). Per frame one sorted
 * list, [nframes][desc_pitch]: bv_words ascending (the std::map's order), bv_values beside them, bv_counts[f] entries.
 *  - a stopped word (weight 0) does not enter the vector;
 *  - TF and TF_IDF add a word's weights in ascending feature index, IDF and BINARY keep the first;
 *  - TF and TF_IDF under a scoring object that does not normalise (DOT_PRODUCT) divide by the number of words in the vector;
 *  - otherwise the vector is divided by its L1 norm, or its L2 norm (L2_NORM: sqrt of the squares' sum), summed in ascending word
 *    order by one thread and applied only when it is greater than 0.
 * Weighting and scoring are the tb_vocab's. The values are doubles and come out bit for bit as DBoW2's: one operation per
 * statement, no FMA, no tree reduction. Device pointers, asynchronous on the context's stream; desc_pitch <= 8192; null or
 * inconsistent arguments are TB_EINVAL. Two such vectors are scored by tb_bow_score* below. */
int tb_bow_vector_batch_dev(tb_ctx* ctx, const tb_vocab* voc, int nframes, const int32_t* word_ids, const double* weights,
                            const int32_t* counts, int desc_pitch, int32_t* bv_words, double* bv_values, int32_t* bv_counts);
/* Scoring two BowVectors -- TemplatedVocabulary::score(v1, v2) (third_part/DBoW2/DBoW2/TemplatedVocabulary.h:156-162, :1199-1203),
 * which forwards to the vocabulary's scoring object (ScoringObject.cpp:23-311). A vector is the sorted list tb_bow_vector_batch_dev
 * writes: words ascending, values beside them. `scoring` is the code of tb_vocabulary (tb_types.h). One term per common word,
 * added in ascending word order into one accumulator that starts at 0, then the closing formula:
 *   0 L1_NORM        fabs(vi - wi) - fabs(vi) - fabs(wi)            -score / 2.0                                  (:23-68)
 *   1 L2_NORM        vi * wi                                        score >= 1 ? 1.0 : 1.0 - sqrt(1.0 - score)    (:73-120)
 *   2 CHI_SQUARE     vi * wi / (vi + wi) where vi + wi != 0.0       2. * score                                    (:125-170)
 *   3 KL             vi * log(vi / wi) where both are non-zero; a word of v1 alone that lies before a word of v2 adds
 *                    vi * (log(vi) - LOG_EPS), and so does one past v2's last word when vi != 0; LOG_EPS = log(DBL_EPSILON)
 *                    (:18, :175-221). Not symmetric: v1 (a) is the query. Lower is more similar; for the other five, higher
 *   4 BHATTACHARYYA  sqrt(vi * wi)                                                                                (:226-266)
 *   5 DOT_PRODUCT    vi * wi                                                                                      (:271-311)
 * Codes 0, 1, 2, 4, 5 come out bit for bit on the host and on the device: one rounding per statement, IEEE division and sqrt, the
 * terms of a pair computed in parallel and added serially in word order (no tree, no per-lane partial sums). KL keeps the order;
 * its log is the C library's on the host and the device library's on the device.
 * tb_bow_score: host pointers, no context, plain C++ built with contraction off: one pair. na / nb >= 0 (a null list needs
 * a count of 0).
 * tb_bow_score_batch_dev: device pointers, lists [n][pitch] with counts [n] (clamped to 0 .. pitch), asynchronous on the
 * context's stream. mode TB_SCORE_PAIRWISE: na == nb, out[i] = score(a_i, b_i); TB_SCORE_ALL_PAIRS: out[i * nb + j] =
 * score(a_i, b_j). Pitches in 1..8192 (a query is staged in LDS). TB_EINVAL: null or inconsistent arguments, scoring outside
 * 0..5, another mode, a pitch out of range. */
enum { TB_SCORE_PAIRWISE = 0, TB_SCORE_ALL_PAIRS = 1 };
int tb_bow_score(int scoring, const int32_t* a_words, const double* a_values, int na, const int32_t* b_words, const double* b_values,
                 int nb, double* out);
int tb_bow_score_batch_dev(tb_ctx* ctx, int scoring, int mode, int na, const int32_t* a_words, const double* a_values,
                           const int32_t* a_counts, int a_pitch, int nb, const int32_t* b_words, const double* b_values,
                           const int32_t* b_counts, int b_pitch, double* out);
/* A device-resident keyframe database: per sequence a ring of the last `capacity` keyframes' BowVectors, scored by
 * TemplatedVocabulary::score as above. (DBoW2's TemplatedDatabase and its inverted index are not part of the reference's tree:
 * a query scores every held entry.) All nseq sequences step together.
 *   add    add number a (0, 1, ...) puts sequence s's vector (bv_* [nseq][src_pitch], bv_counts [nseq]) into slot a % capacity
 *          of every sequence, overwriting the oldest, with kf_id (>= 0). The host counts the adds, so nothing is read back
 *   query  q_* [nseq][q_pitch]: sequence s's query is v1, scored against the slots of its own ring into scores [nseq][capacity].
 *          A slot that is empty, or among the exclude_newest most recent adds, is not ranked and its score is a quiet NaN.
 *          top_slot / top_kf / top_score [nseq][topk] list the best min(topk, ranked) slots, best first: descending score
 *          (ascending for KL), ties to the lower kf_id, then to the lower slot; the unused tail holds -1 (top_score: a quiet
 *          NaN, as in scores); top_count [nseq] (nullable) = the entries listed. With topk 0 the top_* arrays may be NULL
 *   state  device views: words / values [nseq][capacity][pitch], counts and kf_ids [nseq][capacity] (-1 = empty), *nadded
 * Add, query and clear are asynchronous on the context's stream and make no host <-> device copy. The database must be
 * destroyed before its context. TB_EINVAL: null or inconsistent arguments, scoring outside 0..5, nseq < 1, capacity outside
 * 1..1024, pitch outside 1..8192, kf_id < 0, topk < 0 or > capacity, exclude_newest < 0, a source or query pitch < 1 or larger
 * than the database's. */
typedef struct tb_bow_db tb_bow_db;
int tb_bow_db_create(tb_ctx* ctx, int nseq, int capacity, int pitch, int scoring, tb_bow_db** out);
void tb_bow_db_destroy(tb_bow_db* db);
int tb_bow_db_clear(tb_bow_db* db);
int tb_bow_db_add_dev(tb_bow_db* db, const int32_t* bv_words, const double* bv_values, const int32_t* bv_counts, int src_pitch,
                      int32_t kf_id);
int tb_bow_db_query_dev(tb_bow_db* db, const int32_t* q_words, const double* q_values, const int32_t* q_counts, int q_pitch,
                        int exclude_newest, int topk, double* scores, int32_t* top_slot, int32_t* top_kf, double* top_score,
                        int32_t* top_count);
int tb_bow_db_state_dev(tb_bow_db* db, const int32_t** words, const double** values, const int32_t** counts, const int32_t** kf_ids,
                        int* nadded);
/* A device-resident keyframe store and the verification of keyframe-database candidates: a relocalisation pose.
 * tb_bow_db ranks keyframes by their BowVectors; a candidate is verified as ORB-SLAM verifies one, with the reference's own
 * operators: Matcher::searchByBow (matcher.cpp:619-721) of the query frame against the stored keyframe, PoseOptimization's rows
 * through the matches (LocalBA.cpp:333-363) and LocalBA::PoseOptimization (LocalBA.cpp:291-490) seeded with the keyframe's pose.
 * The reference has no such step; the composition is this library's (tests/reloc_reference.py restates it on the CPU oracle).
 *
 * tb_kf_store: per sequence a ring of `capacity` keyframes, ring-aligned with tb_bow_db (add number a goes to slot a % capacity of
 * every sequence, the host counts the adds, kf_id -1 = empty). A slot holds the key count, tb_keypoint[pitch], descriptors
 * [pitch][32], FeatureVector keys uint64[pitch] with their count, map points float[pitch][3] with uint8 validity, Tcw[16], kf_id.
 *   add    the snapshot's arrays [nseq][src_pitch] (counts / fv_counts [nseq], clamped to both pitches) and Tcw [nseq][16] into
 *          the next slot with kf_id (>= 0): only the live entries are copied
 *   state  device views [nseq][capacity][pitch] (counts, fv_counts, kf_ids [nseq][capacity]; Tcw [nseq][capacity][16]), *nadded
 * Add, clear and state are asynchronous on the context's stream and copy nothing to the host. The store owns the verification's
 * work buffers, sized at create for nseq * max_candidates pairs, so a verification allocates nothing. TB_EINVAL: null or
 * inconsistent arguments, nseq < 1, capacity outside 1..1024, pitch outside 1..8192, max_candidates outside 1..capacity,
 * nseq * max_candidates > 65535, kf_id < 0, a source pitch < 1 or larger than the store's. Destroy it before its context.
 *
 * tb_relocalize_batch_dev: the query frames [nseq][q_pitch] (keys, descriptors, FeatureVector keys with fv_counts; counts = the
 * key counts) against the candidates cand_slot [nseq][ncand] (device, int32 ring slots, exactly tb_bow_db_query_dev's top_slot;
 * -1, a slot outside the ring or an empty slot = no candidate). Pair c = s * ncand + r is sequence s, rank r:
 *   match   searchByBow(query s, stored keyframe, map_point_only) with has_mp2 = the stored validity and the Matcher's fields of
 *           tb_reloc_params; the stored keyframe is read in place and the query is not replicated
 *   rows    the descriptor trackers' rule (tb_vo_tracker): a match counts where the stored entry trainIdx has a map point, the last
 *           match in list order wins a key, rows in key order: px = the query key, Xw = the stored map point, invSigma2 =
 *           invLevelSigma2[octave] as tb_scale_factors(nlevels, scale) gives it; outlier flags cleared
 *   pose    tb_pose_opt_batch_dev's kernel on nseq * ncand problems, seeded with the stored keyframe's Tcw: fewer than 3 rows keep
 *           the seed and give 0 inliers. Without a candidate: counts 0, cand_kf -1, the identity
 *   select  per sequence the candidate with the most inliers, ties to the lower rank (candidates that are absent never win);
 *           best_rank[s] = its rank if its inliers >= min_inliers, else -1; best_kf[s] its kf_id or -1; best_Tcw[s] its pose, or
 *           the identity when -1
 * tb_reloc_out (every pointer nullable, device): cand_kf / cand_matches / cand_rows / cand_inliers / cand_flags [nseq][ncand]
 * (flags: searchByBow's), cand_Tcw [nseq][ncand][16], best_rank / best_kf [nseq], best_Tcw [nseq][16]. The call makes no host
 * synchronisation and no host <-> device copy. min_inliers is the caller's: ORB-SLAM's relocalisation asks for 50, the reference
 * has no figure. TB_EINVAL: ncand outside 1..max_candidates, q_pitch < 1 or larger than the store's, nlevels outside
 * 1..16, histo_len outside 1..1024, null inputs.
 * tb_reloc_rows_dev runs the rows stage alone on match lists the caller wrote into the work buffer (tb_kf_store_work_dev's
 * matches, match_counts [nseq * ncand]); cand_rows nullable. tb_kf_store_work_dev lends the last call's work: matches
 * [pairs][pitch], rows tb_obs [pairs][pitch] with row_counts [pairs], outlier flags [pairs][pitch] (of the rows, after the pose
 * stage), *pitch = the store's. */
typedef struct tb_kf_store tb_kf_store;
typedef struct tb_reloc_params {
    int map_point_only, th_low; float nratio; int histo_len, check_orientation;   /* searchByBow's, as in tb_vo_bow */
    int min_inliers;
} tb_reloc_params;
typedef struct tb_reloc_out {
    int32_t *cand_kf, *cand_matches, *cand_rows, *cand_inliers, *cand_flags;
    float* cand_Tcw;
    int32_t *best_rank, *best_kf;
    float* best_Tcw;
} tb_reloc_out;
int tb_kf_store_create(tb_ctx* ctx, int nseq, int capacity, int pitch, int max_candidates, tb_kf_store** out);
void tb_kf_store_destroy(tb_kf_store* st);
int tb_kf_store_clear(tb_kf_store* st);
int tb_kf_store_add_dev(tb_kf_store* st, const tb_keypoint* keys, const uint8_t* desc, const int32_t* counts, const uint64_t* fv_keys,
                        const int32_t* fv_counts, const float* map_points, const uint8_t* mp_valid, int src_pitch, const float* Tcw,
                        int32_t kf_id);
int tb_kf_store_state_dev(tb_kf_store* st, const tb_keypoint** keys, const uint8_t** desc, const int32_t** counts,
                          const uint64_t** fv_keys, const int32_t** fv_counts, const float** map_points, const uint8_t** mp_valid,
                          const float** Tcw, const int32_t** kf_ids, int* nadded);
int tb_kf_store_work_dev(tb_kf_store* st, tb_match** matches, int32_t** match_counts, const tb_obs** rows, const int32_t** row_counts,
                         const uint8_t** outlier, int* pitch);
int tb_relocalize_batch_dev(tb_kf_store* st, const double K[4], int nlevels, float scale, const tb_keypoint* q_keys,
                            const uint8_t* q_desc, const int32_t* q_counts, const uint64_t* q_fv_keys, const int32_t* q_fv_counts,
                            int q_pitch, const int32_t* cand_slot, int ncand, const tb_reloc_params* params, const tb_reloc_out* out);
int tb_reloc_rows_dev(tb_kf_store* st, int nlevels, float scale, const tb_keypoint* q_keys, const int32_t* q_counts, int q_pitch,
                      const int32_t* cand_slot, int ncand, const int32_t* match_counts, int32_t* cand_rows);
/* PnP in front of the pose stage (off unless enabled: a store that does not call it launches exactly what it launched before, and
 * tb_relocalize_batch_dev's signature, tb_reloc_params and tb_reloc_out do not change). The pose stage above trusts the stored
 * keyframe's pose as its seed; from a few metres away, or on a match list that is mostly wrong, PoseOptimization keeps nothing
 * although the good rows are there. With tb_kf_store_pnp_enable(params (null: 256, 5.991, 0), min_consensus, expand) these stages
 * run between rows and pose, per pair (tests/reloc_pnp_reference.py restates the composition on the CPU):
 *   pnp      tb_pnp_ransac_batch_dev's kernel on the pair's rows with the stored Tcw as the prior
 *   gather   consensus >= min_consensus (ORB-SLAM's minInliers is 10): the pair takes the PnP path -- its rows become the
 *            consensus rows, in key order, and the pose stage is seeded with the PnP pose. Otherwise the pair runs as without
 *            PnP, all rows and the stored seed, and its outputs are the same bytes
 *   pose     as above, on the gathered rows
 *   expand   (expand = 1) for a pair on the PnP path: every original row that is an inlier of the optimised pose (the RANSAC's
 *            rule, on the float32 pose) in key order, and the pose stage once more, seeded with the optimised pose; its pose, inlier
 *            count, rows and flags replace the first stage's
 * cand_rows is the number of rows the pair's last pose stage ran on; tb_kf_store_work_dev's rows / row_counts / outlier are
 * those rows. Selection is unchanged. Every buffer is allocated at enable, the second rows buffer only with expand: a
 * verification still allocates nothing. TB_ESTATE: enabled already; TB_EINVAL: hypotheses outside 1..1024, chi2_max, min_consensus
 * < 3, expand not 0 or 1.
 * tb_kf_store_pnp_state_dev lends device views of the last call's per-pair PnP outputs (each nullable): the rows before the gather
 * [pairs][pitch] with row_counts [pairs], consensus [pairs], winner [pairs][2], the PnP pose Tcw [pairs][16], took [pairs] bytes
 * (1: the pair took the PnP path), flags [pairs]. TB_ESTATE when not enabled. */
struct tb_pnp_params;   /* below, with tb_pnp_ransac_batch_dev */
int tb_kf_store_pnp_enable(tb_kf_store* st, const struct tb_pnp_params* params, int min_consensus, int expand);
int tb_kf_store_pnp_state_dev(tb_kf_store* st, const tb_obs** rows, const int32_t** row_counts, const int32_t** consensus,
                              const int32_t** winner, const float** Tcw, const uint8_t** took, const int32_t** flags);
/* A similarity transform between the query frame's own map and each candidate's stored map: a separate query after a
 * tb_relocalize_batch_dev, whose match lists (tb_kf_store_work_dev's matches / match_counts per pair c = s * ncand + r) it reads.
 * It changes no existing signature, struct or buffer: a store that never calls it launches what it launched before. The pose
 * stage above measures the camera against the stored map, an SE(3) that cannot see scale; this one relates the two maps, which
 * is what a loop closure on a drifted map needs (tests/reloc_sim3_reference.py restates rows and select on the CPU). The query
 * frame brings its keys q_keys [nseq][q_pitch] with q_counts, its map points q_map_points [nseq][q_pitch][3] (world) with
 * q_mp_valid [nseq][q_pitch] and its pose q_Tcw [nseq][16]; cand_slot [nseq][ncand] as tb_relocalize_batch_dev took it.
 *   rows    one workgroup per pair, by the rows stage's rule: a match counts where the stored entry trainIdx AND the query key
 *           queryIdx both have a valid map point, the last match in list order wins a key, rows in key order. X1 = q_Tcw[s]
 *           applied to the query key's world point, X2 = the stored keyframe's Tcw applied to its stored world point, both in
 *           float64 (((T0 X + T1 Y) + T2 Z) + T3) and stored as float32; inv_sigma2_1 / _2 = invLevelSigma2[octave] of the two
 *           keys as tb_scale_factors(nlevels, scale) gives it. No candidate: no rows
 *   sim3    tb_sim3_ransac_batch_dev's kernel on the nseq * ncand problems
 *   select  per sequence the candidate with the largest consensus, ties to the lower rank (candidates that are absent never
 *           win); best_rank[s] = its rank if its consensus >= min_consensus, else -1; best_kf[s] its kf_id or -1; best_S12 /
 *           best_srt its transform, or the identity and scale 1 when -1
 * tb_sim3_out (every pointer nullable, device): cand_rows / cand_consensus / cand_flags [nseq][ncand], cand_S12
 * [nseq][ncand][16] float, cand_srt [nseq][ncand][8] double, best_rank / best_kf [nseq], best_S12 [nseq][16], best_srt [nseq][8].
 * min_consensus is the caller's: ORB-SLAM's loop closing asks for 20, the reference has no figure. The rows, their masks and the
 * per-pair outputs a caller does not take live in buffers the store allocates ON THE FIRST CALL, sized for nseq * max_candidates
 * pairs: the first call may allocate, later ones do not. No host synchronisation and no host <-> device copy otherwise.
 * TB_ESTATE: no verification has filled the match lists yet. TB_EINVAL: as tb_sim3_ransac_batch_dev, null inputs, ncand outside
 * 1..max_candidates or not the last verification's, q_pitch < 1 or larger than the store's, nlevels outside 1..16, min_consensus < 0.
 * tb_kf_store_sim3_state_dev lends device views of the last call's rows [pairs][pitch], row_counts [pairs] and masks
 * [pairs][pitch] (each nullable). TB_ESTATE before the first tb_kf_store_sim3_dev. */
struct tb_sim3_params;   /* below, with tb_sim3_ransac_batch_dev */
typedef struct tb_sim3_out {
    int32_t *cand_rows, *cand_consensus, *cand_flags;
    float* cand_S12;
    double* cand_srt;
    int32_t *best_rank, *best_kf;
    float* best_S12;
    double* best_srt;
} tb_sim3_out;
int tb_kf_store_sim3_dev(tb_kf_store* st, const double K[4], int nlevels, float scale, const tb_keypoint* q_keys, const int32_t* q_counts,
                         const float* q_map_points, const uint8_t* q_mp_valid, int q_pitch, const float* q_Tcw, const int32_t* cand_slot,
                         int ncand, const struct tb_sim3_params* params, int min_consensus, const tb_sim3_out* out);
/* The Sim(3) pose graph of the stored keyframes and a query frame, with the last tb_kf_store_sim3_dev's winner as the loop edge,
 * optimised by tb_pose_graph_sim3_batch_dev: a read-only query, no ring and no work buffer of the store changes (DESIGN.md 9o;
 * tests/sim3_graph_reference.py is the composition on the CPU). The store keeps its own device copy of that call's best_kf and
 * best_srt (written by the same selection kernel), so the caller's buffers need not live on; a tb_kf_store_sim3_dev that asked for
 * no best_* output selects nothing and leaves nothing to use.
 * Per sequence, by the rules of the SE(3) loop graph (tb_vo_loop_enable): nodes are the live ring slots in ascending kf_id, then
 * the query frame q_Tcw [nseq][16] (device); which slots are live is host arithmetic on the store's count. A node is the
 * quaternion form of its float32 Tcw with s = 1; node 0 is fixed. Odometry edges Z = S_next S_prev^-1 join consecutive nodes; the
 * loop edge has a = the node of best_kf, b = the frame's node and Z = best_srt copied byte for byte (the rows were X1 = q_Tcw Xw
 * and X2 = Tcw_kf Xw', so S12 maps the keyframe's camera into the frame's). best_kf < 0 or fewer than 2 live keyframes: edge
 * count 0, nodes after = before. A best_kf the ring no longer holds: a = -1, which the solver flags (stats[7] = -1).
 * Then one launch of the solver on the nseq graphs: capacity + 1 nodes, edge pitch capacity + 1, nfixed 1. out (host struct)
 * receives device pointers into the store's buffers; they and the solver's plan are made by the first call, later calls
 * allocate nothing. Asynchronous on the context's stream, no host synchronisation, no host <-> device copy.
 * TB_ESTATE: before a tb_kf_store_sim3_dev that selected a winner (tb_kf_store_clear forgets it). TB_EINVAL: null q_Tcw / out, iters
 * outside 0..99, fixed_scale not 0 or 1, a negative or non-finite weight, a capacity above 63. */
int tb_kf_store_sim3_graph_dev(tb_kf_store* st, const float* q_Tcw, int iters, int fixed_scale, double w_rot, double w_trans, double w_scale,
                               tb_sim3_graph_out* out);
int tb_kf_store_sim3_state_dev(tb_kf_store* st, const tb_sim3_row** rows, const int32_t** row_counts, const uint8_t** inlier);
/* The Sim(3) query's candidates refined on pixels: tb_sim3_optimize_batch_dev on every candidate pair of the last
 * tb_kf_store_sim3_dev (tests/reloc_sim3_opt_reference.py is the composition on the CPU). The caller passes the
 * arguments of that Sim(3) query again -- K, the query frames' keys, map points and poses, cand_slot, ncand -- and nothing may have
 * changed in between. Stages, each one launch:
 *   rows    the pixel rows tb_sim3_obs_row by the Sim(3) query's own row rule (the same kernel, instantiated for the other row
 *           type: same keys, same order), so row i of a pair is row i of the store's tb_sim3_row list and the RANSAC mask lines
 *           up; (u1, v1) and (u2, v2) are the two keys' x, y, as tb_reloc_rows_dev takes them for its tb_obs rows
 *   seeds   a pair with no candidate, or with a consensus below 3, is skipped: it runs as an empty problem from the identity;
 *           every other pair's seed is its cand_srt
 *   refine  tb_sim3_optimize_batch_dev's kernel on the nseq * ncand problems, the active rows the Sim(3) query's inlier masks,
 *           fixed_scale and the other parameters the caller's (min_keep >= 1)
 *   select  the four outputs of every candidate, and of the candidate the Sim(3) query selected (its rule and its min_consensus;
 *           the selection is unchanged); a skipped pair is flagged stats[7] = 2 and has the identity, as has best_* where
 *           nothing was selected. With use_for_graph = 1, where the selected candidate ran (stats[7] = 0) and its refined inliers
 *           reach min_inliers (ORB-SLAM asks for 20), the store's own copy of best_srt takes the refined srt: that is the copy
 *           tb_kf_store_sim3_graph_dev reads, so the next graph query has the refined transform as its loop edge. With
 *           use_for_graph = 0 nothing of the store changes but this query's own buffers
 * After a tb_kf_store_sim3_search_dev with use_for_refine = 1 (below) the rows stage reads that query's widened match lists in place
 * of the verification's and every row starts active; nothing else differs.
 * cand_srt [nseq][ncand][8] and cand_consensus [nseq][ncand]: what the Sim(3) query wrote; each is NULL where that query was not
 * given that output, so that it is in the store's own buffer. tb_sim3_refine_out (every pointer nullable, device): cand_srt
 * [nseq][ncand][8], cand_S12 [nseq][ncand][16], cand_inliers [nseq][ncand], cand_stats [nseq][ncand][8]; best_srt [nseq][8],
 * best_S12 [nseq][16], best_inliers [nseq], best_stats [nseq][8]. Asynchronous, no host synchronisation; the first call may
 * allocate the query's buffers, a store that never calls it launches and holds what it did before.
 * TB_ESTATE: no tb_kf_store_sim3_dev since the store was made or cleared, or a tb_relocalize_batch_dev since that query (its
 * match lists are no longer the ones the query's masks and seeds belong to); cand_srt or cand_consensus NULL although the Sim(3)
 * query wrote it elsewhere; a best_* output or use_for_graph = 1 although the Sim(3) query selected nothing. TB_EINVAL: as
 * tb_sim3_optimize_batch_dev and tb_kf_store_sim3_dev, min_keep < 1, min_inliers < 0, use_for_graph not 0 or 1.
 * tb_kf_store_sim3_refine_state_dev lends device views of the last call's pixel rows [pairs][pitch], row_counts [pairs], the active
 * masks it started from (the Sim(3) query's) and the final inlier masks [pairs][pitch] (each nullable). TB_ESTATE before the first
 * tb_kf_store_sim3_refine_dev. */
struct tb_sim3_opt_params;   /* below, with tb_sim3_optimize_batch_dev */
typedef struct tb_sim3_refine_out {
    double* cand_srt;
    float* cand_S12;
    int32_t* cand_inliers;
    double* cand_stats;
    double* best_srt;
    float* best_S12;
    int32_t* best_inliers;
    double* best_stats;
} tb_sim3_refine_out;
int tb_kf_store_sim3_refine_dev(tb_kf_store* st, const double K[4], int nlevels, float scale, const tb_keypoint* q_keys, const int32_t* q_counts,
                                const float* q_map_points, const uint8_t* q_mp_valid, int q_pitch, const float* q_Tcw, const int32_t* cand_slot,
                                int ncand, const double* cand_srt, const int32_t* cand_consensus, const struct tb_sim3_opt_params* params,
                                int min_inliers, int use_for_graph, const tb_sim3_refine_out* out);
int tb_kf_store_sim3_refine_state_dev(tb_kf_store* st, const tb_sim3_obs_row** rows, const int32_t** row_counts, const uint8_t** active,
                                      const uint8_t** inlier);
/* ORB-SLAM's SearchBySim3 between the Sim(3) query and its refinement: tb_search_by_sim3_batch_dev (below, with the rules) on every
 * candidate pair of the last tb_kf_store_sim3_dev, so that OptimizeSim3 also sees the correspondences searchByBow let drop (one word of
 * the vocabulary, TH_LOW, the ratio test, the rotation histogram) although the similarity already says where they are (DESIGN.md 9r;
 * tests/reloc_sim3_search_reference.py is the composition on the CPU). Valid after a tb_kf_store_sim3_dev, with that query's arguments
 * passed again as tb_kf_store_sim3_refine_dev takes them, plus the query frames' descriptors q_desc [nseq][q_pitch][32] and the
 * image size. cand_srt / cand_consensus: what the Sim(3) query wrote (NULL where it kept them in the store); a caller may pass the
 * REFINED cand_srt instead, to search again under the refined transform. Per pair c = s * ncand + r:
 *   prep    the camera points of EVERY key of both sides, formed exactly as the row kernel forms X1 and X2 (the frame's Tcw applied to
 *           the key's world point, float64, stored as float32). A key is `already matched` if it belongs to a row of the Sim(3)
 *           query's list whose RANSAC mask is 1. A pair with no candidate or with a consensus below 3 (a flagged Sim(3) output has
 *           consensus 0) is skipped: cand_stats flag 2, no pairs, no widened list
 *   search  the operator with side 1 = the query frame, side 2 = the stored keyframe, read in place
 *   merge   the widened match list: the RANSAC-inlier rows' matches (the verification's records, as they stand) united with the new
 *           pairs, in ascending query key, one entry a key; a count goes with it
 * tb_sim3_search_out (every pointer nullable, device): cand_new [nseq][ncand] the new pairs, cand_total [nseq][ncand] the widened
 * list's length, cand_stats [nseq][ncand][8] the operator's; best_new [nseq] and best_total [nseq] for the candidate the Sim(3) query
 * selected (0 where it selected none).
 * With use_for_refine = 1 the next tb_kf_store_sim3_refine_dev builds its pixel rows from the widened lists, by the same row kernel,
 * and starts with every one of those rows active: that is what ORB-SLAM hands OptimizeSim3. Its signature, its skip rule and its
 * selection are unchanged, and tb_kf_store_sim3_refine_state_dev then shows the widened rows and an all-ones active mask;
 * tb_kf_store_work_dev and tb_kf_store_sim3_state_dev keep showing the verification's and the RANSAC's own bytes. A new
 * tb_relocalize_batch_dev, tb_kf_store_sim3_dev or tb_kf_store_clear drops the widened lists. With use_for_refine = 0 nothing of the
 * store changes but this query's own buffers. Asynchronous, no host synchronisation; the first call may allocate the query's
 * buffers, a store that never calls it launches and holds what it did before.
 * TB_ESTATE: as tb_kf_store_sim3_refine_dev's (no Sim(3) query, a tb_relocalize_batch_dev since that query, cand_srt or
 * cand_consensus NULL although the Sim(3) query wrote it elsewhere, a best_* output although nothing was selected). TB_EINVAL: as
 * tb_search_by_sim3_batch_dev and tb_kf_store_sim3_dev, use_for_refine not 0 or 1.
 * tb_kf_store_sim3_search_state_dev lends device views of the last call's match1 [pairs][q_pitch], match2 [pairs][pitch], the new
 * pairs [pairs][pitch] with pair_counts [pairs] and the widened lists [pairs][pitch] with widened_counts [pairs] (each nullable);
 * q_pitch: that call's. TB_ESTATE before the first tb_kf_store_sim3_search_dev. */
typedef struct tb_sim3_search_out {
    int32_t* cand_new;
    int32_t* cand_total;
    int32_t* cand_stats;
    int32_t* best_new;
    int32_t* best_total;
} tb_sim3_search_out;
int tb_kf_store_sim3_search_dev(tb_kf_store* st, const double K[4], int width, int height, int nlevels, float scale, const tb_keypoint* q_keys,
                                const uint8_t* q_desc, const int32_t* q_counts, const float* q_map_points, const uint8_t* q_mp_valid, int q_pitch,
                                const float* q_Tcw, const int32_t* cand_slot, int ncand, const double* cand_srt, const int32_t* cand_consensus,
                                float th, int th_high, int use_for_refine, const tb_sim3_search_out* out);
int tb_kf_store_sim3_search_state_dev(tb_kf_store* st, const int32_t** match1, const int32_t** match2, const tb_match** pairs,
                                      const int32_t** pair_counts, const tb_match** widened, const int32_t** widened_counts, int* q_pitch);
/* Batched, device-resident Matcher::searchByBow(F1, F2, MapPointOnly) (matcher.cpp:619-721) on feature vectors in the
 * list form above, grouped by ascending node id (inside a node, list order is the visiting order): pair p matches frame p
 * of side 1 against frame p of side 2 (keys / descriptors [npairs][pitchX], fv keys [npairs][pitchX] with fv_countsX[p]
 * entries; has_mp2 nullable [npairs][pitch2]). Matches [npairs][cap] in the reference's order, out_counts[p]; flags[p] != 0:
 * a rotation bin outside the histogram (the reference asserts). */
int tb_search_by_bow_batch_dev(tb_ctx* ctx, int npairs, const tb_keypoint* k1, const uint8_t* d1, int pitch1,
                               const uint64_t* fv1, const int32_t* fv_counts1, const tb_keypoint* k2, const uint8_t* d2, int pitch2,
                               const uint64_t* fv2, const int32_t* fv_counts2, const uint8_t* has_mp2, int map_point_only,
                               int th_low, float nratio, int histo_len, int check_orientation, tb_match* out, int cap,
                               int32_t* out_counts, int32_t* flags);

/* Vocabulary training -- TemplatedVocabulary<FORB::TDescriptor, FORB>::create(training_features, k, L, weighting, scoring)
 * (third_part/DBoW2/DBoW2/TemplatedVocabulary.h:558-616; HKmeansStep :642-819, initiateClustersKMpp :833-913, createWords
 * :918-938, setNodeWeights :943-996; FORB::meanValue / distance, FORB.cpp:28-101) on the device, bit for bit:
 *  - root = node 0; a node with n <= k descriptors gets one child per descriptor; a larger one runs Hamming k-means: kmeans++
 *    seeding with D(x) weights (a point at distance 0 is never updated, the next centre is the first index whose running sum
 *    is >= cut_d, seeding stops when the distances sum to 0, so a node of identical descriptors gets one child), then
 *    bit-majority centres (bit set iff count >= n/2 + n%2; a group of one keeps its descriptor) and first-minimum association
 *    until the association repeats;
 *  - children are made for every cluster, then each child with more than one descriptor is expanded while level < L; node ids
 *    follow create's recursion: a node's children get consecutive ids, then the first child's subtree, then the second's;
 *  - words = childless nodes other than the root in id order; weight 1 for TF / BINARY, log(ndocs / Ni) for TF_IDF / IDF with
 *    Ni = documents with a descriptor whose transform() walk ends in the word (C library log of the double quotient, on the
 *    host); a word no training descriptor walks to keeps weight 0.
 * Deviations from the reference:
 *  1. random numbers: the reference seeds rand() from the clock (DUtils/Random.cpp:18-22). Here every k-means node draws from the
 *     counter-based splitmix64 stream (synth.Stream) of seed + (level << 40) + j: level = the level of the children being made
 *     (1 for the root's), j = the rank of the parent among all nodes of the previous level in (parent rank, child index) order.
 *     Draw 0 gives the first centre int(u n), u = (u64 >> 11) 2^-53; every further centre takes the next draw, cut_d = u *
 *     dist_sum (one double multiply), redrawn while cut_d == 0.0;
 *  2. empty cluster: meanValue of an empty group releases the Mat and the reference then reads an empty Mat; here the cluster
 *     keeps its last centre. stats.empty_clusters counts the children that end with no descriptor;
 *  3. iteration cap: the reference loops without bound; here a node stops after its max_iters-th association with the centres
 *     used for it. stats.capped_nodes counts the nodes stopped that way (the association differed from the one before, or
 *     max_iters is 1). stats.iters_per_level[l - 1]: associations run for the children of level l (0: no k-means node).
 * Limits: 2 <= k <= 32, 1 <= L <= TB_VOC_MAX_L, at most 2^26 descriptors in all (TB_EUNSUPPORTED beyond); max_iters >= 1,
 * ndocs >= 0, 0 <= counts[d] <= desc_pitch (TB_EINVAL). No descriptors at all give the root alone (:645).
 * tb_vocab_train_dev: document d has counts[d] descriptors at desc + d * desc_pitch * 32 (device pointers; what lies beyond
 * counts[d] is not read). tb_vocab_train: host pointers, the documents concatenated; staged onto the _dev form. Both
 * synchronise the context's stream. The handle is an ordinary tb_vocab (tb_bow_transform*, tb_vocab_destroy).
 * tb_vocab_info / tb_vocab_export read any tb_vocab back (host arrays of tb_vocabulary's shapes: child_start [nnodes + 1],
 * child_items [nnodes - 1], desc [nnodes][32], word_id / weight [nnodes]; each nullable). */
#define TB_VOC_MAX_L 8
typedef struct tb_vocab_train_params { int k, L, weighting, scoring; uint64_t seed; int max_iters; } tb_vocab_train_params;
typedef struct tb_vocab_train_stats { int nnodes, nwords, capped_nodes, empty_clusters; int iters_per_level[TB_VOC_MAX_L]; } tb_vocab_train_stats;
int tb_vocab_train_dev(tb_ctx* ctx, const tb_vocab_train_params* params, int ndocs, const uint8_t* desc, const int32_t* counts,
                       int desc_pitch, tb_vocab** out, tb_vocab_train_stats* stats);
int tb_vocab_train(tb_ctx* ctx, const tb_vocab_train_params* params, int ndocs, const uint8_t* desc, const int32_t* counts,
                   tb_vocab** out, tb_vocab_train_stats* stats);
int tb_vocab_info(const tb_vocab* voc, int* nnodes, int* nwords, int* k, int* L, int* weighting, int* scoring);
int tb_vocab_export(const tb_vocab* voc, int32_t* child_start, int32_t* child_items, uint8_t* desc, int32_t* word_id, double* weight);

/* Stereo tracks -> PoseOptimization's inputs, batched and device-resident (round 3). For frame f and each of its
 * match_counts[f] left <-> right matches (queryIdx = left key, trainIdx = right key; the output of
 * tb_search_by_bf_batch_dev): Depth = bf / |x_right - x_left| (LocalBA::AddMapPointsByStereo, LocalBA.cpp:60-64), the map
 * point = the left key back-projected with that depth (test/test_vo.cpp:257-267), observed at the right key's pixel with
 * invSigma2[octave of the right key] (LocalBA.cpp:333-363) -- one tb_obs row per match, in match order; matches without
 * disparity or with an octave outside the table are dropped. keys_left / keys_right: [nframes][key_pitch] records; K = fx, fy,
 * cx, cy; inv_sigma2: nlevels floats (host; tb_scale_factors). obs [nframes][obs_pitch], obs_counts [nframes]. Device
 * pointers except K / inv_sigma2; asynchronous on the context's stream. PoseOptimization started at the identity on these rows
 * finds the right camera's pose. */
int tb_stereo_tracks_to_obs_batch_dev(tb_ctx* ctx, int nframes, const tb_keypoint* keys_left, const tb_keypoint* keys_right,
                                      int key_pitch, const tb_match* matches, const int32_t* match_counts, int match_pitch,
                                      const float K[4], float bf, const float* inv_sigma2, int nlevels, tb_obs* obs, int obs_pitch,
                                      int32_t* obs_counts);

/* ---------------------------------------------------------------- pose optimisation / local BA
 * LocalBA::PoseOptimization, LocalBA.cpp:291-490. K = fx,fy,cx,cy. Tcw_in/out: row-major 4x4.
 * outlier: n in/out flags (Frame::GetOutlier/SetOutlier). *n_inliers = nInitialCorrespondences - nBad.
 * stats (nullable, 8 doubles): LM iterations, final robust chi2, final lambda, nBad, t[3], q.w. */
int tb_pose_opt(tb_ctx* ctx, const double K[4], const float Tcw_in[16], const tb_obs* obs, int n,
                uint8_t* outlier, float Tcw_out[16], int* n_inliers, double* stats);
/* Batched device form: problem p reads obs + p*obs_pitch (counts[p] rows), Tcw_in + 16p, outlier +
 * p*obs_pitch; writes Tcw_out + 16p, n_inliers[p], stats + 8p (nullable). Device pointers. */
int tb_pose_opt_batch_dev(tb_ctx* ctx, int nproblems, const double K[4], const float* Tcw_in,
                          const tb_obs* obs, const int32_t* counts, int obs_pitch, uint8_t* outlier,
                          float* Tcw_out, int32_t* n_inliers, double* stats);
/* LocalBA::LinearTriangle, LocalBA.cpp:24-43: two-view DLT with known poses, batched and device-resident, with the gates a map
 * needs before it takes the point. Per point pair, in float64, one operation per statement, only + - * / sqrt
 * (tests/triangulate_reference.py is the definition, statement for statement):
 *   pixels     x = (u - cx) / fx, y = (v - cy) / fy. DEVIATION: the reference passes px_un -- pixels -- against a bare Tcw, and
 *              its rows p * Tcw.row(2) - Tcw.row(0) describe a projection only in normalised coordinates
 *   A          the four rows of LocalBA.cpp:31-35 on (x0, y0) / Tcw0 and (x1, y1) / Tcw1
 *   solve      M = A^T A, 6 cyclic Jacobi sweeps in the pair order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) with the rotation of the
 *              shim's LocalBA::LinearTriangle, a rotation skipped only where M[p][q] == 0, no convergence test (the reference
 *              calls Eigen's JacobiSVD); the column of V at the smallest diagonal entry, the lowest index on a tie;
 *              X = V[0..2] / V[3]
 *   flags      the first failing gate decides:
 *              0  not a candidate: beyond counts[p], or skip set
 *              1  accepted: points = (float)X
 *              2  V[3] == 0, or (float)X is not finite
 *              3  the depth (row 2 of Tcw applied to X) is not above 0 in view 0 or in view 1
 *              4  parallax: the cosine of the two pixel rays R^T (x, y, 1) in the world frame is not below cos_parallax_max
 *              5  reprojection: squared pixel error * inv_sigma2 is above chi2_max in view 0 or in view 1
 * Pair p: counts[p] point pairs (pitch apart; counts nullable = pitch each); xy0 / xy1 [npairs][pitch][2] pixels in view 0 /
 * view 1; Tcw0 / Tcw1 [npairs][16]; K = fx, fy, cx, cy (host); inv_sigma2_0 / _1 [npairs][pitch] nullable (= 1); skip
 * [npairs][pitch] nullable (non-zero: not a candidate). Out: points [npairs][pitch][3] float (WRITTEN ONLY WHERE ACCEPTED), flags
 * [npairs][pitch] bytes, tally [npairs][6] int32 (how many entries of the row carry each code; code 0 counts the whole pitch).
 * Device pointers, asynchronous on the context's stream; at most 65535 pairs per call.
 * tb_linear_triangle: the host form, n point pairs of one pose pair on the batched entry (host pointers; points is zero where a
 * pair was not accepted). The shim's LocalBA::LinearTriangle keeps its own host loop. */
typedef struct tb_triangulate_params {
    double cos_parallax_max;   /* 0.9998: reject when the rays' cosine is >= this */
    double chi2_max;           /* 5.991: reject when either view's squared reprojection error * inv_sigma2 exceeds it */
} tb_triangulate_params;
int tb_linear_triangle_batch_dev(tb_ctx* ctx, int npairs, const float* xy0, const float* xy1, const int32_t* counts, int pitch,
                                 const float* Tcw0, const float* Tcw1, const double K[4], const float* inv_sigma2_0,
                                 const float* inv_sigma2_1, const uint8_t* skip, const tb_triangulate_params* prm, float* points,
                                 uint8_t* flags, int32_t* tally);
int tb_linear_triangle(tb_ctx* ctx, const float* xy0, const float* xy1, int n, const float Tcw0[16], const float Tcw1[16],
                       const double K[4], const float* inv_sigma2_0, const float* inv_sigma2_1, const uint8_t* skip,
                       const tb_triangulate_params* prm, float* points, uint8_t* flags, int32_t tally[6]);
/* A pose from 3D-2D rows without a prior: P3P hypotheses in a RANSAC, batched and device-resident. The reference has no PnP;
 * ORB-SLAM puts one in front of PoseOptimization when it relocalises, which is what this is for (DESIGN.md 9l has the
 * derivation; tests/pnp_reference.py is the definition, statement for statement, and the kernel matches it bit for bit).
 * Problem p reads counts[p] rows tb_obs (u, v, X, Y, Z, inv_sigma2) at obs + p * obs_pitch, as tb_pose_opt_batch_dev does; a
 * count is clamped to [0, obs_pitch]. K = fx, fy, cx, cy (host).
 *   sampling  counter based: draw k of hypothesis h is mix(seed + (8 h + k + 1) * 0x9E3779B97F4A7C15) (splitmix64's output
 *             function; output 8 h + k of synth.Stream(seed)); its high 32 bits times n, shifted right by 32, is a row. Draws
 *             k = 0, 1, ... are taken until three distinct rows are found or 8 are used up; a hypothesis that runs out is void.
 *             The sample depends on (seed, h, n) only, never on p: a problem gives the same bits alone and inside any batch
 *   solver    P3P in float64 with + - * / sqrt and comparisons only and fixed loop counts: the unit bearings and the squared
 *             side lengths give two homogeneous quadrics in the depths, a real root of the cubic det(D1 + g D2) = 0 (80
 *             bisections inside the Cauchy bound, 2 Newton steps) a pair of planes, each plane a quadratic: at most 4 depth
 *             triples, solutions 0, 1 from the first plane and 2, 3 from the second; R = Y X^-1 from the two edge vectors and
 *             their cross product, t = L1 y1 - R x1. Coincident or collinear samples, non-finite rows and depths that are not
 *             all positive give no solution, never a NaN pose
 *   score     every solution against all n rows in float64: a row is an inlier iff its camera depth is > 0 and
 *             ((u - u^)^2 + (v - v^)^2) * inv_sigma2 <= chi2_max. The winner has the most inliers, ties to the lower hypothesis,
 *             then the lower solution. Tcw_prior [nproblems][16] (nullable) is scored as hypothesis -1 and wins ties. Counts are
 *             integer sums; there is no floating-point atomic anywhere
 *   void      n < 3, or no prior and no hypothesis with a solution: consensus 0, winner (-2, 0), Tcw_out = the prior or the
 *             identity, an all-zero mask, flags bit 0 set
 * Out (device, each nullable): Tcw_out [nproblems][16] float (the float32 rounding of the winning float64 pose; a winning prior
 * is returned as given), consensus [nproblems], inlier [nproblems][obs_pitch] bytes (zero beyond the count), winner
 * [nproblems][2] (hypothesis, solution; (-1, 0) the prior), flags [nproblems]. Asynchronous on the context's stream, no host
 * synchronisation, no host <-> device copy, no work buffer: one launch whose state is registers and LDS. At most 65535 problems
 * per call (TB_EUNSUPPORTED). TB_EINVAL: null obs / counts / K / params, obs_pitch < 1, hypotheses outside 1..1024, chi2_max
 * negative or not finite, fx or fy not positive.
 * tb_pnp_ransac: the host form, one problem of n rows on the batched entry (host pointers; Tcw_prior nullable; inlier [n]). */
typedef struct tb_pnp_params {
    int hypotheses;      /* 1..1024; 256 */
    double chi2_max;     /* 5.991, PoseOptimization's chi2Mono */
    uint64_t seed;
} tb_pnp_params;
int tb_pnp_ransac_batch_dev(tb_ctx* ctx, int nproblems, const double K[4], const tb_obs* obs, const int32_t* counts, int obs_pitch,
                            const tb_pnp_params* params, const float* Tcw_prior, float* Tcw_out, int32_t* consensus, uint8_t* inlier,
                            int32_t* winner, int32_t* flags);
int tb_pnp_ransac(tb_ctx* ctx, const double K[4], const tb_obs* obs, int n, const tb_pnp_params* params, const float* Tcw_prior,
                  float Tcw_out[16], int* consensus, uint8_t* inlier, int32_t winner[2], int* flags);
/* A similarity transform from 3D-3D rows: Horn's closed form (Horn 1987, unit quaternions) inside a RANSAC, with a least-squares
 * refit; batched and device-resident. The reference has no such step; ORB-SLAM runs one (Sim3Solver) between the bag-of-words
 * loop candidate and the pose-graph correction, which is what this is for (DESIGN.md 9n has the derivation;
 * tests/sim3_reference.py is the definition, statement for statement, and the kernel matches it bit for bit).
 * Problem p reads counts[p] rows tb_sim3_row (X1 Y1 Z1, X2 Y2 Z2, inv_sigma2_1, inv_sigma2_2: the same physical point in
 * camera-1 and in camera-2 coordinates with the two keys' invLevelSigma2) at rows + p * pitch; a count is clamped to [0, pitch].
 * K = fx, fy, cx, cy (host) serves both cameras. A row's observation in image i is the projection of its own point Xi, as in
 * ORB-SLAM's solver: no pixel goes into the record. The transform sought is X1 = s R12 X2 + t12. float64 with + - * / sqrt fabs
 * and comparisons only, one operation per statement, fixed loop counts.
 *   sampling  tb_pnp_ransac_batch_dev's rule, unchanged: draw k of hypothesis h is mix(seed + (8 h + k + 1) * 0x9E3779B97F4A7C15)
 *             (splitmix64's output function); its high 32 bits times n, shifted right by 32, is a row. Draws are taken until
 *             three distinct rows are found or 8 are used up; a hypothesis that runs out is void. The sample depends on
 *             (seed, h, n) only, never on p: a problem gives the same bits alone and inside any batch
 *   solver    the sums S1, S2 of the m = 3 points of each set (a sum over a sample is ((0 + v0) + v1) + v2) and the centroids
 *             O = S / m; the centred points Pr = X - O; M[i][j] = sum Pr2[i] Pr1[j]; Horn's symmetric 4 x 4
 *             N = (M00+M11+M22, M12-M21, M20-M02, M01-M10; ., M00-M11-M22, M01+M10, M20+M02; ., ., M11-M00-M22, M12+M21;
 *             ., ., ., M22-M00-M11); 5 cyclic Jacobi sweeps in the pair order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) with the
 *             triangulation's rotation (tb_linear_triangle_batch_dev), no convergence test; the eigenvector v_k at the largest
 *             diagonal entry lam_k, the lowest index on a tie, is corrected once to first order from its residual
 *             r = N v_k - lam_k v_k against the N the sweeps started from: v_k + sum_(i != k) (v_i . r) / (lam_k - lam_i) v_i,
 *             a term left out where its denominator is 0. Every product and partial sum of r is carried with its rounding
 *             error (Dekker's product with the splitter 2^27 + 1, Knuth's sum: + - * only) and rounded once at the end, which
 *             is what lets the result agree with LAPACK's to 1e-12 where two eigenvalues lie 1e-5 of the largest apart.
 *             Negated where w < 0, it is the unit quaternion w x y z of R12;
 *             R12 = (1-2(yy+zz), 2(xy-wz), 2(xz+wy); 2(xy+wz), 1-2(xx+zz), 2(yz-wx); 2(xz-wy), 2(yz+wx), 1-2(xx+yy));
 *             P3 = R12 Pr2; s = sum(Pr1 . P3) / sum(P3 . P3), or exactly 1.0 with fixed_scale; t12 = O1 - s (R12 O2). The inverse
 *             is R21 = R12', s21 = 1 / s, t21 = -(R12' t12) / s
 *   void      a sample is void, never a NaN result, when it has a non-finite coordinate, a point whose own Z is not above 0, two
 *             edge vectors a, b in either set with |a x b|^2 <= 1e-6 |a|^2 |b|^2 (coincident or collinear: the sine of the
 *             angle is below 1e-3, where the two largest eigenvalues of N meet and the rotation about the line is free), or
 *             an s that is not finite or not above 0 (or a t12, s21 or t21 that is not finite)
 *   score     every hypothesis against all n rows: Q1 = (s R12) X2 + t12 and Q2 = (s21 R21) X1 + t21; a row is an inlier iff
 *             the four depths Z1, Z2, Q1z, Q2z are above 0 and |proj(Q1) - proj(X1)|^2 * inv_sigma2_1 <= chi2_max and
 *             |proj(Q2) - proj(X2)|^2 * inv_sigma2_2 <= chi2_max (proj(X) = (fx (X / Z) + cx, fy (Y / Z) + cy)). The winner has
 *             the most inliers, ties to the lower hypothesis. Counts are integer sums; there is no floating-point atomic anywhere
 *   refit     the solver's statements once more on all m consensus rows of the winner, centroids first, then the centred sums,
 *             then the scale's two sums (no raw moments). A sum over the rows: row i belongs to thread i mod 256, a thread adds
 *             its rows t, t + 256, ... in ascending order to 0.0, and the 256 partial sums meet in the butterfly
 *             p[t] = p[t] + p[t ^ d], d = 1, 2, 4, ..., 128. The refitted transform is rescored; it replaces the hypothesis iff
 *             it is not void and its consensus is not smaller: then the mask and the count are the refit's and winner[1] = 1.
 *             Fewer than 3 consensus rows, or a void refit, keep the hypothesis and give winner[1] = 0
 *   void problem   n < 3, or no hypothesis with a solution: consensus 0, winner (-2, 0), the identity and scale 1, an all-zero
 *             mask, flags bit 0 set
 * Out (device, each nullable): S12 [nproblems][16] float (the float32 rounding of [s R12 | t12; 0 0 0 1]); srt [nproblems][8]
 * double (the unit quaternion w x y z, t12, s: FP64, the layout of tb_pose_graph_sim3_batch_dev's nodes and edges, which take it
 * without a float32 detour); consensus [nproblems]; inlier [nproblems][pitch] bytes (zero beyond the count); winner [nproblems][2]
 * (hypothesis, refitted); flags [nproblems]. Asynchronous on the context's stream, no host synchronisation, no host <-> device
 * copy, no work buffer: one launch of one 256-thread workgroup per problem whose state is registers and LDS. At most 65535
 * problems per call (TB_EUNSUPPORTED). TB_EINVAL: null rows / counts / K / params, pitch < 1, hypotheses outside 1..1024,
 * fixed_scale not 0 or 1, chi2_max negative or not finite, fx or fy not positive.
 * tb_sim3_ransac: the host form, one problem of n rows on the batched entry (host pointers; inlier [n]; S12 [16]; srt [8]). */
typedef struct tb_sim3_params {
    int hypotheses;      /* 1..1024; 256 */
    int fixed_scale;     /* 0 | 1; a stereo map has a metric scale: 1 */
    double chi2_max;     /* 9.210: chi-square, 2 degrees of freedom, 99 %, ORB-SLAM's Sim3Solver threshold. A default, not a
                            measurement */
    uint64_t seed;
} tb_sim3_params;
int tb_sim3_ransac_batch_dev(tb_ctx* ctx, int nproblems, const double K[4], const tb_sim3_row* rows, const int32_t* counts, int pitch,
                             const tb_sim3_params* params, float* S12, double* srt, int32_t* consensus, uint8_t* inlier, int32_t* winner,
                             int32_t* flags);
int tb_sim3_ransac(tb_ctx* ctx, const double K[4], const tb_sim3_row* rows, int n, const tb_sim3_params* params, float S12[16],
                   double srt[8], int* consensus, uint8_t* inlier, int32_t winner[2], int* flags);
/* The non-linear refinement of a similarity on pixels: ORB-SLAM's Optimizer::OptimizeSim3, which LoopClosing runs on the
 * Sim3Solver's winner before the transform becomes the pose graph's loop edge; batched and device-resident. The reference has no
 * such step. tb_sim3_ransac_batch_dev never sees a pixel and fits in 3D, where every point counts the same although a stereo
 * point's depth error grows with Z^2; this entry minimises the reprojection error in both images instead (DESIGN.md 9p has the
 * derivation and what it buys; tests/sim3_opt_reference.py is the definition, statement for statement).
 * Problem p reads counts[p] rows tb_sim3_obs_row (a tb_sim3_row's X1 Y1 Z1, X2 Y2 Z2, then the pixels u1 v1 and u2 v2 of the two
 * keys that observe the point, then inv_sigma2_1, inv_sigma2_2) at rows + p * pitch; a count below 0 is clamped to 0, one above
 * pitch to pitch. K = fx, fy, cx, cy (host) serves both cameras, proj(X) = (fx X / Z + cx, fy Y / Z + cy). The unknown is one
 * S12 = (s, R12, t12), X1 = s R12 X2 + t12, read from srt_in + 8 p and written to srt_out + 8 p in tb_sim3_ransac_batch_dev's srt
 * layout (FP64: the unit quaternion w x y z, t12, s; srt_out may be srt_in), and to S12 + 16 p as the float32 [s R12 | t12; 0 0 0 1].
 *   cost      with Q1 = s R12 X2 + t12 and Q2 = S12^-1 X1 = R12' (X1 - t12) / s a row has ORB-SLAM's two edges
 *             e12 = (u1, v1) - proj(Q1), chi2 c1 = inv_sigma2_1 |e12|^2, and e21 = (u2, v2) - proj(Q2), c2 = inv_sigma2_2 |e21|^2.
 *             Each goes under g2o's Huber kernel with delta = sqrt(th2): rho(c) = c and rho' = 1 where sqrt(c) <= delta, otherwise
 *             rho(c) = 2 sqrt(c) delta - th2 and rho' = delta / sqrt(c). The robust chi2 is the sum of rho over both edges of
 *             the active rows. A transform that takes an active row's Q1z or Q2z to 0 or below has chi2 = +inf
 *   update    S <- Exp(delta) S, delta = (omega, upsilon, sigma), with tb_pose_graph_sim3_batch_dev's Exp
 *   Jacobians exact: dQ1 / ddelta = [-[Q1]x | I | Q1], dQ2 / ddelta = -(1 / s) R12' [-[X1]x | I | X1], each chained through
 *             -P(Q), P(Q) = (fx / Z, 0, -fx X / Z^2; 0, fy / Z, -fy Y / Z^2). H = sum J' (w rho') J, g = -sum J' (w rho') e.
 *             With fixed_scale = 1 the unknowns are the six (omega, upsilon), sigma = 0, and s keeps its bytes
 *   sums      row i belongs to thread i mod 256; a thread adds its rows t, t + 256, ... in ascending order to 0.0 and the 256
 *             partial sums meet in the butterfly p[t] = p[t] + p[t ^ d], d = 1, 2, 4, ..., 128 (tb_sim3_ransac_batch_dev's rule):
 *             28 + 7 sums for a linearisation, 1 for a trial's chi2. No floating-point atomic anywhere
 *   LM        one round of `iters` iterations is tb_pose_graph_batch_dev's rule, unchanged: lambda0 = 1e-5 max |diag H| at the
 *             round's first iteration (g2o's initialisation); a trial solves (H + lambda I) x = g by an un-pivoted Cholesky (a
 *             failed factorisation is a trial of chi2 DBL_MAX) and is judged on the exact robust chi2 of Exp(x) S:
 *             rho = (chi2 - trial) / (x . (lambda x + g) + 1e-3); accepted on rho > 0 and a finite trial, then
 *             lambda *= max(1/3, min(2/3, 1 - (2 rho - 1)^3)), nu = 2; otherwise lambda *= nu, nu *= 2; at most 10 trials an
 *             iteration; the round stops after 10 rejections, at rho == 0 or after `iters`
 *   procedure (ORB-SLAM's) 0. the seed's quaternion is normalised (w >= 0). The rows that start active are those of active_in
 *             [nproblems][pitch] bytes (NULL: every row; tb_sim3_ransac_batch_dev's mask is the intended input) below the count;
 *             of these a row with a non-finite field, with Z1 or Z2 not above 0, or with Q1z or Q2z not above 0 under the seed
 *             is dropped (stats[5] counts them). 1. Fewer than min_keep rows active: the problem stops as in 3. Otherwise
 *             iters_first LM iterations on the active rows, both edges of each. 2. A row is bad where either of its two edges'
 *             plain chi2 exceeds th2 under the result; bad rows leave, both edges together; nBad is their count. 3. If fewer
 *             than min_keep rows stay the problem stops: inliers 0, an all-zero mask, srt_out is srt_in byte for byte, S12 the
 *             seed's, stats[7] = 1. 4. Otherwise a second round, lambda starting anew as in a second g2o optimize(): iters_bad
 *             iterations if nBad > 0, else iters_clean. 5. The mask marks the rows still active whose two chi2 are both at most
 *             th2 under the final transform; inliers is their count. A problem that accepted no trial returns srt_in byte for byte
 *   malformed a seed with a non-finite entry, a zero quaternion (or one whose norm is not finite) or s not above 0:
 *             stats[7] = -1, srt_out is srt_in byte for byte, S12 the identity, inliers 0, an all-zero mask, the other stats 0
 * Out (device): srt_out [nproblems][8] double, S12 [nproblems][16] float, inliers [nproblems] and stats [nproblems][8] double are
 * nullable; inlier_mask [nproblems][pitch] bytes is not: a thread keeps its rows' active flags there during the call (it may be
 * the buffer active_in points to, which is then overwritten). stats = iterations run, initial robust chi2 (the starting rows
 * under the seed), final robust chi2 (the rows left, under the final transform), trials, nBad, dropped rows, final lambda, flag
 * (0, 1 = stopped below min_keep, -1 = malformed). Asynchronous on the context's stream, no host synchronisation, no host <->
 * device copy, no work buffer: one launch (k_sim3_opt) of one 256-thread workgroup per problem; a problem gives the same bits
 * alone, at any batch position and from run to run. At most 65535 problems per call (TB_EUNSUPPORTED). TB_EINVAL: null rows /
 * counts / K / params / srt_in / inlier_mask, pitch < 1, K not finite, fx or fy not positive, fixed_scale not 0 or 1, th2 negative
 * or not finite, an iteration count outside 0..99, min_keep < 0.
 * tb_sim3_optimize: the host form, one problem of n rows on the batched entry (host pointers; active nullable [n]; srt_in and
 * srt_out [8]; S12 [16]; inlier_mask [n] and stats [8] nullable). */
typedef struct tb_sim3_opt_params {
    double th2;          /* 10.0: ORB-SLAM's (LoopClosing passes 10). A default, not a measurement */
    int iters_first;     /* 0..99; 5 */
    int iters_bad;       /* 0..99; 10: the second round when the first left bad rows */
    int iters_clean;     /* 0..99; 5: the second round otherwise */
    int min_keep;        /* >= 0; 10 */
    int fixed_scale;     /* 0 | 1; a stereo map has a metric scale: 1 */
} tb_sim3_opt_params;
int tb_sim3_optimize_batch_dev(tb_ctx* ctx, int nproblems, const double K[4], const tb_sim3_obs_row* rows, const int32_t* counts, int pitch,
                               const uint8_t* active_in, const double* srt_in, const tb_sim3_opt_params* params, double* srt_out,
                               float* S12, int32_t* inliers, uint8_t* inlier_mask, double* stats);
int tb_sim3_optimize(tb_ctx* ctx, const double K[4], const tb_sim3_obs_row* rows, int n, const uint8_t* active, const double srt_in[8],
                     const tb_sim3_opt_params* params, double srt_out[8], float S12[16], int* inliers, uint8_t* inlier_mask,
                     double stats[8]);
/* Guided mutual matching under a similarity: ORB-SLAM's ORBmatcher::SearchBySim3, which LoopClosing runs between the Sim3Solver and
 * OptimizeSim3 so that the refinement also sees the correspondences the bag-of-words matcher let drop; batched and device-resident.
 * The reference has no such step; tests/sim3_search_reference.py is the definition, statement for statement, and the kernels give
 * the same integers.
 * Pair p has two sides. Side k reads countsk[p] keys (clamped to [0, pitchk]) at keysk + p * pitchk, their descriptors at descK +
 * 32 p pitchk, the keys' points IN THE SIDE'S OWN CAMERA FRAME at pointsk + 3 p pitchk (float32), a validity byte a key (validk: the
 * key has a point) and an `already matched` byte a key (matchedk). srt + 8 p is the similarity in tb_sim3_ransac_batch_dev's layout
 * (FP64: the quaternion w x y z, taken as it is given, then t, then s): X1 = s R X2 + t. Shared by the batch: K = fx, fy, cx, cy
 * (host), the image width x height, and the level table g[l], l < nlevels: the size of a level-l pixel in level-0 pixels, which is
 * tb_scale_factors(nlevels, scale)'s inv_sf (float32; 1.25^l at this project's scale = 0.8) -- ORB-SLAM's mvScaleFactors. (sf, the
 * shrink factor 0.8^l, cannot serve: under it 0.8 minD <= d <= 1.2 maxD below has no solution once sf[nlevels - 1] < 2 / 3.)
 *   1 -> 2    for every key i of side 1 below the count with valid1[i] != 0 and matched1[i] == 0 (a point that is TRIED):
 *             P = R' (X1c[i] - t) / s; skipped unless P.z > 0; u = fx (P.x / P.z) + cx, v likewise; skipped unless 0 <= u < width
 *             and 0 <= v < height; maxD = |X1c[i]| g[octave_i], minD = maxD / g[nlevels - 1]; d = s |P| (the length in side 1's
 *             units); skipped unless 0.8 minD <= d <= 1.2 maxD; the predicted level L is the smallest l with g[l] d >= maxD, or
 *             nlevels - 1 if there is none (ORB-SLAM's ceil(log(maxD / d) / log(1.2)) clamped, written with comparisons against the
 *             table); r = th g[L]. The point has then REACHED THE SEARCH: its candidates are all keys j of side 2 below the count
 *             with |x_j - u| < r, |y_j - v| < r and octave L - 1 or L (a candidate need not have a point and may be matched
 *             already: ORB-SLAM); the best has the smallest Hamming distance between the two KEYS' descriptors, a tie goes to the
 *             lowest j (the minimum of distance << 32 | j: the visiting order decides nothing). match1[i] = j if that distance is
 *             <= th_high, else -1
 *   2 -> 1    the same with P = s (R X2c[j]) + t, d = |P| / s and the sides exchanged: match2[j]
 *   agreement (i, j) is a new pair where match1[i] = j and match2[j] = i; new pairs are listed in ascending i
 *   numbers   float64 from the float32 inputs, one rounding a statement, no contraction, only + - * / sqrt; a dot product adds its
 *             terms left to right; |x| = sqrt((x0 x0 + x1 x1) + x2 x2). No atomic on any path that decides an output
 * Two stated deviations from ORB-SLAM: the key's own descriptor stands for the map point's (a store holds no representative
 * descriptor), and the range test and the level prediction compare lengths in one map's units (s |P|, |P| / s) where ORB-SLAM
 * compares them raw; the two coincide at s = 1.
 * Out (device, each nullable): match1 [npairs][pitch1] and match2 [npairs][pitch2] int32 (-1 beyond the count too); pairs
 * [npairs][cap] tb_match (queryIdx = i, trainIdx = j, imgIdx = -1, distance = the Hamming distance) with pair_counts [npairs]: the
 * list is truncated at cap, the count is not; stats [npairs][8] int32 = points tried 1 -> 2, points that reached the search 1 -> 2,
 * the same two for 2 -> 1, accepted 1 -> 2, accepted 2 -> 1, new pairs, flag. A malformed problem -- a key below a count whose
 * octave lies outside 0 .. nlevels - 1, or an s that is not finite or not above 0 -- is flagged: flag 1, every match -1, counts
 * and the other stats 0. Asynchronous on the context's stream, no host synchronisation, no host <-> device copy; two launches
 * (k_sim3_search: chunks of 256 source keys x 2 directions x pairs; k_sim3_search_agree: one workgroup a pair); a problem gives the
 * same bits alone, in any batch, in any slot and from run to run. At most 65535 pairs per call (TB_EUNSUPPORTED). TB_EINVAL: null
 * inputs, a pitch outside 1..8192, nlevels outside 1..16, th not positive, th_high outside 0..256, width or height not positive,
 * scale not positive, K not finite, fx or fy not positive, cap < 0 (cap < 1 with pairs). ORB-SLAM: th = 7.5, th_high = 100. */
int tb_search_by_sim3_batch_dev(tb_ctx* ctx, int npairs, const double K[4], int width, int height, int nlevels, float scale,
                                const tb_keypoint* keys1, const uint8_t* desc1, const float* points1, const uint8_t* valid1,
                                const uint8_t* matched1, const int32_t* counts1, int pitch1, const tb_keypoint* keys2, const uint8_t* desc2,
                                const float* points2, const uint8_t* valid2, const uint8_t* matched2, const int32_t* counts2, int pitch2,
                                const double* srt, float th, int th_high, int32_t* match1, int32_t* match2, tb_match* pairs, int cap,
                                int32_t* pair_counts, int32_t* stats);
/* A relative pose and first points from 2D-2D rows alone: 8-point hypotheses in a RANSAC, a least-squares refit, the four
 * decompositions of E told apart by triangulation; batched and device-resident. The reference has no such step (its
 * LinearTriangle is handed poses); this is ORB-SLAM's Initializer on its fundamental-matrix branch (DESIGN.md 9m has the
 * derivation and the deviations; tests/two_view_reference.py is the definition, statement for statement, and the kernel
 * matches it bit for bit). Inputs as tb_linear_triangle_batch_dev's: problem p reads xy0 / xy1 [nproblems][pitch][2] float
 * pixels of view 0 / view 1, counts [nproblems] (nullable = pitch each; clamped to [0, pitch]), skip [nproblems][pitch] bytes
 * (nullable), inv_sigma2_0 / _1 [nproblems][pitch] (nullable = 1), K = fx, fy, cx, cy (host), Tcw0 [nproblems][16] (nullable =
 * the identity). float64 with + - * / sqrt and comparisons only, fixed loop counts.
 *   rows       the candidates are the rows below the count whose skip byte is 0, in index order, n of them; n < 8 is void
 *   sampling   counter based: draw k of hypothesis h is mix(seed + (16 h + k + 1) * 0x9E3779B97F4A7C15) (splitmix64's output
 *              function); its high 32 bits times n, shifted right by 32, is a candidate. Draws are taken until eight distinct
 *              candidates are found or 16 are used up; a hypothesis that runs out is void. The sample depends on (seed, h, n)
 *              only, never on p: a problem gives the same bits alone and inside any batch
 *   solver     x = (u - cx) / fx, y = (v - cy) / fy; the 8 x 9 epipolar system in tb_find_fundamental_ransac's row layout
 *              (x1' E x0 = 0, E row-major), Gauss-Jordan with partial pivoting (the unused row with the largest entry, the
 *              lowest row on a tie) and the relative pivot test 1e-12 * scale. Exactly one free column gives the null vector,
 *              which is E; any other count, or a non-finite entry, makes the hypothesis void, never a NaN
 *   score      F = K^-T E K^-1; a row is in the consensus iff both squared point-to-epipolar-line distances in pixels, each times
 *              its view's inv_sigma2, are <= chi2_epi (a NaN is not). The winner has the most rows, ties to the lower
 *              hypothesis. Counts are integer sums; there is no floating-point atomic anywhere
 *   refit      (refit != 0) the 9 x 9 normal matrix of the consensus rows, summed in a fixed order (candidate c in slot c mod 256,
 *              a slot in index order, the slots by the butterfly t ^ 1, 2, ..., 128); 5 cyclic Jacobi sweeps in the pair order
 *              (0,1) (0,2) ... (7,8) with the triangulation's rotation; the eigenvector at the smallest diagonal entry is the new
 *              E, and the consensus is counted once more against it. No Hartley normalisation (it changed nothing measurable)
 *   decompose  6 Jacobi sweeps on E' E give V and the squared singular values; u_i = E v_i / s_i for the two largest,
 *              u3 = u1 x u2, v3 = v1 x v2 (both determinants +1). Candidates 0..3: (U W V', +u3), (U W V', -u3), (U W' V', +u3),
 *              (U W' V', -u3)
 *   cheirality every candidate triangulates every consensus row with tb_linear_triangle_batch_dev's statements and the gates
 *              of `tri`, view 0 at the identity, view 1 at [R | t], |t| = 1, in float64. good[c] counts the flags 1 and 4, tri[c]
 *              the flags 1
 *   decision   c* = the largest good, ties to the lower candidate. status: 0 ok; 1 void (n < 8, or no hypothesis with a solution);
 *              2 good[c*] < min_points or (double) good[c*] < min_good_ratio * (double) consensus; 3 another candidate has
 *              (double) good[c] > ambiguity_ratio * (double) good[c*]; 4 tri[c*] < min_points. The first failing test decides.
 *              min_good_ratio 0.9, ambiguity_ratio 0.7 and min_points 50 are ORB-SLAM's ReconstructF figures
 * Out (device, each nullable): Tcw1 [nproblems][16] float = [R | baseline t] composed onto Tcw0 (the float32 rounding of the
 * float64 product; status != 0: Tcw0 as given, or the identity); points [nproblems][pitch][3] float, world frame, WRITTEN ONLY
 * WHERE point_flags IS 1 AND status IS 0 (the float32 point of view 0's frame times baseline, taken through Tcw0^-1; a failed
 * problem leaves points untouched); point_flags [nproblems][pitch] bytes (the triangulation's codes under c*, 0 for a row that is
 * not in the consensus); inlier [nproblems][pitch] bytes (the consensus mask); consensus [nproblems]; winner [nproblems][2]
 * (hypothesis, candidate; (-1, -1) when void); good / tri [nproblems][4]; status [nproblems]. A void problem reports zeros.
 * Asynchronous on the context's stream, no host synchronisation, no host <-> device copy, no work buffer: one launch of one
 * 256-thread workgroup per problem whose state is registers and LDS, the candidate rows staged once in dynamic LDS (29 bytes per row
 * of the pitch). TB_EUNSUPPORTED: more than
 * 65535 problems, pitch above TB_TWO_VIEW_MAX_PITCH. TB_EINVAL: null xy0 / xy1 / K / params, pitch < 1, hypotheses outside
 * 1..1024, chi2_epi or tri.chi2_max negative or not finite, tri.cos_parallax_max not finite, min_good_ratio or ambiguity_ratio
 * outside (0, 1], min_points < 0, baseline not positive and finite, fx or fy not positive, K not finite.
 * tb_two_view: the host form, one problem of n rows on the batched entry (host pointers; points is zero where nothing was
 * written; good / tri [4], winner [2]). */
#define TB_TWO_VIEW_MAX_PITCH 4096
typedef struct tb_two_view_params {
    int hypotheses;             /* 1..1024; 256 */
    double chi2_epi;            /* 3.841 */
    int refit;                  /* 1 */
    tb_triangulate_params tri;  /* 0.9998, 5.991 */
    double min_good_ratio;      /* 0.9 */
    double ambiguity_ratio;     /* 0.7 */
    int min_points;             /* 50 */
    double baseline;            /* 1.0: the length given to the translation */
    uint64_t seed;
} tb_two_view_params;
int tb_two_view_batch_dev(tb_ctx* ctx, int nproblems, const float* xy0, const float* xy1, const int32_t* counts, int pitch,
                          const uint8_t* skip, const float* inv_sigma2_0, const float* inv_sigma2_1, const double K[4],
                          const float* Tcw0, const tb_two_view_params* params, float* Tcw1, float* points, uint8_t* point_flags,
                          uint8_t* inlier, int32_t* consensus, int32_t* winner, int32_t* good, int32_t* tri, int32_t* status);
int tb_two_view(tb_ctx* ctx, const float* xy0, const float* xy1, int n, const uint8_t* skip, const float* inv_sigma2_0,
                const float* inv_sigma2_1, const double K[4], const float Tcw0[16], const tb_two_view_params* params, float Tcw1[16],
                float* points, uint8_t* point_flags, uint8_t* inlier, int* consensus, int32_t winner[2], int32_t good[4],
                int32_t tri[4], int* status);
/* SURVEY 8(f) row 2, first part -- the optical-flow matcher.
 * tb_optical_flow_pyr_lk replaces the call cv::calcOpticalFlowPyrLK(prev, next, prev_pts, next_pts, status, err,
 * Size(win, win), max_level) of matcher.cpp:744 (default criteria: 30 iterations / eps 0.01, flags 0,
 * minEigThreshold 1e-4). win must be 21 (the reference's), max_level 0..5. Host pointers; prev_pts / next_pts are
 * n (x, y) pairs; err nullable; *top_level (nullable) = coarsest pyramid level used. OpenCV is not part of the
 * reference tree: the routine is restated, parity UNPINNED (oracle/oracle_flow.cpp says what was restated and the one
 * deliberate difference, exact integer window sums).
 * tb_search_by_opflow replaces Matcher::searchByOPFlow(F1, F2, cur_points, equalized, reject), matcher.cpp:724-768:
 * tracks F2's keys (keys2_xy) from img2 into img1, clears the points that leave F1's frame (cam1->width / height,
 * CameraModel.h:33-39) and returns DMatch(i, i) records (distance FLT_MAX, imgIdx -1, as a default-constructed
 * cv::DMatch). equalized != 0: img1 is equalised first, as tb_clahe(3.0, 8 x 8) does (F1->Equalize(), matcher.cpp:736-739).
 * reject != 0: Matcher::rejectWithF (matcher.cpp:853-881) = cv::findFundamentalMat(FM_RANSAC, 1.0, 0.99) clears the
 * flags of the epipolar outliers before the matches are listed (as tb_reject_with_f below). cur_points: n (x, y) pairs out.
 * Runs tb_search_by_opflow_batch_dev on one pair, so TB_ECAPACITY reports the full match count in *count, as the other
 * matcher host forms do. */
/* Frame::Equalize, Frame.cpp:453-458: cv::createCLAHE(clip_limit = 3.0, Size(tiles_x, tiles_y) = 8 x 8)->apply(src, dst)
 * (OpenCV 3.3 routine restated, parity unpinned). Host pointers; dst has the size of src. tb_clahe_dev: device pointers,
 * asynchronous on the context's stream. */
int tb_clahe(tb_ctx* ctx, const uint8_t* src, int width, int height, int stride, double clip_limit, int tiles_x, int tiles_y,
             uint8_t* dst, int dst_stride);
int tb_clahe_dev(tb_ctx* ctx, const uint8_t* src, int width, int height, int stride, double clip_limit, int tiles_x, int tiles_y,
                 uint8_t* dst, int dst_stride);
int tb_optical_flow_pyr_lk(tb_ctx* ctx, const uint8_t* prev, const uint8_t* next, int width, int height, int stride,
                           const float* prev_pts, int n, int win, int max_level, float* next_pts, uint8_t* status,
                           float* err, int* top_level);
int tb_search_by_opflow(tb_ctx* ctx, const uint8_t* img1, const uint8_t* img2, int width, int height, int stride,
                        const tb_camera* cam1, const float* keys2_xy, int n, int equalized, int reject,
                        float* cur_points, tb_match* out, int cap, int* count);
/* Batched device-resident searchByOPFlow: npairs (F1, F2) image pairs of one geometry (pair p at img1 / img2 +
 * p * image_pitch bytes), F2's keys of pair p at keys2_xy + p * pts_pitch (x, y) records (counts[p] of them; counts
 * nullable = pts_pitch each). Outputs per pair: cur_points and status (1 = matched, after the IsInFrame filter) at slot
 * p * pts_pitch, DMatch(i, i) records in index order at out + p * cap, their number in out_counts[p] (clamped to cap).
 * cam1 is a HOST pointer (only width / height are read). Asynchronous on the context's stream. */
int tb_search_by_opflow_batch_dev(tb_ctx* ctx, int npairs, const uint8_t* img1, const uint8_t* img2, int width, int height,
                                  int stride, size_t image_pitch, const tb_camera* cam1, const float* keys2_xy,
                                  const int32_t* counts, int pts_pitch, int equalized, int reject, float* cur_points,
                                  uint8_t* status, tb_match* out, int cap, int32_t* out_counts);
/* Device-resident form of the tracker: images, points and outputs in HBM, asynchronous on the context's stream. */
int tb_optical_flow_pyr_lk_dev(tb_ctx* ctx, const uint8_t* prev, const uint8_t* next, int width, int height, int stride,
                               const float* prev_pts, int n, int win, int max_level, float* next_pts, uint8_t* status,
                               float* err);
/* Batched device form: npairs image pairs of one geometry in one launch per stage (pair p at prev / next +
 * p * image_pitch bytes; its points, results, status and err at slot p * pts_pitch, counts[p] <= pts_pitch of them,
 * counts nullable = pts_pitch each). */
int tb_optical_flow_pyr_lk_batch_dev(tb_ctx* ctx, int npairs, const uint8_t* prev, const uint8_t* next, int width, int height,
                                     int stride, size_t image_pitch, const float* prev_pts, const int32_t* counts,
                                     int pts_pitch, int win, int max_level, float* next_pts, uint8_t* status, float* err);

/* SURVEY 8(f) row 2, second part / row a16 -- the RANSAC stage and the stereo depths.
 * tb_find_fundamental_ransac replaces cv::findFundamentalMat(pts1, pts2, cv::FM_RANSAC, thresh, conf, mask) as
 * Matcher::rejectWithF calls it (matcher.cpp:872): *ok = 1 and mask (n bytes) / F (9 doubles row-major, nullable) / *iters
 * (nullable: RANSAC iterations run) when a mask comes back, *ok = 0 when OpenCV returns none (fewer than 7 points, no model).
 * As in OpenCV, 8..14 points go to the LMedS registrator (fixed iteration count, smallest median error, inliers within
 * sigma; *iters = its iteration count), 15 and more to RANSAC -- host and batched entry points alike. OpenCV 3.3 routines restated, PARITY UNPINNED: the sampling
 * (cv::RNG((uint64)-1), getSubset, collinearity retries), error measure, model update and iteration budget follow OpenCV's
 * structure; the 7-point solver's null space and cubic roots are computed with + - * / sqrt only (oracle/oracle_fund.cpp).
 * tb_reject_with_f replaces Matcher::rejectWithF(cur_pts, last_pts, status) (matcher.cpp:853-881): n (x, y) pairs each,
 * status in/out. At most 8 keys, fewer than 7 tracked points or no model: the reference reads an empty vector (UB); here
 * the flags are left as they are. Host pointers. */
int tb_find_fundamental_ransac(tb_ctx* ctx, const float* pts1, const float* pts2, int n, double thresh, double conf, uint8_t* mask,
                               double* F, int* iters, int* ok);
int tb_reject_with_f(tb_ctx* ctx, const float* cur_pts, const float* last_pts, int n, uint8_t* status);
/* Batched, device-resident Matcher::rejectWithF: pair p has counts[p] keys (all pts_pitch of them when counts is null);
 * cur_pts / last_pts [npairs][pts_pitch][2] floats, status [npairs][pts_pitch] in/out. One workgroup per pair; every pair
 * takes the branch the host form takes for its number of tracked points (none / seven-point / LMedS / RANSAC).
 * Asynchronous on the context's stream. */
int tb_reject_with_f_batch_dev(tb_ctx* ctx, int npairs, const float* cur_pts, const float* last_pts, const int32_t* counts,
                               int pts_pitch, uint8_t* status);
/* LocalBA::AddMapPointsByStereo(current_frame, stereo_frame, bf, fx), LocalBA.cpp:46-68: searchByOPFlow(stereo, current,
 * pts, equalized = true, reject = true), then depth[i] = bf / fabsf(pts[i].x - key[i].x) for the surviving keys i of the
 * current frame and -1 for the others (fx is unused by the reference; its drawing and imshow are dropped). img_stereo /
 * img_current: level-0 images; cam_stereo: the stereo frame's camera (width / height for IsInFrame); keys_xy: the current
 * frame's keys. *n_depth = number of depths set. Host pointers; runs tb_add_map_points_by_stereo_batch_dev on one pair. */
int tb_add_map_points_by_stereo(tb_ctx* ctx, const uint8_t* img_stereo, const uint8_t* img_current, int width, int height, int stride,
                                const tb_camera* cam_stereo, const float* keys_xy, int n, float bf, float* depth, int* n_depth);
/* Batched device form: pair p's images at + p * image_pitch, its keys / tracked points / status / depths at slot
 * p * pts_pitch (counts[p] valid, counts nullable = pts_pitch each). cam_stereo is a HOST pointer. Asynchronous. */
int tb_add_map_points_by_stereo_batch_dev(tb_ctx* ctx, int npairs, const uint8_t* img_stereo, const uint8_t* img_current, int width,
                                          int height, int stride, size_t image_pitch, const tb_camera* cam_stereo, const float* keys_xy,
                                          const int32_t* counts, int pts_pitch, float bf, float* cur_points, uint8_t* status,
                                          float* depth);

/* Multi-keyframe local BA -- north-star extension, NO reference counterpart.
 * poses: nkf x 16 (in/out, first nfixed held), pts: npt x 3 (in/out). A point is observed at most once per
 * keyframe (repeated (kf, pt) pairs are rejected like out-of-range indices); at most 64 free keyframes (128 in all),
 * 2^25 points and 99 iterations per window (TB_EUNSUPPORTED beyond). Windows with up to 10 free keyframes run the
 * MFMA-tiled Schur path; 11..64 (reduced systems up to 384 x 384) the generic large-window kernels. stats (nullable, 8 doubles):
 * iterations, initial chi2, final chi2, final lambda. tb_local_ba takes its observations in any order: it sorts a copy by
 * (point, keyframe), so no bit of the result depends on the order; the batched form wants them grouped by ascending point. */
int tb_local_ba(tb_ctx* ctx, const double K[4], int nkf, int nfixed, float* poses, int npt, float* pts,
                const tb_ba_obs* obs, int nobs, int iters, double* stats);
/* Batched device form: nwindows equally sized windows; window w uses poses + w*nkf*16, pts + w*npt*3,
 * obs + w*obs_pitch (obs_counts[w] rows, GROUPED BY ASCENDING POINT INDEX), stats + 8w (nullable;
 * stats[7] = -1 flags a window whose observations were out of range / not grouped / repeated). Device pointers.
 * Synchronises the stream once (LM termination is data dependent). */
int tb_local_ba_batch_dev(tb_ctx* ctx, int nwindows, const double K[4], int nkf, int nfixed, float* poses, int npt,
                          float* pts, const tb_ba_obs* obs, const int32_t* obs_counts, int obs_pitch, int iters,
                          double* stats);
/* Host-only: the layout of the observation stream the local BA's point passes read in windows of up to 8192 points, 10 free and
 * 64 keyframes. pt_start: npt + 1 ints, the first observation of every point (CSR, observations grouped by point); pos
 * [pt_start[npt]]: pos[pt_start[p] + j] = stream entry of point p's j-th observation. The 64 points [64 B, 64 B + 63] own the
 * entries pt_start[64 B] .. pt_start[64 B + 64]; there all points' observation 0 come first, then all observation 1, ..., each
 * run in point order and holding only the points that have that many. */
int tb_ba_obs_stream_positions(const int32_t* pt_start, int npt, int32_t* pos);

/* SE(3) pose-graph optimisation -- extension, NO reference counterpart: the solver between PoseOptimization (one pose) and the
 * local BA (poses and points), restated in numpy in tests/pose_graph_reference.py.
 * A graph has nnodes poses Tcw (nnodes x 16 row-major, in/out, the first nfixed held) and edges (tb_pg_edge: a, b, Z ~ T_b T_a^-1,
 * w_rot, w_trans). With E = Z^-1 T_b T_a^-1 the residual is r = Log(E) ordered (omega, upsilon) like every solver's update vector
 * here (T <- exp(delta) T, SE3Quat::exp), chi2 = sum r' diag(w_rot I3, w_trans I3) r, no robust kernel; the Jacobians are the
 * exact ones, J_b = Jl^-1(r) Ad(Z^-1), J_a = -Jl^-1(r) Ad(E). Everything is FP64; poses enter through the quaternion extraction of
 * PoseOptimization and the local BA. Levenberg-Marquardt by g2o's rule as the local BA restates it: lambda0 = 1e-5 max diag H; a
 * trial is accepted when rho > 0 and its chi2 is finite, then lambda *= max(1/3, min(2/3, 1 - (2 rho - 1)^3)); otherwise lambda *= nu,
 * nu *= 2; at most 10 trials per iteration; stop at 10 rejections, at rho == 0, or after `iters` iterations.
 * Limits: 1 <= nfixed < nnodes (TB_EINVAL otherwise), nnodes <= 64, at most 256 edges and 99 iterations (TB_EUNSUPPORTED beyond).
 * Any connected edge set works: repeated pairs, edges listed as (b, a), several edges into one node. stats (nullable, 8
 * doubles): iterations, initial chi2, final chi2, final lambda, trials (rejected ones included).
 * A graph keeps EVERY BYTE of its poses when it has no edge, when no trial was accepted (iters == 0 among them; chi2 is still
 * reported) or when it is malformed -- an index outside [0, nnodes), a == b, a count above the pitch, a non-finite Z or weight, a
 * zero quaternion, a negative weight; fixed nodes always keep theirs. tb_pose_graph returns TB_EINVAL for a malformed graph. */
int tb_pose_graph(tb_ctx* ctx, int nnodes, int nfixed, float* poses, const tb_pg_edge* edges, int nedges, int iters, double* stats);
/* Batched device form: ngraphs graphs of one shape; graph g uses poses + g*nnodes*16, edges + g*edge_pitch (edge_counts[g] of
 * them, edge_pitch <= 256), stats + 8g (nullable; stats[7] = -1 flags a malformed graph). Device pointers. One workgroup per
 * graph runs the whole LM loop on the device: the call is asynchronous on the context's stream and makes no host synchronisation
 * and no host <-> device copy (the work buffers are the context's and only grow; a call that grows them waits for the stream
 * first). No floating-point atomics: a graph gives the same bits alone, inside any batch, and from run to run. */
int tb_pose_graph_batch_dev(tb_ctx* ctx, int ngraphs, int nnodes, int nfixed, float* poses, const tb_pg_edge* edges,
                            const int32_t* edge_counts, int edge_pitch, int iters, double* stats);
/* Grows the context's work buffer to what tb_pose_graph_batch_dev needs for this shape, once and ahead of time: a later call of
 * that shape or a smaller one then neither allocates nor waits for the stream. Same argument checks. */
int tb_pose_graph_plan(tb_ctx* ctx, int ngraphs, int nnodes, int nfixed, int edge_pitch);

/* Sim(3) pose-graph optimisation -- extension, NO reference counterpart: the pose graph that can change scale, the consumer of the
 * similarity tb_sim3_ransac_batch_dev measures; restated in numpy in tests/pose_graph_sim3_reference.py.
 * A node is S = (s, R, t), X' = s R X + t, stored as 8 doubles in that solver's srt layout (the quaternion w x y z, t, s): nodes is
 * nnodes x 8, in/out, the first nfixed held, so a device best_srt / cand_srt can be a node or an edge as it is. Edges are
 * tb_pg_sim3_edge (a, b, Z ~ S_b S_a^-1, w_rot, w_trans, w_scale). With E = Z^-1 S_b S_a^-1 the residual is r = Log(E) ordered (omega,
 * upsilon, sigma), chi2 = sum r' diag(w_rot I3, w_trans I3, w_scale) r, the update S <- Exp(delta) S, no robust kernel. Jacobians
 * J_b = Jl^-1(r) Ad(Z^-1), J_a = -Jl^-1(r) Ad(E), Jl^-1 = sum_n B_n / n! ad(r)^n to the fixed order 22 (within 1e-9 of the exact ones for
 * |omega| <= 2, |upsilon| <= 5, |sigma| <= 1; beyond that LM stays safe, a trial being accepted on the exact chi2). Everything is FP64;
 * quaternions are normalised on entry (w >= 0). The LM rule, the limits, stats and the TB_EINVAL / TB_EUNSUPPORTED cases are
 * tb_pose_graph's. fixed_scale (0 | 1, ORB-SLAM's bFixScale; anything else TB_EINVAL): a free node has the 6 unknowns (omega,
 * upsilon) and its s keeps its bytes; the residual's seventh component still counts.
 * A graph keeps EVERY BYTE of its nodes when it has no edge, when no trial was accepted or when it is malformed -- tb_pose_graph's
 * list, and a node or edge with a non-finite entry, a zero quaternion or a scale that is not above 0, and a negative or
 * non-finite w_scale; fixed nodes always keep theirs. tb_pose_graph_sim3 returns TB_EINVAL for a malformed graph. */
int tb_pose_graph_sim3(tb_ctx* ctx, int nnodes, int nfixed, int fixed_scale, double* nodes, const tb_pg_sim3_edge* edges, int nedges,
                       int iters, double* stats);
/* Batched device form, as tb_pose_graph_batch_dev: graph g uses nodes + g*nnodes*8, edges + g*edge_pitch (edge_counts[g] of them),
 * stats + 8g (nullable; stats[7] = -1 flags a malformed graph). One launch (k_pgo_sim3), one 256-thread workgroup per graph, the
 * whole LM loop on the device: asynchronous on the context's stream, no host synchronisation, no host <-> device copy, no
 * floating-point atomics -- a graph gives the same bits alone, inside any batch, and from run to run. */
int tb_pose_graph_sim3_batch_dev(tb_ctx* ctx, int ngraphs, int nnodes, int nfixed, int fixed_scale, double* nodes,
                                 const tb_pg_sim3_edge* edges, const int32_t* edge_counts, int edge_pitch, int iters, double* stats);
/* Grows the context's work buffer to what tb_pose_graph_sim3_batch_dev needs for this shape (about 1.8 MB a graph at 64 nodes and
 * 256 edges; the same for either fixed_scale), once and ahead of time. Same argument checks. */
int tb_pose_graph_sim3_plan(tb_ctx* ctx, int ngraphs, int nnodes, int nfixed, int edge_pitch);

/* ---------------------------------------------------------------- device-resident stereo VO loop
 * The tracking loop of the reference's main program, test/test_vo.cpp test_kitti (:674-850), for nseq independent stereo
 * sequences in lock-step: one tb_vo_step_dev = frame t of every sequence, chained on the context's stream from the batched
 * operators above. Frame t of a sequence:
 *   pose      t = 0: the pose given to tb_vo_reset_dev (:694-697); t > 0: the last frame's Tcw (:688)
 *   tracking  t > 0: searchByOPFlow(cur, last, pts, equalized = 1, reject = 1) (:716): LK from the last frame's raw left image
 *             into the current one's CLAHE image; the new key list = all n tracked points, lost ones included (:717-724); key i
 *             carries the last frame's map point i when its status is set (:731-737); PoseOptimization (:761) on one row per
 *             key with a map point (px = tracked point, invSigma2 = 1, Xw = map point), outlier flags cleared; fewer than 3 rows
 *             leave the pose as it is and n_inliers = 0 (LocalBA.cpp:401)
 *   keyframe  t % keyframe_every == 0, after the pose optimisation (:772-832): ORB operator()(5-level pyramid, target, init_th,
 *             min_th) on the left image; SetKeys(orb keys), whose mvpMapPoints.resize(m, nullptr) (Frame.cpp:114) KEEPS the
 *             map points of entries [0, min(n, m)) and nulls [n, m); AddMapPointsByStereo(cur, right, bf, fx) (:800); every key
 *             j with depth > 0 gets a new map point R * norm * depth + t (R, t of Twc at the optimised pose; norm from
 *             u = (int)x, v = (int)y in double). Deviation: a depth that is not finite (zero disparity) creates no point.
 * Dropped: the viewer, imshow and the printing; SetBow (:705) runs only in a TB_VO_BOW loop, the one that reads its output. Local BA is not part of the loop unless
 * enabled (tb_vo_window_ba_enable below; the reference's map_ptr->AddKeyFrame is commented out, :839).
 * State lives in the object (ping-pong key / map-point buffers, a copy of the last left image); after the first step a step
 * makes no host synchronisation and no host <-> device copy. Key capacity = the extractor's kp_capacity. The object uses its
 * context's stream and must be destroyed before its context. */
typedef struct tb_vo tb_vo;
typedef struct tb_vo_params {
    int width, height;
    int nlevels;            /* ORB pyramid levels (reference: 5) */
    float scale;            /* pyramid scale step (0.8) */
    int target;             /* ORB keys per keyframe (2000) */
    float init_th, min_th;  /* FAST thresholds (80, 30) */
    double K[4];            /* fx, fy, cx, cy */
    float bf;               /* AddMapPointsByStereo's bf = baseline * fx (0.573 * 718.856) */
    int keyframe_every;     /* keyframe period (10) */
} tb_vo_params;
int tb_vo_create(tb_ctx* ctx, const tb_vo_params* params, int nseq, tb_vo** out);
void tb_vo_destroy(tb_vo* vo);
/* Tcw0: device, [nseq][16] row-major; the next step is frame 0. Asynchronous. */
int tb_vo_reset_dev(tb_vo* vo, const float* Tcw0);
/* left / right: nseq device images each, row stride `stride` bytes, `pitch` bytes apart (read during the call's kernels; they
 * may be reused once the stream has passed them). right may be NULL on a step that is not a keyframe (TB_EINVAL on one that
 * is; a mono loop, tb_vo_mono_enable below, reads it at frame 0 only). TB_ESTATE before the first reset. Asynchronous on the context's stream. */
int tb_vo_step_dev(tb_vo* vo, const uint8_t* left, const uint8_t* right, int stride, size_t pitch);
/* Device views of the state after the last step (valid until the next step; every output nullable):
 * Tcw [nseq][16]; keys_xy [nseq][key_pitch][2] float; map_points [nseq][key_pitch][3] float and mp_valid [nseq][key_pitch]
 * bytes (entry j belongs to key j); key_counts [nseq]; obs [nseq][key_pitch] tb_obs rows and obs_counts [nseq] of the step's
 * pose optimisation (0 at frame 0); n_inliers [nseq]; outlier [nseq][key_pitch] flags of those rows. *frame = index of the
 * last frame stepped (-1 before any). */
int tb_vo_state_dev(tb_vo* vo, const float** Tcw, const float** keys_xy, const float** map_points, const uint8_t** mp_valid,
                    const int32_t** key_counts, const tb_obs** obs, const int32_t** obs_counts, const int32_t** n_inliers,
                    const uint8_t** outlier, int* key_pitch, int* frame);

/* ---- ragged batches: per-sequence reset, idle and keyframes
 * The lock-step entry points above give every sequence the same frame index. These three drive the same loop the way batches
 * arrive: a sequence may be restarted in its slot while the others go on, sit a step out, or take a keyframe off the cadence.
 * A sequence inside a ragged batch computes exactly what it computes alone: frame t_s of sequence s is frame t_s of a loop that
 * runs this sequence by itself through tb_vo_step_dev, bit for bit.
 *
 * tb_vo_reset_seq_dev: `which` is a HOST array [nseq]; Tcw0 a device array [nseq][16], read only where which[s] is set. A
 * selected sequence returns to the state tb_vo_reset_dev gives it (no keys, pose Tcw0[s], no keyframe, for TB_VO_BOW no keyframe
 * FeatureVector / BowVector, frame index -1); the other sequences keep every byte. The call puts the loop into ragged mode; it is
 * legal before any reset and at any point of a run. tb_vo_reset_dev leaves ragged mode. In ragged mode tb_vo_step_dev is
 * TB_ESTATE. Asynchronous.
 *
 * tb_vo_step_ragged_dev: `active` and `force_keyframe` are HOST arrays [nseq]; NULL active = every sequence, NULL
 * force_keyframe = none. For every active sequence s, frame t_s = (its frame index) + 1 is processed; it is a keyframe iff
 * t_s % keyframe_every == 0 or force_keyframe[s] (frame 0 always is). `right` is needed (TB_EINVAL otherwise) iff some active
 * sequence has a keyframe. An idle sequence keeps every state tensor of tb_vo_state_dev, tb_vo_tracker_state_dev,
 * tb_vo_bow_state_dev, tb_vo_mp_desc_dev (their live entries: what the counts cover) and its copy of the last left image; its
 * slabs of left / right are not interpreted. An active sequence that was never reset is TB_ESTATE; a step in which every
 * sequence idles is TB_OK and changes nothing. The call is also legal after tb_vo_reset_dev: when every sequence is active, at
 * the same frame, with the same keyframe decision, it launches exactly what tb_vo_step_dev launches; any other step puts the
 * loop into ragged mode. The views' pointers may change from one ragged step to the next: take them again after every step.
 *
 * How a ragged step is made: the host knows the masks, so nothing is decided on the device and nothing is read back. The step
 * uploads the mask and the compacted list of keyframe sequences from pinned memory with one hipMemcpyAsync -- the one host ->
 * device copy a ragged step adds. The tracking half runs over all nseq sequences as at frame t > 0 (a freshly reset sequence has
 * no keys and no keyframe, so it gets no match, no row, and keeps its pose), into a second set of the per-frame outputs; then
 * one kernel gives the idle sequences back what they held and sets a frame-0 sequence's match count, flags and inliers to 0. The
 * keyframe half runs only when some sequence has a keyframe, on a compacted batch of those sequences: its cost follows their
 * number, not nseq.
 *
 * tb_vo_frames: HOST arrays [nseq], each nullable: the frame index of every sequence (-1 before its first step) and the frame
 * index of its keyframe (-1: none). It works in lock-step mode too, where every entry equals tb_vo_state_dev's *frame /
 * tb_vo_tracker_state_dev's *kf_frame. In ragged mode those two report the largest per-sequence value.
 *
 * Supported: TB_VO_OPFLOW, TB_VO_BF, TB_VO_NN, TB_VO_VIOLENCE, TB_VO_PROJECTION, and TB_VO_BOW without a database. TB_EUNSUPPORTED from
 * tb_vo_reset_seq_dev and tb_vo_step_ragged_dev: TB_VO_PROJECTION_MAP (the map's block count and eviction are counted on the host
 * for the whole batch) and a TB_VO_BOW loop after tb_vo_bow_db_enable (database, store, recovery: the ring slot is the host's
 * count of adds for the whole batch). Making those two per-sequence is a later change.
 * A TB_VO_OPFLOW loop after tb_vo_window_ba_enable is refused by both as well (TB_EUNSUPPORTED): the slot of the segment log a
 * frame goes to is the host's count of frames since the keyframe, for the whole batch. */
int tb_vo_reset_seq_dev(tb_vo* vo, const uint8_t* which, const float* Tcw0);
int tb_vo_step_ragged_dev(tb_vo* vo, const uint8_t* left, const uint8_t* right, int stride, size_t pitch, const uint8_t* active,
                          const uint8_t* force_keyframe);
int tb_vo_frames(tb_vo* vo, int32_t* frames, int32_t* kf_frames);

/* The tracker of the loop: test_kitti's four tracking lines (:711-716) are switched by commenting them in and out; besides
 * optical flow (:716) the two descriptor trackers named with full arguments run here:
 *   TB_VO_BF        searchByBF(cur, key_frame, 0, 5, 10, 30) (:712): only the whole-set branch exists (matcher.cpp:177), so
 *                   (min_level, max_level) must be (0, nlevels) -- Frame::GetMaxLevel() returns nLevels -- else TB_EUNSUPPORTED
 *   TB_VO_VIOLENCE  searchByViolence(cur, key_frame, 0, 5, 50) (:713) with the Matcher's TH_LOW, nRatio, HISTO_LENGTH and
 *                   checkOrientation as setBowParam(50, 100, 30, true, 6) (:709) leaves them: 50, 6, 30, 1; histo_len in 1..1024,
 *                   radius > 0 and min_level <= max_level (TB_EINVAL otherwise)
 * A descriptor frame t (test_vo_1 :169-300 is the same loop written out):
 *   extract   ORB operator()(pyramid, target, init_th, min_th) on every left image; the records / descriptors are the frame's keys
 *   tracking  t > 0: the matcher, current frame (query) against the last keyframe (train); for every match whose keyframe entry
 *             trainIdx has a map point, key queryIdx gets it (Frame::AddMapPoint overwrites: a later match in list order wins;
 *             both matchers emit each queryIdx at most once); PoseOptimization from the last frame's pose on one row per key
 *             with a map point, IN KEY ORDER (LocalBA.cpp:333-363): px = the key, Xw = its map point, invSigma2 =
 *             invLevelSigma2[octave]; fewer than 3 rows hold the pose and n_inliers = 0
 *   keyframe  t % keyframe_every == 0: test_kitti's second ORB call on the same pyramid (:774-785) returns the same keys, so
 *             SetKeys resizes m to m and keeps every carried map point: it is not run again; then AddMapPointsByStereo and the new
 *             map points exactly as the optical-flow loop makes them; the frame becomes the keyframe (its records, descriptors,
 *             map points and, for violence, its lookup grid -- built once per keyframe)
 * As for optical flow, after the first step a step makes no host synchronisation and no host <-> device copy; the matcher's flags
 * stay on the device (tb_vo_tracker_state_dev; violence with factor = 1 / HISTO_LENGTH never flags).
 *
 * The projection trackers: test/test_projection.cpp test_projection (:449-646) is test_kitti's loop with the tracking line
 * replaced by one of two commented lines, both named with full arguments:
 *   TB_VO_PROJECTION      setProjectionParam(30, 50, 30, true, 30); searchByProjection(cur, key_frame) (:512-513): nratio 30,
 *                         th_high 50, histo_len 30, check_orientation 1. F1 = the current frame, F2 = the keyframe: its keys
 *                         (octave, angle), its key-aligned map points and those points' descriptors
 *   TB_VO_PROJECTION_MAP  setProjectionParam(30, 50, 30, true, 20); searchByProjection(map_ptr, cur, 0.6) (:516-517): nratio 20,
 *                         radio 0.6, th_high 50, against the sequence's own map; trainIdx indexes the live map
 *                         (map_ptr->GetAllMapPoints().at(trainIdx), :527). The predicted level is the reference's constant 0, so
 *                         only keys of octave 0 can match (Frame.cpp:403, matcher.cpp:568)
 * th_high >= 0, histo_len in 1..1024 and, for the map, map_keyframes >= 1 (TB_EINVAL otherwise). A projection frame t follows
 * the descriptor frame above, with these differences:
 *   every frame  after ORB, AssignFeaturesToGrid on the current frame's keys (:504): the matchers look up the CURRENT frame's
 *                grid. The pose the matcher projects with is the last frame's Tcw (:510)
 *   tracking     t > 0: taken1 is all zero -- Frame::AddMapPoint (Frame.cpp:322-326) never calls AddObservation, so
 *                Observations() is 0 throughout the loop. The matchers emit one match per map point, so several matches may
 *                name one key: the later match in list order wins it. Rows in key order, invSigma2 by octave, fewer than 3 rows
 *                hold the pose, as above
 *   descriptor   a map point's descriptor is the row of the frame that created it (MapPoint.cpp:35-36, :631), not the keyframe's
 *                row at the entry it was carried to: 32 bytes travel with xyz, in the frame state and in the keyframe snapshot
 *   keyframe     as above; with the map, every new point is also appended to it in key order (:631-634) as a tb_mappoint:
 *                pos, normal = (pos - Ow) / |pos - Ow| (MapPoint.cpp:22-24; float32, left to right), min_dist 1 and max_dist
 *                1000 (the constants GetMin/MaxDistanceInvariance return, MapPoint.cpp:207-217: a point nearer than 1 m or farther
 *                than 1000 m never matches -- reproduced, not fixed), bad 0, and the key's descriptor. map_ptr->AddKeyFrame (:635)
 *                has no effect on matching and is dropped
 * The map (the one deviation): the reference's map only grows; device memory is fixed, so the map holds the points of the last
 * map_keyframes keyframes (capacity map_keyframes * key_pitch), in insertion order. When keyframe number map_keyframes + 1 arrives
 * the oldest keyframe's points leave as a block and the rest move down (a keyframe that spawned no point still counts as a
 * block). A run with at most map_keyframes keyframes is the reference's loop exactly. The match list of the map tracker holds one
 * match per map point at most: its capacity is the map's, not key_pitch (tb_vo_map_state_dev). */
enum { TB_VO_OPFLOW = 0, TB_VO_BF = 1, TB_VO_VIOLENCE = 2, TB_VO_PROJECTION = 3, TB_VO_PROJECTION_MAP = 4, TB_VO_BOW = 5 };
typedef struct tb_vo_tracker {
    int kind;                       /* TB_VO_OPFLOW, TB_VO_BF, TB_VO_VIOLENCE, TB_VO_PROJECTION, TB_VO_PROJECTION_MAP */
    float bf_ratio, bf_min_th;      /* searchByBF ratio / minTh (:712: 10, 30) */
    int min_level, max_level;       /* both descriptor trackers (:712, :713: 0, 5) */
    float radius;                   /* searchByViolence search radius (:713: 50) */
    int th_low; float nratio; int histo_len; int check_orientation;   /* the Matcher's fields at :713: 50, 6, 30, 1;
                                       projection: nratio 30 (map: 20), histo_len 30, check_orientation 1 */
    int th_high;                    /* projection trackers: the Matcher's TH_HIGH (50) */
    float radio;                    /* TB_VO_PROJECTION_MAP: searchByProjection's radio (0.6) */
    int map_keyframes;              /* TB_VO_PROJECTION_MAP: keyframes the map holds (4) */
} tb_vo_tracker;
/* tb_vo_create with a tracker; tracker NULL or kind TB_VO_OPFLOW = tb_vo_create. */
int tb_vo_create_ex(tb_ctx* ctx, const tb_vo_params* params, const tb_vo_tracker* tracker, int nseq, tb_vo** out);
/* Device views of a descriptor tracker's state after the last step (valid until the next step; every output nullable; TB_ESTATE
 * for an optical-flow loop):
 *   orb [nseq][key_pitch] tb_keypoint, orb_desc [nseq][key_pitch][32], orb_counts [nseq]: the current frame's ORB keys (= its keys)
 *   matches [nseq][key_pitch] (queryIdx = current key, trainIdx = keyframe key), match_counts [nseq] (0 at frame 0), flags [nseq];
 *   TB_VO_PROJECTION_MAP: matches [nseq][map capacity], trainIdx = live map index
 *   the keyframe: kf_orb / kf_desc / kf_counts as above, kf_map_points [nseq][key_pitch][3], kf_mp_valid [nseq][key_pitch];
 *   *kf_frame = the index of its frame (-1 before any) */
int tb_vo_tracker_state_dev(tb_vo* vo, const tb_keypoint** orb, const uint8_t** orb_desc, const int32_t** orb_counts,
                            const tb_match** matches, const int32_t** match_counts, const int32_t** flags, const tb_keypoint** kf_orb,
                            const uint8_t** kf_desc, const float** kf_map_points, const uint8_t** kf_mp_valid,
                            const int32_t** kf_counts, int* kf_frame);
/* The fourth tracking line of test_kitti, searchByBow (:711), with Frame::SetBow (:705) on the device:
 *   TB_VO_BOW  setBowParam(50, 100, 30, true, 6) (:706); searchByBow(cur, key_frame, true): th_low 50, nratio 6 (which makes the
 *              ratio test vacuous -- reproduced, not fixed), histo_len 30, check_orientation 1, map_point_only 1, levelsup 4
 *              (Frame.cpp:269). test_vo_1's set (:207, :212) is th_low 30, nratio 5, map_point_only 0.
 * :711 as written reads searchByBow(cur_frame_ptr, cur_frame_ptr, true), a frame against itself, which tracks nothing; test_vo_1
 * :212 and the neighbouring lines :712-713 match against key_frame, so the train frame here is the keyframe.
 * A BoW frame t is the descriptor frame above with these differences:
 *   every frame  after ORB, SetBow: tb_bow_transform_batch_dev with levelsup (word, weight and node per key, the FeatureVector
 *                keys), then tb_bow_vector_batch_dev (the BowVector)
 *   tracking     t > 0: tb_search_by_bow_batch_dev, F1 = the current frame, F2 = the keyframe, has_mp2 = the keyframe snapshot's
 *                kf_mp_valid. Each queryIdx occurs at most once; the carry, the rows in key order, invSigma2 by octave and the
 *                rule for fewer than 3 rows are the descriptor frame's
 *   keyframe     the snapshot also keeps the keyframe's word and node ids, FeatureVector keys and BowVector as SetBow computed
 *                them on that frame: they are not computed again
 * The loop has its own creation entry because it needs a vocabulary; tb_vo_tracker keeps its layout and tb_vo_create_ex refuses
 * TB_VO_BOW. voc (tb_vocab_create, tb_vocab_train*, on the same context) is BORROWED: it must outlive the tb_vo; NULL or a
 * vocabulary of another context is TB_EINVAL. histo_len outside 1..1024, levelsup < 0 or th_low < 0 is TB_EINVAL (so is a
 * zero-initialised tb_vo_bow); a key capacity above 8192 is TB_EUNSUPPORTED. The transform's and the matcher's buffers are sized
 * in the create call: after the first step a step makes no host synchronisation and no host <-> device copy.
 * tb_vo_state_dev and tb_vo_tracker_state_dev serve this loop as they serve the other descriptor trackers. */
typedef struct tb_vo_bow {
    int levelsup;           /* Frame::SetBow's levelsup (4) */
    int map_point_only;     /* searchByBow's MapPointOnly (:711: 1): skip keyframe keys without a map point */
    int th_low; float nratio; int histo_len; int check_orientation;   /* the Matcher's fields after :706: 50, 6, 30, 1 */
} tb_vo_bow;
int tb_vo_create_bow(tb_ctx* ctx, const tb_vo_params* params, const tb_vo_bow* bow, const tb_vocab* voc, int nseq, tb_vo** out);
/* The tracking line test_vo_1 itself runs, searchByNN (test/test_vo.cpp:213):
 *   TB_VO_NN  searchByNN(cur_frame_ptr, key_frame, 0, 5, 10, 30) with the Matcher's LshIndexParams(20, 10, 2): ratio 10, min_th
 *             30, (min_level, max_level) = (0, nlevels) -- only the whole-set branch exists, anything else is TB_EUNSUPPORTED --
 *             tables 20, key_size 10, multi_probe_level 2, and the bit table of tb_lsh_create (bits, or drawn from seed when
 *             bits is NULL; read during the call only). The table is fixed for the life of the loop.
 * A frame is the descriptor frame above with the matcher line swapped for tb_search_by_nn_batch_dev, current frame (query)
 * against the keyframe (train); each queryIdx occurs at most once, in ascending order. The matcher keeps no index between
 * calls, so the ragged entry points serve the loop as they serve TB_VO_BF. tb_vo_tracker keeps its layout: the loop has its
 * own creation entry and tb_vo_create_ex answers TB_VO_NN with TB_EINVAL. ratio / min_th not finite and LSH parameters outside
 * tb_lsh_create's limits are TB_EINVAL; a key capacity above 8192 is TB_EUNSUPPORTED. tb_vo_state_dev and
 * tb_vo_tracker_state_dev serve it; after the first step a step makes no host synchronisation and no host <-> device copy. */
enum { TB_VO_NN = 6 };
typedef struct tb_vo_lsh {
    float ratio, min_th;            /* searchByNN ratio / minTh (:213: 10, 30) */
    int min_level, max_level;       /* (:213: 0, 5) */
    int tables, key_size, multi_probe_level;   /* matcher.cpp:18: 20, 10, 2 */
    uint64_t seed;                  /* the bit table's seed when bits is NULL */
    const uint16_t* bits;           /* nullable: an explicit [tables][key_size] table */
} tb_vo_lsh;
int tb_vo_create_lsh(tb_ctx* ctx, const tb_vo_params* params, const tb_vo_lsh* lsh, int nseq, tb_vo** out);
/* Device views of SetBow's outputs after the last step (valid until the next step; every output nullable; TB_ESTATE for any other
 * tracker), for the current frame and, kf_*, for the keyframe as computed on its frame: fv_keys [nseq][key_pitch] uint64
 * (node << 32 | key) with fv_counts [nseq]; bv_words / bv_values [nseq][key_pitch] with bv_counts [nseq]; word_ids and node_ids
 * [nseq][key_pitch], entry j of key j. */
int tb_vo_bow_state_dev(tb_vo* vo, const uint64_t** fv_keys, const int32_t** fv_counts, const int32_t** bv_words, const double** bv_values,
                        const int32_t** bv_counts, const int32_t** word_ids, const int32_t** node_ids, const uint64_t** kf_fv_keys,
                        const int32_t** kf_fv_counts, const int32_t** kf_bv_words, const double** kf_bv_values, const int32_t** kf_bv_counts,
                        const int32_t** kf_word_ids, const int32_t** kf_node_ids);
/* The keyframe database of a TB_VO_BOW loop (off unless enabled): tb_vo_bow_db_enable creates a tb_bow_db of nseq rings of
 * `capacity` slots, pitch = the loop's key pitch, scoring = the vocabulary's. From then on every keyframe step adds the keyframe's
 * BowVector -- the one its snapshot holds -- with kf_id = the frame's index, after the snapshot, and tb_vo_reset_dev clears the
 * database; a step still makes no host synchronisation and no host <-> device copy. TB_ESTATE: another tracker, after the first
 * step, or enabled already; capacity outside 1..1024 is TB_EINVAL. tb_vo_bow_db_get lends the database (tb_bow_db_query_dev with
 * tb_vo_bow_state_dev's bv_* as the query, tb_bow_db_state_dev); it belongs to the loop and goes with it. TB_ESTATE when the
 * database is not enabled. */
int tb_vo_bow_db_enable(tb_vo* vo, int capacity);
int tb_vo_bow_db_get(tb_vo* vo, tb_bow_db** out);
/* Relocalisation in a TB_VO_BOW loop (off unless enabled; a loop that does not enable it launches what it launched before).
 * tb_vo_reloc_enable creates a tb_kf_store with the database's capacity and the loop's key pitch; from then on a keyframe step
 * adds the snapshot right after the database add -- key records, descriptors, FeatureVector keys, kf_map_points, kf_mp_valid, the
 * frame's optimised Tcw, kf_id = the frame's index -- and tb_vo_reset_dev clears the store. TB_ESTATE: another tracker, the
 * database not enabled, after the first step, or enabled already; max_candidates outside 1..capacity is TB_EINVAL.
 * tb_vo_relocalize_dev is a query: tb_bow_db_query_dev(topk, exclude_newest) with the current frame's BowVector, then
 * tb_relocalize_batch_dev of the current frame's ORB records, descriptors and FeatureVector against top_slot with the loop's
 * tb_vo_bow fields. It changes neither the loop's pose nor its carried points nor its keyframe, and makes no host synchronisation
 * and no host <-> device copy. scores [nseq][capacity], top_slot / top_kf / top_score [nseq][topk] and top_count [nseq] are the
 * query's outputs (each nullable: the loop has buffers of its own); topk in 1..max_candidates. TB_ESTATE: not enabled, or before
 * the first step. ORB-SLAM's second stage (searchByProjection with the recovered pose) is not part of it; adopting the pose after
 * a loss is tb_vo_recover_enable's, correcting the trajectory on a revisit tb_vo_loop_enable's. tb_vo_kf_store_get lends the store (TB_ESTATE when not enabled). */
int tb_vo_reloc_enable(tb_vo* vo, int max_candidates);
int tb_vo_relocalize_dev(tb_vo* vo, int topk, int exclude_newest, int min_inliers, double* scores, int32_t* top_slot, int32_t* top_kf,
                         double* top_score, int32_t* top_count, const tb_reloc_out* out);
int tb_vo_kf_store_get(tb_vo* vo, tb_kf_store** out);
/* tb_vo_relocalize_sim3_dev is a query after tb_vo_relocalize_dev: tb_kf_store_sim3_dev with the loop's own current ORB keys, its
 * carried map_points / mp_valid (tb_vo_state_dev's), its Tcw and the top_slot / topk of the last tb_vo_relocalize_dev. It changes
 * no state tensor and makes no host synchronisation and no host <-> device copy (the store's first Sim(3) call may allocate); it
 * works whether or not recovery, loop correction or the PnP verification are on, because it only reads. TB_ESTATE: relocalisation
 * not enabled, before the first step, or no tb_vo_relocalize_dev since the last step. topk sizes the outputs ([nseq][topk]) and
 * must be the topk of that tb_vo_relocalize_dev: anything else is TB_EINVAL and nothing is written. tb_vo_relocalize_dev keeps a
 * device copy of a top_slot the caller took, so that buffer need not outlive the call. */
struct tb_sim3_params;
int tb_vo_relocalize_sim3_dev(tb_vo* vo, int topk, const struct tb_sim3_params* params, int min_consensus, const tb_sim3_out* out);
/* tb_vo_loop_sim3_dev is a query after tb_vo_relocalize_sim3_dev: tb_kf_store_sim3_graph_dev with the loop's current pose as the
 * query frame, whose node carries the frame index in node_kf. TB_ESTATE: relocalisation not enabled, or no
 * tb_vo_relocalize_sim3_dev since the last step (every step and reset invalidates it). No state of the loop or the store changes:
 * adopting the corrected nodes is left to a later change. */
int tb_vo_loop_sim3_dev(tb_vo* vo, int iters, int fixed_scale, double w_rot, double w_trans, double w_scale, tb_sim3_graph_out* out);
/* tb_vo_refine_sim3_dev is a query after tb_vo_relocalize_sim3_dev: tb_kf_store_sim3_refine_dev with the same arguments that call
 * made -- the loop's current ORB keys, its carried map points and pose, the candidates of the last tb_vo_relocalize_dev. cand_srt /
 * cand_consensus: what tb_vo_relocalize_sim3_dev wrote (NULL for one it kept in the store). topk: that of the last
 * tb_vo_relocalize_dev, which sizes every input and output; any other count is TB_EINVAL. TB_ESTATE: relocalisation not enabled, or
 * no tb_vo_relocalize_sim3_dev since the last step (every step and reset invalidates it), or a tb_vo_relocalize_dev since that query
 * (the match lists are no longer the ones its masks and seeds belong to). With use_for_graph = 0 no state of the
 * loop or the store changes, and a loop that never calls it ends in the same bytes; with 1 the next tb_vo_loop_sim3_dev takes the
 * refined transform as its loop edge. */
struct tb_sim3_opt_params;
int tb_vo_refine_sim3_dev(tb_vo* vo, int topk, const double* cand_srt, const int32_t* cand_consensus, const struct tb_sim3_opt_params* params,
                          int min_inliers, int use_for_graph, const tb_sim3_refine_out* out);
/* tb_vo_search_sim3_dev is a query after tb_vo_relocalize_sim3_dev: tb_kf_store_sim3_search_dev with the loop's current ORB keys and
 * descriptors, its carried map points, its pose and its image size, on the candidates of the last tb_vo_relocalize_dev. cand_srt /
 * cand_consensus, topk and TB_ESTATE as tb_vo_refine_sim3_dev's: every step and reset invalidates it, and so does a
 * tb_vo_relocalize_dev after the Sim(3) query. It reads the loop and writes only the store's search buffers: a loop that never calls
 * it ends in the same bytes. With use_for_refine = 1 the next tb_vo_refine_sim3_dev refines on the widened lists. */
int tb_vo_search_sim3_dev(tb_vo* vo, int topk, const double* cand_srt, const int32_t* cand_consensus, float th, int th_high, int use_for_refine,
                          const tb_sim3_search_out* out);
/* tb_kf_store_pnp_enable on the loop's store: tb_vo_relocalize_dev then runs the PnP verification (tb_kf_store_pnp_state_dev on
 * tb_vo_kf_store_get's store lends its per-pair outputs) and stays a query that changes no state tensor. TB_ESTATE: relocalisation
 * not enabled, after the first step, enabled already, or together with tb_vo_recover_enable / tb_vo_loop_enable in either order:
 * their adoption kernels read the verification's rows by key, and have to be read against gathered rows first. */
int tb_vo_reloc_pnp_enable(tb_vo* vo, const tb_pnp_params* params, int min_consensus, int expand);
/* Recovery in a TB_VO_BOW loop with relocalisation (off unless enabled; a loop that does not enable it launches what it launched
 * before): a sequence that loses track adopts the relocalisation pose and tracks against the keyframe that gave it. The reference
 * has no such step; every operator is the reference's -- searchByBow (matcher.cpp:619-721), PoseOptimization and its rows
 * (LocalBA.cpp:291-490, :333-363) -- and the composition is this library's (tests/vo_recover_reference.py restates it on the CPU
 * oracle). At frame t > 0, after the tracking step's pose optimisation and before the keyframe block:
 *   flag    lost[s] = n_inliers[s] < lost_inliers; track_inliers[s] = n_inliers[s]
 *   query   tb_bow_db_query_dev(topk, exclude_newest) with the current BowVectors, as tb_vo_relocalize_dev
 *   mask    a copy of top_slot in which a sequence that is not lost has -1 throughout: its pairs read nothing and can never win
 *   verify  tb_relocalize_batch_dev on the masked slots with the loop's tb_vo_bow fields and min_inliers
 *   adopt   where lost[s] and best_rank[s] >= 0: Tcw = best_Tcw; the carried map points are those of the winning pair's matches
 *           by the rows rule above (the last match in list order wins a key; the failed step's points are dropped; outlier rows
 *           keep theirs); obs, obs_counts, outlier, n_inliers, matches, match_counts and flags are the pair's;
 *           recovered_kf[s] = best_kf[s]. Every other sequence: recovered_kf -1 and no other byte of its state changes
 *   switch  an adopting sequence's rows of the keyframe snapshot (tb_vo_tracker_state_dev's kf_*, tb_vo_bow_state_dev's kf_*) take
 *           the winning ring slot: the store's arrays, the database's BowVector and the word / node ids of two rings
 *           [nseq][capacity][key_pitch] the loop fills at every keyframe step; kf_ids[s] = best_kf[s]. Live entries only
 * then, on a keyframe step, the keyframe block as before: the frame spawns its stereo points at the adopted pose, becomes the
 * keyframe of every sequence (kf_ids[s] = t) and goes into the database, the store and the rings. The stage is on the context's
 * stream: no host synchronisation, no host <-> device copy; which sequences adopt is decided by device predicates alone.
 * tb_vo_tracker_state_dev's *kf_frame stays the last keyframe step. tb_vo_reset_dev clears the state (flags 0, ids -1).
 * tb_vo_recover_enable allocates every buffer. TB_ESTATE: relocalisation not enabled, after the first step, enabled already, or
 * loop correction enabled (tb_vo_loop_enable);
 * TB_EINVAL: null params, lost_inliers < 0, min_inliers < 0, exclude_newest < 0, topk outside 1..max_candidates.
 * tb_vo_recover_state_dev: device views, each nullable (TB_ESTATE when not enabled): lost [nseq] and track_inliers [nseq] of the
 * last step (the tracker's own count, before any adoption), recovered_kf [nseq] (the adopted keyframe's kf_id, or -1), kf_ids
 * [nseq] (the frame index of the keyframe each sequence now tracks against, -1 before any), and the rings kf_word_ring /
 * kf_node_ring [nseq][capacity][key_pitch], slot-aligned with the store. */
typedef struct tb_vo_recover {
    int lost_inliers;     /* a sequence is lost at frame t > 0 when the tracking step's n_inliers < lost_inliers */
    int topk;             /* candidates per lost sequence, 1..max_candidates of tb_vo_reloc_enable */
    int exclude_newest;   /* as tb_bow_db_query_dev */
    int min_inliers;      /* as tb_reloc_params */
} tb_vo_recover;
int tb_vo_recover_enable(tb_vo* vo, const tb_vo_recover* prm);
int tb_vo_recover_state_dev(tb_vo* vo, const uint8_t** lost, const int32_t** track_inliers, const int32_t** recovered_kf,
                            const int32_t** kf_ids, const int32_t** kf_word_ring, const int32_t** kf_node_ring);
/* Loop correction in a TB_VO_BOW loop with relocalisation, lock-step (off unless enabled; a loop that does not enable it launches
 * what it launched before): a verified revisit is spread back over the stored keyframes by tb_pose_graph_batch_dev. The reference
 * has no such step; the composition is this library's, restated on the CPU oracle in tests/vo_loop_reference.py. At a keyframe
 * step t > 0, after the tracking step's pose optimisation and before the keyframe block, all on the context's stream with no host
 * synchronisation and no host <-> device copy:
 *   query   tb_bow_db_query_dev(topk, exclude_newest) and tb_relocalize_batch_dev with the loop's tb_vo_bow fields and
 *           min_inliers, into the loop's own buffers, as tb_vo_relocalize_dev
 *   graph   k_vo_loop_graph: capacity + 1 nodes per sequence -- the live ring slots in ascending kf_id, then the current frame;
 *           the unused nodes hold the identity and no edge names them. Node 0, the oldest, is fixed. Odometry edges join
 *           consecutive nodes, Z = T_next T_prev^-1 from the stored poses and the current pose; one loop edge joins the winning
 *           keyframe's node to the current node, Z = best_Tcw T_j^-1; weights w_rot, w_trans. best_rank < 0, or fewer than 2
 *           keyframes held: edge count 0
 *   solve   tb_pose_graph_batch_dev's kernel on the nseq graphs, nfixed = 1, iters
 *   adopt   k_vo_loop_adopt, where a loop edge was built and the solver did not flag the graph: every stored keyframe's Tcw
 *           becomes its node's pose and its valid map points move rigidly with it, X' = T_new^-1 T_old X in FP64 stored as float32;
 *           the keyframe snapshot (kf_map_points) and the frame's carried map points, copies of the newest keyframe's points, move
 *           by the newest keyframe's correction; the current Tcw becomes the last node's pose. obs, outlier, n_inliers and the
 *           match list stay: they describe the tracking step. Every other sequence keeps every byte
 * then the keyframe block as before: the frame spawns its stereo points at the corrected pose and goes into the database and the
 * store with it. tb_vo_loop_enable allocates every buffer and plans the solver's work buffer (tb_pose_graph_plan), so no step
 * grows it. TB_ESTATE: relocalisation not enabled (any other tracker, no database, no store), after the first step, a ragged
 * loop, enabled already, or recovery enabled (tb_vo_recover_enable on a loop with correction is TB_ESTATE too: combining the two is
 * a later change); TB_EINVAL: null params, a store capacity above 63 (nodes = keyframes + the frame <= 64), topk outside
 * 1..max_candidates, exclude_newest < 0, min_inliers < 0, iters outside 0..99, a negative or non-finite weight.
 * tb_vo_loop_state_dev: device views of the last keyframe step t > 0, each nullable (TB_ESTATE when not enabled): closed [nseq],
 * loop_kf [nseq] (the keyframe's kf_id, -1 when nothing closed), loop_inliers [nseq], nnodes [nseq] (live keyframes + 1), node_kf
 * [nseq][capacity + 1] (kf_id per node, the frame index for the current frame, -1 unused), before / after [nseq][capacity + 1][16],
 * edges [nseq][capacity + 1] with edge_counts [nseq], stats [nseq][8] (tb_pose_graph_batch_dev's). tb_vo_reset_dev clears them. */
typedef struct tb_vo_loop {
    int topk;             /* candidates per sequence, 1..max_candidates of tb_vo_reloc_enable */
    int exclude_newest;   /* as tb_bow_db_query_dev */
    int min_inliers;      /* as tb_reloc_params: a loop closes when the best candidate keeps at least this many */
    int iters;            /* LM iterations of the pose graph */
    double w_rot, w_trans; /* the edges' information, diag(w_rot I3, w_trans I3) */
} tb_vo_loop;
int tb_vo_loop_enable(tb_vo* vo, const tb_vo_loop* prm);
int tb_vo_loop_state_dev(tb_vo* vo, const uint8_t** closed, const int32_t** loop_kf, const int32_t** loop_inliers, const int32_t** nnodes,
                         const int32_t** node_kf, const float** before, const float** after, const tb_pg_edge** edges,
                         const int32_t** edge_counts, const double** stats);
/* Window BA in a TB_VO_OPFLOW loop in lock-step (off unless enabled; a loop that does not enable it launches what it launched
 * before): every keyframe segment is refined by tb_local_ba_batch_dev before the keyframe spawns its stereo points. The reference
 * has no such step (its map_ptr->AddKeyFrame is commented out); the operators are this library's and the composition is restated
 * on the CPU oracle in tests/vo_window_reference.py. Between two keyframes key i of every frame is the same physical point
 * (k_vo_track keeps the index, lost points included), so the E + 1 = keyframe_every + 1 frames from one keyframe to the next are a
 * BA window over the first keyframe's stereo points: with fixed = 1, E free keyframes (10 by default: the MFMA-tiled path's limit).
 *   segment start  at the end of every keyframe step's keyframe block, frame 0 included: slot 0 of the log takes the keyframe's
 *                  keys (after SetKeys) and pose, seg_pts the frame's map points (zeros where a key has none), and seg_spawned[i] = 1 where the keyframe made
 *                  a stereo point at key i in this step (depth > 0 and finite); seg_ok[0] = seg_spawned. An entry that survived
 *                  only through SetKeys' resize is valid but not spawned and never enters a window
 *   log            every frame t > 0, after the tracking half, into slot j = t - (the keyframe's frame): the tracked keys, the
 *                  optimised pose, and seg_ok[j][i] = seg_spawned[i] & valid[i] & !outlier[row(i)], row(i) = key i's rank among
 *                  the frame's valid keys (the order of PoseOptimization's rows). Fewer than 3 rows held the pose: ok is 0
 *   window         on a keyframe step t > 0, after the log and before the keyframe block: a point with at least min_obs ok slots
 *                  gives one tb_ba_obs {kf = slot, pt = key index, u, v, inv_sigma2 = 1} per ok slot, grouped by ascending
 *                  point and, within a point, by ascending slot; obs_counts and the number of such points go beside it
 *   BA             tb_local_ba_batch_dev(nseq windows, nkf = E + 1, nfixed = fixed, npt = key_pitch, obs_pitch = (E + 1) *
 *                  key_pitch, iters) on a COPY of seg_pose / seg_pts (ba_pose / ba_pts: the smoothed segment; the log keeps
 *                  what the tracker measured). A window without observations is left as it is by the BA (no iteration)
 *   adopt          where the window has at least min_points points, stats[7] != -1 and every entry of ba_pose[E] is finite:
 *                  the frame's Tcw = ba_pose[E], adopted = 1; otherwise the pose keeps every bit and adopted = 0. The keyframe
 *                  block then runs unchanged and spawns at that pose. The frame's carried map points are not touched
 * The BA call synchronises the stream once (LM termination is data dependent): the one host synchronisation a keyframe step
 * gains. Tracking steps stay free of host synchronisation and host <-> device copies. A sequence's log, window and adoption do
 * not depend on the batch; the BA's bits are tb_local_ba_batch_dev's, which deals its Schur workgroups by the number of windows.
 * tb_vo_window_ba_enable allocates every buffer and sizes the BA's workspace. TB_ESTATE: not an optical-flow loop, after the
 * first step, or enabled already; TB_EINVAL: null params, iters outside 1..99, fixed outside 1..keyframe_every, min_obs < 2,
 * min_points < 1; TB_EUNSUPPORTED: keyframe_every + 1 - fixed > 64 (the BA's limit on free keyframes; 128 frames in all).
 * tb_vo_reset_dev clears the state. tb_vo_reset_seq_dev and tb_vo_step_ragged_dev are TB_EUNSUPPORTED on an enabled loop.
 * tb_vo_window_state_dev: device views, each nullable (TB_ESTATE when not enabled), E + 1 = *nslots:
 *   seg_keys [nseq][E + 1][key_pitch][2] float, seg_ok [nseq][E + 1][key_pitch] bytes, seg_pose [nseq][E + 1][16],
 *   seg_pts [nseq][key_pitch][3], seg_spawned [nseq][key_pitch] bytes: the log of the running segment (slots 0..*slot are this
 *   segment's, *slot = frames since its keyframe; later slots still hold the previous segment's);
 *   obs [nseq][(E + 1) * key_pitch], obs_counts [nseq], n_points [nseq], stats [nseq][8] (tb_local_ba_batch_dev's), adopted
 *   [nseq] bytes, ba_pose [nseq][E + 1][16] and ba_pts [nseq][key_pitch][3]: the last window and its refined segment. */
typedef struct tb_vo_window_ba {
    int iters;        /* LM iterations (10) */
    int fixed;        /* leading frames of the window held fixed (1: the keyframe; 2 measured worse) */
    int min_obs;      /* ok slots a point needs to enter the window (2) */
    int min_points;   /* points a window needs for its pose to be adopted (3) */
} tb_vo_window_ba;
int tb_vo_window_ba_enable(tb_vo* vo, const tb_vo_window_ba* prm);
int tb_vo_window_state_dev(tb_vo* vo, const float** seg_keys, const uint8_t** seg_ok, const float** seg_pose, const float** seg_pts,
                           const uint8_t** seg_spawned, const tb_ba_obs** obs, const int32_t** obs_counts, const int32_t** n_points,
                           const double** stats, const uint8_t** adopted, const float** ba_pose, const float** ba_pts, int* slot,
                           int* nslots);
/* Monocular map growth in a TB_VO_OPFLOW loop in lock-step (off unless enabled; a loop that does not enable it launches what it
 * launched before): after frame 0 the keyframes need no right image, and new map points come from triangulating the LK tracks.
 * The reference has no such loop; its LocalBA::LinearTriangle is the operator (tb_linear_triangle_batch_dev above) and the
 * composition is restated on the CPU oracle in tests/vo_mono_reference.py. Between two keyframes key i of every frame is the
 * same physical point (k_vo_track keeps the index), so a key seen at the keyframe and now is a point pair with two known poses.
 *   frame 0        unchanged: ORB, stereo depths, stereo points; it needs `right`, which fixes the scale. Then kf_keys = the key
 *                  list as the keyframe left it, kf_Tcw = the frame's pose, alive[i] = 1
 *   tracking       unchanged, plus alive[i] &= status[i] (LK's status of the step)
 *   keyframe t > 0 `right` is not read and may be NULL. After the tracking half (alive updated as above):
 *     triangulate  tb_linear_triangle_batch_dev(kf_keys, the frame's keys, the frame's key counts, kf_Tcw, the optimised Tcw,
 *                  skip[i] = valid[i] || !alive[i], inv_sigma2 NULL) into tri_points / tri_flags / tri_tally; key i gets the map
 *                  point tri_points[i] where tri_flags[i] == 1
 *     merge        the new key list, by one workgroup per sequence (k_vo_kf_merge): first every key that has a map point, in
 *                  index order, with its point (their number -> survivors[s]); then the frame's ORB keys in extractor order,
 *                  without a map point, leaving out a key whose cell x cell pixel cell ((int)x / cell, (int)y / cell) holds a
 *                  survivor (only survivors mark cells; a key outside the ceil(width / cell) x ceil(height / cell) grid marks
 *                  and meets nothing), until the list holds key_pitch keys (their number -> added[s])
 *     afterwards   kf_keys = the new list, kf_Tcw = Tcw, alive = 1. No stereo operator runs and no depth is made
 * A mono loop makes no host synchronisation and no host <-> device copy after the first step.
 * tb_vo_mono_enable: before the first tb_vo_reset_dev. TB_EUNSUPPORTED: any tracker but TB_VO_OPFLOW, or a loop with the window
 * BA enabled (tb_vo_window_ba_enable on a mono loop is refused the same way); TB_ESTATE: after a reset, or enabled already;
 * TB_EINVAL: null or non-finite parameters, cell <= 0, or a cell whose occupancy bitmap (one bit per cell, in LDS) is above 32 KB.
 * tb_vo_reset_seq_dev and tb_vo_step_ragged_dev are TB_EUNSUPPORTED on a mono loop; tb_vo_reset_dev clears the state.
 * tb_vo_mono_state_dev: device views, each nullable (TB_ESTATE when not enabled): kf_keys_xy [nseq][key_pitch][2], kf_Tcw
 * [nseq][16], alive [nseq][key_pitch] bytes, tri_points [nseq][key_pitch][3] (meaningful where tri_flags is 1), tri_flags
 * [nseq][key_pitch] bytes, tri_tally [nseq][6], survivors [nseq], added [nseq]: the tri_* and the two counts are the last mono
 * keyframe's (zero before the first). */
typedef struct tb_vo_mono {
    double cos_parallax_max, chi2_max;   /* tb_triangulate_params (0.9998, 5.991) */
    int cell;                            /* side of the merge's occupancy cells in pixels (8) */
} tb_vo_mono;
int tb_vo_mono_enable(tb_vo* vo, const tb_vo_mono* prm);
int tb_vo_mono_state_dev(tb_vo* vo, const float** kf_keys_xy, const float** kf_Tcw, const uint8_t** alive, const float** tri_points,
                         const uint8_t** tri_flags, const int32_t** tri_tally, const int32_t** survivors, const int32_t** added);
/* The mono loop starting without a right image (off unless enabled: a mono loop that does not call it launches exactly what it
 * launched before): tb_two_view_batch_dev gives the first pose and points, `two_view.baseline` sets the scale. The composition is
 * restated on the CPU in tests/vo_mono_init_reference.py. Per sequence, initialised[s] starts at 0:
 *   frame 0        `right` is not read and may be NULL at every step. ORB only: keys = the ORB list, no key has a map point, Tcw =
 *                  the reset pose; kf_keys = keys, kf_Tcw = Tcw, alive = 1
 *   tracking       LK and alive &= status as in the mono mode. While initialised[s] == 0 no key has a map point, the pose stage
 *                  gets no rows and holds the pose: Tcw stays the reset pose bit for bit. An initialised sequence is the mono mode's
 *   keyframe t > 0 initialised[s] == 0: the sequence takes no part in the triangulation (its tri_flags are 0). The two-view operator
 *                  runs on (kf_keys, keys, the key count, skip = !alive, Tcw0 = kf_Tcw); attempts[s] += 1. Status 0 with at least
 *                  min_tracks alive keys: Tcw = Tcw1, key i takes points[i] where point_flags[i] == 1 (through tri_points /
 *                  tri_flags, which the merge reads), initialised[s] = 1, init_frame[s] = t. Otherwise nothing is adopted. Either
 *                  way the mono mode's merge follows -- with no survivor it yields a fresh ORB list, the re-seed -- and kf_keys,
 *                  kf_Tcw, alive are set as in the mono mode. initialised[s] == 1: the mono mode's keyframe, the same bytes
 * Which sequences initialise is decided on the device (k_vo_init_adopt); a step makes no host round trip.
 * tb_vo_mono_init_enable: after tb_vo_mono_enable and before the first tb_vo_reset_dev. TB_ESTATE: the mono mode is not enabled,
 * after a reset, or enabled already; TB_EINVAL: null parameters, min_tracks < 0, or two-view parameters tb_two_view_batch_dev
 * refuses; TB_EUNSUPPORTED: a key pitch above TB_TWO_VIEW_MAX_PITCH. tb_vo_reset_dev clears the state.
 * tb_vo_mono_init_state_dev: device views, each nullable (TB_ESTATE when not enabled): initialised [nseq] bytes, init_frame [nseq]
 * (-1: not yet), attempts [nseq], and the sequence's last attempt: status, consensus [nseq], winner [nseq][2], good / tri
 * [nseq][4], Tcw1 [nseq][16] (zero before the first). */
typedef struct tb_vo_mono_init {
    tb_two_view_params two_view;
    int min_tracks;              /* 100: fewer alive keys at the keyframe and nothing is adopted */
} tb_vo_mono_init;
int tb_vo_mono_init_enable(tb_vo* vo, const tb_vo_mono_init* prm);
int tb_vo_mono_init_state_dev(tb_vo* vo, const uint8_t** initialised, const int32_t** init_frame, const int32_t** attempts,
                              const int32_t** status, const int32_t** consensus, const int32_t** winner, const int32_t** good,
                              const int32_t** tri, const float** Tcw1);
/* Device views of the descriptors the projection trackers carry with the map points (TB_ESTATE for any other tracker):
 * mp_desc [nseq][key_pitch][32] next to tb_vo_state_dev's map_points, kf_mp_desc next to kf_map_points; entry j is read only
 * where its map point is valid. */
int tb_vo_mp_desc_dev(tb_vo* vo, const uint8_t** mp_desc, const uint8_t** kf_mp_desc);
/* Device views of the map of a TB_VO_PROJECTION_MAP loop after the last step (valid until the next step; every output nullable;
 * TB_ESTATE for a loop without a map): points [nseq][capacity] records in insertion order and desc [nseq][capacity][32], of which
 * counts[s] are live; block_counts [nseq][map_keyframes]: the points each held keyframe added, oldest first (*blocks of them are
 * in use). *capacity = map_keyframes * key_pitch = the match capacity. */
int tb_vo_map_state_dev(tb_vo* vo, const tb_mappoint** points, const uint8_t** desc, const int32_t** counts,
                        const int32_t** block_counts, int* capacity, int* map_keyframes, int* blocks);

/* ---- the depth filter: per sequence up to `pitch` seeds -- a pixel of a reference image with a Gaussian x Beta belief over the
 * inverse range along its ray -- that every later frame with a known pose narrows by an epipolar search, until the seed is a map
 * point. An operator next to the VO loop: it is fed poses and images and touches nothing of a loop. The definition, statement for
 * statement, is tests/depth_filter_reference.py; the kernels (k_depth_filter.hip) are held to it: flag, n, win and score bit for
 * bit, the float64 results at 1e-6 relative. The warp and the patch follow Matcher::FindMatchDirect (matcher.cpp:1518-1592), the
 * alignment the commented-out body of Matcher::Align1D (matcher.cpp:1247-1364), the depth, tau and the update the published SVO /
 * REMODE formulas; everything is float64 unless marked integer, one rounding per statement, sums left to right.
 *
 * A seed (tb_df_seed) starts with mu = 1 / depth_mean, z_range = 1 / depth_min, sigma2 = z_range^2 / 36, a = b = 10, state 1.
 * The update of one active seed against a frame (image, Tcw), with T_cr = Tcw Tcw_ref^-1 = (R, t) and f the unit ray of (u, v):
 *   1 range ends   d = 1 / mu, d_min = 1 / (mu + sqrt(sigma2)), d_max = 1 / max(mu - sqrt(sigma2), 1e-8); A and B are the
 *                  normalised-plane projections of R f d_min + t and R f d_max + t. BEHIND: one of the three depths is <= 0.
 *                  OUTSIDE: the point at d projects outside the image less a margin of 5 px. Both leave the seed unchanged.
 *   2 affine warp  A_cur_ref at depth d, level 0, half size 5. WARP, unchanged: its determinant is outside (1/3, 3) -- the
 *                  project's own rule: the search runs at level 0 only and the warp takes the scale.
 *   3 patch        the warped 10 x 10 patch with border as uint8: floor of the bilinear sample, 0 outside; the inner 8 x 8 is the patch.
 *   4 search       epi_len = the pixel distance of A and B; DEGENERATE, unchanged, below 1e-6. n = max(1, floor(epi_len / 0.7));
 *                  n > max_steps is NO_MATCH. Samples i = 0..n run from B to A, uniform on the normalised plane; each is rounded
 *                  to the integer pixel floor(p + 0.5); a sample on the previous sample's pixel is skipped, and so is a pixel
 *                  closer than 4 to the border. The score is the zero-mean SSD as an exact integer, 64 (sum AA - 2 sum AB + sum BB) -
 *                  (sum A - sum B)^2; the first minimum wins. No sample, or a best score >= 64 zmssd_max, is NO_MATCH.
 *   5 alignment    Align1D from the winning pixel along the unit pixel direction of the line, on the bordered patch, at most
 *                  align_iters iterations, with the mean-difference term, the "error increased" step back and the 0.03 px stop
 *                  of the reference's body; its 64-pixel sums take the butterfly p[t] = p[t] + p[t ^ d], d = 1 .. 32, t = 8 y + x.
 *                  Not converged is NO_MATCH.
 *   6 depth        z from the least-squares intersection of R f and the current unit ray; |det A'A| < 1e-6 is DEGENERATE,
 *                  unchanged -- the project's own rule: SVO counts a failed match there, which penalises the seeds near the
 *                  epipole of a camera that moves forward. tau by SVO's computeTau with px_error_angle = 2 atan(px_noise /
 *                  (2 sqrt(fx fy))) (acos arguments clamped to [-1, 1]); tau_inv = 0.5 (1 / max(1e-7, z - tau) - 1 / (z + tau)).
 *   7 update       the Vogiatzis-Hernandez update with x = 1 / z, tau2 = tau_inv^2. A non-finite sqrt(sigma2 + tau2) is
 *                  NONFINITE, unchanged. NO_MATCH is b += 1 and nothing else (but the count of updates).
 *   8 convergence  CONVERGED when sqrt(sigma2) < z_range / conv_div: state becomes 2; the world point is Tcw_ref^-1 (f / mu).
 *                  Converged and dropped seeds are not updated again.
 * Every update leaves one tb_df_trace an entry (flag -1 for an entry that is not active).
 * Keyframes: a sequence has a ring of ref_slots reference images with their poses. An add takes the slot after the newest one, sets
 * every seed still bound to that slot to state 3 (dropped: its entry counts as free from then on), and appends one seed per
 * offered key that is not skipped, in key order, into the entries that are free (state 0 or 3) in ascending entry order. Keys that
 * do not fit are not added; their count is returned.
 *
 * tb_depth_filter_create: K = (fx, fy, cx, cy); images are width x height. TB_EINVAL: nseq < 1, pitch < 1, ref_slots outside 1..16,
 * depth_min <= 0, depth_mean < depth_min, conv_div or px_noise not positive, max_steps < 1, zmssd_max < 0, align_iters outside 0..99,
 * a focal length that is not positive; TB_EUNSUPPORTED: an image under 16 px in either dimension, more than 65535 sequences.
 * Must be destroyed before its context. A filter that is never created changes nothing in any other call.
 * `active` (add, update) and `which` (clear) are nullable HOST byte masks [nseq], as in tb_vo_step_ragged_dev: NULL = every sequence;
 * an inactive sequence keeps every byte. images: device, sequence s at images + s * image_pitch, rows `stride` bytes apart; Tcw:
 * device float [nseq][16], row-major world -> camera. A NULL image or pose, stride < width or image_pitch < stride * height is TB_EINVAL.
 * tb_depth_filter_add_keyframe_dev: keys_xy device float [nseq][key_pitch][2] (level-0 pixels), counts device int32 [nseq] (clamped
 * to 0..key_pitch), skip nullable device bytes [nseq][key_pitch] (non-zero: the key is not offered), not_added nullable device
 * int32 [nseq] (written for the active sequences).
 * tb_depth_filter_update_dev: one launch of k_df_update per run of consecutive active sequences -- one launch when all are active
 * -- and nothing else: no host synchronisation, no copy.
 * tb_depth_filter_points_dev: points device float [nseq][pitch][3] (zero where flags is 0), flags device bytes [nseq][pitch]: 1 where
 * the entry is converged; release != 0 makes those entries free.
 * tb_depth_filter_state_dev lends the device pointers (each output nullable): seeds / traces [nseq][pitch], slot_Tcw
 * [nseq][ref_slots][16]; newest_slot: HOST int32 [nseq], filled with the slot of each sequence's last keyframe (-1: none yet). */
typedef struct tb_depth_filter tb_depth_filter;
typedef struct tb_depth_filter_params {
    double depth_mean;   /* 15 */
    double depth_min;    /* 2 */
    double conv_div;     /* 200 */
    double px_noise;     /* 1 */
    int max_steps;       /* 1000 */
    int zmssd_max;       /* 2000 */
    int align_iters;     /* 10 */
    int reserved;
} tb_depth_filter_params;
int tb_depth_filter_create(tb_ctx* ctx, int nseq, int pitch, int ref_slots, int width, int height, const double K[4],
                           const tb_depth_filter_params* params, tb_depth_filter** out);
void tb_depth_filter_destroy(tb_depth_filter* df);
int tb_depth_filter_clear(tb_depth_filter* df, const uint8_t* which);
int tb_depth_filter_add_keyframe_dev(tb_depth_filter* df, const uint8_t* images, int stride, size_t image_pitch, const float* Tcw,
                                     const float* keys_xy, const int32_t* counts, int key_pitch, const uint8_t* skip,
                                     const uint8_t* active, int32_t* not_added);
int tb_depth_filter_update_dev(tb_depth_filter* df, const uint8_t* images, int stride, size_t image_pitch, const float* Tcw,
                               const uint8_t* active);
int tb_depth_filter_points_dev(tb_depth_filter* df, float* points, uint8_t* flags, int release);
int tb_depth_filter_state_dev(tb_depth_filter* df, const tb_df_seed** seeds, const tb_df_trace** traces, const float** slot_Tcw,
                              int32_t* newest_slot);

/* ---- multi-GPU batch entry (SURVEY.md section 8(b) `tb_batch_run`, 8(e): frames are independent units through
 * extract -> left/right match, sharded as contiguous blocks of frames, one exchange step at the end).
 * The in-process counterpart of trackingbench_slam_amd/dist.py for a C++ host that holds one context per GPU:
 * frame f of the batch goes to context f * ngpu / nframes; every context's chain -- Frame::ComputePyramid (Frame.cpp:414-427),
 * ORBExtractor::operator() (ORBextractor.cpp:906-978) on the left and the right image, Matcher::searchByBF left <-> right
 * (matcher.cpp:168-228) -- is queued on its own stream before any context is waited for, so the GPUs work concurrently; then
 * the per-frame track records are gathered into the caller's HOST arrays (no collective: the records of a shard come straight
 * from its GPU).  ctxs may name the same device more than once (the shards then share it).
 *   left, right   host frames [nframes][height][stride] (pitch bytes apart)
 *   kps / desc    [2][nframes][cap] records / [2][nframes][cap][32] bytes: side 0 = left, 1 = right
 *   counts        [2][nframes]; matches [nframes][cap] (queryIdx = left key, trainIdx = right key), match_counts [nframes]
 * cap must hold every frame's keypoints and matches (TB_ECAPACITY otherwise). */
typedef struct tb_batch_params {
    int width, height, nlevels;
    float scale;                /* Frame::Frame scale step (0.8) */
    int target;                 /* keypoints per image */
    float init_th, min_th;      /* FAST thresholds */
    float bf_ratio, bf_min_th;  /* searchByBF */
} tb_batch_params;
int tb_batch_run(tb_ctx** ctxs, int ngpu, const tb_batch_params* p, int nframes, const uint8_t* left, const uint8_t* right,
                 int stride, size_t pitch, int cap, tb_keypoint* kps, uint8_t* desc, int32_t* counts, tb_match* matches,
                 int32_t* match_counts);

#ifdef __cplusplus
}
#endif
#endif /* TB_CAPI_H */
