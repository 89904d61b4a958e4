/* Host side of libtb_hip.so: the C ABI of include/tb_capi.h on top of the HIP kernels (k_*.hip).
 * No CPU compute fallback lives here: every operator either runs its kernels or returns an error.
 * Host work is limited to set-up arithmetic the reference also does on the host (scale vectors, level
 * sizes, quotas, resize coefficient tables, cell tables) and data movement: a single-frame (host) form stages its inputs
 * and runs the batched kernels on one pair. The device-resident VO loop that chains these operators (tb_vo_*) is tb_vo.cpp.
 */
#include "tb_internal.h"
#include "tb_math.h"

#include <stdarg.h>
#include <string.h>
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <functional>
#include <memory>
#include <mutex>

/* ------------------------------------------------------------------ errors / context */
int tb_fail(tb_ctx* ctx, int code, const char* fmt, ...) {
    char buf[512]; /* no device binding here: formatting a message needs none, and TB_ENTER reports its own failure */
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    return code;
}

int tb_scratch(tb_ctx* ctx, int slot, size_t bytes, void** out) { /* only called from entry points that have entered */
    if (bytes < 256) bytes = 256;
    if (ctx->scratch_cap[slot] < bytes) {
        if (ctx->scratch[slot]) {
            TB_HIP(ctx, hipStreamSynchronize(ctx->stream));
            TB_HIP(ctx, hipFree(ctx->scratch[slot]));
            ctx->scratch[slot] = nullptr;
            ctx->scratch_cap[slot] = 0;
        }
        const size_t cap = bytes + bytes / 4;
        TB_HIP(ctx, hipMalloc(&ctx->scratch[slot], cap));
        ctx->scratch_cap[slot] = cap;
    }
    *out = ctx->scratch[slot];
    return TB_OK;
}

/* The library's only write of a kernel's dynamic-LDS limit. The limit belongs to the (function, device) pair and is
 * process-wide, while the size a call needs depends on its shapes: a call that wrote its own size would lower the limit
 * under another context's launch on another host thread, or under a captured graph's later replays. So the limit only ever
 * rises: the largest value set so far is kept per (kernel, device) and the runtime is called only for a larger one. The
 * mutex guards the table; it does not close the window between one thread's set and another thread's launch -- that the
 * value is never lowered does, every launch finds at least what its own call asked for. Requests within the 64 KB every
 * kernel has by default need no call. */
int tb_lds_limit(tb_ctx* ctx, const void* kernel, size_t bytes) {
    if (bytes <= 64 * 1024) return TB_OK;
    static std::mutex lock;
    static std::map<std::pair<const void*, int>, size_t> limits;
    std::lock_guard<std::mutex> guard(lock);
    size_t& limit = limits[std::make_pair(kernel, ctx->device)];
    if (bytes > limit) {
        TB_HIP(ctx, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        limit = bytes;
    }
    return TB_OK;
}

static hipEvent_t prof_event(tb_ctx* ctx) {
    if (!ctx->prof_pool.empty()) { hipEvent_t e = ctx->prof_pool.back(); ctx->prof_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    hipEventCreate(&e);
    return e;
}
void tb_prof_begin(tb_ctx* ctx, const char* name) {
    ctx->prof_open = false;
    if (!ctx->prof) return;
    if (!ctx->prof_only.empty() && ctx->prof_only != name) return;
    ctx->prof_open = true;
    tb_ctx::ProfRec r;
    r.name = name;
    r.a = prof_event(ctx);
    r.b = prof_event(ctx);
    hipEventRecord(r.a, ctx->stream);
    ctx->prof_recs.push_back(r);
}
void tb_prof_end(tb_ctx* ctx) {
    if (!ctx->prof || !ctx->prof_open || ctx->prof_recs.empty()) return;
    hipEventRecord(ctx->prof_recs.back().b, ctx->stream);
    ctx->prof_open = false;
}
static void prof_drain(tb_ctx* ctx) {
    hipStreamSynchronize(ctx->stream);
    for (auto& r : ctx->prof_recs) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            auto& acc = ctx->prof_acc[r.name];
            acc.first += 1;
            acc.second += ms;
        }
        ctx->prof_pool.push_back(r.a);
        ctx->prof_pool.push_back(r.b);
    }
    ctx->prof_recs.clear();
}

extern "C" {

int tb_profile_enable(tb_ctx* ctx, int on) {
    TB_ENTER(ctx);
    if (!ctx) return TB_EINVAL;
    prof_drain(ctx);
    ctx->prof_acc.clear();
    ctx->prof = on != 0;
    return TB_OK;
}

int tb_profile_only(tb_ctx* ctx, const char* kernel) {
    TB_ENTER(ctx);
    if (!ctx) return TB_EINVAL;
    ctx->prof_only = kernel ? kernel : "";
    return TB_OK;
}

int tb_profile_report(tb_ctx* ctx, char* buf, int cap) {
    TB_ENTER(ctx);
    if (!ctx || !buf || cap < 1) return TB_EINVAL;
    prof_drain(ctx);
    std::string out;
    char line[256];
    for (auto& kv : ctx->prof_acc) {
        snprintf(line, sizeof line, "%s %ld %.6f\n", kv.first.c_str(), kv.second.first, kv.second.second);
        out += line;
    }
    if ((int)out.size() + 1 > cap) return tb_fail(ctx, TB_ECAPACITY, "profile report needs %d bytes", (int)out.size() + 1);
    memcpy(buf, out.c_str(), out.size() + 1);
    return TB_OK;
}

const char* tb_version(void) { return "trackingbench-slam_amd 0.1 (gfx950)"; }

const char* tb_strerror(int code) {
    switch (code) {
        case TB_OK: return "ok";
        case TB_EINVAL: return "invalid argument";
        case TB_ENOMEM: return "out of memory";
        case TB_ECAPACITY: return "output capacity too small";
        case TB_EUNSUPPORTED: return "unsupported input (reference behaviour undefined)";
        case TB_EDEVICE: return "HIP device error";
        case TB_ESTATE: return "call sequence error";
        default: return "unknown error";
    }
}

int tb_create(int device, tb_ctx** out) {
    if (!out) return TB_EINVAL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return TB_EDEVICE; /* no GPU: fail loudly */
    if (device < 0 || device >= ndev) return TB_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return TB_EDEVICE;
    tb_ctx* ctx = new (std::nothrow) tb_ctx();
    if (!ctx) return TB_ENOMEM;
    ctx->device = device;
    {
        int ncu = 0;
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && ncu > 0) ctx->num_cu = ncu;
    }
    if (hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return TB_EDEVICE;
    }
    ctx->stream = ctx->own_stream;
    *out = ctx;
    return TB_OK;
}

int tb_measure_copy_seconds(tb_ctx* ctx, const void* d_src, void* d_dst, size_t bytes, int reps, double* seconds) {
    TB_ENTER(ctx);
    if (!ctx || !d_src || !d_dst || !seconds || reps < 1 || bytes < 16 || (bytes & 15) || ((uintptr_t)d_src & 15) || ((uintptr_t)d_dst & 15))
        return TB_EINVAL;
    hipEvent_t e0, e1;
    TB_HIP(ctx, hipEventCreate(&e0));
    TB_HIP(ctx, hipEventCreate(&e1));
    int rc = tbk_copy16(ctx, d_src, d_dst, bytes);
    if (rc == TB_OK) {
        hipError_t e = hipEventRecord(e0, ctx->stream);
        for (int i = 0; i < reps && rc == TB_OK; i++) rc = tbk_copy16(ctx, d_src, d_dst, bytes);
        if (e == hipSuccess) e = hipEventRecord(e1, ctx->stream);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        float ms = 0;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        if (e != hipSuccess && rc == TB_OK) rc = tb_fail(ctx, TB_EDEVICE, "tb_measure_copy_seconds: %s", hipGetErrorString(e));
        *seconds = (double)ms * 1e-3 / reps;
    }
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    return rc;
}

int tb_pack_rows_dev(tb_ctx* ctx, const void* src, int row_bytes, int cap, const int32_t* counts, int nframes, void* dst, long long* total) {
    TB_ENTER(ctx);
    if (!ctx || nframes < 0 || cap < 1 || row_bytes < 4 || (row_bytes & 3)) return TB_EINVAL;
    if (nframes == 0) return TB_OK;
    if (!src || !dst || !counts || src == dst) return TB_EINVAL;
    return tbk_pack_rows(ctx, src, row_bytes, cap, counts, nframes, dst, total);
}

int tb_set_concurrency(tb_ctx* ctx, int peers) {
    if (!ctx || peers < 1) return TB_EINVAL;
    ctx->peers = peers;
    return TB_OK;
}

int tb_debug_force_dense_fast(tb_ctx* ctx, int on) {
    if (!ctx) return TB_EINVAL;
    ctx->dbg_fast_dense = on ? 1 : 0;
    return TB_OK;
}

int tb_debug_ba_plain_obs(tb_ctx* ctx, int on) {
    if (!ctx) return TB_EINVAL;
    ctx->dbg_ba_plain_obs = on ? 1 : 0;
    return TB_OK;
}

int tb_debug_bf_scalar(tb_ctx* ctx, int on) {
    if (!ctx) return TB_EINVAL;
    ctx->dbg_bf_scalar = on ? 1 : 0;
    return TB_OK;
}

void tb_destroy(tb_ctx* ctx) {
    if (!ctx) return;
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    ctx->plans.clear();
    while (!ctx->live.empty()) tb_extractor_destroy(*ctx->live.begin()); /* plans never outlive their context */
    for (int i = 0; i < TB_NSLOTS; i++)
        if (ctx->scratch[i]) hipFree(ctx->scratch[i]);
    for (auto& g : ctx->ba_graphs) hipGraphExecDestroy(g.second);
    prof_drain(ctx);
    for (hipEvent_t e : ctx->prof_pool) hipEventDestroy(e);
    if (ctx->own_stream) hipStreamDestroy(ctx->own_stream);
    delete ctx;
}

const char* tb_last_error(const tb_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int tb_set_stream(tb_ctx* ctx, void* hip_stream) {
    TB_ENTER(ctx);
    if (!ctx) return TB_EINVAL;
    TB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    return TB_OK;
}

int tb_synchronize(tb_ctx* ctx) {
    TB_ENTER(ctx);
    if (!ctx) return TB_EINVAL;
    TB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return TB_OK;
}

/* ------------------------------------------------------------------ a1 / a2 / a3 host arithmetic */
int tb_scale_factors(int n, float scale, float* sf, float* inv_sf, float* sigma2, float* inv_sigma2) {
    /* Frame::Frame, Frame.cpp:18-29 (float32 throughout) */
    if (n < 1 || !sf) return TB_EINVAL;
    float cur = 1.f, icur = 1.f;
    for (int i = 0; i < n; i++) {
        if (i > 0) { cur = cur * scale; icur = icur / scale; }
        sf[i] = cur;
        if (inv_sf) inv_sf[i] = icur;
        const float s2 = (i == 0) ? 1.f : cur * cur;
        if (sigma2) sigma2[i] = s2;
        if (inv_sigma2) inv_sigma2[i] = (i == 0) ? 1.f : 1.f / s2;
    }
    return TB_OK;
}

int tb_pyramid_sizes(int width, int height, int nlevels, const float* sf, int* widths, int* heights) {
    /* Frame::ComputePyramid, Frame.cpp:423-424: cv::Size(cols * scale, rows * scale) truncates */
    if (nlevels < 1 || !sf || !widths || !heights) return TB_EINVAL;
    widths[0] = width;
    heights[0] = height;
    for (int i = 1; i < nlevels; i++) {
        widths[i] = (int)((float)width * sf[i]);
        heights[i] = (int)((float)height * sf[i]);
    }
    return TB_OK;
}

int tb_orb_quotas(int nlevels, const float* sf, int target, int* quotas) {
    /* ORBExtractor::operator(), ORBextractor.cpp:919-930; reads sf[1], so one level is undefined there */
    if (nlevels < 2 || !sf || !quotas) return TB_EINVAL;
    float nDesired = target * (1 - sf[1]) / (1 - (float)pow((double)sf[1], (double)nlevels));
    int sum = 0;
    for (int level = 0; level < nlevels - 1; level++) {
        quotas[level] = tbm::cv_round(nDesired);
        sum += quotas[level];
        nDesired *= sf[1];
    }
    quotas[nlevels - 1] = std::max(target - sum, 0);
    return TB_OK;
}

/* ------------------------------------------------------------------ extractor plan */
static void build_resize_tables(int sw, int sh, int dw, int dh, std::vector<ResizeX>& rx, std::vector<ResizeY>& ry) {
    /* cv::resize INTER_LINEAR 8U coefficient set-up (OpenCV 3.3) */
    const double inv_scale_x = (double)dw / sw, inv_scale_y = (double)dh / sh;
    const double scale_x = 1. / inv_scale_x, scale_y = 1. / inv_scale_y;
    rx.resize(dw);
    ry.resize(dh);
    for (int dx = 0; dx < dw; dx++) {
        float fx = (float)((dx + 0.5) * scale_x - 0.5);
        int sx = tbm::cv_floor(fx);
        fx -= sx;
        if (sx < 0) { fx = 0; sx = 0; }
        if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
        rx[dx].sx = (int16_t)sx;
        rx[dx].sx1 = (int16_t)std::min(sx + 1, sw - 1);
        rx[dx].a0 = (int16_t)tbm::cv_round((1.f - fx) * 2048.f);
        rx[dx].a1 = (int16_t)tbm::cv_round(fx * 2048.f);
    }
    for (int dy = 0; dy < dh; dy++) {
        float fy = (float)((dy + 0.5) * scale_y - 0.5);
        int sy = tbm::cv_floor(fy);
        fy -= sy;
        ry[dy].sy0 = std::min(std::max(sy, 0), sh - 1);
        ry[dy].sy1 = std::min(std::max(sy + 1, 0), sh - 1);
        ry[dy].b0 = (int16_t)tbm::cv_round((1.f - fy) * 2048.f);
        ry[dy].b1 = (int16_t)tbm::cv_round(fy * 2048.f);
    }
}

static int fastgrid_ncell(int width, int height, int target) {
    const int cell = (int)sqrtf((float)width * (float)height / (float)target);
    if (cell < 1) return 0;
    const int cols = (int)((float)width / (float)cell), rows = (int)((float)height / (float)cell);
    return std::max((rows + 2) * (cols + 1), target);
}

void tb_extractor_destroy(tb_extractor* ex) {
    if (!ex) return;
    ex->ctx->live.erase(ex);
    for (auto it = ex->ctx->plans.begin(); it != ex->ctx->plans.end();)
        it = (it->second == ex) ? ex->ctx->plans.erase(it) : std::next(it);
    hipSetDevice(ex->ctx->device);
    hipStreamSynchronize(ex->ctx->stream);
    hipFree(ex->d_slab); hipFree(ex->d_img0_copy); hipFree(ex->d_blocks);
    for (int l = 0; l < TB_MAX_LEVELS; l++) { hipFree(ex->d_rx[l]); hipFree(ex->d_ry[l]); }
    hipFree(ex->d_cand); hipFree(ex->d_candCount); hipFree(ex->d_knode); hipFree(ex->d_sel); hipFree(ex->d_selCount);
    hipFree(ex->d_kps); hipFree(ex->d_desc); hipFree(ex->d_counts); hipFree(ex->d_exit); hipFree(ex->d_enode);
    hipFree(ex->d_gridBest); hipFree(ex->d_occ);
    delete ex;
}

int tb_extractor_create(tb_ctx* ctx, int width, int height, int nlevels, const float* sf, const int* widths,
                        const int* heights, int max_images, int max_target, tb_extractor** out) {
    TB_ENTER(ctx);
    if (!ctx || !out) return TB_EINVAL;
    *out = nullptr;
    if (width < 1 || height < 1 || nlevels < 1 || nlevels > TB_MAX_LEVELS || !sf || max_images < 1 || max_target < 1)
        return tb_fail(ctx, TB_EINVAL, "extractor_create: bad geometry %dx%d levels=%d images=%d target=%d", width, height,
                       nlevels, max_images, max_target);
    if (width > 4095 || height > 4095) return tb_fail(ctx, TB_EUNSUPPORTED, "images larger than 4095 px are not supported");
    TB_HIP(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<tb_extractor> exu(new tb_extractor());
    tb_extractor* ex = exu.get();
    ex->ctx = ctx;
    ex->max_images = max_images;
    ex->max_target = max_target;
    ex->sf.assign(sf, sf + nlevels);
    for (int l = 0; l < TB_MAX_LEVELS; l++) { ex->d_rx[l] = nullptr; ex->d_ry[l] = nullptr; ex->quotas[l] = 0; }
    PlanGeom& g = ex->g;
    memset(&g, 0, sizeof g);
    g.nlevels = nlevels;
    g.width = width;
    g.height = height;
    std::vector<int> ws(nlevels), hs(nlevels);
    if (widths && heights) {
        for (int l = 0; l < nlevels; l++) { ws[l] = widths[l]; hs[l] = heights[l]; }
        if (ws[0] != width || hs[0] != height) return tb_fail(ctx, TB_EINVAL, "level 0 size mismatch");
    } else {
        tb_pyramid_sizes(width, height, nlevels, sf, ws.data(), hs.data());
    }
    int maxq[TB_MAX_LEVELS] = {0};
    if (nlevels >= 2) tb_orb_quotas(nlevels, sf, max_target, maxq);
    std::vector<FastBlock> blocks;
    size_t off = 0, candOff = 0;
    int selBase = 0;
    for (int l = 0; l < nlevels; l++) {
        LevelGeom& L = g.lv[l];
        if (ws[l] < 1 || hs[l] < 1 || ws[l] > 4095 || hs[l] > 4095)
            return tb_fail(ctx, TB_EINVAL, "level %d has size %dx%d", l, ws[l], hs[l]);
        L.w = ws[l];
        L.h = hs[l];
        L.stride = (L.w + 63) & ~63;
        L.off = off;
        off += ((size_t)L.stride * L.h + 255) & ~(size_t)255;
        L.sf = sf[l];
        L.inv_sf = 1.f;
        L.patchSize = (float)(int)(31 * sf[l]);
        /* ComputeKeyPointsOctTree grid, ORBextractor.cpp:749-763 */
        const int minB = TB_BORDER, maxBX = L.w - TB_BORDER, maxBY = L.h - TB_BORDER;
        const float fw = (float)(maxBX - minB), fh = (float)(maxBY - minB);
        L.nCols = (int)(fw / 30.f);
        L.nRows = (int)(fh / 30.f);
        L.cellBase = 0;
        L.nCells = 0;
        L.nIni = 0;
        L.hX = 1.f;
        L.wCell = L.hCell = 1;
        if (L.nCols >= 1 && L.nRows >= 1) {
            L.wCell = (int)ceilf(fw / (float)L.nCols);
            L.hCell = (int)ceilf(fh / (float)L.nRows);
            /* The reference walks the cells one by one (ORBextractor.cpp:765-786) and skips those that start at or
             * behind maxBorder - 3 (rows) / maxBorder - 6 (columns); what it does not skip but leaves without a scanned
             * pixel (an ROI under 7 px) yields nothing either. The cells that DO scan are a prefix in both directions,
             * and their scan regions tile [minB + 3, maxB - 3): count them, then cut the grid into blocks. */
            int nRowsEff = 0, nColsEff = 0;
            for (int i = 0; i < L.nRows; i++) {
                const float iniY = (float)minB + (float)i * (float)L.hCell;
                if (iniY >= (float)maxBY - 3.f) continue;
                if ((int)iniY + 3 < maxBY - 3) nRowsEff = i + 1;
            }
            for (int j = 0; j < L.nCols; j++) {
                const float iniX = minB + (float)(j * L.wCell);
                if (iniX >= (float)maxBX - 6.f) continue;
                if ((int)iniX + 3 < maxBX - 3) nColsEff = j + 1;
            }
            if (L.wCell + 6 + 15 > FB_S || L.hCell + 6 > FB_TH)
                return tb_fail(ctx, TB_EUNSUPPORTED, "level %d: FAST cell %dx%d exceeds the LDS tile", l, L.wCell, L.hCell);
            int bx = (FB_S - 6 - 15) / L.wCell, by = (FB_TH - 6) / L.hCell;
            bx = std::min(std::max(bx, 1), FB_MAX_CX);
            by = std::min(std::max(by, 1), FB_MAX_CY);
            for (int i0 = 0; i0 < nRowsEff; i0 += by)
                for (int j0 = 0; j0 < nColsEff; j0 += bx) {
                    FastBlock b;
                    b.level = (int16_t)l;
                    b.ncx = (int16_t)std::min(bx, nColsEff - j0);
                    b.ncy = (int16_t)std::min(by, nRowsEff - i0);
                    b.x0 = (int16_t)(minB + j0 * L.wCell);
                    b.y0 = (int16_t)(minB + i0 * L.hCell);
                    b.x1 = (int16_t)std::min(minB + (j0 + b.ncx) * L.wCell + 6, maxBX);
                    b.y1 = (int16_t)std::min(minB + (i0 + b.ncy) * L.hCell + 6, maxBY);
                    {   /* stage-1 lane map: the tile's column 0 is image column x0 & ~15 */
                        const int cx0 = b.x0 & 15, rw = b.x1 - b.x0, rh = b.y1 - b.y0;
                        const int scanX0 = cx0 + 3, scanX1 = cx0 + rw - 3;
                        b.sA = (int16_t)(scanX0 >> 4);
                        b.nss = (int16_t)(((scanX1 - 1) >> 4) - b.sA + 1);
                        b.rowsPer = (int16_t)(64 / b.nss);
                        b.nPass = (int16_t)((rh - 6 + b.rowsPer - 1) / b.rowsPer);
                        b.invNss = (uint16_t)((32768 + b.nss - 1) / b.nss);
                    }
                    blocks.push_back(b);
                }
            L.nCells = nRowsEff * nColsEff;
            /* DistributeOctTree, ORBextractor.cpp:498-500 (nIni < 1 clamped, see k_octree.hip) */
            int nIni = (int)roundf((float)(maxBX - minB) / (maxBY - minB));
            if (nIni < 1) nIni = 1;
            L.nIni = nIni;
            L.hX = (float)(maxBX - minB) / nIni;
        }
        L.candCap = ((L.w + 1) / 2) * ((L.h + 1) / 2) + 64;
        L.candOff = candOff;
        candOff += (size_t)L.candCap;
        L.quota = maxq[l];
        L.nodeCapAlloc = (L.nCells > 0) ? maxq[l] + 3 + 4 * L.nIni + 8 : 0;
        L.nodeCap = L.nodeCapAlloc;
        L.selBase = selBase;
        selBase += L.nodeCapAlloc;
    }
    g.slabBytes = off;
    g.candPerImage = candOff;
    g.selCap = std::max(std::max(selBase, fastgrid_ncell(width, height, max_target)), 64);
    ex->nBlocksTotal = (int)blocks.size();

    const size_t B = (size_t)max_images;
    TB_HIP(ctx, hipMalloc(&ex->d_slab, B * g.slabBytes));
    TB_HIP(ctx, hipMemsetAsync(ex->d_slab, 0, B * g.slabBytes, ctx->stream));
    if (!blocks.empty()) {
        TB_HIP(ctx, hipMalloc(&ex->d_blocks, blocks.size() * sizeof(FastBlock)));
        TB_HIP(ctx, hipMemcpy(ex->d_blocks, blocks.data(), blocks.size() * sizeof(FastBlock), hipMemcpyHostToDevice));
    }
    for (int l = 1; l < nlevels; l++) {
        std::vector<ResizeX> rx;
        std::vector<ResizeY> ry;
        build_resize_tables(ws[l - 1], hs[l - 1], ws[l], hs[l], rx, ry);
        TB_HIP(ctx, hipMalloc(&ex->d_rx[l], rx.size() * sizeof(ResizeX)));
        TB_HIP(ctx, hipMalloc(&ex->d_ry[l], ry.size() * sizeof(ResizeY)));
        TB_HIP(ctx, hipMemcpy(ex->d_rx[l], rx.data(), rx.size() * sizeof(ResizeX), hipMemcpyHostToDevice));
        TB_HIP(ctx, hipMemcpy(ex->d_ry[l], ry.data(), ry.size() * sizeof(ResizeY), hipMemcpyHostToDevice));
    }
    TB_HIP(ctx, hipMalloc(&ex->d_cand, B * g.candPerImage * sizeof(uint32_t)));
    TB_HIP(ctx, hipMalloc(&ex->d_knode, B * g.candPerImage * sizeof(uint32_t)));
    TB_HIP(ctx, hipMalloc(&ex->d_candCount, B * TB_MAX_LEVELS * sizeof(int32_t)));
    TB_HIP(ctx, hipMalloc(&ex->d_selCount, B * TB_MAX_LEVELS * sizeof(int32_t)));
    TB_HIP(ctx, hipMalloc(&ex->d_sel, B * g.selCap * sizeof(uint32_t)));
    TB_HIP(ctx, hipMalloc(&ex->d_kps, B * g.selCap * sizeof(tb_keypoint)));
    TB_HIP(ctx, hipMalloc(&ex->d_desc, B * g.selCap * 32));
    TB_HIP(ctx, hipMalloc(&ex->d_counts, B * sizeof(int32_t)));
    TB_HIP(ctx, hipMalloc(&ex->d_enode, 256));
    TB_HIP(ctx, hipMalloc(&ex->d_exit, 256));
    ex->enodeCap = 64;
    ex->exitCap = 32;
    TB_HIP(ctx, hipMemsetAsync(ex->d_counts, 0, B * sizeof(int32_t), ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(ex->d_selCount, 0, B * TB_MAX_LEVELS * sizeof(int32_t), ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(ex->d_candCount, 0, B * TB_MAX_LEVELS * sizeof(int32_t), ctx->stream));
    /* level 0 defaults to the slab until frames are attached */
    g.img0 = nullptr;
    g.img0_pitch = 0;
    g.img0_stride = 0;
    ctx->live.insert(ex);
    *out = exu.release();
    return TB_OK;
}

int tb_extractor_set_images_host(tb_extractor* ex, const uint8_t* images, int n, int stride, size_t pitch) {
    TB_ENTER((ex ? ex->ctx : nullptr));
    if (!ex || !images || n < 1 || n > ex->max_images || stride < ex->g.width) return TB_EINVAL;
    tb_ctx* ctx = ex->ctx;
    const LevelGeom& L0 = ex->g.lv[0];
    for (int b = 0; b < n; b++)
        TB_HIP(ctx, hipMemcpy2DAsync(ex->d_slab + (size_t)b * ex->g.slabBytes + L0.off, L0.stride, images + (size_t)b * pitch,
                                     stride, L0.w, L0.h, hipMemcpyHostToDevice, ctx->stream));
    ex->g.img0 = nullptr; /* level 0 lives in the slab */
    return TB_OK;
}

int tb_extractor_set_images_dev(tb_extractor* ex, const uint8_t* dev_images, int n, int stride, size_t pitch) {
    TB_ENTER((ex ? ex->ctx : nullptr));
    if (!ex || !dev_images || n < 1 || n > ex->max_images || stride < ex->g.width) return TB_EINVAL;
    ex->g.img0 = dev_images;
    ex->g.img0_stride = stride;
    ex->g.img0_pitch = pitch;
    return TB_OK;
}

int tb_extractor_set_levels_host(tb_extractor* ex, int index, const uint8_t* const* levels, const int* strides) {
    TB_ENTER((ex ? ex->ctx : nullptr));
    if (!ex || !levels || !strides || index < 0 || index >= ex->max_images) return TB_EINVAL;
    tb_ctx* ctx = ex->ctx;
    for (int l = 0; l < ex->g.nlevels; l++) {
        const LevelGeom& L = ex->g.lv[l];
        if (!levels[l] || strides[l] < L.w) return tb_fail(ctx, TB_EINVAL, "set_levels_host: level %d missing", l);
        TB_HIP(ctx, hipMemcpy2DAsync(ex->d_slab + (size_t)index * ex->g.slabBytes + L.off, L.stride, levels[l], strides[l], L.w,
                                     L.h, hipMemcpyHostToDevice, ctx->stream));
    }
    ex->g.img0 = nullptr;
    return TB_OK;
}

int tb_extractor_build_pyramid(tb_extractor* ex, int n) {
    TB_ENTER((ex ? ex->ctx : nullptr));
    if (!ex || n < 1 || n > ex->max_images) return TB_EINVAL;
    for (int l = 1; l < ex->g.nlevels; l++) {
        int rc = tbk_resize_level(ex, l, n);
        if (rc) return rc;
    }
    return TB_OK;
}

int tb_extractor_get_level_host(tb_extractor* ex, int index, int level, uint8_t* out, int out_stride) {
    TB_ENTER((ex ? ex->ctx : nullptr));
    if (!ex || !out || index < 0 || index >= ex->max_images || level < 0 || level >= ex->g.nlevels) return TB_EINVAL;
    tb_ctx* ctx = ex->ctx;
    const LevelGeom& L = ex->g.lv[level];
    if (out_stride < L.w) return TB_EINVAL;
    const uint8_t* src;
    size_t sp;
    if (level == 0 && ex->g.img0) { src = ex->g.img0 + (size_t)index * ex->g.img0_pitch; sp = ex->g.img0_stride; }
    else { src = ex->d_slab + (size_t)index * ex->g.slabBytes + L.off; sp = L.stride; }
    TB_HIP(ctx, hipMemcpy2DAsync(out, out_stride, src, sp, L.w, L.h, hipMemcpyDeviceToHost, ctx->stream));
    TB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return TB_OK;
}

int tb_extractor_orb(tb_extractor* ex, int n, int target, float init_th, float min_th, int quota_mode,
                     const tb_keypoint* exit_keys, int n_exit) {
    TB_ENTER((ex ? ex->ctx : nullptr));
    if (!ex || n < 1 || n > ex->max_images || target < 0 || n_exit < 0 || (n_exit > 0 && !exit_keys)) return TB_EINVAL;
    tb_ctx* ctx = ex->ctx;
    PlanGeom& g = ex->g;
    if (quota_mode == 0) {
        if (g.nlevels < 2) return tb_fail(ctx, TB_EUNSUPPORTED, "ORB extraction reads sf[1]: needs >= 2 levels");
        if (target > ex->max_target) return tb_fail(ctx, TB_ECAPACITY, "target %d exceeds plan max_target %d", target, ex->max_target);
        tb_orb_quotas(g.nlevels, ex->sf.data(), target, ex->quotas);
        ex->have_quotas = true;
    } else if (!ex->have_quotas) {
        /* AddPoints before operator(): the reference indexes an empty mnFeaturesPerLevel (ORBextractor.cpp:810) */
        return tb_fail(ctx, TB_ESTATE, "AddPoints-mode extraction before any operator()-mode call");
    }
    for (int l = 0; l < g.nlevels; l++) {
        LevelGeom& L = g.lv[l];
        L.quota = ex->quotas[l];
        L.nodeCap = (L.nCells > 0) ? L.quota + 3 + 4 * L.nIni : 0;
        if (L.nodeCap > L.nodeCapAlloc) return tb_fail(ctx, TB_ECAPACITY, "level %d quota %d exceeds the plan", l, L.quota);
    }
    /* cv::FAST clamps its threshold to [0,255]; (int) truncation as at ORBextractor.cpp:786,791 */
    const int ith = std::min(std::max((int)init_th, 0), 255), mth = std::min(std::max((int)min_th, 0), 255);
    if (n_exit > 0) {
        if (n_exit > ex->exitCap) {
            TB_HIP(ctx, hipStreamSynchronize(ctx->stream));
            hipFree(ex->d_exit);
            ex->d_exit = nullptr;
            TB_HIP(ctx, hipMalloc(&ex->d_exit, (size_t)n_exit * 2 * sizeof(float)));
            ex->exitCap = n_exit;
        }
        const size_t need = (size_t)n * g.nlevels * n_exit;
        if (need > ex->enodeCap) {
            TB_HIP(ctx, hipStreamSynchronize(ctx->stream));
            hipFree(ex->d_enode);
            ex->d_enode = nullptr;
            TB_HIP(ctx, hipMalloc(&ex->d_enode, need * sizeof(int32_t)));
            ex->enodeCap = need;
        }
        std::vector<float> xy((size_t)n_exit * 2);
        for (int i = 0; i < n_exit; i++) { xy[2 * i] = exit_keys[i].x; xy[2 * i + 1] = exit_keys[i].y; }
        TB_HIP(ctx, hipMemcpyAsync(ex->d_exit, xy.data(), xy.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        TB_HIP(ctx, hipStreamSynchronize(ctx->stream)); /* xy is a stack-lifetime staging buffer */
    }
    int rc = tbk_fast_cells(ex, n, ith, mth);
    if (rc) return rc;
    rc = tbk_octree(ex, n, n_exit);
    if (rc) return rc;
    rc = tbk_describe(ex, n);
    if (rc) return rc;
    ex->last_n = n;
    ex->last_was_orb = true;
    return TB_OK;
}

int tb_extractor_fastgrid(tb_extractor* ex, int n, const float* inv_sf, int target, float threshold,
                          const uint8_t* occupancy, int n_occupancy) {
    TB_ENTER((ex ? ex->ctx : nullptr));
    if (!ex || n < 1 || n > ex->max_images || !inv_sf || target < 1) return TB_EINVAL;
    tb_ctx* ctx = ex->ctx;
    for (int l = 0; l < ex->g.nlevels; l++) ex->g.lv[l].inv_sf = inv_sf[l];
    int n_occ = 0;
    if (occupancy && n_occupancy > 0) {
        if ((size_t)n_occupancy > ex->occCap) {
            TB_HIP(ctx, hipStreamSynchronize(ctx->stream));
            hipFree(ex->d_occ);
            ex->d_occ = nullptr;
            TB_HIP(ctx, hipMalloc(&ex->d_occ, (size_t)n_occupancy));
            ex->occCap = (size_t)n_occupancy;
        }
        TB_HIP(ctx, hipMemcpyAsync(ex->d_occ, occupancy, (size_t)n_occupancy, hipMemcpyHostToDevice, ctx->stream));
        TB_HIP(ctx, hipStreamSynchronize(ctx->stream));
        n_occ = n_occupancy;
    }
    int rc = tbk_fastgrid(ex, n, target, threshold, n_occ);
    if (rc) return rc;
    ex->last_n = n;
    ex->last_was_orb = false;
    return TB_OK;
}

int tb_extractor_counts_host(tb_extractor* ex, int n, int* counts) {
    TB_ENTER((ex ? ex->ctx : nullptr));
    if (!ex || !counts || n < 1 || n > ex->max_images) return TB_EINVAL;
    tb_ctx* ctx = ex->ctx;
    TB_HIP(ctx, hipMemcpyAsync(counts, ex->d_counts, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    TB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return TB_OK;
}

int tb_extractor_results_host(tb_extractor* ex, int index, tb_keypoint* kps, uint8_t* desc, int cap, int* count) {
    TB_ENTER((ex ? ex->ctx : nullptr));
    if (!ex || !count || index < 0 || index >= ex->max_images) return TB_EINVAL;
    tb_ctx* ctx = ex->ctx;
    int32_t c = 0;
    TB_HIP(ctx, hipMemcpyAsync(&c, ex->d_counts + index, sizeof c, hipMemcpyDeviceToHost, ctx->stream));
    TB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *count = c;
    if (c > cap) return tb_fail(ctx, TB_ECAPACITY, "results: %d keypoints, capacity %d", c, cap);
    if (c > 0 && kps)
        TB_HIP(ctx, hipMemcpyAsync(kps, ex->d_kps + (size_t)index * ex->g.selCap, (size_t)c * sizeof(tb_keypoint),
                                   hipMemcpyDeviceToHost, ctx->stream));
    if (c > 0 && desc && ex->last_was_orb)
        TB_HIP(ctx, hipMemcpyAsync(desc, ex->d_desc + (size_t)index * ex->g.selCap * 32, (size_t)c * 32, hipMemcpyDeviceToHost,
                                   ctx->stream));
    TB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return TB_OK;
}

int tb_extractor_results_dev(tb_extractor* ex, const tb_keypoint** kps, const uint8_t** desc, const int32_t** counts,
                             int* kp_capacity) {
    TB_ENTER((ex ? ex->ctx : nullptr));
    if (!ex) return TB_EINVAL;
    if (kps) *kps = ex->d_kps;
    if (desc) *desc = ex->d_desc;
    if (counts) *counts = ex->d_counts;
    if (kp_capacity) *kp_capacity = ex->g.selCap;
    return TB_OK;
}

__global__ void k_copy_results(const tb_keypoint* __restrict__ skp, const uint8_t* __restrict__ sdesc,
                               const int32_t* __restrict__ scnt, int selCap, tb_keypoint* __restrict__ dkp,
                               uint8_t* __restrict__ ddesc, int32_t* __restrict__ dcnt, int cap) {
    const int b = blockIdx.y;
    const int c = min(scnt[b], cap);
    if (blockIdx.x == 0 && threadIdx.x == 0) dcnt[b] = c;
    /* 60 bytes per keypoint row: 7 dwords of tb_keypoint + 8 dwords of descriptor */
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c * 15) return;
    const int row = i / 15, w = i - row * 15;
    if (w < 7) reinterpret_cast<uint32_t*>(dkp + (size_t)b * cap + row)[w] = reinterpret_cast<const uint32_t*>(skp + (size_t)b * selCap + row)[w];
    else reinterpret_cast<uint32_t*>(ddesc + ((size_t)b * cap + row) * 32)[w - 7] =
             reinterpret_cast<const uint32_t*>(sdesc + ((size_t)b * selCap + row) * 32)[w - 7];
}

int tb_extractor_copy_results_dev(tb_extractor* ex, int n, tb_keypoint* kps, uint8_t* desc, int32_t* counts, int cap) {
    TB_ENTER((ex ? ex->ctx : nullptr));
    if (!ex || n < 1 || n > ex->max_images || !kps || !desc || !counts || cap < 1) return TB_EINVAL;
    tb_ctx* ctx = ex->ctx;
    const int rows = std::min(cap, ex->g.selCap);
    return tb_launch(ctx, "k_copy_results", k_copy_results, dim3((rows * 15 + 255) / 256, n), dim3(256), 0, ex->d_kps, ex->d_desc,
                     ex->d_counts, ex->g.selCap, kps, desc, counts, cap);
}

int tb_extractor_candidates_host(tb_extractor* ex, int index, int level, tb_corner* out, int cap, int* count) {
    TB_ENTER((ex ? ex->ctx : nullptr));
    if (!ex || !count || index < 0 || index >= ex->max_images || level < 0 || level >= ex->g.nlevels) return TB_EINVAL;
    tb_ctx* ctx = ex->ctx;
    const LevelGeom& L = ex->g.lv[level];
    int32_t c = 0;
    TB_HIP(ctx, hipMemcpyAsync(&c, ex->d_candCount + index * TB_MAX_LEVELS + level, sizeof c, hipMemcpyDeviceToHost, ctx->stream));
    TB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (c > L.candCap) return tb_fail(ctx, TB_ECAPACITY, "candidate overflow on level %d", level);
    *count = c;
    if (c > cap) return tb_fail(ctx, TB_ECAPACITY, "candidates: %d, capacity %d", c, cap);
    std::vector<uint32_t> rec((size_t)c);
    if (c > 0) {
        TB_HIP(ctx, hipMemcpyAsync(rec.data(), ex->d_cand + (size_t)index * ex->g.candPerImage + L.candOff, (size_t)c * 4,
                                   hipMemcpyDeviceToHost, ctx->stream));
        TB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    /* the kernel emits in arrival order; present them in the reference's order (cell-major raster) */
    std::vector<std::pair<uint64_t, uint32_t>> keyed((size_t)c);
    for (int i = 0; i < c; i++) {
        const int x = rec[i] & 0xfff, y = (rec[i] >> 12) & 0xfff;
        const int ci = (y - 3) / L.hCell, cj = (x - 3) / L.wCell;
        keyed[i] = std::make_pair(((uint64_t)(ci * L.nCols + cj) << 24) | ((uint64_t)y << 12) | (uint64_t)x, rec[i]);
    }
    std::sort(keyed.begin(), keyed.end());
    for (int i = 0; i < c; i++) {
        out[i].x = keyed[i].second & 0xfff;
        out[i].y = (keyed[i].second >> 12) & 0xfff;
        out[i].score = keyed[i].second >> 24;
    }
    return TB_OK;
}

/* ------------------------------------------------------------------ single-frame operator forms
 * A host form stages its inputs and outputs in TB_SLOT_HOST, runs the batched form (or its launcher) on one frame or pair,
 * and copies the results back behind one synchronisation. */
/* the next 16-byte aligned piece of a staging slot: returns its offset and moves `end` past it */
static size_t stage_piece(size_t& end, size_t bytes) {
    const size_t o = end;
    end += (bytes + 15) & ~(size_t)15;
    return o;
}

#define TB_UPLOAD(ctx, dst, src, bytes) \
    do { if (bytes) TB_HIP(ctx, hipMemcpyAsync((dst), (src), (bytes), hipMemcpyHostToDevice, (ctx)->stream)); } while (0)
#define TB_DOWNLOAD(ctx, dst, src, bytes) \
    do { if (bytes) TB_HIP(ctx, hipMemcpyAsync((dst), (src), (bytes), hipMemcpyDeviceToHost, (ctx)->stream)); } while (0)

static int get_plan(tb_ctx* ctx, const char* tag, int nlevels, const float* sf, const int* ws, const int* hs, int max_target,
                    tb_extractor** out) {
    std::string key = tag;
    char buf[64];
    for (int l = 0; l < nlevels; l++) {
        snprintf(buf, sizeof buf, ":%dx%d:%08x", ws[l], hs[l], *reinterpret_cast<const uint32_t*>(&sf[l]));
        key += buf;
    }
    auto it = ctx->plans.find(key);
    if (it != ctx->plans.end() && it->second->max_target >= max_target) { *out = it->second; return TB_OK; }
    if (it != ctx->plans.end()) tb_extractor_destroy(it->second); /* also drops the cache entry */
    tb_extractor* ex = nullptr;
    int rc = tb_extractor_create(ctx, ws[0], hs[0], nlevels, sf, ws, hs, 1, std::max(max_target, 2048), &ex);
    if (rc) return rc;
    ctx->plans[key] = ex;
    *out = ex;
    return TB_OK;
}

int tb_pyramid(tb_ctx* ctx, const uint8_t* image, int width, int height, int stride, int nlevels, const float* sf,
               uint8_t* const* levels_out, const int* strides_out) {
    TB_ENTER(ctx);
    if (!ctx || !image || !sf || !levels_out || !strides_out || nlevels < 1 || nlevels > TB_MAX_LEVELS) return TB_EINVAL;
    std::vector<int> ws(nlevels), hs(nlevels);
    tb_pyramid_sizes(width, height, nlevels, sf, ws.data(), hs.data());
    tb_extractor* ex = nullptr;
    int rc = get_plan(ctx, "pyr", nlevels, sf, ws.data(), hs.data(), 1, &ex);
    if (rc) return rc;
    rc = tb_extractor_set_images_host(ex, image, 1, stride, 0);
    if (rc) return rc;
    rc = tb_extractor_build_pyramid(ex, 1);
    if (rc) return rc;
    for (int l = 1; l < nlevels; l++) {
        if (!levels_out[l]) continue;
        rc = tb_extractor_get_level_host(ex, 0, l, levels_out[l], strides_out[l]);
        if (rc) return rc;
    }
    return tb_synchronize(ctx);
}

int tb_fast_detect(tb_ctx* ctx, const uint8_t* image, int width, int height, int stride, int threshold, int nms,
                   tb_corner* out, int cap, int* count) {
    TB_ENTER(ctx);
    if (!ctx || !image || !count || width < 0 || height < 0 || width > 4095 || height > 4095) return TB_EINVAL;
    *count = 0;
    if (width < 7 || height < 7) return TB_OK;
    threshold = std::min(std::max(threshold, 0), 255);
    const int rcap = (nms ? ((width + 1) / 2) * ((height + 1) / 2) : width * height) + 64;
    size_t end = 0;
    const size_t oImg = stage_piece(end, (size_t)width * height), oOut = stage_piece(end, (size_t)rcap * 4), oCnt = stage_piece(end, 4);
    char* b;
    int rc;
    if ((rc = tb_scratch(ctx, TB_SLOT_HOST, end, (void**)&b))) return rc;
    TB_HIP(ctx, hipMemcpy2DAsync(b + oImg, width, image, stride, width, height, hipMemcpyHostToDevice, ctx->stream));
    rc = tbk_fast_image(ctx, (const uint8_t*)(b + oImg), width, height, width, threshold, nms, 9, (uint32_t*)(b + oOut), rcap,
                        (int32_t*)(b + oCnt));
    if (rc) return rc;
    int32_t c = 0;
    TB_DOWNLOAD(ctx, &c, b + oCnt, 4);
    TB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *count = c;
    if (c > cap || c > rcap) return tb_fail(ctx, TB_ECAPACITY, "fast_detect: %d corners, capacity %d", c, cap);
    std::vector<uint32_t> rec((size_t)c);
    if (c > 0) {
        TB_HIP(ctx, hipMemcpy(rec.data(), b + oOut, (size_t)c * 4, hipMemcpyDeviceToHost));
        /* raster order of cv::FAST: sort by (y, x) */
        std::sort(rec.begin(), rec.end(), [](uint32_t a, uint32_t b) { return (a & 0xffffff) < (b & 0xffffff); });
    }
    for (int i = 0; i < c && out; i++) {
        out[i].x = rec[i] & 0xfff;
        out[i].y = (rec[i] >> 12) & 0xfff;
        out[i].score = rec[i] >> 24;
    }
    return TB_OK;
}

int tb_orb_extract(tb_ctx* ctx, const uint8_t* const* levels, const int* widths, const int* heights, const int* strides,
                   int nlevels, const float* sf, int target, float init_th, float min_th, const tb_keypoint* exit_keys,
                   int n_exit, int use_quotas, int* quotas_inout, tb_keypoint* kps, uint8_t* desc, int cap, int* count) {
    TB_ENTER(ctx);
    if (!ctx || !levels || !widths || !heights || !strides || !sf || !quotas_inout || !count || nlevels < 1 ||
        nlevels > TB_MAX_LEVELS)
        return TB_EINVAL;
    *count = 0;
    if (!levels[0] || widths[0] < 1 || heights[0] < 1) return TB_OK; /* images.at(0).empty(): silent return */
    if (nlevels < 2) return tb_fail(ctx, TB_EUNSUPPORTED, "ORB extraction reads sf[1]: needs >= 2 levels");
    int qsum = 0;
    if (use_quotas) for (int l = 0; l < nlevels; l++) qsum += quotas_inout[l];
    tb_extractor* ex = nullptr;
    int rc = get_plan(ctx, "orb", nlevels, sf, widths, heights, std::max(target, qsum), &ex);
    if (rc) return rc;
    rc = tb_extractor_set_levels_host(ex, 0, levels, strides);
    if (rc) return rc;
    if (use_quotas) {
        for (int l = 0; l < nlevels; l++) ex->quotas[l] = quotas_inout[l];
        ex->have_quotas = true;
    }
    rc = tb_extractor_orb(ex, 1, target, init_th, min_th, use_quotas ? 1 : 0, exit_keys, n_exit);
    if (rc) return rc;
    if (!use_quotas) for (int l = 0; l < nlevels; l++) quotas_inout[l] = ex->quotas[l];
    return tb_extractor_results_host(ex, 0, kps, desc, cap, count);
}

int tb_fastgrid_extract(tb_ctx* ctx, const uint8_t* const* levels, const int* widths, const int* heights, const int* strides,
                        int nlevels, const float* inv_sf, int target, float threshold, const uint8_t* occupancy,
                        int n_occupancy, tb_keypoint* kps, int cap, int* count) {
    TB_ENTER(ctx);
    if (!ctx || !levels || !widths || !heights || !strides || !inv_sf || !count || nlevels < 1 || nlevels > TB_MAX_LEVELS ||
        target < 1)
        return TB_EINVAL;
    *count = 0;
    if (!levels[0] || widths[0] < 1 || heights[0] < 1) return TB_OK;
    std::vector<float> sf(nlevels);
    for (int l = 0; l < nlevels; l++) sf[l] = 1.f / inv_sf[l]; /* plan key + ORB fields only; unused by fastgrid */
    tb_extractor* ex = nullptr;
    int rc = get_plan(ctx, "fg", nlevels, sf.data(), widths, heights, target, &ex);
    if (rc) return rc;
    rc = tb_extractor_set_levels_host(ex, 0, levels, strides);
    if (rc) return rc;
    rc = tb_extractor_fastgrid(ex, 1, inv_sf, target, threshold, occupancy, n_occupancy);
    if (rc) return rc;
    return tb_extractor_results_host(ex, 0, kps, nullptr, cap, count);
}

/* ------------------------------------------------------------------ matchers */
int tb_descriptor_distance(const uint8_t* a, const uint8_t* b) {
    /* Matcher::DescriptorDistance, matcher.cpp:793-808: 256-bit Hamming distance */
    int dist = 0;
    for (int i = 0; i < 4; i++) {
        uint64_t x, y;
        memcpy(&x, a + 8 * i, 8);
        memcpy(&y, b + 8 * i, 8);
        dist += __builtin_popcountll(x ^ y);
    }
    return dist;
}

int tb_ba_obs_stream_positions(const int32_t* pt_start, int npt, int32_t* pos) {
    if (npt < 0 || !pt_start || (!pos && pt_start[npt] > 0)) return TB_EINVAL;
    for (int r0 = 0; r0 < npt; r0 += 64) { /* one 64-point block = one wavefront of the point passes, slot by slot as they walk it */
        int base = pt_start[r0];
        for (int j = 0;; j++) {
            unsigned long long m = 0;
            for (int l = 0; l < 64 && r0 + l < npt; l++)
                if (pt_start[r0 + l + 1] - pt_start[r0 + l] > j) m |= 1ull << l;
            if (m == 0) break;
            int next = base;
            for (int l = 0; l < 64; l++)
                if ((m >> l) & 1) { next = base; pos[pt_start[r0 + l] + j] = tbm::ba_stream_slot(m, l, &next); }
            base = next;
        }
    }
    return TB_OK;
}

void tb_three_maxima(const int* sizes, int L, int* ind1, int* ind2, int* ind3) {
    tbm::three_maxima(sizes, L, ind1, ind2, ind3);   /* the function the matchers' accept stage runs on the device */
}

/* the end of every single-frame matcher: one synchronisation for the device list's count and flag (cf = count, flag), the
 * flag reported as the error the host form returns, then *count, the capacity check and the copy-out */
static int match_tail(tb_ctx* ctx, const tb_match* dout, const int32_t* dcf, int cap, tb_match* out, int* count) {
    int32_t cf[2] = {0, 0};
    TB_HIP(ctx, hipMemcpyAsync(cf, dcf, sizeof cf, hipMemcpyDeviceToHost, ctx->stream));
    TB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (cf[1] == 1) return tb_fail(ctx, TB_EINVAL, "searchByProjection: a key octave is outside the scale factors");
    if (cf[1] == 2) return tb_fail(ctx, TB_EUNSUPPORTED, "rotation bin outside histogram (reference asserts)");
    *count = cf[0];
    if (cf[0] > cap) return tb_fail(ctx, TB_ECAPACITY, "matches: %d, capacity %d", cf[0], cap);
    if (cf[0] > 0 && out) TB_HIP(ctx, hipMemcpy(out, dout, (size_t)cf[0] * sizeof(tb_match), hipMemcpyDeviceToHost));
    return TB_OK;
}

/* the launcher, best rows staged too: tb_search_by_bf_batch_dev fixes crosscheck and filter to searchByBF's */
static int bf_host(tb_ctx* ctx, const uint8_t* d1, int n1, const uint8_t* d2, int n2, int crosscheck, int filter, float ratio,
                   float min_th, tb_match* out, int cap, int* count) {
    if (!ctx || !count || n1 < 0 || n2 < 0 || (n1 && !d1) || (n2 && !d2)) return TB_EINVAL;
    *count = 0;
    if (n1 == 0 || n2 == 0) return TB_OK;
    const int max_n = std::max(n1, n2);
    const size_t pitch = (size_t)max_n * 32;
    size_t end = 0;
    const size_t oD1 = stage_piece(end, pitch), oD2 = stage_piece(end, pitch), oTb = stage_piece(end, (size_t)max_n * 8),
                 oQb = stage_piece(end, (size_t)max_n * 8), oOut = stage_piece(end, (size_t)n1 * sizeof(tb_match)), oCnt = stage_piece(end, 16);
    char* b;
    int rc;
    if ((rc = tb_scratch(ctx, TB_SLOT_HOST, end, (void**)&b))) return rc;
    const int32_t cnt[4] = {n1, n2, 0, 0}; /* n1, n2, then the match count and a flag that stays 0 */
    int32_t* dcnt = (int32_t*)(b + oCnt);
    TB_UPLOAD(ctx, b + oD1, d1, (size_t)n1 * 32);
    TB_UPLOAD(ctx, b + oD2, d2, (size_t)n2 * 32);
    TB_UPLOAD(ctx, dcnt, cnt, sizeof cnt);
    if ((rc = tbk_bf_batch(ctx, 1, (const uint8_t*)(b + oD1), dcnt, (const uint8_t*)(b + oD2), dcnt + 1, pitch, max_n, crosscheck, filter,
                           ratio, min_th, (tb_match*)(b + oOut), n1, dcnt + 2, (unsigned long long*)(b + oTb), (unsigned long long*)(b + oQb))))
        return rc;
    return match_tail(ctx, (const tb_match*)(b + oOut), dcnt + 2, cap, out, count);
}

int tb_match_bf(tb_ctx* ctx, const uint8_t* d1, int n1, const uint8_t* d2, int n2, int crosscheck, tb_match* out, int cap,
                int* count) {
    TB_ENTER(ctx);
    return bf_host(ctx, d1, n1, d2, n2, crosscheck, 0, 0.f, 0.f, out, cap, count);
}

int tb_search_by_bf(tb_ctx* ctx, const uint8_t* d1, int n1, const uint8_t* d2, int n2, float ratio, float min_th,
                    tb_match* out, int cap, int* count) {
    TB_ENTER(ctx);
    return bf_host(ctx, d1, n1, d2, n2, 1, 1, ratio, min_th, out, cap, count);
}

int tb_search_by_bf_batch_dev(tb_ctx* ctx, int npairs, const uint8_t* desc1, const int32_t* counts1, const uint8_t* desc2,
                              const int32_t* counts2, size_t set_pitch, float ratio, float min_th, tb_match* out, int cap,
                              int32_t* out_counts) {
    TB_ENTER(ctx);
    if (!ctx || npairs < 0 || !desc1 || !desc2 || !counts1 || !counts2 || !out || !out_counts || set_pitch < 32 || cap < 1)
        return TB_EINVAL;
    if (npairs == 0) return TB_OK;
    const int max_n = (int)(set_pitch / 32);
    void *tb, *qb;
    int rc;
    if ((rc = tb_scratch(ctx, TB_SLOT_BF_TRAIN, (size_t)npairs * max_n * 8, &tb))) return rc;
    if ((rc = tb_scratch(ctx, TB_SLOT_BF_QUERY, (size_t)npairs * max_n * 8, &qb))) return rc;
    return tbk_bf_batch(ctx, npairs, desc1, counts1, desc2, counts2, set_pitch, max_n, 1, 1, ratio, min_th, out, cap, out_counts,
                        (unsigned long long*)tb, (unsigned long long*)qb);
}

/* ---- Matcher::searchByNN: the LSH matcher (see include/tb_capi.h) */
#define TB_LSH_MAX_N 8192

static bool lsh_params_ok(int tables, int key_size, int probe) {
    return tables >= 1 && tables <= 32 && key_size >= 1 && key_size <= 32 && probe >= 0 && probe <= key_size;
}

int tb_lsh_draw_bits(int tables, int key_size, uint64_t seed, uint16_t* out) {
    if (!out || tables < 1 || tables > 32 || key_size < 1 || key_size > 32) return TB_EINVAL;
    uint16_t pool[256];
    int have = 0, at = 0;   /* entries left in the pool, the first of them */
    uint64_t word = 0;      /* words of the stream read so far */
    for (int t = 0; t < tables; t++) {
        if (have < key_size) {
            for (int i = 0; i < 256; i++) pool[i] = (uint16_t)i;
            for (int i = 255; i >= 1; i--) {
                uint64_t z = seed + (++word) * 0x9E3779B97F4A7C15ull;
                z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
                z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
                z = z ^ (z >> 31);
                const int j = (int)(z % (uint64_t)(i + 1));
                std::swap(pool[i], pool[j]);
            }
            have = 256; at = 0;
        }
        for (int b = 0; b < key_size; b++) out[(size_t)t * key_size + b] = pool[at + b];
        at += key_size; have -= key_size;
    }
    return TB_OK;
}

int tb_lsh_create(tb_ctx* ctx, int tables, int key_size, int multi_probe_level, uint64_t seed, const uint16_t* bits, tb_lsh** out) {
    TB_ENTER(ctx);
    if (out) *out = nullptr;
    if (!ctx || !out) return TB_EINVAL;
    if (!lsh_params_ok(tables, key_size, multi_probe_level))
        return tb_fail(ctx, TB_EINVAL, "tb_lsh_create: tables %d (1..32), key_size %d (1..32), multi_probe_level %d (0..key_size)", tables,
                       key_size, multi_probe_level);
    std::unique_ptr<tb_lsh, void (*)(tb_lsh*)> h(new tb_lsh(), tb_lsh_destroy);
    h->ctx = ctx; h->T = tables; h->k = key_size; h->L = multi_probe_level;
    h->bits.resize((size_t)tables * key_size);
    if (bits) {
        for (int t = 0; t < tables; t++) {
            bool seen[256] = {};
            for (int b = 0; b < key_size; b++) {
                const uint16_t v = bits[(size_t)t * key_size + b];
                if (v > 255 || seen[v]) return tb_fail(ctx, TB_EINVAL, "tb_lsh_create: bit %d of table %d is %d (0..255, once per table)", b, t, (int)v);
                seen[v] = true;
            }
        }
        std::copy(bits, bits + h->bits.size(), h->bits.begin());
    } else {
        tb_lsh_draw_bits(tables, key_size, seed, h->bits.data());
    }
    std::vector<uint8_t> b8(h->bits.begin(), h->bits.end());
    TB_HIP(ctx, hipMalloc((void**)&h->d_bits, b8.size()));
    TB_HIP(ctx, hipMemcpy(h->d_bits, b8.data(), b8.size(), hipMemcpyHostToDevice));
    *out = h.release();
    return TB_OK;
}

void tb_lsh_destroy(tb_lsh* lsh) {
    if (!lsh) return;
    if (lsh->ctx) hipSetDevice(lsh->ctx->device);
    hipFree(lsh->d_bits);
    delete lsh;
}

int tb_lsh_info(const tb_lsh* lsh, int* tables, int* key_size, int* multi_probe_level, uint16_t* bits) {
    if (!lsh) return TB_EINVAL;
    if (tables) *tables = lsh->T;
    if (key_size) *key_size = lsh->k;
    if (multi_probe_level) *multi_probe_level = lsh->L;
    if (bits) std::copy(lsh->bits.begin(), lsh->bits.end(), bits);
    return TB_OK;
}

/* one pair staged for tbk_lsh_batch, as bf_host stages it for tbk_bf_batch */
static int lsh_host(tb_ctx* ctx, const tb_lsh* lsh, const uint8_t* d1, int n1, const uint8_t* d2, int n2, int filter, float ratio,
                    float min_th, tb_match* out, int cap, int* count) {
    if (!ctx || !lsh || lsh->ctx != ctx || !count || n1 < 0 || n2 < 0 || (n1 && !d1) || (n2 && !d2)) return TB_EINVAL;
    *count = 0;
    if (n1 > TB_LSH_MAX_N || n2 > TB_LSH_MAX_N) return tb_fail(ctx, TB_EINVAL, "searchByNN: sets of %d / %d descriptors (at most %d)", n1, n2, TB_LSH_MAX_N);
    if (n1 == 0 || n2 == 0) return TB_OK;
    const int max_n = std::max(n1, n2);
    const size_t pitch = (size_t)max_n * 32;
    size_t end = 0;
    const size_t oD1 = stage_piece(end, pitch), oD2 = stage_piece(end, pitch), oQb = stage_piece(end, (size_t)max_n * 8),
                 oOut = stage_piece(end, (size_t)n1 * sizeof(tb_match)), oCnt = stage_piece(end, 16);
    char* b;
    int rc;
    if ((rc = tb_scratch(ctx, TB_SLOT_HOST, end, (void**)&b))) return rc;
    const int32_t cnt[4] = {n1, n2, 0, 0}; /* n1, n2, then the match count and a flag that stays 0 */
    int32_t* dcnt = (int32_t*)(b + oCnt);
    TB_UPLOAD(ctx, b + oD1, d1, (size_t)n1 * 32);
    TB_UPLOAD(ctx, b + oD2, d2, (size_t)n2 * 32);
    TB_UPLOAD(ctx, dcnt, cnt, sizeof cnt);
    if ((rc = tbk_lsh_batch(ctx, 1, (const uint8_t*)(b + oD1), dcnt, (const uint8_t*)(b + oD2), dcnt + 1, pitch, max_n, lsh->d_bits, lsh->T,
                            lsh->k, lsh->L, filter, ratio, min_th, (tb_match*)(b + oOut), n1, dcnt + 2, (unsigned long long*)(b + oQb))))
        return rc;
    return match_tail(ctx, (const tb_match*)(b + oOut), dcnt + 2, cap, out, count);
}

int tb_match_lsh(tb_ctx* ctx, const tb_lsh* lsh, const uint8_t* d1, int n1, const uint8_t* d2, int n2, tb_match* out, int cap, int* count) {
    TB_ENTER(ctx);
    return lsh_host(ctx, lsh, d1, n1, d2, n2, 0, 0.f, 0.f, out, cap, count);
}

int tb_search_by_nn(tb_ctx* ctx, const tb_lsh* lsh, const uint8_t* d1, int n1, const uint8_t* d2, int n2, float ratio, float min_th,
                    tb_match* out, int cap, int* count) {
    TB_ENTER(ctx);
    return lsh_host(ctx, lsh, d1, n1, d2, n2, 1, ratio, min_th, out, cap, count);
}

int tb_search_by_nn_batch_dev(tb_ctx* ctx, const tb_lsh* lsh, int npairs, const uint8_t* desc1, const int32_t* counts1, const uint8_t* desc2,
                              const int32_t* counts2, size_t set_pitch, float ratio, float min_th, tb_match* out, int cap,
                              int32_t* out_counts) {
    TB_ENTER(ctx);
    if (!ctx || !lsh || lsh->ctx != ctx || npairs < 0 || !desc1 || !desc2 || !counts1 || !counts2 || !out || !out_counts || set_pitch < 32 ||
        cap < 1)
        return TB_EINVAL;
    if (set_pitch / 32 > TB_LSH_MAX_N) return tb_fail(ctx, TB_EINVAL, "searchByNN: %zu descriptors per set (at most %d)", set_pitch / 32, TB_LSH_MAX_N);
    if (npairs == 0) return TB_OK;
    const int max_n = (int)(set_pitch / 32);
    void* qb;
    int rc;
    if ((rc = tb_scratch(ctx, TB_SLOT_BF_QUERY, (size_t)npairs * max_n * 8, &qb))) return rc;
    return tbk_lsh_batch(ctx, npairs, desc1, counts1, desc2, counts2, set_pitch, max_n, lsh->d_bits, lsh->T, lsh->k, lsh->L, 1, ratio, min_th,
                         out, cap, out_counts, (unsigned long long*)qb);
}

/* ---- DBoW2 transform (see include/tb_capi.h) */
void tb_vocab_destroy(tb_vocab* v) {
    if (!v) return;
    if (v->ctx) hipSetDevice(v->ctx->device);
    hipFree(v->d_child_start); hipFree(v->d_child_items); hipFree(v->d_word_id); hipFree(v->d_desc); hipFree(v->d_weight);
    delete v;
}

int tb_vocab_create(tb_ctx* ctx, const tb_vocabulary* h, tb_vocab** out) {
    TB_ENTER(ctx);
    if (!ctx || !h || !out || h->nnodes < 1 || !h->child_start || !h->desc || !h->word_id || !h->weight) return TB_EINVAL;
    *out = nullptr;
    const int nn = h->nnodes, nc = h->child_start[nn];
    /* the tree must be walkable without a bounds test in the kernel: offsets ascending, children in range, no node its own
     * ancestor (children have larger ids than their parents in every DBoW2 file: ids are assigned in creation order) */
    if (h->child_start[0] != 0 || nc < 0 || nc > nn || (nc && !h->child_items)) return tb_fail(ctx, TB_EINVAL, "vocabulary: child offsets");
    for (int n = 0; n < nn; n++) {
        if (h->child_start[n + 1] < h->child_start[n]) return tb_fail(ctx, TB_EINVAL, "vocabulary: child offsets of node %d", n);
        for (int c = h->child_start[n]; c < h->child_start[n + 1]; c++)
            if (h->child_items[c] <= n || h->child_items[c] >= nn) return tb_fail(ctx, TB_EINVAL, "vocabulary: child %d of node %d", h->child_items[c], n);
    }
    tb_vocab* v = new (std::nothrow) tb_vocab();
    if (!v) return TB_ENOMEM;
    v->ctx = ctx; v->nnodes = nn; v->k = h->k; v->L = h->L; v->weighting = h->weighting; v->scoring = h->scoring;
    hipError_t e = hipMalloc(&v->d_child_start, (size_t)(nn + 1) * 4);
    if (e == hipSuccess) e = hipMalloc(&v->d_child_items, (size_t)std::max(nc, 1) * 4);
    if (e == hipSuccess) e = hipMalloc(&v->d_word_id, (size_t)nn * 4);
    if (e == hipSuccess) e = hipMalloc(&v->d_desc, (size_t)nn * 32);
    if (e == hipSuccess) e = hipMalloc(&v->d_weight, (size_t)nn * 8);
    if (e == hipSuccess) e = hipMemcpy(v->d_child_start, h->child_start, (size_t)(nn + 1) * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && nc) e = hipMemcpy(v->d_child_items, h->child_items, (size_t)nc * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(v->d_word_id, h->word_id, (size_t)nn * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(v->d_desc, h->desc, (size_t)nn * 32, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(v->d_weight, h->weight, (size_t)nn * 8, hipMemcpyHostToDevice);
    if (e != hipSuccess) { tb_vocab_destroy(v); return tb_fail(ctx, TB_EDEVICE, "vocabulary upload: %s", hipGetErrorString(e)); }
    *out = v;
    return TB_OK;
}

/* ---- vocabulary training (see include/tb_capi.h; k_vocab.hip) */
static int vocab_train_args(tb_ctx* ctx, const tb_vocab_train_params* P, int ndocs, const uint8_t* desc, const int32_t* counts,
                            tb_vocab** out, tb_vocab_train_stats* stats) {
    if (!ctx || !P || !out || !stats || ndocs < 0 || (ndocs && !counts)) return TB_EINVAL;
    *out = nullptr;
    if (P->max_iters < 1 || P->k < 0 || P->L < 0 || P->weighting < 0 || P->weighting > 3 || P->scoring < 0 || P->scoring > 5)
        return tb_fail(ctx, TB_EINVAL, "vocabulary training: max_iters %d, k %d, L %d, weighting %d, scoring %d", P->max_iters, P->k, P->L,
                       P->weighting, P->scoring);
    if (P->k < 2 || P->k > 32 || P->L < 1 || P->L > TB_VOC_MAX_L)
        return tb_fail(ctx, TB_EUNSUPPORTED, "vocabulary training: k %d outside 2..32 or L %d outside 1..%d", P->k, P->L, TB_VOC_MAX_L);
    return TB_OK;
}

static int vocab_train_run(tb_ctx* ctx, const tb_vocab_train_params* P, int ndocs, const uint8_t* d_desc, const int32_t* h_counts,
                           int desc_pitch, tb_vocab** out, tb_vocab_train_stats* stats) {
    long long total = 0;
    for (int d = 0; d < ndocs; d++) {
        if (h_counts[d] < 0 || h_counts[d] > desc_pitch) return tb_fail(ctx, TB_EINVAL, "vocabulary training: %d descriptors in document %d", h_counts[d], d);
        total += h_counts[d];
    }
    if (total > (1ll << 26)) return tb_fail(ctx, TB_EUNSUPPORTED, "vocabulary training: %lld descriptors (at most 2^26)", total);
    if (total && !d_desc) return TB_EINVAL;
    tb_vocab* v = new (std::nothrow) tb_vocab();
    if (!v) return TB_ENOMEM;
    v->ctx = ctx; v->k = P->k; v->L = P->L; v->weighting = P->weighting; v->scoring = P->scoring;
    tb_vocab_arrays a;
    const int rc = tbk_vocab_train(ctx, P, ndocs, d_desc, h_counts, desc_pitch, &a, stats);
    if (rc) { delete v; return rc; }
    v->nnodes = a.nnodes; v->d_child_start = a.d_child_start; v->d_child_items = a.d_child_items; v->d_word_id = a.d_word_id;
    v->d_desc = a.d_desc; v->d_weight = a.d_weight;
    *out = v;
    return TB_OK;
}

int tb_vocab_train_dev(tb_ctx* ctx, const tb_vocab_train_params* P, int ndocs, const uint8_t* desc, const int32_t* counts,
                       int desc_pitch, tb_vocab** out, tb_vocab_train_stats* stats) {
    TB_ENTER(ctx);
    int rc;
    if ((rc = vocab_train_args(ctx, P, ndocs, desc, counts, out, stats))) return rc;
    if (desc_pitch < 0) return TB_EINVAL;
    std::vector<int32_t> hc(ndocs);
    if (ndocs) {
        TB_HIP(ctx, hipMemcpyAsync(hc.data(), counts, (size_t)ndocs * 4, hipMemcpyDeviceToHost, ctx->stream));
        TB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return vocab_train_run(ctx, P, ndocs, desc, hc.data(), desc_pitch, out, stats);
}

int tb_vocab_train(tb_ctx* ctx, const tb_vocab_train_params* P, int ndocs, const uint8_t* desc, const int32_t* counts, tb_vocab** out,
                   tb_vocab_train_stats* stats) {
    TB_ENTER(ctx);
    int rc;
    if ((rc = vocab_train_args(ctx, P, ndocs, desc, counts, out, stats))) return rc;
    int pitch = 0;
    long long total = 0;
    for (int d = 0; d < ndocs; d++) {
        if (counts[d] < 0) return tb_fail(ctx, TB_EINVAL, "vocabulary training: %d descriptors in document %d", counts[d], d);
        pitch = std::max(pitch, counts[d]);
        total += counts[d];
    }
    if (total > (1ll << 26)) return tb_fail(ctx, TB_EUNSUPPORTED, "vocabulary training: %lld descriptors (at most 2^26)", total);
    if (total && !desc) return TB_EINVAL;
    /* the documents, one per row of the _dev form's [ndocs][pitch][32]; the padding is never read */
    uint8_t* d_rows = nullptr;
    if (total) {
        TB_HIP(ctx, hipMalloc(&d_rows, (size_t)ndocs * pitch * 32));
        size_t at = 0;
        for (int d = 0; d < ndocs; d++) {
            if (counts[d]) {
                const hipError_t e = hipMemcpyAsync(d_rows + (size_t)d * pitch * 32, desc + at, (size_t)counts[d] * 32, hipMemcpyHostToDevice, ctx->stream);
                if (e != hipSuccess) { hipFree(d_rows); return tb_fail(ctx, TB_EDEVICE, "vocabulary training upload: %s", hipGetErrorString(e)); }
            }
            at += (size_t)counts[d] * 32;
        }
    }
    rc = vocab_train_run(ctx, P, ndocs, d_rows, counts, pitch, out, stats);
    hipStreamSynchronize(ctx->stream);
    hipFree(d_rows);
    return rc;
}

int tb_vocab_info(const tb_vocab* v, int* nnodes, int* nwords, int* k, int* L, int* weighting, int* scoring) {
    if (!v || !v->ctx) return TB_EINVAL;
    TB_ENTER(v->ctx);
    if (nnodes) *nnodes = v->nnodes;
    if (k) *k = v->k;
    if (L) *L = v->L;
    if (weighting) *weighting = v->weighting;
    if (scoring) *scoring = v->scoring;
    if (nwords) {   /* the childless nodes other than the root */
        std::vector<int32_t> cs((size_t)v->nnodes + 1);
        TB_HIP(v->ctx, hipMemcpy(cs.data(), v->d_child_start, cs.size() * 4, hipMemcpyDeviceToHost));
        int n = 0;
        for (int i = 1; i < v->nnodes; i++) n += cs[i + 1] == cs[i];
        *nwords = n;
    }
    return TB_OK;
}

int tb_vocab_export(const tb_vocab* v, int32_t* child_start, int32_t* child_items, uint8_t* desc, int32_t* word_id, double* weight) {
    if (!v || !v->ctx) return TB_EINVAL;
    tb_ctx* ctx = v->ctx;
    TB_ENTER(ctx);
    const size_t nn = (size_t)v->nnodes;
    TB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (child_start) TB_HIP(ctx, hipMemcpy(child_start, v->d_child_start, (nn + 1) * 4, hipMemcpyDeviceToHost));
    if (child_items) {
        int32_t nc = 0;
        TB_HIP(ctx, hipMemcpy(&nc, v->d_child_start + nn, 4, hipMemcpyDeviceToHost));
        if (nc) TB_HIP(ctx, hipMemcpy(child_items, v->d_child_items, (size_t)nc * 4, hipMemcpyDeviceToHost));
    }
    if (desc) TB_HIP(ctx, hipMemcpy(desc, v->d_desc, nn * 32, hipMemcpyDeviceToHost));
    if (word_id) TB_HIP(ctx, hipMemcpy(word_id, v->d_word_id, nn * 4, hipMemcpyDeviceToHost));
    if (weight) TB_HIP(ctx, hipMemcpy(weight, v->d_weight, nn * 8, hipMemcpyDeviceToHost));
    return TB_OK;
}

int tb_bow_transform_batch_dev(tb_ctx* ctx, const tb_vocab* voc, int nframes, const uint8_t* desc, const int32_t* counts,
                               int desc_pitch, int levelsup, int32_t* word_ids, int32_t* node_ids, double* weights,
                               uint64_t* fv_keys, int32_t* fv_counts) {
    TB_ENTER(ctx);
    if (!ctx || !voc || voc->ctx != ctx || nframes < 0 || desc_pitch < 0 || levelsup < 0) return TB_EINVAL;
    if (nframes == 0 || desc_pitch == 0) return TB_OK;
    if (!desc || (fv_keys && (!fv_counts || desc_pitch > 8192))) return TB_EINVAL;
    void *dn = node_ids, *dwt = weights;
    int rc;
    if (fv_keys && !node_ids && (rc = tb_scratch(ctx, TB_SLOT_BOW_NODES, (size_t)nframes * desc_pitch * 4, &dn))) return rc;
    if (fv_keys && !weights && (rc = tb_scratch(ctx, TB_SLOT_BOW_WEIGHTS, (size_t)nframes * desc_pitch * 8, &dwt))) return rc;
    return tbk_bow_transform(ctx, voc->nnodes, voc->L, voc->d_child_start, voc->d_child_items, voc->d_desc, voc->d_word_id, voc->d_weight,
                             nframes, desc, counts, desc_pitch, levelsup, word_ids, (int32_t*)dn, (double*)dwt,
                             (unsigned long long*)fv_keys, fv_counts);
}

int tb_bow_vector_batch_dev(tb_ctx* ctx, const tb_vocab* voc, int nframes, const int32_t* word_ids, const double* weights,
                            const int32_t* counts, int desc_pitch, int32_t* bv_words, double* bv_values, int32_t* bv_counts) {
    TB_ENTER(ctx);
    if (!ctx || !voc || voc->ctx != ctx || nframes < 0 || desc_pitch < 0 || desc_pitch > 8192) return TB_EINVAL;
    if (voc->weighting < 0 || voc->weighting > 3 || voc->scoring < 0 || voc->scoring > 5)
        return tb_fail(ctx, TB_EINVAL, "tb_bow_vector_batch_dev: the vocabulary's weighting %d / scoring %d", voc->weighting, voc->scoring);
    if (nframes == 0 || desc_pitch == 0) return TB_OK;
    if (!word_ids || !weights || !counts || !bv_words || !bv_values || !bv_counts) return TB_EINVAL;
    return tbk_bow_vector(ctx, nframes, word_ids, weights, counts, desc_pitch, voc->weighting, voc->scoring, bv_words, bv_values, bv_counts);
}

/* ---- TemplatedVocabulary::score (TemplatedVocabulary.h:156-162, :1199-1203 -> ScoringObject.cpp:23-311), see include/tb_capi.h.
 * The host form is the walk itself, two cursors on the sorted lists with std::map::lower_bound as std::lower_bound; this file is
 * built with -ffp-contract=off, so every statement is one rounding, as in the reference's build. */
static const double TB_LOG_EPS = log(DBL_EPSILON);   /* GeneralScoring::LOG_EPS, ScoringObject.cpp:18 */

int tb_bow_score(int scoring, const int32_t* aw, const double* av, int na, const int32_t* bw, const double* bv, int nb, double* out) {
    if (scoring < 0 || scoring > 5 || na < 0 || nb < 0 || !out || (na && (!aw || !av)) || (nb && (!bw || !bv))) return TB_EINVAL;
    double score = 0;
    int i = 0, j = 0;
    while (i < na && j < nb) {
        const double vi = av[i], wi = bv[j];
        if (aw[i] == bw[j]) {
            switch (scoring) {
            case 0: score += fabs(vi - wi) - fabs(vi) - fabs(wi); break;          /* :41 */
            case 2: if (vi + wi != 0.0) score += vi * wi / (vi + wi); break;      /* :148 */
            case 3: if (vi != 0 && wi != 0) score += vi * log(vi / wi); break;    /* :195 */
            case 4: score += sqrt(vi * wi); break;                                /* :245 */
            default: score += vi * wi; break;                                     /* :91, :290 */
            }
            ++i; ++j;
        } else if (aw[i] < bw[j]) {
            if (scoring == 3) { score += vi * (log(vi) - TB_LOG_EPS); ++i; }      /* :204: KL moves v1 one step */
            else i = (int)(std::lower_bound(aw + i, aw + na, bw[j]) - aw);
        } else {
            j = (int)(std::lower_bound(bw + j, bw + nb, aw[i]) - bw);
        }
    }
    switch (scoring) {
    case 0: score = -score / 2.0; break;                                          /* :65 */
    case 1: if (score >= 1) score = 1.0; else score = 1.0 - sqrt(1.0 - score); break;   /* :114-117 */
    case 2: score = 2. * score; break;                                            /* :167 */
    case 3:
        for (; i < na; ++i)                                                       /* :216-218 */
            if (av[i] != 0) score += av[i] * (log(av[i]) - TB_LOG_EPS);
        break;
    default: break;
    }
    *out = score;
    return TB_OK;
}

int tb_bow_score_batch_dev(tb_ctx* ctx, int scoring, int mode, int na, const int32_t* a_words, const double* a_values,
                           const int32_t* a_counts, int a_pitch, int nb, const int32_t* b_words, const double* b_values,
                           const int32_t* b_counts, int b_pitch, double* out) {
    TB_ENTER(ctx);
    if (!ctx) return TB_EINVAL;
    if (scoring < 0 || scoring > 5 || (mode != TB_SCORE_PAIRWISE && mode != TB_SCORE_ALL_PAIRS) || na < 0 || nb < 0 || a_pitch < 1 ||
        a_pitch > 8192 || b_pitch < 1 || b_pitch > 8192 || (mode == TB_SCORE_PAIRWISE && na != nb))
        return tb_fail(ctx, TB_EINVAL, "tb_bow_score_batch_dev: scoring %d, mode %d, %d x %d vectors, pitches %d / %d", scoring, mode, na, nb,
                       a_pitch, b_pitch);
    if (na == 0 || nb == 0) return TB_OK;
    if (!a_words || !a_values || !a_counts || !b_words || !b_values || !b_counts || !out) return TB_EINVAL;
    const bool pw = mode == TB_SCORE_PAIRWISE;
    return tbk_bow_score(ctx, scoring, TB_LOG_EPS, na, a_words, a_values, a_counts, a_pitch, b_words, b_values, b_counts, b_pitch,
                         pw ? 1 : nb, pw ? 1 : 0, 0, 0, 0, 0, out);
}

/* ---- the keyframe database: per sequence a ring of BowVectors (see include/tb_capi.h) */
void tb_bow_db_destroy(tb_bow_db* db) {
    if (!db) return;
    if (db->ctx) { hipSetDevice(db->ctx->device); hipStreamSynchronize(db->ctx->stream); }
    db->own.release();
    delete db;
}

int tb_bow_db_clear(tb_bow_db* db) {
    TB_ENTER((db ? db->ctx : nullptr));
    if (!db) return TB_EINVAL;
    tb_ctx* ctx = db->ctx;
    const size_t n = (size_t)db->nseq * db->cap;
    TB_HIP(ctx, hipMemsetAsync(db->counts, 0, n * sizeof(int32_t), ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(db->kf_ids, 0xff, n * sizeof(int32_t), ctx->stream));
    db->nadded = 0;
    return TB_OK;
}

int tb_bow_db_create(tb_ctx* ctx, int nseq, int capacity, int pitch, int scoring, tb_bow_db** out) {
    TB_ENTER(ctx);
    if (!ctx || !out) return TB_EINVAL;
    *out = nullptr;
    if (nseq < 1 || capacity < 1 || capacity > 1024 || pitch < 1 || pitch > 8192 || scoring < 0 || scoring > 5)
        return tb_fail(ctx, TB_EINVAL, "tb_bow_db_create: %d sequences, capacity %d (1..1024), pitch %d (1..8192), scoring %d", nseq,
                       capacity, pitch, scoring);
    std::unique_ptr<tb_bow_db, void (*)(tb_bow_db*)> du(new tb_bow_db(), tb_bow_db_destroy);
    tb_bow_db* db = du.get();
    db->ctx = ctx; db->nseq = nseq; db->cap = capacity; db->pitch = pitch; db->scoring = scoring;
    const size_t n = (size_t)nseq * capacity;
    TB_TRY(tb_dev_alloc(ctx, db->own, &db->words, n * pitch));
    TB_TRY(tb_dev_alloc(ctx, db->own, &db->values, n * pitch));
    TB_TRY(tb_dev_alloc(ctx, db->own, &db->counts, n));
    TB_TRY(tb_dev_alloc(ctx, db->own, &db->kf_ids, n));
    TB_TRY(tb_bow_db_clear(db));
    *out = du.release();
    return TB_OK;
}

int tb_bow_db_add_dev(tb_bow_db* db, const int32_t* bv_words, const double* bv_values, const int32_t* bv_counts, int src_pitch,
                      int32_t kf_id) {
    TB_ENTER((db ? db->ctx : nullptr));
    if (!db) return TB_EINVAL;
    if (!bv_words || !bv_values || !bv_counts || src_pitch < 1 || src_pitch > db->pitch || kf_id < 0)
        return tb_fail(db->ctx, TB_EINVAL, "tb_bow_db_add_dev: source pitch %d (database: %d), kf_id %d", src_pitch, db->pitch, (int)kf_id);
    int rc = tbk_bow_db_add(db->ctx, db->nseq, bv_words, bv_values, bv_counts, src_pitch, db->cap, db->pitch, (int)(db->nadded % db->cap),
                            kf_id, db->words, db->values, db->counts, db->kf_ids);
    if (rc) return rc;
    db->nadded++;
    return TB_OK;
}

int tb_bow_db_query_dev(tb_bow_db* db, const int32_t* q_words, const double* q_values, const int32_t* q_counts, int q_pitch,
                        int exclude_newest, int topk, double* scores, int32_t* top_slot, int32_t* top_kf, double* top_score,
                        int32_t* top_count) {
    TB_ENTER((db ? db->ctx : nullptr));
    if (!db) return TB_EINVAL;
    tb_ctx* ctx = db->ctx;
    if (!q_words || !q_values || !q_counts || !scores || q_pitch < 1 || q_pitch > db->pitch || exclude_newest < 0 || topk < 0 ||
        topk > db->cap || (topk && (!top_slot || !top_kf || !top_score)))
        return tb_fail(ctx, TB_EINVAL, "tb_bow_db_query_dev: query pitch %d (database: %d), exclude_newest %d, topk %d (capacity %d)", q_pitch,
                       db->pitch, exclude_newest, topk, db->cap);
    const int nfilled = (int)std::min<long long>(db->nadded, db->cap);
    const int newest = db->nadded ? (int)((db->nadded - 1) % db->cap) : 0;
    int rc = tbk_bow_score(ctx, db->scoring, TB_LOG_EPS, db->nseq, q_words, q_values, q_counts, q_pitch, db->words, db->values, db->counts,
                           db->pitch, db->cap, db->cap, 1, nfilled, newest, exclude_newest, scores);
    if (rc) return rc;
    if (topk == 0 && !top_count) return TB_OK;
    return tbk_bow_db_rank(ctx, db->nseq, scores, db->kf_ids, db->cap, nfilled, newest, exclude_newest, db->scoring == 3, topk, top_slot,
                           top_kf, top_score, top_count);
}

int tb_bow_db_state_dev(tb_bow_db* db, const int32_t** words, const double** values, const int32_t** counts, const int32_t** kf_ids,
                        int* nadded) {
    if (!db) return TB_EINVAL;
    if (words) *words = db->words;
    if (values) *values = db->values;
    if (counts) *counts = db->counts;
    if (kf_ids) *kf_ids = db->kf_ids;
    if (nadded) *nadded = (int)std::min<long long>(db->nadded, INT_MAX);
    return TB_OK;
}

/* ---- the keyframe store and candidate verification (see include/tb_capi.h) */
void tb_kf_store_destroy(tb_kf_store* st) {
    if (!st) return;
    if (st->ctx) { hipSetDevice(st->ctx->device); hipStreamSynchronize(st->ctx->stream); }
    st->own.release();
    delete st;
}

int tb_kf_store_clear(tb_kf_store* st) {
    TB_ENTER((st ? st->ctx : nullptr));
    if (!st) return TB_EINVAL;
    tb_ctx* ctx = st->ctx;
    const size_t n = (size_t)st->nseq * st->cap;
    TB_HIP(ctx, hipMemsetAsync(st->counts, 0, n * sizeof(int32_t), ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(st->fv_counts, 0, n * sizeof(int32_t), ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(st->kf_ids, 0xff, n * sizeof(int32_t), ctx->stream));
    st->nadded = 0;
    st->s3_best = false;   /* a winner of the ring that was: tb_kf_store_sim3_graph_dev needs a new Sim(3) query */
    st->s3_done = false;   /* and so does tb_kf_store_sim3_refine_dev */
    st->w3_use = false;    /* the widened lists of a search belong to the ring that was */
    return TB_OK;
}

int tb_kf_store_create(tb_ctx* ctx, int nseq, int capacity, int pitch, int max_candidates, tb_kf_store** out) {
    TB_ENTER(ctx);
    if (!ctx || !out) return TB_EINVAL;
    *out = nullptr;
    if (nseq < 1 || capacity < 1 || capacity > 1024 || pitch < 1 || pitch > 8192 || max_candidates < 1 || max_candidates > capacity ||
        (long long)nseq * max_candidates > 65535)
        return tb_fail(ctx, TB_EINVAL, "tb_kf_store_create: %d sequences, capacity %d (1..1024), pitch %d (1..8192), max_candidates %d (1..capacity, at most 65535 pairs)",
                       nseq, capacity, pitch, max_candidates);
    std::unique_ptr<tb_kf_store, void (*)(tb_kf_store*)> su(new tb_kf_store(), tb_kf_store_destroy);
    tb_kf_store* st = su.get();
    st->ctx = ctx; st->nseq = nseq; st->cap = capacity; st->pitch = pitch; st->max_cand = max_candidates;
    const size_t n = (size_t)nseq * capacity, np = n * pitch, pairs = (size_t)nseq * max_candidates, pp = pairs * pitch;
    tb_dev_owner& own = st->own;
    TB_TRY(tb_dev_alloc(ctx, own, &st->keys, np));
    TB_TRY(tb_dev_alloc(ctx, own, &st->desc, np * 32));
    TB_TRY(tb_dev_alloc(ctx, own, &st->fv, np));
    TB_TRY(tb_dev_alloc(ctx, own, &st->mp, np * 3));
    TB_TRY(tb_dev_alloc(ctx, own, &st->valid, np));
    TB_TRY(tb_dev_alloc(ctx, own, &st->Tcw, n * 16));
    TB_TRY(tb_dev_alloc(ctx, own, &st->counts, n));
    TB_TRY(tb_dev_alloc(ctx, own, &st->fv_counts, n));
    TB_TRY(tb_dev_alloc(ctx, own, &st->kf_ids, n));
    TB_TRY(tb_dev_alloc(ctx, own, &st->ix1, pairs));
    TB_TRY(tb_dev_alloc(ctx, own, &st->ix2, pairs));
    TB_TRY(tb_dev_alloc(ctx, own, &st->best, pp * 4));
    TB_TRY(tb_dev_alloc(ctx, own, &st->matches, pp));
    TB_TRY(tb_dev_alloc(ctx, own, &st->obs, pp));
    TB_TRY(tb_dev_alloc(ctx, own, &st->outlier, pp));
    TB_TRY(tb_dev_alloc(ctx, own, &st->err, pp * 3));
    TB_TRY(tb_dev_alloc(ctx, own, &st->seed, pairs * 16));
    TB_TRY(tb_dev_alloc(ctx, own, &st->pose, pairs * 16));
    TB_TRY(tb_dev_alloc(ctx, own, &st->mcounts, pairs, 0));
    TB_TRY(tb_dev_alloc(ctx, own, &st->flags, pairs));
    TB_TRY(tb_dev_alloc(ctx, own, &st->ocounts, pairs, 0));
    TB_TRY(tb_dev_alloc(ctx, own, &st->ninl, pairs));
    TB_TRY(tb_dev_alloc(ctx, own, &st->ckf, pairs));
    TB_TRY(tb_kf_store_clear(st));
    *out = su.release();
    return TB_OK;
}

int tb_kf_store_add_dev(tb_kf_store* st, const tb_keypoint* keys, const uint8_t* desc, const int32_t* counts, const uint64_t* fv_keys,
                        const int32_t* fv_counts, const float* map_points, const uint8_t* mp_valid, int src_pitch, const float* Tcw,
                        int32_t kf_id) {
    TB_ENTER((st ? st->ctx : nullptr));
    if (!st) return TB_EINVAL;
    if (!keys || !desc || !counts || !fv_keys || !fv_counts || !map_points || !mp_valid || !Tcw || src_pitch < 1 || src_pitch > st->pitch ||
        kf_id < 0)
        return tb_fail(st->ctx, TB_EINVAL, "tb_kf_store_add_dev: source pitch %d (store: %d), kf_id %d", src_pitch, st->pitch, (int)kf_id);
    int rc = tbk_kf_store_add(st->ctx, st->nseq, keys, desc, counts, (const unsigned long long*)fv_keys, fv_counts, map_points, mp_valid,
                              src_pitch, Tcw, kf_id, st->cap, st->pitch, (int)(st->nadded % st->cap), st->keys, st->desc,
                              (unsigned long long*)st->fv, st->mp, st->valid, st->Tcw, st->counts, st->fv_counts, st->kf_ids);
    if (rc) return rc;
    st->nadded++;
    return TB_OK;
}

int tb_kf_store_state_dev(tb_kf_store* st, const tb_keypoint** keys, const uint8_t** desc, const int32_t** counts,
                          const uint64_t** fv_keys, const int32_t** fv_counts, const float** map_points, const uint8_t** mp_valid,
                          const float** Tcw, const int32_t** kf_ids, int* nadded) {
    if (!st) return TB_EINVAL;
    if (keys) *keys = st->keys;
    if (desc) *desc = st->desc;
    if (counts) *counts = st->counts;
    if (fv_keys) *fv_keys = st->fv;
    if (fv_counts) *fv_counts = st->fv_counts;
    if (map_points) *map_points = st->mp;
    if (mp_valid) *mp_valid = st->valid;
    if (Tcw) *Tcw = st->Tcw;
    if (kf_ids) *kf_ids = st->kf_ids;
    if (nadded) *nadded = (int)std::min<long long>(st->nadded, INT_MAX);
    return TB_OK;
}

int tb_kf_store_work_dev(tb_kf_store* st, tb_match** matches, int32_t** match_counts, const tb_obs** rows, const int32_t** row_counts,
                         const uint8_t** outlier, int* pitch) {
    if (!st) return TB_EINVAL;
    if (matches) *matches = st->matches;
    if (match_counts) *match_counts = st->mcounts;
    if (rows) *rows = st->obs;
    if (row_counts) *row_counts = st->ocounts;
    if (outlier) *outlier = st->outlier;
    if (pitch) *pitch = st->pitch;
    return TB_OK;
}

int tb_kf_store_pnp_enable(tb_kf_store* st, const tb_pnp_params* prm, int min_consensus, int expand) {
    TB_ENTER((st ? st->ctx : nullptr));
    if (!st) return TB_EINVAL;
    tb_ctx* ctx = st->ctx;
    if (st->pnp_on) return tb_fail(ctx, TB_ESTATE, "tb_kf_store_pnp_enable: enabled already");
    static const tb_pnp_params dflt = {256, 5.991, 0};
    const tb_pnp_params P = prm ? *prm : dflt;
    if (P.hypotheses < 1 || P.hypotheses > 1024 || !(P.chi2_max >= 0.0) || !std::isfinite(P.chi2_max) || min_consensus < 3 ||
        (expand != 0 && expand != 1))
        return tb_fail(ctx, TB_EINVAL, "tb_kf_store_pnp_enable: hypotheses %d (1..1024), chi2_max finite and not negative, min_consensus %d (>= 3), expand %d (0, 1)",
                       P.hypotheses, min_consensus, expand);
    const size_t pairs = (size_t)st->nseq * st->max_cand, pp = pairs * st->pitch;
    tb_dev_owner& own = st->own;
    TB_TRY(tb_dev_alloc(ctx, own, &st->rows0, pp));
    TB_TRY(tb_dev_alloc(ctx, own, &st->pmask, pp));
    TB_TRY(tb_dev_alloc(ctx, own, &st->took, pairs, 0));
    TB_TRY(tb_dev_alloc(ctx, own, &st->ppose, pairs * 16, 0));
    TB_TRY(tb_dev_alloc(ctx, own, &st->seed2, pairs * 16));
    TB_TRY(tb_dev_alloc(ctx, own, &st->cnt0, pairs, 0));
    TB_TRY(tb_dev_alloc(ctx, own, &st->pcons, pairs, 0));
    TB_TRY(tb_dev_alloc(ctx, own, &st->pwin, pairs * 2, 0));
    TB_TRY(tb_dev_alloc(ctx, own, &st->pflags, pairs, 0));
    if (expand) {
        TB_TRY(tb_dev_alloc(ctx, own, &st->rows2, pp));
        TB_TRY(tb_dev_alloc(ctx, own, &st->outlier2, pp));
        TB_TRY(tb_dev_alloc(ctx, own, &st->pose2, pairs * 16));
        TB_TRY(tb_dev_alloc(ctx, own, &st->cnt2, pairs));
        TB_TRY(tb_dev_alloc(ctx, own, &st->ninl2, pairs));
    }
    st->pnp = P; st->pnp_min = min_consensus; st->pnp_expand = expand;
    st->pnp_on = true;
    return TB_OK;
}

int tb_kf_store_pnp_state_dev(tb_kf_store* st, const tb_obs** rows, const int32_t** row_counts, const int32_t** consensus,
                              const int32_t** winner, const float** Tcw, const uint8_t** took, const int32_t** flags) {
    if (!st) return TB_EINVAL;
    if (!st->pnp_on) return tb_fail(st->ctx, TB_ESTATE, "tb_kf_store_pnp_state_dev: PnP verification is not enabled");
    if (rows) *rows = st->rows0;
    if (row_counts) *row_counts = st->cnt0;
    if (consensus) *consensus = st->pcons;
    if (winner) *winner = st->pwin;
    if (Tcw) *Tcw = st->ppose;
    if (took) *took = st->took;
    if (flags) *flags = st->pflags;
    return TB_OK;
}

/* the checks both verification entry points share, and invLevelSigma2 */
static int reloc_check(tb_kf_store* st, const char* who, int nlevels, float scale, const void* q_keys, const void* q_counts, int q_pitch,
                       const void* cand_slot, int ncand, float* inv_sigma2) {
    tb_ctx* ctx = st->ctx;
    if (!q_keys || !q_counts || !cand_slot || ncand < 1 || ncand > st->max_cand || q_pitch < 1 || q_pitch > st->pitch || nlevels < 1 ||
        nlevels > TB_MAX_LEVELS || !std::isfinite(scale))
        return tb_fail(ctx, TB_EINVAL, "%s: ncand %d (1..%d), query pitch %d (store: %d), %d levels", who, ncand, st->max_cand, q_pitch,
                       st->pitch, nlevels);
    float sf[TB_MAX_LEVELS];
    return tb_scale_factors(nlevels, scale, sf, nullptr, nullptr, inv_sigma2);
}

int tb_reloc_rows_dev(tb_kf_store* st, int nlevels, float scale, const tb_keypoint* q_keys, const int32_t* q_counts, int q_pitch,
                      const int32_t* cand_slot, int ncand, const int32_t* match_counts, int32_t* cand_rows) {
    TB_ENTER((st ? st->ctx : nullptr));
    if (!st) return TB_EINVAL;
    if (!match_counts) return tb_fail(st->ctx, TB_EINVAL, "tb_reloc_rows_dev: match_counts is required");
    float inv_sigma2[TB_MAX_LEVELS];
    int rc;
    if ((rc = reloc_check(st, "tb_reloc_rows_dev", nlevels, scale, q_keys, q_counts, q_pitch, cand_slot, ncand, inv_sigma2))) return rc;
    tb_ctx* ctx = st->ctx;
    if ((rc = tbk_reloc_pairs(ctx, st->nseq, ncand, st->cap, cand_slot, st->kf_ids, st->Tcw, st->ix1, st->ix2, st->seed, st->ckf))) return rc;
    return tbk_reloc_rows(ctx, st->nseq * ncand, q_keys, q_counts, q_pitch, st->ix1, st->ix2, st->matches, match_counts, st->mp, st->valid,
                          st->counts, st->pitch, inv_sigma2, nlevels, st->obs, st->ocounts, st->outlier, cand_rows);
}

int tb_relocalize_batch_dev(tb_kf_store* st, const double K[4], int nlevels, float scale, const tb_keypoint* q_keys,
                            const uint8_t* q_desc, const int32_t* q_counts, const uint64_t* q_fv_keys, const int32_t* q_fv_counts,
                            int q_pitch, const int32_t* cand_slot, int ncand, const tb_reloc_params* prm, const tb_reloc_out* out) {
    TB_ENTER((st ? st->ctx : nullptr));
    if (!st) return TB_EINVAL;
    tb_ctx* ctx = st->ctx;
    if (!K || !q_desc || !q_fv_keys || !q_fv_counts || !prm || prm->histo_len < 1 || prm->histo_len > 1024 || !std::isfinite(prm->nratio))
        return tb_fail(ctx, TB_EINVAL, "tb_relocalize_batch_dev: null arguments or searchByBow fields (histo_len %d)", prm ? prm->histo_len : 0);
    float inv_sigma2[TB_MAX_LEVELS];
    int rc;
    if ((rc = reloc_check(st, "tb_relocalize_batch_dev", nlevels, scale, q_keys, q_counts, q_pitch, cand_slot, ncand, inv_sigma2))) return rc;
    static const tb_reloc_out none = {};
    const tb_reloc_out& o = out ? *out : none;
    const int pairs = st->nseq * ncand;
    int32_t* ckf = o.cand_kf ? o.cand_kf : st->ckf;
    int32_t* mcounts = o.cand_matches ? o.cand_matches : st->mcounts;
    int32_t* flags = o.cand_flags ? o.cand_flags : st->flags;
    int32_t* ninl = o.cand_inliers ? o.cand_inliers : st->ninl;
    float* pose = o.cand_Tcw ? o.cand_Tcw : st->pose;
    if ((rc = tbk_reloc_pairs(ctx, st->nseq, ncand, st->cap, cand_slot, st->kf_ids, st->Tcw, st->ix1, st->ix2, st->seed, ckf))) return rc;
    /* side 1 = the query frame s, side 2 = the stored keyframe s * cap + slot, both read where they lie */
    if ((rc = tbk_bow_search_batch(ctx, pairs, q_keys, q_desc, q_pitch, (const unsigned long long*)q_fv_keys, q_fv_counts, st->keys, st->desc,
                                   st->pitch, (const unsigned long long*)st->fv, st->fv_counts, st->valid, prm->map_point_only, prm->th_low,
                                   prm->nratio, prm->histo_len, prm->check_orientation, st->matches, st->pitch, mcounts, flags, st->best,
                                   st->ix1, st->ix2)))
        return rc;
    if (!st->pnp_on) {
        if ((rc = tbk_reloc_rows(ctx, pairs, q_keys, q_counts, q_pitch, st->ix1, st->ix2, st->matches, mcounts, st->mp, st->valid, st->counts,
                                 st->pitch, inv_sigma2, nlevels, st->obs, st->ocounts, st->outlier, o.cand_rows)))
            return rc;
        if ((rc = tbk_pose_batch(ctx, pairs, K, st->seed, st->obs, st->ocounts, st->pitch, st->outlier, pose, ninl, nullptr, st->err))) return rc;
    } else {
        /* rows -> P3P-RANSAC with the stored pose as the prior -> the consensus rows and the PnP pose into the pose stage, or every
         * row and the stored seed where the consensus is short -> (expand) the optimised pose's inliers among all rows, once more */
        TB_TRY(tbk_reloc_rows(ctx, pairs, q_keys, q_counts, q_pitch, st->ix1, st->ix2, st->matches, mcounts, st->mp, st->valid, st->counts,
                              st->pitch, inv_sigma2, nlevels, st->rows0, st->cnt0, st->outlier, nullptr));
        TB_TRY(tbk_pnp_batch(ctx, pairs, K, st->rows0, st->cnt0, st->pitch, st->pnp.hypotheses, st->pnp.chi2_max, st->pnp.seed, st->seed,
                             st->ppose, st->pcons, st->pmask, st->pwin, st->pflags));
        TB_TRY(tbk_pnp_gather(ctx, pairs, 0, K, st->pnp.chi2_max, st->pnp_min, st->rows0, st->cnt0, st->pitch, st->pmask, st->pcons, st->ppose,
                              st->seed, st->took, st->obs, st->ocounts, st->outlier, st->seed2, o.cand_rows));
        TB_TRY(tbk_pose_batch(ctx, pairs, K, st->seed2, st->obs, st->ocounts, st->pitch, st->outlier, pose, ninl, nullptr, st->err));
        if (st->pnp_expand) {
            TB_TRY(tbk_pnp_gather(ctx, pairs, 1, K, st->pnp.chi2_max, st->pnp_min, st->rows0, st->cnt0, st->pitch, nullptr, nullptr, pose,
                                  nullptr, st->took, st->rows2, st->cnt2, st->outlier2, nullptr, o.cand_rows));
            TB_TRY(tbk_pose_batch(ctx, pairs, K, pose, st->rows2, st->cnt2, st->pitch, st->outlier2, st->pose2, st->ninl2, nullptr, st->err));
            TB_TRY(tbk_pnp_adopt(ctx, pairs, st->took, st->pitch, st->rows2, st->cnt2, st->outlier2, st->pose2, st->ninl2, st->obs, st->ocounts,
                                 st->outlier, pose, ninl));
        }
    }
    if (mcounts != st->mcounts)   /* tb_kf_store_work_dev lends the last call's counts */
        TB_HIP(ctx, hipMemcpyAsync(st->mcounts, mcounts, (size_t)pairs * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
    st->reloc_done = true;   /* the match lists are filled, pair-major at this ncand: tb_kf_store_sim3_dev may read them */
    st->s3_done = false;     /* and they are no longer those the last Sim(3) query's masks and seeds belong to: no refinement on them */
    st->w3_use = false;      /* nor on the widened lists a search made of them */
    st->reloc_ncand = ncand;
    if (!o.best_rank && !o.best_kf && !o.best_Tcw) return TB_OK;
    return tbk_reloc_select(ctx, st->nseq, ncand, prm->min_inliers, ckf, ninl, pose, o.best_rank, o.best_kf, o.best_Tcw);
}

int tb_kf_store_sim3_dev(tb_kf_store* st, const double K[4], int nlevels, float scale, const tb_keypoint* q_keys, const int32_t* q_counts,
                         const float* q_map_points, const uint8_t* q_mp_valid, int q_pitch, const float* q_Tcw, const int32_t* cand_slot,
                         int ncand, const tb_sim3_params* prm, int min_consensus, const tb_sim3_out* out) {
    TB_ENTER((st ? st->ctx : nullptr));
    if (!st) return TB_EINVAL;
    tb_ctx* ctx = st->ctx;
    if (!K || !q_map_points || !q_mp_valid || !q_Tcw || !prm || !tb_sim3_params_ok(prm) || min_consensus < 0 || !(K[0] > 0.0) || !(K[1] > 0.0) ||
        !std::isfinite(K[0]) || !std::isfinite(K[1]) || !std::isfinite(K[2]) || !std::isfinite(K[3]))
        return tb_fail(ctx, TB_EINVAL, "tb_kf_store_sim3_dev: null arguments, the Sim(3) parameters (hypotheses 1..1024, fixed_scale 0 or 1, chi2_max), "
                                       "min_consensus %d or K", min_consensus);
    float inv_sigma2[TB_MAX_LEVELS];
    int rc;
    if ((rc = reloc_check(st, "tb_kf_store_sim3_dev", nlevels, scale, q_keys, q_counts, q_pitch, cand_slot, ncand, inv_sigma2))) return rc;
    if (!st->reloc_done) return tb_fail(ctx, TB_ESTATE, "tb_kf_store_sim3_dev: no verification (tb_relocalize_batch_dev) has filled the match lists");
    if (ncand != st->reloc_ncand)
        return tb_fail(ctx, TB_EINVAL, "tb_kf_store_sim3_dev: ncand %d, but the match lists were filled for %d candidates a sequence", ncand, st->reloc_ncand);
    if (!st->s3_ready) {   /* the first call allocates, later ones do not */
        const size_t pairs = (size_t)st->nseq * st->max_cand, pp = pairs * st->pitch;
        /* a buffer is allocated only while its pointer is null, so a call that failed half way is finished by the next one */
        if (!st->s3_rows) TB_TRY(tb_dev_alloc(ctx, st->own, &st->s3_rows, pp));
        if (!st->s3_mask) TB_TRY(tb_dev_alloc(ctx, st->own, &st->s3_mask, pp, 0));
        if (!st->s3_cnt) TB_TRY(tb_dev_alloc(ctx, st->own, &st->s3_cnt, pairs, 0));
        if (!st->s3_kf) TB_TRY(tb_dev_alloc(ctx, st->own, &st->s3_kf, pairs));
        if (!st->s3_cons) TB_TRY(tb_dev_alloc(ctx, st->own, &st->s3_cons, pairs));
        if (!st->s3_flags) TB_TRY(tb_dev_alloc(ctx, st->own, &st->s3_flags, pairs));
        if (!st->s3_S12) TB_TRY(tb_dev_alloc(ctx, st->own, &st->s3_S12, pairs * 16));
        if (!st->s3_srt) TB_TRY(tb_dev_alloc(ctx, st->own, &st->s3_srt, pairs * 8));
        if (!st->s3_best_kf) TB_TRY(tb_dev_alloc(ctx, st->own, &st->s3_best_kf, (size_t)st->nseq));
        if (!st->s3_best_srt) TB_TRY(tb_dev_alloc(ctx, st->own, &st->s3_best_srt, (size_t)st->nseq * 8));
        st->s3_ready = true;
    }
    static const tb_sim3_out none = {};
    const tb_sim3_out& o = out ? *out : none;
    const int pairs = st->nseq * ncand;
    int32_t* cons = o.cand_consensus ? o.cand_consensus : st->s3_cons;
    float* S12 = o.cand_S12 ? o.cand_S12 : st->s3_S12;
    double* srt = o.cand_srt ? o.cand_srt : st->s3_srt;
    TB_TRY(tbk_sim3_rows(ctx, pairs, ncand, st->cap, cand_slot, st->kf_ids, q_keys, q_counts, q_map_points, q_mp_valid, q_pitch, q_Tcw,
                         st->matches, st->mcounts, st->keys, st->mp, st->valid, st->counts, st->Tcw, st->pitch, inv_sigma2, nlevels, st->s3_rows,
                         st->s3_cnt, st->s3_kf, o.cand_rows));
    TB_TRY(tbk_sim3_batch(ctx, pairs, K, st->s3_rows, st->s3_cnt, st->pitch, prm->hypotheses, prm->fixed_scale, prm->chi2_max, prm->seed, S12, srt,
                          cons, st->s3_mask, nullptr, o.cand_flags ? o.cand_flags : st->s3_flags));
    st->s3_best = false;   /* tb_kf_store_sim3_graph_dev needs the winner this call selects, if it selects one */
    st->s3_done = true;    /* tb_kf_store_sim3_refine_dev may run; it is told where cand_srt and cand_consensus went */
    st->w3_use = false;    /* on this query's masks, not on the widened lists an earlier search left */
    st->s3_own_srt = !o.cand_srt;
    st->s3_own_cons = !o.cand_consensus;
    st->s3_min_cons = -1;
    if (!o.best_rank && !o.best_kf && !o.best_S12 && !o.best_srt) return TB_OK;
    TB_TRY(tbk_sim3_select(ctx, st->nseq, ncand, min_consensus, st->s3_kf, cons, S12, srt, o.best_rank, o.best_kf, o.best_S12, o.best_srt,
                           st->s3_best_kf, st->s3_best_srt));
    st->s3_best = true;
    st->s3_min_cons = min_consensus;
    return TB_OK;
}

int tb_kf_store_sim3_refine_dev(tb_kf_store* st, const double K[4], int nlevels, float scale, const tb_keypoint* q_keys, const int32_t* q_counts,
                                const float* q_map_points, const uint8_t* q_mp_valid, int q_pitch, const float* q_Tcw, const int32_t* cand_slot,
                                int ncand, const double* cand_srt, const int32_t* cand_consensus, const tb_sim3_opt_params* prm, int min_inliers,
                                int use_for_graph, const tb_sim3_refine_out* out) {
    TB_ENTER((st ? st->ctx : nullptr));
    if (!st) return TB_EINVAL;
    tb_ctx* ctx = st->ctx;
    if (!K || !q_map_points || !q_mp_valid || !q_Tcw || !prm || !tb_sim3_opt_params_ok(prm) || prm->min_keep < 1 || min_inliers < 0 ||
        (use_for_graph != 0 && use_for_graph != 1) || !(K[0] > 0.0) || !(K[1] > 0.0) || !std::isfinite(K[0]) || !std::isfinite(K[1]) ||
        !std::isfinite(K[2]) || !std::isfinite(K[3]))
        return tb_fail(ctx, TB_EINVAL, "tb_kf_store_sim3_refine_dev: null arguments, the optimiser's parameters (th2, iteration counts 0..99, "
                                       "min_keep >= 1, fixed_scale 0 or 1), min_inliers %d, use_for_graph %d (0, 1) or K", min_inliers, use_for_graph);
    float inv_sigma2[TB_MAX_LEVELS];
    int rc;
    if ((rc = reloc_check(st, "tb_kf_store_sim3_refine_dev", nlevels, scale, q_keys, q_counts, q_pitch, cand_slot, ncand, inv_sigma2))) return rc;
    if (!st->s3_ready || !st->s3_done || !st->reloc_done)
        return tb_fail(ctx, TB_ESTATE, "tb_kf_store_sim3_refine_dev: no tb_kf_store_sim3_dev since the store was made or cleared or the last verification");
    if (ncand != st->reloc_ncand)
        return tb_fail(ctx, TB_EINVAL, "tb_kf_store_sim3_refine_dev: ncand %d, but the match lists were filled for %d candidates a sequence", ncand, st->reloc_ncand);
    if ((!cand_srt && !st->s3_own_srt) || (!cand_consensus && !st->s3_own_cons))
        return tb_fail(ctx, TB_ESTATE, "tb_kf_store_sim3_refine_dev: the Sim(3) query wrote cand_srt / cand_consensus to the caller's buffer: pass it");
    static const tb_sim3_refine_out none = {};
    const tb_sim3_refine_out& o = out ? *out : none;
    const bool wants_best = o.best_srt || o.best_S12 || o.best_inliers || o.best_stats || use_for_graph;
    if (wants_best && !st->s3_best)
        return tb_fail(ctx, TB_ESTATE, "tb_kf_store_sim3_refine_dev: the Sim(3) query selected no candidate (it was given no best_* output)");
    if (!st->o3_ready) {   /* the first call allocates, later ones do not */
        const size_t pairs = (size_t)st->nseq * st->max_cand, pp = pairs * st->pitch;
        if (!st->o3_rows) TB_TRY(tb_dev_alloc(ctx, st->own, &st->o3_rows, pp));
        if (!st->o3_mask) TB_TRY(tb_dev_alloc(ctx, st->own, &st->o3_mask, pp, 0));
        if (!st->o3_cnt) TB_TRY(tb_dev_alloc(ctx, st->own, &st->o3_cnt, pairs, 0));
        if (!st->o3_kf) TB_TRY(tb_dev_alloc(ctx, st->own, &st->o3_kf, pairs));
        if (!st->o3_run) TB_TRY(tb_dev_alloc(ctx, st->own, &st->o3_run, pairs, 0));
        if (!st->o3_inl) TB_TRY(tb_dev_alloc(ctx, st->own, &st->o3_inl, pairs));
        if (!st->o3_seed) TB_TRY(tb_dev_alloc(ctx, st->own, &st->o3_seed, pairs * 8));
        if (!st->o3_srt) TB_TRY(tb_dev_alloc(ctx, st->own, &st->o3_srt, pairs * 8));
        if (!st->o3_stats) TB_TRY(tb_dev_alloc(ctx, st->own, &st->o3_stats, pairs * 8));
        if (!st->o3_S12) TB_TRY(tb_dev_alloc(ctx, st->own, &st->o3_S12, pairs * 16));
        st->o3_ready = true;
    }
    const int pairs = st->nseq * ncand;
    const double* seeds = cand_srt ? cand_srt : st->s3_srt;
    const int32_t* cons = cand_consensus ? cand_consensus : st->s3_cons;
    /* after a search with use_for_refine: the widened lists through the same row kernel, every row active (ORB-SLAM hands
     * OptimizeSim3 the RANSAC's inliers and SearchBySim3's pairs) */
    const bool wide = st->w3_use;
    if (wide && q_pitch != st->w3_qpitch)
        return tb_fail(ctx, TB_EINVAL, "tb_kf_store_sim3_refine_dev: query pitch %d, but the search whose lists it refines ran with %d", q_pitch,
                       st->w3_qpitch);
    TB_TRY(tbk_sim3_obs_rows(ctx, pairs, ncand, st->cap, cand_slot, st->kf_ids, q_keys, q_counts, q_map_points, q_mp_valid, q_pitch, q_Tcw,
                             wide ? st->w3_wide : st->matches, wide ? st->w3_wcnt : st->mcounts, st->keys, st->mp, st->valid, st->counts, st->Tcw,
                             st->pitch, inv_sigma2, nlevels, st->o3_rows, st->o3_cnt, st->o3_kf));
    TB_TRY(tbk_sim3_refine_prep(ctx, pairs, st->o3_kf, cons, seeds, st->o3_cnt, st->o3_run, st->o3_seed));
    TB_TRY(tbk_sim3_opt_batch(ctx, pairs, K, st->o3_rows, st->o3_run, st->pitch, wide ? st->w3_ones : st->s3_mask, st->o3_seed, prm, st->o3_srt,
                              st->o3_S12, st->o3_inl, st->o3_mask, st->o3_stats));
    st->o3_wide = wide;
    return tbk_sim3_refine_select(ctx, st->nseq, ncand, st->s3_best ? st->s3_min_cons : -1, min_inliers, use_for_graph, st->o3_kf, cons, st->o3_srt,
                                  st->o3_S12, st->o3_inl, st->o3_stats, o.cand_srt, o.cand_S12, o.cand_inliers, o.cand_stats, o.best_srt,
                                  o.best_S12, o.best_inliers, o.best_stats, st->s3_best_srt);
}

int tb_kf_store_sim3_refine_state_dev(tb_kf_store* st, const tb_sim3_obs_row** rows, const int32_t** row_counts, const uint8_t** active,
                                      const uint8_t** inlier) {
    if (!st) return TB_EINVAL;
    if (!st->o3_ready) return tb_fail(st->ctx, TB_ESTATE, "tb_kf_store_sim3_refine_state_dev: before the first tb_kf_store_sim3_refine_dev");
    if (rows) *rows = st->o3_rows;
    if (row_counts) *row_counts = st->o3_cnt;
    if (active) *active = st->o3_wide ? st->w3_ones : st->s3_mask;
    if (inlier) *inlier = st->o3_mask;
    return TB_OK;
}

int tb_kf_store_sim3_search_dev(tb_kf_store* st, const double K[4], int width, int height, int nlevels, float scale, const tb_keypoint* q_keys,
                                const uint8_t* q_desc, const int32_t* q_counts, const float* q_map_points, const uint8_t* q_mp_valid, int q_pitch,
                                const float* q_Tcw, const int32_t* cand_slot, int ncand, const double* cand_srt, const int32_t* cand_consensus,
                                float th, int th_high, int use_for_refine, const tb_sim3_search_out* out) {
    TB_ENTER((st ? st->ctx : nullptr));
    if (!st) return TB_EINVAL;
    tb_ctx* ctx = st->ctx;
    if (!K || !q_desc || !q_map_points || !q_mp_valid || !q_Tcw || !(th > 0.f) || !std::isfinite(th) || th_high < 0 || th_high > 256 ||
        width < 1 || height < 1 || !(scale > 0.f) || (use_for_refine != 0 && use_for_refine != 1) || !(K[0] > 0.0) || !(K[1] > 0.0) ||
        !std::isfinite(K[0]) || !std::isfinite(K[1]) || !std::isfinite(K[2]) || !std::isfinite(K[3]))
        return tb_fail(ctx, TB_EINVAL, "tb_kf_store_sim3_search_dev: null arguments, th (positive), th_high %d (0..256), image %d x %d, scale "
                                       "(positive), use_for_refine %d (0, 1) or K", th_high, width, height, use_for_refine);
    float inv_sigma2[TB_MAX_LEVELS];
    int rc;
    if ((rc = reloc_check(st, "tb_kf_store_sim3_search_dev", nlevels, scale, q_keys, q_counts, q_pitch, cand_slot, ncand, inv_sigma2))) return rc;
    if (!st->s3_ready || !st->s3_done || !st->reloc_done)
        return tb_fail(ctx, TB_ESTATE, "tb_kf_store_sim3_search_dev: no tb_kf_store_sim3_dev since the store was made or cleared or the last verification");
    if (ncand != st->reloc_ncand)
        return tb_fail(ctx, TB_EINVAL, "tb_kf_store_sim3_search_dev: ncand %d, but the match lists were filled for %d candidates a sequence", ncand, st->reloc_ncand);
    if ((!cand_srt && !st->s3_own_srt) || (!cand_consensus && !st->s3_own_cons))
        return tb_fail(ctx, TB_ESTATE, "tb_kf_store_sim3_search_dev: the Sim(3) query wrote cand_srt / cand_consensus to the caller's buffer: pass it");
    static const tb_sim3_search_out none = {};
    const tb_sim3_search_out& o = out ? *out : none;
    if ((o.best_new || o.best_total) && !st->s3_best)
        return tb_fail(ctx, TB_ESTATE, "tb_kf_store_sim3_search_dev: the Sim(3) query selected no candidate (it was given no best_* output)");
    if (!st->w3_ready) {   /* the first call allocates, later ones do not */
        const size_t pairs = (size_t)st->nseq * st->max_cand, pp = pairs * st->pitch;
        if (!st->w3_pts1) TB_TRY(tb_dev_alloc(ctx, st->own, &st->w3_pts1, pp * 3));
        if (!st->w3_pts2) TB_TRY(tb_dev_alloc(ctx, st->own, &st->w3_pts2, pp * 3));
        if (!st->w3_m1) TB_TRY(tb_dev_alloc(ctx, st->own, &st->w3_m1, pp));
        if (!st->w3_m2) TB_TRY(tb_dev_alloc(ctx, st->own, &st->w3_m2, pp));
        if (!st->w3_ones) TB_TRY(tb_dev_alloc(ctx, st->own, &st->w3_ones, pp, 1));
        if (!st->w3_wink) TB_TRY(tb_dev_alloc(ctx, st->own, &st->w3_wink, pp));
        if (!st->w3_match1) TB_TRY(tb_dev_alloc(ctx, st->own, &st->w3_match1, pp, 0xff));
        if (!st->w3_match2) TB_TRY(tb_dev_alloc(ctx, st->own, &st->w3_match2, pp, 0xff));
        if (!st->w3_pairs) TB_TRY(tb_dev_alloc(ctx, st->own, &st->w3_pairs, pp));
        if (!st->w3_wide) TB_TRY(tb_dev_alloc(ctx, st->own, &st->w3_wide, pp));
        if (!st->w3_pcnt) TB_TRY(tb_dev_alloc(ctx, st->own, &st->w3_pcnt, pairs, 0));
        if (!st->w3_wcnt) TB_TRY(tb_dev_alloc(ctx, st->own, &st->w3_wcnt, pairs, 0));
        if (!st->w3_skip) TB_TRY(tb_dev_alloc(ctx, st->own, &st->w3_skip, pairs));
        if (!st->w3_f1) TB_TRY(tb_dev_alloc(ctx, st->own, &st->w3_f1, pairs));
        if (!st->w3_f2) TB_TRY(tb_dev_alloc(ctx, st->own, &st->w3_f2, pairs));
        if (!st->w3_stats) TB_TRY(tb_dev_alloc(ctx, st->own, &st->w3_stats, pairs * 8));
        st->w3_ready = true;
    }
    const int pairs = st->nseq * ncand;
    const double* srt = cand_srt ? cand_srt : st->s3_srt;
    const int32_t* cons = cand_consensus ? cand_consensus : st->s3_cons;
    float sf[TB_MAX_LEVELS], px[TB_MAX_LEVELS];
    TB_TRY(tb_scale_factors(nlevels, scale, sf, px, nullptr, nullptr));
    st->w3_use = false;   /* the lists it referred to are overwritten from here on */
    TB_TRY(tbk_sim3_search_prep(ctx, pairs, ncand, st->cap, cand_slot, st->kf_ids, q_counts, q_map_points, q_mp_valid, q_pitch, q_Tcw, st->matches,
                                st->mcounts, st->mp, st->valid, st->counts, st->Tcw, st->pitch, cons, st->s3_mask, st->w3_pts1, st->w3_pts2,
                                st->w3_m1, st->w3_m2, st->w3_wink, st->w3_skip, st->w3_f1, st->w3_f2));
    /* side 1 = the query frame s, side 2 = the stored keyframe s * cap + slot, both read where they lie */
    const tbk_sim3_search_side s1 = {q_keys, q_desc, q_mp_valid, q_counts, st->w3_f1, st->w3_pts1, st->w3_m1, q_pitch};
    const tbk_sim3_search_side s2 = {st->keys, st->desc, st->valid, st->counts, st->w3_f2, st->w3_pts2, st->w3_m2, st->pitch};
    TB_TRY(tbk_sim3_search_batch(ctx, pairs, K, width, height, nlevels, px, &s1, &s2, srt, st->w3_skip, th, th_high, st->w3_match1, st->w3_match2,
                                 st->w3_pairs, st->pitch, st->w3_pcnt, st->w3_stats));
    TB_TRY(tbk_sim3_search_merge(ctx, st->nseq, ncand, st->s3_best ? st->s3_min_cons : -1, q_counts, q_pitch, st->pitch, st->matches, st->w3_wink,
                                 st->w3_skip, st->w3_match1, st->w3_match2, st->w3_pairs, st->w3_pcnt, st->w3_stats, st->s3_kf, cons, st->w3_wide,
                                 st->w3_wcnt, o.cand_new, o.cand_total, o.cand_stats, o.best_new, o.best_total));
    st->w3_qpitch = q_pitch;
    st->w3_use = use_for_refine == 1;
    return TB_OK;
}

int tb_kf_store_sim3_search_state_dev(tb_kf_store* st, const int32_t** match1, const int32_t** match2, const tb_match** pairs,
                                      const int32_t** pair_counts, const tb_match** widened, const int32_t** widened_counts, int* q_pitch) {
    if (!st) return TB_EINVAL;
    if (!st->w3_ready) return tb_fail(st->ctx, TB_ESTATE, "tb_kf_store_sim3_search_state_dev: before the first tb_kf_store_sim3_search_dev");
    if (match1) *match1 = st->w3_match1;
    if (match2) *match2 = st->w3_match2;
    if (pairs) *pairs = st->w3_pairs;
    if (pair_counts) *pair_counts = st->w3_pcnt;
    if (widened) *widened = st->w3_wide;
    if (widened_counts) *widened_counts = st->w3_wcnt;
    if (q_pitch) *q_pitch = st->w3_qpitch;
    return TB_OK;
}

int tb_kf_store_sim3_graph_run(tb_kf_store* st, const char* who, const float* q_Tcw, int frame_id, int iters, int fixed_scale, double w_rot,
                               double w_trans, double w_scale, tb_sim3_graph_out* out) {
    tb_ctx* ctx = st->ctx;
    const double w[3] = {w_rot, w_trans, w_scale};
    bool wok = true;
    for (double v : w) wok = wok && std::isfinite(v) && v >= 0.0;
    if (!q_Tcw || !out || iters < 0 || iters > 99 || (fixed_scale != 0 && fixed_scale != 1) || !wok)
        return tb_fail(ctx, TB_EINVAL, "%s: null arguments, iters %d (0..99), fixed_scale %d (0, 1) or a weight that is negative or not finite", who,
                       iters, fixed_scale);
    if (st->cap > 63) return tb_fail(ctx, TB_EINVAL, "%s: capacity %d, but a graph holds at most 64 nodes (capacity + 1)", who, st->cap);
    if (!st->s3_best)
        return tb_fail(ctx, TB_ESTATE, "%s: no tb_kf_store_sim3_dev has selected a winner (best_* outputs) since the store was made or cleared", who);
    const int S = st->nseq, cap = st->cap, nn = cap + 1;
    if (!st->g3_ready) {   /* the first call allocates and plans, later ones do not */
        const size_t SN = (size_t)S * nn;
        if (!st->g3_nnodes) TB_TRY(tb_dev_alloc(ctx, st->own, &st->g3_nnodes, (size_t)S, 0));
        if (!st->g3_ecount) TB_TRY(tb_dev_alloc(ctx, st->own, &st->g3_ecount, (size_t)S, 0));
        if (!st->g3_node_kf) TB_TRY(tb_dev_alloc(ctx, st->own, &st->g3_node_kf, SN));
        if (!st->g3_before) TB_TRY(tb_dev_alloc(ctx, st->own, &st->g3_before, SN * 8));
        if (!st->g3_after) TB_TRY(tb_dev_alloc(ctx, st->own, &st->g3_after, SN * 8));
        if (!st->g3_edges) TB_TRY(tb_dev_alloc(ctx, st->own, &st->g3_edges, SN));
        if (!st->g3_stats) TB_TRY(tb_dev_alloc(ctx, st->own, &st->g3_stats, (size_t)S * 8));
        TB_TRY(tb_pose_graph_sim3_plan(ctx, S, nn, 1, nn));
        st->g3_ready = true;
    }
    const int nlive = (int)std::min<long long>(st->nadded, cap), oldest = st->nadded >= cap ? (int)(st->nadded % cap) : 0;
    TB_TRY(tbk_sim3_graph(ctx, S, cap, nlive, oldest, frame_id, w_rot, w_trans, w_scale, st->Tcw, st->kf_ids, q_Tcw, st->s3_best_kf,
                          st->s3_best_srt, st->g3_before, st->g3_after, st->g3_node_kf, st->g3_nnodes, st->g3_edges, st->g3_ecount));
    TB_TRY(tb_pose_graph_sim3_batch_dev(ctx, S, nn, 1, fixed_scale, st->g3_after, st->g3_edges, st->g3_ecount, nn, iters, st->g3_stats));
    out->nn = nn;
    out->nnodes = st->g3_nnodes; out->node_kf = st->g3_node_kf; out->before = st->g3_before; out->after = st->g3_after;
    out->edges = st->g3_edges; out->edge_counts = st->g3_ecount; out->stats = st->g3_stats;
    return TB_OK;
}

int tb_kf_store_sim3_graph_dev(tb_kf_store* st, const float* q_Tcw, int iters, int fixed_scale, double w_rot, double w_trans, double w_scale,
                               tb_sim3_graph_out* out) {
    TB_ENTER((st ? st->ctx : nullptr));
    if (!st) return TB_EINVAL;
    return tb_kf_store_sim3_graph_run(st, "tb_kf_store_sim3_graph_dev", q_Tcw, -2, iters, fixed_scale, w_rot, w_trans, w_scale, out);
}

int tb_kf_store_sim3_state_dev(tb_kf_store* st, const tb_sim3_row** rows, const int32_t** row_counts, const uint8_t** inlier) {
    if (!st) return TB_EINVAL;
    if (!st->s3_ready) return tb_fail(st->ctx, TB_ESTATE, "tb_kf_store_sim3_state_dev: before the first tb_kf_store_sim3_dev");
    if (rows) *rows = st->s3_rows;
    if (row_counts) *row_counts = st->s3_cnt;
    if (inlier) *inlier = st->s3_mask;
    return TB_OK;
}

int tb_bow_transform(tb_ctx* ctx, const tb_vocab* voc, const uint8_t* desc, int n, int levelsup, int32_t* word_ids, double* weights,
                     int32_t* node_ids) {
    TB_ENTER(ctx);
    if (!ctx || !voc || voc->ctx != ctx || n < 0 || levelsup < 0 || (n && (!desc || !word_ids || !weights || !node_ids))) return TB_EINVAL;
    if (n == 0) return TB_OK;
    size_t end = 0;
    const size_t oD = stage_piece(end, (size_t)n * 32), oW = stage_piece(end, (size_t)n * 4), oN = stage_piece(end, (size_t)n * 4),
                 oWt = stage_piece(end, (size_t)n * 8);
    char* b;
    int rc;
    if ((rc = tb_scratch(ctx, TB_SLOT_HOST, end, (void**)&b))) return rc;
    TB_UPLOAD(ctx, b + oD, desc, (size_t)n * 32);
    if ((rc = tb_bow_transform_batch_dev(ctx, voc, 1, (const uint8_t*)(b + oD), nullptr, n, levelsup, (int32_t*)(b + oW), (int32_t*)(b + oN),
                                         (double*)(b + oWt), nullptr, nullptr)))
        return rc;
    TB_DOWNLOAD(ctx, word_ids, b + oW, (size_t)n * 4);
    TB_DOWNLOAD(ctx, node_ids, b + oN, (size_t)n * 4);
    TB_DOWNLOAD(ctx, weights, b + oWt, (size_t)n * 8);
    TB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return TB_OK;
}

int tb_search_by_bow_batch_dev(tb_ctx* ctx, int npairs, const tb_keypoint* k1, const uint8_t* d1, int pitch1, const uint64_t* fv1,
                               const int32_t* fv_counts1, const tb_keypoint* k2, const uint8_t* d2, int pitch2, const uint64_t* fv2,
                               const int32_t* fv_counts2, const uint8_t* has_mp2, int map_point_only, int th_low, float nratio,
                               int histo_len, int check_orientation, tb_match* out, int cap, int32_t* out_counts, int32_t* flags) {
    TB_ENTER(ctx);
    if (!ctx || npairs < 0 || pitch1 < 1 || pitch2 < 1 || histo_len < 1 || histo_len > 1024 || cap < 0) return TB_EINVAL;
    if (npairs == 0) return TB_OK;
    if (!k1 || !d1 || !fv1 || !fv_counts1 || !k2 || !d2 || !fv2 || !fv_counts2 || !out_counts || !flags || (cap && !out)) return TB_EINVAL;
    void* best;
    int rc;
    if ((rc = tb_scratch(ctx, TB_SLOT_WORK, (size_t)npairs * pitch1 * 16, &best))) return rc;
    return tbk_bow_search_batch(ctx, npairs, k1, d1, pitch1, (const unsigned long long*)fv1, fv_counts1, k2, d2, pitch2,
                                (const unsigned long long*)fv2, fv_counts2, has_mp2, map_point_only, th_low, nratio, histo_len,
                                check_orientation, out, cap, out_counts, flags, (int32_t*)best);
}

int tb_stereo_tracks_to_obs_batch_dev(tb_ctx* ctx, int nframes, const tb_keypoint* keys_left, const tb_keypoint* keys_right,
                                      int key_pitch, const tb_match* matches, const int32_t* match_counts, int match_pitch,
                                      const float K[4], float bf, const float* inv_sigma2, int nlevels, tb_obs* obs, int obs_pitch,
                                      int32_t* obs_counts) {
    TB_ENTER(ctx);
    if (!ctx || nframes < 0 || !K || !inv_sigma2 || nlevels < 1 || nlevels > TB_MAX_LEVELS || key_pitch < 1 || match_pitch < 1 || obs_pitch < 1)
        return TB_EINVAL;
    if (nframes == 0) return TB_OK;
    if (!keys_left || !keys_right || !matches || !match_counts || !obs || !obs_counts) return TB_EINVAL;
    void* dsig;
    int rc;
    if ((rc = tb_scratch(ctx, TB_SLOT_STEREO_SIGMA, TB_MAX_LEVELS * sizeof(float), &dsig))) return rc;
    /* the table is a few floats of host memory: staged through a pinned-free async copy (the stream orders it before the kernel) */
    TB_HIP(ctx, hipMemcpyAsync(dsig, inv_sigma2, (size_t)nlevels * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    return tbk_stereo_obs(ctx, nframes, keys_left, keys_right, key_pitch, matches, match_counts, match_pitch, K, bf, (const float*)dsig, nlevels,
                          obs, obs_pitch, obs_counts);
}

int tb_search_by_violence(tb_ctx* ctx, const tb_keypoint* k1, const uint8_t* d1, int n1, const tb_keypoint* k2,
                          const uint8_t* d2, int n2, int img2_width, int img2_height, int min_level, int max_level,
                          float radius, int th_low, float nratio, int histo_len, int check_orientation, tb_match* out,
                          int cap, int* count) {
    TB_ENTER(ctx);
    if (!ctx || !count || n1 < 0 || n2 < 0 || histo_len < 1 || histo_len > 1024 || img2_width < 1 || img2_height < 1) return TB_EINVAL;
    *count = 0;
    if (n1 == 0) return TB_OK;
    if ((n1 && (!k1 || !d1)) || (n2 && (!k2 || !d2))) return TB_EINVAL;
    const size_t p2 = (size_t)std::max(n2, 1), kb = sizeof(tb_keypoint);
    size_t end = 0;
    const size_t oK1 = stage_piece(end, n1 * kb), oD1 = stage_piece(end, (size_t)n1 * 32), oK2 = stage_piece(end, p2 * kb),
                 oD2 = stage_piece(end, p2 * 32), oCs = stage_piece(end, (TB_GRID_CELLS + 1) * 4), oCi = stage_piece(end, p2 * 4),
                 oOut = stage_piece(end, (size_t)n1 * sizeof(tb_match)), oCnt = stage_piece(end, 16);
    char* b;
    int rc;
    if ((rc = tb_scratch(ctx, TB_SLOT_HOST, end, (void**)&b))) return rc;
    const int32_t cnt[4] = {n1, n2, 0, 0}; /* n1, n2, then the match count and flag */
    int32_t* dcnt = (int32_t*)(b + oCnt);
    TB_UPLOAD(ctx, b + oK1, k1, n1 * kb);
    TB_UPLOAD(ctx, b + oD1, d1, (size_t)n1 * 32);
    TB_UPLOAD(ctx, b + oK2, k2, n2 * kb);
    TB_UPLOAD(ctx, b + oD2, d2, (size_t)n2 * 32);
    TB_UPLOAD(ctx, dcnt, cnt, sizeof cnt);
    const tb_keypoint *dk1 = (const tb_keypoint*)(b + oK1), *dk2 = (const tb_keypoint*)(b + oK2);
    if ((rc = tbk_grid_build_batch(ctx, 1, dk2, dcnt + 1, (int)p2, img2_width, img2_height, (int32_t*)(b + oCs), (int32_t*)(b + oCi))))
        return rc;
    if ((rc = tb_search_by_violence_batch_dev(ctx, 1, dk1, (const uint8_t*)(b + oD1), dcnt, n1, dk2, (const uint8_t*)(b + oD2), dcnt + 1,
                                              (int)p2, (const int32_t*)(b + oCs), (const int32_t*)(b + oCi), img2_width, img2_height,
                                              min_level, max_level, radius, th_low, nratio, histo_len, check_orientation,
                                              (tb_match*)(b + oOut), n1, dcnt + 2, dcnt + 3)))
        return rc;
    return match_tail(ctx, (const tb_match*)(b + oOut), dcnt + 2, cap, out, count);
}

/* one DBoW2 feature vector (CSR: nodes, start, items) as the batched form's key list (node << 32) | feature, nodes ascending and a
 * node's features in CSR order. With `other` (F2's nodes), F1's nodes that F2 lacks are left out: they can match nothing. */
static int bow_keys(tb_ctx* ctx, const char* frame, const uint32_t* nodes, const int32_t* start, const uint32_t* items, int nn, int n,
                    const uint32_t* other, int nother, std::vector<uint64_t>& keys) {
    for (int a = 0; a < nn; a++) {
        if (a && nodes[a] <= nodes[a - 1]) return tb_fail(ctx, TB_EINVAL, "searchByBow: node ids of %s not strictly ascending", frame);
        if (start[a] < 0 || start[a + 1] < start[a]) return tb_fail(ctx, TB_EINVAL, "searchByBow: feature vector offsets");
        if (other && !std::binary_search(other, other + nother, nodes[a])) continue;
        for (int p = start[a]; p < start[a + 1]; p++) {
            if (items[p] >= (uint32_t)n) return tb_fail(ctx, TB_EINVAL, "searchByBow: feature index %u of %s out of range", items[p], frame);
            keys.push_back((uint64_t)nodes[a] << 32 | items[p]);
        }
    }
    return TB_OK;
}

/* ---- Matcher::searchByBow (matcher.cpp:619-721). The two frames' DBoW2 feature vectors are inputs. */
int tb_search_by_bow(tb_ctx* ctx, const tb_keypoint* k1, const uint8_t* d1, int n1, const uint32_t* nodes1, const int32_t* start1,
                     const uint32_t* items1, int nn1, const tb_keypoint* k2, const uint8_t* d2, int n2, const uint8_t* has_mp2,
                     const uint32_t* nodes2, const int32_t* start2, const uint32_t* items2, int nn2, int map_point_only, int th_low,
                     float nratio, int histo_len, int check_orientation, tb_match* out, int cap, int* count) {
    TB_ENTER(ctx);
    if (!ctx || !count || n1 < 0 || n2 < 0 || nn1 < 0 || nn2 < 0 || histo_len < 1 || histo_len > 1024 || cap < 0) return TB_EINVAL;
    *count = 0;
    if ((nn1 && (!nodes1 || !start1)) || (nn2 && (!nodes2 || !start2)) || (n1 && (!k1 || !d1)) || (n2 && (!k2 || !d2))) return TB_EINVAL;
    std::vector<uint64_t> fv1, fv2;
    int rc;
    if ((rc = bow_keys(ctx, "F2", nodes2, start2, items2, nn2, n2, nullptr, 0, fv2))) return rc;
    if ((rc = bow_keys(ctx, "F1", nodes1, start1, items1, nn1, n1, nodes2, nn2, fv1))) return rc;
    if (fv1.empty()) return TB_OK;
    /* a feature listed under two nodes is queried twice: the pitches cover both the keys and the lists */
    const int nq = (int)fv1.size(), nf2 = (int)fv2.size();
    const size_t p1 = (size_t)std::max(n1, nq), p2 = (size_t)std::max({n2, nf2, 1}), kb = sizeof(tb_keypoint);
    size_t end = 0;
    const size_t oK1 = stage_piece(end, p1 * kb), oD1 = stage_piece(end, p1 * 32), oF1 = stage_piece(end, p1 * 8),
                 oK2 = stage_piece(end, p2 * kb), oD2 = stage_piece(end, p2 * 32), oF2 = stage_piece(end, p2 * 8),
                 oMp = stage_piece(end, p2), oOut = stage_piece(end, (size_t)nq * sizeof(tb_match)), oCnt = stage_piece(end, 16);
    char* b;
    if ((rc = tb_scratch(ctx, TB_SLOT_HOST, end, (void**)&b))) return rc;
    const int32_t cnt[4] = {nq, nf2, 0, 0}; /* list lengths, then the match count and flag */
    int32_t* dcnt = (int32_t*)(b + oCnt);
    TB_UPLOAD(ctx, b + oK1, k1, n1 * kb);
    TB_UPLOAD(ctx, b + oD1, d1, (size_t)n1 * 32);
    TB_UPLOAD(ctx, b + oF1, fv1.data(), (size_t)nq * 8);
    TB_UPLOAD(ctx, b + oK2, k2, n2 * kb);
    TB_UPLOAD(ctx, b + oD2, d2, (size_t)n2 * 32);
    TB_UPLOAD(ctx, b + oF2, fv2.data(), (size_t)nf2 * 8);
    if (has_mp2) TB_UPLOAD(ctx, b + oMp, has_mp2, (size_t)n2);
    TB_UPLOAD(ctx, dcnt, cnt, sizeof cnt);
    if ((rc = tb_search_by_bow_batch_dev(ctx, 1, (const tb_keypoint*)(b + oK1), (const uint8_t*)(b + oD1), (int)p1, (const uint64_t*)(b + oF1),
                                         dcnt, (const tb_keypoint*)(b + oK2), (const uint8_t*)(b + oD2), (int)p2, (const uint64_t*)(b + oF2),
                                         dcnt + 1, has_mp2 ? (const uint8_t*)(b + oMp) : nullptr, map_point_only, th_low, nratio, histo_len,
                                         check_orientation, (tb_match*)(b + oOut), nq, dcnt + 2, dcnt + 3)))
        return rc;
    return match_tail(ctx, (const tb_match*)(b + oOut), dcnt + 2, cap, out, count);
}

/* ---- Matcher::searchByProjection, both overloads (matcher.cpp:406-617). F1 staged with its lookup grid,
 * the nq map points (k2: their keys, frame overload only) after it. */
static int projection_host(tb_ctx* ctx, int map_mode, const float Tcw1[16], const tb_camera* cam1, int img1_w, int img1_h,
                           const tb_keypoint* k1, const uint8_t* d1, const uint8_t* taken1, int n1, const tb_keypoint* k2,
                           const tb_mappoint* mps, const uint8_t* mp_desc, int nq, const float* sf, int nlevels, float nratio,
                           float radio, int th_high, int histo_len, int check_orientation, tb_match* out, int cap, int* count) {
    const size_t p1 = (size_t)std::max(n1, 1), kb = sizeof(tb_keypoint);
    size_t end = 0;
    const size_t oT = stage_piece(end, 64), oK1 = stage_piece(end, p1 * kb), oD1 = stage_piece(end, p1 * 32), oTk = stage_piece(end, p1),
                 oCs = stage_piece(end, (TB_GRID_CELLS + 1) * 4), oCi = stage_piece(end, p1 * 4), oK2 = stage_piece(end, k2 ? nq * kb : 0),
                 oMp = stage_piece(end, nq * sizeof(tb_mappoint)), oMd = stage_piece(end, (size_t)nq * 32),
                 oOut = stage_piece(end, (size_t)nq * sizeof(tb_match)), oCnt = stage_piece(end, 16);
    char* b;
    int rc;
    if ((rc = tb_scratch(ctx, TB_SLOT_HOST, end, (void**)&b))) return rc;
    const int32_t cnt[4] = {n1, nq, 0, 0}; /* n1, map points, then the match count and flag */
    int32_t* dcnt = (int32_t*)(b + oCnt);
    TB_UPLOAD(ctx, b + oT, Tcw1, 64);
    TB_UPLOAD(ctx, b + oK1, k1, n1 * kb);
    TB_UPLOAD(ctx, b + oD1, d1, (size_t)n1 * 32);
    if (taken1) TB_UPLOAD(ctx, b + oTk, taken1, (size_t)n1);
    else TB_HIP(ctx, hipMemsetAsync(b + oTk, 0, p1, ctx->stream));
    if (k2) TB_UPLOAD(ctx, b + oK2, k2, nq * kb);
    TB_UPLOAD(ctx, b + oMp, mps, nq * sizeof(tb_mappoint));
    TB_UPLOAD(ctx, b + oMd, mp_desc, (size_t)nq * 32);
    TB_UPLOAD(ctx, dcnt, cnt, sizeof cnt);
    const tb_keypoint* dk1 = (const tb_keypoint*)(b + oK1);
    const int32_t *cs = (const int32_t*)(b + oCs), *ci = (const int32_t*)(b + oCi);
    if ((rc = tbk_grid_build_batch(ctx, 1, dk1, dcnt, (int)p1, img1_w, img1_h, (int32_t*)(b + oCs), (int32_t*)(b + oCi)))) return rc;
    auto run = [&](int check) {
        const float* dT = (const float*)(b + oT);
        const uint8_t *dd1 = (const uint8_t*)(b + oD1), *dtk = (const uint8_t*)(b + oTk), *dmd = (const uint8_t*)(b + oMd);
        const tb_mappoint* dmp = (const tb_mappoint*)(b + oMp);
        tb_match* dout = (tb_match*)(b + oOut);
        if (map_mode)
            return tb_search_by_projection_map_batch_dev(ctx, 1, dT, cam1, img1_w, img1_h, dk1, dd1, dtk, dcnt, (int)p1, cs, ci, dmp, dmd,
                                                         dcnt + 1, nq, nq, sf, nlevels, nratio, radio, th_high, dout, nq, dcnt + 2, dcnt + 3);
        return tb_search_by_projection_batch_dev(ctx, 1, dT, cam1, img1_w, img1_h, dk1, dd1, dtk, dcnt, (int)p1, cs, ci,
                                                 (const tb_keypoint*)(b + oK2), dmp, dmd, dcnt + 1, nq, sf, nlevels, nratio, th_high,
                                                 histo_len, check, dout, nq, dcnt + 2, dcnt + 3);
    };
    if ((rc = run(check_orientation))) return rc;
    rc = match_tail(ctx, (const tb_match*)(b + oOut), dcnt + 2, cap, out, count);
    if (rc == TB_EUNSUPPORTED && check_orientation) {
        /* the histogram's flag (2) overwrites the search's (1), but an octave outside the table is the error the host form
         * reports first: look again without the histogram */
        int32_t flag = 0;
        if (const int e = run(0)) return e;
        TB_HIP(ctx, hipMemcpyAsync(&flag, dcnt + 3, sizeof flag, hipMemcpyDeviceToHost, ctx->stream));
        TB_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (flag == 1) return tb_fail(ctx, TB_EINVAL, "searchByProjection: a key octave is outside the scale factors");
    }
    return rc;
}

int tb_search_by_projection(tb_ctx* ctx, const float Tcw1[16], const tb_camera* cam1, int img1_width, int img1_height,
                            const tb_keypoint* k1, const uint8_t* d1, const uint8_t* taken1, int n1, const tb_keypoint* k2,
                            const tb_mappoint* mp2, const uint8_t* mp2_desc, int n2, const float* scale_factors, int nlevels,
                            float nratio, int th_high, int histo_len, int check_orientation, tb_match* out, int cap, int* count) {
    TB_ENTER(ctx);
    if (!ctx || !count || !Tcw1 || !cam1 || n1 < 0 || n2 < 0 || histo_len < 1 || histo_len > 1024 || nlevels < 1 ||
        nlevels > TB_MAX_LEVELS * 2 || !scale_factors || img1_width < 1 || img1_height < 1)
        return TB_EINVAL;
    *count = 0;
    if (n2 == 0) return TB_OK;
    if ((n1 && (!k1 || !d1)) || !k2 || !mp2 || !mp2_desc) return TB_EINVAL;
    return projection_host(ctx, 0, Tcw1, cam1, img1_width, img1_height, k1, d1, taken1, n1, k2, mp2, mp2_desc, n2, scale_factors, nlevels,
                           nratio, 0.f, th_high, histo_len, check_orientation, out, cap, count);
}

int tb_search_by_projection_map(tb_ctx* ctx, const float Tcw1[16], const tb_camera* cam1, int img1_width, int img1_height,
                                const tb_keypoint* k1, const uint8_t* d1, const uint8_t* taken1, int n1, const tb_mappoint* mps,
                                const uint8_t* mp_desc, int nmp, const float* scale_factors, int nlevels, float nratio, float radio,
                                int th_high, tb_match* out, int cap, int* count) {
    TB_ENTER(ctx);
    if (!ctx || !count || !Tcw1 || !cam1 || n1 < 0 || nmp < 0 || nlevels < 1 || nlevels > TB_MAX_LEVELS * 2 || !scale_factors ||
        img1_width < 1 || img1_height < 1)
        return TB_EINVAL;
    *count = 0;
    if (nmp == 0) return TB_OK;
    if ((n1 && (!k1 || !d1)) || !mps || !mp_desc) return TB_EINVAL;
    return projection_host(ctx, 1, Tcw1, cam1, img1_width, img1_height, k1, d1, taken1, n1, nullptr, mps, mp_desc, nmp, scale_factors,
                           nlevels, nratio, radio, th_high, 1, 0, out, cap, count);
}

/* ---- device-resident lookup grid + batched projection search */
int tb_frame_grid_batch_dev(tb_ctx* ctx, int nframes, const tb_keypoint* keys, const int32_t* counts, int key_pitch, int img_width,
                            int img_height, int32_t* cell_start, int32_t* cell_items) {
    TB_ENTER(ctx);
    if (!ctx || nframes < 0 || key_pitch < 1 || img_width < 1 || img_height < 1 || (nframes && (!keys || !counts || !cell_start || !cell_items)))
        return TB_EINVAL;
    return tbk_grid_build_batch(ctx, nframes, keys, counts, key_pitch, img_width, img_height, cell_start, cell_items);
}

int tb_search_by_projection_batch_dev(tb_ctx* ctx, int npairs, const float* Tcw1, const tb_camera* cam1, int img1_width,
                                      int img1_height, const tb_keypoint* k1, const uint8_t* d1, const uint8_t* taken1,
                                      const int32_t* n1, int pitch1, const int32_t* cell_start, const int32_t* cell_items,
                                      const tb_keypoint* k2, const tb_mappoint* mp2, const uint8_t* mp2_desc, const int32_t* n2,
                                      int pitch2, const float* scale_factors, int nlevels, float nratio, int th_high, int histo_len,
                                      int check_orientation, tb_match* out, int cap, int32_t* out_counts, int32_t* flags) {
    TB_ENTER(ctx);
    if (!ctx || npairs < 0 || !cam1 || !scale_factors || nlevels < 1 || nlevels > TB_MAX_LEVELS * 2 || histo_len < 1 || histo_len > 1024 ||
        pitch1 < 1 || pitch2 < 1 || cap < 0 || img1_width < 1 || img1_height < 1)
        return TB_EINVAL;
    if (npairs == 0) return TB_OK;
    if (!Tcw1 || !k1 || !d1 || !taken1 || !n1 || !cell_start || !cell_items || !k2 || !mp2 || !mp2_desc || !n2 || !out || !out_counts || !flags)
        return TB_EINVAL;
    void* dbest;
    int rc = tb_scratch(ctx, TB_SLOT_WORK, (size_t)npairs * pitch2 * 6 * sizeof(int32_t), &dbest);
    if (rc) return rc;
    return tbk_projection_batch(ctx, npairs, Tcw1, cam1, img1_width, img1_height, k1, d1, taken1, n1, pitch1, cell_start, cell_items, k2, mp2,
                                mp2_desc, n2, pitch2, scale_factors, nlevels, nratio, th_high, histo_len, check_orientation,
                                (int32_t*)dbest, out, cap, out_counts, flags, 0, 0.f, pitch2);
}

int tb_search_by_projection_map_batch_dev(tb_ctx* ctx, int npairs, const float* Tcw1, const tb_camera* cam1, int img1_width,
                                          int img1_height, const tb_keypoint* k1, const uint8_t* d1, const uint8_t* taken1,
                                          const int32_t* n1, int pitch1, const int32_t* cell_start, const int32_t* cell_items,
                                          const tb_mappoint* mps, const uint8_t* mp_desc, const int32_t* nmp, int mp_pitch,
                                          int max_nmp, const float* scale_factors, int nlevels, float nratio, float radio,
                                          int th_high, tb_match* out, int cap, int32_t* out_counts, int32_t* flags) {
    TB_ENTER(ctx);
    if (!ctx || npairs < 0 || !cam1 || !scale_factors || nlevels < 1 || nlevels > TB_MAX_LEVELS * 2 || pitch1 < 1 || mp_pitch < 0 ||
        max_nmp < 1 || (mp_pitch > 0 && mp_pitch < max_nmp) || cap < 0 || img1_width < 1 || img1_height < 1)
        return TB_EINVAL;
    if (npairs == 0) return TB_OK;
    if (!Tcw1 || !k1 || !d1 || !taken1 || !n1 || !cell_start || !cell_items || !mps || !mp_desc || !nmp || !out || !out_counts || !flags)
        return TB_EINVAL;
    void* dbest;
    int rc = tb_scratch(ctx, TB_SLOT_WORK, (size_t)npairs * max_nmp * 6 * sizeof(int32_t), &dbest);
    if (rc) return rc;
    return tbk_projection_batch(ctx, npairs, Tcw1, cam1, img1_width, img1_height, k1, d1, taken1, n1, pitch1, cell_start, cell_items,
                                nullptr, mps, mp_desc, nmp, mp_pitch, scale_factors, nlevels, nratio, th_high, 1, 0, (int32_t*)dbest, out,
                                cap, out_counts, flags, 1, radio, max_nmp);
}

int tb_search_by_violence_batch_dev(tb_ctx* ctx, int npairs, const tb_keypoint* k1, const uint8_t* d1, const int32_t* n1, int pitch1,
                                    const tb_keypoint* k2, const uint8_t* d2, const int32_t* n2, int pitch2,
                                    const int32_t* cell_start2, const int32_t* cell_items2, int img2_width, int img2_height,
                                    int min_level, int max_level, float radius, int th_low, float nratio, int histo_len,
                                    int check_orientation, tb_match* out, int cap, int32_t* out_counts, int32_t* flags) {
    TB_ENTER(ctx);
    if (!ctx || npairs < 0 || histo_len < 1 || histo_len > 1024 || pitch1 < 1 || pitch2 < 1 || cap < 0 || img2_width < 1 || img2_height < 1)
        return TB_EINVAL;
    if (npairs == 0) return TB_OK;
    if (!k1 || !d1 || !n1 || !k2 || !d2 || !n2 || !cell_start2 || !cell_items2 || !out || !out_counts || !flags) return TB_EINVAL;
    void* dbest;
    int rc = tb_scratch(ctx, TB_SLOT_WORK, (size_t)npairs * pitch1 * 4 * sizeof(int32_t), &dbest);
    if (rc) return rc;
    return tbk_violence_batch(ctx, npairs, k1, d1, n1, pitch1, k2, d2, n2, pitch2, cell_start2, cell_items2, img2_width, img2_height,
                              min_level, max_level, radius, th_low, nratio, histo_len, check_orientation, (int32_t*)dbest, out, cap,
                              out_counts, flags);
}

/* ------------------------------------------------------------------ pose optimisation / local BA */
int tb_pose_opt_batch_dev(tb_ctx* ctx, int nproblems, const double K[4], const float* Tcw_in, const tb_obs* obs,
                          const int32_t* counts, int obs_pitch, uint8_t* outlier, float* Tcw_out, int32_t* n_inliers,
                          double* stats) {
    TB_ENTER(ctx);
    if (!ctx || nproblems < 0 || !K || !Tcw_in || !obs || !counts || !outlier || !Tcw_out || !n_inliers || obs_pitch < 1)
        return TB_EINVAL;
    void* derr;
    int rc = tb_scratch(ctx, TB_SLOT_LK, (size_t)nproblems * obs_pitch * 3 * sizeof(double), &derr);
    if (rc) return rc;
    return tbk_pose_batch(ctx, nproblems, K, Tcw_in, obs, counts, obs_pitch, outlier, Tcw_out, n_inliers, stats, (double*)derr);
}

int tb_pose_opt(tb_ctx* ctx, const double K[4], const float Tcw_in[16], const tb_obs* obs, int n, uint8_t* outlier,
                float Tcw_out[16], int* n_inliers, double* stats) {
    TB_ENTER(ctx);
    if (!ctx || !K || !Tcw_in || !Tcw_out || !n_inliers || n < 0 || (n && (!obs || !outlier))) return TB_EINVAL;
    const int pitch = std::max(n, 1);
    size_t end = 0;
    const size_t oObs = stage_piece(end, (size_t)pitch * sizeof(tb_obs)), oOut = stage_piece(end, (size_t)pitch), oTin = stage_piece(end, 64),
                 oTout = stage_piece(end, 64), oStats = stage_piece(end, 64), oCnt = stage_piece(end, 8);
    char* b;
    int rc;
    if ((rc = tb_scratch(ctx, TB_SLOT_HOST, end, (void**)&b))) return rc;
    int32_t* dcnt = (int32_t*)(b + oCnt); /* the row count, then the inliers */
    TB_UPLOAD(ctx, b + oObs, obs, (size_t)n * sizeof(tb_obs));
    TB_UPLOAD(ctx, b + oOut, outlier, (size_t)n);
    TB_UPLOAD(ctx, b + oTin, Tcw_in, 64);
    TB_UPLOAD(ctx, dcnt, &n, 4);
    if ((rc = tb_pose_opt_batch_dev(ctx, 1, K, (const float*)(b + oTin), (const tb_obs*)(b + oObs), dcnt, pitch, (uint8_t*)(b + oOut),
                                    (float*)(b + oTout), dcnt + 1, (double*)(b + oStats))))
        return rc;
    int32_t ninl = 0;
    TB_DOWNLOAD(ctx, Tcw_out, b + oTout, 64);
    TB_DOWNLOAD(ctx, &ninl, dcnt + 1, 4);
    TB_DOWNLOAD(ctx, outlier, b + oOut, (size_t)n);
    if (stats) TB_DOWNLOAD(ctx, stats, b + oStats, 64);
    TB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n_inliers = ninl;
    return TB_OK;
}

/* ------------------------------------------------------------------ linear triangulation */
static bool triangulate_params_ok(const tb_triangulate_params* prm) {
    return prm && std::isfinite(prm->cos_parallax_max) && std::isfinite(prm->chi2_max);
}

int tb_linear_triangle_batch_dev(tb_ctx* ctx, int npairs, const float* xy0, const float* xy1, const int32_t* counts, int pitch,
                                 const float* Tcw0, const float* Tcw1, const double K[4], const float* inv_sigma2_0,
                                 const float* inv_sigma2_1, const uint8_t* skip, const tb_triangulate_params* prm, float* points,
                                 uint8_t* flags, int32_t* tally) {
    TB_ENTER(ctx);
    if (!ctx || npairs < 0 || pitch < 1 || !xy0 || !xy1 || !Tcw0 || !Tcw1 || !K || !points || !flags || !tally) return TB_EINVAL;
    if (!triangulate_params_ok(prm) || !(K[0] > 0.0) || !(K[1] > 0.0) || !std::isfinite(K[2]) || !std::isfinite(K[3]))
        return tb_fail(ctx, TB_EINVAL, "tb_linear_triangle_batch_dev: parameters / K must be finite, fx and fy positive");
    if (npairs > 65535) return tb_fail(ctx, TB_EUNSUPPORTED, "tb_linear_triangle_batch_dev: %d pairs (at most 65535 per call)", npairs);
    return tbk_linear_triangle(ctx, npairs, xy0, xy1, counts, pitch, Tcw0, Tcw1, K, inv_sigma2_0, inv_sigma2_1, skip,
                               prm->cos_parallax_max, prm->chi2_max, points, flags, tally);
}

int tb_linear_triangle(tb_ctx* ctx, const float* xy0, const float* xy1, int n, const float Tcw0[16], const float Tcw1[16],
                       const double K[4], const float* inv_sigma2_0, const float* inv_sigma2_1, const uint8_t* skip,
                       const tb_triangulate_params* prm, float* points, uint8_t* flags, int32_t tally[6]) {
    TB_ENTER(ctx);
    if (!ctx || n < 0 || !Tcw0 || !Tcw1 || !K || !prm || !tally || (n && (!xy0 || !xy1 || !points || !flags))) return TB_EINVAL;
    const size_t pitch = (size_t)std::max(n, 1);
    size_t end = 0;
    const size_t oA = stage_piece(end, pitch * 8), oB = stage_piece(end, pitch * 8), oT0 = stage_piece(end, 64), oT1 = stage_piece(end, 64),
                 oS0 = stage_piece(end, pitch * 4), oS1 = stage_piece(end, pitch * 4), oSkip = stage_piece(end, pitch),
                 oPts = stage_piece(end, pitch * 12), oFlags = stage_piece(end, pitch), oTally = stage_piece(end, 24), oCnt = stage_piece(end, 4);
    char* b;
    int rc;
    if ((rc = tb_scratch(ctx, TB_SLOT_HOST, end, (void**)&b))) return rc;
    const int32_t cnt = n;
    TB_UPLOAD(ctx, b + oA, xy0, (size_t)n * 8);
    TB_UPLOAD(ctx, b + oB, xy1, (size_t)n * 8);
    TB_UPLOAD(ctx, b + oT0, Tcw0, 64);
    TB_UPLOAD(ctx, b + oT1, Tcw1, 64);
    TB_UPLOAD(ctx, b + oCnt, &cnt, 4);
    if (inv_sigma2_0) TB_UPLOAD(ctx, b + oS0, inv_sigma2_0, (size_t)n * 4);
    if (inv_sigma2_1) TB_UPLOAD(ctx, b + oS1, inv_sigma2_1, (size_t)n * 4);
    if (skip) TB_UPLOAD(ctx, b + oSkip, skip, (size_t)n);
    TB_HIP(ctx, hipMemsetAsync(b + oPts, 0, pitch * 12, ctx->stream));   /* the operator writes accepted points only */
    if ((rc = tb_linear_triangle_batch_dev(ctx, 1, (const float*)(b + oA), (const float*)(b + oB), (const int32_t*)(b + oCnt), (int)pitch,
                                           (const float*)(b + oT0), (const float*)(b + oT1), K, inv_sigma2_0 ? (const float*)(b + oS0) : nullptr,
                                           inv_sigma2_1 ? (const float*)(b + oS1) : nullptr, skip ? (const uint8_t*)(b + oSkip) : nullptr, prm,
                                           (float*)(b + oPts), (uint8_t*)(b + oFlags), (int32_t*)(b + oTally))))
        return rc;
    TB_DOWNLOAD(ctx, points, b + oPts, (size_t)n * 12);
    TB_DOWNLOAD(ctx, flags, b + oFlags, (size_t)n);
    TB_DOWNLOAD(ctx, tally, b + oTally, 24);
    TB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (n == 0) tally[0] = 0;   /* the staged row of one entry is beyond the count */
    return TB_OK;
}

int tb_pnp_ransac_batch_dev(tb_ctx* ctx, int nproblems, const double K[4], const tb_obs* obs, const int32_t* counts, int obs_pitch,
                            const tb_pnp_params* prm, const float* Tcw_prior, float* Tcw_out, int32_t* consensus, uint8_t* inlier,
                            int32_t* winner, int32_t* flags) {
    TB_ENTER(ctx);
    if (!ctx || nproblems < 0 || obs_pitch < 1 || !K || !obs || !counts || !prm) return TB_EINVAL;
    if (prm->hypotheses < 1 || prm->hypotheses > 1024 || !(prm->chi2_max >= 0.0) || !std::isfinite(prm->chi2_max) || !(K[0] > 0.0) ||
        !(K[1] > 0.0) || !std::isfinite(K[0]) || !std::isfinite(K[1]) || !std::isfinite(K[2]) || !std::isfinite(K[3]))
        return tb_fail(ctx, TB_EINVAL, "tb_pnp_ransac_batch_dev: hypotheses 1..1024, chi2_max finite and not negative, K finite, fx and fy positive");
    if (nproblems > 65535) return tb_fail(ctx, TB_EUNSUPPORTED, "tb_pnp_ransac_batch_dev: %d problems (at most 65535 per call)", nproblems);
    return tbk_pnp_batch(ctx, nproblems, K, obs, counts, obs_pitch, prm->hypotheses, prm->chi2_max, prm->seed, Tcw_prior, Tcw_out,
                         consensus, inlier, winner, flags);
}

int tb_pnp_ransac(tb_ctx* ctx, const double K[4], const tb_obs* obs, int n, const tb_pnp_params* prm, const float* Tcw_prior,
                  float Tcw_out[16], int* consensus, uint8_t* inlier, int32_t winner[2], int* flags) {
    TB_ENTER(ctx);
    if (!ctx || n < 0 || !K || !prm || (n && !obs)) return TB_EINVAL;
    const size_t pitch = (size_t)std::max(n, 1);
    size_t end = 0;
    const size_t oObs = stage_piece(end, pitch * sizeof(tb_obs)), oPrior = stage_piece(end, 64), oT = stage_piece(end, 64),
                 oInl = stage_piece(end, pitch), oRes = stage_piece(end, 16), oCnt = stage_piece(end, 4);
    char* b;
    int rc;
    if ((rc = tb_scratch(ctx, TB_SLOT_HOST, end, (void**)&b))) return rc;
    const int32_t cnt = n;
    TB_UPLOAD(ctx, b + oObs, obs, (size_t)n * sizeof(tb_obs));
    TB_UPLOAD(ctx, b + oCnt, &cnt, 4);
    if (Tcw_prior) TB_UPLOAD(ctx, b + oPrior, Tcw_prior, 64);
    int32_t* res = (int32_t*)(b + oRes);   /* consensus, winner[2], flags */
    if ((rc = tb_pnp_ransac_batch_dev(ctx, 1, K, (const tb_obs*)(b + oObs), (const int32_t*)(b + oCnt), (int)pitch, prm,
                                      Tcw_prior ? (const float*)(b + oPrior) : nullptr, (float*)(b + oT), res, (uint8_t*)(b + oInl),
                                      res + 1, res + 3)))
        return rc;
    int32_t h[4];
    float T[16];
    TB_DOWNLOAD(ctx, T, b + oT, 64);
    TB_DOWNLOAD(ctx, h, res, 16);
    if (inlier) TB_DOWNLOAD(ctx, inlier, b + oInl, (size_t)n);
    TB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (Tcw_out) memcpy(Tcw_out, T, 64);
    if (consensus) *consensus = h[0];
    if (winner) { winner[0] = h[1]; winner[1] = h[2]; }
    if (flags) *flags = h[3];
    return TB_OK;
}

/* ------------------------------------------------------------------ Sim(3) from 3D-3D rows */
int tb_sim3_ransac_batch_dev(tb_ctx* ctx, int nproblems, const double K[4], const tb_sim3_row* rows, const int32_t* counts, int pitch,
                             const tb_sim3_params* prm, float* S12, double* srt, int32_t* consensus, uint8_t* inlier, int32_t* winner,
                             int32_t* flags) {
    TB_ENTER(ctx);
    if (!ctx || nproblems < 0 || pitch < 1 || !K || !rows || !counts || !prm) return TB_EINVAL;
    if (!tb_sim3_params_ok(prm) || !(K[0] > 0.0) || !(K[1] > 0.0) || !std::isfinite(K[0]) || !std::isfinite(K[1]) || !std::isfinite(K[2]) ||
        !std::isfinite(K[3]))
        return tb_fail(ctx, TB_EINVAL, "tb_sim3_ransac_batch_dev: hypotheses 1..1024, fixed_scale 0 or 1, chi2_max finite and not negative, K finite, fx and fy positive");
    if (nproblems > 65535) return tb_fail(ctx, TB_EUNSUPPORTED, "tb_sim3_ransac_batch_dev: %d problems (at most 65535 per call)", nproblems);
    return tbk_sim3_batch(ctx, nproblems, K, rows, counts, pitch, prm->hypotheses, prm->fixed_scale, prm->chi2_max, prm->seed, S12, srt,
                          consensus, inlier, winner, flags);
}

int tb_sim3_ransac(tb_ctx* ctx, const double K[4], const tb_sim3_row* rows, int n, const tb_sim3_params* prm, float S12[16], double srt[8],
                   int* consensus, uint8_t* inlier, int32_t winner[2], int* flags) {
    TB_ENTER(ctx);
    if (!ctx || n < 0 || !K || !prm || (n && !rows)) return TB_EINVAL;
    const size_t pitch = (size_t)std::max(n, 1);
    size_t end = 0;
    const size_t oRows = stage_piece(end, pitch * sizeof(tb_sim3_row)), oS = stage_piece(end, 64), oQ = stage_piece(end, 64),
                 oInl = stage_piece(end, pitch), oRes = stage_piece(end, 16), oCnt = stage_piece(end, 4);
    char* b;
    int rc;
    if ((rc = tb_scratch(ctx, TB_SLOT_HOST, end, (void**)&b))) return rc;
    const int32_t cnt = n;
    TB_UPLOAD(ctx, b + oRows, rows, (size_t)n * sizeof(tb_sim3_row));
    TB_UPLOAD(ctx, b + oCnt, &cnt, 4);
    int32_t* res = (int32_t*)(b + oRes);   /* consensus, winner[2], flags */
    if ((rc = tb_sim3_ransac_batch_dev(ctx, 1, K, (const tb_sim3_row*)(b + oRows), (const int32_t*)(b + oCnt), (int)pitch, prm, (float*)(b + oS),
                                       (double*)(b + oQ), res, (uint8_t*)(b + oInl), res + 1, res + 3)))
        return rc;
    int32_t h[4];
    float S[16];
    double q[8];
    TB_DOWNLOAD(ctx, S, b + oS, 64);
    TB_DOWNLOAD(ctx, q, b + oQ, 64);
    TB_DOWNLOAD(ctx, h, res, 16);
    if (inlier) TB_DOWNLOAD(ctx, inlier, b + oInl, (size_t)n);
    TB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (S12) memcpy(S12, S, 64);
    if (srt) memcpy(srt, q, 64);
    if (consensus) *consensus = h[0];
    if (winner) { winner[0] = h[1]; winner[1] = h[2]; }
    if (flags) *flags = h[3];
    return TB_OK;
}

/* ------------------------------------------------------------------ Sim(3) refinement on pixel rows */
int tb_sim3_optimize_batch_dev(tb_ctx* ctx, int nproblems, const double K[4], const tb_sim3_obs_row* rows, const int32_t* counts, int pitch,
                               const uint8_t* active_in, const double* srt_in, const tb_sim3_opt_params* prm, double* srt_out, float* S12,
                               int32_t* inliers, uint8_t* inlier_mask, double* stats) {
    TB_ENTER(ctx);
    if (!ctx || nproblems < 0 || pitch < 1 || !K || !rows || !counts || !prm || !srt_in || !inlier_mask) return TB_EINVAL;
    if (!tb_sim3_opt_params_ok(prm) || !(K[0] > 0.0) || !(K[1] > 0.0) || !std::isfinite(K[0]) || !std::isfinite(K[1]) || !std::isfinite(K[2]) ||
        !std::isfinite(K[3]))
        return tb_fail(ctx, TB_EINVAL, "tb_sim3_optimize_batch_dev: th2 finite and not negative, iteration counts 0..99, min_keep >= 0, fixed_scale 0 or 1, K finite, fx and fy positive");
    if (nproblems > 65535) return tb_fail(ctx, TB_EUNSUPPORTED, "tb_sim3_optimize_batch_dev: %d problems (at most 65535 per call)", nproblems);
    return tbk_sim3_opt_batch(ctx, nproblems, K, rows, counts, pitch, active_in, srt_in, prm, srt_out, S12, inliers, inlier_mask, stats);
}

int tb_sim3_optimize(tb_ctx* ctx, const double K[4], const tb_sim3_obs_row* rows, int n, const uint8_t* active, const double srt_in[8],
                     const tb_sim3_opt_params* prm, double srt_out[8], float S12[16], int* inliers, uint8_t* inlier_mask, double stats[8]) {
    TB_ENTER(ctx);
    if (!ctx || n < 0 || !K || !prm || !srt_in || (n && !rows)) return TB_EINVAL;
    const size_t pitch = (size_t)std::max(n, 1);
    size_t end = 0;
    const size_t oRows = stage_piece(end, pitch * sizeof(tb_sim3_obs_row)), oIn = stage_piece(end, 64), oOut = stage_piece(end, 64),
                 oS = stage_piece(end, 64), oStats = stage_piece(end, 64), oAct = stage_piece(end, pitch), oMask = stage_piece(end, pitch),
                 oCnt = stage_piece(end, 8);
    char* b;
    int rc;
    if ((rc = tb_scratch(ctx, TB_SLOT_HOST, end, (void**)&b))) return rc;
    const int32_t cnt = n;
    TB_UPLOAD(ctx, b + oRows, rows, (size_t)n * sizeof(tb_sim3_obs_row));
    TB_UPLOAD(ctx, b + oIn, srt_in, 64);
    TB_UPLOAD(ctx, b + oCnt, &cnt, 4);
    if (active && n) TB_UPLOAD(ctx, b + oAct, active, (size_t)n);
    int32_t* res = (int32_t*)(b + oCnt) + 1;   /* inliers */
    if ((rc = tb_sim3_optimize_batch_dev(ctx, 1, K, (const tb_sim3_obs_row*)(b + oRows), (const int32_t*)(b + oCnt), (int)pitch,
                                         active && n ? (const uint8_t*)(b + oAct) : nullptr, (const double*)(b + oIn), prm, (double*)(b + oOut),
                                         (float*)(b + oS), res, (uint8_t*)(b + oMask), (double*)(b + oStats))))
        return rc;
    double q[8], st[8];
    float S[16];
    int32_t h;
    TB_DOWNLOAD(ctx, q, b + oOut, 64);
    TB_DOWNLOAD(ctx, S, b + oS, 64);
    TB_DOWNLOAD(ctx, st, b + oStats, 64);
    TB_DOWNLOAD(ctx, &h, res, 4);
    if (inlier_mask && n) TB_DOWNLOAD(ctx, inlier_mask, b + oMask, (size_t)n);
    TB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (srt_out) memcpy(srt_out, q, 64);
    if (S12) memcpy(S12, S, 64);
    if (stats) memcpy(stats, st, 64);
    if (inliers) *inliers = h;
    return TB_OK;
}

/* ------------------------------------------------------------------ SearchBySim3 */
int tb_search_by_sim3_batch_dev(tb_ctx* ctx, int npairs, const double K[4], int width, int height, int nlevels, float scale,
                                const tb_keypoint* keys1, const uint8_t* desc1, const float* points1, const uint8_t* valid1,
                                const uint8_t* matched1, const int32_t* counts1, int pitch1, const tb_keypoint* keys2, const uint8_t* desc2,
                                const float* points2, const uint8_t* valid2, const uint8_t* matched2, const int32_t* counts2, int pitch2,
                                const double* srt, float th, int th_high, int32_t* match1, int32_t* match2, tb_match* pairs, int cap,
                                int32_t* pair_counts, int32_t* stats) {
    TB_ENTER(ctx);
    if (!ctx) return TB_EINVAL;
    if (npairs < 0 || !K || !keys1 || !desc1 || !points1 || !valid1 || !matched1 || !counts1 || !keys2 || !desc2 || !points2 || !valid2 ||
        !matched2 || !counts2 || !srt || pitch1 < 1 || pitch1 > 8192 || pitch2 < 1 || pitch2 > 8192 || nlevels < 1 || nlevels > TB_MAX_LEVELS ||
        !(th > 0.f) || !std::isfinite(th) || th_high < 0 || th_high > 256 || width < 1 || height < 1 || cap < 0 || (pairs && cap < 1) ||
        !(scale > 0.f) || !std::isfinite(scale) || !(K[0] > 0.0) || !(K[1] > 0.0) || !std::isfinite(K[0]) || !std::isfinite(K[1]) ||
        !std::isfinite(K[2]) || !std::isfinite(K[3]))
        return tb_fail(ctx, TB_EINVAL, "tb_search_by_sim3_batch_dev: null inputs, pitches %d, %d (1..8192), %d levels (1..%d), th (positive), "
                                       "th_high %d (0..256), image %d x %d, cap %d, scale (positive) or K", pitch1, pitch2, nlevels, TB_MAX_LEVELS,
                       th_high, width, height, cap);
    if (npairs > 65535) return tb_fail(ctx, TB_EUNSUPPORTED, "tb_search_by_sim3_batch_dev: %d pairs (at most 65535 per call)", npairs);
    if (npairs == 0) return TB_OK;
    float sf[TB_MAX_LEVELS], px[TB_MAX_LEVELS];
    TB_TRY(tb_scale_factors(nlevels, scale, sf, px, nullptr, nullptr));
    if (!match1 || !match2) {   /* the agreement pass needs both directions' lists: the caller's, or work */
        void* w;
        TB_TRY(tb_scratch(ctx, TB_SLOT_WORK, (size_t)npairs * ((size_t)pitch1 + pitch2) * sizeof(int32_t), &w));
        if (!match1) match1 = (int32_t*)w;
        if (!match2) match2 = (int32_t*)w + (size_t)npairs * pitch1;
    }
    const tbk_sim3_search_side s1 = {keys1, desc1, valid1, counts1, nullptr, points1, matched1, pitch1};
    const tbk_sim3_search_side s2 = {keys2, desc2, valid2, counts2, nullptr, points2, matched2, pitch2};
    return tbk_sim3_search_batch(ctx, npairs, K, width, height, nlevels, px, &s1, &s2, srt, nullptr, th, th_high, match1, match2, pairs, cap,
                                 pair_counts, stats);
}

/* ------------------------------------------------------------------ two-view initialisation */
int tb_two_view_batch_dev(tb_ctx* ctx, int nproblems, const float* xy0, const float* xy1, const int32_t* counts, int pitch,
                          const uint8_t* skip, const float* inv_sigma2_0, const float* inv_sigma2_1, const double K[4],
                          const float* Tcw0, const tb_two_view_params* prm, float* Tcw1, float* points, uint8_t* point_flags,
                          uint8_t* inlier, int32_t* consensus, int32_t* winner, int32_t* good, int32_t* tri, int32_t* status) {
    TB_ENTER(ctx);
    if (!ctx || nproblems < 0 || pitch < 1 || !K || !xy0 || !xy1 || !prm) return TB_EINVAL;
    if (!tb_two_view_params_ok(prm) || !(K[0] > 0.0) || !(K[1] > 0.0) || !std::isfinite(K[0]) || !std::isfinite(K[1]) ||
        !std::isfinite(K[2]) || !std::isfinite(K[3]))
        return tb_fail(ctx, TB_EINVAL, "tb_two_view_batch_dev: hypotheses 1..1024, thresholds finite and not negative, ratios in (0, 1], "
                                       "min_points >= 0, baseline positive and finite, K finite, fx and fy positive");
    if (nproblems > 65535) return tb_fail(ctx, TB_EUNSUPPORTED, "tb_two_view_batch_dev: %d problems (at most 65535 per call)", nproblems);
    if (pitch > TB_TWO_VIEW_MAX_PITCH)
        return tb_fail(ctx, TB_EUNSUPPORTED, "tb_two_view_batch_dev: pitch %d (at most %d rows are staged)", pitch, TB_TWO_VIEW_MAX_PITCH);
    return tbk_two_view(ctx, nproblems, xy0, xy1, counts, skip, inv_sigma2_0, inv_sigma2_1, pitch, K, Tcw0, prm, Tcw1, points, point_flags,
                        inlier, consensus, winner, good, tri, status);
}

int tb_two_view(tb_ctx* ctx, const float* xy0, const float* xy1, int n, const uint8_t* skip, const float* inv_sigma2_0,
                const float* inv_sigma2_1, const double K[4], const float Tcw0[16], const tb_two_view_params* prm, float Tcw1[16],
                float* points, uint8_t* point_flags, uint8_t* inlier, int* consensus, int32_t winner[2], int32_t good[4],
                int32_t tri[4], int* status) {
    TB_ENTER(ctx);
    if (!ctx || n < 0 || !K || !prm || (n && (!xy0 || !xy1))) return TB_EINVAL;
    const size_t pitch = (size_t)std::max(n, 1);
    size_t end = 0;
    const size_t oA = stage_piece(end, pitch * 8), oB = stage_piece(end, pitch * 8), oT0 = stage_piece(end, 64), oT1 = stage_piece(end, 64),
                 oS0 = stage_piece(end, pitch * 4), oS1 = stage_piece(end, pitch * 4), oSkip = stage_piece(end, pitch),
                 oPts = stage_piece(end, pitch * 12), oFlags = stage_piece(end, pitch), oInl = stage_piece(end, pitch),
                 oRes = stage_piece(end, 48), oCnt = stage_piece(end, 4);
    char* b;
    int rc;
    if ((rc = tb_scratch(ctx, TB_SLOT_HOST, end, (void**)&b))) return rc;
    const int32_t cnt = n;
    TB_UPLOAD(ctx, b + oA, xy0, (size_t)n * 8);
    TB_UPLOAD(ctx, b + oB, xy1, (size_t)n * 8);
    TB_UPLOAD(ctx, b + oCnt, &cnt, 4);
    if (Tcw0) TB_UPLOAD(ctx, b + oT0, Tcw0, 64);
    if (inv_sigma2_0) TB_UPLOAD(ctx, b + oS0, inv_sigma2_0, (size_t)n * 4);
    if (inv_sigma2_1) TB_UPLOAD(ctx, b + oS1, inv_sigma2_1, (size_t)n * 4);
    if (skip) TB_UPLOAD(ctx, b + oSkip, skip, (size_t)n);
    TB_HIP(ctx, hipMemsetAsync(b + oPts, 0, pitch * 12, ctx->stream));   /* the operator writes accepted points only */
    int32_t* res = (int32_t*)(b + oRes);   /* consensus, winner[2], good[4], tri[4], status */
    if ((rc = tb_two_view_batch_dev(ctx, 1, (const float*)(b + oA), (const float*)(b + oB), (const int32_t*)(b + oCnt), (int)pitch,
                                    skip ? (const uint8_t*)(b + oSkip) : nullptr, inv_sigma2_0 ? (const float*)(b + oS0) : nullptr,
                                    inv_sigma2_1 ? (const float*)(b + oS1) : nullptr, K, Tcw0 ? (const float*)(b + oT0) : nullptr, prm,
                                    (float*)(b + oT1), (float*)(b + oPts), (uint8_t*)(b + oFlags), (uint8_t*)(b + oInl), res, res + 1, res + 3,
                                    res + 7, res + 11)))
        return rc;
    int32_t h[12];
    float T[16];
    TB_DOWNLOAD(ctx, T, b + oT1, 64);
    TB_DOWNLOAD(ctx, h, res, 48);
    if (points) TB_DOWNLOAD(ctx, points, b + oPts, (size_t)n * 12);
    if (point_flags) TB_DOWNLOAD(ctx, point_flags, b + oFlags, (size_t)n);
    if (inlier) TB_DOWNLOAD(ctx, inlier, b + oInl, (size_t)n);
    TB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (Tcw1) memcpy(Tcw1, T, 64);
    if (consensus) *consensus = h[0];
    if (winner) { winner[0] = h[1]; winner[1] = h[2]; }
    if (good) memcpy(good, h + 3, 16);
    if (tri) memcpy(tri, h + 7, 16);
    if (status) *status = h[11];
    return TB_OK;
}

int tb_local_ba_batch_dev(tb_ctx* ctx, int nwindows, const double K[4], int nkf, int nfixed, float* poses, int npt, float* pts,
                          const tb_ba_obs* obs, const int32_t* obs_counts, int obs_pitch, int iters, double* stats) {
    TB_ENTER(ctx);
    if (!ctx || !K || !poses || !pts || !obs || !obs_counts || nwindows < 0 || nkf < 1 || npt < 1 || obs_pitch < 1 || nfixed < 0 ||
        nfixed > nkf || iters < 0)
        return TB_EINVAL;
    if (nwindows == 0) return TB_OK;
    const size_t wb = tbk_local_ba_work_bytes(ctx, nwindows, nkf, nfixed, npt, obs_pitch);
    void* dwork;
    int rc = tb_scratch(ctx, TB_SLOT_WORK, wb, &dwork);
    if (rc) return rc;
    return tbk_local_ba_batch(ctx, nwindows, K, nkf, nfixed, poses, npt, pts, obs, obs_counts, obs_pitch, iters, stats, dwork, wb);
}

int tb_local_ba(tb_ctx* ctx, const double K[4], int nkf, int nfixed, float* poses, int npt, float* pts, const tb_ba_obs* obs,
                int nobs, int iters, double* stats) {
    TB_ENTER(ctx);
    if (!ctx || !K || !poses || !pts || !obs || nkf < 1 || npt < 1 || nobs < 1 || nfixed < 0 || nfixed > nkf || iters < 0)
        return TB_EINVAL;
    for (int e = 0; e < nobs; e++)
        if (obs[e].kf < 0 || obs[e].kf >= nkf || obs[e].pt < 0 || obs[e].pt >= npt)
            return tb_fail(ctx, TB_EINVAL, "local_ba: observation %d out of range", e);
    /* the kernels want observations grouped by point; within a point by keyframe, so that the order of every sum, and with it
     * every bit of the result, is independent of the caller's row order (a repeated (keyframe, point) pair is rejected below) */
    std::vector<tb_ba_obs> sorted(obs, obs + nobs);
    std::stable_sort(sorted.begin(), sorted.end(),
                     [](const tb_ba_obs& a, const tb_ba_obs& b) { return a.pt != b.pt ? a.pt < b.pt : a.kf < b.kf; });
    size_t end = 0;
    const size_t oPoses = stage_piece(end, (size_t)nkf * 64), oPts = stage_piece(end, (size_t)npt * 12),
                 oObs = stage_piece(end, (size_t)nobs * sizeof(tb_ba_obs)), oStats = stage_piece(end, 64), oCnt = stage_piece(end, 4);
    char* b;
    int rc;
    if ((rc = tb_scratch(ctx, TB_SLOT_HOST, end, (void**)&b))) return rc;
    float *dposes = (float*)(b + oPoses), *dpts = (float*)(b + oPts);
    TB_UPLOAD(ctx, dposes, poses, (size_t)nkf * 64);
    TB_UPLOAD(ctx, dpts, pts, (size_t)npt * 12);
    TB_UPLOAD(ctx, b + oObs, sorted.data(), (size_t)nobs * sizeof(tb_ba_obs));
    TB_UPLOAD(ctx, b + oCnt, &nobs, 4);
    if ((rc = tb_local_ba_batch_dev(ctx, 1, K, nkf, nfixed, dposes, npt, dpts, (const tb_ba_obs*)(b + oObs), (const int32_t*)(b + oCnt), nobs,
                                    iters, (double*)(b + oStats))))
        return rc;
    double st[8];
    TB_DOWNLOAD(ctx, poses, dposes, (size_t)nkf * 64);
    TB_DOWNLOAD(ctx, pts, dpts, (size_t)npt * 12);
    TB_DOWNLOAD(ctx, st, b + oStats, 64);
    TB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (stats) memcpy(stats, st, 64);
    if (st[7] < 0) return tb_fail(ctx, TB_EINVAL, "local_ba: observations rejected by the device-side check");
    return TB_OK;
}

int tb_pose_graph_plan(tb_ctx* ctx, int ngraphs, int nnodes, int nfixed, int edge_pitch) {
    TB_ENTER(ctx);
    if (!ctx || ngraphs < 0 || nfixed < 1 || nfixed >= nnodes || edge_pitch < 1) return TB_EINVAL;
    if (nnodes > 64 || edge_pitch > 256)
        return tb_fail(ctx, TB_EUNSUPPORTED, "pose_graph: %d nodes, %d edges (at most 64, 256)", nnodes, edge_pitch);
    void* dwork;
    return ngraphs ? tb_scratch(ctx, TB_SLOT_WORK, tbk_pose_graph_work_bytes(ngraphs, nnodes, nfixed, edge_pitch), &dwork) : TB_OK;
}

int tb_pose_graph_batch_dev(tb_ctx* ctx, int ngraphs, int nnodes, int nfixed, float* poses, const tb_pg_edge* edges,
                            const int32_t* edge_counts, int edge_pitch, int iters, double* stats) {
    TB_ENTER(ctx);
    if (!ctx || !poses || !edges || !edge_counts || ngraphs < 0 || nfixed < 1 || nfixed >= nnodes || edge_pitch < 1 || iters < 0)
        return TB_EINVAL;
    if (nnodes > 64 || edge_pitch > 256 || iters > 99)
        return tb_fail(ctx, TB_EUNSUPPORTED, "pose_graph: %d nodes, %d edges, %d iterations (at most 64, 256, 99)", nnodes, edge_pitch, iters);
    if (ngraphs == 0) return TB_OK;
    void* dwork;
    TB_TRY(tb_scratch(ctx, TB_SLOT_WORK, tbk_pose_graph_work_bytes(ngraphs, nnodes, nfixed, edge_pitch), &dwork));
    return tbk_pose_graph_batch(ctx, ngraphs, nnodes, nfixed, poses, edges, edge_counts, edge_pitch, iters, stats, dwork);
}

int tb_pose_graph(tb_ctx* ctx, int nnodes, int nfixed, float* poses, const tb_pg_edge* edges, int nedges, int iters, double* stats) {
    TB_ENTER(ctx);
    if (!ctx || !poses || (!edges && nedges > 0) || nedges < 0 || nfixed < 1 || nfixed >= nnodes || iters < 0) return TB_EINVAL;
    if (nnodes > 64 || nedges > 256 || iters > 99)
        return tb_fail(ctx, TB_EUNSUPPORTED, "pose_graph: %d nodes, %d edges, %d iterations (at most 64, 256, 99)", nnodes, nedges, iters);
    const int pitch = std::max(nedges, 1);
    size_t end = 0;
    const size_t oPoses = stage_piece(end, (size_t)nnodes * 64), oEdges = stage_piece(end, (size_t)pitch * sizeof(tb_pg_edge)),
                 oStats = stage_piece(end, 64), oCnt = stage_piece(end, 4);
    char* b;
    int rc;
    if ((rc = tb_scratch(ctx, TB_SLOT_HOST, end, (void**)&b))) return rc;
    TB_UPLOAD(ctx, b + oPoses, poses, (size_t)nnodes * 64);
    TB_UPLOAD(ctx, b + oEdges, edges, (size_t)nedges * sizeof(tb_pg_edge));
    TB_UPLOAD(ctx, b + oCnt, &nedges, 4);
    if ((rc = tb_pose_graph_batch_dev(ctx, 1, nnodes, nfixed, (float*)(b + oPoses), (const tb_pg_edge*)(b + oEdges), (const int32_t*)(b + oCnt),
                                      pitch, iters, (double*)(b + oStats))))
        return rc;
    double st[8];
    TB_DOWNLOAD(ctx, poses, b + oPoses, (size_t)nnodes * 64);
    TB_DOWNLOAD(ctx, st, b + oStats, 64);
    TB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (stats) memcpy(stats, st, 64);
    if (st[7] < 0) return tb_fail(ctx, TB_EINVAL, "pose_graph: edges rejected by the device-side check");
    return TB_OK;
}

int tb_pose_graph_sim3_plan(tb_ctx* ctx, int ngraphs, int nnodes, int nfixed, int edge_pitch) {
    TB_ENTER(ctx);
    if (!ctx || ngraphs < 0 || nfixed < 1 || nfixed >= nnodes || edge_pitch < 1) return TB_EINVAL;
    if (nnodes > 64 || edge_pitch > 256)
        return tb_fail(ctx, TB_EUNSUPPORTED, "pose_graph_sim3: %d nodes, %d edges (at most 64, 256)", nnodes, edge_pitch);
    void* dwork;
    return ngraphs ? tb_scratch(ctx, TB_SLOT_WORK, tbk_pose_graph_sim3_work_bytes(ngraphs, nnodes, nfixed, edge_pitch), &dwork) : TB_OK;
}

int tb_pose_graph_sim3_batch_dev(tb_ctx* ctx, int ngraphs, int nnodes, int nfixed, int fixed_scale, double* nodes,
                                 const tb_pg_sim3_edge* edges, const int32_t* edge_counts, int edge_pitch, int iters, double* stats) {
    TB_ENTER(ctx);
    if (!ctx || !nodes || !edges || !edge_counts || ngraphs < 0 || nfixed < 1 || nfixed >= nnodes || edge_pitch < 1 || iters < 0 ||
        (fixed_scale != 0 && fixed_scale != 1))
        return TB_EINVAL;
    if (nnodes > 64 || edge_pitch > 256 || iters > 99)
        return tb_fail(ctx, TB_EUNSUPPORTED, "pose_graph_sim3: %d nodes, %d edges, %d iterations (at most 64, 256, 99)", nnodes, edge_pitch,
                       iters);
    if (ngraphs == 0) return TB_OK;
    void* dwork;
    TB_TRY(tb_scratch(ctx, TB_SLOT_WORK, tbk_pose_graph_sim3_work_bytes(ngraphs, nnodes, nfixed, edge_pitch), &dwork));
    return tbk_pose_graph_sim3_batch(ctx, ngraphs, nnodes, nfixed, fixed_scale, nodes, edges, edge_counts, edge_pitch, iters, stats, dwork);
}

int tb_pose_graph_sim3(tb_ctx* ctx, int nnodes, int nfixed, int fixed_scale, double* nodes, const tb_pg_sim3_edge* edges, int nedges,
                       int iters, double* stats) {
    TB_ENTER(ctx);
    if (!ctx || !nodes || (!edges && nedges > 0) || nedges < 0 || nfixed < 1 || nfixed >= nnodes || iters < 0 ||
        (fixed_scale != 0 && fixed_scale != 1))
        return TB_EINVAL;
    if (nnodes > 64 || nedges > 256 || iters > 99)
        return tb_fail(ctx, TB_EUNSUPPORTED, "pose_graph_sim3: %d nodes, %d edges, %d iterations (at most 64, 256, 99)", nnodes, nedges, iters);
    const int pitch = std::max(nedges, 1);
    size_t end = 0;
    const size_t oNodes = stage_piece(end, (size_t)nnodes * 64), oEdges = stage_piece(end, (size_t)pitch * sizeof(tb_pg_sim3_edge)),
                 oStats = stage_piece(end, 64), oCnt = stage_piece(end, 4);
    char* b;
    int rc;
    if ((rc = tb_scratch(ctx, TB_SLOT_HOST, end, (void**)&b))) return rc;
    TB_UPLOAD(ctx, b + oNodes, nodes, (size_t)nnodes * 64);
    TB_UPLOAD(ctx, b + oEdges, edges, (size_t)nedges * sizeof(tb_pg_sim3_edge));
    TB_UPLOAD(ctx, b + oCnt, &nedges, 4);
    if ((rc = tb_pose_graph_sim3_batch_dev(ctx, 1, nnodes, nfixed, fixed_scale, (double*)(b + oNodes), (const tb_pg_sim3_edge*)(b + oEdges),
                                           (const int32_t*)(b + oCnt), pitch, iters, (double*)(b + oStats))))
        return rc;
    double st[8];
    TB_DOWNLOAD(ctx, nodes, b + oNodes, (size_t)nnodes * 64);
    TB_DOWNLOAD(ctx, st, b + oStats, 64);
    TB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (stats) memcpy(stats, st, 64);
    if (st[7] < 0) return tb_fail(ctx, TB_EINVAL, "pose_graph_sim3: nodes or edges rejected by the device-side check");
    return TB_OK;
}

int tb_clahe_dev(tb_ctx* ctx, const uint8_t* src, int width, int height, int stride, double clip_limit, int tiles_x, int tiles_y,
                 uint8_t* dst, int dst_stride) {
    TB_ENTER(ctx);
    if (!ctx || !src || !dst || width < 1 || height < 1 || stride < width || dst_stride < width || tiles_x < 1 || tiles_y < 1) return TB_EINVAL;
    void* lut;
    int rc;
    if ((rc = tb_scratch(ctx, TB_SLOT_WORK, (size_t)tiles_x * tiles_y * 256, &lut))) return rc;
    return tbk_clahe(ctx, 1, src, width, height, stride, 0, clip_limit, tiles_x, tiles_y, dst, dst_stride, 0, (uint8_t*)lut);
}

int tb_clahe(tb_ctx* ctx, const uint8_t* src, int width, int height, int stride, double clip_limit, int tiles_x, int tiles_y,
             uint8_t* dst, int dst_stride) {
    TB_ENTER(ctx);
    if (!ctx || !src || !dst || width < 1 || height < 1 || stride < width || dst_stride < width || tiles_x < 1 || tiles_y < 1) return TB_EINVAL;
    size_t end = 0;
    const size_t oSrc = stage_piece(end, (size_t)stride * height), oDst = stage_piece(end, (size_t)dst_stride * height);
    char* b;
    int rc;
    if ((rc = tb_scratch(ctx, TB_SLOT_HOST, end, (void**)&b))) return rc;
    TB_UPLOAD(ctx, b + oSrc, src, (size_t)stride * height);
    if ((rc = tb_clahe_dev(ctx, (const uint8_t*)(b + oSrc), width, height, stride, clip_limit, tiles_x, tiles_y, (uint8_t*)(b + oDst), dst_stride)))
        return rc;
    TB_HIP(ctx, hipMemcpy2DAsync(dst, dst_stride, b + oDst, dst_stride, width, height, hipMemcpyDeviceToHost, ctx->stream));
    TB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return TB_OK;
}

int tb_optical_flow_pyr_lk_dev(tb_ctx* ctx, const uint8_t* prev, const uint8_t* next, int width, int height, int stride,
                               const float* prev_pts, int n, int win, int max_level, float* next_pts, uint8_t* status, float* err) {
    TB_ENTER(ctx);
    if (!ctx || !prev || !next || n < 0 || width < 1 || height < 1 || stride < width) return TB_EINVAL;
    if (n && (!prev_pts || !next_pts || !status)) return TB_EINVAL;
    if (max_level < 0 || max_level > 5) return tb_fail(ctx, TB_EUNSUPPORTED, "optical flow: max_level %d (0..5)", max_level);
    void* work;
    int rc;
    if ((rc = tb_scratch(ctx, TB_SLOT_LK, tbk_lk_work_bytes(width, height, max_level, 1), &work))) return rc;
    return tbk_lk_track(ctx, 1, prev, next, width, height, stride, 0, prev_pts, nullptr, n, n, win, max_level, next_pts, status, err, work,
                        nullptr);
}

int tb_optical_flow_pyr_lk_batch_dev(tb_ctx* ctx, int npairs, const uint8_t* prev, const uint8_t* next, int width, int height,
                                     int stride, size_t image_pitch, const float* prev_pts, const int32_t* counts, int pts_pitch,
                                     int win, int max_level, float* next_pts, uint8_t* status, float* err) {
    TB_ENTER(ctx);
    if (!ctx || npairs < 0 || pts_pitch < 0 || width < 1 || height < 1 || stride < width) return TB_EINVAL;
    if (npairs == 0 || pts_pitch == 0) return TB_OK;
    if (!prev || !next || !prev_pts || !next_pts || !status || image_pitch < (size_t)stride * height) return TB_EINVAL;
    if (max_level < 0 || max_level > 5) return tb_fail(ctx, TB_EUNSUPPORTED, "optical flow: max_level %d (0..5)", max_level);
    void* work;
    int rc;
    if ((rc = tb_scratch(ctx, TB_SLOT_LK, tbk_lk_work_bytes(width, height, max_level, npairs), &work))) return rc;
    return tbk_lk_track(ctx, npairs, prev, next, width, height, stride, image_pitch, prev_pts, counts, pts_pitch, pts_pitch, win, max_level,
                        next_pts, status, err, work, nullptr);
}

int tb_optical_flow_pyr_lk(tb_ctx* ctx, const uint8_t* prev, const uint8_t* next, int width, int height, int stride,
                           const float* prev_pts, int n, int win, int max_level, float* next_pts, uint8_t* status, float* err,
                           int* top_level) {
    TB_ENTER(ctx);
    if (!ctx || !prev || !next || n < 0 || width < 1 || height < 1 || stride < width) return TB_EINVAL;
    if (n && (!prev_pts || !next_pts || !status)) return TB_EINVAL;
    if (max_level < 0 || max_level > 5) return tb_fail(ctx, TB_EUNSUPPORTED, "optical flow: max_level %d (0..5)", max_level);
    const size_t img = (size_t)stride * height, np2 = (size_t)n * 2 * sizeof(float);
    size_t end = 0;
    const size_t oPrev = stage_piece(end, img), oNext = stage_piece(end, img), oPts = stage_piece(end, np2), oOut = stage_piece(end, np2),
                 oSt = stage_piece(end, (size_t)n), oErr = stage_piece(end, (size_t)n * sizeof(float));
    char* b;
    void* work;
    int rc;
    if ((rc = tb_scratch(ctx, TB_SLOT_HOST, end, (void**)&b))) return rc;
    if ((rc = tb_scratch(ctx, TB_SLOT_LK, tbk_lk_work_bytes(width, height, max_level, 1), &work))) return rc;
    TB_UPLOAD(ctx, b + oPrev, prev, img);
    TB_UPLOAD(ctx, b + oNext, next, img);
    TB_UPLOAD(ctx, b + oPts, prev_pts, np2);
    int top = 0;
    rc = tbk_lk_track(ctx, 1, (const uint8_t*)(b + oPrev), (const uint8_t*)(b + oNext), width, height, stride, 0, (const float*)(b + oPts),
                      nullptr, n, n, win, max_level, (float*)(b + oOut), (uint8_t*)(b + oSt), (float*)(b + oErr), work, &top);
    if (rc) return rc;
    TB_DOWNLOAD(ctx, next_pts, b + oOut, np2);
    TB_DOWNLOAD(ctx, status, b + oSt, (size_t)n);
    if (err) TB_DOWNLOAD(ctx, err, b + oErr, (size_t)n * sizeof(float));
    TB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (top_level) *top_level = top;
    return TB_OK;
}

int tb_search_by_opflow(tb_ctx* ctx, const uint8_t* img1, const uint8_t* img2, int width, int height, int stride,
                        const tb_camera* cam1, const float* keys2_xy, int n, int equalized, int reject, float* cur_points,
                        tb_match* out, int cap, int* count) {
    TB_ENTER(ctx);
    if (!ctx || !count || !cam1 || n < 0 || cap < 0 || (n && (!cur_points || !keys2_xy)) || (cap && !out)) return TB_EINVAL;
    *count = 0;
    if (!img1 || !img2 || width < 1 || height < 1 || stride < width) return TB_EINVAL;
    /* one pair of n keys (pitch 1 when n = 0: the images are still checked and equalised); the list holds every match */
    const size_t img = (size_t)stride * height, p = (size_t)std::max(n, 1);
    size_t end = 0;
    const size_t oI1 = stage_piece(end, img), oI2 = stage_piece(end, img), oKeys = stage_piece(end, p * 2 * sizeof(float)),
                 oCur = stage_piece(end, p * 2 * sizeof(float)), oSt = stage_piece(end, p), oOut = stage_piece(end, p * sizeof(tb_match)),
                 oCnt = stage_piece(end, 16);
    char* b;
    int rc;
    if ((rc = tb_scratch(ctx, TB_SLOT_HOST, end, (void**)&b))) return rc;
    const int32_t cnt[3] = {n, 0, 0}; /* n, then the match count and a flag that stays 0 */
    int32_t* dcnt = (int32_t*)(b + oCnt);
    TB_UPLOAD(ctx, b + oI1, img1, img);
    TB_UPLOAD(ctx, b + oI2, img2, img);
    TB_UPLOAD(ctx, b + oKeys, keys2_xy, (size_t)n * 2 * sizeof(float));
    TB_UPLOAD(ctx, dcnt, cnt, sizeof cnt);
    if ((rc = tb_search_by_opflow_batch_dev(ctx, 1, (const uint8_t*)(b + oI1), (const uint8_t*)(b + oI2), width, height, stride, img, cam1,
                                            (const float*)(b + oKeys), dcnt, (int)p, equalized, reject, (float*)(b + oCur),
                                            (uint8_t*)(b + oSt), (tb_match*)(b + oOut), (int)p, dcnt + 1)))
        return rc;
    TB_DOWNLOAD(ctx, cur_points, b + oCur, (size_t)n * 2 * sizeof(float));
    return match_tail(ctx, (const tb_match*)(b + oOut), dcnt + 1, cap, out, count);
}

int tb_search_by_opflow_batch_dev(tb_ctx* ctx, int npairs, const uint8_t* img1, const uint8_t* img2, int width, int height, int stride,
                                  size_t image_pitch, const tb_camera* cam1, const float* keys2_xy, const int32_t* counts, int pts_pitch,
                                  int equalized, int reject, float* cur_points, uint8_t* status, tb_match* out, int cap,
                                  int32_t* out_counts) {
    TB_ENTER(ctx);
    if (!ctx || !cam1 || npairs < 0 || pts_pitch < 0 || cap < 0 || width < 1 || height < 1 || stride < width) return TB_EINVAL;
    if (npairs == 0) return TB_OK;
    if (!img1 || !img2 || !out_counts || image_pitch < (size_t)stride * height) return TB_EINVAL;
    if (pts_pitch && (!keys2_xy || !cur_points || !status || (cap && !out))) return TB_EINVAL;
    int rc;
    const uint8_t* next = img1;
    if (equalized) { /* matcher.cpp:736-739: img1 = F1->Equalize() (Frame.cpp:453-458) */
        void *eq, *lut;
        if ((rc = tb_scratch(ctx, TB_SLOT_OPFLOW_EQ, (size_t)npairs * image_pitch, &eq))) return rc;
        if ((rc = tb_scratch(ctx, TB_SLOT_WORK, (size_t)npairs * 8 * 8 * 256, &lut))) return rc;
        if ((rc = tbk_clahe(ctx, npairs, img1, width, height, stride, image_pitch, 3.0, 8, 8, (uint8_t*)eq, stride, image_pitch, (uint8_t*)lut))) return rc;
        next = (const uint8_t*)eq;
    }
    if (pts_pitch) {
        void* work;
        if ((rc = tb_scratch(ctx, TB_SLOT_LK, tbk_lk_work_bytes(width, height, 3, npairs), &work))) return rc;
        /* matcher.cpp:744: calcOpticalFlowPyrLK(img2, img1, keys of F2, cur_points, ..., Size(21, 21), 3) */
        if ((rc = tbk_lk_track(ctx, npairs, img2, next, width, height, stride, image_pitch, keys2_xy, counts, pts_pitch, pts_pitch, 21, 3,
                               cur_points, status, nullptr, work, nullptr)))
            return rc;
    }
    if ((rc = tbk_flow_accept(ctx, npairs, cur_points, status, counts, pts_pitch, cam1->width, cam1->height, out, cap, out_counts))) return rc;
    if (reject && pts_pitch) {
        /* matcher.cpp:751-755: rejectWithF(cur_points, F2->GetCVKeys(), status); then the matches of what is left (pairs with
         * 8..14 tracked points take cv::findFundamentalMat's LMedS branch inside the same kernel, as in tb_reject_with_f) */
        void *work, *fl;
        if ((rc = tb_scratch(ctx, TB_SLOT_RANSAC, tbk_ransac_work_bytes(npairs, pts_pitch), &work))) return rc;
        if ((rc = tb_scratch(ctx, TB_SLOT_RANSAC_FLAGS, (size_t)npairs * sizeof(int32_t), &fl))) return rc;
        if ((rc = tbk_ransac_f(ctx, npairs, cur_points, keys2_xy, status, counts, pts_pitch, 0, 1.0, 0.99, work, (int32_t*)fl, nullptr, nullptr)))
            return rc;
        rc = tbk_flow_accept(ctx, npairs, cur_points, status, counts, pts_pitch, cam1->width, cam1->height, out, cap, out_counts);
    }
    return rc;
}

/* Matcher::rejectWithF / cv::findFundamentalMat, host forms: the launcher, which returns F and the iteration count */
static int ransac_host(tb_ctx* ctx, const float* p1, const float* p2, int n, uint8_t* status, int mode, double thresh, double conf,
                       double* F, int* iters, int* flag) {
    const size_t nb = (size_t)n * 2 * sizeof(float);
    size_t end = 0;
    const size_t o1 = stage_piece(end, nb), o2 = stage_piece(end, nb), oSt = stage_piece(end, (size_t)n), oFl = stage_piece(end, 8),
                 oF = stage_piece(end, 9 * sizeof(double));
    char* b;
    void* work;
    int rc;
    if ((rc = tb_scratch(ctx, TB_SLOT_HOST, end, (void**)&b)) || (rc = tb_scratch(ctx, TB_SLOT_RANSAC, tbk_ransac_work_bytes(1, n), &work)))
        return rc;
    int32_t* dfl = (int32_t*)(b + oFl); /* flag, then the iterations */
    TB_UPLOAD(ctx, b + o1, p1, nb);
    TB_UPLOAD(ctx, b + o2, p2, nb);
    TB_UPLOAD(ctx, b + oSt, status, (size_t)n);
    TB_HIP(ctx, hipMemsetAsync(b + oF, 0, 9 * sizeof(double), ctx->stream)); /* F stays 0 where no model comes back */
    if ((rc = tbk_ransac_f(ctx, 1, (const float*)(b + o1), (const float*)(b + o2), (uint8_t*)(b + oSt), nullptr, n, mode, thresh, conf, work,
                           dfl, (double*)(b + oF), dfl + 1)))
        return rc;
    int32_t h[2] = {0, 0};
    double hF[9];
    TB_DOWNLOAD(ctx, status, b + oSt, (size_t)n);
    TB_DOWNLOAD(ctx, h, dfl, sizeof h);
    TB_DOWNLOAD(ctx, hF, b + oF, sizeof hF);
    TB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (flag) *flag = h[0];
    if (iters) *iters = h[1];
    if (F) memcpy(F, hF, sizeof hF);
    return TB_OK;
}

int tb_find_fundamental_ransac(tb_ctx* ctx, const float* pts1, const float* pts2, int n, double thresh, double conf, uint8_t* mask,
                               double* F, int* iters, int* ok) {
    TB_ENTER(ctx);
    if (!ctx || n < 0 || !ok || (n && (!pts1 || !pts2 || !mask))) return TB_EINVAL;
    *ok = 0;
    if (iters) *iters = 0;
    if (n < 7) return TB_OK;                     /* cv::findFundamentalMat returns an empty matrix and no mask */
    int flag = 0;
    memset(mask, 0, (size_t)n);
    const int rc = ransac_host(ctx, pts1, pts2, n, mask, 1, thresh, conf, F, iters, &flag);
    if (rc) return rc;
    *ok = flag == 0 ? 1 : 0;
    return TB_OK;
}

int tb_reject_with_f_batch_dev(tb_ctx* ctx, int npairs, const float* cur_pts, const float* last_pts, const int32_t* counts,
                               int pts_pitch, uint8_t* status) {
    TB_ENTER(ctx);
    if (!ctx || npairs < 0 || pts_pitch < 0) return TB_EINVAL;
    if (npairs == 0 || pts_pitch == 0) return TB_OK;
    if (!cur_pts || !last_pts || !status) return TB_EINVAL;
    void *work, *fl;
    int rc;
    if ((rc = tb_scratch(ctx, TB_SLOT_RANSAC, tbk_ransac_work_bytes(npairs, pts_pitch), &work))) return rc;
    if ((rc = tb_scratch(ctx, TB_SLOT_RANSAC_FLAGS, (size_t)npairs * sizeof(int32_t), &fl))) return rc;
    return tbk_ransac_f(ctx, npairs, cur_pts, last_pts, status, counts, pts_pitch, 0, 1.0, 0.99, work, (int32_t*)fl, nullptr, nullptr);
}

int tb_reject_with_f(tb_ctx* ctx, const float* cur_pts, const float* last_pts, int n, uint8_t* status) {
    TB_ENTER(ctx);
    if (!ctx || n < 0 || (n && (!cur_pts || !last_pts || !status))) return TB_EINVAL;
    if (!(n > 8)) return TB_OK;                  /* matcher.cpp:870: findFundamentalMat is not called */
    int flag = 0;
    const int rc = ransac_host(ctx, cur_pts, last_pts, n, status, 0, 1.0, 0.99, nullptr, nullptr, &flag);
    if (rc) return rc;
    return TB_OK;
}

int tb_add_map_points_by_stereo_batch_dev(tb_ctx* ctx, int npairs, const uint8_t* img_stereo, const uint8_t* img_current, int width,
                                          int height, int stride, size_t image_pitch, const tb_camera* cam_stereo, const float* keys_xy,
                                          const int32_t* counts, int pts_pitch, float bf, float* cur_points, uint8_t* status,
                                          float* depth) {
    TB_ENTER(ctx);
    if (!ctx || !cam_stereo || npairs < 0 || pts_pitch < 0) return TB_EINVAL;
    if (npairs == 0 || pts_pitch == 0) return TB_OK;
    if (!depth || !cur_points || !status || !keys_xy) return TB_EINVAL;
    void *m, *mc;
    int rc;
    if ((rc = tb_scratch(ctx, TB_SLOT_STEREO_MATCHES, (size_t)npairs * pts_pitch * sizeof(tb_match), &m))) return rc;
    if ((rc = tb_scratch(ctx, TB_SLOT_STEREO_COUNTS, (size_t)npairs * sizeof(int32_t), &mc))) return rc;
    /* LocalBA.cpp:54: matcher->searchByOPFlow(stereo_frame, current_frame, pts, true, true) */
    if ((rc = tb_search_by_opflow_batch_dev(ctx, npairs, img_stereo, img_current, width, height, stride, image_pitch, cam_stereo, keys_xy,
                                            counts, pts_pitch, 1, 1, cur_points, status, (tb_match*)m, pts_pitch, (int32_t*)mc)))
        return rc;
    return tbk_stereo_depth(ctx, npairs, cur_points, keys_xy, status, counts, pts_pitch, bf, depth);
}

int tb_add_map_points_by_stereo(tb_ctx* ctx, const uint8_t* img_stereo, const uint8_t* img_current, int width, int height, int stride,
                                const tb_camera* cam_stereo, const float* keys_xy, int n, float bf, float* depth, int* n_depth) {
    TB_ENTER(ctx);
    if (!ctx || !cam_stereo || n < 0 || !n_depth || (n && (!keys_xy || !depth)) || !img_stereo || !img_current) return TB_EINVAL;
    *n_depth = 0;
    for (int i = 0; i < n; i++) depth[i] = -1.0f;
    if (n == 0) return TB_OK;
    if (width < 1 || height < 1 || stride < width) return TB_EINVAL;
    const size_t img = (size_t)stride * height;
    size_t end = 0;
    const size_t oI1 = stage_piece(end, img), oI2 = stage_piece(end, img), oKeys = stage_piece(end, (size_t)n * 2 * sizeof(float)),
                 oCur = stage_piece(end, (size_t)n * 2 * sizeof(float)), oSt = stage_piece(end, (size_t)n),
                 oDepth = stage_piece(end, (size_t)n * sizeof(float));
    char* b;
    int rc;
    if ((rc = tb_scratch(ctx, TB_SLOT_HOST, end, (void**)&b))) return rc;
    TB_UPLOAD(ctx, b + oI1, img_stereo, img);
    TB_UPLOAD(ctx, b + oI2, img_current, img);
    TB_UPLOAD(ctx, b + oKeys, keys_xy, (size_t)n * 2 * sizeof(float));
    if ((rc = tb_add_map_points_by_stereo_batch_dev(ctx, 1, (const uint8_t*)(b + oI1), (const uint8_t*)(b + oI2), width, height, stride, img,
                                                    cam_stereo, (const float*)(b + oKeys), nullptr, n, bf, (float*)(b + oCur),
                                                    (uint8_t*)(b + oSt), (float*)(b + oDepth))))
        return rc;
    std::vector<uint8_t> status((size_t)n);
    TB_DOWNLOAD(ctx, depth, b + oDepth, (size_t)n * sizeof(float));
    TB_DOWNLOAD(ctx, status.data(), b + oSt, (size_t)n);
    TB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n_depth = (int)std::count(status.begin(), status.end(), 1); /* the keys that kept a match */
    return TB_OK;
}

/* ---- multi-GPU batch entry: see include/tb_capi.h */
int tb_batch_run(tb_ctx** ctxs, int ngpu, const tb_batch_params* p, int nframes, const uint8_t* left, const uint8_t* right,
                 int stride, size_t pitch, int cap, tb_keypoint* kps, uint8_t* desc, int32_t* counts, tb_match* matches,
                 int32_t* match_counts) {
    if (!ctxs || ngpu < 1 || !p || nframes < 0 || !kps || !desc || !counts || !matches || !match_counts || cap < 1) return TB_EINVAL;
    for (int i = 0; i < ngpu; i++)
        if (!ctxs[i]) return TB_EINVAL;
    if (nframes == 0) return TB_OK;
    tb_ctx* c0 = ctxs[0];
    if (!left || !right || stride < p->width || pitch < (size_t)stride * p->height || p->nlevels < 2 || p->nlevels > TB_MAX_LEVELS)
        return tb_fail(c0, TB_EINVAL, "tb_batch_run: frame geometry / level count");
    std::vector<float> sf(p->nlevels), tmp(p->nlevels);
    tb_scale_factors(p->nlevels, p->scale, sf.data(), tmp.data(), tmp.data(), tmp.data());
    struct Shard {
        tb_ctx* ctx = nullptr;
        tb_extractor* ex = nullptr;
        int f0 = 0, m = 0;
        tb_keypoint* d_kps = nullptr; uint8_t* d_desc = nullptr; int32_t* d_counts = nullptr;   /* [2 m][cap] compact records */
        tb_match* d_matches = nullptr; int32_t* d_mcounts = nullptr;
    };
    std::vector<Shard> sh(ngpu);
    auto release = [&]() {
        for (Shard& s : sh) {
            if (!s.ctx) continue;
            hipSetDevice(s.ctx->device);
            hipStreamSynchronize(s.ctx->stream);
            if (s.ex) tb_extractor_destroy(s.ex);
            hipFree(s.d_kps); hipFree(s.d_desc); hipFree(s.d_counts); hipFree(s.d_matches); hipFree(s.d_mcounts);
        }
    };
    int rc = TB_OK;
    /* 1. queue every shard's chain: contiguous blocks of frames, left images [0, m), right images [m, 2 m) of the plan */
    for (int i = 0; i < ngpu && rc == TB_OK; i++) {
        Shard& s = sh[i];
        const int f0 = (int)((long long)nframes * i / ngpu), f1 = (int)((long long)nframes * (i + 1) / ngpu);
        if (f1 == f0) continue;
        s.ctx = ctxs[i]; s.f0 = f0; s.m = f1 - f0;
        tb_ctx* ctx = s.ctx;
        const int m = s.m;
        if ((rc = tb_extractor_create(ctx, p->width, p->height, p->nlevels, sf.data(), nullptr, nullptr, 2 * m, p->target, &s.ex))) break;
        tb_extractor* ex = s.ex;   /* tb_extractor_create has bound this thread to the context's device */
        const LevelGeom& L0 = ex->g.lv[0];
        hipError_t e = hipSuccess;
        for (int side = 0; side < 2 && e == hipSuccess; side++)
            for (int f = 0; f < m && e == hipSuccess; f++)
                e = hipMemcpy2DAsync(ex->d_slab + (size_t)(side * m + f) * ex->g.slabBytes + L0.off, L0.stride,
                                     (side ? right : left) + (size_t)(f0 + f) * pitch, stride, L0.w, L0.h, hipMemcpyHostToDevice,
                                     ctx->stream);
        if (e != hipSuccess) { rc = tb_fail(ctx, TB_EDEVICE, "tb_batch_run: frame upload: %s", hipGetErrorString(e)); break; }
        ex->g.img0 = nullptr;
        if ((rc = tb_extractor_build_pyramid(ex, 2 * m))) break;
        if ((rc = tb_extractor_orb(ex, 2 * m, p->target, p->init_th, p->min_th, 0, nullptr, 0))) break;
        if (hipMalloc(&s.d_kps, (size_t)2 * m * cap * sizeof(tb_keypoint)) != hipSuccess ||
            hipMalloc(&s.d_desc, (size_t)2 * m * cap * 32) != hipSuccess || hipMalloc(&s.d_counts, (size_t)2 * m * sizeof(int32_t)) != hipSuccess ||
            hipMalloc(&s.d_matches, (size_t)m * cap * sizeof(tb_match)) != hipSuccess ||
            hipMalloc(&s.d_mcounts, (size_t)m * sizeof(int32_t)) != hipSuccess) {
            rc = tb_fail(ctx, TB_ENOMEM, "tb_batch_run: record buffers of shard %d", i);
            break;
        }
        if ((rc = tb_extractor_copy_results_dev(ex, 2 * m, s.d_kps, s.d_desc, s.d_counts, cap))) break;
        /* searchByBF on the plan's own descriptor sets: left set f against right set m + f */
        const uint8_t* dsc = nullptr; const int32_t* cnt = nullptr; int selCap = 0;
        tb_extractor_results_dev(ex, nullptr, &dsc, &cnt, &selCap);
        if ((rc = tb_search_by_bf_batch_dev(ctx, m, dsc, cnt, dsc + (size_t)m * selCap * 32, cnt + m, (size_t)selCap * 32, p->bf_ratio,
                                            p->bf_min_th, s.d_matches, cap, s.d_mcounts)))
            break;
    }
    /* 2. the exchange step: every shard's records into the caller's arrays (waits for that shard only; the others keep working) */
    for (int i = 0; i < ngpu && rc == TB_OK; i++) {
        Shard& s = sh[i];
        if (!s.ctx) continue;
        tb_ctx* ctx = s.ctx;
        const int m = s.m, f0 = s.f0;
        hipError_t e = hipSetDevice(ctx->device);
        for (int side = 0; side < 2 && e == hipSuccess; side++) {
            e = hipMemcpyAsync(kps + ((size_t)side * nframes + f0) * cap, s.d_kps + (size_t)side * m * cap, (size_t)m * cap * sizeof(tb_keypoint),
                               hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess)
                e = hipMemcpyAsync(desc + ((size_t)side * nframes + f0) * cap * 32, s.d_desc + (size_t)side * m * cap * 32, (size_t)m * cap * 32,
                                   hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess)
                e = hipMemcpyAsync(counts + (size_t)side * nframes + f0, s.d_counts + (size_t)side * m, (size_t)m * sizeof(int32_t),
                                   hipMemcpyDeviceToHost, ctx->stream);
        }
        if (e == hipSuccess) e = hipMemcpyAsync(matches + (size_t)f0 * cap, s.d_matches, (size_t)m * cap * sizeof(tb_match), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(match_counts + f0, s.d_mcounts, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) { rc = tb_fail(ctx, TB_EDEVICE, "tb_batch_run: gather of shard %d: %s", i, hipGetErrorString(e)); break; }
        /* the compact records were cut at cap: say so instead of handing back a truncated frame */
        std::vector<int32_t> full(2 * m);
        if (tb_extractor_counts_host(s.ex, 2 * m, full.data()) == TB_OK)
            for (int k = 0; k < 2 * m; k++)
                if (full[k] > cap) { rc = tb_fail(ctx, TB_ECAPACITY, "tb_batch_run: %d keypoints in a frame of shard %d, capacity %d", full[k], i, cap); break; }
    }
    release();
    return rc;
}

/* ---- the depth filter (see include/tb_capi.h; kernels in k_depth_filter.hip) */
void tb_depth_filter_destroy(tb_depth_filter* df) {
    if (!df) return;
    if (df->ctx) { hipSetDevice(df->ctx->device); hipStreamSynchronize(df->ctx->stream); }
    df->own.release();
    delete df;
}

/* fn(s0, n) for every run of consecutive sequences the nullable host mask selects */
static int df_for_runs(int nseq, const uint8_t* mask, const std::function<int(int, int)>& fn) {
    for (int s = 0; s < nseq;) {
        if (mask && !mask[s]) { s++; continue; }
        int e = s + 1;
        while (e < nseq && (!mask || mask[e])) e++;
        TB_TRY(fn(s, e - s));
        s = e;
    }
    return TB_OK;
}

int tb_depth_filter_clear(tb_depth_filter* df, const uint8_t* which) {
    TB_ENTER((df ? df->ctx : nullptr));
    if (!df) return TB_EINVAL;
    tb_ctx* ctx = df->ctx;
    return df_for_runs(df->nseq, which, [&](int s0, int n) -> int {
        const size_t at = (size_t)s0 * df->pitch, cnt = (size_t)n * df->pitch;
        TB_HIP(ctx, hipMemsetAsync(df->seeds + at, 0, cnt * sizeof(tb_df_seed), ctx->stream));
        TB_HIP(ctx, hipMemsetAsync(df->traces + at, 0, cnt * sizeof(tb_df_trace), ctx->stream));
        TB_HIP(ctx, hipMemsetAsync(df->newest + s0, 0xff, (size_t)n * sizeof(int32_t), ctx->stream));
        for (int s = s0; s < s0 + n; s++) df->h_newest[s] = -1;
        return TB_OK;
    });
}

int tb_depth_filter_create(tb_ctx* ctx, int nseq, int pitch, int ref_slots, int width, int height, const double K[4],
                           const tb_depth_filter_params* prm, tb_depth_filter** out) {
    TB_ENTER(ctx);
    if (!ctx || !out) return TB_EINVAL;
    *out = nullptr;
    if (!K || !prm) return tb_fail(ctx, TB_EINVAL, "tb_depth_filter_create: null K / params");
    if (nseq < 1 || pitch < 1 || ref_slots < 1 || ref_slots > 16 || width < 1 || height < 1)
        return tb_fail(ctx, TB_EINVAL, "tb_depth_filter_create: %d sequences, pitch %d, %d reference slots (1..16), %d x %d", nseq, pitch,
                       ref_slots, width, height);
    if (!(prm->depth_min > 0.0) || !(prm->depth_mean >= prm->depth_min) || !std::isfinite(prm->depth_mean) || !(prm->conv_div > 0.0) ||
        !std::isfinite(prm->conv_div) || !(prm->px_noise > 0.0) || !std::isfinite(prm->px_noise) || prm->max_steps < 1 ||
        prm->zmssd_max < 0 || prm->align_iters < 0 || prm->align_iters > 99)
        return tb_fail(ctx, TB_EINVAL, "tb_depth_filter_create: depth_mean %g, depth_min %g, conv_div %g, px_noise %g, max_steps %d, "
                       "zmssd_max %d, align_iters %d (0..99)", prm->depth_mean, prm->depth_min, prm->conv_div, prm->px_noise, prm->max_steps,
                       prm->zmssd_max, prm->align_iters);
    if (!(K[0] > 0.0) || !(K[1] > 0.0) || !std::isfinite(K[0]) || !std::isfinite(K[1]) || !std::isfinite(K[2]) || !std::isfinite(K[3]))
        return tb_fail(ctx, TB_EINVAL, "tb_depth_filter_create: K");
    if (width < 16 || height < 16) return tb_fail(ctx, TB_EUNSUPPORTED, "tb_depth_filter_create: a %d x %d image (16 x 16 at least)", width, height);
    if (nseq > 65535) return tb_fail(ctx, TB_EUNSUPPORTED, "tb_depth_filter_create: %d sequences (65535 at most)", nseq);
    std::unique_ptr<tb_depth_filter, void (*)(tb_depth_filter*)> du(new tb_depth_filter(), tb_depth_filter_destroy);
    tb_depth_filter* df = du.get();
    df->ctx = ctx; df->nseq = nseq; df->pitch = pitch; df->ref_slots = ref_slots; df->width = width; df->height = height;
    for (int i = 0; i < 4; i++) df->K[i] = K[i];
    df->prm = *prm;
    df->px_err = 2.0 * std::atan(prm->px_noise / (2.0 * std::sqrt(K[0] * K[1])));
    df->h_newest.assign(nseq, -1);
    const size_t n = (size_t)nseq * pitch;
    TB_TRY(tb_dev_alloc(ctx, df->own, &df->seeds, n));
    TB_TRY(tb_dev_alloc(ctx, df->own, &df->traces, n));
    TB_TRY(tb_dev_alloc(ctx, df->own, &df->freelist, n, 0));
    TB_TRY(tb_dev_alloc(ctx, df->own, &df->ring, (size_t)nseq * ref_slots * width * height, 0));
    TB_TRY(tb_dev_alloc(ctx, df->own, &df->ring_Tcw, (size_t)nseq * ref_slots * 16, 0));
    TB_TRY(tb_dev_alloc(ctx, df->own, &df->newest, (size_t)nseq));
    TB_TRY(tb_depth_filter_clear(df, nullptr));
    *out = du.release();
    return TB_OK;
}

static int df_frame_args(tb_depth_filter* df, const char* who, const uint8_t* images, int stride, size_t image_pitch, const float* Tcw) {
    if (!images || !Tcw) return tb_fail(df->ctx, TB_EINVAL, "%s: null images / Tcw", who);
    if (stride < df->width || image_pitch < (size_t)stride * df->height)
        return tb_fail(df->ctx, TB_EINVAL, "%s: stride %d, image pitch %zu for %d x %d images", who, stride, image_pitch, df->width, df->height);
    return TB_OK;
}

int tb_depth_filter_add_keyframe_dev(tb_depth_filter* df, const uint8_t* images, int stride, size_t image_pitch, const float* Tcw,
                                     const float* keys_xy, const int32_t* counts, int key_pitch, const uint8_t* skip,
                                     const uint8_t* active, int32_t* not_added) {
    TB_ENTER((df ? df->ctx : nullptr));
    if (!df) return TB_EINVAL;
    TB_TRY(df_frame_args(df, "tb_depth_filter_add_keyframe_dev", images, stride, image_pitch, Tcw));
    if (!keys_xy || !counts || key_pitch < 1) return tb_fail(df->ctx, TB_EINVAL, "tb_depth_filter_add_keyframe_dev: keys / counts / key pitch %d", key_pitch);
    return df_for_runs(df->nseq, active, [&](int s0, int n) -> int {
        TB_TRY(tbk_df_add(df, s0, n, images, stride, image_pitch, Tcw, keys_xy, counts, key_pitch, skip, not_added));
        for (int s = s0; s < s0 + n; s++) df->h_newest[s] = (df->h_newest[s] + 1) % df->ref_slots;
        return TB_OK;
    });
}

int tb_depth_filter_update_dev(tb_depth_filter* df, const uint8_t* images, int stride, size_t image_pitch, const float* Tcw,
                               const uint8_t* active) {
    TB_ENTER((df ? df->ctx : nullptr));
    if (!df) return TB_EINVAL;
    TB_TRY(df_frame_args(df, "tb_depth_filter_update_dev", images, stride, image_pitch, Tcw));
    return df_for_runs(df->nseq, active, [&](int s0, int n) -> int { return tbk_df_update(df, s0, n, images, stride, image_pitch, Tcw); });
}

int tb_depth_filter_points_dev(tb_depth_filter* df, float* points, uint8_t* flags, int release) {
    TB_ENTER((df ? df->ctx : nullptr));
    if (!df) return TB_EINVAL;
    if (!points || !flags) return tb_fail(df->ctx, TB_EINVAL, "tb_depth_filter_points_dev: null points / flags");
    return tbk_df_points(df, points, flags, release);
}

int tb_depth_filter_state_dev(tb_depth_filter* df, const tb_df_seed** seeds, const tb_df_trace** traces, const float** slot_Tcw,
                              int32_t* newest_slot) {
    TB_ENTER((df ? df->ctx : nullptr));
    if (!df) return TB_EINVAL;
    if (seeds) *seeds = df->seeds;
    if (traces) *traces = df->traces;
    if (slot_Tcw) *slot_Tcw = df->ring_Tcw;
    if (newest_slot)
        for (int s = 0; s < df->nseq; s++) newest_slot[s] = df->h_newest[s];
    return TB_OK;
}

}  // extern "C"
