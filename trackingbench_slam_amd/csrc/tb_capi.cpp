/* Host side of libtb_hip.so: the C ABI of include/tb_capi.h on top of the HIP kernels (k_*.hip).
 * No CPU compute fallback lives here: every operator either runs its kernels or returns an error.
 * Host work is limited to set-up arithmetic the reference also does on the host (scale vectors, level
 * sizes, quotas, resize coefficient tables, cell tables) and data movement: a single-frame (host) form stages its inputs
 * and runs the batched kernels on one pair.
 */
#include "tb_internal.h"
#include "tb_math.h"

#include <stdarg.h>
#include <string.h>
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <memory>

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
    tb_prof_begin(ctx, "k_copy_results");
    hipLaunchKernelGGL(k_copy_results, dim3((rows * 15 + 255) / 256, n), dim3(256), 0, ctx->stream, ex->d_kps, ex->d_desc,
                       ex->d_counts, ex->g.selCap, kps, desc, counts, cap);
    tb_prof_end(ctx);
    TB_HIP(ctx, hipGetLastError());
    return TB_OK;
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

void tb_three_maxima(const int* sizes, int L, int* ind1, int* ind2, int* ind3) {
    /* Matcher::ComputeThreeMaxima, matcher.cpp:810-851 (caller initialises the indices, :379) */
    int max1 = 0, max2 = 0, max3 = 0;
    for (int i = 0; i < L; i++) {
        const int s = sizes[i];
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; *ind3 = *ind2; *ind2 = *ind1; *ind1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; *ind3 = *ind2; *ind2 = i; }
        else if (s > max3) { max3 = s; *ind3 = i; }
    }
    if ((float)max2 < 0.1f * (float)max1) { *ind2 = -1; *ind3 = -1; }
    else if ((float)max3 < 0.1f * (float)max1) { *ind3 = -1; }
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

/* ---- DBoW2 transform (see include/tb_capi.h) */
struct tb_vocab {
    tb_ctx* ctx = nullptr;
    int nnodes = 0, k = 0, L = 0, weighting = 0, scoring = 0;
    int32_t *d_child_start = nullptr, *d_child_items = nullptr, *d_word_id = nullptr;
    uint8_t* d_desc = nullptr;
    double* d_weight = nullptr;
};

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
struct tb_bow_db {
    tb_ctx* ctx = nullptr;
    int nseq = 0, cap = 0, pitch = 0, scoring = 0;
    long long nadded = 0;             /* adds since the last clear: the next one goes to slot nadded % cap */
    int32_t* words = nullptr;         /* [nseq][cap][pitch] */
    double* values = nullptr;         /* [nseq][cap][pitch] */
    int32_t* counts = nullptr;        /* [nseq][cap] */
    int32_t* kf_ids = nullptr;        /* [nseq][cap], -1 = empty */
};

void tb_bow_db_destroy(tb_bow_db* db) {
    if (!db) return;
    if (db->ctx) { hipSetDevice(db->ctx->device); hipStreamSynchronize(db->ctx->stream); }
    hipFree(db->words); hipFree(db->values); hipFree(db->counts); hipFree(db->kf_ids);
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
    TB_HIP(ctx, hipMalloc(&db->words, n * pitch * sizeof(int32_t)));
    TB_HIP(ctx, hipMalloc(&db->values, n * pitch * sizeof(double)));
    TB_HIP(ctx, hipMalloc(&db->counts, n * sizeof(int32_t)));
    TB_HIP(ctx, hipMalloc(&db->kf_ids, n * sizeof(int32_t)));
    int rc = tb_bow_db_clear(db);
    if (rc) return rc;
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
struct tb_kf_store {
    tb_ctx* ctx = nullptr;
    int nseq = 0, cap = 0, pitch = 0, max_cand = 0;
    long long nadded = 0;                 /* adds since the last clear: the next one goes to slot nadded % cap */
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
};

void tb_kf_store_destroy(tb_kf_store* st) {
    if (!st) return;
    if (st->ctx) { hipSetDevice(st->ctx->device); hipStreamSynchronize(st->ctx->stream); }
    hipFree(st->keys); hipFree(st->desc); hipFree(st->fv); hipFree(st->mp); hipFree(st->valid); hipFree(st->Tcw); hipFree(st->counts);
    hipFree(st->fv_counts); hipFree(st->kf_ids); hipFree(st->ix1); hipFree(st->ix2); hipFree(st->best); hipFree(st->matches);
    hipFree(st->obs); hipFree(st->outlier); hipFree(st->err); hipFree(st->seed); hipFree(st->pose); hipFree(st->mcounts);
    hipFree(st->flags); hipFree(st->ocounts); hipFree(st->ninl); hipFree(st->ckf);
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
    TB_HIP(ctx, hipMalloc(&st->keys, np * sizeof(tb_keypoint)));
    TB_HIP(ctx, hipMalloc(&st->desc, np * 32));
    TB_HIP(ctx, hipMalloc(&st->fv, np * sizeof(uint64_t)));
    TB_HIP(ctx, hipMalloc(&st->mp, np * 3 * sizeof(float)));
    TB_HIP(ctx, hipMalloc(&st->valid, np));
    TB_HIP(ctx, hipMalloc(&st->Tcw, n * 16 * sizeof(float)));
    TB_HIP(ctx, hipMalloc(&st->counts, n * sizeof(int32_t)));
    TB_HIP(ctx, hipMalloc(&st->fv_counts, n * sizeof(int32_t)));
    TB_HIP(ctx, hipMalloc(&st->kf_ids, n * sizeof(int32_t)));
    TB_HIP(ctx, hipMalloc(&st->ix1, pairs * sizeof(int32_t)));
    TB_HIP(ctx, hipMalloc(&st->ix2, pairs * sizeof(int32_t)));
    TB_HIP(ctx, hipMalloc(&st->best, pp * 16));
    TB_HIP(ctx, hipMalloc(&st->matches, pp * sizeof(tb_match)));
    TB_HIP(ctx, hipMalloc(&st->obs, pp * sizeof(tb_obs)));
    TB_HIP(ctx, hipMalloc(&st->outlier, pp));
    TB_HIP(ctx, hipMalloc(&st->err, pp * 3 * sizeof(double)));
    TB_HIP(ctx, hipMalloc(&st->seed, pairs * 16 * sizeof(float)));
    TB_HIP(ctx, hipMalloc(&st->pose, pairs * 16 * sizeof(float)));
    TB_HIP(ctx, hipMalloc(&st->mcounts, pairs * sizeof(int32_t)));
    TB_HIP(ctx, hipMalloc(&st->flags, pairs * sizeof(int32_t)));
    TB_HIP(ctx, hipMalloc(&st->ocounts, pairs * sizeof(int32_t)));
    TB_HIP(ctx, hipMalloc(&st->ninl, pairs * sizeof(int32_t)));
    TB_HIP(ctx, hipMalloc(&st->ckf, pairs * sizeof(int32_t)));
    TB_HIP(ctx, hipMemsetAsync(st->mcounts, 0, pairs * sizeof(int32_t), ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(st->ocounts, 0, pairs * sizeof(int32_t), ctx->stream));
    int rc = tb_kf_store_clear(st);
    if (rc) return rc;
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
    if ((rc = tbk_reloc_rows(ctx, pairs, q_keys, q_counts, q_pitch, st->ix1, st->ix2, st->matches, mcounts, st->mp, st->valid, st->counts,
                             st->pitch, inv_sigma2, nlevels, st->obs, st->ocounts, st->outlier, o.cand_rows)))
        return rc;
    if ((rc = tbk_pose_batch(ctx, pairs, K, st->seed, st->obs, st->ocounts, st->pitch, st->outlier, pose, ninl, nullptr, st->err))) return rc;
    if (mcounts != st->mcounts)   /* tb_kf_store_work_dev lends the last call's counts */
        TB_HIP(ctx, hipMemcpyAsync(st->mcounts, mcounts, (size_t)pairs * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
    if (!o.best_rank && !o.best_kf && !o.best_Tcw) return TB_OK;
    return tbk_reloc_select(ctx, st->nseq, ncand, prm->min_inliers, ckf, ninl, pose, o.best_rank, o.best_kf, o.best_Tcw);
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
    /* the kernels want observations grouped by point: stable sort keeps each point's edges in caller order */
    std::vector<tb_ba_obs> sorted(obs, obs + nobs);
    std::stable_sort(sorted.begin(), sorted.end(), [](const tb_ba_obs& a, const tb_ba_obs& b) { return a.pt < b.pt; });
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

/* ---- device-resident stereo VO loop (test/test_vo.cpp test_kitti): see include/tb_capi.h */
struct tb_vo {
    tb_ctx* ctx = nullptr;
    tb_vo_params p;
    int nseq = 0, P = 0;        /* sequences, key capacity (= the extractor's kp_capacity) */
    tb_extractor* ex = nullptr;
    tb_camera cam;              /* width / height: CameraModel::IsInFrame of both frames */
    int next = -1;              /* frame index of the next step (-1: not reset) */
    int cur = 0;                /* which half of the ping-pong buffers holds the last frame */
    /* ping-pong state: the last frame's and the current frame's */
    uint8_t* img[2] = {nullptr, nullptr};    /* [nseq][h][w] left images */
    float* keys[2] = {nullptr, nullptr};     /* [nseq][P][2] */
    int32_t* kcnt[2] = {nullptr, nullptr};   /* [nseq] */
    float* mp[2] = {nullptr, nullptr};       /* [nseq][P][3] */
    uint8_t* valid[2] = {nullptr, nullptr};  /* [nseq][P] */
    float* Tcw[2] = {nullptr, nullptr};      /* [nseq][16] */
    /* per-step buffers */
    uint8_t* right = nullptr;                /* [nseq][h][w] */
    uint8_t* status = nullptr;               /* [nseq][P] LK status of the tracking step */
    tb_match* matches = nullptr;             /* [nseq][P] */
    int32_t* mcounts = nullptr;              /* [nseq] */
    tb_obs* obs = nullptr;                   /* [nseq][P] */
    int32_t* obs_counts = nullptr;           /* [nseq] */
    uint8_t* outlier = nullptr;              /* [nseq][P] */
    int32_t* n_inliers = nullptr;            /* [nseq] */
    float* st_pts = nullptr;                 /* [nseq][P][2] stereo tracks */
    uint8_t* st_status = nullptr;            /* [nseq][P] */
    float* depth = nullptr;                  /* [nseq][P] */
    /* descriptor trackers (tr.kind != TB_VO_OPFLOW): the current frame's ORB results, the keyframe's snapshot */
    tb_vo_tracker tr;
    float inv_sigma2[TB_MAX_LEVELS];         /* Frame::GetInverseScaleSigmaSquares */
    tb_keypoint* orb = nullptr;              /* [nseq][P] */
    uint8_t* orb_desc = nullptr;             /* [nseq][P][32] */
    int32_t* orb_cnt = nullptr;              /* [nseq] */
    int32_t* mflags = nullptr;               /* [nseq] matcher flags */
    int32_t* win = nullptr;                  /* [nseq][P] k_vo_match_carry work */
    tb_keypoint* kf_orb = nullptr;           /* [nseq][P] */
    uint8_t* kf_desc = nullptr;              /* [nseq][P][32] */
    int32_t* kf_cnt = nullptr;               /* [nseq] */
    float* kf_mp = nullptr;                  /* [nseq][P][3] */
    uint8_t* kf_valid = nullptr;             /* [nseq][P] */
    int32_t* kf_cell_start = nullptr;        /* [nseq][4321] violence: the keyframe's lookup grid */
    int32_t* kf_cell_items = nullptr;        /* [nseq][P] */
    int kf_frame = -1;
    /* projection trackers (TB_VO_PROJECTION, TB_VO_PROJECTION_MAP) */
    int Mcap = 0;                            /* match capacity: P, or the map's capacity */
    float sf[TB_MAX_LEVELS];                 /* Frame::GetScaleFactors */
    int32_t* cell_start = nullptr;           /* [nseq][4321] the current frame's lookup grid */
    int32_t* cell_items = nullptr;           /* [nseq][P] */
    uint8_t* taken = nullptr;                /* [nseq][P] zero: Observations() is 0 throughout the loop */
    uint8_t* mp_desc = nullptr;              /* [nseq][P][32] the descriptors of the current frame's map points */
    uint8_t* kf_mp_desc = nullptr;           /* [nseq][P][32] */
    tb_mappoint* kf_rec = nullptr;           /* [nseq][P] TB_VO_PROJECTION: the keyframe's map points as the matcher reads them */
    /* the map (TB_VO_PROJECTION_MAP): two sets, eviction moves the survivors from one into the other */
    int mapK = 0, map_cap = 0, map_cur = 0, map_nblk = 0;   /* keyframes held, capacity, live set, blocks in use */
    tb_mappoint* map_rec[2] = {nullptr, nullptr};   /* [nseq][map_cap] */
    uint8_t* map_desc[2] = {nullptr, nullptr};      /* [nseq][map_cap][32] */
    int32_t* map_n[2] = {nullptr, nullptr};         /* [nseq] live counts */
    int32_t* map_blocks[2] = {nullptr, nullptr};    /* [nseq][mapK] points per held keyframe, oldest first */
    /* searchByBow (TB_VO_BOW): the borrowed vocabulary, Frame::SetBow's outputs of the current frame ([0]) and the keyframe ([1]) */
    tb_vo_bow bw;
    const tb_vocab* voc = nullptr;
    double* bow_wt = nullptr;                       /* [nseq][P] word weights of the current frame */
    int32_t* bow_word[2] = {nullptr, nullptr};      /* [nseq][P] word ids */
    int32_t* bow_node[2] = {nullptr, nullptr};      /* [nseq][P] node ids */
    uint64_t* fv_keys[2] = {nullptr, nullptr};      /* [nseq][P] FeatureVector keys */
    int32_t* fv_cnt[2] = {nullptr, nullptr};        /* [nseq] */
    int32_t* bv_word[2] = {nullptr, nullptr};       /* [nseq][P] BowVector words */
    double* bv_val[2] = {nullptr, nullptr};         /* [nseq][P] BowVector values */
    int32_t* bv_cnt[2] = {nullptr, nullptr};        /* [nseq] */
    tb_bow_db* db = nullptr;                        /* the keyframe database (tb_vo_bow_db_enable), owned */
    /* relocalisation (tb_vo_reloc_enable): the keyframe store, owned, and the query's outputs a caller does not take */
    tb_kf_store* store = nullptr;
    double *rl_scores = nullptr, *rl_top_score = nullptr;   /* [nseq][capacity], [nseq][max_candidates] */
    int32_t *rl_top_slot = nullptr, *rl_top_kf = nullptr;   /* [nseq][max_candidates] */
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
    /* ragged batches (tb_vo_reset_seq_dev / tb_vo_step_ragged_dev): the per-sequence frame counters live on the host in both
     * modes; everything else is allocated by the first call that needs it (vo_ragged_init) */
    bool ragged = false;                            /* the sequences no longer share one frame counter */
    std::vector<int32_t> seq_frame, seq_kf_frame;   /* [nseq] last frame, frame of the keyframe (-1: none) */
    std::vector<uint8_t> seq_reset;                 /* [nseq] the sequence has been reset at least once */
    bool rg_ready = false;
    tb_vo_frame_out rg_prev;                        /* the second set of per-frame outputs: a ragged step swaps the two */
    uint8_t* rg_left = nullptr;                     /* [nseq][h][w] the keyframe block's left images, compacted */
    float* rg_keys = nullptr;                       /* [nseq][P][2] its keys */
    int32_t* rg_kcnt = nullptr;                     /* [nseq] */
    int32_t* rg_dev = nullptr;                      /* [2][nseq] the step's mask and its keyframe index list */
    enum { RG_RING = 8 };
    int32_t* rg_pin = nullptr;                      /* [RG_RING][2][nseq] pinned staging; a slot is reused after its copy ran */
    hipEvent_t rg_ev[RG_RING] = {};
    unsigned rg_slot = 0;
};

static bool vo_is_proj(const tb_vo* vo) { return vo->tr.kind == TB_VO_PROJECTION || vo->tr.kind == TB_VO_PROJECTION_MAP; }

void tb_vo_destroy(tb_vo* vo) {
    if (!vo) return;
    hipSetDevice(vo->ctx->device);
    hipStreamSynchronize(vo->ctx->stream);
    if (vo->ex) tb_extractor_destroy(vo->ex);
    tb_bow_db_destroy(vo->db);
    tb_kf_store_destroy(vo->store);
    hipFree(vo->rl_scores); hipFree(vo->rl_top_score); hipFree(vo->rl_top_slot); hipFree(vo->rl_top_kf);
    hipFree(vo->rc_lost); hipFree(vo->rc_track); hipFree(vo->rc_kf); hipFree(vo->rc_kf_ids); hipFree(vo->rc_best_rank);
    hipFree(vo->rc_best_kf); hipFree(vo->rc_best_Tcw); hipFree(vo->rc_masked); hipFree(vo->rc_word_ring); hipFree(vo->rc_node_ring);
    for (int k = 0; k < 2; k++) {
        hipFree(vo->img[k]); hipFree(vo->keys[k]); hipFree(vo->kcnt[k]); hipFree(vo->mp[k]); hipFree(vo->valid[k]); hipFree(vo->Tcw[k]);
    }
    hipFree(vo->right); hipFree(vo->status); hipFree(vo->matches); hipFree(vo->mcounts); hipFree(vo->obs); hipFree(vo->obs_counts);
    hipFree(vo->outlier); hipFree(vo->n_inliers); hipFree(vo->st_pts); hipFree(vo->st_status); hipFree(vo->depth);
    hipFree(vo->orb); hipFree(vo->orb_desc); hipFree(vo->orb_cnt); hipFree(vo->mflags); hipFree(vo->win); hipFree(vo->kf_orb);
    hipFree(vo->kf_desc); hipFree(vo->kf_cnt); hipFree(vo->kf_mp); hipFree(vo->kf_valid); hipFree(vo->kf_cell_start);
    hipFree(vo->kf_cell_items);
    hipFree(vo->cell_start); hipFree(vo->cell_items); hipFree(vo->taken); hipFree(vo->mp_desc); hipFree(vo->kf_mp_desc); hipFree(vo->kf_rec);
    for (int k = 0; k < 2; k++) {
        hipFree(vo->map_rec[k]); hipFree(vo->map_desc[k]); hipFree(vo->map_n[k]); hipFree(vo->map_blocks[k]);
    }
    hipFree(vo->bow_wt);
    for (int k = 0; k < 2; k++) {
        hipFree(vo->bow_word[k]); hipFree(vo->bow_node[k]); hipFree(vo->fv_keys[k]); hipFree(vo->fv_cnt[k]); hipFree(vo->bv_word[k]);
        hipFree(vo->bv_val[k]); hipFree(vo->bv_cnt[k]);
    }
    {
        const tb_vo_frame_out& q = vo->rg_prev;
        hipFree(q.obs); hipFree(q.obs_counts); hipFree(q.outlier); hipFree(q.n_inliers); hipFree(q.orb); hipFree(q.orb_desc);
        hipFree(q.orb_cnt); hipFree(q.matches); hipFree(q.mcounts); hipFree(q.mflags); hipFree(q.mp_desc); hipFree(q.bow_word);
        hipFree(q.bow_node); hipFree(q.fv_keys); hipFree(q.fv_cnt); hipFree(q.bv_word); hipFree(q.bv_val); hipFree(q.bv_cnt);
        hipFree(vo->rg_left); hipFree(vo->rg_keys); hipFree(vo->rg_kcnt); hipFree(vo->rg_dev);
        if (vo->rg_pin) hipHostFree(vo->rg_pin);
        for (hipEvent_t e : vo->rg_ev)
            if (e) hipEventDestroy(e);
    }
    delete vo;
}

static int vo_create(tb_ctx* ctx, const tb_vo_params* p, const tb_vo_tracker* tr, int nseq, tb_vo** out, const tb_vo_bow* bow = nullptr,
                     const tb_vocab* voc = nullptr) {
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
    if (vo->tr.kind == TB_VO_PROJECTION_MAP) {
        if ((size_t)vo->tr.map_keyframes * (size_t)vo->P > (size_t)INT32_MAX / 64)
            return tb_fail(ctx, TB_EINVAL, "tb_vo_create_ex: map_keyframes %d x %d keys is too large", vo->tr.map_keyframes, vo->P);
        vo->mapK = vo->tr.map_keyframes;
        vo->map_cap = vo->Mcap = vo->mapK * vo->P;
    }
    memset(&vo->cam, 0, sizeof vo->cam);
    vo->cam.fx = (float)p->K[0]; vo->cam.fy = (float)p->K[1]; vo->cam.cx = (float)p->K[2]; vo->cam.cy = (float)p->K[3];
    vo->cam.width = p->width; vo->cam.height = p->height;
    const size_t S = (size_t)nseq, P = (size_t)vo->P, img = (size_t)p->width * p->height;
    for (int k = 0; k < 2; k++) {
        TB_HIP(ctx, hipMalloc(&vo->img[k], S * img));
        TB_HIP(ctx, hipMalloc(&vo->keys[k], S * P * 2 * sizeof(float)));
        TB_HIP(ctx, hipMalloc(&vo->kcnt[k], S * sizeof(int32_t)));
        TB_HIP(ctx, hipMalloc(&vo->mp[k], S * P * 3 * sizeof(float)));
        TB_HIP(ctx, hipMalloc(&vo->valid[k], S * P));
        TB_HIP(ctx, hipMalloc(&vo->Tcw[k], S * 16 * sizeof(float)));
    }
    TB_HIP(ctx, hipMalloc(&vo->right, S * img));
    TB_HIP(ctx, hipMalloc(&vo->status, S * P));
    TB_HIP(ctx, hipMalloc(&vo->matches, S * (size_t)vo->Mcap * sizeof(tb_match)));
    TB_HIP(ctx, hipMalloc(&vo->mcounts, S * sizeof(int32_t)));
    TB_HIP(ctx, hipMalloc(&vo->obs, S * P * sizeof(tb_obs)));
    TB_HIP(ctx, hipMalloc(&vo->obs_counts, S * sizeof(int32_t)));
    TB_HIP(ctx, hipMalloc(&vo->outlier, S * P));
    TB_HIP(ctx, hipMalloc(&vo->n_inliers, S * sizeof(int32_t)));
    TB_HIP(ctx, hipMalloc(&vo->st_pts, S * P * 2 * sizeof(float)));
    TB_HIP(ctx, hipMalloc(&vo->st_status, S * P));
    TB_HIP(ctx, hipMalloc(&vo->depth, S * P * sizeof(float)));
    for (int k = 0; k < 2; k++) {
        TB_HIP(ctx, hipMemsetAsync(vo->kcnt[k], 0, S * sizeof(int32_t), ctx->stream));
        TB_HIP(ctx, hipMemsetAsync(vo->valid[k], 0, S * P, ctx->stream));
    }
    TB_HIP(ctx, hipMemsetAsync(vo->obs_counts, 0, S * sizeof(int32_t), ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->n_inliers, 0, S * sizeof(int32_t), ctx->stream));
    /* every scratch slot the step's operators use, at its largest size now: a step never grows one (growth synchronises) */
    const size_t pitch = img;
    void* d;
    if ((rc = tb_scratch(ctx, TB_SLOT_OPFLOW_EQ, S * pitch, &d)) || (rc = tb_scratch(ctx, TB_SLOT_WORK, S * 8 * 8 * 256, &d)) ||
        (rc = tb_scratch(ctx, TB_SLOT_LK, std::max(tbk_lk_work_bytes(p->width, p->height, 3, nseq), S * P * 3 * sizeof(double)), &d)) ||
        (rc = tb_scratch(ctx, TB_SLOT_RANSAC, tbk_ransac_work_bytes(nseq, vo->P), &d)) || (rc = tb_scratch(ctx, TB_SLOT_RANSAC_FLAGS, S * sizeof(int32_t), &d)) ||
        (rc = tb_scratch(ctx, TB_SLOT_STEREO_MATCHES, S * P * sizeof(tb_match), &d)) || (rc = tb_scratch(ctx, TB_SLOT_STEREO_COUNTS, S * sizeof(int32_t), &d)))
        return rc;
    if (vo->tr.kind != TB_VO_OPFLOW) {
        tb_scale_factors(p->nlevels, p->scale, tmp.data(), nullptr, nullptr, vo->inv_sigma2);
        TB_HIP(ctx, hipMalloc(&vo->orb, S * P * sizeof(tb_keypoint)));
        TB_HIP(ctx, hipMalloc(&vo->orb_desc, S * P * 32));
        TB_HIP(ctx, hipMalloc(&vo->orb_cnt, S * sizeof(int32_t)));
        TB_HIP(ctx, hipMalloc(&vo->mflags, S * sizeof(int32_t)));
        TB_HIP(ctx, hipMalloc(&vo->win, S * P * sizeof(int32_t)));
        TB_HIP(ctx, hipMalloc(&vo->kf_orb, S * P * sizeof(tb_keypoint)));
        TB_HIP(ctx, hipMalloc(&vo->kf_desc, S * P * 32));
        TB_HIP(ctx, hipMalloc(&vo->kf_cnt, S * sizeof(int32_t)));
        TB_HIP(ctx, hipMalloc(&vo->kf_mp, S * P * 3 * sizeof(float)));
        TB_HIP(ctx, hipMalloc(&vo->kf_valid, S * P));
        TB_HIP(ctx, hipMalloc(&vo->kf_cell_start, S * 4321 * sizeof(int32_t)));
        TB_HIP(ctx, hipMalloc(&vo->kf_cell_items, S * P * sizeof(int32_t)));
        TB_HIP(ctx, hipMemsetAsync(vo->orb_cnt, 0, S * sizeof(int32_t), ctx->stream));
        TB_HIP(ctx, hipMemsetAsync(vo->kf_cnt, 0, S * sizeof(int32_t), ctx->stream));
        TB_HIP(ctx, hipMemsetAsync(vo->mcounts, 0, S * sizeof(int32_t), ctx->stream));
        TB_HIP(ctx, hipMemsetAsync(vo->mflags, 0, S * sizeof(int32_t), ctx->stream));
        /* an all-zero table is an empty grid: a ragged step runs the matcher for sequences that have no keyframe yet */
        TB_HIP(ctx, hipMemsetAsync(vo->kf_cell_start, 0, S * 4321 * sizeof(int32_t), ctx->stream));
        /* the matcher's slots: searchByBF's best rows per side, searchByViolence's (WORK, shared with CLAHE) */
        if (vo->tr.kind == TB_VO_BF) {
            if ((rc = tb_scratch(ctx, TB_SLOT_BF_TRAIN, S * P * 8, &d)) || (rc = tb_scratch(ctx, TB_SLOT_BF_QUERY, S * P * 8, &d))) return rc;
        } else if (vo_is_proj(vo)) {
            /* the projection matchers' best rows: 6 words per map point */
            if ((rc = tb_scratch(ctx, TB_SLOT_WORK, S * (size_t)vo->Mcap * 6 * sizeof(int32_t), &d))) return rc;
        } else if ((rc = tb_scratch(ctx, TB_SLOT_WORK, S * P * 16, &d))) {
            return rc;
        }
    }
    if (bow) {
        /* every output of the transform is a buffer of the loop, so tb_bow_transform_batch_dev takes no scratch; the matcher's
         * best rows (WORK) were sized above */
        TB_HIP(ctx, hipMalloc(&vo->bow_wt, S * P * sizeof(double)));
        for (int k = 0; k < 2; k++) {
            TB_HIP(ctx, hipMalloc(&vo->bow_word[k], S * P * sizeof(int32_t)));
            TB_HIP(ctx, hipMalloc(&vo->bow_node[k], S * P * sizeof(int32_t)));
            TB_HIP(ctx, hipMalloc(&vo->fv_keys[k], S * P * sizeof(uint64_t)));
            TB_HIP(ctx, hipMalloc(&vo->fv_cnt[k], S * sizeof(int32_t)));
            TB_HIP(ctx, hipMalloc(&vo->bv_word[k], S * P * sizeof(int32_t)));
            TB_HIP(ctx, hipMalloc(&vo->bv_val[k], S * P * sizeof(double)));
            TB_HIP(ctx, hipMalloc(&vo->bv_cnt[k], S * sizeof(int32_t)));
            TB_HIP(ctx, hipMemsetAsync(vo->fv_cnt[k], 0, S * sizeof(int32_t), ctx->stream));
            TB_HIP(ctx, hipMemsetAsync(vo->bv_cnt[k], 0, S * sizeof(int32_t), ctx->stream));
        }
    }
    if (vo_is_proj(vo)) {
        for (int l = 0; l < p->nlevels; l++) vo->sf[l] = sf[l];
        TB_HIP(ctx, hipMalloc(&vo->cell_start, S * 4321 * sizeof(int32_t)));
        TB_HIP(ctx, hipMalloc(&vo->cell_items, S * P * sizeof(int32_t)));
        TB_HIP(ctx, hipMalloc(&vo->taken, S * P));
        TB_HIP(ctx, hipMalloc(&vo->mp_desc, S * P * 32));
        TB_HIP(ctx, hipMalloc(&vo->kf_mp_desc, S * P * 32));
        TB_HIP(ctx, hipMemsetAsync(vo->taken, 0, S * P, ctx->stream));
        TB_HIP(ctx, hipMemsetAsync(vo->mp_desc, 0, S * P * 32, ctx->stream));
        TB_HIP(ctx, hipMemsetAsync(vo->kf_mp_desc, 0, S * P * 32, ctx->stream));
        if (vo->tr.kind == TB_VO_PROJECTION) {
            TB_HIP(ctx, hipMalloc(&vo->kf_rec, S * P * sizeof(tb_mappoint)));
        } else {
            const size_t C = (size_t)vo->map_cap;
            for (int k = 0; k < 2; k++) {
                TB_HIP(ctx, hipMalloc(&vo->map_rec[k], S * C * sizeof(tb_mappoint)));
                TB_HIP(ctx, hipMalloc(&vo->map_desc[k], S * C * 32));
                TB_HIP(ctx, hipMalloc(&vo->map_n[k], S * sizeof(int32_t)));
                TB_HIP(ctx, hipMalloc(&vo->map_blocks[k], S * vo->mapK * sizeof(int32_t)));
                TB_HIP(ctx, hipMemsetAsync(vo->map_n[k], 0, S * sizeof(int32_t), ctx->stream));
                TB_HIP(ctx, hipMemsetAsync(vo->map_blocks[k], 0, S * vo->mapK * sizeof(int32_t), ctx->stream));
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

static int vo_recover_clear(tb_vo* vo);

int tb_vo_reset_dev(tb_vo* vo, const float* Tcw0) {
    TB_ENTER((vo ? vo->ctx : nullptr));
    if (!vo || !Tcw0) return TB_EINVAL;
    tb_ctx* ctx = vo->ctx;
    /* frame 0 reads the "last frame": no keys, pose Tcw0 */
    TB_HIP(ctx, hipMemcpyAsync(vo->Tcw[vo->cur], Tcw0, (size_t)vo->nseq * 16 * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(vo->kcnt[vo->cur], 0, (size_t)vo->nseq * sizeof(int32_t), ctx->stream));
    if (vo->tr.kind != TB_VO_OPFLOW) {   /* no keyframe yet */
        TB_HIP(ctx, hipMemsetAsync(vo->kf_cnt, 0, (size_t)vo->nseq * sizeof(int32_t), ctx->stream));
        vo->kf_frame = -1;
    }
    if (vo->tr.kind == TB_VO_BOW) {
        TB_HIP(ctx, hipMemsetAsync(vo->fv_cnt[1], 0, (size_t)vo->nseq * sizeof(int32_t), ctx->stream));
        TB_HIP(ctx, hipMemsetAsync(vo->bv_cnt[1], 0, (size_t)vo->nseq * sizeof(int32_t), ctx->stream));
        int rc;
        if (vo->db && (rc = tb_bow_db_clear(vo->db))) return rc;   /* a new run: no keyframes yet */
        if (vo->store && (rc = tb_kf_store_clear(vo->store))) return rc;
        if (vo->rec_on && (rc = vo_recover_clear(vo))) return rc;
    }
    if (vo->mapK) {   /* an empty map */
        TB_HIP(ctx, hipMemsetAsync(vo->map_n[vo->map_cur], 0, (size_t)vo->nseq * sizeof(int32_t), ctx->stream));
        TB_HIP(ctx, hipMemsetAsync(vo->map_blocks[vo->map_cur], 0, (size_t)vo->nseq * vo->mapK * sizeof(int32_t), ctx->stream));
        vo->map_nblk = 0;
    }
    vo->next = 0;
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

/* The recovery stage of frame t > 0 (include/tb_capi.h, tb_vo_recover): flag, query, mask, verify, adopt, switch the tracking
 * keyframe. Every launch is on the context's stream; which sequences adopt is decided on the device. */
static int vo_recover_stage(tb_vo* vo, int b) {
    tb_ctx* ctx = vo->ctx;
    tb_kf_store* st = vo->store;
    tb_bow_db* db = vo->db;
    const tb_vo_recover& r = vo->rec;
    const int S = vo->nseq, P = vo->P;
    int rc;
    if ((rc = tb_bow_db_query_dev(db, vo->bv_word[0], vo->bv_val[0], vo->bv_cnt[0], P, r.exclude_newest, r.topk, vo->rl_scores,
                                  vo->rl_top_slot, vo->rl_top_kf, vo->rl_top_score, nullptr)))
        return rc;
    if ((rc = tbk_vo_recover_mask(ctx, S, r.topk, r.lost_inliers, vo->n_inliers, vo->rl_top_slot, vo->rc_lost, vo->rc_track, vo->rc_masked)))
        return rc;
    tb_reloc_params prm;
    prm.map_point_only = vo->bw.map_point_only; prm.th_low = vo->bw.th_low; prm.nratio = vo->bw.nratio; prm.histo_len = vo->bw.histo_len;
    prm.check_orientation = vo->bw.check_orientation; prm.min_inliers = r.min_inliers;
    tb_reloc_out out = {};
    out.best_rank = vo->rc_best_rank; out.best_kf = vo->rc_best_kf; out.best_Tcw = vo->rc_best_Tcw;
    if ((rc = tb_relocalize_batch_dev(st, vo->p.K, vo->p.nlevels, vo->p.scale, vo->orb, vo->orb_desc, vo->orb_cnt, vo->fv_keys[0], vo->fv_cnt[0],
                                      P, vo->rc_masked, r.topk, &prm, &out)))
        return rc;
    tb_vo_recover_args a;
    a.topk = r.topk; a.pitch = P;
    a.lost = vo->rc_lost; a.best_rank = vo->rc_best_rank; a.best_kf = vo->rc_best_kf; a.ix2 = st->ix2; a.best_Tcw = vo->rc_best_Tcw;
    a.w_matches = st->matches; a.w_obs = st->obs; a.w_outlier = st->outlier; a.w_mcounts = st->mcounts; a.w_flags = st->flags;
    a.w_ocounts = st->ocounts; a.w_ninl = st->ninl;
    a.s_keys = st->keys; a.s_desc = st->desc; a.s_fv = (const unsigned long long*)st->fv; a.s_mp = st->mp; a.s_valid = st->valid;
    a.s_counts = st->counts; a.s_fv_counts = st->fv_counts;
    a.db_words = db->words; a.db_values = db->values; a.db_counts = db->counts;
    a.word_ring = vo->rc_word_ring; a.node_ring = vo->rc_node_ring;
    a.orb_counts = vo->orb_cnt;
    a.Tcw = vo->Tcw[b]; a.mp = vo->mp[b]; a.valid = vo->valid[b]; a.obs = vo->obs; a.outlier = vo->outlier; a.matches = vo->matches;
    a.obs_counts = vo->obs_counts; a.n_inliers = vo->n_inliers; a.mcounts = vo->mcounts; a.mflags = vo->mflags; a.recovered_kf = vo->rc_kf;
    a.kf_orb = vo->kf_orb; a.kf_desc = vo->kf_desc; a.kf_fv = (unsigned long long*)vo->fv_keys[1]; a.kf_mp = vo->kf_mp;
    a.kf_valid = vo->kf_valid; a.kf_cnt = vo->kf_cnt; a.kf_fv_cnt = vo->fv_cnt[1];
    a.kf_bv_word = vo->bv_word[1]; a.kf_bv_val = vo->bv_val[1]; a.kf_bv_cnt = vo->bv_cnt[1];
    a.kf_word = vo->bow_word[1]; a.kf_node = vo->bow_node[1]; a.kf_ids = vo->rc_kf_ids;
    if ((rc = tbk_vo_recover_adopt(ctx, S, &a))) return rc;
    return tbk_vo_recover_switch(ctx, S, &a);
}

/* A descriptor tracker's frame t after the left images are in img[b] (see include/tb_capi.h, tb_vo_tracker). */
static int vo_step_desc(tb_vo* vo, int t, bool keyframe, const uint8_t* right, int stride, size_t pitch) {
    tb_ctx* ctx = vo->ctx;
    const tb_vo_params& p = vo->p;
    const tb_vo_tracker& tr = vo->tr;
    const int S = vo->nseq, P = vo->P, W = p.width, H = p.height;
    const size_t ip = (size_t)W * H, SP = (size_t)S * P;
    const int a = vo->cur, b = a ^ 1;
    int rc;
    /* ORB operator() on every frame; the extractor's results do not outlive its next call, so they are copied out */
    if ((rc = tb_extractor_set_images_dev(vo->ex, vo->img[b], S, W, ip))) return rc;
    if ((rc = tb_extractor_build_pyramid(vo->ex, S))) return rc;
    if ((rc = tb_extractor_orb(vo->ex, S, p.target, p.init_th, p.min_th, 0, nullptr, 0))) return rc;
    if ((rc = tb_extractor_copy_results_dev(vo->ex, S, vo->orb, vo->orb_desc, vo->orb_cnt, P))) return rc;
    if (tr.kind == TB_VO_BOW) {
        /* :705 cur_frame_ptr->SetBow(vocabulary) on every frame: voc->transform(descriptors, mBowVec, mFeatVec, levelsup) */
        if ((rc = tb_bow_transform_batch_dev(ctx, vo->voc, S, vo->orb_desc, vo->orb_cnt, P, vo->bw.levelsup, vo->bow_word[0], vo->bow_node[0],
                                             vo->bow_wt, vo->fv_keys[0], vo->fv_cnt[0])))
            return rc;
        if ((rc = tb_bow_vector_batch_dev(ctx, vo->voc, S, vo->bow_word[0], vo->bow_wt, vo->orb_cnt, P, vo->bv_word[0], vo->bv_val[0],
                                          vo->bv_cnt[0])))
            return rc;
    }
    if (t == 0) {
        TB_HIP(ctx, hipMemcpyAsync(vo->Tcw[b], vo->Tcw[a], (size_t)S * 16 * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
        TB_HIP(ctx, hipMemsetAsync(vo->mcounts, 0, (size_t)S * sizeof(int32_t), ctx->stream));
        TB_HIP(ctx, hipMemsetAsync(vo->mflags, 0, (size_t)S * sizeof(int32_t), ctx->stream));
        TB_HIP(ctx, hipMemsetAsync(vo->n_inliers, 0, (size_t)S * sizeof(int32_t), ctx->stream));
    } else if (tr.kind == TB_VO_BOW) {
        /* searchByBow(cur, key_frame, MapPointOnly): F1 = the current frame, F2 = the keyframe, whose map points are has_mp2 */
        if ((rc = tb_search_by_bow_batch_dev(ctx, S, vo->orb, vo->orb_desc, P, vo->fv_keys[0], vo->fv_cnt[0], vo->kf_orb, vo->kf_desc, P,
                                             vo->fv_keys[1], vo->fv_cnt[1], vo->kf_valid, vo->bw.map_point_only, tr.th_low, tr.nratio,
                                             tr.histo_len, tr.check_orientation, vo->matches, P, vo->mcounts, vo->mflags)))
            return rc;
    } else if (tr.kind == TB_VO_BF) {
        /* :712 searchByBF(cur, key_frame, 0, nLevels, ratio, minTh): the whole-set branch */
        if ((rc = tb_search_by_bf_batch_dev(ctx, S, vo->orb_desc, vo->orb_cnt, vo->kf_desc, vo->kf_cnt, (size_t)P * 32, tr.bf_ratio,
                                            tr.bf_min_th, vo->matches, P, vo->mcounts)))
            return rc;
    } else {
        /* :713 searchByViolence(cur, key_frame, min_level, max_level, radius) over the keyframe's lookup grid */
        if ((rc = tb_search_by_violence_batch_dev(ctx, S, vo->orb, vo->orb_desc, vo->orb_cnt, P, vo->kf_orb, vo->kf_desc, vo->kf_cnt, P,
                                                  vo->kf_cell_start, vo->kf_cell_items, W, H, tr.min_level, tr.max_level, tr.radius,
                                                  tr.th_low, tr.nratio, tr.histo_len, tr.check_orientation, vo->matches, P, vo->mcounts,
                                                  vo->mflags)))
            return rc;
    }
    /* the keys, the map points the matches carry over and the pose rows (match count 0 at frame 0: a fresh frame) */
    if ((rc = tbk_vo_match_carry(ctx, S, vo->orb, vo->orb_cnt, vo->matches, vo->mcounts, vo->kf_mp, vo->kf_valid, vo->kf_cnt, P,
                                 vo->inv_sigma2, p.nlevels, vo->win, vo->keys[b], vo->kcnt[b], vo->mp[b], vo->valid[b], vo->obs,
                                 vo->obs_counts, vo->outlier)))
        return rc;
    if (t > 0 &&
        (rc = tb_pose_opt_batch_dev(ctx, S, p.K, vo->Tcw[a], vo->obs, vo->obs_counts, P, vo->outlier, vo->Tcw[b], vo->n_inliers, nullptr)))
        return rc;
    if (vo->rec_on && t > 0 && (rc = vo_recover_stage(vo, b))) return rc;
    if (keyframe) {
        /* :774-785 extracts again on the same pyramid: the same keys, so SetKeys resizes m to m and keeps every carried map
         * point -- nothing to do. Then :800 AddMapPointsByStereo and the new map points (:802-832), as the optical-flow loop. */
        if ((rc = tbk_vo_copy_image(ctx, S, right, W, H, stride, pitch, vo->right))) return rc;
        if ((rc = tb_add_map_points_by_stereo_batch_dev(ctx, S, vo->right, vo->img[b], W, H, W, ip, &vo->cam, vo->keys[b], vo->kcnt[b], P, p.bf,
                                                        vo->st_pts, vo->st_status, vo->depth)))
            return rc;
        if ((rc = tbk_vo_kf_spawn(ctx, S, vo->keys[b], vo->kcnt[b], vo->depth, vo->Tcw[b], p.K, P, vo->mp[b], vo->valid[b]))) return rc;
        /* key_frame = cur_frame_ptr (:836): a snapshot of fixed-size slabs; violence's lookup grid once per keyframe */
        TB_HIP(ctx, hipMemcpyAsync(vo->kf_orb, vo->orb, SP * sizeof(tb_keypoint), hipMemcpyDeviceToDevice, ctx->stream));
        TB_HIP(ctx, hipMemcpyAsync(vo->kf_desc, vo->orb_desc, SP * 32, hipMemcpyDeviceToDevice, ctx->stream));
        TB_HIP(ctx, hipMemcpyAsync(vo->kf_cnt, vo->orb_cnt, (size_t)S * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
        TB_HIP(ctx, hipMemcpyAsync(vo->kf_mp, vo->mp[b], SP * 3 * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
        TB_HIP(ctx, hipMemcpyAsync(vo->kf_valid, vo->valid[b], SP, hipMemcpyDeviceToDevice, ctx->stream));
        if (tr.kind == TB_VO_VIOLENCE &&
            (rc = tb_frame_grid_batch_dev(ctx, S, vo->kf_orb, vo->kf_cnt, P, W, H, vo->kf_cell_start, vo->kf_cell_items)))
            return rc;
        if (tr.kind == TB_VO_BOW) {   /* the keyframe keeps the vectors SetBow gave it: they are not computed again */
            TB_HIP(ctx, hipMemcpyAsync(vo->bow_word[1], vo->bow_word[0], SP * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
            TB_HIP(ctx, hipMemcpyAsync(vo->bow_node[1], vo->bow_node[0], SP * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
            TB_HIP(ctx, hipMemcpyAsync(vo->fv_keys[1], vo->fv_keys[0], SP * sizeof(uint64_t), hipMemcpyDeviceToDevice, ctx->stream));
            TB_HIP(ctx, hipMemcpyAsync(vo->fv_cnt[1], vo->fv_cnt[0], (size_t)S * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
            TB_HIP(ctx, hipMemcpyAsync(vo->bv_word[1], vo->bv_word[0], SP * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
            TB_HIP(ctx, hipMemcpyAsync(vo->bv_val[1], vo->bv_val[0], SP * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
            TB_HIP(ctx, hipMemcpyAsync(vo->bv_cnt[1], vo->bv_cnt[0], (size_t)S * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
            /* the keyframe database, when enabled: the snapshot's BowVector into the ring slot of this keyframe */
            if (vo->db && (rc = tb_bow_db_add_dev(vo->db, vo->bv_word[1], vo->bv_val[1], vo->bv_cnt[1], P, t))) return rc;
            /* the keyframe store, when enabled: the snapshot itself and the frame's optimised pose into the same ring slot */
            if (vo->store && (rc = tb_kf_store_add_dev(vo->store, vo->kf_orb, vo->kf_desc, vo->kf_cnt, vo->fv_keys[1], vo->fv_cnt[1], vo->kf_mp,
                                                       vo->kf_valid, P, vo->Tcw[b], t)))
                return rc;
            /* recovery, when enabled: the snapshot's word / node ids into the same ring slot (the store has just counted this
             * add); this keyframe is what every sequence tracks against from now on */
            if (vo->rec_on) {
                if ((rc = tbk_vo_recover_ring_add(ctx, S, vo->bow_word[1], vo->bow_node[1], vo->kf_cnt, vo->store->cap, P,
                                                  (int)((vo->store->nadded - 1) % vo->store->cap), vo->rc_word_ring, vo->rc_node_ring)))
                    return rc;
                TB_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)vo->rc_kf_ids, t, (size_t)S, ctx->stream));
            }
        }
        vo->kf_frame = t;
    }
    return TB_OK;
}

/* A projection tracker's frame t after the left images are in img[b] (see include/tb_capi.h, tb_vo_tracker). */
static int vo_step_proj(tb_vo* vo, int t, bool keyframe, const uint8_t* right, int stride, size_t pitch) {
    tb_ctx* ctx = vo->ctx;
    const tb_vo_params& p = vo->p;
    const tb_vo_tracker& tr = vo->tr;
    const bool map = tr.kind == TB_VO_PROJECTION_MAP;
    const int S = vo->nseq, P = vo->P, W = p.width, H = p.height;
    const size_t ip = (size_t)W * H, SP = (size_t)S * P;
    const int a = vo->cur, b = a ^ 1;
    int rc;
    /* test_projection.cpp:495-504: ORB operator(), SetKeys, AssignFeaturesToGrid on every frame */
    if ((rc = tb_extractor_set_images_dev(vo->ex, vo->img[b], S, W, ip))) return rc;
    if ((rc = tb_extractor_build_pyramid(vo->ex, S))) return rc;
    if ((rc = tb_extractor_orb(vo->ex, S, p.target, p.init_th, p.min_th, 0, nullptr, 0))) return rc;
    if ((rc = tb_extractor_copy_results_dev(vo->ex, S, vo->orb, vo->orb_desc, vo->orb_cnt, P))) return rc;
    if ((rc = tb_frame_grid_batch_dev(ctx, S, vo->orb, vo->orb_cnt, P, W, H, vo->cell_start, vo->cell_items))) return rc;
    if (t == 0) {
        TB_HIP(ctx, hipMemcpyAsync(vo->Tcw[b], vo->Tcw[a], (size_t)S * 16 * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
        TB_HIP(ctx, hipMemsetAsync(vo->mcounts, 0, (size_t)S * sizeof(int32_t), ctx->stream));
        TB_HIP(ctx, hipMemsetAsync(vo->mflags, 0, (size_t)S * sizeof(int32_t), ctx->stream));
        TB_HIP(ctx, hipMemsetAsync(vo->n_inliers, 0, (size_t)S * sizeof(int32_t), ctx->stream));
    } else if (map) {
        /* :516-517 searchByProjection(map_ptr, cur, radio) at the last frame's pose (:510) */
        if ((rc = tb_search_by_projection_map_batch_dev(ctx, S, vo->Tcw[a], &vo->cam, W, H, vo->orb, vo->orb_desc, vo->taken, vo->orb_cnt, P,
                                                        vo->cell_start, vo->cell_items, vo->map_rec[vo->map_cur], vo->map_desc[vo->map_cur],
                                                        vo->map_n[vo->map_cur], vo->map_cap, vo->map_cap, vo->sf, p.nlevels, tr.nratio,
                                                        tr.radio, tr.th_high, vo->matches, vo->Mcap, vo->mcounts, vo->mflags)))
            return rc;
    } else {
        /* :512-513 searchByProjection(cur, key_frame) at the last frame's pose (:510) */
        if ((rc = tb_search_by_projection_batch_dev(ctx, S, vo->Tcw[a], &vo->cam, W, H, vo->orb, vo->orb_desc, vo->taken, vo->orb_cnt, P,
                                                    vo->cell_start, vo->cell_items, vo->kf_orb, vo->kf_rec, vo->kf_mp_desc, vo->kf_cnt, P,
                                                    vo->sf, p.nlevels, tr.nratio, tr.th_high, tr.histo_len, tr.check_orientation,
                                                    vo->matches, vo->Mcap, vo->mcounts, vo->mflags)))
            return rc;
    }
    /* :520-530: the keys, the map points (and their descriptors) the matches carry over, the pose rows (no match at frame 0) */
    if (map) {
        rc = tbk_vo_proj_carry(ctx, S, 1, vo->orb, vo->orb_cnt, vo->matches, vo->mcounts, vo->Mcap, nullptr, nullptr, vo->map_rec[vo->map_cur],
                               vo->map_desc[vo->map_cur], vo->map_n[vo->map_cur], vo->map_cap, P, vo->inv_sigma2, p.nlevels, vo->win,
                               vo->keys[b], vo->kcnt[b], vo->mp[b], vo->valid[b], vo->mp_desc, vo->obs, vo->obs_counts, vo->outlier);
    } else {
        rc = tbk_vo_proj_carry(ctx, S, 0, vo->orb, vo->orb_cnt, vo->matches, vo->mcounts, vo->Mcap, vo->kf_mp, vo->kf_valid, nullptr,
                               vo->kf_mp_desc, vo->kf_cnt, P, P, vo->inv_sigma2, p.nlevels, vo->win, vo->keys[b], vo->kcnt[b], vo->mp[b],
                               vo->valid[b], vo->mp_desc, vo->obs, vo->obs_counts, vo->outlier);
    }
    if (rc) return rc;
    if (t > 0 &&
        (rc = tb_pose_opt_batch_dev(ctx, S, p.K, vo->Tcw[a], vo->obs, vo->obs_counts, P, vo->outlier, vo->Tcw[b], vo->n_inliers, nullptr)))
        return rc;
    if (keyframe) {
        /* :577-634: the second ORB call returns the same keys (see vo_step_desc); stereo depths, the new map points */
        if ((rc = tbk_vo_copy_image(ctx, S, right, W, H, stride, pitch, vo->right))) return rc;
        if ((rc = tb_add_map_points_by_stereo_batch_dev(ctx, S, vo->right, vo->img[b], W, H, W, ip, &vo->cam, vo->keys[b], vo->kcnt[b], P, p.bf,
                                                        vo->st_pts, vo->st_status, vo->depth)))
            return rc;
        if ((rc = tbk_vo_kf_spawn(ctx, S, vo->keys[b], vo->kcnt[b], vo->depth, vo->Tcw[b], p.K, P, vo->mp[b], vo->valid[b]))) return rc;
        int slot = 0;
        if (map) {
            if (vo->map_nblk == vo->mapK) {   /* the oldest keyframe's points leave; the survivors move into the other set */
                const int c = vo->map_cur, d = c ^ 1;
                if ((rc = tbk_vo_map_evict(ctx, S, vo->map_rec[c], vo->map_desc[c], vo->map_n[c], vo->map_blocks[c], vo->mapK, vo->map_cap,
                                           vo->map_rec[d], vo->map_desc[d], vo->map_n[d], vo->map_blocks[d])))
                    return rc;
                vo->map_cur = d;
                vo->map_nblk = vo->mapK - 1;
            }
            slot = vo->map_nblk++;
        }
        const int c = vo->map_cur;
        if ((rc = tbk_vo_kf_append(ctx, S, vo->kcnt[b], vo->depth, vo->mp[b], vo->valid[b], vo->orb_desc, vo->Tcw[b], P, vo->mp_desc,
                                   map ? nullptr : vo->kf_rec, map ? vo->map_rec[c] : nullptr, map ? vo->map_desc[c] : nullptr,
                                   map ? vo->map_n[c] : nullptr, map ? vo->map_blocks[c] : nullptr, map ? vo->mapK : 0, slot, vo->map_cap)))
            return rc;
        /* key_frame = cur_frame_ptr (:641) */
        TB_HIP(ctx, hipMemcpyAsync(vo->kf_orb, vo->orb, SP * sizeof(tb_keypoint), hipMemcpyDeviceToDevice, ctx->stream));
        TB_HIP(ctx, hipMemcpyAsync(vo->kf_desc, vo->orb_desc, SP * 32, hipMemcpyDeviceToDevice, ctx->stream));
        TB_HIP(ctx, hipMemcpyAsync(vo->kf_cnt, vo->orb_cnt, (size_t)S * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
        TB_HIP(ctx, hipMemcpyAsync(vo->kf_mp, vo->mp[b], SP * 3 * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
        TB_HIP(ctx, hipMemcpyAsync(vo->kf_valid, vo->valid[b], SP, hipMemcpyDeviceToDevice, ctx->stream));
        TB_HIP(ctx, hipMemcpyAsync(vo->kf_mp_desc, vo->mp_desc, SP * 32, hipMemcpyDeviceToDevice, ctx->stream));
        vo->kf_frame = t;
    }
    return TB_OK;
}

/* The optical-flow tracker's frame t > 0 after the left images are in img[b]. */
static int vo_track_opflow(tb_vo* vo) {
    tb_ctx* ctx = vo->ctx;
    const tb_vo_params& p = vo->p;
    const int S = vo->nseq, P = vo->P, W = p.width, H = p.height;
    const size_t ip = (size_t)W * H;
    const int a = vo->cur, b = a ^ 1;
    int rc;
    /* test_vo.cpp:716: searchByOPFlow(cur, last, pts, true, true) -- the tracked points land in this frame's key list */
    if ((rc = tb_search_by_opflow_batch_dev(ctx, S, vo->img[b], vo->img[a], W, H, W, ip, &vo->cam, vo->keys[a], vo->kcnt[a], P, 1, 1,
                                            vo->keys[b], vo->status, vo->matches, P, vo->mcounts)))
        return rc;
    if ((rc = tbk_vo_track(ctx, S, vo->kcnt[a], vo->status, vo->keys[b], vo->mp[a], vo->valid[a], P, vo->kcnt[b], vo->mp[b], vo->valid[b],
                           vo->obs, vo->obs_counts, vo->outlier)))
        return rc;
    /* :761 LocalBA::PoseOptimization, started from the last frame's pose (:688) */
    return tb_pose_opt_batch_dev(ctx, S, p.K, vo->Tcw[a], vo->obs, vo->obs_counts, P, vo->outlier, vo->Tcw[b], vo->n_inliers, nullptr);
}

/* Frame t of every sequence (the arguments are checked): what tb_vo_step_dev launches. */
static int vo_step_lock(tb_vo* vo, int t, bool keyframe, const uint8_t* left, const uint8_t* right, int stride, size_t pitch) {
    tb_ctx* ctx = vo->ctx;
    const tb_vo_params& p = vo->p;
    const int S = vo->nseq, P = vo->P, W = p.width, H = p.height;
    const size_t ip = (size_t)W * H;
    const int a = vo->cur, b = a ^ 1;   /* a: last frame, b: this frame */
    int rc;
    if ((rc = tbk_vo_copy_image(ctx, S, left, W, H, stride, pitch, vo->img[b]))) return rc;
    if (vo->tr.kind != TB_VO_OPFLOW) {
        if ((rc = vo_is_proj(vo) ? vo_step_proj(vo, t, keyframe, right, stride, pitch) : vo_step_desc(vo, t, keyframe, right, stride, pitch)))
            return rc;
    } else if (t == 0) {
        TB_HIP(ctx, hipMemcpyAsync(vo->Tcw[b], vo->Tcw[a], (size_t)S * 16 * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
        TB_HIP(ctx, hipMemsetAsync(vo->kcnt[b], 0, (size_t)S * sizeof(int32_t), ctx->stream));
        TB_HIP(ctx, hipMemsetAsync(vo->obs_counts, 0, (size_t)S * sizeof(int32_t), ctx->stream));
        TB_HIP(ctx, hipMemsetAsync(vo->n_inliers, 0, (size_t)S * sizeof(int32_t), ctx->stream));
    } else if ((rc = vo_track_opflow(vo))) {
        return rc;
    }
    if (keyframe && vo->tr.kind == TB_VO_OPFLOW) {
        /* :774-785 ORB operator()(pyramid, sf, target, init_th, min_th) + SetKeys */
        if ((rc = tbk_vo_copy_image(ctx, S, right, W, H, stride, pitch, vo->right))) return rc;
        if ((rc = tb_extractor_set_images_dev(vo->ex, vo->img[b], S, W, ip))) return rc;
        if ((rc = tb_extractor_build_pyramid(vo->ex, S))) return rc;
        if ((rc = tb_extractor_orb(vo->ex, S, p.target, p.init_th, p.min_th, 0, nullptr, 0))) return rc;
        const tb_keypoint* kps = nullptr; const int32_t* cnt = nullptr; int selCap = 0;
        tb_extractor_results_dev(vo->ex, &kps, nullptr, &cnt, &selCap);
        if ((rc = tbk_vo_kf_pack(ctx, S, kps, cnt, selCap, P, vo->keys[b], vo->kcnt[b], vo->valid[b]))) return rc;
        /* :800 AddMapPointsByStereo(cur, right, d * fx, fx), then the new map points (:802-832) */
        if ((rc = tb_add_map_points_by_stereo_batch_dev(ctx, S, vo->right, vo->img[b], W, H, W, ip, &vo->cam, vo->keys[b], vo->kcnt[b], P, p.bf,
                                                        vo->st_pts, vo->st_status, vo->depth)))
            return rc;
        if ((rc = tbk_vo_kf_spawn(ctx, S, vo->keys[b], vo->kcnt[b], vo->depth, vo->Tcw[b], p.K, P, vo->mp[b], vo->valid[b]))) return rc;
    }
    vo->cur = b;
    vo->next = t + 1;
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
    if (keyframe && !right) return tb_fail(ctx, TB_EINVAL, "tb_vo_step_dev: frame %d is a keyframe and needs the right images", t);
    return vo_step_lock(vo, t, keyframe, left, right, stride, pitch);
}

/* ---- ragged batches: see include/tb_capi.h, tb_vo_step_ragged_dev */
static const char* vo_ragged_unsupported(const tb_vo* vo) {
    if (vo->tr.kind == TB_VO_PROJECTION_MAP) return "TB_VO_PROJECTION_MAP counts the map's blocks and evicts for the whole batch";
    if (vo->db) return "the keyframe database's ring slot is counted for the whole batch";
    return nullptr;
}

/* the per-frame outputs the loop owns, as a set */
static tb_vo_frame_out vo_frame_out(const tb_vo* vo) {
    tb_vo_frame_out o;
    o.obs = vo->obs; o.obs_counts = vo->obs_counts; o.outlier = vo->outlier; o.n_inliers = vo->n_inliers;
    if (vo->tr.kind != TB_VO_OPFLOW) {
        o.orb = vo->orb; o.orb_desc = vo->orb_desc; o.orb_cnt = vo->orb_cnt; o.matches = vo->matches; o.mcounts = vo->mcounts;
        o.mflags = vo->mflags; o.mp_desc = vo->mp_desc;
    }
    if (vo->tr.kind == TB_VO_BOW) {
        o.bow_word = vo->bow_word[0]; o.bow_node = vo->bow_node[0]; o.fv_keys = vo->fv_keys[0]; o.fv_cnt = vo->fv_cnt[0];
        o.bv_word = vo->bv_word[0]; o.bv_val = vo->bv_val[0]; o.bv_cnt = vo->bv_cnt[0];
    }
    return o;
}

/* The step writes the other set from now on; rg_prev keeps what the last step left. */
static void vo_swap_frame_out(tb_vo* vo) {
    const tb_vo_frame_out cur = vo_frame_out(vo), n = vo->rg_prev;
    vo->obs = n.obs; vo->obs_counts = n.obs_counts; vo->outlier = n.outlier; vo->n_inliers = n.n_inliers;
    if (vo->tr.kind != TB_VO_OPFLOW) {
        vo->orb = n.orb; vo->orb_desc = n.orb_desc; vo->orb_cnt = n.orb_cnt; vo->matches = n.matches; vo->mcounts = n.mcounts;
        vo->mflags = n.mflags; vo->mp_desc = n.mp_desc;
    }
    if (vo->tr.kind == TB_VO_BOW) {
        vo->bow_word[0] = n.bow_word; vo->bow_node[0] = n.bow_node; vo->fv_keys[0] = n.fv_keys; vo->fv_cnt[0] = n.fv_cnt;
        vo->bv_word[0] = n.bv_word; vo->bv_val[0] = n.bv_val; vo->bv_cnt[0] = n.bv_cnt;
    }
    vo->rg_prev = cur;
}

/* Everything ragged mode needs beyond the lock-step loop, allocated once (allocation synchronises; a step never grows it). */
static int vo_ragged_init(tb_vo* vo) {
    if (vo->rg_ready) return TB_OK;
    tb_ctx* ctx = vo->ctx;
    const size_t S = (size_t)vo->nseq, P = (size_t)vo->P, img = (size_t)vo->p.width * vo->p.height;
    tb_vo_frame_out& q = vo->rg_prev;
    TB_HIP(ctx, hipMalloc(&q.obs, S * P * sizeof(tb_obs)));
    TB_HIP(ctx, hipMalloc(&q.obs_counts, S * sizeof(int32_t)));
    TB_HIP(ctx, hipMalloc(&q.outlier, S * P));
    TB_HIP(ctx, hipMalloc(&q.n_inliers, S * sizeof(int32_t)));
    TB_HIP(ctx, hipMemsetAsync(q.obs_counts, 0, S * sizeof(int32_t), ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(q.n_inliers, 0, S * sizeof(int32_t), ctx->stream));
    if (vo->tr.kind != TB_VO_OPFLOW) {
        TB_HIP(ctx, hipMalloc(&q.orb, S * P * sizeof(tb_keypoint)));
        TB_HIP(ctx, hipMalloc(&q.orb_desc, S * P * 32));
        TB_HIP(ctx, hipMalloc(&q.orb_cnt, S * sizeof(int32_t)));
        TB_HIP(ctx, hipMalloc(&q.matches, S * (size_t)vo->Mcap * sizeof(tb_match)));
        TB_HIP(ctx, hipMalloc(&q.mcounts, S * sizeof(int32_t)));
        TB_HIP(ctx, hipMalloc(&q.mflags, S * sizeof(int32_t)));
        TB_HIP(ctx, hipMemsetAsync(q.orb_cnt, 0, S * sizeof(int32_t), ctx->stream));
        TB_HIP(ctx, hipMemsetAsync(q.mcounts, 0, S * sizeof(int32_t), ctx->stream));
        TB_HIP(ctx, hipMemsetAsync(q.mflags, 0, S * sizeof(int32_t), ctx->stream));
        if (vo->mp_desc) {
            TB_HIP(ctx, hipMalloc(&q.mp_desc, S * P * 32));
            TB_HIP(ctx, hipMemsetAsync(q.mp_desc, 0, S * P * 32, ctx->stream));
        }
    }
    if (vo->tr.kind == TB_VO_BOW) {
        TB_HIP(ctx, hipMalloc(&q.bow_word, S * P * sizeof(int32_t)));
        TB_HIP(ctx, hipMalloc(&q.bow_node, S * P * sizeof(int32_t)));
        TB_HIP(ctx, hipMalloc(&q.fv_keys, S * P * sizeof(uint64_t)));
        TB_HIP(ctx, hipMalloc(&q.fv_cnt, S * sizeof(int32_t)));
        TB_HIP(ctx, hipMalloc(&q.bv_word, S * P * sizeof(int32_t)));
        TB_HIP(ctx, hipMalloc(&q.bv_val, S * P * sizeof(double)));
        TB_HIP(ctx, hipMalloc(&q.bv_cnt, S * sizeof(int32_t)));
        TB_HIP(ctx, hipMemsetAsync(q.fv_cnt, 0, S * sizeof(int32_t), ctx->stream));
        TB_HIP(ctx, hipMemsetAsync(q.bv_cnt, 0, S * sizeof(int32_t), ctx->stream));
    }
    TB_HIP(ctx, hipMalloc(&vo->rg_left, S * img));
    TB_HIP(ctx, hipMalloc(&vo->rg_keys, S * P * 2 * sizeof(float)));
    TB_HIP(ctx, hipMalloc(&vo->rg_kcnt, S * sizeof(int32_t)));
    TB_HIP(ctx, hipMalloc(&vo->rg_dev, 2 * S * sizeof(int32_t)));
    TB_HIP(ctx, hipHostMalloc((void**)&vo->rg_pin, (size_t)tb_vo::RG_RING * 2 * S * sizeof(int32_t), hipHostMallocDefault));
    for (hipEvent_t& e : vo->rg_ev) TB_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
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
    int rc;
    if ((rc = vo_ragged_init(vo))) return rc;
    const int S = vo->nseq;
    int32_t* pin;
    if ((rc = vo_ragged_stage(vo, &pin))) return rc;
    for (int s = 0; s < S; s++) { pin[s] = which[s] ? 1 : 0; pin[S + s] = 0; }
    if ((rc = vo_ragged_upload(vo, pin))) return rc;
    const bool desc = vo->tr.kind != TB_VO_OPFLOW, bow = vo->tr.kind == TB_VO_BOW;
    if ((rc = tbk_vo_reset_seq(ctx, S, vo->rg_dev, Tcw0, vo->Tcw[vo->cur], vo->kcnt[vo->cur], desc ? vo->kf_cnt : nullptr,
                               bow ? vo->fv_cnt[1] : nullptr, bow ? vo->bv_cnt[1] : nullptr,
                               vo->tr.kind == TB_VO_VIOLENCE ? vo->kf_cell_start : nullptr, 4321)))
        return rc;
    for (int s = 0; s < S; s++)
        if (which[s]) { vo->seq_frame[s] = -1; vo->seq_kf_frame[s] = -1; vo->seq_reset[s] = 1; }
    vo->ragged = true;
    vo->next = 1 + *std::max_element(vo->seq_frame.begin(), vo->seq_frame.end());
    vo->kf_frame = *std::max_element(vo->seq_kf_frame.begin(), vo->seq_kf_frame.end());
    return TB_OK;
}

/* The keyframe block of a ragged step on the compacted batch of the nk sequences h_idx / d_idx name (ascending). */
static int vo_keyframe_ragged(tb_vo* vo, int nk, const int32_t* h_idx, const int32_t* d_idx, const uint8_t* right, int stride, size_t pitch) {
    tb_ctx* ctx = vo->ctx;
    const tb_vo_params& p = vo->p;
    const int P = vo->P, W = p.width, H = p.height, b = vo->cur;
    const size_t ip = (size_t)W * H;
    int rc;
    if ((rc = tbk_vo_copy_image(ctx, nk, right, W, H, stride, pitch, vo->right, d_idx))) return rc;
    if ((rc = tbk_vo_copy_image(ctx, nk, vo->img[b], W, H, W, ip, vo->rg_left, d_idx))) return rc;
    if (vo->tr.kind == TB_VO_OPFLOW) {
        if ((rc = tb_extractor_set_images_dev(vo->ex, vo->rg_left, nk, W, ip))) return rc;
        if ((rc = tb_extractor_build_pyramid(vo->ex, nk))) return rc;
        if ((rc = tb_extractor_orb(vo->ex, nk, p.target, p.init_th, p.min_th, 0, nullptr, 0))) return rc;
        const tb_keypoint* kps = nullptr; const int32_t* cnt = nullptr; int selCap = 0;
        tb_extractor_results_dev(vo->ex, &kps, nullptr, &cnt, &selCap);
        if ((rc = tbk_vo_kf_pack(ctx, nk, kps, cnt, selCap, P, vo->keys[b], vo->kcnt[b], vo->valid[b], d_idx))) return rc;
    }
    if ((rc = tbk_vo_kf_gather(ctx, nk, d_idx, vo->keys[b], vo->kcnt[b], P, vo->rg_keys, vo->rg_kcnt))) return rc;
    if ((rc = tb_add_map_points_by_stereo_batch_dev(ctx, nk, vo->right, vo->rg_left, W, H, W, ip, &vo->cam, vo->rg_keys, vo->rg_kcnt, P, p.bf,
                                                    vo->st_pts, vo->st_status, vo->depth)))
        return rc;
    if ((rc = tbk_vo_kf_spawn(ctx, nk, vo->keys[b], vo->kcnt[b], vo->depth, vo->Tcw[b], p.K, P, vo->mp[b], vo->valid[b], d_idx))) return rc;
    if (vo->tr.kind == TB_VO_OPFLOW) return TB_OK;
    if (vo->tr.kind == TB_VO_PROJECTION &&
        (rc = tbk_vo_kf_append(ctx, nk, vo->kcnt[b], vo->depth, vo->mp[b], vo->valid[b], vo->orb_desc, vo->Tcw[b], P, vo->mp_desc, vo->kf_rec,
                               nullptr, nullptr, nullptr, nullptr, 0, 0, vo->map_cap, d_idx)))
        return rc;
    /* key_frame = cur_frame_ptr for these sequences only */
    const tb_vo_frame_out cur = vo_frame_out(vo);
    tb_vo_kf_out kf;
    kf.orb = vo->kf_orb; kf.desc = vo->kf_desc; kf.cnt = vo->kf_cnt; kf.mp = vo->kf_mp; kf.valid = vo->kf_valid; kf.mp_desc = vo->kf_mp_desc;
    if (vo->tr.kind == TB_VO_BOW) {
        kf.bow_word = vo->bow_word[1]; kf.bow_node = vo->bow_node[1]; kf.fv_keys = vo->fv_keys[1]; kf.fv_cnt = vo->fv_cnt[1];
        kf.bv_word = vo->bv_word[1]; kf.bv_val = vo->bv_val[1]; kf.bv_cnt = vo->bv_cnt[1];
    }
    if ((rc = tbk_vo_kf_snapshot(ctx, nk, d_idx, P, &cur, vo->mp[b], vo->valid[b], &kf))) return rc;
    if (vo->tr.kind == TB_VO_VIOLENCE) {
        /* the keyframe's lookup grid, one call per run of neighbouring sequences */
        for (int j = 0; j < nk;) {
            int e = j + 1;
            while (e < nk && h_idx[e] == h_idx[e - 1] + 1) e++;
            const size_t s0 = (size_t)h_idx[j];
            if ((rc = tb_frame_grid_batch_dev(ctx, e - j, vo->kf_orb + s0 * P, vo->kf_cnt + s0, P, W, H, vo->kf_cell_start + s0 * 4321,
                                              vo->kf_cell_items + s0 * P)))
                return rc;
            j = e;
        }
    }
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
    int rc;
    if (nact == S && same_t && (nkf == 0 || nkf == S)) {
        /* every sequence at the same frame with the same decision: this is tb_vo_step_dev's step, launch for launch */
        if ((rc = vo_step_lock(vo, t0, nkf == S, left, right, stride, pitch))) return rc;
        if (vo->ragged) vo->kf_frame = *std::max_element(vo->seq_kf_frame.begin(), vo->seq_kf_frame.end());
        return TB_OK;
    }
    if ((rc = vo_ragged_init(vo))) return rc;
    /* the masks, known to the host, go up in one copy; nothing is decided on the device and nothing is read back */
    int32_t* pin;
    if ((rc = vo_ragged_stage(vo, &pin))) return rc;
    nkf = 0;
    for (int s = 0; s < S; s++) {
        const bool act = !active || active[s];
        const int t = vo->seq_frame[s] + 1;
        pin[s] = act ? (t == 0 ? 2 : 1) : 0;
        if (act && (t % p.keyframe_every == 0 || (force_keyframe && force_keyframe[s]))) pin[S + nkf++] = s;
    }
    for (int j = nkf; j < S; j++) pin[S + j] = 0;
    if ((rc = vo_ragged_upload(vo, pin))) return rc;
    const int P = vo->P, W = p.width, H = p.height;
    const int a = vo->cur, b = a ^ 1;
    if ((rc = tbk_vo_copy_image(ctx, S, left, W, H, stride, pitch, vo->img[b]))) return rc;
    /* the tracking half over all sequences, as frame t > 0 of the lock-step loop, into the other set of per-frame outputs: a
     * sequence without keys or keyframe gets no match, no row and keeps its pose; an idle one is restored below */
    vo_swap_frame_out(vo);
    if (vo->tr.kind == TB_VO_OPFLOW) rc = vo_track_opflow(vo);
    else if (vo_is_proj(vo)) rc = vo_step_proj(vo, 1, false, nullptr, 0, 0);
    else rc = vo_step_desc(vo, 1, false, nullptr, 0, 0);
    if (rc) { vo_swap_frame_out(vo); return rc; }
    tb_vo_hold_args h;
    h.mask = vo->rg_dev; h.pitch = P; h.match_pitch = vo->Mcap; h.npx = (size_t)W * H;
    h.img[0] = vo->img[a]; h.img[1] = vo->img[b]; h.keys[0] = vo->keys[a]; h.keys[1] = vo->keys[b]; h.mp[0] = vo->mp[a]; h.mp[1] = vo->mp[b];
    h.valid[0] = vo->valid[a]; h.valid[1] = vo->valid[b]; h.kcnt[0] = vo->kcnt[a]; h.kcnt[1] = vo->kcnt[b];
    h.Tcw[0] = vo->Tcw[a]; h.Tcw[1] = vo->Tcw[b];
    h.prev = vo->rg_prev; h.cur = vo_frame_out(vo);
    if ((rc = tbk_vo_hold(ctx, S, &h))) return rc;
    vo->cur = b;
    if (nkf && (rc = vo_keyframe_ragged(vo, nkf, pin + S, vo->rg_dev + S, right, stride, pitch))) return rc;
    for (int s = 0; s < S; s++)
        if (pin[s]) vo->seq_frame[s]++;
    for (int j = 0; j < nkf; j++) vo->seq_kf_frame[pin[S + j]] = vo->seq_frame[pin[S + j]];
    vo->ragged = true;
    vo->next = 1 + *std::max_element(vo->seq_frame.begin(), vo->seq_frame.end());
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
    if (Tcw) *Tcw = vo->Tcw[c];
    if (keys_xy) *keys_xy = vo->keys[c];
    if (map_points) *map_points = vo->mp[c];
    if (mp_valid) *mp_valid = vo->valid[c];
    if (key_counts) *key_counts = vo->kcnt[c];
    if (obs) *obs = vo->obs;
    if (obs_counts) *obs_counts = vo->obs_counts;
    if (n_inliers) *n_inliers = vo->n_inliers;
    if (outlier) *outlier = vo->outlier;
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
    if (orb) *orb = vo->orb;
    if (orb_desc) *orb_desc = vo->orb_desc;
    if (orb_counts) *orb_counts = vo->orb_cnt;
    if (matches) *matches = vo->matches;
    if (match_counts) *match_counts = vo->mcounts;
    if (flags) *flags = vo->mflags;
    if (kf_orb) *kf_orb = vo->kf_orb;
    if (kf_desc) *kf_desc = vo->kf_desc;
    if (kf_map_points) *kf_map_points = vo->kf_mp;
    if (kf_mp_valid) *kf_mp_valid = vo->kf_valid;
    if (kf_counts) *kf_counts = vo->kf_cnt;
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
    if (fv_keys) *fv_keys = vo->fv_keys[0];
    if (fv_counts) *fv_counts = vo->fv_cnt[0];
    if (bv_words) *bv_words = vo->bv_word[0];
    if (bv_values) *bv_values = vo->bv_val[0];
    if (bv_counts) *bv_counts = vo->bv_cnt[0];
    if (word_ids) *word_ids = vo->bow_word[0];
    if (node_ids) *node_ids = vo->bow_node[0];
    if (kf_fv_keys) *kf_fv_keys = vo->fv_keys[1];
    if (kf_fv_counts) *kf_fv_counts = vo->fv_cnt[1];
    if (kf_bv_words) *kf_bv_words = vo->bv_word[1];
    if (kf_bv_values) *kf_bv_values = vo->bv_val[1];
    if (kf_bv_counts) *kf_bv_counts = vo->bv_cnt[1];
    if (kf_word_ids) *kf_word_ids = vo->bow_word[1];
    if (kf_node_ids) *kf_node_ids = vo->bow_node[1];
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
    int rc = tb_kf_store_create(ctx, vo->nseq, vo->db->cap, vo->P, max_candidates, &vo->store);
    if (rc) return rc;
    const size_t S = (size_t)vo->nseq;
    TB_HIP(ctx, hipMalloc(&vo->rl_scores, S * vo->db->cap * sizeof(double)));
    TB_HIP(ctx, hipMalloc(&vo->rl_top_score, S * max_candidates * sizeof(double)));
    TB_HIP(ctx, hipMalloc(&vo->rl_top_slot, S * max_candidates * sizeof(int32_t)));
    TB_HIP(ctx, hipMalloc(&vo->rl_top_kf, S * max_candidates * sizeof(int32_t)));
    return TB_OK;
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
    int rc = tb_bow_db_query_dev(vo->db, vo->bv_word[0], vo->bv_val[0], vo->bv_cnt[0], vo->P, exclude_newest, topk, scores, top_slot, top_kf,
                                 top_score, top_count);
    if (rc) return rc;
    tb_reloc_params prm;
    prm.map_point_only = vo->bw.map_point_only; prm.th_low = vo->bw.th_low; prm.nratio = vo->bw.nratio; prm.histo_len = vo->bw.histo_len;
    prm.check_orientation = vo->bw.check_orientation; prm.min_inliers = min_inliers;
    return tb_relocalize_batch_dev(vo->store, vo->p.K, vo->p.nlevels, vo->p.scale, vo->orb, vo->orb_desc, vo->orb_cnt, vo->fv_keys[0],
                                   vo->fv_cnt[0], vo->P, top_slot, topk, &prm, out);
}

int tb_vo_recover_enable(tb_vo* vo, const tb_vo_recover* prm) {
    TB_ENTER((vo ? vo->ctx : nullptr));
    if (!vo) return TB_EINVAL;
    tb_ctx* ctx = vo->ctx;
    if (!vo->store) return tb_fail(ctx, TB_ESTATE, "tb_vo_recover_enable: relocalisation is not enabled (tb_vo_reloc_enable)");
    if (vo->next > 0) return tb_fail(ctx, TB_ESTATE, "tb_vo_recover_enable after a step (frame %d)", vo->next - 1);
    if (vo->rec_on) return tb_fail(ctx, TB_ESTATE, "tb_vo_recover_enable: recovery is enabled already");
    if (!prm) return tb_fail(ctx, TB_EINVAL, "tb_vo_recover_enable: null parameters");
    if (prm->lost_inliers < 0 || prm->min_inliers < 0 || prm->exclude_newest < 0 || prm->topk < 1 || prm->topk > vo->store->max_cand)
        return tb_fail(ctx, TB_EINVAL, "tb_vo_recover_enable: lost_inliers %d, topk %d (1..%d), exclude_newest %d, min_inliers %d",
                       prm->lost_inliers, prm->topk, vo->store->max_cand, prm->exclude_newest, prm->min_inliers);
    const size_t S = (size_t)vo->nseq, ring = S * vo->store->cap * vo->P;
    TB_HIP(ctx, hipMalloc(&vo->rc_lost, S));
    TB_HIP(ctx, hipMalloc(&vo->rc_track, S * sizeof(int32_t)));
    TB_HIP(ctx, hipMalloc(&vo->rc_kf, S * sizeof(int32_t)));
    TB_HIP(ctx, hipMalloc(&vo->rc_kf_ids, S * sizeof(int32_t)));
    TB_HIP(ctx, hipMalloc(&vo->rc_best_rank, S * sizeof(int32_t)));
    TB_HIP(ctx, hipMalloc(&vo->rc_best_kf, S * sizeof(int32_t)));
    TB_HIP(ctx, hipMalloc(&vo->rc_best_Tcw, S * 16 * sizeof(float)));
    TB_HIP(ctx, hipMalloc(&vo->rc_masked, S * prm->topk * sizeof(int32_t)));
    TB_HIP(ctx, hipMalloc(&vo->rc_word_ring, ring * sizeof(int32_t)));
    TB_HIP(ctx, hipMalloc(&vo->rc_node_ring, ring * sizeof(int32_t)));
    int rc = vo_recover_clear(vo);
    if (rc) return rc;
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
    if (mp_desc) *mp_desc = vo->mp_desc;
    if (kf_mp_desc) *kf_mp_desc = vo->kf_mp_desc;
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

}  // extern "C"
