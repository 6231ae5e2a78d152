// acq_lowres.hip - acquisition straight from the LOW-resolution classifier logits on gfx950 (MI355X): the tile scorers, the scores and
// the class probabilities at listed pixels, and the body every low-resolution *_topk entry shares (run_lowres_select; acq_mc.hip's
// entries go through it too).  The selection itself is acq_topk.hip's; acq_device.h and acq_host.h state what crosses.
#include <cmath>

#include "acq_host.h"
#include "acq_score.h"
#include "lowres_tile.h"

namespace pp {

// ---- SURVEY.md §8f-1 -----------------------------------------------------------------------------------
// Replaces  deeplab.py:55-56  F.interpolate(pred, size=inputs.shape[2:], mode='bilinear', align_corners=True)
//        +  query.py:190      softmax(model(x)["pred"][:, :, :h, :w])  + score + exclusion + top-k
// without ever writing the full-resolution logits (10 MB per 256x512x19 image written and read back; the algorithmic
// input drops 16x to the 64x128x19 classifier output).  A block owns a 64-column x 4*PPT-row LowresTile (lowres_tile.h) of
// OUTPUT pixels, stages the low-resolution patch the tile interpolates from in LDS ((4*PPT*s+2) x (64*s+2) pixels, 13.7 KB at
// s = 1/4), and every lane interpolates its pixels' class vectors from the tile's taps - the same bits pp_bilinear_fwd writes -
// then scores them like acq_kernel.  Wave w of the tile owns PPT consecutive rows, so the row weights are wave-uniform.

template <int CMAX, bool EXACT, int PPT, bool LDS, int MATH, int STRAT = -1>
__global__ __launch_bounds__(kBlock, 2) void acq_lowres_kernel(LowresParams p)
{
    extern __shared__ __attribute__((aligned(16))) float s_patch[];
    __shared__ uint64_t s_surv[kBlock / kWave][kSurvCap];
    __shared__ uint32_t s_cnt[kBlock / kWave];
    __shared__ uint64_t s_top[(kBlock / kWave) * kSmallKMax];
    const int tiles = p.tiles_x * p.tiles_y;
    const int img = blockIdx.x / tiles;
    const int t = blockIdx.x - img * tiles;
    const int ty = t / p.tiles_x, tx = t - ty * p.tiles_x;
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    // large-k selection: the block counts its scores into the image's histogram (as acq_kernel<..., HIST>; bins in the survivor lists)
    uint32_t* qbins = p.qhist ? reinterpret_cast<uint32_t*>(&s_surv[0][0]) : nullptr;
    if (qbins) {
        for (int i = tid; i < kQBins; i += kBlock) qbins[i] = 0u;
        __syncthreads();
    }
    const int C = EXACT ? CMAX : p.C;
    const bool largest = p.strategy != PP_ACQ_MARGIN;
    const float fill = largest ? 0.0f : 1.0f;
    const int64_t N = (int64_t)p.Hc * p.Wc;
    LowresTile<LDS> tile(p, C, tx, ty, (kBlock / kWave) * PPT, kBlock);
    const float* base = p.low + (int64_t)img * p.h * p.w * p.ldx;
    if constexpr (LDS) {
        tile.stage(p, s_patch, base);
        __syncthreads();
    }
    tile.set_lane(p, lane);
    const uint8_t* excl = p.exclude ? p.exclude + (int64_t)img * N : nullptr;
    float* omap = p.out_map ? p.out_map + (int64_t)img * N : nullptr;
    const float* src = LDS ? s_patch : base;

    uint32_t kh[PPT], kl[PPT];
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const int Y = tile.Y0 + wv * PPT + j;
        if (Y < p.Hc && tile.xin) {
            float x[CMAX];
            const auto tp = tile.taps(src, tile.row(p, Y));
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                if (EXACT || c < C) x[c] = tp.at(c);
            float sc;
            if constexpr (MATH == 0) sc = pixel_score_fast<CMAX, EXACT, STRAT>(x, p.C, p.strategy);
            else sc = pixel_score<CMAX, EXACT>(x, p.C, p.strategy, 0);
            lowres_emit_key(sc, (int64_t)Y * p.Wc + tile.X, largest, fill, excl, omap, qbins, p.qscale, kh[j], kl[j]);
        } else {
            kh[j] = 0u; kl[j] = 0u;
        }
        __builtin_amdgcn_sched_barrier(0);   // one pixel's class vector live at a time
    }
    if (qbins) {
        lowres_hist_flush(qbins, p.qhist + (int64_t)img * kQBins);
        return;
    }
    if (p.cand)
        block_emit_topk<PPT>(kh, kl, p.k, p.cand + ((int64_t)img * tiles + t) * p.k, p.reduce_mode, s_surv, s_cnt, s_top);
}

// The strategy's score at a list of picked pixels (QueryStats: entropy at the queried pixels, query.py:262-266),
// interpolated from the low-resolution logits with the same arithmetic.  One thread per pixel.
template <int CMAX, bool EXACT>
__global__ __launch_bounds__(kBlock) void acq_lowres_at_kernel(const float* low, int64_t ldx, int h, int w, float sh,
                                                             float sw, int align, int Wc, int C, int strategy,
                                                             const int32_t* img_idx, const int32_t* pix_idx,
                                                             int64_t n, float* out)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int pix = pix_idx[i], Y = pix / Wc, X = pix - Y * Wc;
    const Lerp lh = lerp_src(Y, h, sh, align), lw = lerp_src(X, w, sw, align);
    const float* base = low + (int64_t)img_idx[i] * h * w * ldx;
    float x[CMAX];
    const auto tp = lowres_taps(base, ldx, w, lh, lw);
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
        if (EXACT || c < C) x[c] = tp.at(c);
    out[i] = pixel_score_fast<CMAX, EXACT>(x, C, strategy);
}

// LowresTile<false> (PPT = 4, no LDS patch): every class of a pixel is interpolated from the four low-resolution neighbours in
// memory on each pass (LowresTaps::at(): the bits pp_bilinear_fwd writes)
template <int MATH>
__global__ __launch_bounds__(kBlock) void acq_lowres_stream_kernel(LowresParams p)
{
    constexpr int PPT = 4;
    __shared__ uint64_t s_surv[kBlock / kWave][kSurvCap];
    __shared__ uint32_t s_cnt[kBlock / kWave];
    __shared__ uint64_t s_top[(kBlock / kWave) * kSmallKMax];
    const int tiles = p.tiles_x * p.tiles_y;
    const int img = blockIdx.x / tiles;
    const int t = blockIdx.x - img * tiles;
    const int ty = t / p.tiles_x, tx = t - ty * p.tiles_x;
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool largest = p.strategy != PP_ACQ_MARGIN;
    const float fill = largest ? 0.0f : 1.0f;
    const int64_t N = (int64_t)p.Hc * p.Wc;
    LowresTile<false> tile(p, p.C, tx, ty, (kBlock / kWave) * PPT, kBlock);
    tile.set_lane(p, lane);
    const float* base = p.low + (int64_t)img * p.h * p.w * p.ldx;
    const uint8_t* excl = p.exclude ? p.exclude + (int64_t)img * N : nullptr;
    float* omap = p.out_map ? p.out_map + (int64_t)img * N : nullptr;
    uint32_t kh[PPT], kl[PPT];
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const int Y = tile.Y0 + wv * PPT + j;
        if (Y < p.Hc && tile.xin) {
            const auto tp = tile.taps(base, tile.row(p, Y));
            float s[1];
            score_stream<1, MATH>([&](int c, float (&v)[1]) { v[0] = tp.at(c); }, p.C, p.strategy, s);
            lowres_emit_key(s[0], (int64_t)Y * p.Wc + tile.X, largest, fill, excl, omap, nullptr, 0.0f, kh[j], kl[j]);
        } else {
            kh[j] = 0u; kl[j] = 0u;
        }
    }
    if (p.cand)
        block_emit_topk<PPT>(kh, kl, p.k, p.cand + ((int64_t)img * tiles + t) * p.k, p.reduce_mode, s_surv, s_cnt, s_top);
}

__global__ __launch_bounds__(kBlock) void acq_lowres_at_stream_kernel(const float* low, int64_t ldx, int h, int w, float sh, float sw,
                                                                     int align, int Wc, int C, int strategy, const int32_t* img_idx,
                                                                     const int32_t* pix_idx, int64_t n, float* out)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int pix = pix_idx[i], Y = pix / Wc, X = pix - Y * Wc;
    const Lerp lh = lerp_src(Y, h, sh, align), lw = lerp_src(X, w, sw, align);
    const float* base = low + (int64_t)img_idx[i] * h * w * ldx;
    const auto tp = lowres_taps(base, ldx, w, lh, lw);
    float s[1];
    score_stream<1, 0>([&](int c, float (&v)[1]) { v[0] = tp.at(c); }, C, strategy, s);
    out[i] = s[0];
}

// ---- pp_acq_lowres_prob_at_u8: the class probabilities at listed pixels as bytes (include/pixelpick_hip.h) -------------------
// pp_acq_lowres_score_at's sibling: one thread per listed pixel, the class vector interpolated with the same taps, the softmax with the
// scorer's arithmetic (acq_score.h: m = max, e_c = fast_exp(x_c - m), S = sum e_c in class order, p_c = e_c / S).  A row leaves as whole
// dwords, four codes each; an entry outside the batch or the crop writes a zero row and never reads `low`.
__device__ __forceinline__ uint32_t prob_code(float e, float S)
{
    const float v = 255.0f * (e / S);
    return v == v ? (uint32_t)min(255, (int)rintf(v)) : 0u;      // NaN -> 0
}

// true: entry i is in range; otherwise its row was zeroed here
__device__ __forceinline__ bool prob_at_entry(int img, int pix, int B, int npix, uint32_t* row, int ldw)
{
    if (img >= 0 && img < B && pix >= 0 && pix < npix) return true;
    for (int j = 0; j < ldw; ++j) row[j] = 0u;
    return false;
}

template <int CMAX, bool EXACT>
__global__ __launch_bounds__(kBlock) void prob_at_kernel(const float* low, int64_t ldx, int B, int h, int w, float sh, float sw, int align,
                                                       int Wc, int npix, int C_, const int32_t* img_idx, const int32_t* pix_idx, int64_t n,
                                                       uint32_t* out, int ldw)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int C = EXACT ? CMAX : C_;
    const int img = img_idx[i], pix = pix_idx[i];
    uint32_t* row = out + i * ldw;
    if (!prob_at_entry(img, pix, B, npix, row, ldw)) return;
    const int Y = pix / Wc, X = pix - Y * Wc;
    const Lerp lh = lerp_src(Y, h, sh, align), lw = lerp_src(X, w, sw, align);
    const float* base = low + (int64_t)img * h * w * ldx;
    float x[CMAX];
    const auto tp = lowres_taps(base, ldx, w, lh, lw);
    lowres_class_vector<CMAX, EXACT>(tp, C, x);
    float m = x[0];
#pragma unroll
    for (int c = 1; c < CMAX; ++c)
        if (EXACT || c < C) m = fmaxf(m, x[c]);
    float S = 0.0f;
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
        if (EXACT || c < C) {
            x[c] = fast_exp(x[c] - m);
            S += x[c];
        }
    constexpr int kWords = (CMAX + 3) / 4;
#pragma unroll
    for (int j = 0; j < kWords; ++j) {
        uint32_t word = 0u;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int c = 4 * j + b;
            if (c < CMAX && (EXACT || c < C)) word |= prob_code(x[c], S) << (8 * b);
        }
        if (j < ldw) row[j] = word;
    }
    for (int j = kWords; j < ldw; ++j) row[j] = 0u;
}

// heads wider than the register forms: three passes over the pixel's classes (max, sum, emit), the later ones served by L2; the same
// expressions in the same order - forced onto a C <= 64 input the bytes are those of prob_at_kernel
__global__ __launch_bounds__(kBlock) void prob_at_stream_kernel(const float* low, int64_t ldx, int B, int h, int w, float sh, float sw,
                                                              int align, int Wc, int npix, int C, const int32_t* img_idx,
                                                              const int32_t* pix_idx, int64_t n, uint32_t* out, int ldw)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int img = img_idx[i], pix = pix_idx[i];
    uint32_t* row = out + i * ldw;
    if (!prob_at_entry(img, pix, B, npix, row, ldw)) return;
    const int Y = pix / Wc, X = pix - Y * Wc;
    const Lerp lh = lerp_src(Y, h, sh, align), lw = lerp_src(X, w, sw, align);
    const float* base = low + (int64_t)img * h * w * ldx;
    const auto tp = lowres_taps(base, ldx, w, lh, lw);
    float m = tp.at(0);
    for (int c = 1; c < C; ++c) m = fmaxf(m, tp.at(c));
    float S = 0.0f;
    for (int c = 0; c < C; ++c) S += fast_exp(tp.at(c) - m);
    for (int j = 0; j < ldw; ++j) {
        uint32_t word = 0u;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int c = 4 * j + b;
            if (c < C) word |= prob_code(fast_exp(tp.at(c) - m), S) << (8 * b);
        }
        row[j] = word;
    }
}

// ---- low-resolution path: host side ---------------------------------------------------------------------
constexpr size_t kLowresLdsMax = 54 * 1024;      // + 8.2 KB of static survivor lists = the 64 KB a block may ask for
constexpr size_t kLowresLdsSoft = 32 * 1024;     // above this the 32-row tile gives way to the 16-row tile

LowresPlan make_lowres_plan(int64_t B, int64_t C, int64_t h, int64_t w, int64_t Hc, int64_t Wc, float sh, float sw, bool force_ppt4)
{
    LowresPlan pl;
    const int64_t tiles8 = cdiv(Wc, kWave) * cdiv(Hc, (kBlock / kWave) * 8);
    pl.ppt = (!force_ppt4 && B * tiles8 * (kBlock / kWave) >= 2048) ? 8 : 4;
    // x2 models (FPNSeg, decoders.py:101): a 32-row tile interpolates from 19 x 35 source pixels = 50.5 KB at C = 19; the 16-row
    // tile's patch (29 KB) keeps the LDS path and two more blocks per CU
    if (pl.ppt == 8 && g_knobs.tune_ppt != 8) {      // pp_debug_set_acq_tuning(., 4 | 8) forces a tile height (A/B)
        if ((size_t)lowres_patch_floats(sh, sw, h, w, (kBlock / kWave) * 8, C) * 4 > kLowresLdsSoft) pl.ppt = 4;
    }
    if (g_knobs.tune_ppt == 4) pl.ppt = 4;
    pl.tiles_x = (int)cdiv(Wc, kWave);
    pl.tiles_y = (int)cdiv(Hc, (kBlock / kWave) * pl.ppt);
    pl.waves_per_image = pl.tiles_x * pl.tiles_y;      // candidate lists per image: one per block (tile)
    const int64_t fl = lowres_patch_floats(sh, sw, h, w, (kBlock / kWave) * pl.ppt, C);
    pl.lds = (size_t)fl * 4 <= kLowresLdsMax;
    pl.patch_cap = pl.lds ? (int)fl : 0;
    pl.lds_bytes = pl.lds ? (size_t)fl * 4 : 0;
    return pl;
}

template <int CMAX, bool EXACT>
static int launch_lowres(const LowresParams& p, const LowresPlan& pl, int64_t B, hipStream_t st)
{
    EventScope ev(st);
    dim3 grid((unsigned)(B * pl.tiles_x * pl.tiles_y)), block(kBlock);
    if (exact_formula()) {        // reference operation order: 4-row variant only
        if (pl.lds) hipLaunchKernelGGL((acq_lowres_kernel<CMAX, EXACT, 4, true, 1>), grid, block, pl.lds_bytes, st, p);
        else        hipLaunchKernelGGL((acq_lowres_kernel<CMAX, EXACT, 4, false, 1>), grid, block, 0, st, p);
    } else if (EXACT && pl.lds && g_knobs.acq_strat_spec) {
        // the dataset class counts with the patch in LDS (every production shape): strategy-specialised scorer (this kernel is VALU-bound)
        by_strategy(p.strategy, [&](auto s) {
            constexpr int S = decltype(s)::value;
            if (pl.ppt == 8) hipLaunchKernelGGL((acq_lowres_kernel<CMAX, EXACT, 8, true, 0, S>), grid, block, pl.lds_bytes, st, p);
            else             hipLaunchKernelGGL((acq_lowres_kernel<CMAX, EXACT, 4, true, 0, S>), grid, block, pl.lds_bytes, st, p);
        });
    } else if (pl.ppt == 8) {
        if (pl.lds) hipLaunchKernelGGL((acq_lowres_kernel<CMAX, EXACT, 8, true, 0>), grid, block, pl.lds_bytes, st, p);
        else        hipLaunchKernelGGL((acq_lowres_kernel<CMAX, EXACT, 8, false, 0>), grid, block, 0, st, p);
    } else {
        if (pl.lds) hipLaunchKernelGGL((acq_lowres_kernel<CMAX, EXACT, 4, true, 0>), grid, block, pl.lds_bytes, st, p);
        else        hipLaunchKernelGGL((acq_lowres_kernel<CMAX, EXACT, 4, false, 0>), grid, block, 0, st, p);
    }
    return check_launch("acq_lowres_kernel");
}

static int dispatch_lowres(const LowresParams& p, const LowresPlan& pl, int64_t B, hipStream_t st)
{
    if (stream_classes(p.C)) {
        EventScope ev(st);
        if (pl.ppt != 4) return fail(PP_ERR_BAD_ARG, "streamed low-resolution scorer: plan with %d rows per wave", pl.ppt);
        dim3 grid((unsigned)(B * pl.tiles_x * pl.tiles_y)), block(kBlock);
        if (exact_formula()) hipLaunchKernelGGL((acq_lowres_stream_kernel<1>), grid, block, 0, st, p);
        else                 hipLaunchKernelGGL((acq_lowres_stream_kernel<0>), grid, block, 0, st, p);
        return check_launch("acq_lowres_stream_kernel");
    }
    return lowres_by_classes(p.C, [&](auto cmax, auto exact) { return launch_lowres<decltype(cmax)::value, decltype(exact)::value>(p, pl, B, st); });
}

int validate_lowres(const float* low, int64_t ldx, int64_t B, int64_t C, int64_t h, int64_t w, int64_t H, int64_t W, int64_t Hc, int64_t Wc,
                    int strategy)
{
    if (int rc = validate(low, B, C, Hc, Wc, strategy)) return rc;
    if (h < 1 || w < 1 || H < 1 || W < 1) return fail(PP_ERR_BAD_ARG, "bad low-res/full-res shape %lldx%lld -> %lldx%lld",
                                                    (long long)h, (long long)w, (long long)H, (long long)W);
    if (Hc > H || Wc > W) return fail(PP_ERR_BAD_ARG, "crop %lldx%lld exceeds the interpolated size %lldx%lld", (long long)Hc,
                                      (long long)Wc, (long long)H, (long long)W);
    if (ldx < C) return fail(PP_ERR_BAD_ARG, "ldx=%lld < C=%lld", (long long)ldx, (long long)C);
    if (B * h * w * ldx > 0x7FFFFFFFFFFFll) return fail(PP_ERR_UNSUPPORTED, "low-res tensor too large");
    return PP_OK;
}

// The body the four low-resolution *_topk entries share, after their own validation.  `launch` runs the entry's scorer with the
// finished p (plan, map, candidate lists or histogram filled in): map only (k == 0); k <= 48: per-tile candidate lists + merge;
// larger k: the score map (the caller's, or the workspace's) + the large-k selection on it at `qscale`, with the quantised
// histogram counted by the scorer itself where the entry allows it (hist_ok).
int run_lowres_select(LowresParams& p, const LowresPlan& pl, int64_t B, int64_t k, int32_t* out_idx, float* out_val, void* workspace,
                      size_t ws_bytes, hipStream_t st, float qscale, bool hist_ok, const std::function<int()>& launch)
{
    const int64_t N = (int64_t)p.Hc * p.Wc;
    p.tiles_x = pl.tiles_x; p.tiles_y = pl.tiles_y; p.patch_cap = pl.patch_cap;
    if (k == 0) {     // score map only
        if (!p.out_map) return fail(PP_ERR_BAD_ARG, "k == 0 (map only) needs out_map");
        return launch();
    }
    if (int rc = check_select_args(k, N, "H*W", out_idx, workspace, ws_bytes, pp_acq_lowres_workspace_bytes(B, p.C, p.Hc, p.Wc, k))) return rc;
    const int largest = p.strategy != PP_ACQ_MARGIN;
    if (k <= kSmallKMax) {
        const SmallKLists ws = small_k_lists(workspace, B, pl.waves_per_image, k);
        p.cand = ws.cand;
        p.k = (int)k;
        if (int rc = launch()) return rc;
        return run_merge(ws.cand, ws.n_cand, ws.other, B, (int)k, largest, out_idx, out_val, st);
    }
    float* map = p.out_map ? p.out_map : reinterpret_cast<float*>(workspace);
    uint64_t* gbuf = reinterpret_cast<uint64_t*>(reinterpret_cast<char*>(workspace) + align_up((size_t)B * N * 4, 256));
    p.out_map = map;
    if (hist_ok) {
        p.qhist = large_hist(gbuf, B, k);
        p.qscale = qscale;
        if (hipMemsetAsync(p.qhist, 0, (size_t)B * kQBins * 4, st) != hipSuccess) return fail(PP_ERR_LAUNCH, "topk: memset failed");
    }
    if (int rc = launch()) return rc;
    return run_large(map, B, N, k, largest, gbuf, out_idx, out_val, st, qscale, hist_ok);
}

LowresParams make_lowres_params(const float* low, int64_t ldx, const uint8_t* exclude, float* out_map, int64_t C, int64_t h, int64_t w,
                                int64_t H, int64_t W, int align_corners, int64_t Hc, int64_t Wc, int strategy)
{
    LowresParams p{};
    p.low = low; p.ldx = ldx; p.exclude = exclude; p.out_map = out_map;
    p.h = (int)h; p.w = (int)w; p.Hc = (int)Hc; p.Wc = (int)Wc;
    lowres_scales(h, w, H, W, align_corners, p.sh, p.sw);
    p.align = align_corners ? 1 : 0;
    p.C = (int)C; p.strategy = strategy; p.reduce_mode = g_knobs.reduce_mode;
    return p;
}

int lowres_at_begin(const char* who, int64_t h, int64_t w, int64_t H, int64_t W, int align_corners, const int32_t* img_idx,
                    const int32_t* pix_idx, const void* out, int64_t n, LowresAt& at)
{
    at.any = n != 0;
    if (!at.any) return PP_OK;
    if (n < 0 || !img_idx || !pix_idx || !out) return fail(PP_ERR_BAD_ARG, "%s: null pointer or n < 0", who);
    lowres_scales(h, w, H, W, align_corners, at.sh, at.sw);
    at.align = align_corners ? 1 : 0;
    at.grid = dim3((unsigned)cdiv(n, kBlock));
    return PP_OK;
}

}  // namespace pp

using namespace pp;

extern "C" {

size_t pp_acq_lowres_workspace_bytes(int64_t B, int64_t C, int64_t Hc, int64_t Wc, int64_t k)
{
    (void)C;
    if (B < 1 || Hc < 1 || Wc < 1 || k < 1 || Hc > 0x7FFFFFFFll || Wc > 0x7FFFFFFFll || Hc * Wc > 0x7FFFFFFFll || k > Hc * Wc || B > 0x7FFFFFFFll) return 0;
    if (k <= kSmallKMax) {   // sized for the 4-row tile (most waves)
        const int64_t waves = cdiv(Wc, kWave) * cdiv(Hc, (kBlock / kWave) * 4) * (kBlock / kWave);
        return merge_ws_bytes(B, waves * k, k);
    }
    return align_up((size_t)B * Hc * Wc * 4, 256) + pp_topk_workspace_bytes(B, Hc * Wc, k);
}

int pp_acq_lowres_score_topk(const float* low, int64_t ldx, int64_t B, int64_t C, int64_t h, int64_t w, int64_t H,
                             int64_t W, int align_corners, int64_t Hc, int64_t Wc, const uint8_t* exclude, int strategy,
                             int64_t k, int32_t* out_idx, float* out_val, float* out_map, void* workspace,
                             size_t ws_bytes, pp_stream_t stream)
{
    const ExactScope exact_scope(strategy);
    if (int rc = validate_lowres(low, ldx, B, C, h, w, H, W, Hc, Wc, strategy)) return rc;
    hipStream_t st = as_stream(stream);
    LowresParams p = make_lowres_params(low, ldx, exclude, out_map, C, h, w, H, W, align_corners, Hc, Wc, strategy);
    const LowresPlan pl = make_lowres_plan(B, C, h, w, Hc, Wc, p.sh, p.sw, exact_formula() != 0 || stream_classes(C));
    const float qs = score_qscale(strategy, C);
    const bool hist_ok = g_knobs.hist_fuse && large_q_ok(B, k, qs) && !stream_classes(C);      // (acq_lowres_kernel only: the streamed form has no histogram epilogue)
    return run_lowres_select(p, pl, B, k, out_idx, out_val, workspace, ws_bytes, st, qs, hist_ok, [&] { return dispatch_lowres(p, pl, B, st); });
}

int pp_acq_lowres_score_at(const float* low, int64_t ldx, int64_t B, int64_t C, int64_t h, int64_t w, int64_t H,
                           int64_t W, int align_corners, int64_t Hc, int64_t Wc, int strategy, const int32_t* img_idx,
                           const int32_t* pix_idx, int64_t n, float* out, pp_stream_t stream)
{
    const ExactScope exact_scope(strategy);
    if (int rc = validate_lowres(low, ldx, B, C, h, w, H, W, Hc, Wc, strategy)) return rc;
    LowresAt at;
    if (int rc = lowres_at_begin("score_at", h, w, H, W, align_corners, img_idx, pix_idx, out, n, at)) return rc;
    if (!at.any) return PP_OK;
    hipStream_t st = as_stream(stream);
    const dim3 block(kBlock);
    if (stream_classes(C)) {
        hipLaunchKernelGGL(acq_lowres_at_stream_kernel, at.grid, block, 0, st, low, ldx, (int)h, (int)w, at.sh, at.sw, at.align, (int)Wc, (int)C,
                           strategy, img_idx, pix_idx, n, out);
        return check_launch("acq_lowres_at_stream_kernel");
    }
    lowres_by_classes(C, [&](auto cmax, auto exact) {
        hipLaunchKernelGGL((acq_lowres_at_kernel<decltype(cmax)::value, decltype(exact)::value>), at.grid, block, 0, st, low, ldx, (int)h, (int)w,
                           at.sh, at.sw, at.align, (int)Wc, (int)C, strategy, img_idx, pix_idx, n, out);
        return 0;
    });
    return check_launch("acq_lowres_at_kernel");
}

int pp_acq_lowres_prob_at_u8(const float* low, int64_t ldx, int64_t B, int64_t C, int64_t h, int64_t w, int64_t H, int64_t W,
                             int align_corners, int64_t Hc, int64_t Wc, const int32_t* img_idx, const int32_t* pix_idx, int64_t n,
                             uint8_t* out, int64_t ldf, pp_stream_t stream)
{
    if (int rc = validate_lowres(low, ldx, B, C, h, w, H, W, Hc, Wc, PP_ACQ_ENTROPY)) return rc;
    if (C > 256) return fail(PP_ERR_UNSUPPORTED, "prob_at_u8: C=%lld > 256 classes", (long long)C);
    if (B > 0x7FFFFFFFll) return fail(PP_ERR_UNSUPPORTED, "prob_at_u8: B=%lld > 2^31 - 1 images", (long long)B);
    if (ldf < C || ldf % 4 != 0 || ldf > 0x7FFFFFFFll)
        return fail(PP_ERR_BAD_ARG, "prob_at_u8: ldf=%lld must be a multiple of 4 and at least C=%lld", (long long)ldf, (long long)C);
    if (reinterpret_cast<uintptr_t>(out) % 4 != 0) return fail(PP_ERR_BAD_ARG, "prob_at_u8: out is not 4-byte aligned");
    LowresAt at;
    if (int rc = lowres_at_begin("prob_at_u8", h, w, H, W, align_corners, img_idx, pix_idx, out, n, at)) return rc;
    if (!at.any) return PP_OK;
    if (cdiv(n, kBlock) > 0x7FFFFFFFll) return fail(PP_ERR_UNSUPPORTED, "prob_at_u8: n=%lld listed pixels", (long long)n);
    hipStream_t st = as_stream(stream);
    const dim3 block(kBlock);
    uint32_t* out32 = reinterpret_cast<uint32_t*>(out);
    if (stream_classes(C)) {
        hipLaunchKernelGGL(prob_at_stream_kernel, at.grid, block, 0, st, low, ldx, (int)B, (int)h, (int)w, at.sh, at.sw, at.align, (int)Wc,
                           (int)(Hc * Wc), (int)C, img_idx, pix_idx, n, out32, (int)(ldf / 4));
        return check_launch("prob_at_stream_kernel");
    }
    lowres_by_classes(C, [&](auto cmax, auto exact) {
        hipLaunchKernelGGL((prob_at_kernel<decltype(cmax)::value, decltype(exact)::value>), at.grid, block, 0, st, low, ldx, (int)B, (int)h,
                           (int)w, at.sh, at.sw, at.align, (int)Wc, (int)(Hc * Wc), (int)C, img_idx, pix_idx, n, out32, (int)(ldf / 4));
        return 0;
    });
    return check_launch("prob_at_kernel");
}

}  // extern "C"
