// acq_mc.hip - MC-dropout acquisition on gfx950 (MI355X), three families: the mean over the passes of the strategy's score, the hard
// vote, and the scores of the mean probability with BALD - each from the classifier-resolution logits (one LowresTile per block) and,
// for the hard vote and the mean probability, on the full-size route's accumulated tensors.  The *_topk entries end in acq_lowres.hip's
// run_lowres_select; acq_device.h and acq_host.h state what crosses.
#include <cmath>

#include "acq_host.h"
#include "acq_score.h"
#include "lowres_tile.h"

namespace pp {

// ---- MC-dropout acquisition from the low-resolution classifier output (query.py:177-187) --------------------------------
// The mean over T stochastic passes of the strategy's score, without the T full-resolution logit tensors (T x 10 MB per 256x512x19
// image written by pp_bilinear_fwd and read back by softmax_sum_kernel): one LowresTile, its patch staged once per pass.  `low`
// is image-major, passes t = 0..T-1 of image b are entries b*T + t.  Per pass every lane interpolates its pixels' class vectors
// from the tile's taps and adds mc_pass_score() - softmax_sum_kernel's arithmetic - to a per-pixel register accumulator;
// scale * sum and the selection tail (lowres_emit_key) follow.  A shape whose patch does not fit the LDS a block may ask for
// (make_lowres_plan) runs the LDS = false form, which reads the four neighbours from memory; that the patch fits patch_cap is the
// HOST's guarantee here (lowres_patch_floats()): the one tile kernel that stages without the frame's capacity trap.
struct LowresMcParams {
    LowresParams g;      // low: [B*T,h,w,ldx]
    int T;
    float scale;
};

template <int CMAX, bool EXACT, int PPT, bool LDS, int STRAT>
__global__ __launch_bounds__(kBlock, 2) void acq_lowres_mc_kernel(LowresMcParams q)
{
    extern __shared__ __attribute__((aligned(16))) float s_patch[];
    __shared__ uint64_t s_surv[kBlock / kWave][kSurvCap];
    __shared__ uint32_t s_cnt[kBlock / kWave];
    __shared__ uint64_t s_top[(kBlock / kWave) * kSmallKMax];
    const LowresParams& p = q.g;
    const int tiles = p.tiles_x * p.tiles_y;
    const int img = blockIdx.x / tiles;
    const int t = blockIdx.x - img * tiles;
    const int ty = t / p.tiles_x, tx = t - ty * p.tiles_x;
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
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
    tile.set_lane(p, lane);
    const int64_t pass_stride = (int64_t)p.h * p.w * p.ldx;
    const float* img_base = p.low + (int64_t)img * q.T * pass_stride;

    float uc[PPT];
#pragma unroll
    for (int j = 0; j < PPT; ++j) uc[j] = 0.0f;
    for (int ps = 0; ps < q.T; ++ps) {
        const float* base = img_base + (int64_t)ps * pass_stride;
        if constexpr (LDS) {
            if (ps) __syncthreads();          // every wave has finished reading the previous pass's patch
            // tile.stage() spelled out, without its capacity trap: in this kernel the trap costs the generic forms 36 B of scratch and
            // the call <21, 4 rows, entropy> a wave per SIMD (profiles/lowres_tile_resources.txt)
            const int n = tile.ph * tile.pw * C;
            for (int e = tid; e < n; e += kBlock) {
                const int pc = e / C, ch = e - pc * C;
                const int r = pc / tile.pw, c = pc - r * tile.pw;
                s_patch[pc * (C | 1) + ch] = base[((int64_t)(tile.r_lo + r) * p.w + tile.c_lo + c) * p.ldx + ch];
            }
            __syncthreads();
        }
        const float* src = LDS ? s_patch : base;
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            const int Y = tile.Y0 + wv * PPT + j;
            if (Y < p.Hc && tile.xin) {
                float x[CMAX];
                const auto tp = tile.taps(src, tile.row(p, Y));
#pragma unroll
                for (int c = 0; c < CMAX; ++c)
                    if (EXACT || c < C) x[c] = tp.at(c);
                uc[j] += mc_pass_score<STRAT, CMAX, EXACT>([&](int c) { return x[c]; }, C, p.strategy, [](int, float) {});
            }
            __builtin_amdgcn_sched_barrier(0);   // one pixel's class vector live at a time
        }
    }

    const uint8_t* excl = p.exclude ? p.exclude + (int64_t)img * N : nullptr;
    float* omap = p.out_map ? p.out_map + (int64_t)img * N : nullptr;
    uint32_t kh[PPT], kl[PPT];
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const int Y = tile.Y0 + wv * PPT + j;
        if (Y < p.Hc && tile.xin) {
            lowres_emit_key(q.scale * uc[j], (int64_t)Y * p.Wc + tile.X, largest, fill, excl, omap, qbins, p.qscale, kh[j], kl[j]);
        } else {
            kh[j] = 0u; kl[j] = 0u;
        }
    }
    if (qbins) {
        lowres_hist_flush(qbins, p.qhist + (int64_t)img * kQBins);
        return;
    }
    if (p.cand)
        block_emit_topk<PPT>(kh, kl, p.k, p.cand + ((int64_t)img * tiles + t) * p.k, p.reduce_mode, s_surv, s_cnt, s_top);
}

// The strategy's score OF THE MEAN PROBABILITY over the T passes at listed pixels: p_c = scale * sum_t softmax(x_t)_c, accumulated
// as softmax_sum_kernel accumulates its per-class sums, then pp_uncertainty_from_prob's formulas (QueryStats._get_entropy(query,
// prob) at the picked pixels only, query.py:262-264).  One thread per pixel.
template <int CMAX, bool EXACT>
__global__ __launch_bounds__(kBlock) void acq_lowres_mc_at_kernel(const float* low, int64_t ldx, int T, int h, int w, float sh, float sw,
                                                                int align, int Wc, int C, int strategy, float scale,
                                                                const int32_t* img_idx, const int32_t* pix_idx, int64_t n, float* out)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int pix = pix_idx[i], Y = pix / Wc, X = pix - Y * Wc;
    const Lerp lh = lerp_src(Y, h, sh, align), lw = lerp_src(X, w, sw, align);
    const int64_t pass_stride = (int64_t)h * w * ldx;
    const float* base = low + (int64_t)img_idx[i] * T * pass_stride;
    float acc[CMAX];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) acc[c] = 0.0f;
    for (int t = 0; t < T; ++t) {
        float x[CMAX];
        const auto tp = lowres_taps(base + (int64_t)t * pass_stride, ldx, w, lh, lw);
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
            if (EXACT || c < C) x[c] = tp.at(c);
        // (STRAT = least-confidence: only the probabilities are wanted here, no logf per pass)
        (void)mc_pass_score<PP_ACQ_LEAST_CONFIDENCE, CMAX, EXACT>([&](int c) { return x[c]; }, C, 0, [&](int c, float pc) { acc[c] += pc; });
    }
#pragma unroll
    for (int c = 0; c < CMAX; ++c) acc[c] = scale * acc[c];
    out[i] = pixel_score<CMAX, EXACT>(acc, C, strategy, 1);
}

// ---- MC-dropout HARD vote (args.py:34 --vote_type hard; query.py:31,177-187) ----------------------------------------------
// Query by committee: pass t votes for a_t = argmax_c x_t[c] (exactly equal logits: the LOWEST class index), n_c = #{t : a_t = c},
// n_(1) >= n_(2) the two largest counts, and the pixel's score is a function of the counts alone:
//   entropy           float(sum_c tab[n_c]) * 2^-24, tab[n] = llrint(-(n/T) ln(n/T) 2^24) built in double on the HOST (tab[0] = 0) and
//                     summed as integers: a function of the multiset of counts, no device logf, the same bits in any restatement
//   least-confidence  float(T - n_(1)) / float(T)        margin  float(n_(1) - n_(2)) / float(T)       (one IEEE division each)
// Excluded pixels get -1.0 (entropy, least-confidence) / 2.0 (margin), NOT the soft scorers' 0.0 / 1.0: those are the scores of every
// unanimous pixel, and an excluded pixel must sort strictly behind every un-excluded one.  Scores take few distinct values, so most
// picks are decided by the tie rule (lower flat index first); no NaN can occur.  T <= 255: the counts are bytes.
// The table travels BY VALUE in the kernel arguments (1 KB, no host-to-device copy: the call stays recordable by csrc/plan.hip).
struct VoteTable { uint32_t v[256]; };

__device__ __forceinline__ float vote_score(int strategy, uint32_t n1, uint32_t n2, uint32_t ent_q, int T)
{
    if (strategy == PP_ACQ_ENTROPY) return (float)ent_q * 5.9604644775390625e-08f;            // 2^-24: exact
    const uint32_t num = strategy == PP_ACQ_LEAST_CONFIDENCE ? (uint32_t)T - n1 : n1 - n2;
    return __fdiv_rn((float)num, (float)T);
}
__device__ __forceinline__ float vote_fill(int strategy) { return strategy != PP_ACQ_MARGIN ? -1.0f : 2.0f; }

// acq_lowres_mc_kernel's pass loop over one LowresTile and its selection tail; per pass a running maximum in
// ascending class order (strict >: the lowest class wins ties) and ONE vote into the pixel's counters - bytes packed four to a
// 32-bit register, (CMAX+3)/4 words per pixel, bumped by an unrolled compare-and-add (no run-time register index: no scratch).
// No expf / logf in the pass loop.  The table is staged once per block into the survivor lists' LDS (free until block_emit_topk).
struct LowresVoteParams {
    LowresParams g;      // low: [B*T,h,w,ldx]; qhist unused (k > 48: the map, then the generic selection)
    int T;
    VoteTable tab;
};

template <int CMAX, bool EXACT, int PPT, bool LDS>
__global__ __launch_bounds__(kBlock, 2) void acq_lowres_mc_vote_kernel(LowresVoteParams q)
{
    extern __shared__ __attribute__((aligned(16))) float s_patch[];
    __shared__ uint64_t s_surv[kBlock / kWave][kSurvCap];
    __shared__ uint32_t s_cnt[kBlock / kWave];
    __shared__ uint64_t s_top[(kBlock / kWave) * kSmallKMax];
    const LowresParams& p = q.g;
    constexpr int NW = (CMAX + 3) / 4;
    const int tiles = p.tiles_x * p.tiles_y;
    const int img = blockIdx.x / tiles;
    const int t = blockIdx.x - img * tiles;
    const int ty = t / p.tiles_x, tx = t - ty * p.tiles_x;
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int C = EXACT ? CMAX : p.C;
    const bool largest = p.strategy != PP_ACQ_MARGIN;
    const int64_t N = (int64_t)p.Hc * p.Wc;
    LowresTile<LDS> tile(p, C, tx, ty, (kBlock / kWave) * PPT, kBlock);
    tile.set_lane(p, lane);
    const int64_t pass_stride = (int64_t)p.h * p.w * p.ldx;
    const float* img_base = p.low + (int64_t)img * q.T * pass_stride;

    uint32_t cnt[PPT][NW];
#pragma unroll
    for (int j = 0; j < PPT; ++j)
#pragma unroll
        for (int i = 0; i < NW; ++i) cnt[j][i] = 0u;
    for (int ps = 0; ps < q.T; ++ps) {
        const float* base = img_base + (int64_t)ps * pass_stride;
        if constexpr (LDS) {
            if (ps) __syncthreads();          // every wave has finished reading the previous pass's patch
            tile.stage(p, s_patch, base);
            __syncthreads();
        }
        const float* src = LDS ? s_patch : base;
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            const int Y = tile.Y0 + wv * PPT + j;
            if (Y < p.Hc && tile.xin) {
                const auto tp = tile.taps(src, tile.row(p, Y));
                float best = tp.at(0);
                int bi = 0;
#pragma unroll
                for (int c = 1; c < CMAX; ++c)
                    if (EXACT || c < C) {
                        const float v = tp.at(c);
                        if (v > best) { best = v; bi = c; }
                    }
                const uint32_t inc = 1u << ((bi & 3) * 8);
                const int wd = bi >> 2;
#pragma unroll
                for (int i = 0; i < NW; ++i) cnt[j][i] += wd == i ? inc : 0u;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    uint32_t* s_tab = reinterpret_cast<uint32_t*>(&s_surv[0][0]);
    static_assert(kBlock == 256, "one table entry per thread");
    s_tab[tid] = q.tab.v[tid];
    __syncthreads();
    const uint8_t* excl = p.exclude ? p.exclude + (int64_t)img * N : nullptr;
    float* omap = p.out_map ? p.out_map + (int64_t)img * N : nullptr;
    const bool want_ent = p.strategy == PP_ACQ_ENTROPY;
    uint32_t kh[PPT], kl[PPT];
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const int Y = tile.Y0 + wv * PPT + j;
        if (Y < p.Hc && tile.xin) {
            uint32_t n1 = 0u, n2 = 0u, eq = 0u;
#pragma unroll
            for (int c = 0; c < CMAX; ++c) {
                const uint32_t n = (cnt[j][c >> 2] >> ((c & 3) * 8)) & 0xFFu;      // classes beyond C hold 0 votes: tab[0] = 0
                n2 = max(n2, min(n1, n));
                n1 = max(n1, n);
                if (want_ent) eq += s_tab[n];
            }
            lowres_emit_key(vote_score(p.strategy, n1, n2, eq, q.T), (int64_t)Y * p.Wc + tile.X, largest, vote_fill(p.strategy), excl, omap,
                            nullptr, 0.0f, kh[j], kl[j]);
        } else {
            kh[j] = 0u; kl[j] = 0u;
        }
    }
    if (p.cand) {
        __syncthreads();                      // the table's LDS becomes the survivor lists
        block_emit_topk<PPT>(kh, kl, p.k, p.cand + ((int64_t)img * tiles + t) * p.k, p.reduce_mode, s_surv, s_cnt, s_top);
    }
}

// ---- MC-dropout: scores of the MEAN PROBABILITY over the passes, and BALD ----------------------------------------------------
// p_c = scale * sum_t softmax(x_t)_c (fp32, ascending t, one multiply: softmax_sum_kernel's prob_out), then
//   entropy / least-confidence / margin   pixel_score(p, from_prob = 1): pp_uncertainty_from_prob's formulas on the consensus
//   PP_ACQ_BALD                           H(p) - scale * sum_t H(p_t): the second term is softmax_sum_kernel's uc_out for the entropy
//                                         strategy; ONE subtraction, not clamped (rounding may leave it a few ulp below 0)
// Excluded pixels get the hard vote's fills: 0.0 is the BALD of every deterministic pixel.
__device__ __forceinline__ float mean_fill(int strategy) { return strategy != PP_ACQ_MARGIN ? -1.0f : 2.0f; }

// psum: the per-class sums over the passes, hsum: the sum of the per-pass entropies (BALD only)
template <int CMAX, bool EXACT>
__device__ __forceinline__ float mean_prob_score(const float (&psum)[CMAX], int C, int strategy, float hsum, float scale)
{
#pragma clang fp contract(off)      // the mean entropy and the difference are rounded separately, as the two launches of the full-size route do
    float pm[CMAX];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) pm[c] = scale * psum[c];
    if (strategy != PP_ACQ_BALD) return pixel_score<CMAX, EXACT>(pm, C, strategy, 1);
    const float mean_ent = scale * hsum;
    return pixel_score<CMAX, EXACT>(pm, C, PP_ACQ_ENTROPY, 1) - mean_ent;
}

// mc_pass_score's arithmetic with the class vector RE-READ for the maximum, the sum and the probabilities instead of held in
// registers (that function's CMAX == 0 form: expf evaluated twice per class, the same value both times), but unrolled to CMAX with a
// per-class predicate, so that on_prob(c, p_c) meets the caller's accumulators at constant indices.  Returns the pass's entropy (ENT).
// The compiler barriers keep the three sweeps apart: merged, they are the register form again, with the class vector live beside
// the accumulators.
template <bool ENT, int CMAX, typename X, typename P>
__device__ __forceinline__ float mc_pass_probs_streamed(X x, int C, P on_prob)
{
    float m = x(0);
#pragma unroll
    for (int c = 1; c < CMAX; ++c)
        if (c < C) m = fmaxf(m, x(c));
    asm volatile("" ::: "memory");
    float S = 0.0f;
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
        if (c < C) S += expf(x(c) - m);
    asm volatile("" ::: "memory");
    float ent = 0.0f;
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
        if (c < C) {
            const float pc = expf(x(c) - m) / S;
            on_prob(c, pc);
            if (ENT) ent = fmaf(-pc, logf(pc), ent);
        }
    return ent;
}

// acq_lowres_mc_kernel's tile (4 rows per wave) and selection tail with per-class accumulators.  Two loop orders:
//   LDS   passes outer (the patch is staged once per pass), rows inner: 4 x CMAX accumulators per lane; CMAX <= 32
//   !LDS  rows outer, passes inner, taps read from memory: CMAX accumulators per lane - the form of the <= 64 instantiation, whose
//         4 x 64 accumulators would not fit the register file, and of every shape whose patch does not fit the LDS
// Either way a pixel's sums grow in ascending t.  BALD: the per-pass entropy is kept as well (logf per class and pass); the
// other three strategies run no logf in the pass loop.  The final formula's strategy is a run-time value.
template <int CMAX, bool EXACT, bool LDS, bool BALD>
__global__ __launch_bounds__(kBlock, 2) void acq_lowres_mc_mean_kernel(LowresMcParams q)
{
    extern __shared__ __attribute__((aligned(16))) float s_patch[];
    __shared__ uint64_t s_surv[kBlock / kWave][kSurvCap];
    __shared__ uint32_t s_cnt[kBlock / kWave];
    __shared__ uint64_t s_top[(kBlock / kWave) * kSmallKMax];
    static_assert(!LDS || CMAX <= 32, "the LDS form keeps 4 x CMAX accumulators");
    constexpr int PPT = 4;
    constexpr int kPass = BALD ? PP_ACQ_ENTROPY : PP_ACQ_LEAST_CONFIDENCE;      // what mc_pass_score computes beside the probabilities
    const LowresParams& p = q.g;
    const int tiles = p.tiles_x * p.tiles_y;
    const int img = blockIdx.x / tiles;
    const int t = blockIdx.x - img * tiles;
    const int ty = t / p.tiles_x, tx = t - ty * p.tiles_x;
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int C = EXACT ? CMAX : p.C;
    const bool largest = p.strategy != PP_ACQ_MARGIN;
    const float fill = mean_fill(p.strategy);
    const int64_t N = (int64_t)p.Hc * p.Wc;
    LowresTile<LDS> tile(p, C, tx, ty, (kBlock / kWave) * PPT, kBlock);
    tile.set_lane(p, lane);
    const int64_t pass_stride = (int64_t)p.h * p.w * p.ldx;
    const float* img_base = p.low + (int64_t)img * q.T * pass_stride;
    const uint8_t* excl = p.exclude ? p.exclude + (int64_t)img * N : nullptr;
    float* omap = p.out_map ? p.out_map + (int64_t)img * N : nullptr;
    uint32_t kh[PPT], kl[PPT];

    if constexpr (LDS) {
        float acc[PPT][CMAX], hs[PPT];
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            hs[j] = 0.0f;
#pragma unroll
            for (int c = 0; c < CMAX; ++c) acc[j][c] = 0.0f;
        }
        for (int ps = 0; ps < q.T; ++ps) {
            const float* base = img_base + (int64_t)ps * pass_stride;
            if (ps) __syncthreads();          // every wave has finished reading the previous pass's patch
            // acq_lowres_mc_kernel's staging loop (the patch fits patch_cap by the host's lowres_patch_floats())
            const int n = tile.ph * tile.pw * C;
            for (int e = tid; e < n; e += kBlock) {
                const int pc = e / C, ch = e - pc * C;
                const int r = pc / tile.pw, c = pc - r * tile.pw;
                s_patch[pc * (C | 1) + ch] = base[((int64_t)(tile.r_lo + r) * p.w + tile.c_lo + c) * p.ldx + ch];
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < PPT; ++j) {
                const int Y = tile.Y0 + wv * PPT + j;
                if (Y < p.Hc && tile.xin) {
                    float x[CMAX];
                    const auto tp = tile.taps(s_patch, tile.row(p, Y));
#pragma unroll
                    for (int c = 0; c < CMAX; ++c)
                        if (EXACT || c < C) x[c] = tp.at(c);
                    const float e = mc_pass_score<kPass, CMAX, EXACT>([&](int c) { return x[c]; }, C, 0, [&](int c, float pc) { acc[j][c] += pc; });
                    if (BALD) hs[j] += e;
                }
                __builtin_amdgcn_sched_barrier(0);   // one pixel's class vector live at a time
            }
        }
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            const int Y = tile.Y0 + wv * PPT + j;
            if (Y < p.Hc && tile.xin) {
                lowres_emit_key(mean_prob_score<CMAX, EXACT>(acc[j], C, p.strategy, hs[j], q.scale), (int64_t)Y * p.Wc + tile.X, largest, fill,
                                excl, omap, nullptr, 0.0f, kh[j], kl[j]);
            } else {
                kh[j] = 0u; kl[j] = 0u;
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            const int Y = tile.Y0 + wv * PPT + j;
            if (Y < p.Hc && tile.xin) {
                float acc[CMAX], hs = 0.0f;
#pragma unroll
                for (int c = 0; c < CMAX; ++c) acc[c] = 0.0f;
                const Lerp lh = tile.row(p, Y);
                for (int ps = 0; ps < q.T; ++ps) {
                    const auto tp = tile.taps(img_base + (int64_t)ps * pass_stride, lh);
                    float e;
                    if constexpr (CMAX > 32) {      // 64 accumulators: no room for the class vector beside them
                        e = mc_pass_probs_streamed<BALD, CMAX>([&](int c) { return tp.at(c); }, C, [&](int c, float pc) { acc[c] += pc; });
                    } else {
                        float x[CMAX];
#pragma unroll
                        for (int c = 0; c < CMAX; ++c)
                            if (EXACT || c < C) x[c] = tp.at(c);
                        e = mc_pass_score<kPass, CMAX, EXACT>([&](int c) { return x[c]; }, C, 0, [&](int c, float pc) { acc[c] += pc; });
                    }
                    if (BALD) hs += e;
                }
                lowres_emit_key(mean_prob_score<CMAX, EXACT>(acc, C, p.strategy, hs, q.scale), (int64_t)Y * p.Wc + tile.X, largest, fill, excl,
                                omap, nullptr, 0.0f, kh[j], kl[j]);
            } else {
                kh[j] = 0u; kl[j] = 0u;
            }
            __builtin_amdgcn_sched_barrier(0);   // one pixel's accumulators live at a time
        }
    }
    if (p.cand)
        block_emit_topk<PPT>(kh, kl, p.k, p.cand + ((int64_t)img * tiles + t) * p.k, p.reduce_mode, s_surv, s_cnt, s_top);
}

// Full-size route, any class count and any strides: the same scores from a GIVEN mean probability prob [B,C,H,W] (what
// softmax_sum_kernel's prob_out holds) and, for BALD, the mean per-pass entropy mean_ent [B,N] (its uc_out).  One thread per pixel
// streams the classes in class order - pixel_score(from_prob = 1)'s operations, so the map equals pp_uncertainty_from_prob's bit
// for bit at the class counts that entry scores from registers.
struct MeanMapParams {
    const float* prob;
    const float* mean_ent;    // [B,N]: BALD only
    const uint8_t* exclude;   // [B,N] or null
    float* out_map;           // [B,N]
    int64_t N, sB, sC, sH, sW;
    int C, W, strategy;
};

__global__ __launch_bounds__(kBlock) void mean_prob_score_kernel(MeanMapParams p)
{
#pragma clang fp contract(off)      // as pixel_score
    const int64_t pix = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (pix >= p.N) return;
    const int64_t img = blockIdx.y, o = img * p.N + pix;
    const int64_t hh = pix / p.W, ww = pix - hh * p.W;
    const float* x = p.prob + img * p.sB + hh * p.sH + ww * p.sW;
    float sc;
    if (p.strategy == PP_ACQ_ENTROPY || p.strategy == PP_ACQ_BALD) {
        float acc = 0.0f;
        for (int c = 0; c < p.C; ++c) {
            const float v = x[(int64_t)c * p.sC];
            acc += (-v) * logf(v);
        }
        sc = p.strategy == PP_ACQ_BALD ? acc - p.mean_ent[o] : acc;
    } else {
        float t1 = -INFINITY, t2 = -INFINITY;
        for (int c = 0; c < p.C; ++c) {
            const float v = x[(int64_t)c * p.sC];
            t2 = fmaxf(t2, fminf(t1, v));
            t1 = fmaxf(t1, v);
        }
        sc = p.strategy == PP_ACQ_LEAST_CONFIDENCE ? 1.0f - t1 : fabsf(t1 - t2);
    }
    if (p.exclude && p.exclude[o]) sc = mean_fill(p.strategy);
    p.out_map[o] = sc;
}

// Full-size route, any class count: votes u8 [C,N] (+)= the per-class vote counts of the T passes in logits [T,C,H,W] (element
// strides).  One thread per pixel streams the classes with the running best and bumps ONE byte per pass.
__global__ __launch_bounds__(kBlock) void vote_accumulate_kernel(const float* logits, int T, int C, int W, int64_t N, int64_t sT, int64_t sC,
                                                                int64_t sH, int64_t sW, uint8_t* votes, int accumulate)
{
    const int64_t pix = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (pix >= N) return;
    const int64_t hh = pix / W, ww = pix - hh * W;
    const float* base = logits + hh * sH + ww * sW;
    if (!accumulate)
        for (int c = 0; c < C; ++c) votes[(int64_t)c * N + pix] = 0;
    for (int t = 0; t < T; ++t) {
        const float* xt = base + (int64_t)t * sT;
        float best = xt[0];
        int bi = 0;
        for (int c = 1; c < C; ++c) {
            const float v = xt[(int64_t)c * sC];
            if (v > best) { best = v; bi = c; }
        }
        uint8_t* slot = votes + (int64_t)bi * N + pix;
        *slot = (uint8_t)(*slot + 1u);
    }
}

struct VoteScoreParams {
    const uint8_t* votes;     // [B,C,N]
    const uint8_t* exclude;   // [B,N] or null
    float* out_map;           // [B,N]
    int64_t N;
    int C, T, strategy;
    VoteTable tab;
};

__global__ __launch_bounds__(kBlock) void vote_score_kernel(VoteScoreParams p)
{
    __shared__ uint32_t s_tab[256];
    s_tab[threadIdx.x] = p.tab.v[threadIdx.x];
    __syncthreads();
    const int64_t pix = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (pix >= p.N) return;
    const int64_t img = blockIdx.y;
    const uint8_t* v = p.votes + img * p.C * p.N + pix;
    uint32_t n1 = 0u, n2 = 0u, eq = 0u;
    for (int c = 0; c < p.C; ++c) {
        const uint32_t n = v[(int64_t)c * p.N];
        n2 = max(n2, min(n1, n));
        n1 = max(n1, n);
        eq += s_tab[n];
    }
    float sc = vote_score(p.strategy, n1, n2, eq, p.T);
    if (p.exclude && p.exclude[img * p.N + pix]) sc = vote_fill(p.strategy);
    p.out_map[img * p.N + pix] = sc;
}

// ---- MC-dropout low-resolution path: host side ---------------------------------------------------------
static int validate_lowres_mc(const float* low, int64_t ldx, int64_t B, int64_t T, int64_t C, int64_t h, int64_t w, int64_t H,
                              int64_t W, int64_t Hc, int64_t Wc, int strategy)
{
    if (T < 1 || T > 0x7FFFFFFFll) return fail(PP_ERR_BAD_ARG, "bad number of passes T=%lld", (long long)T);
    if (int rc = validate_lowres(low, ldx, B, C, h, w, H, W, Hc, Wc, strategy)) return rc;
    if (C > PP_ACQ_MAX_CLASSES)
        return fail(PP_ERR_UNSUPPORTED, "MC-dropout low-resolution scorer: C=%lld > %d classes", (long long)C, PP_ACQ_MAX_CLASSES);
    if (h * w * ldx > 0x7FFFFFFFFFFFll / (B * T)) return fail(PP_ERR_UNSUPPORTED, "low-res tensor too large");
    return PP_OK;
}

// make_lowres_plan's tile, except that the 8-row tile is kept for the dataset class counts with the patch in LDS: the generic
// instantiations (per-class predicates) and the form that reads from memory run the 4-row tile only (no scratch in any form)
static LowresPlan make_lowres_mc_plan(int64_t B, int64_t C, int64_t h, int64_t w, int64_t Hc, int64_t Wc, float sh, float sw)
{
    LowresPlan pl = make_lowres_plan(B, C, h, w, Hc, Wc, sh, sw, !(C == 11 || C == 19 || C == 21));
    if (!pl.lds && pl.ppt != 4) pl = make_lowres_plan(B, C, h, w, Hc, Wc, sh, sw, true);
    return pl;
}

template <int CMAX, bool EXACT>
static int launch_lowres_mc(const LowresMcParams& q, const LowresPlan& pl, int64_t B, hipStream_t st)
{
    EventScope ev(st);
    dim3 grid((unsigned)(B * pl.tiles_x * pl.tiles_y)), block(kBlock);
    // strategy-specialised: the least-confidence and margin kernels carry no logf
    auto go = [&](auto rows, auto lds) {
        constexpr int P = decltype(rows)::value;
        constexpr bool L = decltype(lds)::value;
        by_strategy(q.g.strategy, [&](auto s) {
            hipLaunchKernelGGL((acq_lowres_mc_kernel<CMAX, EXACT, P, L, decltype(s)::value>), grid, block, L ? pl.lds_bytes : 0, st, q);
        });
    };
    using R4 = std::integral_constant<int, 4>;
    using R8 = std::integral_constant<int, 8>;
    if (!pl.lds) {
        if (pl.ppt != 4) return fail(PP_ERR_BAD_ARG, "MC-dropout low-resolution scorer: plan without LDS patch and %d rows per wave", pl.ppt);
        go(R4{}, std::false_type{});
    } else if (pl.ppt == 8) {
        if constexpr (EXACT) go(R8{}, std::true_type{});
        else return fail(PP_ERR_BAD_ARG, "MC-dropout low-resolution scorer: 8 rows per wave planned for C=%d", q.g.C);
    } else {
        go(R4{}, std::true_type{});
    }
    return check_launch("acq_lowres_mc_kernel");
}

static int dispatch_lowres_mc(const LowresMcParams& q, const LowresPlan& pl, int64_t B, hipStream_t st)
{
    return lowres_by_classes(q.g.C, [&](auto cmax, auto exact) { return launch_lowres_mc<decltype(cmax)::value, decltype(exact)::value>(q, pl, B, st); });
}

// ---- MC-dropout hard vote: host side ---------------------------------------------------------------------
constexpr int64_t kVoteMaxPasses = 255;      // the vote counts are bytes

static int validate_vote_passes(int64_t T)
{
    if (T < 1 || T > kVoteMaxPasses)
        return fail(PP_ERR_UNSUPPORTED, "hard vote: T=%lld passes outside [1, %lld] (the vote counts are bytes)", (long long)T,
                    (long long)kVoteMaxPasses);
    return PP_OK;
}

// tab[n] = llrint(-(n/T) ln(n/T) 2^24) in double, tab[0] = 0 (and 0 beyond T)
static void fill_vote_table(int64_t T, VoteTable& tab)
{
    for (int n = 0; n < 256; ++n) tab.v[n] = 0u;
    for (int64_t n = 1; n <= T; ++n) {
        const double p = (double)n / (double)T;
        tab.v[n] = (uint32_t)llrint(-p * log(p) * 16777216.0);
    }
}

// make_lowres_mc_plan's tiles: 8 rows per wave for the dataset class counts with the patch in LDS (48 counter words at C = 21), 4
// rows for the generic instantiations (64 counter words at CMAX = 64) and the form that reads from memory
template <int CMAX, bool EXACT>
static int launch_lowres_mc_vote(const LowresVoteParams& q, const LowresPlan& pl, int64_t B, hipStream_t st)
{
    EventScope ev(st);
    dim3 grid((unsigned)(B * pl.tiles_x * pl.tiles_y)), block(kBlock);
#define PP_VOTE(P, L) hipLaunchKernelGGL((acq_lowres_mc_vote_kernel<CMAX, EXACT, P, L>), grid, block, (L) ? pl.lds_bytes : 0, st, q)
    if (!pl.lds) {
        if (pl.ppt != 4) return fail(PP_ERR_BAD_ARG, "hard-vote low-resolution scorer: plan without LDS patch and %d rows per wave", pl.ppt);
        PP_VOTE(4, false);
    } else if (pl.ppt == 8) {
        if constexpr (EXACT) PP_VOTE(8, true);
        else return fail(PP_ERR_BAD_ARG, "hard-vote low-resolution scorer: 8 rows per wave planned for C=%d", q.g.C);
    } else {
        PP_VOTE(4, true);
    }
#undef PP_VOTE
    return check_launch("acq_lowres_mc_vote_kernel");
}

static int dispatch_lowres_mc_vote(const LowresVoteParams& q, const LowresPlan& pl, int64_t B, hipStream_t st)
{
    return lowres_by_classes(q.g.C, [&](auto cmax, auto exact) { return launch_lowres_mc_vote<decltype(cmax)::value, decltype(exact)::value>(q, pl, B, st); });
}

// ---- MC-dropout mean-probability scores and BALD: host side ------------------------------------------------------------
// The strategy of the two mean-probability entries: 0..2 and PP_ACQ_BALD, no PP_ACQ_REFERENCE_ORDER (there is one operation order)
static int validate_mean_strategy(int strategy)
{
    if (strategy & PP_ACQ_REFERENCE_ORDER)
        return fail(PP_ERR_BAD_ARG, "mean-probability scorer: PP_ACQ_REFERENCE_ORDER has no meaning here (strategy 0x%x)", strategy);
    if (strategy < 0 || strategy > PP_ACQ_BALD) return fail(PP_ERR_BAD_ARG, "unknown strategy %d", strategy);
    return PP_OK;
}

// The 4-row tile in every form (acq_lowres_mc_mean_kernel); heads wider than 32 classes read their taps from memory
static LowresPlan make_lowres_mc_mean_plan(int64_t B, int64_t C, int64_t h, int64_t w, int64_t Hc, int64_t Wc, float sh, float sw)
{
    LowresPlan pl = make_lowres_plan(B, C, h, w, Hc, Wc, sh, sw, true);
    if (C > 32) {
        pl.lds = false;
        pl.patch_cap = 0;
        pl.lds_bytes = 0;
    }
    return pl;
}

template <int CMAX, bool EXACT>
static int launch_lowres_mc_mean(const LowresMcParams& q, const LowresPlan& pl, int64_t B, hipStream_t st)
{
    EventScope ev(st);
    if (pl.ppt != 4) return fail(PP_ERR_BAD_ARG, "mean-probability low-resolution scorer: plan with %d rows per wave", pl.ppt);
    dim3 grid((unsigned)(B * pl.tiles_x * pl.tiles_y)), block(kBlock);
    const bool bald = q.g.strategy == PP_ACQ_BALD;
#define PP_MEAN(L, D) hipLaunchKernelGGL((acq_lowres_mc_mean_kernel<CMAX, EXACT, L, D>), grid, block, (L) ? pl.lds_bytes : 0, st, q)
    if constexpr (CMAX <= 32) {
        if (pl.lds) {
            if (bald) PP_MEAN(true, true);
            else PP_MEAN(true, false);
            return check_launch("acq_lowres_mc_mean_kernel");
        }
    }
    if (pl.lds) return fail(PP_ERR_BAD_ARG, "mean-probability low-resolution scorer: LDS patch planned for C=%d", q.g.C);
    if (bald) PP_MEAN(false, true);
    else PP_MEAN(false, false);
#undef PP_MEAN
    return check_launch("acq_lowres_mc_mean_kernel");
}

static int dispatch_lowres_mc_mean(const LowresMcParams& q, const LowresPlan& pl, int64_t B, hipStream_t st)
{
    return lowres_by_classes(q.g.C, [&](auto cmax, auto exact) { return launch_lowres_mc_mean<decltype(cmax)::value, decltype(exact)::value>(q, pl, B, st); });
}

}  // namespace pp

using namespace pp;

extern "C" {

int pp_acq_lowres_mc_score_topk(const float* low, int64_t ldx, int64_t B, int64_t T, int64_t C, int64_t h, int64_t w, int64_t H,
                                int64_t W, int align_corners, int64_t Hc, int64_t Wc, const uint8_t* exclude, int strategy,
                                float scale, int64_t k, int32_t* out_idx, float* out_val, float* out_map, void* workspace,
                                size_t ws_bytes, pp_stream_t stream)
{
    if (int rc = validate_lowres_mc(low, ldx, B, T, C, h, w, H, W, Hc, Wc, strategy)) return rc;
    hipStream_t st = as_stream(stream);
    LowresMcParams q{make_lowres_params(low, ldx, exclude, out_map, C, h, w, H, W, align_corners, Hc, Wc, strategy), (int)T, scale};
    const LowresPlan pl = make_lowres_mc_plan(B, C, h, w, Hc, Wc, q.g.sh, q.g.sw);
    // the mean of T scores lies in the score's own range: the quantised-histogram select applies unchanged
    const float qs = score_qscale(strategy, C);
    const bool hist_ok = g_knobs.hist_fuse && large_q_ok(B, k, qs);
    return run_lowres_select(q.g, pl, B, k, out_idx, out_val, workspace, ws_bytes, st, qs, hist_ok, [&] { return dispatch_lowres_mc(q, pl, B, st); });
}

int pp_acq_lowres_mc_score_at(const float* low, int64_t ldx, int64_t B, int64_t T, int64_t C, int64_t h, int64_t w, int64_t H,
                              int64_t W, int align_corners, int64_t Hc, int64_t Wc, int strategy, float scale,
                              const int32_t* img_idx, const int32_t* pix_idx, int64_t n, float* out, pp_stream_t stream)
{
    if (int rc = validate_lowres_mc(low, ldx, B, T, C, h, w, H, W, Hc, Wc, strategy)) return rc;
    LowresAt at;
    if (int rc = lowres_at_begin("score_at", h, w, H, W, align_corners, img_idx, pix_idx, out, n, at)) return rc;
    if (!at.any) return PP_OK;
    hipStream_t st = as_stream(stream);
    lowres_by_classes(C, [&](auto cmax, auto exact) {
        hipLaunchKernelGGL((acq_lowres_mc_at_kernel<decltype(cmax)::value, decltype(exact)::value>), at.grid, dim3(kBlock), 0, st, low, ldx, (int)T,
                           (int)h, (int)w, at.sh, at.sw, at.align, (int)Wc, (int)C, strategy, scale, img_idx, pix_idx, n, out);
        return 0;
    });
    return check_launch("acq_lowres_mc_at_kernel");
}

int pp_acq_vote_accumulate(const float* logits, int64_t T, int64_t C, int64_t H, int64_t W, int64_t sT, int64_t sC, int64_t sH,
                           int64_t sW, uint8_t* votes, int accumulate, pp_stream_t stream)
{
    if (!votes) return fail(PP_ERR_BAD_ARG, "vote_accumulate: votes is null");
    if (!logits) return fail(PP_ERR_BAD_ARG, "logits is null");
    if (int rc = validate_vote_passes(T)) return rc;
    if (int rc = validate(logits, T, C, H, W, 0)) return rc;
    const int64_t N = H * W;
    hipLaunchKernelGGL(vote_accumulate_kernel, dim3((unsigned)cdiv(N, kBlock)), dim3(kBlock), 0, as_stream(stream), logits, (int)T, (int)C,
                       (int)W, N, sT, sC, sH, sW, votes, accumulate);
    return check_launch("vote_accumulate_kernel");
}

int pp_acq_vote_score_map(const uint8_t* votes, int64_t B, int64_t T, int64_t C, int64_t H, int64_t W, const uint8_t* exclude,
                          int strategy, float* out_map, pp_stream_t stream)
{
    if (!votes) return fail(PP_ERR_BAD_ARG, "vote_score_map: votes is null");
    if (!out_map) return fail(PP_ERR_BAD_ARG, "out_map is null");
    if (int rc = validate_vote_passes(T)) return rc;
    if (int rc = validate(reinterpret_cast<const float*>(votes), B, C, H, W, strategy)) return rc;
    if (B > 65535) return fail(PP_ERR_UNSUPPORTED, "vote_score_map: B=%lld > 65535 images per call", (long long)B);
    VoteScoreParams p{votes, exclude, out_map, H * W, (int)C, (int)T, strategy, {}};
    fill_vote_table(T, p.tab);
    hipLaunchKernelGGL(vote_score_kernel, dim3((unsigned)cdiv(p.N, kBlock), (unsigned)B), dim3(kBlock), 0, as_stream(stream), p);
    return check_launch("vote_score_kernel");
}

int pp_acq_lowres_mc_vote_topk(const float* low, int64_t ldx, int64_t B, int64_t T, int64_t C, int64_t h, int64_t w, int64_t H,
                               int64_t W, int align_corners, int64_t Hc, int64_t Wc, const uint8_t* exclude, int strategy, int64_t k,
                               int32_t* out_idx, float* out_val, float* out_map, void* workspace, size_t ws_bytes, pp_stream_t stream)
{
    if (!low) return fail(PP_ERR_BAD_ARG, "logits is null");
    if (int rc = validate_vote_passes(T)) return rc;
    if (int rc = validate_lowres_mc(low, ldx, B, T, C, h, w, H, W, Hc, Wc, strategy)) return rc;
    hipStream_t st = as_stream(stream);
    LowresVoteParams q{make_lowres_params(low, ldx, exclude, out_map, C, h, w, H, W, align_corners, Hc, Wc, strategy), (int)T, {}};
    fill_vote_table(T, q.tab);
    const LowresPlan pl = make_lowres_mc_plan(B, C, h, w, Hc, Wc, q.g.sh, q.g.sw);
    // k > 48: the map, then pp_topk_select's selection on it (qscale 0) - without the scorers' fused histogram, whose bins clamp the
    // fills (-1.0 / 2.0 lie outside the score range) into the end bins
    return run_lowres_select(q.g, pl, B, k, out_idx, out_val, workspace, ws_bytes, st, 0.0f, false, [&] { return dispatch_lowres_mc_vote(q, pl, B, st); });
}

int pp_acq_mean_prob_score_map(const float* prob, int64_t B, int64_t C, int64_t H, int64_t W, int64_t sB, int64_t sC, int64_t sH,
                               int64_t sW, const float* mean_ent, const uint8_t* exclude, int strategy, float* out_map,
                               pp_stream_t stream)
{
    if (!prob) return fail(PP_ERR_BAD_ARG, "mean_prob_score_map: prob is null");
    if (!out_map) return fail(PP_ERR_BAD_ARG, "out_map is null");
    if (int rc = validate_mean_strategy(strategy)) return rc;
    if ((strategy == PP_ACQ_BALD) != (mean_ent != nullptr))
        return fail(PP_ERR_BAD_ARG, "mean_prob_score_map: mean_ent is required for PP_ACQ_BALD and must be null otherwise (strategy %d)", strategy);
    if (int rc = validate(prob, B, C, H, W, strategy == PP_ACQ_BALD ? PP_ACQ_ENTROPY : strategy)) return rc;
    if (B > 65535) return fail(PP_ERR_UNSUPPORTED, "mean_prob_score_map: B=%lld > 65535 images per call", (long long)B);
    MeanMapParams p{prob, mean_ent, exclude, out_map, H * W, sB, sC, sH, sW, (int)C, (int)W, strategy};
    hipLaunchKernelGGL(mean_prob_score_kernel, dim3((unsigned)cdiv(p.N, kBlock), (unsigned)B), dim3(kBlock), 0, as_stream(stream), p);
    return check_launch("mean_prob_score_kernel");
}

int pp_acq_lowres_mc_mean_topk(const float* low, int64_t ldx, int64_t B, int64_t T, int64_t C, int64_t h, int64_t w, int64_t H,
                               int64_t W, int align_corners, int64_t Hc, int64_t Wc, const uint8_t* exclude, int strategy,
                               float scale, int64_t k, int32_t* out_idx, float* out_val, float* out_map, void* workspace,
                               size_t ws_bytes, pp_stream_t stream)
{
    if (!low) return fail(PP_ERR_BAD_ARG, "logits is null");
    if (int rc = validate_mean_strategy(strategy)) return rc;
    if (int rc = validate_lowres_mc(low, ldx, B, T, C, h, w, H, W, Hc, Wc, strategy == PP_ACQ_BALD ? PP_ACQ_ENTROPY : strategy)) return rc;
    hipStream_t st = as_stream(stream);
    LowresMcParams q{make_lowres_params(low, ldx, exclude, out_map, C, h, w, H, W, align_corners, Hc, Wc, strategy), (int)T, scale};
    const LowresPlan pl = make_lowres_mc_mean_plan(B, C, h, w, Hc, Wc, q.g.sh, q.g.sw);
    // k > 48: the map, then pp_topk_select's selection on it (qscale 0), as the hard vote: the fills lie outside the score range
    return run_lowres_select(q.g, pl, B, k, out_idx, out_val, workspace, ws_bytes, st, 0.0f, false, [&] { return dispatch_lowres_mc_mean(q, pl, B, st); });
}

}  // extern "C"
