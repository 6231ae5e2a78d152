// acq.hip — fused acquisition for PixelPick on gfx950 (MI355X).
//
// Replaces, for a batch of images and in ONE read of the logits:
//   query.py:190      prob = F.softmax(model(x)["pred"][:, :, :h, :w], dim=1)
//   query.py:229-239  UncertaintySampler._entropy / _least_confidence / _margin_sampling
//   query.py:195-201  uc_map[mask] = fill ; uc_map[mask_void] = fill
//   query.py:57-61    uc_map.flatten().topk(k, largest).indices
//
// Bandwidth-bound integer/float streaming work: no MFMA.  Each lane keeps the C class logits of its
// pixels in registers (softmax needs no second memory pass), planes are read as 16 B/lane coalesced
// loads, per-wave top-k candidates are extracted with DPP reductions and merged by a tiny second
// kernel, so the logits are read exactly once and nothing full-size is written unless asked for.
//
// This source holds the FULL-SIZE scorers and the list select that rides on them, and nothing else (bench.py keys the scorer's traffic
// record to this file's hash).  The selection on a score map is acq_topk.hip, the scorers on the classifier-resolution logits are
// acq_lowres.hip, the MC-dropout families acq_mc.hip, the planners' switches acq_knobs.hip; acq_device.h and acq_host.h state what
// crosses between them.
#include <algorithm>
#include <cmath>

#include "acq_host.h"
#include "acq_score.h"

namespace pp {

typedef float f32x4_nt __attribute__((ext_vector_type(4)));
typedef float f32x2_nt __attribute__((ext_vector_type(2)));      // (native vector type: __builtin_nontemporal_load does not take HIP's float4 struct)

// ---- main kernel ---------------------------------------------------------------------------------
// VEC == 4: planes are flat & 16-B aligned (sW == 1, sH == W, N % 4 == 0): float4 per class plane.
// VEC == 1: arbitrary element strides (NHWC views, cropped views), one pixel per load.
// A block covers kBlock*VEC*G consecutive pixels of ONE image.
// MATH: 0 = default scorer, 1 = reference operation order, 2 = input already holds probabilities.
// HIST (map-writing launches of the large-k selection, VEC == 4): the block also counts its scores into the image's kQBins-bin histogram
// (LDS bins in the survivor lists' storage - no candidates are extracted in that mode - then one global atomic per non-empty bin): what
// select_qhist_kernel did in a second pass over the map.
template <int CMAX, bool EXACT, int VEC, int G, int MATH, int OCC = 3, int STRAT = -1, bool HIST = false, bool NT = true, bool EMIT = false>
__global__ __launch_bounds__(kBlock, OCC) void acq_kernel(AcqParams p)
{
    constexpr int PPT = VEC * G;
    static_assert(!HIST || VEC == 4, "histogram epilogue: the flat float4 form");
    static_assert(!EMIT || (VEC == 4 && !HIST), "candidate emission: the flat float4 form");
    __shared__ uint64_t s_surv[kBlock / kWave][kSurvCap];
    static_assert(sizeof(uint64_t) * (kBlock / kWave) * kSurvCap >= sizeof(uint32_t) * kQBins, "the bins live in the survivor lists");
    uint32_t* lh = reinterpret_cast<uint32_t*>(&s_surv[0][0]);
    if constexpr (HIST) {
        for (int i = threadIdx.x; i < kQBins; i += kBlock) lh[i] = 0u;
        __syncthreads();
    }
    __shared__ uint32_t s_cnt[kBlock / kWave];
    __shared__ uint64_t s_top[(kBlock / kWave) * kSmallKMax];
    int lb = blockIdx.x;
    if (p.xcd_per) {
        // Large class planes (>= 4 MB: 1024 x 2048 logits): a block's C streams lie a whole plane apart, and with blocks dealt
        // round-robin to the eight XCDs every XCD walks every plane end to end.  Giving each XCD one contiguous eighth of the
        // launch lifts a pure read of this layout from 0.65 to 0.74 of 8 TB/s (tools/probe/plane_read.hip, profiles/r04_acq_layout.txt).
        lb = (int)(blockIdx.x & 7u) * p.xcd_per + (int)(blockIdx.x >> 3);
        if (lb >= p.nb) return;
    }
    const int img = lb / p.blocks_per_image;
    const int blk = lb - img * p.blocks_per_image;
    const int tid = threadIdx.x;
    const bool largest = p.strategy != PP_ACQ_MARGIN;
    const float fill = largest ? 0.0f : 1.0f;
    const float* base = p.logits + (int64_t)img * p.sB;
    const uint8_t* excl = p.exclude ? p.exclude + (int64_t)img * p.N : nullptr;
    float* omap = p.out_map ? p.out_map + (int64_t)img * p.N : nullptr;

    uint32_t kh[PPT], kl[PPT];

#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int64_t pix0 = ((int64_t)blk * G + g) * (kBlock * VEC) + (int64_t)tid * VEC;
        float s[VEC];
        if (pix0 < p.N) {
            if constexpr (VEC == 4) {
                float x[4][CMAX];
#pragma unroll
                for (int c = 0; c < CMAX; ++c)
                    if (EXACT || c < p.C) {
                        if constexpr (NT) {
                            // the logits are read exactly once: non-temporal loads (no L2 / MALL allocation for a 2.6 GB stream that
                            // nobody reads again) - measured 0.420-0.425 -> 0.392-0.396 ms per launch at B=256 x 256x512x19, i.e. 0.76 ->
                            // 0.82 of 8 TB/s; pp_debug_set_acq_tuning bit 11 selects the ordinary loads for A/B
                            const f32x4_nt v = __builtin_nontemporal_load(reinterpret_cast<const f32x4_nt*>(base + (int64_t)c * p.sC + pix0));
                            x[0][c] = v.x; x[1][c] = v.y; x[2][c] = v.z; x[3][c] = v.w;
                        } else {
                        const float4 v = *reinterpret_cast<const float4*>(base + (int64_t)c * p.sC + pix0);
                        x[0][c] = v.x; x[1][c] = v.y; x[2][c] = v.z; x[3][c] = v.w;
                        }
                    }
                uint32_t ex = excl ? *reinterpret_cast<const uint32_t*>(excl + pix0) : 0u;
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    if constexpr (MATH == 0) s[v] = pixel_score_fast<CMAX, EXACT, STRAT>(x[v], p.C, p.strategy);
                    else s[v] = pixel_score<CMAX, EXACT>(x[v], p.C, p.strategy, MATH == 2);
                    if ((ex >> (8 * v)) & 0xFFu) s[v] = fill;
                    if constexpr (HIST) atomicAdd(&lh[qbin(s[v], largest, p.qscale)], 1u);
                    __builtin_amdgcn_sched_barrier(0);  // one pixel's temporaries at a time (VGPR budget)
                }
                if (omap) *reinterpret_cast<float4*>(omap + pix0) = make_float4(s[0], s[1], s[2], s[3]);
            } else {
                const int64_t h = pix0 / p.W, w = pix0 - h * p.W;
                const float* px = base + h * p.sH + w * p.sW;
                float x[CMAX];
#pragma unroll
                for (int c = 0; c < CMAX; ++c)
                    if (EXACT || c < p.C) x[c] = NT ? __builtin_nontemporal_load(px + (int64_t)c * p.sC) : px[(int64_t)c * p.sC];
                if constexpr (MATH == 0) s[0] = pixel_score_fast<CMAX, EXACT>(x, p.C, p.strategy);
                else s[0] = pixel_score<CMAX, EXACT>(x, p.C, p.strategy, MATH == 2);
                if (excl && excl[pix0]) s[0] = fill;
                if (omap) omap[pix0] = s[0];
            }
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                kh[g * VEC + v] = order_key(s[v], largest);
                kl[g * VEC + v] = 0xFFFFFFFFu - (uint32_t)(pix0 + v);
            }
        } else {
#pragma unroll
            for (int v = 0; v < VEC; ++v) { kh[g * VEC + v] = 0u; kl[g * VEC + v] = 0u; }
        }
        // keep one group's class vector live at a time (occupancy hides the HBM latency, not hoisted loads)
        __builtin_amdgcn_sched_barrier(0);
    }

    if constexpr (EMIT) {
        // keys at or beyond the image's threshold key form an upper set of the (key, index) order: if the image's lists hold >= k words
        // the k picks are among them (topk_lsel_kernel checks that).  Ballot order inside the segment; the select ranks exactly.
        const uint32_t tk = p.tkey[img];
        const int wave = tid >> 6, lane = tid & (kWave - 1);
        const int seg = blk * (kBlock / kWave) + wave;
        uint64_t* dst = p.elist + (int64_t)img * p.eimg + (int64_t)seg * p.segst;
        const uint64_t below = (1ull << lane) - 1ull;
        uint32_t n = 0;
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            const bool sv = kh[j] >= tk;                 // (pixels past the end of the image carry key 0, tk >= 1)
            const uint64_t bal = __ballot(sv);
            if (sv) dst[n + (uint32_t)__popcll(bal & below)] = ((uint64_t)kh[j] << 32) | kl[j];
            n += (uint32_t)__popcll(bal);
        }
        if (lane == 0) p.ecnt[(int64_t)img * p.nseg + seg] = n;
        return;
    }
    if constexpr (HIST) {
        __syncthreads();
        uint32_t* Hg = p.qhist + (int64_t)img * kQBins;
        for (int d = threadIdx.x; d < kQBins; d += kBlock) {
            const uint32_t c = lh[d];
            if (c) atomicAdd(&Hg[d], c);
        }
        return;
    }
    if (p.cand)
        block_emit_topk<PPT>(kh, kl, p.k, p.cand + ((int64_t)img * p.blocks_per_image + blk) * p.k, p.reduce_mode, s_surv, s_cnt, s_top);
}

// ---- dense NHWC (channels-last) input ----------------------------------------------------------------
// Pixel-major storage: one pixel's C logits are contiguous (76 B at C=19).  A per-lane strided read touches 38
// cache lines per wave-instruction; instead the block streams its pixel range as flat coalesced float4 loads
// into LDS and every lane then reads its own pixel's class vector back (stride C floats: conflict-free for odd C).
// Measured (B=256 x 256x512x19, entropy, k=20): 4.02 TB/s vs 3.17 TB/s for the per-lane strided path and
// 5.98 TB/s for NCHW planes; issuing the next group's loads into registers ahead of the compute was slower (2.6).
template <int CMAX, bool EXACT, int G, int MATH>
__global__ __launch_bounds__(kBlock, 3) void acq_nhwc_kernel(AcqParams p)
{
    __shared__ __attribute__((aligned(16))) float s_x[kBlock * CMAX];
    __shared__ uint64_t s_surv[kBlock / kWave][kSurvCap];
    __shared__ uint32_t s_cnt[kBlock / kWave];
    __shared__ uint64_t s_top[(kBlock / kWave) * kSmallKMax];
    const int img = blockIdx.x / p.blocks_per_image;
    const int blk = blockIdx.x - img * p.blocks_per_image;
    const int tid = threadIdx.x;
    const bool largest = p.strategy != PP_ACQ_MARGIN;
    const float fill = largest ? 0.0f : 1.0f;
    const int C = EXACT ? CMAX : p.C;
    const float* base = p.logits + (int64_t)img * p.sB;
    const uint8_t* excl = p.exclude ? p.exclude + (int64_t)img * p.N : nullptr;
    float* omap = p.out_map ? p.out_map + (int64_t)img * p.N : nullptr;
    uint32_t kh[G], kl[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int64_t pix_blk = ((int64_t)blk * G + g) * kBlock;          // first pixel of this group
        const int64_t npix = p.N - pix_blk < kBlock ? p.N - pix_blk : kBlock;
        if (npix > 0) {
            const int64_t nfl = npix * C;                                 // floats to stage (multiple of 4: N % 4 == 0)
            const float4* src = reinterpret_cast<const float4*>(base + pix_blk * C);
            for (int64_t i = tid; i < nfl / 4; i += kBlock)         // (read once: non-temporal, as acq_kernel)
                reinterpret_cast<f32x4_nt*>(s_x)[i] = __builtin_nontemporal_load(reinterpret_cast<const f32x4_nt*>(src) + i);
        }
        __syncthreads();
        const int64_t pix = pix_blk + tid;
        if (pix < p.N) {
            float x[CMAX];
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                if (EXACT || c < C) x[c] = s_x[tid * C + c];
            float sc;
            if constexpr (MATH == 0) sc = pixel_score_fast<CMAX, EXACT>(x, p.C, p.strategy);
            else sc = pixel_score<CMAX, EXACT>(x, p.C, p.strategy, MATH == 2);
            if (excl && excl[pix]) sc = fill;
            if (omap) omap[pix] = sc;
            kh[g] = order_key(sc, largest);
            kl[g] = 0xFFFFFFFFu - (uint32_t)pix;
        } else {
            kh[g] = 0u; kl[g] = 0u;
        }
        __syncthreads();
    }
    if (p.cand)
        block_emit_topk<G>(kh, kl, p.k, p.cand + ((int64_t)img * p.blocks_per_image + blk) * p.k, p.reduce_mode, s_surv, s_cnt, s_top);
}

// ---- dense NHWC, asynchronous variant ------------------------------------------------------------------
// Same pixel -> wave mapping and the same results as acq_nhwc_kernel, but every WAVE streams its own 64-pixel slices
// into a private, double-buffered LDS slot with LDS-DMA (global_load_lds_dwordx4: 1 KiB per wave instruction, no
// staging registers, no ds_write pass) and keeps the NEXT slice in flight while it scores the current one: the only
// synchronisation is the issuing wave's counted `s_waitcnt vmcnt(N)` (MI355X_MICROARCH.md item 7) - no barrier at all.
// The DMA pieces are written in inline asm so that hipcc's own s_waitcnt bookkeeping (which would drain vmcnt(0) in
// front of the first LDS read) does not see them.
__device__ __forceinline__ void glds16(const float* gsrc, uint32_t lds_dst)
{
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
__device__ __forceinline__ void glds1(const uint8_t* gsrc, uint32_t lds_dst)
{
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_ubyte %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory"); }

template <int CMAX, int G>
__global__ __launch_bounds__(kBlock, (CMAX > 19 ? 2 : 3)) void acq_nhwc_dma_kernel(AcqParams p)
{
    constexpr int NW = kBlock / kWave;
    constexpr int NCH = (CMAX * 256 + 1023) / 1024;      // 1-KiB DMA pieces per 64-pixel slice (5 at C = 19)
    constexpr int SLOT = NCH * 256;                      // floats per slot (the last piece may overhang the slice)
    __shared__ __attribute__((aligned(1024))) float s_x[NW][2][SLOT];
    __shared__ __attribute__((aligned(256))) uint32_t s_e[NW][2][kWave];   // sub-dword LDS-DMA lands one DWORD per lane
    __shared__ uint64_t s_surv[NW][kSurvCap];
    __shared__ uint32_t s_cnt[NW];
    __shared__ uint64_t s_top[NW * kSmallKMax];
    const int img = blockIdx.x / p.blocks_per_image;
    const int blk = blockIdx.x - img * p.blocks_per_image;
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool largest = p.strategy != PP_ACQ_MARGIN;
    const float fill = largest ? 0.0f : 1.0f;
    const float* base = p.logits + (int64_t)img * p.sB;
    const uint8_t* excl = p.exclude ? p.exclude + (int64_t)img * p.N : nullptr;
    float* omap = p.out_map ? p.out_map + (int64_t)img * p.N : nullptr;
    const uint32_t lds_x = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)&s_x[wave][0][0]);
    const uint32_t lds_e = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)&s_e[wave][0][0]);

    auto issue = [&](int g, int buf) {
        const int64_t pix0 = ((int64_t)blk * G + g) * kBlock + wave * kWave;          // first pixel of this wave's slice
        const int64_t left = p.N - pix0;
        const int nflt = (int)(left <= 0 ? 0 : (left < kWave ? left : kWave)) * CMAX;  // valid floats of the slice
        const float* src0 = base + (left > 0 ? pix0 : 0) * CMAX;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the slot's previous contents have been read
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const int f = (j * kWave + lane) * 4;
            glds16(src0 + (f < nflt ? f : 0), lds_x + (uint32_t)(buf * SLOT * 4 + j * 1024));   // every lane active: fixed op count
        }
        if (excl) glds1(excl + (lane < left ? pix0 + lane : 0), lds_e + (uint32_t)(buf * kWave * 4));
    };

    uint32_t kh[G], kl[G];
    issue(0, 0);
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (g + 1 < G) {
            issue(g + 1, (g + 1) & 1);
            if (excl) wait_vmcnt<NCH + 1>(); else wait_vmcnt<NCH>();     // slice g has landed, slice g+1 stays in flight
        } else {
            wait_vmcnt<0>();
        }
        const int64_t pix = ((int64_t)blk * G + g) * kBlock + tid;
        if (pix < p.N) {
            const float* sx = &s_x[wave][g & 1][lane * CMAX];
            float x[CMAX];
#pragma unroll
            for (int c = 0; c < CMAX; ++c) x[c] = sx[c];
            float sc = pixel_score_fast<CMAX, true>(x, p.C, p.strategy);
            if (excl && (s_e[wave][g & 1][lane] & 0xFFu)) sc = fill;
            if (omap) omap[pix] = sc;
            kh[g] = order_key(sc, largest);
            kl[g] = 0xFFFFFFFFu - (uint32_t)pix;
        } else {
            kh[g] = 0u; kl[g] = 0u;
        }
    }
    if (p.cand)
        block_emit_topk<G>(kh, kl, p.k, p.cand + ((int64_t)img * p.blocks_per_image + blk) * p.k, p.reduce_mode, s_surv, s_cnt, s_top);
}

// acq_kernel's block geometry (a block covers kBlock * VEC * G consecutive pixels of one image), class vector streamed
template <int VEC, int G, int MATH>
__global__ __launch_bounds__(kBlock) void acq_stream_kernel(AcqParams p)
{
    constexpr int PPT = VEC * G;
    __shared__ uint64_t s_surv[kBlock / kWave][kSurvCap];
    __shared__ uint32_t s_cnt[kBlock / kWave];
    __shared__ uint64_t s_top[(kBlock / kWave) * kSmallKMax];
    const int img = blockIdx.x / p.blocks_per_image;
    const int blk = blockIdx.x - img * p.blocks_per_image;
    const int tid = threadIdx.x;
    const bool largest = p.strategy != PP_ACQ_MARGIN;
    const float fill = largest ? 0.0f : 1.0f;
    const float* base = p.logits + (int64_t)img * p.sB;
    const uint8_t* excl = p.exclude ? p.exclude + (int64_t)img * p.N : nullptr;
    float* omap = p.out_map ? p.out_map + (int64_t)img * p.N : nullptr;
    uint32_t kh[PPT], kl[PPT];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int64_t pix0 = ((int64_t)blk * G + g) * (kBlock * VEC) + (int64_t)tid * VEC;
        if (pix0 < p.N) {
            float s[VEC];
            if constexpr (VEC == 4) {
                const float* px = base + pix0;
                const int64_t sC = p.sC;
                score_stream<4, MATH>([&](int c, float (&v)[4]) {
                    const float4 q = *reinterpret_cast<const float4*>(px + (int64_t)c * sC);
                    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
                }, p.C, p.strategy, s);
                const uint32_t ex = excl ? *reinterpret_cast<const uint32_t*>(excl + pix0) : 0u;
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    if ((ex >> (8 * v)) & 0xFFu) s[v] = fill;
                if (omap) *reinterpret_cast<float4*>(omap + pix0) = make_float4(s[0], s[1], s[2], s[3]);
            } else {
                const int64_t h = pix0 / p.W, w = pix0 - h * p.W;
                const float* px = base + h * p.sH + w * p.sW;
                const int64_t sC = p.sC;
                score_stream<1, MATH>([&](int c, float (&v)[1]) { v[0] = px[(int64_t)c * sC]; }, p.C, p.strategy, s);
                if (excl && excl[pix0]) s[0] = fill;
                if (omap) omap[pix0] = s[0];
            }
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                kh[g * VEC + v] = order_key(s[v], largest);
                kl[g * VEC + v] = 0xFFFFFFFFu - (uint32_t)(pix0 + v);
            }
        } else {
#pragma unroll
            for (int v = 0; v < VEC; ++v) { kh[g * VEC + v] = 0u; kl[g * VEC + v] = 0u; }
        }
    }
    if (p.cand)
        block_emit_topk<PPT>(kh, kl, p.k, p.cand + ((int64_t)img * p.blocks_per_image + blk) * p.k, p.reduce_mode, s_surv, s_cnt, s_top);
}

// ---- large-k WITHOUT the score map: sampled threshold -> candidate emission in the scorer -> list select ---------------------------------
// The map-writing scorer pays 16 % for a 5 % larger stream (mixed read / write traffic).  Instead: (1) acq_sample_thr_kernel scores a sample of
// the image - sample_locs jittered locations of 4 * sample_gpl consecutive pixels (spatially correlated maps give about one independent draw
// per location) - and takes the edge of the quantised bin at which the sample's count from the top reaches mult * k / N of the sample as the
// image's threshold key (a conservative guess: about mult * k pixels pass); (2) the scorer (acq_kernel<..., EMIT>) writes only the pixels at or
// beyond that key, as (key, index) words into per-wave segments (~1 B / pixel instead of 4); (3) topk_lsel_kernel histograms the image's lists
// into kLBins bins spanning only [threshold, end of the score range] (the lists hold nothing else: bins ~30x finer than topk_qsel_kernel's for
// the same LDS), finds the bin of the k-th element, drops that bin and the ones above into LDS and ranks every candidate inside its bin.  The
// RESULT never depends on the sample: an image whose lists hold fewer than k words (the sample misled), or whose candidates do not fit (ties),
// is redone exactly by its own block (score map + one-block radix select, see topk_lsel_kernel).
constexpr int kSampleThreads = 512;
constexpr int kLBins = 4096;

template <int CMAX>
__global__ __launch_bounds__(kSampleThreads) void acq_sample_thr_kernel(AcqParams p, float qscale, uint32_t want, uint32_t* tkey_out)
{
    __shared__ uint32_t lh[kQBins];
    __shared__ uint32_t wsum[kSampleThreads / kWave];
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const bool largest = p.strategy != PP_ACQ_MARGIN;
    const float fill = largest ? 0.0f : 1.0f;
    const float* base = p.logits + (int64_t)img * p.sB;
    const uint8_t* excl = p.exclude ? p.exclude + (int64_t)img * p.N : nullptr;
    for (int i = tid; i < kQBins; i += kSampleThreads) lh[i] = 0u;
    __syncthreads();
    const int gpl = p.sample_gpl, groups = p.sample_locs * gpl;
    const int64_t stride = p.N / p.sample_locs;                    // >= 4 * gpl pixels (host)
    const uint32_t slots = (uint32_t)(stride / (4 * gpl));
#pragma unroll 1
    for (int g = tid; g < groups; g += kSampleThreads) {
        const uint32_t loc = (uint32_t)(g / gpl);
        const uint32_t h = (loc * 2654435761u + (uint32_t)img * 40503u + 0x9E3779B9u) >> 7;
        const int64_t pix0 = ((int64_t)loc * stride + (int64_t)(h % slots) * (4 * gpl) + (g - (int)loc * gpl) * 4) & ~3ll;
        float x[4][CMAX];
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
            const float4 v = *reinterpret_cast<const float4*>(base + (int64_t)c * p.sC + pix0);
            x[0][c] = v.x; x[1][c] = v.y; x[2][c] = v.z; x[3][c] = v.w;
        }
        const uint32_t ex = excl ? *reinterpret_cast<const uint32_t*>(excl + pix0) : 0u;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            float sc = pixel_score_fast<CMAX, true>(x[v], p.C, p.strategy);
            if ((ex >> (8 * v)) & 0xFFu) sc = fill;
            atomicAdd(&lh[qbin(sc, largest, qscale)], 1u);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    __syncthreads();
    // thread t owns OWN bins from the top: kQBins - 1 - OWN t - u; inclusive scan over the threads
    constexpr int OWN = kQBins / kSampleThreads;
    uint32_t own[OWN], tot = 0;
#pragma unroll
    for (int u = 0; u < OWN; ++u) { own[u] = lh[kQBins - 1 - (OWN * tid + u)]; tot += own[u]; }
    uint32_t incl = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)incl, o, 64);
        if (lane >= o) incl += v;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t cum = incl - tot;
    for (int w = 0; w < wave; ++w) cum += wsum[w];
#pragma unroll
    for (int u = 0; u < OWN; ++u) {
        const uint32_t before = cum;
        cum += own[u];
        if (before < want && want <= cum) {
            const int qb = kQBins - 1 - (OWN * tid + u);                // qbin value: every score with qbin >= qb should pass
            const int qi = largest ? qb : kQBins - 1 - qb;             // linear bin of the score
            const float edge = largest ? (float)qi / qscale : (float)(qi + 1) / qscale;      // the bin's far edge
            uint32_t tk = order_key(edge, largest);
            if (qb == 0 || tk < 1u) tk = 1u;                            // the last bin: everything passes
            tkey_out[img] = tk;
        }
    }
}

// bins of the list select: linear in the distance from the image's threshold towards the selected end of the score range
__device__ __forceinline__ uint32_t lbin(uint32_t key, bool lg, float tv, float lscale)
{
    const float s = key_to_float(key, lg);
    if (s != s) return lg ? (uint32_t)(kLBins - 1) : 0u;
    const float t = (lg ? s - tv : tv - s) * lscale;
    return (uint32_t)(t >= (float)(kLBins - 1) ? kLBins - 1 : (t > 0.0f ? (int)t : 0));
}

// One 1024-thread block per image; cnt / list: the scorer's per-wave segments (nseg segments, segsz entries apart).  range: the scorers'
// value range (ln C or 1).  An image whose lists do not do (fewer than k words: the sample misled; candidates that do not fit: ties) is
// redone exactly by its own block, right here: the score map of the image - the default scorer's arithmetic, written over the image's own,
// by then consumed, list segments - and the one-block radix select on it.  Slow (one block scores 10 MB of logits) and rare; nothing is
// launched for it, so the usual case pays nothing (two idle launches - a map kernel over a flagged list and topk_large_kernel - cost 9 us).
// Test build only (pp_debug_set_lsel_probe): one word per image saying how the image was finished - 0 from the lists, 1 redone and finished by
// the quantised select on the rewritten map, 2 redone and finished by the radix select.  The product's kernel has no such parameter.
#ifdef PP_DEBUG_KNOBS
#define PP_LSEL_PROBE_PARAM , uint32_t* probe
#define PP_LSEL_PROBE_ARG , g_knobs.lsel_probe
#define PP_LSEL_PROBE(how) do { if (probe && threadIdx.x == 0) probe[blockIdx.x] = (how); } while (0)
#else
#define PP_LSEL_PROBE_PARAM
#define PP_LSEL_PROBE_ARG
#define PP_LSEL_PROBE(how) do { } while (0)
#endif
template <int CMAX>
__global__ __launch_bounds__(kLargeThreads) void topk_lsel_kernel(AcqParams p, const uint64_t* list, const uint32_t* cnt, const uint32_t* tkey,
                                                                 int64_t eimg, int nseg, int segsz, int k, int largest, float range,
                                                                 int32_t* out_idx, float* out_val PP_LSEL_PROBE_PARAM)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint64_t* buf = reinterpret_cast<uint64_t*>(smem);                                   // kQCap candidates, grouped by bin
    uint32_t* start = reinterpret_cast<uint32_t*>(smem + (size_t)kQCap * 8);             // [kLBins] first slot of a bin's segment
    uint32_t* hist = start + kLBins;                                                     // [kLBins] bin counts, then the drop cursors
    uint32_t* misc = hist + kLBins;                                                      // 32 words
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool lg = largest != 0;
    const uint64_t* L = list + (int64_t)blockIdx.x * eimg;
    const uint32_t* C = cnt + (int64_t)blockIdx.x * nseg;
    const uint32_t tk = tkey[blockIdx.x];
    float tv = key_to_float(tk, lg);
    if (tk == 1u) tv = lg ? 0.0f : range;                              // "everything passes"
    if (tv != tv) tv = lg ? range : 0.0f;
    if (lg && tv < 0.0f) tv = 0.0f;
    const float span = lg ? range - tv : tv;
    const float lscale = (float)kLBins / (span > 1e-12f ? span : 1e-12f);
    constexpr int OWN = kLBins / kLargeThreads;
#pragma unroll
    for (int u = 0; u < OWN; ++u) hist[tid + u * kLargeThreads] = 0u;
    if (tid < 4) misc[tid] = 0u;
    __syncthreads();
    // A wave takes kSegW consecutive segments of every 16 * kSegW: their counts in one load, then one load per segment in flight (a segment
    // usually holds fewer than 64 words; the rest of a fuller one is walked afterwards).  With <= 16 * kSegW segments per image (256 x 512 at
    // 8 pixels per thread: exactly) the words stay in registers between the histogram pass and the drop pass: the lists are read once
    // (PMC: 61.9 -> ~35 MB fetched per launch).
    constexpr int kSegW = 16;
    const bool one_chunk = nseg <= (kLargeThreads / 64) * kSegW;
    uint32_t c[kSegW];
    uint64_t v[kSegW];
    auto load_chunk = [&](int c0) {
        const int s0 = c0 + wave * kSegW;
        const uint32_t mine = (lane < kSegW && s0 + lane < nseg) ? C[s0 + lane] : 0u;
#pragma unroll
        for (int u = 0; u < kSegW; ++u) c[u] = (uint32_t)__shfl((int)mine, u, 64);
#pragma unroll
        for (int u = 0; u < kSegW; ++u) v[u] = (uint32_t)lane < c[u] ? L[(int64_t)(s0 + u) * segsz + lane] : 0ull;
    };
    auto walk_chunk = [&](int c0, auto&& fn) {
        const int s0 = c0 + wave * kSegW;
#pragma unroll
        for (int u = 0; u < kSegW; ++u)
            if ((uint32_t)lane < c[u]) fn(v[u]);
#pragma unroll
        for (int u = 0; u < kSegW; ++u)
            for (uint32_t e = (uint32_t)lane + 64u; e < c[u]; e += 64u) fn(L[(int64_t)(s0 + u) * segsz + e]);
    };
    auto sweep = [&](bool reload, auto&& fn) {
        for (int c0 = 0; c0 < nseg; c0 += (kLargeThreads / 64) * kSegW) {
            if (reload) load_chunk(c0);
            walk_chunk(c0, fn);
        }
    };
    sweep(true, [&](uint64_t w) { atomicAdd(&hist[lbin((uint32_t)(w >> 32), lg, tv, lscale)], 1u); });
    __syncthreads();
    {
        // thread t owns bins kLBins - 1 - OWN t - u (from the top)
        uint32_t own[OWN], tot = 0;
#pragma unroll
        for (int u = 0; u < OWN; ++u) { own[u] = hist[kLBins - 1 - (OWN * tid + u)]; tot += own[u]; }
        uint32_t incl = tot;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t v = (uint32_t)__shfl_up((int)incl, o, 64);
            if (lane >= o) incl += v;
        }
        if (lane == 63) misc[8 + wave] = incl;
        __syncthreads();
        uint32_t cum = incl - tot;
        for (int w = 0; w < wave; ++w) cum += misc[8 + w];
#pragma unroll
        for (int u = 0; u < OWN; ++u) {
            const int bin = kLBins - 1 - (OWN * tid + u);
            const uint32_t excl = cum;
            cum += own[u];
            start[bin] = excl;
            hist[bin] = 0u;                                                    // from here on: the bin's drop cursor
            if (excl < (uint32_t)k && (uint32_t)k <= cum) { misc[0] = (uint32_t)bin; misc[1] = cum; misc[3] = 1u; }
            if (excl < (uint32_t)k && own[u] > (uint32_t)kQMaxPop) misc[2] = 1;   // an over-full bin among those that hold candidates
        }
        __syncthreads();
    }
    const uint32_t tb = misc[0], count = misc[1];
    // fewer than k words in the lists (misc[3] unset: the sampled threshold was too high), or no room: the exact fallback
    if (!misc[3] || count > (uint32_t)kQCap || misc[2]) {              // block-uniform
        const int img = blockIdx.x;
        const float fill = lg ? 0.0f : 1.0f;
        const float* base = p.logits + (int64_t)img * p.sB;
        const uint8_t* excl = p.exclude ? p.exclude + (int64_t)img * p.N : nullptr;
        float* fmap = reinterpret_cast<float*>(const_cast<uint64_t*>(L));          // N floats <= eimg words
        const float qscale = (float)kQBins / range;
        __syncthreads();                                                             // (the list passes' bins are read no more)
        hist[tid] = 0u;                                                              // kQBins == kLargeThreads words
        __syncthreads();
        auto score1 = [&](const float (&xx)[CMAX]) -> float {       // (the strategy-specialised scorers: the same bits as the generic one, fewer registers)
            if (p.strategy == PP_ACQ_ENTROPY) return pixel_score_fast<CMAX, true, PP_ACQ_ENTROPY>(xx, p.C, p.strategy);
            if (p.strategy == PP_ACQ_LEAST_CONFIDENCE) return pixel_score_fast<CMAX, true, PP_ACQ_LEAST_CONFIDENCE>(xx, p.C, p.strategy);
            return pixel_score_fast<CMAX, true, PP_ACQ_MARGIN>(xx, p.C, p.strategy);
        };
        constexpr int PXF = CMAX > 19 ? 1 : 2;                       // pixels per thread and pass: PXF x CMAX registers under the 1024-thread budget
        for (int64_t pix = (int64_t)tid * PXF; pix < p.N; pix += kLargeThreads * PXF) {  // (flat planes, N % 4 == 0: the emitting scorer's layout)
            float x[PXF][CMAX], sc[PXF];
#pragma unroll
            for (int c = 0; c < CMAX; ++c) {
                if constexpr (PXF == 2) {
                    const f32x2_nt v = *reinterpret_cast<const f32x2_nt*>(base + (int64_t)c * p.sC + pix);
                    x[0][c] = v.x; x[1][c] = v.y;
                } else {
                    x[0][c] = base[(int64_t)c * p.sC + pix];
                }
            }
#pragma unroll
            for (int u = 0; u < PXF; ++u) {
                sc[u] = score1(x[u]);
                if (excl && excl[pix + u]) sc[u] = fill;
                fmap[pix + u] = sc[u];
                atomicAdd(&hist[qbin(sc[u], lg, qscale)], 1u);
                __builtin_amdgcn_sched_barrier(0);                  // one pixel's temporaries at a time
            }
        }
        __syncthreads();
        // First the quantised select over the whole score range on the map just written (what topk_qsel_kernel does: kQBins bins were
        // counted while scoring): an image that is here because the sample misled - not because of ties - is done in two more passes
        // over its 0.5 MB map; only ties / constant regions go on to the radix select (one bad sample would otherwise cost 1.4 ms).
        {
            const int bin = kQBins - 1 - tid;                       // kLargeThreads == kQBins
            const uint32_t own = hist[bin];
            uint32_t incl = own;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t x2 = (uint32_t)__shfl_up((int)incl, o, 64);
                if (lane >= o) incl += x2;
            }
            if (lane == 63) misc[8 + wave] = incl;
            if (tid == 0) { misc[2] = 0u; misc[3] = 0u; }
            __syncthreads();
            uint32_t pre = 0;
            for (int w = 0; w < wave; ++w) pre += misc[8 + w];
            incl += pre;
            const uint32_t excl2 = incl - own;
            __syncthreads();                                        // (every thread has read its bin: the words become the drop cursors)
            start[bin] = excl2;
            hist[bin] = 0u;
            if (excl2 < (uint32_t)k && (uint32_t)k <= incl) { misc[0] = (uint32_t)bin; misc[1] = incl; misc[3] = 1u; }
            if (excl2 < (uint32_t)k && own > (uint32_t)kQMaxPop) misc[2] = 1u;
            __syncthreads();
        }
        if (misc[3] && misc[1] <= (uint32_t)kQCap && !misc[2]) {     // block-uniform
            const uint32_t tb2 = misc[0], cnt2 = misc[1];
            PP_LSEL_PROBE(1u);
            for (int64_t pix = tid; pix < p.N; pix += kLargeThreads) {
                const float sc = fmap[pix];
                const uint32_t q = qbin(sc, lg, qscale);
                if (q >= tb2) buf[start[q] + atomicAdd(&hist[q], 1u)] = ((uint64_t)order_key(sc, lg) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)pix);
            }
            __syncthreads();
            for (uint32_t e = (uint32_t)tid; e < cnt2; e += kLargeThreads) {
                const uint64_t me = buf[e];
                const uint32_t q = qbin(key_to_float((uint32_t)(me >> 32), lg), lg, qscale);
                const uint32_t a = start[q], b = a + hist[q];
                uint32_t rank = a;
                for (uint32_t t = a; t < b; ++t) rank += buf[t] > me ? 1u : 0u;
                if (rank < (uint32_t)k) {
                    out_idx[(int64_t)img * k + rank] = (int32_t)(0xFFFFFFFFu - (uint32_t)me);
                    if (out_val) out_val[(int64_t)img * k + rank] = key_to_float((uint32_t)(me >> 32), lg);
                }
            }
            return;
        }
        __syncthreads();
        PP_LSEL_PROBE(2u);
        uint32_t* rh = reinterpret_cast<uint32_t*>(smem);                           // 256 + 64 words, then P 64-bit words (P <= 8192: k <= 7281)
        int P = 1;
        while (P < k) P <<= 1;
        topk_large_body(fmap, p.N, k, lg, rh, rh + 256, reinterpret_cast<uint64_t*>(smem + (256 + 64) * 4), P, out_idx + (int64_t)img * k,
                        out_val ? out_val + (int64_t)img * k : nullptr);
        return;
    }
    PP_LSEL_PROBE(0u);
    sweep(!one_chunk, [&](uint64_t w) {
        const uint32_t q = lbin((uint32_t)(w >> 32), lg, tv, lscale);
        if (q >= tb) buf[start[q] + atomicAdd(&hist[q], 1u)] = w;
    });
    __syncthreads();
    for (uint32_t p = (uint32_t)tid; p < count; p += kLargeThreads) {
        const uint64_t me = buf[p];
        const uint32_t q = lbin((uint32_t)(me >> 32), lg, tv, lscale);
        const uint32_t a = start[q], b = a + hist[q];
        uint32_t rank = a;
        for (uint32_t t = a; t < b; ++t) rank += buf[t] > me ? 1u : 0u;
        if (rank < (uint32_t)k) {
            out_idx[(int64_t)blockIdx.x * k + rank] = (int32_t)(0xFFFFFFFFu - (uint32_t)me);
            if (out_val) out_val[(int64_t)blockIdx.x * k + rank] = key_to_float((uint32_t)(me >> 32), lg);
        }
    }
}
constexpr int kLSelLds = kQCap * 8 + 2 * kLBins * 4 + 128;

// ---- host side ---------------------------------------------------------------------------------------
// Sum over T forward passes of softmax(logits[t]) per pixel and of the strategy's score of each pass (the MC-dropout
// branch, query.py:181-187: `uc_map += uc_map_; prob += prob_`), scaled: p_c = exp(x_c - m) / S and the score formulas in
// the reference's operation order (libm expf / logf), one thread per pixel, any strides.
__global__ __launch_bounds__(kBlock) void softmax_sum_kernel(const float* logits, int T, int C, int W, int64_t N, int64_t sT, int64_t sC,
                                                            int64_t sH, int64_t sW, float* out, float* uc_out, int strategy, float scale,
                                                            int accumulate)
{
    const int64_t pix = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (pix >= N) return;
    const int64_t hh = pix / W, ww = pix - hh * W;
    const float* base = logits + hh * sH + ww * sW;
    // per-class sums live in registers, PP_ACQ_MAX_CLASSES at a time: wider heads repeat the T passes per chunk of classes (the
    // per-pass maximum and sum are recomputed; the strategy's score is accumulated in the first chunk's round only)
    float uc = 0.0f;
    for (int c0 = 0; c0 < C; c0 += PP_ACQ_MAX_CLASSES) {
        const int cn = C - c0 < PP_ACQ_MAX_CLASSES ? C - c0 : PP_ACQ_MAX_CLASSES;
        float acc[PP_ACQ_MAX_CLASSES];
        for (int c = 0; c < cn; ++c) acc[c] = 0.0f;
        for (int t = 0; t < T; ++t) {
            const float* xt = base + (int64_t)t * sT;
            if (c0 == 0) {
                uc += mc_pass_score<-1, 0, false>([&](int c) { return xt[(int64_t)c * sC]; }, C, strategy,
                                                  [&](int c, float pc) { if (c < cn) acc[c] += pc; });
            } else {
                float m = xt[0];
                for (int c = 1; c < C; ++c) m = fmaxf(m, xt[(int64_t)c * sC]);
                float S = 0.0f;
                for (int c = 0; c < C; ++c) S += expf(xt[(int64_t)c * sC] - m);
                for (int c = 0; c < cn; ++c) acc[c] += expf(xt[(int64_t)(c0 + c) * sC] - m) / S;
            }
        }
        if (out)
            for (int c = 0; c < cn; ++c) {
                const int64_t o = (int64_t)(c0 + c) * N + pix;
                out[o] = accumulate ? fmaf(scale, acc[c], out[o]) : scale * acc[c];
            }
    }
    if (uc_out) uc_out[pix] = accumulate ? fmaf(scale, uc, uc_out[pix]) : scale * uc;
}

static bool is_flat_vec4(const float* logits, const uint8_t* exclude, const float* out_map, int64_t H, int64_t W,
                         int64_t sB, int64_t sC, int64_t sH, int64_t sW)
{
    const int64_t N = H * W;
    return sW == 1 && (sH == W || H == 1) && N % 4 == 0 && sC % 4 == 0 && sB % 4 == 0 &&
           (reinterpret_cast<uintptr_t>(logits) & 15) == 0 && (reinterpret_cast<uintptr_t>(exclude) & 3) == 0 &&
           (reinterpret_cast<uintptr_t>(out_map) & 15) == 0;
}

static bool is_dense_nhwc(const float* logits, int64_t C, int64_t H, int64_t W, int64_t sB, int64_t sC, int64_t sH, int64_t sW)
{
    return C > 1 && C <= 32 && sC == 1 && sW == C && (sH == W * C || H == 1) && (H * W) % 4 == 0 && sB % 4 == 0 &&
           (reinterpret_cast<uintptr_t>(logits) & 15) == 0;
}

// Deterministic in (B, N, vec4) so that pp_acq_workspace_bytes can size the candidate buffer.
Plan make_plan(int64_t B, int64_t N, bool vec4, bool force_ppt4)
{
    Plan pl;
    pl.vec4 = vec4;
    // want >= ~2048 waves in flight (256 CUs x 8) before growing the per-thread tile
    // measured on MI355X (profiles/r01_acq_tuning.txt): 8 pixels/thread at 3 waves/SIMD streams at 5.95 TB/s;
    // 16 pixels/thread spills, 4 waves/SIMD spills.
    const int64_t waves8 = B * cdiv(N, (int64_t)kBlock * 8) * (kBlock / kWave);
    pl.ppt = (waves8 >= 2048 && !force_ppt4) ? 8 : 4;
    // class planes of 4 MB and more: XCD-contiguous block order (1024 x 2048, least confidence, B = 8: 0.655 -> 0.677 of 8 TB/s; on
    // 512 KB planes it costs 5 %, on 2 MB planes it is neutral: profiles/r04_acq_layout.txt)
    pl.xcd = vec4 && g_knobs.tune_xcd != 1 && (g_knobs.tune_xcd == 2 || N * 4 >= (4ll << 20));
    if (g_knobs.tune_ppt && vec4 && !force_ppt4) pl.ppt = g_knobs.tune_ppt;
    pl.blocks_per_image = (int)cdiv(N, (int64_t)kBlock * pl.ppt);
    pl.waves_per_image = pl.blocks_per_image;          // candidate lists per image: one per BLOCK since round 5 (block_emit_topk)
    return pl;
}

constexpr int kAcqOcc21 = 2, kAcqOcc11 = 3;     // defaults of the C = 21 / C = 11 scorers (see launch_acq)

template <int CMAX, bool EXACT>
static int launch_acq(const AcqParams& p, const Plan& pl, int64_t B, hipStream_t st)
{
    EventScope ev(st);
    dim3 grid((unsigned)(B * pl.blocks_per_image)), block(kBlock);
    // the non-default scorers (reference-order, from-prob) are only built for the 4-pixel tile
    const bool alt = p.from_prob || exact_formula();
    if (pl.nhwc) {
        if constexpr (EXACT && CMAX <= 21) {
            // asynchronous LDS-DMA variant for the three dataset class counts (tuning value 8 keeps the synchronous kernel)
            if (!alt && g_knobs.tune_occ != 8) {
                if (pl.ppt == 8) hipLaunchKernelGGL((acq_nhwc_dma_kernel<CMAX, 8>), grid, block, 0, st, p);
                else             hipLaunchKernelGGL((acq_nhwc_dma_kernel<CMAX, 4>), grid, block, 0, st, p);
                return check_launch("acq_nhwc_dma_kernel");
            }
        }
        if constexpr (CMAX <= 32) {
            if (p.from_prob)          hipLaunchKernelGGL((acq_nhwc_kernel<CMAX, EXACT, 4, 2>), grid, block, 0, st, p);
            else if (exact_formula()) hipLaunchKernelGGL((acq_nhwc_kernel<CMAX, EXACT, 4, 1>), grid, block, 0, st, p);
            else if (pl.ppt == 8)     hipLaunchKernelGGL((acq_nhwc_kernel<CMAX, EXACT, 8, 0>), grid, block, 0, st, p);
            else                      hipLaunchKernelGGL((acq_nhwc_kernel<CMAX, EXACT, 4, 0>), grid, block, 0, st, p);
            return check_launch("acq_nhwc_kernel");
        }
    }
#define PP_LAUNCH_ACQ4(VEC, G)                                                                                    \
    do {                                                                                                          \
        if (p.from_prob)          hipLaunchKernelGGL((acq_kernel<CMAX, EXACT, VEC, G, 2>), grid, block, 0, st, p); \
        else if (exact_formula()) hipLaunchKernelGGL((acq_kernel<CMAX, EXACT, VEC, G, 1>), grid, block, 0, st, p); \
        else                      hipLaunchKernelGGL((acq_kernel<CMAX, EXACT, VEC, G, 0>), grid, block, 0, st, p); \
    } while (0)
    if (pl.vec4) {
        if constexpr (CMAX == 11 || CMAX == 19 || CMAX == 21) {
            // the three dataset class counts: pixels per thread x waves per SIMD chosen per count (profiles/r04_acq_layout.txt);
            // pp_debug_set_acq_tuning overrides either for A/B.  C = 21: 21 planes x 8 pixels do not fit the 170-VGPR budget of
            // 3 waves/SIMD (23 spilled registers, 0.56 of the HBM roofline on VOC 320x320) - 2 waves/SIMD, or 4 pixels per thread.
            if (!alt) {
                int occ = CMAX == 21 ? kAcqOcc21 : (CMAX == 11 ? kAcqOcc11 : 3);
                const int g = pl.ppt == 8 ? 2 : 1;
                if (g_knobs.tune_occ >= 2 && g_knobs.tune_occ <= 4) occ = g_knobs.tune_occ;
                AcqParams q = p;
                if (pl.xcd) {
                    q.nb = (int)grid.x;
                    q.xcd_per = (int)cdiv(q.nb, 8);
                    grid = dim3((unsigned)(q.xcd_per * 8));
                }
                if (q.elist) {       // large-k selection without the map: candidates beyond the sampled threshold key
                    by_strategy(q.strategy, [&](auto s) {
                        constexpr int S = decltype(s)::value;
                        if (g == 2) hipLaunchKernelGGL((acq_kernel<CMAX, EXACT, 4, 2, 0, 3, S, false, true, true>), grid, block, 0, st, q);
                        else        hipLaunchKernelGGL((acq_kernel<CMAX, EXACT, 4, 1, 0, 3, S, false, true, true>), grid, block, 0, st, q);
                    });
                    return check_launch("acq_kernel<emit>");
                }
                if (q.qhist) {       // large-k selection: map + the image's score histogram in one pass (run_large skips its histogram pass)
                    constexpr int O = CMAX == 21 ? kAcqOcc21 : (CMAX == 11 ? kAcqOcc11 : 3);
                    if (g == 2) hipLaunchKernelGGL((acq_kernel<CMAX, EXACT, 4, 2, 0, O, -1, true>), grid, block, 0, st, q);
                    else        hipLaunchKernelGGL((acq_kernel<CMAX, EXACT, 4, 1, 0, O, -1, true>), grid, block, 0, st, q);
                    return check_launch("acq_kernel<hist>");
                }
#define PP_ACQ_GO(G, O) hipLaunchKernelGGL((acq_kernel<CMAX, EXACT, 4, G, 0, O>), grid, block, 0, st, q)
                if (g_knobs.acq_strat_spec && !g_knobs.tune_occ && !q.out_map) {            // (with the map written - large k - the generic kernel measured no slower)
                    // the strategy as a compile-time constant: the chains the other two strategies need are not computed (100-145 VGPRs
                    // instead of 168-184: entropy runs four waves per SIMD, C = 21 three instead of two); bit 10 of the tuning word: off
                    by_strategy(q.strategy, [&](auto s) {
                        constexpr int S = decltype(s)::value;
                        if (g_knobs.nt_off) {
                            if (g == 2) hipLaunchKernelGGL((acq_kernel<CMAX, EXACT, 4, 2, 0, 3, S, false, false>), grid, block, 0, st, q);
                            else        hipLaunchKernelGGL((acq_kernel<CMAX, EXACT, 4, 1, 0, 3, S, false, false>), grid, block, 0, st, q);
                        } else {
                            if (g == 2) hipLaunchKernelGGL((acq_kernel<CMAX, EXACT, 4, 2, 0, 3, S>), grid, block, 0, st, q);
                            else        hipLaunchKernelGGL((acq_kernel<CMAX, EXACT, 4, 1, 0, 3, S>), grid, block, 0, st, q);
                        }
                    });
                    return check_launch("acq_kernel");
                }
                if (g == 2) { if (occ == 2) PP_ACQ_GO(2, 2); else if (occ == 4) PP_ACQ_GO(2, 4); else PP_ACQ_GO(2, 3); }
                else        { if (occ == 2) PP_ACQ_GO(1, 2); else if (occ == 4) PP_ACQ_GO(1, 4); else PP_ACQ_GO(1, 3); }
#undef PP_ACQ_GO
                return check_launch("acq_kernel");
            }
        }
        if constexpr (CMAX <= 32) {
            if (pl.ppt == 8 && !alt) hipLaunchKernelGGL((acq_kernel<CMAX, EXACT, 4, 2, 0>), grid, block, 0, st, p);
            else                     PP_LAUNCH_ACQ4(4, 1);
        }
    } else {
        if (pl.ppt == 8 && !alt) hipLaunchKernelGGL((acq_kernel<CMAX, EXACT, 1, 8, 0>), grid, block, 0, st, p);
        else                     PP_LAUNCH_ACQ4(1, 4);
    }
#undef PP_LAUNCH_ACQ4
    return check_launch("acq_kernel");
}

// class counts beyond the register-resident scorers (or forced, for A/B): streamed class vector, 4 pixels per thread
bool stream_classes(int64_t C) { return C > PP_ACQ_MAX_CLASSES || g_knobs.tune_occ == 10; }

static int launch_acq_stream(const AcqParams& p, const Plan& pl, int64_t B, hipStream_t st)
{
    EventScope ev(st);
    if (pl.ppt != 4) return fail(PP_ERR_BAD_ARG, "streamed scorer: plan with %d pixels per thread", pl.ppt);
    dim3 grid((unsigned)(B * pl.blocks_per_image)), block(kBlock);
    const int math = p.from_prob ? 2 : (exact_formula() ? 1 : 0);
#define PP_STREAM(VEC, G)                                                                                  \
    do {                                                                                                   \
        if (math == 2)      hipLaunchKernelGGL((acq_stream_kernel<VEC, G, 2>), grid, block, 0, st, p);     \
        else if (math == 1) hipLaunchKernelGGL((acq_stream_kernel<VEC, G, 1>), grid, block, 0, st, p);     \
        else                hipLaunchKernelGGL((acq_stream_kernel<VEC, G, 0>), grid, block, 0, st, p);     \
    } while (0)
    if (pl.vec4) PP_STREAM(4, 1); else PP_STREAM(1, 4);
#undef PP_STREAM
    return check_launch("acq_stream_kernel");
}

// which launches can take the histogram epilogue (acq_kernel<..., HIST>): the flat float4 form of the three dataset class counts
static bool acq_hist_fusable(const AcqParams& p, const Plan& pl)
{
    return g_knobs.hist_fuse && pl.vec4 && !p.from_prob && !exact_formula() && !g_knobs.tune_occ && !stream_classes(p.C) && p.out_map && !p.cand &&
           (p.C == 11 || p.C == 19 || p.C == 21);
}

// ---- the list select (sampled threshold + candidate emission) ---------------------------------------------------------------------
static bool emit_size_ok(int64_t N, int64_t k) { return N >= 16384 && k * 8 <= N; }
// Entries per image: a wave's segment holds PPT * 64 words and is followed by kSegPad unused ones, so that the segments do not all start
// on a 4 KB boundary.  (The scorer launch costs 0.365 ms without the list stores and 0.38-0.42 with them - the spread is between boxes /
// hours, not between layouts: the pad, whole-wave stores from an LDS staging list and non-temporal stores all measured the same.)
constexpr int kSegPad = 32;
static size_t emit_list_entries(int64_t N) { return align_up((size_t)N, 2048) / 256 * (256 + kSegPad); }
// first region of the large-k workspace: the score map, or the per-wave candidate segments (the exact fallback writes an image's score
// map over that image's own segments once its block has consumed them)
static size_t map_region_bytes(int64_t B, int64_t N, int64_t k)
{
    return emit_size_ok(N, k) ? align_up((size_t)B * emit_list_entries(N) * 8, 256) : align_up((size_t)B * N * 4, 256);
}
static size_t emit_extra_bytes(int64_t B, int64_t N, int64_t k)
{
    if (!emit_size_ok(N, k)) return 0;
    // threshold keys, per-wave counts
    return align_up((size_t)B * 4, 256) + align_up((size_t)B * (align_up((size_t)N, 2048) / 256) * 4, 256);
}
static bool acq_emit_ok(const AcqParams& p, const Plan& pl, int64_t B, int64_t k, float qs, bool caller_map)
{
    return g_knobs.emit && !caller_map && emit_size_ok(p.N, k) && large_q_ok(B, k, qs) && pl.vec4 && !p.from_prob && !exact_formula() &&
           !g_knobs.tune_occ && !stream_classes(p.C) && (p.C == 11 || p.C == 19 || p.C == 21);
}

static int dispatch_acq(const AcqParams& p, Plan pl, int64_t B, hipStream_t st);

// p: the map-writing launch's parameters; region0: the first workspace region (candidate segments); tail: what follows the large-k scratch
static int run_emit_select(AcqParams p, const Plan& pl, int64_t B, int64_t k, int largest, float qs, void* region0, void* tail,
                           int32_t* out_idx, float* out_val, hipStream_t st)
{
    uint32_t* tkey = reinterpret_cast<uint32_t*>(tail);
    uint32_t* ecnt = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(tail) + align_up((size_t)B * 4, 256));
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(topk_lsel_kernel<11>), hipFuncAttributeMaxDynamicSharedMemorySize, kLSelLds);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(topk_lsel_kernel<19>), hipFuncAttributeMaxDynamicSharedMemorySize, kLSelLds);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(topk_lsel_kernel<21>), hipFuncAttributeMaxDynamicSharedMemorySize, kLSelLds);
        attr_set = true;
    }
    const int segsz = pl.ppt * kWave + kSegPad;
    AcqParams q = p;
    q.out_map = nullptr;
    q.tkey = tkey;
    q.elist = reinterpret_cast<uint64_t*>(region0);
    q.ecnt = ecnt;
    q.eimg = (int64_t)emit_list_entries(p.N);
    q.nseg = pl.blocks_per_image * (kBlock / kWave);
    q.segst = segsz;
    q.sample_locs = g_knobs.sample_locs;
    q.sample_gpl = g_knobs.sample_gpl;
    while ((int64_t)q.sample_locs * q.sample_gpl * 4 * 4 > p.N && q.sample_locs > 16) q.sample_locs >>= 1;      // (16384 pixels and up: >= 4 slots per location)
    const int64_t sample_n = (int64_t)q.sample_locs * q.sample_gpl * 4;
    int64_t want = (sample_n * g_knobs.emit_mult16 * k + 16 * p.N - 1) / (16 * p.N);
    if (want < 1) want = 1;
    if (want > sample_n) want = sample_n;
    const dim3 sgrid((unsigned)B), sblock(kSampleThreads), lblock(kLargeThreads);
    const float range = (float)kQBins / qs;
#define PP_BY_C(KERNEL, GRID, BLOCK, LDS, ...)                                                                 \
    switch (p.C) {                                                                                             \
        case 11: hipLaunchKernelGGL((KERNEL<11>), GRID, BLOCK, LDS, st, __VA_ARGS__); break;                   \
        case 19: hipLaunchKernelGGL((KERNEL<19>), GRID, BLOCK, LDS, st, __VA_ARGS__); break;                   \
        default: hipLaunchKernelGGL((KERNEL<21>), GRID, BLOCK, LDS, st, __VA_ARGS__); break;                   \
    }
    PP_BY_C(acq_sample_thr_kernel, sgrid, sblock, 0, q, qs, (uint32_t)want, tkey);
    if (int rc = check_launch("acq_sample_thr_kernel")) return rc;
    if (int rc = dispatch_acq(q, pl, B, st)) return rc;
    PP_BY_C(topk_lsel_kernel, sgrid, lblock, kLSelLds, q, (const uint64_t*)q.elist, (const uint32_t*)ecnt, (const uint32_t*)tkey, q.eimg, q.nseg,
            segsz, (int)k, largest, range, out_idx, out_val PP_LSEL_PROBE_ARG);
#undef PP_BY_C
    return check_launch("topk_lsel_kernel");
}

static int dispatch_acq(const AcqParams& p, Plan pl, int64_t B, hipStream_t st)
{
    if (stream_classes(p.C)) return launch_acq_stream(p, pl, B, st);
    if (p.C > 32) pl.vec4 = false;  // 64-class bucket only on the scalar path (register budget)
    if (!pl.vec4 && g_knobs.tune_occ != 9)   // (tuning value 9 forces the generic strided path for A/B)
        pl.nhwc = is_dense_nhwc(p.logits, p.C, p.N / p.W, p.W, p.sB, p.sC, p.sH, p.sW);
    if (pl.nhwc && (exact_formula() || p.from_prob) && pl.ppt != 4) pl.nhwc = false;
    switch (p.C) {
        case 11: return launch_acq<11, true>(p, pl, B, st);   // CamVid      (args.py:109-116)
        case 19: return launch_acq<19, true>(p, pl, B, st);   // Cityscapes  (args.py:89-94)
        case 21: return launch_acq<21, true>(p, pl, B, st);   // VOC 2012    (args.py:131-141)
        default: break;
    }
    if (p.C <= 32) return launch_acq<32, false>(p, pl, B, st);
    return launch_acq<64, false>(p, pl, B, st);
}

int validate(const float* logits, int64_t B, int64_t C, int64_t H, int64_t W, int strategy)
{
    if (!logits) return fail(PP_ERR_BAD_ARG, "logits is null");
    if (B < 1 || C < 1 || H < 1 || W < 1) return fail(PP_ERR_BAD_ARG, "bad shape B=%lld C=%lld H=%lld W=%lld",
                                                        (long long)B, (long long)C, (long long)H, (long long)W);
    if (C > 0x7FFFFFFFll) return fail(PP_ERR_UNSUPPORTED, "C=%lld", (long long)C);
    if (H * W > 0x7FFFFFFFll || B * H * W / 1024 > 0x7FFFFFFFll) return fail(PP_ERR_UNSUPPORTED, "image too large");
    if (strategy < 0 || strategy > 2) return fail(PP_ERR_BAD_ARG, "unknown strategy %d", strategy);
    return PP_OK;
}

}  // namespace pp

using namespace pp;

extern "C" {

size_t pp_acq_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W, int64_t k)
{
    (void)C;
    if (B < 1 || H < 1 || W < 1 || k < 1 || H > 0x7FFFFFFFll || W > 0x7FFFFFFFll || H * W > 0x7FFFFFFFll || k > H * W || B > 0x7FFFFFFFll) return 0;
    const int64_t N = H * W;
    if (k <= kSmallKMax) {
        // sized for the 4-pixel tile (most waves), an upper bound for every plan
        Plan pl = make_plan(B, N, true, true);
        return merge_ws_bytes(B, (int64_t)pl.waves_per_image * k, k);
    }
    // score map (used when the caller passes no out_map) or candidate segments + large-k scratch + the list select's threshold keys / counts
    return map_region_bytes(B, N, k) + pp_topk_workspace_bytes(B, N, k) + emit_extra_bytes(B, N, k);
}

int pp_acq_score_map(const float* logits, int64_t B, int64_t C, int64_t H, int64_t W, int64_t sB, int64_t sC,
                     int64_t sH, int64_t sW, const uint8_t* exclude, int strategy, float* out_map,
                     pp_stream_t stream)
{
    const ExactScope exact_scope(strategy);
    if (int rc = validate(logits, B, C, H, W, strategy)) return rc;
    if (!out_map) return fail(PP_ERR_BAD_ARG, "out_map is null");
    const int64_t N = H * W;
    Plan pl = make_plan(B, N, is_flat_vec4(logits, exclude, out_map, H, W, sB, sC, sH, sW), exact_formula() != 0 || stream_classes(C));
    AcqParams p{logits, exclude, out_map, nullptr, sB, sC, sH, sW, (int)C, (int)W, N, pl.blocks_per_image, 0,
                strategy, g_knobs.reduce_mode, 0};
    return dispatch_acq(p, pl, B, as_stream(stream));
}

int pp_acq_softmax_sum(const float* logits, int64_t T, int64_t C, int64_t H, int64_t W, int64_t sT, int64_t sC, int64_t sH,
                       int64_t sW, float* prob_out, float* uc_out, int strategy, float scale, int accumulate, pp_stream_t stream)
{
    const ExactScope exact_scope(strategy);
    if (int rc = validate(logits, T, C, H, W, strategy)) return rc;
    if (!prob_out && !uc_out) return fail(PP_ERR_BAD_ARG, "softmax_sum: both outputs are null");
    const int64_t N = H * W;
    const int64_t blocks = (N + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(softmax_sum_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, as_stream(stream), logits, (int)T, (int)C, (int)W, N,
                       sT, sC, sH, sW, prob_out, uc_out, strategy, scale, accumulate);
    return check_launch("softmax_sum_kernel");
}

int pp_uncertainty_from_prob(const float* prob, int64_t B, int64_t C, int64_t H, int64_t W, int64_t sB, int64_t sC,
                             int64_t sH, int64_t sW, int strategy, float* out_map, pp_stream_t stream)
{
    const ExactScope exact_scope(strategy);
    if (int rc = validate(prob, B, C, H, W, strategy)) return rc;
    if (!out_map) return fail(PP_ERR_BAD_ARG, "out_map is null");
    const int64_t N = H * W;
    Plan pl = make_plan(B, N, is_flat_vec4(prob, nullptr, out_map, H, W, sB, sC, sH, sW), true);     // (4 pixels per thread: also what the streamed scorer needs)
    AcqParams p{prob, nullptr, out_map, nullptr, sB, sC, sH, sW, (int)C, (int)W, N, pl.blocks_per_image, 0,
                strategy, g_knobs.reduce_mode, 1};
    return dispatch_acq(p, pl, B, as_stream(stream));
}

int pp_acq_score_topk(const float* logits, int64_t B, int64_t C, int64_t H, int64_t W, int64_t sB, int64_t sC,
                      int64_t sH, int64_t sW, const uint8_t* exclude, int strategy, int64_t k, int32_t* out_idx,
                      float* out_val, float* out_map, void* workspace, size_t ws_bytes, pp_stream_t stream)
{
    const ExactScope exact_scope(strategy);
    if (int rc = validate(logits, B, C, H, W, strategy)) return rc;
    const int64_t N = H * W;
    if (int rc = check_select_args(k, N, "H*W", out_idx, workspace, ws_bytes, pp_acq_workspace_bytes(B, C, H, W, k))) return rc;
    hipStream_t st = as_stream(stream);
    const int largest = strategy != PP_ACQ_MARGIN;

    if (k <= kSmallKMax) {
        Plan pl = make_plan(B, N, is_flat_vec4(logits, exclude, out_map, H, W, sB, sC, sH, sW), exact_formula() != 0 || stream_classes(C));
        const SmallKLists ws = small_k_lists(workspace, B, pl.waves_per_image, k);
        AcqParams p{logits, exclude, out_map, ws.cand, sB, sC, sH, sW, (int)C, (int)W, N, pl.blocks_per_image,
                    (int)k, strategy, g_knobs.reduce_mode, 0};
        if (int rc = dispatch_acq(p, pl, B, st)) return rc;
        return run_merge(ws.cand, ws.n_cand, ws.other, B, (int)k, largest, out_idx, out_val, st);
    }
    // large k: materialise the score map once, then radix-select + sort per image
    float* map = out_map ? out_map : reinterpret_cast<float*>(workspace);
    uint64_t* gbuf = reinterpret_cast<uint64_t*>(reinterpret_cast<char*>(workspace) + map_region_bytes(B, N, k));
    Plan pl = make_plan(B, N, is_flat_vec4(logits, exclude, map, H, W, sB, sC, sH, sW), exact_formula() != 0 || stream_classes(C));
    AcqParams p{logits, exclude, map, nullptr, sB, sC, sH, sW, (int)C, (int)W, N, pl.blocks_per_image, 0, strategy,
                g_knobs.reduce_mode, 0};
    const float qs = score_qscale(strategy, C);
    if (acq_emit_ok(p, pl, B, k, qs, out_map != nullptr))
        return run_emit_select(p, pl, B, k, largest, qs, workspace, reinterpret_cast<char*>(gbuf) + pp_topk_workspace_bytes(B, N, k),
                               out_idx, out_val, st);
    const bool fuse_hist = large_q_ok(B, k, qs) && acq_hist_fusable(p, pl);
    if (fuse_hist) {
        p.qhist = large_hist(gbuf, B, k);
        p.qscale = qs;
        if (hipMemsetAsync(p.qhist, 0, (size_t)B * kQBins * 4, st) != hipSuccess) return fail(PP_ERR_LAUNCH, "topk: memset failed");
    }
    if (int rc = dispatch_acq(p, pl, B, st)) return rc;
    return run_large(map, B, N, k, largest, gbuf, out_idx, out_val, st, qs, fuse_hist);
}

}  // extern "C"
