// acq_device.h - what crosses between the acquisition sources (acq.hip, acq_topk.hip, acq_lowres.hip, acq_mc.hip) on the DEVICE side,
// and nothing else does: the block and selection constants, the scorers' parameter blocks, the per-block candidate extraction every
// scorer ends in, the quantised score bins, the low-resolution scorers' selection tail and the one-block radix select (its own kernel
// in acq_topk.hip, the list select's fallback in acq.hip).  The per-pixel scorers are in acq_score.h, the tile frame in lowres_tile.h;
// the host side's counterpart is acq_host.h.
#pragma once
#include "pp_common.h"

namespace pp {

constexpr int kBlock = 256;
constexpr int kSmallKMax = 48;        // fused per-wave extraction up to this k (measured: 0.74/0.70/0.62 of HBM at k=20/32/48, 0.37 at 64); beyond: map + radix select
constexpr int kMergeItems = 16;       // merge kernel: candidates per thread
constexpr int kMergeChunk = kBlock * kMergeItems;
constexpr int kLargeThreads = 1024;
constexpr int kLargeLdsMaxP = 16384;  // 128 KiB of u64 sort keys in LDS
constexpr int kQCap = 8192;           // quantised / list select: candidates per image held in LDS (64 KiB of (key, index) words)
constexpr int kQMaxPop = 1024;        // a bin holding more candidates than this (ties, constant regions) sends the image to the fallback

struct AcqParams {
    const float* logits;
    const uint8_t* exclude;
    float* out_map;      // [B,N] or null
    uint64_t* cand;      // [B, waves_per_image, k] or null
    int64_t sB, sC, sH, sW;
    int C, W;
    int64_t N;           // H*W
    int blocks_per_image;
    int k;
    int strategy;
    int reduce_mode;
    int from_prob;       // 1: input already holds probabilities (UncertaintySampler.__call__, query.py:246-247)
    uint32_t* qhist = nullptr;   // HIST kernels: [B][kQBins] bin counts of the scores written to out_map (zeroed by the host), qscale bins per unit score
    float qscale = 0.0f;
    int xcd_per = 0;     // > 0: XCD-contiguous block order (acq_kernel only): hardware block b works on logical block
    int nb = 0;          //      (b % 8) * xcd_per + b / 8 of nb, so that the blocks one XCD holds walk ONE contiguous eighth of the launch
    // EMIT kernels (large-k selection without the score map): every wave appends the (key, index) words of its pixels at or beyond the image's
    // sampled threshold key to its OWN fixed segment of the image's list and stores how many it wrote - no atomics, no block-level exchange
    const uint32_t* tkey = nullptr;   // [B] threshold order key (acq_sample_thr_kernel)
    uint64_t* elist = nullptr;        // [B][eimg]; wave (blk, w) owns entries [(blk * 4 + w) * PPT * 64, +PPT * 64)
    uint32_t* ecnt = nullptr;         // [B][nseg]
    int64_t eimg = 0;
    int nseg = 0;
    int segst = 0;                    // entries from one segment to the next: PPT * 64 + kSegPad (not a multiple of 4 KB: see emit_list_entries)
    int sample_locs = 0, sample_gpl = 0;   // acq_sample_thr_kernel: locations per image, 4-pixel groups per location
};

// ---- per-wave top-k extraction -------------------------------------------------------------------
// Each lane holds PPT (key, ~idx) pairs; k rounds of {lane-local max, two DPP wave reductions,
// knock out the winner}.  Winner order == global order (key desc, index asc).  Lane 0 stores.
template <int PPT>
__device__ __forceinline__ void wave_extract_topk(uint32_t (&kh)[PPT], uint32_t (&kl)[PPT], int k,
                                                  uint64_t* dst, int mode)
{
    const int lane = threadIdx.x & (kWave - 1);
    for (int r = 0; r < k; ++r) {
        uint32_t lh = 0;
#pragma unroll
        for (int j = 0; j < PPT; ++j) lh = kh[j] > lh ? kh[j] : lh;
        uint32_t ll = 0;
#pragma unroll
        for (int j = 0; j < PPT; ++j) ll = (kh[j] == lh && kl[j] > ll) ? kl[j] : ll;
        const uint32_t mh = wave_umax(lh, mode);
        const uint32_t ml = wave_umax(lh == mh ? ll : 0u, mode);
        if (lane == 0) dst[r] = mh == 0u ? 0ull : (((uint64_t)mh << 32) | ml);
        if (mh == 0u) {  // exhausted (wave-uniform)
            for (int q = r + 1; q < k; ++q)
                if (lane == 0) dst[q] = 0ull;
            break;
        }
#pragma unroll
        for (int j = 0; j < PPT; ++j)
            if (kh[j] == mh && kl[j] == ml) kh[j] = 0u;
    }
}

// Threshold-prefiltered variant (same result).  tau = k-th largest of the 64 lane-local maxima (ballot
// bit search, mostly SALU); the wave's top-k all have key >= tau, and typically only ~k..2k keys survive.
// Survivors go to a per-wave LDS list, each is ranked against the list (broadcast reads) and written
// straight to its sorted slot.  Falls back to the exact loop when ties blow the list up (e.g. a wave
// that sees only excluded pixels).
constexpr int kSurvCap = 256;   // 4 survivors per lane; k up to 64 expects ~k..2k survivors

template <int PPT>
__device__ __forceinline__ void wave_extract_topk_prefilter(uint32_t (&kh)[PPT], uint32_t (&kl)[PPT], int k,
                                                            uint64_t* dst, int mode, volatile uint64_t* sbuf,
                                                            volatile uint32_t* scnt)
{
    const int lane = threadIdx.x & (kWave - 1);
    uint32_t lm = 0;
#pragma unroll
    for (int j = 0; j < PPT; ++j) lm = kh[j] > lm ? kh[j] : lm;
    uint32_t tau = 0;
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t t = tau | (1u << bit);
        if (__popcll(__ballot(lm >= t)) >= k) tau = t;
    }
    if (tau == 0u) tau = 1u;  // fewer than k lanes hold a valid key: every valid key survives
    if (lane == 0) *scnt = 0u;
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int j = 0; j < PPT; ++j)
        if (kh[j] >= tau) {
            const uint32_t pos = atomicAdd(const_cast<uint32_t*>(scnt), 1u);
            if (pos < (uint32_t)kSurvCap) sbuf[pos] = ((uint64_t)kh[j] << 32) | kl[j];
        }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const uint32_t total = *scnt;
    if (total > (uint32_t)kSurvCap) {  // wave-uniform
        wave_extract_topk<PPT>(kh, kl, k, dst, mode);
        return;
    }
    constexpr int SPL = kSurvCap / kWave;          // survivors per lane
    uint64_t sv[SPL];
    int rk[SPL];
#pragma unroll
    for (int j = 0; j < SPL; ++j) {
        sv[j] = (uint32_t)(lane + j * kWave) < total ? sbuf[lane + j * kWave] : 0ull;
        rk[j] = 0;
    }
    if (total <= (uint32_t)kWave) {                 // common case (k ~ 20): one survivor per lane at most
        for (uint32_t i = 0; i < total; ++i) rk[0] += sbuf[i] > sv[0];
    } else {
        for (uint32_t i = 0; i < total; ++i) {
            const uint64_t v = sbuf[i];
#pragma unroll
            for (int j = 0; j < SPL; ++j) rk[j] += v > sv[j];
        }
    }
#pragma unroll
    for (int j = 0; j < SPL; ++j)
        if (sv[j] != 0ull && rk[j] < k) dst[rk[j]] = sv[j];
    for (int r = (int)total + lane; r < k; r += kWave) dst[r] = 0ull;
}

// ---- per-BLOCK candidate list --------------------------------------------------------------------------
// Every wave extracts its own sorted top-k into LDS; wave 0 then merges the block's NW lists by rank (keys are unique - the pixel
// index sits in the low word - so "how many of the NW*k candidates are greater" IS the slot) and ONE list of k leaves the block.
// A quarter of the candidate traffic of per-wave lists, and at 256x512 (64 blocks per image -> 1280 candidates) the merge below needs
// one level instead of two.  s_top: NW * kSmallKMax keys.  dst == nullptr: the merged list stays in s_top[0..k) (cand_merge_kernel).
template <int PPT>
__device__ __forceinline__ void block_emit_topk(uint32_t (&kh)[PPT], uint32_t (&kl)[PPT], int k, uint64_t* dst, int mode,
                                                uint64_t (*s_surv)[kSurvCap], uint32_t* s_cnt, uint64_t* s_top)
{
    constexpr int NW = kBlock / kWave;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
    if (mode == 2) wave_extract_topk<PPT>(kh, kl, k, s_top + wave * k, 0);
    else wave_extract_topk_prefilter<PPT>(kh, kl, k, s_top + wave * k, mode, s_surv[wave], &s_cnt[wave]);
    __syncthreads();
    if (wave != 0) return;
    const int n = NW * k;                                  // <= 192
    constexpr int J = (NW * kSmallKMax + kWave - 1) / kWave;
    uint64_t mine[J];
    int rk[J];
    int nvalid = 0;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int i = lane + j * kWave;
        mine[j] = i < n ? s_top[i] : 0ull;
        rk[j] = 0;
        nvalid += __popcll(__ballot(mine[j] != 0ull));
    }
    if (n <= kWave) {
        for (int i = 0; i < n; ++i) rk[0] += s_top[i] > mine[0];
    } else {
        for (int i = 0; i < n; ++i) {
            const uint64_t v = s_top[i];
#pragma unroll
            for (int j = 0; j < J; ++j) rk[j] += v > mine[j];
        }
    }
    __builtin_amdgcn_wave_barrier();                       // dst may be s_top itself: every lane has finished reading
#pragma unroll
    for (int j = 0; j < J; ++j)
        if (mine[j] != 0ull && rk[j] < k) dst[rk[j]] = mine[j];
    for (int r = nvalid + lane; r < k; r += kWave) dst[r] = 0ull;
}

// ---- quantised score bins (the large-k selection's threshold search, see select_qhist_kernel) ----------------------------------
constexpr int kQBins = 1024;
__device__ __forceinline__ uint32_t qbin(float s, bool lg, float scale)
{
    if (s != s) return lg ? (uint32_t)(kQBins - 1) : 0u;             // NaN: first for largest, last for smallest (order_key's policy)
    const float t = s * scale;
    const int qi = t >= (float)(kQBins - 1) ? kQBins - 1 : (t > 0.0f ? (int)t : 0);
    return (uint32_t)(lg ? qi : kQBins - 1 - qi);
}

// ---- the scorers on the LOW-resolution classifier logits (acq_lowres.hip, acq_mc.hip): a block owns one LowresTile of output pixels ----
struct LowresParams {
    const float* low;    // [B,h,w,ldx] channels-last, C valid channels
    int64_t ldx;
    const uint8_t* exclude;   // [B,Hc,Wc] or null
    float* out_map;           // [B,Hc,Wc] or null
    uint64_t* cand;           // [B, waves_per_image, k] or null
    int h, w, Hc, Wc;
    float sh, sw;
    int align;
    int C, tiles_x, tiles_y, k, strategy, reduce_mode;
    int patch_cap;            // floats of dynamic LDS available for the patch
    uint32_t* qhist = nullptr;   // large-k selection: [B][kQBins] bin counts of the scores written to out_map (zeroed by the host); NULL: none
    float qscale = 0.0f;
};

// The per-pixel selection tail of the low-resolution scorers: exclusion fill, map store, the score's bin (qbins: the block's LDS
// histogram, or null) and the candidate key (larger = selected earlier; ties: the lower flat index).
__device__ __forceinline__ void lowres_emit_key(float sc, int64_t pix, bool largest, float fill, const uint8_t* excl, float* omap,
                                                uint32_t* qbins, float qscale, uint32_t& kh, uint32_t& kl)
{
    if (excl && excl[pix]) sc = fill;
    if (omap) omap[pix] = sc;
    if (qbins) atomicAdd(&qbins[qbin(sc, largest, qscale)], 1u);
    kh = order_key(sc, largest);
    kl = 0xFFFFFFFFu - (uint32_t)pix;
}

// the block's bins -> the image's histogram Hg (non-zero bins only)
__device__ __forceinline__ void lowres_hist_flush(const uint32_t* qbins, uint32_t* Hg)
{
    __syncthreads();
    for (int d = threadIdx.x; d < kQBins; d += kBlock) {
        const uint32_t c = qbins[d];
        if (c) atomicAdd(&Hg[d], c);
    }
}

// ---- large-k: radix select + bitonic sort, one 1024-thread block per image ------------------------------
// query.py:36 top_n_percent mode: k = int(h*w*0.05) (6553 at 256x512) value-sorted indices.
// s: the image's scores; hist: 256 words, misc: 64 words of LDS; buf: P 64-bit words (LDS or global); oi / ov: the image's output rows.
// All kLargeThreads threads of the block.
__device__ __forceinline__ void topk_large_body(const float* s, int64_t N, int k, bool lg, uint32_t* hist, uint32_t* misc, uint64_t* buf,
                                                int P, int32_t* oi, float* ov)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // 1. radix select: T = k-th largest key, need_eq = how many keys == T to take (lowest index first)
    uint32_t prefix = 0, mask = 0, remaining = (uint32_t)k;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (int64_t i = tid; i < N; i += kLargeThreads) {
            const uint32_t key = order_key(s[i], lg);
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t cum = 0;
            int d = 255;
            for (; d > 0; --d) {
                const uint32_t cnt = hist[d];
                if (cum + cnt >= remaining) break;
                cum += cnt;
            }
            misc[0] = (uint32_t)d;
            misc[1] = remaining - cum;
        }
        __syncthreads();
        prefix |= misc[0] << shift;
        mask |= 0xFFu << shift;
        remaining = misc[1];
        __syncthreads();
    }
    const uint32_t T = prefix, need_eq = remaining;

    // 2. compaction (index order matters only among keys == T)
    if (tid == 0) { misc[2] = 0; /* out count */ misc[3] = 0; /* eq seen so far */ }
    __syncthreads();
    for (int64_t base = 0; base < N; base += kLargeThreads) {
        const int64_t i = base + tid;
        const uint32_t key = i < N ? order_key(s[i], lg) : 0u;
        const bool gt = key > T, eq = (i < N) && key == T;
        const unsigned long long bal = __ballot(eq);
        if (lane == 0) misc[8 + wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t before = misc[3];
        for (int q = 0; q < wave; ++q) before += misc[8 + q];
        const uint32_t rank = before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        const bool take = gt || (eq && rank < need_eq);
        if (take) {
            const uint32_t pos = atomicAdd(&misc[2], 1u);
            buf[pos] = ((uint64_t)key << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)i);
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t tot = 0;
            for (int q = 0; q < kLargeThreads / kWave; ++q) tot += misc[8 + q];
            misc[3] += tot;
        }
        __syncthreads();
    }
    for (int j = k + tid; j < P; j += kLargeThreads) buf[j] = 0ull;
    __syncthreads();

    // 3. bitonic sort, descending
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (P >> 1); t += kLargeThreads) {
                const int pos = 2 * t - (t & (stride - 1));
                const uint64_t a = buf[pos], b = buf[pos + stride];
                const bool desc = (pos & size) == 0;
                if ((a < b) == desc) { buf[pos] = b; buf[pos + stride] = a; }
            }
            __syncthreads();
        }
    }
    for (int j = tid; j < k; j += kLargeThreads) {
        const uint64_t v = buf[j];
        oi[j] = (int32_t)(0xFFFFFFFFu - (uint32_t)v);
        if (ov) ov[j] = key_to_float((uint32_t)(v >> 32), lg);
    }
}

}  // namespace pp
