// acq_topk.hip - the selection on a SCORE MAP on gfx950 (MI355X): pp_topk_select, and the tail of every acquisition entry that ranks
// a map or a set of per-block candidate lists (acq.hip, acq_lowres.hip, acq_mc.hip call run_merge / run_large through acq_host.h).
//   k <= 48   per-block candidate lists (block_emit_topk, acq_device.h) + cand_merge_kernel
//   larger k  the quantised-histogram select where the score range is known or can be taken in one pass, else the four-pass radix
//             select; the one-block radix select (topk_large_body, acq_device.h) is the exact fallback of both
#include <cmath>

#include "acq_host.h"

namespace pp {

// ---- small-k selection straight from a score map (pp_topk_select) ------------------------------------
template <int G>
__global__ __launch_bounds__(kBlock) void topk_small_from_scores_kernel(const float* scores, int64_t N,
                                                                        int blocks_per_image, int k,
                                                                        int largest, uint64_t* cand, int mode)
{
    const int img = blockIdx.x / blocks_per_image;
    const int blk = blockIdx.x - img * blocks_per_image;
    const int tid = threadIdx.x;
    const float* s = scores + (int64_t)img * N;
    uint32_t kh[G], kl[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int64_t pix = ((int64_t)blk * G + g) * kBlock + tid;
        if (pix < N) {
            kh[g] = order_key(s[pix], largest != 0);
            kl[g] = 0xFFFFFFFFu - (uint32_t)pix;
        } else {
            kh[g] = 0u; kl[g] = 0u;
        }
    }
    __shared__ uint64_t s_surv[kBlock / kWave][kSurvCap];
    __shared__ uint32_t s_cnt[kBlock / kWave];
    __shared__ uint64_t s_top[(kBlock / kWave) * kSmallKMax];
    block_emit_topk<G>(kh, kl, k, cand + ((int64_t)img * blocks_per_image + blk) * k, mode, s_surv, s_cnt, s_top);
}

// ---- candidate merge ---------------------------------------------------------------------------------
// grid (nchunks, B): block (c,b) reduces up to kMergeChunk candidate keys of image b to their top-k with the machinery the scoring
// kernels end in - per-wave threshold prefilter + rank inside LDS (block_emit_topk) - instead of k rounds of a block-wide arg-max
// with two barriers each (10.5 us per level at k = 20; this form: ~3 us).  The last level (nchunks == 1) decodes to out_idx / out_val.
__global__ __launch_bounds__(kBlock) void cand_merge_kernel(const uint64_t* in, int64_t n_in, uint64_t* out_keys,
                                                           int32_t* out_idx, float* out_val, int k, int largest,
                                                           int mode)
{
    __shared__ uint64_t s_surv[kBlock / kWave][kSurvCap];
    __shared__ uint32_t s_cnt[kBlock / kWave];
    __shared__ uint64_t s_top[(kBlock / kWave) * kSmallKMax];
    const int b = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
    const uint64_t* src = in + (int64_t)b * n_in;
    const int64_t lo = (int64_t)c * kMergeChunk;
    uint32_t kh[kMergeItems], kl[kMergeItems];
#pragma unroll
    for (int j = 0; j < kMergeItems; ++j) {
        const int64_t i = lo + (int64_t)j * kBlock + tid;
        uint64_t v = i < n_in ? src[i] : 0ull;
        kh[j] = (uint32_t)(v >> 32);
        kl[j] = (uint32_t)v;
    }
    if (out_keys) {
        block_emit_topk<kMergeItems>(kh, kl, k, out_keys + ((int64_t)b * gridDim.x + c) * k, mode, s_surv, s_cnt, s_top);
        return;
    }
    block_emit_topk<kMergeItems>(kh, kl, k, s_top, mode, s_surv, s_cnt, s_top);      // merged list -> s_top[0..k)
    if (tid < kWave) {
        __builtin_amdgcn_wave_barrier();
        for (int r = tid; r < k; r += kWave) {
            const uint64_t v = s_top[r];
            const uint32_t mh = (uint32_t)(v >> 32), ml = (uint32_t)v;
            out_idx[(int64_t)b * k + r] = mh == 0u ? -1 : (int32_t)(0xFFFFFFFFu - ml);
            if (out_val) out_val[(int64_t)b * k + r] = key_to_float(mh, largest != 0);
        }
    }
}

__global__ __launch_bounds__(kLargeThreads) void topk_large_kernel(const float* scores, int64_t N, int k, int largest,
                                                                  uint64_t* gbuf, int P, int32_t* out_idx,
                                                                  float* out_val, const int* only_if = nullptr)
{
    if (only_if && !only_if[blockIdx.x]) return;      // fallback launch of the quantised select: flagged images only
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t* hist = reinterpret_cast<uint32_t*>(smem);            // 256
    uint32_t* misc = hist + 256;                                   // 64
    uint64_t* buf = gbuf ? gbuf + (int64_t)blockIdx.x * P : reinterpret_cast<uint64_t*>(smem + (256 + 64) * 4);
    topk_large_body(scores + (int64_t)blockIdx.x * N, N, k, largest != 0, hist, misc, buf, P, out_idx + (int64_t)blockIdx.x * k,
                    out_val ? out_val + (int64_t)blockIdx.x * k : nullptr);
}

// ---- large-k, multi-block: the radix select of topk_large_kernel taken out of the one-block-per-image kernel -------------
// Four histogram passes over the score map (8 key bits each, 256 bins), every pass a grid of blocks_per_image x B
// blocks that add their LDS histograms into the image's global one with integer atomics (order-independent, exact).  No
// separate scan launch: the blocks of pass p (and the final kernel) re-derive the digits chosen so far from the earlier
// histograms - a 256-bin scan per earlier pass.  The final one-block-per-image kernel then knows the threshold key T, how
// many keys equal to T it must take and how many exist, compacts in one barrier-free sweep and sorts.
constexpr int kSelBins = 256;         // 8-bit digits, four passes: 8 KiB of LDS histograms per block instead of 64 KiB (the 2048-bin
constexpr int kSelPasses = 4;         // / three-pass form spent most of a pass zeroing and flushing its LDS: 84 us per pass)
constexpr int kSelSub = 8;            // sub-histograms per block (lane & 7): same-address LDS atomics conflict 8x less

__device__ __forceinline__ uint32_t sel_digit(uint32_t key, int pass) { return (key >> (24 - 8 * pass)) & 255u; }
__device__ __forceinline__ int sel_shift(int pass) { return 24 - 8 * pass; }
__device__ __forceinline__ uint32_t sel_mask(int pass) { return pass == 0 ? 0u : (0xFFFFFFFFu << (32 - 8 * pass)); }

// From the top bin down: the digit d with  #(bins above d) < remaining <= #(bins above d) + hist[d]  (d = 0 if the bins above
// it hold fewer than `remaining`).  Parallel: thread t < 256 owns bin 255 - t, an inclusive scan over the threads gives the
// count of bins at or above each one (a serial walk with its dependent LDS reads costs ~10 us per 256-bin histogram).
// h: 256 words in LDS or global; sh: >= 8 words of LDS; out[0] = d, out[1] = remaining - #above, out[2] = hist[d].
// Must be called by all threads of the block (two barriers); blocks of 256 or more threads.
__device__ __forceinline__ void sel_find_digit(const uint32_t* h, uint32_t remaining, uint32_t* sh, uint32_t* out)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    uint32_t own = 0, incl = 0;
    if (t < kSelBins) {
        own = h[kSelBins - 1 - t];
        incl = own;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t v = (uint32_t)__shfl_up((int)incl, o, 64);
            if (lane >= o) incl += v;
        }
        if (lane == 63) sh[wave] = incl;
    }
    __syncthreads();
    if (t < kSelBins) {
        uint32_t base = 0;
        for (int w = 0; w < wave; ++w) base += sh[w];
        incl += base;
        const uint32_t excl = incl - own;
        const bool hit = excl < remaining && remaining <= incl;
        if ((hit && t < kSelBins - 1) || (t == kSelBins - 1 && excl < remaining)) {      // bin 0 takes whatever is left
            out[0] = (uint32_t)(kSelBins - 1 - t);
            out[1] = remaining - excl;
            out[2] = own;
        }
    }
    __syncthreads();
}

__device__ __forceinline__ void sel_scan(const uint32_t* hist, uint32_t remaining, uint32_t* sh /*[kSelBins]*/, uint32_t* out /*[3]*/)
{
    sel_find_digit(hist, remaining, sh, out);
}

// hist: [B][kSelPasses][kSelBins] (zeroed by the host before pass 0)
__global__ __launch_bounds__(kBlock) void select_hist_kernel(const float* scores, int64_t N, int k, int largest, int pass, uint32_t* hist)
{
    __shared__ uint32_t lh[kSelSub][kSelBins];
    __shared__ uint32_t sh[kBlock];
    __shared__ uint32_t res[3];
    const int b = blockIdx.y;
    const float* s = scores + (int64_t)b * N;
    uint32_t* H = hist + (int64_t)b * kSelPasses * kSelBins;
    const bool lg = largest != 0;
    uint32_t prefix = 0, remaining = (uint32_t)k;
    for (int q = 0; q < pass; ++q) {
        sel_scan(H + q * kSelBins, remaining, sh, res);
        prefix |= res[0] << sel_shift(q);
        remaining = res[1];
        __syncthreads();
    }
    for (int i = threadIdx.x; i < kSelSub * kSelBins; i += kBlock) (&lh[0][0])[i] = 0u;
    __syncthreads();
    const uint32_t mask = sel_mask(pass);
    const int sub = threadIdx.x & (kSelSub - 1);
    const int64_t per = (N + gridDim.x - 1) / gridDim.x;
    const int64_t i0 = (int64_t)blockIdx.x * per, i1 = i0 + per < N ? i0 + per : N;
    int64_t i = i0 + threadIdx.x;
    for (; i + 3 * kBlock < i1; i += 4 * kBlock) {            // four loads in flight per thread
        const float v0 = s[i], v1 = s[i + kBlock], v2 = s[i + 2 * kBlock], v3 = s[i + 3 * kBlock];
        const uint32_t k0 = order_key(v0, lg), k1 = order_key(v1, lg), k2 = order_key(v2, lg), k3 = order_key(v3, lg);
        if ((k0 & mask) == prefix) atomicAdd(&lh[sub][sel_digit(k0, pass)], 1u);
        if ((k1 & mask) == prefix) atomicAdd(&lh[sub][sel_digit(k1, pass)], 1u);
        if ((k2 & mask) == prefix) atomicAdd(&lh[sub][sel_digit(k2, pass)], 1u);
        if ((k3 & mask) == prefix) atomicAdd(&lh[sub][sel_digit(k3, pass)], 1u);
    }
    for (; i < i1; i += kBlock) {
        const uint32_t key = order_key(s[i], lg);
        if ((key & mask) == prefix) atomicAdd(&lh[sub][sel_digit(key, pass)], 1u);
    }
    __syncthreads();
    uint32_t* Hp = H + pass * kSelBins;
    for (int d = threadIdx.x; d < kSelBins; d += kBlock) {
        uint32_t c = 0;
#pragma unroll
        for (int u = 0; u < kSelSub; ++u) c += lh[u][d];
        if (c) atomicAdd(&Hp[d], c);
    }
}

// One 1024-thread block per image: threshold from the three histograms, barrier-free compaction, bitonic sort.
__global__ __launch_bounds__(kLargeThreads) void topk_large_sel_kernel(const float* scores, int64_t N, int k, int largest, const uint32_t* hist,
                                                                      uint64_t* gbuf, int P, int32_t* out_idx, float* out_val)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t* shs = reinterpret_cast<uint32_t*>(smem);            // 256: scan partials
    uint32_t* misc = shs + 256;                                    // 64
    uint64_t* buf = gbuf ? gbuf + (int64_t)blockIdx.x * P : reinterpret_cast<uint64_t*>(smem + (256 + 64) * 4);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* s = scores + (int64_t)blockIdx.x * N;
    const uint32_t* H = hist + (int64_t)blockIdx.x * kSelPasses * kSelBins;
    const bool lg = largest != 0;
    uint32_t T = 0, need_eq = (uint32_t)k, total_eq = 0;
    for (int q = 0; q < kSelPasses; ++q) {
        sel_scan(H + q * kSelBins, need_eq, shs, misc);
        T |= misc[0] << sel_shift(q);
        need_eq = misc[1];
        total_eq = misc[2];
        __syncthreads();
    }
    if (tid == 0) { misc[4] = 0; /* out count */ misc[5] = 0; /* eq seen so far (ordered path) */ }
    __syncthreads();
    const bool all_eq = need_eq == total_eq;          // every key equal to T is taken: their order is irrelevant (the sort fixes it)
    auto push = [&](uint32_t key, int64_t i, bool valid) {
        const bool take = valid && (key > T || (all_eq && key == T));
        const unsigned long long bal = __ballot(take);
        if (bal) {
            uint32_t wbase = 0;
            if (lane == 0) wbase = atomicAdd(&misc[4], (uint32_t)__popcll(bal));
            wbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)wbase);
            if (take) buf[wbase + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = ((uint64_t)key << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)i);
        }
    };
    {
        int64_t base = 0;
        for (; base + 4 * kLargeThreads <= N; base += 4 * kLargeThreads) {        // four loads in flight per thread
            const int64_t i = base + tid;
            const float v0 = s[i], v1 = s[i + kLargeThreads], v2 = s[i + 2 * kLargeThreads], v3 = s[i + 3 * kLargeThreads];
            push(order_key(v0, lg), i, true);
            push(order_key(v1, lg), i + kLargeThreads, true);
            push(order_key(v2, lg), i + 2 * kLargeThreads, true);
            push(order_key(v3, lg), i + 3 * kLargeThreads, true);
        }
        for (; base < N; base += kLargeThreads) {
            const int64_t i = base + tid;
            push(i < N ? order_key(s[i], lg) : 0u, i, i < N);
        }
    }
    __syncthreads();
    if (!all_eq) {
        // ties at the threshold (constant regions): the need_eq keys == T with the LOWEST indices, found in index order
        for (int64_t base = 0; base < N; base += kLargeThreads) {
            const int64_t i = base + tid;
            const bool eq = i < N && order_key(s[i], lg) == T;
            const unsigned long long bal = __ballot(eq);
            if (lane == 0) misc[8 + wave] = (uint32_t)__popcll(bal);
            __syncthreads();
            uint32_t before = misc[5];
            for (int q = 0; q < wave; ++q) before += misc[8 + q];
            const uint32_t rank = before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
            if (eq && rank < need_eq) {
                const uint32_t pos = atomicAdd(&misc[4], 1u);
                buf[pos] = ((uint64_t)T << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)i);
            }
            __syncthreads();
            if (tid == 0) {
                uint32_t tot = 0;
                for (int q = 0; q < kLargeThreads / kWave; ++q) tot += misc[8 + q];
                misc[5] += tot;
            }
            __syncthreads();
            if (misc[5] >= need_eq) break;
        }
        __syncthreads();
    }
    for (int j = k + tid; j < P; j += kLargeThreads) buf[j] = 0ull;
    __syncthreads();
    // bitonic sort, descending.  Strides >= 8 exchange through `buf`; the three last stages of every size (strides 4, 2, 1)
    // and the whole of sizes 2..8 run in registers on the thread's own 8 consecutive keys: 66 barrier phases instead of 91.
    auto reg_stages = [&](int size, bool head) {
        for (int g = tid; g < (P >> 3); g += kLargeThreads) {
            uint64_t v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = buf[8 * g + j];
            auto stage = [&](auto S_, int sz) {
                constexpr int S = decltype(S_)::value;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    if ((j & S) == 0) {
                        const bool desc = ((8 * g + j) & sz) == 0;
                        const uint64_t a = v[j], b = v[j + S];
                        const bool sw = (a < b) == desc;
                        v[j] = sw ? b : a;
                        v[j + S] = sw ? a : b;
                    }
                }
            };
            using I1 = std::integral_constant<int, 1>;
            using I2 = std::integral_constant<int, 2>;
            using I4 = std::integral_constant<int, 4>;
            if (head) {
                stage(I1{}, 2);
                stage(I2{}, 4); stage(I1{}, 4);
                stage(I4{}, 8); stage(I2{}, 8); stage(I1{}, 8);
            } else {
                stage(I4{}, size); stage(I2{}, size); stage(I1{}, size);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) buf[8 * g + j] = v[j];
        }
        __syncthreads();
    };
    if (P >= 8) {
        reg_stages(8, true);                                // sizes 2, 4, 8 entirely in registers
        for (int size = 16; size <= P; size <<= 1) {
            for (int stride = size >> 1; stride >= 8; stride >>= 1) {
                for (int t = tid; t < (P >> 1); t += kLargeThreads) {
                    const int pos = 2 * t - (t & (stride - 1));
                    const uint64_t a = buf[pos], b = buf[pos + stride];
                    const bool desc = (pos & size) == 0;
                    if ((a < b) == desc) { buf[pos] = b; buf[pos + stride] = a; }
                }
                __syncthreads();
            }
            reg_stages(size, false);                        // strides 4, 2, 1 of this size
        }
    } else {
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
    }
    for (int j = tid; j < k; j += kLargeThreads) {
        const uint64_t v = buf[j];
        out_idx[(int64_t)blockIdx.x * k + j] = (int32_t)(0xFFFFFFFFu - (uint32_t)v);
        if (out_val) out_val[(int64_t)blockIdx.x * k + j] = key_to_float((uint32_t)(v >> 32), lg);
    }
}

// ---- large-k with a KNOWN score range: one quantised histogram pass, compaction, register / shuffle bitonic sort ------------
// The scorers' outputs live in a known interval (entropy [0, ln C], least confidence and margin [0, 1]), so the 32-bit radix
// digits of the generic select are not needed to find a threshold: kQBins LINEAR bins of the score - a monotone map of the order
// key, so every element of a higher bin precedes every element of a lower one - are filled in ONE pass over the map, the bin that
// holds the k-th element is found by a scan, and everything in that bin or above (k + the bin's population: k + ~130 of 131072
// at the reference's default k = 6553) is dropped into LDS bin by bin and ranked exactly on the full (key, index) words.  Replaces four
// histogram passes + a 66-barrier LDS sort; an image whose candidates do not fit (kQCap in all, kQMaxPop in a bin: heavy ties, constant
// maps) raises its overflow flag and is redone by topk_large_kernel (the exact one-block radix select): the result never depends on the data.
constexpr int kQSub = 8;             // sub-histograms per block (lane & 7)

// Generic maps (pp_topk_select: the random strategy's maps, MC-dropout means - no score range known): one pass takes every image's finite
// minimum and maximum as order keys (mm[2 b] = largest key seen, mm[2 b + 1] = largest complemented key, both zeroed by the host), and the
// quantised select bins (s - lo) * kQBins / (hi - lo) per image.  Infinities fall into the end bins, NaN where order_key puts it; an image
// with a single value fills one bin and goes to the exact fallback like any heavily tied map.
__device__ __forceinline__ void image_range(const uint32_t* mm, int b, float& lo, float& scale)
{
    const uint32_t kmax = mm[2 * b], kmin = ~mm[2 * b + 1];
    const float hi = key_to_float(kmax, true);
    lo = key_to_float(kmin, true);
    if (kmax == 0u || !(hi > lo)) { lo = 0.0f; scale = 1.0f; return; }          // no finite value, or a single one
    scale = (float)kQBins / (hi - lo);
    if (!(scale < 3.0e38f)) scale = 3.0e38f;
}

__global__ __launch_bounds__(kBlock) void select_minmax_kernel(const float* scores, int64_t N, uint32_t* mm)
{
    __shared__ uint32_t smax[kBlock / kWave], smin[kBlock / kWave];
    const int b = blockIdx.y;
    const float* s = scores + (int64_t)b * N;
    const int64_t per = (N + gridDim.x - 1) / gridDim.x;
    const int64_t i0 = (int64_t)blockIdx.x * per, i1 = i0 + per < N ? i0 + per : N;
    uint32_t kx = 0u, kn = 0u;                                  // largest key, largest complemented key (0 = nothing seen)
    for (int64_t i = i0 + threadIdx.x; i < i1; i += kBlock) {
        const float v = s[i];
        if (fabsf(v) <= 3.4028234e38f) {                        // finite (NaN compares false)
            const uint32_t key = order_key(v, true);
            kx = key > kx ? key : kx;
            kn = ~key > kn ? ~key : kn;
        }
    }
    kx = wave_umax(kx, 0);
    kn = wave_umax(kn, 0);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    if (lane == 0) { smax[wave] = kx; smin[wave] = kn; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / kWave; ++w) { kx = smax[w] > kx ? smax[w] : kx; kn = smin[w] > kn ? smin[w] : kn; }
        if (kx) atomicMax(&mm[2 * b], kx);
        if (kn) atomicMax(&mm[2 * b + 1], kn);
    }
}

// hist: [B][kQBins], zeroed by the host
__global__ __launch_bounds__(kBlock) void select_qhist_kernel(const float* scores, int64_t N, int largest, float scale, uint32_t* hist, const uint32_t* mm = nullptr)
{
    __shared__ uint32_t lh[kQSub][kQBins];
    const int b = blockIdx.y;
    const float* s = scores + (int64_t)b * N;
    const bool lg = largest != 0;
    float lo = 0.0f;
    if (mm) image_range(mm, b, lo, scale);                     // generic maps: the image's own finite value range (select_minmax_kernel)
    for (int i = threadIdx.x; i < kQSub * kQBins; i += kBlock) (&lh[0][0])[i] = 0u;
    __syncthreads();
    const int sub = threadIdx.x & (kQSub - 1);
    const int64_t per = (N + gridDim.x - 1) / gridDim.x;
    const int64_t i0 = (int64_t)blockIdx.x * per, i1 = i0 + per < N ? i0 + per : N;
    int64_t i = i0 + threadIdx.x;
    if (i1 > i0 && (per & 3) == 0 && (reinterpret_cast<uintptr_t>(s + i0) & 15) == 0) {
        const float4* s4 = reinterpret_cast<const float4*>(s + i0);
        const int64_t n4 = (i1 - i0) >> 2;                      // (a ragged end of the last block goes through the scalar loop below)
        int64_t j = threadIdx.x;
        auto add4 = [&](const float4& q) {
            atomicAdd(&lh[sub][qbin(q.x - lo, lg, scale)], 1u); atomicAdd(&lh[sub][qbin(q.y - lo, lg, scale)], 1u);
            atomicAdd(&lh[sub][qbin(q.z - lo, lg, scale)], 1u); atomicAdd(&lh[sub][qbin(q.w - lo, lg, scale)], 1u);
        };
        for (; j + 3 * kBlock < n4; j += 4 * kBlock) {          // four 16-byte loads in flight per thread
            const float4 q0 = s4[j], q1 = s4[j + kBlock], q2 = s4[j + 2 * kBlock], q3 = s4[j + 3 * kBlock];
            add4(q0); add4(q1); add4(q2); add4(q3);
        }
        for (; j < n4; j += kBlock) add4(s4[j]);
        i = i0 + 4 * n4 + threadIdx.x;
    }
    for (; i + 3 * kBlock < i1; i += 4 * kBlock) {            // four loads in flight per thread
        const float v0 = s[i], v1 = s[i + kBlock], v2 = s[i + 2 * kBlock], v3 = s[i + 3 * kBlock];
        atomicAdd(&lh[sub][qbin(v0 - lo, lg, scale)], 1u);
        atomicAdd(&lh[sub][qbin(v1 - lo, lg, scale)], 1u);
        atomicAdd(&lh[sub][qbin(v2 - lo, lg, scale)], 1u);
        atomicAdd(&lh[sub][qbin(v3 - lo, lg, scale)], 1u);
    }
    for (; i < i1; i += kBlock) atomicAdd(&lh[sub][qbin(s[i] - lo, lg, scale)], 1u);
    __syncthreads();
    uint32_t* H = hist + (int64_t)b * kQBins;
    for (int d = threadIdx.x; d < kQBins; d += kBlock) {
        uint32_t c = 0;
#pragma unroll
        for (int u = 0; u < kQSub; ++u) c += lh[u][d];
        if (c) atomicAdd(&H[d], c);
    }
}

// One 1024-thread block per image.  The histogram already IS the coarse sort: the number of elements in the bins above bin d is
// where bin d's elements start in the value-sorted output.  Every candidate is dropped into its bin's segment of an LDS list (one
// LDS atomic on the bin's cursor - no wave ballots, no ordering among the threads), then ranks itself inside its segment by
// counting the segment's larger (key, index) words - ~130 comparisons per candidate at 1024 bins - and goes straight to its final
// slot.  No sorting network at all: the round-3 kernel spent ~150 us in a 66-barrier bitonic sort of 8192 words per image.
constexpr int kQSelLds = kQCap * 8 + 2 * kQBins * 4 + 128;

__global__ __launch_bounds__(kLargeThreads) void topk_qsel_kernel(const float* scores, int64_t N, int k, int largest, float scale,
                                                                 const uint32_t* hist, int32_t* out_idx, float* out_val, int* overflow,
                                                                 const uint32_t* mm = nullptr)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint64_t* buf = reinterpret_cast<uint64_t*>(smem);                                   // kQCap candidates, grouped by bin
    uint32_t* start = reinterpret_cast<uint32_t*>(smem + (size_t)kQCap * 8);             // [kQBins] first slot of a bin's segment
    uint32_t* cursor = start + kQBins;                                                   // [kQBins] candidates dropped so far
    uint32_t* misc = cursor + kQBins;                                                    // 32 words
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* s = scores + (int64_t)blockIdx.x * N;
    const bool lg = largest != 0;
    float lo = 0.0f;
    if (mm) image_range(mm, (int)blockIdx.x, lo, scale);
    // thread t owns bin kQBins - 1 - t; an inclusive scan over the threads counts the elements at or above each bin
    {
        const int bin = kQBins - 1 - tid;
        const uint32_t own = hist[(int64_t)blockIdx.x * kQBins + bin];
        uint32_t incl = own;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t v = (uint32_t)__shfl_up((int)incl, o, 64);
            if (lane >= o) incl += v;
        }
        if (lane == 63) misc[8 + wave] = incl;
        if (tid == 0) misc[2] = 0;
        __syncthreads();
        uint32_t base = 0;
        for (int w = 0; w < wave; ++w) base += misc[8 + w];
        incl += base;
        const uint32_t excl = incl - own;
        start[bin] = excl;
        cursor[bin] = 0;
        if (excl < (uint32_t)k && (uint32_t)k <= incl) { misc[0] = (uint32_t)bin; misc[1] = incl; }
        if (excl < (uint32_t)k && own > (uint32_t)kQMaxPop) misc[2] = 1;      // an over-full bin among those that hold candidates
        __syncthreads();
    }
    const uint32_t tb = misc[0], count = misc[1];
    if (count > (uint32_t)kQCap || misc[2]) {          // block-uniform: this image goes to the exact fallback launch
        if (tid == 0) overflow[blockIdx.x] = 1;
        return;
    }
    if (tid == 0) overflow[blockIdx.x] = 0;
    auto drop = [&](float v, int64_t i) {
        const uint32_t q = qbin(v - lo, lg, scale);
        if (q >= tb) {
            const uint32_t pos = start[q] + atomicAdd(&cursor[q], 1u);
            buf[pos] = ((uint64_t)order_key(v, lg) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)i);
        }
    };
    if ((N & 3) == 0 && (reinterpret_cast<uintptr_t>(s) & 15) == 0) {
        // one block reads its image's whole map (512 KB at 256 x 512): four 16-byte loads in flight per thread = 64 KB per CU
        const float4* s4 = reinterpret_cast<const float4*>(s);
        const int64_t n4 = N >> 2;
        auto drop4 = [&](const float4& q, int64_t i4) { drop(q.x, 4 * i4); drop(q.y, 4 * i4 + 1); drop(q.z, 4 * i4 + 2); drop(q.w, 4 * i4 + 3); };
        int64_t base = 0;
        for (; base + 4 * kLargeThreads <= n4; base += 4 * kLargeThreads) {
            const int64_t i = base + tid;
            const float4 q0 = s4[i], q1 = s4[i + kLargeThreads], q2 = s4[i + 2 * kLargeThreads], q3 = s4[i + 3 * kLargeThreads];
            drop4(q0, i); drop4(q1, i + kLargeThreads); drop4(q2, i + 2 * kLargeThreads); drop4(q3, i + 3 * kLargeThreads);
        }
        for (int64_t i = base + tid; i < n4; i += kLargeThreads) drop4(s4[i], i);
    } else {
        int64_t base = 0;
        for (; base + 4 * kLargeThreads <= N; base += 4 * kLargeThreads) {        // four loads in flight per thread
            const int64_t i = base + tid;
            const float v0 = s[i], v1 = s[i + kLargeThreads], v2 = s[i + 2 * kLargeThreads], v3 = s[i + 3 * kLargeThreads];
            drop(v0, i); drop(v1, i + kLargeThreads); drop(v2, i + 2 * kLargeThreads); drop(v3, i + 3 * kLargeThreads);
        }
        for (int64_t i = base + tid; i < N; i += kLargeThreads) drop(s[i], i);
    }
    __syncthreads();
    // rank inside the bin's segment; neighbouring slots share a segment, so most of a wave's reads are broadcasts
    for (uint32_t p = (uint32_t)tid; p < count; p += kLargeThreads) {
        const uint64_t me = buf[p];
        const uint32_t q = qbin(key_to_float((uint32_t)(me >> 32), lg) - lo, lg, scale);
        const uint32_t a = start[q], b = a + cursor[q];
        uint32_t rank = a;
        for (uint32_t t = a; t < b; ++t) rank += buf[t] > me ? 1u : 0u;
        if (rank < (uint32_t)k) {
            out_idx[(int64_t)blockIdx.x * k + rank] = (int32_t)(0xFFFFFFFFu - (uint32_t)me);
            if (out_val) out_val[(int64_t)blockIdx.x * k + rank] = key_to_float((uint32_t)(me >> 32), lg);
        }
    }
}

// (k <= N < 2^31 is checked by every caller: for k above 2^30 the doubling used to overflow and never end - found by tests/test_abi_asan.py)
static int next_pow2(int64_t v) { int64_t p = 1; while (p < v && p < (1ll << 30)) p <<= 1; return (int)p; }

int check_select_args(int64_t k, int64_t N, const char* n_name, const int32_t* out_idx, const void* workspace, size_t ws_bytes, size_t need)
{
    if (k < 1 || k > N) return fail(PP_ERR_BAD_K, "k=%lld outside [1, %s=%lld]", (long long)k, n_name, (long long)N);
    if (!out_idx) return fail(PP_ERR_BAD_ARG, "out_idx is null");
    if (!workspace || ws_bytes < need)
        return fail(PP_ERR_WORKSPACE, "workspace %zu B < required %zu B", ws_bytes, need);
    if (reinterpret_cast<uintptr_t>(workspace) & 255) return fail(PP_ERR_BAD_ARG, "workspace must be 256-B aligned");
    return PP_OK;
}

SmallKLists small_k_lists(void* workspace, int64_t B, int64_t lists, int64_t k)
{
    const int64_t n_cand = lists * k;
    return {n_cand, reinterpret_cast<uint64_t*>(workspace),
            reinterpret_cast<uint64_t*>(reinterpret_cast<char*>(workspace) + align_up((size_t)B * n_cand * 8, 256))};
}

size_t merge_ws_bytes(int64_t B, int64_t n_cand, int64_t k)
{
    // ping-pong: level-0 list + the (smaller) next level
    size_t a = align_up((size_t)B * n_cand * 8, 256);
    size_t b = align_up((size_t)B * cdiv(n_cand, kMergeChunk) * k * 8, 256);
    return a + b;
}

int run_merge(uint64_t* cand, int64_t n_cand, uint64_t* other, int64_t B, int k, int largest,
              int32_t* out_idx, float* out_val, hipStream_t st)
{
    uint64_t* cur = cand;
    uint64_t* nxt = other;
    int64_t n = n_cand;
    for (;;) {
        const int nch = (int)cdiv(n, kMergeChunk);
        dim3 grid(nch, (unsigned)B);
        if (nch == 1) {
            hipLaunchKernelGGL(cand_merge_kernel, grid, dim3(kBlock), 0, st, cur, n, (uint64_t*)nullptr, out_idx,
                               out_val, k, largest, g_knobs.reduce_mode);
            return check_launch("cand_merge_kernel");
        }
        hipLaunchKernelGGL(cand_merge_kernel, grid, dim3(kBlock), 0, st, cur, n, nxt, (int32_t*)nullptr,
                           (float*)nullptr, k, largest, g_knobs.reduce_mode);
        if (int rc = check_launch("cand_merge_kernel")) return rc;
        n = (int64_t)nch * k;
        uint64_t* t = cur; cur = nxt; nxt = t;
    }
}

static size_t large_ws_bytes(int64_t B, int64_t k)
{
    const int P = next_pow2(k);
    const size_t g = P <= kLargeLdsMaxP ? 256 : align_up((size_t)B * P * 8, 256);
    // histograms: four 256-bin radix passes, or the 1024 linear bins of the quantised select (the same bytes) + its overflow flags
    // + the per-image value range of the generic quantised select
    return g + align_up((size_t)B * kSelPasses * kSelBins * 4, 256) + align_up((size_t)B * 4, 256) + align_up((size_t)B * 8, 256);
}

// The scorers' value range as bins per unit score (0: unknown - the generic radix select)
float score_qscale(int strategy, int64_t C)
{
    const float range = strategy == PP_ACQ_ENTROPY ? logf((float)(C > 1 ? C : 2)) : 1.0f;
    return (float)kQBins / range;
}

// the quantised select's conditions and its histogram's place in the large-k scratch (also asked by the scorer launches that fill it)
bool large_q_ok(int64_t B, int64_t k, float qscale)
{
    return qscale > 0.0f && g_knobs.large_q && g_knobs.large_multiblock && B <= 65535 && k + (k / 8 > 256 ? k / 8 : 256) <= kQCap;
}
uint32_t* large_hist(void* ws, int64_t B, int64_t k)
{
    const int P = next_pow2(k);
    return reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(ws) + (P <= kLargeLdsMaxP ? 256 : align_up((size_t)B * P * 8, 256)));
}

// blocks per image of a pass over the map: >= ~2048 blocks per pass, at least 4096 elements per block
static unsigned pass_blocks_per_image(int64_t B, int64_t N)
{
    int64_t bpi = cdiv(2048, B);
    const int64_t by_size = cdiv(N, 4096);
    if (bpi > by_size) bpi = by_size;
    if (bpi < 1) bpi = 1;
    return (unsigned)bpi;
}

// hist_done: the scorer launch already filled the (host-zeroed) quantised histogram
int run_large(const float* map, int64_t B, int64_t N, int64_t k, int largest, void* ws,
              int32_t* out_idx, float* out_val, hipStream_t st, float qscale, bool hist_done)
{
    const dim3 pass_grid(pass_blocks_per_image(B, N), (unsigned)B);
    const int P = next_pow2(k);
    const bool in_lds = P <= kLargeLdsMaxP;
    uint64_t* gbuf = reinterpret_cast<uint64_t*>(ws);
    uint32_t* hist = large_hist(ws, B, k);
    const size_t lds = (256 + 64) * 4 + (in_lds ? (size_t)P * 8 : 0);
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(topk_large_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (256 + 64) * 4 + kLargeLdsMaxP * 8);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(topk_large_sel_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (256 + 64) * 4 + kLargeLdsMaxP * 8);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(topk_qsel_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, kQSelLds);
        attr_set = true;
    }
    // room for the threshold bin's population beside the k picks: the quantised select - over the scorers' known range, or (generic maps,
    // qscale == 0) over every image's own finite range, taken in one more pass: three passes over the map instead of the radix select's five
    const bool generic_q = qscale <= 0.0f && g_knobs.generic_q && large_q_ok(B, k, 1.0f);
    if (large_q_ok(B, k, qscale) || generic_q) {
        static_assert(kQBins * 4 == kSelPasses * kSelBins * 4, "the two histogram layouts share their workspace slot");
        int* flags = reinterpret_cast<int*>(reinterpret_cast<char*>(hist) + align_up((size_t)B * kQBins * 4, 256));
        uint32_t* mm = nullptr;
        if (generic_q) {
            mm = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(flags) + align_up((size_t)B * 4, 256));
            if (hipMemsetAsync(mm, 0, (size_t)B * 8, st) != hipSuccess) return fail(PP_ERR_LAUNCH, "topk: memset failed");
            hipLaunchKernelGGL(select_minmax_kernel, pass_grid, dim3(kBlock), 0, st, map, N, mm);
            if (int rc = check_launch("select_minmax_kernel")) return rc;
            qscale = 1.0f;
        }
        if (!hist_done) {
            if (hipMemsetAsync(hist, 0, (size_t)B * kQBins * 4, st) != hipSuccess) return fail(PP_ERR_LAUNCH, "topk: memset failed");
            hipLaunchKernelGGL(select_qhist_kernel, pass_grid, dim3(kBlock), 0, st, map, N, largest, qscale, hist,
                               (const uint32_t*)mm);
            if (int rc = check_launch("select_qhist_kernel")) return rc;
        }
        hipLaunchKernelGGL(topk_qsel_kernel, dim3((unsigned)B), dim3(kLargeThreads), kQSelLds, st, map, N, (int)k, largest, qscale,
                           hist, out_idx, out_val, flags, (const uint32_t*)mm);
        if (int rc = check_launch("topk_qsel_kernel")) return rc;
        // images whose candidates did not fit (ties at the threshold, constant maps): the exact one-block radix select; the others return at once
        hipLaunchKernelGGL(topk_large_kernel, dim3((unsigned)B), dim3(kLargeThreads), lds, st, map, N, (int)k, largest,
                           in_lds ? (uint64_t*)nullptr : gbuf, P, out_idx, out_val, (const int*)flags);
        return check_launch("topk_large_kernel");
    }
    if (!g_knobs.large_multiblock || B > 65535) {
        hipLaunchKernelGGL(topk_large_kernel, dim3((unsigned)B), dim3(kLargeThreads), lds, st, map, N, (int)k, largest,
                           in_lds ? (uint64_t*)nullptr : gbuf, P, out_idx, out_val, (const int*)nullptr);
        return check_launch("topk_large_kernel");
    }
    if (hipMemsetAsync(hist, 0, (size_t)B * kSelPasses * kSelBins * 4, st) != hipSuccess) return fail(PP_ERR_LAUNCH, "topk: memset failed");
    for (int pass = 0; pass < kSelPasses; ++pass) {
        hipLaunchKernelGGL(select_hist_kernel, pass_grid, dim3(kBlock), 0, st, map, N, (int)k, largest, pass, hist);
        if (int rc = check_launch("select_hist_kernel")) return rc;
    }
    hipLaunchKernelGGL(topk_large_sel_kernel, dim3((unsigned)B), dim3(kLargeThreads), lds, st, map, N, (int)k, largest, hist,
                       in_lds ? (uint64_t*)nullptr : gbuf, P, out_idx, out_val);
    return check_launch("topk_large_sel_kernel");
}

}  // namespace pp

using namespace pp;

extern "C" {

size_t pp_topk_workspace_bytes(int64_t B, int64_t N, int64_t k)
{
    if (B < 1 || N < 1 || k < 1 || N > 0x7FFFFFFFll || k > N || B > 0x7FFFFFFFll) return 0;
    if (k <= kSmallKMax) {
        Plan pl = make_plan(B, N, false);
        return merge_ws_bytes(B, (int64_t)pl.waves_per_image * k, k);
    }
    return large_ws_bytes(B, k);
}

int pp_topk_select(const float* scores, int64_t B, int64_t N, int64_t k, int largest, int32_t* out_idx,
                   float* out_val, void* workspace, size_t ws_bytes, pp_stream_t stream)
{
    if (!scores || !out_idx) return fail(PP_ERR_BAD_ARG, "null pointer");
    if (B < 1 || N < 1 || N > 0x7FFFFFFFll) return fail(PP_ERR_BAD_ARG, "bad shape B=%lld N=%lld", (long long)B, (long long)N);
    if (int rc = check_select_args(k, N, "N", out_idx, workspace, ws_bytes, pp_topk_workspace_bytes(B, N, k))) return rc;
    hipStream_t st = as_stream(stream);
    if (k <= kSmallKMax) {
        Plan pl = make_plan(B, N, false);
        const SmallKLists ws = small_k_lists(workspace, B, pl.waves_per_image, k);
        dim3 grid((unsigned)(B * pl.blocks_per_image)), block(kBlock);
        if (pl.ppt == 8)
            hipLaunchKernelGGL((topk_small_from_scores_kernel<8>), grid, block, 0, st, scores, N,
                               pl.blocks_per_image, (int)k, largest, ws.cand, g_knobs.reduce_mode);
        else
            hipLaunchKernelGGL((topk_small_from_scores_kernel<4>), grid, block, 0, st, scores, N,
                               pl.blocks_per_image, (int)k, largest, ws.cand, g_knobs.reduce_mode);
        if (int rc = check_launch("topk_small_from_scores_kernel")) return rc;
        return run_merge(ws.cand, ws.n_cand, ws.other, B, (int)k, largest, out_idx, out_val, st);
    }
    return run_large(scores, B, N, k, largest, reinterpret_cast<uint64_t*>(workspace), out_idx, out_val, st);
}

}  // extern "C"
