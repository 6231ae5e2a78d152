// metrics.hip — device-side step metrics: argmax over classes + confusion-matrix histogram.
//
// Replaces, per train/val step, `logits.argmax(dim=1)`, two full-map D2H copies and a numpy bincount
// (model.py:124-125,194-196; utils/metrics.py:168-177 RunningScore._fast_hist/update): only the C x C
// histogram ever leaves the device.  Integer atomics: deterministic.
#include "pp_common.h"

namespace pp {

__global__ __launch_bounds__(256) void confusion_kernel(const float* logits, const int64_t* target, int B, int C, int64_t HW,
                                                        int64_t sB, int64_t sC, unsigned long long* hist)
{
    extern __shared__ unsigned int sh[];   // C*C block-private counters
    for (int i = threadIdx.x; i < C * C; i += 256) sh[i] = 0u;
    __syncthreads();
    const int64_t total = (int64_t)B * HW;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t t = target[e];
        if (t < 0 || t >= C) continue;                       // utils/metrics.py:169 mask
        const int64_t b = e / HW, pix = e - b * HW;
        const float* px = logits + b * sB + pix;
        float m = px[0];
        int am = 0;
        for (int c = 1; c < C; ++c) {
            const float v = px[c * sC];
            if (v > m) { m = v; am = c; }                    // first maximum, like torch.argmax on CPU
        }
        atomicAdd(&sh[(int)t * C + am], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C * C; i += 256)
        if (sh[i]) atomicAdd(&hist[i], (unsigned long long)sh[i]);
}

// ---- any class count the label format carries (C <= 256) ------------------------------------------------------------------
// A C x C image of block-private counters stops fitting in LDS at 105 classes, so wider heads count straight into the global
// int64 histogram - after the wave has aggregated: the lanes that hold the same (target, prediction) pair elect their first lane,
// which adds their number in ONE atomic.  Label maps are spatially coherent, so the 64 neighbouring pixels of a wave usually
// hold a handful of distinct pairs.  Integer counts: exact, whatever order the atomics arrive in.
__device__ __forceinline__ void wave_count_pairs(int key /* t*C + p, or -1: not counted */, unsigned long long* hist)
{
    const int lane = (int)(threadIdx.x & (kWave - 1));
    unsigned long long todo = __ballot(key >= 0);
    while (todo) {                                           // wave-uniform: one round per distinct pair
        const int leader = __ffsll((long long)todo) - 1;
        const int k0 = __shfl(key, leader, kWave);
        const unsigned long long same = __ballot(key == k0);
        if (lane == leader) atomicAdd(&hist[k0], (unsigned long long)__popcll(same));
        todo &= ~same;
    }
}

__device__ __forceinline__ int64_t load_label(const void* target, int kind, int64_t e)
{
    return kind == 1 ? (int64_t) reinterpret_cast<const uint8_t*>(target)[e] : reinterpret_cast<const int64_t*>(target)[e];
}

// FROM_LABELS: pred is a u8 label map, hist[t, pred] += 1 where 0 <= t < C and pred < C;
// otherwise the prediction is the streamed argmax of the logits (first maximum: equal logits give the lowest class).
template <bool FROM_LABELS>
__global__ __launch_bounds__(256) void confusion_wide_kernel(const float* logits, const uint8_t* pred, const void* target,
                                                             int target_kind, int C, int64_t HW, int64_t sB, int64_t sC, int64_t total,
                                                             unsigned long long* hist)
{
    // every lane of a wave takes part in wave_count_pairs: the loop bound is the wave's first element
    const int64_t lane = threadIdx.x & (kWave - 1);
    for (int64_t e0 = (int64_t)blockIdx.x * 256 + threadIdx.x - lane; e0 < total; e0 += (int64_t)gridDim.x * 256) {
        const int64_t e = e0 + lane;
        int key = -1;
        if (e < total) {
            const int64_t t = load_label(target, target_kind, e);
            if (t >= 0 && t < C) {                               // utils/metrics.py:169 mask
                int am;
                if (FROM_LABELS) {
                    am = pred[e];
                } else {
                    const int64_t b = e / HW, pix = e - b * HW;
                    const float* px = logits + b * sB + pix;
                    float m = px[0];
                    am = 0;
#pragma unroll 8
                    for (int c = 1; c < C; ++c) {
                        const float v = px[c * sC];
                        if (v > m) { m = v; am = c; }
                    }
                }
                if (am < C) key = (int)t * C + am;
            }
        }
        wave_count_pairs(key, hist);
    }
}

}  // namespace pp

using namespace pp;

extern "C" {

int pp_confusion_matrix_update(const float* logits, int B, int C, int64_t HW, int64_t sB, int64_t sC, const int64_t* target,
                               int64_t* hist, pp_stream_t stream)
{
    if (!logits || !target || !hist) return fail(PP_ERR_BAD_ARG, "confusion_matrix: null");
    if (C < 1 || C > 256) return fail(PP_ERR_UNSUPPORTED, "confusion_matrix: C=%d (1..256 classes)", C);
    int64_t nblk = cdiv((int64_t)B * HW, 256 * 8);
    if (nblk > 2048) nblk = 2048;
    if (nblk < 1) nblk = 1;
    if (C > 104) {   // no C x C image in LDS: wave-aggregated counts into the global histogram
        hipLaunchKernelGGL(confusion_wide_kernel<false>, dim3((unsigned)nblk), dim3(256), 0, as_stream(stream), logits,
                           (const uint8_t*)nullptr, (const void*)target, 2, C, HW, sB, sC, (int64_t)B * HW,
                           reinterpret_cast<unsigned long long*>(hist));
        return check_launch("confusion_wide_kernel");
    }
    hipLaunchKernelGGL(confusion_kernel, dim3((unsigned)nblk), dim3(256), (size_t)C * C * 4, as_stream(stream), logits, target, B, C,
                       HW, sB, sC, reinterpret_cast<unsigned long long*>(hist));
    return check_launch("confusion_kernel");
}

int pp_confusion_matrix_from_labels(const uint8_t* pred, const void* target, int target_kind, int64_t n, int C, int64_t* hist,
                                    pp_stream_t stream)
{
    if (!pred || !target || !hist) return fail(PP_ERR_BAD_ARG, "confusion_matrix_from_labels: null");
    if (target_kind != 1 && target_kind != 2) return fail(PP_ERR_BAD_ARG, "confusion_matrix_from_labels: unknown target_kind %d", target_kind);
    if (n < 0) return fail(PP_ERR_BAD_ARG, "confusion_matrix_from_labels: n=%lld", (long long)n);
    if (C < 1 || C > 256) return fail(PP_ERR_UNSUPPORTED, "confusion_matrix_from_labels: C=%d (pred is one byte per pixel: 1..256 classes)", C);
    if (n == 0) return PP_OK;
    int64_t nblk = cdiv(n, 256 * 8);
    if (nblk > 2048) nblk = 2048;
    hipLaunchKernelGGL(confusion_wide_kernel<true>, dim3((unsigned)nblk), dim3(256), 0, as_stream(stream), (const float*)nullptr, pred,
                       target, target_kind, C, (int64_t)1, (int64_t)0, (int64_t)0, n, reinterpret_cast<unsigned long long*>(hist));
    return check_launch("confusion_wide_kernel");
}

}  // extern "C"
