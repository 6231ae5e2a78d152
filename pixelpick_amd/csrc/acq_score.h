// acq_score.h — the default per-pixel scorer of the acquisition kernels (acq.hip), shared with every kernel that has to
// produce the same bits from the same class vector (vis.hip: the confidence / margin / entropy panels).
#pragma once
#include "pp_common.h"

namespace pp {

// Default scorer: algebraically identical, ~5x fewer VALU slots.  With d_c = x_c - m, e_c = exp(d_c):
//   entropy = -sum p_c log p_c = log S + (sum e_c (m - x_c)) / S      (both terms >= 0: no cancellation)
//   least-confidence = 1 - 1/S ;  margin = |1/S - exp(x_(2) - m)/S|
// e_c uses v_exp_f32 on d*log2(e): absolute error <= ~1e-7 on every term (terms are <= 1), the same
// class as the ulp differences between libm implementations.  The reference's 0*log 0 = NaN behaviour
// (query.py:230) is kept exactly: NaN iff the smallest p_c = exp(x_min - m)/S rounds to 0.
__device__ __forceinline__ float fast_exp(float d) { return __builtin_amdgcn_exp2f(d * 1.44269504088896340736f); }

// STRAT >= 0: the strategy is a compile-time constant - the chains the other two strategies need (second maximum: margin only;
// minimum and the e * d sum: entropy only) are not computed at all (fewer VALU slots and registers: C = 21 fits three waves per SIMD).
template <int CMAX, bool EXACT, int STRAT = -1>
__device__ __forceinline__ float pixel_score_fast(const float (&x)[CMAX], int C, int strategy_rt)
{
    const int strategy = STRAT >= 0 ? STRAT : strategy_rt;
    constexpr bool kX2 = STRAT < 0 || STRAT == PP_ACQ_MARGIN, kEnt = STRAT < 0 || STRAT == PP_ACQ_ENTROPY;
    float m = x[0], x2 = -INFINITY, xmin = x[0];
#pragma unroll
    for (int c = 1; c < CMAX; ++c)
        if (EXACT || c < C) {
            if (kX2) x2 = fmaxf(x2, fminf(m, x[c]));
            m = fmaxf(m, x[c]);
            if (kEnt) xmin = fminf(xmin, x[c]);
        }
    float S = 0.0f, T = 0.0f;
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
        if (EXACT || c < C) {
            const float d = x[c] - m;
            const float e = fast_exp(d);
            S += e;
            if (kEnt) T = fmaf(e, -d, T);
        }
    if (strategy == PP_ACQ_ENTROPY) {
        float ent = logf(S) + T / S;
        if (xmin - m < -87.0f) {                    // rare: possible underflow of the smallest probability
            if (expf(xmin - m) / S == 0.0f) ent = __uint_as_float(0x7FC00000u);
        }
        return ent;
    } else if (strategy == PP_ACQ_LEAST_CONFIDENCE) {
        return 1.0f - 1.0f / S;
    } else {
        return fabsf(1.0f / S - expf(x2 - m) / S);
    }
}

}  // namespace pp
