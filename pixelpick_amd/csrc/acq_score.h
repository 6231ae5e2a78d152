// acq_score.h — the per-pixel scorers of the acquisition kernels (acq.hip, acq_lowres.hip, acq_mc.hip): the default scorer, shared
// with every kernel that has to produce the same bits from the same class vector (vis.hip: the confidence / margin / entropy panels),
// the reference-order scorer, one MC-dropout pass, and the streamed form for class counts beyond the register-resident scorers.
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

// ---- per-pixel score ----------------------------------------------------------------------------
// Same operation order as the reference: p_c = exp(x_c - m) / S ; then the strategy's formula.
template <int CMAX, bool EXACT>
__device__ __forceinline__ float pixel_score(const float (&x)[CMAX], int C, int strategy, int from_prob)
{
    // (-p) * log p and the running sum are rounded separately, as torch and the oracle do (hipcc contracts a * b + c by default, and
    // whether it does depends on how the loop was unrolled: the HIP __fmul_rn / __fadd_rn are plain operators and do not stop it)
#pragma clang fp contract(off)
    if (from_prob) {  // x is prob: the UncertaintySampler formulas verbatim
        if (strategy == PP_ACQ_ENTROPY) {
            float acc = 0.0f;
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                if (EXACT || c < C) acc += (-x[c]) * logf(x[c]);
            return acc;
        }
        float t1 = -INFINITY, t2 = -INFINITY;
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
            if (EXACT || c < C) {
                t2 = fmaxf(t2, fminf(t1, x[c]));
                t1 = fmaxf(t1, x[c]);
            }
        return strategy == PP_ACQ_LEAST_CONFIDENCE ? 1.0f - t1 : fabsf(t1 - t2);
    }
    float m = x[0];
#pragma unroll
    for (int c = 1; c < CMAX; ++c)
        if (EXACT || c < C) m = fmaxf(m, x[c]);
    float e[CMAX];
    float S = 0.0f;
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
        if (EXACT || c < C) {
            e[c] = expf(x[c] - m);
            S += e[c];
        }
    if (strategy == PP_ACQ_ENTROPY) {  // query.py:230  (-p*log p).sum(dim=1); 0*log 0 -> NaN as reference
        float acc = 0.0f;
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
            if (EXACT || c < C) {
                float p = e[c] / S;
                acc += (-p) * logf(p);
            }
        return acc;
    } else if (strategy == PP_ACQ_LEAST_CONFIDENCE) {  // query.py:234  1 - max_c p ; max e == exp(0) == 1
        return 1.0f - 1.0f / S;
    } else {  // query.py:238-239  |top1 - top2| of p ; division is monotone so top-2 of e give top-2 of p
        float t1 = -INFINITY, t2 = -INFINITY;
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
            if (EXACT || c < C) {
                t2 = fmaxf(t2, fminf(t1, e[c]));
                t1 = fmaxf(t1, e[c]);
            }
        return fabsf(t1 / S - t2 / S);
    }
}

// ---- MC-dropout: the score of ONE stochastic pass at one pixel (query.py:181-187) ---------------------------------
// softmax_sum_kernel's arithmetic, shared with the low-resolution MC scorers so that both produce the same bits:
//   m = max_c x_c ; S = sum_c expf(x_c - m) ; p_c = expf(x_c - m) / S ; then the strategy's formula on p in class order
// (libm expf / logf, the reference's operation order; the entropy term is ONE fused multiply-add per class, spelled out so that
// it does not depend on how a caller's loop was unrolled).  x(c): the pass's logit of class c; on_prob(c, p_c): called once per class.
//   CMAX == 0  any class count: the loops run to C and expf is evaluated twice per class (softmax_sum_kernel)
//   CMAX  > 0  C <= CMAX (EXACT: C == CMAX), loops unrolled, expf(x_c - m) stays in registers between the sum and the division
//   STRAT >= 0 the strategy is a compile-time constant: only its own chain is computed (no logf outside entropy)
template <int STRAT, int CMAX, bool EXACT, typename X, typename P>
__device__ __forceinline__ float mc_pass_score(X x, int C, int strategy_rt, P on_prob)
{
    constexpr bool kReg = CMAX > 0;
    constexpr bool kEnt = STRAT < 0 || STRAT == PP_ACQ_ENTROPY, kT1 = STRAT < 0 || STRAT != PP_ACQ_ENTROPY,
                   kT2 = STRAT < 0 || STRAT == PP_ACQ_MARGIN;
    const int strategy = STRAT >= 0 ? STRAT : strategy_rt;
    const int n = kReg ? CMAX : C;
    float e[kReg ? CMAX : 1];
    float m = x(0);
    if constexpr (kReg) {
#pragma unroll
        for (int c = 1; c < CMAX; ++c)
            if (EXACT || c < C) m = fmaxf(m, x(c));
    } else {
        for (int c = 1; c < n; ++c) m = fmaxf(m, x(c));
    }
    float S = 0.0f;
    if constexpr (kReg) {
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
            if (EXACT || c < C) {
                e[c] = expf(x(c) - m);
                S += e[c];
            }
    } else {
        for (int c = 0; c < n; ++c) S += expf(x(c) - m);
    }
    float ent = 0.0f, t1 = -INFINITY, t2 = -INFINITY;
    auto one = [&](int c, float ec) {
        const float pc = ec / S;
        on_prob(c, pc);
        if (kEnt) ent = fmaf(-pc, logf(pc), ent);
        if (kT2) t2 = fmaxf(t2, fminf(t1, pc));
        if (kT1) t1 = fmaxf(t1, pc);
    };
    if constexpr (kReg) {
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
            if (EXACT || c < C) one(c, e[c]);
    } else {
        for (int c = 0; c < n; ++c) one(c, expf(x(c) - m));
    }
    return strategy == PP_ACQ_ENTROPY ? ent : (strategy == PP_ACQ_LEAST_CONFIDENCE ? 1.0f - t1 : fabsf(t1 - t2));
}

// ---- any class count: C > PP_ACQ_REG_CLASSES ------------------------------------------------------------
// The scorers above keep a pixel's class vector in registers (C <= 64).  The reference takes whatever class count the model emits
// (query.py:190 softmaxes dim 1 of any width), so wider heads STREAM the class vector instead: two (default scorer) or three
// (reference operation order) passes over the pixel's classes, the later ones served by L2, with the same expressions in the same
// order as pixel_score_fast / pixel_score - forced onto a C <= 64 input (pp_debug_set_acq_tuning occ = 10) the maps are bit-equal
// to the register kernels' (tests/test_acq_gpu.py).  Load(c, v) fills v[0..VEC) with class c of the thread's VEC pixels.
template <int VEC, int MATH, typename Load>
__device__ __forceinline__ void score_stream(Load load, int C, int strategy, float (&s)[VEC])
{
#pragma clang fp contract(off)      // as pixel_score; the default scorer's fused steps are spelled fmaf()
    float v[VEC];
    if constexpr (MATH == 2) {                       // input holds probabilities (UncertaintySampler.__call__)
        float acc[VEC], t1[VEC], t2[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) { acc[i] = 0.0f; t1[i] = -INFINITY; t2[i] = -INFINITY; }
        for (int c = 0; c < C; ++c) {
            load(c, v);
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                if (strategy == PP_ACQ_ENTROPY) acc[i] += (-v[i]) * logf(v[i]);
                else { t2[i] = fmaxf(t2[i], fminf(t1[i], v[i])); t1[i] = fmaxf(t1[i], v[i]); }
            }
        }
#pragma unroll
        for (int i = 0; i < VEC; ++i)
            s[i] = strategy == PP_ACQ_ENTROPY ? acc[i] : (strategy == PP_ACQ_LEAST_CONFIDENCE ? 1.0f - t1[i] : fabsf(t1[i] - t2[i]));
        return;
    }
    float m[VEC], x2[VEC], xmin[VEC];
    load(0, v);
#pragma unroll
    for (int i = 0; i < VEC; ++i) { m[i] = v[i]; x2[i] = -INFINITY; xmin[i] = v[i]; }
    for (int c = 1; c < C; ++c) {
        load(c, v);
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            x2[i] = fmaxf(x2[i], fminf(m[i], v[i]));
            m[i] = fmaxf(m[i], v[i]);
            xmin[i] = fminf(xmin[i], v[i]);
        }
    }
    float S[VEC], T[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) { S[i] = 0.0f; T[i] = 0.0f; }
    if constexpr (MATH == 0) {
        for (int c = 0; c < C; ++c) {
            load(c, v);
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const float d = v[i] - m[i];
                const float e = fast_exp(d);
                S[i] += e;
                T[i] = fmaf(e, -d, T[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            if (strategy == PP_ACQ_ENTROPY) {
                float ent = logf(S[i]) + T[i] / S[i];
                if (xmin[i] - m[i] < -87.0f) {
                    if (expf(xmin[i] - m[i]) / S[i] == 0.0f) ent = __uint_as_float(0x7FC00000u);
                }
                s[i] = ent;
            } else if (strategy == PP_ACQ_LEAST_CONFIDENCE) {
                s[i] = 1.0f - 1.0f / S[i];
            } else {
                s[i] = fabsf(1.0f / S[i] - expf(x2[i] - m[i]) / S[i]);
            }
        }
    } else {                                         // reference operation order (query.py:190,229-239)
        for (int c = 0; c < C; ++c) {
            load(c, v);
#pragma unroll
            for (int i = 0; i < VEC; ++i) S[i] += expf(v[i] - m[i]);
        }
        if (strategy == PP_ACQ_LEAST_CONFIDENCE) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) s[i] = 1.0f - 1.0f / S[i];
            return;
        }
        float t1[VEC], t2[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) { T[i] = 0.0f; t1[i] = -INFINITY; t2[i] = -INFINITY; }
        for (int c = 0; c < C; ++c) {
            load(c, v);
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const float e = expf(v[i] - m[i]);
                if (strategy == PP_ACQ_ENTROPY) {
                    const float pr = e / S[i];
                    T[i] += (-pr) * logf(pr);
                } else {
                    t2[i] = fmaxf(t2[i], fminf(t1[i], e));
                    t1[i] = fmaxf(t1[i], e);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < VEC; ++i) s[i] = strategy == PP_ACQ_ENTROPY ? T[i] : fabsf(t1[i] / S[i] - t2[i] / S[i]);
    }
}

}  // namespace pp
