// lowres_tile.h - what every kernel that works from the LOW-resolution classifier output shares: the four bilinear taps of an
// output pixel, the tile of output pixels a block owns with the source patch it interpolates from, and the host's bound on that
// patch.  The values are bilerp()'s (pp_common.h) - the bits pp_bilinear_fwd writes - in every user: pp_acq_lowres_*,
// pp_predict_lowres, pp_vis_lowres, pp_sparse_ce_lowres_fwd_bwd.
#pragma once
#include "pp_common.h"

#include <algorithm>
#include <cmath>
#include <type_traits>

namespace pp {

// A tile of T output pixels spans at most ceil(scale*(T-1)) + 3 source pixels along an axis (i0 of the first .. i1 of the last:
// the source coordinates of the two ends lie scale*(T-1) apart, truncation and the +1 of i1 add at most two, the ceil one more),
// and never more than the axis has.  Floats of the patch of a 64-column x tile_rows tile at the odd pixel pitch C | 1: the
// `patch_cap` LowresTile::stage() traps on, so the planners size the dynamic LDS with this and nothing else.
inline int64_t lowres_patch_floats(float sh, float sw, int64_t h, int64_t w, int tile_rows, int64_t C)
{
    const int64_t pw = std::min<int64_t>(w, (int64_t)std::ceil((double)sw * (kWave - 1)) + 3);
    const int64_t ph = std::min<int64_t>(h, (int64_t)std::ceil((double)sh * (tile_rows - 1)) + 3);
    return ph * pw * (C | 1);
}

// f(integral_constant<int, CMAX>, bool_constant<EXACT>) of the class-vector instantiation that serves C classes: the three dataset
// class counts exactly (no per-class predicate), any other count up to 32 / 64 on the generic forms
template <typename F>
inline int lowres_by_classes(int64_t C, F&& f)
{
    switch (C) {
        case 11: return f(std::integral_constant<int, 11>{}, std::true_type{});
        case 19: return f(std::integral_constant<int, 19>{}, std::true_type{});
        case 21: return f(std::integral_constant<int, 21>{}, std::true_type{});
        default: break;
    }
    if (C <= 32) return f(std::integral_constant<int, 32>{}, std::false_type{});
    return f(std::integral_constant<int, 64>{}, std::false_type{});
}

// The four source pixels of one output pixel (class vectors, contiguous) and its weights; at(c) is class c interpolated.  Kept as
// two row pointers and two column offsets, not four pointers: in the tile kernels a wave owns whole output rows, so the rows are
// wave-uniform (scalar registers) and only the offsets are per lane - four pointers cost the widest instantiations their last
// free VGPRs.  Off: the offsets' type - 32 bits are enough inside an LDS patch, and keep the address arithmetic in 32 bits.
template <typename Off = int64_t>
struct LowresTaps {
    const float *r0, *r1;
    Off o0, o1;
    float h0, h1, w0, w1;
    __device__ __forceinline__ float at(int c) const { return bilerp(h0, h1, w0, w1, r0[o0 + c], r0[o1 + c], r1[o0 + c], r1[o1 + c]); }
};

// base: source pixel (row 0, column 0) of lh / lw's indices, in rows of w pixels, `pitch` floats from a pixel to the next
__device__ __forceinline__ LowresTaps<> lowres_taps(const float* base, int64_t pitch, int w, const Lerp& lh, const Lerp& lw)
{
    const int64_t row_pitch = w * pitch;
    return LowresTaps<>{base + lh.i0 * row_pitch, base + lh.i1 * row_pitch, lw.i0 * pitch, lw.i1 * pitch, lh.l0, lh.l1, lw.l0, lw.l1};
}

template <int CMAX, bool EXACT, typename Off>
__device__ __forceinline__ void lowres_class_vector(const LowresTaps<Off>& t, int C, float (&x)[CMAX])
{
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
        if (EXACT || c < C) x[c] = t.at(c);
}

// The tile of one block: 64 output columns (one per lane) x `tile_rows` output rows of a [Hc, Wc] crop, and the source patch
// [r_lo, r_lo + ph) x [c_lo, c_lo + pw) it interpolates from.  LDS: the patch is staged at the odd pixel pitch CP = C | 1 (lanes on
// neighbouring source columns hit different banks) and the taps point into it; otherwise the "patch" is the whole image in memory
// (origin 0, pitch ldx).  P is any parameter block with h, w, Hc, Wc, sh, sw, align, ldx, patch_cap; the frame holds what it
// derives from it and takes `p` again where it needs the geometry (a copy held in the frame stays live in scalar registers through
// the whole kernel, and the wide instantiations have none to spare).  Two steps: the constructor (what stage() needs) and
// set_lane() (what taps() needs), so that a kernel that stages once keeps the lane's columns out of the staging loop.  Lanes
// right of the crop (!xin) take the crop's last column: valid addresses for a kernel that keeps its wave converged.
template <bool LDS>
struct LowresTile {
    using Off = std::conditional_t<LDS, int, int64_t>;
    int C, nthr;
    int c_lo, r_lo, pw, ph;
    int X0, Y0, X;            // first output column and row of the tile; this lane's output column
    bool xin;                 // X lies inside the crop
    float w0, w1;             // this lane's column weights
    Off o0, o1, row_pitch;    // this lane's two source columns, and a source row, in floats from the patch's origin

    template <typename P>
    __device__ __forceinline__ LowresTile(const P& p, int C_, int tx, int ty, int tile_rows, int nthr_) : C(C_), nthr(nthr_)
    {
        X0 = tx * kWave;
        Y0 = ty * tile_rows;
        const int X1 = min(X0 + kWave - 1, p.Wc - 1), Y1 = min(Y0 + tile_rows - 1, p.Hc - 1);
        if constexpr (LDS) {
            c_lo = lerp_src(X0, p.w, p.sw, p.align).i0;
            r_lo = lerp_src(Y0, p.h, p.sh, p.align).i0;
            pw = lerp_src(X1, p.w, p.sw, p.align).i1 - c_lo + 1;
            ph = lerp_src(Y1, p.h, p.sh, p.align).i1 - r_lo + 1;
        } else {
            c_lo = 0; r_lo = 0; pw = p.w; ph = p.h;
        }
    }

    template <typename P>
    __device__ __forceinline__ void set_lane(const P& p, int lane)
    {
        X = X0 + lane;
        xin = X < p.Wc;
        const Lerp lw = lerp_src(xin ? X : p.Wc - 1, p.w, p.sw, p.align);
        const Off pitch = LDS ? (Off)(C | 1) : (Off)p.ldx;
        w0 = lw.l0; w1 = lw.l1;
        o0 = (lw.i0 - c_lo) * pitch; o1 = (lw.i1 - c_lo) * pitch;
        row_pitch = pw * pitch;
    }

    // the patch of the image at `base` -> s_patch.  NO barrier: the caller orders it against the patch's readers
    template <typename P>
    __device__ __forceinline__ void stage(const P& p, float* s_patch, const float* base) const
    {
        if constexpr (LDS) {
            const int CP = C | 1;
            if (ph * pw * CP > p.patch_cap) __builtin_trap();   // host sizing bug: never silently write past the patch
            const int n = ph * pw * C;
            for (int e = threadIdx.x; e < n; e += nthr) {
                const int pc = e / C, ch = e - pc * C;
                const int r = pc / pw, c = pc - r * pw;
                s_patch[pc * CP + ch] = base[((int64_t)(r_lo + r) * p.w + c_lo + c) * p.ldx + ch];
            }
        }
    }

    template <typename P>
    __device__ __forceinline__ Lerp row(const P& p, int Y) const { return lerp_src(Y, p.h, p.sh, p.align); }

    // this lane's taps on output row Y (lh = row(p, Y)); src: the staged patch (LDS) / the image the patch would be staged from
    __device__ __forceinline__ LowresTaps<Off> taps(const float* src, const Lerp& lh) const
    {
        return LowresTaps<Off>{src + (lh.i0 - r_lo) * row_pitch, src + (lh.i1 - r_lo) * row_pitch, o0, o1, lh.l0, lh.l1, w0, w1};
    }
};

}  // namespace pp
