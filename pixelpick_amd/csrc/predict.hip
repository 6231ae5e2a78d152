// predict.hip — the label map and the confusion matrix straight from the LOW-resolution classifier output.
//
// Replaces  deeplab.py:55-56          F.interpolate(pred, size=inputs.shape[2:], mode='bilinear', align_corners=True)
//        +  model.py:124-125,196-199  prob.argmax(dim=1); running_score.update(y, pred)      (eval.py:60-63 in evaluate())
//        +  utils/metrics.py:168-177  RunningScore._fast_hist
// without writing the [B,C,H,W] logits: at 256x512x19 that tensor is 10 MB written and read back per image to be reduced to one
// byte per pixel; the inputs needed are 0.62 MB of 64x128x19 logits and the labels.
//
// Geometry is LowresTile's (lowres_tile.h): a block owns 64 output columns x (4 waves x ppt rows), stages the low-resolution
// patch the tile interpolates from in LDS, and every lane interpolates its pixels from the tile's taps - the bits
// pp_bilinear_fwd writes.  Unlike the scorer, argmax needs only a running maximum: the classes are a run-time loop, no
// class vector lives in registers and there is no per-C instantiation.  Blocks walk the tiles with a grid stride so that the
// block-private C x C histogram is flushed (64-bit integer atomics, non-zero cells only) by at most kPredMaxBlocks blocks.
#include "pp_common.h"
#include "lowres_tile.h"

#include <algorithm>
#include <cmath>

namespace pp {

constexpr int kPredBlock = 256;
constexpr int kPredWaves = kPredBlock / kWave;
constexpr int kPredMaxBlocks = 2048;
constexpr int kPredAggRounds = 4;                   // wave-aggregated histogram adds before the plain LDS atomics
constexpr size_t kPredLdsMax = 48 * 1024;           // histogram + patch per block: three blocks per CU at the worst
constexpr size_t kPredLdsSoft = 32 * 1024;          // above this the 32-row tile gives way to the 16-row tile

struct PredictParams {
    const float* low;         // [B,h,w,ldx] channels-last, C valid channels
    int64_t ldx;
    const void* target;       // [B,Hc,Wc] u8 (kind 1) / i64 (kind 2), or null
    uint8_t* pred;            // [B,Hc,Wc] or null
    unsigned long long* hist; // [C,C] accumulated into, or null
    int64_t total_tiles;      // B * tiles_x * tiles_y
    int h, w, Hc, Wc;
    float sh, sw;
    int align, target_kind;
    int C, tiles_x, tiles_y, ppt;
    int patch_cap;            // floats of dynamic LDS available for the patch
};

// hist[cell] += 1 for every lane with `pending`, one LDS add per distinct cell of the wave while the cells repeat (neighbouring
// pixels mostly share label and prediction): the first pending lane's cell is broadcast, the lanes that share it are counted with
// a ballot and one lane adds the count.  Called by all 64 lanes (uniform control flow).
__device__ __forceinline__ void wave_hist_add(uint32_t* s_hist, int cell, bool pending, int lane)
{
#pragma unroll 1
    for (int r = 0; r < kPredAggRounds; ++r) {
        const unsigned long long act = __ballot(pending);
        if (!act) return;
        const int leader = __ffsll(act) - 1;
        const int lead = __builtin_amdgcn_readlane(cell, leader);
        const bool same = pending && cell == lead;
        const unsigned long long grp = __ballot(same);
        if (lane == leader) atomicAdd(&s_hist[lead], (uint32_t)__popcll(grp));
        pending = pending && !same;
    }
    if (pending) atomicAdd(&s_hist[cell], 1u);
}

// G consecutive output rows Y .. Y+G-1 that interpolate from ONE pair of source rows (at x4 nearly every group of four does): per
// class the two horizontal lerps are taken once and only the vertical one is per row, and the four LDS reads are shared -
// the same operations in the same order as bilerp(), so the same bits.  Lanes right of the crop compute on the clamped last
// column (valid addresses) and write nothing, so the wave stays converged for the ballots of wave_hist_add.
template <int G, bool HIST>
__device__ __forceinline__ void predict_rows(const PredictParams& p, const float* p00, const float* p01, const float* p10,
                                             const float* p11, float w0, float w1, int Y, int X, bool xin, int64_t img_pix,
                                             uint32_t* s_hist, int lane)
{
    const int C = p.C;
    float h0[G], h1[G], m[G];
    int am[G];
    const float top0 = lerp2(w0, w1, p00[0], p01[0]), bot0 = lerp2(w0, w1, p10[0], p11[0]);
#pragma unroll
    for (int r = 0; r < G; ++r) {
        const Lerp lh = lerp_src(Y + r, p.h, p.sh, p.align);
        h0[r] = lh.l0; h1[r] = lh.l1;
        m[r] = lerp2(h0[r], h1[r], top0, bot0);
        am[r] = 0;
    }
#pragma unroll 2
    for (int c = 1; c < C; ++c) {
        const float top = lerp2(w0, w1, p00[c], p01[c]), bot = lerp2(w0, w1, p10[c], p11[c]);
#pragma unroll
        for (int r = 0; r < G; ++r) {
            const float v = lerp2(h0[r], h1[r], top, bot);
            if (v > m[r]) { m[r] = v; am[r] = c; }              // first maximum, as confusion_kernel / torch.argmax on the CPU
        }
    }
#pragma unroll
    for (int r = 0; r < G; ++r) {
        const int64_t pix = img_pix + (int64_t)(Y + r) * p.Wc + X;
        if (xin && p.pred) p.pred[pix] = (uint8_t)am[r];
        if constexpr (HIST) {
            int64_t tv = -1;
            if (xin)
                tv = p.target_kind == 1 ? (int64_t) reinterpret_cast<const uint8_t*>(p.target)[pix]
                                        : reinterpret_cast<const int64_t*>(p.target)[pix];
            const bool valid = tv >= 0 && tv < C;               // utils/metrics.py:169 mask
            wave_hist_add(s_hist, valid ? (int)tv * C + am[r] : 0, valid, lane);
        }
    }
}

template <bool LDS, bool HIST>
__global__ __launch_bounds__(kPredBlock) void predict_lowres_kernel(PredictParams p)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_mem[];
    const int C = p.C;
    uint32_t* s_hist = s_mem;                                                   // C*C block-private counters (HIST)
    float* s_patch = reinterpret_cast<float*>(s_mem + (HIST ? C * C : 0));
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    if constexpr (HIST) {
        for (int i = tid; i < C * C; i += kPredBlock) s_hist[i] = 0u;
        __syncthreads();
    }
    const int TR = kPredWaves * p.ppt;
    const int tiles = p.tiles_x * p.tiles_y;
    const int64_t N = (int64_t)p.Hc * p.Wc;

    for (int64_t blk = blockIdx.x; blk < p.total_tiles; blk += gridDim.x) {
        const int64_t img = blk / tiles;
        const int t = (int)(blk - img * tiles);
        const int ty = t / p.tiles_x, tx = t - ty * p.tiles_x;
        LowresTile<LDS> tile(p, C, tx, ty, TR, kPredBlock);
        const float* base = p.low + img * p.h * p.w * p.ldx;
        if constexpr (LDS) {
            if (blk != blockIdx.x) __syncthreads();             // the previous tile's readers are done with the patch
            tile.stage(p, s_patch, base);
            __syncthreads();
        }
        tile.set_lane(p, lane);
        const float* src = LDS ? s_patch : base;
        const int Yw = tile.Y0 + wv * p.ppt;                         // the wave's rows: Yw .. Yw + nrows - 1 (wave-uniform)
        const int nrows = min(p.ppt, p.Hc - Yw);
#pragma unroll 1
        for (int j = 0; j < nrows;) {
            const int Y = Yw + j;
            const Lerp lh = tile.row(p, Y);
            int g = 1;                                           // rows from Y on that share lh's source rows (i1 follows from i0)
            while (g < 4 && j + g < nrows && tile.row(p, Y + g).i0 == lh.i0) ++g;
            const auto tp = tile.taps(src, lh);
            if (g == 4) {
                predict_rows<4, HIST>(p, tp.r0 + tp.o0, tp.r0 + tp.o1, tp.r1 + tp.o0, tp.r1 + tp.o1, tp.w0, tp.w1, Y, tile.X, tile.xin, img * N, s_hist, lane);
                j += 4;
            } else if (g >= 2) {
                predict_rows<2, HIST>(p, tp.r0 + tp.o0, tp.r0 + tp.o1, tp.r1 + tp.o0, tp.r1 + tp.o1, tp.w0, tp.w1, Y, tile.X, tile.xin, img * N, s_hist, lane);
                j += 2;
            } else {
                predict_rows<1, HIST>(p, tp.r0 + tp.o0, tp.r0 + tp.o1, tp.r1 + tp.o0, tp.r1 + tp.o1, tp.w0, tp.w1, Y, tile.X, tile.xin, img * N, s_hist, lane);
                j += 1;
            }
        }
    }
    if constexpr (HIST) {
        __syncthreads();
        for (int i = tid; i < C * C; i += kPredBlock) {
            const uint32_t n = s_hist[i];
            if (n) atomicAdd(&p.hist[i], (unsigned long long)n);
        }
    }
}

}  // namespace pp

using namespace pp;

extern "C" {

int pp_predict_lowres(const float* low, int64_t ldx, int64_t B, int64_t C, int64_t h, int64_t w, int64_t H, int64_t W,
                      int align_corners, int64_t Hc, int64_t Wc, const void* target, int target_kind, uint8_t* pred,
                      int64_t* hist, pp_stream_t stream)
{
    if (!low) return fail(PP_ERR_BAD_ARG, "predict_lowres: low is null");
    if (!pred && !hist) return fail(PP_ERR_BAD_ARG, "predict_lowres: neither pred nor hist is given");
    if (B < 1 || C < 1 || h < 1 || w < 1 || H < 1 || W < 1 || Hc < 1 || Wc < 1)
        return fail(PP_ERR_BAD_ARG, "predict_lowres: bad shape B=%lld C=%lld %lldx%lld -> %lldx%lld crop %lldx%lld", (long long)B,
                    (long long)C, (long long)h, (long long)w, (long long)H, (long long)W, (long long)Hc, (long long)Wc);
    if (Hc > H || Wc > W) return fail(PP_ERR_BAD_ARG, "predict_lowres: crop %lldx%lld exceeds the interpolated size %lldx%lld",
                                      (long long)Hc, (long long)Wc, (long long)H, (long long)W);
    if (ldx < C) return fail(PP_ERR_BAD_ARG, "predict_lowres: ldx=%lld < C=%lld", (long long)ldx, (long long)C);
    if (target_kind < 0 || target_kind > 2) return fail(PP_ERR_BAD_ARG, "predict_lowres: unknown target_kind %d", target_kind);
    if ((target_kind != 0) != (target != nullptr))
        return fail(PP_ERR_BAD_ARG, "predict_lowres: target_kind %d with a %s target", target_kind, target ? "non-null" : "null");
    if (hist && !target) return fail(PP_ERR_BAD_ARG, "predict_lowres: hist needs a target");
    if (C > 0x7FFFFFFFll) return fail(PP_ERR_UNSUPPORTED, "predict_lowres: C=%lld", (long long)C);
    if (hist && C > 104) return fail(PP_ERR_UNSUPPORTED, "predict_lowres: C=%lld (LDS histogram holds up to 104 classes)", (long long)C);
    if (pred && C > 256) return fail(PP_ERR_UNSUPPORTED, "predict_lowres: C=%lld (pred is one byte per pixel: up to 256 classes)", (long long)C);
    const int64_t i31 = 0x7FFFFFFFll;
    if (H > i31 || W > i31 || h > i31 || w > i31 || H * W > i31 || h * w > i31 || B > i31 * 1024 / (Hc * Wc))
        return fail(PP_ERR_UNSUPPORTED, "predict_lowres: image too large");
    if (ldx > i31 || B > 0x7FFFFFFFFFFFll / (h * w * ldx)) return fail(PP_ERR_UNSUPPORTED, "predict_lowres: low-res tensor too large");

    PredictParams p;
    p.low = low; p.ldx = ldx; p.target = hist ? target : nullptr; p.pred = pred;
    p.hist = reinterpret_cast<unsigned long long*>(hist);
    p.h = (int)h; p.w = (int)w; p.Hc = (int)Hc; p.Wc = (int)Wc;
    lowres_scales(h, w, H, W, align_corners, p.sh, p.sw);
    p.align = align_corners ? 1 : 0; p.target_kind = target_kind; p.C = (int)C;

    const size_t hist_bytes = hist ? (size_t)(C * C) * 4 : 0;
    auto patch_floats = [&](int ppt) { return lowres_patch_floats(p.sh, p.sw, h, w, kPredWaves * ppt, C); };
    p.tiles_x = (int)cdiv(Wc, kWave);
    const int64_t tiles8 = p.tiles_x * cdiv(Hc, kPredWaves * 8);
    p.ppt = (B * tiles8 >= 256 && hist_bytes + (size_t)patch_floats(8) * 4 <= kPredLdsSoft) ? 8 : 4;
    p.tiles_y = (int)cdiv(Hc, kPredWaves * p.ppt);
    p.total_tiles = B * p.tiles_x * p.tiles_y;
    const int64_t fl = patch_floats(p.ppt);
    // the patch pays only where source pixels are shared between output pixels; when it does not fit beside the histogram
    // (strong down-sampling, the largest class counts) every lane reads its four neighbours from memory
    const bool lds = hist_bytes + (size_t)fl * 4 <= kPredLdsMax;
    p.patch_cap = lds ? (int)fl : 0;
    const size_t lds_bytes = hist_bytes + (lds ? (size_t)fl * 4 : 0);

    hipStream_t st = as_stream(stream);
    dim3 grid((unsigned)std::min<int64_t>(p.total_tiles, kPredMaxBlocks)), block(kPredBlock);
    if (hist) {
        if (lds) hipLaunchKernelGGL((predict_lowres_kernel<true, true>), grid, block, lds_bytes, st, p);
        else     hipLaunchKernelGGL((predict_lowres_kernel<false, true>), grid, block, lds_bytes, st, p);
    } else {
        if (lds) hipLaunchKernelGGL((predict_lowres_kernel<true, false>), grid, block, lds_bytes, st, p);
        else     hipLaunchKernelGGL((predict_lowres_kernel<false, false>), grid, block, lds_bytes, st, p);
    }
    return check_launch("predict_lowres_kernel");
}

}  // extern "C"
