// vis.hip — the per-epoch picture's byte panels straight from the LOW-resolution classifier output.
//
// Replaces  deeplab.py:55-56          F.interpolate(pred, size=inputs.shape[2:], mode='bilinear', align_corners=True)
//        +  model.py:124,150-156      softmax, argmax, the three _query maps of the first image, margin negated
//        +  utils/utils.py:394-417    Visualiser._preprocess: palette lookup (a per-pixel .item() loop) / min-max normalisation to bytes
// without the full-resolution logits, their softmax or any float map on the host: what leaves the device is one byte per pixel
// and panel.  Resize and PNG encoding stay on the host (utils/utils.py:418-432).
//
// Two launches on the stream:
//   vis_score_kernel   LowresTile (lowres_tile.h): a block owns 64 output columns x (4 waves x ppt rows), stages the
//                      low-resolution patch in LDS, every lane interpolates its pixels' class vectors from the tile's taps.
//                      argmax (first maximum: pp_predict_lowres's bits) -> prediction panel; label -> target panel;
//                      pixel_score_fast (acq_score.h: pp_acq_lowres_score_topk's bits) x 3 -> fp32 scores in the workspace; the
//                      block's min / max of the three scores and of its input pixels -> its own row of a slab in the workspace
//                      (no atomics, nothing to initialise, reproducible).
//   vis_quant_kernel   elementwise: every block first reduces its image's slab (one row per tile: a few hundred), then turns
//                      scores and input into bytes:  t = v - min ; d = max(t) + 1e-7 ; byte = trunc(clamp(t / d * 255, 0, 255)),
//                      every operation rounded on its own in fp32, as torch does on the CPU.
#include "pp_common.h"
#include "acq_score.h"
#include "lowres_tile.h"

#include <algorithm>
#include <cmath>

namespace pp {

constexpr int kVisBlock = 256;
constexpr int kVisWaves = kVisBlock / kWave;
constexpr int kVisQuantPix = 4;                    // pixels per thread of vis_quant_kernel
constexpr size_t kVisLdsMax = 48 * 1024;           // patch per block (+ 0.9 KB static)
constexpr size_t kVisLdsSoft = 32 * 1024;          // above this the 32-row tile gives way to the 16-row tile

struct VisParams {
    const float* low;         // [B,h,w,ldx] channels-last, C valid channels
    int64_t ldx;
    const float* image;       // [B,3,Hc,Wc] with strides isn / isc / isr (columns dense), or null
    int64_t isn, isc, isr;
    const void* target;       // [B,Hc,Wc] u8 (kind 1) / i64 (kind 2), or null
    const uint8_t* palette;   // [256][3]
    uint8_t* rgb;             // [B][n_rgb][Hc][Wc][3]
    uint8_t* gray;            // [B][3][Hc][Wc]
    float* ranges;            // [B][4][2] or null
    float* scores;            // workspace: [B][3][Hc*Wc]  confidence, margin (negated), entropy
    float* slab;              // workspace: [B][tiles][8]  (min, max) of input, confidence, margin, entropy per tile
    int h, w, Hc, Wc;
    float sh, sw;
    int align, target_kind;
    int C, tiles_x, tiles_y, ppt;
    int patch_cap;            // floats of dynamic LDS available for the patch
    int n_rgb, panel_target, panel_pred;
    int quant_blocks;         // vis_quant_kernel: blocks per image
};

__device__ __forceinline__ void vis_put_rgb(uint8_t* dst, const uint8_t* pal, int idx)
{
    dst[0] = pal[idx * 3 + 0];
    dst[1] = pal[idx * 3 + 1];
    dst[2] = pal[idx * 3 + 2];
}

// fminf / fmaxf return the other operand when one is NaN: NaN scores (entropy's 0 * log 0) drop out of the range.
__device__ __forceinline__ void vis_range(float v, float& mn, float& mx) { mn = fminf(mn, v); mx = fmaxf(mx, v); }

template <int CMAX, bool EXACT, bool LDS>
__global__ __launch_bounds__(kVisBlock, 2) void vis_score_kernel(VisParams p)
{
    extern __shared__ __attribute__((aligned(16))) float s_patch[];
    __shared__ uint8_t s_pal[768];
    __shared__ float s_red[kVisWaves][8];
    const int tiles = p.tiles_x * p.tiles_y;
    const int img = blockIdx.x / tiles;
    const int t = blockIdx.x - img * tiles;
    const int ty = t / p.tiles_x, tx = t - ty * p.tiles_x;
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int C = EXACT ? CMAX : p.C;
    const int64_t N = (int64_t)p.Hc * p.Wc;
    LowresTile<LDS> tile(p, C, tx, ty, kVisWaves * p.ppt, kVisBlock);
    const float* base = p.low + (int64_t)img * p.h * p.w * p.ldx;
    for (int i = tid; i < 768; i += kVisBlock) s_pal[i] = p.palette[i];
    tile.stage(p, s_patch, base);
    __syncthreads();
    tile.set_lane(p, lane);
    const int X = tile.X;
    const float* src = LDS ? s_patch : base;
    // the template arguments pp_acq_lowres_score_topk's launch takes for this C: strategy-specialised where the class count is
    // one of the datasets' and the patch is in LDS, the run-time strategy otherwise
    constexpr bool kSpec = EXACT && LDS;

    float mn[4], mx[4];                       // input, confidence, margin, entropy
#pragma unroll
    for (int q = 0; q < 4; ++q) { mn[q] = INFINITY; mx[q] = -INFINITY; }
#pragma unroll 1
    for (int j = 0; j < p.ppt; ++j) {
        const int Y = tile.Y0 + wv * p.ppt + j;
        if (Y < p.Hc && tile.xin) {
            float x[CMAX];
            const auto tp = tile.taps(src, tile.row(p, Y));
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                if (EXACT || c < C) x[c] = tp.at(c);
            float m = x[0];
            int am = 0;
#pragma unroll
            for (int c = 1; c < CMAX; ++c)
                if (EXACT || c < C)
                    if (x[c] > m) { m = x[c]; am = c; }             // first maximum, as predict_lowres_kernel / torch.argmax on the CPU
            float lc, mg, en;
            if constexpr (kSpec) {
                lc = pixel_score_fast<CMAX, EXACT, PP_ACQ_LEAST_CONFIDENCE>(x, C, PP_ACQ_LEAST_CONFIDENCE);
                mg = pixel_score_fast<CMAX, EXACT, PP_ACQ_MARGIN>(x, C, PP_ACQ_MARGIN);
                en = pixel_score_fast<CMAX, EXACT, PP_ACQ_ENTROPY>(x, C, PP_ACQ_ENTROPY);
            } else {
                lc = pixel_score_fast<CMAX, EXACT>(x, C, PP_ACQ_LEAST_CONFIDENCE);
                mg = pixel_score_fast<CMAX, EXACT>(x, C, PP_ACQ_MARGIN);
                en = pixel_score_fast<CMAX, EXACT>(x, C, PP_ACQ_ENTROPY);
            }
            mg = -mg;                                               // model.py:155: smaller margins are drawn brighter
            const int64_t pix = (int64_t)Y * p.Wc + X;
            float* sc = p.scores + (int64_t)img * 3 * N + pix;
            sc[0] = lc; sc[N] = mg; sc[2 * N] = en;
            vis_range(lc, mn[1], mx[1]);
            vis_range(mg, mn[2], mx[2]);
            vis_range(en, mn[3], mx[3]);
            uint8_t* panels = p.rgb + (int64_t)img * p.n_rgb * N * 3;
            vis_put_rgb(panels + ((int64_t)p.panel_pred * N + pix) * 3, s_pal, am);
            if (p.target) {
                const int64_t tv = p.target_kind == 1 ? (int64_t) reinterpret_cast<const uint8_t*>(p.target)[(int64_t)img * N + pix]
                                                      : reinterpret_cast<const int64_t*>(p.target)[(int64_t)img * N + pix];
                uint8_t* d = panels + ((int64_t)p.panel_target * N + pix) * 3;
                if (tv >= 0 && tv <= 255) vis_put_rgb(d, s_pal, (int)tv);
                else { d[0] = 0; d[1] = 0; d[2] = 0; }
            }
            if (p.image) {
                const float* ip = p.image + (int64_t)img * p.isn + (int64_t)Y * p.isr + X;
#pragma unroll
                for (int c = 0; c < 3; ++c) vis_range(ip[(int64_t)c * p.isc], mn[0], mx[0]);
            }
        }
    }
    // block's ranges -> its slab row (lanes outside the crop hold the identities)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mn[q] = fminf(mn[q], __shfl_xor(mn[q], o, 64));
            mx[q] = fmaxf(mx[q], __shfl_xor(mx[q], o, 64));
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) { s_red[wv][2 * q] = mn[q]; s_red[wv][2 * q + 1] = mx[q]; }
    }
    __syncthreads();
    if (tid < 8) {
        float a = s_red[0][tid];
        for (int k = 1; k < kVisWaves; ++k) a = (tid & 1) ? fmaxf(a, s_red[k][tid]) : fminf(a, s_red[k][tid]);
        p.slab[((int64_t)img * tiles + t) * 8 + tid] = a;
    }
}

// utils/utils.py:410-412,417: every operation rounded on its own (no contraction, true division); NaN -> 0
__device__ __forceinline__ uint8_t vis_quant(float v, float mn, float d)
{
#pragma clang fp contract(off)
    const float t = __fsub_rn(v, mn);
    const float q = __fmul_rn(__fdiv_rn(t, d), 255.0f);
    return (uint8_t)(int)fminf(fmaxf(q, 0.0f), 255.0f);
}

__global__ __launch_bounds__(kVisBlock) void vis_quant_kernel(VisParams p)
{
    __shared__ float s_r[kVisBlock / 8][8];
    const int tiles = p.tiles_x * p.tiles_y;
    const int img = blockIdx.x / p.quant_blocks;
    const int chunk = blockIdx.x - img * p.quant_blocks;
    const int tid = threadIdx.x, comp = tid & 7, part = tid >> 3;
    const int64_t N = (int64_t)p.Hc * p.Wc;
    const bool is_max = comp & 1;
    float a = is_max ? -INFINITY : INFINITY;
    for (int e = part; e < tiles; e += kVisBlock / 8) {
        const float v = p.slab[((int64_t)img * tiles + e) * 8 + comp];
        a = is_max ? fmaxf(a, v) : fminf(a, v);
    }
    s_r[part][comp] = a;
    __syncthreads();
    for (int off = kVisBlock / 16; off > 0; off >>= 1) {
        if (part < off) s_r[part][comp] = is_max ? fmaxf(s_r[part][comp], s_r[part + off][comp]) : fminf(s_r[part][comp], s_r[part + off][comp]);
        __syncthreads();
    }
    float mn[4], d[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        mn[q] = s_r[0][2 * q];
        d[q] = __fadd_rn(__fsub_rn(s_r[0][2 * q + 1], mn[q]), 1e-7f);     // max(v - min) = max(v) - min: rounding is monotone
    }
    if (p.ranges && chunk == 0 && tid < 8) p.ranges[(int64_t)img * 8 + tid] = (!p.image && tid < 2) ? 0.0f : s_r[0][tid];
    const float* sc = p.scores + (int64_t)img * 3 * N;
    uint8_t* g = p.gray + (int64_t)img * 3 * N;
    uint8_t* in_panel = p.rgb + (int64_t)img * p.n_rgb * N * 3;           // the input is panel 0 when there is one
#pragma unroll
    for (int j = 0; j < kVisQuantPix; ++j) {
        const int64_t e = ((int64_t)chunk * kVisQuantPix + j) * kVisBlock + tid;
        if (e >= N) break;
#pragma unroll
        for (int s = 0; s < 3; ++s) g[s * N + e] = vis_quant(sc[s * N + e], mn[s + 1], d[s + 1]);
        if (p.image) {
            const int y = (int)(e / p.Wc), x = (int)(e - (int64_t)y * p.Wc);
            const float* ip = p.image + (int64_t)img * p.isn + (int64_t)y * p.isr + x;
#pragma unroll
            for (int c = 0; c < 3; ++c) in_panel[e * 3 + c] = vis_quant(ip[(int64_t)c * p.isc], mn[0], d[0]);   // HWC
        }
    }
}

// slab rows of the smallest tile (16 rows): an upper bound of what any plan writes
static int64_t vis_tiles_max(int64_t Hc, int64_t Wc) { return cdiv(Wc, kWave) * cdiv(Hc, kVisWaves * 4); }

static bool vis_size_ok(int64_t B, int64_t Hc, int64_t Wc)
{
    const int64_t i31 = 0x7FFFFFFFll;
    if (B < 1 || Hc < 1 || Wc < 1 || Hc > i31 || Wc > i31 || Hc * Wc > i31) return false;
    if (B > i31 * 1024 / (Hc * Wc)) return false;
    return B * vis_tiles_max(Hc, Wc) <= i31 && B * cdiv(Hc * Wc, kVisBlock * kVisQuantPix) <= i31;
}

static size_t vis_scores_bytes(int64_t B, int64_t Hc, int64_t Wc) { return align_up((size_t)(B * 3 * Hc * Wc) * 4, 256); }

template <int CMAX, bool EXACT>
static void launch_vis_score(const VisParams& p, bool lds, size_t lds_bytes, dim3 grid, hipStream_t st)
{
    if (lds) hipLaunchKernelGGL((vis_score_kernel<CMAX, EXACT, true>), grid, dim3(kVisBlock), lds_bytes, st, p);
    else     hipLaunchKernelGGL((vis_score_kernel<CMAX, EXACT, false>), grid, dim3(kVisBlock), 0, st, p);
}

}  // namespace pp

using namespace pp;

extern "C" {

size_t pp_vis_lowres_workspace_bytes(int64_t B, int64_t Hc, int64_t Wc)
{
    if (!vis_size_ok(B, Hc, Wc)) return 0;
    return vis_scores_bytes(B, Hc, Wc) + (size_t)(B * vis_tiles_max(Hc, Wc)) * 8 * sizeof(float);
}

int pp_vis_lowres(const float* low, int64_t ldx, int64_t B, int64_t C, int64_t h, int64_t w, int64_t H, int64_t W,
                  int align_corners, int64_t Hc, int64_t Wc, const float* image, int64_t image_sn, int64_t image_sc,
                  int64_t image_sr, const void* target, int target_kind, const uint8_t* palette, uint8_t* rgb, uint8_t* gray,
                  float* ranges, void* workspace, size_t ws_bytes, pp_stream_t stream)
{
    if (!low) return fail(PP_ERR_BAD_ARG, "vis_lowres: low is null");
    if (!palette || !rgb || !gray) return fail(PP_ERR_BAD_ARG, "vis_lowres: palette, rgb or gray is null");
    if (B < 1 || C < 1 || h < 1 || w < 1 || H < 1 || W < 1 || Hc < 1 || Wc < 1)
        return fail(PP_ERR_BAD_ARG, "vis_lowres: bad shape B=%lld C=%lld %lldx%lld -> %lldx%lld crop %lldx%lld", (long long)B,
                    (long long)C, (long long)h, (long long)w, (long long)H, (long long)W, (long long)Hc, (long long)Wc);
    if (Hc > H || Wc > W) return fail(PP_ERR_BAD_ARG, "vis_lowres: crop %lldx%lld exceeds the interpolated size %lldx%lld",
                                      (long long)Hc, (long long)Wc, (long long)H, (long long)W);
    if (ldx < C) return fail(PP_ERR_BAD_ARG, "vis_lowres: ldx=%lld < C=%lld", (long long)ldx, (long long)C);
    if (target_kind < 0 || target_kind > 2) return fail(PP_ERR_BAD_ARG, "vis_lowres: unknown target_kind %d", target_kind);
    if ((target_kind != 0) != (target != nullptr))
        return fail(PP_ERR_BAD_ARG, "vis_lowres: target_kind %d with a %s target", target_kind, target ? "non-null" : "null");
    if (image && (image_sr < Wc || image_sc < 0 || image_sn < 0))
        return fail(PP_ERR_BAD_ARG, "vis_lowres: image strides n=%lld c=%lld row=%lld (rows of %lld dense columns)", (long long)image_sn,
                    (long long)image_sc, (long long)image_sr, (long long)Wc);
    if (C > PP_ACQ_MAX_CLASSES)
        return fail(PP_ERR_UNSUPPORTED, "vis_lowres: C=%lld (the scorer holds up to %d classes)", (long long)C, PP_ACQ_MAX_CLASSES);
    const int64_t i31 = 0x7FFFFFFFll;
    if (H > i31 || W > i31 || h > i31 || w > i31 || H * W > i31 || h * w > i31 || !vis_size_ok(B, Hc, Wc))
        return fail(PP_ERR_UNSUPPORTED, "vis_lowres: image too large");
    if (ldx > i31 || B > 0x7FFFFFFFFFFFll / (h * w * ldx)) return fail(PP_ERR_UNSUPPORTED, "vis_lowres: low-res tensor too large");
    const size_t need = pp_vis_lowres_workspace_bytes(B, Hc, Wc);
    if (!workspace || ws_bytes < need)
        return fail(PP_ERR_WORKSPACE, "vis_lowres: workspace of %zu bytes, %zu needed", workspace ? ws_bytes : (size_t)0, need);

    VisParams p;
    p.low = low; p.ldx = ldx;
    p.image = image; p.isn = image_sn; p.isc = image_sc; p.isr = image_sr;
    p.target = target; p.target_kind = target_kind; p.palette = palette;
    p.rgb = rgb; p.gray = gray; p.ranges = ranges;
    p.scores = reinterpret_cast<float*>(workspace);
    p.slab = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + vis_scores_bytes(B, Hc, Wc));
    p.h = (int)h; p.w = (int)w; p.Hc = (int)Hc; p.Wc = (int)Wc;
    lowres_scales(h, w, H, W, align_corners, p.sh, p.sw);
    p.align = align_corners ? 1 : 0; p.C = (int)C;
    p.panel_target = image ? 1 : 0;
    p.panel_pred = p.panel_target + (target ? 1 : 0);
    p.n_rgb = p.panel_pred + 1;

    auto patch_floats = [&](int ppt) { return lowres_patch_floats(p.sh, p.sw, h, w, kVisWaves * ppt, C); };
    p.tiles_x = (int)cdiv(Wc, kWave);
    const int64_t tiles8 = p.tiles_x * cdiv(Hc, kVisWaves * 8);
    p.ppt = (B * tiles8 >= 256 && (size_t)patch_floats(8) * 4 <= kVisLdsSoft) ? 8 : 4;
    p.tiles_y = (int)cdiv(Hc, kVisWaves * p.ppt);
    const int64_t fl = patch_floats(p.ppt);
    const bool lds = (size_t)fl * 4 <= kVisLdsMax;       // otherwise every lane reads its four neighbours from memory
    p.patch_cap = lds ? (int)fl : 0;
    const size_t lds_bytes = lds ? (size_t)fl * 4 : 0;
    p.quant_blocks = (int)cdiv(Hc * Wc, kVisBlock * kVisQuantPix);

    hipStream_t st = as_stream(stream);
    const dim3 grid((unsigned)(B * p.tiles_x * p.tiles_y));
    lowres_by_classes(C, [&](auto cmax, auto exact) {
        launch_vis_score<decltype(cmax)::value, decltype(exact)::value>(p, lds, lds_bytes, grid, st);
        return 0;
    });
    if (int rc = check_launch("vis_score_kernel")) return rc;
    hipLaunchKernelGGL(vis_quant_kernel, dim3((unsigned)(B * p.quant_blocks)), dim3(kVisBlock), 0, st, p);
    return check_launch("vis_quant_kernel");
}

}  // extern "C"
