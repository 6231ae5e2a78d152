// acq_host.h - what crosses between the acquisition sources on the HOST side, and nothing else does:
//   acq.hip         the full-size scorers and the list select      acq_topk.hip   the selection on a score map (pp_topk_select)
//   acq_lowres.hip  the scorers on the classifier-resolution logits acq_mc.hip     the MC-dropout families
//   acq_knobs.hip   the planners' switches (defined there once; every source reads the same object)
// Each function is defined in the source named above its declaration.  (The device side's counterpart is acq_device.h.)
#pragma once
#include <functional>
#include <type_traits>

#include "pp_common.h"
#include "acq_device.h"

namespace pp {

// ---- acq_knobs.hip: the planners' switches ------------------------------------------------------------------------------------
// Written by the test build's pp_debug_set_* only (include/pixelpick_hip_knobs.h); the product keeps the defaults.  ONE object: a
// static or inline copy in this header would give every source its own, and an A/B test would compare a path with itself.
struct AcqKnobs {
    int reduce_mode = 0;
    int exact_formula = 0;    // 1: reference operation order (19 exp + 19 div + 19 log per pixel) as the process default
    int tune_occ = 0;         // tuning knobs (C == 19 flat path only): waves/SIMD bound, pixels per thread
    int tune_ppt = 0;
    int acq_strat_spec = 1;   // strategy-specialised scorers of the three dataset class counts (pp_debug_set_acq_tuning bit 10 of `occ`: off)
    int nt_off = 0;           // A/B: ordinary instead of non-temporal logit loads in the strategy-specialised scorers (bit 11 of `occ`)
    int tune_xcd = 0;         // 0: by plane size, 1: never, 2: always (bits 8-9 of `occ`)
    int large_multiblock = 1; // 0: the one-block-per-image radix select (pp_debug_set_reduce_mode bit 8), for A/B
    int large_q = 1;          // 0: no quantised-histogram select (bit 9), for A/B
    int generic_q = 1;        // 0: generic maps through the radix select (bit 22), for A/B
    int hist_fuse = 1;        // 0: no histogram epilogue in the scorer launches (bit 10), for A/B
    int emit = 1;             // 0: the map-writing scorer + topk_qsel_kernel instead of the list select (bit 11), for A/B
    int emit_mult16 = 40;     // sampled threshold aims at mult16 / 16 x k pixels passing (bits 12-17; 0 = default)
    int sample_locs = 128;    // bits 18-19: 128 / 64 / 256 / 512 locations per image
    int sample_gpl = 4;       // bits 20-21: 4 / 2 / 1 / 8 four-pixel groups per location
    uint32_t* lsel_probe = nullptr;   // pp_debug_set_lsel_probe: one word per image from topk_lsel_kernel (test build's kernel only)
};
extern AcqKnobs g_knobs;

// The reference operation order PER CALL: `strategy | PP_ACQ_REFERENCE_ORDER` at an entry point.  The flag lives in a thread-local for
// the duration of that call (the planners read exact_formula()), so concurrent callers on other threads / streams do not see it.
extern thread_local int t_exact_call;
inline int exact_formula() { return t_exact_call | g_knobs.exact_formula; }
struct ExactScope {
    int keep;
    explicit ExactScope(int& strategy) : keep(t_exact_call)
    {
        if (strategy >= 0 && (strategy & PP_ACQ_REFERENCE_ORDER)) { t_exact_call = 1; strategy &= ~PP_ACQ_REFERENCE_ORDER; }
    }
    ~ExactScope() { t_exact_call = keep; }
};

// f(integral_constant<int, S>) for the strategy-specialised instantiation that serves `strategy` (lowres_by_classes' style)
template <typename F>
inline void by_strategy(int strategy, F&& f)
{
    if (strategy == PP_ACQ_ENTROPY) f(std::integral_constant<int, PP_ACQ_ENTROPY>{});
    else if (strategy == PP_ACQ_LEAST_CONFIDENCE) f(std::integral_constant<int, PP_ACQ_LEAST_CONFIDENCE>{});
    else f(std::integral_constant<int, PP_ACQ_MARGIN>{});
}

// ---- acq.hip ------------------------------------------------------------------------------------------------------------------
struct Plan {
    bool nhwc = false;    // dense channels-last input: LDS-transposed path
    bool vec4;            // flat float4 path
    int ppt;              // pixels per thread
    int blocks_per_image;
    int waves_per_image;
    bool xcd = false;     // XCD-contiguous block order (flat float4 path, class planes >= 4 MB)
};
Plan make_plan(int64_t B, int64_t N, bool vec4, bool force_ppt4 = false);
int validate(const float* logits, int64_t B, int64_t C, int64_t H, int64_t W, int strategy);
bool stream_classes(int64_t C);

// ---- acq_topk.hip -------------------------------------------------------------------------------------------------------------
size_t merge_ws_bytes(int64_t B, int64_t n_cand, int64_t k);
int run_merge(uint64_t* cand, int64_t n_cand, uint64_t* other, int64_t B, int k, int largest, int32_t* out_idx, float* out_val,
              hipStream_t st);
float score_qscale(int strategy, int64_t C);
bool large_q_ok(int64_t B, int64_t k, float qscale);
uint32_t* large_hist(void* ws, int64_t B, int64_t k);
int run_large(const float* map, int64_t B, int64_t N, int64_t k, int largest, void* ws, int32_t* out_idx, float* out_val, hipStream_t st,
              float qscale = 0.0f, bool hist_done = false);
// What every selecting entry checks after its own arguments: k in [1, N] (n_name: how the entry's message calls N), out_idx, and the
// workspace against the entry's own sizer (`need`) and the 256-B alignment
int check_select_args(int64_t k, int64_t N, const char* n_name, const int32_t* out_idx, const void* workspace, size_t ws_bytes, size_t need);
// The small-k workspace: the level-0 candidate lists (`lists` per image, k keys each) and the merge's other buffer (merge_ws_bytes)
struct SmallKLists {
    int64_t n_cand;
    uint64_t *cand, *other;
};
SmallKLists small_k_lists(void* workspace, int64_t B, int64_t lists, int64_t k);

// ---- acq_lowres.hip -----------------------------------------------------------------------------------------------------------
struct LowresPlan {
    int ppt, tiles_x, tiles_y, waves_per_image;
    bool lds;
    size_t lds_bytes;
    int patch_cap;
};
LowresPlan make_lowres_plan(int64_t B, int64_t C, int64_t h, int64_t w, int64_t Hc, int64_t Wc, float sh, float sw, bool force_ppt4);
int validate_lowres(const float* low, int64_t ldx, int64_t B, int64_t C, int64_t h, int64_t w, int64_t H, int64_t W, int64_t Hc, int64_t Wc,
                    int strategy);
// the parameter block of a *_topk entry before planning: scales from (h, w) -> (H, W), no tiles, no candidate lists, no histogram
LowresParams make_lowres_params(const float* low, int64_t ldx, const uint8_t* exclude, float* out_map, int64_t C, int64_t h, int64_t w,
                                int64_t H, int64_t W, int align_corners, int64_t Hc, int64_t Wc, int strategy);
// What the *_at entries share after their own validation: n == 0 (any = false: nothing to do), the list's pointers (`who` names the
// entry in the message), the scales and the one-thread-per-listed-pixel grid
struct LowresAt {
    bool any;
    float sh, sw;
    int align;
    dim3 grid;
};
int lowres_at_begin(const char* who, int64_t h, int64_t w, int64_t H, int64_t W, int align_corners, const int32_t* img_idx,
                    const int32_t* pix_idx, const void* out, int64_t n, LowresAt& at);
int run_lowres_select(LowresParams& p, const LowresPlan& pl, int64_t B, int64_t k, int32_t* out_idx, float* out_val, void* workspace,
                      size_t ws_bytes, hipStream_t st, float qscale, bool hist_ok, const std::function<int()>& launch);

}  // namespace pp
