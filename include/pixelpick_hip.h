/*
 * pixelpick_hip.h — C ABI of libpixelpick_hip.so (MI355X / gfx950 native hot path of PixelPick).
 *
 * The reference (NoelShin/PixelPick) has no FFI layer: its hot path is reached through the Python
 * call surface of query.py and networks/.  This header is the boundary a drop-in replacement binds
 * instead (ctypes stub in INTEGRATION.md).  Every entry point cites the reference lines it replaces
 * (paths relative to the reference repo root).
 *
 * Conventions
 *   - plain pointers + sizes; no torch types.  All pointers are DEVICE pointers unless stated.
 *   - the caller owns every buffer including the workspace; the library never allocates, frees or
 *     synchronises the device (all work is enqueued on `stream`, graph-capturable).
 *   - return 0 = ok, negative = error (PP_ERR_*); message via pp_last_error() (thread local).
 *   - outputs are fully overwritten.
 */
#ifndef PIXELPICK_HIP_H
#define PIXELPICK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* pp_stream_t; /* hipStream_t */

enum {
    PP_OK = 0,
    PP_ERR_BAD_ARG = -1,      /* null pointer, bad shape/stride, unknown enum */
    PP_ERR_BAD_K = -2,        /* k < 1 or k > H*W */
    PP_ERR_WORKSPACE = -3,    /* workspace too small */
    PP_ERR_UNSUPPORTED = -4,  /* shape outside the supported range (e.g. an image of 2^31 pixels or more) */
    PP_ERR_LAUNCH = -5        /* hipLaunch failure (message holds hipGetErrorString) */
};

/* query.py:229-239 UncertaintySampler strategies.  (`random`, query.py:242-244, is host RNG.) */
enum { PP_ACQ_ENTROPY = 0, PP_ACQ_LEAST_CONFIDENCE = 1, PP_ACQ_MARGIN = 2 };
/* Mutual information between the prediction and the dropout mask (BALD).  Valid ONLY at pp_acq_mean_prob_score_map and
 * pp_acq_lowres_mc_mean_topk (below); every other entry keeps rejecting it as an unknown strategy. */
enum { PP_ACQ_BALD = 3 };
/* OR-ed into `strategy` at any acquisition entry point: score in the reference's OPERATION ORDER - p_c = exp(x_c - m) / S, then
 * sum(-p_c log p_c) with libm-accurate exp / log, each product and sum rounded separately (query.py:190,230) - instead of the default
 * algebraic form (entropy = log S + sum e_c (m - x_c) / S, v_exp_f32 exponentials; identical NaN behaviour).  Both forms are held to the
 * oracle's picks at full size; the reference-order form runs at about half the rate (0.40 of HBM).  Per call, no process state. */
#define PP_ACQ_REFERENCE_ORDER 0x100

/* Class counts up to this are scored from registers (one read of the logits); wider heads take the streamed scorers (acq_stream_kernel:
 * the class vector is read two or three times, the later passes from L2) - the reference softmaxes whatever width the model emits
 * (query.py:190), so no class count is rejected. */
#define PP_ACQ_MAX_CLASSES 64

int pp_version(void);
const char* pp_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * Acquisition: query.py:190-204 + query.py:33-69 for a batch of B images in ONE pass over logits.
 *
 *   logits   f32, element (b,c,h,w) at logits[b*sB + c*sC + h*sH + w*sW] (NCHW or NHWC strides);
 *            replaces F.softmax(model(x)["pred"][:, :, :h, :w], dim=1)               query.py:190
 *   strategy PP_ACQ_*; score = UncertaintySampler(prob)                               query.py:192,229-239
 *   exclude  u8 [B,H,W] or NULL; non-zero = already queried or void; such pixels get score
 *            0.0 (entropy, least-confidence) or 1.0 (margin)                          query.py:195-201
 *   k        pixels returned per image: uc_map.flatten().topk(k, largest = strategy in
 *            {entropy, least_confidence}).indices                                     query.py:36,57-61
 *   out_idx  i32 [B,k] flat index h*W+w, value-sorted; ties -> lower index first; NaN scores
 *            (0*log 0, query.py:230) sort first for largest, last for smallest.
 *   out_val  f32 [B,k] or NULL — the scores of out_idx.
 *   out_map  f32 [B,H,W] or NULL — the score map after exclusion (what query.py calls uc_map).  With k > 48 and no out_map the
 *   map is never formed (flat fp32 class planes, C = 11 / 19 / 21, k <= H*W / 8, H*W >= 16384): a sampled per-image threshold, the
 *   scorer writes only the candidates beyond it, a list select picks from them; images the sample misleads are redone exactly.
 *   k larger than the number of un-excluded pixels is NOT an error (as in the reference, excluded
 *   pixels are then returned, lowest index first).
 *   (SURVEY.md 8(b)'s sketch carries a `sorted` flag after k.  It is deliberately absent: the reference's torch.topk runs with its
 *   default sorted=True and its callers rely on that order (query.py:50-54 takes the first n of the value-sorted candidates), and the
 *   rank-merge that joins the per-block candidate lists yields the value-sorted order as a by-product - an unsorted mode would
 *   neither match a reference call nor save a launch.)
 */
size_t pp_acq_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W, int64_t k);

int pp_acq_score_topk(const float* logits, int64_t B, int64_t C, int64_t H, int64_t W,
                      int64_t sB, int64_t sC, int64_t sH, int64_t sW,
                      const uint8_t* exclude, int strategy, int64_t k,
                      int32_t* out_idx, float* out_val, float* out_map,
                      void* workspace, size_t ws_bytes, pp_stream_t stream);

/* Score map only (query.py:190-201; also model.py:241-260 Model._query).  exclude may be NULL. */
int pp_acq_score_map(const float* logits, int64_t B, int64_t C, int64_t H, int64_t W,
                     int64_t sB, int64_t sC, int64_t sH, int64_t sW,
                     const uint8_t* exclude, int strategy, float* out_map, pp_stream_t stream);

/* MC-dropout accumulation (query.py:181-187 `uc_map += uc_map_; prob += prob_`, then / mc_n_steps): over the T passes in
 * logits [T,C,H,W] (element strides sT,sC,sH,sW), prob_out [C,H,W] (+)= scale * sum_t softmax(logits[t]) and
 * uc_out [H,W] (+)= scale * sum_t score(softmax(logits[t])) with the strategy's formula on the probabilities; either
 * output may be NULL; accumulate == 0 overwrites.  No [T,C,H,W] probability tensor exists. */
int pp_acq_softmax_sum(const float* logits, int64_t T, int64_t C, int64_t H, int64_t W, int64_t sT, int64_t sC, int64_t sH,
                       int64_t sW, float* prob_out, float* uc_out, int strategy, float scale, int accumulate, pp_stream_t stream);

/* query.py:246-247 UncertaintySampler.__call__(prob): prob f32 [B,C,H,W] (already softmaxed, any
 * strides) -> out_map f32 [B,H,W]; formulas of query.py:229-239 verbatim (no exclusion). */
int pp_uncertainty_from_prob(const float* prob, int64_t B, int64_t C, int64_t H, int64_t W,
                             int64_t sB, int64_t sC, int64_t sH, int64_t sW,
                             int strategy, float* out_map, pp_stream_t stream);

/* query.py:57-61 on a GIVEN score map: scores f32 [B,N] contiguous -> out_idx i32 [B,k] (+ out_val).
 * largest != 0 selects the k largest.  Same ordering policy as pp_acq_score_topk. */
size_t pp_topk_workspace_bytes(int64_t B, int64_t N, int64_t k);

int pp_topk_select(const float* scores, int64_t B, int64_t N, int64_t k, int largest,
                   int32_t* out_idx, float* out_val,
                   void* workspace, size_t ws_bytes, pp_stream_t stream);

/* Acquisition straight from the LOW-resolution classifier output.  Replaces, in one launch
 * and without materialising the full-resolution logits,
 *   deeplab.py:55-56   pred = F.interpolate(pred, size=inputs.shape[2:], mode='bilinear', align_corners=True)
 *   query.py:190       prob = F.softmax(model(x)["pred"][:, :, :h, :w], dim=1)      ([:h,:w] = the VOC crop, :171-174)
 *   query.py:229-239, 195-201, 57-61   score, exclusion, top-k   (as pp_acq_score_topk)
 *   low      f32 [B,h,w,ldx] channels-last classifier output (what SegmentHead's 1x1 conv writes), C valid channels
 *   H, W     the size the reference interpolates to (the network input size); align_corners as F.interpolate's flag
 *   Hc, Wc   the crop scored and indexed: pixel (Y,X), Y < Hc <= H, X < Wc <= W, has flat index Y*Wc + X
 *   exclude  u8 [B,Hc,Wc] or NULL;  out_idx i32 [B,k], out_val f32 [B,k] or NULL, out_map f32 [B,Hc,Wc] or NULL
 *   k == 0   writes out_map only (out_idx / workspace may be NULL).
 * The interpolated logits are bit-identical to pp_bilinear_fwd's, so the result equals pp_bilinear_fwd followed by
 * pp_acq_score_topk bit for bit (tested). */
size_t pp_acq_lowres_workspace_bytes(int64_t B, int64_t C, int64_t Hc, int64_t Wc, int64_t k);

int pp_acq_lowres_score_topk(const float* low, int64_t ldx, int64_t B, int64_t C, int64_t h, int64_t w,
                             int64_t H, int64_t W, int align_corners, int64_t Hc, int64_t Wc,
                             const uint8_t* exclude, int strategy, int64_t k,
                             int32_t* out_idx, float* out_val, float* out_map,
                             void* workspace, size_t ws_bytes, pp_stream_t stream);

/* The strategy's score (no exclusion) at n listed pixels of the interpolated map: pixel i is image img_idx[i] (i32),
 * flat index pix_idx[i] = Y*Wc + X (i32) -> out[i].  QueryStats' "entropy at the queried pixels" (query.py:262-266)
 * without the full softmax map. */
int pp_acq_lowres_score_at(const float* low, int64_t ldx, int64_t B, int64_t C, int64_t h, int64_t w,
                           int64_t H, int64_t W, int align_corners, int64_t Hc, int64_t Wc, int strategy,
                           const int32_t* img_idx, const int32_t* pix_idx, int64_t n, float* out,
                           pp_stream_t stream);

/* MC-dropout acquisition straight from the low-resolution classifier output: the mean over T stochastic passes of the
 * strategy's score, then exclusion and top-k, in one launch and without the T full-resolution logit tensors.  Replaces
 *   deeplab.py:55-56   the x4 (x2) bilinear upsample of every pass
 *   query.py:177-187   uc_map += uncertainty_sampler(softmax(model(x)["pred"][:, :, :h, :w])) per pass, / mc_n_steps
 *   query.py:190, 195-201, 57-61   softmax, exclusion fill, top-k   (as pp_acq_lowres_score_topk)
 *   low      f32 [B*T,h,w,ldx] channels-last, IMAGE-MAJOR: passes t = 0..T-1 of image b are entries b*T + t
 *   scale    the factor on the sum over the passes (1 / mc_n_steps)
 * Everything else - H, W, align_corners, the crop Hc x Wc, exclude, k == 0 (map only), the ordering policy, the error codes and
 * the workspace, pp_acq_lowres_workspace_bytes(B, C, Hc, Wc, k) (T does not enter) - is pp_acq_lowres_score_topk's.
 * C <= 64 (PP_ACQ_MAX_CLASSES); wider heads return PP_ERR_UNSUPPORTED (pp_bilinear_fwd + pp_acq_softmax_sum serve them).
 * The result equals pp_bilinear_fwd of the B*T entries, pp_acq_softmax_sum(accumulate = 0) per image, the fill at excluded
 * pixels and pp_topk_select, bit for bit (tested): per-pass scores in the reference's operation order, NaN (0 * log 0,
 * query.py:230) in any pass makes the mean NaN. */
int pp_acq_lowres_mc_score_topk(const float* low, int64_t ldx, int64_t B, int64_t T, int64_t C, int64_t h, int64_t w,
                                int64_t H, int64_t W, int align_corners, int64_t Hc, int64_t Wc,
                                const uint8_t* exclude, int strategy, float scale, int64_t k,
                                int32_t* out_idx, float* out_val, float* out_map,
                                void* workspace, size_t ws_bytes, pp_stream_t stream);

/* The strategy's score OF THE MEAN PROBABILITY p_c = scale * sum_t softmax(x_t)_c (no exclusion) at n listed pixels, as
 * pp_acq_lowres_score_at lists them: QueryStats._get_entropy(query, prob) of the MC-dropout branch (query.py:262-264 on the
 * `prob` of :177-187) at the picked pixels only - no [C,H,W] mean-probability map.  Formulas: pp_uncertainty_from_prob's. */
int pp_acq_lowres_mc_score_at(const float* low, int64_t ldx, int64_t B, int64_t T, int64_t C, int64_t h, int64_t w,
                              int64_t H, int64_t W, int align_corners, int64_t Hc, int64_t Wc, int strategy, float scale,
                              const int32_t* img_idx, const int32_t* pix_idx, int64_t n, float* out, pp_stream_t stream);

/* MC-dropout HARD vote (args.py:34 `--vote_type hard`, stored at query.py:31 and read by nothing in the reference: the semantics
 * below are this library's specification).  In the MC-dropout branch (query.py:177-187) every stochastic pass t casts ONE vote per
 * pixel, a_t = argmax_c x_t[c] of its logits (no softmax: it is monotone; exactly equal logits -> the LOWEST class index), and the
 * score is a function of the vote counts n_c = #{t : a_t = c} (sum n_c = T), n_(1) >= n_(2) the two largest (n_(2) = 0: unanimous):
 *   PP_ACQ_ENTROPY           float(sum_c tab[n_c]) * 2^-24, tab[0] = 0, tab[n] = (uint32) llrint(-(n/T) ln(n/T) 2^24) evaluated in
 *                            double on the host; an integer sum - a function of the multiset of counts, independent of class order
 *   PP_ACQ_LEAST_CONFIDENCE  float(T - n_(1)) / float(T)        PP_ACQ_MARGIN  float(n_(1) - n_(2)) / float(T)    (one IEEE division)
 * Largest scores win for entropy / least-confidence, smallest for margin, as everywhere.  Excluded pixels get -1.0 (entropy,
 * least-confidence) or 2.0 (margin) - NOT the soft scorers' 0.0 / 1.0, which here are the scores of every unanimous pixel: an
 * excluded pixel sorts strictly behind every un-excluded one (and is still returned, lowest index first, when k exceeds the number
 * of un-excluded pixels).  Ordering policy unchanged: value-sorted, ties -> lower flat index; no NaN can occur.  The scores take few
 * distinct values, so ties decide most picks.  T in [1, 255] (the counts are bytes), otherwise PP_ERR_UNSUPPORTED; PP_ACQ_REFERENCE_ORDER
 * has no meaning here and is PP_ERR_BAD_ARG.
 *
 * pp_acq_vote_accumulate: over the T passes in logits [T,C,H,W] (element strides sT,sC,sH,sW; any C), votes u8 [C,H,W] (+)= the
 * per-class vote counts; accumulate == 0 overwrites.  The caller keeps the total over all accumulating calls <= 255.
 * Null logits / votes, bad shape: PP_ERR_BAD_ARG. */
int pp_acq_vote_accumulate(const float* logits, int64_t T, int64_t C, int64_t H, int64_t W,
                           int64_t sT, int64_t sC, int64_t sH, int64_t sW,
                           uint8_t* votes, int accumulate, pp_stream_t stream);

/* votes u8 [B,C,H,W] of T passes each -> out_map f32 [B,H,W]: the hard-vote score above, the fills at exclude (u8 [B,H,W] or NULL).
 * Null votes / out_map, bad shape, unknown strategy: PP_ERR_BAD_ARG; T outside [1, 255] or B > 65535: PP_ERR_UNSUPPORTED. */
int pp_acq_vote_score_map(const uint8_t* votes, int64_t B, int64_t T, int64_t C, int64_t H, int64_t W,
                          const uint8_t* exclude, int strategy, float* out_map, pp_stream_t stream);

/* pp_acq_lowres_mc_score_topk with the hard vote in place of the mean score: votes of the T passes of the interpolated (cropped)
 * logits, score, fills and top-k in one launch, no full-resolution logits of any pass.  low, ldx, B, T, C, h, w, H, W, align_corners,
 * Hc, Wc, exclude, k == 0 (map only), out_idx / out_val / out_map and the workspace, pp_acq_lowres_workspace_bytes(B, C, Hc, Wc, k)
 * (T does not enter), are that entry's; out_map holds the fills above.  C <= 64 (PP_ACQ_MAX_CLASSES), wider heads return
 * PP_ERR_UNSUPPORTED (pp_bilinear_fwd + pp_acq_vote_accumulate + pp_acq_vote_score_map serve them), as does T outside [1, 255];
 * PP_ERR_BAD_K / PP_ERR_WORKSPACE / PP_ERR_BAD_ARG as pp_acq_lowres_score_topk.  The result equals pp_bilinear_fwd of the B*T entries,
 * pp_acq_vote_accumulate per image, pp_acq_vote_score_map and pp_topk_select, bit for bit (tested). */
int pp_acq_lowres_mc_vote_topk(const float* low, int64_t ldx, int64_t B, int64_t T, int64_t C, int64_t h, int64_t w,
                               int64_t H, int64_t W, int align_corners, int64_t Hc, int64_t Wc,
                               const uint8_t* exclude, int strategy, int64_t k,
                               int32_t* out_idx, float* out_val, float* out_map,
                               void* workspace, size_t ws_bytes, pp_stream_t stream);

/* MC-dropout scores of the MEAN PROBABILITY over the passes, and BALD.  The reference accumulates the mean probability
 * (`prob += prob_`, query.py:185-187) but ranks pixels by the mean of the per-pass scores; the semantics below are this library's
 * specification.  Per pixel, over T passes with logits x_t:
 *   p_t = softmax(x_t)                       m = max_c x_c, S = sum_c expf(x_c - m), p_c = expf(x_c - m) / S (pp_acq_softmax_sum's)
 *   pm_c = scale * sum_t p_t,c               fp32, ascending t, then one multiply: what pp_acq_softmax_sum writes to prob_out
 *   PP_ACQ_ENTROPY / PP_ACQ_LEAST_CONFIDENCE / PP_ACQ_MARGIN   pp_uncertainty_from_prob's formulas on pm (the committee's consensus)
 *   PP_ACQ_BALD    H(pm) - scale * sum_t H(p_t): the first term is the consensus entropy above, the second is what
 *                  pp_acq_softmax_sum(..., uc_out, PP_ACQ_ENTROPY, scale, ...) writes; ONE IEEE subtraction, not clamped - rounding
 *                  may leave the score of a deterministic pixel a few ulp below 0
 * The largest scores win for entropy, least-confidence and BALD, the smallest for margin.  Excluded pixels get -1.0 (entropy,
 * least-confidence, BALD) or 2.0 (margin), the hard vote's fills: 0.0 is the BALD of every deterministic pixel, and an excluded pixel
 * sorts strictly behind those.  Ordering policy unchanged: value-sorted, ties -> lower flat index, NaN (0 * log 0 in a pass or in pm)
 * first for largest; k beyond the number of un-excluded pixels returns excluded pixels, lowest index first.  PP_ACQ_REFERENCE_ORDER
 * has no meaning here and is PP_ERR_BAD_ARG, as is any strategy above PP_ACQ_BALD.
 *
 * pp_acq_mean_prob_score_map - the tail of the full-size route: prob f32 [B,C,H,W] (element strides sB,sC,sH,sW; any class count)
 * holds pm, mean_ent f32 [B,H,W] holds scale * sum_t H(p_t) - required for PP_ACQ_BALD, NULL otherwise (else PP_ERR_BAD_ARG) -,
 * exclude u8 [B,H,W] or NULL -> out_map f32 [B,H,W].  Without exclusion the three consensus maps equal pp_uncertainty_from_prob's
 * bit for bit.  Null prob / out_map, bad shape: PP_ERR_BAD_ARG; B > 65535: PP_ERR_UNSUPPORTED. */
int pp_acq_mean_prob_score_map(const float* prob, int64_t B, int64_t C, int64_t H, int64_t W,
                               int64_t sB, int64_t sC, int64_t sH, int64_t sW,
                               const float* mean_ent, const uint8_t* exclude, int strategy, float* out_map, pp_stream_t stream);

/* pp_acq_lowres_mc_score_topk with the scores above in place of the mean score: the passes, the consensus or BALD score, the fills
 * and the top-k in one launch, no full-resolution logits of any pass and no [C,H,W] probability map.  Every argument, k == 0 (map
 * only), the workspace pp_acq_lowres_workspace_bytes(B, C, Hc, Wc, k) and the error codes are that entry's; C <= 64
 * (PP_ACQ_MAX_CLASSES), wider heads return PP_ERR_UNSUPPORTED (the full-size route serves them).  The result equals pp_bilinear_fwd
 * of the B*T entries, pp_acq_softmax_sum(prob_out, uc_out with PP_ACQ_ENTROPY, accumulate = 0) per image,
 * pp_acq_mean_prob_score_map and pp_topk_select, bit for bit (tested). */
int pp_acq_lowres_mc_mean_topk(const float* low, int64_t ldx, int64_t B, int64_t T, int64_t C, int64_t h, int64_t w,
                               int64_t H, int64_t W, int align_corners, int64_t Hc, int64_t Wc,
                               const uint8_t* exclude, int strategy, float scale, int64_t k,
                               int32_t* out_idx, float* out_val, float* out_map,
                               void* workspace, size_t ws_bytes, pp_stream_t stream);

/* Spread-out picks: a minimum pixel distance between the picks of one image.  Stands beside query.py:57-64 - the top-k and the
 * reference's only answer to clustered picks, a RANDOM sub-sample of the best top_n_percent - as a deterministic alternative; the
 * semantics below are this library's specification.  Per image:
 *   cand     i32 [B,M]: flat indices y*W + x in RANK order - what every *_topk entry writes to out_idx with k = M
 *   W        the row length the flat indices were formed with; N the pixels per image (exclude's row length); 1 <= k <= M <= N
 *   d        minimum distance in pixels, d >= 1;  exclude u8 [B,N] or NULL
 *   spread phase  walk i = 0 .. M-1: skip cand[i] when exclude[cand[i]] != 0; accept it iff (y-y')^2 + (x-x')^2 >= d^2 for every
 *                 pick (y',x') accepted so far (exact integer arithmetic, 64-bit where a coordinate difference can exceed 46340);
 *                 stop at k accepted picks.  n = the number accepted.
 *   fill phase    n < k: the remaining k - n slots take the earliest list positions the spread phase did not accept, in list order,
 *                 the distance rule dropped (excluded candidates included) - k picks always come back, as from plain top-k.
 *   out_idx  i32 [B,k] in acceptance order, then fill order;  out_pos i32 [B,k] the list position of each pick (to gather the
 *            *_topk entry's out_val, or anything else kept per candidate);  out_n i32 [B] = n.
 * d == 1 returns the first k un-excluded candidates.  A candidate outside [0, N) is treated as EXCLUDED: its exclusion byte is never
 * read, the spread phase never accepts it, the fill phase may return it as it stands.
 * One pick blocks at most A(d) = #{(dy,dx) : dy^2 + dx^2 < d^2} candidates, itself included, so with M = min(N, max(k, (k-1) A(d) + 1))
 * the result equals the greedy pass over the image's whole ranking whenever the first M ranks hold no excluded pixel (tested).
 * No workspace, no synchronisation.  k <= 1024 (the picks live in LDS), beyond: PP_ERR_UNSUPPORTED, as is B > 2^31 - 1.  Null cand /
 * out_idx / out_pos / out_n, B / M / W / N / k / d < 1, k > M, M > N, N or W > 2^31 - 1: PP_ERR_BAD_ARG. */
int pp_spread_select(const int32_t* cand, int64_t B, int64_t M, int64_t W, int64_t N, int64_t k, int64_t d,
                     const uint8_t* exclude, int32_t* out_idx, int32_t* out_pos, int32_t* out_n, pp_stream_t stream);

/* Region-aware acquisition: window impurity x window uncertainty ("region impurity and prediction uncertainty", Xie et al., CVPR 2022).
 * The reference has no such score; the semantics below are this library's specification (tests/region_oracle.py restates them).
 * Per image of H x W pixels and a radius r, 1 <= r <= 16, at the pixel (y, x):
 *   window      Omega = {(y',x') : |y'-y| <= r, |x'-x| <= r, 0 <= y' < H, 0 <= x' < W}: clipped at the image border, never wrapped, never
 *               reaching into the next image of the batch.  N = |Omega| = (clipped rows) * (clipped columns), 1 <= N <= (2r+1)^2 <= 1089.
 *   counts      n_c = #{p in Omega : pred[p] == c}, c = 0 .. C-1; a byte >= C (pp_predict_lowres writes none) is counted in ONE extra
 *               bin C, so no input indexes out of range.
 *   impurity    exact in integers: tab[n] = llrint(n * ln(n) * 2^16) computed in double on the host, tab[0] = tab[1] = 0 (the largest
 *               entry, tab[1089] = 499 082 426, fits 31 bits).  G = sum_c tab[n_c], D = tab[N] - G: an integer >= 0, and 0 exactly
 *               where the window holds one label.  P = (float)D / (float)(N * 65536): one int -> float conversion (round to nearest
 *               even), one correctly rounded fp32 division; this is ln N - (1/N) sum_c n_c ln n_c, the entropy of the window's labels.
 *               The integer sum makes P independent of the order in which the window is visited.
 *   uncertainty u[p] = flip ? 1.0f - unc[p] : unc[p];  U = (sum_{p in Omega} u[p]) / (float)N, the sum in fp32 in a fixed order (the
 *               2r+1 columns of each window row left to right from the first, then the 2r+1 row sums top to bottom from the first;
 *               positions outside the image enter as +0.0f), so the same input gives the same bits on every run.  A NaN in unc makes
 *               NaN exactly the outputs whose window holds it and changes no other output (no running sums over floats).
 *   score       mode 0: P * U (one fp32 multiplication), mode 1: P, mode 2: U.  The LARGEST score wins in every mode (flip = 1 turns
 *               the margin, whose smallest value is the most uncertain, into 1 - margin).
 *   exclusion   exclude[p] != 0 sets the output AT p to -1.0f (0.0 is the legitimate score of every pure window, the fill ranks
 *               behind it); the excluded pixel still counts inside other pixels' windows.
 * pp_acq_region_table_words(r) = (2r+1)^2 + 1, 0 for r outside [1,16].  pp_acq_region_table fills host_tab[0 .. words) on the HOST (no
 * launch; null host_tab: PP_ERR_BAD_ARG, r outside [1,16]: PP_ERR_UNSUPPORTED); the caller copies it to the device once per radius and
 * owns that copy, like every workspace here.
 * pp_acq_region_score_map: pred u8 [B,H,W] (what pp_predict_lowres writes), unc f32 [B,H,W] (what pp_acq_lowres_score_topk writes with
 * k == 0), tab the DEVICE copy of the table for this r, exclude u8 [B,H,W] or NULL, out_map f32 [B,H,W], fully overwritten.  unc may
 * be NULL in mode 1; pred and tab may be NULL in mode 2.  One launch; no workspace, no atomics, no synchronisation.
 * PP_ERR_BAD_ARG: mode outside 0..2, a null required pointer, B / H / W < 1, C outside [1,256].  PP_ERR_UNSUPPORTED: r outside [1,16],
 * H*W > 2^31 - 1, a grid past 2^31 - 1 blocks (one block per 64 x 64 tile of an image).  Every refusal comes before anything is
 * enqueued and no pointer is read. */
size_t pp_acq_region_table_words(int64_t r);
int pp_acq_region_table(int64_t r, uint32_t* host_tab);
int pp_acq_region_score_map(const uint8_t* pred, const float* unc, int64_t B, int64_t C, int64_t H, int64_t W, int64_t r, int mode,
                            int flip, const uint32_t* tab, const uint8_t* exclude, float* out_map, pp_stream_t stream);

/* Class-balanced picks: the picks of one image handed out round-robin over the PREDICTED classes of a rank-ordered pool.  Stands beside
 * query.py:63-64 - the reference draws n_pixels_by_us of the best top_n_percent at random, blind to classes - as a deterministic
 * alternative; the reference has no such step, the semantics below are this library's specification (tests/balance_oracle.py restates
 * them).  Per image b:
 *   cand     i32 [B,M]: flat pixel indices in RANK order - what every *_topk entry writes to out_idx with k = M
 *   label    u8 [B,N]: the label map pp_predict_lowres writes;  exclude u8 [B,N] or NULL;  N the pixels per image, 1 <= k <= M <= N
 *   eligible list position i is eligible iff 0 <= cand[i] < N and (exclude == NULL or exclude[b*N + cand[i]] == 0).  For an ineligible
 *            position neither label nor exclude is read at an out-of-range index.
 *   class    c_i = label[b*N + cand[i]], the byte as it stands, 0 .. 255 (unsigned).  There is no class-count argument: always 256 bins,
 *            no input indexes out of range.
 *   rank     r_i = #{j < i : j eligible and c_j == c_i}, counted in list order (32-bit counts: a class may hold more than 65 535
 *            entries of a long list).
 *   balanced phase  E = the number of eligible positions, n = min(k, E).  The picks are the n eligible positions smallest in the
 *            lexicographic key (r_i, i), written in that order: round 0 holds the best entry of every class in the pool, in list order,
 *            round 1 every class's second entry, and so on.  Every class's picks are a prefix of its own ranking; the pick counts of
 *            two classes differ by at most one unless the smaller class is exhausted.
 *   fill phase      n < k: the remaining k - n slots take the earliest INELIGIBLE list positions, in list order - k picks always come
 *            back, as from plain top-k and from pp_spread_select.
 * A repeated index in cand is two list entries: nothing is de-duplicated.
 *   out_idx  i32 [B,k] = cand at the picked positions;  out_pos i32 [B,k] their list positions;  out_n i32 [B] = n.
 * One launch, no workspace, no global atomics (the same bits on every run), no synchronisation.  PP_ERR_BAD_ARG: null cand / label /
 * out_idx / out_pos / out_n, B / M / N / k < 1, k > M, M > N, N > 2^31 - 1.  PP_ERR_UNSUPPORTED: k > 1024 (pp_spread_select's cap: one
 * slot counter per round lives in LDS), B > 2^31 - 1.  Every refusal comes before anything is enqueued and no pointer is read. */
int pp_class_balance_select(const int32_t* cand, int64_t B, int64_t M, int64_t N, int64_t k,
                            const uint8_t* label, const uint8_t* exclude,
                            int32_t* out_idx, int32_t* out_pos, int32_t* out_n, pp_stream_t stream);

/* Feature-diverse picks: k-centre greedy (core-set) selection over the class-probability vectors of a rank-ordered pool.  Stands beside
 * query.py:63-64 as the fourth deterministic alternative to the random sub-sample; the reference has no such step, the semantics below
 * are this library's specification (tests/diverse_oracle.py restates them).
 *
 * pp_acq_lowres_prob_at_u8: the features.  pp_acq_lowres_score_at's sibling - the same geometry and validation, the class vector of
 * listed pixel i (image img_idx[i], flat crop index pix_idx[i]) interpolated to the bits pp_bilinear_fwd writes - but what leaves is the
 * softmax itself, as bytes: row out[i*ldf .. i*ldf + ldf), byte c < C = min(255, (int) rintf(255.0f * p_c)) with p the fp32 softmax in
 * the default scorer's arithmetic (m = max, e_c = 2^((x_c - m) log2 e), p_c = e_c / sum e), a NaN probability -> 0; bytes C .. ldf-1
 * are written as 0.  An entry with img_idx[i] outside [0,B) or pix_idx[i] outside [0,Hc*Wc) gets an all-zero row and `low` is not read
 * for it.  Rows leave as whole dwords.  ldf >= C, ldf % 4 == 0, out 4-byte aligned, else PP_ERR_BAD_ARG; C > 256: PP_ERR_UNSUPPORTED;
 * n == 0: PP_OK without a launch; null img_idx / pix_idx / out with n > 0: PP_ERR_BAD_ARG.  Heads up to 64 classes keep the class
 * vector in registers, wider ones stream it in three passes (max, sum, emit) - the same bytes. */
int pp_acq_lowres_prob_at_u8(const float* low, int64_t ldx, int64_t B, int64_t C, int64_t h, int64_t w,
                             int64_t H, int64_t W, int align_corners, int64_t Hc, int64_t Wc,
                             const int32_t* img_idx, const int32_t* pix_idx, int64_t n,
                             uint8_t* out, int64_t ldf, pp_stream_t stream);

/* pp_diverse_select: the selection.  Per image b:
 *   cand     i32 [B,M]: flat pixel indices in RANK order - what every *_topk entry writes to out_idx with k = M
 *   feat     u8 [B,M,ldf]: row i belongs to LIST POSITION i; only its first F bytes have meaning (1 <= F <= 256, ldf >= F,
 *            ldf % 4 == 0, feat 4-byte aligned).  No byte of a row past F enters the result.
 *   eligible pp_class_balance_select's rule: 0 <= cand[i] < N and (exclude == NULL or exclude[b*N + cand[i]] == 0); exclude is never
 *            read at an out-of-range index.
 *   D(i,j)   sum_{f<F} (feat[i][f] - feat[j][f])^2 in exact integers (at most 256 * 255^2 = 16 646 400: 32-bit accumulation).
 *   greedy phase  E = the number of eligible positions, n = min(k, E).  Pick 0 is the earliest eligible position (the pool's most
 *            uncertain pixel); pick t >= 1 the eligible, not yet picked position i with the largest r_i = min over the picks so far of
 *            D(i, pick), ties to the smallest i.  A picked position is never picked again, even when r_i = 0 for everything left:
 *            identical features come back in list order.  Ineligible positions are never centres and never picked here.
 *   fill phase    n < k: the remaining slots take the earliest INELIGIBLE positions in list order (pp_class_balance_select's rule).
 * A repeated index in cand is two list entries.
 *   out_idx  i32 [B,k] = cand at the picked positions;  out_pos i32 [B,k] the positions;  out_n i32 [B] = n;
 *   out_dist i32 [B,k] = r_i at the moment pick t >= 1 was taken (the k-centre radius sequence: non-increasing over t = 1 .. n-1);
 *            pick 0 and the fill slots hold -1.
 * Integer arithmetic only and no global atomics: the same bytes on every run.  One launch, one block per image: the RESIDENT form
 * (M <= pp_diverse_resident_candidates(F); 0 = no such form in this build) stages the rows once as dword planes in LDS with r behind
 * them and runs the k steps there; the STREAMING form reads rows and r (the workspace, u32 [B,M]) from memory every step and takes
 * every M <= N.  workspace: at least pp_diverse_workspace_bytes(B, M, F) bytes (>= 4*B*M; 0 for arguments no launch accepts), 4-byte
 * aligned, required by both forms.
 * PP_ERR_BAD_ARG: null cand / feat / out_idx / out_pos / out_dist / out_n / workspace, B / M / N / k / F < 1, k > M, M > N,
 * N > 2^31 - 1, F > 256, ldf < F or not a multiple of 4, a misaligned feat, a workspace too small.  PP_ERR_UNSUPPORTED: k > 1024 (the
 * cap of the other two selectors), B > 2^31 - 1, B*M > 2^40.  Every refusal comes before anything is enqueued and no pointer is read. */
size_t pp_diverse_workspace_bytes(int64_t B, int64_t M, int64_t F);
int64_t pp_diverse_resident_candidates(int64_t F);   /* host arithmetic only */
int pp_diverse_select(const int32_t* cand, int64_t B, int64_t M, int64_t N, int64_t k,
                      const uint8_t* feat, int64_t F, int64_t ldf, const uint8_t* exclude,
                      int32_t* out_idx, int32_t* out_pos, int32_t* out_dist, int32_t* out_n,
                      void* workspace, size_t ws_bytes, pp_stream_t stream);


/* =============================================================================================
 * Network layers (DeepLabv3+-MobileNetV2 / FPN-ResNet50 forward + backward), NHWC fp32.
 *
 * Activations are [B,H,W,C] with an explicit pixel stride `ld` (elements): a channel slice of a wider
 * tensor is addressed by offsetting the pointer, which is how the reference's torch.cat tensors
 * (aspp.py:73, deeplab.py:50) are produced and consumed without a copy.  Dense-conv weights are HWIO
 * [kh][kw][Cin][Cout]; depthwise weights [3][3][C].  All reductions are deterministic (two-stage, no
 * float atomics).  Workspaces are caller-owned.
 * ============================================================================================= */

/* nn.Conv2d forward (dense, groups=1) as an implicit GEMM on the fp32 MFMA pipe.
 * networks/mobilenet_v2.py:9,42,48,56; aspp.py:9-10,55,58; deeplab.py:24; decoders.py:107,111,116;
 * backbones/resnet_models.py Bottleneck convs; decoders.py:25-28,92 (bias != NULL).
 * y[b,oh,ow,n] = bias[n] + sum x[b, oh*stride - pad + th*dil, ow*stride - pad + tw*dil, c] * w[th,tw,c,n] */
/* `workspace` (optional, may be NULL / 0): scratch for the split-K form used when the output has too few tiles to
 * fill the 256 CUs (partial sums [splits][M][Cout], reduced in fixed order: deterministic).  Size it with
 * pp_conv2d_fwd_workspace_bytes (0 = this shape never splits); with less, the single-pass form runs. */
size_t pp_conv2d_fwd_workspace_bytes(int B, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad, int dil);
int pp_conv2d_fwd(const float* x, int64_t ldx, int B, int H, int W, int Cin, const float* w, const float* bias,
                  int kh, int kw, int stride, int pad, int dil, float* y, int64_t ldy, int Cout, void* workspace,
                  size_t ws_bytes, pp_stream_t stream);

/* ---- training BatchNorm split over its neighbours (SURVEY.md 7 hard part (b); mobilenet_v2.py:42-56: pw -> BN -> ReLU6 -> dw ->
 * BN -> ReLU6 -> pw).  The producer's epilogue delivers partial column statistics (pp_conv2d_fwd_stats, pp_dwconv3x3_fwd_fused),
 * pp_bn_finalize_partials turns them into mean / invstd / running statistics and the folded per-channel scale / shift, and the
 * CONSUMER applies act(fma(x, scale, shift)) where it loads its input (pp_dwconv3x3_fwd_fused, pp_conv2d_fwd_affine_in,
 * pp_dwconv3x3_bwd_weight_affine_in): the normalised tensor is never written.  Arithmetic = pp_scale_shift_act's, so a consumer of
 * the raw tensor + (scale, shift, act) computes what it would compute from the materialised tensor, bit for bit.
 *   pp_bn_finalize_partials            stats [rows][2][C] (sum, sum of squares) over M rows -> mean, invstd, scale = gamma*invstd,
 *                                      shift = beta - mean*scale, running-stat update (nn.BatchNorm2d training semantics)
 *   pp_dwconv3x3_fwd_stats_rows        partial rows pp_dwconv3x3_fwd_fused writes for this shape
 *   pp_dwconv3x3_fwd_fused             depthwise 3x3 with optional input affine (in_scale may be NULL) and optional output statistics
 *   pp_dwconv3x3_bwd_weight_affine_in  pp_dwconv3x3_bwd_weight on x = act(fma(x_raw, in_scale, in_shift))
 *   pp_conv2d_fwd_accepts_affine_in    1 when pp_conv2d_fwd_affine_in has a kernel for this shape (stride-1 pad-0 pointwise layers:
 *                                      the in-block split-K kernel, or the 128x32-tiled kernel for <= 32 output channels)
 *   pp_conv2d_fwd_affine_in            pp_conv2d_fwd on x = act(fma(x_raw, in_scale, in_shift)); fails (no fallback) on other shapes */
int pp_bn_finalize_partials(const float* stats, int64_t rows, int64_t M, int C, const float* gamma, const float* beta, float eps,
                            float momentum, float* running_mean, float* running_var, float* mean, float* invstd, float* scale,
                            float* shift, pp_stream_t stream);
int64_t pp_dwconv3x3_fwd_stats_rows(int B, int H, int W, int C, int stride, int pad, int dil);
int pp_dwconv3x3_fwd_fused(const float* x, int64_t ldx, int B, int H, int W, int C, const float* w, int stride, int pad, int dil,
                           const float* in_scale, const float* in_shift, int in_act, float* y, int64_t ldy, float* stats,
                           size_t stats_floats, pp_stream_t stream);
int pp_dwconv3x3_bwd_weight_affine_in(const float* x_raw, int64_t ldx, int B, int H, int W, int C, const float* in_scale,
                                      const float* in_shift, int in_act, const float* dy, int64_t lddy, int stride, int pad, int dil,
                                      float* dw, void* workspace, size_t ws_bytes, pp_stream_t stream);
int pp_conv2d_fwd_accepts_affine_in(int B, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad, int dil);
int pp_conv2d_fwd_affine_in(const float* x_raw, int64_t ldx, int B, int H, int W, int Cin, const float* in_scale, const float* in_shift,
                            int in_act, const float* w, const float* bias, int kh, int kw, int stride, int pad, int dil, float* y,
                            int64_t ldy, int Cout, void* workspace, size_t ws_bytes, pp_stream_t stream);

/* Inference form of Conv2d -> BatchNorm2d(eval) [-> + residual] -> ReLU/ReLU6 in ONE launch (mobilenet_v2.py:7-12,
 * 36-57; aspp.py:9-20; decoders.py:107-113; resnet_models.py:71-92): the epilogue folds scale = gamma/sqrt(running_var+eps),
 * shift = beta - running_mean*scale with the arithmetic of pp_bn_eval_affine + pp_scale_shift_act (bit-identical results).
 * gamma == NULL: no BatchNorm (bias / residual / activation only).  act: 0 none, 1 ReLU, 2 ReLU6. */
int pp_conv2d_fwd_bn_act(const float* x, int64_t ldx, int B, int H, int W, int Cin, const float* w, const float* bias,
                         int kh, int kw, int stride, int pad, int dil, const float* gamma, const float* beta,
                         const float* running_mean, const float* running_var, float eps, const float* residual,
                         int64_t ldr, int act, float* y, int64_t ldy, int Cout, void* workspace, size_t ws_bytes,
                         pp_stream_t stream);

/* dL/dx of the above (what autograd computes at model.py:121); any stride (the stride-2 Bottleneck convs of
 * backbones/resnet_models.py:63-64,142-144 gather dY rows where (row + pad - tap*dil) is divisible by the stride).
 * B,H,W,Cin describe the conv INPUT for the workspace query.  accumulate != 0: dx += result (the tensor already holds
 * the gradient of another consumer of x, e.g. the residual branch of mobilenet_v2.py:62-63). */
size_t pp_conv2d_bwd_data_workspace_bytes(int B, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad, int dil);
int pp_conv2d_bwd_data(const float* dy, int64_t lddy, int B, int Ho, int Wo, int Cout, const float* w, int kh, int kw,
                       int stride, int pad, int dil, float* dx, int64_t lddx, int H, int W, int Cin, int accumulate,
                       void* workspace, size_t ws_bytes, pp_stream_t stream);

/* dL/dw (HWIO) and optionally dL/dbias [Cout]; workspace holds the split-M partial sums. */
size_t pp_conv2d_bwd_weight_workspace_bytes(int B, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad, int dil);
int pp_conv2d_bwd_weight(const float* x, int64_t ldx, int B, int H, int W, int Cin, const float* dy, int64_t lddy,
                         int Cout, int kh, int kw, int stride, int pad, int dil, float* dw, float* dbias,
                         void* workspace, size_t ws_bytes, pp_stream_t stream);

/* bf16x3 operand planes shared between the calls of one layer.  The MFMA-bound convolutions (layers the planner puts on the bf16x3 kernels) read their
 * activation operand as three chunk-major bf16 planes; by default every call splits its operand into its workspace.  The
 * forward's operand x is also the weight gradient's, and the backward-data's operand dy is the weight gradient's other one:
 * a caller may split a tensor ONCE with pp_x3_split and pass the planes to every *_pre call that reads it (NULL = split
 * inside, as the plain entry points do; planes are ignored by calls that do not run a bf16x3 kernel).
 * pp_conv2d_x3_planes_bytes(which, ...): 0 if the call (which = 0 forward, 1 backward-data, 2 weight gradient) would not use
 * planes, else the size of its activation planes (forward / weight gradient: of x; backward-data: of dy).
 * which = 3 / 4: the forward / backward-data call reads WEIGHT planes (pp_x3_split_weights, that direction's
 * layout) when it gets them through *_pre2 - asked by callers that keep the weight planes of a step - else 0. */
/* Backward-data of up to four convolutions that read ONE input, as one launch (+ its split-K reduce): the ASPP branches of
 * /root/reference/networks/aspp.py:49-57,64-67 - x1..x4 = aspp1..4(x): a 1x1 and three dilated 3x3 convolutions, stride 1, "same"
 * padding d*(k-1)/2 - whose input gradient torch forms as four conv-backward results added up.  dy [B,H,W,>= nb*Cout] holds branch b's
 * output gradient in channels [b*Cout, (b+1)*Cout); w_b is HWIO [k_b,k_b,Cin,Cout]; dx [B,H,W,Cin] (+)= the sum over the branches.
 * The workspace query returns 0 where the merged form is not offered (the caller then issues pp_conv2d_bwd_data per branch). */
size_t pp_conv2d_bwd_data_multi_workspace_bytes(int B, int H, int W, int Cin, int Cout, int nb, int k0, int d0, int k1, int d1, int k2, int d2,
                                                int k3, int d3);
int pp_conv2d_bwd_data_multi(const float* dy, int64_t lddy, int B, int H, int W, int Cout, int nb, const float* w0, int k0, int d0,
                             const float* w1, int k1, int d1, const float* w2, int k2, int d2, const float* w3, int k3, int d3, float* dx,
                             int64_t lddx, int Cin, int accumulate, void* workspace, size_t ws_bytes, pp_stream_t stream);

size_t pp_x3_planes_bytes(int64_t rows, int C);
int pp_x3_split(const float* x, int64_t ldx, int64_t rows, int C, void* planes, size_t planes_bytes, pp_stream_t stream);
size_t pp_conv2d_x3_planes_bytes(int which, int B, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad, int dil);
int pp_conv2d_fwd_pre(const float* x, int64_t ldx, int B, int H, int W, int Cin, const float* w, const float* bias,
                      int kh, int kw, int stride, int pad, int dil, float* y, int64_t ldy, int Cout, void* workspace,
                      size_t ws_bytes, const void* x_planes, pp_stream_t stream);
int pp_conv2d_bwd_data_pre(const float* dy, int64_t lddy, int B, int Ho, int Wo, int Cout, const float* w, int kh, int kw,
                           int stride, int pad, int dil, float* dx, int64_t lddx, int H, int W, int Cin, int accumulate,
                           void* workspace, size_t ws_bytes, const void* dy_planes, pp_stream_t stream);
/* The WEIGHTS' planes as well (round 5): they change once per optimiser step, so a training loop may split them at the start of the step on
 * another stream - transpose = 1: the forward's layout, 0: the backward-data's - and pass them to the *_pre2 forms (NULL = split inside;
 * ignored by calls that do not run a bf16x3 kernel).  /root/reference/networks/decoders.py:107-114 (the SegmentHead convolutions). */
size_t pp_x3_weight_planes_bytes(int kh_kw, int Cin, int Cout, int transpose);
int pp_x3_split_weights(const float* w, int kh_kw, int Cin, int Cout, int transpose, void* planes, size_t planes_bytes, pp_stream_t stream);
int pp_conv2d_fwd_pre2(const float* x, int64_t ldx, int B, int H, int W, int Cin, const float* w, const float* bias,
                       int kh, int kw, int stride, int pad, int dil, float* y, int64_t ldy, int Cout, void* workspace,
                       size_t ws_bytes, const void* x_planes, const void* w_planes, pp_stream_t stream);
int pp_conv2d_bwd_data_pre2(const float* dy, int64_t lddy, int B, int Ho, int Wo, int Cout, const float* w, int kh, int kw,
                            int stride, int pad, int dil, float* dx, int64_t lddx, int H, int W, int Cin, int accumulate,
                            void* workspace, size_t ws_bytes, const void* dy_planes, const void* w_planes, pp_stream_t stream);
int pp_conv2d_bwd_weight_pre(const float* x, int64_t ldx, int B, int H, int W, int Cin, const float* dy, int64_t lddy,
                             int Cout, int kh, int kw, int stride, int pad, int dil, float* dw, float* dbias,
                             void* workspace, size_t ws_bytes, const void* x_planes, const void* dy_planes, pp_stream_t stream);

/* Convolution + training BatchNorm (+ residual, activation) in ONE launch (mobilenet_v2.py:42-43,48-49,56-57: conv -> BatchNorm2d
 * [-> ReLU6]): the blocks of the convolution exchange their column sums the way the blocks of pp_bn_train_fwd_fused do (same
 * fine-grained `xchg` / `sync` areas, same epoch protocol) and normalise the tile they still hold in registers.  conv_out
 * receives the raw convolution (the BatchNorm backward's input), y the normalised output; mean / invstd / running statistics as
 * pp_bn_train_fwd_fused.  Only for shapes whose whole grid is co-resident: ask pp_conv2d_fwd_bn_train_ok (1 / 0) first - the call
 * refuses other shapes instead of falling back. */
int pp_conv2d_fwd_bn_train_ok(int B, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad, int dil);
size_t pp_conv2d_fwd_bn_train_xchg_bytes(int B, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad, int dil);
int pp_conv2d_fwd_bn_train(const float* x, int64_t ldx, int B, int H, int W, int Cin, const float* w, int kh, int kw, int stride, int pad,
                           int dil, float* conv_out, int64_t ldc, const float* gamma, const float* beta, float eps, float momentum,
                           float* running_mean, float* running_var, float* mean, float* invstd, const float* residual, int64_t ldr,
                           int act, float* y, int64_t ldy, int Cout, void* xchg, size_t xchg_bytes, int32_t* sync, size_t sync_ints,
                           pp_stream_t stream);

/* Backward-data convolution + the BatchNorm backward of the layer in FRONT of it, in one launch (the mirror of
 * pp_conv2d_fwd_bn_train; conv -> BatchNorm -> activation -> THIS convolution, the activated tensor having no other consumer:
 * mobilenet_v2.py:52-56, depthwise BatchNorm / ReLU6 -> project convolution).  dy is the gradient of this convolution's output;
 * bn_x / mean / invstd / gamma / beta / act describe the BatchNorm whose output this convolution read; dx_bn receives the gradient of
 * the BatchNorm's INPUT (what pp_bn_bwd_fused would have written), dgamma / dbeta its parameter gradients.  The gradient of the
 * BatchNorm's output is never written.  Same xchg / sync areas as the single-launch BatchNorm; ask *_ok first.
 * A BatchNorm output with more consumers (mobilenet_v2.py:63-66: the block output feeds the next block's expand convolution AND
 * its residual add) is handled when THIS convolution's backward is the last of them to run: grad_in (or NULL) = the gradient the
 * output already holds from the others, added to the tile first (the `accumulate` of a plain backward-data); dres (or NULL) receives
 * the gradient of the BatchNorm's own residual input (the masked total gradient, what pp_bn_bwd_fused writes to its dres). */
int pp_conv2d_bwd_data_bn_bwd_ok(int B, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad, int dil);
size_t pp_conv2d_bwd_data_bn_bwd_xchg_bytes(int B, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad, int dil);
int pp_conv2d_bwd_data_bn_bwd(const float* dy, int64_t lddy, int B, int Ho, int Wo, int Cout, const float* w, int kh, int kw, int stride,
                              int pad, int dil, int H, int W, int Cin, const float* bn_x, int64_t ldbx, const float* mean,
                              const float* invstd, const float* gamma, const float* beta, int act, float* dgamma, float* dbeta,
                              float* dx_bn, int64_t lddx, const float* grad_in, int64_t ldgi, float* dres, int64_t lddr,
                              void* xchg, size_t xchg_bytes, int32_t* sync, size_t sync_ints, pp_stream_t stream);

/* Deferred reduces.  A weight gradient is a partial-sum kernel ([slices][...] in the workspace) followed by a small
 * fixed-order reduce; a backward pass has ~60 of them (model.py:121 loss.backward()).  The *_partials forms run only the
 * first kernel and describe the reduce in *job (kind 0: nothing left to do - the call completed the gradient itself, e.g.
 * when a bias gradient is asked for); pp_wgrad_reduce_batch then runs any number of jobs in one launch per 64 jobs, with
 * the arithmetic of the single-layer kernels (bit-identical).  The caller keeps every job's workspace untouched until
 * the batch has been enqueued on the same stream. */
typedef struct pp_reduce_job {
    const float* part;   /* partial sums */
    float* dst;          /* the gradient tensor */
    int64_t cn;          /* elements per tap (kinds 1, 2) / outputs (kind 3) */
    int32_t splits;      /* partial slices */
    int32_t ntaps;       /* live taps (kinds 1, 2) */
    int32_t kind;        /* 0 none, 1 float4 sequential, 2 32-lane tree, 3 32-lane fp64 (depthwise) */
    uint8_t widx[12];    /* weight-tensor tap index of every live tap */
} pp_reduce_job;
int pp_conv2d_bwd_weight_partials(const float* x, int64_t ldx, int B, int H, int W, int Cin, const float* dy, int64_t lddy,
                                  int Cout, int kh, int kw, int stride, int pad, int dil, float* dw, float* dbias,
                                  void* workspace, size_t ws_bytes, pp_reduce_job* job, pp_stream_t stream);
int pp_dwconv3x3_bwd_weight_partials(const float* x, int64_t ldx, int B, int H, int W, int C, const float* dy, int64_t lddy,
                                     int stride, int pad, int dil, float* dw, void* workspace, size_t ws_bytes, pp_reduce_job* job,
                                     pp_stream_t stream);
int pp_wgrad_reduce_batch(const pp_reduce_job* jobs, int n, pp_stream_t stream);

/* Column-reduction workspace shared by pp_bn_train_fwd, pp_bn_bwd and pp_dwconv3x3_bwd_weight. */
size_t pp_colreduce_workspace_bytes(int64_t M, int C);

/* nn.BatchNorm2d, training mode (mobilenet_v2.py:10,39,49,57; aspp.py:11,56,59; deeplab.py:25;
 * decoders.py:108,112): batch mean / biased variance over the M = B*H*W rows, running-stat update
 * (momentum, unbiased variance), and the per-channel affine  scale = gamma*invstd,
 * shift = beta - mean*scale  to be applied by pp_scale_shift_act.  running_* may be NULL. */
int pp_bn_train_fwd(const float* x, int64_t ldx, int64_t M, int C, const float* gamma, const float* beta, float eps,
                    float momentum, float* running_mean, float* running_var, float* mean, float* invstd, float* scale,
                    float* shift, void* workspace, size_t ws_bytes, pp_stream_t stream);

/* The same BatchNorm2d training forward INCLUDING the apply (+ residual, + activation) in ONE launch
 * (column strips x row chunks; blocks exchange their partial sums inside the launch; see nn_ops.hip).
 * `workspace` (pp_bn_fused_workspace_bytes, 8-byte aligned) holds one 64-bit {launch tag, value} word per partial and
 * `sync` (pp_bn_fused_sync_ints ints) the launch epoch and a done-counter.  BOTH MUST be FINE-GRAINED device memory
 * (hipExtMallocWithFlags(hipDeviceMallocFinegrained)), zero-filled ONCE before first use and then left alone: the
 * blocks of a launch sit on different XCDs whose L2s are not coherent for ordinary allocations (stale partials and
 * run-to-run differences were observed with ordinary memory; pixelpick_amd/engine.py `_bn_exchange` allocates the area
 * once per device).  They must not be shared by launches that can run concurrently.  Results are deterministic. */
size_t pp_bn_fused_workspace_bytes(int64_t M, int C);
/* 1 when a [M, C] map is small enough for the single-launch training BatchNorm kernels to keep every thread's rows in
 * registers between their two passes (no second read of x / dy); then the depthwise convolution in front of a BatchNorm is
 * also computed inside that launch (pp_dwconv3x3_bn_train_fwd_fused) at no extra traffic.  mobilenet_v2.py:38-39,52-53. */
int pp_bn_fused_rows_cached(int64_t M, int C);
size_t pp_bn_fused_sync_ints(int C);
int pp_bn_train_fwd_fused(const float* x, int64_t ldx, int64_t M, int C, const float* gamma, const float* beta, float eps,
                          float momentum, float* running_mean, float* running_var, float* mean, float* invstd,
                          const float* residual, int64_t ldr, int act, float drop_p, uint64_t drop_seed,
                          const uint64_t* drop_seed_dev, float* y, int64_t ldy, void* workspace,
                          size_t ws_bytes, int32_t* sync, size_t sync_ints, pp_stream_t stream);
/* drop_p > 0: the nn.Dropout(p) that follows BN -> ReLU (aspp.py:60-61, decoders.py:108-114) is applied in the same pass
 * with pp_dropout's mask stream (same seed / seed_dev -> same mask), act must be 0 or 1. */

/* Training-mode BatchNorm whose statistics come from the PRODUCER of x (round 2): pp_conv2d_fwd_stats writes, next to the
 * convolution output, per-wave (or, behind a split-K convolution, per reduce-block) column sums and sums of squares
 * stats[rows][2][Cout] (rows = pp_conv2d_fwd_stats_rows(shape); 0 = this shape delivers none), and
 * pp_bn_train_fwd_partials reduces them (fixed order, fp64) in every block and applies scale/shift (+ residual, activation,
 * dropout) in one pass over x: no statistics pass, no exchange between blocks, no co-residency requirement
 * (mobilenet_v2.py:42-43,56-57 conv -> BatchNorm pairs and every other dense conv -> BatchNorm pair of the networks). */
int64_t pp_conv2d_fwd_stats_rows(int B, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad, int dil);
int pp_conv2d_fwd_stats(const float* x, int64_t ldx, int B, int H, int W, int Cin, const float* w, const float* bias,
                        int kh, int kw, int stride, int pad, int dil, float* y, int64_t ldy, int Cout, void* workspace,
                        size_t ws_bytes, float* stats, size_t stats_floats, pp_stream_t stream);
int pp_bn_train_fwd_partials(const float* x, int64_t ldx, int64_t M, int C, const float* stats, int64_t stat_rows, const float* gamma,
                             const float* beta, float eps, float momentum, float* running_mean, float* running_var, float* mean,
                             float* invstd, const float* residual, int64_t ldr, int act, float drop_p, uint64_t drop_seed,
                             const uint64_t* drop_seed_dev, float* y, int64_t ldy, pp_stream_t stream);

/* Depthwise 3x3 convolution + training-mode BatchNorm (+ residual) + activation in ONE launch (mobilenet_v2.py:38-40, 52-54):
 * the single-launch BatchNorm computes the convolution in its statistics pass, writes it to x_out [B,Ho,Wo,C] (BatchNorm's
 * input, needed by the backward pass) and applies the normalisation from there.  Bit-identical to pp_dwconv3x3_fwd followed
 * by pp_bn_train_fwd_fused.  workspace / sync as pp_bn_train_fwd_fused (fine-grained memory). */
int pp_dwconv3x3_bn_train_fwd_fused(const float* in, int64_t ld_in, int B, int H, int W, int C, const float* w, int stride, int pad,
                                    int dil, float* x_out, int64_t ldx, const float* gamma, const float* beta, float eps,
                                    float momentum, float* running_mean, float* running_var, float* mean, float* invstd,
                                    const float* residual, int64_t ldr, int act, float* y, int64_t ldy, void* workspace,
                                    size_t ws_bytes, int32_t* sync, size_t sync_ints, pp_stream_t stream);

/* Single-launch form of pp_bn_bwd (same arguments + sync).  grad_scale = 1/(1-p) when a dropout was fused into the
 * forward (its mask is recovered from y_act == 0), else 1.  y_act == NULL with beta != NULL (no residual, no dropout):
 * the ReLU/ReLU6 mask is recomputed from x with the forward's own fma (bit-identical), y_act is not read. */
int pp_bn_bwd_fused(const float* x, int64_t ldx, const float* dy, int64_t lddy, const float* y_act, int64_t ldya, int act,
                    int64_t M, int C, const float* mean, const float* invstd, const float* gamma, float* dgamma,
                    float* dbeta, float* dx, int64_t lddx, float* dres, int64_t lddr, float grad_scale, const float* beta,
                    void* workspace, size_t ws_bytes, int32_t* sync, size_t sync_ints, pp_stream_t stream);

/* Sparse output gradients.  The loss of a sparsely labelled batch (model.py:113-119: 20 labelled pixels per image, ignore_index
 * elsewhere) has a gradient that is zero in all but a few hundred of the 32768 low-resolution rows.  pp_row_flags marks the non-zero
 * rows of a [M, C] gradient (flags[r] = 1 when any entry of row r is non-zero); pp_conv1x1_bwd_data_sparse is the backward-data of a
 * pointwise convolution (w: HWIO of a 1x1 kernel = [Cin][Cout]) that writes zeros for the unflagged rows of dx and computes the flagged
 * ones; pp_bn_bwd_fused_sparse is pp_bn_bwd_fused told that the unflagged rows of dy are exact zeros: its statistics pass visits only
 * the flagged rows (in the dense kernel's order: dgamma / dbeta / dx are bit-equal to pp_bn_bwd_fused on the same dy) and its dx pass
 * never reads dy elsewhere.  A row cache variant of the kernel (small maps) ignores the flags. */
int pp_row_flags(const float* dy, int64_t lddy, int64_t M, int C, unsigned char* flags, pp_stream_t stream);
/* The weight (and, dbias != NULL, bias) gradient of that pointwise convolution over the flagged rows only: dw [Cin][Cout] (HWIO of a 1x1
 * kernel) = sum_r x[r][:]^T dy[r][:], rows in ascending order inside fixed 512-row blocks, blocks in order (deterministic; equal to the
 * dense gradient up to the order of the fp32 additions).  Cin * Cout + Cout <= 8192.  decoders.py:64 / :120 classifiers behind
 * model.py:113-119's sparse labels. */
size_t pp_conv1x1_bwd_weight_sparse_workspace_bytes(int64_t M, int Cin, int Cout);
int pp_conv1x1_bwd_weight_sparse(const float* x, int64_t ldx, int64_t M, int Cin, const float* dy, int64_t lddy, int Cout,
                                 const unsigned char* row_flags, float* dw, float* dbias, void* workspace, size_t ws_bytes, pp_stream_t stream);
int pp_conv1x1_bwd_data_sparse(const float* dy, int64_t lddy, int64_t M, int Cout, const float* w, int Cin, const unsigned char* row_flags,
                             float* dx, int64_t lddx, pp_stream_t stream);
int pp_bn_bwd_fused_sparse(const float* x, int64_t ldx, const float* dy, int64_t lddy, const float* y_act, int64_t ldya, int act,
                         int64_t M, int C, const float* mean, const float* invstd, const float* gamma, float* dgamma,
                         float* dbeta, float* dx, int64_t lddx, float* dres, int64_t lddr, float grad_scale, const float* beta,
                         void* workspace, size_t ws_bytes, int32_t* sync, size_t sync_ints, const unsigned char* row_flags,
                         pp_stream_t stream);

/* nn.BatchNorm2d, eval mode: scale/shift from the running statistics. */
int pp_bn_eval_affine(int C, const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                      float eps, float* scale, float* shift, pp_stream_t stream);

/* y = act(x*scale + shift [+ residual]);  act 0 none, 1 ReLU, 2 ReLU6.  BN apply + nn.ReLU/ReLU6
 * (+ the residual add of mobilenet_v2.py:62-63 / resnet Bottleneck) in one pass. */
int pp_scale_shift_act(const float* x, int64_t ldx, int64_t M, int C, const float* scale, const float* shift,
                       const float* residual, int64_t ldr, int act, float* y, int64_t ldy, pp_stream_t stream);

/* Backward of [BN(train) -> (+residual) -> act]: g = dy * act'(y_act); dgamma, dbeta, dx; dres = g
 * (NULL if no residual).  y_act is the activation OUTPUT (needed when act != 0). */
int pp_bn_bwd(const float* x, int64_t ldx, const float* dy, int64_t lddy, const float* y_act, int64_t ldya, int act,
              int64_t M, int C, const float* mean, const float* invstd, const float* gamma, float* dgamma, float* dbeta,
              float* dx, int64_t lddx, float* dres, int64_t lddr, void* workspace, size_t ws_bytes, pp_stream_t stream);

/* Depthwise 3x3 convolution (groups = C), mobilenet_v2.py:38,52; generic stride / padding / dilation.
 * H, W are always the INPUT spatial size. */
int pp_dwconv3x3_fwd(const float* x, int64_t ldx, int B, int H, int W, int C, const float* w, int stride, int pad, int dil,
                     float* y, int64_t ldy, pp_stream_t stream);

/* Inference form of the depthwise 3x3 -> BatchNorm2d(eval) -> ReLU6 (mobilenet_v2.py:38-40,52-54) in one launch;
 * same epilogue contract as pp_conv2d_fwd_bn_act. */
int pp_dwconv3x3_fwd_bn_act(const float* x, int64_t ldx, int B, int H, int W, int C, const float* w, int stride, int pad,
                            int dil, const float* gamma, const float* beta, const float* running_mean,
                            const float* running_var, float eps, const float* residual, int64_t ldr, int act, float* y,
                            int64_t ldy, pp_stream_t stream);
int pp_dwconv3x3_bwd_data(const float* dy, int64_t lddy, int B, int H, int W, int C, const float* w, int stride, int pad,
                          int dil, float* dx, int64_t lddx, pp_stream_t stream);
int pp_dwconv3x3_bwd_weight(const float* x, int64_t ldx, int B, int H, int W, int C, const float* dy, int64_t lddy,
                            int stride, int pad, int dil, float* dw, void* workspace, size_t ws_bytes, pp_stream_t stream);

/* nn.GroupNorm(G, C) [+ nn.ReLU] (decoders.py:92-94), x [B,P=H*W,C]: statistics per (image, group) over P*(C/G)
 * elements, biased variance, eps inside the sqrt.  mean/rstd [B*G] are outputs of fwd and inputs of bwd; y (the
 * activation output) supplies the ReLU mask in bwd. */
size_t pp_groupnorm_workspace_bytes(int B, int64_t P, int C);
int pp_groupnorm_relu_fwd(const float* x, int64_t ldx, int B, int64_t P, int C, int G, const float* gamma, const float* beta,
                          float eps, int relu, float* y, int64_t ldy, float* mean, float* rstd, void* workspace,
                          size_t ws_bytes, pp_stream_t stream);
int pp_groupnorm_relu_bwd(const float* x, int64_t ldx, const float* dy, int64_t lddy, const float* y, int64_t ldy, int B,
                          int64_t P, int C, int G, const float* mean, const float* rstd, const float* gamma, float* dgamma,
                          float* dbeta, float* dx, int64_t lddx, void* workspace, size_t ws_bytes, pp_stream_t stream);

/* nn.MaxPool2d(ksize, stride, pad) (resnet_models.py:121), torch's first-maximum rule; argmax u8 [B,Ho,Wo,C] holds the
 * winning tap (kh*ksize + kw) and drives the deterministic gather in bwd.  H, W are the INPUT size in both calls. */
int pp_maxpool2d_fwd(const float* x, int64_t ldx, int B, int H, int W, int C, int ksize, int stride, int pad, float* y,
                     int64_t ldy, unsigned char* argmax, pp_stream_t stream);
int pp_maxpool2d_bwd(const float* dy, int64_t lddy, const unsigned char* argmax, int B, int H, int W, int C, int ksize, int stride,
                     int pad, float* dx, int64_t lddx, pp_stream_t stream);

/* fixed_padding (mobilenet_v2.py:15-21): zero-pad [B,H,W,C] to [B,Hp,Wp,C]; and its adjoint
 * y = crop(xp) (+ add), used for the gradient of the padded block input (+ the residual gradient). */
int pp_pad2d(const float* x, int64_t ldx, int B, int H, int W, int C, int pad_top, int pad_left, int Hp, int Wp, float* y,
             int64_t ldy, pp_stream_t stream);
int pp_crop2d_add(const float* xp, int64_t ldxp, int B, int Hp, int Wp, int C, int pad_top, int pad_left, const float* add,
                  int64_t ldadd, float* y, int64_t ldy, int H, int W, pp_stream_t stream);

/* F.interpolate(mode="bilinear") with torch's index arithmetic (deeplab.py:49,55; aspp.py:70;
 * decoders.py:82,101).  align_corners as given; scale_h/scale_w > 0 reproduce the `scale_factor=`
 * call form (decoders.py:101), 0 uses in/out.  out_nchw: y is [B,C,Ho,Wo] contiguous (the model's
 * "pred", deeplab.py:55-56).  Backward is a deterministic gather; dy_nchw likewise. */
int pp_bilinear_fwd(const float* x, int64_t ldx, int B, int H, int W, int C, float* y, int64_t ldy, int Ho, int Wo,
                    int align_corners, float scale_h, float scale_w, int out_nchw, pp_stream_t stream);
/* workspace (optional, may be NULL): B*Ho*W*C floats let up-sampling factors >= 3 run as two separable gathers. */
size_t pp_bilinear_bwd_workspace_bytes(int B, int Ho, int W, int C);
int pp_bilinear_bwd(const float* dy, int64_t lddy, int B, int Ho, int Wo, int C, float* dx, int64_t lddx, int H, int W,
                    int align_corners, float scale_h, float scale_w, int dy_nchw, void* workspace, size_t ws_bytes,
                    pp_stream_t stream);

/* out[b][c] = mul * sum_p x[b][p][c]  (nn.AdaptiveAvgPool2d(1), aspp.py:54, with mul = 1/P; also the
 * adjoint of the broadcast below) and y[b][p][c] = mul * v[b][c] (the 1x1 -> HxW bilinear broadcast of
 * aspp.py:70, and the adjoint of the pool). */
int pp_image_colsum(const float* x, int64_t ldx, int B, int64_t P, int C, float mul, float* out, int64_t ldo, pp_stream_t stream);
int pp_image_broadcast(const float* v, int64_t ldv, int B, int64_t P, int C, float mul, float* y, int64_t ldy, pp_stream_t stream);

/* nn.Dropout (aspp.py:61; decoders.py:110,114): y = x * keep / (1-p), keep from a counter-based hash of
 * (seed, element index) — the backward pass calls this again on dy with the same seed. */
/* seed_dev (NULL or a device u64): added (hashed) to `seed` when the kernel RUNS, so a launch captured in a hipGraph
 * draws a fresh mask on every replay once the host bumps that word. */
int pp_dropout(const float* x, int64_t ldx, float* y, int64_t ldy, int64_t M, int C, float p, uint64_t seed,
               const uint64_t* seed_dev, pp_stream_t stream);

/* ---- training-time augmentation on the device (datasets/base_dataset.py:48-141) -----------------
 * Images are HWC uint8 RGB (what PIL hands the reference), label maps / query masks [H,W] uint8.  The host builds the
 * resampling tables (pixelpick_amd/augment.py restates libImaging's precompute_coeffs / nearest index rules and torch's
 * nearest rule); the kernels evaluate them bit-exactly: clip8((2^21 + sum px*k) >> 22) per pass.
 *   pp_aug_resample_h   TF.resize(x, BILINEAR), horizontal pass: src [H,W,3] -> dst [H,Wout,3]; bounds [Wout,2] (first
 *                       source column, count), kk [Wout,ksize] 22-bit fixed-point coefficients.
 *   pp_aug_vcrop        vertical pass evaluated only where TF.pad(fill) -> TF.crop(start, size) -> TF.hflip look:
 *                       tmp [h_in, w_rs, 3] -> out [ch,cw,3]; rows/columns beyond (h_rs, w_rs) take the fill colour.
 *   pp_aug_labels       label map through PIL-NEAREST tables (ty, tx), query mask through torch-nearest tables (qy, qx),
 *                       same pad (ignore_index / 0) / crop / flip; y_out int64 [ch,cw], q_out uint8 0/1 (base_dataset.py:114).
 *   pp_aug_jitter       in place; op 0 brightness, 1 contrast, 2 saturation (PIL ImageEnhance blends), 3 hue (PIL RGB->HSV,
 *                       uint8 wrap-around shift, HSV->RGB), 4 RandomGrayscale (convert("L") x3); contrast needs 8 scratch bytes.
 *   pp_aug_blur         cv2.GaussianBlur(img, (ks,ks), sigma) with a host-built float kernel; scratch [H*W*3] floats (the float32
 *                       separable filter cv2 ran for 8-bit images before 3.4.2).
 *   pp_aug_blur_q8      the same call as OpenCV >= 3.4.2 / 4.x computes it for 8-bit images (base_dataset.py:208 today): host-built
 *                       8.8 fixed-point taps summing to 256 (device array), exact integer row pass into scratch [H*W*3] uint16,
 *                       16.16 column pass, round half up; BORDER_REFLECT_101.
 *   pp_aug_to_tensor    TF.normalize(TF.to_tensor(x), mean, std): HWC uint8 -> CHW float32; mean3 / std3 are HOST arrays. */
int pp_aug_resample_h(const uint8_t* src, int H, int W, const int32_t* bounds, const int32_t* kk, int ksize, int Wout, uint8_t* dst,
                      pp_stream_t stream);
int pp_aug_vcrop(const uint8_t* tmp, const int32_t* bounds, const int32_t* kk, int ksize, int h_rs, int w_rs, int start_h, int start_w,
                 int ch, int cw, int flip, int fill_r, int fill_g, int fill_b, uint8_t* out, pp_stream_t stream);
int pp_aug_labels(const uint8_t* y, const uint8_t* q, int W, const int32_t* ty, const int32_t* tx, const int32_t* qy, const int32_t* qx,
                  int h_rs, int w_rs, int start_h, int start_w, int ch, int cw, int flip, int ignore_index, int64_t* y_out,
                  uint8_t* q_out, pp_stream_t stream);
int pp_aug_jitter(uint8_t* img, int64_t n_pixels, int op, float factor, unsigned long long* scratch_sum, pp_stream_t stream);
int pp_aug_blur(uint8_t* img, int H, int W, const float* kernel, int ks, float* scratch, pp_stream_t stream);
int pp_aug_blur_q8(uint8_t* img, int H, int W, const uint16_t* kernel_q8, int ks, uint16_t* scratch, pp_stream_t stream);
int pp_aug_to_tensor(const uint8_t* img, int64_t n_pixels, const float* mean3, const float* std3, float* out, pp_stream_t stream);

/* nn.Dropout2d (mobilenet_v2.py:114-115 on the high-level features in MC-dropout TRAINING, :127,133-134 on the low-level
 * features): x, y [B,P,C] channels-last; one keep/drop draw per (sample, channel) from the hash of (seed, b*C + c).  The
 * backward pass calls it again on dy with the same seed. */
int pp_dropout2d(const float* x, int64_t ldx, float* y, int64_t ldy, int B, int64_t P, int C, float p, uint64_t seed,
                 const uint64_t* seed_dev, pp_stream_t stream);

/* F.cross_entropy(logits, target, ignore_index) (model.py:116) on NCHW logits (plane stride 1 within a
 * class: element (b,c,pix) at b*sB + c*sC + pix): *loss = mean over labelled pixels, *count = their
 * number; dlogits (NULL to skip) = grad_out * (softmax - onehot)/count on labelled pixels, 0 elsewhere,
 * [B,C,HW] contiguous.  grad_out NULL means 1. */
size_t pp_sparse_ce_workspace_bytes(void);
int pp_sparse_ce_fwd_bwd(const float* logits, int B, int C, int64_t HW, int64_t sB, int64_t sC, const int64_t* target,
                         int ignore_index, float* loss, float* count, const float* grad_out, float* dlogits, void* workspace,
                         size_t ws_bytes, pp_stream_t stream);

/* The same loss and its gradient taken straight from the LOW-resolution classifier output, for a model whose last op is
 * deeplab.py:55-56  F.interpolate(low, size=(H,W), mode='bilinear', align_corners):
 *   *loss = F.cross_entropy(F.interpolate(low), target, ignore_index)  (model.py:116),  *count = labelled pixels,
 *   dlow (NULL to skip) f32 [B,h,w,lddx] = grad_out * d loss / d low  (what autograd hands to the classifier conv).
 * low f32 [B,h,w,ldx] channels-last, C valid channels; target i64 [B,H,W].  The labels are scanned once, the class vector
 * is interpolated only at labelled pixels (80 of 524 288 in the BASELINE step) and the backward gathers per low-res
 * pixel in a fixed order (no atomics: bitwise reproducible).  Neither the [B,C,H,W] logits nor their gradient exist.
 * Any class count: up to 64 classes the class vector lives in registers, wider heads walk it from memory in chunks of 64 (the
 * same semantics, the same workspace, the same reproducibility). */
size_t pp_sparse_ce_lowres_workspace_bytes(void);
int pp_sparse_ce_lowres_fwd_bwd(const float* low, int64_t ldx, int B, int C, int h, int w, int H, int W, int align_corners,
                                const int64_t* target, int ignore_index, float* loss, float* count, const float* grad_out,
                                float* dlow, int64_t lddx, void* workspace, size_t ws_bytes, pp_stream_t stream);

/* The two entries above with the arguments a user of model.py:116's call reaches for first when classes are imbalanced:
 *   F.cross_entropy(x, y, weight=class_weight, ignore_index=ignore_index, reduction="mean", label_smoothing=eps)
 * Per labelled pixel i with target y_i:  lp_c = x_c - m - log S,  m = max_c x_c,  S = sum_c expf(x_c - m)  (classes ascending, one
 * running sum, as in the un-weighted kernels);  w = class_weight, NULL = all ones (so smoothing alone works):
 *   A    = sum_i w[y_i] * (-lp_{y_i})                   Bsm = sum_i sum_c w[c] * (-lp_c)   (only when eps > 0)
 *   Wsum = sum_i w[y_i]                                 Wall = sum_c w[c]                  (fp32, classes ascending)
 *   *loss = (1 - eps) * A / Wsum + (eps / C) * Bsm / Wsum,    *wsum = Wsum   (the place of the un-weighted entries' *count)
 *   d loss / d x_c at pixel i = [ (1 - eps) * w[y_i] * (p_c - [c == y_i]) + (eps / C) * (p_c * Wall - w[c]) ] / Wsum
 * dlogits / dlow (NULL: loss only) = grad_out (NULL: 1) times that gradient, chained through the interpolation for the
 * low-resolution entry; fully written, zero wherever no pixel is labelled (pp_row_flags and the sparse backward still apply).
 * A pixel is labelled iff target != ignore_index AND 0 <= target < C: any other target adds to no sum and no gradient, and
 * class_weight (f32 [C], device) is never indexed out of range.  Wsum == 0 (no labelled pixel, or all of them in classes of
 * weight 0) gives a NaN loss, as torch does.  Layouts, lddx, the workspace (pp_sparse_ce_(lowres_)workspace_bytes()), the
 * double-precision fixed-order finalize, the class-count dispatch (registers up to 64 classes, streamed in chunks of 64 beyond) and
 * the bitwise reproducibility are the un-weighted entries'; with weights all 1.0 and eps 0 the outputs equal theirs bit for bit
 * (up to the sign of a zero).
 * Errors: PP_ERR_BAD_ARG  a NULL among logits / low, target, loss, wsum; a shape below 1, ldx < C, lddx < C with dlow;
 *                         label_smoothing outside [0, 1] or NaN - all before anything is enqueued;
 *         PP_ERR_WORKSPACE   workspace NULL or smaller than the query's answer;
 *         PP_ERR_UNSUPPORTED more than 65535 chunks of 64 classes;  PP_ERR_LAUNCH a failed launch. */
int pp_sparse_ce_weighted_fwd_bwd(const float* logits, int B, int C, int64_t HW, int64_t sB, int64_t sC, const int64_t* target,
                                  int ignore_index, const float* class_weight, float label_smoothing, float* loss, float* wsum,
                                  const float* grad_out, float* dlogits, void* workspace, size_t ws_bytes, pp_stream_t stream);
int pp_sparse_ce_lowres_weighted_fwd_bwd(const float* low, int64_t ldx, int B, int C, int h, int w, int H, int W, int align_corners,
                                         const int64_t* target, int ignore_index, const float* class_weight, float label_smoothing,
                                         float* loss, float* wsum, const float* grad_out, float* dlow, int64_t lddx, void* workspace,
                                         size_t ws_bytes, pp_stream_t stream);

/* Step metrics on the device (model.py:124-125,194-196 + utils/metrics.py:168-177): hist[t*C + argmax_c logits] += 1
 * for every pixel whose target t is in [0, C) (ignore_index >= C is skipped like RunningScore._fast_hist).  hist is
 * an int64 [C,C] accumulator the caller zeroes / reads (C*C*8 bytes D2H instead of two full maps).
 * C in [1, 256] (else PP_ERR_UNSUPPORTED): up to 104 classes count in block-private LDS counters, wider heads aggregate equal
 * (target, prediction) pairs inside each wave and add them to hist with integer atomics.  Exact counts either way. */
int pp_confusion_matrix_update(const float* logits, int B, int C, int64_t HW, int64_t sB, int64_t sC, const int64_t* target,
                               int64_t* hist, pp_stream_t stream);

/* The same histogram from two LABEL maps: stands in for
 *   utils/metrics.py:168-177  RunningScore._fast_hist / update(label_trues, label_preds)
 *   model.py:124-125,196-199  ... running_score.update(y, pred)          where pred already is a label map on the device
 * (pp_predict_lowres writes one: a head too wide for its LDS histogram takes its label map here, one byte per pixel between the
 * two launches).
 *   pred     u8 [n] predicted labels;  target [n] labels, target_kind 1 uint8, 2 int64 (pp_predict_lowres's meaning)
 *   hist     i64 [C,C], ACCUMULATED into: hist[t*C + pred] += 1 where 0 <= t < C; pixels with pred >= C are not counted
 * C in [1, 256] (else PP_ERR_UNSUPPORTED); nulls, another target_kind or n < 0: PP_ERR_BAD_ARG; n == 0: PP_OK without a launch.
 * Integer counts only: reproducible run to run. */
int pp_confusion_matrix_from_labels(const uint8_t* pred, const void* target, int target_kind, int64_t n, int C, int64_t* hist,
                                    pp_stream_t stream);

/* The label map and the step metrics straight from the LOW-resolution classifier output: replaces, in one launch and without
 * materialising the full-resolution logits,
 *   deeplab.py:55-56          pred = F.interpolate(pred, size=inputs.shape[2:], mode='bilinear', align_corners=True)
 *   model.py:124-125,196-199  prob.argmax(dim=1) ... running_score.update(y, pred)      eval.py:60-63 the same in evaluate()
 *   utils/metrics.py:168-177  RunningScore._fast_hist / update
 *   low      f32 [B,h,w,ldx] channels-last classifier output, C valid channels; (H,W) the size interpolated to, (Hc,Wc) <= (H,W)
 *            the top-left crop kept (VOC); scales and arithmetic are pp_acq_lowres_score_topk's, i.e. pp_bilinear_fwd's bits
 *   target   [B,Hc,Wc] labels, target_kind 0 none (NULL), 1 uint8, 2 int64
 *   pred     u8 [B,Hc,Wc] or NULL: the FIRST maximum over the classes of every interpolated pixel (C <= 256)
 *   hist     i64 [C,C] or NULL, ACCUMULATED into: hist[t*C + argmax] += 1 where 0 <= t < C (labels >= C, 255, negative: ignored);
 *            needs target; C <= 104 (block-private LDS counters; a wider head takes pred and pp_confusion_matrix_from_labels)
 * At least one of pred / hist.  Integer counts only: reproducible run to run.  Equal bit for bit to pp_bilinear_fwd followed by
 * argmax / pp_confusion_matrix_update (tested). */
int pp_predict_lowres(const float* low, int64_t ldx, int64_t B, int64_t C, int64_t h, int64_t w, int64_t H, int64_t W,
                      int align_corners, int64_t Hc, int64_t Wc, const void* target, int target_kind, uint8_t* pred,
                      int64_t* hist, pp_stream_t stream);

/* The per-epoch picture's byte panels straight from the LOW-resolution classifier output: replaces, in two launches and without
 * the full-resolution logits, their softmax or any float map on the host,
 *   deeplab.py:55-56        F.interpolate(pred, size, mode='bilinear', align_corners=True)
 *   model.py:124,150-156    softmax / argmax / the three _query maps of one image (margin negated)
 *   utils/utils.py:394-417  Visualiser._preprocess: palette lookup, min-max normalisation to bytes
 * (the resize to half size, the grid and the PNG stay with the caller: utils/utils.py:418-432).
 *   low, ldx, B, C, h, w, H, W, align_corners, Hc, Wc   exactly pp_predict_lowres's meaning and validation; C <= PP_ACQ_MAX_CLASSES
 *            (wider heads: PP_ERR_UNSUPPORTED)
 *   image    f32 [B,3,Hc,Wc] or NULL, element (n,c,y,x) at n*image_sn + c*image_sc + y*image_sr + x
 *   target   [B,Hc,Wc] labels or NULL, target_kind 0 none, 1 uint8, 2 int64
 *   palette  device u8 [256][3]
 *   rgb      u8 [B][n_rgb][Hc][Wc][3], every panel contiguous, in the order: input (if image), target (if target), prediction
 *            input       one (min, max) over all three channels, written HWC
 *            target      palette[label] for 0 <= label <= 255, black otherwise (the reference raises KeyError for a label its
 *                        palette dict lacks)
 *            prediction  palette[first maximum of the interpolated logits]: the label pp_predict_lowres writes
 *   gray     u8 [B][3][Hc][Wc]: least confidence, -|p1 - p2| (the negated margin model.py:155 passes), entropy - the values
 *            pp_acq_lowres_score_topk writes to its score map in its default scorer form (the same device function)
 *   ranges   f32 [B][4][2] or NULL: (min, max) of input, confidence, negated margin, entropy as used below ((0, 0) without image)
 * A float panel v becomes bytes, per image and in fp32 with every operation rounded on its own, as torch does on the CPU:
 *   mn = min v ; t = v - mn ; d = max(t) + 1e-7f ; byte = trunc(clamp((t / d) * 255.0f, 0, 255))
 * min and max skip NaN (entropy is NaN where a probability underflows: 0 * log 0) and a NaN pixel becomes 0; the reference's
 * min() would be NaN there and blank the whole panel.  All outputs are fully overwritten; no atomics: reproducible run to run.
 * workspace: pp_vis_lowres_workspace_bytes(B, Hc, Wc) bytes (0 for sizes no launch would accept); too small: PP_ERR_WORKSPACE. */
size_t pp_vis_lowres_workspace_bytes(int64_t B, int64_t Hc, int64_t Wc);
int pp_vis_lowres(const float* low, int64_t ldx, int64_t B, int64_t C, int64_t h, int64_t w, int64_t H, int64_t W,
                  int align_corners, int64_t Hc, int64_t Wc, const float* image, int64_t image_sn, int64_t image_sc,
                  int64_t image_sr, const void* target, int target_kind, const uint8_t* palette, uint8_t* rgb, uint8_t* gray,
                  float* ranges, void* workspace, size_t ws_bytes, pp_stream_t stream);

/* torch.optim.Adam step on flat buffers (utils/utils.py:125-141): elements [0,n_split) use lr_a (the
 * backbone/encoder group at lr/10), the rest lr_b; L2 weight decay; `step` is 1-based; grads are
 * multiplied by grad_scale first (1/world_size after the gradient all-reduce). */
/* hyper_dev (NULL or device f32[4] = {lr_a, lr_b, 1-beta1^step, sqrt(1-beta2^step)}): when given, these four
 * replace the by-value arguments at RUN time, so the launch can be replayed from a hipGraph with a moving step. */
int pp_adam_step_flat(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, int64_t n_split,
                      float lr_a, float lr_b, float beta1, float beta2, float eps, float weight_decay, int64_t step,
                      float grad_scale, const float* hyper_dev, pp_stream_t stream);

/* torch.optim.SGD(momentum, weight_decay) on flat buffers with the same two-segment learning rate: the optimiser the
 * reference builds for voc and for optimizer_type "SGD" (utils/utils.py:208-270: lr 1e-3 backbone/encoder, 1e-2 the
 * rest, momentum 0.9, weight decay 5e-4 / 1e-4).  step == 1 initialises the momentum buffer with the gradient, as
 * torch does.  hyper_dev (optional): [lr_a, lr_b] read at run time. */
int pp_sgd_step_flat(float* params, const float* grads, float* momentum_buf, int64_t n, int64_t n_split, float lr_a, float lr_b,
                     float momentum, float weight_decay, int64_t step, float grad_scale, const float* hyper_dev,
                     pp_stream_t stream);

/* y = a + b on [M,C] matrices with pixel strides (gradient accumulation for tensors with several
 * consumers: the residual input of mobilenet_v2.py:62, the ASPP input of aspp.py:64-69). */
int pp_add2d(const float* a, int64_t lda, const float* b, int64_t ldb, float* y, int64_t ldy, int64_t M, int C, pp_stream_t stream);

/* [B,C,H,W] -> [B,H,W,C] (the network input; deeplab.py:43 receives NCHW). */
int pp_nchw_to_nhwc(const float* x, int B, int C, int64_t HW, float* y, int64_t ldy, pp_stream_t stream);
/* [B,H,W,C] (pixel stride ldx) -> [B,C,H,W] contiguous: the FPN model's "pred"/"emb" outputs (decoders.py:77). */
int pp_nhwc_to_nchw(const float* x, int64_t ldx, int B, int C, int64_t HW, float* y, pp_stream_t stream);

/* Blocks of the single-launch BatchNorm kernels that fit on the device at once (occupancy x CUs; 0 = no device).  A launch
 * uses at most half of it, so that two spin-waiting launches (second stream / second process) are always co-resident. */
int pp_bn_fused_capacity(void);
/* Measurement yardsticks (stateless launches; bench.py reports the product kernels against them).
 * pp_yardstick_stream_read: a kernel that only reads `bytes` of x (float4 per lane, `blocks` blocks of 256 threads, 0 = 256;
 * blocks < 0: -blocks blocks, non-temporal loads) - acq_kernel's bandwidth is quoted against what this reaches on the same buffer.
 * pp_yardstick_mfma_stream: conv_x3_kernel's MFMA stream from registers only; data_kind 0 zeros, 1 near-constant, 2 random operands. */
int pp_yardstick_stream_read(const void* x, size_t bytes, int blocks, float* sink, pp_stream_t stream);
int pp_yardstick_mfma_stream(int data_kind, int iters, float* sink, pp_stream_t stream);

/* The A/B and ablation switches of earlier rounds (process-global planner state, `pp_debug_*`) are NOT part of this library: they exist
 * only in the test build, libpixelpick_hip_knobs.so (same sources + -DPP_DEBUG_KNOBS, see pixelpick_hip_knobs.h); `nm -D` of
 * libpixelpick_hip.so shows none of them, and its planners run on their compiled-in defaults. */
#ifdef PP_DEBUG_KNOBS
#include "pixelpick_hip_knobs.h"
#endif

/* ---------------------------------------------------------------------------------------------
 * Launch plans: the train step of model.py:101-122 (model.train(); forward; cross_entropy; backward; optimizer.step()) as ONE
 * foreign call.  The reference re-runs that Python per iteration (model.py:106 loop); with static shapes every C-ABI call of
 * a step repeats with identical arguments, so the host records them once and this executor re-issues them (csrc/plan.hip).
 * A recorded call goes through its entry point again - same planning, kernels, queues and results as the eager call.
 *
 *   pp_plan_add_call       fn = address of one of this library's enqueuing entry points; slots = its arguments, one 8-byte
 *                          slot each (integers sign-extended, pointers as addresses, float in the low 4 bytes);
 *                          PP_ERR_UNSUPPORTED for any other address, PP_ERR_BAD_ARG when n_slots is not its arity
 *                          (pp_plan_entry_args(fn), -1 = not an entry point).
 *   pp_plan_add_event_record / _stream_wait    hipEventRecord(event, stream) / hipStreamWaitEvent(stream, event):
 *                          the fork of the weight-gradient queue; caller-owned hipEvent_t.
 *   pp_plan_add_join       `waiting` waits for everything enqueued on `waited_for` so far (plan-owned event).
 *   pp_plan_add_host_break pp_plan_replay returns here so that the caller can act (the gradient all-reduce of a data-parallel
 *                          step, trainer.py) and resume.
 *   pp_plan_replay         issues ops [from, ...) until the end or the next host break; *next = index to resume from
 *                          (== pp_plan_size: finished).  Returns the failing entry point's code (then *next = its index).
 * The plan stores addresses only: every buffer, stream and event it names must outlive it. */
typedef void* pp_plan_t;
pp_plan_t pp_plan_create(void);
void pp_plan_destroy(pp_plan_t plan);
int64_t pp_plan_size(pp_plan_t plan);
int pp_plan_entry_args(const void* fn);
int pp_plan_add_call(pp_plan_t plan, const void* fn, const uint64_t* slots, int n_slots);
int pp_plan_add_event_record(pp_plan_t plan, void* event, pp_stream_t stream);
int pp_plan_add_stream_wait(pp_plan_t plan, pp_stream_t stream, void* event);
int pp_plan_add_join(pp_plan_t plan, pp_stream_t waiting, pp_stream_t waited_for);
int pp_plan_add_host_break(pp_plan_t plan);
int pp_plan_replay(pp_plan_t plan, int64_t from, int64_t* next);

/* Data-parallel training (trainer.py: RCCL all-reduce of the flat gradient under the backward pass): `cus` compute units are set
 * aside for the communication kernel that stays resident meanwhile.  Launches whose blocks wait for each other (the single-launch
 * BatchNorm kernels, convolution + BatchNorm in one launch) size themselves against occupancy x (CUs - cus); shapes that no longer
 * fit take their multi-launch form.  Default 0, or PIXELPICK_COMM_CU_RESERVE at load time.  Changes the launch plans: set it before
 * the first step. */
void pp_set_comm_cu_reserve(int cus);
int pp_get_comm_cu_reserve(void);
/* Profiling hook for bench.py: `starts`/`stops` are HOST arrays of n caller-created hipEvent_t.  The
 * i-th launch of a dominant kernel (acq_kernel, conv_igemm_kernel) after this call records starts[i] / stops[i] on its
 * stream immediately before / after the launch.  Pass (NULL, NULL, 0) to switch off.  The arrays must
 * stay alive until then.  Process-global and meant for ONE measuring thread (the only state besides pp_set_comm_cu_reserve that a call
 * can leave behind in this library). */
void pp_set_kernel_events(void** starts, void** stops, int n);

#ifdef __cplusplus
}
#endif
#endif /* PIXELPICK_HIP_H */
