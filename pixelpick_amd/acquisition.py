"""Host-side functional API over the acquisition entry points of the C ABI.

Everything here only marshals torch device tensors (pointers, strides, current stream) into
include/pixelpick_hip.h calls; all arithmetic runs in the hand-written HIP kernels (csrc/acq.hip: the
full-size scorers; csrc/acq_lowres.hip: the scorers on the classifier-resolution logits; csrc/acq_mc.hip: the MC-dropout families;
csrc/acq_topk.hip: the ranking of a score map; csrc/acq_select.hip: the selectors that run after it).
"""
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib

STRATEGY_ID = {"entropy": 0, "least_confidence": 1, "margin_sampling": 2, "margin": 2}
# "random" (query.py:242-244) has no score kernel: its map is host RNG output (torch.rand on the CPU, as the reference);
# only its exclusion fill / top-k direction are listed here and the selection itself runs through topk_select().
LARGEST = {"entropy": True, "least_confidence": True, "margin_sampling": False, "margin": False, "random": False}
FILL = {"entropy": 0.0, "least_confidence": 0.0, "margin_sampling": 1.0, "margin": 1.0, "random": 1.0}


def strategy_id(strategy: str) -> int:
    try:
        return STRATEGY_ID[strategy]
    except KeyError:
        raise ValueError(f"no score kernel for query strategy {strategy!r} (kernels: {sorted(STRATEGY_ID)}; 'random' maps "
                         f"come from the host RNG and go through topk_select)") from None


def _require_cuda_f32(t: torch.Tensor, name: str, ndim: int):
    if not isinstance(t, torch.Tensor) or t.ndim != ndim:
        raise ValueError(f"{name} must be a {ndim}-d tensor")
    if not t.is_cuda:
        raise _lib.PixelPickHipError(f"{name} must live on the GPU: the HIP path has no CPU fallback")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {t.dtype}")


def _mask_u8(exclude, device):
    """An exclusion mask (numpy or tensor; bool, uint8 or anything compared with 0) as uint8 on the device, in its own shape."""
    if isinstance(exclude, np.ndarray):
        exclude = np.ascontiguousarray(exclude)       # also resolves negative strides (flipped views)
    ex = torch.as_tensor(exclude)
    if ex.dtype == torch.bool:
        # reinterpret, do not convert: a torch CPU op on a 131 K-element mask costs milliseconds on a many-core host
        # (OpenMP fork/join per op) - it was 90 % of the per-image time of an acquisition round
        ex = ex.contiguous().view(torch.uint8)
    elif ex.dtype != torch.uint8:
        ex = (ex != 0).contiguous().view(torch.uint8)
    return ex.to(device, non_blocking=True)


def _exclude_u8(exclude, B, H, W, device):
    return None if exclude is None else _mask_u8(exclude, device).reshape(B, H, W).contiguous()


# ---- the pool the selectors after the ranking work on: a rank-ordered list per image, an exclusion mask, idx / pos / n out ----
def _pool_cand(cand):
    """The list argument of every selector, int32 [B,M] on the GPU -> (cand contiguous, B, M, device)."""
    if not isinstance(cand, torch.Tensor) or cand.ndim != 2 or cand.dtype != torch.int32:
        raise ValueError("cand must be a 2-d int32 tensor [B,M]")
    if not cand.is_cuda:
        raise _lib.PixelPickHipError("cand must live on the GPU: the HIP path has no CPU fallback")
    return (cand.contiguous(), *cand.shape, cand.device)


def _pool_exclude(exclude, B, device, n_pixels=None, whose="n_pixels ="):
    """The selectors' exclusion mask and pixel count -> (uint8 [B,N] on the device or None, N).  N is n_pixels where the caller knows
    it (`whose` names its source in the message), else the mask's entries per image, else 2^31 - 1: no bound on the indices is known."""
    N = None if n_pixels is None else int(n_pixels)
    if exclude is None:
        return None, 0x7FFFFFFF if N is None else N
    ex = _mask_u8(exclude, device)
    if ex.ndim == 0 or ex.shape[0] != B:
        raise ValueError(f"exclude must be [B, ...] with B = {B} images, got {tuple(ex.shape)}")
    ex = ex.reshape(B, -1).contiguous()
    if N is not None and ex.shape[1] != N:
        raise ValueError(f"exclude holds {ex.shape[1]} pixels per image, {whose} {N}")
    return ex, ex.shape[1]


def _pool_out(B, k, device, lists=2):
    """`lists` int32 [B,k] tensors (idx, pos, ...) and n int32 [B] for a selector's picks."""
    return [torch.empty((B, max(k, 0)), dtype=torch.int32, device=device) for _ in range(lists)] + \
           [torch.empty((B,), dtype=torch.int32, device=device)]


def _ws(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


REFERENCE_ORDER = 0x100      # PP_ACQ_REFERENCE_ORDER (include/pixelpick_hip.h): OR-ed into the strategy id of one call


def score_topk(logits: torch.Tensor, exclude, strategy: str, k: int, return_map: bool = False, reference_order: bool = False
               ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """softmax -> score -> exclusion -> per-image top-k in one pass (query.py:190-204,57-61).
    reference_order: score in query.py:190,230's own operation order (p = exp(x - m) / S, then sum(-p log p)) instead of the
    default algebraic form - a per-call flag, about half the rate.

    logits [B,C,H,W] f32 on the GPU with any strides (NCHW, channels_last, cropped view).
    Returns (idx int32 [B,k] flat h*W+w value-sorted, val f32 [B,k], map f32 [B,H,W] | None).
    """
    _require_cuda_f32(logits, "logits", 4)
    B, C, H, W = logits.shape
    L = _lib.lib()
    dev = logits.device
    ex = _exclude_u8(exclude, B, H, W, dev)
    idx = torch.empty((B, k), dtype=torch.int32, device=dev)
    val = torch.empty((B, k), dtype=torch.float32, device=dev)
    omap = torch.empty((B, H, W), dtype=torch.float32, device=dev) if return_map else None
    nbytes = L.pp_acq_workspace_bytes(B, C, H, W, k)
    ws = _ws(nbytes, dev)
    sB, sC, sH, sW = logits.stride()
    with torch.cuda.device(dev):
        rc = L.pp_acq_score_topk(logits.data_ptr(), B, C, H, W, sB, sC, sH, sW,
                                 ex.data_ptr() if ex is not None else None,
                                 strategy_id(strategy) | (REFERENCE_ORDER if reference_order else 0), k,
                                 idx.data_ptr(), val.data_ptr(), omap.data_ptr() if omap is not None else None,
                                 ws.data_ptr(), ws.numel(), _lib.current_stream_ptr(dev))
    _lib.check(rc, "pp_acq_score_topk")
    return idx, val, omap


def score_map(logits: torch.Tensor, exclude, strategy: str, reference_order: bool = False) -> torch.Tensor:
    """[B,C,H,W] logits -> [B,H,W] uncertainty map after exclusion (query.py:190-201)."""
    _require_cuda_f32(logits, "logits", 4)
    B, C, H, W = logits.shape
    L = _lib.lib()
    dev = logits.device
    ex = _exclude_u8(exclude, B, H, W, dev)
    omap = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    sB, sC, sH, sW = logits.stride()
    with torch.cuda.device(dev):
        rc = L.pp_acq_score_map(logits.data_ptr(), B, C, H, W, sB, sC, sH, sW,
                                ex.data_ptr() if ex is not None else None,
                                strategy_id(strategy) | (REFERENCE_ORDER if reference_order else 0),
                                omap.data_ptr(), _lib.current_stream_ptr(dev))
    _lib.check(rc, "pp_acq_score_map")
    return omap


def uncertainty_from_prob(prob: torch.Tensor, strategy: str) -> torch.Tensor:
    """UncertaintySampler.__call__ on an already-softmaxed tensor (query.py:229-239,246-247)."""
    _require_cuda_f32(prob, "prob", 4)
    B, C, H, W = prob.shape
    L = _lib.lib()
    dev = prob.device
    omap = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    sB, sC, sH, sW = prob.stride()
    with torch.cuda.device(dev):
        rc = L.pp_uncertainty_from_prob(prob.data_ptr(), B, C, H, W, sB, sC, sH, sW, strategy_id(strategy),
                                        omap.data_ptr(), _lib.current_stream_ptr(dev))
    _lib.check(rc, "pp_uncertainty_from_prob")
    return omap


def mc_accumulate_(logits: torch.Tensor, prob_out: Optional[torch.Tensor], uc_out: Optional[torch.Tensor], strategy: str,
                   scale: float, accumulate: bool = True):
    """MC-dropout accumulation (query.py:181-187) in one kernel pass over logits [T,C,H,W]: prob_out [C,H,W] (+)= scale *
    sum_t softmax(logits[t]), uc_out [H,W] (+)= scale * sum_t strategy-score(softmax(logits[t])).  Either may be None."""
    _require_cuda_f32(logits, "logits", 4)
    T, C, H, W = logits.shape
    for t, shape in ((prob_out, (C, H, W)), (uc_out, (H, W))):
        if t is not None and (tuple(t.shape) != shape or not t.is_contiguous() or t.dtype != torch.float32 or t.device != logits.device):
            raise ValueError(f"output must be a contiguous float32 {shape} tensor on the logits' device")
    sT, sC, sH, sW = logits.stride()
    sid = strategy_id(strategy) if uc_out is not None else 0
    with torch.cuda.device(logits.device):
        rc = _lib.lib().pp_acq_softmax_sum(logits.data_ptr(), T, C, H, W, sT, sC, sH, sW,
                                           prob_out.data_ptr() if prob_out is not None else None,
                                           uc_out.data_ptr() if uc_out is not None else None, sid, float(scale),
                                           int(bool(accumulate)), _lib.current_stream_ptr(logits.device))
    _lib.check(rc, "pp_acq_softmax_sum")


def topk_select(scores: torch.Tensor, k: int, largest: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """scores [B,N] f32 -> (idx int32 [B,k], val f32 [B,k]); uc_map.flatten().topk (query.py:57-61)."""
    _require_cuda_f32(scores, "scores", 2)
    scores = scores.contiguous()
    B, N = scores.shape
    L = _lib.lib()
    dev = scores.device
    idx = torch.empty((B, k), dtype=torch.int32, device=dev)
    val = torch.empty((B, k), dtype=torch.float32, device=dev)
    ws = _ws(L.pp_topk_workspace_bytes(B, N, k), dev)
    with torch.cuda.device(dev):
        rc = L.pp_topk_select(scores.data_ptr(), B, N, k, int(bool(largest)), idx.data_ptr(), val.data_ptr(),
                              ws.data_ptr(), ws.numel(), _lib.current_stream_ptr(dev))
    _lib.check(rc, "pp_topk_select")
    return idx, val


# ---- acquisition from the low-resolution classifier output -------------------------------
def _lowres_geom(low: torch.Tensor, size, crop):
    _require_cuda_f32(low, "low", 4)
    if low.stride(3) != 1 or low.stride(1) != low.shape[2] * low.stride(2) or low.stride(0) != low.shape[1] * low.stride(1):
        raise ValueError("low must be a dense channels-last [B,h,w,C] tensor (a channel slice of one is fine)")
    B, h, w, C = low.shape
    H, W = int(size[0]), int(size[1])
    Hc, Wc = (H, W) if crop is None else (int(crop[0]), int(crop[1]))
    return B, h, w, C, low.stride(2), H, W, Hc, Wc


def score_topk_lowres(low: torch.Tensor, size, exclude, strategy: str, k: int, crop=None, align_corners: bool = True,
                      return_map: bool = False) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor], Optional[torch.Tensor]]:
    """F.interpolate(low, size, 'bilinear', align_corners)[:, :, :crop_h, :crop_w] -> softmax -> score -> exclusion ->
    top-k in ONE launch, never writing the full-resolution logits (deeplab.py:55-56 + query.py:190-204,57-61).

    low [B,h,w,C] f32 channels-last on the GPU (the classifier output as the engine keeps it).  Returns
    (idx int32 [B,k] flat y*crop_w+x, val f32 [B,k], map f32 [B,crop_h,crop_w] | None); k == 0 -> (None, None, map)."""
    B, h, w, C, ldx, H, W, Hc, Wc = _lowres_geom(low, size, crop)
    L = _lib.lib()
    dev = low.device
    ex = _exclude_u8(exclude, B, Hc, Wc, dev)
    want_map = return_map or k == 0
    idx = torch.empty((B, k), dtype=torch.int32, device=dev) if k else None
    val = torch.empty((B, k), dtype=torch.float32, device=dev) if k else None
    omap = torch.empty((B, Hc, Wc), dtype=torch.float32, device=dev) if want_map else None
    ws = _ws(L.pp_acq_lowres_workspace_bytes(B, C, Hc, Wc, k), dev) if k else None
    with torch.cuda.device(dev):
        rc = L.pp_acq_lowres_score_topk(low.data_ptr(), ldx, B, C, h, w, H, W, int(bool(align_corners)), Hc, Wc,
                                        ex.data_ptr() if ex is not None else None, strategy_id(strategy), k,
                                        idx.data_ptr() if k else None, val.data_ptr() if k else None,
                                        omap.data_ptr() if omap is not None else None,
                                        ws.data_ptr() if k else None, ws.numel() if k else 0, _lib.current_stream_ptr(dev))
    _lib.check(rc, "pp_acq_lowres_score_topk")
    return idx, val, omap


def score_at_lowres(low: torch.Tensor, size, img_idx, pix_idx, strategy: str = "entropy", crop=None,
                    align_corners: bool = True) -> torch.Tensor:
    """The strategy's score (no exclusion) at listed pixels of the interpolated map: pixel i = image img_idx[i], flat
    index pix_idx[i] = y*crop_w + x.  -> f32 [n] on the GPU.  (QueryStats' entropy at the queried pixels, query.py:262-266.)"""
    B, h, w, C, ldx, H, W, Hc, Wc = _lowres_geom(low, size, crop)
    dev = low.device
    ii = torch.as_tensor(img_idx).to(torch.int32).to(dev).contiguous()
    pp = torch.as_tensor(pix_idx).to(torch.int32).to(dev).contiguous()
    if ii.shape != pp.shape or ii.ndim != 1:
        raise ValueError("img_idx and pix_idx must be 1-d and of equal length")
    n = ii.numel()
    out = torch.empty((n,), dtype=torch.float32, device=dev)
    if n == 0:
        return out
    with torch.cuda.device(dev):
        rc = _lib.lib().pp_acq_lowres_score_at(low.data_ptr(), ldx, B, C, h, w, H, W, int(bool(align_corners)), Hc, Wc,
                                               strategy_id(strategy), ii.data_ptr(), pp.data_ptr(), n, out.data_ptr(),
                                               _lib.current_stream_ptr(dev))
    _lib.check(rc, "pp_acq_lowres_score_at")
    return out


# ---- MC-dropout from the low-resolution classifier output (query.py:177-187) -------------------------------------
MC_LOWRES_MAX_CLASSES = 64     # PP_ACQ_MAX_CLASSES (include/pixelpick_hip.h): wider heads are PP_ERR_UNSUPPORTED there


def _mc_geom(low: torch.Tensor, n_passes: int, size, crop):
    T = int(n_passes)
    if isinstance(low, torch.Tensor) and low.ndim == 4 and (T < 1 or low.shape[0] % T != 0):
        raise ValueError(f"low holds {low.shape[0]} entries: not a multiple of n_passes = {n_passes}")
    BT, h, w, C, ldx, H, W, Hc, Wc = _lowres_geom(low, size, crop)
    return BT // T, T, h, w, C, ldx, H, W, Hc, Wc


def mc_score_topk_lowres(low: torch.Tensor, n_passes: int, size, exclude, strategy: str, k: int, crop=None,
                         align_corners: bool = True, return_map: bool = False
                         ) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor], Optional[torch.Tensor]]:
    """score_topk_lowres on the MEAN over n_passes stochastic passes of the strategy's score (query.py:177-187): one launch, no
    full-resolution logits of any pass.

    low [B*n_passes,h,w,C] f32 channels-last on the GPU, image-major (the passes of image b are entries b*n_passes ..
    (b+1)*n_passes - 1).  exclude [B,crop_h,crop_w].  Returns (idx int32 [B,k], val f32 [B,k], map f32 [B,crop_h,crop_w] | None);
    k == 0 -> (None, None, map)."""
    B, T, h, w, C, ldx, H, W, Hc, Wc = _mc_geom(low, n_passes, size, crop)
    L = _lib.lib()
    dev = low.device
    ex = _exclude_u8(exclude, B, Hc, Wc, dev)
    want_map = return_map or k == 0
    idx = torch.empty((B, k), dtype=torch.int32, device=dev) if k else None
    val = torch.empty((B, k), dtype=torch.float32, device=dev) if k else None
    omap = torch.empty((B, Hc, Wc), dtype=torch.float32, device=dev) if want_map else None
    ws = _ws(L.pp_acq_lowres_workspace_bytes(B, C, Hc, Wc, k), dev) if k else None
    with torch.cuda.device(dev):
        rc = L.pp_acq_lowres_mc_score_topk(low.data_ptr(), ldx, B, T, C, h, w, H, W, int(bool(align_corners)), Hc, Wc,
                                           ex.data_ptr() if ex is not None else None, strategy_id(strategy), 1.0 / T, k,
                                           idx.data_ptr() if k else None, val.data_ptr() if k else None,
                                           omap.data_ptr() if omap is not None else None,
                                           ws.data_ptr() if k else None, ws.numel() if k else 0, _lib.current_stream_ptr(dev))
    _lib.check(rc, "pp_acq_lowres_mc_score_topk")
    return idx, val, omap


def mc_score_at_lowres(low: torch.Tensor, n_passes: int, size, img_idx, pix_idx, strategy: str = "entropy", crop=None,
                       align_corners: bool = True) -> torch.Tensor:
    """The strategy's score of the MEAN PROBABILITY over the n_passes passes (no exclusion) at listed pixels: pixel i = image
    img_idx[i], flat index pix_idx[i] = y*crop_w + x.  -> f32 [n] on the GPU.  (QueryStats._get_entropy(query, prob) of the
    MC-dropout branch, query.py:262-264, at the queried pixels only.)"""
    B, T, h, w, C, ldx, H, W, Hc, Wc = _mc_geom(low, n_passes, size, crop)
    dev = low.device
    ii = torch.as_tensor(img_idx).to(torch.int32).to(dev).contiguous()
    pp = torch.as_tensor(pix_idx).to(torch.int32).to(dev).contiguous()
    if ii.shape != pp.shape or ii.ndim != 1:
        raise ValueError("img_idx and pix_idx must be 1-d and of equal length")
    n = ii.numel()
    out = torch.empty((n,), dtype=torch.float32, device=dev)
    if n == 0:
        return out
    with torch.cuda.device(dev):
        rc = _lib.lib().pp_acq_lowres_mc_score_at(low.data_ptr(), ldx, B, T, C, h, w, H, W, int(bool(align_corners)), Hc, Wc,
                                                  strategy_id(strategy), 1.0 / T, ii.data_ptr(), pp.data_ptr(), n, out.data_ptr(),
                                                  _lib.current_stream_ptr(dev))
    _lib.check(rc, "pp_acq_lowres_mc_score_at")
    return out


# ---- MC-dropout HARD vote (args.py:34 --vote_type hard; query.py:31,177-187) ---------------------------------------------
# Every pass votes for its arg-max class (equal logits: the lowest index) and the score is a function of the vote counts
# (include/pixelpick_hip.h, pp_acq_vote_*).  Excluded pixels get VOTE_FILL, not FILL: 0.0 / 1.0 are the scores of unanimous pixels.
MC_VOTE_MAX_PASSES = 255       # the vote counts are bytes
VOTE_FILL = {"entropy": -1.0, "least_confidence": -1.0, "margin_sampling": 2.0, "margin": 2.0}


def _vote_passes(n_passes) -> int:
    T = int(n_passes)
    if T < 1 or T > MC_VOTE_MAX_PASSES:
        raise ValueError(f"hard vote: n_passes = {n_passes} outside [1, {MC_VOTE_MAX_PASSES}] (the vote counts are bytes); "
                         f"there is no fall-back to the soft vote")
    return T


def mc_vote_topk_lowres(low: torch.Tensor, n_passes: int, size, exclude, strategy: str, k: int, crop=None,
                        align_corners: bool = True) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor], torch.Tensor]:
    """mc_score_topk_lowres with the hard vote in place of the mean score: the vote counts of the n_passes passes of the interpolated
    logits -> vote entropy / least-confidence / margin -> VOTE_FILL at excluded pixels -> top-k, one launch.

    low [B*n_passes,h,w,C] f32 channels-last on the GPU, image-major; exclude [B,crop_h,crop_w].  Returns (idx int32 [B,k],
    val f32 [B,k], map f32 [B,crop_h,crop_w]); k == 0 -> (None, None, map)."""
    _vote_passes(n_passes)
    B, T, h, w, C, ldx, H, W, Hc, Wc = _mc_geom(low, n_passes, size, crop)
    L = _lib.lib()
    dev = low.device
    ex = _exclude_u8(exclude, B, Hc, Wc, dev)
    idx = torch.empty((B, k), dtype=torch.int32, device=dev) if k else None
    val = torch.empty((B, k), dtype=torch.float32, device=dev) if k else None
    omap = torch.empty((B, Hc, Wc), dtype=torch.float32, device=dev)
    ws = _ws(L.pp_acq_lowres_workspace_bytes(B, C, Hc, Wc, k), dev) if k else None
    with torch.cuda.device(dev):
        rc = L.pp_acq_lowres_mc_vote_topk(low.data_ptr(), ldx, B, T, C, h, w, H, W, int(bool(align_corners)), Hc, Wc,
                                          ex.data_ptr() if ex is not None else None, strategy_id(strategy), k,
                                          idx.data_ptr() if k else None, val.data_ptr() if k else None, omap.data_ptr(),
                                          ws.data_ptr() if k else None, ws.numel() if k else 0, _lib.current_stream_ptr(dev))
    _lib.check(rc, "pp_acq_lowres_mc_vote_topk")
    return idx, val, omap


def mc_vote_accumulate_(logits: torch.Tensor, votes: torch.Tensor, accumulate: bool = True):
    """votes u8 [C,H,W] (+)= the per-class vote counts of the T passes in logits [T,C,H,W] (any strides, any C), one kernel pass.
    The total over all accumulating calls must stay <= MC_VOTE_MAX_PASSES."""
    _require_cuda_f32(logits, "logits", 4)
    T, C, H, W = logits.shape
    _vote_passes(T)
    if (not isinstance(votes, torch.Tensor) or tuple(votes.shape) != (C, H, W) or not votes.is_contiguous() or votes.dtype != torch.uint8
            or votes.device != logits.device):
        raise ValueError(f"votes must be a contiguous uint8 {(C, H, W)} tensor on the logits' device")
    sT, sC, sH, sW = logits.stride()
    with torch.cuda.device(logits.device):
        rc = _lib.lib().pp_acq_vote_accumulate(logits.data_ptr(), T, C, H, W, sT, sC, sH, sW, votes.data_ptr(),
                                               int(bool(accumulate)), _lib.current_stream_ptr(logits.device))
    _lib.check(rc, "pp_acq_vote_accumulate")


def vote_score_map(votes: torch.Tensor, n_passes: int, exclude, strategy: str) -> torch.Tensor:
    """votes u8 [B,C,H,W] (or [C,H,W]) of n_passes passes each -> the hard-vote score map f32 [B,H,W], VOTE_FILL at excluded pixels."""
    T = _vote_passes(n_passes)
    if isinstance(votes, torch.Tensor) and votes.ndim == 3:
        votes = votes[None]
    if not isinstance(votes, torch.Tensor) or votes.ndim != 4 or votes.dtype != torch.uint8:
        raise ValueError("votes must be a uint8 [B,C,H,W] tensor")
    if not votes.is_cuda:
        raise _lib.PixelPickHipError("votes must live on the GPU: the HIP path has no CPU fallback")
    votes = votes.contiguous()
    B, C, H, W = votes.shape
    dev = votes.device
    ex = _exclude_u8(exclude, B, H, W, dev)
    omap = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().pp_acq_vote_score_map(votes.data_ptr(), B, T, C, H, W, ex.data_ptr() if ex is not None else None,
                                              strategy_id(strategy), omap.data_ptr(), _lib.current_stream_ptr(dev))
    _lib.check(rc, "pp_acq_vote_score_map")
    return omap


# ---- MC-dropout scores of the MEAN PROBABILITY over the passes, and BALD (include/pixelpick_hip.h, pp_acq_mean_prob_score_map) ----
# The consensus of the committee: entropy / least-confidence / margin of pm = mean_t softmax(x_t), and the mutual information
# H(pm) - mean_t H(p_t).  A strategy table of its own: STRATEGY_ID stays closed, so every other entry keeps refusing "bald".
# Excluded pixels get MEAN_FILL (the hard vote's fills): 0.0 is the BALD of every deterministic pixel.
MEAN_STRATEGY_ID = {"entropy": 0, "least_confidence": 1, "margin_sampling": 2, "margin": 2, "bald": 3}
MEAN_LARGEST = {"entropy": True, "least_confidence": True, "margin_sampling": False, "margin": False, "bald": True}
MEAN_FILL = {"entropy": -1.0, "least_confidence": -1.0, "margin_sampling": 2.0, "margin": 2.0, "bald": -1.0}


def mean_strategy_id(strategy: str) -> int:
    try:
        return MEAN_STRATEGY_ID[strategy]
    except KeyError:
        raise ValueError(f"no mean-probability scorer for query strategy {strategy!r} (kernels: {sorted(MEAN_STRATEGY_ID)})") from None


def mc_mean_topk_lowres(low: torch.Tensor, n_passes: int, size, exclude, strategy: str, k: int, crop=None,
                        align_corners: bool = True, return_map: bool = False
                        ) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor], Optional[torch.Tensor]]:
    """mc_score_topk_lowres with the score of the MEAN PROBABILITY over the n_passes passes (strategy "entropy",
    "least_confidence", "margin_sampling") or their mutual information ("bald") in place of the mean score: passes, score,
    MEAN_FILL at excluded pixels and top-k in one launch, no full-resolution logits and no [C,H,W] probability map.

    low [B*n_passes,h,w,C] f32 channels-last on the GPU, image-major; exclude [B,crop_h,crop_w].  Returns (idx int32 [B,k],
    val f32 [B,k], map f32 [B,crop_h,crop_w] | None); k == 0 -> (None, None, map)."""
    sid = mean_strategy_id(strategy)
    B, T, h, w, C, ldx, H, W, Hc, Wc = _mc_geom(low, n_passes, size, crop)
    L = _lib.lib()
    dev = low.device
    ex = _exclude_u8(exclude, B, Hc, Wc, dev)
    want_map = return_map or k == 0
    idx = torch.empty((B, k), dtype=torch.int32, device=dev) if k else None
    val = torch.empty((B, k), dtype=torch.float32, device=dev) if k else None
    omap = torch.empty((B, Hc, Wc), dtype=torch.float32, device=dev) if want_map else None
    ws = _ws(L.pp_acq_lowres_workspace_bytes(B, C, Hc, Wc, k), dev) if k else None
    with torch.cuda.device(dev):
        rc = L.pp_acq_lowres_mc_mean_topk(low.data_ptr(), ldx, B, T, C, h, w, H, W, int(bool(align_corners)), Hc, Wc,
                                          ex.data_ptr() if ex is not None else None, sid, 1.0 / T, k,
                                          idx.data_ptr() if k else None, val.data_ptr() if k else None,
                                          omap.data_ptr() if omap is not None else None,
                                          ws.data_ptr() if k else None, ws.numel() if k else 0, _lib.current_stream_ptr(dev))
    _lib.check(rc, "pp_acq_lowres_mc_mean_topk")
    return idx, val, omap


def mean_prob_score_map(prob: torch.Tensor, mean_ent: Optional[torch.Tensor], exclude, strategy: str) -> torch.Tensor:
    """The same scores from a GIVEN mean probability: prob [B,C,H,W] f32 on the GPU (any strides, any class count; what
    mc_accumulate_ leaves in prob_out) and, for "bald" only, mean_ent [B,H,W] = the mean per-pass entropy (its uc_out with the
    entropy strategy; None for the other strategies) -> f32 [B,H,W], MEAN_FILL at excluded pixels."""
    sid = mean_strategy_id(strategy)
    _require_cuda_f32(prob, "prob", 4)
    B, C, H, W = prob.shape
    dev = prob.device
    if (strategy == "bald") != (mean_ent is not None):
        raise ValueError("mean_ent is required for 'bald' and must be None for every other strategy")
    if mean_ent is not None and (not isinstance(mean_ent, torch.Tensor) or tuple(mean_ent.shape) != (B, H, W) or not mean_ent.is_contiguous()
                                 or mean_ent.dtype != torch.float32 or mean_ent.device != dev):
        raise ValueError(f"mean_ent must be a contiguous float32 {(B, H, W)} tensor on prob's device")
    ex = _exclude_u8(exclude, B, H, W, dev)
    omap = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    sB, sC, sH, sW = prob.stride()
    with torch.cuda.device(dev):
        rc = _lib.lib().pp_acq_mean_prob_score_map(prob.data_ptr(), B, C, H, W, sB, sC, sH, sW,
                                                   mean_ent.data_ptr() if mean_ent is not None else None,
                                                   ex.data_ptr() if ex is not None else None, sid, omap.data_ptr(),
                                                   _lib.current_stream_ptr(dev))
    _lib.check(rc, "pp_acq_mean_prob_score_map")
    return omap


# ---- spread-out picks: a minimum pixel distance between the picks of one image (include/pixelpick_hip.h, pp_spread_select) ----
SPREAD_MAX_PICKS = 1024        # the accepted picks live in LDS: more per image is PP_ERR_UNSUPPORTED


def spread_reach(d: int) -> int:
    """A(d) = #{(dy,dx) in Z^2 : dy^2 + dx^2 < d^2}: the candidates ONE pick can block at minimum distance d, itself included.
    An exact count (integer arithmetic): A(1) = 1, A(2) = 9, A(8) = 193, A(16) = 793."""
    d = int(d)
    if d < 1:
        raise ValueError(f"min_distance = {d}: must be >= 1")
    from math import isqrt
    # row dy holds the dx with dx^2 <= d^2 - 1 - dy^2
    return sum(2 * isqrt(d * d - 1 - dy * dy) + 1 for dy in range(-(d - 1), d))


def spread_candidates(k: int, d: int, N: int) -> int:
    """M = min(N, max(k, (k-1) A(d) + 1)): among the first (k-1) A(d) + 1 un-excluded ranks there is always room for the k-th pick, so
    the greedy pass over the top-M list equals the greedy pass over the whole ranking (as long as the first M ranks hold no excluded
    pixel, i.e. at least M un-excluded pixels score strictly better than the exclusion fill)."""
    k, N = int(k), int(N)
    if k < 1 or N < 1:
        raise ValueError(f"k = {k}, N = {N}: both must be >= 1")
    return min(N, max(k, (k - 1) * spread_reach(d) + 1))


def spread_select(cand: torch.Tensor, width: int, k: int, min_distance: int, exclude=None, n_pixels: Optional[int] = None
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Greedy minimum-distance selection (pp_spread_select): cand int32 [B,M] on the GPU, flat indices y*width + x in RANK order (the
    idx of any *_topk function called with k = M).  Walks the list, skips excluded candidates, accepts one iff it lies >= min_distance
    pixels from every pick accepted so far, stops at k; a list that ends first is topped up with its earliest unaccepted entries.
    exclude: [B, ...] with n_pixels entries per image, or None; n_pixels defaults to exclude's entries per image (without a mask: no
    bound on the indices is known, 2^31 - 1).  A candidate outside [0, n_pixels) counts as excluded.
    Returns (idx int32 [B,k], pos int32 [B,k] = list position of each pick, n int32 [B] = picks that satisfy the distance rule)."""
    cand, B, M, dev = _pool_cand(cand)
    ex, N = _pool_exclude(exclude, B, dev, n_pixels)
    k = int(k)
    idx, pos, n = _pool_out(B, k, dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().pp_spread_select(cand.data_ptr(), B, M, int(width), N, k, int(min_distance),
                                         ex.data_ptr() if ex is not None else None, idx.data_ptr(), pos.data_ptr(), n.data_ptr(),
                                         _lib.current_stream_ptr(dev))
    _lib.check(rc, "pp_spread_select")
    return idx, pos, n


# ---- region-aware acquisition: window impurity x window uncertainty (include/pixelpick_hip.h, pp_acq_region_score_map) ----
REGION_TILE = (64, 64)         # (TH, TW) of region_score_kernel: one block per tile of one image (csrc/acq_select.hip, kRegionTH / kRegionTW)
REGION_MAX_RADIUS = 16
REGION_MODE_ID = {"product": 0, "impurity": 1, "uncertainty": 2}
REGION_FILL = -1.0             # at excluded pixels: 0.0 is the score of every pure window; the largest score wins in every mode
_region_tables = {}


def _region_radius(radius) -> int:
    r = int(radius)
    if r < 1 or r > REGION_MAX_RADIUS:
        raise ValueError(f"radius = {radius} outside [1, {REGION_MAX_RADIUS}]")
    return r


def region_table(radius: int, device) -> torch.Tensor:
    """tab[n] = llrint(n ln(n) 2^16), n = 0 .. (2r+1)^2, computed on the host by pp_acq_region_table: a uint32 tensor on `device`,
    made once per (radius, device) and kept."""
    r = _region_radius(radius)
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.PixelPickHipError("region_table: the table is a device tensor: the HIP path has no CPU fallback")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (r, device.index)
    tab = _region_tables.get(key)
    if tab is None:
        L = _lib.lib()
        host = np.empty(L.pp_acq_region_table_words(r), dtype=np.uint32)
        _lib.check(L.pp_acq_region_table(r, host.ctypes.data), "pp_acq_region_table")
        tab = _region_tables[key] = torch.from_numpy(host).to(device)
    return tab


def region_score_map(pred: Optional[torch.Tensor], unc: Optional[torch.Tensor], radius: int, n_classes: int, exclude=None,
                     mode: str = "product", flip: bool = False) -> torch.Tensor:
    """Per pixel, over its (2 radius + 1)^2 window clipped at the image border: the entropy of the predicted labels P ("impurity"),
    the mean U of unc ("uncertainty"; flip: of 1 - unc, for the margin) or P * U ("product") -> f32 [B,H,W], REGION_FILL at excluded
    pixels, the LARGEST score wins (pp_acq_region_score_map; one launch).

    pred uint8 [B,H,W] (predict_lowres), unc f32 [B,H,W] (score_topk_lowres with k = 0), both contiguous on the GPU; pred may be None
    in mode "uncertainty", unc in mode "impurity".  n_classes in [1, 256]: a label >= n_classes counts in one extra bin."""
    try:
        mid = REGION_MODE_ID[mode]
    except (KeyError, TypeError):
        raise ValueError(f"unknown region mode {mode!r} (modes: {sorted(REGION_MODE_ID)})") from None
    r = _region_radius(radius)
    C = int(n_classes)
    if C < 1 or C > 256:
        raise ValueError(f"n_classes = {n_classes} outside [1, 256] (the labels are bytes)")
    need_pred, need_unc = mid != 2, mid != 1
    if (need_pred and pred is None) or (need_unc and unc is None):
        raise ValueError(f"mode {mode!r} needs {'pred' if pred is None and need_pred else 'unc'}")
    ref = pred if need_pred else unc
    for t, name, dtype in ((pred, "pred", torch.uint8), (unc, "unc", torch.float32)):
        if t is None or not (need_pred if name == "pred" else need_unc):
            continue
        if not isinstance(t, torch.Tensor) or t.ndim != 3:
            raise ValueError(f"{name} must be a 3-d tensor [B,H,W]")
        if not t.is_cuda:
            raise _lib.PixelPickHipError(f"{name} must live on the GPU: the HIP path has no CPU fallback")
        if t.dtype != dtype:
            raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        if t.shape != ref.shape or t.device != ref.device:
            raise ValueError(f"pred {tuple(pred.shape)} on {pred.device} and unc {tuple(unc.shape)} on {unc.device} must agree")
    B, H, W = ref.shape
    dev = ref.device
    ex = _exclude_u8(exclude, B, H, W, dev)
    tab = region_table(r, dev) if need_pred else None
    omap = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().pp_acq_region_score_map(pred.data_ptr() if need_pred else None, unc.data_ptr() if need_unc else None,
                                                B, C, H, W, r, mid, int(bool(flip)), tab.data_ptr() if tab is not None else None,
                                                ex.data_ptr() if ex is not None else None, omap.data_ptr(), _lib.current_stream_ptr(dev))
    _lib.check(rc, "pp_acq_region_score_map")
    return omap


# ---- class-balanced picks: round-robin over the predicted classes of a rank-ordered pool (include/pixelpick_hip.h, pp_class_balance_select) ----
BALANCE_MAX_PICKS = 1024       # one slot counter per round lives in LDS (pp_spread_select's cap): more per image is PP_ERR_UNSUPPORTED


def class_balance_select(cand: torch.Tensor, label: torch.Tensor, k: int, exclude=None
                         ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Round-robin selection over the predicted classes (pp_class_balance_select): cand int32 [B,M] on the GPU, flat pixel indices in
    RANK order (the idx of any *_topk function called with k = M); label uint8 [B, ...] with N entries per image on the same device
    (predict_lowres).  An entry is eligible when it lies in [0, N) and is not excluded; its rank inside its class counts the eligible
    entries of that class in front of it.  The picks are the min(k, eligible) entries smallest in (rank inside the class, list
    position): the best entry of every class in the pool first, then every class's second entry, and so on; a pool with fewer than
    k eligible entries is topped up with its earliest ineligible ones.  exclude: [B, ...] with the same N entries per image, or None.
    Returns (idx int32 [B,k], pos int32 [B,k] = list position of each pick, n int32 [B] = picks of the balanced phase)."""
    cand, B, M, dev = _pool_cand(cand)
    if not isinstance(label, torch.Tensor) or label.ndim < 2 or label.dtype != torch.uint8:
        raise ValueError("label must be a uint8 tensor [B, ...] (the label map predict_lowres writes)")
    if not label.is_cuda or label.device != dev:
        raise _lib.PixelPickHipError("label must live on the GPU with cand: the HIP path has no CPU fallback")
    if label.shape[0] != B:
        raise ValueError(f"label holds {label.shape[0]} images, cand {B}")
    label = label.reshape(B, -1).contiguous()
    ex, N = _pool_exclude(exclude, B, dev, label.shape[1], whose="label")
    k = int(k)
    idx, pos, n = _pool_out(B, k, dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().pp_class_balance_select(cand.data_ptr(), B, M, N, k, label.data_ptr(), ex.data_ptr() if ex is not None else None,
                                                idx.data_ptr(), pos.data_ptr(), n.data_ptr(), _lib.current_stream_ptr(dev))
    _lib.check(rc, "pp_class_balance_select")
    return idx, pos, n


# ---- feature-diverse picks: k-centre greedy over the class probabilities of a rank-ordered pool (include/pixelpick_hip.h, pp_diverse_select) ----
DIVERSE_MAX_PICKS = 1024       # the cap of the other two selectors (pp_spread_select, pp_class_balance_select): more per image is PP_ERR_UNSUPPORTED
DIVERSE_MAX_FEATURES = 256     # bytes of a feature row that enter a distance: one per class of the widest label map


def prob_at_lowres(low: torch.Tensor, size, img_idx, pix_idx, crop=None, align_corners: bool = True, ldf: Optional[int] = None
                   ) -> torch.Tensor:
    """The class probabilities (softmax of the interpolated class vector, the default scorer's arithmetic) at listed pixels, as bytes
    min(255, rint(255 p)): pixel i = image img_idx[i], flat index pix_idx[i] = y*crop_w + x (pp_acq_lowres_prob_at_u8).  ldf: the row
    pitch, a multiple of 4 and at least C (None: C rounded up to 4); bytes C .. ldf-1 are 0, and so is the whole row of an entry
    outside the batch or the crop.  -> uint8 [n, ldf] on the GPU."""
    B, h, w, C, ldx, H, W, Hc, Wc = _lowres_geom(low, size, crop)
    dev = low.device
    ii = torch.as_tensor(img_idx).to(torch.int32).to(dev).contiguous()
    pp = torch.as_tensor(pix_idx).to(torch.int32).to(dev).contiguous()
    if ii.shape != pp.shape or ii.ndim != 1:
        raise ValueError("img_idx and pix_idx must be 1-d and of equal length")
    ldf = (C + 3) // 4 * 4 if ldf is None else int(ldf)
    if ldf < C or ldf % 4:
        raise ValueError(f"ldf = {ldf} must be a multiple of 4 and at least C = {C}")
    n = ii.numel()
    out = torch.empty((n, ldf), dtype=torch.uint8, device=dev)
    if n == 0:
        return out
    with torch.cuda.device(dev):
        rc = _lib.lib().pp_acq_lowres_prob_at_u8(low.data_ptr(), ldx, B, C, h, w, H, W, int(bool(align_corners)), Hc, Wc, ii.data_ptr(),
                                                 pp.data_ptr(), n, out.data_ptr(), ldf, _lib.current_stream_ptr(dev))
    _lib.check(rc, "pp_acq_lowres_prob_at_u8")
    return out


def diverse_select(cand: torch.Tensor, feat: torch.Tensor, k: int, n_features: Optional[int] = None, exclude=None,
                   n_pixels: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """k-centre greedy selection in feature space (pp_diverse_select): cand int32 [B,M] on the GPU, flat pixel indices in RANK order
    (the idx of any *_topk function called with k = M); feat uint8 [B,M,ldf] on the same device, row i the features of list position
    i, of which the first n_features bytes count (None: all ldf).  An entry is eligible when it lies in [0, N) and is not excluded.
    Pick 0 is the earliest eligible entry; every further pick is the eligible entry farthest (sum of squared byte differences) from
    the picks so far, ties to the earliest; a pool with fewer than k eligible entries is topped up with its earliest ineligible ones.
    exclude: [B, ...] with N entries per image, or None.  n_pixels: N, the pixels per image; None: that of exclude, and without
    exclude 2^31 - 1 (every non-negative index is inside).  Returns (idx int32 [B,k], pos int32 [B,k] = list position of each pick, dist int32 [B,k] = squared
    distance to the nearest earlier pick, -1 for pick 0 and the top-up, n int32 [B] = picks of the greedy phase)."""
    cand, B, M, dev = _pool_cand(cand)
    if not isinstance(feat, torch.Tensor) or feat.ndim != 3 or feat.dtype != torch.uint8:
        raise ValueError("feat must be a uint8 tensor [B,M,ldf] (the rows prob_at_lowres writes)")
    if not feat.is_cuda or feat.device != dev:
        raise _lib.PixelPickHipError("feat must live on the GPU with cand: the HIP path has no CPU fallback")
    if feat.shape[0] != B:
        raise ValueError(f"feat holds {feat.shape[0]} images, cand {B}")
    if feat.shape[1] != M:
        raise ValueError(f"feat holds {feat.shape[1]} rows per image, cand {M} list entries")
    feat = feat.contiguous()
    ldf = feat.shape[2]
    F = ldf if n_features is None else int(n_features)
    ex, N = _pool_exclude(exclude, B, dev, n_pixels)
    k = int(k)
    L = _lib.lib()
    idx, pos, dist, n = _pool_out(B, k, dev, lists=3)
    ws = _ws(L.pp_diverse_workspace_bytes(B, M, F), dev)
    with torch.cuda.device(dev):
        rc = L.pp_diverse_select(cand.data_ptr(), B, M, N, k, feat.data_ptr(), F, ldf, ex.data_ptr() if ex is not None else None,
                                 idx.data_ptr(), pos.data_ptr(), dist.data_ptr(), n.data_ptr(), ws.data_ptr(), ws.numel(),
                                 _lib.current_stream_ptr(dev))
    _lib.check(rc, "pp_diverse_select")
    return idx, pos, dist, n
