"""The label map and the confusion matrix straight from the network's low-resolution classifier output.

`predict_lowres` marshals torch device tensors into pp_predict_lowres (csrc/predict.hip): F.interpolate(low, size, 'bilinear')
[:, :, :crop_h, :crop_w] -> argmax over the classes (-> uint8 label map) and, with a target, the RunningScore histogram
(deeplab.py:55-56 + model.py:124-125,196-199 + utils/metrics.py:168-177) in ONE launch that never writes the full-resolution
logits.  All arithmetic runs in the hand-written HIP kernel; there is no CPU fallback.
"""
from typing import Optional, Tuple

import torch

from . import _lib
from .acquisition import _lowres_geom

_TARGET_KIND = {torch.uint8: 1, torch.int64: 2}


def predict_lowres(low: torch.Tensor, size, crop=None, align_corners: bool = True, target: Optional[torch.Tensor] = None,
                   hist: Optional[torch.Tensor] = None, want_pred: bool = True
                   ) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """low [B,h,w,C] f32 channels-last on the GPU (the classifier output as the engine keeps it); size = (H, W) interpolated
    to; crop = (Hc, Wc) <= size, the top-left region kept (VOC).  target [B,Hc,Wc] uint8 or int64 on the same device and
    hist int64 [C,C] (ACCUMULATED into: hist[t, argmax] += 1 where 0 <= t < C) go together; C <= 104 with hist, <= 256 with
    want_pred (a wider head's histogram: take the label map and hand it to RunningScore.update_from_labels /
    pp_confusion_matrix_from_labels, as RunningScore.update_from_lowres does).  Returns (pred uint8 [B,Hc,Wc] | None, hist | None); enqueued on the current stream, no sync."""
    B, h, w, C, ldx, H, W, Hc, Wc = _lowres_geom(low, size, crop)
    dev = low.device
    if not want_pred and hist is None:
        raise ValueError("nothing to compute: want_pred is False and no hist is given")
    if (target is None) != (hist is None):
        raise ValueError("target and hist go together")
    kind = 0
    if target is not None:
        if not isinstance(target, torch.Tensor) or target.dtype not in _TARGET_KIND:
            raise ValueError(f"target must be a uint8 or int64 tensor, got {getattr(target, 'dtype', type(target))}")
        if tuple(target.shape) != (B, Hc, Wc):
            raise ValueError(f"target must be [B,crop_h,crop_w] = {(B, Hc, Wc)}, got {tuple(target.shape)}")
        if target.device != dev:
            raise _lib.PixelPickHipError("target must live on the GPU with low: the HIP path has no CPU fallback")
        target = target.contiguous()
        kind = _TARGET_KIND[target.dtype]
        if (not isinstance(hist, torch.Tensor) or hist.dtype != torch.int64 or tuple(hist.shape) != (C, C)
                or not hist.is_contiguous() or hist.device != dev):
            raise ValueError(f"hist must be a contiguous int64 [{C},{C}] tensor on low's device")
    pred = torch.empty((B, Hc, Wc), dtype=torch.uint8, device=dev) if want_pred else None
    with torch.cuda.device(dev):
        rc = _lib.lib().pp_predict_lowres(low.data_ptr(), ldx, B, C, h, w, H, W, int(bool(align_corners)), Hc, Wc,
                                          target.data_ptr() if target is not None else None, kind,
                                          pred.data_ptr() if pred is not None else None,
                                          hist.data_ptr() if hist is not None else None, _lib.current_stream_ptr(dev))
    _lib.check(rc, "pp_predict_lowres")
    return pred, hist
