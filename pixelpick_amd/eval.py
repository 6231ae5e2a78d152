"""Stand-alone validation with the reference's call surface (eval.py:15-94 `evaluate`) on the HIP path.

The network stops at its classifier output (`forward_lowres`); the confusion matrix comes from `RunningScore.update_from_lowres`
and the label map, when a visualizer asks for it, from `predict_lowres` - one launch each, interpolating on the fly, so the
full-resolution logits, their softmax and the two device-to-host maps of eval.py:60-63 never exist.  A `visualizer` that offers
`from_lowres` (utils.utils.Visualiser) gets the picture the same way: its byte panels are rendered from the classifier output in
one call per forwarded batch (visualise.render_lowres); any other callable receives the reference's dict of CPU tensors.
"""
import os
from math import ceil
from typing import Callable, Optional

import numpy as np
import torch
import torch.nn.functional as F

from . import acquisition as acq
from .model import write_log
from .predict import predict_lowres
from .utils.metrics import RunningScore


@torch.no_grad()
def evaluate(model, dataloader, experim_name: str, epoch: Optional[int] = None, dir_ckpt: Optional[str] = None,
             visualizer: Optional[Callable] = None, visualize_interval: Optional[int] = 100, stride_total: int = 8,
             device: torch.device = torch.device("cuda:0"), debug: bool = False, val_batch_size: int = 8) -> float:
    """eval.py:15-94.  `dataloader` yields the reference's batch dicts {'x','y'}; its `.dataset` offers `n_classes` and
    `dataset_name` ("voc": reflect-pad to a multiple of `stride_total`, crop back).  Consecutive batches of equal size are
    forwarded `val_batch_size` images at a time, as Model._val does (eval mode: the result per image does not depend on the
    batch).  With `dir_ckpt`, log_val.txt (header epoch,miou,pixel_acc + one row) is written to <dir_ckpt>[/eNN]/val and, every
    `visualize_interval`-th batch, the first image's picture goes to <that directory>/<num_iter>.png: through
    `visualizer.from_lowres(...)` when the visualizer has it (our Visualiser; heads of up to 64 classes), otherwise
    `visualizer(dict_tensors, fp=...)` receives input / target / pred / confidence / margin (negated) / entropy on the CPU.
    -> mean IoU."""
    if not callable(getattr(model, "forward_lowres", None)):
        raise TypeError(f"evaluate() needs a model with forward_lowres(); {type(model).__name__} has none")
    if dir_ckpt is not None:
        dir_ckpt = f"{dir_ckpt}/e{epoch:02d}/val" if epoch is not None else f"{dir_ckpt}/val"
        os.makedirs(dir_ckpt, exist_ok=True)
    model.eval()
    voc = getattr(dataloader.dataset, "dataset_name", None) == "voc"
    align = bool(getattr(model, "LOWRES_ALIGN_CORNERS", True))
    tracker = RunningScore(n_classes=dataloader.dataset.n_classes)
    pend = []                                   # (num_iter, x on the device, y on the device)

    def flush():
        if not pend:
            return
        xs, ys = torch.cat([p[1] for p in pend], dim=0), torch.cat([p[2] for p in pend], dim=0)
        crop = None
        if voc:
            h, w = ys.shape[1:]
            pad_h = ceil(h / stride_total) * stride_total - xs.shape[2]
            pad_w = ceil(w / stride_total) * stride_total - xs.shape[3]
            xp = F.pad(xs, pad=(0, pad_w, 0, pad_h), mode='reflect')
            crop = (h, w)
        else:
            xp = xs
        low, size = model.forward_lowres(xp)
        tracker.update_from_lowres(ys, low, size, crop=crop, align_corners=align)
        fused = callable(getattr(visualizer, "from_lowres", None)) and low.shape[-1] <= 64 and xs.shape[2:] == ys.shape[1:]
        if dir_ckpt is not None and visualizer is not None and fused:
            # our Visualiser: the due images' byte panels in ONE render_lowres call on the classifier output, one copy to the host
            offs = np.cumsum([0] + [p[1].shape[0] for p in pend])
            due = [(int(offs[i]), f"{dir_ckpt}/{p[0]}.png") for i, p in enumerate(pend) if p[0] % visualize_interval == 0]
            if due:
                visualizer.from_lowres(low, size, xs, ys, [fp for _, fp in due], crop=crop, align_corners=align,
                                       index=[i for i, _ in due])
        elif dir_ckpt is not None and visualizer is not None:
            off = 0
            for num_iter, x, y in pend:
                if num_iter % visualize_interval == 0:
                    lo = low[off:off + 1]
                    pred = predict_lowres(lo, size, crop=crop, align_corners=align)[0]
                    ent, lc, ms = [acq.score_topk_lowres(lo, size, None, uc, 0, crop=crop, align_corners=align, return_map=True)[2][0].cpu()
                                   for uc in ("entropy", "least_confidence", "margin_sampling")]
                    visualizer({'input': x[0].cpu(), 'target': y[0].cpu(), 'pred': pred[0].to(torch.int64).cpu(),
                                'confidence': lc, 'margin': -ms,           # minus sign: smaller margins are drawn brighter
                                'entropy': ent}, fp=f"{dir_ckpt}/{num_iter}.png")
                off += x.shape[0]
        pend.clear()

    for num_iter, dict_data in enumerate(dataloader):
        x, y = dict_data['x'].to(device), dict_data['y'].to(device)
        if pend and (pend[0][1].shape[1:] != x.shape[1:] or pend[0][2].shape[1:] != y.shape[1:]
                     or sum(p[1].shape[0] for p in pend) + x.shape[0] > val_batch_size):
            flush()
        pend.append((num_iter, x, y))
        if debug:
            break
    flush()
    scores = tracker.get_scores()[0]
    miou, pixel_acc = scores['Mean IoU'], scores['Pixel Acc']
    if dir_ckpt is not None:
        write_log(f"{dir_ckpt}/log_val.txt", header=["epoch", "miou", "pixel_acc"])
        write_log(f"{dir_ckpt}/log_val.txt", list_entities=[epoch, miou, pixel_acc])
    print(f"\n{'=' * 100}"
          f"\nExperim name: {experim_name}"
          f"\nEpoch {epoch} | miou: {miou:.3f} | pixel_acc.: {pixel_acc:.3f}"
          f"\n{'=' * 100}\n")
    return miou
