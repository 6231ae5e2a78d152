#!/usr/bin/env python3
"""Generate the evaluation fixture by IMPORTING the reference (authoring container only).

Runs only where the reference checkout exists.  Writes tests/golden/eval_lowres.npz: data only (inputs + the reference's
outputs); no reference source is copied.

Reference call sites exercised:
  deeplab.py:55-56          F.interpolate(pred, size, mode='bilinear', align_corners=True)
  model.py:124,197, eval.py:61   logits.argmax(dim=1)     (eval.py:55: the VOC crop [:, :, :h, :w])
  utils/metrics.py:162-204  RunningScore.update / get_scores

Two cases: CamVid-like 2 x 11 x (23,31) -> (67,101), ignore index 11; VOC-like 2 x 21 x (20,20) -> (80,80) cropped to (77,70),
ignore index 255.  Per case: the low-resolution logits (randn * 3, seeded), the labels, the reference's label map, its per-pixel
gap between the two largest logits (the guard the tests use: a build may differ from the reference only where that gap is within
fp32 rounding of zero), its confusion matrix, Mean IoU and Pixel Acc.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_acq import REF  # noqa: E402  (the reference checkout, put on sys.path there)
from utils.metrics import RunningScore  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")

CASES = [("cv", (2, 11, 23, 31), (67, 101), None, 11, 4100),
         ("voc", (2, 21, 20, 20), (80, 80), (77, 70), 255, 4200)]


def main():
    os.makedirs(OUT, exist_ok=True)
    out = {}
    for tag, (b, c, h, w), size, crop, ignore, seed in CASES:
        torch.manual_seed(seed)
        rng = np.random.RandomState(seed)
        low = torch.randn(b, c, h, w) * 3
        hc, wc = size if crop is None else crop
        y = rng.randint(0, c, size=(b, hc, wc)).astype(np.int64)
        y[rng.rand(b, hc, wc) < 0.1] = ignore
        logits = F.interpolate(low, size=size, mode="bilinear", align_corners=True)[:, :, :hc, :wc]
        pred = logits.argmax(dim=1)
        top2 = logits.topk(2, dim=1).values
        gap = (top2[:, 0] - top2[:, 1]).numpy().astype(np.float32)
        rs = RunningScore(c)
        rs.update(y, pred.numpy())
        scores = rs.get_scores()[0]
        out[f"{tag}_low"] = low.numpy()
        out[f"{tag}_size"] = np.array(size, dtype=np.int64)
        out[f"{tag}_crop"] = np.array([hc, wc], dtype=np.int64)
        out[f"{tag}_ignore"] = np.int64(ignore)
        out[f"{tag}_y"] = y.astype(np.uint8)
        out[f"{tag}_pred"] = pred.numpy().astype(np.uint8)
        out[f"{tag}_gap"] = gap
        out[f"{tag}_hist"] = rs.confusion_matrix.astype(np.int64)
        out[f"{tag}_miou"] = np.float64(scores["Mean IoU"])
        out[f"{tag}_pixel_acc"] = np.float64(scores["Pixel Acc"])
        print(tag, "unguarded share", float((gap <= 1e-4).mean()), "mIoU", scores["Mean IoU"], "acc", scores["Pixel Acc"])
    path = os.path.join(OUT, "eval_lowres.npz")
    np.savez_compressed(path, **out)
    print("eval fixture written", os.path.getsize(path))


if __name__ == "__main__":
    main()
