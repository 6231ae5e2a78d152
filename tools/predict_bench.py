#!/usr/bin/env python3
"""Confusion matrix / label map from the low-resolution classifier output in one launch (pp_predict_lowres) against the pair of
launches it replaces (pp_bilinear_fwd -> pp_confusion_matrix_update), per dataset shape.

One process, warmed up, device events; the variants alternate inside every repetition, and the spread over the repetitions
(min .. max of the per-repetition means) is printed beside the median so that "slower" can be read against it.  Bytes are
algorithmic, from the shapes: fused = B*(h*w*C*4 + Hc*Wc*(target bytes + 1)), pair = B*(h*w*C*4 + 2*C*Hc*Wc*4 + Hc*Wc*8)
(the logits written and read back, int64 labels).  The bound is HBM: the last column is the fused call's share of 8 TB/s.

    python tools/predict_bench.py [--reps 7] [--iters 20]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pixelpick_amd import _lib  # noqa: E402
from pixelpick_amd import engine as E  # noqa: E402
from pixelpick_amd.predict import predict_lowres  # noqa: E402

DEV = "cuda:0"
HBM = 8e12

ROWS = [
    # name, B, C, (h,w), (H,W), crop, align, target dtype
    ("cs i64", 256, 19, (64, 128), (256, 512), None, True, torch.int64),
    ("cs u8", 256, 19, (64, 128), (256, 512), None, True, torch.uint8),
    ("camvid", 64, 11, (90, 120), (360, 480), None, True, torch.int64),
    ("voc crop", 64, 21, (80, 80), (320, 320), (317, 301), True, torch.int64),
    ("fpn x2", 16, 19, (128, 256), (256, 512), None, False, torch.int64),
    ("cs full", 8, 19, (256, 512), (1024, 2048), None, True, torch.int64),
]


def mean_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    L = _lib.lib()
    print(f"{'row':9s} {'B':>4s} | {'pair ms (min..max)':>26s} | {'fused hist ms':>26s} | {'fused hist+pred ms':>26s} | {'pair/fused':>10s} | "
          f"{'pair MB':>8s} {'fused MB':>8s} | {'GB/s':>7s} {'of 8TB/s':>8s}")
    for name, B, C, (h, w), size, crop, align, tdt in ROWS:
        torch.manual_seed(0)
        hc, wc = size if crop is None else crop
        low = torch.randn(B, h, w, C, device=DEV) * 3
        # labels in contiguous regions with ~3 % void, as a label map has (8 x 8 blocks of one class)
        coarse = torch.randint(0, C, (B, (hc + 7) // 8, (wc + 7) // 8), device=DEV)
        y = coarse.repeat_interleave(8, dim=1).repeat_interleave(8, dim=2)[:, :hc, :wc]
        y = torch.where(torch.rand(B, hc, wc, device=DEV) < 0.03, torch.full_like(y, 255), y).to(tdt).contiguous()
        hist_p = torch.zeros((C, C), dtype=torch.int64, device=DEV)
        hist_f = torch.zeros((C, C), dtype=torch.int64, device=DEV)

        def pair():
            logits = E.bilinear(E.Tape(False), E.Var(low), size, align, 0.0, out_nchw=True).t
            if crop is not None:
                logits = logits[:, :, :hc, :wc].contiguous()
            yy = y.to(torch.int64)            # (what RunningScore.update_from_logits does with a uint8 label map)
            rc = L.pp_confusion_matrix_update(logits.data_ptr(), B, C, hc * wc, logits.stride(0), logits.stride(1), yy.data_ptr(),
                                              hist_p.data_ptr(), _lib.current_stream_ptr())
            _lib.check(rc, "pp_confusion_matrix_update")

        def fused():
            predict_lowres(low, size, crop=crop, align_corners=align, target=y, hist=hist_f, want_pred=False)

        def fused_pred():
            predict_lowres(low, size, crop=crop, align_corners=align, target=y, hist=hist_f)

        variants = (pair, fused, fused_pred)
        for fn in variants:                   # warm-up (allocator, first launch)
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        hist_p.zero_(), hist_f.zero_()
        pair(), fused()
        assert torch.equal(hist_p, hist_f), f"{name}: the two paths disagree"
        t = [[] for _ in variants]
        for _ in range(a.reps):
            for i, fn in enumerate(variants):
                t[i].append(mean_ms(fn, a.iters))
        med = [float(np.median(v)) for v in t]
        cell = lambda v, m: f"{m:9.4f} ({min(v):.4f}..{max(v):.4f})"
        tb = 8 if tdt == torch.int64 else 1
        by_f = B * (h * w * C * 4 + hc * wc * (tb + 1))
        by_p = B * (h * w * C * 4 + 2 * C * hc * wc * 4 + hc * wc * 8)
        gbs = by_f / (med[2] * 1e-3) / 1e9
        print(f"{name:9s} {B:4d} | {cell(t[0], med[0]):>26s} | {cell(t[1], med[1]):>26s} | {cell(t[2], med[2]):>26s} | {med[0] / med[1]:10.2f} | "
              f"{by_p / 1e6:8.1f} {by_f / 1e6:8.1f} | {gbs:7.1f} {100 * gbs * 1e9 / HBM:7.2f}%", flush=True)


if __name__ == "__main__":
    main()
