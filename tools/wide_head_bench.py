#!/usr/bin/env python3
"""A head wider than 64 classes (150: ADE20K) on the low-resolution routes against the only routes that could serve it before.

  train step   DeepLab (MobileNetV2), 150 classes, B = 4, 256 x 512, 20 labelled pixels per image: FlatTrainer.train_step with the
               loss taken from the classifier output (streamed loss kernels) against PIXELPICK_SPARSE_LOWRES_CE=0 (full-size logits,
               dense loss, bilinear backward) - two trainers in one process, the flag flipped around each step.
  metrics      the confusion matrix of B images at 150 classes from the classifier output (RunningScore.update_from_lowres:
               pp_predict_lowres label map + pp_confusion_matrix_from_labels) against pp_bilinear_fwd -> pp_confusion_matrix_update.

One process, warmed up, device events; the variants alternate inside every repetition; median and (min..max) of the per-repetition
means.  Writes the table to profiles/wide_heads.txt as well.  A record, not a gate: no test asserts a time.

    python tools/wide_head_bench.py [--reps 5] [--iters 10] [--out profiles/wide_heads.txt]
"""
import argparse
import os
import sys
import warnings
from argparse import Namespace

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from pixelpick_amd import _lib  # noqa: E402
from pixelpick_amd import engine as E  # noqa: E402
from pixelpick_amd import trainer as T  # noqa: E402
from pixelpick_amd.utils.metrics import RunningScore  # noqa: E402
from pixelpick_amd.utils.utils import get_model  # noqa: E402

DEV = "cuda:0"
C, B, H, W, N_LAB, IGN = 150, 4, 256, 512, 20, 255


def mean_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def alternate(variants, reps, iters):
    for fn in variants:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = [[] for _ in variants]
    for _ in range(reps):
        for i, fn in enumerate(variants):
            t[i].append(mean_ms(fn, iters))
    return t


def cell(v):
    return f"{float(np.median(v)):9.4f} ({min(v):.4f}..{max(v):.4f})"


def train_rows(reps, iters):
    torch.manual_seed(0)
    x = torch.randn(B, 3, H, W, device=DEV)
    y = torch.full((B, H, W), IGN, dtype=torch.int64)
    for b in range(B):
        y[b].view(-1)[torch.randperm(H * W)[:N_LAB]] = torch.randint(0, C, (N_LAB,))
    y = y.to(DEV)
    args = Namespace(use_mc_dropout=False, mc_dropout_p=0.2, n_classes=C, network_name="deeplab", weight_type="random",
                     use_dilated_resnet=True, n_layers=50, width_multiplier=1.0)
    trainers = {}
    for lowres in (True, False):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            trainers[lowres] = T.FlatTrainer(get_model(args).to(DEV).train(), ignore_index=IGN)

    def step(lowres):
        def run():
            T.SPARSE_LOWRES_CE = lowres
            trainers[lowres].train_step(x, y, keep_logits="low" if lowres else True)
        return run
    before = T.SPARSE_LOWRES_CE
    try:
        t = alternate((step(True), step(False)), reps, iters)
    finally:
        T.SPARSE_LOWRES_CE = before
    return [f"train step, DeepLab C={C} B={B} {H}x{W}, {N_LAB} labelled px/img (eager steps, ms)",
            f"  loss from the classifier output (streamed kernels)   {cell(t[0])}",
            f"  PIXELPICK_SPARSE_LOWRES_CE=0 (full-size logits)      {cell(t[1])}",
            f"  dense / low-resolution                               {float(np.median(t[1])) / float(np.median(t[0])):9.2f}"]


def metrics_rows(reps, iters):
    torch.manual_seed(0)
    L = _lib.lib()
    h, w = H // 4, W // 4
    out = []
    for Bm in (4, 32):
        low = torch.randn(Bm, h, w, C, device=DEV) * 3
        coarse = torch.randint(0, C, (Bm, (H + 7) // 8, (W + 7) // 8), device=DEV)
        y = coarse.repeat_interleave(8, dim=1).repeat_interleave(8, dim=2)[:, :H, :W]
        y = torch.where(torch.rand(Bm, H, W, device=DEV) < 0.03, torch.full_like(y, IGN), y).contiguous()
        hist_p = torch.zeros((C, C), dtype=torch.int64, device=DEV)
        rs = RunningScore(C)

        def pair():
            logits = E.bilinear(E.Tape(False), E.Var(low), (H, W), True, 0.0, out_nchw=True).t
            rc = L.pp_confusion_matrix_update(logits.data_ptr(), Bm, C, H * W, logits.stride(0), logits.stride(1), y.data_ptr(),
                                              hist_p.data_ptr(), _lib.current_stream_ptr())
            _lib.check(rc, "pp_confusion_matrix_update")

        def lowres():
            rs.update_from_lowres(y, low, (H, W), align_corners=True)

        pair(), lowres()
        assert torch.equal(hist_p, rs._dev_hist), "the two paths disagree"
        t = alternate((lowres, pair), reps, iters)
        out += [f"confusion matrix, C={C} B={Bm} {h}x{w} -> {H}x{W} (ms)",
                f"  from the classifier output (label map + from_labels) {cell(t[0])}",
                f"  pp_bilinear_fwd -> pp_confusion_matrix_update        {cell(t[1])}",
                f"  pair / low-resolution                                {float(np.median(t[1])) / float(np.median(t[0])):9.2f}"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_heads.txt"))
    a = ap.parse_args()
    lines = [f"tools/wide_head_bench.py --reps {a.reps} --iters {a.iters}: median (min..max) of the per-repetition means, variants alternating",
             f"device: {torch.cuda.get_device_name(0)}", ""]
    lines += metrics_rows(a.reps, a.iters) + [""] + train_rows(a.reps, a.iters)
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
