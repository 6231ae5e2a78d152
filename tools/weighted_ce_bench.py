#!/usr/bin/env python3
"""What class weights and label smoothing cost in the train step, and what the un-weighted step costs against the parent commit.

  train step   DeepLab (MobileNetV2), B = 4, 256 x 512, 20 labelled pixels per image, at 19 classes (register loss kernels) and at
               150 (streamed ones): FlatTrainer.train_step after enable_replay (the recorded step: GPU-bound, so a kernel's cost is
               visible), with the loss options off (the un-weighted entry, today's step) and with weights + label_smoothing = 0.1 -
               two trainers in one process, alternating inside every repetition.
  parent       the same un-weighted step from ANOTHER checkout with its own build (--parent DIR: the parent commit, built in place).
               One process holds one library, so every tree is timed in a child process of its own, both with the un-weighted
               trainer alone (the same process contents on both sides); the children alternate (this tree, parent, this tree,
               ...) `--runs` times, and the parent's own run-to-run spread is the yardstick the un-weighted step of this tree is
               read against.
  loss alone   the low-resolution loss entry on a DENSELY labelled map (every pixel of 4 x 256 x 512 labelled, sparse=False), where
               the extra per-class terms could show: off / weights / weights + smoothing.

Warmed up, device events; median and (min..max) of the per-repetition means.  Writes the table to profiles/weighted_ce.txt as well.
A record, not a gate: no test asserts a time.

    python tools/weighted_ce_bench.py [--parent DIR] [--runs 3] [--reps 5] [--iters 10] [--out profiles/weighted_ce.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import warnings
from argparse import Namespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))
DEV = "cuda:0"
B, H, W, N_LAB, IGN, EPS = 4, 256, 512, 20, 255, 0.1
CLASSES = (19, 150)


# ----------------------------------------------------------------------------------------------------------------- worker
def worker(root, weighted, reps, iters):
    """Times one tree (the package under `root`) in this process; prints one JSON line."""
    sys.path.insert(0, root)
    import torch
    from pixelpick_amd import engine as E
    from pixelpick_amd import trainer as T
    from pixelpick_amd.utils.utils import get_model

    def mean_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / iters

    def alternate(variants):
        for fn in variants:
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t = [[] for _ in variants]
        for _ in range(reps):
            for i, fn in enumerate(variants):
                t[i].append(mean_ms(fn))
        return t

    def weights(C):
        u = torch.rand(C, generator=torch.Generator().manual_seed(5))
        return torch.pow(2.0, 4.0 * u - 2.0)

    res = {"device": torch.cuda.get_device_name(0), "step": {}, "loss": {}}
    for C in CLASSES:
        torch.manual_seed(0)
        x = torch.randn(B, 3, H, W, device=DEV)
        y = torch.full((B, H, W), IGN, dtype=torch.int64)
        for b in range(B):
            y[b].view(-1)[torch.randperm(H * W)[:N_LAB]] = torch.randint(0, C, (N_LAB,))
        y = y.to(DEV)
        args = Namespace(use_mc_dropout=False, mc_dropout_p=0.2, n_classes=C, network_name="deeplab", weight_type="random",
                         use_dilated_resnet=True, n_layers=50, width_multiplier=1.0)
        options = [("off", {})] + ([("weighted", dict(class_weight=weights(C).tolist(), label_smoothing=EPS))] if weighted else [])
        trainers = []
        for _, kw in options:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                trainers.append(T.FlatTrainer(get_model(args).to(DEV).train(), ignore_index=IGN, **kw))
        try:
            for tr in trainers:
                tr.enable_replay(x, y, warmup=1, keep_logits="low")
            t = alternate([(lambda tr=tr: tr.train_step(x, y, keep_logits="low")) for tr in trainers])
        finally:
            for tr in trainers:
                tr.close()
        res["step"][str(C)] = {name: t[i] for i, (name, _) in enumerate(options)}
        del trainers
        # the loss entry alone, every pixel labelled
        low = torch.randn(B, H // 4, W // 4, C, device=DEV) * 3
        yd = torch.randint(0, C, (B, H, W), device=DEV)
        wd = weights(C).to(DEV)
        forms = [("off", {})] + ([("weights", dict(class_weight=wd)), ("weights+smoothing", dict(class_weight=wd, label_smoothing=EPS))]
                                 if weighted else [])
        t = alternate([(lambda kw=kw: E.cross_entropy_lowres(low, (H, W), yd, IGN, sparse=False, **kw)) for _, kw in forms])
        res["loss"][str(C)] = {name: t[i] for i, (name, _) in enumerate(forms)}
    print("RESULT " + json.dumps(res), flush=True)


def run_child(root, weighted, reps, iters):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--reps", str(reps), "--iters", str(iters)]
    if weighted:
        cmd.append("--weighted")
    env = dict(os.environ, PIXELPICK_MNV2_WEIGHTS="random")
    out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    for line in out.stdout.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    raise RuntimeError(f"worker for {root} failed (exit {out.returncode}):\n{out.stdout[-4000:]}")


# ------------------------------------------------------------------------------------------------------------------- table
def cell(v):
    return f"{float(np.median(v)):9.4f} ({min(v):.4f}..{max(v):.4f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="checkout of the parent commit with its own build (timed un-weighted)")
    ap.add_argument("--runs", type=int, default=3, help="child processes per tree, alternating")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weighted_ce.txt"))
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--weighted", action="store_true")
    a = ap.parse_args()
    if a.worker:
        worker(os.path.abspath(a.root), a.weighted, a.reps, a.iters)
        return
    here, alone, parent = [], [], []
    for i in range(a.runs):
        here.append(run_child(ROOT, True, a.reps, a.iters))
        if a.parent:
            alone.append(run_child(ROOT, False, a.reps, a.iters))
            parent.append(run_child(os.path.abspath(a.parent), False, a.reps, a.iters))
        print(f"run {i + 1} of {a.runs} done", file=sys.stderr, flush=True)
    lines = [f"tools/weighted_ce_bench.py --runs {a.runs} --reps {a.reps} --iters {a.iters}: one child process per run and tree, trees alternating;",
             "inside a process the variants alternate; per run: median of the per-repetition means (ms)",
             f"device: {here[0]['device']}", ""]
    for C in CLASSES:
        k = str(C)
        off = [float(np.median(r["step"][k]["off"])) for r in here]
        wtd = [float(np.median(r["step"][k]["weighted"])) for r in here]
        lines.append(f"train step, DeepLab C={C} B={B} {H}x{W}, {N_LAB} labelled px/img (recorded step replayed, ms; runs: "
                     + " ".join(f"{v:.4f}" for v in off) + ")")
        if parent:
            par = [float(np.median(r["step"][k]["off"])) for r in parent]
            one = [float(np.median(r["step"][k]["off"])) for r in alone]
            inside = min(par) <= float(np.median(one)) <= max(par)
            lines.append(f"  parent commit, its own build, un-weighted alone      {cell(par)}")
            lines.append(f"  this tree, un-weighted trainer alone in the process  {cell(one)}")
            lines.append(f"  this tree's median inside the parent's spread        {'yes' if inside else 'no'}"
                         f"   (this / parent = {float(np.median(one)) / float(np.median(par)):.4f})")
        lines.append(f"  this tree, loss options off, beside the weighted one {cell(off)}")
        lines.append(f"  this tree, weights + label_smoothing={EPS}             {cell(wtd)}")
        lines.append(f"  weighted - off (same process, median of runs)        {float(np.median([w - o for w, o in zip(wtd, off)])):+9.4f}")
        lines.append("")
    for C in CLASSES:
        k = str(C)
        lines.append(f"loss entry alone, C={C} B={B} {H // 4}x{W // 4} -> {H}x{W}, every pixel labelled, forward + backward (ms)")
        for name in ("off", "weights", "weights+smoothing"):
            lines.append(f"  this tree, {name:<20}                      {cell([float(np.median(r['loss'][k][name])) for r in here])}")
        if parent:
            lines.append(f"  parent commit, off                                   {cell([float(np.median(r['loss'][k]['off'])) for r in parent])}")
        lines.append("")
    text = "\n".join(lines)
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
