#!/usr/bin/env python3
"""What class_balanced costs on the device, and what it buys: 256 images 256x512x19, entropy, pool 6553 (top 5 %), k = 10.

Times, between device events: the plain top-5 % scoring op (pp_acq_lowres_score_topk at k = 6553: what a round launches without the
option), the label-map launch (pp_predict_lowres), pp_class_balance_select alone on the pool and the label map made beforehand, and the
whole op a round launches with the option on (the three together).  `iters` back-to-back launches per window after a warm-up, `repeats`
windows per op, the ops alternating; median and spread of the windows are printed.  On the same pools it then counts the distinct
predicted classes among the 10 picks of an image: the kernel's, and those of the reference's random sub-sample of the pool
(query.py:63-64, numpy seed 0), beside the classes the eligible pool holds.

    python tools/class_balance_bench.py [--maps smooth|noise] [--B 256] [--iters 20] [--repeats 5] [--out FILE]
    python tools/class_balance_bench.py --top5-only --package-root DIR   # the plain top-5 % op with another commit's build under DIR

`smooth` maps (a coarse random field, upsampled, plus a little noise) have label blobs with real edges, so one uncertain region can
dominate a pool as on real images; `noise` maps (independent logits per low-resolution pixel) spread every class over every pool.
--out appends the printed lines to FILE (profiles/class_balance.txt is such a file).
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

DEV = "cuda:0"
C, LOW, SIZE, K, TOP, STRATEGY = 19, (64, 128), (256, 512), 10, 0.05, "entropy"
_out = [None]


def say(line=""):
    print(line, flush=True)
    if _out[0] is not None:
        with open(_out[0], "a") as f:
            f.write(line + "\n")


def windows(fns, iters, repeats, warm=5):
    """fns: name -> callable.  -> name -> list of ms per call, one entry per window; the ops alternate window by window."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[name].append(a.elapsed_time(b) / iters)
    return out


def show(name, ts):
    say(f"  {name:66s} {statistics.median(ts):8.4f} ms  (windows: {', '.join(f'{t:.4f}' for t in ts)}; spread {max(ts) - min(ts):.4f})")
    return statistics.median(ts)


def make_inputs(B, maps):
    torch.manual_seed(0)
    h, w = LOW
    if maps == "smooth":
        coarse = torch.randn(B, C, 8, 16, device=DEV) * 3
        low = torch.nn.functional.interpolate(coarse, size=(h, w), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
        low = (low + 0.05 * torch.randn(B, h, w, C, device=DEV)).contiguous()
    else:
        low = torch.randn(B, h, w, C, device=DEV) * 3
    excl = (torch.rand(B, *SIZE, device=DEV) < 0.05).to(torch.uint8)
    return low, excl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", default="smooth", choices=("smooth", "noise"))
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--top5-only", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--package-root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    a = ap.parse_args()
    _out[0] = a.out
    sys.path.insert(0, os.path.abspath(a.package_root))
    from pixelpick_amd import acquisition as acq
    from pixelpick_amd.predict import predict_lowres

    if not torch.cuda.is_available():
        raise SystemExit("class_balance_bench needs a GPU: nothing here is measured on the CPU")
    low, excl = make_inputs(a.B, a.maps)
    N = SIZE[0] * SIZE[1]
    M = int(N * TOP)
    say(f"{a.B} images {SIZE[0]}x{SIZE[1]}x{C}, {STRATEGY}, pool M = {M}, k = {K}, {a.maps} maps, {torch.cuda.get_device_name(0)}; "
        f"package: {os.path.dirname(os.path.abspath(acq.__file__))}; {a.iters} launches per window, {a.repeats} windows per op")

    def score(k):
        return acq.score_topk_lowres(low, SIZE, excl, STRATEGY, k)[0]

    if a.top5_only:
        show(f"plain top-5 % scoring op, k = {M}", windows({"top5": lambda: score(M)}, a.iters, a.repeats)["top5"])
        return

    def labels():
        return predict_lowres(low, SIZE, want_pred=True)[0]

    cand, pred = score(M), labels()
    fns = {
        "top5": lambda: score(M),
        "labels": labels,
        "select": lambda: acq.class_balance_select(cand, pred, K, exclude=excl),
        "whole": lambda: acq.class_balance_select(score(M), labels(), K, exclude=excl),
    }
    ts = windows(fns, a.iters, a.repeats)
    t5 = show(f"plain top-5 % scoring op, k = {M} (the round without the option)", ts["top5"])
    tl = show("pp_predict_lowres alone (the label map)", ts["labels"])
    tsel = show("pp_class_balance_select alone (class_balance_kernel)", ts["select"])
    tw = show("scoring op at M + pp_predict_lowres + pp_class_balance_select", ts["whole"])
    say(f"  -> the option costs {tw - t5:+.4f} ms per {a.B} images ({tw / t5:.2f}x the plain top-5 % op): {tl:.4f} ms the label map, "
        f"{tsel:.4f} ms the selection itself")

    # what it buys: distinct predicted classes among the K picks of an image
    idx, pos, n = acq.class_balance_select(cand, pred, K, exclude=excl)
    torch.cuda.synchronize()
    cand_h, pred_h, excl_h = cand.cpu().numpy(), pred.cpu().numpy().reshape(a.B, -1), excl.cpu().numpy().reshape(a.B, -1)
    idx_h, pos_h = idx.cpu().numpy(), pos.cpu().numpy()
    np.random.seed(0)
    kern, rand, pool, last = [], [], [], []
    for b in range(a.B):
        ok = excl_h[b][cand_h[b]] == 0
        pool.append(len(set(pred_h[b][cand_h[b][ok]].tolist())))
        kern.append(len(set(pred_h[b][idx_h[b]].tolist())))
        rand.append(len(set(pred_h[b][np.random.choice(cand_h[b], K, False)].tolist())))
        last.append(int(pos_h[b].max()))
    say(f" distinct predicted classes among the {K} picks of an image, mean over {a.B} images: class_balanced {np.mean(kern):.2f}, the "
        f"reference's random sub-sample of the pool {np.mean(rand):.2f}; classes in the eligible pool {np.mean(pool):.2f} "
        f"(min(k, pool) = {np.mean(np.minimum(pool, K)):.2f}); balanced picks per image: min {int(n.min())}")
    say(f" list position of the deepest pick: mean {np.mean(last):.0f}, max {max(last)} of {M}")


if __name__ == "__main__":
    main()
