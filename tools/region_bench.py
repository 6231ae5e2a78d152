#!/usr/bin/env python3
"""What region-aware acquisition costs on the device: 256 images 256x512, C = 19, entropy, k = 10, r in {1, 3, 16}.

Times, between device events, the region kernel alone (pp_acq_region_score_map on maps made beforehand, all three modes at r = 3), the
whole op a round launches with the option on (pp_predict_lowres + pp_acq_lowres_score_topk at k = 0 + pp_acq_region_score_map +
pp_topk_select at k = 10), its two producer launches by themselves, and beside them the plain pp_acq_lowres_score_topk k = 10 op - what
the round launches without the option.  `iters` back-to-back launches per window after a warm-up, `repeats` windows per op, the ops
alternating; median and spread of the windows are printed.  The region kernel moves 9 B per pixel (1 B label + 4 B score in, 4 B out);
the line under each timing sets that against 8 TB/s.

    python tools/region_bench.py [--B 256] [--iters 20] [--repeats 5]
    python tools/region_bench.py --k10-only --package-root DIR     # the k = 10 op with another commit's build of the package under DIR
"""
import argparse
import os
import statistics
import sys

import torch

DEV = "cuda:0"
C, LOW, SIZE, K, STRATEGY = 19, (64, 128), (256, 512), 10, "entropy"
RADII = (1, 3, 16)
HBM_BYTES_PER_S = 8e12


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
    print(f"  {name:66s} {statistics.median(ts):8.4f} ms  (windows: {', '.join(f'{t:.4f}' for t in ts)}; spread {max(ts) - min(ts):.4f})")
    return statistics.median(ts)


def make_inputs(B):
    """Smooth classifier outputs (a coarse random field, upsampled, plus a little noise): label regions with real edges."""
    torch.manual_seed(0)
    h, w = LOW
    coarse = torch.randn(B, C, 8, 16, device=DEV) * 3
    low = torch.nn.functional.interpolate(coarse, size=(h, w), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    low = (low + 0.05 * torch.randn(B, h, w, C, device=DEV)).contiguous()
    excl = (torch.rand(B, *SIZE, device=DEV) < 0.05).to(torch.uint8)
    return low, excl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--k10-only", action="store_true")
    ap.add_argument("--package-root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    from pixelpick_amd import acquisition as acq

    if not torch.cuda.is_available():
        raise SystemExit("region_bench needs a GPU: nothing here is measured on the CPU")
    low, excl = make_inputs(a.B)
    H, W = SIZE
    N = H * W
    print(f"{a.B} images {H}x{W}x{C}, {STRATEGY}, k = {K}, {torch.cuda.get_device_name(0)}; "
          f"package: {os.path.dirname(os.path.abspath(acq.__file__))}; {a.iters} launches per window, {a.repeats} windows per op")

    def score(k):
        return acq.score_topk_lowres(low, SIZE, excl, STRATEGY, k)[0]

    if a.k10_only:
        show(f"scoring op, k = {K}", windows({"k10": lambda: score(K)}, a.iters, a.repeats)["k10"])
        return
    from pixelpick_amd.predict import predict_lowres

    def producers():
        pred, _ = predict_lowres(low, SIZE, want_pred=True)
        return pred, acq.score_topk_lowres(low, SIZE, None, STRATEGY, 0)[2]

    pred, unc = producers()

    def region(r, mode="product"):
        return acq.region_score_map(pred, unc, r, C, exclude=excl, mode=mode)

    def whole(r):
        p, u = producers()
        m = acq.region_score_map(p, u, r, C, exclude=excl)
        return acq.topk_select(m.reshape(a.B, N), K, True)[0]

    fns = {"k10": lambda: score(K), "producers": producers,
           "topk": lambda m=region(3): acq.topk_select(m.reshape(a.B, N), K, True)}
    for r in RADII:
        fns[f"region{r}"] = lambda r=r: region(r)
        fns[f"whole{r}"] = lambda r=r: whole(r)
    for mode in ("impurity", "uncertainty"):
        fns[f"region3_{mode}"] = lambda mode=mode: region(3, mode)
    ts = windows(fns, a.iters, a.repeats)
    t10 = show(f"scoring op, k = {K} (the round without the option)", ts["k10"])
    tp = show("the two producer launches (label map + score map, no selection)", ts["producers"])
    show(f"pp_topk_select alone on a region map, k = {K}", ts["topk"])
    nbytes = 9.0 * a.B * N
    floor_ms = nbytes / HBM_BYTES_PER_S * 1e3
    print(f"  the region kernel moves 9 B per pixel: {nbytes / 1e6:.0f} MB per launch, {floor_ms:.4f} ms at 8 TB/s")
    for r in RADII:
        tr = show(f"pp_acq_region_score_map alone, r = {r} (region_score_kernel, product)", ts[f"region{r}"])
        print(f"    -> {nbytes / (tr * 1e-3) / 1e12:.3f} TB/s of its 9 B per pixel, {tr / floor_ms:.1f}x the HBM floor; "
              f"{a.B * N / (tr * 1e-3) / 1e9:.1f} Gpixels/s")
        tw = show(f"whole op, r = {r}: producers + region + pp_topk_select", ts[f"whole{r}"])
        print(f"    -> {tw / t10:.2f}x the k = {K} op ({tw - t10:+.4f} ms per {a.B} images); the producers are {tp / tw:.0%} of it")
    for mode in ("impurity", "uncertainty"):
        show(f"pp_acq_region_score_map alone, r = 3, mode {mode}", ts[f"region3_{mode}"])


if __name__ == "__main__":
    main()
