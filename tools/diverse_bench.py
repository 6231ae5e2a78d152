#!/usr/bin/env python3
"""What diverse_picks costs on the device, and what it buys: 256 images 256x512x19, entropy, pool 6553 (top 5 %), k = 10.

Times, between device events: the plain top-5 % scoring op (pp_acq_lowres_score_topk at k = 6553: what a round launches without the
option), pp_acq_lowres_prob_at_u8 alone on the pool (the features), pp_diverse_select alone on the pool and the features made beforehand
- in the form the library chooses and, on the test build, with the streaming form forced onto the same input - and the whole op a round
launches with the option on (the three together).  `iters` back-to-back launches per window after a warm-up, `repeats` windows per op,
the ops alternating; median and spread of the windows are printed.  On the same pools it then reports, per image and averaged: the final
k-centre radius of the 10 picks (the largest squared feature distance of an eligible pool entry to its nearest pick) and the distinct
predicted classes among them - for diverse_picks, for the reference's random sub-sample of the pool (query.py:63-64, numpy seed 0) and for
class_balanced.  A whole round and real pools are out of scope here.

    python tools/diverse_bench.py [--maps smooth|noise] [--B 256] [--iters 20] [--repeats 5] [--out FILE]
    python tools/diverse_bench.py --top5-only --package-root DIR   # the plain top-5 % op with another commit's build under DIR

`smooth` maps (a coarse random field, upsampled, plus a little noise) have label blobs with real edges, so one uncertain region can
dominate a pool as on real images; `noise` maps (independent logits per low-resolution pixel) spread every class over every pool.
--out appends the printed lines to FILE (profiles/diverse_select.txt is such a file).
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
    say(f"  {name:72s} {statistics.median(ts):8.4f} ms  (windows: {', '.join(f'{t:.4f}' for t in ts)}; spread {max(ts) - min(ts):.4f})")
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


def radius(feat_b, ok_b, picks_pos):
    """The k-centre radius of one image: the largest squared distance of an eligible pool entry to its nearest pick."""
    f = feat_b[:, :C].astype(np.int64)
    d = np.min([((f - f[p]) ** 2).sum(axis=1) for p in picks_pos], axis=0)
    return int(d[ok_b].max())


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
    from pixelpick_amd import _lib
    from pixelpick_amd import acquisition as acq
    from pixelpick_amd.predict import predict_lowres

    if not torch.cuda.is_available():
        raise SystemExit("diverse_bench needs a GPU: nothing here is measured on the CPU")
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

    img = torch.arange(a.B, dtype=torch.int32, device=DEV).repeat_interleave(M)

    def features(cand):
        return acq.prob_at_lowres(low, SIZE, img, cand.reshape(-1)).view(a.B, M, -1)

    def select(cand, feat):
        return acq.diverse_select(cand, feat, K, n_features=C, exclude=excl)

    cand = score(M)
    feat = features(cand)
    L = _lib.lib()
    resident = int(L.pp_diverse_resident_candidates(C))
    fns = {
        "top5": lambda: score(M),
        "features": lambda: features(cand),
        "select": lambda: select(cand, feat),
        "whole": lambda: (lambda c: select(c, features(c)))(score(M)),
    }
    if _lib.knobs_build() and M <= resident:
        def streamed():
            L.pp_debug_set_acq_tuning(11, 0)
            try:
                return select(cand, feat)
            finally:
                L.pp_debug_set_acq_tuning(0, 0)
        fns["select_stream"] = streamed
        want, got = select(cand, feat), streamed()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(want, got)), "the two forms disagree"
    ts = windows(fns, a.iters, a.repeats)
    t5 = show(f"plain top-5 % scoring op, k = {M} (the round without the option)", ts["top5"])
    tf = show(f"pp_acq_lowres_prob_at_u8 alone, {a.B} x {M} listed pixels (prob_at_kernel)", ts["features"])
    form = "resident" if M <= resident else "streaming"
    tsel = show(f"pp_diverse_select alone, the form the library chooses: {form} (resident up to M = {resident})", ts["select"])
    if "select_stream" in ts:
        tst = show("pp_diverse_select alone, the streaming form forced onto the same input", ts["select_stream"])
        say(f"  -> resident / streaming = {tsel / tst:.2f}")
    else:
        say("  (the streaming form is forced through a switch of the test build only: run with PIXELPICK_KNOBS_BUILD=1 for the A/B)")
    tw = show("scoring op at M + pp_acq_lowres_prob_at_u8 + pp_diverse_select", ts["whole"])
    say(f"  -> the option costs {tw - t5:+.4f} ms per {a.B} images ({tw / t5:.2f}x the plain top-5 % op): {tf:.4f} ms the features, "
        f"{tsel:.4f} ms the selection itself")

    # what it buys, on these synthetic pools
    pred = predict_lowres(low, SIZE, want_pred=True)[0]
    idx, pos, dist, n = select(cand, feat)
    bal_idx, bal_pos, _ = acq.class_balance_select(cand, pred, K, exclude=excl)
    torch.cuda.synchronize()
    cand_h, pred_h, excl_h = cand.cpu().numpy(), pred.cpu().numpy().reshape(a.B, -1), excl.cpu().numpy().reshape(a.B, -1)
    feat_h, pos_h, bal_h, dist_h = feat.cpu().numpy(), pos.cpu().numpy(), bal_pos.cpu().numpy(), dist.cpu().numpy()
    np.random.seed(0)
    rad, cls = {"diverse": [], "random": [], "balanced": []}, {"diverse": [], "random": [], "balanced": []}
    for b in range(a.B):
        ok = excl_h[b][cand_h[b]] == 0
        picks = {"diverse": pos_h[b], "random": np.random.choice(M, K, False), "balanced": bal_h[b]}
        for name, p in picks.items():
            rad[name].append(radius(feat_h[b], ok, p))
            cls[name].append(len(set(pred_h[b][cand_h[b][p]].tolist())))
    say(f" final k-centre radius of the {K} picks (squared byte distance, mean over {a.B} images): diverse_picks {np.mean(rad['diverse']):.0f}, "
        f"the reference's random sub-sample {np.mean(rad['random']):.0f}, class_balanced {np.mean(rad['balanced']):.0f} "
        f"(its square root in probability units: {np.sqrt(np.mean(rad['diverse'])) / 255:.3f} / {np.sqrt(np.mean(rad['random'])) / 255:.3f} / "
        f"{np.sqrt(np.mean(rad['balanced'])) / 255:.3f}); the last pick's own distance {dist_h[:, -1].mean():.0f}")
    say(f" distinct predicted classes among the {K} picks: diverse_picks {np.mean(cls['diverse']):.2f}, the reference's random sub-sample "
        f"{np.mean(cls['random']):.2f}, class_balanced {np.mean(cls['balanced']):.2f}; greedy picks per image: min {int(n.min())}")
    say(" a whole round and real pools were not measured")


if __name__ == "__main__":
    main()
