#!/usr/bin/env python3
"""MC-dropout acquisition round (query.py:176-188 as intended: mean over mc_n_steps stochastic passes) through the real
DeepLabv3+-MobileNetV2, 16 images of 256x512, 19 classes, entropy, device-synchronised wall time per round:

  * the full-size route (all passes of an image in one forward, pp_bilinear_fwd -> pp_acq_softmax_sum -> pp_topk_select, mean
    probability map read back for the statistics) against the route from the classifier output (pp_acq_lowres_mc_score_topk /
    pp_acq_lowres_mc_score_at) - same process, alternating, `--repeats` rounds each after a warm-up round of every route; the
    spread of the full-size route's repeats is the run's own noise;
  * --chunks: all passes in one forward (mc_chunk = 32) vs one forward per pass (mc_chunk = 1), the earlier record;
  * --vote_type hard (args.py:34): the same two routes with the hard vote (pp_acq_lowres_mc_vote_topk / pp_acq_vote_accumulate +
    pp_acq_vote_score_map), the classifier-output route with the soft vote beside them, and the scorer call alone - the vote scorer
    next to the soft scorer at one image's shape (device events over `--scorer_calls` calls, `--repeats` blocks each, alternating;
    the spread of the soft scorer's blocks is the run's own noise);
  * --vote_type consensus / --query_strategy bald: the scores of the mean probability and the mutual information
    (pp_acq_lowres_mc_mean_topk / pp_acq_softmax_sum + pp_acq_mean_prob_score_map) on both routes, with TWO selectors of the soft
    classifier-output route beside them in the same run: the ratio to the soft route is stated next to the difference between those
    two, the run's own noise.  The 20 forwards dominate a round: no gain is expected or claimed.

    python tools/mc_dropout_bench.py [--repeats 3] [--images 16] [--steps 20] [--chunks] [--only lowres|full]
                                     [--vote_type soft|hard|consensus] [--query_strategy entropy|least_confidence|margin_sampling|bald]
                                     [--scorer_calls 200] [--out FILE]
(--only: one route alone, for a kernel trace of it.)"""
import argparse
import contextlib
import io
import os
import sys
import tempfile
import time
import warnings
from argparse import Namespace

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pixelpick_amd import acquisition as acq
from pixelpick_amd import query as ppq
from pixelpick_amd.utils.utils import get_model

warnings.simplefilter("ignore")
C, h, w = 19, 256, 512


class DS:
    def __init__(s, n):
        s.xs = torch.randn(n, 3, h, w); s.ys = torch.randint(0, C, (n, h, w)); s.queries = [np.zeros((h, w), bool) for _ in range(n)]

    def label_queries(s, d, k):
        pass


class DL:
    def __init__(s, d):
        s.dataset = d

    def __iter__(s):
        for i in range(len(s.dataset.xs)):
            yield {"x": s.dataset.xs[i][None], "y": s.dataset.ys[i][None], "p_img": [f"/i{i}.png"]}


def one_round(qs, model, nth):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        qs(nth, model)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def scorer_times(steps, repeats, calls, say):
    """The scorer call of ONE image (B = 1, the selector's launch) on random classifier-output logits: microseconds per call."""
    low = torch.randn(steps, h // 4, w // 4, C, device="cuda:0") * 3
    excl = torch.zeros(1, h, w, dtype=torch.uint8, device="cuda:0")
    fns = [("soft scorer (acq_lowres_mc_kernel)", lambda: acq.mc_score_topk_lowres(low, steps, (h, w), excl, "entropy", 20)),
           ("vote scorer (acq_lowres_mc_vote_kernel)", lambda: acq.mc_vote_topk_lowres(low, steps, (h, w), excl, "entropy", 20))]
    us = [[] for _ in fns]
    for rep in range(repeats + 1):                             # block 0 of each: warm-up
        for i, (_, fn) in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if rep:
                us[i].append(e0.elapsed_time(e1) * 1e3 / calls)
    say(f"scorer call alone (scorer + candidate merge + wrapper), 1 image {h}x{w} from {h // 4}x{w // 4}, C={C}, T={steps}, entropy, k=20; "
        f"{repeats} blocks of {calls} calls, alternating")
    for (name, _), u in zip(fns, us):
        say(f"  {name:48s} {np.mean(u):8.1f} us/call  (blocks: {', '.join(f'{x:.1f}' for x in u)}; spread {max(u) - min(u):.1f})")
    say(f"  vote / soft: {np.mean(us[1]) / np.mean(us[0]):.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--chunks", action="store_true")
    ap.add_argument("--only", choices=["lowres", "full"], default=None)
    ap.add_argument("--vote_type", choices=["soft", "hard", "consensus"], default="soft")
    ap.add_argument("--query_strategy", choices=["entropy", "least_confidence", "margin_sampling", "bald"], default="entropy")
    ap.add_argument("--scorer_calls", type=int, default=200)
    ap.add_argument("--out", default=None)
    o = ap.parse_args()
    n = o.images
    model = get_model(Namespace(use_mc_dropout=True, mc_dropout_p=0.2, n_classes=C, network_name="deeplab", weight_type="random")).cuda()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    with tempfile.TemporaryDirectory() as td:
        def selector(**kw):
            a = Namespace(dataset_name="cs", debug=False, dir_root=td, experim_name="mc", ignore_index=C, mc_n_steps=o.steps, n_classes=C,
                          n_pixels_by_us=20, network_name="deeplab", weight_type="random", reverse_order=False, stride_total=16, top_n_percent=0.0,
                          use_mc_dropout=True, mc_chunk=32, **dict(dict(vote_type=o.vote_type, query_strategy=o.query_strategy), **kw))
            return ppq.QuerySelector(a, DL(DS(n)), device=torch.device("cuda:0"))

        routes = [("full-size route", False), ("classifier-output route", True)]
        if o.only:
            routes = [r for r in routes if r[1] == (o.only == "lowres")][:1]
        sels = [selector() for _ in routes]
        if o.vote_type == "hard":
            routes = [(f"{name}, hard vote", fused) for name, fused in routes]
            if o.only != "full":
                routes.append(("classifier-output route, soft vote", True))
                sels.append(selector(vote_type="soft"))
        mean_mode = o.vote_type == "consensus" or o.query_strategy == "bald"
        if mean_mode:
            mode = "BALD" if o.query_strategy == "bald" else f"consensus {o.query_strategy}"
            routes = [(f"{name}, {mode}", fused) for name, fused in routes]
            if o.only != "full":
                for tag in ("a", "b"):
                    routes.append((f"classifier-output route, soft vote ({tag})", True))
                    sels.append(selector(vote_type="soft", query_strategy="entropy" if o.query_strategy == "bald" else o.query_strategy))
        times = [[] for _ in routes]
        for rep in range(o.repeats + 1):                       # round 0 of every route: warm-up
            for i, (_, fused) in enumerate(routes):
                ppq.FUSED_LOWRES = fused
                t = one_round(sels[i], model, rep + 1)
                if rep:
                    times[i].append(t)
        say(f"MC-dropout acquisition round, {n} images {h}x{w}, C={C}, mc_n_steps={o.steps}, vote_type={o.vote_type}, {o.query_strategy}, k=20; "
            f"{o.repeats} rounds per route, alternating")
        rates = []
        for (name, _), ts in zip(routes, times):
            r = [n / t for t in ts]
            rates.append(r)
            say(f"  {name:48s} {np.mean(r):7.1f} images/s  (rounds: {', '.join(f'{x:.1f}' for x in r)}; spread {max(r) - min(r):.1f})")
        if len(rates) >= 2 and not o.only:
            say(f"  ratio to the full-size route: {np.mean(rates[1]) / np.mean(rates[0]):.2f}x")
        if mean_mode and not o.only:
            new, sa, sb = (float(np.mean(r)) for r in rates[1:4])
            say(f"  classifier-output route, {mode} / soft vote: {new / ((sa + sb) / 2):.3f}  (the two soft selectors of this run: "
                f"{sa:.1f} and {sb:.1f} images/s, {abs(sa - sb) / ((sa + sb) / 2) * 100:.1f} % apart); no pass/fail bar")
        if o.vote_type == "hard":
            scorer_times(o.steps, o.repeats, o.scorer_calls, say)
        if o.chunks:
            ppq.FUSED_LOWRES = False
            for chunk in (32, 1):
                qs = selector()
                qs.mc_chunk = chunk
                one_round(qs, model, 1)
                say(f"  full-size route, mc_chunk={chunk:2d}: {n / one_round(qs, model, 2):6.1f} images/s")
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
