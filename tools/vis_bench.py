#!/usr/bin/env python3
"""The per-epoch picture at 256 x 512 x 19: Visualiser.from_lowres (byte panels rendered from the classifier output on the GPU,
one copy) against the hook path it replaces (predict_lowres + three score_topk_lowres(return_map=True) launches, three float
maps read back, then the generic Visualiser.__call__), the host part broken down into resize and PNG encoding, and the driver's
epoch (Model._train_epoch + Model._val on synthetic data) with the pictures on against off.

One process, warmed up; wall-clock times with a device synchronisation on both sides (the picture ends in a file, so the host
is part of it); the variants alternate inside every repetition and min .. max over the repetitions is printed beside the median.

    python tools/vis_bench.py [--reps 7] [--epochs 3]
"""
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
from pixelpick_amd import acquisition as acq  # noqa: E402
from pixelpick_amd.model import Model  # noqa: E402
from pixelpick_amd.predict import predict_lowres  # noqa: E402
from pixelpick_amd.synthetic import SyntheticDataset  # noqa: E402
from pixelpick_amd.trainer import FlatTrainer  # noqa: E402
from pixelpick_amd.utils.utils import Visualiser, get_model  # noqa: E402
from pixelpick_amd.visualise import compose, render_lowres  # noqa: E402

DEV = "cuda:0"
C, H, W = 19, 256, 512


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def cell(v):
    return f"{float(np.median(v)):8.3f} ms ({min(v):.3f}..{max(v):.3f})"


def pictures(reps, td):
    torch.manual_seed(0)
    low = torch.randn(1, H // 4, W // 4, C, device=DEV) * 3
    x = torch.randn(1, 3, H, W, device=DEV)
    y = torch.randint(0, C + 1, (1, H, W), device=DEV)
    size = (H, W)
    vis = Visualiser("cs")

    def fused():
        vis.from_lowres(low, size, x, y, f"{td}/fused.png")

    def hook():
        pred = predict_lowres(low, size)[0]
        ent, lc, ms = [acq.score_topk_lowres(low, size, None, uc, 0, return_map=True)[2][0].cpu()
                       for uc in ("entropy", "least_confidence", "margin_sampling")]
        vis({'input': x[0].cpu(), 'target': y[0].cpu(), 'pred': pred[0].to(torch.int64).cpu(), 'confidence': lc, 'margin': -ms,
             'entropy': ent}, fp=f"{td}/hook.png")

    def device_only():
        render_lowres(low, size, image=x, target=y, palette=vis.palette)

    def device_and_copy():
        render_lowres(low, size, image=x, target=y, palette=vis.palette)["buffer"].cpu()

    out = render_lowres(low, size, image=x, target=y, palette=vis.palette)
    rgb, gray = out["rgb"].cpu().numpy()[0], out["gray"].cpu().numpy()[0]
    panels = [rgb[0], rgb[1], rgb[2], gray[0], gray[1], gray[2]]
    grid = compose(panels)

    def resize():
        compose(panels)

    def encode():
        grid.save(f"{td}/encode.png")

    variants = [("from_lowres (fused), per picture", fused), ("hook path (4 launches, 3 maps, __call__), per picture", hook),
                ("  render_lowres, launches only", device_only), ("  render_lowres + the one copy", device_and_copy),
                ("  host: 6 x fromarray + resize + paste", resize), ("  host: PNG encoding of the grid", encode)]
    for _, fn in variants:
        for _ in range(2):
            fn()
    t = [[] for _ in variants]
    for _ in range(reps):
        for i, (_, fn) in enumerate(variants):
            t[i].append(wall_ms(fn))
    print(f"one picture, {H} x {W} x {C} (low {H // 4} x {W // 4}), grid {grid.size[0]} x {grid.size[1]}:")
    for (name, _), v in zip(variants, t):
        print(f"  {name:55s} {cell(v)}")
    f, h = float(np.median(t[0])), float(np.median(t[1]))
    print(f"  hook / fused = {h / f:.2f}x" + ("" if f < h else "   (the fused path is NOT faster in this run)"))
    from PIL import Image
    same = np.array_equal(np.asarray(Image.open(f"{td}/fused.png")), np.asarray(Image.open(f"{td}/hook.png")))
    print(f"  the two files are pixel-equal: {same}")


def driver(epochs, td):
    n = int(os.environ.get("N", 128))
    ds = SyntheticDataset(n, H, W, C, C, n_init_pixels=20, seed=1)
    ds_val = SyntheticDataset(16, H, W, C, C, seed=2)
    mk = lambda d, b, sh: torch.utils.data.DataLoader(d, batch_size=b, shuffle=sh, drop_last=True)
    args = Namespace(dataset_name="cs", debug=False, dir_root=td, experim_name="drv", ignore_index=C, mc_n_steps=20, n_classes=C,
                     n_pixels_by_us=10, network_name="deeplab", weight_type="random", query_strategy="entropy", reverse_order=False,
                     stride_total=16, top_n_percent=0.0, use_mc_dropout=False, vote_type="hard", mc_dropout_p=0.2, n_init_pixels=20,
                     max_budget=20, n_epochs=1, lr_scheduler_type="Poly",
                     optimizer_params={"lr": 5e-4, "betas": (0.9, 0.999), "weight_decay": 2e-4, "eps": 1e-7})
    dev = torch.device(DEV)
    m = Model(args, mk(ds, 4, True), mk(ds, 1, False), mk(ds_val, 1, False), device=dev)
    m._open_logs(td)
    os.makedirs(f"{m.dir_checkpoints}/{m.nth_query}_query", exist_ok=True)
    model = get_model(args).to(dev)
    tr = FlatTrainer(model, lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=2e-4, ignore_index=C)
    vis = Visualiser("cs")

    def epoch(e, on):
        m._visualise, m.vis = on, (vis if on else None)
        m._train_epoch(e, model, tr, 1000)
        m._val(e, model)

    t = {False: [], True: []}
    with contextlib.redirect_stdout(io.StringIO()):
        for on in (False, True):
            epoch(1, on)                                # warm-up (records the replayed step, first launches of the picture)
        for e in range(epochs):
            for on in (False, True):
                t[on].append(wall_ms(lambda: epoch(2 + e, on)))
    print(f"driver epoch ({n} train images in batches of 4 + 16 validation images; the parent's loop = pictures off):")
    print(f"  pictures off  {cell(t[False])}")
    print(f"  pictures on   {cell(t[True])}   (+{float(np.median(t[True])) - float(np.median(t[False])):.2f} ms for two pictures)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--epochs", type=int, default=3)
    a = ap.parse_args()
    warnings.simplefilter("ignore")
    print(f"tools/vis_bench.py --reps {a.reps} --epochs {a.epochs}   ({torch.cuda.get_device_name(0)})")
    with tempfile.TemporaryDirectory() as td:
        pictures(a.reps, td)
        driver(a.epochs, td)


if __name__ == "__main__":
    main()
