#!/usr/bin/env python3
"""Generate the visualiser fixture by IMPORTING the reference (authoring container only).

Runs only where the reference checkout exists.  Writes tests/golden/vis_panels.npz: data only (inputs + the reference's
outputs and its palette tables as arrays); no reference source is copied.

Reference call sites exercised:
  deeplab.py:55-56         F.interpolate(pred, size, mode='bilinear', align_corners=True)   (model.py:191: the VOC crop)
  model.py:124,150-156     softmax / argmax / Model._query x 3 / -ms
  utils/utils.py:376-453   Visualiser._preprocess, _make_grid, __call__

Cases (tests/test_vis_lowres_gpu.py cases A and B):
  a   Cityscapes-like  2 x 19 x (10,18) -> (40,72) cropped to (37,70), uint8 labels 0..19 (19 = void)
  b   VOC              1 x 21 x (10,18) -> (40,72), int64 labels 0..20 and 255
Per case and image: the low-resolution logits (randn * 3, seeded), x, y, the reference's prediction and three float maps, its
pre-resize byte panels (Visualiser._preprocess(t, seg, downsample=1): Pillow returns a copy at equal size); for image 0 the
final grid of Visualiser.__call__ (downsample 2, written to a PNG and read back) and the five-panel grid with target=None.
"""
import os
import sys
import tempfile

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_acq import REF  # noqa: E402,F401  (the reference checkout, put on sys.path there)
from model import Model  # noqa: E402
from utils import utils as ref_utils  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")

CASES = [("a", "cs", (2, 19, 10, 18), (40, 72), (37, 70), 5100),
         ("b", "voc", (1, 21, 10, 18), (40, 72), None, 5200)]


def labels(tag, rng, b, c, hc, wc):
    y = rng.randint(0, c, size=(b, hc, wc))
    if tag == "a":
        y[rng.rand(b, hc, wc) < 0.1] = c            # void
        return y.astype(np.uint8)
    y[rng.rand(b, hc, wc) < 0.1] = 255
    return y.astype(np.int64)


def f64_shares(logits, maps32):
    """The share of pixels the GPU tests' float64 restatement guards as exact (q more than 0.01 from an integer; top-two logit gap
    above 1e-4), printed so that the seeds can be seen to hold the tests' caps on the float64 side alone."""
    lg = logits.double()
    top2 = lg.topk(2, dim=0).values
    out = [float(((top2[0] - top2[1]) > 1e-4).float().mean())]
    p = lg.softmax(dim=0)
    t2 = p.topk(2, dim=0).values
    for v in (1.0 - p.max(dim=0)[0], -(t2[0] - t2[1]).abs(), (-p * p.log()).sum(dim=0)):
        t = v - v.min()
        q = t / (t.max() + 1e-7) * 255
        out.append(float(((q - q.round()).abs() > 0.01).float().mean()))
    return out


def main():
    os.makedirs(OUT, exist_ok=True)
    out = {}
    for name in ("cv", "cs", "voc"):
        pal = getattr(ref_utils, f"palette_{name}")
        keys = sorted(pal)
        out[f"palette_{name}_keys"] = np.array(keys, dtype=np.int64)
        out[f"palette_{name}_vals"] = np.array([list(pal[k]) for k in keys], dtype=np.uint8)
    tmp = tempfile.mkdtemp()
    for tag, ds, (b, c, h, w), size, crop, seed in CASES:
        torch.manual_seed(seed)
        rng = np.random.RandomState(seed)
        low = torch.randn(b, c, h, w) * 3
        hc, wc = size if crop is None else crop
        x = torch.randn(b, 3, hc, wc)
        y = labels(tag, rng, b, c, hc, wc)
        logits = F.interpolate(low, size=size, mode="bilinear", align_corners=True)[:, :, :hc, :wc]
        prob, pred = F.softmax(logits, dim=1), logits.argmax(dim=1)
        vis = ref_utils.Visualiser(ds)
        rgb = np.zeros((b, 3, hc, wc, 3), np.uint8)
        gray = np.zeros((b, 3, hc, wc), np.uint8)
        maps = np.zeros((b, 3, hc, wc), np.float32)
        for i in range(b):
            ent, lc, ms = [Model._query(prob[i:i + 1], uc)[0] for uc in ["entropy", "least_confidence", "margin_sampling"]]
            d = {'input': x[i], 'target': torch.from_numpy(y[i]), 'pred': pred[i], 'confidence': lc, 'margin': -ms, 'entropy': ent}
            maps[i] = np.stack([lc.numpy(), (-ms).numpy(), ent.numpy()])
            for j, (k, seg) in enumerate((('input', False), ('target', True), ('pred', True))):
                rgb[i, j] = np.asarray(vis._preprocess(d[k].clone(), seg=seg, downsample=1))
            for j, k in enumerate(('confidence', 'margin', 'entropy')):
                gray[i, j] = np.asarray(vis._preprocess(d[k].clone(), seg=False, downsample=1))
            if i == 0:
                for key, target in (("grid6", d['target']), ("grid5", None)):
                    fp = os.path.join(tmp, f"{tag}_{key}.png")
                    vis({k: (v.clone() if v is not None else None) for k, v in dict(d, target=target).items()}, fp=fp)
                    out[f"{tag}_{key}"] = np.asarray(Image.open(fp).convert("RGB"))
            print(tag, i, "float64 guarded shares (pred, confidence, margin, entropy):", f64_shares(logits[i], maps[i]))
        out[f"{tag}_low"] = low.numpy()
        out[f"{tag}_size"] = np.array(size, dtype=np.int64)
        out[f"{tag}_crop"] = np.array([hc, wc], dtype=np.int64)
        out[f"{tag}_x"] = x.numpy()
        out[f"{tag}_y"] = y
        out[f"{tag}_pred"] = pred.numpy().astype(np.uint8)
        out[f"{tag}_maps"] = maps                    # confidence, margin (negated), entropy: what model.py:150-156 hands over
        out[f"{tag}_rgb"] = rgb                      # input, target, pred before the resize
        out[f"{tag}_gray"] = gray                    # confidence, margin, entropy before the resize
    path = os.path.join(OUT, "vis_panels.npz")
    np.savez_compressed(path, **out)
    print("vis fixture written", os.path.getsize(path))


if __name__ == "__main__":
    main()
