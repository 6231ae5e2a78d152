"""pp_vis_lowres (csrc/vis.hip) through visualise.render_lowres: the picture's byte panels from the classifier-resolution logits.

Check 1  against this library's own entries, exact on every pixel (predict_lowres, score_topk_lowres's maps, the fp32 formula).
Check 2  against a float64 restatement in torch on the CPU (and, for the fixture's cases, the reference's own panels): within one
         grey level everywhere and equal wherever the float64 value is not within 0.01 of a rounding boundary; the prediction equal
         wherever the float64 top-two logit gap exceeds 1e-4.  fp32 torch against float64 differs by at most 9.7e-4 in q on these
         shapes, so 0.01 leaves 10x; the guarded shares are asserted (>= 0.95 per gray panel, >= 0.99 for the prediction).
Check 3  NaN entropy (0 * log 0): skipped by min / max, drawn 0, the other image of the batch untouched.
Check 4  a head wider than 64 classes is refused.
The shapes are the smallest that reach a second column tile, ragged right and bottom edges, the crop, both interpolation modes
and per-image ranges; G is the smallest down-sampling case whose patch does not fit the block's LDS."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pixelpick_amd import _lib
from pixelpick_amd import acquisition as acq
from pixelpick_amd.predict import predict_lowres
from pixelpick_amd.visualise import PALETTES, render_lowres

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vis_panels.npz")

#        C   low       size      crop      align  B  scale palette seed
SHAPES = {
    "C": (5, (20, 36), (40, 72), (37, 70), False, 2, 3.0, "cv", 5300),
    "D": (19, (16, 32), (64, 128), None, True, 3, 1.0, "cs", 5400),
    "E": (64, (6, 10), (24, 40), None, True, 1, 3.0, "cv", 5500),
    # x1/2: a 16 x 64 tile interpolates from 33 x 129 source pixels, 323 KB at C = 19 - past the 48 KB a block stages, so every
    # lane reads its four neighbours from memory (vis_score_kernel<..., LDS = false>); two tiles each way, both ragged
    "G": (19, (40, 140), (20, 70), None, False, 1, 3.0, "cs", 5600),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(low [B,C,h,w] f32, x, y | None, size, crop, align, palette) on the CPU, never modified."""
    if name in ("A", "B", "F"):
        g = np.load(GOLDEN)
        tag = "b" if name == "B" else "a"
        d = dict(low=torch.from_numpy(g[f"{tag}_low"]), x=torch.from_numpy(g[f"{tag}_x"]), y=torch.from_numpy(g[f"{tag}_y"]),
                 size=tuple(int(v) for v in g[f"{tag}_size"]), crop=tuple(int(v) for v in g[f"{tag}_crop"]), align=True,
                 palette=PALETTES["voc" if name == "B" else "cs"], ref_rgb=g[f"{tag}_rgb"], ref_gray=g[f"{tag}_gray"])
        if name == "F":
            d.update(x=None, y=None)
        return d
    C, (h, w), size, crop, align, B, scale, pal, seed = SHAPES[name]
    torch.manual_seed(seed)
    hc, wc = crop or size
    return dict(low=torch.randn(B, C, h, w) * scale, x=torch.randn(B, 3, hc, wc), y=None, size=size, crop=crop or size, align=align,
                palette=PALETTES[pal])


def nhwc(low):
    return low.permute(0, 2, 3, 1).contiguous().cuda()


@functools.lru_cache(maxsize=None)
def rendered(name, plant=False):
    """One render of the case (+ the library's own label map and score maps from the same logits), fetched to the host."""
    c = case(name)
    low = c["low"].clone()
    if plant:
        low[0, 0, 0, 0] = 200.0
    lo = nhwc(low)
    x = c["x"].cuda() if c["x"] is not None else None
    y = c["y"].cuda() if c["y"] is not None else None
    out = render_lowres(lo, c["size"], image=x, target=y, palette=c["palette"], crop=c["crop"], align_corners=c["align"])
    pred = predict_lowres(lo, c["size"], crop=c["crop"], align_corners=c["align"])[0]
    maps = [acq.score_topk_lowres(lo, c["size"], None, uc, 0, crop=c["crop"], align_corners=c["align"], return_map=True)[2]
            for uc in ("least_confidence", "margin_sampling", "entropy")]
    torch.cuda.synchronize()
    maps = [m.cpu().numpy() for m in maps]
    maps[1] = -maps[1]
    return dict(rgb=out["rgb"].cpu().numpy(), gray=out["gray"].cpu().numpy(), ranges=out["ranges"].cpu().numpy(),
                panels=out["panels"], pred=pred.cpu().numpy(), maps=np.stack(maps, axis=1))


def quant32(v):
    """The header's formula in numpy fp32, every operation rounded on its own; min / max skip NaN, a NaN pixel is 0."""
    v = np.asarray(v, dtype=np.float32)
    mn = np.nanmin(v)
    t = v - mn
    d = np.float32(np.nanmax(t)) + np.float32(1e-7)
    q = (t / d) * np.float32(255.0)
    assert q.dtype == np.float32
    return np.clip(np.where(np.isnan(q), np.float32(0), q), 0, 255).astype(np.uint8)


def restate64(c):
    """float64 on the CPU: interpolate, crop, softmax, the three formulas, the normalisation.  -> (top-two logit gap, argmax,
    q [B,3,Hc,Wc] before truncation)."""
    hc, wc = c["crop"]
    lg = F.interpolate(c["low"].double(), size=c["size"], mode="bilinear", align_corners=c["align"])[:, :, :hc, :wc]
    top2 = lg.topk(2, dim=1).values
    p = lg.softmax(dim=1)
    t2 = p.topk(2, dim=1).values
    qs = []
    for v in (1.0 - p.max(dim=1)[0], -(t2[:, 0] - t2[:, 1]).abs(), (-p * p.log()).sum(dim=1)):
        t = v - v.amin(dim=(1, 2), keepdim=True)
        qs.append(t / (t.amax(dim=(1, 2), keepdim=True) + 1e-7) * 255)
    return (top2[:, 0] - top2[:, 1]).numpy(), lg.argmax(dim=1).numpy(), torch.stack(qs, dim=1).numpy()


ALL = ["A", "B", "C", "D", "E", "F", "G"]


@pytest.mark.parametrize("name", ALL)
def test_panels_equal_the_librarys_own_entries(name):
    c, r = case(name), rendered(name)
    B = c["low"].shape[0]
    hc, wc = c["crop"]
    want_panels = (["input"] if c["x"] is not None else []) + (["target"] if c["y"] is not None else []) + ["pred"]
    assert r["panels"] == want_panels and r["rgb"].shape == (B, len(want_panels), hc, wc, 3) and r["gray"].shape == (B, 3, hc, wc)
    assert np.array_equal(r["rgb"][:, want_panels.index("pred")], c["palette"][r["pred"]])
    for b in range(B):
        for j in range(3):
            assert r["ranges"][b, j + 1, 0] == r["maps"][b, j].min() and r["ranges"][b, j + 1, 1] == r["maps"][b, j].max(), (b, j)
            assert np.array_equal(r["gray"][b, j], quant32(r["maps"][b, j])), (b, j)
        if c["x"] is not None:
            xb = c["x"][b].numpy()
            assert r["ranges"][b, 0, 0] == xb.min() and r["ranges"][b, 0, 1] == xb.max()
            assert np.array_equal(r["rgb"][b, 0], quant32(xb).transpose(1, 2, 0))
        else:
            assert (r["ranges"][b, 0] == 0).all()
    if c["y"] is not None:
        y = c["y"].numpy().astype(np.int64)
        assert np.array_equal(r["rgb"][:, 1], c["palette"][y])           # every label of the cases is in 0..255
    assert len({tuple(r["ranges"][b, 3]) for b in range(B)}) == B        # per-image ranges


def test_without_image_and_target_the_other_outputs_do_not_change():
    a, f = rendered("A"), rendered("F")
    assert f["rgb"].shape[1] == 1 and np.array_equal(f["rgb"][:, 0], a["rgb"][:, 2])
    assert np.array_equal(f["gray"], a["gray"]) and np.array_equal(f["ranges"][:, 1:], a["ranges"][:, 1:])


def _guarded_check(tag, got_gray, got_pred_rgb, palette, gap, am, q):
    exact = np.abs(q - np.round(q)) > 0.01
    want = np.clip(np.floor(q), 0, 255).astype(np.int64)
    diff = np.abs(got_gray.astype(np.int64) - want)
    for b in range(q.shape[0]):
        for j in range(3):
            share = exact[b, j].mean()
            print(f"{tag} image {b} panel {j}: guarded share {share:.4f}, max |diff| {diff[b, j].max()}, "
                  f"differing guarded pixels {(diff[b, j][exact[b, j]] != 0).sum()}")
            assert share >= 0.95
    assert diff.max() <= 1
    assert (diff[exact] == 0).all()
    sure = gap > 1e-4
    print(f"{tag} prediction: guarded share {sure.mean():.4f}")
    assert sure.mean() >= 0.99
    assert np.array_equal(got_pred_rgb[sure], palette[am][sure])


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E", "G"])
def test_panels_against_float64(name):
    c, r = case(name), rendered(name)
    gap, am, q = restate64(c)
    _guarded_check(name, r["gray"], r["rgb"][:, r["panels"].index("pred")], c["palette"], gap, am, q)


@pytest.mark.parametrize("name", ["A", "B"])
def test_reference_panels_against_float64_and_ours(name):
    """The reference's own byte panels (fixture) hold the same bounds against float64; its input and target panels - fp32
    operations rounded one by one on both sides, a table lookup - are ours bit for bit."""
    c, r = case(name), rendered(name)
    gap, am, q = restate64(c)
    _guarded_check(name + " reference", c["ref_gray"], c["ref_rgb"][:, 2], c["palette"], gap, am, q)
    assert np.array_equal(r["rgb"][:, 0], c["ref_rgb"][:, 0])
    assert np.array_equal(r["rgb"][:, 1], c["ref_rgb"][:, 1])
    assert np.abs(r["gray"].astype(np.int64) - c["ref_gray"].astype(np.int64)).max() <= 1


def test_nan_entropy_is_skipped_by_the_range_and_drawn_black():
    c, r, base = case("A"), rendered("A", plant=True), rendered("A")
    nan = np.isnan(r["maps"][0, 2])
    assert nan.any() and not nan.all() and not np.isnan(r["maps"][1]).any()
    assert (r["gray"][0, 2][nan] == 0).all()
    assert np.isfinite(r["ranges"]).all()
    assert r["ranges"][0, 3, 0] == np.nanmin(r["maps"][0, 2]) and r["ranges"][0, 3, 1] == np.nanmax(r["maps"][0, 2])
    for j in range(3):
        assert np.array_equal(r["gray"][0, j], quant32(r["maps"][0, j])), j
    assert np.array_equal(r["rgb"][0, 2], c["palette"][r["pred"][0]])
    for k in ("rgb", "gray", "ranges"):
        assert np.array_equal(r[k][1], base[k][1]), k


def test_heads_wider_than_64_classes_are_refused():
    low = torch.zeros(1, 6, 10, 65, device="cuda")
    with pytest.raises(_lib.PixelPickHipError):
        render_lowres(low, (24, 40))
