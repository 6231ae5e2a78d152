"""GPU tests of pp_predict_lowres (csrc/predict.hip) through pixelpick_amd.predict.predict_lowres and
RunningScore.update_from_lowres: the label map and the confusion matrix taken straight from the low-resolution classifier output,
  * bit for bit against the pair of launches it replaces (pp_bilinear_fwd -> crop -> pp_confusion_matrix_update, argmax of the
    same tensor on the CPU), with int64 and uint8 targets,
  * against the CPU oracle (oracle.acq.bilinear_resize + argmax) and the reference-generated fixture
    (tests/golden/eval_lowres.npz, tools/gen_golden_eval.py) wherever the top-2 logit gap exceeds 1e-4 - over 10x the
    interpolation error the suite allows on logits of magnitude <~ 15 (test_interpolated_logits_match_golden: rtol 1e-5, atol
    2e-6) - with the share of pixels the guard leaves out capped at 0.05 %."""
import os

import numpy as np
import pytest
import torch

from oracle import acq as orc
from pixelpick_amd import _lib
from pixelpick_amd import engine as E
from pixelpick_amd.predict import predict_lowres
from pixelpick_amd.utils.metrics import RunningScore

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 1e-4
MAX_UNGUARDED = 5e-4

CASES = [
    # B, C, (h,w), (H,W), crop, align
    (2, 19, (16, 32), (64, 128), None, True),
    (1, 11, (23, 31), (67, 101), None, True),               # ragged
    (3, 21, (40, 40), (160, 160), (157, 150), True),        # VOC crop
    (2, 19, (32, 64), (64, 128), None, False),              # FPN x2
    (2, 7, (40, 60), (20, 30), None, True),                 # down-sampling
    (2, 40, (12, 20), (48, 80), None, True),
    (1, 104, (6, 10), (24, 40), None, True),                # largest histogram
    (2, 19, (16, 32), (16, 32), None, True),                # identity
    (1, 19, (200, 300), (25, 40), None, True),              # patch exceeds LDS -> global-read variant
    (4, 19, (64, 128), (256, 512), None, True),             # many tiles per image (32-row tiles, grid-stride walk)
]
IDS = [f"B{c[0]}C{c[1]}_{c[2][0]}x{c[2][1]}to{c[3][0]}x{c[3][1]}" for c in CASES]


def _low_np(case):
    B, C, (h, w), _, _, _ = case
    return (np.random.RandomState(1000 + C + h).randn(B, C, h, w) * 3).astype(np.float32)


def _nhwc(low_nchw: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(low_nchw.transpose(0, 2, 3, 1))).to(DEV)


def _targets(case, kind):
    """[B,Hc,Wc] labels with ~10 % ignored pixels drawn from {C, 255} (and -1 for int64); the last image is ignored entirely."""
    B, C, _, size, crop, _ = case
    hc, wc = size if crop is None else crop
    rng = np.random.RandomState(77 + C + hc)
    y = rng.randint(0, C, size=(B, hc, wc)).astype(np.int64)
    ign = rng.rand(B, hc, wc) < 0.1
    pool = np.array([C, 255] + ([-1] if kind == "int64" else []), dtype=np.int64)
    y[ign] = pool[rng.randint(0, len(pool), size=int(ign.sum()))]
    if B > 1:
        y[B - 1] = pool[rng.randint(0, len(pool), size=(hc, wc))]
    return torch.from_numpy(y if kind == "int64" else y.astype(np.uint8))


_PAIR = {}


def _pair(ci):
    """The two-launch path the fused call replaces, computed once per case and never modified: the cropped full-resolution logits
    on the device and their argmax taken on the CPU."""
    if ci not in _PAIR:
        B, C, lo, size, crop, align = CASES[ci]
        low = _nhwc(_low_np(CASES[ci]))
        logits = E.bilinear(E.Tape(False), E.Var(low), size, align, 0.0, out_nchw=True).t
        if crop is not None:
            logits = logits[:, :, :crop[0], :crop[1]].contiguous()
        _PAIR[ci] = (low, logits, logits.cpu().argmax(dim=1).to(torch.uint8))
    return _PAIR[ci]


def _pair_hist(logits, y):
    B, C, H, W = logits.shape
    hist = torch.zeros((C, C), dtype=torch.int64, device=DEV)
    rc = _lib.lib().pp_confusion_matrix_update(logits.data_ptr(), B, C, H * W, logits.stride(0), logits.stride(1),
                                               y.to(DEV, torch.int64).contiguous().data_ptr(), hist.data_ptr(), _lib.current_stream_ptr())
    _lib.check(rc, "pp_confusion_matrix_update")
    return hist


@pytest.mark.parametrize("kind", ["int64", "uint8"])
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_fused_equals_the_pair_it_replaces_bit_for_bit(ci, kind):
    B, C, lo, size, crop, align = CASES[ci]
    low, logits, pred_ref = _pair(ci)
    y = _targets(CASES[ci], kind)
    hist_ref = _pair_hist(logits, y)
    hist = torch.zeros((C, C), dtype=torch.int64, device=DEV)
    pred, h = predict_lowres(low, size, crop=crop, align_corners=align, target=y.to(DEV), hist=hist)
    assert h is hist and pred.dtype == torch.uint8 and tuple(pred.shape) == tuple(y.shape)
    assert torch.equal(pred.cpu(), pred_ref)
    assert torch.equal(hist, hist_ref)
    n_valid = int(((y.to(torch.int64) >= 0) & (y.to(torch.int64) < C)).sum())
    assert int(hist.sum()) == n_valid and n_valid > 0


@pytest.mark.parametrize("ci", [0, 2, 6, 8, 9], ids=[IDS[i] for i in (0, 2, 6, 8, 9)])
def test_accumulation_determinism_and_single_outputs(ci):
    B, C, lo, size, crop, align = CASES[ci]
    low, logits, pred_ref = _pair(ci)
    y = _targets(CASES[ci], "int64").to(DEV)
    hist = torch.zeros((C, C), dtype=torch.int64, device=DEV)
    pred1, _ = predict_lowres(low, size, crop=crop, align_corners=align, target=y, hist=hist)
    once = hist.clone()
    pred2, _ = predict_lowres(low, size, crop=crop, align_corners=align, target=y, hist=hist)
    assert torch.equal(hist, 2 * once), "hist is accumulated into: two calls give the sum"
    assert torch.equal(pred1, pred2)
    again = torch.zeros_like(hist)
    predict_lowres(low, size, crop=crop, align_corners=align, target=y, hist=again)
    assert torch.equal(again, once), "two identical runs give identical counts"
    h_only = torch.zeros_like(hist)
    p_none, _ = predict_lowres(low, size, crop=crop, align_corners=align, target=y, hist=h_only, want_pred=False)
    assert p_none is None and torch.equal(h_only, once)
    p_only, h_none = predict_lowres(low, size, crop=crop, align_corners=align)
    assert h_none is None and torch.equal(p_only, pred1)


def test_exact_ties_take_the_first_maximum():
    case = CASES[0]
    low_np = _low_np(case)
    low_np[:, 3] += 100.0
    low_np[:, 7] = low_np[:, 3]
    low_np[:, 12] = low_np[:, 3]
    pred, _ = predict_lowres(_nhwc(low_np), case[3])
    assert (pred == 3).all()
    case = CASES[8]                                    # the global-read variant
    low_np = _low_np(case)
    low_np[:, 3] += 100.0
    low_np[:, 7] = low_np[:, 3]
    low_np[:, 12] = low_np[:, 3]
    pred, _ = predict_lowres(_nhwc(low_np), case[3])
    assert (pred == 3).all()


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_against_the_cpu_oracle(ci):
    B, C, lo, size, crop, align = CASES[ci]
    low, _, _ = _pair(ci)
    ref = orc.bilinear_resize(_low_np(CASES[ci]), size, align_corners=align)
    if crop is not None:
        ref = ref[:, :, :crop[0], :crop[1]]
    lab = ref.argmax(axis=1)
    top2 = np.partition(ref, C - 2, axis=1)[:, C - 2:]
    ok = (top2[:, 1] - top2[:, 0]) > GUARD
    share = 1.0 - ok.mean()
    print(f"{IDS[ci]}: unguarded share {share:.6f}")
    assert share <= MAX_UNGUARDED
    pred, _ = predict_lowres(low, size, crop=crop, align_corners=align)
    np.testing.assert_array_equal(pred.cpu().numpy()[ok], lab[ok])


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "eval_lowres.npz"))


@pytest.mark.parametrize("tag", ["cv", "voc"])
def test_against_the_reference_fixture(g, tag):
    low = _nhwc(g[f"{tag}_low"])
    C = low.shape[3]
    size, crop = tuple(int(v) for v in g[f"{tag}_size"]), tuple(int(v) for v in g[f"{tag}_crop"])
    ok = g[f"{tag}_gap"] > GUARD
    n_un = int((~ok).sum())
    assert n_un / ok.size <= MAX_UNGUARDED
    y = g[f"{tag}_y"]
    # the confusion matrix restricted to the guarded pixels: the others are handed over as ignored
    y_guard = np.where(ok, y, 255).astype(np.uint8)
    hist = torch.zeros((C, C), dtype=torch.int64, device=DEV)
    pred, _ = predict_lowres(low, size, crop=crop, target=torch.from_numpy(y_guard).to(DEV), hist=hist)
    pred = pred.cpu().numpy()
    np.testing.assert_array_equal(pred[ok], g[f"{tag}_pred"][ok])
    m = ok & (y < C)
    want = np.bincount(C * y[m].astype(np.int64) + g[f"{tag}_pred"][m], minlength=C * C).reshape(C, C)
    np.testing.assert_array_equal(hist.cpu().numpy(), want)
    # the scores over ALL pixels: at most n_un pixels may sit in another cell
    for ydev in (torch.from_numpy(y).to(DEV), torch.from_numpy(y.astype(np.int64))):
        rs = RunningScore(C)
        s = rs.update_from_lowres(ydev, low, size, crop=crop).get_scores()[0]
        counted = int((y < C).sum())
        assert rs.confusion_matrix.sum() == counted == g[f"{tag}_hist"].sum()
        tol = 2.0 * n_un / counted
        assert abs(s["Mean IoU"] - float(g[f"{tag}_miou"])) <= tol
        assert abs(s["Pixel Acc"] - float(g[f"{tag}_pixel_acc"])) <= tol
        if n_un == 0:
            np.testing.assert_array_equal(rs.confusion_matrix, g[f"{tag}_hist"])


def test_errors():
    err = (ValueError, _lib.PixelPickHipError)
    low = _nhwc(_low_np(CASES[0]))
    size = CASES[0][3]
    y = torch.zeros((2,) + size, dtype=torch.int64, device=DEV)
    hist = torch.zeros((19, 19), dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.PixelPickHipError):
        predict_lowres(low.cpu(), size)                                      # CPU tensor
    with pytest.raises(err):
        predict_lowres(low, size, crop=(65, 128))                            # crop > size
    with pytest.raises(err):
        predict_lowres(low, size, crop=(64, 129))
    with pytest.raises(ValueError):
        predict_lowres(low.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1), size)      # NCHW memory: not channels-last
    with pytest.raises(err):                                                 # C = 105 with hist
        predict_lowres(torch.zeros((1, 4, 4, 105), device=DEV), (8, 8), target=torch.zeros((1, 8, 8), dtype=torch.int64, device=DEV),
                       hist=torch.zeros((105, 105), dtype=torch.int64, device=DEV))
    assert predict_lowres(torch.zeros((1, 4, 4, 105), device=DEV), (8, 8))[0].shape == (1, 8, 8)    # pred alone takes C <= 256
    with pytest.raises(err):
        predict_lowres(low, size, target=y[:, :-1], hist=hist)               # target shape
    with pytest.raises(err):
        predict_lowres(low, size, target=y.to(torch.int32), hist=hist)       # target dtype
    with pytest.raises(err):
        predict_lowres(low, size, target=y.cpu(), hist=hist)                 # target on the host
    with pytest.raises(err):
        predict_lowres(low, size, target=y, hist=hist.to(torch.int32))       # hist dtype
    with pytest.raises(err):
        predict_lowres(low, size, target=y)                                  # target without hist
    with pytest.raises(err):
        predict_lowres(low, size, want_pred=False)                           # both outputs null
    with pytest.raises(err):
        RunningScore(11).update_from_lowres(y, low, size)                    # class count mismatch
    assert int(hist.sum()) == 0
