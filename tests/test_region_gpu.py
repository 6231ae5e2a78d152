"""GPU tests of pp_acq_region_score_map (csrc/acq_select.hip, region_score_kernel) against the numpy oracle (tests/region_oracle.py).

The impurity is an integer computation: mode 1 must be BIT-equal.  The window uncertainty is an fp32 sum of K = (2r+1)^2 non-negative
terms, one division and one int -> float conversion, each at most 2^-24 relative, doubled: (K+2) 2^-23 relative to float64; the
product adds one multiplication and P's own division: (K+4) 2^-23.  The bounds are derived, not measured.  The shapes sit around the
kernel's tile (acquisition.REGION_TILE), at windows larger than the image, and at C = 256 where one wave holds the counts."""
import numpy as np
import pytest
import torch

import region_oracle as ro
from pixelpick_amd import _lib
from pixelpick_amd import acquisition as acq

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TH, TW = acq.REGION_TILE
# (B, H, W, C, r)
CASES = [(1, 5, 7, 3, 1), (1, 9, 11, 4, 16), (2, 37, 53, 19, 1), (2, TH - 1, TW + 1, 21, 2), (3, TH + 1, 2 * TW - 1, 11, 8),
         (2, 40, 70, 21, 16), (1, 70, 130, 256, 3)]
IDS = [f"B{b}_{h}x{w}_C{c}_r{r}" for b, h, w, c, r in CASES]
PATTERNS = ("iid", "blobs", "constant")
EPS = 2.0 ** -23


def _labels(pattern, rng, B, H, W, C):
    if pattern == "iid":
        lab = rng.randint(0, C, (B, H, W))
        if C == 256:
            lab.reshape(-1)[:256] = rng.permutation(256)          # every byte value is present
        return lab.astype(np.uint8)
    if pattern == "constant":
        return np.full((B, H, W), C - 1, dtype=np.uint8)
    # piecewise constant: every pixel takes the label of its nearest seed (realistic edges)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.empty((B, H, W), dtype=np.uint8)
    for b in range(B):
        n = rng.randint(2, 9)
        sy, sx, sl = rng.uniform(0, H, n), rng.uniform(0, W, n), rng.randint(0, C, n)
        out[b] = sl[np.argmin((yy[None] - sy[:, None, None]) ** 2 + (xx[None] - sx[:, None, None]) ** 2, axis=0)]
    return out


_inputs = {}


def _case(i, pattern):
    """(pred u8, unc f32 in [0, ln C], host and device) of a case, made once and left unchanged."""
    key = (i, pattern)
    if key not in _inputs:
        B, H, W, C, r = CASES[i]
        rng = np.random.RandomState(100 * i + PATTERNS.index(pattern))
        pred = _labels(pattern, rng, B, H, W, C)
        unc = (rng.rand(B, H, W) * np.log(C)).astype(np.float32)
        _inputs[key] = (pred, unc, torch.from_numpy(pred).to(DEV), torch.from_numpy(unc).to(DEV))
    return _inputs[key]


def _run(pred_d, unc_d, r, C, **kw):
    out = acq.region_score_map(pred_d, unc_d, r, C, **kw)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and out.is_contiguous()
    return out.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_rel(got, want64, bound, what):
    """|got - want| <= bound * |want| elementwise (want finite); prints the largest ratio before asserting."""
    got = got.astype(np.float64)
    err = np.abs(got - want64)
    lim = bound * np.abs(want64)
    worst = float((err / np.maximum(np.abs(want64), 1e-300)).max()) if err.size else 0.0
    print(f"{what}: max relative error {worst:.3e}, bound {bound:.3e}")
    assert (err <= lim).all(), (what, worst, bound)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_impurity_is_bit_equal_to_the_oracle(i, pattern):
    B, H, W, C, r = CASES[i]
    pred, _, pred_d, _ = _case(i, pattern)
    got = _run(pred_d, None, r, C, mode="impurity")
    assert got.shape == (B, H, W)
    for b in range(B):
        want = ro.impurity(pred[b], C, r)
        assert (_bits(got[b]) == _bits(want)).all(), (IDS[i], pattern, b)
    if pattern == "constant":
        assert (_bits(got) == 0).all()                            # exactly +0.0
    else:
        assert got.max() > 0


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_window_uncertainty_is_within_the_derived_bound(i, flip):
    B, H, W, C, r = CASES[i]
    _, unc, _, unc_d = _case(i, "iid")
    if flip:                                                      # 1 - unc must stay non-negative: a margin lies in [0, 1]
        unc = (unc / np.float32(np.log(C))).astype(np.float32).clip(0, 1)
        unc_d = torch.from_numpy(unc).to(DEV)
    got = _run(None, unc_d, r, C, mode="uncertainty", flip=flip)
    K = (2 * r + 1) ** 2
    for b in range(B):
        _assert_rel(got[b], ro.uncertainty64(unc[b], r, flip), (K + 2) * EPS, f"U {IDS[i]} flip={flip} image {b}")


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_product_is_within_the_derived_bound_and_zero_on_pure_windows(i, pattern):
    B, H, W, C, r = CASES[i]
    pred, unc, pred_d, unc_d = _case(i, pattern)
    got = _run(pred_d, unc_d, r, C, mode="product")
    K = (2 * r + 1) ** 2
    for b in range(B):
        P = ro.impurity(pred[b], C, r)
        _assert_rel(got[b], P.astype(np.float64) * ro.uncertainty64(unc[b], r), (K + 4) * EPS, f"P*U {IDS[i]} {pattern} image {b}")
        assert (got[b][P == 0] == 0.0).all()
    if pattern == "constant":
        assert (got == 0.0).all()


@pytest.mark.parametrize("i", [2, 4, 5], ids=[IDS[2], IDS[4], IDS[5]])
def test_an_image_of_a_batch_is_the_image_alone(i):
    """No halo leaks across images: image b of the batched call is bit-equal to the call on image b alone."""
    B, H, W, C, r = CASES[i]
    _, _, pred_d, unc_d = _case(i, "blobs")
    ex = torch.from_numpy(np.random.RandomState(i).rand(B, H, W) < 0.1).to(DEV)
    for mode in ("product", "impurity", "uncertainty"):
        full = _run(pred_d, unc_d, r, C, mode=mode, exclude=ex)
        for b in range(B):
            one = _run(pred_d[b:b + 1].contiguous(), unc_d[b:b + 1].contiguous(), r, C, mode=mode, exclude=ex[b:b + 1])
            assert (_bits(full[b]) == _bits(one[0])).all(), (mode, b)


@pytest.mark.parametrize("i", [3, 5], ids=[IDS[3], IDS[5]])
def test_a_nan_reaches_exactly_its_window(i):
    B, H, W, C, r = CASES[i]
    _, unc, pred_d, _ = _case(i, "iid")
    for (y, x) in ((H // 2, W // 2), (0, W - 1)):                 # one in the interior, one in a corner
        base = unc.copy()
        base[B - 1, y, x] = 0.5
        bad = base.copy()
        bad[B - 1, y, x] = np.nan
        win = np.zeros((B, H, W), dtype=bool)
        win[B - 1, max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1] = True
        for mode in ("uncertainty", "product"):
            want = _run(pred_d, torch.from_numpy(base).to(DEV), r, C, mode=mode)
            got = _run(pred_d, torch.from_numpy(bad).to(DEV), r, C, mode=mode)
            assert not np.isnan(want).any()
            assert (np.isnan(got) == win).all(), (mode, y, x)
            assert (_bits(got)[~win] == _bits(want)[~win]).all(), (mode, y, x)
        imp = _run(pred_d, None, r, C, mode="impurity")           # the impurity never reads unc
        assert not np.isnan(imp).any()


@pytest.mark.parametrize("i", [0, 4, 6], ids=[IDS[0], IDS[4], IDS[6]])
def test_exclusion_fills_the_centre_pixel_only(i):
    B, H, W, C, r = CASES[i]
    _, _, pred_d, unc_d = _case(i, "blobs")
    ex = np.random.RandomState(7 + i).rand(B, H, W) < 0.3
    for mode in ("product", "impurity", "uncertainty"):
        plain = _run(pred_d, unc_d, r, C, mode=mode)
        assert (plain >= 0).all()
        for mask in (ex, ex.astype(np.uint8) * 3, torch.from_numpy(ex).to(DEV)):
            got = _run(pred_d, unc_d, r, C, mode=mode, exclude=mask)
            assert (_bits(got)[ex] == _bits(np.float32(-1.0))).all()
            assert (_bits(got)[~ex] == _bits(plain)[~ex]).all()
        allx = _run(pred_d, unc_d, r, C, mode=mode, exclude=np.ones((B, H, W), dtype=bool))
        assert (allx == ro.FILL).all()


@pytest.mark.parametrize("i", [4, 5, 6], ids=[IDS[4], IDS[5], IDS[6]])
def test_two_runs_give_the_same_bits(i):
    B, H, W, C, r = CASES[i]
    _, _, pred_d, unc_d = _case(i, "iid")
    for mode in ("product", "impurity", "uncertainty"):
        a = _run(pred_d, unc_d, r, C, mode=mode)
        b = _run(pred_d, unc_d, r, C, mode=mode)
        assert (_bits(a) == _bits(b)).all(), mode


@pytest.mark.parametrize("i", [2, 5], ids=[IDS[2], IDS[5]])
def test_labels_past_the_class_count_share_one_bin(i):
    B, H, W, C, r = CASES[i]
    rng = np.random.RandomState(50 + i)
    pred = rng.randint(0, 256, (B, H, W)).astype(np.uint8)        # most bytes are >= C
    got = _run(torch.from_numpy(pred).to(DEV), None, r, C, mode="impurity")
    folded = _run(torch.from_numpy(np.minimum(pred, C).astype(np.uint8)).to(DEV), None, r, C + 1, mode="impurity")
    for b in range(B):
        assert (_bits(got[b]) == _bits(ro.impurity(pred[b], C, r))).all()
    assert (_bits(got) == _bits(folded)).all()


@pytest.mark.parametrize("k", [9, 49])
def test_selection_from_the_map_is_the_stable_ranking(k):
    i = 4
    B, H, W, C, r = CASES[i]
    _, _, pred_d, unc_d = _case(i, "blobs")
    ex = torch.from_numpy(np.random.RandomState(3).rand(B, H, W) < 0.05).to(DEV)
    for mode in ("product", "impurity"):                          # the impurity map is tie-heavy: the ties go to the lower index
        m = acq.region_score_map(pred_d, unc_d, r, C, exclude=ex, mode=mode)
        idx, val = acq.topk_select(m.reshape(B, H * W), k, True)
        torch.cuda.synchronize()
        mh = m.cpu().numpy()
        for b in range(B):
            want = ro.ranking(mh[b], k)
            assert idx[b].cpu().numpy().tolist() == want.tolist(), (mode, b)
            assert (_bits(val[b].cpu().numpy()) == _bits(mh[b].reshape(-1)[want])).all()


def test_the_table_is_cached_per_radius():
    a, b = acq.region_table(3, DEV), acq.region_table(3, torch.device(DEV))
    assert a is b and a.dtype == torch.uint32 and a.is_cuda and a.cpu().numpy().tolist() == ro.table(3).tolist()
    assert acq.region_table(4, DEV) is not a


def test_wrapper_errors():
    pred = torch.zeros(2, 8, 9, dtype=torch.uint8, device=DEV)
    unc = torch.zeros(2, 8, 9, device=DEV)
    with pytest.raises(_lib.PixelPickHipError, match="no CPU fallback"):
        acq.region_score_map(pred.cpu(), unc, 1, 3)
    with pytest.raises(_lib.PixelPickHipError, match="no CPU fallback"):
        acq.region_score_map(pred, unc.cpu(), 1, 3)
    with pytest.raises(ValueError, match="uint8"):
        acq.region_score_map(pred.to(torch.int32), unc, 1, 3)
    with pytest.raises(ValueError, match="float32"):
        acq.region_score_map(pred, unc.double(), 1, 3)
    with pytest.raises(ValueError, match="3-d"):
        acq.region_score_map(pred[0], unc, 1, 3)
    with pytest.raises(ValueError, match="agree"):
        acq.region_score_map(pred, unc[:, :, :8].contiguous(), 1, 3)
    with pytest.raises(ValueError, match="contiguous"):
        acq.region_score_map(pred, unc.transpose(1, 2), 1, 3)
    for r in (0, 17):
        with pytest.raises(ValueError, match="radius"):
            acq.region_score_map(pred, unc, r, 3)
    with pytest.raises(ValueError, match="mode"):
        acq.region_score_map(pred, unc, 1, 3, mode="max")
    out = acq.region_score_map(pred, unc, 1, 3)                   # and the well-formed call goes through
    assert out.shape == (2, 8, 9) and float(out.abs().max()) == 0.0
