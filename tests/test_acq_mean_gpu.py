"""GPU tests of the MC-dropout mean-probability scores and BALD (pp_acq_lowres_mc_mean_topk / pp_acq_mean_prob_score_map,
acquisition.mc_mean_topk_lowres / mean_prob_score_map):
  1. the low-resolution entry bit for bit against the composition it stands for: pp_bilinear_fwd of the [B*T,h,w,C] tensor ->
     pp_acq_softmax_sum per image (prob_out, uc_out with the entropy strategy, accumulate = 0) -> pp_acq_mean_prob_score_map ->
     pp_topk_select,
  2. the map against torch float64 on the host (softmax per pass -> mean -> formulas).  Bars: the consensus scores rtol 2e-5 / atol 2e-6
     (test_score_at_is_the_score_of_the_mean_probability's); BALD is the difference of a consensus entropy and a mean score (bar rtol
     1e-5 / atol 1e-6), so its bar is the sum of the two, elementwise: 2e-5 |H(pm)| + 1e-5 |mean H| + 3e-6,
  3. the selection against a stable sort of the device's own map (ties -> lower flat index, NaN first for `largest`),
  4. fewer free pixels than k: the excluded pixels follow, lowest index first, with the fills -1.0 / 2.0,
  5. NaN (0 * log 0 in a pass, or in the mean) at the composition's positions, picked first,
  6. pp_acq_mean_prob_score_map on a 150-class head against float64, and on a 19-class input - NCHW and channels-last - bit for bit
     against pp_uncertainty_from_prob (the register path of the class counts up to 64)."""
import functools

import numpy as np
import pytest
import torch

from pixelpick_amd import acquisition as acq
from pixelpick_amd import engine as E

pytestmark = pytest.mark.gpu
STRATS = ["entropy", "least_confidence", "margin_sampling", "bald"]
DEV = "cuda:0"

# C, (h, w), (H, W), crop, align_corners, T, B, channel pad (ldx = C + pad): the shapes of tests/test_acq_mc_lowres_gpu.py
CASES = {
    "cs_1.5tiles": (19, (16, 24), (64, 96), None, True, 4, 2, 0),        # 1 1/2 tiles across, several down
    "voc_crop": (21, (20, 23), (80, 92), (77, 90), True, 3, 1, 0),       # the VOC branch: padded size, cropped back
    "fpn_x2": (19, (24, 40), (48, 80), None, False, 2, 3, 0),            # x2, align_corners = False: FPNSeg's geometry
    "camvid_T1": (11, (9, 13), (36, 52), None, True, 1, 1, 0),           # one pass: the mean is the pass, BALD is 0
    "c7_slice": (7, (16, 24), (64, 96), None, True, 3, 1, 5),            # generic <= 32 instantiation, a channel slice (ldx = C + 5)
    "c40": (40, (16, 24), (64, 96), None, True, 3, 1, 0),                # the <= 64 instantiation: rows outer, taps from memory
    "cs_8row_tiles": (19, (32, 64), (128, 256), None, True, 2, 32, 0),   # 512 tiles of 32 rows: where the mean-score kernel runs 8 rows per wave
    "c21_many_tiles": (21, (8, 16), (32, 64), None, True, 2, 512, 0),    # C = 21, 512 32-row tiles: the 8-row plan has to step down to 4 rows
    "down_8x_memory": (19, (200, 300), (25, 40), None, True, 2, 1, 0),   # 8x down-sampling: the patch exceeds LDS -> the form that reads memory
    "down_c21_memory": (21, (120, 150), (30, 50), (27, 45), True, 3, 2, 0),    # the same form, cropped, another class count
    "down_c7_memory": (7, (200, 300), (25, 40), None, False, 2, 1, 0),   # the generic instantiation of that form, align_corners = False
}
SMALL = [n for n in CASES if CASES[n][6] <= 3]      # the float64 reference runs on the host


def _ks(hc, wc):
    return [9, 48, 49, int(0.05 * hc * wc)]      # both sides of the fused-extraction limit (48) and the top-5 % mode


def _low(rng, B, T, C, h, w, pad):
    t = torch.from_numpy((rng.randn(B * T, h, w, C) * 3).astype(np.float32)).to(DEV)
    if pad:
        wide = torch.full((B * T, h, w, C + pad), 7.0, device=DEV)
        wide[..., :C] = t
        return wide[..., :C]
    return t


def _exclude(rng, B, hc, wc):
    """2 % random pixels plus one fully excluded 64-column x 32-row block (a whole tile of the scorer, clipped to the image)."""
    ex = rng.rand(B, hc, wc) < 0.02
    if hc <= 32 and wc <= 64:       # the whole image is one block: exclude a quarter of it instead
        ex[:, :hc // 2, :wc // 2] = True
    else:
        ex[:, :32, :64] = True
    return ex


def _pred(low, size, crop, align):
    """pp_bilinear_fwd of every pass, NCHW, cropped view: what model(x)["pred"][:, :, :h, :w] holds on the full-size route."""
    pred = E.bilinear(E.Tape(False), E.Var(low), size, align, 0.0, out_nchw=True).t
    return pred if crop is None else pred[:, :, :crop[0], :crop[1]]


def _accumulated(pred, B, T):
    """pp_acq_softmax_sum per image, accumulate = 0: the mean probability [B,C,hc,wc] and the mean per-pass entropy [B,hc,wc]."""
    C, hc, wc = pred.shape[1:]
    prob = torch.empty((B, C, hc, wc), dtype=torch.float32, device=DEV)
    ment = torch.empty((B, hc, wc), dtype=torch.float32, device=DEV)
    for b in range(B):
        acq.mc_accumulate_(pred[b * T:(b + 1) * T], prob[b], ment[b], "entropy", 1.0 / T, accumulate=False)
    return prob, ment


def _composition(prob, ment, excl, st):
    return acq.mean_prob_score_map(prob, ment if st == "bald" else None, excl, st)


def _stable_order(m: np.ndarray, largest: bool) -> np.ndarray:
    """Flat indices in the ABI's order: value descending (ascending), ties -> lower index, NaN first for largest (last otherwise)."""
    v = m.reshape(-1).astype(np.float64)
    key = np.where(np.isnan(v), -np.inf, -v) if largest else np.where(np.isnan(v), np.inf, v)
    return np.lexsort((np.arange(v.size), key))


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """One case: the classifier outputs, the exclusion mask and what the full-size route accumulates from them (shared by the strategies)."""
    C, (h, w), size, crop, align, T, B, pad = CASES[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    low = _low(rng, B, T, C, h, w, pad)
    hc, wc = size if crop is None else crop
    excl = _exclude(rng, B, hc, wc)
    prob, ment = _accumulated(_pred(low, size, crop, align), B, T)
    return low, excl, prob, ment


@functools.lru_cache(maxsize=None)
def _run(name, st):
    """One case, one strategy: the new call at every k and the composition, computed once for tests 1 and 3."""
    C, (h, w), size, crop, align, T, B, pad = CASES[name]
    low, excl, prob, ment = _inputs(name)
    hc, wc = size if crop is None else crop
    ref_map = _composition(prob, ment, excl, st)
    out = {"ref_map": ref_map.cpu().numpy(), "ks": _ks(hc, wc), "largest": acq.MEAN_LARGEST[st]}
    _, _, m0 = acq.mc_mean_topk_lowres(low, T, size, excl, st, 0, crop=crop, align_corners=align)
    out["map0"] = m0.cpu().numpy()
    for k in out["ks"]:
        ri, rv = acq.topk_select(ref_map.reshape(B, hc * wc), k, acq.MEAN_LARGEST[st])
        i1, v1, m1 = acq.mc_mean_topk_lowres(low, T, size, excl, st, k, crop=crop, align_corners=align, return_map=True)
        i2, v2, none = acq.mc_mean_topk_lowres(low, T, size, excl, st, k, crop=crop, align_corners=align)      # the production call: no map
        assert none is None
        out[k] = tuple(t.cpu().numpy() for t in (ri, rv, i1, v1, m1, i2, v2))
    return out


@pytest.mark.parametrize("st", STRATS)
@pytest.mark.parametrize("name", list(CASES))
def test_equals_the_composition_bit_for_bit(name, st):
    r = _run(name, st)
    assert np.array_equal(r["map0"], r["ref_map"], equal_nan=True)                  # k == 0: the map only
    excl = _inputs(name)[1]
    assert (r["map0"][excl] == acq.MEAN_FILL[st]).all()
    for k in r["ks"]:
        ri, rv, i1, v1, m1, i2, v2 = r[k]
        assert np.array_equal(m1, r["ref_map"], equal_nan=True), k
        assert np.array_equal(i1, ri) and np.array_equal(v1, rv, equal_nan=True), k
        assert np.array_equal(i2, ri) and np.array_equal(v2, rv, equal_nan=True), k


@pytest.mark.parametrize("st", STRATS)
@pytest.mark.parametrize("name", list(CASES))
def test_selection_is_the_stable_sort_of_the_returned_map(name, st):
    r = _run(name, st)
    for k in r["ks"]:
        _, _, i1, v1, m1, _, _ = r[k]
        for b in range(m1.shape[0]):
            want = _stable_order(m1[b], r["largest"])[:k]
            assert i1[b].tolist() == want.tolist(), (k, b)
            assert np.array_equal(v1[b], m1[b].reshape(-1)[want], equal_nan=True)


def _host_f64(pred: torch.Tensor, B, T):
    """softmax of every pass in float64 on the host: [B,T,C,hc,wc]."""
    p = torch.softmax(pred.double().cpu(), dim=1)
    return p.reshape(B, T, *p.shape[1:])


def _entropy_f64(p: torch.Tensor) -> torch.Tensor:
    return (-p * p.log()).sum(dim=-3)


def _assert_within_bars(got: np.ndarray, p: torch.Tensor, ment: torch.Tensor, st: str):
    """got against float64 from the mean probability p [..,C,h,w] and the mean per-pass entropy ment [..,h,w] (bald only)."""
    got = got.astype(np.float64)
    if st == "bald":
        hbar = _entropy_f64(p)
        err = np.abs(got - (hbar - ment).numpy())
        bar = 2e-5 * hbar.abs().numpy() + 1e-5 * ment.abs().numpy() + 3e-6
        print(f"bald: max error {err.max():.3e}, smallest slack {(bar - err).min():.3e}")
        assert (err <= bar).all(), float((err - bar).max())
        return
    if st == "entropy":
        want = _entropy_f64(p)
    else:
        top = p.topk(2, dim=-3).values
        want = 1.0 - top.select(-3, 0) if st == "least_confidence" else (top.select(-3, 0) - top.select(-3, 1)).abs()
    print(f"{st}: max error {np.abs(got - want.numpy()).max():.3e}")
    np.testing.assert_allclose(got, want.numpy(), rtol=2e-5, atol=2e-6)


@pytest.mark.parametrize("st", STRATS)
@pytest.mark.parametrize("name", SMALL)
def test_map_matches_float64(name, st):
    C, (h, w), size, crop, align, T, B, pad = CASES[name]
    rng = np.random.RandomState(17 + C)
    low = _low(rng, B, T, C, h, w, pad)
    _, _, m = acq.mc_mean_topk_lowres(low, T, size, None, st, 0, crop=crop, align_corners=align)
    p = _host_f64(_pred(low, size, crop, align), B, T)
    _assert_within_bars(m.cpu().numpy(), p.mean(dim=1), _entropy_f64(p).mean(dim=1), st)
    if st == "bald" and T == 1:       # one pass: no mutual information, within the same bar of 0
        h1 = _entropy_f64(p[:, 0]).numpy()
        assert (np.abs(m.cpu().numpy().astype(np.float64)) <= 3e-5 * h1 + 3e-6).all()


@pytest.mark.parametrize("st", STRATS)
@pytest.mark.parametrize("k", [9, 49])
def test_fewer_free_pixels_than_k(st, k):
    """Excluded pixels are then returned, lowest index first, with the fills -1.0 / 2.0 - strictly behind every free pixel."""
    C, (h, w), size, T, B = 19, (16, 24), (64, 96), 3, 2
    rng = np.random.RandomState(21)
    low = _low(rng, B, T, C, h, w, 0)
    excl = np.ones((B,) + size, dtype=bool)
    excl.reshape(B, -1)[:, rng.choice(size[0] * size[1], 5, replace=False)] = False
    prob, ment = _accumulated(_pred(low, size, None, True), B, T)
    ref_map = _composition(prob, ment, excl, st)
    ri, rv = acq.topk_select(ref_map.reshape(B, -1), k, acq.MEAN_LARGEST[st])
    i1, v1, m1 = acq.mc_mean_topk_lowres(low, T, size, excl, st, k, return_map=True)
    assert torch.equal(m1, ref_map) and torch.equal(i1, ri) and torch.equal(v1, rv)
    for b in range(B):
        free = np.flatnonzero(~excl[b].reshape(-1))
        assert set(i1[b, :5].tolist()) == set(free.tolist())
        assert i1[b, 5:].tolist() == [int(p) for p in np.flatnonzero(excl[b].reshape(-1))[:k - 5]]
        assert (v1[b, 5:].cpu().numpy() == acq.MEAN_FILL[st]).all() and (v1[b, :5].cpu().numpy() != acq.MEAN_FILL[st]).all()


@pytest.mark.parametrize("st", ["entropy", "bald"])
@pytest.mark.parametrize("k", [9, 49])
def test_nan_positions_and_order(st, k):
    """A low-resolution 2x2 region with a logit of +120 in one class.  In ONE pass (region a): that pass's other probabilities underflow
    to 0, its entropy - so the mean entropy and BALD - is NaN, while the mean probability stays positive.  In EVERY pass (region b): the
    mean probability holds zeros as well and the consensus entropy is NaN too.  Same positions as the composition, picked first."""
    C, (h, w), size, T, B = 19, (16, 24), (64, 96), 3, 1
    rng = np.random.RandomState(8)
    low = _low(rng, B, T, C, h, w, 0)
    low[1, 5:7, 9:11, 4] = 120.0
    low[:, 11:13, 17:19, 6] = 120.0
    prob, ment = _accumulated(_pred(low, size, None, True), B, T)
    ref = _composition(prob, ment, None, st).cpu().numpy()
    i1, v1, m1 = acq.mc_mean_topk_lowres(low, T, size, None, st, k, return_map=True)
    m1 = m1.cpu().numpy()
    nan = np.flatnonzero(np.isnan(m1[0]).reshape(-1))
    assert nan.size >= 1 and np.array_equal(np.isnan(m1), np.isnan(ref)) and np.array_equal(m1, ref, equal_nan=True)
    ys, xs = nan // size[1], nan % size[1]
    in_a = (ys >= 16) & (ys <= 28) & (xs >= 32) & (xs <= 44)
    in_b = (ys >= 42) & (ys <= 54) & (xs >= 66) & (xs <= 78)
    assert (in_a | in_b).all() and in_b.any()                                          # around the regions' footprints, nowhere else
    assert in_a.any() == (st == "bald")                                                # one NaN pass: BALD only
    n = min(k, nan.size)
    assert i1[0, :n].tolist() == nan[:n].tolist()                                       # NaN first, lower index first
    assert i1[0].tolist() == _stable_order(m1[0], True)[:k].tolist()
    assert np.isnan(v1[0, :n].cpu().numpy()).all()


# ---------------------------------------------------------------- pp_acq_mean_prob_score_map on its own
@pytest.mark.parametrize("st", STRATS)
def test_score_map_of_a_wide_head_matches_float64(st):
    B, C, H, W = 2, 150, 37, 53                                                        # odd sizes, more than one block, C > 64
    g = torch.Generator().manual_seed(150)
    prob = torch.softmax(torch.randn(B, C, H, W, generator=g) * 3, dim=1).to(DEV)
    ment = (torch.rand(B, H, W, generator=g) * 2).to(DEV)
    excl = torch.rand(B, H, W, generator=g) < 0.05
    got = acq.mean_prob_score_map(prob, ment if st == "bald" else None, excl, st).cpu().numpy()
    assert (got[excl.numpy()] == acq.MEAN_FILL[st]).all()
    free = ~excl.numpy()
    got_free = np.where(free, acq.mean_prob_score_map(prob, ment if st == "bald" else None, None, st).cpu().numpy(), 0.0)
    assert np.array_equal(np.where(free, got, 0.0), got_free)
    _assert_within_bars(acq.mean_prob_score_map(prob, ment if st == "bald" else None, None, st).cpu().numpy(), prob.double().cpu(),
                        ment.double().cpu(), st)


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
@pytest.mark.parametrize("st", STRATS)
def test_score_map_equals_the_register_path_bit_for_bit(st, layout):
    B, C, H, W = 2, 19, 37, 53
    g = torch.Generator().manual_seed(19)
    prob = torch.softmax(torch.randn(B, C, H, W, generator=g) * 3, dim=1).to(DEV)
    ment = (torch.rand(B, H, W, generator=g) * 2).to(DEV)
    if layout == "channels_last":
        prob = prob.contiguous(memory_format=torch.channels_last)
        assert prob.stride(1) == 1
    got = acq.mean_prob_score_map(prob, ment if st == "bald" else None, None, st)
    want = acq.uncertainty_from_prob(prob, "entropy" if st == "bald" else st)
    if st == "bald":
        want = want - ment                                                             # one IEEE subtraction
    assert torch.equal(got, want)


def test_wrapper_errors():
    low = torch.randn(6, 8, 8, 19, device=DEV)
    with pytest.raises(ValueError):                      # crop larger than the interpolated size
        acq.mc_mean_topk_lowres(low, 3, (32, 32), None, "bald", 5, crop=(33, 32))
    with pytest.raises(ValueError):                      # k > crop_h * crop_w
        acq.mc_mean_topk_lowres(low, 3, (4, 4), None, "entropy", 17)
    with pytest.raises(Exception, match="64"):           # heads wider than 64 classes: PP_ERR_UNSUPPORTED, the full-size route serves them
        acq.mc_mean_topk_lowres(torch.randn(2, 4, 4, 65, device=DEV), 2, (16, 16), None, "bald", 5)
    prob = torch.rand(1, 19, 4, 4, device=DEV)
    with pytest.raises(ValueError, match="mean_ent"):
        acq.mean_prob_score_map(prob, None, None, "bald")
    with pytest.raises(ValueError, match="mean_ent"):
        acq.mean_prob_score_map(prob, torch.zeros(1, 4, 4, device=DEV), None, "entropy")
