"""GPU tests of the MC-dropout acquisition from the classifier-resolution logits (pp_acq_lowres_mc_score_topk /
pp_acq_lowres_mc_score_at, acquisition.mc_score_topk_lowres / mc_score_at_lowres, the selector's route for models with forward_lowres):
  1. bit for bit against the launches it replaces: pp_bilinear_fwd of the [B*T,h,w,C] tensor -> pp_acq_softmax_sum per image -> fill at
     excluded pixels -> pp_topk_select,
  2. the arithmetic against torch float64 on the host (rtol 1e-5 / atol 1e-6, the bar of test_mc_accumulate_matches_torch_softmax_and_scores),
  3. the selection against a stable sort of the device's own map (ties -> lower flat index, NaN first for `largest`),
  4. the score of the mean probability at listed pixels against float64 (2e-5 relative / 2e-6 absolute, DESIGN.md §3's score bar),
  5. the selector through the real DeepLab: same coordinates and statistics as the full-size route."""
import functools
import tempfile
from argparse import Namespace

import numpy as np
import pytest
import torch

from pixelpick_amd import _lib
from pixelpick_amd import acquisition as acq
from pixelpick_amd import engine as E
from pixelpick_amd import query as ppq

pytestmark = pytest.mark.gpu
STRATS = ["entropy", "least_confidence", "margin_sampling"]
DEV = "cuda:0"

# C, (h, w), (H, W), crop, align_corners, T, B, channel pad (ldx = C + pad)
CASES = {
    "cs_1.5tiles": (19, (16, 24), (64, 96), None, True, 4, 2, 0),        # 1 1/2 tiles across, several down
    "voc_crop": (21, (20, 23), (80, 92), (77, 90), True, 3, 1, 0),       # the VOC branch: padded size, cropped back
    "fpn_x2": (19, (24, 40), (48, 80), None, False, 2, 3, 0),            # x2, align_corners = False: FPNSeg's geometry
    "camvid_T5": (11, (9, 13), (36, 52), None, True, 5, 1, 0),
    "camvid_T1": (11, (9, 13), (36, 52), None, True, 1, 1, 0),           # one pass: the mean is the pass
    "c7_slice": (7, (16, 24), (64, 96), None, True, 3, 1, 5),            # generic <= 32 instantiation, a channel slice (ldx = C + 5)
    "c40": (40, (16, 24), (64, 96), None, True, 3, 1, 0),                # generic <= 64 instantiation
    "cs_8row_tiles": (19, (32, 64), (128, 256), None, True, 2, 32, 0),   # 512 tiles of 32 rows: the planner's 8-rows-per-wave form
    "down_8x_memory": (19, (200, 300), (25, 40), None, True, 2, 1, 0),   # 8x down-sampling: the patch exceeds LDS -> the form that reads memory
    "down_c21_memory": (21, (120, 150), (30, 50), (27, 45), True, 3, 2, 0),    # the same form, cropped, another class count
    "down_c7_memory": (7, (200, 300), (25, 40), None, False, 2, 1, 0),   # the generic instantiation of that form, align_corners = False
    "replan_8row": (19, (40, 60), (20, 30), None, True, 1, 512, 0),      # 512 tiles with 8 rows per wave forced: no LDS patch -> re-planned
}
# cases run with the test build's pp_debug_set_acq_tuning(0, 8): the planner then keeps 8 rows per wave where it would step down to 4 for
# the size of the patch, so a patch beyond LDS meets an 8-row plan and make_lowres_mc_plan has to re-plan it (no 8-row memory form exists)
FORCE_8_ROWS = {"replan_8row"}


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


def _replaced_map(pred, B, T, excl_dev, st):
    """pp_acq_softmax_sum per image (accumulate = 0) and the fill at excluded pixels, as QuerySelector's full-size route does them."""
    hc, wc = pred.shape[2:]
    maps = []
    for b in range(B):
        uc = torch.empty((hc, wc), dtype=torch.float32, device=DEV)
        acq.mc_accumulate_(pred[b * T:(b + 1) * T], None, uc, st, 1.0 / T, accumulate=False)
        if excl_dev is not None:
            uc[excl_dev[b]] = acq.FILL[st]
        maps.append(uc)
    return torch.stack(maps)


def _stable_order(m: np.ndarray, largest: bool) -> np.ndarray:
    """Flat indices in the ABI's order: value descending (ascending), ties -> lower index, NaN first for largest (last otherwise)."""
    v = m.reshape(-1).astype(np.float64)
    key = np.where(np.isnan(v), -np.inf, -v) if largest else np.where(np.isnan(v), np.inf, v)
    return np.lexsort((np.arange(v.size), key))


@functools.lru_cache(maxsize=None)
def _run(name, st):
    """One case, one strategy: the new call at every k and the launches it replaces, computed once for tests 1 and 3."""
    C, (h, w), size, crop, align, T, B, pad = CASES[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    low = _low(rng, B, T, C, h, w, pad)
    hc, wc = size if crop is None else crop
    excl = _exclude(rng, B, hc, wc)
    excl_dev = torch.from_numpy(excl).to(DEV)
    ref_map = _replaced_map(_pred(low, size, crop, align), B, T, excl_dev, st)
    out = {"ref_map": ref_map.cpu().numpy(), "ks": _ks(hc, wc), "largest": acq.LARGEST[st]}
    refs = {k: acq.topk_select(ref_map.reshape(B, hc * wc), k, acq.LARGEST[st]) for k in out["ks"]}
    try:
        if name in FORCE_8_ROWS:
            _lib.lib().pp_debug_set_acq_tuning(0, 8)
        _, _, m0 = acq.mc_score_topk_lowres(low, T, size, excl, st, 0, crop=crop, align_corners=align)
        out["map0"] = m0.cpu().numpy()
        for k in out["ks"]:
            ri, rv = refs[k]
            i1, v1, m1 = acq.mc_score_topk_lowres(low, T, size, excl, st, k, crop=crop, align_corners=align, return_map=True)
            i2, v2, _ = acq.mc_score_topk_lowres(low, T, size, excl, st, k, crop=crop, align_corners=align)      # the production call: no map
            out[k] = tuple(t.cpu().numpy() for t in (ri, rv, i1, v1, m1, i2, v2))
    finally:
        if name in FORCE_8_ROWS:
            _lib.lib().pp_debug_set_acq_tuning(0, 0)
    return out


@pytest.mark.parametrize("st", STRATS)
@pytest.mark.parametrize("name", list(CASES))
def test_equals_the_launches_it_replaces_bit_for_bit(name, st):
    r = _run(name, st)
    assert np.array_equal(r["map0"], r["ref_map"], equal_nan=True)                  # k == 0: the map only
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


@pytest.mark.parametrize("st", STRATS)
@pytest.mark.parametrize("k", [9, 49])
def test_fewer_free_pixels_than_k(st, k):
    """Excluded pixels are then returned, lowest index first (as pp_acq_score_topk): same picks as the launches replaced."""
    C, (h, w), size, T, B = 19, (16, 24), (64, 96), 3, 2
    rng = np.random.RandomState(21)
    low = _low(rng, B, T, C, h, w, 0)
    excl = np.ones((B,) + size, dtype=bool)
    excl.reshape(B, -1)[:, rng.choice(size[0] * size[1], 5, replace=False)] = False
    ref_map = _replaced_map(_pred(low, size, None, True), B, T, torch.from_numpy(excl).to(DEV), st)
    ri, rv = acq.topk_select(ref_map.reshape(B, -1), k, acq.LARGEST[st])
    i1, v1, m1 = acq.mc_score_topk_lowres(low, T, size, excl, st, k, return_map=True)
    assert torch.equal(m1, ref_map) and torch.equal(i1, ri) and torch.equal(v1, rv)
    for b in range(B):
        free = np.flatnonzero(~excl[b].reshape(-1))
        assert set(i1[b, :5].tolist()) == set(free.tolist())
        assert i1[b, 5:].tolist() == [int(p) for p in np.flatnonzero(excl[b].reshape(-1))[:k - 5]]


@pytest.mark.parametrize("k", [9, 49])
def test_entropy_nan_positions_and_order(k):
    """A low-resolution 2x2 region with a logit of +120 in one class, in ONE pass: the probabilities of the other classes underflow to 0
    at the pixels interpolated inside it, the entropy of that pass and so the mean are NaN (query.py:230) - at the same positions as on
    the full-size route, and they are picked first."""
    C, (h, w), size, T, B = 19, (16, 24), (64, 96), 3, 1
    rng = np.random.RandomState(8)
    low = _low(rng, B, T, C, h, w, 0)
    low[1, 5:7, 9:11, 4] = 120.0
    ref_map = _replaced_map(_pred(low, size, None, True), B, T, None, "entropy")
    i1, v1, m1 = acq.mc_score_topk_lowres(low, T, size, None, "entropy", k, return_map=True)
    m1, ref = m1.cpu().numpy(), ref_map.cpu().numpy()
    nan = np.flatnonzero(np.isnan(m1[0]).reshape(-1))
    assert nan.size >= 1 and np.array_equal(np.isnan(m1), np.isnan(ref)) and np.array_equal(m1, ref, equal_nan=True)
    ys, xs = nan // size[1], nan % size[1]
    assert ys.min() >= 16 and ys.max() <= 28 and xs.min() >= 32 and xs.max() <= 44      # around the region's footprint, nowhere else
    n = min(k, nan.size)
    assert i1[0, :n].tolist() == nan[:n].tolist()                                       # NaN first, lower index first
    assert i1[0].tolist() == _stable_order(m1[0], True)[:k].tolist()
    assert np.isnan(v1[0, :n].cpu().numpy()).all()


def _host_f64(pred: torch.Tensor, B, T):
    """softmax of every pass in float64 on the host: [B,T,C,hc,wc]."""
    p = torch.softmax(pred.double().cpu(), dim=1)
    return p.reshape(B, T, *p.shape[1:])


def _scores_f64(p: torch.Tensor, st: str) -> torch.Tensor:
    """The strategy's score (query.py:229-239) of probabilities along dim -3."""
    if st == "entropy":
        return (-p * p.log()).sum(dim=-3)
    top = p.topk(2, dim=-3).values
    return 1.0 - top.select(-3, 0) if st == "least_confidence" else (top.select(-3, 0) - top.select(-3, 1)).abs()


@pytest.mark.parametrize("st", STRATS)
@pytest.mark.parametrize("name", ["cs_1.5tiles", "voc_crop", "fpn_x2", "c40", "down_8x_memory", "down_c21_memory", "down_c7_memory"])
def test_map_matches_float64_softmax_scores_and_mean(name, st):
    C, (h, w), size, crop, align, T, B, pad = CASES[name]
    rng = np.random.RandomState(17 + C)
    low = _low(rng, B, T, C, h, w, pad)
    _, _, m = acq.mc_score_topk_lowres(low, T, size, None, st, 0, crop=crop, align_corners=align)
    want = _scores_f64(_host_f64(_pred(low, size, crop, align), B, T), st).mean(dim=1)
    np.testing.assert_allclose(m.cpu().numpy().astype(np.float64), want.numpy(), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("st", ["entropy", "least_confidence"])
@pytest.mark.parametrize("name", ["cs_1.5tiles", "voc_crop", "fpn_x2", "c7_slice", "camvid_T5", "c40"])
def test_score_at_is_the_score_of_the_mean_probability(name, st):
    C, (h, w), size, crop, align, T, B, pad = CASES[name]
    rng = np.random.RandomState(29 + C)
    low = _low(rng, B, T, C, h, w, pad)
    hc, wc = size if crop is None else crop
    n = 200
    img = rng.randint(0, B, n)
    pix = rng.randint(0, hc * wc, n)
    pix[:6] = [0, wc - 1, (hc - 1) * wc, hc * wc - 1, (hc - 1) * wc + wc // 2, (hc // 2) * wc + wc - 1]     # corners, last row / column
    img[:6] = [0, B - 1, 0, B - 1, 0, B - 1]
    got = acq.mc_score_at_lowres(low, T, size, img, pix, st, crop=crop, align_corners=align)
    assert got.shape == (n,) and got.dtype == torch.float32
    pbar = _host_f64(_pred(low, size, crop, align), B, T).mean(dim=1)                    # [B,C,hc,wc]
    want = _scores_f64(pbar, st).reshape(B, -1)[torch.from_numpy(img), torch.from_numpy(pix)]
    np.testing.assert_allclose(got.cpu().numpy().astype(np.float64), want.numpy(), rtol=2e-5, atol=2e-6)
    empty = acq.mc_score_at_lowres(low, T, size, [], [], st, crop=crop, align_corners=align)
    assert empty.numel() == 0 and empty.dtype == torch.float32


def test_wrapper_errors():
    low = torch.randn(6, 8, 8, 19, device=DEV)
    with pytest.raises(ValueError):                      # 6 entries are not a multiple of 4 passes
        acq.mc_score_topk_lowres(low, 4, (32, 32), None, "entropy", 5)
    with pytest.raises(ValueError):
        acq.mc_score_at_lowres(low, 4, (32, 32), [0], [0])
    with pytest.raises(ValueError):                      # crop larger than the interpolated size
        acq.mc_score_topk_lowres(low, 3, (32, 32), None, "entropy", 5, crop=(33, 32))
    with pytest.raises(ValueError):                      # k > crop_h * crop_w
        acq.mc_score_topk_lowres(low, 3, (4, 4), None, "entropy", 17)
    with pytest.raises(Exception):                       # heads wider than 64 classes: PP_ERR_UNSUPPORTED
        acq.mc_score_topk_lowres(torch.randn(2, 4, 4, 65, device=DEV), 2, (16, 16), None, "entropy", 5)


# ---------------------------------------------------------------- the selector through the real network
class _DS:
    def __init__(self, xs, ys, queries, names):
        self.xs, self.ys, self.queries, self.names, self.labelled = xs, ys, queries, names, None

    def label_queries(self, d, nth):
        self.labelled = (d, nth)


class _DL:
    def __init__(self, ds):
        self.dataset = ds

    def __iter__(self):
        for i in range(len(self.dataset.xs)):
            yield {"x": self.dataset.xs[i][None], "y": self.dataset.ys[i][None], "p_img": [self.dataset.names[i]]}


def _args(**kw):
    base = dict(dataset_name="cs", debug=False, dir_root="/tmp", experim_name="mc", ignore_index=19, mc_n_steps=4, n_classes=19,
                n_pixels_by_us=20, network_name="deeplab", query_strategy="entropy", reverse_order=False, stride_total=8,
                top_n_percent=0.0, use_mc_dropout=True, vote_type="hard")
    base.update(kw)
    return Namespace(**base)


def _deeplab(C):
    from pixelpick_amd.networks.deeplab import DeepLab
    return DeepLab(Namespace(use_mc_dropout=True, mc_dropout_p=0.2, n_classes=C, use_aspp=True, use_softmax=False, use_img_inp=False)).to(DEV)


def _data(dataset, C, n, seed=3):
    h, w = (77, 90) if dataset == "voc" else (64, 96)
    torch.manual_seed(seed)
    xs, ys = torch.randn(n, 3, h, w), torch.randint(0, C + 1, (n, h, w))
    ys[ys == C] = 255 if dataset == "voc" else C
    rng = np.random.RandomState(0)
    prev = [rng.rand(h, w) < 0.01 for _ in range(n)]
    return xs, ys, prev, [f"/img{i}.png" for i in range(n)], (h, w)


def _round(monkeypatch, model, data, fused, **kw):
    """One acquisition round with spies on the three calls that tell the routes apart -> (queries, QueryStats, call counts)."""
    xs, ys, prev, names, _ = data
    calls = {"forward_lowres": 0, "forward": 0, "mc_accumulate_": 0}

    def spy(name, fn):
        def wrapped(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapped

    with monkeypatch.context() as mp:
        mp.setattr(ppq, "FUSED_LOWRES", fused)
        mp.setattr(model, "forward_lowres", spy("forward_lowres", model.forward_lowres), raising=False)
        mp.setattr(model, "forward", spy("forward", model.forward), raising=False)
        mp.setattr(acq, "mc_accumulate_", spy("mc_accumulate_", acq.mc_accumulate_))
        with tempfile.TemporaryDirectory() as td:
            np.random.seed(4)
            E.set_dropout_seed(7)
            qs = ppq.QuerySelector(_args(dir_root=td, **kw), _DL(_DS(xs, ys, prev, names)), device=torch.device(DEV))
            dq = qs(nth_query=1, model=model)
    return dq, qs.query_stats, calls


def _assert_same_round(a, b, names, size, exact_entropy):
    (dqa, sa, _), (dqb, sb, _) = a, b
    for nme in names:
        np.testing.assert_array_equal(dqa[nme]["x_coords"], dqb[nme]["x_coords"])
        np.testing.assert_array_equal(dqa[nme]["y_coords"], dqb[nme]["y_coords"])
        assert (dqa[nme]["height"], dqa[nme]["width"]) == size
    assert sa.dict_label_cnt == sb.dict_label_cnt
    assert sa.list_n_unique_labels == sb.list_n_unique_labels
    assert sa.list_spatial_coverage == sb.list_spatial_coverage
    assert len(sa.list_entropy) == len(sb.list_entropy) >= len(names)
    if exact_entropy:
        assert sa.list_entropy == sb.list_entropy
    else:
        np.testing.assert_allclose(np.asarray(sa.list_entropy, dtype=np.float64), np.asarray(sb.list_entropy, dtype=np.float64),
                                   rtol=2e-5, atol=2e-6)


@pytest.mark.parametrize("dataset,st,top_n", [("cs", "entropy", 0.0), ("voc", "margin_sampling", 0.0), ("cs", "least_confidence", 0.05)])
def test_selector_mc_lowres_route_gives_the_full_size_routes_round(monkeypatch, dataset, st, top_n):
    """The forward sees the tensor the full-size route forwards, so the dropout masks are the same, and so are the coordinates and the
    statistics - without model.forward and pp_acq_softmax_sum."""
    C = 21 if dataset == "voc" else 19
    model = _deeplab(C)
    data = _data(dataset, C, 3)
    kw = dict(query_strategy=st, dataset_name=dataset, n_classes=C, ignore_index=255 if dataset == "voc" else C, top_n_percent=top_n)
    fused = _round(monkeypatch, model, data, True, **kw)
    plain = _round(monkeypatch, model, data, False, **kw)
    assert fused[2]["forward_lowres"] == 3 and fused[2]["forward"] == 0 and fused[2]["mc_accumulate_"] == 0
    assert plain[2]["forward_lowres"] == 0 and plain[2]["forward"] == 3 and plain[2]["mc_accumulate_"] == 3
    _assert_same_round(fused, plain, data[3], data[4], exact_entropy=False)
    if top_n == 0.0:
        assert all(len(fused[0][n]["x_coords"]) == 20 for n in data[3])


def test_selector_keeps_the_chunked_route_when_the_passes_do_not_fit_one_forward(monkeypatch):
    """mc_chunk = 3 < mc_n_steps = 4: the passes run in two forwards, which the one-launch scorer does not take."""
    model = _deeplab(19)
    data = _data("cs", 19, 3)
    fused = _round(monkeypatch, model, data, True, mc_chunk=3)
    plain = _round(monkeypatch, model, data, False, mc_chunk=3)
    assert fused[2] == plain[2] == {"forward_lowres": 0, "forward": 6, "mc_accumulate_": 6}
    _assert_same_round(fused, plain, data[3], data[4], exact_entropy=True)
