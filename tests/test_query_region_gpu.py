"""Selector-level GPU tests of `region_radius`: a QuerySelector round on the pipelined and on the fused non-pipelined route gives the
picks of the composition called by hand through the wrappers (predict_lowres -> score_topk_lowres k = 0 -> region_score_map ->
topk_select -> spread_select), the region map behind those picks holds to the numpy oracle (tests/region_oracle.py) on the device's own
label and score maps, and the option switched off changes nothing.

Stub models hand the selector PREPARED classifier outputs (tests/test_query_spread_gpu.py's arrangement) at the 64 x 96 golden size."""
import tempfile
from argparse import Namespace

import numpy as np
import pytest
import torch

import region_oracle as ro
from pixelpick_amd import acquisition as acq
from pixelpick_amd import engine as E
from pixelpick_amd import query as ppq
from pixelpick_amd.predict import predict_lowres

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_IMG, C, LOWSIZE, SIZE = 2, 19, (16, 24), (64, 96)
K, D = 6, 5
STRATEGIES = ["entropy", "least_confidence", "margin_sampling"]
EPS = 2.0 ** -23


def _pred(low, size, align=True):
    return E.bilinear(E.Tape(False), E.Var(low), size, align, 0.0, out_nchw=True).t


class _Stub(torch.nn.Module):
    """The prepared classifier outputs lows[i] [1,h,w,C] of the images whose indices sit in x[:,0,0,0]."""
    LOWRES_ALIGN_CORNERS = True

    def __init__(self, lows, size, with_lowres=True):
        super().__init__()
        self.lows, self.size, self.n_classes = lows, size, lows[0].shape[-1]
        self.calls = {"forward_lowres": 0, "forward": 0}
        if with_lowres:
            self.forward_lowres = self._forward_lowres

    def turn_on_dropout(self):
        pass

    def _low(self, x):
        return torch.cat([self.lows[int(round(float(v)))][:1] for v in x[:, 0, 0, 0].cpu()], dim=0)

    def _forward_lowres(self, x):
        self.calls["forward_lowres"] += 1
        return self._low(x), self.size

    def forward(self, x):
        self.calls["forward"] += 1
        return {"pred": _pred(self._low(x), self.size, self.LOWRES_ALIGN_CORNERS)}


class _StubFPN(_Stub):
    """FPNSeg's geometry: the classifier output at half resolution, interpolated x2 with align_corners=False."""
    LOWRES_ALIGN_CORNERS = False


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
    base = dict(dataset_name="cs", debug=False, dir_root="/tmp", experim_name="region", ignore_index=C, mc_n_steps=4, n_classes=C,
                n_pixels_by_us=K, network_name="deeplab", query_strategy="entropy", reverse_order=False, stride_total=8,
                top_n_percent=0.0, use_mc_dropout=False, vote_type="soft")
    base.update(kw)
    return Namespace(**base)


def _make(lowsize, seed):
    """Smooth classifier outputs (a coarse random field, upsampled, plus a little noise): label blobs with real edges."""
    rng = np.random.RandomState(seed)
    h, w = lowsize
    lows = []
    for _ in range(N_IMG):
        coarse = torch.from_numpy(rng.randn(1, C, 4, 6).astype(np.float32) * 3)
        base = torch.nn.functional.interpolate(coarse, size=(h, w), mode="bilinear", align_corners=True)[0].permute(1, 2, 0).numpy()
        lows.append(torch.from_numpy((base[None] + 0.5 * rng.randn(1, h, w, C)).astype(np.float32)).to(DEV))
    H, W = SIZE
    xs = torch.zeros(N_IMG, 3, H, W)
    xs[:, 0, 0, 0] = torch.arange(N_IMG, dtype=torch.float32)
    ys = torch.from_numpy(rng.randint(0, C + 1, (N_IMG, H, W)))           # label C = ignore_index
    prev = [rng.rand(H, W) < 0.01 for _ in range(N_IMG)]
    return lows, xs, ys, prev, [f"/img{i}.png" for i in range(N_IMG)]


@pytest.fixture(scope="module")
def data():
    return _make(LOWSIZE, 31)


@pytest.fixture(scope="module")
def data_fpn():
    return _make((32, 48), 32)


def _round(model, data, pipeline=True, **kw):
    _, xs, ys, prev, names = data
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ppq, "QUERY_PIPELINE", pipeline)
        with tempfile.TemporaryDirectory() as td:
            np.random.seed(4)
            E.set_dropout_seed(7)
            qs = ppq.QuerySelector(_args(dir_root=td, **kw), _DL(_DS(xs, ys, prev, names)), device=torch.device(DEV))
            dq = qs(nth_query=1, model=model)
    return dq, qs.query_stats


def _picks(dq, name):
    W = SIZE[1]
    return (dq[name]["y_coords"].astype(np.int64) * W + dq[name]["x_coords"]).tolist()


def _excl(data):
    _, _, ys, prev, _ = data
    return np.stack([prev[i] | (ys[i].numpy() == C) for i in range(N_IMG)])


def _maps(data, st, align=True):
    """The producers' outputs for the whole batch, as the selector launches them: (pred u8, unc f32) on the device."""
    low = torch.cat([l[:1] for l in data[0]], dim=0)
    pred, _ = predict_lowres(low, SIZE, crop=SIZE, align_corners=align, want_pred=True)
    unc = acq.score_topk_lowres(low, SIZE, None, st, 0, crop=SIZE, align_corners=align)[2]
    return pred, unc


def _by_hand(data, st, r, mode="product", d=0, top=0.0, align=True):
    """The composition through the wrappers -> the sorted picks per image."""
    H, W = SIZE
    excl = torch.from_numpy(_excl(data)).to(DEV)
    pred, unc = _maps(data, st, align)
    rmap = acq.region_score_map(pred, unc, r, C, exclude=excl, mode=mode, flip=st == "margin_sampling")
    k = int(H * W * top) if top > 0 else (acq.spread_candidates(K, d, H * W) if d >= 2 else K)
    idx, _ = acq.topk_select(rmap.reshape(N_IMG, H * W), k, True)
    if d >= 2:
        idx = acq.spread_select(idx, W, K, d, exclude=excl, n_pixels=H * W)[0]
    idx = idx.cpu().numpy().astype(np.int64)
    if top > 0:                                                   # query.py:63-64 with the seed _round fixes, image by image
        np.random.seed(4)
        return [sorted(idx[i][np.random.choice(k, K, False)].tolist()) for i in range(N_IMG)]
    return [sorted(idx[i].tolist()) for i in range(N_IMG)]


@pytest.mark.parametrize("r", [1, 4])
@pytest.mark.parametrize("st", STRATEGIES)
def test_round_gives_the_composition_called_by_hand(data, st, r):
    lows, _, _, _, names = data
    for d in (0, D):
        want = _by_hand(data, st, r, d=d)
        model = _Stub(lows, SIZE)
        piped = _round(model, data, True, region_radius=r, query_strategy=st, min_pixel_distance=d)
        fused = _round(model, data, False, region_radius=r, query_strategy=st, min_pixel_distance=d)
        assert model.calls == {"forward_lowres": 2, "forward": 0}
        for i, nme in enumerate(names):
            assert _picks(piped[0], nme) == want[i] and _picks(fused[0], nme) == want[i], (st, r, d, i)
            assert len(want[i]) == K and not _excl(data)[i].reshape(-1)[want[i]].any()
        assert len(piped[1].list_entropy) == len(fused[1].list_entropy) == N_IMG * K
        np.testing.assert_allclose(np.asarray(piped[1].list_entropy, dtype=np.float64), np.asarray(fused[1].list_entropy, dtype=np.float64),
                                   rtol=2e-5, atol=2e-6)
        assert piped[1].dict_label_cnt == fused[1].dict_label_cnt
    # the region score is not the per-pixel score: the picks move
    plain = _round(_Stub(lows, SIZE), data, True, query_strategy=st)
    assert any(_picks(plain[0], nme) != want_i for nme, want_i in zip(names, _by_hand(data, st, r)))


@pytest.mark.parametrize("mode", ["impurity", "uncertainty"])
def test_round_with_another_region_mode(data, mode):
    lows, _, _, _, names = data
    want = _by_hand(data, "entropy", 4, mode=mode)
    got = _round(_Stub(lows, SIZE), data, True, region_radius=4, region_mode=mode)
    for i, nme in enumerate(names):
        assert _picks(got[0], nme) == want[i]


@pytest.mark.parametrize("pipeline", [True, False], ids=["pipelined", "fused"])
def test_round_with_the_random_sub_sample_of_the_best_five_percent(data, pipeline):
    lows, _, _, _, names = data
    want = _by_hand(data, "entropy", 4, top=0.05)
    got = _round(_Stub(lows, SIZE), data, pipeline, region_radius=4, top_n_percent=0.05)
    for i, nme in enumerate(names):
        assert _picks(got[0], nme) == want[i]
    assert len(got[1].list_entropy) == N_IMG * K


def test_round_with_reverse_order(data):
    """reverse_order is only a wider exclusion mask: the picks come from the drawn 5 % candidate set, never from the excluded pixels."""
    lows, _, _, _, names = data
    H, W = SIZE
    got = _round(_Stub(lows, SIZE), data, True, region_radius=2, reverse_order=True, top_n_percent=0.05)
    np.random.seed(4)
    excl = _excl(data)
    pred, unc = _maps(data, "entropy")
    for i, nme in enumerate(names):
        cand = np.zeros(H * W, dtype=bool)
        cand[np.random.choice(range(H * W), int(H * W * 0.05), False)] = True
        ex = excl[i] | ~cand.reshape(H, W)
        rmap = acq.region_score_map(pred[i:i + 1].contiguous(), unc[i:i + 1].contiguous(), 2, C, exclude=ex[None])
        want = ro.ranking(rmap[0].cpu().numpy(), K)
        assert _picks(got[0], nme) == sorted(want.tolist()) and not ex.reshape(-1)[want].any()


@pytest.mark.parametrize("r", [1, 4])
@pytest.mark.parametrize("st", STRATEGIES)
def test_the_map_behind_the_picks_holds_to_the_oracle(data, st, r):
    """On the device's own label and score maps: P bit-equal, U and P * U within the bounds of tests/test_region_gpu.py."""
    flip = st == "margin_sampling"
    pred, unc = _maps(data, st)
    ph, uh = pred.cpu().numpy(), unc.cpu().numpy()
    excl = _excl(data)
    Kw = (2 * r + 1) ** 2
    P = acq.region_score_map(pred, None, r, C, mode="impurity").cpu().numpy()
    U = acq.region_score_map(None, unc, r, C, mode="uncertainty", flip=flip).cpu().numpy()
    S = acq.region_score_map(pred, unc, r, C, exclude=excl, flip=flip).cpu().numpy()
    for i in range(N_IMG):
        Pw, Uw = ro.impurity(ph[i], C, r), ro.uncertainty64(uh[i], r, flip)
        # the scale of the bound: the window mean of |u| - U itself wherever the device's scores are non-negative (a score map may
        # hold a rounding-sized negative value at a confident pixel; the sum's error is bounded by the terms' magnitudes)
        Ua = ro.uncertainty64(uh[i], r, flip, absolute=True)
        assert (P[i].view(np.uint32) == Pw.view(np.uint32)).all() and Pw.max() > 0
        assert (np.abs(U[i] - Uw) <= (Kw + 2) * EPS * Ua).all()
        want = Pw.astype(np.float64) * Uw
        keep = ~excl[i]
        assert (np.abs(S[i] - want)[keep] <= ((Kw + 4) * EPS * Pw * Ua)[keep]).all()
        assert (S[i][excl[i]] == ro.FILL).all() and (S[i][keep & (Pw == 0)] == 0.0).all()


@pytest.mark.parametrize("pipeline", [True, False], ids=["pipelined", "fused"])
def test_the_option_is_inert_when_off(data, pipeline):
    lows, _, _, _, names = data
    for kw in (dict(), dict(top_n_percent=0.05), dict(min_pixel_distance=D)):
        ref = _round(_Stub(lows, SIZE), data, pipeline, **kw)
        for off in (dict(region_radius=0), dict(region_radius=None), dict(region_radius=0, region_mode="impurity")):
            got = _round(_Stub(lows, SIZE), data, pipeline, **kw, **off)
            for nme in names:
                assert _picks(got[0], nme) == _picks(ref[0], nme) and len(_picks(ref[0], nme)) == K
            assert got[1].list_entropy == ref[1].list_entropy and got[1].list_spatial_coverage == ref[1].list_spatial_coverage
            assert got[1].dict_label_cnt == ref[1].dict_label_cnt and got[1].list_n_unique_labels == ref[1].list_n_unique_labels


def test_fpn_geometry(data_fpn):
    """x2, align_corners=False: the selector hands the model's own geometry to all three producers."""
    lows, _, _, _, names = data_fpn
    want = _by_hand(data_fpn, "entropy", 4, align=False)
    model = _StubFPN(lows, SIZE)
    piped = _round(model, data_fpn, True, region_radius=4)
    fused = _round(model, data_fpn, False, region_radius=4)
    assert model.calls == {"forward_lowres": 2, "forward": 0}
    for i, nme in enumerate(names):
        assert _picks(piped[0], nme) == want[i] and _picks(fused[0], nme) == want[i]
    assert want != _by_hand(data_fpn, "entropy", 4, align=True)


@pytest.mark.parametrize("kw,with_lowres,fused_on", [(dict(use_mc_dropout=True), True, True), (dict(query_strategy="random"), True, True),
                                                     (dict(region_radius=17), True, True), (dict(region_mode="sum"), True, True),
                                                     (dict(), False, True), (dict(), True, False)])
def test_refused_combinations_raise(data, kw, with_lowres, fused_on):
    lows = data[0]
    model = _Stub(lows, SIZE, with_lowres=with_lowres)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ppq, "FUSED_LOWRES", fused_on)
        with pytest.raises(ValueError, match="region_radius"):
            _round(model, data, True, **dict(dict(region_radius=3), **kw))
    assert model.calls == {"forward_lowres": 0, "forward": 0}
