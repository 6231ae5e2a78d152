"""Selector-level GPU tests of `class_balanced`: a QuerySelector round on the pipelined and on the fused non-pipelined route gives the
picks of the composition called by hand through the wrappers (score_topk_lowres at k = 307 -> predict_lowres -> class_balance_select;
with region_radius the region ranking in the scorer's place), those picks are the oracle's (tests/balance_oracle.py) on the device's own
candidate list and label map, and the option switched off changes nothing.

Stub models hand the selector PREPARED classifier outputs (tests/test_query_region_gpu.py's arrangement) at the 64 x 96 golden size."""
import tempfile
from argparse import Namespace

import numpy as np
import pytest
import torch

import balance_oracle as bo
from pixelpick_amd import acquisition as acq
from pixelpick_amd import engine as E
from pixelpick_amd import query as ppq
from pixelpick_amd.predict import predict_lowres

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_IMG, C, LOWSIZE, SIZE = 2, 19, (16, 24), (64, 96)
K, TOP = 6, 0.05
POOL = int(SIZE[0] * SIZE[1] * TOP)
STRATEGIES = ["entropy", "least_confidence", "margin_sampling"]


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
    base = dict(dataset_name="cs", debug=False, dir_root="/tmp", experim_name="balance", ignore_index=C, mc_n_steps=4, n_classes=C,
                n_pixels_by_us=K, network_name="deeplab", query_strategy="entropy", reverse_order=False, stride_total=8,
                top_n_percent=TOP, use_mc_dropout=False, vote_type="soft")
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


def _by_hand(data, st, align=True, r=0):
    """The composition through the wrappers -> (picks in selection order int64 [n,K], candidate list, label map, n), host arrays."""
    H, W = SIZE
    low = torch.cat([l[:1] for l in data[0]], dim=0)
    excl = torch.from_numpy(_excl(data)).to(DEV)
    pred, _ = predict_lowres(low, SIZE, crop=SIZE, align_corners=align, want_pred=True)
    if r:
        unc = acq.score_topk_lowres(low, SIZE, None, st, 0, crop=SIZE, align_corners=align)[2]
        rmap = acq.region_score_map(pred, unc, r, C, exclude=excl, flip=st == "margin_sampling")
        cand, _ = acq.topk_select(rmap.reshape(N_IMG, H * W), POOL, True)
    else:
        cand, _, _ = acq.score_topk_lowres(low, SIZE, excl, st, POOL, crop=SIZE, align_corners=align)
    idx, pos, n = acq.class_balance_select(cand, pred, K, exclude=excl)
    return idx.cpu().numpy().astype(np.int64), cand.cpu().numpy(), pred.cpu().numpy(), n.cpu().numpy()


def _hold(data, st, model, align=True, r=0):
    """Both routes against the composition, the composition against the oracle, and what the rule promises about the picks."""
    names = data[4]
    excl = _excl(data)
    want, cand, pred, n = _by_hand(data, st, align, r)
    assert cand.shape == (N_IMG, POOL) and POOL == 307
    o_idx, o_pos, o_n = bo.select_batch(cand, pred, K, excl)
    assert want.tolist() == o_idx.tolist() and n.tolist() == o_n.tolist() == [K] * N_IMG
    kw = dict(class_balanced=True, query_strategy=st, region_radius=r)
    piped = _round(model, data, True, **kw)
    fused = _round(model, data, False, **kw)
    assert model.calls == {"forward_lowres": 2, "forward": 0}
    low = torch.cat([l[:1] for l in data[0]], dim=0)
    for i, nme in enumerate(names):
        assert _picks(piped[0], nme) == sorted(want[i].tolist()) and _picks(fused[0], nme) == sorted(want[i].tolist()), (st, r, i)
        assert len(set(want[i].tolist())) == K and not excl[i].reshape(-1)[want[i]].any()
        # the distinct predicted classes among the picks: as many as the eligible pool offers, up to K
        pool_classes = {int(pred[i].reshape(-1)[c]) for c in cand[i] if not excl[i].reshape(-1)[c]}
        assert len({int(pred[i].reshape(-1)[c]) for c in want[i]}) == min(K, len(pool_classes))
    # QueryStats: the entropies of the picks, image by image in ascending pixel order
    flat = np.concatenate([np.sort(w_) for w_ in want])
    ent = acq.score_at_lowres(low, SIZE, np.repeat(np.arange(N_IMG), K), flat, "entropy", crop=SIZE, align_corners=align).cpu().numpy()
    for got in (piped, fused):
        assert np.asarray(got[1].list_entropy, dtype=np.float32).tolist() == ent.astype(np.float32).tolist()
    assert piped[1].dict_label_cnt == fused[1].dict_label_cnt and piped[1].list_n_unique_labels == fused[1].list_n_unique_labels
    return want


@pytest.mark.parametrize("st", STRATEGIES)
def test_round_gives_the_composition_called_by_hand(data, st):
    want = _hold(data, st, _Stub(data[0], SIZE))
    # the rule is not the random sub-sample: a plain top-5 % round under the fixed seed picks other pixels
    plain = _round(_Stub(data[0], SIZE), data, True, query_strategy=st)
    assert any(_picks(plain[0], nme) != sorted(w_.tolist()) for nme, w_ in zip(data[4], want))


@pytest.mark.parametrize("st", STRATEGIES)
def test_fpn_geometry(data_fpn, st):
    """x2, align_corners=False: the selector hands the model's own geometry to the scorer and to the label map."""
    want = _hold(data_fpn, st, _StubFPN(data_fpn[0], SIZE), align=False)
    if st == "entropy":
        assert want.tolist() != _by_hand(data_fpn, st, align=True)[0].tolist()


@pytest.mark.parametrize("st", STRATEGIES)
def test_on_the_region_ranking_the_label_map_is_made_once(data, st, monkeypatch):
    calls = []
    real = ppq.predict_lowres

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    want = _by_hand(data, st, r=2)[0]
    monkeypatch.setattr(ppq, "predict_lowres", counted)
    _hold(data, st, _Stub(data[0], SIZE), r=2)
    assert len(calls) == 2                            # two rounds of one batch each: pp_predict_lowres once per batch
    assert want.tolist() != _by_hand(data, st)[0].tolist()      # the region ranking is another pool


def test_label_map_launches_without_the_region_score(data, monkeypatch):
    calls = []
    real = ppq.predict_lowres
    monkeypatch.setattr(ppq, "predict_lowres", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    _round(_Stub(data[0], SIZE), data, True, class_balanced=True)
    _round(_Stub(data[0], SIZE), data, False, class_balanced=True)
    assert len(calls) == 2
    _round(_Stub(data[0], SIZE), data, True)
    assert len(calls) == 2                            # off: no label map at all


@pytest.mark.parametrize("pipeline", [True, False], ids=["pipelined", "fused"])
def test_the_option_is_inert_when_off(data, pipeline):
    lows, _, _, _, names = data
    for kw in (dict(), dict(top_n_percent=0.0), dict(region_radius=2)):
        ref = _round(_Stub(lows, SIZE), data, pipeline, **kw)
        for off in (dict(class_balanced=False), dict(class_balanced=None)):
            got = _round(_Stub(lows, SIZE), data, pipeline, **kw, **off)
            for nme in names:
                assert _picks(got[0], nme) == _picks(ref[0], nme) and len(_picks(ref[0], nme)) == K
            assert got[1].list_entropy == ref[1].list_entropy and got[1].list_spatial_coverage == ref[1].list_spatial_coverage
            assert got[1].dict_label_cnt == ref[1].dict_label_cnt and got[1].list_n_unique_labels == ref[1].list_n_unique_labels


def test_switched_on_numpy_stream_is_left_alone(data):
    _round(_Stub(data[0], SIZE), data, True, class_balanced=True)       # seeds numpy with 4, then runs the round
    after = np.random.rand()
    np.random.seed(4)
    assert np.random.rand() == after


@pytest.mark.parametrize("pipeline", [True, False], ids=["pipelined", "fused"])
def test_a_pool_smaller_than_the_picks_is_refused_at_the_round(data, pipeline):
    with pytest.raises(ValueError, match="class_balanced.*n_pixels_by_us = 400"):
        _round(_Stub(data[0], SIZE), data, pipeline, class_balanced=True, n_pixels_by_us=400)


@pytest.mark.parametrize("with_lowres,fused_on", [(False, True), (True, False)])
def test_the_full_size_route_is_refused(data, with_lowres, fused_on):
    model = _Stub(data[0], SIZE, with_lowres=with_lowres)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ppq, "FUSED_LOWRES", fused_on)
        with pytest.raises(ValueError, match="class_balanced"):
            _round(model, data, True, class_balanced=True)
    assert model.calls == {"forward_lowres": 0, "forward": 0}
