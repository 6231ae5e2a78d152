"""Selector-level GPU tests of `min_pixel_distance`: one QuerySelector round on every scoring route, held to the numpy oracle's greedy
pass (tests/spread_oracle.py) over the FULL ranking of that route's own score map - the selector only ever sees the first
M = spread_candidates(k, d, h*w) < h*w ranks, so the candidate bound does the work - and the option switched off changes nothing.

Stub models hand the selector PREPARED classifier outputs (tests/test_query_vote_gpu.py's arrangement) at the 64 x 96 golden size."""
import tempfile
from argparse import Namespace

import numpy as np
import pytest
import torch

import spread_oracle as so
from pixelpick_amd import acquisition as acq
from pixelpick_amd import engine as E
from pixelpick_amd import query as ppq

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_IMG, C, T, LOWSIZE, SIZE = 2, 19, 4, (16, 24), (64, 96)
K, D = 6, 5
# name -> selector arguments
MODES = {
    "single": dict(use_mc_dropout=False),
    "mc_soft": dict(use_mc_dropout=True, vote_type="soft"),
    "mc_hard": dict(use_mc_dropout=True, vote_type="hard"),
    "mc_consensus": dict(use_mc_dropout=True, vote_type="consensus"),
    "mc_bald": dict(use_mc_dropout=True, vote_type="soft", query_strategy="bald"),
}


def _pred(low, size, align=True):
    return E.bilinear(E.Tape(False), E.Var(low), size, align, 0.0, out_nchw=True).t


class _Stub(torch.nn.Module):
    """The prepared classifier outputs lows[i] [T,h,w,C] of the images whose indices sit in x[:,0,0,0].  A single-pass forward takes
    pass 0 of every image of the batch; an MC forward (T copies of one image) takes that image's T passes."""
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
        ids = [int(round(float(v))) for v in x[:, 0, 0, 0].cpu()]
        if len(ids) == self.lows[0].shape[0] and len(set(ids)) == 1 and len(ids) > 1:
            return self.lows[ids[0]]
        return torch.cat([self.lows[i][:1] for i in ids], dim=0)

    def _forward_lowres(self, x):
        self.calls["forward_lowres"] += 1
        return self._low(x), self.size

    def forward(self, x):
        self.calls["forward"] += 1
        return {"pred": _pred(self._low(x), self.size)}


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
    base = dict(dataset_name="cs", debug=False, dir_root="/tmp", experim_name="spread", ignore_index=C, mc_n_steps=T, n_classes=C,
                n_pixels_by_us=K, network_name="deeplab", query_strategy="entropy", reverse_order=False, stride_total=8,
                top_n_percent=0.0, use_mc_dropout=False, vote_type="soft")
    base.update(kw)
    return Namespace(**base)


@pytest.fixture(scope="module")
def data():
    """Smooth classifier outputs (a coarse random field, upsampled): the uncertain pixels sit together, as on a real map."""
    rng = np.random.RandomState(21)
    h, w = LOWSIZE
    lows = []
    for _ in range(N_IMG):
        coarse = torch.from_numpy(rng.randn(1, C, 4, 6).astype(np.float32) * 3)
        base = torch.nn.functional.interpolate(coarse, size=(h, w), mode="bilinear", align_corners=True)[0].permute(1, 2, 0).numpy()
        lows.append(torch.from_numpy((base[None] + 0.7 * rng.randn(T, h, w, C)).astype(np.float32)).to(DEV))
    H, W = SIZE
    xs = torch.zeros(N_IMG, 3, H, W)
    xs[:, 0, 0, 0] = torch.arange(N_IMG, dtype=torch.float32)
    ys = torch.from_numpy(rng.randint(0, C + 1, (N_IMG, H, W)))           # label C = ignore_index
    prev = [rng.rand(H, W) < 0.01 for _ in range(N_IMG)]
    return lows, xs, ys, prev, [f"/img{i}.png" for i in range(N_IMG)]


def _round(model, data, fused=True, pipeline=True, **kw):
    _, xs, ys, prev, names = data
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ppq, "FUSED_LOWRES", fused)
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


def _route_map(mode, low, excl, st):
    """The route's own score map of one image, from the entry's out_map (k = 0: map only), and its fill / direction."""
    e = excl[None]
    if mode == "single":
        m = acq.score_topk_lowres(low[:1], SIZE, e, st, 0)[2]
        return m, acq.FILL[st], acq.LARGEST[st]
    if mode == "full_size":
        m = acq.score_topk(_pred(low[:1], SIZE), e, st, 1, return_map=True)[2]
        return m, acq.FILL[st], acq.LARGEST[st]
    if mode == "mc_soft":
        m = acq.mc_score_topk_lowres(low, T, SIZE, e, st, 0)[2]
        return m, acq.FILL[st], acq.LARGEST[st]
    if mode == "mc_hard":
        m = acq.mc_vote_topk_lowres(low, T, SIZE, e, st, 0)[2]
        return m, acq.VOTE_FILL[st], acq.LARGEST[st]
    m = acq.mc_mean_topk_lowres(low, T, SIZE, e, st, 0)[2]
    return m, acq.MEAN_FILL[st], acq.MEAN_LARGEST[st]


def _want(mode, data, i, st):
    lows, _, ys, prev, _ = data
    excl = prev[i] | (ys[i].numpy() == C)
    m, fill, largest = _route_map(mode, lows[i], excl, st)
    m = m[0].cpu().numpy().reshape(-1)
    ex = excl.reshape(-1)
    N = m.size
    M = acq.spread_candidates(K, D, N)
    assert M < N and M == 5 * 69 + 1                           # the selector sees 346 of 6144 ranks
    # the precondition of the bound: every un-excluded score differs from the fill, and at least M pixels are un-excluded
    assert (m[~ex] != np.float32(fill)).all() and (m[ex] == np.float32(fill)).all() and (~ex).sum() >= M
    idx, _, n = so.select(so.ranking(m, largest), SIZE[1], K, D, ex)
    assert n == K and not ex[idx].any()
    yy, xx = np.divmod(idx.astype(np.int64), SIZE[1])
    d2 = (yy[:, None] - yy[None]) ** 2 + (xx[:, None] - xx[None]) ** 2
    assert (d2[~np.eye(K, dtype=bool)] >= D * D).all()
    return sorted(idx.tolist())


def _assert_same_stats(sa, sb):
    assert sa.dict_label_cnt == sb.dict_label_cnt
    assert sa.list_n_unique_labels == sb.list_n_unique_labels
    assert sa.list_spatial_coverage == sb.list_spatial_coverage
    assert len(sa.list_entropy) == len(sb.list_entropy) == N_IMG * K
    np.testing.assert_allclose(np.asarray(sa.list_entropy, dtype=np.float64), np.asarray(sb.list_entropy, dtype=np.float64),
                               rtol=2e-5, atol=2e-6)


@pytest.mark.parametrize("st", ["entropy", "margin_sampling"])
def test_single_pass_routes(data, st):
    """The pipelined pass, the fused pass without the pipeline and the full-size pass of a model that has forward_lowres."""
    lows, _, _, _, names = data
    model = _Stub(lows, SIZE)
    piped = _round(model, data, True, True, min_pixel_distance=D, query_strategy=st)
    assert model.calls == {"forward_lowres": 1, "forward": 0}
    fused = _round(model, data, True, False, min_pixel_distance=D, query_strategy=st)
    assert model.calls == {"forward_lowres": 2, "forward": 0}
    plain = _round(model, data, False, False, min_pixel_distance=D, query_strategy=st)
    assert model.calls == {"forward_lowres": 2, "forward": 1}
    for i, nme in enumerate(names):
        want = _want("single", data, i, st)
        assert _picks(piped[0], nme) == want and _picks(fused[0], nme) == want and _picks(plain[0], nme) == want
    _assert_same_stats(piped[1], fused[1])
    _assert_same_stats(piped[1], plain[1])


@pytest.mark.parametrize("st", ["entropy", "least_confidence"])
def test_full_size_route_of_a_model_without_forward_lowres(data, st):
    lows, _, _, _, names = data
    model = _Stub(lows, SIZE, with_lowres=False)
    dq, stats = _round(model, data, min_pixel_distance=D, query_strategy=st)
    assert model.calls == {"forward_lowres": 0, "forward": 1} and len(stats.list_entropy) == N_IMG * K
    for i, nme in enumerate(names):
        assert _picks(dq, nme) == _want("full_size", data, i, st)


@pytest.mark.parametrize("mode", ["mc_soft", "mc_hard", "mc_consensus", "mc_bald"])
def test_mc_dropout_routes(data, mode):
    """From the classifier output in one launch, and the full-size route's pp_topk_select on the composed map: the same picks."""
    lows, _, _, _, names = data
    kw = dict(MODES[mode], min_pixel_distance=D)
    st = kw.get("query_strategy", "entropy")
    model = _Stub(lows, SIZE)
    fused = _round(model, data, True, **kw)
    assert model.calls == {"forward_lowres": N_IMG, "forward": 0}
    plain = _round(model, data, False, **kw)
    assert model.calls == {"forward_lowres": N_IMG, "forward": N_IMG}
    for i, nme in enumerate(names):
        want = _want(mode, data, i, st)
        assert _picks(fused[0], nme) == want and _picks(plain[0], nme) == want
    _assert_same_stats(fused[1], plain[1])


def test_the_picks_differ_from_plain_top_k_and_cover_more(data):
    """The point of the option: on a smooth map plain top-k clusters, the distance rule does not."""
    lows, _, _, _, names = data
    off = _round(_Stub(lows, SIZE), data)
    on = _round(_Stub(lows, SIZE), data, min_pixel_distance=D)
    assert any(_picks(off[0], nme) != _picks(on[0], nme) for nme in names)
    assert np.mean(on[1].list_spatial_coverage) > np.mean(off[1].list_spatial_coverage)


@pytest.mark.parametrize("mode", sorted(MODES) + ["full_size"])
def test_the_option_is_inert_when_off(data, mode):
    lows, _, _, _, names = data
    kw = dict(MODES.get(mode, {}))
    ref = _round(_Stub(lows, SIZE, with_lowres=mode != "full_size"), data, **kw)
    for d in (0, 1):
        got = _round(_Stub(lows, SIZE, with_lowres=mode != "full_size"), data, min_pixel_distance=d, **kw)
        for nme in names:
            assert _picks(got[0], nme) == _picks(ref[0], nme) and len(_picks(ref[0], nme)) == K
        assert got[1].list_entropy == ref[1].list_entropy and got[1].list_spatial_coverage == ref[1].list_spatial_coverage
