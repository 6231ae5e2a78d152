"""Selector-level GPU tests of the MC-dropout mean-probability modes: QuerySelector with use_mc_dropout and `vote_type="consensus"` scores
the strategy on the mean probability of the passes, `query_strategy="bald"` their mutual information (tests/mean_oracle.py) - on the
route from the classifier output (pp_acq_lowres_mc_mean_topk) and on the full-size route (pp_acq_softmax_sum +
pp_acq_mean_prob_score_map + pp_topk_select) - and every other `vote_type` is left as it was.

A stub model hands the selector PREPARED classifier outputs (tests/test_query_vote_gpu.py's arrangement); the real DeepLab runs at the
64 x 96 golden size."""
import tempfile
from argparse import Namespace

import numpy as np
import pytest
import torch

import mean_oracle as mo
from pixelpick_amd import acquisition as acq
from pixelpick_amd import engine as E
from pixelpick_amd import query as ppq

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (query_strategy, vote_type)
MODES = [("entropy", "consensus"), ("least_confidence", "consensus"), ("margin_sampling", "consensus"), ("bald", "soft"), ("bald", "consensus")]


def _pred(low, size, align=True):
    return E.bilinear(E.Tape(False), E.Var(low), size, align, 0.0, out_nchw=True).t


class _Stub(torch.nn.Module):
    """forward_lowres returns the prepared [T,h,w,C] tensor of the image whose index sits in x[0,0,0,0]; forward() is its pp_bilinear_fwd."""
    LOWRES_ALIGN_CORNERS = True

    def __init__(self, lows, size, with_lowres=True):
        super().__init__()
        self.lows, self.size, self.n_classes = lows, size, lows[0].shape[-1]
        self.calls = {"forward_lowres": 0, "forward": 0}
        self.cursor = {}
        if with_lowres:
            self.forward_lowres = self._forward_lowres

    def turn_on_dropout(self):
        pass

    def _low(self, x):
        """The next x.shape[0] passes of the image (all of them in one forward unless the selector chunks the passes)."""
        i = int(round(float(x[0, 0, 0, 0])))
        c = self.cursor.get(i, 0) % self.lows[i].shape[0]
        self.cursor[i] = c + x.shape[0]
        assert c + x.shape[0] <= self.lows[i].shape[0]
        return self.lows[i][c:c + x.shape[0]]

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
    base = dict(dataset_name="cs", debug=False, dir_root="/tmp", experim_name="mean", ignore_index=19, mc_n_steps=4, n_classes=19,
                n_pixels_by_us=20, network_name="deeplab", query_strategy="entropy", reverse_order=False, stride_total=8,
                top_n_percent=0.0, use_mc_dropout=True, vote_type="consensus")
    base.update(kw)
    return Namespace(**base)


def _stub_data(n, C, T, lowsize, size, seed=5):
    rng = np.random.RandomState(seed)
    h, w = lowsize
    lows = [torch.from_numpy((np.repeat(rng.randn(1, h, w, C) * 3, T, axis=0) + 0.7 * rng.randn(T, h, w, C)).astype(np.float32)).to(DEV)
            for _ in range(n)]
    H, W = size
    xs = torch.zeros(n, 3, H, W)
    xs[:, 0, 0, 0] = torch.arange(n, dtype=torch.float32)
    ys = torch.from_numpy(rng.randint(0, C + 1, (n, H, W)))              # label C = ignore_index
    prev = [rng.rand(H, W) < 0.01 for _ in range(n)]
    return lows, xs, ys, prev, [f"/img{i}.png" for i in range(n)]


def _round(model, xs, ys, prev, names, fused, **kw):
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ppq, "FUSED_LOWRES", fused)
        with tempfile.TemporaryDirectory() as td:
            np.random.seed(4)
            E.set_dropout_seed(7)
            qs = ppq.QuerySelector(_args(dir_root=td, **kw), _DL(_DS(xs, ys, prev, names)), device=torch.device(DEV))
            dq = qs(nth_query=1, model=model)
    return dq, qs.query_stats


def _flat(dq, name, W):
    return (dq[name]["y_coords"].astype(np.int64) * W + dq[name]["x_coords"]).tolist()


def _assert_same_stats(sa, sb):
    """The bar of the MC selector test (tests/test_acq_mc_lowres_gpu.py): everything equal, the entropies to 2e-5 / 2e-6."""
    assert sa.dict_label_cnt == sb.dict_label_cnt
    assert sa.list_n_unique_labels == sb.list_n_unique_labels
    assert sa.list_spatial_coverage == sb.list_spatial_coverage
    assert len(sa.list_entropy) == len(sb.list_entropy) > 0
    np.testing.assert_allclose(np.asarray(sa.list_entropy, dtype=np.float64), np.asarray(sb.list_entropy, dtype=np.float64),
                               rtol=2e-5, atol=2e-6)


def _composition_picks(passes_nchw, chunks, excl, st, k):
    """What the full-size route launches for one image: pp_acq_softmax_sum per chunk of passes, pp_acq_mean_prob_score_map, pp_topk_select."""
    T, C, H, W = passes_nchw.shape
    prob = torch.empty((1, C, H, W), dtype=torch.float32, device=DEV)
    ment = torch.empty((H, W), dtype=torch.float32, device=DEV)
    at = 0
    for t in chunks:
        acq.mc_accumulate_(passes_nchw[at:at + t], prob[0], ment, "entropy", 1.0 / T, accumulate=at > 0)
        at += t
    m = acq.mean_prob_score_map(prob, ment[None] if st == "bald" else None, excl[None], st)
    idx, _ = acq.topk_select(m.reshape(1, H * W), k, acq.MEAN_LARGEST[st])
    return sorted(idx[0].cpu().numpy().astype(np.int64).tolist())


@pytest.mark.parametrize("st,vote", MODES)
def test_both_routes_return_the_kernels_picks_and_the_same_statistics(st, vote):
    n, C, T, lowsize, size = 2, 19, 4, (16, 24), (64, 96)
    lows, xs, ys, prev, names = _stub_data(n, C, T, lowsize, size)
    model = _Stub(lows, size)
    fused = _round(model, xs, ys, prev, names, True, query_strategy=st, vote_type=vote)
    assert model.calls == {"forward_lowres": n, "forward": 0}
    plain = _round(model, xs, ys, prev, names, False, query_strategy=st, vote_type=vote)
    assert model.calls == {"forward_lowres": n, "forward": n}
    for i, nme in enumerate(names):
        excl = prev[i] | (ys[i].numpy() == C)
        idx, _, _ = acq.mc_mean_topk_lowres(lows[i], T, size, excl[None], st, 20)
        want = sorted(idx[0].cpu().numpy().astype(np.int64).tolist())
        assert not excl.reshape(-1)[want].any()
        assert _flat(fused[0], nme, size[1]) == want and _flat(plain[0], nme, size[1]) == want
        # and those are the float64 oracle's picks wherever the 20th and 21st scores are further apart than the kernels' error
        m = mo.score_map(_pred(lows[i], size).cpu().numpy(), excl, st)
        order = mo.picks(m, 21, st)
        if abs(m.reshape(-1)[order[19]] - m.reshape(-1)[order[20]]) > 1e-4:
            assert want == sorted(order[:20].tolist())
    _assert_same_stats(fused[1], plain[1])


def _disagreement_image(with_b):
    """Identity geometry, T = 4, C = 19.  A: the passes split 2 : 2 between two classes, each pass confident.  B: unanimous passes with a
    flat softmax (entropy ~ ln C).  B': unanimous passes, two classes at 0.8 : 0.2 (per-pass entropy ~ 0.5).  Elsewhere confident and
    unanimous."""
    C, T, size = 19, 4, (16, 24)
    x = np.full((T, size[0], size[1], C), -20.0, dtype=np.float32)
    x[..., 7] = 20.0
    a, b, b2 = (5, 9), (11, 3), (13, 20)
    x[:, a[0], a[1], :] = -20.0
    x[:2, a[0], a[1], 2] = 20.0
    x[2:, a[0], a[1], 12] = 20.0
    if with_b:
        x[:, b[0], b[1], :] = 0.0
        x[:, b[0], b[1], 4] = 0.01
    x[:, b2[0], b2[1], :] = -20.0
    x[:, b2[0], b2[1], 4] = float(np.log(4.0))
    x[:, b2[0], b2[1], 9] = 0.0
    return [torch.from_numpy(x).to(DEV)], size, a, b, b2


@pytest.mark.parametrize("fused", [True, False])
def test_bald_consensus_and_soft_disagree_where_they_must(fused):
    """With one pixel per image: BALD picks A (all of its entropy is disagreement), the consensus entropy and the soft vote pick B (the
    most ambiguous pixel).  Without B: the consensus picks A (ln 2 > 0.5) while the soft vote - the mean of per-pass entropies that are
    ~ 0 at A - picks B'."""
    def pick(lows, size, **kw):
        xs, ys = torch.zeros(1, 3, *size), torch.zeros(1, *size, dtype=torch.int64)
        dq, _ = _round(_Stub(lows, size), xs, ys, [np.zeros(size, dtype=bool)], ["/img0.png"], fused, n_pixels_by_us=1, **kw)
        return int(dq["/img0.png"]["y_coords"][0]), int(dq["/img0.png"]["x_coords"][0])

    lows, size, a, b, b2 = _disagreement_image(True)
    assert pick(lows, size, query_strategy="bald", vote_type="soft") == a
    assert pick(lows, size, query_strategy="entropy", vote_type="consensus") == b
    assert pick(lows, size, query_strategy="entropy", vote_type="soft") == b
    lows, size, a, b, b2 = _disagreement_image(False)
    assert pick(lows, size, query_strategy="bald", vote_type="soft") == a
    assert pick(lows, size, query_strategy="entropy", vote_type="consensus") == a
    assert pick(lows, size, query_strategy="entropy", vote_type="soft") == b2


@pytest.mark.parametrize("st,vote", [("entropy", "consensus"), ("bald", "soft")])
def test_chunked_passes_take_the_full_size_route(st, vote):
    """mc_chunk = 3 < mc_n_steps = 4: two forwards per image, the mean probability (and mean entropy) accumulated over both."""
    n, C, T, lowsize, size = 2, 19, 4, (16, 24), (64, 96)
    lows, xs, ys, prev, names = _stub_data(n, C, T, lowsize, size, seed=9)
    model = _Stub(lows, size)                  # forward_lowres exists and is not called: the passes do not fit one forward
    dq, _ = _round(model, xs, ys, prev, names, True, mc_chunk=3, query_strategy=st, vote_type=vote)
    assert model.calls == {"forward_lowres": 0, "forward": 2 * n} and model.cursor == {0: T, 1: T}
    for i, nme in enumerate(names):
        excl = prev[i] | (ys[i].numpy() == C)
        assert _flat(dq, nme, size[1]) == _composition_picks(_pred(lows[i], size), [3, 1], excl, st, 20)


@pytest.mark.parametrize("st,vote", [("least_confidence", "consensus"), ("bald", "consensus")])
def test_models_without_forward_lowres_and_wide_heads_are_served(st, vote):
    """Unlike the hard vote no model is left out: both take the full-size route, silently and with the specified scores."""
    T, lowsize, size = 3, (8, 12), (32, 48)
    for C, with_lowres in ((19, False), (70, True)):
        lows, xs, ys, prev, names = _stub_data(1, C, T, lowsize, size, seed=C)
        model = _Stub(lows, size, with_lowres=with_lowres)
        dq, _ = _round(model, xs, ys, prev, names, True, mc_n_steps=T, n_classes=C, ignore_index=C, query_strategy=st, vote_type=vote)
        assert model.calls == {"forward_lowres": 0, "forward": 1}
        excl = prev[0] | (ys[0].numpy() == C)
        assert _flat(dq, names[0], size[1]) == _composition_picks(_pred(lows[0], size), [T], excl, st, 20)


def test_any_other_vote_type_keeps_the_soft_vote():
    n, C, T, lowsize, size = 2, 19, 4, (16, 24), (64, 96)
    lows, xs, ys, prev, names = _stub_data(n, C, T, lowsize, size)
    for fused in (True, False):
        dq, _ = _round(_Stub(lows, size), xs, ys, prev, names, fused, vote_type="anything-else")
        for i, nme in enumerate(names):
            excl = prev[i] | (ys[i].numpy() == C)
            idx, _, _ = acq.mc_score_topk_lowres(lows[i], T, size, excl[None], "entropy", 20)
            assert _flat(dq, nme, size[1]) == sorted(idx[0].cpu().numpy().astype(np.int64).tolist())


def test_random_strategy_ignores_the_vote_type():
    n, C, T, lowsize, size = 2, 19, 4, (16, 24), (64, 96)
    lows, xs, ys, prev, names = _stub_data(n, C, T, lowsize, size)
    out = []
    for vote in ("consensus", "soft"):
        torch.manual_seed(13)
        dq, _ = _round(_Stub(lows, size), xs, ys, prev, names, True, query_strategy="random", vote_type=vote)
        out.append([_flat(dq, nme, size[1]) for nme in names])
    assert out[0] == out[1]


# ---------------------------------------------------------------- the real network at the golden size
def _deeplab(C):
    from pixelpick_amd.networks.deeplab import DeepLab
    return DeepLab(Namespace(use_mc_dropout=True, mc_dropout_p=0.2, n_classes=C, use_aspp=True, use_softmax=False, use_img_inp=False)).to(DEV)


@pytest.mark.parametrize("st,vote,top_n", [("bald", "soft", 0.0), ("entropy", "consensus", 0.0), ("margin_sampling", "consensus", 0.05)])
def test_one_round_through_deeplab_both_routes(monkeypatch, st, vote, top_n):
    C, n, (h, w) = 19, 2, (64, 96)
    model = _deeplab(C)
    torch.manual_seed(3)
    xs, ys = torch.randn(n, 3, h, w), torch.randint(0, C + 1, (n, h, w))
    rng = np.random.RandomState(0)
    prev = [rng.rand(h, w) < 0.01 for _ in range(n)]
    names = [f"/img{i}.png" for i in range(n)]
    seen = []
    orig = model.forward_lowres
    monkeypatch.setattr(model, "forward_lowres", lambda x: (lambda r: (seen.append(r[0].clone()), r)[1])(orig(x)), raising=False)
    kw = dict(query_strategy=st, vote_type=vote, top_n_percent=top_n)
    fused = _round(model, xs, ys, prev, names, True, **kw)
    assert len(seen) == n
    plain = _round(model, xs, ys, prev, names, False, **kw)
    assert len(seen) == n                                      # the full-size route does not stop in front of the upsample
    k = int(h * w * top_n) if top_n > 0 else 20
    np.random.seed(4)                                          # the selector's host draws (top-5 % sub-sample), image by image
    for i, nme in enumerate(names):
        assert _flat(fused[0], nme, w) == _flat(plain[0], nme, w)
        excl = prev[i] | (ys[i].numpy() == C)
        idx, _, _ = acq.mc_mean_topk_lowres(seen[i], 4, (h, w), excl[None], st, k)
        pk = idx[0].cpu().numpy().astype(np.int64)
        if top_n > 0:
            pk = pk[np.random.choice(k, 20, False)]
        assert _flat(fused[0], nme, w) == sorted(pk.tolist())
    _assert_same_stats(fused[1], plain[1])
