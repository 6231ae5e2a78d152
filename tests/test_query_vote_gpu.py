"""Selector-level GPU tests of `vote_type="hard"` (args.py:34): QuerySelector with use_mc_dropout scores the vote shares of the passes
(tests/vote_oracle.py) on the route from the classifier output (pp_acq_lowres_mc_vote_topk) and on the full-size route
(pp_acq_vote_accumulate + pp_acq_vote_score_map + pp_topk_select), and leaves `vote_type="soft"` as it was.

A stub model hands the selector PREPARED classifier outputs, so the oracle sees the very logits the kernels vote on (the device's own
pp_bilinear_fwd output, downloaded): coordinates are compared for equality.  The real DeepLab runs at the 64 x 96 golden size."""
import tempfile
from argparse import Namespace

import numpy as np
import pytest
import torch

import vote_oracle as vo
from pixelpick_amd import acquisition as acq
from pixelpick_amd import engine as E
from pixelpick_amd import query as ppq

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STRATS = ["entropy", "least_confidence", "margin_sampling"]


def _pred(low, size, align=True):
    return E.bilinear(E.Tape(False), E.Var(low), size, align, 0.0, out_nchw=True).t


class _Stub(torch.nn.Module):
    """forward_lowres returns the prepared [T,h,w,C] tensor of the image whose index sits in x[0,0,0,0]; forward() is its pp_bilinear_fwd."""
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
        low = self.lows[int(round(float(x[0, 0, 0, 0])))]
        assert x.shape[0] == low.shape[0], "the passes of one image arrive in one forward"
        return low

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
    base = dict(dataset_name="cs", debug=False, dir_root="/tmp", experim_name="vote", ignore_index=19, mc_n_steps=4, n_classes=19,
                n_pixels_by_us=20, network_name="deeplab", query_strategy="entropy", reverse_order=False, stride_total=8,
                top_n_percent=0.0, use_mc_dropout=True, vote_type="hard")
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


@pytest.mark.parametrize("st", STRATS)
def test_hard_vote_returns_the_oracles_coordinates_on_both_routes(st):
    n, C, T, lowsize, size = 2, 19, 4, (16, 24), (64, 96)
    lows, xs, ys, prev, names = _stub_data(n, C, T, lowsize, size)
    model = _Stub(lows, size)
    fused = _round(model, xs, ys, prev, names, True, query_strategy=st)
    assert model.calls == {"forward_lowres": n, "forward": 0}
    plain = _round(model, xs, ys, prev, names, False, query_strategy=st)
    assert model.calls == {"forward_lowres": n, "forward": n}
    for i, nme in enumerate(names):
        excl = prev[i] | (ys[i].numpy() == C)
        want = vo.score_map(_pred(lows[i], size).cpu().numpy(), excl, st)
        picks = sorted(vo.picks(want, 20, st).tolist())
        assert not excl.reshape(-1)[picks].any()
        assert _flat(fused[0], nme, size[1]) == picks
        assert _flat(plain[0], nme, size[1]) == picks
    _assert_same_stats(fused[1], plain[1])


def test_a_model_without_forward_lowres_keeps_the_mean_score_and_says_so():
    """The vote is specified on pp_bilinear_fwd's logits: a model that does not expose its classifier output keeps the picks it had
    (tests/test_acq_gpu.py pins them with vote_type="hard" in its arguments), with a warning - not silently."""
    n, C, T, lowsize, size = 2, 19, 4, (16, 24), (64, 96)
    lows, xs, ys, prev, names = _stub_data(n, C, T, lowsize, size)
    with pytest.warns(RuntimeWarning, match="forward_lowres"):
        hard = _round(_Stub(lows, size, with_lowres=False), xs, ys, prev, names, True)
    soft = _round(_Stub(lows, size, with_lowres=False), xs, ys, prev, names, True, vote_type="soft")
    for nme in names:
        assert _flat(hard[0], nme, size[1]) == _flat(soft[0], nme, size[1])


def test_hard_vote_chunked_passes_take_the_full_size_route():
    """mc_chunk = 3 < mc_n_steps = 4: two forwards per image, the votes accumulated over both."""
    n, C, T, lowsize, size = 2, 19, 4, (16, 24), (64, 96)
    lows, xs, ys, prev, names = _stub_data(n, C, T, lowsize, size, seed=9)

    class _Chunked(_Stub):
        """Hands out the passes of an image in the order the selector asks for them."""
        def __init__(self, *a):
            super().__init__(*a)               # forward_lowres exists and is not called: the passes do not fit one forward
            self.cursor = {}

        def _low(self, x):
            i = int(round(float(x[0, 0, 0, 0])))
            c = self.cursor.get(i, 0)
            self.cursor[i] = c + x.shape[0]
            return self.lows[i][c:c + x.shape[0]]

    model = _Chunked(lows, size)
    dq, _ = _round(model, xs, ys, prev, names, True, mc_chunk=3)
    assert model.calls == {"forward_lowres": 0, "forward": 2 * n} and model.cursor == {0: T, 1: T}
    for i, nme in enumerate(names):
        excl = prev[i] | (ys[i].numpy() == C)
        want = vo.score_map(_pred(lows[i], size).cpu().numpy(), excl, "entropy")
        assert _flat(dq, nme, size[1]) == sorted(vo.picks(want, 20, "entropy").tolist())


@pytest.mark.parametrize("st", STRATS)
def test_soft_vote_is_the_mean_score_as_before(st):
    """vote_type="soft" (and any value other than "hard"): the picks of pp_acq_lowres_mc_score_topk, the entry this change leaves alone,
    on both routes."""
    n, C, T, lowsize, size = 2, 19, 4, (16, 24), (64, 96)
    lows, xs, ys, prev, names = _stub_data(n, C, T, lowsize, size)
    model = _Stub(lows, size)
    for vote in ("soft", "anything-else"):
        fused = _round(model, xs, ys, prev, names, True, query_strategy=st, vote_type=vote)
        plain = _round(model, xs, ys, prev, names, False, query_strategy=st, vote_type=vote)
        for i, nme in enumerate(names):
            excl = prev[i] | (ys[i].numpy() == C)
            idx, _, _ = acq.mc_score_topk_lowres(lows[i], T, size, excl[None], st, 20)
            want = sorted(idx[0].cpu().numpy().astype(np.int64).tolist())
            assert _flat(fused[0], nme, size[1]) == want and _flat(plain[0], nme, size[1]) == want
        _assert_same_stats(fused[1], plain[1])


def test_hard_and_soft_votes_disagree_where_they_must():
    """Identity geometry.  Pixel A: the passes split evenly between two classes, each pass confident - soft entropy ~ 0, vote entropy
    ln 2.  Pixel B: unanimous passes with a flat softmax - soft entropy ~ ln C, vote entropy 0.  Everywhere else: confident and
    unanimous.  With one pixel per image the hard vote picks A and the soft vote picks B."""
    C, T, size = 19, 4, (16, 24)
    x = np.full((T, size[0], size[1], C), -20.0, dtype=np.float32)
    x[..., 7] = 20.0
    a, b = (5, 9), (11, 3)
    x[:, a[0], a[1], :] = -20.0
    x[:2, a[0], a[1], 2] = 20.0
    x[2:, a[0], a[1], 12] = 20.0
    x[:, b[0], b[1], :] = 0.0
    x[:, b[0], b[1], 4] = 0.01
    lows = [torch.from_numpy(x).to(DEV)]
    xs, ys = torch.zeros(1, 3, *size), torch.zeros(1, *size, dtype=torch.int64)
    prev, names = [np.zeros(size, dtype=bool)], ["/img0.png"]
    for fused in (True, False):
        model = _Stub(lows, size)
        hard, _ = _round(model, xs, ys, prev, names, fused, n_pixels_by_us=1, vote_type="hard")
        soft, _ = _round(model, xs, ys, prev, names, fused, n_pixels_by_us=1, vote_type="soft")
        assert (int(hard[names[0]]["y_coords"][0]), int(hard[names[0]]["x_coords"][0])) == a
        assert (int(soft[names[0]]["y_coords"][0]), int(soft[names[0]]["x_coords"][0])) == b


def test_random_strategy_ignores_the_vote_type():
    n, C, T, lowsize, size = 2, 19, 4, (16, 24), (64, 96)
    lows, xs, ys, prev, names = _stub_data(n, C, T, lowsize, size)
    out = []
    for vote in ("hard", "soft"):
        torch.manual_seed(13)
        dq, _ = _round(_Stub(lows, size), xs, ys, prev, names, True, query_strategy="random", vote_type=vote)
        out.append([_flat(dq, nme, size[1]) for nme in names])
    assert out[0] == out[1]


# ---------------------------------------------------------------- the real network at the golden size
def _deeplab(C):
    from pixelpick_amd.networks.deeplab import DeepLab
    return DeepLab(Namespace(use_mc_dropout=True, mc_dropout_p=0.2, n_classes=C, use_aspp=True, use_softmax=False, use_img_inp=False)).to(DEV)


@pytest.mark.parametrize("st,top_n", [("entropy", 0.0), ("margin_sampling", 0.0), ("least_confidence", 0.05)])
def test_hard_vote_through_deeplab_both_routes_and_the_oracle(monkeypatch, st, top_n):
    C, n, (h, w) = 19, 3, (64, 96)
    model = _deeplab(C)
    torch.manual_seed(3)
    xs, ys = torch.randn(n, 3, h, w), torch.randint(0, C + 1, (n, h, w))
    rng = np.random.RandomState(0)
    prev = [rng.rand(h, w) < 0.01 for _ in range(n)]
    names = [f"/img{i}.png" for i in range(n)]
    seen = []
    orig = model.forward_lowres
    monkeypatch.setattr(model, "forward_lowres", lambda x: (lambda r: (seen.append(r[0].clone()), r)[1])(orig(x)), raising=False)
    kw = dict(query_strategy=st, top_n_percent=top_n)
    fused = _round(model, xs, ys, prev, names, True, **kw)
    assert len(seen) == n
    plain = _round(model, xs, ys, prev, names, False, **kw)
    assert len(seen) == n                                      # the full-size route does not stop in front of the upsample
    k = int(h * w * top_n) if top_n > 0 else 20
    np.random.seed(4)                                          # the selector's host draws (top-5 % sub-sample), image by image
    for i, nme in enumerate(names):
        assert _flat(fused[0], nme, w) == _flat(plain[0], nme, w)
        excl = prev[i] | (ys[i].numpy() == C)
        want = vo.score_map(_pred(seen[i], (h, w)).cpu().numpy(), excl, st)
        pk = vo.picks(want, k, st)
        if top_n > 0:
            pk = pk[np.random.choice(k, 20, False)]
        assert _flat(fused[0], nme, w) == sorted(pk.tolist())
    _assert_same_stats(fused[1], plain[1])
