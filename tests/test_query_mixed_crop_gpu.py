"""Selector-level GPU test of the mixed-crop split: two images whose PADDED shapes are equal (voc, stride_total = 16: 64 x 96 and
56 x 96 both forward as 64 x 96) but whose crops differ land in one pending batch, and a round with class_balanced or diverse_picks
(alone and on the region ranking) re-batches them by crop, because the rules after the ranking work on one crop per launch.  Every
image's picks equal the composition called by hand through the wrappers at that image's OWN crop, on the pipelined and on the
one-launch route, and numpy's stream is left where it was.

Stub model and loader in tests/test_query_balance_gpu.py's arrangement: prepared 16 x 24 classifier outputs, full size 64 x 96."""
import tempfile
from argparse import Namespace

import numpy as np
import pytest
import torch

from pixelpick_amd import acquisition as acq
from pixelpick_amd import query as ppq
from pixelpick_amd.predict import predict_lowres

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C, LOWSIZE, SIZE = 19, (16, 24), (64, 96)
CROPS = [(64, 96), (56, 96)]
K, TOP = 6, 0.05


class _Stub(torch.nn.Module):
    """The prepared classifier outputs lows[i] [1,h,w,C] of the images whose indices sit in x[:,0,0,0] (reflect padding at the right
    and bottom leaves that element alone)."""
    LOWRES_ALIGN_CORNERS = True

    def __init__(self, lows):
        super().__init__()
        self.lows, self.n_classes, self.batches = lows, C, []

    def turn_on_dropout(self):
        pass

    def forward_lowres(self, x):
        assert tuple(x.shape[2:]) == SIZE
        ids = [int(round(float(v))) for v in x[:, 0, 0, 0].cpu()]
        self.batches.append(ids)
        return torch.cat([self.lows[i] for i in ids], dim=0), SIZE

    def forward(self, x):
        raise AssertionError("the full-size route is not taken")


class _DS:
    def __init__(self, xs, ys, queries):
        self.xs, self.ys, self.queries, self.labelled = xs, ys, queries, None

    def label_queries(self, d, nth):
        self.labelled = (d, nth)


class _DL:
    def __init__(self, ds):
        self.dataset = ds

    def __iter__(self):
        for i, (x, y) in enumerate(zip(self.dataset.xs, self.dataset.ys)):
            yield {"x": x[None], "y": y[None], "p_img": [f"/img{i}.png"]}


@pytest.fixture(scope="module")
def data():
    rng = np.random.RandomState(41)
    lows, xs, ys, prev = [], [], [], []
    for i, (h, w) in enumerate(CROPS):
        coarse = torch.from_numpy(rng.randn(1, C, 4, 6).astype(np.float32) * 3)
        base = torch.nn.functional.interpolate(coarse, size=LOWSIZE, mode="bilinear", align_corners=True)[0].permute(1, 2, 0).numpy()
        lows.append(torch.from_numpy((base[None] + 0.5 * rng.randn(1, *LOWSIZE, C)).astype(np.float32)).to(DEV))
        x = torch.zeros(3, h, w)
        x[0, 0, 0] = float(i)
        xs.append(x)
        ys.append(torch.from_numpy(rng.randint(0, C + 1, (h, w))))           # label C = ignore_index
        prev.append(rng.rand(h, w) < 0.01)
    return lows, xs, ys, prev


def _round(data, pipeline, **kw):
    lows, xs, ys, prev = data
    model = _Stub(lows)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ppq, "QUERY_PIPELINE", pipeline)
        with tempfile.TemporaryDirectory() as td:
            args = Namespace(dataset_name="voc", debug=False, dir_root=td, experim_name="mixed", ignore_index=C, mc_n_steps=4, n_classes=C,
                             n_pixels_by_us=K, network_name="deeplab", query_strategy="entropy", reverse_order=False, stride_total=16,
                             top_n_percent=TOP, use_mc_dropout=False, vote_type="soft", **kw)
            np.random.seed(4)
            qs = ppq.QuerySelector(args, _DL(_DS(xs, ys, prev)), device=torch.device(DEV))
            dq = qs(nth_query=1, model=model)
    return dq, model


def _by_hand(data, i, rule, r):
    """Image i alone, at its own crop, through the wrappers -> its picks, ascending."""
    lows, _, ys, prev = data
    h, w = CROPS[i]
    geom = dict(crop=(h, w), align_corners=True)
    M = int(h * w * TOP)
    excl = torch.from_numpy((prev[i] | (ys[i].numpy() == C))[None]).to(DEV)
    pred, _ = predict_lowres(lows[i], SIZE, want_pred=True, **geom)
    if r:
        unc = acq.score_topk_lowres(lows[i], SIZE, None, "entropy", 0, **geom)[2]
        rmap = acq.region_score_map(pred, unc, r, C, exclude=excl)
        cand, _ = acq.topk_select(rmap.reshape(1, h * w), M, True)
    else:
        cand, _, _ = acq.score_topk_lowres(lows[i], SIZE, excl, "entropy", M, **geom)
    assert cand.shape == (1, M)
    if rule == "class_balanced":
        idx = acq.class_balance_select(cand, pred, K, exclude=excl)[0]
    else:
        feat = acq.prob_at_lowres(lows[i], SIZE, np.zeros(M, dtype=np.int32), cand.reshape(-1), **geom)
        idx = acq.diverse_select(cand, feat.view(1, M, -1), K, n_features=C, exclude=excl, n_pixels=h * w)[0]
    return sorted(idx[0].cpu().numpy().astype(np.int64).tolist())


@pytest.mark.parametrize("r", [0, 1])
@pytest.mark.parametrize("rule", ["class_balanced", "diverse_picks"])
def test_each_image_is_selected_at_its_own_crop(data, rule, r):
    assert [int(h * w * TOP) for h, w in CROPS] == [307, 268]
    want = [_by_hand(data, i, rule, r) for i in range(len(CROPS))]
    assert all(len(set(p)) == K for p in want) and want[0] != want[1]
    for pipeline in (True, False):
        dq, model = _round(data, pipeline, region_radius=r, **{rule: True})
        after = np.random.rand()
        np.random.seed(4)
        assert np.random.rand() == after              # nothing was drawn from numpy's stream
        assert model.batches == [[0], [1]]            # one pending batch of equal padded shapes, split by crop
        for i, (h, w) in enumerate(CROPS):
            q = dq[f"/img{i}.png"]
            assert (q["height"], q["width"]) == (h, w)
            got = (q["y_coords"].astype(np.int64) * w + q["x_coords"]).tolist()
            assert got == want[i], (rule, r, pipeline, i)
