"""Selector-level GPU tests of `diverse_picks`: a QuerySelector round on the pipelined and on the fused non-pipelined route gives the
picks of the composition called by hand through the wrappers (score_topk_lowres at k = 307 -> prob_at_lowres -> diverse_select; with
region_radius the region ranking in the scorer's place), those picks are the oracle's (tests/diverse_oracle.py) on the device's own
candidate list and features, the full-size forward is never called, and the option switched off changes nothing.

The stub models, the loader and the prepared classifier outputs at the 64 x 96 golden size are tests/test_query_balance_gpu.py's."""
import numpy as np
import pytest
import torch

import diverse_oracle as do
from pixelpick_amd import acquisition as acq
from pixelpick_amd import query as ppq
from pixelpick_amd.predict import predict_lowres
from test_query_balance_gpu import C, DEV, K, LOWSIZE, N_IMG, POOL, SIZE, STRATEGIES, _Stub, _StubFPN, _excl, _make, _picks, _round

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def data():
    return _make(LOWSIZE, 41)


@pytest.fixture(scope="module")
def data_fpn():
    return _make((32, 48), 42)


def _by_hand(data, st, align=True, r=0):
    """The composition through the wrappers -> (picks in selection order int64 [n,K], candidate list, features, dist, n), host arrays."""
    H, W = SIZE
    low = torch.cat([l[:1] for l in data[0]], dim=0)
    excl = torch.from_numpy(_excl(data)).to(DEV)
    if r:
        pred, _ = predict_lowres(low, SIZE, crop=SIZE, align_corners=align, want_pred=True)
        unc = acq.score_topk_lowres(low, SIZE, None, st, 0, crop=SIZE, align_corners=align)[2]
        rmap = acq.region_score_map(pred, unc, r, C, exclude=excl, flip=st == "margin_sampling")
        cand, _ = acq.topk_select(rmap.reshape(N_IMG, H * W), POOL, True)
    else:
        cand, _, _ = acq.score_topk_lowres(low, SIZE, excl, st, POOL, crop=SIZE, align_corners=align)
    img = torch.arange(N_IMG, dtype=torch.int32, device=DEV).repeat_interleave(POOL)
    feat = acq.prob_at_lowres(low, SIZE, img, cand.reshape(-1), crop=SIZE, align_corners=align).view(N_IMG, POOL, -1)
    idx, pos, dist, n = acq.diverse_select(cand, feat, K, n_features=C, exclude=excl)
    return idx.cpu().numpy().astype(np.int64), cand.cpu().numpy(), feat.cpu().numpy(), dist.cpu().numpy(), n.cpu().numpy()


def _hold(data, st, model, align=True, r=0):
    """Both routes against the composition, the composition against the oracle, and what the rule promises about the picks."""
    names = data[4]
    excl = _excl(data)
    want, cand, feat, dist, n = _by_hand(data, st, align, r)
    assert cand.shape == (N_IMG, POOL) and POOL == 307 and feat.shape == (N_IMG, POOL, 20)
    o_idx, o_pos, o_dist, o_n = do.select_batch(cand, feat, K, C, excl)
    assert want.tolist() == o_idx.tolist() and dist.tolist() == o_dist.tolist() and n.tolist() == o_n.tolist() == [K] * N_IMG
    kw = dict(diverse_picks=True, query_strategy=st, region_radius=r)
    piped = _round(model, data, True, **kw)
    fused = _round(model, data, False, **kw)
    assert model.calls == {"forward_lowres": 2, "forward": 0}
    for i, nme in enumerate(names):
        assert _picks(piped[0], nme) == sorted(want[i].tolist()) and _picks(fused[0], nme) == sorted(want[i].tolist()), (st, r, i)
        assert len(set(want[i].tolist())) == K and not excl[i].reshape(-1)[want[i]].any()
        radii = dist[i][1:].tolist()
        assert dist[i][0] == -1 and radii == sorted(radii, reverse=True)
    low = torch.cat([l[:1] for l in data[0]], dim=0)
    flat = np.concatenate([np.sort(w_) for w_ in want])
    ent = acq.score_at_lowres(low, SIZE, np.repeat(np.arange(N_IMG), K), flat, "entropy", crop=SIZE, align_corners=align).cpu().numpy()
    for got in (piped, fused):
        assert np.asarray(got[1].list_entropy, dtype=np.float32).tolist() == ent.astype(np.float32).tolist()
    assert piped[1].dict_label_cnt == fused[1].dict_label_cnt and piped[1].list_n_unique_labels == fused[1].list_n_unique_labels
    return want


@pytest.mark.parametrize("r", [0, 1], ids=["pixel", "region"])
@pytest.mark.parametrize("st", STRATEGIES)
def test_round_gives_the_composition_called_by_hand(data, st, r):
    want = _hold(data, st, _Stub(data[0], SIZE), r=r)
    if r == 0:       # the rule is not the random sub-sample: a plain top-5 % round under the fixed seed picks other pixels
        plain = _round(_Stub(data[0], SIZE), data, True, query_strategy=st)
        assert any(_picks(plain[0], nme) != sorted(w_.tolist()) for nme, w_ in zip(data[4], want))
    else:
        assert want.tolist() != _by_hand(data, st)[0].tolist()      # the region ranking is another pool


@pytest.mark.parametrize("r", [0, 1], ids=["pixel", "region"])
@pytest.mark.parametrize("st", STRATEGIES)
def test_fpn_geometry(data_fpn, st, r):
    """x2, align_corners=False: the selector hands the model's own geometry to the scorer and to the features."""
    want = _hold(data_fpn, st, _StubFPN(data_fpn[0], SIZE), align=False, r=r)
    if st == "entropy" and r == 0:
        assert want.tolist() != _by_hand(data_fpn, st, align=True)[0].tolist()


@pytest.mark.parametrize("pipeline", [True, False], ids=["pipelined", "fused"])
def test_the_option_is_inert_when_off(data, pipeline):
    """Off, None and absent: the picks, the statistics and numpy's stream of a selector that never heard of the option."""
    lows, _, _, _, names = data
    for kw in (dict(), dict(top_n_percent=0.0), dict(region_radius=1), dict(class_balanced=True)):
        ref = _round(_Stub(lows, SIZE), data, pipeline, **kw)
        ref_next = np.random.rand()
        for off in (dict(diverse_picks=False), dict(diverse_picks=None)):
            got = _round(_Stub(lows, SIZE), data, pipeline, **kw, **off)
            assert np.random.rand() == ref_next
            for nme in names:
                assert _picks(got[0], nme) == _picks(ref[0], nme) and len(_picks(ref[0], nme)) == K
            assert got[1].list_entropy == ref[1].list_entropy and got[1].list_spatial_coverage == ref[1].list_spatial_coverage
            assert got[1].dict_label_cnt == ref[1].dict_label_cnt and got[1].list_n_unique_labels == ref[1].list_n_unique_labels


def test_switched_on_numpy_stream_is_left_alone(data):
    _round(_Stub(data[0], SIZE), data, True, diverse_picks=True)        # seeds numpy with 4, then runs the round
    after = np.random.rand()
    np.random.seed(4)
    assert np.random.rand() == after


@pytest.mark.parametrize("pipeline", [True, False], ids=["pipelined", "fused"])
def test_a_pool_smaller_than_the_picks_is_refused_at_the_round(data, pipeline):
    with pytest.raises(ValueError, match="diverse_picks.*n_pixels_by_us = 400"):
        _round(_Stub(data[0], SIZE), data, pipeline, diverse_picks=True, n_pixels_by_us=400)


@pytest.mark.parametrize("with_lowres,fused_on", [(False, True), (True, False)])
def test_the_full_size_route_is_refused(data, with_lowres, fused_on):
    model = _Stub(data[0], SIZE, with_lowres=with_lowres)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ppq, "FUSED_LOWRES", fused_on)
        with pytest.raises(ValueError, match="diverse_picks"):
            _round(model, data, True, diverse_picks=True)
    assert model.calls == {"forward_lowres": 0, "forward": 0}
