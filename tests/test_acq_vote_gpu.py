"""GPU tests of the MC-dropout HARD vote (pp_acq_lowres_mc_vote_topk, pp_acq_vote_accumulate, pp_acq_vote_score_map;
acquisition.mc_vote_topk_lowres / mc_vote_accumulate_ / vote_score_map) against tests/vote_oracle.py.

The oracle is fed the DEVICE'S OWN pp_bilinear_fwd output, downloaded: the interpolation is held to float64 elsewhere, and an arg-max
on bit-identical floats is exact - so every comparison in this file is an EQUALITY (no tolerance, no share of exempt pixels):
  1. the fused entry's map, picks and values equal the oracle's,
  2. the fused entry equals pp_bilinear_fwd -> pp_acq_vote_accumulate -> pp_acq_vote_score_map -> pp_topk_select bit for bit, and
     splitting the passes into two accumulate calls changes nothing,
  3. arg-max ties go to the lowest class index (constant logits at T = 255: a full byte lane; a duplicated channel),
  4. the entropy table, read back through the map, for every split n / T - n of T in {5, 20, 255},
  5. k beyond the number of un-excluded pixels: the un-excluded first, then the excluded in index order,
  6. pp_acq_vote_accumulate at C = 150 with NCHW and channels-last strides against np.argmax."""
import functools

import numpy as np
import pytest
import torch

import vote_oracle as vo
from pixelpick_amd import acquisition as acq
from pixelpick_amd import engine as E

pytestmark = pytest.mark.gpu
STRATS = ["entropy", "least_confidence", "margin_sampling"]
DEV = "cuda:0"

# C, (h, w), (H, W), crop, align_corners, T, B, channel pad (ldx = C + pad): the smallest geometry at which each kernel form and each
# counter layout is reached (the geometries of tests/test_acq_mc_lowres_gpu.py)
CASES = {
    "cs_1.5tiles": (19, (16, 24), (64, 96), None, True, 4, 2, 0),        # C = 19: five counter words, 1 1/2 tiles across
    "voc_crop": (21, (20, 23), (80, 92), (77, 90), True, 3, 1, 0),       # C = 21: six words; padded size, cropped back
    "fpn_x2": (19, (24, 40), (48, 80), None, False, 2, 3, 0),            # x2, align_corners = False
    "c7_slice": (7, (16, 24), (64, 96), None, True, 3, 1, 5),            # generic <= 32 instantiation, a channel slice (ldx = C + 5)
    "c40": (40, (16, 24), (64, 96), None, True, 3, 1, 0),                # generic <= 64 instantiation: ten counter words in use
    "down_8x_memory": (19, (200, 300), (25, 40), None, True, 2, 1, 0),   # the patch exceeds LDS: the form that reads memory
    "cs_8row_tiles": (19, (32, 64), (128, 256), None, True, 2, 32, 0),   # 512 tiles of 32 rows: the 8-rows-per-wave plan
    "T20": (19, (16, 24), (64, 96), None, True, 20, 1, 0),
    "T1": (19, (16, 24), (64, 96), None, True, 1, 1, 0),                 # every un-excluded score identical: the pure tie-break
    "T255_c64": (64, (4, 6), (16, 24), None, True, 255, 1, 0),           # the limits of both T and C
}
KINDS = ["base+noise", "plain"]


def _ks(hc, wc):
    return [9, 48, 49, int(0.05 * hc * wc)]      # both sides of the fused-extraction limit (48) and the top-5 % mode


def _low(rng, kind, B, T, C, h, w, pad):
    if kind == "plain":                          # maximal disagreement between the passes
        x = rng.randn(B * T, h, w, C) * 3
    else:                                        # counts from unanimous to split
        x = np.repeat(rng.randn(B, 1, h, w, C) * 3, T, axis=1).reshape(B * T, h, w, C) + 0.7 * rng.randn(B * T, h, w, C)
    t = torch.from_numpy(x.astype(np.float32)).to(DEV)
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


def _votes(pred, B, T, split=None):
    """pp_acq_vote_accumulate per image -> u8 [B,C,hc,wc]; split: the passes in two calls (overwrite, then accumulate)."""
    C, hc, wc = pred.shape[1:]
    votes = torch.full((B, C, hc, wc), 77, dtype=torch.uint8, device=DEV)         # stale contents: the first call overwrites
    for b in range(B):
        p = pred[b * T:(b + 1) * T]
        if split is None:
            acq.mc_vote_accumulate_(p, votes[b], accumulate=False)
        else:
            acq.mc_vote_accumulate_(p[:split], votes[b], accumulate=False)
            acq.mc_vote_accumulate_(p[split:], votes[b], accumulate=True)
    return votes


@functools.lru_cache(maxsize=None)
def _setup(name, kind):
    """One geometry, one kind of input: the device's interpolated logits (downloaded once), the oracle's vote counts, the chain's votes."""
    C, (h, w), size, crop, align, T, B, pad = CASES[name]
    rng = np.random.RandomState(sum(map(ord, name + kind)))
    low = _low(rng, kind, B, T, C, h, w, pad)
    hc, wc = size if crop is None else crop
    excl = _exclude(rng, B, hc, wc)
    pred = _pred(low, size, crop, align)
    pred_h = pred.cpu().numpy().reshape(B, T, C, hc, wc)
    counts = np.stack([vo.vote_counts(pred_h[b]) for b in range(B)])
    votes = _votes(pred, B, T)
    votes_split = _votes(pred, B, T, split=T // 2) if T >= 2 else votes
    return dict(low=low, excl=excl, counts=counts, votes=votes, votes_split=votes_split, geom=(C, size, crop, align, T, B, hc, wc))


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("kind", KINDS)
def test_accumulated_votes_are_the_oracles_counts(name, kind):
    s = _setup(name, kind)
    T = s["geom"][4]
    got = s["votes"].cpu().numpy()
    assert got.dtype == np.uint8 and np.array_equal(got.astype(np.int64), s["counts"])
    assert (s["counts"].sum(axis=1) == T).all()
    assert torch.equal(s["votes_split"], s["votes"])                    # two accumulate calls == one


@pytest.mark.parametrize("st", STRATS)
@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("kind", KINDS)
def test_fused_entry_equals_the_oracle_and_the_chain(name, kind, st):
    s = _setup(name, kind)
    C, size, crop, align, T, B, hc, wc = s["geom"]
    low, excl = s["low"], s["excl"]
    want = np.stack([np.where(excl[b], np.float32(vo.FILL[st]), vo.score_from_counts(s["counts"][b], T, st)) for b in range(B)])
    assert want.dtype == np.float32
    chain_map = acq.vote_score_map(s["votes"], T, excl, st)
    assert np.array_equal(chain_map.cpu().numpy(), want)
    _, _, m0 = acq.mc_vote_topk_lowres(low, T, size, excl, st, 0, crop=crop, align_corners=align)       # k == 0: the map only
    assert m0.dtype == torch.float32 and np.array_equal(m0.cpu().numpy(), want)
    for k in _ks(hc, wc):
        idx, val, m = acq.mc_vote_topk_lowres(low, T, size, excl, st, k, crop=crop, align_corners=align)
        ci, cv = acq.topk_select(chain_map.reshape(B, hc * wc), k, acq.LARGEST[st])
        assert torch.equal(m, chain_map), k
        assert torch.equal(idx, ci) and torch.equal(val, cv), k
        idx_h, val_h = idx.cpu().numpy(), val.cpu().numpy()
        for b in range(B):
            pk = vo.picks(want[b], k, st)
            assert idx_h[b].tolist() == pk.tolist(), (k, b)
            assert np.array_equal(val_h[b], want[b].reshape(-1)[pk]), (k, b)


def test_T1_is_a_constant_map_and_the_pure_tie_break():
    s = _setup("T1", "plain")
    C, size, crop, align, T, B, hc, wc = s["geom"]
    for st, const in (("entropy", 0.0), ("least_confidence", 0.0), ("margin_sampling", 1.0)):
        idx, val, m = acq.mc_vote_topk_lowres(s["low"], T, size, s["excl"], st, 49)
        m = m.cpu().numpy()
        assert set(np.unique(m[~s["excl"]]).tolist()) == {const} and set(np.unique(m[s["excl"]]).tolist()) == {vo.FILL[st]}
        assert idx[0].tolist() == np.flatnonzero(~s["excl"][0].reshape(-1))[:49].tolist()
        assert (val == const).all()


@pytest.mark.parametrize("st", STRATS)
def test_constant_logits_give_class_0_every_vote_in_a_full_byte_lane(st):
    """T = 255 passes of constant logits: class 0's byte holds 255 and carries nothing into class 1's."""
    C, (h, w), size, T = 64, (4, 6), (16, 24), 255
    low = torch.full((T, h, w, C), 0.25, device=DEV)
    votes = _votes(_pred(low, size, None, True), 1, T)
    assert (votes[0, 0] == 255).all() and (votes[0, 1:] == 0).all()
    _, _, m = acq.mc_vote_topk_lowres(low, T, size, None, st, 0)
    assert (m == (1.0 if st == "margin_sampling" else 0.0)).all()
    assert torch.equal(m, acq.vote_score_map(votes, T, None, st))


@pytest.mark.parametrize("C,lo,hi", [(19, 2, 5), (19, 3, 4), (40, 7, 36), (64, 31, 63)])
def test_duplicated_channel_votes_for_the_lower_copy(C, lo, hi):
    (h, w), size, T = (16, 24), (64, 96), 6
    rng = np.random.RandomState(C + lo)
    x = rng.randn(T, h, w, C).astype(np.float32)
    x[..., lo] = np.abs(x[..., lo]) + 9.0                     # the winner everywhere ...
    x[..., hi] = x[..., lo]                                   # ... and its exact copy at a higher index
    low = torch.from_numpy(x).to(DEV)
    votes = _votes(_pred(low, size, None, True), 1, T)
    assert (votes[0, lo] == T).all() and (votes[0, hi] == 0).all() and int(votes.sum()) == T * size[0] * size[1]
    for st in STRATS:
        _, _, m = acq.mc_vote_topk_lowres(low, T, size, None, st, 0)
        assert (m == (1.0 if st == "margin_sampling" else 0.0)).all()


@pytest.mark.parametrize("T", [5, 20, 255])
def test_entropy_table_read_back_through_the_map(T):
    """Identity geometry (h, w) == (H, W); at pixel p class 3 wins the first n = p mod (T + 1) passes and class 11 the others:
    the map is float32(tab[n] + tab[T - n]) * 2^-24 for every n in 0 .. T, and the other strategies follow the counts."""
    C, (h, w) = 19, (16, 16)
    n = (np.arange(h * w) % (T + 1)).reshape(h, w)
    assert set(n.reshape(-1).tolist()) == set(range(T + 1))
    x = np.full((T, h, w, C), -1.0, dtype=np.float32)
    x[..., 11] = 0.5
    x[..., 3] = np.where(np.arange(T)[:, None, None] < n[None], 1.0, 0.0)
    low = torch.from_numpy(x).to(DEV)
    tab = vo.table(T).astype(np.int64)
    want = (tab[n] + tab[T - n]).astype(np.float32) * np.float32(2.0 ** -24)
    _, _, m = acq.mc_vote_topk_lowres(low, T, (h, w), None, "entropy", 0)
    assert np.array_equal(m[0].cpu().numpy(), want)
    votes = _votes(_pred(low, (h, w), None, True), 1, T)
    assert np.array_equal(votes[0, 3].cpu().numpy(), n) and np.array_equal(votes[0, 11].cpu().numpy(), T - n)
    assert np.array_equal(acq.vote_score_map(votes, T, None, "entropy")[0].cpu().numpy(), want)
    hi, lo_ = np.maximum(n, T - n), np.minimum(n, T - n)
    _, _, lc = acq.mc_vote_topk_lowres(low, T, (h, w), None, "least_confidence", 0)
    _, _, mg = acq.mc_vote_topk_lowres(low, T, (h, w), None, "margin_sampling", 0)
    assert np.array_equal(lc[0].cpu().numpy(), (T - hi).astype(np.float32) / np.float32(T))
    assert np.array_equal(mg[0].cpu().numpy(), (hi - lo_).astype(np.float32) / np.float32(T))


@pytest.mark.parametrize("st", STRATS)
@pytest.mark.parametrize("k", [9, 49])
def test_fewer_free_pixels_than_k(st, k):
    """The un-excluded pixels come first (in the oracle's order), then the excluded ones, lowest index first."""
    C, (h, w), size, T, B = 19, (16, 24), (64, 96), 4, 2
    rng = np.random.RandomState(21)
    low = _low(rng, "plain", B, T, C, h, w, 0)
    excl = np.ones((B,) + size, dtype=bool)
    excl.reshape(B, -1)[:, rng.choice(size[0] * size[1], 5, replace=False)] = False
    pred_h = _pred(low, size, None, True).cpu().numpy().reshape(B, T, C, *size)
    idx, val, m = acq.mc_vote_topk_lowres(low, T, size, excl, st, k)
    for b in range(B):
        want = vo.score_map(pred_h[b], excl[b], st)
        assert np.array_equal(m[b].cpu().numpy(), want)
        free = np.flatnonzero(~excl[b].reshape(-1))
        got = idx[b].tolist()
        assert got == vo.picks(want, k, st).tolist()
        assert set(got[:5]) == set(free.tolist())
        assert got[5:] == np.flatnonzero(excl[b].reshape(-1))[:k - 5].tolist()
        assert (val[b, 5:] == vo.FILL[st]).all() and (val[b, :5] != vo.FILL[st]).all()


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
def test_vote_accumulate_streams_any_class_count(layout):
    T, C, H, W = 5, 150, 13, 37
    rng = np.random.RandomState(150)
    x = (rng.randn(T, C, H, W) * 2).astype(np.float32)
    x[:, 149] = x[:, 17]                                       # an exact tie far apart: the lower index takes it
    t = torch.from_numpy(x).to(DEV)
    if layout == "channels_last":
        t = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert t.stride(1) == 1
    votes = torch.full((C, H, W), 200, dtype=torch.uint8, device=DEV)
    acq.mc_vote_accumulate_(t[:2], votes, accumulate=False)
    acq.mc_vote_accumulate_(t[2:], votes, accumulate=True)
    want = vo.vote_counts(x)
    assert np.array_equal(votes.cpu().numpy().astype(np.int64), want) and (votes[149] == 0).all()
    for st in STRATS:
        assert np.array_equal(acq.vote_score_map(votes, T, None, st)[0].cpu().numpy(), vo.score_from_counts(want, T, st))


def test_wrapper_errors():
    low = torch.randn(6, 8, 8, 19, device=DEV)
    with pytest.raises(ValueError):                      # 6 entries are not a multiple of 4 passes
        acq.mc_vote_topk_lowres(low, 4, (32, 32), None, "entropy", 5)
    with pytest.raises(ValueError):                      # k > crop_h * crop_w
        acq.mc_vote_topk_lowres(low, 3, (4, 4), None, "entropy", 17)
    with pytest.raises(ValueError, match="255"):         # more passes than a byte counts: never a silent soft vote
        acq.mc_vote_topk_lowres(torch.randn(256, 2, 2, 19, device=DEV), 256, (8, 8), None, "entropy", 5)
    with pytest.raises(Exception):                       # heads wider than 64 classes: PP_ERR_UNSUPPORTED
        acq.mc_vote_topk_lowres(torch.randn(2, 4, 4, 65, device=DEV), 2, (16, 16), None, "entropy", 5)
    with pytest.raises(ValueError):                      # votes of the wrong shape
        acq.mc_vote_accumulate_(torch.randn(2, 19, 4, 4, device=DEV), torch.zeros(19, 4, 5, dtype=torch.uint8, device=DEV))
