"""The top-5 % acquisition route (query.py:36,57-64 as QuerySelector calls it: a score strategy, k = 5 % of the pixels, no caller's
map) against the ORACLE'S OWN PICKS on the same logits - never against a device map, so an error shared by the device's scorers and
selects cannot hide.  For the default scorer that call selects from candidate lists (acq_sample_thr_kernel -> acq_kernel<..., EMIT> ->
topk_lsel_kernel), and an image the sample misled is redone inside topk_lsel_kernel; pp_debug_set_lsel_probe says per image which of
the two happened, so that every case here knows what it tested.

The builders and checkers are tests/acq_top5_cases.py (tested on the CPU in tests/test_oracle_golden.py).  The tolerance is the
suite's score tolerance (tests/test_acq_gpu.py): tol(s) = ATOL + RTOL |s|.

Which calls take the list route is the dispatcher's rule (csrc/acq.hip, acq_emit_ok), restated in `takes_list_route` and held to the
probe in every case: the default scorer only (the reference-order scorer always writes the map), flat NCHW planes, H W >= 16384,
8 k <= H W, and k + max(k / 8, 256) <= 8192 candidates in the select's LDS - so 11 x 360 x 480 (k = 8640) and 19 x 1024 x 2048
(k = 104857) go through the score map and the probe stays unwritten there; their picks are held to the oracle all the same."""
import contextlib
import os
import pickle
import tempfile

import numpy as np
import pytest
import torch

import acq_top5_cases as tc
from oracle import acq as orc
from pixelpick_amd import _lib
from pixelpick_amd import acquisition as acq
from pixelpick_amd import query as ppq
from test_acq_gpu import _DL, _DS, _OneConv, _args

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STRATS = list(tc.STRATS)
NOT_RUN = -1                     # what the probe buffer holds where topk_lsel_kernel did not run
AIM_HIGH, AIM_LOW = 1 << 12, 63 << 12      # the sample aims at k / 16 (every image is redone) / at 3.9 k passing pixels


def takes_list_route(C, H, W, k, reference_order=False, flat=True):
    return (not reference_order and flat and C in (11, 19, 21) and H * W >= 16384 and (H * W) % 4 == 0 and 8 * k <= H * W
            and k + max(k // 8, 256) <= 8192)


@contextlib.contextmanager
def lsel_probe(B):
    """with lsel_probe(B) as read: ... read() -> the per-image route of the calls since the previous read() ([B] ints)."""
    L = _lib.lib()
    buf = torch.full((B,), NOT_RUN, dtype=torch.int32, device=DEV)

    def read():
        torch.cuda.synchronize()
        out = buf.cpu().numpy().tolist()
        buf.fill_(NOT_RUN)
        return out
    L.pp_debug_set_lsel_probe(buf.data_ptr())
    try:
        yield read
    finally:
        torch.cuda.synchronize()
        L.pp_debug_set_lsel_probe(None)
        L.pp_debug_set_reduce_mode(0)
        L.pp_debug_set_exact_formula(0)


def _assert_exact(idx, val, o_idx, o_val, what):
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    for b in range(idx.shape[0]):
        bad = tc.exact_rank_violations(idx[b], val[b], o_idx[b], o_val[b])
        assert not bad, (what, f"image {b}", bad)


# ---------------------------------------------------------------------------------------------- (a) graded cases: every rank exact
GRADED = [(19, 256, 512, 6553, 8), (19, 256, 512, 6553, 3), (21, 320, 320, 5120, 2), (11, 360, 480, 8640, 2)]


@pytest.mark.parametrize("ro", [False, True], ids=["default-scorer", "reference-order-scorer"])
@pytest.mark.parametrize("st", STRATS)
@pytest.mark.parametrize("C,H,W,k,B", GRADED, ids=[f"{c}x{h}x{w}-k{k}-B{b}" for c, h, w, k, b in GRADED])
def test_graded_picks_equal_the_oracles_at_every_rank(C, H, W, k, B, st, ro):
    """k + 6 planted pixels 6 tol apart, every possible rival made confident (guard >= 4 tol asserted on the oracle's map by the
    builder): idx must be the oracle's at EVERY rank, val within tol.  Images of a batch have their own seeds; B = 8 is the 8-pixel
    tile at 256 x 512, B = 3 the 4-pixel tile.  The probe must say that the lists were used (0 for every image) wherever the
    dispatcher's rule sends the call there, and stay unwritten elsewhere.  Then the same input with the sample's aim forced far too
    high - every image redone in the kernel (probe 1 or 2) - and far too low (probe 0): the same picks."""
    logits, excl, o_idx, o_val = tc.graded_case(C, H, W, st, k, B)
    lg, ex = torch.from_numpy(logits).to(DEV), torch.from_numpy(excl)
    lists = takes_list_route(C, H, W, k, ro)
    L = _lib.lib()
    with lsel_probe(B) as read:
        idx, val, _ = acq.score_topk(lg, ex, st, k, reference_order=ro)
        route = read()
        assert route == [0 if lists else NOT_RUN] * B, (st, route)
        _assert_exact(idx, val, o_idx, o_val, (st, "default aim", route))
        if lists:
            for mode, want in ((AIM_HIGH, (1, 2)), (AIM_LOW, (0,))):
                L.pp_debug_set_reduce_mode(mode)
                idx, val, _ = acq.score_topk(lg, ex, st, k)
                route = read()
                assert all(r in want for r in route), (st, hex(mode), route)
                print(f"graded {C}x{H}x{W} B{B} {st} aim {hex(mode)}: probe {route}")
                _assert_exact(idx, val, o_idx, o_val, (st, hex(mode), route))


# ---------------------------------------------------------------------------------------------- (b) natural data: rank-tolerant
def _natural(name, st):
    """-> (logits [B,C,H,W] torch CPU tensor (its memory format matters), excl [B,H,W] u8 | None, k, flat)"""
    C = 19
    if name in ("iid", "iid-channels-last", "ragged", "mostly-excluded", "nan"):
        rng = np.random.RandomState(3)
        logits = torch.from_numpy((rng.randn(8, C, 256, 512) * 3).astype(np.float32))
        excl = (rng.rand(8, 256, 512) < 0.05).astype(np.uint8)
        if name == "iid":
            return logits, excl, 6553, True
        if name == "iid-channels-last":
            return logits.contiguous(memory_format=torch.channels_last), excl, 6553, False
        if name == "ragged":
            return logits[:2, :, :100, :172].contiguous(), np.ascontiguousarray(excl[:2, :100, :172]), 860, True
        if name == "mostly-excluded":                          # image 0 constant (all ties), 78 % of image 1 excluded: one huge bin
            lg = torch.zeros((2, C, 128, 256))
            lg[1] = logits[0, :, :128, :256]
            ex = np.zeros((2, 128, 256), np.uint8)
            ex[1, :100] = 1
            return lg, ex, 1638, True
        nanl = logits[:2, :, :128, :128].clone()               # p -> 0 for the others: 0 * log 0 = NaN (query.py:230)
        nanl[0, 0, 3, 5:40] = 200.0
        return nanl.contiguous(), None, 819, True
    if name == "smooth":                                       # spatially correlated scores mislead the sample
        rng = np.random.RandomState(5)
        lo = torch.from_numpy((rng.randn(2, C, 16, 32) * 4).astype(np.float32))
        return torch.nn.functional.interpolate(lo, size=(256, 512), mode="bilinear").contiguous(), None, 6553, True
    Cx, H, W, k, B, seed = {"C21-320x320": (21, 320, 320, 5120, 2, 4), "C11-128x160": (11, 128, 160, 1024, 2, 6),
                            "C19-1024x2048": (19, 1024, 2048, 104857, 1, 8)}[name]
    rng = np.random.RandomState(seed)
    return (torch.from_numpy((rng.randn(B, Cx, H, W) * 3).astype(np.float32)), (rng.rand(B, H, W) < 0.05).astype(np.uint8), k, True)


NATURAL = ([(n, st) for n in ("iid", "smooth", "ragged", "C21-320x320", "C11-128x160", "mostly-excluded", "iid-channels-last")
            for st in STRATS] + [("nan", "entropy"), ("C19-1024x2048", "least_confidence")])


@pytest.mark.parametrize("name,st", NATURAL, ids=[f"{n}-{s}" for n, s in NATURAL])
def test_natural_picks_hold_the_rank_tolerant_rules(name, st):
    """Data nobody shaped: rules 1-5 of acq_top5_cases.rank_tolerant_violations against the oracle's map of the same logits - what a
    scorer within tol of the oracle cannot violate.  The share of ranks that rule 5 pins exactly and the probe's reading are part of
    every message; on iid data the lists must have been used."""
    logits, excl, k, flat = _natural(name, st)
    B, C, H, W = logits.shape
    largest = tc.largest_of(st)
    np_logits = logits.numpy()
    _, _, o_map = orc.score_topk(np_logits, excl, st, k, want_map=True)
    with lsel_probe(B) as read:
        idx, val, _ = acq.score_topk(logits.to(DEV), torch.from_numpy(excl) if excl is not None else None, st, k)
        route = read()
    lists = takes_list_route(C, H, W, k, False, flat)
    assert all((r in (0, 1, 2)) if lists else (r == NOT_RUN) for r in route), (name, st, route)
    if name == "iid":
        assert route == [0] * B, (name, st, route)
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    for b in range(B):
        om = orc.apply_exclude(o_map[b], excl[b], st) if excl is not None else o_map[b]
        bad, info = tc.rank_tolerant_violations(idx[b], val[b], om, excl[b] if excl is not None else None, k, largest)
        assert not bad, (name, st, f"image {b}", f"probe {route}", info, bad)
        print(f"{name} {st} image {b}: probe {route[b]} {info}")


# ---------------------------------------------------------------------------------------------- the reference's default call
@pytest.fixture(scope="module")
def g5(golden_dir):
    return np.load(os.path.join(golden_dir, "acq_top5_default.npz"))


@pytest.mark.parametrize("st", STRATS)
def test_top5_default_fixture_order_from_the_lists(g5, st):
    """tests/golden/acq_top5_default.npz: score_topk without a map reproduces the REFERENCE's value-sorted 5 % order (its own
    uc_map.topk, query.py:57-61) at every rank, from the lists (probe 0) - two images at once and one at a time."""
    logits, _, _, excl, _, k = tc.rebuild_top5_default(g5, st)
    want = g5[f"{st}_order"]
    assert takes_list_route(19, 128, 128, k)
    with lsel_probe(2) as read:
        idx, _, _ = acq.score_topk(torch.from_numpy(logits).to(DEV), torch.from_numpy(excl), st, k)
        assert read() == [0, 0]
        for i in range(2):
            assert idx[i].cpu().numpy().tolist() == want[i].tolist(), (st, i)
            one, _, _ = acq.score_topk(torch.from_numpy(logits[i:i + 1]).to(DEV), torch.from_numpy(excl[i:i + 1]), st, k)
            assert read()[0] == 0
            assert one[0].cpu().numpy().tolist() == want[i].tolist(), (st, i)


@pytest.mark.parametrize("bs", [1, 2])
@pytest.mark.parametrize("st", STRATS)
def test_query_selector_default_call_matches_reference(g5, st, bs):
    """QuerySelector.__call__ with the reference's defaults (top_n_percent = 0.05, n_pixels_by_us = 10) and the stored numpy seed:
    the drawn coordinates and the query statistics are the reference's.  The images are the logits (identity 1x1 classifier)."""
    logits, prev, ys, _, names, k = tc.rebuild_top5_default(g5, st)
    C = logits.shape[1]
    model = _OneConv(torch.eye(C, device=DEV).reshape(C, C, 1, 1), torch.zeros(C, device=DEV))
    x0 = torch.from_numpy(logits[:1]).to(DEV)
    assert torch.equal(model(x0)["pred"], x0), "the identity 1x1 convolution must hand the logits on bit for bit"
    ds = _DS(torch.from_numpy(logits), torch.from_numpy(ys), prev, names)
    with tempfile.TemporaryDirectory() as td, lsel_probe(bs) as read:
        qs = ppq.QuerySelector(_args(query_strategy=st, dir_root=td, top_n_percent=0.05, n_pixels_by_us=10, query_batch_size=bs),
                               _DL(ds), device=torch.device(DEV))
        np.random.seed(int(g5["np_seed"]))
        dq = qs(nth_query=1, model=model)
        route = read()
        stats = pickle.load(open(f"{td}/checkpoints/golden/1_query/query_stats.pkl", "rb"))
    assert route == [0] * bs, route                      # (the last batch's images: the selector took the list route)
    assert list(dq.keys()) == names
    for i, n in enumerate(names):
        assert dq[n]["height"] == 128 and dq[n]["width"] == 128
        np.testing.assert_array_equal(dq[n]["x_coords"], g5[f"{st}_x_{i}"])
        np.testing.assert_array_equal(dq[n]["y_coords"], g5[f"{st}_y_coords_{i}"])
    np.testing.assert_array_equal(np.array([stats["label_distribution"][l] for l in range(19)]), g5[f"{st}_stats_label_cnt"])
    assert abs(stats["avg_entropy"] - float(g5[f"{st}_stats_avg_entropy"])) < 1e-5
    assert abs(stats["avg_n_unique_labels"] - float(g5[f"{st}_stats_avg_n_unique"])) < 1e-9
    assert abs(stats["avg_spatial_coverage"] - float(g5[f"{st}_stats_avg_cov"])) < 1e-9
    assert ds.labelled is not None and ds.labelled[1] == 1
