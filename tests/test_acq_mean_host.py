"""CPU-only: the mean-probability / BALD oracle (tests/mean_oracle.py) against hand values, the two new symbols in the header, both
builds and the binding, argument validation of pp_acq_mean_prob_score_map / pp_acq_lowres_mc_mean_topk on the PRODUCT library (a
process of its own on libpixelpick_hip.so, no launch: every call below is refused before anything is enqueued, the pointers are never
read), and the errors the Python layer raises without a GPU."""
import json
import math
import os
import re
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

import mean_oracle as mo
from pixelpick_amd import _lib
from pixelpick_amd import acquisition as acq
from pixelpick_amd import query as ppq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pp_acq_mean_prob_score_map", "pp_acq_lowres_mc_mean_topk")


# ---------------------------------------------------------------- the oracle, by hand
def _pixels():
    """T = 4, C = 3, three pixels in a row.  A: every pass confident, the passes split 2 : 2 between two classes.  B: unanimous and
    flat.  D: unanimous and confident (deterministic)."""
    x = np.full((4, 3, 1, 3), -40.0)
    x[:2, 0, 0, 0] = 40.0
    x[2:, 2, 0, 0] = 40.0
    x[:, :, 0, 1] = 0.0
    x[:, 1, 0, 2] = 40.0
    return x


def test_oracle_hand_values():
    x = _pixels()
    ln2, ln3 = math.log(2.0), math.log(3.0)
    ent = mo.score_map(x, None, "entropy")[0]
    assert abs(ent[0] - ln2) < 1e-12 and abs(ent[1] - ln3) < 1e-12 and abs(ent[2]) < 1e-12
    bald = mo.score_map(x, None, "bald")[0]
    assert abs(bald[0] - ln2) < 1e-12           # A: all of its entropy is disagreement between the passes
    assert abs(bald[1]) < 1e-12                 # B: ambiguous, but every pass says the same
    assert abs(bald[2]) < 1e-12                 # D: deterministic
    lc = mo.score_map(x, None, "least_confidence")[0]
    assert abs(lc[0] - 0.5) < 1e-12 and abs(lc[1] - 2.0 / 3.0) < 1e-12 and abs(lc[2]) < 1e-12
    mg = mo.score_map(x, None, "margin_sampling")[0]
    assert abs(mg[0]) < 1e-12 and abs(mg[1]) < 1e-12 and abs(mg[2] - 1.0) < 1e-12
    assert np.allclose(mo.mean_entropy(x)[0], [0.0, ln3, 0.0], atol=1e-12)


def test_oracle_fills_and_picks():
    x = _pixels()
    ex = np.array([[False, True, False]])
    assert [float(mo.score_map(x, ex, s)[0, 1]) for s in ("entropy", "least_confidence", "bald", "margin_sampling")] == [-1.0, -1.0, -1.0, 2.0]
    assert acq.MEAN_FILL == {"entropy": -1.0, "least_confidence": -1.0, "margin_sampling": 2.0, "margin": 2.0, "bald": -1.0}
    # the fill sorts strictly behind the 0.0 of a deterministic pixel; ties -> lower flat index; NaN first for largest
    assert mo.picks(mo.score_map(x, ex, "bald"), 3, "bald").tolist() == [0, 2, 1]
    assert mo.picks(np.array([0.0, np.nan, 0.5, 0.0, -1.0]), 5, "bald").tolist() == [1, 2, 0, 3, 4]
    assert mo.picks(np.array([1.0, 2.0, 0.25, 0.25]), 4, "margin_sampling").tolist() == [2, 3, 0, 1]
    # T = 1: the mean is the pass, no mutual information
    assert np.abs(mo.score_map(np.random.RandomState(0).randn(1, 5, 4, 4), None, "bald")).max() < 1e-12


# ---------------------------------------------------------------- declared, exported, bound
def test_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "pixelpick_hip.h")).read()
    assert re.search(r"enum\s*\{\s*PP_ACQ_BALD\s*=\s*3\s*\}", hdr)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES and _lib._is_launch(name)
        res, args = _lib.SIGNATURES[name]
        assert res is _lib._int and set(args) <= {_lib._int, _lib._i64, _lib._sz, _lib._f, _lib._p}
    assert len(_lib.SIGNATURES[NEW[0]][1]) == 14 and len(_lib.SIGNATURES[NEW[1]][1]) == 22
    assert _lib.SIGNATURES[NEW[1]] == _lib.SIGNATURES["pp_acq_lowres_mc_score_topk"]
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(_lib.KNOBS_LIB_PATH)):
        from pixelpick_amd import build
        build.build(verbose=False)
    for path in (_lib.LIB_PATH, _lib.KNOBS_LIB_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for name in NEW:
            assert re.search(r"\bT %s$" % name, syms, re.M), (path, name)
    assert "bald" not in acq.STRATEGY_ID and acq.MEAN_STRATEGY_ID["bald"] == 3
    assert {k: v for k, v in acq.MEAN_STRATEGY_ID.items() if k != "bald"} == acq.STRATEGY_ID


# ---------------------------------------------------------------- the C ABI without a GPU
_DRIVER = r"""
import json, sys
sys.path.insert(0, %r)
from pixelpick_amd import _lib
L = _lib.lib()
assert not _lib.knobs_build() and L._name.endswith('libpixelpick_hip.so')
P, Q = 0x10000, 0x10001          # a 256-B aligned and a misaligned address (never dereferenced)
B, T, C, h, w, H, W, k = 2, 3, 19, 16, 24, 64, 96, 20
need = L.pp_acq_lowres_workspace_bytes(B, C, H, W, k)
need_large = L.pp_acq_lowres_workspace_bytes(B, C, H, W, 307)
assert need > 0 and need_large > 0

def topk(low=P, ldx=C, B=B, T=T, C=C, Hc=H, Wc=W, k=k, out_idx=P, ws=P, ws_bytes=need, strategy=0, entry="pp_acq_lowres_mc_mean_topk"):
    rc = getattr(L, entry)(low, ldx, B, T, C, h, w, H, W, 1, Hc, Wc, None, strategy, 0.25, k, out_idx, None, None, ws, ws_bytes, None)
    return [rc, L.pp_last_error().decode()]

def smap(prob=P, B=B, C=C, H=H, W=W, mean_ent=None, strategy=0, out=P):
    rc = L.pp_acq_mean_prob_score_map(prob, B, C, H, W, C * H * W, H * W, W, 1, mean_ent, None, strategy, out, None)
    return [rc, L.pp_last_error().decode()]

res = {
    "topk:all zero": [L.pp_acq_lowres_mc_mean_topk(*([None] + [0] * 11 + [None, 0, 0.0, 0, None, None, None, None, 0, None])), L.pp_last_error().decode()],
    "topk:null low": topk(low=None), "topk:null out_idx": topk(out_idx=None), "topk:null workspace": topk(ws=None),
    "topk:T=0": topk(T=0), "topk:C=65": topk(C=65, ldx=65), "topk:C=65 bald": topk(C=65, ldx=65, strategy=3), "topk:C=0": topk(C=0, ldx=19),
    "topk:ldx<C": topk(ldx=18), "topk:crop>size": topk(Hc=H + 1), "topk:k>HcWc": topk(k=H * W + 1),
    "topk:workspace 1 B short": topk(ws_bytes=need - 1), "topk:large-k workspace 1 B short": topk(k=307, ws_bytes=need_large - 1),
    "topk:misaligned workspace": topk(ws=Q), "topk:strategy 4": topk(strategy=4), "topk:strategy -1": topk(strategy=-1),
    "topk:reference-order flag": topk(strategy=0x100), "topk:reference-order flag on bald": topk(strategy=0x103),
    "topk:k=0 without map": topk(k=0), "topk:k=0 without map, bald": topk(k=0, strategy=3),
    "map:all zero": [L.pp_acq_mean_prob_score_map(*([None] + [0] * 8 + [None, None, 0, None, None])), L.pp_last_error().decode()],
    "map:null prob": smap(prob=None), "map:null out_map": smap(out=None), "map:C=0": smap(C=0), "map:B=0": smap(B=0),
    "map:strategy 4": smap(strategy=4), "map:bald without mean_ent": smap(strategy=3),
    "map:entropy with mean_ent": smap(strategy=0, mean_ent=P), "map:margin with mean_ent": smap(strategy=2, mean_ent=P),
    "map:reference-order flag": smap(strategy=0x100), "map:reference-order flag on bald": smap(strategy=0x103, mean_ent=P),
    "map:B=65536": smap(B=65536, H=4, W=4),
    "old:mc_score_topk strategy 3": topk(strategy=3, entry="pp_acq_lowres_mc_score_topk"),
}
print("RESULT " + json.dumps(res))
"""

CODES = {"topk:C=65": -4, "topk:C=65 bald": -4, "topk:k>HcWc": -2, "topk:workspace 1 B short": -3, "topk:large-k workspace 1 B short": -3,
         "topk:null workspace": -3, "map:B=65536": -4}
CASES = ["topk:all zero", "topk:null low", "topk:null out_idx", "topk:null workspace", "topk:T=0", "topk:C=65", "topk:C=65 bald", "topk:C=0",
         "topk:ldx<C", "topk:crop>size", "topk:k>HcWc", "topk:workspace 1 B short", "topk:large-k workspace 1 B short",
         "topk:misaligned workspace", "topk:strategy 4", "topk:strategy -1", "topk:reference-order flag",
         "topk:reference-order flag on bald", "topk:k=0 without map", "topk:k=0 without map, bald", "map:all zero", "map:null prob",
         "map:null out_map", "map:C=0", "map:B=0", "map:strategy 4", "map:bald without mean_ent", "map:entropy with mean_ent",
         "map:margin with mean_ent", "map:reference-order flag", "map:reference-order flag on bald", "map:B=65536",
         "old:mc_score_topk strategy 3"]


@pytest.fixture(scope="module")
def results():
    if not os.path.exists(_lib.LIB_PATH):
        from pixelpick_amd import build
        build.build(verbose=False)
    env = dict(os.environ, PIXELPICK_KNOBS_BUILD="0")
    out = subprocess.run([sys.executable, "-c", _DRIVER % ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


@pytest.mark.parametrize("case", CASES)
def test_bad_arguments_are_refused_with_a_message(results, case):
    rc, msg = results[case]
    assert rc < 0 and msg, (case, rc, msg)
    assert rc == CODES.get(case, -1), (case, rc, msg)          # PP_ERR_BAD_ARG unless listed


def test_every_case_ran(results):
    assert set(results) == set(CASES)


# ---------------------------------------------------------------- the Python layer without a GPU
def test_wrappers_raise_without_a_gpu():
    low = torch.zeros(6, 4, 4, 19)
    with pytest.raises(ValueError, match="multiple of n_passes"):
        acq.mc_mean_topk_lowres(low, 4, (16, 16), None, "bald", 5)
    with pytest.raises(ValueError, match="no mean-probability scorer"):
        acq.mc_mean_topk_lowres(low, 3, (16, 16), None, "random", 5)
    with pytest.raises(_lib.PixelPickHipError, match="no CPU fallback"):
        acq.mc_mean_topk_lowres(low, 3, (16, 16), None, "bald", 5)
    prob = torch.zeros(1, 19, 4, 4)
    with pytest.raises(_lib.PixelPickHipError, match="no CPU fallback"):
        acq.mean_prob_score_map(prob, None, None, "entropy")
    with pytest.raises(ValueError, match="no mean-probability scorer"):
        acq.mean_prob_score_map(prob, None, None, "random")
    # the existing wrappers keep refusing "bald": the strategy table they look it up in is closed
    with pytest.raises(ValueError, match="no score kernel"):
        acq.strategy_id("bald")
    assert acq.mean_strategy_id("bald") == 3 and acq.MEAN_LARGEST["bald"] and not acq.MEAN_LARGEST["margin_sampling"]


class _DL:
    class dataset:
        queries = []


def _args(**kw):
    base = dict(dataset_name="cs", debug=False, dir_root="/tmp", experim_name="m", ignore_index=19, mc_n_steps=4, n_classes=19,
                n_pixels_by_us=5, network_name="deeplab", query_strategy="bald", reverse_order=False, stride_total=8,
                top_n_percent=0.0, use_mc_dropout=True, vote_type="soft")
    base.update(kw)
    return Namespace(**base)


def test_selector_refuses_bald_without_passes_or_with_the_hard_vote():
    with pytest.raises(ValueError, match="use_mc_dropout"):
        ppq.QuerySelector(_args(use_mc_dropout=False), _DL(), device=torch.device("cpu"))
    with pytest.raises(ValueError, match="hard"):
        ppq.QuerySelector(_args(vote_type="hard"), _DL(), device=torch.device("cpu"))
    qs = ppq.QuerySelector(_args(), _DL(), device=torch.device("cpu"))            # bald over soft / consensus passes: accepted
    assert qs._largest and "bald" in ppq._LARGEST_STRATEGIES
    assert ppq.QuerySelector(_args(vote_type="consensus"), _DL(), device=torch.device("cpu"))._largest

    class _M:
        def eval(self): return self
        def turn_on_dropout(self): pass
        def forward_lowres(self, x): raise AssertionError("refused before any forward")

    qs.use_mc_dropout = False                     # changed after construction: the round itself refuses
    with pytest.raises(ValueError, match="use_mc_dropout"):
        qs(nth_query=1, model=_M())


def test_uncertainty_sampler_has_no_bald_of_a_single_prob():
    with pytest.raises(ValueError, match="single prob"):
        ppq.UncertaintySampler("bald")(torch.zeros(1, 19, 4, 4))
