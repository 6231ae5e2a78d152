"""CPU-only: the hard-vote oracle (tests/vote_oracle.py) against hand values, argument validation of pp_acq_vote_accumulate /
pp_acq_vote_score_map / pp_acq_lowres_mc_vote_topk on the PRODUCT library (a process of its own on libpixelpick_hip.so, no launch: every
call below is refused before anything is enqueued, the pointers are never read), and the errors the Python wrappers raise without a GPU."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import vote_oracle as vo
from pixelpick_amd import _lib
from pixelpick_amd import acquisition as acq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _counts_logits(per_pass_class, C):
    """One pixel: logits [T,C,1,1] whose pass t has its maximum at per_pass_class[t]."""
    T = len(per_pass_class)
    x = np.zeros((T, C, 1, 1), dtype=np.float32)
    for t, c in enumerate(per_pass_class):
        x[t, c] = 1.0
    return x


def test_oracle_hand_values_T4():
    x = _counts_logits([0, 2, 0, 1], 3)                       # counts (2, 1, 1)
    assert vo.vote_counts(x).reshape(-1).tolist() == [2, 1, 1]
    ent = float(vo.score_map(x, None, "entropy")[0, 0])
    assert abs(ent - 1.0397208) < 1e-6 and abs(ent - (0.5 * math.log(2) + 0.5 * math.log(4))) < 1e-6
    assert float(vo.score_map(x, None, "least_confidence")[0, 0]) == 0.5
    assert float(vo.score_map(x, None, "margin_sampling")[0, 0]) == 0.25
    u = _counts_logits([1, 1, 1, 1], 3)                       # unanimous
    assert [float(vo.score_map(u, None, s)[0, 0]) for s in ("entropy", "least_confidence", "margin_sampling")] == [0.0, 0.0, 1.0]
    ex = np.ones((1, 1), dtype=bool)                          # excluded
    assert [float(vo.score_map(x, ex, s)[0, 0]) for s in ("entropy", "least_confidence", "margin_sampling")] == [-1.0, -1.0, 2.0]


def test_oracle_ties_table_and_picks():
    x = np.zeros((3, 5, 1, 1), dtype=np.float32)              # exactly equal logits: the lowest class index takes every vote
    assert vo.vote_counts(x).reshape(-1).tolist() == [3, 0, 0, 0, 0]
    for T in (1, 5, 20, 255):
        tab = vo.table(T)
        assert tab[0] == 0 and tab[T] == 0 and tab.dtype == np.uint32
        for n in range(1, T):
            assert tab[n] == int(round(-(n / T) * math.log(n / T) * 2.0 ** 24))
        assert int(tab.astype(np.int64).max()) * 64 < 2 ** 29
    # the entropy is a function of the multiset of counts
    a = vo.score_from_counts(np.array([[3], [0], [2]]), 5, "entropy")
    b = vo.score_from_counts(np.array([[2], [3], [0]]), 5, "entropy")
    assert a.tobytes() == b.tobytes() and a.dtype == np.float32
    m = np.array([[0.5, 0.0, 0.5], [-1.0, 0.5, 0.0]], dtype=np.float32)
    assert vo.picks(m, 6, "entropy").tolist() == [0, 2, 4, 1, 5, 3]       # ties -> lower flat index, the fill last
    m2 = np.array([[1.0, 0.25, 2.0], [0.25, 1.0, 0.0]], dtype=np.float32)
    assert vo.picks(m2, 6, "margin_sampling").tolist() == [5, 1, 3, 0, 4, 2]


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

def topk(low=P, ldx=C, B=B, T=T, C=C, Hc=H, Wc=W, k=k, out_idx=P, ws=P, ws_bytes=need, strategy=0):
    rc = L.pp_acq_lowres_mc_vote_topk(low, ldx, B, T, C, h, w, H, W, 1, Hc, Wc, None, strategy, k, out_idx, None, None, ws, ws_bytes, None)
    return [rc, L.pp_last_error().decode()]

def accum(logits=P, T=T, C=C, H=H, W=W, votes=P):
    rc = L.pp_acq_vote_accumulate(logits, T, C, H, W, C * H * W, H * W, W, 1, votes, 0, None)
    return [rc, L.pp_last_error().decode()]

def score(votes=P, B=B, T=T, C=C, H=H, W=W, strategy=0, out=P):
    rc = L.pp_acq_vote_score_map(votes, B, T, C, H, W, None, strategy, out, None)
    return [rc, L.pp_last_error().decode()]

res = {
    "topk:null low": topk(low=None), "topk:null out_idx": topk(out_idx=None), "topk:null workspace": topk(ws=None),
    "topk:T=0": topk(T=0), "topk:T=256": topk(T=256), "topk:C=65": topk(C=65, ldx=65), "topk:C=0": topk(C=0, ldx=19),
    "topk:ldx<C": topk(ldx=18), "topk:crop>size": topk(Hc=H + 1), "topk:k>HcWc": topk(k=H * W + 1),
    "topk:workspace 1 B short": topk(ws_bytes=need - 1), "topk:large-k workspace 1 B short": topk(k=307, ws_bytes=need_large - 1),
    "topk:misaligned workspace": topk(ws=Q), "topk:strategy 3": topk(strategy=3), "topk:reference-order flag": topk(strategy=0x100),
    "topk:k=0 without map": topk(k=0),
    "accum:null logits": accum(logits=None), "accum:null votes": accum(votes=None), "accum:T=0": accum(T=0), "accum:T=256": accum(T=256),
    "accum:C=0": accum(C=0),
    "score:null votes": score(votes=None), "score:null out_map": score(out=None), "score:T=0": score(T=0), "score:T=256": score(T=256),
    "score:strategy 3": score(strategy=3), "score:C=0": score(C=0),
}
print("RESULT " + json.dumps(res))
"""

CODES = {"topk:T=0": -4, "topk:T=256": -4, "topk:C=65": -4, "topk:k>HcWc": -2, "topk:workspace 1 B short": -3,
         "topk:large-k workspace 1 B short": -3, "topk:null workspace": -3, "accum:T=0": -4, "accum:T=256": -4, "score:T=0": -4,
         "score:T=256": -4}
CASES = ["topk:null low", "topk:null out_idx", "topk:null workspace", "topk:T=0", "topk:T=256", "topk:C=65", "topk:C=0", "topk:ldx<C",
         "topk:crop>size", "topk:k>HcWc", "topk:workspace 1 B short", "topk:large-k workspace 1 B short", "topk:misaligned workspace",
         "topk:strategy 3", "topk:reference-order flag", "topk:k=0 without map", "accum:null logits", "accum:null votes", "accum:T=0",
         "accum:T=256", "accum:C=0", "score:null votes", "score:null out_map", "score:T=0", "score:T=256", "score:strategy 3", "score:C=0"]


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
    if case.endswith(("T=0", "T=256")):
        assert "255" in msg, msg                               # the message names the limit


def test_every_case_ran(results):
    assert set(results) == set(CASES)


def test_wrappers_raise_without_a_gpu():
    low = torch.zeros(6, 4, 4, 19)
    with pytest.raises(ValueError, match="multiple of n_passes"):
        acq.mc_vote_topk_lowres(low, 4, (16, 16), None, "entropy", 5)
    for bad in (0, 256):
        with pytest.raises(ValueError, match="255"):
            acq.mc_vote_topk_lowres(torch.zeros(max(bad, 1), 4, 4, 19), bad, (16, 16), None, "entropy", 5)
        with pytest.raises(ValueError, match="255"):
            acq.vote_score_map(torch.zeros(1, 19, 4, 4, dtype=torch.uint8), bad, None, "entropy")
    with pytest.raises(_lib.PixelPickHipError, match="no CPU fallback"):
        acq.mc_vote_topk_lowres(low, 3, (16, 16), None, "entropy", 5)
    with pytest.raises(_lib.PixelPickHipError, match="no CPU fallback"):
        acq.mc_vote_accumulate_(torch.zeros(3, 19, 4, 4), torch.zeros(19, 4, 4, dtype=torch.uint8))
    with pytest.raises(_lib.PixelPickHipError, match="no CPU fallback"):
        acq.vote_score_map(torch.zeros(1, 19, 4, 4, dtype=torch.uint8), 3, None, "entropy")
    assert acq.MC_VOTE_MAX_PASSES == 255


def test_selector_refuses_more_passes_than_a_byte_counts():
    """vote_type='hard' with mc_n_steps = 256: a ValueError, never a silent soft vote."""
    from argparse import Namespace
    from pixelpick_amd import query as ppq

    class _M:
        def eval(self): return self
        def turn_on_dropout(self): pass
        def forward_lowres(self, x): raise AssertionError("refused before any forward")

    class _DL:
        class dataset:
            queries = []
    a = Namespace(dataset_name="cs", debug=False, dir_root="/tmp", experim_name="v", ignore_index=19, mc_n_steps=256, n_classes=19,
                  n_pixels_by_us=5, network_name="deeplab", query_strategy="entropy", reverse_order=False, stride_total=8,
                  top_n_percent=0.0, use_mc_dropout=True, vote_type="hard")
    with pytest.raises(ValueError, match="255"):
        ppq.QuerySelector(a, _DL(), device=torch.device("cpu"))(nth_query=1, model=_M())
