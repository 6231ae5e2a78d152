"""CPU-only tests of the minimum-pixel-distance selection: the reach A(d) and the candidate bound M against the numpy oracle
(tests/spread_oracle.py), argument validation of pp_spread_select on the PRODUCT library (a process of its own on libpixelpick_hip.so,
no launch: every call is refused before anything is enqueued, the pointers are never read), and what QuerySelector refuses to combine
with `min_pixel_distance`."""
import json
import os
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

import spread_oracle as so
from pixelpick_amd import _lib
from pixelpick_amd import acquisition as acq
from pixelpick_amd import query as ppq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reach_is_the_brute_force_count():
    assert [so.reach(d) for d in (1, 2, 8, 16)] == [1, 9, 193, 793]
    for d in range(1, 33):
        assert acq.spread_reach(d) == so.reach(d), d
    with pytest.raises(ValueError):
        acq.spread_reach(0)


def test_candidate_count():
    assert acq.spread_candidates(10, 8, 256 * 512) == 1738 and acq.spread_candidates(10, 16, 256 * 512) == 7138
    assert acq.spread_candidates(10, 1, 1000) == 10            # d = 1 blocks nothing but the pick itself
    assert acq.spread_candidates(1, 30, 1000) == 1
    assert acq.spread_candidates(6, 5, 300) == 300             # never more than the image holds
    for k, d, N in ((1, 1, 1), (6, 5, 64 * 96), (11, 8, 1200), (3, 2, 7)):
        assert acq.spread_candidates(k, d, N) == so.candidates(k, d, N)


def _blob_map(rng, H, W):
    """A smooth map of a few bumps quantised to 8 levels: long runs of exactly equal scores next to each other, all >= 1."""
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W))
    for _ in range(rng.randint(1, 4)):
        cy, cx, s = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(1.5, 6.0)
        m += rng.uniform(0.5, 1.0) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    return (1 + np.floor(7 * m / m.max())).astype(np.float32)


def test_top_m_list_gives_the_greedy_pass_over_the_whole_ranking():
    """Random tie-heavy blob maps, largest-first with the fill 0.0 below every score: the greedy pass over the first M ranks equals the
    greedy pass over all N.  Where the whole ranking hosts k picks, idx and pos are compared in full.  Where it does not, the accepted
    prefix is: pick j of the full pass sits among the first (j-1) A(d) + 1 un-excluded ranks, all of which the top-M list holds (the
    excluded pixels rank last), so both passes accept the same n picks; their fills differ only in how far the list reaches."""
    rng = np.random.RandomState(0)
    cases = short = 0
    for with_excl in (False, True):
        for _ in range(400):
            H, W = rng.randint(5, 31), rng.randint(5, 41)
            d, k = int(rng.choice([1, 2, 3, 5, 8])), rng.randint(1, 12)
            N = H * W
            m = _blob_map(rng, H, W)
            ex = (rng.rand(N) < 0.10) if with_excl else np.zeros(N, dtype=bool)
            if N - ex.sum() < k:
                ex[:] = False
            filled = np.where(ex, np.float32(0.0), m.reshape(-1))
            assert (filled[~ex] > 0.0).all()
            rank = so.ranking(filled, True)
            M = so.candidates(k, d, N)
            f_idx, f_pos, f_n = so.select(rank, W, k, d, ex)
            t_idx, t_pos, t_n = so.select(rank[:M], W, k, d, ex)
            cases += 1
            assert t_n == f_n, (H, W, d, k)
            if f_n == k:
                assert t_idx.tolist() == f_idx.tolist() and t_pos.tolist() == f_pos.tolist(), (H, W, d, k)
            else:
                short += 1
                assert t_idx[:t_n].tolist() == f_idx[:f_n].tolist() and t_pos[:t_n].tolist() == f_pos[:f_n].tolist(), (H, W, d, k)
            # the oracle's own contract on the way
            pk = [divmod(int(c), W) for c in f_idx[:f_n]]
            assert all((a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2 >= d * d for i, a in enumerate(pk) for b in pk[:i])
            assert not ex[f_idx[:f_n]].any() and len(set(f_pos.tolist())) == k
    assert cases >= 400
    assert short < 0.20 * cases, (short, cases)                # images too small to host k picks at distance d


def test_oracle_hand_case():
    # one row of 10 pixels in rank order 0..9, d = 3: 0, 3, 6, 9 are accepted; k = 6 is topped up with positions 1, 2
    idx, pos, n = so.select(np.arange(10), 10, 6, 3)
    assert (idx.tolist(), pos.tolist(), n) == ([0, 3, 6, 9, 1, 2], [0, 3, 6, 9, 1, 2], 4)
    ex = np.zeros(10, dtype=np.uint8)
    ex[0] = 1                                                  # the best candidate is hidden: 1, 4, 7 - and 0 comes back in the fill
    idx, pos, n = so.select(np.arange(10), 10, 5, 3, ex)
    assert (idx.tolist(), n) == ([1, 4, 7, 0, 2], 3)
    idx, pos, n = so.select([5, 3, 9], 10, 2, 1)               # d = 1: the first k
    assert (idx.tolist(), pos.tolist(), n) == ([5, 3], [0, 1], 2)


_DRIVER = r"""
import json, sys
sys.path.insert(0, %r)
from pixelpick_amd import _lib
L = _lib.lib()
assert not _lib.knobs_build() and L._name.endswith('libpixelpick_hip.so')
P = 0x10000          # an address that is never dereferenced: every call below is refused before anything is enqueued

def call(cand=P, B=2, M=300, W=96, N=64 * 96, k=6, d=5, out_idx=P, out_pos=P, out_n=P):
    rc = L.pp_spread_select(cand, B, M, W, N, k, d, None, out_idx, out_pos, out_n, None)
    return [rc, L.pp_last_error().decode()]

res = {
    "null cand": call(cand=None), "null out_idx": call(out_idx=None), "null out_pos": call(out_pos=None), "null out_n": call(out_n=None),
    "k=0": call(k=0), "k>M": call(k=301), "M>N": call(M=64 * 96 + 1), "d=0": call(d=0), "W=0": call(W=0), "N=2^31": call(N=2 ** 31),
    "B=0": call(B=0), "M=0": call(M=0, k=1), "k past the cap": call(k=1025, M=2000),
}
print("RESULT " + json.dumps(res))
"""

# case -> (code, the argument its message names)
CASES = {"null cand": (-1, "cand"), "null out_idx": (-1, "out_idx"), "null out_pos": (-1, "out_pos"), "null out_n": (-1, "out_n"),
         "k=0": (-1, "k="), "k>M": (-1, "k="), "M>N": (-1, "M="), "d=0": (-1, "d="), "W=0": (-1, "W="), "N=2^31": (-1, "N="),
         "B=0": (-1, "B="), "M=0": (-1, "M="), "k past the cap": (-4, "k=")}


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


@pytest.mark.parametrize("case", sorted(CASES))
def test_bad_arguments_are_refused_with_a_message(results, case):
    rc, msg = results[case]
    code, names = CASES[case]
    assert rc == code and "spread_select" in msg and names in msg, (case, rc, msg)
    if case == "k past the cap":
        assert str(acq.SPREAD_MAX_PICKS) in msg


def test_every_case_ran(results):
    assert set(results) == set(CASES)


def test_entry_is_a_recordable_launch():
    assert "pp_spread_select" in _lib.SIGNATURES and _lib._is_launch("pp_spread_select")
    res, args = _lib.SIGNATURES["pp_spread_select"]
    assert len(args) == 12


def test_wrapper_raises_without_a_gpu():
    with pytest.raises(_lib.PixelPickHipError, match="no CPU fallback"):
        acq.spread_select(torch.zeros(1, 8, dtype=torch.int32), 4, 2, 2)
    with pytest.raises(ValueError, match="int32"):
        acq.spread_select(torch.zeros(1, 8, dtype=torch.int64), 4, 2, 2)


# ---------------------------------------------------------------- the selector's option
class _M:
    def eval(self): return self
    def turn_on_dropout(self): pass
    def forward_lowres(self, x): raise AssertionError("refused before any forward")


class _DL:
    class dataset:
        queries = []


def _args(**kw):
    base = dict(dataset_name="cs", debug=False, dir_root="/tmp", experim_name="s", ignore_index=19, mc_n_steps=4, n_classes=19,
                n_pixels_by_us=6, network_name="deeplab", query_strategy="entropy", reverse_order=False, stride_total=8,
                top_n_percent=0.0, use_mc_dropout=False, vote_type="soft")
    base.update(kw)
    return Namespace(**base)


@pytest.mark.parametrize("kw,names", [(dict(top_n_percent=0.05), "top_n_percent = 0"), (dict(reverse_order=True, top_n_percent=0.0), "reverse_order"),
                                      (dict(reverse_order=True, top_n_percent=0.05), "min_pixel_distance"), (dict(query_strategy="random"), "random")])
def test_selector_refuses_what_the_distance_rule_replaces(kw, names):
    with pytest.raises(ValueError, match="min_pixel_distance") as e:
        ppq.QuerySelector(_args(min_pixel_distance=4, **kw), _DL(), device=torch.device("cpu"))
    assert names in str(e.value)
    # and again at the round, for a selector whose attributes were changed after construction
    qs = ppq.QuerySelector(_args(min_pixel_distance=4), _DL(), device=torch.device("cpu"))
    for key, v in kw.items():
        setattr(qs, key, v)
    with pytest.raises(ValueError, match="min_pixel_distance"):
        qs(nth_query=1, model=_M())


def test_selector_constructs_with_the_option_off_or_alone():
    for kw in ({}, dict(min_pixel_distance=0), dict(min_pixel_distance=1), dict(min_pixel_distance=None)):
        for mode in (dict(top_n_percent=0.05), dict(reverse_order=True, top_n_percent=0.05), dict(query_strategy="random")):
            qs = ppq.QuerySelector(_args(**kw, **mode), _DL(), device=torch.device("cpu"))
            assert qs.min_pixel_distance < 2 and not qs._spread_on
            assert qs._k_launch(64, 96) == (6 if mode.get("reverse_order") or not mode.get("top_n_percent") else int(64 * 96 * 0.05))
    qs = ppq.QuerySelector(_args(min_pixel_distance=4), _DL(), device=torch.device("cpu"))
    assert qs._spread_on and qs._k_launch(64, 96) == acq.spread_candidates(6, 4, 64 * 96) == 5 * 45 + 1
    with pytest.raises(ValueError, match="min_pixel_distance"):
        ppq.QuerySelector(_args(min_pixel_distance=-3), _DL(), device=torch.device("cpu"))
