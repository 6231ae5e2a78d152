"""CPU-only tests of the class-balanced selection: the oracle (tests/balance_oracle.py) on the header's worked cases and against the
properties the specification promises, argument validation of pp_class_balance_select on the PRODUCT library (a process of its own on
libpixelpick_hip.so, no launch: every call is refused before anything is enqueued, the pointers are never read), and what QuerySelector
refuses to combine with `class_balanced` - and leaves alone without it."""
import json
import os
import subprocess
import sys
from argparse import Namespace
from collections import Counter

import numpy as np
import pytest
import torch

import balance_oracle as bo
from pixelpick_amd import _lib
from pixelpick_amd import acquisition as acq
from pixelpick_amd import query as ppq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the oracle
def _along(labels):
    """Labels written along the list: candidate i is pixel i, so list position and pixel index coincide."""
    lab = np.asarray([ord(c) for c in labels.split()], dtype=np.uint8)
    return np.arange(len(lab)), lab


def test_worked_cases_of_the_header():
    cand, lab = _along("a a a b a c b a a c")
    idx, pos, n = bo.select(cand, lab, 6)
    assert (pos.tolist(), n) == ([0, 3, 5, 1, 6, 9], 6) and idx.tolist() == pos.tolist()
    ex = np.zeros(10, dtype=np.uint8)
    ex[0] = 1
    idx, pos, n = bo.select(cand, lab, 6, ex)
    assert (pos.tolist(), n) == ([1, 3, 5, 2, 6, 9], 6)
    cand, lab = _along("a a b a")
    ex = np.asarray([0, 1, 0, 1], dtype=np.uint8)
    idx, pos, n = bo.select(cand, lab, 4, ex)
    assert (pos.tolist(), n) == ([0, 2, 1, 3], 2)


def test_list_positions_are_not_pixel_indices():
    # a shuffled list with a repeated pixel and two candidates outside [0, N): idx is cand at pos, nothing is de-duplicated
    lab = np.asarray([7, 7, 9, 255, 0, 9, 1, 1], dtype=np.uint8)
    cand = [5, 5, -1, 2, 3, 8, 0, 4]                 # classes 9 9 . 9 255 . 7 0
    idx, pos, n = bo.select(cand, lab, 8)
    assert (pos.tolist(), n) == ([0, 4, 6, 7, 1, 3, 2, 5], 6)
    assert idx.tolist() == [5, 3, 0, 4, 5, 2, -1, 8]


def _random_case(rng):
    N = rng.randint(1, 400)
    M = rng.randint(1, N + 1)
    k = rng.randint(1, M + 1)
    n_cls = rng.randint(1, 8)
    classes = rng.choice(256, n_cls, replace=False)
    weights = rng.dirichlet(np.full(n_cls, 0.4))
    lab = classes[rng.choice(n_cls, N, p=weights)].astype(np.uint8)
    cand = rng.choice(N, M, replace=False).astype(np.int64)
    if rng.rand() < 0.3:                             # some candidates outside [0, N)
        bad = rng.rand(M) < 0.1
        cand[bad] = rng.choice([-1, -5, N, N + 3], bad.sum())
    ex = (rng.rand(N) < rng.choice([0.0, 0.1, 0.9])).astype(np.uint8) if rng.rand() < 0.7 else None
    return cand, lab, k, ex, N


def test_properties_on_random_lists():
    rng = np.random.RandomState(0)
    fills = 0
    for _ in range(600):
        cand, lab, k, ex, N = _random_case(rng)
        idx, pos, n = bo.select(cand, lab, k, ex)
        elig = [i for i, c in enumerate(cand) if 0 <= c < N and (ex is None or ex[c] == 0)]
        cls = {i: int(lab[cand[i]]) for i in elig}
        assert n == min(k, len(elig)) and len(set(pos.tolist())) == k and idx.tolist() == [int(cand[i]) for i in pos]
        picked = pos[:n].tolist()
        assert set(picked) <= set(elig)
        per_class = {c: [i for i in elig if cls[i] == c] for c in set(cls.values())}
        got = Counter(cls[i] for i in picked)
        for c, members in per_class.items():         # every class's picks are a prefix of its own ranking
            assert sorted(i for i in picked if cls[i] == c) == members[:got[c]]
        for a in per_class:                          # counts differ by at most one unless the smaller class is exhausted
            for b in per_class:
                if got[a] < got[b] - 1:
                    assert got[a] == len(per_class[a])
        assert len(got) == min(n, len(per_class))    # distinct classes among the picks
        # the order: (rank inside the class, list position) ascends
        keys = [(per_class[cls[i]].index(i), i) for i in picked]
        assert keys == sorted(keys)
        # the fill: the earliest ineligible positions, in list order
        inel = [i for i in range(len(cand)) if i not in cls]
        assert pos[n:].tolist() == inel[:k - n]
        fills += n < k
    assert fills > 20


def test_one_class_gives_the_first_k_eligible_and_k_equal_to_E_a_permutation():
    rng = np.random.RandomState(1)
    for _ in range(50):
        N = rng.randint(4, 200)
        cand = rng.permutation(N)[:rng.randint(2, N + 1)]
        ex = (rng.rand(N) < 0.3).astype(np.uint8)
        elig = [i for i, c in enumerate(cand) if ex[c] == 0]
        if not elig:
            continue
        k = rng.randint(1, len(elig) + 1)
        _, pos, n = bo.select(cand, np.full(N, 200, dtype=np.uint8), k, ex)
        assert pos.tolist() == elig[:k] and n == k
        lab = rng.randint(0, 5, N).astype(np.uint8)
        _, pos, n = bo.select(cand, lab, len(elig), ex)
        assert n == len(elig) and sorted(pos.tolist()) == elig


# ---------------------------------------------------------------- the entry's refusals
_DRIVER = r"""
import json, sys
sys.path.insert(0, %r)
from pixelpick_amd import _lib
L = _lib.lib()
assert not _lib.knobs_build() and L._name.endswith('libpixelpick_hip.so')
P = 0x10000          # an address that is never dereferenced: every call below is refused before anything is enqueued

def call(cand=P, B=2, M=307, N=64 * 96, k=6, label=P, out_idx=P, out_pos=P, out_n=P):
    rc = L.pp_class_balance_select(cand, B, M, N, k, label, None, out_idx, out_pos, out_n, None)
    return [rc, L.pp_last_error().decode()]

res = {
    "null cand": call(cand=None), "null label": call(label=None), "null out_idx": call(out_idx=None), "null out_pos": call(out_pos=None),
    "null out_n": call(out_n=None), "B=0": call(B=0), "M=0": call(M=0, k=1), "N=0": call(N=0), "k=0": call(k=0), "k>M": call(k=308),
    "M>N": call(M=64 * 96 + 1), "N=2^31": call(N=2 ** 31), "k past the cap": call(k=1025, M=2000), "B=2^31": call(B=2 ** 31),
    "all zero": [L.pp_class_balance_select(None, 0, 0, 0, 0, None, None, None, None, None, None), L.pp_last_error().decode()],
}
print("RESULT " + json.dumps(res))
"""

# case -> (code, the argument its message names)
CASES = {"null cand": (-1, "cand"), "null label": (-1, "label"), "null out_idx": (-1, "out_idx"), "null out_pos": (-1, "out_pos"),
         "null out_n": (-1, "out_n"), "B=0": (-1, "B="), "M=0": (-1, "M="), "N=0": (-1, "N="), "k=0": (-1, "k="), "k>M": (-1, "k="),
         "M>N": (-1, "M="), "N=2^31": (-1, "N="), "k past the cap": (-4, "k="), "B=2^31": (-4, "B="), "all zero": (-1, "")}


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
    assert rc == code and "class_balance_select" in msg and names in msg, (case, rc, msg)
    if case == "k past the cap":
        assert str(acq.BALANCE_MAX_PICKS) in msg and acq.BALANCE_MAX_PICKS == acq.SPREAD_MAX_PICKS == 1024


def test_every_case_ran(results):
    assert set(results) == set(CASES)


def test_entry_is_a_recordable_launch():
    assert "pp_class_balance_select" in _lib.SIGNATURES and _lib._is_launch("pp_class_balance_select")
    res, args = _lib.SIGNATURES["pp_class_balance_select"]
    assert len(args) == 11
    hdr = open(os.path.join(ROOT, "include", "pixelpick_hip.h")).read()
    assert "int pp_class_balance_select(const int32_t* cand, int64_t B, int64_t M, int64_t N, int64_t k," in hdr
    assert "PP_PLAN_ENTRY(pp_class_balance_select)" in open(os.path.join(ROOT, "pixelpick_amd", "csrc", "plan.hip")).read()


def test_wrapper_raises_without_a_gpu():
    lab = torch.zeros(1, 16, dtype=torch.uint8)
    with pytest.raises(_lib.PixelPickHipError, match="no CPU fallback"):
        acq.class_balance_select(torch.zeros(1, 8, dtype=torch.int32), lab, 2)
    with pytest.raises(ValueError, match="int32"):
        acq.class_balance_select(torch.zeros(1, 8, dtype=torch.int64), lab, 2)
    with pytest.raises(ValueError, match="2-d"):
        acq.class_balance_select(torch.zeros(8, dtype=torch.int32), lab, 2)


# ---------------------------------------------------------------- the selector's option
class _M:
    def eval(self): return self
    def turn_on_dropout(self): pass
    def forward_lowres(self, x): raise AssertionError("refused before any forward")


class _NoLowres:
    def eval(self): return self
    def turn_on_dropout(self): pass
    def __call__(self, x): raise AssertionError("refused before any forward")


class _DL:
    class dataset:
        queries = []


def _args(**kw):
    base = dict(dataset_name="cs", debug=False, dir_root="/tmp", experim_name="b", ignore_index=19, mc_n_steps=4, n_classes=19,
                n_pixels_by_us=6, network_name="deeplab", query_strategy="entropy", reverse_order=False, stride_total=8,
                top_n_percent=0.05, use_mc_dropout=False, vote_type="soft")
    base.update(kw)
    return Namespace(**base)


REFUSED = [(dict(top_n_percent=0.0), "top_n_percent"), (dict(top_n_percent=-1.0), "top_n_percent"), (dict(reverse_order=True), "reverse_order"),
           (dict(query_strategy="random"), "random"), (dict(query_strategy="bald"), "bald"),
           (dict(query_strategy="bald", use_mc_dropout=True), "bald"), (dict(use_mc_dropout=True), "use_mc_dropout"),
           (dict(min_pixel_distance=2), "min_pixel_distance"), (dict(min_pixel_distance=8, top_n_percent=0.0), "class_balanced"),
           (dict(n_pixels_by_us=1025), "n_pixels_by_us"), (dict(n_classes=257), "n_classes")]


@pytest.mark.parametrize("kw,names", REFUSED)
def test_selector_refuses_what_the_rule_cannot_serve(kw, names):
    with pytest.raises(ValueError, match="class_balanced") as e:
        ppq.QuerySelector(_args(class_balanced=True, **kw), _DL(), device=torch.device("cpu"))
    assert names in str(e.value)
    # and again at the round, for a selector whose attributes were changed after construction
    qs = ppq.QuerySelector(_args(class_balanced=True), _DL(), device=torch.device("cpu"))
    for key, v in kw.items():
        setattr(qs, key, v)
    with pytest.raises(ValueError, match="class_balanced") as e:
        qs(nth_query=1, model=_M())
    assert names in str(e.value)


def test_selector_refuses_the_full_size_route_at_the_round(monkeypatch):
    qs = ppq.QuerySelector(_args(class_balanced=True), _DL(), device=torch.device("cpu"))
    with pytest.raises(ValueError, match="class_balanced.*forward_lowres"):
        qs(nth_query=1, model=_NoLowres())
    monkeypatch.setattr(ppq, "FUSED_LOWRES", False)
    with pytest.raises(ValueError, match="class_balanced.*FUSED_LOWRES"):
        qs(nth_query=1, model=_M())


def test_switched_on_after_construction_is_checked_at_the_round():
    qs = ppq.QuerySelector(_args(top_n_percent=0.0), _DL(), device=torch.device("cpu"))
    qs.class_balanced = True
    with pytest.raises(ValueError, match="class_balanced.*top_n_percent"):
        qs(nth_query=1, model=_M())


def test_off_or_absent_nothing_changes():
    """_k_launch and _draw are what they are without the attribute: "pos" is drawn and numpy's stream advances by the same amount."""
    for mode in (dict(top_n_percent=0.05), dict(top_n_percent=0.0), dict(reverse_order=True), dict(min_pixel_distance=4, top_n_percent=0.0)):
        ref = ppq.QuerySelector(_args(**mode), _DL(), device=torch.device("cpu"))
        np.random.seed(11)
        ref_draw, ref_next = ref._draw(64, 96), np.random.rand()
        for off in (dict(class_balanced=False), dict(class_balanced=None), dict(class_balanced=0)):
            qs = ppq.QuerySelector(_args(**mode, **off), _DL(), device=torch.device("cpu"))
            assert not qs._balance_on and qs._k_launch(64, 96) == ref._k_launch(64, 96)
            np.random.seed(11)
            d = qs._draw(64, 96)
            assert sorted(d) == sorted(ref_draw) and all((d[key] == ref_draw[key]).all() for key in d)
            assert np.random.rand() == ref_next
    qs = ppq.QuerySelector(_args(), _DL(), device=torch.device("cpu"))
    assert qs._k_launch(64, 96) == 307
    np.random.seed(11)
    d = qs._draw(64, 96)
    assert sorted(d) == ["pos"] and d["pos"].shape == (6,) and d["pos"].max() < 307
    np.random.seed(11)
    assert (d["pos"] == np.random.choice(307, 6, False)).all()


def test_on_the_pool_is_the_references_and_nothing_is_drawn():
    qs = ppq.QuerySelector(_args(class_balanced=True), _DL(), device=torch.device("cpu"))
    assert qs._balance_on and qs._k_launch(64, 96) == 307
    np.random.seed(11)
    want = np.random.rand()
    np.random.seed(11)
    assert "pos" not in qs._draw(64, 96) and qs._draw(64, 96) == {}
    assert np.random.rand() == want                   # numpy's stream was not touched
    # with region_radius it still is the pool of the region ranking
    qs = ppq.QuerySelector(_args(class_balanced=True, region_radius=2), _DL(), device=torch.device("cpu"))
    assert qs._k_launch(64, 96) == 307 and qs._draw(64, 96) == {}
