"""CPU-only tests of the feature-diverse selection: the oracle (tests/diverse_oracle.py) against the properties the specification promises,
argument validation of pp_diverse_select / pp_acq_lowres_prob_at_u8 on the PRODUCT library (a process of its own on libpixelpick_hip.so,
no launch: every call is refused before anything is enqueued, the pointers are never read), the workspace and resident-form queries, and
what QuerySelector refuses to combine with `diverse_picks` - and leaves alone without it."""
import json
import os
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

import diverse_oracle as do
from pixelpick_amd import _lib
from pixelpick_amd import acquisition as acq
from pixelpick_amd import query as ppq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the oracle
def test_worked_cases():
    # one feature: values along the list; pick 0 is position 0, then the farthest, ties to the earliest position
    feat = np.asarray([[10], [12], [200], [10], [105], [200]], dtype=np.uint8)
    idx, pos, dist, n = do.select(np.arange(6), feat, 6)
    assert pos.tolist() == [0, 2, 4, 1, 3, 5] and n == 6
    assert dist.tolist() == [-1, 190 ** 2, 95 ** 2, 2 ** 2, 0, 0] and idx.tolist() == pos.tolist()
    # position 0 excluded, positions 2 and 5 ineligible (outside [0, N)): they are never centres, and fill the end in list order
    cand = [0, 1, -3, 3, 4, 6]
    ex = np.asarray([1, 0, 0, 0, 0, 0], dtype=np.uint8)
    idx, pos, dist, n = do.select(cand, feat, 6, exclude=ex)
    assert (pos.tolist(), n) == ([1, 4, 3, 0, 2, 5], 3) and dist.tolist() == [-1, 93 ** 2, 2 ** 2, -1, -1, -1]
    assert idx.tolist() == [1, 4, 3, 0, -3, 6]


def _random_case(rng):
    N = rng.randint(1, 300)
    M = rng.randint(1, N + 1)
    k = rng.randint(1, M + 1)
    F = rng.randint(1, 9)
    ldf = (F + 3) // 4 * 4 + 4 * rng.randint(0, 2)
    levels = rng.choice([2, 4, 256])                 # few levels: exact ties and zero distances
    feat = (rng.randint(0, levels, (M, ldf)) * (255 // (levels - 1))).astype(np.uint8)
    cand = rng.choice(N, M, replace=False).astype(np.int64)
    if rng.rand() < 0.3:
        bad = rng.rand(M) < 0.1
        cand[bad] = rng.choice([-1, -5, N, N + 3], bad.sum())
    ex = (rng.rand(N) < rng.choice([0.0, 0.1, 0.9])).astype(np.uint8) if rng.rand() < 0.7 else None
    return cand, feat, k, F, ex, N


def test_properties_on_random_lists():
    rng = np.random.RandomState(0)
    fills = 0
    for _ in range(400):
        cand, feat, k, F, ex, N = _random_case(rng)
        idx, pos, dist, n = do.select(cand, feat, k, F, ex, N)
        elig = [i for i, c in enumerate(cand) if 0 <= c < N and (ex is None or ex[c] == 0)]
        assert n == min(k, len(elig)) and len(set(pos.tolist())) == k and idx.tolist() == [int(cand[i]) for i in pos]
        picked = pos[:n].tolist()
        assert set(picked) <= set(elig)              # every pick of the greedy phase is eligible
        if n:
            assert picked[0] == elig[0] and dist[0] == -1
        radii = dist[1:n].tolist()
        assert radii == sorted(radii, reverse=True) and all(r >= 0 for r in radii)     # the k-centre radius sequence
        f = feat[:, :F].astype(np.int64)
        for t in range(1, n):                        # each pick is the farthest of what was left, ties to the smallest position
            d = np.min([((f - f[c]) ** 2).sum(axis=1) for c in picked[:t]], axis=0)
            left = [i for i in elig if i not in picked[:t]]
            assert dist[t] == d[picked[t]] == max(d[i] for i in left)
            assert picked[t] == min(i for i in left if d[i] == dist[t])
        inel = [i for i in range(len(cand)) if i not in set(elig)]
        assert pos[n:].tolist() == inel[:k - n] and (dist[n:] == -1).all()
        other = feat.copy()                          # no byte past F enters the result
        other[:, F:] = 255 - other[:, F:]
        assert all((a == b).all() for a, b in zip(do.select(cand, other, k, F, ex, N)[:3], (idx, pos, dist)))
        fills += n < k
    assert fills > 20


def test_prob_codes_are_the_rounded_softmax():
    rng = np.random.RandomState(3)
    low = (rng.randn(2, 4, 6, 5) * 3).astype(np.float32)
    img, pix = np.asarray([0, 1, 1]), np.asarray([0, 7, 95])
    q = do.prob_codes(low, (8, 12), img, pix)
    assert q.shape == (3, 5) and q.dtype == np.uint8 and (np.abs(q.astype(int).sum(axis=1) - 255) <= 3).all()
    x = low[0, 0, 0].astype(np.float64)              # pixel 0 is source pixel 0 with align_corners
    p = np.exp(x - x.max()) / np.exp(x - x.max()).sum()
    assert q[0].tolist() == np.rint(255 * p).astype(int).tolist()


# ---------------------------------------------------------------- the entries' refusals
_DRIVER = r"""
import json, sys
sys.path.insert(0, %r)
from pixelpick_amd import _lib
L = _lib.lib()
assert not _lib.knobs_build() and L._name.endswith('libpixelpick_hip.so')
P = 0x10000          # an address that is never dereferenced: every call below is refused before anything is enqueued

def sel(cand=P, B=2, M=307, N=64 * 96, k=6, feat=P, F=19, ldf=20, out_idx=P, out_pos=P, out_dist=P, out_n=P, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = max(L.pp_diverse_workspace_bytes(B, M, F), 4 * max(B, 0) * max(M, 0))
    rc = L.pp_diverse_select(cand, B, M, N, k, feat, F, ldf, None, out_idx, out_pos, out_dist, out_n, ws, ws_bytes, None)
    return [rc, L.pp_last_error().decode()]

def prob(low=P, ldx=19, B=2, C=19, h=16, w=24, H=64, W=96, Hc=64, Wc=96, img=P, pix=P, n=10, out=P, ldf=20):
    rc = L.pp_acq_lowres_prob_at_u8(low, ldx, B, C, h, w, H, W, 1, Hc, Wc, img, pix, n, out, ldf, None)
    return [rc, L.pp_last_error().decode()]

res = {
    "null cand": sel(cand=None), "null feat": sel(feat=None), "null out_idx": sel(out_idx=None), "null out_pos": sel(out_pos=None),
    "null out_dist": sel(out_dist=None), "null out_n": sel(out_n=None), "null workspace": sel(ws=None),
    "B=0": sel(B=0), "M=0": sel(M=0, k=1), "N=0": sel(N=0), "k=0": sel(k=0), "F=0": sel(F=0), "k>M": sel(k=308),
    "M>N": sel(M=64 * 96 + 1), "N=2^31": sel(N=2 ** 31), "F=257": sel(F=257, ldf=260), "ldf<F": sel(ldf=16), "ldf odd": sel(ldf=22),
    "feat misaligned": sel(feat=P + 2), "workspace small": sel(ws_bytes=4 * 2 * 307 - 1),
    "k past the cap": sel(k=1025, M=2000), "B=2^31": sel(B=2 ** 31, ws_bytes=2 ** 62),
    "all zero": [L.pp_diverse_select(None, 0, 0, 0, 0, None, 0, 0, None, None, None, None, None, None, 0, None), L.pp_last_error().decode()],
    "prob: null low": prob(low=None), "prob: ldf<C": prob(ldf=16), "prob: ldf odd": prob(ldf=22), "prob: out misaligned": prob(out=P + 1),
    "prob: C=257": prob(C=257, ldx=257, ldf=260), "prob: null img": prob(img=None), "prob: null pix": prob(pix=None),
    "prob: null out": prob(out=None), "prob: n<0": prob(n=-1), "prob: crop too large": prob(Hc=65),
    "prob: n=0": prob(n=0, img=None, pix=None, out=None),
}
sizes = {"ws": [[B, M, F, L.pp_diverse_workspace_bytes(B, M, F)] for B, M, F in
                ((1, 1, 1), (3, 307, 19), (256, 6553, 19), (2, 70000, 256), (0, 5, 5), (5, 0, 5), (5, 5, 0), (5, 5, 257))],
         "res": [[F, L.pp_diverse_resident_candidates(F)] for F in (0, 1, 4, 5, 19, 64, 256, 257)]}
print("RESULT " + json.dumps([res, sizes]))
"""

# case -> (code, the entry its message names, the argument its message names)
CASES = {"null cand": (-1, "cand"), "null feat": (-1, "feat"), "null out_idx": (-1, "out_idx"), "null out_pos": (-1, "out_pos"),
         "null out_dist": (-1, "out_dist"), "null out_n": (-1, "out_n"), "null workspace": (-1, "workspace"), "B=0": (-1, "B="),
         "M=0": (-1, "M="), "N=0": (-1, "N="), "k=0": (-1, "k="), "F=0": (-1, "F="), "k>M": (-1, "k="), "M>N": (-1, "M="),
         "N=2^31": (-1, "N="), "F=257": (-1, "F="), "ldf<F": (-1, "ldf="), "ldf odd": (-1, "ldf="), "feat misaligned": (-1, "aligned"),
         "workspace small": (-1, "workspace"), "k past the cap": (-4, "k="), "B=2^31": (-4, "B="), "all zero": (-1, ""),
         "prob: null low": (-1, "null"), "prob: ldf<C": (-1, "ldf="), "prob: ldf odd": (-1, "ldf="), "prob: out misaligned": (-1, "aligned"),
         "prob: C=257": (-4, "C="), "prob: null img": (-1, "null"), "prob: null pix": (-1, "null"), "prob: null out": (-1, "null"),
         "prob: n<0": (-1, "n < 0"), "prob: crop too large": (-1, "crop"), "prob: n=0": (0, None)}


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
    rc, msg = results[0][case]
    code, names = CASES[case]
    assert rc == code, (case, rc, msg)
    if names is None:
        return
    if case.startswith("prob: "):
        assert names in msg, (case, msg)
    else:
        assert "diverse_select" in msg and names in msg, (case, rc, msg)
    if case == "k past the cap":
        assert str(acq.DIVERSE_MAX_PICKS) in msg and acq.DIVERSE_MAX_PICKS == acq.BALANCE_MAX_PICKS == acq.SPREAD_MAX_PICKS == 1024
    if case == "F=257":
        assert acq.DIVERSE_MAX_FEATURES == 256


def test_every_case_ran(results):
    assert set(results[0]) == set(CASES)


def test_workspace_and_resident_queries(results):
    for B, M, F, ws in results[1]["ws"]:
        ok = B >= 1 and M >= 1 and 1 <= F <= 256
        assert (ws >= 4 * B * M and ws < 4 * B * M + 4096) if ok else ws == 0, (B, M, F, ws)
    res = dict(results[1]["res"])
    assert res[0] == res[257] == 0
    if res[19] > 0:                                  # a resident form is shipped: whole rows and r in the 160 KiB of one CU
        for F in (1, 4, 5, 19, 64, 256):
            dw = (F + 3) // 4
            assert res[F] >= 1 and res[F] * 4 * dw <= 160 * 1024 < (res[F] + 1) * 4 * (dw + 1) + 2048
        assert res[1] == res[4] >= res[5] >= res[19] >= 6553 > res[64] >= res[256]
    else:
        assert all(v == 0 for v in res.values())


def test_entries_are_declared_exported_bound_and_recordable():
    hdr = open(os.path.join(ROOT, "include", "pixelpick_hip.h")).read()
    plan = open(os.path.join(ROOT, "pixelpick_amd", "csrc", "plan.hip")).read()
    assert "int pp_acq_lowres_prob_at_u8(const float* low, int64_t ldx, int64_t B, int64_t C, int64_t h, int64_t w," in hdr
    assert "int pp_diverse_select(const int32_t* cand, int64_t B, int64_t M, int64_t N, int64_t k," in hdr
    assert "size_t pp_diverse_workspace_bytes(int64_t B, int64_t M, int64_t F);" in hdr
    assert "int64_t pp_diverse_resident_candidates(int64_t F);" in hdr
    arity = {"pp_acq_lowres_prob_at_u8": 17, "pp_diverse_select": 16, "pp_diverse_workspace_bytes": 3, "pp_diverse_resident_candidates": 1}
    for name, n_args in arity.items():
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args
        launch = name in ("pp_acq_lowres_prob_at_u8", "pp_diverse_select")
        assert _lib._is_launch(name) == launch and (f"PP_PLAN_ENTRY({name})" in plan) == launch
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(_lib.KNOBS_LIB_PATH)):
        from pixelpick_amd import build
        build.build(verbose=False)
    for path in (_lib.LIB_PATH, _lib.KNOBS_LIB_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert all(f" T {name}\n" in syms for name in arity), path


def test_wrappers_raise_without_a_gpu():
    feat = torch.zeros(1, 8, 4, dtype=torch.uint8)
    with pytest.raises(_lib.PixelPickHipError, match="no CPU fallback"):
        acq.diverse_select(torch.zeros(1, 8, dtype=torch.int32), feat, 2)
    with pytest.raises(ValueError, match="int32"):
        acq.diverse_select(torch.zeros(1, 8, dtype=torch.int64), feat, 2)
    with pytest.raises(ValueError, match="2-d"):
        acq.diverse_select(torch.zeros(8, dtype=torch.int32), feat, 2)
    with pytest.raises(_lib.PixelPickHipError, match="no CPU fallback"):
        acq.prob_at_lowres(torch.zeros(1, 4, 4, 19), (8, 8), [0], [0])


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
           (dict(min_pixel_distance=2), "min_pixel_distance"), (dict(n_pixels_by_us=1025), "n_pixels_by_us"),
           (dict(n_classes=257), "n_classes")]


@pytest.mark.parametrize("kw,names", REFUSED)
def test_selector_refuses_what_the_rule_cannot_serve(kw, names):
    with pytest.raises(ValueError, match="diverse_picks") as e:
        ppq.QuerySelector(_args(diverse_picks=True, **kw), _DL(), device=torch.device("cpu"))
    assert names in str(e.value)
    # and again at the round, for a selector whose attributes were changed after construction
    qs = ppq.QuerySelector(_args(diverse_picks=True), _DL(), device=torch.device("cpu"))
    for key, v in kw.items():
        setattr(qs, key, v)
    with pytest.raises(ValueError, match="diverse_picks") as e:
        qs(nth_query=1, model=_M())
    assert names in str(e.value)


def test_selector_refuses_two_selection_rules():
    with pytest.raises(ValueError, match="diverse_picks.*class_balanced"):
        ppq.QuerySelector(_args(diverse_picks=True, class_balanced=True), _DL(), device=torch.device("cpu"))
    qs = ppq.QuerySelector(_args(class_balanced=True), _DL(), device=torch.device("cpu"))
    qs.diverse_picks = True
    with pytest.raises(ValueError, match="diverse_picks.*class_balanced"):
        qs(nth_query=1, model=_M())


def test_selector_refuses_the_full_size_route_at_the_round(monkeypatch):
    qs = ppq.QuerySelector(_args(diverse_picks=True), _DL(), device=torch.device("cpu"))
    with pytest.raises(ValueError, match="diverse_picks.*forward_lowres"):
        qs(nth_query=1, model=_NoLowres())
    monkeypatch.setattr(ppq, "FUSED_LOWRES", False)
    with pytest.raises(ValueError, match="diverse_picks.*FUSED_LOWRES"):
        qs(nth_query=1, model=_M())


def test_switched_on_after_construction_is_checked_at_the_round():
    qs = ppq.QuerySelector(_args(top_n_percent=0.0), _DL(), device=torch.device("cpu"))
    qs.diverse_picks = True
    with pytest.raises(ValueError, match="diverse_picks.*top_n_percent"):
        qs(nth_query=1, model=_M())


def test_off_or_absent_nothing_changes():
    """_k_launch and _draw are what they are without the attribute: "pos" is drawn and numpy's stream advances by the same amount;
    and none of the option's refusals fires for a combination it would refuse."""
    for mode in (dict(top_n_percent=0.05), dict(top_n_percent=0.0), dict(reverse_order=True), dict(min_pixel_distance=4, top_n_percent=0.0),
                 dict(class_balanced=True), dict(query_strategy="random"), dict(use_mc_dropout=True), dict(n_classes=300)):
        ref = ppq.QuerySelector(_args(**mode), _DL(), device=torch.device("cpu"))
        np.random.seed(11)
        torch.manual_seed(11)
        ref_draw, ref_next = ref._draw(64, 96), np.random.rand()
        for off in (dict(diverse_picks=False), dict(diverse_picks=None), dict(diverse_picks=0)):
            qs = ppq.QuerySelector(_args(**mode, **off), _DL(), device=torch.device("cpu"))
            assert not qs._diverse_on and qs._k_launch(64, 96) == ref._k_launch(64, 96)
            np.random.seed(11)
            torch.manual_seed(11)
            d = qs._draw(64, 96)
            assert sorted(d) == sorted(ref_draw) and all((d[key] == ref_draw[key]).all() for key in d)
            assert np.random.rand() == ref_next
    qs = ppq.QuerySelector(_args(), _DL(), device=torch.device("cpu"))
    np.random.seed(11)
    d = qs._draw(64, 96)
    np.random.seed(11)
    assert sorted(d) == ["pos"] and (d["pos"] == np.random.choice(307, 6, False)).all()


def test_on_the_pool_is_the_references_and_nothing_is_drawn():
    qs = ppq.QuerySelector(_args(diverse_picks=True), _DL(), device=torch.device("cpu"))
    assert qs._diverse_on and qs._k_launch(64, 96) == 307
    np.random.seed(11)
    want = np.random.rand()
    np.random.seed(11)
    assert "pos" not in qs._draw(64, 96) and qs._draw(64, 96) == {}
    assert np.random.rand() == want                   # numpy's stream was not touched
    # with region_radius it still is the pool of the region ranking
    qs = ppq.QuerySelector(_args(diverse_picks=True, region_radius=2), _DL(), device=torch.device("cpu"))
    assert qs._k_launch(64, 96) == 307 and qs._draw(64, 96) == {}
