"""CPU-only tests of the region-aware acquisition: the n ln(n) table of pp_acq_region_table against the numpy oracle
(tests/region_oracle.py), every refusal of pp_acq_region_score_map on the PRODUCT library (a process of its own on
libpixelpick_hip.so, no launch: each call is refused before anything is enqueued and no pointer is read), the binding tables, the
wrappers' own argument checks and what QuerySelector refuses to combine with `region_radius`."""
import ctypes
import json
import os
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

import region_oracle as ro
from pixelpick_amd import _lib
from pixelpick_amd import acquisition as acq
from pixelpick_amd import query as ppq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib_table(r):
    L = _lib.lib()
    n = L.pp_acq_region_table_words(r)
    host = np.full(n + 2, 0xDEADBEEF, dtype=np.uint32)            # two guard words behind the table
    assert L.pp_acq_region_table(r, host.ctypes.data) == 0
    assert host[n:].tolist() == [0xDEADBEEF] * 2
    return host[:n]


def test_table_equals_the_oracle_for_every_radius():
    for r in range(1, ro.MAX_RADIUS + 1):
        got = _lib_table(r)
        assert got.shape == ((2 * r + 1) ** 2 + 1,) and got.tolist() == ro.table(r).tolist(), r
    t = ro.table(16)
    assert t[0] == t[1] == 0 and t[2] == round(2 * np.log(2) * 65536) and int(t[1089]) == 499082426 and int(t.max()) < 2 ** 31
    assert (np.diff(t.astype(np.int64))[1:] > 0).all()


def test_table_products_stay_clear_of_a_half():
    """The rounding of n ln(n) 2^16 is safe against the last bits of log(): no product comes near a half-integer."""
    n = np.arange(2, 1090, dtype=np.float64)
    v = n * np.log(n) * 65536.0
    assert np.abs(v - np.floor(v) - 0.5).min() > 1e-4


def test_word_count_and_table_refusals():
    L = _lib.lib()
    assert [L.pp_acq_region_table_words(r) for r in (1, 2, 16)] == [10, 26, 1090]
    assert [L.pp_acq_region_table_words(r) for r in (0, -1, 17, 2 ** 40)] == [0, 0, 0, 0]
    buf = (ctypes.c_uint32 * 4)(7, 7, 7, 7)
    assert L.pp_acq_region_table(3, None) == -1 and b"host_tab" in L.pp_last_error()
    for r in (0, 17, -5):
        assert L.pp_acq_region_table(r, ctypes.addressof(buf)) == -4 and b"r=" in L.pp_last_error()
    assert list(buf) == [7, 7, 7, 7]


def test_oracle_hand_cases():
    # one label: D = 0 everywhere, P exactly 0
    assert (ro.impurity_int(np.full((6, 9), 3, np.uint8), 5, 2) == 0).all()
    # a 3 x 3 image, r = 1, the centre sees 9 pixels: five 0s and four 1s
    pred = np.array([[0, 1, 0], [1, 0, 1], [0, 1, 0]], np.uint8)
    tab = ro.table(1).astype(np.int64)
    D = ro.impurity_int(pred, 2, 1)
    assert D[1, 1] == tab[9] - tab[5] - tab[4] and D[0, 0] == tab[4] - 2 * tab[2]
    assert ro.window_size(3, 3, 1).tolist() == [[4, 6, 4], [6, 9, 6], [4, 6, 4]]
    P = ro.impurity(pred, 2, 1)
    assert P.dtype == np.float32 and abs(float(P[0, 0]) - np.log(2)) < 1e-5
    # a label >= C falls into the one extra bin: 7 and 9 are the same label when C = 2
    a = ro.impurity_int(np.array([[0, 7, 9]], np.uint8), 2, 1)
    b = ro.impurity_int(np.array([[0, 2, 2]], np.uint8), 2, 1)
    assert a.tolist() == b.tolist() and a[0, 2] == 0
    # the window mean, clipped; a NaN stays in its window
    unc = np.arange(12, dtype=np.float32).reshape(3, 4)
    U = ro.uncertainty64(unc, 1)
    assert U[0, 0] == (0 + 1 + 4 + 5) / 4 and U[1, 1] == unc[0:3, 0:3].sum() / 9
    unc[0, 0] = np.nan
    assert np.isnan(ro.uncertainty64(unc, 1)).tolist() == [[True, True, False, False], [True, True, False, False], [False] * 4]
    assert ro.ranking(np.array([[1., 3.], [3., -1.]]), 3).tolist() == [1, 2, 0]


_DRIVER = r"""
import json, sys
sys.path.insert(0, %r)
from pixelpick_amd import _lib
L = _lib.lib()
assert not _lib.knobs_build() and L._name.endswith('libpixelpick_hip.so')
P = 0x10000          # an address that is never dereferenced: every call below is refused before anything is enqueued

def call(pred=P, unc=P, B=2, C=19, H=40, W=70, r=3, mode=0, flip=0, tab=P, exclude=None, out=P):
    rc = L.pp_acq_region_score_map(pred, unc, B, C, H, W, r, mode, flip, tab, exclude, out, None)
    return [rc, L.pp_last_error().decode()]

res = {
    "null pred": call(pred=None), "null unc": call(unc=None), "null tab": call(tab=None), "null out": call(out=None),
    "null pred mode 1": call(pred=None, mode=1), "null tab mode 1": call(tab=None, mode=1), "null unc mode 2": call(unc=None, mode=2),
    "B=0": call(B=0), "H=0": call(H=0), "W=-1": call(W=-1), "C=0": call(C=0), "C=257": call(C=257), "mode=3": call(mode=3),
    "mode=-1": call(mode=-1), "r=0": call(r=0), "r=17": call(r=17), "H*W=2^31": call(H=2 ** 16, W=2 ** 15),
    "grid": call(B=2 ** 31 - 1, H=65, W=64),
}
print("RESULT " + json.dumps(res))
"""

# case -> (code, the argument its message names)
CASES = {"null pred": (-1, "pred"), "null unc": (-1, "unc"), "null tab": (-1, "tab"), "null out": (-1, "out_map"),
         "null pred mode 1": (-1, "pred"), "null tab mode 1": (-1, "tab"), "null unc mode 2": (-1, "unc"),
         "B=0": (-1, "B="), "H=0": (-1, "H="), "W=-1": (-1, "W="), "C=0": (-1, "C="), "C=257": (-1, "C="), "mode=3": (-1, "mode="),
         "mode=-1": (-1, "mode="), "r=0": (-4, "r="), "r=17": (-4, "r="), "H*W=2^31": (-4, "H*W"), "grid": (-4, "grid")}


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
    assert rc == code and "region_score_map" in msg and names in msg, (case, rc, msg)


def test_every_case_ran(results):
    assert set(results) == set(CASES)


def test_entries_are_bound_and_the_launch_is_recordable():
    for name, nargs in (("pp_acq_region_table_words", 1), ("pp_acq_region_table", 2), ("pp_acq_region_score_map", 13)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
    assert _lib._is_launch("pp_acq_region_score_map")
    assert not _lib._is_launch("pp_acq_region_table") and not _lib._is_launch("pp_acq_region_table_words")
    L = _lib.lib()
    for name, want in (("pp_acq_region_score_map", 13), ("pp_acq_region_table", -1), ("pp_acq_region_table_words", -1)):
        fn = getattr(L, name)
        assert L.pp_plan_entry_args(ctypes.cast(getattr(fn, "__wrapped__", fn), ctypes.c_void_p)) == want, name
    hdr = open(os.path.join(ROOT, "include", "pixelpick_hip.h")).read()
    assert "int pp_acq_region_score_map(const uint8_t* pred, const float* unc, int64_t B, int64_t C, int64_t H, int64_t W" in hdr


def test_wrappers_refuse_on_the_host():
    pred, unc = torch.zeros(1, 4, 4, dtype=torch.uint8), torch.zeros(1, 4, 4)
    with pytest.raises(_lib.PixelPickHipError, match="no CPU fallback"):
        acq.region_score_map(pred, unc, 1, 3)
    with pytest.raises(_lib.PixelPickHipError, match="no CPU fallback"):
        acq.region_table(1, "cpu")
    for r in (0, 17, -1):
        with pytest.raises(ValueError, match="radius"):
            acq.region_score_map(pred, unc, r, 3)
        with pytest.raises(ValueError, match="radius"):
            acq.region_table(r, "cuda:0")
    with pytest.raises(ValueError, match="mode"):
        acq.region_score_map(pred, unc, 1, 3, mode="sum")
    for C in (0, 257):
        with pytest.raises(ValueError, match="n_classes"):
            acq.region_score_map(pred, unc, 1, C)
    with pytest.raises(ValueError, match="pred"):
        acq.region_score_map(None, unc, 1, 3)
    with pytest.raises(ValueError, match="unc"):
        acq.region_score_map(pred, None, 1, 3)
    assert acq.REGION_TILE == (64, 64) and acq.REGION_MAX_RADIUS == ro.MAX_RADIUS and acq.REGION_FILL == float(ro.FILL)


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
    base = dict(dataset_name="cs", debug=False, dir_root="/tmp", experim_name="s", ignore_index=19, mc_n_steps=4, n_classes=19,
                n_pixels_by_us=6, network_name="deeplab", query_strategy="entropy", reverse_order=False, stride_total=8,
                top_n_percent=0.0, use_mc_dropout=False, vote_type="soft")
    base.update(kw)
    return Namespace(**base)


REFUSED = [(dict(query_strategy="random"), "random"), (dict(query_strategy="bald", use_mc_dropout=True), "bald"),
           (dict(use_mc_dropout=True), "use_mc_dropout"), (dict(use_mc_dropout=True, vote_type="hard"), "use_mc_dropout"),
           (dict(n_classes=257), "n_classes"), (dict(region_radius=17), "region_radius = 17"), (dict(region_radius=-2), "region_radius = -2"),
           (dict(region_mode="sum"), "region_mode")]


@pytest.mark.parametrize("kw,names", REFUSED)
def test_selector_refuses_what_is_not_region_scored(kw, names):
    with pytest.raises(ValueError, match="region_radius") as e:
        ppq.QuerySelector(_args(**dict(dict(region_radius=4), **kw)), _DL(), device=torch.device("cpu"))
    assert names in str(e.value)
    # and again at the round, for a selector whose attributes were changed after construction
    qs = ppq.QuerySelector(_args(region_radius=4), _DL(), device=torch.device("cpu"))
    for key, v in kw.items():
        setattr(qs, key, v)
    with pytest.raises(ValueError, match="region_radius"):
        qs(nth_query=1, model=_M())


def test_selector_refuses_a_model_without_forward_lowres_at_the_round():
    qs = ppq.QuerySelector(_args(region_radius=2), _DL(), device=torch.device("cpu"))
    with pytest.raises(ValueError, match="forward_lowres"):
        qs(nth_query=1, model=_NoLowres())
    with pytest.MonkeyPatch.context() as mp:                  # the full-size route of a model that has it
        mp.setattr(ppq, "FUSED_LOWRES", False)
        with pytest.raises(ValueError, match="forward_lowres"):
            qs(nth_query=1, model=_M())


def test_selector_accepts_the_option_off_alone_and_combined():
    for kw in ({}, dict(region_radius=0), dict(region_radius=None)):
        for mode in (dict(query_strategy="random"), dict(use_mc_dropout=True), dict(n_classes=300), dict(region_mode="sum")):
            qs = ppq.QuerySelector(_args(**kw, **mode), _DL(), device=torch.device("cpu"))
            assert qs.region_radius == 0 and not qs._region_on
    for st in ("entropy", "least_confidence", "margin_sampling"):
        for mode in ("product", "impurity", "uncertainty", None):
            qs = ppq.QuerySelector(_args(region_radius=1, region_mode=mode, query_strategy=st), _DL(), device=torch.device("cpu"))
            assert qs._region_on and qs.region_mode == (mode or "product")
    for kw in (dict(top_n_percent=0.05), dict(reverse_order=True, top_n_percent=0.05), dict(min_pixel_distance=5), dict(n_classes=256)):
        qs = ppq.QuerySelector(_args(region_radius=16, **kw), _DL(), device=torch.device("cpu"))
        assert qs._region_on
    qs = ppq.QuerySelector(_args(region_radius=3, top_n_percent=0.05), _DL(), device=torch.device("cpu"))
    assert qs._k_launch(64, 96) == int(64 * 96 * 0.05)
    qs = ppq.QuerySelector(_args(region_radius=3, min_pixel_distance=4), _DL(), device=torch.device("cpu"))
    assert qs._k_launch(64, 96) == acq.spread_candidates(6, 4, 64 * 96)
