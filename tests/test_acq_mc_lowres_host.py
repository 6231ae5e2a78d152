"""CPU-only: argument validation of pp_acq_lowres_mc_score_topk / pp_acq_lowres_mc_score_at on the PRODUCT library (a process of its
own on libpixelpick_hip.so, no launch: every call below is refused before anything is enqueued, the pointers are never read), and the
errors the Python wrappers raise without a GPU."""
import json
import os
import subprocess
import sys

import pytest
import torch

from pixelpick_amd import _lib
from pixelpick_amd import acquisition as acq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

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
    rc = L.pp_acq_lowres_mc_score_topk(low, ldx, B, T, C, h, w, H, W, 1, Hc, Wc, None, strategy, 1.0 / max(T, 1), k, out_idx, None, None,
                                       ws, ws_bytes, None)
    return [rc, L.pp_last_error().decode()]

def at(low=P, ldx=C, B=B, T=T, C=C, Hc=H, Wc=W, img=P, pix=P, n=5, out=P, strategy=0):
    rc = L.pp_acq_lowres_mc_score_at(low, ldx, B, T, C, h, w, H, W, 1, Hc, Wc, strategy, 1.0 / max(T, 1), img, pix, n, out, None)
    return [rc, L.pp_last_error().decode()]

res = {
    "topk:T=0": topk(T=0), "topk:C=0": topk(C=0, ldx=19), "topk:C=65": topk(C=65, ldx=65), "topk:ldx<C": topk(ldx=18),
    "topk:crop>size": topk(Hc=H + 1), "topk:k>HcWc": topk(k=H * W + 1), "topk:null out_idx": topk(out_idx=None),
    "topk:workspace 1 B short": topk(ws_bytes=need - 1), "topk:large-k workspace 1 B short": topk(k=307, ws_bytes=need_large - 1),
    "topk:misaligned workspace": topk(ws=Q), "topk:null low": topk(low=None), "topk:strategy 3": topk(strategy=3),
    "topk:T<0": topk(T=-1), "topk:k=0 without map": topk(k=0),
    "at:T=0": at(T=0), "at:C=0": at(C=0, ldx=19), "at:C=65": at(C=65, ldx=65), "at:ldx<C": at(ldx=18), "at:crop>size": at(Wc=W + 1),
    "at:null low": at(low=None), "at:null img_idx": at(img=None), "at:null out": at(out=None), "at:n<0": at(n=-1),
    "at:n=0 is ok": at(n=0, img=None, pix=None, out=None),
}
print("RESULT " + json.dumps(res))
"""

CODES = {"topk:C=65": -4, "at:C=65": -4, "topk:k>HcWc": -2, "topk:workspace 1 B short": -3, "topk:large-k workspace 1 B short": -3}
CASES = ["topk:T=0", "topk:C=0", "topk:C=65", "topk:ldx<C", "topk:crop>size", "topk:k>HcWc", "topk:null out_idx",
         "topk:workspace 1 B short", "topk:large-k workspace 1 B short", "topk:misaligned workspace", "topk:null low", "topk:strategy 3",
         "topk:T<0", "topk:k=0 without map", "at:T=0", "at:C=0", "at:C=65", "at:ldx<C", "at:crop>size", "at:null low", "at:null img_idx",
         "at:null out", "at:n<0"]


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


def test_every_case_ran_and_an_empty_list_is_not_an_error(results):
    assert set(results) == set(CASES) | {"at:n=0 is ok"}
    assert results["at:n=0 is ok"][0] == 0


def test_wrappers_raise_without_a_gpu():
    low = torch.zeros(6, 4, 4, 19)
    with pytest.raises(ValueError, match="multiple of n_passes"):
        acq.mc_score_topk_lowres(low, 4, (16, 16), None, "entropy", 5)
    with pytest.raises(ValueError, match="multiple of n_passes"):
        acq.mc_score_at_lowres(low, 4, (16, 16), [0], [0])
    with pytest.raises(ValueError):
        acq.mc_score_topk_lowres(low, 0, (16, 16), None, "entropy", 5)
    with pytest.raises(_lib.PixelPickHipError, match="no CPU fallback"):
        acq.mc_score_topk_lowres(low, 3, (16, 16), None, "entropy", 5)
    with pytest.raises(_lib.PixelPickHipError, match="no CPU fallback"):
        acq.mc_score_at_lowres(low, 3, (16, 16), [0], [0])
