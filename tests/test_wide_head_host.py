"""CPU tests of the wide-head surface: pp_confusion_matrix_from_labels is declared, exported, bound and validates its arguments on the
host; the loss entry no longer refuses a class count before it looks at the workspace; RunningScore.update_from_labels has no CPU
fallback."""
import os
import re
import subprocess

import pytest
import torch

from pixelpick_amd import _lib
from pixelpick_amd.utils.metrics import RunningScore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x7F0000000000          # a fake device address: never read on the host


def _ensure_built():
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(_lib.KNOBS_LIB_PATH)):
        from pixelpick_amd import build
        build.build(verbose=False)


def test_confusion_matrix_from_labels_is_declared_exported_and_bound():
    _ensure_built()
    hdr = open(os.path.join(ROOT, "include", "pixelpick_hip.h")).read()
    assert re.search(r"\bint\s+pp_confusion_matrix_from_labels\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    for path in (_lib.LIB_PATH, _lib.KNOBS_LIB_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert " T pp_confusion_matrix_from_labels" in out, path
    assert "pp_confusion_matrix_from_labels" in _lib.SIGNATURES and "pp_debug_set_ce_stream" in _lib.KNOB_SIGNATURES
    assert "pp_debug_set_ce_stream" not in subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert _lib._is_launch("pp_confusion_matrix_from_labels")


def test_confusion_matrix_from_labels_validates_on_the_host():
    _ensure_built()
    L = _lib.lib()
    f = L.pp_confusion_matrix_from_labels
    for args in ((None, P, 1, 8, 19, P, None), (P, None, 1, 8, 19, P, None), (P, P, 1, 8, 19, None, None)):
        assert f(*args) == -1 and b"null" in L.pp_last_error()
    assert f(P, P, 2, -1, 19, P, None) == -1 and b"n=-1" in L.pp_last_error()
    for kind in (0, 3, -1):
        assert f(P, P, kind, 8, 19, P, None) == -1 and b"target_kind" in L.pp_last_error()
    for C in (0, 257, -5):
        assert f(P, P, 1, 8, C, P, None) == -4 and b"256" in L.pp_last_error()
    for kind in (1, 2):
        for C in (1, 19, 150, 256):
            assert f(P, P, kind, 0, C, P, None) == 0               # nothing to count: PP_OK without a launch


def test_wide_heads_pass_the_host_side_checks_of_the_loss_and_the_histogram():
    """Parent: PP_ERR_UNSUPPORTED (-4) for C > 64 / C > 104 before anything else was looked at."""
    _ensure_built()
    L = _lib.lib()
    for C in (65, 150, 256, 1000):
        rc = L.pp_sparse_ce_lowres_fwd_bwd(P, C, 1, C, 4, 4, 8, 8, 1, P, 255, P, P, None, P, C, None, 0, None)
        assert rc == -3 and b"workspace" in L.pp_last_error(), (C, rc, L.pp_last_error())
    assert L.pp_confusion_matrix_update(P, 1, 257, 16, 257 * 16, 16, P, P, None) == -4
    assert L.pp_confusion_matrix_update(P, 1, 0, 16, 0, 16, P, P, None) == -4
    assert L.pp_confusion_matrix_update(None, 1, 150, 16, 150 * 16, 16, P, P, None) == -1


def test_update_from_labels_has_no_cpu_fallback():
    rs = RunningScore(150)
    with pytest.raises(_lib.PixelPickHipError, match="no CPU fallback"):
        rs.update_from_labels(torch.zeros(8, dtype=torch.int64), torch.zeros(8, dtype=torch.uint8))
