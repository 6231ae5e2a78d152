"""CPU tests of the weighted-loss surface: utils.balanced_class_weights, the host-side refusals of FlatTrainer's class_weight /
label_smoothing (trainer.check_loss_options needs no device), and the two weighted entries declared, exported, bound, in the launch
plan's table, and refusing a bad label_smoothing on the host."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from pixelpick_amd import _lib
from pixelpick_amd.trainer import check_loss_options
from pixelpick_amd.utils.utils import balanced_class_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x7F0000000000          # a fake device address: never read on the host
ENTRIES = {"pp_sparse_ce_weighted_fwd_bwd": 17, "pp_sparse_ce_lowres_weighted_fwd_bwd": 21}


def _ensure_built():
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(_lib.KNOBS_LIB_PATH)):
        from pixelpick_amd import build
        build.build(verbose=False)


def test_balanced_class_weights_known_counts():
    w = balanced_class_weights([10, 30, 60])
    assert isinstance(w, list) and all(isinstance(v, float) for v in w)
    assert w == [100 / 30, 100 / 90, 100 / 180]
    # the weights average 1 over the labels counted: the loss keeps its scale
    assert abs(sum(c * v for c, v in zip([10, 30, 60], w)) / 100 - 1.0) < 1e-15
    assert balanced_class_weights([5, 5, 5, 5]) == [1.0] * 4
    assert balanced_class_weights({0: 10, 2: 30}) == [40 / 20, 1.0, 40 / 60]          # QueryStats.dict_label_cnt's form


def test_balanced_class_weights_zero_counts():
    w = balanced_class_weights([10, 0, 30])
    assert w == [40 / 20, 1.0, 40 / 60]                   # K counts the classes seen; a class with no count keeps 1.0
    assert balanced_class_weights([0, 0, 0]) == [1.0, 1.0, 1.0]
    assert balanced_class_weights(np.array([0, 7])) == [1.0, 1.0]
    for bad in ([1, -1], [1, float("nan")], [float("inf"), 1]):
        with pytest.raises(ValueError):
            balanced_class_weights(bad)


def test_trainer_loss_options_accepted():
    assert check_loss_options(None, 0.0, 19) == (None, 0.0)
    assert check_loss_options(None, 0.1) == (None, 0.1)
    w, eps = check_loss_options([1, 0, 2.5], 0, 3)
    assert w == [1.0, 0.0, 2.5] and eps == 0.0 and isinstance(eps, float)
    w, _ = check_loss_options(torch.tensor([0.25, 4.0]), 0.5, 2)
    assert w == [0.25, 4.0]
    w, _ = check_loss_options(np.array([1.0, 2.0], dtype=np.float32), 0.0, 2)
    assert w == [1.0, 2.0]


@pytest.mark.parametrize("weights,eps,n", [
    ([1.0, 2.0], 0.0, 3),                                 # length
    ([1.0] * 20, 0.0, 19),
    ([], 0.0, None),
    ([1.0, float("nan"), 1.0], 0.0, 3),                   # finiteness
    ([1.0, float("inf"), 1.0], 0.0, 3),
    ([1.0, -0.5, 1.0], 0.0, 3),                           # sign
    (torch.ones(2, 3), 0.0, 6),                           # shape
    ("abc", 0.0, 3),
    (None, -0.1, 3),                                      # label_smoothing in [0, 1)
    (None, 1.0, 3),
    (None, 1.5, 3),
    (None, float("nan"), 3),
    (None, "x", 3),
])
def test_trainer_loss_options_refused(weights, eps, n):
    with pytest.raises(ValueError):
        check_loss_options(weights, eps, n)


def test_weighted_entries_are_declared_exported_bound_and_planned():
    _ensure_built()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pixelpick_hip.h")).read(), flags=re.S)
    L = _lib.lib()
    for name, arity in ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", hdr)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        assert len(params) == arity
        i = next(k for k, p in enumerate(params) if p == "int ignore_index")
        assert params[i + 1] == "const float* class_weight" and params[i + 2] == "float label_smoothing"
        assert params[i + 3] == "float* loss" and params[i + 4] == "float* wsum"
        for path in (_lib.LIB_PATH, _lib.KNOBS_LIB_PATH):
            assert f" T {name}" in subprocess.check_output(["nm", "-D", "--defined-only", path]).decode(), path
        res, args = _lib.SIGNATURES[name]
        assert len(args) == arity and args[i + 1] is _lib._p and args[i + 2] is _lib._f
        assert _lib._is_launch(name)
        assert L.pp_plan_entry_args(ctypes.cast(getattr(_lib.lib_real(), name), ctypes.c_void_p)) == arity      # csrc/plan.hip kEntries
    # the un-weighted entries keep their signatures
    assert len(_lib.SIGNATURES["pp_sparse_ce_fwd_bwd"][1]) == 15 and len(_lib.SIGNATURES["pp_sparse_ce_lowres_fwd_bwd"][1]) == 19


def test_weighted_entries_validate_on_the_host():
    _ensure_built()
    L = _lib.lib()
    low = L.pp_sparse_ce_lowres_weighted_fwd_bwd
    nchw = L.pp_sparse_ce_weighted_fwd_bwd
    for eps in (-0.1, 1.5, float("nan"), float("inf")):
        assert low(P, 19, 1, 19, 4, 4, 16, 16, 1, P, 255, P, eps, P, P, None, P, 19, P, 1 << 20, None) == -1
        assert b"label_smoothing" in L.pp_last_error()
        assert nchw(P, 1, 19, 16, 19 * 16, 16, P, 255, None, eps, P, P, None, P, P, 1 << 20, None) == -1
        assert b"label_smoothing" in L.pp_last_error()
    # a valid smoothing (0, 1 and in between; weights NULL or not) gets as far as the workspace check, whatever the class count
    for C in (19, 65, 150, 1000):
        for eps in (0.0, 0.1, 1.0):
            assert low(P, C, 1, C, 4, 4, 16, 16, 1, P, 255, None, eps, P, P, None, P, C, None, 0, None) == -3
            assert nchw(P, 1, C, 16, C * 16, 16, P, 255, P, eps, P, P, None, None, None, 0, None) == -3
    assert low(None, 19, 1, 19, 4, 4, 16, 16, 1, P, 255, P, 0.1, P, P, None, P, 19, P, 1 << 20, None) == -1 and b"null" in L.pp_last_error()
    assert low(P, 19, 1, 19, 4, 4, 16, 16, 1, P, 255, P, 0.1, P, None, None, P, 19, P, 1 << 20, None) == -1 and b"null" in L.pp_last_error()
    assert low(P, 18, 1, 19, 4, 4, 16, 16, 1, P, 255, P, 0.1, P, P, None, P, 19, P, 1 << 20, None) == -1 and b"shape" in L.pp_last_error()
    assert low(P, 19, 1, 19, 4, 4, 16, 16, 1, P, 255, P, 0.1, P, P, None, P, 18, P, 1 << 20, None) == -1 and b"shape" in L.pp_last_error()
    assert nchw(P, 1, 19, 16, 19 * 16, 16, None, 255, P, 0.1, P, P, None, P, P, 1 << 20, None) == -1 and b"null" in L.pp_last_error()
    assert nchw(P, 1, 0, 16, 0, 16, P, 255, P, 0.1, P, P, None, P, P, 1 << 20, None) == -1 and b"shape" in L.pp_last_error()
