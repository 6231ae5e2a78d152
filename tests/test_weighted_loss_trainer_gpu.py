"""GPU tests of the train step with class weights and label smoothing (FlatTrainer(class_weight=, label_smoothing=)): the
low-resolution loss route against the dense order, the weighted step recorded and replayed, and the switched-off options leaving the
un-weighted step as it was.  The form and the bars of tests/test_wide_head_trainer_gpu.py, at B = 2, 64 x 96, 19 classes."""
import warnings
from argparse import Namespace

import numpy as np
import pytest
import torch

import formula_init as fi
from pixelpick_amd import engine as E
from pixelpick_amd.networks.layers import Dropout
from pixelpick_amd.trainer import FlatTrainer
from pixelpick_amd.utils.utils import get_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C, B, H, W = 19, 2, 64, 96
EPS = 0.1


def _weights():
    u = torch.rand(C, generator=torch.Generator().manual_seed(5))
    w = torch.pow(2.0, 4.0 * u - 2.0)
    w[C // 2] = 0.0
    return w.tolist()


def _build(network):
    a = Namespace(use_mc_dropout=False, mc_dropout_p=0.2, n_classes=C, network_name=network, weight_type="random",
                  use_dilated_resnet=True, n_layers=50, width_multiplier=1.0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = get_model(a)
    m.load_state_dict(fi.formula_state_dict(m.state_dict()))
    for mod in m.modules():
        if isinstance(mod, Dropout):
            mod.p = 0.0
    return m.to(DEV)


def test_fpn_weighted_low_resolution_step_equals_the_dense_order(monkeypatch):
    """FPNSeg has no dropout, so the weighted + smoothed step through the low-resolution loss kernels and the step through full-size
    logits + the weighted NCHW loss are the same arithmetic in another order."""
    import pixelpick_amd.trainer as T
    x = fi.formula_input(B, H, W, key="wce-fl").to(DEV)
    y = fi.formula_labels(B, H, W, C, 255, 20, key="wce-fl").to(DEV)
    res = {}
    for lowres in (True, False):
        monkeypatch.setattr(T, "SPARSE_LOWRES_CE", lowres)
        m = _build("FPN").train()
        tr = FlatTrainer(m, ignore_index=255, class_weight=_weights(), label_smoothing=EPS)
        loss = tr.forward_backward(x, y, keep_logits=True)
        torch.cuda.synchronize()
        res[lowres] = (loss.item(), {k: tr._grad_view[id(p)].clone() for k, p in m.named_parameters()}, tr.last_logits.clone())
    la, ga, za = res[True]
    lb, gb, zb = res[False]
    worst = max(((ga[k] - gb[k]).norm() / (gb[k].norm() + 1e-12)).item() for k in gb)
    print(f"loss {la:.9g} vs {lb:.9g}; logits max err {(za - zb).abs().max().item():.3e} of {zb.abs().max().item():.3e}; worst gradient {worst:.3e}")
    assert np.isfinite(la) and abs(la - lb) <= 2e-6 * max(1.0, abs(lb))
    assert tuple(za.shape) == tuple(zb.shape) == (B, C, H, W)
    assert (za - zb).abs().max().item() <= 2e-5 * zb.abs().max().item()
    assert worst <= 5e-5, worst
    # the options reach the loss: the un-weighted step on the same input has another loss
    monkeypatch.setattr(T, "SPARSE_LOWRES_CE", True)
    plain = FlatTrainer(_build("FPN").train(), ignore_index=255).forward_backward(x, y).item()
    assert abs(plain - la) > 1e-3 * abs(plain), (plain, la)


def _run_steps(data, use_plan, expect, reject, **options):
    tr = FlatTrainer(_build("deeplab").train(), ignore_index=255, **options)
    E.set_dropout_device_seed(tr._seed_dev)
    losses = []
    try:
        for i in range(4):
            xb, yb = data[i % 2]
            if not use_plan:
                tr.step_count += 1
                tr._stage_hyper()
                losses.append(tr._step_body(xb, yb, "low", True).item())
            elif i == 0:
                tr.enable_replay(xb, yb, warmup=0, keep_logits="low")
                names = {getattr(fn, "__name__", "") for fn, _ in tr._plan.calls}
                assert expect in names and reject not in names, names
                losses.append(tr.last_loss.item())
            else:
                losses.append(tr.train_step(xb, yb, keep_logits="low").item())
        p = tr.flat_p.clone()
    finally:
        tr.disable_replay()
        E.set_dropout_device_seed(None)
    return p, losses


def _data(key):
    return [(fi.formula_input(B, H, W, key=f"{key}{i}").to(DEV), fi.formula_labels(B, H, W, C, 255, 20, key=f"{key}{i}").to(DEV))
            for i in range(2)]


def test_weighted_step_is_recorded_and_replayed():
    """FlatTrainer.enable_replay records the weighted entry like any other - the float label_smoothing travels through a plan slot, the
    weight vector is the trainer's own device tensor - and the replayed steps walk the eager trajectory bit for bit."""
    data = _data("wce-r")
    opts = dict(class_weight=_weights(), label_smoothing=EPS)
    p_eager, l_eager = _run_steps(data, False, None, None, **opts)
    p_plan, l_plan = _run_steps(data, True, "pp_sparse_ce_lowres_weighted_fwd_bwd", "pp_sparse_ce_lowres_fwd_bwd", **opts)
    assert all(np.isfinite(l_eager)) and l_eager == l_plan, (l_eager, l_plan)
    assert torch.equal(p_eager, p_plan)


def test_switched_off_options_leave_the_unweighted_step():
    data = _data("wce-o")
    p_off, l_off = _run_steps(data, True, "pp_sparse_ce_lowres_fwd_bwd", "pp_sparse_ce_lowres_weighted_fwd_bwd", class_weight=None,
                              label_smoothing=0.0)
    p_none, l_none = _run_steps(data, True, "pp_sparse_ce_lowres_fwd_bwd", "pp_sparse_ce_lowres_weighted_fwd_bwd")
    assert all(np.isfinite(l_off)) and l_off == l_none
    assert torch.equal(p_off, p_none)


def test_class_weight_length_is_held_to_the_models_class_count_at_construction():
    m = _build("FPN")
    assert m.n_classes == C and _build("deeplab").n_classes == C
    with pytest.raises(ValueError, match="18 elements for 19 classes"):
        FlatTrainer(m, ignore_index=255, class_weight=[1.0] * (C - 1))
    with pytest.raises(ValueError, match="7 classes"):
        FlatTrainer(m, ignore_index=255, class_weight=[1.0] * C, n_classes=7)
    del m.n_classes                                   # a model that does not state its width: the argument is required
    with pytest.raises(ValueError, match="class count"):
        FlatTrainer(m, ignore_index=255, class_weight=[1.0] * C)
    FlatTrainer(m, ignore_index=255, class_weight=[1.0] * C, n_classes=C).close()
    FlatTrainer(m, ignore_index=255, label_smoothing=0.1).close()
