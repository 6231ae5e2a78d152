"""GPU tests of the train step on a head wider than 64 classes: FlatTrainer's low-resolution loss route (streamed loss kernels)
against the dense order, DeepLab's step with keep_logits="low" feeding the wide confusion matrix, and the classifier convolutions
those steps depend on against float64."""
import warnings
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import formula_init as fi
from pixelpick_amd import _lib
from pixelpick_amd import engine as E
from pixelpick_amd.networks.layers import Dropout
from pixelpick_amd.trainer import FlatTrainer
from pixelpick_amd.utils.metrics import RunningScore
from pixelpick_amd.utils.utils import get_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C, B, H, W = 150, 2, 64, 96


def _build(n_classes, network):
    a = Namespace(use_mc_dropout=False, mc_dropout_p=0.2, n_classes=n_classes, network_name=network, weight_type="random",
                  use_dilated_resnet=True, n_layers=50, width_multiplier=1.0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = get_model(a)
    m.load_state_dict(fi.formula_state_dict(m.state_dict()))
    for mod in m.modules():
        if isinstance(mod, Dropout):
            mod.p = 0.0
    return m.to(DEV)


def test_fpn_wide_low_resolution_step_equals_the_dense_order(monkeypatch):
    """tests/test_networks_gpu.py::test_fpn_low_resolution_training_tail_equals_the_dense_order at 150 classes, with its bars: FPNSeg has
    no dropout, so the step through the streamed loss kernels and the step through full-size logits + dense loss are the same
    arithmetic in another order."""
    import pixelpick_amd.trainer as T
    x = fi.formula_input(B, H, W, key="wide-fl").to(DEV)
    y = fi.formula_labels(B, H, W, C, 255, 20, key="wide-fl").to(DEV)
    res = {}
    for lowres in (True, False):
        monkeypatch.setattr(T, "SPARSE_LOWRES_CE", lowres)
        m = _build(C, "FPN").train()
        tr = FlatTrainer(m, ignore_index=255)
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


def test_deeplab_wide_steps_keep_the_classifier_output_for_the_metrics():
    m = _build(C, "deeplab").train()
    tr = FlatTrainer(m, ignore_index=255)
    for i in range(2):
        x = fi.formula_input(B, H, W, key=f"wide-dl{i}").to(DEV)
        y = fi.formula_labels(B, H, W, C, 255, 20, key=f"wide-dl{i}").to(DEV)
        loss = tr.train_step(x, y, keep_logits="low")
        assert np.isfinite(loss.item())
        assert tr.last_logits is None and tuple(tr.last_low.shape) == (B, 16, 24, C)
        full = fi.formula_labels(B, H, W, C, 255, H * W // 2, key=f"wide-dl-full{i}").to(DEV)
        rs = RunningScore(C)
        rs.update_from_lowres(full, tr.last_low, tr.last_low_size, align_corners=tr.last_low_align)
        rs._sync()
        logits = E.bilinear(E.Tape(False), E.Var(tr.last_low), tr.last_low_size, tr.last_low_align, 0.0, out_nchw=True).t
        ref = RunningScore(C)
        ref.update([full.cpu().numpy()], [logits.cpu().argmax(dim=1).numpy()])
        np.testing.assert_array_equal(rs.confusion_matrix, ref.confusion_matrix)
        assert ref.confusion_matrix.sum() > 0


def test_wide_step_is_recorded_and_replayed():
    """FlatTrainer.enable_replay records the wide step - the loss entry is a launch-plan entry whatever kernels it dispatches to - and
    the replayed steps walk the eager trajectory bit for bit (the form of test_launch_plan_replay_matches_eager_steps)."""
    data = [(fi.formula_input(B, H, W, key=f"wide-r{i}").to(DEV), fi.formula_labels(B, H, W, C, 255, 20, key=f"wide-r{i}").to(DEV))
            for i in range(2)]

    def run(use_plan):
        tr = FlatTrainer(_build(C, "FPN").train(), ignore_index=255)
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
                    assert "pp_sparse_ce_lowres_fwd_bwd" in names and "pp_sparse_ce_fwd_bwd" not in names
                    losses.append(tr.last_loss.item())
                else:
                    losses.append(tr.train_step(xb, yb, keep_logits="low").item())
                    assert tuple(tr.last_low.shape) == (B, H // 2, W // 2, C)
            p = tr.flat_p.clone()
        finally:
            tr.disable_replay()
            E.set_dropout_device_seed(None)
        return p, losses
    p_eager, l_eager = run(False)
    p_plan, l_plan = run(True)
    assert all(np.isfinite(l_eager)) and l_eager == l_plan, (l_eager, l_plan)
    assert torch.equal(p_eager, p_plan)


LINK_CASES = [(256, 65), (256, 150), (256, 255), (128, 150)]


@pytest.mark.parametrize("Cin,Cout", LINK_CASES)
def test_classifier_convolution_of_a_wide_head_matches_float64(Cin, Cout):
    """The 1x1 classifier with bias at the widths the wide step needs (DeepLab 256 -> C, FPNSeg 128 -> C), 2 x 16 x 24 rows: forward,
    backward-data and weight / bias gradient against F.conv2d in float64, with tests/test_conv_dispatch_gpu.py's fp32-accumulation bars
    (rel-L2, max error over the reference's largest magnitude): 2e-6 / 6e-6 for forward and backward-data, 1e-6 / 1.5e-6 for the
    weight and bias gradients."""
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    Bn, Hn, Wn = 2, 16, 24
    gen = torch.Generator(device=DEV).manual_seed(1234 + Cout)
    x = torch.randn(Bn, Hn, Wn, Cin, device=DEV, generator=gen)
    w = torch.randn(1, 1, Cin, Cout, device=DEV, generator=gen) / np.sqrt(Cin)
    bias = torch.randn(Cout, device=DEV, generator=gen)
    dy = torch.randn(Bn, Hn, Wn, Cout, device=DEV, generator=gen)
    geom = (Bn, Hn, Wn, Cin, Cout, 1, 1, 1, 0, 1)

    def ws(nb):
        return torch.empty(max(int(nb), 256), dtype=torch.uint8, device=DEV), int(nb)

    y = torch.full((Bn, Hn, Wn, Cout), float("nan"), device=DEV)
    buf, nb = ws(L.pp_conv2d_fwd_workspace_bytes(*geom))
    _lib.check(L.pp_conv2d_fwd(x.data_ptr(), Cin, Bn, Hn, Wn, Cin, w.data_ptr(), bias.data_ptr(), 1, 1, 1, 0, 1, y.data_ptr(), Cout, Cout,
                               buf.data_ptr(), nb, st), "pp_conv2d_fwd")
    dx = torch.full((Bn, Hn, Wn, Cin), float("nan"), device=DEV)
    buf2, nb2 = ws(L.pp_conv2d_bwd_data_workspace_bytes(*geom))
    _lib.check(L.pp_conv2d_bwd_data(dy.data_ptr(), Cout, Bn, Hn, Wn, Cout, w.data_ptr(), 1, 1, 1, 0, 1, dx.data_ptr(), Cin, Hn, Wn, Cin, 0,
                                    buf2.data_ptr(), nb2, st), "pp_conv2d_bwd_data")
    dw = torch.zeros((1, 1, Cin, Cout), device=DEV)
    db = torch.full((Cout,), float("nan"), device=DEV)
    buf3, nb3 = ws(L.pp_conv2d_bwd_weight_workspace_bytes(*geom))
    _lib.check(L.pp_conv2d_bwd_weight(x.data_ptr(), Cin, Bn, Hn, Wn, Cin, dy.data_ptr(), Cout, Cout, 1, 1, 1, 0, 1, dw.data_ptr(),
                                      db.data_ptr(), buf3.data_ptr(), nb3, st), "pp_conv2d_bwd_weight")
    torch.cuda.synchronize()
    xd, wd = x.double().cpu().permute(0, 3, 1, 2), w.double().cpu().permute(3, 2, 0, 1)
    dyd = dy.double().cpu().permute(0, 3, 1, 2)
    ref = {"y": F.conv2d(xd, wd, bias.double().cpu()).permute(0, 2, 3, 1),
           "dx": torch.nn.grad.conv2d_input((Bn, Cin, Hn, Wn), wd, dyd).permute(0, 2, 3, 1),
           "dw": torch.nn.grad.conv2d_weight(xd, (Cout, Cin, 1, 1), dyd).permute(2, 3, 1, 0),
           "db": dy.double().cpu().sum(dim=(0, 1, 2))}
    got = {"y": y, "dx": dx, "dw": dw, "db": db}
    bars = {"y": (2e-6, 6e-6), "dx": (2e-6, 6e-6), "dw": (1e-6, 1.5e-6), "db": (1e-6, 1.5e-6)}
    errs = {}
    for k in ref:
        dlt = got[k].double().cpu() - ref[k]
        errs[k] = ((dlt.norm() / ref[k].norm()).item(), (dlt.abs().max() / ref[k].abs().max()).item())
    print(" | ".join(f"{k} rel-l2 {e[0]:.2e} max-rel {e[1]:.2e}" for k, e in errs.items()))
    for k, (e2, emax) in errs.items():
        assert e2 <= bars[k][0] and emax <= bars[k][1], f"{k}: rel-l2 {e2:.3e} (bar {bars[k][0]:g}), max-rel {emax:.3e} (bar {bars[k][1]:g})"
