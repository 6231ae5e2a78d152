"""GPU tests of the class-weighted / label-smoothed sparse-pixel loss (pp_sparse_ce_weighted_fwd_bwd and
pp_sparse_ce_lowres_weighted_fwd_bwd: the WT = true instantiations of the loss kernels in csrc/nn_ops.hip).  The reference is torch on the
CPU in float64: autograd through F.interpolate + F.cross_entropy(weight=, label_smoothing=); the second yardstick is the library's own
dense path (pp_bilinear_fwd -> pp_sparse_ce_weighted_fwd_bwd -> pp_bilinear_bwd).  The inputs are built as
tests/test_wide_head_loss_gpu.py::_inputs builds them and the bars are that file's (1e-5 loss, 2e-5 gradient against float64; 2e-6 / 1e-5
against the dense path): torch's own float32 path stays within 2.1e-7 / 1.5e-6 of float64 on shapes like these, so the bars leave the
kernels a factor of ten or more."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from pixelpick_amd import _lib
from pixelpick_amd import engine as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAD_ARG = -1


def close(a, b, tol, what=""):
    a, b = a.double().cpu(), b.double().cpu()
    scale = max(b.abs().max().item(), 1e-6)
    err = (a - b).abs().max().item()
    print(f"{what}: max err {err:.3e} vs scale {scale:.3e} (bar {tol:.1e} * scale)")
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def _weights(C):
    """2^(4u-2), u uniform: weights in [0.25, 4]; class C//2 has weight 0, so that a zero-weight class occurs among the targets."""
    u = torch.rand(C, generator=torch.Generator().manual_seed(5))
    w = torch.pow(2.0, 4.0 * u - 2.0).float()
    w[C // 2] = 0.0
    return w


@functools.lru_cache(maxsize=None)
def _inputs(B, C, lo, size, n_lab, ign):
    """(low [B,C,h,w] CPU, y [B,H,W] CPU, low_d: channel slice of a wider device buffer (ldx > C), y on the device, weights CPU / device);
    built once per case and never modified."""
    torch.manual_seed(8)
    H, W = size
    n = H * W if n_lab is None else n_lab
    low = torch.randn(B, C, *lo) * 3
    y = torch.full((B, H, W), ign, dtype=torch.int64)
    for b in range(B):
        idx = torch.randperm(H * W)[:n]
        y[b].view(-1)[idx] = torch.randint(0, C, (len(idx),))
    wide = torch.full((B, *lo, C + 3), 5.0, device=DEV)
    wide[..., :C] = low.permute(0, 2, 3, 1).to(DEV)
    w = _weights(C)
    return low, y, wide[..., :C], y.to(DEV), w, w.to(DEV)


@functools.lru_cache(maxsize=None)
def _reference64(B, C, lo, size, n_lab, ign, align, use_w, eps):
    low, y, _, _, w, _ = _inputs(B, C, lo, size, n_lab, ign)
    l64 = low.double().requires_grad_(True)
    lr = F.cross_entropy(F.interpolate(l64, size=size, mode="bilinear", align_corners=align), y, weight=w.double() if use_w else None,
                         ignore_index=ign, label_smoothing=eps)
    lr.backward()
    return lr.item(), l64.grad


CASES = [
    # B, C, (h,w), (H,W), labelled px/img (None: every pixel), ignore_index, align_corners
    (2, 19, (8, 8), (32, 32), 64, 19, True),              # exact-class form
    (2, 26, (8, 8), (32, 32), 64, 26, True),              # generic <= 32
    (1, 40, (8, 8), (32, 32), 50, 255, True),             # generic <= 64
    (1, 19, (9, 13), (33, 47), None, 19, True),           # every pixel labelled: borders, clamped taps
    (2, 21, (6, 10), (12, 20), 30, 255, False),           # the x2 arithmetic
    (2, 65, (8, 8), (32, 32), 64, 255, True),             # first streamed width
    (2, 129, (6, 10), (12, 20), 30, 255, False),          # a chunk tail of one class
    (1, 150, (9, 13), (33, 47), None, 255, True),
    (1, 256, (8, 8), (32, 32), 50, 256, True),
]
MODES = [(True, 0.0), (False, 0.1), (True, 0.1)]          # (weights?, label_smoothing)


@pytest.mark.parametrize("use_w,eps", MODES)
@pytest.mark.parametrize("B,C,lo,size,n_lab,ign,align", CASES)
def test_weighted_cross_entropy_from_lowres_logits(B, C, lo, size, n_lab, ign, align, use_w, eps):
    low, y, low_d, yd, w, wd = _inputs(B, C, lo, size, n_lab, ign)
    ref_loss, ref_grad = _reference64(B, C, lo, size, n_lab, ign, align, use_w, eps)
    kw = dict(class_weight=wd if use_w else None, label_smoothing=eps)
    loss, dlow = E.cross_entropy_lowres(low_d, size, yd, ign, align_corners=align, **kw)
    print(f"loss {loss.item():.9g} vs float64 {ref_loss:.9g}: err {abs(loss.item() - ref_loss):.3e}")
    assert abs(loss.item() - ref_loss) < 1e-5 * max(1.0, abs(ref_loss))
    close(dlow.permute(0, 3, 1, 2), ref_grad, tol=2e-5, what="dlow vs float64 autograd")
    # dense product path
    tape = E.Tape(True)
    lv = E.Var(low_d.contiguous())
    pred = E.bilinear(tape, lv, size, align, 0.0, out_nchw=True)
    loss2, dl = E.cross_entropy_nchw(pred.t, yd, ign, **kw)
    tape.backward(pred, dl)
    assert abs(loss.item() - loss2.item()) < 2e-6 * max(1.0, abs(loss2.item()))
    close(dlow, lv.grad, tol=1e-5, what="dlow vs dense path")
    # fixed-order gather: bitwise reproducible
    loss3, dlow3 = E.cross_entropy_lowres(low_d, size, yd, ign, align_corners=align, **kw)
    assert torch.equal(loss3, loss) and torch.equal(dlow3, dlow)
    # densely labelled mode: the same kernels, the same bits, no row flags
    loss4, dlow4 = E.cross_entropy_lowres(low_d, size, yd, ign, align_corners=align, sparse=False, **kw)
    assert torch.equal(loss4, loss) and torch.equal(dlow4, dlow)
    assert getattr(dlow4, "_pp_rowflags", None) is None


def _raw_lowres(low_d, C, lo, size, yd, ign, w_ptr, eps, g=None, lddx=None, want_grad=True, fill=7.0):
    """The C entry itself: (rc, out = [loss, wsum], dlow buffer [B,h,w,lddx] pre-filled with `fill`)."""
    L = _lib.lib()
    B = low_d.shape[0]
    lddx = C if lddx is None else lddx
    ws = torch.empty(L.pp_sparse_ce_lowres_workspace_bytes(), dtype=torch.uint8, device=DEV)
    out = torch.full((2,), -3.0, device=DEV)
    d = torch.full((B, *lo, lddx), fill, device=DEV)
    rc = L.pp_sparse_ce_lowres_weighted_fwd_bwd(low_d.data_ptr(), low_d.stride(2), B, C, lo[0], lo[1], size[0], size[1], 1, yd.data_ptr(),
                                                ign, w_ptr, eps, out.data_ptr(), out[1:].data_ptr(),
                                                g.data_ptr() if g is not None else None, d.data_ptr() if want_grad else None, lddx,
                                                ws.data_ptr(), ws.numel(), _lib.current_stream_ptr())
    torch.cuda.synchronize()
    return rc, out, d


@pytest.mark.parametrize("C", [19, 40])
@pytest.mark.parametrize("use_w,eps", MODES)
def test_weighted_streamed_kernels_agree_with_the_register_kernels(C, use_w, eps):
    """pp_debug_set_ce_stream forces the streamed form for the weighted entry too; bars of
    tests/test_wide_head_loss_gpu.py::test_streamed_kernels_agree_with_the_register_kernels."""
    case = (2, C, (8, 8), (32, 32), 64, 19, True) if C == 19 else (1, C, (8, 8), (32, 32), 50, 255, True)
    _, _, low_d, yd, _, wd = _inputs(*case[:6])
    kw = dict(class_weight=wd if use_w else None, label_smoothing=eps)
    L = _lib.lib()
    loss_r, dlow_r = E.cross_entropy_lowres(low_d, case[3], yd, case[5], **kw)
    L.pp_debug_launch_log(None, 0)
    try:
        L.pp_debug_set_ce_stream(1)
        loss_s, dlow_s = E.cross_entropy_lowres(low_d, case[3], yd, case[5], **kw)
        cbuf = ctypes.create_string_buffer(4096)
        L.pp_debug_launch_log(cbuf, 4096)
        names = cbuf.value.decode()
    finally:
        L.pp_debug_set_ce_stream(0)
    assert "ce_lowres_stream_partial_kernel" in names and "ce_lowres_stream_bwd_kernel" in names, names
    assert abs(loss_s.item() - loss_r.item()) < 2e-6 * max(1.0, abs(loss_r.item()))
    close(dlow_s, dlow_r, tol=1e-5, what="streamed vs register kernels")


@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[4], CASES[5], CASES[7]], ids=lambda c: f"C{c[1]}")
def test_unit_weights_without_smoothing_are_the_unweighted_bits(case):
    """Weights all 1.0 and label_smoothing 0 go through the weighted kernels (an explicit weight vector selects them) and must give the
    un-weighted entry's bits: register form, streamed form (forced on the narrow heads, native on the wide ones) and the NCHW entry."""
    B, C, lo, size, n_lab, ign, align = case
    _, _, low_d, yd, _, _ = _inputs(B, C, lo, size, n_lab, ign)
    ones = torch.ones(C, device=DEV)
    L = _lib.lib()
    for stream in (0, 1):
        try:
            L.pp_debug_set_ce_stream(stream)
            L.pp_debug_launch_log(None, 0)
            l0, d0 = E.cross_entropy_lowres(low_d, size, yd, ign, align_corners=align)
            l1, d1 = E.cross_entropy_lowres(low_d, size, yd, ign, align_corners=align, class_weight=ones)
            cbuf = ctypes.create_string_buffer(4096)
            L.pp_debug_launch_log(cbuf, 4096)
        finally:
            L.pp_debug_set_ce_stream(0)
        assert "<weighted>" in cbuf.value.decode(), cbuf.value.decode()
        assert torch.equal(l0, l1) and torch.equal(d0, d1), f"forced stream {stream}"
    pred = E.bilinear(E.Tape(False), E.Var(low_d.contiguous()), size, align, 0.0, out_nchw=True).t
    l0, d0 = E.cross_entropy_nchw(pred, yd, ign)
    l1, d1 = E.cross_entropy_nchw(pred, yd, ign, class_weight=ones)
    assert torch.equal(l0, l1) and torch.equal(d0, d1)


@pytest.mark.parametrize("case", [CASES[0], CASES[7]], ids=lambda c: f"C{c[1]}")
def test_weighted_entry_honours_wsum_grad_out_lddx_and_loss_only(case):
    B, C, lo, size, n_lab, ign, align = case
    _, y, low_d, yd, w, wd = _inputs(B, C, lo, size, n_lab, ign)
    loss, dlow = E.cross_entropy_lowres(low_d, size, yd, ign, class_weight=wd, label_smoothing=0.1)
    loss_only, none = E.cross_entropy_lowres(low_d, size, yd, ign, class_weight=wd, label_smoothing=0.1, want_grad=False)
    assert none is None and torch.equal(loss_only, loss)
    g = torch.full((1,), 0.25, device=DEV)
    rc, out, d2 = _raw_lowres(low_d, C, lo, size, yd, ign, wd.data_ptr(), 0.1, g=g, lddx=C + 3)
    assert rc == 0
    assert out[0].item() == loss.item()
    wsum64 = w.double()[y[y != ign]].sum().item()
    print(f"wsum {out[1].item():.9g} vs float64 {wsum64:.9g}")
    assert abs(out[1].item() - wsum64) <= 1e-6 * wsum64
    assert (d2[..., C:] == 7.0).all()                                   # lddx > C: the spare channels stay untouched
    assert torch.equal(d2[..., :C], dlow * 0.25)                        # a power of two scales exactly


@pytest.mark.parametrize("C", [19, 150])
def test_target_outside_the_classes_counts_as_unlabelled(C):
    """A target of C + 5 (not the ignore index) adds to no sum and no gradient - and never indexes the weight vector."""
    case = CASES[0] if C == 19 else (1, 150, (8, 8), (32, 32), 50, 255, True)
    B, _, lo, size, n_lab, _, _ = case
    ign = 255
    _, y, low_d, _, _, wd = _inputs(B, C, lo, size, n_lab, ign)
    pos = (y.view(-1) != ign).nonzero()[3].item()
    y_bad, y_ign = y.clone(), y.clone()
    y_bad.view(-1)[pos] = C + 5
    y_ign.view(-1)[pos] = ign
    for kw in (dict(class_weight=wd, label_smoothing=0.1), dict(class_weight=None, label_smoothing=0.1)):
        la, da = E.cross_entropy_lowres(low_d, size, y_bad.to(DEV), ign, **kw)
        lb, db = E.cross_entropy_lowres(low_d, size, y_ign.to(DEV), ign, **kw)
        assert math.isfinite(la.item()) and torch.equal(la, lb) and torch.equal(da, db)
    pred = E.bilinear(E.Tape(False), E.Var(low_d.contiguous()), size, True, 0.0, out_nchw=True).t
    la, da = E.cross_entropy_nchw(pred, y_bad.to(DEV), ign, class_weight=wd, label_smoothing=0.1)
    lb, db = E.cross_entropy_nchw(pred, y_ign.to(DEV), ign, class_weight=wd, label_smoothing=0.1)
    assert torch.equal(la, lb) and torch.equal(da, db)


@pytest.mark.parametrize("C", [19, 150])
def test_only_zero_weight_labels_give_a_nan_loss(C):
    low = torch.randn(1, 8, 8, C, device=DEV)
    y = torch.full((1, 32, 32), 255, dtype=torch.int64, device=DEV)
    y[0, 3, 5] = C // 2
    y[0, 20, 11] = C // 2
    wd = _weights(C).to(DEV)
    for eps in (0.0, 0.1):
        loss, _ = E.cross_entropy_lowres(low, (32, 32), y, 255, class_weight=wd, label_smoothing=eps)
        assert torch.isnan(loss).all()                     # 0/0 like F.cross_entropy
    pred = E.bilinear(E.Tape(False), E.Var(low), (32, 32), True, 0.0, out_nchw=True).t
    for eps in (0.0, 0.1):                                 # eps > 0: the folded numerator is positive, the finalize answers NaN by hand
        loss, _ = E.cross_entropy_nchw(pred, y, 255, class_weight=wd, label_smoothing=eps)
        assert torch.isnan(loss).all()


@pytest.mark.parametrize("eps", [-0.1, 1.5, float("nan")])
def test_label_smoothing_outside_the_unit_interval_is_refused(eps):
    B, C, lo, size, n_lab, ign, _ = CASES[0]
    _, _, low_d, yd, _, wd = _inputs(B, C, lo, size, n_lab, ign)
    rc, out, d = _raw_lowres(low_d, C, lo, size, yd, ign, wd.data_ptr(), eps)
    assert rc == BAD_ARG
    assert (out == -3.0).all() and (d == 7.0).all()        # nothing was enqueued
    L = _lib.lib()
    pred = torch.zeros(1, C, 4, 4, device=DEV)
    y = torch.zeros(1, 4, 4, dtype=torch.int64, device=DEV)
    ws = torch.empty(L.pp_sparse_ce_workspace_bytes(), dtype=torch.uint8, device=DEV)
    out = torch.full((2,), -3.0, device=DEV)
    dl = torch.full((1, C, 4, 4), 7.0, device=DEV)
    rc = L.pp_sparse_ce_weighted_fwd_bwd(pred.data_ptr(), 1, C, 16, C * 16, 16, y.data_ptr(), ign, None, eps, out.data_ptr(),
                                         out[1:].data_ptr(), None, dl.data_ptr(), ws.data_ptr(), ws.numel(), _lib.current_stream_ptr())
    torch.cuda.synchronize()
    assert rc == BAD_ARG and (out == -3.0).all() and (dl == 7.0).all()
    with pytest.raises(ValueError):
        E.cross_entropy_lowres(low_d, size, yd, ign, label_smoothing=eps)


def test_engine_refuses_a_bad_weight_vector_before_any_launch():
    B, C, lo, size, n_lab, ign, _ = CASES[0]
    _, _, low_d, yd, w, wd = _inputs(B, C, lo, size, n_lab, ign)
    pred = torch.zeros(B, C, *size, device=DEV)
    L = _lib.lib()
    L.pp_debug_launch_log(None, 0)
    for bad in (w, wd.double(), torch.ones(C + 1, device=DEV), torch.ones(C - 1, device=DEV), torch.ones(1, C, device=DEV), [1.0] * C):
        with pytest.raises(ValueError):
            E.cross_entropy_lowres(low_d, size, yd, ign, class_weight=bad)
        with pytest.raises(ValueError):
            E.cross_entropy_nchw(pred, yd, ign, class_weight=bad)
    cbuf = ctypes.create_string_buffer(4096)
    L.pp_debug_launch_log(cbuf, 4096)
    assert "ce_" not in cbuf.value.decode(), cbuf.value.decode()
