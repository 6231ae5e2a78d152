"""GPU tests of the low-resolution loss on heads wider than 64 classes (csrc/nn_ops.hip: ce_lowres_stream_partial_kernel /
ce_lowres_stream_bwd_kernel behind pp_sparse_ce_lowres_fwd_bwd).  The reference is torch on the CPU in float64: autograd through
F.interpolate + F.cross_entropy; the second yardstick is the library's own dense path (pp_bilinear_fwd -> pp_sparse_ce_fwd_bwd ->
pp_bilinear_bwd).  The inputs are built as tests/test_nn_ops_gpu.py::test_cross_entropy_from_lowres_logits builds them, and the bars
are that test's: on exactly these inputs torch's own float32 path stays within 1.2e-7 (loss) and 7.2e-7 (gradient) of float64, so
1e-5 / 2e-5 leave the kernels more than a factor of 20."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from pixelpick_amd import _lib
from pixelpick_amd import engine as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def close(a, b, tol, what=""):
    a, b = a.double().cpu(), b.double().cpu()
    scale = max(b.abs().max().item(), 1e-6)
    err = (a - b).abs().max().item()
    print(f"{what}: max err {err:.3e} vs scale {scale:.3e} (bar {tol:.1e} * scale)")
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def _inputs(B, C, lo, size, n_lab, ign, mode):
    torch.manual_seed(8)
    H, W = size
    low = torch.randn(B, C, *lo) * (30 if mode == "x30" else 3)
    if mode == "last_chunk_max":            # the maximum sits in the last chunk, the first class far below everything
        low[:, C - 1] += 60.0
        low[:, 0] -= 60.0
    y = torch.full((B, H, W), ign, dtype=torch.int64)
    for b in range(B):
        idx = torch.randperm(H * W)[:n_lab]
        y[b].view(-1)[idx] = torch.randint(0, C, (len(idx),))
    wide = torch.full((B, *lo, C + 3), 5.0, device=DEV)                   # channel slice of a wider buffer (ldx > C)
    wide[..., :C] = low.permute(0, 2, 3, 1).to(DEV)
    return low, y, wide[..., :C]


def _reference64(low, y, size, ign, align):
    l64 = low.double().requires_grad_(True)
    lr = F.cross_entropy(F.interpolate(l64, size=size, mode="bilinear", align_corners=align), y, ignore_index=ign)
    lr.backward()
    return lr.item(), l64.grad


WIDE_CASES = [
    # B, C, (h,w), (H,W), labelled px/img (None: every pixel), ignore_index, align_corners, input mode
    (2, 65, (8, 8), (32, 32), 64, 255, True, ""),                   # first width beyond the registers
    (1, 150, (9, 13), (33, 47), None, 255, True, ""),               # dense labels, borders, a chunk tail of 22
    (2, 129, (6, 10), (12, 20), 30, 255, False, ""),                # one class past a chunk, the other arithmetic
    (1, 255, (8, 8), (32, 32), 50, 255, True, ""),                  # the widest byte-labelled head
    (1, 256, (8, 8), (32, 32), 50, 256, True, ""),
    (1, 150, (16, 16), (16, 16), 30, 255, True, ""),                # identity size
    (1, 150, (8, 8), (32, 32), 50, 255, True, "last_chunk_max"),    # a wrong running maximum overflows or flushes the sum
    (1, 200, (8, 8), (32, 32), None, 255, True, "x30"),
]


@pytest.mark.parametrize("B,C,lo,size,n_lab,ign,align,mode", WIDE_CASES)
def test_wide_cross_entropy_from_lowres_logits(B, C, lo, size, n_lab, ign, align, mode):
    H, W = size
    low, y, low_d = _inputs(B, C, lo, size, H * W if n_lab is None else n_lab, ign, mode)
    ref_loss, ref_grad = _reference64(low, y, size, ign, align)
    yd = y.to(DEV)
    loss, dlow = E.cross_entropy_lowres(low_d, size, yd, ign, align_corners=align)
    print(f"loss {loss.item():.9g} vs float64 {ref_loss:.9g}: err {abs(loss.item() - ref_loss):.3e}")
    assert abs(loss.item() - ref_loss) < 1e-5 * max(1.0, abs(ref_loss))
    close(dlow.permute(0, 3, 1, 2), ref_grad, tol=2e-5, what="dlow vs float64 autograd")
    # dense product path
    tape = E.Tape(True)
    lv = E.Var(low_d.contiguous())
    pred = E.bilinear(tape, lv, size, align, 0.0, out_nchw=True)
    loss2, dl = E.cross_entropy_nchw(pred.t, yd, ign)
    tape.backward(pred, dl)
    assert abs(loss.item() - loss2.item()) < 2e-6 * max(1.0, abs(loss2.item()))
    close(dlow, lv.grad, tol=1e-5, what="dlow vs dense path")
    # fixed-order gather: bitwise reproducible
    loss3, dlow3 = E.cross_entropy_lowres(low_d, size, yd, ign, align_corners=align)
    assert torch.equal(loss3, loss) and torch.equal(dlow3, dlow)
    # densely labelled mode: the same kernels, the same bits
    loss4, dlow4 = E.cross_entropy_lowres(low_d, size, yd, ign, align_corners=align, sparse=False)
    assert torch.equal(loss4, loss) and torch.equal(dlow4, dlow)
    assert getattr(dlow4, "_pp_rowflags", None) is None


def test_wide_cross_entropy_without_labels_is_nan():
    low = torch.randn(1, 8, 8, 150, device=DEV)
    y = torch.full((1, 32, 32), 255, dtype=torch.int64, device=DEV)
    loss, dlow = E.cross_entropy_lowres(low, (32, 32), y, 255)
    assert torch.isnan(loss).all()                     # 0/0 like F.cross_entropy


def test_wide_cross_entropy_honours_grad_out_and_count():
    """grad_out scales dlow, *count is the number of labelled pixels, and a loss-only call (dlow NULL) gives the same loss."""
    low, y, low_d = _inputs(1, 150, (8, 8), (32, 32), 50, 255, "")
    yd = y.to(DEV)
    loss, dlow = E.cross_entropy_lowres(low_d, (32, 32), yd, 255)
    loss_only, none = E.cross_entropy_lowres(low_d, (32, 32), yd, 255, want_grad=False)
    assert none is None and torch.equal(loss_only, loss)
    L = _lib.lib()
    ws = torch.empty(L.pp_sparse_ce_lowres_workspace_bytes(), dtype=torch.uint8, device=DEV)
    out = torch.zeros(2, device=DEV)
    g = torch.full((1,), 0.25, device=DEV)
    d2 = torch.full((1, 8, 8, 153), 7.0, device=DEV)                   # lddx > C: the three spare channels stay untouched
    rc = L.pp_sparse_ce_lowres_fwd_bwd(low_d.data_ptr(), low_d.stride(2), 1, 150, 8, 8, 32, 32, 1, yd.data_ptr(), 255, out.data_ptr(),
                                       out[1:].data_ptr(), g.data_ptr(), d2.data_ptr(), 153, ws.data_ptr(), ws.numel(),
                                       _lib.current_stream_ptr())
    _lib.check(rc, "pp_sparse_ce_lowres_fwd_bwd")
    assert out[1].item() == 50 and out[0].item() == loss.item()
    assert (d2[..., 150:] == 7.0).all()
    close(d2[..., :150], dlow * 0.25, tol=1e-6, what="grad_out")


@pytest.mark.parametrize("C", [19, 21, 40, 64])
def test_streamed_kernels_agree_with_the_register_kernels(C):
    """The test build's pp_debug_set_ce_stream forces the streamed kernels onto narrow heads, where the register kernels are the
    well-tested yardstick."""
    low, y, low_d = _inputs(2, C, (9, 13), (33, 47), 200, 255, "")
    yd = y.to(DEV)
    L = _lib.lib()
    loss_r, dlow_r = E.cross_entropy_lowres(low_d, (33, 47), yd, 255)
    L.pp_debug_launch_log(None, 0)
    try:
        L.pp_debug_set_ce_stream(1)
        loss_s, dlow_s = E.cross_entropy_lowres(low_d, (33, 47), yd, 255)
        cbuf = ctypes.create_string_buffer(4096)
        L.pp_debug_launch_log(cbuf, 4096)
        names = cbuf.value.decode()
    finally:
        L.pp_debug_set_ce_stream(0)
    assert "ce_lowres_stream_partial_kernel" in names and "ce_lowres_stream_bwd_kernel" in names, names
    assert abs(loss_s.item() - loss_r.item()) < 2e-6 * max(1.0, abs(loss_r.item()))
    close(dlow_s, dlow_r, tol=1e-5, what="streamed vs register kernels")
