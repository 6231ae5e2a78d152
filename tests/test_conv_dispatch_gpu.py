"""Every branch of the convolution dispatcher (csrc/conv_igemm.hip: launch_conv, the strided backward-data phases, the ASPP multi-branch
backward-data, the weight-gradient launchers) against a float64 CPU reference, at a shape that REACHES that branch.  The test build's
launch log (pp_debug_launch_log) names the kernels each call launched; every row states the kernel it was written for, so a new branch
put in front of the others cannot quietly move a row to another kernel.

Rows carry the entry point, the geometry (B, H, W, Cin, Cout, k, stride, pad, dil), planner knobs and the kernel the log must hold.
test_every_dispatched_kernel_is_reached holds the union of the logged names to EXPECTED; tests/test_host_logic.py holds every kernel
name the dispatcher can log to EXPECTED or to ELSEWHERE (the test that covers it there, or why no test does).

Single-tap problems whose tap is not weight tap 0 are the edge that matters most here: the 3x3 stride-2 backward-data phase (0, 0)
(ResNet50 layer2.0.conv2 at 256x512, widx 4) and a dilation wider than the map keep only the centre tap; a stride-3 phase keeps one
tap at a non-zero offset, which the pointwise GEMM (gemm_pw.hip) must refuse."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pixelpick_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# fp32-accumulation bars (rel-L2, and max error over the reference's largest magnitude, both vs float64), about 3-4x the worst row
# of each class measured on an MI355X: fp32 kernels 6.1e-7 / 1.6e-6, bf16x3 kernels 5.2e-7 / 1.4e-6, weight gradients 2.3e-7 / 3.4e-7.
# A wrong tap, offset or weight pointer gives errors of O(0.1 - 1).
TOL = {"fp32": (2e-6, 6e-6), "x3": (2e-6, 5e-6), "wgrad": (1e-6, 1.5e-6)}

# name -> (setter, default) of the planner knobs a row may set; every row puts them back in a finally
KNOBS = {"x3": ("pp_debug_set_x3", 1), "gemm_pw": ("pp_debug_set_gemm_pw", 1), "variant": ("pp_debug_set_conv_variant", 0)}
DMA_OFF = 256 | 262144              # pp_debug_set_conv_variant: LDS-DMA kernels of the 128-row and the 64x64 tiles off
BK32 = 4096                         # 32-deep K step of the 128x128 tiles
WGRAD_DMA64 = 1 << 21               # LDS-DMA weight-gradient kernel of the 64x64 tiles on


def _case(cid, op, geom, expect, knobs=None, tol="fp32", **opt):
    return pytest.param(dict(op=op, geom=geom, expect=expect, knobs=knobs or {}, tol=tol, opt=opt), id=cid)


CASES = [
    # a. the finding: FPN layer2.0.conv2 (128 -> 128, 3x3, stride 2) backward-data at 256x512; phase (0, 0) keeps only the centre tap
    #    (widx 4) and has 4096 / 8192 rows: the pointwise GEMM
    _case("a-l2conv2-B2", "bwd_data", (2, 64, 128, 128, 128, 3, 2, 1, 1), {"gemm_pw_kernel", "bwd_phase_interleave_kernel"}),
    _case("a-l2conv2-B4", "bwd_data", (4, 64, 128, 128, 128, 3, 2, 1, 1), {"gemm_pw_kernel", "bwd_phase_interleave_kernel"}),
    _case("a-l2conv2-B2-accumulate", "bwd_data", (2, 64, 128, 128, 128, 3, 2, 1, 1), {"gemm_pw_kernel"}, accumulate=True),
    _case("a-l2conv2-B2-slice", "bwd_data", (2, 64, 128, 128, 128, 3, 2, 1, 1), {"gemm_pw_kernel"}, slice=(160, 16)),
    # b. pad 0: phase (1, 1) holds the single centre tap, 2 x 32 x 64 rows
    _case("b-s2-pad0", "bwd_data", (2, 65, 129, 128, 128, 3, 2, 0, 1), {"gemm_pw_kernel", "bwd_phase_interleave_kernel"}),
    # c. dilation 12 on an 8x8 map: only the centre tap is live (64 x 64 = 4096 rows)
    _case("c-dil12-fwd-x3off", "fwd", (64, 8, 8, 128, 128, 3, 1, 12, 12), {"gemm_pw_kernel"}, knobs={"x3": 0}),
    _case("c-dil12-fwd", "fwd", (64, 8, 8, 128, 128, 3, 1, 12, 12), set()),
    _case("c-dil12-bwd-x3off", "bwd_data", (64, 8, 8, 128, 128, 3, 1, 12, 12), {"gemm_pw_kernel"}, knobs={"x3": 0}),
    _case("c-dil12-bwd", "bwd_data", (64, 8, 8, 128, 128, 3, 1, 12, 12), set()),
    _case("c-dil12-wgrad", "bwd_weight", (64, 8, 8, 128, 128, 3, 1, 12, 12), {"conv_wgrad_dma_kernel"}, tol="wgrad", nan_fill=True),
    # d. one live tap at a non-zero offset (3x3 stride-3 phase (2, 2): dh = dw = +1; a 1x1 conv with the folded padding: -1): every
    #    single-tap kernel but the pointwise GEMM
    _case("d-s3-rows", "bwd_data", (16, 96, 96, 32, 64, 3, 3, 1, 1), {"conv1x1_rows_kernel"}),
    _case("d-s3-ksplit", "bwd_data", (4, 96, 96, 128, 256, 3, 3, 1, 1), {"conv1x1_ksplit_dma_kernel"}),
    _case("d-s3-tiled", "bwd_data", (8, 96, 96, 128, 128, 3, 3, 1, 1), {"conv_igemm_dma_kernel<64x64>"}),
    _case("d-1x1pad1-fwd", "fwd", (4, 30, 30, 128, 128, 1, 1, 1, 1), {"conv_igemm_dma_kernel<64x64>"}),
    _case("d-1x1pad1-bwd", "bwd_data", (4, 30, 30, 128, 128, 1, 1, 1, 1), {"conv_igemm_dma_kernel<64x64>"}),
    # f. the remaining branches, forward and backward where the branch has both
    _case("f-widen-fwd", "fwd", (2, 128, 160, 16, 96, 1, 1, 0, 1), {"conv1x1_fwd_widen_kernel"}),
    _case("f-widen-bwd", "bwd_data", (2, 128, 136, 96, 24, 1, 1, 0, 1), {"conv1x1_fwd_widen_kernel<bwd>"}),
    _case("f-rows-fwd", "fwd", (2, 128, 160, 32, 16, 1, 1, 0, 1), {"conv1x1_rows_kernel"}),
    _case("f-rows-bwd", "bwd_data", (2, 128, 160, 16, 96, 1, 1, 0, 1), {"conv1x1_rows_kernel"}),
    _case("f-stem-fwd", "fwd", (2, 256, 264, 3, 32, 3, 2, 1, 1), {"conv_stem3x3s2_fwd_kernel"}),
    _case("f-ksplit-fwd", "fwd", (4, 16, 32, 1280, 256, 1, 1, 0, 1), {"conv1x1_ksplit_dma_kernel"}),
    _case("f-gemm_pw-fwd", "fwd", (4, 32, 64, 256, 1024, 1, 1, 0, 1), {"gemm_pw_kernel"}),
    _case("f-gemm_pw-bwd", "bwd_data", (4, 32, 64, 256, 1024, 1, 1, 0, 1), {"gemm_pw_kernel"}),
    _case("f-x3-fwd", "fwd", (2, 96, 128, 128, 256, 3, 1, 1, 1), {"x3_split_kernel", "x3_split_w_kernel", "conv_x3_kernel"}, tol="x3"),
    _case("f-x3-bwd", "bwd_data", (2, 96, 128, 256, 128, 3, 1, 1, 1), {"x3_split_kernel", "x3_split_w_kernel", "conv_x3_kernel"}, tol="x3"),
    _case("f-x3-fwd-pre2", "fwd_pre2", (2, 96, 128, 128, 256, 3, 1, 1, 1), {"conv_x3_kernel"}, tol="x3"),
    _case("f-x3-bwd-pre2", "bwd_data_pre2", (2, 96, 128, 256, 128, 3, 1, 1, 1), {"conv_x3_kernel"}, tol="x3"),
    _case("f-dma128-fwd", "fwd", (2, 96, 128, 128, 256, 3, 1, 1, 1), {"conv_igemm_dma_kernel<128x128>"}, knobs={"x3": 0}),
    _case("f-dma128-bwd", "bwd_data", (2, 96, 128, 256, 128, 3, 1, 1, 1), {"conv_igemm_dma_kernel<128x128>"}, knobs={"x3": 0}),
    _case("f-dma128x64-fwd", "fwd", (2, 96, 128, 64, 304, 3, 1, 1, 1), {"conv_igemm_dma_kernel<128x64>"}, knobs={"x3": 0}),
    _case("f-dma128x64-bwd", "bwd_data", (2, 96, 128, 304, 64, 3, 1, 1, 1), {"conv_igemm_dma_kernel<128x64>"}, knobs={"x3": 0}),
    _case("f-dma64-fwd", "fwd", (2, 32, 64, 64, 64, 3, 1, 1, 1), {"conv_igemm_dma_kernel<64x64>"}),
    _case("f-dma64-bwd", "bwd_data", (2, 32, 64, 64, 64, 3, 1, 1, 1), {"conv_igemm_dma_kernel<64x64>"}),
    _case("f-reg128x32-fwd", "fwd", (2, 32, 64, 64, 32, 3, 1, 1, 1), {"conv_igemm_kernel<128x32>"}),
    _case("f-reg128x32-bwd", "bwd_data", (2, 32, 64, 32, 64, 3, 1, 1, 1), {"conv_igemm_kernel<128x32>"}),
    _case("f-reg128-fwd", "fwd", (2, 96, 128, 128, 256, 3, 1, 1, 1), {"conv_igemm_kernel<128x128>"}, knobs={"x3": 0, "variant": DMA_OFF}),
    _case("f-reg128-bwd", "bwd_data", (2, 96, 128, 256, 128, 3, 1, 1, 1), {"conv_igemm_kernel<128x128>"}, knobs={"x3": 0, "variant": DMA_OFF}),
    _case("f-reg128x64-fwd", "fwd", (2, 96, 128, 64, 304, 3, 1, 1, 1), {"conv_igemm_kernel<128x64>"}, knobs={"x3": 0, "variant": DMA_OFF}),
    _case("f-reg64-fwd", "fwd", (2, 32, 64, 64, 64, 3, 1, 1, 1), {"conv_igemm_kernel<64x64>"}, knobs={"variant": DMA_OFF}),
    _case("f-reg64-bwd", "bwd_data", (2, 32, 64, 64, 64, 3, 1, 1, 1), {"conv_igemm_kernel<64x64>"}, knobs={"variant": DMA_OFF}),
    _case("f-bk64-fwd", "fwd", (1, 64, 64, 256, 64, 3, 1, 1, 1), {"conv_igemm_kernel<64x64 bk64>", "splitk_reduce_kernel"},
          knobs={"variant": DMA_OFF}),
    _case("f-bk32-fwd", "fwd", (2, 96, 128, 128, 256, 3, 1, 1, 1), {"conv_igemm_kernel<128x128 bk32>"}, knobs={"x3": 0, "variant": BK32}),
    _case("f-splitk-fwd", "fwd", (2, 16, 32, 320, 256, 3, 1, 6, 6), {"conv_igemm_dma_kernel<64x64>", "splitk_reduce_kernel"}),
    _case("f-splitk-bwd", "bwd_data", (2, 16, 32, 320, 256, 3, 1, 6, 6), {"conv_igemm_dma_kernel<64x64>", "splitk_reduce_kernel"}),
    _case("f-aspp-multi", "bwd_data_multi", (2, 16, 24, 64, 32), {"conv_igemm_dma_kernel<multi>"}, accumulate=True),
    _case("f-wgrad-narrow-in", "bwd_weight", (2, 128, 160, 16, 96, 1, 1, 0, 1), {"wgrad_narrow_in_kernel", "wgrad_reduce_wide_kernel"},
          tol="wgrad"),
    _case("f-wgrad-narrow-out", "bwd_weight", (2, 128, 136, 96, 24, 1, 1, 0, 1), {"wgrad_narrow_out_kernel", "bias_grad_final_kernel"},
          tol="wgrad", bias=True),
    _case("f-wgrad-stem3", "bwd_weight", (2, 256, 264, 3, 32, 3, 2, 1, 1), {"wgrad_stem3x3s2_kernel"}, tol="wgrad"),
    _case("f-wgrad-stem7", "bwd_weight", (2, 256, 264, 3, 64, 7, 2, 3, 1), {"wgrad_stem7x7s2_kernel"}, tol="wgrad"),
    _case("f-wgrad-dma", "bwd_weight", (2, 32, 64, 128, 128, 3, 1, 1, 1), {"conv_wgrad_dma_kernel", "wgrad_reduce_kernel"}, tol="wgrad"),
    _case("f-wgrad-dma64", "bwd_weight", (2, 32, 64, 64, 64, 3, 1, 1, 1), {"conv_wgrad_dma_kernel<64x64>"}, knobs={"variant": WGRAD_DMA64},
          tol="wgrad"),
    _case("f-wgrad-reg-bias", "bwd_weight", (2, 32, 64, 64, 64, 3, 1, 1, 1), {"conv_wgrad_kernel", "bias_grad_final_kernel"}, tol="wgrad",
          bias=True),
    _case("f-wgrad-x3-bias", "bwd_weight", (2, 96, 128, 128, 256, 3, 1, 1, 1),
          {"x3_split_kernel", "conv_wgrad_x3_kernel", "bias_grad_partial_kernel", "bias_grad_final_kernel"}, tol="x3", bias=True),
]

# every kernel name the rows above log between them (tests/test_host_logic.py: with ELSEWHERE, every name the dispatcher can log)
EXPECTED = {
    "gemm_pw_kernel", "bwd_phase_interleave_kernel", "conv1x1_rows_kernel", "conv1x1_ksplit_dma_kernel", "conv1x1_fwd_widen_kernel",
    "conv1x1_fwd_widen_kernel<bwd>", "conv_stem3x3s2_fwd_kernel", "x3_split_kernel", "x3_split_w_kernel", "conv_x3_kernel",
    "conv_igemm_dma_kernel<128x128>", "conv_igemm_dma_kernel<128x64>", "conv_igemm_dma_kernel<64x64>", "conv_igemm_kernel<128x32>",
    "conv_igemm_kernel<128x128>", "conv_igemm_kernel<128x64>", "conv_igemm_kernel<64x64>", "conv_igemm_kernel<64x64 bk64>",
    "conv_igemm_kernel<128x128 bk32>", "splitk_reduce_kernel", "conv_igemm_dma_kernel<multi>", "wgrad_narrow_in_kernel",
    "wgrad_narrow_out_kernel", "wgrad_stem3x3s2_kernel", "wgrad_stem7x7s2_kernel", "wgrad_reduce_wide_kernel", "conv_wgrad_dma_kernel",
    "conv_wgrad_dma_kernel<64x64>", "conv_wgrad_kernel", "conv_wgrad_x3_kernel", "wgrad_reduce_kernel", "bias_grad_final_kernel",
    "bias_grad_partial_kernel",
}
# names the dispatcher can log that no row above reaches: the test that covers each, or why none does
ELSEWHERE = {
    "conv_igemm_kernel<bn>": "tests/test_nn_ops_gpu.py::test_conv_batchnorm_in_one_launch (every fused forward form)",
    "conv1x1_ksplit_dma_kernel<bn>": "tests/test_nn_ops_gpu.py::test_conv_batchnorm_in_one_launch",
    "conv_igemm_kernel<bn bwd>": "tests/test_nn_ops_gpu.py::test_batchnorm_backward_inside_the_consumer_convolutions_backward_data",
    "conv_igemm_dma_kernel<bn bwd>": "tests/test_nn_ops_gpu.py::test_batchnorm_backward_inside_the_consumer_convolutions_backward_data",
    "conv1x1_ksplit_dma_kernel<bn bwd>": "tests/test_nn_ops_gpu.py::test_batchnorm_backward_inside_the_last_consumers_backward_data",
    "splitk_reduce_stats_kernel": "tests/test_nn_ops_gpu.py::test_conv_epilogue_statistics_feed_the_batchnorm",
    "wgrad_reduce_batch_kernel": "tests/test_nn_ops_gpu.py::test_batched_weight_gradient_reduces_are_bit_identical",
    "mfma_stream_kernel": "a timing yardstick (pp_yardstick_mfma_stream): computes nothing to compare",
}


def launch_log():
    """The names logged since the previous call (and clears the log)."""
    buf = ctypes.create_string_buffer(1 << 20)
    n = int(_lib.lib().pp_debug_launch_log(buf, len(buf)))
    assert n < len(buf), "launch log cut short"
    return [s for s in buf.value.decode().split(";") if s]


def _geom_out(H, W, k, s, p, d):
    return (H + 2 * p - d * (k - 1) - 1) // s + 1, (W + 2 * p - d * (k - 1) - 1) // s + 1


def _ws(nb):
    return torch.empty(max(int(nb), 256), dtype=torch.uint8, device=DEV), int(nb)


def _ptr(t):
    return t.data_ptr() if t is not None else None


ASPP = [(1, 1), (3, 6), (3, 12), (3, 18)]      # (kernel size, dilation) of the four branches (aspp.py:49-57)


def _run(c, seed=0):
    """Builds the row's operands (NHWC / HWIO on the GPU), launches it, returns (result tensors, fp64 reference thunk, logged names)."""
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    op, opt = c["op"], c["opt"]
    gen = torch.Generator(device=DEV).manual_seed(1234 + seed)
    if op == "bwd_data_multi":
        B, H, W, Cin, Cout = c["geom"]
        nb = len(ASPP)
        ws_ = [torch.randn(k, k, Cin, Cout, device=DEV, generator=gen) / np.sqrt(k * k * Cout) for k, _ in ASPP]
        dbuf = torch.randn(B, H, W, nb * Cout + 8, device=DEV, generator=gen)[..., :nb * Cout]
        base = torch.randn(B, H, W, Cin, device=DEV, generator=gen)
        dx = base.clone()
        ws, nws = _ws(L.pp_conv2d_bwd_data_multi_workspace_bytes(B, H, W, Cin, Cout, nb, *[v for kd in ASPP for v in kd]))
        assert nws > 0
        args = []
        for (k, d), w in zip(ASPP, ws_):
            args += [w.data_ptr(), k, d]
        launch_log()
        _lib.check(L.pp_conv2d_bwd_data_multi(dbuf.data_ptr(), dbuf.stride(2), B, H, W, Cout, nb, *args, dx.data_ptr(), Cin, Cin, 1,
                                              ws.data_ptr(), nws, st), "pp_conv2d_bwd_data_multi")
        torch.cuda.synchronize()
        names = launch_log()

        def ref():
            r = base.double().cpu().permute(0, 3, 1, 2)
            for b, ((k, d), w) in enumerate(zip(ASPP, ws_)):
                dyb = dbuf[..., b * Cout:(b + 1) * Cout].double().cpu().permute(0, 3, 1, 2)
                r = r + torch.nn.grad.conv2d_input((B, Cin, H, W), w.double().cpu().permute(3, 2, 0, 1), dyb, 1, d * (k - 1) // 2, d)
            return {"dx": r.permute(0, 2, 3, 1)}
        return {"dx": dx}, ref, names

    B, H, W, Cin, Cout, k, s, p, d = c["geom"]
    Ho, Wo = _geom_out(H, W, k, s, p, d)
    x = torch.randn(B, H, W, Cin, device=DEV, generator=gen)
    w = torch.randn(k, k, Cin, Cout, device=DEV, generator=gen) / np.sqrt(k * k * Cin)
    dy = torch.randn(B, Ho, Wo, Cout, device=DEV, generator=gen)
    out = {}

    def xd():
        return x.double().cpu().permute(0, 3, 1, 2)

    def wd():
        return w.double().cpu().permute(3, 2, 0, 1)

    def dyd():
        return dy.double().cpu().permute(0, 3, 1, 2)

    if op in ("fwd", "fwd_pre2"):
        y = torch.full((B, Ho, Wo, Cout), float("nan"), device=DEV)
        ws, nws = _ws(L.pp_conv2d_fwd_workspace_bytes(B, H, W, Cin, Cout, k, k, s, p, d))
        if op == "fwd_pre2":
            na = int(L.pp_conv2d_x3_planes_bytes(0, B, H, W, Cin, Cout, k, k, s, p, d))
            nw = int(L.pp_conv2d_x3_planes_bytes(3, B, H, W, Cin, Cout, k, k, s, p, d))
            assert na > 0 and nw > 0, "the row's shape takes no planes"
            xp = torch.empty(na, dtype=torch.uint8, device=DEV)
            wp = torch.empty(nw, dtype=torch.uint8, device=DEV)
            _lib.check(L.pp_x3_split(x.data_ptr(), Cin, B * H * W, Cin, xp.data_ptr(), na, st), "pp_x3_split")
            _lib.check(L.pp_x3_split_weights(w.data_ptr(), k * k, Cin, Cout, 1, wp.data_ptr(), nw, st), "pp_x3_split_weights")
            launch_log()
            rc = L.pp_conv2d_fwd_pre2(x.data_ptr(), Cin, B, H, W, Cin, w.data_ptr(), None, k, k, s, p, d, y.data_ptr(), Cout, Cout,
                                      ws.data_ptr(), nws, xp.data_ptr(), wp.data_ptr(), st)
        else:
            launch_log()
            rc = L.pp_conv2d_fwd(x.data_ptr(), Cin, B, H, W, Cin, w.data_ptr(), None, k, k, s, p, d, y.data_ptr(), Cout, Cout,
                                 ws.data_ptr(), nws, st)
        _lib.check(rc, op)
        out["y"] = y

        def ref():
            return {"y": F.conv2d(xd(), wd(), None, s, p, d).permute(0, 2, 3, 1)}
    elif op in ("bwd_data", "bwd_data_pre2"):
        lddx, off = opt.get("slice", (Cin, 0))
        buf = torch.full((B, H, W, lddx), 7.0, device=DEV)
        dx = buf[..., off:off + Cin]
        base = None
        if opt.get("accumulate"):
            base = torch.randn(B, H, W, Cin, device=DEV, generator=gen)
            dx.copy_(base)
        ws, nws = _ws(L.pp_conv2d_bwd_data_workspace_bytes(B, H, W, Cin, Cout, k, k, s, p, d))
        acc = 1 if base is not None else 0
        if op == "bwd_data_pre2":
            na = int(L.pp_conv2d_x3_planes_bytes(1, B, H, W, Cin, Cout, k, k, s, p, d))
            nw = int(L.pp_conv2d_x3_planes_bytes(4, B, H, W, Cin, Cout, k, k, s, p, d))
            assert na > 0 and nw > 0, "the row's shape takes no planes"
            dp = torch.empty(na, dtype=torch.uint8, device=DEV)
            wp = torch.empty(nw, dtype=torch.uint8, device=DEV)
            _lib.check(L.pp_x3_split(dy.data_ptr(), Cout, B * Ho * Wo, Cout, dp.data_ptr(), na, st), "pp_x3_split")
            _lib.check(L.pp_x3_split_weights(w.data_ptr(), k * k, Cin, Cout, 0, wp.data_ptr(), nw, st), "pp_x3_split_weights")
            launch_log()
            rc = L.pp_conv2d_bwd_data_pre2(dy.data_ptr(), Cout, B, Ho, Wo, Cout, w.data_ptr(), k, k, s, p, d, dx.data_ptr(), lddx, H, W, Cin,
                                           acc, ws.data_ptr(), nws, dp.data_ptr(), wp.data_ptr(), st)
        else:
            launch_log()
            rc = L.pp_conv2d_bwd_data(dy.data_ptr(), Cout, B, Ho, Wo, Cout, w.data_ptr(), k, k, s, p, d, dx.data_ptr(), lddx, H, W, Cin, acc,
                                      ws.data_ptr(), nws, st)
        _lib.check(rc, op)
        out["dx"] = dx
        out["guard"] = torch.cat([buf[..., :off], buf[..., off + Cin:]], dim=-1)

        def ref():
            r = torch.nn.grad.conv2d_input((B, Cin, H, W), wd(), dyd(), s, p, d).permute(0, 2, 3, 1)
            return {"dx": r + base.double().cpu() if base is not None else r}
    elif op == "bwd_weight":
        dw = torch.full((k, k, Cin, Cout), float("nan") if opt.get("nan_fill") else 0.0, device=DEV)
        db = torch.full((Cout,), float("nan"), device=DEV) if opt.get("bias") else None
        ws, nws = _ws(L.pp_conv2d_bwd_weight_workspace_bytes(B, H, W, Cin, Cout, k, k, s, p, d))
        launch_log()
        _lib.check(L.pp_conv2d_bwd_weight(x.data_ptr(), Cin, B, H, W, Cin, dy.data_ptr(), Cout, Cout, k, k, s, p, d, dw.data_ptr(), _ptr(db),
                                          ws.data_ptr(), nws, st), op)
        out["dw"] = dw
        if db is not None:
            out["db"] = db

        def ref():
            r = {"dw": torch.nn.grad.conv2d_weight(xd(), (Cout, Cin, k, k), dyd(), s, p, d).permute(2, 3, 1, 0)}
            if db is not None:
                r["db"] = dy.double().cpu().sum(dim=(0, 1, 2))
            return r
    else:
        raise AssertionError(op)
    torch.cuda.synchronize()
    return out, ref, launch_log()


def _errors(got, ref):
    dlt = got.double().cpu() - ref
    return (dlt.norm() / ref.norm()).item(), (dlt.abs().max() / ref.abs().max()).item()


def _set_knobs(knobs):
    L = _lib.lib()
    for name, v in knobs.items():
        getattr(L, KNOBS[name][0])(v)


def _reset_knobs(knobs):
    L = _lib.lib()
    for name in knobs:
        setter, default = KNOBS[name]
        getattr(L, setter)(default)


@pytest.mark.parametrize("c", CASES)
def test_dispatch_branch_matches_float64(c):
    _set_knobs(c["knobs"])
    try:
        out, ref, names = _run(c)
    finally:
        _reset_knobs(c["knobs"])
    r = ref()
    tl2, tmax = TOL[c["tol"]]
    msg = []
    for key, want in r.items():
        e2, emax = _errors(out[key], want)
        msg.append(f"{key} rel-l2 {e2:.2e} max-rel {emax:.2e}")
        assert e2 <= tl2 and emax <= tmax, f"{key}: rel-l2 {e2:.3e} (bar {tl2:g}), max-rel {emax:.3e} (bar {tmax:g}); kernels {names}"
    print(f"\n[dispatch] {' | '.join(msg)} | {';'.join(sorted(set(names)))}")
    missing = c["expect"] - set(names)
    assert not missing, f"the row did not reach {sorted(missing)}: it launched {names}"
    if "guard" in out:
        assert bool((out["guard"] == 7.0).all()), "backward-data wrote outside its channel slice"
    if c["opt"].get("nan_fill"):
        k = c["geom"][5]
        live = torch.zeros(k, k, dtype=torch.bool)
        live[k // 2, k // 2] = True
        assert bool((out["dw"][~live.to(DEV)] == 0).all()), "the dead taps' weight gradient must be exactly 0"


def test_every_gemm_pw_tile_form_on_the_centre_tap_phase():
    """Row a with each tile form of the pointwise GEMM forced (from one row on): the SAME bits, as for the 1x1 layers
    (tests/test_gemm_pw_gpu.py), and the fp64 result."""
    L = _lib.lib()
    c = dict(op="bwd_data", geom=(2, 64, 128, 128, 128, 3, 2, 1, 1), expect={"gemm_pw_kernel"}, knobs={}, tol="fp32", opt={})
    outs = []
    try:
        for form in range(6):
            L.pp_debug_set_gemm_pw((2 + form) | (1 << 4))
            out, ref, names = _run(c)
            assert "gemm_pw_kernel" in names, (form, names)
            outs.append(out["dx"])
    finally:
        L.pp_debug_set_gemm_pw(1)
    r = ref()["dx"]
    e2, emax = _errors(outs[0], r)
    print(f"\n[dispatch] gemm_pw forms on the widx-4 phase: rel-l2 {e2:.2e} max-rel {emax:.2e}")
    assert e2 <= TOL["fp32"][0] and emax <= TOL["fp32"][1]
    for form in range(1, 6):
        assert torch.equal(outs[0], outs[form]), f"form {form} differs from form 0"


def test_every_dispatched_kernel_is_reached():
    """The union of the kernels the table's rows launch is EXPECTED: a kernel no row reaches any more (a branch moved in front) or a
    new one no row was written for fails here."""
    seen = set()
    for prm in CASES:
        c = prm.values[0]
        _set_knobs(c["knobs"])
        try:
            _, _, names = _run(c)
        finally:
            _reset_knobs(c["knobs"])
        seen |= set(names)
    assert seen == EXPECTED, f"not reached: {sorted(EXPECTED - seen)}; not listed: {sorted(seen - EXPECTED)}"
