"""GPU tests that the planner switches REACH the source that reads them.  The acquisition stages live in separate sources (csrc/acq.hip,
acq_topk.hip, acq_lowres.hip, acq_mc.hip) and the switches are one object defined in a fifth (acq_knobs.hip): a copy of that state per
source would let a pp_debug_set_* call miss its reader silently, and every A/B test would compare a path with itself.  Each case sets one
switch, makes one call and holds the test build's launch log (the names recorded where each launch is checked) to the sequence of kernels
that switch must produce; the reference-order cases hold the per-call flag to the process switch, bit for bit."""
import ctypes

import pytest
import torch

from pixelpick_amd import _lib
from pixelpick_amd import acquisition as acq

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 19


def _launches():
    """The names of the kernels launched since the previous call, in order."""
    b = ctypes.create_string_buffer(1 << 16)
    assert int(_lib.lib().pp_debug_launch_log(b, len(b))) < len(b), "launch log cut short"
    return [s.strip() for s in b.value.decode().split(";") if s.strip()]


def _logged(call, reduce_mode=0, tuning=0):
    """The launch log of ONE call made with the two switches set; both are restored whatever happens."""
    L = _lib.lib()
    try:
        L.pp_debug_set_reduce_mode(reduce_mode)
        L.pp_debug_set_acq_tuning(tuning, 0)
        torch.cuda.synchronize()
        L.pp_debug_launch_log(None, 0)   # drain: whatever earlier tests left in the log, of any length
        call()
        torch.cuda.synchronize()
        return _launches()
    finally:
        L.pp_debug_set_reduce_mode(0)
        L.pp_debug_set_acq_tuning(0, 0)


def _logits(H, W, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn((1, C, H, W), device=DEV, generator=g) * 3


def _low(h, w, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn((1, h, w, C), device=DEV, generator=g) * 3


# pp_acq_score_topk, B = 1, C = 19, 128 x 128 contiguous NCHW, entropy, k = 64, no out_map: the smallest size the list route takes
# (N >= 16384, 8 k <= N, k > 48)
@pytest.mark.parametrize("mode, want", [
    (0, ["acq_sample_thr_kernel", "acq_kernel<emit>", "topk_lsel_kernel"]),
    (2048, ["acq_kernel<hist>", "topk_qsel_kernel", "topk_large_kernel"]),
    (2048 | 1024, ["acq_kernel", "select_qhist_kernel", "topk_qsel_kernel", "topk_large_kernel"]),
    (2048 | 512, ["acq_kernel"] + ["select_hist_kernel"] * 4 + ["topk_large_sel_kernel"]),
    (2048 | 512 | 256, ["acq_kernel", "topk_large_kernel"]),
])
def test_reduce_mode_reaches_the_full_size_scorer_and_the_map_select(mode, want):
    x = _logits(128, 128)
    assert _logged(lambda: acq.score_topk(x, None, "entropy", 64), reduce_mode=mode) == want


# pp_topk_select on a 16 384-element map, k = 64
@pytest.mark.parametrize("mode, want", [
    (0, ["select_minmax_kernel", "select_qhist_kernel", "topk_qsel_kernel", "topk_large_kernel"]),
    (1 << 22, ["select_hist_kernel"] * 4 + ["topk_large_sel_kernel"]),
])
def test_reduce_mode_reaches_topk_select(mode, want):
    g = torch.Generator(device=DEV).manual_seed(1)
    s = torch.rand((1, 16384), device=DEV, generator=g)
    assert _logged(lambda: acq.topk_select(s, 64, True), reduce_mode=mode) == want


# pp_acq_lowres_score_topk, 16 x 16 -> 64 x 64, C = 19, k = 64
@pytest.mark.parametrize("mode, want", [
    (0, ["acq_lowres_kernel", "topk_qsel_kernel", "topk_large_kernel"]),
    (1024, ["acq_lowres_kernel", "select_qhist_kernel", "topk_qsel_kernel", "topk_large_kernel"]),
])
def test_reduce_mode_reaches_the_low_resolution_scorer(mode, want):
    low = _low(16, 16)
    assert _logged(lambda: acq.score_topk_lowres(low, (64, 64), None, "entropy", 64), reduce_mode=mode) == want


def test_tuning_reaches_every_streamed_scorer():
    """pp_debug_set_acq_tuning(10, 0): the streamed class vector at any class count, in the full-size and the low-resolution sources."""
    x, low = _logits(64, 64), _low(16, 16)
    ii = torch.zeros(5, dtype=torch.int32)
    pp = torch.tensor([0, 1, 63, 64, 4095], dtype=torch.int32)
    for call, want in ((lambda: acq.score_map(x, None, "entropy"), "acq_stream_kernel"),
                       (lambda: acq.score_topk_lowres(low, (64, 64), None, "entropy", 0), "acq_lowres_stream_kernel"),
                       (lambda: acq.score_at_lowres(low, (64, 64), ii, pp), "acq_lowres_at_stream_kernel"),
                       (lambda: acq.prob_at_lowres(low, (64, 64), ii, pp), "prob_at_stream_kernel")):
        assert _logged(call, tuning=10) == [want]
        assert _logged(call) != [want], "the default plan must not be the streamed one: the case would prove nothing"


def _lowres_map(low, strategy_word):
    """pp_acq_lowres_score_topk with k = 0 (map only), 16 x 16 -> 64 x 64, the strategy word passed as it is."""
    B, h, w, _ = low.shape
    omap = torch.empty((B, 64, 64), dtype=torch.float32, device=DEV)
    with torch.cuda.device(DEV):
        rc = _lib.lib().pp_acq_lowres_score_topk(low.data_ptr(), low.stride(2), B, C, h, w, 64, 64, 1, 64, 64, None, strategy_word, 0, None, None,
                                                 omap.data_ptr(), None, 0, _lib.current_stream_ptr(torch.device(DEV)))
    _lib.check(rc, "pp_acq_lowres_score_topk")
    return omap


@pytest.mark.parametrize("entry", ["pp_acq_score_map", "pp_acq_lowres_score_topk"])
def test_reference_order_flag_equals_the_process_switch(entry):
    """64 x 64, C = 19, logits = 3 x standard normal: the map under `strategy | PP_ACQ_REFERENCE_ORDER` equals the map under
    pp_debug_set_exact_formula(1) bit for bit, and differs from the default-order map somewhere (else the equality says nothing)."""
    sid = acq.strategy_id("entropy")
    if entry == "pp_acq_score_map":
        x = _logits(64, 64, seed=2)
        run = lambda ref: acq.score_map(x, None, "entropy", reference_order=ref)
    else:
        low = _low(16, 16, seed=2)
        run = lambda ref: _lowres_map(low, sid | (acq.REFERENCE_ORDER if ref else 0))
    L = _lib.lib()
    default, flagged = run(False), run(True)
    try:
        L.pp_debug_set_exact_formula(1)
        switched = run(False)
    finally:
        L.pp_debug_set_exact_formula(0)
    torch.cuda.synchronize()
    assert torch.equal(flagged, switched)
    assert not torch.equal(flagged, default)
    assert torch.equal(run(False), default)
