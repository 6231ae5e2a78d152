"""GPU tests of the confusion matrix on heads wider than the LDS histogram (csrc/metrics.hip: confusion_wide_kernel behind
pp_confusion_matrix_update for C > 104 and behind pp_confusion_matrix_from_labels) through RunningScore.  Every comparison is
exact (integer counts) against RunningScore.update, the reference's numpy bincount."""
import numpy as np
import pytest
import torch

from pixelpick_amd import engine as E
from pixelpick_amd.utils.metrics import RunningScore

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _host_scores(C, y, pred):
    ref = RunningScore(C)
    ref.update([y.cpu().numpy().astype(np.int64)], [pred.cpu().numpy().astype(np.int64)])
    return ref.confusion_matrix


def _targets(C, shape, seed):
    """randint(0, C + 1) with a band of 255; for C = 256 (int64 labels only) also -1, 256 and 1000."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, C + 1, shape, generator=g, dtype=torch.int64)
    y[:, 5:9] = 255
    if C == 256:
        y[:, 12, ::3] = -1
        y[:, 13, ::2] = 256
        y[:, 14, 1::2] = 1000
    return y


@pytest.mark.parametrize("C", [105, 150, 256])
def test_update_from_logits_on_wide_heads(C):
    B, H, W = 3, 37, 53
    torch.manual_seed(C)
    logits = torch.randn(B, C, H, W) * 3
    y = _targets(C, (B, H, W), seed=C + 1)
    expect = _host_scores(C, y, logits.argmax(dim=1))
    rs = RunningScore(C)
    rs.update_from_logits(y.to(DEV), logits.to(DEV))
    rs._sync()
    np.testing.assert_array_equal(rs.confusion_matrix, expect)
    rs.update_from_logits(y.to(DEV), logits.to(DEV))          # accumulates: on the device and across syncs
    rs.update_from_logits(y.to(DEV), logits.to(DEV))
    rs._sync()
    np.testing.assert_array_equal(rs.confusion_matrix, 3 * expect)
    assert expect.sum() > 0


def test_one_pair_everywhere_is_counted_exactly():
    """Maximum contention: every lane of every wave holds the same (target, prediction) pair."""
    C = 150
    logits = torch.zeros(1, C, 64, 64, device=DEV)
    logits[:, 7] = 1.0
    y = torch.full((1, 64, 64), 7, dtype=torch.int64, device=DEV)
    rs = RunningScore(C)
    rs.update_from_logits(y, logits)
    rs._sync()
    expect = np.zeros((C, C))
    expect[7, 7] = 4096
    np.testing.assert_array_equal(rs.confusion_matrix, expect)


def test_equal_maxima_across_chunks_take_the_first():
    C = 150
    torch.manual_seed(4)
    logits = torch.randn(1, C, 16, 24)
    logits[:, 3] = 50.0
    logits[:, 70] = 50.0
    logits[:, 149] = 50.0
    y = torch.randint(0, C, (1, 16, 24))
    rs = RunningScore(C)
    rs.update_from_logits(y.to(DEV), logits.to(DEV))
    rs._sync()
    np.testing.assert_array_equal(rs.confusion_matrix, _host_scores(C, y, torch.full_like(y, 3)))
    assert rs.confusion_matrix[:, 3].sum() == 16 * 24


@pytest.mark.parametrize("kind", ["uint8", "int64"])
@pytest.mark.parametrize("n", [1, 63, 65, 3 * 37 * 53])
@pytest.mark.parametrize("C", [19, 150, 256])
def test_update_from_labels(C, n, kind):
    g = torch.Generator().manual_seed(C * 7 + n)
    pred = torch.randint(0, 256, (n,), generator=g, dtype=torch.int64).to(torch.uint8)       # predictions >= C: skipped
    if kind == "uint8":
        y = torch.randint(0, 256, (n,), generator=g, dtype=torch.int64).to(torch.uint8)
    else:
        y = torch.randint(-2, C + 40, (n,), generator=g, dtype=torch.int64)
        y[::11] = 1000
    y[0] = min(C - 1, 5)                                                                       # at least one counted label ...
    pred[0] = 2                                                                                # ... with a counted prediction
    keep = pred.to(torch.int64) < C
    expect = _host_scores(C, y.to(torch.int64)[keep], pred[keep])
    rs = RunningScore(C)
    assert rs.update_from_labels(y.to(DEV), pred.to(DEV)) is rs
    rs._sync()
    np.testing.assert_array_equal(rs.confusion_matrix, expect)
    assert expect.sum() > 0


LOWRES_CASES = [
    # C, B, (h,w), (H,W), crop, align_corners
    (150, 2, (6, 10), (24, 40), (21, 37), True),
    (105, 1, (5, 7), (10, 14), None, False),
]


@pytest.mark.parametrize("C,B,lo,size,crop,align", LOWRES_CASES, ids=["C150-crop-align", "C105-halfpixel"])
@pytest.mark.parametrize("kind", ["uint8", "int64"])
def test_update_from_lowres_on_wide_heads(C, B, lo, size, crop, align, kind):
    """Against the launches it stands in for: pp_bilinear_fwd, crop, argmax on the host, bincount."""
    torch.manual_seed(C + lo[0])
    low = (torch.randn(B, *lo, C) * 3).to(DEV)
    logits = E.bilinear(E.Tape(False), E.Var(low), size, align, 0.0, out_nchw=True).t
    hc, wc = size if crop is None else crop
    pred = logits[:, :, :hc, :wc].cpu().argmax(dim=1)
    y = torch.randint(0, C + 1, (B, hc, wc))
    y[:, 2:4] = 255
    if kind == "uint8":
        y = y.to(torch.uint8)
    expect = _host_scores(C, y, pred)
    rs = RunningScore(C)
    assert rs.update_from_lowres(y.to(DEV), low, size, crop=crop, align_corners=align) is rs
    rs._sync()
    np.testing.assert_array_equal(rs.confusion_matrix, expect)
    assert expect.sum() > 0
