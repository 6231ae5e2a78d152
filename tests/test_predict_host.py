"""CPU tests of the low-resolution prediction path (pp_predict_lowres): the reference fixture against the CPU oracle, and the
entry's argument validation, which runs on the host before any device call and therefore needs no GPU."""
import os

import numpy as np
import pytest

from oracle import acq as orc
from pixelpick_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GUARD = 1e-4          # top-2 logit gap below which two fp32 evaluation orders of the interpolation may pick different classes
MAX_UNGUARDED = 5e-4  # 0.05 % of the pixels


def _fast_hist(t, p, C):
    m = (t >= 0) & (t < C)
    return np.bincount(C * t[m].astype(np.int64) + p[m], minlength=C * C).reshape(C, C)


@pytest.mark.parametrize("tag", ["cv", "voc"])
def test_fixture_is_reproduced_by_the_cpu_oracle(tag):
    """tests/golden/eval_lowres.npz (F.interpolate + argmax + the reference's RunningScore) from its own `low` by
    oracle.acq.bilinear_resize + argmax + np.bincount: equal on every pixel whose stored top-2 gap exceeds the guard, and the
    guard leaves out at most 0.05 % of the pixels."""
    g = np.load(os.path.join(GOLDEN, "eval_lowres.npz"))
    low, size, (hc, wc) = g[f"{tag}_low"], tuple(int(v) for v in g[f"{tag}_size"]), (int(v) for v in g[f"{tag}_crop"])
    C = low.shape[1]
    logits = orc.bilinear_resize(low, size, align_corners=True)[:, :, :hc, :wc]
    pred = logits.argmax(axis=1)
    ok = g[f"{tag}_gap"] > GUARD
    assert 1.0 - ok.mean() <= MAX_UNGUARDED, f"guard leaves out {1.0 - ok.mean():.5f} of the pixels"
    np.testing.assert_array_equal(pred[ok], g[f"{tag}_pred"][ok])
    y = g[f"{tag}_y"].astype(np.int64)
    # the stored matrix is the reference's over ALL pixels; on the guarded pixels both label maps give the same matrix, and the
    # whole matrices differ by at most the unguarded pixels
    np.testing.assert_array_equal(_fast_hist(y[ok], pred[ok], C), _fast_hist(y[ok], g[f"{tag}_pred"][ok].astype(np.int64), C))
    assert np.abs(_fast_hist(y.ravel(), pred.ravel(), C) - g[f"{tag}_hist"]).sum() <= 2 * int((~ok).sum())
    assert g[f"{tag}_hist"].sum() == int(((y >= 0) & (y < C)).sum())
    assert int(g[f"{tag}_ignore"]) >= C and (y == int(g[f"{tag}_ignore"])).any()


def test_predict_lowres_validates_its_arguments_without_a_gpu():
    L = _lib.lib()
    P = 0x7F0000000000            # a fake DEVICE address: validation never dereferences it
    f = L.pp_predict_lowres

    def bad(*a, code=-1, word=None):
        rc = f(*a)
        assert rc == code, (a, rc, L.pp_last_error())
        msg = L.pp_last_error()
        assert msg, a
        if word is not None:
            assert word in msg, (word, msg)

    ok = dict(low=P, ldx=19, B=2, C=19, h=16, w=32, H=64, W=128, align=1, Hc=64, Wc=128, target=P, kind=2, pred=P, hist=P)

    def args(**kw):
        d = dict(ok, **kw)
        return (d["low"], d["ldx"], d["B"], d["C"], d["h"], d["w"], d["H"], d["W"], d["align"], d["Hc"], d["Wc"], d["target"],
                d["kind"], d["pred"], d["hist"], None)

    bad(*args(low=None), word=b"null")
    bad(*args(pred=None, hist=None), word=b"neither")
    bad(*args(kind=3), word=b"target_kind")
    bad(*args(kind=-1), word=b"target_kind")
    bad(*args(kind=0), word=b"target")                       # kind "none" with a target pointer
    bad(*args(target=None), word=b"target")                  # a kind without a pointer
    bad(*args(target=None, kind=0), word=b"hist")            # hist without a target
    bad(*args(Hc=65), word=b"crop")
    bad(*args(Wc=129), word=b"crop")
    bad(*args(C=0))
    bad(*args(B=0))
    bad(*args(h=0))
    bad(*args(ldx=18), word=b"ldx")
    bad(*args(C=105, ldx=105), code=-4, word=b"104")         # LDS histogram limit
    bad(*args(C=257, ldx=257, hist=None, target=None, kind=0), code=-4, word=b"256")
    bad(*args(H=1 << 20, W=1 << 20, Hc=4, Wc=4), code=-4)
    bad(*args(B=1 << 40), code=-4)
    # (only rejected calls here: the pointers are fake, and a call that passes validation would launch where there is a GPU)
