"""GPU tests of pp_class_balance_select (csrc/acq_select.hip, class_balance_kernel) against the plain-Python oracle (tests/balance_oracle.py):
idx, pos and n must be equal, integer for integer.  The shapes sit where the kernel can go wrong: the edges of its 64-candidate chunks and
of the 1024-candidate strides of its counting walk, the pools of the 64 x 96 golden size (307) and of 256 x 512 (6553), one class and 256 of
them, a class that only appears at the end of the list, the fill phase, candidates outside the image, several images per launch and a
class with more entries than 16 bits count."""
import numpy as np
import pytest
import torch

import balance_oracle as bo
from pixelpick_amd import _lib
from pixelpick_amd import acquisition as acq

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LABELS = ["one", "distinct", "ends", "skew", "late"]
EXCLUSIONS = ["none", "tenth", "most", "outside"]


def _check(cand, label, k, exclude=None):
    """Run the entry on cand [B,M] / label [B,N] and hold it to the oracle; returns the oracle's (idx, pos, n)."""
    cand = np.ascontiguousarray(np.asarray(cand, dtype=np.int32))
    label = np.ascontiguousarray(np.asarray(label, dtype=np.uint8))
    want = bo.select_batch(cand, label, k, exclude)
    idx, pos, n = acq.class_balance_select(torch.from_numpy(cand).to(DEV), torch.from_numpy(label).to(DEV), k, exclude=exclude)
    torch.cuda.synchronize()
    got = (idx.cpu().numpy(), pos.cpu().numpy(), n.cpu().numpy())
    for g, w_, name in zip(got, want, ("idx", "pos", "n")):
        assert g.dtype == np.int32 and g.shape == w_.shape, name
        assert g.tolist() == w_.tolist(), (name, cand.shape, k)
    return want


def _labels(kind, rng, cand, N):
    M = len(cand)
    if kind == "one":
        return np.full(N, 7, dtype=np.uint8)
    lab = np.zeros(N, dtype=np.uint8)
    if kind == "distinct":                           # every list entry another class (M <= 256; a longer list wraps round)
        lab[cand] = np.arange(M) % 256
    elif kind == "ends":                             # bytes 0 and 255 both present: the class is the byte, unsigned
        lab[:] = rng.choice(np.asarray([0, 255, 3], dtype=np.uint8), N)
        lab[cand[0]], lab[cand[M // 2]] = 255, 0
    elif kind == "skew":                             # two classes 95 % / 5 %
        lab[:] = np.where(rng.rand(N) < 0.05, 18, 2)
    elif kind == "late":                             # a class whose first entry is the last list position
        lab[:] = 4
        lab[cand[M - 1]] = 200
    return lab


def _exclusion(kind, rng, cand, N, k):
    """-> (cand, exclude | None)"""
    M = len(cand)
    if kind == "none":
        return cand, None
    if kind == "tenth":
        return cand, (rng.rand(N) < 0.10).astype(np.uint8)
    if kind == "most":                               # fewer than k eligible entries: the fill phase runs
        ex = np.ones(N, dtype=np.uint8)
        ex[cand[rng.permutation(M)[:k // 2]]] = 0
        return cand, ex
    cand = cand.copy()                               # candidates outside [0, N), negative ones included; a tenth excluded as well
    bad = rng.rand(M) < 0.15
    cand[bad] = rng.choice(np.asarray([-1, -2 ** 31, N, N + 5, 2 ** 31 - 1], dtype=np.int64), int(bad.sum()))
    return cand, (rng.rand(N) < 0.10).astype(np.uint8)


def _ks(M):
    return sorted({1, min(6, M), min(1024, M)} | ({M} if M <= 307 else set()))


@pytest.mark.parametrize("M", [1, 63, 64, 65, 127, 129, 307, 1024, 1025, 6553])
def test_against_the_oracle(M):
    rng = np.random.RandomState(M)
    N = M + (0 if M == 1 else 101)
    fills = late = 0
    for k in _ks(M):
        for ekind in EXCLUSIONS:
            images = []
            for lkind in LABELS:
                cand = rng.permutation(N)[:M].astype(np.int64)
                lab = _labels(lkind, rng, cand, N)
                cand, ex = _exclusion(ekind, rng, cand, N, k)
                idx, pos, n = _check(cand[None], lab[None], k, None if ex is None else ex[None])        # B = 1
                fills += int(n[0]) < k
                late += lkind == "late" and ekind == "none" and k >= 2 and M >= 2 and int(pos[0][1]) == M - 1
                images.append((cand, lab, ex))
            for first in (0, 2):                     # B = 3, another content per image
                trio = images[first:first + 3]
                _check(np.stack([t[0] for t in trio]), np.stack([t[1] for t in trio]), k,
                       None if ex is None else np.stack([t[2] for t in trio]))
    assert fills > 0 or M == 1
    assert late > 0 or M == 1                        # the class at the end of the list was picked second: the list was walked to its end


def test_more_entries_in_a_class_than_sixteen_bits_count():
    """M = 70 000: class 5 holds more than 65 536 eligible entries, class 9 shows up only behind position 65 600.  A rank kept in 16 bits
    wraps round to 0 at class 5's entry 65 536 and hands it a slot of round 0."""
    M, N, k = 70_000, 70_011, 8
    rng = np.random.RandomState(5)
    cand = rng.permutation(N)[:M].astype(np.int64)
    lab = np.full(N, 5, dtype=np.uint8)
    rare = [65_601, 66_000, 69_999]
    lab[cand[rare]] = 9
    idx, pos, n = _check(cand[None], lab[None], k)
    assert pos[0].tolist() == [0, 65_601, 1, 66_000, 2, 69_999, 3, 4] and n.tolist() == [k]
    ex = np.zeros(N, dtype=np.uint8)
    ex[cand[:3]] = 1
    idx, pos, n = _check(cand[None], lab[None], k, ex[None])
    assert pos[0].tolist() == [3, 65_601, 4, 66_000, 5, 69_999, 6, 7]


def test_two_runs_give_equal_bytes():
    rng = np.random.RandomState(2)
    B, M, N, k = 3, 6553, 256 * 512, 10
    cand = torch.from_numpy(np.stack([rng.permutation(N)[:M] for _ in range(B)]).astype(np.int32)).to(DEV)
    lab = torch.from_numpy(rng.randint(0, 19, (B, 256, 512)).astype(np.uint8)).to(DEV)
    ex = torch.from_numpy(rng.rand(B, 256, 512) < 0.05).to(DEV)
    a = acq.class_balance_select(cand, lab, k, exclude=ex)
    b = acq.class_balance_select(cand, lab, k, exclude=ex)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    want = bo.select_batch(cand.cpu().numpy(), lab.cpu().numpy(), k, ex.cpu().numpy())
    assert a[0].cpu().numpy().tolist() == want[0].tolist() and a[2].cpu().numpy().tolist() == [k] * B


def test_wrapper_validation_on_the_device():
    cand = torch.zeros(2, 8, dtype=torch.int32, device=DEV)
    lab = torch.zeros(2, 4, 4, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="uint8"):
        acq.class_balance_select(cand, lab.to(torch.int64), 2)
    with pytest.raises(ValueError, match="images"):
        acq.class_balance_select(cand, lab[:1], 2)
    with pytest.raises(ValueError, match="pixels per image"):
        acq.class_balance_select(cand, lab, 2, exclude=np.zeros((2, 15), dtype=bool))
    with pytest.raises(_lib.PixelPickHipError, match="no CPU fallback"):
        acq.class_balance_select(cand, lab.cpu(), 2)
    with pytest.raises(ValueError, match="k=9"):
        acq.class_balance_select(cand, lab, 9)                           # k > M: the library refuses
    with pytest.raises(_lib.PixelPickHipError, match="1024"):
        acq.class_balance_select(torch.zeros(1, 2000, dtype=torch.int32, device=DEV), torch.zeros(1, 2000, dtype=torch.uint8, device=DEV), 1025)
