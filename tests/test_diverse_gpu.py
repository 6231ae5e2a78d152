"""GPU tests of pp_diverse_select (csrc/acq_select.hip, diverse_kernel) against the numpy oracle (tests/diverse_oracle.py): idx, pos, dist and n
must be equal, integer for integer.  The shapes sit where the kernel can go wrong: one candidate, the edges of a wave and of the
1024-thread block, the pools of the 64 x 96 golden size (307) and of 256 x 512 (6553), the switch between the resident and the streaming
form, feature rows of one byte, of whole and of ragged dwords and of the full 256 bytes, padded rows, the fill phase, candidates outside
the image and several images per launch."""
import ctypes

import numpy as np
import pytest
import torch

import diverse_oracle as do
from pixelpick_amd import _lib
from pixelpick_amd import acquisition as acq

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CONTENTS = ["random", "constant", "clusters", "copies", "outlier", "mirrored", "extremes", "far_ineligible"]
LONG_CONTENTS = ["random", "constant", "copies", "far_ineligible"]
EXCLUSIONS = ["none", "tenth", "most", "outside"]
ALL_M = [1, 2, 63, 64, 65, 255, 256, 257, 307, 1025, 6553]
ALL_F = [1, 3, 4, 5, 19, 21, 64, 65, 256]


def _resident(F):
    return int(_lib.lib().pp_diverse_resident_candidates(F))


def _launches():
    """The names of the kernels launched since the previous call (the test build's launch log)."""
    b = ctypes.create_string_buffer(1 << 20)
    assert int(_lib.lib().pp_debug_launch_log(b, len(b))) < len(b), "launch log cut short"
    return b.value.decode()


def _check(cand, feat, k, F, exclude=None, N=None):
    """Run the entry on cand [B,M] / feat [B,M,ldf] and hold it to the oracle; returns the oracle's (idx, pos, dist, n)."""
    cand = np.ascontiguousarray(np.asarray(cand, dtype=np.int32))
    feat = np.ascontiguousarray(np.asarray(feat, dtype=np.uint8))
    want = do.select_batch(cand, feat, k, F, exclude, N)
    got = acq.diverse_select(torch.from_numpy(cand).to(DEV), torch.from_numpy(feat).to(DEV), k, n_features=F, exclude=exclude, n_pixels=N)
    torch.cuda.synchronize()
    for g, w_, name in zip(got, want, ("idx", "pos", "dist", "n")):
        g = g.cpu().numpy()
        assert g.dtype == np.int32 and g.shape == w_.shape, name
        assert g.tolist() == w_.tolist(), (name, cand.shape, feat.shape, F, k)
    return want


def _features(kind, rng, M, F, ldf):
    """-> (uint8 [M, ldf] with the pad bytes 0, the list positions that must not be eligible | None)"""
    f = np.zeros((M, ldf), dtype=np.uint8)
    bad = None
    if kind == "random":
        f[:, :F] = rng.randint(0, 256, (M, F))
    elif kind == "constant":                         # every distance is 0: the first n eligible positions, in list order
        f[:, :F] = rng.randint(0, 256, F)
    elif kind == "clusters":                         # two tight clusters: the picks alternate
        centre = np.where(rng.rand(M, 1) < 0.5, 30, 220)
        f[:, :F] = centre + rng.randint(-3, 4, (M, F))
    elif kind == "copies":                           # copies of pick 0 all through the list: never chosen before a non-copy
        f[:, :F] = rng.randint(0, 256, (M, F))
        f[rng.rand(M) < 0.3] = f[0]
    elif kind == "outlier":                          # the farthest row is the last list position
        f[:, :F] = rng.randint(100, 120, (M, F))
        f[M - 1, :F] = 255
    elif kind == "mirrored":                         # rows i and M-1-i are reflections about 128 of one another; row 0 is the centre
        half = rng.randint(-100, 101, ((M + 1) // 2, F))
        full = np.concatenate([half, -half[:M // 2][::-1]])
        full[0] = 0
        if M > 1:
            full[M - 1] = 0
        f[:, :F] = 128 + full
    elif kind == "extremes":                         # only 0 and 255: at F = 256 the largest distance there is
        f[:, :F] = 255 * rng.randint(0, 2, (M, F))
        f[0, :F] = 0
        f[M // 2, :F] = 255
    elif kind == "far_ineligible":                   # the farthest rows belong to positions that must not be picked
        f[:, :F] = rng.randint(90, 110, (M, F))
        bad = np.flatnonzero(rng.rand(M) < 0.2)
        bad = bad[bad > 0]
        f[bad, :F] = rng.choice(np.asarray([0, 255]), (len(bad), 1))
    return f, bad


def _exclusion(kind, rng, cand, N, k, bad):
    """-> (cand, exclude | None); the list positions in `bad` end up ineligible whatever the kind."""
    M = len(cand)
    cand = cand.copy()
    ex = None
    if kind == "tenth":
        ex = (rng.rand(N) < 0.10).astype(np.uint8)
    elif kind == "most":                             # fewer than k eligible entries: the fill phase runs
        ex = np.ones(N, dtype=np.uint8)
        ex[cand[rng.permutation(M)[:k // 2]]] = 0
    elif kind == "outside":                          # candidates outside [0, N), negative ones included; a tenth excluded as well
        out = rng.rand(M) < 0.15
        cand[out] = rng.choice(np.asarray([-1, -2 ** 31, N, N + 5, 2 ** 31 - 1], dtype=np.int64), int(out.sum()))
        ex = (rng.rand(N) < 0.10).astype(np.uint8)
    if bad is not None and len(bad):
        if ex is None:
            ex = np.zeros(N, dtype=np.uint8)
        inside = (cand[bad] >= 0) & (cand[bad] < N)
        ex[cand[bad][inside]] = 1
    return cand, ex


def _ks(M):
    return sorted({1, min(2, M), min(10, M), min(M, 1024)})


def _run_shape(M, F, ldf, contents=CONTENTS, exclusions=EXCLUSIONS, ks=None):
    rng = np.random.RandomState(M * 1000 + F)
    N = M + (0 if M == 1 else 101)
    seen = dict(fills=0, outlier=0, alternate=0, copies=0, extreme=0)
    for k in ks or _ks(M):
        for ekind in exclusions:
            images = []
            # many picks: the contents whose outcome depends on the number of steps (the oracle takes a pass over the list per pick)
            long = [c for c in contents if c in LONG_CONTENTS]
            for ckind in (contents if k <= 10 else long if M <= 2000 else long[:1] + long[-1:]):
                cand = rng.permutation(N)[:M].astype(np.int64)
                feat, bad = _features(ckind, rng, M, F, ldf)
                cand, ex = _exclusion(ekind, rng, cand, N, k, bad)
                idx, pos, dist, n = _check(cand[None], feat[None], k, F, None if ex is None else ex[None], N)     # B = 1
                idx, pos, dist, n = idx[0], pos[0], dist[0], int(n[0])
                seen["fills"] += n < k
                if ekind == "none" and n >= 2:
                    if ckind == "constant":
                        assert pos.tolist() == list(range(k)) and (dist[1:] == 0).all()
                    if ckind == "outlier" and M >= 3:
                        seen["outlier"] += int(pos[1]) == M - 1
                    if ckind == "clusters" and n >= 4 and F >= 3:
                        side = feat[pos[:4], 0] > 128
                        seen["alternate"] += bool(side[0] != side[1] and len(set(side.tolist())) == 2)
                    if ckind == "copies":            # a copy of pick 0 is at distance 0: it comes after every row that is not one
                        is_copy = (feat[pos[:n]] == feat[pos[0]]).all(axis=1)
                        assert (dist[:n][is_copy][1:] == 0).all()
                        first_copy = np.flatnonzero(is_copy[1:])
                        if len(first_copy) and F >= 4:       # (random rows this wide do not repeat: only copies are at distance 0)
                            assert is_copy[1 + first_copy[0]:].all() and (dist[1:1 + first_copy[0]] > 0).all()
                        seen["copies"] += 1
                    if ckind == "extremes" and F == 256:
                        seen["extreme"] += int(dist[1]) == 256 * 255 * 255
                    if ckind == "mirrored" and M >= 4 and n >= 3:
                        assert dist[1] == dist[2] and pos[1] < pos[2]      # two positions tie exactly: the lower one first
                if ckind == "far_ineligible" and bad is not None:
                    assert not set(pos[:n].tolist()) & set(bad.tolist())
                images.append((cand, feat, ex))
            for first in ((0, len(images) - 3) if k <= 10 or M <= 2000 else ()):       # B = 3, another content per image
                trio = images[max(first, 0):max(first, 0) + 3]
                if len(trio) == 3:
                    exs = [np.zeros(N, dtype=np.uint8) if t[2] is None else t[2] for t in trio]
                    _check(np.stack([t[0] for t in trio]), np.stack([t[1] for t in trio]), k, F, np.stack(exs), N)
    return seen


@pytest.mark.parametrize("M", ALL_M)
def test_class_probability_rows_against_the_oracle(M):
    """F = 19, the workload's feature, at every M, at the minimal row pitch and at a padded one."""
    seen = _run_shape(M, 19, 20)
    seen2 = _run_shape(M, 19, 28, contents=["random", "outlier", "far_ineligible"], exclusions=["none", "most"])
    if M >= 3:
        assert seen["fills"] > 0 and seen2["fills"] > 0 and seen["outlier"] > 0
    if M >= 63:
        assert seen["alternate"] > 0 and seen["copies"] > 0


@pytest.mark.parametrize("M", [65, 307])
@pytest.mark.parametrize("F", [f for f in ALL_F if f != 19])
def test_every_row_width_against_the_oracle(F, M):
    ldf = (F + 3) // 4 * 4
    seen = _run_shape(M, F, ldf)
    _run_shape(M, F, ldf + 8, contents=["random", "extremes", "mirrored"], exclusions=["none", "outside"], ks=[10])
    assert seen["fills"] > 0 and seen["outlier"] > 0
    if F == 256:
        assert seen["extreme"] > 0


@pytest.mark.parametrize("F", [4, 19, 256])
def test_both_forms_on_either_side_of_the_switch(F):
    R = _resident(F)
    if R == 0:                                       # a build that ships the streaming form alone has no switch to stand beside
        return
    ldf = (F + 3) // 4 * 4
    contents, ks = ["random", "outlier", "far_ineligible"], [10]
    _launches()
    _run_shape(R, F, ldf, contents=contents, exclusions=["none", "most"], ks=ks)
    log = _launches()
    assert "diverse_resident_kernel" in log and "diverse_stream_kernel" not in log
    _run_shape(R + 1, F, ldf, contents=contents, exclusions=["none", "most"], ks=ks)
    log = _launches()
    assert "diverse_stream_kernel" in log and "diverse_resident_kernel" not in log


def test_the_streaming_form_forced_onto_resident_shapes():
    """pp_debug_set_acq_tuning(11, 0): the streaming form at any M - the same integers from the other code path."""
    L = _lib.lib()
    try:
        L.pp_debug_set_acq_tuning(11, 0)
        _launches()
        for M, F, ldf in ((307, 19, 20), (6553, 19, 24), (65, 3, 4), (257, 256, 256)):
            _run_shape(M, F, ldf, contents=["random", "copies", "mirrored"], exclusions=["none", "outside"], ks=[2, 10])
        log = _launches()
        assert "diverse_stream_kernel" in log and "diverse_resident_kernel" not in log
    finally:
        L.pp_debug_set_acq_tuning(0, 0)


def test_pad_bytes_do_not_enter_the_result():
    rng = np.random.RandomState(4)
    for M, F, ldf in ((307, 19, 20), (307, 19, 28), (65, 5, 16), (6553, 21, 24), (257, 1, 4)):
        N = M + 50
        cand = np.stack([rng.permutation(N)[:M] for _ in range(2)]).astype(np.int32)
        feat = np.zeros((2, M, ldf), dtype=np.uint8)
        feat[:, :, :F] = rng.randint(0, 256, (2, M, F))
        want = _check(cand, feat, 10, F, N=N)
        feat[:, :, F:] = 0xFF
        again = _check(cand, feat, 10, F, N=N)
        assert all((a == b).all() for a, b in zip(want, again))


def test_two_runs_give_equal_bytes():
    rng = np.random.RandomState(2)
    B, M, N, F, k = 3, 6553, 256 * 512, 19, 10
    cand = torch.from_numpy(np.stack([rng.permutation(N)[:M] for _ in range(B)]).astype(np.int32)).to(DEV)
    feat = torch.from_numpy(rng.randint(0, 256, (B, M, 20)).astype(np.uint8)).to(DEV)
    ex = torch.from_numpy(rng.rand(B, 256, 512) < 0.05).to(DEV)
    a = acq.diverse_select(cand, feat, k, n_features=F, exclude=ex)
    b = acq.diverse_select(cand, feat, k, n_features=F, exclude=ex)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    want = do.select_batch(cand.cpu().numpy(), feat.cpu().numpy(), k, F, ex.cpu().numpy().reshape(B, -1))
    assert all(g.cpu().numpy().tolist() == w_.tolist() for g, w_ in zip(a, want)) and a[3].cpu().numpy().tolist() == [k] * B


def test_wrapper_validation_on_the_device():
    cand = torch.zeros(2, 8, dtype=torch.int32, device=DEV)
    feat = torch.zeros(2, 8, 4, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="uint8"):
        acq.diverse_select(cand, feat.to(torch.int64), 2)
    with pytest.raises(ValueError, match="images"):
        acq.diverse_select(cand, feat[:1], 2)
    with pytest.raises(ValueError, match="rows per image"):
        acq.diverse_select(cand, feat[:, :7], 2)
    with pytest.raises(ValueError, match="pixels per image"):
        acq.diverse_select(cand, feat, 2, exclude=np.zeros((2, 15), dtype=bool), n_pixels=16)
    with pytest.raises(_lib.PixelPickHipError, match="no CPU fallback"):
        acq.diverse_select(cand, feat.cpu(), 2)
    with pytest.raises(ValueError, match="k=9"):
        acq.diverse_select(cand, feat, 9)                                # k > M: the library refuses
    with pytest.raises(ValueError, match="F=5"):
        acq.diverse_select(cand, feat, 2, n_features=5)                  # more features than the row holds
    with pytest.raises(ValueError, match="ldf=6"):
        acq.diverse_select(cand, torch.zeros(2, 8, 6, dtype=torch.uint8, device=DEV), 2)
    with pytest.raises(_lib.PixelPickHipError, match="1024"):
        acq.diverse_select(torch.zeros(1, 2000, dtype=torch.int32, device=DEV), torch.zeros(1, 2000, 4, dtype=torch.uint8, device=DEV), 1025)
