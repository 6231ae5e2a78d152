"""GPU tests of pp_spread_select (csrc/acq_select.hip, spread_select_kernel) against the numpy oracle (tests/spread_oracle.py): idx, pos and n
must be bit-equal.  The shapes sit where the kernel can go wrong: the edges of its 64-candidate chunks, the rank order inside one chunk,
a pick of an earlier chunk that blocks a later one, the fill phase, masks, several images per launch and coordinates whose squared
difference leaves 32 bits."""
import numpy as np
import pytest
import torch

import spread_oracle as so
from pixelpick_amd import acquisition as acq

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _check(cand, W, k, d, exclude=None, N=None):
    """Run the entry on cand [B,M] and hold it to the oracle; returns the oracle's (idx, pos, n)."""
    cand = np.ascontiguousarray(np.asarray(cand, dtype=np.int32))
    if cand.ndim == 1:
        cand = cand[None]
        exclude = None if exclude is None else np.asarray(exclude)[None]
    want = so.select_batch(cand, W, k, d, exclude, N)
    idx, pos, n = acq.spread_select(torch.from_numpy(cand).to(DEV), W, k, d, exclude=exclude, n_pixels=N)
    torch.cuda.synchronize()
    got = (idx.cpu().numpy(), pos.cpu().numpy(), n.cpu().numpy())
    for g, w_, name in zip(got, want, ("idx", "pos", "n")):
        assert g.dtype == np.int32 and g.shape == w_.shape, name
        assert g.tolist() == w_.tolist(), (name, W, k, d)
    return want


def _flat(pts, W):
    return [y * W + x for y, x in pts]


@pytest.mark.parametrize("M", [1, 63, 64, 65, 300])
def test_chunk_edges(M):
    """Lists that end one short of, at and one past a chunk; k = 1, a few, and k = M (d = 1 accepts all M; d = 3 forces the fill)."""
    H, W = 24, 40
    rng = np.random.RandomState(M)
    cand = rng.permutation(H * W)[:M]
    ex = rng.rand(H * W) < 0.1
    for k in sorted({1, min(7, M), M}):
        for d in (1, 3, 6):
            _check(cand, W, k, d, N=H * W)
            _check(cand, W, k, d, ex)


def test_distance_larger_than_the_image():
    H, W = 12, 17
    cand = np.random.RandomState(1).permutation(H * W)[:150]
    idx, pos, n = _check(cand, W, 9, 40, N=H * W)
    assert n.tolist() == [1] and pos[0].tolist() == list(range(9))      # one pick, then the list from its start


@pytest.mark.parametrize("order", ["row_major", "from_the_centre"])
def test_dense_blob_in_one_chunk(order):
    """A 20 x 20 blob, every pixel a candidate: the lanes of a chunk are alive together and block each other in rank order."""
    W = 64
    pts = [(y, x) for y in range(7, 27) for x in range(30, 50)]
    if order == "from_the_centre":
        pts.sort(key=lambda p: ((p[0] - 16.5) ** 2 + (p[1] - 39.5) ** 2, p[0] * W + p[1]))
    idx, pos, n = _check(_flat(pts, W), W, 30, 3, N=40 * W)
    assert n[0] == 30
    _check(_flat(pts, W), W, 400, 3, N=40 * W)                           # k = M: 400 picks, most of them from the fill


def test_pick_of_the_first_chunk_blocks_a_candidate_of_the_second():
    W, d = 200, 10
    a, b, c = (50, 50), (50, 59), (120, 150)                             # b is 9 from a; c is far from both
    near = [(y, x) for y in range(41, 60) for x in range(41, 60) if 0 < (y - 50) ** 2 + (x - 50) ** 2 < d * d and (y, x) != b]
    cand = _flat([a] + near[:63] + [b, c], W)
    assert len(cand) == 66
    idx, pos, n = _check(cand, W, 2, d, N=200 * W)
    assert pos[0].tolist() == [0, 65] and n[0] == 2
    # without a, b is the first pick of its chunk
    idx, pos, n = _check(cand[1:], W, 2, d, N=200 * W)
    assert pos[0, 0] == 0


def test_excluded_candidates_come_back_only_in_the_fill():
    H, W = 16, 30
    rng = np.random.RandomState(3)
    cand = rng.permutation(H * W)[:200]
    ex = np.zeros(H * W, dtype=bool)
    ex[cand[:5]] = True                                                  # the five best are hidden
    ex[cand[70]] = True
    idx, pos, n = _check(cand, W, 6, 4, ex)
    assert n[0] == 6 and pos[0].min() >= 5 and 70 not in pos[0].tolist()
    idx, pos, n = _check(cand, W, 60, 9, ex)                             # the image hosts fewer than 60 picks at d = 9
    assert n[0] < 60 and pos[0, n[0]:n[0] + 5].tolist() == [0, 1, 2, 3, 4]
    _check(cand, W, 200, 2, np.ones(H * W, dtype=np.uint8))              # everything excluded: n = 0, the list as it stands
    bad = cand.copy()
    bad[[0, 3, 64]] = [-7, H * W, 2 ** 31 - 1]                           # outside [0, N): treated as excluded, never looked up
    _check(bad, W, 8, 3, ex)
    _check(bad, W, 200, 3, ex)


def test_three_images_finish_in_chunk_one_in_chunk_three_and_never():
    W, H, d, k, M = 120, 90, 12, 4, 300
    far = [(5 + 20 * i, 7 + 25 * j) for i in range(4) for j in range(4)]                    # 16 pixels >= 20 apart
    blob = [(y, x) for y in range(33, 58) for x in range(33, 58) if 0 < (y - 45) ** 2 + (x - 45) ** 2 < d * d]
    rest = [(y, x) for y in range(70, 90) for x in range(120)]
    img0 = far + rest[:M - len(far)]
    img1 = [(45, 45)] + blob[:139] + [(5, 7), (25, 32), (65, 100)] + rest[:M - 143]
    img2 = [(45, 45)] + blob[:M - 1]
    cand = np.array([_flat(im, W) for im in (img0, img1, img2)])
    assert cand.shape == (3, M)
    idx, pos, n = _check(cand, W, k, d, N=H * W)
    assert n.tolist() == [4, 4, 1] and pos[0].max() < 64 and 128 <= pos[1].max() < 192
    ex = np.random.RandomState(5).rand(3, H * W) < 0.2
    _check(cand, W, k, d, ex)


def test_one_row_and_one_column():
    rng = np.random.RandomState(7)
    cand = rng.permutation(500)[:130]
    for W, N in ((500, 500), (1, 500)):                                  # H = 1; W = 1
        for d in (1, 2, 17):
            _check(cand, W, 12, d, N=N)
        _check(cand, W, 130, 40, rng.rand(N) < 0.3)


def test_squared_differences_beyond_32_bits():
    """H = 2, W = 100000: dx^2 passes 2^31 at 46341 columns and 2^32 at 65536."""
    W, N = 100000, 200000
    cand = _flat([(0, 0), (0, 46999), (0, 50000), (1, 99999), (1, 46400), (0, 3000)], W)
    idx, pos, n = _check(cand, W, 4, 47000, N=N)
    assert pos[0].tolist() == [0, 2, 3, 1] and n[0] == 3
    cand = _flat([(0, 0), (0, 69999), (1, 70000), (0, 99999), (1, 140)], W)
    idx, pos, n = _check(cand, W, 3, 70000, N=N)
    assert pos[0].tolist() == [0, 2, 1] and n[0] == 2
    _check(cand, W, 5, 2 ** 40, N=N)                                     # a distance no image holds
    rng = np.random.RandomState(11)
    _check(rng.permutation(N)[:200], W, 6, 30000, rng.rand(N) < 0.1)


@pytest.mark.parametrize("W,H", [(37, 29), (70000, 3)])
def test_properties_on_random_lists(W, H):
    rng = np.random.RandomState(W)
    N, B, M = W * H, 4, 257
    cand = np.stack([rng.choice(N, M, replace=False) for _ in range(B)]).astype(np.int32)
    ex = rng.rand(B, N) < 0.15
    for k, d in ((5, 2), (20, 7 if W < 100 else 9000), (M, 4)):
        idx, pos, n = acq.spread_select(torch.from_numpy(cand).to(DEV), W, k, d, exclude=ex)
        idx, pos, n = idx.cpu().numpy(), pos.cpu().numpy(), n.cpu().numpy()
        for b in range(B):
            nb = int(n[b])
            assert 0 <= nb <= k
            assert (idx[b] == cand[b][pos[b]]).all()
            assert (np.diff(pos[b, :nb]) > 0).all() and (np.diff(pos[b, nb:]) > 0).all()
            assert not ex[b][idx[b, :nb]].any()
            ys, xs = (idx[b, :nb] // W).astype(np.int64), (idx[b, :nb] % W).astype(np.int64)
            d2 = (ys[:, None] - ys[None]) ** 2 + (xs[:, None] - xs[None]) ** 2
            assert (d2[~np.eye(nb, dtype=bool)] >= d * d).all()
            assert len(set(pos[b].tolist())) == k
        _check(cand, W, k, d, ex)
