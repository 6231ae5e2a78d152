"""numpy restatement of pp_spread_select (include/pixelpick_hip.h): the greedy minimum-distance pass over a rank-ordered candidate
list, its fill phase, the reach A(d) of one pick and the candidate bound M - in python integers, so no width can overflow."""
import numpy as np


def reach(d: int) -> int:
    """A(d) = #{(dy,dx) in Z^2 : dy^2 + dx^2 < d^2}, counted point by point."""
    d = int(d)
    return sum(1 for dy in range(-d, d + 1) for dx in range(-d, d + 1) if dy * dy + dx * dx < d * d)


def candidates(k: int, d: int, N: int) -> int:
    return min(int(N), max(int(k), (int(k) - 1) * reach(d) + 1))


def select(cand, W: int, k: int, d: int, exclude=None, N=None):
    """One image.  cand: flat indices y*W + x in rank order; exclude: bytes [N] or None; an index outside [0, N) counts as excluded.
    -> (idx [k], pos [k], n): accepted picks in acceptance order, then the fill, their list positions, the accepted count."""
    cand = [int(c) for c in np.asarray(cand).reshape(-1)]
    ex = None if exclude is None else np.asarray(exclude).reshape(-1)
    if N is None:
        N = len(ex) if ex is not None else 2 ** 31 - 1
    W, k, d = int(W), int(k), int(d)
    assert 1 <= k <= len(cand) and d >= 1 and W >= 1
    picks, pos = [], []
    for i, c in enumerate(cand):
        if len(picks) == k:
            break
        if c < 0 or c >= N or (ex is not None and ex[c] != 0):
            continue
        y, x = divmod(c, W)
        if all((y - py) ** 2 + (x - px) ** 2 >= d * d for py, px in picks):
            picks.append((y, x))
            pos.append(i)
    n = len(pos)
    taken = set(pos)
    for i in range(len(cand)):
        if len(pos) == k:
            break
        if i not in taken:
            pos.append(i)
    return (np.array([cand[i] for i in pos], dtype=np.int32), np.array(pos, dtype=np.int32), n)


def select_batch(cand, W, k, d, exclude=None, N=None):
    """cand [B,M], exclude [B,N] or None -> (idx [B,k], pos [B,k], n [B]) as the entry returns them."""
    cand = np.asarray(cand)
    out = [select(cand[b], W, k, d, None if exclude is None else np.asarray(exclude)[b], N) for b in range(cand.shape[0])]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], dtype=np.int32))


def ranking(score_map, largest: bool):
    """The *_topk entries' order over a whole map: value-sorted, ties -> the lower flat index first (no NaN expected here)."""
    m = np.asarray(score_map).reshape(-1)
    assert not np.isnan(m).any()
    return np.argsort(-m if largest else m, kind="stable")
