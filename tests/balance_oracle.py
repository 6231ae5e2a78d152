"""Plain-Python restatement of pp_class_balance_select (include/pixelpick_hip.h): a loop over the rank-ordered list, a dictionary of class
counts, a sort by (rank inside the class, list position), then the fill with the earliest ineligible positions."""
import numpy as np


def select(cand, label, k, exclude=None):
    """cand: the flat indices of ONE image in rank order [M]; label: its label map, N bytes; exclude: N entries or None.
    -> (idx int32 [k], pos int32 [k], n)."""
    cand = [int(c) for c in np.asarray(cand).reshape(-1)]
    label = np.asarray(label).reshape(-1)
    N = len(label)
    if exclude is not None:
        exclude = np.asarray(exclude).reshape(-1)
        assert len(exclude) == N
    assert 1 <= k <= len(cand) <= N
    seen = {}
    keyed, ineligible = [], []
    for i, c in enumerate(cand):
        if not 0 <= c < N or (exclude is not None and exclude[c] != 0):
            ineligible.append(i)                     # neither map is read at an index outside [0, N)
            continue
        cls = int(label[c]) & 0xFF
        r = seen.get(cls, 0)
        seen[cls] = r + 1
        keyed.append((r, i))
    n = min(k, len(keyed))
    pos = [i for _, i in sorted(keyed)[:n]] + ineligible[:k - n]
    assert len(pos) == k
    return np.asarray([cand[i] for i in pos], dtype=np.int32), np.asarray(pos, dtype=np.int32), n


def select_batch(cand, label, k, exclude=None):
    """cand [B,M], label [B,...], exclude [B,...] | None -> (idx [B,k], pos [B,k], n [B])."""
    B = len(cand)
    out = [select(cand[b], label[b], k, None if exclude is None else exclude[b]) for b in range(B)]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.asarray([o[2] for o in out], dtype=np.int32))
