"""numpy restatement of the MC-dropout HARD vote (include/pixelpick_hip.h, pp_acq_vote_*) on full-size logits [T,C,H,W] - a helper of
tests/test_acq_vote_*.py and tests/test_query_vote_gpu.py, not a test.

  vote      a_t = argmax_c x_t[c] (np.argmax: the first maximum, i.e. the lowest class index on equal logits), n_c = #{t : a_t = c}
  entropy   float32(sum_c tab[n_c]) * 2^-24, tab[0] = 0, tab[n] = rint(-(n/T) ln(n/T) 2^24) in float64, an integer sum
  least_confidence  float32(T - n_(1)) / float32(T)          margin_sampling  float32(n_(1) - n_(2)) / float32(T)
  excluded pixels   -1.0 (entropy, least_confidence) / 2.0 (margin_sampling)
  picks     stable sort on (-score | score, flat index): largest first for entropy / least_confidence, smallest for margin_sampling
"""
import numpy as np

FILL = {"entropy": -1.0, "least_confidence": -1.0, "margin_sampling": 2.0}
LARGEST = {"entropy": True, "least_confidence": True, "margin_sampling": False}


def table(T: int) -> np.ndarray:
    """tab[0..T] as uint32."""
    tab = np.zeros(T + 1, dtype=np.uint32)
    p = np.arange(1, T + 1, dtype=np.float64) / np.float64(T)
    tab[1:] = np.rint(-p * np.log(p) * 2.0 ** 24).astype(np.uint32)
    return tab


def vote_counts(logits: np.ndarray) -> np.ndarray:
    """logits [T,C,H,W] -> counts int64 [C,H,W]."""
    T, C, H, W = logits.shape
    a = np.argmax(logits, axis=1).reshape(T, H * W)
    flat = (a * (H * W) + np.arange(H * W)[None, :]).reshape(-1)
    return np.bincount(flat, minlength=C * H * W).reshape(C, H, W)


def score_from_counts(counts: np.ndarray, T: int, strategy: str) -> np.ndarray:
    """counts [C,...] (sum over C == T) -> float32 [...]."""
    counts = np.asarray(counts, dtype=np.int64)
    if strategy == "entropy":
        s = table(T)[counts].astype(np.int64).sum(axis=0)
        return s.astype(np.float32) * np.float32(2.0 ** -24)
    srt = np.sort(counts, axis=0)
    n1 = srt[-1]
    n2 = srt[-2] if counts.shape[0] > 1 else np.zeros_like(n1)
    num = (T - n1) if strategy == "least_confidence" else (n1 - n2)
    return num.astype(np.float32) / np.float32(T)


def score_map(logits: np.ndarray, exclude, strategy: str) -> np.ndarray:
    """logits [T,C,H,W], exclude bool [H,W] | None -> float32 [H,W] with the fills."""
    m = score_from_counts(vote_counts(logits), logits.shape[0], strategy)
    if exclude is not None:
        m = np.where(np.asarray(exclude, dtype=bool), np.float32(FILL[strategy]), m)
    return m.astype(np.float32)


def picks(m: np.ndarray, k: int, strategy: str) -> np.ndarray:
    """The k flat indices in the ABI's order: value-sorted, ties -> lower flat index."""
    v = m.reshape(-1).astype(np.float64)
    return np.lexsort((np.arange(v.size), -v if LARGEST[strategy] else v))[:k]
