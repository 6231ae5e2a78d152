"""Host oracle of the MC-dropout mean-probability scores and BALD (include/pixelpick_hip.h, pp_acq_mean_prob_score_map), numpy float64.

Per pixel, over the T passes of logits [T,C,H,W]:  p_t = softmax(x_t),  pm = mean_t p_t,
    entropy  H(pm)        least_confidence  1 - max_c pm        margin_sampling  pm_(1) - pm_(2)        bald  H(pm) - mean_t H(p_t)
Excluded pixels get -1.0 (entropy, least_confidence, bald) or 2.0 (margin_sampling).  0 * log 0 is NaN, as in the kernels."""
import numpy as np

LARGEST = {"entropy": True, "least_confidence": True, "margin_sampling": False, "bald": True}
FILL = {"entropy": -1.0, "least_confidence": -1.0, "margin_sampling": 2.0, "bald": -1.0}


def softmax(x: np.ndarray) -> np.ndarray:
    """logits [T,C,H,W] -> float64 probabilities."""
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def entropy(p: np.ndarray, axis: int) -> np.ndarray:
    with np.errstate(divide="ignore", invalid="ignore"):
        return (-p * np.log(p)).sum(axis=axis)


def mean_entropy(x: np.ndarray) -> np.ndarray:
    """mean_t H(p_t): [H,W]."""
    return entropy(softmax(x), 1).mean(axis=0)


def score_map(x: np.ndarray, exclude, strategy: str) -> np.ndarray:
    """logits [T,C,H,W] of one image -> float64 [H,W]."""
    p = softmax(x)
    pm = p.mean(axis=0)
    if strategy == "entropy":
        s = entropy(pm, 0)
    elif strategy == "bald":
        s = entropy(pm, 0) - entropy(p, 1).mean(axis=0)
    else:
        top = np.sort(pm, axis=0)[::-1]
        s = 1.0 - top[0] if strategy == "least_confidence" else np.abs(top[0] - top[1])
    if exclude is not None:
        s = np.where(np.asarray(exclude, dtype=bool), FILL[strategy], s)
    return s


def picks(m: np.ndarray, k: int, strategy: str) -> np.ndarray:
    """The ABI's order on a score map: value descending (ascending for margin), ties -> lower flat index, NaN first for largest."""
    v = np.asarray(m, dtype=np.float64).reshape(-1)
    key = np.where(np.isnan(v), -np.inf, -v) if LARGEST[strategy] else np.where(np.isnan(v), np.inf, v)
    return np.lexsort((np.arange(v.size), key))[:k]
