"""Builders and checkers for the top-5 % acquisition tests (query.py:36,57-64: the value-sorted leading 5 % of the score map).

Two kinds of input, both judged against the CPU oracle (oracle.acq: reference operation order, host libm, stable sort) on the SAME
logits, never against a device map:

* graded cases: k + 6 planted pixels whose scores are 6 tol apart, every random pixel that could compete pushed away, so that the
  oracle's picks are the only right answer FOR EVERY RANK for any scorer within tol of the oracle (2 tol would do; the guard asserts
  4 tol on the oracle's map).  `exact_rank_violations` is their checker.
* natural data nobody shaped: `rank_tolerant_violations` states what a scorer within tol of the oracle must still satisfy.

tol(s) = ATOL + RTOL |s| with the suite's score tolerance (tests/test_acq_gpu.py).  No GPU is needed for anything in here; the
builder and the checkers are themselves tested on the CPU (tests/test_oracle_golden.py)."""
import functools

import numpy as np

from oracle import acq as orc

RTOL, ATOL = 2e-5, 2e-6
STRATS = ("entropy", "least_confidence", "margin_sampling")
STEP_TOLS = 6.0          # planted scores are this many tol apart
GUARD_TOLS = 4.0         # asserted on the oracle's map: least gap among the k + 1 leading scores
CONFIDENT = 12.0         # added to the arg-max logit of a random pixel that could compete
EXTRA = 6                # planted pixels beyond k
NAN_AS = 7.0             # NaN scores compare as this (above ln C and 1: first for largest, last for smallest, as the oracle sorts them)


def tol(s):
    return ATOL + RTOL * np.abs(s)


def largest_of(st):
    return st != "margin_sampling"


def planted_logit(st, C, targets):
    """a such that the class vector (a, 0, ..., 0) scores `targets` (float64): closed forms for least confidence
    s = (C-1)/(e^a + C-1) and the margin s = (e^a - 1)/(e^a + C-1), bisection for the entropy (falling in a for a >= 0)."""
    t = np.asarray(targets, np.float64)
    if st == "least_confidence":
        return np.log((C - 1) / t - (C - 1))
    if st == "margin_sampling":
        return np.log((1 + t * (C - 1)) / (1 - t))

    def ent(a):
        S = np.exp(a) + C - 1
        p1, q = np.exp(a) / S, 1 / S
        return -(p1 * np.log(p1) + (C - 1) * q * np.log(q))
    lo, hi = np.zeros_like(t), np.full_like(t, 30.0)
    for _ in range(80):
        mid = (lo + hi) / 2
        big = ent(mid) > t
        lo, hi = np.where(big, mid, lo), np.where(big, hi, mid)
    return (lo + hi) / 2


def planted_targets(st, C, n):
    """n scores starting near the selected end of the range, each STEP_TOLS tol further from it."""
    largest = largest_of(st)
    s = [np.log(C) * 0.97 if st == "entropy" else ((C - 1) / C * 0.97 if largest else 0.002)]
    for _ in range(n - 1):
        step = STEP_TOLS * tol(s[-1])
        s.append(s[-1] - step if largest else s[-1] + step)
    return np.array(s, np.float64)


def random_base(C, H, W, seed):
    """The unshaped image: logits randn * 3, 5 % exclusion; returns the RandomState for what the builder draws next."""
    rng = np.random.RandomState(seed)
    logits = (rng.randn(1, C, H, W) * 3).astype(np.float32)
    excl = (rng.rand(1, H, W) < 0.05).astype(np.uint8)
    return logits, excl, rng


def shape_image(logits, rivals, spots, a):
    """Apply a graded case's shaping to a base image [1,C,H,W] in place: rivals (bool [H*W]) become confident, spots get (a_j, 0, ...)."""
    C = logits.shape[1]
    fl = logits.reshape(1, C, -1)
    pix = np.flatnonzero(rivals)
    top = fl[0][:, pix].argmax(axis=0)
    fl[0, top, pix] += np.float32(CONFIDENT)
    fl[0][:, spots] = 0.0
    fl[0, 0, spots] = np.asarray(a, np.float32)
    return logits


def leading_gaps_in_tol(o_map_excl, k, largest):
    """Adjacent gaps among the k + 1 leading scores of a map (after exclusion), in units of tol of the score nearer the selected end."""
    srt = np.sort(np.nan_to_num(o_map_excl.reshape(-1).astype(np.float64), nan=NAN_AS))
    lead = srt[::-1][:k + 1] if largest else srt[:k + 1]
    return np.abs(np.diff(lead)) / tol(lead[:-1])


def graded_image(C, H, W, st, k, seed):
    """One graded image.  Returns a dict: logits [1,C,H,W], excl [1,H,W] u8, rivals (bool [H*W]), spots (k + 6 flat indices, in
    rank order), a (their float32 logit), o_idx / o_val [k] (the oracle's picks), min_gap_tol.  The guard is asserted, not assumed."""
    largest = largest_of(st)
    logits, excl, rng = random_base(C, H, W, seed)
    n = k + EXTRA
    s = planted_targets(st, C, n)
    a = planted_logit(st, C, s).astype(np.float32)
    m = orc.score_map(logits, st)[0]
    slack = 0.05 if largest else 0.01
    with np.errstate(invalid="ignore"):
        rivals = ((m > s[-1] - slack) if largest else (m < s[-1] + slack)) | np.isnan(m)
    rivals = rivals.reshape(-1)
    free = np.flatnonzero((excl[0] == 0).reshape(-1) & ~rivals)
    spots = rng.choice(free, n, replace=False)
    shape_image(logits, rivals, spots, a)
    o_idx, o_val, o_map = orc.score_topk(logits, excl, st, k, want_map=True)
    gaps = leading_gaps_in_tol(orc.apply_exclude(o_map, excl, st), k, largest)
    assert gaps.min() >= GUARD_TOLS, (C, H, W, st, k, seed, gaps.min())
    assert o_idx[0].tolist() == spots[:k].tolist(), (C, H, W, st, k, seed)
    return dict(logits=logits, excl=excl, rivals=rivals, spots=spots, a=a, o_idx=o_idx[0], o_val=o_val[0], min_gap_tol=float(gaps.min()))


@functools.lru_cache(maxsize=None)
def graded_case(C, H, W, st, k, B, seed0=1):
    """B graded images (seeds seed0 .. seed0 + B - 1) as one batch: (logits [B,C,H,W], excl [B,H,W], o_idx [B,k], o_val [B,k])."""
    imgs = [_graded_image_cached(C, H, W, st, k, seed0 + b) for b in range(B)]
    return (np.concatenate([i["logits"] for i in imgs]), np.concatenate([i["excl"] for i in imgs]),
            np.stack([i["o_idx"] for i in imgs]), np.stack([i["o_val"] for i in imgs]))


@functools.lru_cache(maxsize=None)
def _graded_image_cached(C, H, W, st, k, seed):
    return graded_image(C, H, W, st, k, seed)


# ------------------------------------------------------------------------------------------------ checkers (one image each)
def exact_rank_violations(idx, val, o_idx, o_val):
    """Graded cases: every rank is the oracle's pixel, every value within tol of the oracle's."""
    idx, o_idx = np.asarray(idx).astype(np.int64), np.asarray(o_idx).astype(np.int64)
    out = []
    bad = np.flatnonzero(idx != o_idx)
    if bad.size:
        r = int(bad[0])
        out.append(f"idx: {bad.size} of {idx.size} ranks differ, first at rank {r}: got pixel {int(idx[r])}, the oracle's is {int(o_idx[r])}")
    err = np.abs(np.asarray(val, np.float64) - np.asarray(o_val, np.float64)) / tol(np.asarray(o_val, np.float64))
    if not (err <= 1.0).all():                                   # (a NaN fails too)
        out.append(f"val: worst |val - oracle| = {np.nanmax(err):.3f} tol at rank {int(np.nanargmax(err))}")
    return out


def rank_tolerant_violations(idx, val, o_map_excl, excl, k, largest):
    """Natural data.  With o the oracle's map after exclusion, v_o[r] its r-th selected value and d[r] the device's r-th pick, a
    scorer within tol of the oracle must give:
      1. k distinct picks in range, none excluded (unless fewer than k pixels are free);
      2. |val[r] - o[d[r]]| <= tol;
      3. |o[d[r]] - v_o[r]| <= 2 tol for every r (order statistics move by at most the per-pixel error);
      4. every pixel whose oracle score beats v_o[k-1] by more than 2 tol is among the picks;
      5. at every rank whose oracle neighbours (r - 1, r + 1; for r = k - 1 the best unselected pixel) are both more than 2 tol away,
         d[r] is the oracle's pick.
    NaN scores compare as NAN_AS on both sides.  Returns (violations, info); info['strict_share'] = the share of ranks rule 5 covers."""
    d = np.asarray(idx).astype(np.int64).reshape(-1)
    val = np.nan_to_num(np.asarray(val, np.float64).reshape(-1), nan=NAN_AS)
    o = np.nan_to_num(o_map_excl.reshape(-1).astype(np.float64), nan=NAN_AS)
    N = o.size
    out = []
    order = np.argsort(-o if largest else o, kind="stable")
    o_idx, v_o = order[:k], o[order[:k]]
    nxt = o[order[k]] if k < N else (-np.inf if largest else np.inf)
    t = tol(v_o)
    if d.size != k or (d < 0).any() or (d >= N).any():
        return [f"rule 1: {d.size} picks for k = {k}, range [{d.min()}, {d.max()}] of {N}"], {}
    if np.unique(d).size != k:
        out.append(f"rule 1: only {np.unique(d).size} distinct picks of {k}")
    if excl is not None:
        ex = np.asarray(excl).reshape(-1) != 0
        if (N - int(ex.sum())) >= k and ex[d].any():
            out.append(f"rule 1: {int(ex[d].sum())} excluded pixels picked although {N - int(ex.sum())} >= k are free")
    e2 = np.abs(val - o[d]) / tol(o[d])
    if not (e2 <= 1.0).all():
        out.append(f"rule 2: worst |val - oracle score of the picked pixel| = {np.nanmax(e2):.3f} tol at rank {int(np.nanargmax(e2))}")
    e3 = np.abs(o[d] - v_o) / t
    if not (e3 <= 2.0).all():
        out.append(f"rule 3: worst |oracle score of pick r - oracle's r-th value| = {np.nanmax(e3):.3f} tol at rank {int(np.nanargmax(e3))}")
    sure = (o > v_o[-1] + 2 * t[-1]) if largest else (o < v_o[-1] - 2 * t[-1])
    picked = np.zeros(N, bool)
    picked[d] = True
    missing = np.flatnonzero(sure & ~picked)
    if missing.size:
        out.append(f"rule 4: {missing.size} pixels beat the k-th value by more than 2 tol and are not picked, e.g. pixel {int(missing[0])}")
    g = np.abs(np.diff(np.r_[v_o, nxt]))                         # g[r]: gap between rank r and r + 1 (the best unselected after k - 1)
    up = np.r_[np.inf, g[:-1]]
    strict = (up > 2 * t) & (g > 2 * t)
    wrong = np.flatnonzero(strict & (d != o_idx))
    if wrong.size:
        r = int(wrong[0])
        out.append(f"rule 5: {wrong.size} of {int(strict.sum())} separated ranks differ, first at rank {r}: got pixel {int(d[r])}, the oracle's is {int(o_idx[r])}")
    info = dict(strict_share=float(strict.mean()), equal_share=float((d == o_idx).mean()),
                worst_rule2_tol=float(np.nanmax(e2)), worst_rule3_tol=float(np.nanmax(e3)))
    return out, info


# ------------------------------------------------------------------------------------------------ tests/golden/acq_top5_default.npz
def rebuild_top5_default(g, st):
    """The inputs of the reference-generated fixture of the default call (tools/gen_golden_acq.py, gen_top5_default), rebuilt bit for
    bit from its seeds and shaping data: (logits [n,C,h,w], prev (n bool maps), ys [n,h,w] int64, excl [n,h,w] u8, names, k)."""
    C, h, w, n_img, k = (int(v) for v in g["meta"])
    logits, prev, ys, excl = [], [], [], []
    for i in range(n_img):
        base, ex, _ = random_base(C, h, w, int(g[f"{st}_seed_{i}"]))
        rivals = np.unpackbits(g[f"{st}_rivals_{i}"])[:h * w].astype(bool)
        logits.append(shape_image(base, rivals, g[f"{st}_spots_{i}"].astype(np.int64), g[f"{st}_a_{i}"]))
        prev.append(np.unpackbits(g[f"{st}_prev_{i}"])[:h * w].astype(bool).reshape(h, w))
        ys.append(g[f"{st}_y_{i}"].astype(np.int64))
        excl.append((prev[-1] | (ys[-1] == C)).astype(np.uint8))
        assert (excl[-1] == ex[0]).all()
    return np.concatenate(logits), prev, np.stack(ys), np.stack(excl), [str(n) for n in g["names"]], k
