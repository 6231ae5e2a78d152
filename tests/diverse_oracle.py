"""Plain-numpy restatement of pp_diverse_select and of the features pp_acq_lowres_prob_at_u8 writes (include/pixelpick_hip.h).

select: a loop over the k picks - the squared distances of every list position to the last pick in int64, the running minimum, the
first position that holds the largest one - then the fill with the earliest ineligible positions.  prob_codes: the float64 softmax of the
logits oracle.acq.bilinear_resize gives (the fp32 rule pp_bilinear_fwd follows), quantised as min(255, rint(255 p))."""
import numpy as np

from oracle import acq as oacq

FAR = 0x7FFFFFFF         # "no pick yet": above every distance (at most 256 * 255^2)


def select(cand, feat, k, n_features=None, exclude=None, n_pixels=None):
    """cand: the flat indices of ONE image in rank order [M]; feat: uint8 [M, ldf], row i the features of list position i, of which the
    first n_features bytes count (None: all); exclude: N entries or None; n_pixels: N (None: len(exclude), without exclude 2^31 - 1).
    -> (idx int32 [k], pos int32 [k], dist int32 [k], n)."""
    cand = [int(c) for c in np.asarray(cand).reshape(-1)]
    feat = np.asarray(feat)
    assert feat.dtype == np.uint8 and feat.ndim == 2 and feat.shape[0] == len(cand)
    F = feat.shape[1] if n_features is None else int(n_features)
    assert 1 <= F <= min(256, feat.shape[1])
    f = feat[:, :F].astype(np.int64)
    if exclude is not None:
        exclude = np.asarray(exclude).reshape(-1)
    N = n_pixels if n_pixels is not None else (len(exclude) if exclude is not None else FAR)
    assert 1 <= k <= len(cand) <= N
    eligible = np.asarray([0 <= c < N and (exclude is None or exclude[c] == 0) for c in cand], dtype=bool)   # never read out of range
    M = len(cand)
    r = np.full(M, FAR, dtype=np.int64)
    alive = eligible.copy()
    pos, dist = [], []
    while len(pos) < k and alive.any():
        live = np.flatnonzero(alive)
        i = int(live[np.argmax(r[live])])            # argmax returns the first of equal values: ties to the smallest position
        dist.append(-1 if not pos else int(r[i]))
        pos.append(i)
        alive[i] = False
        r = np.minimum(r, ((f - f[i]) ** 2).sum(axis=1))
    n = len(pos)
    fill = np.flatnonzero(~eligible)[:k - n].tolist()
    pos += fill
    dist += [-1] * len(fill)
    assert len(pos) == k
    return (np.asarray([cand[i] for i in pos], dtype=np.int32), np.asarray(pos, dtype=np.int32), np.asarray(dist, dtype=np.int32), n)


def select_batch(cand, feat, k, n_features=None, exclude=None, n_pixels=None):
    """cand [B,M], feat [B,M,ldf], exclude [B,...] | None -> (idx [B,k], pos [B,k], dist [B,k], n [B])."""
    out = [select(cand[b], feat[b], k, n_features, None if exclude is None else exclude[b], n_pixels) for b in range(len(cand))]
    return tuple(np.stack([o[j] for o in out]) for j in range(3)) + (np.asarray([o[3] for o in out], dtype=np.int32),)


def prob_codes(low, size, img_idx, pix_idx, crop=None, align_corners=True):
    """low: float32 [B,h,w,C] (channels last, as the kernels take it); -> uint8 [n,C]: min(255, rint(255 p)) of the float64 softmax of
    the interpolated class vector at pixel pix_idx[i] (flat in the crop) of image img_idx[i]."""
    low = np.asarray(low, dtype=np.float32)
    pred = oacq.bilinear_resize(np.ascontiguousarray(low.transpose(0, 3, 1, 2)), size, align_corners)       # [B,C,H,W]
    hc, wc = size if crop is None else crop
    pred = pred[:, :, :hc, :wc].reshape(pred.shape[0], pred.shape[1], hc * wc)
    x = pred[np.asarray(img_idx), :, np.asarray(pix_idx)].astype(np.float64)                                 # [n,C]
    e = np.exp(x - x.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    return np.minimum(255, np.rint(255.0 * p)).astype(np.uint8)
