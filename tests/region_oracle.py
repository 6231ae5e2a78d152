"""numpy restatement of pp_acq_region_score_map (include/pixelpick_hip.h): the table, the window impurity P through the same integer
path (cast to float32 and divided in float32), the window uncertainty U in float64, the score, the exclusion fill and a stable
ranking.  Windows are clipped at the image border; every image of a batch is scored on its own."""
import numpy as np

FILL = np.float32(-1.0)
MAX_RADIUS = 16


def table(r: int) -> np.ndarray:
    """tab[n] = rint(n ln(n) 2^16) for n = 0 .. (2r+1)^2, tab[0] = tab[1] = 0; uint32."""
    K = (2 * int(r) + 1) ** 2
    n = np.arange(K + 1, dtype=np.float64)
    t = np.zeros(K + 1, dtype=np.float64)
    t[2:] = np.rint(n[2:] * np.log(n[2:]) * 65536.0)
    assert t.max() < 2 ** 31
    return t.astype(np.uint32)


def _window_sum(a: np.ndarray, r: int) -> np.ndarray:
    """a [H,W] -> the sum over the clipped (2r+1)^2 window, in a's dtype, by summed-area table (exact for integers)."""
    H, W = a.shape
    s = np.zeros((H + 1, W + 1), dtype=a.dtype)
    s[1:, 1:] = a.cumsum(0).cumsum(1)
    y0, y1 = np.maximum(np.arange(H) - r, 0), np.minimum(np.arange(H) + r, H - 1) + 1
    x0, x1 = np.maximum(np.arange(W) - r, 0), np.minimum(np.arange(W) + r, W - 1) + 1
    return s[y1][:, x1] - s[y0][:, x1] - s[y1][:, x0] + s[y0][:, x0]


def window_size(H: int, W: int, r: int) -> np.ndarray:
    """N [H,W]: the pixels of the clipped window - from the extents, as the kernel takes it."""
    ny = np.minimum(np.arange(H) + r, H - 1) - np.maximum(np.arange(H) - r, 0) + 1
    nx = np.minimum(np.arange(W) + r, W - 1) - np.maximum(np.arange(W) - r, 0) + 1
    return (ny[:, None] * nx[None, :]).astype(np.int64)


def impurity_int(pred: np.ndarray, C: int, r: int) -> np.ndarray:
    """pred u8 [H,W] -> D = tab[N] - sum_c tab[n_c], int64 [H,W]; a label >= C counts in the one extra bin C."""
    tab = table(r).astype(np.int64)
    H, W = pred.shape
    lab = np.minimum(pred.astype(np.int64), C)
    G = np.zeros((H, W), dtype=np.int64)
    for c in np.unique(lab):
        G += tab[_window_sum((lab == c).astype(np.int64), r)]
    D = tab[window_size(H, W, r)] - G
    assert (D >= 0).all()
    return D


def impurity(pred: np.ndarray, C: int, r: int) -> np.ndarray:
    """P float32 [H,W] = (float)D / (float)(N * 65536): one conversion, one float32 division."""
    H, W = pred.shape
    D = impurity_int(pred, C, r)
    return D.astype(np.float32) / (window_size(H, W, r) * 65536).astype(np.float32)


def uncertainty64(unc: np.ndarray, r: int, flip: bool = False, absolute: bool = False) -> np.ndarray:
    """U float64 [H,W]: the window mean of u = flip ? 1.0f - unc : unc (u formed in float32, as the kernel forms it).
    absolute: the window mean of |u| - the scale of an fp32 sum's error bound when the terms may differ in sign (equal to U itself
    on non-negative terms)."""
    u = unc.astype(np.float32)
    if flip:
        u = np.float32(1.0) - u
    if absolute:
        u = np.abs(u)
    H, W = u.shape
    # shifted adds over the zero-padded map, not a summed-area table: no cancellation (the relative error stays ~K * 2^-53 on
    # non-negative terms, however small the window's values are), and a NaN stays inside the windows that hold it
    pad = np.zeros((H + 2 * r, W + 2 * r), dtype=np.float64)
    pad[r:r + H, r:r + W] = u
    acc = np.zeros((H, W), dtype=np.float64)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            acc += pad[dy:dy + H, dx:dx + W]
    return acc / window_size(H, W, r)


def score64(pred, unc, C: int, r: int, mode: int, flip: bool = False) -> np.ndarray:
    """One image -> float64 [H,W]: mode 0 = P (float32 value) * U (float64), 1 = P, 2 = U.  No exclusion."""
    if mode == 1:
        return impurity(pred, C, r).astype(np.float64)
    if mode == 2:
        return uncertainty64(unc, r, flip)
    return impurity(pred, C, r).astype(np.float64) * uncertainty64(unc, r, flip)


def apply_exclusion(score: np.ndarray, exclude) -> np.ndarray:
    out = np.array(score, copy=True)
    if exclude is not None:
        out[np.asarray(exclude) != 0] = FILL
    return out


def ranking(score_map, k=None) -> np.ndarray:
    """The selection order over one image's map: the largest first, ties -> the lower flat index first (no NaN expected)."""
    m = np.asarray(score_map).reshape(-1)
    assert not np.isnan(m).any()
    order = np.argsort(-m, kind="stable")
    return order if k is None else order[:k]
