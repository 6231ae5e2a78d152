"""GPU tests of pp_acq_lowres_prob_at_u8 (csrc/acq_lowres.hip, prob_at_kernel / prob_at_stream_kernel) against the oracle's codes
(tests/diverse_oracle.py: float64 softmax of the fp32-interpolated logits, min(255, rint(255 p))).

A code can only differ from the oracle's when 255 p lies within the fp32 error of a half-integer: no code may differ by more than 1, and
at most 0.1 % of a case's codes may differ at all (numpy fp32 against float64 on these inputs moves a share of 5e-6 or less; a truncating
or mis-scaled quantiser moves about half).  Rows of out-of-range entries and the pad bytes are zero; the streamed form, forced onto a
64-class head, writes the register form's bytes."""
import numpy as np
import pytest
import torch

import diverse_oracle as do
from pixelpick_amd import _lib
from pixelpick_amd import acquisition as acq

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_LISTED, B = 2000, 3
# name -> (low size, full size, crop | None, align_corners, channel pad of ldx)
GEOMETRIES = {
    "x4_aligned": ((16, 24), (64, 96), None, True, 0),
    "x2_fpn": ((32, 48), (64, 96), None, False, 0),
    "crop_padded": ((16, 24), (64, 96), (50, 77), True, 5),
}
CLASSES = [2, 11, 19, 21, 64, 65, 150, 256]


def _case(C, geometry, seed):
    (h, w), size, crop, align, pad = GEOMETRIES[geometry]
    rng = np.random.RandomState(seed)
    low_h = (rng.randn(B, h, w, C + pad) * 3).astype(np.float32)
    low = torch.from_numpy(low_h).to(DEV)[..., :C]   # a channel slice of a wider tensor: ldx = C + pad
    hc, wc = size if crop is None else crop
    img = rng.randint(0, B, N_LISTED)
    pix = rng.randint(0, hc * wc, N_LISTED)
    pix[:6] = [0, wc - 1, (hc - 1) * wc, hc * wc - 1, (hc - 1) * wc + wc // 2, (hc // 2) * wc + wc - 1]     # corners, last row / column
    img[:6] = [0, B - 1, 0, B - 1, 0, B - 1]
    return low, low_h[..., :C], size, crop, align, img, pix


def _hold(got, want, C, what):
    got = got.cpu().numpy()
    assert got.dtype == np.uint8 and got.shape[0] == want.shape[0] and got.shape[1] % 4 == 0 and got.shape[1] >= C
    assert not got[:, C:].any(), f"{what}: pad bytes are not zero"
    diff = np.abs(got[:, :C].astype(np.int32) - want.astype(np.int32))
    share = float((diff != 0).mean())
    print(f"{what}: largest code difference {int(diff.max())}, share of differing codes {share:.2e}")
    assert diff.max() <= 1, what
    assert share <= 1e-3, what


@pytest.mark.parametrize("geometry", sorted(GEOMETRIES))
@pytest.mark.parametrize("C", CLASSES)
def test_codes_against_the_float64_oracle(C, geometry):
    low, low_h, size, crop, align, img, pix = _case(C, geometry, 100 + C)
    want = do.prob_codes(low_h, size, img, pix, crop=crop, align_corners=align)
    got = acq.prob_at_lowres(low, size, img, pix, crop=crop, align_corners=align)
    assert got.shape == (N_LISTED, (C + 3) // 4 * 4)
    _hold(got, want, C, f"C={C} {geometry}")
    wide = acq.prob_at_lowres(low, size, img, pix, crop=crop, align_corners=align, ldf=(C + 3) // 4 * 4 + 8)
    assert wide.shape == (N_LISTED, (C + 3) // 4 * 4 + 8)
    _hold(wide, want, C, f"C={C} {geometry} padded rows")
    assert wide[:, :got.shape[1]].cpu().numpy().tobytes() == got.cpu().numpy().tobytes()
    assert (want.astype(int).sum(axis=1) > 200).all()       # the oracle's rows are probability vectors, not zeros


@pytest.mark.parametrize("C", [19, 64, 150])
def test_out_of_range_entries_get_zero_rows(C):
    low, low_h, size, crop, align, img, pix = _case(C, "crop_padded", 7)
    hc, wc = crop
    img, pix = img.copy(), pix.copy()
    bad_img = np.arange(10, N_LISTED, 97)
    bad_pix = np.arange(20, N_LISTED, 89)
    img[bad_img] = np.resize([-1, B, 2 ** 31 - 1, -2 ** 31], len(bad_img))
    pix[bad_pix] = np.resize([-1, hc * wc, 2 ** 31 - 1, -2 ** 31, hc * wc + 5], len(bad_pix))
    bad = np.zeros(N_LISTED, dtype=bool)
    bad[bad_img] = bad[bad_pix] = True
    ldf = (C + 3) // 4 * 4 + 4
    dirty = torch.full((N_LISTED, ldf), 0xAA, dtype=torch.uint8, device=DEV)       # the allocator hands this block to the next request
    del dirty
    got = acq.prob_at_lowres(low, size, img, pix, crop=crop, align_corners=align, ldf=ldf)
    g = got.cpu().numpy()
    assert not g[bad].any()
    ok = ~bad
    want = do.prob_codes(low_h, size, img[ok], pix[ok], crop=crop, align_corners=align)
    _hold(got[torch.from_numpy(ok).to(DEV)], want, C, f"C={C} beside out-of-range entries")


def test_streamed_and_register_forms_agree_byte_for_byte():
    """pp_debug_set_acq_tuning(10, 0) forces the streamed class vector at any C (tests/test_acq_wide_gpu.py): C = 64 and 19 run both."""
    L = _lib.lib()
    for C, geometry in ((64, "x4_aligned"), (64, "crop_padded"), (19, "x2_fpn")):
        low, _, size, crop, align, img, pix = _case(C, geometry, 5)
        reg = acq.prob_at_lowres(low, size, img, pix, crop=crop, align_corners=align, ldf=72)
        try:
            L.pp_debug_set_acq_tuning(10, 0)
            streamed = acq.prob_at_lowres(low, size, img, pix, crop=crop, align_corners=align, ldf=72)
        finally:
            L.pp_debug_set_acq_tuning(0, 0)
        assert reg.cpu().numpy().tobytes() == streamed.cpu().numpy().tobytes() and reg.cpu().numpy().any()


def test_wrapper_validation_on_the_device():
    low = torch.randn(2, 8, 8, 19, device=DEV)
    assert acq.prob_at_lowres(low, (32, 32), [], []).shape == (0, 20)
    with pytest.raises(ValueError, match="ldf"):
        acq.prob_at_lowres(low, (32, 32), [0], [0], ldf=16)
    with pytest.raises(ValueError, match="ldf"):
        acq.prob_at_lowres(low, (32, 32), [0], [0], ldf=22)
    with pytest.raises(ValueError, match="equal length"):
        acq.prob_at_lowres(low, (32, 32), [0, 1], [0])
    with pytest.raises(_lib.PixelPickHipError, match="256"):
        acq.prob_at_lowres(torch.randn(1, 4, 4, 257, device=DEV), (8, 8), [0], [0])
