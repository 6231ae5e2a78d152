"""CPU-only: the Visualiser's generic host path, the shared composer and the palettes against the reference's recorded output
(tests/golden/vis_panels.npz, tools/gen_golden_vis.py), and pp_vis_lowres's argument validation."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from pixelpick_amd import _lib
from pixelpick_amd.utils.utils import Visualiser
from pixelpick_amd.visualise import PALETTES, compose

CASES = [("a", "cs"), ("b", "voc")]


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "vis_panels.npz"))


def _dict(g, tag, target=True):
    lc, mg, en = (torch.from_numpy(g[f"{tag}_maps"][0, j].copy()) for j in range(3))
    return {'input': torch.from_numpy(g[f"{tag}_x"][0].copy()), 'target': torch.from_numpy(g[f"{tag}_y"][0].copy()) if target else None,
            'pred': torch.from_numpy(g[f"{tag}_pred"][0].astype(np.int64)), 'confidence': lc, 'margin': mg, 'entropy': en}


@pytest.mark.parametrize("tag,ds", CASES)
@pytest.mark.parametrize("target", [True, False])
def test_visualiser_call_writes_the_reference_grid(gold, tmp_path, tag, ds, target):
    """Visualiser.__call__ on the tensors model.py:150-156 hands over: the saved PNG, read back, is the reference's grid on every
    pixel - six panels with a target, five without - and the caller's tensors are left as they were."""
    want = gold[f"{tag}_grid6" if target else f"{tag}_grid5"]
    d = _dict(gold, tag, target)
    keep = {k: (v.clone() if v is not None else None) for k, v in d.items()}
    fp = str(tmp_path / "p.png")
    assert Visualiser(ds)(d, fp=fp) is None
    got = np.asarray(Image.open(fp).convert("RGB"))
    hc, wc = gold[f"{tag}_crop"]
    assert got.shape == want.shape == (hc // 2, (6 if target else 5) * (wc // 2), 3)
    assert np.array_equal(got, want)
    for k, v in keep.items():
        assert v is None or torch.equal(v, d[k]), k


@pytest.mark.parametrize("tag,ds", CASES)
def test_composer_on_the_reference_panels_gives_the_reference_grid(gold, tmp_path, tag, ds):
    """The composer both paths end in, fed the reference's own pre-resize byte panels: the grid object and the PNG read back."""
    rgb, gray = gold[f"{tag}_rgb"][0], gold[f"{tag}_gray"][0]
    for key, panels in (("grid6", [rgb[0], rgb[1], rgb[2], gray[0], gray[1], gray[2]]),
                        ("grid5", [rgb[0], rgb[2], gray[0], gray[1], gray[2]])):
        fp = str(tmp_path / f"{key}.png")
        grid = compose(panels, fp=fp)
        assert np.array_equal(np.asarray(grid), gold[f"{tag}_{key}"]), key
        assert np.array_equal(np.asarray(Image.open(fp).convert("RGB")), gold[f"{tag}_{key}"]), key


@pytest.mark.parametrize("tag,ds", CASES)
def test_host_panels_equal_the_reference_panels(gold, tag, ds):
    """Before the resize: table-lookup colouring and the fp32 normalisation give the reference's bytes for every image of the case."""
    v = Visualiser(ds)
    for i in range(gold[f"{tag}_x"].shape[0]):
        assert np.array_equal(v._float(torch.from_numpy(gold[f"{tag}_x"][i])), gold[f"{tag}_rgb"][i, 0])
        assert np.array_equal(v._seg(torch.from_numpy(gold[f"{tag}_y"][i])), gold[f"{tag}_rgb"][i, 1])
        assert np.array_equal(v._seg(torch.from_numpy(gold[f"{tag}_pred"][i])), gold[f"{tag}_rgb"][i, 2])
        for j in range(3):
            assert np.array_equal(v._float(torch.from_numpy(gold[f"{tag}_maps"][i, j])), gold[f"{tag}_gray"][i, j])


def test_palettes_equal_the_reference_tables(gold):
    for name in ("cv", "cs", "voc"):
        keys, vals = gold[f"palette_{name}_keys"], gold[f"palette_{name}_vals"]
        assert PALETTES[name].shape == (256, 3) and PALETTES[name].dtype == np.uint8
        assert np.array_equal(PALETTES[name][keys], vals), name
    assert (PALETTES["cv"][11] == 0).all() and (PALETTES["cs"][19] == 0).all() and (PALETTES["voc"][255] == 255).all()
    assert (PALETTES["cv"][12:] == 0).all() and (PALETTES["cs"][20:] == 0).all()
    assert Visualiser("custom").palette is PALETTES["cv"] and Visualiser("voc").palette is PALETTES["voc"]


def test_labels_outside_the_table_are_black():
    v = Visualiser("voc")
    arr = v._seg(torch.tensor([[0, 1, 255], [256, -1, 20]], dtype=torch.int64))
    assert arr[0, 1].tolist() == [128, 0, 0] and arr[0, 2].tolist() == [255, 255, 255]
    assert arr[1, 0].tolist() == [0, 0, 0] and arr[1, 1].tolist() == [0, 0, 0] and arr[1, 2].tolist() == [0, 64, 128]


def test_vis_lowres_argument_validation_without_gpu():
    L = _lib.lib()
    P = 0x7F0000000000          # fake device addresses: validation never reads them
    B, C, h, w, H, W, Hc, Wc = 2, 19, 10, 18, 40, 72, 37, 70
    ws = L.pp_vis_lowres_workspace_bytes(B, Hc, Wc)
    assert ws >= B * 3 * Hc * Wc * 4 + B * 2 * 3 * 8 * 4          # three fp32 maps + one slab row per 64 x 16 tile
    assert L.pp_vis_lowres_workspace_bytes(2 * B, Hc, Wc) > ws

    def call(low=P, C=C, Hc=Hc, Wc=Wc, ws_bytes=ws, ldx=None, target=P, kind=1):
        return L.pp_vis_lowres(low, C if ldx is None else ldx, B, C, h, w, H, W, 1, Hc, Wc, P, 3 * Hc * Wc, Hc * Wc, Wc, target, kind,
                               P, P, P, P, P, ws_bytes, None)

    assert call(low=None) == -1 and b"null" in L.pp_last_error()
    assert call(C=65) == -4 and b"65" in L.pp_last_error()
    assert call(Hc=H + 1) == -1 and b"crop" in L.pp_last_error()
    assert call(Wc=W + 1) == -1
    assert call(ws_bytes=ws - 1) == -3 and b"workspace" in L.pp_last_error()
    assert call(ldx=C - 1) == -1
    assert call(target=None, kind=1) == -1 and call(target=P, kind=0) == -1 and call(kind=3) == -1
    assert L.pp_vis_lowres(*([None] + [0] * 10 + [None, 0, 0, 0, None, 0] + [None] * 5 + [0, None])) < 0 and L.pp_last_error()
    # the query answers 0 instead of wrapping around at sizes no launch would accept
    assert L.pp_vis_lowres_workspace_bytes(1, 1 << 16, 1 << 16) == 0
    assert L.pp_vis_lowres_workspace_bytes(1, 2**31 - 1, 2**31 - 1) == 0
    assert L.pp_vis_lowres_workspace_bytes(1 << 40, 256, 512) == 0
    assert L.pp_vis_lowres_workspace_bytes(0, 256, 512) == 0 and L.pp_vis_lowres_workspace_bytes(1, -1, 512) == 0
