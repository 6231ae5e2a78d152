"""GPU: the pictures through the driver surfaces - evaluate()'s visualizer hook on our Visualiser (fused: panels rendered from
the classifier output) against the same Visualiser fed today's dicts through a plain callable, and Model's opt-in
<epoch>_train.png / <epoch>_val.png.  Shapes follow tests/test_driver_gpu.py: synthetic data, 64 x 96, 5 classes."""
import os
import warnings
from argparse import Namespace

import numpy as np
import pytest
import torch
from PIL import Image

import formula_init as fi
from pixelpick_amd import engine as E
from pixelpick_amd.eval import evaluate
from pixelpick_amd.model import Model
from pixelpick_amd.networks.layers import Dropout
from pixelpick_amd.synthetic import SyntheticDataset
from pixelpick_amd.utils.utils import Visualiser, get_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C, H, W = 5, 64, 96


def _build():
    a = Namespace(use_mc_dropout=False, mc_dropout_p=0.2, n_classes=C, network_name="deeplab", weight_type="random")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = get_model(a)
    m.load_state_dict(fi.formula_state_dict(m.state_dict()))
    for mod in m.modules():
        if isinstance(mod, Dropout):
            mod.p = 0.0
    return m.to(DEV)


class _PaddedVoc(torch.utils.data.Dataset):
    """VOC-style validation items: a size that is no multiple of the stride (reflect-padded, cropped back), label 255 = void."""
    n_classes, dataset_name = C, "voc"

    def __init__(self, n=3, h=50, w=70):
        rng = np.random.RandomState(5)
        self.items = []
        for i in range(n):
            y = rng.randint(0, C, size=(h, w)).astype(np.int64)
            y[rng.rand(h, w) < 0.07] = 255
            self.items.append((fi.formula_input(1, h, w, key=f"vis_voc{i}")[0], torch.from_numpy(y)))

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return {'x': self.items[i][0], 'y': self.items[i][1]}


@pytest.mark.parametrize("kind", ["synthetic", "voc"])
def test_evaluate_fused_pictures_equal_the_dict_path(tmp_path, kind):
    m = _build()
    if kind == "synthetic":
        ds, name, shape = SyntheticDataset(5, H, W, C, 5, seed=2), "cs", (H, W)
        ds.dataset_name = "cs"
    else:
        ds, name, shape = _PaddedVoc(), "voc", (50, 70)
    loader = torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False)
    vis = Visualiser(name)
    calls = []
    kw = dict(epoch=1, visualize_interval=2, stride_total=16, device=torch.device(DEV), val_batch_size=4)
    a = evaluate(m, loader, "fused", dir_ckpt=str(tmp_path / "fused"), visualizer=vis, **kw)
    b = evaluate(m, loader, "dicts", dir_ckpt=str(tmp_path / "dicts"),
                 visualizer=lambda d, fp: (calls.append(fp), vis(d, fp=fp)), **kw)
    assert a == b
    due = [i for i in range(len(ds)) if i % 2 == 0]
    assert len(calls) == len(due)
    for i in due:
        got = Image.open(tmp_path / "fused" / "e01" / "val" / f"{i}.png")
        want = Image.open(tmp_path / "dicts" / "e01" / "val" / f"{i}.png")
        assert got.size == want.size == (6 * (shape[1] // 2), shape[0] // 2) and got.mode == want.mode == "RGB"
        assert np.array_equal(np.asarray(got), np.asarray(want)), i
    assert sorted(os.listdir(tmp_path / "fused" / "e01" / "val")) == sorted(os.listdir(tmp_path / "dicts" / "e01" / "val"))


def _args(td, **kw):
    base = dict(dataset_name="cs", debug=False, dir_root=td, experim_name="synthetic", ignore_index=5, mc_n_steps=20,
                n_classes=C, n_pixels_by_us=10, network_name="deeplab", query_strategy="margin_sampling", reverse_order=False,
                stride_total=16, top_n_percent=0.0, use_mc_dropout=False, vote_type="hard", mc_dropout_p=0.2,
                n_init_pixels=10, max_budget=10, n_epochs=2, lr_scheduler_type="Poly",
                optimizer_params={"lr": 5e-4, "betas": (0.9, 0.999), "weight_decay": 2e-4, "eps": 1e-7})
    base.update(kw)
    return Namespace(**base)


def test_model_writes_the_pictures_only_when_asked(tmp_path, monkeypatch):
    warnings.simplefilter("ignore")
    monkeypatch.delenv("PIXELPICK_VISUALISE", raising=False)
    res = {}
    for mode in ("on", "unset"):
        torch.manual_seed(0)
        np.random.seed(0)
        E.set_dropout_seed(0)
        ds = SyntheticDataset(8, H, W, C, 5, n_init_pixels=10, seed=1)
        ds_val = SyntheticDataset(3, H, W, C, 5, seed=2)
        g = torch.Generator().manual_seed(3)
        mk = lambda d, b, sh: torch.utils.data.DataLoader(d, batch_size=b, shuffle=sh, generator=g if sh else None)
        args = _args(str(tmp_path / mode), **({"visualise": True} if mode == "on" else {}))
        m = Model(args, mk(ds, 4, True), mk(ds, 1, False), mk(ds_val, 1, False), device=torch.device(DEV))
        m()
        res[mode] = list(m.history)
        for nth in range(2):
            d = tmp_path / mode / "checkpoints" / "synthetic" / f"{nth}_query"
            pngs = sorted(f for f in os.listdir(d) if f.endswith(".png"))
            if mode == "on":
                assert pngs == ["1_train.png", "1_val.png", "2_train.png", "2_val.png"]
                for f in pngs:
                    im = Image.open(d / f)
                    assert im.size == (6 * (W // 2), H // 2) and im.mode == "RGB"
                    assert np.asarray(im).std() > 0
            else:
                assert pngs == []
    assert len(res["on"]) == 2 * 2 * 2 and res["on"] == res["unset"]
