"""GPU tests of the prediction / evaluation surface built on pp_predict_lowres: DeepLab.predict / FPNSeg.predict,
FlatTrainer's keep_logits="low" mode (eager and replayed), Model's metrics taken from the classifier output, and
pixelpick_amd.eval.evaluate().  Shapes follow tests/test_driver_gpu.py: synthetic data, 64 x 96, 5 classes."""
import warnings
from argparse import Namespace
from math import ceil

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import formula_init as fi
from pixelpick_amd import engine as E
from pixelpick_amd.eval import evaluate
from pixelpick_amd.model import Model
from pixelpick_amd.networks.layers import Dropout
from pixelpick_amd.synthetic import SyntheticDataset
from pixelpick_amd.trainer import FlatTrainer
from pixelpick_amd.utils.metrics import RunningScore
from pixelpick_amd.utils.utils import get_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C, H, W = 5, 64, 96


def _build(network="deeplab", n_classes=C):
    a = Namespace(use_mc_dropout=False, mc_dropout_p=0.2, n_classes=n_classes, network_name=network, weight_type="random",
                  use_dilated_resnet=True, n_layers=50, width_multiplier=1.0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = get_model(a)
    m.load_state_dict(fi.formula_state_dict(m.state_dict()))
    for mod in m.modules():
        if isinstance(mod, Dropout):
            mod.p = 0.0
    return m.to(DEV)


def test_deeplab_predict_equals_argmax_of_forward():
    m = _build("deeplab").eval()
    x = fi.formula_input(3, H, W, key="predict").to(DEV)
    with torch.no_grad():
        ref = m(x)["pred"].cpu().argmax(dim=1)
    pred = m.predict(x)
    assert pred.dtype == torch.uint8 and tuple(pred.shape) == (3, H, W) and pred.is_cuda
    assert torch.equal(pred.cpu().to(torch.int64), ref)
    assert ref.unique().numel() > 1, "a constant label map tests nothing"


def test_fpn_predict_equals_argmax_of_forward_on_guarded_pixels():
    """FPNSeg.forward() sums its branches at full resolution, predict() interpolates the classifier output: the same map in exact
    arithmetic.  tests/test_networks_gpu.py holds the two orders' logits to 2e-5 * max|logit| of each other, so a pixel whose two
    largest logits are further apart than twice that bound has the same argmax in both."""
    m = _build("FPN").eval()
    x = fi.formula_input(2, H, W, key="predict_fpn").to(DEV)
    with torch.no_grad():
        z = m(x)["pred"].cpu()
    top2 = z.topk(2, dim=1).values
    ok = (top2[:, 0] - top2[:, 1]) > 2 * 2e-5 * z.abs().max().item()
    print("FPN guarded share", ok.float().mean().item())
    assert ok.float().mean().item() > 0.5
    pred = m.predict(x).cpu().to(torch.int64)
    assert tuple(pred.shape) == (2, H, W)
    assert torch.equal(pred[ok], z.argmax(dim=1)[ok])


def _batches(n=3, B=2):
    return [(fi.formula_input(B, H, W, key=f"low{i}").to(DEV), fi.formula_labels(B, H, W, C, C, 20, key=f"low{i}").to(DEV))
            for i in range(n)]


@pytest.mark.parametrize("replay", [False, True], ids=["eager", "replayed"])
@pytest.mark.parametrize("network", ["deeplab", "FPN"])
def test_trainer_keep_logits_low(network, replay):
    data = _batches()
    out = {}
    for keep in (True, "low"):
        tr = FlatTrainer(_build(network).train(), ignore_index=C)
        losses, hists = [], []
        try:
            for i, (x, y) in enumerate(data):
                if replay and i == 1:
                    tr._ensure_train_mode()
                    tr.enable_replay(x, y, warmup=0, keep_logits=keep)       # the recorded step IS step 1 (as Model does)
                else:
                    tr.train_step(x, y, keep_logits=keep)
                assert (tr._plan is not None) == (replay and i >= 1)
                losses.append(tr.last_loss.item())
                rs = RunningScore(C)
                full = fi.formula_labels(2, H, W, C, C, H * W, key=f"full{i}").to(DEV)      # a dense label map for the metrics
                if keep == "low":
                    assert tr.last_logits is None and tr.last_low is not None
                    assert tr.last_low.shape[0] == 2 and tr.last_low.shape[3] == C and tr.last_low.shape[1] < H
                    assert tuple(tr.last_low_size) == (H, W)
                    assert tr.last_low_align == (network == "deeplab")
                    rs.update_from_lowres(full, tr.last_low, tr.last_low_size, align_corners=tr.last_low_align)
                else:
                    assert tr.last_low is None and tuple(tr.last_logits.shape) == (2, C, H, W)
                    rs.update_from_logits(full, tr.last_logits)
                rs.get_scores()
                hists.append(rs.confusion_matrix.copy())
            torch.cuda.synchronize()
            out[keep] = (losses, tr.flat_p.clone(), hists)
            if replay:
                tr.disable_replay()
                assert tr.last_low is None and tr.last_logits is None
        finally:
            tr.close()
    (la, pa, ha), (lb, pb, hb) = out[True], out["low"]
    assert la == lb, "losses must be bit-equal"
    assert torch.equal(pa, pb), "parameters after 3 steps must be bit-equal"
    for a, b in zip(ha, hb):
        assert a.sum() > 0
        np.testing.assert_array_equal(a, b)


def test_keep_logits_low_needs_the_lowres_loss_path(monkeypatch):
    import pixelpick_amd.trainer as T
    monkeypatch.setattr(T, "SPARSE_LOWRES_CE", False)
    tr = FlatTrainer(_build("deeplab").train(), ignore_index=C)
    x, y = _batches(1)[0]
    with pytest.raises(ValueError):
        tr.train_step(x, y, keep_logits="low")
    tr.close()


def _args(td, **kw):
    base = dict(dataset_name="cs", debug=False, dir_root=td, experim_name="synthetic", ignore_index=5, mc_n_steps=20,
                n_classes=5, n_pixels_by_us=10, network_name="deeplab", query_strategy="margin_sampling", reverse_order=False,
                stride_total=16, top_n_percent=0.0, use_mc_dropout=False, vote_type="hard", mc_dropout_p=0.2,
                n_init_pixels=10, max_budget=10, n_epochs=2, lr_scheduler_type="Poly",
                optimizer_params={"lr": 5e-4, "betas": (0.9, 0.999), "weight_decay": 2e-4, "eps": 1e-7})
    base.update(kw)
    return Namespace(**base)


def test_model_history_and_logs_do_not_depend_on_the_metrics_path(tmp_path, monkeypatch):
    """Model with PIXELPICK_METRICS_LOWRES unset (metrics from the classifier output) and 0 (full-resolution logits), same seeds,
    DeepLab: history and both log files are identical; and the switch really selects the path."""
    warnings.simplefilter("ignore")
    calls = {}
    for name in ("update_from_lowres", "update_from_logits"):
        orig = getattr(RunningScore, name)

        def spy(self, *a, _orig=orig, _name=name, **k):
            calls[_name] = calls.get(_name, 0) + 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(RunningScore, name, spy)
    res = {}
    for mode in ("unset", "0"):
        if mode == "unset":
            monkeypatch.delenv("PIXELPICK_METRICS_LOWRES", raising=False)
        else:
            monkeypatch.setenv("PIXELPICK_METRICS_LOWRES", "0")
        torch.manual_seed(0)
        np.random.seed(0)
        E.set_dropout_seed(0)
        calls.clear()
        ds = SyntheticDataset(10, H, W, C, 5, n_init_pixels=10, seed=1)      # batch 4: two replayed batches + a ragged eager one
        ds_val = SyntheticDataset(4, H, W, C, 5, seed=2)
        g = torch.Generator().manual_seed(3)
        mk = lambda d, b, sh: torch.utils.data.DataLoader(d, batch_size=b, shuffle=sh, generator=g if sh else None)
        m = Model(_args(str(tmp_path / mode)), mk(ds, 4, True), mk(ds, 1, False), mk(ds_val, 1, False), device=torch.device(DEV))
        m()
        logs = {}
        for nth in range(2):
            for f in ("log_train.txt", "log_val.txt"):
                logs[(nth, f)] = open(tmp_path / mode / "checkpoints" / "synthetic" / f"{nth}_query" / f).read()
        res[mode] = (list(m.history), logs, dict(calls))
    assert res["unset"][2].get("update_from_lowres", 0) > 0 and res["unset"][2].get("update_from_logits", 0) == 0
    assert res["0"][2].get("update_from_logits", 0) > 0 and res["0"][2].get("update_from_lowres", 0) == 0
    assert len(res["0"][0]) == 2 * 2 * 2 and all(np.isfinite(h[3]) for h in res["0"][0])
    assert res["unset"][0] == res["0"][0]
    assert res["unset"][1] == res["0"][1]


class _RaggedVoc(torch.utils.data.Dataset):
    """VOC-style validation items: sizes that are no multiple of the stride, label 255 = void."""
    n_classes, dataset_name = C, "voc"
    SIZES = [(50, 70), (50, 70), (50, 70), (61, 43), (61, 43), (50, 70), (37, 53)]

    def __init__(self):
        rng = np.random.RandomState(5)
        self.items = []
        for i, (h, w) in enumerate(self.SIZES):
            x = fi.formula_input(1, h, w, key=f"voc{i}")[0]
            y = rng.randint(0, C, size=(h, w)).astype(np.int64)
            y[rng.rand(h, w) < 0.07] = 255
            self.items.append((x, torch.from_numpy(y)))

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return {'x': self.items[i][0], 'y': self.items[i][1]}


def test_evaluate_on_a_ragged_voc_style_loader(tmp_path, capsys):
    stride = 16
    m = _build("deeplab")
    ds = _RaggedVoc()
    loader = torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False)
    # the reference's loop (eval.py:45-63): one image per forward, full-resolution logits, argmax, numpy RunningScore.update
    ref = RunningScore(C)
    preds = []
    m.eval()
    with torch.no_grad():
        for x, y in ds.items:
            h, w = y.shape
            xp = F.pad(x[None].to(DEV), pad=(0, ceil(w / stride) * stride - w, 0, ceil(h / stride) * stride - h), mode='reflect')
            p = m(xp)['pred'][:, :, :h, :w].cpu().argmax(dim=1)
            preds.append(p[0])
            ref.update(y[None].numpy(), p.numpy())
    s = ref.get_scores()[0]
    seen = []
    miou = evaluate(m, loader, "ragged", epoch=3, dir_ckpt=str(tmp_path), visualizer=lambda d, fp: seen.append((d, fp)),
                    visualize_interval=3, stride_total=stride, device=torch.device(DEV), val_batch_size=1)
    assert miou == s["Mean IoU"]
    assert not m.training
    d = tmp_path / "e03" / "val"
    assert open(d / "log_val.txt").read() == f"epoch,miou,pixel_acc\n3,{s['Mean IoU']},{s['Pixel Acc']}\n"
    assert "Experim name: ragged" in capsys.readouterr().out
    assert [fp for _, fp in seen] == [f"{d}/{i}.png" for i in (0, 3, 6)]
    for (t, _), i in zip(seen, (0, 3, 6)):
        h, w = ds.SIZES[i]
        assert set(t) == {"input", "target", "pred", "confidence", "margin", "entropy"}
        assert tuple(t["input"].shape) == (3, h, w) and torch.equal(t["input"], ds.items[i][0])
        assert torch.equal(t["target"], ds.items[i][1])
        assert t["pred"].dtype == torch.int64 and torch.equal(t["pred"], preds[i])
        for k in ("confidence", "margin", "entropy"):
            assert tuple(t[k].shape) == (h, w) and t[k].dtype == torch.float32 and not t[k].is_cuda
        assert (t["margin"] <= 0).all() and (t["margin"] >= -1).all()
        assert (t["entropy"] >= 0).all() and (t["confidence"] >= 0).all() and (t["confidence"] <= 1).all()
    # equal-sized neighbours forwarded together: the per-image result does not depend on the batch beyond a near-tie argmax
    # flipping with the summation order (tests/test_driver_gpu.py allows the same)
    miou_b = evaluate(m, loader, "ragged", stride_total=stride, device=torch.device(DEV), val_batch_size=8)
    assert abs(miou_b - miou) < 1e-3
    assert not (tmp_path / "val").exists()          # no dir_ckpt: nothing written
    # debug: a single iteration
    one = RunningScore(C)
    one.update(ds.items[0][1][None].numpy(), preds[0][None].numpy())
    assert evaluate(m, loader, "ragged", stride_total=stride, device=torch.device(DEV), debug=True) == one.get_scores()[0]["Mean IoU"]
