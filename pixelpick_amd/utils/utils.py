"""Factories with the reference's names (utils/utils.py): get_model, get_optimizer, get_lr_scheduler, and its Visualiser."""
import numpy as np
import torch

from ..networks.deeplab import DeepLab


def get_model(args):
    """utils/utils.py:15-51."""
    if args.network_name == "deeplab":
        return DeepLab(args)
    if args.network_name == "deeplab_r50":        # not a reference choice (args.py:19): the assembled extra of SURVEY.md 0.1
        return DeepLab(args, backbone='resnet', output_stride=8)
    if args.network_name == "FPN":
        from ..networks.model import FPNSeg
        return FPNSeg(args)
    raise ValueError(args.network_name)


def optimizer_spec(args):
    """What utils/utils.py:112-306 builds, as plain numbers: (kind, slow_lr, lr, weight_decay, momentum).

    cs, and cv/custom with optimizer_type "Adam": Adam(backbone|encoder at lr/10, rest at lr, weight_decay) - the
    reference hands ONLY lr and weight_decay to torch.optim.Adam, so betas and eps are torch's defaults (0.9, 0.999) and
    1e-8 even though args.optimizer_params carries "betas" and "eps": 1e-7.  voc, and cv/custom with optimizer_type "SGD":
    SGD(momentum 0.9) with HARD-CODED lr 1e-3 (backbone|encoder) / 1e-2 (rest) and weight decay 5e-4 (1e-4 for voc + FPN);
    args.optimizer_params is not read at all there."""
    op = args.optimizer_params
    name, fpn = args.dataset_name, args.network_name == "FPN"
    if name == "voc":
        return "sgd", 1e-3, 1e-2, (1e-4 if fpn else 5e-4), 0.9
    if name != "cs" and getattr(args, "optimizer_type", "Adam") == "SGD":
        return "sgd", 1e-3, 1e-2, 5e-4, 0.9
    return "adam", op['lr'] / 10, op['lr'], op['weight_decay'], 0.0


def balanced_class_weights(counts):
    """Per-class loss weights from label counts (QueryStats.dict_label_cnt's values in class order, or a data set's published
    class frequencies): n_total / (K * n_c) for the K classes with n_c > 0 - the weights average 1 over the labels counted, so
    the loss keeps its scale - and 1.0 for a class with no count.  float64 on the host; returns a list for
    FlatTrainer(class_weight=) / args.class_weight.  A mapping is read by class index (missing classes count 0)."""
    if isinstance(counts, dict):
        n = (max(int(k) for k in counts) + 1) if counts else 0
        counts = [counts.get(c, 0) for c in range(n)]
    c = np.asarray(list(counts), dtype=np.float64).reshape(-1)
    if not np.all(np.isfinite(c)) or np.any(c < 0):
        raise ValueError("balanced_class_weights: counts must be finite and non-negative")
    seen = c > 0
    w = np.ones_like(c)
    if seen.any():
        w[seen] = c.sum() / (float(seen.sum()) * c[seen])
    return w.tolist()


def _param_groups(args, model, slow_lr, lr, weight_decay, extra):
    if args.network_name == "FPN":
        parts = [(model.encoder, slow_lr), (model.decoder, lr)]
    else:
        parts = [(model.backbone, slow_lr), (model.aspp, lr), (model.low_level_conv, lr), (model.seg_head, lr)]
    return [dict({'params': m.parameters(), 'lr': l, 'weight_decay': weight_decay}, **extra) for m, l in parts]


def get_optimizer(args, model):
    """utils/utils.py:112-306 (see optimizer_spec for the quirks that are reproduced)."""
    kind, slow_lr, lr, wd, momentum = optimizer_spec(args)
    if kind == "sgd":
        from torch.optim import SGD
        return SGD(_param_groups(args, model, slow_lr, lr, wd, {'momentum': momentum}))
    from torch.optim import Adam
    return Adam(_param_groups(args, model, slow_lr, lr, wd, {}))


def get_lr_scheduler(args, optimizer, iters_per_epoch=-1):
    """utils/utils.py:309-335."""
    if args.dataset_name == "voc" or args.lr_scheduler_type == "Poly":
        from .lr_scheduler import Poly
        return Poly(optimizer, args.n_epochs, iters_per_epoch)
    return torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=[20, 40], gamma=0.1)


class Visualiser:
    """utils/utils.py:376-453 with the reference's call surface: `Visualiser(dataset_name)(dict_tensors, fp=...)` writes the strip
    input | target | prediction | confidence | margin | entropy at half size.  Two ways in, one composer (visualise.compose):

    __call__     the generic host path: tensors on any device, colouring by table lookup (the reference loops over the pixels
                 with .item()), the reference's normalisation in torch fp32 on the CPU.
    from_lowres  the fast path: the byte panels come from the classifier-resolution logits on the GPU (visualise.render_lowres,
                 csrc/vis.hip) and one device-to-host copy fetches them.
    Labels a palette does not name are drawn black (the reference raises KeyError)."""

    def __init__(self, dataset_name):
        from ..visualise import palette_for
        self.palette = palette_for(dataset_name)

    def _seg(self, tensor) -> np.ndarray:
        idx = torch.as_tensor(tensor).detach().cpu().numpy().astype(np.int64)
        if idx.ndim != 2:
            raise ValueError(f"{idx.shape}")
        ok = (idx >= 0) & (idx <= 255)
        arr = self.palette[np.where(ok, idx, 0)]
        arr[~ok] = 0
        return arr

    @staticmethod
    def _float(tensor) -> np.ndarray:
        """utils/utils.py:410-417 (on a copy: the reference normalises the caller's tensor in place)."""
        t = torch.as_tensor(tensor).detach().to("cpu", torch.float32, copy=True)
        if t.ndim not in (2, 3):
            raise ValueError(f"{t.shape}")
        t -= t.min()
        t = t / (t.max() + 1e-7)
        t *= 255
        if t.ndim == 3:
            t = t.permute(1, 2, 0)
        with np.errstate(invalid="ignore"):
            return np.clip(t.numpy(), 0, 255).astype(np.uint8)

    def __call__(self, dict_tensors, fp='', show=False):
        from ..visualise import compose
        panels = [self._float(dict_tensors['input'])]
        if dict_tensors['target'] is not None:
            panels.append(self._seg(dict_tensors['target']))
        panels.append(self._seg(dict_tensors['pred']))
        panels += [self._float(dict_tensors[k]) for k in ('confidence', 'margin', 'entropy')]
        compose(panels, fp=fp, show=show)

    def from_lowres(self, low, size, x, y, fp, crop=None, align_corners=True, index=0):
        """The picture of image `index` of a batch from its classifier output: low [B,h,w,C] on the GPU, size = (H, W)
        interpolated to, x [B,3,Hc,Wc] f32 and y [B,Hc,Wc] uint8 / int64 or None (any device), crop as render_lowres.
        `index` and `fp` may be equally long sequences: those images are rendered in ONE render_lowres call and fetched with
        one copy."""
        from ..visualise import compose, render_lowres
        many = not isinstance(index, int)
        idx, fps = (list(index), list(fp)) if many else ([index], [fp])
        if len(idx) != len(fps):
            raise ValueError(f"{len(idx)} images for {len(fps)} file names")
        dev = low.device
        sel = torch.as_tensor(idx, dtype=torch.int64)
        lo = low.index_select(0, sel.to(dev)) if many or low.shape[0] != 1 else low
        xs = x.index_select(0, sel.to(x.device)).to(dev, torch.float32)
        ys = None if y is None else y.index_select(0, sel.to(y.device)).to(dev)
        if ys is not None and ys.dtype not in (torch.uint8, torch.int64):
            ys = ys.to(torch.int64)
        out = render_lowres(lo, size, image=xs, target=ys, palette=self.palette, crop=crop, align_corners=align_corners)
        n_rgb = len(out["panels"])
        host = out["buffer"].cpu().numpy()                                    # the one device-to-host copy
        B, _, Hc, Wc, _ = out["rgb"].shape
        rgb = host[:B * n_rgb * Hc * Wc * 3].reshape(B, n_rgb, Hc, Wc, 3)
        gray = host[B * n_rgb * Hc * Wc * 3:].reshape(B, 3, Hc, Wc)
        for i, f in enumerate(fps):
            compose([rgb[i, j] for j in range(n_rgb)] + [gray[i, j] for j in range(3)], fp=f)
