"""AverageMeter / RunningScore with the reference's interface (utils/metrics.py:85-132,162-206).

RunningScore keeps the reference's numpy `update(label_trues, label_preds)` for host arrays and adds
`update_from_logits(y, logits)`: argmax + confusion-matrix histogram on the device (pp_confusion_matrix_update),
so a train/val step ships C*C int64 to the host instead of two full-resolution maps (model.py:124-125), and
`update_from_lowres(y, low, size)`: the same histogram taken straight from the low-resolution classifier output
(pp_predict_lowres), for networks whose logits are a bilinear interpolation of it, and `update_from_labels(y, pred)`: the
histogram of two label maps that already live on the device (pp_confusion_matrix_from_labels).  All three take up to 256 classes."""
import numpy as np
import torch

from .. import _lib


class AverageMeter(object):
    def __init__(self):
        self.reset()

    def reset(self):
        self.initialized, self.val, self.avg, self.sum, self.count = False, 0, 0, 0, 0

    def update(self, val, weight=1):
        if not self.initialized:
            self.val, self.avg, self.sum, self.count, self.initialized = val, val, val * weight, weight, True
        else:
            self.val = val
            self.sum = self.sum + val * weight
            self.count = self.count + weight
            self.avg = self.sum / self.count

    @property
    def value(self):
        return self.val

    @property
    def average(self):
        return np.round(self.avg, 5)


class RunningScore(object):
    def __init__(self, n_classes):
        self.n_classes = n_classes
        self.confusion_matrix = np.zeros((n_classes, n_classes))
        self._dev_hist = None

    @staticmethod
    def _fast_hist(label_true, label_pred, n_class):
        mask = (label_true >= 0) & (label_true < n_class)
        return np.bincount(n_class * label_true[mask].astype(int) + label_pred[mask], minlength=n_class ** 2).reshape(n_class, n_class)

    def update(self, label_trues, label_preds):
        for lt, lp in zip(label_trues, label_preds):
            self.confusion_matrix += self._fast_hist(lt.flatten(), lp.flatten(), self.n_classes)

    def update_from_logits(self, y: torch.Tensor, logits: torch.Tensor):
        """y [B,H,W] int64, logits [B,C,H,W] f32, both on the GPU; accumulates on the device, no sync.  Up to 256 classes."""
        assert logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 4
        B, C, H, W = logits.shape
        assert C == self.n_classes and logits.stride(3) == 1 and logits.stride(2) == W
        y = y.to(logits.device, torch.int64).contiguous()
        if self._dev_hist is None:
            self._dev_hist = torch.zeros((C, C), dtype=torch.int64, device=logits.device)
        rc = _lib.lib().pp_confusion_matrix_update(logits.data_ptr(), B, C, H * W, logits.stride(0), logits.stride(1), y.data_ptr(),
                                                   self._dev_hist.data_ptr(), _lib.current_stream_ptr(logits.device))
        _lib.check(rc, "pp_confusion_matrix_update")

    def update_from_labels(self, y: torch.Tensor, pred: torch.Tensor):
        """update(y, pred) for two label maps on the GPU (utils/metrics.py:168-177): y int64 or uint8, pred uint8, the same
        number of elements; hist[t, p] += 1 where 0 <= t < n_classes, predictions >= n_classes are not counted.  Accumulates on
        the device, no sync; up to 256 classes."""
        if not (isinstance(y, torch.Tensor) and isinstance(pred, torch.Tensor) and y.is_cuda and pred.is_cuda):
            raise _lib.PixelPickHipError("update_from_labels needs both label maps on the GPU: the HIP path has no CPU fallback")
        if pred.dtype != torch.uint8:
            raise ValueError(f"pred must be a uint8 label map, got {pred.dtype}")
        if y.dtype not in (torch.uint8, torch.int64):
            y = y.to(torch.int64)
        if y.device != pred.device or y.numel() != pred.numel():
            raise ValueError(f"y and pred must hold the same number of labels on one device, got {tuple(y.shape)} and {tuple(pred.shape)}")
        y, pred = y.contiguous(), pred.contiguous()
        C = self.n_classes
        if self._dev_hist is None:
            self._dev_hist = torch.zeros((C, C), dtype=torch.int64, device=pred.device)
        with torch.cuda.device(pred.device):
            rc = _lib.lib().pp_confusion_matrix_from_labels(pred.data_ptr(), y.data_ptr(), 1 if y.dtype == torch.uint8 else 2, y.numel(), C,
                                                            self._dev_hist.data_ptr(), _lib.current_stream_ptr(pred.device))
        _lib.check(rc, "pp_confusion_matrix_from_labels")
        return self

    def update_from_lowres(self, y: torch.Tensor, low: torch.Tensor, size, crop=None, align_corners: bool = True):
        """update_from_logits(y, F.interpolate(low, size, 'bilinear', align_corners)[:, :, :crop_h, :crop_w]) - the same counts,
        bit for bit - without ever writing the full-resolution logits.  Up to 104 classes: one launch (pp_predict_lowres with its
        LDS histogram); wider heads (<= 256): pp_predict_lowres writes the uint8 label map and update_from_labels counts it - one
        byte per pixel between the two launches instead of 4 C.  low [B,h,w,C] f32 channels-last classifier output on the GPU;
        y [B,crop_h,crop_w] int64 or uint8; accumulates on the device, no sync."""
        from ..predict import predict_lowres
        if low.dim() != 4 or low.shape[3] != self.n_classes:
            raise ValueError(f"low must be [B,h,w,{self.n_classes}] channels-last, got {tuple(low.shape)}")
        y = torch.as_tensor(y)
        if y.dtype not in (torch.uint8, torch.int64):
            y = y.to(torch.int64)
        y = y.to(low.device).contiguous()
        if self.n_classes > 104:
            pred, _ = predict_lowres(low, size, crop=crop, align_corners=align_corners, want_pred=True)
            if tuple(y.shape) != tuple(pred.shape):
                raise ValueError(f"y must be [B,crop_h,crop_w] = {tuple(pred.shape)}, got {tuple(y.shape)}")
            return self.update_from_labels(y, pred)
        if self._dev_hist is None:
            self._dev_hist = torch.zeros((self.n_classes, self.n_classes), dtype=torch.int64, device=low.device)
        predict_lowres(low, size, crop=crop, align_corners=align_corners, target=y, hist=self._dev_hist, want_pred=False)
        return self

    def _sync(self):
        if self._dev_hist is not None:
            self.confusion_matrix += self._dev_hist.cpu().numpy()
            self._dev_hist.zero_()

    def get_scores(self):
        self._sync()
        hist = self.confusion_matrix
        with np.errstate(divide="ignore", invalid="ignore"):
            acc = np.diag(hist).sum() / hist.sum()
            acc_cls = np.nanmean(np.diag(hist) / hist.sum(axis=1))
            iu = np.diag(hist) / (hist.sum(axis=1) + hist.sum(axis=0) - np.diag(hist))
            mean_iu = np.nanmean(iu)
            freq = hist.sum(axis=1) / hist.sum()
            fwavacc = (freq[freq > 0] * iu[freq > 0]).sum()
        return ({"Pixel Acc": acc, "Mean Acc": acc_cls, "FreqW Acc": fwavacc, "Mean IoU": mean_iu}, dict(zip(range(self.n_classes), iu)))

    def reset(self):
        self.confusion_matrix = np.zeros((self.n_classes, self.n_classes))
        if self._dev_hist is not None:
            self._dev_hist.zero_()
