"""The per-epoch picture (input | target | prediction | confidence | margin | entropy) from the network's low-resolution
classifier output.

`render_lowres` marshals torch device tensors into pp_vis_lowres (csrc/vis.hip): F.interpolate(low, size, 'bilinear')
[:, :, :crop_h, :crop_w] -> softmax -> argmax + the three uncertainty scores -> per-image min / max -> 8-bit panels
(deeplab.py:55-56 + model.py:124,150-156 + utils/utils.py:394-417) in two launches; neither the full-resolution logits nor a float
map ever reach the host.  All arithmetic runs in the hand-written HIP kernels; there is no CPU fallback.

`compose` is the host end both paths of `utils.utils.Visualiser` share: the reference's per-panel resize, the grid and the PNG
(utils/utils.py:418-432).  The palettes are the datasets' published colours as [256, 3] lookup tables.
"""
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .acquisition import _lowres_geom

_TARGET_KIND = {torch.uint8: 1, torch.int64: 2}


def _table(rows) -> np.ndarray:
    t = np.zeros((256, 3), dtype=np.uint8)           # labels a palette does not name are black
    rows = np.asarray(rows, dtype=np.uint8).reshape(-1, 3)
    t[:len(rows)] = rows
    return t


def _voc_table() -> np.ndarray:
    """The PASCAL VOC colour map: bit k of the label's three interleaved bit planes goes to bit 7 - k of r, g, b; 255 (void) is white."""
    t = np.zeros((256, 3), dtype=np.uint8)
    for label in range(256):
        c = label
        for k in range(8):
            for ch in range(3):
                t[label, ch] |= ((c >> ch) & 1) << (7 - k)
            c >>= 3
    t[255] = 255
    return t


PALETTES: Dict[str, np.ndarray] = {
    # CamVid's 11 classes (sky, building, pole, road, pavement, tree, sign, fence, car, pedestrian, bicyclist); 11 = void: black
    "cv": _table([128, 128, 128, 128, 0, 0, 192, 192, 128, 128, 64, 128, 0, 0, 192, 128, 128, 0, 192, 128, 128, 64, 64, 128,
                  64, 0, 128, 64, 64, 0, 0, 128, 192]),
    # Cityscapes' 19 train ids (road ... bicycle); 19 = void: black
    "cs": _table([128, 64, 128, 244, 35, 232, 70, 70, 70, 102, 102, 156, 190, 153, 153, 153, 153, 153, 250, 170, 30, 220, 220, 0,
                  107, 142, 35, 152, 251, 152, 70, 130, 180, 220, 20, 60, 255, 0, 0, 0, 0, 142, 0, 0, 70, 0, 60, 100, 0, 80, 100,
                  0, 0, 230, 119, 11, 32]),
    "voc": _voc_table(),
}


def palette_for(dataset_name: str) -> np.ndarray:
    """utils/utils.py:377-392: "cv", "cs", "voc"; any other name gets the CamVid palette."""
    return PALETTES.get(dataset_name, PALETTES["cv"])


_device_palettes: Dict = {}


def _palette_on(palette, dev) -> torch.Tensor:
    if isinstance(palette, torch.Tensor):
        if palette.dtype != torch.uint8 or tuple(palette.shape) != (256, 3):
            raise ValueError("palette must be a uint8 [256, 3] table")
        return palette.to(dev).contiguous()
    arr = np.ascontiguousarray(palette)
    if arr.dtype != np.uint8 or arr.shape != (256, 3):
        raise ValueError("palette must be a uint8 [256, 3] table")
    key = (arr.tobytes(), str(dev))
    t = _device_palettes.get(key)
    if t is None:
        t = _device_palettes[key] = torch.from_numpy(arr.copy()).to(dev)
    return t


def render_lowres(low: torch.Tensor, size, image: Optional[torch.Tensor] = None, target: Optional[torch.Tensor] = None,
                  palette=PALETTES["cv"], crop=None, align_corners: bool = True) -> Dict[str, object]:
    """low [B,h,w,C] f32 channels-last on the GPU (C <= 64); size = (H, W) interpolated to; crop = (Hc, Wc) <= size, the top-left
    region kept (VOC).  image f32 [B,3,Hc,Wc] and target uint8 / int64 [B,Hc,Wc] (both optional) on the same device; palette a
    uint8 [256,3] table (numpy or torch).  Returns, all on the device:
        'rgb'     uint8 [B,n_rgb,Hc,Wc,3]  the panels named by 'panels': input (with image), target (with target), pred
        'gray'    uint8 [B,3,Hc,Wc]        confidence, margin (negated: small margins are bright), entropy
        'ranges'  f32   [B,4,2]            (min, max) of input, confidence, margin, entropy behind the normalisation
        'buffer'  uint8 flat               the one allocation 'rgb' and 'gray' are views of (one copy brings both to the host)
    Enqueued on the current stream, no sync."""
    B, h, w, C, ldx, H, W, Hc, Wc = _lowres_geom(low, size, crop)
    dev = low.device
    sn = sc = sr = 0
    if image is not None:
        if not isinstance(image, torch.Tensor) or image.dtype != torch.float32 or tuple(image.shape) != (B, 3, Hc, Wc):
            raise ValueError(f"image must be a float32 [B,3,crop_h,crop_w] = {(B, 3, Hc, Wc)} tensor, got "
                             f"{getattr(image, 'dtype', type(image))} {tuple(getattr(image, 'shape', ()))}")
        if image.device != dev:
            raise _lib.PixelPickHipError("image must live on the GPU with low: the HIP path has no CPU fallback")
        if image.stride(3) != 1 or min(image.stride()) < 0:
            image = image.contiguous()
        sn, sc, sr = image.stride(0), image.stride(1), image.stride(2)
    kind = 0
    if target is not None:
        if not isinstance(target, torch.Tensor) or target.dtype not in _TARGET_KIND:
            raise ValueError(f"target must be a uint8 or int64 tensor, got {getattr(target, 'dtype', type(target))}")
        if tuple(target.shape) != (B, Hc, Wc):
            raise ValueError(f"target must be [B,crop_h,crop_w] = {(B, Hc, Wc)}, got {tuple(target.shape)}")
        if target.device != dev:
            raise _lib.PixelPickHipError("target must live on the GPU with low: the HIP path has no CPU fallback")
        target = target.contiguous()
        kind = _TARGET_KIND[target.dtype]
    pal = _palette_on(palette, dev)
    panels = (["input"] if image is not None else []) + (["target"] if target is not None else []) + ["pred"]
    n_rgb, N = len(panels), Hc * Wc
    L = _lib.lib()
    buf = torch.empty(B * (n_rgb * 3 + 3) * N, dtype=torch.uint8, device=dev)
    rgb, gray = buf[:B * n_rgb * N * 3].view(B, n_rgb, Hc, Wc, 3), buf[B * n_rgb * N * 3:].view(B, 3, Hc, Wc)
    ranges = torch.empty((B, 4, 2), dtype=torch.float32, device=dev)
    ws = torch.empty(max(int(L.pp_vis_lowres_workspace_bytes(B, Hc, Wc)), 256), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = L.pp_vis_lowres(low.data_ptr(), ldx, B, C, h, w, H, W, int(bool(align_corners)), Hc, Wc,
                             image.data_ptr() if image is not None else None, sn, sc, sr,
                             target.data_ptr() if target is not None else None, kind, pal.data_ptr(),
                             rgb.data_ptr(), gray.data_ptr(), ranges.data_ptr(), ws.data_ptr(), ws.numel(),
                             _lib.current_stream_ptr(dev))
    _lib.check(rc, "pp_vis_lowres")
    return {"rgb": rgb, "gray": gray, "ranges": ranges, "panels": panels, "buffer": buf}


def compose(panels: Sequence[np.ndarray], fp: str = '', show: bool = False, downsample: int = 2):
    """utils/utils.py:418-432 on byte panels ([H,W,3] or [H,W] uint8): every panel on its own through
    Image.fromarray(..).resize((w // downsample, h // downsample)) with PIL's default filter, pasted left to right into an RGB
    grid, saved to `fp` when given.  -> the grid (PIL image)."""
    from PIL import Image
    imgs = []
    for arr in panels:
        arr = np.ascontiguousarray(arr)
        h, w = arr.shape[:2]
        imgs.append(Image.fromarray(arr).resize((w // downsample, h // downsample)))
    grid = Image.new("RGB", (sum(im.width for im in imgs), imgs[0].height))
    x_offset = 0
    for im in imgs:
        grid.paste(im, (x_offset, 0))
        x_offset += im.width
    if fp:
        grid.save(fp)
    if show:
        grid.show()
    return grid
