"""ImagePreprocessor on the MI355X: the resize step of the reference's `Extractor.extract` (`lightglue/utils.py:12-38`, applied at
`:143`), as one fused HIP kernel (`lightglue_amd/csrc/lg_preprocess.hip`: `lg_preprocess_plan` + `lg_preprocess_resize`).

The reference calls `kornia.geometry.transform.resize(img, resize, side=, antialias=, align_corners=)` — `interpolation` is in its conf
but never forwarded, so the mode is always bilinear — and returns `(img, scale)` with `scale = [W_out / W_in, H_out / H_in]`.  The
definition built here (target size, per-axis Gaussian antialias on the reflect-padded image, ATen's bilinear coordinate rule) is written
down in `include/lightglue_amd.h`; fixtures come from the reference's own `utils.py` executed over a plain-torch stand-in for kornia's
`resize` (`tools/make_golden_preprocess.py`).  Image FILE I/O (`read_image` / `load_image` / `resize_image`, cv2) stays out of scope.

Extensions over the reference: uint8 input (converted as `float(v) / 255`, i.e. `numpy_image_to_torch` on the device: a 12 MP RGB photo
crosses PCIe as 36 MB instead of 144 MB) and strided input (a channels-last `hwc.permute(2, 0, 1)` view or a crop is read in place)."""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace
from typing import Tuple

import numpy as np
import torch

from . import _cabi


def numpy_image_to_torch(image: np.ndarray) -> torch.Tensor:
    """ref utils.py:85-93: HxWxC (or HxW) array in [0, 255] -> CxHxW float32 tensor in [0, 1] (host side)."""
    if image.ndim == 3:
        image = image.transpose((2, 0, 1))
    elif image.ndim == 2:
        image = image[None]
    else:
        raise ValueError(f"Not an image: {image.shape}")
    return torch.tensor(image / 255.0, dtype=torch.float)


def make_plan(h: int, w: int, resize, side: str = "long", antialias: bool = True, align_corners=None) -> _cabi.LgResizePlan:
    """`lg_preprocess_plan`: target size, per-axis blur taps / sigma and `scale` for an h x w image (host arithmetic only, no GPU).
    `resize`: an edge length or an (h, w) pair.  Raises ValueError for an unknown side, AssertionError outside the envelope."""
    if side not in _cabi.LG_SIDE:
        raise ValueError(f"side must be one of {sorted(_cabi.LG_SIDE)}, got {side!r}")
    if isinstance(resize, (tuple, list)):
        if len(resize) != 2:
            raise ValueError(f"resize must be an int or an (h, w) pair, got {resize!r}")
        rh, rw = int(resize[0]), int(resize[1])
        if rh < 1 or rw < 1:
            raise ValueError(f"resize (h, w) must be positive, got {resize!r}")
    else:
        rh, rw = int(resize), _cabi.LG_RESIZE_EDGE
    plan = _cabi.LgResizePlan()
    _cabi.check(_cabi.load().lg_preprocess_plan(int(h), int(w), rh, rw, _cabi.LG_SIDE[side], int(bool(antialias)), int(bool(align_corners)), C.byref(plan)))
    return plan


class ImagePreprocessor:
    default_conf = {
        "resize": None,  # target edge length, None for no resizing
        "side": "long",
        "interpolation": "bilinear",
        "align_corners": None,
        "antialias": True,
    }

    def __init__(self, **conf) -> None:
        super().__init__()
        self.conf = {**self.default_conf, **conf}
        self.conf = SimpleNamespace(**self.conf)

    def __call__(self, img: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """Resize and preprocess an image, return image and resize scale (ref utils.py:26-38).  img: [C, H, W] or [B, C, H, W], C = 1 | 3,
        float32 or uint8, any strides, on the GPU.  A float32 image that needs no resizing is returned as is (the same object)."""
        if img.device.type != "cuda":
            raise RuntimeError("lightglue_amd.ImagePreprocessor runs on MI355X (ROCm device type 'cuda') only; there is no CPU fallback. "
                               f"Got an image on {img.device}.")
        if img.dim() not in (3, 4):
            raise ValueError(f"image must be [C, H, W] or [B, C, H, W], got {tuple(img.shape)}")
        if img.dtype not in (torch.float32, torch.uint8):
            raise TypeError(f"image must be float32 or uint8, got {img.dtype}")
        c = self.conf
        h, w = img.shape[-2:]
        if c.resize is None:
            plan = make_plan(h, w, (h, w))
        else:
            plan = make_plan(h, w, c.resize, c.side, c.antialias, c.align_corners)
        device = img.device
        scale = torch.tensor([plan.scale_x, plan.scale_y], dtype=torch.float32).to(device)
        if plan.identity and img.dtype == torch.float32:
            return img, scale
        src = img if img.dim() == 4 else img[None]
        bsz, ch = src.shape[:2]
        out = torch.empty((bsz, ch, plan.h_out, plan.w_out), device=device, dtype=torch.float32)
        if out.numel():
            sb, sc, sy, sx = src.stride()
            with torch.cuda.device(device):
                stream = torch.cuda.current_stream(device).cuda_stream
                _cabi.check(_cabi.load().lg_preprocess_resize(
                    src.data_ptr(), _cabi.LG_DTYPE_U8 if img.dtype == torch.uint8 else _cabi.LG_DTYPE_F32, bsz, ch, h, w, sb, sc, sy, sx,
                    C.byref(plan), out.data_ptr(), C.c_void_p(stream)))
        return (out if img.dim() == 4 else out[0]), scale
