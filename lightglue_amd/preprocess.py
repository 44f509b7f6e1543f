"""ImagePreprocessor on the MI355X: the resize step of the reference's `Extractor.extract` (`lightglue/utils.py:12-38`, applied at
`:143`), as one fused HIP kernel (`lightglue_amd/csrc/lg_preprocess.hip`: `lg_preprocess_plan` + `lg_preprocess_resize`); `to_canvas` puts a
whole mixed-size image set into the canvas of a ragged batch in one launch (`lg_preprocess_ragged_plan` + `lg_preprocess_resize_ragged`).

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
from typing import List, Optional, Sequence, Tuple

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

    def plan_images(self, shapes_hw: Sequence[Tuple[int, int]]) -> List[_cabi.LgResizePlan]:
        """`make_plan` under this preprocessor's conf for every `(h, w)` of `shapes_hw` (`resize=None`: identity plans).  Host arithmetic only: the target
        sizes `(plan.h_out, plan.w_out)` of a whole image set are known before any image is touched."""
        c = self.conf
        if c.resize is None:
            return [make_plan(h, w, (h, w)) for h, w in shapes_hw]
        return [make_plan(h, w, c.resize, c.side, c.antialias, c.align_corners) for h, w in shapes_hw]

    def to_canvas(self, images: Sequence[torch.Tensor], channels: Optional[int] = None, canvas_size: Optional[Tuple[int, int]] = None,
                  out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, List[List[int]], torch.Tensor]:
        """A set of images of DIFFERENT sizes, preprocessed into the top-left corners of one canvas by ONE kernel launch (`lg_preprocess_resize_ragged`): the
        input of an extractor's ragged `forward`.  `images`: [C, H, W] or [1, C, H, W] tensors, C = 1 | 3, float32 or uint8, any strides, all on one GPU.
        `channels`: the canvas's channel count — None = the largest among the images, 1 turns 3-channel images into gray (`0.299 r + 0.587 g + 0.114 b`
        of the resized channels, as the float32 tensor expression evaluates it), 3 writes a 1-channel image to all three planes.  `canvas_size`: (Hc, Wc),
        None = the elementwise maximum of the target sizes.  `out`: an existing contiguous float32 canvas [B, channels, Hc, Wc] to write into — nothing outside
        the images' corners is touched; absent, the canvas is allocated and cleared by the library (zeros outside the corners).
        Returns `(canvas, valid_size, scales)`: `canvas[b, :, :h_b, :w_b]` is bit for bit what `self(images[b])` returns (an identity plan copies / converts
        the values as they are), `valid_size` the host list `[[w_b, h_b], ...]` for `forward`, `scales` [B, 2] float32 on the device, row b = `self(images[b])[1]`.
        Per call: one upload (the image table together with `scales`), one kernel, no framework kernel."""
        images = list(images)
        if not images:
            raise ValueError("to_canvas needs at least one image")
        if channels not in (None, 1, 3):
            raise ValueError(f"channels must be None, 1 or 3, got {channels!r}")
        srcs = []
        for i, img in enumerate(images):
            if img.dim() == 3:
                img = img[None]
            if img.dim() != 4 or img.shape[0] != 1:
                raise ValueError(f"image {i} must be [C, H, W] or [1, C, H, W], got {tuple(img.shape)}")
            if img.shape[1] not in (1, 3):
                raise ValueError(f"image {i} must have 1 or 3 channels, got {img.shape[1]}")
            if img.dtype not in (torch.float32, torch.uint8):
                raise TypeError(f"image {i} must be float32 or uint8, got {img.dtype}")
            if img.device.type != "cuda":
                raise RuntimeError("lightglue_amd.ImagePreprocessor runs on MI355X (ROCm device type 'cuda') only; there is no CPU fallback. "
                                   f"Got image {i} on {img.device}.")
            if img.device != images[0].device:
                raise ValueError(f"all images must be on one GPU: image {i} is on {img.device}, image 0 on {images[0].device}")
            srcs.append(img)
        if len(srcs) > _cabi.LG_PREPROCESS_RAGGED_MAX_BATCH:
            raise ValueError(f"to_canvas takes at most {_cabi.LG_PREPROCESS_RAGGED_MAX_BATCH} images per call, got {len(srcs)}")
        device, n = srcs[0].device, len(srcs)
        plans = self.plan_images([tuple(t.shape[-2:]) for t in srcs])
        if channels is None:
            channels = max(t.shape[1] for t in srcs)
        if canvas_size is None:
            canvas_size = (max(p.h_out for p in plans), max(p.w_out for p in plans))
        hc, wc = int(canvas_size[0]), int(canvas_size[1])
        if out is not None:
            if out.dtype != torch.float32 or out.device != device or not out.is_contiguous() or tuple(out.shape) != (n, channels, hc, wc):
                raise ValueError(f"out must be a contiguous float32 tensor [{n}, {channels}, {hc}, {wc}] on {device}, got {out.dtype} {tuple(out.shape)} on {out.device}")

        lib = _cabi.load()
        nbytes = int(lib.lg_preprocess_ragged_table_bytes(n))
        host = np.zeros(nbytes + 8 * n, dtype=np.uint8)         # the table, then `scales`: one upload
        sources = (_cabi.LgImageSource * n)()
        for s, t in zip(sources, srcs):
            s.data, s.dtype = t.data_ptr(), (_cabi.LG_DTYPE_U8 if t.dtype == torch.uint8 else _cabi.LG_DTYPE_F32)
            s.channels, s.h, s.w = t.shape[1:]
            s.stride_b, s.stride_c, s.stride_y, s.stride_x = t.stride()
        tiles, lds = C.c_int64(), C.c_int64()
        _cabi.check(lib.lg_preprocess_ragged_plan(sources, (_cabi.LgResizePlan * n)(*plans), n, channels, hc, wc, host.ctypes.data, nbytes,
                                                  C.byref(tiles), C.byref(lds), None, None))
        host[nbytes:].view(np.float32)[:] = np.array([[p.scale_x, p.scale_y] for p in plans], dtype=np.float64).reshape(-1)      # double -> float32, rounded once like torch.tensor
        table = torch.from_numpy(host).to(device)
        canvas = out if out is not None else torch.empty((n, channels, hc, wc), device=device, dtype=torch.float32)
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device).cuda_stream
            _cabi.check(lib.lg_preprocess_resize_ragged(host.ctypes.data, table.data_ptr(), n, canvas.data_ptr(), int(out is None), C.c_void_p(stream)))
        scales = table[nbytes:].view(torch.float32).view(n, 2)
        return canvas, [[p.w_out, p.h_out] for p in plans], scales
