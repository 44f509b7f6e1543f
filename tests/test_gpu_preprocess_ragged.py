"""`ImagePreprocessor.to_canvas` on the MI355X (csrc/lg_preprocess.hip, `pp_resize_ragged_kernel`): a mixed-size image set resized / converted into the
canvas of a ragged batch by ONE launch, and `extract_batch` of both extractors on top of it.

The bar is bit identity with the per-image path: `canvas[b, :, :h_b, :w_b]` is `torch.equal` to `ImagePreprocessor.__call__` on image b (the uniform
kernel, pinned by tests/test_gpu_preprocess.py), gray values to the float32 tensor expression `0.299 * r + 0.587 * g + 0.114 * b`, and `extract_batch` to
`collate_features([extract(i) ...])`.

The group of the first tests, under `resize=96`: a uint8 RGB channels-last 201 x 333 photo, a float32 gray 192 x 1536 strip (factor 16: 31 blur taps on
both axes, tiles of a few outputs), a float32 RGB 96 x 70 image (identity: the copy path), a float32 gray 60 x 80 image (upscale, 1 tap) and a cropped
strided uint8 view — five tile shapes and LDS sizes in one launch, the first and the last image of the prefix search, output sizes that are no multiple
of the tile.  (The strip is 192 x 1536 and not 256 x 2048: at `resize=96` the latter needs 41 taps, outside LG_PREPROCESS_MAX_TAPS = 33 — it is refused
here as it is by `__call__`, which the first test also checks.)  A 9 x 40 image (one tile) joins where the plan allows it."""
import pytest
import torch

import make_golden_preprocess as GP
from conftest import require_gpu

_cache = {}


def _group():
    """the seeded image set on the GPU, made once and never modified"""
    if "group" not in _cache:
        photo = GP.preprocess_image(40, "uint8", 1, 3, 201, 333)[0].cuda().permute(1, 2, 0).contiguous().permute(2, 0, 1)      # channels-last view
        assert not photo.is_contiguous() and photo.stride(0) == 1
        _cache["group"] = [photo,
                           GP.preprocess_image(43, "float32", 1, 1, 192, 1536)[0].cuda(),
                           GP.preprocess_image(44, "float32", 1, 3, 96, 70)[0].cuda(),
                           GP.preprocess_image(45, "float32", 1, 1, 60, 80)[0].cuda(),
                           photo[:, 5:-7, 3:-11]]
        _cache["tile"] = GP.preprocess_image(46, "uint8", 1, 1, 9, 40)[0].cuda()
    return list(_cache["group"])


def _per_image(pre, images):
    """`pre(img)` of every image (the uniform kernel; a float32 identity is the image itself), computed once per configuration"""
    key = ("per_image", tuple(sorted((k, str(v)) for k, v in vars(pre.conf).items())), len(images))
    if key not in _cache:
        _cache[key] = [pre(img) for img in images]
    return _cache[key]


def _gray(o):
    return 0.299 * o[0:1] + 0.587 * o[1:2] + 0.114 * o[2:3] if o.shape[0] == 3 else o


def _check(pre, images, channels, canvas, valid, scales):
    assert canvas.dtype == torch.float32 and canvas.is_contiguous() and canvas.shape[:2] == (len(images), channels)
    assert scales.dtype == torch.float32 and scales.device == canvas.device and tuple(scales.shape) == (len(images), 2)
    for b, (o, s) in enumerate(_per_image(pre, images)):
        h, w = o.shape[-2:]
        assert valid[b] == [w, h], b
        assert torch.equal(scales[b], s), b
        want = _gray(o) if channels == 1 else o.expand(3, -1, -1)
        assert torch.equal(canvas[b, :, :h, :w], want), f"image {b} ({tuple(images[b].shape)} {images[b].dtype} -> {h} x {w}, canvas channels {channels})"


@pytest.mark.gpu
@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("resize", [96, None])
def test_one_launch_equals_the_per_image_path(resize, channels):
    """tests 1 and 2 of the module docstring: every plan of the group in one launch (channels = 3: gray images on all three planes), and the same group
    turned gray in the store (channels = 1); with resize = None every plan is an identity and uint8 goes through / 255"""
    require_gpu()
    from lightglue_amd import ImagePreprocessor
    from lightglue_amd.preprocess import make_plan
    pre = ImagePreprocessor(resize=resize)
    images = _group()
    if resize is None:
        images.append(_cache["tile"])
    else:
        p = make_plan(192, 1536, 96)
        assert (p.ks_y, p.ks_x, p.h_out, p.w_out) == (31, 31, 12, 96) and make_plan(60, 80, 96).ks_x == 1 and make_plan(96, 70, 96).identity
        with pytest.raises(AssertionError, match="LG_PREPROCESS_MAX_TAPS"):
            pre.to_canvas(images + [torch.empty((1, 256, 2048), device="cuda")])
    canvas, valid, scales = pre.to_canvas(images, channels=channels)
    torch.cuda.synchronize()
    assert tuple(canvas.shape[-2:]) == (max(h for _, h in valid), max(w for w, _ in valid))
    _check(pre, images, channels, canvas, valid, scales)
    if channels == 3:      # the default is the largest channel count of the set
        again, valid2, scales2 = pre.to_canvas(images)
        assert torch.equal(again, canvas) and valid2 == valid and torch.equal(scales2, scales)
    for b, (w, h) in enumerate(valid):      # cleared by the library outside the corners
        assert not canvas[b, :, h:, :].any() and not canvas[b, :, :, w:].any(), b


@pytest.mark.gpu
def test_padding_is_never_written():
    require_gpu()
    from lightglue_amd import ImagePreprocessor
    pre = ImagePreprocessor(resize=96)
    images = _group()
    per = _per_image(pre, images)
    hc, wc = max(o.shape[-2] for o, _ in per) + 5, max(o.shape[-1] for o, _ in per) + 3      # larger than every image on both axes
    for channels in (3, 1):
        out = torch.full((len(images), channels, hc, wc), float("nan"), device="cuda")
        canvas, valid, scales = pre.to_canvas(images, channels=channels, canvas_size=(hc, wc), out=out)
        torch.cuda.synchronize()
        assert canvas is out
        _check(pre, images, channels, canvas, valid, scales)
        bits = out.view(torch.int32)
        nan = torch.full((1,), float("nan"), device="cuda").view(torch.int32)
        for b, (w, h) in enumerate(valid):
            assert h < hc and w < wc
            assert bool((bits[b, :, h:, :] == nan).all()) and bool((bits[b, :, :, w:] == nan).all()), b      # the very bits it was filled with
        fresh, _, _ = pre.to_canvas(images, channels=channels, canvas_size=(hc, wc))
        assert torch.equal(fresh, torch.nan_to_num(out, nan=0.0)) and not torch.isnan(fresh).any()      # without out: exactly 0 outside the corners
    with pytest.raises(ValueError, match="out must be"):
        pre.to_canvas(images, channels=3, canvas_size=(hc, wc), out=torch.empty((len(images), 1, hc, wc), device="cuda"))
    with pytest.raises(AssertionError, match="does not fit the canvas"):
        pre.to_canvas(images, canvas_size=(hc - 6, wc))


@pytest.mark.gpu
def test_group_shapes_and_order():
    """B = 1 with the image equal to the canvas (also as a single tile), two images of the same size, and the group reversed: planes permuted, values identical"""
    require_gpu()
    from lightglue_amd import ImagePreprocessor
    pre = ImagePreprocessor(resize=96)
    images = _group()
    for img, conf in ((images[0], dict(resize=96)), (images[0], dict()), (_cache["tile"], dict()), (images[3], dict(resize=(10, 40))), (images[4], dict(resize=(16, 64)))):
        one = ImagePreprocessor(**conf)
        canvas, valid, scales = one.to_canvas([img[None]])      # [1, C, H, W] is accepted like [C, H, W]
        o, s = one(img)
        assert tuple(canvas.shape) == (1,) + tuple(o.shape) and torch.equal(canvas[0], o) and torch.equal(scales[0], s), conf
    twins = [images[3], GP.preprocess_image(47, "float32", 1, 1, 60, 80)[0].cuda()]
    canvas, valid, _ = pre.to_canvas(twins)
    assert valid[0] == valid[1] and torch.equal(canvas[0], pre(twins[0])[0]) and torch.equal(canvas[1], pre(twins[1])[0]) and not torch.equal(canvas[0], canvas[1])
    fwd, vf, sf = pre.to_canvas(images, channels=1)
    rev, vr, sr = pre.to_canvas(images[::-1], channels=1)
    assert vr == vf[::-1] and torch.equal(sr, sf.flip(0)) and torch.equal(rev, fwd.flip(0))


@pytest.mark.gpu
def test_no_framework_kernels_inside_to_canvas():
    """Between the start of to_canvas and its return the torch profiler sees exactly one kernel, of namespace lg; everything else is Memcpy / Memset."""
    require_gpu()
    from torch.profiler import ProfilerActivity, profile
    from lightglue_amd import ImagePreprocessor
    sizes = [(120, 160), (160, 120), (100, 100), (90, 170), (131, 77)]
    images = [GP.preprocess_image(50 + i, "uint8", 1, 3, h, w)[0].cuda().permute(1, 2, 0).contiguous().permute(2, 0, 1) for i, (h, w) in enumerate(sizes)]
    pre = ImagePreprocessor(resize=64)
    pre.to_canvas(images, channels=1); torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        canvas, valid, scales = pre.to_canvas(images, channels=1)
        torch.cuda.synchronize()
    device = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    kernels = [k for k in device if "Memcpy" not in k and "Memset" not in k]
    assert len(kernels) == 1 and "lg::" in kernels[0] and "pp_resize_ragged" in kernels[0], f"device activity inside to_canvas: {sorted(set(device))}"
    assert len([k for k in device if "Memcpy" in k]) <= 2, device      # the table (with the scales)
    _check(pre, images, 1, canvas, valid, scales)


def _image_sets():
    """(kind, extractor, six images around 72 x 96, 96 x 72 and 80 x 80: uint8 RGB channels-last photos and float32 gray images in turn)"""
    import numpy as np
    import make_golden_aliked as GA
    import make_golden_superpoint as GS
    from test_gpu_preprocess import _extractors
    shapes = [(72, 96), (96, 72), (80, 80), (72, 96), (96, 72), (80, 80)]
    for kind, ext, _ in _extractors():
        images = []
        for i, (h, w) in enumerate(shapes):
            c = 3 if i % 2 == 0 else 1
            if kind == "aliked":
                img = GA.aliked_image(70 + i, 1, h, w, c)[0]
            else:
                img = torch.from_numpy(np.clip(np.concatenate([GS.encoder_image(70 + 3 * i + j, 1, h, w)[0] for j in range(c)]), 0, 1))
            if c == 3:
                img = (img.clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous().permute(2, 0, 1)
            images.append(img.cuda())
        yield kind, ext, images


@pytest.mark.gpu
@pytest.mark.parametrize("resize", [64, None])
def test_extract_batch_preprocesses_a_group_in_one_launch(resize):
    """extract_batch == collate_features of the extract loop, key for key, and the preprocess kernel runs once per GROUP (2), not once per image (6)"""
    require_gpu()
    from torch.profiler import ProfilerActivity, profile
    from lightglue_amd import ImagePreprocessor, collate_features, plan_image_batches
    conf = {} if resize is None else {"resize": resize}
    for kind, ext, images in _image_sets():
        want = collate_features([ext.extract(i, **conf) for i in images])
        got = ext.extract_batch(images, batch_size=4, **conf)
        torch.cuda.synchronize()
        assert sorted(got) == sorted(want), kind
        for key in want:
            assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (kind, key)
            assert torch.equal(got[key], want[key]), (kind, resize, key)
        assert int(got["num_keypoints"].max()) > 0, kind
        plans = ImagePreprocessor(**conf).plan_images([tuple(i.shape[-2:]) for i in images])
        groups = plan_image_batches([(p.h_out, p.w_out) for p in plans], 4)
        assert len(groups) == 2
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            ext.extract_batch(images, batch_size=4, **conf)
            torch.cuda.synchronize()
        launches = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "pp_resize" in e.name]
        assert len(launches) == len(groups), (kind, resize, launches)
