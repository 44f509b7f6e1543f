"""ImagePreprocessor on the MI355X (lightglue_amd/preprocess.py, csrc/lg_preprocess.hip) against tests/golden/preprocess/: the reference's own
utils.py executed over the plain-torch stand-in for kornia's `resize` (tools/make_golden_preprocess.py), and its wiring through `extract()` /
`match_pair()`.

Bound of the fixture comparison: max |gpu - ref| <= max(2 err64, (2 (ks_y + ks_x) + 12) 2^-24).  err64 is the reference's own float32 error
(its output against the same definition in float64, stored in the fixture; twice, because two independent float32 evaluations are compared);
the second term is the derived floor for convex combinations of values in [0, 1]: a ks_x-, a ks_y- and two 2-term dot products with rounded
weights, on each side.  Neither comes from the code under test."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import make_golden_preprocess as GP
from conftest import require_gpu

GOLD = Path(__file__).resolve().parent / "golden" / "preprocess"
NAMES = sorted(GP.CASES)


def _pre(case):
    from lightglue_amd import ImagePreprocessor
    return ImagePreprocessor(resize=case["resize"], side=case["side"], antialias=case["antialias"], align_corners=case["align_corners"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_resize_matches_reference(name):
    require_gpu()
    z = np.load(GOLD / f"{name}.npz")
    case = GP.case_from_fixture(z)
    assert case == GP.CASES[name]
    img = GP.preprocess_image(case["seed"], case["dtype"], case["B"], case["C"], case["H"], case["W"]).cuda()
    out, scale = _pre(case)(img)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == tuple(z["out"].shape)
    assert scale.dtype == torch.float32 and scale.device == img.device
    np.testing.assert_array_equal(scale.cpu().numpy(), z["scale"])
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - z["out"].astype(np.float64)).max())
    ks_y, ks_x = (int(v) for v in z["ks"])
    bound = max(2.0 * float(z["err64"]), (2 * (ks_y + ks_x) + 12) * 2.0 ** -24)
    print(f"{name}: max |gpu - ref| {err:.3e}  bound {bound:.3e}  (err64 {float(z['err64']):.3e}, ks {ks_y} x {ks_x})")
    assert err <= bound, f"{name}: {err:.3e} > {bound:.3e}"


@pytest.mark.gpu
def test_input_forms_are_bit_identical():
    """uint8 == float32 of v / 255; a channels-last / cropped strided view == its contiguous copy; [C, H, W] == [1, C, H, W]; identity returns its input."""
    require_gpu()
    from lightglue_amd import ImagePreprocessor
    u8 = GP.preprocess_image(40, "uint8", 2, 3, 201, 333)
    f32 = torch.tensor(u8.numpy() / 255.0, dtype=torch.float)           # the reference's numpy_image_to_torch arithmetic
    for kw in (dict(resize=96), dict(resize=(77, 130), antialias=False), dict(resize=400), dict()):
        pre = ImagePreprocessor(**kw)
        a, sa = pre(u8.cuda()); b, sb = pre(f32.cuda())
        assert a.dtype == torch.float32 and torch.equal(a, b) and torch.equal(sa, sb), kw
    assert torch.equal(ImagePreprocessor()(u8.cuda())[0], f32.cuda())   # no resize: uint8 still goes through the kernel (the / 255 conversion)
    pre = ImagePreprocessor(resize=120)
    for src in (u8.cuda(), f32.cuda()):
        nhwc = src.permute(0, 2, 3, 1).contiguous()                     # what a decoded photo looks like
        view = nhwc.permute(0, 3, 1, 2)
        assert not view.is_contiguous() and view.stride(1) == 1
        assert torch.equal(pre(view)[0], pre(src)[0])
        crop = view[:, :, 5:-7, 3:-11]
        assert torch.equal(pre(crop)[0], pre(crop.contiguous())[0])
        crop = src[1:, :, 10:150, 20:300]
        assert torch.equal(pre(crop)[0], pre(crop.contiguous())[0])
        one = pre(src[0])[0]
        assert one.dim() == 3 and torch.equal(one, pre(src[:1])[0][0])
        gray = src[:, 1:2]                                               # one channel of three, in place
        assert torch.equal(pre(gray)[0], pre(gray.contiguous())[0])
    img = f32[0].cuda()
    for kw in (dict(), dict(resize=333), dict(resize=(201, 333)), dict(resize=201, side="short")):
        same, scale = ImagePreprocessor(**kw)(img)
        assert same is img and scale.tolist() == [1.0, 1.0], kw
    with pytest.raises(TypeError):
        ImagePreprocessor(resize=64)(img.double())
    with pytest.raises(AssertionError, match="LG_PREPROCESS_MAX_TAPS"):
        ImagePreprocessor(resize=8)(img)
    with pytest.raises(AssertionError, match="channels"):
        ImagePreprocessor(resize=64)(f32[:, :2].cuda())


def _extractors():
    import make_golden_aliked as GA
    import make_golden_superpoint as GS
    from lightglue_amd import ALIKED, SuperPoint
    sp = SuperPoint(weights=GS.encoder_state_dict(0), max_num_keypoints=256).cuda().eval()
    al = ALIKED(weights=GA.aliked_state_dict(0, "aliked-n16"), model_name="aliked-n16", detection_threshold=0.5).cuda().eval()
    return (("superpoint", sp, torch.from_numpy(np.clip(GS.encoder_image(10, 1, 240, 320), 0, 1)).cuda()),
            ("aliked", al, GA.aliked_image(0, 1, 240, 320, 3).cuda()))


@pytest.mark.gpu
def test_extract_honours_resize():
    """extract(img, resize=R) == forward on the preprocessed image + extracted_to_image_frame, bit for bit; extract(img) == what it returned before
    (forward on the image itself + image_size)."""
    require_gpu()
    from lightglue_amd import ImagePreprocessor, extracted_to_image_frame
    for kind, ext, img in _extractors():
        h, w = img.shape[-2:]
        for kw in (dict(resize=160), dict(resize=(100, 180), antialias=False), dict(resize=200, side="short")):
            got = ext.extract(img[0], **kw)
            small, scale = ImagePreprocessor(**kw)(img)
            assert tuple(small.shape[-2:]) != (h, w)
            want = extracted_to_image_frame(ext({"image": small}), (h, w), scale)
            assert sorted(got) == sorted(want), kind
            for key in want:
                assert torch.equal(got[key], want[key]), (kind, kw, key)
            assert got["image_size"].tolist() == [[float(w), float(h)]]
            n = int(got["num_keypoints"][0])
            kp = got["keypoints"][0, :n]
            assert n > 20 and bool((kp >= 0).all()) and bool((kp[:, 0] <= w - 1).all()) and bool((kp[:, 1] <= h - 1).all()), (kind, kw)
        got, want = ext.extract(img), ext({"image": img})
        for key in want:
            assert torch.equal(got[key], want[key]), (kind, key)
        assert got["image_size"].tolist() == [[float(w), float(h)]] and got["image_size"].dtype == torch.float32
        same = ext.extract(img, resize=max(h, w))      # a resize that changes nothing is the same as none
        assert torch.equal(same["keypoints"], want["keypoints"])


@pytest.mark.gpu
def test_match_pair_with_resize():
    require_gpu()
    import gpu_util
    import make_golden_superpoint as GS
    from lightglue_amd import SuperPoint, match_pair
    from lightglue_amd import synthetic as synth
    ext = SuperPoint(weights=GS.encoder_state_dict(0), max_num_keypoints=128).cuda().eval()
    img0 = torch.from_numpy(np.clip(GS.encoder_image(10, 1, 240, 320), 0, 1))[0].cuda()
    img1 = torch.roll(img0, shifts=(6, 10), dims=(-2, -1))[:, :230, :300]
    matcher = gpu_util.make_model(synth.make_state_dict(0, recipe="A"), "f16x3", depth_confidence=-1, width_confidence=-1)
    f0, f1, m01 = match_pair(ext, matcher, img0, img1, resize=160)
    assert f0["image_size"].tolist() == [320.0, 240.0] and f1["image_size"].tolist() == [300.0, 230.0]
    assert f0["keypoints"].shape == (128, 2) and f1["descriptors"].shape == (128, 256) and m01["matches0"].shape == (128,) and m01["matches"].shape[1] == 2
    assert float(f0["keypoints"][:, 0].max()) > 160 and float(f0["keypoints"].max()) <= 319        # original frame, not the 120 x 160 one
    g0 = ext.extract(img0, resize=160)
    assert torch.equal(g0["keypoints"][0], f0["keypoints"])


@pytest.mark.gpu
def test_superpoint_extract_matches_reference_end_to_end():
    """The reference class's own extract(img, resize=160) (fixture) under the rules of test_superpoint_full.test_full_extractor_matches_reference."""
    require_gpu()
    from lightglue_amd import SuperPoint
    name = "e2e_superpoint_240x320_to160"
    z = np.load(GOLD / f"{name}.npz")
    meta = json.loads(str(z["meta"]))
    img = GP.e2e_image("superpoint", meta["iseed"], meta["c"], meta["h"], meta["w"]).cuda()
    model = SuperPoint(weights=GP.e2e_state_dict("superpoint", meta["wseed"], meta["conf"]), **meta["conf"]).cuda().eval()
    out = model.extract(img, resize=meta["resize"])
    assert out["image_size"].cpu().numpy().tolist() == z["image_size"].tolist() == [[float(meta["w"]), float(meta["h"])]]
    kp, sc, desc = (out[k][0].cpu().numpy() for k in ("keypoints", "keypoint_scores", "descriptors"))
    n = int(out["num_keypoints"][0])
    ref_kp, ref_sc, ref_desc = z["keypoints"][0], z["keypoint_scores"][0], z["descriptors"][0]
    scale = z["scale"].astype(np.float64)
    cell = lambda k: tuple(int(v) for v in np.rint((k.astype(np.float64) + 0.5) * scale - 0.5))    # the pixel of the resized image the detector fired on
    got = {cell(k): i for i, k in enumerate(kp[:n])}
    ref = {cell(k): i for i, k in enumerate(ref_kp)}
    assert len(got) == n and len(ref) == len(ref_kp)
    common = sorted(set(got) & set(ref))
    print(f"{name}: {n} keypoints, reference {len(ref)}, common {len(common)}")
    assert len(common) >= 0.99 * len(ref) and abs(n - len(ref)) <= max(1, len(ref) // 100), (n, len(ref), len(common))
    gi = np.array([got[c] for c in common]); ri = np.array([ref[c] for c in common])
    print(f"  max |d keypoint| {np.abs(kp[gi] - ref_kp[ri]).max():.2e}  max |d score| {np.abs(sc[gi] - ref_sc[ri]).max():.2e}  max |d desc| {np.abs(desc[gi] - ref_desc[ri]).max():.2e}")
    assert np.abs(kp[gi] - ref_kp[ri]).max() <= 1e-3                    # after the (k + 0.5) / scale - 0.5 map
    np.testing.assert_allclose(sc[gi], ref_sc[ri], atol=2e-6, rtol=2e-5)
    np.testing.assert_allclose(desc[gi], ref_desc[ri], atol=2e-5, rtol=0)
    if len(common) == len(ref) == n:
        np.testing.assert_allclose(kp[:n], ref_kp, atol=1e-3, rtol=0)   # raster order of the resized image


@pytest.mark.gpu
def test_aliked_extract_matches_reference_end_to_end():
    """The reference ALIKED class's own extract(img, resize=160) under test_gpu_aliked._compare."""
    require_gpu()
    from test_gpu_aliked import _compare
    from lightglue_amd import ALIKED
    name = "e2e_aliked_n16_240x320_to160"
    z = np.load(GOLD / f"{name}.npz")
    meta = json.loads(str(z["meta"]))
    conf = dict(meta["conf"])
    img = GP.e2e_image("aliked", meta["iseed"], meta["c"], meta["h"], meta["w"]).cuda()
    model = ALIKED(weights=GP.e2e_state_dict("aliked", meta["wseed"], conf), **conf).eval().cuda()
    out = model.extract(img, resize=meta["resize"])
    assert out["image_size"].cpu().numpy().tolist() == z["image_size"].tolist()
    print(f"{name}: {int(out['num_keypoints'][0])} keypoints, reference {int(z['counts'][0])}, margins {meta['threshold_margin']:.2e} / {meta['nms_tie_margin']:.2e}")
    _compare(meta, {k: z[k] for k in z.files if k != "meta"}, out)


@pytest.mark.gpu
def test_no_framework_kernels_inside_the_preprocessor():
    """Between the start of ImagePreprocessor.__call__ and its return the torch profiler sees memcpy / memset activity and kernels of namespace lg only."""
    require_gpu()
    from torch.profiler import ProfilerActivity, profile
    from lightglue_amd import ImagePreprocessor
    u8 = GP.preprocess_image(41, "uint8", 1, 3, 480, 640).cuda().permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    f32 = GP.preprocess_image(42, "float32", 1, 1, 480, 640).cuda()
    pre = ImagePreprocessor(resize=256)
    pre(u8); pre(f32[0]); torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        pre(u8); pre(f32[0]); pre(f32)
        torch.cuda.synchronize()
    kernels = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.name and "Memset" not in e.name]
    foreign = [k for k in kernels if any(tag in k for tag in ("at::", "at_cuda", "c10::", "rocprim", "hipcub", "elementwise", "Elementwise"))]
    ours = [k for k in kernels if "lg::" in k]
    assert len(ours) == 3 and len(kernels) == 3 and not foreign, f"kernels inside ImagePreprocessor: {sorted(set(kernels))}"
