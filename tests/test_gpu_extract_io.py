"""Every flag combination the six extractor stages accept (include/lightglue_amd.h LG_EXTRACT_*), reached through the Python API on one small case: two images
whose sizes are multiples of neither 8 nor 32 — 41 x 65 and 33 x 57, where SuperPoint's cell cropping and ALIKED's per-image padding have something to do — on
their common canvas, the padding NaN.
  lg_sp_encode              {uniform, ragged} x {fp32, split}     the crops / the canvas, per conv_precision
  lg_sp_detect              {uniform, ragged}
  lg_sp_sample_descriptors  {uniform, ragged} x {f32, f16}
  lg_aliked_encode, lg_aliked_detect   {uniform, ragged}
  lg_aliked_describe        {uniform, ragged} x {f32, f16}
Bit identity (torch.equal on every output key): the rows of the ragged call equal the B = 1 call on the crop, and float16 descriptors equal `.half()` of the
fp32 ones with every other key unchanged."""
import pytest
import torch

import make_golden_aliked as GA
import make_golden_superpoint as GS
from conftest import require_gpu

SIZES = [(41, 65), (33, 57)]      # (h, w)
CANVAS = (41, 65)
KEYS = ("keypoints", "keypoint_scores", "descriptors")


def _canvas(images):
    c = torch.full((len(images), images[0].shape[1]) + CANVAS, float("nan"), device="cuda")
    for b, im in enumerate(images):
        c[b, :, : im.shape[-2], : im.shape[-1]] = im[0]
    return c


def _check(make, images):
    """make(dtype) -> extractor.  The four calls {crop, canvas} x {float32, float16} against each other."""
    canvas, valid = _canvas(images), [[w, h] for h, w in SIZES]
    out = {}
    for name, dtype in (("f32", torch.float32), ("f16", torch.float16)):
        model = make(dtype)
        out[name] = (model({"image": canvas, "valid_size": valid}), [model({"image": im}) for im in images])
    counts = []
    for name, (ragged, crops) in out.items():
        assert ragged["descriptors"].dtype is (torch.float16 if name == "f16" else torch.float32)
        for b, ref in enumerate(crops):      # ragged rows == the B = 1 call on the crop
            n = int(ref["num_keypoints"][0])
            assert int(ragged["num_keypoints"][b]) == n, (name, b)
            for k in KEYS:
                assert ragged[k].dtype is ref[k].dtype and torch.equal(ragged[k][b, :n], ref[k][0, :n]), (name, k, b)
                assert not ragged[k][b, n:].any(), (name, k, b)
            counts.append(n)
    for f16, f32 in [(out["f16"][0], out["f32"][0])] + list(zip(out["f16"][1], out["f32"][1])):      # float16 == .half() of fp32, ragged and uniform
        assert sorted(f16) == sorted(f32)
        for k in f32:
            assert torch.equal(f16[k], f32[k].half() if k == "descriptors" else f32[k]), k
    print("keypoints per image (f32 ragged, f16 ragged):", counts)
    assert max(counts) > 0, counts      # there are rows to compare


@pytest.mark.gpu
@pytest.mark.parametrize("conv_precision", ["fp32", "f16x3"])
def test_superpoint_flag_combinations(conv_precision):
    require_gpu()
    from lightglue_amd import SuperPoint
    sd = GS.encoder_state_dict(0)
    images = [torch.from_numpy(GS.encoder_image(30 + i, 1, h, w)).cuda() for i, (h, w) in enumerate(SIZES)]
    _check(lambda dtype: SuperPoint(weights=sd, conv_precision=conv_precision, max_num_keypoints=50, descriptor_dtype=dtype).cuda().eval(), images)


@pytest.mark.gpu
def test_aliked_flag_combinations():
    require_gpu()
    from lightglue_amd import ALIKED
    sd = GA.aliked_state_dict(3, "aliked-n16")
    images = [GA.aliked_image(50 + i, 1, h, w, 3).cuda() for i, (h, w) in enumerate(SIZES)]
    _check(lambda dtype: ALIKED(weights=sd, model_name="aliked-n16", detection_threshold=0.2, descriptor_dtype=dtype).eval().cuda(), images)
