"""Ragged-batch SuperPoint extraction, the parts that need no GPU: the batch planner of `extract_batch`, the host-side validation of
`valid_size`, and the stage entry points' refusals under `LG_EXTRACT_RAGGED` (null pointers, small canvases) before the device is touched."""
import ctypes

import pytest
import torch

import make_golden_superpoint as G
from lightglue_amd import SuperPoint, _cabi, plan_image_batches
from lightglue_amd.superpoint_head import check_sizes

SIZES = [(96, 160), (75, 109), (67, 91), (40, 64), (41, 65), (17, 33), (8, 8), (160, 96), (75, 109), (96, 160), (120, 40)]


def _check_plan(plan, sizes, batch_size):
    seen = sorted(i for idx, _ in plan for i in idx)
    assert seen == list(range(len(sizes)))                                   # every index exactly once
    for idx, (hc, wc) in plan:
        assert 1 <= len(idx) <= batch_size
        assert hc == max(sizes[i][0] for i in idx) and wc == max(sizes[i][1] for i in idx)    # canvas = the group's elementwise maximum


@pytest.mark.parametrize("order", ["size", "input"])
@pytest.mark.parametrize("batch_size", [1, 3, 8, 64])
def test_planner_covers_every_image_once(batch_size, order):
    plan = plan_image_batches(SIZES, batch_size, order=order)
    _check_plan(plan, SIZES, batch_size)
    assert plan == plan_image_batches(list(SIZES), batch_size, order=order)  # deterministic
    assert len(plan) >= -(-len(SIZES) // batch_size)
    if order == "input":
        assert [i for idx, _ in plan for i in idx] == list(range(len(SIZES)))


def test_planner_groups_equal_sizes_without_padding():
    sizes = [(480, 640), (640, 480)] * 8
    plan = plan_image_batches(sizes, 8)
    _check_plan(plan, sizes, 8)
    assert len(plan) == 2 and all(len({sizes[i] for i in idx}) == 1 for idx, _ in plan)
    mixed = plan_image_batches(sizes, 8, order="input")
    assert [c for _, c in mixed] == [(640, 640), (640, 640)]
    assert plan_image_batches([], 8) == []


def test_planner_honours_the_workspace_cap():
    nbytes = _cabi.load().lg_sp_encode_workspace_bytes
    cap = nbytes(3, 96, 160)
    plan = plan_image_batches(SIZES, 8, max_workspace_bytes=cap)
    _check_plan(plan, SIZES, 8)
    assert all(nbytes(len(idx), hc, wc) <= cap for idx, (hc, wc) in plan)
    assert max(len(idx) for idx, _ in plan) > 1 and len(plan) > len(plan_image_batches(SIZES, 8))
    with pytest.raises(ValueError, match=r"image 7 \(160 x 96\).*max_workspace_bytes"):
        plan_image_batches(SIZES, 8, max_workspace_bytes=nbytes(1, 160, 96) - 1)
    with pytest.raises(ValueError, match="image 0"):
        plan_image_batches([(96, 160)], 8, max_workspace_bytes=nbytes(1, 96, 160) - 1)
    with pytest.raises(ValueError, match="at least 8 x 8"):
        plan_image_batches([(16, 16), (7, 16)], 8)
    with pytest.raises(ValueError):
        plan_image_batches(SIZES, 0)


def test_valid_size_is_validated_on_the_host():
    assert check_sizes([[160, 96], [8, 8]], 2, (96, 160)) == [[160, 96], [8, 8]]
    assert check_sizes(torch.tensor([[160.0, 96.0]]), 1, (96, 160)) == [[160, 96]]           # integer-VALUED is enough
    with pytest.raises(ValueError, match="shape"):
        check_sizes([[160, 96]], 2, (96, 160))
    with pytest.raises(ValueError, match="shape"):
        check_sizes([160, 96], 1, (96, 160))
    with pytest.raises(ValueError, match=r"valid_size\[1\].*minimum"):
        check_sizes([[160, 96], [7, 96]], 2, (96, 160))
    with pytest.raises(ValueError, match=r"valid_size\[1\].*canvas"):
        check_sizes([[160, 96], [160, 97]], 2, (96, 160))
    with pytest.raises(ValueError, match=r"valid_size\[0\].*canvas"):
        check_sizes([[161, 96]], 1, (96, 160))
    with pytest.raises(ValueError, match=r"valid_size\[1\].*integer"):
        check_sizes([[160.0, 96.0], [100.5, 96.0]], 2, (96, 160))
    # forward / encode validate before they look at the device: a bad valid_size is a ValueError, a good one reaches the "no CPU fallback" error
    m = SuperPoint(weights=G.encoder_state_dict(0))
    img = torch.zeros(2, 1, 96, 160)
    for bad in ([[160, 96]], [[160, 96], [4, 96]], [[160, 96], [168, 96]], [[160, 96], [99.5, 96]]):
        with pytest.raises(ValueError, match="valid_size"):
            m({"image": img, "valid_size": bad})
        with pytest.raises(ValueError, match="valid_size"):
            m.encode(img, valid_size=bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m({"image": img, "valid_size": [[160, 96], [109, 75]]})


def test_extract_batch_refuses_empty_sets_and_cpu_tensors():
    m = SuperPoint(weights=G.encoder_state_dict(0))
    with pytest.raises(ValueError, match="at least one image"):
        m.extract_batch([])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.extract_batch([torch.zeros(1, 32, 48), torch.zeros(1, 48, 32)])


def test_ragged_entry_points_refuse_bad_arguments_without_gpu():
    lib = _cabi.load()
    fake = 16
    arr = (ctypes.c_void_p * 24)(*[16] * 24)
    inv = _cabi.LG_ERR_INVALID
    big = 1 << 40
    RAGGED, SPLIT, F16 = _cabi.LG_EXTRACT_RAGGED, _cabi.LG_EXTRACT_SPLIT, _cabi.LG_EXTRACT_DESC_F16

    def encode(**kw):
        io = _cabi.LgSpEncodeIO(**{**dict(batch=2, h=64, w=64, flags=RAGGED, image=fake, sizes=fake, params=arr, workspace=fake, workspace_bytes=big, scores=fake,
                                          desc_map=fake), **kw})
        return lib.lg_sp_encode(ctypes.byref(io), None)
    # lg_sp_encode, LG_EXTRACT_RAGGED: canvas below 8 x 8, batch < 1, null image / sizes / outputs, the split form's 2^25-pixel canvas
    assert encode(h=7) == inv and b"at least 8" in lib.lg_last_error()
    assert encode(w=7, flags=RAGGED | SPLIT) == inv
    assert encode(batch=0) == inv
    assert encode(sizes=None) == inv and b"null pointer" in lib.lg_last_error()
    assert encode(image=None) == inv and b"null pointer" in lib.lg_last_error()
    assert encode(scores=None) == inv
    assert encode(workspace_bytes=16) == inv and b"workspace" in lib.lg_last_error()
    assert encode(batch=1, h=8192, w=4096, flags=RAGGED | SPLIT) == inv and b"2^25" in lib.lg_last_error()

    def detect(**kw):
        io = _cabi.LgSpDetectIO(**{**dict(batch=1, h=64, w=64, flags=RAGGED, scores=fake, sizes=fake, nms_radius=4, remove_borders=4, detection_threshold=0.0005,
                                          max_keypoints=0, capacity=64, max_candidates=4096, workspace=fake, workspace_bytes=big, keypoints=fake, kp_scores=fake,
                                          counts=fake, totals=None), **kw})
        return lib.lg_sp_detect(ctypes.byref(io), None)
    # lg_sp_detect, LG_EXTRACT_RAGGED
    assert detect(sizes=None) == inv and b"null pointer" in lib.lg_last_error()
    assert detect(scores=None) == inv and b"null pointer" in lib.lg_last_error()
    assert detect(h=7) == inv and b"at least 8" in lib.lg_last_error()
    assert detect(batch=0) == inv

    # lg_sp_sample_descriptors, LG_EXTRACT_RAGGED with and without LG_EXTRACT_DESC_F16
    for flags in (RAGGED, RAGGED | F16):
        def sample(**kw):
            io = _cabi.LgSpSampleIO(**{**dict(batch=1, channels=256, h=8, w=8, flags=flags, desc_map=fake, sizes=fake, keypoints=fake, num=None, n=4, cell=8,
                                              normalize_dense=1, workspace=fake, out=fake), **kw})
            return lib.lg_sp_sample_descriptors(ctypes.byref(io), None)
        assert sample(sizes=None) == inv and b"null pointer" in lib.lg_last_error()
        assert sample(desc_map=None) == inv and b"null pointer" in lib.lg_last_error()
        assert sample(batch=0) == inv
        assert sample(h=0) == inv
