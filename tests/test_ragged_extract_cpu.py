"""Ragged-batch SuperPoint extraction, the parts that need no GPU: the batch planner of `extract_batch`, the host-side validation of
`valid_size`, and the `*_ragged` entry points' refusals (null pointers, small canvases) before the device is touched."""
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
    fake = ctypes.c_void_p(16)
    arr = (ctypes.c_void_p * 24)(*[16] * 24)
    inv = _cabi.LG_ERR_INVALID
    big = 1 << 40
    # lg_sp_encode_ragged: canvas below 8 x 8, batch < 1, null image / sizes / outputs, the split form's 2^25-pixel canvas
    assert lib.lg_sp_encode_ragged(fake, 2, 7, 64, fake, arr, fake, big, fake, fake, 0, None) == inv and b"at least 8" in lib.lg_last_error()
    assert lib.lg_sp_encode_ragged(fake, 2, 64, 7, fake, arr, fake, big, fake, fake, 1, None) == inv
    assert lib.lg_sp_encode_ragged(fake, 0, 64, 64, fake, arr, fake, big, fake, fake, 0, None) == inv
    assert lib.lg_sp_encode_ragged(fake, 2, 64, 64, None, arr, fake, big, fake, fake, 0, None) == inv and b"null pointer" in lib.lg_last_error()
    assert lib.lg_sp_encode_ragged(None, 2, 64, 64, fake, arr, fake, big, fake, fake, 0, None) == inv and b"null pointer" in lib.lg_last_error()
    assert lib.lg_sp_encode_ragged(fake, 2, 64, 64, fake, arr, fake, big, None, fake, 0, None) == inv
    assert lib.lg_sp_encode_ragged(fake, 2, 64, 64, fake, arr, fake, 16, fake, fake, 0, None) == inv and b"workspace" in lib.lg_last_error()
    assert lib.lg_sp_encode_ragged(fake, 1, 8192, 4096, fake, arr, fake, big, fake, fake, 1, None) == inv and b"2^25" in lib.lg_last_error()
    # lg_sp_detect_ragged
    tail = (4, 4, 0.0005, 0, 64, 4096, fake, big, fake, fake, fake, None, None)
    assert lib.lg_sp_detect_ragged(fake, 1, 64, 64, None, *tail) == inv and b"null pointer" in lib.lg_last_error()
    assert lib.lg_sp_detect_ragged(None, 1, 64, 64, fake, *tail) == inv and b"null pointer" in lib.lg_last_error()
    assert lib.lg_sp_detect_ragged(fake, 1, 7, 64, fake, *tail) == inv and b"at least 8" in lib.lg_last_error()
    assert lib.lg_sp_detect_ragged(fake, 0, 64, 64, fake, *tail) == inv
    # lg_sp_sample_descriptors_ragged / _half
    for fn in (lib.lg_sp_sample_descriptors_ragged, lib.lg_sp_sample_descriptors_ragged_half):
        assert fn(fake, 1, 256, 8, 8, None, fake, None, 4, 8, 1, fake, fake, None) == inv and b"null pointer" in lib.lg_last_error()
        assert fn(None, 1, 256, 8, 8, fake, fake, None, 4, 8, 1, fake, fake, None) == inv and b"null pointer" in lib.lg_last_error()
        assert fn(fake, 0, 256, 8, 8, fake, fake, None, 4, 8, 1, fake, fake, None) == inv
        assert fn(fake, 1, 256, 0, 8, fake, fake, None, 4, 8, 1, fake, fake, None) == inv
