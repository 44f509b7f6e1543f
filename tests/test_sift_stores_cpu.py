"""SIFT feature stores, the parts that need no GPU: the C ABI's flags and refusals (LG_FLAG_DESC*_U8 / LG_FLAG_ROOTSIFT*, lg_rootsift, lg_sift_filter), the dtype
and `descriptor_transform` rules of the Python plumbing, and the reference's own outputs (tests/golden/sift/sift_helpers.npz, written by tools/make_golden_sift.py
with the reference's filter_dog_point / sift_to_rootsift) against the CPU branch of `sift_to_rootsift` and a numpy restatement of the filter's rules — the
rules include/lightglue_amd.h states for lg_sift_filter, which tests/test_gpu_sift_stores.py then holds the device to."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import lightglue_amd
from lightglue_amd import _cabi, collate_features, sift_to_rootsift
from lightglue_amd._call import normalise_side

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "lightglue_amd.h").read_text()
GOLDEN = np.load(ROOT / "tests" / "golden" / "sift" / "sift_helpers.npz")
NEW_FLAGS = (("LG_FLAG_DESC0_U8", 64), ("LG_FLAG_DESC1_U8", 128), ("LG_FLAG_ROOTSIFT0", 256), ("LG_FLAG_ROOTSIFT1", 512))


def test_flags_and_entry_points_are_declared_bound_and_exported():
    for name, value in NEW_FLAGS:
        assert int(re.search(r"#define %s (\d+)u" % name, HEADER).group(1)) == value == getattr(_cabi, name)
    flags = [_cabi.LG_FLAG_NO_PRUNING, _cabi.LG_FLAG_EXT, _cabi.LG_FLAG_CHECK_FINITE, _cabi.LG_FLAG_INDEXED, _cabi.LG_FLAG_DESC0_F16, _cabi.LG_FLAG_DESC1_F16]
    flags += [getattr(_cabi, name) for name, _ in NEW_FLAGS]
    assert sorted(flags) == [1 << i for i in range(10)]
    lib = _cabi.load()
    for fn in ("lg_rootsift", "lg_sift_filter", "lg_sift_filter_workspace_bytes"):
        assert re.search(r"\b(int|int64_t) %s\(" % fn, HEADER) and fn in _cabi.EXPORTED_SYMBOLS and getattr(lib, fn) is not None
    for name in ("sift_to_rootsift", "filter_dog_point", "sift_features"):
        assert name in lightglue_amd.__all__ and callable(getattr(lightglue_amd, name))


def _engine(input_dim=128):
    lib, h = _cabi.load(), ctypes.c_void_p()
    cfg = _cabi.LgConfig(input_dim, 256, 9, 4, 1, 0.95, 0.99, 0.1, -1, 4, -1)
    assert lib.lg_engine_create(ctypes.byref(cfg), ctypes.byref(h)) == _cabi.LG_OK
    return lib, h


def test_sift_store_flags_are_refused_without_touching_a_gpu():
    """The pattern of tests/test_f16_descriptors_cpu.py: LG_ERR_INVALID with a message on an engine WITHOUT weights, so ahead of any state, allocation or launch;
    a call that passes the argument checks reaches the engine's state and is LG_ERR_STATE."""
    lib, h = _engine()
    io = _cabi.LgForwardIO()
    io.batch, io.n0, io.n1 = 1, 4, 4
    io.desc0 = io.desc1 = 4096
    every = [getattr(_cabi, name) for name, _ in NEW_FLAGS]
    for flag in every + [sum(every)]:
        io.flags = flag                                                   # without LG_FLAG_EXT
        assert lib.lg_engine_forward(h, ctypes.byref(io), None) == _cabi.LG_ERR_INVALID and b"LG_FLAG_EXT" in lib.lg_last_error()
    for u8, f16 in ((_cabi.LG_FLAG_DESC0_U8, _cabi.LG_FLAG_DESC0_F16), (_cabi.LG_FLAG_DESC1_U8, _cabi.LG_FLAG_DESC1_F16)):
        io.flags = _cabi.LG_FLAG_EXT | u8 | f16                           # one store, two formats
        assert lib.lg_engine_forward(h, ctypes.byref(io), None) == _cabi.LG_ERR_INVALID and b"one side" in lib.lg_last_error()
    io.flags = _cabi.LG_FLAG_EXT | _cabi.LG_FLAG_DESC0_U8 | _cabi.LG_FLAG_DESC1_F16     # a uint8 store joined with a float16 one is fine
    assert lib.lg_engine_forward(h, ctypes.byref(io), None) == _cabi.LG_ERR_STATE
    for flag, field in ((_cabi.LG_FLAG_DESC0_U8, "desc0"), (_cabi.LG_FLAG_DESC1_U8, "desc1")):
        io.flags = _cabi.LG_FLAG_EXT | flag
        io.desc0 = io.desc1 = 4096
        setattr(io, field, 4096 + 4)                                      # 4-byte aligned: enough for the loads, refused by the rule
        assert lib.lg_engine_forward(h, ctypes.byref(io), None) == _cabi.LG_ERR_INVALID and b"16-byte aligned" in lib.lg_last_error()
        other = _cabi.LG_FLAG_DESC1_U8 if flag == _cabi.LG_FLAG_DESC0_U8 else _cabi.LG_FLAG_DESC0_U8
        rs = _cabi.LG_FLAG_ROOTSIFT0 if flag == _cabi.LG_FLAG_DESC0_U8 else _cabi.LG_FLAG_ROOTSIFT1
        io.flags = _cabi.LG_FLAG_EXT | other | rs                         # the misaligned side is fp32 + RootSIFT now: past the argument checks
        assert lib.lg_engine_forward(h, ctypes.byref(io), None) == _cabi.LG_ERR_STATE
    io.flags, io.desc0, io.desc1 = _cabi.LG_FLAG_EXT | sum(every), 4096, 8192
    assert lib.lg_engine_forward(h, ctypes.byref(io), None) == _cabi.LG_ERR_STATE
    lib.lg_engine_destroy(h)
    # input_dim % 4 != 0 cannot reach a forward: no engine exists for it (input_dim is a multiple of 64), so the check in check_forward_io is a second line
    bad = _cabi.LgConfig(130, 256, 9, 4, 1, 0.95, 0.99, 0.1, -1, 4, -1)
    assert lib.lg_engine_create(ctypes.byref(bad), ctypes.byref(h)) == _cabi.LG_ERR_INVALID and b"input_dim" in lib.lg_last_error()
    lib, h = _engine(320)                                                 # RootSIFT holds a row in one wave: 256 values at most
    io.flags = _cabi.LG_FLAG_EXT | _cabi.LG_FLAG_ROOTSIFT1
    assert lib.lg_engine_forward(h, ctypes.byref(io), None) == _cabi.LG_ERR_INVALID and b"at most 256" in lib.lg_last_error()
    io.flags = _cabi.LG_FLAG_EXT | _cabi.LG_FLAG_DESC0_U8                 # uint8 rows alone have no such limit
    assert lib.lg_engine_forward(h, ctypes.byref(io), None) == _cabi.LG_ERR_STATE
    lib.lg_engine_destroy(h)


def test_helper_entry_points_refuse_bad_arguments_without_touching_a_gpu():
    lib = _cabi.load()
    p = ctypes.c_void_p(4096)
    assert lib.lg_rootsift(p, 0, 0, 128, p, 0, None) == _cabi.LG_OK                                  # no rows: a no-op
    for kind, dim, word in ((3, 128, b"src_kind"), (0, 130, b"dim"), (0, 260, b"dim"), (0, 0, b"dim")):
        assert lib.lg_rootsift(p, kind, 5, dim, p, 0, None) == _cabi.LG_ERR_INVALID and word in lib.lg_last_error()
    assert lib.lg_rootsift(None, 2, 5, 128, p, 0, None) == _cabi.LG_ERR_INVALID and b"null" in lib.lg_last_error()
    assert lib.lg_rootsift(ctypes.c_void_p(4096 + 4), 0, 5, 128, p, 0, None) == _cabi.LG_ERR_INVALID and b"aligned" in lib.lg_last_error()
    assert lib.lg_rootsift(p, 2, 5, 128, ctypes.c_void_p(4096 + 8), 0, None) == _cabi.LG_ERR_INVALID and b"aligned" in lib.lg_last_error()
    need = lib.lg_sift_filter_workspace_bytes(2, 300, 24, 40)
    assert need >= 2 * 2 * 24 * 40 * 4 + 2 * 300 and need % 256 == 0
    assert lib.lg_sift_filter_workspace_bytes(0, 300, 24, 40) == 0 and lib.lg_sift_filter_workspace_bytes(1, 300, 65536, 65536) == 0
    args = lambda ws_bytes, radius=1, images=2: (p, p, p, None, None, p, images, 300, 24, 40, radius, p, ws_bytes, p, p, None)
    assert lib.lg_sift_filter(*args(need - 1)) == _cabi.LG_ERR_INVALID and b"workspace" in lib.lg_last_error()
    assert lib.lg_sift_filter(*args(need, radius=-1)) == _cabi.LG_ERR_INVALID and b"nms_radius" in lib.lg_last_error()
    assert lib.lg_sift_filter(*args(need, images=0)) == _cabi.LG_ERR_INVALID and b"images" in lib.lg_last_error()
    assert lib.lg_sift_filter(p, p, p, None, None, None, 2, 300, 24, 40, 1, p, need, p, p, None) == _cabi.LG_ERR_INVALID and b"null" in lib.lg_last_error()


def _feats(K=2, N=3, dim=8, dtype=torch.uint8, **extra):
    return {"keypoints": torch.zeros(K, N, 2), "descriptors": torch.arange(K * N * dim).reshape(K, N, dim).to(dtype), **extra}


def test_normalise_side_passes_uint8_through_and_reads_the_transform():
    cpu = torch.device("cpu")
    f = _feats()
    s = normalise_side(f, cpu, 8, False)
    assert s.desc.dtype is torch.uint8 and s.desc.data_ptr() == f["descriptors"].data_ptr() and s.desc_u8 and not s.desc_f16 and not s.rootsift
    s = normalise_side(_feats(descriptor_transform="rootsift"), cpu, 8, False)
    assert s.desc_u8 and s.rootsift
    assert not normalise_side(_feats(descriptor_transform=None), cpu, 8, False).rootsift
    for dtype, want in ((torch.float16, (True, False)), (torch.float32, (False, False)), (torch.float64, (False, False))):
        s = normalise_side(_feats(dtype=dtype, descriptor_transform="rootsift"), cpu, 8, False)
        assert (s.desc_f16, s.desc_u8) == want and s.rootsift and s.desc.dtype is (dtype if dtype is not torch.float64 else torch.float32)
    nc = f["descriptors"].transpose(1, 2).contiguous().transpose(1, 2)    # not contiguous: ONE uint8 copy
    s = normalise_side({**f, "descriptors": nc}, cpu, 8, False)
    assert s.desc.dtype is torch.uint8 and s.desc.is_contiguous() and s.desc_u8 and torch.equal(s.desc, f["descriptors"])
    odd = torch.zeros(4 + 48, dtype=torch.uint8)[4:].view(2, 3, 8)        # 4 bytes off a 16-byte boundary: copied, still uint8
    s = normalise_side({**f, "descriptors": odd}, cpu, 8, False)
    assert s.desc.dtype is torch.uint8 and s.desc.data_ptr() % 16 == 0 and s.desc_u8
    for bad in ("l2", "RootSIFT", 1):
        with pytest.raises(ValueError, match="descriptor_transform"):
            normalise_side(_feats(descriptor_transform=bad), cpu, 8, False)


def test_the_transform_is_per_side():
    """Each side of a call reads its own dict: the flags LightGlue._launch sets come from s0 / s1 separately."""
    cpu = torch.device("cpu")
    plain, root = _feats(dtype=torch.float32), _feats(descriptor_transform="rootsift")
    s0, s1 = normalise_side(plain, cpu, 8, False), normalise_side(root, cpu, 8, False)
    assert (s0.desc_u8, s0.rootsift, s1.desc_u8, s1.rootsift) == (False, False, True, True)
    from lightglue_amd.parallel import _take
    part = _take({"image0": plain, "image1": root}, slice(1, 2))          # the pair-sharded matcher's shard of a batch keeps the key
    assert part["image1"]["descriptor_transform"] == "rootsift" and part["image1"]["descriptors"].shape == (1, 3, 8) and "descriptor_transform" not in part["image0"]
    part = _take({"image0": plain, "image1": root}, torch.tensor([1]))
    assert part["image1"]["descriptor_transform"] == "rootsift" and part["image1"]["descriptors"].dtype is torch.uint8


def _item(n, dtype, fill, **extra):
    return {"keypoints": torch.zeros(n, 2), "descriptors": torch.full((n, 8), fill, dtype=dtype), **extra}


def test_collate_features_dtype_and_transform_rules():
    both = collate_features([_item(3, torch.uint8, 200), _item(2, torch.uint8, 7)])
    assert both["descriptors"].dtype is torch.uint8 and both["descriptors"].shape == (2, 3, 8) and both["num_keypoints"].tolist() == [3, 2]
    assert int(both["descriptors"][1, 1, 0]) == 7 and int(both["descriptors"][1, 2, 0]) == 0 and "descriptor_transform" not in both
    for items in ([_item(3, torch.uint8, 200), _item(2, torch.float32, 0.5)], [_item(2, torch.float32, 0.5), _item(3, torch.uint8, 200)],
                  [_item(3, torch.uint8, 200), _item(2, torch.float16, 0.5)], [_item(2, torch.float16, 0.5), _item(3, torch.uint8, 200)]):
        out = collate_features(items)
        assert out["descriptors"].dtype is torch.float32
        b = 0 if items[0]["descriptors"].dtype is torch.uint8 else 1
        assert float(out["descriptors"][b, 0, 0]) == 200.0 and float(out["descriptors"][1 - b, 0, 0]) == 0.5
    t = dict(descriptor_transform="rootsift")
    out = collate_features([_item(3, torch.uint8, 1, **t), _item(2, torch.uint8, 2, **t)])
    assert out["descriptor_transform"] == "rootsift" and out["descriptors"].dtype is torch.uint8
    batched = {"keypoints": torch.zeros(1, 3, 2), "descriptors": torch.ones(1, 3, 8, dtype=torch.uint8), **t}    # an item with its batch dimension of 1
    assert collate_features([batched, batched])["descriptor_transform"] == "rootsift"
    assert "descriptor_transform" not in collate_features([_item(3, torch.uint8, 1, descriptor_transform=None), _item(2, torch.uint8, 2)])
    with pytest.raises(ValueError, match="descriptor_transform"):
        collate_features([_item(3, torch.uint8, 1, **t), _item(2, torch.uint8, 2)])
    with pytest.raises(ValueError, match="descriptor_transform"):
        collate_features([_item(3, torch.uint8, 1, descriptor_transform="l2")])


def test_batch_to_device_leaves_the_transform_alone():
    from lightglue_amd import batch_to_device
    out = batch_to_device(collate_features([_item(3, torch.uint8, 1, descriptor_transform="rootsift")]), "cpu")
    assert out["descriptor_transform"] == "rootsift" and out["descriptors"].dtype is torch.uint8 and out["descriptors"].element_size() == 1


def test_cpu_rootsift_equals_the_reference():
    for key in ("desc", "desc64"):
        x = torch.from_numpy(GOLDEN[key])
        want = torch.from_numpy(GOLDEN[f"rootsift_{key}"])
        for given in (x, x.float(), x.half()):                            # 0 .. 255 is exact in all three
            got = sift_to_rootsift(given)
            assert got.dtype is torch.float32 and torch.equal(got, want), key
        assert torch.equal(sift_to_rootsift(x, out_dtype=torch.float16), want.half())
    keep = x.float()
    sift_to_rootsift(keep)
    assert torch.equal(keep, x.float()), "the input is not written"
    assert np.allclose(GOLDEN["rootsift_desc"][0], 1 / np.sqrt(128), rtol=1e-6, atol=0)       # the all-zero row: clip makes it uniform
    with pytest.raises(ValueError, match="out_dtype"):
        sift_to_rootsift(x, out_dtype=torch.bfloat16)


def numpy_filter(points, scales, angles, shape, radius, scores=None):
    """filter_dog_point's rules as include/lightglue_amd.h states them for lg_sift_filter, in plain loops: nothing of the reference's buffers or pooling."""
    h, w = shape
    s = scales if scores is None else scores
    pix = [(int(np.round(y - np.float32(0.5))), int(np.round(x - np.float32(0.5)))) for x, y in points]
    inside = [0 <= r < h and 0 <= c < w for r, c in pix]
    m1 = {}
    for i, p in enumerate(pix):
        if inside[i]:
            m1[p] = max(m1.get(p, np.float32(0)), s[i])
    k1 = [i for i, p in enumerate(pix) if inside[i] and s[i] == m1[p]]
    m2 = {}
    for i in k1:
        m2[pix[i]] = min(m2.get(pix[i], np.float32(np.inf)), abs(angles[i]))
    k2 = [i for i in k1 if abs(angles[i]) == m2[pix[i]]]
    if radius > 0:
        kept = {pix[i]: s[i] for i in k2}
        def window_max(r, c):
            return max(kept.get((y, x), np.float32(0)) for y in range(max(r - radius, 0), min(r + radius, h - 1) + 1)
                       for x in range(max(c - radius, 0), min(c + radius, w - 1) + 1))
        k2 = [i for i in k2 if kept[pix[i]] == window_max(*pix[i])]
    return np.array(k2, dtype=np.int64)


@pytest.mark.parametrize("image", ["a", "b"])
@pytest.mark.parametrize("by", ["scale", "score"])
@pytest.mark.parametrize("radius", [0, 1, 3])
def test_the_stated_rules_reproduce_the_reference(radius, by, image):
    g = GOLDEN
    want = g[f"keep_{image}_r{radius}_{by}"]
    n = len(g[f"points_{image}"])
    got = numpy_filter(g[f"points_{image}"], g[f"scales_{image}"], g[f"angles_{image}"], tuple(g[f"shape_{image}"]), radius, g[f"scores_{image}"] if by == "score" else None)
    assert 0 < len(want) < n and np.array_equal(got, want)
    assert (np.diff(want) > 0).all(), "ascending: np.where's order"


def test_golden_inputs_are_what_the_tests_need():
    g = GOLDEN
    assert g["points_a"].shape == (300, 2) and tuple(g["shape_a"]) == (24, 40) and g["points_b"].shape == (200, 2) and tuple(g["shape_b"]) == (17, 23)
    assert all(g[k].dtype == np.float32 for k in ("points_a", "scales_a", "angles_a", "scores_a"))
    assert len(np.unique(g["scores_a"])) == 300 and (g["scores_a"] < 0).any(), "distinct scores (no ties for top-k), some of them negative"
    assert len(np.unique(g["points_a"], axis=0)) <= 150, "half of the detections repeat another one's point"
    d = g["desc"]
    assert d.dtype == np.uint8 and d.shape == (300, 128) and not d[0].any() and (d[1] > 0).sum() == 1 and d[1].max() == 255 and (d[2] == 255).all()
    counts = [len(g[f"keep_a_r{r}_score"]) for r in (0, 1, 3)]
    assert counts[0] > counts[1] > counts[2] > 0 and counts[0] > int(g["topk"]) == len(g["topk_a"])
    keep0 = g["keep_a_r0_score"]
    order = keep0[np.argsort(-g["scores_a"][keep0], kind="stable")][: int(g["topk"])]
    assert np.array_equal(g["topk_a"], order), "torch.topk's order: descending score"
