"""ALIKED without a GPU: the module tree against the reference's (names / shapes recorded by tools/make_golden_aliked.py), the fixture
tool's deform_conv2d restatement, configuration validation and the C ABI's refusals."""
import ctypes as C
import json
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

import make_golden_aliked as G

GOLD = Path(__file__).resolve().parent / "golden"


@pytest.mark.parametrize("model", ["aliked-n16", "aliked-n32"])
def test_state_dict_matches_reference_tree(model):
    from lightglue_amd import ALIKED
    tree = json.loads((GOLD / "reference_aliked_state_dict.json").read_text())[model]
    got = [[k, list(v.shape)] for k, v in ALIKED(model_name=model).state_dict().items()]
    assert got == tree
    m = ALIKED(weights=G.aliked_state_dict(0, model), model_name=model)   # strict=True load
    assert m.n_pos == (32 if model == "aliked-n32" else 16)


def test_n16rot_has_the_n16_tree():
    from lightglue_amd import ALIKED
    a, b = ALIKED(model_name="aliked-n16rot").state_dict(), ALIKED(model_name="aliked-n16").state_dict()
    assert [(k, v.shape) for k, v in a.items()] == [(k, v.shape) for k, v in b.items()]


def test_config_validation():
    from lightglue_amd import ALIKED
    with pytest.raises(ValueError, match="aliked-t16"):
        ALIKED(model_name="aliked-t16")
    with pytest.raises(ValueError):
        ALIKED(model_name="aliked-x")
    with pytest.raises(ValueError):
        ALIKED(max_num_keypoints=20001)
    with pytest.raises(RuntimeError):   # strict load: a missing name fails
        sd = G.aliked_state_dict(0)
        sd.pop("desc_head.agg_weights")
        ALIKED(weights=sd)
    m = ALIKED()
    assert m._dkd() == (-1, 0.2, 20000)                                 # ref :680-689: threshold mode, n_limit_max
    assert ALIKED(detection_threshold=-1, max_num_keypoints=512)._dkd() == (512, -1.0, 512)
    assert ALIKED(max_num_keypoints=100)._dkd() == (-1, 0.2, 100)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m({"image": torch.zeros(1, 3, 32, 32)})


def test_deform_conv2d_zero_offset_is_conv2d():
    g = torch.Generator().manual_seed(0)
    x, w, b = torch.randn(2, 5, 9, 11, generator=g), torch.randn(7, 5, 3, 3, generator=g), torch.randn(7, generator=g)
    off = torch.zeros(2, 18, 9, 11)
    torch.testing.assert_close(G.deform_conv2d(x, off, w, b, padding=(1, 1)), F.conv2d(x, w, b, padding=1), rtol=1e-5, atol=1e-5)


def test_deform_conv2d_matches_grid_sample_construction():
    """Fractional and out-of-range offsets: every tap sampled with grid_sample (bilinear, zeros, align_corners=True) at the displaced position —
    the same function as torchvision's per-corner bounds rules, which give zero exactly where a corner lies outside the map."""
    g = torch.Generator().manual_seed(1)
    B, Cin, H, W, Cout = 2, 4, 8, 10, 3
    x, w = torch.randn(B, Cin, H, W, generator=g), torch.randn(Cout, Cin, 3, 3, generator=g)
    off = torch.randn(B, 18, H, W, generator=g) * 2.5
    off[:, :, 0, 0] = 40.0   # far outside
    got = G.deform_conv2d(x, off, w, None, padding=(1, 1))
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    cols = []
    for k in range(9):
        i, j = divmod(k, 3)
        py, px = ys - 1 + i + off[:, 2 * k], xs - 1 + j + off[:, 2 * k + 1]
        grid = torch.stack([px / (W - 1) * 2 - 1, py / (H - 1) * 2 - 1], -1)
        cols.append(F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=True))
    ref = torch.einsum("bckhw,ock->bohw", torch.stack(cols, 2), w.reshape(Cout, Cin, 9))
    torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-4)


def test_cabi_refusals_without_gpu():
    from lightglue_amd import _cabi
    lib = _cabi.load()
    assert lib.lg_aliked_packed_bytes(16) > 0 and lib.lg_aliked_packed_bytes(32) > lib.lg_aliked_packed_bytes(16)
    assert lib.lg_aliked_packed_bytes(8) == 0
    assert lib.lg_aliked_workspace_bytes(1, 8192, 4096, 16) == 0          # >= 2^25 padded pixels
    rc = lib.lg_aliked_encode(C.byref(_cabi.LgAlikedEncodeIO(batch=1, channels=3, h=8192, w=4096, n_pos=16)), None)
    assert rc == _cabi.LG_ERR_INVALID and b"2^25" in lib.lg_last_error()
    rc = lib.lg_aliked_encode(C.byref(_cabi.LgAlikedEncodeIO(batch=1, channels=3, h=64, w=64, n_pos=24)), None)
    assert rc == _cabi.LG_ERR_INVALID and b"unknown ALIKED model" in lib.lg_last_error()
    rc = lib.lg_aliked_detect(C.byref(_cabi.LgAlikedDetectIO(batch=1, h=64, w=64, nms_radius=2, scores_th=0.2, top_k=-1, n_limit=20001, capacity=20001)), None)
    assert rc == _cabi.LG_ERR_INVALID and b"20000" in lib.lg_last_error()
    rc = lib.lg_aliked_pack_weights(16, None, 68, None, 0, None)
    assert rc == _cabi.LG_ERR_INVALID
    # encode workspace + level maps of a 1024 x 768 image: far below the 128-channel dense map (which is never written)
    b, h, w = 1, 768, 1024
    assert lib.lg_aliked_workspace_bytes(b, h, w, 16) + lib.lg_aliked_levels_bytes(b, h, w) < b * h * w * 128 * 4


@pytest.mark.parametrize("shape", [(1, 8, 8), (2, 31, 33), (3, 40, 56), (1, 40, 300), (2, 64, 96)])
def test_level_maps_views_tile_the_buffer(shape):
    """ALIKED.level_maps restates lg_aliked.hip's level layout: its total is lg_aliked_levels_bytes (asserted inside), the views are
    [B, Hp >> s, Wp >> s, 32] at 256-byte aligned offsets, they share the buffer's memory and do not overlap."""
    from lightglue_amd import ALIKED, _cabi
    b, h, w = shape
    buf = torch.zeros(_cabi.load().lg_aliked_levels_bytes(b, h, w), dtype=torch.uint8)
    maps = ALIKED.level_maps(buf, shape)
    hp, wp = (h + 31) // 32 * 32, (w + 31) // 32 * 32
    assert [tuple(m.shape) for m in maps] == [(b, hp >> s, wp >> s, 32) for s in (0, 1, 3, 5)]
    for i, m in enumerate(maps):
        assert m.dtype == torch.float32 and m.is_contiguous() and (m.data_ptr() - buf.data_ptr()) % 256 == 0
        m.fill_(float(i + 1))
    for i, m in enumerate(maps):
        assert (m == float(i + 1)).all()
        assert i == 0 or m.data_ptr() >= maps[i - 1].data_ptr() + 4 * maps[i - 1].numel()
    with pytest.raises(AssertionError, match="level layout"):
        ALIKED.level_maps(buf[:-256], shape)
