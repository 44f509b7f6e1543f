"""float16 descriptors, the parts that need no GPU: the C ABI's declarations and argument checks, the dtype rules of the Python plumbing, and what the storage
format costs — the numpy oracle on float16-rounded descriptors against the reference's golden outputs (tools/f16_descriptor_drift.py)."""
import ctypes
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from lightglue_amd import ALIKED, SuperPoint, _cabi, collate_features, superpoint_head

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "lightglue_amd.h").read_text()


def test_flags_and_entry_points_are_declared_bound_and_exported():
    for name, value in (("LG_FLAG_DESC0_F16", 16), ("LG_FLAG_DESC1_F16", 32)):
        assert int(re.search(r"#define %s (\d+)u" % name, HEADER).group(1)) == value == getattr(_cabi, name)
    flags = [_cabi.LG_FLAG_NO_PRUNING, _cabi.LG_FLAG_EXT, _cabi.LG_FLAG_CHECK_FINITE, _cabi.LG_FLAG_INDEXED, _cabi.LG_FLAG_DESC0_F16, _cabi.LG_FLAG_DESC1_F16]
    assert sorted(flags) == [1, 2, 4, 8, 16, 32]
    # the extractors' binary16 output is a flag of the two descriptor stages' io (tests/test_cabi_symbols.py checks the structs and the flag values
    # against the header, and that exactly these two stages accept the bit): the output fields are void*, the flag says which element type
    assert int(re.search(r"#define LG_EXTRACT_DESC_F16\s+(\d+)u", HEADER).group(1)) == _cabi.LG_EXTRACT_DESC_F16
    lib = _cabi.load()
    for fn, mirror, field in (("lg_sp_sample_descriptors", _cabi.LgSpSampleIO, "out"), ("lg_aliked_describe", _cabi.LgAlikedDescribeIO, "descriptors")):
        assert fn in _cabi.EXPORTED_SYMBOLS and getattr(lib, fn).argtypes == [ctypes.POINTER(mirror), ctypes.c_void_p]
        assert dict(mirror._fields_)[field] is ctypes.c_void_p and re.search(r"void \*%s;" % field, HEADER)


def test_float16_flags_are_refused_without_touching_a_gpu():
    """The pattern of tests/test_cabi_symbols.py::test_envelope_is_refused_without_touching_a_gpu: LG_ERR_INVALID with a message ahead of any state, allocation or launch."""
    lib = _cabi.load()
    h = ctypes.c_void_p()
    cfg = _cabi.LgConfig(256, 256, 9, 4, 0, 0.95, 0.99, 0.1, -1, 4, -1)
    assert lib.lg_engine_create(ctypes.byref(cfg), ctypes.byref(h)) == _cabi.LG_OK
    io = _cabi.LgForwardIO()
    io.batch, io.n0, io.n1 = 1, 4, 4
    io.desc0 = io.desc1 = 4096
    for flag in (_cabi.LG_FLAG_DESC0_F16, _cabi.LG_FLAG_DESC1_F16, _cabi.LG_FLAG_DESC0_F16 | _cabi.LG_FLAG_DESC1_F16):
        io.flags = flag                                                   # without LG_FLAG_EXT
        assert lib.lg_engine_forward(h, ctypes.byref(io), None) == _cabi.LG_ERR_INVALID and b"LG_FLAG_EXT" in lib.lg_last_error()
    for flag, field in ((_cabi.LG_FLAG_DESC0_F16, "desc0"), (_cabi.LG_FLAG_DESC1_F16, "desc1")):
        io.flags = _cabi.LG_FLAG_EXT | flag
        io.desc0 = io.desc1 = 4096
        setattr(io, field, 4096 + 8)                                      # 8-byte aligned: fine for fp32 rows, refused for the 16-byte loads of float16 rows
        assert lib.lg_engine_forward(h, ctypes.byref(io), None) == _cabi.LG_ERR_INVALID and b"16-byte aligned" in lib.lg_last_error()
        other = _cabi.LG_FLAG_DESC1_F16 if flag == _cabi.LG_FLAG_DESC0_F16 else _cabi.LG_FLAG_DESC0_F16
        io.flags = _cabi.LG_FLAG_EXT | other                              # the misaligned side is fp32 now: past the argument check, the engine has no weights
        assert lib.lg_engine_forward(h, ctypes.byref(io), None) == _cabi.LG_ERR_STATE
    io.flags, io.desc0, io.desc1 = _cabi.LG_FLAG_EXT | _cabi.LG_FLAG_DESC0_F16 | _cabi.LG_FLAG_DESC1_F16, 4096, 8192
    assert lib.lg_engine_forward(h, ctypes.byref(io), None) == _cabi.LG_ERR_STATE
    lib.lg_engine_destroy(h)


def _feat(n, dtype, fill):
    return {"keypoints": torch.zeros(n, 2), "descriptors": torch.full((n, 8), fill, dtype=dtype)}


def test_collate_features_dtype_rule():
    """float16 only if EVERY item's descriptors are float16, otherwise fp32 — in either order, without rounding the fp32 items."""
    x = 1.0 + 2.0 ** -20                                                  # fp32 keeps it, float16 rounds it to 1
    both = collate_features([_feat(3, torch.float16, 0.5), _feat(2, torch.float16, 0.25)])
    assert both["descriptors"].dtype is torch.float16 and both["descriptors"].shape == (2, 3, 8) and both["num_keypoints"].tolist() == [3, 2]
    assert float(both["descriptors"][1, 1, 0]) == 0.25 and float(both["descriptors"][1, 2, 0]) == 0.0
    for items in ([_feat(3, torch.float16, 0.5), _feat(2, torch.float32, x)], [_feat(2, torch.float32, x), _feat(3, torch.float16, 0.5)]):
        out = collate_features(items)
        assert out["descriptors"].dtype is torch.float32
        b = 1 if items[1]["descriptors"].dtype is torch.float32 else 0
        assert float(out["descriptors"][b, 0, 0]) == x and float(out["descriptors"][1 - b, 0, 0]) == 0.5
    assert collate_features([_feat(3, torch.float32, x), _feat(2, torch.float32, x)])["descriptors"].dtype is torch.float32
    assert both["keypoints"].dtype is torch.float32


def test_descriptor_dtype_is_checked():
    for dtype in (torch.bfloat16, torch.float64, "float16"):
        with pytest.raises(ValueError, match="descriptor_dtype"):
            SuperPoint(descriptor_dtype=dtype)
        with pytest.raises(ValueError, match="descriptor_dtype"):
            ALIKED(descriptor_dtype=dtype)
    with pytest.raises(ValueError, match="descriptor_dtype"):
        superpoint_head.descriptor_head(torch.zeros(1, 4, 2), torch.zeros(1, 256, 8, 8), dtype=torch.bfloat16)
    assert SuperPoint().conf.descriptor_dtype is torch.float32 and ALIKED().conf.descriptor_dtype is torch.float32         # the defaults stay fp32
    assert SuperPoint(descriptor_dtype=torch.float16).conf.descriptor_dtype is torch.float16
    assert ALIKED(descriptor_dtype=torch.float16).conf.descriptor_dtype is torch.float16


def test_engine_descriptors_dtype_rule_on_the_host():
    """The rule LightGlue.forward / _store apply (no GPU needed for the part that decides): float16 stays float16 and contiguous, everything else becomes fp32."""
    from lightglue_amd.lightglue import _engine_descriptors
    cpu = torch.device("cpu")
    h = torch.arange(24, dtype=torch.float16).reshape(1, 3, 8)
    t = _engine_descriptors(h, cpu)
    assert t.dtype is torch.float16 and t.data_ptr() == h.data_ptr()
    nc = h.transpose(1, 2).contiguous().transpose(1, 2)
    t = _engine_descriptors(nc, cpu)
    assert t.dtype is torch.float16 and t.is_contiguous() and torch.equal(t, h)
    odd = torch.zeros(1 + 24, dtype=torch.float16)[1:].view(1, 3, 8)      # 2 bytes off a 16-byte boundary: copied, still float16
    t = _engine_descriptors(odd, cpu)
    assert t.data_ptr() % 16 == 0 and t.dtype is torch.float16
    for dtype in (torch.float64, torch.bfloat16):
        t = _engine_descriptors(h.to(dtype), cpu)
        assert t.dtype is torch.float32
    f = h.float()
    t = _engine_descriptors(f, cpu)
    assert t.dtype is torch.float32 and t.data_ptr() == f.data_ptr()


RECORD = json.loads((ROOT / "tests" / "golden" / "f16_descriptor_drift.json").read_text())


@pytest.mark.parametrize("name", sorted(RECORD))
def test_storage_format_drift_is_pinned_to_the_reference(name):
    """Storing descriptors as float16 is the user's choice and OUTSIDE the 1e-3 score bar: this pins how far outside, against the reference's golden outputs.  The
    oracle on float16-rounded descriptors keeps every index of the golden, and its max |d score| is the recorded one within 1.25 x (deterministic numpy; the margin
    covers BLAS summation order across thread counts)."""
    import f16_descriptor_drift as tool
    assert sorted(RECORD) == sorted(tool.PINNED)
    got, rec = tool.drift(name), RECORD[name]
    print(f"{name}: flips {got['index_flips']} / {got['entries']}, max |d score| {got['max_dscore']:.3e} (recorded {rec['max_dscore']:.3e}), "
          f"norms {got['norm_min']:.3f} - {got['norm_max']:.3f}")
    assert got["index_flips"] == 0 == rec["index_flips"] and got["entries"] == rec["entries"]
    assert rec["max_dscore"] / 1.25 <= got["max_dscore"] <= rec["max_dscore"] * 1.25
    assert rec["max_dscore"] > 1e-3, "these fixtures are outside the 1e-3 bar with float16-stored descriptors: nothing may claim otherwise"
    np.testing.assert_allclose([got["norm_min"], got["norm_max"]], [rec["norm_min"], rec["norm_max"]], rtol=1e-6)
