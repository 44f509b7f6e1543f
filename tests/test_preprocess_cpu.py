"""ImagePreprocessor, the parts that need no GPU: the host-only plan function (`lg_preprocess_plan`) against the Python size / ks / sigma
rule of the fixture generator (tools/make_golden_preprocess.py `resize_rule`, the restatement of kornia's `resize`), the envelope refusals of
both C entry points, the Python surface, and — where the reference checkout is present — the generator against the committed fixtures."""
import ctypes as C
import json
import math
from pathlib import Path

import numpy as np
import pytest
import torch

import make_golden_preprocess as GP
from lightglue_amd import _cabi

GOLD = Path(__file__).resolve().parent / "golden" / "preprocess"
SIDES = ("long", "short", "vert", "horz")
MAX_TAPS = _cabi.LG_PREPROCESS_MAX_TAPS


def _plan(h, w, resize, side="long", antialias=True, align_corners=False):
    """(return code, plan) of lg_preprocess_plan"""
    lib = _cabi.load()
    plan = _cabi.LgResizePlan()
    if isinstance(resize, tuple):
        rh, rw = resize
    else:
        rh, rw = resize, _cabi.LG_RESIZE_EDGE
    rc = lib.lg_preprocess_plan(h, w, rh, rw, _cabi.LG_SIDE[side], int(antialias), int(bool(align_corners)), C.byref(plan))
    return rc, plan


def _expect(h, w, resize, side, antialias):
    """The Python rule, or None where it yields a zero target side, torch's reflect pad would refuse (ks // 2 >= axis length) or the tap cap is exceeded."""
    h_out, w_out, ks, sigma = GP.resize_rule(h, w, resize, side, antialias)
    if h_out < 1 or w_out < 1:
        return None
    if ks[0] // 2 >= h or ks[1] // 2 >= w or max(ks) > MAX_TAPS:
        return None
    return h_out, w_out, ks, sigma


def _ulp(x):
    return math.ulp(x) if x else 0.0


def _check(h, w, resize, side, antialias):
    rc, p = _plan(h, w, resize, side, antialias)
    want = _expect(h, w, resize, side, antialias)
    if want is None:
        assert rc == _cabi.LG_ERR_INVALID, (h, w, resize, side, antialias)
        return 0
    assert rc == _cabi.LG_OK, (h, w, resize, side, antialias, _cabi.load().lg_last_error())
    h_out, w_out, ks, sigma = want
    assert (p.h_in, p.w_in, p.h_out, p.w_out, p.ks_y, p.ks_x) == (h, w, h_out, w_out, ks[0], ks[1]), (h, w, resize, side, antialias)
    assert abs(p.sigma_y - sigma[0]) <= _ulp(sigma[0]) and abs(p.sigma_x - sigma[1]) <= _ulp(sigma[1]), (h, w, resize, side, antialias)
    assert p.identity == int((h_out, w_out) == (h, w))
    assert p.scale_x == w_out / w and p.scale_y == h_out / h
    return 1


def test_plan_matches_the_python_rule_on_a_sweep():
    """Every h, w in 1 .. 160, a handful of edge lengths on all four sides and of (h, w) pairs: integers equal, sigma to 1 ulp of double; refusals
    exactly where the Python rule gives a zero side, where F.pad(mode="reflect") would refuse, or above the tap cap."""
    accepted = refused = 0
    edges, pairs = (1, 7, 64, 100, 1024), ((5, 9), (64, 48), (200, 3), (160, 160))
    for h in range(1, 161):
        for w in range(1, 161):
            for s in edges:
                for side in SIDES:
                    ok = _check(h, w, s, side, True)
                    accepted += ok; refused += 1 - ok
            for pr in pairs:
                ok = _check(h, w, pr, "long", True)
                accepted += ok; refused += 1 - ok
    assert accepted > 100000 and refused > 1000, (accepted, refused)     # both branches are exercised
    for h in range(1, 161, 7):       # antialias off: ks = 1 whatever the factor, nothing to refuse but zero sides
        for w in range(1, 161, 5):
            for s in (1, 64):
                for side in SIDES:
                    _check(h, w, s, side, False)
            _check(h, w, (3, 200), "long", False)


def test_plan_of_every_committed_fixture():
    names = sorted(p for p in GOLD.glob("*.npz") if not p.stem.startswith("e2e_"))
    assert len(names) >= 14
    for path in names:
        z = np.load(path)
        case = GP.case_from_fixture(z)
        rc, p = _plan(case["H"], case["W"], case["resize"], case["side"], case["antialias"], case["align_corners"])
        assert rc == _cabi.LG_OK, path.stem
        assert (p.h_out, p.w_out, p.ks_y, p.ks_x) == (int(z["h_out"]), int(z["w_out"]), int(z["ks"][0]), int(z["ks"][1])), path.stem
        assert abs(p.sigma_y - float(z["sigma"][0])) <= _ulp(float(z["sigma"][0])) and abs(p.sigma_x - float(z["sigma"][1])) <= _ulp(float(z["sigma"][1]))
        np.testing.assert_array_equal(np.array([p.scale_x, p.scale_y], np.float32), z["scale"])
        assert tuple(z["out"].shape) == (case["B"], case["C"], p.h_out, p.w_out)
        assert p.align_corners == int(bool(case["align_corners"]))
    # the cases the issue names are there: ks = 31, different ks per axis, int() truncation, a width >= 1000
    ks = {p.stem: tuple(int(v) for v in np.load(p)["ks"]) for p in names}
    assert (31, 31) in ks.values() and any(a != b for a, b in ks.values())
    assert any(int(np.load(p)["W"]) >= 1000 for p in names) and any(str(np.load(p)["dtype"]) == "uint8" for p in names)


def test_envelope_is_refused_without_touching_a_gpu():
    lib = _cabi.load()
    err = lambda: lib.lg_last_error().decode()
    # tap cap: 2000 -> 100 is factor 20 -> ks 39
    rc, _ = _plan(2000, 2000, 100)
    assert rc == _cabi.LG_ERR_INVALID and "LG_PREPROCESS_MAX_TAPS" in err() and "33" in err()
    rc, p = _plan(1700, 1700, 100)     # factor 17: sigma 8, ks 33 = the cap
    assert rc == _cabi.LG_OK and (p.ks_y, p.ks_x) == (33, 33)
    # reflect padding: 8 x 400 -> (1, 50): ks_y = 15, 7 >= 8 is false -> fine; 7 x 400: 13 // 2 = 6 < 7 fine; 2 x 400 -> (1, 200): ks_y = 3, 1 < 2 fine; 1 x 400 -> (1, 200): ks_y = 3, 1 >= 1
    rc, _ = _plan(1, 400, (1, 200))
    assert rc == _cabi.LG_ERR_INVALID and "ks / 2 < axis length" in err()
    rc, _ = _plan(6, 400, (1, 400))    # factor 6 -> sigma 2.5, ks 11: 5 < 6 holds
    assert rc == _cabi.LG_OK
    rc, _ = _plan(5, 400, (1, 400))    # factor 5 -> sigma 2, ks 8 -> 9: 4 < 5 holds
    assert rc == _cabi.LG_OK
    rc, _ = _plan(4, 400, (1, 100))    # ks_y = 7: 3 < 4 holds; ks_x = 7
    assert rc == _cabi.LG_OK
    rc, _ = _plan(3, 400, (1, 100))    # factor 3 -> sigma 1, ks 4 -> 5: 2 < 3 holds
    assert rc == _cabi.LG_OK
    # zero / negative sizes, a zero target side, unknown side, sides above the limit
    for args in ((0, 10, 5), (10, -1, 5), (10, 10, 0), (10, 10, -4), (10, 10, (0, 5)), (10, 10, (5, -2))):
        rc, _ = _plan(*args)
        assert rc == _cabi.LG_ERR_INVALID and "positive" in err(), args
    rc, _ = _plan(100, 3, 10)          # long side 100 -> 10: int(10 / (100 / 3) ...) -> width int(10 * 0.03) = 0
    assert rc == _cabi.LG_ERR_INVALID and "zero side" in err()
    plan = _cabi.LgResizePlan()
    assert lib.lg_preprocess_plan(10, 10, 5, _cabi.LG_RESIZE_EDGE, 4, 1, 0, C.byref(plan)) == _cabi.LG_ERR_INVALID and "side" in err()
    assert lib.lg_preprocess_plan(10, 10, 5, _cabi.LG_RESIZE_EDGE, -1, 1, 0, C.byref(plan)) == _cabi.LG_ERR_INVALID
    rc, _ = _plan(2 ** 23 + 1, 10, (10, 10), antialias=False)
    assert rc == _cabi.LG_ERR_INVALID and "LG_PREPROCESS_MAX_SIDE" in err()
    assert lib.lg_preprocess_plan(10, 10, 5, _cabi.LG_RESIZE_EDGE, 0, 1, 0, None) == _cabi.LG_ERR_INVALID

    # the resize call: everything is checked before the stream or the pointers are used
    fake = C.c_void_p(4096)
    rc, p = _plan(64, 64, 32)
    assert rc == _cabi.LG_OK
    call = lambda dtype=0, b=1, c=3, h=64, w=64, sb=3 * 4096, sc=4096, sy=64, sx=1, plan=p, src=fake, dst=fake: lib.lg_preprocess_resize(
        src, dtype, b, c, h, w, sb, sc, sy, sx, C.byref(plan) if plan is not None else None, dst, None)
    assert call(dtype=2) == _cabi.LG_ERR_INVALID and "dtype" in err()
    assert call(c=2) == _cabi.LG_ERR_INVALID and "channels" in err()
    assert call(b=0) == _cabi.LG_ERR_INVALID and "batch" in err()
    assert call(h=65) == _cabi.LG_ERR_INVALID and "plan" in err()
    assert call(sy=-64) == _cabi.LG_ERR_INVALID and "strides" in err()
    assert call(sc=2 ** 30 + 1) == _cabi.LG_ERR_INVALID and "2^31" in err()
    assert call(sy=2 ** 26) == _cabi.LG_ERR_INVALID and "2^31" in err()
    assert call(src=None) == _cabi.LG_ERR_INVALID and "null" in err()
    assert call(plan=None) == _cabi.LG_ERR_INVALID
    bad = _cabi.LgResizePlan.from_buffer_copy(p); bad.ks_x = 35; bad.sigma_x = 8.5
    assert call(plan=bad) == _cabi.LG_ERR_INVALID and "LG_PREPROCESS_MAX_TAPS" in err()
    bad = _cabi.LgResizePlan.from_buffer_copy(p); bad.ks_y = 4
    assert call(plan=bad) == _cabi.LG_ERR_INVALID and "odd" in err()
    bad = _cabi.LgResizePlan.from_buffer_copy(p); bad.h_in, bad.ks_y, bad.sigma_y = 3, 7, 1.5
    assert call(h=3, plan=bad) == _cabi.LG_ERR_INVALID and "ks / 2 < axis length" in err()
    bad = _cabi.LgResizePlan.from_buffer_copy(p); bad.w_out = 0
    assert call(plan=bad) == _cabi.LG_ERR_INVALID and "positive" in err()


def test_header_constants_match_the_binding():
    import re
    header = (Path(__file__).resolve().parent.parent / "include" / "lightglue_amd.h").read_text()
    assert int(re.search(r"#define LG_PREPROCESS_MAX_TAPS (\d+)", header).group(1)) == _cabi.LG_PREPROCESS_MAX_TAPS >= 33
    assert int(re.search(r"#define LG_PREPROCESS_MAX_SIDE (\d+)", header).group(1)) == _cabi.LG_PREPROCESS_MAX_SIDE
    body = re.search(r"typedef struct lg_resize_plan \{(.*?)\} lg_resize_plan;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f[0] for f in _cabi.LgResizePlan._fields_]
    for key, val in _cabi.LG_SIDE.items():
        assert re.search(r"LG_SIDE_%s = %d\b" % (key.upper(), val), header)


def test_host_api():
    import lightglue_amd
    from lightglue_amd import ALIKED, ImagePreprocessor, SuperPoint, numpy_image_to_torch
    assert ImagePreprocessor.default_conf == {"resize": None, "side": "long", "interpolation": "bilinear", "align_corners": None, "antialias": True}
    assert list(ImagePreprocessor.default_conf) == ["resize", "side", "interpolation", "align_corners", "antialias"]
    assert "ImagePreprocessor" in lightglue_amd.__all__ and "numpy_image_to_torch" in lightglue_amd.__all__
    pre = ImagePreprocessor(resize=32, side="short")
    assert pre.conf.resize == 32 and pre.conf.side == "short" and pre.conf.antialias is True
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pre(torch.zeros(1, 16, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ImagePreprocessor()(torch.zeros(1, 3, 16, 16, dtype=torch.uint8))
    rng = np.random.default_rng(0)
    hwc = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    t = numpy_image_to_torch(hwc)
    assert t.shape == (3, 5, 7) and t.dtype == torch.float32
    np.testing.assert_array_equal(t.numpy(), (hwc.transpose(2, 0, 1) / 255.0).astype(np.float32))
    hw = rng.integers(0, 256, (5, 7), dtype=np.uint8)
    assert numpy_image_to_torch(hw).shape == (1, 5, 7)
    with pytest.raises(ValueError, match="Not an image"):
        numpy_image_to_torch(np.zeros((2, 3, 4, 5)))
    assert SuperPoint.preprocess_conf == {"resize": None} and ALIKED.preprocess_conf == {"resize": None}
    # the float(v) / 255.0f conversion of the kernel is numpy_image_to_torch's, for all 256 values (float64 division, then the cast)
    v = np.arange(256, dtype=np.uint8)
    np.testing.assert_array_equal(numpy_image_to_torch(v[None])[0, 0].numpy(), v.astype(np.float32) / np.float32(255.0))


def test_generator_reproduces_the_committed_fixtures():
    """The resize fixtures bit for bit (pad, two 1-D convolutions and F.interpolate give the same bits for every thread count); the end-to-end
    ones with the same keypoints and everything else to the bars of the extractor tests — the reference networks' CPU convolutions are not
    bit-reproducible across thread counts, the resize in front of them is."""
    if not (GP.REF_DIR / "utils.py").exists():
        pytest.skip("needs the reference checkout (build container)")
    mods = GP.load_reference("superpoint", "aliked")
    for name, case in GP.CASES.items():
        z = np.load(GOLD / f"{name}.npz")
        assert GP.case_from_fixture(z) == case, name
        got = GP.run_case(mods["utils"], case)
        assert sorted(got) == sorted(z.files)
        for key in z.files:
            np.testing.assert_array_equal(np.asarray(got[key]), z[key], err_msg=f"{name}: {key}")
    assert sorted(p.stem for p in GOLD.glob("*.npz")) == sorted(list(GP.CASES) + list(GP.E2E_CASES))
    for name in GP.E2E_CASES:
        z = np.load(GOLD / f"{name}.npz")
        got = GP.run_e2e(mods, name)
        assert sorted(got) == sorted(z.files)
        meta, want = json.loads(str(got["meta"])), json.loads(str(z["meta"]))
        assert {k: v for k, v in meta.items() if "margin" not in k} == {k: v for k, v in want.items() if "margin" not in k}
        np.testing.assert_array_equal(got["image_size"], z["image_size"]); np.testing.assert_array_equal(got["scale"], z["scale"])
        assert got["keypoints"].shape == z["keypoints"].shape
        np.testing.assert_allclose(got["keypoints"], z["keypoints"], atol=1e-3, rtol=0)
        np.testing.assert_allclose(got["keypoint_scores"], z["keypoint_scores"], atol=1e-5, rtol=2e-5)
        np.testing.assert_allclose(got["descriptors"], z["descriptors"], atol=2e-4, rtol=0)
