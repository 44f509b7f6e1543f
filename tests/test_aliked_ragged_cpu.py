"""Ragged-batch ALIKED extraction, the parts that need no GPU: the host-side validation of `valid_size`, the batch planner with ALIKED's own byte
function, the per-image padding geometry the header documents for `LG_EXTRACT_RAGGED`, and the stages' refusal of a ragged call without sizes."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

from lightglue_amd import ALIKED, _cabi, plan_image_batches

HEADER = (Path(__file__).resolve().parent.parent / "include" / "lightglue_amd.h").read_text()
# (h, w) of the GPU test's canvas of four: centred pads 12 / 12; pads 15 + 16 and 0 + 1; no pad; one 32-pixel tile
SIZES = [(40, 72), (33, 31), (64, 96), (8, 8)]


def test_valid_size_errors_name_the_image():
    model = ALIKED()
    canvas = torch.zeros(2, 3, 64, 96)      # a CPU canvas: the sizes are checked first, on the host
    for call in (lambda v: model.encode(canvas, valid_size=v), lambda v: model({"image": canvas, "valid_size": v}),
                 lambda v: model.detect(canvas[:, 0], valid_size=v), lambda v: model.describe(None, (2, 64, 96), None, None, valid_size=v)):
        with pytest.raises(ValueError, match=r"valid_size\[1\].*canvas"):
            call([[96, 64], [97, 64]])
        with pytest.raises(ValueError, match=r"valid_size\[0\].*canvas"):
            call([[96, 65], [96, 64]])
        with pytest.raises(ValueError, match=r"valid_size\[1\].*minimum"):
            call([[96, 64], [7, 64]])           # the uniform entry point refuses images below 8 x 8
        with pytest.raises(ValueError, match=r"valid_size\[1\].*integer"):
            call(torch.tensor([[96.0, 64.0], [40.5, 64.0]]))
        with pytest.raises(ValueError, match="shape"):
            call([[96, 64]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # valid sizes: the CPU image is refused next
        model.encode(canvas, valid_size=[[96, 64], [8, 8]])


def test_valid_size_with_image_size_is_refused():
    model = ALIKED()
    canvas = torch.zeros(2, 3, 64, 96)
    sizes, image_size = [[96, 64], [31, 33]], torch.tensor([[96.0, 64.0], [31.0, 33.0]])
    with pytest.raises(ValueError, match="valid_size and image_size"):
        model({"image": canvas, "valid_size": sizes, "image_size": image_size})
    with pytest.raises(ValueError, match="valid_size and image_size"):
        model.detect(canvas[:, 0], image_size, valid_size=sizes)


def test_extract_batch_refusals():
    model = ALIKED()
    with pytest.raises(ValueError, match="at least one image"):
        model.extract_batch([])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.extract_batch([torch.zeros(3, 32, 32)])
    with pytest.raises(ValueError, match="image 0 must be"):
        model.extract_batch([torch.zeros(2, 3, 32, 32)])


def test_planner_with_the_aliked_byte_function():
    lib = _cabi.load()
    nbytes = lambda n, h, w: lib.lg_aliked_workspace_bytes(n, h, w, 16)      # noqa: E731
    sizes = [(96, 160), (75, 109), (67, 91), (40, 64), (41, 65), (17, 33), (8, 8), (160, 96), (75, 109), (96, 160), (120, 40)]
    cap = nbytes(3, 96, 160)
    plan = plan_image_batches(sizes, 8, max_workspace_bytes=cap, workspace_bytes=nbytes)
    assert sorted(i for idx, _ in plan for i in idx) == list(range(len(sizes)))
    for idx, (hc, wc) in plan:
        assert hc == max(sizes[i][0] for i in idx) and wc == max(sizes[i][1] for i in idx)
        assert nbytes(len(idx), hc, wc) <= cap
    assert max(len(idx) for idx, _ in plan) > 1 and len(plan) > len(plan_image_batches(sizes, 8))
    with pytest.raises(ValueError, match=r"image 7 \(160 x 96\).*max_workspace_bytes"):
        plan_image_batches(sizes, 8, max_workspace_bytes=nbytes(1, 160, 96) - 1, workspace_bytes=nbytes)
    # ALIKED's workspace is not SuperPoint's: the default byte function (SuperPoint's) groups differently under the same cap
    assert nbytes(3, 96, 160) != lib.lg_sp_encode_workspace_bytes(3, 96, 160)


def _padder(h, w):
    """InputPadder(divis_by=32): (Hp, Wp, top, bottom, left, right), the padding centred, the odd pixel on the far side"""
    ph, pw = ((h // 32 + 1) * 32 - h) % 32, ((w // 32 + 1) * 32 - w) % 32
    return h + ph, w + pw, ph // 2, ph - ph // 2, pw // 2, pw - pw // 2


def test_per_image_padding_geometry():
    expect = {(40, 72): (64, 96, 12, 12, 12, 12), (33, 31): (64, 32, 15, 16, 0, 1), (64, 96): (64, 96, 0, 0, 0, 0), (8, 8): (32, 32, 12, 12, 12, 12)}
    for hw in SIZES:
        assert _padder(*hw) == expect[hw]
    # 1/32-level maps of 2 x 3, 2 x 1, 2 x 3 and 1 x 1
    assert [(_padder(h, w)[0] >> 5, _padder(h, w)[1] >> 5) for h, w in SIZES] == [(2, 3), (2, 1), (2, 3), (1, 1)]
    # the padded canvas: 64 x 96 pads to itself, 70 x 100 to 96 x 128 (tiles outside every image); the padding is monotone, so every frame fits it
    assert _padder(64, 96)[:2] == (64, 96) and _padder(70, 100)[:2] == (96, 128)
    for hc, wc in ((64, 96), (70, 100), (200, 200)):
        for h in range(8, hc + 1):
            assert _padder(h, 8)[0] <= _padder(hc, wc)[0]
        for w in range(8, wc + 1):
            assert _padder(8, w)[1] <= _padder(hc, wc)[1]
    # the level buffer and the workspace of a ragged call are those of the canvas: the library's totals follow the padded canvas, whatever the images
    lib = _cabi.load()
    for (hc, wc) in ((64, 96), (70, 100)):
        hp, wp = _padder(hc, wc)[:2]
        total = sum((4 * 4 * (hp >> s) * (wp >> s) * 32 + 255) // 256 * 256 for s in (0, 1, 3, 5))
        assert lib.lg_aliked_levels_bytes(4, hc, wc) == total
        assert lib.lg_aliked_workspace_bytes(4, hc, wc, 16) == lib.lg_aliked_workspace_bytes(4, hp, wp, 16)


def test_ragged_is_a_flag_of_each_stage_declared_and_bound():
    """A ragged call and its uniform twin cannot drift apart: they are ONE prototype and ONE struct per stage, the ragged form being `LG_EXTRACT_RAGGED` plus the
    struct's `sizes`.  Each stage is declared once, exported, bound as (const io*, stream); its io declares `flags` and `const int32_t *sizes`; no `_ragged` /
    `_half` symbol of a stage is left in the header, the binding or the library."""
    lib = _cabi.load()
    stages = {"lg_aliked_encode": ("lg_aliked_encode_io", _cabi.LgAlikedEncodeIO), "lg_aliked_detect": ("lg_aliked_detect_io", _cabi.LgAlikedDetectIO),
              "lg_aliked_describe": ("lg_aliked_describe_io", _cabi.LgAlikedDescribeIO)}
    for fn, (struct, mirror) in stages.items():
        assert len(re.findall(r"\bint %s\(const %s\* io, void\* hip_stream\);" % (fn, struct), HEADER)) == 1, fn
        assert len(re.findall(r"\bint %s\w*\(" % fn, HEADER)) == 1, fn                      # the stage has no second prototype under a longer name
        assert fn in _cabi.EXPORTED_SYMBOLS and getattr(lib, fn).argtypes == [C.POINTER(mirror), C.c_void_p]
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), HEADER, re.S).group(1)
        assert re.search(r"\buint32_t flags;", body) and re.search(r"\bconst int32_t \*sizes;", body), struct
        fields = dict(mirror._fields_)
        assert fields["flags"] is C.c_uint32 and fields["sizes"] is C.c_void_p
        for suffix in ("_ragged", "_half", "_ragged_half"):
            assert fn + suffix not in _cabi.EXPORTED_SYMBOLS and not hasattr(lib, fn + suffix), fn + suffix
    assert re.search(r"#define LG_EXTRACT_RAGGED\s+1u", HEADER) and _cabi.LG_EXTRACT_RAGGED == 1


def test_ragged_entry_points_refuse_null_sizes_before_the_device():
    lib = _cabi.load()
    one = 1      # any non-null value: refusals come before a pointer is used
    R = _cabi.LG_EXTRACT_RAGGED
    io = _cabi.LgAlikedEncodeIO(batch=2, channels=3, h=64, w=96, n_pos=16, flags=R, image=one, sizes=None, packed=one, levels=one, workspace=one,
                                workspace_bytes=1 << 40, scores=one)
    rc = lib.lg_aliked_encode(C.byref(io), None)
    assert rc == _cabi.LG_ERR_INVALID and b"null pointer" in lib.lg_last_error()
    io = _cabi.LgAlikedDetectIO(batch=2, h=64, w=96, flags=R, scores=one, sizes=None, image_size=None, nms_radius=2, scores_th=0.2, top_k=-1, n_limit=100,
                                capacity=100, workspace=one, workspace_bytes=1 << 40, keypoints=one, kp_scores=one, kp_norm=one, counts=one)
    rc = lib.lg_aliked_detect(C.byref(io), None)
    assert rc == _cabi.LG_ERR_INVALID and b"null pointer" in lib.lg_last_error()
    io = _cabi.LgAlikedDescribeIO(batch=2, h=64, w=96, n_pos=16, flags=R, levels=one, sizes=None, packed=one, kp_norm=one, counts=one, n=10, workspace=one,
                                  workspace_bytes=1 << 40, descriptors=one)
    rc = lib.lg_aliked_describe(C.byref(io), None)
    assert rc == _cabi.LG_ERR_INVALID and b"null pointer" in lib.lg_last_error()
