"""Ragged-batch ALIKED extraction, the parts that need no GPU: the host-side validation of `valid_size`, the batch planner with ALIKED's own byte
function, the per-image padding geometry the `lg_aliked_*_ragged` entry points document, and the presence of their symbols."""
import re
from pathlib import Path

import pytest
import torch

from lightglue_amd import ALIKED, _cabi, plan_image_batches

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "lightglue_amd.h").read_text()
RAGGED_SYMBOLS = ("lg_aliked_encode_ragged", "lg_aliked_detect_ragged", "lg_aliked_describe_ragged", "lg_aliked_describe_ragged_half")
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


def test_ragged_symbols_declared_and_bound():
    lib = _cabi.load()
    for fn in RAGGED_SYMBOLS:
        assert re.search(r"\bint %s\(" % fn, HEADER) and fn in _cabi.EXPORTED_SYMBOLS and getattr(lib, fn) is not None
        assert not re.search(r"\d", fn)
    # each is its uniform twin plus `const int32_t* sizes`
    for fn in RAGGED_SYMBOLS:
        twin = fn.replace("_ragged", "")
        args = lambda name: re.search(r"\bint %s\(([^;]*)\);" % name, HEADER).group(1)      # noqa: E731
        ragged, uniform = [a.strip() for a in args(fn).replace("\n", " ").split(",")], [a.strip() for a in args(twin).replace("\n", " ").split(",")]
        assert "const int32_t* sizes" in ragged
        ragged.remove("const int32_t* sizes")
        assert ragged == uniform, (fn, ragged, uniform)


def test_ragged_entry_points_refuse_null_sizes_before_the_device():
    lib = _cabi.load()
    one = 1      # any non-null value: refusals come before a pointer is used
    rc = lib.lg_aliked_encode_ragged(one, 2, 3, 64, 96, None, 16, one, one, one, 1 << 40, one, None)
    assert rc == _cabi.LG_ERR_INVALID and b"null pointer" in lib.lg_last_error()
    rc = lib.lg_aliked_detect_ragged(one, 2, 64, 96, None, None, 2, 0.2, -1, 100, 100, one, 1 << 40, one, one, one, one, None)
    assert rc == _cabi.LG_ERR_INVALID and b"null pointer" in lib.lg_last_error()
    rc = lib.lg_aliked_describe_ragged(one, 2, 64, 96, None, 16, one, one, one, 10, one, 1 << 40, one, None)
    assert rc == _cabi.LG_ERR_INVALID and b"null pointer" in lib.lg_last_error()
