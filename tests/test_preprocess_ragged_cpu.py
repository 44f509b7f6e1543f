"""The ragged preprocess call (`lg_preprocess_ragged_plan` / `ImagePreprocessor.to_canvas`), the parts that need no GPU: the planner is host-only
arithmetic, so its refusals and its launch geometry are checked on the library as it loads on a CPU box, and the Python side refuses bad image sets
before it touches a device."""
import ctypes as C

import pytest
import torch

from lightglue_amd import ImagePreprocessor, _cabi
from lightglue_amd.preprocess import make_plan

FAKE = 4096          # a non-null "device pointer": nothing here dereferences it


def _source(c, h, w, dtype=_cabi.LG_DTYPE_F32, data=FAKE, strides=None):
    sb, sc, sy, sx = strides if strides is not None else (c * h * w, h * w, w, 1)
    return _cabi.LgImageSource(data, dtype, c, h, w, sb, sc, sy, sx)


def _plan(sources, plans, c_out, hc, wc, table_bytes=None, with_arrays=False, null=()):
    """(rc, message, total_tiles, lds_bytes, prefix, image_lds) of one lg_preprocess_ragged_plan call"""
    lib = _cabi.load()
    n = len(sources)
    nbytes = int(lib.lg_preprocess_ragged_table_bytes(n)) if table_bytes is None else table_bytes
    buf = (C.c_uint8 * max(nbytes, 1))()
    tiles, lds = C.c_int64(-1), C.c_int64(-1)
    prefix, each = (C.c_int32 * max(n, 1))(), (C.c_int32 * max(n, 1))()
    args = dict(sources=(_cabi.LgImageSource * max(n, 1))(*sources), plans=(_cabi.LgResizePlan * max(n, 1))(*plans), table=C.cast(buf, C.c_void_p),
                tiles=C.byref(tiles), lds=C.byref(lds))
    for name in null:
        args[name] = None
    rc = lib.lg_preprocess_ragged_plan(args["sources"], args["plans"], n, c_out, hc, wc, args["table"], nbytes, args["tiles"], args["lds"],
                                       prefix if with_arrays else None, each if with_arrays else None)
    return rc, lib.lg_last_error().decode(), tiles.value, lds.value, list(prefix)[:n], list(each)[:n]


def test_table_bytes():
    lib = _cabi.load()
    assert _cabi.LG_PREPROCESS_RAGGED_MAX_BATCH == 256
    assert lib.lg_preprocess_ragged_table_bytes(0) == 0 and lib.lg_preprocess_ragged_table_bytes(257) == 0
    one, two = lib.lg_preprocess_ragged_table_bytes(1), lib.lg_preprocess_ragged_table_bytes(2)
    assert 0 < one < two and lib.lg_preprocess_ragged_table_bytes(256) == one + 255 * (two - one)


def test_planner_refusals():
    """Everything outside the envelope is LG_ERR_INVALID with a message; the planner makes no HIP call (this box has no device to make one on)."""
    ident = make_plan(32, 48, (32, 48))
    good = _source(1, 32, 48)
    rc, msg, tiles, lds, _, _ = _plan([good], [ident], 1, 32, 48)
    assert rc == _cabi.LG_OK and tiles >= 1 and lds > 0, msg
    cases = {
        "batch 0": dict(sources=[], plans=[], c_out=1, hc=32, wc=48, table_bytes=4096),
        "batch 257": dict(sources=[good] * 257, plans=[ident] * 257, c_out=1, hc=32, wc=48, table_bytes=1 << 20),
        "2-channel image": dict(sources=[_source(2, 32, 48)], plans=[ident], c_out=1, hc=32, wc=48),
        "c_out 2": dict(sources=[good], plans=[ident], c_out=2, hc=32, wc=48),
        "target taller than the canvas": dict(sources=[good], plans=[ident], c_out=1, hc=31, wc=48),
        "target wider than the canvas": dict(sources=[good], plans=[ident], c_out=1, hc=32, wc=47),
        "negative stride": dict(sources=[_source(1, 32, 48, strides=(0, 0, -48, 1))], plans=[ident], c_out=1, hc=32, wc=48),
        "2^31 elements": dict(sources=[_source(1, 32, 48, strides=(0, 0, 2 ** 31 // 31 + 1, 1))], plans=[ident], c_out=1, hc=32, wc=48),
        "table one byte short": dict(sources=[good, good], plans=[ident, ident], c_out=1, hc=32, wc=48,
                                     table_bytes=int(_cabi.load().lg_preprocess_ragged_table_bytes(2)) - 1),
        "null image pointer": dict(sources=[_source(1, 32, 48, data=None)], plans=[ident], c_out=1, hc=32, wc=48),
        "null sources": dict(sources=[good], plans=[ident], c_out=1, hc=32, wc=48, null=("sources",)),
        "null plans": dict(sources=[good], plans=[ident], c_out=1, hc=32, wc=48, null=("plans",)),
        "null table": dict(sources=[good], plans=[ident], c_out=1, hc=32, wc=48, null=("table",)),
        "null outputs": dict(sources=[good], plans=[ident], c_out=1, hc=32, wc=48, null=("tiles", "lds")),
        "canvas of 2^31 pixels": dict(sources=[good], plans=[ident], c_out=1, hc=2 ** 16, wc=2 ** 15),
        "plan of another size": dict(sources=[_source(1, 33, 48)], plans=[ident], c_out=1, hc=64, wc=64),
        "unknown dtype": dict(sources=[_source(1, 32, 48, dtype=7)], plans=[ident], c_out=1, hc=32, wc=48),
    }
    for name, kw in cases.items():
        rc, msg, *_ = _plan(kw.pop("sources"), kw.pop("plans"), kw.pop("c_out"), kw.pop("hc"), kw.pop("wc"), **kw)
        assert rc == _cabi.LG_ERR_INVALID and msg, name
    # the launch refuses before the GPU too: null pointers, and a host table the planner did not fill
    lib = _cabi.load()
    blank = (C.c_uint8 * 4096)()
    assert lib.lg_preprocess_resize_ragged(None, FAKE, 1, FAKE, 0, None) == _cabi.LG_ERR_INVALID
    assert lib.lg_preprocess_resize_ragged(C.cast(blank, C.c_void_p), None, 1, FAKE, 0, None) == _cabi.LG_ERR_INVALID
    assert lib.lg_preprocess_resize_ragged(C.cast(blank, C.c_void_p), FAKE, 1, None, 0, None) == _cabi.LG_ERR_INVALID
    assert lib.lg_preprocess_resize_ragged(C.cast(blank, C.c_void_p), FAKE, 1, FAKE, 0, None) == _cabi.LG_ERR_INVALID and lib.lg_last_error()


def test_launch_geometry_of_a_mixed_group():
    """201 x 333 -> 96, 256 x 2048 -> 128 (31 taps across: 1-row tiles), 96 x 70 identity, 60 x 80 -> 200 (upscale): the grid is the sum of the images' tiles,
    the LDS the largest image's, the prefix exclusive and increasing — each image's own numbers come from planning it alone."""
    group = [(3, 201, 333, make_plan(201, 333, 96)), (1, 256, 2048, make_plan(256, 2048, 128)), (3, 96, 70, make_plan(96, 70, (96, 70))),
             (1, 60, 80, make_plan(60, 80, 200))]
    assert [p.identity for *_, p in group] == [0, 0, 1, 0] and group[1][3].ks_x == 31 and group[3][3].ks_x == 1
    hc, wc = max(p.h_out for *_, p in group), max(p.w_out for *_, p in group)
    alone = []
    for c, h, w, p in group:
        rc, msg, tiles, lds, prefix, each = _plan([_source(c, h, w)], [p], 3, hc, wc, with_arrays=True)
        assert rc == _cabi.LG_OK, msg
        assert tiles >= 1 and 0 < lds <= 64 * 1024 and prefix == [0] and each == [lds]
        alone.append((tiles, lds))
    assert len({a for a in alone}) == len(alone)                      # four different tilings in one launch
    assert alone[1][0] >= group[1][3].h_out                           # 1-row tiles: at least one tile per output row
    rc, msg, tiles, lds, prefix, each = _plan([_source(c, h, w) for c, h, w, _ in group], [p for *_, p in group], 3, hc, wc, with_arrays=True)
    assert rc == _cabi.LG_OK, msg
    assert tiles == sum(t for t, _ in alone)
    assert lds == max(l for _, l in alone) and each == [l for _, l in alone]
    assert prefix == [sum(t for t, _ in alone[:i]) for i in range(len(alone))]
    assert prefix[0] == 0 and all(a < b for a, b in zip(prefix, prefix[1:])) and prefix[-1] < tiles


def test_plan_images_equals_make_plan():
    shapes = [(201, 333), (256, 2048), (96, 70), (60, 80)]
    fields = [f[0] for f in _cabi.LgResizePlan._fields_]
    for conf in (dict(resize=128), dict(resize=(77, 130), antialias=False), dict(resize=120, side="short", align_corners=True), dict()):
        pre = ImagePreprocessor(**conf)
        plans = pre.plan_images(shapes)
        assert len(plans) == len(shapes)
        for (h, w), got in zip(shapes, plans):
            c = pre.conf
            want = make_plan(h, w, (h, w)) if c.resize is None else make_plan(h, w, c.resize, c.side, c.antialias, c.align_corners)
            assert [getattr(got, f) for f in fields] == [getattr(want, f) for f in fields], (conf, h, w)
            assert bool(got.identity) == ((got.h_out, got.w_out) == (h, w))
    assert all(p.identity for p in ImagePreprocessor().plan_images(shapes))
    assert ImagePreprocessor().plan_images([]) == []


def test_to_canvas_refuses_before_any_gpu_use(monkeypatch):
    monkeypatch.setattr(_cabi, "load", lambda: pytest.fail("to_canvas reached the library"))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: pytest.fail("to_canvas reached the GPU"))
    pre = ImagePreprocessor(resize=64)
    with pytest.raises(ValueError, match="at least one image"):
        pre.to_canvas([])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pre.to_canvas([torch.zeros(1, 32, 48)])
    with pytest.raises(RuntimeError, match="image 0"):
        pre.to_canvas([torch.zeros(1, 3, 32, 48, dtype=torch.uint8)] * 2)
    with pytest.raises(TypeError, match="float32 or uint8"):
        pre.to_canvas([torch.zeros(1, 32, 48, dtype=torch.float64)])
    with pytest.raises(ValueError, match="1 or 3 channels"):
        pre.to_canvas([torch.zeros(2, 32, 48)])
    with pytest.raises(ValueError, match="channels must be"):
        pre.to_canvas([torch.zeros(1, 32, 48)], channels=2)
    with pytest.raises(ValueError, match=r"\[C, H, W\]"):
        pre.to_canvas([torch.zeros(32, 48)])
    with pytest.raises(ValueError, match=r"\[C, H, W\]"):
        pre.to_canvas([torch.zeros(2, 1, 32, 48)])
