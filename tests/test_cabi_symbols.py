"""The C-ABI library loads on a box without a GPU and exports every symbol include/lightglue_amd.h
declares (no compute calls here)."""
import ctypes
import re
from pathlib import Path

import pytest

from lightglue_amd import _cabi

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "lightglue_amd.h").read_text()


def declared_functions():
    # prototypes look like:  <ret> lg_xxx(...);
    return sorted(set(re.findall(r"\b(lg_[a-z_]+)\s*\(", HEADER)))


def test_library_is_built():
    assert _cabi.library_path().exists(), "run __graft_entry__.build() first"


def test_exports_every_declared_symbol():
    lib = _cabi.load()
    names = declared_functions()
    assert set(names) == set(_cabi.EXPORTED_SYMBOLS), (names, _cabi.EXPORTED_SYMBOLS)
    for n in names:
        assert getattr(lib, n) is not None


def typed_fields_of(struct_name):
    """[(name, C element type, is a pointer)] of a `typedef struct X { ... } X;` of the header, in declaration order"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct_name, struct_name), HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        parts = [p.strip() for p in decl.split(",")]
        first = re.fullmatch(r"(.*?)(\w+)", parts[0])                       # type (with the first declarator's stars), first name
        ctype = first.group(1).replace("const", "").replace("*", "").strip()
        out.append((first.group(2), ctype, "*" in first.group(1)))
        out += [(p.lstrip("* "), ctype, p.startswith("*")) for p in parts[1:]]
    return out


def fields_of(struct_name):
    return [name for name, _, _ in typed_fields_of(struct_name)]


# the six extractor stages: header struct -> ctypes mirror
EXTRACT_IO = {"lg_sp_encode_io": _cabi.LgSpEncodeIO, "lg_sp_detect_io": _cabi.LgSpDetectIO, "lg_sp_sample_io": _cabi.LgSpSampleIO,
              "lg_aliked_encode_io": _cabi.LgAlikedEncodeIO, "lg_aliked_detect_io": _cabi.LgAlikedDetectIO, "lg_aliked_describe_io": _cabi.LgAlikedDescribeIO}
SCALARS = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}


def test_struct_layouts_match_header():
    # field order of the ctypes mirrors == order of the declarations in the header
    assert fields_of("lg_config") == [f[0] for f in _cabi.LgConfig._fields_]
    assert fields_of("lg_forward_io") == [f[0] for f in _cabi.LgForwardIO._fields_]
    assert fields_of("lg_unpack_io") == [f[0] for f in _cabi.LgUnpackIO._fields_]
    assert fields_of("lg_nn_io") == [f[0] for f in _cabi.LgNnIO._fields_]
    # the extractor stages' io structs: order AND element type of every field (an int32 mirrored as int64 keeps the order and shifts everything behind it)
    assert set(_cabi.EXTRACT_STAGES.values()) == set(EXTRACT_IO.values())
    for name, mirror in EXTRACT_IO.items():
        want = []
        for field, ctype, pointer in typed_fields_of(name):
            if pointer:
                want.append((field, ctypes.POINTER(ctypes.c_void_p) if field == "params" else ctypes.c_void_p))
            else:
                want.append((field, SCALARS[ctype]))
        assert want == list(mirror._fields_), name
        assert "flags" in dict(want) and dict(want)["flags"] is ctypes.c_uint32 and dict(want)["sizes"] is ctypes.c_void_p, name
    # every stage is bound as (const io*, stream), and nothing of a removed variant is left in the header or the binding
    lib = _cabi.load()
    for fn, mirror in _cabi.EXTRACT_STAGES.items():
        assert getattr(lib, fn).argtypes == [ctypes.POINTER(mirror), ctypes.c_void_p], fn
        assert re.search(r"\bint %s\(const %s\* io, void\* hip_stream\);" % (fn, [k for k, v in EXTRACT_IO.items() if v is mirror][0]), HEADER), fn
    assert not re.search(r"lg_(sp|aliked)_\w*(_ragged|_half)\b|lg_sp_encode_split", HEADER)
    assert "uint16_t" not in HEADER      # descriptor outputs are void*: LG_EXTRACT_DESC_F16 says which element type
    # the three flags: the header's values are _cabi's, and distinct bits
    values = [int(re.search(r"#define %s\s+(\d+)u" % n, HEADER).group(1)) for n in ("LG_EXTRACT_RAGGED", "LG_EXTRACT_DESC_F16", "LG_EXTRACT_SPLIT")]
    assert values == [_cabi.LG_EXTRACT_RAGGED, _cabi.LG_EXTRACT_DESC_F16, _cabi.LG_EXTRACT_SPLIT]
    assert all(v and v & (v - 1) == 0 for v in values) and len(set(values)) == 3
    # the wire width of the Python side == LG_WIRE_WIDTH of the header
    macro = re.search(r"#define LG_WIRE_WIDTH\(n0, n1\) (.*?)\s+/\*", HEADER).group(1)
    assert eval(macro.replace("LL", ""), {"n0": 300, "n1": 77}) == _cabi.wire_width(300, 77)


def test_envelope_is_refused_without_touching_a_gpu():
    """LG_MAX_KEYPOINTS / LG_MAX_ROWS / LG_MAX_SIM_ELEMS (include/lightglue_amd.h): a call outside the envelope returns LG_ERR_INVALID with a message before any
    allocation or launch (4.3 M rows must be an error, not silently dropped stores)."""
    lib = _cabi.load()
    limits = {k: int(re.search(r"#define %s (\d+)" % k, HEADER).group(1)) for k in ("LG_MAX_KEYPOINTS", "LG_MAX_ROWS", "LG_MAX_SIM_ELEMS")}
    assert limits == {"LG_MAX_KEYPOINTS": 8192, "LG_MAX_ROWS": 2 ** 21, "LG_MAX_SIM_ELEMS": 2 ** 31 - 1}
    h = ctypes.c_void_p()
    ok = _cabi.LgConfig(256, 256, 9, 4, 0, 0.95, 0.99, 0.1, -1, 4, -1)
    assert lib.lg_engine_create(ctypes.byref(ok), ctypes.byref(h)) == _cabi.LG_OK
    for (B, n0, n1, word) in ((1, 8193, 100, b"LG_MAX_KEYPOINTS"), (1050, 2048, 2048, b"LG_MAX_ROWS"), (129, 4096, 4096, b"LG_MAX_SIM_ELEMS"), (513, 2048, 2048, b"LG_MAX_ROWS")):
        assert lib.lg_engine_reserve(h, B, n0, n1) == _cabi.LG_ERR_INVALID, (B, n0, n1)
        assert word in lib.lg_last_error(), lib.lg_last_error()
    lib.lg_engine_destroy(h)
    # the receiving side of the wire: bad strides / counts are refused, an empty gather is a no-op
    io = _cabi.LgUnpackIO()
    io.rows, io.n0, io.n1, io.pairs_out = 0, 16, 16, 0
    assert lib.lg_unpack_wire(ctypes.byref(io), None) == _cabi.LG_OK
    io.rows, io.pairs_out, io.wire, io.wire_stride = 2, 2, 1 << 20, _cabi.wire_width(16, 16) - 1
    assert lib.lg_unpack_wire(ctypes.byref(io), None) == _cabi.LG_ERR_INVALID


def test_argument_validation_without_gpu():
    lib = _cabi.load()
    assert lib.lg_version().decode().startswith("lightglue_amd")
    h = ctypes.c_void_p()
    bad = _cabi.LgConfig(256, 128, 9, 4, 0, 0.95, 0.99, 0.1, -1, 4, -1)  # descriptor_dim != 256
    assert lib.lg_engine_create(ctypes.byref(bad), ctypes.byref(h)) == _cabi.LG_ERR_INVALID
    assert b"descriptor_dim" in lib.lg_last_error()
    with pytest.raises(AssertionError):
        _cabi.check(_cabi.LG_ERR_INVALID)
    ok = _cabi.LgConfig(256, 256, 9, 4, 0, 0.95, 0.99, 0.1, -1, 4, -1)
    assert lib.lg_engine_create(ctypes.byref(ok), ctypes.byref(h)) == _cabi.LG_OK
    # forward before weights -> state error, no GPU touched
    io = _cabi.LgForwardIO()
    io.batch, io.n0, io.n1 = 1, 4, 4
    assert lib.lg_engine_forward(h, ctypes.byref(io), None) == _cabi.LG_ERR_STATE
    # options: unknown keys (and the switches of removed experiments) are refused, with a message
    assert lib.lg_engine_set_option(h, b"fused_next", 0) == _cabi.LG_OK
    assert lib.lg_engine_set_option(h, b"no_such_option", 1) == _cabi.LG_ERR_INVALID and b"no_such_option" in lib.lg_last_error()
    assert lib.lg_engine_set_option(h, b"tail_variant", 1) == _cabi.LG_ERR_INVALID
    lib.lg_engine_destroy(h)
    # the split-f16 conv stack addresses one image with 32-bit element offsets: larger images are refused before anything is touched
    fake = ctypes.c_void_p(16)
    arr = (ctypes.c_void_p * 24)(*[16] * 24)
    io = _cabi.LgSpEncodeIO(batch=1, h=8192, w=4096, flags=_cabi.LG_EXTRACT_SPLIT, image=16, params=arr, workspace=16, workspace_bytes=1 << 40, scores=16, desc_map=16)
    assert lib.lg_sp_encode(ctypes.byref(io), None) == _cabi.LG_ERR_INVALID and b"2^25" in lib.lg_last_error()
    assert lib.lg_sp_pack_conv_weight_split(fake, 65, 64, 3, fake, None) == _cabi.LG_ERR_INVALID       # 3 x 3 layers: cout % 64
    assert lib.lg_sp_pack_conv_weight_split(fake, 64, 48, 1, fake, None) == _cabi.LG_ERR_INVALID       # cin % 32
    # precision enum: every named mode is accepted; the removed split-bf16 value (3) and anything past the last one are not
    for name, val in _cabi.LG_PREC.items():
        cfg = _cabi.LgConfig(256, 256, 9, 4, 0, 0.95, 0.99, 0.1, -1, val, -1)
        assert lib.lg_engine_create(ctypes.byref(cfg), ctypes.byref(h)) == _cabi.LG_OK, name
        lib.lg_engine_destroy(h)
    for val in (3, max(_cabi.LG_PREC.values()) + 1):
        cfg = _cabi.LgConfig(256, 256, 9, 4, 0, 0.95, 0.99, 0.1, -1, val, -1)
        assert lib.lg_engine_create(ctypes.byref(cfg), ctypes.byref(h)) == _cabi.LG_ERR_INVALID and b"precision" in lib.lg_last_error()
    # attention precision: the linear precision itself, or one f16 plane together with f16x3 (the fast opt-in); nothing else
    P = _cabi.LG_PREC
    for prec, attn, want in ((P["f16x3"], P["f16x3"], _cabi.LG_OK), (P["f16x3"], P["fp16"], _cabi.LG_OK), (P["f16x3"], P["bf16"], _cabi.LG_ERR_INVALID),
                             (P["fp32"], P["fp16"], _cabi.LG_ERR_INVALID), (P["bf16"], P["bf16"], _cabi.LG_OK)):
        cfg = _cabi.LgConfig(256, 256, 9, 4, 0, 0.95, 0.99, 0.1, -1, prec, attn)
        assert lib.lg_engine_create(ctypes.byref(cfg), ctypes.byref(h)) == want, (prec, attn)
        if want == _cabi.LG_OK:
            lib.lg_engine_destroy(h)


def _extract_ios():
    """One well-formed io per extractor stage, every pointer a fake non-null value (a refusal comes before anything is dereferenced)"""
    arr = (ctypes.c_void_p * 24)(*[16] * 24)
    big = 1 << 40
    return {
        "lg_sp_encode": _cabi.LgSpEncodeIO(batch=2, h=64, w=64, image=16, sizes=16, params=arr, workspace=16, workspace_bytes=big, scores=16, desc_map=16),
        "lg_sp_detect": _cabi.LgSpDetectIO(batch=2, h=64, w=64, scores=16, sizes=16, nms_radius=4, remove_borders=4, detection_threshold=0.0005, max_keypoints=0,
                                           capacity=64, max_candidates=4096, workspace=16, workspace_bytes=big, keypoints=16, kp_scores=16, counts=16),
        "lg_sp_sample_descriptors": _cabi.LgSpSampleIO(batch=2, channels=256, h=8, w=8, desc_map=16, sizes=16, keypoints=16, n=4, cell=8, normalize_dense=1,
                                                       workspace=16, out=16),
        "lg_aliked_encode": _cabi.LgAlikedEncodeIO(batch=2, channels=3, h=64, w=96, n_pos=16, image=16, sizes=16, packed=16, levels=16, workspace=16,
                                                   workspace_bytes=big, scores=16),
        "lg_aliked_detect": _cabi.LgAlikedDetectIO(batch=2, h=64, w=96, scores=16, sizes=16, nms_radius=2, scores_th=0.2, top_k=-1, n_limit=100, capacity=100,
                                                   workspace=16, workspace_bytes=big, keypoints=16, kp_scores=16, kp_norm=16, counts=16),
        "lg_aliked_describe": _cabi.LgAlikedDescribeIO(batch=2, h=64, w=96, n_pos=16, levels=16, sizes=16, packed=16, kp_norm=16, counts=16, n=10, workspace=16,
                                                       workspace_bytes=big, descriptors=16),
    }


# the flag bits each stage defines (include/lightglue_amd.h)
STAGE_FLAGS = {"lg_sp_encode": _cabi.LG_EXTRACT_RAGGED | _cabi.LG_EXTRACT_SPLIT, "lg_sp_detect": _cabi.LG_EXTRACT_RAGGED,
               "lg_sp_sample_descriptors": _cabi.LG_EXTRACT_RAGGED | _cabi.LG_EXTRACT_DESC_F16, "lg_aliked_encode": _cabi.LG_EXTRACT_RAGGED,
               "lg_aliked_detect": _cabi.LG_EXTRACT_RAGGED, "lg_aliked_describe": _cabi.LG_EXTRACT_RAGGED | _cabi.LG_EXTRACT_DESC_F16}


@pytest.mark.parametrize("stage", sorted(STAGE_FLAGS))
def test_extract_stage_refuses_null_io_undefined_flags_and_null_sizes(stage):
    """The rules all six stages share: a null io, a flag bit the stage does not define (LG_EXTRACT_SPLIT outside lg_sp_encode, LG_EXTRACT_DESC_F16 on an encode or
    detect stage, any bit above 4) and LG_EXTRACT_RAGGED with sizes == NULL are LG_ERR_INVALID with a message, before anything is touched: every pointer here is a
    fake non-null value, so a refusal that came later would have crashed."""
    lib = _cabi.load()
    fn, inv = getattr(lib, stage), _cabi.LG_ERR_INVALID
    assert sorted(STAGE_FLAGS) == sorted(_cabi.EXTRACT_STAGES)
    assert fn(None, None) == inv and b"null io" in lib.lg_last_error() and stage.encode() in lib.lg_last_error()
    undefined = [bit for bit in (1, 2, 4) if not STAGE_FLAGS[stage] & bit] + [8, 16, 1 << 31]
    assert len(undefined) >= 4
    for bit in undefined:
        for base in (0, STAGE_FLAGS[stage]):
            io = _extract_ios()[stage]
            io.flags = base | bit
            assert fn(ctypes.byref(io), None) == inv, (stage, base, bit)
            assert b"flag" in lib.lg_last_error() and stage.encode() in lib.lg_last_error(), lib.lg_last_error()
    for flags in {_cabi.LG_EXTRACT_RAGGED, STAGE_FLAGS[stage]}:
        io = _extract_ios()[stage]
        io.flags, io.sizes = flags, None
        assert fn(ctypes.byref(io), None) == inv and b"null pointer" in lib.lg_last_error(), (stage, flags)
    # without the flag `sizes` is not read: a null one is no refusal, and the call goes on to its own argument checks (batch 0 here)
    io = _extract_ios()[stage]
    io.flags, io.sizes, io.batch = 0, None, 0
    assert fn(ctypes.byref(io), None) == inv and b"null pointer" not in lib.lg_last_error() and b"flag" not in lib.lg_last_error()
