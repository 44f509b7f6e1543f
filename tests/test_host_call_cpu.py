"""The host side the entry points over a pair list or a caller's workspace share (lightglue_amd/csrc/lg_host_call.h): lg_engine_forward, lg_nn_match,
lg_twoview_verify and lg_sift_filter refuse a bad pair list and a bad workspace in the same words, each under its own name, before the GPU is touched;
tests/cpp/host_call_check.cpp walks the refusals and the three workspace layouts on the host alone.  No GPU."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import pytest

from lightglue_amd import _cabi

ROOT = Path(__file__).resolve().parent.parent
PTR = 1 << 20              # an aligned integer for every pointer: each call has something wrong, so it returns before it reads through any of them
N = 64


def _engine(lib, **over):
    h = C.c_void_p()
    assert lib.lg_engine_create(C.byref(_cabi.LgConfig(256, 256, 9, 4, 0, 0.95, 0.99, 0.1, -1, 4, -1)), C.byref(h)) == _cabi.LG_OK
    io = _cabi.LgForwardIO()
    io.batch, io.n0, io.n1, io.flags = 2, N, N, _cabi.LG_FLAG_EXT | _cabi.LG_FLAG_INDEXED
    io.status, io.index0, io.index1, io.images0, io.images1 = PTR, PTR, PTR, 4, 4
    for k, v in over.items():
        setattr(io, k, v)
    try:
        return lib.lg_engine_forward(h, C.byref(io), None)
    finally:
        lib.lg_engine_destroy(h)


def _nn(lib, **over):
    io = _cabi.LgNnIO(pairs=2, n0=N, n1=N, dim=128, flags=_cabi.LG_FLAG_INDEXED | _cabi.LG_FLAG_NN_MUTUAL, desc0=PTR, desc1=PTR, index0=PTR, index1=PTR,
                      images0=4, images1=4, workspace=PTR, workspace_bytes=1 << 40, raw0=PTR, raw1=PTR, matches0=PTR, matches1=PTR, scores0=PTR, scores1=PTR,
                      matches=PTR, match_scores=PTR, list_rows=N, n_matches=PTR, status=PTR)
    for k, v in over.items():
        setattr(io, k, v)
    return lib.lg_nn_match(C.byref(io), None)


def _twoview(lib, **over):
    io = _cabi.LgTwoViewIO(pairs=2, n0=N, n1=N, images0=4, images1=4, flags=_cabi.LG_TWOVIEW_HOMOGRAPHY | _cabi.LG_FLAG_INDEXED, threshold=3.0, num_hypotheses=256,
                           seed=0, kpts0=PTR, kpts1=PTR, index0=PTR, index1=PTR, matches0=PTR, workspace=PTR, workspace_bytes=1 << 40, models=PTR, inliers0=PTR,
                           num_inliers=PTR, status=PTR)
    for k, v in over.items():
        setattr(io, k, v)
    return lib.lg_twoview_verify(C.byref(io), None)


def _sift_filter(lib, workspace=PTR, workspace_bytes=1 << 40):
    return lib.lg_sift_filter(PTR, PTR, PTR, None, None, PTR, 2, N, 48, 64, 0, workspace, workspace_bytes, PTR, PTR, None)


STAGES = {
    "lg_engine_forward": (_engine, None),
    "lg_nn_match": (_nn, lambda lib: ("lg_nn_workspace_bytes", lib.lg_nn_workspace_bytes(4, 4, N, N, 128, _cabi.LG_FLAG_INDEXED | _cabi.LG_FLAG_NN_MUTUAL))),
    "lg_twoview_verify": (_twoview, lambda lib: ("lg_twoview_workspace_bytes", lib.lg_twoview_workspace_bytes(2, N, _cabi.LG_TWOVIEW_HOMOGRAPHY | _cabi.LG_FLAG_INDEXED))),
    "lg_sift_filter": (_sift_filter, lambda lib: ("lg_sift_filter_workspace_bytes", lib.lg_sift_filter_workspace_bytes(2, N, 48, 64))),
}
PAIR_LIST_WORDS = (b"LG_FLAG_INDEXED", b"index0, index1", b"images0")
APPLY = {"lg_engine_forward": "ab", "lg_nn_match": "abcd", "lg_twoview_verify": "abcd", "lg_sift_filter": "cd"}
CASES = [(stage, case) for stage, cases in APPLY.items() for case in cases]


@pytest.mark.parametrize("stage,case", CASES)
def test_entry_points_refuse_in_the_same_words(stage, case):
    """(a) LG_FLAG_INDEXED with a null index1, (b) images0 = 0, (c) a workspace pointer at + 64, (d) a workspace one byte short.  The engine owns its workspace
    and lg_sift_filter takes no pair list: the cases that do not apply to them are left out."""
    lib = _cabi.load()
    call, size = STAGES[stage]
    words = PAIR_LIST_WORDS
    if case == "a":
        rc = call(lib, index1=None)
    elif case == "b":
        rc = call(lib, images0=0)
    elif case == "c":
        rc, words = call(lib, workspace=PTR + 64), (b"256-byte aligned",)
    else:
        name, need = size(lib)
        assert need > 0
        rc, words = call(lib, workspace_bytes=need - 1), (b"workspace holds %d bytes, %s = %d" % (need - 1, name.encode(), need),)
    said = lib.lg_last_error()
    assert rc == _cabi.LG_ERR_INVALID and said.startswith(stage.encode() + b": "), said
    for word in words:
        assert word in said, said


def test_null_workspace_is_refused():
    lib = _cabi.load()
    for stage in ("lg_nn_match", "lg_twoview_verify", "lg_sift_filter"):
        assert STAGES[stage][0](lib, workspace=None) == _cabi.LG_ERR_INVALID and (stage.encode() + b": null workspace") in lib.lg_last_error(), stage


def test_refusals_and_layouts_hold_on_the_whole_grid(tmp_path):
    """the header is host-only C++17: the stand-alone program is built as plain C++ with the host compiler (no device pass) and walks the refusal table, the
    three workspace layouts piece by piece, the solvers' byte totals and envelopes, the Cholesky's panel loop and the cut of a pair list into launches.
    (For a sanitizer run of the header, build the same program with
    -fsanitize=address,undefined.)"""
    cxx = shutil.which("hipcc") or shutil.which("c++")
    assert cxx, "needs a C++17 host compiler (hipcc or c++)"
    exe = tmp_path / "host_call_check"
    src = ROOT / "tests" / "cpp" / "host_call_check.cpp"
    r = subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    assert int(r.stdout.split()[1]) > 4000, r.stdout   # the grid was walked
