"""The mechanics of one call over feature stores, written once for `LightGlue`, `NearestNeighborMatcher` and the seven geometry classes (each module keeps its
class: configuration, the io struct of its entry point and the public methods): what a caller reads of one side (`build_side`; `normalise_side` is the engine's
reading), the opening of a call (`sides`, `batch_sides` for `forward`, `store_pairs`, `pair_list` and `device_index` for a pair list), how a pair list is cut into
engine calls (`plan_pair_chunks`), the output set of a call (`Outputs`) and its assembly into the reference's dict (`ragged_outputs`, `DeferredMatches`); for
the nearest-neighbour matcher and the geometry classes also the setting checks (`ransac_settings`, `int_in`, `positive`), THE device call (`device_call`:
device, stream, library, workspace, entry point), the index pointers (`index_ptrs`), the summary | status buffer (`summary_status`) and the per-item status
error (`raise_on_status`, `raise_with_outputs`).  `_readers.py` holds the readers of cameras, poses and tracks.  Plain tensor and pointer arithmetic:
`device_call` is the only place that enters the library, through the entry point it is given.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import torch

from . import _cabi


def require_gpu(device, what: str = "keypoints") -> None:
    """THE device check of the matcher (forward, match_pairs, InflightMatcher): a missing GPU is an error, never another path."""
    if device.type != "cuda":
        raise RuntimeError(f"lightglue_amd runs on MI355X (ROCm device type 'cuda') only; there is no CPU fallback. Got {what} on {device}.")


PAIR_STATUS = {_cabi.LG_ERR_RANGE: "values outside the f16 operand range (|x| >= 65504, inf or NaN; LG_ERR_RANGE)",
               _cabi.LG_ERR_DEVICE: "an internal device-side wait expired (LG_ERR_DEVICE)",
               _cabi.LG_ERR_INDEX: "an image index outside its feature store (LG_ERR_INDEX): the pair was not matched",
               _cabi.LG_ERR_CAMERA: "a camera whose focal length is not finite and > 0, or whose principal point is not finite (LG_ERR_CAMERA)"}


def raise_on_status(status, noun: str = "pair", what: dict = PAIR_STATUS) -> None:
    """Per-item status codes (lg_forward_io.status, in the order of the call's pair list; the solvers' status per image) -> LightGlueAmdError naming the
    items as `noun` with the texts of the table `what`."""
    bad = [(i, int(c)) for i, c in enumerate(status) if int(c) != _cabi.LG_OK]
    if bad:
        raise _cabi.LightGlueAmdError("; ".join(f"{noun} {i}: {what.get(c, c)}" for i, c in bad[:8]))


def ragged_outputs(host, mlist, mscores, stop):
    """The part of the output assembly (ref :593-629) that needs the host, for `Outputs.finish` and `parallel.Pending.wait`: host = [[stop per pair],
    [matches per pair], [status per pair]] -> (matches List[[S_i, 2]], scores List[[S_i]], stop: an int for one pair, else the tensor `stop`); raises on a status."""
    raise_on_status(host[2])
    counts = host[1]
    matches = [row[:c] for row, c in zip(mlist.unbind(0), counts)]
    scores = [row[:c] for row, c in zip(mscores.unbind(0), counts)]
    return matches, scores, int(host[0][0]) if len(counts) == 1 else stop


class DeferredMatches:
    """Handle of a forward whose outputs are on their way (LightGlue.forward_deferred)."""

    def __init__(self, done, host_sizes, assemble, buffers=()):
        self._done, self._host, self._assemble, self._out = done, host_sizes, assemble, None
        self.buffers = buffers     # the allocations every output tensor is a view of (InflightMatcher hands THEM to the consumer's stream: 3 - 4 record_stream calls, not one per output)

    def result(self) -> dict:
        if self._out is None:
            self._done.synchronize()
            self._out = self._assemble(self._host.tolist())
            self._assemble = None
        return self._out


# ---------------------------------------------------------------------- the geometry estimators over a match list (TwoViewVerifier, RelativePoseEstimator,
# AbsolutePoseEstimator; the Triangulator reads matches0 the same way)
def ransac_settings(threshold, num_hypotheses, seed) -> tuple:
    """THE constructor check of the three hypothesise-and-verify estimators: (threshold, num_hypotheses, seed) as (float, int, int), or the ValueError."""
    if not float(threshold) > 0.0:
        raise ValueError(f"threshold must be > 0, got {threshold!r}")
    if int(num_hypotheses) % 256 or not 256 <= int(num_hypotheses) <= 65536:
        raise ValueError(f"num_hypotheses must be a multiple of 256 in [256, 65536], got {num_hypotheses!r}")
    if not 0 <= int(seed) < 2 ** 32:
        raise ValueError(f"seed must lie in [0, 2^32), got {seed!r}")
    return float(threshold), int(num_hypotheses), int(seed)


def int_in(name: str, value, lo: int, hi: int, refuse_bool: bool = False, what: str = None) -> int:
    """THE check of an integer setting in [lo, hi]: int(value), or the ValueError `{name} {what}, got ...` (what: "must be an integer in [lo, hi]" unless given).
    1.0 passes, "3" does not; True passes as 1 unless refuse_bool."""
    if (refuse_bool and isinstance(value, bool)) or int(value) != value or not lo <= int(value) <= hi:
        raise ValueError(f"{name} {what or f'must be an integer in [{lo}, {hi}]'}, got {value!r}")
    return int(value)


def positive(name: str, value, suffix: str = "") -> float:
    """THE check of a setting that is finite and > 0: float(value), or the ValueError `{name} must be > 0{suffix}, got ...`."""
    if not 0.0 < float(value) < float("inf"):
        raise ValueError(f"{name} must be > 0{suffix}, got {value!r}")
    return float(value)


def as_matches0(result, P: int, N: int, device) -> torch.Tensor:
    """matches0 [P, N] as the C ABI reads it — int64, contiguous, on `device` — from a matcher's result: its dict, a `DeferredMatches` or the tensor itself.
    A tensor that already qualifies passes through untouched."""
    if isinstance(result, DeferredMatches):
        result = result.result()
    m0 = result["matches0"] if isinstance(result, dict) else result
    assert torch.is_tensor(m0) and tuple(m0.shape) == (P, N), f"matches0 must have shape [{P}, {N}], got {tuple(m0.shape)}"
    if m0.dtype is not torch.int64 or m0.device != device or not m0.is_contiguous():
        m0 = m0.detach().to(device=device, dtype=torch.int64).contiguous()
    return m0


def ragged_matches(mask: torch.Tensor, verified: torch.Tensor, counts) -> list:
    """The ragged `matches` lists List[[S_i, 2]] without a synchronisation of their own: a stable sort puts every pair's inlier rows (mask [P, N] bool) first,
    in ascending order, beside their matches (verified [P, N]); their numbers `counts` are on the host already."""
    order = torch.sort((~mask).to(torch.uint8), dim=1, stable=True)[1]
    listed = torch.stack([order, torch.gather(verified, 1, order)], -1)
    return [listed[b, :c] for b, c in enumerate(counts)]


def raise_with_outputs(status, out: dict, noun: str = "pair", what: dict = PAIR_STATUS) -> dict:
    """`out`, or `raise_on_status`'s error carrying it as `.outputs`: the items with status LG_OK are complete."""
    try:
        raise_on_status(status, noun, what)
    except _cabi.LightGlueAmdError as err:
        err.outputs = out
        raise
    return out


def index_ptrs(index) -> tuple:
    """(index0, index1) of an io struct: the addresses of the two rows of the int32 [2, P] index (`store_pairs`), (None, None) without one."""
    return (None, None) if index is None else (index[0].data_ptr(), index[1].data_ptr())


def summary_status(n: int, K: int, device) -> tuple:
    """The solvers' "n doubles of summary | K int32 of status" in ONE zeroed allocation: (the status [K] on `device`, the summary's address, the status's
    address, read); read() is THE host sync of the call and gives (summary [n] float64, status [K] int32) as numpy views of one host copy."""
    small = torch.zeros((2 * n + K,), device=device, dtype=torch.int32)

    def read():
        host = small.cpu().numpy()
        return host[:2 * n].view(np.float64), host[2 * n:]
    return small[2 * n:], small.data_ptr(), small.data_ptr() + 8 * n, read


def device_call(device, entry: str, sizer: str, size_args: tuple, make_io, skip: bool = False, floor: int = 256):
    """THE device call of the nearest-neighbour matcher and the geometry classes: on `device` and its current stream, the workspace of
    lib.<sizer>(*size_args) bytes (at least `floor`: 256 everywhere but for the matcher, whose scratch is the stores' rows), io = make_io(workspace address,
    workspace bytes), lib.<entry>(io, stream) through `_cabi.check`.  A size of -1 (outside the envelope) reaches the entry point with 0 bytes: its message
    is the error the caller sees.  skip: nothing is called (the matcher and the three estimators over an empty pair list).  Returns the stream."""
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device)
        if not skip:
            lib = _cabi.load()
            nbytes = getattr(lib, sizer)(*size_args)
            ws = torch.empty((max(nbytes, floor),), device=device, dtype=torch.uint8)
            io = make_io(_ptr(ws), max(nbytes, 0))
            _cabi.check(getattr(lib, entry)(C.byref(io), C.c_void_p(stream.cuda_stream)))
    return stream


def plan_pair_chunks(P: int, n0: int, n1: int, max_rows: int = _cabi.LG_MAX_ROWS, max_sim_elems: int = _cabi.LG_MAX_SIM_ELEMS) -> list:
    """Cut a list of P pairs of n0 x n1 keypoints into the FEWEST contiguous chunks [(start, stop), ...] that each fit one engine call
    (include/lightglue_amd.h: pairs * (cap0 + cap1) <= max_rows and pairs * cap0 * cap1 <= max_sim_elems, cap = n rounded up to 128).  Chunk sizes differ
    by at most one, larger chunks first: the first chunk is the largest call, so the engine's workspace grows at most once.  Pure host arithmetic."""
    P, n0, n1 = int(P), int(n0), int(n1)
    if n0 > _cabi.LG_MAX_KEYPOINTS or n1 > _cabi.LG_MAX_KEYPOINTS:    # what lg_engine_forward answers (AssertionError through _cabi.check): no chunking helps
        raise AssertionError("more than LG_MAX_KEYPOINTS (8192) keypoints in one image")
    if P <= 0:
        return []
    c0, c1 = (n0 + 127) // 128 * 128, (n1 + 127) // 128 * 128
    per_call = P
    if c0 + c1:
        per_call = min(per_call, int(max_rows) // (c0 + c1))
    if c0 * c1:
        per_call = min(per_call, int(max_sim_elems) // (c0 * c1))
    if per_call < 1:
        raise ValueError(f"one pair of {n0} x {n1} keypoints needs {c0 + c1} rows and {c0 * c1} similarity entries: "
                         f"more than max_rows = {max_rows} / max_sim_elems = {max_sim_elems} allow")
    chunks = -(-P // per_call)
    size, larger = divmod(P, chunks)
    out, start = [], 0
    for i in range(chunks):
        stop = start + size + (1 if i < larger else 0)
        out.append((start, stop))
        start = stop
    return out


def pair_list(pairs, K0: int, K1: int, validate: bool = True) -> torch.Tensor:
    """THE pair list of a `match_pairs` call (LightGlue's and NearestNeighborMatcher's): `pairs` (sequence, CPU or device tensor) -> an integer tensor [P, 2].
    validate: shape, dtype and range are checked on the host (a device tensor is copied there once) and a ValueError names the offending positions."""
    as_given = torch.is_tensor(pairs)
    pt = pairs if as_given else torch.as_tensor(pairs)
    if not as_given and pt.numel() == 0:
        pt = pt.reshape(0, 2).to(torch.int64)
    if pt.dim() != 2 or pt.shape[1] != 2:
        raise ValueError(f"pairs must have shape [P, 2], got {tuple(pt.shape)}")
    if pt.dtype not in (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8):
        raise ValueError(f"pairs must hold integers, got {pt.dtype}")
    if validate and pt.shape[0]:
        host = pt.cpu()
        lo, hi0, hi1 = int(host.min()), int(host[:, 0].max()), int(host[:, 1].max())
        if lo < 0 or hi0 >= K0 or hi1 >= K1:
            bad = ((host < 0) | (host >= torch.tensor([K0, K1]))).any(1).nonzero().flatten().tolist()
            raise ValueError(f"pairs {bad[:8]} index outside the feature stores of {K0} and {K1} images")
    return pt


# ---------------------------------------------------------------------- one side of a call
def _engine_descriptors(t: torch.Tensor, device, keep=(torch.float16, torch.uint8)) -> torch.Tensor:
    """Descriptors as the engine reads them; the returned tensor's dtype is the side's storage format.  float16 and uint8 (SIFT as COLMAP / OpenCV store it)
    tensors are read IN PLACE (the side's LG_FLAG_DESC*_F16 / _U8: the engine widens every value exactly where the descriptors enter it, so the forward is
    bit-identical to one on `t.float()`) — untouched when on the device, contiguous and 16-byte aligned, otherwise through one copy in the same dtype; every
    dtype outside `keep` becomes contiguous fp32 (keep = (): what every other input of a side goes through)."""
    dtype = t.dtype if t.dtype in keep else torch.float32
    if t.dtype is not dtype or t.device != device or not t.is_contiguous():
        t = t.detach().to(device=device, dtype=dtype).contiguous()
    if dtype is not torch.float32 and t.data_ptr() % 16:      # a view at an odd element offset (whole rows are multiples of 128 bytes)
        t = t.clone()
    return t


class Side:
    """K images of N keypoint rows as the engine reads them: contiguous fp32 / int32 tensors on the device (descriptors fp32, float16 or uint8), absent pieces
    None.  `rootsift`: the engine replaces every descriptor row by its RootSIFT where it enters (the store's "descriptor_transform")."""
    __slots__ = ("K", "N", "kpts", "desc", "rootsift", "size", "scales", "oris", "num")
    desc_f16 = property(lambda self: self.desc.dtype is torch.float16)
    desc_u8 = property(lambda self: self.desc.dtype is torch.uint8)

    def flags(self, side: int) -> int:
        """The LG_FLAG_DESC*_F16 / _DESC*_U8 / LG_FLAG_ROOTSIFT* bits of this side as side 0 or 1 of a call (side 1's flag is side 0's << 1)."""
        return (_cabi.LG_FLAG_DESC0_F16 * self.desc_f16 | _cabi.LG_FLAG_DESC0_U8 * self.desc_u8 | _cabi.LG_FLAG_ROOTSIFT0 * self.rootsift) << side


DESCRIPTOR_TRANSFORMS = (None, "rootsift")


def descriptor_transform(feats: dict, what: str = "feats"):
    """The optional non-tensor key `descriptor_transform` of a feature dict: None or "rootsift"."""
    tr = feats.get("descriptor_transform")
    if tr not in DESCRIPTOR_TRANSFORMS:
        raise ValueError(f"{what}: descriptor_transform must be None or 'rootsift', got {tr!r}")
    return tr


def build_side(feats: dict, device, what: str = "feats", *, keypoints: bool = True, descriptors=None, image_size: bool = False, scale_ori: bool = False) -> Side:
    """THE reader of one side of a call (LightGlue, NearestNeighborMatcher, TwoViewVerifier): a feature dict -> Side, holding what the caller reads and None
    elsewhere.  keypoints: [K, N, 2].  descriptors: None = not read, "any" = [K, N, D] of any D, an int = exactly that D; with them the optional non-tensor key
    descriptor_transform (None | "rootsift"; anything else is a ValueError).  image_size: the optional [K, 2] | [1, 2] | [2], broadcast as the reference does
    (ref :35-42).  scale_ori: scales / oris [K, N].  num_keypoints [K] is optional everywhere and clamped into [0, N].  Only data pointers are handed on, so
    every shape is checked here (AssertionError naming the key) and tensors that already qualify pass through untouched: no copy, no kernel."""
    f32 = lambda t: _engine_descriptors(t, device, keep=())
    s = Side()
    s.kpts = s.desc = s.size = s.scales = s.oris = s.num = None
    s.rootsift = False
    kpts, desc = feats["keypoints"] if keypoints else None, None if descriptors is None else feats["descriptors"]
    if keypoints:
        assert kpts.dim() == 3 and kpts.shape[-1] == 2, f"{what}: keypoints must have shape [K, N, 2], got {tuple(kpts.shape)}"
        K, N = kpts.shape[0], kpts.shape[1]
    if desc is not None:      # [K, N, D]: K and N the keypoints' where those are read, D the caller's unless any will do
        assert desc.dim() == 3 and (not keypoints or (desc.shape[0], desc.shape[1]) == (K, N)) and descriptors in ("any", desc.shape[2]), \
            f"{what}: descriptors must have shape [{K if keypoints else 'K'}, {N if keypoints else 'N'}, {'D' if descriptors == 'any' else descriptors}], got {tuple(desc.shape)}"
        K, N = desc.shape[0], desc.shape[1]
    s.K, s.N = K, N
    if keypoints:
        s.kpts = f32(kpts)
    if desc is not None:
        s.desc = _engine_descriptors(desc, device)
        s.rootsift = descriptor_transform(feats, what) == "rootsift"
    size = feats.get("image_size") if image_size else None
    if size is not None:
        if not isinstance(size, torch.Tensor):
            size = torch.tensor(size, dtype=torch.float32)
        size = f32(size).reshape(-1, 2)
        assert size.shape[0] in (1, K), f"{what}: image_size must have shape [2], [1, 2] or [{K}, 2]"
        s.size = size if size.shape[0] == K else size.expand(K, 2).contiguous()
    if scale_ori:
        s.scales, s.oris = f32(feats["scales"]), f32(feats["oris"])
        assert tuple(s.scales.shape) == (K, N) and tuple(s.oris.shape) == (K, N), f"{what}: scales / oris must have shape [{K}, {N}]"
    num = feats.get("num_keypoints")
    if num is not None:
        num = torch.as_tensor(num).detach().to(device=device, dtype=torch.int32).contiguous()
        assert num.shape == (K,), f"{what}: num_keypoints must have shape [{K}]"
        s.num = num.clamp(0, N)
    return s


def normalise_side(feats: dict, device, input_dim: int, add_scale_ori: bool, what: str = "feats") -> Side:
    """What the engine reads of one side: keypoints, descriptors [K, N, input_dim], image_size, scales / oris iff add_scale_ori (`build_side`)."""
    return build_side(feats, device, what, descriptors=input_dim, image_size=True, scale_ori=add_scale_ori)


def sides(feats0: dict, feats1: dict, names, build, key: str = "keypoints", check=None):
    """(device, side 0, side 1) of a call, each converted at most once by build(feats, device, what); a non-GPU device (that of feats0[key]) is refused first,
    side 1 IS side 0 over one store, check(s0, s1) is the caller's own test of the two together."""
    device = feats0[key].device
    require_gpu(device, key)
    s0 = build(feats0, device, names[0])
    s1 = s0 if feats1 is feats0 else build(feats1, device, names[1])
    if check is not None:
        check(s0, s1)
    return device, s0, s1


def batch_sides(data: dict, keys, build, key: str = "keypoints", check=None):
    """The opening of every `forward(data)`: both of `keys` present, `sides` of data[keys[0]] / data[keys[1]], as many images on either side."""
    for k in keys:
        assert k in data, f"Missing key {k} in data"
    device, s0, s1 = sides(data[keys[0]], data[keys[1]], keys, build, key, check)
    assert s0.K == s1.K, f"image0 and image1 must hold the same number of images, got {s0.K} and {s1.K}"
    return device, s0, s1


def store_pairs(feats0: dict, pairs, feats1, validate: bool, key: str = "keypoints"):
    """The opening of every call over a pair list (match_pairs, verify_pairs, score_models): (same, P, index).  same: both sides read the store feats0
    (feats1 None or feats0 itself); the stores hold feats[key].shape[0] images; `pairs` goes through `pair_list` (malformed pairs raise before any device
    check); index: the int32 [2, P] tensor index0 | index1 on the store's device (a chunk of the list is an offset into both), None for an empty list."""
    same = feats1 is None or feats1 is feats0
    K0 = int(feats0[key].shape[0])
    K1 = K0 if same else int(feats1[key].shape[0])
    pt = pair_list(pairs, K0, K1, validate)
    return same, int(pt.shape[0]), device_index(pt, feats0[key].device)


def device_index(pt: torch.Tensor, device):
    """A pair list [P, 2] as the int32 [2, P] tensor index0 | index1 on `device`, None for an empty list."""
    return pt.to(device=device, dtype=torch.int32).t().contiguous() if pt.shape[0] else None


# ---------------------------------------------------------------------- the outputs of a call
@functools.lru_cache(maxsize=256)
def carve_plan(b: int, m: int, n: int, pruning: bool) -> tuple:
    """(sizes, offsets) x (int32, fp32, int64): the pieces of the three output allocations of `b` pairs of m x n keypoints, every piece at a 4-element
    (16-byte) offset.  A pure function of the shape, cached: the host path of a B = 1 forward is ~0.3 ms, and this was a tenth of it."""
    def carve(sizes):
        off = [0]
        for x in sizes:
            off.append(off[-1] + ((x + 3) & ~3))
        return tuple(off)
    kmax = min(m, n)
    isz = (b * m, b * n, b * kmax * 2, b * m if pruning else 0, b * n if pruning else 0, 3 * b)
    fsz = (b * m, b * n, b * kmax, 0 if pruning else b * m, 0 if pruning else b * n)
    lsz = (b * m, b * n, b * kmax * 2, b, b * m if pruning else 0, b * n if pruning else 0)
    return isz, carve(isz), fsz, carve(fsz), lsz, carve(lsz)


def _ptr(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


class Outputs:
    """The outputs of `b` pairs: ONE int32, ONE int64 and ONE fp32 allocation, carved into the tensors of the C ABI (`carve_plan`).  The engine's last kernel
    writes the reference's dtypes itself (int64 indices / stop / prune counters, float prune0/1 without pruning, ref :616-629; round-5 extension of
    lg_forward_io): no framework kernel runs between or behind the engine's launches.  Every piece is contiguous with the pair as its leading dimension, so
    the outputs of pairs [start, stop) are the same pieces at a pointer offset (`io`).  `raw_mode`: no int64 allocation (LightGlue.forward_raw)."""

    def __init__(self, b, m, n, device, pruning, raw_mode=False, log_assignment=False):
        self.b, self.m, self.n, self.pruning, self.raw_mode = b, m, n, pruning, raw_mode
        kmax = min(m, n)
        isz, ioff, fsz, foff, lsz, loff = carve_plan(b, m, n, pruning)

        def piece(buf, off, sz, k, *shape):
            return buf[off[k]: off[k] + sz[k]].view(shape)
        ibuf = self.ibuf = torch.empty((ioff[-1],), device=device, dtype=torch.int32)
        self.m0, self.m1, self.mlist = piece(ibuf, ioff, isz, 0, b, m), piece(ibuf, ioff, isz, 1, b, n), piece(ibuf, ioff, isz, 2, b, kmax, 2)
        self.prune0_i32 = piece(ibuf, ioff, isz, 3, b, m) if pruning else None
        self.prune1_i32 = piece(ibuf, ioff, isz, 4, b, n) if pruning else None
        self.stop_nm = piece(ibuf, ioff, isz, 5, 3, b)              # [0] = stop, [1] = n_matches, [2] = status (LG_OK / LG_ERR_RANGE / LG_ERR_DEVICE / LG_ERR_INDEX)
        fbuf = self.fbuf = torch.empty((foff[-1],), device=device, dtype=torch.float32)
        self.ms0, self.ms1 = piece(fbuf, foff, fsz, 0, b, m), piece(fbuf, foff, fsz, 1, b, n)
        self.mscore_list = piece(fbuf, foff, fsz, 2, b, kmax)
        self.m0_64 = self.m1_64 = self.mlist64 = self.stop64 = self.prune0 = self.prune1 = self.lbuf = None
        if not raw_mode:
            lbuf = self.lbuf = torch.empty((loff[-1],), device=device, dtype=torch.int64)
            self.m0_64, self.m1_64 = piece(lbuf, loff, lsz, 0, b, m), piece(lbuf, loff, lsz, 1, b, n)
            self.mlist64, self.stop64 = piece(lbuf, loff, lsz, 2, b, kmax, 2), piece(lbuf, loff, lsz, 3, b)
            if pruning:
                self.prune0, self.prune1 = piece(lbuf, loff, lsz, 4, b, m), piece(lbuf, loff, lsz, 5, b, n)
            else:   # ref :616-617 (padding rows of a ragged batch: 0)
                self.prune0, self.prune1 = piece(fbuf, foff, fsz, 3, b, m), piece(fbuf, foff, fsz, 4, b, n)
        self.log_assignment = None
        if log_assignment and m > 0 and n > 0:
            self.log_assignment = torch.empty((b, m + 1, n + 1), device=device, dtype=torch.float32)

    def io(self, start, count, flags, s0: Side, s1: Side, wire=None, index=None):
        """lg_forward_io of one engine call that writes pairs [start, start + count).  The sides are passed whole; `index`: the int32 [2, P] tensor
        index0 | index1 of an LG_FLAG_INDEXED call, offset like the outputs."""
        def at(t):     # the piece's rows from pair `start` on ([pairs, ...] contiguous)
            return None if t is None or t.numel() == 0 else t.data_ptr() + start * t.stride(0) * t.element_size()
        row = lambda k: self.stop_nm.data_ptr() + (k * self.b + start) * 4
        i64 = not self.raw_mode
        counters, fill = (i64 and self.pruning), (i64 and not self.pruning)     # prune0 / prune1 hold int64 counters or the reference's float fill
        io = _cabi.LgForwardIO(
            count, self.m, self.n, flags,
            _ptr(s0.kpts), _ptr(s1.kpts), _ptr(s0.desc), _ptr(s1.desc), _ptr(s0.size), _ptr(s1.size), _ptr(s0.scales), _ptr(s0.oris), _ptr(s1.scales), _ptr(s1.oris),
            at(self.m0), at(self.m1), at(self.ms0), at(self.ms1), row(0), at(self.prune0_i32), at(self.prune1_i32),
            at(self.mlist), at(self.mscore_list), row(1), _ptr(s0.num), _ptr(s1.num), at(self.log_assignment),
            at(self.m0_64), at(self.m1_64), at(self.mlist64), at(self.stop64),
            at(self.prune0) if counters else None, at(self.prune1) if counters else None, at(self.prune0) if fill else None, at(self.prune1) if fill else None,
            _ptr(wire), 0 if wire is None else wire.stride(0), row(2))
        if index is not None:
            io.index0, io.index1 = index[0].data_ptr() + 4 * start, index[1].data_ptr() + 4 * start
            io.images0, io.images1 = s0.K, s1.K
        return io

    def raw(self) -> dict:
        """What forward_raw returns.  "pruning": the wire row's prune block holds int counters (else the float fill's bits)."""
        return {"matches0": self.m0, "matches1": self.m1, "matching_scores0": self.ms0, "matching_scores1": self.ms1, "stop": self.stop_nm[0],
                "status": self.stop_nm[2], "pruning": self.pruning}

    def _assemble(self, host):
        matches, scores, stop = ragged_outputs(host, self.mlist64, self.mscore_list, self.stop64)
        extra_out = {} if self.log_assignment is None else {"log_assignment": self.log_assignment}
        return {**extra_out, "matches0": self.m0_64, "matches1": self.m1_64, "matching_scores0": self.ms0, "matching_scores1": self.ms1,
                "stop": stop, "matches": matches, "scores": scores, "prune0": self.prune0, "prune1": self.prune1}

    def finish(self, stream, defer):
        """Output assembly (ref :593-629) behind the last engine call: the engine has written every fixed-shape tensor; only the ragged lists need the host."""
        if defer:   # the sizes travel to pinned host memory behind an event; nothing waits here
            hbuf = torch.empty((3, self.b), dtype=torch.int32, pin_memory=True)
            hbuf.copy_(self.stop_nm, non_blocking=True)
            done = torch.cuda.Event()
            done.record(stream)
            return DeferredMatches(done, hbuf, self._assemble, tuple(t for t in (self.ibuf, self.fbuf, self.lbuf, self.log_assignment) if t is not None))
        return self._assemble(self.stop_nm.tolist())  # THE host sync of the call: the ragged lists need their sizes (and B = 1 its `stop`)
