"""GPU tests of LightGlue.match_pairs: a pair list matched over device feature stores through the indexed engine call (include/lightglue_amd.h
LG_FLAG_INDEXED), in chunked calls.  Everything is compared bit for bit with `forward` on the stacked tensors {k: v[index]}; shapes are the smallest that
cross a 64-row tile and a 128-row capacity step (N = 200: caps of 256, counts 200 / 131 / 64 / 1 / 0)."""
import pytest
import torch

import gpu_util
from conftest import require_gpu
from lightglue_amd import _cabi, _call
from lightglue_amd import synthetic as synth

pytestmark = pytest.mark.gpu

_PER_IMAGE = ("keypoints", "descriptors", "scales", "oris", "image_size", "num_keypoints")
ADAPTIVE = dict(pruning_min_kpts=-1)                          # recipe C with every size above the pruning threshold: pairs stop early and prune
FIXED = dict(depth_confidence=-1, width_confidence=-1)


def _model(dim=256, scale_ori=False, adaptive=False, seed=0):
    sd = synth.make_state_dict(seed, input_dim=dim, add_scale_ori=scale_ori, recipe="C" if adaptive else "A")
    return gpu_util.make_model(sd, "f16x3", input_dim=dim, add_scale_ori=scale_ori, **(ADAPTIVE if adaptive else FIXED))


def _store(seed, counts, N, dim=256, scale_ori=False, image_size=True, poison=True):
    """K images of one synthetic scene (every image a jittered, re-ordered subset of the same keypoints, so pairs do match), `counts[i]` live rows in image i
    and NaN in every row past them: the engine must never read those."""
    g = torch.Generator().manual_seed(seed)
    K = len(counts)
    base_k = torch.rand(N, 2, generator=g) * torch.tensor([1024.0, 768.0])
    base_d = torch.nn.functional.normalize(torch.randn(N, dim, generator=g), dim=-1)
    st = {"keypoints": torch.empty(K, N, 2), "descriptors": torch.empty(K, N, dim), "keypoint_scores": torch.rand(K, N, generator=g)}
    if scale_ori:
        st["scales"], st["oris"] = 1.0 + 4.0 * torch.rand(K, N, generator=g), (torch.rand(K, N, generator=g) * 2 - 1) * 3.14159
    for i in range(K):
        perm = torch.randperm(N, generator=g)
        st["keypoints"][i] = base_k[perm] + 2.0 * torch.randn(N, 2, generator=g)
        st["descriptors"][i] = torch.nn.functional.normalize(base_d[perm] + 0.05 * torch.randn(N, dim, generator=g), dim=-1)
    if poison:
        for i, c in enumerate(counts):
            for key in ("keypoints", "descriptors", "scales", "oris"):
                if key in st:
                    st[key][i, c:] = float("nan")
    if image_size:
        st["image_size"] = torch.tensor([[1024.0 + 32 * i, 768.0 + 16 * i] for i in range(K)])     # differs per image: the size is read through the index too
    st["num_keypoints"] = torch.tensor(counts, dtype=torch.int32)
    return {k: v.cuda() for k, v in st.items()}


def _stacked(store, index):
    index = torch.as_tensor(index, device="cuda")
    return {k: store[k][index] for k in _PER_IMAGE if k in store}


def _assert_same_dict(got, want, what=""):
    assert list(got.keys()) == list(want.keys()), (what, list(got.keys()), list(want.keys()))
    for key, a in got.items():
        b = want[key]
        if isinstance(a, list):
            assert len(a) == len(b), (what, key)
            for i, (x, y) in enumerate(zip(a, b)):
                assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), (what, key, i)
        elif torch.is_tensor(a):
            assert torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (what, key)
        else:
            assert type(a) is type(b) and a == b, (what, key, a, b)


COUNTS = [200, 131, 64, 1, 0]
#        self    both orders    a repeated image    the empty image on either side    one keypoint    (and again, out of order)
PAIRS = [(0, 0), (0, 1), (1, 0), (1, 2), (1, 3), (4, 0), (2, 4), (3, 2), (3, 3), (2, 1), (4, 4)]


@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("dim,scale_ori", [(256, False), (128, False), (128, True)])
def test_indexed_equals_stacked_bitwise(dim, scale_ori, adaptive):
    """Every tensor and list of the dict == forward on {k: v[index]}: the fused first projection (256-d) and the staged one (128-d, with and without
    scales / oris), image_size given per image and absent (bounding boxes), fixed depth and adaptive depth + width."""
    require_gpu()
    model = _model(dim, scale_ori, adaptive)
    i0, i1 = [p[0] for p in PAIRS], [p[1] for p in PAIRS]
    for image_size in (True, False):
        store = _store(3, COUNTS, 200, dim, scale_ori, image_size)
        want = model({"image0": _stacked(store, i0), "image1": _stacked(store, i1)})
        got = model.match_pairs(store, PAIRS)
        _assert_same_dict(got, want, (dim, scale_ori, adaptive, image_size))
        assert model.last_pair_chunks == [(0, len(PAIRS))]
        assert got["stop"].dtype == torch.int64 and got["matches0"].dtype == torch.int64 and got["matches0"].shape == (len(PAIRS), 200)
        assert got["prune0"].dtype == (torch.int64 if adaptive else torch.float32)
        assert (got["matches0"][:3] > -1).any(1).all(), "the pairs of the two largest images must produce matches"    # not all -1: the equality above compares something
        assert int(got["stop"][5]) == 1 and (got["matches1"][5] == -1).all() and (got["matches0"][6] == -1).all()      # an empty image: stop 1, no match
        if adaptive:
            live = got["prune0"] >= 1                                       # padding rows carry 0
            assert (live & (got["prune0"] < got["stop"][:, None])).any(), "pruning_min_kpts = -1: these sizes must prune"
        one = model.match_pairs(store, [PAIRS[1]])                          # P = 1: `stop` is an int, as in forward
        _assert_same_dict(one, model({"image0": _stacked(store, [0]), "image1": _stacked(store, [1])}), "single pair")
        assert isinstance(one["stop"], int)


@pytest.mark.parametrize("adaptive", [False, True])
def test_two_stores_of_different_size(adaptive):
    """Side 1 indexes a second store (K1 = 3 images of N1 = 136 keypoints): n0 != n1, and each side's index is checked against its own store."""
    require_gpu()
    model = _model(adaptive=adaptive)
    s0, s1 = _store(3, COUNTS, 200), _store(4, [136, 70, 0], 136)
    pairs = [(0, 0), (1, 1), (4, 0), (0, 2), (3, 1), (2, 0), (1, 0), (0, 0)]
    want = model({"image0": _stacked(s0, [p[0] for p in pairs]), "image1": _stacked(s1, [p[1] for p in pairs])})
    got = model.match_pairs(s0, pairs, s1)
    _assert_same_dict(got, want)
    assert got["matches1"].shape == (len(pairs), 136) and len(got["matches"]) == len(pairs)
    with pytest.raises(ValueError, match=r"pairs \[1\]"):
        model.match_pairs(s0, [(0, 0), (0, 3)], s1)                         # 3 is an image of the first store only


def test_empty_pair_list_and_zero_keypoint_stores():
    require_gpu()
    model = _model()
    store = _store(3, COUNTS, 200)
    out = model.match_pairs(store, [])
    assert out["matches0"].shape == (0, 200) and out["matches0"].dtype == torch.int64 and out["matches"] == [] and out["scores"] == []
    assert out["stop"].shape == (0,) and out["stop"].dtype == torch.int64 and model.last_pair_chunks == []
    none = {"keypoints": torch.zeros(2, 0, 2, device="cuda"), "descriptors": torch.zeros(2, 0, 256, device="cuda")}
    got = model.match_pairs(store, [(0, 1), (4, 0)], none)                  # a store without keypoints on one side: the engine's empty result
    want = model({"image0": _stacked(store, [0, 4]), "image1": _stacked(none, [1, 0])})
    _assert_same_dict(got, want)


@pytest.mark.parametrize("adaptive", [False, True])
def test_chunked_equals_one_call_bitwise(adaptive):
    """P = 7 at N = 200 (caps 256): max_rows_per_call = 1536 plans 3 / 2 / 2, max_sim_elems_per_call = 131072 plans 2 / 2 / 2 / 1; every chunk writes its
    slice of the same outputs, so the dict — the log-assignment side output included — equals the one-call dict, deferred or not, whatever `pairs` is."""
    require_gpu()
    model = _model(adaptive=adaptive)
    model.return_log_assignment = True
    store = _store(5, [200, 131, 64, 1, 0, 177], 200)
    pairs = [(0, 1), (1, 5), (4, 2), (5, 0), (2, 2), (3, 1), (5, 1)]
    whole = model.match_pairs(store, pairs)
    assert model.last_pair_chunks == [(0, 7)] and whole["log_assignment"].shape == (7, 201, 201)
    _assert_same_dict(whole, model({"image0": _stacked(store, [p[0] for p in pairs]), "image1": _stacked(store, [p[1] for p in pairs])}))
    for limit, value, plan in (("max_rows_per_call", 1536, [(0, 3), (3, 5), (5, 7)]), ("max_sim_elems_per_call", 131072, [(0, 2), (2, 4), (4, 6), (6, 7)])):
        setattr(model, limit, value)
        for given in (pairs, torch.tensor(pairs, device="cuda"), torch.tensor(pairs, dtype=torch.int32)):
            model.last_pair_chunks = None
            _assert_same_dict(model.match_pairs(store, given), whole, (limit, type(given)))
            assert model.last_pair_chunks == plan
        handle = model.match_pairs(store, torch.tensor(pairs, device="cuda"), deferred=True, validate=False)
        assert hasattr(handle, "result") and model.last_pair_chunks == plan
        _assert_same_dict(handle.result(), whole, (limit, "deferred"))
        setattr(model, limit, None)
    from lightglue_amd import match_pairs
    model.max_rows_per_call = 1536
    per_pair = match_pairs(model, store, pairs)                             # the glue helper: one trimmed dict per pair
    counts = store["num_keypoints"].tolist()
    for b, (i, j) in enumerate(pairs):
        assert per_pair[b]["matches0"].shape == (counts[i],) and per_pair[b]["matches1"].shape == (counts[j],)
        assert torch.equal(per_pair[b]["matches0"], whole["matches0"][b, :counts[i]]) and torch.equal(per_pair[b]["matches"], whole["matches"][b])
        assert per_pair[b]["stop"] == int(whole["stop"][b])


def test_range_guard_covers_every_chunk():
    """check_finite == "first": the guard is armed for the whole first call, not for its first engine call — descriptors far outside the f16 operand range in an
    image that only the LAST chunk reads raise, and the message names the pair by its position in the list."""
    require_gpu()
    model = _model()
    model.max_rows_per_call = 1536
    store = _store(6, [200] * 5, 200, poison=False)
    store["descriptors"][4] *= 1e6
    pairs = [(0, 1), (1, 2), (2, 3), (3, 0), (0, 2), (1, 3), (2, 4)]
    assert model.check_finite == "first"
    with pytest.raises(_cabi.LightGlueAmdError, match="pair 6") as err:
        model.match_pairs(store, pairs)
    assert model.last_pair_chunks == [(0, 3), (3, 5), (5, 7)] and "LG_ERR_RANGE" in str(err.value) and "pair 5" not in str(err.value)
    model.match_pairs(store, pairs)                                         # second call: guard off (the documented default), no raise
    model.check_finite = True
    with pytest.raises(_cabi.LightGlueAmdError, match="pair 6"):
        model.match_pairs(store, pairs)


def test_device_index_guard():
    """validate=False hands a device pair list to the engine unchecked: its own check (init_state_kernel) must stop every index outside the store.  The stores
    are views [1 : K + 1] of a K + 2 allocation, so a read through -1 or K would still land in allocated memory — the status, not a fault, is the evidence."""
    require_gpu()
    model = _model()
    K = 4
    full = _store(7, [200] * (K + 2), 200, poison=False)
    store = {k: v[1:K + 1] for k, v in full.items()}
    assert all(v.is_contiguous() and v.data_ptr() != full[k].data_ptr() for k, v in store.items())
    good = model.match_pairs(store, [(0, 1), (2, 0)])
    pairs = torch.tensor([(0, 1), (-1, 2), (1, K), (2, 0), (K + 1, -7)], device="cuda")
    with pytest.raises(ValueError, match=r"pairs \[1, 2, 4\]"):
        model.match_pairs(store, pairs)                                     # the host check names the same pairs first
    with pytest.raises(_cabi.LightGlueAmdError, match="LG_ERR_INDEX") as err:
        model.match_pairs(store, pairs, validate=False)
    msg = str(err.value)
    assert "pair 1:" in msg and "pair 2:" in msg and "pair 4:" in msg and "pair 0:" not in msg and "pair 3:" not in msg
    handle = model.match_pairs(store, pairs, validate=False, deferred=True)           # what the engine wrote for the call: bad pairs are EMPTY pairs,
    with pytest.raises(_cabi.LightGlueAmdError, match="LG_ERR_INDEX"):                # their neighbours are untouched
        handle.result()
    ibuf, fbuf, lbuf = handle.buffers[:3]
    _, ioff, _, _, _, loff = _call.carve_plan(5, 200, 200, False)     # where the pieces of the three output allocations start
    m0, stop = lbuf[:5 * 200].view(5, 200), lbuf[loff[3]:loff[3] + 5]
    assert torch.equal(m0[0], good["matches0"][0]) and torch.equal(m0[3], good["matches0"][1])
    assert stop.tolist() == [int(good["stop"][0]), 1, 1, int(good["stop"][1]), 1]
    assert (m0[[1, 2, 4]] == -1).all() and (fbuf[:5 * 200].view(5, 200)[[1, 2, 4]] == 0).all()
    assert ibuf[ioff[5] + 10:ioff[5] + 15].tolist() == [_cabi.LG_OK, _cabi.LG_ERR_INDEX, _cabi.LG_ERR_INDEX, _cabi.LG_OK, _cabi.LG_ERR_INDEX]
    _assert_same_dict(model.match_pairs(store, [(0, 1), (2, 0)]), good)     # and the engine stays usable


def test_extractor_output_goes_straight_into_match_pairs():
    """SuperPoint on a 4-image batch -> its output dict, unchanged, is the store."""
    require_gpu()
    from lightglue_amd import SuperPoint
    torch.manual_seed(0)
    feats = SuperPoint().cuda().eval()({"image": torch.rand(4, 1, 64, 96, device="cuda")})
    assert feats["keypoints"].shape[0] == 4 and feats["keypoints"].shape[1] > 0 and "keypoint_scores" in feats
    model = _model()
    pairs = [(0, 1), (2, 3), (0, 2)]
    got = model.match_pairs(feats, pairs)
    keys = ("keypoints", "descriptors", "num_keypoints")
    want = model({"image0": {k: feats[k][[0, 2, 0]] for k in keys}, "image1": {k: feats[k][[1, 3, 2]] for k in keys}})
    _assert_same_dict(got, want)


@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("dim,scale_ori", [(256, False), (128, True)])
def test_every_route_of_the_one_call_path_returns_the_same_bits(dim, scale_ori, adaptive):
    """forward, forward_deferred, forward_raw and match_pairs with the identity pair list are ONE call path: the same dict, bit for bit, on inputs that every
    route has to normalise — image_size of side 0 a Python list (broadcast), float16 descriptors on side 1 only, non-contiguous keypoints on side 0."""
    require_gpu()
    model = _model(dim, scale_ori, adaptive)
    feats0, feats1 = _store(3, COUNTS, 200, dim, scale_ori), _store(4, [136, 70, 0, 136, 5], 136, dim, scale_ori)
    feats0["image_size"] = [1024, 768]
    feats1["descriptors"] = feats1["descriptors"].half()
    feats0["keypoints"] = feats0["keypoints"].transpose(1, 2).contiguous().transpose(1, 2)
    assert not feats0["keypoints"].is_contiguous() and feats0["keypoints"].shape == (5, 200, 2)
    data = {"image0": feats0, "image1": feats1}
    want = model(data)
    what = (dim, scale_ori, adaptive)
    _assert_same_dict(model.forward_deferred(data).result(), want, (*what, "deferred"))
    _assert_same_dict(model.match_pairs(feats0, [(i, i) for i in range(5)], feats1), want, (*what, "match_pairs"))
    assert model.last_pair_chunks == [(0, 5)]
    raw = model.forward_raw(data)
    assert raw["pruning"] is adaptive and (raw["status"] == _cabi.LG_OK).all() and raw["status"].shape == (5,)
    for key in ("matches0", "matches1", "stop"):
        assert raw[key].dtype == torch.int32 and want[key].dtype == torch.int64 and raw[key].shape == want[key].shape and torch.equal(raw[key].long(), want[key]), (what, key)
    for key in ("matching_scores0", "matching_scores1"):
        assert raw[key].dtype == torch.float32 and torch.equal(raw[key], want[key]), (what, key)
    assert want["matches0"].shape == (5, 200) and want["matches1"].shape == (5, 136)
    assert int(want["stop"][4]) == 1 and (want["matches1"][4] == -1).all()            # an empty image on side 0: stop 1, no match
    assert (want["matches0"] > -1).any() and sum(len(x) for x in want["matches"]) > 0     # not all -1: the equalities above compare something


def test_three_consumers_read_one_pair_list_alike():
    """The engine, the nearest-neighbour matcher and the verifier over ONE store (K = 4 images of 130 rows, dim 128: two row-workgroups of the NN kernel, and
    70 live rows = one full LG_NN_TILE plus a remainder) and ONE device pair list with two indices outside the store: each of them reports LG_ERR_INDEX for
    pairs 1 and 2 and for no other, leaves -1 / 0 / False in every row at or beyond num_keypoints, and gives the good pairs the bits of a call over them alone."""
    require_gpu()
    from lightglue_amd import NearestNeighborMatcher, TwoViewVerifier
    K, n, num = 4, 130, [130, 70, 0, 1]
    store = _store(23, num, n, dim=128)
    listed = [(0, 1), (-1, 1), (1, 4), (2, 0), (3, 3), (1, 0)]
    good_at = [0, 3, 4, 5]
    pairs, good_pairs, P = torch.tensor(listed, device="cuda"), [listed[p] for p in good_at], len(listed)
    want_status = [_cabi.LG_OK, _cabi.LG_ERR_INDEX, _cabi.LG_ERR_INDEX, _cabi.LG_OK, _cabi.LG_OK, _cabi.LG_OK]

    def written(handle):       # what a matcher wrote for the call, read from its three output allocations (as the engine's test above does)
        ibuf, fbuf, lbuf = handle.buffers[:3]
        _, ioff, _, foff, _, loff = _call.carve_plan(P, n, n, False)
        piece = lambda buf, off, k: buf[off[k]:off[k] + P * n].view(P, n)
        return {"matches0": piece(lbuf, loff, 0), "matches1": piece(lbuf, loff, 1), "matching_scores0": piece(fbuf, foff, 0), "matching_scores1": piece(fbuf, foff, 1),
                "status": ibuf[ioff[5] + 2 * P:ioff[5] + 3 * P].tolist()}

    def check_rows(m, fill, side):       # rows at or beyond num of the image a good pair reads; every row of a bad pair
        for p, ij in enumerate(listed):
            live = num[ij[side]] if p in good_at else 0
            assert (m[p, live:] == fill).all(), (p, side)

    nn_m0 = None
    for matcher in (_model(dim=128), NearestNeighborMatcher(mutual=True, ratio_threshold=0.95)):
        good = matcher.match_pairs(store, good_pairs)
        with pytest.raises(_cabi.LightGlueAmdError, match="LG_ERR_INDEX") as err:
            matcher.match_pairs(store, pairs, validate=False)
        msg = str(err.value)
        assert "pair 1:" in msg and "pair 2:" in msg and all(f"pair {p}:" not in msg for p in good_at)
        handle = matcher.match_pairs(store, pairs, validate=False, deferred=True)
        with pytest.raises(_cabi.LightGlueAmdError, match="LG_ERR_INDEX"):
            handle.result()
        got = written(handle)
        assert got["status"] == want_status, type(matcher).__name__
        for key, fill, side in (("matches0", -1, 0), ("matches1", -1, 1), ("matching_scores0", 0, 0), ("matching_scores1", 0, 1)):
            check_rows(got[key], fill, side)
            assert torch.equal(got[key][good_at], good[key]), (type(matcher).__name__, key)
        nn_m0, nn_good = got["matches0"], good
    assert (nn_good["matches0"][0] > -1).sum() >= 8           # the verifier below has something to verify

    verifier = TwoViewVerifier(model="homography", num_hypotheses=256)
    good = verifier.verify_pairs(store, good_pairs, nn_good)
    with pytest.raises(_cabi.LightGlueAmdError, match="LG_ERR_INDEX") as err:
        verifier.verify_pairs(store, pairs, nn_m0, validate=False)
    msg, got = str(err.value), err.value.outputs
    named = [p for p in range(P) if f"pair {p}:" in msg]
    assert [_cabi.LG_ERR_INDEX if p in named else _cabi.LG_OK for p in range(P)] == want_status and msg.count("LG_ERR_INDEX") == len(named)
    check_rows(got["inliers0"], False, 0)
    check_rows(got["matches0"], -1, 0)
    for key in ("models", "inliers0", "num_inliers", "matches0", "best_hypothesis"):
        assert torch.equal(got[key][good_at], good[key]), key
    assert all(torch.equal(got["matches"][p], good["matches"][q]) for q, p in enumerate(good_at))
    assert got["num_inliers"][[1, 2]].tolist() == [0, 0] and got["best_hypothesis"][[1, 2]].tolist() == [-1, -1] and len(got["matches"][1]) == len(got["matches"][2]) == 0
