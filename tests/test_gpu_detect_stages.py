"""The shared detection kernels of lg_extract.hip (nms_kernel, row_count_kernel, compact_kernel, radix_select / select_kernel, selected_rank)
and ALIKED's ak_decide_kernel / ak_refine_kernel at the sizes where their loops take more than one pass, and at ties.

Every map runs through BOTH callers: `superpoint_head.detect_keypoints` against `superpoint_oracle.detect_keypoints`, and `ALIKED.detect`
(a freshly constructed ALIKED per configuration; detection needs no weights) against `aliked_oracle.dkd_select` / `dkd_refine`.  Both oracles are
pinned to the reference's own outputs on the CPU (test_superpoint_head.py, test_aliked_oracle_cpu.py).  Maps come from the seeded generators of
tools/make_golden_aliked.py.

Bars.  Discrete outputs are exact: counts, the order of the keypoints, SuperPoint's integer positions and copied scores.  ALIKED returns refined
positions only, so its order and pixels are checked through them: output row i must be the refinement of the oracle's i-th pixel.  NMS maxima lie
more than r pixels apart and the bar is below 2e-4 px, so a wrong pixel or a swapped pair cannot pass.  Continuous outputs (knorm, pixel
keypoints, bilinear score) get 4 x T_ref of the same quantity (aliked_oracle.T_REF: the reference's own fp32 distance from the float64 oracle;
x 2 because the kernel sums in another order than torch's CPU kernels, x 2 for expf / division implementations).  T_ref of the pixel keypoints was
measured on a 600-wide map and is an error of knorm times (size - 1) / 2, so smaller maps get proportionally less, never more."""
import functools

import numpy as np
import pytest
import torch

import make_golden_aliked as G
from conftest import require_gpu
from oracle import aliked_oracle as AO
from oracle import superpoint_oracle as SO

ALL = 0.04        # an ALIKED threshold below every pixel of score_maps (uniform(0.05, 0.95)): every NMS maximum is a candidate, no fallback
SP_ALL = 0.0005   # SuperPoint's default threshold, likewise


@functools.lru_cache(maxsize=None)
def maps(kind, *args):
    m = {"uniform": G.score_maps, "quantised": G.quantised_maps, "plateau": G.plateau_maps}[kind](*args)
    m.setflags(write=False)
    return m


def check_superpoint(smap, radius, border, th, limit):
    """detect_keypoints == the oracle, exactly; returns the keypoints per image"""
    from lightglue_amd import superpoint_head as H
    b, h, w = smap.shape
    kw = dict(nms_radius=radius, remove_borders=border, detection_threshold=th, max_num_keypoints=limit)
    kp, sc, num = H.detect_keypoints(torch.from_numpy(np.ascontiguousarray(smap)).cuda(), capacity=h * w, **kw)
    kp, sc, num = kp.cpu().numpy(), sc.cpu().numpy(), num.cpu().tolist()
    out = []
    for i in range(b):
        rkp, rsc = SO.detect_keypoints(smap[i], **kw)
        assert num[i] == len(rsc), (i, num[i], len(rsc))
        np.testing.assert_array_equal(sc[i, :num[i]], rsc)
        np.testing.assert_array_equal(kp[i, :num[i]], rkp)
        out.append(rkp)
    return out


def check_aliked(smap, radius, th, mnk, image_size=None):
    """ALIKED.detect == dkd_select (counts, order, pixels) and dkd_refine (4 x T_ref); rows beyond the count are zero.  Returns (the oracle's
    indices per image, the kernel's pixel keypoints per image)."""
    from lightglue_amd import ALIKED
    model = ALIKED(detection_threshold=th, max_num_keypoints=mnk, nms_radius=radius)
    b, h, w = smap.shape
    isz = None if image_size is None else torch.tensor(image_size, dtype=torch.float32)
    kpts, ks, kn, counts = model.detect(torch.from_numpy(np.ascontiguousarray(smap)).cuda(), isz)
    torch.cuda.synchronize()
    kpts, ks, kn, counts = kpts.cpu().numpy(), ks.cpu().numpy(), kn.cpu().numpy(), counts.cpu().tolist()
    top_k, sth, n_limit = model._dkd()
    sel = AO.dkd_select(smap, radius, top_k, sth, n_limit, image_size)
    assert counts == [len(s) for s in sel]
    tol_px = 4 * AO.T_REF["keypoints"] * max(h, w) / 600.0
    got = []
    for i in range(b):
        n = counts[i]
        rkn, rkp, rks = AO.dkd_refine(smap[i], sel[i], radius)
        err = [float(np.abs(a - r).max(initial=0)) for a, r in ((kn[i, :n], rkn), (kpts[i, :n], rkp), (ks[i, :n], rks))]
        print(f"image {i}: {n} keypoints, knorm {err[0]:.2e} px {err[1]:.2e} score {err[2]:.2e}")
        assert err[1] <= tol_px, f"image {i}: pixel keypoints (order, pixel or refinement) off by {err[1]:.2e}"
        assert err[0] <= 4 * AO.T_REF["knorm"], f"image {i}: knorm off by {err[0]:.2e}"
        assert err[2] <= 4 * AO.T_REF["keypoint_scores"], f"image {i}: scores off by {err[2]:.2e}"
        assert not kpts[i, n:].any() and not ks[i, n:].any() and not kn[i, n:].any(), "rows beyond the count are zero"
        got.append(kpts[i, :n])
    return sel, got


def check_both(smap, radius, limit, sp_border=None, th=ALL, sp_th=SP_ALL):
    """the SuperPoint caller, ALIKED's threshold mode with n_limit and ALIKED's top-k mode (sort_always) on one map"""
    sp = check_superpoint(smap, radius, radius if sp_border is None else sp_border, sp_th, limit) if radius <= 4 else None
    sel_th, _ = check_aliked(smap, radius, th, -1 if limit is None else limit)
    sel_top, _ = check_aliked(smap, radius, -1, 20000 if limit is None else limit)
    return sp, sel_th, sel_top


# --------------------------------------------------------------------------- both callers
@pytest.mark.gpu
@pytest.mark.parametrize("limit", [None, 500])
def test_tall_map_second_prefix_stride(limit):
    """B = 2, 300 x 40, r = 2, about 780 candidates per image.  Rows 256 .. 299 are the only ones for which compact_kernel's prefix loop
    `for (yy = tid; yy < y; yy += 256)` takes its SECOND STRIDE: a wrong prefix there shifts or overwrites every candidate of those rows."""
    require_gpu()
    sp, sel, _ = check_both(maps("uniform", 1, 2, 300, 40), 2, limit)
    assert all(700 < len(s) for s in AO.dkd_select(maps("uniform", 1, 2, 300, 40), 2, -1, ALL, 20000))
    if limit is None:
        assert all((s // 40 >= 256).sum() > 50 for s in sel)     # candidates past the first stride exist


@pytest.mark.gpu
@pytest.mark.parametrize("limit", [None, 500])
def test_wide_map_three_x_passes(limit):
    """B = 2, 24 x 600, r = 2, about 860 candidates per image: three X-PASSES of compact_kernel's `x0 += 256` loop (the running offset carried
    across passes, the last pass partly beyond W) and ten NMS tiles across with their halos."""
    require_gpu()
    _, sel, _ = check_both(maps("uniform", 2, 2, 24, 600), 2, limit)
    if limit is None:
        assert all(((s % 600) >= 512).sum() > 50 for s in sel)   # candidates in the third pass exist


@pytest.mark.gpu
@pytest.mark.parametrize("limit", [None, 4096, 1500, 1025, 1024, 1023, 1])
def test_many_candidates_select_passes_and_rank_tiles(limit):
    """B = 1, 272 x 96, r = 1, border 1: about 4 500 candidates, so radix_select's histogram loop and select_kernel's `i0 += 1024` loop take
    five SELECT PASSES (`taken` / `eq_taken` carried across), and every sorted output above 1024 entries reaches selected_rank's second RANK
    TILE (4096: four tiles; none in top-k mode: all ~4 500 sorted, five tiles).  1025 / 1024 / 1023 sit on the tile edge; 1 is the smallest cut."""
    require_gpu()
    smap = maps("uniform", 3, 1, 272, 96)
    sp, sel_th, sel_top = check_both(smap, 1, limit)
    total = len(AO.dkd_select(smap, 1, -1, ALL, 20000)[0])
    assert 4096 < total < 5120, total                           # five passes of 1024
    assert len(sel_top[0]) == (total if limit is None else limit) == len(sp[0])


@pytest.mark.gpu
def test_plateau_need_inside_a_tie_group():
    """B = 3, 48 x 80, r = 2, limit 1100.  Image 0 is constant 0.5: all 44 x 76 = 3 344 interior pixels are NMS maxima with ONE key, so the
    radix select ends with prefix = that key and `need` = 1100 INSIDE A TIE GROUP: the kernel's rule keeps exactly the first 1100 in raster
    order (`eoff`, `eq_taken` across four select passes), and selected_rank orders equal keys by raster index.  Image 1 is 0.75 in the top half
    (22 x 76 = 1 672 maxima): the cut falls inside the better group and the whole 0.5 group below must go.  Image 2 is 0.75 in the top
    quarter (760 maxima): they are all kept (key > prefix) and the cut falls inside the lower group, need = 340."""
    require_gpu()
    smap = maps("plateau")
    sp, sel_th, sel_top = check_both(smap, 2, 1100, th=0.2)
    interior = np.array([y * 80 + x for y in range(2, 46) for x in range(2, 78)])
    below_step = np.array([y * 80 + x for y in range(14, 46) for x in range(2, 78)])   # rows 12, 13 are within r of the 0.75 rows: no maxima
    for sel in (sel_th, sel_top):
        assert sel[0].tolist() == interior[:1100].tolist()
        assert sel[1].tolist() == interior[:1100].tolist()                  # 1 100 of the 1 672 in the upper group, none from below
        assert sel[2].tolist() == interior[:760].tolist() + below_step[:340].tolist()
    for b, want in enumerate((interior[:1100], interior[:1100], np.concatenate([interior[:760], below_step[:340]]))):
        np.testing.assert_array_equal(sp[b], np.stack([want % 80, want // 80], -1).astype(np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("limit", [1500, 3000])
def test_quantised_map_large_tie_groups(limit):
    """The 272 x 96 map rounded to 1/16: about 5 100 candidates (plateau pixels are all maxima) over 15 distinct values, so every radix pass
    after the first sees one bucket only, the cut splits a group of several hundred (`need` inside a tie group, spread over all five select
    passes) and the ranking of every group is by raster index."""
    require_gpu()
    smap = maps("quantised", 3, 1, 272, 96)
    _, sel_th, _ = check_both(smap, 1, limit)
    kept = smap[0].reshape(-1)[sel_th[0]]
    everything = smap[0].reshape(-1)[AO.dkd_select(smap, 1, -1, ALL, 20000)[0]]
    assert len(np.unique(everything)) <= 16 and (everything == kept.min()).sum() > (kept == kept.min()).sum() > 1   # the cut splits a group


@pytest.mark.gpu
def test_ulp_ladder_last_radix_byte():
    """47 x 62, r = 2: 108 isolated peaks every 2r + 1 pixels on a 0.01 background, valued 0x3F000001 .. 0x3F00006C in shuffled order; the limit
    is half of them.  All keys agree in their top 24 bits, so only radix_select's LAST RADIX BYTE (shift 0) separates kept from dropped, and the
    ranking must order by single ulps."""
    require_gpu()
    smap, n = G.ulp_ladder_map(1, 47, 62, 2)
    assert n == 108
    sp, sel_th, sel_top = check_both(smap, 2, n // 2, th=0.2, sp_th=0.2)
    for sel in (sel_th, sel_top):
        bits = smap[0].reshape(-1)[sel[0]].view(np.uint32)
        assert bits.tolist() == list(range(0x3F000000 + n, 0x3F000000 + n - n // 2, -1))


@pytest.mark.gpu
@pytest.mark.parametrize("radius", [3, 4, 5, 7, 8])
@pytest.mark.parametrize("limit", [None, 20])
def test_radii(radius, limit):
    """B = 2, 70 x 130.  r = 3, 4 (SuperPoint and ALIKED): the widest halos of the NR = 4 instance of nms_kernel.  r = 5, 7, 8 (ALIKED only;
    SuperPoint's ABI stops at 4): the NR = 8 instance, whose 2r halo at r = 8 spans a whole 16-row tile on each side, and the 289-tap soft-argmax of
    ak_refine_kernel."""
    require_gpu()
    check_both(maps("uniform", 4, 2, 70, 130), radius, limit)


# --------------------------------------------------------------------------- ALIKED only
@pytest.mark.gpu
def test_batch_wide_fallback_rule():
    """ak_decide_kernel's BATCH-WIDE `any`: B = 3 with every pixel below scores_th = 0.99 -> every image falls back to its OWN mean (three
    different thresholds); one pixel of ONE image above -> no fallback anywhere, and the other two images return 0 keypoints."""
    require_gpu()
    smap = maps("uniform", 5, 3, 40, 56).copy()
    sel, _ = check_aliked(smap, 2, 0.99, -1)
    means = AO.image_mean(smap)
    assert len(set(means.tolist())) == 3 and all(len(s) > 50 for s in sel)
    for b in range(3):   # the mean of THIS image decides, not another image's or the batch's
        assert sel[b].tolist() == np.nonzero(AO.dkd_nms(smap, 2)[b].reshape(-1) > means[b])[0].tolist()
    smap[1, 20, 30] = 0.995
    sel, _ = check_aliked(smap, 2, 0.99, -1)
    assert [s.tolist() for s in sel] == [[], [20 * 56 + 30], []]


@pytest.mark.gpu
def test_mean_mode():
    """scores_th <= 0 (`ALIKED(detection_threshold=-1, max_num_keypoints=-1)`: top_k = -1, so threshold mode): the per-image mean, always."""
    require_gpu()
    smap = maps("uniform", 6, 2, 40, 56)
    sel, _ = check_aliked(smap, 2, -1, -1)
    means = AO.image_mean(smap)
    for b in range(2):
        assert sel[b].tolist() == np.nonzero(AO.dkd_nms(smap, 2)[b].reshape(-1) > means[b])[0].tolist() and len(sel[b]) > 50


@pytest.mark.gpu
def test_all_zero_map_gives_no_keypoints():
    """an all-zero image (beside an ordinary one, and alone): count 0, zeroed rows; alone, the fallback's mean threshold is 0 and nothing is > 0"""
    require_gpu()
    smap = maps("uniform", 6, 2, 40, 56).copy()
    smap[0] = 0
    sel, _ = check_aliked(smap, 2, 0.2, -1)
    assert len(sel[0]) == 0 and len(sel[1]) > 50
    for th, mnk in ((0.2, -1), (0.2, 10), (-1, 10), (-1, -1)):
        sel, _ = check_aliked(smap[:1], 2, th, mnk)
        assert len(sel[0]) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("radius", [2, 3])
def test_image_size_moves_only_the_far_borders(radius):
    """`image_size` = (w', h') (truncated like .long()): in threshold mode below n_limit the detections are exactly the full run's with
    x < w' - r and y < h' - r, in the same order and with the same coordinates (the map's own W and H normalise them, not image_size).
    Asserted as a property of the kernel's own two outputs and against the oracle."""
    require_gpu()
    smap = maps("uniform", 7, 2, 40, 56)
    sizes = [[49.9, 33.0], [56.0, 21.5]]
    sel_full, got_full = check_aliked(smap, radius, 0.2, -1)
    sel_part, got_part = check_aliked(smap, radius, 0.2, -1, image_size=sizes)
    for b, (wl, hl) in enumerate(sizes):
        y, x = np.divmod(sel_full[b], 56)
        keep = (x < int(wl) - radius) & (y < int(hl) - radius)
        assert 0 < keep.sum() < len(keep)
        assert sel_part[b].tolist() == sel_full[b][keep].tolist()
        np.testing.assert_array_equal(got_part[b], got_full[b][keep])
