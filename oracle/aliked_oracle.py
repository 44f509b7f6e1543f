"""TEST INFRASTRUCTURE ONLY — numpy restatement of the reference's ALIKED stages: the encoder, DKD and SDDH.

Only tests/ may import this file; the product path (lightglue_amd/aliked.py -> lg_aliked.hip, lg_extract.hip) never does.
Follows lightglue/aliked.py by line number: simple_nms (:68-91, the same function as superpoint.py:52-70, so `superpoint_oracle.simple_nms`
is reused), DKD.forward (:127-261), get_patches (:48-65), SDDH.forward (:534-609), the dense map of extract_dense_map (:728-738) and the pixel
keypoints of ALIKED.forward (:757), and the encoder of extract_dense_map (:709-740) with its blocks (InputPadder :264-288, DeformableConv2d
:328-349, ConvBlock :412-415, ResBlock :460-476) in `encoder`, BatchNorm applied as written (never folded).  torch ops are restated from
their documented semantics: `nn.Upsample(mode="bilinear", align_corners=True)`, `F.grid_sample(mode="bilinear", padding_mode="zeros",
align_corners=True)`, `F.normalize(p=2, eps=1e-12)`, `nn.SELU`, `nn.BatchNorm2d` (eval), `nn.AvgPool2d`, `F.pad(mode="replicate")`,
`torchvision.ops.deform_conv2d`.
Everything discrete (NMS, thresholds, selection, `.long()` truncations, patch corners) is computed on the fp32 values in the reference's
operation order; everything continuous is float64.  Parity with the reference's own modules is pinned by tests/golden/aliked_stages/*.npz
(tools/make_golden_aliked.py --stages) in tests/test_aliked_oracle_cpu.py."""
from __future__ import annotations

import numpy as np

from .superpoint_oracle import simple_nms

F32 = np.float32
SELU_ALPHA, SELU_SCALE = 1.6732632423543772848170429916717, 1.0507009873554804934193349852946


def selu(x: np.ndarray) -> np.ndarray:
    return SELU_SCALE * np.where(x > 0, x, SELU_ALPHA * np.expm1(np.minimum(x, 0)))


# --------------------------------------------------------------------------- DKD: which pixels
def dkd_nms(scores: np.ndarray, radius: int, image_size=None) -> np.ndarray:
    """ref :141-153.  scores [B, H, W] fp32 -> NMS scores with the borders zeroed at depth `radius`; the far borders start at the truncated
    `image_size[b] = (w, h)` when it is given (:146-150)."""
    scores = np.ascontiguousarray(scores, dtype=F32)
    b, h, w = scores.shape
    nms = np.stack([simple_nms(scores[i], radius) for i in range(b)])                    # ref :141
    nms[:, :radius, :] = 0                                                               # ref :144
    nms[:, :, :radius] = 0                                                               # ref :145
    for i in range(b):
        wl, hl = (int(image_size[i][0]), int(image_size[i][1])) if image_size is not None else (w, h)   # ref :148 (.long(): truncation)
        nms[i, max(hl - radius, 0):, :] = 0                                              # ref :149 / :152
        nms[i, :, max(wl - radius, 0):] = 0                                              # ref :150 / :153
    return nms


def image_mean(scores: np.ndarray) -> np.ndarray:
    """The per-image mean threshold (ref :163, :166) as the kernel forms it: a float64 sum over the map, divided, rounded to fp32 once."""
    b = scores.shape[0]
    return (scores.reshape(b, -1).astype(np.float64).sum(axis=1) / float(scores[0].size)).astype(F32)


def best_first(values: np.ndarray, limit: int) -> np.ndarray:
    """positions of the `limit` largest values: score descending, the lower position first among equal scores; a tie group the cut splits
    keeps its lowest positions.  (torch.topk / sort leave both open; this is the rule of select_kernel / selected_rank.)"""
    return np.lexsort((np.arange(len(values)), -values.astype(np.float64)))[:limit]


def dkd_select(scores: np.ndarray, radius: int, top_k: int, scores_th: float, n_limit: int, image_size=None) -> list:
    """ref :127-179: the raster indices (y * W + x) of every image's keypoints, in output order.  All comparisons are exact on fp32 values.

    * top_k > 0: the `top_k` best POSITIVE NMS maxima, best first (the reference's topk pads with zero-score pixels in an unspecified
      order when there are fewer; the kernels return fewer).
    * else threshold mode: nms > scores_th; the per-image mean replaces scores_th only when NO pixel of the WHOLE batch passes (:162) or
      when scores_th <= 0 (:165-167).  Raster order (:173); more than `n_limit` hits: the n_limit best, best first (:174-178).
    * Coordinates: y, x = divmod(index, W) with the MAP's own W.  The reference reassigns `w, h` from `image_size` (:148) and then forms
      `indices % w` and `wh` from them (:181, :197), which gives the pixel only when image_size equals the map size; the kernels (and
      this oracle) always use the map's W and H, so `image_size` moves the far borders and nothing else."""
    scores = np.ascontiguousarray(scores, dtype=F32)
    b = scores.shape[0]
    nms = dkd_nms(scores, radius, image_size).reshape(b, -1)
    flat = scores.reshape(b, -1)
    out = []
    if top_k > 0:                                                                        # ref :156-158
        for i in range(b):
            idx = np.nonzero(nms[i] > 0)[0]
            out.append(idx[best_first(flat[i][idx], top_k)])
        return out
    th = np.full(b, F32(scores_th), F32)
    if not (scores_th > 0 and (nms > F32(scores_th)).any()):                             # ref :160-167
        th = image_mean(scores)
    for i in range(b):
        idx = np.nonzero(nms[i] > th[i])[0]                                              # ref :173
        if len(idx) > n_limit:                                                           # ref :174-178
            idx = idx[best_first(flat[i][idx], n_limit)]
        out.append(idx)
    return out


# --------------------------------------------------------------------------- DKD: sub-pixel refinement
def bilinear_zeros(m: np.ndarray, ix: np.ndarray, iy: np.ndarray) -> np.ndarray:
    """grid_sample(bilinear, align_corners=True, padding zeros) of m [H, W, ...] at pixel positions (ix, iy) [N] -> [N, ...], float64."""
    h, w = m.shape[:2]
    x0, y0 = np.floor(ix), np.floor(iy)
    tx, ty = ix - x0, iy - y0
    out = np.zeros((len(ix),) + m.shape[2:], np.float64)
    for dy, dx, wgt in ((0, 0, (1 - tx) * (1 - ty)), (0, 1, tx * (1 - ty)), (1, 0, (1 - tx) * ty), (1, 1, tx * ty)):
        x, y = (x0 + dx).astype(np.int64), (y0 + dy).astype(np.int64)
        ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        vals = m[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)]
        out += vals * (wgt * ok).reshape((-1,) + (1,) * (m.ndim - 2))
    return out


def dkd_refine(scores: np.ndarray, indices: np.ndarray, radius: int):
    """ref :188-233 and :757 for ONE image: scores [H, W], raster indices [M] -> (knorm [M, 2] in [-1, 1], pixel keypoints [M, 2],
    bilinear score [M]), float64.  Soft-argmax with temperature 0.1 over the (2r+1)^2 window (nn.Unfold: zero padding)."""
    s = scores.astype(np.float64)
    h, w = s.shape
    r, k = radius, 2 * radius + 1
    pad = np.zeros((h + 2 * r, w + 2 * r))
    pad[r:r + h, r:r + w] = s
    ys, xs = np.divmod(np.asarray(indices, np.int64), w)                                 # ref :196-199
    win = np.stack([pad[ys + dy, xs + dx] for dy in range(k) for dx in range(k)], 1)     # ref :188-195  [M, k*k], row-major window
    grid = np.array([[dx - r, dy - r] for dy in range(k) for dx in range(k)], np.float64)   # ref :120-125 hw_grid, (x, y)
    x_exp = np.exp((win - win.max(axis=1, keepdims=True)) / 0.1)                         # ref :202-205
    resid = x_exp @ grid / x_exp.sum(axis=1, keepdims=True)                              # ref :208-210
    wh = np.array([w - 1, h - 1], np.float64)
    knorm = (np.stack([xs, ys], 1) + resid) / wh * 2 - 1                                 # ref :223-224
    pix = (knorm + 1) / 2 * wh                                                           # grid_sample's un-normalisation
    kscore = bilinear_zeros(s, pix[:, 0], pix[:, 1])                                     # ref :226-233
    return knorm, wh * (knorm + 1) / 2.0, kscore                                         # ref :757


# --------------------------------------------------------------------------- SDDH
def padded_dims(h: int, w: int, div: int = 32):
    """InputPadder (ref :267-277) -> (Hp, Wp, top, left)"""
    ph, pw = ((h // div + 1) * div - h) % div, ((w // div + 1) * div - w) % div
    return h + ph, w + pw, ph // 2, pw // 2


def upsample_align(m: np.ndarray, hp: int, wp: int) -> np.ndarray:
    """nn.Upsample(bilinear, align_corners=True) of m [h, w, C] to [hp, wp, C], float64"""
    h, w = m.shape[:2]

    def axis(n_in, n_out):
        src = np.arange(n_out, dtype=np.float64) * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
        i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
        return i0, np.minimum(i0 + 1, n_in - 1), src - i0

    y0, y1, ty = axis(h, hp)
    x0, x1, tx = axis(w, wp)
    m = m.astype(np.float64)
    rows = m[y0] * (1 - ty)[:, None, None] + m[y1] * ty[:, None, None]
    return rows[:, x0] * (1 - tx)[None, :, None] + rows[:, x1] * tx[None, :, None]


def dense_map(levels, shape) -> np.ndarray:
    """ref :728-738: x1234 [B, H, W, 128] from the level maps x1 .. x4 [B, Hp >> s, Wp >> s, 32] (after conv + SELU): upsample to the padded
    size, concatenate, L2-normalise over channels, unpad."""
    h, w = shape
    hp, wp, pt, pl = padded_dims(h, w)
    out = []
    for b in range(levels[0].shape[0]):
        x = np.concatenate([upsample_align(l[b], hp, wp) for l in levels], axis=-1)       # ref :728-731
        x = x / np.maximum(np.sqrt((x * x).sum(-1, keepdims=True)), 1e-12)               # ref :734
        out.append(x[pt:pt + h, pl:pl + w])                                              # ref :737
    return np.stack(out)


def keypoint_pixels(knorm: np.ndarray, h: int, w: int):
    """ref :546, :551 and get_patches :52-54 in fp32, in the reference's operation order (the truncations are discontinuous, so they must see the
    reference's roundings): (kptsi_wh [N, 2] fp32, patch corner [N, 2] int (x, y))."""
    wh = np.array([w - 1, h - 1], F32)
    kwh = (knorm.astype(F32) / F32(2) + F32(0.5)) * wh                                   # ref :546
    long = np.trunc(kwh).astype(np.int64)                                                # ref :551 .long()
    corner = np.trunc(long.astype(F32) - F32(1.5) + F32(1)).astype(np.int64)             # ref :52 (ps = 3)
    corner[:, 0] = np.clip(corner[:, 0], 0, w - 1 - 3)                                   # ref :53
    corner[:, 1] = np.clip(corner[:, 1], 0, h - 1 - 3)                                   # ref :54
    return kwh, corner


def sddh(levels, shape, knorm, weights: dict, n_pos: int) -> list:
    """ref :534-609 on the dense map of `levels`: knorm = per image [N_b, 2] normalised keypoints -> per image descriptors [N_b, 128], float64.
    `weights`: desc_head.offset_conv.0 / .2 (weight, bias), desc_head.sf_conv.weight, desc_head.agg_weights."""
    h, w = shape
    x = dense_map(levels, shape)
    g = lambda n: np.asarray(weights[f"desc_head.{n}"], np.float64)   # noqa: E731
    w0, b0, w2, b2 = g("offset_conv.0.weight"), g("offset_conv.0.bias"), g("offset_conv.2.weight")[:, :, 0, 0], g("offset_conv.2.bias")
    wsf, agg = g("sf_conv.weight")[:, :, 0, 0], g("agg_weights")
    wh = np.array([w - 1, h - 1], np.float64)
    max_offset = max(h, w) / 4.0                                                         # ref :539
    out = []
    for b in range(x.shape[0]):
        k = np.asarray(knorm[b], F32).reshape(-1, 2)
        if len(k) == 0:
            out.append(np.zeros((0, 128)))
            continue
        kwh, corner = keypoint_pixels(k, h, w)
        patch = np.stack([x[b, corner[:, 1] + dy, corner[:, 0] + dx] for dy in range(3) for dx in range(3)], 1)   # ref :48-65  [N, 9 (dy, dx), C]
        off = np.einsum("ntc,oct->no", patch, w0.reshape(w0.shape[0], w0.shape[1], 9)) + b0   # ref :561 offset_conv.0 (3 x 3, no padding)
        off = selu(off) @ w2.T + b2                                                      # SELU, offset_conv.2 (1 x 1)
        off = np.clip(off, -max_offset, max_offset)                                      # ref :561-563
        off = off.reshape(len(k), 2, n_pos).transpose(0, 2, 1)                           # ref :571-573  [N, n_pos, (x, y)]
        pos = kwh.astype(np.float64)[:, None, :] + off                                   # ref :577
        pos = 2.0 * pos / wh - 1                                                         # ref :578
        pix = (pos + 1) / 2 * wh                                                         # grid_sample's un-normalisation
        feat = bilinear_zeros(x[b], pix[..., 0].ravel(), pix[..., 1].ravel()).reshape(len(k), n_pos, -1)   # ref :582-587  [N, n_pos, C]
        feat = selu(feat @ wsf.T)                                                        # ref :591
        d = np.einsum("npc,pcd->nd", feat, agg)                                          # ref :596-598
        out.append(d / np.maximum(np.sqrt((d * d).sum(-1, keepdims=True)), 1e-12))       # ref :606
    return out


# --------------------------------------------------------------------------- encoder (extract_dense_map, ref :709-740)
BN_EPS = 1e-5                                                                            # nn.BatchNorm2d's default


def replicate_pad(x: np.ndarray, div: int = 32) -> np.ndarray:
    """InputPadder(div).pad (ref :267-281) of x [B, H, W, C]: replicate padding, centred, the odd pixel on the far side"""
    h, w = x.shape[1:3]
    hp, wp, pt, pl = padded_dims(h, w, div)
    return np.pad(x, ((0, 0), (pt, hp - h - pt), (pl, wp - w - pl), (0, 0)), mode="edge")


def conv2d(x: np.ndarray, weight: np.ndarray, bias=None) -> np.ndarray:
    """nn.Conv2d(k x k, stride 1, zero padding k // 2) of x [B, H, W, Cin] with weight [Cout, Cin, k, k] -> [B, H, W, Cout], float64"""
    weight = np.asarray(weight, np.float64)
    k = weight.shape[2]
    r = k // 2
    b, h, w, _ = x.shape
    xp = np.pad(np.asarray(x, np.float64), ((0, 0), (r, r), (r, r), (0, 0)))
    out = np.zeros((b, h, w, weight.shape[0]))
    for i in range(k):
        for j in range(k):
            out += xp[:, i:i + h, j:j + w] @ weight[:, :, i, j].T
    return out if bias is None else out + np.asarray(bias, np.float64)


def batch_norm(x: np.ndarray, weights: dict, name: str, eps: float = BN_EPS) -> np.ndarray:
    """nn.BatchNorm2d in eval mode, as written (not folded into the convolution): (x - running_mean) / sqrt(running_var + eps) * weight + bias"""
    g = lambda n: np.asarray(weights[f"{name}.{n}"], np.float64)   # noqa: E731
    return (x - g("running_mean")) / np.sqrt(g("running_var") + eps) * g("weight") + g("bias")


def avg_pool(x: np.ndarray, f: int) -> np.ndarray:
    """nn.AvgPool2d(f, stride f) of x [B, H, W, C], H and W multiples of f"""
    b, h, w, c = x.shape
    return x.reshape(b, h // f, f, w // f, f, c).mean(axis=(2, 4))


def deform_positions(offsets: np.ndarray):
    """sample positions of a 3 x 3, padding 1, stride 1 deformable convolution: offsets [B, h, w, 18], tap k = 3 i + j with (dy, dx) in channels
    (2k, 2k + 1) -> (py, px) [B, h, w, 9] = the tap's own pixel (y - 1 + i, x - 1 + j) plus its offset"""
    b, h, w, _ = offsets.shape
    ys, xs = np.arange(h, dtype=np.float64)[None, :, None, None], np.arange(w, dtype=np.float64)[None, None, :, None]
    ki, kj = np.divmod(np.arange(9), 3)
    return ys - 1 + ki + offsets[..., 0::2], xs - 1 + kj + offsets[..., 1::2]


def sample_classes(py: np.ndarray, px: np.ndarray, h: int, w: int):
    """where deformable samples fall on an h x w map -> boolean (inside, partly, outside): `outside` gives a zero sample (torchvision: py <= -1, py >= h,
    px <= -1 or px >= w), `inside` has its whole bilinear cell on the map (0 <= py <= h - 1, 0 <= px <= w - 1), `partly` is the rest: a cell that straddles
    the border, some corners dropped"""
    outside = (py <= -1) | (py >= h) | (px <= -1) | (px >= w)
    inside = (py >= 0) & (py <= h - 1) & (px >= 0) & (px <= w - 1)
    return inside, ~inside & ~outside, outside


def deform_conv2d(x: np.ndarray, offsets: np.ndarray, weight: np.ndarray) -> np.ndarray:
    """torchvision.ops.deform_conv2d (3 x 3, padding 1, stride 1, one offset group, no mask, no bias) from its documented rules: x [B, h, w, Cin],
    offsets [B, h, w, 18] (already clamped), weight [Cout, Cin, 3, 3] -> [B, h, w, Cout].  A sample outside (-1, h) x (-1, w) is zero; otherwise it is
    the bilinear mix of the four pixels around it, each of which counts as zero on its own when it lies off the map."""
    b, h, w, cin = x.shape
    weight = np.asarray(weight, np.float64)
    py, px = deform_positions(offsets)
    _, _, outside = sample_classes(py, px, h, w)
    out = np.zeros((b, h, w, weight.shape[0]))
    for i in range(b):
        cols = bilinear_zeros(x[i], px[i].ravel(), py[i].ravel()).reshape(h, w, 9, cin)   # the per-corner rule
        cols[outside[i]] = 0                                                             # the whole-sample rule (implied by the corners; stated)
        out[i] = np.einsum("hwkc,ock->hwo", cols, weight.reshape(weight.shape[0], cin, 9))
    return out


def encoder(image: np.ndarray, weights: dict, trace: dict = None, eps: float = BN_EPS):
    """ref extract_dense_map (:709-740) behind forward's gray broadcast (:744-745): image [B, 1|3, H, W], `weights` the state dict under the
    reference's names -> (levels, scores): x1 .. x4 after conv1 .. conv4 + SELU as [B, Hp >> s, Wp >> s, 32] for s = 0, 1, 3, 5 over the whole padded
    extent (the layout of ALIKED.level_maps), and the unpadded score map [B, H, W]; all float64.  Independent of n_pos.  `trace`, when given, receives
    "offsets": the clamped offsets [B, h, w, 18] of block3.conv1, block3.conv2, block4.conv1, block4.conv2, in that order.  `eps` is BatchNorm's."""
    g = lambda n: np.asarray(weights[n], np.float64)   # noqa: E731
    x = np.asarray(image, np.float64)
    _, c, h, w = x.shape
    assert c in (1, 3)
    if c == 1:
        x = np.concatenate([x, x, x], axis=1)                                            # ref :744-745
    hp, wp, pt, pl = padded_dims(h, w)
    x = replicate_pad(x.transpose(0, 2, 3, 1))                                           # ref :712-713, NHWC from here on
    offsets = []

    def conv(name, t):
        if f"{name}.weight" in weights:
            return conv2d(t, g(f"{name}.weight"))
        lh, lw = t.shape[1:3]
        max_offset = max(lh, lw) / 4.0                                                   # ref :329-330
        off = conv2d(t, g(f"{name}.offset_conv.weight"), g(f"{name}.offset_conv.bias"))   # ref :332
        off = np.clip(off, -max_offset, max_offset)                                      # ref :340
        offsets.append(off)
        return deform_conv2d(t, off, g(f"{name}.regular_conv.weight"))                   # ref :341-348

    def res_block(name, t):                                                              # ref :460-476
        out = selu(batch_norm(conv(f"{name}.conv1", t), weights, f"{name}.bn1", eps))
        out = batch_norm(conv(f"{name}.conv2", out), weights, f"{name}.bn2", eps)
        return selu(out + conv2d(t, g(f"{name}.downsample.weight"), g(f"{name}.downsample.bias")))

    x1 = selu(batch_norm(conv("block1.conv1", x), weights, "block1.bn1", eps))           # ref :413
    x1 = selu(batch_norm(conv("block1.conv2", x1), weights, "block1.bn2", eps))          # ref :414
    x2 = res_block("block2", avg_pool(x1, 2))                                            # ref :717-718
    x3 = res_block("block3", avg_pool(x2, 4))                                            # ref :719-720
    x4 = res_block("block4", avg_pool(x3, 4))                                            # ref :721-722
    levels = [selu(conv2d(t, g(f"conv{i + 1}.weight"))) for i, t in enumerate((x1, x2, x3, x4))]   # ref :724-727
    x1234 = np.stack([np.concatenate([upsample_align(l[b], hp, wp) for l in levels], axis=-1) for b in range(x.shape[0])])   # ref :728-731
    s = x1234
    for i in (0, 2, 4):                                                                  # ref :733 (:671-679)
        s = selu(conv2d(s, g(f"score_head.{i}.weight")))
    s = conv2d(s, g("score_head.6.weight"))[..., 0]
    scores = 1.0 / (1.0 + np.exp(-s))
    if trace is not None:
        trace["offsets"] = offsets
    return levels, scores[:, pt:pt + h, pl:pl + w]                                       # ref :738


# T_ref: the largest deviation of the REFERENCE's fp32 results from this float64 oracle over all stage fixtures, per quantity (measured and
# asserted in tests/test_aliked_oracle_cpu.py, which states where each figure comes from).  The GPU stage tests allow the kernels 4 x T_ref.
T_REF = {"knorm": 1.7e-7, "keypoints": 4.6e-5, "keypoint_scores": 3.6e-5, "descriptors": 1.1e-6,
         "x1": 1.6e-6, "x2": 2.2e-6, "x3": 3.2e-6, "x4": 1.6e-6, "encoder_scores": 7.2e-6}
