"""The adaptive step behind one layer — early stop (ref :547-550, :645-656) and point pruning (ref :551-566, :636-643) — as a pure numpy function
of what the step reads, for ONE pair.  The arithmetic is that of oracle/lightglue_oracle.py `forward_pair` (the block behind its `layer_trace` call)
and `confidence_thresholds_f32`; nothing here is taken from lg_adaptive.hip.  tests/test_adaptive_oracle_cpu.py replays a whole adaptive
`forward_pair` through `step_pair` and pins every tie; tests/test_gpu_adaptive_stages.py holds the device's decide / compact kernels to it.

Comparisons, all in float32 as torch makes them between a float32 tensor and a Python scalar:
  stop   ratio = 1 - #(conf < thr[layer]) / (m + n) over BOTH images' live rows, m and n the ORIGINAL counts; the pair stops iff ratio > depth_confidence
  keep   mscore > 1 - width_confidence, or (early stop on) conf <= thr[layer]; applied to an image only while it has MORE than pruning_min_kpts rows
  empty  an image left without rows ends the pair at the next layer's guard (ref :539-540): final_layer = layer + 1
"""
import collections

import numpy as np

from oracle import lightglue_oracle as O

#: per pair: `stop`; per image (2-tuples): `keep` mask over the live rows, `dst` (destination row, -1 = dropped; kept rows ascending), `len`, `len_old`
#: (-1: pruning not applied), `ind` (new index set), `prune_inc` (increments of the prune counters, original index space); and the pair's `active` /
#: `final_layer` behind the step
Step = collections.namedtuple("Step", "stop keep dst len len_old ind prune_inc active final_layer")


def stop_ratio(conf0, conf1, len_orig, layer, n_layers):
    """ref :653-656: float32 sum of a 0 / 1 mask over the live rows, divided by the original point count, taken from 1 — all float32"""
    thr = O.confidence_thresholds_f32(n_layers)[layer]
    conf_all = np.concatenate([np.asarray(conf0, np.float32), np.asarray(conf1, np.float32)])
    below = (conf_all < thr).astype(np.float32).sum(dtype=np.float32)
    return np.float32(1.0) - np.float32(below) / np.float32(len_orig[0] + len_orig[1])


def step_pair(conf, mscore, length, len_orig, active, final_layer, ind, layer, n_layers, depth_confidence, width_confidence, pruning_min_kpts):
    """conf / mscore: per image a float32 array whose first length[image] entries are the live rows' token confidences / matchabilities (conf is not
    read when depth_confidence <= 0, mscore not when width_confidence <= 0); ind: per image the index set (first length[image] entries)."""
    assert 0 <= layer < n_layers - 1, "no adaptive step behind the last layer (ref :544-545)"
    do_stop, do_prune = depth_confidence > 0, width_confidence > 0   # ref :528-529
    thr = O.confidence_thresholds_f32(n_layers)[layer]
    live = [int(length[0]), int(length[1])]
    keep = [np.ones(n, bool) for n in live]
    len_old = [-1, -1]
    inc = [np.zeros(int(n), np.int64) for n in len_orig]
    new_ind = [np.asarray(ind[im])[:live[im]].copy() for im in (0, 1)]
    stop = False
    if active:   # a pair that has ended is not looked at again
        tok = [np.asarray(conf[im], np.float32)[:live[im]] for im in (0, 1)] if do_stop else [None, None]
        if do_stop:
            stop = bool(stop_ratio(tok[0], tok[1], len_orig, layer, n_layers) > np.float32(depth_confidence))   # ref :656: `>`
        if stop:
            active, final_layer = 0, layer
        else:
            for im in (0, 1):
                if not (do_prune and live[im] > pruning_min_kpts):   # ref :551 / :559: `>`
                    continue
                k = np.asarray(mscore[im], np.float32)[:live[im]] > np.float32(1.0 - width_confidence)   # ref :640: `>`
                if do_stop:
                    k = k | (tok[im] <= thr)   # ref :641-642: `<=`
                keep[im], len_old[im] = k, live[im]
                new_ind[im] = new_ind[im][k]
                inc[im][new_ind[im]] += 1   # ref :558 / :566
            if keep[0].sum() == 0 or keep[1].sum() == 0:   # ref :539-540 at the next iteration
                active, final_layer = 0, layer + 1
    dst = [np.where(k, np.cumsum(k) - 1, -1).astype(np.int64) for k in keep]
    return Step(stop, tuple(keep), tuple(dst), tuple(int(k.sum()) for k in keep), tuple(len_old), tuple(new_ind), tuple(inc), int(active), int(final_layer))


def apply_step(step, image, *arrays):
    """The rows of one image behind the step: arrays[j][:len_old][keep], by plain fancy indexing (x, cos, sin, ind, ... of the segment)"""
    rows = np.where(step.keep[image])[0]
    return tuple(np.asarray(a)[rows] for a in arrays)
