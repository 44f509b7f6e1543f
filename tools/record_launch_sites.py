#!/usr/bin/env python3
"""Launch sites per kernel class (`profile_read`) of one forward, for every case of tests/test_gpu_forward_plan.py; with --write the table becomes
tests/golden/forward_launch_sites.json.  The counts do not depend on the data (the host enqueues every layer whatever stops early), so a change of the
forward's orchestration is recorded on the library BEFORE the change (LIGHTGLUE_AMD_LIB selects it) and must reproduce the table exactly."""
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import gpu_util
from lightglue_amd import synthetic as synth

GOLDEN = ROOT / "tests" / "golden" / "forward_launch_sites.json"
SHAPE = (2, 129, 17)        # the smallest shapes that put a tile edge on both sides
MODES = {"fixed": dict(depth_confidence=-1, width_confidence=-1),
         "adaptive": dict(),                               # default pruning_min_kpts: nothing can prune
         "adaptive_prune64": dict(pruning_min_kpts=64)}
DIMS = (256, 128)
OPTION_SETS = {"defaults": {}, "fused_next=0": {"fused_next": 0}, "fused_prep=0": {"fused_prep": 0}, "adapt_gather=0": {"adapt_gather": 0}, "fused_tail=0": {"fused_tail": 0}}
DEFAULTS = {"fused_next": 1, "fused_prep": 1, "adapt_gather": 1, "fused_tail": 1}
PAIRS = [(0, 1), (1, 0), (0, 0)]     # the indexed path: 3 pairs over a 2-image store


def make_model(mode, dim):
    return gpu_util.make_model(synth.make_state_dict(0, input_dim=dim, recipe="A"), "f16x3", input_dim=dim, **MODES[mode])


def make_data(dim):
    return gpu_util.to_torch(synth.make_batch(7, *SHAPE, dim=dim))


def make_store():
    """A 2-image store: the image0 side of a batch of two, the second image with 17 live keypoints."""
    store = gpu_util.to_torch(synth.make_batch(7, 2, SHAPE[1], SHAPE[1]))["image0"]
    store["num_keypoints"] = torch.tensor([SHAPE[1], SHAPE[2]], dtype=torch.int32, device="cuda")
    return store


def profiled(model, options, run):
    """(launch sites per kernel class that ran, output) of one `run()` under the engine options `options`."""
    for key, value in {**DEFAULTS, **options}.items():
        model.set_option(key, value)
    model.profile(True)
    model.profile_read()
    out = run()
    torch.cuda.synchronize()
    counts = {name: int(cnt) for name, (_, cnt) in model.profile_read().items() if cnt}
    model.profile(False)
    return counts, out


def forward_cases(mode, dim):
    """{option set: (counts, output)} of one model / one batch"""
    model, data = make_model(mode, dim), make_data(dim)
    model(data)                                            # the first forward of a model runs with the range guard on
    return {name: profiled(model, options, lambda: model(data)) for name, options in OPTION_SETS.items()}


def match_pairs_case():
    model, store = make_model("fixed", 256), make_store()
    model.match_pairs(store, PAIRS)
    return profiled(model, {}, lambda: model.match_pairs(store, PAIRS))


def case_key(mode, dim, option_set):
    return f"{mode}/dim{dim}/{option_set}"


def record():
    table = {}
    for mode in MODES:
        for dim in DIMS:
            for name, (counts, _) in forward_cases(mode, dim).items():
                table[case_key(mode, dim, name)] = counts
    table["match_pairs/fixed/dim256/defaults"] = match_pairs_case()[0]
    return table


if __name__ == "__main__":
    table = record()
    text = json.dumps(table, indent=1, sort_keys=True) + "\n"
    if "--write" in sys.argv:
        GOLDEN.write_text(text)
    out = [a for a in sys.argv[1:] if a != "--write"]
    if out:
        Path(out[0]).write_text(text)
    print(text)
