"""What STORING descriptors as float16 costs, pinned to the reference: the numpy oracle (oracle/lightglue_oracle.py) on the committed matcher fixtures with
`descriptors.astype(float16).astype(float32)`, against the reference's own golden outputs on the fp32 descriptors (tests/golden/*.npz).

    python tools/f16_descriptor_drift.py            # the four pinned fixtures -> tests/golden/f16_descriptor_drift.json (tests/test_f16_descriptors_cpu.py)
    python tools/f16_descriptor_drift.py --all      # every matcher fixture, as the markdown table of the README; nothing is written

Per fixture: index flips (matches0 and matches1 together), max |d score| over both sides at equal indices, and the range of the descriptor norms.  The figure
contains the oracle's own fp32 distance from the reference (<= 2e-4, recipe E 7e-4: tests/test_oracle_golden.py); the rounding of the descriptors dominates it."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests"))

PINNED = ("nonadaptive_bbox_300x200", "disk128_256x320", "trained_stats_512", "trained_stats_confident_512")
RECORD = ROOT / "tests" / "golden" / "f16_descriptor_drift.json"


def drift(name: str) -> dict:
    import make_golden
    from conftest import load_golden, oracle_conf_for
    from oracle import lightglue_oracle as O
    meta, gold = load_golden(name)
    sd, data = make_golden.case_inputs(meta["case"])
    norms = np.concatenate([np.linalg.norm(np.asarray(data[k]["descriptors"], np.float64), axis=-1).ravel() for k in ("image0", "image1")])
    rounded = {k: {**v, "descriptors": np.asarray(v["descriptors"]).astype(np.float16).astype(np.float32)} for k, v in data.items()}
    out = O.forward(sd, oracle_conf_for(meta["case"]), rounded)
    flips, entries, worst = 0, 0, 0.0
    for side in ("0", "1"):
        m, gm = np.asarray(out["matches" + side]), gold["matches" + side]
        s, gs = np.asarray(out["matching_scores" + side]), gold["matching_scores" + side]
        same = m == gm
        flips += int((~same).sum()); entries += int(same.size)
        if same.any():
            worst = max(worst, float(np.abs(s - gs)[same].max()))
    return {"index_flips": flips, "entries": entries, "max_dscore": worst,
            "norm_min": float(norms.min()) if norms.size else 0.0, "norm_max": float(norms.max()) if norms.size else 0.0}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--all", action="store_true", help="every matcher fixture, printed as a markdown table (nothing is written)")
    args = ap.parse_args()
    if args.all:
        from conftest import golden_names
        print("| fixture | index flips | max \\|d score\\| at equal indices | descriptor norms |\n|---|---|---|---|")
        for name in golden_names():
            r = drift(name)
            print(f"| `{name}` | {r['index_flips']} / {r['entries']} | {r['max_dscore']:.1e} | {r['norm_min']:.2f} – {r['norm_max']:.2f} |", flush=True)
        return
    rec = {name: drift(name) for name in PINNED}
    RECORD.write_text(json.dumps(rec, indent=1, sort_keys=True) + "\n")
    print(json.dumps(rec, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
