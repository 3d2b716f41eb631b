"""FETCH_SIZE passes of scripts/wide_pmc_step.py (wide leg, ragged leg) -> the fetched bytes of ONE decode step per leg, as markdown.

    python scripts/summarize_wide_pmc.py WIDE_DIR RAGGED_DIR STEPS ROWS KV_LEN > profiles/wide_decode_pmc.md

A kernel belongs to the decode steps when its launch count is a multiple of STEPS (5: the prefill's per-layer kernels run 36 or 72 times);
kernels that the prefill and the steps share are listed as left out.  Counters are in KiB and FETCH_SIZE reports half of the bytes of wide
coalesced streaming reads on gfx950 (scripts/summarize_pmc.py): bytes = FETCH_SIZE * 1024 * 2."""
import csv
import glob
import os
import sys
from collections import defaultdict


def load(d):
    acc = defaultdict(lambda: [0, 0.0])
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if r.get("Counter_Name") != "FETCH_SIZE":
                continue
            n = r["Kernel_Name"].replace("void ", "")
            n = n[: n.index("(")] if "(" in n else n[:70]
            acc[n][0] += 1
            acc[n][1] += float(r["Counter_Value"])
    return acc


wide_dir, ragged_dir, steps, rows, kv = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
formula_mb = 36 * (52.75 + 33.82 * 8) + 1024 * kv * rows * 36 / 1e6 + 50.48
print(f"# Fetched bytes of one decode step at {rows} rows (batch {rows // 2}), counters only\n")
print(f"`rocprofv3 --pmc FETCH_SIZE` alone (no tracing in the run), {steps} eager steps behind a {kv - steps}-token prefill, full 36 layers, synthetic bf16 "
      f"weights.  BASELINE section 3 at rows = {rows}, 8 experts hit, L = {kv}: **{formula_mb / 1e3:.2f} GB/step**.\n")
for name, d in (("wide (UMOE_WIDE_DECODE=1)", wide_dir), ("ragged (UMOE_WIDE_DECODE=0)", ragged_dir)):
    acc = load(d)
    step_k = {k: v for k, v in acc.items() if v[0] % steps == 0}
    left = {k: v for k, v in acc.items() if v[0] % steps != 0 and v[0] > 36}
    total = sum(v[1] for v in step_k.values()) * 2048 / steps
    print(f"## {name}: {total / 1e9:.2f} GB/step fetched = {total / 1e6 / formula_mb:.2f} x the formula\n")
    print("| kernel | launches per step | fetch MB per step (x2) |\n|---|---|---|")
    for k, v in sorted(step_k.items(), key=lambda kv_: -kv_[1][1]):
        if v[1] * 2048 / steps / 1e6 >= 1.0:
            print(f"| `{k}` | {v[0] // steps} | {v[1] * 2048 / steps / 1e6:.1f} |")
    if left:
        print("\nshared with the prefill and left out of the sum: " + ", ".join(f"`{k}` ({v[0]} launches)" for k, v in left.items()))
    print()
