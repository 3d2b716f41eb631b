"""Step time of the wide decode step against the ragged path it replaces, one process, synthetic bf16 weights, the full 36
layers and the prompt of bench.py.

    python scripts/wide_bench.py [--steps 300 --warmup 20 --runs 3 --batches 8,9,12,16,24,32] -> profiles/wide_decode.json

Per batch size above 8: both legs (UMOE_WIDE_DECODE=0, then 1), `runs` runs each, alternating; a leg's figure is the median of
its runs and its spread max - min; the tokens of two runs of the same leg must be equal.  A size where the wide leg does not beat the ragged
leg by more than the larger spread is reported with "wide_wins": false.  Per-class times come from umoe_engine_profile_step."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--prompt", type=int, default=300)
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--batches", default="8,9,12,16,24,32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_decode.json"))
    a = ap.parse_args()
    args = argparse.Namespace(prompt=a.prompt, steps=a.steps, warmup=a.warmup, no_graph=False, layers=a.layers, codec_channels=0)
    dev = torch.device("cuda:0")
    cfg = bench.make_cfg(args)
    model, _ = bench.build_model(cfg, dev)
    res = {"steps": a.steps, "warmup": a.warmup, "runs": a.runs, "prompt": a.prompt, "layers": cfg.num_hidden_layers, "batches": {}}

    def leg(B, wide):
        os.environ["UMOE_WIDE_DECODE"] = "1" if wide else "0"      # (1: the wide form whatever the measured default of the size is)
        info = bench.decode_leg(model, cfg, args, dev, 0, B, profile=True)
        os.environ.pop("UMOE_WIDE_DECODE", None)
        return info

    for B in [int(v) for v in a.batches.split(",")]:
        legs = {"wide": []} if B <= 8 else {"ragged": [], "wide": []}
        for _ in range(a.runs):
            for name in legs:
                legs[name].append(leg(B, name == "wide"))
        entry = {}
        for name, runs in legs.items():
            for r in runs[1:]:
                assert torch.equal(r["tokens"], runs[0]["tokens"]), (B, name, "tokens differ between two runs of the same leg")
            ms = [1e3 * r["dt"] / r["steps"] for r in runs]
            med = statistics.median(ms)
            entry[name] = {"ms_per_step": med, "ms_runs": ms, "spread_ms": max(ms) - min(ms), "audio_tokens_per_s": B * 1e3 / med,
                           "expert_launch": runs[-1]["expert_launch"],
                           "per_class": {k: {"ms_per_launch": v[0], "launches": v[1]} for k, v in runs[-1]["prof"].items()}}
        if B > 8:
            spread = max(entry["wide"]["spread_ms"], entry["ragged"]["spread_ms"])
            entry["wide_wins"] = entry["ragged"]["ms_per_step"] - entry["wide"]["ms_per_step"] > spread
        res["batches"][str(B)] = entry
        print(B, {k: (round(v["ms_per_step"], 4), round(v["spread_ms"], 4), round(v["audio_tokens_per_s"])) for k, v in entry.items() if isinstance(v, dict)},
              entry.get("wide_wins"), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
