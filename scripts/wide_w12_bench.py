"""Step time of the wide decode step on the lossless 12-bit copies of the bf16 expert weights (WP12) against the same step on the
WP16 packs, in one process: the 36-layer synthetic model and prompt of bench.py.

    python scripts/wide_w12_bench.py [--steps 300 --warmup 20 --runs 3 --batches 16,24,32] -> profiles/wide_w12.json

Per batch size two legs of DecodeEngine(w12_wide=True) under UMOE_WIDE_DECODE=1: UMOE_WIDE_W12=0 (the WP16 launches) and the default (the
WP12 launches), `runs` runs each, alternating, through the step graph; a leg's figure is the median of its runs and its spread max - min.
The tokens of every run of both legs must be equal (WP12 holds the bf16 bits).  Per-class times (gate/up and down among them) come from
umoe_engine_profile_step.  `w12_wins`: the WP12 leg beat the WP16 leg by more than the larger of the two spreads -- the rule by which
model.WIDE_W12_DEFAULT is set (at every measured batch, or not at all).  No target: the figures are what they are."""
import argparse
import json
import os
import statistics
import sys
import time

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
    ap.add_argument("--batches", default="16,24,32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_w12.json"))
    a = ap.parse_args()
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    from unimoe_audio_amd.model import DecodeEngine
    args = argparse.Namespace(prompt=a.prompt, steps=a.steps, warmup=a.warmup, no_graph=False, layers=a.layers, codec_channels=0)
    dev = torch.device("cuda:0")
    cfg = bench.make_cfg(args)
    model, _ = bench.build_model(cfg, dev)
    t0 = time.perf_counter()
    packable = sum(l is not None for l in model.packed_w12())
    torch.cuda.synchronize()
    os.environ["UMOE_WIDE_DECODE"] = "1"          # the wide form at every size
    K, W, T = a.steps, a.warmup, a.prompt
    res = {"steps": K, "warmup": W, "runs": a.runs, "prompt": T, "layers": cfg.num_hidden_layers, "layers_packable": packable,
           "pack_s": time.perf_counter() - t0, "batches": {}}

    def leg(B, fmt):
        if fmt == "wp16":
            os.environ["UMOE_WIDE_W12"] = "0"     # read per enqueue: the step graph captures the choice
        else:
            os.environ.pop("UMOE_WIDE_W12", None)
        eng = DecodeEngine(model, B, Lmax=T + K + W + 80, Tmax=K + W + 72, expert_weights="bf16", w12_wide=True)
        ids, am, codec = bench.synth_prompt(cfg, B, T, dev, 0)
        eng.prefill(model.calculate_input_embedding(ids, codec).reshape(-1, cfg.hidden_size).contiguous(), am)
        pre, psteps = prepare_audio_prompt(cfg, [None] * B)
        eng.start_decode(pre, psteps, K + W + 64, K + W + 64, cfg_scale=3.0, temperature=1.2, top_p=0.95, top_k=45, eos_mul=0.8, do_sample=True,
                         seed=1234)
        for _ in range(W):
            eng.step(True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(K):
            eng.step(True)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out = dict(ms=1e3 * dt / K, tokens=eng.tokens[:, : K + W + 2].cpu().clone(), prof=eng.profile_steps(4), expert_launch=eng.info("expert_launch"),
                   expert_w12=eng.info("expert_w12"), row_tiles=eng.info("row_tiles"))
        if eng.handoff_error():
            raise SystemExit("wide_w12_bench: an in-launch hand-off timed out")
        eng.close()
        torch.cuda.empty_cache()
        os.environ.pop("UMOE_WIDE_W12", None)
        return out

    for B in [int(v) for v in a.batches.split(",")]:
        legs = {"wp16": [], "wp12": []}
        for _ in range(a.runs):
            for fmt in legs:
                legs[fmt].append(leg(B, fmt))
        first = legs["wp16"][0]["tokens"]
        entry = {}
        for fmt, runs in legs.items():
            for r in runs:
                assert torch.equal(r["tokens"], first), (B, fmt, "tokens differ between the legs or between two runs of a leg")
                assert r["expert_launch"] == 4 and r["expert_w12"] == (fmt == "wp12"), (B, fmt, r["expert_launch"], r["expert_w12"])
            ms = [r["ms"] for r in runs]
            med = statistics.median(ms)
            entry[fmt] = {"ms_per_step": med, "ms_runs": ms, "spread_ms": max(ms) - min(ms), "audio_tokens_per_s": B * 1e3 / med,
                          "row_tiles": runs[-1]["row_tiles"],
                          "per_class": {k: {"ms_per_launch": v[0], "launches": v[1]} for k, v in runs[-1]["prof"].items()}}
        spread = max(entry["wp16"]["spread_ms"], entry["wp12"]["spread_ms"])
        entry["wp12_over_wp16"] = entry["wp12"]["ms_per_step"] / entry["wp16"]["ms_per_step"]
        entry["w12_wins"] = entry["wp16"]["ms_per_step"] - entry["wp12"]["ms_per_step"] > spread
        res["batches"][str(B)] = entry
        print(B, {k: (round(v["ms_per_step"], 4), round(v["spread_ms"], 4), round(v["audio_tokens_per_s"])) for k, v in entry.items() if isinstance(v, dict)},
              {k: {c: round(1e3 * v["per_class"][c]["ms_per_launch"], 1) for c in v["per_class"] if c in ("gateup", "down", "gate_up")}
               for k, v in entry.items() if isinstance(v, dict)}, round(entry["wp12_over_wp16"], 4), entry["w12_wins"], flush=True)
    res["default_on"] = all(e["w12_wins"] for e in res["batches"].values())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
