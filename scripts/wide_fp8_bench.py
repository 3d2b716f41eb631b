"""Step time of the wide decode step on fp8 expert weights against the bf16 wide step of the same process: the 36-layer synthetic
model of bench.py with its experts quantized once (quantize_experts_: the bf16 leg then streams W_deq, the same bytes per step as the
unquantized model), the prompt of scripts/wide_bench.py.

    python scripts/wide_fp8_bench.py [--steps 300 --warmup 20 --runs 3 --batches 16,24,32] -> profiles/wide_fp8.json

Per batch size both legs (bf16 wide with UMOE_WIDE_DECODE=1, fp8 wide with DecodeEngine(fp8_wide=True)), `runs` runs each, alternating,
through the step graph; a leg's figure is the median of its runs and its spread max - min.  The tokens of every run of both legs must be
equal (q * 2^e is exact in bf16).  Per-class times (gate/up and down among them) come from umoe_engine_profile_step.  No target: the
figures are what they are."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_fp8.json"))
    a = ap.parse_args()
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    from unimoe_audio_amd.model import DecodeEngine
    args = argparse.Namespace(prompt=a.prompt, steps=a.steps, warmup=a.warmup, no_graph=False, layers=a.layers, codec_channels=0)
    dev = torch.device("cuda:0")
    cfg = bench.make_cfg(args)
    model, _ = bench.build_model(cfg, dev)
    model.quantize_experts_("fp8")
    torch.cuda.synchronize()
    os.environ["UMOE_WIDE_DECODE"] = "1"          # the wide form at every size, for the bf16 leg too
    K, W, T = a.steps, a.warmup, a.prompt
    res = {"steps": K, "warmup": W, "runs": a.runs, "prompt": T, "layers": cfg.num_hidden_layers, "batches": {}}

    def leg(B, fmt):
        eng = DecodeEngine(model, B, Lmax=T + K + W + 80, Tmax=K + W + 72, expert_weights=fmt, fp8_wide=fmt == "fp8")
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
                   expert_fp8=eng.info("expert_fp8"), row_tiles=eng.info("row_tiles"))
        if eng.handoff_error():
            raise SystemExit("wide_fp8_bench: an in-launch hand-off timed out")
        eng.close()
        torch.cuda.empty_cache()
        return out

    for B in [int(v) for v in a.batches.split(",")]:
        legs = {"bf16": [], "fp8": []}
        for _ in range(a.runs):
            for fmt in legs:
                legs[fmt].append(leg(B, fmt))
        first = legs["bf16"][0]["tokens"]
        entry = {}
        for fmt, runs in legs.items():
            for r in runs:
                assert torch.equal(r["tokens"], first), (B, fmt, "tokens differ between the legs or between two runs of a leg")
                assert r["expert_launch"] == 4 and r["expert_fp8"] == (fmt == "fp8"), (B, fmt, r["expert_launch"], r["expert_fp8"])
            ms = [r["ms"] for r in runs]
            med = statistics.median(ms)
            entry[fmt] = {"ms_per_step": med, "ms_runs": ms, "spread_ms": max(ms) - min(ms), "audio_tokens_per_s": B * 1e3 / med,
                          "row_tiles": runs[-1]["row_tiles"],
                          "per_class": {k: {"ms_per_launch": v[0], "launches": v[1]} for k, v in runs[-1]["prof"].items()}}
        spread = max(entry["bf16"]["spread_ms"], entry["fp8"]["spread_ms"])
        entry["fp8_over_bf16"] = entry["fp8"]["ms_per_step"] / entry["bf16"]["ms_per_step"]
        entry["fp8_wins"] = entry["bf16"]["ms_per_step"] - entry["fp8"]["ms_per_step"] > spread
        res["batches"][str(B)] = entry
        print(B, {k: (round(v["ms_per_step"], 4), round(v["spread_ms"], 4), round(v["audio_tokens_per_s"])) for k, v in entry.items() if isinstance(v, dict)},
              {k: {c: round(1e3 * v["per_class"][c]["ms_per_launch"], 1) for c in v["per_class"] if c in ("gateup", "down", "gate_up")}
               for k, v in entry.items() if isinstance(v, dict)}, round(entry["fp8_over_bf16"], 4), entry["fp8_wins"], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
