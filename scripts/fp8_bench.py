"""A/B of the bf16 and fp8 expert weights of the decode engine in one process: the 36-layer synthetic model of bench.py, quantized
once (the bf16 engine then runs on W_deq -- the same bytes per step as the unquantized model), batch 8 and batch 1, N graph replays
each (--eager: eager steps instead of graph replays -- the host cost of a step shows there).  Prints one JSON line per leg.

  python scripts/fp8_bench.py [--steps 300] [--warmup 20] [--batches 8,1] [--fmts bf16,fp8] [--eager]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batches", default="8,1")
    ap.add_argument("--fmts", default="bf16,fp8")
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--eager", action="store_true")
    args = ap.parse_args()
    import bench
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    from unimoe_audio_amd.config import UniMoEAudioConfig
    from unimoe_audio_amd.model import DecodeEngine
    dev = torch.device("cuda:0")
    cfg = UniMoEAudioConfig()
    model, _ = bench.build_model(cfg, dev)
    model.quantize_experts_("fp8")
    torch.cuda.synchronize()
    for B in [int(b) for b in args.batches.split(",")]:
        for fmt in args.fmts.split(","):
            K, W, T = args.steps, args.warmup, args.prompt
            eng = DecodeEngine(model, B, Lmax=T + K + W + 80, Tmax=K + W + 72, expert_weights=fmt)
            ids, am, codec = bench.synth_prompt(cfg, B, T, dev)
            eng.prefill(model.calculate_input_embedding(ids, codec).reshape(-1, cfg.hidden_size).contiguous(), am)
            pre, psteps = prepare_audio_prompt(cfg, [None] * B)
            eng.start_decode(pre, psteps, K + W + 64, K + W + 64, cfg_scale=3.0, temperature=1.2, top_p=0.95, top_k=45, eos_mul=0.8,
                             do_sample=True, seed=1234)
            for _ in range(W):
                eng.step(not args.eager)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(K):
                eng.step(not args.eager)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            ms = 1e3 * dt / K
            print(json.dumps({"batch": B, "expert_weights": fmt, "steps": K, "graph": not args.eager, "ms_per_step": round(ms, 4),
                              "audio_tokens_per_s": round(B * K / dt, 1), "expert_fp8": eng.info("expert_fp8"),
                              "expert_launch": eng.info("expert_launch"), "handoff_error": eng.handoff_error()}), flush=True)
            if eng.handoff_error():
                raise SystemExit("fp8_bench: an in-launch hand-off timed out")
            eng.close()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
