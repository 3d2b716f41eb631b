"""Step time of the flagship decode (bench.py's model, prompt and settings) with scalar sampling settings against a per-request
table whose rows all carry those settings (umoe_row_params): alternating legs in one process, one JSON line.
The tokens of the two must be the same, which is checked.

    python scripts/row_params_bench.py --steps 300 --warmup 20 --runs 3"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def leg(model, cfg, a, device, table):
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    from unimoe_audio_amd.model import DecodeEngine
    B, T, K, W = a.batch, a.prompt, a.steps, a.warmup
    max_tokens = K + W + 64
    eng = DecodeEngine(model, B, Lmax=T + max_tokens + 8, Tmax=max_tokens + 64)
    ids, am, codec = bench.synth_prompt(cfg, B, T, device)
    eng.prefill(model.calculate_input_embedding(ids, codec).reshape(-1, cfg.hidden_size).contiguous(), am)
    pre, psteps = prepare_audio_prompt(cfg, [None] * B)
    rows = (lambda v: [v] * B) if table else (lambda v: v)
    eng.start_decode(pre, psteps, rows(max_tokens), rows(max_tokens), cfg_scale=rows(3.0), temperature=rows(1.2), top_p=rows(0.95),
                     top_k=rows(45), eos_mul=rows(0.8), do_sample=rows(True), seed=rows(1234))
    assert (eng.io.row_params is not None) == table
    for _ in range(W):
        eng.step(True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(K):
        eng.step(True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    tokens = eng.tokens[:, : K + W + 2].cpu().clone()
    assert eng.handoff_error() == 0
    eng.close()
    return dt / K * 1e3, tokens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--prompt", type=int, default=300)
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--codec-channels", type=int, default=0)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    device = torch.device("cuda:0")
    cfg = bench.make_cfg(a)
    model, _ = bench.build_model(cfg, device)
    ms = {"scalars": [], "table": []}
    ref = None
    for _ in range(a.runs):
        for name, table in (("scalars", False), ("table", True)):
            t, tok = leg(model, cfg, a, device, table)
            ms[name].append(round(t, 4))
            if ref is None:
                ref = tok
            assert torch.equal(tok, ref), f"{name}: the tokens differ from the first leg's"
    print(json.dumps({"metric": "ms_per_step, scalar settings vs a table of equal rows", "batch": a.batch, "steps": a.steps, "warmup": a.warmup,
                      "scalars_ms_per_step": ms["scalars"], "table_ms_per_step": ms["table"],
                      "scalars_median": statistics.median(ms["scalars"]), "table_median": statistics.median(ms["table"]),
                      "tokens_identical": True, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
