"""fp8-only expert weights on the 36-layer synthetic model of bench.py, one process:

    python scripts/fp8_only_bench.py [--runs 5 --layers 0] -> profiles/fp8_only.json

  * expert bytes resident in the three modes (bf16, fp8 that kept bf16, fp8-only), counted from the tensors an engine of that mode reads or
    the model holds: parameters, WP16 packs, WP8 blocks + exponents;
  * prefill of 16 rows x 300 tokens (batch 8): the bf16 tiled path (umoe_tiled_gemm, the ping-pong kernel at this size) against the fp8-only engine
    (umoe_tiled_gemm_wp8, 256-token tiles with register staging);
  * an admission prefill of 2 x 64 rows into a serving batch, both ways (bf16 experts: MOE_TILED on W_deq at 128 rows);
  * a serving-style run: 8 rows decoding through the step graph with an admission every 20 steps, both ways;
  * the short-prefill figures of tests/test_gpu_fp8_prefill.py (2 layers at the reference width): fp8-only MOE_TILED against fp8 MOE_RAGGED
    at B = 1, and the bf16 tiled-against-ragged yardstick at B = 3.
Both legs of every comparison alternate, `runs` runs each; a figure is the median and its spread max - min.  Both engines sit on the SAME
quantized model (the fp8-only engine gets no bf16 expert pointer), so their outputs can be compared.  No target: the figures are what they are."""
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


def med(xs):
    return {"median_s": statistics.median(xs), "spread_s": max(xs) - min(xs), "runs_s": xs}


def expert_bytes(model):
    from unimoe_audio_amd import quant
    par = wp16 = wp8 = 0
    pk = model.packed()
    for li, layer in enumerate(model.language_model.layers):
        routed, shared = quant.expert_modules(layer)
        for m in routed + shared:
            par += sum(p.numel() * p.element_size() for p in m.parameters())
            wp8 += sum(t.numel() * t.element_size() for k in ("gu", "dn") for t in m._fp8[k])
        moe = pk["layers"][li]["moe"]
        wp16 += sum(t.numel() * t.element_size() for k in ("exp_gu", "exp_dn", "sh_gu", "sh_dn") for t in moe[k])
    return {"bf16": par + wp16, "fp8_kept_bf16": par + wp16 + wp8, "fp8_only": wp8, "parameters": par, "wp16_packs": wp16, "wp8_blocks": wp8}


def short_prefill(dev):
    """the two relative-L2 figures of the short-prefill test, on its 2-layer model and prompts"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_fp8_prefill as T
    cfg = T.ref_cfg()
    m = T.build(cfg, 31).to(dev)
    m.quantize_experts_("fp8")
    a = T.run_engine(m, cfg, 1, "fp8", 1, False, dev)
    b = T.run_engine(m, cfg, 1, "fp8-only", 1, False, dev)
    os.environ["UMOE_TILED_PREFILL"] = "1"
    y1 = T.run_engine(m, cfg, 3, "bf16", 1, False, dev)
    os.environ["UMOE_TILED_PREFILL"] = "0"
    y0 = T.run_engine(m, cfg, 3, "bf16", 1, False, dev)
    del os.environ["UMOE_TILED_PREFILL"]
    out = {"fp8only_vs_fp8_rel_l2_B1": T.rel_l2(b["logits0"], a["logits0"]), "yardstick_bf16_tiled_vs_ragged_rel_l2_B3": T.rel_l2(y1["logits0"], y0["logits0"]),
           "masks_equal_fp8": bool(torch.equal(a["mask0"], b["mask0"])), "masks_equal_yardstick": bool(torch.equal(y1["mask0"], y0["mask0"]))}
    del m
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--prompt", type=int, default=300)
    ap.add_argument("--batch", type=int, default=8)       # 16 CFG rows x 300 tokens = 4 800 rows, the prefill of bench.py
    ap.add_argument("--serve-steps", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp8_only.json"))
    a = ap.parse_args()
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    from unimoe_audio_amd.model import DecodeEngine
    dev = torch.device("cuda:0")
    res = {"runs": a.runs, "short_prefill": short_prefill(dev)}
    print("short prefill", res["short_prefill"], flush=True)
    args = argparse.Namespace(prompt=a.prompt, steps=8, warmup=2, no_graph=False, layers=a.layers, codec_channels=0)
    cfg = bench.make_cfg(args)
    model, _ = bench.build_model(cfg, dev)
    model.quantize_experts_("fp8")
    torch.cuda.synchronize()
    res["layers"] = cfg.num_hidden_layers
    res["expert_bytes"] = expert_bytes(model)
    print("expert bytes", res["expert_bytes"], flush=True)
    MODES = ("fp8", "fp8-only")          # "fp8" on this model: bf16 expert weights W_deq on every prefill path, as the parent runs them

    # ---- prefill of batch x prompt tokens
    B, T = a.batch, a.prompt
    ids, am, codec = bench.synth_prompt(cfg, B, T, dev, 0)
    x = model.calculate_input_embedding(ids, codec).reshape(-1, cfg.hidden_size).contiguous()
    times = {m: [] for m in MODES}
    hidden = {}
    for mode in MODES:
        eng = DecodeEngine(model, B, Lmax=T + 96, Tmax=80, expert_weights=mode, fp8_wide=True)
        eng.prefill(x, am)                               # warm-up: workspace, first-launch costs
        torch.cuda.synchronize()
        hidden[mode] = eng
    for _ in range(a.runs):
        for mode in MODES:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hidden[mode].prefill(x, am)
            torch.cuda.synchronize()
            times[mode].append(time.perf_counter() - t0)
    k = {m: hidden[m].copy_buffer("k_cache", torch.bfloat16, (cfg.num_hidden_layers, 2 * B, cfg.num_key_value_heads, hidden[m].Lmax, cfg.head_dim))[:, :, :, :T]
         for m in MODES}
    res["prefill"] = {"rows": 2 * B * T, "bf16_tiled": med(times["fp8"]), "fp8_only": med(times["fp8-only"]),
                      "prefill_fp8": {m: hidden[m].info("prefill_fp8") for m in MODES},
                      "k_cache_rel_l2": float((k["fp8-only"].float() - k["fp8"].float()).norm() / k["fp8"].float().norm())}
    res["prefill"]["fp8_only_over_bf16"] = res["prefill"]["fp8_only"]["median_s"] / res["prefill"]["bf16_tiled"]["median_s"]
    print("prefill", {m: (round(1e3 * statistics.median(v), 2), round(1e3 * (max(v) - min(v)), 2)) for m, v in times.items()},
          round(res["prefill"]["fp8_only_over_bf16"], 3), flush=True)
    for e in hidden.values():
        e.close()
    del hidden, k
    torch.cuda.empty_cache()

    # ---- admission prefill of 2 x 64 rows, and a serving-style run with admissions
    SLOTS, TA = 8, 64
    ids, am, codec = bench.synth_prompt(cfg, 1, TA, dev, 1)
    xa = model.calculate_input_embedding(ids, codec).reshape(-1, cfg.hidden_size).contiguous()
    pre, ps = prepare_audio_prompt(cfg, [None])
    kw = dict(cfg_scale=3.0, temperature=1.2, top_p=0.95, top_k=45, eos_mul=0.8, do_sample=True, seed=7, min_tokens=10 ** 6, max_tokens=a.serve_steps + 60)
    engs = {}
    for mode in MODES:
        eng = DecodeEngine(model, SLOTS, Lmax=TA + a.serve_steps + 160, Tmax=a.serve_steps + 136, expert_weights=mode, fp8_wide=True)
        eng.start_serving(TA)
        eng.admit(0, xa, am.cpu(), pre[0], ps[0], **kw)      # warm-up
        torch.cuda.synchronize()
        engs[mode] = eng
    adm = {m: [] for m in MODES}
    for r in range(a.runs):
        for mode in MODES:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            engs[mode].admit(1 + r % (SLOTS - 1), xa, am.cpu(), pre[0], ps[0], **kw)
            torch.cuda.synchronize()
            adm[mode].append(time.perf_counter() - t0)
    res["admission_prefill"] = {"rows": 2 * TA, "bf16": med(adm["fp8"]), "fp8_only": med(adm["fp8-only"]),
                                "prefill_fp8": {m: engs[m].info("prefill_fp8") for m in MODES}}
    res["admission_prefill"]["fp8_only_over_bf16"] = res["admission_prefill"]["fp8_only"]["median_s"] / res["admission_prefill"]["bf16"]["median_s"]
    print("admission", {m: (round(1e3 * statistics.median(v), 3), round(1e3 * (max(v) - min(v)), 3)) for m, v in adm.items()},
          round(res["admission_prefill"]["fp8_only_over_bf16"], 3), flush=True)
    for e in engs.values():
        e.close()
    torch.cuda.empty_cache()

    def serve(mode):
        eng = DecodeEngine(model, SLOTS, Lmax=TA + a.serve_steps + 160, Tmax=a.serve_steps + 136, expert_weights=mode, fp8_wide=True)
        eng.start_serving(TA)
        for b in range(SLOTS):
            eng.admit(b, xa, am.cpu(), pre[0], ps[0], **dict(kw, seed=7 + b))
        for _ in range(5):
            eng.step(True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n_adm = 0
        for s in range(a.serve_steps):
            if s % 20 == 10:                                 # a request ends and the next one takes its row
                eng.admit(n_adm % SLOTS, xa, am.cpu(), pre[0], ps[0], **dict(kw, seed=100 + n_adm))
                n_adm += 1
            eng.step(True)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        tok = eng.tokens.cpu().clone()
        eng.close()
        torch.cuda.empty_cache()
        return dt, n_adm, tok

    sv = {m: [] for m in MODES}
    toks = {}
    for _ in range(max(3, a.runs // 2)):
        for mode in MODES:
            dt, n_adm, tok = serve(mode)
            sv[mode].append(dt)
            toks[mode] = tok
    res["serving"] = {"slots": SLOTS, "steps": a.serve_steps, "admissions": n_adm, "prompt_rows": 2 * TA, "bf16": med(sv["fp8"]), "fp8_only": med(sv["fp8-only"]),
                      "tokens_equal": bool(torch.equal(toks["fp8"], toks["fp8-only"]))}
    res["serving"]["fp8_only_over_bf16"] = res["serving"]["fp8_only"]["median_s"] / res["serving"]["bf16"]["median_s"]
    print("serving", {m: (round(statistics.median(v), 4), round(max(v) - min(v), 4)) for m, v in sv.items()}, round(res["serving"]["fp8_only_over_bf16"], 4),
          res["serving"]["tokens_equal"], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
