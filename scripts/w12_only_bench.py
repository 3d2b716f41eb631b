"""w12-only expert weights on the 36-layer synthetic model of bench.py, one process:

    python scripts/w12_only_bench.py [--runs 5 --layers 0] -> profiles/w12_only.json

The default bf16 engine against the w12-only engine on the SAME weights (two models from one seed: one keeps its parameters, the other is
released to its WP12 copies):
  * expert bytes resident, from torch.cuda.memory_allocated() differences around model construction, release and engine construction,
    next to the sums of the tensors (parameters, WP16 packs, WP12 copies);
  * the prefill of 16 rows x 300 tokens (batch 8): umoe_tiled_gemm (the ping-pong kernel at this size) against umoe_tiled_gemm_w12 (256-token
    tiles with register staging);
  * an admission prefill of 2 x 64 rows into a serving batch;
  * a serving-style run: 8 rows decoding through the step graph for 100 steps with 5 admissions;
  * decode ms/step at batch 8 (the flat launch) and 16 (the wide form): the same kernels on the same WP12 copies in both legs, so equality
    inside the spread is the expectation.
Both legs of every comparison alternate, `runs` runs each; a figure is the median and its spread max - min.  The tokens of both legs must
be equal.  The yardstick of every row is the bf16 leg of the same run, never a fixed number."""
import argparse
import gc
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402

MODES = ("bf16", "w12-only")


def med(xs):
    return {"median_s": statistics.median(xs), "spread_s": max(xs) - min(xs), "runs_s": xs}


def allocated():
    gc.collect()
    torch.cuda.synchronize()
    return torch.cuda.memory_allocated()


def requested():
    return int(torch.cuda.memory_stats().get("requested_bytes.all.current", -1))


def nbytes(ts):
    return sum(t.numel() * t.element_size() for t in ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--prompt", type=int, default=300)
    ap.add_argument("--batch", type=int, default=8)       # 16 CFG rows x 300 tokens = 4 800 rows, the prefill of bench.py
    ap.add_argument("--serve-steps", type=int, default=100)
    ap.add_argument("--decode-steps", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "w12_only.json"))
    a = ap.parse_args()
    from unimoe_audio_amd import quant
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    from unimoe_audio_amd.model import DecodeEngine
    dev = torch.device("cuda:0")
    args = argparse.Namespace(prompt=a.prompt, steps=8, warmup=2, no_graph=False, layers=a.layers, codec_channels=0)
    cfg = bench.make_cfg(args)
    res = {"runs": a.runs, "layers": cfg.num_hidden_layers}

    # ---- the two models and what they hold
    m0 = allocated()
    model_bf, _ = bench.build_model(cfg, dev)
    m1 = allocated()
    par = sum(nbytes(x.parameters()) for layer in model_bf.language_model.layers for grp in quant.expert_modules(layer) for x in grp)
    eng = DecodeEngine(model_bf, a.batch, Lmax=a.prompt + 96, Tmax=80, expert_weights="bf16")      # packs WP16 and (16 rows: the flat launch) WP12
    m2 = allocated()
    wp16 = sum(nbytes(lp["moe"][k]) for lp in model_bf.packed()["layers"] for k in ("exp_gu", "exp_dn", "sh_gu", "sh_dn"))
    w12_bf = sum(nbytes(t for k in ("gu", "dn") for pr in c[k] for t in pr) for c in model_bf.packed_w12() if c is not None)
    eng.close()
    del eng
    m3 = allocated()
    model_w, _ = bench.build_model(cfg, dev)
    m4 = allocated()
    r4 = requested()
    model_w.quantize_experts_("w12", keep_bf16=False)
    m5 = allocated()
    r5 = requested()
    eng = DecodeEngine(model_w, a.batch, Lmax=a.prompt + 96, Tmax=80)
    assert eng.expert_weights == "w12-only" and eng.info("expert_bf16_resident") == 0 and eng.info("w12_only_layers") == cfg.num_hidden_layers
    m6 = allocated()
    eng.close()
    del eng
    w12_w = sum(nbytes(t for k in ("gu", "dn") for pr in c[k] for t in pr) for c in model_w.packed_w12())
    engine_other = m6 - m5                                  # what an engine allocates that is no expert weight (attention packs, caches, workspace)
    res["expert_bytes"] = {
        "tensors": {"parameters": par, "wp16_packs": wp16, "wp12_copies": w12_w, "wp12_copies_of_the_bf16_model": w12_bf},
        "bf16_engine_measured": par + (m2 - m1) - engine_other,          # parameters + what the engine build added beyond the non-expert part
        "w12_only_engine_measured": par - (m4 - m5),                     # parameters minus what the release gave back
        "w12_only_engine_requested_bytes": par - (r4 - r5),              # the same from the sizes the tensors were asked for (no allocator remainder)
        "model_bf16_allocated": m1 - m0, "model_released_allocated": m5 - m3, "engine_non_expert_allocated": engine_other,
    }
    res["expert_bytes"]["ratio"] = res["expert_bytes"]["w12_only_engine_measured"] / res["expert_bytes"]["bf16_engine_measured"]
    print("expert bytes", json.dumps(res["expert_bytes"]), flush=True)
    models = {"bf16": model_bf, "w12-only": model_w}

    def embed(mode, ids, codec):
        return models[mode].calculate_input_embedding(ids, codec).reshape(-1, cfg.hidden_size).contiguous()

    # ---- prefill of batch x prompt tokens
    B, T = a.batch, a.prompt
    ids, am, codec = bench.synth_prompt(cfg, B, T, dev, 0)
    x = embed("bf16", ids, codec)
    times, engs = {m: [] for m in MODES}, {}
    for mode in MODES:
        engs[mode] = DecodeEngine(models[mode], B, Lmax=T + 96, Tmax=80, expert_weights=mode)
        engs[mode].prefill(x, am)                            # warm-up: workspace, first-launch costs
        torch.cuda.synchronize()
    for _ in range(a.runs):
        for mode in MODES:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            engs[mode].prefill(x, am)
            torch.cuda.synchronize()
            times[mode].append(time.perf_counter() - t0)
    k = {m: engs[m].copy_buffer("k_cache", torch.bfloat16, (cfg.num_hidden_layers, 2 * B, cfg.num_key_value_heads, engs[m].Lmax, cfg.head_dim))[:, :, :, :T]
         for m in MODES}
    res["prefill"] = {"rows": 2 * B * T, "bf16": med(times["bf16"]), "w12_only": med(times["w12-only"]),
                      "prefill_w12": {m: engs[m].info("prefill_w12") for m in MODES},
                      "k_cache_equal": bool(torch.equal(k["bf16"].view(torch.int16), k["w12-only"].view(torch.int16))),
                      "k_cache_rel_l2": float((k["w12-only"].float() - k["bf16"].float()).norm() / k["bf16"].float().norm())}
    res["prefill"]["w12_only_over_bf16"] = res["prefill"]["w12_only"]["median_s"] / res["prefill"]["bf16"]["median_s"]
    print("prefill", {m: (round(1e3 * statistics.median(v), 2), round(1e3 * (max(v) - min(v)), 2)) for m, v in times.items()},
          round(res["prefill"]["w12_only_over_bf16"], 3), res["prefill"]["k_cache_equal"], flush=True)
    for e in engs.values():
        e.close()
    del engs, k
    torch.cuda.empty_cache()

    # ---- admission prefill of 2 x 64 rows, and a serving-style run with admissions
    SLOTS, TA = 8, 64
    ids, am, codec = bench.synth_prompt(cfg, 1, TA, dev, 1)
    xa = embed("bf16", ids, codec)
    pre, ps = prepare_audio_prompt(cfg, [None])
    kw = dict(cfg_scale=3.0, temperature=1.2, top_p=0.95, top_k=45, eos_mul=0.8, do_sample=True, seed=7, min_tokens=10 ** 6, max_tokens=a.serve_steps + 60)
    engs = {}
    for mode in MODES:
        eng = DecodeEngine(models[mode], SLOTS, Lmax=TA + a.serve_steps + 160, Tmax=a.serve_steps + 136, expert_weights=mode)
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
    res["admission_prefill"] = {"rows": 2 * TA, "bf16": med(adm["bf16"]), "w12_only": med(adm["w12-only"]),
                                "prefill_w12": {m: engs[m].info("prefill_w12") for m in MODES}}
    res["admission_prefill"]["w12_only_over_bf16"] = res["admission_prefill"]["w12_only"]["median_s"] / res["admission_prefill"]["bf16"]["median_s"]
    print("admission", {m: (round(1e3 * statistics.median(v), 3), round(1e3 * (max(v) - min(v)), 3)) for m, v in adm.items()},
          round(res["admission_prefill"]["w12_only_over_bf16"], 3), flush=True)
    for e in engs.values():
        e.close()
    del engs
    torch.cuda.empty_cache()

    def serve(mode):
        eng = DecodeEngine(models[mode], SLOTS, Lmax=TA + a.serve_steps + 160, Tmax=a.serve_steps + 136, expert_weights=mode)
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

    sv, toks = {m: [] for m in MODES}, {}
    for _ in range(a.runs):
        for mode in MODES:
            dt, n_adm, tok = serve(mode)
            sv[mode].append(dt)
            toks[mode] = tok
    res["serving"] = {"slots": SLOTS, "steps": a.serve_steps, "admissions": n_adm, "prompt_rows": 2 * TA, "bf16": med(sv["bf16"]), "w12_only": med(sv["w12-only"]),
                      "tokens_equal": bool(torch.equal(toks["bf16"], toks["w12-only"]))}
    res["serving"]["w12_only_over_bf16"] = res["serving"]["w12_only"]["median_s"] / res["serving"]["bf16"]["median_s"]
    print("serving", {m: (round(statistics.median(v), 4), round(max(v) - min(v), 4)) for m, v in sv.items()}, round(res["serving"]["w12_only_over_bf16"], 4),
          res["serving"]["tokens_equal"], flush=True)

    # ---- decode ms/step: the same launches on the same WP12 copies in both legs
    res["decode"] = {}
    for B in (8, 16):
        Td = 32
        ids, am, codec = bench.synth_prompt(cfg, B, Td, dev, 2)
        xd = embed("bf16", ids, codec)
        pre, ps = prepare_audio_prompt(cfg, [None] * B)
        engs, dt, toks = {}, {m: [] for m in MODES}, {}
        n_steps = 8 + a.runs * a.decode_steps
        for mode in MODES:
            eng = DecodeEngine(models[mode], B, Lmax=Td + n_steps + 80, Tmax=n_steps + 72, expert_weights=mode, w12_wide=True)
            eng.prefill(xd, am)
            eng.start_decode(pre, ps, n_steps + 8, 10 ** 6, cfg_scale=3.0, temperature=1.2, top_p=0.95, top_k=45, eos_mul=0.8, do_sample=True, seed=11)
            for _ in range(8):
                eng.step(True)
            torch.cuda.synchronize()
            engs[mode] = eng
        for _ in range(a.runs):
            for mode in MODES:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.decode_steps):
                    engs[mode].step(True)
                torch.cuda.synchronize()
                dt[mode].append((time.perf_counter() - t0) / a.decode_steps)
        for mode in MODES:
            toks[mode] = engs[mode].tokens.cpu().clone()
        res["decode"][f"batch_{B}"] = {"rows": 2 * B, "bf16_s_per_step": med(dt["bf16"]), "w12_only_s_per_step": med(dt["w12-only"]),
                                       "expert_launch": {m: engs[m].info("expert_launch") for m in MODES},
                                       "expert_w12": {m: engs[m].info("expert_w12") for m in MODES},
                                       "tokens_equal": bool(torch.equal(toks["bf16"], toks["w12-only"]))}
        r = res["decode"][f"batch_{B}"]
        r["w12_only_over_bf16"] = r["w12_only_s_per_step"]["median_s"] / r["bf16_s_per_step"]["median_s"]
        print("decode batch", B, {m: (round(1e3 * statistics.median(v), 4), round(1e3 * (max(v) - min(v)), 4)) for m, v in dt.items()},
              round(r["w12_only_over_bf16"], 4), r["tokens_equal"], flush=True)
        for e in engs.values():
            e.close()
        del engs
        torch.cuda.empty_cache()
    res["tokens_equal"] = bool(res["serving"]["tokens_equal"] and all(v["tokens_equal"] for v in res["decode"].values()))
    # (k_cache_equal of the 4 800-row prefill is reported, not required: at that size the bf16 leg runs the 256 x 256 ping-pong kernel, which
    # promises equality with tgemm_kernel only up to summation order)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    assert res["tokens_equal"], "the two legs disagree"


if __name__ == "__main__":
    main()
