"""Cost of admission into a decoding batch (per-row clocks) on bench.py's model, prompt and settings; writes
profiles/serve_bench.json and prints it as one JSON line.

  step time     the flagship decode on the one clock against the same batch on a zero-offset clock table (all rows live), alternating
                legs in one process; the tokens of the two must be the same, which is checked
  parked rows   step time with 4 of 8 rows parked against 8 live rows at the same context length, with the KV bytes a parked row no
                longer reads (1 KiB per cached token per row per layer, bench.py's figure)
  mixed queue   a queue of fixed-length requests (min_tokens = max_tokens) served through unimoe_audio_amd.serve.Scheduler against
                lockstep waves of 8 (DecodeEngine.run with per-row lengths).  ASSERTED: the step counts only -- waves cost the sum of the
                per-wave maxima, serving the greedy makespan.  Wall times and the admission cost per request are recorded.

    python scripts/serve_bench.py --steps 300 --warmup 20 --runs 3"""
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

SET = dict(cfg_scale=3.0, temperature=1.2, top_p=0.95, top_k=45, eos_mul=0.8, do_sample=True, seed=1234)


def timed_steps(eng, W, K):
    for _ in range(W):
        eng.step(True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(K):
        eng.step(True)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / K * 1e3


def clock_leg(model, cfg, a, device, clock):
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    from unimoe_audio_amd.model import DecodeEngine
    B, T, K, W = a.batch, a.prompt, a.steps, a.warmup
    max_tokens = K + W + 64
    eng = DecodeEngine(model, B, Lmax=T + max_tokens + 8, Tmax=max_tokens + 64)
    ids, am, codec = bench.synth_prompt(cfg, B, T, device)
    eng.prefill(model.calculate_input_embedding(ids, codec).reshape(-1, cfg.hidden_size).contiguous(), am)
    pre, psteps = prepare_audio_prompt(cfg, [None] * B)
    eng.start_decode(pre, psteps, max_tokens, max_tokens, **SET)
    if clock:
        eng.use_row_clock()
    ms = timed_steps(eng, W, K)
    tokens = eng.tokens[:, : K + W + 2].cpu().clone()
    assert eng.handoff_error() == 0
    eng.close()
    return ms, tokens


def pair_inputs(model, cfg, a, device):
    """one CFG pair of bench.py's prompt: embeddings [2T, D], mask [2, T]"""
    ids, am, codec = bench.synth_prompt(cfg, 1, a.prompt, device)
    return model.calculate_input_embedding(ids, codec).reshape(-1, cfg.hidden_size).contiguous(), am


def parked_leg(model, cfg, a, device, live):
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    from unimoe_audio_amd.model import DecodeEngine
    B, T, K, W = a.batch, a.prompt, a.steps, a.warmup
    max_tokens = K + W + 64
    eng = DecodeEngine(model, B, Lmax=T + max_tokens + 8, Tmax=max_tokens + 64)
    eng.start_serving(T)
    x, am = pair_inputs(model, cfg, a, device)
    pre, ps = prepare_audio_prompt(cfg, [None])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for b in range(live):
        eng.admit(b, x, am, pre[0], ps[0], max_tokens=max_tokens, min_tokens=max_tokens, **SET)
    torch.cuda.synchronize()
    admit_ms = (time.perf_counter() - t0) / live * 1e3
    ms = timed_steps(eng, W, K)
    assert eng.handoff_error() == 0
    eng.close()
    return ms, admit_ms


def queue_legs(model, cfg, a, device):
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    from unimoe_audio_amd.model import DecodeEngine
    from unimoe_audio_amd.serve import Scheduler, makespan_steps
    B, T = a.batch, a.prompt
    md = max(cfg.codec_delay_pattern)
    lengths = [int(v) for v in a.queue.split(",")]                 # max_tokens = min_tokens of each request
    top = max(lengths)
    x, am = pair_inputs(model, cfg, a, device)
    pre1, ps1 = prepare_audio_prompt(cfg, [None])
    steps_of = lambda n: n - 1                                     # noqa: E731  forced ending at cur = n - md, md steps of countdown, from cur = 1
    # ---- waves of B: lockstep, each wave as long as its longest row
    ids, amB, codec = bench.synth_prompt(cfg, B, T, device)
    xB = model.calculate_input_embedding(ids, codec).reshape(-1, cfg.hidden_size).contiguous()
    preB, psB = prepare_audio_prompt(cfg, [None] * B)
    eng = DecodeEngine(model, B, Lmax=T + top + 8, Tmax=top + 64)
    wave_steps, wave_expect = 0, 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for w in range(0, len(lengths), B):
        wave = lengths[w:w + B]
        wave = wave + [wave[-1]] * (B - len(wave))
        eng.prefill(xB, amB)
        kw = {k: [v] * B for k, v in SET.items()}
        eng.start_decode(preB, psB, wave, wave, **kw)
        wave_steps += eng.run(use_graph=True, poll_every=a.poll_every)        # polls like the served leg; never beyond the longest row's bound
        wave_expect += min(-(-steps_of(max(wave)) // a.poll_every) * a.poll_every, max(wave))
    torch.cuda.synchronize()
    waves_s = time.perf_counter() - t0
    eng.close()
    assert wave_steps == wave_expect, (wave_steps, wave_expect)
    # ---- served: a row takes the next request as soon as it is free
    eng = DecodeEngine(model, B, Lmax=T + top + 8, Tmax=top + 64)
    eng.start_serving(T)
    admit_s = []

    class Rows:
        def admit(self, row, n):
            torch.cuda.synchronize()
            t = time.perf_counter()
            eng.admit(row, x, am, pre1[0], ps1[0], max_tokens=n, min_tokens=n, **SET)
            torch.cuda.synchronize()
            admit_s.append(time.perf_counter() - t)

        def steps(self, n):
            for _ in range(n):
                eng.step(True)

        poll = staticmethod(lambda: eng.poll())
        row_done = staticmethod(lambda st, row: eng.row_done(st, row))

        def take(self, row):
            codes, length = eng.take(row)
            return length

    sched = Scheduler(Rows(), B, a.poll_every)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = dict(sched.run(lengths))
    torch.cuda.synchronize()
    served_s = time.perf_counter() - t0
    eng.close()
    assert [got[i] for i in range(len(lengths))] == [n - md - ps1[0] for n in lengths], got
    expect = makespan_steps([steps_of(n) for n in lengths], B, a.poll_every)
    assert sched.steps_run == expect, (sched.steps_run, expect)
    return dict(queue_max_tokens=lengths, poll_every=a.poll_every, wave_steps=wave_steps, served_steps=sched.steps_run, waves_wall_s=round(waves_s, 3),
                served_wall_s=round(served_s, 3), admit_ms_per_request=round(statistics.mean(admit_s) * 1e3, 3),
                admit_ms_max=round(max(admit_s) * 1e3, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--prompt", type=int, default=300)
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--codec-channels", type=int, default=0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--poll-every", type=int, default=16)
    ap.add_argument("--queue", default="1000,150,150,150,150,150,150,150,1000,150,150,150,150,150,150,150,150,150,150,150,150,150,150,150")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "serve_bench.json"))
    a = ap.parse_args()
    device = torch.device("cuda:0")
    cfg = bench.make_cfg(a)
    model, _ = bench.build_model(cfg, device)
    ms = {"scalar": [], "clock": [], "live8": [], "live4": []}
    admit = []
    ref = None
    for _ in range(a.runs):
        for name, clock in (("scalar", False), ("clock", True)):
            t, tok = clock_leg(model, cfg, a, device, clock)
            ms[name].append(round(t, 4))
            ref = tok if ref is None else ref
            assert torch.equal(tok, ref), f"{name}: the tokens differ from the first leg's"
        for name, live in (("live8", a.batch), ("live4", a.batch // 2)):
            t, adm = parked_leg(model, cfg, a, device, live)
            ms[name].append(round(t, 4))
            admit.append(adm)
    med = {k: statistics.median(v) for k, v in ms.items()}
    ctx = a.prompt + a.warmup + a.steps / 2                        # mean cached tokens per row over the timed steps
    out = {"metric": "ms_per_step: one clock vs per-row clocks; 8 live rows vs 4 live + 4 parked; a mixed queue served vs in waves",
           "batch": a.batch, "prompt": a.prompt, "steps": a.steps, "warmup": a.warmup, "layers": cfg.num_hidden_layers,
           "scalar_ms_per_step": ms["scalar"], "clock_ms_per_step": ms["clock"], "scalar_median": med["scalar"], "clock_median": med["clock"],
           "tokens_identical": True,
           "live8_ms_per_step": ms["live8"], "live4_parked4_ms_per_step": ms["live4"], "live8_median": med["live8"], "live4_parked4_median": med["live4"],
           "parked_kv_bytes_saved_per_step": int((a.batch // 2) * 2 * ctx * 1024 * cfg.num_hidden_layers),
           "admit_ms_per_request_prompt": round(statistics.median(admit), 3),
           "queue": queue_legs(model, cfg, a, device), "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
