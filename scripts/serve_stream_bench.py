"""Streamed serving (UniMoEAudio.serve(stream=True)) on the 36-layer synthetic model of bench.py with a random DAC of the
16 kHz geometry: a queue of music and speech requests of 2 to 6 s (min_audio_seconds = max_audio_seconds: every request runs to its
length), several times the slot count, served three ways that alternate in ONE process, `--runs` times each:

  nonstream   serve(stream=False): each request's wav when it has ended
  ragged      serve(stream=True), the per-row table kernels: one launch per DAC layer for all rows
  grouped     serve(stream=True, stream_ragged=False): the same bookkeeping, one umoe_dac_*_win launch per layer and row with news

at 8 slots (bf16) and 32 slots (fp8 expert weights, the wide step), with poll_every 16 and 25.  Per leg: the makespan (median of the
runs, with the spread max - min), admission -> first chunk per request (median and worst), GPU milliseconds of the DAC work and library
calls per state read, and the makespan over the non-streamed leg's.  The ragged executor is judged against the grouped leg of the same
process.  Writes profiles/serve_stream.json and prints it as one JSON line.

--dac-conv mfma: the codec in conv_form="mfma" (DESIGN 4q).  --dac-conv both: the nonstream and ragged legs in BOTH forms, alternating in
one process (legs nonstream_direct, ragged_direct, nonstream_mfma, ragged_mfma; no grouped leg), and per setting whether the MFMA
form's DAC milliseconds per read beat the direct form's by more than the two spreads added.  Either writes profiles/serve_stream_mfma.json.

    python scripts/serve_stream_bench.py [--slots 8,32] [--polls 16,25] [--runs 3] [--per-slot 3] [--dac-conv direct|mfma|both]
"""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Tokenizer:
    """stands in for the HF tokenizer (an asset that is not in the tree): special tokens and characters hashed to ids, left padding"""

    def __init__(self, placeholder_id):
        self.placeholder_id = placeholder_id

    def __call__(self, texts, add_special_tokens=False, return_tensors="pt", padding=True):
        import re
        import types
        rows = []
        for t in texts:
            ids = []
            for piece in re.split(r"(<\|[A-Za-z_]+\|>)", t):
                if piece == "<|AUDIO_PLACEHOLDER|>":
                    ids.append(self.placeholder_id)
                elif piece.startswith("<|"):
                    ids.append(200 + (sum(map(ord, piece)) % 80))
                else:
                    ids += [1 + (ord(ch) % 190) for ch in piece]
            rows.append(ids)
        T = max(len(r) for r in rows)
        return types.SimpleNamespace(input_ids=torch.tensor([[0] * (T - len(r)) + r for r in rows]),
                                     attention_mask=torch.tensor([[0] * (T - len(r)) + [1] * len(r) for r in rows]))


def queue(n, seed):
    from unimoe_audio_amd.api import MusicRequest, SpeechRequest
    rng = random.Random(seed)
    voice = [[rng.randrange(1024) for _ in range(12)] for _ in range(60)]
    reqs = []
    for i in range(n):
        s = rng.choice([2, 3, 4, 5, 6])
        if i % 2:
            reqs.append(SpeechRequest(f"sentence number {i} of the queue", "the text of the voice prompt", prompt_codec=voice, max_audio_seconds=s,
                                      min_audio_seconds=s, seed=100 + i))
        else:
            reqs.append(MusicRequest(f"a piece of music, number {i}", max_audio_seconds=s, min_audio_seconds=s, seed=100 + i))
    return reqs


def run_leg(app, D, reqs, leg, slots, poll_every):
    """one serving of the queue -> makespan, first-chunk latencies, DAC ms and library calls per read.  leg: nonstream / ragged / grouped,
    or one of them with the codec's form behind it (ragged_mfma)"""
    leg, _, form = leg.partition("_")
    if form:
        app.dac.model.set_conv_form(form)
        app.dac.model._folded()              # (the weights of this form, outside the timed span)
    kw = dict(slots=slots, poll_every=poll_every, max_prompt_tokens=256, max_audio_seconds=6)
    spans, calls, per_read_calls = [], [0], []
    lib_call, push, flush = D._lib_call, D.DacRowStreamDecoder.push, D.DacRowStreamDecoder.flush

    def counted(name, *a):
        calls[0] += 1
        return lib_call(name, *a)

    def timed(fn, kind):
        def run(self, *a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            c0 = calls[0]
            e0.record()
            out = fn(self, *a, **k)
            e1.record()
            spans.append((kind, e0, e1))
            if kind == "push":
                per_read_calls.append(0)
            per_read_calls[-1] += calls[0] - c0
            return out
        return run

    D._lib_call, D.DacRowStreamDecoder.push, D.DacRowStreamDecoder.flush = counted, timed(push, "push"), timed(flush, "flush")
    first = {}
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if leg == "nonstream":
            with tempfile.TemporaryDirectory() as td:
                for _ in app.serve(iter(reqs), output_dir=td, **kw):
                    pass
        else:
            for ch in app.serve(iter(reqs), output_dir=None, stream=True, stream_ragged=leg == "ragged", **kw):
                now = time.perf_counter()
                if ch.row not in first and ch.pcm.numel():
                    first[ch.row] = now
        torch.cuda.synchronize()
        span = time.perf_counter() - t0
    finally:
        D._lib_call, D.DacRowStreamDecoder.push, D.DacRowStreamDecoder.flush = lib_call, push, flush
    out = {"makespan_s": span}
    if leg != "nonstream":
        per_read = []
        for kind, a, b in spans:
            if kind == "push":
                per_read.append(0.0)
            per_read[-1] += a.elapsed_time(b)
        out.update(dac_ms_per_read=statistics.mean(per_read), dac_ms_max_read=max(per_read), dac_s_total=sum(per_read) / 1e3, reads=len(per_read),
                   calls_per_read_min=min(per_read_calls), calls_per_read_max=max(per_read_calls), first_at=first, t0=t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="8,32")
    ap.add_argument("--polls", default="16,25")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--per-slot", type=int, default=3, help="requests in the queue per slot")
    ap.add_argument("--layers", type=int, default=0, help="debug only: override num_hidden_layers (0 = 36)")
    ap.add_argument("--dac-conv", choices=["direct", "mfma", "both"], default="direct")
    ap.add_argument("--out", default=None, help="default: profiles/serve_stream.json, or profiles/serve_stream_mfma.json with --dac-conv mfma / both")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "serve_stream.json" if args.dac_conv == "direct" else "serve_stream_mfma.json")
    both = args.dac_conv == "both"
    legs = ["nonstream_direct", "ragged_direct", "nonstream_mfma", "ragged_mfma"] if both else ["nonstream", "ragged", "grouped"]
    import bench
    from unimoe_audio_amd import dac as D
    from unimoe_audio_amd import serve as S
    from unimoe_audio_amd.api import UniMoEAudio
    from unimoe_audio_amd.config import UniMoEAudioConfig
    dev = torch.device("cuda:0")
    cfg = UniMoEAudioConfig()
    if args.layers:
        cfg.num_hidden_layers = args.layers
    res = {"metric": "serve_stream", "dac": "16kHz random, decoder_dim 1536", "layers": cfg.num_hidden_layers, "runs": args.runs,
           "queue": "music and speech, 2..6 s each (min = max), per_slot x slots requests", "per_slot": args.per_slot, "dac_conv": args.dac_conv,
           "legs": {}}
    # admission times of the streamed legs: Scheduler._admit_free_rows stamps them
    stamps = {}
    admit = S.Scheduler._admit_free_rows

    def stamped(self, source):
        n = len(self.admitted)
        admit(self, source)
        now = time.perf_counter()
        for index, _, _ in self.admitted[n:]:
            stamps[index] = now

    S.Scheduler._admit_free_rows = stamped
    for slots in [int(v) for v in args.slots.split(",")]:
        model, _ = bench.build_model(cfg, dev)
        fmt = "fp8" if slots > 8 else "bf16"
        if fmt == "fp8":
            model.quantize_experts_("fp8")
        app = UniMoEAudio(None, 0, model=model)
        app._tokenizer = Tokenizer(cfg.codec_placeholder_value)
        app.dac = D.Dac(model=D.DacModel(**D.DAC_16KHZ).init_random(0).to(dev).float(), conv_form="direct" if both else args.dac_conv)
        reqs = queue(args.per_slot * slots, slots)
        for poll_every in [int(v) for v in args.polls.split(",")]:
            key = f"slots{slots}_{fmt}_poll{poll_every}"
            # warm-up: the engine, the graph capture, DAC weight folding and every kernel once per leg, on a short queue
            for leg in legs:
                run_leg(app, D, reqs[:slots + 1], leg, slots, poll_every)
            runs = {leg: [] for leg in legs}
            for _ in range(args.runs):
                for leg in runs:
                    stamps.clear()
                    r = run_leg(app, D, reqs, leg, slots, poll_every)
                    if not leg.startswith("nonstream"):
                        lat = [r["first_at"][i] - stamps[i] for i in sorted(r["first_at"])]
                        r.update(first_chunk_median_s=statistics.median(lat), first_chunk_worst_s=max(lat))
                        del r["first_at"], r["t0"]
                    runs[leg].append(r)
            out = {}
            for leg, rs in runs.items():
                spans = [r["makespan_s"] for r in rs]
                out[leg] = {"makespan_s": round(statistics.median(spans), 4), "makespan_spread_s": round(max(spans) - min(spans), 4)}
                for k in rs[0]:
                    if k != "makespan_s":
                        out[leg][k] = round(statistics.median(r[k] for r in rs), 4)
                if "dac_ms_per_read" in rs[0]:
                    out[leg]["dac_ms_per_read_spread"] = round(max(r["dac_ms_per_read"] for r in rs) - min(r["dac_ms_per_read"] for r in rs), 4)
            for leg in legs:
                if not leg.startswith("nonstream"):
                    base = out["nonstream" + leg.partition("_")[1] + leg.partition("_")[2]]["makespan_s"]
                    out[leg]["makespan_over_nonstream"] = round(out[leg]["makespan_s"] / base, 4)
            if both:
                a, b = out["ragged_direct"], out["ragged_mfma"]
                d = a["dac_ms_per_read"] - b["dac_ms_per_read"]
                out["dac_ms_per_read_direct_over_mfma"] = round(a["dac_ms_per_read"] / b["dac_ms_per_read"], 3)
                out["mfma_beats_direct_by_ms_per_read"] = round(d, 4)
                out["beyond_spreads"] = bool(d > a["dac_ms_per_read_spread"] + b["dac_ms_per_read_spread"])
                out["streamed_makespan_direct_over_mfma"] = round(a["makespan_s"] / b["makespan_s"], 4)
            else:
                d = out["grouped"]["makespan_s"] - out["ragged"]["makespan_s"]
                spread = max(out["grouped"]["makespan_spread_s"], out["ragged"]["makespan_spread_s"])
                out["ragged_beats_grouped_by_s"] = round(d, 4)
                out["beyond_spread"] = bool(d > spread)
            out["requests"] = len(reqs)
            res["legs"][key] = out
            print(key, json.dumps(out), flush=True)
        model._engine.close()
        model._engine = None
        del app, model
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
