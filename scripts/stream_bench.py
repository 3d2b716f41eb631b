"""Streaming vs non-streamed generation of one request on the 36-layer synthetic model of bench.py, with a random DAC of the 16 kHz
geometry (decoder_dim 1536): 10 s of audio (500 decode steps; min_audio_seconds = max_audio_seconds, so every row runs to the end),
at batch 8 and batch 1.  Per batch:
  first_chunk_s      request start -> the first AudioChunk in the caller's hands (UniMoEAudio._stream_audio, the streamed task path)
  last_sample_s      request start -> the last chunk of the last row
  nonstream_s        the same request non-streamed: generate_codes, then one Dac.decode per row (UniMoEAudio._finish, wav files included)
  dac_ms_per_chunk   GPU time of the streaming DAC work of one state read (events around push + flush on the decode stream): mean, max
Prints one JSON line.

  python scripts/stream_bench.py [--batches 8,1] [--seconds 10] [--chunk 25] [--prompt 512]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="8,1")
    ap.add_argument("--seconds", type=int, default=10)
    ap.add_argument("--chunk", type=int, default=25)
    ap.add_argument("--prompt", type=int, default=512)
    args = ap.parse_args()
    import bench
    from unimoe_audio_amd import dac as D
    from unimoe_audio_amd.api import UniMoEAudio
    from unimoe_audio_amd.config import UniMoEAudioConfig
    dev = torch.device("cuda:0")
    cfg = UniMoEAudioConfig()
    model, _ = bench.build_model(cfg, dev)
    app = UniMoEAudio(None, 0, model=model)
    app.dac = D.Dac(model=D.DacModel(**D.DAC_16KHZ).init_random(0).to(dev).float())
    # GPU time of the DAC work per state read: events on the decode stream around push() and flush()
    spans = []                     # (kind, start event, end event)
    push, flush = D.DacStreamDecoder.push, D.DacStreamDecoder.flush

    def timed(fn, kind):
        def run(self, *a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(self, *a, **k)
            e1.record()
            spans.append((kind, e0, e1))
            return out
        return run

    D.DacStreamDecoder.push, D.DacStreamDecoder.flush = timed(push, "push"), timed(flush, "flush")
    S = args.seconds
    gen = dict(cfg_scale=3.0, temperature=1.2, top_p=0.95, cfg_filter_top_k=45, eos_prob_mul_factor=0.8, do_sample=True)
    res = {"metric": "stream_latency", "seconds": S, "chunk_frames": args.chunk, "prompt": args.prompt, "dac": "16kHz random, decoder_dim 1536"}
    for B in [int(b) for b in args.batches.split(",")]:
        ids, am, codec = bench.synth_prompt(cfg, B, args.prompt, dev)
        codec_rows = codec.shape[0] // (2 * B)
        # warm-up: engine build (sized for S seconds), DAC weight folding, kernel loading: one streamed and one non-streamed request
        for _ in app._stream_audio(ids, am, codec, S, S, args.chunk, None, "w", **gen):
            pass
        with tempfile.TemporaryDirectory() as td:
            app._finish(app.generate_codes(ids, am, codec, S, S, **gen), td, "w")
        torch.cuda.synchronize()
        spans.clear()
        t0 = time.perf_counter()
        first = last = None
        n_chunks, samples = 0, [0] * B
        for ch in app._stream_audio(ids, am, codec, S, S, args.chunk, None, "s", **gen):
            now = time.perf_counter()
            first = now if first is None else first
            last = now
            n_chunks += 1
            samples[ch.row] += ch.pcm.numel()
        torch.cuda.synchronize()
        per_read = []                  # every state read pushes once; a flush belongs to the read before it
        for kind, a, b in spans:
            if kind == "push":
                per_read.append(0.0)
            per_read[-1] += a.elapsed_time(b)
        with tempfile.TemporaryDirectory() as td:
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            audios = app.generate_codes(ids, am, codec, S, S, **gen)
            t2 = time.perf_counter()
            app._finish(audios, td, "n")
            t3 = time.perf_counter()
        res[f"b{B}"] = {"first_chunk_s": round(first - t0, 4), "last_sample_s": round(last - t0, 4), "nonstream_s": round(t3 - t1, 4),
                        "nonstream_codes_s": round(t2 - t1, 4), "nonstream_dac_s": round(t3 - t2, 4),
                        "last_over_nonstream": round((last - t0) / (t3 - t1), 4), "chunks": n_chunks, "state_reads": len(per_read),
                        "dac_ms_per_chunk": round(sum(per_read) / len(per_read), 3), "dac_ms_max_chunk": round(max(per_read), 3),
                        "samples_per_row": samples[0], "codec_prompt_frames": codec_rows}
        model._engine.close()
        model._engine = None
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
