"""CLI mirror of the reference's examples/inference.py (flags --task/-t --input/-i --ref-audio/-ra --ref-text/-rt
--video/-v --output/-o --model/-m --device/-d --no-reuse; exit code 0/1, reference examples/inference.py:152-235).
--requests FILE.json (not in the reference): speech and music requests with their own settings in ONE decode batch; with --serve the
list is a queue served by --slots rows, each request admitted as soon as a row is free; --serve --stream prints every request's
chunks as they arrive and writes the same wav files."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
_MODEL = None


def inference(task, input_text, model_path, ref_audio=None, ref_text=None, video=None, output="./output", device=0, reuse=True,
              expert_weights="bf16", stream=False, dac_conv="direct"):
    global _MODEL
    from unimoe_audio_amd.api import UniMoEAudio
    try:
        if _MODEL is None or not reuse:
            _MODEL = UniMoEAudio(model_path, device, expert_weights=expert_weights, dac_conv=dac_conv)
        if stream:
            return _stream(_MODEL, task, input_text, ref_audio, ref_text, video, output)
        if task == "text_to_speech":
            return _MODEL.text_to_speech(input_text, ref_text, ref_audio, output_dir=output)
        if task == "text_to_music":
            return _MODEL.text_to_music(input_text, output_dir=output)
        if task == "video_text_to_music":
            return _MODEL.video_text_to_music(video, input_text, output_dir=output)
        raise ValueError(f"unknown task {task}")
    except Exception as e:   # the reference swallows every exception and returns None (examples/inference.py:116-118)
        print(f"inference failed: {e}")
        return None


def load_requests(path):
    """FILE.json: a list of objects, {"task": "text_to_speech", "transcription": ..., "prompt_transcription": ..., "prompt_wav": ...}
    or {"task": "text_to_music", "caption": ...}, each with any further field of SpeechRequest / MusicRequest (max_audio_seconds,
    temperature, cfg_scale, seed, ...)"""
    from unimoe_audio_amd.api import MusicRequest, SpeechRequest
    kinds = {"text_to_speech": SpeechRequest, "text_to_music": MusicRequest}
    reqs = []
    for i, item in enumerate(json.load(open(path))):
        item = dict(item)
        task = item.pop("task", None)
        if task not in kinds:
            raise ValueError(f"{path}: request {i}: task must be one of {sorted(kinds)}")
        reqs.append(kinds[task](**item))
    return reqs


def batch_inference(requests_file, model_path, output="./output", device=0, reuse=True, expert_weights="bf16", stream=False, serve=False,
                    slots=8, prefix_cache=False, dac_conv="direct"):
    global _MODEL
    from unimoe_audio_amd.api import UniMoEAudio
    try:
        reqs = load_requests(requests_file)
        if _MODEL is None or not reuse:
            _MODEL = UniMoEAudio(model_path, device, expert_weights=expert_weights, dac_conv=dac_conv)
        if serve:
            # continuous batching: `slots` rows decode together, a request takes a row as soon as one is free
            import time
            t0, paths = time.perf_counter(), {}
            kw = dict(slots=slots, output_dir=output, max_audio_seconds=max(r.max_audio_seconds for r in reqs), prefix_cache=prefix_cache)
            if stream:
                # every request's audio in chunks as its frames become final, chunks of different requests interleaved
                for ch in _MODEL.serve(reqs, stream=True, **kw):
                    print(f"{time.perf_counter() - t0:8.3f} s  request {ch.row}  samples {ch.start_sample}..{ch.start_sample + ch.pcm.numel()}"
                          f"{'  (last)' if ch.final else ''}", flush=True)
                return [os.path.join(output, f"generated_{r.save_name}_{i}.wav") for i, r in enumerate(reqs)]
            for i, path in _MODEL.serve(reqs, slots=slots, output_dir=output, max_audio_seconds=max(r.max_audio_seconds for r in reqs),
                                        prefix_cache=prefix_cache):
                hit, n = _MODEL.served_prefix.get(i, (False, 0))
                note = f"  (voice prefix of {n} tokens {'reused' if hit else 'prefilled'})" if n else ""
                print(f"{time.perf_counter() - t0:8.3f} s  request {i}  {path}{note}", flush=True)
                paths[i] = path
            return [paths[i] for i in sorted(paths)]
        if not stream:
            return _MODEL.generate_batch(reqs, output_dir=output)
        import time
        t0 = time.perf_counter()
        for ch in _MODEL.generate_batch(reqs, output_dir=output, stream=True):
            print(f"{time.perf_counter() - t0:8.3f} s  request {ch.row}  samples {ch.start_sample}..{ch.start_sample + ch.pcm.numel()}"
                  f"{'  (last)' if ch.final else ''}", flush=True)
        return [os.path.join(output, f"generated_{r.save_name}_{i}.wav") for i, r in enumerate(reqs)]
    except Exception as e:
        print(f"inference failed: {e}")
        return None


def _stream(m, task, input_text, ref_audio, ref_text, video, output):
    """the *_stream twins: print when each chunk arrives, then the same wav files as the non-streaming methods"""
    import time
    t0 = time.perf_counter()
    if task == "text_to_speech":
        chunks = m.text_to_speech_stream(input_text, ref_text, ref_audio, output_dir=output)
    elif task == "text_to_music":
        chunks = m.text_to_music_stream(input_text, output_dir=output)
    elif task == "video_text_to_music":
        chunks = m.video_text_to_music_stream(video, input_text, output_dir=output)
    else:
        raise ValueError(f"unknown task {task}")
    rows = set()
    for ch in chunks:
        rows.add(ch.row)
        print(f"{time.perf_counter() - t0:8.3f} s  row {ch.row}  samples {ch.start_sample}..{ch.start_sample + ch.pcm.numel()}"
              f"{'  (last)' if ch.final else ''}", flush=True)
    stem = {"text_to_speech": "speech", "text_to_music": "music", "video_text_to_music": "video_music"}[task]
    return [os.path.join(output, f"generated_{stem}_{i}.wav") for i in sorted(rows)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", "-t", choices=["text_to_speech", "text_to_music", "video_text_to_music"])
    ap.add_argument("--input", "-i")
    ap.add_argument("--requests", help="a JSON list of text_to_speech / text_to_music requests, each with its own settings, decoded as "
                                       "one batch (UniMoEAudio.generate_batch); replaces --task / --input")
    ap.add_argument("--ref-audio", "-ra")
    ap.add_argument("--ref-text", "-rt")
    ap.add_argument("--video", "-v")
    ap.add_argument("--output", "-o", default="./output")
    ap.add_argument("--model", "-m", required=True)
    ap.add_argument("--device", "-d", type=int, default=0)
    ap.add_argument("--no-reuse", action="store_true")
    ap.add_argument("--expert-weights", choices=["bf16", "fp8", "fp8-only", "w12-only"], default="bf16",
                    help="fp8: weight-only e4m3 expert weights in the decode engine (half the expert bytes per step; with --serve at every --slots 1..32); "
                         "fp8-only: the same and the bf16 expert weights are released (5.5 GB of experts instead of 27 GB, prefill on the e4m3 copies); "
                         "w12-only: the bf16 expert weights are released in favour of their lossless 12-bit copies (no result changes by a bit; prefill on the copies)")
    ap.add_argument("--dac-conv", choices=["direct", "mfma"], default="direct",
                    help="mfma: the codec's convolutions on the f32 matrix cores (exact fp32, another summation order: the last bits of a waveform differ)")
    ap.add_argument("--stream", action="store_true", help="stream the audio in chunks while the decode loop runs (prints each chunk's arrival)")
    ap.add_argument("--serve", action="store_true", help="with --requests: serve the list as a queue (UniMoEAudio.serve): --slots rows decode "
                                                         "together and a request is admitted as soon as a row is free; any number of requests")
    ap.add_argument("--slots", type=int, default=8, help="rows of the serving batch (1..32)")
    ap.add_argument("--prefix-cache", action="store_true", help="with --serve: speech requests with the same reference audio and prompt text share one "
                                                                "prefilled voice prompt; each admission prefills only its sentence")
    a = ap.parse_args()
    if a.requests:
        if a.prefix_cache and not a.serve:
            ap.error("--prefix-cache goes with --serve")
        out = batch_inference(a.requests, a.model, a.output, a.device, not a.no_reuse, a.expert_weights, a.stream, a.serve, a.slots, a.prefix_cache,
                              a.dac_conv)
        sys.exit(0 if out else 1)
    if not a.task or a.input is None:
        ap.error("--task and --input are required (or --requests FILE.json)")
    out = inference(a.task, a.input, a.model, a.ref_audio, a.ref_text, a.video, a.output, a.device, not a.no_reuse, a.expert_weights,
                    a.stream, a.dac_conv)
    sys.exit(0 if out else 1)


if __name__ == "__main__":
    main()
