"""Measurement (not a test): the DAC side of a request at the reference's 16 kHz / 50 Hz geometry (descript-audio-codec 1.0.0: encoder_dim
64, decoder_dim 1536, rates 2 4 5 8, 12 codebooks), synthetic weights, one MI355X: decode of N frames of codes (RVQ from_codes + the
conv decoder) and encode of a prompt clip (conv encoder + 12-level residual RVQ).  Prints one JSON line.

  python scripts/dac_bench.py [--frames 500] [--prompt-seconds 4.5] [--conv-form direct|mfma|both]

--conv-form both: the direct fp32 kernels and the f32 MFMA kernels in ONE process on two models with the same weights,
alternating, median of 3 with the spread (max - min): decode of 10 s and 30 s of codes, encode of the prompt, and per decoder layer
the time, FLOP and achieved TFLOP/s (against the 157 TF f32-matrix peak) of the full form at B = 1 and of one per-row read of 16
frames at 8 and 32 rows (DacRowStreamDecoder in its steady state, every row with news; one decoder per form, their reads alternating).
A read's total is taken as it runs in serving, host enqueue included.  The per-layer times are taken in reads of their own, each queued
behind a few large matrix products, so that every launch of the read is enqueued before the first one starts: the events around a
launch then bracket the kernel alone, not the host's time between two enqueues (with the fast form the GPU otherwise runs ahead of the
host and an event pair measures the Python side).  Writes profiles/dac_mfma.json too.

--reads-only: nothing but per-row reads (8 rows direct, 8 rows mfma, 32 rows direct, 32 rows mfma; 3 reads to fill the look-ahead, then
3 more each), for a kernel trace: `rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/dac_bench.py --reads-only`
gives every launch's own duration on the GPU, 30 conv launches per read in layer order.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from unimoe_audio_amd import dac as D

PEAK_TF = 157.0          # f32-input MFMA, MI355X


def t_ms(fn, n=5):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return sorted(ts)[len(ts) // 2] * 1e3


def layer_flop(ly, n_out):
    """multiply-adds x 2 of n_out output positions per channel plane"""
    taps = ly.K if ly.kind == "conv" else ly.K / ly.stride
    return 2.0 * ly.cin * ly.cout * taps * n_out


def med(xs):
    return round(statistics.median(xs), 4), round(max(xs) - min(xs), 4)


def pair(direct, mfma):
    """two lists of times -> medians, spreads, and whether mfma beats direct by more than the two spreads added"""
    (d, ds), (m, ms) = med(direct), med(mfma)
    return {"direct_ms": d, "direct_spread_ms": ds, "mfma_ms": m, "mfma_spread_ms": ms, "direct_over_mfma": round(d / m, 3),
            "beyond_spreads": bool(d - m > ds + ms)}


def layer_rows(plan, n_out, times):
    """times: {form: [per run [per layer ms]]} -> the per-layer table"""
    rows = []
    for i, ly in enumerate(plan.layers):
        fl = layer_flop(ly, n_out[i])
        r = {"layer": i, "kind": ly.kind, "cin": ly.cin, "cout": ly.cout, "K": ly.K, "stride": ly.stride, "dil": ly.dil, "outputs": n_out[i],
             "gflop": round(fl / 1e9, 3), "routed": "mfma" if D.uses_mfma(ly.cin, ly.cout, ly.K, ly.stride) else "direct"}
        r.update(pair([run[i] for run in times["direct"]], [run[i] for run in times["mfma"]]))
        for form in ("direct", "mfma"):
            r[f"{form}_tflops"] = round(fl / (r[f"{form}_ms"] * 1e-3) / 1e12, 2) if r[f"{form}_ms"] > 0 else None
        r["mfma_pct_of_peak"] = round(100 * r["mfma_tflops"] / PEAK_TF, 1)
        rows.append(r)
    return rows


_LAG = {}


def lag(n=3):
    """a few large fp32 matrix products on the current stream (some 20 ms): what is enqueued behind them starts when they end"""
    if not _LAG:
        _LAG["a"] = torch.randn(6144, 6144, device="cuda")
        _LAG["c"] = torch.empty_like(_LAG["a"])
    for _ in range(n):
        torch.mm(_LAG["a"], _LAG["a"], out=_LAG["c"])


def timed_layers(model, fn):
    """fn() with every DacModel._conv call between two events, queued behind lag() -> [ms per call]"""
    evs, conv = [], model._conv

    def wrapped(m, x, f, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        y = conv(m, x, f, **kw)
        e1.record()
        evs.append((e0, e1, y.shape[2]))
        return y

    model._conv = wrapped
    try:
        lag()
        fn()
    finally:
        del model._conv
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b, _ in evs], [n for _, _, n in evs]


class RowReader:
    """DacRowStreamDecoder in its steady state, every row `frames` more frames per read (after three reads that fill the look-ahead)"""

    def __init__(self, model, slots, frames, reads):
        z = torch.randn(slots, model.latent_dim, frames * (reads + 3), device="cuda")

        def src(requests, slab):
            for row, f0, n, col in requests:
                slab[row, :, col:col + n] = z[row, :, f0:f0 + n]

        self.dec, self.slots, self.frames, self.evs = D.DacRowStreamDecoder(model, slots, src, max_frames=frames), slots, frames, []
        conv_rows = self.dec._conv_rows

        def wrapped(i, wins, wave, table):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            conv_rows(i, wins, wave, table)
            e1.record()
            self.evs.append((e0, e1, max((v.n for v in wins), default=0)))

        self.dec._conv_rows = wrapped
        for _ in range(3):
            self.read()

    def read(self, behind_lag=False):
        """one read -> (ms of the whole read, [ms per layer], [outputs per layer and row])"""
        del self.evs[:]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if behind_lag:
            lag()
        e0.record()
        self.dec.push([self.frames] * self.slots)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), [x.elapsed_time(y) for x, y, _ in self.evs], [n for _, _, n in self.evs]


def both(a):
    dev = torch.device("cuda:0")
    models = {"direct": D.DacModel().init_random(5).to(dev).float(), "mfma": D.DacModel().init_random(5).to(dev).float().set_conv_form("mfma")}
    plan = D.stream_plan(models["direct"])
    wav = torch.randn(1, 1, int(a.prompt_seconds * 16000), device=dev) * 0.1
    res = {"metric": "dac_mfma", "workload": "DAC 16 kHz / 50 Hz, synthetic weights, fp32, 1 x MI355X; direct = fp32 VALU kernels, mfma = v_mfma_f32_16x16x4_f32",
           "runs": a.runs, "peak_tflops_f32_matrix": PEAK_TF}
    with torch.no_grad():
        for tag, frames in (("decode_10s", 500), ("decode_30s", 1500)):
            codes = torch.randint(0, 1024, (1, 12, frames), device=dev)
            ts = {"direct": [], "mfma": []}
            for _ in range(a.runs):
                for form, m in models.items():
                    ts[form].append(t_ms(lambda: m.decode(m.from_codes(codes)), 3))
            res[tag] = pair(ts["direct"], ts["mfma"])
            print(tag, json.dumps(res[tag]), flush=True)
        ts = {"direct": [], "mfma": []}
        for _ in range(a.runs):
            for form, m in models.items():
                ts[form].append(t_ms(lambda: m.encode(m.preprocess(wav, 16000)), 3))
        res["encode_prompt"] = dict(pair(ts["direct"], ts["mfma"]), seconds=a.prompt_seconds)
        print("encode_prompt", json.dumps(res["encode_prompt"]), flush=True)
        # per layer, full form, B = 1, 10 s
        codes = torch.randint(0, 1024, (1, 12, 500), device=dev)
        zq = models["direct"].from_codes(codes)
        lt, n_out = {"direct": [], "mfma": []}, None
        for _ in range(a.runs):
            for form, m in models.items():
                ms, n_out = timed_layers(m, lambda: m.decode(zq))
                lt[form].append(ms)
        res["layers_full_10s"] = layer_rows(plan, n_out, lt)
        for slots in (8, 32):
            tot, lay = {"direct": [], "mfma": []}, {"direct": [], "mfma": []}
            readers = {form: RowReader(m, slots, 16, 2 * a.runs) for form, m in models.items()}
            for _ in range(a.runs):                      # the reads as they run in serving, the forms alternating
                for form, rd in readers.items():
                    tot[form].append(rd.read()[0])
            for _ in range(a.runs):                      # per layer: kernel time, every launch enqueued before the read starts
                for form, rd in readers.items():
                    _, pl, n_out = rd.read(behind_lag=True)
                    lay[form].append(pl)
            res[f"read_16_frames_{slots}_rows"] = dict(pair(tot["direct"], tot["mfma"]), layers=layer_rows(plan, [n * slots for n in n_out], lay))
            print(f"read_16_frames_{slots}_rows", json.dumps({k: v for k, v in res[f"read_16_frames_{slots}_rows"].items() if k != "layers"}), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=500)             # 10 s of 50 Hz frames
    ap.add_argument("--prompt-seconds", type=float, default=4.5)   # a 4.5 s reference clip
    ap.add_argument("--conv-form", choices=["direct", "mfma", "both"], default="direct")
    ap.add_argument("--runs", type=int, default=3, help="with --conv-form both: runs per form, alternating")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dac_mfma.json"), help="with --conv-form both")
    ap.add_argument("--reads-only", action="store_true")
    a = ap.parse_args()
    if a.reads_only:
        with torch.no_grad():
            for slots in (8, 32):
                for form in ("direct", "mfma"):
                    m = D.DacModel().init_random(5).to("cuda:0").float().set_conv_form(form)
                    rd = RowReader(m, slots, 16, 3)
                    print(slots, form, [round(rd.read()[0], 3) for _ in range(3)], flush=True)
        return
    if a.conv_form == "both":
        return both(a)
    dev = torch.device("cuda:0")
    m = D.DacModel().init_random(5).to(dev).float().set_conv_form(a.conv_form)
    n_par = sum(p.numel() for p in m.parameters())
    codes = torch.randint(0, 1024, (1, 12, a.frames), device=dev)

    with torch.no_grad():
        dec_ms = t_ms(lambda: m.decode(m.from_codes(codes)))
        wav = torch.randn(1, 1, int(a.prompt_seconds * 16000), device=dev) * 0.1
        enc_ms = t_ms(lambda: m.encode(m.preprocess(wav, 16000)))
    kind = "fp32 conv kernels" if a.conv_form == "direct" else "fp32 MFMA conv kernels"
    print(json.dumps({"workload": f"DAC 16 kHz / 50 Hz, {n_par / 1e6:.1f} M parameters, {kind}, synthetic weights, 1 x MI355X",
                      "decode_frames": a.frames, "decode_audio_seconds": a.frames / 50.0, "decode_ms": round(dec_ms, 2),
                      "encode_prompt_seconds": a.prompt_seconds, "encode_ms": round(enc_ms, 2)}))


if __name__ == "__main__":
    main()
