"""Cost of an admission with and without a cached voice prefix on bench.py's synthetic model; writes
profiles/prefix_cache.json and prints it as one JSON line.

One voice: a prompt prefix of `--prefix` tokens (250 of them audio placeholders); sentences of `--sentence` tokens behind it, so the pair is
T = prefix + sentence + 6 tokens per row and the negative row is left padded by the sentence.  In ONE process, alternating, `--runs` times:

  one_shot   DecodeEngine.admit of the whole pair (2 x T tokens through the prefill body), with the embedding of all its tokens
  miss       build_prefix (the prefix alone, one row) + admit behind it
  hit        admit behind a store that is there: the install launch + 2 x (T - prefix) tokens, embedding of those columns only
  serving    wall time of 8 rows x `--steps` decode steps with 5 admissions (one every steps / 5), every admission one_shot against
             the first a miss and the other four hits
             (a loop of engine admit / step calls: the scheduler's polling and the tokeniser of UniMoEAudio.serve are not in it)

The reference audio's DAC encode, which a VoicePrompt also saves per request, is not part of any figure (no codec weights here).
Nothing is asserted but equal results of miss and hit; `hit_faster_beyond_spread` says whether the hit's slowest run beat the one-shot's
fastest.

    python scripts/prefix_bench.py --runs 3"""
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


class Voice:
    """ids / codes of one voice and of sentences in it, laid out as UniMoEAudio._speech_texts lays them out"""

    def __init__(self, model, cfg, a, device):
        g = torch.Generator().manual_seed(11)
        self.model, self.cfg, self.device, self.P = model, cfg, device, a.prefix
        self.prefix = torch.randint(0, 151643, (a.prefix,), generator=g)
        self.prefix[-252:-2] = cfg.codec_placeholder_value
        self.pc = torch.randint(0, 1024, (250, cfg.codec_channels), generator=g).to(device)
        self.tail = torch.randint(0, 151643, (6,), generator=g)
        self.sentence = torch.randint(0, 151643, (a.sentence,), generator=g)
        self.T = a.prefix + a.sentence + 6
        self.ids = torch.zeros(2, self.T, dtype=torch.long)
        self.am = torch.zeros(2, self.T, dtype=torch.long)
        for r, row in enumerate((torch.cat([self.prefix, self.tail]), torch.cat([self.prefix, self.sentence, self.tail]))):
            self.ids[r, self.T - len(row):], self.am[r, self.T - len(row):] = row, 1
        self.ids_dev = self.ids.to(device)
        self.x_prefix = model.calculate_input_embedding(self.prefix[None].to(device), self.pc)[0].contiguous()     # cached with the voice

    def x_full(self):
        x = self.model.calculate_input_embedding(self.ids_dev, torch.cat([self.pc, self.pc]))
        return x.reshape(-1, x.shape[-1]).contiguous()

    def x_suffix(self):
        P, first = self.P, self.T - int(self.am[0].sum())
        x = self.model.language_model.embed_tokens.weight[self.ids_dev[:, P:]]
        x[0, :first] = self.x_prefix[P - first:]                  # the shorter row repeats its last prefix tokens behind its pads
        return x.reshape(-1, x.shape[-1]).contiguous()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--prefix", type=int, default=272)
    ap.add_argument("--sentence", type=int, default=30)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--codec-channels", type=int, default=0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefix_cache.json"))
    a = ap.parse_args()
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    from unimoe_audio_amd.model import DecodeEngine
    device = torch.device("cuda:0")
    cfg = bench.make_cfg(a)
    model, _ = bench.build_model(cfg, device)
    with torch.no_grad():
        v = Voice(model, cfg, a, device)
        B, T, P = a.slots, v.T, v.P
        max_tokens = a.steps + 64
        eng = DecodeEngine(model, B, Lmax=T + max_tokens + 8, Tmax=max_tokens + 64)
        pre, ps = prepare_audio_prompt(cfg, [None])
        kw = dict(max_tokens=max_tokens, min_tokens=max_tokens, **SET)

        def one_shot(row):
            eng.admit(row, v.x_full(), v.am, pre[0], ps[0], **kw)

        def behind(row, store):
            eng.admit(row, v.x_suffix(), v.am, pre[0], ps[0], prefix=store, prefix_len=P, **kw)

        def miss(row):
            store = eng.build_prefix(row, v.x_prefix)
            behind(row, store)
            return store

        shape = (cfg.num_hidden_layers, 2 * B, cfg.num_key_value_heads, eng.Lmax, cfg.head_dim)
        ms = {"one_shot": [], "miss": [], "hit": [], "serve_one_shot_wall": [], "serve_prefix_wall": []}
        eng.start_serving(T)
        one_shot(0)
        miss(1)                                                   # (first calls: group tables, lazy allocations)
        for _ in range(a.runs):
            eng.start_serving(T)
            ms["one_shot"].append(timed(lambda: one_shot(0))[0])
            t, store = timed(lambda: miss(1))
            ms["miss"].append(t)
            ms["hit"].append(timed(lambda: behind(2, store))[0])
            k = eng.copy_buffer("k_cache", torch.bfloat16, shape)
            for r, first in enumerate((a.sentence, 0)):          # (below its first valid slot a row keeps whatever was there)
                assert torch.equal(k[:, 2 + r, :, first:T].view(torch.int16), k[:, 4 + r, :, first:T].view(torch.int16)), "hit and miss wrote different keys"
            del k
            for name in ("serve_one_shot_wall", "serve_prefix_wall"):
                eng.start_serving(T)
                for b in range(B - 5):                            # the rows that decode from the start
                    one_shot(b)
                every, store = a.steps // 5, None

                def leg():
                    nonlocal store
                    for s in range(a.steps):
                        if s % every == 0 and s // every < 5:
                            row = B - 5 + s // every
                            if name == "serve_one_shot_wall":
                                one_shot(row)
                            elif store is None:
                                store = miss(row)
                            else:
                                behind(row, store)
                        eng.step(True)
                ms[name].append(timed(leg)[0])
                assert eng.handoff_error() == 0
        eng.close()
    med = {k: round(statistics.median(x), 3) for k, x in ms.items()}
    out = {"metric": "ms per admission of one CFG pair: whole prompt vs behind a cached voice prefix; wall ms of 8 rows x steps with 5 admissions",
           "slots": B, "layers": cfg.num_hidden_layers, "prefix_tokens": P, "sentence_tokens": a.sentence, "pair_tokens_per_row": T,
           "columns_behind_the_prefix": T - P, "steps": a.steps, "runs": a.runs,
           **{k + "_ms": [round(x, 3) for x in xs] for k, xs in ms.items()}, **{k + "_median_ms": m for k, m in med.items()},
           "hit_faster_beyond_spread": max(ms["hit"]) < min(ms["one_shot"]),
           "serve_faster_beyond_spread": max(ms["serve_prefix_wall"]) < min(ms["serve_one_shot_wall"]),
           "store_bytes": cfg.num_hidden_layers * 2 * cfg.num_key_value_heads * P * cfg.head_dim * 2,
           "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", "").split(":")[0]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
