"""An optimizer step over A = 2 and A = 4 micro-batches in fp32 main gradients (train.train_step_accum: the weight-gradient GEMMs add
into the main gradients, one fold launch per micro-batch, AdamW reads fp32) next to the only thing the code offered before: A calls of
forward_train + backward() with autograd's bf16 `grad +=`, then opt.step() and opt.zero_grad().  Synthetic model of
scripts/optim_bench.py (AB_LAYERS, default 12) at batch 4 x 1560.  Both legs run in ONE process, alternating, one untimed iteration
after every switch (the gradient buffers and the optimizers' tables change with the leg), median of AB_REPS (3) with the spreads; one
backward alone in both forms and the peak memory of each leg are recorded too.

For A = 4 it also records the relative error of the accumulated gradient of both legs against the float64 sum of the four micro-batch
gradients (each taken on its own in fp32 main gradients from zero) -- the figure that justifies the feature.
Writes one JSON object to --out (default profiles/grad_accum.json) and prints it."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from unimoe_audio_amd import train as TR  # noqa: E402
from unimoe_audio_amd.config import UniMoEAudioConfig  # noqa: E402
from unimoe_audio_amd.model import UniAudioRVQQwen2_5VLMoEForConditionalGeneration  # noqa: E402
from unimoe_audio_amd.optim import AdamW  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "grad_accum.json"))
args = ap.parse_args()
layers = int(os.environ.get("AB_LAYERS", "12"))
reps = int(os.environ.get("AB_REPS", "3"))
B, T = int(os.environ.get("AB_BATCH", "4")), int(os.environ.get("AB_T", "1560"))
MAX_NORM, LR, WD = 1.0, 1e-5, 0.01
dev = torch.device("cuda:0")
cfg = UniMoEAudioConfig()
cfg.num_hidden_layers = layers
torch.set_default_dtype(torch.bfloat16)
with torch.device(dev):
    model = UniAudioRVQQwen2_5VLMoEForConditionalGeneration(cfg)
torch.set_default_dtype(torch.float32)
model.init_synthetic(1234).train()
for p in model.parameters():
    p.requires_grad_(True)
n_text = 40


def micro_batch(seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, 151643, (B, T), generator=g)
    ids[:, n_text:] = cfg.codec_placeholder_value
    codec = torch.randint(0, 1024, (B * (T - n_text), cfg.codec_channels), generator=g)
    labels = torch.randint(0, 1024, (B, T, cfg.codec_channels), generator=g)
    labels[:, :n_text] = -100
    return ids, codec, torch.ones(B, T, dtype=torch.long), labels


mbs = [micro_batch(11 + i) for i in range(4)]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(ts):
    s = sorted(ts)
    return dict(median_ms=round(s[len(s) // 2], 3), min_ms=round(s[0], 3), max_ms=round(s[-1], 3))


main = TR.attach_main_grads(model)
opt_main = AdamW(TR.moe_param_groups(model, weight_decay=WD), lr=LR, max_grad_norm=MAX_NORM)
opt_bf16 = AdamW(TR.moe_param_groups(model, weight_decay=WD), lr=LR, max_grad_norm=MAX_NORM)
n_param = sum(p.numel() for p in main.params)


def use_main(on: bool):
    """switches the leg: the gradient buffers of the other leg go (a GEMM-route weight keeps no zeroed bf16 .grad for the fold to read)"""
    (main.attach if on else main.detach)()
    for p in model.parameters():
        p.grad = None
    main.zero_()


def step_main(A):
    TR.train_step_accum(model, opt_main, mbs[:A])


def step_bf16(A):
    for mb in mbs[:A]:
        loss, _, _ = TR.forward_train(model, *mb)
        (loss / A).backward()                      # autograd: bf16 grad += dW, one torch add kernel per parameter
    opt_bf16.step()
    opt_bf16.zero_grad(set_to_none=False)


def backward_only(fold):
    loss, _, _ = TR.forward_train(model, *mbs[0])
    t = timed(loss.backward)
    t_fold = timed(main.fold) if fold else 0.0
    return t, t_fold


if os.environ.get("AB_LEG"):                       # one leg alone, four steps of A = 2, for a kernel trace (rocprofv3 --kernel-trace --stats
    leg = os.environ["AB_LEG"]                      # --output-format csv -d DIR -- python scripts/accum_bench.py; then scripts/kstat.py DIR name)
    use_main(leg == "main")
    for _ in range(4):
        (step_main if leg == "main" else step_bf16)(2)
    torch.cuda.synchronize()
    sys.exit(0)

res, peak = {}, {}
bwd = {"main_grad": [], "main_grad_fold": [], "bf16": []}
for A in (2, 4):
    tm, tb = [], []
    for r in range(reps):
        use_main(True)
        step_main(1)                                # untimed: allocations, table uploads
        torch.cuda.reset_peak_memory_stats()
        tm.append(timed(lambda: step_main(A)))
        peak[f"main_grad_A{A}"] = max(peak.get(f"main_grad_A{A}", 0), torch.cuda.max_memory_allocated())
        if A == 2:
            t, tf = backward_only(True)
            bwd["main_grad"].append(t)
            bwd["main_grad_fold"].append(tf)
        use_main(False)
        step_bf16(1)
        torch.cuda.reset_peak_memory_stats()
        tb.append(timed(lambda: step_bf16(A)))
        peak[f"bf16_A{A}"] = max(peak.get(f"bf16_A{A}", 0), torch.cuda.max_memory_allocated())
        if A == 2:
            bwd["bf16"].append(backward_only(False)[0])
    m, b = stats(tm), stats(tb)
    spread = max(m["max_ms"] - m["min_ms"], b["max_ms"] - b["min_ms"])
    res[f"A{A}"] = {"main_grad_step": m, "bf16_grad_step": b, "ratio_main_over_bf16": round(m["median_ms"] / b["median_ms"], 4),
                    "spread_ms": round(spread, 3), "main_not_slower_than_bf16_by_more_than_the_spread": bool(m["median_ms"] <= b["median_ms"] + spread)}
assert int(opt_main.skipped_steps) == 0 and int(opt_bf16.skipped_steps) == 0, "a benchmark step was skipped"


# ---- accuracy at A = 4: both legs against the float64 sum of the four micro-batch gradients (each on its own, fp32 main grads from zero)
def one(mb, scale, seed):
    model.training_steps = 0                       # the aux-loss weight follows a schedule: the same weight for every run
    torch.manual_seed(seed)
    loss, _, _ = TR.forward_train(model, *mb)
    (loss * scale).backward()


use_main(True)
each = []
for i, mb in enumerate(mbs):
    main.zero_()
    one(mb, 0.25, 100 + i)
    main.fold()
    each.append(main.flat.clone())
main.zero_()
for i, mb in enumerate(mbs):
    one(mb, 0.25, 100 + i)
    main.fold()
acc32 = main.flat.clone()
use_main(False)
for i, mb in enumerate(mbs):
    one(mb, 0.25, 100 + i)
torch.cuda.synchronize()
num32 = num16 = den = 0.0
worst16 = 0.0
for p, o in zip(main.params, main.offsets):
    if p.grad is None:
        continue
    sl = slice(o, o + p.numel())
    ref = sum(e[sl].double() for e in each)
    d = float((ref ** 2).sum())
    e16 = float(((p.grad.reshape(-1).double() - ref) ** 2).sum())
    num32 += float(((acc32[sl].double() - ref) ** 2).sum())
    num16 += e16
    den += d
    if d > 0:
        worst16 = max(worst16, (e16 / d) ** 0.5)
del each, acc32
out = {
    "workload": f"optimizer step over A micro-batches, synthetic {layers}-layer model ({n_param / 1e9:.3f} B bf16 parameters), batch {B} x {T}, 1 x MI355X",
    "layers": layers, "parameters": n_param, "reps": reps, "batch": B, "tokens": T,
    "legs": {"main_grad": "train.train_step_accum: fp32 main gradients, umoe_tiled_gemm_tn_acc + umoe_optim_fold, AdamW on fp32 gradients",
             "bf16": "A x (forward_train, backward with autograd's bf16 grad +=), opt.step(), opt.zero_grad()"},
    **res,
    "backward_alone": {"main_grad": stats(bwd["main_grad"]), "main_grad_fold": stats(bwd["main_grad_fold"]), "bf16": stats(bwd["bf16"])},
    "peak_GiB": {k: round(v / 2 ** 30, 1) for k, v in peak.items()},
    "main_grad_bytes": main.nbytes, "main_grad_bytes_per_parameter": round(main.nbytes / n_param, 3),
    "accumulated_gradient_A4": {"reference": "float64 sum of the four micro-batch gradients, each taken in fp32 main gradients from zero",
                                "rel_error_main_grad": (num32 / den) ** 0.5, "rel_error_bf16_grad": (num16 / den) ** 0.5,
                                "worst_tensor_rel_error_bf16_grad": worst16},
}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
