"""The optimizer step (unimoe_audio_amd/optim.py) on the synthetic model of scripts/train_bench.py, next to what a user can assemble
from torch today: fp32 master copies, gradients cast up (torch._foreach_copy_), clip_grad_norm_(foreach=True), AdamW(fused=True),
torch._foreach_copy_ back into the bf16 parameters.  Both legs run in ONE process, alternating, median of OB_REPS (3) with the spreads;
the three stages are timed on their own as well, and train.train_step end to end next to forward + backward alone.

OB_LAYERS (default 12): the two legs' state does not fit next to each other at 36 layers (12 + 16 bytes per parameter on top of weights,
gradients and activations), so both legs run the same reduced depth; the per-parameter figures do not depend on the depth.
Writes one JSON object to --out (default profiles/optim_step.json) and prints it."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from unimoe_audio_amd import _lib as L  # noqa: E402
from unimoe_audio_amd import train as TR  # noqa: E402
from unimoe_audio_amd.config import UniMoEAudioConfig  # noqa: E402
from unimoe_audio_amd.model import UniAudioRVQQwen2_5VLMoEForConditionalGeneration  # noqa: E402
from unimoe_audio_amd.optim import AdamW, make_hyper  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "optim_step.json"))
args = ap.parse_args()
layers = int(os.environ.get("OB_LAYERS", "12"))
reps = int(os.environ.get("OB_REPS", "3"))
B, T = int(os.environ.get("OB_BATCH", "4")), int(os.environ.get("OB_T", "1560"))
MAX_NORM, LR, WD = 1.0, 1e-5, 0.01
COPY_TBS = 6.29          # the copy rate of MI355X_MICROARCH.md the issue measures against
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
g = torch.Generator().manual_seed(11)
n_text = 40
ids = torch.randint(0, 151643, (B, T), generator=g)
ids[:, n_text:] = cfg.codec_placeholder_value
codec = torch.randint(0, 1024, (B * (T - n_text), cfg.codec_channels), generator=g)
labels = torch.randint(0, 1024, (B, T, cfg.codec_channels), generator=g)
labels[:, :n_text] = -100
am = torch.ones(B, T, dtype=torch.long)


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


def fwd_bwd():
    loss, _, _ = TR.forward_train(model, ids, codec, am, labels)
    loss.backward()


# ---- end to end: forward + backward alone, then train_step (the optimizer's state is allocated by the first step)
mem0 = torch.cuda.memory_allocated()
opt = AdamW(TR.moe_param_groups(model, weight_decay=WD), lr=LR, max_grad_norm=MAX_NORM)
fwd_bwd()
opt.zero_grad(set_to_none=False)
t_fb = [timed(fwd_bwd) for _ in range(reps + 1)][1:]
opt.step()                                                   # allocates master / m / v
torch.cuda.synchronize()
state_alloc = torch.cuda.memory_allocated() - mem0 - sum(p.grad.numel() * p.grad.element_size() for p in model.parameters() if p.grad is not None)
opt.zero_grad(set_to_none=False)
t_ts = [timed(lambda: TR.train_step(model, opt, ids, codec, am, labels)) for _ in range(reps + 1)][1:]
peak_train = torch.cuda.max_memory_allocated()
fwd_bwd()                                                    # real gradients for the step-only legs below
params = [p for p in model.parameters() if p.grad is not None]
n_param = sum(p.numel() for p in params)

# ---- the torch leg
masters = [p.detach().float().clone().requires_grad_(True) for p in params]
for m_ in masters:
    m_.grad = torch.zeros_like(m_)
topt = torch.optim.AdamW(masters, lr=LR, weight_decay=WD, fused=True)
g32 = [m_.grad for m_ in masters]
g16 = [p.grad for p in params]
pdata = [p.data for p in params]


def torch_step():
    torch._foreach_copy_(g32, g16)
    torch.nn.utils.clip_grad_norm_(masters, MAX_NORM, foreach=True)
    topt.step()
    with torch.no_grad():
        torch._foreach_copy_(pdata, masters)


torch_step()
mem_torch_state = sum(t.numel() * 4 for t in masters) * 2 + sum(v.numel() * v.element_size() for st in topt.state.values() for v in st.values()
                                                              if isinstance(v, torch.Tensor))
# ---- the stages on their own (the optimizer's own tables)
lib, hy = L.lib(), make_hyper(opt.param_groups, MAX_NORM)
nt, nc = len(opt._params), len(opt._chunks_host)
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)      # noqa: E731
stage = {
    "sqsum": lambda: L.check(lib.umoe_optim_sqsum(opt._tensors.data_ptr(), nt, opt._chunks.data_ptr(), nc, opt.chunk_elems, None, None, hy.num_groups, 0,
                                                  opt._partial.data_ptr(), opt._flags.data_ptr(), stream())),
    "scalars": lambda: L.check(lib.umoe_optim_scalars(opt._partial.data_ptr(), opt._flags.data_ptr(), nc, C.byref(hy), opt._counters.data_ptr(),
                                                      opt._rec.data_ptr(), stream())),
    "adamw": lambda: L.check(lib.umoe_optim_adamw(opt._tensors.data_ptr(), nt, opt._chunks.data_ptr(), nc, opt.chunk_elems, None, None, 0, C.byref(hy),
                                                  opt._rec.data_ptr(), -1, opt._counters.data_ptr(), stream())),
}
opt.step()
hip, tor, st = [], [], {k: [] for k in stage}
for _ in range(reps):
    hip.append(timed(opt.step))
    tor.append(timed(torch_step))
    for k, fn in stage.items():
        st[k].append(timed(fn))
assert int(opt.skipped_steps) == 0, "a benchmark step was skipped"
h, t = stats(hip), stats(tor)
spread = max(h["max_ms"] - h["min_ms"], t["max_ms"] - t["min_ms"])
adamw_ms = stats(st["adamw"])["median_ms"]
out = {
    "workload": f"optimizer step, synthetic {layers}-layer model ({n_param / 1e9:.3f} B bf16 parameters), 1 x MI355X",
    "layers": layers, "layers_note": "36 layers do not fit with both legs' state resident; both legs run this depth",
    "parameters": n_param, "tensors": nt, "chunks": nc, "chunk_elems": opt.chunk_elems, "reps": reps,
    "hip_step": h, "torch_step": t, "ratio_hip_over_torch": round(h["median_ms"] / t["median_ms"], 4), "spread_ms": round(spread, 3),
    "hip_not_slower_than_torch_by_more_than_the_spread": bool(h["median_ms"] <= t["median_ms"] + spread),
    "stages": {k: stats(v) for k, v in st.items()},
    "bytes_per_parameter": {"adamw": 28, "sqsum": 2, "hip_step": 30,
                            "torch_leg": {"cast_up": 6, "norm": 4, "clip_scale_when_clipping": 8, "fused_adamw": 32, "copy_back": 6}},
    "adamw_TBps": round(28.0 * n_param / (adamw_ms * 1e-3) / 1e12, 3), "adamw_frac_of_copy_rate": round(28.0 * n_param / (adamw_ms * 1e-3) / 1e12 / COPY_TBS, 3),
    "sqsum_TBps": round(2.0 * n_param / (stats(st["sqsum"])["median_ms"] * 1e-3) / 1e12, 3),
    "optimizer_state_bytes": opt.state_bytes(), "optimizer_state_allocated_bytes": int(state_alloc),
    "optimizer_state_bytes_per_parameter": round(opt.state_bytes() / n_param, 3), "torch_leg_state_bytes": int(mem_torch_state),
    "train": {"batch": B, "tokens": T, "fwd_bwd": stats(t_fb), "train_step": stats(t_ts), "peak_GiB_train_step": round(peak_train / 2 ** 30, 1)},
    "grad_norm": float(opt.grad_norm), "steps": int(opt.steps),
}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
