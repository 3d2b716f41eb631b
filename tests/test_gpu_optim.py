"""GPU suite of the optimizer step (csrc/umoe_optim.hip, unimoe_audio_amd/optim.py, train.train_step).

Stage 3 is compared per element with the fp64 restatement of tests/optim_ref.py (pinned to torch.optim.AdamW behind clip_grad_norm_ by
tests/test_optim_cpu.py), which is handed the kernel's OWN fp32 scalars (clip, bc1, bc2) and the previous state; the bounds are the
ones derived in optim_ref's docstring from the kernel's operation chain (c = 12 on |update|, 3 (1 + lr wd) on |w|, 4 on m, 6 on v --
counted roundings, not fitted).  The bf16 parameter must equal bf16_rne of the kernel's own stored master bit for bit.  Worst error /
bound is printed under -s.  Tensor sizes: 0, 1, 7, 8, 9, CH - 1, CH, CH + 1, 2 CH + 3 (CH = 16384, the product's chunk)."""
import ctypes as C

import numpy as np
import pytest
import torch

import optim_ref as R

pytestmark = pytest.mark.gpu
CH = 16384
SIZES = [0, 1, 7, 8, 9, CH - 1, CH, CH + 1, 2 * CH + 3]
PAD = 16
SENT = 12345.0                       # exact in bf16 and fp32
HP = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1), dict(lr=3e-4, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.0)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from unimoe_audio_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def leave_nothing_behind():
    """the models, optimizers and engines of this file are garbage once it ends: collect them and hand their blocks back, so that files
    that measure torch.cuda.memory_allocated() differences start from the allocator state they would have had without this one"""
    yield
    import gc
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def hyper(max_norm=None, hp=HP):
    from unimoe_audio_amd.optim import make_hyper
    return make_hyper(hp, max_norm)


def padded(dev, vals, dtype, off=0):
    """a buffer with PAD sentinel elements in front (+ off: the view starts at an odd element) and behind; -> (buffer, view)"""
    n = len(vals)
    buf = torch.full((PAD + off + n + PAD,), SENT, dtype=dtype)
    buf[PAD + off: PAD + off + n] = torch.from_numpy(np.asarray(vals, dtype=np.float32)).to(dtype)
    buf = buf.to(dev)
    return buf, buf[PAD + off: PAD + off + n]


def make_state(dev, seed, sizes=SIZES, fp32_at=(7,), offsets=None, zero_grad=False, zero_m=False):
    """one record per size: bf16 p / g with fp32 master (p = bf16(master)), or fp32 p / g; groups alternate.  offsets[i] = element
    offsets of (p, g, master, m, v) inside their buffers."""
    rng = np.random.default_rng(seed)
    out = []
    for i, n in enumerate(sizes):
        is32 = i in fp32_at
        dt = torch.float32 if is32 else torch.bfloat16
        off = (offsets or {}).get(i, (0, 0, 0, 0, 0))
        w = rng.normal(0, 0.03, n).astype(np.float32)
        g = np.zeros(n, np.float32) if zero_grad else rng.normal(0, 2e-3, n).astype(np.float32)
        m = np.zeros(n, np.float32) if zero_m else rng.normal(0, 1e-3, n).astype(np.float32)
        v = rng.normal(0, 2e-3, n).astype(np.float32) ** 2 + np.float32(1e-9)
        t = dict(group=i % 2, n=n, bufs={})
        t["bufs"]["p"], t["p"] = padded(dev, w, dt, off[0])
        t["bufs"]["g"], t["g"] = padded(dev, g, dt, off[1])
        if is32:
            t["master"] = None
        else:
            t["bufs"]["master"], t["master"] = padded(dev, w, torch.float32, off[2])
        t["bufs"]["m"], t["m"] = padded(dev, m, torch.float32, off[3])
        t["bufs"]["v"], t["v"] = padded(dev, v, torch.float32, off[4])
        out.append(t)
    return out


def snapshot(tensors):
    return [{k: b.clone() for k, b in t["bufs"].items()} for t in tensors]


def unchanged(tensors, snap, keys=None):
    return all(torch.equal(t["bufs"][k].view(torch.uint8), s[k].view(torch.uint8)) for t, s in zip(tensors, snap) for k in s if keys is None or k in keys)


def sentinels_intact(tensors):
    for t in tensors:
        for k, b in t["bufs"].items():
            view = t[k]
            lead = view.storage_offset() - b.storage_offset()
            if not (bool((b[:lead] == SENT).all()) and bool((b[lead + view.numel():] == SENT).all())):
                return False
    return True


def host(t, k):
    return t[k].float().cpu().numpy()


def check_update(tensors, before, rec, hp=HP, label=""):
    """every tensor against the restatement from `before` (host copies of w, m, v, g) with the record's scalars"""
    worst = np.zeros(3)
    for t, b in zip(tensors, before):
        if t["n"] == 0:
            continue
        h = hp[t["group"]]
        gi = t["group"]
        sc = dict(clip=rec["clip"], bc1=rec["bc1"][gi], bc2=rec["bc2"][gi])
        w1, m1, v1, parts = R.adamw_fp64(b["w"], b["m"], b["v"], b["g"], lr=h["lr"], beta1=h["betas"][0], beta2=h["betas"][1], eps=h["eps"],
                                         wd=h["weight_decay"], **sc)
        bw, bm, bv = R.adamw_bounds(parts, lr=h["lr"], wd=h["weight_decay"], bc1=sc["bc1"])
        wk = host(t, "p") if t["master"] is None else host(t, "master")
        tiny = np.finfo(np.float32).tiny
        assert np.all(np.abs(w1) > tiny) and np.all(v1 > tiny)                       # the bounds assume normal numbers
        ratios = (np.abs(wk - w1) / bw, np.abs(host(t, "m") - m1) / bm, np.abs(host(t, "v") - v1) / bv)
        for j, r in enumerate(ratios):
            assert np.all(np.isfinite(r))
            worst[j] = max(worst[j], float(r.max()))
        if t["master"] is not None:                                                  # p = bf16_rne(the kernel's own master), bit for bit
            bits = t["p"].view(torch.int16).cpu().numpy().view(np.uint16)
            assert np.array_equal(bits, R.bf16_rne(wk)), (label, t["n"])
    print(f"\nADAMW {label}: worst error / bound  w {worst[0]:.3f}  m {worst[1]:.3f}  v {worst[2]:.3f}")
    assert worst.max() <= 1.0, (label, worst)
    return worst


def before_of(tensors):
    return [dict(w=host(t, "p") if t["master"] is None else host(t, "master"), m=host(t, "m"), v=host(t, "v"), g=host(t, "g")) for t in tensors]


def run_all(tb, hy, grid_cap=0):
    assert tb.sqsum(grid_cap=grid_cap) == 0 and tb.scalars(hy) == 0 and tb.adamw(hy, grid_cap=grid_cap) == 0
    torch.cuda.synchronize()


# odd element offsets: tensor 8 (2 CH + 3) with every stream 3 elements in (bf16 6 bytes, fp32 12 bytes: 16-byte aligned together after
# 5 more elements -- the head / tail path); tensor 5 (CH - 1) with the parameter alone one element in (never aligned together: scalar)
OFFSETS = {8: (3, 3, 3, 3, 3), 5: (1, 0, 0, 0, 0), 6: (0, 0, 1, 2, 3)}


@pytest.mark.parametrize("t0", [0, 1, 999])
def test_update_per_element_against_fp64(dev, t0):
    """steps 1, 2 and 1000 (device counter set to 0, 1, 999); two groups with their own lr / wd / betas / eps, the second with wd = 0;
    tensor 7 (CH + 1) is an fp32 parameter without a master; offsets as above; clipping active (max_norm below the norm)"""
    tensors = make_state(dev, 10 + t0, offsets=OFFSETS)
    tb = R.Tables(tensors, CH, 2)
    tb.counters[0] = t0
    before = before_of(tensors)
    hy = hyper(max_norm=0.05)
    run_all(tb, hy)
    rec = tb.record()
    assert rec["skip"] == 0 and 0.0 < rec["clip"] < 1.0 and tb.counters.tolist() == [t0 + 1, 0]
    check_update(tensors, before, rec, label=f"t={t0}")
    assert sentinels_intact(tensors)
    # the same through the one-launch form (no record: clip 1, bias corrections from the host's counter)
    tensors = make_state(dev, 10 + t0, offsets=OFFSETS)
    tb = R.Tables(tensors, CH, 2)
    before = before_of(tensors)
    assert tb.adamw(hyper(), t_host=t0) == 0
    torch.cuda.synchronize()
    assert tb.counters.tolist() == [t0 + 1, 0]
    _, _, bcs = R.scalars_fp64([], None, [h["betas"] for h in HP], t0)
    rec1 = dict(clip=np.float32(1.0), bc1=[np.float32(b[0]) for b in bcs], bc2=[np.float32(b[1]) for b in bcs])
    check_update(tensors, before, rec1, label=f"t={t0} one launch")
    assert sentinels_intact(tensors)


def test_zero_gradients_without_decay_leave_the_weights_bit_identical(dev):
    hp = [dict(h, weight_decay=0.0) for h in HP]
    tensors = make_state(dev, 21, zero_grad=True, zero_m=True, offsets=OFFSETS)
    tb = R.Tables(tensors, CH, 2)
    snap = snapshot(tensors)
    v0 = [host(t, "v") for t in tensors]
    run_all(tb, hyper(max_norm=1.0, hp=hp))
    rec = tb.record()
    assert rec["norm"] == 0.0 and rec["clip"] == 1.0 and rec["skip"] == 0
    assert unchanged(tensors, snap, keys=("p", "master", "g", "m"))
    for t, v in zip(tensors, v0):                                           # v' = fl(fl(beta2) v) + 0, exactly
        assert np.array_equal(host(t, "v"), np.float32(hp[t["group"]]["betas"][1]) * v)
    assert sentinels_intact(tensors)


def test_zero_learning_rate_changes_nothing_but_the_moments(dev):
    hp = [dict(h, lr=0.0) for h in HP]
    tensors = make_state(dev, 22, offsets=OFFSETS)
    tb = R.Tables(tensors, CH, 2)
    snap = snapshot(tensors)
    before = before_of(tensors)
    run_all(tb, hyper(max_norm=None, hp=hp))
    rec = tb.record()
    assert rec["clip"] == 1.0
    assert unchanged(tensors, snap, keys=("p", "master", "g"))
    for t, b in zip(tensors, before):
        if t["n"]:
            h = hp[t["group"]]
            _, m1, v1 = R.adamw_emulated(b["w"], b["m"], b["v"], b["g"], lr=0.0, beta1=h["betas"][0], beta2=h["betas"][1], eps=h["eps"],
                                         wd=h["weight_decay"], clip=1.0, bc1=1.0, bc2=1.0)
            assert np.array_equal(host(t, "m"), m1) and np.array_equal(host(t, "v"), v1)      # and the moments DID move, exactly as emulated
            assert not np.array_equal(host(t, "m"), b["m"])
    assert sentinels_intact(tensors)


@pytest.mark.parametrize("t0", [0, 1, 999])
def test_norm_clip_and_bias_corrections_against_fp64(dev, t0):
    tensors = make_state(dev, 30 + t0, offsets=OFFSETS)
    grads = [host(t, "g") for t in tensors]
    hy = hyper(max_norm=0.05)
    recs, parts = [], []
    for cap in (0, 0, 3):                                   # twice the same; then 3 workgroups striding over the 11 chunks
        tb = R.Tables(tensors, CH, 2)
        tb.counters[0] = t0
        assert tb.sqsum(grid_cap=cap) == 0 and tb.scalars(hy) == 0
        torch.cuda.synchronize()
        recs.append(tb.rec.cpu().numpy().tobytes())
        parts.append(tb.partial.cpu().numpy().tobytes() + tb.flags.cpu().numpy().tobytes())
        assert tb.counters.tolist() == [t0 + 1, 0]
    assert recs[0] == recs[1] == recs[2] and parts[0] == parts[1] == parts[2]
    assert tb.n_chunks == 11 and not tb.flags.any()
    rec = tb.record()
    norm, _, bcs = R.scalars_fp64(grads, 0.05, [h["betas"] for h in HP], t0)
    nb = R.norm_rel_bound(CH)
    print(f"\nNORM t={t0}: {rec['norm']!r} vs {norm!r}: error / bound {abs(float(rec['norm']) - norm) / (nb * norm):.3f}")
    assert abs(float(rec["norm"]) - norm) <= nb * norm
    clip = min(1.0, 0.05 / (float(rec["norm"]) + 1e-6))                     # from the kernel's own norm
    assert clip < 1.0 and abs(float(rec["clip"]) - clip) <= R.CLIP_REL_BOUND * clip
    for gi, (b1, b2) in enumerate(bcs):
        assert abs(float(rec["bc1"][gi]) - b1) <= R.BC_REL_BOUND * b1 and abs(float(rec["bc2"][gi]) - b2) <= R.BC_REL_BOUND * b2, (gi, t0)
    # clipping off / not needed: exactly 1
    tb = R.Tables(tensors, CH, 2)
    for mn in (None, 1e6):
        assert tb.sqsum() == 0 and tb.scalars(hyper(max_norm=mn)) == 0
        torch.cuda.synchronize()
        assert tb.record()["clip"] == 1.0


@pytest.mark.parametrize("what", ["inf", "nan", "both"])
def test_a_step_with_a_non_finite_gradient_is_skipped_on_the_device(dev, what):
    tensors = make_state(dev, 40, offsets=OFFSETS)
    big = tensors[8]                                                          # 2 CH + 3 elements: chunks [0, CH), [CH, 2 CH), [2 CH, 2 CH + 3)
    clean = big["g"].clone()
    if what in ("inf", "both"):
        big["g"][CH] = float("inf")                                           # first element of a chunk
    if what in ("nan", "both"):
        big["g"][CH - 1] = float("nan")                                       # last element of a chunk
    tb = R.Tables(tensors, CH, 2)
    tb.counters[0] = 5
    snap = snapshot(tensors)
    hy = hyper(max_norm=0.05)
    run_all(tb, hy)
    assert tb.record()["skip"] == 1 and tb.counters.tolist() == [5, 1]
    assert int(tb.flags.sum()) == (2 if what == "both" else 1)
    assert unchanged(tensors, snap)
    big["g"].copy_(clean)                                                     # the next clean step proceeds from t = 5
    before = before_of(tensors)
    run_all(tb, hy)
    rec = tb.record()
    assert rec["skip"] == 0 and tb.counters.tolist() == [6, 1]
    assert abs(float(rec["bc1"][0]) - (1 - 0.9 ** 6)) <= R.BC_REL_BOUND
    check_update(tensors, before, rec, label=f"after a skipped step ({what})")
    assert sentinels_intact(tensors)


def test_tensors_outside_the_table_and_left_out_tensors_do_not_matter(dev):
    tensors = make_state(dev, 50, sizes=[CH + 1, 9, 2 * CH + 3, 100])
    for k in ("g", "m", "v", "master"):                                       # tensor 1: not in the table at all; tensor 3: in it, gradient None
        tensors[1][k].fill_(float("nan"))
        tensors[3][k].fill_(float("nan"))
    outside = tensors.pop(1)
    tensors[2]["g_kept"], tensors[2]["g"] = tensors[2]["g"], None
    tb = R.Tables(tensors, CH, 2)
    snap_out, snap_left = snapshot([outside]), snapshot([tensors[2]])
    before = before_of(tensors[:2])
    run_all(tb, hyper(max_norm=0.05))
    rec = tb.record()
    assert rec["skip"] == 0 and np.isfinite(rec["norm"]) and tb.counters.tolist() == [1, 0]
    assert unchanged([outside], snap_out) and unchanged([tensors[2]], snap_left)
    check_update(tensors[:2], before, rec, label="NaN outside the table")
    assert sentinels_intact(tensors[:2])


def test_an_empty_table_is_a_no_op_and_refusals_leave_everything_untouched(dev):
    from unimoe_audio_amd import _lib as L
    from unimoe_audio_amd.optim import OptimHyper, build_chunk_table
    hy = hyper(max_norm=0.05)
    empty = R.Tables(make_state(dev, 60, sizes=[0, 0]), CH, 2)
    assert empty.n_chunks == 0
    outs = lambda tb: [x.clone() for x in (tb.partial, tb.flags, tb.rec, tb.counters)]     # noqa: E731
    o = outs(empty)
    assert empty.sqsum() == 0 and empty.scalars(hy) == 0 and empty.adamw(hy) == 0 and empty.adamw(hy, t_host=3) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(o, outs(empty)))
    tensors = make_state(dev, 61, sizes=[CH + 1, 9])
    tb = R.Tables(tensors, CH, 2)
    snap, o = snapshot(tensors), outs(tb)
    h17 = OptimHyper(num_groups=17, max_norm=-1.0)
    crossing = build_chunk_table([CH + 1, 9], CH)
    crossing["first"][1] = 2 * CH                                             # past the end of tensor 0
    overlap = build_chunk_table([CH + 1, 9], CH)
    overlap["first"][1] = 8                                                   # inside, but not a chunk boundary: it would run into chunk 0
    bad_tensor = build_chunk_table([CH + 1, 9], CH)
    bad_tensor["tensor"][2] = 2
    refused = [
        tb.sqsum(tensors=None), tb.sqsum(chunks=None), tb.sqsum(partial=None), tb.sqsum(flags=None), tb.sqsum(num_groups=17), tb.sqsum(num_groups=0),
        tb.sqsum(chunk_elems=0), tb.sqsum(chunk_elems=12), tb.sqsum(hc=None),
        tb.scalars(hy, partial=None), tb.scalars(hy, rec=None), tb.scalars(hy, counters=None), tb.scalars(hy, hyper=None), tb.scalars(h17),
        tb.adamw(hy, tensors=None), tb.adamw(hy, chunks=None), tb.adamw(h17), tb.adamw(hy, chunk_elems=0), tb.adamw(hy, hyper=None),
        tb.adamw(hy, rec=None), tb.adamw(hy, t_host=4, rec=tb.rec.data_ptr()),
    ]
    for table in (crossing, overlap, bad_tensor):
        refused += [tb.sqsum(hc=table.ctypes.data), tb.adamw(hy, hc=table.ctypes.data)]
    assert all(rc < 0 for rc in refused), refused
    assert L.lib().umoe_last_error()
    torch.cuda.synchronize()
    assert unchanged(tensors, snap) and all(torch.equal(a, b) for a, b in zip(o, outs(tb)))
    # an unchecked device table with the same faults: the kernels skip those chunks instead of leaving their tensor
    tb2 = R.Tables(tensors, CH, 2, chunks=np.concatenate([crossing[1:2], bad_tensor[2:3]]))
    assert tb2.sqsum(host=False) == 0 and tb2.scalars(hyper()) == 0 and tb2.adamw(hyper(), host=False) == 0
    torch.cuda.synchronize()
    assert tb2.partial.tolist() == [0.0, 0.0] and unchanged(tensors, snap)


# ------------------------------------------------------------------------------------------------------------ the Python class
def small_cfg(**over):
    from unimoe_audio_amd.config import UniMoEAudioConfig
    kw = dict(hidden_size=256, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, vocab_size=320,
              dynamic_intermediate_size=128, shared_intermediate_size=64, codec_placeholder_value=300)
    kw.update(over)
    return UniMoEAudioConfig(**kw)


def build_model(cfg, seed, std=0.05):
    from unimoe_audio_amd.model import UniAudioRVQQwen2_5VLMoEForConditionalGeneration
    torch.manual_seed(seed)
    m = UniAudioRVQQwen2_5VLMoEForConditionalGeneration(cfg)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "layernorm" in n or n.endswith("norm.weight"):
                p.copy_(1 + 0.05 * torch.randn_like(p))
            elif n.endswith("bias"):
                p.normal_(0, 0.02)
            else:
                p.normal_(0, std)
    return m.to(torch.bfloat16)


def batch(cfg, B=2, T=40):
    torch.manual_seed(5)
    ids = torch.randint(0, 290, (B, T))
    am = torch.ones(B, T, dtype=torch.long)
    am[0, :6] = 0
    ids[:, -5:-2] = cfg.codec_placeholder_value
    codec = torch.randint(0, 1024, (B * 3, cfg.codec_channels))
    labels = torch.randint(0, 1024, (B, T, cfg.codec_channels))
    labels[:, :8] = -100
    return ids, codec, am, labels


def trainable(dev, seed=3):
    cfg = small_cfg()
    gm = build_model(cfg, seed).to(dev).train()
    for p in gm.parameters():
        p.requires_grad_(True)
    return cfg, gm


def fake_grads(params, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    for p in params:
        p.grad = (torch.randn(p.shape, generator=g) * 2e-3).to(p.dtype).to(p.device)


def first_step_logits(cfg, gm, dev):
    """prefill + one decode step of an engine built NOW on gm: the codec-head logits"""
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    B, T = 2, 12
    torch.manual_seed(2)
    ids = torch.randint(0, 290, (2 * B, T))
    am = torch.ones(2 * B, T, dtype=torch.long)
    am[0, :3] = 0
    ids[:, -5:-2] = cfg.codec_placeholder_value
    codec = torch.randint(0, 1024, (2 * B * 3, cfg.codec_channels))
    pre, psteps = prepare_audio_prompt(cfg, [None] * B)
    forced = torch.randint(0, 1024, (B, pre.shape[1] + 8, cfg.codec_channels)).to(torch.int32)
    keep = pre.to(torch.int32) != -1
    forced[:, : pre.shape[1]][keep] = pre.to(torch.int32)[keep]
    with torch.no_grad():
        eng = gm.engine(B, T, 64)
        eng.prefill(gm.calculate_input_embedding(ids.to(dev), codec.to(dev)).reshape(-1, cfg.hidden_size).contiguous(), am.to(dev))
        eng.start_decode(forced, psteps, 64, 6, cfg_scale=3.0, temperature=1.0, top_p=1.0, top_k=45, eos_mul=0.8, do_sample=False)
        eng.step(use_graph=False)
        got = eng.copy_buffer("logits", torch.float32, (2 * B, cfg.codec_channels * cfg.codec_vocab_size)).cpu()
        eng.close()
    return got


def test_train_steps_lower_the_loss_and_later_engines_see_the_new_weights(dev):
    from unimoe_audio_amd import train as TR
    from unimoe_audio_amd.optim import AdamW
    cfg, gm = trainable(dev)
    before_logits = first_step_logits(cfg, gm.eval(), dev)            # fills the pack caches of the OLD weights
    gm.train()
    opt = AdamW(TR.moe_param_groups(gm, weight_decay=0.01), lr=1e-3, max_grad_norm=1.0)
    assert 2 <= len(opt.param_groups) <= 16
    ids, codec, am, labels = batch(cfg)
    # step 1 by hand: the norm of the gradients that were there, in fp64 on the host
    versions = {n: p._version for n, p in gm.named_parameters()}
    w_old = {n: p.detach().clone() for n, p in gm.named_parameters()}
    loss0, _, _ = TR.forward_train(gm, ids, codec, am, labels)
    loss0.backward()
    with_grad = {n for n, p in gm.named_parameters() if p.grad is not None}
    ref_norm = float(np.sqrt(sum(float((p.grad.double() ** 2).sum()) for p in gm.parameters() if p.grad is not None)))
    opt.step()
    got = float(opt.grad_norm)
    print(f"\nGRAD NORM {got!r} vs fp64 {ref_norm!r}")
    assert ref_norm > 0.0 and abs(got - ref_norm) <= R.norm_rel_bound(opt.chunk_elems) * ref_norm
    assert int(opt.steps) == 1 and int(opt.skipped_steps) == 0
    moved = 0
    for n, p in gm.named_parameters():
        if n in with_grad:
            assert p._version > versions[n], n
            moved += int(not torch.equal(p.detach(), w_old[n]))
            st = opt.state[p]
            assert torch.equal(p.detach(), st["master"].to(torch.bfloat16)) and st["master"].dtype == torch.float32, n
    assert len(with_grad) > 40 and moved > 0.5 * len(with_grad)
    opt.zero_grad(set_to_none=False)
    losses = [float(loss0.detach())]
    for _ in range(3):
        loss, closs, auxm, gnorm = TR.train_step(gm, opt, ids, codec, am, labels)
        losses.append(float(loss))
        assert gnorm.is_cuda and float(gnorm) > 0.0
    print("LOSSES", losses)
    assert losses[-1] < losses[0] and int(opt.steps) == 4
    assert all(p.grad is not None and not p.grad.any() for n, p in gm.named_parameters() if n in with_grad)
    # an engine built after the steps decodes on the new weights: bit for bit what a fresh model loaded with them gives
    after = first_step_logits(cfg, gm.eval(), dev)
    fresh = build_model(cfg, 99)
    fresh.load_state_dict({k: v.cpu() for k, v in gm.state_dict().items()})
    ref = first_step_logits(cfg, fresh.to(dev).eval(), dev)
    assert torch.equal(after, ref) and not torch.equal(after, before_logits)


def test_scheduler_checkpoint_and_zero_grad_modes(dev):
    from unimoe_audio_amd import train as TR
    from unimoe_audio_amd.optim import AdamW

    def run(set_to_none, reload_at=None, check_finite=True, max_norm=0.05):
        cfg, gm = trainable(dev, seed=4)
        params = list(gm.parameters())
        mk = lambda: AdamW(TR.moe_param_groups(gm, weight_decay=0.01), lr=1e-3, max_grad_norm=max_norm, check_finite=check_finite)     # noqa: E731
        opt = mk()
        for s in range(4):
            if s == reload_at:
                sd = opt.state_dict()
                opt = mk()
                opt.load_state_dict(sd)
            fake_grads(params, 100 + s)
            opt.step()
            opt.zero_grad(set_to_none=set_to_none)
        torch.cuda.synchronize()
        return gm, opt

    gm_a, opt_a = run(False)
    final = lambda gm, opt: [p.detach().cpu() for p in gm.parameters()] + [opt.state[p][k].cpu() for p in gm.parameters() for k in ("master", "exp_avg", "exp_avg_sq")]      # noqa: E731
    ref = final(gm_a, opt_a)
    assert int(opt_a.steps) == 4
    for kw in (dict(set_to_none=True), dict(set_to_none=False, reload_at=2), dict(set_to_none=True, reload_at=1)):
        gm_b, opt_b = run(**kw)
        assert int(opt_b.steps) == 4, kw
        assert all(torch.equal(a, b) for a, b in zip(ref, final(gm_b, opt_b))), kw
    # the one-launch form (no norm pass) keeps its own counter on the host and the device, through a checkpoint too
    gm_c, opt_c = run(False, check_finite=False, max_norm=None)
    gm_d, opt_d = run(True, reload_at=2, check_finite=False, max_norm=None)
    assert int(opt_c.steps) == int(opt_d.steps) == 4 and bool(torch.isnan(opt_c.grad_norm))
    assert all(torch.equal(a, b) for a, b in zip(final(gm_c, opt_c), final(gm_d, opt_d)))
    # a LambdaLR schedule: the lr of the second step is the scheduled one (and the unscheduled one is rejected by the same bound)
    cfg, gm = trainable(dev, seed=4)
    opt = AdamW(list(gm.parameters()), lr=1e-3, weight_decay=0.01, max_grad_norm=0.05)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: 0.25 ** e)
    p = gm.language_model.norm.weight
    fake_grads(list(gm.parameters()), 7)
    opt.step()
    sched.step()
    assert opt.param_groups[0]["lr"] == 2.5e-4
    fake_grads(list(gm.parameters()), 8)
    st = opt.state[p]
    b = dict(w=st["master"].cpu().numpy(), m=st["exp_avg"].cpu().numpy(), v=st["exp_avg_sq"].cpu().numpy(), g=p.grad.float().cpu().numpy())
    opt.step()
    from unimoe_audio_amd.optim import RECORD_DTYPE
    rec = opt._rec.cpu().numpy().view(RECORD_DTYPE)[0]
    ratio = {}
    for lr in (2.5e-4, 1e-3):
        w1, _, _, parts = R.adamw_fp64(b["w"], b["m"], b["v"], b["g"], lr=lr, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01, clip=rec["clip"],
                                       bc1=rec["bc1"][0], bc2=rec["bc2"][0])
        bw, _, _ = R.adamw_bounds(parts, lr=lr, wd=0.01, bc1=rec["bc1"][0])
        ratio[lr] = float(np.max(np.abs(st["master"].cpu().numpy() - w1) / bw))
    print("\nSCHEDULED LR: worst error / bound", ratio)
    assert ratio[2.5e-4] <= 1.0 < ratio[1e-3]


def test_adamw_refusals_on_the_device(dev):
    from unimoe_audio_amd._lib import UmoeError
    from unimoe_audio_amd.optim import AdamW
    P = torch.nn.Parameter
    with pytest.raises(UmoeError, match="not contiguous"):
        AdamW([P(torch.zeros(8, 8, dtype=torch.bfloat16, device=dev).t())], lr=1e-3)
    p = P(torch.zeros(64, dtype=torch.bfloat16, device=dev))
    opt = AdamW([p], lr=1e-3)
    if hasattr(p, "grad_dtype"):                              # torch itself refuses a gradient of another dtype unless told otherwise
        p.grad_dtype = None
    p.grad = torch.zeros(64, dtype=torch.float32, device=dev)
    with pytest.raises(UmoeError, match="gradient of parameter 0 is torch.float32"):
        opt.step()
    p.grad = torch.zeros(128, dtype=torch.bfloat16, device=dev)[::2]
    with pytest.raises(UmoeError, match="not contiguous"):
        opt.step()
    torch.cuda.synchronize()
    assert int(opt.steps) == 0 and not p.detach().any()
    p.grad = None                                             # nothing to do: no step is counted, as in torch
    opt.step()
    assert int(opt.steps) == 0
