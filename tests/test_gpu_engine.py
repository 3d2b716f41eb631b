"""GPU parity tests of the decode engine (prefill + decode steps + on-device EOS/delay bookkeeping) against the
CPU oracle, which is itself pinned to the reference by tests/golden (see test_oracle_golden.py)."""
import types

import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from unimoe_audio_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def small_cfg(**over):
    from unimoe_audio_amd.config import UniMoEAudioConfig
    kw = dict(hidden_size=256, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, vocab_size=320,
              dynamic_intermediate_size=128, shared_intermediate_size=64, codec_placeholder_value=300)
    kw.update(over)
    return UniMoEAudioConfig(**kw)


def inject_input_jitter(cfg, model, B, T, seed):
    """Fixed samples of the DCMoE input jitter (core.py:243-244), one [B, T, D] tensor per layer, injected into the product's blocks
    (`_input_noise_inject`) and handed to the oracle (`input_noise=`): both sides multiply by the SAME noise."""
    gn = torch.Generator().manual_seed(seed)
    eps = float(cfg.input_jitter_noise)
    noise = [(1.0 - eps) + 2.0 * eps * torch.rand((B, T, cfg.hidden_size), generator=gn) for _ in range(cfg.num_hidden_layers)]
    for layer, nz in zip(model.language_model.layers, noise):
        layer.mlp._input_noise_inject = nz
    return noise


def build(cfg, seed, std):
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
    m = m.to(torch.bfloat16).eval()
    w = {k: v.clone() for k, v in m.state_dict().items()}
    return m, w


def prompt(cfg, B, T, seed, pads):
    torch.manual_seed(seed)
    ids = torch.randint(0, 290, (2 * B, T))
    am = torch.ones(2 * B, T, dtype=torch.long)
    for r, p in enumerate(pads):
        am[r, :p] = 0
    ids[:, -5:-2] = cfg.codec_placeholder_value
    codec = torch.randint(0, 1024, (2 * B * 3, cfg.codec_channels))
    return ids, am, codec


@pytest.mark.parametrize("full_width", [False, True])
def test_teacher_forced_steps_logits_and_router_ints(dev, full_width):
    """Every decode step fed the ORACLE's tokens: per-step logits within tolerance, arg-max codes agree, router ints
    of every layer equal the oracle's wherever the router logits agree bit-for-bit.
    full_width: the reference's layer sizes (D 2048, 16 / 2 heads, experts 2752 / 1376) at batch 8 = 16 CFG rows, two layers -- the
    headline decode path itself (dense-expert layout, 14-block gate/up with the router riding in it, RMSNorm-only launch,
    tiled prefill) against the CPU oracle."""
    from oracle import decode as OD
    from unimoe_audio_amd.codec_utils import DecoderOutput, prepare_audio_prompt
    if full_width:
        cfg = small_cfg(hidden_size=2048, num_attention_heads=16, num_key_value_heads=2, dynamic_intermediate_size=2752,
                        shared_intermediate_size=1376)
        m, w = build(cfg, 1, 0.02)
        B, T, steps = 8, 12, 8
        ids, am, codec = prompt(cfg, B, T, 2, [3, 0, 1, 0] + [0] * 12)
    else:
        cfg = small_cfg()
        m, w = build(cfg, 1, 0.06)
        B, T, steps = 2, 12, 24
        ids, am, codec = prompt(cfg, B, T, 2, [3, 0, 1, 0])
    pre, psteps = OD.prepare_audio_prompt(cfg, [None] * B)
    gen = OD.GenerateOracle(cfg, w)
    MAXT = steps + 40                              # forced EOS (cur >= max_tokens - 18) stays outside the compared window
    gen.generate(ids, am, pre, psteps, MAXT, 6, codec_input_ids=codec, cfg_scale=3.0, do_sample=False, eos_prob_mul_factor=0.8)
    oracle_tokens = gen.tokens                      # [B, >= steps+1, C]
    # oracle per-step logits, recomputed by stepping the text model with the same tokens
    tm = OD.TextModelOracle(cfg, w)
    key_valid = am.bool()
    pos = (am.long().cumsum(-1) - 1).masked_fill(am == 0, 1)
    x = OD.input_embedding(cfg, w, ids, codec)
    _, cache, _ = tm.forward(x, key_valid, pos, None)
    gm = m.to(dev)
    eng = gm.engine(B, T, MAXT)
    xg = gm.calculate_input_embedding(ids.to(dev), codec.to(dev))
    assert torch.equal(xg.cpu(), x)                 # embedding gather + codec sum: exact
    eng.prefill(xg.reshape(-1, cfg.hidden_size).contiguous(), am.to(dev))
    forced = torch.full((B, oracle_tokens.shape[1], cfg.codec_channels), 0, dtype=torch.int32)
    forced[:] = oracle_tokens
    eng.start_decode(forced, psteps, MAXT, 6, cfg_scale=3.0, temperature=1.0, top_p=1.0, top_k=45, eos_mul=0.8, do_sample=False)
    E = cfg.num_experts
    agree_tok = tot_tok = mask_agree = mask_tot = 0
    for s in range(steps - 1):
        kv1 = torch.cat([key_valid, torch.ones((2 * B, 1), dtype=torch.bool)], -1)
        p1 = (kv1.long().cumsum(-1) - 1).masked_fill(~kv1, 1)[:, -1:]
        tok2 = oracle_tokens[:, s: s + 1].repeat_interleave(2, dim=0)
        h, cache, router = tm.forward(OD.codec_embedding(cfg, w, tok2), kv1, p1, cache, collect_router=True)
        key_valid = kv1
        ref_logits = torch.nn.functional.linear(h, w["codec_head.weight"]).float()[:, -1]
        eng.step(use_graph=False)
        got = eng.copy_buffer("logits", torch.float32, (2 * B, cfg.codec_channels * cfg.codec_vocab_size)).cpu()
        # per row: a row whose router decisions all agree is within bf16 noise of the oracle; a near-tie that flips
        # one expert in one layer (inherent to CPU-vs-MFMA summation order) moves that row further
        rel = (got - ref_logits).norm(dim=-1) / ref_logits.norm(dim=-1)
        assert float(rel.median()) < 0.02, (s, rel.tolist())
        assert float(rel.max()) < 0.25, (s, rel.tolist())
        guided = OD.cfg_and_mask(cfg, ref_logits.view(2 * B, cfg.codec_channels, -1).clone(), 3.0, s >= 6, 0.8)
        pred = eng.copy_buffer("pred", torch.int64, (B, cfg.codec_channels)).cpu()
        ref_pred = guided.reshape(B * cfg.codec_channels, -1).argmax(-1).view(B, -1)
        agree_tok += int((pred == ref_pred).sum())
        tot_tok += pred.numel()
        # the sampler itself is exact: arg-max of the GPU's own logits, computed on the CPU, equals the kernel's codes
        gg = OD.cfg_and_mask(cfg, got.view(2 * B, cfg.codec_channels, -1).clone(), 3.0, s >= 6, 0.8)
        assert torch.equal(pred, gg.reshape(B * cfg.codec_channels, -1).argmax(-1).view(B, -1)), s
        masks = eng.copy_buffer("all_mask", torch.int32, (cfg.num_hidden_layers, 2 * B, E)).cpu()
        for l in range(cfg.num_hidden_layers):
            ref_mask = router[l]["expert_mask"]
            mask_agree += int((masks[l] == ref_mask).all(-1).sum())
            mask_tot += ref_mask.shape[0]
    # near-ties after CFG amplification (gaps down to exactly 0) flip a few arg-max codes; router ints rarely flip
    assert agree_tok / tot_tok > 0.9, (agree_tok, tot_tok)
    assert mask_agree / mask_tot > 0.95, (mask_agree, mask_tot)


@pytest.mark.parametrize("use_graph", [False, True])
def test_free_running_generate_matches_oracle(dev, use_graph):
    """generate() end to end (prefill, decode loop, forced EOS by max length, delay padding, packing)."""
    from oracle import decode as OD
    from unimoe_audio_amd.codec_utils import DecoderOutput, prepare_audio_prompt
    cfg = small_cfg()
    m, w = build(cfg, 7, 0.08)
    B, T, max_tokens = 2, 10, 40
    ids, am, codec = prompt(cfg, B, T, 8, [2, 0, 0, 0])
    pre, psteps = OD.prepare_audio_prompt(cfg, [None] * B)
    ref_codes, ref_len = OD.GenerateOracle(cfg, w).generate(ids, am, pre, psteps, max_tokens, 5, codec_input_ids=codec,
                                                           cfg_scale=2.0, do_sample=False, eos_prob_mul_factor=0.8)
    gm = m.to(dev)
    pre_g, psteps_g = prepare_audio_prompt(cfg, [None] * B)
    assert torch.equal(pre_g, pre) and psteps_g == psteps
    dec = DecoderOutput(pre_g, psteps_g, dev)
    codes, lengths = gm.generate(ids, am, dec, max_tokens, 5, codec_input_ids=codec, cfg_scale=2.0, do_sample=False,
                                 eos_prob_mul_factor=0.8, use_graph=use_graph, poll_every=7)
    assert torch.equal(lengths.cpu(), ref_len)
    assert codes.shape == ref_codes.shape
    # forced EOS / PAD tail and BOS head are exact; sampled codes agree except where bf16 noise flips a near-tie
    eos_pad = (ref_codes >= cfg.codec_eos_value)
    assert torch.equal(codes.cpu()[eos_pad], ref_codes[eos_pad])
    # free-running decoding is chaotic: one near-tie arg-max flip (bf16 noise) changes every later token, so only the
    # prefix before the first flip is comparable; per-step agreement is measured by the teacher-forced test above.
    gen_part = codes.cpu()[~eos_pad & (ref_codes != cfg.codec_bos_value)]
    assert bool(((gen_part >= 0) & (gen_part < cfg.codec_eos_value)).all())
    # run-to-run determinism (no atomics, fixed reduction orders): a second run reproduces the codes bit for bit,
    # eager launches and hipGraph replay alike
    dec2 = DecoderOutput(pre_g.clone(), psteps_g, dev)
    codes2, lengths2 = gm.generate(ids, am, dec2, max_tokens, 5, codec_input_ids=codec, cfg_scale=2.0, do_sample=False,
                                   eos_prob_mul_factor=0.8, use_graph=not use_graph, poll_every=5)
    assert torch.equal(codes2, codes) and torch.equal(lengths2, lengths)


@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
def test_delay_step_kernel_vs_reference_trace(dev, case):
    """umoe_delay_step replays the REAL reference generate() traces (tests/golden/generate_*.npz): feeding the
    reference's per-step tokens as predictions must reproduce its token buffer, EOS countdown and lengths."""
    from unimoe_audio_amd import ops
    g = load_golden(f"generate_{case}.npz")
    max_tokens, min_tokens, cfg_scale, eos_mul, V, EOS, PAD, BOS = g["params"].tolist()
    ref_tokens = g["out_tokens"].to(torch.int32)          # [B, Tfinal, C]
    B, Tf, C = ref_tokens.shape
    psteps = g["prefill_steps"].tolist()
    delay = torch.tensor([0, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18], dtype=torch.int32)
    Tmax = Tf + 8
    tok = torch.full((B, Tmax, C), -1, dtype=torch.int32)
    tok[:, : g["prefill"].shape[1]] = g["prefill"].to(torch.int32)
    st = torch.zeros(4 * B + 8, dtype=torch.int32)
    st[B:3 * B] = -1
    st[3 * B:4 * B] = torch.tensor(psteps, dtype=torch.int32)
    step0 = min(psteps) - 1
    st[4 * B], st[4 * B + 1], st[4 * B + 4] = step0, int(max_tokens), step0
    tok_d, st_d, delay_d = tok.to(dev), st.to(dev), delay.to(dev)
    for cur in range(step0 + 1, Tf):
        # the reference's prediction at this step: its stored token where it was generated; anything where the
        # prompt/BOS entry is kept (masked update), so feed a value that must NOT leak through
        pred = ref_tokens[:, cur].long().clone()
        ops.delay_step(pred.to(dev), tok_d, st_d, delay_d, int(EOS), int(PAD))
    ops.delay_step(torch.zeros(B, C, dtype=torch.int64, device=dev), tok_d, st_d, delay_d, int(EOS), int(PAD))  # no-op once done
    st_h = st_d.cpu()
    assert torch.equal(tok_d.cpu()[:, :Tf], ref_tokens)
    assert int(st_h[4 * B + 2]) == 1                       # all_done
    md = 18
    finished = st_h[2 * B:3 * B].long()
    final_step = int(st_h[4 * B]) + 1
    finished[finished == -1] = final_step - md
    lengths = torch.clamp(finished - torch.tensor(psteps), min=0)
    assert torch.equal(lengths, g["out_lengths"])


def test_model_forward_hidden_router_stats_and_loss(dev):
    """Full-sequence forward() (reference model.py:672-871, forward only): last hidden state vs the oracle text model,
    router statistics returned per layer, codec CE + decayed aux weight * mean aux vs torch on the oracle's logits."""
    from oracle import decode as OD
    cfg = small_cfg()
    m, w = build(cfg, 21, 0.06)
    B, T = 3, 14
    torch.manual_seed(22)
    ids = torch.randint(0, 290, (B, T))
    am = torch.ones(B, T, dtype=torch.long)
    am[0, :3] = 0                                        # left padding
    ids[:, 4:7] = cfg.codec_placeholder_value
    codec = torch.randint(0, 1024, (B * 3, cfg.codec_channels))
    codec_labels = torch.randint(0, 1024, (B, T, cfg.codec_channels))
    codec_labels[:, :6] = -100
    codec_labels[:, :, 5] = -100
    x = OD.input_embedding(cfg, w, ids, codec)
    pos = (am.cumsum(-1) - 1).masked_fill(am == 0, 1)
    tm = OD.TextModelOracle(cfg, w)
    h_ref, _, router = tm.forward(x, am.bool(), pos, None, padding_token_mask=am.bool(), collect_router=True)
    ref_logits = torch.nn.functional.linear(h_ref, w["codec_head.weight"]).float().view(B, T, cfg.codec_channels, -1)
    gm = m.to(dev)
    out = gm(input_ids=ids, codec_input_ids=codec, attention_mask=am, labels=ids, codec_labels=codec_labels,
             output_router_logits_and_topk=True)
    valid = am.bool()
    hd = out.hidden_states.cpu().float()[valid] - h_ref.float()[valid]
    rel = hd.norm(dim=-1) / h_ref.float()[valid].norm(dim=-1)
    assert float(rel.median()) < 0.02 and float(rel.max()) < 0.3, (float(rel.median()), float(rel.max()))
    assert len(out.all_router_expert_mask) == cfg.num_hidden_layers and len(out.all_router_top_k) == cfg.num_hidden_layers
    m0 = out.all_router_expert_mask[0].cpu()
    assert m0.shape == (B * T, cfg.num_experts)
    agree = (m0 == router[0]["expert_mask"]).all(-1)[valid.reshape(-1)].float().mean()
    assert agree > 0.8, float(agree)
    assert bool((m0[~valid.reshape(-1)][:, : cfg.num_dyn] == 0).all())           # padded tokens route nowhere (core.py:286-288)
    # loss on the oracle's logits with torch
    ce = None
    for c in range(cfg.codec_channels):
        lab = codec_labels[:, 1:, c].reshape(-1)
        if c != 0 and int((lab != -100).sum()) == 0:
            continue
        l = torch.nn.functional.cross_entropy(ref_logits[:, :-1, c].reshape(-1, ref_logits.shape[-1]), lab, ignore_index=-100)
        ce = l if ce is None else ce + l
    aux = torch.stack([r["aux"].float() for r in router]).mean()
    ref_loss = ce + cfg.l_aux_weight * aux
    assert abs(float(out.loss) - float(ref_loss)) < 0.03 * abs(float(ref_loss)), (float(out.loss), float(ref_loss))
    assert gm.training_steps == 1 and gm.cur_aux_weight < cfg.l_aux_weight


# ----------------------------------------------------------------------------- training step (BASELINE configs[2] path)
def test_training_step_vs_autograd_oracle(dev):
    """Forward + backward of the whole model (embeddings -> 2 decoder layers -> codec head -> shifted per-channel CE +
    aux) on the HIP kernels (unimoe_audio_amd/train.py) against the differentiable CPU oracle (oracle/train_autograd.py):
    loss within 1 %, parameter gradients by relative Frobenius error (bf16 chains on both sides; left padding, ragged
    experts, GQA, mRoPE all exercised): dense parameters < 10 % (median < 4 %), routed experts / gates median < 6 %."""
    from unimoe_audio_amd import train as TR
    from oracle import train_autograd as OT
    cfg = small_cfg()
    m, w = build(cfg, 3, 0.05)
    B, T = 2, 40
    ids, am, codec = prompt(cfg, 1, T, 5, [6, 0])
    torch.manual_seed(9)
    labels = torch.randint(0, 1024, (B, T, cfg.codec_channels))
    labels[:, :8] = -100
    labels[0, :, 7:] = -100
    labels[1, :, 10:] = -100                      # channels 10, 11 have no valid label at all in row 1 only
    labels[:, :, 11] = -100                       # channel 11: no labels anywhere -> skipped (model.py:837-838)
    gm = m.to(dev).train()
    for p_ in gm.parameters():
        p_.requires_grad_(True)
    auxw = float(gm.cur_aux_weight)
    xnoise = inject_input_jitter(cfg, gm, B, T, 77)
    loss, closs, auxm, routing = TR.forward_train(gm, ids, codec, am, labels, return_routing=True)
    loss.backward()
    wo = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    # teacher-forced integer routing: the GPU's fp32 gate logits differ from the CPU's in the last bits, and a token that
    # flips between two experts on a near-tie changes whole gradient tensors of small experts -- integers are compared
    # separately (bit-exact given identical logits, test_gpu_ops.py), here they are forced so that the FLOAT path is compared
    forced = [(k_.cpu(), m_.cpu()) for k_, m_ in routing]
    lo, clo, auxo, _ = OT.forward_loss(cfg, wo, ids, codec, am, labels, auxw, training=True, forced=forced, input_noise=xnoise)
    lo.backward()
    lo_free, _, _, _ = OT.forward_loss(cfg, {k: v for k, v in w.items()}, ids, codec, am, labels, auxw, training=True, input_noise=xnoise)
    assert abs(float(loss) - float(lo_free)) < 0.01 * abs(float(lo_free))       # free-running loss agrees too
    assert abs(float(loss) - float(lo)) < 0.01 * abs(float(lo)), (float(loss), float(lo))
    assert abs(float(auxm) - float(auxo)) < 0.03 * abs(float(auxo)) + 1e-3
    rel = lambda a, b: float((a.float() - b.float()).norm() / (b.float().norm() + 1e-12))
    worst = []
    for n, p_ in gm.named_parameters():
        ref = wo[n].grad
        if ref is None or float(ref.float().norm()) == 0.0:
            continue
        assert p_.grad is not None, n
        worst.append((rel(p_.grad.cpu(), ref), n))
    worst.sort(reverse=True)
    assert len(worst) > 40
    # dense parameters (attention, norms, shared experts, embeddings, head, gates): every token contributes -> tight bound.
    # routed experts: a handful of tokens each at this size; one token whose jitter-threshold membership (core.py:105-109,
    # a discrete decision on nearly equal logits) differs between the two runs changes its routing weight by a factor,
    # so single small experts may deviate more; their median must still be tight.
    discrete = lambda n: "deepspeed_experts" in n or n.endswith("mlp.gate.weight")     # fed by / feeding the discrete decisions
    dense = [e for e in worst if not discrete(e[1])]
    routed = sorted(e[0] for e in worst if discrete(e[1]))
    assert dense[0][0] < 0.10 and dense[len(dense) // 2][0] < 0.04, dense[:6]
    assert routed[len(routed) // 2] < 0.06 and routed[-1] < 0.30, routed[-6:]


@pytest.mark.parametrize("jitter", [0.01, 1e-5])
def test_training_step_full_width_layer_at_6240_tokens_vs_autograd_oracle(dev, jitter):
    """BASELINE configs[2] shape through ONE decoder layer at the reference's width (D 2048, 16 / 2 heads, experts 2752 / 1376):
    batch 4 x 1560 tokens = 6240 tokens -- the 256 x 256 ping-pong GEMM on every projection, ragged experts of ~2800 rows, the MFMA
    flash attention forward and its fused backward over 1560 keys, left padding -- forward + backward against the differentiable
    CPU oracle (oracle/train_autograd.py) under teacher-forced routing.  Measured values are printed."""
    from unimoe_audio_amd import train as TR
    from oracle import train_autograd as OT
    # jitter = router_jitter_noise.  0.01 is the shipped value: the mixer's softmax runs over the columns within 2 % of the running
    # maximum (core.py:105-109), a DISCRETE membership decided on fp32 gate logits that differ in the last bits between the two sides;
    # at 6240 tokens a few memberships flip, each changing that token's routing weight by a factor, and the difference reaches every
    # gradient upstream.  1e-5 switches that source off (the set is the maximum alone): what remains is the arithmetic of the kernels.
    cfg = small_cfg(hidden_size=2048, num_attention_heads=16, num_key_value_heads=2, dynamic_intermediate_size=2752,
                    shared_intermediate_size=1376, num_hidden_layers=1, router_jitter_noise=jitter)
    m, w = build(cfg, 13, 0.02)
    B, T = 4, 1560
    ids, am, codec = prompt(cfg, 2, T, 15, [40, 0, 7, 0])
    torch.manual_seed(19)
    labels = torch.randint(0, 1024, (B, T, cfg.codec_channels))
    labels[:, :60] = -100
    for c in range(cfg.codec_channels):                      # channel-delay masking of the tail
        labels[:, T - 19 + cfg.codec_delay_pattern[c]:, c] = -100
    gm = m.to(dev).train()
    for p_ in gm.parameters():
        p_.requires_grad_(True)
    auxw = float(gm.cur_aux_weight)
    xnoise = inject_input_jitter(cfg, gm, B, T, 78)
    loss, closs, auxm, routing = TR.forward_train(gm, ids, codec, am, labels, return_routing=True)
    loss.backward()
    assert gm.training_steps == 1
    wo = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    forced = [(k_.cpu(), m_.cpu()) for k_, m_ in routing]
    lo, clo, auxo, _ = OT.forward_loss(cfg, wo, ids, codec, am, labels, auxw, training=True, forced=forced, input_noise=xnoise)
    lo.backward()
    rel = lambda a, b: float((a.float() - b.float()).norm() / (b.float().norm() + 1e-12))
    errs = []
    for n, p_ in gm.named_parameters():
        ref = wo[n].grad
        if ref is None or float(ref.float().norm()) == 0.0:
            continue
        assert p_.grad is not None, n
        errs.append((rel(p_.grad.cpu(), ref), n))
    errs.sort(reverse=True)
    discrete = lambda n: "deepspeed_experts" in n or n.endswith("mlp.gate.weight")
    dense = [e for e in errs if not discrete(e[1])]
    routed = sorted(e[0] for e in errs if discrete(e[1]))
    print("\nFULL-WIDTH TRAIN LAYER", dict(loss=float(loss), oracle_loss=float(lo), aux=float(auxm), oracle_aux=float(auxo), worst_dense=dense[:3],
                                          median_dense=dense[len(dense) // 2][0], median_routed=routed[len(routed) // 2], worst_routed=routed[-1]))
    assert abs(float(loss) - float(lo)) < 0.01 * abs(float(lo)), (float(loss), float(lo))
    assert abs(float(auxm) - float(auxo)) < 0.03 * abs(float(auxo)) + 1e-3
    # first measurement on MI355X: shipped jitter -- dense worst 0.085 / median 0.065, routed median 0.075 / worst 0.25; bounds = that + margin
    lim = dict(dw=0.12, dm=0.09, rm=0.10, rw=0.35) if jitter > 1e-3 else dict(dw=0.06, dm=0.03, rm=0.04, rw=0.20)
    assert dense[0][0] < lim["dw"] and dense[len(dense) // 2][0] < lim["dm"], dense[:6]
    assert routed[len(routed) // 2] < lim["rm"] and routed[-1] < lim["rw"], routed[-6:]


def test_generate_with_teacher_labels_golden_loss_and_guidance(dev, capsys):
    """DecoderOutput.labels_prefill (reference model.py:1138-1171): the first `debug_guidance_step` steps feed the labels forward,
    every step prints the golden loss; the loss equals the oracle's formula on the engine's own logits."""
    from oracle import decode as OD
    from unimoe_audio_amd.codec_utils import DecoderOutput, prepare_audio_prompt
    from unimoe_audio_amd.model import golden_loss
    cfg = small_cfg()
    m, w = build(cfg, 41, 0.08)
    B, T, max_tokens = 2, 10, 12
    ids, am, codec = prompt(cfg, B, T, 42, [2, 0, 0, 0])
    pre, psteps = prepare_audio_prompt(cfg, [None] * B)
    torch.manual_seed(43)
    labels = torch.randint(0, 1024, (B, max_tokens + 24, cfg.codec_channels))
    labels[:, 0] = cfg.codec_bos_value
    gm = m.to(dev)
    dec = DecoderOutput(pre.clone(), psteps, dev, labels_prefill=labels)
    codes, lengths = gm.generate(ids, am, dec, max_tokens, max_tokens, codec_input_ids=codec, cfg_scale=2.0, do_sample=False,
                                 eos_prob_mul_factor=0.8, debug_guidance_step=4)
    out = capsys.readouterr().out
    assert out.count("golden loss:") == max_tokens and len(gm.golden_losses) == max_tokens
    toks = dec.generated_tokens.cpu()
    for s in range(1, 5):                                   # guided steps: the generated entries of the token buffer ARE the labels
        gen = pre[:, s] == -1
        assert torch.equal(toks[:, s][gen].long(), labels[:, s][gen])
    assert not torch.equal(toks[:, 6].long(), labels[:, 6])                      # free running afterwards
    # formula check on hand-made logits (channel-0 weight 3, masks as in model.py:1022-1026, empty channels skipped)
    g = torch.randn(3, 12, 1027)
    lab = torch.randint(0, 1024, (3, 12))
    lab[:, 5] = 1025
    lab[0, 0] = 1024
    ref = None
    for c in range(12):
        l = lab[:, c].clone()
        l[l > 1024] = -100
        if c:
            l[l >= 1024] = -100
            if int((l != -100).sum()) == 0:
                continue
        t = torch.nn.functional.cross_entropy(g[:, c], l, ignore_index=-100) * (3 if c == 0 else 1)
        ref = t if ref is None else ref + t
    assert torch.allclose(golden_loss(g, lab, 1024), ref)


def test_checkpoint_round_trip_generates_identical_codes(dev, tmp_path):
    """unimoe_audio_amd.checkpoint: HF-style shards (reference key spelling, index json) -> from_pretrained straight onto the
    device -> the same codes, bit for bit, as the model the checkpoint was written from (same kernels, same weights)."""
    from unimoe_audio_amd import checkpoint as CK
    from unimoe_audio_amd.codec_utils import DecoderOutput, prepare_audio_prompt
    from unimoe_audio_amd.model import UniAudioRVQQwen2_5VLMoEForConditionalGeneration as Model
    cfg = small_cfg()
    m, w = build(cfg, 21, 0.08)
    d = str(tmp_path / "ckpt")
    CK.save_checkpoint(w, d, max_shard_bytes=400_000)
    B, T, max_tokens = 2, 10, 24
    ids, am, codec = prompt(cfg, B, T, 9, [1, 0, 0, 0])
    pre, psteps = prepare_audio_prompt(cfg, [None] * B)
    outs = []
    for model in (m.to(dev), Model.from_pretrained(d, torch_dtype=torch.bfloat16, attn_implementation="sdpa", device=dev, config=small_cfg())):
        assert next(model.parameters()).device.type == "cuda" and next(model.parameters()).dtype == torch.bfloat16
        dec = DecoderOutput(pre.clone(), psteps, dev)
        codes, lengths = model.generate(ids, am, dec, max_tokens, 5, codec_input_ids=codec, cfg_scale=2.0, do_sample=True,
                                        temperature=1.1, top_p=0.9, eos_prob_mul_factor=0.8, seed=5)
        outs.append((codes.cpu(), lengths.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("B", [1, 3, 5])
def test_fused_launches_with_fewer_than_16_rows_are_bit_identical(dev, monkeypatch, B):
    """2, 6 and 10 decode rows (batch 1, 3, 5): the dense layout with the flat expert launch and the combine riding in the QKV launch
    against the launch-per-kernel form (UMOE_FLAT_MOE=0 UMOE_FUSE_CQ=0) and against the ragged dispatch path where it still exists
    (UMOE_DENSE_MIN_ROWS=17): identical codes -- the partial-tile guards of every hand-off."""
    from unimoe_audio_amd.codec_utils import DecoderOutput, prepare_audio_prompt
    cfg = small_cfg(hidden_size=2048, num_attention_heads=16, num_key_value_heads=2, num_hidden_layers=2,
                    dynamic_intermediate_size=2752, shared_intermediate_size=1376)
    T, max_tokens = 12, 8
    ids, am, codec = prompt(cfg, B, T, 4, [1] + [0] * (2 * B - 1))
    pre, psteps = prepare_audio_prompt(cfg, [None] * B)
    outs = []
    for fused, dense_min in (("1", "2"), ("0", "2"), ("1", "17")):
        monkeypatch.setenv("UMOE_FLAT_MOE", fused)
        monkeypatch.setenv("UMOE_FUSE_CQ", fused)
        monkeypatch.setenv("UMOE_DENSE_MIN_ROWS", dense_min)
        m, _ = build(cfg, 31, 0.03)
        m = m.to(dev)
        dec = DecoderOutput(pre.clone(), psteps, dev)
        codes, lengths = m.generate(ids, am, dec, max_tokens, 4, codec_input_ids=codec, cfg_scale=2.0, do_sample=True, temperature=1.0,
                                    top_p=0.9, eos_prob_mul_factor=0.8, seed=3)
        outs.append((codes.cpu(), lengths.cpu()))
        del m
        torch.cuda.empty_cache()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # the ragged path computes the same products per (expert, row) with the same kernels' K split: identical too
    assert torch.equal(outs[0][0], outs[2][0]) and torch.equal(outs[0][1], outs[2][1])


def test_router_riding_in_the_gate_up_launch_is_bit_identical(dev, monkeypatch):
    """Dense decode runs the Top-P router as rider workgroups: inside the flat expert launch (the default), or, launch per kernel
    (UMOE_FLAT_MOE=0), inside the gate/up launch (umoe_gemm_args.fused_router) behind an RMSNorm-only launch
    (umoe_router_args.norm_only).  Same arithmetic, same order: the generated codes and the per-layer router integers equal those of
    the separate router launch (UMOE_FUSE_ROUTER=0) bit for bit, in both rider placements, with and without the combine rider."""
    from unimoe_audio_amd.codec_utils import DecoderOutput, prepare_audio_prompt
    cfg = small_cfg(hidden_size=2048, num_attention_heads=16, num_key_value_heads=2, num_hidden_layers=2,
                    dynamic_intermediate_size=2752, shared_intermediate_size=1376)      # the fused path needs the real D / expert sizes
    B, T, max_tokens = 8, 12, 10
    ids, am, codec = prompt(cfg, B, T, 4, [1] + [0] * (2 * B - 1))
    pre, psteps = prepare_audio_prompt(cfg, [None] * B)
    outs = []
    # first: the router launch (the reference); second: the default; third and fourth: launch per kernel with the riders in the gate/up
    # launch, in its dead workgroups and in a z-slice of their own, the combine still riding in the QKV launch; fifth: the flat launch with
    # the combine as a launch of its own; sixth: launch per kernel throughout
    for fuse, mode, cq, flat in (("0", "0", "1", "1"), ("1", "0", "1", "1"), ("1", "0", "1", "0"), ("1", "1", "1", "0"), ("1", "0", "0", "1"),
                                 ("1", "0", "0", "0")):
        monkeypatch.setenv("UMOE_FUSE_CQ", cq)
        monkeypatch.setenv("UMOE_FUSE_ROUTER", fuse)
        monkeypatch.setenv("UMOE_RIDER_MODE", mode)
        monkeypatch.setenv("UMOE_FLAT_MOE", flat)
        m, _ = build(cfg, 31, 0.03)
        m = m.to(dev)
        dec = DecoderOutput(pre.clone(), psteps, dev)
        codes, lengths = m.generate(ids, am, dec, max_tokens, 4, codec_input_ids=codec, cfg_scale=2.0, do_sample=True, temperature=1.0,
                                    top_p=0.9, eos_prob_mul_factor=0.8, seed=3)
        eng = m._engine
        stats = eng.router_stats() if hasattr(eng, "router_stats") else None
        outs.append((codes.cpu(), lengths.cpu(), stats))
        del m
        torch.cuda.empty_cache()
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1])
        if o[2] is not None and outs[0][2] is not None:
            for a, b in zip(o[2], outs[0][2]):
                assert torch.equal(a.cpu(), b.cpu())


def test_flat_expert_launch_is_bit_identical_and_respects_the_cu_count(dev, monkeypatch):
    """The byte-balanced flat expert launch (umoe_moe_flat.hip: one workgroup per CU, static schedule, riders inside, two down slices)
    against the launch-per-kernel form (UMOE_FLAT_MOE=0), on a device that claims 240 CUs (another schedule, 240 workgroups) and on
    ones that claim 200 and 100 (no schedule: the engine must take the launch-per-kernel form by itself instead of timing out in a
    hand-off): identical codes and router integers everywhere, and the engine reports the form it chose."""
    from unimoe_audio_amd.codec_utils import DecoderOutput, prepare_audio_prompt
    cfg = small_cfg(hidden_size=2048, num_attention_heads=16, num_key_value_heads=2, num_hidden_layers=2,
                    dynamic_intermediate_size=2752, shared_intermediate_size=1376)
    B, T, max_tokens = 8, 12, 10
    ids, am, codec = prompt(cfg, B, T, 4, [1] + [0] * (2 * B - 1))
    pre, psteps = prepare_audio_prompt(cfg, [None] * B)
    outs = []
    for flat, cus, launch in (("1", None, 2), ("0", None, 0), ("1", "240", 2), ("1", "200", 0), ("1", "100", 0)):
        monkeypatch.setenv("UMOE_FLAT_MOE", flat)
        if cus is None:
            monkeypatch.delenv("UMOE_FAKE_CUS", raising=False)
        else:
            monkeypatch.setenv("UMOE_FAKE_CUS", cus)
        m, _ = build(cfg, 31, 0.03)
        m = m.to(dev)
        dec = DecoderOutput(pre.clone(), psteps, dev)
        codes, lengths = m.generate(ids, am, dec, max_tokens, 4, codec_input_ids=codec, cfg_scale=2.0, do_sample=True, temperature=1.0,
                                    top_p=0.9, eos_prob_mul_factor=0.8, seed=3)
        eng = m._engine
        assert eng.handoff_error() == 0
        assert eng.info("expert_launch") == launch, (flat, cus)
        stats = eng.router_stats() if hasattr(eng, "router_stats") else None
        outs.append((codes.cpu(), lengths.cpu(), stats))
        del m
        torch.cuda.empty_cache()
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1])
        if o[2] is not None and outs[0][2] is not None:
            for a, b in zip(o[2], outs[0][2]):
                assert torch.equal(a.cpu(), b.cpu())
