"""GPU tests of the fp8 (e4m3) expert weights of the decode engine (moe_flat_fp8_kernel): bit-identical to the bf16 engine run on the
dequantized weights W_deq, host-side refusals, and the accuracy cost against the unquantized model (synthetic weights)."""
import json

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from unimoe_audio_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def ref_cfg(layers=2):
    from unimoe_audio_amd.config import UniMoEAudioConfig
    return UniMoEAudioConfig(hidden_size=2048, num_hidden_layers=layers, num_attention_heads=16, num_key_value_heads=2, vocab_size=320,
                             dynamic_intermediate_size=2752, shared_intermediate_size=1376, codec_placeholder_value=300)


def build(cfg, seed, std=0.03):
    from unimoe_audio_amd.model import UniAudioRVQQwen2_5VLMoEForConditionalGeneration
    torch.manual_seed(seed)
    m = UniAudioRVQQwen2_5VLMoEForConditionalGeneration(cfg)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "layernorm" in n or n.endswith("norm.weight"):
                p.copy_(1 + 0.05 * torch.randn_like(p))
            else:
                p.normal_(0, 0.02 if n.endswith("bias") else std)
    return m.to(torch.bfloat16).eval()


def prompt(cfg, B, T, seed):
    torch.manual_seed(seed)
    ids = torch.randint(0, 290, (2 * B, T))
    am = torch.ones(2 * B, T, dtype=torch.long)
    am[0, :1] = 0
    ids[:, -5:-2] = cfg.codec_placeholder_value
    codec = torch.randint(0, 1024, (2 * B * 3, cfg.codec_channels))
    return ids, am, codec


def run_engine(m, cfg, B, fmt, steps, use_graph, dev):
    """prefill + `steps` sampled decode steps of a fresh engine -> (tokens, router masks, top-k, logits, per-layer router logits of an
    eager probe step, info)."""
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    from unimoe_audio_amd.model import DecodeEngine
    T = 12
    ids, am, codec = prompt(cfg, B, T, 4)
    eng = DecodeEngine(m, B, Lmax=T + steps + 80, Tmax=steps + 72, expert_weights=fmt)
    x = m.calculate_input_embedding(ids.to(dev), codec.to(dev))
    eng.prefill(x.reshape(-1, cfg.hidden_size).contiguous(), am.to(dev))
    pre, psteps = prepare_audio_prompt(cfg, [None] * B)
    eng.start_decode(pre, psteps, steps + 8, 4, cfg_scale=2.0, temperature=1.0, top_p=0.9, top_k=45, eos_mul=0.8, do_sample=True, seed=3)
    for _ in range(steps):
        eng.step(use_graph)
    torch.cuda.synchronize()
    E = cfg.num_experts
    out = dict(tokens=eng.tokens.cpu().clone(),
               mask=eng.copy_buffer("all_mask", torch.int32, (cfg.num_hidden_layers, 2 * B, E)).cpu(),
               topk=eng.copy_buffer("all_topk", torch.int64, (cfg.num_hidden_layers, 2 * B)).cpu(),
               logits=eng.copy_buffer("logits", torch.float32, (2 * B, cfg.codec_channels * cfg.codec_vocab_size)).cpu())
    probe = eng.set_probe(dump_logits=True)          # one eager step with the per-layer router logits dumped
    eng.step(False)
    torch.cuda.synchronize()
    out["router_logits"] = probe["logits"].cpu().clone()
    eng.set_probe()
    out["expert_fp8"] = eng.info("expert_fp8")
    out["expert_launch"] = eng.info("expert_launch")
    out["handoff"] = eng.handoff_error()
    eng.close()
    return out


def assert_same(a, b):
    for k in ("tokens", "mask", "topk", "logits", "router_logits"):
        assert torch.equal(a[k], b[k]), k


def test_device_conversion_of_every_e4m3_code_at_every_scale(dev):
    """The fp8 launch's conversion path (flat_f8_frag: v_cvt_scalef32_pk_bf16_fp8 on both words of a lane's 8 bytes, scale 2^e built from
    the exponent bits) over all 256 e4m3 codes x e in [-24, 8], against float8_e4m3fn -> float * 2^e: the same bf16 bits (the two NaN
    codes skipped).  Pins the byte order, subnormal inputs and the scale semantics at the range ends."""
    import ctypes as C
    from unimoe_audio_amd import _lib as L
    exps = torch.arange(-24, 9, dtype=torch.int8)
    N, K = exps.numel(), 256
    codes = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    q = torch.stack([codes.roll(int(r)) for r in range(N)])          # every code at every byte position of a lane's 8 bytes
    out = torch.empty(N, K, dtype=torch.int16, device=dev)
    qd, ed = q.to(dev).contiguous(), exps.to(dev).contiguous()
    fn = L.lib().umoe_fp8_convert_probe
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.check(fn(qd.data_ptr(), ed.data_ptr(), N, K, out.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "umoe_fp8_convert_probe")
    torch.cuda.synchronize()
    ref = (q.view(torch.float8_e4m3fn).float() * torch.exp2(exps.float())[:, None]).to(torch.bfloat16).view(torch.int16)
    ok = (q & 0x7F) != 0x7F
    got = out.cpu()
    assert torch.equal(got[ok], ref[ok]), int((got[ok] != ref[ok]).sum())


def test_expert_parallel_engine_refuses_fp8_layers(dev):
    """The C side refuses too (umoe_engine_set_layer_fp8 on an engine with ep_size 2), with nothing launched."""
    import ctypes as C
    import types
    from unimoe_audio_amd import _lib as L
    from unimoe_audio_amd.model import DecodeEngine
    cfg = ref_cfg()
    m = build(cfg, 31).to(dev)
    eng = DecodeEngine(m, 1, Lmax=64, Tmax=64, ep=types.SimpleNamespace(rank=0, size=2), ep_connect=False, expert_weights="bf16")
    G = cfg.mlp_dynamic_expert_num + cfg.mlp_fixed_expert_num
    t = torch.zeros(1024, dtype=torch.uint8, device=dev)
    arr = (C.c_void_p * G)(*([t.data_ptr()] * G))
    assert L.lib().umoe_engine_set_layer_fp8(eng.h, 0, arr, arr, arr, arr) != 0
    assert "expert parallel" in L.lib().umoe_last_error().decode()
    eng.close()


def test_quantized_parameters_are_exact_and_the_engine_needs_them_fresh(dev):
    from unimoe_audio_amd import _lib as L
    from unimoe_audio_amd.model import DecodeEngine
    cfg = ref_cfg()
    m = build(cfg, 31).to(dev)
    m.quantize_experts_("fp8")
    from unimoe_audio_amd.quant import dequantize_fp8_rows, expert_qe
    mod = m.language_model.layers[1].mlp.fixed_real_moe[0]
    q, e = expert_qe(mod, "down_proj")
    assert torch.equal(dequantize_fp8_rows(q.to(dev), e.to(dev)), mod.down_proj.weight.data)
    # a weight edited after quantization: the fp8 engine refuses (no launch: the refusal is in the constructor)
    with torch.no_grad():
        mod.down_proj.weight[0, 0] += 1.0
    with pytest.raises(L.UmoeError, match="changed after"):
        DecodeEngine(m, 1, Lmax=64, Tmax=64, expert_weights="fp8")


@pytest.mark.parametrize("B", [1, 3, 8])
def test_fp8_engine_is_bit_identical_to_bf16_on_the_dequantized_weights(dev, monkeypatch, B):
    """2 layers at the reference width: the fp8 flat launch against the bf16 engine on the same quantized model -- eager and graph
    replay, on the device's own schedule and on a 240-CU one: identical codes, router integers, router logits and final logits.  The fp8
    engine with the combine as a launch of its own (UMOE_FUSE_CQ=0) decodes too, bit-identical to the fp8 engine with the combine rider."""
    cfg = ref_cfg()
    m = build(cfg, 31).to(dev)
    m.quantize_experts_("fp8")
    for use_graph, cus in ((True, None), (False, None), (True, "240"), (False, "240")):
        if cus is None:
            monkeypatch.delenv("UMOE_FAKE_CUS", raising=False)
        else:
            monkeypatch.setenv("UMOE_FAKE_CUS", cus)
        a = run_engine(m, cfg, B, "bf16", 6, use_graph, dev)
        b = run_engine(m, cfg, B, "fp8", 6, use_graph, dev)
        assert a["handoff"] == 0 and b["handoff"] == 0
        assert a["expert_fp8"] == 0 and b["expert_fp8"] == 1 and b["expert_launch"] == 2
        assert_same(a, b)
        if use_graph and cus is None:
            monkeypatch.setenv("UMOE_FUSE_CQ", "0")
            c = run_engine(m, cfg, B, "fp8", 6, use_graph, dev)
            monkeypatch.delenv("UMOE_FUSE_CQ")
            assert c["handoff"] == 0 and c["expert_fp8"] == 1 and c["expert_launch"] == 2
            assert_same(b, c)


def test_fp8_engine_full_depth_is_bit_identical(dev):
    cfg = ref_cfg(36)
    m = build(cfg, 5, std=0.02).to(dev)
    m.quantize_experts_("fp8")
    a = run_engine(m, cfg, 8, "bf16", 20, True, dev)
    b = run_engine(m, cfg, 8, "fp8", 20, True, dev)
    assert b["expert_fp8"] == 1 and a["handoff"] == 0 and b["handoff"] == 0
    assert_same(a, b)
    del m
    torch.cuda.empty_cache()


@pytest.mark.parametrize("env", [{"UMOE_FLAT_MOE": "0"}, {"UMOE_FUSE_ROUTER": "0"}, {"UMOE_FAKE_CUS": "100"}])
def test_fp8_engine_refuses_every_path_but_the_flat_launch(dev, monkeypatch, env):
    """No silent fall-back to a bf16 expert path: the step is refused on the host, before anything is enqueued."""
    from unimoe_audio_amd import _lib as L
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    from unimoe_audio_amd.model import DecodeEngine
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg = ref_cfg()
    m = build(cfg, 31).to(dev)
    m.quantize_experts_("fp8")
    ids, am, codec = prompt(cfg, 2, 12, 4)
    eng = DecodeEngine(m, 2, Lmax=100, Tmax=80, expert_weights="fp8")
    eng.prefill(m.calculate_input_embedding(ids.to(dev), codec.to(dev)).reshape(-1, cfg.hidden_size).contiguous(), am.to(dev))
    pre, psteps = prepare_audio_prompt(cfg, [None] * 2)
    eng.start_decode(pre, psteps, 16, 4, cfg_scale=2.0, temperature=1.0, top_p=0.9, top_k=45, eos_mul=0.8, do_sample=True, seed=3)
    before = eng.tokens.cpu().clone()
    for use_graph in (False, True):
        with pytest.raises(L.UmoeError, match="fp8"):
            eng.step(use_graph)
    torch.cuda.synchronize()
    assert torch.equal(eng.tokens.cpu(), before) and eng.info("expert_fp8") == 0
    eng.close()


def test_fp8_accuracy_against_the_unquantized_model_is_reported(dev):
    """Teacher-forced logits of the fp8 model against the unquantized bf16 model on SYNTHETIC weights (not the checkpoint): a loose
    bound; the measured numbers are printed for the record (profiles/)."""
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    from unimoe_audio_amd.model import DecodeEngine
    cfg = ref_cfg()
    res = []
    for fmt in ("bf16", "fp8"):
        m = build(cfg, 31).to(dev)
        if fmt == "fp8":
            m.quantize_experts_("fp8")
        B, T = 4, 12
        ids, am, codec = prompt(cfg, B, T, 4)
        eng = DecodeEngine(m, B, Lmax=120, Tmax=90, expert_weights=fmt)
        eng.prefill(m.calculate_input_embedding(ids.to(dev), codec.to(dev)).reshape(-1, cfg.hidden_size).contiguous(), am.to(dev))
        pre, psteps = prepare_audio_prompt(cfg, [None] * B)
        torch.manual_seed(9)
        forced = torch.randint(0, 1024, (B, pre.shape[1] + 12, cfg.codec_channels)).to(torch.int32)
        keep = pre.to(torch.int32) != -1
        forced[:, : pre.shape[1]][keep] = pre.to(torch.int32)[keep]
        eng.start_decode(forced, psteps, 16, 6, cfg_scale=3.0, temperature=1.0, top_p=1.0, top_k=45, eos_mul=0.8, do_sample=False)
        logits = []
        for _ in range(4):
            eng.step(True)
            logits.append(eng.copy_buffer("logits", torch.float32, (2 * B, cfg.codec_channels * cfg.codec_vocab_size)).cpu())
        res.append(torch.stack(logits))
        eng.close()
        del m
        torch.cuda.empty_cache()
    rel = ((res[1] - res[0]).norm(dim=-1) / res[0].norm(dim=-1)).flatten()
    out = {"median_rel_l2": float(rel.median()), "max_rel_l2": float(rel.max()), "weights": "synthetic N(0, 0.03)"}
    print("fp8 accuracy:", json.dumps(out))
    assert out["median_rel_l2"] < 0.1 and out["max_rel_l2"] < 0.5, out      # measured 0.046 / 0.334 (synthetic weights)
