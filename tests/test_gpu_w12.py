"""GPU tests of the WP12 expert weights of the flat expert launch (moe_flat_w12_kernel: the bf16 weights in 12 bits, lossless): the
engine on its WP12 copies is bit-identical to the engine on the WP16 packs (UMOE_FLAT_W12=0) -- on synthetic weights, with exceptions
planted where the kernel's exception cursor turns (wave and K-quarter edges, every block), and when a layer is not packable."""
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
    """2 layers at the reference width: the smallest model the flat schedule accepts (K = 2048, 8 + 2 experts of 2752 / 1376)."""
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


def run_engine(m, cfg, B, steps, use_graph, dev):
    """prefill + `steps` sampled decode steps of a fresh bf16 engine -> tokens, router masks, top-k, logits, info."""
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    from unimoe_audio_amd.model import DecodeEngine
    T = 12
    ids, am, codec = prompt(cfg, B, T, 4)
    eng = DecodeEngine(m, B, Lmax=T + steps + 80, Tmax=steps + 72, expert_weights="bf16")
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
               logits=eng.copy_buffer("logits", torch.float32, (2 * B, cfg.codec_channels * cfg.codec_vocab_size)).cpu(),
               expert_w12=eng.info("expert_w12"), expert_launch=eng.info("expert_launch"), handoff=eng.handoff_error())
    eng.close()
    return out


def assert_same(a, b):
    for k in ("tokens", "mask", "topk", "logits"):
        assert torch.equal(a[k], b[k]), k


def ab(m, cfg, B, dev, monkeypatch, want_w12=1):
    """eager and graph replay, on the device's own schedule and on a 240-CU one: WP12 against UMOE_FLAT_W12=0."""
    for use_graph, cus in ((True, None), (False, None), (True, "240"), (False, "240")):
        if cus is None:
            monkeypatch.delenv("UMOE_FAKE_CUS", raising=False)
        else:
            monkeypatch.setenv("UMOE_FAKE_CUS", cus)
        monkeypatch.setenv("UMOE_FLAT_W12", "0")
        a = run_engine(m, cfg, B, 6, use_graph, dev)
        monkeypatch.delenv("UMOE_FLAT_W12")
        b = run_engine(m, cfg, B, 6, use_graph, dev)
        assert a["handoff"] == 0 and b["handoff"] == 0
        assert a["expert_launch"] == 2 and b["expert_launch"] == 2
        assert a["expert_w12"] == 0 and b["expert_w12"] == want_w12
        assert_same(a, b)


def wave_bounds(KB):
    """first k-step of each of the 8 waves of a workgroup (flat_gateup / flat_down)"""
    return [2 * ((KB // 2 * w) // 8) for w in range(9)] if KB % 2 == 0 else [(KB * w) // 8 for w in range(9)]


def plant(W):
    """Exceptions (0, 2^-30, 8.0) in EVERY 16-row block of a row-major weight [N][K] -- so in the first and the last block of every slice,
    in gate and up blocks, and at the same k-steps in neighbouring tiles: in each of the 4 K quarters the first and the last k-step of
    one wave's K range (the wave rotates with the block) and the two edges of the quarter.  16 per block (+ the natural ones): under the cap."""
    N, K = W.shape
    KB, q, b = K // 32, K // 4, wave_bounds(K // 32)
    rows, cols = [], []
    for nb in range(N // 16):
        w, r = nb % 8, nb * 16 + (5 * nb + 3) % 16
        for h in range(4):
            for i, j in ((b[w], 0), (b[w + 1] - 1, 7), (0, 1), (KB - 1, 6)):
                rows.append(r), cols.append(h * q + i * 8 + j)
    vals = torch.tensor([0.0, 2.0 ** -30, 8.0]).repeat(len(rows) // 3 + 1)[: len(rows)].to(W.dtype)
    with torch.no_grad():
        W[torch.tensor(rows), torch.tensor(cols)] = vals


def experts(m):
    for layer in m.language_model.layers:
        for e in list(layer.mlp.dynamic_real_moe.deepspeed_moe.experts.deepspeed_experts) + list(layer.mlp.fixed_real_moe):
            yield e


@pytest.fixture(scope="module")
def models(dev):
    cfg = ref_cfg()
    plain = build(cfg, 31)
    planted = build(cfg, 32)
    for e in experts(planted):              # routed and shared experts, gate, up and down
        for lin in (e.gate_proj, e.up_proj, e.down_proj):
            plant(lin.weight.data)
    return cfg, plain.to(dev), planted.to(dev)


@pytest.mark.parametrize("B", [1, 3, 8])
def test_w12_engine_is_bit_identical_to_the_bf16_launch(dev, monkeypatch, models, B):
    cfg, plain, _ = models
    ab(plain, cfg, B, dev, monkeypatch)


@pytest.mark.parametrize("B", [1, 3, 8])
def test_w12_engine_with_planted_exceptions_is_bit_identical(dev, monkeypatch, models, B):
    from unimoe_audio_amd import w12
    cfg, _, planted = models
    pk = planted.packed_w12()
    assert all(l is not None for l in pk)
    for l in pk:                           # every block of every matrix carries its 16 planted exceptions
        for d, meta in l["gu"] + l["dn"]:
            assert int(w12.exceptions_per_block(meta).min()) >= 16
    ab(planted, cfg, B, dev, monkeypatch)


def test_layer_over_the_cap_falls_back_to_the_bf16_launch(dev, monkeypatch):
    from unimoe_audio_amd import w12
    cfg = ref_cfg()
    m = build(cfg, 33)
    sh = m.language_model.layers[1].mlp.fixed_real_moe[0]
    with torch.no_grad():
        sh.down_proj.weight[16:32, : 3] = 0          # 48 exceptions in block 1 of a shared expert's down weights of the LAST layer
    m = m.to(dev)
    pk = m.packed_w12()
    assert pk[0] is not None and pk[1] is None
    ab(m, cfg, 3, dev, monkeypatch, want_w12=0)       # ("expert_w12" speaks of the last dense layer: it ran the bf16 launch)
