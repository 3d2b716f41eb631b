"""CPU suite of the fp8 (e4m3) expert weights: the per-row power-of-two quantizer, the WP8 packing (include/umoe.h), the fp8 schedule
of the flat expert launch (host side only) and the new ABI exports.  No kernel runs."""
import ctypes as C
import re

import pytest
import torch

from unimoe_audio_amd import _lib
from unimoe_audio_amd import quant as Q


def rows(N=48, K=2048, seed=0, std=0.02):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g) * std
    w[1] *= 1e4                               # amax > 448: a positive exponent
    w[2] *= 1e-6                              # a tiny row
    return w.to(torch.bfloat16)


def test_dequantized_weights_are_exact_in_bf16():
    q, e = Q.quantize_fp8_rows(rows())
    exact = q.view(torch.float8_e4m3fn).double() * torch.exp2(e.double())[:, None]
    assert torch.equal(Q.dequantize_fp8_rows(q, e).double(), exact)


def test_row_exponent_puts_amax_in_224_448():
    w = rows()
    q, e = Q.quantize_fp8_rows(w)
    r = w.double().abs().amax(1) / torch.exp2(e.double())
    assert bool((r > 224).all()) and bool((r <= 448).all()), r
    # ... and the quantized amax never saturates: e4m3 of |w| / 2^e is the nearest even of a value <= 448 (no NaN code)
    assert not bool(((q & 0x7F) == 0x7F).any())


def test_zero_rows_and_nonfinite_input():
    w = rows(N=20)
    w[5] = 0
    q, e = Q.quantize_fp8_rows(w)
    assert int(e[5]) == 0 and not bool(q[5].view(torch.float8_e4m3fn).float().any())
    for bad in (float("inf"), float("-inf"), float("nan")):
        w2 = w.clone()
        w2[3, 7] = bad
        with pytest.raises(ValueError):
            Q.quantize_fp8_rows(w2)


def test_quantization_is_idempotent():
    q, e = Q.quantize_fp8_rows(rows(K=1376))
    d = Q.dequantize_fp8_rows(q, e)
    q2, e2 = Q.quantize_fp8_rows(d)
    assert torch.equal(q, q2) and torch.equal(e, e2) and torch.equal(Q.dequantize_fp8_rows(q2, e2), d)


def test_rounding_is_nearest_even_without_the_casts_overflow():
    # 464 would be NaN through torch's cast; every row here is scaled first, so values land on the e4m3 grid by RNE
    w = torch.tensor([[448.0, 464.0 - 1e-3, 1.0, -3.0] + [0.0] * 28], dtype=torch.float32)
    q, e = Q.quantize_fp8_rows(w)
    d = Q.dequantize_fp8_rows(q, e).float()
    assert int(e[0]) == 1 and float(d[0, 0]) == 448.0 and torch.isfinite(d).all()


def wp8_formula(q, e):
    N, K = q.shape
    KB2, NB = (K // 32 + 1) // 2, -(-N // 16)
    out = torch.zeros(NB * KB2 * 64 * 16, dtype=torch.uint8)
    for nb in range(NB):
        for i in range(KB2):
            for lane in range(64):
                r, h = nb * 16 + (lane & 15), lane >> 4
                if r >= N:
                    continue
                base = ((nb * KB2 + i) * 64 + lane) * 16
                for j in range(16):
                    k = 16 * i + j
                    if k < K // 4:
                        out[base + j] = q[r, h * (K // 4) + k]
    ex = torch.zeros(NB * 16, dtype=torch.int8)
    ex[:N] = e
    return out, ex


@pytest.mark.parametrize("N,K", [(37, 2048), (20, 1376), (16, 1376)])
def test_wp8_packer_matches_the_layout_formula(N, K):
    q, e = Q.quantize_fp8_rows(rows(N=N, K=K, seed=N))
    p, x = Q.pack_wp8(q, e)
    rp, rx = wp8_formula(q, e)
    assert p.numel() == Q.wp8_bytes(N, K) and torch.equal(p, rp) and torch.equal(x, rx)


def test_wp8_gate_up_interleaves_blocks():
    qg, eg = Q.quantize_fp8_rows(rows(N=32, K=1376, seed=3))
    qu, eu = Q.quantize_fp8_rows(rows(N=32, K=1376, seed=4))
    p, x = Q.pack_wp8_gate_up(qg, eg, qu, eu)
    pg, xg = Q.pack_wp8(qg, eg)
    pu, xu = Q.pack_wp8(qu, eu)
    blk = pg.numel() // 2
    assert torch.equal(p.view(4, blk), torch.stack([pg.view(2, blk), pu.view(2, blk)], 1).view(4, blk))
    assert torch.equal(x.view(4, 16), torch.stack([xg.view(2, 16), xu.view(2, 16)], 1).view(4, 16))


def plan(probe, n_wg, S=16, D=2048, Id=2752, Is=1376):
    L = C.CDLL(_lib.build())
    fn = getattr(L, probe)
    fn.argtypes = [C.c_int] * 7 + [C.POINTER(C.c_double), C.c_int]
    out = (C.c_double * (3 + 9 * n_wg))()
    assert fn(n_wg, S, D, Id, Is, 8, 2, out, len(out)) == 0
    return bool(out[0]), out[1], out[2], [[int(v) for v in out[3 + 9 * j: 12 + 9 * j]] for j in range(n_wg)]


@pytest.mark.parametrize("n_wg", [256, 240, 224])
def test_fp8_plan_covers_every_pair_and_block_exactly_once(n_wg):
    ok, makespan, mean, rws = plan("umoe_moe_flat_plan_fp8_probe", n_wg)
    assert ok
    pairs = [1376 // 16] * 2 + [2752 // 16] * 8
    nxt = 0
    for j, r in enumerate(rws):
        assert r[0] == nxt and 4 <= r[1] <= 7 and r[2] == (j + 1 if j < 16 else 0)
        nxt += r[1]
    assert nxt == sum(pairs)
    cover = {g: [] for g in range(10)}
    for r in rws:
        for k in range(2):
            g, nb0, nd = r[3 + 3 * k: 6 + 3 * k]
            if nd:
                cover[g].extend(range(nb0, nb0 + nd))
    for g in range(10):
        assert sorted(cover[g]) == list(range(2048 // 16)), g
    # the fp8 model charges half the KiB per pair and block: a shorter model makespan than the bf16 plan's
    ok16, makespan16, mean16, _ = plan("umoe_moe_flat_plan_probe", n_wg)
    assert ok16 and makespan < makespan16 and mean < mean16


def test_new_abi_exports_exist_and_are_declared():
    import os
    L = C.CDLL(_lib.build())
    for name in ("umoe_engine_set_layer_fp8", "umoe_moe_flat_plan_fp8_probe", "umoe_moe_flat_plan_probe"):
        assert hasattr(L, name), name
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "umoe.h")).read()
    assert re.search(r"int umoe_engine_set_layer_fp8\(umoe_engine\* e, int layer,", hdr)
    assert "umoe_engine_set_layer_fp8" in _lib.EXPORTS
    assert len(_lib.STRUCT_MIRRORS) == 16 and _lib.lib().umoe_abi_version() == 1      # no struct grew, none was added


def test_quantize_experts_on_a_tiny_cpu_model_and_stale_weight_detection():
    from unimoe_audio_amd.config import UniMoEAudioConfig
    from unimoe_audio_amd.model import UniAudioRVQQwen2_5VLMoEForConditionalGeneration
    cfg = UniMoEAudioConfig(hidden_size=256, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, vocab_size=320,
                            dynamic_intermediate_size=128, shared_intermediate_size=64, codec_placeholder_value=300)
    torch.manual_seed(0)
    m = UniAudioRVQQwen2_5VLMoEForConditionalGeneration(cfg).to(torch.bfloat16)
    gate_before = m.language_model.layers[0].mlp.gate.weight.detach().clone()
    m.quantize_experts_("fp8")
    assert Q.is_quantized(m)
    assert torch.equal(m.language_model.layers[0].mlp.gate.weight, gate_before)     # the router gate stays bf16
    routed, shared = Q.expert_modules(m.language_model.layers[1])
    for mod in routed + shared:
        for name in ("gate_proj", "up_proj", "down_proj"):
            q, e = Q.expert_qe(mod, name)
            assert torch.equal(Q.dequantize_fp8_rows(q, e), getattr(mod, name).weight.data)
    Q.check_quantized(m)
    m.quantize_experts_("fp8")                          # idempotent: the same values again
    Q.check_quantized(m)
    with torch.no_grad():
        shared[0].up_proj.weight[3, 5] += 0.5
    with pytest.raises(_lib.UmoeError, match="changed after"):
        Q.check_quantized(m)


def test_wp8_unpack_inverts_the_packer():
    for N, K in ((37, 2048), (20, 1376)):
        q, e = Q.quantize_fp8_rows(rows(N=N, K=K, seed=K))
        q2, e2 = Q.unpack_wp8(*Q.pack_wp8(q, e), N, K)
        assert torch.equal(q, q2) and torch.equal(e, e2)


def test_fp8_engine_refuses_expert_parallel_before_touching_a_device():
    import types
    from unimoe_audio_amd.config import UniMoEAudioConfig
    from unimoe_audio_amd.model import DecodeEngine, UniAudioRVQQwen2_5VLMoEForConditionalGeneration
    cfg = UniMoEAudioConfig(hidden_size=256, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=1, vocab_size=320,
                            dynamic_intermediate_size=128, shared_intermediate_size=64, codec_placeholder_value=300)
    m = UniAudioRVQQwen2_5VLMoEForConditionalGeneration(cfg).to(torch.bfloat16)
    m.quantize_experts_("fp8")
    with pytest.raises(_lib.UmoeError, match="expert parallel"):
        DecodeEngine(m, 1, Lmax=64, Tmax=64, ep=types.SimpleNamespace(rank=0, size=2), expert_weights="fp8")
