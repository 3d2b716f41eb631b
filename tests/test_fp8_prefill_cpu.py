"""CPU suite of fp8-only expert weights: the granule addressing of tgemm_wp8_kernel restated on the host against
quant.unpack_wp8 (with planted errors that the same checker rejects), the quantize / release / dequantize round trip, loading a
checkpoint straight into fp8-only, the new C-ABI symbol, and the new kernel's instantiations compiled for gfx950 without scratch."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT
from unimoe_audio_amd import checkpoint as CK
from unimoe_audio_amd import quant
from unimoe_audio_amd.config import UniMoEAudioConfig
from unimoe_audio_amd.model import UniAudioRVQQwen2_5VLMoEForConditionalGeneration as Model

KS = [32, 96, 352, 1376, 2048]


# ------------------------------------------------------------------------------------------------ granule addressing
def granule_offset(n, k, K, swiglu_half=None, j0_bug=False, swap_gate_up=False, quarter_bug=False):
    """Byte offset in the WP8 blocks of the 8-element granule at column k of weight row n, and the index of the row's exponent -- what
    tgemm_wp8_kernel computes (umoe_tgemm_packed.hip).  swiglu_half 0 / 1: gate / up row n of an interleaved pair."""
    assert K % 32 == 0 and k % 8 == 0 and k < K
    Q, KB2 = K // 4, (K + 63) // 64
    h = k // Q
    if quarter_bug:
        h = min(3, (k + 8) // Q)            # planted: a granule at a quarter's last 8 columns goes to the next quarter
    o = k - h * Q
    i, j0 = o // 16, o % 16
    if j0_bug:
        j0 = 8 - j0                         # planted: the two granules of a 16-byte lane chunk swapped
    blk = n // 16
    if swiglu_half is not None:
        half = swiglu_half ^ 1 if swap_gate_up else swiglu_half
        blk = 2 * (n // 16) + half
    return ((blk * KB2 + i) * 64 + 16 * h + (n & 15)) * 16 + j0, blk * 16 + (n & 15)


def gather(packed, ex, N, K, **kw):
    """q [N][K] and e [N] as the kernel's addressing reads them out of the blocks (None: a read left the quarter / the blocks)"""
    q = torch.empty(N, K, dtype=torch.uint8)
    e = torch.empty(N, dtype=torch.int8)
    for n in range(N):
        for k in range(0, K, 8):
            off, ei = granule_offset(n, k, K, **kw)
            if off < 0 or off + 8 > packed.numel():
                return None, None
            q[n, k:k + 8] = packed[off:off + 8]
            e[n] = ex[ei]
    return q, e


def random_qe(N, K, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (N, K), generator=g).to(torch.uint8), torch.randint(-24, 9, (N,), generator=g).to(torch.int8)


@pytest.mark.parametrize("K", KS)
def test_granule_addressing_reads_what_unpack_wp8_reads(K):
    for N in (16, 40):                                       # 40: a last block with 8 padded rows
        q, e = random_qe(N, K, K + N)
        packed, ex = quant.pack_wp8(q, e)
        uq, ue = quant.unpack_wp8(packed, ex, N, K)
        assert torch.equal(uq, q) and torch.equal(ue, e)
        # every byte the kernel must not read is made different from what it would need
        live, _ = quant.pack_wp8(torch.ones_like(q), torch.ones_like(e))
        poisoned = torch.where(live == 0, torch.full_like(packed, 0x7F), packed)
        gq, ge = gather(poisoned, ex, N, K)
        assert torch.equal(gq, q) and torch.equal(ge, e)


@pytest.mark.parametrize("K", KS)
def test_granule_addressing_of_the_interleaved_gate_up_pair(K):
    N = 32
    (qg, eg), (qu, eu) = random_qe(N, K, K), random_qe(N, K, K + 1)
    packed, ex = quant.pack_wp8_gate_up(qg, eg, qu, eu)
    for half, (q, e) in enumerate(((qg, eg), (qu, eu))):
        gq, ge = gather(packed, ex, N, K, swiglu_half=half)
        assert torch.equal(gq, q) and torch.equal(ge, e)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("bug", ["j0_bug", "swap_gate_up", "quarter_bug"])
def test_a_planted_addressing_error_is_rejected(K, bug):
    N = 32
    (qg, eg), (qu, eu) = random_qe(N, K, K), random_qe(N, K, K + 1)
    packed, ex = quant.pack_wp8_gate_up(qg, eg, qu, eu)
    gq, ge = gather(packed, ex, N, K, swiglu_half=0, **{bug: True})
    assert gq is None or not (torch.equal(gq, qg) and torch.equal(ge, eg)), (K, bug)


# ------------------------------------------------------------------------------------------------ release / restore
def _tiny(seed=3):
    cfg = UniMoEAudioConfig.tiny()
    m = Model(cfg)
    with torch.no_grad():
        g = torch.Generator().manual_seed(seed)
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    return cfg, m.to(torch.bfloat16)


def _experts(m):
    return [x for layer in m.language_model.layers for grp in quant.expert_modules(layer) for x in grp]


def test_release_and_dequantize_round_trip_is_exact():
    from unimoe_audio_amd import _lib as L
    _, kept = _tiny()
    _, only = _tiny()
    quant.quantize_experts_(kept, "fp8")
    want = {k: v.clone() for k, v in kept.state_dict().items()}
    quant.quantize_experts_(only, "fp8", keep_bf16=False)
    assert quant.expert_format(only) == "fp8-only" and quant.is_quantized(only) and quant.is_released(only)
    for a, b in zip(_experts(kept), _experts(only)):
        assert b._fp8["shape"] == a._fp8["shape"]
        for n in ("gate_proj", "up_proj", "down_proj"):
            assert getattr(b, n).weight.numel() == 0 and getattr(b, n).weight.dtype == torch.bfloat16
        assert torch.equal(a._fp8["gu"][0], b._fp8["gu"][0]) and torch.equal(a._fp8["dn"][1], b._fp8["dn"][1])
    quant.check_quantized(only)                                # released parameters are accepted
    quant.quantize_experts_(only, "fp8", keep_bf16=False)      # idempotent
    with pytest.raises(L.UmoeError, match="dequantize_experts_"):
        only.state_dict()
    with pytest.raises(L.UmoeError, match="dequantize_experts_"):
        quant.quantize_experts_(only, "fp8")                   # the bf16 parameters are gone: not by quantizing again
    with pytest.raises(L.UmoeError, match="dequantize_experts_"):
        only.language_model.layers[0].mlp(torch.zeros(1, 2, only.config.hidden_size, dtype=torch.bfloat16))
    quant.dequantize_experts_(only)
    assert quant.expert_format(only) == "fp8" and not quant.is_released(only)
    got = only.state_dict()
    assert got.keys() == want.keys()
    for k in want:
        assert torch.equal(got[k], want[k]), k
    quant.check_quantized(only)


def test_from_pretrained_fp8_only_equals_loading_then_quantizing(tmp_path):
    cfg, src = _tiny()
    d = str(tmp_path / "ckpt")
    names = CK.save_checkpoint(src.state_dict(), d, max_shard_bytes=200_000)     # experts spread over several shards
    assert len(names) > 3
    a = Model.from_pretrained(d, config=cfg)
    quant.quantize_experts_(a, "fp8", keep_bf16=False)
    b = Model.from_pretrained(d, config=cfg, expert_weights="fp8-only")
    assert quant.expert_format(b) == "fp8-only" and quant.is_released(b)
    for x, y in zip(_experts(a), _experts(b)):
        for k in ("gu", "dn"):
            assert torch.equal(x._fp8[k][0], y._fp8[k][0]) and torch.equal(x._fp8[k][1], y._fp8[k][1])
        assert x._fp8["shape"] == y._fp8["shape"] and not hasattr(y, "_unallocated")
        assert all(p.numel() == 0 for p in y.parameters())
    quant.dequantize_experts_(a)
    quant.dequantize_experts_(b)
    sa, sb = a.state_dict(), b.state_dict()
    assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa)
    # the expert parameters never had storage before their tensor arrived
    from unimoe_audio_amd import dcmoe
    with dcmoe.unallocated_experts():
        lean = Model(cfg)
    assert all(p.numel() == 0 for x in _experts(lean) for p in x.parameters())
    assert all(x._unallocated["down_proj"] == (cfg.hidden_size, x.intermediate_size) for x in _experts(lean))
    # a checkpoint that lacks one projection of one expert cannot become fp8-only
    from safetensors.torch import load_file, save_file
    idx = os.path.join(d, CK.INDEX_NAME)
    os.remove(idx)
    victim = None
    for fn in sorted(os.listdir(d)):
        sd = load_file(os.path.join(d, fn))
        ks = [k for k in sd if k.endswith("fixed_real_moe.0.up_proj.weight")]
        if ks:
            victim = ks[0]
            del sd[victim]
            save_file(sd, os.path.join(d, fn), metadata={"format": "pt"})
            break
    assert victim
    with pytest.raises(KeyError):
        Model.from_pretrained(d, config=cfg, expert_weights="fp8-only")


# ------------------------------------------------------------------------------------------------ ABI and code generation
def test_new_symbol_is_exported_and_declared():
    from unimoe_audio_amd import _lib, ops
    L = ctypes.CDLL(_lib.build())
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "umoe.h")).read(), flags=re.S)
    assert hasattr(L, "umoe_tiled_gemm_wp8") and re.search(r"\bumoe_tiled_gemm_wp8\s*\(", txt) and "umoe_tiled_gemm_wp8" in _lib.EXPORTS
    assert _lib.lib().umoe_abi_version() == 1
    assert ctypes.sizeof(_lib.TGroup) == int(_lib.lib().umoe_struct_size(b"umoe_tgroup_t"))      # umoe_tgroup_t did not grow
    assert callable(ops.tiled_gemm_wp8)


def test_wp8_tile_kernels_compile_for_gfx950_without_scratch(tmp_path):
    csrc = os.path.join(ROOT, "unimoe_audio_amd", "csrc")
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found"
    out = str(tmp_path / "umoe_tgemm_packed.s")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt", "--offload-arch=gfx950",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "--cuda-device-only", "-S", os.path.join(csrc, "umoe_tgemm_packed.hip"),
                           "-o", out], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    txt = open(out).read()
    recs = re.findall(r"\.name:\s+(\S*tgemm_wp8_kernel\S*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)"
                      r"(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", txt)
    kern = {name: (int(s), int(v), int(sp)) for name, s, v, sp in recs}
    assert len(kern) == 4, sorted(kern)                      # SwiGLU and BF16 epilogues x 128- and 256-token tiles
    for name, (scratch, vgprs, spills) in kern.items():
        assert scratch == 0 and spills == 0, (name, scratch, spills)
        assert vgprs <= 256, (name, vgprs)                   # two workgroups of 4 waves per CU (__launch_bounds__(256, 2))
    # the conversion is the hardware's scaled e4m3 -> bf16 instruction, and the tile goes into LDS as 16-byte writes
    assert "v_cvt_scalef32_pk_bf16_fp8" in txt and ("ds_write_b128" in txt or "ds_store_b128" in txt)
