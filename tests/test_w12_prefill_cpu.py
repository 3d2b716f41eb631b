"""CPU suite of w12-only expert weights: the granule addressing of tgemm_w12_kernel restated on the host against w12.pack /
w12.unpack (with planted errors that the same checker rejects), the release / dequantize round trip (bit for bit, special values
included), a layer over the exception cap, loading a checkpoint straight into w12-only, the new C-ABI symbol, and the new kernel's
instantiations compiled for gfx950 without scratch and without an EXEC-predicated MFMA."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import ROOT
from unimoe_audio_amd import checkpoint as CK
from unimoe_audio_amd import quant, w12
from unimoe_audio_amd.config import UniMoEAudioConfig
from unimoe_audio_amd.model import UniAudioRVQQwen2_5VLMoEForConditionalGeneration as Model

SHAPES = [(32, 64), (48, 1376), (64, 2048)]      # KB 2 (2-step chunks), 43 (1-step chunks, Q = 344), 64


# ------------------------------------------------------------------------------------------------ granule addressing
def granule(n, k, K, swiglu_half=None, swap_steps=False, force_cs=None, quarter_bug=False):
    """What tgemm_w12_kernel computes (umoe_tgemm_packed.hip) for the 8-element granule at column k of weight row n: (byte offset of its 8
    low bytes, byte offset of its code word, word index of its block's window base).  swiglu_half 0 / 1: gate / up row n of an
    interleaved pair.  The nibble of element j of the granule: byte (0, 1, 0, 1, 2, 3, 2, 3)[j] of the code word, high half for j in
    (2, 3, 6, 7) (nibble())."""
    assert K % 32 == 0 and k % 8 == 0 and k < K
    KB, Q = K // 32, K // 4
    CS = (2 if KB % 2 == 0 else 1) if force_cs is None else force_cs      # planted: an odd-KB block read as 2-step chunks
    h = k // Q
    if quarter_bug:
        h = min(3, (k + 8) // Q)            # planted: a granule at a quarter's last 8 columns is taken from the next quarter
    i = (k - h * Q) // 8
    if swap_steps and CS == 2:
        i ^= 1                              # planted: the two k-steps of a chunk swapped
    blk = n // 16 if swiglu_half is None else 2 * (n // 16) + swiglu_half
    lane = 16 * h + (n & 15)
    u = ((i // CS) * 64 + lane) * CS + i % CS
    base = blk * KB * 768
    return base + u * 8, base + KB * 512 + u * 4, blk * w12.META + w12.META - 1


def nibble(word_bytes, j):
    b = word_bytes[(0, 1, 0, 1, 2, 3, 2, 3)[j]]
    return (b >> 4) if j in (2, 3, 6, 7) else (b & 0xF)


def rebuild(data, meta, N, K, exceptions=True, **kw):
    """The row-major int16 matrix [N][K] as the kernel's addressing and arithmetic rebuild it out of the packed bytes (None: a read left
    the blocks); exceptions patched from the records re-keyed by column"""
    d = data.tolist()
    m = (meta.to(torch.int64) & 0xFFFFFFFF).tolist()
    out = torch.empty(N, K, dtype=torch.int32)
    for n in range(N):
        for k in range(0, K, 8):
            lo, co, wi = granule(n, k, K, **kw)
            if lo < 0 or i_end(lo, co) > len(d) or wi >= len(m):
                return None
            wb = m[wi] & 0xFF
            for j in range(8):
                c = nibble(d[co:co + 4], j)
                out[n, k + j] = ((((c & 8) << 4) | ((c & 7) + wb)) << 8) | d[lo + j]
    if exceptions:
        half = kw.get("swiglu_half")
        for blk in range(len(m) // w12.META):
            if half is not None and (blk & 1) != half:
                continue
            for en in m[blk * w12.META: blk * w12.META + w12.CAP]:
                if en == w12.SENTINEL:
                    break
                n, k, v = entry_column(en, blk if half is None else blk // 2, K)
                out[n, k] = v
    return torch.where(out >= 0x8000, out - 0x10000, out).to(torch.int16)


def i_end(lo, co):
    return max(lo + 8, co + 4)


def entry_column(en, row_block, K):
    """(weight row, column, bf16 bits) of a record entry: k-step << 25 | lane << 19 | element << 16 | bits -- the kernel's re-keying"""
    ks, lane, j = en >> 25, (en >> 19) & 63, (en >> 16) & 7
    return 16 * row_block + (lane & 15), (lane >> 4) * (K // 4) + 8 * ks + j, en & 0xFFFF


def random_rows(N, K, seed, special=True):
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn(N, K, generator=g) * 0.02).to(torch.bfloat16)
    if special:
        Q = K // 4
        for x, (n, k) in enumerate([(0, 0), (N - 1, K - 1), (3, Q - 1), (3, Q), (17, 2 * Q - 8), (17, 2 * Q + 7), (N - 2, 3 * Q - 1), (N - 2, 3 * Q), (5, 8), (5, 9)]):
            W[n % N, k] = (0.0, -0.0, 2.0 ** -30, 8.0, float("inf"), -float("inf"), 2.0 ** -130)[x % 7]
    return W


@pytest.mark.parametrize("N,K", SHAPES)
def test_granule_addressing_rebuilds_the_row_major_matrix(N, K):
    W = random_rows(N, K, N + K)
    p = w12.pack(w12.wp16_from_rows(W), K // 32)
    assert p is not None and int(w12.exceptions_per_block(p[1]).max()) > 0
    got = rebuild(p[0], p[1], N, K)
    assert got is not None and torch.equal(got, W.view(torch.int16))
    assert not torch.equal(rebuild(p[0], p[1], N, K, exceptions=False), W.view(torch.int16))      # (the exceptions matter)
    assert torch.equal(w12.rows_from_wp16(w12.unpack(p[0], p[1], K // 32), N, K).view(torch.int16), W.view(torch.int16))


def test_granule_addressing_at_the_production_down_width():
    N, K = 32, 2752
    W = random_rows(N, K, 5)
    p = w12.pack(w12.wp16_from_rows(W), K // 32)
    assert torch.equal(rebuild(p[0], p[1], N, K), W.view(torch.int16))


@pytest.mark.parametrize("N,K", SHAPES[:2])
def test_granule_addressing_of_the_interleaved_gate_up_pair(N, K):
    Wg, Wu = random_rows(N, K, K), random_rows(N, K, K + 1)
    p = w12.pack(w12.wp16_gate_up(Wg, Wu), K // 32)
    assert p is not None
    for half, W in enumerate((Wg, Wu)):
        assert torch.equal(rebuild(p[0], p[1], N, K, swiglu_half=half), W.view(torch.int16)), half
    assert not torch.equal(rebuild(p[0], p[1], N, K, swiglu_half=1), Wg.view(torch.int16))


def test_granule_offsets_window_base_and_nibbles_at_the_edges():
    """spot values: both chunk forms, the quarter edges, the block interleave"""
    # KB 2 (K = 64, Q = 16, CS 2): column 8 of row 1 is k-step 1 of quarter 0 -> u = (0 * 64 + 1) * 2 + 1
    assert granule(1, 8, 64) == (3 * 8, 2 * 512 + 3 * 4, 39)
    # the first granule of quarter 1: lane 16 + 1
    assert granule(1, 16, 64) == (34 * 8, 2 * 512 + 34 * 4, 39)
    # KB 43 (K = 1376, Q = 344, CS 1): the last granule of quarter 0 (k-step 42) and the first of quarter 1 (k-step 0), row 17 (block 1, lane 1 / 17)
    b = 43 * 768
    assert granule(17, 336, 1376) == (b + (42 * 64 + 1) * 8, b + 43 * 512 + (42 * 64 + 1) * 4, 79)
    assert granule(17, 344, 1376) == (b + 17 * 8, b + 43 * 512 + 17 * 4, 79)
    # SwiGLU: gate row 17 in block 2, up row 17 in block 3
    assert granule(17, 0, 64, swiglu_half=0)[2] == 2 * 40 + 39 and granule(17, 0, 64, swiglu_half=1)[2] == 3 * 40 + 39
    assert granule(17, 0, 64, swiglu_half=1)[0] == 3 * 2 * 768 + 1 * 2 * 8
    assert [nibble([0x21, 0x43, 0x65, 0x87], j) for j in range(8)] == [1, 3, 2, 4, 5, 7, 6, 8]


@pytest.mark.parametrize("bug,N,K", [("swap_steps", 32, 64), ("swap_steps", 64, 2048), ("force_cs", 48, 1376), ("quarter_bug", 32, 64),
                                     ("quarter_bug", 48, 1376), ("quarter_bug", 64, 2048)])
def test_a_planted_addressing_error_is_rejected(bug, N, K):
    W = random_rows(N, K, N + K, special=False)
    p = w12.pack(w12.wp16_from_rows(W), K // 32)
    got = rebuild(p[0], p[1], N, K, **{bug: 2 if bug == "force_cs" else True})
    assert got is None or not torch.equal(got, W.view(torch.int16)), (bug, K)


# ------------------------------------------------------------------------------------------------ release / restore
def _tiny(seed=3, **over):
    cfg = UniMoEAudioConfig.tiny(**over)
    m = Model(cfg)
    with torch.no_grad():
        g = torch.Generator().manual_seed(seed)
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    return cfg, m.to(torch.bfloat16)


def _experts(m):
    return [x for layer in m.language_model.layers for grp in quant.expert_modules(layer) for x in grp]


def _bits(sd):
    return {k: (v.view(torch.int16) if v.dtype == torch.bfloat16 else v).clone() for k, v in sd.items()}


def _plant_specials(m):
    with torch.no_grad():
        x = _experts(m)
        x[0].gate_proj.weight[0, 0] = 0.0
        x[0].gate_proj.weight[1, 5] = -0.0
        x[0].up_proj.weight[17, 33] = 2.0 ** -130           # a denormal
        x[1].down_proj.weight[3, 7] = float("inf")
        x[1].down_proj.weight[4, 7] = -float("inf")
        x[-1].up_proj.weight[2, 2] = 8.0                     # an outlier
        x[-1].down_proj.weight[127, 63] = 2.0 ** -30


def test_release_and_dequantize_round_trip_is_bit_for_bit():
    from unimoe_audio_amd import _lib as L
    _, m = _tiny()
    _plant_specials(m)
    want = _bits(m.state_dict())
    assert torch.equal(want["language_model.layers.0.mlp.dynamic_real_moe.deepspeed_moe.experts.deepspeed_experts.0.gate_proj.weight"][1, 5],
                       torch.tensor(-32768, dtype=torch.int16))
    quant.quantize_experts_(m, "w12", keep_bf16=False)
    assert quant.expert_format(m) == "w12-only" and quant.is_released(m) and not quant.is_quantized(m)
    assert m._expert_weights == "w12-only"
    for x in _experts(m):
        for n in ("gate_proj", "up_proj", "down_proj"):
            assert getattr(x, n).weight.numel() == 0 and getattr(x, n).weight.dtype == torch.bfloat16
        assert x._w12["gu"][0].dtype == torch.uint8 and x._w12["dn"][1].dtype == torch.int32
    quant.quantize_experts_(m, "w12", keep_bf16=False)         # idempotent
    with pytest.raises(L.UmoeError, match="dequantize_experts_"):
        m.state_dict()
    with pytest.raises(L.UmoeError, match="dequantize_experts_"):
        m.language_model.layers[0].mlp(torch.zeros(1, 2, m.config.hidden_size, dtype=torch.bfloat16))
    with pytest.raises(L.UmoeError, match="dequantize_experts_"):
        m.text_forward(torch.zeros(1, 2, m.config.hidden_size, dtype=torch.bfloat16))
    with pytest.raises(L.UmoeError, match="dequantize_experts_"):
        quant.quantize_experts_(m, "fp8")
    # the released blocks build no expert WP16 packs, and packed_w12() would hand the engine the copies made at release time
    for layer in m.language_model.layers:
        pk = layer.mlp.prepare()
        assert pk["released"] and pk["exp_gu"] == [] and pk["sh_dn"] == []
        c = quant.w12_layer_copies(layer)
        assert c is not None and c["gu"][0][0] is quant.expert_modules(layer)[0][0]._w12["gu"][0]
    quant.dequantize_experts_(m)
    assert quant.expert_format(m) == "bf16" and not quant.is_released(m) and not any(hasattr(x, "_w12") for x in _experts(m))
    got = _bits(m.state_dict())
    assert got.keys() == want.keys()
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_w12_with_keep_bf16_raises():
    from unimoe_audio_amd import _lib as L
    _, m = _tiny()
    with pytest.raises(L.UmoeError, match="nothing to do"):
        quant.quantize_experts_(m, "w12", keep_bf16=True)
    with pytest.raises(L.UmoeError, match="nothing to do"):
        m.quantize_experts_("w12")
    assert quant.expert_format(m) == "bf16" and not quant.is_released(m)


def test_a_layer_over_the_cap_keeps_its_parameters():
    _, m = _tiny()
    with torch.no_grad():
        w = m.language_model.layers[1].mlp.fixed_real_moe[1].down_proj.weight      # the LAST expert of the layer: the others were released first
        w[16:18, :17] = 0.0                                                         # 34 zeros in one 16-row block
    want = _bits(m.state_dict())
    assert w12.pack(w12.wp16_from_rows(w.detach()), w.shape[1] // 32) is None
    quant.quantize_experts_(m, "w12", keep_bf16=False)
    l0, l1 = m.language_model.layers
    assert all(p.numel() == 0 for grp in quant.expert_modules(l0) for x in grp for p in x.parameters())
    assert all(p.numel() > 0 and not hasattr(x, "_w12") for grp in quant.expert_modules(l1) for x in grp for p in x.parameters())
    assert quant.w12_layer_copies(l0) is not None and quant.w12_layer_copies(l1) is None
    assert quant.expert_format(m) == "w12-only" and quant.is_released(m) and not quant.is_released(l1.mlp)
    sd1 = _bits(l1.state_dict())                               # the kept layer saves, bit for bit
    for k, v in sd1.items():
        assert torch.equal(v, want["language_model.layers.1." + k]), k
    quant.dequantize_experts_(m)
    got = _bits(m.state_dict())
    assert all(torch.equal(got[k], want[k]) for k in want)


def test_from_pretrained_w12_only_equals_loading_then_releasing(tmp_path):
    cfg, src = _tiny()
    _plant_specials(src)
    d = str(tmp_path / "ckpt")
    names = CK.save_checkpoint(src.state_dict(), d, max_shard_bytes=200_000)     # experts spread over several shards
    assert len(names) > 3
    a = Model.from_pretrained(d, config=cfg)
    quant.quantize_experts_(a, "w12", keep_bf16=False)
    b = Model.from_pretrained(d, config=cfg, expert_weights="w12-only")
    assert quant.expert_format(b) == "w12-only" and quant.is_released(b)
    for x, y in zip(_experts(a), _experts(b)):
        for k in ("gu", "dn"):
            assert torch.equal(x._w12[k][0], y._w12[k][0]) and torch.equal(x._w12[k][1], y._w12[k][1])
        assert x._w12["shape"] == y._w12["shape"] and not hasattr(y, "_unallocated")
        assert all(p.numel() == 0 for p in y.parameters())
    quant.dequantize_experts_(a)
    quant.dequantize_experts_(b)
    sa, sb, ss = _bits(a.state_dict()), _bits(b.state_dict()), _bits(src.state_dict())
    assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) and torch.equal(sa[k], ss[k]) for k in sa)


def test_copies_follow_a_model_that_moved_after_the_release():
    """The WP12 copies sit in a plain dict on the expert modules, which nn.Module.to() does not move: w12_layer_copies(layer, device)
    (what packed_w12() hands the engine) moves them, once, in the module's own store.  (The "meta" device: no GPU needed.)"""
    _, m = _tiny()
    quant.quantize_experts_(m, "w12", keep_bf16=False)
    layer = m.language_model.layers[0]
    c = quant.w12_layer_copies(layer)
    assert all(t.device.type == "cpu" for k in ("gu", "dn") for pr in c[k] for t in pr)
    moved = quant.w12_layer_copies(layer, torch.device("meta"))
    assert all(t.device.type == "meta" for k in ("gu", "dn") for pr in moved[k] for t in pr)
    assert all(t.device.type == "meta" for x in quant.expert_modules(layer)[0] + quant.expert_modules(layer)[1] for k in ("gu", "dn") for t in x._w12[k])
    again = quant.w12_layer_copies(layer, torch.device("meta"))
    assert all(p is q for k in ("gu", "dn") for pr, qr in zip(moved[k], again[k]) for p, q in zip(pr, qr))      # moved once
    other = m.language_model.layers[1]
    assert all(t.device.type == "cpu" for k in ("gu", "dn") for pr in quant.w12_layer_copies(other)[k] for t in pr)


def test_an_engine_asked_for_w12_only_on_a_model_that_was_not_released_is_refused():
    from unimoe_audio_amd import _lib as L
    from unimoe_audio_amd.model import DecodeEngine
    _, m = _tiny()
    with pytest.raises(L.UmoeError, match="keep_bf16=False"):
        DecodeEngine(m, 2, Lmax=64, Tmax=64, expert_weights="w12-only")


# ------------------------------------------------------------------------------------------------ ABI and code generation
def test_new_symbol_is_exported_and_declared():
    from unimoe_audio_amd import _lib, ops
    L = ctypes.CDLL(_lib.build())
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "umoe.h")).read(), flags=re.S)
    assert hasattr(L, "umoe_tiled_gemm_w12") and re.search(r"\bumoe_tiled_gemm_w12\s*\(", txt) and "umoe_tiled_gemm_w12" in _lib.EXPORTS
    assert _lib.lib().umoe_abi_version() == 1
    assert ctypes.sizeof(_lib.TGroup) == int(_lib.lib().umoe_struct_size(b"umoe_tgroup_t"))      # umoe_tgroup_t did not grow
    assert callable(ops.tiled_gemm_w12)


def test_w12_tile_kernels_compile_for_gfx950_without_scratch_or_predicated_mfma(tmp_path):
    csrc = os.path.join(ROOT, "unimoe_audio_amd", "csrc")
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found"
    out = str(tmp_path / "umoe_tgemm_packed.s")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt", "--offload-arch=gfx950",
                        "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "--cuda-device-only", "-S", os.path.join(csrc, "umoe_tgemm_packed.hip"),
                        "-Rpass-analysis=kernel-resource-usage", "-o", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    # the compiler's own resource remarks, one block per kernel of the file (the WP8 kernels live beside the WP12 ones): four kernels of
    # each family, no scratch, no spill, two workgroups of 4 waves per CU
    blocks = {b.split()[0]: b for b in r.stdout.split("Function Name: ")[1:]}
    assert sum(bool(re.search(r"\dtgemm_w12_kernelI", n)) for n in blocks) == 4, sorted(blocks)     # SwiGLU and BF16 epilogues x 128- and 256-token tiles
    assert sum(bool(re.search(r"\dtgemm_wp8_kernelI", n)) for n in blocks) == 4 and len(blocks) == 8, sorted(blocks)
    for n, b in blocks.items():
        assert [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", b)] == [0], (n, b)
        assert [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", b)] == [0] and [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", b)] == [0], (n, b)
        occ = re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", b)
        assert len(occ) == 1 and int(occ[0]) >= 2, (n, b)
    txt = open(out).read()
    recs = re.findall(r"\.name:\s+(\S*tgemm_w12_kernel\S*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)"
                      r"(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", txt)
    kern = {name: (int(s), int(v), int(sp)) for name, s, v, sp in recs}
    assert len(kern) == 4, sorted(kern)
    for name, (scratch, vgprs, spills) in kern.items():
        assert scratch == 0 and spills == 0 and vgprs <= 256, (name, scratch, vgprs, spills)
    # the rebuild is byte permutes, the tile goes into LDS as 16-byte writes, an exception as a 2-byte one
    assert "v_perm_b32" in txt and ("ds_write_b128" in txt or "ds_store_b128" in txt) and ("ds_write_b16" in txt or "ds_store_b16" in txt)
    scan = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "scan_mfma_exec.py"), out], stdout=subprocess.PIPE, text=True, timeout=120)
    # (32 MFMAs per kernel: 128 in the four WP12 kernels, as many in the four WP8 kernels of the file)
    assert scan.returncode == 0 and " 0 under s_and_saveexec" in scan.stdout and "256 MFMA" in scan.stdout, scan.stdout
    for name in kern:
        assert txt.split("\n" + name + ":")[1].split(".Lfunc_end")[0].count("v_mfma") == 32, name
