"""CPU suite of the fp8 form of the wide decode step (umoe_gemm_wide_fp8, umoe_engine_set_fp8_wide): the new C-ABI symbols, the
spill and MFMA-guard checks of every wstream_wide kernel, and the weight-stream addressing of wstream_wide_f8 restated on the host -- which
bytes of the WP8 blocks feed the MFMA of k-step i of wave w, in both stream forms -- run through the emulation of the wide kernel."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import ROOT
from test_wide_cpu import BF16, SWIGLU, emu_wide, step_cols, wide_wave_steps

bf16 = torch.bfloat16
NEW_SYMBOLS = ["umoe_gemm_wide_fp8", "umoe_engine_set_fp8_wide"]
WV = 8
# K -> (epilogue, U) of the launch that streams it in the decode step: gate/up at the hidden size, down at the two intermediate sizes
LAUNCH = {2048: (SWIGLU, 1), 2752: (BF16, 2), 1376: (BF16, 2)}


def test_new_symbols_are_exported_and_declared():
    from unimoe_audio_amd import _lib, ops
    L = ctypes.CDLL(_lib.build())
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "umoe.h")).read(), flags=re.S)
    for n in NEW_SYMBOLS:
        assert hasattr(L, n), n
        assert re.search(r"\b" + n + r"\s*\(", txt), n
        assert n in _lib.EXPORTS
    assert _lib.lib().umoe_abi_version() == 1
    assert len(_lib.STRUCT_MIRRORS) == 16          # plain scalar and pointer arguments: no new argument struct
    assert callable(ops.gemm_wide_fp8)


def test_wide_kernels_do_not_spill_and_guard_every_mfma_with_a_scalar_branch(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from scan_mfma_exec import scan
    csrc = os.path.join(ROOT, "unimoe_audio_amd", "csrc")
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found"
    out = str(tmp_path / "umoe_gemm_wide.s")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt", "--offload-arch=gfx950",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "--cuda-device-only", "-S", os.path.join(csrc, "umoe_gemm_wide.hip"),
                           "-o", out], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    # the kernel records of the code object's metadata: name and scratch bytes of every kernel
    recs = re.findall(r"\.name:\s+(\S*wstream_wide\S*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", open(out).read())
    wide = {name: int(scratch) for name, scratch in recs}
    # the instantiations of each family, by the whole kernel name (wstream_wide is a prefix of the other two): the mangled name carries the
    # name's length in front and the template arguments' "I" behind
    family = {f: sum(bool(re.search(r"\d" + f + "I", n)) for n in wide) for f in ("wstream_wide", "wstream_wide_f8", "wstream_wide_w12")}
    assert family == {"wstream_wide": 28, "wstream_wide_f8": 8, "wstream_wide_w12": 8} and len(wide) == 44, (family, len(wide))
    assert all(v == 0 for v in wide.values()), {n: v for n, v in wide.items() if v}
    n, bad = scan(out)
    assert n > 0 and not bad, bad[:3]


# ------------------------------------------------------------------------------------------------ stream addressing
def stream_form(KB, U):
    """wstream_wide_f8: k-steps per ring stage -- 2 (one 16-byte lane load) unless the launch splits in 2-step chunks and KB is odd"""
    return 1 if (U == 2 and KB % 2) else 2


def step_address(KB, U, i0, i1, i, swap_halves=False):
    """k-step i of a wave with the slice [i0, i1) -> (chunk, half, byte offset of lane 0 in the block, bytes the load brings).  The 16-byte
    form loads whole chunks, so the slice must start and end on a chunk; the 8-byte form loads the step's own half and nothing else."""
    assert i0 <= i < i1 <= KB
    cs = stream_form(KB, U)
    chunk, half = i >> 1, i & 1
    if cs == 2:
        assert i0 % 2 == 0 and i1 % 2 == 0, "a 16-byte stage would carry a k-step of the next wave (or a padded one)"
        return chunk, half, chunk * 1024 + 8 * half, 16
    if swap_halves:
        half ^= 1
    return chunk, half, chunk * 1024 + 8 * half, 8


def step_bytes(packed, NB, KB, off0):
    """the 8 bytes every lane of every block feeds to the MFMA: lane l reads at off0 + 16 l of its block -> uint8 [NB, 64, 8]"""
    KB2 = (KB + 1) // 2
    idx = off0 + 16 * torch.arange(64)[:, None] + torch.arange(8)[None, :]
    assert int(idx.max()) < KB2 * 1024
    return packed.view(NB, KB2 * 1024)[:, idx]


def dequant_through_addressing(packed, exps, NB, K, U, swap_halves=False, exp_from_quarter=False):
    """W [NB * 16, K] as the kernel sees it: every k-step of every wave read at its address, scaled by the row exponent the lane loads"""
    KB = K // 32
    W = torch.full((NB * 16, K), float("nan"))
    lane = torch.arange(64)
    sel = (lane >> 4) if exp_from_quarter else (lane & 15)
    scale = torch.exp2(exps.view(NB, 16)[:, sel].float())                                    # [NB, 64]
    seen = []
    for i0, i1 in wide_wave_steps(KB, U, WV):
        for i in range(i0, i1):
            _, _, off0, _ = step_address(KB, U, i0, i1, i, swap_halves)
            v = step_bytes(packed, NB, KB, off0).view(torch.float8_e4m3fn).float() * scale[:, :, None]          # [NB, lane = 16 h + r, 8]
            W[:, step_cols(K, [i])] = v.view(NB, 4, 16, 8).permute(0, 2, 1, 3).reshape(NB * 16, 32)
            seen.append(i)
    assert sorted(seen) == list(range(KB))                                                  # every k-step once, none padded
    return W.to(bf16)


def quantized(N, K, seed):
    from unimoe_audio_amd import quant
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g) * K ** -0.5 * torch.exp2((torch.arange(N) % 7 - 3).float())[:, None]   # exponents differ within a block
    q, e = quant.quantize_fp8_rows(w)
    assert len(set(e[:16].tolist())) > 1
    return q, e


@pytest.mark.parametrize("K", [2048, 2752, 1376])
def test_stream_addressing_reads_the_bytes_of_every_k_step(K):
    from unimoe_audio_amd import quant
    epi, U = LAUNCH[K]
    KB, NB = K // 32, 3
    assert KB in (64, 86, 43) and stream_form(KB, U) == (1 if KB == 43 else 2)
    q, e = quantized(NB * 16, K, K)
    packed, _ = quant.pack_wp8(q, e)
    if KB % 2:      # the unused half of the last chunk of every K quarter: the format says zero; nothing below may read it
        assert bool((packed.view(NB, -1, 64, 16)[:, -1, :, 8:] == 0).all())
        packed.view(NB, -1, 64, 16)[:, -1, :, 8:] = 0x7F
    for wave, (i0, i1) in enumerate(wide_wave_steps(KB, U, WV)):
        for i in range(i0, i1):
            chunk, half, off0, nbytes = step_address(KB, U, i0, i1, i)
            assert (chunk, half) == (i // 2, i % 2) and nbytes == (8 if KB % 2 else 16)
            got = step_bytes(packed, NB, KB, off0).view(NB, 4, 16, 8).permute(0, 2, 1, 3).reshape(NB * 16, 32)
            assert torch.equal(got, q[:, step_cols(K, [i])]), (K, wave, i)
    if KB == 43:    # the slice boundaries land on either half of a chunk
        assert [a for a, _ in wide_wave_steps(KB, U, WV)] + [KB] == [0, 5, 10, 16, 21, 26, 32, 37, 43]


@pytest.mark.parametrize("K", [2048, 2752, 1376])
def test_emulation_on_the_addressed_weights_equals_the_dequantized_weights(K):
    from unimoe_audio_amd import quant
    epi, U = LAUNCH[K]
    rows, N, NB = 34, 32, 2
    g = torch.Generator().manual_seed(K + 1)
    A = torch.randn(rows, K, generator=g).to(bf16)
    qe = [quantized(N, K, 10 * K + j) for j in range(2 if epi == SWIGLU else 1)]
    deq = [quant.dequantize_fp8_rows(q, e) for q, e in qe]
    if epi == SWIGLU:
        packed, exps = quant.pack_wp8_gate_up(*qe[0], *qe[1])
        split = lambda W: [W.view(NB, 2, 16, K)[:, j].reshape(N, K) for j in (0, 1)]          # blocks interleaved: 2 i gate, 2 i + 1 up
        blocks = 2 * NB
    else:
        packed, exps = quant.pack_wp8(*qe[0])
        split = lambda W: [W]
        blocks = NB
    want = emu_wide(A, deq, K, rows, epi, U, WV)
    seen = split(dequant_through_addressing(packed, exps, blocks, K, U))
    assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(seen, deq))
    assert torch.equal(emu_wide(A, seen, K, rows, epi, U, WV).view(torch.int16), want.view(torch.int16))
    # planted errors: the row exponent taken from the lane's K quarter, and (8-byte form) the halves of a chunk swapped
    wrong = split(dequant_through_addressing(packed, exps, blocks, K, U, exp_from_quarter=True))
    assert not torch.equal(emu_wide(A, wrong, K, rows, epi, U, WV).view(torch.int16), want.view(torch.int16))
    if stream_form(K // 32, U) == 1:
        wrong = split(dequant_through_addressing(packed, exps, blocks, K, U, swap_halves=True))
        assert not torch.equal(emu_wide(A, wrong, K, rows, epi, U, WV).view(torch.int16), want.view(torch.int16))
