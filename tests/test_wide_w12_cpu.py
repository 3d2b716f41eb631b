"""CPU suite of the WP12 form of the wide decode step (umoe_gemm_wide_w12, umoe_engine_set_w12_wide): the new C-ABI symbols, the
scratch / spill / MFMA-guard checks of every wstream_wide_w12 kernel, and the weight-stream addressing of the kernel restated on the host --
which low bytes, which code word and which record word feed the MFMA of k-step i of wave w, in both chunk forms and for both U, with the
exception cursor starting at the wave's i0 -- run through the emulation of the wide kernel (test_wide_cpu.emu_wide)."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import ROOT
from test_wide_cpu import BF16, SWIGLU, emu_wide, step_cols, wide_wave_steps

bf16 = torch.bfloat16
NEW_SYMBOLS = ["umoe_gemm_wide_w12", "umoe_engine_set_w12_wide"]
WV = 8
# K -> (epilogue, U) of the launch that streams it in the decode step: gate/up at the hidden size, down at the two intermediate sizes
LAUNCH = {2048: (SWIGLU, 1), 2752: (BF16, 2), 1376: (BF16, 2)}


def test_new_symbols_are_exported_and_declared():
    from unimoe_audio_amd import _lib, ops
    from unimoe_audio_amd.model import DecodeEngine
    L = ctypes.CDLL(_lib.build())
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "umoe.h")).read(), flags=re.S)
    for n in NEW_SYMBOLS:
        assert hasattr(L, n), n
        assert re.search(r"\b" + n + r"\s*\(", txt), n
        assert n in _lib.EXPORTS
    assert _lib.lib().umoe_abi_version() == 1
    assert len(_lib.STRUCT_MIRRORS) == 16          # plain scalar and pointer arguments: no new argument struct
    assert callable(ops.gemm_wide_w12)
    assert _lib.lib().umoe_gemm_wide_w12.argtypes is not None and _lib.lib().umoe_engine_set_w12_wide.argtypes is not None
    assert inspect.signature(DecodeEngine.__init__).parameters["w12_wide"].default is False


def test_w12_wide_kernels_have_no_scratch_no_spill_and_guard_every_mfma_with_a_scalar_branch(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from scan_mfma_exec import scan
    csrc = os.path.join(ROOT, "unimoe_audio_amd", "csrc")
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found"
    out = str(tmp_path / "umoe_gemm_wide.s")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt", "--offload-arch=gfx950",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "--cuda-device-only", "-S", os.path.join(csrc, "umoe_gemm_wide.hip"),
                           "-o", out], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    # the kernel records of the code object's metadata: name, scratch bytes, VGPRs and spilled VGPRs of every kernel
    recs = re.findall(r"\.name:\s+(\S*wstream_wide_w12\S*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n"
                      r"\s+\.vgpr_spill_count:\s+(\d+)", open(out).read())
    kernels = {name: (int(scratch), int(vgprs), int(spill)) for name, scratch, vgprs, spill in recs}
    # (gate/up, down) x (two tiles, three or four tiles) x (ring refilled or not)
    assert len(kernels) == 8, sorted(kernels)
    for name, (scratch, vgprs, spill) in kernels.items():
        assert scratch == 0 and spill == 0 and 0 < vgprs <= 256, (name, scratch, vgprs, spill)
    n, bad = scan(out)
    assert n > 0 and not bad, bad[:3]


# ------------------------------------------------------------------------------------------------ stream addressing
def stream_form(KB, U):
    """wstream_wide_w12: k-steps per ring stage -- 2 (16 low bytes + 8 code bytes per lane) unless the launch splits in 2-step chunks and KB
    is odd (8 + 4 bytes); the packer chunks the same way (w12.steps_per_chunk)"""
    return 1 if (U == 2 and KB % 2) else 2


def step_address(KB, U, i0, i1, i, lane, swap_steps=False):
    """k-step i of a wave with the slice [i0, i1), lane l -> (byte offset of its 8 low bytes in the block, byte offset of its code word in
    the block, word of the block record the lane holds)"""
    assert i0 <= i < i1 <= KB and 0 <= lane < 64
    cs = stream_form(KB, U)
    rec = min(lane, 39)
    if cs == 2:
        assert i0 % 2 == 0 and i1 % 2 == 0, "a 2-step stage would carry a k-step of the next wave"
        c, s = i >> 1, i & 1
        if swap_steps:
            s ^= 1
        return (c * 64 + lane) * 16 + 8 * s, KB * 512 + (c * 64 + lane) * 8 + 4 * s, rec
    return (i * 64 + lane) * 8, KB * 512 + (i * 64 + lane) * 4, rec


def rebuild_through_addressing(data, meta, NB, K, U, swap_steps=False, cursor_from_zero=False):
    """W [NB * 16, K] (bf16) as the kernel sees it: every k-step of every wave read at its addresses, decoded with the block's window base,
    and patched from the record by a cursor that starts at the first entry of a k-step >= the wave's i0 and only ever advances past
    entries of the k-step under the MFMA (flat_w12_cursor / flat_w12_patch)"""
    from unimoe_audio_amd import w12
    KB = K // 32
    assert w12.steps_per_chunk(KB) == stream_form(KB, U)
    blocks = data.view(NB, KB * 768).to(torch.int64)
    rec_all = meta.view(NB, w12.META).to(torch.int64) & 0xFFFFFFFF
    W = torch.full((NB * 16, K), -1, dtype=torch.int64)
    lanes = torch.arange(64)
    seen = []
    for i0, i1 in wide_wave_steps(KB, U, WV):
        # the record as the wave's lanes hold it, gathered through the lane -> word map
        word = torch.tensor([step_address(KB, U, i0, i1, i0, int(l))[2] for l in lanes]) if i1 > i0 else None
        cur = [0] * NB
        if i1 > i0 and not cursor_from_zero:
            for nb in range(NB):
                held = rec_all[nb][word]                                                    # lane l = word min(l, 39)
                cur[nb] = int(((held >> 25) < i0)[:33].sum())                               # (sorted by k-step; lanes 0..32 vote)
        for i in range(i0, i1):
            addr = [step_address(KB, U, i0, i1, i, int(l), swap_steps) for l in lanes]
            lo_off = torch.tensor([a[0] for a in addr])[:, None] + torch.arange(8)[None, :]
            cw_off = torch.tensor([a[1] for a in addr])[:, None] + torch.arange(4)[None, :]
            assert int(lo_off.max()) < KB * 512 <= int(cw_off.min()) and int(cw_off.max()) < KB * 768
            lo = blocks[:, lo_off]                                                          # [NB, 64, 8]
            cb = blocks[:, cw_off]                                                          # [NB, 64, 4]
            l4, h4 = cb & 0xF, cb >> 4
            code = torch.stack([l4[..., 0], l4[..., 1], h4[..., 0], h4[..., 1], l4[..., 2], l4[..., 3], h4[..., 2], h4[..., 3]], -1)
            wb = rec_all[:, w12.META - 1].view(NB, 1, 1)
            v = ((((code & 8) << 4) | ((code & 7) + wb)) << 8) | lo
            for nb in range(NB):
                while int(rec_all[nb, cur[nb]] >> 25) == i:                                 # the scalar compare, then the patch loop
                    en = int(rec_all[nb, cur[nb]])
                    v[nb, (en >> 19) & 63, (en >> 16) & 7] = en & 0xFFFF
                    cur[nb] += 1
            W[:, step_cols(K, [i])] = v.view(NB, 4, 16, 8).permute(0, 2, 1, 3).reshape(NB * 16, 32)
            seen.append(i)
    assert sorted(seen) == list(range(KB))                                                  # every k-step once, none padded
    return torch.where(W >= 0x8000, W - 0x10000, W).to(torch.int16).view(bf16)


def planted(N, K, seed):
    """N(0, 0.02^2) with exceptions (0, 2^-30, 8.0) in every block: in every K quarter the first and the last k-step of every wave's slice
    of the launch that streams this K (so in both k-steps of a chunk), one row per (block, quarter), and two entries in one k-step of one
    quarter; with the entry per wave below 18 per block, under the cap of 32 with the natural ones (at most 9, test_w12_cpu.py)"""
    _, U = LAUNCH[K]
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn(N, K, generator=g) * 0.02).to(bf16)
    vals = [0.0, 2.0 ** -30, 8.0]
    n = 0
    for nb in range(N // 16):
        i0, i1 = wide_wave_steps(K // 32, U, WV)[(3 * nb + 1) % WV]
        for h in range(4):
            r = nb * 16 + (5 * nb + 3 * h) % 16
            for i, j in ((i0, 0), (i1 - 1, 7)) + (((i0 + 1, 2), (i0 + 1, 5)) if h == nb % 4 else ()):
                W[r, h * (K // 4) + i * 8 + j] = vals[n % 3]
                n += 1
    # one entry in the slice of every other wave too (quarter nb % 4), so a cursor that does not skip to i0 stalls in every wave but the first
    for nb in range(N // 16):
        for w, (i0, i1) in enumerate(wide_wave_steps(K // 32, U, WV)):
            W[nb * 16 + w, (nb % 4) * (K // 4) + (i1 - 1) * 8 + 3] = vals[(nb + w) % 3]
    return W


@pytest.mark.parametrize("K", [2048, 2752, 1376])
def test_stream_addressing_reads_the_bytes_of_every_k_step(K):
    from unimoe_audio_amd import w12
    epi, U = LAUNCH[K]
    KB, NB = K // 32, 3
    assert KB in (64, 86, 43) and stream_form(KB, U) == (1 if KB == 43 else 2)
    W = planted(NB * 16, K, K)
    wp16 = w12.wp16_from_rows(W)
    pk = w12.pack(wp16.view(torch.int16), KB)
    assert pk is not None
    data, meta = pk
    assert 18 <= int(w12.exceptions_per_block(meta).min()) and int(w12.exceptions_per_block(meta).max()) <= w12.CAP
    lo_want = (wp16.view(torch.int16).to(torch.int32) & 0xFF).view(NB, KB, 64, 8)
    blocks = data.view(NB, KB * 768).to(torch.int64)
    for wave, (i0, i1) in enumerate(wide_wave_steps(KB, U, WV)):
        for i in range(i0, i1):
            for lane in (0, 17, 39, 40, 63):
                lo, cw, rec = step_address(KB, U, i0, i1, i, lane)
                assert lo % 8 == 0 and cw % 4 == 0 and rec == min(lane, 39)
                assert torch.equal(blocks[:, lo:lo + 8], lo_want[:, i, lane].to(torch.int64)), (K, wave, i, lane)
    if KB == 43:    # the uneven split: slices start on either k-step parity
        assert [a for a, _ in wide_wave_steps(KB, U, WV)] + [KB] == [0, 5, 10, 16, 21, 26, 32, 37, 43]
    got = rebuild_through_addressing(data, meta, NB, K, U)
    assert torch.equal(got.view(torch.int16), W.view(torch.int16))


@pytest.mark.parametrize("K", [2048, 2752, 1376])
def test_emulation_on_the_addressed_weights_equals_the_wp16_weights(K):
    from unimoe_audio_amd import w12
    epi, U = LAUNCH[K]
    rows, N, NB = 34, 32, 2
    KB = K // 32
    g = torch.Generator().manual_seed(K + 1)
    A = torch.randn(rows, K, generator=g).to(bf16)
    ws = [planted(N, K, 10 * K + j) for j in range(2 if epi == SWIGLU else 1)]
    if epi == SWIGLU:
        wp16 = w12.wp16_gate_up(ws[0], ws[1])
        split = lambda W: [W.view(NB, 2, 16, K)[:, j].reshape(N, K) for j in (0, 1)]          # blocks interleaved: 2 i gate, 2 i + 1 up
        blocks = 2 * NB
    else:
        wp16 = w12.wp16_from_rows(ws[0])
        split = lambda W: [W]
        blocks = NB
    pk = w12.pack(wp16.view(torch.int16), KB)
    assert pk is not None
    data, meta = pk
    want = emu_wide(A, ws, K, rows, epi, U, WV)
    seen = split(rebuild_through_addressing(data, meta, blocks, K, U))
    assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(seen, ws))
    assert torch.equal(emu_wide(A, seen, K, rows, epi, U, WV).view(torch.int16), want.view(torch.int16))
    # planted errors: a cursor that starts at entry 0 instead of at the wave's i0, and (2-step chunks) the two k-steps of a chunk swapped
    wrong = split(rebuild_through_addressing(data, meta, blocks, K, U, cursor_from_zero=True))
    assert not torch.equal(emu_wide(A, wrong, K, rows, epi, U, WV).view(torch.int16), want.view(torch.int16))
    if stream_form(KB, U) == 2:
        wrong = split(rebuild_through_addressing(data, meta, blocks, K, U, swap_steps=True))
        assert not torch.equal(emu_wide(A, wrong, K, rows, epi, U, WV).view(torch.int16), want.view(torch.int16))
