"""CPU suite of the wide decode step (batches of 9 to 32 requests, every weight streamed once): the new C-ABI symbols, the
MFMA guards of umoe_gemm_wide.hip, the serving ceiling of the scheduler, and the K split of the wide kernel restated on the emulation of
the 16-row kernel (tests/test_gpu_wstream_fp64.py)."""
import ctypes
import os
import random
import re
import subprocess
import sys

import pytest
import torch

from conftest import ROOT
from test_serve_cpu import FakeEngine, greedy_makespan
from test_gpu_wstream_fp64 import BF16, F32, MARGIN, PLAIN, RESID, SWIGLU, emu, kernel_of, rbf32, step_cols, wave_steps

bf16 = torch.bfloat16
NEW_SYMBOLS = ["umoe_gemm_wide", "umoe_pack_rows"]


def test_new_symbols_are_exported_and_declared():
    from unimoe_audio_amd import _lib
    L = ctypes.CDLL(_lib.build())
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "umoe.h")).read(), flags=re.S)
    for n in NEW_SYMBOLS:
        assert hasattr(L, n), n
        assert re.search(r"\b" + n + r"\s*\(", txt), n
        assert n in _lib.EXPORTS
    assert _lib.lib().umoe_abi_version() == 1
    assert len(_lib.STRUCT_MIRRORS) == 16          # plain scalar and pointer arguments: no new argument struct
    from unimoe_audio_amd import ops
    assert callable(ops.gemm_wide) and callable(ops.pack_rows)


def test_no_mfma_of_the_wide_kernel_is_predicated_through_exec(tmp_path):
    """MFMA ignores EXEC: every guard around an MFMA of umoe_gemm_wide.hip must be a scalar branch (scripts/scan_mfma_exec.py)."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from scan_mfma_exec import scan
    csrc = os.path.join(ROOT, "unimoe_audio_amd", "csrc")
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found"
    out = str(tmp_path / "umoe_gemm_wide.s")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt", "--offload-arch=gfx950",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "--cuda-device-only", "-S", os.path.join(csrc, "umoe_gemm_wide.hip"),
                           "-o", out], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    n, bad = scan(out)
    assert n > 0 and not bad, bad[:3]


# ------------------------------------------------------------------------------------------------ scheduler
@pytest.mark.parametrize("slots,poll_every,seed", [(16, 16, 0), (9, 4, 1), (32, 16, 2)])
def test_scheduler_serves_more_than_eight_rows_when_allowed(slots, poll_every, seed):
    from unimoe_audio_amd.serve import Scheduler, makespan_steps
    rng = random.Random(seed)
    reqs = [(f"r{i}", rng.choice([1, 7, 16, 40, 150, 151, 400, 1000])) for i in range(3 * slots + 5)]
    eng = FakeEngine(slots)
    sched = Scheduler(eng, slots, poll_every, max_slots=32)
    out = list(sched.run(iter(reqs)))
    assert sorted(i for i, _ in out) == list(range(len(reqs)))
    assert all(name == reqs[i][0] for i, name in out)
    admits = [e for e in eng.log if e[0] == "admit"]
    assert [e[3] for e in admits] == [r[0] for r in reqs]                   # first in, first out
    assert {e[2] for e in admits} == set(range(slots))                      # every row is used
    for row in range(slots):
        kinds = [e[0] for e in eng.log if e[2] == row]
        assert kinds == ["admit", "take"] * (len(kinds) // 2)
    want = greedy_makespan([r[1] for r in reqs], slots, poll_every)
    assert sched.steps_run == eng.clock == want
    assert makespan_steps([r[1] for r in reqs], slots, poll_every, max_slots=32) == want


def test_scheduler_ceiling():
    from unimoe_audio_amd.serve import MAX_SLOTS, Scheduler
    assert MAX_SLOTS == 8
    with pytest.raises(ValueError):
        Scheduler(FakeEngine(9), 9)                      # the default ceiling stays 8
    with pytest.raises(ValueError):
        Scheduler(FakeEngine(33), 33, max_slots=33)      # 32 rows is the most any caller may ask for
    with pytest.raises(ValueError):
        Scheduler(FakeEngine(8), 8, max_slots=33)
    with pytest.raises(ValueError):
        Scheduler(FakeEngine(17), 17, max_slots=16)
    assert Scheduler(FakeEngine(32), 32, max_slots=32).slots == 32


# ------------------------------------------------------------------------------------------------ K split
def wide_wave_steps(KB, U, WV):
    """wstream_wide (umoe_gemm_wide.hip), restated from its source: the k-steps [i0, i1) of every wave of a workgroup"""
    out = []
    for wave in range(WV):
        if KB % U == 0:
            units = KB // U
            out.append((U * (units * wave // WV), U * (units * (wave + 1) // WV)))
        else:
            out.append((KB * wave // WV, KB * (wave + 1) // WV))
    return out


def emu_wide(A, ws, K, rows, epi, U, WV, bias=None, resid=None):
    """the wide launch in the arithmetic of test_gpu_wstream_fp64.emu: per 16-row tile (pad rows zero, never returned) every wave adds
    its k-steps in ascending order into one accumulator, the waves' partial tiles are added in wave order, then the epilogue"""
    tiles = (rows + 15) // 16
    outs = []
    for t in range(tiles):
        r0, r1 = 16 * t, min(16 * t + 16, rows)
        a = torch.zeros(16, K, dtype=bf16)
        a[:r1 - r0] = A[r0:r1]
        accs = []
        for w_ in ws:
            acc = torch.zeros(r1 - r0, w_.shape[0])
            for i0, i1 in wide_wave_steps(K // 32, U, WV):
                if i1 > i0:
                    cols = step_cols(K, range(i0, i1))
                    acc = acc + a[:r1 - r0, cols].float() @ w_[:, cols].float().t()
            accs.append(acc)
        if epi == SWIGLU:
            gt, up = rbf32(accs[0]), rbf32(accs[1])
            o = (rbf32(gt / (1.0 + torch.exp(-gt))) * up).to(bf16)
        else:
            v = accs[0] if bias is None else accs[0] + bias
            o = rbf32(v) if epi == F32 else (v.to(bf16) if epi == BF16 else (resid[r0:r1].float() + rbf32(v)).to(bf16))
        outs.append(o)
    return torch.cat(outs)


# (epilogue, nt / waves of the 16-row spec that selects the split, (WV, U) expected of it)
SPLITS = [("qkv", BF16, 1, 0, (4, 16)), ("o_proj", RESID, 1, 0, (4, 16)), ("head", F32, 2, 0, (4, 8)), ("gate_up", SWIGLU, 2, 8, (8, 1)),
          ("down", BF16, 1, 8, (8, 2))]


@pytest.mark.parametrize("K", [2048, 2752, 1376])
@pytest.mark.parametrize("name,epi,nt,waves,wvu", SPLITS, ids=[s[0] for s in SPLITS])
def test_wide_k_split_equals_the_16_row_kernels_on_every_tile(name, epi, nt, waves, wvu, K):
    WV, U = wvu
    spec = dict(nt=nt, waves=waves, pro=PLAIN, groups=[dict(k=K)])
    _, u16, wv16, _ = kernel_of(spec, epi)
    assert (wv16, u16) == (WV, U)                      # the 16-row launch this GEMM of the decode step takes
    assert wide_wave_steps(K // 32, U, WV) == wave_steps(K // 32, 0, 1, U, WV)[2]
    g = torch.Generator().manual_seed(K + 7 * WV + U)
    rows, N = 34, 32                                   # three tiles, the last one of 2 rows
    A = torch.randn(rows, K, generator=g).to(bf16)
    ws = [(torch.randn(N, K, generator=g) * K ** -0.5).to(bf16) for _ in range(2 if epi == SWIGLU else 1)]
    bias = torch.randn(N, generator=g) * 0.5 if name == "qkv" else None
    resid = torch.randn(rows, N, generator=g).to(bf16)
    got = emu_wide(A, ws, K, rows, epi, U, WV, bias=bias, resid=resid)
    assert got.shape == (rows, N)
    for t in range(3):
        r0, r1 = 16 * t, min(16 * t + 16, rows)
        d = dict(rows=r1 - r0, k=K, N=N, w=ws, arows=torch.arange(r1 - r0), ac=0, orows=torch.arange(r1 - r0))
        if bias is not None:
            d["bias"] = bias
        c = dict(spec=spec, pro=PLAIN, sw=epi == SWIGLU, kind="g", A=A[r0:r1], resid=resid[r0:r1], groups=[d], RO=r1 - r0, ldo=N, n_valid=N)
        want = emu(c, epi)[MARGIN:MARGIN + r1 - r0, :N]
        assert want.dtype == got.dtype
        assert torch.equal(want.view(torch.int16 if want.dtype == bf16 else torch.int32),
                           got[r0:r1].view(torch.int16 if got.dtype == bf16 else torch.int32)), (name, K, t)
