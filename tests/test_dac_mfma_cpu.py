"""CPU suite of the DAC convolutions on the f32 MFMA (conv_form="mfma"; csrc/umoe_dac_mfma.hip).

  index math   walk() restates on the host what the kernels sum: per output the ordered terms (input channel, tap, input position) of the
               implicit GEMM -- r = ci K + k for conv1d; per phase (t + pad) mod stride, r = ci M + m with k = phase + m stride and
               input (t + pad) / stride - m for the transposed form -- in k-chunks of 32 with the zero-filled tail, read from the
               k-major weight wt [Cin][K][Cout].  It evaluates them as the MFMA does: an fp32 fma chain in ascending r, the product in
               float64 (exact: 24 + 24 bits), one rounding to fp32 per term.  The result passes check_conv / check_win of
               tests/test_gpu_dac_fp64.py on every case of that file: its bound (n + 2) u S + u |ref| holds for ANY summation order and
               charges one rounding per term plus one per product, so a chain with one rounding per term is inside it.
               Q2 adds transposed cases with a second and a third q tile (q = (t + pad) / stride, 64 per phase and tile), which that
               file's cases (L <= 33) never reach.
  planted      the same walk with one thing wrong is rejected: a tap shifted by one from the second position tile on (conv1d and, on Q2,
               the transposed form's second q tile), the reduction tail
               (the last partial k-chunk) dropped, the transposed phase off by one, the k-major weight indexed as [Cin][Cout][K], the bias
               missing on the last channel tile, tanh and the residual swapped.
  routing      dac.uses_mfma is the only rule: with a mocked _lib_call the full, windowed and per-row calls of every layer take the same
               form; a default DacModel makes no _mfma call and builds no k-major copy.
  interface    the six names in _lib.EXPORTS and umoe.h; ValueError on a form that is neither "direct" nor "mfma".
  code         umoe_dac_mfma.hip cross-compiled for gfx950: six kernels, no scratch, no spills, 32 f32-input MFMAs each, none under an
               EXEC mask (scripts/scan_mfma_exec.py).
"""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch

import test_gpu_dac_fp64 as F64
from conftest import ROOT
from test_gpu_dac_fp64 import CONV_GROUPS, CONVT_GROUPS, Stats, all_cases, check_conv, check_win, conv_case, ct, emu_win, snake32, win_buffers, windows_of
from unimoe_audio_amd import _lib as L
from unimoe_audio_amd import dac as D

TM, TN, KC = 64, 64, 32          # the kernels' tile (channels x positions) and k-chunk
MFMA_NAMES = ["umoe_dac_conv1d_mfma", "umoe_dac_conv_transpose1d_mfma", "umoe_dac_conv1d_win_mfma", "umoe_dac_conv_transpose1d_win_mfma",
              "umoe_dac_conv1d_win_rows_mfma", "umoe_dac_conv_transpose1d_win_rows_mfma"]


Q2 = [ct("mc_t_q66", 9, 5, 4, 65, 2, 1), ct("mc_t_s4_q130", 3, 66, 8, 129, 4, 2)]      # transposed, two and three q tiles


def case_of(spec, snake):
    """conv_case of a spec of this file (that function looks its spec up by name)"""
    F64.SPECS[spec["name"]] = spec
    try:
        return conv_case(spec["name"], snake)
    finally:
        del F64.SPECS[spec["name"]]


# ------------------------------------------------------------------------------------------------ the kernels' index math
def terms(c, plant=None):
    """The k-steps every output of case c passes through, in the kernels' order, zero-filled steps included.  Yields (ci, widx, pos):
    ci the input channel (None: a step past the reduction's end, both operands zero), widx [Cout][Lout] the flat index into wt
    [Cin][K][Cout] (-1: the weight is zero), pos [Lout] the input position (-1: the input is zero)."""
    Cin, Cout, K, L, s, pad, Lout = c["Cin"], c["Cout"], c["K"], c["L"], c["stride"], c["pad"], c["Lout"]
    t = torch.arange(Lout)
    co = torch.arange(Cout)[:, None]
    if c["kind"] == "conv":
        R, tile = Cin * K, t // TN
        taps = [(r // K, torch.full_like(t, r % K)) for r in range(R)]
        where = lambda k: t * s - pad + k * c["dil"]                                  # noqa: E731
    else:
        M = (K + s - 1) // s
        u = t + pad + (1 if plant == "phase" else 0)
        ph, q = u % s, u // s
        R, tile = Cin * M, (q - pad // s) // TN
        taps = [(r // M, ph + (r % M) * s) for r in range(R)]
        where = lambda k: q - (k - ph) // s                                           # noqa: E731
    steps = (R + KC - 1) // KC * KC
    if plant == "tail":
        assert R % KC
        R = R // KC * KC
    for r in range(steps):
        if r >= R:
            yield None, None, None
            continue
        ci, k = taps[r]
        pos = where(k)
        if plant == "tap":
            pos = pos + ((tile >= 1) & (k == K - 1)).long()
        live = (k < K) & (pos >= 0) & (pos < L)
        widx = (ci * Cout + co) * K + k[None] if plant == "kmajor" else (ci * K + k[None]) * Cout + co
        yield ci, torch.where((k < K)[None], widx, torch.full_like(widx, -1)), torch.where(live, pos, torch.full_like(pos, -1))


def walk(c, plant=None):
    """the launch as the MFMA kernels compute it: staging (fp32 Snake), the fma chain over terms(), the store's epilogue"""
    x = c["x"] if c["alpha"] is None else snake32(c["x"], c["alpha"])
    wt = D.kmajor(c["w"], c["kind"] == "convt").reshape(-1)
    acc = torch.zeros(x.shape[0], c["Cout"], c["Lout"])
    for ci, widx, pos in terms(c, plant):
        if ci is None:
            continue                                                                  # fma(0, 0, acc) == acc
        a = torch.where(widx >= 0, wt[widx.clamp(0, wt.numel() - 1)], torch.zeros(()))            # [Cout][Lout]
        b = torch.where(pos >= 0, x[:, ci, pos.clamp(min=0)], torch.zeros(()))        # [B][Lout]
        acc = (acc.double() + a.double()[None] * b.double()[:, None]).float()         # one rounding per term
    bias = c["b"].clone()
    if plant == "bias":
        bias[(c["Cout"] - 1) // TM * TM:] = 0
    v = acc + bias.reshape(1, -1, 1)
    if plant == "swap":
        return torch.tanh(v + c["resid"])
    if c["tanh"]:
        v = torch.tanh(v)
    return v if c["resid"] is None else v + c["resid"]


def _rejects(fn):
    with pytest.raises(AssertionError):
        fn()


def test_walk_passes_the_fp64_checkers():
    st = Stats()
    for groups, tag in ((CONV_GROUPS, "conv1d"), (CONVT_GROUPS, "transposed")):
        for c in all_cases(groups) + ([case_of(s, sn) for s in Q2 for sn in (False, True)] if groups is CONVT_GROUPS else []):
            y = walk(c)
            check_conv(c, y, st, tag)
            for t0, n in windows_of(c["Lout"]):
                wb = win_buffers(c, t0, n)
                check_win(c, wb, emu_win(c, wb, y), st, tag + " windows")
    st.show("MFMA walk")
    assert max(st.values()) <= 1.0


def test_walk_is_the_convolution_on_exact_data():
    """small integers: every partial sum is exact, so the walk must equal the float64 convolution bit for bit -- the index math alone"""
    g = torch.Generator().manual_seed(3)
    for name in ("res_d3_L100", "stride_5_L72", "cin_17", "t_s5_op1_L33", "t_K_2s1", "t_K_lt_s", "t_ci9_co65"):
        c = dict(conv_case(name, False))
        c["x"] = torch.randint(-4, 5, c["x"].shape, generator=g).float()
        c["w"] = torch.randint(-4, 5, c["w"].shape, generator=g).float()
        c["b"] = torch.randint(-4, 5, c["b"].shape, generator=g).float()
        c["resid"] = None
        ref = F64._conv(c, c["x"].double(), c["w"].double(), c["b"].double())
        assert torch.equal(walk(c).double(), ref), name


def test_planted_errors_are_rejected():
    def full(name, snake, plant):
        c = conv_case(name, snake) if isinstance(name, str) else case_of(name, snake)
        check_conv(c, walk(c), Stats())
        _rejects(lambda: check_conv(c, walk(c, plant), Stats()))

    for snake in (False, True):
        for spec in Q2:                                                              # the transposed form's second q tile
            full(spec, snake, "tap")
            full(spec, snake, "phase")
        for name in ("pos_L129", "cout_65", "res_d3_L100"):                          # cases with a second position tile
            full(name, snake, "tap")
        for name in ("cin_1", "cin_7", "cin_9", "cin_17", "t_ci7_co1", "t_ci9_co65", "res_d1_L100"):      # Cin K = 3, 21, 27, 51; Cin M = 14, 18; 63
            full(name, snake, "tail")
        for name in ("t_s2_op0_L9", "t_s5_op1_L8", "t_s8_op0_L33", "t_K_lt_s", "t_K_2s1"):
            full(name, snake, "phase")
        for name in ("cout_65", "cin_9", "res_d9_L100", "t_ci9_co65", "t_s4_op0_L8"):
            full(name, snake, "kmajor")
        for name in ("cout_1", "cout_65", "cout_130", "t_ci9_co65"):
            full(name, snake, "bias")
    full("tanh_resid", True, "swap")


# ------------------------------------------------------------------------------------------------ routing
def _shape_of(name, a):
    """(cin, cout, K, stride) out of the argument list of a conv entry"""
    at = {"umoe_dac_conv1d": 6, "umoe_dac_conv_transpose1d": 5, "umoe_dac_conv1d_win": 10, "umoe_dac_conv_transpose1d_win": 7,
          "umoe_dac_conv1d_win_rows": 7, "umoe_dac_conv_transpose1d_win_rows": 7}[name]
    if name in ("umoe_dac_conv1d_win_rows", "umoe_dac_conv_transpose1d_win_rows"):
        return a[at], a[at + 1], a[at + 2], a[at + 3]
    return a[at], a[at + 2], a[at + 3], a[at + 4]


@pytest.fixture
def recorded(monkeypatch):
    """dac.py with the library mocked: every _lib_call is recorded as (entry without _mfma, form, layer shape); tensors stay on the CPU"""
    calls = []

    def rec(name, *a):
        if "dac_conv" not in name:
            calls.append((name, None, None))
            return
        stem = name[:-5] if name.endswith("_mfma") else name
        cin, cout, K, stride = _shape_of(stem, a)
        if "win" not in stem:                                                      # the full forms report Lout
            if stem == "umoe_dac_conv1d":
                a[15]._obj.value = (a[7] + 2 * a[12] - a[11] * (K - 1) - 1) // stride + 1
            else:
                a[13]._obj.value = (a[6] - 1) * stride - 2 * a[10] + K + a[11]
        calls.append((stem, "mfma" if name.endswith("_mfma") else "direct", (cin, cout, K, stride)))

    monkeypatch.setattr(D, "_lib_call", rec)
    monkeypatch.setattr(D, "_dev_f32", lambda t: None if t is None else C.c_void_p(t.data_ptr()))
    monkeypatch.setattr(D, "_stream", lambda: None)
    return calls


def _tiny():
    return D.DacModel(encoder_dim=4, encoder_rates=(2, 4, 5, 8), latent_dim=6, decoder_dim=16, decoder_rates=(8, 5, 4, 2), n_codebooks=12,
                      codebook_size=16, codebook_dim=4).init_random(0).float()


def _run_everything(m):
    """decode in all three forms: full, DacStreamDecoder (_win), DacRowStreamDecoder ragged (_win_rows) and grouped (_win)"""
    z = torch.randn(1, m.latent_dim, 9)
    m.decode(z)
    dec = D.DacStreamDecoder(m, 1, lambda rows, f0, n, out, col: None)
    dec.push(5)
    dec.push(4)
    dec.flush([0])
    for ragged in (True, False):
        rd = D.DacRowStreamDecoder(m, 2, lambda requests, slab: None, ragged=ragged)
        rd.push([5, 0])
        rd.push([4, 3])
        rd.flush([0])


@pytest.mark.parametrize("rule", [lambda cin, cout, K, stride: True, lambda cin, cout, K, stride: K == 7,
                                  lambda cin, cout, K, stride: cout > 1 and stride == 1], ids=["all", "K7", "not_head_stride1"])
def test_uses_mfma_is_the_only_routing_rule(recorded, monkeypatch, rule):
    monkeypatch.setattr(D, "uses_mfma", rule)
    m = _tiny().set_conv_form("mfma")
    _run_everything(m)
    forms = {}
    for stem, form, shape in recorded:
        if form is not None:
            forms.setdefault(shape, {}).setdefault(form, set()).add(stem)
    assert len(forms) >= 8
    for shape, by_form in forms.items():
        assert list(by_form) == ["mfma" if rule(*shape) else "direct"], (shape, by_form)
        kinds = {s.replace("_transpose", "") for s in by_form[list(by_form)[0]]}
        assert kinds == {"umoe_dac_conv1d", "umoe_dac_conv1d_win", "umoe_dac_conv1d_win_rows"}, (shape, kinds)      # full, windowed, per-row
    # the encoder follows the same rule
    del recorded[:]
    m._run(m.encoder.items(), torch.randn(1, 1, 640), m._folded())
    assert recorded and all(form == ("mfma" if rule(*shape) else "direct") for _, form, shape in recorded if form)
    # the k-major copies: exactly the layers the rule names, [Cin][K][Cout]
    f = m._folded()
    convs = [w for part in (m.encoder, m.decoder) for w in part.modules() if isinstance(w, D._WN)]
    assert set(f["wt"]) == {w for w in convs if rule(*w.shape4())}
    for w, wt in f["wt"].items():
        cin, cout, K, _ = w.shape4()
        assert tuple(wt.shape) == (cin, K, cout) and wt.is_contiguous()
        assert torch.equal(wt, f[w][0].permute(0, 2, 1) if w.geom["transposed"] else f[w][0].permute(1, 2, 0))


def test_default_model_makes_no_mfma_call_and_no_copies(recorded, monkeypatch):
    def no_copy(*a):
        raise AssertionError("a k-major copy in the direct form")

    monkeypatch.setattr(D, "kmajor", no_copy)
    m = _tiny()
    assert m.conv_form == "direct" and D.Dac(model=m).conv_form == "direct"
    _run_everything(m)
    m._run(m.encoder.items(), torch.randn(1, 1, 640), m._folded())
    assert recorded and all(form in (None, "direct") for _, form, _ in recorded)
    assert m._folded()["wt"] == {}
    # the cache is keyed by the form: switching rebuilds it, switching back drops the copies
    monkeypatch.undo()
    f_direct = m._folded()
    assert m.set_conv_form("mfma")._folded() is not f_direct and len(m._folded()["wt"]) > 0
    assert m.set_conv_form("direct")._folded()["wt"] == {}


def test_names_and_bad_forms():
    header = open(os.path.join(ROOT, "include", "umoe.h")).read()
    for name in MFMA_NAMES:
        assert name in L.EXPORTS and re.search(r"\bint " + name + r"\(", header), name
    assert "#define UMOE_DAC_ROW_WORDS 12" in header
    m = _tiny()
    for bad in ("MFMA", "bf16", "", None):
        with pytest.raises(ValueError):
            m.set_conv_form(bad)
        if bad is not None:                                                            # (Dac: None leaves a given model's form alone)
            with pytest.raises(ValueError):
                D.Dac(model=m, conv_form=bad)
        with pytest.raises(ValueError):
            D.conv1d(torch.zeros(1, 1, 8), torch.zeros(1, 1, 3), None, form=bad)
        with pytest.raises(ValueError):
            D.conv_transpose1d(torch.zeros(1, 1, 8), torch.zeros(1, 1, 4), None, stride=2, padding=1, form=bad)
        from unimoe_audio_amd.api import UniMoEAudio
        with pytest.raises(ValueError):
            UniMoEAudio(None, 0, dac_conv=bad)
    assert m.conv_form == "direct"
    assert D.Dac(model=m, conv_form="mfma").conv_form == "mfma" and m.conv_form == "mfma"
    assert D.Dac(model=m).conv_form == "mfma"                                          # a model handed in keeps the form it has
    assert D.Dac(model=m, conv_form="direct").conv_form == "direct" and m.conv_form == "direct"
    assert D.uses_mfma(768, 768, 7, 1) is True


# ------------------------------------------------------------------------------------------------ the compiled kernels
def test_mfma_kernels_compile_for_gfx950_without_scratch_or_predicated_mfma(tmp_path):
    csrc = os.path.join(ROOT, "unimoe_audio_amd", "csrc")
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found"
    out = str(tmp_path / "umoe_dac_mfma.s")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt", "--offload-arch=gfx950",
                        "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "--cuda-device-only", "-S", os.path.join(csrc, "umoe_dac_mfma.hip"),
                        "-Rpass-analysis=kernel-resource-usage", "-o", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    blocks = {b.split()[0]: b for b in r.stdout.split("Function Name: ")[1:]}
    assert len(blocks) == 6 and all("mfma_kernel" in n for n in blocks), sorted(blocks)      # full + windowed x 2 flavours, per-row x 2
    for n, b in blocks.items():
        assert [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", b)] == [0], (n, b)
        assert [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", b)] == [0] and [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", b)] == [0], (n, b)
        assert [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", b)] == [2 * KC * 80 * 4], (n, b)
        occ = re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", b)
        assert len(occ) == 1 and int(occ[0]) >= 2, (n, b)
    txt = open(out).read()
    for name in blocks:
        body = txt.split("\n" + name + ":")[1].split(".Lfunc_end")[0]
        assert body.count("v_mfma_f32_16x16x4_f32") == 32 and body.count("v_mfma") == 32, name      # 8 k-steps x 2 x 2 tiles per chunk
        assert "scratch_" not in body, name
    scan = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "scan_mfma_exec.py"), out], stdout=subprocess.PIPE, text=True, timeout=120)
    assert scan.returncode == 0 and " 0 under s_and_saveexec" in scan.stdout and "192 MFMA" in scan.stdout, scan.stdout
