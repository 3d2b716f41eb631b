"""The weight-streaming decode GEMM -- wstream_gemm / wstream_body (csrc/umoe_gemm.hip) through umoe_grouped_gemm -- per element
against a float64 product on the CPU of the same input bits, in every instantiation the launcher can reach, with nt / waves / ksplit
given explicitly (no variant is forced through the environment).

Three kinds of input
  1. exact ("x_", "xs_"): activations are integers 2^-3, weights integers 2^-4 (|integer| <= 4; <= 8 for the activations where
     512 <= K < 2048, so that enough accumulators need the bf16 rounding), the bias integers 2^-7.  Every product and every partial sum
     in ANY order is an integer 2^-7 below 2^24 (asserted on the CPU), so the fp32 accumulator EQUALS the float64 product whatever the
     order of MFMAs, waves and slabs: no tolerance.  F32_RAW == ref (with ksplit: slab s == ref over k-steps [KB s / ksplit,
     KB (s + 1) / ksplit) of every K quarter, the bias in slab 0 only), BF16 / F32 == rb(ref + bias), BF16_RESID ==
     bf16(fp32(r + rb(ref + bias))), all bit for bit.  SwiGLU: gate / up are known exactly, y = swiglu_y(rb(g), rb(u)); the only
     slack is the fp32 error of g / (1 + expf(-g)) (8 u |silu|): an element whose silu lies within it of a bf16 midpoint is flagged and
     may take either neighbour; exact zero gates count as flagged (with zero width).  At most 2e-2 of a case may be flagged.
  2. permutation ("p_"): W[n, :] = e_perm(n): an output is one product with 1.0 plus zeros -- exact for any activation bits.  Plain
     prologue: out == x[:, perm] bit for bit (pins lds_chunk_off, the quarter layout of WP16, the chunk clamps).  RMSNorm prologue: the
     launch returns h = bf16(nw bf16(x rs)) itself.  rs in float64 with a relative window of 8 u in all: the fp32 sum of squares,
     division, + eps and rsqrtf (measured on the emulated trees: at most 0.53 x 8 u = 4.2 u) AND the 1 u of the fp32 product x rs; an
     element whose x rs lies within that window of a bf16 midpoint is flagged and may take either neighbour, propagated through nw; at
     most 1e-3 of a case.  All staging forms: single round at 4 and 8 waves, the K = 2048 / 8-wave butterfly, two passes (K = 2752, 4096
     at 4 waves).  N = K in every case, so every element of the staged rows is read back: up to K = 2080 as one group; for K = 2752 /
     4096 as two / four groups of one launch that stage the SAME activation rows and take consecutive slices of one permutation (each
     weight stays under 8 MB); test_coverage_cpu asserts that every column is named.
  3. Gaussian ("g_", "gs_"): bf16 randn activations, randn K^-1/2 weights.  E32 = K_eff u sum |a w| (u = 2^-24; K_eff = K, the slab's
     length for a slab, K + ksplit for the summed slabs), + u |acc + bias| with a bias; intervals per epilogue as in
     test_gpu_gemm_fp64.py.  RMSNorm with general weights: h_lo / h_hi from the rule of kind 2, the product is taken at their mean and
     sum_k |W[n, k]| (h_hi - h_lo) / 2 is added to the bound.  SwiGLU (this kernel stores no pre-activations): gate and up get their
     BF16 intervals, y the hull of swiglu_y over their ends (and over the bf16 next to silu's minimum where a gate interval holds it).
     At K >= 2048 most bf16 intervals hold two values; the sharp statement is kind 1.  "acc" is |F32_RAW - ref| / E32.

Memory (every case): operands and outputs are windows of larger buffers.  NaN fills everything the header says is not read:
activation rows behind a count, rows no gather list names (entries of a list outside [row_off, row_off + count) point at one), columns
outside [a_col_off, a_col_off + k) of a wider lda, bias entries >= n_valid, the residual outside the written window, norm_w behind K,
the bytes around a packed weight.  Outputs are prefilled with 7.0: rows behind a count, rows between groups, columns >= n_valid (for
SwiGLU >= I; for a group of fewer blocks >= 16 n_blocks: a stored tail tile lands there) up to ldo keep it bit for bit; a NaN anywhere
fails.

Dispatch: launch_gemm_nt / auto_nt / use8 / the BV predicate are restated (kernel_of); test_coverage_cpu asserts that the case list
reaches every instantiation of REQUIRED and both sides of: use8 by LDS size, BV, descriptors by value / from memory,
(ib - ia) % U == 0, the whole-chunk fast path of U >= 4, bias_vec, ldo % 4, static / ragged order of requests, the three RMSNorm forms.
Note on K = 512 at U = 16 (nt 1): 16 steps are ONE whole chunk, so the unit split hands all of them to wave 3 and three waves idle.

CPU self-checks (test_*_cpu): a torch emulation of wstream_body (K quarters, the per-wave step ranges i0..i1 as the code computes
them, the fixed-order wave sum, the epilogues' rounding points, the three RMSNorm summation trees) passes every checker for every
case; each planted error of PLANTS is rejected; the exactness precondition, the >= 5 % rounded share (per case over its groups with K >= 512) and the flagged-share
conditions hold.

Found by this file
  * F32_RAW with ksplit > 1 added the group's bias in EVERY slab, so the documented use (sum the slabs) gave acc + ksplit bias.  No
    caller passed both.  wstream_body now adds it in slab 0 only (include/umoe.h says so); case x_ksplit pins it: slabs 1.. of the
    parent commit differ from their reference by the bias.

Measured on an MI355X (the whole file: 47 GPU tests in 1.2 s on the card; the four tests without a GPU in 5 s).  -s prints per case
the instantiations it ran <NT,U,WV; v = descriptors by value at compile time>, the flagged share and the worst error / bound per
epilogue; an interval ratio is 0 or 1 (an output sits in its interval; 1 = a two-valued interval met at its other end).
  exact data, linear   x_nt1 <1,16,4v>, x_nt2 <2,8,4v>, x_nt8 <8,2,4>, x_nt8_lds <8,2,8>, x_nt4 <4,4,4>, x_nt5 <5,3,4>, x_nt5w8 <5,3,8>,
                       x_nt6 <6,2,4>, x_nt6w8 <6,2,8v>, x_w8nt1 <1,2,8>, x_w8nt2 <2,2,8>, x_w8nt4 <4,2,8>, x_mem13 <1,16,4>, x_ragged <2,8,4v>,
                       x_ragged_nt8 <8,2,8>, x_ksplit <1,16,4v>, x_ksplit_nt8 <8,2,4>: every ratio 0 -- every output of every epilogue, every
                       slab and every sum of slabs (ksplit 2, 3, 4) bit for bit, nothing flagged
  exact data, SwiGLU   flagged (= the reference's own share, test_emulation_passes_cpu): xs_nt2 6.3e-3, xs_nt4 4.6e-3, xs_nt6 2.6e-3,
                       xs_nt8 5.6e-3, xs_nt8_lds 2.0e-3, xs_w8nt2 1.2e-2, xs_w8nt4 2.6e-3, xs_nt14 3.5e-3, xs_mem13 1.2e-2 (the K = 32 / 96 / 128
                       groups set it: exact zero gates); every unflagged element bit for bit
                       rounded share of the accumulators (test_exact_preconditions_cpu): >= 5 % asserted per case over its K >= 512 groups
  permutation, plain   p_plain_2048, p_plain_2080, p_plain_1376 <8,2,8>, p_plain_96: out == x[:, perm] bit for bit
  permutation, RMSNorm flagged p_rms_96 0, p_rms_512 0, p_rms_2048 4.3e-4, p_rms_bfly 5.5e-4, p_rms_2752w8 5.3e-4, p_rms_2752 0, p_rms_4096 0
                       (lumpy: a bf16 x has 128 mantissas, so one mantissa of a row near a midpoint flags all its elements); every
                       unflagged element bit for bit, BF16 and F32.  Worst |rs_fp32 - rs_float64| / (8 u rs) of the emulated summation
                       trees: single 0.41, butterfly 0.17, two passes 0.53 -- 8 u in all (rs and the product) holds on the card, not widened
  Gaussian             g_nt1 acc 0.0087, g_nt8 acc 1.0e-4, g_ksplit slab 1.4e-3 / sum 2.1e-4 (worst of ksplit 2, 3); interval ratios 1;
                       flagged (RMSNorm prologue, SwiGLU) g_rms_nt1 8.6e-4, g_rms_nt8 4.1e-4, gs_nt14 5.2e-4, gs_rms_nt4 4.5e-4, others 0
No accumulator came near its bound: nothing speaks against round-to-nearest adds inside and between the MFMAs, u stays 2^-24.
"""
import functools

import pytest
import torch

from test_gpu_bwd_fp64 import check, keeps_sentinel, mid_dist, ulp_bf16
from test_gpu_gemm_fp64 import Stats as _Stats, check_bf16, interval, interval_resid, rb, swiglu_y

gpu = pytest.mark.gpu

U32 = 2.0 ** -24        # fp32 unit roundoff
RS_W = 8 * U32          # fp32(x rs) against float64, relative: rs = rsqrtf(ss / K + eps) and the product's own rounding
SENT = 7.0
NAN = float("nan")
EPS = 1e-6
G0 = -1.2784645         # argmin of silu
f64 = torch.float64
bf16 = torch.bfloat16
PLAIN, RMS = 0, 1
BF16, RESID, SWIGLU, F32, RAW = 0, 1, 2, 3, 4          # UMOE_EPI_*
EPI_NAME = {BF16: "bf16", RESID: "resid", SWIGLU: "swiglu", F32: "f32", RAW: "raw"}
ALL4 = (BF16, RESID, F32, RAW)
MARGIN = 4              # sentinel rows in front of and behind the output window
GROUPS_INLINE = 12


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from unimoe_audio_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


class Stats(_Stats):
    prefix = "WSTREAM FP64"


def rbf32(x):
    return x.to(bf16).float()


# ------------------------------------------------------------------------------------------------ case list (specs only: no data)
def G(rows, nb, k, dev=False, gather=False):
    return dict(rows=rows, nb=nb, k=k, dev=dev, gather=gather)


def case(name, groups, epis, nt, waves=0, pro=PLAIN, ksplits=(0,), cut=0, ldo="v", bias="none", max_rows=None):
    """kind from the name's prefix; cut: n_valid = 16 max(nb) - cut; ldo "v" (multiple of 4) / "odd"; bias "none" / "al" (16-byte
    aligned) / "off1" (one float behind that)"""
    pre = name.split("_")[0]
    return dict(name=name, kind=pre[0], sw=pre.endswith("s"), groups=groups, epis=epis, nt=nt, waves=waves, pro=pro, ksplits=ksplits,
                cut=cut, ldo=ldo, bias=bias, max_rows=max_rows)


_RAGGED = [G(0, 3, 128, True, True), G(1, 3, 96, True), G(16, 4, 512, True, True), G(17, 5, 2048, True), G(17, 3, 128, True, True),
           G(16, 2, 96, True), G(1, 5, 32, True, True), G(0, 2, 128, True)]
CASES = [
    # ---- exact data, linear epilogues
    case("x_nt1", [G(17, 5, 2048), G(1, 3, 32), G(16, 5, 512), G(15, 2, 2080)], ALL4, 1, bias="al", cut=3),
    case("x_nt2", [G(15, 5, 2080), G(33, 3, 96), G(16, 4, 1376)], ALL4, 2, bias="off1", cut=1, ldo="odd"),
    case("x_nt8", [G(17, 11, 1376), G(1, 9, 128), G(33, 3, 2048)], ALL4, 8, waves=4, cut=13),
    case("x_nt8_lds", [G(16, 10, 2752), G(17, 3, 2752)], (BF16, RAW), 8, bias="al"),                      # 8 waves by use8's LDS rule
    case("x_nt4", [G(16, 6, 2048), G(17, 5, 2080), G(1, 4, 96)], (BF16,), 4, bias="off1", cut=1),
    case("x_nt5", [G(17, 7, 1376), G(15, 5, 96)], (BF16,), 5, bias="al", cut=3),                          # waves auto: 4
    case("x_nt5w8", [G(16, 7, 2752), G(1, 6, 512)], (BF16,), 5, waves=8, cut=1, ldo="odd"),
    case("x_nt6", [G(17, 7, 2752), G(16, 6, 32)], (BF16,), 6, waves=4, bias="off1"),
    case("x_nt6w8", [G(16, 8, 2752), G(33, 7, 1376)], (BF16,), 6, waves=8, bias="al", cut=13),
    case("x_w8nt1", [G(17, 3, 2048), G(1, 2, 32)], (BF16,), 1, waves=8, bias="al", cut=1),
    case("x_w8nt2", [G(16, 3, 1376), G(15, 2, 2080)], (BF16,), 2, waves=8, ldo="odd"),
    case("x_w8nt4", [G(15, 5, 4096), G(16, 3, 128)], (BF16,), 4, waves=8, bias="off1", cut=3),
    case("x_mem13", [G(1 + i % 3, 2 + i % 2, 96 if i == 5 else 128) for i in range(13)], (BF16, RAW), 1, bias="al", cut=1),
    case("x_ragged", _RAGGED, ALL4, 2, bias="al", cut=3, max_rows=40),
    case("x_ragged_nt8", _RAGGED, (BF16, RESID), 8, waves=8, bias="off1", cut=1, ldo="odd", max_rows=40),
    case("x_ksplit", [G(17, 3, 1376), G(5, 2, 64), G(16, 3, 2080)], (RAW,), 1, ksplits=(2, 3, 4), bias="al", cut=3),
    case("x_ksplit_nt8", [G(17, 9, 1376), G(1, 3, 64)], (RAW,), 8, waves=4, ksplits=(2, 3, 4), cut=1),
    # ---- exact data, SwiGLU (nb counts gate / up blocks: I = 8 nb)
    case("xs_nt2", [G(17, 6, 2048), G(1, 4, 32), G(16, 2, 96)], (SWIGLU,), 2),
    case("xs_nt4", [G(16, 6, 512), G(15, 10, 2080)], (SWIGLU,), 4),
    case("xs_nt6", [G(17, 8, 2752), G(1, 6, 128)], (SWIGLU,), 6),
    case("xs_nt8", [G(33, 10, 4096), G(16, 6, 96)], (SWIGLU,), 8, waves=4),
    case("xs_nt8_lds", [G(16, 12, 2752)], (SWIGLU,), 8),
    case("xs_w8nt2", [G(17, 4, 2048), G(15, 6, 32)], (SWIGLU,), 2, waves=8),
    case("xs_w8nt4", [G(16, 6, 1376)], (SWIGLU,), 4, waves=8),
    case("xs_nt14", [G(16, 30, 2048), G(15, 30, 2752), G(1, 12, 512)], (SWIGLU,), 14),
    case("xs_mem13", [G((0, 1, 16, 17)[i % 4], 2 + 2 * (i % 2), 96 if i == 4 else 128, True, i % 3 == 0) for i in range(13)], (SWIGLU,), 2,
         max_rows=33),
    # ---- permutation weights
    case("p_plain_2048", [G(17, 128, 2048)], (BF16,), 1),
    case("p_plain_2080", [G(15, 130, 2080)], (BF16,), 1),
    case("p_plain_1376", [G(16, 86, 1376)], (BF16,), 8, waves=8),
    case("p_plain_96", [G(33, 6, 96)], (BF16,), 2),
    case("p_rms_96", [G(16, 6, 96)], (BF16, F32), 1, pro=RMS),
    case("p_rms_512", [G(17, 32, 512)], (BF16, F32), 8, waves=4, pro=RMS),
    case("p_rms_2048", [G(33, 128, 2048)], (BF16, F32), 1, pro=RMS),
    case("p_rms_bfly", [G(16, 128, 2048)], (BF16, F32), 8, waves=8, pro=RMS),
    case("p_rms_2752w8", [G(15, 86, 2752)] * 2, (BF16,), 8, pro=RMS),             # groups of a permutation case share their rows
    case("p_rms_2752", [G(17, 86, 2752)] * 2, (BF16, F32), 1, pro=RMS),
    case("p_rms_4096", [G(16, 64, 4096)] * 4, (BF16,), 1, pro=RMS),
    # ---- Gaussian data
    case("g_nt1", [G(17, 5, 2048), G(16, 3, 96)], ALL4, 1, bias="al", cut=3),
    case("g_nt8", [G(33, 10, 2752)], ALL4, 8, bias="off1", cut=1, ldo="odd"),
    case("g_ksplit", [G(17, 4, 1376)], (RAW,), 2, ksplits=(2, 3), bias="al"),
    case("gs_nt14", [G(16, 30, 2048)], (SWIGLU,), 14),
    case("gs_nt4", [G(17, 6, 512)], (SWIGLU,), 4),
    case("g_rms_nt1", [G(17, 5, 2048)], (BF16, F32), 1, pro=RMS, cut=3),
    case("g_rms_nt8", [G(16, 9, 4096)], (BF16, F32), 8, waves=4, pro=RMS),
    case("gs_rms_nt2", [G(17, 4, 2048)], (SWIGLU,), 2, pro=RMS),
    case("gs_rms_nt4", [G(16, 6, 512)], (SWIGLU,), 4, pro=RMS),
    case("gs_rms_nt8", [G(15, 10, 2752)], (SWIGLU,), 8, pro=RMS),
]
SPEC = {s["name"]: s for s in CASES}
assert len(SPEC) == len(CASES)

REQUIRED = {
    (PLAIN, BF16): {(1, 16, 4), (2, 8, 4), (4, 4, 4), (5, 3, 4), (5, 3, 8), (6, 2, 4), (6, 2, 8), (8, 2, 4), (8, 2, 8), (1, 2, 8), (2, 2, 8), (4, 2, 8)},
    (PLAIN, RESID): {(1, 16, 4), (2, 8, 4), (8, 2, 4)},
    (PLAIN, F32): {(1, 16, 4), (2, 8, 4), (8, 2, 4)},
    (PLAIN, RAW): {(1, 16, 4), (2, 8, 4), (8, 2, 4)},
    (PLAIN, SWIGLU): {(2, 8, 4), (4, 4, 4), (6, 2, 4), (8, 2, 4), (8, 2, 8), (2, 1, 8), (4, 1, 8), (14, 1, 8)},
    (RMS, BF16): {(1, 16, 4), (8, 2, 4)},
    (RMS, F32): {(1, 16, 4), (8, 2, 4)},
    (RMS, SWIGLU): {(2, 8, 4), (4, 4, 4), (8, 2, 4)},
}


# ------------------------------------------------------------------------------------------------ dispatch, restated
def lds_bytes(max_k, nt, wv, ksplit, pro=PLAIN):
    """gemm_lds_bytes"""
    per = -(-(max_k >> 5) // max(ksplit, 1))
    qs = (per * 16 + 255) & ~255
    a = 16 * 4 * qs + (max_k * 2 if pro == RMS else 0)
    return max(a, wv * nt * 64 * 16)


def kernel_of(spec, epi, ksplit=0):
    """umoe_grouped_gemm / launch_gemm_nt / use8 / launch_gemm for explicit nt -> (NT, U, WV, BV)"""
    nt, waves, pro = spec["nt"], spec["waves"], spec["pro"]
    max_k, ng = max(q["k"] for q in spec["groups"]), len(spec["groups"])

    def use8(n):
        return waves == 8 if waves else lds_bytes(max_k, n, 4, ksplit) > 80 * 1024

    small = {1: (1, 16), 2: (2, 8), 4: (4, 4)}
    if epi == SWIGLU and pro == RMS:
        k = (2, 8, 4) if nt <= 2 else ((4, 4, 4) if nt == 4 else (8, 2, 4))
    elif epi == SWIGLU:
        assert nt >= 2
        if nt in (2, 4) and waves == 8:
            k = (nt, 1, 8)
        elif nt in (2, 4):
            k = small[nt] + (4,)
        elif nt == 6:
            k = (6, 2, 4)
        elif nt == 14:
            k = (14, 1, 8)
        else:
            k = (8, 2, 8 if use8(8) else 4)
    elif pro == PLAIN and epi == BF16 and waves == 8 and nt in small:
        k = (nt, 2, 8)
    elif nt in small:
        k = small[nt] + (4,)
    else:
        k = (nt, {5: 3, 6: 2, 8: 2}[nt], 8 if use8(nt) else 4)
    NT, _, WV = k
    bv = pro == PLAIN and ((NT <= 2 and WV == 4 and epi != SWIGLU) or (NT == 6 and WV == 8 and epi == BF16)) and ng <= GROUPS_INLINE
    assert lds_bytes(max_k, NT, WV, ksplit, pro) <= 160 * 1024
    return k + (bv,)


def wave_steps(KB, ks, ksplit, U, WV):
    """wstream_body: k-steps [ia, ib) of slab ks and the (i0, i1) of every wave"""
    ia, ib = KB * ks // ksplit, KB * (ks + 1) // ksplit
    out = []
    for w in range(WV):
        if (ib - ia) % U == 0:
            units = (ib - ia) // U
            out.append((ia + U * (units * w // WV), ia + U * (units * (w + 1) // WV)))
        else:
            out.append((ia + (ib - ia) * w // WV, ia + (ib - ia) * (w + 1) // WV))
    return ia, ib, out


def step_cols(k, steps):
    """columns of W / A that MFMA k-steps `steps` contract: chunk i (8 columns) of each K quarter"""
    steps = torch.as_tensor(list(steps), dtype=torch.long)
    return (torch.arange(4)[None, :, None] * (k // 4) + steps[:, None, None] * 8 + torch.arange(8)[None, None, :]).reshape(-1)


def rms_form(k, wv):
    tpr, q8 = 4 * wv, k // 32
    if q8 > 4 * tpr:
        return "two_pass"
    return "butterfly" if (tpr == 32 and q8 == 64) else "single"


# ------------------------------------------------------------------------------------------------ data
def xrange_of(k):
    return 8 if 512 <= k < 2048 else 4


@functools.lru_cache(maxsize=None)
def build(name):
    """CPU buffers of a case.  Out rows: 3 sentinel rows in front of and between the groups' blocks; device groups get out_row_base 2 and
    a row_off; A: every group has a pool of rows + 3 rows, the last one never named (NaN); a_col_off 0 / 8 / 16 inside a wider lda."""
    s = SPEC[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)) + 3)
    kind, sw, pro = s["kind"], s["sw"], s["pro"]
    max_nb = max(q["nb"] for q in s["groups"])
    width = 8 * max_nb if sw else 16 * max_nb
    n_valid = width - s["cut"]
    assert not (sw and s["cut"])
    ldo = (width + 7) // 4 * 4 + (1 if s["ldo"] == "odd" else 0)
    lda = max(8 * (i % 3) + q["k"] for i, q in enumerate(s["groups"])) + 8
    max_k = max(q["k"] for q in s["groups"])
    plan, ob, ab = [], 3, 2
    for q in s["groups"]:
        plan.append((ob, ab))
        ob, ab = ob + q["rows"] + 3, ab + q["rows"] + 3
    RO, RA = ob, ab
    A = torch.full((RA, lda), NAN, dtype=bf16)
    resid = torch.full((RO, ldo), NAN, dtype=bf16)
    nw = None
    if pro == RMS:
        assert len({q["k"] for q in s["groups"]}) == 1
        nw = torch.full((max_k + 64,), NAN, dtype=bf16)
        nw[:max_k] = (1 + 0.1 * torch.randn(max_k, generator=g)).to(bf16)
    groups = []
    share = kind == "p" and len(s["groups"]) > 1          # one permutation over several groups: all of them stage group 0's rows
    if share:
        assert len({(q["rows"], q["k"], q["nb"]) for q in s["groups"]}) == 1 and sum(16 * q["nb"] for q in s["groups"]) == max_k
        whole_perm = torch.randperm(max_k, generator=g)
    for i, (q, (ob, ab)) in enumerate(zip(s["groups"], plan)):
        rows, nb, k = q["rows"], q["nb"], q["k"]
        d = dict(q, ac=8 * (i % 3), orows=ob + torch.arange(rows))
        if share:
            ab, d["ac"] = plan[0][1], 8
        pool, roff = rows + 3, 0
        if q["dev"]:
            d["out_row_base"] = 2
            roff = ob - 2
            d["row_off"], d["count"] = torch.tensor([roff], dtype=torch.int32), torch.tensor([rows], dtype=torch.int32)
        else:
            d["out_row_base"] = ob
        if q["gather"]:
            named = ab + torch.randint(0, pool - 1, (rows,), generator=g)
            if rows > 3:
                named[1], named[2] = named[0], ab + pool - 2                      # a repeated row and one out of order; others are skipped
            lst = torch.full((roff + rows + 9,), ab + pool - 1, dtype=torch.int32)
            lst[roff:roff + rows] = named.to(torch.int32)
            d["rows_list"], d["arows"], d["a_row_base"] = lst, named, 0
        else:
            d["arows"], d["a_row_base"] = ab + torch.arange(rows), ab - roff
        ua = torch.unique(d["arows"])
        N = 8 * nb if sw else min(16 * nb, n_valid)
        d["N"] = N

        def ints(shape, r):
            return torch.randint(-r, r + 1, shape, generator=g).to(f64)
        if kind == "x":
            A[ua[:, None], d["ac"] + torch.arange(k)] = (ints((ua.numel(), k), xrange_of(k)) / 8).to(bf16)
            ws = [(ints((N, k), 4) / 16).to(bf16) for _ in range(2 if sw else 1)]
            b = (ints((N,), 64) / 128).float()
        else:
            if not (share and i):
                A[ua[:, None], d["ac"] + torch.arange(k)] = torch.randn(ua.numel(), k, generator=g).to(bf16)
            if kind == "p":
                d["perm"] = whole_perm[i * N:(i + 1) * N] if share else torch.randperm(k, generator=g)[:N]
                w = torch.zeros(N, k, dtype=bf16)
                w[torch.arange(N), d["perm"]] = 1.0
                ws = [w]
            else:
                ws = [(torch.randn(N, k, generator=g) * k ** -0.5).to(bf16) for _ in range(2 if sw else 1)]
            b = torch.randn(N, generator=g) * 0.5
        d["w"] = ws
        if s["bias"] != "none":
            d["bias"] = b
        resid[d["orows"][:, None], torch.arange(N)] = torch.randn(rows, N, generator=g).to(bf16)
        groups.append(d)
    return dict(spec=s, name=name, kind=kind, sw=sw, pro=pro, A=A, resid=resid, nw=nw, groups=groups, RO=RO, RA=RA, ldo=ldo, lda=lda,
                n_valid=n_valid, max_k=max_k, max_rows=s["max_rows"] or max(q["rows"] for q in s["groups"]))


def a_of(c, d):
    return c["A"][d["arows"]][:, d["ac"]:d["ac"] + d["k"]]


def h_bounds(x, nw, k):
    """RMSNorm prologue in float64 -> (h_lo, h_hi, flagged): h = bf16(nw bf16(x rs))"""
    x, nw = x.to(f64), nw.to(f64)
    rs = ((x * x).sum(-1, keepdim=True) / k + EPS) ** -0.5
    v = x * rs
    w = RS_W * v.abs()
    h1, h2 = rb(nw * rb(v - w)), rb(nw * rb(v + w))
    return torch.minimum(h1, h2), torch.maximum(h1, h2), mid_dist(v) <= w


def ref_of(c):
    """per group: float64 accumulators (acc: one per weight), sum |a w| (ab), the RMSNorm width term (ex), flagged prologue elements"""
    if "ref" in c:
        return c["ref"]
    out = []
    for d in c["groups"]:
        a, k = a_of(c, d), d["k"]
        r = dict(hflag=0, hn=0)
        if c["pro"] == RMS:
            lo, hi, fl = h_bounds(a, c["nw"][:k], k)
            am, ah, aa = (lo + hi) / 2, (hi - lo) / 2, torch.maximum(lo.abs(), hi.abs())
            r["hflag"], r["hn"] = int(fl.sum()), fl.numel()
        else:
            am = a.to(f64)
            ah, aa = torch.zeros_like(am), am.abs()
        r["am"], r["ah"], r["aa"] = am, ah, aa
        if c["kind"] == "p":
            r["acc"], r["ab"], r["ex"] = [am[:, d["perm"]]], [aa[:, d["perm"]]], [ah[:, d["perm"]]]
        else:
            ws = [w.to(f64) for w in d["w"]]
            r["acc"], r["ab"], r["ex"] = [am @ w.t() for w in ws], [aa @ w.abs().t() for w in ws], [ah @ w.abs().t() for w in ws]
        out.append(r)
    c["ref"] = out
    return out


def e32_of(c, k_eff, ab):
    """fp32 summation bound of an accumulator: none for the exact and the permutation data"""
    return k_eff * U32 * ab if c["kind"] == "g" else torch.zeros_like(ab)


def slab_ref(c, d, r, ks, ksplit):
    """(acc, E32) of K-split slab ks"""
    ia, ib, _ = wave_steps(d["k"] // 32, ks, ksplit, 1, 1)
    cols = step_cols(d["k"], range(ia, ib))
    w = d["w"][0].to(f64)[:, cols]
    return r["am"][:, cols] @ w.t(), e32_of(c, cols.numel(), r["aa"][:, cols] @ w.abs().t()), ib - ia


def with_bias(c, d, v, e):
    if "bias" in d:
        v = v + d["bias"].to(f64)
        if c["kind"] == "g":
            e = e + U32 * v.abs()
    return v, e


def lin_interval(c, d, r, epi):
    """(centre, half width) of a group's outputs in a linear epilogue without ksplit"""
    v, e = with_bias(c, d, r["acc"][0], e32_of(c, d["k"], r["ab"][0]) + r["ex"][0])
    if epi == RAW:
        return v, e
    if epi == RESID:
        return interval_resid(v, e, c["resid"][d["orows"][:, None], torch.arange(d["N"])])
    return interval(v, e)


def swiglu_interval(c, d, r):
    """(centre, half width, flagged) of y: the hull of swiglu_y over the ends of the gate's and the up's BF16 intervals"""
    ends = []
    for j in range(2):
        v, e = r["acc"][j], e32_of(c, d["k"], r["ab"][j]) + r["ex"][j]
        ends.append((rb(v - e), rb(v + e)))
    (glo, ghi), (ulo, uhi) = ends
    gm = torch.minimum(torch.maximum(rb(torch.full_like(glo, G0)), glo), ghi)
    lo = hi = flag = None
    for gt in (glo, ghi, gm):
        for up in (ulo, uhi):
            mid, half, fl = swiglu_y(gt, up)
            lo = mid - half if lo is None else torch.minimum(lo, mid - half)
            hi = mid + half if hi is None else torch.maximum(hi, mid + half)
            flag = fl if flag is None else flag | fl
    return (lo + hi) / 2, (hi - lo) / 2, flag | (glo == 0)


# ------------------------------------------------------------------------------------------------ emulation of wstream_body
def out_dtype(epi):
    return torch.float32 if epi in (F32, RAW) else bf16


def new_out(c, epi, ksplit, device="cpu"):
    shape = (c["RO"] + 2 * MARGIN, c["ldo"])
    return torch.full(((max(ksplit, 1),) + shape) if ksplit > 1 else shape, SENT, dtype=out_dtype(epi), device=device)


def _bfly(v, n):
    idx = torch.arange(n)
    o = n // 2
    while o >= 1:
        v = v + v[..., idx ^ o]
        o //= 2
    return v[..., 0]


def emu_rs(x, k, wv, short=False):
    """rs of the staging code in fp32 with its summation tree (rms_form)"""
    tpr, q8, rows = 4 * wv, k // 32, x.shape[0]
    sq = (x.float() * x.float()).view(rows, 4, q8, 8).clone()
    if short:
        sq[:, 3, -4:, :] = 0.0                                    # planted: the sum misses 32 elements
    form, sub = rms_form(k, wv), torch.arange(tpr)
    if form == "butterfly":
        cs = torch.zeros(rows, 4, q8)
        for j in range(8):
            cs = cs + sq[..., j]
        q4 = _bfly(cs[:, :, :32] + cs[:, :, 32:], 32)
        ss = ((q4[:, 0] + q4[:, 1]) + q4[:, 2]) + q4[:, 3]
    else:
        t = torch.zeros(rows, tpr)
        if form == "single":
            chunks = [(n >> 2, sub + tpr * (n & 3), q8) for n in range(16)]
            src = sq
        else:
            chunks = [(0, c0 + sub, 4 * q8) for c0 in range(0, 4 * q8, tpr)]
            src = sq.view(rows, 1, 4 * q8, 8)
        for h, i, lim in chunks:
            own = (i < lim)[None, :]
            for j in range(8):
                t = t + torch.where(own, src[:, h, i.clamp(max=lim - 1), j], torch.zeros(()))
        ss = _bfly(t, tpr)
    return torch.rsqrt(ss / torch.tensor(float(k)) + torch.tensor(EPS, dtype=torch.float32))[:, None]


PLANTS = ("drop_step", "dup_step", "swap_chunks", "quarter_neighbour", "bias_twice", "resid_first", "col_nvalid", "tail_tile", "row_behind",
          "swap_gate_up", "rs_short")


def emu(c, epi, ksplit=0, plant=None, pg=0):
    """the launch in fp32 / bf16 torch arithmetic -> the whole output buffer (margins included).  plant (on group pg): a wrong kernel"""
    s = c["spec"]
    _, U, WV, _ = kernel_of(s, epi, ksplit)
    ksn = max(ksplit, 1)
    big = new_out(c, epi, ksplit)
    slabs = big if ksplit > 1 else big[None]
    for gi, d in enumerate(c["groups"]):
        hit = plant if gi == pg else None
        rows, k, N = d["rows"], d["k"], d["N"]
        if rows == 0:
            continue
        a = a_of(c, d)
        if c["pro"] == RMS:
            rs = emu_rs(a, k, WV, short=hit == "rs_short")
            a = (c["nw"][:k].float() * rbf32(a.float() * rs)).to(bf16)
        if hit == "swap_chunks":                                  # two 16-byte chunks of the first row staged in each other's place
            a = a.clone()
            a[0, 0:8], a[0, 8:16] = a[0, 8:16].clone(), a[0, 0:8].clone()
        elif hit == "quarter_neighbour":                          # K quarter 1 of every row taken from the row behind it
            a, q = a.clone(), k // 4
            a[:-1, q:2 * q] = a[1:, q:2 * q].clone()
        orow = MARGIN + d["orows"]
        at = (orow[:, None], torch.arange(N))
        for ks in range(ksn):
            _, _, waves = wave_steps(k // 32, ks, ksn, U, WV)
            busy = [w for w, (i0, i1) in enumerate(waves) if i1 > i0]
            accs = []
            for w_ in d["w"]:
                acc = torch.zeros(rows, N)
                for w, (i0, i1) in enumerate(waves):
                    steps = list(range(i0, i1))
                    if busy and w == busy[-1] and ks == ksn - 1:
                        if hit == "drop_step":
                            steps = steps[:-1]
                        elif hit == "dup_step":                   # MFMA ignores EXEC: a guarded step of a partial chunk run on its clamped operands
                            steps = steps + steps[-1:]
                    if steps:
                        cols = step_cols(k, steps)
                        acc = acc + a[:, cols].float() @ w_[:, cols].float().t()
                accs.append(acc)
            o = slabs[ks]
            if epi == SWIGLU:
                gt, up = rbf32(accs[0]), rbf32(accs[1])
                if hit == "swap_gate_up":
                    gt, up = up, gt
                o[at] = (rbf32(gt / (1.0 + torch.exp(-gt))) * up).to(bf16)
            else:
                v = accs[0]
                if "bias" in d and ks == 0:
                    v = v + d["bias"] * (2 if hit == "bias_twice" else 1)
                if epi == RAW:
                    o[at] = v
                elif epi == F32:
                    o[at] = rbf32(v)
                elif epi == BF16:
                    o[at] = v.to(bf16)
                else:
                    r = c["resid"][d["orows"][:, None], torch.arange(N)].float()
                    o[at] = (r + v).to(bf16) if hit == "resid_first" else (r + rbf32(v)).to(bf16)
            if hit == "row_behind":
                o[orow[-1] + 1, :N] = o[orow[-1], :N]
            elif hit == "col_nvalid":
                assert N == c["n_valid"] < c["ldo"]
                o[orow[0], N] = 0.5
            elif hit == "tail_tile":                              # the tile behind the group's last block stored: it re-read that block
                lim = c["ldo"] if c["sw"] else c["n_valid"]
                n1 = min(N + (8 if c["sw"] else 16), lim)
                assert n1 > N
                o[orow[:, None], torch.arange(N, n1)] = o[orow[:, None], torch.arange(N - (n1 - N), N)]
    return big


# ------------------------------------------------------------------------------------------------ the checker
def check_case(c, epi, ksplit, big, stats):
    """every element of every group against its interval, everything else against the sentinel -> flagged share (SwiGLU, RMSNorm)"""
    ref = ref_of(c)
    big = big.detach().cpu()
    slabs = big if ksplit > 1 else big[None]
    RO = c["RO"]
    keeps_sentinel(f"{c['name']}: rows around the output window", torch.cat([slabs[:, :MARGIN], slabs[:, MARGIN + RO:]], 1))
    outs = slabs[:, MARGIN:MARGIN + RO]
    written = torch.zeros((RO, c["ldo"]), dtype=torch.bool)
    n_flag = n_all = 0
    tag = EPI_NAME[epi]
    for d, r in zip(c["groups"], ref):
        if d["rows"] == 0:
            continue
        at = (d["orows"][:, None], torch.arange(d["N"]))
        written[at] = True
        n_flag, n_all = n_flag + r["hflag"], n_all + r["hn"]
        if epi == SWIGLU:
            mid, half, flag = swiglu_interval(c, d, r)
            check(tag, outs[0][at], mid, half, stats)
            n_flag, n_all = n_flag + int(flag.sum()), n_all + flag.numel()
        elif ksplit > 1:
            assert epi == RAW
            tot = torch.zeros(d["rows"], d["N"])
            for ks in range(ksplit):
                v, e, steps = slab_ref(c, d, r, ks, ksplit)
                if ks == 0:
                    v, e = with_bias(c, d, v, e)
                got = outs[ks][at]
                check(f"slab/{ksplit}", got, v, e, stats)
                if steps == 0 and not (ks == 0 and "bias" in d):
                    assert bool((got == 0).all()), "a K slice of no steps must store exact zeros"
                tot = tot + got
            v, e = with_bias(c, d, r["acc"][0], e32_of(c, d["k"] + ksplit, r["ab"][0]))
            check(f"sum/{ksplit}", tot, v, e, stats)
        elif epi == BF16 and c["kind"] == "g" and "bias" not in d and c["pro"] == PLAIN:
            check_bf16(tag, outs[0][at], r["acc"][0], e32_of(c, d["k"], r["ab"][0]), stats)
        else:
            check("acc" if epi == RAW else tag, outs[0][at], *lin_interval(c, d, r, epi), stats)
    for ks in range(slabs.shape[0]):
        keeps_sentinel(f"{c['name']} {tag}: output outside every group's window (slab {ks})", outs[ks][~written])
    return n_flag / max(n_all, 1)


def flag_limit(c):
    return 2e-2 if c["sw"] and c["kind"] == "x" else 1e-3


# ------------------------------------------------------------------------------------------------ the launch
def launch(c, epi, ksplit, dev):
    from unimoe_audio_amd import ops
    s = c["spec"]
    if "dv" not in c:
        def window(t, front, back, fill):
            buf = torch.full((front + t.shape[0] + back,) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=dev)
            buf[front:front + t.shape[0]] = t.to(dev)
            return buf, buf[front:front + t.shape[0]]
        dv = dict(groups=[])
        dv["A"] = window(c["A"], 2, 2, NAN)
        dv["resid"] = window(c["resid"], MARGIN, MARGIN, NAN)
        if c["nw"] is not None:
            dv["nw"] = c["nw"].to(dev)
        for d in c["groups"]:
            t = {key: d[key].to(dev) for key in ("row_off", "count", "rows_list") if key in d}
            ws = [w.to(dev) for w in d["w"]]
            packed = ops.pack_gate_up(ws[0], ws[1]) if c["sw"] else ops.pack_weight(ws[0])
            t["w"] = window(packed, 512, 512, NAN)                # 1 KiB of NaN on either side of the packed weight
            if "bias" in d:
                off = 4 if s["bias"] == "al" else 5
                bb = torch.full((off + 16 * d["nb"] + 8,), NAN, device=dev)
                bb[off:off + d["N"]] = d["bias"].to(dev)
                t["bias"] = (bb, bb[off:off + 16 * d["nb"]])
                assert (t["bias"][1].data_ptr() % 16 == 0) == (s["bias"] == "al")
            dv["groups"].append(t)
        c["dv"] = dv
    dv = c["dv"]
    groups = []
    for d, t in zip(c["groups"], dv["groups"]):
        q = dict(w=t["w"][1], n_blocks=d["nb"], k=d["k"], a_row_base=d["a_row_base"], out_row_base=d["out_row_base"], a_col_off=d["ac"])
        if "bias" in t and epi != SWIGLU:
            q["bias"] = t["bias"][1]
        if d["dev"]:
            q.update(row_off=t["row_off"], count=t["count"])
        else:
            q["static_count"] = d["rows"]
        if d["gather"]:
            q["rows"] = t["rows_list"]
        groups.append(q)
    tab = ops.GroupTable(groups, dev)
    big = new_out(c, epi, ksplit, dev)
    out = (big[0] if ksplit > 1 else big)[MARGIN:MARGIN + c["RO"]]
    ops.grouped_gemm(tab, dv["A"][1], out, max_rows=c["max_rows"], prologue=c["pro"], epilogue=epi,
                     norm_w=dv["nw"][:c["max_k"]] if c["pro"] == RMS else None, rms_eps=EPS, resid=dv["resid"][1] if epi == RESID else None,
                     n_valid=c["n_valid"], nt=s["nt"], waves=s["waves"], ksplit=ksplit, part_stride=big.stride(0) if ksplit > 1 else 0)
    return big


def runs_of(s):
    return [(epi, ks) for epi in s["epis"] for ks in s["ksplits"]]


def run_case(name, dev):
    c = build(name)
    st, share = Stats(), 0.0
    kernels = []
    for epi, ks in runs_of(c["spec"]):
        NT, U, WV, bv = kernel_of(c["spec"], epi, ks)
        kernels.append(f"{NT},{U},{WV}" + ("v" if bv else ""))
        share = max(share, check_case(c, epi, ks, launch(c, epi, ks, dev), st))
    st.show(f"{name} <{' '.join(sorted(set(kernels)))}> flagged {share:.2e}")
    assert share <= flag_limit(c), share


# ================================================================================================ checkers without a GPU
def bits(t):
    return t.view(torch.int16 if t.dtype == bf16 else torch.int32)


def _rejects(fn):
    with pytest.raises(AssertionError):
        fn()


def test_coverage_cpu():
    """the case list reaches every instantiation of the issue's table and both sides of every predicate of the dispatch and the body"""
    reached, seen = {}, {}

    def note(key, val):
        seen.setdefault(key, set()).add(val)
    for s in CASES:
        ng = len(s["groups"])
        note("descriptors from memory", ng > GROUPS_INLINE)
        if ng > GROUPS_INLINE:
            note("from memory: epilogue", s["epis"][0])
        note("ldo % 4 == 0", s["ldo"] == "v")
        note("bias", s["bias"])
        note("cut", s["cut"])
        for epi, ks in runs_of(s):
            NT, U, WV, bv = kernel_of(s, epi, ks)
            reached.setdefault((s["pro"], epi), set()).add((NT, U, WV))
            note("BV", bv)
            if not s["waves"] and NT >= 5 and NT != 14 and not (epi == SWIGLU and (s["pro"] == RMS or NT == 6)):
                note("use8 by LDS", WV == 8)
            if epi == RESID:
                note("resid vector path", s["ldo"] == "v")
            for q in s["groups"]:
                note("ragged", bool(q["dev"] or q["gather"]))
                note(("tail tile", NT > 1), q["nb"] % NT != 0)
                if s["pro"] == RMS:
                    note("rms form", rms_form(q["k"], WV))
                for k_ in range(max(ks, 1)):
                    ia, ib, waves = wave_steps(q["k"] // 32, k_, max(ks, 1), U, WV)
                    note("(ib - ia) % U == 0", (ib - ia) % U == 0)
                    note("idle wave", any(i0 == i1 for i0, i1 in waves))
                    if ks > 1:
                        note("empty slab", ib == ia)
                    if U >= 4:
                        for i0, i1 in waves:
                            for i in range(i0, i1, U):
                                note("whole chunk (U >= 4)", i + U <= i1)
    for key, want in REQUIRED.items():
        assert want <= reached.get(key, set()), (key, want - reached.get(key, set()))
    for key in ("descriptors from memory", "ldo % 4 == 0", "BV", "use8 by LDS", "resid vector path", "ragged", ("tail tile", True), "(ib - ia) % U == 0",
                "idle wave", "empty slab", "whole chunk (U >= 4)"):
        assert seen[key] == {True, False}, (key, seen[key])
    assert seen["from memory: epilogue"] == {BF16, SWIGLU} and seen["bias"] == {"none", "al", "off1"} and seen["cut"] == {0, 1, 3, 13}
    assert seen["rms form"] == {"single", "butterfly", "two_pass"}
    # the issue's shape lists
    allg = [q for s in CASES for q in s["groups"]]
    assert {32, 96, 128, 512, 2048, 2080, 1376, 2752, 4096} <= {q["k"] for q in allg}
    assert {1, 15, 16, 17, 33} <= {q["rows"] for q in allg if not q["dev"]}
    for ga in (False, True):
        assert {0, 1, 16, 17} <= {q["rows"] for q in allg if q["dev"] and q["gather"] == ga}
    assert all(max(q["rows"] for q in s["groups"]) <= 40 and (s["max_rows"] or 0) <= 40 for s in CASES)
    assert all(s["max_rows"] > max(q["rows"] for q in s["groups"]) for s in CASES if s["name"].startswith("x_ragged"))
    assert any(q["nb"] == 30 for q in SPEC["xs_nt14"]["groups"])
    assert all(16 * q["nb"] * q["k"] * 2 <= 8.7e6 for q in allg)
    for name in ("x_ksplit", "x_ksplit_nt8"):
        assert set(SPEC[name]["ksplits"]) == {2, 3, 4}
        assert any(all((q["k"] // 32) % n for n in (2, 3, 4)) for q in SPEC[name]["groups"]) and any(q["k"] == 64 for q in SPEC[name]["groups"])
    # permutation cases read every column of the staged rows back (N = K, over the groups of a launch where one weight would pass 8 MB)
    for s in CASES:
        if s["kind"] == "p":
            c = build(s["name"])
            named = torch.cat([d["perm"] for d in c["groups"]])
            assert torch.equal(torch.sort(named).values, torch.arange(c["max_k"])), s["name"]
            assert len({(tuple(d["arows"].tolist()), d["ac"]) for d in c["groups"]}) == 1, s["name"]
    # two SwiGLU K's per flagged-share figure of the issue
    assert {32, 96, 512, 2048, 2752, 4096} <= {q["k"] for s in CASES if s["sw"] and s["kind"] == "x" for q in s["groups"]}


def test_exact_preconditions_cpu():
    """exact data: operands are the stated integer multiples, max sum |x w| 2^7 (+ |bias| 2^7) < 2^24; at K >= 512 at least 5 % of the
    accumulators of a case (all its groups with K >= 512 together) need the bf16 rounding"""
    for s in CASES:
        if s["kind"] != "x":
            continue
        c = build(s["name"])
        n_round = n_acc = 0
        for d, r in zip(c["groups"], ref_of(c)):
            if d["rows"] == 0:
                continue
            a = a_of(c, d).to(f64)
            assert torch.equal(a * 8, torch.round(a * 8)) and float(a.abs().max()) <= xrange_of(d["k"]) / 8
            for w, ab, acc in zip(d["w"], r["ab"], r["acc"]):
                w = w.to(f64)
                assert torch.equal(w * 16, torch.round(w * 16)) and float(w.abs().max()) <= 0.25
                top = ab.max() * 128
                if "bias" in d:
                    b = d["bias"].to(f64)
                    assert torch.equal(b * 128, torch.round(b * 128))
                    top = top + b.abs().max() * 128
                assert float(top) < 2 ** 24, (s["name"], float(top))
                assert torch.equal(acc * 128, torch.round(acc * 128))
                if d["k"] >= 512:
                    n_round, n_acc = n_round + int((rb(acc) != acc).sum()), n_acc + acc.numel()
        assert n_round >= 0.05 * n_acc, (s["name"], n_round, n_acc)


def test_emulation_passes_cpu():
    """the emulation of wstream_body passes every checker for every case; flagged shares stay under their limits; prints the worst
    |rs_fp32 - rs_float64| / (8 u rs) of the three summation trees"""
    st, worst_rs, flagged = Stats(), {}, {}
    for s in CASES:
        c = build(s["name"])
        share = 0.0
        for epi, ks in runs_of(s):
            share = max(share, check_case(c, epi, ks, emu(c, epi, ks), st))
            if s["pro"] == RMS:
                WV = kernel_of(s, epi, ks)[2]
                for d in c["groups"]:
                    x = a_of(c, d)
                    rs64 = ((x.to(f64) ** 2).sum(-1, keepdim=True) / d["k"] + EPS) ** -0.5
                    ratio = float(((emu_rs(x, d["k"], WV).to(f64) - rs64).abs() / (RS_W * rs64)).max())
                    form = rms_form(d["k"], WV)
                    worst_rs[form] = max(worst_rs.get(form, 0.0), ratio)
        assert share <= flag_limit(c), (s["name"], share)
        flagged[s["name"]] = share
    assert max(st.values()) <= 1.0
    assert max(worst_rs.values()) <= 1.0, worst_rs
    st.show("emulated cases")
    print("WSTREAM FP64 flagged share per case:", ", ".join(f"{k} {v:.3g}" for k, v in flagged.items() if v))
    print("WSTREAM FP64 rs ratio per staging form:", ", ".join(f"{k} {v:.3g}" for k, v in worst_rs.items()))


# (plant, case, epilogue, ksplit, group)
PLANTED = [
    ("drop_step", "x_nt1", RAW, 0, 0), ("drop_step", "x_nt2", BF16, 0, 2), ("drop_step", "x_ksplit", RAW, 3, 0), ("drop_step", "xs_nt14", SWIGLU, 0, 1),
    ("drop_step", "p_plain_2080", BF16, 0, 0), ("drop_step", "g_nt8", RAW, 0, 0),
    ("dup_step", "x_nt2", BF16, 0, 0), ("dup_step", "x_nt8", F32, 0, 0), ("dup_step", "x_ksplit_nt8", RAW, 2, 0), ("dup_step", "xs_nt4", SWIGLU, 0, 1),
    ("dup_step", "p_plain_1376", BF16, 0, 0),
    ("swap_chunks", "x_nt1", BF16, 0, 0), ("swap_chunks", "p_plain_96", BF16, 0, 0), ("swap_chunks", "p_rms_2048", BF16, 0, 0),
    ("quarter_neighbour", "x_nt8", RAW, 0, 2), ("quarter_neighbour", "p_plain_2048", BF16, 0, 0), ("quarter_neighbour", "xs_nt2", SWIGLU, 0, 0),
    ("bias_twice", "x_nt1", BF16, 0, 0), ("bias_twice", "x_nt2", RESID, 0, 1), ("bias_twice", "x_ksplit", RAW, 2, 1), ("bias_twice", "g_nt1", F32, 0, 0),
    ("resid_first", "x_nt1", RESID, 0, 0), ("resid_first", "x_ragged", RESID, 0, 3),
    ("col_nvalid", "x_nt1", BF16, 0, 0), ("col_nvalid", "x_nt2", RAW, 0, 0), ("col_nvalid", "x_nt8", RESID, 0, 0),
    ("tail_tile", "x_nt2", BF16, 0, 1), ("tail_tile", "x_nt8", RAW, 0, 2), ("tail_tile", "xs_nt4", SWIGLU, 0, 0), ("tail_tile", "x_ragged", F32, 0, 1),
    ("row_behind", "x_nt1", BF16, 0, 1), ("row_behind", "x_ragged", RAW, 0, 3), ("row_behind", "xs_mem13", SWIGLU, 0, 1), ("row_behind", "x_ksplit", RAW, 4, 1),
    ("swap_gate_up", "xs_nt2", SWIGLU, 0, 0), ("swap_gate_up", "gs_nt4", SWIGLU, 0, 0), ("swap_gate_up", "gs_rms_nt8", SWIGLU, 0, 0),
    ("rs_short", "p_rms_96", BF16, 0, 0), ("rs_short", "p_rms_bfly", F32, 0, 0), ("rs_short", "p_rms_2752", BF16, 0, 0), ("rs_short", "p_rms_4096", BF16, 0, 0),
    ("rs_short", "p_rms_2752w8", BF16, 0, 0),
]


def test_planted_errors_cpu():
    """each planted error of the issue's list is rejected (the unplanted emulation of the same run passes: test_emulation_passes_cpu)"""
    assert {p[0] for p in PLANTED} == set(PLANTS)
    for plant, name, epi, ks, pg in PLANTED:
        c = build(name)
        assert (epi, ks) in runs_of(c["spec"]), (plant, name)
        bad = emu(c, epi, ks, plant, pg)
        assert not torch.equal(bits(bad), bits(emu(c, epi, ks))), (plant, name, "the plant changed nothing")
        with pytest.raises(AssertionError):
            check_case(c, epi, ks, bad, Stats())
            pytest.fail(f"planted error {plant} in {name} / {EPI_NAME[epi]} was accepted", pytrace=False)
    # a NaN let through, and a single bf16 ulp on an exact element
    c = build("x_nt1")
    good = emu(c, BF16, 0)
    d = c["groups"][0]
    bad = good.clone()
    bad[MARGIN + d["orows"][3], 5] = NAN
    _rejects(lambda: check_case(c, BF16, 0, bad, Stats()))
    bad = good.clone()
    v = bad[MARGIN + d["orows"][3], 5].to(f64)
    bad[MARGIN + d["orows"][3], 5] = float(v + ulp_bf16(v))
    _rejects(lambda: check_case(c, BF16, 0, bad, Stats()))
    # bias in every slab (the defect this file found): slab 1 of the parent commit
    c = build("x_ksplit")
    bad = emu(c, RAW, 2)
    d = c["groups"][0]
    bad[1][MARGIN + d["orows"][:, None], torch.arange(d["N"])] += d["bias"]
    _rejects(lambda: check_case(c, RAW, 2, bad, Stats()))


# ================================================================================================ GPU tests
@gpu
@pytest.mark.parametrize("name", [s["name"] for s in CASES if s["kind"] == "x"])
def test_wstream_exact_vs_fp64(dev, name):
    """exact data: every output bit for bit (SwiGLU: outside the flagged elements), in every instantiation of REQUIRED, static and ragged
    rows, tail tiles, dead workgroups, n_valid cuts, odd ldo, bias absent / aligned / offset, K-split slabs with the bias in slab 0"""
    run_case(name, dev)


@gpu
@pytest.mark.parametrize("name", [s["name"] for s in CASES if s["kind"] == "p"])
def test_wstream_permutation_vs_fp64(dev, name):
    """permutation weights: the staged tile read back -- x[:, perm] bit for bit, or the RMSNorm prologue's h per element"""
    run_case(name, dev)


@gpu
@pytest.mark.parametrize("name", [s["name"] for s in CASES if s["kind"] == "g"])
def test_wstream_gaussian_vs_fp64(dev, name):
    """Gaussian data: every output inside its interval; prints the acc ratio |F32_RAW - ref| / E32"""
    run_case(name, dev)
