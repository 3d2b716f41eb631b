"""The tiled MFMA GEMM family -- umoe_tiled_gemm (NT: tgemm_kernel and tgemm_pp_kernel, csrc/umoe_tgemm.hip), its k-major form
(tgemm_nn_kernel) and umoe_tiled_gemm_tn with tn_reduce_kernel (csrc/umoe_tgemm_tn.hip) -- per element against a float64 product
on the CPU of the same input bits, at every tile edge.

Rules of the whole file
  * reference: float64.  bf16 x bf16 products are exact in fp32, so the only fp32 error of an accumulator is its summation:
      E32 = K_eff u sum_k |a_k w_k|,  u = 2^-24,  for ANY summation order (round-to-nearest adds inside and between MFMAs);
      K_eff = the contraction length, + k_split for a split TN product (the fixed-order sum of the partials);
      + u |acc + bias| where a bias is added.
  * comparison: per element, never a norm.  Every epilogue but SwiGLU is a monotone map of the accumulator, so an output has an
    INTERVAL and no flagged elements:
      BF16, F32      out in [bf16(ref - E32), bf16(ref + E32)]
      F32_RAW        |out - ref| <= E32
      BF16_RESID     lo = bf16(ref - E32), hi = bf16(ref + E32): out in [bf16(fp32(r + lo)), bf16(fp32(r + hi))], the double rounding
                     include/umoe.h documents
      TN, NN         the BF16 interval
    (an interval [lo, hi] is handed to `check` as |out - (lo + hi) / 2| <= (hi - lo) / 2: both exact in float64)
  * SwiGLU: the stored pre-activations (aux_out: gate | up) get the BF16 interval; y is checked against the KERNEL'S OWN gate / up
    bits: y = bf16(bf16(silu(g)) u) with silu in float64, rounded where tg_epilogue rounds.  The only slack is the fp32 error of
    g / (1 + expf(-g)): 8 u |silu|.  An element whose float64 silu lies within that window of a bf16 midpoint is flagged and may
    take either neighbour (one bf16 ulp of silu, propagated through the product); at most 1e-3 of a case's elements may be flagged
    (checked without a GPU on the reference's gates for every case the GPU tests run).  The same launch with aux_out = NULL (the
    inference path) must give bit-identical y.
  * untouched memory: outputs are prefilled with a sentinel (7.0); rows behind a group's count, padding rows between 8-aligned
    groups, columns outside [out_col_off, out_col_off + n) of a wider ldo, rows of nobody and the columns beyond 2n of a wider
    ld_aux keep it bit for bit.
  * unread memory: operands are windows of wider buffers and everything the header says is not read holds NaN: activation rows
    behind the count, rows a gather list does not name, columns outside [a_col_off, a_col_off + k), weight rows >= n and columns
    >= k, bias entries >= n, the residual outside the output window, rows outside a TN K window, the TN surplus columns up to
    roundup8(m) / roundup8(n), rows of a k-major weight behind k (a view into a taller buffer).  The k-major activation's last
    8-column chunk holds zeros (train._pad8).  Any NaN in an output fails.
  * dispatch: launch_tgemm's predicates (max_rows >= 1024, tgemm_pp_pays) are restated (kernel_of) and test_dispatch_cpu asserts
    that the case lists lie on both sides of them.  No variant is forced through the environment.
    tgemm_kernel<EPI, 8, 4, 3> (256-token tiles of the small kernel) is UNREACHABLE with the default UMOE_TGEMM_PP=2: tgemm_tm
    wants ceil(rows / 256) ceil(n / 128) G >= 512 workgroups, and since ceil(n / 128) <= 2 ceil(n / 256) that means
    ceil(rows / 256) ceil(n / 256) G >= 256 >= 128, where tgemm_pp_pays has already taken the launch (SwiGLU alike with 64 / 128).
    test_dispatch_cpu checks the implication over a grid of shapes.  The code stays in this change.
Every GPU test prints its worst error / bound under -s ("GEMM FP64 ..."); a ratio above 1 fails.  A bf16 interval is usually one
value, so the interval ratios are 0 or 1; "acc" is the informative figure: |F32_RAW output - ref| / E32.

The checkers are tested without a GPU (test_*_cpu): an fp32 / bf16 torch emulation of the kernel's arithmetic (K summed in tiles of
32, the epilogue's rounding points) passes for every case, and each planted error is rejected.

Found by this file
  * tgemm_nn_kernel with w2 and k_w1 < 96 (no product shape: k_w1 is an intermediate size): the running weight pointer of the steady
    loop was re-based onto w2 only when the loop REACHED tile k_w1 / 32, but the loop starts at tile 3 (the prologue stages tiles
    0..2).  With k_w1 = 32 or 64 and k > 128 tiles 3..KT-2 came from rows 96.. of w instead of w2: wrong sums and reads behind w's
    k_w1 rows.  Case nn_seam group 2 (k_w1 = 32, k = 161) shows it (NaN from the rows behind k_w1); fixed in umoe_tgemm_tn.hip.

Measured on an MI355X (the whole file: 20 GPU tests in 2 s on the card; the four tests without a GPU in 4 s).  Every interval ratio
that -s prints is 0 or 1 -- an output sits in its interval, which is one bf16 value for all but about 1e-4 of the elements; every
test reports 1 for each of its epilogues, except where noted -- so the table gives per test "acc" / "acc+b", the worst
|F32_RAW output - ref| / E32 without / with bias, and "off", the share of outputs that are not the bf16 nearest to the float64 value
itself (expected: about E32 / ulp; bias-free BF16 epilogue, aux_out gate / up, TN and NN outputs):
  tgemm_kernel
    odd_ldo              acc 0.020, acc+b 0.028; off 8.8e-5
    ldo8                 acc 0.020, acc+b 0.020; off 1.1e-4
    ldo4                 acc 0.109, acc+b 0.187 (the k = 8 group); off 6.0e-5
    ragged               acc 0.019, acc+b 0.020; off 0; SwiGLU: aux off 0 / 1.7e-4, y ratio 0 (every interval one value, all met), flagged 0
    swiglu               aux off 1.5e-4 / 8.1e-5, flagged 8.3e-5
    rows1025_few_tiles   acc 0.019, acc+b 0.024; off 8.6e-5; SwiGLU: aux off 8.6e-5 / 6.5e-5, flagged 3.6e-5
  tgemm_pp_kernel
    pp_static            acc 0.170, acc+b 0.433
    pp_ldo4              acc 0.167, acc+b 0.373; SwiGLU: aux off 5.3e-5 / 5.1e-5, flagged 9.0e-5
    pp_ragged            acc 0.150, acc+b 0.267
    ppsw_static          aux off 8.6e-5 / 8.1e-5, flagged 1.0e-4
    ppsw_ldaux4          aux off 5.5e-5 / 3.3e-5, flagged 7.7e-5
    ppsw_ragged          aux off 1.6e-4 / 1.2e-4, flagged 7.9e-5
    (acc is set by the k = 8 groups, where 8 u sum|a w| is a small bound; acc+b by the groups whose bias dominates: the one rounding
    of the add is half an ulp against a bound of one.  y without aux_out is bit-identical to y with it in every SwiGLU case, the LDS
    epilogue against direct stores included.)
  tgemm_nn_kernel
    nn_static            off 7.6e-5
    nn_seam              off 9.4e-5   (before the fix in umoe_tgemm_tn.hip: NaN in group 2, see above)
    nn_ragged            off 6.3e-5
  tgemm_tn_kernel (+ tn_reduce_kernel)
    tn_static            off 0 - 4.6e-5 over the windows of 0 - 300 rows; the empty window: ratio 0, exact zeros
    tn_device            off 0 - 7.8e-5; the empty window exact zeros
    tn_device_empty      ratio 0, exact zeros
    tn_split             k_split 2, 3, 4: off 0 - 4.6e-5 with K_eff = K + k_split
    tn_auto              the library chose 2; off 1.3e-4
No accumulator came near its bound (worst 0.17 without a bias): nothing speaks against round-to-nearest adds inside and between the
MFMAs, u stays 2^-24.
"""
import functools

import pytest
import torch

from test_gpu_bwd_fp64 import Stats as _Stats, check, keeps_sentinel, mid_dist, rbf, ulp_bf16

gpu = pytest.mark.gpu

U = 2.0 ** -24          # fp32 unit roundoff
SILU_W = 8 * U          # fp32 error of g / (1 + expf(-g)), relative
SENT = 7.0
NAN = float("nan")
f64 = torch.float64
bf16 = torch.bfloat16
BF16, RESID, SWIGLU, F32, RAW = 0, 1, 2, 3, 4          # UMOE_EPI_*
EPI_NAME = {BF16: "bf16", RESID: "resid", SWIGLU: "swiglu", F32: "f32", RAW: "raw"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from unimoe_audio_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


class Stats(_Stats):
    """the dict holds error / bound ratios only; the "off" shares are kept apart in .shares"""
    prefix = "GEMM FP64"

    def share(self, name, v):
        self.__dict__.setdefault("shares", {})
        self.shares[name] = max(self.shares.get(name, 0.0), float(v))

    def show(self, title):
        shares = self.__dict__.get("shares", {})
        print(f"\n{self.prefix} {title}: " + ", ".join(f"{k} {v:.3g}" for k, v in self.items()) +
              (" | off: " + ", ".join(f"{k} {v:.3g}" for k, v in shares.items()) if shares else ""))


# ------------------------------------------------------------------------------------------------ helpers
def r8(n):
    return (n + 7) & ~7


def cdiv(a, b):
    return -(-a // b)


def rb(x):
    """float64 -> nearest bf16 (ties to even), exactly (rbf goes through fp32: a second rounding)"""
    ul = ulp_bf16(x)
    return torch.round(x / ul) * ul


def interval(v, e):
    """[bf16(v - e), bf16(v + e)] as (centre, half width)"""
    lo, hi = rb(v - e), rb(v + e)
    return (lo + hi) / 2, (hi - lo) / 2


def interval_resid(v, e, r):
    lo, hi = rb(v - e), rb(v + e)
    lo2 = (r.float() + lo.float()).to(bf16).to(f64)          # fp32(r + lo) is one fp32 add of two bf16 values, as in the kernel
    hi2 = (r.float() + hi.float()).to(bf16).to(f64)
    return (lo2 + hi2) / 2, (hi2 - lo2) / 2


def swiglu_y(gate, up):
    """y = bf16(bf16(silu(g)) u) from gate / up BITS -> (centre, half width, flagged): silu in float64; its fp32 value lies within
    8 u |silu|, so bf16(silu) is one of rb(silu -+ window) -- two values only for a flagged element -- and s u is exact in fp32."""
    g, u = gate.to(f64), up.to(f64)
    silu = g * torch.sigmoid(g)
    w = SILU_W * silu.abs()
    y1, y2 = rb(rb(silu - w) * u), rb(rb(silu + w) * u)
    lo, hi = torch.minimum(y1, y2), torch.maximum(y1, y2)
    return (lo + hi) / 2, (hi - lo) / 2, mid_dist(silu) <= w


def check_bf16(name, got, v, e, stats):
    """the BF16 interval of (v, e); also notes the share of outputs that are not the bf16 nearest to v itself ("off": about E32 / ulp)"""
    check(name, got, *interval(v, e), stats)
    if got.numel():
        stats.share(name, float((got.detach().cpu().to(f64) != rb(v)).double().mean()))


def randbf(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(bf16)


# ------------------------------------------------------------------------------------------------ case lists (specs only: no data)
def G(rows, n, k, oc=0, ac=0, dev=False, gather=False, k_w1=0):
    return dict(rows=rows, n=n, k=k, oc=oc, ac=ac, dev=dev, gather=gather, k_w1=k_w1)


# 1. tgemm_kernel: 128-row tiles, K steps of 64, 128 (SwiGLU 64) columns per tile
NT_SMALL = [
    dict(name="odd_ldo", ldo=283, groups=[G(1, 5, 8), G(127, 130, 56, oc=7, ac=8), G(300, 264, 200, oc=11, ac=16)]),       # scalar stores
    dict(name="ldo8", ldo=280, groups=[G(128, 8, 64, oc=8, ac=8), G(129, 136, 72, oc=16), G(300, 264, 200, oc=8, ac=24)]),
    dict(name="ldo4", ldo=276, groups=[G(129, 130, 200, oc=4), G(1, 264, 8, oc=12, ac=8), G(127, 5, 64, oc=4)]),
    dict(name="ragged", ldo=144, max_rows=129, sw=True, ld_aux=280,
         groups=[G(0, 136, 72, oc=8, dev=True, gather=True), G(1, 130, 56, oc=4, dev=True, gather=True), G(17, 130, 56, oc=4, dev=True),
                 G(129, 136, 200, oc=8, dev=True, gather=True)]),
    dict(name="swiglu", ldo=208, sw=True, only_sw=True, ld_aux=408, groups=[G(129, 96, 72, oc=8), G(300, 200, 200, ac=8)]),
    dict(name="rows1025_few_tiles", ldo=136, sw=True, ld_aux=272, groups=[G(1025, 136, 72)]),      # >= 1024 rows but 5 big tiles: still tgemm_kernel
]
# 2. tgemm_pp_kernel: 256 x 256 (SwiGLU 256 x 128) tiles, K tiles of 32; the grid counts max_rows x max_n x groups, so ONE group per
#    launch is large and the tile count comes from the number of groups
_TINY = [G(9, 8, 8), G(1, 5, 8, oc=8), G(40, 8, 8), G(3, 16, 8), G(8, 8, 8, oc=16), G(2, 8, 8), G(5, 8, 8)]
PP_COUNTS = [1300, 0, 1, 255, 256, 257, 1025, 40]
NT_PP = [
    dict(name="pp_static", ldo=536, groups=[G(1025, 520, 296, oc=8, ac=8), G(1279, 264, 136, oc=16), G(1024, 248, 128, oc=4), G(1280, 504, 8, oc=8),
                                            G(300, 8, 136), G(1, 520, 128, oc=8), G(17, 5, 8, oc=8), G(255, 136, 8), G(40, 8, 8)]),
    dict(name="pp_ldo4", ldo=532, sw=True, ld_aux=1048, groups=[G(1025, 520, 136, oc=4), G(1024, 264, 8, oc=12)] + _TINY),
    dict(name="pp_ragged", ldo=528, max_rows=1300,
         groups=[G(c, n, k, oc=oc, dev=True, gather=ga) for c, n, k, oc, ga in zip(PP_COUNTS, [520, 8, 264, 248, 504, 136, 264, 5], [296, 8, 128, 136, 8, 296, 136, 128],
                                                                                    [8, 0, 8, 4, 8, 16, 0, 8], [True, True, False, True, False, True, False, True])]),
    dict(name="ppsw_static", ldo=272, sw=True, only_sw=True, ld_aux=536,
         groups=[G(1025, 264, 296, oc=8), G(1279, 136, 128), G(1024, 120, 136, oc=8), G(1280, 8, 8, oc=8), G(300, 100, 136, oc=8),       # n = 100: aux16 fails
                 G(257, 264, 8, oc=4), G(9, 8, 8), G(1, 5, 8, oc=8), G(40, 8, 8)]),                                                  # oc = 4: al16 fails
    dict(name="ppsw_ldaux4", ldo=272, sw=True, only_sw=True, ld_aux=532, groups=[G(1025, 264, 136, oc=8), G(300, 136, 8)] + _TINY),
    dict(name="ppsw_ragged", ldo=272, sw=True, only_sw=True, ld_aux=536, max_rows=1300,
         groups=[G(c, n, k, oc=oc, dev=True, gather=ga) for c, n, k, oc, ga in zip(PP_COUNTS, [264, 8, 136, 120, 264, 100, 136, 5], [136, 8, 128, 296, 8, 136, 296, 128],
                                                                                    [8, 0, 8, 0, 8, 8, 0, 8], [True, False, True, True, False, True, False, True])]),
]
# 3. tgemm_nn_kernel: k-major weights, 256 x 256 tiles at any size; k need not be a multiple of 8; w2 continues behind k_w1 rows of w
NN = [
    dict(name="nn_static", ldo=272, kmajor=True, groups=[G(1, 8, 1, oc=4), G(255, 248, 11, oc=8), G(256, 256, 31), G(257, 264, 32, oc=4), G(520, 264, 33, oc=8, ac=8),
                                                         G(300, 8, 136, oc=12, ac=16), G(257, 256, 300, oc=16, ac=8)]),
    dict(name="nn_seam", ldo=272, kmajor=True, groups=[G(257, 264, 33, k_w1=32), G(1, 8, 72, k_w1=32), G(300, 248, 161, k_w1=32, oc=4), G(255, 256, 129, k_w1=128),
                                                       G(256, 8, 168, k_w1=128, oc=8), G(520, 264, 257, k_w1=128, ac=8)]),
    dict(name="nn_ragged", ldo=272, kmajor=True, max_rows=520,
         groups=[G(300, 264, 136, oc=4, dev=True), G(0, 8, 11, dev=True, gather=True), G(520, 248, 33, oc=8, dev=True, gather=True), G(0, 264, 300, dev=True),
                 G(17, 8, 300, oc=12, dev=True)]),
]
NT_ALL = NT_SMALL + NT_PP + NN
SPEC = {s["name"]: s for s in NT_ALL}


def T(m, n, k, pco=0, qco=0, oc=0, dev=False, own=False):
    return dict(m=m, n=n, k=k, pco=pco, qco=qco, oc=oc, dev=dev, own=own)


# 4. tgemm_tn_kernel (+ tn_reduce_kernel)
TN_WINDOWS = [0, 1, 31, 32, 33, 127, 128, 129, 300]
TN = [
    dict(name="tn_static", ldo=272, groups=[T(8, 4, 0), T(12, 252, 1, oc=4), T(250, 256, 31, pco=8), T(256, 260, 32, qco=8, own=True), T(264, 4, 33, oc=8),
                                            T(8, 252, 127, own=True), T(12, 256, 128), T(250, 260, 129, oc=4, pco=16, qco=8), T(264, 260, 300, oc=8)]),
    dict(name="tn_device", ldo=264, groups=[T(264, 260, 33, dev=True), T(256, 252, 0, dev=True), T(250, 256, 300, dev=True, own=True), T(12, 4, 129, oc=4, dev=True)]),
    dict(name="tn_device_empty", ldo=264, groups=[T(264, 260, 0, dev=True)]),
    dict(name="tn_split", ldo=260, dense=True, splits=(2, 3, 4), groups=[T(12, 260, 300), T(264, 260, 33), T(250, 260, 127), T(8, 260, 0)]),
    dict(name="tn_auto", ldo=260, dense=True, splits=(-1,), groups=[T(264, 260, 1100)]),
]
TN_SPEC = {s["name"]: s for s in TN}


# ------------------------------------------------------------------------------------------------ dispatch, restated
def kernel_of(spec, sw=False):
    """launch_tgemm / umoe_tiled_gemm with the default environment -> "nn" | "pp" | "small" """
    if spec.get("kmajor"):
        return "nn"
    rows, n, ng = max_rows_of(spec), max(g["n"] for g in spec["groups"]), len(spec["groups"])
    pays = rows >= 1024 and cdiv(rows, 256) * cdiv(n, 128 if sw else 256) * ng >= 128            # tgemm_pp_pays (UMOE_TGEMM_PP_MINWG = 128)
    return "pp" if pays else "small"


def tm_of(rows, n, ng, sw):
    """tgemm_tm: 256-token tiles of tgemm_kernel (UMOE_TGEMM_MINWG = 512)"""
    if rows < 1024:
        return 128
    return 256 if cdiv(rows, 256) * cdiv(n, 64 if sw else 128) * ng >= 512 else 128


def max_rows_of(spec):
    return spec.get("max_rows", max(g["rows"] for g in spec["groups"]))


def epilogues_of(spec):
    """(epilogue, with bias) runs of a case"""
    if spec.get("kmajor"):
        return [(BF16, False)]
    if spec.get("only_sw"):
        return []
    if spec in NT_SMALL:
        return [(e, b) for e in (BF16, RESID, F32, RAW) for b in (False, True)]
    return [(BF16, True), (RESID, True), (RESID, False), (F32, False), (RAW, True), (RAW, False)]


# ------------------------------------------------------------------------------------------------ NT / NN cases: data, reference
@functools.lru_cache(maxsize=None)
def nt_case(name):
    """Buffers of a case (CPU).  A group's output block starts at an 8-aligned row (padding rows and one spare block of 8 between groups);
    device groups get row_off (and out_row_base 0 or 8), gather groups a list whose entries outside [row_off, row_off + count) point at a
    NaN row and whose tokens repeat and come out of order; rows of the token pool the list does not name stay NaN."""
    spec = SPEC[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)) + 11)
    km, sw = bool(spec.get("kmajor")), bool(spec.get("sw"))
    lda = r8(max(q["ac"] + r8(q["k"]) for q in spec["groups"])) + 8
    ob, ab, plan = 8, 8, []
    for i, q in enumerate(spec["groups"]):
        rows, cap = q["rows"], r8(q["rows"]) + 8
        pool = cap
        plan.append((ob, ab, pool))
        ob, ab = ob + cap, ab + pool + 3
    RO, RA = ob, ab
    A = torch.full((RA, lda), NAN, dtype=bf16)
    resid = torch.full((RO, spec["ldo"]), NAN, dtype=bf16)
    groups = []
    for i, (q, (ob, ab, pool)) in enumerate(zip(spec["groups"], plan)):
        rows, n, k, oc, ac = q["rows"], q["n"], q["k"], q["oc"], q["ac"]
        d = dict(q)
        d["orows"] = ob + torch.arange(rows)
        roff = 0
        if q["dev"]:
            d["out_row_base"] = 8 if i % 2 else 0
            roff = ob - d["out_row_base"]
            d["row_off"] = torch.tensor([roff], dtype=torch.int32)
            d["count"] = torch.tensor([rows], dtype=torch.int32)
        else:
            d["out_row_base"] = ob
        if q["gather"]:
            named = ab + torch.randint(0, max(pool - 1, 1), (rows,), generator=g)         # (the pool's last row is never named: it stays NaN)
            if rows > 3:
                named[1] = named[0]                                                        # a repeated token
                named[2] = ab + pool - 2                                                   # ... and one out of order
            lst = torch.full((roff + rows + 9,), ab + pool - 1, dtype=torch.int32)
            lst[roff:roff + rows] = named.to(torch.int32)
            d["rows_list"], d["arows"], d["a_row_base"] = lst, named, 0
        else:
            d["arows"], d["a_row_base"] = ab + torch.arange(rows), ab - roff
        ua = torch.unique(d["arows"])
        A[ua[:, None], ac + torch.arange(k)] = randbf(g, ua.numel(), k)
        if km:
            A[ua[:, None], ac + k + torch.arange(r8(k) - k)] = 0.0                         # the last 8-column chunk is zero padded (train._pad8)
            k1 = q["k_w1"] or k
            d["wbuf"] = torch.full((k + 8, n + 8), NAN, dtype=bf16)                        # a taller, wider buffer: w is rows [0, k1) of it
            d["wbuf"][:k1, :n] = randbf(g, k1, n, scale=k ** -0.5)
            if q["k_w1"]:
                d["w2buf"] = torch.full((k - k1 + 3, n + 8), NAN, dtype=bf16)
                d["w2buf"][:k - k1, :n] = randbf(g, k - k1, n, scale=k ** -0.5)
        else:
            d["wbuf"] = torch.full((n + 2, k + 8), NAN, dtype=bf16)
            d["wbuf"][:n, :k] = randbf(g, n, k, scale=k ** -0.5)
            if sw:
                d["w2buf"] = torch.full((n + 2, k + 8), NAN, dtype=bf16)
                d["w2buf"][:n, :k] = randbf(g, n, k, scale=k ** -0.5)
            d["bbuf"] = torch.full((n + 4,), NAN)
            d["bbuf"][:n] = torch.randn(n, generator=g) * 0.5
        resid[d["orows"][:, None], oc + torch.arange(n)] = randbf(g, rows, n)
        groups.append(d)
    return dict(spec=spec, name=name, A=A, resid=resid, groups=groups, RO=RO, ldo=spec["ldo"], km=km, sw=sw, max_rows=max_rows_of(spec))


def _operands(c, d):
    """(a [rows][k], w [n][k], w2 [n][k] or None) of a group, bf16, exactly what the header says is read"""
    k, n = d["k"], d["n"]
    a = c["A"][d["arows"]][:, d["ac"]:d["ac"] + k]
    if c["km"]:
        k1 = d["k_w1"] or k
        w = d["wbuf"][:k1, :n]
        if d["k_w1"]:
            w = torch.cat([w, d["w2buf"][:k - k1, :n]], 0)
        return a, w.t(), None
    return a, d["wbuf"][:n, :k], (d["w2buf"][:n, :k] if c["sw"] else None)


def nt_ref(c):
    """float64 accumulators and sum |a w| of every group, once per case"""
    if "ref" not in c:
        ref = []
        for d in c["groups"]:
            a, w, w2 = _operands(c, d)
            a, w = a.to(f64), w.to(f64)
            r = dict(acc=a @ w.t(), ab=a.abs() @ w.abs().t())
            if w2 is not None:
                r["acc2"], r["ab2"] = a @ w2.to(f64).t(), a.abs() @ w2.to(f64).abs().t()
            ref.append(r)
        c["ref"] = ref
    return c["ref"]


def emu_acc(a, w):
    """fp32 accumulator as the kernels build it: K in tiles of 32, one after the other"""
    a, w = a.float(), w.float()
    acc = torch.zeros(a.shape[0], w.shape[0])
    for t in range(0, a.shape[1], 32):
        acc += a[:, t:t + 32] @ w[:, t:t + 32].t()
    return acc


def out_dtype(epi):
    return torch.float32 if epi in (F32, RAW) else bf16


def emu_nt(c, epi, with_bias, plant=None, pg=None):
    """the launch in fp32 / bf16 torch arithmetic with the rounding points of tg_epilogue -> (out, aux).  plant (on group pg): a wrong
    kernel -- see PLANTS_NT"""
    out = torch.full((c["RO"], c["ldo"]), SENT, dtype=out_dtype(epi))
    aux = torch.full((c["RO"], c["spec"]["ld_aux"]), SENT, dtype=bf16) if epi == SWIGLU else None
    for i, d in enumerate(c["groups"]):
        hit = plant if i == pg else None
        a, w, w2 = _operands(c, d)
        n, oc, rows = d["n"], d["oc"], d["rows"]
        acc = emu_acc(a, w)
        if hit == "kchunk":                                       # one 8-column K chunk of the last output tile dropped
            r0, c0, k0 = (rows - 1) // 128 * 128, (n - 1) // 128 * 128, min(8, d["k"] - 8)
            acc[r0:, c0:] -= a[r0:, k0:k0 + 8].float() @ w[c0:, k0:k0 + 8].float().t()
        cols = oc + torch.arange(n)
        at = (d["orows"][:, None], cols)
        if epi == SWIGLU:
            gt, up = rbf(acc), rbf(emu_acc(a, w2))
            si = rbf(gt / (1.0 + torch.exp(-gt)))
            out[at] = (si * up).to(bf16)
            if hit == "swap_aux":
                gt, up = up, gt
            aux[d["orows"][:, None], torch.arange(n)] = gt.to(bf16)
            aux[d["orows"][:, None], n + torch.arange(n)] = up.to(bf16)
            continue
        if with_bias:
            b = d["bbuf"][:n].clone()
            if hit == "bias_last":                                # bias missed on the last ragged column group (4 columns per lane)
                b[(n - 1) // 4 * 4:] = 0
            acc = acc + b
        if epi == RAW or (epi == F32 and hit == "f32_unrounded"):
            out[at] = acc
        elif epi == F32:
            out[at] = rbf(acc)
        elif epi == BF16:
            out[at] = acc.to(bf16)
        else:
            r = c["resid"][at].float()
            out[at] = (r + acc).to(bf16) if hit == "resid_first" else (r + rbf(acc)).to(bf16)
        if hit == "row_behind":                                 # a row written behind the count
            out[d["orows"][-1] + 1, cols] = out[d["orows"][-1], cols]
        elif hit == "col_outside":                                # a column written outside the window
            out[d["orows"][0], oc - 1 if oc else oc + n] = 0.5
        elif hit == "nan":
            out[d["orows"][0], oc] = NAN
    return out, aux


def nt_interval(c, d, r, epi, with_bias):
    """(centre, half width) of a group's outputs in a linear epilogue"""
    v, e = r["acc"], d["k"] * U * r["ab"]
    if with_bias:
        v = v + d["bbuf"][:d["n"]].to(f64)
        e = e + U * v.abs()
    if epi == RAW:
        return v, e
    if epi == RESID:
        return interval_resid(v, e, c["resid"][d["orows"][:, None], d["oc"] + torch.arange(d["n"])])
    return interval(v, e)


def plant_ulp(c, epi, with_bias, out, pg):
    """one element of group pg one bf16 ulp above an interval that is a single value"""
    d = c["groups"][pg]
    mid, half = nt_interval(c, d, nt_ref(c)[pg], epi, with_bias)
    i, j = torch.nonzero((half == 0) & (mid > 0))[-1].tolist()
    out[d["orows"][i], d["oc"] + j] = float(mid[i, j] + ulp_bf16(mid[i, j]))
    return out


def check_nt(c, epi, with_bias, out, stats, aux=None):
    """every element of every group against its interval, everything else against the sentinel.  -> flagged share (SwiGLU)"""
    ref = nt_ref(c)
    out = out.detach().cpu()
    aux = aux.detach().cpu() if aux is not None else None
    written = torch.zeros(out.shape, dtype=torch.bool)
    aux_written = torch.zeros(aux.shape, dtype=torch.bool) if aux is not None else None
    n_flag = n_all = 0
    tag = EPI_NAME[epi] + ("+b" if with_bias else "")
    for d, r in zip(c["groups"], ref):
        n, k, cols = d["n"], d["k"], d["oc"] + torch.arange(d["n"])
        at = (d["orows"][:, None], cols)
        written[at] = True
        got = out[at]
        if epi == SWIGLU:
            ag, au = (d["orows"][:, None], torch.arange(n)), (d["orows"][:, None], n + torch.arange(n))
            aux_written[ag] = aux_written[au] = True
            check_bf16("aux gate", aux[ag], r["acc"], k * U * r["ab"], stats)
            check_bf16("aux up", aux[au], r["acc2"], k * U * r["ab2"], stats)
            mid, half, flag = swiglu_y(aux[ag], aux[au])
            check("swiglu y", got, mid, half, stats)
            n_flag, n_all = n_flag + int(flag.sum()), n_all + flag.numel()
            continue
        check(("acc" + ("+b" if with_bias else "")) if epi == RAW else tag, got, *nt_interval(c, d, r, epi, with_bias), stats)
        if epi == BF16 and not with_bias and got.numel():
            stats.share("bf16", float((got.to(f64) != rb(r["acc"])).double().mean()))
    keeps_sentinel(f"{c['name']} {tag}: output outside every group's window", out[~written])
    if aux is not None:
        keeps_sentinel(f"{c['name']}: aux_out outside (gate | up) of every group", aux[~aux_written])
    return n_flag / max(n_all, 1)


def ref_flag_share(c):
    """flagged share of a SwiGLU case on the reference's own gates (no GPU)"""
    n_flag = n_all = 0
    for r in nt_ref(c):
        g = rb(r["acc"])
        silu = g * torch.sigmoid(g)
        n_flag, n_all = n_flag + int((mid_dist(silu) <= SILU_W * silu.abs()).sum()), n_all + g.numel()
    return n_flag / max(n_all, 1)


def launch_nt(c, epi, with_bias, dev, with_aux=True):
    """the case through ops.tiled_gemm -> (out, aux)"""
    from unimoe_audio_amd import ops
    if "dev" not in c:
        dv = dict(A=c["A"].to(dev), resid=c["resid"].to(dev), groups=[])
        for d in c["groups"]:
            t = {key: d[key].to(dev) for key in ("wbuf", "w2buf", "bbuf", "row_off", "count", "rows_list") if key in d}
            dv["groups"].append(t)
        c["dev"] = dv
    dv = c["dev"]
    groups = []
    for d, t in zip(c["groups"], dv["groups"]):
        n, k = d["n"], d["k"]
        if c["km"]:
            k1 = d["k_w1"] or k
            q = dict(w=t["wbuf"][:k1, :n], w_kmajor=1, k=k, k_w1=d["k_w1"])
            if d["k_w1"]:
                q["w2"] = t["w2buf"][:k - k1, :n]
        else:
            q = dict(w=t["wbuf"][:n], k=k)
            if epi == SWIGLU:
                q["w2"] = t["w2buf"][:n]
            elif with_bias:
                q["bias"] = t["bbuf"][:n]
        q.update(a_row_base=d["a_row_base"], out_row_base=d["out_row_base"], a_col_off=d["ac"], out_col_off=d["oc"])
        if d["dev"]:
            q.update(row_off=t["row_off"], count=t["count"])
        else:
            q["static_count"] = d["rows"]
        if d["gather"]:
            q["rows"] = t["rows_list"]
        groups.append(q)
    out = torch.full((c["RO"], c["ldo"]), SENT, dtype=out_dtype(epi), device=dev)
    aux = torch.full((c["RO"], c["spec"]["ld_aux"]), SENT, dtype=bf16, device=dev) if (epi == SWIGLU and with_aux) else None
    ops.tiled_gemm(groups, dv["A"], out, max_rows=c["max_rows"], epilogue=epi, resid=dv["resid"] if epi == RESID else None, aux_out=aux)
    return out, aux


def run_nt_case(name, dev):
    c = nt_case(name)
    spec = c["spec"]
    st = Stats()
    for epi, wb in epilogues_of(spec):
        out, _ = launch_nt(c, epi, wb, dev)
        check_nt(c, epi, wb, out, st)
    share = None
    if spec.get("sw"):
        out, aux = launch_nt(c, SWIGLU, False, dev)
        share = check_nt(c, SWIGLU, False, out, st, aux)
        assert share <= 1e-3, share
        out2, _ = launch_nt(c, SWIGLU, False, dev, with_aux=False)
        assert torch.equal(out2.view(torch.int16), out.view(torch.int16)), "SwiGLU: y without aux_out differs from y with aux_out"
    st.show(f"{kernel_of(spec, bool(spec.get('only_sw')))} {name}" + (f" (flagged {share:.2e})" if share is not None else ""))


# ------------------------------------------------------------------------------------------------ TN cases
@functools.lru_cache(maxsize=None)
def tn_case(name):
    """P [rows][ldp], Q [rows][ldq] (NaN outside every window, the surplus columns up to roundup8 included); windows at row offsets
    that are no multiples of 8, three NaN rows between them; a group with own = True has operands and output of its own."""
    spec = TN_SPEC[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)) + 5)
    ldp = r8(max(q["pco"] + q["m"] for q in spec["groups"])) + 8
    ldq = r8(max(q["qco"] + q["n"] for q in spec["groups"])) + 8
    rows_total = 3 + sum(q["k"] + 5 for q in spec["groups"])
    P = torch.full((rows_total, ldp), NAN, dtype=bf16)
    Q = torch.full((rows_total, ldq), NAN, dtype=bf16)
    koff, ob, groups = 3, 0 if spec.get("dense") else 8, []
    for q in spec["groups"]:
        d = dict(q)
        m, n, k = q["m"], q["n"], q["k"]
        scale = max(k, 1) ** -0.25
        p, qq = randbf(g, k, m, scale=scale), randbf(g, k, n, scale=scale)
        d["p"], d["q"] = p, qq
        if q["own"]:
            d["pbuf"] = torch.full((5 + k + 3, r8(q["pco"] + m) + 8), NAN, dtype=bf16)
            d["qbuf"] = torch.full((5 + k + 3, r8(q["qco"] + n) + 16), NAN, dtype=bf16)
            d["pbuf"][5:5 + k, q["pco"]:q["pco"] + m] = p
            d["qbuf"][5:5 + k, q["qco"]:q["qco"] + n] = qq
            d["k_off"], d["out_row_base"], d["RO"] = 5, 4, m + 9
        else:
            P[koff:koff + k, q["pco"]:q["pco"] + m] = p
            Q[koff:koff + k, q["qco"]:q["qco"] + n] = qq
            d["k_off"], d["out_row_base"] = koff, ob
            koff += k + 5
            ob += m if spec.get("dense") else r8(m) + 8
        groups.append(d)
    return dict(spec=spec, name=name, P=P, Q=Q, groups=groups, RO=ob, ldo=spec["ldo"])


def tn_ref(c):
    if "ref" not in c:
        c["ref"] = [dict(acc=d["p"].to(f64).t() @ d["q"].to(f64), ab=d["p"].to(f64).abs().t() @ d["q"].to(f64).abs()) for d in c["groups"]]
    return c["ref"]


def tn_parts(k, ks):
    """the K windows of a split: whole 32-row tiles per part (tgemm_tn_kernel)"""
    if ks <= 1:
        return [(0, k)]
    per = cdiv(cdiv(k, 32), ks) * 32
    return [(min(p * per, k), min(p * per + per, k)) for p in range(ks)]


def emu_tn(c, ks, plant=None, pg=None):
    """-> (launch output, {group index: output of its own})"""
    out = torch.full((c["RO"], c["ldo"]), SENT, dtype=bf16)
    own = {}
    for i, d in enumerate(c["groups"]):
        m, n, k = d["m"], d["n"], d["k"]
        parts = [emu_acc(d["p"][lo:hi].t(), d["q"][lo:hi].t()) for lo, hi in tn_parts(k, ks)]
        if plant == "part" and i == pg:
            parts = parts[1:]                                      # one K-split partial left out (the first: the last may be empty)
        acc = parts[0]
        for p in parts[1:]:
            acc = acc + p
        if plant == "kchunk" and i == pg:
            acc[:, -4:] -= d["p"][8:16].float().t() @ d["q"][8:16, -4:].float()
        tgt = out
        if d["own"]:
            tgt = own[i] = torch.full((d["RO"], c["ldo"]), SENT, dtype=bf16)
        tgt[d["out_row_base"]:d["out_row_base"] + m, d["oc"]:d["oc"] + n] = acc.to(bf16)
        if plant == "row_behind" and i == pg:
            tgt[d["out_row_base"] + m, d["oc"]:d["oc"] + n] = 0.0
    return out, own


def check_tn(c, ks, out, own, stats):
    ref = tn_ref(c)
    out = out.detach().cpu()
    written = torch.zeros(out.shape, dtype=torch.bool)
    for i, (d, r) in enumerate(zip(c["groups"], ref)):
        m, n, k = d["m"], d["n"], d["k"]
        rs, cs = slice(d["out_row_base"], d["out_row_base"] + m), slice(d["oc"], d["oc"] + n)
        k_eff = k + (ks if ks > 1 else 0)
        if d["own"]:
            o = own[i].detach().cpu()
            w = torch.zeros(o.shape, dtype=torch.bool)
            w[rs, cs] = True
            keeps_sentinel(f"{c['name']}: group {i}'s own output outside its window", o[~w])
            got = o[rs, cs]
        else:
            written[rs, cs] = True
            got = out[rs, cs]
        check_bf16(f"k={k}" if len(c["groups"]) > 1 else "tn", got, r["acc"], k_eff * U * r["ab"], stats)
        if k == 0:
            assert bool((got == 0).all()), "an empty window must give exact zeros"
    keeps_sentinel(f"{c['name']}: output outside every group's window", out[~written])


def launch_tn(c, ks, dev):
    from unimoe_audio_amd import ops
    if "dev" not in c:
        c["dev"] = dict(P=c["P"].to(dev), Q=c["Q"].to(dev), groups=[
            dict(pbuf=d["pbuf"].to(dev), qbuf=d["qbuf"].to(dev)) if d["own"] else {} for d in c["groups"]])
    dv = c["dev"]
    out = torch.full((c["RO"], c["ldo"]), SENT, dtype=bf16, device=dev)
    groups, own = [], {}
    for i, (d, t) in enumerate(zip(c["groups"], dv["groups"])):
        q = dict(m=d["m"], n=d["n"], p_col_off=d["pco"], q_col_off=d["qco"], out_row_base=d["out_row_base"], out_col_off=d["oc"])
        if d["dev"]:
            q.update(k_off_dev=torch.tensor([d["k_off"]], dtype=torch.int32, device=dev), k_count_dev=torch.tensor([d["k"]], dtype=torch.int32, device=dev))
        else:
            q.update(k_off=d["k_off"], k=d["k"])
        if d["own"]:
            own[i] = torch.full((d["RO"], c["ldo"]), SENT, dtype=bf16, device=dev)
            q.update(p=t["pbuf"], q=t["qbuf"], out=own[i])
        groups.append(q)
    ops.tiled_gemm_tn(groups, dv["P"], dv["Q"], out, k_split=ks)
    return out, own


def tn_library_split(c):
    """umoe_tiled_gemm_tn_split for the case with k_split = -1"""
    import ctypes as C
    from unimoe_audio_amd import _lib as L
    arr = (L.TnGroup * len(c["groups"]))()
    for i, d in enumerate(c["groups"]):
        arr[i].m, arr[i].n, arr[i].k, arr[i].out_row_base = d["m"], d["n"], d["k"], d["out_row_base"]
    a = L.TGemmTnArgs(groups=C.cast(arr, C.c_void_p), num_groups=len(c["groups"]), ldo=c["ldo"], k_split=-1)
    return L.lib().umoe_tiled_gemm_tn_split(C.byref(a))


# ================================================================================================ checkers without a GPU
def _rejects(fn):
    with pytest.raises(AssertionError):
        fn()


def test_dispatch_cpu():
    """the case lists lie on both sides of launch_tgemm's predicates, and every shape list of the issue is covered"""
    for s in NT_SMALL:
        assert kernel_of(s) == "small" and kernel_of(s, True) == "small", s["name"]
    for s in NT_PP:
        assert kernel_of(s, bool(s.get("only_sw"))) == "pp", s["name"]
        if s.get("sw"):
            assert kernel_of(s, True) == "pp", s["name"]
    assert any(max_rows_of(s) < 1024 for s in NT_SMALL) and any(max_rows_of(s) >= 1024 for s in NT_SMALL)       # max_rows >= 1024 alone does not pay
    assert all(kernel_of(s) == "nn" for s in NN)
    assert any(max_rows_of(s) >= 1024 for s in NT_PP) and all(max_rows_of(s) < 1024 for s in NN)
    # both tile orders of the pp kernel and of the nn kernel
    for lst in (NT_PP, NN):
        assert any(any(q["dev"] for q in s["groups"]) for s in lst) and any(not any(q["dev"] for q in s["groups"]) for s in lst)
    # the 256-token tiles of tgemm_kernel: wherever tgemm_tm would choose them, tgemm_pp_pays has taken the launch
    for rows in (1, 1023, 1024, 1025, 4096, 6240, 65536):
        for n in (1, 64, 65, 128, 129, 256, 257, 2048, 12324):
            for ng in range(1, 13):
                for sw in (False, True):
                    if tm_of(rows, n, ng, sw) == 256:
                        assert rows >= 1024 and cdiv(rows, 256) * cdiv(n, 128 if sw else 256) * ng >= 128, (rows, n, ng, sw)
    # the issue's shape lists
    small = [q for s in NT_SMALL for q in s["groups"]]
    assert {1, 127, 128, 129, 300} <= {q["rows"] for q in small} and {8, 5, 130, 136, 264} <= {q["n"] for q in small}
    assert {8, 56, 64, 72, 200} <= {q["k"] for q in small} and {0, 1, 17, 129} <= {q["rows"] for q in small if q["dev"]}
    assert {96, 200} <= {q["n"] for q in SPEC["swiglu"]["groups"]}
    pp = [q for s in NT_PP for q in s["groups"]]
    assert {1024, 1025, 1279, 1280} <= {q["rows"] for q in pp} and {8, 128, 136, 296} <= {q["k"] for q in pp}
    assert {248, 264, 504, 520} <= {q["n"] for q in pp}
    assert any(s["ldo"] % 8 for s in NT_PP) and any(q["oc"] == 4 for q in pp) and any(q["oc"] == 8 for q in pp)
    aux16 = {(s["ld_aux"] | q["n"]) % 8 == 0 for s in NT_PP if s.get("sw") for q in s["groups"]}
    assert aux16 == {True, False}
    nn = [q for s in NN for q in s["groups"]]
    assert {1, 255, 256, 257, 520} <= {q["rows"] for q in nn} and {8, 248, 256, 264} <= {q["n"] for q in nn}
    assert {1, 11, 31, 32, 33, 136, 300} <= {q["k"] for q in nn}
    assert {(a, b) for a in (32, 128) for b in (1, 40, 129)} == {(q["k_w1"], q["k"] - q["k_w1"]) for q in nn if q["k_w1"]}
    tn = [q for s in TN for q in s["groups"]]
    assert {8, 12, 250, 256, 264} <= {q["m"] for q in tn} and {4, 252, 256, 260} <= {q["n"] for q in tn}
    assert set(TN_WINDOWS) <= {q["k"] for q in TN_SPEC["tn_static"]["groups"]}
    ks = [q["k"] for q in TN_SPEC["tn_device"]["groups"]]
    assert 0 in ks and max(ks) > sum(ks) - max(ks)
    assert all(any(q["k"] % s for q in TN_SPEC["tn_split"]["groups"]) for s in (2, 3, 4))


def test_nt_checkers_cpu():
    """every NT / NN case: the emulation passes in every epilogue the GPU test runs; the SwiGLU cases flag at most 1e-3"""
    st = Stats()
    for s in NT_ALL:
        c = nt_case(s["name"])
        for epi, wb in epilogues_of(s):
            check_nt(c, epi, wb, emu_nt(c, epi, wb)[0], st)
        if s.get("sw"):
            assert ref_flag_share(c) <= 1e-3, (s["name"], ref_flag_share(c))
            out, aux = emu_nt(c, SWIGLU, False)
            assert check_nt(c, SWIGLU, False, out, st, aux) <= 1e-3
    assert max(st.values()) <= 1.0
    st.show("emulated NT / NN cases")


PLANTS_NT = [("kchunk", BF16, False), ("kchunk", RAW, True), ("ulp", BF16, True), ("ulp", F32, False), ("ulp", RESID, True), ("bias_last", BF16, True),
             ("bias_last", RESID, True), ("resid_first", RESID, True), ("f32_unrounded", F32, False), ("row_behind", BF16, False),
             ("col_outside", RAW, False), ("nan", BF16, False), ("nan", RAW, True)]


def test_nt_planted_errors_cpu():
    for name, pg in (("odd_ldo", 1), ("ragged", 3), ("nn_seam", 2)):
        c = nt_case(name)
        for plant, epi, wb in PLANTS_NT:
            if c["km"] and (epi != BF16 or wb):
                continue
            check_nt(c, epi, wb, emu_nt(c, epi, wb)[0], Stats())
            bad = plant_ulp(c, epi, wb, emu_nt(c, epi, wb)[0], pg) if plant == "ulp" else emu_nt(c, epi, wb, plant, pg)[0]
            _rejects(lambda: check_nt(c, epi, wb, bad, Stats()))
    c = nt_case("swiglu")
    for plant in ("swap_aux", "kchunk"):
        out, aux = emu_nt(c, SWIGLU, False, plant, 1)
        _rejects(lambda: check_nt(c, SWIGLU, False, out, Stats(), aux))
    out, aux = emu_nt(c, SWIGLU, False)
    bad = aux.clone()
    bad[c["groups"][0]["orows"][0], 2 * 96] = 0.0                         # a column beyond 2n of aux_out written
    _rejects(lambda: check_nt(c, SWIGLU, False, out, Stats(), bad))
    bad = out.clone()
    d = c["groups"][1]
    v = bad[d["orows"][7], d["oc"] + 3].to(f64)
    bad[d["orows"][7], d["oc"] + 3] = float(v + ulp_bf16(v) * (1 if v >= 0 else -1))     # y one bf16 ulp off the kernel's own gate / up
    _rejects(lambda: check_nt(c, SWIGLU, False, bad, Stats(), aux))


def test_tn_checkers_cpu():
    st = Stats()
    for s in TN:
        c = tn_case(s["name"])
        for ks in s.get("splits", (1,)):
            check_tn(c, 2 if ks < 0 else ks, *emu_tn(c, 2 if ks < 0 else ks), st)
    assert max(st.values()) <= 1.0
    st.show("emulated TN cases")
    c = tn_case("tn_static")
    for plant, pg in (("kchunk", 8), ("row_behind", 3), ("row_behind", 6)):
        _rejects(lambda: check_tn(c, 1, *emu_tn(c, 1, plant, pg), Stats()))
    out, own = emu_tn(c, 1)
    bad = out.clone()
    bad[c["groups"][0]["out_row_base"], 0] = 2.0 ** -100                  # an empty window that is not exactly zero
    _rejects(lambda: check_tn(c, 1, bad, own, Stats()))
    bad = out.clone()
    bad[c["groups"][6]["out_row_base"] + 11, 255] = NAN                   # one NaN let through (the surplus columns of m = 12 hold NaN)
    _rejects(lambda: check_tn(c, 1, bad, own, Stats()))
    c = tn_case("tn_split")
    for ks in (2, 3, 4):
        for pg in (0, 2):
            _rejects(lambda: check_tn(c, ks, *emu_tn(c, ks, "part", pg), Stats()))


# ================================================================================================ GPU tests
@gpu
@pytest.mark.parametrize("name", [s["name"] for s in NT_SMALL])
def test_tgemm_small_vs_fp64(dev, name):
    """tgemm_kernel (128-row tiles, K steps of 64): every epilogue with and without bias, static groups with a_row_base / out_row_base /
    out_col_off / a_col_off in leading dimensions that are odd, 4 mod 8 and 0 mod 8, ragged groups (device counts 0, 1, 17, 129, row_off,
    gather lists), SwiGLU from separate w / w2 with and without aux_out, and 1025 rows in too few tiles for the 256 x 256 kernel."""
    assert kernel_of(SPEC[name]) == "small"
    run_nt_case(name, dev)


@gpu
@pytest.mark.parametrize("name", [s["name"] for s in NT_PP])
def test_tgemm_pp_vs_fp64(dev, name):
    """tgemm_pp_kernel under the default dispatch (>= 1024 rows, >= 128 tiles from many groups): 1, 4, 5 and 10 K tiles, rows and columns
    around the tile edges, both tile orders, the LDS epilogue (8-aligned ldo and out_col_off) and the direct one (out_col_off 4, ldo 4
    mod 8), aux_out through LDS (ld_aux and n multiples of 8) and direct."""
    spec = SPEC[name]
    assert kernel_of(spec, bool(spec.get("only_sw"))) == "pp"
    run_nt_case(name, dev)


@gpu
@pytest.mark.parametrize("name", [s["name"] for s in NN])
def test_tgemm_nn_vs_fp64(dev, name):
    """tgemm_nn_kernel: k-major weights as views into taller, wider NaN buffers, k of any length, the w / w2 seam, ragged groups."""
    run_nt_case(name, dev)


@gpu
@pytest.mark.parametrize("name", [s["name"] for s in TN])
def test_tgemm_tn_vs_fp64(dev, name):
    """tgemm_tn_kernel and tn_reduce_kernel: windows of 0 .. 300 rows at offsets that are no multiples of 8, static and on the device,
    per-group p / q / out, out_col_off, m % 8 != 0, K splits of 2, 3, 4 and the library's own (K_eff = K + k_split)."""
    c = tn_case(name)
    st = Stats()
    for ks in c["spec"].get("splits", (1,)):
        eff = ks
        if ks < 0:
            eff = tn_library_split(c)
            assert eff > 1, f"the library chose k_split = {eff}: the case is meant to be split"
        out, own = launch_tn(c, ks, dev)
        check_tn(c, eff, out, own, st)
    st.show(name)
