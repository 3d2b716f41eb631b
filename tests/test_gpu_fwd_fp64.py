"""The forward row-wise kernels (csrc/umoe_misc.hip: combine_kernel, rmsnorm_kernel; csrc/umoe_attn.hip: rope_append_kernel) and the four
kernels of csrc/umoe_vision.hip, each against a float64 restatement on the CPU of the same operation on the same input bits.

Rules of the whole file
  * reference: float64; bf16 / fp32 inputs are upcast exactly; where a kernel documents a rounding of an intermediate to bf16 the
    reference rounds its float64 value at the same place;
  * comparison: per element, never a norm over a tensor;
  * candidate rule (combine, RMSNorm, SwiGLU pair): after the one inexact fp32 step of these kernels every later operation is an exact
    fp32 operation (a product or a sum of two bf16 values) or a bf16 rounding, so the float64 restatement fixes the output BITS.  The
    exception is an intermediate whose float64 value lies within the fp32 error window of a bf16 rounding midpoint: it is flagged.
    Unflagged elements must match bit for bit; a flagged element must equal one of the chains obtained by rounding that intermediate
    down or up and carrying it through the remaining stages (two flagged points: any of the four chains).  The windows are derived,
    u = 2^-24:
      combine       (n_sel + 1) u sum|w_e y_e| for the routed sum (n_sel products and their sum), u |y_i sw_i| for a shared product
      RMSNorm       x rs: (4 ceil(D / 2048) + 9) u |x rs| -- sum of positive terms of depth 8 per 2048 columns (the adds of one thread) + 6
                    (wave) + 3 (block) + 1 (the squares are exact, the first add is not), the divide and the add of eps 1 each, all
                    halved by the root; rsqrtf 2 u; the product 1 u: 13 u at D <= 2048, 17 u at D <= 4096, 21 u at D <= 6144
      SwiGLU pair   6.5 u |silu|: expf 3 u, the add u, the divide 2.5 u (the OpenCL limits the device library is built to)
    a case may flag at most 1e-2 of its elements: a condition on the inputs, checked without a GPU on the case lists the GPU tests run;
  * exact rule (mRoPE + KV append; the exact-data pass of combine): every step is an exact fp32 operation or a bf16 rounding, the
    reference fixes every bit, there is no tolerance and there are no flags;
  * bound rule (vision_rope, vision_attn, gelu): |got - ref| <= bound per element, the bound spelled out at each reference;
  * untouched memory: outputs the caller owns are prefilled with a sentinel (bf16 7.0) and whatever the kernel must not write keeps it
    bit for bit; everything a kernel must not read (or must not use) holds NaN: expert rows no token selected, the weights of
    unselected experts, the dynamic columns of global_w, guard tokens between attention segments.  (ops.combine, ops.rmsnorm and the
    q of ops.qkv_mrope_kvappend allocate their outputs themselves: every element of those is compared.)
Every GPU test prints its figures under -s ("FWD FP64 ..."): worst error / bound of the bound rule, flagged share and the number of
flagged elements that took the alternative chain of the candidate rule.

The checkers are tested without a GPU (test_*_cpu): a result emulated in fp32 / bf16 torch arithmetic from the same inputs passes at
the shapes the GPU tests use, the flagged shares stay under the cap, and each planted error is rejected.

The expert-parallel form combine_kernel<true> is not launched here (it waits on peer flags; tests/test_gpu_ep.py covers it).

Measured on an MI355X (the whole file: 106 GPU tests in 2 s), over the cases of each test:
  combine       39 cases x (Gaussian, exact data): flagged share of out 0 - 7.8e-3 (one element of 128 at D = 8; 5.6e-3 at 16 experts, 90 %
                selected), 6 flagged elements took the alternative chain; fused norm: flagged share 0 - 1.4e-3, 2 alternative chains;
                the exact-data pass bit for bit everywhere
  rmsnorm       18 shapes x (plain, residual): flagged share 0 - 1.8e-3, 283 flagged elements took the alternative chain (196 at 6144 x 257:
                the flagged elements of a row share one rs and go the same way); sum_out bit for bit
  mrope         10 cases bit for bit, every unnamed cache slot at the sentinel
  vision_rope   worst error / bound 0.60 - 0.996 (a bf16 rounding reaches its half ulp)
  vision_attn   worst error / bound 0.77 - 0.79; 2710 planted segment-edge mutations per case, every one outside the bound
  swiglu_pair   flagged share 0 - 2.9e-4, no flagged element took the alternative chain; padding +0
  gelu          worst error / bound 0 (n = 1) - 0.97
Found by this file: the dense form of combine_kernel (and any form that broadcasts its tables inside the row loop) returned NaN rows at
D = 8 (cases 25 and 38; D = 536 is case 37): only lanes with a chunk of the row entered the loop, so with D / 8 % 64 < n_real the table
registers of the missing lanes were never loaded.  The loop now admits whole waves (csrc/umoe_misc.hip).
"""
import functools
import math

import pytest
import torch

gpu = pytest.mark.gpu

U = 2.0 ** -24          # fp32 unit roundoff
BF = 2.0 ** -8          # bf16: half an ulp relative to the value, at most
SENT = 7.0              # sentinel of the bf16 output buffers
CAP = 1e-2              # largest flagged share of a case
FLT_MAX = 3.4028234663852886e38
f64 = torch.float64
f32 = torch.float32
bf16 = torch.bfloat16
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from unimoe_audio_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ helpers
def gen(seed):
    return torch.Generator().manual_seed(seed)


def rbf(x):
    """round a float64 (or float32) tensor to bf16, returned in the input's dtype"""
    return x.to(f32).to(bf16).to(x.dtype)


def to_bf(x):
    return x.to(f32).to(bf16)


def ulp_bf16(x):
    """spacing of the bf16 grid at |x|: |x| = m 2^e, m in [0.5, 1) -> 2^(e - 8), never below the subnormal spacing 2^-133"""
    _, e = torch.frexp(x.abs().to(f64))
    return torch.ldexp(torch.ones_like(x, dtype=f64), (e - 8).clamp(min=-133))


def mid_dist(x):
    """distance of x to the nearest bf16 rounding midpoint"""
    ul = ulp_bf16(x)
    t = x.abs().to(f64) / ul
    return (t - torch.floor(t) - 0.5).abs() * ul


def other_bf16(x):
    """the bf16 neighbour of x on the far side of the rounding midpoint next to x"""
    r = rbf(x)
    return r + torch.sign(x - r) * ulp_bf16(x)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def same_bits(name, got, want):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (name, g.shape, w.shape)
    if not torch.equal(g, w):
        bad = torch.nonzero(g != w)
        raise AssertionError(f"{name}: {bad.shape[0]} of {g.numel()} elements differ in their bits, the first at {bad[0].tolist()}")


def bf16_out(ref, e32):
    return BF * ref.abs() + (1 + BF) * e32


def r8(n):
    return (n + 7) & ~7


class Stats(dict):
    def note(self, name, v):
        self[name] = max(self.get(name, 0.0), float(v))

    def add(self, name, v):
        self[name] = self.get(name, 0) + v

    def show(self, title):
        print(f"\nFWD FP64 {title}: " + ", ".join(f"{k} {v:.3g}" for k, v in self.items()))


def check(name, got, ref, bound, stats):
    """|got - ref| <= bound per element; got must be finite everywhere"""
    got = got.detach().cpu().to(f64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite value"
    err = (got - ref).abs()
    ratio = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    stats.note(name, worst)
    if not worst <= 1.0:
        i = int(ratio.argmax())
        raise AssertionError(f"{name}: error / bound = {worst:.4g} (error {float(err.flatten()[i]):.4g}, bound {float(bound.flatten()[i]):.4g}, flat index {i})")


def two_way(v, win):
    """one bf16 rounding point of the candidate rule: -> ([rbf(v)] or [rbf(v), the same with the flagged elements on their other
    neighbour], flag).  win: the fp32 error window of v (absolute, per element); win == 0 never flags (an exact step, where a value ON a
    midpoint rounds to even in both)."""
    base = rbf(v)
    flag = (mid_dist(v) <= win) & (win > 0)
    if not bool(flag.any()):
        return [base], flag
    return [base, torch.where(flag, other_bf16(v), base)], flag


def check_cands(name, got, cands, flag, stats):
    """got (bf16) equals cands[0] bit for bit wherever flag is False, and one of cands where it is True (the candidates equal
    cands[0] wherever nothing is flagged, by construction).  Counts the flagged elements that took another chain than the first."""
    g = bits(got)
    base = bits(to_bf(cands[0]))
    assert g.shape == base.shape, (name, g.shape, base.shape)
    ok = g == base
    alt = ~ok
    for c in cands[1:]:
        ok |= g == bits(to_bf(c))
    stats.note(name + " flagged share", float(flag.double().mean()) if flag.numel() else 0.0)
    stats.add(name + " alternative chains taken", int((alt & ok).sum()))
    if not bool(ok.all()):
        bad = torch.nonzero(~ok)
        n_unflagged = int((~ok & ~flag).sum())
        raise AssertionError(f"{name}: {bad.shape[0]} of {g.numel()} elements match no chain of the reference ({n_unflagged} of them unflagged), "
                             f"the first at {bad[0].tolist()}: got {float(got.detach().cpu()[tuple(bad[0])]):.6g}, reference {float(cands[0][tuple(bad[0])]):.6g}")


def _rejects(fn):
    with pytest.raises(AssertionError):
        fn()


# ------------------------------------------------------------------------------------------------ RMSNorm (also the fused norm of combine)
RMS_EPS = 1e-6
EPS32 = float(torch.tensor(RMS_EPS, dtype=f32))         # the kernel takes eps as a float


def rms_window(D):
    return (4 * -(-D // 2048) + 9) * U


def ref_rms_y(x, w, D):
    """x [S, D] float64 (bf16 values), w [D] float64 -> (chains of y = rbf(w rbf(x rs)), flag).  rs = 1 / sqrt(sum x^2 / D + eps) with the
    sum of squares overflowing to inf where fp32 overflows (then rs = 0 and y = +-0, as in the reference model's fp32 variance)."""
    ss = x.pow(2).sum(-1, keepdim=True)
    ss = torch.where(ss > FLT_MAX, torch.full_like(ss, math.inf), ss)
    rs = 1.0 / torch.sqrt(ss / D + EPS32)
    v = x * rs
    vs, flag = two_way(v, rms_window(D) * v.abs())
    return [rbf(w * t) for t in vs], flag


RMS_CASES = [(D, S) for D in (8, 504, 2048, 2056, 4096, 6144) for S in (1, 3, 257)]
RMS_SPECIAL = 10         # S = 257: rows 10 .. 14 are the special rows


def _rms_seed(D, S):
    return 7000 + D + S


@functools.lru_cache(maxsize=None)
def make_rms(D, S):
    g = gen(_rms_seed(D, S))
    x = torch.randn(S, D, generator=g)
    r = torch.randn(S, D, generator=g)
    if S > RMS_SPECIAL + 5:
        k = RMS_SPECIAL
        x[k] *= 1e-3                        # mean(x^2) ~ eps
        x[k + 1] *= 2.0 ** -20              # mean(x^2) << eps
        x[k + 2] = 0                        # a zero row
        x[k + 3] *= 2.0 ** 60               # sum of squares ~ D 2^120: overflows fp32 at D >= 504
        x[k + 4, : min(4, D)] *= 2.0 ** 60  # a few large elements: 2^122, no overflow
        r[k:k + 5] = x[k:k + 5]             # (x + r = 2 x keeps the rows what they are)
    x, r = x.to(bf16), r.to(bf16)
    w = ((1 + 0.1 * torch.randn(D, generator=g)) * torch.where(torch.rand(D, generator=g) < 0.5, -1.0, 1.0)).to(bf16)      # negative weights
    return dict(D=D, S=S, x=x, r=r, w=w)


@functools.lru_cache(maxsize=None)
def ref_rms(D, S, with_r):
    c = make_rms(D, S)
    xs = rbf(c["x"].to(f64) + c["r"].to(f64)) if with_r else c["x"].to(f64)
    ys, flag = ref_rms_y(xs, c["w"].to(f64), D)
    return dict(xs=xs, ys=ys, flag=flag, share=float(flag.double().mean()))


def emu_rms(c, with_r, bug=None):
    D = c["D"]
    x = c["x"].float()
    if with_r:
        x = rbf(x + c["r"].float())
    ss = (x * x).sum(-1, keepdim=True)
    mean = ss / float(D - 8 if bug == "mean over D - 8" else D)
    rs = torch.rsqrt(mean if bug == "eps omitted" else mean + torch.tensor(RMS_EPS, dtype=f32))
    v = x * rs
    y = c["w"].float() * (v if bug == "weight before the rounding" else rbf(v))
    return y.to(bf16), (x.to(bf16) if with_r else None)


def check_rms(c, r, y, s, stats):
    if s is not None:
        same_bits("sum_out", s, to_bf(r["xs"]))
    check_cands("y", y, r["ys"], r["flag"], stats)
    if c["S"] > RMS_SPECIAL + 5:
        z = y.detach().cpu()[RMS_SPECIAL + 2].float()
        assert bool((z == 0).all()), "y: the zero row is not exactly zero"
        assert bool(torch.isfinite(y.detach().cpu().float()).all()), "y: inf / NaN"


# ------------------------------------------------------------------------------------------------ combine
def K(form="slot", S=16, D=504, n_real=8, n_dyn=9, n_fix=2, shared=True, parts=0, row0=False, resid=True, norm=False, ld="real", dr=0,
      nan0=False, p=0.5):
    """form: 'slot' (ragged slot_of, -1 for unselected) or 'mask' (dense layout: row e * dense_rows + s, expert_mask [S, mask_ld]);
    shared: shared experts' rows given (y_shared, or with row0 inside the partial slabs at shared_row0); parts: number of fp32 partial
    slabs (0: bf16 y_slots); ld: 'real' (mask_ld = n_real) or 'E' (n_dyn + n_fix > n_real, the engine's); dr: dense_rows - S; nan0: row 0
    selected by nobody and NaN; p: share of selected experts"""
    assert not row0 or (parts and shared)
    assert ld == "real" or n_dyn + n_fix > n_real
    return dict(form=form, S=S, D=D, n_real=n_real, n_dyn=n_dyn, n_fix=n_fix, shared=shared, parts=parts, row0=row0, resid=resid, norm=norm,
                ld=ld, dr=dr, nan0=nan0, p=p)


COMBINE_CASES = [
    # the ragged form; fast path (n_real <= 16 and n_fix <= 4, no slabs)
    K(D=2048, norm=True),                                            # 0  production 9/8/2
    K(D=8),                                                          # 1
    K(S=1, D=504, resid=False),                                      # 2
    K(D=2056, norm=True),                                            # 3  thread 0 takes a second pass
    K(D=4096, norm=True),                                            # 4
    K(S=257, norm=True),                                             # 5
    K(n_real=1, n_dyn=1, n_fix=0, resid=False),                      # 6
    K(n_real=15, n_dyn=15, n_fix=1),                                 # 7
    K(n_real=16, n_dyn=16, n_fix=4, p=0.9, D=2048),                  # 8  the last fast shape, ~90 % selected
    K(n_real=16, n_dyn=17, n_fix=0, norm=True),                      # 9
    K(shared=False),                                                 # 10 y_shared = None with n_fix > 0
    # the loop path
    K(n_real=16, n_dyn=16, n_fix=5, D=2056, norm=True),              # 11 n_fix = 5
    K(n_real=17, n_dyn=17, n_fix=4),                                 # 12 n_real = 17
    K(n_real=20, n_dyn=20, n_fix=0, resid=False),                    # 13
    K(n_real=17, n_dyn=18, n_fix=1, shared=False),                   # 14
    K(n_fix=5, nan0=True),                                           # 15 row 0 selected by nobody, NaN
    K(parts=1),                                                      # 16 slabs; shared rows from y_shared
    K(parts=2, row0=True, D=2048, norm=True),                        # 17 shared rows inside the slabs
    K(parts=4, row0=True, D=2056, norm=True),                        # 18
    K(parts=2, shared=False, resid=False),                           # 19
    K(parts=4, row0=True, S=257, n_fix=1),                           # 20
    # the dense form the decode engine launches (combine_kernel<false, true>)
    K("mask", D=2048, n_dyn=8, norm=True),                           # 21 mask_ld = n_real
    K("mask", D=2048, ld="E", norm=True),                            # 22 production 9/8/2, mask_ld = E = 11
    K("mask", D=2056, ld="E", norm=True),                            # 23 thread 0's second pass: tables broadcast in the first only
    K("mask", ld="E", dr=5),                                         # 24 dense_rows > S
    K("mask", D=8, ld="E", resid=False),                             # 25
    K("mask", S=1, ld="E", dr=3),                                    # 26
    K("mask", S=257, ld="E", norm=True),                             # 27
    K("mask", D=4096, ld="E", norm=True),                            # 28
    K("mask", n_real=16, n_dyn=16, n_fix=4, ld="E", p=0.9),          # 29
    K("mask", n_real=1, n_dyn=1, n_fix=1, ld="E"),                   # 30
    K("mask", n_real=15, n_dyn=16, n_fix=1, ld="E", resid=False),    # 31
    # a mask with the generic kernel: fast path, loop path, slabs
    K("mask", n_fix=0, ld="E"),                                      # 32
    K("mask", shared=False, ld="E", dr=2),                           # 33
    K("mask", n_real=17, n_dyn=18, n_fix=2, ld="E"),                 # 34
    K("mask", n_fix=5, ld="E", norm=True),                           # 35
    K("mask", parts=2, row0=True, ld="E", dr=1),                     # 36
    # a wave with fewer lanes in the row loop than there are experts (the dense form broadcasts its tables inside that loop)
    K("mask", D=536, ld="E", norm=True),                             # 37 wave 1 has 3 lanes in the loop
    K("mask", D=8, n_real=16, n_dyn=16, n_fix=4, ld="E", p=0.9),     # 38 one lane, 16 experts
]


@functools.lru_cache(maxsize=None)
def make_combine(idx, exact):
    """exact: weights m / 16, m = 1 .. 7 (3 mantissa bits), y / resid n / 128, |n| <= 255 (slabs: integers / 512 in both passes, their
    sums exact in fp32): every product lies on a grid of 2^-13 below 2^8, every fp32 operation of the kernel is exact"""
    k = COMBINE_CASES[idx]
    S, D, n_real, n_dyn, n_fix = k["S"], k["D"], k["n_real"], k["n_dyn"], k["n_fix"]
    E = n_dyn + n_fix
    g = gen(9000 + 10 * idx + (1 if exact else 0))

    def values(*shape):
        if exact:
            return (torch.randint(-255, 256, shape, generator=g).float() / 128).to(bf16)
        return torch.randn(*shape, generator=g).to(bf16)

    def weights(*shape):
        if exact:
            return torch.randint(1, 8, shape, generator=g).float() / 16
        return torch.rand(*shape, generator=g) + 0.05

    sel = torch.rand(S, n_real, generator=g) < k["p"]
    if S >= 3:
        sel[1] = False           # a token that selected nothing
        sel[2] = True            # a token that selected every expert
    elif idx % 2 == 0:
        sel[0] = True
    row_of = torch.full((S, n_real), -1, dtype=torch.int64)
    if k["form"] == "slot":
        off = 8                  # rows 0 .. 7 belong to nobody (the fast path re-reads row 0 for an unselected expert)
        for e in range(n_real):
            rows = torch.nonzero(sel[:, e]).flatten()
            row_of[rows, e] = off + torch.arange(rows.numel())
            off = r8(off + rows.numel()) + 8
        n_rows, dense_rows = off, 0
    else:
        dense_rows = S + k["dr"]
        row_of = torch.arange(n_real)[None, :] * dense_rows + torch.arange(S)[:, None]
        n_rows = n_real * dense_rows
    used = torch.zeros(n_rows, dtype=torch.bool)
    used[row_of[sel]] = True
    keep = used.clone()
    keep[0] = not k["nan0"]      # row 0 stays finite: the fast path re-reads it for unselected experts (value never used)
    assert not (k["nan0"] and bool(used[0]))
    n_sh = n_fix * S if k["shared"] else 0
    c = dict(k=k, idx=idx, sel=sel, row_of=row_of, dense_rows=dense_rows, used=used, y_slots=None, y_parts=None, y_shared=None, shared_row0=-1)
    if k["parts"]:
        tot = n_rows + (n_sh if k["row0"] else 0)
        P = torch.randint(-1024, 1025, (k["parts"], tot, D), generator=g).float() / 512
        P[:, :n_rows][:, ~keep] = NAN
        y_all = rbf(P.to(f64).sum(0))
        c["y_parts"], c["y64"] = P, y_all[:n_rows]
        if k["row0"]:
            c["shared_row0"], c["ysh64"] = n_rows, y_all[n_rows:]
    else:
        y = values(n_rows, D)
        y[~keep] = NAN
        c["y_slots"], c["y64"] = y, y.to(f64)
    if k["shared"] and not k["row0"]:
        c["y_shared"] = values(n_sh, D) if n_sh else None
        c["ysh64"] = c["y_shared"].to(f64) if n_sh else torch.zeros(0, D, dtype=f64)
    w = weights(S, n_real) * sel
    if not exact:
        w = w / w.sum(-1, keepdim=True).clamp_min(1e-3)
    w[~sel] = NAN                # the weight of an unselected expert is read into a lane and never used
    gw = torch.full((S, E), NAN)
    gw[:, n_dyn:] = weights(S, n_fix) * (1.0 if exact else 0.4)
    c["w"], c["gw"] = w.contiguous(), gw.contiguous()
    c["resid"] = values(S, D) if k["resid"] else None
    c["norm_w"] = ((1 + 0.1 * torch.randn(D, generator=g)) * torch.where(torch.rand(D, generator=g) < 0.5, -1.0, 1.0)).to(bf16) if k["norm"] else None
    if k["form"] == "slot":
        c["slot_of"], c["mask"], c["mask_ld"] = row_of.to(torch.int32).contiguous(), None, 0
    else:
        ld = n_real if k["ld"] == "real" else E
        m = (torch.rand(S, ld, generator=g) < 0.5).to(torch.int32)          # the columns at and beyond n_real: not the kernel's business
        if ld > n_real and n_fix:
            m[:, ld - n_fix:] = 1
        m[:, :n_real] = sel.to(torch.int32)
        c["slot_of"], c["mask"], c["mask_ld"] = None, m.contiguous(), ld
    return c


@functools.lru_cache(maxsize=None)
def ref_combine(idx, exact):
    """a = rbf(sum_e w y) over the selected experts; per shared expert a = rbf(a + rbf(y_sh gw[n_dyn + i])); out = rbf(resid + a).
    -> chains of out, flag (any flagged point of the first chain), share"""
    c = make_combine(idx, exact)
    k = c["k"]
    S, D, n_real, n_dyn, n_fix = k["S"], k["D"], k["n_real"], k["n_dyn"], k["n_fix"]
    w, y = c["w"].to(f64), c["y64"]
    acc, ab = torch.zeros(S, D, dtype=f64), torch.zeros(S, D, dtype=f64)
    for e in range(n_real):
        rows = torch.nonzero(c["sel"][:, e]).flatten()
        t = w[rows, e, None] * y[c["row_of"][rows, e]]
        acc[rows] += t
        ab[rows] += t.abs()
    n_sel = c["sel"].sum(-1, keepdim=True).to(f64)
    chains, flag = two_way(acc, torch.zeros_like(ab) if exact else (n_sel + 1) * U * ab)
    if k["shared"]:
        for i in range(n_fix):
            p = c["ysh64"][i * S:(i + 1) * S] * c["gw"].to(f64)[:, n_dyn + i, None]
            ps, f = two_way(p, torch.zeros_like(p) if exact else U * p.abs())
            flag = flag | f
            chains = [rbf(a + q) for a in chains for q in ps]            # the sum of two bf16 values is exact in fp32
    if c["resid"] is not None:
        chains = [rbf(c["resid"].to(f64) + a) for a in chains]
    assert bool(torch.isfinite(chains[0]).all())
    return dict(out=chains, flag=flag, share=float(flag.double().mean()))


def emu_combine(c, bug=None):
    """the kernel's arithmetic in fp32 torch operations, experts in ascending order; bug: one of the planted errors"""
    k = c["k"]
    S, D, n_real, n_dyn, n_fix = k["S"], k["D"], k["n_real"], k["n_dyn"], k["n_fix"]
    y = c["y64"].float()
    sel, w = c["sel"].clone(), c["w"].clone()
    if bug == "mask_ld taken as n_real":
        sel = c["mask"].flatten()[: S * n_real].view(S, n_real) != 0
    if bug == "one selected expert dropped":
        sel[2, n_real // 2] = False
    if bug == "the neighbour's weight":
        w[2] = w[2].roll(1)
    acc = torch.zeros(S, D)
    for e in range(n_real):
        rows = torch.nonzero(sel[:, e]).flatten()
        acc[rows] = acc[rows] + w[rows, e, None] * y[c["row_of"][rows, e].clamp_min(0)]
    if bug == "an unselected NaN row added":
        acc[0] = acc[0] + 0.0 * y[int(torch.nonzero(torch.isnan(y[:, 0]))[0])]
    once = bug == "rounded once at the end"
    a = acc if once else rbf(acc)
    res = c["resid"].float() if c["resid"] is not None else None
    if k["shared"]:
        for i in range(n_fix):
            col = i if bug == "shared weight from column i" else n_dyn + i
            p = c["ysh64"].float()[i * S:(i + 1) * S] * c["gw"][:, col, None]
            if once:
                a = a + p
            elif bug == "residual before the last rounding" and i == n_fix - 1:
                a, res = rbf(a + rbf(p) + res), None
            else:
                a = rbf(a + rbf(p))
    if res is not None:
        a = res + a
    return a.to(bf16)


def emu_norm(out, c, bug=None):
    return emu_rms(dict(D=c["k"]["D"], x=out, w=c["norm_w"]), False, bug)[0]


def check_combine(c, r, out, hn, stats):
    """out against the chains; the fused norm against the RMSNorm rule applied to the out it was given"""
    check_cands("out", out, r["out"], r["flag"], stats)
    if c["norm_w"] is not None:
        ys, flag = ref_rms_y(out.detach().cpu().to(f64), c["norm_w"].to(f64), c["k"]["D"])
        check_cands("norm_out", hn, ys, flag, stats)
        return float(flag.double().mean())
    assert hn is None
    return 0.0


# ------------------------------------------------------------------------------------------------ mRoPE + KV append
ROPE_POS = 5000          # rows of the cos / sin tables
ROPE_CASES = [          # H, KVH, hd, sections, T, rows
    (1, 1, 8, (1, 2, 1), 1, 1), (1, 1, 8, (2, 1, 1), 5, 3), (1, 1, 8, (0, 4, 0), 37, 1),
    (2, 1, 64, (3, 2, 27), 37, 1), (2, 1, 64, (16, 8, 8), 5, 3), (2, 1, 64, (11, 13, 8), 1, 3),
    (16, 2, 128, (16, 24, 24), 37, 3), (16, 2, 128, (3, 2, 59), 1, 3), (16, 2, 128, (16, 24, 24), 5, 1), (16, 2, 128, (17, 23, 24), 37, 1),
]


@functools.lru_cache(maxsize=None)
def make_rope(idx):
    H, KVH, hd, sec, T, rows = ROPE_CASES[idx]
    g = gen(11000 + idx)
    n_tok, half = rows * T, hd // 2
    Lmax = T + 8
    qkv = torch.randn(n_tok, (H + 2 * KVH) * hd, generator=g).to(bf16)
    cos = (2 * torch.rand(ROPE_POS, half, generator=g) - 1).to(bf16)            # (not cos and sin of anything: every entry its own value)
    sin = (2 * torch.rand(ROPE_POS, half, generator=g) - 1).to(bf16)
    pos3 = torch.randint(2000, ROPE_POS - 2100, (3, n_tok), generator=g)       # three distinct streams, all below the last row
    pos3[1] = pos3[0] + 1 + torch.randint(0, 1000, (n_tok,), generator=g)
    pos3[2] = pos3[1] + 1 + torch.randint(0, 1000, (n_tok,), generator=g)
    pos3[0, 0] = ROPE_POS - 1                                                    # the tables' last row
    if n_tok >= 3:
        pos3[1, n_tok - 1], pos3[2, n_tok // 2] = ROPE_POS - 1, ROPE_POS - 1
    pos3 = pos3.to(torch.int32)
    kv = []
    for r in range(rows):                                                        # distinct slots in no order; slot Lmax - 1 and slot 0 named
        first = Lmax - 1 if r % 2 == 0 else 0
        rest = [v for v in torch.randperm(Lmax, generator=g).tolist() if v != first][: T - 1]
        kv.append(torch.tensor([first] + rest, dtype=torch.int64))
    kv_pos = torch.cat(kv).to(torch.int32)
    return dict(H=H, KVH=KVH, hd=hd, sec=sec, T=T, rows=rows, n_tok=n_tok, Lmax=Lmax, qkv=qkv, cos=cos, sin=sin, pos3=pos3.contiguous(), kv_pos=kv_pos)


def rope_chain(c, x, mul, add, bug=None):
    """q / k rotated and the expected caches; x the qkv values, mul(a, b) / add(a, b) the rounded operations"""
    H, KVH, hd, (s0, s1, _), T = c["H"], c["KVH"], c["hd"], c["sec"], c["T"]
    n_tok, half, Lmax = c["n_tok"], hd // 2, c["Lmax"]
    i = torch.arange(half)
    b0 = s0 + (1 if bug == "section boundary off by one" else 0)
    stream = (i >= b0).long() + (i >= s0 + s1).long() * (0 if bug == "stream 1 for section 2" else 1)
    pos = c["pos3"].long()[stream, :].t()                                        # [n_tok, half]
    cs, sn = c["cos"].to(x.dtype)[pos, i[None]][:, None], c["sin"].to(x.dtype)[pos, i[None]][:, None]
    x = x.view(n_tok, H + 2 * KVH, hd)
    x1, x2 = x[:, :H + KVH, :half], x[:, :H + KVH, half:]
    sg = 1.0 if bug == "sign of the sine term" else -1.0
    rot = torch.cat([add(mul(x1, cs), mul(sg * x2, sn)), add(mul(x2, cs), mul(x1, sn))], -1)
    kc = torch.full((c["rows"], KVH, Lmax, hd), SENT, dtype=x.dtype)
    vc = torch.full((c["rows"], KVH, Lmax, hd), SENT, dtype=x.dtype)
    row = torch.arange(n_tok) // T
    slot = (c["kv_pos"].long() + (1 if bug == "slot kv_pos + 1" else 0)) % Lmax
    kc[row, :, slot] = rot[:, H:]
    vc[row, :, slot] = x[:, H + KVH:]
    return rot[:, :H].reshape(n_tok, H * hd), kc, vc


@functools.lru_cache(maxsize=None)
def ref_rope(idx):
    """o1 = rbf(rbf(x1 c) + rbf(-x2 s)), o2 = rbf(rbf(x2 c) + rbf(x1 s)), V copied: products of two bf16 values and sums of two bf16
    values are exact in fp32, so float64 with the same roundings fixes every bit"""
    c = make_rope(idx)
    return [to_bf(t) for t in rope_chain(c, c["qkv"].to(f64), lambda a, b: rbf(a * b), lambda a, b: rbf(a + b))]


def emu_rope(c, bug=None):
    return rope_chain(c, c["qkv"].clone(), torch.mul, torch.add, bug)            # torch's bf16 operations round every result once


def check_rope(ref, q, kc, vc):
    same_bits("q_out", q, ref[0])
    same_bits("k_cache", kc, ref[1])
    same_bits("v_cache", vc, ref[2])


# ------------------------------------------------------------------------------------------------ vision_rope
VROPE_CASES = [(1, 1, 8), (7, 1, 80), (7, 16, 8), (1, 16, 128), (7, 16, 80), (7, 1, 128)]          # S, H, hd
VROPE_BIG = (1100, 16, 80)                                                                       # S 2 H hd / 2 > 4096 * 256


def make_vrope(S, H, hd):
    g = gen(12000 + S + 3 * H + hd)
    qkv = torch.randn(S, 3, H, hd, generator=g).to(bf16)
    ang = 6.3 * torch.rand(S, hd, generator=g)                                   # first and second half differ (the model's are equal)
    return dict(S=S, H=H, hd=hd, qkv=qkv, cos=ang.cos().contiguous(), sin=(ang + 0.3 * torch.rand(S, hd, generator=g)).sin().contiguous())


def ref_vrope(c):
    """out[d] = a c[d] - b s[d], out[d + half] = b c[d + half] + a s[d + half] in fp32, one rounding: two products and a sum,
    bound 2^-8 |ref| + (1 + 2^-8) 2 u (|a c| + |b s|)"""
    half = c["hd"] // 2
    x = c["qkv"].to(f64)[:, :2]
    a, b = x[..., :half], x[..., half:]
    cs, sn = c["cos"].to(f64)[:, None, None], c["sin"].to(f64)[:, None, None]
    lo, hi = a * cs[..., :half] - b * sn[..., :half], b * cs[..., half:] + a * sn[..., half:]
    e_lo = 2 * U * ((a * cs[..., :half]).abs() + (b * sn[..., :half]).abs())
    e_hi = 2 * U * ((b * cs[..., half:]).abs() + (a * sn[..., half:]).abs())
    ref = torch.cat([lo, hi], -1)
    return ref, bf16_out(ref, torch.cat([e_lo, e_hi], -1))


def emu_vrope(c, bug=None):
    half = c["hd"] // 2
    x = c["qkv"].float()[:, :2]
    a, b = x[..., :half], x[..., half:]
    cs, sn = c["cos"][:, None, None], c["sin"][:, None, None]
    c1 = cs[..., :half] if bug == "second-half cos from the first half" else cs[..., half:]
    out = c["qkv"].clone()
    out[:, :2] = torch.cat([a * cs[..., :half] + (-b) * sn[..., :half], b * c1 + a * sn[..., half:]], -1).to(bf16)
    return out


def check_vrope(c, ref, bound, got, stats):
    check("q, k", got.detach().cpu()[:, :2], ref, bound, stats)
    same_bits("v", got.detach().cpu()[:, 2], c["qkv"][:, 2])


# ------------------------------------------------------------------------------------------------ vision_attn
C1, C2 = 1.25, 2.0 ** -18            # form, constants and justification: tests/test_gpu_attn_decode.py
SEG_LENS = (1, 2, 63, 64, 65, 128, 129)
VATTN_CASES = [(1, 8), (2, 64), (1, 72), (16, 80), (2, 128), (16, 128), (16, 8), (1, 64)]          # H, hd
SIGMA_K = 0.3                        # score std ~0.3: every key matters


def vattn_layout():
    """guard, segment, guard, segment ... guard: the segments' edges are no multiples of 64; a guard's own segment is empty"""
    segs, t = [], 1
    for n in SEG_LENS:
        segs.append((t, t + n))
        t += n + 1
    S = t
    lo, hi = torch.arange(S, dtype=torch.int32), torch.arange(S, dtype=torch.int32)
    for a, b in segs:
        lo[a:b], hi[a:b] = a, b
    real = hi > lo
    assert all(a % 64 and b % 64 for a, b in segs)
    return S, segs, lo, hi, real


@functools.lru_cache(maxsize=None)
def make_vattn(H, hd, indicator):
    g = gen(13000 + 7 * H + hd + (1 if indicator else 0))
    S, segs, lo, hi, real = vattn_layout()
    qkv = torch.randn(S, 3, H, hd, generator=g)
    qkv[:, 1] *= SIGMA_K
    if indicator:
        qkv[:, 2] = (torch.arange(S)[:, None] % hd == torch.arange(hd)[None, :]).float()[:, None, :]
    qkv[~real] = NAN
    qkv = qkv.to(bf16).contiguous()
    return dict(S=S, H=H, hd=hd, segs=segs, lo=lo, hi=hi, real=real, qkv=qkv, scale=float(hd) ** -0.5, vmax=float(qkv[real][:, 2].float().abs().max()))


def vattn_keys(c, mutation=None):
    """per segment the keys its tokens attend to; mutation: the error planted into the reference"""
    out = []
    for i, (a, b) in enumerate(c["segs"]):
        keys = list(range(a, b))
        if mutation == "first key dropped":
            keys = keys[1:]
        elif mutation == "last key dropped":
            keys = keys[:-1]
        elif mutation == "the neighbour segment's first key added":
            keys = keys + [c["segs"][(i + 1) % len(c["segs"])][0]]
        out.append(keys)
    return out


def vattn_ref(c, dtype=f64, mutation=None, scale=None):
    """scores -> softmax -> P V per (token, head) in `dtype`; rows outside every segment (and tokens left without a key) are zeros"""
    S, H, hd = c["S"], c["H"], c["hd"]
    x = c["qkv"].to(dtype)
    out = torch.zeros(S, H, hd, dtype=dtype)
    for (a, b), keys in zip(c["segs"], vattn_keys(c, mutation)):
        if not keys:
            continue
        kk = torch.tensor(keys)
        s = torch.einsum("qhd,khd->hqk", x[a:b, 0], x[kk, 1]) * (c["scale"] if scale is None else scale)
        out[a:b] = torch.einsum("hqk,khd->qhd", torch.softmax(s, -1), x[kk, 2])
    return out


def vattn_bound(ref, vmax):
    return C1 * BF * ref.abs() + C2 * vmax


def check_vattn(c, ref, got, stats):
    got = got.detach().cpu().view(c["S"], c["H"], c["hd"])
    assert not bool(torch.isnan(got.float()).any()), "out: NaN (a guard token's q, k or v leaked into a sum)"
    assert bool((bits(got[~c["real"]]) == 0).all()), "out: a token with an empty segment is not exactly +0"
    check("out", got, ref, vattn_bound(ref, c["vmax"]), stats)


def vattn_self_check(c, got):
    """the reference with the first or the last key of a segment dropped, or with the neighbour segment's first key added, must break
    the bound on every token of every segment"""
    got = got.detach().cpu().view(c["S"], c["H"], c["hd"]).to(f64)
    n = 0
    for mutation in ("first key dropped", "last key dropped", "the neighbour segment's first key added"):
        mut = vattn_ref(c, f64, mutation)
        viol = ((got - mut).abs() > vattn_bound(mut, c["vmax"])).flatten(1).any(-1)
        for a, b in c["segs"]:
            assert bool(viol[a:b].all()), f"self-check: '{mutation}' in segment [{a}, {b}) stays within the bound"
            n += b - a
    return n


# ------------------------------------------------------------------------------------------------ swiglu_pair
SPECIAL_G = [0.0, -0.0, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0]        # expf(88) is finite, expf(100) overflows, expf(-100) flushes
SWIGLU_CASES = sorted({(I, ldh, S) for I in (8, 348, 3420) for ldh in (I, r8(I), I + 24) for S in (1, 5)})
SWIGLU_BIG = (3420, 3424, 613)                                          # S ldh > 8192 * 256


@functools.lru_cache(maxsize=None)
def make_swiglu(I, ldh, S):
    g = gen(14000 + I + ldh + S)
    gu = torch.randn(S, 2 * I, generator=g)
    gu[0, :len(SPECIAL_G)] = torch.tensor(SPECIAL_G)
    gu[0, I:I + len(SPECIAL_G)] = torch.tensor([1.5, -1.5, 1.25, 1.75, -1.5, 1.5, 1.5, -1.25])      # (keeps silu(-88) u a normal number)
    if S > 1:
        gu[S - 1, I - len(SPECIAL_G):I] = torch.tensor(SPECIAL_G)
        gu[S - 1, 2 * I - len(SPECIAL_G):] = torch.tensor([-1.5, 1.5, -1.25, 1.75, 1.5, 1.5, -1.5, 1.25])
    return dict(I=I, ldh=ldh, S=S, gu=gu.to(bf16).contiguous())


@functools.lru_cache(maxsize=None)
def ref_swiglu(I, ldh, S):
    """h = rbf(rbf(g / (1 + exp(-g))) u): the quotient is the one inexact step, window 6.5 u |silu| (expf 3 u, add u, divide 2.5 u);
    the product of two bf16 values is exact in fp32.  Columns [I, ldh) are +0."""
    c = make_swiglu(I, ldh, S)
    gt, up = c["gu"][:, :I].to(f64), c["gu"][:, I:].to(f64)
    raw = gt * torch.sigmoid(gt)
    ss, flag = two_way(raw, 6.5 * U * raw.abs())
    pad = torch.zeros(S, ldh - I, dtype=f64)
    return dict(h=[torch.cat([rbf(s * up), pad], -1) for s in ss], flag=torch.cat([flag, pad.bool()], -1), share=float(flag.double().mean()))


def emu_swiglu(c, bug=None):
    I, ldh, S = c["I"], c["ldh"], c["S"]
    gt, up = c["gu"][:, :I].float(), c["gu"][:, I:].float()
    silu = gt / (1.0 + torch.exp(-gt))
    h = torch.full((S, ldh), SENT if bug == "padding not zeroed" else 0.0, dtype=bf16)
    h[:, :I] = ((silu if bug == "silu not rounded" else rbf(silu)) * up).to(bf16)
    return h


# ------------------------------------------------------------------------------------------------ gelu
GELU_N = (1, 255, 256, 257)
GELU_BIG = 8192 * 256 + 777


@functools.lru_cache(maxsize=None)
def make_gelu(n):
    g = gen(15000 + n % 1000)
    pool = torch.cat([torch.linspace(-8, 8, 2049), torch.randn(4096, generator=g), torch.tensor([0.0, -0.0])])
    x = pool[torch.randint(0, pool.numel(), (n,), generator=g)]
    x[-1] = -0.0
    if n > 2:
        x[0], x[1] = 0.0, -8.0
    return x.to(bf16)


def ref_gelu(x):
    """0.5 v (1 + erf(v / sqrt 2)), fp32, one rounding.  bound 2^-8 |ref| + (1 + 2^-8) 0.5 |v| (16 2 u |erf| + 3 u |1 + erf|): erff within
    16 ulp (the OpenCL limit; it matters in the negative tail, where 1 + erf cancels), the scaling of the argument, the add and the
    two products.  1 + erf is taken as erfc(-v / sqrt 2), which does not cancel."""
    v = x.to(f64)
    t = v / math.sqrt(2.0)
    erf, one_p = torch.special.erf(t), torch.special.erfc(-t)
    ref = 0.5 * v * one_p
    return ref, bf16_out(ref, 0.5 * v.abs() * (16 * 2 * U * erf.abs() + 3 * U * one_p.abs()))


def emu_gelu(x, bug=None):
    v = x.float()
    return (0.5 * v * (1.0 + torch.erf(v if bug == "erf argument unscaled" else v * 0.70710678118654752440))).to(bf16)


# ================================================================================================ CPU self-checks
def test_helpers_cpu():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, 1.0 + 2.0 ** -8 - 2.0 ** -20, -3.0, 0.0, 3.7e-42], dtype=f64)
    assert rbf(x).tolist()[:5] == [1.0, 1.0, 1.0 + 2.0 ** -7, 1.0, -3.0]
    assert ulp_bf16(x).tolist()[:5] == [2.0 ** -7, 2.0 ** -7, 2.0 ** -7, 2.0 ** -7, 2.0 ** -6]
    assert float(ulp_bf16(x)[6]) == 2.0 ** -133
    assert mid_dist(x).tolist()[1] == 0.0 and abs(mid_dist(x).tolist()[2] - 2.0 ** -20) < 1e-18
    assert other_bf16(x[2:4]).tolist() == [1.0, 1.0 + 2.0 ** -7]
    cands, flag = two_way(x[:5], 2.0 ** -19 * torch.ones(5, dtype=f64))
    assert flag.tolist() == [False, True, True, True, False] and len(cands) == 2
    st = Stats()
    check_cands("t", to_bf(cands[1]), cands, flag, st)
    bad = cands[0].clone()
    bad[0] = 1.0 + 2.0 ** -7                                       # an unflagged element on its other neighbour
    _rejects(lambda: check_cands("t", to_bf(bad), cands, flag, Stats()))
    assert two_way(x[1:2], torch.zeros(1, dtype=f64))[1].tolist() == [False]       # an exact step never flags


def test_rmsnorm_checker_cpu():
    st = Stats()
    for D, S in RMS_CASES:
        c = make_rms(D, S)
        for with_r in (False, True):
            r = ref_rms(D, S, with_r)
            assert r["share"] <= CAP and (r["share"] == 0 or S * D >= 1.0 / CAP), (D, S, with_r, r["share"])
            check_rms(c, r, *emu_rms(c, with_r), st)
    st.show("rmsnorm (emulation)")
    for D in (504, 2048, 6144):
        S = 257 if D < 6144 else 3
        c, r = make_rms(D, S), ref_rms(D, S, False)
        for bug in (("eps omitted",) if S == 257 else ()) + ("weight before the rounding", "mean over D - 8"):
            _rejects(lambda: check_rms(c, r, *emu_rms(c, False, bug), Stats()))
    c, r = make_rms(504, 257), ref_rms(504, 257, True)
    y, s = emu_rms(c, True)
    bad = s.clone()
    bad[100, 7] = c["x"][100, 7]                                   # sum_out without its residual
    _rejects(lambda: check_rms(c, r, y, bad, Stats()))
    bad = y.clone()
    bad[RMS_SPECIAL + 2, 5] = 2.0 ** -100                          # the zero row not exactly zero
    _rejects(lambda: check_rms(c, r, bad, s, Stats()))


def test_combine_checker_cpu():
    st = Stats()
    for idx in range(len(COMBINE_CASES)):
        for exact in (False, True):
            c, r = make_combine(idx, exact), ref_combine(idx, exact)
            k = c["k"]
            assert r["share"] <= CAP and (r["share"] == 0 or k["S"] * k["D"] >= 1.0 / CAP), (idx, exact, r["share"])
            assert not exact or (r["share"] == 0 and len(r["out"]) == 1)
            out = emu_combine(c)
            share = check_combine(c, r, out, emu_norm(out, c) if k["norm"] else None, st)
            assert share <= CAP, (idx, exact, share)
    st.show("combine (emulation)")
    # the forms the case list must reach
    ks = COMBINE_CASES
    assert {k["n_real"] for k in ks} >= {1, 15, 16, 17, 20} and {k["n_fix"] for k in ks} >= {0, 1, 4, 5}
    assert {k["parts"] for k in ks} >= {0, 1, 2, 4} and {k["D"] for k in ks} >= {8, 504, 2048, 2056, 4096} and {k["S"] for k in ks} >= {1, 16, 257}
    assert any(k["form"] == "mask" and k["dr"] > 0 for k in ks) and any(k["parts"] and not k["row0"] for k in ks)
    for idx, bugs in ((0, ("one selected expert dropped", "the neighbour's weight", "shared weight from column i", "rounded once at the end",
                           "residual before the last rounding", "an unselected NaN row added")),
                      (22, ("mask_ld taken as n_real", "one selected expert dropped", "an unselected NaN row added")),
                      (17, ("rounded once at the end", "shared weight from column i"))):
        c, r = make_combine(idx, False), ref_combine(idx, False)
        for bug in bugs:
            _rejects(lambda: check_combine(c, r, emu_combine(c, bug), emu_norm(emu_combine(c, bug), c) if c["k"]["norm"] else None, Stats()))
    c, r = make_combine(0, True), ref_combine(0, True)                           # the exact-data pass sees a rounding left out
    _rejects(lambda: check_combine(c, r, emu_combine(c, "rounded once at the end"), emu_norm(emu_combine(c), c), Stats()))
    c, r = make_combine(0, False), ref_combine(0, False)                         # the fused norm is checked too
    out = emu_combine(c)
    for bug in ("weight before the rounding", "mean over D - 8"):                # (a missing eps shows only on a small row: test_rmsnorm_checker_cpu)
        _rejects(lambda: check_combine(c, r, out, emu_norm(out, c, bug), Stats()))


def test_rope_checker_cpu():
    for idx in range(len(ROPE_CASES)):
        check_rope(ref_rope(idx), *emu_rope(make_rope(idx)))
    for idx in (1, 3, 6):
        c, ref = make_rope(idx), ref_rope(idx)
        assert c["sec"][0] % 8 or c["sec"] == (16, 24, 24)
        for bug in ("section boundary off by one", "sign of the sine term", "stream 1 for section 2", "slot kv_pos + 1"):
            _rejects(lambda: check_rope(ref, *emu_rope(c, bug)))
    c = make_rope(6)
    assert int(c["pos3"].max()) == ROPE_POS - 1 and bool((c["pos3"][0] != c["pos3"][1]).all() and (c["pos3"][1] != c["pos3"][2]).all())
    assert bool((c["kv_pos"].view(c["rows"], -1).diff(dim=-1) < 0).any())       # not monotonic
    assert {int(v) for v in c["kv_pos"]} >= {0, c["Lmax"] - 1}


def test_vision_rope_checker_cpu():
    st = Stats()
    for S, H, hd in VROPE_CASES:
        c = make_vrope(S, H, hd)
        check_vrope(c, *ref_vrope(c), emu_vrope(c), st)
    assert max(st.values()) <= 1.0
    S, H, hd = VROPE_BIG
    assert S * 2 * H * (hd // 2) > 4096 * 256
    c = make_vrope(7, 16, 80)
    _rejects(lambda: check_vrope(c, *ref_vrope(c), emu_vrope(c, "second-half cos from the first half"), Stats()))
    bad = emu_vrope(c)
    bad[3, 2, 5, 7] = 0.5                                          # V touched
    _rejects(lambda: check_vrope(c, *ref_vrope(c), bad, Stats()))


def test_vision_attn_checker_cpu():
    st = Stats()
    for H, hd in VATTN_CASES[:5]:
        for indicator in (True, False):
            c = make_vattn(H, hd, indicator)
            ref, emu = vattn_ref(c), vattn_ref(c, f32).to(bf16)
            check_vattn(c, ref, emu, st)
            assert vattn_self_check(c, emu) == 3 * sum(SEG_LENS)
            for mutation in ("first key dropped", "last key dropped", "the neighbour segment's first key added"):
                _rejects(lambda: check_vattn(c, ref, vattn_ref(c, f32, mutation).to(bf16), Stats()))
            _rejects(lambda: check_vattn(c, ref, vattn_ref(c, f32, scale=1.0).to(bf16), Stats()))          # scale omitted
    assert max(st.values()) <= 1.0
    c = make_vattn(2, 64, False)
    ref = vattn_ref(c)
    bad = vattn_ref(c, f32).to(bf16)
    bad[0, 1, 3] = -0.0                                            # a guard row not exactly +0
    _rejects(lambda: check_vattn(c, ref, bad, Stats()))
    bad = vattn_ref(c, f32).to(bf16)
    bad[c["segs"][3][0], 0, 0] = NAN
    _rejects(lambda: check_vattn(c, ref, bad, Stats()))


def test_swiglu_pair_checker_cpu():
    st = Stats()
    for I, ldh, S in SWIGLU_CASES + [SWIGLU_BIG]:
        c, r = make_swiglu(I, ldh, S), ref_swiglu(I, ldh, S)
        assert r["share"] <= CAP and (r["share"] == 0 or S * I >= 1.0 / CAP), (I, ldh, S, r["share"])
        check_cands("h", emu_swiglu(c), r["h"], r["flag"], st)
    st.show("swiglu_pair (emulation)")
    assert SWIGLU_BIG[1] * SWIGLU_BIG[2] > 8192 * 256
    for case in ((348, 372, 5), (3420, 3424, 5)):
        c, r = make_swiglu(*case), ref_swiglu(*case)
        for bug in ("silu not rounded", "padding not zeroed"):
            _rejects(lambda: check_cands("h", emu_swiglu(c, bug), r["h"], r["flag"], Stats()))
        bad = emu_swiglu(c)
        bad[2, c["I"]] = -0.0                                      # padding -0 instead of +0
        _rejects(lambda: check_cands("h", bad, r["h"], r["flag"], Stats()))


def test_gelu_checker_cpu():
    st = Stats()
    for n in GELU_N + (GELU_BIG,):
        x = make_gelu(n)
        check("gelu", emu_gelu(x), *ref_gelu(x), st)
    assert max(st.values()) <= 1.0
    x = make_gelu(257)
    _rejects(lambda: check("gelu", emu_gelu(x, "erf argument unscaled"), *ref_gelu(x), Stats()))
    x = make_gelu(GELU_BIG)
    _rejects(lambda: check("gelu", emu_gelu(x, "erf argument unscaled"), *ref_gelu(x), Stats()))


# ================================================================================================ GPU tests
def _d(t, dev):
    return None if t is None else t.to(dev)


def _unchanged(name, on_dev, on_cpu):
    if on_cpu is not None:
        same_bits(name + " (an input)", on_dev, on_cpu)


@gpu
@pytest.mark.parametrize("idx", range(len(COMBINE_CASES)))
def test_combine_vs_fp64(dev, idx):
    """ops.combine at COMBINE_CASES[idx]: the Gaussian pass under the candidate rule, then the exact-data pass bit for bit; the fused norm
    under the RMSNorm rule against the out the kernel produced; inputs unchanged."""
    from unimoe_audio_amd import ops
    st = Stats()
    for exact in (False, True):
        c, r = make_combine(idx, exact), ref_combine(idx, exact)
        k = c["k"]
        names = ("y_slots", "slot_of", "w", "y_shared", "gw", "resid", "norm_w", "y_parts", "mask")
        d = {n: _d(c[n], dev) for n in names}
        res = ops.combine(d["y_slots"], d["slot_of"], d["w"], d["y_shared"], d["gw"], d["resid"], k["n_dyn"], k["n_fix"], norm_w=d["norm_w"],
                          rms_eps=RMS_EPS, y_parts=d["y_parts"], shared_row0=c["shared_row0"], expert_mask=d["mask"], mask_ld=c["mask_ld"],
                          dense_rows=c["dense_rows"])
        out, hn = res if k["norm"] else (res, None)
        assert out.shape == (k["S"], k["D"]) and out.dtype == bf16
        if exact:
            same_bits("out (exact data)", out, to_bf(r["out"][0]))
        share = check_combine(c, r, out, hn, st)
        assert share <= CAP, share
        for n in names:
            _unchanged(n, d[n], c[n])
    st.show(f"combine case {idx} {({a: b for a, b in COMBINE_CASES[idx].items() if b != K()[a]})}")


@gpu
@pytest.mark.parametrize("D,S", RMS_CASES)
def test_rmsnorm_vs_fp64(dev, D, S):
    """ops.rmsnorm with and without a residual: sum_out = rbf(x + r) bit for bit, y under the candidate rule; at S = 257 the rows with
    mean(x^2) ~ eps and << eps, the zero row (exactly zero), the rows of magnitude 2^60; negative weights everywhere."""
    from unimoe_audio_amd import ops
    c = make_rms(D, S)
    st = Stats()
    x, rr, w = c["x"].to(dev), c["r"].to(dev), c["w"].to(dev)
    y = ops.rmsnorm(x, w, RMS_EPS)
    check_rms(c, ref_rms(D, S, False), y, None, st)
    y, s = ops.rmsnorm(x, w, RMS_EPS, resid=rr)
    check_rms(c, ref_rms(D, S, True), y, s, st)
    for n, t in (("x", x), ("r", rr), ("w", w)):
        _unchanged(n, t, c[n])
    st.show(f"rmsnorm D={D} S={S}")


@gpu
@pytest.mark.parametrize("idx", range(len(ROPE_CASES)))
def test_mrope_kvappend_vs_fp64(dev, idx):
    """ops.qkv_mrope_kvappend: q_out, the named K slots and the named V slots bit for bit; every other cache slot keeps the sentinel."""
    from unimoe_audio_amd import ops
    c = make_rope(idx)
    kc = torch.full((c["rows"], c["KVH"], c["Lmax"], c["hd"]), SENT, dtype=bf16, device=dev)
    vc = torch.full_like(kc, SENT)
    d = {n: c[n].to(dev) for n in ("qkv", "cos", "sin", "pos3", "kv_pos")}
    q = ops.qkv_mrope_kvappend(d["qkv"], d["cos"], d["sin"], d["pos3"], d["kv_pos"], c["T"], c["H"], c["KVH"], c["hd"], list(c["sec"]), kc, vc)
    check_rope(ref_rope(idx), q, kc, vc)
    for n, t in d.items():
        _unchanged(n, t, c[n])


@gpu
def test_mrope_kvappend_guards(dev):
    """n_tok = 0 is a success that writes nothing; a section sum that is not hd / 2 and an n_tok that is no multiple of T are refused."""
    import ctypes as C
    from unimoe_audio_amd import _lib as L, ops
    c = make_rope(4)
    kc = torch.full((c["rows"], c["KVH"], c["Lmax"], c["hd"]), SENT, dtype=bf16, device=dev)
    vc = torch.full_like(kc, SENT)
    d = {n: c[n].to(dev) for n in ("qkv", "cos", "sin", "pos3", "kv_pos")}
    q = torch.full((c["n_tok"], c["H"] * c["hd"]), SENT, dtype=bf16, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    a = L.RopeArgs(qkv=p(d["qkv"]), cos_tab=p(d["cos"]), sin_tab=p(d["sin"]), pos3=p(d["pos3"]), kv_pos=p(d["kv_pos"]), n_tok=0, T=c["T"],
                   H=c["H"], KVH=c["KVH"], hd=c["hd"], sec0=c["sec"][0], sec1=c["sec"][1], sec2=c["sec"][2], Lmax=c["Lmax"],
                   q_out=p(q), k_cache=p(kc), v_cache=p(vc))
    assert L.lib().umoe_qkv_mrope_kvappend(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    with pytest.raises(L.UmoeError):
        ops.qkv_mrope_kvappend(d["qkv"], d["cos"], d["sin"], d["pos3"], d["kv_pos"], c["T"], c["H"], c["KVH"], c["hd"], [16, 8, 7], kc, vc)
    with pytest.raises(L.UmoeError):
        ops.qkv_mrope_kvappend(d["qkv"], d["cos"], d["sin"], d["pos3"], d["kv_pos"], c["T"] - 1, c["H"], c["KVH"], c["hd"], list(c["sec"]), kc, vc)
    torch.cuda.synchronize()
    for n, t in (("q_out", q), ("k_cache", kc), ("v_cache", vc)):
        same_bits(n + " after refused / empty calls", t, torch.full_like(t, SENT))


@gpu
@pytest.mark.parametrize("S,H,hd", VROPE_CASES + [VROPE_BIG])
def test_vision_rope_vs_fp64(dev, S, H, hd):
    from unimoe_audio_amd import ops
    c = make_vrope(S, H, hd)
    st = Stats()
    buf = torch.full((S + 1, 3, H, hd), SENT, dtype=bf16, device=dev)          # one row more than the kernel owns
    buf[:S] = c["qkv"].to(dev)
    cos, sin = c["cos"].to(dev), c["sin"].to(dev)
    ops.vision_rope(buf, cos, sin, S, H, hd)
    check_vrope(c, *ref_vrope(c), buf[:S], st)
    same_bits("the row behind the last token", buf[S:], torch.full_like(buf[S:], SENT))
    _unchanged("cos", cos, c["cos"])
    _unchanged("sin", sin, c["sin"])
    st.show(f"vision_rope S={S} H={H} hd={hd}")


@gpu
@pytest.mark.parametrize("H,hd", VATTN_CASES)
def test_vision_attn_vs_fp64(dev, H, hd):
    """segments of 1 .. 129 keys back to back with NaN guard tokens between them, an indicator-V and a random-V pass, the self-check on
    the kernel's own output"""
    from unimoe_audio_amd import ops
    st = Stats()
    n = 0
    for indicator in (True, False):
        c = make_vattn(H, hd, indicator)
        qkv, lo, hi = c["qkv"].to(dev), c["lo"].to(dev), c["hi"].to(dev)
        out = torch.full((c["S"] + 1, H * hd), SENT, dtype=bf16, device=dev)
        ops.vision_attn(qkv, lo, hi, c["S"], H, hd, c["scale"], out)
        check_vattn(c, vattn_ref(c), out[:c["S"]], st)
        n += vattn_self_check(c, out[:c["S"]])
        same_bits("the row behind the last token", out[c["S"]:], torch.full_like(out[c["S"]:], SENT))
        _unchanged("qkv", qkv, c["qkv"])
    st["self-check mutations seen"] = n
    st.show(f"vision_attn H={H} hd={hd}")


@gpu
def test_vision_attn_refuses_head_dims(dev):
    from unimoe_audio_amd import _lib as L, ops
    for hd in (136, 12):
        qkv = torch.zeros(4, 3, 1, hd, dtype=bf16, device=dev)
        lo, hi = torch.zeros(4, dtype=torch.int32, device=dev), torch.full((4,), 4, dtype=torch.int32, device=dev)
        out = torch.full((4, hd), SENT, dtype=bf16, device=dev)
        with pytest.raises(L.UmoeError):
            ops.vision_attn(qkv, lo, hi, 4, 1, hd, 1.0, out)
        same_bits("out of a refused call", out, torch.full_like(out, SENT))


@gpu
@pytest.mark.parametrize("I,ldh,S", SWIGLU_CASES + [SWIGLU_BIG])
def test_swiglu_pair_vs_fp64(dev, I, ldh, S):
    from unimoe_audio_amd import ops
    c, r = make_swiglu(I, ldh, S), ref_swiglu(I, ldh, S)
    st = Stats()
    gu = c["gu"].to(dev)
    h = torch.full((S + 1, ldh), SENT, dtype=bf16, device=dev)
    ops.swiglu_pair(gu, S, I, ldh, h)
    check_cands("h", h[:S], r["h"], r["flag"], st)
    assert bool((bits(h[:S, I:]) == 0).all()), "h: a padding column is not exactly +0"
    same_bits("the row behind the last token", h[S:], torch.full_like(h[S:], SENT))
    _unchanged("gu", gu, c["gu"])
    st.show(f"swiglu_pair I={I} ldh={ldh} S={S}")


@gpu
@pytest.mark.parametrize("n", GELU_N + (GELU_BIG,))
def test_gelu_vs_fp64(dev, n):
    from unimoe_audio_amd import ops
    x = make_gelu(n)
    st = Stats()
    buf = torch.full((n + 8,), SENT, dtype=bf16, device=dev)
    buf[:n] = x.to(dev)
    ops.gelu(buf, n)
    check("gelu", buf[:n], *ref_gelu(x), st)
    same_bits("the elements behind n", buf[n:], torch.full_like(buf[n:], SENT))
    ops.gelu(buf[n:], 0)                                           # n = 0: success, nothing written
    same_bits("the elements behind n", buf[n:], torch.full_like(buf[n:], SENT))
    st.show(f"gelu n={n}")
