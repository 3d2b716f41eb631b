"""The row-wise / per-token kernels of the MoE block's training path (csrc/umoe_bwd.hip) and the token-drop pair
(csrc/umoe_router.hip), each against a float64 restatement on the CPU of the same operation on the same input bits.

Rules of the whole file
  * reference: float64; bf16 / fp32 inputs are upcast exactly; where a kernel's header comment documents a rounding of an
    intermediate to bf16 (silu and dh*u of SwiGLU backward, xh of the RMSNorm weight gradient, the round_t points of the
    bf16 token-drop finisher) the reference rounds its float64 value at the same place;
  * comparison: per element (per row / token where one reduction is shared by a row), never a norm over a tensor;
  * bounds are derived, with u = 2^-24 (fp32 unit roundoff):
      bf16 output                 2^-8 |ref|  (round to nearest: half an ulp <= 2^-8 |ref|)  + (1 + 2^-8) E32
      fp32 output                 E32
      E32                         first-order sum of the fp32 roundings that feed the element: a sum of n terms contributes
                                  n u sum|terms|, an elementwise fp32 operation u |its result|, expf / rsqrtf 2 u (1 ulp)
      flush floor                 2^-126 where a result may flush
    each test's docstring spells its E32 out;
  * rounding-boundary allowance (dw of RMSNorm, du of SwiGLU only): an element whose float64 intermediate lies within relative
    2^-20 of a bf16 rounding midpoint is flagged and gets one bf16 ulp of that intermediate, propagated; at most 1e-3 of the
    elements of a case may be flagged (checked without a GPU for every case the GPU tests run).  The bf16 token-drop finisher has
    five more such rounding points; ref_drop_floats treats them alike, with the fp32 error of the intermediate as the window;
  * untouched memory: output buffers the caller owns are prefilled with a sentinel (bf16 7.0) and whatever the kernel must not
    write keeps it bit for bit.  (ops.permute_bwd, ops.rmsnorm_bwd, ops.aux_loss_bwd, ops.router_bwd and ops.token_drop allocate
    their outputs themselves: every element of those is compared, there is no memory of the caller's to keep.)
Every GPU test prints its worst error / bound under -s ("BWD FP64 ..."); a ratio above 1 fails.

The checkers are tested without a GPU (test_*_cpu): a result emulated in fp32 / bf16 torch arithmetic from the same inputs passes,
and each planted error is rejected.

Measured on an MI355X, worst error / bound over the cases of each test (the whole file: 68 GPU tests in 7 s):
  combine_bwd    dy_slots / dy_shared 0.993 - 0.996 (a bf16 rounding reaches its half ulp), d_mw / d_gs 8e-5 - 1e-4 at D >= 2048, 9e-3 at D = 64
  permute_bwd    dx 0.996
  swiglu_bwd     dg 0.74 - 0.996, du 0.80 - 0.988; flagged share 0 - 6.8e-4 (4.9e-4 at 6240 x 1376)
  rmsnorm_bwd    dh 0.93 - 0.996, dw 0.66 - 0.988; flagged share 0 - 9.4e-4
  aux_loss_bwd   fp32 logits 0.0063, bf16 logits 0.028
  router_bwd     fp32-oracle ratio max|g32 - g64| / N = 0.9e-8 - 2.5e-8 per test; the kernel's own 1.5e-8 - 4.3e-8, i.e. 0.06 - 0.24 of
                 its bound of 16 x the oracle ratio; bf16 "rf": 16 (9/8/2) and 4 (4/4/0) rounds whose mask_for_one differs from the
                 float64 graph's, every one a tie within GATE_TIE
  token_drop     masks exact; fp32 logits routing 0.26, global 0.30, moe 0.13; bf16 logits 0.98 - 0.996, flagged share of the
                 intermediates 5.3e-4 (S = 257), 6.5e-4 (S = 1000), outputs that carry the propagated ulp 1.4e-3 / 7.5e-4
"""
import math

import pytest
import torch

gpu = pytest.mark.gpu

U = 2.0 ** -24          # fp32 unit roundoff
BF = 2.0 ** -8          # bf16: half an ulp relative to the value, at most
TINY = 2.0 ** -126      # flush floor
WINDOW = 2.0 ** -20     # rounding-boundary window (relative)
SENT = 7.0              # sentinel of the bf16 output buffers
f64 = torch.float64
bf16 = torch.bfloat16


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
    return x.to(torch.float32).to(bf16).to(x.dtype)


def ulp_bf16(x):
    """spacing of the bf16 grid at |x| (normal range): |x| = m 2^e, m in [0.5, 1) -> 2^(e - 8)"""
    _, e = torch.frexp(x.abs().to(f64))
    return torch.ldexp(torch.ones_like(x, dtype=f64), e - 8)


def mid_dist(x):
    """distance of x to the nearest bf16 rounding midpoint"""
    ul = ulp_bf16(x)
    t = x.abs().to(f64) / ul
    return (t - torch.floor(t) - 0.5).abs() * ul


def flagged(x, rel=WINDOW):
    return mid_dist(x) <= rel * x.abs()


def bf16_out(ref, e32):
    return BF * ref.abs() + (1 + BF) * e32


class Stats(dict):
    def note(self, name, v):
        self[name] = max(self.get(name, 0.0), float(v))

    def show(self, title):
        print(f"\nBWD FP64 {title}: " + ", ".join(f"{k} {v:.3g}" for k, v in self.items()))


def check(name, got, ref, bound, stats):
    """|got - ref| <= bound per element; ref non-finite: got must be NaN exactly there."""
    got = got.detach().cpu().to(f64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), f"{name}: NaN pattern differs"
    assert bool(torch.isfinite(got[~nan]).all()), f"{name}: non-finite value"
    err = (got - ref).abs()[~nan]
    b = bound[~nan]
    ratio = torch.where(b > 0, err / b, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    stats.note(name, worst)
    if not worst <= 1.0:
        i = int(ratio.argmax())
        raise AssertionError(f"{name}: error / bound = {worst:.4g} (error {float(err[i]):.4g}, bound {float(b[i]):.4g}, flat index {i} of the finite elements)")


def keeps_sentinel(name, t, what=SENT):
    t = t.detach().cpu()
    assert torch.equal(t.contiguous().view(torch.int16), torch.full_like(t, what).contiguous().view(torch.int16)), f"{name}: sentinel overwritten"


def r8(n):
    return (n + 7) & ~7


# ------------------------------------------------------------------------------------------------ combine / permute backward
GEOMS = [(2048, 8, 9, 2, True), (64, 8, 9, 2, True), (2056, 8, 9, 2, True), (2048, 12, 12, 4, True), (2048, 13, 13, 2, True),
         (2048, 8, 9, 0, True), (2048, 8, 9, 2, False)]           # D, n_real, n_dyn, n_fix, y_shared given
S_MODES = [(1, "all"), (1, "none"), (257, "mixed")]


def make_combine(S, mode, D, n_real, n_dyn, n_fix, seed):
    g = gen(seed)
    sel = torch.rand(S, n_real, generator=g) < 0.5
    if mode == "all":
        sel[:] = True
    elif mode == "none":
        sel[:] = False
    else:
        sel[0] = False           # a token that selected nothing
        sel[1] = True            # a token that selected every expert
        sel[S - 1] = False
        sel[S - 2] = True
    slot_of = torch.full((S, n_real), -1, dtype=torch.int64)
    off = 8                       # rows 0..7 belong to nobody (the kernels read row 0 for an unselected expert, never write it)
    for e in range(n_real):
        rows = torch.nonzero(sel[:, e]).flatten()
        slot_of[rows, e] = off + torch.arange(rows.numel())
        off = r8(off + rows.numel()) + 8          # pad rows up to a multiple of 8 and one spare block: rows no token references
    cap = off
    E = n_dyn + n_fix
    c = dict(S=S, D=D, n_real=n_real, n_dyn=n_dyn, n_fix=n_fix, sel=sel, slot_of=slot_of, cap=cap,
             y=torch.randn(cap, D, generator=g).to(bf16), ysh=torch.randn(max(1, n_fix) * S, D, generator=g).to(bf16),
             w=torch.rand(S, n_real, generator=g) + 0.05, gw=torch.rand(S, E, generator=g) + 0.05,
             dout=torch.randn(S, D, generator=g).to(bf16),
             dxe=torch.randn(cap, D, generator=g).to(bf16), dxsh=torch.randn(max(1, n_fix) * S, D, generator=g).to(bf16),
             extra=torch.randn(S, D, generator=g).to(bf16))
    return c


def ref_combine(c, shared):
    """dy[slot(s,e)] = bf16(w[s][e] * dout[s])      E32 = u |ref|                    (one fp32 product)
       d_mw[s][e]    = sum_D dout[s] * y[slot]      E32 = D u sum|dout * y|          (bf16 x bf16 products are exact in fp32)
       the shared experts alike with gw[s][n_dyn + i] and row i S + s."""
    S, D, n_real, n_dyn, n_fix = c["S"], c["D"], c["n_real"], c["n_dyn"], c["n_fix"]
    d, y, w = c["dout"].to(f64), c["y"].to(f64), c["w"].to(f64)
    dy = torch.zeros(c["cap"], D, dtype=f64)
    used = torch.zeros(c["cap"], dtype=torch.bool)
    mw, mw_abs = torch.zeros(S, n_real, dtype=f64), torch.zeros(S, n_real, dtype=f64)
    for e in range(n_real):
        rows = torch.nonzero(c["sel"][:, e]).flatten()
        sl = c["slot_of"][rows, e]
        dy[sl] = w[rows, e, None] * d[rows]
        used[sl] = True
        mw[rows, e] = (d[rows] * y[sl]).sum(-1)
        mw_abs[rows, e] = (d[rows] * y[sl]).abs().sum(-1)
    r = dict(dy=dy, used=used, mw=mw, b_dy=bf16_out(dy, U * dy.abs()), b_mw=D * U * mw_abs)
    if shared and n_fix:
        ysh, g = c["ysh"].to(f64).view(n_fix, S, D), c["gw"].to(f64)[:, n_dyn:]
        r["dysh"] = (g.t()[:, :, None] * d[None]).reshape(n_fix * S, D)
        r["b_dysh"] = bf16_out(r["dysh"], U * r["dysh"].abs())
        r["gs"] = (d[None] * ysh).sum(-1).t().contiguous()
        r["b_gs"] = D * U * (d[None] * ysh).abs().sum(-1).t().contiguous()
    return r


def emu_combine(c, shared):
    S, D, n_fix, n_dyn = c["S"], c["D"], c["n_fix"], c["n_dyn"]
    d = c["dout"].float()
    dy = torch.full((c["cap"], D), SENT, dtype=bf16)
    dysh = torch.full((max(1, n_fix) * S, D), SENT, dtype=bf16)
    mw = torch.zeros(S, c["n_real"])
    for e in range(c["n_real"]):
        rows = torch.nonzero(c["sel"][:, e]).flatten()
        sl = c["slot_of"][rows, e]
        dy[sl] = (c["w"][rows, e, None] * d[rows]).to(bf16)
        mw[rows, e] = (d[rows] * c["y"].float()[sl]).sum(-1)
    gs = None
    if shared and n_fix:
        dysh = (c["gw"][:, n_dyn:].t()[:, :, None] * d[None]).reshape(n_fix * S, D).to(bf16)
        gs = (d[None] * c["ysh"].float().view(n_fix, S, D)).sum(-1).t().contiguous()
    return dy, dysh, mw, gs


def check_combine(c, r, shared, dy, dysh, mw, gs, stats):
    used = r["used"]
    check("dy_slots", dy.cpu()[used], r["dy"][used], r["b_dy"][used], stats)
    keeps_sentinel("dy_slots rows no token references", dy.cpu()[~used])
    check("d_mw", mw, r["mw"], r["b_mw"], stats)
    assert bool((mw.cpu()[~c["sel"]] == 0).all()), "d_mw: non-zero entry for an expert the token did not select"
    if shared and c["n_fix"]:
        check("dy_shared", dysh, r["dysh"], r["b_dysh"], stats)
        check("d_gs", gs, r["gs"], r["b_gs"], stats)
    else:
        keeps_sentinel("dy_shared without shared experts", dysh)


def ref_permute(c, with_extra):
    """dx[s] = bf16(sum of the token's slot rows + its shared rows + extra[s]), n bf16 terms added in fp32: E32 = n u sum|terms|."""
    S, D, n_fix = c["S"], c["D"], c["n_fix"]
    x = c["dxe"].to(f64)
    ref, ab, n = torch.zeros(S, D, dtype=f64), torch.zeros(S, D, dtype=f64), torch.zeros(S, 1, dtype=f64)
    for e in range(c["n_real"]):
        rows = torch.nonzero(c["sel"][:, e]).flatten()
        t = x[c["slot_of"][rows, e]]
        ref[rows] += t
        ab[rows] += t.abs()
        n[rows] += 1
    for i in range(n_fix):
        t = c["dxsh"].to(f64)[i * S:(i + 1) * S]
        ref, ab, n = ref + t, ab + t.abs(), n + 1
    if with_extra:
        t = c["extra"].to(f64)
        ref, ab, n = ref + t, ab + t.abs(), n + 1
    return dict(dx=ref, b_dx=bf16_out(ref, n * U * ab))


def emu_permute(c, with_extra):
    S, n_fix = c["S"], c["n_fix"]
    acc = torch.zeros(S, c["D"])
    for e in range(c["n_real"]):
        rows = torch.nonzero(c["sel"][:, e]).flatten()
        acc[rows] += c["dxe"].float()[c["slot_of"][rows, e]]
    for i in range(n_fix):
        acc += c["dxsh"].float()[i * S:(i + 1) * S]
    if with_extra:
        acc += c["extra"].float()
    return acc.to(bf16)


def check_permute(c, r, with_extra, dx, stats):
    check("dx", dx, r["dx"], r["b_dx"], stats)
    if c["n_fix"] == 0:          # a token without a slot: exactly `extra`, or zeros
        lone = ~c["sel"].any(-1)
        want = c["extra"][lone] if with_extra else torch.zeros_like(c["extra"][lone])
        assert torch.equal(dx.cpu()[lone].view(torch.int16), want.view(torch.int16)), "dx: a token without a slot is not exactly extra / zero"


def _combine_seed(D, n_real, n_fix, S, mode):
    return 1000 + D + 7 * n_real + 3 * n_fix + S + len(mode)


# ------------------------------------------------------------------------------------------------ SwiGLU backward
SPECIAL_G = [0.0, -0.0, 30.0, -30.0, 100.0, -100.0]
SWIGLU_CASES = [(I, rows) for I in (8, 96, 1376) for rows in (1, 77)]
SWIGLU_BIG = (1376, 6240)                     # rows * I / 8 > 4096 * 256: the grid-stride loop


def make_swiglu(I, rows, seed):
    g = gen(seed)
    gu = torch.randn(rows, 2 * I, generator=g).to(bf16)            # (scale 1: the bf16 values whose silu sits on a rounding midpoint -- -3.046875, 0.2236328125, 4.03125 ... -- stay under 1e-3 of the elements)
    gu[0, :len(SPECIAL_G)] = torch.tensor(SPECIAL_G).to(bf16)
    if rows > 1:
        gu[rows - 1, I - len(SPECIAL_G):I] = torch.tensor(SPECIAL_G).to(bf16)
    dh = torch.randn(rows, I, generator=g).to(bf16)
    return dict(I=I, rows=rows, gu=gu, dh=dh)


def ref_swiglu(c):
    """sg = 1 / (1 + expf(-g)), silu = rbf(g sg), du = bf16(dh silu), ds = rbf(dh u) (exact product: the same in fp32 and float64),
    dg = bf16(ds f), f = sg (1 + g (1 - sg)).  fp32 roundings, first order, delta(sg) <= 4 u sg (expf 2 u, add, divide):
      du: E32 = u |du|                                              (silu is rounded to bf16 in both; flagged elements below)
      dg: E32 = u |ds| sg (|g| (4 sg + (1 - sg)) + |g (1 - sg)| + 6 |1 + g (1 - sg)|) + u |dg|
          -- 1 - sg carries 4 u sg + u (1 - sg), times |g|; the product g (1 - sg) and the sum 1 + . one rounding each; sg . carries
          4 u of sg and one rounding; the last product one rounding.
    floor 2^-126 on both: at g = -100 expf overflows, sg and silu become 0 where float64 has 4e-44 and -4e-42.
    flagged (du only): float64 g sg within relative 2^-20 of a bf16 midpoint -> + |dh| ulp_bf16(silu)."""
    I = c["I"]
    g, u, d = c["gu"][:, :I].to(f64), c["gu"][:, I:].to(f64), c["dh"].to(f64)
    sg = torch.sigmoid(g)
    one_m = torch.where(g > 0, torch.exp(-g) / (1 + torch.exp(-g)), 1 - sg)        # 1 - sg without cancellation
    raw = g * sg
    silu = rbf(raw)
    du = d * silu
    ds = rbf(d * u)
    t = g * one_m
    p = 1 + t
    dg = ds * sg * p
    flag = flagged(raw)
    e_du = U * du.abs() + flag * d.abs() * ulp_bf16(raw)
    e_dg = U * ds.abs() * sg * (g.abs() * (4 * sg + one_m) + t.abs() + 6 * p.abs()) + U * dg.abs()
    return dict(dg=dg, du=du, b_dg=bf16_out(dg, e_dg) + TINY, b_du=bf16_out(du, e_du) + TINY, share=float(flag.double().mean()))


def emu_swiglu(c):
    I = c["I"]
    g, u, d = c["gu"][:, :I].float(), c["gu"][:, I:].float(), c["dh"].float()
    sg = 1.0 / (1.0 + torch.exp(-g))
    silu = rbf(g * sg)
    ds = rbf(d * u)
    return torch.cat([(ds * (sg * (1.0 + g * (1.0 - sg)))).to(bf16), (d * silu).to(bf16)], -1)


def check_swiglu(c, r, dgu, total, stats):
    """dgu [max_rows][2I] (already cut out of its wider buffer); rows >= total keep the sentinel"""
    I = c["I"]
    out = dgu.cpu()
    check("dg", out[:total, :I], r["dg"][:total], r["b_dg"][:total], stats)
    check("du", out[:total, I:], r["du"][:total], r["b_du"][:total], stats)
    keeps_sentinel("dgu rows at and beyond total_rows", out[total:])


# ------------------------------------------------------------------------------------------------ RMSNorm backward
RMS_D = (8, 256, 2048, 2056, 4096, 8192)
RMS_S = (1, 3, 13, 16, 17, 511, 512, 513, 1030)
RMS_CASES = sorted({(D, S) for D in RMS_D for S in (17, 513)} | {(D, S) for D in (256, 2048) for S in RMS_S})
RMS_EPS = 1e-6


def make_rms(D, S, seed):
    g = gen(seed)
    h = torch.randn(S, D, generator=g).to(bf16)
    w = (1 + 0.1 * torch.randn(D, generator=g)).to(bf16)
    dy = (0.5 * h.float() + torch.randn(S, D, generator=g)).to(bf16)          # correlated with h: mean(gy xh) is not noise
    dsum = torch.randn(S, D, generator=g).to(bf16)
    return dict(D=D, S=S, h=h, w=w, dy=dy, dsum=dsum)


def rms_parts(S):
    n_wg = min(S, 512)
    rpw = -(-S // n_wg)
    return rpw, -(-S // rpw)


def ref_rms(c, with_dsum):
    """rs = rsqrtf(sum h^2 / D + eps), xh = h rs, gy = dy w (exact), m = sum(gy xh) / D, dh = bf16(rs (gy - xh m) + dsum),
    dw[c] = bf16(sum_s dy rbf(xh)).  First order, per row:
      rho   = delta(rs) / rs <= ((D + 2) / 2 + 2) u           (D-term sum of squares, divide, add eps; half of it through the root; rsqrtf 2 u)
      dmean = ((D + 3) u + rho) sum|gy xh| / D                (every term carries two roundings and rho; the D-term sum; the divide)
      dh: E32 = rs (|xh| dmean + |xh m| (rho + 2 u)) + (rho + 2 u) |rs (gy - xh m)| + u |dh|
      dw: E32 = S u sum_s |dy rbf(xh)|                        (bf16 x bf16 products exact; S terms over the row loop and the column sum)
    flagged (dw only): float64 xh within relative 2^-20 of a bf16 midpoint -> + |dy| ulp_bf16(xh) on its column."""
    D, S = c["D"], c["S"]
    h, w, dy = c["h"].to(f64), c["w"].to(f64), c["dy"].to(f64)
    rs = (h.pow(2).mean(-1, keepdim=True) + RMS_EPS).rsqrt()
    xh, gy = h * rs, dy * w
    m = (gy * xh).mean(-1, keepdim=True)
    core = rs * (gy - xh * m)
    dh = core + (c["dsum"].to(f64) if with_dsum else 0)
    rho = ((D + 2) / 2 + 2) * U
    dmean = ((D + 3) * U + rho) * (gy * xh).abs().mean(-1, keepdim=True)
    e_dh = rs * (xh.abs() * dmean + (xh * m).abs() * (rho + 2 * U)) + (rho + 2 * U) * core.abs() + U * dh.abs()
    xr = rbf(xh)
    flag = flagged(xh)
    dw = (dy * xr).sum(0)
    e_dw = S * U * (dy * xr).abs().sum(0) + (flag * dy.abs() * ulp_bf16(xh)).sum(0)
    return dict(dh=dh, dw=dw, b_dh=bf16_out(dh, e_dh), b_dw=bf16_out(dw, e_dw), share=float(flag.double().mean()))


def emu_rms(c, with_dsum, ss_div=None, mean_div=None, drop_part=None):
    D, S = c["D"], c["S"]
    h, w, dy = c["h"].float(), c["w"].float(), c["dy"].float()
    rs = torch.rsqrt(h.pow(2).sum(-1, keepdim=True) / float(ss_div or D) + RMS_EPS)
    xh, gy = h * rs, dy * w
    mean = (gy * xh).sum(-1, keepdim=True) / float(mean_div or D)
    o = rs * (gy - xh * mean)
    if with_dsum:
        o = o + c["dsum"].float()
    rpw, used = rms_parts(S)
    terms = dy * rbf(xh)
    parts = torch.stack([terms[p * rpw:(p + 1) * rpw].sum(0) for p in range(used)])
    if drop_part is not None:
        parts[drop_part] = 0
    return o.to(bf16), parts.sum(0).to(bf16)


def check_rms(c, r, dh, dw, stats):
    check("dh", dh, r["dh"], r["b_dh"], stats)
    check("dw", dw, r["dw"], r["b_dw"], stats)


# ------------------------------------------------------------------------------------------------ aux loss backward
def make_aux(S, dt, n_dyn, n_fix, seed):
    g = gen(seed)
    E = n_dyn + n_fix
    logits = (torch.randn(S, E, generator=g) * 1.2).to(dt)
    mask = (torch.rand(S, E, generator=g) < 0.45).to(torch.int32)
    mask[:, n_dyn:] = 1
    mask[:, 5] = 0                       # a column that no token selected
    if S > 2:
        mask[2, :n_dyn] = 0              # a token whose dynamic columns are all masked: the finfo-min fill path
    else:
        mask[0, 0] = 1
    tokw = torch.rand(S, generator=g) + 0.1
    return dict(S=S, n_dyn=n_dyn, E=E, logits=logits, mask=mask, tokw=tokw, d_aux=0.7)


def aux_graph(z, mask, n_dyn, tokw, lowest):
    """oracle.dcmoe_autograd.aux_loss with the fill value as a parameter (the oracle takes finfo.min of the logits' dtype, which is
    float64's here); test_aux_cpu checks that the two agree"""
    prob = torch.softmax(z.masked_fill(mask == 0, lowest)[:, :n_dyn], dim=-1)
    m = mask[:, :n_dyn].to(z.dtype)
    if tokw is None:
        return (m.mean(0) * prob.mean(0)).sum() * n_dyn
    w = tokw.to(z.dtype).reshape(-1, 1)
    return ((m * w).sum(0) / w.sum(0) * ((prob * w).sum(0) / w.sum(0))).sum() * n_dyn


def ref_aux(c, with_w):
    """out[s][e] = scale p_e (f_e - fdot) on kept dynamic columns, 0 elsewhere; scale = d_aux n_dyn w_s / W, f_e = sum_s w mask / W,
    p = softmax over the n_dyn filled logits, fdot = sum_a f_a p_a.  First order, n = n_dyn:
      f_e    relative (2 S + 1) u        (two S-term sums of non-negative terms, one divide)
      p_e    relative tau_s = (2 (2 + max_a |x_a - max|) + n + 2) u      (x - max carries u |x - max| into the exponent, expf 2 u, for the
                                                                         element and for the denominator; the n-term sum; the divide)
      fdot   relative (2 S + 2 + n) u + tau_s    (non-negative terms)
      scale  relative (S + 6) u
      E32 = |scale| p_e ((2 S + 1) u f_e + fdot ((2 S + 2 + n) u + tau_s) + |f_e - fdot| (tau_s + (S + 7) u)),  floor 2^-126."""
    S, n, E = c["S"], c["n_dyn"], c["E"]
    dt = c["logits"].dtype
    lowest = torch.finfo(dt).min
    z = c["logits"].to(f64).requires_grad_(True)
    tokw = c["tokw"] if with_w else None
    (c["d_aux"] * aux_graph(z, c["mask"], n, tokw, lowest)).backward()
    w = (c["tokw"] if with_w else torch.ones(S)).to(f64)
    W = w.sum()
    m = c["mask"][:, :n].to(f64)
    f = (m * w[:, None]).sum(0) / W
    x = c["logits"].to(f64)[:, :n].masked_fill(m == 0, lowest)
    span = (x - x.max(-1, keepdim=True)[0]).abs()
    span = torch.where(m != 0, span, torch.zeros_like(span)).max(-1, keepdim=True)[0]
    p = torch.softmax(x, -1)
    fdot = (f * p).sum(-1, keepdim=True)
    tau = (2 * (2 + span) + n + 2) * U
    scale = (c["d_aux"] * n * w / W).abs()[:, None]
    e = scale * p * ((2 * S + 1) * U * f + fdot * ((2 * S + 2 + n) * U + tau) + (f - fdot).abs() * (tau + (S + 7) * U))
    bound = torch.zeros(S, E, dtype=f64)
    bound[:, :n] = (e + TINY) * m                   # exactly zero wherever the column did not keep its logit
    return dict(g=z.grad, bound=bound)


def emu_aux(c, with_w):
    z = c["logits"].float().clone().requires_grad_(True)
    (c["d_aux"] * aux_graph(z, c["mask"], c["n_dyn"], c["tokw"] if with_w else None, torch.finfo(c["logits"].dtype).min)).backward()
    return z.grad


# ------------------------------------------------------------------------------------------------ router backward
ROUTER_GEOMS = [(9, 8, 2), (4, 4, 0)]
ROUTER_S = (1, 255, 256, 257, 1030)
TOP_P, JIT = 0.9, 0.01


def make_router(S, dt, n_dyn, n_real, n_fix, seed, with_in):
    g = gen(seed)
    E = n_dyn + n_fix
    logits = torch.randn(S, E, generator=g) * 1.2
    if S > 40:
        logits[30, :n_dyn] = 0.25           # all equal: the Top-P count reaches n_dyn
        logits[31, :n_dyn] = -1.0
    logits = logits.to(dt)
    am = torch.ones(S, dtype=torch.bool)
    if S > 40:
        am[:17] = False                      # padded tokens
    return dict(S=S, n_dyn=n_dyn, n_real=n_real, n_fix=n_fix, E=E, logits=logits, am=am,
                d_mw=torch.randn(S, n_real, generator=g), d_gs=torch.randn(S, max(1, n_fix), generator=g)[:, :n_fix].contiguous(),
                d_in=torch.randn(S, E, generator=g) if with_in else None,
                gumbel=-torch.log(-torch.log(torch.rand(S, n_dyn, n_dyn, generator=g).clamp(1e-6, 1 - 1e-6))),
                rand_u=torch.rand(S, n_dyn, generator=g))


def argmax_rounds(dyn, k):
    """selection order of the eval branch: round j takes the largest logit not yet taken, lowest index among equals"""
    S, n = dyn.shape
    order = torch.full((S, n), -1, dtype=torch.int32)
    taken = torch.zeros((S, n), dtype=torch.bool)
    for j in range(int(k.max()) if S else 0):
        _, idx = dyn.masked_fill(taken, float("-inf")).max(-1, keepdim=True)       # torch.max: first maximal index
        live = k > j
        order[:, j] = torch.where(live, idx.squeeze(-1).to(torch.int32), order[:, j])
        taken |= torch.zeros((S, n), dtype=torch.bool).scatter(1, idx, True) & live[:, None]
    return order


def rounds_train(dyn, k, eps, gumbel, rand, factor):
    """oracle.dcmoe_autograd.routing_weights_train, restated so that mask_for_one can be GIVEN (factor [S, n_dyn], the kernel's
    round_factor): it is a decision -- "is the selected column the arg-max of the softmaxed gates" -- that the forward takes on
    gates of the logits' dtype; bf16 gates tie where float64 gates do not.  -> (weights, mask, order, the graph's own
    mask_for_one, margin of that decision per round: |gate_selected - largest other gate| / gate_max)"""
    from oracle.dcmoe_autograd import _RoutingFn
    S, n = dyn.shape
    taken = torch.zeros((S, n), dtype=torch.bool)
    w = torch.zeros_like(dyn)
    order = torch.full((S, n), -1, dtype=torch.int32)
    own = torch.ones((S, n), dtype=dyn.dtype)
    margin = torch.ones((S, n), dtype=dyn.dtype)
    for j in range(int(k.max()) if S else 0):
        live = (k > j).unsqueeze(-1)
        masked = dyn.masked_fill(taken, float("-inf"))
        with torch.no_grad():
            mx, _ = masked.max(dim=-1, keepdim=True)
            far = ((mx - dyn) / dyn.abs().clamp(min=mx.abs())) > (2 * eps)
        gates = masked.masked_fill(far, float("-inf"))
        sel = (gates + gumbel[:, j]).max(dim=-1)[1].unsqueeze(-1)
        gates = torch.softmax(gates, dim=-1)
        mo = gates.gather(dim=-1, index=sel)
        gm, mi = gates.max(dim=-1, keepdim=True)
        one = torch.add(0.3333, torch.logical_or(sel == mi, rand[:, j:j + 1] > 0.75), alpha=0.6667).type_as(gates)
        own[:, j] = torch.where(live, one, own[:, j:j + 1]).squeeze(-1).detach()
        rival = gates.detach().scatter(1, sel, -1.0).max(dim=-1, keepdim=True)[0]
        margin[:, j] = ((mo - rival).abs() / gm).squeeze(-1).detach()
        mult = _RoutingFn.apply(dyn, mo, sel, gates, factor[:, j:j + 1].to(dyn.dtype))
        pick = torch.zeros((S, n), dtype=torch.bool).scatter(1, sel, True) & live
        w = w + torch.where(pick, torch.zeros_like(w).scatter(1, sel, mult), torch.zeros_like(w))
        order[:, j] = torch.where(live.squeeze(-1), sel.squeeze(-1).to(torch.int32), order[:, j])
        taken = taken | pick
    return w, taken.to(torch.int32), order, own, margin


GATE_TIE = 2.0 ** -7 + 2.0 ** -20


def factor_agrees(c, fac, k, dt):
    """mask_for_one of the forward (fac, its round_factor) against the float64 graph's own (c["own_factor"], c["gate_margin"] of the
    router_graph call just made) on every live round.  fp32 logits: equal.  bf16 logits: the forward rounds each softmaxed gate once
    to bf16; rounding to nearest keeps a > b apart whenever a - b > ulp(a), and ulp(a) <= 2^-7 a <= 2^-7 gate_max; the fp32 softmax
    ahead of the rounding moves a gate by less than 2^-20 relative.  So the two may differ only on a round whose margin
    |gate_selected - largest other gate| / gate_max is at most GATE_TIE = 2^-7 + 2^-20: a tie that bf16 cannot resolve.
    -> the number of such rounds"""
    live = torch.arange(c["n_dyn"])[None] < k[:, None]
    differ = ((c["own_factor"].to(f64) - fac.to(f64)).abs() > 1e-2) & live          # the factor is 1 or 0.3333 (0.333 in bf16)
    if dt != bf16:
        assert not bool(differ.any()), "mask_for_one of the forward and of the float64 graph differ"
    worst = float(c["gate_margin"][differ].max()) if bool(differ.any()) else 0.0
    assert worst <= GATE_TIE, f"mask_for_one of the forward and of the float64 graph differ on a round with gate margin {worst:.4g}"
    return int(differ.sum())


def drop_cap(mask, n_dyn):
    """a capacity that drops about a third of the selections"""
    return int(0.67 * float(mask[:, :n_dyn].sum(0).float().mean()))


def router_post_mask(c, mask):
    from oracle.dcmoe import drop_keep_mask
    post = drop_keep_mask(c["logits"], mask, c["n_dyn"], drop_cap(mask, c["n_dyn"]), "probs")
    if c["S"] > 40:
        post[20, :c["n_dyn"]] = 0           # a live token that loses every dynamic column to the drop
    return post


def router_graph(c, form, k, post, dtype, factor=None):
    """-> (d logits, selection order, pre-drop mask) of the routing graph in `dtype` (float64: the reference; float32: the yardstick)
    plain: oracle.dcmoe_autograd.routing_weights + the lines of oracle.dcmoe_autograd.forward that follow it;
    drop:  the same with the post-drop mask and r2 = q / (sum q + 1e-6), q = r * mask_after_drop (core.py:328-329);
    rf:    oracle.dcmoe_autograd.routing_weights_train with the noise as input (its backward ignores mask_for_one), restated in
           rounds_train."""
    from oracle import dcmoe_autograd as OA
    n_dyn, n_real, n_fix = c["n_dyn"], c["n_real"], c["n_fix"]
    z = c["logits"].to(dtype).clone().requires_grad_(True)
    dyn = z[:, :n_dyn]
    if form == "rf":
        rw, picked, order, own, margin = rounds_train(dyn, k, JIT, c["gumbel"].to(dtype), c["rand_u"], factor)
        c["own_factor"], c["gate_margin"] = own, margin
    else:
        rw, picked = OA.routing_weights(dyn, k, JIT, None)
        order = argmax_rounds(dyn.detach(), k)
    mask = torch.cat([picked * c["am"][:, None].int(), torch.zeros((c["S"], n_fix), dtype=torch.int32)], -1)
    if n_fix:
        mask[:, n_dyn:] = 1
    rw = rw / (rw.sum(-1, keepdim=True) + 1e-6)
    m = mask
    if form == "drop":
        m = post
        rw = rw.masked_fill(m[:, :n_dyn] == 0, 0.0)
        rw = rw / (rw.sum(-1, keepdim=True) + 1e-6)
    if n_fix:
        G = torch.softmax(z.masked_fill(m == 0, float("-inf")), dim=-1)
        gw = torch.cat([rw * G[:, :n_dyn].sum(-1, keepdim=True), G[:, n_dyn:]], -1)
    else:
        gw = rw
    loss = (gw[:, :n_real] * m[:, :n_real] * c["d_mw"].to(dtype)).sum()
    if n_fix:
        loss = loss + (gw[:, n_dyn:] * c["d_gs"].to(dtype)).sum()
    if c["d_in"] is not None:
        loss = loss + (z * c["d_in"].to(dtype)).sum()
    loss.backward()
    return z.grad, order, mask


def router_norm(c):
    n = c["d_mw"].to(f64).abs().sum(-1) + c["d_gs"].to(f64).abs().sum(-1)
    if c["d_in"] is not None:
        n = n + c["d_in"].to(f64).abs().max(-1)[0]
    return n


def token_ratio(g, g64, norm):
    return (g.to(f64) - g64).abs().max(-1)[0] / norm


# ------------------------------------------------------------------------------------------------ token drop
DROP_S = (1, 255, 256, 257, 1000, 6240)
DROP_GEOM = (9, 8, 2)


def drop_key_bits(logits):
    """the kernel's order-preserving integer image of a logit (larger logit = larger key), -0.0 and +0.0 sharing one key"""
    if logits.dtype == bf16:
        u = logits.contiguous().view(torch.int16).to(torch.int64) & 0xffff
        u = torch.where(u == 0x8000, torch.zeros_like(u), u)
        return torch.where((u & 0x8000) != 0, ~u & 0xffff, u | 0x8000)
    u = logits.contiguous().view(torch.int32).to(torch.int64) & 0xffffffff
    u = torch.where(u == 0x80000000, torch.zeros_like(u), u)
    return torch.where((u & 0x80000000) != 0, ~u & 0xffffffff, u | 0x80000000)


def emu_drop_mask(logits, mask, n_dyn, cap, policy, keys=None, higher_index_wins=False):
    """the selection the kernel makes, restated on its integer keys (not on float comparisons)"""
    S, E = mask.shape
    out = mask.clone()
    keys = drop_key_bits(logits) if keys is None else keys
    for e in range(E):
        sel = torch.nonzero(mask[:, e]).flatten()
        if policy == "position":
            out[sel[cap:], e] = 0
            continue
        if e >= n_dyn or sel.numel() <= min(cap, S):
            continue
        idx = sel if not higher_index_wins else -sel
        order = sorted(range(sel.numel()), key=lambda i: (-int(keys[sel[i], e]), int(idx[i])))
        out[sel[torch.tensor(order[min(cap, S):], dtype=torch.int64)], e] = 0
    return out


def check_drop_mask(got, logits, mask, n_dyn, cap, policy):
    from oracle.dcmoe import drop_keep_mask
    want = drop_keep_mask(logits, mask, n_dyn, cap, policy)
    got = got.cpu()
    if not torch.equal(got, want):
        bad = torch.nonzero((got != want).any(0)).flatten().tolist()
        tok = torch.nonzero((got != want).any(1)).flatten().tolist()
        raise AssertionError(f"token drop ({policy}, capacity {cap}): mask differs in columns {bad}, tokens {tok[:12]}")
    return want


def make_drop(S, dt, seed):
    n_dyn, n_real, n_fix = DROP_GEOM
    g = gen(seed)
    E = n_dyn + n_fix
    logits = (torch.randn(S, E, generator=g) * 1.2).to(dt)
    dens = torch.tensor([0.15 + 0.07 * e for e in range(n_dyn)])
    mask = (torch.rand(S, E, generator=g)[:, :] < torch.cat([dens, torch.ones(n_fix)])).to(torch.int32)
    mask[:, n_dyn:] = 1
    mask[0, 0] = 1
    rw = torch.rand(S, n_dyn, generator=g) + 0.01
    return dict(S=S, logits=logits, mask=mask, rw=rw)


def drop_caps(c):
    from unimoe_audio_amd import ops
    n_dyn = DROP_GEOM[0]
    cnt = c["mask"][:, :n_dyn].sum(0)
    lo, hi = int(cnt.min()), int(cnt.max())
    return sorted({0, 1, max(lo - 1, 0), (lo + hi) // 2, c["S"] + 3, ops.expert_capacity(c["S"], n_dyn, 6.0, 8)})


def make_drop_ties(S, dt, seed):
    """hand-built columns (capacity CAP = S // 3):
      0  every selected logit equal
      1  CAP - 3 logits above a value shared by 10 tokens that lie in different threads' token ranges, the rest below
      2  the shared value 2^127: key byte 255 in the highest radix pass, 0 in the lowest (bf16 0x7f00, fp32 0x7f000000)
      3  negative logits with a shared value
      4  +0.0 and -0.0 at the boundary, the -0.0 at the lower token index"""
    c = make_drop(S, dt, seed)
    n_dyn = DROP_GEOM[0]
    cap = S // 3
    g = gen(seed + 1)
    L, M = c["logits"].float(), c["mask"]
    M[:, :5] = 1
    M[5::7, :5] = 0
    sel = torch.nonzero(M[:, 0]).flatten()
    assert sel.numel() > cap + 20

    def place(col, tie_val, above, n_tie, below):
        perm = sel[torch.randperm(sel.numel(), generator=g)]
        step = sel.numel() // n_tie
        ties = sel[torch.arange(n_tie) * step + 1]                  # spread over the whole token range
        rest = perm[~torch.isin(perm, ties)]
        L[rest[:cap - 3], col] = above(cap - 3)
        L[rest[cap - 3:], col] = below(rest.numel() - (cap - 3))
        L[ties, col] = tie_val
        return ties

    L[:, 0] = 0.5
    place(1, 0.75, lambda n: 1.0 + torch.rand(n, generator=g), 10, lambda n: -torch.rand(n, generator=g))
    place(2, 2.0 ** 127, lambda n: torch.full((n,), 2.0 ** 127 * 1.5), 10, lambda n: torch.rand(n, generator=g))
    place(3, -1.5, lambda n: -1.0 + 0.25 * torch.rand(n, generator=g), 10, lambda n: -2.0 - torch.rand(n, generator=g))
    ties = place(4, 0.0, lambda n: 0.5 + torch.rand(n, generator=g), 10, lambda n: -0.5 - torch.rand(n, generator=g))
    L[ties[0::2], 4] = -0.0                                           # -0.0 at the lowest index, then alternating
    c["logits"] = L.to(dt)                                            # (the shared values are exact in bf16; rounding the others keeps their side)
    c["cap"], c["zero_ties"] = cap, ties
    return c


def other_bf16(x):
    """the bf16 neighbour of x on the far side of the rounding midpoint next to x"""
    r = rbf(x)
    return r + torch.sign(x - r) * ulp_bf16(x)


def drop_chain(c, post, flip=None):
    """the finisher's chain in float64 with its bf16 rounding points (bf16 logits; none with fp32 logits).  flip = (stage, [bool]):
    at that rounding point the marked intermediates take their other bf16 neighbour.  -> unrounded last-step values, intermediates,
    first-order fp32 errors"""
    n_dyn, n_real, n_fix = DROP_GEOM
    E = n_dyn + n_fix
    is_bf = c["logits"].dtype == bf16

    def rnd(stage, t):
        if not is_bf:
            return t
        if flip is not None and flip[0] == stage:
            return torch.where(flip[1], other_bf16(t), rbf(t))
        return rbf(t)

    md = post[:, :n_dyn] != 0
    q = c["rw"].to(f64) * md
    ssum = q.sum(-1, keepdim=True)
    e_sum = n_dyn * U * ssum
    den_raw = rnd("sum", ssum) + float(torch.tensor(1e-6, dtype=torch.float32))
    r_raw = q / rnd("den", den_raw)
    e_r = (U if is_bf else (n_dyn + 3) * U) * r_raw
    r = rnd("r", r_raw)
    x = c["logits"].to(f64).masked_fill(post == 0, float("-inf"))
    G_raw = torch.softmax(x, -1)
    fin = torch.where(post != 0, (x - x.max(-1, keepdim=True)[0]).abs(), torch.zeros_like(x))
    fin = torch.nan_to_num(fin, nan=0.0, posinf=0.0)
    tau = (fin + 2 + (G_raw * (fin + 2)).sum(-1, keepdim=True) + E + 3) * U
    e_G = torch.nan_to_num(tau * G_raw, nan=0.0)
    G = rnd("G", G_raw)
    gd_raw = G[:, :n_dyn].sum(-1, keepdim=True)
    e_gd = (0 if is_bf else e_G[:, :n_dyn].sum(-1, keepdim=True)) + n_dyn * U * gd_raw
    if is_bf:       # a sum of a few bf16 values is usually exact in fp32 (and then often exactly ON a midpoint, where both round to even)
        s32 = G[:, 0].float()
        for j in range(1, n_dyn):
            s32 = s32 + G[:, j].float()
        e_gd = torch.where(s32.to(f64)[:, None] == gd_raw, torch.zeros_like(gd_raw), e_gd)
    gdyn_raw = r * rnd("gd", gd_raw)
    e_gdyn = U * gdyn_raw if is_bf else r_raw * e_gd + gd_raw * e_r + U * gdyn_raw
    return dict(r=r_raw, gw=torch.cat([gdyn_raw, G_raw[:, n_dyn:]], -1), e_r=e_r, e_gw=torch.cat([e_gdyn, e_G[:, n_dyn:]], -1),
                points=dict(sum=(ssum, e_sum), den=(den_raw, U * den_raw), r=(r_raw, e_r), G=(G_raw, e_G), gd=(gd_raw, e_gd)))


def drop_float_cases(S, dt):
    """the cases of test_token_drop_ties_and_floats: the hand-built ties under both policies, then the random masks at every capacity"""
    c = make_drop_ties(S, dt, 6500 + S)
    cr = make_drop(S, dt, 6000 + S)
    return [(c, c["cap"], "probs"), (c, c["cap"], "position")] + [(cr, cap, pol) for pol in ("probs", "position") for cap in drop_caps(cr)]


def ref_drop_floats(c, post):
    """float64 restatement of core.py:328-329 and :178-193 on the post-drop mask:
      r = q / (sum q + 1e-6), q = routing_w * mask;  G = softmax over the kept columns;  gw = [r sum_dyn G | G shared];  moe_w = gw mask.
    fp32 logits, first order (n = n_dyn, E columns):
      r     E32 = (n + 3) u r                       (n-term sum of non-negative terms, the add of 1e-6, the divide)
      G_e   E32 = tau_e G_e, tau_e = ((|x_e - max| + 2) + sum_a G_a (|x_a - max| + 2) + E + 3) u    (x - max carries u |x - max| into the exponent,
            the exponential 2 u -- for the element, and G-weighted for the denominator; the E-term sum; reciprocal and multiply)
      gw    E32 = r (sum_dyn E32(G) + n u sum_dyn G) + sum_dyn G E32(r) + u gw   on the dynamic columns
    bf16 logits: the finisher rounds to bf16 at sum, sum + 1e-6, r, G_e, sum_dyn G and r sum_dyn G (round_t), the reference at the same
    places (drop_chain).  Every output is then a bf16 value: bound 2^-8 |v| + (1 + 2^-8) E32 around the UNROUNDED float64 value v of
    its last step (from rounded inputs), E32 the fp32 error of that last step alone.
    Flagged intermediates (bf16 only): an intermediate at one of the five inner rounding points whose float64 value lies within its
    own E32 (about 2^-20 relative) of a rounding midpoint may round to the other neighbour in fp32.  Its one bf16 ulp is propagated
    exactly: the chain is evaluated once more per rounding point with the flagged intermediates on their other neighbour, and
    (1 + 2^-8) |v_other - v| is added to the bound of the outputs that move.  G_e of a shared column feeds no further step (its own
    output is compared around G_raw), so it is neither flagged nor counted.  No other element gets any allowance.  share = flagged /
    non-zero intermediates that feed a further step.  floor 2^-126.  A token that keeps no column at all is NaN in G, gw, moe_w (softmax over nothing), finite (0) in r."""
    n_dyn, n_real, n_fix = DROP_GEOM
    is_bf = c["logits"].dtype == bf16
    base = drop_chain(c, post)
    x_r, x_gw = torch.zeros_like(base["r"]), torch.zeros_like(base["gw"])
    n_flag = n_all = 0
    if is_bf:
        for stage, (v, e) in base["points"].items():
            flag = (mid_dist(v) <= e) & (e > 0)          # e == 0: exact in fp32 (and then often exactly ON a midpoint, where both round to even)
            if stage == "G":                             # a shared column's G_e feeds nothing further
                v, flag = v[:, :n_dyn], flag & (torch.arange(v.shape[1]) < n_dyn)
            n_flag += int(flag.sum())
            n_all += int((torch.nan_to_num(v, nan=0.0) != 0).sum())
            if bool(flag.any()):
                alt = drop_chain(c, post, (stage, flag))
                x_r += (1 + BF) * (alt["r"] - base["r"]).abs()
                x_gw += (1 + BF) * torch.nan_to_num((alt["gw"] - base["gw"]).abs(), nan=0.0)
        b_r = bf16_out(base["r"], base["e_r"]) + x_r + TINY
        b_gw = torch.nan_to_num(bf16_out(base["gw"], base["e_gw"]), nan=0.0) + x_gw + TINY
    else:
        b_r, b_gw = base["e_r"] + TINY, torch.nan_to_num(base["e_gw"], nan=0.0) + TINY
    keepf = (post[:, :n_real] != 0).to(f64)
    moved = int((x_r > 0).sum() + (x_gw > 0).sum())
    return dict(r=base["r"], b_r=b_r, gw=base["gw"], b_gw=b_gw, mw=base["gw"][:, :n_real] * keepf, b_mw=b_gw[:, :n_real] * keepf,
                share=n_flag / max(n_all, 1), moved=moved / (x_r.numel() + x_gw.numel()))


def emu_drop_floats(c, post):
    n_dyn, n_real, n_fix = DROP_GEOM
    is_bf = c["logits"].dtype == bf16
    rnd = rbf if is_bf else (lambda t: t)
    md = post[:, :n_dyn] != 0
    q = c["rw"] * md
    s = q[:, 0].clone()
    for j in range(1, n_dyn):
        s = s + q[:, j]
    den = rnd(rnd(s) + torch.tensor(1e-6, dtype=torch.float32))
    r = rnd(q / den[:, None])
    x = c["logits"].float().masked_fill(post == 0, float("-inf"))
    e = torch.exp(x - x.max(-1, keepdim=True)[0])
    G = rnd(e * (1.0 / e.sum(-1, keepdim=True)))
    ds = rnd(G[:, :n_dyn].sum(-1, keepdim=True))
    gw = torch.cat([rnd(r * ds), G[:, n_dyn:]], -1)
    return r, gw, gw[:, :n_real] * (post[:, :n_real] != 0).float()


def check_drop_floats(ref, r, gw, mw, stats):
    check("routing_weights", r, ref["r"], ref["b_r"], stats)
    check("global_weight", gw, ref["gw"], ref["b_gw"], stats)
    check("moe_weight", mw, ref["mw"], ref["b_mw"], stats)


# ================================================================================================ CPU self-checks
def _rejects(fn):
    with pytest.raises(AssertionError):
        fn()


def test_combine_permute_checkers_cpu():
    st = Stats()
    for (D, n_real, n_dyn, n_fix, shared) in [(2048, 8, 9, 2, True), (64, 8, 9, 0, True), (2048, 8, 9, 2, False)]:
        for S, mode in [(1, "all"), (1, "none"), (41, "mixed")]:
            c = make_combine(S, mode, D, n_real, n_dyn, n_fix, _combine_seed(D, n_real, n_fix, S, mode))
            r = ref_combine(c, shared)
            check_combine(c, r, shared, *emu_combine(c, shared), st)
            for ex in (True, False):
                check_permute(c, ref_permute(c, ex), ex, emu_permute(c, ex), st)
    assert max(st.values()) <= 1.0
    c = make_combine(41, "mixed", 2048, 8, 9, 2, 5)
    r = ref_combine(c, True)
    s = 1                                                      # selected every expert
    # one 8-element chunk of one row zeroed
    dy, dysh, mw, gs = emu_combine(c, True)
    dy[c["slot_of"][s, 3], 1024:1032] = 0
    _rejects(lambda: check_combine(c, r, True, dy, dysh, mw, gs, Stats()))
    # two experts' slot rows swapped for one token
    dy, dysh, mw, gs = emu_combine(c, True)
    a, b = c["slot_of"][s, 2], c["slot_of"][s, 5]
    dy[torch.stack([a, b])] = dy[torch.stack([b, a])]
    _rejects(lambda: check_combine(c, r, True, dy, dysh, mw, gs, Stats()))
    # one shared-expert row taken from token s + 1
    dy, dysh, mw, gs = emu_combine(c, True)
    dysh[41 + s] = dysh[41 + s + 1]
    _rejects(lambda: check_combine(c, r, True, dy, dysh, mw, gs, Stats()))
    # a d_mw entry for an unselected expert non-zero
    dy, dysh, mw, gs = emu_combine(c, True)
    mw[0, 4] = 1e-30
    _rejects(lambda: check_combine(c, r, True, dy, dysh, mw, gs, Stats()))
    # a pad row written
    dy, dysh, mw, gs = emu_combine(c, True)
    dy[3] = 0
    _rejects(lambda: check_combine(c, r, True, dy, dysh, mw, gs, Stats()))
    # a wrong column order inside pairs of chunks (the production path's failure mode: c ^ 1)
    dy, dysh, mw, gs = emu_combine(c, True)
    dy[c["slot_of"][s, 0]] = dy[c["slot_of"][s, 0]].view(-1, 2, 8).flip(1).reshape(-1)
    _rejects(lambda: check_combine(c, r, True, dy, dysh, mw, gs, Stats()))
    # permute: a chunk zeroed; a shared row of token s + 1; a token without a slot not exactly extra
    rp = ref_permute(c, True)
    dx = emu_permute(c, True)
    dx[7, 8:16] = 0
    _rejects(lambda: check_permute(c, rp, True, dx, Stats()))
    dx = emu_permute(c, True) .float()
    dx[s] += (c["dxsh"].float()[s + 1] - c["dxsh"].float()[s])
    _rejects(lambda: check_permute(c, rp, True, dx.to(bf16), Stats()))
    c0 = make_combine(41, "mixed", 2048, 8, 9, 0, 6)
    dx = emu_permute(c0, False)
    dx[0, 5] = -0.0
    _rejects(lambda: check_permute(c0, ref_permute(c0, False), False, dx, Stats()))


def _swiglu_seed(I, rows):
    return 2000 + I + rows


def test_swiglu_checker_cpu():
    st = Stats()
    for I, rows in SWIGLU_CASES + [SWIGLU_BIG]:
        c = make_swiglu(I, rows, _swiglu_seed(I, rows))
        r = ref_swiglu(c)
        assert r["share"] <= 1e-3, (I, rows, r["share"])
        if rows <= 77:
            out = torch.full((rows + 2, 2 * I), SENT, dtype=bf16)
            out[:rows] = emu_swiglu(c)
            check_swiglu(c, r, out, rows, st)
    assert max(st.values()) <= 1.0
    c = make_swiglu(96, 77, _swiglu_seed(96, 77))
    r = ref_swiglu(c)
    good = torch.full((77, 192), SENT, dtype=bf16)
    good[:74] = emu_swiglu(c)[:74]
    check_swiglu(c, r, good, 74, Stats())
    bad = good.clone()
    bad[40, 96 + 16:96 + 24] = 0                               # one chunk zeroed
    _rejects(lambda: check_swiglu(c, r, bad, 74, Stats()))
    bad = good.clone()
    bad[73] = SENT                                             # the last row of the ragged block left at the sentinel
    _rejects(lambda: check_swiglu(c, r, bad, 74, Stats()))
    bad = good.clone()
    bad[74] = emu_swiglu(c)[74]                                # a row beyond total_rows written
    _rejects(lambda: check_swiglu(c, r, bad, 74, Stats()))


def _rms_seed(D, S):
    return 3000 + D + S + (100000 if (D, S) == (2048, 16) else 0)       # 3000 + 2048 + 16 flags more than 1e-3 of its elements


def test_rmsnorm_checker_cpu():
    st = Stats()
    for D, S in RMS_CASES:
        c = make_rms(D, S, _rms_seed(D, S))
        for ds in ((False, True) if S in (17, 513) else (True,)):              # (the flags do not depend on dsum)
            r = ref_rms(c, ds)
            assert r["share"] <= 1e-3, (D, S, r["share"])
            check_rms(c, r, *emu_rms(c, ds), st)
    assert max(st.values()) <= 1.0
    c = make_rms(256, 513, _rms_seed(256, 513))
    r = ref_rms(c, True)
    dh, dw = emu_rms(c, True)
    bad = dh.clone()
    bad[100, 64:72] = 0
    _rejects(lambda: check_rms(c, r, bad, dw, Stats()))
    _rejects(lambda: check_rms(c, r, *emu_rms(c, True, mean_div=256 - 8), Stats()))       # mean of gy xh divided by D - 8
    _rejects(lambda: check_rms(c, r, *emu_rms(c, True, ss_div=256 - 8), Stats()))         # mean of squares divided by D - 8
    _rejects(lambda: check_rms(c, r, *emu_rms(c, True, drop_part=200), Stats()))          # one dropped part in the column sum
    bad = dh.clone()
    bad[512] = bad[511]                                                                    # the short last workgroup's row
    _rejects(lambda: check_rms(c, r, bad, dw, Stats()))


def test_aux_checker_cpu():
    from oracle import dcmoe_autograd as OA
    st = Stats()
    for S in (1, 255, 257, 1030):
        for dt in (torch.float32, bf16):
            c = make_aux(S, dt, 9, 2, 4000 + S)
            for ww in (True, False):
                r = ref_aux(c, ww)
                check("d_logits", emu_aux(c, ww), r["g"], r["bound"], st)
                z = c["logits"].to(f64).requires_grad_(True)               # the oracle's own function on float64 logits agrees
                (c["d_aux"] * OA.aux_loss(c["mask"], 9, z, c["tokw"].to(f64).reshape(1, S) if ww else None)).backward()
                assert float((z.grad - r["g"]).abs().max()) <= 1e-5 * float(r["g"].abs().max()) + 1e-15    # (the oracle takes the mask's means in float32)
    assert max(st.values()) <= 1.0
    c = make_aux(257, bf16, 9, 2, 4257)
    r = ref_aux(c, True)
    bad = emu_aux(c, True)
    bad[100] = bad[101]
    _rejects(lambda: check("d_logits", bad, r["g"], r["bound"], Stats()))
    bad = emu_aux(c, True)
    bad[2, 3] = 1e-20                                                       # a masked column with a gradient
    _rejects(lambda: check("d_logits", bad, r["g"], r["bound"], Stats()))


def check_router(got, g64, bound_ratio, norm, stats, name="d_logits"):
    ratio = token_ratio(got.cpu(), g64, norm)
    worst = float((ratio / bound_ratio).max())
    stats.note(name, worst)
    stats.note("kernel ratio", float(ratio.max()))
    assert worst <= 1.0, f"{name}: token error / bound = {worst:.4g} at token {int(ratio.argmax())}"


def test_router_checker_cpu():
    from oracle import router as OR
    st = Stats()
    for dt in (torch.float32, bf16):
        for form in ("plain", "drop", "rf"):
            c = make_router(257, dt, 9, 8, 2, 5000, True)
            o = OR.route(c["logits"], 9, 8, 2, TOP_P, 0, JIT, c["am"])
            k = o["top_k"].clone()
            post = router_post_mask(c, o["expert_mask"]) if form == "drop" else None
            fac = None
            if form == "rf":        # the factor a forward would hand over: the float32 graph's own mask_for_one, in the logits' dtype
                router_graph(c, form, k, None, torch.float32, torch.ones(257, 9))
                fac = c["own_factor"].to(dt).float()
                assert bool((fac < 0.5).any()) and bool((fac > 0.5).any())
            g64, order, mask = router_graph(c, form, k, post, f64, fac)
            live = torch.arange(9)[None] < k[:, None]
            if form == "rf":
                assert factor_agrees(c, fac, k, dt) == 0
                s_, j_ = [int(v) for v in torch.nonzero(live & (c["gate_margin"] > 0.1))[0]]
                bad = fac.clone()
                bad[s_, j_] = 1.3333 - bad[s_, j_]                          # a decision the gates leave no doubt about, taken the other way
                _rejects(lambda: factor_agrees(c, bad, k, dt))
            else:
                assert torch.equal(mask, o["expert_mask"])
                assert torch.equal(order[live], o["sel"][live])
            g32, _, _ = router_graph(c, form, k, post, torch.float32, fac)
            norm = router_norm(c)
            yard = 16 * float(token_ratio(g32, g64, norm).max())
            check_router(g32, g64, yard, norm, st)
            bad = g32.clone()
            bad[100] = bad[101]                                             # one token's gradient taken from its neighbour
            _rejects(lambda: check_router(bad, g64, yard, norm, Stats()))
            bad = g32.clone()
            bad[200, 3] += 1e-3
            _rejects(lambda: check_router(bad, g64, yard, norm, Stats()))
            if form == "rf":                                                # the gradient of a graph that takes every mask_for_one as 1
                bad, _, _ = router_graph(c, form, k, post, torch.float32, torch.ones(257, 9))
                _rejects(lambda: check_router(bad, g64, yard, norm, Stats()))


def test_rounds_train_restatement_equals_oracle_cpu():
    """rounds_train fed its own mask_for_one is oracle.dcmoe_autograd.routing_weights_train bit for bit, gradient included"""
    from oracle import dcmoe_autograd as OA
    c = make_router(257, torch.float32, 9, 8, 2, 5, True)
    k = torch.randint(0, 10, (257,), generator=gen(9))
    z = c["logits"].to(f64)[:, :9].clone().requires_grad_(True)
    w0, t0, o0 = OA.routing_weights_train(z, k, JIT, c["gumbel"].to(f64), c["rand_u"])
    (w0 * c["d_mw"].to(f64).sum(-1, keepdim=True)).sum().backward()
    g0, z.grad = z.grad.clone(), None
    own = rounds_train(z, k, JIT, c["gumbel"].to(f64), c["rand_u"], torch.ones(257, 9))[3]
    w1, t1, o1, _, _ = rounds_train(z, k, JIT, c["gumbel"].to(f64), c["rand_u"], own)
    (w1 * c["d_mw"].to(f64).sum(-1, keepdim=True)).sum().backward()
    assert torch.equal(w0, w1) and torch.equal(t0, t1) and torch.equal(o0, o1) and torch.equal(g0, z.grad)


def test_token_drop_checkers_cpu():
    st = Stats()
    for dt in (torch.float32, bf16):
        for S in (1, 257):
            c = make_drop(S, dt, 6000 + S)
            for policy in ("probs", "position"):
                for cap in drop_caps(c):
                    post = check_drop_mask(emu_drop_mask(c["logits"], c["mask"], 9, cap, policy), c["logits"], c["mask"], 9, cap, policy)
                    if S == 257:
                        check_drop_floats(ref_drop_floats(c, post), *emu_drop_floats(c, post), st)
        c = make_drop_ties(257, dt, 6500)
        cap = c["cap"]
        post = check_drop_mask(emu_drop_mask(c["logits"], c["mask"], 9, cap, "probs"), c["logits"], c["mask"], 9, cap, "probs")
        ref = ref_drop_floats(c, post)
        assert ref["share"] <= 1e-3, ref["share"]
        check_drop_floats(ref, *emu_drop_floats(c, post), st)
        zt = c["zero_ties"]
        assert bool(post[zt[:3], 4].all()) and not bool(post[zt[3:], 4].any())          # the three lowest indices of the ten zeros stay
        # a tie broken toward the higher index
        _rejects(lambda: check_drop_mask(emu_drop_mask(c["logits"], c["mask"], 9, cap, "probs", higher_index_wins=True), c["logits"], c["mask"], 9, cap, "probs"))
        # +0.0 ranked above -0.0 (distinct keys: the sign bit folded like any other)
        raw = c["logits"].contiguous().view(torch.int16 if dt == bf16 else torch.int32).to(torch.int64) & (0xffff if dt == bf16 else 0xffffffff)
        sign = 0x8000 if dt == bf16 else 0x80000000
        old = torch.where((raw & sign) != 0, ~raw & (2 * sign - 1), raw | sign)
        _rejects(lambda: check_drop_mask(emu_drop_mask(c["logits"], c["mask"], 9, cap, "probs", keys=old), c["logits"], c["mask"], 9, cap, "probs"))
        # one token kept beyond capacity
        bad = post.clone()
        dropped = torch.nonzero((c["mask"][:, 1] != 0) & (post[:, 1] == 0)).flatten()
        bad[dropped[0], 1] = 1
        _rejects(lambda: check_drop_mask(bad, c["logits"], c["mask"], 9, cap, "probs"))
        for policy in ("position",):
            bad = emu_drop_mask(c["logits"], c["mask"], 9, cap, policy)
            bad[torch.nonzero((c["mask"][:, 10] != 0) & (bad[:, 10] == 0)).flatten()[0], 10] = 1
            _rejects(lambda: check_drop_mask(bad, c["logits"], c["mask"], 9, cap, policy))
        # floats: a weight of a dropped column not zero; a token's global weights from its neighbour
        r, gw, mw = emu_drop_floats(c, post)
        bad = r.clone()
        bad[dropped[0], 1] = 1e-3
        _rejects(lambda: check_drop_floats(ref, bad, gw, mw, Stats()))
        bad = gw.clone()
        bad[50] = gw[51]
        _rejects(lambda: check_drop_floats(ref, r, bad, mw, Stats()))
    assert max(st.values()) <= 1.0


def test_token_drop_flagged_share_cpu():
    """every case of test_token_drop_ties_and_floats flags at most 1e-3 of its intermediates, and the emulated finisher passes on it"""
    from oracle.dcmoe import drop_keep_mask
    st = Stats()
    for S in (257, 1000):
        for cc, cap, pol in drop_float_cases(S, bf16):
            post = drop_keep_mask(cc["logits"], cc["mask"], 9, cap, pol)
            ref = ref_drop_floats(cc, post)
            assert ref["share"] <= 1e-3, (S, cap, pol, ref["share"])
            check_drop_floats(ref, *emu_drop_floats(cc, post), st)
    assert max(st.values()) <= 1.0


# ================================================================================================ GPU tests
@gpu
@pytest.mark.parametrize("D,n_real,n_dyn,n_fix,shared", GEOMS)
def test_combine_bwd_vs_fp64(dev, D, n_real, n_dyn, n_fix, shared):
    """ref_combine states the bounds.  D = 2048 with n_real <= 12, n_fix <= 4 and (y_shared or n_fix == 0) is the register-resident
    path; 13 experts, D = 64 and D = 2056 (257 chunks: a second trip of the chunk loop for one thread) the fallback loop."""
    from unimoe_audio_amd import ops
    st = Stats()
    for S, mode in S_MODES:
        c = make_combine(S, mode, D, n_real, n_dyn, n_fix, _combine_seed(D, n_real, n_fix, S, mode))
        r = ref_combine(c, shared)
        dy = torch.full((c["cap"], D), SENT, dtype=bf16, device=dev)
        dysh = torch.full((max(1, n_fix) * S, D), SENT, dtype=bf16, device=dev)
        ysh = c["ysh"].to(dev) if (shared and n_fix) else None
        d_mw, d_gs = ops.combine_bwd(c["dout"].to(dev), c["y"].to(dev), c["slot_of"].to(torch.int32).to(dev), c["w"].to(dev), ysh,
                                     c["gw"].to(dev), n_dyn, n_fix, dy, dysh if n_fix else None)
        check_combine(c, r, shared, dy, dysh, d_mw, d_gs, st)
    st.show(f"combine_bwd D={D} {n_real}/{n_dyn}/{n_fix} shared={shared}")


@gpu
@pytest.mark.parametrize("D,n_real,n_dyn,n_fix,shared", GEOMS[:6])
def test_permute_bwd_vs_fp64(dev, D, n_real, n_dyn, n_fix, shared):
    """ref_permute states the bound.  (GEOMS[6] differs from GEOMS[0] only in y_shared, which permute_bwd does not have.)"""
    from unimoe_audio_amd import ops
    st = Stats()
    for S, mode in S_MODES:
        c = make_combine(S, mode, D, n_real, n_dyn, n_fix, _combine_seed(D, n_real, n_fix, S, mode))
        for ex in (True, False):
            dx = ops.permute_bwd(c["dxe"].to(dev), c["slot_of"].to(torch.int32).to(dev), c["dxsh"].to(dev) if n_fix else None, n_fix,
                                 extra=c["extra"].to(dev) if ex else None)
            check_permute(c, ref_permute(c, ex), ex, dx, st)
    st.show(f"permute_bwd D={D} {n_real}/{n_dyn}/{n_fix}")


@gpu
@pytest.mark.parametrize("I,rows", SWIGLU_CASES + [SWIGLU_BIG])
def test_swiglu_bwd_vs_fp64(dev, I, rows):
    """ref_swiglu states the bounds.  Contiguous buffers with total_rows = None; column views of wider buffers (leading dimensions
    I + 24, 2 I + 40, 2 I + 16) with *total_rows equal to max_rows (the only view case with data at rows = 1), below it, and 0."""
    from unimoe_audio_amd import ops
    st = Stats()
    c = make_swiglu(I, rows, _swiglu_seed(I, rows))
    r = ref_swiglu(c)
    assert r["share"] <= 1e-3
    out = torch.full((rows, 2 * I), SENT, dtype=bf16, device=dev)
    ops.swiglu_bwd(c["dh"].to(dev), c["gu"].to(dev), I, out, total_rows=None, max_rows=rows)
    check_swiglu(c, r, out, rows, st)
    if rows <= 77:
        wdh = torch.full((rows, I + 24), 3.0, dtype=bf16, device=dev)
        wgu = torch.full((rows, 2 * I + 40), 3.0, dtype=bf16, device=dev)
        wdh[:, 8:8 + I] = c["dh"].to(dev)
        wgu[:, 16:16 + 2 * I] = c["gu"].to(dev)
        for total in sorted({rows, max(rows - 3, 0), 0}):
            wout = torch.full((rows, 2 * I + 16), SENT, dtype=bf16, device=dev)
            ops.swiglu_bwd(wdh[:, 8:8 + I], wgu[:, 16:16 + 2 * I], I, wout[:, 8:8 + 2 * I],
                           total_rows=torch.tensor([total], dtype=torch.int32, device=dev), max_rows=rows)
            check_swiglu(c, r, wout[:, 8:8 + 2 * I], total, st)
            keeps_sentinel("pad columns of dgu", torch.cat([wout[:, :8], wout[:, 8 + 2 * I:]], -1))
    st.show(f"swiglu_bwd I={I} rows={rows} flagged {r['share']:.2e}")


@gpu
@pytest.mark.parametrize("D,S", RMS_CASES)
def test_rmsnorm_bwd_vs_fp64(dev, D, S):
    """ref_rms states the bounds.  D selects the thread quarters in use (8: 1 thread; 256: 32 threads; 2048: one quarter full;
    2056: a second quarter with one thread; 8192: all four), S the rows per workgroup (1, 2, 3 with a short last workgroup) and the
    part count of the column sum around its 16-wide unrolled loop."""
    from unimoe_audio_amd import ops
    st = Stats()
    c = make_rms(D, S, _rms_seed(D, S))
    for ds in (False, True):
        r = ref_rms(c, ds)
        assert r["share"] <= 1e-3
        dh, dw = ops.rmsnorm_bwd(c["h"].to(dev), c["w"].to(dev), c["dy"].to(dev), RMS_EPS, dsum=c["dsum"].to(dev) if ds else None)
        check_rms(c, r, dh, dw, st)
    st.show(f"rmsnorm_bwd D={D} S={S} flagged {r['share']:.2e}")


@gpu
@pytest.mark.parametrize("dt", [torch.float32, bf16])
def test_aux_loss_bwd_vs_fp64(dev, dt):
    """ref_aux states the bound; masked columns and the shared columns are exactly zero."""
    from unimoe_audio_amd import ops
    st = Stats()
    for S in (1, 255, 257, 1030):
        c = make_aux(S, dt, 9, 2, 4000 + S)
        for ww in (True, False):
            r = ref_aux(c, ww)
            got = ops.aux_loss_bwd(c["logits"].to(dev), c["mask"].to(dev), 9, c["tokw"].to(dev) if ww else None, torch.tensor(c["d_aux"], device=dev))
            check("d_logits", got, r["g"], r["bound"], st)
    st.show(f"aux_loss_bwd {dt}")


@gpu
@pytest.mark.parametrize("form", ["plain", "drop", "rf"])
@pytest.mark.parametrize("n_dyn,n_real,n_fix", ROUTER_GEOMS)
@pytest.mark.parametrize("dt", [torch.float32, bf16])
def test_router_bwd_vs_fp64(dev, dt, n_dyn, n_real, n_fix, form):
    """Per token: |got - g64|_inf / N_s <= 16 * max over the test's tokens (every S of this test) of |g32 - g64|_inf / N_s, with
    N_s = sum|d_moe_w| + sum|d_gw_shared| + |d_logits_in|_inf and g32 / g64 the same oracle graph on the CPU in float32 / float64
    (router_graph; form "rf" takes mask_for_one from the forward kernel, see rounds_train).  The integer decisions of ops.router_fwd equal those of the graph (order, mask) before gradients are compared;
    the Top-P count is the kernel's (two tokens get k = 0 and an empty mask by hand); mask_for_one: factor_agrees.  d_logits_in is
    given for odd S only."""
    from unimoe_audio_amd import ops
    st = Stats()
    runs, tied = [], 0
    for S in ROUTER_S:
        c = make_router(S, dt, n_dyn, n_real, n_fix, 5000 + S + n_dyn, with_in=(S % 2 == 1))
        lg = c["logits"].to(dev)
        kw = dict(gumbel=c["gumbel"].to(dev), rand_u=c["rand_u"].to(dev)) if form == "rf" else {}
        rt = ops.router_fwd(None, None, n_dyn=n_dyn, n_real=n_real, n_fix=n_fix, top_p=TOP_P, jitter_eps=JIT, logits_in=lg,
                            attn_mask=c["am"].to(dev), **kw)
        k, sel, mask_k = rt["top_k"].cpu().clone(), rt["sel"].cpu().clone(), rt["expert_mask"].cpu().clone()
        if S > 40:                                         # k = 0 with an empty mask
            k[18:20] = 0
            mask_k[18:20, :n_dyn] = 0
            c["am"][18:20] = False
        post = router_post_mask(c, mask_k) if form == "drop" else None
        fac = rt["round_factor"].cpu() if form == "rf" else None
        g64, order, mask = router_graph(c, form, k, post, f64, fac)
        assert torch.equal(mask, mask_k), "expert_mask of ops.router_fwd and of the float64 graph differ"
        if form == "rf":
            tied += factor_agrees(c, fac, k, dt)
        live = torch.arange(n_dyn)[None] < k[:, None]
        assert torch.equal(order[live], sel[live]), "selection order of ops.router_fwd and of the float64 graph differ"
        if S > 40:
            assert int(k.max()) == n_dyn and int(k.min()) == 0
        g32, _, _ = router_graph(c, form, k, post, torch.float32, fac)
        used_mask = post if form == "drop" else mask_k
        got = ops.router_bwd(lg, sel.to(dev), k.to(dev), used_mask.to(dev), c["d_mw"].to(dev), c["d_gs"].to(dev) if n_fix else None,
                             c["d_in"].to(dev) if c["d_in"] is not None else None, n_dyn, n_real, n_fix, JIT, token_drop=(form == "drop"),
                             round_factor=rt["round_factor"] if form == "rf" else None)
        runs.append((got.cpu(), g32, g64, router_norm(c)))
    yard = max(float(token_ratio(g32, g64, n).max()) for _, g32, g64, n in runs)
    st.note("fp32 oracle ratio", yard)
    for got, g32, g64, n in runs:
        check_router(got, g64, 16 * yard, n, st)
    st.show(f"router_bwd {dt} {n_dyn}/{n_real}/{n_fix} {form}" + (f" (rounds whose mask_for_one bf16 gates decide as a tie: {tied})" if form == "rf" else ""))


@gpu
@pytest.mark.parametrize("dt", [torch.float32, bf16])
@pytest.mark.parametrize("policy", ["probs", "position"])
def test_token_drop_mask_exact(dev, dt, policy):
    """the post-drop mask equals oracle.dcmoe.drop_keep_mask for every token: S around the one-token-per-thread limit (256) and the
    training size (6240: 25 tokens per thread), capacities 0, 1, below every column's count, between the smallest and the largest,
    >= S and the configured one."""
    from unimoe_audio_amd import ops
    n_dyn, n_real, n_fix = DROP_GEOM
    lost = kept_all = 0
    for S in DROP_S:
        c = make_drop(S, dt, 6000 + S)
        for cap in drop_caps(c):
            o = ops.token_drop(c["logits"].to(dev), c["mask"].to(dev), c["rw"].to(dev), n_dyn=n_dyn, n_real=n_real, n_fix=n_fix, capacity=cap, policy=policy)
            want = check_drop_mask(o["expert_mask"], c["logits"], c["mask"], n_dyn, cap, policy)
            before, after = c["mask"].sum(0), want.sum(0)
            lost += int(((after < before)).sum())
            kept_all += int(((after == before) & (before > 0)).sum())
        assert lost > 0 and kept_all > 0, (S, lost, kept_all)
        lost = kept_all = 0
    print(f"\nBWD FP64 token_drop mask {dt} {policy}: exact for every token")


@gpu
@pytest.mark.parametrize("dt", [torch.float32, bf16])
@pytest.mark.parametrize("S", [257, 1000])
def test_token_drop_ties_and_floats(dev, dt, S):
    """the hand-built tie columns of make_drop_ties (mask exact, the three lowest-index zeros of either sign kept), and the float
    outputs of these cases and of the random ones per element (ref_drop_floats states the bounds); "position" at capacity 0 and 1
    leaves tokens without any column: NaN exactly where the restatement is NaN."""
    from unimoe_audio_amd import ops
    n_dyn, n_real, n_fix = DROP_GEOM
    st = Stats()
    cases = drop_float_cases(S, dt)
    c = cases[0][0]
    saw_nan = False
    share = moved = 0.0
    for cc, cap, pol in cases:
        o = ops.token_drop(cc["logits"].to(dev), cc["mask"].to(dev), cc["rw"].to(dev), n_dyn=n_dyn, n_real=n_real, n_fix=n_fix, capacity=cap, policy=pol)
        post = check_drop_mask(o["expert_mask"], cc["logits"], cc["mask"], n_dyn, cap, pol)
        if cc is c and pol == "probs":
            zt = c["zero_ties"]
            assert bool(post[zt[:3], 4].all()) and not bool(post[zt[3:], 4].any())
        ref = ref_drop_floats(cc, post)
        saw_nan |= bool(torch.isnan(ref["gw"]).any())
        share, moved = max(share, ref["share"]), max(moved, ref["moved"])
        assert ref["share"] <= 1e-3, (cap, pol, ref["share"])
        check_drop_floats(ref, o["routing_weights"], o["global_weight"], o["moe_weight"], st)
    assert saw_nan
    st.show(f"token_drop floats {dt} S={S} flagged {share:.2e} (outputs that carry an allowance {moved:.2e})")

