"""The last stretch from codec tokens to the waveform -- the two direct convolution kernels of csrc/umoe_dac.hip (dac_conv1d_kernel,
dac_convt1d_kernel) with the fused Snake, bias, tanh and residual, their windowed twins, the polyphase resampler, and the RVQ sums
umoe_rvq_from_codes / umoe_rvq_from_delayed (csrc/umoe_misc.hip) -- per element against float64 on the CPU from the same fp32 input
bits, at every tile edge (tiles of 64 channels x 64 positions, input channels in chunks of 8).

Rules of the whole file
  * reference: float64.  F.conv1d / F.conv_transpose1d in float64 on snake64(x) = x + sin(alpha x)^2 / (alpha + 1e-9) in float64.
  * comparison: per element, never a norm.  With u = 2^-24 and for ANY summation order
      E_acc = (n + 2) u S + u |ref|,   S = sum |snake64(x)| |w| + |bias|  (the same float64 convolution on absolute values),
      n     = the taps an output sums: Cin K for conv1d, Cin x (taps k = (t + pad) mod stride, + stride, ... < K) for the transposed form;
      Snake adds E_x = sum |w| e_snake(x) (the same absolute-value convolution), e_snake = 4 E_snake,
      E_snake = (2 |alpha x| + 8) u / (alpha + 1e-9) + 2 u |snake64|: the envelope of the codec's own fp32 formula (torch fp32 on the
      CPU stays at or below 0.49 E_snake in every band of |alpha x| up to 4096: test_snake_formula_cpu); the factor 4 is what a fast
      sine may add -- a second rounding of the argument (the scaling to revolutions) and the hardware's approximation error;
      tanh: E = E_pre + 4 u (|tanh'| <= 1, tanhf a few ulp); then the residual add: + u |y|.  tanh comes BEFORE the residual.
  * untouched memory: outputs are prefilled with a sentinel (7.0).  A full-sequence launch writes into the middle of a longer buffer
    whose 64 floats on either side keep the sentinel; a windowed launch leaves the columns of y outside [t_begin, t_begin + n) alone,
    umoe_rvq_from_delayed the rows of z that the row map skips and the columns outside [z_off, z_off + n).
  * unread memory: a windowed launch gets input and residual buffers that hold exactly the positions its outputs need and NaN in a
    margin of 2 on either side (inside [0, L), where the kernel may load them into outputs it never stores, and past L, where it may
    not load at all).  Only stored outputs are checked; a NaN in one fails.
  * exact values: an output none of whose taps falls on an input (padding wider than the filter's reach, a transposed phase with no
    tap) equals the bias bit for bit; Snake with alpha = 0 returns x bit for bit.
  * refusals: a nonzero return, umoe_last_error names the cause, nothing is written.
Every GPU test prints its worst error / bound under -s ("DAC FP64 ..."); a ratio above 1 fails.

Cases (B = 3 for the convolutions; each with and without Snake unless noted)
  snake        1x1 conv1d with identity weights and no bias = snake(x) + exact zeros: 20 channels alpha = 0.05 .. 20 (log-spaced) and one
               alpha = 0 channel, |alpha x| in (0, 8], (8, 64], (64, 512], (512, 1608], (1608, 4096], 52 000 elements per band
  conv1d       pos      K = 1, Cin 3, Cout 5, L 1 / 63 / 64 / 65 / 129
               cout     Cout 1 / 63 / 64 / 65 / 130, Cin 9, K 3, pad 1, L 70
               cin      Cin 1 / 7 / 8 / 9 / 17, Cout 5, K 3, L 70
               resunit  K 7, dilation 1 / 3 / 9, pad 3 dil, + residual, L 100 and L 20 (receptive field 55 > L)
               strided  stride 2 / 4 / 5 / 8, K = 2 stride, pad = ceil(stride / 2), L % stride != 0 with Lout = 65; stride 5 also with Lout = 72
               padding  pad 0 (K 5, dilation 2) and pad 4 > (K - 1) dil = 2: the two outputs at either edge equal the bias
               head     Cout 1, K 7, pad 3, Snake, tanh, pre-activations spanning +-4; and tanh with a residual (no layer of the product)
               refusals K 32 at stride 8 (82 688 bytes of LDS); every (L, K, dil, stride, pad) of a small grid with an empty output,
                        L=2 K=3 stride=2 pad=0 and L=1 K=4 stride=3 pad=1 among them, through umoe_dac_conv1d, umoe_dac_conv1d_win
                        and dac.conv1d
  transposed   product  stride 2 / 4 / 5 / 8, K = 2 stride, pad = ceil(stride / 2), out_pad 0 / 1 for stride 5, L 1 / 8 / 9 / 33
               general  K = stride, K = 2 stride + 1, K 3 < stride 5 with pad 1 and pad 0, K = 2 stride with pad 0
               channels Cin 1 / 7 / 9 x Cout 1 / 65
  windows      every geometry above with Lout >= 70: outputs [0, 5), [61, 70), [1, Lout - 1) (more than one tile), [Lout - 3, Lout)
  resampler    44100 / 24000 / 22050 / 8000 -> 16000 and 16000 -> 44100, B = 2, L 1 / 5 / 700, every sample, float64 sum over the fp32
               filter bits of dac.resample_filter, bound (K_taps + 1) u sum |k x|
  rvq          from_codes: NQ 1 / 12 x Dl 1 / 255 / 256 / 257 x T 1 / 3, codes 0, CB - 1 and out of range on both sides (clamped), bound
               (cd + NQ + 2) u sum |.|; from_delayed: the same sums through the delay pattern, frames at or past t_valid read pad, a row
               map with a repeated and two out-of-range rows, z_off = 2 in a wider Lz

The checkers are tested without a GPU (test_*_cpu): an fp32 torch emulation (fp32 Snake, fp32 convolution) passes every case above,
and each planted error is rejected: a tap shifted by one position from t = 64 on, the last partial input-channel chunk dropped, the
transposed phase off by one, tanh and the residual swapped, the bias missing on the last channel tile, 1 / alpha for
1 / (alpha + 1e-9) at alpha = 0, an element written outside a window, a NaN stored, a frame past t_valid not read as pad, a code
not clamped.

Found by this file
  1. Output length rounded the wrong way.  umoe_dac_conv1d and umoe_dac_conv1d_win computed (L + 2 pad - dil (K - 1) - 1) / stride + 1
     with C's truncating division: a numerator in (-stride, 0) gave Lout = 1 for an empty output (L=2 K=3 stride=2 pad=0), and the
     kernel stored one element per channel behind the empty y that dac.conv1d had allocated.  Fixed: dac_conv_out_len() takes the
     floor, both entry points refuse an empty output by name before they look at y, and dac.conv1d raises that error.
  2. No defect: the fast sine.  snake() uses __sinf, which compiles to one multiply by 1 / 2 pi and v_sin_f32 with no reduction of the
     argument (read in the ISA).  On this card v_sin_f32 does NOT give up past 256 revolutions (|alpha x| ~ 1608): it reduces the
     argument itself, and what __sinf adds to an accurate sine is the second rounding of the argument, about 1.45 |alpha x| u radians
     at any size (max |__sinf(p) - sin64(p)| over 400 000 draws per band, p = fl(alpha x): 11 u, 93 u, 743 u, 1.9e3 u, 5.9e3 u; sinf:
     1.0 - 1.2 u).  e_snake = 4 E_snake covers that with room: every band, the one beyond 1608 included, stays at or below 0.2.  The same
     draws through a sine reduced to [-0.5, 0.5] revolutions with an fma and the low half of 1 / 2 pi gave 0.11 - 0.12 and through
     sinf 0.09 - 0.12: a gain that nothing here asks for.  No band fails, so snake() stays as it is.
  3. Nothing else: every tile, chunk, stride, padding and window edge above, the resampler and the RVQ sums pass at the first run.

Measured on an MI355X (the whole file: 17 GPU tests in 1.2 s on the card; the five tests without a GPU in 3 s), worst error / bound:
  snake                (0, 8] 0.14, (8, 64] 0.17, (64, 512] 0.20, (512, 1608] 0.18, (1608, 4096] 0.18 of e_snake = 4 E_snake; alpha = 0 exact
  conv1d               without Snake / with Snake (the Snake term widens the bound, so the ratio falls):
    pos                0.38 / 0.12        cout     0.15 / 0.062       cin      0.36 / 0.071      resunit  0.070 / 0.036
    strided            0.054 / 0.034      padding  0.091 / 0.037      head     0.0085 (tanh), 0.031 (tanh + residual)
  conv_transpose1d     product 0.18 / 0.069, general 0.30 / 0.089, channels 0.49 / 0.12 (Cin = 1: a sum of two products against a bound of four roundings)
  windows              conv1d (104 launches): [0, 5) 0.27, [61, 70) 0.34, [1, Lout - 1) 0.38, [Lout - 3, Lout) 0.22
                       conv_transpose1d (128 launches): 0.42, 0.41, 0.49, 0.38; no sentinel touched, no NaN stored
  refusals             all refused by name, nothing written
  resample             44100->16000 0.0090, 24000->16000 0.14, 22050->16000 0.0066, 8000->16000 0.28, 16000->44100 0.022
  rvq_from_codes       NQ = 1 0.21, NQ = 12 0.062         rvq_from_delayed   0.060 / 0.054 / 0.048
The largest ratios belong to the shortest sums (K = 1 with Cin = 3, Cin = 1), where a bound of n + 2 roundings is tight; the long sums
of the product's shapes stay below 0.1.  The windowed kernels give the ratios of the full kernels, as their bit-identity promises.
"""
import ctypes as C
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from test_gpu_bwd_fp64 import Stats as _Stats, check, keeps_sentinel

gpu = pytest.mark.gpu

U = 2.0 ** -24          # fp32 unit roundoff
SNAKE_K = 4.0           # e_snake = SNAKE_K * E_snake
SENT = 7.0
NAN = float("nan")
GUARD = 64              # sentinel floats on either side of a full-sequence output
MARGIN = 2              # NaN positions on either side of what a windowed launch needs
B = 3
f64 = torch.float64
BANDS = [(0.0, 8.0), (8.0, 64.0), (64.0, 512.0), (512.0, 1608.0), (1608.0, 4096.0)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from unimoe_audio_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


class Stats(_Stats):
    def show(self, title):
        print(f"\nDAC FP64 {title}: " + ", ".join(f"{k} {v:.3g}" for k, v in self.items()))


def gen(name):
    return torch.Generator().manual_seed(sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % (2 ** 31))


# ------------------------------------------------------------------------------------------------ Snake
def snake32(x, a):
    """the codec's own arithmetic: fp32 torch"""
    a = a.reshape(1, -1, 1)
    return x + torch.sin(a * x) ** 2 / (a + 1e-9)


def snake64(x, a):
    x, a = x.to(f64), a.to(f64).reshape(1, -1, 1)
    return x + torch.sin(a * x) ** 2 / (a + 1e-9)


def snake_env(x, a):
    """E_snake"""
    x64, a64 = x.to(f64), a.to(f64).reshape(1, -1, 1)
    return (2 * (a64 * x64).abs() + 8) * U / (a64 + 1e-9) + 2 * U * snake64(x, a).abs()


def draw_bands(g, alphas, per):
    """x [1][C][5 per] with |alpha x| uniform in each band, random signs"""
    cols = []
    for lo, hi in BANDS:
        lo2, hi2 = lo * (1 + 1e-5), hi * (1 - 1e-5)
        t = lo2 + (hi2 - lo2) * torch.rand(alphas.numel(), per, generator=g, dtype=f64)
        sign = torch.randint(0, 2, t.shape, generator=g).to(f64) * 2 - 1
        cols.append(sign * t / alphas.to(f64)[:, None])
    return torch.cat(cols, 1).float()[None].contiguous()


def band_masks(x, a):
    t = (a.to(f64).reshape(1, -1, 1) * x.to(f64)).abs()
    return [(t > lo) & (t <= hi) for lo, hi in BANDS]


@functools.lru_cache(maxsize=None)
def snake_case():
    g = gen("snake bands")
    alphas = torch.exp(torch.linspace(math.log(0.05), math.log(20.0), 20, dtype=f64)).float()
    per = 2600
    x = draw_bands(g, alphas, per)
    x = torch.cat([x, 3 * torch.randn(1, 1, 5 * per, generator=g)], 1).contiguous()          # the alpha = 0 channel
    a = torch.cat([alphas, torch.zeros(1)])
    Cn = a.numel()
    c = dict(kind="conv", name="snake", Cin=Cn, Cout=Cn, K=1, L=5 * per, stride=1, dil=1, pad=0, out_pad=0, tanh=False,
             x=x, w=torch.eye(Cn).reshape(Cn, Cn, 1).contiguous(), b=None, alpha=a, resid=None, Lout=5 * per)
    c["ref"] = snake64(x, a)
    c["bound"] = SNAKE_K * snake_env(x, a)
    c["masks"] = band_masks(x, a)
    return c


def check_snake(c, y, stats):
    """per band; the alpha = 0 channel returns x bit for bit"""
    y = y.detach().cpu()
    for i, m in enumerate(c["masks"]):
        assert int(m.sum()) >= 50000, (i, int(m.sum()))
        check(f"({BANDS[i][0]:g}, {BANDS[i][1]:g}]", y[m], c["ref"][m], c["bound"][m], stats)
    check("all", y, c["ref"], c["bound"], stats)
    assert torch.equal(y[:, -1].contiguous().view(torch.int32), c["x"][:, -1].contiguous().view(torch.int32)), "Snake with alpha = 0 must return x exactly"


# ------------------------------------------------------------------------------------------------ convolution cases (specs only)
def c1(name, Cin, Cout, K, L, stride=1, dil=1, pad=0, resid=False, tanh=False, snakes=(False, True), span=None):
    return dict(kind="conv", name=name, Cin=Cin, Cout=Cout, K=K, L=L, stride=stride, dil=dil, pad=pad, out_pad=0, resid=resid, tanh=tanh,
                snakes=snakes, span=span)


def ct(name, Cin, Cout, K, L, stride, pad, out_pad=0):
    return dict(kind="convt", name=name, Cin=Cin, Cout=Cout, K=K, L=L, stride=stride, dil=1, pad=pad, out_pad=out_pad, resid=False, tanh=False,
                snakes=(False, True), span=None)


def _strided_L(s, lout):
    """smallest L that is no multiple of the stride with floor((L + 2 pad - 2 s) / s) + 1 == lout"""
    p = math.ceil(s / 2)
    L = (lout - 1) * s + 2 * s - 2 * p
    return L if L % s else L + 1


CONV_GROUPS = {
    "pos": [c1(f"pos_L{L}", 3, 5, 1, L) for L in (1, 63, 64, 65, 129)],
    "cout": [c1(f"cout_{co}", 9, co, 3, 70, pad=1) for co in (1, 63, 64, 65, 130)],
    "cin": [c1(f"cin_{ci}", ci, 5, 3, 70) for ci in (1, 7, 8, 9, 17)],
    "resunit": [c1(f"res_d{d}_L{L}", 9, 9, 7, L, dil=d, pad=3 * d, resid=True) for d in (1, 3, 9) for L in (100, 20)],
    "strided": [c1(f"stride_{s}", 9, 5, 2 * s, _strided_L(s, 65), stride=s, pad=math.ceil(s / 2)) for s in (2, 4, 5, 8)] +
               [c1("stride_5_L72", 9, 5, 10, _strided_L(5, 72), stride=5, pad=3)],
    "padding": [c1("pad_0", 9, 5, 5, 80, dil=2, pad=0), c1("pad_wide", 9, 5, 3, 70, pad=4)],
    "head": [c1("head", 17, 1, 7, 70, pad=3, tanh=True, snakes=(True,), span=4.0),
             c1("tanh_resid", 9, 5, 3, 70, pad=1, resid=True, tanh=True, snakes=(True,), span=2.0)],      # no layer of the product: pins tanh BEFORE the residual
}
CONVT_GROUPS = {
    "product": [ct(f"t_s{s}_op{op}_L{L}", 9, 5, 2 * s, L, s, math.ceil(s / 2), op) for s in (2, 4, 5, 8) for op in ((0, 1) if s % 2 else (0,))
                for L in (1, 8, 9, 33)],
    "general": [ct("t_K_eq_s", 9, 5, 4, 20, 4, 1), ct("t_K_2s1", 9, 5, 9, 20, 4, 2), ct("t_K_lt_s", 9, 5, 3, 20, 5, 1), ct("t_K_lt_s_pad0", 9, 5, 3, 20, 5, 0),
                ct("t_pad0", 9, 5, 8, 20, 4, 0)],
    "channels": [ct(f"t_ci{ci}_co{co}", ci, co, 8, 20, 4, 2) for ci in (1, 7, 9) for co in (1, 65)],
}
SPECS = {s["name"]: s for grp in list(CONV_GROUPS.values()) + list(CONVT_GROUPS.values()) for s in grp}
LDS_REFUSAL = dict(Cin=8, Cout=8, K=32, L=600, stride=8, dil=1, pad=4)


def out_len(s, L=None):
    L = s["L"] if L is None else L
    if s["kind"] == "conv":
        num = L + 2 * s["pad"] - s["dil"] * (s["K"] - 1) - 1
        return 0 if num < 0 else num // s["stride"] + 1
    return (L - 1) * s["stride"] - 2 * s["pad"] + s["K"] + s["out_pad"]


def windows_of(lout):
    return [(0, 5), (61, 9), (1, lout - 2), (lout - 3, 3)] if lout >= 70 else []


def empty_geometries():
    """(L, K, dil, stride, pad) of a small grid whose output is truly empty"""
    out = [(L, K, d, s, p) for L in (1, 2, 3, 4) for K in (2, 3, 4, 5) for d in (1, 2) for s in (1, 2, 3, 4) for p in (0, 1)
           if L + 2 * p - d * (K - 1) - 1 < 0]
    assert (2, 3, 1, 2, 0) in out and (1, 4, 1, 3, 1) in out
    return out


# ------------------------------------------------------------------------------------------------ convolution cases: data, reference
def _conv(c, x, w, b):
    if c["kind"] == "conv":
        return F.conv1d(x, w, b, stride=c["stride"], padding=c["pad"], dilation=c["dil"])
    return F.conv_transpose1d(x, w, b, stride=c["stride"], padding=c["pad"], output_padding=c["out_pad"])


@functools.lru_cache(maxsize=None)
def conv_case(name, snake):
    """inputs (CPU, fp32), float64 reference and bound of a case, computed once"""
    c = dict(SPECS[name])
    g = gen(name + ("+snake" if snake else ""))
    Cin, Cout, K, L = c["Cin"], c["Cout"], c["K"], c["L"]
    c["snake"] = snake
    c["x"] = 1.5 * torch.randn(B, Cin, L, generator=g)
    wshape = (Cout, Cin, K) if c["kind"] == "conv" else (Cin, Cout, K)
    c["w"] = torch.randn(wshape, generator=g) / (Cin * K) ** 0.5
    c["b"] = 0.1 * torch.randn(Cout, generator=g)
    c["alpha"] = (0.3 + 2.7 * torch.rand(Cin, generator=g)) if snake else None
    c["Lout"] = out_len(c)
    c["resid"] = torch.randn(B, Cout, c["Lout"], generator=g) if c["resid"] else None
    xin = snake64(c["x"], c["alpha"]) if snake else c["x"].to(f64)
    if c["span"]:                                   # scale the weights so that the pre-activations span about +- span
        pre = _conv(c, xin, c["w"].to(f64), None)
        c["w"] = (c["w"] * (c["span"] / float(pre.abs().max()))).contiguous()
    w64, b64 = c["w"].to(f64), c["b"].to(f64)
    pre = _conv(c, xin, w64, b64)
    S = _conv(c, xin.abs(), w64.abs(), b64.abs())
    ones = _conv(c, torch.ones(1, 1, L, dtype=f64), torch.ones(1, 1, K, dtype=f64), None)[0, 0]
    c["no_tap"] = ones == 0                                                      # outputs that see no input at all
    if c["kind"] == "conv":
        n = torch.full((c["Lout"],), float(Cin * K), dtype=f64)
    else:
        n = torch.tensor([Cin * len(range((t + c["pad"]) % c["stride"], K, c["stride"])) for t in range(c["Lout"])], dtype=f64)
    E = (n + 2) * U * S + U * pre.abs()
    if snake:
        E = E + _conv(c, SNAKE_K * snake_env(c["x"], c["alpha"]), w64.abs(), None)
    ref = pre
    if c["tanh"]:
        ref, E = torch.tanh(pre), E + 4 * U
        c["pre_span"] = float(pre.abs().max())
    if c["resid"] is not None:
        ref = ref + c["resid"].to(f64)
        E = E + U * ref.abs()
    c["ref"], c["bound"] = ref, E
    return c


def all_cases(groups):
    return [conv_case(s["name"], sn) for grp in groups.values() for s in grp for sn in s["snakes"]]


def emu_conv(c, plant=None):
    """the launch in fp32 torch arithmetic (any summation order will do: the bound is order-free).  plant: a wrong kernel"""
    Cin, Cout, K = c["Cin"], c["Cout"], c["K"]
    x, w, a = c["x"], c["w"].clone(), c["alpha"]
    b = torch.zeros(Cout) if c["b"] is None else c["b"].clone()
    xin = x if a is None else snake32(x, a)
    if plant == "alpha0":                                         # 1 / alpha for 1 / (alpha + 1e-9)
        xin = x + torch.sin(a.reshape(1, -1, 1) * x) ** 2 / a.reshape(1, -1, 1)
    if plant == "chunk":                                          # the last partial chunk of 8 input channels dropped
        assert Cin % 8
        if c["kind"] == "conv":
            w[:, Cin // 8 * 8:] = 0
        else:
            w[Cin // 8 * 8:] = 0
    pre = _conv(c, xin, w, None)
    if plant == "tap":                                            # from t = 64 on the last tap reads one position further
        wl = torch.zeros_like(w)
        wl[..., K - 1] = w[..., K - 1]
        d = _conv(c, torch.roll(xin, -1, -1), wl, None) - _conv(c, xin, wl, None)
        pre[..., 64:] += d[..., 64:]
    if plant == "bias":                                           # no bias on the last channel tile
        b[(Cout - 1) // 64 * 64:] = 0
    pre = pre + b.reshape(1, -1, 1)
    if plant == "phase":                                          # (t + pad + 1) % stride, (t + pad + 1) / stride
        pre = torch.roll(pre, -1, -1)
    if plant == "swap":
        return torch.tanh(pre + c["resid"])
    y = torch.tanh(pre) if c["tanh"] else pre
    if c["resid"] is not None:
        y = y + c["resid"]
    if plant == "nan":
        y[0, 0, -1] = NAN
    return y


def check_conv(c, y, stats, tag=None):
    """a full-sequence output, every element"""
    y = y.detach().cpu()
    check(tag or c["name"], y, c["ref"], c["bound"], stats)
    if not c["tanh"] and c["resid"] is None and bool(c["no_tap"].any()):
        got = y[:, :, c["no_tap"]]
        assert torch.equal(got.view(torch.int32), c["b"].reshape(1, -1, 1).expand_as(got).contiguous().view(torch.int32)), \
            f"{c['name']}: an output without a tap must equal the bias"


def win_reads(c, t0, n):
    """[a, b] of the input positions inside [0, L) that outputs [t0, t0 + n) read (a > b: none)"""
    s, p, K = c["stride"], c["pad"], c["K"]
    if c["kind"] == "conv":
        lo, hi = t0 * s - p, (t0 + n - 1) * s - p + (K - 1) * c["dil"]
    else:
        lo, hi = -((K - 1 - t0 - p) // s), (t0 + n - 1 + p) // s
    return max(lo, 0), min(hi, c["L"] - 1)


def win_buffers(c, t0, n):
    """x / resid: the needed positions and a NaN margin; y: the window inside a sentinel buffer.  -> dict of CPU tensors and offsets"""
    a, b = win_reads(c, t0, n)
    if a <= b:
        x_off = max(a - MARGIN, 0)
        xb = torch.full((B, c["Cin"], b + 1 + MARGIN - x_off), NAN)
        xb[:, :, a - x_off:b + 1 - x_off] = c["x"][:, :, a:b + 1]
    else:
        x_off, xb = 0, torch.full((B, c["Cin"], MARGIN), NAN)
    d = dict(x=xb, x_off=x_off, t0=t0, n=n, r=None, r_off=0)
    if c["resid"] is not None:
        d["r_off"] = max(t0 - MARGIN, 0)
        d["r"] = torch.full((B, c["Cout"], t0 + n + MARGIN - d["r_off"]), NAN)
        d["r"][:, :, t0 - d["r_off"]:t0 - d["r_off"] + n] = c["resid"][:, :, t0:t0 + n]
    d["y_off"] = max(t0 - 3, 0)
    d["y"] = torch.full((B, c["Cout"], t0 + n + 5 - d["y_off"]), SENT)
    return d


def emu_win(c, wb, y_full, plant=None):
    y = wb["y"].clone()
    lo = wb["t0"] - wb["y_off"]
    y[:, :, lo:lo + wb["n"]] = y_full[:, :, wb["t0"]:wb["t0"] + wb["n"]]
    if plant == "outside":                                        # one element written outside the window
        y[B - 1, c["Cout"] - 1, lo + wb["n"]] = 0.5
    return y


def check_win(c, wb, y, stats, tag=None):
    y = y.detach().cpu()
    lo, n, t0 = wb["t0"] - wb["y_off"], wb["n"], wb["t0"]
    check(tag or c["name"], y[:, :, lo:lo + n], c["ref"][:, :, t0:t0 + n], c["bound"][:, :, t0:t0 + n], stats)
    inside = torch.zeros(y.shape, dtype=torch.bool)
    inside[:, :, lo:lo + n] = True
    keeps_sentinel(f"{c['name']} window [{t0}, {t0 + n}): y outside the window", y[~inside])


# ------------------------------------------------------------------------------------------------ launches
def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _lib():
    from unimoe_audio_amd import _lib as L
    return L.lib()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def last_error():
    msg = _lib().umoe_last_error()
    return msg.decode() if msg else ""


def on_dev(c, dev):
    if "dev" not in c:
        c["dev"] = {k: (None if c[k] is None else c[k].to(dev).contiguous()) for k in ("x", "w", "b", "alpha", "resid")}
    return c["dev"]


def launch_full(c, dev):
    """the full-sequence kernel into the middle of a sentinel buffer -> y [B][Cout][Lout] (CPU); the guards are checked here"""
    d = on_dev(c, dev)
    nb = c["x"].shape[0]
    numel = nb * c["Cout"] * c["Lout"]
    buf = torch.full((numel + 2 * GUARD,), SENT, dtype=torch.float32, device=dev)
    y = C.c_void_p(buf.data_ptr() + 4 * GUARD)
    lo = C.c_int(-1)
    if c["kind"] == "conv":
        rc = _lib().umoe_dac_conv1d(_p(d["x"]), _p(d["w"]), _p(d["b"]), _p(d["alpha"]), _p(d["resid"]), nb, c["Cin"], c["L"], c["Cout"],
                                    c["K"], c["stride"], c["dil"], c["pad"], int(c["tanh"]), y, C.byref(lo), _stream())
    else:
        rc = _lib().umoe_dac_conv_transpose1d(_p(d["x"]), _p(d["w"]), _p(d["b"]), _p(d["alpha"]), nb, c["Cin"], c["L"], c["Cout"], c["K"],
                                              c["stride"], c["pad"], c["out_pad"], y, C.byref(lo), _stream())
    assert rc == 0, (c["name"], last_error())
    assert lo.value == c["Lout"], (c["name"], lo.value, c["Lout"])
    buf = buf.cpu()
    keeps_sentinel(f"{c['name']}: before y", buf[:GUARD])
    keeps_sentinel(f"{c['name']}: behind y", buf[GUARD + numel:])
    return buf[GUARD:GUARD + numel].view(nb, c["Cout"], c["Lout"])


def launch_win(c, wb, dev):
    d = on_dev(c, dev)
    x, r, y = wb["x"].to(dev), (None if wb["r"] is None else wb["r"].to(dev)), wb["y"].to(dev)
    if c["kind"] == "conv":
        rc = _lib().umoe_dac_conv1d_win(_p(x), wb["x_off"], x.shape[2], _p(d["w"]), _p(d["b"]), _p(d["alpha"]), _p(r), wb["r_off"],
                                        0 if r is None else r.shape[2], B, c["Cin"], c["L"], c["Cout"], c["K"], c["stride"], c["dil"], c["pad"],
                                        int(c["tanh"]), wb["t0"], wb["n"], _p(y), wb["y_off"], y.shape[2], _stream())
    else:
        rc = _lib().umoe_dac_conv_transpose1d_win(_p(x), wb["x_off"], x.shape[2], _p(d["w"]), _p(d["b"]), _p(d["alpha"]), B, c["Cin"], c["L"], c["Cout"],
                                                  c["K"], c["stride"], c["pad"], c["out_pad"], wb["t0"], wb["n"], _p(y), wb["y_off"], y.shape[2],
                                                  _stream())
    assert rc == 0, (c["name"], wb["t0"], wb["n"], last_error())
    return y.cpu()


# ------------------------------------------------------------------------------------------------ resampler
RATES = [(44100, 16000), (24000, 16000), (22050, 16000), (8000, 16000), (16000, 44100)]
RES_L = (1, 5, 700)


@functools.lru_cache(maxsize=None)
def res_case(orig, new, L):
    from unimoe_audio_amd import dac as D
    kern, o, n, width = D.resample_filter(orig, new)
    K = 2 * width + o
    assert kern.dtype == torch.float32 and tuple(kern.shape) == (n, K)
    g = gen(f"resample {orig} {new} {L}")
    x = torch.randn(2, L, generator=g)
    lout = math.ceil(n * L / o)
    frames = -(-lout // n)
    c = dict(orig=orig, new=new, L=L, x=x, kern=kern, o=o, n=n, width=width, K=K, Lout=lout, frames=frames)
    ref, ab = res_sum(c, f64)
    c["ref"], c["bound"] = ref, (K + 1) * U * ab
    return c


def res_sum(c, dt):
    """y[b][frame n + phase] = sum_t kern[phase][t] x[b][frame o - width + t] in dtype dt -> (y, the same sum of absolute values)"""
    right = max(0, (c["frames"] - 1) * c["o"] + c["K"] - c["width"] - c["L"])
    xp = F.pad(c["x"].to(dt), (c["width"], right))[:, None]
    k = c["kern"].to(dt)[:, None]
    y = F.conv1d(xp, k, stride=c["o"])[:, :, :c["frames"]]
    ab = F.conv1d(xp.abs(), k.abs(), stride=c["o"])[:, :, :c["frames"]]
    flat = lambda t: t.transpose(1, 2).reshape(t.shape[0], -1)[:, :c["Lout"]].contiguous()
    return flat(y), flat(ab)


# ------------------------------------------------------------------------------------------------ RVQ sums
CB, CD = 11, 8
RVQ_SHAPES = [(nq, dl, t) for nq in (1, 12) for dl in (1, 255, 256, 257) for t in (1, 3)]
SPECIAL = [0, CB - 1, -1, CB, -2 ** 31, 2 ** 31 - 1]


@functools.lru_cache(maxsize=None)
def rvq_tables(nq, dl):
    g = gen(f"rvq {nq} {dl}")
    return dict(cb=torch.randn(nq, CB, CD, generator=g), ow=torch.randn(nq, dl, CD, generator=g) / CD ** 0.5, ob=0.1 * torch.randn(nq, dl, generator=g))


def rvq_ref(tb, codes, dt=f64, clamp=True):
    """codes [NQ][T] (any integers) -> (z [Dl][T], sum |.|) in dtype dt"""
    cb, ow, ob = tb["cb"].to(dt), tb["ow"].to(dt), tb["ob"].to(dt)
    nq, T = codes.shape
    z = torch.zeros(ow.shape[1], T, dtype=dt)
    ab = torch.zeros_like(z)
    for q in range(nq):
        cq = codes[q].long()
        cq = cq.clamp(0, CB - 1) if clamp else cq % CB
        e = cb[q][cq]                                             # [T][cd]
        z += ow[q] @ e.t() + ob[q][:, None]
        ab += ow[q].abs() @ e.abs().t() + ob[q].abs()[:, None]
    return z, ab


@functools.lru_cache(maxsize=None)
def rvq_case(i):
    nq, dl, T = RVQ_SHAPES[i]
    g = gen(f"codes {i}")
    codes = torch.randint(0, CB, (nq, T), generator=g, dtype=torch.int32)
    flat = codes.view(-1)
    for j in range(min(flat.numel(), len(SPECIAL))):
        flat[j] = SPECIAL[(i + j) % len(SPECIAL)]
    tb = rvq_tables(nq, dl)
    z, ab = rvq_ref(tb, codes)
    return dict(nq=nq, dl=dl, T=T, codes=codes, tb=tb, ref=z, bound=(CD + nq + 2) * U * ab)


DELAYED = [(12, 257), (1, 1), (12, 256)]


@functools.lru_cache(maxsize=None)
def delayed_case(i):
    """tokens [3][Tmax][NQ]; frames [f0, f0 + n) of rows (1, 1, 7, 0, -1) into columns [z_off, z_off + n) of z [5][Dl][Lz]"""
    nq, dl = DELAYED[i]
    g = gen(f"delayed {i}")
    Bt, Tmax, t_valid, pad, f0, n, z_off = 3, 14, 9, 5, 1, 8, 2
    tokens = torch.randint(0, CB, (Bt, Tmax, nq), generator=g, dtype=torch.int32)
    tokens[:, t_valid:] = (pad + 1 + torch.randint(0, CB - 1, (Bt, Tmax - t_valid, nq), generator=g, dtype=torch.int32)) % CB       # never the pad code
    tokens[0, 1, 0], tokens[1, 3, nq - 1], tokens[2, 2, 0] = -3, CB + 7, CB                                                   # clamped
    prefill = torch.tensor([0, 2, 1], dtype=torch.int32)
    delay = torch.tensor([0] + [1 + (q * 5) % 4 for q in range(1, nq)], dtype=torch.int32)
    rows = torch.tensor([1, 1, 7, 0, -1], dtype=torch.int32)
    tb = rvq_tables(nq, dl)
    c = dict(nq=nq, dl=dl, B=Bt, Tmax=Tmax, t_valid=t_valid, pad=pad, f0=f0, n=n, z_off=z_off, Lz=n + 5, tokens=tokens, prefill=prefill, delay=delay,
             rows=rows, tb=tb)
    c["ref"], c["bound"] = {}, {}
    for r, row in enumerate(rows.tolist()):
        if 0 <= row < Bt:
            z, ab = rvq_ref(tb, delayed_codes(c, row))
            c["ref"][r], c["bound"][r] = z, (CD + nq + 2) * U * ab
    assert any(int(prefill[row]) + f0 + n - 1 + int(delay.max()) >= t_valid for row in (0, 1)) and int(prefill.max()) + f0 < t_valid
    return c


def delayed_codes(c, row, past_valid_reads_pad=True):
    """the delay pattern reverted: code[q][t - f0] = tokens[row][prefill + t + delay[q]][q], pad at or past t_valid"""
    codes = torch.empty(c["nq"], c["n"], dtype=torch.int64)
    for q in range(c["nq"]):
        for j in range(c["n"]):
            p = int(c["prefill"][row]) + c["f0"] + j + int(c["delay"][q])
            inside = p < (c["t_valid"] if past_valid_reads_pad else c["Tmax"])
            codes[q, j] = int(c["tokens"][row, p, q]) if inside else c["pad"]
    return codes


def emu_delayed(c, plant=None):
    z = torch.full((c["rows"].numel(), c["dl"], c["Lz"]), SENT)
    for r, row in enumerate(c["rows"].tolist()):
        if 0 <= row < c["B"]:
            z[r, :, c["z_off"]:c["z_off"] + c["n"]] = rvq_ref(c["tb"], delayed_codes(c, row, plant != "valid"), torch.float32, plant != "clamp")[0]
    if plant == "row":
        z[2] = z[1]
    if plant == "column":
        z[0, 0, c["z_off"] + c["n"]] = 0.0
    return z


def check_delayed(c, z, stats):
    z = z.detach().cpu()
    written = torch.zeros(z.shape, dtype=torch.bool)
    for r in c["ref"]:
        cols = slice(c["z_off"], c["z_off"] + c["n"])
        written[r, :, cols] = True
        check(f"NQ={c['nq']} Dl={c['dl']}", z[r, :, cols], c["ref"][r], c["bound"][r], stats)
    keeps_sentinel(f"from_delayed NQ={c['nq']} Dl={c['dl']}: z outside the frames of the mapped rows", z[~written])


# ================================================================================================ checkers without a GPU
def _rejects(fn):
    with pytest.raises(AssertionError):
        fn()


def test_case_lists_cpu():
    """the case lists hold the shapes they are meant to hold"""
    assert [out_len(s) for s in CONV_GROUPS["strided"]] == [65, 65, 65, 65, 72] and all(s["L"] % s["stride"] for s in CONV_GROUPS["strided"])
    assert {out_len(s) for s in CONV_GROUPS["pos"]} == {1, 63, 64, 65, 129}
    assert {(s["stride"], s["L"]): out_len(s) for s in CONVT_GROUPS["product"] if s["stride"] == 8 and s["L"] in (8, 9)} == {(8, 8): 64, (8, 9): 72}
    assert any(s["dil"] * (s["K"] - 1) + 1 > s["L"] for s in CONV_GROUPS["resunit"])
    assert any(s["pad"] > (s["K"] - 1) * s["dil"] for s in CONV_GROUPS["padding"])
    assert conv_case("pad_wide", False)["no_tap"].tolist() == [True, True] + [False] * 72 + [True, True]
    assert int(conv_case("t_K_lt_s", False)["no_tap"].sum()) > 30 and int(conv_case("t_K_lt_s_pad0", False)["no_tap"].sum()) > 30
    assert 3.5 < conv_case("head", True)["pre_span"] < 4.5
    for s in SPECS.values():
        assert out_len(s) > 0, s["name"]
        for t0, n in windows_of(out_len(s)):
            assert 0 <= t0 and n > 0 and t0 + n <= out_len(s)
    with_windows = [s["name"] for s in SPECS.values() if out_len(s) >= 70]
    assert len(with_windows) >= 30 and {"pos_L129", "cout_130", "res_d9_L100", "stride_5_L72", "pad_wide", "head", "t_s8_op0_L9", "t_K_lt_s"} <= set(with_windows)
    s = LDS_REFUSAL
    xw = 63 * s["stride"] + (s["K"] - 1) * s["dil"] + 1
    assert (8 * xw + 8 * s["K"] * 64) * 4 > 64 * 1024
    assert len(empty_geometries()) > 100
    assert all(int(m.sum()) >= 50000 for m in snake_case()["masks"])


def test_snake_formula_cpu():
    """E_snake is the envelope of the codec's fp32 formula: fp32 torch against float64 stays below it in every band (0.49 at 2M draws
    per band; here 200 000), and the 1x1 identity convolution of the Snake case passes with e_snake = 4 E_snake"""
    g = gen("snake formula")
    alphas = torch.exp(torch.linspace(math.log(0.05), math.log(20.0), 100, dtype=f64)).float()
    x = draw_bands(g, alphas, 2000)
    st = Stats()
    for i, m in enumerate(band_masks(x, alphas)):
        check(f"({BANDS[i][0]:g}, {BANDS[i][1]:g}]", snake32(x, alphas)[m], snake64(x, alphas)[m], snake_env(x, alphas)[m], st)
    st.show("fp32 torch Snake / E_snake")
    assert max(st.values()) < 1.0
    c = snake_case()
    st = Stats()
    check_snake(c, emu_conv(c), st)
    st.show("emulated Snake case / e_snake")
    _rejects(lambda: check_snake(c, emu_conv(c, "alpha0"), Stats()))
    bad = emu_conv(c)
    m = c["masks"][4]
    bad[m] = c["x"][m]                                            # a sine that gives up past 256 revolutions
    _rejects(lambda: check_snake(c, bad, Stats()))


def test_conv_checkers_cpu():
    """the fp32 emulation passes every convolution case, full and windowed"""
    st = Stats()
    for groups, tag in ((CONV_GROUPS, "conv1d"), (CONVT_GROUPS, "transposed")):
        for c in all_cases(groups):
            y = emu_conv(c)
            check_conv(c, y, st, tag)
            for t0, n in windows_of(c["Lout"]):
                wb = win_buffers(c, t0, n)
                check_win(c, wb, emu_win(c, wb, y), st, tag + " windows")
    assert max(st.values()) <= 1.0
    st.show("emulated cases")


def test_conv_planted_errors_cpu():
    def full(name, snake, plant):
        c = conv_case(name, snake)
        check_conv(c, emu_conv(c), Stats())
        _rejects(lambda: check_conv(c, emu_conv(c, plant), Stats()))

    for snake in (False, True):
        full("pos_L129", snake, "tap")
        full("cout_65", snake, "tap")
        full("res_d3_L100", snake, "tap")
        for name in ("cin_1", "cin_7", "cin_9", "cin_17", "t_ci7_co1", "t_ci9_co65"):
            full(name, snake, "chunk")
        for name in ("t_s2_op0_L9", "t_s5_op1_L8", "t_s8_op0_L33", "t_K_lt_s", "t_K_2s1"):
            full(name, snake, "phase")
        for name in ("cout_1", "cout_65", "cout_130", "t_ci9_co65"):
            full(name, snake, "bias")
        full("cin_9", snake, "nan")
    full("tanh_resid", True, "swap")
    # 1 / alpha: one alpha = 0 channel
    c = dict(conv_case("cin_9", True))
    c["alpha"] = c["alpha"].clone()
    c["alpha"][3] = 0.0
    c["ref"], c["bound"] = None, None
    xin = snake64(c["x"], c["alpha"])
    w64, b64 = c["w"].to(f64), c["b"].to(f64)
    c["ref"] = _conv(c, xin, w64, b64)
    c["bound"] = (c["Cin"] * c["K"] + 2) * U * _conv(c, xin.abs(), w64.abs(), b64.abs()) + U * c["ref"].abs() + \
        _conv(c, SNAKE_K * snake_env(c["x"], c["alpha"]), w64.abs(), None)
    check_conv(c, emu_conv(c), Stats())
    _rejects(lambda: check_conv(c, emu_conv(c, "alpha0"), Stats()))
    # windows: an element outside, a NaN inside, a window taken one position off
    for name in ("cout_65", "res_d9_L100", "t_s8_op0_L9"):
        c = conv_case(name, True)
        y = emu_conv(c)
        for t0, n in windows_of(c["Lout"]):
            wb = win_buffers(c, t0, n)
            check_win(c, wb, emu_win(c, wb, y), Stats())
            _rejects(lambda: check_win(c, wb, emu_win(c, wb, y, "outside"), Stats()))
            _rejects(lambda: check_win(c, wb, emu_win(c, wb, torch.roll(y, 1, -1)), Stats()))
            bad = emu_win(c, wb, y)
            bad[0, 0, t0 - wb["y_off"]] = NAN
            _rejects(lambda: check_win(c, wb, bad, Stats()))
        # the buffers hold NaN everywhere but at the needed positions
        wb = win_buffers(c, 61, 9)
        a, b = win_reads(c, 61, 9)
        assert int(torch.isnan(wb["x"]).sum()) == (wb["x"].shape[2] - (b - a + 1)) * B * c["Cin"] and wb["x"].shape[2] == b - a + 1 + 2 * MARGIN
        if wb["r"] is not None:
            assert int((~torch.isnan(wb["r"])).sum()) == 9 * B * c["Cout"]


def test_resample_rvq_checkers_cpu():
    st = Stats()
    for orig, new in RATES:
        for L in RES_L:
            c = res_case(orig, new, L)
            y = res_sum(c, torch.float32)[0]
            assert tuple(y.shape) == (2, c["Lout"])
            check("resample", y, c["ref"], c["bound"], st)
    c = res_case(44100, 16000, 700)
    y = res_sum(c, torch.float32)[0]
    bad = dict(c, kern=torch.roll(c["kern"], 1, 0))                                                      # every sample through its neighbour phase's filter
    _rejects(lambda: check("resample", res_sum(bad, torch.float32)[0], c["ref"], c["bound"], Stats()))
    _rejects(lambda: check("resample", torch.roll(y, 1, 1), c["ref"], c["bound"], Stats()))
    seen = set()
    for i in range(len(RVQ_SHAPES)):
        c = rvq_case(i)
        seen |= set(c["codes"].view(-1).tolist())
        check("from_codes", rvq_ref(c["tb"], c["codes"], torch.float32)[0], c["ref"], c["bound"], st)
        if bool(((c["codes"] < 0) | (c["codes"] >= CB)).any()):                                             # a code wrapped instead of clamped
            _rejects(lambda: check("from_codes", rvq_ref(c["tb"], c["codes"], torch.float32, clamp=False)[0], c["ref"], c["bound"], Stats()))
    assert set(SPECIAL) <= seen
    for i in range(len(DELAYED)):
        c = delayed_case(i)
        check_delayed(c, emu_delayed(c), st)
        for plant in ("valid", "clamp", "row", "column"):
            _rejects(lambda: check_delayed(c, emu_delayed(c, plant), Stats()))
    assert max(st.values()) <= 1.0
    st.show("emulated resampler / RVQ")


# ================================================================================================ GPU tests
@gpu
def test_snake_bands_vs_fp64(dev):
    """the fused Snake alone (1x1 identity convolution), |alpha x| up to 4096, against float64 within e_snake = 4 E_snake, per band"""
    c = snake_case()
    st = Stats()
    try:
        check_snake(c, launch_full(c, dev), st)
    finally:
        st.show("snake, per band of |alpha x|")


@gpu
@pytest.mark.parametrize("group", list(CONV_GROUPS))
def test_conv1d_vs_fp64(dev, group):
    st = Stats()
    for s in CONV_GROUPS[group]:
        for sn in s["snakes"]:
            c = conv_case(s["name"], sn)
            check_conv(c, launch_full(c, dev), st, s["name"] + ("+snake" if sn and len(s["snakes"]) > 1 else ""))
    st.show(f"conv1d {group}")


@gpu
@pytest.mark.parametrize("group", list(CONVT_GROUPS))
def test_conv_transpose1d_vs_fp64(dev, group):
    st = Stats()
    for s in CONVT_GROUPS[group]:
        for sn in s["snakes"]:
            c = conv_case(s["name"], sn)
            check_conv(c, launch_full(c, dev), st, s["name"] + ("+snake" if sn else ""))
    st.show(f"conv_transpose1d {group}")


@gpu
@pytest.mark.parametrize("groups,tag", [(CONV_GROUPS, "conv1d"), (CONVT_GROUPS, "conv_transpose1d")], ids=["conv1d", "conv_transpose1d"])
def test_windows_vs_fp64(dev, groups, tag):
    """the windowed twins against the float64 reference itself, from buffers that hold the needed positions and NaN around them, into
    a sentinel buffer"""
    st = Stats()
    count = 0
    for c in all_cases(groups):
        for t0, n in windows_of(c["Lout"]):
            wb = win_buffers(c, t0, n)
            check_win(c, wb, launch_win(c, wb, dev), st, f"[{t0 if t0 < 62 else 'Lout-3'}, +{n if n < 10 else 'Lout-2'})")
            count += 1
    st.show(f"{tag} windows ({count} launches)")


@gpu
def test_conv1d_refusals(dev):
    """a tile that needs more than 64 KB of LDS and every empty output: nonzero return, the cause by name, nothing written"""
    from unimoe_audio_amd import _lib as L, dac as D
    lib = _lib()
    x = torch.randn(1, 8, 600, device=dev)
    w = torch.randn(8, 8, 32, device=dev)
    y = torch.full((4096,), SENT, device=dev)
    s = LDS_REFUSAL
    lo = C.c_int(-1)
    rc = lib.umoe_dac_conv1d(_p(x), _p(w), None, None, None, 1, s["Cin"], s["L"], s["Cout"], s["K"], s["stride"], s["dil"], s["pad"], 0, _p(y), C.byref(lo),
                             _stream())
    assert rc != 0 and "LDS" in last_error(), (rc, last_error())
    rc = lib.umoe_dac_conv1d_win(_p(x), 0, s["L"], _p(w), None, None, None, 0, 0, 1, s["Cin"], s["L"], s["Cout"], s["K"], s["stride"], s["dil"], s["pad"],
                                 0, 0, 1, _p(y), 0, 64, _stream())
    assert rc != 0 and "LDS" in last_error(), (rc, last_error())
    with pytest.raises(L.UmoeError, match="LDS"):
        D.conv1d(x, w, None, stride=s["stride"], padding=s["pad"])
    for (Lx, K, d, st, p) in empty_geometries():
        lo = C.c_int(-1)
        rc = lib.umoe_dac_conv1d(_p(x), _p(w), None, None, None, 1, 2, Lx, 3, K, st, d, p, 0, _p(y), C.byref(lo), _stream())
        assert rc != 0 and "empty output" in last_error() and lo.value == -1, (Lx, K, d, st, p, rc, last_error(), lo.value)
        rc = lib.umoe_dac_conv1d_win(_p(x), 0, Lx, _p(w), None, None, None, 0, 0, 1, 2, Lx, 3, K, st, d, p, 0, 0, 1, _p(y), 0, 64, _stream())
        assert rc != 0 and "empty output" in last_error(), (Lx, K, d, st, p, rc, last_error())
    for (Lx, K, st, p) in ((2, 3, 2, 0), (1, 4, 3, 1), (1, 7, 1, 0)):
        with pytest.raises(L.UmoeError, match="empty output"):
            D.conv1d(x[:, :2, :Lx].contiguous(), w[:3, :2, :K].contiguous(), None, stride=st, padding=p)
    torch.cuda.synchronize()
    keeps_sentinel("refused launches", y)


@gpu
def test_resample_vs_fp64(dev):
    from unimoe_audio_amd import dac as D
    st = Stats()
    for orig, new in RATES:
        for L in RES_L:
            c = res_case(orig, new, L)
            y = D.resample(c["x"].to(dev), orig, new)
            assert tuple(y.shape) == (2, c["Lout"])
            check(f"{orig}->{new}", y, c["ref"], c["bound"], st)
    st.show("resample")


@gpu
def test_rvq_from_codes_vs_fp64(dev):
    st = Stats()
    for i in range(len(RVQ_SHAPES)):
        c = rvq_case(i)
        tb = {k: v.to(dev).contiguous() for k, v in c["tb"].items()}
        numel = c["dl"] * c["T"]
        buf = torch.full((numel + 2 * GUARD,), SENT, device=dev)
        codes = c["codes"].to(dev)
        rc = _lib().umoe_rvq_from_codes(_p(codes), _p(tb["cb"]), _p(tb["ow"]), _p(tb["ob"]), c["nq"], CB, CD, c["dl"], c["T"],
                                        C.c_void_p(buf.data_ptr() + 4 * GUARD), _stream())
        assert rc == 0, last_error()
        buf = buf.cpu()
        keeps_sentinel("from_codes: around z", torch.cat([buf[:GUARD], buf[GUARD + numel:]]))
        check(f"NQ={c['nq']}", buf[GUARD:GUARD + numel].view(c["dl"], c["T"]), c["ref"], c["bound"], st)
    st.show("rvq_from_codes")


@gpu
def test_rvq_from_delayed_vs_fp64(dev):
    st = Stats()
    for i in range(len(DELAYED)):
        c = delayed_case(i)
        tb = {k: v.to(dev).contiguous() for k, v in c["tb"].items()}
        tokens, prefill, delay, rows = (c[k].to(dev) for k in ("tokens", "prefill", "delay", "rows"))
        z = torch.full((rows.numel(), c["dl"], c["Lz"]), SENT, device=dev)
        rc = _lib().umoe_rvq_from_delayed(_p(tokens), c["B"], c["Tmax"], c["nq"], _p(prefill), _p(delay), c["t_valid"], c["pad"], _p(rows), rows.numel(),
                                          c["f0"], c["n"], _p(tb["cb"]), _p(tb["ow"]), _p(tb["ob"]), CB, CD, c["dl"], _p(z), c["z_off"], c["Lz"], _stream())
        assert rc == 0, last_error()
        check_delayed(c, z, st)
    st.show("rvq_from_delayed")
