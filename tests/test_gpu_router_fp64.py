"""The forward side of the Top-P router (csrc/umoe_router.hip, csrc/umoe_router_dev.h: router_kernel, router_kernel4, router_norm_kernel, the
router riding inside the gate/up launch of csrc/umoe_gemm.hip) and the tables built from its mask (dispatch_small_kernel, dispatch_kernel,
permute_kernel), each against a float64 restatement on the CPU of the same operation on the same input bits.

1. Launch forms.  CASES lists (form, S, D, n_dyn, n_fix, flags); form_of() restates launch_router / umoe_router_fwd / route_token and
   test_table_cpu asserts that every case reaches the form it names, that the shapes the forms switch at are in the list and that every
   option (both logit types, norm_w, h_out, attn_mask, top_p = 0 with fixed_top_k) occurs in every form.  (9, 2) with n_real = 9 / 1 is
   listed with the generic geometries but is dispatched to the <9,2> instantiation: n_real only bounds moe_weight.
2. Front end.
   h_out    the candidate rule of test_gpu_fwd_fp64.py (its helpers are imported): bit for bit against rbf(w rbf(x rs)) in float64, except where
            x rs lies within the fp32 window of a bf16 rounding midpoint; then either neighbour's chain; at most CAP = 1e-2 of a case
            flagged (checked on the CPU on the inputs the GPU tests use).  The window, u = 2^-24: the sum of squares is a sum of positive
            terms of depth d = 8 c + 6 (c chunks per lane; 6 wave levels) + 3 in router_kernel4 (the four wave sums, in order), so its
            relative error is d u; the divide and the add of eps 1 u each; all halved by the root; rsqrtf 2 u; the product 1 u:
            ((d + 2) / 2 + 3) u |x rs| (h_window).  Without norm_w h_out is x, bit for bit.
   logits   reference: z64 = the float64 dot product of the kernel's own h (read back: an exact bf16 input of the GEMV) with the gate rows.
            A lane sums the 8 products of a chunk in order (8 adds), adds the chunk sums of its c chunks (c adds), six butterfly levels
            join the 64 lanes and router_kernel4 adds the four wave sums in order: depth = 8 + c + 6 (+ 2).  (The adds onto 0.0 are exact,
            which covers the third add across the waves: the longest chain has 7 + (c - 1) + 6 + 3 inexact adds.)  bf16 x bf16 products
            are exact in fp32 (16 significant bits), so with u = 2^-24 every result of this order, contracted to FMAs or not, obeys
            |got - z64| <= ((1 + u)^(depth - 1) - 1) sum|h w| <= b = depth u sum|h w|.  With x_noise the gate sees fl32(float(h) * x_noise)
            (one fp32 multiply the kernel states; the reference takes it as the input) and its product with a gate weight is no longer
            exact: one more rounding, depth + 1.  fp32 logit type: |got - z64| <= b.  bf16 logit type: rbf(z64 - b) <= got <= rbf(z64 + b),
            no exclusions.  No bit identity with an emulation is asked (FMA contraction is the compiler's choice); the emulation of the
            summation order (emu_logits) must lie inside the interval, on the CPU.
   exact    small-integer x and gate rows (and x_noise), no norm, fp32 logits: every form equals float64 with no tolerance; permutation-like
            gate rows (a single 1 per row at the chunk, lane-wrap and wave seams of the form) read single elements of the row back.
3. Chain.  For every case the logits the GPU wrote go through oracle.router.route: top_k, sel, expert_mask and the three weight tensors
   equal it for every token; sel is -1 beyond k; masked tokens have an all-zero dynamic mask and the shared columns on.  Planted through the
   gate: identical gate rows (exact ties in every token), a token aligned with one gate row (k = 1), a zero token (uniform: k = n_dyn).
4. Training branch (logits_in + gumbel + rand_u): given the kernel's sel, top_k and round_factor the three weight tensors per element against
   train_weights (the rounds_train logic of test_gpu_bwd_fp64.py with the selection given) in float64; bound 16 x the largest distance of
   the same graph in float32 from float64, per tensor; bf16 adds one bf16 ulp of the reference per rounding of the chain (routing 5:
   softmax, the product with mask_for_one, the sum, the denominator, the quotient; global dynamic 8: these, the softmax over E, its
   dynamic sum, the product; shared 1).  The jitter decision "(max - z) / max(|z|, |max|) > 2 eps" is an integer decision the contract
   takes in T (oracle/router_oracle.c; section 3 pins it bit for bit): far_T restates it in T and both graphs take it as given.
5. Rider: umoe_grouped_gemm with fused_router (SwiGLU, nt = 14) in both rider forms -- the extra z-slice (one group) and the dead
   workgroups of short groups (three groups) -- against umoe_router_fwd and against the same launch without the rider, bit for bit.
6. Tables: umoe_router_dispatch_fwd (dispatch_small_kernel at S <= 16), umoe_dispatch_build, umoe_dispatch_build_aligned and
   umoe_permute_fwd against oracle.router.dispatch.  ld = 11 wherever n_real <= 11 (n_real = 16 needs ld >= 16: ld = 19 there).
7. Guards: NaN in x rows >= S, gate rows >= E, norm weights >= D, x_noise rows >= S, gumbel / rand_u of rounds >= k; every output lies in a
   larger buffer between sentinels (PAD elements on either side) that must stay intact; S = 0 and every refusal write nothing.
The library is driven through its C entry points (unimoe_audio_amd._lib + ctypes): ops.router_fwd and ops.dispatch_build allocate their
outputs themselves, which leaves no place for the sentinels.  ops.pack_rows, ops.pack_gate_up and ops.GroupTable are used as they are.

Without a GPU (test_*_cpu): fp32 emulations of every form's summation order pass every checker at the cases the GPU tests run, the
flagged shares stay under the cap, and each planted error is rejected.

Every GPU test prints its figures under -s ("ROUTER FP64 ..."); test_report prints them once more per launch form.

Measured on an MI355X (the whole file: 126 GPU tests in 2 s).  Per form over its cases -- largest fp32 logits error / b, largest bf16
logits error / (b + ulp / 2), bf16 logits that are not rbf(z64), largest flagged share of h, flagged elements on the alternative chain ("-": no such case in the form):
  router_kernel4<9,2>        0.046   0.991   0   5.8e-4    0        router_kernel4<8,2>        0.069   0.991   2   3.8e-4   0
  fast <9,2> 64 threads      -       0.991   0   4.9e-4    7        fast <8,2> 64 threads      0.025   -       -   -        -
  fast <9,2> 256 threads     0.015   -       -   6.9e-4    0        fast <8,2> 256 threads     -       0.994   0   3.3e-4   0
  loop <9,2> 64 threads      0.081   0.986   0   0         0        loop <8,2> 64 threads      -       0.988   0   -        -
  loop <9,2> 256 threads     -       0.997   0   6.2e-4    0        loop <8,2> 256 threads     0.015   -       -   7.5e-4   0
  loop <0,0> 64 threads      0.061   0.995   0   7.2e-4    0        loop <0,0> 256 threads     0.026   0.998   2   -        -
  router_norm_kernel         -       -       -   2.9e-4    26 (the flagged elements of a row share one rs and go the same way)
  (a bf16 logit reaches its half ulp, hence 0.99; the fp32 sums stay under a tenth of the worst-case bound.)  k = 1 and k = n_dyn occur in
  every form; exact data and the permutation rows bit for bit everywhere; the chain equals the oracle in all 43 cases.
  training branch: fp32 yardstick (largest |float32 graph - float64 graph|) routing 4.6e-8, global / MoE 1.1e-7 at (9, 2) and 4.6e-8 at
  (4, 0); largest error / bound fp32 0.0625 in every tensor (the kernel's worst element is the float32 graph's: k = 1, w / (w + 1e-6)),
  bf16 routing 0.25, global 0.50, MoE 0.24; the jitter gate decided in T never differed from float64 on these inputs.
  rider: 24 launches (D 2048 / 4096, both rider forms, S 1 / 5 / 16, both logit types) bit-identical to umoe_router_fwd, GEMM output unchanged.
This file found no error in the kernels.
"""
import ctypes as C
import functools
import math

import pytest
import torch

from test_gpu_fwd_fp64 import CAP, U, _rejects, check_cands, gen, rbf, same_bits, to_bf, two_way, ulp_bf16

gpu = pytest.mark.gpu

f64, f32, bf16 = torch.float64, torch.float32, torch.bfloat16
NAN = float("nan")
SENT = 7.0                    # sentinel of float buffers
ISENT = 0x5A5A5A5A            # sentinel of integer buffers
PAD = 64                      # sentinel elements on either side of every output
JIT = 0.01
RMS_EPS = 1e-6
EPS32 = float(torch.tensor(RMS_EPS, dtype=f32))
MAXE = 16                     # UMOE_MAXE


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from unimoe_audio_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def stop_after_gpu_error(request):
    """a GPU test that leaves the device in an error state ends the session: nothing more is launched on a card that has faulted"""
    yield
    if request.node.get_closest_marker("gpu") is not None and torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            pytest.exit(f"the GPU reports an error after {request.node.name}: {e}", returncode=3)


class Stats(dict):
    def note(self, name, v):
        self[name] = max(self.get(name, 0.0), float(v))

    def add(self, name, v):
        self[name] = self.get(name, 0) + v

    def merge(self, other):
        for k, v in other.items():
            if k in self.SUMS:
                self.add(k, v)
            else:
                self.note(k, v)

    SUMS = ("h alternative chains taken", "bf16 logits off rbf(z64)", "launches bit-identical", "jitter gates T decides unlike float64 (round 0)",
            "tokens whose selection differs from the float32 restatement")

    def show(self, title):
        print(f"\nROUTER FP64 {title}: " + ", ".join(f"{k} {v:.3g}" for k, v in self.items()))


REPORT = {}                   # form -> Stats, filled by the GPU tests, printed by test_report
SEEN = set()                  # the cases that ran in this session


def report(form):
    return REPORT.setdefault(form, Stats())


def bits(t):
    """the bit pattern of a float tensor as integers (integer tensors as they are)"""
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]) if t.dtype.is_floating_point else t


def rbf64(x):
    """float64 -> the nearest bf16 (ties to even) in one rounding, as float64"""
    ul = ulp_bf16(x)
    return torch.round(x / ul) * ul


# ================================================================================================ 1. the table of launch forms
def form_of(S, D, n_dyn, n_fix, noise=False, logits_in=False, norm_only=False):
    """umoe_router_fwd -> launch_router<ND,NF> -> route_token, restated: the kernel, its instantiation, the branch of route_token and the
    workgroup width"""
    if norm_only:
        return "norm"                                   # router_norm_kernel<9,2,1>, whatever the geometry
    g = "<9,2>" if (n_dyn, n_fix) == (9, 2) else "<8,2>" if (n_dyn, n_fix) == (8, 2) else "<0,0>"
    if g != "<0,0>" and S <= 256 and not logits_in and not noise and D in (2048, 4096):
        return "k4" + g                                 # router_kernel4: one token per 256-thread workgroup
    threads = 64 if S <= 256 else 256                   # router_kernel: one wave per token, 1 or 4 tokens per workgroup
    if logits_in:
        return f"given{g}/{threads}"
    fast = g != "<0,0>" and D <= 2048 and D % 512 == 0 and not noise
    return f"{'fast' if fast else 'loop'}{g}/{threads}"


def chunks_per_lane(form, D):
    if form.startswith("k4") or form == "norm":
        return D // 2048
    return -(-(D // 8) // 64)


def logit_depth(form, D, noise):
    return 8 + chunks_per_lane(form, D) + 6 + (2 if form.startswith("k4") else 0) + (1 if noise else 0)


def h_window(form, D):
    d = 8 * chunks_per_lane(form, D) + 6 + (3 if form.startswith("k4") or form == "norm" else 0)
    return ((d + 2) / 2 + 3) * U


def case(form, S, D, n_dyn=9, n_fix=2, flags="", n_real=None, top_p=0.9):
    """flags: b bf16 logit type, n norm_w, h h_out, a attn_mask, k top_p = 0 with fixed_top_k, x x_noise, t two identical gate rows"""
    assert set(flags) <= set("bnhakxt")
    return dict(form=form, S=S, D=D, n_dyn=n_dyn, n_fix=n_fix, n_real=min(8, n_dyn) if n_real is None else n_real, bf="b" in flags,
                norm="n" in flags, h="h" in flags, am="a" in flags, topk=(2 if n_dyn > 1 else 1) if "k" in flags else 0, noise="x" in flags,
                tie="t" in flags, top_p=0.0 if "k" in flags else top_p)


CASES = [
    # ---- router_kernel4: S <= 256, D 2048 / 4096, shipped geometries, no logits_in, no x_noise
    case("k4<9,2>", 1, 2048, 9, 2, "bnh"), case("k4<9,2>", 16, 2048, 9, 2, "na"), case("k4<9,2>", 255, 2048, 9, 2, "bat"),
    case("k4<9,2>", 256, 2048, 9, 2, "nhk"), case("k4<9,2>", 1, 4096, 9, 2, ""), case("k4<9,2>", 16, 4096, 9, 2, "bnht"),
    case("k4<9,2>", 255, 4096, 9, 2, "nhak"), case("k4<9,2>", 256, 4096, 9, 2, "b"),
    case("k4<8,2>", 1, 2048, 8, 2, "n"), case("k4<8,2>", 16, 2048, 8, 2, "bhk"), case("k4<8,2>", 255, 2048, 8, 2, "nht"),
    case("k4<8,2>", 256, 2048, 8, 2, "ba"), case("k4<8,2>", 1, 4096, 8, 2, "bnh"), case("k4<8,2>", 16, 4096, 8, 2, "a"),
    case("k4<8,2>", 255, 4096, 8, 2, "bn"), case("k4<8,2>", 256, 4096, 8, 2, "nhat"),
    # ---- router_kernel, fast branch: shipped geometries, D 512 .. 2048 in steps of 512, no x_noise
    case("fast<9,2>/64", 1, 512, 9, 2, "bnh"), case("fast<8,2>/64", 256, 512, 8, 2, "at"), case("fast<8,2>/64", 1, 1536, 8, 2, "k"),
    case("fast<9,2>/64", 256, 1536, 9, 2, "bnha"),
    case("fast<9,2>/256", 257, 2048, 9, 2, "nht"), case("fast<8,2>/256", 258, 2048, 8, 2, "bk"), case("fast<8,2>/256", 257, 1024, 8, 2, "bnha"),
    case("fast<9,2>/256", 258, 1024, 9, 2, "a"),
    # ---- router_kernel, loop branch: other D, D = 4096 beyond router_kernel4, any D with x_noise
    case("loop<9,2>/64", 3, 8, 9, 2, "bn"), case("loop<9,2>/64", 5, 256, 9, 2, "nha"), case("loop<8,2>/64", 7, 520, 8, 2, "bhk"),
    case("loop<9,2>/64", 6, 2560, 9, 2, "nkt"), case("loop<9,2>/256", 257, 4096, 9, 2, "bnha"), case("loop<8,2>/256", 257, 4096, 8, 2, "na"),
    case("loop<9,2>/64", 16, 2048, 9, 2, "xa"), case("loop<8,2>/64", 5, 512, 8, 2, "xbk"), case("loop<9,2>/256", 257, 520, 9, 2, "xbt"),
    # ---- generic geometry <0,0>: always the loop branch
    case("loop<0,0>/64", 16, 2048, 6, 1, "bnh"), case("loop<0,0>/256", 257, 256, 6, 1, "ak"), case("loop<0,0>/64", 9, 520, 4, 0, "nhat"),
    case("loop<0,0>/64", 256, 1024, 4, 0, "b"), case("loop<0,0>/64", 5, 4096, 1, 0, "bna"), case("loop<0,0>/64", 12, 8, 1, 0, "hk"),
    case("loop<0,0>/64", 16, 4096, 14, 2, "nh", top_p=0.95), case("loop<0,0>/256", 258, 512, 14, 2, "bxat", top_p=0.95),
    case("k4<9,2>", 16, 2048, 9, 2, "bn", n_real=9), case("loop<9,2>/64", 4, 2560, 9, 2, "ha", n_real=1),
]
NORM_CASES = [(S, D) for D in (2048, 4096) for S in (1, 16, 256)]          # router_norm_kernel (norm_only)
KINDS = ("k4", "fast", "loop<9,2>", "loop<8,2>", "loop<0,0>")


def kind_of(form):
    return next(k for k in KINDS if form.startswith(k))


def seed_of(i):
    return 9100 + 17 * i


@functools.lru_cache(maxsize=None)
def make_case(i, exact=False):
    """host inputs of CASES[i].  Gaussian x (bf16) with a few large-magnitude rows, gate rows scaled to logits of std ~1.2, norm weights
    around 1.  Planted tokens (where S allows): 1 the zero row (uniform gates: k = n_dyn), 2 aligned with gate row 1 (k = 1), 3 and S - 1
    of large / small magnitude.  exact: small integers everywhere, no norm, fp32 logits."""
    c = dict(CASES[i])
    S, D, nd, nf = c["S"], c["D"], c["n_dyn"], c["n_fix"]
    E = nd + nf
    g = gen(seed_of(i) + (1 if exact else 0))
    if exact:
        c.update(norm=False, bf=False)
        x = torch.randint(-4, 5, (S, D), generator=g).float()
        gate = torch.randint(-3, 4, (E, D), generator=g).float()
        noise = torch.randint(1, 3, (S, D), generator=g).float() * torch.where(torch.rand(S, D, generator=g) < 0.5, -1.0, 1.0)
    else:
        scale = 1.2 / math.sqrt(D)
        x = torch.randn(S, D, generator=g)
        gate = torch.randn(E, D, generator=g) * scale
        noise = 1 + 0.02 * (2 * torch.rand(S, D, generator=g) - 1)                 # the reference's jitter: uniform in [1 - eps, 1 + eps]
        if c["tie"] and nd >= 3:
            gate[2] = gate[0]                                                       # exact ties between columns 0 and 2 in every token
        if S > 1:
            x[1] = 0
        if S > 2:
            x[2] = gate[min(1, nd - 1)] / scale * (4 if D < 64 else 1)
        if S > 3:
            x[3] *= 256
        if S > 4:
            x[S - 1] *= 2.0 ** -6
    c["x"], c["gate"] = x.to(bf16), gate.to(bf16)
    c["nw"] = (1 + 0.1 * torch.randn(D, generator=g)).to(bf16) if c["norm"] else None
    c["xn"] = noise.contiguous() if c["noise"] else None
    c["amask"] = (torch.arange(S) % 5 != 4) if c["am"] else None
    assert form_of(S, D, nd, nf, c["noise"]) == c["form"]
    return c


# ================================================================================================ 2. the front end: references, emulations, checkers
def ref_h(x, nw, form, D):
    """-> (chains of rbf(w rbf(x rs)) in float64, flag); x [S, D] bf16, nw [D] bf16"""
    xd = x.to(f64)
    ss = xd.pow(2).sum(-1, keepdim=True)
    rs = 1.0 / torch.sqrt(ss / D + EPS32)
    v = xd * rs
    vs, flag = two_way(v, h_window(form, D) * v.abs())
    return [rbf(nw.to(f64) * t) for t in vs], flag


def emu_h(x, nw, D, bug=None):
    """fp32 emulation of the norm; bug "single rounding": rbf(w x rs) where the kernel rounds twice"""
    xf = x.float()
    ss = (xf * xf).sum(-1, keepdim=True)
    rs = torch.rsqrt(ss / float(D) + torch.tensor(RMS_EPS, dtype=f32))
    v = xf * rs
    if bug == "single rounding":
        return (nw.float() * v).to(bf16)
    return (nw.float() * rbf(v)).to(bf16)


def check_h(name, c, got, stats):
    """h_out of a case: x itself without norm_w, else the candidate rule"""
    if c["nw"] is None:
        same_bits(name + " h (no norm: x itself)", got, c["x"])
        return 0.0
    ys, flag = ref_h(c["x"], c["nw"], c["form"], c["D"])
    try:
        check_cands("h", got, ys, flag, stats)
    except AssertionError as e:
        raise AssertionError(f"{name}: {e}") from None
    share = float(flag.double().mean())
    assert share <= CAP, (name, share)
    return share


def _tree64(v):
    """the butterfly of reduce16_to_lanes over the last axis (64 lanes): offsets 32, 16, 8, 4, 2, 1"""
    n = 64
    while n > 1:
        n //= 2
        v = v[..., :n] + v[..., n:2 * n]
    return v[..., 0]


def emu_logits(h, gate, form, noise=None, bug=None, token=0):
    """fp32 emulation of the summation order of a form (no FMA): h [S, D] bf16 (or fl32 with noise), gate [E, D] bf16 -> [S, E] fp32.
    bugs, planted in one token: "chunk" one 8-element chunk missing, "wave" one wave's partial sum missing (router_kernel4),
    "row" every column read from the neighbouring gate row"""
    S, D = h.shape
    E = gate.shape[0]
    hf = h.float() if noise is None else h.float() * noise
    w = gate.float()
    p = (hf[:, None, :] * w[None]).view(S, E, D // 8, 8)
    d = p[..., 0]
    for j in range(1, 8):
        d = d + p[..., j]
    if bug == "chunk":
        d[token, :, (D // 8) // 2] = 0
    if form.startswith("k4"):
        nch = D // 2048
        q = d.view(S, E, nch, 4, 64)                 # chunk c = (n * 4 + wave) * 64 + lane
        acc = q[:, :, 0]
        for n in range(1, nch):
            acc = acc + q[:, :, n]
        part = _tree64(acc)                          # [S, E, 4]
        if bug == "wave":
            part[token, :, 2] = 0
        out = ((part[..., 0] + part[..., 1]) + part[..., 2]) + part[..., 3]
    else:
        C_ = D // 8
        ncl = -(-C_ // 64)
        q = torch.zeros(S, E, ncl * 64)
        q[..., :C_] = d
        q = q.view(S, E, ncl, 64)                    # chunk c = n * 64 + lane
        acc = q[:, :, 0]
        for n in range(1, ncl):
            acc = acc + q[:, :, n]
        out = _tree64(acc)
    if bug == "row":
        out[token] = out[token].roll(1)
    return out


def ref_logits(h, gate, form, D, noise=None):
    """-> (z64, b) of the docstring"""
    hd = h.to(f64) if noise is None else (h.float() * noise).to(f64)
    wd = gate.to(f64)
    return hd @ wd.T, logit_depth(form, D, noise is not None) * U * (hd.abs() @ wd.abs().T)


def check_logits(name, got, z64, b, is_bf16, stats):
    g = got.to(f64)
    assert g.shape == z64.shape, (name, g.shape, z64.shape)
    assert bool(torch.isfinite(g).all()), f"{name}: non-finite logit"
    if is_bf16:
        lo, hi = rbf64(z64 - b), rbf64(z64 + b)
        bad = (g < lo) | (g > hi)
        stats.add("bf16 logits off rbf(z64)", int((g != rbf64(z64)).sum()))
        stats.note("bf16 logits error / (b + ulp / 2)", float(((g - z64).abs() / (b + ulp_bf16(z64) / 2)).max()))
        if bool(bad.any()):
            i = torch.nonzero(bad)[0].tolist()
            raise AssertionError(f"{name}: {int(bad.sum())} bf16 logits outside [rbf(z64 - b), rbf(z64 + b)], the first at {i}: got {float(g[tuple(i)]):.8g}, "
                                 f"z64 {float(z64[tuple(i)]):.8g}, b {float(b[tuple(i)]):.3g}")
        return
    err = (g - z64).abs()
    ratio = torch.where(b > 0, err / b, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    worst = float(ratio.max())
    stats.note("logits error / b", worst)
    if not worst <= 1.0:
        i = int(ratio.argmax())
        raise AssertionError(f"{name}: logits error / b = {worst:.4g} (error {float(err.flatten()[i]):.4g}, b {float(b.flatten()[i]):.4g}, flat index {i})")


# ================================================================================================ 3. the chain
INTS = ("top_k", "sel", "expert_mask")
WEIGHTS = ("routing_weights", "global_weight", "moe_weight")


def check_chain(name, c, logits, got):
    """every output of the chain against oracle.router.route fed the logits the kernel wrote (logits: bf16 or fp32 tensor, the type T)"""
    from oracle import router as OR
    nd, nf, nr = c["n_dyn"], c["n_fix"], c["n_real"]
    o = OR.route(logits, nd, nr, nf, c["top_p"], c["topk"], JIT, c["amask"])
    for key in INTS:
        assert got[key].shape == o[key].shape and torch.equal(got[key].to(o[key].dtype), o[key]), f"{name}: {key} differs from the oracle"
    for key in WEIGHTS:
        assert bool(torch.isfinite(got[key]).all()), f"{name}: {key} not finite"
        assert torch.equal(got[key], o[key].float()), f"{name}: {key} differs from the oracle"
    k = got["top_k"]
    assert bool(((k >= 1) & (k <= nd)).all()), f"{name}: top_k outside 1 .. n_dyn"
    beyond = torch.arange(nd)[None] >= k[:, None]
    assert bool((got["sel"][beyond] == -1).all()), f"{name}: sel not -1 beyond k"
    assert bool(((got["sel"][~beyond] >= 0) & (got["sel"][~beyond] < nd)).all()), f"{name}: sel outside the dynamic columns"
    m = got["expert_mask"]
    assert bool((m[:, nd:] == 1).all()), f"{name}: a shared column is off"
    if c["amask"] is not None:
        assert bool((m[~c["amask"], :nd] == 0).all()), f"{name}: a masked token keeps a dynamic column"
    live = m[:, :nd].sum(-1)
    ok = live == (k if c["amask"] is None else k * c["amask"].long())
    assert bool(ok.all()), f"{name}: the mask does not hold k columns"
    if nf == 0:
        assert torch.equal(got["global_weight"], got["routing_weights"]), f"{name}: no shared experts, yet global_weight is not routing_weights"
    return k


# ================================================================================================ 4. the training branch
TRAIN_GEOMS = [(9, 8, 2), (4, 4, 0)]
TRAIN_S = (255, 257)
TOP_P = 0.9
ROUNDINGS = dict(routing_weights=5, global_dyn=8, global_shared=1)


def round_t(x, is_bf16):
    return rbf(x) if is_bf16 else x


@functools.lru_cache(maxsize=None)
def make_train(S, is_bf16, n_dyn, n_real, n_fix):
    g = gen(6100 + S + 7 * n_dyn + (1 if is_bf16 else 0))
    E = n_dyn + n_fix
    logits = torch.randn(S, E, generator=g) * 1.2
    logits[30, :n_dyn] = 0.25                                       # all equal: the Top-P count reaches n_dyn
    logits[31, 0] = 9.0                                             # one dominant column: k = 1
    logits = logits.to(bf16 if is_bf16 else f32)
    am = torch.ones(S, dtype=torch.bool)
    am[:17] = False
    return dict(S=S, n_dyn=n_dyn, n_real=n_real, n_fix=n_fix, bf=is_bf16, logits=logits, amask=am, top_p=TOP_P, topk=0,
                gumbel=-torch.log(-torch.log(torch.rand(S, n_dyn, n_dyn, generator=g).clamp(1e-6, 1 - 1e-6))),
                rand_u=torch.rand(S, n_dyn, generator=g))


def factor_values(is_bf16):
    """the two values mask_for_one takes, as the kernel forms them: round_t(0.3333f + 0.6667f) and round_t(0.3333f)"""
    a, b = torch.tensor(0.3333, dtype=f32), torch.tensor(0.6667, dtype=f32)
    return float(round_t(a + b, is_bf16)), float(round_t(a, is_bf16))


def far_T(c, sel, k):
    """[rounds][S, n_dyn] bool: the jitter gate of each round in the arithmetic of the contract (fp32 operations, results rounded to T)"""
    nd, T = c["n_dyn"], c["bf"]
    dyn = c["logits"].float()[:, :nd]
    two_eps = round_t(torch.tensor(2.0 * JIT, dtype=f64).to(f32), T)
    taken = torch.zeros_like(dyn, dtype=torch.bool)
    out = []
    for j in range(int(k.max())):
        thr = dyn.masked_fill(taken, -math.inf).max(-1, keepdim=True)[0]
        d = round_t(thr - dyn, T)
        q = round_t(d / torch.maximum(dyn.abs(), thr.abs()), T)
        out.append(q > two_eps)
        live = (k > j)[:, None]
        taken = taken | (torch.zeros_like(taken).scatter(1, sel[:, j].clamp(min=0).long()[:, None], True) & live)
    return out


def train_weights(c, sel, k, fac, dtype, far=None):
    """the rounds_train logic of test_gpu_bwd_fp64.py with the selection given, followed by the lines of the forward behind it
    (renormalisation, mask, global weights) -> dict of the three weight tensors and the mask, in dtype"""
    nd, nf, nr, S = c["n_dyn"], c["n_fix"], c["n_real"], c["S"]
    far = far_T(c, sel, k) if far is None else far
    z = c["logits"].to(dtype)
    dyn = z[:, :nd]
    taken = torch.zeros((S, nd), dtype=torch.bool)
    w = torch.zeros_like(dyn)
    for j in range(int(k.max())):
        live = (k > j)[:, None]
        gates = dyn.masked_fill(taken | far[j], -math.inf)
        p = torch.softmax(gates, dim=-1)
        sj = sel[:, j].clamp(min=0).long()[:, None]
        mult = p.gather(1, sj) * fac[:, j:j + 1].to(dtype)
        pick = torch.zeros((S, nd), dtype=torch.bool).scatter(1, sj, True) & live
        w = torch.where(pick, mult.expand(S, nd), w)
        taken = taken | pick
    rw = w / (w.sum(-1, keepdim=True) + 1e-6)
    mask = torch.cat([taken.int() * c["amask"][:, None].int(), torch.ones((S, nf), dtype=torch.int32)], -1)
    if nf:
        G = torch.softmax(z.masked_fill(mask == 0, -math.inf), dim=-1)
        gw = torch.cat([rw * G[:, :nd].sum(-1, keepdim=True), G[:, nd:]], -1)
    else:
        gw = rw
    return dict(routing_weights=rw, global_weight=gw, moe_weight=gw[:, :nr] * mask[:, :nr], expert_mask=mask)


def emu_train(c, sel, k, fac):
    """the kernel's chain in fp32 with its roundings to T (the contract's order is not restated: this is the float32 graph + roundings)"""
    T = c["bf"]
    nd, nf, nr, S = c["n_dyn"], c["n_fix"], c["n_real"], c["S"]
    far = far_T(c, sel, k)
    z = c["logits"].float()
    dyn = z[:, :nd]
    taken = torch.zeros((S, nd), dtype=torch.bool)
    w = torch.zeros_like(dyn)
    for j in range(int(k.max())):
        live = (k > j)[:, None]
        p = round_t(torch.softmax(dyn.masked_fill(taken | far[j], -math.inf), dim=-1), T)
        sj = sel[:, j].clamp(min=0).long()[:, None]
        mult = round_t(p.gather(1, sj) * fac[:, j:j + 1], T)
        pick = torch.zeros((S, nd), dtype=torch.bool).scatter(1, sj, True) & live
        w = torch.where(pick, mult.expand(S, nd), w)
        taken = taken | pick
    den = round_t(round_t(w.sum(-1, keepdim=True), T) + 1e-6, T)
    rw = round_t(w / den, T)
    mask = torch.cat([taken.int() * c["amask"][:, None].int(), torch.ones((S, nf), dtype=torch.int32)], -1)
    if nf:
        G = round_t(torch.softmax(z.masked_fill(mask == 0, -math.inf), dim=-1), T)
        gw = torch.cat([round_t(rw * round_t(G[:, :nd].sum(-1, keepdim=True), T), T), G[:, nd:]], -1)
    else:
        gw = rw
    return dict(routing_weights=rw, global_weight=gw, moe_weight=gw[:, :nr] * mask[:, :nr], expert_mask=mask, round_factor=fac)


def check_train(name, c, got, stats):
    """got: top_k, sel, expert_mask, round_factor and the three weight tensors of the training branch (cpu)"""
    nd, T = c["n_dyn"], c["bf"]
    k, sel, fac = got["top_k"], got["sel"], got["round_factor"]
    live = torch.arange(nd)[None] < k[:, None]
    one, third = factor_values(T)
    assert bool(((fac[live] == one) | (fac[live] == third)).all()), f"{name}: round_factor is neither {one} nor {third} on a live round"
    assert bool((fac[~live] == 0).all()), f"{name}: round_factor not 0 beyond k"
    assert bool((sel[~live] == -1).all()) and bool(((sel[live] >= 0) & (sel[live] < nd)).all()), f"{name}: sel"
    times = torch.zeros(sel.shape[0], nd).scatter_add(1, sel.clamp(min=0).long(), live.float())
    assert float(times.max()) <= 1, f"{name}: a column selected twice"
    far = far_T(c, sel, k)
    r64 = train_weights(c, sel, k, fac, f64, far)
    r32 = train_weights(c, sel, k, fac, f32, far)
    assert torch.equal(got["expert_mask"], r64["expert_mask"]), f"{name}: expert_mask differs from the selection"
    d = c["logits"].to(f64)[:, :nd]
    mx = d.max(-1, keepdim=True)[0]
    far64 = (mx - d) / torch.maximum(d.abs(), mx.abs()) > 2 * JIT
    stats.add("jitter gates T decides unlike float64 (round 0)", int((far64 != far[0]).sum()))
    for key in WEIGHTS:
        yard = float((r32[key].to(f64) - r64[key]).abs().max())
        stats.note(f"fp32 yardstick {key}", yard)
        bound = torch.full_like(r64[key], 16 * yard)
        if T:
            n = torch.full_like(r64[key], float(ROUNDINGS["routing_weights"]))
            if key != "routing_weights":
                n[:, :min(nd, n.shape[1])] = ROUNDINGS["global_dyn"] if c["n_fix"] else ROUNDINGS["routing_weights"]
                n[:, nd:] = ROUNDINGS["global_shared"]
            bound = bound + n * ulp_bf16(r64[key])
        g = got[key].to(f64)
        assert bool(torch.isfinite(g).all()), f"{name}: {key} not finite"
        err = (g - r64[key]).abs()
        ratio = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
        worst = float(ratio.max())
        stats.note(f"{key} error / bound", worst)
        if not worst <= 1.0:
            i = torch.nonzero(ratio == ratio.max())[0].tolist()
            raise AssertionError(f"{name}: {key} error / bound = {worst:.4g} at {i} (got {float(g[tuple(i)]):.8g}, float64 {float(r64[key][tuple(i)]):.8g}, "
                                 f"bound {float(bound[tuple(i)]):.3g}, yardstick {yard:.3g})")
        if T:
            assert torch.equal(got[key], rbf(got[key])), f"{name}: {key} is not a bf16 value"


# ================================================================================================ 6. the tables
def table_ld(n_real):
    return 11 if n_real <= 11 else n_real + 3


@functools.lru_cache(maxsize=None)
def make_mask(S, n_real):
    """random mask [S, ld] with a full column (0), an empty column (1) and a column holding only the last token (n_real - 1), as far as n_real
    allows; NaN-free garbage in the columns >= n_real"""
    ld = table_ld(n_real)
    g = gen(4400 + 31 * S + n_real)
    m = (torch.rand(S, ld, generator=g) < 0.45).to(torch.int32)
    m[:, n_real:] = torch.randint(-9, 10, (S, ld - n_real), generator=g).to(torch.int32) * 1237
    if n_real >= 2:
        m[:, 0] = 1
    if n_real >= 3:
        m[:, 1] = 0
    m[:, n_real - 1] = 0
    m[S - 1, n_real - 1] = 1
    return m


def emu_tables(mask, n_real, align):
    """python restatement of dispatch_kernel -> (counts, offsets, slot_token [capacity] with ISENT behind the tables, slot_of)"""
    S = mask.shape[0]
    cap = S * n_real + n_real * (align - 1)
    counts = torch.zeros(n_real, dtype=torch.int32)
    offsets = torch.zeros(n_real + 1, dtype=torch.int32)
    st = torch.full((max(1, cap),), ISENT, dtype=torch.int32)
    so = torch.full((S, n_real), -1, dtype=torch.int32)
    off = 0
    for e in range(n_real):
        tok = torch.nonzero(mask[:, e] != 0).flatten().to(torch.int32)
        n = tok.numel()
        padded = -(-n // align) * align
        counts[e], offsets[e] = n, off
        st[off:off + n] = tok
        st[off + n:off + padded] = 0
        so[tok.long(), e] = torch.arange(off, off + n, dtype=torch.int32)
        off += padded
    offsets[n_real] = off
    return counts, offsets, st, so


def check_tables(name, mask, n_real, align, counts, offsets, slot_token, slot_of):
    """cpu int32 tensors; slot_token is the whole buffer the caller owns: behind offsets[n_real] it must keep the sentinel"""
    from oracle import router as OR
    o = OR.dispatch(mask, n_real)
    assert torch.equal(counts, o["counts"]), f"{name}: counts (unpadded) differ from the oracle"
    off = 0
    want_of = torch.full_like(o["slot_of"], -1)
    for e in range(n_real):
        n = int(o["counts"][e])
        assert int(offsets[e]) % align == 0, f"{name}: offsets[{e}] = {int(offsets[e])} is no multiple of {align}"
        assert int(offsets[e]) == off, f"{name}: offsets[{e}] = {int(offsets[e])}, expected {off}"
        o0 = int(o["offsets"][e])
        assert torch.equal(slot_token[off:off + n], o["slot_token"][o0:o0 + n]), f"{name}: live slots of expert {e} differ from the oracle"
        padded = -(-n // align) * align
        assert bool((slot_token[off + n:off + padded] == 0).all()), f"{name}: a padding slot of expert {e} is not 0"
        on = mask[:, e] != 0
        want_of[on, e] = o["slot_of"][on, e] + (off - o0)
        off += padded
    assert int(offsets[n_real]) == off, f"{name}: offsets[n_real] = {int(offsets[n_real])}, the padded total is {off}"
    assert bool((slot_token[off:] == ISENT).all()), f"{name}: slot_token written behind the padded total"
    assert bool(((slot_of == -1) == (mask[:, :n_real] == 0)).all()), f"{name}: slot_of is not -1 exactly where the mask is 0"
    assert torch.equal(slot_of, want_of), f"{name}: slot_of differs from the oracle"


# ================================================================================================ without a GPU
def test_table_cpu():
    """every case reaches the form it names (form_of restates the launcher); the issue's shapes and options are all there"""
    by_kind = {}
    for i, c in enumerate(CASES):
        assert form_of(c["S"], c["D"], c["n_dyn"], c["n_fix"], c["noise"]) == c["form"], (i, c)
        assert c["S"] <= 300 and c["D"] <= 4096 and c["D"] % 8 == 0 and c["n_dyn"] + c["n_fix"] <= MAXE and c["n_real"] <= c["n_dyn"]
        assert not (c["noise"] and (c["norm"] or c["h"]))
        by_kind.setdefault(kind_of(c["form"]), []).append(c)
    have = {(c["form"], c["S"], c["D"]) for c in CASES}
    for g in ("<9,2>", "<8,2>"):
        for S in (1, 16, 255, 256):
            for D in (2048, 4096):
                assert ("k4" + g, S, D) in have
    fast = {(c["S"], c["D"], c["form"].split("/")[1]) for c in by_kind["fast"]}
    assert {(1, 512, "64"), (256, 512, "64"), (1, 1536, "64"), (256, 1536, "64"), (257, 2048, "256"), (258, 2048, "256"), (257, 1024, "256"),
            (258, 1024, "256")} <= fast
    loop = [c for k in KINDS[2:] for c in by_kind[k]]
    assert {8, 256, 520, 2560} <= {c["D"] for c in loop if c["S"] <= 16 and not c["noise"]}
    assert any(c["D"] == 4096 and c["S"] == 257 for c in loop)
    noisy = [c for c in CASES if c["noise"]]
    assert any(c["D"] == 2048 and c["S"] <= 256 for c in noisy) and any(c["D"] == 512 for c in noisy) and all(c["form"].startswith("loop") for c in noisy)
    geoms = {(c["n_dyn"], c["n_fix"]) for c in by_kind["loop<0,0>"]}
    assert geoms == {(6, 1), (4, 0), (1, 0), (14, 2)} and all(c["form"].startswith("loop<0,0>") for c in by_kind["loop<0,0>"])
    assert {c["n_real"] for c in CASES if (c["n_dyn"], c["n_fix"]) == (9, 2)} >= {9, 8, 1}
    for kind, cs in by_kind.items():
        for key in ("bf", "norm", "h", "am"):
            assert {bool(c[key]) for c in cs} == {True, False}, (kind, key)
        assert any(c["topk"] and c["top_p"] == 0.0 for c in cs) and any(not c["topk"] for c in cs), kind
    assert set(by_kind) == set(KINDS)
    for S, D in NORM_CASES:
        assert form_of(S, D, 9, 2, norm_only=True) == "norm"
    # the forms the other entry points reach
    assert form_of(257, 0, 9, 2, logits_in=True) == "given<9,2>/256" and form_of(255, 0, 4, 0, logits_in=True) == "given<0,0>/64"
    assert form_of(257, 2048, 9, 2) == "fast<9,2>/256" and form_of(256, 2048, 9, 2) == "k4<9,2>"           # the first S that leaves router_kernel4


def test_helpers_cpu():
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -40, -3.0, 0.0], dtype=f64)
    assert rbf64(x).tolist() == [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -3.0, 0.0]          # ties to even; one rounding from float64
    y = torch.randn(4096, generator=gen(1), dtype=f64)
    assert torch.equal(rbf64(y.float().to(f64)), rbf(y.float()).to(f64))
    assert factor_values(False) == (1.0, float(torch.tensor(0.3333, dtype=f32))) and factor_values(True)[1] == float(rbf(torch.tensor(0.3333)))
    v = torch.randn(3, 64, generator=gen(2))
    assert torch.allclose(_tree64(v.clone()), v.sum(-1), atol=1e-5)


def emu_case(i, exact=False, bug=None):
    """(h, logits in T, chain outputs) of a case as an fp32 emulation of its form would leave them"""
    from oracle import router as OR
    c = make_case(i, exact)
    h = emu_h(c["x"], c["nw"], c["D"], bug) if c["nw"] is not None else c["x"]
    z = emu_logits(h, c["gate"], c["form"], c["xn"], bug, token=min(5, c["S"] - 1))
    lg = z.to(bf16) if c["bf"] else z
    o = OR.route(lg, c["n_dyn"], c["n_real"], c["n_fix"], c["top_p"], c["topk"], JIT, c["amask"])
    got = {k: o[k].clone() for k in INTS}
    got.update({k: o[k].float() for k in WEIGHTS})
    return c, h, lg, got


def front_checks(name, c, h, lg, stats):
    share = check_h(name, c, h, stats)
    z64, b = ref_logits(h, c["gate"], c["form"], c["D"], c["xn"])
    check_logits(name, lg, z64, b, c["bf"], stats)
    return share


@pytest.mark.parametrize("kind", KINDS)
def test_front_end_checkers_cpu(kind):
    """the emulation of every case passes h, logits and chain checks (Gaussian and exact data), the flagged share of h stays under the cap,
    and the planted front-end errors are rejected"""
    st = Stats()
    idx = [i for i, c in enumerate(CASES) if kind_of(c["form"]) == kind]
    for i in idx:
        c, h, lg, got = emu_case(i)
        front_checks(f"case {i}", c, h, lg, st)
        check_chain(f"case {i}", c, lg, got)
        c, h, lg, got = emu_case(i, exact=True)
        z64, _ = ref_logits(h, c["gate"], c["form"], c["D"], c["xn"])
        assert torch.equal(lg.to(f64), z64), f"case {i}: exact data"
    st.show(f"emulation, {kind}")
    big = [i for i in idx if CASES[i]["S"] >= 5 and CASES[i]["D"] >= 256]
    for bf in (False, True):
        sub = [i for i in big if CASES[i]["bf"] == bf]
        assert sub, (kind, bf)
        i = sub[0]
        for bug in ("chunk", "row") + (("wave",) if kind == "k4" else ()):
            c, h, lg, _ = emu_case(i, bug=bug)
            z64, b = ref_logits(h, c["gate"], c["form"], c["D"], c["xn"])
            _rejects(lambda: check_logits(f"case {i} {bug}", lg, z64, b, c["bf"], Stats()))
    normed = [i for i in big if CASES[i]["norm"]]
    c = make_case(normed[0])
    _rejects(lambda: check_h("single rounding", c, emu_h(c["x"], c["nw"], c["D"], "single rounding"), Stats()))
    bad = emu_h(c["x"], c["nw"], c["D"]).clone()
    bad[0, 3] = bad[0, 4] + 1
    _rejects(lambda: check_h("one element", c, bad, Stats()))


def test_exact_permutation_cpu():
    """the permutation-like gate rows name the seams of every form; the emulation reads the named elements back"""
    for form, S, D, nd, nf in PERM_CASES:
        x, gate, pos = make_perm(form, S, D, nd + nf)
        assert len(set(pos)) == len(pos) and max(pos) < D
        z = emu_logits(x, gate, form)
        assert torch.equal(z, x.float()[:, pos])
        cpl = chunks_per_lane(form, D)
        assert {0, 7, 8, D - 1} <= set(pos) or D == 8
        if D >= 1024:
            assert 511 in pos and 512 in pos                      # lane 63 -> the next wave (router_kernel4) or the lane's next chunk
        if cpl > 1 and form.startswith("k4"):
            assert 2047 in pos and 2048 in pos                    # the second chunk of wave 0
        if D > 8:
            assert not torch.equal(emu_logits(x.roll(8, 1), gate, form), x.float()[:, pos])          # every chunk read from its neighbour


def test_chain_checker_cpu():
    """planted chain errors: sel left unfilled beyond k, two equal-logit experts swapped in order, a weight from the neighbour, a masked
    token that keeps a column"""
    i = next(i for i, c in enumerate(CASES) if c["tie"] and c["S"] >= 255 and not c["topk"] and not c["am"] and c["n_dyn"] >= 3)
    c, h, lg, got = emu_case(i)
    check_chain("emulation", c, lg, got)
    k = got["top_k"]
    bad = {key: v.clone() for key, v in got.items()}
    s = int(torch.nonzero(k < c["n_dyn"])[0])
    bad["sel"][s, int(k[s]):] = 0
    _rejects(lambda: check_chain("sel unfilled", c, lg, bad))
    sel = got["sel"]
    both = torch.nonzero(((sel == 0).any(-1)) & ((sel == 2).any(-1))).flatten()
    assert both.numel() > 0, "no token selects both tied columns"
    s = int(both[0])
    j0, j2 = int(torch.nonzero(sel[s] == 0)[0]), int(torch.nonzero(sel[s] == 2)[0])
    assert j0 < j2 and float(lg[s, 0]) == float(lg[s, 2])                     # lowest index first among equals
    bad = {key: v.clone() for key, v in got.items()}
    bad["sel"][s, j0], bad["sel"][s, j2] = 2, 0
    _rejects(lambda: check_chain("tie order", c, lg, bad))
    for key in WEIGHTS:
        bad = {kk: v.clone() for kk, v in got.items()}
        bad[key][5] = bad[key][6] + 2.0 ** -20
        _rejects(lambda: check_chain(key, c, lg, bad))
    j = next(j for j, q in enumerate(CASES) if q["am"] and q["S"] >= 16)
    c, h, lg, got = emu_case(j)
    bad = {key: v.clone() for key, v in got.items()}
    bad["expert_mask"][4, int(got["sel"][4, 0])] = 1
    _rejects(lambda: check_chain("masked token", c, lg, bad))


def train_decisions(c):
    """(sel, top_k, round_factor) as a forward would hand them over: the float32 graph's own decisions"""
    from oracle import router as OR
    nd, T = c["n_dyn"], c["bf"]
    k = OR.route(c["logits"], nd, c["n_real"], c["n_fix"], TOP_P, 0, JIT, c["amask"])["top_k"]
    one, third = factor_values(T)
    S = c["S"]
    dyn = c["logits"].float()[:, :nd]
    sel = torch.full((S, nd), -1, dtype=torch.int32)
    fac = torch.zeros(S, nd)
    taken = torch.zeros((S, nd), dtype=torch.bool)
    two_eps = round_t(torch.tensor(2.0 * JIT, dtype=f64).to(f32), T)
    for j in range(int(k.max())):
        live = k > j
        masked = dyn.masked_fill(taken, -math.inf)
        thr = masked.max(-1, keepdim=True)[0]
        q = round_t(round_t(thr - dyn, T) / torch.maximum(dyn.abs(), thr.abs()), T)
        gates = masked.masked_fill(q > two_eps, -math.inf)
        sj = (gates + c["gumbel"][:, j]).max(-1)[1]
        p = round_t(torch.softmax(gates, -1), T)
        is_one = (sj == p.max(-1)[1]) | (c["rand_u"][:, j] > 0.75)
        sel[:, j] = torch.where(live, sj.int(), sel[:, j])
        fac[:, j] = torch.where(live, torch.where(is_one, one, third), fac[:, j])
        taken |= torch.zeros_like(taken).scatter(1, sj[:, None], True) & live[:, None]
    return sel, k, fac


@pytest.mark.parametrize("is_bf16", [False, True])
def test_train_checker_cpu(is_bf16):
    st = Stats()
    for nd, nr, nf in TRAIN_GEOMS:
        c = make_train(257, is_bf16, nd, nr, nf)
        sel, k, fac = train_decisions(c)
        assert int(k.min()) == 1 and int(k.max()) == nd and bool((fac == factor_values(is_bf16)[1]).any())
        got = emu_train(c, sel, k, fac)
        got.update(top_k=k, sel=sel)
        check_train("emulation", c, got, st)
        for key in WEIGHTS:
            bad = dict(got)
            bad[key] = got[key].clone()
            bad[key][100] = got[key][101]
            _rejects(lambda: check_train(key, c, bad, Stats()))
        bad = dict(got)
        bad["round_factor"] = fac.clone()
        s = int(torch.nonzero(k >= 2)[0])
        bad["round_factor"][s, 0] = 0.5
        _rejects(lambda: check_train("factor", c, bad, Stats()))
        bad["round_factor"] = fac.clone()
        s = int(torch.nonzero(k < nd)[0])
        bad["round_factor"][s, nd - 1] = 1.0
        _rejects(lambda: check_train("factor beyond k", c, bad, Stats()))
        flip = fac.clone()                                   # every weight computed with mask_for_one = 1
        flip[fac > 0] = factor_values(is_bf16)[0]
        wrong = emu_train(c, sel, k, flip)
        wrong.update(top_k=k, sel=sel, round_factor=fac)
        _rejects(lambda: check_train("mask_for_one ignored", c, wrong, Stats()))
    st.show(f"training-branch emulation, {'bf16' if is_bf16 else 'fp32'}")


def test_tables_checker_cpu():
    for S, nr, align in [(1, 8, 1), (16, 8, 1), (17, 1, 1), (257, 8, 8), (513, 16, 256), (255, 8, 256)]:
        m = make_mask(S, nr)
        cnt, off, st, so = emu_tables(m, nr, align)
        check_tables("emulation", m, nr, align, cnt, off, st, so)
        if nr >= 3:
            assert int(cnt[0]) == S and int(cnt[1]) == 0 and int(cnt[nr - 1]) == 1
        bad = off.clone()
        bad[nr // 2 + (1 if nr > 1 else 0)] += 1
        _rejects(lambda: check_tables("offset off by one", m, nr, align, cnt, bad, st, so))
        s, e = [int(v) for v in torch.nonzero(m[:, :nr] == 0)[0]] if bool((m[:, :nr] == 0).any()) else (None, None)
        if s is not None:
            bad = so.clone()
            bad[s, e] = 0
            _rejects(lambda: check_tables("slot_of 0", m, nr, align, cnt, off, st, bad))
        bad = st.clone()
        bad[int(off[nr])] = 0
        _rejects(lambda: check_tables("written behind the total", m, nr, align, cnt, off, bad, so))
        if align > 1 and int(cnt[nr - 1]) % align:
            bad = st.clone()
            bad[int(off[nr - 1]) + int(cnt[nr - 1])] = 3
            _rejects(lambda: check_tables("padding slot", m, nr, align, cnt, off, bad, so))


# ================================================================================================ the GPU side: buffers and launches
class Guarded:
    """outputs inside larger buffers: PAD sentinel elements on either side of each"""

    def __init__(self, dev):
        self.dev, self.bufs = dev, {}

    def new(self, name, shape, dtype):
        n = 1
        for d in shape:
            n *= d
        fill = SENT if dtype.is_floating_point else ISENT
        buf = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=self.dev)
        self.bufs[name] = (buf, n, tuple(shape), fill)
        return buf[PAD:PAD + n]

    def ptr(self, name):
        return self.bufs[name][0][PAD:].data_ptr()

    def get(self, name):
        buf, n, shape, _ = self.bufs[name]
        return buf[PAD:PAD + n].view(shape).cpu().clone()

    def pads_intact(self, what=""):
        for name, (buf, n, _, fill) in self.bufs.items():
            b = buf.cpu()
            assert bool((b[:PAD] == fill).all()) and bool((b[PAD + n:] == fill).all()), f"{what}: sentinel around {name} overwritten"

    def untouched(self, what=""):
        for name, (buf, _, _, fill) in self.bufs.items():
            assert bool((buf.cpu() == fill).all()), f"{what}: {name} was written"


def nan_tail(t, dev, tail):
    """t on the device, followed by `tail` rows (elements of a vector) of NaN"""
    tail = max(tail, 1 if t.shape[0] == 0 else 0)               # never an empty allocation: its pointer would be NULL
    buf = torch.full((t.shape[0] + tail,) + tuple(t.shape[1:]), NAN if t.dtype.is_floating_point else 0, dtype=t.dtype, device=dev)
    buf[:t.shape[0]] = t.to(dev)
    return buf


OUT_FIELDS = dict(logits="logits_out", top_k="top_k", sel="sel", expert_mask="expert_mask", routing_weights="routing_w", global_weight="global_w",
                  moe_weight="moe_w", h="h_out", round_factor="round_factor")


def prep(dev, c, logits_in=None, gumbel=None, rand_u=None, want=None, norm_only=False, over=None, drop=()):
    """RouterArgs of a case (inputs with NaN behind them, outputs guarded) -> (args, Guarded, keep-alive list).  over: raw field values put
    in last (refusals); drop: inputs / outputs left NULL; S_alloc sizes the outputs when S itself is bad"""
    from unimoe_audio_amd import _lib as L
    S, D, nd, nf, nr = c["S"], c.get("D", 0), c["n_dyn"], c["n_fix"], c["n_real"]
    Sa, E = max(c.get("S_alloc", S), 1), nd + nf
    G, keep = Guarded(dev), []
    is_bf = (logits_in.dtype == bf16) if logits_in is not None else c["bf"]
    shapes = dict(logits=((Sa, E), bf16 if is_bf else f32), top_k=((Sa,), torch.int64), sel=((Sa, nd), torch.int32), expert_mask=((Sa, E), torch.int32),
                  routing_weights=((Sa, nd), f32), global_weight=((Sa, E), f32), moe_weight=((Sa, max(nr, 1)), f32))
    if want is None:
        want = list(shapes) + (["h"] if c.get("h") else []) + (["round_factor"] if gumbel is not None else [])
    if "h" in want:
        shapes["h"] = ((Sa, max(D, 8)), bf16)
    if "round_factor" in want:
        shapes["round_factor"] = ((Sa, nd), f32)
    a = L.RouterArgs(S=S, D=D, n_dyn=nd, n_real=nr, n_fix=nf, logits_bf16=int(is_bf), top_p=c["top_p"], fixed_top_k=c["topk"], jitter_eps=JIT,
                     rms_eps=RMS_EPS, norm_only=int(norm_only))
    for name in want:
        if name in drop:
            continue
        shape, dt = shapes[name]
        G.new(name, shape, dt)
        setattr(a, OUT_FIELDS[name], G.ptr(name))

    def put(field, t, tail):
        if t is None or field in drop:
            return
        keep.append(nan_tail(t, dev, tail))
        setattr(a, field, keep[-1].data_ptr())
    if logits_in is not None:
        put("logits_in", logits_in, 0)
    else:
        put("x", c.get("x"), 2)
        put("gate_w", c.get("gate"), 2)
        put("norm_w", c.get("nw"), 8)
        put("x_noise", c.get("xn"), 2)
    if c.get("amask") is not None:
        keep.append(c["amask"].to(torch.uint8).to(dev))
        a.attn_mask = keep[-1].data_ptr()
    put("gumbel", gumbel, 0)
    put("rand_u", rand_u, 0)
    for k_, v in (over or {}).items():
        setattr(a, k_, v)
    return a, G, keep


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def launch(dev, c, **kw):
    """umoe_router_fwd on a case -> (rc, outputs on the cpu shaped [S, ...], Guarded)"""
    from unimoe_audio_amd import _lib as L
    a, G, keep = prep(dev, c, **kw)
    rc = L.lib().umoe_router_fwd(C.byref(a), stream())
    torch.cuda.synchronize()
    G.pads_intact("umoe_router_fwd")
    S = c["S"]
    out = {name: G.get(name)[:S] for name in G.bufs} if rc == 0 and S > 0 else {}
    if "moe_weight" in out:
        out["moe_weight"] = out["moe_weight"][:, :c["n_real"]]
    if "h" in out:
        out["h"] = out["h"][:, :c["D"]]
    return rc, out, G


def run_case(dev, c, name):
    """the launch of a case; without h_out a second launch with h_out reads h back (every other output must not change)"""
    rc, out, _ = launch(dev, c)
    assert rc == 0, name
    if c["h"] or c["nw"] is None:
        h = out["h"] if c["h"] else c["x"]
    else:
        rc, out2, _ = launch(dev, dict(c, h=True))
        assert rc == 0
        for key in out:
            assert torch.equal(bits(out[key]), bits(out2[key])), f"{name}: {key} changes with h_out"
        h = out2["h"]
    return out, h


# ================================================================================================ GPU tests
@gpu
@pytest.mark.parametrize("i", range(len(CASES)))
def test_router_case_vs_fp64(dev, i):
    """sections 2 (Gaussian data), 3 and 7 on case i"""
    c = make_case(i)
    name = f"case {i} {c['form']} S={c['S']} D={c['D']}"
    st = Stats()
    out, h = run_case(dev, c, name)
    front_checks(name, c, h, out["logits"], st)
    k = check_chain(name, c, out["logits"], out)
    if not c["topk"] and c["S"] >= 3:
        st["k = 1 seen"] = max(st.get("k = 1 seen", 0), int(bool((k == 1).any())))
        st["k = n_dyn seen"] = max(st.get("k = n_dyn seen", 0), int(bool((k == c["n_dyn"]).any())))
    if c["tie"] and c["n_dyn"] >= 3:
        lg = out["logits"]
        assert torch.equal(bits(lg[:, 0]), bits(lg[:, 2])), f"{name}: identical gate rows, different logits"
    SEEN.add(i)
    st.show(name)
    report(c["form"]).merge(st)


@gpu
@pytest.mark.parametrize("i", range(len(CASES)))
def test_router_exact_data(dev, i):
    """small-integer x, gate rows and x_noise, no norm, fp32 logits: equal to float64, no tolerance; the chain as everywhere"""
    c = make_case(i, exact=True)
    name = f"exact case {i} {c['form']}"
    out, h = run_case(dev, c, name)
    z64, _ = ref_logits(h, c["gate"], c["form"], c["D"], c["xn"])
    assert torch.equal(out["logits"].to(f64), z64), f"{name}: logits differ from float64 on exact data"
    if c["h"]:
        same_bits(name + " h", out["h"], c["x"])
    check_chain(name, c, out["logits"], out)


def seams(form, D):
    """element positions at the chunk, lane-wrap and wave seams of a form, the first E taken"""
    cand = [0, 7, 8, D - 1, 511, 512, 2047, 2048, D - 8, 15, 16, 1023, 1024, 1535, 1536, 2559, 2560, 3071, 3072, 519, 504, D // 2, D // 2 - 1, 3, 4, 5]
    out = []
    for p in cand:
        if 0 <= p < D and p not in out:
            out.append(p)
    return out


PERM_CASES = [("k4<9,2>", 16, 2048, 9, 2), ("k4<8,2>", 5, 4096, 8, 2), ("fast<9,2>/64", 7, 1536, 9, 2), ("fast<8,2>/256", 257, 2048, 8, 2),
              ("loop<9,2>/64", 5, 520, 9, 2), ("loop<8,2>/64", 3, 2560, 8, 2), ("loop<9,2>/256", 257, 4096, 9, 2), ("loop<0,0>/64", 16, 2048, 14, 2),
              ("loop<0,0>/64", 4, 8, 4, 0)]


@functools.lru_cache(maxsize=None)
def make_perm(form, S, D, E):
    pos = seams(form, D)[:E]
    assert len(pos) == E, (form, D, E)
    i, s = torch.arange(D)[None], torch.arange(S)[:, None]
    x = (((i * 7 + s * 13) % 251) - 125).float().to(bf16)
    gate = torch.zeros(E, D)
    gate[torch.arange(E), torch.tensor(pos)] = 1
    return x, gate.to(bf16), pos


@gpu
@pytest.mark.parametrize("form,S,D,nd,nf", PERM_CASES)
def test_router_permutation_rows(dev, form, S, D, nd, nf):
    """a single 1 per gate row: logit e of token s IS x[s, pos[e]]"""
    assert form_of(S, D, nd, nf) == form
    x, gate, pos = make_perm(form, S, D, nd + nf)
    c = dict(form=form, S=S, D=D, n_dyn=nd, n_fix=nf, n_real=min(8, nd), bf=False, h=False, x=x, gate=gate, nw=None, xn=None, amask=None,
             top_p=0.9, topk=0)
    rc, out, _ = launch(dev, c)
    assert rc == 0
    want = x.float()[:, pos]
    if not torch.equal(out["logits"], want):
        bad = torch.nonzero(out["logits"] != want)[0].tolist()
        raise AssertionError(f"{form}: logit {bad} reads {float(out['logits'][tuple(bad)])}, element {pos[bad[1]]} of the row holds {float(want[tuple(bad)])}")
    check_chain(form, c, out["logits"], out)


def host_unpack(t, tiles, K):
    """operand-order tiles of ops.pack_rows -> rows [tiles * 16, K]"""
    return t[:tiles * 16 * K].view(tiles, K // 32, 4, 16, 8).permute(0, 3, 2, 1, 4).reshape(tiles * 16, K)


@gpu
@pytest.mark.parametrize("S,D", NORM_CASES)
def test_router_norm_only_vs_fp64(dev, S, D):
    """router_norm_kernel against float64 (candidate rule), and bit-identical to the h_out of the full router_kernel4 body and to
    ops.pack_rows(norm_w=...)"""
    from unimoe_audio_amd import ops
    g = gen(7700 + S + D)
    x = torch.randn(S, D, generator=g)
    if S > 3:
        x[1] = 0
        x[2] *= 300
        x[3] *= 2.0 ** -9
    x = x.to(bf16)
    nw = (1 + 0.1 * torch.randn(D, generator=g)).to(bf16)
    gate = (torch.randn(11, D, generator=g) * 1.2 / math.sqrt(D)).to(bf16)
    c = dict(form="norm", S=S, D=D, n_dyn=9, n_fix=2, n_real=8, bf=True, h=True, x=x, gate=gate, nw=nw, xn=None, amask=None, top_p=0.9, topk=0)
    st = Stats()
    rc, out, G = launch(dev, c, want=["h"], norm_only=True)
    assert rc == 0
    check_h(f"norm_only S={S} D={D}", c, out["h"], st)
    if S > 3:
        assert bool((out["h"][1].float() == 0).all()), "the zero row is not exactly zero"
    rc, full, _ = launch(dev, dict(c, form="k4<9,2>"))
    assert rc == 0
    same_bits("h_out of router_kernel4 against norm_only", full["h"], out["h"])
    xd = nan_tail(x, dev, 2)
    tiles = (S + 15) // 16
    packed = torch.full((tiles * 16 * D + 64,), SENT, dtype=bf16, device=dev)
    ops.pack_rows(xd[:S], norm_w=nan_tail(nw, dev, 8)[:D], rms_eps=RMS_EPS, out=packed)
    rows = host_unpack(packed.cpu(), tiles, D)
    same_bits("ops.pack_rows(norm_w) against norm_only", rows[:S], out["h"])
    assert bool((rows[S:].float() == 0).all()) and bool((packed.cpu()[tiles * 16 * D:].float() == SENT).all())
    st.show(f"norm_only S={S} D={D}")
    report("norm").merge(st)


@gpu
@pytest.mark.parametrize("is_bf16", [False, True])
@pytest.mark.parametrize("n_dyn,n_real,n_fix", TRAIN_GEOMS)
def test_router_train_weights_vs_fp64(dev, is_bf16, n_dyn, n_real, n_fix):
    """section 4; gumbel and rand_u hold NaN in the rounds >= k"""
    from oracle import router as OR
    st = Stats()
    for S in TRAIN_S:
        c = make_train(S, is_bf16, n_dyn, n_real, n_fix)
        k0 = OR.route(c["logits"], n_dyn, n_real, n_fix, TOP_P, 0, JIT, c["amask"])["top_k"]
        dead = torch.arange(n_dyn)[None] >= k0[:, None]
        gum, ru = c["gumbel"].clone(), c["rand_u"].clone()
        gum[dead] = NAN
        ru[dead] = NAN
        rc, out, _ = launch(dev, c, logits_in=c["logits"], gumbel=gum, rand_u=ru)
        assert rc == 0
        name = f"train S={S} {form_of(S, 0, n_dyn, n_fix, logits_in=True)}"
        assert torch.equal(out["top_k"], k0), f"{name}: top_k differs from the oracle"
        assert int(k0.min()) == 1 and int(k0.max()) == n_dyn
        same_bits(name + " logits_out", out["logits"], c["logits"])
        check_train(name, c, out, st)
        sel_e = train_decisions(c)[0]
        st.add("tokens whose selection differs from the float32 restatement", int((sel_e != out["sel"]).any(-1).sum()))
    st.show(f"training branch {'bf16' if is_bf16 else 'fp32'} {n_dyn}/{n_real}/{n_fix}")
    report(f"train {'bf16' if is_bf16 else 'fp32'} ({n_dyn},{n_fix})").merge(st)


# ------------------------------------------------------------------------------------------------ 5. the rider
RIDER_NB = 212          # 16 n_blocks columns x 2: I = 1696; ceil(212 / 14) = 16 workgroups, the last one of 2 blocks
EPI_SWIGLU = 2


@functools.lru_cache(maxsize=None)
def rider_weights(D, dev_str):
    from unimoe_audio_amd import ops
    dev = torch.device(dev_str)
    g = torch.Generator(device=dev).manual_seed(77 + D)
    ws = []
    for nb in (RIDER_NB, 4, 4):
        wg = (torch.randn(8 * nb, D, generator=g, device=dev) * 0.02).to(bf16)
        wu = (torch.randn(8 * nb, D, generator=g, device=dev) * 0.02).to(bf16)
        ws.append(ops.pack_gate_up(wg, wu))
    a = torch.randn(16, D, generator=g, device=dev).to(bf16)
    return ws, a


def rider_launch(dev, D, n_groups, rows, router_args):
    """the gate/up launch (SwiGLU, nt = 14, plain prologue, host descriptors) -> (rc, the whole output buffer on the cpu)"""
    from unimoe_audio_amd import _lib as L
    from unimoe_audio_amd import ops
    ws, a = rider_weights(D, str(dev))
    nbs = (RIDER_NB, 4, 4)[:n_groups]
    groups = [dict(w=ws[i], n_blocks=nbs[i], k=D, static_count=rows if i == 0 else min(rows, 5), a_row_base=0, out_row_base=16 * i) for i in range(n_groups)]
    tab = ops.GroupTable(groups, dev)
    ldo = 8 * RIDER_NB + 8
    out = torch.full((16 * n_groups + 2, ldo), SENT, dtype=bf16, device=dev)
    args = L.GemmArgs(groups=tab.dev.data_ptr(), num_groups=n_groups, max_rows=rows, max_n_blocks=RIDER_NB, max_k=D, a=a.data_ptr(), lda=D,
                      out=out.data_ptr(), ldo=ldo, n_valid=8 * RIDER_NB, prologue=0, epilogue=EPI_SWIGLU, nt=14, waves=0, ksplit=0, part_stride=0,
                      groups_host=C.cast(tab.host, C.c_void_p), cache_policy=0)
    if router_args is not None:
        args.fused_router = C.cast(C.pointer(router_args), C.c_void_p)
    rc = L.lib().umoe_grouped_gemm(C.byref(args), stream())
    torch.cuda.synchronize()
    return rc, out.cpu()


@gpu
@pytest.mark.parametrize("n_groups", [1, 3])
@pytest.mark.parametrize("D", [2048, 4096])
def test_router_rider_equals_router_fwd(dev, D, n_groups, monkeypatch):
    """n_groups 1: no dead workgroup, the riders are an extra z-slice; 3: 30 dead workgroups of the two short groups carry the tokens"""
    monkeypatch.delenv("UMOE_RIDER_MODE", raising=False)
    assert -(-RIDER_NB // 14) == 16 and (n_groups - 1) * (16 - 1) >= 16 * (n_groups > 1)
    st = report("rider")
    for S in (1, 5, 16):
        for is_bf in (False, True):
            g = gen(8800 + S + D + is_bf)
            x = torch.randn(S, D, generator=g).to(bf16)
            c = dict(form="k4<9,2>", S=S, D=D, n_dyn=9, n_fix=2, n_real=8, bf=is_bf, h=(S == 5), x=x, top_p=0.9, topk=0, xn=None,
                     gate=(torch.randn(11, D, generator=g) * 1.2 / math.sqrt(D)).to(bf16), nw=(1 + 0.1 * torch.randn(D, generator=g)).to(bf16) if S != 1 else None,
                     amask=(torch.arange(S) % 3 != 1) if S == 16 else None)
            name = f"rider D={D} groups={n_groups} S={S} {'bf16' if is_bf else 'fp32'}"
            rc, alone, _ = launch(dev, c)
            assert rc == 0
            rc, plain = rider_launch(dev, D, n_groups, 16, None)
            assert rc == 0
            a, G, keep = prep(dev, c)
            rc, ridden = rider_launch(dev, D, n_groups, 16, a)
            assert rc == 0, name
            G.pads_intact(name)
            for key in alone:
                got = G.get(key)[:S]
                got = got[:, :8] if key == "moe_weight" else got
                assert torch.equal(bits(got), bits(alone[key])), f"{name}: {key} of the rider differs from umoe_router_fwd"
            assert torch.equal(bits(ridden), bits(plain)), f"{name}: the GEMM's output changes with the rider"
            body = plain[:16, :8 * RIDER_NB].float()
            assert bool(torch.isfinite(body).all()) and bool((body != SENT).any()) and bool((plain[16 * n_groups:].float() == SENT).all())
            st.add("launches bit-identical", 1)
    # a shape the launcher must refuse: more tokens than workgroups in x (S = 16 against ceil(70 / 14) = 5 is not built here: the same
    # REQUIRE is reached with S = 17 > 16)
    c17 = dict(c, S=17, x=torch.randn(17, D, generator=g).to(bf16), amask=None)
    a, G, keep = prep(dev, c17)
    rc, out = rider_launch(dev, D, n_groups, 16, a)
    assert rc != 0, "S = 17 riders in a launch of 16 workgroups per group accepted"
    G.untouched("refused rider launch")
    assert bool((out.float() == SENT).all()), "a refused launch wrote GEMM output"
    for bad in (dict(n_dyn=8), dict(D=1024), dict(norm_only=1)):
        a, G, keep = prep(dev, c, over=bad)
        rc, out = rider_launch(dev, D, n_groups, 16, a)
        assert rc != 0, bad
        G.untouched(f"refused rider launch {bad}")
        assert bool((out.float() == SENT).all())


# ------------------------------------------------------------------------------------------------ 6. tables and permute
def tables(dev, S, n_real, align=1):
    G = Guarded(dev)
    cap = max(1, S * n_real + n_real * (align - 1))
    G.new("counts", (n_real,), torch.int32)
    G.new("offsets", (n_real + 1,), torch.int32)
    G.new("slot_token", (cap,), torch.int32)
    G.new("slot_of", (max(S, 1), n_real), torch.int32)
    return G


def table_ptrs(G):
    return [C.c_void_p(G.ptr(n)) for n in ("counts", "offsets", "slot_token", "slot_of")]


@gpu
@pytest.mark.parametrize("n_real", [1, 8, 16])
def test_dispatch_build_vs_oracle(dev, n_real):
    """dispatch_kernel through umoe_dispatch_build at its 256-token chunk edges"""
    from unimoe_audio_amd import _lib as L
    for S in (17, 255, 256, 257, 511, 512, 513):
        m = make_mask(S, n_real)
        md = nan_tail(m, dev, 0)
        G = tables(dev, S, n_real)
        rc = L.lib().umoe_dispatch_build(C.c_void_p(md.data_ptr()), S, m.shape[1], n_real, *table_ptrs(G), stream())
        torch.cuda.synchronize()
        assert rc == 0
        G.pads_intact(f"dispatch_build S={S}")
        check_tables(f"dispatch_build S={S} n_real={n_real}", m, n_real, 1, G.get("counts"), G.get("offsets"), G.get("slot_token"), G.get("slot_of")[:S])


@gpu
@pytest.mark.parametrize("align", [1, 8, 256])
def test_dispatch_build_aligned_vs_oracle(dev, align):
    from unimoe_audio_amd import _lib as L
    for S, n_real in [(17, 8), (256, 8), (257, 8), (513, 8), (257, 1), (255, 16)]:
        m = make_mask(S, n_real)
        md = nan_tail(m, dev, 0)
        G = tables(dev, S, n_real, align)
        rc = L.lib().umoe_dispatch_build_aligned(C.c_void_p(md.data_ptr()), S, m.shape[1], n_real, align, *table_ptrs(G), stream())
        torch.cuda.synchronize()
        assert rc == 0
        G.pads_intact(f"dispatch_build_aligned S={S}")
        check_tables(f"dispatch_build_aligned S={S} n_real={n_real} align={align}", m, n_real, align, G.get("counts"), G.get("offsets"),
                     G.get("slot_token"), G.get("slot_of")[:S])


@gpu
def test_dispatch_refusals_write_nothing(dev):
    from unimoe_audio_amd import _lib as L
    S, n_real = 40, 8
    m = make_mask(S, 16)                     # ld = 19: large enough for every variant below, were one accepted
    md = nan_tail(m, dev, 0)
    mp = C.c_void_p(md.data_ptr())
    for what in ("align 3", "align 512", "align 0", "ld < n_real", "null mask", "null counts", "null offsets", "null slot_token", "null slot_of",
                 "n_real 17", "n_real 0"):
        for aligned in (True, False):
            if what.startswith("align") and not aligned:
                continue
            G = tables(dev, S, 17 if what == "n_real 17" else n_real, 512)
            p = table_ptrs(G)
            if what.startswith("null "):
                key = what[5:]
                if key != "mask":
                    p[("counts", "offsets", "slot_token", "slot_of").index(key)] = None
            nr = 17 if what == "n_real 17" else 0 if what == "n_real 0" else n_real
            ld = n_real - 1 if what == "ld < n_real" else 19
            al = int(what[6:]) if what.startswith("align") else 8
            mk = None if what == "null mask" else mp
            if aligned:
                rc = L.lib().umoe_dispatch_build_aligned(mk, S, ld, nr, al, *p, stream())
            else:
                rc = L.lib().umoe_dispatch_build(mk, S, ld, nr, *p, stream())
            torch.cuda.synchronize()
            assert rc != 0, (what, aligned)
            G.untouched(f"refused dispatch ({what})")


@gpu
@pytest.mark.parametrize("S", [0, 1, 15, 16, 17])
def test_router_dispatch_fwd_vs_oracle(dev, S):
    """umoe_router_dispatch_fwd: dispatch_small_kernel at S <= 16, dispatch_kernel beyond; both from x and from planted logits_in (a full, an
    empty and a last-token-only column); the router's outputs equal umoe_router_fwd's"""
    from unimoe_audio_amd import _lib as L
    g = gen(3300 + S)
    D, nd, nf, nr = 512, 9, 2, 8
    lg = torch.randn(S, 11, generator=g)
    lg[:, 0], lg[:, 1], lg[:, nr - 1] = 5.0, -50.0, -40.0
    if S:
        lg[S - 1, nr - 1] = 4.0
    base = dict(S=S, D=D, n_dyn=nd, n_fix=nf, n_real=nr, bf=True, h=True, x=torch.randn(S, D, generator=g).to(bf16), xn=None, amask=None,
                gate=(torch.randn(11, D, generator=g) * 0.05).to(bf16), nw=(1 + 0.1 * torch.randn(D, generator=g)).to(bf16), top_p=0.9, topk=0)
    for mode in ("x", "logits bf16", "logits fp32"):
        c = dict(base)
        kw = {}
        if mode != "x":
            c.update(top_p=0.0, topk=3, h=False, x=None, gate=None, nw=None, D=0)
            kw["logits_in"] = lg.to(bf16 if mode == "logits bf16" else f32)
        a, G, keep = prep(dev, c, **kw)
        T = tables(dev, S, nr)
        rc = L.lib().umoe_router_dispatch_fwd(C.byref(a), *table_ptrs(T), stream())
        torch.cuda.synchronize()
        assert rc == 0, mode
        if S == 0:
            G.untouched("S = 0")
            T.untouched("S = 0")
            continue
        G.pads_intact(mode)
        T.pads_intact(mode)
        rc, alone, _ = launch(dev, c, **kw)
        assert rc == 0
        for key in alone:
            got = G.get(key)[:S]
            assert torch.equal(bits(got), bits(alone[key])), f"{mode}: {key} differs from umoe_router_fwd"
        mask = alone["expert_mask"]
        check_chain(f"router_dispatch_fwd {mode}", c, alone["logits"], alone)
        if mode != "x":
            cnt = mask[:, :nr].sum(0)
            assert int(cnt[0]) == S and int(cnt[1]) == 0 and int(cnt[nr - 1]) == 1, cnt
        check_tables(f"router_dispatch_fwd {mode} S={S}", mask, nr, 1, T.get("counts"), T.get("offsets"), T.get("slot_token"), T.get("slot_of")[:S])
    a, G, keep = prep(dev, dict(base, S=max(S, 1), x=torch.zeros(max(S, 1), D).to(bf16)))
    T = tables(dev, max(S, 1), nr)
    p = table_ptrs(T)
    p[S % 4] = None
    rc = L.lib().umoe_router_dispatch_fwd(C.byref(a), *p, stream())
    torch.cuda.synchronize()
    assert rc != 0
    G.untouched("null table")
    T.untouched("null table")


@gpu
@pytest.mark.parametrize("S,D", [(17, 8), (257, 520), (40, 2048)])
def test_permute_leaves_dead_slots(dev, S, D):
    """permute_kernel with more workgroups than live slots: rows >= offsets[n_real] keep the sentinel"""
    from unimoe_audio_amd import _lib as L
    n_real = 8
    m = make_mask(S, n_real)
    md = nan_tail(m, dev, 0)
    T = tables(dev, S, n_real)
    assert L.lib().umoe_dispatch_build(C.c_void_p(md.data_ptr()), S, m.shape[1], n_real, *table_ptrs(T), stream()) == 0
    total = int(T.get("offsets")[n_real])
    max_slots = S * n_real
    assert 0 < total < max_slots
    x = torch.randn(S, D, generator=gen(S + D)).to(bf16)
    xd = nan_tail(x, dev, 2)
    G = Guarded(dev)
    G.new("out", (max_slots, D), bf16)
    tot_ptr = T.ptr("offsets") + 4 * n_real
    rc = L.lib().umoe_permute_fwd(C.c_void_p(xd.data_ptr()), D, C.c_void_p(T.ptr("slot_token")), C.c_void_p(tot_ptr), max_slots, C.c_void_p(G.ptr("out")),
                                  stream())
    torch.cuda.synchronize()
    assert rc == 0
    G.pads_intact("permute")
    out = G.get("out")
    st = T.get("slot_token")[:total].long()
    same_bits("permuted rows", out[:total], x[st])
    assert bool((out[total:].float() == SENT).all()), "a row >= the live total was written"
    G2 = Guarded(dev)
    G2.new("out", (max_slots, D), bf16)
    assert L.lib().umoe_permute_fwd(C.c_void_p(xd.data_ptr()), D, C.c_void_p(T.ptr("slot_token")), C.c_void_p(tot_ptr), 0, C.c_void_p(G2.ptr("out")), stream()) == 0
    assert L.lib().umoe_permute_fwd(C.c_void_p(xd.data_ptr()), D + 4, C.c_void_p(T.ptr("slot_token")), C.c_void_p(tot_ptr), max_slots, C.c_void_p(G2.ptr("out")), stream()) != 0
    assert L.lib().umoe_permute_fwd(None, D, C.c_void_p(T.ptr("slot_token")), C.c_void_p(tot_ptr), max_slots, C.c_void_p(G2.ptr("out")), stream()) != 0
    torch.cuda.synchronize()
    G2.untouched("permute: nothing to do / refused")


# ------------------------------------------------------------------------------------------------ 7. S = 0 and the refusals
def _small(S=5, D=2048, **kw):
    g = gen(123)
    c = dict(form="", S=S, D=D, n_dyn=9, n_fix=2, n_real=8, bf=True, h=True, x=torch.randn(max(S, 1), D, generator=g).to(bf16)[:max(S, 0)], xn=None,
             amask=None, gate=(torch.randn(16, D, generator=g) * 0.03).to(bf16), nw=(1 + 0.1 * torch.randn(D, generator=g)).to(bf16), top_p=0.9, topk=0)
    c.update(kw)
    return c


@gpu
def test_router_s0_and_refusals_write_nothing(dev):
    """S = 0 returns 0; every UMOE_REQUIRE of router_check and of the norm_only branch returns its error; nothing is written either way"""
    from unimoe_audio_amd import _lib as L
    for c, kw in [(_small(S=0), {}), (_small(S=0, D=0, x=None, gate=None, nw=None, h=False), dict(logits_in=torch.zeros(0, 11)))]:
        rc, _, G = launch(dev, c, **kw)
        assert rc == 0, "S = 0"
        G.untouched("S = 0")
    assert L.lib().umoe_router_fwd(None, stream()) != 0                                            # null argument
    noise = torch.ones(5, 2048)
    gum, ru = torch.zeros(5, 9, 9), torch.zeros(5, 9)
    lg = torch.zeros(5, 11)
    refusals = [
        ("expert_mask NULL", _small(), dict(drop=("expert_mask",))),
        ("S < 0", _small(S_alloc=5), dict(over=dict(S=-1))),
        ("n_dyn = 0", _small(), dict(over=dict(n_dyn=0))),
        ("E > 16", _small(), dict(over=dict(n_dyn=14, n_fix=3))),
        ("n_real > n_dyn", _small(), dict(over=dict(n_real=10))),
        ("x NULL", _small(), dict(drop=("x",))),
        ("gate_w NULL", _small(), dict(drop=("gate_w",))),
        ("D = 0", _small(), dict(over=dict(D=0))),
        ("D % 8", _small(), dict(over=dict(D=2044))),
        ("gumbel without rand_u", _small(h=False, D=0, x=None, gate=None, nw=None), dict(logits_in=lg, gumbel=gum, rand_u=ru, drop=("rand_u",))),
        ("x_noise with norm_w", _small(h=False, xn=noise), {}),
        ("x_noise with h_out", _small(nw=None, xn=noise), {}),
        ("x_noise with logits_in", _small(h=False, nw=None, xn=noise), dict(logits_in=lg)),
        ("x_noise without x", _small(h=False, nw=None, xn=noise), dict(drop=("x",))),
        ("norm_only: x NULL", _small(), dict(want=["h"], norm_only=True, drop=("x",))),
        ("norm_only: norm_w NULL", _small(nw=None), dict(want=["h"], norm_only=True)),
        ("norm_only: h_out NULL", _small(), dict(want=["h"], norm_only=True, drop=("h",))),
        ("norm_only: S = 0", _small(S_alloc=5), dict(want=["h"], norm_only=True, over=dict(S=0))),
        ("norm_only: S = 257", _small(S_alloc=5), dict(want=["h"], norm_only=True, over=dict(S=257))),
        ("norm_only: D = 1024", _small(), dict(want=["h"], norm_only=True, over=dict(D=1024))),
    ]
    for what, c, kw in refusals:
        a, G, keep = prep(dev, c, **kw)
        if what == "x_noise with logits_in":                                                       # a real pointer, not the placeholder
            keep.append(noise.to(dev))
            a.x_noise = keep[-1].data_ptr()
        rc = L.lib().umoe_router_fwd(C.byref(a), stream())
        torch.cuda.synchronize()
        assert rc != 0, f"{what}: accepted"
        assert L.lib().umoe_last_error(), what
        G.untouched(what)
    rc, out, _ = launch(dev, _small())                                                             # the same arguments, nothing wrong: accepted
    assert rc == 0 and bool(torch.isfinite(out["h"].float()).all())


@gpu
def test_report(dev):
    """the per-form report (run after the tests above; -s shows it): launch form, largest logits error / b, flagged midpoint share of h,
    fp32 yardstick of the training branch; and the k = 1 / k = n_dyn extremes occurred in every kernel form"""
    print()
    for form in sorted(REPORT):
        Stats(REPORT[form]).show(f"report {form}")
    if len(SEEN) < len(CASES):              # a selection of the tests (-k): the figures above are partial, nothing to assert
        return
    for kind in KINDS:
        forms = [f for f in REPORT if f.startswith(kind)]
        assert forms, kind
        assert any(REPORT[f].get("k = 1 seen") for f in forms), f"{kind}: no token with k = 1"
        assert any(REPORT[f].get("k = n_dyn seen") for f in forms), f"{kind}: no token with k = n_dyn"
