"""The two ends of a training step and the path of every attention gradient (csrc/umoe_misc.hip: ce_row_kernel, ce_reduce_kernel,
ce_total_kernel, ce_bwd_kernel, aux_loss_kernel, aux_loss_part_kernel + aux_loss_fin_kernel, codec_embed_kernel, codec_embed_bwd_kernel,
codec_embed_bwd_rows_kernel, mul_noise_kernel; csrc/umoe_bwd.hip: rope_bwd_kernel), each against a float64 restatement on the CPU of
the same operation on the same input bits.

Rules of the whole file (those of tests/test_gpu_bwd_fp64.py and tests/test_gpu_fwd_fp64.py)
  * reference: float64; bf16 / fp32 inputs are upcast exactly; where a kernel documents a rounding of an intermediate to bf16 (the
    probabilities and the unweighted mean of the bf16 aux loss, every step of the embedding chain, the two products of the mRoPE
    backward) the reference rounds its float64 value at the same place;
  * comparison: per element, never a norm over a tensor;
  * bound rule (cross-entropy, aux loss, embedding backward (b), mRoPE backward beside its exact rule): |got - ref| <= bound, derived
    with u = 2^-24 (fp32 unit roundoff), first order:
      bf16 output    2^-8 |ref| + (1 + 2^-8) E32;      fp32 output    E32
      E32            a sum of n terms n u sum|terms| (n the depth of the summation tree: the adds of one thread + 6 (wave) + 3 (block)),
                     an elementwise fp32 operation u |its result|, expf 3 u, logf 3 u, a divide 2.5 u -- the limits of
                     tests/test_gpu_fwd_fp64.py (the OpenCL limits the device library is built to), not the 2 u of test_gpu_bwd_fp64.py;
                     2^-126 where a result may flush
    each reference's docstring spells its E32 out;
  * exact rule (embedding forward, embedding backward (a), jitter, mRoPE backward): every step is one IEEE fp32 operation or a bf16
    rounding, the restatement fixes every bit, there is no tolerance;
  * interval rule (aux loss, bf16 logits): the output is one scalar, so the candidate rule of test_gpu_fwd_fp64.py becomes an interval.
    A probability whose float64 value lies within its fp32 error window of a bf16 midpoint is flagged and widens the bound by
    n_dyn f_e (w_s / W) ulp_bf16(p); a per-expert mean within its window of a midpoint admits either neighbour, which makes the
    reference an interval [lo, hi]; got must lie in [lo - bound, hi + bound].  A case may flag at most 1e-2 of its probabilities: a
    condition on the inputs, checked without a GPU on the case lists the GPU tests run;
  * untouched memory: every buffer the caller owns is allocated with a tail of sentinels (bf16 / fp32 7.0) behind it, prefilled with the
    sentinel where the kernel must write all of it, and whatever the kernel must not write keeps its bits; everything a kernel must not
    read holds NaN: the logit columns past n_dyn, the aux workspace before the launch, the cache slots of dk / dv no kv_pos names.
Every GPU test prints its figures under -s ("LOSS FP64 ..."): the worst error / bound of the bound rule, the flagged share.

The checkers are tested without a GPU (test_*_cpu): a result emulated in fp32 / bf16 torch arithmetic from the same inputs passes at
the GPU tests' own case lists, the flagged shares stay under the cap, the exponent condition of the embedding data holds, and each
planted error is rejected.

Measured on an MI355X (the whole file: 82 GPU tests in 5 s), worst error / bound over the cases of each test:
  cross-entropy   nll 0.025 - 0.80, probs 0.063 - 0.82, dlogits 0.068 - 0.79: the 0.80 is the +-40 spread, where the one rounding of
                  lse ~ 40 reaches its half ulp (32 u of the 40 u the bound gives it); Gaussian logits 0.31 - 0.55 at N >= 37.
                  ch_loss 0.011 - 0.11, total 0 - 0.11: far below 1, the bound adds up the worst case of every row of a channel and the
                  rows' errors do not line up.  ch_count, the +0 of ignored rows, NaN (channel 0 empty) and +inf (-inf at a label) exact
  aux loss        one launch 0 - 0.035, workspace form 0 - 0.020, ops.aux_loss 3e-4 - 0.015: far below 1 -- the bound charges each of the
                  2 n_dyn + 1 sums its whole depth (up to 83 u) in one direction, the kernels' errors are a few u with mixed signs;
                  flagged share of the probabilities 0 - 4.4e-4 (cap 1e-2)
  embedding       forward: 8 cases bit for bit (fp32 and float64 chain alike).  backward: 13 cases (a) bit for bit in both kernels, (b)
                  0 - 0.996 (a bf16 rounding reaches its half ulp; 0.28 - 0.65 at >= 3000 hits per id, where n u sum|terms| dominates),
                  (c) / (d) exact; per-id and rows kernel agree bit for bit on 3 pairs; CodecEmbedFn / EmbedFn at D = 4096 bit for bit
  jitter          5 cases bit for bit
  mRoPE backward  16 cases bit for bit against the fp32 chain; against the unrounded float64 rotation 0.71 - 0.95
Found by this file: umoe_codec_embed_sum_bwd refused rows = 0 although its contract is rows >= 0 -- the pointer of an empty tensor is
null and the launcher demanded tok and d_out before it looked at rows, so ops.codec_embed_sum_bwd raised on an empty batch instead of
returning the zero gradient (EMB_BWD_ID case (0, 2, 5, 8)).  umoe_codec_embed_sum and umoe_mul_noise had the same order of checks.
All three now accept null pointers where there is nothing to read (csrc/umoe_misc.hip; test_empty_inputs_through_ops).  No kernel
computed a wrong value at any shape of this file.
"""
import functools
import math

import pytest
import torch

gpu = pytest.mark.gpu

U = 2.0 ** -24          # fp32 unit roundoff
BF = 2.0 ** -8          # bf16: half an ulp relative to the value, at most
TINY = 2.0 ** -126      # flush floor
EXPF = 3 * U            # expf, logf, divide: the OpenCL limits, as tests/test_gpu_fwd_fp64.py takes them
LOGF = 3 * U
DIV = 2.5 * U
SENT = 7.0              # sentinel of the output buffers
TAIL = 64               # sentinel elements behind every buffer the caller owns
CAP = 1e-2              # largest flagged share of a case
f64 = torch.float64
f32 = torch.float32
bf16 = torch.bfloat16
NAN = float("nan")
INF = float("inf")


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


class Stats(dict):
    def note(self, name, v):
        self[name] = max(self.get(name, 0.0), float(v))

    def show(self, title):
        print(f"\nLOSS FP64 {title}: " + ", ".join(f"{k} {v:.3g}" for k, v in self.items()))


def check(name, got, ref, bound, stats):
    """|got - ref| <= bound per element; where ref is NaN got must be NaN, where ref is +-inf got must be the same infinity"""
    got = got.detach().cpu().to(f64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    nan, inf = torch.isnan(ref), torch.isinf(ref)
    assert torch.equal(torch.isnan(got), nan), f"{name}: NaN pattern differs"
    assert torch.equal(got[inf], ref[inf]), f"{name}: infinities differ"
    fin = ~nan & ~inf
    assert bool(torch.isfinite(got[fin]).all()), f"{name}: non-finite value"
    err, b = (got - ref).abs()[fin], bound[fin]
    ratio = torch.where(b > 0, err / b, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    stats.note(name, worst)
    if not worst <= 1.0:
        i = int(ratio.argmax())
        raise AssertionError(f"{name}: error / bound = {worst:.4g} (error {float(err[i]):.4g}, bound {float(b[i]):.4g}, flat index {i} of the finite elements)")


def _rejects(fn):
    with pytest.raises(AssertionError):
        fn()


def cdiv(a, b):
    return -(-a // b)


# ================================================================================================ 1. codec cross-entropy
CE_CASES = [            # N, C, V, kind, grad
    (1, 3, 2, "gauss", 1.0), (257, 3, 2, "gauss", 0.37), (37, 12, 19, "gauss", 1.0), (700, 3, 19, "spread", 0.37),
    (255, 3, 255, "gauss", 0.37), (257, 1, 255, "gauss", 1.0), (255, 1, 256, "gauss", 1.0), (256, 3, 256, "inf_label", 0.37),
    (257, 3, 256, "ch0_empty", 1.0), (1, 3, 257, "gauss", 0.37), (700, 3, 257, "gauss", 1.0), (37, 12, 1027, "gauss", 0.37),
    (700, 1, 1027, "gauss", 1.0), (700, 3, 1027, "gauss", 0.37), (700, 12, 1027, "gauss", 1.0),
]
CE_PLANT = 13           # (700, 3, 1027): the case of the planted errors


@functools.lru_cache(maxsize=None)
def make_ce(idx):
    """Labels: rows 0 / 1 / 2 hold 0, V - 1 and -100 in every channel, rows 6 / 7 hold V and V + 5 (ignored, as the kernel documents);
    with C >= 3 channel 1 has no valid label and channel C - 1 exactly one, in the last row; "ch0_empty": channel 0 has none;
    logits: Gaussian x 2 ("spread": uniform in +-40), row 3 all equal, row 4 -inf at every third column away from the label,
    "inf_label": -inf at the label of row 5, channel 0."""
    N, C, V, kind, grad = CE_CASES[idx]
    g = gen(21000 + idx)
    x = 2 * torch.randn(N, C, V, generator=g)
    if kind == "spread":
        x = 40 * (2 * torch.rand(N, C, V, generator=g) - 1)
    lab = torch.randint(0, V, (N, C), generator=g)
    lab[torch.rand(N, C, generator=g) < 0.3] = -100
    if N >= 37:
        lab[0], lab[1], lab[2], lab[6], lab[7] = 0, V - 1, -100, V, V + 5
        x[3] = 1.25
        lab[4] = V - 1
        x[4, :, ::3] = -INF
        x[4, :, V - 1] = 0.5
    else:
        lab[0, 0] = 0
    if N > 256:
        lab[256, 0] = 1
    if C >= 3:
        lab[:, 1] = torch.where(torch.rand(N, generator=g) < 0.5, torch.tensor(-100), V + torch.randint(0, 9, (N,), generator=g))
        lab[:, C - 1] = -100
        lab[N - 1, C - 1] = V - 1
    if kind == "ch0_empty":
        lab[:, 0] = -100
    if kind == "inf_label":
        lab[5, 0] = 3
        x[5, 0, 3] = -INF
    return dict(N=N, C=C, V=V, kind=kind, grad=float(torch.tensor(grad, dtype=f32)), x=x.contiguous(), lab=lab.contiguous())


@functools.lru_cache(maxsize=None)
def ref_ce(idx):
    """float64 log-sum-exp per row.  E32, first order, d = x - mx (mx is exact):
      e_v = expf(d_v)     relative u |d_v| + EXPF (the rounding of d lands in the exponent); exactly 0 at x = -inf
      sm                  sum_v e_v (u |d_v| + EXPF) + (ceil(V / 256) + 9) u sm + V 2^-126 (terms that flush)
      lse = mx + logf(sm) E_lse = delta(sm) / sm + LOGF |log sm| + u |lse|
      nll = lse - x[lab]  E_lse + u |nll|; exactly 0 at an ignored label, +inf where x[lab] = -inf
      probs = expf(x - lse)  p (E_lse + u |x - lse| + EXPF) + 2^-126; exactly 0 at x = -inf
      ch_loss = s / cnt   (sum_n E_nll + (ceil(N / 256) + 9) u sum_n |nll|) / cnt + DIV |ch_loss|; cnt exact (a float sum of ones below 2^24)
      total               sum_c E_ch + C u sum_c |ch_loss|
      dlogits = sc p', sc = grad / cnt, p' = p - onehot:  |sc| (E_p + u |p - 1| at the label) + (DIV + u) |dlogits|; +0 on ignored rows"""
    c = make_ce(idx)
    N, C, V = c["N"], c["C"], c["V"]
    x, lab = c["x"].to(f64), c["lab"]
    valid = (lab >= 0) & (lab < V)
    mx = x.max(-1, keepdim=True).values
    d = x - mx
    ad = torch.where(torch.isinf(d), torch.zeros_like(d), d.abs())
    e = torch.exp(d)
    sm = e.sum(-1, keepdim=True)
    lse = mx + torch.log(sm)
    dsm = (e * (U * ad + EXPF)).sum(-1, keepdim=True) + (cdiv(V, 256) + 9) * U * sm + V * TINY
    e_lse = dsm / sm + LOGF * torch.log(sm).abs() + U * lse.abs()
    xl = torch.gather(x, -1, lab.clamp(0, V - 1)[..., None])
    nll = torch.where(valid, (lse - xl)[..., 0], torch.zeros(N, C, dtype=f64))
    nll_fin = torch.where(torch.isinf(nll), torch.zeros_like(nll), nll)
    e_nll = torch.where(valid, e_lse[..., 0] + U * nll_fin.abs(), torch.zeros(N, C, dtype=f64))
    p = torch.exp(x - lse)
    axl = torch.where(torch.isinf(x), torch.zeros_like(x), (x - lse).abs())
    e_p = p * (e_lse + U * axl + EXPF) + TINY
    e_p = torch.where(torch.isinf(x), torch.zeros_like(e_p), e_p)
    cnt = valid.sum(0)
    cf = cnt.to(f64).clamp(min=1)
    loss = nll.sum(0) / cf
    e_ch = (e_nll.sum(0) + (cdiv(N, 256) + 9) * U * nll_fin.abs().sum(0)) / cf + DIV * loss.abs()
    loss = torch.where(cnt > 0, loss, torch.zeros_like(loss))
    if int(cnt[0]) == 0:
        loss[0] = NAN
    inc = cnt > 0
    inc[0] = True
    total = loss[inc].sum().reshape(1)
    fin = torch.where(torch.isfinite(loss), loss, torch.zeros_like(loss))
    e_tot = (e_ch[inc].sum() + C * U * fin[inc].abs().sum()).reshape(1)
    onehot = torch.zeros(N, C, V, dtype=f64)
    onehot.scatter_(-1, lab.clamp(0, V - 1)[..., None], 1.0)
    sc = torch.where(valid, c["grad"] / cf[None], torch.zeros(N, C, dtype=f64))[..., None]
    dl = sc * (p - onehot)
    e_dl = sc.abs() * (e_p + onehot * U * (p - 1).abs()) + (DIV + U) * dl.abs()
    return dict(valid=valid, nll=nll, e_nll=e_nll, p=p, e_p=e_p, cnt=cnt, loss=loss, e_ch=e_ch, total=total, e_tot=e_tot, dl=dl, e_dl=e_dl)


def emu_ce(c, bug=None, want_probs=True):
    N, C, V = c["N"], c["C"], c["V"]
    x, lab = c["x"], c["lab"]
    valid = (lab >= 0) & (lab < V)
    mx = x.max(-1, keepdim=True).values
    e = (x - mx).exp()
    if bug == "last v missing":
        e[..., V - 1] = 0
    lse = mx + e.sum(-1, keepdim=True).log()
    nll = torch.where(valid, (lse - torch.gather(x, -1, lab.clamp(0, V - 1)[..., None]))[..., 0], torch.zeros(N, C))
    p = (x - lse).exp()
    cnt = valid.sum(0)
    s = nll.clone()
    if bug == "row 256 missing":
        s[256] = 0
    cnt_used = cnt + (1 if bug == "count off by one" else 0)
    loss = torch.where(cnt > 0, s.sum(0) / cnt_used.float().clamp(min=1), torch.zeros(C))
    if int(cnt[0]) == 0:
        loss[0] = NAN
    total = loss[0].clone()
    for ch in range(1, C):
        if int(cnt[ch]) > 0:
            total = total + loss[ch]
        elif bug == "skipped channel added":
            total = total + torch.tensor(NAN)        # torch's mean over nothing
    onehot = torch.zeros(N, C, V)
    onehot.scatter_(-1, ((lab + (1 if bug == "onehot at lab + 1" else 0)) % V).clamp(0, V - 1)[..., None], 1.0)
    onehot = onehot * valid[..., None]                          # an ignored label matches no column
    sc = torch.where(valid, torch.tensor(c["grad"]) / cnt.float().clamp(min=1)[None], torch.zeros(N, C))[..., None]
    dl = sc * (p - onehot)
    return dict(nll=nll, probs=p if want_probs else None, ch_loss=loss, ch_count=cnt_used.to(torch.int32), total=total.reshape(1), dl=dl)


def check_ce(r, o, st):
    check("nll", o["nll"], r["nll"], r["e_nll"], st)
    same_bits("nll of ignored labels (+0)", o["nll"].detach().cpu()[~r["valid"]], torch.zeros(int((~r["valid"]).sum()), dtype=f32))
    if o["probs"] is not None:
        check("probs", o["probs"], r["p"], r["e_p"], st)
    assert torch.equal(o["ch_count"].detach().cpu().long(), r["cnt"]), "ch_count"
    check("ch_loss", o["ch_loss"], r["loss"], r["e_ch"], st)
    check("total", o["total"], r["total"], r["e_tot"], st)
    if o["dl"] is not None:
        check("dlogits", o["dl"], r["dl"], r["e_dl"], st)
        dead = o["dl"].detach().cpu()[~r["valid"]]
        same_bits("dlogits of ignored rows (+0)", dead, torch.zeros_like(dead))


def test_ce_checker_cpu():
    st = Stats()
    for idx in range(len(CE_CASES)):
        c = make_ce(idx)
        check_ce(ref_ce(idx), emu_ce(c), st)
        o = emu_ce(c, want_probs=False)
        o["dl"] = None
        check_ce(ref_ce(idx), o, st)
    st.show("cross-entropy (emulation)")
    # the case lists hold what the issue asks for
    for V in (2, 19, 255, 256, 257, 1027):
        ns = [a[0] for a in CE_CASES if a[2] == V]
        assert min(ns) < 256 and max(ns) >= 256, (V, ns)
    assert {a[1] for a in CE_CASES if a[0] == 700 and a[2] == 1027} == {1, 3, 12}
    assert {a[0] for a in CE_CASES} == {1, 37, 255, 256, 257, 700}
    c, r = make_ce(CE_PLANT), ref_ce(CE_PLANT)
    assert int(r["cnt"][1]) == 0 and int(r["cnt"][2]) == 1 and bool(r["valid"][256, 0])
    for bug in ("last v missing", "row 256 missing", "count off by one", "onehot at lab + 1", "skipped channel added"):
        _rejects(lambda: check_ce(r, emu_ce(c, bug), Stats()))
    r8, r7 = ref_ce(8), ref_ce(7)
    assert math.isnan(float(r8["total"])) and float(r7["total"]) == INF and float(r7["loss"][0]) == INF


# ================================================================================================ 2. aux load-balancing loss
AUX_S = (1, 5, 63, 64, 65, 255, 257, 2047, 2049, 6240)
AUX_GEOMS = [(11, 9), (9, 9), (16, 16), (4, 1)]            # E, n_dyn
AUX_SCALES = (0.05, 1.5, 6.0)
AUX_PARTS = 64
AUX_OPS = [(S, 11, 9, b, w, 1.5) for S in (2047, 2048, 2049) for b, w in ((True, False), (False, True))]


def aux_cases(S):
    """four cases per S: bf16 / fp32 logits x without / with token weights, geometry and scale rotating"""
    i = AUX_S.index(S)
    return [(S,) + AUX_GEOMS[(i + j) % 4] + (j < 2, j % 2 == 1, AUX_SCALES[(i + j) % 3]) for j in range(4)]


@functools.lru_cache(maxsize=None)
def make_aux(S, E, n_dyn, isbf, weighted, scale):
    g = gen(31000 + S + 17 * E + 3 * n_dyn + 2 * isbf + weighted)
    logits = torch.randn(S, E, generator=g) * scale
    logits[:, n_dyn:] = NAN                                    # columns the kernels must not read
    logits = logits.to(bf16) if isbf else logits
    mask = (torch.rand(S, E, generator=g) < 0.45).to(torch.int32)
    mask[3::7, :n_dyn] = 0                                     # rows with no selected dynamic column: a uniform softmax
    tw = torch.rand(S, generator=g) if weighted else None
    return dict(S=S, E=E, n_dyn=n_dyn, isbf=isbf, weighted=weighted, logits=logits.contiguous(), mask=mask.contiguous(), tw=tw)


def aux_depth(S, form):
    return cdiv(S, 256) + 9 if form == "one" else cdiv(cdiv(S, AUX_PARTS), 256) + 9 + AUX_PARTS


@functools.lru_cache(maxsize=None)
def ref_aux(case, form):
    """float64 of core.py:361-389 -> (lo, hi, bound, flagged share).  E32, first order, d = x - mx, n = aux_depth (the adds of one
    thread + 9, + 64 for the finisher's sum over the parts):
      p          relative u |d| + EXPF (the term) + sum_e e (u |d| + EXPF) / sm + n_dyn u (the sum) + DIV; bf16 logits: p rounded to bf16
                 where it is not flagged (no error left), one bf16 ulp where it is
      b_e        sum_s w_s delta(p) (+ u w_s p with weights: the product) + n u b_e;   a_e  n u a_e;   W  n u W
      f_e = a_e / W, m_e = b_e / W     delta(a or b) / W + (a or b) delta(W) / W^2 + DIV (f or m); bf16 without weights: m_e rounded to
                 bf16 (no error left), either neighbour where m_e lies within that error of a midpoint
      out = n_dyn sum_e f_e m_e        n_dyn (sum_e f delta(m) + m delta(f) + u f m + n_dyn u sum_e f m) + u |out|"""
    c = make_aux(*case)
    S, n_dyn, isbf, weighted = c["S"], c["n_dyn"], c["isbf"], c["weighted"]
    low = float(torch.finfo(bf16 if isbf else f32).min)
    m = c["mask"][:, :n_dyn] != 0
    x = torch.where(m, c["logits"][:, :n_dyn].to(f64), torch.full((S, n_dyn), low, dtype=f64))
    d = x - x.max(-1, keepdim=True).values
    e = torch.exp(d)
    sm = e.sum(-1, keepdim=True)
    p = e / sm
    rel = U * d.abs() + EXPF + (e * (U * d.abs() + EXPF)).sum(-1, keepdim=True) / sm + n_dyn * U + DIV
    dp = p * rel                                              # (0 where e = 0: |d| u stays finite)
    if isbf:
        flag = (mid_dist(p) <= dp) & (p > 0)
        dp = torch.where(flag, ulp_bf16(p), torch.zeros_like(p))
        p = rbf(p)
    else:
        flag = torch.zeros_like(m)
    w = (c["tw"].to(f64) if weighted else torch.ones(S, dtype=f64))[:, None]
    n = aux_depth(S, form)
    W = w.sum()
    a, b = (w * m).sum(0), (w * p).sum(0)
    e_b = (w * (dp + (U * p if weighted else 0))).sum(0) + n * U * b
    e_a, e_w = n * U * a, n * U * W
    f, mean = a / W, b / W
    e_f = e_a / W + a * e_w / W ** 2 + DIV * f
    e_m = e_b / W + b * e_w / W ** 2 + DIV * mean
    lo = hi = mean
    if isbf and not weighted:
        fm = mid_dist(mean) <= e_m
        r, o = rbf(mean), other_bf16(mean)
        lo, hi = torch.where(fm, torch.minimum(r, o), r), torch.where(fm, torch.maximum(r, o), r)
        e_m = torch.zeros_like(e_m)
    out_lo, out_hi = n_dyn * (f * lo).sum(), n_dyn * (f * hi).sum()
    bound = n_dyn * ((f * e_m + hi * e_f + U * f * hi).sum() + n_dyn * U * (f * hi).sum()) + U * out_hi
    return float(out_lo), float(out_hi), float(bound), float(flag.double().mean())


def emu_aux(c, form, bug=None):
    S, E, n_dyn, isbf, weighted = c["S"], c["E"], c["n_dyn"], c["isbf"], c["weighted"]
    low = 0.0 if bug == "min replaced by 0" else float(torch.finfo(bf16 if isbf else f32).min)
    m = c["mask"][:, :n_dyn] != 0
    x = torch.where(m, c["logits"][:, :n_dyn].float(), torch.full((S, n_dyn), low))
    e = (x - x.max(-1, keepdim=True).values).exp()
    p = e / e.sum(-1, keepdim=True)
    p = rbf(p) if isbf else p
    w = (c["tw"] if weighted else torch.ones(S))[:, None]
    per = S if form == "one" else cdiv(S, AUX_PARTS)
    parts = [(q * per, min(S, (q + 1) * per)) for q in range(cdiv(S, per))]
    if bug == "last token missing":
        parts[-1] = (parts[-1][0], S - 1)
    if bug == "part counted twice":
        parts.append(parts[1])
    a, b, W = torch.zeros(n_dyn), torch.zeros(n_dyn), torch.zeros(())
    for s0, s1 in parts:
        a, b, W = a + (w[s0:s1] * m[s0:s1]).sum(0), b + (w[s0:s1] * p[s0:s1]).sum(0), W + w[s0:s1].sum()
    pm = b / W
    if isbf and not weighted and bug != "mean unrounded":
        pm = rbf(pm)
    return ((a / W) * pm).sum() * float(E if bug == "E in the factor" else n_dyn)


def check_aux(name, got, ref, st):
    lo, hi, bound, share = ref
    got = float(got)
    assert math.isfinite(got), (name, got)
    out = max(lo - got, got - hi, 0.0)
    ratio = out / bound if bound > 0 else (0.0 if out == 0 else math.inf)      # (no column selected anywhere: exactly 0)
    st.note(name, ratio)
    st.note("flagged share", share)
    assert ratio <= 1.0, f"{name}: {got!r} outside [{lo!r}, {hi!r}] by {ratio:.4g} of the bound {bound:.4g}"


def test_aux_checker_cpu():
    st = Stats()
    for case in [k for S in AUX_S for k in aux_cases(S)] + AUX_OPS:
        c = make_aux(*case)
        for form in ("one", "ws"):
            r = ref_aux(case, form)
            assert r[3] <= CAP, (case, r[3])
            check_aux(form, emu_aux(c, form), r, st)
    st.show("aux loss (emulation)")
    assert bool((make_aux(*aux_cases(257)[0])["mask"][3, :9] == 0).all())
    geoms = {(k[1:3], k[3], k[4]) for S in AUX_S for k in aux_cases(S)}
    assert {g[0] for g in geoms} == set(AUX_GEOMS) and len(geoms) >= 12
    for case, form, bug in ((aux_cases(65)[0], "ws", "last token missing"), (aux_cases(257)[3], "one", "last token missing"),
                            (aux_cases(6240)[0], "ws", "part counted twice"), (aux_cases(6240)[2], "ws", "part counted twice"),
                            (aux_cases(257)[0], "one", "min replaced by 0"), (aux_cases(2049)[2], "ws", "min replaced by 0"),
                            ([k for S in AUX_S for k in aux_cases(S) if k[3] and not k[4] and k[0] >= 255][0], "ws", "mean unrounded"),
                            ([k for S in AUX_S for k in aux_cases(S) if k[1] != k[2]][0], "one", "E in the factor")):
        c = make_aux(*case)
        _rejects(lambda: check_aux(bug, emu_aux(c, form, bug), ref_aux(case, form), Stats()))


# ================================================================================================ 3. embedding, forward and backward
EMB_FWD = [             # rows, C, V, D
    (1, 1, 1, 8), (37, 2, 19, 64), (700, 12, 1027, 2048), (37, 12, 19, 2056), (37, 2, 1027, 4096), (700, 1, 19, 4096), (1, 12, 1027, 64),
    (700, 2, 1, 8),
]
EMB_EMIN, EMB_EMAX = -6, 3     # table entries: +-2^t, t uniform in [EMB_EMIN, EMB_EMAX)


def odd_ids(tok, V, g, share=0.1):
    """-1, -100, V and V + 5 mixed into a copy of tok"""
    tok = tok.clone()
    pick = torch.rand(tok.shape, generator=g) < share
    odd = torch.tensor([-1, -100, V, V + 5])[torch.randint(0, 4, tok.shape, generator=g)]
    return torch.where(pick, odd, tok)


@functools.lru_cache(maxsize=None)
def make_emb_fwd(idx):
    rows, C, V, D = EMB_FWD[idx]
    g = gen(41000 + idx)
    t = EMB_EMIN + (EMB_EMAX - EMB_EMIN) * torch.rand(C, V, D, generator=g)
    emb = (torch.exp2(t) * torch.where(torch.rand(C, V, D, generator=g) < 0.5, -1.0, 1.0)).to(bf16)
    tok = odd_ids(torch.randint(0, V, (rows, C), generator=g), V, g).to(torch.int32)
    if rows >= 4 and C >= 1:
        tok[0, 0], tok[1, 0], tok[2, 0], tok[3, 0] = -1, -100, V, V + 5
    return dict(rows=rows, C=C, V=V, D=D, emb=emb, tok=tok)


def emb_chain(c, dt):
    """acc = e_0, then acc = bf16(acc + e_ch) in channel order, ids clamped into [0, V - 1] as the kernel does; dt: the arithmetic"""
    tok = c["tok"].long().clamp(0, c["V"] - 1)
    acc = c["emb"][0][tok[:, 0]].to(dt)
    for ch in range(1, c["C"]):
        acc = rbf(acc + c["emb"][ch][tok[:, ch]].to(dt))
    return to_bf(acc)


def emb_exponents_ok(c):
    """The condition on the inputs under which the fp32 chain and the float64 chain give the same bits: every table entry is non-zero
    with exponents within 16 of each other -- here within s = spread of EMB_EMIN .. EMB_EMAX -- and s + 8 + ceil(log2 C) <= 24: every
    partial sum is a multiple of the smallest entry's last bit and below C times the largest entry, so every add is exact in fp32."""
    _, ex = torch.frexp(c["emb"].float())
    spread = int(ex.max() - ex.min())
    return bool((c["emb"] != 0).all()) and spread <= 16 and spread + 8 + math.ceil(math.log2(c["C"])) <= 24


def test_embed_fwd_checker_cpu():
    for idx in range(len(EMB_FWD)):
        c = make_emb_fwd(idx)
        assert emb_exponents_ok(c), idx
        same_bits(f"fp32 chain vs float64 chain, case {idx}", emb_chain(c, f32), emb_chain(c, f64))
    assert {k[3] for k in EMB_FWD} == {8, 64, 2048, 2056, 4096} and {k[1] for k in EMB_FWD} == {1, 2, 12}
    assert {k[0] for k in EMB_FWD} == {1, 37, 700} and {k[2] for k in EMB_FWD} == {1, 19, 1027}
    c = make_emb_fwd(3)
    want = emb_chain(c, f32)
    bad = dict(c, tok=c["tok"].clamp(min=0))
    bad["tok"] = torch.where(c["tok"] >= c["V"], torch.zeros_like(c["tok"]), bad["tok"])      # ids >= V wrapped to 0, not clamped to V - 1
    _rejects(lambda: same_bits("out", emb_chain(bad, f32), want))
    rev = dict(c, emb=c["emb"].flip(0), tok=c["tok"].flip(1))                                  # the chain in descending channel order
    _rejects(lambda: same_bits("out", emb_chain(rev, f32), want))


# ---- backward
EMB_BWD_ID = [          # rows, C, V, D, kind: the per-id kernel (V <= 4 rows, or no rows)
    (0, 2, 5, 8, ""), (1, 1, 3, 2056, ""), (255, 2, 19, 4096, ""), (256, 1, 7, 16384, ""), (257, 3, 19, 2048, ""), (257, 1, 3, 8, "order"),
    (16384, 1, 5, 8, ""), (16385, 2, 5, 8, "late"), (20000, 2, 11, 64, "late"),
]
EMB_BWD_ROWS = [        # the rows kernel (V > 4 rows)
    (1, 2, 5, 2056, ""), (257, 1, 1500, 4096, "own"), (600, 2, 5000, 64, "own"), (16385, 2, 65541, 8, "late"),
]
EMB_BWD_PAIR = [        # rows, C, V (per-id kernel), V padded (rows kernel), D
    (257, 2, 19, 1100, 2056), (600, 1, 11, 2500, 64), (16385, 1, 5, 65541, 8),
]
EMB_PASS = 16384        # rows per pass of both kernels


@functools.lru_cache(maxsize=None)
def make_emb_bwd(rows, C, V, D, kind):
    """kind "late": channel 0 gives every row to id 2 (V = 5) or repeats the id of row 3 at row 16384 (a duplicate whose first hit is in
    the first pass), and the last channel hits id V - 1 only at rows >= 16384; "own": row 0 holds -1 and row 1 holds V + 5, the rows that
    would own ids 0 and V - 1 had the ids been clamped, and ids 0 and V - 1 come later; "order": every row hits id 1, with 2^30, -2^30
    in rows 0 and 1 and 1.0 elsewhere: ascending the sum is 255, descending 256"""
    g = gen(42000 + rows + 7 * V + D + 3 * C)
    tok = torch.randint(0, V, (rows, C), generator=g)
    dy = torch.randn(rows, D, generator=g)
    if kind == "order":
        tok[:] = 1
        dy[:] = 1.0
        dy[0], dy[1] = 2.0 ** 30, -2.0 ** 30
    else:
        tok = odd_ids(tok, V, g, 0.05)
    if kind == "late":
        if V == 5:
            tok[:, 0] = 2
        else:
            tok[EMB_PASS, 0] = tok[3, 0] = 4
        last = tok[:, C - 1]
        last[:EMB_PASS][last[:EMB_PASS] == V - 1] = 0
        last[EMB_PASS:] = V - 1
    if kind == "own":
        tok[0], tok[1] = -1, V + 5
        tok[5], tok[6] = 0, V - 1
        tok[rows - 1] = tok[7]                                 # a duplicate
    return dict(rows=rows, C=C, V=V, D=D, tok=tok.to(torch.int32).contiguous(), dy=dy.to(bf16).contiguous())


def emb_bwd_seq(c, bug=None):
    """(a): the fp32 sum of the bf16 rows of d_out that chose an id, one IEEE add per row in ascending row order, rounded once to bf16.
    The k-th hits of all ids are added in one vector operation, k ascending."""
    rows, C, V, D = c["rows"], c["C"], c["V"], c["D"]
    out = torch.zeros(C, V, D)
    dy = c["dy"].float()
    for ch in range(C):
        t = c["tok"][:, ch].long()
        if bug == "clamped":
            t = t.clamp(0, V - 1)
        r = torch.nonzero((t >= 0) & (t < V))[:, 0]
        if bug == "second pass missing":
            r = r[r < EMB_PASS]
        if r.numel() == 0:
            continue
        if bug == "descending":
            r = r.flip(0)
        ids, order = torch.sort(t[r], stable=True)
        r = r[order]
        start = torch.searchsorted(ids, ids)                   # the first position of each id's group
        rank = torch.arange(ids.numel()) - start
        by_rank = torch.argsort(rank, stable=True)
        ids, r, cnt = ids[by_rank], r[by_rank], torch.bincount(rank)
        pos = 0
        for n in cnt.tolist():
            out[ch].index_put_((ids[pos:pos + n],), out[ch][ids[pos:pos + n]] + dy[r[pos:pos + n]])
            pos += n
    if bug == "q = 1 chunk zero":
        out[..., 2048:4096] = 0
    return to_bf(out)


@functools.lru_cache(maxsize=None)
def ref_emb_bwd(rows, C, V, D, kind):
    """(b): float64 index_add; bound 2^-8 |ref| + (1 + 2^-8) n u sum|terms|, n the hit count of the id -> (ref, bound, hits)"""
    c = make_emb_bwd(rows, C, V, D, kind)
    ref, ab, hits = torch.zeros(C, V, D, dtype=f64), torch.zeros(C, V, D, dtype=f64), torch.zeros(C, V, dtype=f64)
    dy = c["dy"].to(f64)
    for ch in range(C):
        t = c["tok"][:, ch].long()
        ok = (t >= 0) & (t < V)
        ref[ch].index_add_(0, t[ok], dy[ok])
        ab[ch].index_add_(0, t[ok], dy[ok].abs())
        hits[ch].index_add_(0, t[ok], torch.ones(int(ok.sum()), dtype=f64))
    return ref, bf16_out(ref, hits[..., None] * U * ab), hits


def check_emb_bwd(case, got, st, seq=None):
    """(a) bit for bit, (b) per element within the bound, (c) ids nobody chose exactly +0 ((d): out-of-range ids are in neither reference)"""
    c = make_emb_bwd(*case)
    ref, bound, hits = ref_emb_bwd(*case)
    got = got.detach().cpu()
    same_bits("d_emb vs the ascending fp32 sum", got, emb_bwd_seq(c) if seq is None else seq)
    check("d_emb", got, ref, bound, st)
    idle = got[hits == 0]
    same_bits("d_emb of ids nobody chose (+0)", idle, torch.zeros_like(idle))


def test_embed_bwd_checker_cpu():
    st = Stats()
    for case in EMB_BWD_ID + EMB_BWD_ROWS:
        rows, C, V, D, kind = case
        assert (V > 4 * rows and rows > 0) == (case in EMB_BWD_ROWS)
        check_emb_bwd(case, emb_bwd_seq(make_emb_bwd(*case)), st)
    st.show("embedding backward (emulation)")
    assert {k[3] for k in EMB_BWD_ID} >= {8, 2048, 2056, 4096, 16384} and {k[0] for k in EMB_BWD_ID} == {0, 1, 255, 256, 257, 16384, 16385, 20000}
    c = make_emb_bwd(16385, 2, 5, 8, "late")
    assert bool((c["tok"][:, 0] == 2).all()) and int((c["tok"][:, 1] == 4).nonzero()[0]) == EMB_PASS
    c = make_emb_bwd(16385, 2, 65541, 8, "late")
    assert int((c["tok"][:, 1] == 65540).nonzero()[0]) == EMB_PASS and int(c["tok"][3, 0]) == int(c["tok"][EMB_PASS, 0])
    for case, bug in (((255, 2, 19, 4096, ""), "q = 1 chunk zero"), ((257, 1, 1500, 4096, "own"), "q = 1 chunk zero"),
                      ((16385, 2, 5, 8, "late"), "second pass missing"), ((16385, 2, 65541, 8, "late"), "second pass missing"),
                      ((20000, 2, 11, 64, "late"), "second pass missing"), ((257, 1, 3, 8, "order"), "descending"),
                      ((257, 3, 19, 2048, ""), "clamped"), ((600, 2, 5000, 64, "own"), "clamped")):
        bad = emb_bwd_seq(make_emb_bwd(*case), bug)
        _rejects(lambda: check_emb_bwd(case, bad, Stats()))
    c = make_emb_bwd(257, 1, 3, 8, "order")
    assert float(emb_bwd_seq(c)[0, 1, 0]) == 255.0 and float(emb_bwd_seq(c, "descending")[0, 1, 0]) == 256.0
    for rows, C, V, Vp, D in EMB_BWD_PAIR:
        assert V <= 4 * rows < Vp


# ================================================================================================ 4. input jitter
NOISE_N = (0, 8, 8 * 257, 8 * (4096 * 256 + 300))


@functools.lru_cache(maxsize=None)
def make_noise(n, arbitrary):
    g = gen(51000 + n % 9973 + arbitrary)
    x = torch.randn(n, generator=g).to(bf16)
    if arbitrary:
        nz = torch.randn(n, generator=g) * 3
        if n >= 8:
            nz[0], nz[1], nz[2], nz[n - 1] = 0.0, -1.5, -0.0, -2.0 ** -130
    else:
        nz = torch.empty(n).uniform_(0.99, 1.01, generator=g)
    return x, nz


def ref_noise(x, nz):
    return (x.float() * nz).to(bf16)


def test_mul_noise_checker_cpu():
    x, nz = make_noise(8 * 257, True)
    want = ref_noise(x, nz)
    same_bits("y", to_bf(rbf(x.to(f64) * nz.to(f64))), want)          # the fp32 product is rounded once more: float64 agrees off midpoints
    bad = want.clone()
    bad[-8:] = SENT                                                     # the last chunk not written
    _rejects(lambda: same_bits("y", bad, want))
    _rejects(lambda: same_bits("y", (x * nz.to(bf16)), want))           # the noise rounded to bf16 first
    assert NOISE_N[3] // 8 > 4096 * 256 and NOISE_N[3] // 8 < 2 * 4096 * 256


# ================================================================================================ 5. mRoPE backward
ROPE_POS = 3000
ROPE_GEOMS = [(16, 2, 128, (16, 24, 24)), (4, 4, 64, (8, 12, 12)), (2, 1, 128, (16, 24, 24)), (16, 1, 128, (64, 0, 0))]
ROPE_CASES = [g + (B, T) for g in ROPE_GEOMS for B in (1, 3) for T in (1, 17)]


@functools.lru_cache(maxsize=None)
def make_rope(idx):
    H, KVH, hd, sec, B, T = ROPE_CASES[idx]
    g = gen(61000 + idx)
    n_tok, half, Lmax = B * T, hd // 2, T + 8
    dq = torch.randn(n_tok, H * hd, generator=g).to(bf16)
    kv_pos = torch.cat([torch.randperm(Lmax, generator=g)[:T] for _ in range(B)]).to(torch.int32)     # a permutation per row, Lmax > T
    row = torch.arange(n_tok) // T
    dk = torch.full((B, KVH, Lmax, hd), NAN).to(bf16)                                                  # NaN in every slot nobody names
    dv = torch.full((B, KVH, Lmax, hd), NAN).to(bf16)
    dk[row, :, kv_pos.long()] = torch.randn(n_tok, KVH, hd, generator=g).to(bf16)
    dv[row, :, kv_pos.long()] = torch.randn(n_tok, KVH, hd, generator=g).to(bf16)
    cos = (2 * torch.rand(ROPE_POS, half, generator=g) - 1).to(bf16)            # (not cos and sin of anything: every entry its own value)
    sin = (2 * torch.rand(ROPE_POS, half, generator=g) - 1).to(bf16)
    pos3 = torch.randint(0, ROPE_POS - 2000, (3, n_tok), generator=g)          # three different rows
    pos3[1] = pos3[0] + 1 + torch.randint(0, 900, (n_tok,), generator=g)
    pos3[2] = pos3[1] + 1 + torch.randint(0, 900, (n_tok,), generator=g)
    pos3[2, 0] = ROPE_POS - 1
    return dict(H=H, KVH=KVH, hd=hd, sec=sec, B=B, T=T, n_tok=n_tok, Lmax=Lmax, dq=dq, dk=dk, dv=dv, cos=cos, sin=sin,
                pos3=pos3.to(torch.int32).contiguous(), kv_pos=kv_pos)


def rope_bwd_parts(c, dt, bug=None):
    """y [n_tok, H + KVH, hd] gathered from dq and the named slots of dk, v from dv, cos / sin per (token, i); dt the arithmetic"""
    H, KVH, hd, (s0, s1, _), T = c["H"], c["KVH"], c["hd"], c["sec"], c["T"]
    n_tok, half = c["n_tok"], hd // 2
    i = torch.arange(half)
    b0 = s0 + (1 if bug == "section boundary off by one" else 0)
    stream = (i >= b0).long() + (i >= s0 + s1).long()
    pos = c["pos3"].long()[stream, :].t()                                        # [n_tok, half]
    cs, sn = c["cos"].to(dt)[pos, i[None]][:, None], c["sin"].to(dt)[pos, i[None]][:, None]
    row = torch.arange(n_tok) // T
    slot = (torch.arange(n_tok) % T) if bug == "dk at slot t" else c["kv_pos"].long()
    y = torch.cat([c["dq"].view(n_tok, H, hd), c["dk"][row, :, slot]], 1).to(dt)
    return y[..., :half], y[..., half:], cs, sn, c["dv"][row, :, c["kv_pos"].long()].to(dt)


def rope_bwd_chain(c, dt, bug=None):
    """d = y c - rot(y) s with rot(y) = (-y2, y1): lower half bf16(bf16(y1 c) - bf16(-y2 s)), upper half bf16(bf16(y2 c) - bf16(y1 s)); the
    products of two bf16 values are exact in fp32 (and float64), the difference of two bf16 values is one IEEE operation; V copied"""
    y1, y2, cs, sn, v = rope_bwd_parts(c, dt, bug)
    up = 1.0 if bug == "rot sign on the upper half" else -1.0
    lo, hi = rbf(rbf(y1 * cs) - rbf(-y2 * sn)), rbf(rbf(y2 * cs) + up * rbf(y1 * sn))
    if bug == "V rotated":
        vh = v.shape[-1] // 2
        v = torch.cat([rbf(rbf(v[..., :vh] * cs) - rbf(-v[..., vh:] * sn)), rbf(rbf(v[..., vh:] * cs) - rbf(v[..., :vh] * sn))], -1)
    return to_bf(torch.cat([torch.cat([lo, hi], -1), v], 1).reshape(c["n_tok"], -1))


@functools.lru_cache(maxsize=None)
def ref_rope_bwd(idx):
    """the float64 rotation dy cos - rot(dy) sin without any rounding, and the bound of the chain's three bf16 roundings:
    2^-8 (|a| + |b|) (1 + 2^-8) for the two products a, b, then 2^-8 |ref| for the result; V exact (bound 0)"""
    c = make_rope(idx)
    y1, y2, cs, sn, v = rope_bwd_parts(c, f64)
    ref = torch.cat([torch.cat([y1 * cs + y2 * sn, y2 * cs - y1 * sn], -1), v], 1).reshape(c["n_tok"], -1)
    ab = torch.cat([torch.cat([(y1 * cs).abs() + (y2 * sn).abs(), (y2 * cs).abs() + (y1 * sn).abs()], -1), torch.zeros_like(v)], 1)
    rot = torch.cat([torch.ones_like(ab[:, :c["H"] + c["KVH"]]), torch.zeros_like(v)], 1).reshape(c["n_tok"], -1)
    return ref, BF * (1 + BF) * ab.reshape(c["n_tok"], -1) + BF * ref.abs() * rot


def check_rope_bwd(idx, got, st):
    c = make_rope(idx)
    same_bits("dqkv vs the fp32 chain", got, rope_bwd_chain(c, f32))
    check("dqkv", got, *ref_rope_bwd(idx), st)


def test_rope_bwd_checker_cpu():
    st = Stats()
    for idx in range(len(ROPE_CASES)):
        c = make_rope(idx)
        assert c["Lmax"] > c["T"] and (c["T"] == 1 or not torch.equal(c["kv_pos"][:c["T"]].long(), torch.arange(c["T"])))
        assert not torch.equal(c["pos3"][0], c["pos3"][1]) and not torch.equal(c["pos3"][1], c["pos3"][2])
        same_bits("fp32 chain vs float64 chain", rope_bwd_chain(c, f32), rope_bwd_chain(c, f64))
        check_rope_bwd(idx, rope_bwd_chain(c, f32), st)
    st.show("mRoPE backward (emulation)")
    for idx in (3, 7, 11):                                       # B = 3, T = 17 of three geometries with more than one section
        c = make_rope(idx)
        for bug in ("rot sign on the upper half", "section boundary off by one", "dk at slot t", "V rotated"):
            _rejects(lambda: check_rope_bwd(idx, rope_bwd_chain(c, f32, bug), Stats()))
            if bug != "dk at slot t":                             # (that one reads NaN; the others the bound rule rejects alone, too)
                _rejects(lambda: check("dqkv", rope_bwd_chain(c, f32, bug), *ref_rope_bwd(idx), Stats()))


# ================================================================================================ GPU tests
def _abi():
    import ctypes as C
    from unimoe_audio_amd import _lib as L
    return C, L, L.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t, off=0):
    import ctypes as C
    return C.c_void_p(0 if t is None else t.data_ptr() + off)


def owned(n, dtype, dev, fill=SENT):
    """a buffer of n elements the caller owns, filled with `fill`, with TAIL sentinels behind it -> (whole buffer, the n elements)"""
    buf = torch.full((n + TAIL,), SENT, dtype=dtype, device=dev)
    buf[:n] = fill
    return buf, buf[:n]


def tail_kept(name, buf, n):
    same_bits(name + ": the sentinels behind it", buf[n:], torch.full((TAIL,), SENT, dtype=buf.dtype))


def _unchanged(name, on_dev, on_cpu):
    same_bits(name + " (an input)", on_dev, on_cpu)


@gpu
@pytest.mark.parametrize("idx", range(len(CE_CASES)))
def test_ce_vs_fp64(dev, idx):
    """umoe_codec_ce_fwd + umoe_codec_ce_bwd at CE_CASES[idx]: nll_ws, probs, ch_loss, ch_count, total and dlogits per element under the
    bounds of ref_ce, then the forward alone with probs = NULL; nothing written behind any of the six buffers."""
    C_, L, lib, s = _abi()
    c, r = make_ce(idx), ref_ce(idx)
    N, C, V = c["N"], c["C"], c["V"]
    x, lab = c["x"].to(dev), c["lab"].to(dev)
    st = Stats()
    for with_probs in (True, False):
        nll_b, nll = owned(N * C, f32, dev)
        pr_b, pr = owned(N * C * V, f32, dev)
        cl_b, cl = owned(C, f32, dev)
        cc_b, cc = owned(C, torch.int32, dev)
        tt_b, tt = owned(1, f32, dev)
        dl_b, dl = owned(N * C * V, f32, dev)
        L.check(lib.umoe_codec_ce_fwd(_p(x), _p(lab), N, C, V, _p(nll), _p(pr) if with_probs else _p(None), _p(cl), _p(cc), _p(tt), s),
                "umoe_codec_ce_fwd")
        if with_probs:
            L.check(lib.umoe_codec_ce_bwd(_p(pr), _p(lab), _p(cc), N, C, V, C_.c_float(c["grad"]), _p(dl), s), "umoe_codec_ce_bwd")
        torch.cuda.synchronize()
        o = dict(nll=nll.view(N, C), probs=pr.view(N, C, V) if with_probs else None, ch_loss=cl, ch_count=cc, total=tt,
                 dl=dl.view(N, C, V) if with_probs else None)
        check_ce(r, o, st)
        for name, b, n in (("nll_ws", nll_b, N * C), ("probs", pr_b, N * C * V), ("ch_loss", cl_b, C), ("ch_count", cc_b, C), ("total", tt_b, 1),
                           ("dlogits", dl_b, N * C * V)):
            tail_kept(name, b, n)
        if not with_probs:
            same_bits("probs with probs = NULL", pr, torch.full((N * C * V,), SENT))
    _unchanged("logits", x, c["x"])
    st.show(f"cross-entropy case {idx} {CE_CASES[idx]}")


@gpu
def test_ce_through_ops(dev):
    """ops.codec_ce (grad = 1) returns what the C ABI returns: the same checks at the training-like case"""
    from unimoe_audio_amd import ops
    idx = 12
    c, r = make_ce(idx), ref_ce(idx)
    assert c["grad"] == 1.0
    total, ch_loss, ch_cnt, dl = ops.codec_ce(c["x"].to(dev), c["lab"].to(dev), want_grad=True)
    st = Stats()
    check("ch_loss", ch_loss, r["loss"], r["e_ch"], st)
    check("total", total.reshape(1), r["total"], r["e_tot"], st)
    check("dlogits", dl, r["dl"], r["e_dl"], st)
    assert torch.equal(ch_cnt.cpu().long(), r["cnt"])
    st.show("ops.codec_ce")


def _run_aux(dev, c, form):
    C_, L, lib, s = _abi()
    lg, mk = c["logits"].to(dev), c["mask"].to(dev)
    tw = None if c["tw"] is None else c["tw"].to(dev)
    out = torch.full((3,), SENT, dtype=f32, device=dev)
    if form == "one":
        L.check(lib.umoe_aux_loss_fwd(_p(lg), int(c["isbf"]), _p(mk), _p(tw), c["S"], c["E"], c["n_dyn"], _p(out, 4), s), "umoe_aux_loss_fwd")
    else:
        n = int(lib.umoe_aux_loss_workspace_floats())
        ws_b, _ = owned(n, f32, dev, NAN)
        L.check(lib.umoe_aux_loss_fwd_ws(_p(lg), int(c["isbf"]), _p(mk), _p(tw), c["S"], c["E"], c["n_dyn"], _p(out, 4), _p(ws_b), s),
                "umoe_aux_loss_fwd_ws")
        torch.cuda.synchronize()
        tail_kept("the aux workspace", ws_b, n)
    torch.cuda.synchronize()
    same_bits("beside out", out[[0, 2]], torch.full((2,), SENT))
    _unchanged("logits", lg, c["logits"])
    return float(out[1])


@gpu
@pytest.mark.parametrize("S", AUX_S)
def test_aux_loss_vs_fp64(dev, S):
    """umoe_aux_loss_fwd and umoe_aux_loss_fwd_ws at the four cases of aux_cases(S), each held to the interval and bound of ref_aux for its
    own summation depth (they are re-associations of each other: neither is held to the other); NaN in the logit columns past n_dyn and
    in the workspace before the launch, sentinels behind the workspace and on both sides of out."""
    st = Stats()
    for case in aux_cases(S):
        c = make_aux(*case)
        for form in ("one", "ws"):
            r = ref_aux(case, form)
            assert r[3] <= CAP
            check_aux(f"{form} E={case[1]} n_dyn={case[2]} {'bf16' if case[3] else 'fp32'}{' weighted' if case[4] else ''} x{case[5]}",
                      _run_aux(dev, c, form), r, st)
    st.show(f"aux loss S={S}")


@gpu
@pytest.mark.parametrize("case", AUX_OPS)
def test_aux_loss_through_ops(dev, case):
    """ops.aux_loss on both sides of its switch at S = 2048: the one-launch form below, the workspace form from 2048 on"""
    from unimoe_audio_amd import ops
    c = make_aux(*case)
    got = ops.aux_loss(c["logits"].to(dev), c["mask"].to(dev), c["n_dyn"], None if c["tw"] is None else c["tw"].to(dev))
    st = Stats()
    check_aux("ops.aux_loss", float(got), ref_aux(case, "one" if case[0] < 2048 else "ws"), st)
    st.show(f"ops.aux_loss {case}")


@gpu
@pytest.mark.parametrize("idx", range(len(EMB_FWD)))
def test_embed_fwd_bit_for_bit(dev, idx):
    """umoe_codec_embed_sum at EMB_FWD[idx] against the fp32 chain bf16(acc + e) in channel order (the float64 chain gives the same bits on
    this data: emb_exponents_ok), ids -1, -100, V and V + 5 clamped into the table; the sentinels behind out kept."""
    C_, L, lib, s = _abi()
    c = make_emb_fwd(idx)
    rows, C, V, D = EMB_FWD[idx]
    assert emb_exponents_ok(c)
    tok, emb = c["tok"].to(dev), c["emb"].to(dev)
    out_b, out = owned(rows * D, bf16, dev)
    L.check(lib.umoe_codec_embed_sum(_p(tok), _p(emb), rows, C, V, D, _p(out), s), "umoe_codec_embed_sum")
    torch.cuda.synchronize()
    same_bits("out", out.view(rows, D), emb_chain(c, f32))
    same_bits("out vs the float64 chain", out.view(rows, D), emb_chain(c, f64))
    tail_kept("out", out_b, rows * D)
    _unchanged("emb", emb, c["emb"])
    print(f"\nLOSS FP64 embedding forward case {idx} {EMB_FWD[idx]}: bit for bit")


def _run_emb_bwd(dev, c, V=None):
    C_, L, lib, s = _abi()
    rows, C, D = c["rows"], c["C"], c["D"]
    V = c["V"] if V is None else V
    tok, dy = c["tok"].to(dev), c["dy"].to(dev)
    de_b, de = owned(C * V * D, bf16, dev)
    L.check(lib.umoe_codec_embed_sum_bwd(_p(tok), _p(dy), rows, C, V, D, _p(de), s), "umoe_codec_embed_sum_bwd")
    torch.cuda.synchronize()
    tail_kept("d_emb", de_b, C * V * D)
    _unchanged("d_out", dy, c["dy"])
    return de.view(C, V, D)


@gpu
@pytest.mark.parametrize("case", EMB_BWD_ID + EMB_BWD_ROWS)
def test_embed_bwd_vs_fp64(dev, case):
    """umoe_codec_embed_sum_bwd, the per-id kernel (EMB_BWD_ID) and the rows kernel (EMB_BWD_ROWS): (a) bit for bit against the ascending
    fp32 sum, (b) per element within 2^-8 |ref| + (1 + 2^-8) n u sum|terms|, (c) ids nobody chose +0, (d) out-of-range ids nowhere."""
    st = Stats()
    check_emb_bwd(case, _run_emb_bwd(dev, make_emb_bwd(*case)), st)
    st.show(f"embedding backward {case}")


@gpu
@pytest.mark.parametrize("rows,C,V,Vp,D", EMB_BWD_PAIR)
def test_embed_bwd_kernels_agree(dev, rows, C, V, Vp, D):
    """(e): the same tok / d_out through the per-id kernel (V <= 4 rows) and, with the table padded to Vp > 4 rows, through the rows
    kernel: the shared table rows bit for bit, the padding +0."""
    c = make_emb_bwd(rows, C, V, D, "late" if rows > EMB_PASS else "")
    c = dict(c, tok=torch.where(c["tok"] >= V, c["tok"] - V + Vp, c["tok"]))      # V and V + 5 become Vp and Vp + 5: outside both tables
    a, b = _run_emb_bwd(dev, c), _run_emb_bwd(dev, c, Vp)
    same_bits("rows kernel vs per-id kernel", b[:, :V], a)
    same_bits("padding (+0)", b[:, V:], torch.zeros(C, Vp - V, D, dtype=bf16))
    same_bits("per-id kernel vs the ascending fp32 sum", a, emb_bwd_seq(c))


@gpu
def test_embed_bwd_refuses_wide_rows(dev):
    """D = 16392 (a ninth chunk per thread) is refused and nothing is written"""
    C_, L, lib, s = _abi()
    rows, C, V, D = 3, 1, 2, 16392
    tok = torch.zeros(rows, C, dtype=torch.int32, device=dev)
    dy = torch.ones(rows, D, dtype=bf16, device=dev)
    de_b, de = owned(C * V * D, bf16, dev)
    with pytest.raises(L.UmoeError):
        L.check(lib.umoe_codec_embed_sum_bwd(_p(tok), _p(dy), rows, C, V, D, _p(de), s), "umoe_codec_embed_sum_bwd")
    torch.cuda.synchronize()
    same_bits("d_emb after the refused call", de_b, torch.full((C * V * D + TAIL,), SENT, dtype=bf16))


@gpu
def test_empty_inputs_through_ops(dev):
    """no rows: ops.codec_embed_sum and ops.mul_noise return empty tensors, ops.codec_embed_sum_bwd a table gradient of +0 (the pointers
    of empty tensors are null: the launchers must not refuse them)"""
    from unimoe_audio_amd import ops
    C, V, D = 2, 5, 64
    tok = torch.zeros(0, C, dtype=torch.int32, device=dev)
    emb = torch.ones(C, V, D, dtype=bf16, device=dev)
    assert ops.codec_embed_sum(tok, emb).shape == (0, D)
    same_bits("d_emb", ops.codec_embed_sum_bwd(tok, torch.zeros(0, D, dtype=bf16, device=dev), V), torch.zeros(C, V, D, dtype=bf16))
    assert ops.mul_noise(torch.zeros(0, D, dtype=bf16, device=dev), torch.zeros(0, D, device=dev)).shape == (0, D)


@gpu
def test_embed_autograd_at_4096(dev):
    """train.CodecEmbedFn and train.EmbedFn once at D = 4096 through .backward(): the forward bit for bit (placeholder ids -1 read row 0),
    the table gradients bit for bit against the ascending fp32 sum, id -1 contributing nowhere."""
    from unimoe_audio_amd import train as TR
    rows, C, V, D = 37, 2, 19, 4096
    g = gen(43000)
    tok = torch.randint(0, V, (rows, C), generator=g)
    dy = torch.randn(rows, D, generator=g).to(bf16)
    t = EMB_EMIN + (EMB_EMAX - EMB_EMIN) * torch.rand(C, V, D, generator=g)
    emb = torch.exp2(t).to(bf16)
    c = dict(rows=rows, C=C, V=V, D=D, tok=tok.to(torch.int32), dy=dy, emb=emb)
    tabs = [emb[ch].to(dev).requires_grad_(True) for ch in range(C)]
    out = TR.CodecEmbedFn.apply(tok.to(dev), *tabs)
    same_bits("CodecEmbedFn forward", out, emb_chain(c, f32))
    out.backward(dy.to(dev))
    want = emb_bwd_seq(c)
    for ch in range(C):
        same_bits(f"CodecEmbedFn table gradient {ch}", tabs[ch].grad, want[ch])
    Vt = 1027                                                   # V > 4 rows: the rows kernel
    ids = torch.randint(0, Vt, (1, rows), generator=g)
    ids[0, ::5] = -1                                            # placeholder positions, as forward_train marks them
    ids[0, 7] = ids[0, 3]
    tab = torch.randn(Vt, D, generator=g).to(bf16)
    tab_d = tab.to(dev).requires_grad_(True)
    e = TR.EmbedFn.apply(ids.to(dev), tab_d)
    same_bits("EmbedFn forward", e, tab[ids.clamp(min=0)])
    e.backward(dy.to(dev).reshape(1, rows, D))
    ct = dict(rows=rows, C=1, V=Vt, D=D, tok=ids.reshape(rows, 1).to(torch.int32), dy=dy)
    same_bits("EmbedFn table gradient", tab_d.grad, emb_bwd_seq(ct)[0])


@gpu
@pytest.mark.parametrize("n,arbitrary", [(n, False) for n in NOISE_N] + [(8 * 257, True)])
def test_mul_noise_bit_for_bit(dev, n, arbitrary):
    """umoe_mul_noise == (x.float() * noise).to(bfloat16) bit for bit at NOISE_N (the last: every thread of the 4096-workgroup grid strides
    once, 300 of them twice), noise in [0.99, 1.01] or arbitrary fp32 with 0, -0, a negative value and a subnormal; sentinels behind y."""
    C_, L, lib, s = _abi()
    x, nz = make_noise(n, arbitrary)
    if not arbitrary and n:
        assert 0.99 <= float(nz.min()) and float(nz.max()) <= 1.01
    xd, nd = x.to(dev), nz.to(dev)                               # (n = 0: empty tensors, their pointers null)
    y_b, y = owned(n, bf16, dev)
    L.check(lib.umoe_mul_noise(_p(xd), _p(nd), n, _p(y_b), s), "umoe_mul_noise")
    torch.cuda.synchronize()
    same_bits("y", y, ref_noise(x, nz))
    tail_kept("y", y_b, n)
    print(f"\nLOSS FP64 jitter n={n}{' arbitrary noise' if arbitrary else ''}: bit for bit")


@gpu
def test_mul_noise_refusals(dev):
    """a pointer that is not 16-byte aligned (x, noise or y) and n % 8 != 0 are refused; nothing is written"""
    C_, L, lib, s = _abi()
    x = torch.ones(64, dtype=bf16, device=dev)
    nz = torch.ones(64, device=dev)
    y_b, y = owned(32, bf16, dev)
    for args in ((_p(x, 2), _p(nz), 16, _p(y_b)), (_p(x), _p(nz, 4), 16, _p(y_b)), (_p(x), _p(nz), 16, _p(y_b, 2)), (_p(x), _p(nz), 12, _p(y_b))):
        with pytest.raises(L.UmoeError):
            L.check(lib.umoe_mul_noise(*args, s), "umoe_mul_noise")
    torch.cuda.synchronize()
    same_bits("y after refused calls", y_b, torch.full((32 + TAIL,), SENT, dtype=bf16))


def _rope_args(c, d, sec=None):
    C_, L, lib, s = _abi()
    sec = c["sec"] if sec is None else sec
    return L.RopeArgs(qkv=None, cos_tab=d["cos"].data_ptr(), sin_tab=d["sin"].data_ptr(), pos3=d["pos3"].data_ptr(), kv_pos=d["kv_pos"].data_ptr(),
                      n_tok=c["n_tok"], T=c["T"], H=c["H"], KVH=c["KVH"], hd=c["hd"], sec0=sec[0], sec1=sec[1], sec2=sec[2], Lmax=c["Lmax"],
                      q_out=None, k_cache=None, v_cache=None)


@gpu
@pytest.mark.parametrize("idx", range(len(ROPE_CASES)))
def test_rope_bwd_vs_fp64(dev, idx):
    """umoe_qkv_mrope_bwd at ROPE_CASES[idx]: bit for bit against the fp32 chain bf16(bf16(y c) - bf16(rot(y) s)), and per element against
    the unrounded float64 rotation within the chain's three bf16 roundings; three different position rows, kv_pos a permutation per row,
    Lmax = T + 8, NaN in every slot of dk / dv that no kv_pos names; the sentinels behind dqkv kept."""
    C_, L, lib, s = _abi()
    c = make_rope(idx)
    d = {n: c[n].to(dev) for n in ("dq", "dk", "dv", "cos", "sin", "pos3", "kv_pos")}
    n = c["n_tok"] * (c["H"] + 2 * c["KVH"]) * c["hd"]
    out_b, out = owned(n, bf16, dev)
    a = _rope_args(c, d)
    L.check(lib.umoe_qkv_mrope_bwd(C_.byref(a), _p(d["dq"]), _p(d["dk"]), _p(d["dv"]), _p(out), s), "umoe_qkv_mrope_bwd")
    torch.cuda.synchronize()
    st = Stats()
    check_rope_bwd(idx, out.view(c["n_tok"], -1), st)
    tail_kept("dqkv", out_b, n)
    for name in ("dq", "dk", "dv"):
        _unchanged(name, d[name], c[name])
    st.show(f"mRoPE backward case {idx} {ROPE_CASES[idx]}")


@gpu
def test_rope_bwd_refusals(dev):
    """sections that do not sum to hd / 2 are refused and nothing is written; n_tok = 0 is a success that writes nothing"""
    C_, L, lib, s = _abi()
    c = make_rope(3)
    d = {n: c[n].to(dev) for n in ("dq", "dk", "dv", "cos", "sin", "pos3", "kv_pos")}
    n = c["n_tok"] * (c["H"] + 2 * c["KVH"]) * c["hd"]
    out_b, out = owned(n, bf16, dev)
    a = _rope_args(c, d, (16, 24, 23))
    with pytest.raises(L.UmoeError):
        L.check(lib.umoe_qkv_mrope_bwd(C_.byref(a), _p(d["dq"]), _p(d["dk"]), _p(d["dv"]), _p(out), s), "umoe_qkv_mrope_bwd")
    a = _rope_args(c, d)
    a.n_tok = 0
    L.check(lib.umoe_qkv_mrope_bwd(C_.byref(a), _p(d["dq"]), _p(d["dk"]), _p(d["dv"]), _p(out), s), "umoe_qkv_mrope_bwd")
    torch.cuda.synchronize()
    same_bits("dqkv after a refused and an empty call", out_b, torch.full((n + TAIL,), SENT, dtype=bf16))
