"""GPU parity tests (run with -m gpu on an MI355X): every HIP op, called through the C-ABI, against the
CPU oracle (oracle/*) on the same seeded inputs, plus the golden fixtures generated from the reference.

Bar: bit-exact for integer outputs (k, expert ids/order, masks, dispatch tables, arg-max codes); stated
tolerances for bf16/fp32 tensors.
"""
import glob
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

BF16_TOL = dict(rtol=2 ** -6, atol=2 ** -8)      # ~2 bf16 ulps relative + small absolute (accumulation order differs)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from unimoe_audio_amd import _lib
    _lib.lib()                                    # raises if the HIP library is missing: no silent fallback
    return torch.device("cuda:0")


def _ref_linear(x, w, bias=None):
    y = x.float() @ w.float().t()
    if bias is not None:
        y = y + bias.float()
    return y


# ----------------------------------------------------------------------------- GEMM family
@pytest.mark.parametrize("S,K,N", [(300, 2048, 2560), (129, 2752, 2048), (128, 1376, 2048), (1, 64, 8), (257, 72, 130),
                                   (640, 2048, 12324),
                                   # >= 1024 rows and >= 128 tiles of 256 x 256: the ping-pong variant (K tail, ragged last tiles)
                                   (2048, 520, 4000), (2300, 256, 3600)])
def test_tiled_gemm_plain_bias_resid_f32(dev, S, K, N):
    """umoe_tiled_gemm (row-major weights, 128x128x64 MFMA tiles) against an fp32 torch reference with the reference's
    rounding points: Linear output rounded to bf16, then bias-free residual add rounded again."""
    from unimoe_audio_amd import ops
    g = torch.Generator().manual_seed(S * 7 + K + N)
    x = (torch.randn(S, K, generator=g) * 1.5).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) * 0.03).to(torch.bfloat16)
    b = torch.randn(N, generator=g) * 0.1
    r = torch.randn(S, N, generator=g).to(torch.bfloat16)
    xd, wd, bd, rd = x.to(dev), w.to(dev), b.to(dev), r.to(dev)
    ref = _ref_linear(x, w, b)
    y = ops.tlinear(xd, wd, bias=bd).cpu()
    torch.testing.assert_close(y.float(), ref.to(torch.bfloat16).float(), **BF16_TOL)
    y2 = ops.tlinear(xd, wd, resid=rd).cpu()
    ref2 = (r.float() + _ref_linear(x, w).to(torch.bfloat16).float()).to(torch.bfloat16)
    # a 1-ulp flip of the rounded Linear output survives the residual add unscaled: bound it by the ulp of the addends
    lin = _ref_linear(x, w)
    assert (y2.float() - ref2.float()).abs().max() <= 2 ** -7 * max(float(lin.abs().max()), float(r.float().abs().max()))
    assert ((y2.float() - ref2.float()).abs() > 2 ** -8 * (1 + ref2.float().abs())).float().mean() < 1e-3
    y3 = ops.tlinear(xd, wd, out_f32=True).cpu()
    torch.testing.assert_close(y3, _ref_linear(x, w).to(torch.bfloat16).float(), **BF16_TOL)
    # same numbers as the weight-streaming kernel up to accumulation order (both round the fp32 sum once)
    if K % 32 == 0 and S <= 300:
        y4 = ops.linear(xd, ops.pack_weight(wd), N, bias=bd).cpu()
        assert (y4.float() - y.float()).abs().max() <= 2 ** -6 * ref.abs().max()


@pytest.mark.parametrize("T,M,N,G,ksplit", [(6240, 2560, 2048, 1, 1),       # dense weight gradient (QKV), full training width
                                            (1000, 264, 520, 1, 1),        # ragged last tiles, K tail (1000 = 31 * 32 + 8)
                                            (31, 256, 256, 1, 1),          # fewer rows than one K tile
                                            (4099, 1376, 2048, 2, 1),      # two static groups with windows of their own
                                            (6240, 2048, 2048, 1, 3),      # K split with the fixed-order fp32 reduction
                                            (5000, 528, 264, 1, 4),
                                            (520, 2816, 3072, 1, 1),       # 132 tiles: the transposed-copy path runs the 256 x 256 kernel too
                                            (1304, 12324, 256, 1, -1)])    # m not a multiple of 8 (codec head), split chosen by the library
def test_tiled_gemm_tn_static_windows(dev, T, M, N, G, ksplit):
    """umoe_tiled_gemm_tn: out[m][n] = sum_k P[k][m] Q[k][n] straight from row-major activations (transposing LDS reads) against an fp32
    torch reference, and BIT-IDENTICAL to umoe_tiled_gemm over transposed copies when the window is not split (same K tiles of 32 rows in
    the same order; inside a tile the MFMA adds the same 32 products)."""
    from unimoe_audio_amd import ops
    g = torch.Generator().manual_seed(T + M + N)
    Pm = (torch.randn(G * T, ((M + 7) & ~7) + 16, generator=g) * 0.5).to(torch.bfloat16).to(dev)     # operands are column windows of wider buffers
    Qm = (torch.randn(G * T, N + 8, generator=g) * 0.5).to(torch.bfloat16).to(dev)
    out = torch.full((G * M, N), 7.0, dtype=torch.bfloat16, device=dev)
    groups = [dict(m=M, n=N, p_col_off=8, q_col_off=8, k_off=i * T, k=T, out_row_base=i * M) for i in range(G)]
    ops.tiled_gemm_tn(groups, Pm, Qm, out, k_split=ksplit)
    for i in range(G):
        Pg, Qg = Pm[i * T:(i + 1) * T, 8:8 + M], Qm[i * T:(i + 1) * T, 8:8 + N]
        ref = Pg.float().t() @ Qg.float()
        got = out[i * M:(i + 1) * M].float()
        scale = float(ref.abs().max())
        assert (got - ref).abs().max() <= 2 ** -7 * scale + 1e-3, (i, float((got - ref).abs().max()), scale)
        if ksplit == 1 and T % 8 == 0 and M % 8 == 0:
            nt = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
            ops.tiled_gemm([dict(w=ops.transpose(Qg.contiguous()), static_count=M)], ops.transpose(Pg.contiguous()), nt, max_rows=M)
            if M >= 1024 and -(-M // 256) * -(-N // 256) >= 128:   # the 256 x 256 ping-pong kernel ran: same K tiles, same k slots
                assert torch.equal(nt, out[i * M:(i + 1) * M])
            else:
                assert (nt.float() - got).abs().max() <= 2 ** -7 * scale + 1e-3


@pytest.mark.parametrize("S,K,N,k1", [(6240, 2560, 2048, 0),          # dX of the QKV projection at the training width
                                      (300, 12324, 2048, 0),          # codec head: contraction length not a multiple of 8 (zero-padded dY)
                                      (1100, 11, 2048, 0),            # router gate: 11 experts in 16 padded columns
                                      (2304, 704, 3584, 352),         # (dG | dU) against Wg then Wu: the contraction continues in a second matrix
                                      (2600, 520, 264, 0)])
def test_tiled_gemm_kmajor_weights(dev, S, K, N, k1):
    """umoe_tiled_gemm with umoe_tgroup_t.w_kmajor: Y = A W on a weight whose ROW is the contraction index (dX = dY W on an nn.Linear
    weight as stored) against an fp32 reference, and bit-identical to the same product on a transposed copy where that runs the 256 x 256
    kernel as well."""
    from unimoe_audio_amd import ops
    g = torch.Generator().manual_seed(S + K + N)
    K8 = (K + 7) & ~7
    a = torch.zeros(S, K8, dtype=torch.bfloat16)
    a[:, :K] = (torch.randn(S, K, generator=g) * 0.5).to(torch.bfloat16)
    w = (torch.randn(K, N, generator=g) * 0.05).to(torch.bfloat16)
    ad, wd = a.to(dev), w.to(dev)
    out = torch.full((S, N), 5.0, dtype=torch.bfloat16, device=dev)
    if k1:
        w1, w2 = wd[:k1].contiguous(), wd[k1:].contiguous()
        ops.tiled_gemm([dict(w=w1, w2=w2, w_kmajor=1, k=K, k_w1=k1, static_count=S)], ad, out, max_rows=S)
    else:
        ops.tiled_gemm([dict(w=wd, w_kmajor=1, static_count=S)], ad, out, max_rows=S)
    ref = ad[:, :K].float() @ wd.float()                 # (fp32 reference on the device: the host's 256 threads take seconds for it)
    assert (out.float() - ref).abs().max() <= 2 ** -7 * float(ref.abs().max()) + 1e-3
    if K % 8 == 0 and S >= 1024 and -(-S // 256) * -(-N // 256) >= 128:
        nt = ops.tlinear(ad, ops.transpose(wd))
        assert torch.equal(nt, out)


def test_tiled_gemm_kmajor_weights_ragged_groups(dev):
    """k-major weights with the routed experts' row conventions: per-group row offset and count read on the device, rows behind a count
    untouched."""
    from unimoe_audio_amd import ops
    g = torch.Generator().manual_seed(77)
    E, D, I = 4, 512, 352
    counts = [300, 0, 1025, 17]
    offs, tot = [], 0
    for c in counts:
        offs.append(tot)
        tot += (c + 7) & ~7
    dy = (torch.randn(tot, D, generator=g) * 0.5).to(torch.bfloat16).to(dev)
    wd = [(torch.randn(D, I, generator=g) * 0.05).to(torch.bfloat16).to(dev) for _ in range(E)]     # down_proj [D][I]: dH = dY Wd
    cnt = torch.tensor(counts, dtype=torch.int32, device=dev)
    off = torch.tensor(offs, dtype=torch.int32, device=dev)
    out = torch.full((tot, I), 9.0, dtype=torch.bfloat16, device=dev)
    ops.tiled_gemm([dict(w=wd[e], w_kmajor=1, row_off=off[e:e + 1], count=cnt[e:e + 1]) for e in range(E)], dy, out, max_rows=max(counts))
    for e in range(E):
        c, o = counts[e], offs[e]
        if c:
            ref = dy[o:o + c].float() @ wd[e].float()
            assert (out[o:o + c].float() - ref).abs().max() <= 2 ** -7 * float(ref.abs().max()) + 1e-3
        assert bool((out[o + c:o + ((c + 7) & ~7)] == 9.0).all())


def test_tiled_gemm_tn_and_kmajor_random_shapes(dev):
    """Twenty-four seeded random shapes through both k-major kernels (ragged last tiles in every dimension, K tails of every length mod 32,
    column windows, row windows, K splits) against fp32 references on the device."""
    from unimoe_audio_amd import ops
    rng = np.random.default_rng(2024)
    for case in range(24):
        T = int(rng.integers(1, 700))
        M = int(rng.integers(1, 80)) * 8
        N = int(rng.integers(1, 80)) * 8
        po, qo = int(rng.integers(0, 3)) * 8, int(rng.integers(0, 3)) * 8
        k0 = int(rng.integers(0, 40))
        g = torch.Generator().manual_seed(case)
        P = (torch.randn(k0 + T + 3, po + M + 8, generator=g) * 0.5).to(torch.bfloat16).to(dev)
        Q = (torch.randn(k0 + T + 3, qo + N + 16, generator=g) * 0.5).to(torch.bfloat16).to(dev)
        out = torch.full((M, N), 2.0, dtype=torch.bfloat16, device=dev)
        ks = int(rng.choice([1, 1, 2, 3])) if T >= 64 else 1
        ops.tiled_gemm_tn([dict(m=M, n=N, p_col_off=po, q_col_off=qo, k_off=k0, k=T)], P, Q, out, k_split=ks)
        ref = P[k0:k0 + T, po:po + M].float().t() @ Q[k0:k0 + T, qo:qo + N].float()
        assert (out.float() - ref).abs().max() <= 2 ** -7 * float(ref.abs().max()) + 1e-3, ("tn", case, T, M, N, ks)
        # Y = A W with the weight's row as the contraction index: S rows, K = T (any length; A zero-padded to a multiple of 8 columns)
        S = int(rng.integers(1, 600))
        K8 = (T + 7) & ~7
        A = torch.zeros(S, K8, dtype=torch.bfloat16)
        A[:, :T] = (torch.randn(S, T, generator=g) * 0.5).to(torch.bfloat16)
        W = (torch.randn(T, N, generator=g) * 0.1).to(torch.bfloat16)
        Ad, Wd = A.to(dev), W.to(dev)
        y = torch.full((S, N), 4.0, dtype=torch.bfloat16, device=dev)
        ops.tiled_gemm([dict(w=Wd, w_kmajor=1, static_count=S)], Ad, y, max_rows=S)
        ref2 = Ad[:, :T].float() @ Wd.float()
        assert (y.float() - ref2).abs().max() <= 2 ** -7 * float(ref2.abs().max()) + 1e-3, ("kmajor", case, S, T, N)


@pytest.mark.parametrize("E,D,I,counts", [(8, 2048, 2752, [2700, 0, 3111, 8, 1, 2999, 4096, 2048]),
                                          (3, 512, 264, [40, 300, 31])])
def test_tiled_gemm_tn_expert_windows_on_device(dev, E, D, I, counts):
    """The routed experts' weight gradients as ONE grouped launch: per-expert slot windows (offset, count) read on the device, an expert
    without tokens gets zeros, the rows behind a window are never read (they hold NaN here)."""
    from unimoe_audio_amd import ops
    g = torch.Generator().manual_seed(E * 31 + D)
    offs, tot = [], 0
    for c in counts:
        offs.append(tot)
        tot += (c + 7) & ~7                                  # 8-aligned slot ranges (umoe_dispatch_build_aligned)
    dgu = (torch.randn(tot, 2 * I, generator=g) * 0.5).to(torch.bfloat16)
    xe = (torch.randn(tot, D, generator=g) * 0.5).to(torch.bfloat16)
    for c, o in zip(counts, offs):                           # padding rows of a slot range
        dgu[o + c:o + ((c + 7) & ~7)] = float("nan")
        xe[o + c:o + ((c + 7) & ~7)] = float("nan")
    dgu_d, xe_d = dgu.to(dev), xe.to(dev)
    cnt = torch.tensor(counts, dtype=torch.int32, device=dev)
    off = torch.tensor(offs, dtype=torch.int32, device=dev)
    for half in (0, 1):                                      # gate / up halves of (dG | dU)
        out = torch.full((E, I, D), 3.0, dtype=torch.bfloat16, device=dev)
        groups = [dict(m=I, n=D, p_col_off=half * I, k_off_dev=off[e:e + 1], k_count_dev=cnt[e:e + 1], out_row_base=e * I) for e in range(E)]
        ops.tiled_gemm_tn(groups, dgu_d, xe_d, out.view(E * I, D))
        for e in range(E):
            c, o = counts[e], offs[e]
            ref = dgu_d[o:o + c, half * I:(half + 1) * I].float().t() @ xe_d[o:o + c].float()
            got = out[e].float()
            assert torch.isfinite(got).all()
            assert (got - ref).abs().max() <= 2 ** -7 * float(ref.abs().max() if c else 0.0) + 1e-3, (half, e)


@pytest.mark.parametrize("S,D,I,E,p_sel", [(700, 256, 352, 4, 0.4),
                                           (2600, 512, 1024, 8, 0.25)])   # 704 / 176 tiles of 256 x 256: ping-pong variant, ragged order
def test_tiled_gemm_ragged_swiglu_groups(dev, S, D, I, E, p_sel):
    """Routed experts at training-like sizes: ragged row lists (device-side counts / offsets / gather list), SwiGLU
    epilogue from separate gate/up matrices, then the down projection over the slot rows; oracle = oracle.dcmoe.swiglu_mlp."""
    from unimoe_audio_amd import ops
    from oracle import dcmoe as OD
    g = torch.Generator().manual_seed(5)
    x = torch.randn(S, D, generator=g).to(torch.bfloat16)
    mask = (torch.rand(S, E + 3, generator=g) < p_sel).to(torch.int32)
    mask[:, 2] = 0                                   # an expert nobody chose
    wg = [(torch.randn(I, D, generator=g) * 0.06).to(torch.bfloat16) for _ in range(E)]
    wu = [(torch.randn(I, D, generator=g) * 0.06).to(torch.bfloat16) for _ in range(E)]
    wd = [(torch.randn(D, I, generator=g) * 0.06).to(torch.bfloat16) for _ in range(E)]
    xd = x.to(dev)
    disp = ops.dispatch_build(mask.to(dev), E)
    slots = int(disp["offsets"][E].item())
    hbuf = torch.zeros(slots, I, dtype=torch.bfloat16, device=dev)
    ybuf = torch.zeros(slots, D, dtype=torch.bfloat16, device=dev)
    g1 = [dict(w=wg[e].to(dev), w2=wu[e].to(dev), rows=disp["slot_token"], row_off=disp["offsets"][e:e + 1], count=disp["counts"][e:e + 1])
          for e in range(E)]
    g2 = [dict(w=wd[e].to(dev), row_off=disp["offsets"][e:e + 1], count=disp["counts"][e:e + 1]) for e in range(E)]
    ops.tiled_gemm(g1, xd, hbuf, max_rows=S, epilogue=ops.EPI_SWIGLU)
    ops.tiled_gemm(g2, hbuf, ybuf, max_rows=S, epilogue=ops.EPI_BF16)
    st, off, cnt = disp["slot_token"].cpu(), disp["offsets"].cpu(), disp["counts"].cpu()
    assert int(cnt[2]) == 0
    for e in range(E):
        rows = st[int(off[e]): int(off[e]) + int(cnt[e])].long()
        assert torch.equal(rows, torch.nonzero(mask[:, e]).flatten())          # token order preserved
        if rows.numel() == 0:
            continue
        ref = OD.swiglu_mlp(x[rows], wg[e], wu[e], wd[e])
        got = ybuf[int(off[e]): int(off[e]) + int(cnt[e])].cpu()
        err = (got.float() - ref.float()).norm() / ref.float().norm()
        assert err < 2 ** -7, (e, float(err))


@pytest.mark.parametrize("S,K,N", [(16, 2048, 2560), (5, 2048, 2048), (40, 2752, 2048), (16, 1376, 2048),
                                   (16, 2048, 12324), (16, 64, 96), (3, 96, 64), (33, 128, 48)])
def test_linear_plain_bias_resid(dev, S, K, N):
    from unimoe_audio_amd import ops
    torch.manual_seed(S * 7 + K + N)
    x = (torch.randn(S, K) * 0.5).to(torch.bfloat16)
    w = (torch.randn(N, K) * 0.05).to(torch.bfloat16)
    b = torch.randn(N) * 0.1
    r = torch.randn(S, N).to(torch.bfloat16)
    xd, wd = x.to(dev), w.to(dev)
    wp = ops.pack_weight(wd)
    ref = _ref_linear(x, w)
    assert torch.allclose(ops.linear(xd, wp, N).float().cpu(), ref.to(torch.bfloat16).float(), **BF16_TOL)
    y = ops.linear(xd, wp, N, bias=b.to(dev)).float().cpu()
    assert torch.allclose(y, (ref + b).to(torch.bfloat16).float(), **BF16_TOL)
    y = ops.linear(xd, wp, N, resid=r.to(dev)).float().cpu()
    assert torch.allclose(y, (r.float() + ref.to(torch.bfloat16).float()).to(torch.bfloat16).float(), **BF16_TOL)
    y = ops.linear(xd, wp, N, out_f32=True).cpu()
    assert y.dtype == torch.float32
    assert torch.allclose(y, ref.to(torch.bfloat16).float(), **BF16_TOL)


@pytest.mark.parametrize("S,K,N", [(16, 2048, 2560), (7, 128, 64), (16, 2048, 12324)])
def test_linear_rmsnorm_prologue(dev, S, K, N):
    from oracle import decode as OD
    from unimoe_audio_amd import ops
    torch.manual_seed(K + N)
    x = (torch.randn(S, K) * 2.0).to(torch.bfloat16)
    nw = (1 + 0.1 * torch.randn(K)).to(torch.bfloat16)
    w = (torch.randn(N, K) * 0.03).to(torch.bfloat16)
    h = OD.rmsnorm(x, nw, 1e-6)
    ref = _ref_linear(h, w).to(torch.bfloat16).float()
    y = ops.linear(x.to(dev), ops.pack_weight(w.to(dev)), N, norm_w=nw.to(dev), rms_eps=1e-6).float().cpu()
    assert torch.allclose(y, ref, **BF16_TOL)
    yn = ops.rmsnorm(x.to(dev), nw.to(dev), 1e-6).cpu()
    assert torch.allclose(yn.float(), h.float(), rtol=2 ** -7, atol=1e-6)


# ----------------------------------------------------------------------------- router: ints bit-exact
def test_router_ints_vs_reference_goldens(dev):
    """logits in -> (k, ids, order, mask) out, against fixtures produced by the REAL reference."""
    from unimoe_audio_amd import ops
    g = load_golden("router_ids.npz")
    tags = sorted({k.split("__")[0] for k in g})
    total = 0
    for tag in tags:
        lg = g[tag + "__logits"]
        top_p = float(tag.split("_p")[1].split("_k")[0])
        top_k = int(tag.split("_k")[1])
        r = ops.router_fwd(None, None, n_dyn=9, n_real=8, n_fix=2, top_p=top_p, fixed_top_k=top_k, jitter_eps=0.01,
                           logits_in=lg.to(dev))
        assert torch.equal(r["top_k"].cpu(), g[tag + "__top_k"].long()), tag
        assert torch.equal(r["expert_mask"].cpu(), g[tag + "__expert_mask"]), tag
        assert torch.equal(r["sel"].cpu(), g[tag + "__sel"]), tag
        tol = 2 ** -7 if lg.dtype == torch.bfloat16 else 1e-6
        assert torch.allclose(r["global_weight"].cpu(), g[tag + "__global_weight"].float(), rtol=tol, atol=tol * 1e-2), tag
        total += lg.shape[0]
    assert total > 60000


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("scale", [0.05, 0.9, 3.0])
def test_router_ints_vs_oracle_large(dev, dt, scale):
    """1M tokens per case: every integer output AND every weight bit-identical to the C oracle."""
    from oracle import router as OR
    from unimoe_audio_amd import ops
    torch.manual_seed(int(scale * 100) + (1 if dt == torch.float32 else 0))
    S = 1 << 20
    lg = (torch.randn(S, 11) * scale).to(dt)
    lg[::97, 3] = lg[::97, 5]                    # exact ties
    am = (torch.rand(S) > 0.1)
    r = ops.router_fwd(None, None, n_dyn=9, n_real=8, n_fix=2, top_p=0.7, jitter_eps=0.01, logits_in=lg.to(dev),
                       attn_mask=am.to(dev))
    o = OR.route(lg, 9, 8, 2, 0.7, 0, 0.01, am)
    assert torch.equal(r["top_k"].cpu(), o["top_k"])
    assert torch.equal(r["sel"].cpu(), o["sel"])
    assert torch.equal(r["expert_mask"].cpu(), o["expert_mask"])
    assert torch.equal(r["routing_weights"].cpu(), o["routing_weights"].float())
    assert torch.equal(r["global_weight"].cpu(), o["global_weight"].float())
    assert torch.equal(r["moe_weight"].cpu(), o["moe_weight"].float())


def test_router_fused_gate_and_norm(dev):
    """x -> RMSNorm -> gate GEMV -> routing in one kernel: logits to tolerance; ints exact once the oracle is
    fed the logits the GPU produced (the contract of SURVEY.md 7 'hard parts')."""
    from oracle import decode as OD
    from oracle import router as OR
    from unimoe_audio_amd import ops
    torch.manual_seed(5)
    S, D = 777, 2048
    x = torch.randn(S, D).to(torch.bfloat16)
    nw = (1 + 0.05 * torch.randn(D)).to(torch.bfloat16)
    gw = (torch.randn(11, D) * 0.02).to(torch.bfloat16)
    r = ops.router_fwd(x.to(dev), gw.to(dev), n_dyn=9, n_real=8, n_fix=2, top_p=0.7, jitter_eps=0.01, norm_w=nw.to(dev),
                       want_h=True)
    h = OD.rmsnorm(x, nw, 1e-6)
    assert torch.allclose(r["h"].float().cpu(), h.float(), rtol=2 ** -7, atol=1e-6)
    ref_logits = torch.nn.functional.linear(h, gw)
    got = r["logits"].cpu()
    assert torch.allclose(got.float(), ref_logits.float(), rtol=2 ** -6, atol=2 ** -7)
    o = OR.route(got, 9, 8, 2, 0.7, 0, 0.01, None)
    assert torch.equal(r["top_k"].cpu(), o["top_k"]) and torch.equal(r["expert_mask"].cpu(), o["expert_mask"])
    assert torch.equal(r["sel"].cpu(), o["sel"])
    o2 = OR.route(ref_logits, 9, 8, 2, 0.7, 0, 0.01, None)
    mism = int((o2["expert_mask"] != o["expert_mask"]).any(-1).sum())
    assert mism <= S * 0.03, f"index mismatch rate from logit rounding too high: {mism}/{S}"


@pytest.mark.parametrize("S,nd,nf", [(16, 9, 2), (5, 9, 2), (16, 8, 2), (7, 6, 1), (40, 9, 2)])
def test_router_dispatch_fused_equals_two_step(dev, S, nd, nf):
    """The single-launch decode path (S <= 16) must equal router_fwd + dispatch_build bit for bit, and the oracle."""
    from oracle import router as OR
    from unimoe_audio_amd import ops
    torch.manual_seed(S + nd)
    D, nr = 256, min(8, nd)
    x = torch.randn(S, D).to(torch.bfloat16).to(dev)
    gw = (torch.randn(nd + nf, D) * 0.06).to(torch.bfloat16).to(dev)
    nw = (1 + 0.05 * torch.randn(D)).to(torch.bfloat16).to(dev)
    f = ops.router_dispatch_fwd(x, gw, n_dyn=nd, n_real=nr, n_fix=nf, top_p=0.7, norm_w=nw)
    r = ops.router_fwd(x, gw, n_dyn=nd, n_real=nr, n_fix=nf, top_p=0.7, norm_w=nw, want_h=True)
    d = ops.dispatch_build(r["expert_mask"], nr)
    for k in ("logits", "top_k", "sel", "expert_mask", "routing_weights", "global_weight", "moe_weight", "h"):
        assert torch.equal(f[k], r[k]), k
    tot = int(d["offsets"][nr])
    assert torch.equal(f["counts"][:nr], d["counts"][:nr]) and torch.equal(f["offsets"][:nr + 1], d["offsets"][:nr + 1])
    assert torch.equal(f["slot_of"], d["slot_of"]) and torch.equal(f["slot_token"][:tot], d["slot_token"][:tot])
    o = OR.route(f["logits"].cpu(), nd, nr, nf, 0.7, 0, 0.01, None)
    assert torch.equal(f["expert_mask"].cpu(), o["expert_mask"]) and torch.equal(f["sel"].cpu(), o["sel"])
    assert torch.equal(f["global_weight"].cpu(), o["global_weight"].float())


@pytest.mark.parametrize("S", [0, 1, 16, 257, 6240])
def test_dispatch_tables_exact(dev, S):
    from oracle import router as OR
    from unimoe_audio_amd import ops
    torch.manual_seed(S)
    mask = (torch.rand(S, 11) < 0.45).to(torch.int32)
    if S > 3:
        mask[:, 2] = 0
        mask[:, 6] = 1
    d = ops.dispatch_build(mask.to(dev), 8) if S else None
    if S == 0:
        return
    o = OR.dispatch(mask, 8)
    assert torch.equal(d["counts"][:8].cpu(), o["counts"])
    assert torch.equal(d["offsets"][:9].cpu(), o["offsets"])
    assert torch.equal(d["slot_of"].cpu(), o["slot_of"])
    assert torch.equal(d["slot_token"][: o["total"]].cpu(), o["slot_token"])
    x = torch.randn(S, 64).to(torch.bfloat16)
    p = ops.permute_fwd(x.to(dev), d, 8).cpu()
    assert torch.equal(p[: o["total"]], x[o["slot_token"].long()])


# ----------------------------------------------------------------------------- whole DCMoE block
def _mk_block(cfgd, weights, dev):
    from unimoe_audio_amd.dcmoe import UniMoEAudioSparseMoeBlock
    cfg = types.SimpleNamespace(**cfgd)
    blk = UniMoEAudioSparseMoeBlock(cfg)
    sd = {k: v.to(torch.bfloat16) for k, v in weights.items()}
    missing, unexpected = blk.load_state_dict(sd, strict=True), None
    return blk.to(dev).to(torch.bfloat16)


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "dcmoe_bf16_*.npz"))), ids=os.path.basename)
def test_dcmoe_block_vs_reference_goldens(dev, path):
    """The drop-in module (reference parameter names, reference 6-tuple) against outputs of the real reference."""
    from oracle import router as OR
    g = load_golden(os.path.basename(path))
    cfgd = g["cfg_json"]
    w = {k[2:]: v for k, v in g.items() if k.startswith("w.")}
    blk = _mk_block(cfgd, w, dev)
    blk.train(bool(int(g["train"])))
    if "in_input_noise" in g:     # input jitter (core.py:243-244): the samples the reference run was given, injected
        blk._input_noise_inject = g["in_input_noise"]
    am = g.get("in_attention_mask")
    aw = g.get("in_aux_balance_weight")
    with torch.no_grad():
        out = blk(g["in_x"].to(dev), None if am is None else am.to(dev), None if aw is None else aw.to(dev))
    hid, logits, top_k, mask, weight, aux = [o.cpu() for o in out]
    ref_logits = g["out_logits"]
    assert logits.dtype == ref_logits.dtype
    assert torch.allclose(logits.float(), ref_logits.float(), rtol=2 ** -6, atol=2 ** -7)
    n_dyn = cfgd["mlp_dynamic_expert_num"] + cfgd["mlp_dynamic_null_expert_num"]
    n_fix = cfgd["mlp_fixed_expert_num"]
    same = (logits.float() == ref_logits.float()).all(-1)           # tokens whose logits came out bit-identical
    if logits.dtype == torch.bfloat16:                              # fp32 logits differ in the last bits by summation order
        assert same.float().mean() > 0.5
    # for ALL tokens: ints must equal the oracle fed with the GPU's own logits
    o = OR.route(logits, n_dyn, cfgd["mlp_dynamic_expert_num"], n_fix, float(cfgd["mlp_dynamic_top_p"]),
                 int(cfgd["mlp_dynamic_top_k"]), float(cfgd["router_jitter_noise"]),
                 None if am is None else am.reshape(-1))
    assert torch.equal(top_k.long(), o["top_k"])
    if not cfgd["token_drop"]:
        assert torch.equal(top_k.long()[same], g["out_top_k"].long()[same])
        assert torch.equal(mask[same], g["out_mask"][same])
        assert torch.equal(mask, o["expert_mask"])
    else:
        # token drop (umoe_token_drop): the post-drop mask equals the oracle's selection on the GPU's own logits -- bit-exact
        # integers for every token -- and the reference's own mask whenever every logit came out bit-identical
        from oracle.dcmoe import capacity_of, drop_keep_mask
        cap = capacity_of(logits.shape[0], n_dyn, cfgd["capacity_factor"], cfgd["min_capacity"])
        kept = drop_keep_mask(logits, o["expert_mask"], n_dyn, cap, cfgd["drop_policy"])
        assert torch.equal(mask, kept)
        assert int((kept != o["expert_mask"]).sum()) > 0
        assert torch.equal(top_k.long()[same], g["out_top_k"].long()[same])
        if bool(same.all()):
            assert torch.equal(mask, g["out_mask"])
    agree = (mask == g["out_mask"]).all(-1).reshape(hid.shape[:2])
    ok = torch.isfinite(g["out_hidden"].float()).all(-1) & agree
    assert ok.float().mean() > 0.5
    assert torch.allclose(hid.float()[ok], g["out_hidden"].float()[ok], rtol=2 ** -5, atol=2 ** -7)
    okw = ok.reshape(-1)
    assert torch.allclose(weight.float()[okw], g["out_weight"].float()[okw], rtol=2 ** -6, atol=2 ** -8)
    # aux load-balancing loss (fp32 scalar): against the oracle's formula on the GPU's OWN logits and (pre-drop) mask to 1e-4 --
    # what the kernel's arithmetic is responsible for; against the reference's value within what bf16 logit noise moves it
    from oracle.dcmoe import aux_loss as oracle_aux
    aux_ref = oracle_aux(o["expert_mask"], n_dyn, logits, None if aw is None else aw)
    assert torch.allclose(aux.float(), aux_ref.float(), rtol=1e-4, atol=1e-6), (float(aux), float(aux_ref))
    if bool(agree.all()) and bool(torch.isfinite(g["out_aux"])):
        assert torch.allclose(aux.float(), g["out_aux"].float(), rtol=3e-2, atol=1e-3)


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "dcmoebwd_*.npz"))), ids=os.path.basename)
def test_dcmoe_block_backward_vs_reference_autograd(dev, path):
    """Training step of the block: HIP forward + HIP backward (torch.autograd.Function over the C-ABI) against the
    gradients the REFERENCE's own autograd produced for loss = sum(out * G) + aux_coef * aux (oracle/gen_golden.py,
    dcmoebwd family).  Tolerance: relative Frobenius error per gradient tensor (bf16 autograd chains on both sides)."""
    g = load_golden(os.path.basename(path))
    cfgd = g["cfg_json"]
    w = {k[2:]: v for k, v in g.items() if k.startswith("w.")}
    blk = _mk_block(cfgd, w, dev)
    blk.train(bool(int(g["train"])))
    if "in_gumbel" in g:          # the mixer's training branch (core.py:111-137): the reference's own noise draws, injected
        blk._router_noise = (g["in_gumbel"], g["in_rand"])
    if "in_input_noise" in g:     # input jitter (core.py:243-244): on the gate's fp32 copy (fp32 gate) / on the rows themselves (bf16 gate)
        blk._input_noise_inject = g["in_input_noise"]
    for p_ in blk.parameters():
        p_.requires_grad_(True)
    am, aw = g.get("in_attention_mask"), g.get("in_aux_balance_weight")
    x = g["in_x"].to(dev).requires_grad_(True)
    G = g["in_G"].to(dev)
    out = blk(x, None if am is None else am.to(dev), None if aw is None else aw.to(dev))
    mask_ok = bool((out[3].cpu() == g["out_mask"]).all())
    loss = (out[0].float() * G.float()).sum() + float(g["aux_coef"]) * out[5].float()
    loss.backward()
    # ("position" token drop: rows that lose every column are NaN in the reference -- softmax over all -inf, core.py:188,321-323 --
    #  and so are the gradients they feed; the same rows must be NaN here, everything finite is compared)
    fin = torch.isfinite(g["out_hidden"].float()).all(-1)
    hid = out[0].detach().cpu().float()
    assert not mask_ok or torch.equal(torch.isfinite(hid).all(-1), fin)
    assert torch.allclose(hid[fin], g["out_hidden"].float()[fin], rtol=2 ** -5, atol=2 ** -6) or not mask_ok

    def rel(a, b):
        ok = torch.isfinite(b.float())
        return float((a.float()[ok] - b.float()[ok]).norm() / (b.float()[ok].norm() + 1e-12))

    # A near-tie may route a few tokens differently from the CPU run that made the fixture.  The test never skips: rows are independent
    # (the input gradient of every OTHER token is compared as usual), a routed expert that no differing token touches in either mask
    # keeps the strict bound, and the tensors every token feeds (gate, shared experts, touched experts) get the bound widened by what
    # a fraction f of differing tokens can move a sum over tokens (2 sqrt(f)); f itself is bounded so the check cannot dissolve.
    got_mask, ref_mask = out[3].cpu().reshape(-1, out[3].shape[-1]), g["out_mask"].reshape(-1, g["out_mask"].shape[-1])
    bad = (got_mask != ref_mask).any(-1)
    f_bad = float(bad.float().mean())
    assert f_bad <= 0.02, f"{int(bad.sum())} of {bad.numel()} tokens route differently from the fixture: more than near-ties explain"
    touched = ((got_mask[bad] != 0) | (ref_mask[bad] != 0)).any(0) if bool(bad.any()) else torch.zeros(got_mask.shape[-1], dtype=torch.bool)
    gx, rx = x.grad.cpu().reshape(-1, x.shape[-1]), g["grad_x"].reshape(-1, x.shape[-1])
    errs = {"x": rel(gx[~bad], rx[~bad])}
    loose = set()
    for n, p_ in blk.named_parameters():
        ref = g["g." + n]
        if not bool(torch.isfinite(ref.float()).all()):
            assert p_.grad is not None and not bool(torch.isfinite(p_.grad.float()).all()), n       # NaN where the reference is NaN
            continue
        if float(ref.float().norm()) == 0.0:
            assert mask_ok is False or p_.grad is None or float(p_.grad.float().norm()) == 0.0, n
            continue
        assert p_.grad is not None, n
        errs[n] = rel(p_.grad.cpu(), ref)
        if not mask_ok:
            m_ = re.search(r"deepspeed_experts\.(\d+)\.", n)
            if m_ is None or bool(touched[int(m_.group(1))]):
                loose.add(n)
    bound = {n: 0.03 + (2.0 * f_bad ** 0.5 if n in loose else 0.0) for n in errs}
    over = {n: (e, bound[n]) for n, e in errs.items() if e >= bound[n]}
    assert not over, (over, errs, f_bad)


def test_dcmoe_block_backward_multitile_vs_autograd_oracle(dev):
    """Many rows per expert (several 128-row tiles, several 64-deep K steps in the weight-gradient contractions),
    padding mask and aux weights: HIP forward/backward against the differentiable CPU oracle (itself pinned to the
    reference's autograd by the dcmoebwd fixtures)."""
    from oracle import dcmoe_autograd as OA
    cfgd = dict(hidden_size=256, mlp_dynamic_expert_num=8, mlp_dynamic_null_expert_num=1, mlp_dynamic_top_p=0.7,
                mlp_dynamic_top_k=2, mlp_fixed_expert_num=2, ignore_differentiable_router=True, ep_size=1,
                router_jitter_noise=0.01, input_jitter_noise=0.0, min_capacity=8, capacity_factor=6.0, token_drop=False,
                drop_policy="probs", avg_hidden_states_last=False, drop_token_num_print=False, fp32_gate=True,
                dynamic_intermediate_size=352, shared_intermediate_size=176, hidden_act="silu",
                enable_expert_tensor_parallelism=False)
    cfg = types.SimpleNamespace(**cfgd)
    gen = torch.Generator().manual_seed(77)
    D, Id, Is = 256, 352, 176
    w = {"gate.weight": (torch.randn(11, D, generator=gen) * 0.2).to(torch.bfloat16)}
    for e in range(8):
        for p_, shp in (("gate", (Id, D)), ("up", (Id, D)), ("down", (D, Id))):
            w[OA.EXPERT_FMT.format(e=e, p=p_)] = (torch.randn(*shp, generator=gen) * 0.05).to(torch.bfloat16)
    for i in range(2):
        for p_, shp in (("gate", (Is, D)), ("up", (Is, D)), ("down", (D, Is))):
            w[OA.SHARED_FMT.format(i=i, p=p_)] = (torch.randn(*shp, generator=gen) * 0.05).to(torch.bfloat16)
    B, T = 2, 450
    x = torch.randn(B, T, D, generator=gen).to(torch.bfloat16)
    G = torch.randn(B, T, D, generator=gen).to(torch.bfloat16)
    am = torch.ones(B, T, dtype=torch.bool)
    am[0, :37] = False
    aw = torch.rand(B, T, generator=gen)
    wo = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    xo = x.clone().requires_grad_(True)
    ro = OA.forward(cfg, wo, xo, am, aw, training=True)
    ((ro[0].float() * G.float()).sum() + 0.5 * ro[5].float()).backward()
    blk = _mk_block(cfgd, w, dev)
    blk.train(True)
    for p_ in blk.parameters():
        p_.requires_grad_(True)
    xg = x.to(dev).requires_grad_(True)
    rg = blk(xg, am.to(dev), aw.to(dev))
    ((rg[0].float() * G.to(dev).float()).sum() + 0.5 * rg[5].float()).backward()
    same = (rg[3].cpu() == ro[3]).all(-1)
    assert same.float().mean() > 0.97            # fp32 gate logits differ in the last bits: a few near-ties may flip
    rel = lambda a, b: float((a.float() - b.float()).norm() / (b.float().norm() + 1e-12))
    assert rel(rg[0].detach().cpu().reshape(-1, D)[same], ro[0].detach().reshape(-1, D)[same]) < 0.01
    tol = 0.03 if bool(same.all()) else 0.08     # a flipped token moves one row between two experts' gradients
    assert rel(xg.grad.cpu().reshape(-1, D)[same], xo.grad.reshape(-1, D)[same]) < tol
    for n, p_ in blk.named_parameters():
        assert rel(p_.grad.cpu(), wo[n].grad) < tol, (n, rel(p_.grad.cpu(), wo[n].grad))


def test_dcmoe_block_fullsize_vs_oracle(dev):
    """Full utils/config.json sizes, 16 rows (decode shape) and 300 rows, against the CPU oracle."""
    from oracle.dcmoe import DCMoEOracle
    from unimoe_audio_amd.config import UniMoEAudioConfig
    from unimoe_audio_amd.dcmoe import UniMoEAudioSparseMoeBlock
    cfg = UniMoEAudioConfig()
    torch.manual_seed(1234)
    blk = UniMoEAudioSparseMoeBlock(cfg)
    with torch.no_grad():
        for p in blk.parameters():
            p.normal_(0, 0.02)
    blk = blk.to(torch.bfloat16).eval()
    w = {k: v.clone() for k, v in blk.state_dict().items()}
    orc = DCMoEOracle(cfg, w)
    gpu = blk.to(dev)
    for S in (16, 300):
        x = torch.randn(1, S, cfg.hidden_size).to(torch.bfloat16)
        with torch.no_grad():
            out = [o.cpu() for o in gpu(x.to(dev), None, None)]
        ref = orc(x, None, None)
        same = (out[1].float() == ref[1].float()).all(-1)
        assert same.float().mean() > 0.9
        assert torch.equal(out[2][same], ref[2][same]) and torch.equal(out[3][same], ref[3][same])
        assert torch.allclose(out[0].float()[0][same], ref[0].float()[0][same], rtol=2 ** -5, atol=2 ** -9)


@pytest.mark.parametrize("case", ["all_padded", "null_expert_only", "every_expert", "one_expert_takes_all", "single_token", "seventeen_tokens",
                                  "half_padded_ragged"])
def test_dcmoe_block_edge_cases_vs_oracle(dev, case):
    """The block at the edges of its routing domain (small width, every size ragged on purpose), against the CPU oracle (itself pinned
    to the reference's fixtures): every token padded (no routed rows at all, shared experts only), every token on the NULL expert only
    (all eight real experts idle: empty groups in the grouped launches), every token on all nine columns (maximum fan-out, top-p close
    to 1), one expert taking every row while seven stay empty, one token, 17 tokens (one past a 16-row tile), a padded half."""
    from oracle import router as OR
    from oracle.dcmoe import DCMoEOracle
    cfgd = dict(hidden_size=64, mlp_dynamic_expert_num=8, mlp_dynamic_null_expert_num=1, mlp_dynamic_top_p=0.7, mlp_dynamic_top_k=2,
                mlp_fixed_expert_num=2, ignore_differentiable_router=True, ep_size=1, router_jitter_noise=0.01, input_jitter_noise=0.0,
                min_capacity=8, capacity_factor=6.0, token_drop=False, drop_policy="probs", avg_hidden_states_last=False,
                drop_token_num_print=False, fp32_gate=True, dynamic_intermediate_size=96, shared_intermediate_size=64, hidden_act="silu",
                enable_expert_tensor_parallelism=False)
    B, T = 3, 11
    if case == "every_expert":
        cfgd["mlp_dynamic_top_p"] = 0.9999
    if case == "single_token":
        B, T = 1, 1
    if case == "seventeen_tokens":
        B, T = 1, 17
    cfg = types.SimpleNamespace(**cfgd)
    torch.manual_seed({"all_padded": 1, "null_expert_only": 2, "every_expert": 3, "one_expert_takes_all": 4, "single_token": 5,
                       "seventeen_tokens": 6, "half_padded_ragged": 7}[case])
    from unimoe_audio_amd.dcmoe import UniMoEAudioSparseMoeBlock
    blk = UniMoEAudioSparseMoeBlock(cfg)
    with torch.no_grad():
        for n, p_ in blk.named_parameters():
            p_.normal_(0, 0.35 if n == "gate.weight" else 0.08)
        x = torch.randn(B, T, 64)
        if case in ("null_expert_only", "one_expert_takes_all"):
            # a gate row aligned with a direction every input carries: that column wins by a wide margin (softmax mass > top-p alone)
            col = 8 if case == "null_expert_only" else 3
            x[..., 0] = 6.0
            blk.gate.weight.zero_()
            blk.gate.weight[col, 0] = 2.0
        if case == "every_expert":
            blk.gate.weight[:9].mul_(0.02)               # nearly flat dynamic logits: the cumulative mass passes 0.9999 only at the last column
    blk = blk.to(torch.bfloat16).eval()
    x = x.to(torch.bfloat16)
    am = None
    if case == "all_padded":
        am = torch.zeros(B, T, dtype=torch.bool)
    if case == "half_padded_ragged":
        am = torch.ones(B, T, dtype=torch.bool)
        am[0, :7] = False
        am[1, :] = False
        am[2, :1] = False
    w = {k: v.clone() for k, v in blk.state_dict().items()}
    ref = DCMoEOracle(cfg, w)(x, am, None)
    with torch.no_grad():
        out = [o.cpu() for o in blk.to(dev)(x.to(dev), None if am is None else am.to(dev), None)]
    hid, logits, top_k, mask, weight, aux = out
    o = OR.route(logits, 9, 8, 2, float(cfg.mlp_dynamic_top_p), 2, 0.01, None if am is None else am.reshape(-1))
    assert torch.equal(top_k.long(), o["top_k"]) and torch.equal(mask, o["expert_mask"])       # ints exact on the GPU's own logits
    same = (logits.float() == ref[1].float()).all(-1)
    assert torch.equal(top_k.long()[same], ref[2].long()[same]) and torch.equal(mask[same], ref[3][same])
    routed = mask[:, :8].sum(0)
    if case == "all_padded":
        assert int(mask[:, :9].sum()) == 0 and bool((mask[:, 9:] == 1).all())
    if case == "null_expert_only":
        assert int(routed.sum()) == 0 and bool((mask[:, 8] == 1).all()) and bool((top_k == 1).all())
    if case == "every_expert":
        assert bool((top_k == 9).all()) and bool((mask[:, :9] == 1).all())
    if case == "one_expert_takes_all":
        assert int(routed[3]) == B * T and int(routed.sum()) == B * T
    agree = (mask == ref[3]).all(-1)
    assert agree.float().mean() > 0.8
    assert torch.isfinite(hid.float()).all()
    ok = agree.reshape(B, T)
    assert torch.allclose(hid.float()[ok], ref[0].float()[ok], rtol=2 ** -5, atol=2 ** -7)
    assert torch.allclose(weight.float()[agree], ref[4].float()[agree], rtol=2 ** -6, atol=2 ** -8)


@pytest.mark.parametrize("case", ["null_expert_only", "one_expert_takes_all"])
def test_dcmoe_block_backward_with_idle_experts(dev, case):
    """Training step of the block when real experts receive NO row (every token on the null expert / on expert 3 only): the grouped
    forward and weight-gradient launches see empty groups.  Against the differentiable CPU oracle: idle experts' weight gradients are
    exactly zero, everything else within the block-level tolerance."""
    from oracle import dcmoe_autograd as OA
    from unimoe_audio_amd.dcmoe import UniMoEAudioSparseMoeBlock
    cfg = types.SimpleNamespace(hidden_size=64, mlp_dynamic_expert_num=8, mlp_dynamic_null_expert_num=1, mlp_dynamic_top_p=0.7, mlp_dynamic_top_k=2,
                                mlp_fixed_expert_num=2, ignore_differentiable_router=True, ep_size=1, router_jitter_noise=0.01,
                                input_jitter_noise=0.0, min_capacity=8, capacity_factor=6.0, token_drop=False, drop_policy="probs",
                                avg_hidden_states_last=False, drop_token_num_print=False, fp32_gate=True, dynamic_intermediate_size=96,
                                shared_intermediate_size=64, hidden_act="silu", enable_expert_tensor_parallelism=False)
    torch.manual_seed(21 if case == "null_expert_only" else 22)
    B, T = 3, 24
    blk = UniMoEAudioSparseMoeBlock(cfg)
    col = 8 if case == "null_expert_only" else 3
    with torch.no_grad():
        for n, p_ in blk.named_parameters():
            p_.normal_(0, 0.08)
        x = torch.randn(B, T, 64)
        x[..., 0] = 6.0
        blk.gate.weight.zero_()
        blk.gate.weight[col, 0] = 2.0
    blk = blk.to(torch.bfloat16).train()
    x = x.to(torch.bfloat16)
    G = torch.randn(B, T, 64).to(torch.bfloat16)
    w = {k: v.clone() for k, v in blk.state_dict().items()}
    wo = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    xo = x.clone().requires_grad_(True)
    ro = OA.forward(cfg, wo, xo, None, None, training=True)
    ((ro[0].float() * G.float()).sum() + 0.3 * ro[5].float()).backward()
    gm = blk.to(dev)
    for p_ in gm.parameters():
        p_.requires_grad_(True)
    xg = x.to(dev).requires_grad_(True)
    out = gm(xg, None, None)
    assert torch.equal(out[3].cpu(), ro[3])
    ((out[0].float() * G.to(dev).float()).sum() + 0.3 * out[5].float()).backward()
    assert torch.allclose(out[0].detach().cpu().float(), ro[0].detach().float(), rtol=2 ** -5, atol=2 ** -6)
    rel = lambda a, b: float((a.float() - b.float()).norm() / (b.float().norm() + 1e-12))
    assert rel(xg.grad.cpu(), xo.grad) < 0.03
    for n, p_ in gm.named_parameters():
        ref = wo[n].grad
        idle = "deepspeed_experts" in n and not (case == "one_expert_takes_all" and ".3." in n)
        if idle or ref is None or float(ref.float().norm()) == 0.0:
            assert p_.grad is None or float(p_.grad.float().abs().max()) == 0.0, n         # no row, no gradient: exactly zero
        else:
            assert p_.grad is not None and rel(p_.grad.cpu(), ref) < 0.03, (n, rel(p_.grad.cpu(), ref))


# ----------------------------------------------------------------------------- rope / attention
def _attn_setup(rows, T, H, KVH, hd, Lmax, pads, seed):
    from oracle import decode as OD
    torch.manual_seed(seed)
    cfg = types.SimpleNamespace(hidden_size=H * hd, num_attention_heads=H, num_key_value_heads=KVH, rope_theta=1e6,
                                mrope_section=[16, 24, 24], rms_norm_eps=1e-6)
    D = H * hd
    w = {"a.q_proj.weight": (torch.randn(H * hd, D) * 0.03).to(torch.bfloat16), "a.q_proj.bias": (torch.randn(H * hd) * 0.1).to(torch.bfloat16),
         "a.k_proj.weight": (torch.randn(KVH * hd, D) * 0.03).to(torch.bfloat16), "a.k_proj.bias": (torch.randn(KVH * hd) * 0.1).to(torch.bfloat16),
         "a.v_proj.weight": (torch.randn(KVH * hd, D) * 0.03).to(torch.bfloat16), "a.v_proj.bias": (torch.randn(KVH * hd) * 0.1).to(torch.bfloat16),
         "a.o_proj.weight": (torch.randn(D, H * hd) * 0.03).to(torch.bfloat16)}
    x = torch.randn(rows, T + 2, D).to(torch.bfloat16)
    valid = torch.ones(rows, T + 2, dtype=torch.bool)
    for r, p in enumerate(pads):
        valid[r, :p] = False
    pos = (valid.long().cumsum(-1) - 1).masked_fill(~valid, 1)
    pos3 = torch.stack([pos, pos + 3, pos * 2], 0)
    return cfg, w, x, valid, pos3


def test_rope_attention_prefill_and_decode(dev):
    from oracle import decode as OD
    from unimoe_audio_amd import ops
    rows, T, H, KVH, hd, Lmax = 3, 37, 16, 2, 128, 64
    cfg, w, x, valid, pos3 = _attn_setup(rows, T, H, KVH, hd, Lmax, [5, 0, 1], 11)
    cos3, sin3 = OD.rope_cos_sin(pos3, hd, 1e6, torch.bfloat16)
    cos, sin = OD.mrope_select(cos3, cfg.mrope_section), OD.mrope_select(sin3, cfg.mrope_section)
    cos_tab, sin_tab = ops.rope_tables(256, hd, 1e6, dev)
    wqkv = torch.cat([w["a.q_proj.weight"], w["a.k_proj.weight"], w["a.v_proj.weight"]], 0)
    bqkv = torch.cat([w["a.q_proj.bias"], w["a.k_proj.bias"], w["a.v_proj.bias"]], 0).float()
    wqkv_p, wo_p = ops.pack_weight(wqkv.to(dev)), ops.pack_weight(w["a.o_proj.weight"].to(dev))
    kc = torch.zeros(rows, KVH, Lmax, hd, dtype=torch.bfloat16, device=dev)
    vc = torch.zeros_like(kc)
    kv_start = torch.tensor([5, 0, 1], dtype=torch.int32, device=dev)
    cache = None
    for (a, b, splits) in ((0, T, 1), (T, T + 1, 4), (T + 1, T + 2, 8)):
        nq = b - a
        xs = x[:, a:b]
        ref, cache = OD.attention(cfg, w, "a.", xs, cos[:, a:b], sin[:, a:b], cache, valid[:, :b])
        xd = xs.reshape(rows * nq, -1).contiguous().to(dev)
        qkv = ops.linear(xd, wqkv_p, wqkv.shape[0], bias=bqkv.to(dev))
        p3 = pos3[:, :, a:b].reshape(3, rows * nq).to(torch.int32).contiguous().to(dev)
        kvp = torch.arange(a, b, dtype=torch.int32).repeat(rows).to(dev)
        q0 = torch.full((rows,), a, dtype=torch.int32, device=dev)
        if nq == 1:   # decode: the fused kernel (mRoPE + KV append inside attention) on copies of the caches
            kc2, vc2 = kc.clone(), vc.clone()
            ao_f = ops.attention(None, kc2, vc2, kv_start, q0, 1, H, splits=splits, qkv_raw=qkv, cos_tab=cos_tab, sin_tab=sin_tab,
                                 pos3=p3, sections=cfg.mrope_section)
        q = ops.qkv_mrope_kvappend(qkv, cos_tab, sin_tab, p3, kvp, nq, H, KVH, hd, cfg.mrope_section, kc, vc)
        ao = ops.attention(q, kc, vc, kv_start, q0, nq, H, splits=splits)
        if nq == 1:
            assert torch.equal(kc2, kc) and torch.equal(vc2, vc)          # same rotated K / V landed in the cache
            assert torch.allclose(ao_f.float(), ao.float(), rtol=2 ** -7, atol=2 ** -9)
        out = ops.linear(ao, wo_p, H * hd).reshape(rows, nq, -1).cpu()
        qv = valid[:, a:b]
        # q/k/v proj -> rope -> attention -> o_proj chains ~4 bf16 roundings through a 2048-term sum.  The torch-CPU
        # oracle itself sits 0.0061 (relative Frobenius) away from the same algorithm with ideally rounded (fp64
        # accumulate) linears -- measured in the build container -- so the tolerance is 2.5 bf16 eps in that norm
        # and 3% of the output range for the worst element.
        d = (out.float()[qv] - ref.float()[qv])
        assert float(d.norm() / ref.float()[qv].norm()) < 2.5 * 2 ** -8, (a, b, float(d.norm() / ref.float()[qv].norm()))
        assert float(d.abs().max()) < 0.03 * float(ref.float()[qv].abs().max()), (a, b)
        # cache contents = the oracle's rotated keys / values (bf16, every rope op rounded like torch)
        kref, vref = cache
        got_k = kc[:, :, :b].cpu()
        sel = valid[:, :b].unsqueeze(1).expand(-1, KVH, -1)
        dk = got_k.float()[sel] - kref.float()[sel]      # rope sums can cancel: bound by ulps of the operands
        assert float(dk.norm() / kref.float()[sel].norm()) < 2 ** -7 and float(dk.abs().max()) < 0.07


def test_gemm256_forced_in_child_process():
    """The 256 x 256 ping-pong GEMM is chosen by size; UMOE_TGEMM_PP=1 forces it for EVERY tiled GEMM.  Re-run the GEMM,
    ragged / SwiGLU, block-backward and backward-kernel tests with it forced (small and odd shapes: partial tiles, K tails,
    gather lists, contraction windows, pre-activation outputs, fp32 outputs), in a child process because the library reads
    the switch once."""
    import subprocess, sys
    env = dict(os.environ, UMOE_TGEMM_PP="1")
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(here, "test_gpu_ops.py"), os.path.join(here, "test_gpu_bwd.py"), "-x", "-q",
                        "-m", "gpu", "-k", "tiled or ragged or backward or multitile or bwd", "-p", "no:cacheprovider"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "no tests ran" not in r.stdout, r.stdout[-500:]


# ----------------------------------------------------------------------------- codec side
def test_codec_embed_sum(dev):
    from unimoe_audio_amd import ops
    torch.manual_seed(3)
    C, V, D, rows = 12, 1027, 2048, 16
    emb = (torch.randn(C, V, D) * 0.02).to(torch.bfloat16)
    tok = torch.randint(0, V, (rows, C))
    ref = None
    for c in range(C):
        e = emb[c][tok[:, c]]
        ref = e if ref is None else ref + e
    got = ops.codec_embed_sum(tok.to(dev), emb.to(dev)).cpu()
    assert torch.equal(got, ref)                  # same bf16 adds in the same order: exact


def test_cfg_sampler_vs_reference_goldens(dev):
    from oracle import decode as OD
    from unimoe_audio_amd import ops
    g = load_golden("sampler.npz")
    lg = g["logits"]                               # [24, 1027] treated as B=2, C=12 guided logits (cfg_scale=0 path)
    B, C, V = 2, 12, 1027
    two = torch.stack([torch.zeros_like(lg), lg], 1).reshape(B, C, 2, V).permute(0, 2, 1, 3).reshape(2 * B, C * V).contiguous()
    # arg-max path, no masks beyond those already in the logits: compare with the reference's T=0 result
    cfgo = types.SimpleNamespace(codec_eos_value=1024)
    guided = OD.cfg_and_mask(cfgo, two.view(2 * B, C, V).clone(), 0.0, True, 1.0).reshape(B * C, V)
    pred = ops.cfg_sample(two.to(dev), B, C, V, cfg_scale=0.0, temperature=0.0, top_p=1.0, top_k=45, eos=1024, eos_mul=1.0,
                          enable_eos=True, do_sample=False).cpu().reshape(-1)
    assert torch.equal(pred, torch.argmax(guided, -1))
    for n in "abcd":
        T, tp, tk = g[f"params_{n}"].tolist()
        ref = OD.sample_next_token(guided.clone(), T, tp, None if tk < 0 else int(tk), 1024, return_probs=True)
        pred, probs = ops.cfg_sample(two.to(dev), B, C, V, cfg_scale=0.0, temperature=T, top_p=tp, top_k=None if tk < 0 else int(tk),
                                     eos=1024, eos_mul=1.0, enable_eos=True, do_sample=True, seed=7, want_probs=True)
        probs = probs.cpu()
        assert torch.equal(probs > 0, ref > 0), n
        assert torch.allclose(probs, ref, rtol=1e-4, atol=1e-7), n
        assert bool((probs.gather(1, pred.cpu().reshape(-1, 1)) > 0).all())      # draws land on kept entries
    # CFG mixing + EOS masks (model.py:991-1017) with a real uncond row
    torch.manual_seed(9)
    lg2 = torch.randn(2 * B, C * V) * 2
    ref = OD.cfg_and_mask(cfgo, lg2.view(2 * B, C, V).clone(), 3.0, True, 0.8).reshape(B * C, V)
    pred = ops.cfg_sample(lg2.to(dev), B, C, V, cfg_scale=3.0, temperature=0.0, top_p=1.0, top_k=45, eos=1024, eos_mul=0.8,
                          enable_eos=True, do_sample=False).cpu().reshape(-1)
    assert torch.equal(pred, torch.argmax(ref, -1))
    ref = OD.cfg_and_mask(cfgo, lg2.view(2 * B, C, V).clone(), 3.0, False, 0.8).reshape(B * C, V)
    pred = ops.cfg_sample(lg2.to(dev), B, C, V, cfg_scale=3.0, temperature=0.0, top_p=1.0, top_k=45, eos=1024, eos_mul=0.8,
                          enable_eos=False, do_sample=False).cpu().reshape(-1)
    assert torch.equal(pred, torch.argmax(ref, -1))


def test_rvq_roundtrip_code_ids_exact(dev):
    """RVQ with synthetic codebooks: from_codes -> nearest returns the same code ids when the codebooks are
    well separated (encode(decode(codes)) == codes), and from_codes matches a plain fp32 restatement."""
    from unimoe_audio_amd import ops
    torch.manual_seed(21)
    NQ, CB, cd, Dl, T = 12, 1024, 8, 64, 50
    cb = torch.nn.functional.normalize(torch.randn(NQ, CB, cd), dim=-1)
    # orthonormal-ish in/out projections per level so residual levels do not interfere: block structure
    out_w = torch.zeros(NQ, Dl, cd)
    in_w = torch.zeros(NQ, cd, Dl)
    for q in range(NQ):
        blk = torch.zeros(Dl, cd)
        blk[(q * 5) % (Dl - cd):(q * 5) % (Dl - cd) + cd] = torch.eye(cd) * (0.5 ** q)
        out_w[q] = blk
        in_w[q] = blk.t() / (0.25 ** q)
    codes = torch.randint(0, CB, (NQ, T))
    z = ops.rvq_from_codes(codes.to(dev), cb.to(dev), out_w.to(dev), None).cpu()
    ref = torch.zeros(Dl, T)
    for q in range(NQ):
        ref += out_w[q] @ cb[q][codes[q]].t()
    assert torch.allclose(z, ref, rtol=1e-5, atol=1e-6)
    q0 = ops.rvq_nearest(z.to(dev), cb[:1].contiguous().to(dev), in_w[:1].contiguous().to(dev), None,
                         out_w[:1].contiguous().to(dev), None).cpu()
    e0 = (in_w[0] @ z).t()
    sim = torch.nn.functional.normalize(e0, dim=-1) @ torch.nn.functional.normalize(cb[0], dim=-1).t()
    assert torch.equal(q0[0].long(), sim.argmax(-1))


def test_rvq_nearest_all_levels_vs_fp64_restatement(dev):
    """The whole residual loop of ResidualVectorQuantize.forward (third-party descript-audio-codec 1.0.0, called at
    utils/UniMoE_Audio_utils.py:113; PARITY UNPINNED: the package is absent offline, the algorithm is restated from its published
    form): per level in_proj -> L2-normalised nearest neighbour over 1024 entries -> subtract out_proj(code) -> next level.
    Generic dense projections with biases (not the block structure of the round-trip test), 12 levels, fp64 restatement: every
    code id of every level bit-exact, wherever the fp64 top-2 similarity gap is not itself below fp32 resolution."""
    from unimoe_audio_amd import ops
    g = torch.Generator().manual_seed(5)
    NQ, CB, cd, Dl, T = 12, 1024, 8, 96, 300
    cb = torch.randn(NQ, CB, cd, generator=g)
    in_w = torch.randn(NQ, cd, Dl, generator=g) / Dl ** 0.5
    in_b = 0.1 * torch.randn(NQ, cd, generator=g)
    out_w = torch.randn(NQ, Dl, cd, generator=g) / cd ** 0.5 * 0.5
    out_b = 0.05 * torch.randn(NQ, Dl, generator=g)
    z = torch.randn(Dl, T, generator=g)
    codes = ops.rvq_nearest(z.to(dev), cb.to(dev), in_w.to(dev), in_b.to(dev), out_w.to(dev), out_b.to(dev)).cpu().long()
    res = z.double().t().clone()                                           # [T, Dl]
    cbn = torch.nn.functional.normalize(cb.double(), dim=-1)
    exact = total = 0
    for q in range(NQ):
        e = res @ in_w[q].double().t() + in_b[q].double()
        sim = torch.nn.functional.normalize(e, dim=-1) @ cbn[q].t()       # [T, CB]
        top2 = sim.topk(2, dim=-1)
        ref = top2.indices[:, 0]
        clear = (top2.values[:, 0] - top2.values[:, 1]) > 1e-5             # fp32 cannot be asked to split closer pairs
        assert torch.equal(codes[q][clear], ref[clear]), q
        exact += int((codes[q] == ref).sum())
        total += T
        # continue the fp64 loop with the KERNEL's codes: a (legitimate) near-tie flip must not poison the later levels' check
        res = res - (cbn[q][codes[q]] * 0 + cb[q].double()[codes[q]]) @ out_w[q].double().t() - out_b[q].double()
    assert exact / total > 0.995, (exact, total)
    # from_codes (utils.py:123) inverts the sum the loop subtracted: z - residual == sum_q out_proj_q(cb_q[code])
    zq = ops.rvq_from_codes(codes.to(dev), cb.to(dev), out_w.to(dev), out_b.to(dev)).cpu()
    assert torch.allclose(zq.double().t(), z.double().t() - res, rtol=1e-4, atol=1e-4)


# ----------------------------------------------------------------------------- expert parallel (HIP path, 2 virtual ranks)
def test_dcmoe_expert_parallel_two_virtual_ranks(dev):
    """ep_size = 2 on ONE GPU: two module instances (4 local experts each) exchange rows through a thread-rendezvous
    all-to-all; every rank's output must be bit-identical to the ep_size = 1 block on the same tokens."""
    import threading
    from unimoe_audio_amd import ep as EP
    from unimoe_audio_amd.config import UniMoEAudioConfig
    from unimoe_audio_amd.dcmoe import UniMoEAudioSparseMoeBlock
    cfg1 = UniMoEAudioConfig(hidden_size=256, dynamic_intermediate_size=128, shared_intermediate_size=64)
    torch.manual_seed(77)
    full = UniMoEAudioSparseMoeBlock(cfg1)
    with torch.no_grad():
        for n, p in full.named_parameters():
            p.normal_(0, 0.3 if n == "gate.weight" else 0.06)
    full = full.to(torch.bfloat16).eval().to(dev)
    world, S = 2, 11
    cfg2 = UniMoEAudioConfig(hidden_size=256, dynamic_intermediate_size=128, shared_intermediate_size=64, ep_size=world)
    ranks = []
    fsd = full.state_dict()
    for r in range(world):
        blk = UniMoEAudioSparseMoeBlock(cfg2).to(torch.bfloat16).eval()
        sd = {}
        for k, v in blk.state_dict().items():
            if "deepspeed_experts." in k:
                e_loc = int(k.split("deepspeed_experts.")[1].split(".")[0])
                sd[k] = fsd[k.replace(f"deepspeed_experts.{e_loc}.", f"deepspeed_experts.{r * 4 + e_loc}.")]
            else:
                sd[k] = fsd[k]
        blk.load_state_dict(sd)
        blk = blk.to(dev)
        blk.dynamic_real_moe.set_deepspeed_parallelism(ep_group=("virtual", r))
        ranks.append(blk)
    xs = [torch.randn(1, S, 256).to(torch.bfloat16).to(dev) for _ in range(world)]
    bar = threading.Barrier(world)
    box = {}

    # the block's ragged exchange (ep.py) goes through two module-level functions: the header all-to-all and the row all-to-all with split
    # sizes; here both are thread rendezvous between the two "ranks" of this one process
    def fake_hdr(send, group, ep_size, dev_):
        r = group[1]
        box[("h", r)] = send
        bar.wait()
        out = torch.stack([box[("h", src)][r] for src in range(world)])
        bar.wait()
        return out

    def fake_rows(buf, in_splits, out_splits, n_out, group):
        r = group[1]
        box[("r", r)] = (buf, in_splits)
        torch.cuda.synchronize()
        bar.wait()
        parts = []
        for src in range(world):
            b_src, sp = box[("r", src)]
            o = sum(sp[:r])
            parts.append(b_src[o: o + sp[r]])
            assert sp[r] == out_splits[src]
        out = torch.cat(parts) if parts else buf.new_zeros((0, buf.shape[1]))
        torch.cuda.synchronize()
        bar.wait()
        return out
    orig = (EP._hdr_exchange, EP._rows_exchange)
    EP._hdr_exchange, EP._rows_exchange = fake_hdr, fake_rows
    outs, errs = [None] * world, []

    def run(r):
        try:
            with torch.no_grad():
                outs[r] = ranks[r](xs[r], None, None)
        except Exception as e:  # pragma: no cover
            errs.append(e)
            bar.abort()
    try:
        th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
        [t.start() for t in th]
        [t.join() for t in th]
    finally:
        EP._hdr_exchange, EP._rows_exchange = orig
    assert not errs, errs
    for r in range(world):
        with torch.no_grad():
            ref = full(xs[r], None, None)
        assert torch.equal(outs[r][3], ref[3]) and torch.equal(outs[r][2], ref[2])
        assert torch.equal(outs[r][0], ref[0]), float((outs[r][0].float() - ref[0].float()).abs().max())


@pytest.mark.parametrize("S,K,N,ks", [(16, 2752, 2048, 2), (9, 1376, 2048, 2), (16, 2048, 512, 4), (5, 96, 64, 2)])
def test_gemm_ksplit_partial_slabs(dev, S, K, N, ks):
    """K split over workgroups: the fp32 partial slabs must add up to the unsplit product."""
    from unimoe_audio_amd import ops
    torch.manual_seed(K + N + ks)
    x = (torch.randn(S, K) * 0.5).to(torch.bfloat16)
    w = (torch.randn(N, K) * 0.05).to(torch.bfloat16)
    tab = ops.GroupTable([dict(w=ops.pack_weight(w.to(dev)), static_count=S, n_blocks=(N + 15) // 16, k=K)], dev)
    parts = torch.zeros(ks, S, N, dtype=torch.float32, device=dev)
    ops.grouped_gemm(tab, x.to(dev), parts, max_rows=S, epilogue=ops.EPI_F32_RAW, n_valid=N, ksplit=ks, part_stride=parts.stride(0), nt=8 if N >= 512 else 1)
    ref = x.float() @ w.float().t()
    got = parts.sum(0).cpu()
    assert torch.allclose(got, ref, rtol=1e-4, atol=1e-4)
    assert float(parts[0].abs().sum()) > 0 and float(parts[ks - 1].abs().sum()) > 0


def test_codec_cross_entropy_fwd_bwd(dev):
    """12 per-channel CrossEntropyLoss terms (reference model.py:830-847) incl. ignored labels and a channel without labels;
    the gradient w.r.t. the logits against torch autograd (fp32 tolerance)."""
    from unimoe_audio_amd import ops
    torch.manual_seed(4)
    N, C, V = 37, 12, 1027
    logits = (torch.randn(N, C, V) * 2).requires_grad_(True)
    labels = torch.randint(0, 1024, (N, C))
    labels[torch.rand(N, C) < 0.3] = -100
    labels[:, 7] = -100                                   # a channel with no valid label is skipped (c != 0)
    ref = None
    for c in range(C):
        if c != 0 and int((labels[:, c] != -100).sum()) == 0:
            continue
        l = torch.nn.functional.cross_entropy(logits[:, c], labels[:, c], ignore_index=-100)
        ref = l if ref is None else ref + l
    ref.backward()
    total, ch_loss, ch_cnt, dl = ops.codec_ce(logits.detach().to(dev), labels.to(dev), want_grad=True)
    assert torch.allclose(total.cpu(), ref.detach(), rtol=1e-5, atol=1e-5)
    assert int(ch_cnt[7]) == 0 and torch.equal(ch_cnt.cpu().long(), (labels != -100).sum(0))
    assert torch.allclose(dl.cpu(), logits.grad, rtol=1e-4, atol=1e-7)


def test_ep_all_to_all_rccl_single_rank(dev):
    """umoe_ep_all_to_all through librccl with a one-rank communicator built by umoe_ep_unique_id / umoe_ep_comm_create:
    the exchange with oneself returns the slab unchanged (plumbing, stream ordering, error path).  The multi-rank semantics
    of the exchange are covered by tests/test_ep_gloo.py (world size 2)."""
    from unimoe_audio_amd import ep as EP
    comm = EP.UmoeEpComm(None, dev)
    assert comm.size == 1 and comm.rank == 0
    x = torch.randn(3, 257, 64, device=dev).to(torch.bfloat16)
    y = torch.empty_like(x)
    comm.all_to_all(y, x)
    torch.cuda.synchronize()
    assert torch.equal(x, y)
    comm.close()




@pytest.mark.parametrize("weighted,bf16", [(False, True), (True, True), (False, False)])
def test_aux_loss_two_launch_form_vs_oracle(dev, weighted, bf16):
    """umoe_aux_loss_fwd_ws (training sizes: 64 workgroups + a finisher) against the oracle's formula (core.py:361-389) at 6 240 tokens and
    against the one-workgroup kernel: the same sums, re-associated."""
    import ctypes as C
    from oracle.dcmoe import aux_loss as oracle_aux
    from unimoe_audio_amd import ops, _lib as L
    g = torch.Generator().manual_seed(17)
    S, E, n_dyn = 6240, 11, 9
    logits = (torch.randn(S, E, generator=g) * 1.5)
    logits = logits.to(torch.bfloat16) if bf16 else logits
    mask = (torch.rand(S, E, generator=g) < 0.45).to(torch.int32)
    mask[:, 0] |= (mask[:, :n_dyn].sum(-1) == 0).to(torch.int32)
    tw = torch.rand(S, generator=g) if weighted else None
    got = ops.aux_loss(logits.to(dev), mask.to(dev), n_dyn, None if tw is None else tw.to(dev))
    ref = oracle_aux(mask, n_dyn, logits, None if tw is None else tw.reshape(1, S))
    assert torch.allclose(got.cpu().float(), ref.float(), rtol=1e-4, atol=1e-6), (float(got), float(ref))
    one = torch.empty(1, dtype=torch.float32, device=dev)
    lg, mk = logits.to(dev).contiguous(), mask.to(dev).contiguous()
    twd = None if tw is None else tw.to(dev).float().contiguous()
    L.check(L.lib().umoe_aux_loss_fwd(C.c_void_p(lg.data_ptr()), int(bf16), C.c_void_p(mk.data_ptr()), C.c_void_p(0 if twd is None else twd.data_ptr()),
                                      S, E, n_dyn, C.c_void_p(one.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "umoe_aux_loss_fwd")
    assert torch.allclose(got.cpu().float(), one.cpu()[0].float(), rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("I_dyn,I_sh", [(128, 64), (136, 72)])
def test_backward_is_deterministic_and_sees_weight_updates(dev, I_dyn, I_sh):
    """Repeated backward passes over unchanged weights give the same gradients bit for bit, and an in-place weight update is seen by the
    next pass: nothing weight-dependent is kept across calls (round 2 cached transposed weight copies; the input gradients now read the
    weights as stored -- intermediate sizes that are multiples of 32 -- or transpose them per call)."""
    from unimoe_audio_amd.config import UniMoEAudioConfig
    from unimoe_audio_amd.dcmoe import UniMoEAudioSparseMoeBlock
    torch.manual_seed(4)
    cfg = UniMoEAudioConfig(hidden_size=256, dynamic_intermediate_size=I_dyn, shared_intermediate_size=I_sh, input_jitter_noise=0.0)
    blk = UniMoEAudioSparseMoeBlock(cfg)
    with torch.no_grad():
        for p in blk.parameters():
            p.normal_(0, 0.05)
    blk = blk.to(dev, torch.bfloat16).train()
    for p in blk.parameters():
        p.requires_grad_(True)
    x0 = torch.randn(1, 160, 256).to(torch.bfloat16).to(dev)
    G = torch.randn(1, 160, 256).to(torch.bfloat16).to(dev)

    def run():
        for p in blk.parameters():
            p.grad = None
        x = x0.clone().requires_grad_(True)
        out = blk(x, None, None)
        (out[0].float() * G.float()).sum().backward()
        return [x.grad.clone()] + [p.grad.clone() for p in blk.parameters()]
    a, b, c = run(), run(), run()
    for u, v, w in zip(a, b, c):
        assert torch.equal(u, v) and torch.equal(u, w)
    with torch.no_grad():
        next(iter(blk._experts()[0].parameters())).mul_(1.5)
    d = run()
    assert not torch.equal(d[0], a[0])           # the new weights were used
    e = run()
    assert all(torch.equal(p, q) for p, q in zip(d, e))


def test_mul_noise_is_the_three_torch_ops(dev):
    """umoe_mul_noise == (x.float() * noise).to(bfloat16), bit for bit (core.py:240-244 input jitter on the gate's copy)."""
    from unimoe_audio_amd import ops
    g = torch.Generator().manual_seed(9)
    x = torch.randn(333, 2048, generator=g).to(torch.bfloat16).to(dev)
    nz = torch.empty(333, 2048).uniform_(0.99, 1.01, generator=g).to(dev)
    assert torch.equal(ops.mul_noise(x, nz), (x.float() * nz).to(torch.bfloat16))


@pytest.mark.parametrize("rows,C,V,D", [(700, 12, 1027, 2048), (37, 3, 19, 64), (20000, 2, 11, 256), (600, 1, 5000, 256), (300, 2, 1500, 64)])
def test_codec_embed_sum_bwd_vs_index_add(dev, rows, C, V, D):
    """umoe_codec_embed_sum_bwd (gradient of the stacked codec embedding tables, model.py:655-661 under autograd) against an fp64
    index_add of the same rows: one bf16 rounding of a sum accumulated in fp32; ids nobody chose get exact zeros; the autograd
    wrapper (train.CodecEmbedFn) returns the same through .backward()."""
    from unimoe_audio_amd import ops, train as TR
    g = torch.Generator().manual_seed(rows + V)
    tok = torch.randint(0, V, (rows, C), generator=g)
    dy = torch.randn(rows, D, generator=g).to(torch.bfloat16)
    got = ops.codec_embed_sum_bwd(tok.to(dev), dy.to(dev), V).cpu()
    ref = torch.zeros(C, V, D, dtype=torch.float64)
    for c in range(C):
        ref[c].index_add_(0, tok[:, c], dy.double())
    assert torch.allclose(got.double(), ref, rtol=2 ** -7, atol=1e-6)
    for c in range(C):
        unused = torch.ones(V, dtype=torch.bool)
        unused[tok[:, c]] = False
        assert float(got[c][unused].float().abs().sum()) == 0.0
    tabs = [torch.randn(V, D, generator=g).to(torch.bfloat16).to(dev).requires_grad_(True) for _ in range(C)]
    out = TR.CodecEmbedFn.apply(tok.to(dev), *tabs)
    want = sum(t.detach().cpu()[tok[:, c]] for c, t in enumerate(tabs))          # bf16 adds in channel order
    assert torch.equal(out.cpu(), want)
    out.backward(dy.to(dev))
    for c in range(C):
        assert torch.equal(tabs[c].grad.cpu(), got[c])
    # the single-table form (text embedding, model.py:655) through the same kernel
    tab = torch.randn(V, D, generator=g).to(torch.bfloat16).to(dev).requires_grad_(True)
    ids = tok[:, 0].reshape(1, rows).to(dev)
    e = TR.EmbedFn.apply(ids, tab)
    assert torch.equal(e.cpu(), tab.detach().cpu()[tok[:, 0]].reshape(1, rows, D))
    e.backward(dy.to(dev).reshape(1, rows, D))
    assert torch.equal(tab.grad.cpu(), got[0])


@pytest.mark.parametrize("T,H,KVH,pads", [(333, 16, 2, (70, 0)), (64, 4, 4, (0, 5)), (17, 2, 1, (3, 0)), (1560, 16, 2, (0, 40))])
def test_attention_prefill_mfma_vs_oracle(dev, T, H, KVH, pads):
    """umoe_attn_prefill_fwd (flash-attention forward on the matrix cores, transposing LDS reads for V^T) against the fp32
    softmax restatement of the reference's attention (oracle/decode.py arithmetic): causal, GQA, left padding, query
    counts that are not multiples of the 16-query / 64-key tiles."""
    from unimoe_audio_amd import ops
    g = torch.Generator().manual_seed(T + H)
    B, hd = len(pads), 128
    q = (torch.randn(B * T, H * hd, generator=g) * 1.2).to(torch.bfloat16)
    k = (torch.randn(B, KVH, T, hd, generator=g) * 1.2).to(torch.bfloat16)
    v = torch.randn(B, KVH, T, hd, generator=g).to(torch.bfloat16)
    first = torch.tensor(pads, dtype=torch.int32)
    out = ops.attention(q.to(dev), k.to(dev), v.to(dev), first.to(dev), torch.zeros(B, dtype=torch.int32, device=dev), T, H, splits=1).cpu()
    gq = H // KVH
    qf = q.float().view(B, T, H, hd).transpose(1, 2)
    sc = torch.matmul(qf, k.float().repeat_interleave(gq, 1).transpose(2, 3)) * hd ** -0.5
    pos = torch.arange(T)
    allowed = (pos.view(1, 1, 1, T) <= pos.view(1, 1, T, 1)) & (pos.view(1, 1, 1, T) >= first.view(B, 1, 1, 1))
    p = torch.nan_to_num(torch.softmax(sc.masked_fill(~allowed, float("-inf")), -1), nan=0.0)
    ref = torch.matmul(p.to(torch.bfloat16).float(), v.float().repeat_interleave(gq, 1)).transpose(1, 2).reshape(B * T, H * hd)
    valid = (pos.view(1, T) >= first.view(B, 1)).reshape(-1)
    err = (out.float()[valid] - ref[valid]).norm() / ref[valid].norm()
    assert float(err) < 2.5 * 2 ** -8, float(err)
    assert float(out.float()[~valid].abs().sum()) == 0.0 or not bool((~valid).any())     # fully masked queries -> 0
