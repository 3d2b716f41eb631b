"""GPU suite of umoe_gemm_wide / umoe_pack_rows (csrc/umoe_gemm_wide.hip): 17..64 rows as 2, 3 or 4 sixteen-row tiles, every
weight streamed once.

Shapes: rows 18 / 32 / 34 / 48 / 64 (tiles 2, 2, 3, 3, 4; a partial tile of 2 rows at 18 and 34), K 2048 / 2752 / 1376, one group and three
groups with unequal n_blocks and K.  n_blocks is one more than a multiple of the launcher's blocks per workgroup (1 or 2), so the last
workgroup of a group is partial; the SwiGLU launch takes blocks in fours (gate/up pairs, I % 32 == 0) and 8 / 4 blocks per workgroup, there
n_blocks = 12, 4, 20 leaves a half-filled workgroup at two tiles.  Every epilogue runs at its own (waves, u).

 (a) Gaussian data, bit for bit against umoe_grouped_gemm on the rows of each tile alone with nt / waves selecting the same K split;
 (b) small-integer data (every product and sum exact in fp32) against the float64 product.  SwiGLU: the device's expf is not the host's, so
     bf16(silu) may be either bf16 neighbour of the float64 value; y must be bf16(si * up) for one of the two;
 (c) guards, checked in every run of (a) and (b) and once on their own: NaN in the pad rows of the row-major source of the re-lay and in
     the weight blocks behind n_blocks; a sentinel in the pad rows and tail columns of row-major outputs, the gaps of ldo > N, and behind
     the operand-order tiles;
 (d) pack_rows with the norm against umoe_router_fwd(norm_only) + a host re-lay, bit for bit; pad rows zero."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

bf16, f64 = torch.bfloat16, torch.float64
BF16, RESID, SWIGLU, F32 = 0, 1, 2, 3
SENT = 7.0
NAN = float("nan")
ROWS = [18, 32, 34, 48, 64]
KS = [2048, 2752, 1376]
# name -> (epilogue, waves, u, (nt, waves) of the 16-row launch with the same K split, n_blocks of three groups, cut: n_valid = 16 nb - cut)
EPIS = {
    "qkv": (BF16, 4, 16, (1, 0), [3, 2, 1], 0),
    "o_proj": (RESID, 4, 16, (1, 0), [3, 1, 2], 4),
    "head": (F32, 4, 8, (2, 0), [3, 5, 1], 12),
    "head_small": (F32, 4, 16, (1, 0), [2, 3, 1], 0),
    "head_large": (F32, 4, 2, (8, 4), [3, 1, 5], 5),
    "gate_up": (SWIGLU, 8, 1, (2, 8), [12, 4, 20], 0),
    "down": (BF16, 8, 2, (1, 8), [3, 5, 1], 0),
}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from unimoe_audio_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def host_pack(x, K):
    """rows [S, K] -> operand-order tiles, flat: [tile][k-step i][lane = quarter * 16 + row][8]; pad rows zero"""
    S = x.shape[0]
    T = (S + 15) // 16
    p = torch.zeros(T * 16, K, dtype=x.dtype)
    p[:S] = x[:, :K]
    return p.view(T, 16, 4, K // 32, 8).permute(0, 3, 2, 1, 4).contiguous().reshape(-1)


def host_unpack(t, tiles, K):
    return t[:tiles * 16 * K].view(tiles, K // 32, 4, 16, 8).permute(0, 3, 2, 1, 4).reshape(tiles * 16, K)


def bits(t):
    return t.view(torch.int16 if t.dtype == bf16 else torch.int32)


def make(name, rows, K, n_groups, kind, seed):
    """host data of one launch: per group A [rows, K], weights, bias, resid"""
    epi, waves, u, _, nbs, cut = EPIS[name]
    g = torch.Generator().manual_seed(seed)
    ks = [KS[(KS.index(K) + i) % 3] for i in range(n_groups)]
    groups = []
    for i in range(n_groups):
        k, nb = ks[i], nbs[i]
        N = 8 * nb if epi == SWIGLU else 16 * nb
        nw = 2 if epi == SWIGLU else 1
        if kind == "int":
            r = 8 if 512 <= k < 2048 else 4
            A = (torch.randint(-r, r + 1, (rows, k), generator=g).to(f64) / 8).to(bf16)
            ws = [(torch.randint(-4, 5, (N, k), generator=g).to(f64) / 16).to(bf16) for _ in range(nw)]
            b = (torch.randint(-64, 65, (N,), generator=g).to(f64) / 128).float()
        else:
            A = torch.randn(rows, k, generator=g).to(bf16)
            ws = [(torch.randn(N, k, generator=g) * k ** -0.5).to(bf16) for _ in range(nw)]
            b = torch.randn(N, generator=g) * 0.5
        groups.append(dict(k=k, nb=nb, N=N, A=A, w=ws, bias=b if name == "qkv" else None,
                           resid=torch.randn(rows, N, generator=g).to(bf16) if epi == RESID else None))
    n_valid = 16 * max(nbs[:n_groups]) - cut
    return dict(name=name, epi=epi, waves=waves, u=u, rows=rows, groups=groups, n_valid=n_valid)


def run_wide(c, dev):
    """the wide launch with every guard of (c) in place -> per group the output buffer (with its margins)"""
    from unimoe_audio_amd import ops
    rows, epi = c["rows"], c["epi"]
    tiles = (rows + 15) // 16
    ws, bs, outs, biases, resids, keep = [], [], [], [], [], []
    ldo = 16 * max(q["nb"] for q in c["groups"]) + 12          # ldo > N: a gap behind every row
    for q in c["groups"]:
        k, nb = q["k"], q["nb"]
        if epi == SWIGLU:
            wp = ops.pack_gate_up(q["w"][0].to(dev), q["w"][1].to(dev))
        else:
            wp = ops.pack_weight(q["w"][0].to(dev))
        wpad = torch.full((wp.numel() + 3 * 16 * k,), NAN, dtype=bf16, device=dev)         # NaN blocks behind n_blocks
        wpad[:wp.numel()] = wp
        src = torch.full((tiles * 16 + 2, k + 8), NAN, dtype=bf16, device=dev)             # NaN pad rows (and columns behind K) in the source
        src[:rows, :k] = q["A"].to(dev)
        b = torch.full((tiles * 16 * k + 64,), SENT, dtype=bf16, device=dev)
        ops.pack_rows(src[:rows, :k], out=b)
        q["packed"] = b
        if epi == SWIGLU:
            o = torch.full((tiles * 16 * q["N"] + 64,), SENT, dtype=bf16, device=dev)
        else:
            o = torch.full((tiles * 16 + 4, ldo), SENT, dtype=torch.float32 if epi == F32 else bf16, device=dev)
        ws.append(wpad); bs.append(b); outs.append(o)
        biases.append(None if q["bias"] is None else q["bias"].to(dev))
        if epi == RESID:
            r = torch.full((tiles * 16 + 4, ldo), NAN, dtype=bf16, device=dev)
            r[:rows, :q["N"]] = q["resid"].to(dev)
            resids.append(r)
    ops.gemm_wide(ws, [q["nb"] for q in c["groups"]], [q["k"] for q in c["groups"]], rows, bs, outs, epilogue=epi, waves=c["waves"], u=c["u"],
                  bias=biases if any(b is not None for b in biases) else None, resid=resids or None,
                  n_valid=None if epi == SWIGLU else c["n_valid"])
    torch.cuda.synchronize()
    return [o.cpu() for o in outs]


def check_guards(c, outs):
    rows, epi = c["rows"], c["epi"]
    tiles = (rows + 15) // 16
    for q, o in zip(c["groups"], outs):
        pk = q["packed"].cpu()
        k = q["k"]
        assert torch.equal(bits(pk[:tiles * 16 * k]), bits(host_pack(q["A"], k))), "re-lay"          # pad rows zero, source NaN not read
        assert bool((pk[tiles * 16 * k:] == SENT).all())
        if epi == SWIGLU:
            I = q["N"]
            y = host_unpack(o, tiles, I)
            assert bool(torch.isfinite(y.float()).all())
            assert bool((y[rows:] == 0).all()), "pad rows of the operand-order output are zero"
            assert bool((o[tiles * 16 * I:] == SENT).all())
        else:
            nv = min(q["N"], c["n_valid"])
            assert bool(torch.isfinite(o[:rows, :nv].float()).all())
            assert bool((o[rows:] == SENT).all()), "pad rows stored"
            assert bool((o[:rows, nv:] == SENT).all()), "tail columns / ldo gap stored"


def result(c, q, o):
    rows = c["rows"]
    if c["epi"] == SWIGLU:
        return host_unpack(o, (rows + 15) // 16, q["N"])[:rows]
    return o[:rows, :min(q["N"], c["n_valid"])]


def ref16(c, dev):
    """umoe_grouped_gemm on the rows of each tile alone, the 16-row kernel with the same K split"""
    from unimoe_audio_amd import ops
    epi, rows = c["epi"], c["rows"]
    nt, waves = EPIS[c["name"]][3]
    outs = []
    for q in c["groups"]:
        wp = ops.pack_gate_up(q["w"][0].to(dev), q["w"][1].to(dev)) if epi == SWIGLU else ops.pack_weight(q["w"][0].to(dev))
        nv = q["N"] if epi == SWIGLU else min(q["N"], c["n_valid"])
        o = torch.zeros((rows, q["N"]), dtype=torch.float32 if epi == F32 else bf16, device=dev)
        bias = None if q["bias"] is None else q["bias"].to(dev)
        resid = None if q["resid"] is None else q["resid"].to(dev)
        for r0 in range(0, rows, 16):
            r1 = min(r0 + 16, rows)
            tab = ops.GroupTable([dict(w=wp, bias=bias, static_count=r1 - r0, n_blocks=q["nb"], k=q["k"])], dev)
            ops.grouped_gemm(tab, q["A"][r0:r1].to(dev).contiguous(), o[r0:r1], max_rows=r1 - r0, epilogue=epi,
                             resid=None if resid is None else resid[r0:r1], n_valid=nv, nt=nt, waves=waves)
        torch.cuda.synchronize()
        outs.append(o.cpu()[:, :nv])
    return outs


def neighbours(s64):
    """the bf16 values next below-or-equal and above-or-equal a float64 tensor"""
    nb = s64.float().to(bf16)
    b = nb.view(torch.int16).to(torch.int32)
    cands = torch.stack([nb.to(f64), (b - 1).to(torch.int16).view(bf16).to(f64), (b + 1).to(torch.int16).view(bf16).to(f64)])
    inf = torch.full_like(s64, float("inf"))
    lo = torch.where(cands <= s64, cands, -inf).max(0).values
    hi = torch.where(cands >= s64, cands, inf).min(0).values
    return lo, hi


def check_fp64(c, outs):
    for q, o in zip(c["groups"], outs):
        got = result(c, q, o)
        A = q["A"].to(f64)
        accs = [A @ w.to(f64).t() for w in q["w"]]
        assert all(bool((a.float().to(f64) == a).all()) for a in accs)          # exact in fp32: no rounding inside the kernel's sums
        if c["epi"] == SWIGLU:
            gt, up = accs[0].float().to(bf16).to(f64), accs[1].float().to(bf16).to(f64)
            lo, hi = neighbours(gt / (1.0 + torch.exp(-gt)))
            y_lo, y_hi = (lo * up).float().to(bf16), (hi * up).float().to(bf16)          # (a product of two bf16 values is exact in fp32)
            ok = (bits(got) == bits(y_lo)) | (bits(got) == bits(y_hi)) | ((got == 0) & (y_lo == 0))
            assert bool(ok.all()), (c["name"], int((~ok).sum()))
            continue
        v = accs[0] if q["bias"] is None else accs[0] + q["bias"].to(f64)
        v = v[:, :got.shape[1]].float()                                             # (ints / 128: exact)
        if c["epi"] == F32:
            want = v.to(bf16).float()
        elif c["epi"] == BF16:
            want = v.to(bf16)
        else:
            want = (q["resid"][:, :got.shape[1]].float() + v.to(bf16).float()).to(bf16)      # one fp32 addition, as the kernel's
        assert torch.equal(bits(got), bits(want)), (c["name"], q["k"])


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", list(EPIS))
def test_wide_bit_for_bit_against_the_16_row_kernel(dev, name, rows):
    for K in KS:
        for n_groups in (1, 3):
            c = make(name, rows, K, n_groups, "gauss", 1000 * rows + K + n_groups)
            outs = run_wide(c, dev)
            check_guards(c, outs)
            for q, o, want in zip(c["groups"], outs, ref16(c, dev)):
                got = result(c, q, o)
                assert torch.equal(bits(got), bits(want)), (name, rows, K, n_groups, q["k"], int((bits(got) != bits(want)).sum()))


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", list(EPIS))
def test_wide_exact_against_fp64(dev, name, rows):
    for K in KS:
        for n_groups in (1, 3):
            c = make(name, rows, K, n_groups, "int", 2000 * rows + K + n_groups)
            outs = run_wide(c, dev)
            check_guards(c, outs)
            check_fp64(c, outs)


@pytest.mark.parametrize("name", list(EPIS))
def test_wide_guards(dev, name):
    """pad rows, tail columns, ldo gaps and the NaN-filled surroundings at the two partial-tile row counts"""
    for rows in (18, 34):
        c = make(name, rows, 1376, 3, "gauss", rows)
        check_guards(c, run_wide(c, dev))


def test_wide_refusals(dev):
    from unimoe_audio_amd import _lib, ops
    c = make("down", 32, 1376, 1, "gauss", 1)
    q = c["groups"][0]
    w, b = ops.pack_weight(q["w"][0].to(dev)), ops.pack_rows(q["A"].to(dev))
    o = torch.zeros((80, q["N"]), dtype=bf16, device=dev)
    for rows, epi, waves, u in [(16, BF16, 8, 2), (65, BF16, 8, 2), (32, BF16, 8, 1), (32, F32, 8, 2), (32, SWIGLU, 8, 1)]:
        with pytest.raises(_lib.UmoeError):
            ops.gemm_wide([w], [q["nb"]], [q["k"]], rows, [b], [o], epilogue=epi, waves=waves, u=u)          # (3 blocks: no gate/up fours)


@pytest.mark.parametrize("rows", [18, 34, 64])
def test_pack_rows(dev, rows):
    from unimoe_audio_amd import _lib as L, ops
    g = torch.Generator().manual_seed(rows)
    tiles = (rows + 15) // 16
    for K in KS + [4096]:
        x = torch.randn(rows, K, generator=g).to(bf16)
        src = torch.full((tiles * 16, K + 16), NAN, dtype=bf16, device=dev)
        src[:rows, :K] = x.to(dev)
        got = ops.pack_rows(src[:rows, :K]).cpu()
        assert torch.equal(bits(got), bits(host_pack(x, K))), K
        assert bool((host_unpack(got, tiles, K)[rows:] == 0).all())
    for K in (2048, 4096):
        x = (torch.randn(rows, K, generator=g) * 3).to(bf16).to(dev)
        nw = (1 + 0.1 * torch.randn(K, generator=g)).to(bf16).to(dev)
        h = torch.full((rows, K), NAN, dtype=bf16, device=dev)
        a = L.RouterArgs(x=x.data_ptr(), norm_w=nw.data_ptr(), h_out=h.data_ptr(), S=rows, D=K, n_dyn=9, n_real=8, n_fix=2, logits_bf16=1,
                         rms_eps=1e-6, norm_only=1)
        L.check(L.lib().umoe_router_fwd(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "umoe_router_fwd")
        src = torch.full((tiles * 16, K), NAN, dtype=bf16, device=dev)
        src[:rows] = x
        got = ops.pack_rows(src[:rows], norm_w=nw, rms_eps=1e-6).cpu()
        torch.cuda.synchronize()
        assert torch.equal(bits(got), bits(host_pack(h.cpu(), K))), K
        assert bool((host_unpack(got, tiles, K)[rows:] == 0).all())
