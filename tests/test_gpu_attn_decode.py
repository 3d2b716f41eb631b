"""The split-key attention kernel (umoe_attn.hip: attn_kernel<G> + attn_combine_kernel<S>) against a float64 restatement at the
context lengths decode runs at, called straight through ops.attention.

Each split gets chunk = roundup16(ceil(n_keys / splits)) keys and each of its 4 waves takes 16-key tiles at 16w, 16w + 64, ...
alternating between two register buffers, then the waves merge in LDS and the splits in the combine launch.  One launch here
holds rows whose key counts cross every tile, wave, slice and split boundary (1 .. ~4100 keys, different left pads and query
positions), at every split specialisation (1 = direct write, 2 / 4 / 8, generic 3 / 5 / 16) and every GQA instantiation.

The reference reads exactly the bf16 tensors the kernel reads (roped q, K / V cache) and computes scores -> masked softmax -> P V in
float64.  The tolerance discriminates by construction:
  * indicator V (column j = 1 where key % 128 == j): an output element sums ~n/128 probabilities, so one lost, doubled or
    misaddressed key moves it by ~128/n of itself, far above a bf16 ulp at n <= 4100; a second pass uses random V;
  * every cache slot outside [kv_start, kend) holds NaN in K and V, so any read that leaks into a sum shows;
  * self-check: the fp64 reference with the first or the last key of any split's slice dropped must break the bound, so every
    test proves it would see the error it is there for.
Each test prints its measured worst ratios on one line ("ATTN DECODE BOUNDS <case> {...}", shown with pytest -s)."""
import json
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

HD = 128
GEOM = {1: (2, 2), 2: (4, 2), 3: (6, 2), 4: (8, 2), 8: (16, 2), 16: (16, 1)}    # G -> (H, KVH)
SPLITS = (1, 2, 3, 4, 5, 8, 16)
NKEYS = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 511, 512, 513, 810, 1025, 2049, 4100]
LMAX = 4224
SIGMA_K = 0.3        # score std ~0.3: no key's probability falls below ~e^-1.1 of the mean, so dropping ANY key is visible
# per element: |got - ref64| <= C1 * 2^-8 * |ref64| + C2 * max|V|.  The output is rounded to bf16 once (up to 2^-8 relative at the
# bottom of a binade); every other step is fp32.  First MI355X run (the printed lines), over every case: relative
# part up to 0.9961 * 2^-8, absolute slack beyond C1 * 2^-8 |ref| at most 8.7e-9 * max|V| (~2^-27), worst ratio to the bound 0.793;
# the self-check passes with C1 = 1.25, which leaves ~2.7x between the bound and the effect of one key at 4100 keys.
C1, C2 = 1.25, 2.0 ** -18


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from unimoe_audio_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _record(key, rec):
    print(f"\nATTN DECODE BOUNDS {key} {json.dumps(rec)}")


def _layout(nkeys, nq, fused):
    """kv_start (left pad) and q_pos0 per row so that the LAST query of row r sees nkeys[r] keys (fused: nkeys[r] - 1 cached keys
    plus the new token at slot q_pos0).  Valid cache slots: [kv_start, q_pos0 + nq) (fused: [kv_start, q_pos0))."""
    ks, q0 = [], []
    for r, n in enumerate(nkeys):
        s = 3 + (11 * r) % 61
        p = s + n - (1 if fused else nq)
        if p < 0:                      # queries before the first key: they see nothing
            s, p = s - p, 0
        assert p + nq <= LMAX
        ks.append(s)
        q0.append(p)
    return ks, q0


def _caches(rows, KVH, ks, vend, indicator, g):
    """K [rows, KVH, LMAX, HD] bf16 ~ N(0, SIGMA_K^2); V indicator or N(0, 1); NaN outside [ks[r], vend[r])."""
    K = (torch.randn(rows, KVH, LMAX, HD, generator=g) * SIGMA_K).to(torch.bfloat16)
    if indicator:
        V = (torch.arange(LMAX)[:, None] % HD == torch.arange(HD)[None, :]).to(torch.bfloat16).expand(rows, KVH, -1, -1).clone()
    else:
        V = torch.randn(rows, KVH, LMAX, HD, generator=g).to(torch.bfloat16)
    for r in range(rows):
        for t in (K, V):
            t[r, :, : ks[r]] = float("nan")
            t[r, :, vend[r]:] = float("nan")
    return K, V


def _ref_row(q, K, V, ks, q0, ts):
    """float64 attention of one row: q [len(ts), H, HD] (bf16 values), K / V [KVH, LMAX, HD]; query ts[i] sees keys
    [ks, q0 + ts[i] + 1).  Returns out [T, H, HD], and the pieces of the self-check: e [T, H, n] (exp(s - m)), N = e V, D = sum e,
    and the first key index of the window."""
    KVH = K.shape[0]
    T, H = q.shape[0], q.shape[1]
    G = H // KVH
    ts = torch.as_tensor(ts)
    hi = max(q0 + int(ts.max()) + 1, ks)
    Kw = K[:, ks:hi].double()
    Vw = V[:, ks:hi].double()
    s = torch.einsum("tkgd,knd->tkgn", q.double().view(T, KVH, G, HD), Kw) * (HD ** -0.5)
    allowed = torch.arange(ks, hi)[None, :] < (q0 + ts + 1)[:, None]
    s = s.masked_fill(~allowed[:, None, None, :], -math.inf)
    m = s.amax(-1, keepdim=True) if s.shape[-1] else torch.zeros(T, KVH, G, 1, dtype=torch.float64)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.exp(s - m)
    D = e.sum(-1)
    N = torch.einsum("tkgn,knd->tkgd", e, Vw)
    out = torch.where(D[..., None] > 0, N / D.clamp_min(1e-300)[..., None], torch.zeros_like(N))     # nan_to_num of the reference
    return out.reshape(T, H, HD), e.reshape(T, H, -1), N.reshape(T, H, HD), D.reshape(T, H), Vw


def _bound(ref, vmax):
    return C1 * 2.0 ** -8 * ref.abs() + C2 * vmax


def _self_check(got, e, N, D, Vw, ks, q0, ts, splits, vmax, G):
    """Dropping the first or the last key of any non-empty split slice of any query from the reference must break the bound on
    at least one element of that query's output."""
    n_checked = 0
    for i, t in enumerate(ts):
        kend = q0 + t + 1
        nk = max(kend - ks, 0)
        if nk == 0:
            continue
        chunk = (-(-nk // splits) + 15) & ~15
        drop = []
        for sp in range(splits):
            b = ks + sp * chunk
            en = min(b + chunk, kend)
            if b < en:
                drop += [b, en - 1]
        idx = torch.tensor(drop) - ks
        ek = e[i][:, idx]                                        # [H, m]
        vk = Vw[:, idx].repeat_interleave(G, 0)                  # [H, m, HD]
        Nm = N[i][:, None, :] - ek[..., None] * vk
        Dm = D[i][:, None] - ek
        mut = torch.where(Dm[..., None] > 0, Nm / Dm.clamp_min(1e-300)[..., None], torch.zeros_like(Nm))
        viol = ((got[i].double()[:, None, :] - mut).abs() > _bound(mut, vmax)).flatten(start_dim=2).any(-1).any(0)   # [m]
        assert bool(viol.all()), f"self-check: dropping key(s) {[drop[j] for j in (~viol).nonzero().flatten().tolist()]} " \
                                 f"(t={t}, kv_start={ks}, q_pos0={q0}, splits={splits}) stays within the bound"
        n_checked += len(drop)
    return n_checked


class _Stats:
    def __init__(self):
        self.worst = 0.0          # max |d| / bound
        self.c1 = 0.0             # max |d| / (2^-8 |ref|) over indicator-V elements with ref > 0
        self.c2 = 0.0             # max (|d| - C1 2^-8 |ref|)+ / max|V|: the absolute slack the elements need beyond the relative term
        self.selfcheck = 0

    def add(self, got, ref, vmax, indicator, what):
        g = got.double()
        assert bool(torch.isfinite(g).all()), f"{what}: non-finite output (a read outside [kv_start, kend) leaked into a sum)"
        d = (g - ref).abs()
        r = float((d / _bound(ref, vmax)).max())
        self.worst = max(self.worst, r)
        if indicator:
            pos = ref > 0
            if bool(pos.any()):
                self.c1 = max(self.c1, float((d[pos] / (2.0 ** -8 * ref[pos])).max()))
            assert bool((g[~pos] == 0).all()), f"{what}: a column no key addresses is nonzero"
        self.c2 = max(self.c2, float((d - C1 * 2.0 ** -8 * ref.abs()).clamp_min(0).max()) / vmax)
        assert r <= 1.0, f"{what}: |got - ref64| / bound = {r:.3g}"

    def rec(self):
        return {"worst_ratio_to_bound": round(self.worst, 4), "c1_measured": round(self.c1, 4), "c2_measured": self.c2,
                "self_check_drops": self.selfcheck}


def _run_nonfused(dev, G, nq, nkeys, seed, stats, splits_list=SPLITS):
    from unimoe_audio_amd import ops
    H, KVH = GEOM[G]
    rows = len(nkeys)
    ks, q0 = _layout(nkeys, nq, fused=False)
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(rows, nq, H, HD, generator=g).to(torch.bfloat16)
    qd = q.reshape(rows * nq, H * HD).to(dev)
    ksd = torch.tensor(ks, dtype=torch.int32, device=dev)
    q0d = torch.tensor(q0, dtype=torch.int32, device=dev)
    ts = list(range(nq))
    for indicator in (True, False):
        K, V = _caches(rows, KVH, ks, [p + nq for p in q0], indicator, g)
        vmax = float(V[torch.isfinite(V)].abs().max())
        refs = [_ref_row(q[r], K[r], V[r], ks[r], q0[r], ts) for r in range(rows)]
        Kd, Vd = K.to(dev), V.to(dev)
        for splits in splits_list:
            out = ops.attention(qd, Kd, Vd, ksd, q0d, nq, H, splits=splits).cpu().view(rows, nq, H, HD)
            for r in range(rows):
                what = f"G={G} nq={nq} splits={splits} row={r} keys={nkeys[r]} kv_start={ks[r]} q_pos0={q0[r]} indicator={indicator}"
                ref, e, N, D, Vw = refs[r]
                stats.add(out[r], ref, vmax, indicator, what)
                if indicator:
                    stats.selfcheck += _self_check(out[r], e, N, D, Vw, ks[r], q0[r], ts, splits, vmax, G)
        # the caches are inputs only on this path
        assert torch.equal(Kd.cpu().view(torch.int16), K.view(torch.int16)) and torch.equal(Vd.cpu().view(torch.int16), V.view(torch.int16))


@pytest.mark.parametrize("G", [1, 2, 3, 4, 8, 16])
def test_decode_attention_one_query_vs_fp64(dev, G):
    """nq = 1 (decode with the rope applied beforehand): every key count of NKEYS in one launch, at every split count."""
    st = _Stats()
    _run_nonfused(dev, G, 1, NKEYS, 100 + G, st)
    _record(f"decode_nq1_G{G}", st.rec())


@pytest.mark.parametrize("G,nq", [(1, 5), (3, 15), (8, 5), (8, 15), (16, 15), (16, 16), (16, 17)])
def test_attention_several_queries_vs_fp64(dev, G, nq):
    """nq queries per row, causal among themselves; rows with few keys have queries that see no key at all (exact zeros).
    G = 16 with nq >= 16 goes through umoe_attn_prefill_fwd, which hands it to this kernel (the MFMA prefill stops at G = 8)."""
    st = _Stats()
    _run_nonfused(dev, G, nq, NKEYS, 200 + 7 * G + nq, st)
    _record(f"multi_nq{nq}_G{G}", st.rec())


def _rope_torch(x, cos, sin):
    """x [..., HD] bf16, cos / sin [..., HD] bf16: x cos + rotate_half(x) sin with torch's bf16 rounding of every op"""
    from oracle import decode as OD
    return x * cos + OD.rotate_half(x) * sin


@pytest.mark.parametrize("G", [1, 3, 8, 16])
def test_fused_rope_append_decode_vs_fp64(dev, G):
    """qkv_raw path: mRoPE of q and k at three distinct, large positions (tables at the engine's size), the new K / V appended at
    slot q_pos0 by the kernel itself.  The cache slot must equal torch's bf16 rope of the same raw row bit for bit, V must be
    copied bit for bit, no other slot may change; a row with no cached key returns the new V exactly."""
    from oracle import decode as OD
    from unimoe_audio_amd import ops
    H, KVH = GEOM[G]
    rows = len(NKEYS)
    sections = [16, 24, 24]
    ks, q0 = _layout(NKEYS, 1, fused=True)
    max_pos = LMAX + 4104                         # DecodeEngine._pack_weights
    cos_tab, sin_tab = ops.rope_tables(max_pos, HD, 1e6, dev)
    pos3 = torch.tensor([[max_pos - 1 - 5 * r for r in range(rows)],
                         [256 + 173 * r for r in range(rows)],
                         [(q0[r] + 1000 * r) % 8000 + 300 for r in range(rows)]], dtype=torch.int64)
    assert int(pos3.max()) >= 8000 and bool((pos3[0] != pos3[1]).all() and (pos3[1] != pos3[2]).all() and (pos3[0] != pos3[2]).all())
    cos3, sin3 = OD.rope_cos_sin(pos3[:, :, None], HD, 1e6, torch.bfloat16)      # [3, rows, 1, HD]
    cos = OD.mrope_select(cos3, sections)[:, 0]                                  # [rows, HD]
    sin = OD.mrope_select(sin3, sections)[:, 0]
    g = torch.Generator().manual_seed(300 + G)
    ksd = torch.tensor(ks, dtype=torch.int32, device=dev)
    q0d = torch.tensor(q0, dtype=torch.int32, device=dev)
    p3d = pos3.to(torch.int32).contiguous().to(dev)
    st = _Stats()
    for indicator in (True, False):
        qraw = torch.randn(rows, H, HD, generator=g).to(torch.bfloat16)
        kraw = (torch.randn(rows, KVH, HD, generator=g) * SIGMA_K).to(torch.bfloat16)
        if indicator:
            vnew = (torch.tensor(q0)[:, None, None] % HD == torch.arange(HD)[None, None, :]).to(torch.bfloat16).expand(-1, KVH, -1).clone()
        else:
            vnew = torch.randn(rows, KVH, HD, generator=g).to(torch.bfloat16)
        qkv = torch.cat([qraw.reshape(rows, -1), kraw.reshape(rows, -1), vnew.reshape(rows, -1)], 1).contiguous()
        q_rot = _rope_torch(qraw, cos[:, None], sin[:, None])                      # [rows, H, HD]
        k_rot = _rope_torch(kraw, cos[:, None], sin[:, None])                      # [rows, KVH, HD]
        K, V = _caches(rows, KVH, ks, q0, indicator, g)                            # slot q_pos0 is stale: NaN
        K_exp, V_exp = K.clone(), V.clone()
        for r in range(rows):
            K_exp[r, :, q0[r]] = k_rot[r]
            V_exp[r, :, q0[r]] = vnew[r]
        vmax = float(V_exp[torch.isfinite(V_exp)].abs().max())
        refs = [_ref_row(q_rot[r][None], K_exp[r], V_exp[r], ks[r], q0[r], [0]) for r in range(rows)]
        qkvd = qkv.to(dev)
        for splits in SPLITS:
            Kd, Vd = K.to(dev), V.to(dev)
            out = ops.attention(None, Kd, Vd, ksd, q0d, 1, H, splits=splits, qkv_raw=qkvd, cos_tab=cos_tab, sin_tab=sin_tab,
                                pos3=p3d, sections=sections).cpu().view(rows, 1, H, HD)
            tag = f"fused G={G} splits={splits} indicator={indicator}"
            # cache: slot q_pos0 = torch's rope of the raw row / the raw V, every other slot untouched (NaN slots compared as bits)
            assert torch.equal(Kd.cpu().view(torch.int16), K_exp.view(torch.int16)), tag + ": K cache"
            assert torch.equal(Vd.cpu().view(torch.int16), V_exp.view(torch.int16)), tag + ": V cache"
            for r in range(rows):
                what = f"{tag} row={r} keys={NKEYS[r]} kv_start={ks[r]} q_pos0={q0[r]} pos3={pos3[:, r].tolist()}"
                ref, e, N, D, Vw = refs[r]
                if q0[r] == ks[r]:         # no cached key: softmax over the new token alone
                    assert torch.equal(out[r, 0].view(torch.int16), vnew[r].repeat_interleave(G, 0).view(torch.int16)), what
                st.add(out[r], ref, vmax, indicator, what)
                if indicator:
                    st.selfcheck += _self_check(out[r], e, N, D, Vw, ks[r], q0[r], [0], splits, vmax, G)
    _record(f"fused_G{G}", st.rec())


def test_row_by_row_fallback_vs_fp64(dev):
    """rows * nq > 65535 query workgroups: umoe_attn_decode launches row by row (partials reused across rows).  2 rows x 32800
    queries at G = 16 (the MFMA prefill stops at G = 8), checked on a fixed sample of queries."""
    from unimoe_audio_amd import ops
    G, nq, splits = 16, 32800, 3
    H, KVH = GEOM[G]
    rows = 2
    ks, q0 = [5, 0], [9, 31]
    Lmax = 32832
    assert rows * nq > 65535 and max(q0) + nq <= Lmax
    g = torch.Generator().manual_seed(401)
    K = (torch.randn(rows, KVH, Lmax, HD, generator=g) * SIGMA_K).to(torch.bfloat16)
    V = (torch.arange(Lmax)[:, None] % HD == torch.arange(HD)[None, :]).to(torch.bfloat16).expand(rows, KVH, -1, -1).clone()
    for r in range(rows):
        for t in (K, V):
            t[r, :, : ks[r]] = float("nan")
            t[r, :, q0[r] + nq:] = float("nan")
    gd = torch.Generator(device=dev).manual_seed(402)
    qd = torch.randn(rows * nq, H * HD, generator=gd, device=dev).to(torch.bfloat16)
    out = ops.attention(qd, K.to(dev), V.to(dev), torch.tensor(ks, dtype=torch.int32, device=dev),
                        torch.tensor(q0, dtype=torch.int32, device=dev), nq, H, splits=splits)
    ts = sorted(set([0, 1, 2, 3, 15, 16, 17, 63, 64, 65] + list(range(0, nq, 2731)) + [nq - 4, nq - 3, nq - 2, nq - 1]))
    q = qd.view(rows, nq, H, HD)[:, ts].cpu()
    got = out.view(rows, nq, H, HD)[:, ts].cpu()
    st = _Stats()
    for r in range(rows):
        ref, e, N, D, Vw = _ref_row(q[r], K[r], V[r], ks[r], q0[r], ts)
        st.add(got[r], ref, 1.0, True, f"row-by-row row={r}")
        # one key out of n moves an indicator column by ~128/n of itself: below the bf16 bound past ~4100 keys, so the self-check
        # covers the sampled queries that see at most 4100 keys
        short = [i for i, t in enumerate(ts) if q0[r] + t + 1 - ks[r] <= 4100]
        st.selfcheck += _self_check(got[r][short], e[short], N[short], D[short], Vw, ks[r], q0[r], [ts[i] for i in short], splits,
                                    1.0, G)
    _record("row_by_row", st.rec())
