"""WP12 (bf16 expert weights in 12 bits, lossless: unimoe_audio_amd/w12.py, include/umoe.h): the packer's round trip, the exception
list, the cap -- and the kernel's decode arithmetic (flat_w12_frag, the exception cursor of flat_w12_cursor / flat_w12_patch) restated
in integer torch over the packed bytes."""
import torch

from unimoe_audio_amd import w12


def _rows(N, K, seed=0, std=0.02):
    torch.manual_seed(seed)
    return (torch.randn(N, K) * std).to(torch.bfloat16)


def _bits(vals):
    return torch.tensor([v - 0x10000 if v >= 0x8000 else v for v in vals], dtype=torch.int16).view(torch.bfloat16)


def _round_trip(W):
    N, K = W.shape
    p = w12.wp16_from_rows(W)
    r = w12.pack(p, K // 32)
    assert r is not None
    d, m = r
    assert d.dtype == torch.uint8 and d.numel() == N * K * 3 // 2 and m.numel() == N // 16 * w12.META
    assert torch.equal(w12.unpack(d, m, K // 32), p)
    assert torch.equal(w12.rows_from_wp16(w12.unpack(d, m, K // 32), N, K).view(torch.int16), W.view(torch.int16))
    _kernel_decode_matches(p, d, m, K // 32)
    return d, m


def _kernel_decode_matches(p, d, m, KB):
    """flat_w12_frag + the cursor walk of every wave over its K range, as the kernel does them, against the WP16 operand dwords."""
    NB = m.numel() // w12.META
    CS = w12.steps_per_chunk(KB)
    blk = d.view(NB, KB * 768).to(torch.int64)
    lo = blk[:, : KB * 512].view(NB, KB // CS, 64, CS, 2, 4)                       # [nb][chunk][lane][step][l0 / l1][byte]
    cw = blk[:, KB * 512:].view(NB, KB // CS, 64, CS, 4)
    word = lambda b: b[..., 0] | b[..., 1] << 8 | b[..., 2] << 16 | b[..., 3] << 24
    l0, l1, c = word(lo[..., 0, :]), word(lo[..., 1, :]), word(cw)                 # [nb][chunk][lane][step]
    mm = m.view(NB, w12.META).to(torch.int64) & 0xFFFFFFFF
    wb4 = ((mm[:, w12.META - 1] & 0xFF) * 0x01010101).view(NB, 1, 1, 1)
    hl = (((c & 0x07070707) + wb4) | ((c & 0x08080808) << 4)) & 0xFFFFFFFF
    hh = ((((c >> 4) & 0x07070707) + wb4) | (c & 0x80808080)) & 0xFFFFFFFF

    def perm(s0, s1, sel):                                                          # v_perm_b32: selector 0..3 -> s1, 4..7 -> s0
        out = torch.zeros_like(s0)
        for b in range(4):
            k = (sel >> (8 * b)) & 0xFF
            src = s1 if k < 4 else s0
            out |= ((src >> (8 * (k & 3))) & 0xFF) << (8 * b)
        return out
    op = torch.stack([perm(hl, l0, 0x05010400), perm(hh, l0, 0x05030402), perm(hl, l1, 0x07010600), perm(hh, l1, 0x07030602)], -1)
    op = op.permute(0, 1, 3, 2, 4).reshape(NB, KB, 64, 4)                          # [nb][k-step][lane][dword]
    # the patch path: every wave walks its K range with the cursor the kernel keeps (8 waves, the K split of flat_gateup / flat_down)
    if KB % 2 == 0:
        bounds = [2 * ((KB // 2 * w) // 8) for w in range(9)]
    else:
        bounds = [(KB * w) // 8 for w in range(9)]
    seen = 0
    for nb in range(NB):
        ent = mm[nb].tolist()
        for w in range(8):
            i0, i1 = bounds[w], bounds[w + 1]
            cur = sum(1 for l in range(33) if (ent[l] >> 25) < i0)
            for ii in range(i0, i1):
                while (ent[cur] >> 25) == ii:
                    en = ent[cur]
                    lane, j, val = (en >> 19) & 63, (en >> 16) & 7, en & 0xFFFF
                    sh = (j & 1) * 16
                    op[nb, ii, lane, j >> 1] = (int(op[nb, ii, lane, j >> 1]) & ~(0xFFFF << sh) & 0xFFFFFFFF) | (val << sh)
                    cur += 1
                    seen += 1
            assert cur <= 32
    assert seen == int(w12.exceptions_per_block(m).sum())
    ref = p.view(NB, KB, 64, 4, 2).to(torch.int64) & 0xFFFF
    assert torch.equal(op, ref[..., 0] | ref[..., 1] << 16)


def test_round_trip_on_synthetic_weights():
    for N, K in ((32, 2048), (32, 1376)):          # KB 64 (2-step chunks) and 43 (odd: 1-step chunks)
        d, m = _round_trip(_rows(N, K))
        assert int(w12.exceptions_per_block(m).max()) <= w12.CAP


def test_round_trip_with_planted_special_values():
    for N, K in ((32, 2048), (32, 1376)):
        W = _rows(N, K, 1)
        sp = _bits([0x0000, 0x8000, 0x0001, 0x807F, 0x7F80, 0xFF80, 0x7FC1, 0xFFFF, 0x7FA5, 0x4100, 0x3080])   # +-0, denormals, +-inf, NaNs, 8.0, 2^-30
        W[3, 5:5 + sp.numel()] = sp
        W[17, K - 3:] = sp[:3]
        W[31, 0] = sp[6]
        d, m = _round_trip(W)
        assert int(w12.exceptions_per_block(m)[0]) >= sp.numel()


def test_block_spanning_more_than_16_binades_and_a_constant_block():
    K = 2048
    W = _rows(32, K, 2)
    e = torch.arange(K) % 40 - 30                    # 40 binades in every row of block 0: most values leave the window ...
    W[:16] = (torch.exp2(e.float()) * 1.5).to(torch.bfloat16)
    p = w12.wp16_from_rows(W)
    assert w12.pack(p, K // 32) is None              # ... and the matrix is not packable
    W[:16] = _rows(16, K, 3)
    W[0, :20] = (torch.exp2(torch.arange(20).float() - 25) * 1.25).to(torch.bfloat16)      # a few values over 20 binades: exceptions
    W[16:] = torch.tensor(0.0123).to(torch.bfloat16)                                        # a constant block
    d, m = _round_trip(W)
    assert int(w12.exceptions_per_block(m)[1]) == 0
    W[16:] = 0                                                                              # ... of zeros: the window covers them
    d, m = _round_trip(W)
    assert int(w12.exceptions_per_block(m)[1]) == 0


def test_several_exceptions_in_one_lane_unit():
    for K in (2048, 1376):
        W = _rows(16, K, 4)
        W[5, 8:16] = 0                               # all eight elements of one lane's k-step
        W[5, 16:19] = _bits([0x4100, 0x0000, 0x3080])
        q = K // 4
        W[9, q + 24], W[9, q + 26], W[9, q + 31] = 0, 8.0, 2.0 ** -30       # three in one unit of another K quarter
        d, m = _round_trip(W)
        assert int(w12.exceptions_per_block(m)[0]) >= 14


def test_over_cap_block_is_not_packable():
    K = 2048
    W = _rows(32, K, 5)
    W = torch.where(W.float().abs() < 2.0 ** -18, torch.full_like(W, 0.01), W)     # no natural exceptions
    p = w12.wp16_from_rows(W)
    assert int(w12.exceptions_per_block(w12.pack(p, K // 32)[1]).max()) == 0
    W[16, : w12.CAP] = 0
    d, m = _round_trip(W)
    assert int(w12.exceptions_per_block(m)[1]) == w12.CAP
    W[16, w12.CAP] = 0                               # one more than the cap in block 1
    assert w12.pack(w12.wp16_from_rows(W), K // 32) is None
    assert w12.pack(w12.wp16_from_rows(W[:16]), K // 32) is not None


def test_no_fallback_on_benchmark_weights():
    """A synthetic-init layer (N(0, 0.02^2), the benchmark's) at the real sizes: 8 routed + 2 shared experts, gate/up and down -- no
    block over the cap, so the flagship never falls back to the bf16 launch."""
    torch.manual_seed(0)
    D, I_d, I_s = 2048, 2752, 1376
    worst = 0
    for n, I in ((8, I_d), (2, I_s)):
        for _ in range(n):
            g, u, dn = ((torch.randn(s) * 0.02).to(torch.bfloat16) for s in ((I, D), (I, D), (D, I)))
            for p, kb in ((w12.wp16_gate_up(g, u), D // 32), (w12.wp16_from_rows(dn), I // 32)):
                r = w12.pack(p, kb)
                assert r is not None
                worst = max(worst, int(w12.exceptions_per_block(r[1]).max()))
    assert worst <= w12.CAP, worst


def _plan(probe, n_wg, S, D=2048, Id=2752, Is=1376):
    import ctypes as C
    from unimoe_audio_amd import _lib
    L = C.CDLL(_lib.build())
    fn = getattr(L, probe)
    fn.argtypes = [C.c_int] * 7 + [C.POINTER(C.c_double), C.c_int]
    out = (C.c_double * (3 + 9 * n_wg))()
    assert fn(n_wg, S, D, Id, Is, 8, 2, out, len(out)) == 0
    return bool(out[0]), out[1], [[int(v) for v in out[3 + 9 * j: 12 + 9 * j]] for j in range(n_wg)]


def test_plan_at_the_wp12_byte_cost_covers_every_pair_and_block_once():
    """The static schedule moe_flat_w12_kernel runs (a pair and a block cost 0.75 of the KiB, the fixed costs stay): contiguous gate/up
    slices within the kernel's variants, every down block of every expert exactly once, and a model makespan between 0.75 of the bf16
    plan's and the bf16 plan's."""
    for n_wg, S in ((256, 16), (256, 2), (256, 6), (240, 16), (240, 2)):
        ok, makespan, rows = _plan("umoe_moe_flat_plan_w12_probe", n_wg, S)
        ok16, makespan16, _ = _plan("umoe_moe_flat_plan_probe", n_wg, S)
        assert ok and ok16 and 0.75 * makespan16 <= makespan < makespan16
        nxt = 0
        for j, r in enumerate(rows):
            assert r[0] == nxt and 4 <= r[1] <= 7 and r[2] == (j + 1 if j < S else 0)
            nxt += r[1]
        assert nxt == 2 * (1376 // 16) + 8 * (2752 // 16)
        cover = {g: [] for g in range(10)}
        for r in rows:
            for k in range(2):
                g, nb0, nd = r[3 + 3 * k: 6 + 3 * k]
                if nd:
                    assert nd <= (10 if g < 2 else 6)
                    cover[g].append((nb0, nd))
        for g, sl in cover.items():
            at = 0
            for nb0, nd in sorted(sl):
                assert nb0 == at
                at += nd
            assert at == 2048 // 16
