"""GPU suite of gradient accumulation in fp32 main gradients: umoe_tiled_gemm_tn_acc, the accumulate expert composites,
umoe_optim_fold, the optimizer stages on fp32 gradients of bf16 parameters, and train.train_step_accum end to end.

The GEMM cases are test_gpu_gemm_fp64's `tn_case` table (windows of 0 .. 1100 rows, m = 8 .. 264, n % 4 edges, out_row_base, out_col_off,
per-group outputs, forced K splits 2, 3, 4 and the library's choice) plus three ragged groups with the middle one empty; the checkers
and their derivation are in tests/test_grad_accum_cpu.py, which runs them on a host emulation and on planted errors.  The optimizer's
bounds are tests/optim_ref.py's, unchanged, with the fp32 gradient as input.

Measured on MI355X (-s prints them).  Accumulate GEMM, worst error / bound: 0.955 at k = 1 (the bound is then one rounding of the
product plus one of the add), 0.04 - 0.06 at k = 31 .. 33, below 0.011 from k = 127 on, 6.9e-4 under the library's own split of k = 1100.
Optimizer on fp32 gradients: norm 0.02 - 0.03 of its bound, update w 0.70, m 0.58, v 0.45.  Four micro-batches on the 2-layer model:
accumulated gradient 2.8e-8 (relative 2-norm) from the float64 sum, autograd's bf16 `grad +=` 2.7e-3 (printed, not asserted).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import optim_ref as R
import test_gpu_gemm_fp64 as G
import test_gpu_optim as TO
import test_grad_accum_cpu as A

pytestmark = pytest.mark.gpu
GUARD = 16                  # sentinel elements in front of and behind every output buffer (64 bytes: the view stays 16-byte aligned)
SENT = TO.SENT
CH = TO.CH
bf16 = torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from unimoe_audio_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def leave_nothing_behind():
    yield
    import gc
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


# ================================================================================================ GEMM level
def guarded(host, dev):
    n = host.numel()
    flat = torch.full((GUARD + n + GUARD,), SENT, dtype=host.dtype)
    flat[GUARD:GUARD + n] = host.reshape(-1)
    flat = flat.to(dev)
    return flat, flat[GUARD:GUARD + n].view(host.shape)


def guards_intact(flat):
    return bool((flat[:GUARD] == SENT).all()) and bool((flat[-GUARD:] == SENT).all())


def dev_operands(c, dev):
    if "dev" not in c:
        c["dev"] = dict(P=c["P"].to(dev), Q=c["Q"].to(dev), groups=[
            dict(pbuf=d["pbuf"].to(dev), qbuf=d["qbuf"].to(dev)) if d["own"] else {} for d in c["groups"]])
    return c["dev"]


def launch_acc(c, ks, dev, prev, calls=1):
    """`calls` launches of umoe_tiled_gemm_tn_acc into guarded copies of prev -> (out, {group: own out}) on the host"""
    from unimoe_audio_amd import ops
    dv = dev_operands(c, dev)
    flat, out = guarded(prev[0], dev)
    flats, own, groups = [flat], {}, []
    for i, (d, t) in enumerate(zip(c["groups"], dv["groups"])):
        q = dict(m=d["m"], n=d["n"], p_col_off=d["pco"], q_col_off=d["qco"], out_row_base=d["out_row_base"], out_col_off=d["oc"])
        if d["dev"]:
            q.update(k_off_dev=torch.tensor([d["k_off"]], dtype=torch.int32, device=dev), k_count_dev=torch.tensor([d["k"]], dtype=torch.int32, device=dev))
        else:
            q.update(k_off=d["k_off"], k=d["k"])
        if d["own"]:
            f, own[i] = guarded(prev[1][i], dev)
            flats.append(f)
            q.update(p=t["pbuf"], q=t["qbuf"], out=own[i])
        groups.append(q)
    for _ in range(calls):
        ops.tiled_gemm_tn(groups, dv["P"], dv["Q"], out, k_split=ks, accumulate=True)
    torch.cuda.synchronize()
    assert all(guards_intact(f) for f in flats), f"{c['name']}: a sentinel around an output buffer was overwritten"
    return out.cpu(), {i: t.cpu() for i, t in own.items()}


def eff_split(c, ks):
    if ks >= 0:
        return ks
    eff = G.tn_library_split(c)
    assert eff > 1, f"the library chose k_split = {eff}: the case is meant to be split"
    return eff


@pytest.mark.parametrize("name", A.CASES)
def test_tn_acc_per_element_against_fp64(dev, name):
    """out_after inside prev + sum +- (e_sum + 2^-24 (|prev| + |sum| + e_sum)) with random fp32 prev; NaN in every output row and column
    outside [m) x [n) and in the operand rows outside the windows; nothing outside the windows changes a bit; sentinels intact."""
    c = G.tn_case(name)
    st = G.Stats()
    st.prefix = "GRAD ACCUM"
    for ks in A.splits_of(c):
        prev = A.make_prev(c, "rand", 1)
        got = launch_acc(c, ks, dev, prev)
        A.check_outside(c, prev, got)
        A.check_fp64(c, eff_split(c, ks), prev, got, st)
    st.show(name)


@pytest.mark.parametrize("name", A.CASES)
def test_tn_acc_small_integers_are_exact(dev, name):
    c = A.int_case(name)
    for ks in A.splits_of(c):
        prev = A.make_prev(c, "int", 2)
        got = launch_acc(c, ks, dev, prev)
        A.check_outside(c, prev, got)
        A.check_exact(c, prev, got)


@pytest.mark.parametrize("name", A.CASES)
def test_tn_acc_from_zero_is_the_bf16_entry_and_repeats_exactly(dev, name):
    """from a zeroed out: bf16_rne(out) = umoe_tiled_gemm_tn's output for every split (the K-split sum has the bits the bf16 entry rounds);
    two calls in a row = fp32(fp32(0 + s) + s) from the host, bit for bit; two runs bit-identical"""
    c = G.tn_case(name)
    for ks in A.splits_of(c):
        zero = A.make_prev(c, "zero")
        once = launch_acc(c, ks, dev, zero)
        plain = G.launch_tn(c, ks, dev)
        A.check_from_zero(c, once, (plain[0].cpu(), {i: t.cpu() for i, t in plain[1].items()}))
        twice = launch_acc(c, ks, dev, zero, calls=2)
        A.check_repeat(c, once, twice)
        again = launch_acc(c, ks, dev, zero, calls=2)
        assert torch.equal(A.bits(twice[0]), A.bits(again[0])) and all(torch.equal(A.bits(twice[1][i]), A.bits(again[1][i])) for i in twice[1])


def test_tn_acc_empty_ragged_group_keeps_its_bytes(dev):
    """three ragged groups, the middle one of count 0: its output window keeps a planted NaN payload bit for bit"""
    c = G.tn_case("tn_acc_ragged3")
    assert [d["k"] for d in c["groups"]] == [33, 0, 129] and all(d["dev"] for d in c["groups"])
    prev = A.make_prev(c, "rand", 7)
    e = c["groups"][1]
    rs, cs = slice(e["out_row_base"], e["out_row_base"] + e["m"]), slice(e["oc"], e["oc"] + e["n"])
    prev[0][rs, cs][::3] = torch.full((1,), A.NAN_BITS, dtype=torch.int32).view(torch.float32)
    prev[0][rs, cs][1::3] = -0.0
    got = launch_acc(c, 1, dev, prev)
    A.check_outside(c, prev, got)
    assert torch.equal(A.bits(got[0][rs, cs]), A.bits(prev[0][rs, cs])) and int((A.bits(got[0][rs, cs]) == A.NAN_BITS).sum()) > 1000
    A.check_fp64(c, 1, prev, got, G.Stats())
    c1 = G.tn_case("tn_device_empty")
    p1 = A.make_prev(c1, "nan")
    g1 = launch_acc(c1, 1, dev, p1)
    assert torch.equal(A.bits(g1[0]), A.bits(p1[0]))


def test_tn_acc_refusals_leave_the_output_untouched(dev):
    from unimoe_audio_amd import ops
    from unimoe_audio_amd._lib import UmoeError
    c = G.tn_case("tn_static")
    dv = dev_operands(c, dev)
    prev = A.make_prev(c, "rand", 8)
    flat, out = guarded(prev[0], dev)
    snap = flat.clone()
    ok = dict(m=8, n=8, k_off=3, k=16)
    one = torch.tensor([16], dtype=torch.int32, device=dev)
    mis = flat[GUARD + 1: GUARD + 1 + 16 * c["ldo"]].view(16, c["ldo"])                 # 4 bytes off a 16-byte boundary
    dense = flat[GUARD: GUARD + 16 * 8].view(16, 8)
    bad = [
        lambda: ops.tiled_gemm_tn([ok], dv["P"], dv["Q"], mis, accumulate=True),                                   # misaligned fp32 out
        lambda: ops.tiled_gemm_tn([dict(ok, out=mis)], dv["P"], dv["Q"], out, accumulate=True),                   # ... of a group
        lambda: ops.tiled_gemm_tn([dict(ok, n=6)], dv["P"], dv["Q"], out, accumulate=True),                       # n % 4
        lambda: ops.tiled_gemm_tn([dict(ok, p_col_off=4)], dv["P"], dv["Q"], out, accumulate=True),               # column offset % 8
        lambda: ops.tiled_gemm_tn([dict(ok, out_col_off=2)], dv["P"], dv["Q"], out, accumulate=True),             # out_col_off % 4
        lambda: ops.tiled_gemm_tn([dict(ok, k=-1)], dv["P"], dv["Q"], out, accumulate=True),                      # bad static window
        lambda: ops.tiled_gemm_tn([dict(ok, k_off_dev=one)], dv["P"], dv["Q"], out, accumulate=True),             # k_off_dev without k_count_dev
        lambda: ops.tiled_gemm_tn([ok], dv["P"], dv["Q"], out, k_split=2, accumulate=True),                       # split: not one dense slab
        lambda: ops.tiled_gemm_tn([dict(m=8, n=8, k_off_dev=one, k_count_dev=one)], dv["P"], dv["Q"], dense, k_split=2, accumulate=True),   # split: device window
        lambda: ops.tiled_gemm_tn([dict(ok, m=8)], dv["P"], dv["Q"], dense, k_split=2, accumulate=True),          # split: the groups do not cover the slab
        lambda: ops.tiled_gemm_tn([ok] * 25, dv["P"], dv["Q"], out, accumulate=True),                             # more than 24 groups
        lambda: ops.tiled_gemm_tn([ok], dv["P"], dv["Q"], out.to(bf16), accumulate=True),                         # a bf16 output
        lambda: ops.tiled_gemm_tn([ok], dv["P"], dv["Q"], out),                                                   # an fp32 output for the bf16 entry
    ]
    for i, fn in enumerate(bad):
        with pytest.raises(UmoeError):
            fn()
    torch.cuda.synchronize()
    assert torch.equal(A.bits(flat), A.bits(snap))
    ops.tiled_gemm_tn([dict(ok, out_row_base=8)], dv["P"], dv["Q"], out, accumulate=True)      # and arguments without a fault do run (group 0's window)
    torch.cuda.synchronize()
    assert not torch.equal(A.bits(flat), A.bits(snap)) and guards_intact(flat)


# ================================================================================================ expert composites
def expert_inputs(dev, routed, seed):
    g = torch.Generator().manual_seed(seed)
    D, I, S = 64, 32, 48
    rnd = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(bf16).to(dev)      # noqa: E731
    if routed:
        Gn, counts, offsets = 3, [37, 0, 21], [0, 40, 40, 64]
        rows = 72
        kw = dict(counts=torch.tensor(counts, dtype=torch.int32, device=dev), offsets=torch.tensor(offsets, dtype=torch.int32, device=dev),
                  slot_token=torch.randint(0, S, (rows,), generator=g).to(torch.int32).to(dev))
    else:
        Gn, rows = 2, 2 * S
        kw = dict(row_base=0)
    ws = [(rnd(I, D, sc=0.1), rnd(I, D, sc=0.1), rnd(D, I, sc=0.1)) for _ in range(Gn)]
    kw.update(x=rnd(S, D), h=rnd(rows, I), gu=rnd(rows, 2 * I), dy=rnd(rows, D, sc=0.1), D=D, I=I, max_rows=S)
    return ws, kw, (Gn, D, I, rows)


@pytest.mark.parametrize("routed", [True, False], ids=["routed", "shared"])
def test_expert_composites_accumulate(dev, routed):
    """dx_slots bit-identical to the bf16 composite; from zeroed main grads bf16_rne of the three gradients = the bf16 composite's;
    a second call doubles them exactly (fp32(s + s)); the empty expert's main gradients stay zero"""
    from unimoe_audio_amd import ops
    ws, kw, (Gn, D, I, rows) = expert_inputs(dev, routed, 11 + routed)
    dx0 = torch.full((rows, D), 3.0, dtype=bf16, device=dev)
    dwg, dwu, dwd = ops.experts_swiglu_bwd(ws, dx_slots=dx0, **kw)
    # main gradients stacked the way ops.experts_swiglu_bwd stacks the bf16 ones (the shared experts' K-split slab test is on fp32 elements)
    flat_gu, mgu = guarded(torch.zeros((2, Gn, I, D)), dev)
    flat_d, mgd = guarded(torch.zeros((Gn, D, I)), dev)
    mgs = [(mgu[0, g], mgu[1, g], mgd[g]) for g in range(Gn)]
    dx1 = torch.full((rows, D), 3.0, dtype=bf16, device=dev)
    assert ops.experts_swiglu_bwd(ws, dx_slots=dx1, main_grads=mgs, **kw) == (None, None, None)
    torch.cuda.synchronize()
    assert torch.equal(dx0.view(torch.int16), dx1.view(torch.int16))
    once = [t.clone() for t in (mgu, mgd)]
    for g in range(Gn):
        for got, want, nm in ((mgu[0, g], dwg[g], "gate"), (mgu[1, g], dwu[g], "up"), (mgd[g], dwd[g], "down")):
            A.same_numbers_bits_where_nonzero(got.to(bf16).cpu(), want.cpu(), f"expert {g} dW {nm}")
    if routed:
        assert not mgu[:, 1].any() and not mgd[1].any() and bool(mgu[:, 0].any()) and bool(mgd[2].any())
    dx2 = torch.full((rows, D), 3.0, dtype=bf16, device=dev)
    ops.experts_swiglu_bwd(ws, dx_slots=dx2, main_grads=mgs, **kw)
    torch.cuda.synchronize()
    assert torch.equal(dx0.view(torch.int16), dx2.view(torch.int16))
    for s, t in zip(once, (mgu, mgd)):
        assert torch.equal(A.bits(t), A.bits(s + s))
    assert guards_intact(flat_gu) and guards_intact(flat_d)
    # main gradients that are NOT one stacked slab (each parameter's run of a flat buffer) give the same bits
    sep = [tuple(torch.zeros_like(m) for m in tr) for tr in mgs]
    ops.experts_swiglu_bwd(ws, dx_slots=dx2, main_grads=sep, **kw)
    torch.cuda.synchronize()
    for g in range(Gn):
        for a, b in zip(sep[g], (once[0][0, g], once[0][1, g], once[1][g])):
            A.same_numbers_bits_where_nonzero(a.cpu(), b.cpu(), f"expert {g}: separate main gradients")
    from unimoe_audio_amd._lib import UmoeError
    with pytest.raises(UmoeError):
        ops.experts_swiglu_bwd(ws, dx_slots=dx2, main_grads=[tuple(m.to(bf16) for m in tr) for tr in mgs], **kw)
    with pytest.raises(UmoeError):
        ops.experts_swiglu_bwd(ws, dx_slots=dx2, main_grads=mgs[:1], **kw)


# ================================================================================================ fold
FOLD_OFFSETS = {8: (3, 3), 5: (1, 0), 6: (0, 1), 4: (0, 4)}          # (g, main) element offsets: head / tail path; never co-aligned (twice); aligned


def fold_state(dev, seed, null_at=(3,)):
    rng = np.random.default_rng(seed)
    out = []
    for i, n in enumerate(TO.SIZES):
        og, om = FOLD_OFFSETS.get(i, (0, 0))
        t = dict(n=n, bufs={})
        t["bufs"]["g"], t["g"] = TO.padded(dev, rng.normal(0, 2e-3, n), bf16, og)
        t["bufs"]["main"], t["main"] = TO.padded(dev, rng.normal(0, 1.0, n), torch.float32, om)
        t["null"] = i in null_at
        out.append(t)
    return out


class FoldTable:
    def __init__(self, tensors, chunks=None):
        from unimoe_audio_amd import optim as O
        self.tensors = tensors
        dev = tensors[0]["g"].device
        self.th = np.zeros(len(tensors), dtype=O.FOLD_DTYPE)
        for i, t in enumerate(tensors):
            self.th[i] = (0 if t["null"] else t["g"].data_ptr(), t["main"].data_ptr(), t["n"])
        self.chh = O.build_chunk_table([t["n"] for t in tensors], CH) if chunks is None else chunks
        self.td = torch.from_numpy(self.th.view(np.uint8).reshape(-1).copy()).to(dev)
        self.cd = torch.from_numpy(self.chh.view(np.int64).reshape(-1).copy()).to(dev)

    def fold(self, grid_cap=0, host=True, **over):
        from unimoe_audio_amd import _lib as L
        a = dict(tensors=self.td.data_ptr(), n_tensors=len(self.tensors), chunks=self.cd.data_ptr(), n_chunks=len(self.chh), chunk_elems=CH,
                 ht=self.th.ctypes.data if host else None, hc=self.chh.ctypes.data if host else None)
        a.update(over)
        return L.lib().umoe_optim_fold(a["tensors"], a["n_tensors"], a["chunks"], a["n_chunks"], a["chunk_elems"], a["ht"], a["hc"], grid_cap,
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("cap", [0, 3])
def test_fold_is_main_plus_g_and_clears_g(dev, cap):
    tensors = fold_state(dev, 70)
    before = [(t["main"].cpu().clone(), t["g"].cpu().clone()) for t in tensors]
    snap = TO.snapshot(tensors)
    tb = FoldTable(tensors)
    assert len(tb.chh) == 11
    assert tb.fold(grid_cap=cap) == 0
    torch.cuda.synchronize()
    for t, (m0, g0), s in zip(tensors, before, snap):
        if t["null"]:
            assert TO.unchanged([t], [s])
        else:
            A.check_fold(m0, g0, t["main"].cpu(), t["g"].cpu())
    assert TO.sentinels_intact(tensors)
    assert tb.fold(grid_cap=cap) == 0                       # folding the cleared gradients again changes nothing
    torch.cuda.synchronize()
    for t, (m0, g0) in zip(tensors, before):
        if not t["null"]:
            assert torch.equal(A.bits(t["main"]), A.bits(m0 + g0.float()))


def test_fold_refusals_write_nothing(dev):
    from unimoe_audio_amd import _lib as L
    from unimoe_audio_amd.optim import build_chunk_table
    tensors = fold_state(dev, 71)
    tb = FoldTable(tensors)
    snap = TO.snapshot(tensors)
    sizes = [t["n"] for t in tensors]
    crossing = build_chunk_table(sizes, CH)
    crossing["first"][-1] = 4 * CH
    overlap = build_chunk_table(sizes, CH)
    overlap["first"][-1] = 8
    bad_tensor = build_chunk_table(sizes, CH)
    bad_tensor["tensor"][0] = len(sizes)
    no_main = tb.th.copy()
    no_main["main"][8] = 0
    refused = [tb.fold(tensors=None), tb.fold(chunks=None), tb.fold(chunk_elems=0), tb.fold(chunk_elems=12), tb.fold(hc=None), tb.fold(ht=None),
               tb.fold(n_tensors=-1), tb.fold(grid_cap=-1), tb.fold(ht=no_main.ctypes.data)]
    refused += [tb.fold(hc=t.ctypes.data) for t in (crossing, overlap, bad_tensor)]
    assert all(rc < 0 for rc in refused), refused
    assert L.lib().umoe_last_error()
    torch.cuda.synchronize()
    assert TO.unchanged(tensors, snap)
    # an unchecked device table with the same faults: the kernel skips those chunks
    tb2 = FoldTable(tensors, chunks=np.concatenate([crossing[-1:], bad_tensor[:1]]))
    assert tb2.fold(host=False) == 0
    torch.cuda.synchronize()
    assert TO.unchanged(tensors, snap)
    assert FoldTable(tensors, chunks=build_chunk_table([0] * len(sizes), CH)).fold() == 0          # an empty table is a no-op


# ================================================================================================ optimizer stages on fp32 gradients
G32_OFFSETS = {8: (3, 3, 3, 3, 3), 5: (1, 0, 0, 0, 0), 6: (0, 1, 0, 0, 0)}


def mixed_state(dev, seed, null_at=()):
    """TO.make_state's records (bf16 p / g with masters; tensor 7 an fp32 parameter) with the gradients of tensors 2, 4, 5, 6, 8 replaced by
    fp32 main gradients of the bf16 parameters (flag bit 1); tensors 1, 3 keep bf16 gradients; null_at: gradient NULL"""
    tensors = TO.make_state(dev, seed, offsets=G32_OFFSETS)
    rng = np.random.default_rng(seed + 1)
    for i in (2, 4, 5, 6, 8):
        t = tensors[i]
        off = G32_OFFSETS.get(i, (0, 0, 0, 0, 0))[1]
        t["bufs"]["g"], t["g"] = TO.padded(dev, rng.normal(0, 2e-3, t["n"]), torch.float32, off)       # fp32 values bf16 cannot hold
        t["g32"] = True
    for i in null_at:
        tensors[i]["g_kept"], tensors[i]["g"] = tensors[i]["g"], None
    return tensors


def tables_of(tensors):
    from unimoe_audio_amd import optim as O
    tb = R.Tables(tensors, CH, 2)
    for i, t in enumerate(tensors):
        if t.get("g32"):
            tb.th["p_fp32"][i] |= O.G_FP32
    assert sorted(set(tb.th["p_fp32"].tolist())) == [0, 1, 2]
    tb.td.copy_(torch.from_numpy(tb.th.view(np.uint8).reshape(-1).copy()))
    return tb


@pytest.mark.parametrize("t0", [0, 999])
def test_norm_clip_and_update_with_fp32_gradients(dev, t0):
    tensors = mixed_state(dev, 80 + t0)
    grads = [TO.host(t, "g") for t in tensors]
    assert any(not np.array_equal(g, R.bf16_to_f32(R.bf16_rne(g))) for g in grads)
    hy = TO.hyper(max_norm=0.05)
    recs = []
    for cap in (0, 3):
        tb = tables_of(tensors)
        tb.counters[0] = t0
        assert tb.sqsum(grid_cap=cap) == 0 and tb.scalars(hy) == 0
        torch.cuda.synchronize()
        recs.append(tb.rec.cpu().numpy().tobytes() + tb.partial.cpu().numpy().tobytes())
    assert recs[0] == recs[1] and not tb.flags.any()
    rec = tb.record()
    norm, _, bcs = R.scalars_fp64(grads, 0.05, [h["betas"] for h in TO.HP], t0)
    nb = R.norm_rel_bound(CH)
    print(f"\nNORM (fp32 gradients) t={t0}: {rec['norm']!r} vs {norm!r}: error / bound {abs(float(rec['norm']) - norm) / (nb * norm):.3f}")
    assert abs(float(rec["norm"]) - norm) <= nb * norm
    clip = min(1.0, 0.05 / (float(rec["norm"]) + 1e-6))
    assert clip < 1.0 and abs(float(rec["clip"]) - clip) <= R.CLIP_REL_BOUND * clip
    before = TO.before_of(tensors)
    assert tb.adamw(hy, grid_cap=3) == 0
    torch.cuda.synchronize()
    TO.check_update(tensors, before, rec, label=f"fp32 gradients of bf16 parameters, t={t0}")
    assert TO.sentinels_intact(tensors)
    assert all(np.array_equal(TO.host(t, "g"), g) for t, g in zip(tensors, grads))            # the gradients are read only


def test_null_gradients_and_the_skip_with_fp32_gradients(dev):
    tensors = mixed_state(dev, 90, null_at=(4,))
    for k in ("g_kept", "m", "v", "master"):
        tensors[4][k].fill_(float("nan"))                                                       # a left-out tensor's NaN does not matter
    tb = tables_of(tensors)
    hy = TO.hyper(max_norm=0.05)
    snap4 = TO.snapshot([tensors[4]])
    live = [t for i, t in enumerate(tensors) if i != 4]
    before = TO.before_of(live)
    TO.run_all(tb, hy)
    rec = tb.record()
    assert rec["skip"] == 0 and tb.counters.tolist() == [1, 0] and TO.unchanged([tensors[4]], snap4)
    TO.check_update(live, before, rec, label="NULL gradient beside fp32 gradients")
    for what, at in (("inf", CH), ("nan", CH - 1)):                                            # the bad value sits in a MAIN gradient
        big = tensors[8]
        assert big["g"].dtype == torch.float32
        clean = big["g"].clone()
        big["g"][at] = float(what)
        snap = TO.snapshot(tensors)
        TO.run_all(tb, hy)
        assert tb.record()["skip"] == 1 and int(tb.flags.sum()) == 1 and TO.unchanged(tensors, snap)
        big["g"].copy_(clean)
    assert tb.counters.tolist() == [1, 2] and TO.sentinels_intact(live)


# ================================================================================================ end to end
def micro_batch(cfg, seed, B=2, T=40):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, 290, (B, T), generator=g)
    am = torch.ones(B, T, dtype=torch.long)
    am[0, :6] = 0
    ids[:, -5:-2] = cfg.codec_placeholder_value
    codec = torch.randint(0, 1024, (B * 3, cfg.codec_channels), generator=g)
    labels = torch.randint(0, 1024, (B, T, cfg.codec_channels), generator=g)
    labels[:, :8] = -100
    return ids, codec, am, labels


def fwd_bwd(gm, mb, scale, seed):
    """one forward and backward with everything that could differ between two runs pinned: the jitter's RNG and the aux-weight schedule"""
    from unimoe_audio_amd import train as TR
    gm.training_steps = 0
    torch.manual_seed(seed)
    loss, _, _ = TR.forward_train(gm, *mb)
    (loss * scale).backward()
    return loss.detach()


GEMM_ROUTE = ("o_proj.weight", "codec_head.weight", "gate_proj.weight", "up_proj.weight", "down_proj.weight")


@pytest.fixture(scope="module")
def four(dev):
    """a model with main gradients and the main gradients of four micro-batches, each from zero (loss / 4), shared and left unchanged"""
    from unimoe_audio_amd import train as TR
    cfg, gm = TO.trainable(dev, seed=6)
    main = TR.attach_main_grads(gm)
    mbs = [micro_batch(cfg, 20 + i) for i in range(4)]
    each = []
    for i, mb in enumerate(mbs):
        main.zero_()
        fwd_bwd(gm, mb, 0.25, 50 + i)
        main.fold()
        each.append(main.flat.clone())
    main.zero_()
    torch.cuda.synchronize()
    return cfg, gm, main, mbs, each


def test_one_micro_batch_matches_the_plain_backward(dev):
    from unimoe_audio_amd import train as TR
    cfg, plain = TO.trainable(dev, seed=6)
    _, gm = TO.trainable(dev, seed=6)
    main = TR.attach_main_grads(gm)
    assert main.nbytes >= 4 * sum(p.numel() for p in gm.parameters()) and main is gm._main_grads
    mb = micro_batch(cfg, 20)
    l0 = fwd_bwd(plain, mb, 1.0, 50)
    l1 = fwd_bwd(gm, mb, 1.0, 50)
    assert torch.equal(l0, l1)
    routed = 0
    for (n, p), (_, q) in zip(gm.named_parameters(), plain.named_parameters()):
        if n.endswith(GEMM_ROUTE) and q.grad is not None:
            assert p.grad is None, f"{n} took the GEMM route and still got a .grad"
            routed += 1
    assert routed >= 3 + 6                                   # o_proj per layer, the head, and (gate, up, down) of the experts
    main.fold()
    torch.cuda.synchronize()
    for (n, p), (_, q) in zip(gm.named_parameters(), plain.named_parameters()):
        if q.grad is None:
            assert not p.main_grad.any(), n
        else:
            A.same_numbers_bits_where_nonzero(p.main_grad.to(bf16).cpu(), q.grad.cpu(), n)
            assert p.grad is None or not p.grad.view(torch.int16).any(), n          # folded and cleared to +0
    assert sum(int(p.grad is not None) for p in gm.parameters()) > 10


def test_four_micro_batches_accumulate_in_order(dev, four):
    """the ordering contract: accumulating four micro-batches = the fp32 sum, in order, of their four main gradients taken one at a time
    from zero, bit for bit where non-zero; within 3 * 2^-24 * sum|g_i| of the float64 sum; the bf16 `grad +=` leg's error is printed"""
    cfg, gm, main, mbs, each = four
    main.zero_()
    for i, mb in enumerate(mbs):
        fwd_bwd(gm, mb, 0.25, 50 + i)
        main.fold()
    torch.cuda.synchronize()
    got = main.flat.clone().cpu()
    main.zero_()
    host = [e.cpu() for e in each]
    want = ((host[0] + host[1]) + host[2]) + host[3]
    A.same_numbers_bits_where_nonzero(got, want, "accumulated main gradients")
    ref = sum(e.double() for e in host)
    mag = sum(e.double().abs() for e in host)
    assert bool(((got.double() - ref).abs() <= 3 * 2.0 ** -24 * mag).all()) and float(mag.max()) > 0
    # the yardstick: autograd's bf16 `grad +=` over the same four micro-batches on a model without main gradients
    _, plain = TO.trainable(dev, seed=6)
    for i, mb in enumerate(mbs):
        fwd_bwd(plain, mb, 0.25, 50 + i)
    torch.cuda.synchronize()
    num32 = num16 = den = 0.0
    for p, q in zip(gm.parameters(), plain.parameters()):
        if q.grad is None:
            continue
        o = p.main_grad.data_ptr() - main.flat.data_ptr()
        sl = slice(o // 4, o // 4 + p.numel())
        r = ref[sl]
        num32 += float(((got[sl].double() - r) ** 2).sum())
        num16 += float(((q.grad.double().cpu().reshape(-1) - r) ** 2).sum())
        den += float((r ** 2).sum())
    print(f"\nACCUMULATED GRADIENT, A = 4, relative 2-norm error against the float64 sum: fp32 main grads {np.sqrt(num32 / den):.3e}, "
          f"bf16 grad += {np.sqrt(num16 / den):.3e}")
    assert den > 0


def test_train_step_accum_trains_and_checkpoints(dev):
    from unimoe_audio_amd import train as TR
    from unimoe_audio_amd.optim import AdamW

    def run(reload_at=None):
        cfg, gm = TO.trainable(dev, seed=4)
        mk = lambda: AdamW(TR.moe_param_groups(gm, weight_decay=0.01), lr=1e-3, max_grad_norm=1.0)      # noqa: E731
        opt = mk()
        mbs = [micro_batch(cfg, 30), micro_batch(cfg, 31)]
        losses = []
        for s in range(8):
            if s == reload_at:
                sd = opt.state_dict()
                opt = mk()
                opt.load_state_dict(sd)
            torch.manual_seed(200 + s)
            loss, closs, auxm, gnorm = TR.train_step_accum(gm, opt, mbs)
            assert all(t.is_cuda and t.dim() == 0 for t in (loss, closs, auxm, gnorm))
            losses.append(loss)
        torch.cuda.synchronize()
        return gm, opt, [float(x) for x in losses]

    gm, opt, losses = run()
    print("\nACCUM LOSSES", losses)
    assert losses[-1] < losses[0] and int(opt.steps) == 8 and int(opt.skipped_steps) == 0
    main = gm._main_grads
    assert not main.flat.any()                                                        # zero_grad() zeroes the main gradients too
    assert all(p.grad is None or not p.grad.any() for p in gm.parameters())
    gm2, opt2, losses2 = run(reload_at=4)
    assert losses == losses2 and all(torch.equal(a, b) for a, b in zip(gm.parameters(), gm2.parameters()))
    # one step by hand: grad_norm against the float64 norm of the main gradients, and the version bump
    versions = [p._version for p in gm.parameters()]
    for i, mb in enumerate([micro_batch(gm.config, 30), micro_batch(gm.config, 31)]):
        fwd_bwd(gm, mb, 0.5, 300 + i)
        main.fold()
    ref = float(np.sqrt(float((main.flat.double() ** 2).sum())))
    with_grad = [bool(p.main_grad.any()) for p in gm.parameters()]
    opt.step()
    got = float(opt.grad_norm)
    print(f"GRAD NORM (main gradients) {got!r} vs fp64 {ref!r}")
    assert ref > 0 and abs(got - ref) <= R.norm_rel_bound(opt.chunk_elems) * ref and int(opt.steps) == 9
    assert all(p._version > v for p, v, w in zip(gm.parameters(), versions, with_grad) if w) and sum(with_grad) > 40
    assert all(torch.equal(p.detach(), opt.state[p]["master"].to(bf16)) for p in gm.parameters() if "master" in opt.state[p])
    opt.zero_grad(set_to_none=True)
    assert not main.flat.any() and all(p.grad is None for p in gm.parameters())


def test_detach_restores_the_plain_path(dev):
    from unimoe_audio_amd import train as TR
    from unimoe_audio_amd.optim import AdamW
    cfg, plain = TO.trainable(dev, seed=5)
    _, gm = TO.trainable(dev, seed=5)
    mb = micro_batch(cfg, 40)
    main = TR.attach_main_grads(gm)
    fwd_bwd(gm, mb, 1.0, 60)
    main.fold()
    assert bool(main.flat.any())
    main.detach()
    assert not any(hasattr(p, "main_grad") for p in gm.parameters())
    for p in gm.parameters():
        p.grad = None
    out = []
    for m in (plain, gm):
        opt = AdamW(TR.moe_param_groups(m, weight_decay=0.01), lr=1e-3, max_grad_norm=1.0)
        m.training_steps = 0
        torch.manual_seed(61)
        out.append([t.clone() for t in TR.train_step(m, opt, *mb)])
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(*out))
    assert all(torch.equal(a, b) for a, b in zip(plain.parameters(), gm.parameters()))
    assert all(p.grad is not None for n, p in gm.named_parameters() if n.endswith("o_proj.weight"))


def test_python_level_refusals(dev):
    from unimoe_audio_amd import ops
    from unimoe_audio_amd import train as TR
    from unimoe_audio_amd._lib import UmoeError
    from unimoe_audio_amd.optim import AdamW
    P = torch.nn.Parameter
    p = P(torch.zeros(8, 16, dtype=bf16, device=dev))
    opt = AdamW([p], lr=1e-3)
    for bad, msg in ((torch.zeros(8, 16, dtype=bf16, device=dev), "is fp32"), (torch.zeros(16, 8, dtype=torch.float32, device=dev), "shape"),
                     (torch.zeros(8, 32, dtype=torch.float32, device=dev)[:, ::2], "shape"), (torch.zeros(8, 16, dtype=torch.float32), "no CPU fallback")):
        p.main_grad = bad
        with pytest.raises(UmoeError, match=msg):
            opt.step()
        with pytest.raises(UmoeError):
            ops.linear_weight_grad(torch.zeros(24, 8, dtype=bf16, device=dev), torch.zeros(24, 16, dtype=bf16, device=dev), p, main_grad=bad)
    torch.cuda.synchronize()
    assert int(opt.steps) == 0 and not p.detach().any()
    p.main_grad = torch.ones(8, 16, dtype=torch.float32, device=dev)                     # and a proper one is used, .grad ignored
    opt.step()
    torch.cuda.synchronize()
    assert int(opt.steps) == 1 and bool(p.detach().any())
    cfg, gm = TO.trainable(dev, seed=5)
    gm._fp8 = dict(released=True)                                                     # what quant.release leaves on a model
    with pytest.raises(UmoeError, match="released"):
        TR.train_step_accum(gm, None, [micro_batch(cfg, 1)])
    assert not hasattr(gm, "_main_grads")
