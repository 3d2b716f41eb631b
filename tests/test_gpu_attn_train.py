"""The attention kernels of the training / prefill path against a float64 restatement, per 16 x 16 tile:
  forward   attn_prefill_kernel<GP> (umoe_attn.hip), through ops.attention(..., lse_out=...): O and the log-sum-exp;
  backward  attn_bwd_d_kernel, attn_bwd_dq_kernel<GP>, attn_bwd_dkv_kernel<4|8>, attn_bwd_dkv_sum_kernel (umoe_attn_bwd.hip),
            through _lib.AttnBwdArgs + umoe_attn_prefill_bwd the way train.RopeAttentionFn.backward calls them, on already
            rotated bf16 q / K / V (one case goes through RopeAttentionFn end to end).

Reference (_group): float64, reading exactly the bf16 values the kernels read, per (row, KV head):
    S = scale q K^T masked to kv_start <= key <= q_pos0 + t;  P = softmax(S);  O = P V;  lse = logsumexp(S)
    D = rowsum(dO o O);  dP = dO V^T;  dS = scale P o (dP - D);  dQ = dS K;  dK = sum_heads dS^T Q;  dV = sum_heads P^T dO
and beside it the ROUNDING RESTATEMENT: the same graph with the roundings the kernels document (P to bf16 before P V and P^T dO,
dS to bf16 before the dQ / dK products, O / dQ / dK / dV to bf16 at the end, D from the bf16 O).  The distance between the two is
the noise floor of a tile; it needs no GPU.

Metric: Frobenius norm per tile -- O and dQ per (row, head, 16 queries, 16 columns), dK and dV per (row, KV head, 16 keys = one
wave's keys, 16 columns):   ||got - ref64|| <= M max(||restatement - ref64||, 2^-9 ||ref64||) + ABS_FLOOR max_tiles ||ref64||
(dQ, dK: the expected effect of D's rounding is a third term of the max, see _group).
lse per element: |got - ref64| <= M_LSE 2^-23 max(1, |ref64|), and +inf exactly where a query sees no key.

Self-check: mutants of the float64 reference (_group: a dQ that lost one 64-key step, dK / dV that lost a query tile or a head
of the group, a dV d-block taken from the neighbouring key block, dS without D, O / lse that lost the first or the diagonal key
step) must each put every tile they target outside the bound around the kernel's output.  The same self-check runs on the CPU
with the restatement standing in for the kernel (test_reference_self_check_cpu), so the reference, the metric and the mutants
are tested without a GPU.

Each GPU test prints its measured worst ratios on one line ("ATTN TRAIN BOUNDS <case> {...}", shown with pytest -s).
Time on an MI355X box with 16 CPU threads: 74 s for -m gpu on this file, the seven child processes (47 s) included."""
import ctypes as C
import json
import math
import os
import subprocess
import sys
import time

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu

HD = 128
GEOM = {1: (2, 2), 2: (4, 2), 3: (6, 2), 4: (8, 2), 5: (10, 2), 8: (16, 2), 16: (16, 1)}    # G -> (H, KVH)
T_ALL = (16, 17, 63, 64, 65, 127, 128, 129, 333, 1100)
T_FEW = (17, 64, 129, 333)
# M: ||got - ref64|| of a tile in units of max(||restatement - ref64||, 2^-9 ||ref64||[, D's rounding]).  Measured on an MI355X,
# worst tile over every case and variant (the printed lines): fused kernels O 1.79, dQ 2.40, dK 1.88, dV 1.04, d qkv (end to end)
# 1.82, the training shape 1.16 / 1.46 / 1.21 / 1.01; the unfused composite (UMOE_ATTN_BWD_FUSED=0, and G = 16), which also rounds
# dP to bf16, dQ 3.80, dK 3.16.  Typical per-case worst: 1.1 - 1.7.  No tile class stands out: the worst tiles are those of one or
# two queries with two or three visible keys (kv_start = T - 2), where a handful of roundings make up the whole unit.
# M = 4 = 1.05 x the worst ratio of the composite, 1.57 x the worst of the fused kernels (the margin allowed is 2); the mutants
# move their targets by 45 - 400 units.
M = 4.0
# fp32 accumulation noise of a tile whose float64 value cancels to (near) zero (a query with one visible key has dS = 0 exactly),
# relative to the largest tile of the tensor: 128-term fp32 dot products carry ~2^-20 of their operands' magnitude.
ABS_FLOOR = 2.0 ** -16
# lse: fp32 m + __logf(l) with l summed from __expf in fp32; unit 2^-23 max(1, |lse|).  First MI355X run: worst 2.60 units
# (typically 1.0 - 1.5); M_LSE = 4 = 1.54 x that.  The mutants move lse by >= 0.04 = 3e5 units.
M_LSE = 4.0
REF_DIR_ENV = "UMOE_ATTN_TRAIN_REFDIR"       # children load the parent's float64 references from here
CHILD_ENV = "UMOE_ATTN_TRAIN_CHILD"          # set in a child: children do not spawn children


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from unimoe_audio_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ref_dir(tmp_path_factory):
    d = os.environ.get(REF_DIR_ENV)
    return d if d else str(tmp_path_factory.mktemp("attn_train_refs"))


def _record(key, rec):
    print(f"\nATTN TRAIN BOUNDS {key} {json.dumps(rec)}")


def _bf(x):
    return x.to(torch.bfloat16).double()


# ----------------------------------------------------------------------------- cases
def _pads(T):
    return sorted({p for p in (0, 1, 15, 16, 17, 63, 64, 70, T - 1, T) if 0 <= p <= T})


def make_case(G, nq, kv0, q0=None, seed=0, fill="rand"):
    """rows = len(kv0) sequences in one launch: row r has nq queries at cache slots q0[r] .. q0[r] + nq - 1 and valid keys
    [kv0[r], q0[r] + nq).  q, k ~ sigma_r N(0, 1) with sigma_r from 0.7 to 1.2 over the rows, v, dO ~ N(0, 1), all bf16.
    Cache slots behind the last query hold NaN.  fill: what the slots below kv_start and the q / dO rows of queries that see no
    key hold -- 'rand' (ordinary values), 'zero', 'big' (magnitude 1e4) or, for K and V only, 'nan'."""
    H, KVH = GEOM[G]
    rows = len(kv0)
    q0 = list(q0) if q0 is not None else [0] * rows
    Lmax = max(q0) + nq + 8
    g = torch.Generator().manual_seed(seed)
    sig = torch.linspace(0.7, 1.2, rows) if rows > 1 else torch.tensor([0.9])
    q = (torch.randn(rows, nq, H, HD, generator=g) * sig[:, None, None, None]).to(torch.bfloat16)
    K = (torch.randn(rows, KVH, Lmax, HD, generator=g) * sig[:, None, None, None]).to(torch.bfloat16)
    V = torch.randn(rows, KVH, Lmax, HD, generator=g).to(torch.bfloat16)
    dO = torch.randn(rows, nq, H, HD, generator=g).to(torch.bfloat16)
    big = lambda t: torch.where(t.float() < 0, -1e4, 1e4).to(torch.bfloat16)
    for r in range(rows):
        nblind = min(max(kv0[r] - q0[r], 0), nq)                  # queries that see no key
        for t in (K, V):
            if fill == "zero":
                t[r, :, :kv0[r]] = 0
            elif fill == "big":
                t[r, :, :kv0[r]] = big(t[r, :, :kv0[r]])
            elif fill == "nan":
                t[r, :, :kv0[r]] = float("nan")
            t[r, :, q0[r] + nq:] = float("nan")
        for t in (q, dO):
            if fill == "zero":
                t[r, :nblind] = 0
            elif fill == "big":
                t[r, :nblind] = big(t[r, :nblind])
    return dict(G=G, H=H, KVH=KVH, rows=rows, nq=nq, kv0=list(kv0), q0=q0, Lmax=Lmax, q=q, K=K, V=V, dO=dO, scale=HD ** -0.5,
                name=f"G{G}_nq{nq}_seed{seed}")


def bwd_case(G, T, fill="rand"):
    return make_case(G, T, _pads(T), None, 1000 * G + T, fill)


def training_case():
    return make_case(8, 1560, [0, 40, 0, 333], None, 77)


def fwd_qpos_case(G, nq):
    """nq queries appended behind 1, 63, 64 and 500 cached keys (q_pos0 = kv_start + cached), a different left pad per row"""
    kv0 = [0, 17, 64, 5]
    return make_case(G, nq, kv0, [k + c for k, c in zip(kv0, (1, 63, 64, 500))], 5000 + 10 * G + nq)


# ----------------------------------------------------------------------------- metric
def tiles(x):
    """Frobenius norms of the 16 x 16 tiles of the last two dimensions [n, W] -> [ceil(n / 16), W / 16]"""
    n, W = x.shape[-2], x.shape[-1]
    if n % 16:
        x = F.pad(x, (0, 0, 0, -n % 16))
    x = x.reshape(*x.shape[:-2], -1, 16, W // 16, 16)
    return x.pow(2).sum((-3, -1)).sqrt()


def tile_units(ref, rest):
    """(unit per tile, absolute floor): a tile passes when ||got - ref|| <= M unit + floor"""
    rn = tiles(ref)
    return torch.maximum(tiles(rest - ref), 2.0 ** -9 * rn), ABS_FLOOR * float(rn.max())


def lse_unit(ref):
    return 2.0 ** -23 * torch.where(torch.isinf(ref), torch.ones_like(ref), ref).abs().clamp_min(1.0)


# ----------------------------------------------------------------------------- reference, restatement, mutants
def _group(qg, K, V, dOg, kv0, q0, scale, backward=True, mutants=True):
    """One (row, KV head).  qg / dOg [G, nq, HD], K / V [Lmax, HD] (bf16 values).  Returns dicts ref / rest of float64 tensors
    (o, dq [G, nq, HD]; lse [G, nq]; dk, dv [nq, HD] over cache slots [0, nq), backward only with q0 == 0) and the mutants:
    (kind, tensor name, r0, rows, target) = the reference with its rows [r0, r0 + len) along the query / key axis replaced by
    `rows`; target: boolean mask over the tiles of those rows (lse: over their elements) that the mutant is aimed at."""
    Gn, nq, _ = qg.shape
    hi = q0 + nq
    lo = min(kv0, hi)
    n = hi - lo
    qg = qg.double()
    Kw, Vw = K[lo:hi].double(), V[lo:hi].double()
    kpos = torch.arange(lo, hi)
    qpos = q0 + torch.arange(nq)
    allowed = kpos[None, :] <= qpos[:, None]                                  # [nq, n]
    S = torch.matmul(qg, Kw.t()) * scale
    S.masked_fill_(~allowed[None], -math.inf)
    m = S.amax(-1, keepdim=True) if n else torch.full((Gn, nq, 1), -math.inf, dtype=torch.float64)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    P = torch.exp(S - m)
    del S
    l = P.sum(-1, keepdim=True)
    seen = l > 0
    P /= torch.where(seen, l, torch.ones_like(l))
    lse = torch.where(seen, m + torch.log(l.clamp_min(1e-300)), torch.full_like(l, math.inf))[..., 0]
    Pr = _bf(P)
    ref = {"o": torch.matmul(P, Vw), "lse": lse}
    rest = {"o": _bf(torch.matmul(Pr, Vw)), "lse": lse}
    muts = []
    nqt = (nq + 15) // 16

    def add(kind, name, r0, val, target=None):
        """keep the tiles the mutation changes at all (a query with one visible key has dS = 0: nothing to lose there)"""
        base = ref[name][..., r0:r0 + val.shape[-2], :] if name != "lse" else ref[name][..., r0:r0 + val.shape[-1]]
        if name == "lse":
            changed = (val != base)
        else:
            changed = tiles(val - base) > 0
        target = changed if target is None else (target & changed)
        if bool(target.any()):
            muts.append((kind, name, r0, val, target))

    if mutants and n:
        # 6. forward: a query tile without its first 64-key step / without the keys of its diagonal step, at the last query tile
        # in which EVERY query loses at least 4 % of its probability mass (a tile where one query of 16 loses 4 % moves by
        # ~1 % of its norm, which is rounding noise; all 16 of them move it by >= 4 %)
        for kind in ("fwd_first_step", "fwd_diag_step"):
            for qt in reversed(range(nqt)):
                t0, t1 = qt * 16, min(qt * 16 + 16, nq)
                if kind == "fwd_first_step":
                    a0 = lo & ~63
                    a1 = a0 + 64
                else:
                    a0 = (q0 + t1 - 1) & ~63
                    a1 = q0 + t1
                c0, c1 = max(a0, lo) - lo, min(a1, hi) - lo
                if c1 <= c0:
                    continue
                mass = P[:, t0:t1, c0:c1].sum(-1)                              # [G, <= 16]
                if not bool(((mass >= 0.04) & seen[:, t0:t1, 0]).all()):
                    continue
                rem = (1.0 - mass).clamp_min(0)
                gone = rem < 1e-12
                num = ref["o"][:, t0:t1] - torch.matmul(P[:, t0:t1, c0:c1], Vw[c0:c1])
                add(kind, "o", t0, torch.where(gone[..., None], torch.zeros_like(num), num / rem.clamp_min(1e-300)[..., None]))
                add(kind, "lse", t0, torch.where(gone, torch.full_like(rem, math.inf), lse[:, t0:t1] + torch.log(rem.clamp_min(1e-300))))
                break
    if not backward:
        return ref, rest, muts

    assert q0 == 0, "the backward runs over full sequences"
    dOg = dOg.double()
    T = nq
    nkb = (T + 15) // 16
    dP = torch.matmul(dOg, Vw.t())
    D = (dOg * ref["o"]).sum(-1, keepdim=True)
    Dr = (dOg * _bf(ref["o"])).sum(-1, keepdim=True)
    dS = scale * P * (dP - D)
    dSr = _bf(scale * P * (dP - Dr))

    def full(x):                              # [n, HD] over keys [lo, hi) -> [T, HD] over cache slots [0, T)
        return F.pad(x, (0, 0, lo, 0))

    ref["dq"] = torch.matmul(dS, Kw)
    ref["dk"] = full(torch.einsum("gtn,gtd->nd", dS, qg))
    ref["dv"] = full(torch.einsum("gtn,gtd->nd", P, dOg))
    rest["dq"] = _bf(torch.matmul(dSr, Kw))
    rest["dk"] = _bf(full(torch.einsum("gtn,gtd->nd", dSr, qg)))
    rest["dv"] = _bf(full(torch.einsum("gtn,gtd->nd", Pr, dOg)))
    del dSr, Pr
    # D is formed from a bf16 O: each O element is within 2^-9 of itself, so D carries an error of ~sigma_D = 2^-9 ||dO o O||_2
    # per query, ONE scalar that enters dS as - scale p sigma_D.  In a tile of one query with two keys that scalar is all the
    # noise there is, and a single draw of it (the restatement's) can be 25x smaller than another (the kernel's own O, which
    # differs from bf16(O64) in its last bit): measured on the first MI355X run, T = 17, kv_start = 15.  Its expected size is
    # part of the unit: element-wise rms of the error it causes in dQ and dK.
    sigD = 2.0 ** -9 * (dOg * ref["o"]).pow(2).sum(-1, keepdim=True).sqrt()
    rest["dq_D"] = scale * sigD * torch.matmul(P, Kw).abs()
    rest["dk_D"] = full(torch.einsum("gtn,gtd->nd", (scale * sigD * P).pow(2), qg.pow(2)).sqrt())
    if mutants and n:
        def kb_mask(kbs, dbs=range(8)):
            mk = torch.zeros(nkb, 8, dtype=torch.bool)
            for kb in kbs:
                for db in dbs:
                    mk[kb, db] = True
            return mk

        # the query tile of mutants 1 and 5: the last one whose 16 queries all exist and all see a key.  A row without such a tile
        # builds neither: in a tile of one query, D = dO . O can be ~0 by chance (seen: |D| < 4 sigma_D in one head of T = 65,
        # kv_start = 64), and then "dS without D" is the reference itself
        qts = [x for x in range(nqt) if x * 16 >= lo and x * 16 + 16 <= T]
        qt = qts[-1] if qts else 0
        t0, t1 = qt * 16, min(qt * 16 + 16, T)
        # 1. dQ of that query tile without one 64-key step of attn_bwd_dq_kernel (steps are aligned to 64 cache slots): the first,
        # the last (diagonal) and a middle one; a step counts when it holds >= 16 keys that every query of the tile sees (a step
        # that holds a single key of ~1000 moves the tile by less than the rounding noise), or when no step of the tile does
        steps = [(a0, min(a0 + 64, t0 + 1) - max(a0, lo)) for a0 in range(lo & ~63, t1, 64)]
        good = [a0 for a0, cnt in steps if cnt >= 16] or [a0 for a0, cnt in steps if cnt >= 1]
        for a0 in (sorted({good[0], good[len(good) // 2], good[-1]}) if good and qts else ()):
            c0, c1 = max(a0, lo) - lo, min(a0 + 64, hi) - lo
            add("dq_lost_key_step", "dq", t0, ref["dq"][:, t0:t1] - torch.matmul(dS[:, t0:t1, c0:c1], Kw[c0:c1]))
        # 5. dS of that query tile without the - D term: dQ of the tile is the target
        if qts:
            add("ds_without_D", "dq", t0, torch.matmul(scale * P[:, t0:t1] * dP[:, t0:t1], Kw))
        # 2. dK / dV without the last 16-query tile (target: the key block of those queries, which nobody else sees), and without
        # the query tile that holds the diagonal of a key block in the middle of the visible keys (target: that key block)
        tl = (T - 1) & ~15
        kmid = ((lo + T - 1) // 2) // 16
        for (s0, s1, kbs) in ((tl, T, [tl // 16]), (kmid * 16, min(kmid * 16 + 16, T), [kmid])):
            add("dkv_lost_query_tile", "dk", 0, ref["dk"] - full(torch.einsum("gtn,gtd->nd", dS[:, s0:s1], qg[:, s0:s1])), kb_mask(kbs))
            add("dkv_lost_query_tile", "dv", 0, ref["dv"] - full(torch.einsum("gtn,gtd->nd", P[:, s0:s1], dOg[:, s0:s1])), kb_mask(kbs))
        # 3. dK / dV without one head of the group, each head in turn (a head-split slab lost; added twice is the same distance):
        # every key block whose 16 keys are all visible is a target.  A row without such a block builds no mutant of this kind:
        # in a block of one or two (query, key) pairs a single head's share can be arbitrarily small (0.4 % of the tile at
        # T = 65, kv_start = 63), and a lost slab is lost for every row of the launch alike
        full_kbs = [kb for kb in range(nkb) if kb * 16 >= lo and kb * 16 + 16 <= T]
        head_target = kb_mask(full_kbs)
        for j in range(Gn if full_kbs else 0):
            add("dkv_lost_head", "dk", 0, ref["dk"] - full(torch.matmul(dS[j].t(), qg[j])), head_target)
            add("dkv_lost_head", "dv", 0, ref["dv"] - full(torch.matmul(P[j].t(), dOg[j])), head_target)
        # 4. dV: the last d-block (columns 112 - 127) of one 16-key block holds the values of the next key block
        if len(full_kbs) >= 2:
            kb = full_kbs[(len(full_kbs) - 1) // 2]
            val = ref["dv"][kb * 16:kb * 16 + 16].clone()
            val[:, 112:] = ref["dv"][kb * 16 + 16:kb * 16 + 32, 112:]
            add("dv_dblock_from_neighbour", "dv", kb * 16, val)
    return ref, rest, muts


def build_ref(case, backward=True, mutants=True, keep_rest=False):
    """Reference, tile units and mutants of a whole case.  o, dq [rows, KVH, G, nq, HD]; lse [rows, KVH, G, nq]; dk, dv
    [rows, KVH, nq, HD].  Mutants: (row, kvh, kind, tensor name, r0, rows, target)."""
    rows, KVH, G = case["rows"], case["KVH"], case["G"]
    names = ("o", "lse") + (("dq", "dk", "dv") if backward else ())
    ref = {k: [] for k in names}
    rest = {k: [] for k in names + (("dq_D", "dk_D") if backward else ())}
    muts = []
    for r in range(rows):
        for kh in range(KVH):
            qg = case["q"][r, :, kh * G:(kh + 1) * G].transpose(0, 1)
            dOg = case["dO"][r, :, kh * G:(kh + 1) * G].transpose(0, 1)
            a, b, mm = _group(qg, case["K"][r, kh], case["V"][r, kh], dOg, case["kv0"][r], case["q0"][r], case["scale"], backward, mutants)
            for k in names:
                ref[k].append(a[k])
            for k in rest:
                rest[k].append(b[k])
            muts += [(r, kh) + x for x in mm]
    shp = lambda x: torch.stack(x).reshape(rows, KVH, *x[0].shape)
    ref = {k: shp(v) for k, v in ref.items()}
    rest = {k: shp(v) for k, v in rest.items()}
    R = {"ref": ref, "unit": {}, "floor": {}, "mutants": muts}
    for k in names:
        if k != "lse":
            R["unit"][k], R["floor"][k] = tile_units(ref[k], rest[k])
            if k + "_D" in rest:
                R["unit"][k] = torch.maximum(R["unit"][k], tiles(rest[k + "_D"]))
    if keep_rest:
        R["rest"] = rest
    return R


def cached_ref(ref_dir, case, backward=True):
    """float64 references are the expensive part of this file: one per case and module, and children read the parent's"""
    path = os.path.join(ref_dir, f"{case['name']}_{'bwd' if backward else 'fwd'}.pt") if ref_dir else None
    if path and os.path.exists(path):
        return torch.load(path, weights_only=False)
    R = build_ref(case, backward)
    if path:
        torch.save(R, path + ".tmp")
        os.replace(path + ".tmp", path)
    return R


class Stats:
    def __init__(self):
        self.ratio = {}            # tensor -> worst (||got - ref|| - floor)+ / unit: the measured M
        self.where = {}
        self.selfcheck = {}        # mutant kind -> number of mutants seen

    def check(self, name, got, R, what):
        got, ref = got.double(), R["ref"][name]
        assert bool(torch.isfinite(got[torch.isfinite(ref)]).all()), f"{what} {name}: non-finite output"
        if name == "lse":
            inf = torch.isinf(ref)
            assert bool((got[inf] == math.inf).all()), f"{what}: lse of a query that sees no key is not +inf"
            r = torch.where(inf, torch.zeros_like(ref), (got - ref).abs() / lse_unit(ref))
            limit = M_LSE
        else:
            err = (tiles(got - ref) - R["floor"][name]).clamp_min(0)
            r = torch.where(err > 0, err / R["unit"][name].clamp_min(1e-300), torch.zeros_like(err))
            limit = M
        worst = float(r.max())
        if worst > self.ratio.get(name, 0.0):
            self.ratio[name] = worst
            idx, pos = int(r.argmax()), []
            for s in reversed(r.shape):
                pos.append(idx % s)
                idx //= s
            self.where[name] = f"{what} at {tuple(reversed(pos))} of {tuple(r.shape)}"
        return worst, limit

    def assert_within(self, name, got, R, what):
        worst, limit = self.check(name, got, R, what)
        assert worst <= limit, f"{what} {name}: worst at {worst:.3f} units, bound {limit} ({self.where[name]})"

    def mutants(self, got, R, what, names):
        """every mutant must put every tile it targets outside the bound around `got`"""
        for (r, kh, kind, name, r0, val, target) in R["mutants"]:
            if name not in names:
                continue
            if name == "lse":
                g = got[name][r, kh][..., r0:r0 + val.shape[-1]].double()
                d = (g - val).abs()
                d = torch.where(torch.isnan(d), torch.zeros_like(d), d)          # inf - inf: the same value
                out = d > M_LSE * lse_unit(val)
            else:
                n = val.shape[-2]
                g = got[name][r, kh][..., r0:r0 + n, :].double()
                unit = R["unit"][name][r, kh][..., r0 // 16:r0 // 16 + (n + 15) // 16, :]
                out = tiles(g - val) > M * unit + R["floor"][name]
            assert bool(out[target].all()), \
                f"self-check {what}: mutant {kind} of {name} (row {r}, kv head {kh}) stays within the bound in " \
                f"{int((~out[target]).sum())} of {int(target.sum())} targeted tiles"
            self.selfcheck[kind] = self.selfcheck.get(kind, 0) + 1

    def rec(self):
        return {"worst_units": {k: round(v, 3) for k, v in self.ratio.items()}, "where": self.where, "M": M, "M_lse": M_LSE,
                "self_check": self.selfcheck}


def split_heads(x, case):
    """[rows * nq, H * w] -> [rows, KVH, G, nq, w]"""
    return x.reshape(case["rows"], case["nq"], case["KVH"], case["G"], -1).permute(0, 2, 3, 1, 4)


# ----------------------------------------------------------------------------- the kernels
SENTINEL = -21.75           # exact in bf16; the kernels' outputs are prefilled with it


def run_fwd(dev, case, want_lse=True):
    from unimoe_audio_amd import ops
    rows, nq, H = case["rows"], case["nq"], case["H"]
    lse = torch.full((rows * nq, H), SENTINEL, dtype=torch.float32, device=dev) if want_lse else None
    out = ops.attention(case["q"].reshape(rows * nq, H * HD).to(dev), case["K"].to(dev), case["V"].to(dev),
                        torch.tensor(case["kv0"], dtype=torch.int32, device=dev), torch.tensor(case["q0"], dtype=torch.int32, device=dev),
                        nq, H, splits=1, lse_out=lse)
    return out.cpu(), (lse.cpu() if want_lse else None)


def run_bwd(dev, case, out, lse):
    """umoe_attn_prefill_bwd as train.RopeAttentionFn.backward calls it; out / lse None: the unfused composite.
    Returns dq [rows * T, H * HD], dk / dv [rows, KVH, Lmax, HD] (prefilled with SENTINEL)."""
    from unimoe_audio_amd import _lib as L, ops
    rows, T, H, KVH, Lmax = case["rows"], case["nq"], case["H"], case["KVH"], case["Lmax"]
    assert all(p == 0 for p in case["q0"])
    q = case["q"].reshape(rows * T, H * HD).to(dev)
    Kd, Vd, dOd = case["K"].to(dev), case["V"].to(dev), case["dO"].reshape(rows * T, H * HD).to(dev)
    dq = torch.full_like(q, SENTINEL)
    dk = torch.full_like(Kd, SENTINEL)
    dv = torch.full_like(Vd, SENTINEL)
    kv_host = (C.c_int32 * rows)(*case["kv0"])
    a = L.AttnBwdArgs(q=q.data_ptr(), k_cache=Kd.data_ptr(), v_cache=Vd.data_ptr(), kv_start_host=C.cast(kv_host, C.c_void_p),
                      d_out=dOd.data_ptr(), rows=rows, T=T, H=H, KVH=KVH, hd=HD, Lmax=Lmax, scale=case["scale"], dq=dq.data_ptr(),
                      dk_cache=dk.data_ptr(), dv_cache=dv.data_ptr())
    keep = []
    if out is not None:
        keep = [out.to(dev).contiguous(), lse.to(dev).contiguous()]
        a.out, a.lse = keep[0].data_ptr(), keep[1].data_ptr()
    lib = L.lib()
    nbytes = lib.umoe_attn_prefill_bwd_workspace_bytes(C.byref(a))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    a.ws, a.ws_bytes = ws.data_ptr(), nbytes
    L.check(lib.umoe_attn_prefill_bwd(C.byref(a), ops._stream()), "umoe_attn_prefill_bwd")
    torch.cuda.synchronize()
    return dq.cpu(), dk.cpu(), dv.cpu()


def ref_out_lse(case, R):
    """the forward's outputs as the float64 reference has them, rounded to the kernel's formats: [rows * T, H * HD] bf16, [rows * T, H] fp32"""
    rows, T, H = case["rows"], case["nq"], case["H"]
    o = R["ref"]["o"].permute(0, 3, 1, 2, 4).reshape(rows * T, H * HD).to(torch.bfloat16)
    lse = R["ref"]["lse"].permute(0, 3, 1, 2).reshape(rows * T, H).to(torch.float32)
    return o, lse


def check_padded_positions(case, dq, dk, dv, what):
    """pinned contract (umoe.h, umoe_attn_bwd_args): every dq row and dk / dv positions [0, T) are written; the dq rows of queries
    that see no key and the dk / dv rows below kv_start are exactly zero; slots [T, Lmax) are not touched."""
    rows, T, H = case["rows"], case["nq"], case["H"]
    dq = dq.view(rows, T, H * HD)
    for r in range(rows):
        k0 = min(case["kv0"][r], T)
        assert bool((dq[r, :k0] == 0).all()), f"{what}: dq rows of queries that see no key are not exactly zero (row {r})"
        for name, t in (("dk", dk), ("dv", dv)):
            assert bool((t[r, :, :k0] == 0).all()), f"{what}: {name} below kv_start is not exactly zero (row {r})"
            assert bool((t[r, :, T:] == SENTINEL).all()), f"{what}: {name} written at or behind slot T (row {r})"


def check_fwd(case, R, out, lse, st, what):
    got = {"o": split_heads(out, case), "lse": split_heads(lse, case)[..., 0]}
    for r in range(case["rows"]):                       # queries that see no key: zeros, exactly
        nblind = min(max(case["kv0"][r] - case["q0"][r], 0), case["nq"])
        assert bool((got["o"][r, :, :, :nblind] == 0).all()), f"{what}: output of a query that sees no key is not exactly zero"
    st.assert_within("o", got["o"], R, what)
    st.assert_within("lse", got["lse"], R, what)
    st.mutants(got, R, what, ("o", "lse"))
    return got


def check_bwd(case, R, dq, dk, dv, st, what):
    T = case["nq"]
    check_padded_positions(case, dq, dk, dv, what)
    got = {"dq": split_heads(dq, case), "dk": dk[:, :, :T], "dv": dv[:, :, :T]}
    for k in ("dq", "dk", "dv"):
        st.assert_within(k, got[k], R, what)
    st.mutants(got, R, what, ("dq", "dk", "dv"))
    return got


def fwd_bwd_case(dev, ref_dir, case, st, fused=True):
    """forward, then the backward twice: (a) on the reference's out / lse, (b) on the forward kernel's own"""
    R = cached_ref(ref_dir, case)
    what = case["name"]
    if fused:
        out, lse = run_fwd(dev, case)
        check_fwd(case, R, out, lse, st, what + " fwd")
        o_ref, l_ref = ref_out_lse(case, R)
        check_bwd(case, R, *run_bwd(dev, case, o_ref, l_ref), st, what + " bwd(a: reference out/lse)")
        check_bwd(case, R, *run_bwd(dev, case, out, lse), st, what + " bwd(b: kernel out/lse)")
    else:
        check_bwd(case, R, *run_bwd(dev, case, None, None), st, what + " bwd(unfused)")


# ----------------------------------------------------------------------------- CPU: the reference tests itself
@pytest.mark.parametrize("G,T", [(8, 333), (2, 129), (3, 65), (1, 17), (5, 64), (8, 65), (8, 17), (2, 65), (4, 16), (8, 127), (5, 17)])
def test_reference_self_check_cpu(G, T):
    """No GPU: the restatement stands in for the kernel.  It passes the bound (at one unit by construction, <= M), and every mutant
    of the reference is seen around it in every tile it targets."""
    case = bwd_case(G, T)
    R = build_ref(case, keep_rest=True)
    st = Stats()
    got = {k: R["rest"][k].to(torch.float32 if k == "lse" else torch.bfloat16) for k in R["ref"]}
    for k in ("o", "lse", "dq", "dk", "dv"):
        st.assert_within(k, got[k], R, f"cpu G={G} T={T}")
        assert st.ratio.get(k, 0.0) <= 1.0 + 1e-9
    st.mutants(got, R, f"cpu G={G} T={T}", ("o", "lse", "dq", "dk", "dv"))
    kinds = {"dq_lost_key_step", "ds_without_D", "dkv_lost_query_tile", "dkv_lost_head", "fwd_first_step", "fwd_diag_step"}
    if T >= 64:
        kinds.add("dv_dblock_from_neighbour")
    assert kinds <= set(st.selfcheck), f"mutant kinds not exercised: {kinds - set(st.selfcheck)}"


def test_reference_matches_autograd_cpu():
    """the hand-written float64 backward is the gradient of the float64 forward (torch autograd on the same graph)"""
    case = make_case(3, 40, [0, 5, 39, 40], None, 9)
    R = build_ref(case, mutants=False)
    G, T = case["G"], case["nq"]
    for r in range(case["rows"]):
        for kh in range(case["KVH"]):
            q = case["q"][r, :, kh * G:(kh + 1) * G].transpose(0, 1).double().requires_grad_(True)
            K = case["K"][r, kh, :T].double().requires_grad_(True)
            V = case["V"][r, kh, :T].double().requires_grad_(True)
            dO = case["dO"][r, :, kh * G:(kh + 1) * G].transpose(0, 1).double()
            ok = (torch.arange(T)[None, :] <= torch.arange(T)[:, None]) & (torch.arange(T)[None, :] >= case["kv0"][r])
            s = (q @ K.t() * case["scale"]).masked_fill(~ok, -math.inf)
            p = torch.nan_to_num(torch.softmax(s, -1), nan=0.0)
            o = p @ V
            (o * dO).sum().backward()
            for name, g in (("o", o.detach()), ("dq", q.grad), ("dk", K.grad), ("dv", V.grad)):
                assert torch.allclose(R["ref"][name][r, kh], g, rtol=1e-9, atol=1e-11), (name, r, kh)


# ----------------------------------------------------------------------------- GPU: forward + backward per tile
@gpu
@pytest.mark.parametrize("G,T", [(g, t) for g in (8, 2) for t in T_ALL] + [(g, t) for g in (1, 3, 4, 5) for t in T_FEW])
def test_attn_fwd_bwd_tiles_vs_fp64(dev, ref_dir, G, T):
    """rows with left pads 0, 1, 15, 16, 17, 63, 64, 70, T - 1 and T (a row that sees nothing) in one launch"""
    st = Stats()
    fwd_bwd_case(dev, ref_dir, bwd_case(G, T), st)
    assert all(v > 0 for v in st.selfcheck.values()) and len(st.selfcheck) >= 5
    _record(f"fwd_bwd_G{G}_T{T}", st.rec())


@gpu
def test_attn_bwd_training_shape_vs_fp64(dev, ref_dir):
    """the shape a training step runs: 4 rows x 1560 tokens, 16 heads on 2 KV heads, left pads 0, 40, 0, 333"""
    st = Stats()
    fwd_bwd_case(dev, ref_dir, training_case(), st)
    _record("fwd_bwd_training_shape", st.rec())


@gpu
def test_attn_bwd_unfused_g16_vs_fp64(dev, ref_dir):
    """16 query heads per KV head: outside the fused kernels (G <= 8); umoe_attn_prefill_bwd runs the composite on the tiled GEMM"""
    st = Stats()
    fwd_bwd_case(dev, ref_dir, make_case(16, 45, [0, 1, 17, 44, 45], None, 1600), st, fused=False)
    _record("bwd_unfused_G16_T45", st.rec())


@gpu
@pytest.mark.parametrize("G,nq", [(2, 16), (4, 17), (8, 64), (8, 100), (2, 100), (4, 64)])
def test_attn_fwd_qpos_vs_fp64(dev, ref_dir, G, nq):
    """the MFMA prefill kernel with q_pos0 > 0: nq queries behind 1, 63, 64, 500 cached keys; NaN behind the last visible key"""
    case = fwd_qpos_case(G, nq)
    R = cached_ref(ref_dir, case, backward=False)
    st = Stats()
    out, lse = run_fwd(dev, case)
    check_fwd(case, R, out, lse, st, case["name"])
    assert st.selfcheck.get("fwd_first_step", 0) > 0 and st.selfcheck.get("fwd_diag_step", 0) > 0
    _record(f"fwd_qpos_G{G}_nq{nq}", st.rec())


# ----------------------------------------------------------------------------- GPU: exact properties
def _bits(x):
    return x.contiguous().view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32)


def _visible_equal(case, a, b, what):
    """out / lse / dq rows of queries that see a key, dk / dv rows in [kv_start, T): the same bits"""
    rows, T = case["rows"], case["nq"]
    for name in a:
        x, y = a[name], b[name]
        for r in range(rows):
            k0 = min(case["kv0"][r], T)
            if name in ("dk", "dv"):
                xs, ys = x[r, :, k0:T], y[r, :, k0:T]
            else:
                xs, ys = x.view(rows, T, -1)[r, k0:], y.view(rows, T, -1)[r, k0:]
            assert torch.equal(_bits(xs), _bits(ys)), f"{what}: {name} of row {r} depends on what the masked slots hold"


def _all_outputs(dev, case):
    out, lse = run_fwd(dev, case)
    dq, dk, dv = run_bwd(dev, case, out, lse)
    return {"o": out, "lse": lse, "dq": dq, "dk": dk, "dv": dv}


@gpu
@pytest.mark.parametrize("G,T", [(8, 129), (2, 333), (4, 65), (8, 333)])
def test_attn_masked_slots_do_not_matter(dev, G, T):
    """O, lse, dQ, dK, dV at visible positions are bit-identical whether the cache slots below kv_start and the q / dO rows of
    padded queries hold ordinary values, zeros or values of magnitude 1e4."""
    base = _all_outputs(dev, bwd_case(G, T, fill="rand"))
    for fill in ("zero", "big"):
        case = bwd_case(G, T, fill=fill)
        other = _all_outputs(dev, case)
        _visible_equal(case, base, other, f"G={G} T={T} fill={fill}")
        check_padded_positions(case, other["dq"], other["dk"], other["dv"], f"G={G} T={T} fill={fill}")


@gpu
def test_attn_nan_below_kv_start_precondition(dev):
    """umoe.h states the precondition: K and V slots in [0, T) below kv_start must hold FINITE values (the MFMA kernels stage the
    64-key step that holds kv_start whole and give its masked keys a zero probability: 0 x NaN in the matrix core is NaN).  What
    holds without it and is pinned here: a row whose kv_start is a multiple of 64 never reads a slot below it.  And the caller of
    the training path keeps the precondition: umoe_qkv_mrope_kvappend, as RopeAttentionFn.forward calls it, writes every slot in
    [0, T) of a cache that held NaN with finite values (the engine's prefill makes the same call for all T positions)."""
    from unimoe_audio_amd import ops
    G, T = 8, 200
    kv0 = [0, 64, 128]
    ref = _all_outputs(dev, make_case(G, T, kv0, None, 31, fill="rand"))
    case = make_case(G, T, kv0, None, 31, fill="nan")
    got = _all_outputs(dev, case)
    _visible_equal(case, ref, got, "NaN below a kv_start that is a multiple of 64")
    H, KVH = GEOM[G]
    B = 2
    g = torch.Generator().manual_seed(32)
    qkv = torch.randn(B * T, (H + 2 * KVH) * HD, generator=g).to(torch.bfloat16).to(dev)
    am = torch.ones(B, T, dtype=torch.long)
    am[0, :70] = 0
    pos = (am.cumsum(-1) - 1).masked_fill(am == 0, 1)
    cos, sin = ops.rope_tables(int(pos.max()) + 2, HD, 1e6, dev)
    pos3 = pos[None].expand(3, -1, -1).reshape(3, B * T).to(torch.int32).contiguous().to(dev)
    kv_pos = torch.arange(T, dtype=torch.int32, device=dev).repeat(B)
    kc = torch.full((B, KVH, T, HD), float("nan"), dtype=torch.bfloat16, device=dev)
    vc = torch.full_like(kc, float("nan"))
    ops.qkv_mrope_kvappend(qkv, cos, sin, pos3, kv_pos, T, H, KVH, HD, (16, 24, 24), kc, vc)
    assert bool(torch.isfinite(kc).all()) and bool(torch.isfinite(vc).all())


def _bwd_bits(dev, case):
    out, lse = run_fwd(dev, case)
    return torch.cat([_bits(t).flatten().to(torch.int32) for t in run_bwd(dev, case, out, lse)])


@gpu
def test_attn_bwd_deterministic(dev, tmp_path):
    """one writer and a fixed summation order per element: two backward calls give the same bits, with the dQ pass on the side
    stream (default) -- and the same bits again in a child process with UMOE_BWD_OVERLAP=0."""
    cases = [bwd_case(8, 333), bwd_case(2, 129), bwd_case(4, 333)]
    first = [_bwd_bits(dev, c) for c in cases]
    for c, f in zip(cases, first):
        assert torch.equal(f, _bwd_bits(dev, c)), c["name"]
    given = os.environ.get("UMOE_ATTN_TRAIN_DET_FILE")
    if given:                                    # the child: compare with the parent's (default) bits
        want = torch.load(given, weights_only=False)
        for c, f, w in zip(cases, first, want):
            assert torch.equal(f, w), f"{c['name']}: UMOE_BWD_OVERLAP={os.environ.get('UMOE_BWD_OVERLAP')} differs from the default"
        return
    if os.environ.get(CHILD_ENV):
        return
    path = str(tmp_path / "bwd_default_bits.pt")
    torch.save(first, path)
    _child({"UMOE_BWD_OVERLAP": "0", "UMOE_ATTN_TRAIN_DET_FILE": path}, "test_attn_bwd_deterministic", None, 12)     # 4 s measured


# ----------------------------------------------------------------------------- GPU: the variants the library reads once
def _child(env_extra, k_expr, ref_dir, limit):
    """one pytest child on this file with the given switches.  A child that fails, dies of a signal or runs into its time limit
    fails the caller with its output and is not run again."""
    env = dict(os.environ, **env_extra)
    env[CHILD_ENV] = "1"
    if ref_dir:
        env[REF_DIR_ENV] = ref_dir
    t = time.time()
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-s", "-m", "gpu", "-k", k_expr,
                            "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"child {env_extra} ran into its time limit of {limit} s:\n{str(e.stdout)[-3000:]}")
    assert r.returncode == 0, f"child {env_extra} returned {r.returncode} after {time.time() - t:.0f} s:\n" + r.stdout[-4000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "no tests ran" not in r.stdout, r.stdout[-500:]
    print(f"\nATTN TRAIN CHILD {json.dumps(env_extra)} {time.time() - t:.0f} s: {r.stdout.strip().splitlines()[-1]}")
    for line in r.stdout.splitlines():
        if line.startswith("ATTN TRAIN BOUNDS"):
            print("  " + line)


# (switches, -k expression, time limit in seconds = 3 x the time measured on an MI355X box: 11 s for the backward subset with the
# parent's references on disk, 4 s for the small subsets, interpreter start included)
BWD_SUBSET = "fwd_bwd_tiles or training_shape"
VARIANTS = [
    ({"UMOE_ATTN_BWD_KEYWAVES": "4"}, BWD_SUBSET, 33),
    ({"UMOE_ATTN_BWD_SPLIT": "1"}, BWD_SUBSET, 33),
    ({"UMOE_ATTN_BWD_SPLIT": "2"}, BWD_SUBSET, 33),
    ({"UMOE_BWD_OVERLAP": "0"}, BWD_SUBSET, 33),
    ({"UMOE_ATTN_BWD_FUSED": "0"}, "variant_small", 12),
    ({"UMOE_ATTN_PREFILL_MFMA": "0"}, "fwd_only_small", 12),
]


@gpu
@pytest.mark.parametrize("G,T", [(8, 129), (2, 65), (3, 64), (4, 17), (5, 129), (1, 64)])
def test_attn_bwd_variant_small(dev, ref_dir, G, T):
    """small T, for the unfused composite (it materialises the scores): the backward on the reference's out / lse.  In the parent
    process this is the fused path once more; under UMOE_ATTN_BWD_FUSED=0 the same call runs the composite."""
    case = bwd_case(G, T)
    R = cached_ref(ref_dir, case)
    st = Stats()
    check_bwd(case, R, *run_bwd(dev, case, *ref_out_lse(case, R)), st, case["name"] + f" FUSED={os.environ.get('UMOE_ATTN_BWD_FUSED', '1')}")
    _record(f"bwd_variant_small_G{G}_T{T}", st.rec())


@gpu
@pytest.mark.parametrize("G,T", [(8, 129), (2, 333), (4, 65)])
def test_attn_fwd_only_small(dev, ref_dir, G, T):
    """the forward alone (O; the split-key kernel writes no lse): under UMOE_ATTN_PREFILL_MFMA=0 it is the split-key kernel's turn"""
    case = bwd_case(G, T)
    R = cached_ref(ref_dir, case)
    st = Stats()
    out, _ = run_fwd(dev, case, want_lse=False)
    got = {"o": split_heads(out, case)}
    st.assert_within("o", got["o"], R, case["name"])
    st.mutants(got, R, case["name"], ("o",))
    _record(f"fwd_only_G{G}_T{T}", st.rec())


@gpu
def test_attn_variants_in_child_processes(dev, ref_dir):
    """UMOE_ATTN_BWD_KEYWAVES=4 (64-key dK / dV tiles at T > 64), UMOE_ATTN_BWD_SPLIT=1 / 2 (head split), UMOE_BWD_OVERLAP=0,
    UMOE_ATTN_BWD_FUSED=0 (the composite above T = 9) and UMOE_ATTN_PREFILL_MFMA=0: the library reads each once, so each runs
    its subset of this file in a child process of its own, one at a time; the first child that does not return 0 ends the test
    and nothing is started after it."""
    if os.environ.get(CHILD_ENV):
        return
    for env_extra, k_expr, limit in VARIANTS:
        _child(env_extra, k_expr, ref_dir, limit)


# ----------------------------------------------------------------------------- GPU: end to end through RopeAttentionFn
def _rot_half(x):
    return torch.cat([-x[..., HD // 2:], x[..., :HD // 2]], -1)


class _RoundBf16(torch.autograd.Function):
    """bf16 rounding of a value on the way forward and of its gradient on the way back (the restatement's rounding points)"""
    @staticmethod
    def forward(ctx, x, fwd, bwd):
        ctx.bwd = bwd
        return _bf(x) if fwd else x.clone()

    @staticmethod
    def backward(ctx, g):
        return (_bf(g) if ctx.bwd else g), None, None


def _e2e_graph(x, cos, sin, dO, kv0, B, T, H, KVH, rounded):
    """float64 autograd: qkv -> mRoPE (bf16 tables) -> causal GQA attention -> sum(O o dO); returns (O, d qkv).  rounded: with
    the kernels' rounding points (rotated q / k, P, O to bf16; dS, dq / dk / dv, d qkv to bf16)."""
    rb = (lambda t, f=True, b=True: _RoundBf16.apply(t, f, b)) if rounded else (lambda t, f=True, b=True: t)
    G = H // KVH
    x = x.clone().requires_grad_(True)
    xo = rb(x, False, True)                                    # d qkv rounded once at the end
    q = xo[:, :H * HD].view(B, T, H, HD)
    k = xo[:, H * HD:(H + KVH) * HD].view(B, T, KVH, HD)
    v = xo[:, (H + KVH) * HD:].view(B, T, KVH, HD)
    c, s = cos.view(B, T, 1, HD), sin.view(B, T, 1, HD)
    qr = rb(q * c + _rot_half(q) * s)
    kr = rb(k * c + _rot_half(k) * s)
    vr = rb(v, False, True)
    outs = []
    for b in range(B):
        ok = (torch.arange(T)[None, :] <= torch.arange(T)[:, None]) & (torch.arange(T)[None, :] >= kv0[b])
        for kh in range(KVH):
            qg = qr[b, :, kh * G:(kh + 1) * G].transpose(0, 1)                       # [G, T, HD]
            sraw = rb(qg @ kr[b, :, kh].t(), False, True)                            # d(raw scores) = dS: bf16
            p = torch.nan_to_num(torch.softmax((sraw * HD ** -0.5).masked_fill(~ok, -math.inf), -1), nan=0.0)
            outs.append(rb(rb(p, True, False) @ vr[b, :, kh], True, False))
    o = torch.stack(outs).view(B, KVH, G, T, HD).permute(0, 3, 1, 2, 4).reshape(B * T, H * HD)
    (o * dO).sum().backward()
    return o.detach(), x.grad


@gpu
def test_rope_attention_fn_end_to_end_tiles_vs_fp64(dev):
    """train.RopeAttentionFn forward + backward (umoe_qkv_mrope_kvappend, the attention kernels, umoe_qkv_mrope_bwd) with the
    per-tile metric on the output and on d qkv (16 tokens x 16 columns: every head's d-blocks of dQ | dK | dV)."""
    from oracle import decode as OD
    from unimoe_audio_amd import ops, train as TR
    B, T, H, KVH = 2, 333, 16, 2
    sections = [16, 24, 24]
    g = torch.Generator().manual_seed(4242)
    qkv = (torch.randn(B * T, (H + 2 * KVH) * HD, generator=g) * 0.9).to(torch.bfloat16)
    am = torch.ones(B, T, dtype=torch.long)
    am[0, :70] = 0
    valid = am.bool().reshape(-1)
    dO = torch.randn(B * T, H * HD, generator=g).to(torch.bfloat16) * valid[:, None]
    pos = (am.cumsum(-1) - 1).masked_fill(am == 0, 1)
    cos3, sin3 = OD.rope_cos_sin(pos[None].expand(3, -1, -1), HD, 1e6, torch.bfloat16)
    cos = OD.mrope_select(cos3, sections).reshape(B * T, HD).double()
    sin = OD.mrope_select(sin3, sections).reshape(B * T, HD).double()
    kv0 = [70, 0]
    o64, g64 = _e2e_graph(qkv.double(), cos, sin, dO.double(), kv0, B, T, H, KVH, False)
    o_r, g_r = _e2e_graph(qkv.double(), cos, sin, dO.double(), kv0, B, T, H, KVH, True)
    xg = qkv.to(dev).requires_grad_(True)
    cosd, sind = ops.rope_tables(int(pos.max()) + 2, HD, 1e6, dev)
    pos3 = pos[None].expand(3, -1, -1).reshape(3, B * T).to(torch.int32).contiguous().to(dev)
    kv_pos = torch.arange(T, dtype=torch.int32, device=dev).repeat(B)
    fv = torch.tensor(kv0, dtype=torch.int32)
    ao = TR.RopeAttentionFn.apply(xg, cosd, sind, pos3, kv_pos, fv.to(dev), fv.tolist(), B, T, H, KVH, HD, tuple(sections))
    (ao.float() * dO.to(dev).float()).sum().backward()
    R = {"ref": {"o": o64.view(B, T, -1), "dqkv": g64.view(B, T, -1)}, "unit": {}, "floor": {}}
    R["unit"]["o"], R["floor"]["o"] = tile_units(R["ref"]["o"], o_r.view(B, T, -1))
    R["unit"]["dqkv"], R["floor"]["dqkv"] = tile_units(R["ref"]["dqkv"], _bf(g_r).view(B, T, -1))
    st = Stats()
    st.assert_within("o", ao.detach().cpu().view(B, T, -1), R, "e2e")
    st.assert_within("dqkv", xg.grad.cpu().view(B, T, -1), R, "e2e")
    _record("rope_attention_fn_e2e", st.rec())
