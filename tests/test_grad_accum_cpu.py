"""Gradient accumulation in fp32 main gradients, the part that needs no GPU -- and the checkers tests/test_gpu_grad_accum.py
runs on the kernels' outputs.

The accumulate orders restated on the host in fp32 (umoe_tiled_gemm_tn_acc with and without a K split, umoe_optim_fold) pass these
checkers, and each planted error is rejected by the checker that is meant to see it:

    prior value added before the partials instead of after      the repeated-call check (bit for bit against fp32(s + s))
    a K-split part dropped                                        the per-element float64 interval
    bf16 rounding before the add                                  the per-element float64 interval
    an empty ragged group zeroing its output                      the untouched-bytes check
    the fold not clearing g                                       the fold check

The float64 interval: out_after inside prev + sum +- (e_sum + 2^-24 (|prev| + |sum| + e_sum)), e_sum = K_eff u sum|p q| being
test_gpu_gemm_fp64's derived bound of the fp32 sum before its bf16 term (K_eff = K + k_split), and the one fp32 add of the accumulate
store contributing half an ulp of a result no larger than |prev| + |sum| + e_sum.

Also here: the record layouts against a compiled probe of umoe.h, the flag word's two bits, attach_main_grads' offsets, and the compiled
kernels' scratch / spill counts.
"""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import optim_ref as R
import test_gpu_gemm_fp64 as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
f64 = torch.float64
NAN_BITS = 0x7FC12345           # a quiet NaN with a payload: "untouched" means these very bits

# three ragged groups, the middle one empty (an expert no token reached); an entry of its own beside test_gpu_gemm_fp64's table
G.TN_SPEC.setdefault("tn_acc_ragged3", dict(name="tn_acc_ragged3", ldo=264, groups=[G.T(264, 260, 33, dev=True), G.T(256, 252, 0, dev=True),
                                                                                   G.T(12, 4, 129, oc=4, dev=True)]))
CASES = [s["name"] for s in G.TN] + ["tn_acc_ragged3"]


def splits_of(c):
    return c["spec"].get("splits", (1,))


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def int_case(name):
    """the case `name` with small-integer operands in the same places: every product and every sum is exact in fp32"""
    c = G.tn_case(name)
    key = "int_" + name
    if key in _INT:
        return _INT[key]
    P, Q = c["P"].clone(), c["Q"].clone()
    groups = []
    for d in c["groups"]:
        e = dict(d)
        k, m, n = d["k"], d["m"], d["n"]
        scale = max(k, 1) ** -0.25
        e["p"] = torch.round(d["p"].float() / scale).clamp(-3, 3).to(G.bf16)
        e["q"] = torch.round(d["q"].float() / scale).clamp(-3, 3).to(G.bf16)
        if d["own"]:
            e["pbuf"], e["qbuf"] = d["pbuf"].clone(), d["qbuf"].clone()
            e["pbuf"][5:5 + k, d["pco"]:d["pco"] + m] = e["p"]
            e["qbuf"][5:5 + k, d["qco"]:d["qco"] + n] = e["q"]
        else:
            P[d["k_off"]:d["k_off"] + k, d["pco"]:d["pco"] + m] = e["p"]
            Q[d["k_off"]:d["k_off"] + k, d["qco"]:d["qco"] + n] = e["q"]
        groups.append(e)
    _INT[key] = dict(spec=c["spec"], name=key, P=P, Q=Q, groups=groups, RO=c["RO"], ldo=c["ldo"])
    return _INT[key]


_INT = {}


def windows(c):
    """(group index, None or the index of its own output, row slice, column slice)"""
    return [(i, i if d["own"] else None, slice(d["out_row_base"], d["out_row_base"] + d["m"]), slice(d["oc"], d["oc"] + d["n"]))
            for i, d in enumerate(c["groups"])]


def make_prev(c, kind, seed=0):
    """the fp32 outputs before the call: NaN everywhere outside the groups' windows; inside "rand" (normal), "zero", "int" (integers) or
    "nan" (the payload pattern).  -> (launch output [RO][ldo], {group: output of its own})"""
    g = torch.Generator().manual_seed(1000 + seed)

    def fill(t, rs, cs):
        shape = t[rs, cs].shape
        if kind == "rand":
            t[rs, cs] = torch.randn(shape, generator=g)
        elif kind == "zero":
            t[rs, cs] = 0.0
        elif kind == "int":
            t[rs, cs] = torch.randint(-1000, 1001, shape, generator=g).float()
        else:
            t[rs, cs] = torch.full(shape, NAN_BITS, dtype=torch.int32).view(torch.float32)

    out = torch.full((c["RO"], c["ldo"]), float("nan"), dtype=torch.float32)
    own = {}
    for i, o, rs, cs in windows(c):
        if o is not None:
            own[i] = torch.full((c["groups"][i]["RO"], c["ldo"]), float("nan"), dtype=torch.float32)
        fill(out if o is None else own[i], rs, cs)
    return out, own


def emu_acc_tn(c, ks, prev, plant=None, pg=None):
    """umoe_tiled_gemm_tn_acc restated in fp32 on the host: s = part 0 + part 1 + ... (each part test_gpu_gemm_fp64's emu_acc over its K
    window), then out = prev + s; an empty DEVICE window stores nothing.  plant: "prev_first", "part", "bf16", "empty_zero" on group pg."""
    out, own = prev[0].clone(), {i: t.clone() for i, t in prev[1].items()}
    for i, o, rs, cs in windows(c):
        d = c["groups"][i]
        tgt = out if o is None else own[i]
        hit = plant is not None and i == pg
        if d["dev"] and d["k"] == 0:
            if hit and plant == "empty_zero":
                tgt[rs, cs] = 0.0
            continue
        parts = [G.emu_acc(d["p"][lo:hi].t(), d["q"][lo:hi].t()) for lo, hi in G.tn_parts(d["k"], ks)]
        if hit and plant == "part":
            parts = parts[1:]
        if hit and plant == "prev_first":
            acc = tgt[rs, cs].clone()
            for p in parts:
                acc = acc + p
            tgt[rs, cs] = acc
            continue
        s = parts[0]
        for p in parts[1:]:
            s = s + p
        if hit and plant == "bf16":
            s = s.to(G.bf16).float()
        tgt[rs, cs] = tgt[rs, cs] + s
    return out, own


def pick(pair, o):
    return pair[0] if o is None else pair[1][o]


# ------------------------------------------------------------------------------------------------ the checkers
def check_outside(c, prev, got):
    """nothing outside the groups' windows changed a bit (rows at or beyond m, columns at or beyond n hold NaN), and an empty device
    window kept its bytes"""
    masks = {None: torch.zeros(prev[0].shape, dtype=torch.bool), **{i: torch.zeros(t.shape, dtype=torch.bool) for i, t in prev[1].items()}}
    for i, o, rs, cs in windows(c):
        d = c["groups"][i]
        if not (d["dev"] and d["k"] == 0):
            masks[o][rs, cs] = True
    for o, m in masks.items():
        a, b = bits(pick(prev, o)), bits(pick(got, o))
        assert torch.equal(a[~m], b[~m]), f"{c['name']}: output {o}: bytes outside the windows (or of an empty device window) changed"


def check_fp64(c, ks, prev, got, stats):
    """per element: out_after inside prev + sum +- (e_sum + u (|prev| + |sum| + e_sum)); float64 reference of test_gpu_gemm_fp64"""
    ref = G.tn_ref(c)
    for i, o, rs, cs in windows(c):
        d, r = c["groups"][i], ref[i]
        if d["dev"] and d["k"] == 0:
            continue                                         # (check_outside: the bytes themselves)
        k_eff = d["k"] + (ks if ks > 1 else 0)
        e_sum = k_eff * U * r["ab"]
        pv = pick(prev, o)[rs, cs].to(f64)
        bound = e_sum + U * (pv.abs() + r["acc"].abs() + e_sum)
        G.check(f"k={d['k']}" if len(c["groups"]) > 1 else "acc", pick(got, o)[rs, cs], pv + r["acc"], bound, stats)


def check_exact(c, prev, got):
    """small-integer operands and integer prior values: equal with no tolerance"""
    for i, o, rs, cs in windows(c):
        d = c["groups"][i]
        want = pick(prev, o)[rs, cs].to(f64) + d["p"].to(f64).t() @ d["q"].to(f64)
        assert torch.equal(pick(got, o)[rs, cs].to(f64), want), f"{c['name']}: group {i} (k={d['k']}): integer sums are not exact"


def same_numbers_bits_where_nonzero(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape
    assert bool((a == b).all()), f"{what}: values differ"
    nz = a != 0
    ib = torch.int32 if a.dtype == torch.float32 else torch.int16
    assert torch.equal(a.contiguous().view(ib)[nz], b.contiguous().view(ib)[nz]), f"{what}: bits differ"


def check_from_zero(c, got, plain):
    """from a zeroed output: bf16_rne(out) = the bf16 entry's output as numbers, bit for bit where non-zero (a sum of -0 may come back +0)"""
    for i, o, rs, cs in windows(c):
        same_numbers_bits_where_nonzero(pick(got, o)[rs, cs].to(G.bf16), pick(plain, o)[rs, cs].cpu(), f"{c['name']}: group {i}")


def check_repeat(c, once, twice):
    """two calls in a row from zero = fp32(fp32(0 + s) + s), computed on the host from the first call's s, bit for bit"""
    for i, o, rs, cs in windows(c):
        s = pick(once, o)[rs, cs]
        assert torch.equal(bits(pick(twice, o)[rs, cs]), bits(s + s)), f"{c['name']}: group {i}: second call is not fp32(s + s)"


def emu_fold(main, g, clear=True):
    """umoe_optim_fold on host arrays: (main + float(g), g')"""
    return main + g.float(), (torch.zeros_like(g) if clear else g.clone())


def check_fold(main0, g0, main1, g1):
    assert torch.equal(bits(main1), bits(main0 + g0.float())), "fold: main is not main + float(g) bit for bit"
    assert not g1.contiguous().view(torch.int16).any(), "fold: g was not cleared to +0"


# ------------------------------------------------------------------------------------------------ the emulation passes, plants do not
def test_emulated_accumulate_orders_pass_the_checkers():
    st = G.Stats()
    st.prefix = "GRAD ACCUM"
    for name in CASES:
        c = G.tn_case(name)
        for ks in splits_of(c):
            ks = 2 if ks < 0 else ks
            prev = make_prev(c, "rand", 1)
            got = emu_acc_tn(c, ks, prev)
            check_outside(c, prev, got)
            check_fp64(c, ks, prev, got, st)
            zero = make_prev(c, "zero")
            once = emu_acc_tn(c, ks, zero)
            plain = G.emu_tn(c, ks)
            check_from_zero(c, once, plain)
            check_repeat(c, once, emu_acc_tn(c, ks, once))
            ci = int_case(name)
            pi = make_prev(ci, "int", 2)
            check_exact(ci, pi, emu_acc_tn(ci, ks, pi))
    st.show("emulated accumulate")
    assert max(st.values()) <= 1.0
    c = G.tn_case("tn_acc_ragged3")
    prev = make_prev(c, "nan")
    got = emu_acc_tn(c, 1, prev)
    check_outside(c, prev, got)
    assert torch.equal(bits(got[0])[c["groups"][1]["out_row_base"], :4], torch.full((4,), NAN_BITS, dtype=torch.int32))


def _rejects(fn):
    with pytest.raises(AssertionError):
        fn()


def test_planted_errors_are_rejected():
    c = G.tn_case("tn_split")
    for ks in (2, 3, 4):
        # the prior value added before the partials: as accurate as the right order, so only the bit-for-bit check of a second call sees it
        zero = make_prev(c, "zero")
        once = emu_acc_tn(c, ks, zero)
        for pg in (0, 2):
            bad = emu_acc_tn(c, ks, once, "prev_first", pg)
            _rejects(lambda: check_repeat(c, once, bad))
            prev = make_prev(c, "rand", 3)
            _rejects(lambda: check_fp64(c, ks, prev, emu_acc_tn(c, ks, prev, "part", pg), G.Stats()))
    for name, ks, pg in (("tn_static", 1, 8), ("tn_static", 1, 5), ("tn_split", 2, 0), ("tn_auto", 2, 0)):
        c = G.tn_case(name)
        prev = make_prev(c, "rand", 4)
        _rejects(lambda: check_fp64(c, ks, prev, emu_acc_tn(c, ks, prev, "bf16", pg), G.Stats()))
    ci = int_case("tn_auto")                      # the exact check sees a part left out (bf16 holds most of these small integer sums)
    pi = make_prev(ci, "int", 5)
    _rejects(lambda: check_exact(ci, pi, emu_acc_tn(ci, 2, pi, "part", 0)))
    for name, pg in (("tn_acc_ragged3", 1), ("tn_device", 1), ("tn_device_empty", 0)):
        c = G.tn_case(name)
        for kind in ("rand", "nan"):
            prev = make_prev(c, kind, 6)
            _rejects(lambda: check_outside(c, prev, emu_acc_tn(c, 1, prev, "empty_zero", pg)))
    # bf16_rne of the accumulate output against the bf16 entry: a value one bf16 ulp off is seen
    c = G.tn_case("tn_static")
    once = emu_acc_tn(c, 1, make_prev(c, "zero"))
    plain = G.emu_tn(c, 1)
    bad = plain[0].clone()
    r0 = c["groups"][8]["out_row_base"]
    bad[r0, 8] = float(bad[r0, 8]) * (1 + 2.0 ** -7)
    _rejects(lambda: check_from_zero(c, once, (bad, plain[1])))


def test_fold_emulation_and_the_fold_that_does_not_clear():
    g = torch.Generator().manual_seed(9)
    main0 = torch.randn(1000, generator=g)
    g0 = (torch.randn(1000, generator=g) * 1e-3).to(torch.bfloat16)
    check_fold(main0, g0, *emu_fold(main0, g0))
    _rejects(lambda: check_fold(main0, g0, *emu_fold(main0, g0, clear=False)))
    _rejects(lambda: check_fold(main0, g0, main0 + g0.float() * (1 + 2.0 ** -20), torch.zeros_like(g0)))
    neg0 = torch.full((4,), -0.0, dtype=torch.bfloat16)           # cleared means +0, not -0
    _rejects(lambda: check_fold(main0[:4], g0[:4], main0[:4] + g0[:4].float(), neg0))
    # four accumulations of contributions 2^-9 of the running sum: fp32 keeps them, bf16 `grad +=` loses every one
    big, small = torch.tensor([1.0]), torch.tensor([2.0 ** -9])
    m32, m16 = big.clone(), big.to(torch.bfloat16)
    for _ in range(4):
        m32, _ = emu_fold(m32, small.to(torch.bfloat16))
        m16 = m16 + small.to(torch.bfloat16)
    assert float(m32) == 1.0 + 4 * 2.0 ** -9 and float(m16) == 1.0


# ------------------------------------------------------------------------------------------------ layouts, flags, offsets
def test_record_layouts_and_flag_bits_are_the_headers(tmp_path):
    from unimoe_audio_amd import _lib as L
    from unimoe_audio_amd import optim as O
    recs = {"umoe_optim_tensor": (O.TENSOR_DTYPE, ["p", "g", "master", "m", "v", "n", "group", "p_fp32"]),
            "umoe_optim_chunk": (O.CHUNK_DTYPE, ["tensor", "first"]),
            "umoe_optim_fold_tensor": (O.FOLD_DTYPE, ["g", "main", "n"])}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "umoe.h"', 'int main(void) {',
           '  printf("bits %d %d\\n", UMOE_OPTIM_P_FP32, UMOE_OPTIM_G_FP32);',
           '  printf("tn %zu %zu %zu\\n", sizeof(umoe_tn_group_t), sizeof(umoe_tgemm_tn_args), sizeof(umoe_swiglu_bwd_args));']
    for cname, (_, fields) in recs.items():
        src.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for f in fields:
            src.append(f'  printf("{cname}.{f} %zu %zu\\n", offsetof({cname}, {f}), sizeof((({cname}*)0)->{f}));')
    src += ['  return 0;', '}']
    cfile, exe = tmp_path / "probe.c", tmp_path / "probe"
    cfile.write_text("\n".join(src))
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(cfile), "-o", str(exe)])
    got = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in subprocess.check_output([str(exe)], text=True).splitlines()}
    for cname, (dt, fields) in recs.items():
        assert got[cname] == [dt.itemsize], cname
        assert list(dt.names) == fields
        for f in fields:
            assert got[f"{cname}.{f}"] == [dt.fields[f][1], dt.fields[f][0].itemsize], (cname, f)
    assert (O.TENSOR_DTYPE.itemsize, O.CHUNK_DTYPE.itemsize, O.FOLD_DTYPE.itemsize) == (56, 16, 24)      # unchanged: 56 and 16
    # the flag word: bit 0 "parameter is fp32, own master", bit 1 "gradient is fp32"; 0 and 1 mean what they meant
    assert got["bits"] == [O.P_FP32, O.G_FP32] == [1, 2]
    # the accumulate entries take the bf16 entries' structs, whose layouts did not change
    import ctypes as C
    assert got["tn"] == [C.sizeof(L.TnGroup), C.sizeof(L.TGemmTnArgs), C.sizeof(L.SwigluBwdArgs)]
    assert len(L.STRUCT_MIRRORS) == 16
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "umoe.h")).read(), flags=re.S)
    lib = C.CDLL(L.build())
    for name in ("umoe_tiled_gemm_tn_acc", "umoe_grouped_swiglu_bwd_acc", "umoe_shared_swiglu_bwd_acc", "umoe_optim_fold"):
        assert name in L.EXPORTS and re.search(r"\bint " + name + r"\(", header) and hasattr(lib, name), name


def test_main_grad_offsets_follow_the_alignment_rule():
    from unimoe_audio_amd import optim as O
    # (data_ptr, element size, numel): aligned, a bf16 view 1, 3, 5 and 7 elements in, odd sizes, an empty tensor
    ps = [(4096, 2, 10), (8192 + 2, 2, 7), (12288 + 6, 2, 1), (16384 + 10, 2, 33), (20480 + 14, 2, 16384), (24576, 2, 0), (28672 + 4, 2, 5)]
    offs, total = O.main_grad_offsets(ps)
    end = 0
    for (ptr, es, n), o in zip(ps, offs):
        assert o >= end and o - end < 8                                   # in order, no overlap, at most a slot and a shift of padding
        h = O._head(ptr, es) % 4
        assert (o + h) % 4 == 0                                           # 16-byte aligned after h elements, like the parameter's fp32 streams
        head = O._head(ptr, es)                                           # the update's head is the parameter's: the main gradient is aligned there
        assert ((o + head) * 4) % 16 == 0 and (ptr + head * es) % 16 == 0
        end = o + n
    assert total == end
    # the same offsets as AdamW._allocate gives the moments of the same parameters
    cur, want = 0, []
    for ptr, es, n in ps:
        h = O._head(ptr, es) % 4
        o = -(-cur // 4) * 4 + (-h) % 4
        want.append(o)
        cur = o + n
    assert offs == want


def test_attach_main_grads_refuses_what_it_cannot_serve():
    from unimoe_audio_amd import train as TR
    from unimoe_audio_amd._lib import UmoeError
    with pytest.raises(UmoeError, match="no trainable bf16 parameter"):
        TR.attach_main_grads([torch.nn.Parameter(torch.zeros(4))])
    with pytest.raises(UmoeError, match="no CPU fallback"):
        TR.attach_main_grads([torch.nn.Parameter(torch.zeros(4, dtype=torch.bfloat16))])
    with pytest.raises(ValueError):
        TR.train_step_accum(torch.nn.Linear(2, 2), None, [])


def test_new_kernels_have_no_scratch_and_no_spills(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "unimoe_audio_amd", "csrc")
    want = {"umoe_optim.hip": ["optim_fold_kernel", "optim_sqsum_kernel", "optim_adamw_kernel"],
            "umoe_tgemm_tn.hip": ["tn_reduce_acc_kernel", "tgemm_tn_kernelILi4ELi2E", "tgemm_tn_kernelILi4ELi1E", "tgemm_tn_kernelILi4ELi0E"]}
    procs = []
    for src in want:
        out = str(tmp_path / (src + ".s"))
        procs.append((src, out, subprocess.Popen([hipcc, "-O3", "-std=c++17", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt",
                                                  "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "--cuda-device-only", "-S",
                                                  os.path.join(csrc, src), "-o", out])))
    for src, out, p in procs:
        assert p.wait() == 0, src
        txt = open(out).read()
        for kern in want[src]:
            m = re.search(r"\.name:\s+\S*" + kern + r"\S*\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n"
                          r"(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", txt)
            assert m, kern
            scratch, sspill, vgprs, vspill = (int(x) for x in m.groups())
            assert (scratch, sspill, vspill) == (0, 0, 0), (kern, m.groups())
            if kern.startswith("tgemm_tn_kernel"):
                assert vgprs <= 256, (kern, vgprs)                        # two workgroups of 512 threads per CU (__launch_bounds__(512, 2))
        if src == "umoe_optim.hip":
            body = txt[txt.index("optim_fold_kernel"):]
            assert "global_load_dwordx4" in body and "global_store_dwordx4" in body


def test_flag_word_restated():
    """what umoe_optim.hip reads out of p_fp32, restated: element sizes of the parameter and of the gradient"""
    from unimoe_audio_amd import optim as O
    sizes = {flags: (4 if flags & O.P_FP32 else 2, 4 if flags & (O.P_FP32 | O.G_FP32) else 2) for flags in range(4)}
    assert sizes == {0: (2, 2), 1: (4, 4), 2: (2, 4), 3: (4, 4)}
    src = open(os.path.join(ROOT, "unimoe_audio_amd", "csrc", "umoe_optim.hip")).read()
    assert "p_fp32 != 0" not in src and "p_fp32 ?" not in src             # every test of the word names its bit
    assert np.dtype(O.TENSOR_DTYPE).fields["p_fp32"][0] == np.dtype("<i4") and R.U == U
