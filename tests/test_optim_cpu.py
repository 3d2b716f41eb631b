"""CPU suite of the optimizer step (unimoe_audio_amd/optim.py, csrc/umoe_optim.hip) -- no device:
  * the fp64 restatement the GPU tests compare against (tests/optim_ref.py) IS torch.optim.AdamW behind clip_grad_norm_ (fp64, CPU);
  * the chunk-table builder covers every element once and never crosses a tensor;
  * the record layouts packed by optim.py are the header's (compiled probe);
  * an fp32 emulation of the kernels' operation order stays inside the derived bounds, and planted errors do not;
  * the compiled kernels use no scratch and spill nothing;
  * the refusals of optim.AdamW that need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import optim_ref as R
from conftest import ROOT

CH = 16384
SIZES = [0, 1, 7, 8, 9, CH - 1, CH, CH + 1, 2 * CH + 3]


@pytest.mark.parametrize("max_norm", [None, 0.5])
def test_restatement_is_torch_adamw_behind_clip_grad_norm(max_norm):
    """5 steps, 2 groups with their own lr / wd / betas / eps, 3 tensors; max_norm 0.5 clips (the norms are ~ 8), None does not"""
    rng = np.random.default_rng(3)
    shapes, group_of = [(7, 5), (33,), (4, 9)], [0, 1, 0]
    hp = [dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1), dict(lr=3e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.0)]
    w0 = [rng.normal(0, 0.3, s) for s in shapes]
    params = [torch.nn.Parameter(torch.tensor(w, dtype=torch.float64)) for w in w0]
    opt = torch.optim.AdamW([dict(params=[p for p, g in zip(params, group_of) if g == gi], **hp[gi]) for gi in range(2)])
    w = [x.copy() for x in w0]
    m = [np.zeros(s) for s in shapes]
    v = [np.zeros(s) for s in shapes]
    worst = 0.0
    for t in range(5):
        grads = [rng.normal(0, 1.0, s) for s in shapes]
        for p, g in zip(params, grads):
            p.grad = torch.tensor(g, dtype=torch.float64)
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(params, max_norm)
        opt.step()
        norm, clip, bcs = R.scalars_fp64(grads, max_norm, [h["betas"] for h in hp], t)
        assert (clip < 1.0) == (max_norm is not None)
        for i, gi in enumerate(group_of):
            h = hp[gi]
            w[i], m[i], v[i], _ = R.adamw_fp64(w[i], m[i], v[i], grads[i], lr=h["lr"], beta1=h["betas"][0], beta2=h["betas"][1], eps=h["eps"],
                                               wd=h["weight_decay"], clip=clip, bc1=bcs[gi][0], bc2=bcs[gi][1])
            ref = params[i].detach().numpy()
            worst = max(worst, float(np.max(np.abs(w[i] - ref) / np.abs(ref))))
            assert np.allclose(m[i], opt.state[params[i]]["exp_avg"].numpy(), rtol=1e-12, atol=0)
            assert np.allclose(v[i], opt.state[params[i]]["exp_avg_sq"].numpy(), rtol=1e-12, atol=0)
    assert worst < 1e-12, worst


def test_chunk_table_covers_every_element_once():
    from unimoe_audio_amd.optim import CHUNK_DTYPE, build_chunk_table
    for ch in (CH, 8, 64):
        sizes = [0, 1, 7, 8, 9, ch - 1, ch, ch + 1, 2 * ch + 3, 0]
        t = build_chunk_table(sizes, ch)
        assert t.dtype == CHUNK_DTYPE and t.dtype.itemsize == 16
        seen = [np.zeros(n, dtype=np.int32) for n in sizes]
        for ti, first in zip(t["tensor"].tolist(), t["first"].tolist()):
            n = sizes[ti]
            assert 0 <= first < n and first % ch == 0                      # starts inside its tensor ...
            seen[ti][first:min(first + ch, n)] += 1                          # ... and the kernel ends the chunk at the tensor's end
        assert all((s == 1).all() for s in seen)
        assert 0 not in t["tensor"].tolist() and len(sizes) - 1 not in t["tensor"].tolist()      # empty tensors get no chunk
        assert t["tensor"].tolist() == sorted(t["tensor"].tolist())
        assert len(t) == sum(-(-n // ch) for n in sizes)
    assert len(build_chunk_table([], CH)) == 0 and len(build_chunk_table([0, 0], CH)) == 0
    for bad in (0, -8, 12):
        with pytest.raises(ValueError):
            build_chunk_table([5], bad)


def test_record_layouts_are_the_headers(tmp_path):
    from unimoe_audio_amd import _lib as L
    from unimoe_audio_amd import optim as O
    recs = {"umoe_optim_tensor": (O.TENSOR_DTYPE, ["p", "g", "master", "m", "v", "n", "group", "p_fp32"]),
            "umoe_optim_chunk": (O.CHUNK_DTYPE, ["tensor", "first"]),
            "umoe_optim_record": (O.RECORD_DTYPE, ["norm", "clip", "skip", "reserved", "bc1", "bc2"])}
    hyper = ["num_groups", "reserved", "max_norm", "lr", "beta1", "beta2", "eps", "wd"]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "umoe.h"', 'int main(void) {', '  printf("groups %d\\n", UMOE_OPTIM_MAX_GROUPS);']
    for cname, (_, fields) in list(recs.items()) + [("umoe_optim_hyper", (None, hyper))]:
        src.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for f in fields:
            src.append(f'  printf("{cname}.{f} %zu %zu\\n", offsetof({cname}, {f}), sizeof((({cname}*)0)->{f}));')
    src += ['  return 0;', '}']
    cfile, exe = tmp_path / "probe.c", tmp_path / "probe"
    cfile.write_text("\n".join(src))
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(cfile), "-o", str(exe)])
    got = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in subprocess.check_output([str(exe)], text=True).splitlines()}
    assert got["groups"] == [O.MAX_GROUPS] == [16]
    for cname, (dt, fields) in recs.items():
        assert got[cname] == [dt.itemsize], cname
        assert list(dt.names) == fields
        for f in fields:
            assert got[f"{cname}.{f}"] == [dt.fields[f][1], dt.fields[f][0].itemsize], (cname, f)
    assert (O.TENSOR_DTYPE.itemsize, O.CHUNK_DTYPE.itemsize, O.RECORD_DTYPE.itemsize) == (56, 16, 144)
    assert got["umoe_optim_hyper"] == [C.sizeof(O.OptimHyper)] and [n for n, _ in O.OptimHyper._fields_] == hyper
    for f in hyper:
        assert got[f"umoe_optim_hyper.{f}"] == [getattr(O.OptimHyper, f).offset, getattr(O.OptimHyper, f).size], f
    # no argument struct joined the mirrors; the entries are declared, listed and exported
    assert len(L.STRUCT_MIRRORS) == 16
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "umoe.h")).read(), flags=re.S)
    lib = C.CDLL(L.build())
    for name in ("umoe_optim_sqsum", "umoe_optim_scalars", "umoe_optim_adamw"):
        assert name in L.EXPORTS and re.search(r"\bint " + name + r"\(", header) and hasattr(lib, name), name


def _case(seed, n=20000):
    rng = np.random.default_rng(seed)
    w = rng.normal(0, 0.03, n).astype(np.float32)
    g = R.bf16_to_f32(R.bf16_rne(rng.normal(0, 2e-3, n).astype(np.float32)))
    m = rng.normal(0, 1e-3, n).astype(np.float32)
    v = (rng.normal(0, 2e-3, n).astype(np.float32)) ** 2 + np.float32(1e-9)
    return w, m, v, g


HP = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.1)


def _ratios(plant, t=10, clip=0.37, seed=0):
    w, m, v, g = _case(seed)
    sc = dict(clip=np.float32(clip), bc1=np.float32(1 - 0.9 ** (t + 1)), bc2=np.float32(1 - 0.999 ** (t + 1)))
    w1, m1, v1, parts = R.adamw_fp64(w, m, v, g, **HP, **sc)
    bw, bm, bv = R.adamw_bounds(parts, lr=HP["lr"], wd=HP["wd"], bc1=sc["bc1"])
    ew, em, ev = R.adamw_emulated(w, m, v, g, **HP, **sc, plant=plant)
    return (float(np.max(np.abs(ew - w1) / bw)), float(np.max(np.abs(em - m1) / bm)), float(np.max(np.abs(ev - v1) / bv)))


def test_fp32_emulation_of_the_update_stays_inside_the_bounds():
    for t in (0, 1, 999):
        for clip in (1.0, 0.37):
            r = _ratios(None, t=t, clip=clip, seed=t)
            print("emulated update: worst error / bound (w, m, v) at t", t, "clip", clip, r)
            assert max(r) <= 1.0, (t, clip, r)


@pytest.mark.parametrize("plant", ["no_bias_correction", "l2_decay", "no_clip", "eps_in_sqrt"])
def test_planted_update_errors_are_rejected(plant):
    r = _ratios(plant)
    assert max(r) > 1.0, (plant, r)


def test_parameter_rounded_from_a_bf16_master_is_rejected():
    """the master must stay fp32: an update computed from the bf16-rounded weight leaves the bound of w by orders of magnitude, and
    bf16_rne of the kernel's own master is what the parameter must equal (the GPU test compares bits)"""
    r = _ratios("bf16_master")
    assert r[0] > 100.0 and r[1] <= 1.0 and r[2] <= 1.0, r
    x = np.array([1.0, 1.00390625, 1.01171875, -1.00390625, 3.0e-39], dtype=np.float32)      # two ties: to even, down and up
    assert R.bf16_rne(x).tolist() == torch.tensor(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16).tolist()


def test_emulated_norm_stays_inside_the_bound_and_an_fp32_stage_2_does_not():
    rng = np.random.default_rng(5)
    g = R.bf16_to_f32(R.bf16_rne(rng.normal(0, 1.0, 3 * CH + 11).astype(np.float32)))
    part = R.sqsum_emulated(g, CH)
    exact = np.array([np.sum(g[i:i + CH].astype(np.float64) ** 2) for i in range(0, len(g), CH)])
    assert len(part) == 4 and np.all(np.abs(part - exact) <= R.gamma(74) * exact)
    norm = np.float32(np.sqrt(R.total_emulated(part)))
    ref = float(np.sqrt(exact.sum()))
    bound = R.norm_rel_bound(CH)
    assert 2.2e-6 < bound < 2.4e-6                                   # (gamma_74 / 2 + u): n_t = 65 squares per thread at CH = 16384
    assert abs(float(norm) - ref) <= bound * ref
    # stage 2 in fp32 over as many chunks as the full model has (1.3 M): the running sum loses the low bits of every partial
    many = rng.uniform(0.5, 1.5, 1_300_000).astype(np.float32)
    ref = float(np.sqrt(many.astype(np.float64).sum()))
    good = float(np.float32(np.sqrt(R.total_emulated(many))))
    bad = float(np.float32(np.sqrt(float(np.cumsum(many, dtype=np.float32)[-1]))))
    assert abs(good - ref) <= (R.U + 2.0 ** -40) * ref
    assert abs(bad - ref) > bound * ref, (bad, ref, abs(bad - ref) / ref, bound)


def test_kernels_have_no_scratch_and_no_spills(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "unimoe_audio_amd", "csrc")
    out = str(tmp_path / "umoe_optim.s")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt", "--offload-arch=gfx950",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "--cuda-device-only", "-S", os.path.join(csrc, "umoe_optim.hip"), "-o", out])
    txt = open(out).read()
    seen = 0
    for kern in ("optim_sqsum_kernel", "optim_scalars_kernel", "optim_adamw_kernel"):
        m = re.search(r"\.name:\s+\S*" + kern + r"\S*\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n"
                      r"(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", txt)
        assert m, kern
        assert [int(x) for x in m.groups()] == [0, 0, 0], (kern, m.groups())
        seen += 1
    assert seen == 3
    # 16-byte vector loads and stores on the update's streams
    body = txt[txt.index("optim_adamw_kernel"):]
    assert "global_load_dwordx4" in body and "global_store_dwordx4" in body


def test_adamw_refusals_that_need_no_device():
    from unimoe_audio_amd._lib import UmoeError
    from unimoe_audio_amd.optim import AdamW
    P = torch.nn.Parameter
    with pytest.raises(UmoeError, match="CPU tensor"):
        AdamW([P(torch.zeros(8, dtype=torch.bfloat16))], lr=1e-3)
    with pytest.raises(UmoeError, match="bf16 .* or fp32"):
        AdamW([P(torch.zeros(8, dtype=torch.float16))], lr=1e-3)
    with pytest.raises(UmoeError, match="bf16 .* or fp32"):
        AdamW([P(torch.zeros(8, dtype=torch.float64))], lr=1e-3)
    with pytest.raises(UmoeError, match="parameter groups"):
        AdamW([dict(params=[P(torch.zeros(8))]) for _ in range(17)], lr=1e-3)
    released = P(torch.empty(0, dtype=torch.bfloat16))
    released.allreduce, released.group_name = False, "ep_size_1"
    with pytest.raises(UmoeError, match=r"inference only: `quant.dequantize_experts_` first"):
        AdamW([released], lr=1e-3)
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(capturable=True)):
        with pytest.raises(TypeError):
            AdamW([P(torch.zeros(8))], lr=1e-3, **kw)
    with pytest.raises(TypeError):
        AdamW(torch.nn.Linear(2, 2), lr=1e-3)
    with pytest.raises(ValueError):
        AdamW([P(torch.zeros(8))], lr=-1.0)
    with pytest.raises(ValueError):
        AdamW([P(torch.zeros(8))], lr=1e-3, betas=(0.9, 1.0))
