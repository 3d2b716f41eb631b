"""GPU tests of fp8-only expert weights: the tiled MFMA GEMM on WP8 blocks (umoe_tiled_gemm_wp8) bit for bit against
umoe_tiled_gemm on the dequantized weights and against exact float64 products, the fp8-only engine (prefill on e4m3, no bf16 expert weight
resident) bit for bit against the fp8 engine that kept bf16, the short prefill against a bf16 summation-order yardstick, the memory the
mode frees, and the refusals of everything that would stream a bf16 expert weight."""
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
EPI_BF16, EPI_SWIGLU = 0, 2
SENT = 7.0
KS = [32, 96, 352, 1376, 2048]           # one granule per quarter, quarters of 16 + 8, the production tail (344 = 21 * 16 + 8), no tail
NS = [16, 48, 144, 1376]
ROWS = [1, 17, 63, 64, 129, 300]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from unimoe_audio_amd import _lib, ops
    _lib.lib()
    assert (ops.EPI_BF16, ops.EPI_SWIGLU) == (EPI_BF16, EPI_SWIGLU)
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ 1. / 2. op level
def poisoned_pack(q, e, q2=None, e2=None):
    """WP8 blocks of q [N][K] (+ q2: the interleaved gate/up pair) with every byte the kernel must not read made poisonous: the bytes past
    a K quarter's end and the padded rows hold the e4m3 NaN 0x7F, the exponent slots of padded rows 127 (2^127: a finite product
    overflows, a zero turns NaN with the NaN bytes beside it)."""
    from unimoe_audio_amd import quant
    ones, one_e = torch.ones_like(q), torch.ones_like(e)
    if q2 is None:
        packed, ex = quant.pack_wp8(q, e)
        live, live_e = quant.pack_wp8(ones, one_e)
    else:
        packed, ex = quant.pack_wp8_gate_up(q, e, q2, e2)
        live, live_e = quant.pack_wp8_gate_up(ones, one_e, ones, one_e)
    packed = torch.where(live == 0, torch.full_like(packed, 0x7F), packed)
    ex = torch.where(live_e == 0, torch.full_like(ex, 127), ex)
    return packed.contiguous(), ex.contiguous()


def random_weight(N, K, gen, dev):
    """random e4m3 codes (no NaN code) and exponents in [-24, 8], different per row"""
    q = torch.randint(0, 256, (N, K), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8)
    q = torch.where((q & 0x7F) == 0x7F, torch.full_like(q, 0x3C), q)
    e = torch.randint(-24, 9, (N,), generator=gen, device=dev, dtype=torch.int32).to(torch.int8)
    return q, e


_WEIGHTS = {}


def group_weights(epi, K, N, G, dev, seed=0):
    """G groups' weights of one shape, made once per module: (WP8 dicts, dequantized row-major tensors)"""
    from unimoe_audio_amd.quant import dequantize_fp8_rows
    key = (epi, K, N, G, seed)
    if key not in _WEIGHTS:
        gen = torch.Generator(device=dev).manual_seed(1000 * K + N + 7 * epi + seed)
        out = []
        for _ in range(G):
            q, e = random_weight(N, K, gen, dev)
            if epi == EPI_SWIGLU:
                q2, e2 = random_weight(N, K, gen, dev)
                w8, ex = poisoned_pack(q, e, q2, e2)
                out.append(dict(w8=w8, exps=ex, w=dequantize_fp8_rows(q, e), w2=dequantize_fp8_rows(q2, e2)))
            else:
                w8, ex = poisoned_pack(q, e)
                out.append(dict(w8=w8, exps=ex, w=dequantize_fp8_rows(q, e)))
        _WEIGHTS[key] = out
    return _WEIGHTS[key]


def ragged_case(K, N, counts, dev, seed, int_data=False):
    """Activations, a permuted gather list with per-group row offsets and device-side counts, and sentinel outputs: every activation row
    outside the gather list is NaN.  Group g reads list entries [off_g, off_g + count_g) and writes output rows 2 + off_g + r."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    total = sum(counts)
    RA = 2 * total + 11
    lda = K + 8
    a = torch.full((RA, lda), float("nan"), dtype=bf16)
    pick = torch.randperm(RA, generator=gen)[:total]                  # a permuted list of distinct rows
    vals = torch.randint(-4, 5, (total, K), generator=gen).to(bf16) if int_data else torch.randn((total, K), generator=gen).to(bf16)
    a[pick, :K] = vals
    lead = 3                                                          # list entries in front of the first group: rows that hold NaN
    picked = set(pick.tolist())
    unused = [r for r in range(RA) if r not in picked][:lead]
    rows = torch.cat([torch.tensor(unused, dtype=torch.int64), pick]).to(torch.int32)
    offs, o = [], lead
    for c in counts:
        offs.append(o)
        o += c
    d = dict(a=a.to(dev), rows=rows.to(dev), lda=lda, offs=offs, counts=counts, vals=vals, pick=pick,
             row_off=[torch.tensor([x], dtype=torch.int32, device=dev) for x in offs],
             count=[torch.tensor([c], dtype=torch.int32, device=dev) for c in counts])
    return d


def launch_pair(epi, K, N, ws, case, dev, reference=True):
    """the WP8 launch and (reference) the bf16 launch on the dequantized weights -> (out_wp8, out_bf16, written mask)"""
    from unimoe_audio_amd import ops
    total_rows = 2 + case["offs"][-1] + case["counts"][-1] + 5
    ldo = N + 8
    outs = []
    for kind in (("wp8", "bf16") if reference else ("wp8",)):
        out = torch.full((total_rows, ldo), SENT, dtype=bf16, device=dev)
        groups = []
        for g, w in enumerate(ws):
            d = dict(rows=case["rows"], row_off=case["row_off"][g], count=case["count"][g], out_row_base=2)
            if kind == "wp8":
                d.update(w8=w["w8"], exps=w["exps"], n=N, k=K)
            else:
                d.update(w=w["w"], w2=w.get("w2"))
            groups.append(d)
        fn = ops.tiled_gemm_wp8 if kind == "wp8" else ops.tiled_gemm
        fn(groups, case["a"], out, max_rows=max(case["counts"]), epilogue=epi)
        outs.append(out)
    torch.cuda.synchronize()
    written = torch.zeros((total_rows, ldo), dtype=torch.bool)
    for off, c in zip(case["offs"], case["counts"]):
        written[2 + off: 2 + off + c, :N] = True
    return outs[0].cpu(), (outs[1].cpu() if reference else None), written


def check_written(got, written, what):
    assert bool((got[~written].float() == SENT).all()), f"{what}: a row or column outside the groups changed"
    assert bool(torch.isfinite(got[written].float()).all()), f"{what}: NaN / inf in a group's output (a poisoned byte, exponent or row was read)"
    assert bool((got[written].float() != SENT).any()) or not bool(written.any())


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("epi", [EPI_SWIGLU, EPI_BF16])
def test_wp8_tiled_gemm_is_bit_identical_to_the_bf16_kernel_on_the_dequantized_weights(dev, epi, K):
    """Three groups in one launch with device-side counts {0, 5, rows}, a permuted gather list and row offsets; every byte the kernel
    must not read is NaN (quarter padding, padded rows and their exponents, activation rows outside the list); the output starts as a
    sentinel.  N = 40 (BF16 epilogue) adds a last block with 8 padded rows."""
    for N in NS + ([40] if epi == EPI_BF16 else []):
        ws = group_weights(epi, K, N, 3, dev)
        for rows in ROWS:
            case = ragged_case(K, N, [0, min(5, rows), rows], dev, seed=K + N + rows)
            got, ref, written = launch_pair(epi, K, N, ws, case, dev)
            what = f"epi {epi} K {K} N {N} rows {rows}"
            check_written(got, written, what)
            assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), what


def fp64_interval_ok(got, a_rows, w, K):
    """BF16 epilogue: out in [bf16(ref - E), bf16(ref + E)], E = K u sum |a w| (tests/test_gpu_gemm_fp64.py), per element"""
    a64, w64 = a_rows.double(), w.double().cpu()
    ref, ab = a64 @ w64.T, a64.abs() @ w64.abs().T
    e = K * 2.0 ** -24 * ab
    lo, hi = (ref - e).to(bf16).double(), (ref + e).to(bf16).double()
    g = got.double()
    return bool(((g >= lo) & (g <= hi)).all())


@pytest.mark.parametrize("name", ["tile256_swiglu", "rows1024_bf16"])
def test_wp8_tiled_gemm_at_1024_rows(dev, name):
    """1024 rows x 4 groups of N = 2048: the bf16 call takes tgemm_pp_kernel (256 x 256 ping-pong tiles), whose equality with tgemm_kernel
    umoe_tgemm.hip promises only up to summation order.  tile256_swiglu: the WP8 call runs the 256-token tiles (512 workgroups of them);
    rows1024_bf16: the 128-token tiles.  OBSERVED on MI355X: bit equality in both (the ping-pong kernel also adds one MFMA per 32 columns
    of K to an accumulator, in K order).  Where that ever stops holding the BF16 case falls back to the fp64 interval for both results;
    the SwiGLU epilogue is no monotone map, so its case then has only the exact-data test below behind it and fails here."""
    epi = EPI_SWIGLU if name == "tile256_swiglu" else EPI_BF16
    K, N, G, rows = 352, 2048, 4, 1024
    ws = group_weights(epi, K, N, G, dev)
    case = ragged_case(K, N, [rows] * G, dev, seed=5)
    got, ref, written = launch_pair(epi, K, N, ws, case, dev)
    check_written(got, written, name)
    same = torch.equal(got.view(torch.int16), ref.view(torch.int16))
    print(f"{name}: WP8 tiles vs the bf16 call at {rows} rows bit-identical: {same}")
    if same:
        return
    assert epi == EPI_BF16, "SwiGLU outputs differ from the ping-pong kernel's (summation order): no interval for a non-monotone epilogue"
    o = 0
    for g in range(G):
        a_rows = case["vals"][o:o + rows]
        o += rows
        rs = slice(2 + case["offs"][g], 2 + case["offs"][g] + rows)
        for res in (got, ref):
            assert fp64_interval_ok(res[rs, :N], a_rows, ws[g]["w"], K), (name, g)


@pytest.mark.parametrize("name,K,N,G,rows", [("tail", 1376, 144, 3, 300), ("tile256", 96, 2048, 8, 1024), ("one_granule", 32, 48, 3, 17)])
def test_wp8_tiled_gemm_equals_an_exact_float64_product(dev, name, K, N, G, rows):
    """Activations in -4 .. 4, weights = integers -8 .. 8 times 2^e (e in 0 .. 2): every product and partial sum is an integer below 2^24,
    exact in fp32 in any order, so the bf16 output must equal the rounded float64 product with no tolerance.  Pins the granule addressing
    (quarters, the K = 1376 tail, the exponents) and both tile heights independently of the bf16 kernel."""
    gen = torch.Generator(device="cpu").manual_seed(K + N)
    ws, wref = [], []
    for _ in range(G):
        wi = torch.randint(-8, 9, (N, K), generator=gen).float()
        e = torch.randint(0, 3, (N,), generator=gen).to(torch.int8)
        q = wi.to(torch.float8_e4m3fn).view(torch.uint8)
        assert torch.equal(q.view(torch.float8_e4m3fn).float(), wi)
        w8, ex = poisoned_pack(q.to(dev), e.to(dev))
        ws.append(dict(w8=w8, exps=ex))
        wref.append(wi.double() * torch.exp2(e.double())[:, None])
    counts = [0, min(5, rows), rows] if G == 3 else [rows] * G
    case = ragged_case(K, N, counts, dev, seed=K, int_data=True)
    got, _, written = launch_pair(EPI_BF16, K, N, ws, case, dev, reference=False)
    check_written(got, written, name)
    o = 0
    for g, c in enumerate(counts):
        want = (case["vals"][o:o + c].double() @ wref[g].T).to(bf16)
        o += c
        rs = slice(2 + case["offs"][g], 2 + case["offs"][g] + c)
        assert torch.equal(got[rs, :N].view(torch.int16), want.view(torch.int16)), (name, g)


def test_wp8_tiled_gemm_refuses_what_it_does_not_do(dev):
    from unimoe_audio_amd import _lib as L, ops
    w = group_weights(EPI_BF16, 32, 16, 3, dev)[0]
    a = torch.zeros(8, 40, dtype=bf16, device=dev)
    out = torch.zeros(8, 16, dtype=bf16, device=dev)
    g = dict(w8=w["w8"], exps=w["exps"], n=16, k=32, static_count=8)
    for bad, epi, msg in ((dict(g, k=40), EPI_BF16, "k % 32"), (g, 1, "epilogue"), (dict(g, n=24), EPI_SWIGLU, "n % 16")):
        with pytest.raises(L.UmoeError, match=msg):
            ops.tiled_gemm_wp8([bad], a, out, max_rows=8, epilogue=epi)


# ------------------------------------------------------------------------------------------------ 3. - 6. engine
def ref_cfg(layers=2):
    from unimoe_audio_amd.config import UniMoEAudioConfig
    return UniMoEAudioConfig(hidden_size=2048, num_hidden_layers=layers, num_attention_heads=16, num_key_value_heads=2, vocab_size=320,
                             dynamic_intermediate_size=2752, shared_intermediate_size=1376, codec_placeholder_value=300)


def build(cfg, seed, std=0.03):
    from unimoe_audio_amd.model import UniAudioRVQQwen2_5VLMoEForConditionalGeneration
    torch.manual_seed(seed)
    m = UniAudioRVQQwen2_5VLMoEForConditionalGeneration(cfg)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "layernorm" in n or n.endswith("norm.weight"):
                p.copy_(1 + 0.05 * torch.randn_like(p))
            else:
                p.normal_(0, 0.02 if n.endswith("bias") else std)
    return m.to(bf16).eval()


def prompt(cfg, B, T, seed):
    torch.manual_seed(seed)
    ids = torch.randint(0, 290, (2 * B, T))
    am = torch.ones(2 * B, T, dtype=torch.long)
    am[0, :1] = 0
    ids[:, -5:-2] = cfg.codec_placeholder_value
    codec = torch.randint(0, 1024, (2 * B * 3, cfg.codec_channels))
    return ids, am, codec


def run_engine(m, cfg, B, fmt, steps, use_graph, dev, T=12, pseed=4):
    """prefill + `steps` sampled decode steps of a fresh engine -> tokens, router masks, top-k, logits (after the first and the last step),
    per-layer router logits of an eager probe step, info"""
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    from unimoe_audio_amd.model import DecodeEngine
    ids, am, codec = prompt(cfg, B, T, pseed)
    eng = DecodeEngine(m, B, Lmax=T + steps + 80, Tmax=steps + 72, expert_weights=fmt)
    x = m.calculate_input_embedding(ids.to(dev), codec.to(dev))
    eng.prefill(x.reshape(-1, cfg.hidden_size).contiguous(), am.to(dev))
    out = dict(prefill_fp8=eng.info("prefill_fp8"), bf16_resident=eng.info("expert_bf16_resident"), fmt=eng.expert_weights)
    pre, psteps = prepare_audio_prompt(cfg, [None] * B)
    eng.start_decode(pre, psteps, steps + 8, 4, cfg_scale=2.0, temperature=1.0, top_p=0.9, top_k=45, eos_mul=0.8, do_sample=True, seed=3)
    E = cfg.num_experts
    for i in range(steps):
        eng.step(use_graph)
        if i == 0:
            out["logits0"] = eng.copy_buffer("logits", torch.float32, (2 * B, cfg.codec_channels * cfg.codec_vocab_size)).cpu()
            out["mask0"] = eng.copy_buffer("all_mask", torch.int32, (cfg.num_hidden_layers, 2 * B, E)).cpu()
    torch.cuda.synchronize()
    out.update(tokens=eng.tokens.cpu().clone(),
               mask=eng.copy_buffer("all_mask", torch.int32, (cfg.num_hidden_layers, 2 * B, E)).cpu(),
               topk=eng.copy_buffer("all_topk", torch.int64, (cfg.num_hidden_layers, 2 * B)).cpu(),
               logits=eng.copy_buffer("logits", torch.float32, (2 * B, cfg.codec_channels * cfg.codec_vocab_size)).cpu())
    probe = eng.set_probe(dump_logits=True)
    eng.step(False)
    torch.cuda.synchronize()
    out["router_logits"] = probe["logits"].cpu().clone()
    eng.set_probe()
    out["expert_fp8"] = eng.info("expert_fp8")
    out["handoff"] = eng.handoff_error()
    eng.close()
    return out


@pytest.fixture(scope="module")
def host_model():
    """the 2-layer model at the reference width, initialised once on the host; every test moves a copy of its own to the device"""
    cfg = ref_cfg()
    return build(cfg, 31), cfg


def fresh(host_model, dev):
    import copy
    return copy.deepcopy(host_model[0]).to(dev)


@pytest.fixture(scope="module")
def qmodel(dev, host_model):
    """the quantized 2-layer model that kept bf16 (W_deq): fp8-only engines on it get the same WP8 blocks and no bf16 expert pointer"""
    cfg = host_model[1]
    m = fresh(host_model, dev)
    m.quantize_experts_("fp8")
    yield m, cfg
    del m
    torch.cuda.empty_cache()


@pytest.mark.parametrize("B", [3, 8])
def test_fp8_only_engine_is_bit_identical_to_the_fp8_engine_that_kept_bf16(dev, qmodel, B):
    """Prefill of 72 / 192 rows (MOE_TILED in both: the WP8 tiles against the bf16 tiles on W_deq) and 6 sampled steps, eager and graph."""
    m, cfg = qmodel
    for use_graph in (False, True):
        a = run_engine(m, cfg, B, "fp8", 6, use_graph, dev)
        b = run_engine(m, cfg, B, "fp8-only", 6, use_graph, dev)
        assert (a["prefill_fp8"], a["bf16_resident"], a["fmt"]) == (0, 1, "fp8")
        assert (b["prefill_fp8"], b["bf16_resident"], b["fmt"]) == (1, 0, "fp8-only")
        assert a["handoff"] == 0 and b["handoff"] == 0 and a["expert_fp8"] == 1 and b["expert_fp8"] == 1
        for k in ("tokens", "mask", "topk", "logits", "logits0", "router_logits"):
            assert torch.equal(a[k], b[k]), (k, B, use_graph)


def test_fp8_only_admission_is_bit_identical(dev, qmodel):
    """start_serving / admit with a prompt of T = 40 (an 80-row admission prefill): the admitted row's codes are identical."""
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    from unimoe_audio_amd.model import DecodeEngine
    m, cfg = qmodel
    T = 40
    ids, am, codec = prompt(cfg, 1, T, 9)
    x = m.calculate_input_embedding(ids.to(dev), codec.to(dev)).reshape(-1, cfg.hidden_size).contiguous()
    pre, ps = prepare_audio_prompt(cfg, [None])
    kw = dict(cfg_scale=2.0, temperature=1.0, top_p=0.9, top_k=45, eos_mul=0.8, do_sample=True, seed=3, min_tokens=4, max_tokens=10)
    res = {}
    for fmt in ("fp8", "fp8-only"):
        eng = DecodeEngine(m, 2, Lmax=T + 120, Tmax=96, expert_weights=fmt)
        eng.start_serving(T)
        eng.admit(1, x, am, pre[0], ps[0], **kw)
        pf = eng.info("prefill_fp8")
        n = 0
        while True:
            eng.step(True)
            n += 1
            if eng.row_done(eng.poll(), 1):
                break
            assert n < 200
        codes, length = eng.take(1)
        res[fmt] = (codes.cpu(), length, pf)
        eng.close()
    assert res["fp8"][2] == 0 and res["fp8-only"][2] == 1
    assert res["fp8"][1] == res["fp8-only"][1] and torch.equal(res["fp8"][0], res["fp8-only"][0])


def rel_l2(a, b):
    return float((a - b).norm() / b.norm())


def test_short_prefill_differs_only_by_summation_order(dev, qmodel, monkeypatch):
    """B = 1, T = 12 (24 rows): the fp8-only engine runs MOE_TILED on WP8, the fp8 engine MOE_RAGGED on WP16 -- the same weights, another
    fp32 summation order.  Yardstick from the parent's code: a bf16 engine with UMOE_TILED_PREFILL=1 against one with =0 at B = 3 (72
    rows: tiled against ragged, two summation orders of the same bf16 weights), relative L2 of the first step's logits.  Bound: 4 x the
    yardstick (another row count, a single sample).  Prompt seed 4: the router masks of the two bf16 forms agree on it too, so the metric
    compares logits of the same routing.
    Measured on MI355X (profiles/fp8_only.json "short_prefill"): fp8-only against fp8 0.0047, yardstick 0.0500 (bound 0.200); the router
    masks agree in both pairs."""
    m, cfg = qmodel
    a = run_engine(m, cfg, 1, "fp8", 1, False, dev)
    b = run_engine(m, cfg, 1, "fp8-only", 1, False, dev)
    assert a["prefill_fp8"] == 0 and b["prefill_fp8"] == 1
    monkeypatch.setenv("UMOE_TILED_PREFILL", "1")
    y1 = run_engine(m, cfg, 3, "bf16", 1, False, dev)
    monkeypatch.setenv("UMOE_TILED_PREFILL", "0")
    y0 = run_engine(m, cfg, 3, "bf16", 1, False, dev)
    monkeypatch.delenv("UMOE_TILED_PREFILL")
    got, yard = rel_l2(b["logits0"], a["logits0"]), rel_l2(y1["logits0"], y0["logits0"])
    rec = {"fp8only_vs_fp8_rel_l2_B1": got, "yardstick_bf16_tiled_vs_ragged_rel_l2_B3": yard, "bound": 4 * yard,
           "masks_equal_fp8": bool(torch.equal(a["mask0"], b["mask0"])), "masks_equal_yardstick": bool(torch.equal(y1["mask0"], y0["mask0"]))}
    print("short prefill:", json.dumps(rec))
    assert rec["masks_equal_yardstick"], "pick another prompt seed: the two bf16 forms route differently on this one"
    assert rec["masks_equal_fp8"]
    assert got <= 4 * yard, rec


def expert_elems(cfg):
    D, Id, Is = cfg.hidden_size, cfg.dynamic_intermediate_size, cfg.shared_intermediate_size
    return cfg.num_hidden_layers * 3 * D * (cfg.mlp_dynamic_expert_num * Id + cfg.mlp_fixed_expert_num * Is)


def test_fp8_only_frees_the_bf16_expert_weights(dev, host_model):
    """torch.cuda.memory_allocated() after model and engine, each mode in a fresh model.  With P expert elements: bf16 holds 4 P bytes of
    them (parameters + WP16 packs), fp8 that kept bf16 5 P, fp8-only at most 1.03 P (e4m3 + the K = 1376 quarter padding + exponents)."""
    from unimoe_audio_amd.model import DecodeEngine
    cfg = ref_cfg()
    P = expert_elems(cfg)
    used = {}
    import gc
    for mode in ("bf16", "fp8", "fp8-only"):
        # garbage of earlier tests (models and engines in reference cycles) must go BEFORE the base is read: collected later, inside the
        # measured span, it would be booked as memory this mode gave back
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        m = fresh(host_model, dev)
        if mode != "bf16":
            m.quantize_experts_("fp8", keep_bf16=mode == "fp8")
        eng = DecodeEngine(m, 2, Lmax=64, Tmax=64, expert_weights=mode)
        assert eng.expert_weights == mode and eng.info("expert_bf16_resident") == (0 if mode == "fp8-only" else 1)
        gc.collect()
        torch.cuda.synchronize()
        used[mode] = torch.cuda.memory_allocated() - base
        assert used[mode] > 0, (mode, used[mode], base)
        eng.close()
        del eng, m
    torch.cuda.empty_cache()
    print("expert elements", P, "bytes allocated", used, "in units of P", {k: round(v / P, 3) for k, v in used.items()})
    assert used["bf16"] - used["fp8-only"] >= 2.9 * P, used
    assert used["fp8"] - used["fp8-only"] >= 3.9 * P, used


def test_fp8_only_refuses_every_path_that_would_stream_bf16_expert_weights(dev, host_model, monkeypatch):
    from unimoe_audio_amd import _lib as L, quant
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    from unimoe_audio_amd.model import DecodeEngine
    cfg = host_model[1]
    m = fresh(host_model, dev)
    m.quantize_experts_("fp8")
    before = run_engine(m, cfg, 2, "bf16", 4, True, dev)            # the bf16 engine on W_deq, nothing dropped yet
    m.quantize_experts_("fp8", keep_bf16=False)
    assert quant.expert_format(m) == "fp8-only" and m.language_model.layers[0].mlp.fixed_real_moe[0].down_proj.weight.numel() == 0
    ids, am, codec = prompt(cfg, 2, 12, 4)
    x = m.calculate_input_embedding(ids.to(dev), codec.to(dev))
    # the module forward, saving, and engines that want the bf16 weights
    with pytest.raises(L.UmoeError, match="dequantize_experts_"):
        m.text_forward(x, am.to(dev))
    with pytest.raises(L.UmoeError, match="dequantize_experts_"):
        m.state_dict()
    for fmt in ("bf16", "fp8"):
        with pytest.raises(L.UmoeError, match="dequantize_experts_"):
            DecodeEngine(m, 2, Lmax=100, Tmax=80, expert_weights=fmt)
    # UMOE_TILED_PREFILL=0: the prefill is refused on the host (read at engine creation)
    monkeypatch.setenv("UMOE_TILED_PREFILL", "0")
    eng = DecodeEngine(m, 2, Lmax=100, Tmax=80)
    assert eng.expert_weights == "fp8-only"
    with pytest.raises(L.UmoeError, match="no bf16 expert weights"):
        eng.prefill(x.reshape(-1, cfg.hidden_size).contiguous(), am.to(dev))
    eng.close()
    monkeypatch.delenv("UMOE_TILED_PREFILL")
    # UMOE_FLAT_MOE=0: the decode step is refused, eager and captured, and nothing ran
    eng = DecodeEngine(m, 2, Lmax=100, Tmax=80)
    eng.prefill(x.reshape(-1, cfg.hidden_size).contiguous(), am.to(dev))
    pre, psteps = prepare_audio_prompt(cfg, [None] * 2)
    eng.start_decode(pre, psteps, 16, 4, cfg_scale=2.0, temperature=1.0, top_p=0.9, top_k=45, eos_mul=0.8, do_sample=True, seed=3)
    tok = eng.tokens.cpu().clone()
    monkeypatch.setenv("UMOE_FLAT_MOE", "0")
    for use_graph in (False, True):
        with pytest.raises(L.UmoeError, match="no bf16 expert weights"):
            eng.step(use_graph)
    monkeypatch.delenv("UMOE_FLAT_MOE")
    torch.cuda.synchronize()
    assert torch.equal(eng.tokens.cpu(), tok)
    eng.close()
    # reversible: W_deq comes back exactly, and a bf16 engine decodes the tokens it decoded before anything was dropped
    quant.dequantize_experts_(m)
    after = run_engine(m, cfg, 2, "bf16", 4, True, dev)
    for k in ("tokens", "mask", "topk", "logits"):
        assert torch.equal(before[k], after[k]), k
    del m
    torch.cuda.empty_cache()
