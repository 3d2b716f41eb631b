"""GPU tests of w12-only expert weights: the tiled MFMA GEMM on WP12 blocks (umoe_tiled_gemm_w12) bit for bit against
umoe_tiled_gemm on the same weights given row-major -- plain, with exceptions planted at every edge the kernel has, with poison in
everything it must not read -- and against exact float64 products; its refusals; the w12-only engine (prefill, flat launch and wide step on
the WP12 copies, no bf16 expert weight resident) bit for bit against the default bf16 engine; the short prefill against the bf16 engine's
own summation-order distance; a mixed engine; the memory the mode frees; and the refusals of everything that would stream a bf16 expert
weight."""
import copy
import gc
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
EPI_BF16, EPI_SWIGLU = 0, 2
SENT = 7.0
NAN16 = 0x7FC0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from unimoe_audio_amd import _lib, ops
    _lib.lib()
    assert (ops.EPI_BF16, ops.EPI_SWIGLU) == (EPI_BF16, EPI_SWIGLU)
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ packing with poison behind it
def poison_tail(data, meta, KB, blocks=2):
    """`blocks` more blocks behind the last real one: 0xFF bytes (a window base of 0x7F and low bytes 0xFF rebuild NaN) and records whose
    32 entries would patch NaN into k-step 0 of every lane."""
    from unimoe_audio_amd import w12
    ent = [(0 << 25) | (lane << 19) | (j << 16) | NAN16 for lane in range(8) for j in range(4)]
    rec = torch.tensor(ent + [0xFFFFFFFF] * (w12.META - 33) + [0x78], dtype=torch.int64)
    rec = torch.where(rec >= 2 ** 31, rec - 2 ** 32, rec).to(torch.int32).to(meta.device)
    return (torch.cat([data, torch.full((blocks * w12.block_bytes(KB),), 0xFF, dtype=torch.uint8, device=data.device)]).contiguous(),
            torch.cat([meta] + [rec] * blocks).contiguous())


def pack_rows(W, W2=None):
    """WP12 blocks + records of W [N][K] (N % 16 == 0; with W2 the interleaved gate/up pair), poison behind the last block"""
    from unimoe_audio_amd import w12
    K = W.shape[1]
    p = w12.pack(w12.wp16_from_rows(W) if W2 is None else w12.wp16_gate_up(W, W2), K // 32)
    assert p is not None, "the test's weights must be packable"
    assert torch.equal(w12.unpack(p[0], p[1], K // 32), w12.wp16_from_rows(W) if W2 is None else w12.wp16_gate_up(W, W2))
    return poison_tail(p[0], p[1], K // 32), int(w12.exceptions_per_block(p[1]).max())


def gauss(N, K, gen, dev):
    return (torch.randn((N, K), generator=gen, device=dev) * 0.02).to(bf16)


def plant_plan(N, K, seed, full_block=None):
    """[(n, k, value)] covering, for the matrix [N][K]: the first and the last granule of every K tile of both tile widths (32 and 64
    columns: the 64-wide edges are among the 32-wide ones), both sides of every K-quarter edge, the first and last row of a 16-row block
    and of a 128-row tile, two entries in one granule, two in one k-step in different lanes, and the last real block.  Entries go round
    robin over the blocks; no block gets more than 20.  full_block: that block is topped up with zeros to `full_block[1]` planted."""
    g = torch.Generator().manual_seed(seed)
    vals = (0.0, 2.0 ** -30, 8.0)
    NB, Q = N // 16, K // 4
    cols = []
    for t in range(K // 32):
        cols += [32 * t + int(torch.randint(0, 8, (1,), generator=g)), 32 * t + 24 + int(torch.randint(0, 8, (1,), generator=g))]
    for h in range(1, 4):
        cols += [h * Q - 1, h * Q]
    cols += [0, K - 1]
    plan, per = {}, [0] * NB
    rows_in_block = (0, 15, 7, 8)
    for x, k in enumerate(cols):
        nb = x % NB
        n = 16 * nb + rows_in_block[(x // NB) % 4]
        plan[(n, k)] = vals[x % 3]
    # rows: first / last of a 128-row tile and of the matrix; two in one granule; two in one k-step in different lanes (same block)
    extra = [(0, 8), (min(N, 128) - 1, 16 if K > 16 else 1), (N - 1, K - 9), (N - 1, K - 12), (16 * (NB - 1) + 3, 2), (16 * (NB - 1) + 9, 5)]
    for x, (n, k) in enumerate(extra):
        plan[(n, k % K)] = vals[x % 3]
    for (n, k) in plan:
        per[n // 16] += 1
    assert max(per) <= 20, (N, K, per)
    if full_block is not None:
        nb, want = full_block
        x = 0
        while per[nb] < want:
            n, k = 16 * nb + (x * 7) % 16, (x * 41 + 3) % K
            x += 1
            if (n, k) not in plan:
                plan[(n, k)] = 0.0
                per[nb] += 1
    return [(n, k, v) for (n, k), v in plan.items()]


def planted(N, K, gen, dev, seed, full_block=None):
    W = gauss(N, K, gen, dev)
    plan = plant_plan(N, K, seed, full_block)
    idx = torch.tensor([(n, k) for n, k, _ in plan], device=dev)
    W[idx[:, 0], idx[:, 1]] = torch.tensor([v for _, _, v in plan], device=dev).to(bf16)
    return W, len(plan)


def make_groups(epi, K, N, G, dev, seed, plant=False, full=False):
    """G groups of one shape: dict(w12, meta, n, k, w, w2) -- the WP12 pack (with poison behind it) and the same weights row-major.
    BF16 epilogue and N % 16 != 0: the pack has ceil(N / 16) blocks whose rows >= N are NaN (exceptions that must never be patched)."""
    from unimoe_audio_amd import w12
    gen = torch.Generator(device=dev).manual_seed(seed)
    NP = -(-N // 16) * 16
    out = []
    for g in range(G):
        def one(s):
            if plant:
                W, _ = planted(NP, K, gen, dev, s)
            else:
                W = gauss(NP, K, gen, dev)
            if NP != N:
                W[N:, [0, K // 2, K - 1]] = float("nan")     # 3 per row: 24 in the block's record, next to those of the rows below N
            return W
        W = one(seed + 10 * g)
        if epi == EPI_SWIGLU:
            W2 = one(seed + 10 * g + 5)
            (d, m), mx = pack_rows(W, W2)
            out.append(dict(w12=d, meta=m, n=N, k=K, w=W[:N], w2=W2[:N], maxexc=mx))
        else:
            (d, m), mx = pack_rows(W)
            out.append(dict(w12=d, meta=m, n=N, k=K, w=W[:N].contiguous(), maxexc=mx))
    if full:                                                     # one block at exactly the cap
        W = out[0]["w"].clone()
        nb = (N // 16) - 1
        p0 = w12.pack(w12.wp16_from_rows(W), K // 32)
        have = int(w12.exceptions_per_block(p0[1])[nb])
        x = 0
        while have < w12.CAP:
            n, k = 16 * nb + (x * 7) % 16, (x * 41 + 3) % K
            x += 1
            if float(W[n, k]) != 0.0 and 2.0 ** -10 < abs(float(W[n, k])) < 1.0:
                W[n, k] = 0.0
                have += 1
        assert epi == EPI_BF16
        (d, m), mx = pack_rows(W)
        assert mx == w12.CAP and int(w12.exceptions_per_block(m[:(N // 16) * w12.META])[nb]) == w12.CAP
        out[0] = dict(w12=d, meta=m, n=N, k=K, w=W, maxexc=mx)
    return out


def ragged_case(K, counts, dev, seed, int_data=False):
    """Activations, a permuted gather list with per-group row offsets and device-side counts: every activation row outside the gather
    list is NaN.  Group g reads list entries [off_g, off_g + count_g) and writes output rows 2 + off_g + r."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    total = sum(counts)
    RA = 2 * total + 11
    lda = K + 8
    a = torch.full((RA, lda), float("nan"), dtype=bf16)
    pick = torch.randperm(RA, generator=gen)[:total]
    vals = torch.randint(-4, 5, (total, K), generator=gen).to(bf16) if int_data else torch.randn((total, K), generator=gen).to(bf16)
    a[pick, :K] = vals
    lead = 3
    picked = set(pick.tolist())
    unused = [r for r in range(RA) if r not in picked][:lead]
    rows = torch.cat([torch.tensor(unused, dtype=torch.int64), pick]).to(torch.int32)
    offs, o = [], lead
    for c in counts:
        offs.append(o)
        o += c
    return dict(a=a.to(dev), rows=rows.to(dev), offs=offs, counts=counts, vals=vals,
                row_off=[torch.tensor([x], dtype=torch.int32, device=dev) for x in offs],
                count=[torch.tensor([c], dtype=torch.int32, device=dev) for c in counts])


def launch_pair(epi, N, ws, case, dev, reference=True, ref_chunk=None):
    """the WP12 launch and (reference) umoe_tiled_gemm on the row-major weights -> (out_w12, out_bf16, written mask).  ref_chunk: the
    reference runs in launches of at most that many rows per group (max_rows < 1024: always tgemm_kernel's 128-token tiles)."""
    from unimoe_audio_amd import ops
    total_rows = 2 + case["offs"][-1] + case["counts"][-1] + 5
    ldo = N + 8
    out = torch.full((total_rows, ldo), SENT, dtype=bf16, device=dev)
    groups = [dict(rows=case["rows"], row_off=case["row_off"][g], count=case["count"][g], out_row_base=2, w12=w["w12"], meta=w["meta"], n=w["n"], k=w["k"])
              for g, w in enumerate(ws)]
    ops.tiled_gemm_w12(groups, case["a"], out, max_rows=max(case["counts"]), epilogue=epi)
    ref = None
    if reference:
        ref = torch.full((total_rows, ldo), SENT, dtype=bf16, device=dev)
        step = ref_chunk or max(max(case["counts"]), 1)
        for lo in range(0, max(max(case["counts"]), 1), step):
            groups = []
            for g, w in enumerate(ws):
                c = max(0, min(step, case["counts"][g] - lo))
                groups.append(dict(rows=case["rows"], row_off=torch.tensor([case["offs"][g] + lo], dtype=torch.int32, device=dev),
                                   count=torch.tensor([c], dtype=torch.int32, device=dev), out_row_base=2, w=w["w"], w2=w.get("w2")))
            ops.tiled_gemm(groups, case["a"], ref, max_rows=step, epilogue=epi)
    torch.cuda.synchronize()
    written = torch.zeros((total_rows, ldo), dtype=torch.bool)
    for off, c in zip(case["offs"], case["counts"]):
        written[2 + off: 2 + off + c, :N] = True
    return out.cpu(), (ref.cpu() if reference else None), written


def check_written(got, written, what):
    assert bool((got[~written].float() == SENT).all()), f"{what}: a row or column outside the groups changed"
    assert bool(torch.isfinite(got[written].float()).all()), f"{what}: NaN / inf in a group's output (poison was read or patched in)"
    assert bool((got[written].float() != SENT).any()) or not bool(written.any())


KS = [32, 64, 512, 1376, 2048]          # one K tile and less, KB 43 (odd: 1-step chunks; Q = 344 straddles K tiles), the production width
NS = [16, 80, 128, 272]                 # one block, a ragged last tile, a tile edge, three tile rows with 16 rows in the last


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("epi", [EPI_SWIGLU, EPI_BF16])
def test_w12_tiled_gemm_is_bit_identical_to_the_bf16_kernel_on_the_same_weights(dev, epi, K):
    """N(0, 0.02^2) weights; three groups in one launch with device-side counts {0, 5, rows}, a permuted gather list and row offsets; poison
    behind the last block, NaN in every activation row outside the list, a sentinel in the output.  N = 40 (BF16 epilogue): a last block
    whose rows >= N hold NaN exceptions."""
    for N in NS + ([40] if epi == EPI_BF16 else []):
        ws = make_groups(epi, K, N, 3, dev, seed=1000 * K + N + epi)
        for rows in ((1, 63, 300) if N != 128 else (17, 129)):
            case = ragged_case(K, [0, min(5, rows), rows], dev, seed=K + N + rows)
            got, ref, written = launch_pair(epi, N, ws, case, dev)
            what = f"epi {epi} K {K} N {N} rows {rows}"
            check_written(got, written, what)
            assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), what


@pytest.mark.parametrize("epi", [EPI_SWIGLU, EPI_BF16])
def test_w12_tiled_gemm_at_the_production_down_width(dev, epi):
    """K = 2752 once (KB 86: 2-step chunks, 43 K tiles of 64), with planted exceptions"""
    ws = make_groups(epi, 2752, 272, 2, dev, seed=77 + epi, plant=True)
    case = ragged_case(2752, [40, 130], dev, seed=9)
    got, ref, written = launch_pair(epi, 272, ws, case, dev)
    check_written(got, written, "K 2752")
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16))


@pytest.mark.parametrize("K,N", [(32, 16), (64, 16), (512, 80), (512, 128), (1376, 272), (2048, 272)])
@pytest.mark.parametrize("epi", [EPI_SWIGLU, EPI_BF16])
def test_w12_tiled_gemm_with_planted_exceptions(dev, epi, K, N):
    """0.0, 2^-30 and 8.0 planted by plant_plan (its docstring lists the places); with the natural exceptions every block stays under the
    cap and pack returned a pack (pack_rows asserts it, and that unpack gives the matrix back).  BF16, N = 128: one block is topped up to
    exactly 32 exceptions.  8.0 among weights of 0.02 moves an output by hundreds of ulps: a patch that misses is seen."""
    full = epi == EPI_BF16 and N == 128
    ws = make_groups(epi, K, N, 3, dev, seed=31 * K + N + epi, plant=True, full=full)
    assert max(w["maxexc"] for w in ws) > 4 and (not full or ws[0]["maxexc"] == 32)
    for rows in (5, 130):
        case = ragged_case(K, [0, min(5, rows), rows], dev, seed=K + N + rows + 1)
        got, ref, written = launch_pair(epi, N, ws, case, dev)
        what = f"epi {epi} K {K} N {N} rows {rows}"
        check_written(got, written, what)
        assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), what


@pytest.mark.parametrize("name,epi,G,rows", [("tile256_swiglu", EPI_SWIGLU, 4, 1024), ("tile128_swiglu", EPI_SWIGLU, 4, 1023), ("tile256_bf16", EPI_BF16, 8, 1024)])
def test_w12_tiled_gemm_on_both_sides_of_the_tile_switch(dev, name, epi, G, rows):
    """N = 2048, K = 1376 with planted exceptions: at 1024 rows the WP12 call runs the 256-token tiles (K steps of 32; umoe_tgemm_tm), at
    1023 the 128-token ones.  The yardstick is tgemm_kernel: the reference runs in launches of 512 rows, which never take the 256 x 256
    ping-pong kernel (that one promises equality with tgemm_kernel only up to summation order)."""
    K, N = 1376, 2048
    ws = make_groups(epi, K, N, G, dev, seed=5 + epi, plant=True)
    case = ragged_case(K, [rows] * G, dev, seed=5)
    got, ref, written = launch_pair(epi, N, ws, case, dev, ref_chunk=512)
    check_written(got, written, name)
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), name


@pytest.mark.parametrize("name,K,N,G,rows", [("tail", 1376, 144, 3, 300), ("tile256", 64, 2048, 8, 1024), ("one_granule", 32, 48, 3, 17)])
def test_w12_tiled_gemm_equals_an_exact_float64_product(dev, name, K, N, G, rows):
    """Activations in -4 .. 4, weights k / 16 with 1 <= |k| <= 4 (a zero would be an exception, and a ninth of a matrix is over the cap:
    zeros are replaced by 1 / 16): every product and partial sum is exact in fp32 in any order, so the bf16 output must equal the
    rounded float64 product with no tolerance.  Pins the addressing and both tile heights independently of the bf16 kernel."""
    gen = torch.Generator(device="cpu").manual_seed(K + N)
    ws, wref = [], []
    for _ in range(G):
        wi = torch.randint(-4, 5, (N, K), generator=gen).float()
        wi = torch.where(wi == 0, torch.ones_like(wi), wi) / 16
        (d, m), _ = pack_rows(wi.to(bf16).to(dev))
        ws.append(dict(w12=d, meta=m, n=N, k=K))
        wref.append(wi.double())
    counts = [0, min(5, rows), rows] if G == 3 else [rows] * G
    case = ragged_case(K, counts, dev, seed=K, int_data=True)
    got, _, written = launch_pair(EPI_BF16, N, ws, case, dev, reference=False)
    check_written(got, written, name)
    o = 0
    for g, c in enumerate(counts):
        want = (case["vals"][o:o + c].double() @ wref[g].T).to(bf16)
        o += c
        rs = slice(2 + case["offs"][g], 2 + case["offs"][g] + c)
        assert torch.equal(got[rs, :N].view(torch.int16), want.view(torch.int16)), (name, g)


def test_w12_tiled_gemm_refuses_what_it_does_not_do(dev):
    """every refusal names the argument and leaves the output untouched (nothing launched)"""
    from unimoe_audio_amd import _lib as L, ops
    w = make_groups(EPI_BF16, 32, 16, 1, dev, seed=1)[0]
    a = torch.ones(8, 40, dtype=bf16, device=dev)
    out = torch.full((8, 16), SENT, dtype=bf16, device=dev)
    aux = torch.zeros(8, 32, dtype=bf16, device=dev)
    one = torch.zeros(16, dtype=torch.float32, device=dev)
    ki = torch.zeros(1, dtype=torch.int32, device=dev)
    g = dict(w12=w["w12"], meta=w["meta"], n=16, k=32, static_count=8)
    cases = [(dict(g, k=40), EPI_BF16, {}, "k % 32"), (g, 1, {}, "epilogue"), (g, 3, {}, "epilogue"), (dict(g, n=24), EPI_SWIGLU, {}, "n % 16"),
             (dict(g, w_kmajor=1), EPI_BF16, {}, "w_kmajor"), (dict(g, k_off=ki, k_count=ki), EPI_BF16, {}, "k_off"), (dict(g, bias=one), EPI_BF16, {}, "bias"),
             (g, EPI_SWIGLU, dict(aux_out=aux), "aux_out"), (dict(g, k=127 * 32), EPI_BF16, {}, "k / 32 < 127"),
             (dict(g, w12=None), EPI_BF16, {}, "host_w12"), (dict(g, meta=None), EPI_BF16, {}, "host_meta"),
             (dict(g, w12=w["w12"][8:]), EPI_BF16, {}, "host_w12"), (dict(g, meta=w["meta"].view(torch.uint8)[2:]), EPI_BF16, {}, "host_meta")]
    for bad, epi, kw, msg in cases:
        with pytest.raises(L.UmoeError) as err:
            ops.tiled_gemm_w12([bad], a, out, max_rows=8, epilogue=epi, **kw)
        assert "umoe_tiled_gemm_w12" in str(err.value) and msg in str(err.value), (msg, str(err.value))
    torch.cuda.synchronize()
    assert bool((out.float() == SENT).all())


# ------------------------------------------------------------------------------------------------ engine
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
    """prefill + `steps` sampled decode steps of a fresh engine -> tokens, state, router masks, top-k, logits (after the first and the last
    step), per-layer router logits of an eager probe step, info"""
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    from unimoe_audio_amd.model import DecodeEngine
    ids, am, codec = prompt(cfg, B, T, pseed)
    eng = DecodeEngine(m, B, Lmax=T + steps + 80, Tmax=steps + 72, expert_weights=fmt)
    x = m.calculate_input_embedding(ids.to(dev), codec.to(dev))
    eng.prefill(x.reshape(-1, cfg.hidden_size).contiguous(), am.to(dev))
    out = dict(prefill_w12=eng.info("prefill_w12"), bf16_resident=eng.info("expert_bf16_resident"), fmt=eng.expert_weights,
               only_layers=eng.info("w12_only_layers"))
    pre, psteps = prepare_audio_prompt(cfg, [None] * B)
    eng.start_decode(pre, psteps, steps + 8, 4, cfg_scale=2.0, temperature=1.0, top_p=0.9, top_k=45, eos_mul=0.8, do_sample=True, seed=3)
    E = cfg.num_experts
    for i in range(steps):
        eng.step(use_graph)
        if i == 0:
            out["logits0"] = eng.copy_buffer("logits", torch.float32, (2 * B, cfg.codec_channels * cfg.codec_vocab_size)).cpu()
            out["mask0"] = eng.copy_buffer("all_mask", torch.int32, (cfg.num_hidden_layers, 2 * B, E)).cpu()
    torch.cuda.synchronize()
    out.update(tokens=eng.tokens.cpu().clone(), state=eng.state.cpu().clone(),
               mask=eng.copy_buffer("all_mask", torch.int32, (cfg.num_hidden_layers, 2 * B, E)).cpu(),
               topk=eng.copy_buffer("all_topk", torch.int64, (cfg.num_hidden_layers, 2 * B)).cpu(),
               logits=eng.copy_buffer("logits", torch.float32, (2 * B, cfg.codec_channels * cfg.codec_vocab_size)).cpu())
    out["expert_w12"] = eng.info("expert_w12")
    out["expert_launch"] = eng.info("expert_launch")
    probe = eng.set_probe(dump_logits=True)
    eng.step(False)
    torch.cuda.synchronize()
    out["router_logits"] = probe["logits"].cpu().clone()
    eng.set_probe()
    out["handoff"] = eng.handoff_error()
    eng.close()
    return out


@pytest.fixture(scope="module")
def host_model():
    cfg = ref_cfg()
    return build(cfg, 31), cfg


def fresh(host_model, dev):
    return copy.deepcopy(host_model[0]).to(dev)


@pytest.fixture(scope="module")
def pair(dev, host_model):
    """the 2-layer model at the reference width twice on the device: as it is, and released to w12-only"""
    from unimoe_audio_amd import quant
    cfg = host_model[1]
    a, b = fresh(host_model, dev), fresh(host_model, dev)
    b.quantize_experts_("w12", keep_bf16=False)
    assert quant.expert_format(b) == "w12-only" and quant.is_released(b)
    assert all(p.numel() == 0 for layer in b.language_model.layers for grp in quant.expert_modules(layer) for x in grp for p in x.parameters())
    yield a, b, cfg
    del a, b
    torch.cuda.empty_cache()


KEYS = ("tokens", "state", "mask", "topk", "logits", "logits0", "router_logits")


@pytest.mark.parametrize("B,T", [(1, 32), (3, 12), (8, 12), (9, 12), (16, 12)])
def test_w12_only_engine_is_bit_identical_to_the_default_bf16_engine(dev, pair, B, T, monkeypatch):
    """Prefill of 64 / 72 / 192 / 216 / 384 rows (MOE_TILED in both: the WP12 tiles against the bf16 tiles) and 5 sampled steps, eager and
    through the step graph: the flat launch at B <= 8, the wide form at B = 9 (the bf16 leg with UMOE_WIDE_DECODE=1: both legs the wide
    form, which the wide suites show equal to the ragged one) and at B = 16."""
    a_m, b_m, cfg = pair
    if B == 9:
        monkeypatch.setenv("UMOE_WIDE_DECODE", "1")
    for use_graph in (False, True):
        a = run_engine(a_m, cfg, B, "bf16", 5, use_graph, dev, T=T)
        b = run_engine(b_m, cfg, B, "w12-only", 5, use_graph, dev, T=T)
        assert (a["prefill_w12"], a["bf16_resident"], a["fmt"], a["only_layers"]) == (0, 1, "bf16", 0)
        assert (b["prefill_w12"], b["bf16_resident"], b["fmt"], b["only_layers"]) == (1, 0, "w12-only", cfg.num_hidden_layers)
        assert a["handoff"] == 0 and b["handoff"] == 0 and b["expert_w12"] == 1
        assert a["expert_launch"] == b["expert_launch"] == (2 if B <= 8 else 4)
        for k in KEYS:
            assert torch.equal(a[k], b[k]), (k, B, use_graph)


def test_w12_only_serving_with_admissions_gives_equal_codes(dev, pair):
    """6 slots (12 rows, the flat launch), one captured step graph: four requests admitted (80-row admission prefills), the slot of the
    shortest one reused by a fifth."""
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    from unimoe_audio_amd.model import DecodeEngine
    a_m, b_m, cfg = pair
    T = 40
    pre, ps = prepare_audio_prompt(cfg, [None])
    base = dict(cfg_scale=2.0, temperature=1.0, top_p=0.9, top_k=45, eos_mul=0.8, do_sample=True, min_tokens=4)
    reqs = [dict(seed=3 + i, max_tokens=mt) for i, mt in enumerate((12, 5, 9, 14, 7))]
    res = {}
    for fmt, m in (("bf16", a_m), ("w12-only", b_m)):
        xs = []
        for i in range(len(reqs)):
            ids, am, codec = prompt(cfg, 1, T, 20 + i)
            xs.append((m.calculate_input_embedding(ids.to(dev), codec.to(dev)).reshape(-1, cfg.hidden_size).contiguous(), am))
        eng = DecodeEngine(m, 6, Lmax=T + 120, Tmax=96, expert_weights=fmt)
        eng.start_serving(T)
        slot_of, got, pf = {}, {}, []
        for i in range(4):
            eng.admit(i + 1, xs[i][0], xs[i][1], pre[0], ps[0], **base, **reqs[i])
            pf.append(eng.info("prefill_w12"))
            slot_of[i + 1] = i
        n = 0
        while slot_of:
            eng.step(True)
            n += 1
            assert n < 300
            st = eng.poll()
            for b in list(slot_of):
                if eng.row_done(st, b):
                    r = slot_of.pop(b)
                    codes, length = eng.take(b)
                    got[r] = (codes.cpu(), length)
                    if r == 1:                                   # the reused row
                        eng.admit(b, xs[4][0], xs[4][1], pre[0], ps[0], **base, **reqs[4])
                        slot_of[b] = 4
        res[fmt] = (got, pf, eng.info("expert_w12"))
        eng.close()
    assert res["bf16"][1] == [0] * 4 and res["w12-only"][1] == [1] * 4 and res["w12-only"][2] == 1
    assert sorted(res["bf16"][0]) == sorted(res["w12-only"][0]) == list(range(5))
    for r in range(5):
        assert res["bf16"][0][r][1] == res["w12-only"][0][r][1] and torch.equal(res["bf16"][0][r][0], res["w12-only"][0][r][0]), r


def rel_l2(a, b):
    return float((a - b).norm() / b.norm())


def test_short_prefill_differs_only_by_summation_order(dev, pair, monkeypatch):
    """B = 1, T = 12 (24 rows): the w12-only engine runs MOE_TILED on WP12, the bf16 engine MOE_RAGGED on WP16 -- the same weights, another
    fp32 summation order.  Bound: the relative L2 of the first step's logits between the tiled and the ragged prefill of the bf16 engine
    itself (UMOE_TILED_PREFILL=1 against =0), measured here.  A bf16 engine cannot run its experts tiled under 64 rows, so the yardstick
    is taken at B = 3 (72 rows), on another prompt than the compared value; therefore the w12-only engine is ALSO compared at that same
    B = 3 prompt against the bf16 engine forced ragged, where bound and value come from one input (and are equal: the WP12 tiles are
    bit-identical to the bf16 tiles).  The router masks must be equal.
    Measured on MI355X: w12-only against bf16 at B = 1 0.0049, the bound 0.0506; the masks are equal."""
    a_m, b_m, cfg = pair
    a = run_engine(a_m, cfg, 1, "bf16", 1, False, dev)
    b = run_engine(b_m, cfg, 1, "w12-only", 1, False, dev)
    assert a["prefill_w12"] == 0 and b["prefill_w12"] == 1
    b3 = run_engine(b_m, cfg, 3, "w12-only", 1, False, dev)
    monkeypatch.setenv("UMOE_TILED_PREFILL", "1")
    y1 = run_engine(a_m, cfg, 3, "bf16", 1, False, dev)
    monkeypatch.setenv("UMOE_TILED_PREFILL", "0")
    y0 = run_engine(a_m, cfg, 3, "bf16", 1, False, dev)
    monkeypatch.delenv("UMOE_TILED_PREFILL")
    got, yard = rel_l2(b["logits0"], a["logits0"]), rel_l2(y1["logits0"], y0["logits0"])
    got3 = rel_l2(b3["logits0"], y0["logits0"])
    rec = {"w12only_vs_bf16_rel_l2_B1": got, "w12only_vs_bf16_ragged_rel_l2_B3": got3, "yardstick_bf16_tiled_vs_ragged_rel_l2_B3": yard,
           "masks_equal": bool(torch.equal(a["mask0"], b["mask0"])), "masks_equal_B3": bool(torch.equal(b3["mask0"], y0["mask0"]))}
    print("short prefill:", json.dumps(rec))
    assert rec["masks_equal"] and rec["masks_equal_B3"]
    assert got <= yard, rec
    assert got3 <= yard, rec


def over_the_cap_(m, layer):
    """33 zeros in one 16-row block of one down projection: the layer is not packable"""
    w = m.language_model.layers[layer].mlp.fixed_real_moe[1].down_proj.weight
    with torch.no_grad():
        w[16:18, :17] = 0.0
        assert int((w[16:32] == 0).sum()) >= 33


def test_a_layer_over_the_cap_gives_a_mixed_engine(dev, host_model, monkeypatch):
    """layer 1 keeps its bf16 weights and its paths (the WP16 flat launch, the WP16 wide launches, the bf16 tiles), layer 0 is w12-only;
    B = 9: the bf16 leg with UMOE_WIDE_DECODE=1, as above"""
    from unimoe_audio_amd import quant
    cfg = host_model[1]
    a, b = fresh(host_model, dev), fresh(host_model, dev)
    over_the_cap_(a, 1)
    over_the_cap_(b, 1)
    b.quantize_experts_("w12", keep_bf16=False)
    rel = [all(p.numel() == 0 for grp in quant.expert_modules(layer) for x in grp for p in x.parameters()) for layer in b.language_model.layers]
    kept = [all(p.numel() > 0 for grp in quant.expert_modules(layer) for x in grp for p in x.parameters()) for layer in b.language_model.layers]
    assert rel == [True, False] and kept == [False, True]
    for B in (3, 9):
        if B == 9:
            monkeypatch.setenv("UMOE_WIDE_DECODE", "1")
        ra = run_engine(a, cfg, B, "bf16", 4, True, dev)
        rb = run_engine(b, cfg, B, "w12-only", 4, True, dev)
        assert rb["only_layers"] == cfg.num_hidden_layers - 1 and rb["bf16_resident"] == 1 and rb["prefill_w12"] == 1
        for k in KEYS:
            assert torch.equal(ra[k], rb[k]), (k, B)
    del a, b
    torch.cuda.empty_cache()


def expert_elems(cfg):
    D, Id, Is = cfg.hidden_size, cfg.dynamic_intermediate_size, cfg.shared_intermediate_size
    return cfg.num_hidden_layers * 3 * D * (cfg.mlp_dynamic_expert_num * Id + cfg.mlp_fixed_expert_num * Is)


def test_w12_only_holds_the_wp12_copies_and_nothing_else(dev, host_model, monkeypatch):
    """torch.cuda.memory_allocated() differences.  The w12-only leg: the model arrives on the device (its expert parameters hold
    `par` bytes: sizes that are multiples of 512 bytes, allocated from an empty cache), is released, and gets its engine.  The allocated
    bytes attributable to experts are par + (after the release - before it), plus whatever expert bytes the engine build adds -- bounded
    by the same engine build on the bf16 model (UMOE_FLAT_W12=0: no WP12 copies), which adds the WP16 packs (as many bytes as the
    parameters) to the same non-expert allocations.  They must equal the sum of the WP12 tensors within 1 %."""
    from unimoe_audio_amd import quant
    from unimoe_audio_amd.model import DecodeEngine
    cfg = host_model[1]
    P = expert_elems(cfg)

    def alloc():
        gc.collect()
        torch.cuda.synchronize()
        return torch.cuda.memory_allocated()

    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    m = fresh(host_model, dev)
    par = sum(p.numel() * p.element_size() for layer in m.language_model.layers for grp in quant.expert_modules(layer) for x in grp for p in x.parameters())
    assert par == 2 * P
    a0 = alloc()
    monkeypatch.setenv("UMOE_FLAT_W12", "0")
    eng = DecodeEngine(m, 2, Lmax=64, Tmax=64, expert_weights="bf16")
    monkeypatch.delenv("UMOE_FLAT_W12")
    assert eng.info("expert_bf16_resident") == 1
    a1 = alloc()
    eng.close()
    del eng, m
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    m = fresh(host_model, dev)
    b0 = alloc()
    m.quantize_experts_("w12", keep_bf16=False)
    b1 = alloc()
    w12_bytes = sum(t.numel() * t.element_size() for layer in m.language_model.layers for k in ("gu", "dn") for pr in quant.w12_layer_copies(layer)[k] for t in pr)
    eng = DecodeEngine(m, 2, Lmax=64, Tmax=64)
    assert eng.expert_weights == "w12-only" and eng.info("expert_bf16_resident") == 0
    b2 = alloc()
    eng.close()
    del eng, m
    torch.cuda.empty_cache()
    engine_bf16, engine_w12 = a1 - a0, b2 - b1             # engine_bf16 = the non-expert allocations + the WP16 packs (par bytes)
    experts = par + (b1 - b0) + max(0, engine_w12 - (engine_bf16 - par))
    print("expert elements", P, "parameters", par, "released model", b1 - b0, "engine bf16 / w12-only", engine_bf16, engine_w12,
          "expert bytes of the w12-only leg", experts, "WP12 tensors", w12_bytes)
    assert abs(experts - w12_bytes) <= 0.01 * w12_bytes, (experts, w12_bytes)
    assert engine_w12 <= engine_bf16 - 0.99 * par, (engine_w12, engine_bf16)      # no WP16 pack of an expert was built
    assert 1.49 * P <= w12_bytes <= 1.52 * P


def test_a_model_released_on_the_host_and_moved_decodes_the_same(dev, host_model, pair):
    """The WP12 copies sit in a plain dict on the expert modules, which nn.Module.to() does not move: packed_w12() moves them to the
    model's device, and the engine gets device pointers."""
    from unimoe_audio_amd import quant
    cfg = host_model[1]
    m = copy.deepcopy(host_model[0])
    m.quantize_experts_("w12", keep_bf16=False)
    assert all(t.device.type == "cpu" for layer in m.language_model.layers for k in ("gu", "dn") for pr in quant.w12_layer_copies(layer)[k] for t in pr)
    m = m.to(dev)
    copies = m.packed_w12()
    assert all(t.device == next(m.parameters()).device for c in copies for k in ("gu", "dn") for pr in c[k] for t in pr)
    a = run_engine(pair[1], cfg, 3, "w12-only", 3, True, dev)
    b = run_engine(m, cfg, 3, "w12-only", 3, True, dev)
    assert b["only_layers"] == cfg.num_hidden_layers and b["prefill_w12"] == 1
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    del m
    torch.cuda.empty_cache()


def test_w12_only_refuses_every_path_that_would_stream_bf16_expert_weights(dev, pair, monkeypatch):
    from unimoe_audio_amd import _lib as L
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    from unimoe_audio_amd.model import DecodeEngine
    a_m, m, cfg = pair
    MISSING = "no bf16 expert weights"

    def prompt_x(B):
        ids, am, codec = prompt(cfg, B, 12, 4)
        return m.calculate_input_embedding(ids.to(dev), codec.to(dev)).reshape(-1, cfg.hidden_size).contiguous(), am.to(dev)

    # the module forward, saving, engines that want the bf16 weights, and the no-op format
    x, am = prompt_x(2)
    with pytest.raises(L.UmoeError, match="dequantize_experts_"):
        m.text_forward(x.view(4, 12, -1), am)
    with pytest.raises(L.UmoeError, match="dequantize_experts_"):
        m.state_dict()
    for fmt in ("bf16", "fp8"):
        with pytest.raises(L.UmoeError, match="dequantize_experts_"):
            DecodeEngine(m, 2, Lmax=100, Tmax=80, expert_weights=fmt)
    with pytest.raises(L.UmoeError, match="nothing to do"):
        a_m.quantize_experts_("w12", keep_bf16=True)
    # switches read at engine creation: the prefill (UMOE_TILED_PREFILL) or the first step (UMOE_FUSE_ROUTER, a CU count without a
    # schedule) is refused on the host
    monkeypatch.setenv("UMOE_TILED_PREFILL", "0")
    eng = DecodeEngine(m, 2, Lmax=100, Tmax=80)
    assert eng.expert_weights == "w12-only"
    with pytest.raises(L.UmoeError, match=MISSING):
        eng.prefill(x, am)
    eng.close()
    monkeypatch.delenv("UMOE_TILED_PREFILL")
    pre, psteps = prepare_audio_prompt(cfg, [None] * 2)
    dk = dict(cfg_scale=2.0, temperature=1.0, top_p=0.9, top_k=45, eos_mul=0.8, do_sample=True, seed=3)
    for var, val in (("UMOE_FUSE_ROUTER", "0"), ("UMOE_FAKE_CUS", "100")):
        monkeypatch.setenv(var, val)
        eng = DecodeEngine(m, 2, Lmax=100, Tmax=80)
        monkeypatch.delenv(var)
        eng.prefill(x, am)
        eng.start_decode(pre, psteps, 16, 4, **dk)
        tok = eng.tokens.cpu().clone()
        for use_graph in (False, True):
            with pytest.raises(L.UmoeError, match=MISSING):
                eng.step(use_graph)
        torch.cuda.synchronize()
        assert torch.equal(eng.tokens.cpu(), tok), var
        eng.close()
    # switches read per enqueue, up to 16 rows
    eng = DecodeEngine(m, 2, Lmax=100, Tmax=80)
    eng.prefill(x, am)
    eng.start_decode(pre, psteps, 16, 4, **dk)
    tok = eng.tokens.cpu().clone()
    for var in ("UMOE_FLAT_MOE", "UMOE_FLAT_W12"):
        monkeypatch.setenv(var, "0")
        for use_graph in (False, True):
            with pytest.raises(L.UmoeError, match=MISSING):
                eng.step(use_graph)
        monkeypatch.delenv(var)
    torch.cuda.synchronize()
    assert torch.equal(eng.tokens.cpu(), tok)
    eng.step(True)                                               # and with nothing set it decodes
    torch.cuda.synchronize()
    assert not torch.equal(eng.tokens.cpu(), tok) and eng.info("expert_w12") == 1
    eng.close()
    # above 16 rows
    x9, am9 = prompt_x(9)
    pre9, ps9 = prepare_audio_prompt(cfg, [None] * 9)
    eng = DecodeEngine(m, 9, Lmax=100, Tmax=80)
    eng.prefill(x9, am9)
    eng.start_decode(pre9, ps9, 16, 4, **dk)
    tok = eng.tokens.cpu().clone()
    for var in ("UMOE_WIDE_DECODE", "UMOE_WIDE_W12"):
        monkeypatch.setenv(var, "0")
        for use_graph in (False, True):
            with pytest.raises(L.UmoeError, match=MISSING):
                eng.step(use_graph)
        monkeypatch.delenv(var)
    torch.cuda.synchronize()
    assert torch.equal(eng.tokens.cpu(), tok)
    eng.close()


def test_w12_only_refuses_more_than_12_groups_and_expert_parallel(dev):
    """11 routed + 2 shared experts: the tiled launch has 12 groups, MOE_RAGGED would stream WP16 packs.  (A small width: the refusal comes
    before anything is enqueued.)"""
    from unimoe_audio_amd import _lib as L
    from unimoe_audio_amd.config import UniMoEAudioConfig
    from unimoe_audio_amd.model import DecodeEngine
    cfg = UniMoEAudioConfig(hidden_size=256, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=1, vocab_size=320,
                            dynamic_intermediate_size=64, shared_intermediate_size=32, codec_placeholder_value=300, mlp_dynamic_expert_num=11)
    m = build(cfg, 5, std=0.05).to(dev)
    m.quantize_experts_("w12", keep_bf16=False)
    ids, am, codec = prompt(cfg, 2, 20, 4)
    x = m.calculate_input_embedding(ids.to(dev) % cfg.vocab_size, None).reshape(-1, cfg.hidden_size).contiguous()
    eng = DecodeEngine(m, 2, Lmax=100, Tmax=80)
    assert eng.info("w12_only_layers") == cfg.num_hidden_layers
    with pytest.raises(L.UmoeError, match="no bf16 expert weights"):
        eng.prefill(x, am.to(dev))
    eng.close()

    class FakeLink:
        size, rank = 2, 0
    with pytest.raises(L.UmoeError, match="expert parallel"):
        DecodeEngine(m, 2, Lmax=100, Tmax=80, ep=FakeLink())
