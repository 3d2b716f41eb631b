"""GPU suite of the fp8 form of the wide decode step: umoe_gemm_wide_fp8 streams WP8 expert weights for 17..64 rows, and an fp8
engine of 9 to 32 requests decodes with it.

q * 2^e is exact in bf16, so bit-identity is the only criterion: the kernel against umoe_gemm_wide on the dequantized weights W_deq, the
engine against the bf16 engine of the same (quantized) model, serving against bf16 serving with the same plan.  No tolerance anywhere.

Kernel shapes: rows 18 / 32 / 34 / 48 / 64; gate/up at K 2048 (64 k-steps: wave slices of 4 whole 16-byte chunks); down at K 2752 (86
k-steps, even: 16-byte loads), at K 1376 (43, odd: one 8-byte load per k-step, slices start on either half of a chunk) and with both kinds
of group in one launch.  Guards of every run: e4m3 NaN (0x7F) in the WP8 blocks behind n_blocks and in the unused half of the last chunk of
every K quarter at K 1376 (zero by the format -- NaN there proves that no padded k-step reaches an MFMA), exponent 127 behind the last
block's exponents, and the sentinels and NaN pad rows of test_gpu_wide_gemm."""
import functools

import pytest
import torch

from test_gpu_wide_gemm import BF16, EPIS, F32, NAN, RESID, ROWS, SENT, SWIGLU, bits, check_fp64, check_guards, make, run_wide
from test_gpu_wide_decode import GREEDY, LMAX, ROW, SAMPLED, T, TMAX, run, same_request, serve_run

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
F8_NAN = 0x7F


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from unimoe_audio_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ kernel
def quantize_case(c):
    """every weight of the case -> (q, e) in q["q8"], and W_deq in its place: run_wide then runs the reference on W_deq"""
    from unimoe_audio_amd import quant
    for q in c["groups"]:
        q["q8"] = [quant.quantize_fp8_rows(w.float()) for w in q["w"]]
        q["w"] = [quant.dequantize_fp8_rows(*p) for p in q["q8"]]
    return c


def gauss(name, rows, ks, nbs, seed):
    """a case in the layout of test_gpu_wide_gemm.make with the K and n_blocks of every group given; row r of a weight is scaled by
    2^((r % 7) - 3), so the row exponents differ within a block"""
    epi, waves, u = EPIS[name][:3]
    g = torch.Generator().manual_seed(seed)
    groups = []
    for k, nb in zip(ks, nbs):
        N = 8 * nb if epi == SWIGLU else 16 * nb
        A = torch.randn(rows, k, generator=g).to(bf16)
        ws = [(torch.randn(N, k, generator=g) * k ** -0.5 * torch.exp2((torch.arange(N) % 7 - 3).float())[:, None]).to(bf16)
              for _ in range(2 if epi == SWIGLU else 1)]
        groups.append(dict(k=k, nb=nb, N=N, A=A, w=ws, bias=None, resid=None))
    c = quantize_case(dict(name=name, epi=epi, waves=waves, u=u, rows=rows, groups=groups, n_valid=16 * max(nbs)))
    assert all(len(set(p[1][:16].tolist())) > 1 for q in c["groups"] for p in q["q8"])
    return c


def run_wide_fp8(c, dev, call=None):
    """run_wide of test_gpu_wide_gemm on the WP8 weights, every guard in place -> per group the output buffer (with its margins)"""
    from unimoe_audio_amd import ops, quant
    rows, epi = c["rows"], c["epi"]
    tiles = (rows + 15) // 16
    ws, es, bs, outs = [], [], [], []
    ldo = 16 * max(q["nb"] for q in c["groups"]) + 12          # ldo > N: a gap behind every row
    for q in c["groups"]:
        k, nb = q["k"], q["nb"]
        KB2 = (k // 32 + 1) // 2
        pairs = [(a.to(dev), b.to(dev)) for a, b in q["q8"]]
        wp, ex = quant.pack_wp8_gate_up(*pairs[0], *pairs[1]) if epi == SWIGLU else quant.pack_wp8(*pairs[0])
        assert wp.numel() == nb * KB2 * 1024 and ex.numel() == nb * 16
        if (k // 32) % 2:                                        # the half-used last chunk of every K quarter
            last = wp.view(nb, KB2, 64, 16)[:, -1, :, 8:]
            assert bool((last == 0).all())
            last.fill_(F8_NAN)
        wpad = torch.full((wp.numel() + 3 * KB2 * 1024,), F8_NAN, dtype=torch.uint8, device=dev)      # NaN blocks behind n_blocks
        wpad[:wp.numel()] = wp
        epad = torch.full((ex.numel() + 48,), 127, dtype=torch.int8, device=dev)                     # 2^127 behind the last block's exponents
        epad[:ex.numel()] = ex
        src = torch.full((tiles * 16 + 2, k + 8), NAN, dtype=bf16, device=dev)                       # NaN pad rows (and columns behind K) in the source
        src[:rows, :k] = q["A"].to(dev)
        b = torch.full((tiles * 16 * k + 64,), SENT, dtype=bf16, device=dev)
        ops.pack_rows(src[:rows, :k], out=b)
        q["packed"] = b
        if epi == SWIGLU:
            o = torch.full((tiles * 16 * q["N"] + 64,), SENT, dtype=bf16, device=dev)
        else:
            o = torch.full((tiles * 16 + 4, ldo), SENT, dtype=bf16, device=dev)
        ws.append(wpad); es.append(epad); bs.append(b); outs.append(o)
    if call is None:
        ops.gemm_wide_fp8(ws, es, [q["nb"] for q in c["groups"]], [q["k"] for q in c["groups"]], rows, bs, outs, epilogue=epi, waves=c["waves"],
                          u=c["u"], n_valid=None if epi == SWIGLU else c["n_valid"])
    else:
        call(ws, es, bs, outs)
    torch.cuda.synchronize()
    return [o.cpu() for o in outs]


# (launch, K per group, n_blocks per group)
KERNEL_CASES = [("gate_up", [2048, 2048, 2048], [12, 4, 20]), ("down", [2752, 2752, 2752], [3, 5, 1]), ("down", [1376, 1376, 1376], [3, 5, 1]),
                ("down", [2752, 1376, 2752], [3, 5, 1])]


@pytest.mark.parametrize("rows", ROWS)
def test_fp8_wide_bit_for_bit_against_the_bf16_wide_kernel_on_the_dequantized_weights(dev, rows):
    for n, (name, ks, nbs) in enumerate(KERNEL_CASES):
        c = gauss(name, rows, ks, nbs, 100 * rows + n)
        want = run_wide(c, dev)
        check_guards(c, want)
        got = run_wide_fp8(c, dev)
        check_guards(c, got)
        for q, o, w in zip(c["groups"], got, want):          # the whole buffers: results, pad rows, gaps and margins
            assert torch.equal(bits(o), bits(w)), (name, rows, ks, q["k"], int((bits(o) != bits(w)).sum()))


@pytest.mark.parametrize("rows", [34, 64])
def test_fp8_wide_exact_against_fp64(dev, rows):
    """the small-integer data of test_gpu_wide_gemm: weights k / 16 with |k| <= 4 are exact in e4m3, every product and sum exact in fp32"""
    for name, K, n_groups in [("gate_up", 2048, 1), ("down", 2752, 3), ("down", 1376, 3)]:
        c = make(name, rows, K, n_groups, "int", 3000 * rows + K)
        orig = [[w.clone() for w in q["w"]] for q in c["groups"]]
        quantize_case(c)
        assert all(torch.equal(bits(a), bits(b)) for q, ws in zip(c["groups"], orig) for a, b in zip(q["w"], ws))      # dequantize(quantize(W)) == W
        outs = run_wide_fp8(c, dev)
        check_guards(c, outs)
        check_fp64(c, outs)


def test_fp8_wide_refusals(dev):
    from unimoe_audio_amd import _lib, ops
    down = gauss("down", 64, [1376], [3], 1)                  # (buffers of 64 rows: every row count below fits them)
    gate = gauss("gate_up", 64, [2048], [4], 2)
    for c, rows, epi, waves, u, nb, drop_exps in [(down, 16, BF16, 8, 2, 3, False), (down, 65, BF16, 8, 2, 3, False), (down, 32, BF16, 8, 1, 3, False),
                                                  (down, 32, F32, 8, 2, 3, False), (down, 32, SWIGLU, 4, 1, 3, False), (down, 32, RESID, 4, 16, 3, False),
                                                  (gate, 32, SWIGLU, 8, 1, 3, False),          # 3 blocks: no gate/up fours
                                                  (down, 32, BF16, 8, 2, 3, True)]:
        def call(ws, es, bs, outs):
            with pytest.raises(_lib.UmoeError):
                ops.gemm_wide_fp8(ws, [None] if drop_exps else es, [nb], [c["groups"][0]["k"]], rows, bs, outs, epilogue=epi, waves=waves, u=u,
                                  n_valid=None if epi == SWIGLU else 16 * nb)
        for o in run_wide_fp8(c, dev, call):
            assert bool((o == SENT).all()), (rows, epi, waves, u, drop_exps)          # nothing was launched


# ------------------------------------------------------------------------------------------------ engine
@pytest.fixture(scope="module")
def world8(dev):
    """the two-layer full-width model with quantized experts (its parameters are W_deq) and the prompt pairs of 32 requests, as the world of
    test_gpu_wide_decode; one result cache per engine kind"""
    from test_gpu_engine import prompt
    from test_gpu_fp8 import build, ref_cfg
    cfg = ref_cfg()
    m = build(cfg, 41).to(dev)
    m.quantize_experts_("fp8")
    ids, am, codec = prompt(cfg, 32, T, 6, [3, 0, 1, 0, 2, 0, 0, 4] + [0] * 40 + [1, 2, 0, 5] + [0] * 12)
    with torch.no_grad():
        x = m.calculate_input_embedding(ids.to(dev), codec.to(dev)).reshape(64, T, cfg.hidden_size).contiguous()
    yield dict(m=m, cfg=cfg, x=x, am=am, dev=dev, cache={})
    if m._engine is not None:
        m._engine.close()


def run_kind(world8, monkeypatch, kind, reqs, steps, settings, graph, probe=False, fp8_wide=True):
    """test_gpu_wide_decode.run with the engine it builds of `kind` ("fp8": DecodeEngine(..., expert_weights="fp8", fp8_wide=fp8_wide)),
    plus the logits of the last step and expert_fp8"""
    import unimoe_audio_amd.model as M
    key = (kind, tuple(reqs), steps, settings["do_sample"], graph, probe, fp8_wide)
    if key in world8["cache"]:
        return world8["cache"][key]
    real = M.DecodeEngine

    def engine(m, B, **kw):
        kw.update(expert_weights=kind, fp8_wide=fp8_wide and kind == "fp8")
        return real(m, B, **kw)

    with monkeypatch.context() as mp:
        mp.setattr(M, "DecodeEngine", engine)
        out, eng = run(dict(world8, cache={}), reqs, steps, settings, graph, probe=probe, keep_engine=True)
    cfg = world8["cfg"]
    out["logits"] = eng.copy_buffer("logits", torch.float32, (2 * len(reqs), cfg.codec_channels * cfg.codec_vocab_size)).cpu()
    out["fp8"] = eng.info("expert_fp8")
    eng.close()
    world8["cache"][key] = out
    return out


def same_engine_output(a, b, what):
    for k in ("k", "v", "tokens", "state", "mask", "topk", "logits"):
        assert torch.equal(a[k], b[k]), (what, k)
    assert a["lengths"] == b["lengths"], what


@pytest.mark.parametrize("B,graph", [(16, False), (16, True), (24, False), (32, False), (9, False)], ids=["16-eager", "16-graph", "24", "32", "9"])
def test_fp8_wide_engine_equals_the_bf16_wide_engine_on_the_dequantized_weights(world8, monkeypatch, B, graph):
    if B == 9:
        monkeypatch.setenv("UMOE_WIDE_DECODE", "1")          # (the bf16 engine's default at this size is the ragged path)
    reqs = list(range(B))
    f8 = run_kind(world8, monkeypatch, "fp8", reqs, 6, SAMPLED, graph)
    ref = run_kind(world8, monkeypatch, "bf16", reqs, 6, SAMPLED, graph)
    assert f8["launch"] == 4 and f8["fp8"] == 1 and f8["tiles"] == (2 * B + 15) // 16 and f8["tiles"] in (2, 3, 4) and f8["handoff"] == 0
    assert ref["launch"] == 4 and ref["fp8"] == 0 and ref["tiles"] == f8["tiles"]
    same_engine_output(f8, ref, f"B={B}")
    assert len({tuple(f8["tokens"][b].flatten().tolist()) for b in range(B)}) > B // 4          # (the requests do differ)


def test_fp8_wide_per_layer_probe_and_the_flat_fp8_launch_of_the_first_eight(world8, monkeypatch):
    reqs = list(range(16))
    f8 = run_kind(world8, monkeypatch, "fp8", reqs, 1, GREEDY, False, probe=True)
    ref = run_kind(world8, monkeypatch, "bf16", reqs, 1, GREEDY, False, probe=True)
    assert f8["launch"] == 4 and f8["fp8"] == 1
    for name in ("x1", "logits", "x"):
        a, b = f8["probe"][name], ref["probe"][name]
        for layer in range(a.shape[0]):
            assert torch.equal(a[layer].view(torch.int16), b[layer].view(torch.int16)), (name, layer)
    # requests 0..7 of the batch of 16 against the same requests in a batch of 8: the fp8 flat launch
    big = run_kind(world8, monkeypatch, "fp8", reqs, 6, SAMPLED, False)
    small = run_kind(world8, monkeypatch, "fp8", list(range(8)), 6, SAMPLED, False)
    assert small["launch"] == 2 and small["fp8"] == 1 and small["tiles"] == 1
    for b in range(8):
        same_request(big, b, small, b, "fp8 wide 0..7 against the fp8 flat launch")


def test_fp8_wide_switch(world8, monkeypatch, dev):
    from unimoe_audio_amd import _lib as L
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    from unimoe_audio_amd.model import DecodeEngine
    m, cfg = world8["m"], world8["cfg"]
    monkeypatch.setenv("UMOE_WIDE_DECODE", "0")              # no fp8 ragged path: the step refuses as with the switch off
    eng = DecodeEngine(m, 16, Lmax=LMAX, Tmax=TMAX, expert_weights="fp8", fp8_wide=True)
    try:
        rows = list(range(32))
        eng.prefill(world8["x"][rows].reshape(-1, cfg.hidden_size).contiguous(), world8["am"][rows].to(dev))
        pre, psteps = prepare_audio_prompt(cfg, [None] * 16)
        eng.start_decode(pre, psteps, 40, 4, **GREEDY)
        with pytest.raises(L.UmoeError, match="fp8 expert weights need the dense decode layout"):
            eng.step(False)
        torch.cuda.synchronize()
        assert eng.info("expert_launch") != 4 and eng.info("row_tiles") == 1          # nothing was enqueued
    finally:
        eng.close()
    monkeypatch.delenv("UMOE_WIDE_DECODE")
    # 8 requests with the switch on: the fp8 flat launch, exactly what the engine without the switch runs
    on = run_kind(world8, monkeypatch, "fp8", list(range(8)), 6, SAMPLED, False)
    off = run_kind(world8, monkeypatch, "fp8", list(range(8)), 6, SAMPLED, False, fp8_wide=False)
    assert on["launch"] == off["launch"] == 2 and on["fp8"] == off["fp8"] == 1 and on["tiles"] == 1
    same_engine_output(on, off, "8 requests")


def test_fp8_serving_of_12_rows_equals_bf16_serving(world8, monkeypatch):
    """a few admissions at different steps, row 10 used twice: the fp8 engine model.engine() builds against the bf16 engine on W_deq"""
    monkeypatch.setenv("UMOE_WIDE_DECODE", "1")              # (12 rows: not the bf16 engine's default)
    m = world8["m"]
    # (a request lives 26 to 30 steps and its delayed tail: some row is live at every step, and row 10 is free again at step 60)
    plan = {0: [(r, r) for r in range(5)], 3: [(ROW, 20), (7, 9)], 20: [(11, 21)], 40: [(8, 23)], 60: [(ROW, 22)]}
    f8, c8 = serve_run(world8, plan, True)
    assert m._engine.expert_weights == "fp8" and m._engine.fp8_wide and m._engine.info("expert_fp8") == 1
    m._engine.close()
    m._engine = None
    monkeypatch.setattr(m, "engine", functools.partial(type(m).engine, m, expert_weights="bf16"))
    ref, c16 = serve_run(world8, plan, True)
    assert m._engine.expert_weights == "bf16" and m._engine.info("expert_fp8") == 0
    m._engine.close()
    m._engine = None
    assert c8 == c16 == 1                                    # one graph capture across the admissions
    assert sorted(f8) == sorted(ref) == [0, 1, 2, 3, 4, 9, 20, 21, 22, 23]
    for b in f8:
        assert f8[b][1] == ref[b][1] and torch.equal(f8[b][0], ref[b][0]) and f8[b][2] == ref[b][2], b
