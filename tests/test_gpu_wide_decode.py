"""GPU suite of the wide decode step: a batch of 9 to 32 requests decodes with every weight streamed once, and each request
decodes bit for bit to what it gets in a batch of 8.

Full width, two layers (hidden 2048, 16 / 2 heads, experts 2752 / 1376, vocab 320).  The engines of one test share Lmax, Tmax, attn_splits,
the prompt length T = 12 and the weights; every prompt prefills on the tiled kernels (2 B T >= 64 tokens), and the K / V slabs behind the
prefill are asserted equal between the big engine and the batch-8 engines before anything else is compared.

The wide form is the default only at the sizes where it was measured faster than the ragged path (batch 16 and 24..32); at batch
9 and at the 12 serving rows the tests select it with UMOE_WIDE_DECODE=1, and the default there is asserted to be the ragged path."""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

T, LMAX, TMAX = 12, 112, 96
SAMPLED = dict(cfg_scale=3.0, temperature=1.0, top_p=1.0, top_k=45, eos_mul=1.0, do_sample=True, seed=5)
GREEDY = dict(SAMPLED, do_sample=False)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from unimoe_audio_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def world(dev):
    """the model and the prompt pairs of 32 requests (embedded once); request b = rows 2 b, 2 b + 1"""
    from test_gpu_engine import prompt
    from test_gpu_fp8 import build, ref_cfg
    cfg = ref_cfg()
    m = build(cfg, 41).to(dev)
    ids, am, codec = prompt(cfg, 32, T, 6, [3, 0, 1, 0, 2, 0, 0, 4] + [0] * 40 + [1, 2, 0, 5] + [0] * 12)
    with torch.no_grad():
        x = m.calculate_input_embedding(ids.to(dev), codec.to(dev)).reshape(64, T, cfg.hidden_size).contiguous()
    yield dict(m=m, cfg=cfg, x=x, am=am, dev=dev, cache={})
    if m._engine is not None:
        m._engine.close()


def run(world, reqs, steps, settings, graph, probe=False, keep_engine=False):
    """a fresh engine holding the requests `reqs` (indices into the 32): prefill, `steps` decode steps -> everything the tests compare"""
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    from unimoe_audio_amd.model import DecodeEngine
    key = (tuple(reqs), steps, settings["do_sample"], graph, probe, os.environ.get("UMOE_WIDE_DECODE"))
    if key in world["cache"] and not keep_engine:
        return world["cache"][key]
    m, cfg, dev = world["m"], world["cfg"], world["dev"]
    B = len(reqs)
    rows = [r for b in reqs for r in (2 * b, 2 * b + 1)]
    eng = DecodeEngine(m, B, Lmax=LMAX, Tmax=TMAX, attn_splits=8, expert_weights="bf16")
    eng.prefill(world["x"][rows].reshape(-1, cfg.hidden_size).contiguous(), world["am"][rows].to(dev))
    torch.cuda.synchronize()
    kv = cfg.num_hidden_layers, 2 * B, cfg.num_key_value_heads, LMAX, cfg.head_dim
    out = dict(B=B, k=eng.copy_buffer("k_cache", torch.bfloat16, kv)[:, :, :, :T].cpu(), v=eng.copy_buffer("v_cache", torch.bfloat16, kv)[:, :, :, :T].cpu())
    pre, psteps = prepare_audio_prompt(cfg, [None] * B)
    eng.start_decode(pre, psteps, steps + 40, 4, **settings)           # (a bound beyond the delay pattern: no row is forced to end)
    dumps = eng.set_probe(dump_x1=True, dump_x=True, dump_logits=True) if probe else None
    for _ in range(steps):
        eng.step(graph)
    torch.cuda.synchronize()
    E, Lr = cfg.num_experts, cfg.num_hidden_layers
    out.update(tokens=eng.tokens.cpu().clone(), state=eng.state.cpu().clone(),
               mask=eng.copy_buffer("all_mask", torch.int32, (Lr, 2 * B, E)).cpu(), topk=eng.copy_buffer("all_topk", torch.int64, (Lr, 2 * B)).cpu(),
               launch=eng.info("expert_launch"), tiles=eng.info("row_tiles"), handoff=eng.handoff_error())
    if probe:
        out["probe"] = {k: v.cpu().clone() for k, v in dumps.items()}
        eng.set_probe()
    codes, lengths, _ = eng.finish()
    out["lengths"] = None if lengths is None else lengths.cpu().tolist()
    if keep_engine:
        return out, eng
    eng.close()
    world["cache"][key] = out
    return out


def same_request(big, i, small, j, what):
    """request at batch index i of `big` against index j of `small`: prompt K / V first, then tokens, state words, router ints"""
    Bb, Bs = big["B"], small["B"]
    for r in (0, 1):
        assert torch.equal(big["k"][:, 2 * i + r], small["k"][:, 2 * j + r]) and torch.equal(big["v"][:, 2 * i + r], small["v"][:, 2 * j + r]), (what, "prefill K / V")
    assert torch.equal(big["tokens"][i], small["tokens"][j]), (what, "tokens", i, j)
    for w in range(4):
        assert int(big["state"][w * Bb + i]) == int(small["state"][w * Bs + j]), (what, "state word", w, i, j)
    if big["lengths"] is not None and small["lengths"] is not None:
        assert big["lengths"][i] == small["lengths"][j]
    for r in (0, 1):
        assert torch.equal(big["mask"][:, 2 * i + r], small["mask"][:, 2 * j + r]), (what, "all_mask", i, j)
        assert torch.equal(big["topk"][:, 2 * i + r], small["topk"][:, 2 * j + r]), (what, "all_topk", i, j)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_batch_16_sampled_equals_batches_of_8(world, graph):
    big = run(world, list(range(16)), 12, SAMPLED, graph)
    assert big["launch"] == 4 and big["tiles"] == 2 and big["handoff"] == 0
    first = run(world, list(range(8)), 12, SAMPLED, graph)
    assert first["launch"] != 4 and first["tiles"] == 1
    for b in range(8):                      # draws are indexed by batch entry: equal indices
        same_request(big, b, first, b, "sampled 0..7")
    assert len({tuple(big["tokens"][b].flatten().tolist()) for b in range(16)}) > 8
    bigg = run(world, list(range(16)), 12, GREEDY, graph)
    second = run(world, list(range(8, 16)), 12, GREEDY, graph)
    for b in range(8):
        same_request(bigg, 8 + b, second, b, "greedy 8..15")


@pytest.mark.parametrize("B,tiles", [(9, 2), (24, 3), (32, 4)])
def test_every_group_of_eight_equals_a_batch_of_8(world, B, tiles, monkeypatch):
    if B == 9:
        monkeypatch.setenv("UMOE_WIDE_DECODE", "1")          # (not the default at this size: measured no faster than the ragged path)
    big = run(world, list(range(B)), 6, GREEDY, False)
    assert big["launch"] == 4 and big["tiles"] == tiles and big["handoff"] == 0
    for g0 in range(0, B, 8):
        reqs = [min(g0 + j, B - 1) for j in range(8)]          # the last group padded with copies of the last request
        small = run(world, reqs, 6, GREEDY, False)
        for j in range(min(8, B - g0)):
            same_request(big, g0 + j, small, j, f"B={B} group {g0 // 8}")


def test_per_layer_probe_localises_a_mismatch(world):
    """one eager step at B = 16 with the probe dumping x1 (behind o_proj), x (behind the combine) and the router logits of every layer:
    rows 0..15 and 16..31 equal the dumps of the two batch-8 engines"""
    big = run(world, list(range(16)), 1, GREEDY, False, probe=True)
    assert big["launch"] == 4
    for half in (0, 1):
        small = run(world, list(range(8 * half, 8 * half + 8)), 1, GREEDY, False, probe=True)
        for name in ("x1", "logits", "x"):
            a, b = big["probe"][name], small["probe"][name]
            for layer in range(a.shape[0]):
                assert torch.equal(a[layer, 16 * half:16 * half + 16].view(torch.int16), b[layer].view(torch.int16)), (name, layer, half)


def test_wide_decode_off_takes_the_ragged_path(world, monkeypatch):
    monkeypatch.setenv("UMOE_WIDE_DECODE", "0")
    off = run(world, list(range(9)), 6, GREEDY, False)
    assert off["launch"] != 4 and off["tiles"] == 1 and off["handoff"] == 0
    monkeypatch.delenv("UMOE_WIDE_DECODE")
    default = run(world, list(range(9)), 6, GREEDY, False)
    assert default["launch"] != 4 and default["tiles"] == 1          # batch 9: the measured default is the ragged path
    assert torch.equal(default["tokens"], off["tokens"])
    monkeypatch.setenv("UMOE_WIDE_DECODE", "1")
    on = run(world, list(range(9)), 6, GREEDY, False)
    assert on["launch"] == 4 and on["tiles"] == 2
    monkeypatch.setenv("UMOE_WIDE_DECODE", "0")
    off16 = run(world, list(range(16)), 6, GREEDY, False)             # a size where wide IS the default: the switch turns it off
    assert off16["launch"] != 4 and off16["tiles"] == 1 and off16["handoff"] == 0
    assert off["tokens"].shape == on["tokens"].shape and bool((off["tokens"][:, :T + 6] >= -1).all())


def test_fp8_and_expert_parallel_engines_never_take_the_wide_form(world, dev):
    from unimoe_audio_amd import _lib as L
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    from unimoe_audio_amd.model import DecodeEngine
    from test_gpu_fp8 import build, ref_cfg
    cfg = ref_cfg()
    m8 = build(cfg, 41).to(dev)
    m8.quantize_experts_("fp8")
    eng = DecodeEngine(m8, 16, Lmax=LMAX, Tmax=TMAX, expert_weights="fp8")
    try:
        rows = list(range(32))
        eng.prefill(world["x"][rows].reshape(-1, cfg.hidden_size).contiguous(), world["am"][rows].to(dev))
        pre, psteps = prepare_audio_prompt(cfg, [None] * 16)
        eng.start_decode(pre, psteps, 40, 4, **GREEDY)
        # an fp8 engine has no decode step above 16 rows: its step check refuses before anything is enqueued, as it did before
        with pytest.raises(L.UmoeError, match="fp8 expert weights need the dense decode layout"):
            eng.step(False)
        torch.cuda.synchronize()
        assert eng.info("expert_launch") != 4 and eng.info("row_tiles") == 1
    finally:
        eng.close()
    # expert parallel: more than 16 rows per rank are refused when the engine is created
    c = L.EngineCfg(hidden=cfg.hidden_size, layers=2, heads=16, kv_heads=2, head_dim=128, n_dyn=9, n_real=8, n_fix=2, inter_dyn=2752, inter_shared=1376,
                    codec_channels=cfg.codec_channels, codec_vocab=cfg.codec_vocab_size, eos=cfg.codec_eos_value, pad=cfg.codec_pad_value,
                    bos=cfg.codec_bos_value, mrope0=16, mrope1=24, mrope2=24, rms_eps=1e-6, top_p=0.7, fixed_top_k=0, jitter_eps=0.01, rows=32,
                    Lmax=LMAX, Tmax=TMAX, attn_splits=8, ep_rank=0, ep_size=2)
    h = C.c_void_p()
    assert L.lib().umoe_engine_create(C.byref(c), C.byref(h)) != 0


# ------------------------------------------------------------------------------------------------ serving
SLOTS, ROW = 12, 10


def serve_run(world, plan, graph):
    """a 12-row serving engine driven step by step; plan = {step: [(row, request)]} -> {request: (codes, length, end step)}, captures"""
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    m, cfg, dev = world["m"], world["cfg"], world["dev"]
    pre, ps = prepare_audio_prompt(cfg, [None])
    eng = m.engine(SLOTS, 16, 32)
    eng.start_serving(16)
    held, out, captures, step = {}, {}, 0, 0
    while held or step <= max(plan):
        for row, b in plan.get(step, []):
            was = eng.captured
            x = world["x"][[2 * b, 2 * b + 1]].reshape(-1, cfg.hidden_size).contiguous()
            eng.admit(row, x, world["am"][[2 * b, 2 * b + 1]], pre[0], ps[0], cfg_scale=3.0, temperature=1.0, top_p=1.0, top_k=45, eos_mul=1.0,
                      do_sample=True, seed=100 + b, min_tokens=1000, max_tokens=26 + (b % 5))
            assert eng.captured == was
            held[row] = b
        captures += graph and not eng.captured
        eng.step(graph)
        step += 1
        st = eng.poll()
        for row in sorted(held):
            if eng.row_done(st, row):
                codes, length = eng.take(row)
                out[held.pop(row)] = (codes.cpu(), length, step)
        assert step < 200
    assert eng.info("expert_launch") == 4 and eng.info("row_tiles") == 2 and eng.handoff_error() == 0
    return out, captures


def test_admission_into_a_wide_batch(world, monkeypatch):
    """request 20 into row 10 of an idle 12-row engine at step 0, and into row 10 at step 5 beside 9 live rows: the same codes and length, one
    graph replayed across the admission; the live rows are what they are without the admission"""
    monkeypatch.setenv("UMOE_WIDE_DECODE", "1")              # (12 rows: the wide form is not the measured default)
    others = [(r, r) for r in range(9)]
    alone, c0 = serve_run(world, {0: [(ROW, 20)]}, True)
    quiet, c1 = serve_run(world, {0: others}, True)
    late, c2 = serve_run(world, {0: others, 5: [(ROW, 20)]}, True)
    assert c0 == c1 == c2 == 1
    assert alone[20][1] == late[20][1] and torch.equal(alone[20][0], late[20][0]) and late[20][2] == alone[20][2] + 5
    for b in range(9):
        assert quiet[b][1] == late[b][1] and torch.equal(quiet[b][0], late[b][0]) and quiet[b][2] == late[b][2], b
        assert quiet[b][2] > 5
    world["m"]._engine.close()
    world["m"]._engine = None


def test_serve_12_slots_equals_generate_batch_of_each_request_in_its_row(dev, tmp_path):
    import wave
    import numpy as np
    from test_gpu_api import StandInTokenizer
    from test_gpu_stream import _app, _tiny_model
    from unimoe_audio_amd.api import MusicRequest, SpeechRequest
    m = _tiny_model(dev)
    app = _app(m, dev)
    app._tokenizer = StandInTokenizer(m.config.codec_placeholder_value)
    t = np.arange(6400) / 16000
    src = str(tmp_path / "prompt.wav")
    with wave.open(src, "wb") as wf:
        wf.setnchannels(1); wf.setsampwidth(2); wf.setframerate(16000)
        wf.writeframes((0.3 * np.sin(2 * np.pi * 220 * t) * 32767).astype("<i2").tobytes())
    reqs = []
    for i in range(14):
        if i % 3 == 0:
            reqs.append(MusicRequest(f"caption {i}", max_audio_seconds=1, min_audio_seconds=i % 2, seed=30 + i))
        else:
            reqs.append(SpeechRequest(f"sentence number {i}", "the prompt text", src, max_audio_seconds=1, min_audio_seconds=i % 2, seed=30 + i,
                                      temperature=1.0 + 0.1 * (i % 3)))
    with pytest.raises(ValueError):
        next(app.serve(iter(reqs), slots=33, output_dir=str(tmp_path / "no")))
    got = dict(app.serve(iter(reqs), slots=SLOTS, output_dir=str(tmp_path / "served"), poll_every=8, max_prompt_tokens=256, max_audio_seconds=1))
    assert sorted(got) == list(range(14))
    served_rows = dict(app.served_rows)
    assert set(served_rows.values()) == set(range(SLOTS))
    for i, r in enumerate(reqs):
        ref = app.generate_batch([r] * SLOTS, output_dir=str(tmp_path / f"ref{i}"))
        assert open(got[i], "rb").read() == open(ref[served_rows[i]], "rb").read(), (i, served_rows[i])
    m._engine.close()
    m._engine = None
