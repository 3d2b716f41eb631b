"""Streaming generation on the GPU: the windowed DAC kernels and umoe_rvq_from_delayed bit for bit against the full-sequence ones,
generate_codes_stream against generate_codes, and the streamed task methods' PCM against the wav files of the non-streaming ones."""
import os
import types

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from unimoe_audio_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _win_conv(kind, x, x_off, w, b, a, resid, r_off, L, t0, n, y_off, Ly, **g):
    import ctypes as C
    from unimoe_audio_amd import _lib as L_
    from unimoe_audio_amd.dac import _dev_f32, _stream
    Cout = w.shape[0] if kind == "conv" else w.shape[1]
    y = torch.full((x.shape[0], Cout, Ly), float("nan"), device=x.device)
    if kind == "conv":
        rc = L_.lib().umoe_dac_conv1d_win(_dev_f32(x), x_off, x.shape[2], _dev_f32(w), _dev_f32(b), _dev_f32(a), _dev_f32(resid), r_off,
                                          0 if resid is None else resid.shape[2], x.shape[0], x.shape[1], L, Cout, w.shape[2], g["stride"],
                                          g["dilation"], g["padding"], int(g.get("tanh", False)), t0, n, _dev_f32(y), y_off, Ly, _stream())
    else:
        rc = L_.lib().umoe_dac_conv_transpose1d_win(_dev_f32(x), x_off, x.shape[2], _dev_f32(w), _dev_f32(b), _dev_f32(a), x.shape[0],
                                                    x.shape[1], L, Cout, w.shape[2], g["stride"], g["padding"], 0, t0, n, _dev_f32(y), y_off,
                                                    Ly, _stream())
    return rc, y


@pytest.mark.parametrize("stride", [1, 2, 5, 8])
def test_windowed_convs_are_bit_identical_to_the_full_kernels(dev, stride):
    from unimoe_audio_amd import dac as D
    g = torch.Generator().manual_seed(stride)
    B, Cin, Cout, L = 2, 21, 70, 301
    x = torch.randn(B, Cin, L, generator=g).to(dev)
    alpha = (0.5 + torch.rand(Cin, generator=g)).to(dev)
    b = (0.1 * torch.randn(Cout, generator=g)).to(dev)
    cases = [("conv", dict(stride=stride, dilation=1, padding=3, K=7)), ("conv", dict(stride=1, dilation=9, padding=27, K=7, resid=True, tanh=True)),
             ("conv", dict(stride=stride, dilation=1, padding=0, K=1, resid=stride == 1))]
    if stride > 1:
        cases.append(("convt", dict(stride=stride, padding=(stride + 1) // 2, K=2 * stride)))
    for kind, gm in cases:
        K = gm.pop("K")
        use_res, tanh = gm.pop("resid", False), gm.pop("tanh", False)
        if kind == "conv":
            w = (torch.randn(Cout, Cin, K, generator=g) / (Cin * K) ** 0.5).to(dev)
            Lout = (L + 2 * gm["padding"] - gm["dilation"] * (K - 1) - 1) // gm["stride"] + 1
            res = torch.randn(B, Cout, Lout, generator=g).to(dev) if use_res else None
            full = D.conv1d(x, w, b, stride=gm["stride"], dilation=gm["dilation"], padding=gm["padding"], snake_alpha=alpha, resid=res, tanh=tanh)
            ly = D.StreamLayer("conv", None, None, Cin, Cout, K, gm["stride"], gm["dilation"], gm["padding"], 0, tanh, None)
        else:
            w = (torch.randn(Cin, Cout, K, generator=g) / (Cin * K) ** 0.5).to(dev)
            res = None
            full = D.conv_transpose1d(x, w, b, stride=gm["stride"], padding=gm["padding"], snake_alpha=alpha)
            ly = D.StreamLayer("convt", None, None, Cin, Cout, K, gm["stride"], 1, gm["padding"], 0, False, None)
        Lout = full.shape[2]
        for _ in range(6):
            t0 = int(torch.randint(0, Lout, (1,), generator=g))
            n = int(torch.randint(1, min(150, Lout - t0) + 1, (1,), generator=g))
            lo, hi = ly.reads(t0, t0 + n)
            lo, hi = max(lo, 0), min(hi, L - 1)
            # the input buffer: exactly the positions the window reads, plus a random margin
            x_off = max(0, lo - int(torch.randint(0, 3, (1,), generator=g)))
            x_end = min(L, hi + 1 + int(torch.randint(0, 3, (1,), generator=g)))
            xs = x[:, :, x_off:x_end].contiguous()
            r_off = max(0, t0 - 5)
            rs = res[:, :, r_off:t0 + n + 4].contiguous() if res is not None else None
            y_off = t0 - int(torch.randint(0, 4, (1,), generator=g))
            y_off = max(0, y_off)
            rc, y = _win_conv(kind, xs, x_off, w, b, alpha, rs, r_off, L, t0, n, y_off, t0 + n - y_off + 2, tanh=tanh, **gm)
            assert rc == 0
            torch.cuda.synchronize()
            got = y[:, :, t0 - y_off:t0 - y_off + n]
            assert torch.equal(got.view(torch.int32), full[:, :, t0:t0 + n].view(torch.int32)), (kind, gm, t0, n)
            # one position short on either side of the window's inputs is refused, not read
            if lo > 0 and x_off == lo and kind == "conv":
                rc, _ = _win_conv(kind, x[:, :, lo + 1:x_end].contiguous(), lo + 1, w, b, alpha, rs, r_off, L, t0, n, y_off,
                                  t0 + n - y_off + 2, tanh=tanh, **gm)
                assert rc != 0


def _fake_engine(cfg, tokens, psteps):
    return types.SimpleNamespace(cfg=cfg, tokens=tokens, prefill_steps=psteps)


def test_rvq_from_delayed_is_bit_identical_to_from_codes(dev):
    from unimoe_audio_amd import dac as D
    from unimoe_audio_amd.codec_utils import generate_output
    from unimoe_audio_amd.config import UniMoEAudioConfig
    cfg = UniMoEAudioConfig(hidden_size=256, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=1, vocab_size=320,
                            dynamic_intermediate_size=128, shared_intermediate_size=64, codec_placeholder_value=300)
    dm = D.DacModel(encoder_dim=16, decoder_dim=192).init_random(3).to(dev).float()
    B, Tmax, Cc, md = 3, 120, cfg.codec_channels, max(cfg.codec_delay_pattern)
    torch.manual_seed(0)
    tokens = torch.randint(0, 1024, (B, Tmax, Cc), dtype=torch.int32)
    tokens[1, 40:45] = cfg.codec_eos_value                       # codes past the codebook clamp like from_codes' do
    tokens = tokens.to(dev)
    psteps, lengths, dec_step = [1, 3, 2], [70, 55, 90], 100
    # DecodeEngine.finish()'s packing, then generate_output's revert
    max_len = max(lengths) + md
    out = torch.full((B, max_len, Cc), cfg.codec_pad_value, dtype=torch.long, device=dev)
    for i in range(B):
        seg = tokens[i, psteps[i]: min(psteps[i] + lengths[i] + md, dec_step + 1)]
        out[i, :seg.shape[0]] = seg.long()
    codes = generate_output(cfg, out, torch.tensor(lengths, device=dev))
    src = D.DelayedTokenSource(_fake_engine(cfg, tokens, psteps), dm)
    src.t_valid = dec_step + 1
    for rows, f0, n in (([0, 1, 2], 0, 50), ([2, 0], 13, 7), ([1], 30, 25)):
        z = torch.full((len(rows), dm.latent_dim, n + 9), float("nan"), device=dev)
        src(rows, f0, n, z, 4)
        for k, r in enumerate(rows):
            ref = dm.from_codes(codes[r][f0:f0 + n].transpose(0, 1)[None].to(dev))[0]
            assert torch.equal(z[k, :, 4:4 + n].view(torch.int32), ref.view(torch.int32)), (rows, f0, n, r)


def _tiny_model(dev, seed=0):
    from unimoe_audio_amd.config import UniMoEAudioConfig
    from unimoe_audio_amd.model import UniAudioRVQQwen2_5VLMoEForConditionalGeneration as Model
    cfg = UniMoEAudioConfig(hidden_size=256, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, vocab_size=320,
                            dynamic_intermediate_size=128, shared_intermediate_size=64, codec_placeholder_value=300)
    torch.manual_seed(seed)
    m = Model(cfg)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "norm" in n:
                p.fill_(1.0)
            elif n.endswith("bias"):
                p.zero_()
            else:
                p.normal_(0, 0.05)
    return m.to(dev, torch.bfloat16).eval()


def _app(m, dev):
    from unimoe_audio_amd import dac as D
    from unimoe_audio_amd.api import UniMoEAudio
    from tests.test_gpu_api import StandInTokenizer
    app = UniMoEAudio(None, 0, model=m)
    app._tokenizer = StandInTokenizer(m.config.codec_placeholder_value)
    app.dac = D.Dac(model=D.DacModel(encoder_dim=16, decoder_dim=192).init_random(2).to(dev).float())
    return app


def _prompt(cfg, B, T, seed):
    torch.manual_seed(seed)
    ids = torch.randint(1, 290, (2 * B, T))
    am = torch.ones(2 * B, T, dtype=torch.long)
    am[0, :2] = 0
    return ids, am


def _generate_both(m, ids, am, use_graph, chunk, **kw):
    """generate() + generate_output and generate_stream + the streamed frames' codes, same arguments"""
    from unimoe_audio_amd.api import _frame_codes
    from unimoe_audio_amd.codec_utils import DecoderOutput, generate_output, prepare_audio_prompt
    cfg = m.config
    B = ids.shape[0] // 2
    pre, st = prepare_audio_prompt(cfg, [None] * B)
    codes, lengths = m.generate(ids, am, DecoderOutput(pre.clone(), st, m.device), use_graph=use_graph, **kw)
    ref = generate_output(cfg, codes, lengths)
    got = [[] for _ in range(B)]
    pre, st = prepare_audio_prompt(cfg, [None] * B)
    reads = 0
    for upd in m.generate_stream(ids, am, DecoderOutput(pre, st, m.device), use_graph=use_graph, chunk_frames=chunk, **kw):
        reads += 1
        for r, f0, f1, _ in upd.rows:
            assert f0 == sum(c.shape[0] for c in got[r])
            got[r].append(_frame_codes(m._engine, r, f0, f1, upd.dec_step + 1))
    return ref, [torch.cat(g) if g else torch.zeros(0, cfg.codec_channels, dtype=torch.long) for g in got], reads


def test_generate_codes_stream_equals_generate_codes(dev):
    m = _tiny_model(dev)
    cfg = m.config
    ids, am = _prompt(cfg, 3, 10, 1)
    app = _app(m, dev)
    kw = dict(max_audio_seconds=1, min_audio_seconds=0, temperature=1.0, top_p=1.0, cfg_filter_top_k=45, seed=5)
    lens = set()
    for eos_mul in (1.0, 3.0):
        ref = app.generate_codes(ids, am, None, eos_prob_mul_factor=eos_mul, **kw)
        lens.add(tuple(r.shape[0] for r in ref))
        for chunk in (1, 7, 25):
            got = [[] for _ in range(3)]
            for row, c in app.generate_codes_stream(ids, am, None, eos_prob_mul_factor=eos_mul, chunk_frames=chunk, **kw):
                got[row].append(c)
            for r in range(3):
                assert torch.equal(torch.cat(got[r]), ref[r]), (eos_mul, chunk, r)
    # eager and graph replay of the bf16 engine
    for use_graph in (False, True):
        ref, got, _ = _generate_both(m, ids, am, use_graph, 7, max_tokens=50, min_tokens=0, cfg_scale=3.0, temperature=1.0, top_p=1.0,
                                     cfg_filter_top_k=45, eos_prob_mul_factor=3.0, seed=9)
        lens.add(tuple(r.shape[0] for r in ref))
        for r in range(3):
            assert torch.equal(got[r], ref[r]), (use_graph, r)
    print("row lengths seen:", sorted(lens))
    assert any(len(set(ls)) > 1 for ls in lens), f"every run ended all rows at the same step: {lens}"


def test_generate_stream_on_the_fp8_engine(dev):
    from tests.test_gpu_fp8 import build, ref_cfg
    cfg = ref_cfg()
    m = build(cfg, 31).to(dev)
    m.quantize_experts_("fp8")
    ids, am = _prompt(cfg, 3, 12, 2)
    ref, got, _ = _generate_both(m, ids, am, True, 7, max_tokens=40, min_tokens=0, cfg_scale=2.0, temperature=1.0, top_p=0.9,
                                 cfg_filter_top_k=45, eos_prob_mul_factor=2.0, seed=3)
    assert m._engine.expert_weights == "fp8" and m._engine.info("expert_fp8") == 1
    for r in range(3):
        assert torch.equal(got[r], ref[r]), r
    del m
    torch.cuda.empty_cache()


def test_streamed_task_methods_write_byte_identical_wavs(dev, tmp_path):
    import numpy as np
    import wave
    from unimoe_audio_amd.dac import write_wav_pcm16
    m = _tiny_model(dev)
    app = _app(m, dev)
    t = np.arange(6400) / 16000
    src = str(tmp_path / "prompt.wav")
    with wave.open(src, "wb") as wf:
        wf.setnchannels(1); wf.setsampwidth(2); wf.setframerate(16000)
        wf.writeframes((0.3 * np.sin(2 * np.pi * 220 * t) * 32767).astype("<i2").tobytes())
    kw = dict(max_audio_seconds=1, min_audio_seconds=0, temperature=1.0, top_p=1.0, cfg_filter_top_k=45)
    runs = [("speech", lambda **a: app.text_to_speech(["hello world", "second sentence"], "the prompt text", src, **a),
             lambda **a: app.text_to_speech_stream(["hello world", "second sentence"], "the prompt text", src, **a)),
            ("music", lambda **a: app.text_to_music(["calm piano", "fast drums"], **a), lambda **a: app.text_to_music_stream(["calm piano", "fast drums"], **a))]
    for stem, batch, stream in runs:
        ref = batch(output_dir=str(tmp_path / "ref"), save_name=stem, **kw)
        pcm = [[], []]
        finals = [0, 0]
        for ch in stream(output_dir=str(tmp_path / "st"), save_name=stem, chunk_frames=7, **kw):
            assert ch.start_sample == sum(p.numel() for p in pcm[ch.row]) and ch.pcm.dtype == torch.float32 and not ch.pcm.is_cuda
            assert finals[ch.row] == 0
            pcm[ch.row].append(ch.pcm)
            finals[ch.row] += int(ch.final)
        assert finals == [1, 1]
        for i, p in enumerate(ref):
            mine = str(tmp_path / f"mine_{stem}_{i}.wav")
            write_wav_pcm16(mine, torch.cat(pcm[i])[None], 16000)
            want = open(p, "rb").read()
            assert open(mine, "rb").read() == want, (stem, i)
            assert open(str(tmp_path / "st" / os.path.basename(p)), "rb").read() == want


def test_first_chunk_arrives_before_the_run_ends(dev):
    from unimoe_audio_amd.dac import stream_plan
    m = _tiny_model(dev)
    app = _app(m, dev)
    md = max(m.config.codec_delay_pattern)
    look = stream_plan(app.dac.model).lookahead_frames
    first_step, chunks = None, [0, 0]
    for ch in app.text_to_music_stream(["calm piano", "fast drums"], max_audio_seconds=1, min_audio_seconds=1, chunk_frames=5):
        if first_step is None:
            first_step = m._engine.steps_run
        chunks[ch.row] += 1
    assert first_step is not None and first_step <= 5 + md + look + 1, (first_step, md, look)
    assert m._engine.steps_run > first_step
    assert min(chunks) >= 2, chunks
