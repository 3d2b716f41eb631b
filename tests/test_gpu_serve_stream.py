"""Streamed serving on the GPU: the per-row table kernels bit for bit against the _win entries called row by row,
umoe_rvq_from_delayed_rows against umoe_rvq_from_delayed, the per-row decoder against the grouped executor and DacModel.decode, and
serve(stream=True) against the wav files of serve(stream=False)."""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
OPEN = 1 << 26


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from unimoe_audio_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _rand(g, lo, hi):
    return int(torch.randint(lo, hi + 1, (1,), generator=g))


def _make_row(g, ly, n, mode, use_res, dev):
    """One row's window: buffers that hold NaN wherever no requested output reads, a sentinel-filled output plane.
    mode: "left" (t_begin 0, sequence open), "mid" (open), "right" (true L, the window ends at the sequence's last output)"""
    s, K, pad = ly.stride, ly.K, ly.pad
    t0 = 0 if mode == "left" else _rand(g, 30, 70)
    want = t0 + max(n, 1) + (0 if mode == "right" else 40)          # outputs the sequence has at least
    if ly.kind == "conv":
        Lin = max((want - 1) * s + ly.dil * (K - 1) + 1 - 2 * pad, 1)
    else:
        Lin = max(-(-(want + 2 * pad - K) // s) + 1, 1)
    Lout = ly.out_len(Lin)
    assert Lout >= want
    if mode == "right":
        t0 = Lout - max(n, 1)
    x_full = torch.randn(ly.cin, Lin, generator=g)
    nn_ = max(n, 1)
    lo, hi = ly.reads(t0, t0 + nn_)
    lo, hi = max(lo, 0), min(hi, Lin - 1)
    x_off = max(0, lo - _rand(g, 0, 2))
    x_end = min(Lin, hi + 1 + _rand(g, 0, 2))
    xb = x_full[:, x_off:x_end].clone()
    pos = torch.arange(x_off, x_end)
    xb[:, (pos < lo) | (pos > hi)] = float("nan")
    y_off = max(0, t0 - _rand(g, 0, 3))
    Ly = t0 + nn_ - y_off + _rand(g, 0, 3)
    row = dict(x=xb.to(dev).contiguous(), x_off=x_off, hi=hi, y_off=y_off, Ly=Ly, t0=t0, n=n, L=Lin if mode == "right" else OPEN, Lin=Lin, resid=None, r_off=0)
    if use_res:
        r_off = max(0, t0 - _rand(g, 0, 5))
        rb = torch.randn(ly.cout, t0 + nn_ - r_off + _rand(g, 0, 4), generator=g)
        rpos = torch.arange(r_off, r_off + rb.shape[1])
        rb[:, (rpos < t0) | (rpos >= t0 + n)] = float("nan")
        row.update(resid=rb.to(dev).contiguous(), r_off=r_off)
    return row


def _table(rows, ys):
    from unimoe_audio_amd.dac import dac_row_words
    host = torch.tensor([dac_row_words(x=r["x"].data_ptr(), resid=0 if r["resid"] is None else r["resid"].data_ptr(), y=y.data_ptr(), x_off=r["x_off"],
                                       Lx=r["x"].shape[1], r_off=r["r_off"], Lr=0 if r["resid"] is None else r["resid"].shape[1], y_off=r["y_off"],
                                       Ly=r["Ly"], t_begin=r["t0"], n=r["n"], L=r["L"]) for r, y in zip(rows, ys)], dtype=torch.int64)
    return host


def _call_rows(ly, host, dev_table, rows_n, max_n, w, b, a, tanh):
    from unimoe_audio_amd import _lib as L_
    if ly.kind == "conv":
        return L_.lib().umoe_dac_conv1d_win_rows(_p(host), _p(dev_table), rows_n, max_n, _p(w), _p(b), _p(a), ly.cin, ly.cout, ly.K, ly.stride,
                                                 ly.dil, ly.pad, int(tanh), _stream())
    return L_.lib().umoe_dac_conv_transpose1d_win_rows(_p(host), _p(dev_table), rows_n, max_n, _p(w), _p(b), _p(a), ly.cin, ly.cout, ly.K,
                                                       ly.stride, ly.pad, 0, _stream())


def _call_win(ly, r, y, w, b, a, tanh):
    from unimoe_audio_amd import _lib as L_
    if ly.kind == "conv":
        return L_.lib().umoe_dac_conv1d_win(_p(r["x"]), r["x_off"], r["x"].shape[1], _p(w), _p(b), _p(a), _p(r["resid"]), r["r_off"],
                                            0 if r["resid"] is None else r["resid"].shape[1], 1, ly.cin, r["L"], ly.cout, ly.K, ly.stride, ly.dil,
                                            ly.pad, int(tanh), r["t0"], r["n"], _p(y), r["y_off"], r["Ly"], _stream())
    return L_.lib().umoe_dac_conv_transpose1d_win(_p(r["x"]), r["x_off"], r["x"].shape[1], _p(w), _p(b), _p(a), 1, ly.cin, r["L"], ly.cout, ly.K,
                                                  ly.stride, ly.pad, 0, r["t0"], r["n"], _p(y), r["y_off"], r["Ly"], _stream())


CONV_GEOMS = [dict(K=7, stride=1, dil=1, pad=3), dict(K=7, stride=1, dil=3, pad=9), dict(K=7, stride=1, dil=9, pad=27), dict(K=1, stride=1, dil=1, pad=0),
              dict(K=4, stride=2, dil=1, pad=1)]
CONVT_GEOMS = [dict(K=4, stride=2, dil=1, pad=1), dict(K=10, stride=5, dil=1, pad=3), dict(K=16, stride=8, dil=1, pad=4)]
NS = {1: [65], 3: [130, 0, 1], 5: [64, 0, 63, 130, 1]}
MODES = {1: ["right"], 3: ["left", "mid", "right"], 5: ["mid", "right", "left", "right", "mid"]}


def _cases():
    out = []
    for cin, cout in [(1, 1), (8, 64), (9, 65), (24, 130)]:
        out += [("conv", cin, cout, gm) for gm in CONV_GEOMS]
    for cin, cout in [(9, 65), (24, 8)]:
        out += [("convt", cin, cout, gm) for gm in CONVT_GEOMS]
    return out


@pytest.mark.parametrize("kind,cin,cout,gm", _cases(), ids=lambda v: str(v).replace(" ", "") if not isinstance(v, dict) else "K%(K)ds%(stride)dd%(dil)d" % v)
def test_row_kernels_are_bit_identical_to_the_win_entries_row_by_row(dev, kind, cin, cout, gm):
    from unimoe_audio_amd import dac as D
    g = torch.Generator().manual_seed(cin * 1000 + cout + gm["K"] + 7 * gm["dil"])
    ly = D.StreamLayer(kind, None, None, cin, cout, gm["K"], gm["stride"], gm["dil"], gm["pad"], 0, False, None)
    wshape = (cout, cin, gm["K"]) if kind == "conv" else (cin, cout, gm["K"])
    w = (torch.randn(wshape, generator=g) / (cin * gm["K"]) ** 0.5).to(dev)
    b = (0.1 * torch.randn(cout, generator=g)).to(dev)
    a = (0.5 + torch.rand(cin, generator=g)).to(dev)
    tanh = kind == "conv" and gm["K"] == 1
    for R in (1, 3, 5):
        use_res = kind == "conv" and gm["stride"] == 1 and R != 1
        rows = [_make_row(g, ly, n, mode, use_res, dev) for n, mode in zip(NS[R], MODES[R])]
        assert R == 1 or ({r["x_off"] > 0 for r in rows} == {True, False} and len({r["t0"] for r in rows}) > 1)
        ys = [torch.full((cout, r["Ly"]), SENTINEL, device=dev) for r in rows]
        want = [y.clone() for y in ys]
        for r, y in zip(rows, want):
            if r["n"]:
                assert _call_win(ly, r, y, w, b, a, tanh) == 0
        host = _table(rows, ys)
        max_n = max(r["n"] for r in rows)
        assert _call_rows(ly, host, host.to(dev), R, max_n, w, b, a, tanh) == 0
        torch.cuda.synchronize()
        for k, (r, y, ref) in enumerate(zip(rows, ys, want)):
            assert torch.equal(y.view(torch.int32), ref.view(torch.int32)), (R, k, r["n"], r["t0"])
            inside = y[:, r["t0"] - r["y_off"]:r["t0"] - r["y_off"] + r["n"]]
            assert not torch.isnan(inside).any() and not (inside == SENTINEL).any()
            outside = torch.ones(r["Ly"], dtype=torch.bool)
            outside[r["t0"] - r["y_off"]:r["t0"] - r["y_off"] + r["n"]] = False
            assert (y[:, outside.to(dev)] == SENTINEL).all()            # (an n = 0 row: its whole plane)
        if R != 3:
            continue
        # refusals: each leaves every output as it was
        before = [y.clone() for y in ys]
        bad = []
        k0 = next(k for k, r in enumerate(rows) if r["n"] > 1)
        short = host.clone()
        short[k0, 4] = rows[k0]["hi"] - rows[k0]["x_off"]                # the last input position the window reads is not in the buffer
        bad.append(("window misses its buffer", short, max_n))
        ybad = host.clone()
        ybad[k0, 8] = rows[k0]["t0"] + rows[k0]["n"] - rows[k0]["y_off"] - 1
        bad.append(("output buffer misses the window", ybad, max_n))
        bad.append(("max_n smaller than a row's n", host, max_n - 1))
        nullp = host.clone()
        nullp[k0, 0] = 0
        bad.append(("null plane", nullp, max_n))
        nully = host.clone()
        nully[k0, 2] = 0
        bad.append(("null output plane", nully, max_n))
        past = host.clone()
        if rows[2]["L"] != OPEN:
            past[2, 10] += 1                                             # one output past the sequence's true length
            bad.append(("outputs past the sequence", past, max_n + 1))
        for what, tab, mx in bad:
            assert _call_rows(ly, tab, tab.to(dev), R, mx, w, b, a, tanh) != 0, what
        torch.cuda.synchronize()
        for y, ref in zip(ys, before):
            assert torch.equal(y.view(torch.int32), ref.view(torch.int32))


def test_rvq_from_delayed_rows_is_bit_identical_per_row(dev):
    from unimoe_audio_amd import _lib as L_
    from unimoe_audio_amd import dac as D
    dm = D.DacModel(encoder_dim=16, decoder_dim=192).init_random(3).to(dev).float()
    f = dm._folded()
    B, Tmax, NQ, pad = 5, 120, 12, 1025
    torch.manual_seed(0)
    tokens = torch.randint(0, 1024, (B, Tmax, NQ), dtype=torch.int32)
    tokens[1, 40:45] = 1024
    tokens = tokens.to(dev)
    prefill = torch.tensor([1, 3, 2, 1, 4], dtype=torch.int32, device=dev)
    delay = torch.arange(NQ, dtype=torch.int32, device=dev)
    cb, ow, ob = f["cb"][:NQ].contiguous(), f["out_w"][:NQ].contiguous(), f["out_b"][:NQ].contiguous()
    Dl, Lz = dm.latent_dim, 60
    # (token row, f0, n, t_valid, col): different prefill steps, f0, n, t_valid; row 3 idle; row 4's newest frames lie past its t_valid
    recs = [(0, 0, 50, 100, 4), (1, 13, 7, 60, 0), (2, 30, 25, 80, 9), (3, 0, 0, 0, 0), (4, 20, 16, 40, 2)]
    z = torch.full((B, Dl, Lz), SENTINEL, device=dev)
    want = z.clone()
    rows = torch.arange(B, dtype=torch.int32, device=dev)
    for row, f0, n, tv, col in recs:
        if n:
            rc = L_.lib().umoe_rvq_from_delayed(_p(tokens), B, Tmax, NQ, _p(prefill), _p(delay), tv, pad, _p(rows[row:]), 1, f0, n, _p(cb), _p(ow),
                                                _p(ob), cb.shape[1], cb.shape[2], Dl, _p(want[row]), col, Lz, _stream())
            assert rc == 0
    host = torch.tensor([[row, f0, n, tv, z[row].data_ptr(), col, Lz, 0] for row, f0, n, tv, col in recs], dtype=torch.int64)

    def call(tab, max_n):
        return L_.lib().umoe_rvq_from_delayed_rows(_p(tokens), B, Tmax, NQ, _p(prefill), _p(delay), pad, _p(tab), _p(tab.to(dev)), B, max_n, _p(cb),
                                                   _p(ow), _p(ob), cb.shape[1], cb.shape[2], Dl, _stream())

    assert call(host, 50) == 0
    torch.cuda.synchronize()
    assert torch.equal(z.view(torch.int32), want.view(torch.int32))
    assert (z[3] == SENTINEL).all() and (z[0, :, :4] == SENTINEL).all() and not (z[0, :, 4:54] == SENTINEL).any()
    # positions at or past a row's t_valid read as pad: row 4 (prefill step 4, t_valid 40) reads channel 11 of its frames from
    # 40 - 4 - 11 = 25 on as pad, which is what a token buffer with an all-pad tail gives
    tok2 = tokens.clone()
    tok2[4, 40:] = pad
    ref = torch.full((Dl, Lz), SENTINEL, device=dev)
    assert L_.lib().umoe_rvq_from_delayed(_p(tok2), B, Tmax, NQ, _p(prefill), _p(delay), Tmax, pad, _p(rows[4:]), 1, 20, 16, _p(cb), _p(ow), _p(ob),
                                          cb.shape[1], cb.shape[2], Dl, _p(ref), 2, Lz, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(z[4].view(torch.int32), ref.view(torch.int32))
    # refusals leave z alone
    before = z.clone()
    for k, v in ((0, B), (3, Tmax + 1), (4, 0), (5, Lz - 49), (1, -1)):
        tab = host.clone()
        tab[0, k] = v
        assert call(tab, 50) != 0, k
    assert call(host, 49) != 0
    torch.cuda.synchronize()
    assert torch.equal(z.view(torch.int32), before.view(torch.int32))


def test_row_decoder_ragged_equals_grouped_equals_full_decode(dev):
    from tests.test_serve_stream_cpu import SCHEDULE, _drive, _with_window_log
    from unimoe_audio_amd import dac as D
    dm = D.DacModel(encoder_dim=16, decoder_dim=192).init_random(5).to(dev).float()
    waves = {}
    for ragged in (True, False):
        dec = _with_window_log(D.DacRowStreamDecoder)(dm, 3, None, max_frames=25, ragged=ragged)
        dec.wlog, dec.z = [], {}

        def src(requests, slab, dec=dec):
            for row, f0, n, col in requests:
                slab[row, :, col:col + n] = dec.z[row][:, f0:f0 + n].to(slab)

        dec.source = src
        for b in dec.bufs:
            b.fill_(float("nan"))
        waves[ragged] = _drive(dec, dm)
        assert dec.grown == 0
    assert sorted(waves[True]) == [(0, 0), (1, 0), (2, 0), (2, 1)]
    for key, (wave, z) in waves[True].items():
        ref = dm.decode(z.float().to(dev)[None])[0, 0]
        assert wave.shape == ref.shape and torch.equal(wave.view(torch.int32), ref.view(torch.int32)), key
        assert torch.equal(wave.view(torch.int32), waves[False][key][0].view(torch.int32)), key


# ---------------------------------------------------------------------------------------------------- end to end
def _requests(tmp_path):
    import wave
    import numpy as np
    from unimoe_audio_amd.api import MusicRequest, SpeechRequest
    t = np.arange(6400) / 16000
    src = str(tmp_path / "prompt.wav")
    if not os.path.exists(src):
        with wave.open(src, "wb") as wf:
            wf.setnchannels(1); wf.setsampwidth(2); wf.setframerate(16000)
            wf.writeframes((0.3 * np.sin(2 * np.pi * 220 * t) * 32767).astype("<i2").tobytes())
    # 7 requests, lengths of 1 and 2 s, min 0 and 1 s, their own seeds; the three speech requests share one voice
    return [MusicRequest("calm piano", max_audio_seconds=2, min_audio_seconds=1, seed=22),
            SpeechRequest("hello world", "the prompt text", src, max_audio_seconds=1, min_audio_seconds=1, seed=21),
            MusicRequest("fast drums", max_audio_seconds=1, min_audio_seconds=0, seed=24, save_name="drums"),
            SpeechRequest("a second sentence", "the prompt text", src, max_audio_seconds=2, min_audio_seconds=0, seed=23, temperature=1.2),
            MusicRequest("slow strings", max_audio_seconds=1, min_audio_seconds=1, seed=26),
            SpeechRequest("the last one", "the prompt text", src, max_audio_seconds=1, min_audio_seconds=1, seed=25),
            MusicRequest("a bright flute", max_audio_seconds=2, min_audio_seconds=1, seed=27)]


def _serve_both(app, reqs, tmp_path, tag, monkeypatch, **kw):
    """serve(stream=False) and serve(stream=True) of the same requests -> per read of the streamed run (rows with news, their frame
    positions before the push, library calls of the read)"""
    from unimoe_audio_amd import dac as D
    from unimoe_audio_amd.dac import write_wav_pcm16
    ref = dict(app.serve(iter(reqs), output_dir=str(tmp_path / f"ref_{tag}"), **kw))
    assert sorted(ref) == list(range(len(reqs)))
    reads, calls = [], [0]
    lib_call, push, flush = D._lib_call, D.DacRowStreamDecoder.push, D.DacRowStreamDecoder.flush

    def counted(name, *a):
        calls[0] += 1
        return lib_call(name, *a)

    def push_logged(self, n_new):
        live = [r for r, n in enumerate(n_new) if n]
        at = tuple(self.rows[r].have[0] for r in live)
        c0 = calls[0]
        out = push(self, n_new)
        reads.append((live, at, calls[0] - c0))
        return out

    monkeypatch.setattr(D, "_lib_call", counted)
    monkeypatch.setattr(D.DacRowStreamDecoder, "push", push_logged)
    pcm, finals, nonfinal = {}, {}, {}
    for ch in app.serve(iter(reqs), output_dir=str(tmp_path / f"st_{tag}"), stream=True, **kw):
        have = sum(p.numel() for p in pcm.get(ch.row, []))
        assert ch.start_sample == have and ch.pcm.dtype == torch.float32 and not ch.pcm.is_cuda
        assert finals.get(ch.row, 0) == 0                               # nothing behind a request's final chunk
        pcm.setdefault(ch.row, []).append(ch.pcm)
        finals[ch.row] = finals.get(ch.row, 0) + int(ch.final)
        nonfinal[ch.row] = nonfinal.get(ch.row, 0) + int(not ch.final and ch.pcm.numel() > 0)
    monkeypatch.setattr(D, "_lib_call", lib_call)
    monkeypatch.setattr(D.DacRowStreamDecoder, "push", push)
    assert finals == {i: 1 for i in range(len(reqs))}
    for i, path in ref.items():
        want = open(path, "rb").read()
        mine = str(tmp_path / f"mine_{tag}_{i}.wav")
        write_wav_pcm16(mine, torch.cat(pcm[i])[None], 16000)
        assert open(mine, "rb").read() == want, (tag, i)
        assert open(str(tmp_path / f"st_{tag}" / os.path.basename(path)), "rb").read() == want, (tag, i)
    # every request streamed: at least one chunk of samples ahead of its final one
    assert all(nonfinal[i] >= 1 for i in range(len(reqs))), nonfinal
    return reads, pcm


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_serve_stream_equals_serve(dev, tmp_path, monkeypatch, use_graph):
    from tests.test_gpu_stream import _app, _tiny_model
    m = _tiny_model(dev)
    app = _app(m, dev)
    reqs = _requests(tmp_path)
    kw = dict(slots=3, poll_every=8, max_prompt_tokens=256, max_audio_seconds=2, use_graph=use_graph, prefix_cache=True)
    reads, pcm = _serve_both(app, reqs, tmp_path, "g" if use_graph else "e", monkeypatch, **kw)
    rows = dict(app.served_rows)
    assert sorted(rows) == list(range(7)) and set(rows.values()) == {0, 1, 2}
    # a row is reused by a later request
    assert len(rows) > len(set(rows.values()))
    assert sum(hit for hit, _ in app.served_prefix.values()) >= 2      # the shared voice: one miss, then hits
    # in some read three rows are live on three different timelines
    assert any(len(live) == 3 and len(set(at)) == 3 for live, at, _ in reads), [(live, at) for live, at, _ in reads]
    # the library calls of a read do not depend on how many rows have news
    per = {len(live): {c for lv, _, c in reads if len(lv) == len(live)} for live, _, _ in reads}
    assert 1 in per and 3 in per, sorted(per)
    assert per[1] == per[3] and len(per[1]) == 1, per
    lys = len(app.serve_decoder.plan.layers)
    assert per[1] == {1 + 2 * lys}                                      # the source's launch, a move per buffer, a window launch per layer
    # the grouped executor gives the same bytes
    got = {}
    for ch in app.serve(iter(reqs), output_dir=None, stream=True, stream_ragged=False, **kw):
        got.setdefault(ch.row, []).append(ch.pcm)
    for i in range(7):
        assert torch.equal(torch.cat(got[i]).view(torch.int32), torch.cat(pcm[i]).view(torch.int32)), i
    m._engine.close()
    m._engine = None


def test_serve_stream_at_12_slots_in_the_wide_step(dev, tmp_path, monkeypatch):
    from tests.test_gpu_fp8 import build, ref_cfg
    from tests.test_gpu_stream import _app
    monkeypatch.setenv("UMOE_WIDE_DECODE", "1")              # (12 rows: the wide form is not the measured default)
    m = build(ref_cfg(), 41).to(dev)                          # (layers of the size the wide form takes)
    app = _app(m, dev)
    reqs = _requests(tmp_path)
    _serve_both(app, reqs + reqs, tmp_path, "w", monkeypatch, slots=12, poll_every=8, max_prompt_tokens=256, max_audio_seconds=2)
    assert m._engine.info("expert_launch") == 4
    assert len(set(app.served_rows.values())) < 14                      # 14 requests over 12 rows: a row is reused
    m._engine.close()
    m._engine = None
    del m
    torch.cuda.empty_cache()


def test_serve_stream_on_the_fp8_engine(dev, tmp_path, monkeypatch):
    from tests.test_gpu_fp8 import build, ref_cfg
    from tests.test_gpu_stream import _app
    m = build(ref_cfg(), 31).to(dev)
    m.quantize_experts_("fp8")
    app = _app(m, dev)
    reqs = _requests(tmp_path)
    _serve_both(app, reqs, tmp_path, "f", monkeypatch, slots=3, poll_every=8, max_prompt_tokens=256, max_audio_seconds=2)
    assert m._engine.expert_weights == "fp8" and m._engine.info("expert_fp8") == 1
    m._engine.close()
    m._engine = None
    del m
    torch.cuda.empty_cache()


def test_serve_stream_refusals(dev, tmp_path):
    from tests.test_gpu_stream import _app, _tiny_model
    from unimoe_audio_amd import _lib
    from unimoe_audio_amd import dac as D
    m = _tiny_model(dev)
    app = _app(m, dev)
    reqs = _requests(tmp_path)
    with pytest.raises(ValueError):
        next(app.serve(iter(reqs), slots=33, stream=True))
    with pytest.raises(TypeError):                                      # a video prompt is no request serve() takes
        next(app.serve([("video", "caption")], slots=2, stream=True, max_prompt_tokens=256, max_audio_seconds=1))
    # a DAC with fewer codebooks than the model has codec channels
    app.dac = D.Dac(model=D.DacModel(encoder_dim=16, decoder_dim=192, n_codebooks=8).init_random(2).to(dev).float())
    with pytest.raises(_lib.UmoeError, match="codebooks"):
        next(app.serve(iter(reqs), slots=2, stream=True, output_dir=None, max_prompt_tokens=256, max_audio_seconds=2))
    m._engine.close()
    m._engine = None
