"""GPU tests of per-request settings inside one decode batch (umoe_row_params): the sampler and the delay step read row b's settings
from a device table; a mixed batch gives every row what a uniform batch with that row's settings gives it, bit for bit, from the
kernels up to the task API."""
import os
import wave

import numpy as np
import pytest
import torch

from oracle import decode as OD
from test_gpu_sampler import FAST_K, SLOW_K, TEMPS, TINY, U_ONE_SEED, Tally, eos_of, f32, grid_logits, pack, path_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from unimoe_audio_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


# ----------------------------------------------------------------------------- the sampler
B_S, C_S = 8, 12
ALL_K = FAST_K + SLOW_K                        # 9 values: 4 fast, 5 slow
TOP_PS = (0.5, 0.95, 1.0)
CFGS = (0.0, 1.0, 3.0, 10.0)
N_TABLES = 6                                   # rotations of the assignments below: every top_k meets several (T, top_p, cfg) partners


def table_rows(V, n, step):
    """B_S rows that differ in every field.  Rotation n: rows n % 8 and (n + 3) % 8 are the arg-max rows (do_sample 0 / temperature 0);
    the six sampled rows take consecutive values of ALL_K, so one launch always mixes the fast and the slow path."""
    rows = []
    for b in range(B_S):
        k = ALL_K[(b + 2 * n) % len(ALL_K)]
        rows.append(dict(cfg_scale=CFGS[(b + n) % 4], temperature=TEMPS[(b + n // 2) % 4], top_p=TOP_PS[(b + n) % 3],
                         top_k=V + 5 if k == "over" else k, eos_mul=(0.25, 0.6, 0.75, 0.8, 1.0, 1.5, 2.0, 3.0)[(b + n) % 8],
                         do_sample=True, seed=(U_ONE_SEED, 1, 2 ** 63 + 11, 7919, 2 ** 64 - 1, 0, 12345, 2 ** 40 + 3)[b] + n,
                         # on both sides of `step` (EOS off / on), equal to it, and None
                         min_tokens=(step + 1, step, step - 1, None, step + 7, 0, step + 1, step - 3)[(b + n) % 8], max_tokens=100 + b))
    rows[n % B_S]["do_sample"] = False
    rows[(n + 3) % B_S]["temperature"] = 0.0
    paths = {path_of(r["top_k"]) for r in rows if r["do_sample"] and r["temperature"] != 0.0}
    assert paths == {"fast", "slow"}, paths
    return rows


def is_argmax(r):
    return (not r["do_sample"]) or r["temperature"] == 0.0


def device_table(rows, dev):
    from unimoe_audio_amd import ops
    from unimoe_audio_amd.row_params import SETTINGS, pack_row_params
    t = pack_row_params(len(rows), **{k: [r[k] for r in rows] for k in SETTINGS})
    return ops.row_params_tensor(t, dev)


def launch(dev, lgd, V, step, *, table=None, row=None):
    """One cfg_sample launch over the whole batch: with the device table, or with row `row`'s values as today's scalar arguments.
    The scalar arguments beside a table are deliberately unlike every row: they must not be read."""
    from unimoe_audio_amd import ops
    st = torch.tensor([step], dtype=torch.int32, device=dev)
    if table is not None:
        kw = dict(cfg_scale=-7.0, temperature=9.0, top_p=0.123, top_k=3, eos_mul=-2.0, do_sample=True, seed=999, min_tokens=10 ** 6)
    else:
        kw = {k: row[k] for k in ("cfg_scale", "temperature", "top_p", "top_k", "eos_mul", "do_sample", "seed", "min_tokens")}
    pred, probs = ops.cfg_sample(lgd, B_S, C_S, V, eos=eos_of(V), want_probs=True, step=st, row_params=table, **kw)
    torch.cuda.synchronize()
    return pred.cpu(), probs.cpu().view(B_S, C_S, V)


def sampler_cases(V):
    gen = torch.Generator().manual_seed(4000 + V)
    for n in range(N_TABLES):
        step = 5 + 3 * n
        lg = pack(grid_logits(B_S * C_S, V, gen), grid_logits(B_S * C_S, V, gen), C_S)
        yield n, step, lg, table_rows(V, n, step)


@pytest.mark.parametrize("V", (1027, 2048))
def test_sampler_table_launch_equals_the_scalar_launches(dev, V):
    """For every b, pred[b] and probs_out[b*C:(b+1)*C] of ONE table launch are, bit for bit, those of today's scalar launch with row b's
    values.  (An arg-max row -- do_sample 0 or temperature 0 -- writes no probs_out in either launch: its pred is compared.)"""
    seen = set()
    for n, step, lg, rows in sampler_cases(V):
        lgd = lg.reshape(2 * B_S, C_S * V).to(dev)
        pred_t, probs_t = launch(dev, lgd, V, step, table=device_table(rows, dev))
        for b, r in enumerate(rows):
            pred_s, probs_s = launch(dev, lgd, V, step, row=r)
            assert torch.equal(pred_t[b], pred_s[b]), (V, n, b, r)
            if not is_argmax(r):
                assert torch.equal(probs_t[b].view(torch.int32), probs_s[b].view(torch.int32)), (V, n, b, r)
                seen.add(r["top_k"])
    assert seen == {V + 5 if k == "over" else k for k in ALL_K}, seen           # every top_k of both paths was a sampled row


@pytest.mark.parametrize("V", (1027, 2048))
def test_sampler_table_launch_vs_float64_restatement(dev, V):
    """The same table launches, row by row against oracle.decode (filter_probs / sampler_u / draw) the way test_gpu_sampler.check does:
    its tolerances (rtol 1e-4 beyond TINY, top-p gap 1e-6, CDF margin 1e-6) and its Tally caps."""
    tally = Tally()
    for n, step, lg, rows in sampler_cases(V):
        lgd = lg.reshape(2 * B_S, C_S * V).to(dev)
        pred_t, probs_t = launch(dev, lgd, V, step, table=device_table(rows, dev))
        for b, r in enumerate(rows):
            en = r["min_tokens"] is None or step >= r["min_tokens"]
            what = dict(V=V, n=n, b=b, step=step, en=en, **r)
            pair = lg[2 * b: 2 * b + 2]
            if is_argmax(r):
                gd = OD.cfg_and_mask(type("Cfg", (), dict(codec_eos_value=eos_of(V))), pair.double().clone(), r["cfg_scale"], en, f32(r["eos_mul"]))
                assert torch.equal(pred_t[b], torch.argmax(gd.reshape(-1, V), -1)), what
                continue
            ref, cand, gap = OD.filter_probs(pair, r["cfg_scale"], f32(r["temperature"]), f32(r["top_p"]), r["top_k"], eos_of(V),
                                             f32(r["eos_mul"]), en, details=True)
            u = OD.sampler_u(r["seed"], step, np.arange(b * C_S, (b + 1) * C_S))
            path = path_of(r["top_k"])
            for c in range(C_S):
                tally.rows += 1
                g, f = probs_t[b, c], ref[c]
                assert bool((g >= 0).all()) and abs(float(g.double().sum()) - 1.0) < 1e-5, (what, c)
                if float(gap[c]) < 1e-6:
                    tally.near_top_p += 1
                else:
                    sure = f > TINY
                    assert torch.equal((g > 0)[sure], sure[sure]) and not bool(((g > 0) & (f == 0)).any()), (what, c)
                    assert torch.allclose(g.double(), f, rtol=1e-4, atol=TINY), (what, c)
                lanes = None
                if path == "fast":
                    lanes = torch.nonzero(cand[c]).flatten().numpy()
                    assert len(lanes) == min(r["top_k"], V)
                want, margin = OD.draw(g.numpy(), u[c], path, lanes=lanes, margin=True)
                if int(pred_t[b, c]) != want:
                    assert path == "fast" and margin < 1e-6, (what, c, int(pred_t[b, c]), want, float(u[c]), margin)
                    tally.near_cdf += 1
    tally.bound()


@pytest.mark.parametrize("V", (1027, 2048))
def test_table_of_equal_rows_equals_scalars(dev, V):
    gen = torch.Generator().manual_seed(77 + V)
    for n, (k, top_p, T) in enumerate(((45, 0.95, 1.2), (None, 0.5, 1.0), (64, 1.0, 2.0), (65, 0.95, 0.3))):
        lg = pack(grid_logits(B_S * C_S, V, gen), grid_logits(B_S * C_S, V, gen), C_S)
        lgd = lg.reshape(2 * B_S, C_S * V).to(dev)
        r = dict(cfg_scale=3.0, temperature=T, top_p=top_p, top_k=k, eos_mul=0.8, do_sample=True, seed=2 ** 63 + n, min_tokens=4, max_tokens=50)
        for step in (3, 4):
            pred_t, probs_t = launch(dev, lgd, V, step, table=device_table([r] * B_S, dev))
            pred_s, probs_s = launch(dev, lgd, V, step, row=r)
            assert torch.equal(pred_t, pred_s) and torch.equal(probs_t.view(torch.int32), probs_s.view(torch.int32)), (V, k, step)


# ----------------------------------------------------------------------------- the delay step
def delay_restated(script, prefill, psteps, delay, eos, pad, Tmax, loop_max, row_max):
    """delay_step_kernel's rules with a per-row bound (model.py:1173-1203 + update_one), on host lists"""
    B, C, md = len(psteps), len(delay), max(delay)
    tok = torch.full((B, Tmax, C), -1, dtype=torch.int32)
    tok[:, : prefill.shape[1]] = prefill
    det, cd, fin, step, all_done = [0] * B, [-1] * B, [-1] * B, min(psteps) - 1, 0
    for pred in script:
        if all(v == 0 for v in cd) or step >= loop_max:
            all_done = 1
            continue
        cur, pred = step + 1, pred.clone()
        for b in range(B):
            if cd[b] != 0 and ((not det[b] and int(pred[b, 0]) == eos) or cur >= row_max[b] - md):
                det[b] = 1
                if cd[b] < 0:
                    cd[b], fin[b] = md, cur
        for b in range(B):
            for c in range(C):
                if cd[b] > 0 and md - cd[b] >= delay[c]:
                    pred[b, c] = eos if md - cd[b] == delay[c] else pad
            cd[b] -= cd[b] > 0
        if cur < Tmax:
            tok[:, cur] = torch.where(tok[:, cur] == -1, pred.to(torch.int32), tok[:, cur])
        step += 1
        all_done = int(all(v == 0 for v in cd) or step >= loop_max)
    return tok, det, cd, fin, step, all_done


def test_delay_step_rows_per_row_bound(dev):
    """B = 3 over a scripted pred sequence: row 0 and row 2 are forced to end by THEIR max_tokens (30, 45), row 1 by a sampled EOS on
    channel 0 (cur 20) long before its own (60); the loop bound is the largest.  With equal bounds: identical to umoe_delay_step."""
    from unimoe_audio_amd import ops
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    from unimoe_audio_amd.config import UniMoEAudioConfig
    from unimoe_audio_amd.row_params import pack_row_params
    cfg = UniMoEAudioConfig.tiny()
    delay, eos, pad = list(cfg.codec_delay_pattern), cfg.codec_eos_value, cfg.codec_pad_value
    B, C, md, Tmax = 3, cfg.codec_channels, max(delay), 80
    pre, psteps = prepare_audio_prompt(cfg, [None] * B)
    pre = pre.to(torch.int32)
    gen = torch.Generator().manual_seed(3)
    script = [torch.randint(0, eos, (B, C), generator=gen) for _ in range(70)]
    step0 = min(psteps) - 1
    script[20 - step0 - 1][1, 0] = eos                          # the pred of cur == 20
    script[5][2, 3] = eos                                       # EOS on a delayed channel is no ending

    def run(row_max, loop_max, rows_api):
        tok = torch.full((B, Tmax, C), -1, dtype=torch.int32)
        tok[:, : pre.shape[1]] = pre
        st = torch.zeros(4 * B + 8, dtype=torch.int32)
        st[B:3 * B] = -1
        st[3 * B:4 * B] = torch.tensor(psteps, dtype=torch.int32)
        st[4 * B], st[4 * B + 1], st[4 * B + 4] = step0, loop_max, step0
        tok_d, st_d, delay_d = tok.to(dev), st.to(dev), torch.tensor(delay, dtype=torch.int32, device=dev)
        table = None
        if rows_api:
            t = pack_row_params(B, cfg_scale=1.0, temperature=1.0, top_p=1.0, top_k=None, eos_mul=1.0, do_sample=True, seed=0, min_tokens=None,
                                max_tokens=list(row_max))
            table = ops.row_params_tensor(t, dev)
        for pred in script:
            ops.delay_step(pred.to(dev), tok_d, st_d, delay_d, eos, pad, row_params=table)
        torch.cuda.synchronize()
        return tok_d.cpu(), st_d.cpu()

    row_max = [30, 60, 45]
    tok, st = run(row_max, max(row_max), True)
    r_tok, det, cd, fin, step, all_done = delay_restated(script, pre, psteps, delay, eos, pad, Tmax, max(row_max), row_max)
    assert torch.equal(tok, r_tok)
    assert st[:B].tolist() == det and st[B:2 * B].tolist() == cd and st[2 * B:3 * B].tolist() == fin
    assert int(st[4 * B]) == step and int(st[4 * B + 2]) == all_done == 1
    assert fin == [30 - md, 20, 45 - md], fin                  # own bound, sampled EOS, own bound
    assert step < max(row_max)                                  # the loop ended when the last row had counted down, not at the bound
    for b in range(B):                                          # forced EOS / PAD by the delay pattern behind each row's own end
        for c in range(C):
            if delay[c] < md:                                   # (the countdown covers md steps: delays 0 .. md - 1)
                assert int(tok[b, fin[b] + delay[c], c]) == eos, (b, c)
                assert bool((tok[b, fin[b] + delay[c] + 1: fin[b] + md, c] == pad).all()), (b, c)
    # equal bounds: the table launch and umoe_delay_step write the same tokens and state
    tok_a, st_a = run([40, 40, 40], 40, True)
    tok_b, st_b = run([40, 40, 40], 40, False)
    assert torch.equal(tok_a, tok_b) and torch.equal(st_a, st_b)
    assert int(st_a[4 * B + 2]) == 1


# ----------------------------------------------------------------------------- the engine
MIXED = [  # B = 4; max_tokens: row 0 ends by ITS bound (24) while the others still decode; rows 1 / 3 may sample EOS (see the test)
    dict(cfg_scale=3.0, temperature=1.2, top_p=0.95, top_k=45, eos_mul=0.8, do_sample=True, seed=11, min_tokens=1000, max_tokens=24),
    dict(cfg_scale=1.0, temperature=1.0, top_p=1.0, top_k=None, eos_mul=1.0, do_sample=True, seed=2 ** 63 + 5, min_tokens=8, max_tokens=64),
    dict(cfg_scale=10.0, temperature=0.7, top_p=0.5, top_k=100, eos_mul=0.6, do_sample=True, seed=12, min_tokens=1000, max_tokens=36),
    dict(cfg_scale=2.0, temperature=1.5, top_p=0.9, top_k=5, eos_mul=-1.0, do_sample=True, seed=13, min_tokens=10, max_tokens=64),
]


def _engine_model(fmt, dev):
    """bf16: the small synthetic model of tests/test_gpu_engine.py; fp8: the full-width two-layer one of tests/test_gpu_fp8.py (the
    fp8 flat launch runs at the reference's layer width only).  Channel 0's EOS row of the codec head is scaled up so that EOS is
    often the arg-max in one sign or the other: rows 1 and 3 multiply it by +1 and -1, so one of them can draw it."""
    if fmt == "fp8":
        from test_gpu_fp8 import build, ref_cfg
        cfg = ref_cfg()
        m = build(cfg, 31)
    else:
        from test_gpu_engine import build, small_cfg
        cfg = small_cfg()
        m, _ = build(cfg, 3, 0.06)
    with torch.no_grad():
        m.codec_head.weight[cfg.codec_eos_value] *= 40
    m = m.to(dev)
    if fmt == "fp8":
        m.quantize_experts_("fp8")
    return m, cfg


@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
def test_engine_mixed_batch_equals_its_uniform_batches(dev, fmt):
    """For every b, row b of the mixed run (codes and length of finish()) is row b of the run with the SAME prompts in the same slots
    where all rows carry row b's settings through the scalar arguments.  Eager and graph replay."""
    from test_gpu_engine import prompt
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    from unimoe_audio_amd.row_params import SETTINGS
    gm, cfg = _engine_model(fmt, dev)
    B, T, MAXT = 4, 12, 64
    md = max(cfg.codec_delay_pattern)
    ids, am, codec = prompt(cfg, B, T, 4, [3, 0, 1, 0, 2, 0, 0, 4])          # prompts of different lengths (left padding)
    pre, psteps = prepare_audio_prompt(cfg, [None] * B)
    x = gm.calculate_input_embedding(ids.to(dev), codec.to(dev)).reshape(-1, cfg.hidden_size).contiguous()

    def run(settings, use_graph):
        eng = gm.engine(B, T, MAXT, expert_weights=fmt)
        eng.prefill(x, am.to(dev))
        kw = dict(settings)
        eng.start_decode(pre, psteps, kw.pop("max_tokens"), kw.pop("min_tokens"), **kw)
        assert (eng.io.row_params is not None) == any(isinstance(v, list) for v in settings.values())
        eng.run(use_graph=use_graph, poll_every=5)
        codes, lengths, _ = eng.finish()
        st = eng.state.cpu()
        assert eng.handoff_error() == 0
        if fmt == "fp8":
            assert eng.info("expert_fp8") == 1
        return codes.cpu(), lengths.cpu().tolist(), st[2 * B:3 * B].tolist(), int(st[4 * B])

    mixed_kw = {k: [r[k] for r in MIXED] for k in SETTINGS}
    ends = {}
    for use_graph in (False, True):
        codes, lengths, fin, last = run(mixed_kw, use_graph)
        print(f"{fmt} graph={use_graph}: lengths {lengths} finished_step {fin} last dec_step {last}")
        ends[use_graph] = (codes, lengths, fin)
        # row 0 was ended by ITS max_tokens while rows 1..3 were still decoding (their ends come later)
        assert fin[0] == MIXED[0]["max_tokens"] - md and all(f == -1 or f > fin[0] for f in fin[1:]), fin
        assert fin[2] == MIXED[2]["max_tokens"] - md, fin
        # a sampled EOS ended row 1 or row 3 before its own bound
        assert any(0 < fin[b] < MIXED[b]["max_tokens"] - md for b in (1, 3)), fin
        for b, r in enumerate(MIXED):
            u_codes, u_lengths, u_fin, _ = run(r, use_graph)
            n = lengths[b]
            assert u_lengths[b] == n and u_fin[b] == fin[b], (fmt, use_graph, b, u_lengths, lengths)
            assert torch.equal(codes[b][:n], u_codes[b][:n]), (fmt, use_graph, b)
            assert torch.equal(codes[b][:n + md], u_codes[b][:n + md]), (fmt, use_graph, b)     # with the forced EOS / PAD tail
    assert ends[False][1] == ends[True][1] and torch.equal(ends[False][0], ends[True][0])
    # wrong lengths are refused by name; the table needs room for the LARGEST max_tokens
    from unimoe_audio_amd._lib import UmoeError
    eng = gm.engine(B, T, MAXT, expert_weights=fmt)
    eng.prefill(x, am.to(dev))
    with pytest.raises(UmoeError, match="^temperature: a sequence of 3 values for a batch of 4"):
        eng.start_decode(pre, psteps, MAXT, 4, cfg_scale=1.0, temperature=[1.0] * 3, top_p=1.0, top_k=45, eos_mul=1.0, do_sample=True)
    with pytest.raises(UmoeError, match="too small"):
        eng.start_decode(pre, psteps, [10, 10, eng.Tmax, 10], 4, cfg_scale=1.0, temperature=1.0, top_p=1.0, top_k=45, eos_mul=1.0, do_sample=True)
    eng.close()
    gm._engine = None
    del gm
    torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- streaming and the task API
def test_stream_with_per_row_lengths_and_seeds(dev):
    """generate_codes_stream with per-row lengths and seeds: each row's chunks, concatenated, are generate_codes's codes with the same
    sequences; the short rows are complete while the long row still decodes."""
    from test_gpu_stream import _app, _prompt, _tiny_model
    from unimoe_audio_amd.codec_utils import DecoderOutput, prepare_audio_prompt
    m = _tiny_model(dev)
    app = _app(m, dev)
    ids, am = _prompt(m.config, 3, 10, 1)
    # min == max seconds: EOS stays off, every row ends by its own max_tokens (50, 100, 50)
    kw = dict(max_audio_seconds=[1, 2, 1], min_audio_seconds=[1, 2, 1], temperature=[1.0, 1.2, 0.8], top_p=1.0, cfg_filter_top_k=[45, None, 5],
              eos_prob_mul_factor=1.0, seed=[5, 6, 2 ** 63 + 7])
    ref = app.generate_codes(ids, am, None, **kw)
    md, ps = max(m.config.codec_delay_pattern), prepare_audio_prompt(m.config, [None] * 3)[1]
    assert [r.shape[0] for r in ref] == [50 - md - ps[0], 100 - md - ps[1], 50 - md - ps[2]]
    for chunk in (7, 25):
        got = [[] for _ in range(3)]
        for row, c in app.generate_codes_stream(ids, am, None, chunk_frames=chunk, **kw):
            got[row].append(c)
        for r in range(3):
            assert torch.equal(torch.cat(got[r]), ref[r]), (chunk, r)
    # other seeds give other codes: the per-row seed reaches the sampler
    other = app.generate_codes(ids, am, None, **dict(kw, seed=[5, 6, 8]))
    assert torch.equal(other[0], ref[0]) and torch.equal(other[1], ref[1]) and not torch.equal(other[2], ref[2])
    pre, st = prepare_audio_prompt(m.config, [None] * 3)
    done_at = {}
    for upd in m.generate_stream(ids, am, DecoderOutput(pre, st, m.device), max_tokens=[50, 100, 50], min_tokens=[50, 100, 50], cfg_scale=3.0,
                                 temperature=1.0, top_p=1.0, cfg_filter_top_k=45, eos_prob_mul_factor=1.0, seed=[1, 2, 3], chunk_frames=7):
        for r, _, _, complete in upd.rows:
            if complete:
                done_at[r] = upd.dec_step
    assert done_at[0] < done_at[1] and done_at[2] < done_at[1], done_at
    assert done_at[0] <= 50 + 7 and done_at[1] >= 99, done_at


def test_generate_batch_speech_and_music_in_one_batch(dev, tmp_path):
    """One SpeechRequest and one MusicRequest in one generation: each wav equals, byte for byte, the wav of the single-task call at batch 2
    in which both rows carry that request's prompt, settings and seed, padded to the mixed batch's prompt length."""
    from test_gpu_api import StandInTokenizer
    from test_gpu_stream import _app, _tiny_model
    from unimoe_audio_amd.api import MusicRequest, SpeechRequest

    class PaddedTokenizer(StandInTokenizer):
        min_len = 0

        def __call__(self, texts, **kw):
            enc = super().__call__(texts, **kw)
            extra = self.min_len - enc.input_ids.shape[1]
            if extra > 0:
                z = torch.zeros(enc.input_ids.shape[0], extra, dtype=enc.input_ids.dtype)
                enc.input_ids, enc.attention_mask = torch.cat([z, enc.input_ids], 1), torch.cat([z, enc.attention_mask], 1)
            return enc

    m = _tiny_model(dev)
    app = _app(m, dev)
    app._tokenizer = PaddedTokenizer(m.config.codec_placeholder_value)
    t = np.arange(6400) / 16000
    src = str(tmp_path / "prompt.wav")
    with wave.open(src, "wb") as wf:
        wf.setnchannels(1); wf.setsampwidth(2); wf.setframerate(16000)
        wf.writeframes((0.3 * np.sin(2 * np.pi * 220 * t) * 32767).astype("<i2").tobytes())
    speech = SpeechRequest("hello world", "the prompt text", src, max_audio_seconds=1, min_audio_seconds=0, seed=21)
    music = MusicRequest("calm piano", max_audio_seconds=2, min_audio_seconds=1, seed=22)
    assert (speech.cfg_scale, speech.eos_prob_mul_factor, music.cfg_scale, music.eos_prob_mul_factor) == (1.0, 1.0, 10.0, 0.6)
    out = app.generate_batch([speech, music], output_dir=str(tmp_path / "mixed"))
    assert [os.path.basename(p) for p in out] == ["generated_speech_0.wav", "generated_music_1.wav"]
    T = m._engine.T_prompt
    speech_T = app._speech_prompt("hello world", "the prompt text", src, None, None, None)[0].input_ids.shape[1]
    music_T = app._music_prompt("calm piano").input_ids.shape[1]
    assert T == max(speech_T, music_T) and speech_T != music_T            # one of the two prompts was padded
    app._tokenizer.min_len = T
    ref_s = app.text_to_speech(["hello world", "hello world"], "the prompt text", src, output_dir=str(tmp_path / "speech"), max_audio_seconds=1,
                               min_audio_seconds=0, seed=21)
    ref_m = app.text_to_music(["calm piano", "calm piano"], output_dir=str(tmp_path / "music"), max_audio_seconds=2, min_audio_seconds=1, seed=22)
    assert open(out[0], "rb").read() == open(ref_s[0], "rb").read()       # slot 0
    assert open(out[1], "rb").read() == open(ref_m[1], "rb").read()       # slot 1
    # the streamed form of the same batch: the same PCM, and the same files
    app._tokenizer.min_len = 0
    pcm = [[], []]
    for ch in app.generate_batch([speech, music], output_dir=str(tmp_path / "st"), stream=True, chunk_frames=7):
        pcm[ch.row].append(ch.pcm)
    for i, p in enumerate(out):
        assert open(str(tmp_path / "st" / os.path.basename(p)), "rb").read() == open(p, "rb").read(), i
    assert min(sum(c.numel() for c in pcm[i]) for i in (0, 1)) > 0
    with pytest.raises(TypeError):
        app.generate_batch(["calm piano"], output_dir=str(tmp_path))
