"""GPU tests of admission into a decoding batch: per-row clocks against the one clock, the clock-mode kernels against
restatements, and requests admitted into free rows of a batch that is decoding -- every comparison bit for bit."""
import os

import numpy as np
import pytest
import torch

from test_gpu_row_params import MIXED, _engine_model, device_table
from test_gpu_sampler import eos_of, grid_logits, pack

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from unimoe_audio_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _release(gm):
    if gm._engine is not None:
        gm._engine.close()
    gm._engine = None
    torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- 1. a zero-offset clock table against the one clock
@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
def test_zero_offset_clock_equals_the_scalar_clock(dev, fmt):
    """The MIXED batch of the per-request settings tests (rows end at different steps, by their own bound and by a sampled EOS) on the
    one clock and on a clock table {0, T} per row: codes, lengths, the rows' state words, the step word and every token up to each
    row's end are equal, eager and graph.  (Behind its end a row is parked in clock mode: what it writes there is never read.)"""
    from test_gpu_engine import prompt
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    from unimoe_audio_amd.row_params import SETTINGS
    gm, cfg = _engine_model(fmt, dev)
    B, T, MAXT = 4, 12, 64
    md = max(cfg.codec_delay_pattern)
    ids, am, codec = prompt(cfg, B, T, 4, [3, 0, 1, 0, 2, 0, 0, 4])
    pre, psteps = prepare_audio_prompt(cfg, [None] * B)
    x = gm.calculate_input_embedding(ids.to(dev), codec.to(dev)).reshape(-1, cfg.hidden_size).contiguous()
    kw = {k: [r[k] for r in MIXED] for k in SETTINGS}

    def run(clock, use_graph):
        eng = gm.engine(B, T, MAXT, expert_weights=fmt)
        eng.prefill(x, am.to(dev))
        k = dict(kw)
        eng.start_decode(pre, psteps, k.pop("max_tokens"), k.pop("min_tokens"), **k)
        if clock:
            eng.use_row_clock()
            assert eng.io.row_clock
        else:
            assert not eng.io.row_clock
        eng.run(use_graph=use_graph, poll_every=5)
        codes, lengths, tokens = eng.finish()
        assert eng.handoff_error() == 0
        return codes.cpu(), lengths.cpu().tolist(), tokens.cpu(), eng.state.cpu()

    for use_graph in (False, True):
        c0, l0, t0, s0 = run(False, use_graph)
        c1, l1, t1, s1 = run(True, use_graph)
        print(f"{fmt} graph={use_graph}: lengths {l0} finished {s0[2 * B:3 * B].tolist()} last step {int(s0[4 * B])}")
        assert l0 == l1 and torch.equal(c0, c1)
        assert torch.equal(s0[:4 * B + 5], s1[:4 * B + 5]), (s0.tolist(), s1.tolist())
        fin = s0[2 * B:3 * B].tolist()
        assert all(f > 0 for f in fin) and len(set(fin)) > 1, fin
        for b in range(B):
            assert torch.equal(t0[b, :fin[b] + md], t1[b, :fin[b] + md]), (fmt, use_graph, b)
    _release(gm)


# ----------------------------------------------------------------------------- 2. the kernels
def clock_restated(script, tok, det, cd, fin, psteps, off, step, delay, eos, pad, Tmax, row_max):
    """delay_step_kernel in clock mode on host lists: row b lives at cur_b = step - off[b] + 1"""
    B, C, md = len(psteps), len(delay), max(delay)
    tok, det, cd, fin = tok.clone(), list(det), list(cd), list(fin)
    all_done, bos_over = 0, 0
    for pred in script:
        if all(v == 0 for v in cd):
            all_done = 1
            continue
        pred = pred.clone()
        cur = [step - off[b] + 1 for b in range(B)]
        live = [cd[b] != 0 for b in range(B)]
        for b in range(B):
            if live[b] and ((not det[b] and int(pred[b, 0]) == eos) or cur[b] >= row_max[b] - md):
                det[b] = 1
                if cd[b] < 0:
                    cd[b], fin[b] = md, cur[b]
        for b in range(B):
            for c in range(C):
                if cd[b] > 0 and md - cd[b] >= delay[c]:
                    pred[b, c] = eos if md - cd[b] == delay[c] else pad
            cd[b] -= cd[b] > 0
        if not bos_over:
            bos_over = int(all(cur[b] - psteps[b] >= md for b in range(B)))
        for b in range(B):
            if live[b] and 0 <= cur[b] < Tmax:
                tok[b, cur[b]] = torch.where(tok[b, cur[b]] == -1, pred[b].to(torch.int32), tok[b, cur[b]])
        step += 1
        all_done = int(all(v == 0 for v in cd))
    return tok, det, cd, fin, step, all_done, bos_over


def test_delay_step_clock_vs_host_restatement(dev):
    """B = 4 at the global step 40, rows at different offsets: row 0 began 6 steps ago and ends by ITS max_tokens, row 1 begins now and
    ends by a sampled EOS, row 2 is parked (countdown 0: nothing of it may change), row 3 began 2 steps ago and ends by its bound last.
    The step word passes every row's max_tokens without ending the run; the run ends when every countdown is 0."""
    from unimoe_audio_amd import ops
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    from unimoe_audio_amd.config import UniMoEAudioConfig
    cfg = UniMoEAudioConfig.tiny()
    delay, eos, pad = list(cfg.codec_delay_pattern), cfg.codec_eos_value, cfg.codec_pad_value
    B, C, md, Tmax, g0 = 4, cfg.codec_channels, max(delay), 90, 40
    pre, psteps = prepare_audio_prompt(cfg, [None] * B)
    began = [6, 0, 0, 2]                                          # steps ago
    off = [g0 - (psteps[b] - 1) - began[b] for b in range(B)]
    row_max = [30, 70, 25, 50]
    assert all(m < g0 + 1 for m in row_max[:1])                   # the step word is beyond a live row's own bound from the start
    gen = torch.Generator().manual_seed(5)
    script = [torch.randint(0, eos, (B, C), generator=gen) for _ in range(70)]
    script[12][1, 0] = eos                                        # row 1: a sampled EOS at its local cur 13
    script[3][3, 2] = eos                                         # EOS on a delayed channel is no ending
    tok = torch.full((B, Tmax, C), -1, dtype=torch.int32)
    tok[:, : pre.shape[1]] = pre.to(torch.int32)
    for b in range(B):                                            # what the rows wrote before: their slots up to the local step
        n = psteps[b] + began[b]
        tok[b, psteps[b]:n] = torch.where(tok[b, psteps[b]:n] == -1, torch.randint(0, eos, (n - psteps[b], C), generator=gen).to(torch.int32),
                                          tok[b, psteps[b]:n])
    det, cd, fin = [0, 0, 1, 0], [-1, -1, 0, -1], [-1, -1, 9, -1]
    st = torch.zeros(4 * B + 8, dtype=torch.int32)
    st[:B], st[B:2 * B], st[2 * B:3 * B] = torch.tensor(det), torch.tensor(cd), torch.tensor(fin)
    st[3 * B:4 * B] = torch.tensor(psteps, dtype=torch.int32)
    st[4 * B], st[4 * B + 1] = g0, 10                             # (max_tokens of the state: far below the step word, and not read)
    clk = torch.tensor([[off[b], 17] for b in range(B)], dtype=torch.int32, device=dev)
    table = device_table([dict(cfg_scale=1.0, temperature=1.0, top_p=1.0, top_k=None, eos_mul=1.0, do_sample=True, seed=0, min_tokens=None,
                               max_tokens=m) for m in row_max], dev)
    tok_d, st_d, delay_d = tok.to(dev), st.to(dev), torch.tensor(delay, dtype=torch.int32, device=dev)
    for pred in script:
        ops.delay_step(pred.to(dev), tok_d, st_d, delay_d, eos, pad, row_params=table, row_clock=clk)
    torch.cuda.synchronize()
    got_tok, got = tok_d.cpu(), st_d.cpu()
    r_tok, r_det, r_cd, r_fin, r_step, r_done, r_bos = clock_restated(script, tok, det, cd, fin, psteps, off, g0, delay, eos, pad, Tmax, row_max)
    assert torch.equal(got_tok, r_tok)
    assert got[:B].tolist() == r_det and got[B:2 * B].tolist() == r_cd and got[2 * B:3 * B].tolist() == r_fin
    assert int(got[4 * B]) == r_step and int(got[4 * B + 2]) == r_done == 1 and int(got[4 * B + 3]) == r_bos
    ps = psteps
    assert r_fin == [30 - md, 13, 9, 50 - md], r_fin             # own bound, sampled EOS, untouched, own bound (all LOCAL steps)
    assert torch.equal(got_tok[2], tok[2])                        # the parked row wrote nothing
    assert r_step == g0 + (50 - md - (ps[3] + began[3])) + md     # row 3's countdown ended the run, md steps after its bound
    for b in (0, 1, 3):                                           # forced EOS / PAD by the delay pattern behind each row's own end
        for c in range(C):
            if delay[c] < md:
                assert int(got_tok[b, r_fin[b] + delay[c], c]) == eos, (b, c)
    # NULL table: umoe_delay_step_clock is umoe_delay_step_rows
    a_tok, a_st, b_tok, b_st = tok.to(dev), st.to(dev), tok.to(dev), st.to(dev)
    a_st[4 * B], b_st[4 * B], a_st[4 * B + 1], b_st[4 * B + 1] = 0, 0, 70, 70
    a_st[B + 2], b_st[B + 2] = -1, -1
    zero = torch.zeros((B, 2), dtype=torch.int32, device=dev)
    for pred in script:
        ops.delay_step(pred.to(dev), a_tok, a_st, delay_d, eos, pad, row_params=table)
        ops.delay_step(pred.to(dev), b_tok, b_st, delay_d, eos, pad, row_params=table, row_clock=zero)
    torch.cuda.synchronize()
    assert torch.equal(a_st.cpu()[:4 * B + 1], b_st.cpu()[:4 * B + 1])
    fin_a = a_st.cpu()[2 * B:3 * B].tolist()
    for b in range(B):                                            # (up to each row's end: an ended row writes nothing in clock mode)
        assert fin_a[b] > 0 and torch.equal(a_tok.cpu()[b, :fin_a[b] + md], b_tok.cpu()[b, :fin_a[b] + md]), b


@pytest.mark.parametrize("V", (1027, 2048))
def test_sampler_step_off_equals_scalar_launches_at_the_shifted_steps(dev, V):
    """One launch with a clock table at the global step g: pred and probs of row b are those of a scalar launch (no table) with row b's
    settings at the step g - step_off[b].  min_tokens lies on both sides of the LOCAL step and never of the global one."""
    from unimoe_audio_amd import ops
    B, C, g = 8, 12, 100
    offs = [0, 100, 93, 60, 99, 41, 100, 7]
    gen = torch.Generator().manual_seed(9000 + V)
    lg = pack(grid_logits(B * C, V, gen), grid_logits(B * C, V, gen), C)
    lgd = lg.reshape(2 * B, C * V).to(dev)
    rows = []
    for b in range(B):
        local = g - offs[b]
        rows.append(dict(cfg_scale=(0.0, 1.0, 3.0, 10.0)[b % 4], temperature=(1.0, 1.2, 0.7, 2.0)[b % 4], top_p=(0.5, 0.95, 1.0)[b % 3],
                         top_k=(45, None, 5, 64, 65, 100, 45, None)[b], eos_mul=(0.6, 0.8, 1.0, 1.5)[b % 4], do_sample=b != 5,
                         seed=(11, 2 ** 63 + 5, 12, 13, 2 ** 64 - 1, 0, 7919, 3)[b], min_tokens=(local + 1, local, local - 1, None)[b % 4] if local else 1,
                         max_tokens=500))
    st = torch.tensor([g], dtype=torch.int32, device=dev)
    clk = torch.tensor([[o, 33] for o in offs], dtype=torch.int32, device=dev)
    dummy = dict(cfg_scale=-7.0, temperature=9.0, top_p=0.123, top_k=3, eos_mul=-2.0, do_sample=True, seed=999, min_tokens=10 ** 6)
    pred_t, probs_t = ops.cfg_sample(lgd, B, C, V, eos=eos_of(V), want_probs=True, step=st, row_params=device_table(rows, dev), row_clock=clk, **dummy)
    pred_t, probs_t = pred_t.cpu(), probs_t.cpu().view(B, C, V)
    for b, r in enumerate(rows):
        sb = torch.tensor([g - offs[b]], dtype=torch.int32, device=dev)
        kw = {k: r[k] for k in ("cfg_scale", "temperature", "top_p", "top_k", "eos_mul", "do_sample", "seed", "min_tokens")}
        pred_s, probs_s = ops.cfg_sample(lgd, B, C, V, eos=eos_of(V), want_probs=True, step=sb, **kw)
        assert torch.equal(pred_t[b], pred_s.cpu()[b]), (V, b, r)
        if r["do_sample"]:
            assert torch.equal(probs_t[b].view(torch.int32), probs_s.cpu().view(B, C, V)[b].view(torch.int32)), (V, b, r)
    # the local step reaches the draw: the same table at another global step with the offsets moved along draws the same
    st2 = torch.tensor([g + 17], dtype=torch.int32, device=dev)
    clk2 = torch.tensor([[o + 17, 33] for o in offs], dtype=torch.int32, device=dev)
    pred_u = ops.cfg_sample(lgd, B, C, V, eos=eos_of(V), step=st2, row_params=device_table(rows, dev), row_clock=clk2, **dummy)
    assert torch.equal(pred_u.cpu(), pred_t)


# ----------------------------------------------------------------------------- 3. - 7. requests admitted into a batch
SLOTS, MAX_PROMPT, MAXT = 4, 16, 64
ROW_B = 2                                       # the row request "r" is admitted into
REQ = {   # name: (T, pads of the pair, prompt seed, settings)
    "r": (11, [2, 0], 21, dict(cfg_scale=3.0, temperature=1.2, top_p=0.95, top_k=45, eos_mul=0.8, do_sample=True, seed=31, min_tokens=1000, max_tokens=30)),
    "o0": (14, [0, 3], 22, dict(cfg_scale=1.0, temperature=1.0, top_p=1.0, top_k=None, eos_mul=1.0, do_sample=True, seed=2 ** 63 + 5, min_tokens=8, max_tokens=48)),
    "o1": (9, [1, 0], 23, dict(cfg_scale=10.0, temperature=0.7, top_p=0.5, top_k=100, eos_mul=0.6, do_sample=True, seed=12, min_tokens=1000, max_tokens=40)),
    "o3": (16, [0, 0], 24, dict(cfg_scale=2.0, temperature=1.5, top_p=0.9, top_k=5, eos_mul=-1.0, do_sample=True, seed=13, min_tokens=10, max_tokens=56)),
    "first": (12, [0, 1], 25, dict(cfg_scale=2.0, temperature=1.0, top_p=1.0, top_k=45, eos_mul=1.0, do_sample=True, seed=77, min_tokens=1000, max_tokens=20)),
}
OTHERS = {0: "o0", 1: "o1", 3: "o3"}


class Serving:
    """A serving engine driven step by step: plan = {global step: [(row, request name)]}; a row's result is taken at the first step
    that finds it ended (state read every step: these are tests of the engine, not of the polling policy)."""

    def __init__(self, gm, cfg, fmt, dev):
        from test_gpu_engine import prompt
        from unimoe_audio_amd.codec_utils import prepare_audio_prompt
        self.gm, self.cfg, self.fmt, self.dev = gm, cfg, fmt, dev
        self.pre, self.ps = prepare_audio_prompt(cfg, [None])
        self.inputs = {}
        for name, (T, pads, seed, _) in REQ.items():
            ids, am, codec = prompt(cfg, 1, T, seed, pads)
            x = gm.calculate_input_embedding(ids.to(dev), codec.to(dev)).reshape(-1, cfg.hidden_size).contiguous()
            self.inputs[name] = (x, am)

    def engine(self):
        eng = self.gm.engine(SLOTS, MAX_PROMPT, MAXT, expert_weights=self.fmt)
        eng.start_serving(MAX_PROMPT)
        return eng

    def admit(self, eng, row, name):
        x, am = self.inputs[name]
        eng.admit(row, x, am, self.pre[0], self.ps[0], **REQ[name][3])

    def run(self, plan, use_graph, watch=None):
        eng = self.engine()
        held, out, captures = {}, {}, 0
        last = max(plan)
        step = 0
        while held or step <= last:
            for row, name in plan.get(step, []):
                assert row not in held
                was = eng.captured
                self.admit(eng, row, name)
                assert eng.captured == was            # an admission never invalidates the captured step
                held[row] = name
            captures += use_graph and not eng.captured
            eng.step(use_graph)
            step += 1
            st = eng.poll()
            assert int(st[4 * SLOTS]) == step        # the global word advances by one per step while a row is live
            if watch:
                watch(eng, step, st, held)
            for row in sorted(held):
                if eng.row_done(st, row):
                    codes, length = eng.take(row)
                    out[held.pop(row)] = (codes.cpu(), length, step)
            assert step < 400
        if self.fmt == "fp8":
            assert eng.info("expert_fp8") == 1
        assert captures == (1 if use_graph else 0), captures        # ONE capture for the whole run: replay across admissions
        return out


@pytest.fixture(scope="module", params=["bf16", "fp8"])
def served(request, dev):
    """every scenario of tests 3 - 7, eager and graph, run once per expert format"""
    fmt = request.param
    gm, cfg = _engine_model(fmt, dev)
    S = Serving(gm, cfg, fmt, dev)
    res = {"fmt": fmt, "cfg": cfg}
    for g in (False, True):
        res[("alone", g)] = S.run({0: [(ROW_B, "r")]}, g)                                             # idle engine, step 0
        res[("others", g)] = S.run({0: [(b, n) for b, n in OTHERS.items()]}, g)                       # no admission
        res[("late", g)] = S.run({0: [(b, n) for b, n in OTHERS.items()], 7: [(ROW_B, "r")]}, g)      # r joins at step 7
        # row reuse: "first" runs in ROW_B from step 0 and ends (20 - 1 steps); r takes the row at step 25 while the others decode
        res[("reuse", g)] = S.run({0: [(b, n) for b, n in OTHERS.items()] + [(ROW_B, "first")], 25: [(ROW_B, "r")]}, g)
        parked = []

        def watch(eng, step, st, held):
            q = eng.copy_buffer("q_pos0", torch.int32, (2 * SLOTS,)).tolist()
            k = eng.copy_buffer("kv_start", torch.int32, (2 * SLOTS,)).tolist()
            parked.append((step, dict(held), [int(st[SLOTS + b]) for b in range(SLOTS)], q, k))
        res[("parking", g)] = (S.run({0: [(0, "o1"), (ROW_B, "first")]}, g, watch=watch), parked)      # (o1: EOS off, ends at its bound)
    yield res
    _release(gm)


def _same(a, b):
    return a[1] == b[1] and torch.equal(a[0], b[0])


def test_admission_time_invariance(served):
    """r admitted into row ROW_B of an idle engine at step 0 and into the same row at step 7 while three other prompts decode: the same
    codes and length.  Eager, and graph replayed with no recapture across the admission (Serving.run counts the captures)."""
    md = max(served["cfg"].codec_delay_pattern)
    for g in (False, True):
        alone, late = served[("alone", g)]["r"], served[("late", g)]["r"]
        print(f"{served['fmt']} graph={g}: r alone length {alone[1]} ended at step {alone[2]}; late length {late[1]} ended at step {late[2]}")
        assert alone[1] == REQ["r"][3]["max_tokens"] - md - 1 and alone[0].shape[0] == alone[1] + md
        assert _same(alone, late)
        assert late[2] == alone[2] + 7
    assert _same(served[("alone", False)]["r"], served[("alone", True)]["r"])


def test_admission_does_not_disturb_the_rows_already_decoding(served):
    for g in (False, True):
        quiet, late, reuse = served[("others", g)], served[("late", g)], served[("reuse", g)]
        for name in OTHERS.values():
            assert _same(quiet[name], late[name]) and quiet[name][2] == late[name][2], (g, name)
            assert _same(quiet[name], reuse[name]), (g, name)
        lengths = {n: quiet[n][1] for n in OTHERS.values()}
        print(f"{served['fmt']} graph={g}: lengths of the rows already decoding {lengths}")
        assert all(v[2] > 7 for v in quiet.values())               # they were all still decoding when r was admitted


def test_row_reuse_leaks_nothing(served):
    """two requests in turn through the same row: the second equals the idle-engine reference"""
    for g in (False, True):
        reuse = served[("reuse", g)]
        assert reuse["first"][2] < 25                               # the first request had ended before the second took its row
        assert _same(reuse["r"], served[("alone", g)]["r"]), g
        assert reuse["r"][2] == served[("alone", g)]["r"][2] + 25


def test_ended_row_is_parked(served):
    """after a row ends, q_pos0 == kv_start for its two cache rows at the next step (one key per layer); a live row's grows by one"""
    for g in (False, True):
        out, parked = served[("parking", g)]
        assert out["first"][2] + 3 < out["o1"][2]
        seen = 0
        prev = None
        for step, held, cd, q, k in parked:
            for b in range(SLOTS):
                if prev is not None and prev[b] == 0:
                    # countdown was 0 BEFORE this step's step_prep ran: parked
                    assert q[2 * b] == k[2 * b] and q[2 * b + 1] == k[2 * b + 1], (g, step, b, q, k)
                    seen += b == ROW_B
            if prev is not None and cd[0] != 0 and prev[0] != 0:
                assert q[0] == REQ["o1"][0] + step - 1, (g, step, q)       # t_prompt + n_dec of the live row 0
            prev = cd
        assert seen > 3, seen                                       # ROW_B after "first" ended, while row 0 still decoded
        # rows 1 and 3 were never used in this run: parked from the first step on (kv_start holds what an earlier use of the engine left)
        assert all(p[3][r] == p[4][r] for p in parked for r in (2, 3, 6, 7))


# ----------------------------------------------------------------------------- 5. against the existing path
@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
def test_admitted_row_equals_the_classic_batch_row(dev, fmt):
    """A classic start_decode batch on prompts padded to one T; row b's K / V slabs copied into a serving engine (admit_external): the
    decode tokens equal the classic row b's.  Then the 2-row admission prefill's slabs against the batch prefill's: T = 32 puts both
    on the tiled prefill kernels (64 and 256 tokens); bit-identical slabs => identical tokens through admit."""
    from test_gpu_engine import prompt
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    from unimoe_audio_amd.row_params import SETTINGS
    gm, cfg = _engine_model(fmt, dev)
    B, T, b = 4, 32, 2
    md = max(cfg.codec_delay_pattern)
    ids, am, codec = prompt(cfg, B, T, 6, [3, 0, 1, 0, 2, 5, 0, 4])
    pre, psteps = prepare_audio_prompt(cfg, [None] * B)
    x = gm.calculate_input_embedding(ids.to(dev), codec.to(dev)).reshape(B, 2 * T, cfg.hidden_size).contiguous()
    eng = gm.engine(B, T, MAXT, expert_weights=fmt)
    KVH, hd, Lmax, Lyr = cfg.num_key_value_heads, cfg.head_dim, eng.Lmax, cfg.num_hidden_layers
    shape = (Lyr, 2 * B, KVH, Lmax, hd)
    eng.prefill(x.reshape(-1, cfg.hidden_size), am.to(dev))
    k_ref = eng.copy_buffer("k_cache", torch.bfloat16, shape)[:, 2 * b:2 * b + 2, :, :T].clone()
    v_ref = eng.copy_buffer("v_cache", torch.bfloat16, shape)[:, 2 * b:2 * b + 2, :, :T].clone()
    kw = {k: [r[k] for r in MIXED] for k in SETTINGS}
    eng.start_decode(pre, psteps, kw.pop("max_tokens"), kw.pop("min_tokens"), **kw)
    eng.run(use_graph=True, poll_every=5)
    codes, lengths, _ = eng.finish()
    want = (codes[b][: int(lengths[b]) + md].cpu(), int(lengths[b]))

    def serve_row(external):
        eng.start_serving(T)
        zero = torch.zeros(shape, dtype=torch.bfloat16, device=dev)
        eng.write_buffer("k_cache", zero)
        eng.write_buffer("v_cache", zero)
        if external:
            per_row = KVH * Lmax * hd * 2
            slab = torch.zeros((2, KVH, Lmax, hd), dtype=torch.bfloat16, device=dev)
            for l in range(Lyr):
                for name, ref in (("k_cache", k_ref), ("v_cache", v_ref)):
                    slab[:, :, :T] = ref[l]
                    eng.write_buffer(name, slab, (l * 2 * B + 2 * b) * per_row)
        eng.admit(b, None if external else x[b], am[2 * b:2 * b + 2], pre[b], psteps[b], external=external, **MIXED[b])
        k_adm = eng.copy_buffer("k_cache", torch.bfloat16, shape)
        v_adm = eng.copy_buffer("v_cache", torch.bfloat16, shape)
        others = [r for r in range(2 * B) if r not in (2 * b, 2 * b + 1)]
        assert not bool(k_adm[:, others].any()) and not bool(v_adm[:, others].any())     # no other row's cache changed
        n = 0
        while True:
            eng.step(True)
            n += 1
            if eng.row_done(eng.poll(), b):
                break
            assert n < 200
        c, ln = eng.take(b)
        return (c.cpu(), ln), k_adm[:, 2 * b:2 * b + 2, :, :T], v_adm[:, 2 * b:2 * b + 2, :, :T]

    got, _, _ = serve_row(True)
    assert got[1] == want[1] and torch.equal(got[0], want[0])
    got2, k_adm, v_adm = serve_row(False)
    first = [int(am[2 * b + r].argmax()) for r in range(2)]      # left padding: slots below are the pad positions' keys, never read
    same = True
    for r in range(2):
        dk = (k_adm[:, r, :, first[r]:].float() - k_ref[:, r, :, first[r]:].float()).abs()
        dv = (v_adm[:, r, :, first[r]:].float() - v_ref[:, r, :, first[r]:].float()).abs()
        print(f"{fmt} cache row {2 * b + r}: max |dK| {float(dk.max()):.3e} max |dV| {float(dv.max()):.3e} (2-row admission prefill vs batch prefill)")
        same = same and float(dk.max()) == 0.0 and float(dv.max()) == 0.0
        # never beyond the per-op bf16 tolerance of the full-depth parity test: |a - b| <= 2^-6 |b| + 2^-8
        assert bool((dk <= 2.0 ** -6 * k_ref[:, r, :, first[r]:].float().abs() + 2.0 ** -8).all())
        assert bool((dv <= 2.0 ** -6 * v_ref[:, r, :, first[r]:].float().abs() + 2.0 ** -8).all())
    print(f"{fmt}: admission prefill slabs bit-identical to the batch prefill's: {same}")
    if same:
        assert got2[1] == want[1] and torch.equal(got2[0], want[0])
    _release(gm)


# ----------------------------------------------------------------------------- 9. refusals
def test_admit_refusals_enqueue_nothing(dev):
    from test_gpu_engine import prompt
    from unimoe_audio_amd._lib import UmoeError
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    gm, cfg = _engine_model("bf16", dev)
    S = Serving(gm, cfg, "bf16", dev)
    eng = S.engine()
    S.admit(eng, 0, "o0")
    for _ in range(3):
        eng.step(False)
    torch.cuda.synchronize()

    def snapshot():
        return [t.clone() for t in (eng.tokens, eng.state, eng.row_clock, eng.row_params, eng.copy_buffer("kv_start", torch.int32, (2 * SLOTS,)),
                                    eng.copy_buffer("valid_count", torch.int32, (2 * SLOTS,)), eng.copy_buffer("ep_words", torch.int32, (2,)))]

    before = snapshot()
    pre, ps = prepare_audio_prompt(cfg, [None])
    kw = REQ["r"][3]
    ids, am, codec = prompt(cfg, 1, MAX_PROMPT + 1, 3, [0, 0])
    big = gm.calculate_input_embedding(ids.to(dev), codec.to(dev)).reshape(-1, cfg.hidden_size).contiguous()
    with pytest.raises(UmoeError, match="larger than the reservation"):
        eng.admit(1, big, am, pre[0], ps[0], **kw)
    x, am_r = S.inputs["r"]
    with pytest.raises(UmoeError, match="3-D positions"):
        eng.admit(1, x, am_r, pre[0], ps[0], position_ids=torch.zeros(3, 2, am_r.shape[1], dtype=torch.long), **kw)
    with pytest.raises(UmoeError, match="outside the batch"):
        eng.admit(SLOTS, x, am_r, pre[0], ps[0], **kw)
    with pytest.raises(UmoeError, match="too small"):
        eng.admit(1, x, am_r, pre[0], ps[0], **dict(kw, max_tokens=eng.Tmax))
    # the C entry point refuses the oversized prompt itself, before anything is enqueued
    from unimoe_audio_amd import _lib as L
    import ctypes as C
    valid = am.to(torch.uint8).contiguous()
    rc = L.lib().umoe_engine_admit(eng.h, C.byref(eng.io), 1, big.data_ptr(), valid.data_ptr(), MAX_PROMPT + 1, ps[0], pre.shape[1], eng._stream())
    assert rc != 0 and b"larger than the reservation" in L.lib().umoe_last_error()
    # an expert-parallel engine: refused by the Python face and by the library
    eng.ep_size = 2
    with pytest.raises(UmoeError, match="expert-parallel"):
        eng.admit(1, x, am_r, pre[0], ps[0], **kw)
    with pytest.raises(UmoeError, match="expert-parallel"):
        eng.start_serving(MAX_PROMPT)
    eng.ep_size = 1
    after = snapshot()
    for a, c in zip(before, after):
        assert torch.equal(a, c)
    _release(gm)
    # a real expert-parallel engine (one rank of two, loopback link): the library refuses the reservation, the Python face the serving
    from unimoe_audio_amd.ep import EpLink
    try:
        ep_eng = gm.engine(2, MAX_PROMPT, MAXT, ep=EpLink(rank=0, size=2, mode="loopback"))
        rc = L.lib().umoe_engine_reserve(ep_eng.h, 2 * MAX_PROMPT)
        assert rc != 0 and b"expert parallel" in L.lib().umoe_last_error()
        with pytest.raises(UmoeError, match="expert-parallel"):
            ep_eng.start_serving(MAX_PROMPT)
    finally:
        _release(gm)


# ----------------------------------------------------------------------------- 8. the public API
def test_serve_equals_generate_batch_of_each_request_in_its_row(dev, tmp_path):
    """serve() on a queue of more than `slots` mixed speech / music requests: each wav equals, byte for byte, the wav generate_batch
    writes for that request alone -- a batch of `slots` copies of it, read at the row serve() put it in."""
    import wave
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
    slots = 2
    reqs = [MusicRequest("calm piano", max_audio_seconds=2, min_audio_seconds=1, seed=22),
            SpeechRequest("hello world", "the prompt text", src, max_audio_seconds=1, min_audio_seconds=0, seed=21),
            SpeechRequest("a second sentence", "the prompt text", src, max_audio_seconds=1, min_audio_seconds=1, seed=23, temperature=1.2),
            MusicRequest("fast drums", max_audio_seconds=1, min_audio_seconds=1, seed=24, save_name="drums"),
            SpeechRequest("the last one", "the prompt text", src, max_audio_seconds=1, min_audio_seconds=0, seed=25)]
    got = {}
    gen = app.serve(iter(reqs), slots=slots, output_dir=str(tmp_path / "served"), poll_every=8, max_prompt_tokens=256, max_audio_seconds=2)
    for index, path in gen:
        got[index] = path
    assert sorted(got) == list(range(len(reqs)))
    assert os.path.basename(got[3]) == "generated_drums_3.wav" and os.path.basename(got[0]) == "generated_music_0.wav"
    served_rows = dict(app.served_rows)                   # which row each request decoded in
    assert sorted(served_rows) == list(range(len(reqs))) and set(served_rows.values()) == set(range(slots))
    for i, r in enumerate(reqs):
        ref = app.generate_batch([r] * slots, output_dir=str(tmp_path / f"ref{i}"))
        assert open(got[i], "rb").read() == open(ref[served_rows[i]], "rb").read(), (i, served_rows[i])
    m._engine.close()
    m._engine = None
