"""The cases of tests/test_gpu_prefix.py, which runs them in child processes (this file's name keeps it out of the suite's own collection;
`python -m pytest tests/prefix_gpu_cases.py -m gpu` runs them directly).
GPU tests of prefix reuse across admissions: the install / extract kernel bit for bit, an admission behind a prefix store
built in the same call against one behind a store built earlier through another row (hit equals miss), row reuse, the split admission
against the one-shot admission within the tiled-against-ragged yardstick, refusals, and serve(prefix_cache=True)."""
import ctypes as C
import json
import types

import numpy as np
import pytest
import torch

from test_gpu_admit import OTHERS, REQ, ROW_B, Serving, _release, _same
from test_gpu_row_params import _engine_model

pytestmark = pytest.mark.gpu

SLOTS, MAX_PROMPT, MAXT = 4, 96, 64


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from unimoe_audio_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int16)


# ----------------------------------------------------------------------------- 1. the kernel
def prefix_copy(k, v, store, jobs, extract):
    from unimoe_audio_amd import _lib as L
    Lyr, rows, KVH, Lmax, hd = k.shape
    P = store.shape[3]
    j = torch.tensor(jobs, dtype=torch.int32).contiguous()
    rc = L.lib().umoe_kv_prefix_copy(k.data_ptr(), v.data_ptr(), store.data_ptr(), Lyr, rows, KVH, Lmax, hd, P, j.data_ptr(), len(jobs), int(extract),
                                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("P", (1, 63, 64, 65))
def test_install_and_extract_are_exact_and_touch_nothing_else(dev, P):
    """A store of random bf16 bit patterns installed into rows 2 and 3 of sentinel-filled slabs (3 layers, 6 rows, 2 kv heads, 100 slots)
    behind first_r pads, first_r in {0, 3, P + 2}: slots [first_r, P) hold store tokens [0, P - first_r) bit for bit, every other slot
    of the two rows and every slot of every other row keeps its sentinel; extracting the installed row returns the store."""
    Lyr, rows, KVH, Lmax, hd = 3, 6, 2, 100, 128
    g = torch.Generator().manual_seed(100 + P)
    rnd = lambda *s: torch.randint(-2 ** 15, 2 ** 15, s, generator=g, dtype=torch.int32).to(torch.int16).to(dev).view(torch.bfloat16)      # noqa: E731
    store = rnd(Lyr, 2, KVH, P, hd)
    k0, v0 = rnd(Lyr, rows, KVH, Lmax, hd), rnd(Lyr, rows, KVH, Lmax, hd)
    for firsts in ((0, 3), (3, 0), (P + 2, 0)):
        k, v = k0.clone(), v0.clone()
        jobs = [[2 + r, 0, f, max(P - f, 0)] for r, f in enumerate(firsts)]
        assert prefix_copy(k, v, store, jobs, 0) == 0
        wk, wv = k0.clone(), v0.clone()
        for r, f in enumerate(firsts):
            if P > f:
                wk[:, 2 + r, :, f:P] = store[:, 0, :, :P - f]
                wv[:, 2 + r, :, f:P] = store[:, 1, :, :P - f]
        assert torch.equal(bits(k), bits(wk)) and torch.equal(bits(v), bits(wv)), (P, firsts)
        r0 = 2 + firsts.index(0)
        back = torch.zeros_like(store)
        assert prefix_copy(k, v, back, [[r0, 0, 0, P]], 1) == 0
        assert torch.equal(bits(back), bits(store)), (P, firsts)
        assert torch.equal(bits(k), bits(wk)) and torch.equal(bits(v), bits(wv))           # an extract writes no cache slot
    # a middle piece, two pieces into one row: store tokens [i0, i0 + n) -> slots [s0, s0 + n)
    if P >= 63:
        k, v = k0.clone(), v0.clone()
        assert prefix_copy(k, v, store, [[5, 7, 40, 20], [5, 0, 90, 7], [0, P - 1, Lmax - 1, 1]], 0) == 0
        wk = k0.clone()
        wk[:, 5, :, 40:60], wk[:, 5, :, 90:97], wk[:, 0, :, Lmax - 1:] = store[:, 0, :, 7:27], store[:, 0, :, :7], store[:, 0, :, P - 1:]
        assert torch.equal(bits(k), bits(wk))
    # ranges outside the store or the slabs are refused on the host; nothing is launched
    from unimoe_audio_amd import _lib as L
    k, v = k0.clone(), v0.clone()
    for bad in ([[2, 0, Lmax - P + 1, P]], [[2, 1, 0, P]], [[rows, 0, 0, P]], [[2, -1, 0, 1]], [[2, 0, -1, 1]], [[2, 0, 0, P], [2, 0, P - 1, 1]]):
        assert prefix_copy(k, v, store, bad, 0) != 0, bad
        assert b"umoe_kv_prefix_copy" in L.lib().umoe_last_error()
    back = torch.zeros_like(store)
    assert prefix_copy(k, v, back, [[2, 0, 0, P], [3, 0, 0, P]], 1) != 0          # two extracts into the same store tokens
    assert b"overlap in the store" in L.lib().umoe_last_error()
    assert torch.equal(bits(k), bits(k0)) and torch.equal(bits(v), bits(v0)) and not bool(back.any())


# ----------------------------------------------------------------------------- requests behind a prefix
def make_req(gm, cfg, dev, P, rest, seed):
    """A CFG pair whose rows both begin with the same P random tokens (three of them audio placeholders when P >= 6) and go on with
    rest[r] tokens of their own; left padded to T = P + max(rest)."""
    g = torch.Generator().manual_seed(seed)
    prefix = torch.randint(1, 290, (P,), generator=g)
    codec = None
    if P >= 6:
        prefix[-5:-2] = cfg.codec_placeholder_value
        pc = torch.randint(0, 1024, (3, cfg.codec_channels), generator=g)
        codec = torch.cat([pc, pc]).to(dev)
    T = P + max(rest)
    ids, am = torch.zeros(2, T, dtype=torch.long), torch.zeros(2, T, dtype=torch.long)
    for r in range(2):
        row = torch.cat([prefix, torch.randint(1, 290, (rest[r],), generator=g)])
        ids[r, T - len(row):], am[r, T - len(row):] = row, 1
    x = gm.calculate_input_embedding(ids.to(dev), codec)
    full = [r for r in range(2) if rest[r] == max(rest)][0]
    D = cfg.hidden_size
    return types.SimpleNamespace(P=P, T=T, Tq=T - P, am=am, first=[T - P - rest[0], T - P - rest[1]], x_full=x.reshape(-1, D).contiguous(),
                                 x_prefix=x[full, :P].contiguous(), x_suffix=x[:, P:].reshape(-1, D).contiguous())


P_SET = dict(REQ["r"][3])                                  # EOS off (min_tokens 1000): ends at its bound of 30 tokens
LONG_SET = dict(REQ["first"][3])                           # ends after 20 tokens


class PServing(Serving):
    """test_gpu_admit's step-by-step driver on an engine reserved for 96-token prompts; request "p" is admitted behind a prefix store:
    one built before the run through row `prebuild` (a hit), or, with prebuild None, built in the admission itself through the row
    it goes into (a miss).  "long" is a 96-token request admitted in one piece."""

    def __init__(self, gm, cfg, fmt, dev):
        from test_gpu_engine import prompt
        super().__init__(gm, cfg, fmt, dev)
        self.p = make_req(gm, cfg, dev, 65, (14, 17), 41)             # T 82, pads (3, 0): prefix on the tiled path, 2 x 17 columns behind it
        ids, am, codec = prompt(cfg, 1, MAX_PROMPT, 26, [0, 5])
        self.inputs["long"] = (gm.calculate_input_embedding(ids.to(dev), codec.to(dev)).reshape(-1, cfg.hidden_size).contiguous(), am)
        self.prebuild, self.store, self.slabs = None, None, None

    def engine(self):
        eng = self.gm.engine(SLOTS, MAX_PROMPT, MAXT, expert_weights=self.fmt)
        eng.start_serving(MAX_PROMPT)
        self.store = None if self.prebuild is None else eng.build_prefix(self.prebuild, self.p.x_prefix)
        self.slabs = None
        return eng

    def admit(self, eng, row, name):
        if name == "p":
            if self.store is None:
                self.store = eng.build_prefix(row, self.p.x_prefix)
            eng.admit(row, self.p.x_suffix, self.p.am, self.pre[0], self.ps[0], prefix=self.store, prefix_len=self.p.P, **P_SET)
        else:
            x, am = self.inputs[name]
            eng.admit(row, x, am, self.pre[0], self.ps[0], **(LONG_SET if name == "long" else REQ[name][3]))

    def watch(self, eng, step, st, held):
        """the pair's K / V slabs over [0, T) once "p" is in (decode steps append behind T)"""
        if self.slabs is None and "p" in held.values():
            cfg = self.cfg
            shape = (cfg.num_hidden_layers, 2 * SLOTS, cfg.num_key_value_heads, eng.Lmax, cfg.head_dim)
            row = [r for r, n in held.items() if n == "p"][0]
            self.slabs = [eng.copy_buffer(n, torch.bfloat16, shape)[:, 2 * row:2 * row + 2, :, :self.p.T].clone() for n in ("k_cache", "v_cache")]

    def scenario(self, plan, use_graph, prebuild):
        self.prebuild = prebuild
        out = self.run(plan, use_graph, watch=self.watch)
        return out, self.slabs, self.store


@pytest.fixture(scope="module", params=["bf16", "fp8"])
def served(request, dev):
    fmt = request.param
    gm, cfg = _engine_model(fmt, dev)
    S = PServing(gm, cfg, fmt, dev)
    res = {"fmt": fmt, "cfg": cfg, "p": S.p}
    others = [(b, n) for b, n in OTHERS.items()]
    for g in (False, True):
        res[("miss", g)] = S.scenario({0: [(ROW_B, "p")]}, g, None)                              # store built in the admission, row 2, step 0, idle engine
        res[("quiet", g)] = S.scenario({0: others}, g, None)                                     # no admission
        res[("hit", g)] = S.scenario({0: others, 7: [(ROW_B, "p")]}, g, 0)                        # store built earlier through row 0; p joins at step 7
        res[("reuse", g)] = S.scenario({0: others + [(ROW_B, "long")], 25: [(ROW_B, "p")]}, g, 0)   # into the row a longer request just left
    yield res
    _release(gm)


def slabs_equal(a, b, p):
    """K and V of the pair bit for bit over [first_r, T) of each row"""
    for sa, sb in zip(a, b):
        for r in range(2):
            if not torch.equal(bits(sa[:, r, :, p.first[r]:]), bits(sb[:, r, :, p.first[r]:])):
                return False
    return True


def test_hit_equals_miss(served):
    """The same request behind a store built in the admission itself (row 2, step 0, idle engine) and behind a store built earlier through
    row 0, admitted at step 7 while three other rows decode: the same store, the same K / V slabs over [first_r, T), the same codes and
    length -- eager and graph, one capture per run (Serving.run counts them).  The installed slots hold the store bit for bit."""
    p = served["p"]
    md = max(served["cfg"].codec_delay_pattern)
    for g in (False, True):
        (m_out, m_slabs, m_store), (h_out, h_slabs, h_store) = served[("miss", g)], served[("hit", g)]
        assert torch.equal(bits(m_store), bits(h_store))                       # the store depends on the prefix and the weights only
        assert slabs_equal(m_slabs, h_slabs, p), g
        for kv in range(2):
            for r in range(2):
                n = p.P - p.first[r]
                assert torch.equal(bits(h_slabs[kv][:, r, :, p.first[r]:p.P]), bits(h_store[:, kv, :, :n])), (g, kv, r)
        miss, hit = m_out["p"], h_out["p"]
        print(f"{served['fmt']} graph={g}: p miss length {miss[1]} ended at step {miss[2]}; hit length {hit[1]} ended at step {hit[2]}")
        assert miss[1] == P_SET["max_tokens"] - md - 1 and _same(miss, hit) and hit[2] == miss[2] + 7
    assert _same(served[("miss", False)][0]["p"], served[("miss", True)][0]["p"])
    assert slabs_equal(served[("miss", False)][1], served[("miss", True)][1], p)


def test_prefix_admission_does_not_disturb_the_rows_already_decoding(served):
    for g in (False, True):
        quiet, hit, reuse = served[("quiet", g)][0], served[("hit", g)][0], served[("reuse", g)][0]
        for name in OTHERS.values():
            assert _same(quiet[name], hit[name]) and quiet[name][2] == hit[name][2], (g, name)
            assert _same(quiet[name], reuse[name]), (g, name)
        assert all(v[2] > 7 for v in quiet.values())               # they were all still decoding when p was admitted


def test_prefix_admission_into_a_reused_row(served):
    """p into the row a 96-token request just left: the idle-engine result (nothing of the longer prompt's slots is read)"""
    p = served["p"]
    for g in (False, True):
        out, slabs, _ = served[("reuse", g)]
        assert out["long"][2] < 25
        assert _same(out["p"], served[("miss", g)][0]["p"]) and out["p"][2] == served[("miss", g)][0]["p"][2] + 25
        assert slabs_equal(slabs, served[("miss", g)][1], p)


# ----------------------------------------------------------------------------- 2b. the slab geometry at every shape
@pytest.mark.parametrize("P,rest", [(1, (2, 2)), (5, (15, 12)), (63, (16, 13)), (64, (17, 14)), (65, (14, 17)), (5, (3, 12)), (64, (2, 5))])
def test_build_install_geometry(dev, P, rest):
    """Sentinel slabs, a store built through row 0, sentinels again, then the admission into row 2: slots [first_r, P) of cache rows 4, 5
    hold the store bit for bit, slots [P, T) were written, slots below min(first_r, P) and from T on and every other row keep the
    sentinel.  P on both sides of the tiled threshold, Tq 2 .. 17, pads (0, 0), (3, 0), (0, 3) and a pad larger than P ((5, (3, 12)):
    first 9 > 5)."""
    gm, cfg = _engine_model("bf16", dev)
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    from unimoe_audio_amd.prefix_plan import prefix_plan
    pre, ps = prepare_audio_prompt(cfg, [None])
    q = make_req(gm, cfg, dev, P, rest, 50 + P)
    plan = prefix_plan(q.am, P)
    assert plan.first == q.first
    eng = gm.engine(SLOTS, MAX_PROMPT, MAXT, expert_weights="bf16")
    eng.start_serving(MAX_PROMPT)
    shape = (cfg.num_hidden_layers, 2 * SLOTS, cfg.num_key_value_heads, eng.Lmax, cfg.head_dim)
    sent = torch.full(shape, -3.0, dtype=torch.bfloat16, device=dev)
    store = eng.build_prefix(0, q.x_prefix)
    eng.write_buffer("k_cache", sent)
    eng.write_buffer("v_cache", sent)
    eng.admit(2, q.x_suffix, q.am, pre[0], ps[0], prefix=store, prefix_len=P, **P_SET)
    for kv, name in enumerate(("k_cache", "v_cache")):
        got = eng.copy_buffer(name, torch.bfloat16, shape)
        rest_rows = [r for r in range(2 * SLOTS) if r not in (4, 5)]
        assert torch.equal(got[:, rest_rows], sent[:, rest_rows]), name
        for r in range(2):
            f = q.first[r]
            i0, s0, n = plan.install[r]
            assert (i0, s0, n) == (0, f, max(P - f, 0))
            assert torch.equal(bits(got[:, 4 + r, :, s0:s0 + n]), bits(store[:, kv, :, i0:i0 + n])), (name, r)
            assert torch.equal(got[:, 4 + r, :, :min(f, P)], sent[:, 4 + r, :, :min(f, P)]), (name, r)
            assert torch.equal(got[:, 4 + r, :, q.T:], sent[:, 4 + r, :, q.T:]), (name, r)
            assert not bool((got[:, 4 + r, :, P:q.T] == -3.0).all(-1).any()), (name, r)          # every slot from P on was written
    assert eng.copy_buffer("kv_start", torch.int32, (2 * SLOTS,)).tolist()[4:6] == q.first
    assert eng.copy_buffer("valid_count", torch.int32, (2 * SLOTS,)).tolist()[4:6] == plan.valid_count
    # extract of the installed full row returns the store
    full = q.first.index(0)
    back = torch.zeros_like(store)
    k = eng.copy_buffer("k_cache", torch.bfloat16, shape)
    v = eng.copy_buffer("v_cache", torch.bfloat16, shape)
    assert prefix_copy(k, v, back, [[4 + full, 0, 0, P]], 1) == 0
    assert torch.equal(bits(back), bits(store))
    _release(gm)


def test_one_token_prefix_against_the_first_token_of_a_longer_one(dev):
    """P = 1 takes the one-token launches (rope fused into the attention kernel, one row).  Attention is causal, so the K / V of token 0
    do not depend on what follows: the store of a 1-token prefix against token 0 of the 5-token store of the same first token, within the
    per-op bf16 bound the admission tests use between GEMM paths, |a - b| <= 2^-6 |b| + 2^-8."""
    gm, cfg = _engine_model("bf16", dev)
    q = make_req(gm, cfg, dev, 5, (3, 3), 61)
    eng = gm.engine(SLOTS, MAX_PROMPT, MAXT, expert_weights="bf16")
    eng.start_serving(MAX_PROMPT)
    s5 = eng.build_prefix(0, q.x_prefix)[:, :, :, 0].float()
    s1 = eng.build_prefix(1, q.x_prefix[:1].contiguous())[:, :, :, 0].float()
    d = (s1 - s5).abs()
    print(f"one-token prefix: max |d| {float(d.max()):.3e} against max |ref| {float(s5.abs().max()):.3e}")
    assert bool(s5.abs().max() > 0.01)
    assert bool((d <= 2.0 ** -6 * s5.abs() + 2.0 ** -8).all())
    _release(gm)


def test_engine_held_while_its_model_is_dropped(dev):
    """model.engine() hands out an engine that refers to its model weakly (no model <-> engine cycle) and keeps every tensor it points
    to.  Held while the model is dropped -- the model is gone at once, its freed memory is emptied from the cache and other tensors are
    written over what comes back -- the engine admits in one piece, builds a prefix, admits behind it and decodes to the codes it gave
    with the model alive.  Only what runs the module's own forward needs the model, and says so."""
    import gc
    import weakref
    from test_gpu_engine import prompt
    from unimoe_audio_amd._lib import UmoeError
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    gm, cfg = _engine_model("bf16", dev)
    pre, ps = prepare_audio_prompt(cfg, [None])
    q = make_req(gm, cfg, dev, 65, (14, 17), 41)
    T, pads, seed, o_set = REQ["o0"]
    ids, o_am, codec = prompt(cfg, 1, T, seed, pads)
    o_x = gm.calculate_input_embedding(ids.to(dev), codec.to(dev)).reshape(-1, cfg.hidden_size).contiguous()

    def serve_two(eng):
        eng.start_serving(MAX_PROMPT)
        eng.admit(0, o_x, o_am, pre[0], ps[0], **o_set)
        store = eng.build_prefix(ROW_B, q.x_prefix)
        eng.admit(ROW_B, q.x_suffix, q.am, pre[0], ps[0], prefix=store, prefix_len=q.P, **P_SET)
        out, n = {}, 0
        while len(out) < 2:
            eng.step(True)
            n += 1
            st = eng.poll()
            for b in (0, ROW_B):
                if b not in out and eng.row_done(st, b):
                    codes, length = eng.take(b)
                    out[b] = (codes.cpu(), length)
            assert n < 200
        return out

    eng = gm.engine(SLOTS, MAX_PROMPT, MAXT, expert_weights="bf16")
    assert eng.model is gm
    want = serve_two(eng)
    n_bytes = sum(p.numel() * p.element_size() for p in gm.parameters())
    ref = weakref.ref(gm)
    gc.disable()
    try:
        del gm
        assert ref() is None                                   # no cycle: gone without a collection
    finally:
        gc.enable()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    junk = [torch.full((n_bytes // 8,), 7.0, dtype=torch.bfloat16, device=dev) for _ in range(4)]      # as many bytes as the model had
    with pytest.raises(UmoeError, match="is gone"):
        eng.model
    got = serve_two(eng)
    for b in (0, ROW_B):
        assert got[b][1] == want[b][1] and torch.equal(got[b][0], want[b][0]), b
    assert eng.handoff_error() == 0
    del junk
    eng.close()
    torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- 4. against the one-shot admission
def rel_l2(a, b):
    return float((a - b).norm() / b.norm())


def near_tie(z, top_p, tol):
    """z [n, n_dyn] fp32 gate logits of the dynamic experts; True where a perturbation of every logit by at most tol can change the top-P
    selection: two logits within 2 tol of each other (their order can flip), or a cumulative probability of the sorted softmax within
    2 tol of the threshold (softmax is 2-Lipschitz in the sup norm of the logits, and a cumulative sum of probabilities is at most 1)."""
    s, _ = z.sort(-1, descending=True)
    gap = (s[:, :-1] - s[:, 1:]).min(-1).values
    c = torch.softmax(s, -1).cumsum(-1)
    thr = float(torch.tensor(top_p).to(torch.bfloat16))
    return (gap <= 2 * tol) | ((c - thr).abs().min(-1).values <= 2 * tol)


@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
def test_split_admission_against_the_one_shot_admission(dev, fmt, monkeypatch):
    """The same request admitted in one piece (2 x 82 tokens, the tiled prefill) and behind its 65-token prefix (the prefix alone tiled,
    2 x 17 columns ragged): not bit-identical by construction -- the GEMM path changes with the token count and the attention's 64-key
    steps fall elsewhere -- so the first decode step's logits are compared in relative L2, and the yardstick is the one of
    test_gpu_w12_prefill / test_gpu_fp8_prefill: the one-shot admission on the engine's tiled against its ragged prefill path
    (UMOE_TILED_PREFILL).  The split may be at most 2x that far from the one-shot admission: it reorders the GEMM sums AND the attention's
    online-softmax blocks, each a reordering of the same fp32 sums and bf16 roundings.
    Routing: the expert masks of every layer for the columns behind the prefix equal the one-shot admission's wherever the one-shot gate
    logits are not near a selection tie (near_tie, with tol = the yardstick x the token's logit norm, at least one bf16 step of its
    largest logit); at most 1 % of (token, layer) cases may be set aside on that ground, in the split comparison and in the yardstick
    pair compared with itself.
    Measured on MI355X: see DESIGN 4n."""
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    gm, cfg = _engine_model(fmt, dev)
    pre, ps = prepare_audio_prompt(cfg, [None])
    q = make_req(gm, cfg, dev, 65, (14, 17), 41)
    Lyr, E, nd = cfg.num_hidden_layers, cfg.num_experts, cfg.num_dyn
    CV = cfg.codec_channels * cfg.codec_vocab_size

    def first_step(split):
        eng = gm.engine(SLOTS, MAX_PROMPT, MAXT, expert_weights=fmt)
        eng.start_serving(MAX_PROMPT)
        store = eng.build_prefix(0, q.x_prefix) if split else None
        dump = eng.set_admit_dump(2 * MAX_PROMPT)
        if split:
            eng.admit(ROW_B, q.x_suffix, q.am, pre[0], ps[0], prefix=store, prefix_len=q.P, **P_SET)
            n = q.Tq
        else:
            eng.admit(ROW_B, q.x_full, q.am, pre[0], ps[0], **P_SET)
            n = q.T
        mask = dump["mask"][:, :2 * n].reshape(Lyr, 2, n, E)[:, :, n - q.Tq:].clone().cpu()
        gate = dump["logits"][:, :2 * n].reshape(Lyr, 2, n, E)[:, :, n - q.Tq:].float().cpu()
        eng.set_admit_dump()
        eng.step(False)
        logits = eng.copy_buffer("logits", torch.float32, (2 * SLOTS, CV))[2 * ROW_B:2 * ROW_B + 2].cpu()
        assert eng.handoff_error() == 0
        return logits, mask, gate

    one, m_one, z_one = first_step(False)
    spl, m_spl, _ = first_step(True)
    _release(gm)
    monkeypatch.setenv("UMOE_TILED_PREFILL", "0")
    rag, m_rag, _ = first_step(False)
    _release(gm)
    monkeypatch.delenv("UMOE_TILED_PREFILL")
    yard, got = rel_l2(one, rag), rel_l2(spl, one)
    valid = q.am[:, q.P:].bool()                                            # (pad columns behind the prefix route too; nothing reads them)
    z = z_one[..., :nd]
    tol = torch.maximum(yard * z.norm(dim=-1), 2.0 ** -8 * z.abs().amax(-1))
    tie = near_tie(z.reshape(-1, nd), cfg.mlp_dynamic_top_p, tol.reshape(-1)).reshape(Lyr, 2, q.Tq)
    cases = int(valid.sum()) * Lyr
    rec = {"fmt": fmt, "split_vs_one_shot_rel_l2": got, "yardstick_tiled_vs_ragged_rel_l2": yard, "cases": cases}
    for name, m in (("split", m_spl), ("ragged", m_rag)):
        differ = (m != m_one).any(-1) & valid[None]
        rec[name + "_masks_differ"] = int(differ.sum())
        rec[name + "_set_aside"] = int((differ & tie).sum())
        rec[name + "_differ_away_from_a_tie"] = int((differ & ~tie).sum())
    print("split admission:", json.dumps(rec))
    assert yard > 0.0, rec
    assert got <= 2 * yard, rec
    for name in ("split", "ragged"):
        assert rec[name + "_differ_away_from_a_tie"] == 0, rec
        assert rec[name + "_set_aside"] <= 0.01 * cases, rec


# ----------------------------------------------------------------------------- 5. refusals
def test_prefix_refusals_enqueue_nothing(dev):
    from unimoe_audio_amd import _lib as L
    from unimoe_audio_amd._lib import UmoeError
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    gm, cfg = _engine_model("bf16", dev)
    S = PServing(gm, cfg, "bf16", dev)
    eng = S.engine()
    S.admit(eng, 0, "o0")
    q = S.p
    store = eng.build_prefix(1, q.x_prefix)
    for _ in range(3):
        eng.step(False)
    torch.cuda.synchronize()
    shape = (cfg.num_hidden_layers, 2 * SLOTS, cfg.num_key_value_heads, eng.Lmax, cfg.head_dim)

    def snapshot():
        return [t.clone() for t in (eng.tokens, eng.state, eng.row_clock, eng.row_params, eng.copy_buffer("kv_start", torch.int32, (2 * SLOTS,)),
                                    eng.copy_buffer("valid_count", torch.int32, (2 * SLOTS,)), eng.copy_buffer("ep_words", torch.int32, (2,)),
                                    bits(eng.copy_buffer("k_cache", torch.bfloat16, shape)), bits(eng.copy_buffer("v_cache", torch.bfloat16, shape)))]

    before = snapshot()
    pre, ps = prepare_audio_prompt(cfg, [None])
    n_pre = int(pre.shape[1])
    valid = q.am.to(torch.uint8).contiguous()

    def c_admit(P, T, st=store, v=valid, x=q.x_suffix):
        rc = L.lib().umoe_engine_admit_prefix(eng.h, C.byref(eng.io), 2, None if st is None else st.data_ptr(), P, x.data_ptr(), v.data_ptr(), T, ps[0],
                                              n_pre, eng._stream())
        return rc, L.lib().umoe_last_error()

    def c_build(P, st=store, b=2):
        rc = L.lib().umoe_engine_prefix_build(eng.h, C.byref(eng.io), b, q.x_prefix.data_ptr(), P, None if st is None else st.data_ptr(), eng._stream())
        return rc, L.lib().umoe_last_error()

    hole = valid.clone()
    hole[1, 10] = 0                                                          # a prefix token of row 1 is masked: not what the store holds
    wide = torch.ones(2, 2 * MAX_PROMPT + 8, dtype=torch.uint8)
    for (rc, msg), want in ((c_admit(q.T - 1, q.T), b"2 <= T - P"), (c_admit(0, q.T), b"1 <= P"), (c_admit(-1, q.T), b"1 <= P"),
                            (c_admit(q.P, q.T, st=None), b"null prefix store"), (c_admit(2 * MAX_PROMPT + 1, 2 * MAX_PROMPT + 8, v=wide), b"reservation"),
                            (c_admit(q.P, q.T, v=hole), b"left-padded"), (c_build(0), b"1 <= P"), (c_build(q.P, st=None), b"null prefix store"),
                            (c_build(2 * MAX_PROMPT + 1), b"reservation"), (c_build(q.P, b=SLOTS), b"outside the batch")):
        assert rc != 0 and want in msg, (want, msg)
    # a row with more valid tokens below column P than the install covers cannot be built from a left-padded mask; the Python face
    # refuses the same things before it writes the row's settings or tokens
    kw = dict(prefix=store, prefix_len=q.P, **P_SET)
    with pytest.raises(UmoeError, match="2 <= T - P"):
        eng.admit(2, q.x_suffix, q.am, pre[0], ps[0], **dict(kw, prefix_len=q.T - 1))
    with pytest.raises(UmoeError, match="prefix store"):
        eng.admit(2, q.x_suffix, q.am, pre[0], ps[0], **dict(kw, prefix=None))
    with pytest.raises(UmoeError, match="prefix store"):
        eng.admit(2, q.x_suffix, q.am, pre[0], ps[0], **dict(kw, prefix_len=q.P - 1))      # the store is not one of P - 1 tokens
    with pytest.raises(UmoeError, match="left-padded"):
        eng.admit(2, q.x_suffix, hole.long(), pre[0], ps[0], **kw)
    with pytest.raises(UmoeError, match="embeddings of columns"):
        eng.admit(2, q.x_full, q.am, pre[0], ps[0], **kw)
    with pytest.raises(UmoeError, match="reservation"):
        eng.build_prefix(2, torch.zeros(MAX_PROMPT + 1, cfg.hidden_size, dtype=torch.bfloat16, device=dev))
    # the per-layer probe
    eng.set_probe(dump_x=True)
    for rc, msg in (c_admit(q.P, q.T), c_build(q.P)):
        assert rc != 0 and b"per-layer probe" in msg
    eng.set_probe()
    # an expert-parallel engine: refused by the Python face ...
    eng.ep_size = 2
    with pytest.raises(UmoeError, match="expert-parallel"):
        eng.admit(2, q.x_suffix, q.am, pre[0], ps[0], **kw)
    with pytest.raises(UmoeError, match="expert-parallel"):
        eng.build_prefix(2, q.x_prefix)
    eng.ep_size = 1
    after = snapshot()
    for i, (a, c) in enumerate(zip(before, after)):
        assert torch.equal(a, c), i
    # ... and, on a real one (one rank of two, loopback link), by the library
    _release(gm)
    from unimoe_audio_amd.ep import EpLink
    try:
        ep_eng = gm.engine(2, MAX_PROMPT, MAXT, ep=EpLink(rank=0, size=2, mode="loopback"))
        io = L.DecodeIO(tokens=eng.tokens.data_ptr(), state=eng.state.data_ptr(), row_clock=eng.row_clock.data_ptr())
        st2 = torch.zeros(ep_eng.prefix_store_shape(q.P), dtype=torch.bfloat16, device=dev)
        rc = L.lib().umoe_engine_prefix_build(ep_eng.h, C.byref(io), 0, q.x_prefix.data_ptr(), q.P, st2.data_ptr(), ep_eng._stream())
        assert rc != 0 and b"expert parallel" in L.lib().umoe_last_error()
        rc = L.lib().umoe_engine_admit_prefix(ep_eng.h, C.byref(io), 0, st2.data_ptr(), q.P, q.x_suffix.data_ptr(), valid.data_ptr(), q.T, ps[0], n_pre,
                                              ep_eng._stream())
        assert rc != 0 and b"expert parallel" in L.lib().umoe_last_error()
        assert not bool(st2.any())
    finally:
        _release(gm)


# ----------------------------------------------------------------------------- 6. the public API
def test_serve_with_the_prefix_cache(dev, tmp_path):
    """Six speech requests in two voices on 4 slots: 2 misses and 4 hits, and every request's codes equal those of the same request
    served with the prefix cache as the only one of its voice (a miss), in the same row (music requests in front hold the rows below
    it).  With the cache off nothing is split.  (serve() without the cache against generate_batch: test_gpu_admit, unchanged.)"""
    import wave
    from test_gpu_api import StandInTokenizer
    from test_gpu_stream import _app, _tiny_model
    from unimoe_audio_amd.api import MusicRequest, SpeechRequest
    m = _tiny_model(dev)
    app = _app(m, dev)
    app._tokenizer = StandInTokenizer(m.config.codec_placeholder_value)
    wavs = []
    for i, hz in enumerate((220, 330)):
        t = np.arange(4800 + 1600 * i) / 16000
        wavs.append(str(tmp_path / f"voice{i}.wav"))
        with wave.open(wavs[-1], "wb") as wf:
            wf.setnchannels(1); wf.setsampwidth(2); wf.setframerate(16000)
            wf.writeframes((0.3 * np.sin(2 * np.pi * hz * t) * 32767).astype("<i2").tobytes())
    texts = ["hello world", "a second sentence, longer than the first", "short", "the fourth one", "five", "and the last sentence of all"]
    reqs = [SpeechRequest(tx, f"the prompt text {i % 2}", wavs[i % 2], max_audio_seconds=1, min_audio_seconds=0, seed=21 + i, temperature=1.0 + 0.1 * (i % 3))
            for i, tx in enumerate(texts)]
    kw = dict(slots=SLOTS, output_dir=None, poll_every=8, max_prompt_tokens=256, max_audio_seconds=1)
    got = dict(app.serve(iter(reqs), prefix_cache=True, **kw))
    assert sorted(got) == list(range(6))
    sp, rows = dict(app.served_prefix), dict(app.served_rows)
    assert sorted(sp) == list(range(6))
    assert [sp[i][0] for i in range(6)] == [False, False, True, True, True, True], sp       # 2 misses, 4 hits
    assert all(P > 20 for _, P in sp.values()), sp
    assert len({sp[i][1] for i in (0, 2, 4)}) == 1 and len({sp[i][1] for i in (1, 3, 5)}) == 1 and sp[0][1] != sp[1][1]
    print("served_prefix", sp, "rows", rows)
    filler = MusicRequest("calm piano", max_audio_seconds=1, min_audio_seconds=1, seed=5)
    for i, r in enumerate(reqs):
        alone = dict(app.serve([filler] * rows[i] + [r], prefix_cache=True, **kw))
        assert app.served_prefix[rows[i]] == (False, sp[i][1]) and app.served_rows[rows[i]] == rows[i]
        assert torch.equal(alone[rows[i]].cpu(), got[i].cpu()), (i, rows[i])
    # an explicit voice: the same stores, whatever the switch says; no reference audio in the request
    voice = app.voice("the prompt text 0", wavs[0])
    r0 = SpeechRequest(texts[0], "the prompt text 0", voice=voice, max_audio_seconds=1, min_audio_seconds=0, seed=21, temperature=1.0)
    again = dict(app.serve([r0, r0], **kw))
    assert app.served_prefix == {0: (False, sp[0][1]), 1: (True, sp[0][1])}
    assert torch.equal(again[0].cpu(), got[0].cpu())                       # request 0 decoded in row 0
    assert rows[0] == 0
    off = dict(app.serve(reqs[:2], **kw))
    assert app.served_prefix == {0: (False, 0), 1: (False, 0)} and sorted(off) == [0, 1]
    m._engine.close()
    m._engine = None
