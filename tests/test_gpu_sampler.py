"""GPU tests of the codec-token sampler, cfg_sample_kernel (umoe_misc.hip), against the host restatement in oracle/decode.py: every
draw (mix64 / sampler_u / draw on the kernel's own probabilities), the filtered distribution (filter_probs, float64), the statistics
of many draws, and the seed / step / min_tokens plumbing of a decode engine step, eager and in the captured step graph."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import decode as OD

pytestmark = pytest.mark.gpu

FAST_K = (1, 5, 45, 64)
SLOW_K = (None, 65, 100, 1027, "over")       # "over": V + 5
TEMPS = (0.3, 1.0, 1.2, 2.0)
VS = (2, 7, 1027, 2048)
U_ONE_SEED = 17974134                        # sampler_u(U_ONE_SEED, 0, 0) == 1.0 (tests/test_sampler_cpu.py)
TINY = 1e-37                                 # float64 probabilities below this may underflow to 0 in the kernel's fp32 softmax


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from unimoe_audio_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def eos_of(V):
    return 1 if V == 2 else V - 3            # 1024 of 1027 in the model


def path_of(top_k):
    return "fast" if top_k is not None and 0 < top_k <= 64 else "slow"


def f32(v):
    return float(np.float32(v))              # the kernel's arguments are fp32


def grid_logits(R, V, gen, scale=2.0):
    """[R, V] on a 2^-10 grid in [-15, 15]: the CFG mix (co + s (co - un), s in {0, 3}) is exact in fp32 and in float64, and
    dividing by the temperature keeps the order, so the kernel and the float64 restatement rank the same values."""
    x = (torch.randn(R, V, generator=gen) * scale).clamp(-15, 15)
    return torch.round(x * 1024) / 1024


def pack(co, un, C):
    """co / un [B*C, V] -> the kernel's logits [2B, C, V] (row 2b = uncond, 2b + 1 = cond)"""
    R, V = co.shape
    return torch.stack([un.view(R // C, C, V), co.view(R // C, C, V)], 1).reshape(2 * (R // C), C, V).contiguous()


class Tally:
    def __init__(self):
        self.rows = self.near_top_p = self.near_cdf = 0

    def bound(self):
        assert self.rows > 0
        assert self.near_top_p <= 0.001 * self.rows, (self.near_top_p, self.rows)
        assert self.near_cdf <= 0.001 * self.rows, (self.near_cdf, self.rows)


def sample(dev, lg, *, cfg_scale, T, top_p, top_k, eos_mul=0.75, seed=0, step=None, min_tokens=None, enable_eos=True,
           do_sample=True, want_probs=True):
    from unimoe_audio_amd import ops
    twoB, C, V = lg.shape
    st = None if step is None else torch.tensor([step], dtype=torch.int32, device=dev)
    out = ops.cfg_sample(lg.reshape(twoB, C * V).to(dev), twoB // 2, C, V, cfg_scale=cfg_scale, temperature=T, top_p=top_p,
                         top_k=top_k, eos=eos_of(V), eos_mul=eos_mul, enable_eos=enable_eos, do_sample=do_sample, seed=seed,
                         want_probs=want_probs, step=st, min_tokens=min_tokens)
    return out


def check(dev, lg, tally, *, cfg_scale, T, top_p, top_k, eos_mul=0.75, seed=0, step=None, min_tokens=None, enable_eos=True):
    """One launch with probs_out: (b) support and values against filter_probs, (a) every draw against draw(probs_out, sampler_u)."""
    twoB, C, V = lg.shape
    pred, probs = sample(dev, lg, cfg_scale=cfg_scale, T=T, top_p=top_p, top_k=top_k, eos_mul=eos_mul, seed=seed, step=step,
                         min_tokens=min_tokens, enable_eos=enable_eos)
    en = enable_eos if step is None else (min_tokens is None or step >= min_tokens)
    ref, cand, gap = OD.filter_probs(lg, cfg_scale, f32(T), f32(top_p), top_k, eos_of(V), f32(eos_mul), en, details=True)
    got = probs.cpu()
    pred = pred.cpu().reshape(-1).numpy()
    u = OD.sampler_u(seed, 0 if step is None else step, np.arange(twoB // 2 * C))
    path = path_of(top_k)
    what = dict(V=V, cfg=cfg_scale, T=T, top_p=top_p, top_k=top_k, seed=seed, step=step, en=en)
    for r in range(got.shape[0]):
        tally.rows += 1
        g, f = got[r], ref[r]
        assert bool((g >= 0).all()) and abs(float(g.double().sum()) - 1.0) < 1e-5, (what, r)
        if float(gap[r]) < 1e-6:             # a top-p prefix sum within 1e-6 of top_p: fp32 may decide it the other way
            tally.near_top_p += 1
        else:
            sure = f > TINY
            assert torch.equal((g > 0)[sure], sure[sure]) and not bool(((g > 0) & (f == 0)).any()), \
                (what, r, torch.nonzero((g > 0) != (f > 0)).flatten().tolist()[:8])
            assert torch.allclose(g.double(), f, rtol=1e-4, atol=TINY), (what, r, float(((g.double() - f).abs() / f.clamp(min=TINY)).max()))
        lanes = None
        if path == "fast":
            lanes = torch.nonzero(cand[r]).flatten().numpy()
            assert len(lanes) == min(top_k, V)
        want, margin = OD.draw(g.numpy(), u[r], path, lanes=lanes, margin=True)
        if int(pred[r]) != want:
            # the slow path's sum is restated exactly; the fast path's lanes only when the candidate set matches
            assert path == "fast" and margin < 1e-6, (what, r, int(pred[r]), want, float(u[r]), margin)
            tally.near_cdf += 1
    return pred, got


# ----------------------------------------------------------------------------- the grid: (a) exact draws, (b) distribution
def _grid(dev, V, ks):
    gen = torch.Generator().manual_seed(1000 + V)
    B, C = 8, 12
    tally = Tally()
    n = 0
    for top_k in ks:
        k = V + 5 if top_k == "over" else top_k
        for top_p in ((1.0, 0.95, 1e-4) if path_of(k) == "fast" else (1.0, 0.5)):
            for T in TEMPS:
                for cfg_scale in (0.0, 3.0):
                    co, un = grid_logits(B * C, V, gen), grid_logits(B * C, V, gen)
                    lg = pack(co, un, C)
                    # alternate: no step pointer (step 0 in the hash, host EOS flag) / a device step, EOS on / off by min_tokens
                    if n % 3 == 0:
                        kw = dict(seed=U_ONE_SEED if n % 2 == 0 else n, step=None)          # U_ONE_SEED: row 0 draws u == 1.0
                    elif n % 3 == 1:
                        kw = dict(seed=n * 7919, step=3 + 11 * n, min_tokens=None)
                    else:
                        kw = dict(seed=2 ** 63 + n, step=5 + n, min_tokens=6 + n if n % 2 else 5 + n)
                    check(dev, lg, tally, cfg_scale=cfg_scale, T=T, top_p=top_p, top_k=k, **kw)
                    n += 1
    tally.bound()


@pytest.mark.parametrize("V", VS)
def test_fast_path_grid(dev, V):
    """0 < top_k <= 64: radix select, one-wave top-p / softmax / scan / pick."""
    _grid(dev, V, FAST_K)


@pytest.mark.parametrize("V", VS)
def test_slow_path_grid(dev, V):
    """no top-k or top_k > 64 (65 against 64 pins the switch): rank filter, block softmax, sequential inverse CDF."""
    _grid(dev, V, SLOW_K)


# ----------------------------------------------------------------------------- ties, +-0, masked rows
def _tie_rows(R, V, k, gen, n_eq=10):
    """k - 5 distinct values above, then n_eq equal values at scattered indices: the k-th position falls inside the tie"""
    eos = eos_of(V)
    co = -1 - 9 * torch.rand(R, V, generator=gen)
    co = torch.round(co * 1024) / 1024
    for r in range(R):
        idx = torch.randperm(eos, generator=gen)[: k - 5 + n_eq]
        co[r, idx[: k - 5]] = 2 + torch.randperm(k - 5, generator=gen).float() / 8
        co[r, idx[k - 5:]] = 1.0
    return co


@pytest.mark.parametrize("V", (1027, 2048))
def test_ties_straddling_the_kth_position(dev, V):
    gen = torch.Generator().manual_seed(7)
    C, tally = 12, Tally()
    for k in (5, 45, 100):
        co = _tie_rows(48, V, k, gen)
        for cfg_scale, un in ((0.0, torch.zeros_like(co)), (3.0, co * 0.5)):      # un = co / 2: the mix keeps every tie
            for top_p, T in ((1.0, 1.0), (0.95, 1.2)):
                check(dev, pack(co, un, C), tally, cfg_scale=cfg_scale, T=T, top_p=top_p, top_k=k, seed=k, step=k)
    tally.bound()


def test_all_equal_logits(dev):
    C, tally = 12, Tally()
    for V in (7, 1027, 2048):
        co = torch.full((24, V), 0.5)
        for k in (5, 45, 64, None, 100):
            for top_p in (1.0, 0.937):               # no prefix sum of equal probabilities lands on top_p
                for cfg_scale in (0.0, 3.0):
                    pred, got = check(dev, pack(co, co.clone(), C), tally, cfg_scale=cfg_scale, T=1.2, top_p=top_p, top_k=k, seed=V,
                                      step=2)
                    if k is not None and top_p == 1.0:    # lowest indices first: channel 0 keeps 0..k-1 (EOS is killed, never the arg-max)
                        assert bool((got[0, : min(k, V - 3)] > 0).all()), (V, k)
    tally.bound()


def test_signed_zeros_rank_as_equal(dev):
    """+0.0 and -0.0 have different radix keys; the rank rule treats them as equal, lower index first."""
    gen = torch.Generator().manual_seed(11)
    C, tally = 12, Tally()
    for V in (1027, 2048):
        eos = eos_of(V)
        for k, n_pos in ((5, 2), (45, 40), (100, 95)):
            co = torch.round((-1 - 5 * torch.rand(24, V, generator=gen)) * 1024) / 1024
            for r in range(24):
                idx = torch.randperm(eos, generator=gen)
                co[r, idx[:n_pos]] = 1 + torch.arange(n_pos).float() / 64
                z = idx[n_pos: n_pos + 12].sort().values
                co[r, z] = torch.where(torch.arange(12) % 2 == r % 2, -0.0, 0.0)   # both orders of the signs
            for top_p in (1.0, 0.95):
                pred, got = check(dev, pack(co, torch.zeros_like(co), C), tally, cfg_scale=0.0, T=1.0, top_p=top_p, top_k=k, seed=3,
                                  step=k)
    tally.bound()


def test_fewer_finite_entries_than_k(dev):
    gen = torch.Generator().manual_seed(5)
    V, C, tally = 1027, 12, Tally()
    co = grid_logits(24, V, gen)
    for r in range(24):
        co[r, torch.randperm(V, generator=gen)[:1020]] = float("-inf")
    un = grid_logits(24, V, gen)                              # finite: co - un stays -inf, never nan
    for k in (45, 64, 100):
        for cfg_scale in (0.0, 3.0):
            for top_p in (1.0, 0.5):
                check(dev, pack(co, un, C), tally, cfg_scale=cfg_scale, T=1.0, top_p=top_p, top_k=k, seed=k, step=1)
    tally.bound()


# ----------------------------------------------------------------------------- EOS rules
def test_eos_rules(dev):
    gen = torch.Generator().manual_seed(13)
    V, C, tally = 1027, 12, Tally()
    eos = eos_of(V)
    co = grid_logits(48, V, gen, scale=1.0)
    un = grid_logits(48, V, gen, scale=1.0)
    co[::2, eos] = 12.0                                      # EOS the clear arg-max on every other row (cfg 0: also after x eos_mul)
    co[1::4, eos] = 3.0                                      # a contender on some rows: killed unless it is the arg-max
    lg = pack(co, un, C)
    for k in (45, None):
        for cfg_scale, eos_mul in ((0.0, 0.8), (0.0, 0.25), (3.0, 0.8)):
            # host flag on / off, then min_tokens through the device step: below, equal to, above
            for kw in (dict(enable_eos=True), dict(enable_eos=False), dict(step=9, min_tokens=10), dict(step=10, min_tokens=10),
                       dict(step=11, min_tokens=10), dict(step=4, min_tokens=None)):
                pred, got = check(dev, lg, tally, cfg_scale=cfg_scale, T=1.2, top_p=0.95, top_k=k, eos_mul=eos_mul, seed=21, **kw)
                en = kw.get("enable_eos", True) if "step" not in kw else (kw["min_tokens"] is None or kw["step"] >= kw["min_tokens"])
                g = got.view(-1, C, V)
                assert bool((g[:, :, eos + 1:] == 0).all()) and bool((g[:, 1:, eos:] == 0).all())       # channels >= 1: v >= eos
                if not en:
                    assert bool((g[..., eos:] == 0).all())
                elif cfg_scale == 0.0 and eos_mul == 0.8:
                    assert bool((g[::2, 0, eos] > 0.5).all())                      # 12 * 0.8: still the arg-max, kept
                    assert bool((pred.reshape(-1, C)[::2, 0] == eos).any())
    tally.bound()


# ----------------------------------------------------------------------------- arg-max
def test_argmax_lowest_index_ties(dev):
    gen = torch.Generator().manual_seed(17)
    C = 12
    for V in (2, 7, 1027, 2048):
        co, un = grid_logits(48, V, gen), grid_logits(48, V, gen)
        co[0] = 0.5
        un[0] = 0.5                                          # all equal: index 0
        if V > 7:
            co[1, [3, 5, 9]] = 20.0
            un[1, [3, 5, 9]] = 0.0                               # a three-way tie at the top
            co[2] = -1.0
            co[2, [4, 6]] = torch.tensor([-0.0, 0.0])
            un[2] = co[2]                                     # cfg 3: un = co keeps every value, -0.0 included (co - un = +0)
        for cfg_scale in (0.0, 3.0):
            for en in (True, False):
                gd = OD.cfg_and_mask(SimpleNamespace(codec_eos_value=eos_of(V)), pack(co, un, C).double(), cfg_scale, en, 0.8)
                want = torch.argmax(gd.reshape(-1, V), -1)
                for T, ds in ((1.0, False), (0.0, True), (0.0, False)):
                    pred = sample(dev, pack(co, un, C), cfg_scale=cfg_scale, T=T, top_p=0.95, top_k=45, eos_mul=0.8, seed=1,
                                  enable_eos=en, do_sample=ds, want_probs=False)
                    assert torch.equal(pred.cpu().reshape(-1), want), (V, cfg_scale, en, T, ds)
        if V > 7:
            assert int(want[0]) == 0 and int(want[1]) == 3 and int(want[2]) == 4


def test_step_and_min_tokens_defaults(dev):
    """No step pointer: step 0 in the hash and the host EOS flag -- what an explicit step 0 / min_tokens gives."""
    gen = torch.Generator().manual_seed(19)
    V, C = 1027, 12
    lg = pack(grid_logits(48, V, gen), grid_logits(48, V, gen), C)
    for k in (45, None):
        kw = dict(cfg_scale=3.0, T=1.2, top_p=0.95, top_k=k, seed=4)
        a = sample(dev, lg, **kw, want_probs=False)
        assert torch.equal(a, sample(dev, lg, **kw, step=0, want_probs=False))
        assert torch.equal(sample(dev, lg, **kw, enable_eos=False, want_probs=False),
                           sample(dev, lg, **kw, step=0, min_tokens=1, want_probs=False))
        assert not torch.equal(a, sample(dev, lg, **kw, step=1, want_probs=False))


# ----------------------------------------------------------------------------- (c) statistics of the draws
def chi2_quantile(df, z=4.753424):
    """Wilson-Hilferty: the chi-square quantile at the normal quantile z (4.7534: upper tail 1e-6)"""
    a = 2.0 / (9.0 * df)
    return df * (1.0 - a + z * math.sqrt(a)) ** 3


STATS = [(45, 0.95, 1.2), (5, 1.0, 1.0), (64, 0.5, 2.0), (None, 0.5, 1.0), (100, 1.0, 2.0), (None, 1.0, 0.3)]


@pytest.mark.parametrize("top_k,top_p,T", STATS)
def test_draw_statistics(dev, top_k, top_p, T):
    """One row replicated over B = 64, C = 12: 768 rows x 4 seeds x 66 steps = 202752 draws against the float64 probabilities.
    EOS is off (min_tokens above every step), so every channel has the same distribution. The hash is deterministic: no flakes."""
    gen = torch.Generator().manual_seed(23)
    B, C, V = 64, 12, 1027
    co, un = grid_logits(1, V, gen, scale=0.25), grid_logits(1, V, gen, scale=0.25)      # wide: 5 to 1024 kept entries
    lg = pack(co.expand(B * C, V).contiguous(), un.expand(B * C, V).contiguous(), C)
    p = OD.filter_probs(lg[:2], 3.0, f32(T), f32(top_p), top_k, eos_of(V), f32(0.8), False)[0]
    seeds, steps = (0, 1, 99, 2 ** 40 + 3), range(66)
    lgd = lg.reshape(2 * B, C * V).to(dev)
    from unimoe_audio_amd import ops
    preds = []
    for s in seeds:
        for st in steps:
            stt = torch.tensor([st], dtype=torch.int32, device=dev)
            preds.append(ops.cfg_sample(lgd, B, C, V, cfg_scale=3.0, temperature=T, top_p=top_p, top_k=top_k, eos=eos_of(V),
                                        eos_mul=0.8, seed=s, step=stt, min_tokens=10 ** 6))
    d = torch.stack(preds).cpu().view(len(seeds), len(steps), B * C).numpy()
    N = d.size
    assert N >= 200_000
    assert bool(((d >= 0) & (d < V)).all())
    cnt = np.bincount(d.reshape(-1), minlength=V)
    pn = p.numpy()
    assert cnt[pn == 0].sum() == 0, np.flatnonzero((pn == 0) & (cnt > 0))[:8]
    E = pn * N
    big = E >= 5
    O_b = np.append(cnt[big], cnt[~big & (pn > 0)].sum())
    E_b = np.append(E[big], E[~big & (pn > 0)].sum())
    if E_b[-1] < 5:                                          # fold a small remainder into the smallest kept bin
        O_b, E_b = O_b[:-1].copy(), E_b[:-1].copy()
        j = int(np.argmin(E_b))
        O_b[j] += cnt[~big & (pn > 0)].sum()
        E_b[j] += E[~big & (pn > 0)].sum()
    nz = O_b > 0
    G = 2.0 * float((O_b[nz] * np.log(O_b[nz] / E_b[nz])).sum())
    df = len(E_b) - 1
    if df > 0:
        assert G < chi2_quantile(df), (G, df, chi2_quantile(df))
    # u varies with the row and with the step: neighbouring draws collide about as often as independent ones (sum p^2)
    coll = float((pn ** 2).sum())
    if coll < 0.9:
        across_rows = float((d[:, :, 1:] == d[:, :, :-1]).mean())
        across_steps = float((d[:, 1:, :] == d[:, :-1, :]).mean())
        across_seeds = float((d[1:] == d[:-1]).mean())
        for f in (across_rows, across_steps, across_seeds):
            assert abs(f - coll) < 0.02, (f, coll)


# ----------------------------------------------------------------------------- the engine: seed, step and min_tokens in a step
@pytest.mark.parametrize("top_k", [45, None])
def test_engine_step_samples_with_its_own_step(dev, top_k):
    """A sampled decode (T 1.2, top-p 0.95, top-k 45 / none, min_tokens 4). Before each step the device step counter state[4B] is
    what the sampler will see. The engine's pred equals cfg_sample on the engine's logits at that step and the host draw at that
    step, eagerly and under graph replay, and both runs give the same codes. The channel-0 EOS row of the codec head is scaled up
    so that EOS is often the arg-max: EOS must then be drawn from step min_tokens on, and never before."""
    from test_gpu_engine import build, prompt, small_cfg
    from unimoe_audio_amd import ops
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    cfg = small_cfg()
    m, _ = build(cfg, 3, 0.06)
    C, V, eos = cfg.codec_channels, cfg.codec_vocab_size, cfg.codec_eos_value
    with torch.no_grad():
        m.codec_head.weight[eos] *= 40
    B, T, steps, min_tokens, seed, maxt = 2, 10, 14, 4, 12345, 40
    md = max(cfg.codec_delay_pattern)
    delay = torch.tensor(cfg.codec_delay_pattern)
    ids, am, codec = prompt(cfg, B, T, 4, [2, 0, 0, 1])
    pre, psteps = prepare_audio_prompt(cfg, [None] * B)
    gm = m.to(dev)

    def start():
        e = gm.engine(B, T, maxt)
        e.prefill(gm.calculate_input_embedding(ids.to(dev), codec.to(dev)).reshape(-1, cfg.hidden_size).contiguous(), am.to(dev))
        e.start_decode(pre, psteps, maxt, min_tokens, cfg_scale=3.0, temperature=1.2, top_p=0.95, top_k=top_k, eos_mul=0.8,
                       do_sample=True, seed=seed)
        return e

    # the scaled row's sign: make channel 0's guided EOS logit mostly positive over the steps before min_tokens
    eng, g_eos = start(), 0.0
    for _ in range(min_tokens):
        eng.step(use_graph=False)
        lg = eng.copy_buffer("logits", torch.float32, (B, 2, C, V))[:, :, 0, eos]
        g_eos += float((lg[:, 1] + 3.0 * (lg[:, 1] - lg[:, 0])).sum())
    if g_eos < 0:
        with torch.no_grad():
            gm.codec_head.weight[eos] *= -1                  # a changed weight repacks the engine
    runs, tally = [], Tally()
    for use_graph in (False, True):
        eng = start()
        seen, picks, peak = [], [], []
        for _ in range(steps):
            state = eng.state.cpu()
            st = int(state[4 * B])
            eng.step(use_graph=use_graph)
            lg = eng.copy_buffer("logits", torch.float32, (2 * B, C * V))
            pred = eng.copy_buffer("pred", torch.int64, (B, C)).cpu()
            ref, probs = ops.cfg_sample(lg, B, C, V, cfg_scale=3.0, temperature=1.2, top_p=0.95, top_k=top_k, eos=eos, eos_mul=0.8,
                                        seed=seed, want_probs=True, step=torch.tensor([st], dtype=torch.int32, device=dev),
                                        min_tokens=min_tokens)
            # umoe_delay_step overwrites a sampled code with the forced EOS / PAD once its row counts down (delay pattern)
            cd = state[B: 2 * B].view(B, 1)
            sampled = (cd <= 0) | ((md - cd) < delay.view(1, C))
            assert torch.equal(ref.cpu()[sampled], pred[sampled]), (use_graph, st)
            u = OD.sampler_u(seed, st, np.arange(B * C))
            pr = probs.cpu().numpy()
            for r in torch.nonzero(sampled.view(-1)).flatten().tolist():
                tally.rows += 1
                want, margin = OD.draw(pr[r], u[r], path_of(top_k), margin=True)
                if int(pred.view(-1)[r]) != want:
                    assert path_of(top_k) == "fast" and margin < 1e-6, (use_graph, st, r)
                    tally.near_cdf += 1
            seen.append(st)
            picks.append(torch.where(sampled, pred, -1))
            peak.append(probs.cpu().view(B, C, V).amax(-1))
        runs.append((seen, torch.stack(picks), eng.tokens.cpu().clone(), torch.stack(peak)))
    eng.close()                                              # (one engine: the model caches it per shape)
    tally.bound()
    (s0, p0, t0, pk), (s1, p1, t1, _) = runs
    assert s0 == s1 and s0 == list(range(s0[0], s0[0] + steps)), s0          # the counter advances once per step
    assert s0[0] < min_tokens <= s0[-1] - 2
    assert torch.equal(p0, p1) and torch.equal(t0, t1)
    on = torch.tensor([s >= min_tokens for s in s0])
    ch0 = p0[:, :, 0]
    assert not bool((ch0[~on] == eos).any()) and bool((ch0[on] == eos).any())    # min_tokens reaches the sampler
    assert not bool((p0[:, :, 1:] >= eos).any())                                    # channels >= 1 never sample v >= eos
    # wide distributions (no code above 1/2 at either step): the picks move from step to step. Independent draws would repeat
    # with probability sum p q <= 1/2.
    wide = (pk[1:] < 0.5) & (pk[:-1] < 0.5) & (p0[1:] >= 0) & (p0[:-1] >= 0)
    assert int(wide.sum()) >= 20, int(wide.sum())
    assert float((p0[1:] != p0[:-1])[wide].float().mean()) > 0.4
