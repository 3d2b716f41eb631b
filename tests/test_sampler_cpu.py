"""CPU suite of the host restatement of the device sampler (oracle/decode.py: mix64, sampler_u, filter_probs, scan64, draw), the
yardstick of tests/test_gpu_sampler.py.  No kernel runs."""
import numpy as np
import torch

from conftest import load_golden
from oracle import decode as OD

U_ONE_SEED = 17974134            # sampler_u(U_ONE_SEED, 0, 0) == 1.0: h >> 40 == 2^24 - 1 rounds up in float32


def _mix64_int(z):
    m = (1 << 64) - 1
    z = (z + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def test_mix64_is_splitmix64():
    # the published splitmix64 stream from state 0: outputs 1..3
    assert OD.mix64(0) == 0xE220A8397B1DCDAF
    assert OD.mix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    assert OD.mix64((2 * 0x9E3779B97F4A7C15) & ((1 << 64) - 1)) == 0x06C45D188009454F
    zs = [0, 1, 2 ** 32 + 5, 2 ** 63, 2 ** 64 - 1, 0x0123456789ABCDEF]
    got = OD.mix64(np.array(zs, dtype=np.uint64))
    assert [int(v) for v in got] == [_mix64_int(z) for z in zs]


def test_sampler_u_matches_an_integer_restatement():
    for seed in (0, 7, 2 ** 64 - 1, U_ONE_SEED):
        for step in (0, 1, 5, 2 ** 31 - 1):
            rows = np.arange(40)
            got = OD.sampler_u(seed, step, rows)
            for r in rows:
                h = _mix64_int(seed ^ _mix64_int((step << 32) | int(r)))
                want = np.float32(float(h >> 40) + 0.5) * np.float32(2.0 ** -24)
                assert got[r] == want and got.dtype == np.float32
    u = OD.sampler_u(3, 4, np.arange(100000))
    assert float(u.min()) > 0.0 and float(u.max()) <= 1.0
    assert abs(float(u.mean()) - 0.5) < 0.005
    assert len(np.unique(u)) > 99000                        # row enters the hash
    assert not np.array_equal(u, OD.sampler_u(3, 5, np.arange(100000)))    # step enters the hash
    assert OD.sampler_u(U_ONE_SEED, 0, 0) == np.float32(1.0)
    # above 2^23 the rounding to float32 puts u on a 2^-23 grid
    big = u[u >= 0.5]
    assert np.all(np.round(big.astype(np.float64) * 2 ** 23) == big.astype(np.float64) * 2 ** 23)


def test_scan64_equals_cumsum_when_every_sum_is_exact():
    g = np.random.default_rng(0)
    for n in (1, 2, 7, 33, 63, 64):
        p = g.integers(0, 1 << 10, n).astype(np.float32) * np.float32(2.0 ** -16)   # dyadic: every partial sum is exact
        assert np.array_equal(OD.scan64(p), np.cumsum(p.astype(np.float64)).astype(np.float32))
    # not exact in general: the tree adds in a different order than a sequential loop
    p = np.float32([1.0, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24])
    assert OD.scan64(p)[3] != np.add.accumulate(p, dtype=np.float32)[3]
    assert OD.scan64(p)[3] == np.float32(1.0 + 2.0 ** -23)


def test_draw_rules():
    p = np.float32([0.0, 0.25, 0.0, 0.5, 0.25, 0.0])
    for path in ("slow", "fast"):
        assert OD.draw(p, np.float32(0.1), path) == 1
        assert OD.draw(p, np.float32(0.25), path) == 3        # cum > u is strict
        assert OD.draw(p, np.float32(0.7), path) == 3
        assert OD.draw(p, np.float32(0.75), path) == 4
        assert OD.draw(p, np.float32(1.0), path) == 4         # no cum exceeds u: the last positive entry
        pick, m = OD.draw(p, np.float32(0.7), path, margin=True)
        assert pick == 3 and abs(m - 0.05) < 1e-6
    # fast path: zero-probability candidates hold lanes and change the scan's tree
    q = np.float32([1.0, 2.0 ** -24, 2.0 ** -24, 0.0])
    assert OD.draw(q, np.float32(1.0), "fast", lanes=[0, 1, 2, 3]) == 2
    assert OD.draw(q, np.float32(1.0), "slow") == 2


def _two(lg, C):
    """[rows, V] guided logits -> the kernel's [2B, C, V] layout with zero uncond rows (cfg_scale 0)"""
    B = lg.shape[0] // C
    return torch.stack([torch.zeros_like(lg), lg], 1).reshape(B, C, 2, -1).permute(0, 2, 1, 3).reshape(2 * B, C, -1).contiguous()


def test_filter_probs_vs_reference_goldens():
    g = load_golden("sampler.npz")
    lg = g["logits"]
    cfgo = type("cfg", (), {"codec_eos_value": 1024})
    guided = OD.cfg_and_mask(cfgo, _two(lg, 12).clone(), 0.0, True, 1.0).reshape(24, -1)
    for n in "abcd":
        T, tp, tk = g[f"params_{n}"].tolist()
        tk = None if tk < 0 else int(tk)
        # one channel per row: masks and eos_mul change nothing, so this is the reference's sampler on the raw logits
        p = OD.filter_probs(_two(lg, 1), 0.0, T, tp, tk, 1024, 1.0, True)
        assert p.dtype == torch.float64
        assert torch.equal(p > 0, g[f"probs_{n}"] > 0), n
        assert torch.allclose(p, g[f"probs_{n}"].double(), rtol=1e-5, atol=1e-8), n
        # twelve channels: the EOS masks of channels >= 1 as in the decode step
        p = OD.filter_probs(_two(lg, 12), 0.0, T, tp, tk, 1024, 1.0, True)
        ref = OD.sample_next_token(guided.clone(), T, tp, tk, 1024, return_probs=True)
        assert torch.equal(p > 0, ref > 0), n
        assert torch.allclose(p, ref.double(), rtol=1e-5, atol=1e-8), n


def test_filter_probs_cfg_eos_rules():
    torch.manual_seed(0)
    B, C, V, eos = 2, 3, 9, 6
    lg = torch.randn(2 * B, C, V)
    for cfg_scale, enable_eos, eos_mul in ((0.0, True, 1.0), (3.0, True, 0.8), (3.0, False, 0.8), (2.0, True, 1.5)):
        gd = OD.cfg_and_mask(type("c", (), {"codec_eos_value": eos}), lg.double().clone(), cfg_scale, enable_eos, eos_mul)
        p = OD.filter_probs(lg, cfg_scale, 1.0, 1.0, None, eos, eos_mul, enable_eos).view(B, C, V)
        x = gd / 1.0
        kill = x.argmax(-1) != eos
        x[..., eos] = torch.where(kill, float("-inf"), x[..., eos])
        assert torch.allclose(p, torch.softmax(x, -1), rtol=1e-12, atol=0)
        assert bool((p[:, :, eos + 1:] == 0).all()) and bool((p[:, 1:, eos:] == 0).all())
        if not enable_eos:
            assert bool((p[..., eos:] == 0).all())
    # EOS kept when it is the arg-max after temperature, killed otherwise; eos_mul scales channel 0 only
    x = torch.full((2, 1, V), -2.0)
    x[1, 0, eos], x[1, 0, 0] = 3.0, 2.0
    p = OD.filter_probs(x, 0.0, 0.5, 1.0, None, eos, 1.0, True)
    assert p[0, eos] > 0.5
    p = OD.filter_probs(x, 0.0, 0.5, 1.0, None, eos, 0.5, True)     # 3.0 * 0.5 < 2.0: no longer the arg-max
    assert p[0, eos] == 0 and p[0, 0] > 0.5


def test_filter_probs_tie_rules():
    V = 40
    x = torch.full((V,), -3.0)
    x[[3, 17, 30]] = 2.0
    x[[5, 8, 11, 20, 25, 33]] = 1.0                       # six equal values straddle the 5th position
    p = OD.filter_probs(_two(x[None], 1), 0.0, 1.0, 1.0, 5, V - 1, 1.0, True)[0]
    assert torch.equal(torch.nonzero(p).flatten(), torch.tensor([3, 5, 8, 17, 30]))
    # +0.0 and -0.0 rank as equal: lower index first
    x = torch.full((V,), -3.0)
    x[[2, 9]] = 1.0
    x[[4, 6, 7, 12]] = torch.tensor([-0.0, 0.0, -0.0, 0.0])
    p, cand, gap = OD.filter_probs(_two(x[None], 1), 0.0, 1.0, 1.0, 4, V - 1, 1.0, True, details=True)
    assert torch.equal(torch.nonzero(p[0]).flatten(), torch.tensor([2, 4, 6, 9]))
    assert torch.equal(cand[0], p[0] > 0) and gap.item() == float("inf")
    # top-p order: equal probabilities rank by lower index; mass strictly ahead > top_p removes
    x = torch.log(torch.tensor([0.1, 0.3, 0.1, 0.3, 0.2, 0.0], dtype=torch.float64))     # EOS (index 5) is -inf
    for top_p, kept in ((0.5, [1, 3]), (0.65, [1, 3, 4]), (0.85, [0, 1, 3, 4]), (0.95, [0, 1, 2, 3, 4])):
        p, _, gap = OD.filter_probs(_two(x[None], 1), 0.0, 1.0, top_p, None, 5, 1.0, True, details=True)
        assert torch.equal(torch.nonzero(p[0]).flatten(), torch.tensor(kept)), top_p
        assert abs(gap.item() - min(abs(b - top_p) for b in (0.0, 0.3, 0.6, 0.8, 0.9))) < 1e-12
