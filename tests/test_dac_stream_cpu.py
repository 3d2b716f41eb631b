"""CPU suite: the streaming DAC decoder's plan (pure index arithmetic) and its window schedule, run by a float64 restatement of the
windowed convolutions, against a float64 full decode; the new entry points are declared and exported."""
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

from unimoe_audio_amd import _lib
from unimoe_audio_amd.dac import DAC_16KHZ, DacModel, DacStreamDecoder, stream_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _snake64(x, a):
    a = a.double().reshape(1, -1, 1)
    return x + torch.sin(a * x) ** 2 / (a + 1e-9)


def _full_decode64(model, z):
    """DacModel.decode restated with torch float64 convolutions on the whole sequence"""
    f = model._folded()
    x = z.double()
    outs = [x]
    for ly in stream_plan(model).layers:
        w, b = (t.double() for t in f[ly.mod])
        inp = _snake64(outs[-1], f[ly.snake]) if ly.snake is not None else outs[-1]
        if ly.kind == "conv":
            y = F.conv1d(inp, w, b, stride=ly.stride, padding=ly.pad, dilation=ly.dil)
        else:
            y = F.conv_transpose1d(inp, w, b, stride=ly.stride, padding=ly.pad, output_padding=ly.out_pad)
        if ly.tanh:
            y = torch.tanh(y)
        if ly.res is not None:
            y = y + outs[ly.res]
        outs.append(y)
    return outs[-1][:, 0]


class Stream64(DacStreamDecoder):
    """the decoder's own schedule and buffers; each window computed in float64 from the buffer contents only"""

    def __init__(self, model, batch, z):
        self.z = z.double()
        super().__init__(model, batch, self._src, dtype=torch.float64, device=torch.device("cpu"))
        self.windows = []

    def _src(self, rows, f0, n, out, col):
        assert f0 + n <= self.z.shape[2]
        out[:, :, col:col + n] = self.z[rows, :, f0:f0 + n]

    def _conv(self, ly, x, x_off, L_true, t0, n, resid, r_off, y, y_off):
        self.windows.append((ly.kind, t0, n))
        f = self.model._folded()
        w, b = (t.double() for t in f[ly.mod])
        lo, hi = ly.reads(t0, t0 + n)
        if ly.kind == "convt":
            lo = min(lo, (t0 + ly.pad) // ly.stride)
        seg = torch.zeros(x.shape[0], x.shape[1], hi - lo + 1, dtype=torch.float64)
        a, e = max(lo, 0), min(hi, L_true - 1)
        if a <= e:
            # every position of [0, L) a window reads must be in the buffer the decoder kept
            assert x_off <= a and e < x_off + x.shape[2], (ly.kind, t0, n, a, e, x_off, x.shape[2])
            seg[:, :, a - lo:e - lo + 1] = x[:, :, a - x_off:e - x_off + 1]
        # Snake of a zero-padding position is 0, like the kernels' (padding is applied after the activation)
        inp = _snake64(seg, f[ly.snake]) if ly.snake is not None else seg
        if ly.snake is not None:
            pos = torch.arange(lo, hi + 1)
            inp[:, :, (pos < 0) | (pos >= L_true)] = 0
        if ly.kind == "conv":
            out = F.conv1d(inp, w, b, stride=ly.stride, dilation=ly.dil)[:, :, :n]
        else:
            full = F.conv_transpose1d(inp, w, b, stride=ly.stride)
            u0 = t0 - (lo * ly.stride - ly.pad)
            out = full[:, :, u0:u0 + n]
        assert out.shape[2] == n
        if ly.tanh:
            out = torch.tanh(out)
        if resid is not None:
            out = out + resid[:, :, t0 - r_off:t0 - r_off + n]
        y[:, :, t0 - y_off:t0 - y_off + n] = out


def _tiny(rates=(8, 5, 4, 2), seed=0):
    return DacModel(encoder_dim=4, encoder_rates=(2, 4, 5, 8), latent_dim=6, decoder_dim=16, decoder_rates=rates, n_codebooks=12,
                    codebook_size=16, codebook_dim=4).init_random(seed).double().float()


def test_plan_16khz_geometry():
    p = stream_plan(DacModel(**DAC_16KHZ))
    assert len(p.layers) == 30 and p.hop == 320
    kinds = [(ly.kind, ly.K, ly.stride, ly.dil) for ly in p.layers]
    assert kinds[0] == ("conv", 7, 1, 1) and kinds[-1] == ("conv", 7, 1, 1) and p.layers[-1].tanh
    assert [k for k in kinds if k[0] == "convt"] == [("convt", 16, 8, 1), ("convt", 10, 5, 1), ("convt", 8, 4, 1), ("convt", 4, 2, 1)]
    # left context / lookahead in input positions: K=7 convs pad 3 * dilation on both sides, K=1 none, the upsamplers one frame
    assert [(ly.left, ly.look) for ly in p.layers[:9]] == [(3, 3), (1, 1), (3, 3), (0, 0), (9, 9), (0, 0), (27, 27), (0, 0), (1, 1)]
    assert [ly.res for ly in p.layers[:8]] == [None, None, None, 2, None, 4, None, 6]
    assert p.layers[0].cin == 1024 and p.layers[0].cout == 1536 and p.layers[-1].cout == 1
    # 1.0.0 passes no output_padding: rate 5 yields 5 L - 1, so T frames give 320 T - 8 samples
    for T in (1, 7, 25, 500):
        assert p.out_len(T) == 320 * T - 8
    assert p.lookahead_frames == 10
    assert p.ready(10) == 59 and p.ready(11) == 379 and p.ready(9) == 0
    for A in range(11, 200):
        assert p.ready(A) >= (A - p.lookahead_frames) * p.hop


def test_plan_small_geometry():
    p = stream_plan(_tiny(rates=(3, 2)))
    assert p.hop == 6 and len(p.layers) == 1 + 2 * 7 + 1
    t1, t2 = p.layers[1], p.layers[8]
    assert (t1.K, t1.stride, t1.pad, t2.K, t2.stride, t2.pad) == (6, 3, 2, 4, 2, 1)
    assert (t1.left, t1.look) == (1, 1) and (t2.left, t2.look) == (1, 1)
    # (10 - 1) * 3 - 4 + 6 = 29 at the first upsampler, (29 - 1) * 2 - 2 + 4 = 58 at the second
    assert p.out_len(10) == 58
    # 1 + 39 + 3 positions at the last upsampler's output -> 22 inputs, + 39 -> 61 at the first one's output -> 21 frames, + 3
    assert p.lookahead_frames == 24
    # ready() is a safe dependency bound: changing frames [A, T) changes no sample before ready(A) (a later one may stay put only
    # where the final tanh saturates)
    model = _tiny(rates=(3, 2))
    torch.manual_seed(1)
    T = 40
    z = torch.randn(1, model.latent_dim, T, dtype=torch.float64)
    ref = _full_decode64(model, z)
    for A in (24, 25, 30):
        z2 = z.clone()
        z2[:, :, A:] += 1.0
        diff = (_full_decode64(model, z2) != ref)[0].nonzero()
        assert p.ready(A) <= int(diff[0]) <= p.ready(A) + p.hop, (A, int(diff[0]), p.ready(A))


@pytest.mark.parametrize("rates", [(8, 5, 4, 2), (3, 2)])
def test_stream_schedule_matches_full_decode_float64(rates):
    torch.manual_seed(0)
    model = _tiny(rates)
    B, T = 3, 61
    z = torch.randn(B, model.latent_dim, T, dtype=torch.float64)
    ref = _full_decode64(model, z)
    plan = stream_plan(model)
    assert ref.shape[1] == plan.out_len(T)
    if rates == (8, 5, 4, 2):
        assert ref.shape[1] == 320 * T - 8
    dec = Stream64(model, B, z)
    got = [[] for _ in range(B)]
    # rows part: row 2 stops early at 40 frames, rows 0 / 1 push different schedules of 1, 7 and 25 frames
    sched = [[1, 1, 1], [7, 7, 7], [25, 25, 25], [1, 7, 7], [25, 1, 0], [2, 20, 0]]
    pushed = [0] * B
    for n in sched:
        for r, v in dec.push(n).items():
            got[r].append(v)
        pushed = [p + v for p, v in zip(pushed, n)]
    assert pushed == [T, T, 40]
    lens = [T, T, 40]
    refs = [ref[0], ref[1], _full_decode64(model, z[2:3, :, :40])[0]]
    for r, v in dec.flush([2]).items():
        got[r].append(v)
    for r, v in dec.flush([0, 1], min_duration=None).items():
        got[r].append(v)
    for r in range(B):
        g = torch.cat(got[r])
        assert g.shape[0] == plan.out_len(lens[r]) == refs[r].shape[0]
        assert torch.allclose(g, refs[r], rtol=0, atol=1e-12), (r, (g - refs[r]).abs().max())
    # a window never recomputes an output: per layer the windows tile [0, L)
    assert all(n > 0 for _, _, n in dec.windows)


def test_flush_appends_min_duration_pad_like_dac_decode():
    model = _tiny()
    z = torch.randn(1, model.latent_dim, 12, dtype=torch.float64)
    dec = Stream64(model, 1, z)
    a = dec.push(12).get(0, torch.zeros(0, dtype=torch.float64))
    b = dec.flush(0, min_duration=1)[0]
    n = stream_plan(model).out_len(12)
    sr = model.sample_rate
    assert a.shape[0] + b.shape[0] == n + int((1 - n / sr) * sr)
    assert torch.count_nonzero(b[b.shape[0] - int((1 - n / sr) * sr):]) == 0
    with pytest.raises(ValueError):
        dec.push(1)


def test_stream_entry_points_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "umoe.h")).read()
    for name in ("umoe_dac_conv1d_win", "umoe_dac_conv_transpose1d_win", "umoe_rvq_from_delayed"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.EXPORTS
    assert len(_lib.STRUCT_MIRRORS) == 16
    so = _lib.build()
    import ctypes
    L = ctypes.CDLL(so)
    for name in ("umoe_dac_conv1d_win", "umoe_dac_conv_transpose1d_win", "umoe_rvq_from_delayed"):
        assert hasattr(L, name)
