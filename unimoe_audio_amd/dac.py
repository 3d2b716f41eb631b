"""DAC (descript-audio-codec 1.0.0, 16 kHz / 50 Hz variant) on the HIP path: waveform <-> RVQ codes.

Mirrors what the reference needs from the third-party package (reference utils/UniMoE_Audio_utils.py:56-134):
    Dac()                      weight discovery like the reference (DAC_WEIGHTS, <pkg>/dac_model/weights_16khz.pth, ...; no download: offline)
    Dac.encode(audio_path)     mono mix (:97-98), resample to 16 kHz (:101-110), preprocess, encoder + RVQ -> codes [T][12] as lists (:112-119)
    Dac.decode(codes, path, min_duration)   quantizer.from_codes -> decoder -> zero-pad to min_duration -> 16-bit PCM wav (:121-134)
`DacModel` keeps the package's module tree and parameter names (encoder.block.N..., quantizer.quantizers.N.{in_proj,out_proj,codebook},
decoder.model.N..., weight-norm pairs weight_g / weight_v, Snake alpha), so the published `weights_16khz.pth` loads by name; every
dimension comes from the checkpoint's metadata or tensor shapes.  The arithmetic runs in libumoe_hip.so (umoe_dac_conv1d,
umoe_dac_conv_transpose1d with the preceding Snake fused, umoe_rvq_nearest, umoe_rvq_from_codes).  PARITY UNPINNED: `dac`,
`audiotools` and `torchaudio` are absent offline, so the layers, the resampler (torchaudio's windowed-sinc formula) and the PCM
conversion are restated from their published definitions; tests compare the kernels with plain fp32 torch restatements.
Two forms of the convolutions (DacModel.conv_form, Dac(conv_form=...)): "direct", the fp32 VALU kernels and the default, and "mfma", the
same layers as implicit GEMMs on the f32-input MFMA (umoe_dac_*_mfma on a k-major weight copy; exact fp32 in another summation order,
DESIGN 4q).  uses_mfma() decides per layer shape, for the full, windowed and per-row calls alike.
"""
from __future__ import annotations

import ctypes as C
import functools
import math
import os
import wave
from typing import List, NamedTuple, Optional, Sequence

import torch
import torch.nn as nn

from . import _lib as L
from . import ops


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev_f32(t: Optional[torch.Tensor]):
    if t is None:
        return None
    if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
        raise L.UmoeError("DAC ops need contiguous float32 device tensors (there is no CPU path in the product)")
    return C.c_void_p(t.data_ptr())


CONV_FORMS = ("direct", "mfma")


def _check_form(form) -> str:
    if form not in CONV_FORMS:
        raise ValueError(f"conv form {form!r}: expected one of {CONV_FORMS}")
    return form


def uses_mfma(cin: int, cout: int, K: int, stride: int) -> bool:
    """THE routing rule of conv_form="mfma": whether a layer of this shape runs on the f32 MFMA kernels (umoe_dac_*_mfma) or stays on the
    direct ones.  Static in the layer's shape, and consulted by every call site (full, windowed, per-row), so all forms of one layer
    agree and a model in "mfma" mode stays bit-identical between DacModel.decode and the streaming decoders."""
    return True


def kmajor(w: torch.Tensor, transposed: bool) -> torch.Tensor:
    """the MFMA kernels' weight operand wt [Cin][K][Cout] from w [Cout][Cin][K] (conv1d) or [Cin][Cout][K] (transposed)"""
    return (w.permute(0, 2, 1) if transposed else w.permute(1, 2, 0)).contiguous()


def conv1d(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], *, stride=1, dilation=1, padding=0,
           snake_alpha: Optional[torch.Tensor] = None, resid: Optional[torch.Tensor] = None, tanh: bool = False, form: str = "direct",
           wt: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = [tanh](conv1d(snake?(x)) + bias) [+ resid]; x [B, Cin, L], w [Cout, Cin, K] (weight norm already folded).
    form="mfma": the f32 MFMA kernel on wt = kmajor(w) (made here when the caller has none)."""
    mfma = _check_form(form) == "mfma"
    B, Cin, Lx = x.shape
    Cout, Cin2, K = w.shape
    assert Cin2 == Cin
    Lout = (Lx + 2 * padding - dilation * (K - 1) - 1) // stride + 1
    y = torch.empty((B, Cout, max(Lout, 0)), dtype=torch.float32, device=x.device)      # (an empty output: the library refuses it)
    if resid is not None:
        assert tuple(resid.shape) == tuple(y.shape)
    lo = C.c_int()
    name = "umoe_dac_conv1d_mfma" if mfma else "umoe_dac_conv1d"
    if mfma and wt is None:
        wt = kmajor(w, False)
    _lib_call(name, _dev_f32(x), _dev_f32(wt if mfma else w), _dev_f32(bias), _dev_f32(snake_alpha), _dev_f32(resid), B, Cin, Lx, Cout, K,
              stride, dilation, padding, int(tanh), _dev_f32(y), C.byref(lo), _stream())
    assert lo.value == Lout
    return y


def conv_transpose1d(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], *, stride, padding, output_padding=0,
                     snake_alpha: Optional[torch.Tensor] = None, form: str = "direct", wt: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = conv_transpose1d(snake?(x)) + bias; x [B, Cin, L], w [Cin, Cout, K].  form="mfma": as conv1d, wt = kmajor(w, True)."""
    mfma = _check_form(form) == "mfma"
    B, Cin, Lx = x.shape
    Cin2, Cout, K = w.shape
    assert Cin2 == Cin
    Lout = (Lx - 1) * stride - 2 * padding + K + output_padding
    y = torch.empty((B, Cout, Lout), dtype=torch.float32, device=x.device)
    lo = C.c_int()
    name = "umoe_dac_conv_transpose1d_mfma" if mfma else "umoe_dac_conv_transpose1d"
    if mfma and wt is None:
        wt = kmajor(w, True)
    _lib_call(name, _dev_f32(x), _dev_f32(wt if mfma else w), _dev_f32(bias), _dev_f32(snake_alpha), B, Cin, Lx, Cout, K, stride,
              padding, output_padding, _dev_f32(y), C.byref(lo), _stream())
    assert lo.value == Lout
    return y


# ----------------------------------------------------------------------------------------------- parameter containers
class Snake1d(nn.Module):
    def __init__(self, channels: int):
        super().__init__()
        self.alpha = nn.Parameter(torch.ones(1, channels, 1))


class _WN(nn.Module):
    """A weight-normalised conv as the package stores it (torch.nn.utils.weight_norm: weight_g, weight_v, bias)."""

    def __init__(self, shape, g_shape, bias_n, **geom):
        super().__init__()
        self.weight_g = nn.Parameter(torch.ones(g_shape))
        self.weight_v = nn.Parameter(torch.zeros(shape))
        self.bias = nn.Parameter(torch.zeros(bias_n))
        self.geom = geom

    def shape4(self):
        """(cin, cout, K, stride): what dac.uses_mfma decides on"""
        a, b, K = (int(v) for v in self.weight_v.shape)
        cin, cout = (a, b) if self.geom["transposed"] else (b, a)
        return cin, cout, K, int(self.geom["stride"])

    def folded(self) -> torch.Tensor:
        v = self.weight_v.data.float()
        n = v.reshape(v.shape[0], -1).norm(dim=1).reshape(-1, 1, 1)
        return (self.weight_g.data.float() * v / n).contiguous()


def WNConv1d(cin, cout, kernel_size, stride=1, dilation=1, padding=0):
    return _WN((cout, cin, kernel_size), (cout, 1, 1), cout, stride=stride, dilation=dilation, padding=padding, transposed=False)


def WNConvTranspose1d(cin, cout, kernel_size, stride=1, padding=0, output_padding=0):
    return _WN((cin, cout, kernel_size), (cin, 1, 1), cout, stride=stride, padding=padding, output_padding=output_padding, transposed=True)


class _Seq(nn.Module):
    """nn.Sequential-like numbering under the attribute name the package uses (`block` / `model`)."""

    def __init__(self, name: str, mods: Sequence[nn.Module]):
        super().__init__()
        setattr(self, name, nn.ModuleList(mods))
        self._name = name

    def items(self):
        return list(getattr(self, self._name))


def ResidualUnit(dim, dilation):
    pad = ((7 - 1) * dilation) // 2
    return _Seq("block", [Snake1d(dim), WNConv1d(dim, dim, 7, dilation=dilation, padding=pad), Snake1d(dim), WNConv1d(dim, dim, 1)])


def EncoderBlock(dim, stride):
    return _Seq("block", [ResidualUnit(dim // 2, 1), ResidualUnit(dim // 2, 3), ResidualUnit(dim // 2, 9), Snake1d(dim // 2),
                          WNConv1d(dim // 2, dim, 2 * stride, stride=stride, padding=math.ceil(stride / 2))])


def DecoderBlock(cin, cout, stride, output_padding=0):
    return _Seq("block", [Snake1d(cin), WNConvTranspose1d(cin, cout, 2 * stride, stride=stride, padding=math.ceil(stride / 2),
                                                           output_padding=output_padding),
                          ResidualUnit(cout, 1), ResidualUnit(cout, 3), ResidualUnit(cout, 9)])


class VectorQuantize(nn.Module):
    def __init__(self, input_dim, codebook_size, codebook_dim):
        super().__init__()
        self.in_proj = WNConv1d(input_dim, codebook_dim, 1)
        self.out_proj = WNConv1d(codebook_dim, input_dim, 1)
        self.codebook = nn.Embedding(codebook_size, codebook_dim)


class ResidualVectorQuantize(nn.Module):
    def __init__(self, input_dim, n_codebooks, codebook_size, codebook_dim):
        super().__init__()
        self.quantizers = nn.ModuleList([VectorQuantize(input_dim, codebook_size, codebook_dim) for _ in range(n_codebooks)])


DAC_16KHZ = dict(encoder_dim=64, encoder_rates=[2, 4, 5, 8], decoder_dim=1536, decoder_rates=[8, 5, 4, 2], n_codebooks=12, codebook_size=1024,
                 codebook_dim=8, sample_rate=16000)


class DacModel(nn.Module):
    """dac.DAC's module tree; encode / decode on the HIP kernels."""

    def __init__(self, encoder_dim=64, encoder_rates=(2, 4, 5, 8), latent_dim=None, decoder_dim=1536, decoder_rates=(8, 5, 4, 2), n_codebooks=12,
                 codebook_size=1024, codebook_dim=8, sample_rate=16000, decoder_output_padding=False, **unused):
        super().__init__()
        self.sample_rate, self.hop_length = int(sample_rate), int(math.prod(encoder_rates))
        self.n_codebooks, self.codebook_size, self.codebook_dim = int(n_codebooks), int(codebook_size), int(codebook_dim)
        d = encoder_dim
        enc = [WNConv1d(1, d, 7, padding=3)]
        for s in encoder_rates:
            d *= 2
            enc.append(EncoderBlock(d, s))
        self.latent_dim = int(latent_dim) if latent_dim else d
        enc += [Snake1d(d), WNConv1d(d, self.latent_dim, 3, padding=1)]
        self.encoder = _Seq("block", enc)
        self.quantizer = ResidualVectorQuantize(self.latent_dim, n_codebooks, codebook_size, codebook_dim)
        dec = [WNConv1d(self.latent_dim, decoder_dim, 7, padding=3)]
        cout = decoder_dim
        for i, s in enumerate(decoder_rates):
            cin, cout = decoder_dim // 2 ** i, decoder_dim // 2 ** (i + 1)
            # (1.0.0 passes no output_padding: an odd rate makes the waveform a few samples shorter than frames * hop)
            dec.append(DecoderBlock(cin, cout, s, output_padding=(s % 2 if decoder_output_padding else 0)))
        dec += [Snake1d(cout), WNConv1d(cout, 1, 7, padding=3), nn.Tanh()]
        self.decoder = _Seq("model", dec)
        self._fold = None
        self.conv_form = "direct"

    def set_conv_form(self, form: str) -> "DacModel":
        """"direct": the fp32 VALU kernels (the default); "mfma": every layer that dac.uses_mfma names runs on the f32 MFMA kernels, in
        encode, decode and the streaming decoders alike (one more fp32 copy of those layers' weights, k-major, made at the next use)."""
        self.conv_form = _check_form(form)
        return self

    # ---- weights ------------------------------------------------------------------------------------------------------
    @classmethod
    def load(cls, path: str, device="cuda") -> "DacModel":
        """The package's checkpoint format (audiotools BaseModel.save): {"state_dict", "metadata": {"kwargs": ...}}; a bare
        state dict works too (16 kHz geometry unless the shapes say otherwise)."""
        obj = torch.load(path, map_location="cpu", weights_only=False)
        sd = obj.get("state_dict", obj) if isinstance(obj, dict) else obj
        kw = dict(DAC_16KHZ)
        # geometry from the tensors themselves (every DAC dimension is a load-time parameter), then the metadata where present
        if "encoder.block.0.weight_v" in sd and "decoder.model.0.weight_v" in sd:
            kw["encoder_dim"] = int(sd["encoder.block.0.weight_v"].shape[0])
            kw["decoder_dim"], kw["latent_dim"] = int(sd["decoder.model.0.weight_v"].shape[0]), int(sd["decoder.model.0.weight_v"].shape[1])
            er, dr, i = [], [], 1
            while f"encoder.block.{i}.block.4.weight_v" in sd:
                er.append(int(sd[f"encoder.block.{i}.block.4.weight_v"].shape[2]) // 2)
                i += 1
            i = 1
            while f"decoder.model.{i}.block.1.weight_v" in sd:
                dr.append(int(sd[f"decoder.model.{i}.block.1.weight_v"].shape[2]) // 2)
                i += 1
            if er and dr:
                kw["encoder_rates"], kw["decoder_rates"] = er, dr
        meta = obj.get("metadata", {}) if isinstance(obj, dict) else {}
        kw.update({k: v for k, v in meta.get("kwargs", {}).items() if k in kw or k == "latent_dim"})
        nq = 1 + max((int(k.split(".")[2]) for k in sd if k.startswith("quantizer.quantizers.")), default=kw["n_codebooks"] - 1)
        kw["n_codebooks"] = nq
        cbw = sd.get("quantizer.quantizers.0.codebook.weight")
        if cbw is not None:
            kw["codebook_size"], kw["codebook_dim"] = int(cbw.shape[0]), int(cbw.shape[1])
        m = cls(**kw)
        missing, unexpected = m.load_state_dict(sd, strict=False)
        if missing:
            raise KeyError(f"DAC checkpoint {path!r} lacks {len(missing)} tensors, e.g. {missing[:4]}")
        return m.to(device).float().eval()

    @torch.no_grad()
    def init_random(self, seed: int = 0) -> "DacModel":
        g = torch.Generator().manual_seed(seed)
        for n, p in self.named_parameters():
            if n.endswith("alpha"):
                p.copy_(0.5 + torch.rand(p.shape, generator=g))
            elif n.endswith("weight_g"):
                p.copy_(0.5 + torch.rand(p.shape, generator=g))
            elif n.endswith("bias"):
                p.copy_(0.02 * torch.randn(p.shape, generator=g))
            elif n.endswith("codebook.weight"):
                p.copy_(torch.randn(p.shape, generator=g))
            else:
                fan = p[0].numel() if p.dim() > 1 else 1
                p.copy_(torch.randn(p.shape, generator=g) / fan ** 0.5)
        self._fold = None
        return self

    def _folded(self) -> dict:
        """weight norm folded once (g * v / |v|), keyed by module; the RVQ projections stacked for the RVQ kernels."""
        key = (self.conv_form,) + tuple((p.data_ptr(), p._version) for p in self.parameters())
        if self._fold is not None and self._fold["key"] == key:
            return self._fold
        f = {"key": key, "wt": {}}
        for m in self.modules():
            if isinstance(m, _WN):
                f[m] = (m.folded(), m.bias.data.float().contiguous())
            elif isinstance(m, Snake1d):
                f[m] = m.alpha.data.float().reshape(-1).contiguous()
        if self.conv_form == "mfma":          # the MFMA kernels' weight operand, for the conv stacks' layers that dac.uses_mfma names
            for part in (self.encoder, self.decoder):
                for m in part.modules():
                    if isinstance(m, _WN) and uses_mfma(*m.shape4()):
                        f["wt"][m] = kmajor(f[m][0], m.geom["transposed"])
        q = self.quantizer.quantizers
        f["cb"] = torch.stack([v.codebook.weight.data.float() for v in q], 0).contiguous()                      # [NQ, CB, cd]
        f["in_w"] = torch.stack([f[v.in_proj][0][:, :, 0] for v in q], 0).contiguous()                           # [NQ, cd, Dl]
        f["in_b"] = torch.stack([f[v.in_proj][1] for v in q], 0).contiguous()
        f["out_w"] = torch.stack([f[v.out_proj][0][:, :, 0] for v in q], 0).contiguous()                         # [NQ, Dl, cd]
        f["out_b"] = torch.stack([f[v.out_proj][1] for v in q], 0).contiguous()
        self._fold = f
        return f

    def _route(self, m: "_WN", f: dict):
        """(form, weight operand) of conv m under this model's conv_form: the one place every call site asks"""
        wt = f["wt"].get(m)
        return ("mfma", wt) if wt is not None else ("direct", f[m][0])

    # ---- graph walk: Snake is always followed by a conv, into whose input load it is fused -------------------------------
    def _conv(self, m: "_WN", x, f, **kw):
        form, wsel = self._route(m, f)
        g = m.geom
        if g["transposed"]:
            return conv_transpose1d(x, f[m][0], f[m][1], stride=g["stride"], padding=g["padding"], output_padding=g["output_padding"], form=form,
                                    wt=wsel, **kw)
        return conv1d(x, f[m][0], f[m][1], stride=g["stride"], dilation=g["dilation"], padding=g["padding"], form=form, wt=wsel, **kw)

    def _run(self, mods, x, f):
        alpha = None
        for m in mods:
            if isinstance(m, Snake1d):
                alpha = f[m]
            elif isinstance(m, _WN):
                x = self._conv(m, x, f, snake_alpha=alpha)
                alpha = None
            elif isinstance(m, _Seq) and len(m.items()) == 4 and isinstance(m.items()[0], Snake1d):      # ResidualUnit: x + block(x)
                a0, c0, a1, c1 = m.items()
                t = self._conv(c0, x, f, snake_alpha=f[a0])
                x = self._conv(c1, t, f, snake_alpha=f[a1], resid=x)
            elif isinstance(m, _Seq):
                x = self._run(m.items(), x, f)
            elif isinstance(m, nn.Tanh):
                raise AssertionError("tanh is fused into the last conv")
        return x

    def preprocess(self, audio: torch.Tensor, sample_rate: Optional[int] = None) -> torch.Tensor:
        """right-pad to a multiple of the hop length (dac.DAC.preprocess)"""
        assert sample_rate is None or sample_rate == self.sample_rate
        n = audio.shape[-1]
        pad = math.ceil(n / self.hop_length) * self.hop_length - n
        return torch.nn.functional.pad(audio, (0, pad))

    @torch.no_grad()
    def encode(self, x: torch.Tensor, n_quantizers: Optional[int] = None):
        """x [B, 1, L] float32 -> (z [B, Dl, T], codes [B, NQ, T] int64)"""
        f = self._folded()
        z = self._run(self.encoder.items(), x.float().contiguous(), f)
        nq = self.n_codebooks if n_quantizers is None else int(n_quantizers)
        codes = torch.stack([ops.rvq_nearest(z[b].contiguous(), f["cb"][:nq].contiguous(), f["in_w"][:nq].contiguous(), f["in_b"][:nq].contiguous(),
                                             f["out_w"][:nq].contiguous(), f["out_b"][:nq].contiguous()) for b in range(z.shape[0])], 0)
        return z, codes.long()

    @torch.no_grad()
    def from_codes(self, codes: torch.Tensor) -> torch.Tensor:
        """codes [B, NQ, T] -> z_q [B, Dl, T] (ResidualVectorQuantize.from_codes: sum of out_proj(codebook[code]))"""
        f = self._folded()
        nq = codes.shape[1]
        return torch.stack([ops.rvq_from_codes(codes[b].contiguous(), f["cb"][:nq].contiguous(), f["out_w"][:nq].contiguous(), f["out_b"][:nq].contiguous())
                            for b in range(codes.shape[0])], 0)

    @torch.no_grad()
    def decode(self, z: torch.Tensor) -> torch.Tensor:
        """z [B, Dl, T] -> audio [B, 1, ~T * hop]"""
        f = self._folded()
        mods = self.decoder.items()
        x = self._run(mods[:-3], z.float().contiguous(), f)
        snake, last = mods[-3], mods[-2]
        return self._conv(last, x, f, snake_alpha=f[snake], tanh=True)


# ----------------------------------------------------------------------------------------------- resampler / wav io
def resample_filter(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """The filter bank of resample(): (kern [n, 2 * width + o] float32 on the CPU, o, n, width) with o / n = orig / new over their gcd."""
    g = math.gcd(int(orig_freq), int(new_freq))
    o, n = int(orig_freq) // g, int(new_freq) // g
    base = min(o, n) * rolloff
    width = math.ceil(lowpass_filter_width * o / base)
    idx = torch.arange(-width, width + o, dtype=torch.float64)[None, None] / o
    t = torch.arange(0, -n, -1, dtype=torch.float64)[:, None, None] / n + idx
    t = (t * base).clamp(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    kern = torch.where(t == 0, torch.ones_like(t), t.sin() / t) * window * (base / o)                 # [n, 1, 2*width + o]
    return kern[:, 0].float().contiguous(), o, n, width


def resample(wave_BxL: torch.Tensor, orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99) -> torch.Tensor:
    """torchaudio.transforms.Resample's default algorithm (windowed sinc, Hann window), restated: a bank of `new/gcd` filters applied
    with stride `orig/gcd` (umoe_dac_resample)."""
    if orig_freq == new_freq:
        return wave_BxL
    kern, o, n, width = resample_filter(orig_freq, new_freq, lowpass_filter_width, rolloff)
    B, Lx = wave_BxL.shape
    Lout = math.ceil(n * Lx / o)
    x = wave_BxL.float().contiguous()
    kd = kern.to(x.device).contiguous()                                                                   # [n, 2*width + o]
    y = torch.empty((B, Lout), dtype=torch.float32, device=x.device)
    L.check(L.lib().umoe_dac_resample(_dev_f32(x), _dev_f32(kd), B, Lx, o, n, width, Lout, _dev_f32(y), _stream()), "umoe_dac_resample")
    return y


def read_wav(path: str):
    """PCM wav -> (float32 [channels, samples] in [-1, 1), sample_rate); stdlib only (audiotools / soundfile are absent offline)."""
    import numpy as np
    with wave.open(path, "rb") as wf:
        ch, sw, sr, n = wf.getnchannels(), wf.getsampwidth(), wf.getframerate(), wf.getnframes()
        raw = wf.readframes(n)
    if sw == 2:
        a = np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0
    elif sw == 4:
        a = np.frombuffer(raw, dtype="<i4").astype(np.float32) / 2147483648.0
    elif sw == 1:
        a = (np.frombuffer(raw, dtype=np.uint8).astype(np.float32) - 128.0) / 128.0
    else:
        raise ValueError(f"unsupported sample width {sw} in {path}")
    return torch.from_numpy(a.reshape(-1, ch).T.copy()), sr


def write_wav_pcm16(path: str, audio_CxL: torch.Tensor, sample_rate: int):
    """torchaudio.save(..., encoding="PCM_S", bits_per_sample=16) (reference utils.py:134): scale, round, clamp, little endian."""
    a = (audio_CxL.detach().cpu().float() * 32768.0).round().clamp(-32768, 32767).to(torch.int16)
    with wave.open(path, "wb") as wf:
        wf.setnchannels(a.shape[0])
        wf.setsampwidth(2)
        wf.setframerate(sample_rate)
        wf.writeframes(a.T.contiguous().numpy().tobytes())


class Dac:
    """reference utils/UniMoE_Audio_utils.py:56-134 (same methods and error behaviour; no download offline)."""

    def __init__(self, weights_path: Optional[str] = None, device="cuda", model: Optional[DacModel] = None, conv_form: Optional[str] = None):
        """conv_form "direct" / "mfma": the form of the codec's convolutions (DacModel.set_conv_form).  None, the default: "direct" for
        a model loaded here; a `model` handed in keeps the form it has."""
        self.resampler = dict()
        if conv_form is not None:
            _check_form(conv_form)
        if model is not None:
            self.model = model if conv_form is None else model.set_conv_form(conv_form)
            return
        base_dir = os.path.dirname(__file__)
        candidates = [p for p in (weights_path, os.environ.get("DAC_WEIGHTS")) if p]
        candidates.extend([os.path.join(base_dir, "dac_model", "weights_16khz.pth"), os.path.join(base_dir, "weights_16khz.pth"),
                           os.path.join(os.getcwd(), "utils", "dac_model", "weights_16khz.pth"),
                           os.path.join(os.getcwd(), "dac_model", "weights_16khz.pth")])
        final = next((p for p in candidates if p and os.path.isfile(p)), None)
        if not final:
            raise FileNotFoundError("DAC weights not found. Please place weights_16khz.pth in one of the following locations or set "
                                    "DAC_WEIGHTS to an absolute path:" + "\n - " + "\n - ".join(candidates))
        self.model = DacModel.load(final, device).set_conv_form(conv_form or "direct")

    @property
    def conv_form(self) -> str:
        return self.model.conv_form

    @property
    def device(self):
        return next(self.model.parameters()).device

    def encode(self, audio_path) -> List[List[int]]:
        audio, sr = read_wav(audio_path)
        if audio.shape[0] == 2:
            audio = 0.5 * (audio[:1] + audio[1:])                                 # utils.py:97-98
        audio = audio.to(self.device)
        if sr != self.model.sample_rate:
            audio = resample(audio, sr, self.model.sample_rate)                   # utils.py:101-110
        x = self.model.preprocess(audio[None], self.model.sample_rate)
        _, codes = self.model.encode(x)
        codes = codes[0].transpose(0, 1)
        assert codes.shape[1] == self.model.n_codebooks and codes.dim() == 2      # utils.py:116
        return codes.tolist()

    def decode(self, codes: torch.Tensor, save_path: str, min_duration=None):
        assert codes.shape[0] == 1 and codes.shape[1] == self.model.n_codebooks   # utils.py:122
        z = self.model.from_codes(codes.to(self.device))
        audio_out = self.model.decode(z)[0].detach().cpu()
        sr = self.model.sample_rate
        pad = min_duration_pad(audio_out.size(1), sr, min_duration)
        if pad:
            audio_out = torch.cat((audio_out, torch.zeros((audio_out.size(0), pad), dtype=audio_out.dtype)), dim=1)
        write_wav_pcm16(save_path, audio_out, sr)


def min_duration_pad(n_samples: int, sample_rate: int, min_duration) -> int:
    """zero samples the reference appends so that n_samples last min_duration seconds (utils.py:127-132): Dac.decode's and both flushes'"""
    duration = n_samples / sample_rate
    if min_duration is None or duration >= min_duration:
        return 0
    return int((min_duration - duration) * sample_rate)


# ----------------------------------------------------------------------------------------------- streaming decode
# The decoder is a chain of convolutions with bounded receptive fields, so a prefix of the waveform is fixed by a prefix of the
# latent frames.  stream_plan() walks the graph DacModel._run walks and derives, per conv, which input positions an output reads.
# ONE schedule, _Timeline, turns a sequence's pushes into windows: per layer input one buffer, trimmed to the left context the next
# window needs, and per layer every output that the frames pushed so far fully determine.  TWO executors run its windows, each over
# storage of its own: DacStreamDecoder (rows that share a timeline, a tensor per buffer, every window run as it is produced) and
# DacRowStreamDecoder (a timeline per row over slabs, all windows of a read recorded and run at once; further down).  Each output runs
# through the windowed kernels (umoe_dac_conv1d_win / umoe_dac_conv_transpose1d_win, or their _rows twins), whose arithmetic per
# output is that of the full-sequence kernels, so the streamed waveform is bit-identical to DacModel.decode for any schedule of pushes.

_OPEN = 1 << 26          # true length of a sequence that is still growing: no window reads past what was pushed, so any bound works


class StreamLayer:
    """One conv of the decoder: reads buffer `src` (= its own index), writes buffer src + 1; `res` is the buffer added as the residual.
    `left` / `look`: input positions before / after the one aligned with an output (t * stride for a conv, t // stride for a
    transposed conv) that the output reads."""

    def __init__(self, kind, mod, snake, cin, cout, K, stride, dil, pad, out_pad, tanh, res):
        self.kind, self.mod, self.snake = kind, mod, snake
        self.cin, self.cout, self.K, self.stride, self.dil, self.pad, self.out_pad = cin, cout, K, stride, dil, pad, out_pad
        self.tanh, self.res = tanh, res
        s = stride
        if kind == "conv":
            self.left, self.look = pad, (K - 1) * dil - pad
        else:
            self.left = max(t // s - self.reads(t, t + 1)[0] for t in range(s))
            self.look = max(self.reads(t, t + 1)[1] - t // s for t in range(s))

    def out_len(self, L: int) -> int:
        if self.kind == "conv":
            return (L + 2 * self.pad - self.dil * (self.K - 1) - 1) // self.stride + 1
        return (L - 1) * self.stride - 2 * self.pad + self.K + self.out_pad

    def reads(self, t0: int, t1: int):
        """[lo, hi] of the input positions (unclamped) that outputs [t0, t1) read"""
        s, p, K = self.stride, self.pad, self.K
        if self.kind == "conv":
            return t0 * s - p, (t1 - 1) * s - p + (K - 1) * self.dil
        return -((K - 1 - t0 - p) // s), (t1 - 1 + p) // s

    def ready(self, A: int) -> int:
        """how many outputs the input positions [0, A) determine when more input may follow"""
        s, p, K = self.stride, self.pad, self.K
        n = (A - 1 + p - (K - 1) * self.dil) // s + 1 if self.kind == "conv" else s * A - p
        return max(0, min(n, self.out_len(A)))


class StreamPlan:
    def __init__(self, layers: List[StreamLayer], hop: int, latent_dim: int):
        self.layers, self.hop, self.latent_dim = layers, hop, latent_dim

    def out_len(self, frames: int) -> int:
        L = frames
        for ly in self.layers:
            L = ly.out_len(L)
        return L

    def ready(self, frames: int) -> int:
        """waveform samples that `frames` latent frames determine while more may follow"""
        n = frames
        for ly in self.layers:
            n = ly.ready(n)
        return n

    @property
    def lookahead_frames(self) -> int:
        """frames past a sample's own frame that must arrive before the sample is determined (steady state)"""
        A = 64 * self.hop
        return -((self.ready(A) - A * self.hop) // self.hop)


def stream_plan(model: DacModel) -> StreamPlan:
    """The decoder graph of DacModel._run / decode as a list of StreamLayers (first conv; per DecoderBlock the transposed conv and
    3 x [conv K=7 dilated, conv K=1 + residual]; last conv + tanh).  Pure index arithmetic: runs wherever the model lives."""
    layers: List[StreamLayer] = []

    def add(kind, m, snake, res=None, tanh=False):
        g = m.geom
        shape = m.weight_v.shape
        cin, cout = (shape[0], shape[1]) if g["transposed"] else (shape[1], shape[0])
        layers.append(StreamLayer(kind, m, snake, int(cin), int(cout), int(shape[2]), g["stride"], g.get("dilation", 1), g["padding"],
                                  g.get("output_padding", 0), tanh, res))

    def walk(mods):
        snake = None
        for m in mods:
            if isinstance(m, Snake1d):
                snake = m
            elif isinstance(m, _WN):
                add("convt" if m.geom["transposed"] else "conv", m, snake)
                snake = None
            elif isinstance(m, _Seq) and len(m.items()) == 4 and isinstance(m.items()[0], Snake1d):      # ResidualUnit: x + block(x)
                a0, c0, a1, c1 = m.items()
                unit_in = len(layers)
                add("conv", c0, a0)
                add("conv", c1, a1, res=unit_in)
            elif isinstance(m, _Seq):
                walk(m.items())
            elif isinstance(m, nn.Tanh):
                layers[-1].tanh = True

    walk(model.decoder.items())
    hop = math.prod(ly.stride for ly in layers if ly.kind == "convt")
    return StreamPlan(layers, hop, model.latent_dim)


class _Timeline:
    """One sequence's progress through a StreamPlan, and THE window schedule of both streaming decoders.  Buffer i (layer i's input)
    holds positions [base[i], have[i]) from column 0 of its storage; the windows to come read none before keep[i]; have[-1] counts the
    waveform samples computed; L: the true length per buffer, once the sequence has ended.
    The storage belongs to the decoder: `room(i, kept, shift, n)` makes room for n more positions in buffer i behind the `kept`
    positions [keep, have), which move `shift` columns down to column 0, and returns the column of position have.
    samples / closed: DacRowStreamDecoder's count per row (DacStreamDecoder, whose rows leave their group at a flush, keeps lists)."""

    def __init__(self, n_buf):
        self.have = [0] * (n_buf + 1)
        self.keep = [0] * n_buf
        self.base = [0] * n_buf
        self.L = None
        self.samples = 0                               # handed out so far, a flush's pad included
        self.closed = False

    def fork(self):
        """a second timeline at the same point of an open sequence (DacStreamDecoder: rows that part)"""
        t = type(self)(len(self.keep))
        t.have, t.keep, t.base = list(self.have), list(self.keep), list(self.base)
        return t

    def _room(self, room, i: int, n: int) -> int:
        kept, shift = self.have[i] - self.keep[i], self.keep[i] - self.base[i]
        self.base[i] = self.keep[i]
        return room(i, kept, shift, n)

    def feed(self, n_new: int, room):
        """n_new more latent frames -> (the first one's index, its column in buffer 0)"""
        f0, col = self.have[0], self._room(room, 0, n_new)
        self.have[0] += n_new
        return f0, col

    def windows(self, plan: StreamPlan, final: bool, room):
        """Per layer, in order, the outputs its input now determines (final: up to the true right edge), as
        (layer, x_off, L_true, t0, n, r_off, y_off): RowWindow's fields without the slot.  The output buffer has its room when a window
        is yielded, so it may be run at once or recorded; the left context is trimmed once the generator is exhausted."""
        lys, have = plan.layers, self.have
        if final:
            self.L = [have[0]]
            for ly in lys:
                self.L.append(ly.out_len(self.L[-1]))
        for i, ly in enumerate(lys):
            target = self.L[i + 1] if final else ly.ready(have[i])
            if ly.res is not None:
                target = min(target, have[ly.res])
            t0 = have[i + 1]
            n = target - t0
            if n <= 0:
                continue
            y_off = t0 if i + 1 == len(lys) else t0 - self._room(room, i + 1, n)
            r_off = self.base[ly.res] if ly.res is not None else 0
            have[i + 1] = target
            yield i, self.base[i], self.L[i] if final else _OPEN, t0, n, r_off, y_off
        # left context: what the next window of each reader of buffer i starts at
        for i, ly in enumerate(lys):
            need = max(0, ly.reads(have[i + 1], have[i + 1] + 1)[0])
            for j, lj in enumerate(lys):
                if lj.res == i:
                    need = min(need, have[j + 1])
            self.keep[i] = max(self.keep[i], min(need, have[i]))


class _Group:
    """Rows that share one timeline `t`: bufs[i] is buffer i of all of them, [rows, C, have - base]."""

    def __init__(self, rows, n_buf):
        self.rows = list(rows)
        self.t = _Timeline(n_buf)
        self.bufs = [None] * n_buf

    def split(self, rows):
        g = _Group(rows, len(self.bufs))
        idx = torch.tensor([self.rows.index(r) for r in rows], dtype=torch.long)
        g.t = self.t.fork()
        g.bufs = [None if b is None else b.index_select(0, idx.to(b.device)) for b in self.bufs]
        return g


def _call_operands(dec, ly: StreamLayer):
    """What a _win or _win_rows call of layer ly takes from dec's model: (entry suffix, weight, bias, Snake alpha), the last three as
    device pointers; form and weight are DacModel._route's (uses_mfma stays the only rule).  Resolved once per layer and read: every push
    and flush empties dec._ops (DacModel._folded walks all parameters, more host time than the rest of a windowed call)."""
    ops = dec._ops.get(ly)
    if ops is None:
        f = dec.model._folded()
        form, w = dec.model._route(ly.mod, f)
        alpha = f[ly.snake] if ly.snake is not None else None
        ops = dec._ops[ly] = ("_mfma" if form == "mfma" else "", _dev_f32(w), _dev_f32(f[ly.mod][1]), _dev_f32(alpha))
    return ops


class DacStreamDecoder:
    """Streaming DacModel.decode for `batch` rows.  push(n_new) takes how many more latent frames each row has and returns the new
    waveform samples every row's frames now determine; flush(rows) applies the true right edge (and Dac.decode's min_duration pad).
    For any schedule of pushes the concatenated samples of a row are bit-identical to DacModel.decode(z)[row, 0].
    `source(rows, f0, n, out, col)` writes latent frames [f0, f0 + n) of `rows` into out[:, :, col:col + n] (out [len(rows), Dl, W]).
    Rows that receive the same frames are decoded in one launch per layer; they part when their schedules do.
    All work is queued on the current stream: the decode engine's (see model.DecodeEngine.run_stream)."""

    def __init__(self, model: DacModel, batch: int, source, dtype=torch.float32, device=None):
        self.model, self.batch, self.source = model, int(batch), source
        self.plan = stream_plan(model)
        self.dtype = dtype
        self.device = device if device is not None else next(model.parameters()).device
        self._groups = [_Group(range(self.batch), len(self.plan.layers))]
        self.samples = [0] * self.batch
        self.closed = [False] * self.batch
        self._ops = {}                                 # _call_operands' results of the running push / flush

    # ---- executor of one window (the test suite swaps in a float64 restatement) ---------------------------------------------
    def _conv(self, ly: StreamLayer, x, x_off, L_true, t0, n, resid, r_off, y, y_off):
        """outputs [t0, t0 + n) of layer ly into y (positions [y_off, ...)); x / resid hold positions from x_off / r_off"""
        sfx, w, b, a = _call_operands(self, ly)
        assert x.shape[1] == ly.cin and y.shape[1] == ly.cout and y.shape[0] == x.shape[0]
        assert resid is None or (resid.shape[:2] == y.shape[:2])
        if ly.kind == "conv":
            _lib_call("umoe_dac_conv1d_win" + sfx, _dev_f32(x), x_off, x.shape[2], w, b, a, _dev_f32(resid), r_off,
                      0 if resid is None else resid.shape[2], x.shape[0], ly.cin, L_true, ly.cout, ly.K, ly.stride, ly.dil, ly.pad,
                      int(ly.tanh), t0, n, _dev_f32(y), y_off, y.shape[2], _stream())
        else:
            _lib_call("umoe_dac_conv_transpose1d_win" + sfx, _dev_f32(x), x_off, x.shape[2], w, b, a, x.shape[0],
                      ly.cin, L_true, ly.cout, ly.K, ly.stride, ly.pad, ly.out_pad, t0, n, _dev_f32(y), y_off, y.shape[2], _stream())

    def _empty(self, *shape):
        return torch.empty(shape, dtype=self.dtype, device=self.device)

    def _append(self, g: _Group, i: int, kept: int, shift: int, n: int) -> int:
        """_Timeline's room(): a fresh tensor for buffer i, the kept part copied to its front"""
        old = g.bufs[i]
        g.bufs[i] = self._empty(len(g.rows), self.plan.layers[i].cin, kept + n)
        if kept:
            g.bufs[i][:, :, :kept] = old[:, :, shift:shift + kept]
        return kept

    def _advance(self, g: _Group, n_new: int, final: bool) -> torch.Tensor:
        lys = self.plan.layers
        room = functools.partial(self._append, g)
        if n_new:
            f0, col = g.t.feed(n_new, room)
            self.source(g.rows, f0, n_new, g.bufs[0], col)
        wave = None
        t_wave = g.t.have[-1]
        for i, x_off, L_true, t0, n, r_off, y_off in g.t.windows(self.plan, final, room):          # every window runs as it is produced
            ly = lys[i]
            y = self._empty(len(g.rows), ly.cout, n) if i + 1 == len(lys) else g.bufs[i + 1]
            self._conv(ly, g.bufs[i], x_off, L_true, t0, n, g.bufs[ly.res] if ly.res is not None else None, r_off, y, y_off)
            if i + 1 == len(lys):
                wave = y[:, 0]
        if wave is None:
            wave = self._empty(len(g.rows), 0)
        assert wave.shape[1] == g.t.have[-1] - t_wave
        return wave

    def _regroup(self, key):
        """split every group so that all rows of a group have the same key(row)"""
        out = []
        for g in self._groups:
            ks = {}
            for r in g.rows:
                ks.setdefault(key(r), []).append(r)
            out.extend([g] if len(ks) == 1 else [g.split(rs) for rs in ks.values()])
        self._groups = out

    def push(self, n_new) -> dict:
        """n_new: more latent frames per row (a list of `batch` ints, or one int for all) -> {row: new samples (1-D tensor)}"""
        n_new = [int(n_new)] * self.batch if isinstance(n_new, int) else [int(v) for v in n_new]
        assert len(n_new) == self.batch and min(n_new) >= 0
        for r in range(self.batch):
            if n_new[r] and self.closed[r]:
                raise ValueError(f"row {r} was flushed already")
        self._ops = {}
        self._regroup(lambda r: n_new[r])
        out = {}
        for g in self._groups:
            n = n_new[g.rows[0]]
            if n:
                w = self._advance(g, n, False)
                for k, r in enumerate(g.rows):
                    out[r] = w[k]
                    self.samples[r] += w.shape[1]
        return out

    def flush(self, rows, min_duration=None) -> dict:
        """The rest of each row's waveform: the true right edge (a decode of T frames has plan.out_len(T) samples), then the zero pad
        Dac.decode appends when the audio is shorter than min_duration seconds -> {row: samples (1-D tensor)}"""
        rows = [rows] if isinstance(rows, int) else list(rows)
        todo = set(rows)
        for r in rows:
            if self.closed[r]:
                raise ValueError(f"row {r} was flushed already")
        self._ops = {}
        self._regroup(lambda r: r in todo)
        out = {}
        keep = []
        for g in self._groups:
            if g.rows[0] not in todo:
                keep.append(g)
                continue
            w = self._advance(g, 0, True)
            for k, r in enumerate(g.rows):
                a = w[k]
                pad = min_duration_pad(self.samples[r] + a.shape[0], self.model.sample_rate, min_duration)
                if pad:
                    a = torch.cat((a, torch.zeros(pad, dtype=a.dtype, device=a.device)))
                out[r] = a
                self.samples[r] += a.shape[0]
                self.closed[r] = True
        self._groups = keep
        return out


def _lib_call(name, *args):
    L.check(getattr(L.lib(), name)(*args), name)


class _DelayedSource:
    """What both sources of latent frames share: the engine's delayed token buffer, the delay pattern, the codebooks and output
    projections of the engine's codec channels, and THE umoe_rvq_from_delayed call.  Frame t of row b reverts the delay pattern,
    tokens[b][prefill_step_b + t + delay_c][c], and sums the codebook rows like DacModel.from_codes, bit for bit; token positions at
    or past t_valid read as the pad code, as DecodeEngine.finish() has it."""

    def __init__(self, engine, model: DacModel):
        self.engine, self.model = engine, model
        self.pad = int(engine.cfg.codec_pad_value)
        self.delay = torch.tensor(list(engine.cfg.codec_delay_pattern), dtype=torch.int32, device=engine.tokens.device)

    def _refuse_missing_codebooks(self):
        NQ = self.engine.tokens.shape[2]
        if NQ > self.model.n_codebooks:
            raise L.UmoeError(f"{NQ} codec channels, the DAC has {self.model.n_codebooks} codebooks")

    def _weights(self):
        f, NQ = self.model._folded(), self.engine.tokens.shape[2]
        return f["cb"][:NQ].contiguous(), f["out_w"][:NQ].contiguous(), f["out_b"][:NQ].contiguous()

    def _from_delayed(self, weights, *, prefill, t_valid, rows, n_rows, f0, n, out, col):
        """frames [f0, f0 + n) of the n_rows rows whose ids the int32 tensor `rows` starts with -> out[k, :, col:col + n]; out is
        [n_rows, Dl, W], or for one row its plane [Dl, W].  weights: _weights(), taken once per read (it goes through DacModel._folded)"""
        B, Tmax, NQ = self.engine.tokens.shape
        cb, ow, ob = weights
        _lib_call("umoe_rvq_from_delayed", C.c_void_p(self.engine.tokens.data_ptr()), B, Tmax, NQ, C.c_void_p(prefill.data_ptr()),
                  C.c_void_p(self.delay.data_ptr()), int(t_valid), self.pad, C.c_void_p(rows.data_ptr()), n_rows, f0, n,
                  _dev_f32(cb), _dev_f32(ow), _dev_f32(ob), cb.shape[1], cb.shape[2], ow.shape[1], _dev_f32(out), col, out.shape[-1], _stream())


class DelayedTokenSource(_DelayedSource):
    """Latent frames straight from a decode engine's delayed token buffer, for DacStreamDecoder: all rows on the engine's one clock.
    `t_valid`: dec_step + 1 of the last state read."""

    def __init__(self, engine, model: DacModel):
        super().__init__(engine, model)
        self.prefill = torch.tensor(engine.prefill_steps, dtype=torch.int32, device=engine.tokens.device)
        self.t_valid = 0
        self._rows = {}

    def __call__(self, rows, f0, n, out, col):
        self._refuse_missing_codebooks()
        key = tuple(rows)
        if key not in self._rows:
            self._rows[key] = torch.tensor(rows, dtype=torch.int32, device=self.engine.tokens.device)
        self._from_delayed(self._weights(), prefill=self.prefill, t_valid=self.t_valid, rows=self._rows[key], n_rows=len(rows), f0=f0, n=n,
                           out=out, col=col)


# ----------------------------------------------------------------------------------------------- one timeline per row
# A served batch (UniMoEAudio.serve) admits every request at a poll of its own, so R live rows are on up to R timelines and
# DacStreamDecoder would part them into R groups: R launches per layer and read, each filling a small part of the GPU.
# DacRowStreamDecoder keeps one _Timeline PER ROW (the schedule above, unchanged) over slabs [slots][C][W], records the windows the
# timelines produce and hands every layer the windows of all rows at once: umoe_dac_conv1d_win_rows / umoe_dac_conv_transpose1d_win_rows
# read each row's window from a table (umoe.h "Per-row window tables"), one launch per layer whatever the rows are doing.

DAC_ROW_FIELDS = ("x", "resid", "y", "x_off", "Lx", "r_off", "Lr", "y_off", "Ly", "t_begin", "n", "L")      # umoe.h UMOE_DAC_ROW_WORDS
RVQ_ROW_FIELDS = ("row", "f0", "n", "t_valid", "z", "col", "Lz", "reserved")                                  # UMOE_RVQ_ROW_WORDS
SHIFT_ROW_FIELDS = ("plane", "W", "shift", "count")                                                           # UMOE_SHIFT_ROW_WORDS


def dac_row_words(x=0, resid=0, y=0, x_off=0, Lx=0, r_off=0, Lr=0, y_off=0, Ly=0, t_begin=0, n=0, L=0) -> List[int]:
    """one row of a window table, in the word order of umoe.h (a row that is all zeros is idle: n = 0)"""
    v = dict(x=x, resid=resid, y=y, x_off=x_off, Lx=Lx, r_off=r_off, Lr=Lr, y_off=y_off, Ly=Ly, t_begin=t_begin, n=n, L=L)
    return [int(v[k]) for k in DAC_ROW_FIELDS]


class RowWindow(NamedTuple):
    """outputs [t0, t0 + n) of one layer for the row in `slot`; buffer positions as DacStreamDecoder._conv takes them"""
    slot: int
    x_off: int
    L_true: int
    t0: int
    n: int
    r_off: int
    y_off: int


class DacRowStreamDecoder:
    """DacStreamDecoder with one timeline per row, for rows that come and go (UniMoEAudio.serve(stream=True)).
    push(n_new): how many more latent frames each of the `slots` rows has -> {row: new samples}; flush(rows, min_duration): the true
    right edge and Dac.decode's pad; reset(row): a flushed row starts over at frame 0 for the next request.  For any schedule a row's
    samples between two resets are bit-identical to DacModel.decode of its frames.
    `source(requests, slab)`: requests = [(row, f0, n, col)], writes latent frames [f0, f0 + n) of each row into slab[row, :, col:col + n]
    (slab [slots, Dl, W]); a source with a `table_words` attribute is given its slice of the read's table instead (DelayedRowsSource).
    `max_frames`: the most frames a push brings per row (the slabs are sized for it; a larger push still works, a slab then grows).
    ragged=True: per layer ONE library call for all rows (the table kernels); the number of calls in a push is 1 + buffers + layers,
    whatever the rows do.  ragged=False, the yardstick: the same bookkeeping, one umoe_dac_*_win call per (layer, row with news).
    All work is queued on the current stream."""

    def __init__(self, model: DacModel, slots: int, source, max_frames: int = 25, ragged: bool = True, dtype=torch.float32, device=None):
        self.model, self.slots, self.source, self.ragged = model, int(slots), source, bool(ragged)
        self.plan = stream_plan(model)
        self.dtype = dtype
        self.device = device if device is not None else next(model.parameters()).device
        lys = self.plan.layers
        self.rows = [_Timeline(len(lys)) for _ in range(self.slots)]      # buffer i of row r: columns [0, have - base) of plane bufs[i][r]
        per_frame, self.chan = [1], [lys[0].cin]
        for ly in lys[:-1]:
            per_frame.append(per_frame[-1] * (ly.stride if ly.kind == "convt" else 1))
            self.chan.append(ly.cout)
        room = int(max_frames) + self.plan.lookahead_frames + 2
        self.bufs = [self._empty(self.slots, c, p * room + 64) for c, p in zip(self.chan, per_frame)]
        self.grown = 0
        self.last_plan = None          # what the last push / flush asked of the executor (tests, measurements)
        self._ops = {}                 # _call_operands' results of the running push / flush

    def _empty(self, *shape):
        return torch.empty(shape, dtype=self.dtype, device=self.device)

    # ---- bookkeeping: row r's timeline advances, the work is recorded instead of done -------------------------------------------
    def _room(self, work, r: int, i: int, kept: int, shift: int, n: int) -> int:
        """_Timeline's room() for buffer i of row r: the kept context's move to column 0 is recorded; a slab too narrow for kept + n grows"""
        if shift:
            work["shift"][i].append((r, shift, kept))
        if kept + n > self.bufs[i].shape[2]:
            old = self.bufs[i]
            self.bufs[i] = self._empty(old.shape[0], old.shape[1], 2 * (kept + n))
            self.bufs[i][:, :, :old.shape[2]] = old
            self.grown += 1
        return kept

    def _advance(self, work, r: int, n_new: int, final: bool):
        st, room = self.rows[r], functools.partial(self._room, work, r)
        if n_new:
            f0, col = st.feed(n_new, room)
            work["src"].append((r, f0, n_new, col))
        for i, *window in st.windows(self.plan, final, room):
            work["conv"][i].append(RowWindow(r, *window))

    # ---- executors ------------------------------------------------------------------------------------------------------------
    _conv = DacStreamDecoder._conv     # one window of one row through the _win entry (the grouped executor; tests swap in float64)

    def _planes(self, i: int, w: RowWindow, wave):
        """(x, resid, y) of a window of layer i, each the [1, C, W] plane of the row's slot"""
        ly = self.plan.layers[i]
        s = slice(w.slot, w.slot + 1)
        y = wave[s] if i + 1 == len(self.plan.layers) else self.bufs[i + 1][s]
        return self.bufs[i][s], (self.bufs[ly.res][s] if ly.res is not None else None), y

    def _shift(self, i: int, moves, table=None):
        """buffer i: per (row, shift, count) the columns [shift, shift + count) of the row's plane move to [0, count), one launch for all"""
        buf = self.bufs[i]
        if table is None:
            host = torch.zeros((self.slots, len(SHIFT_ROW_FIELDS)), dtype=torch.int64)
            for r, shift, count in moves:
                host[r] = torch.tensor([buf[r].data_ptr(), buf.shape[2], shift, count])
            table = (host, host.to(self.device))
        host, dev = table
        _lib_call("umoe_dac_shift_rows", C.c_void_p(host.data_ptr()), C.c_void_p(dev.data_ptr()), self.slots, buf.shape[1], _stream())

    def _conv_rows(self, i: int, wins: List[RowWindow], wave, table):
        """layer i: the windows of all rows in one launch; table = (host [slots, 12], its device copy)"""
        ly = self.plan.layers[i]
        sfx, w, b, a = _call_operands(self, ly)
        host, dev = table
        max_n = max((v.n for v in wins), default=0)
        if ly.kind == "conv":
            _lib_call("umoe_dac_conv1d_win_rows" + sfx, C.c_void_p(host.data_ptr()), C.c_void_p(dev.data_ptr()), self.slots, max_n, w, b, a,
                      ly.cin, ly.cout, ly.K, ly.stride, ly.dil, ly.pad, int(ly.tanh), _stream())
        else:
            _lib_call("umoe_dac_conv_transpose1d_win_rows" + sfx, C.c_void_p(host.data_ptr()), C.c_void_p(dev.data_ptr()), self.slots, max_n,
                      w, b, a, ly.cin, ly.cout, ly.K, ly.stride, ly.pad, ly.out_pad, _stream())

    def _tables(self, work, wave):
        """Every table of a read in one int64 tensor [source rows | per buffer the moves | per layer the windows], `slots` rows each (a
        row without news is all zeros: idle), and ONE copy to the device.  -> (host, device) views per section"""
        lys, S = self.plan.layers, self.slots
        nw = getattr(self.source, "table_words", 0)
        ns, nc = len(SHIFT_ROW_FIELDS), len(DAC_ROW_FIELDS)
        host = torch.zeros(S * (nw + ns * len(self.bufs) + nc * len(lys)), dtype=torch.int64)
        o = S * nw
        shift_at, conv_at = [], []
        for i, buf in enumerate(self.bufs):
            sec = host[o:o + S * ns].view(S, ns)
            for r, shift, count in work["shift"][i]:
                sec[r] = torch.tensor([buf[r].data_ptr(), buf.shape[2], shift, count])
            shift_at.append(o)
            o += S * ns
        for i, ly in enumerate(lys):
            sec = host[o:o + S * nc].view(S, nc)
            for v in work["conv"][i]:
                x, resid, y = self._planes(i, v, wave)
                sec[v.slot] = torch.tensor(dac_row_words(x=x.data_ptr(), resid=0 if resid is None else resid.data_ptr(), y=y.data_ptr(),
                                                         x_off=v.x_off, Lx=x.shape[2], r_off=v.r_off, Lr=0 if resid is None else resid.shape[2],
                                                         y_off=v.y_off, Ly=y.shape[2], t_begin=v.t0, n=v.n, L=v.L_true))
            conv_at.append(o)
            o += S * nc
        if nw:
            self.source.fill_table(host[:S * nw].view(S, nw), work["src"], self.bufs[0])
        dev = self._upload(host)
        cut = lambda at, n: (host[at:at + S * n].view(S, n), dev[at:at + S * n].view(S, n))      # noqa: E731
        return cut(0, nw) if nw else None, [cut(at, ns) for at in shift_at], [cut(at, nc) for at in conv_at]

    def _upload(self, host: torch.Tensor) -> torch.Tensor:
        return host.to(self.device)

    def _execute(self, work, wave):
        lys = self.plan.layers
        if self.ragged:
            src_t, shift_t, conv_t = self._tables(work, wave)
            for i in range(len(self.bufs)):          # (the moves first: new frames and outputs land behind the moved context)
                self._shift(i, work["shift"][i], shift_t[i])
            if src_t is not None:
                self.source.run_table(src_t, work["src"], self.bufs[0])
            elif work["src"]:
                self.source(work["src"], self.bufs[0])
            for i in range(len(lys)):
                self._conv_rows(i, work["conv"][i], wave, conv_t[i])
            return
        # the yardstick: moves first (as above, one launch per buffer that has any), then per layer one _win call per row with news
        for i in range(len(self.bufs)):
            if work["shift"][i]:
                self._shift(i, work["shift"][i])
        if work["src"]:
            self.source(work["src"], self.bufs[0])
        for i, ly in enumerate(lys):
            for v in work["conv"][i]:
                x, resid, y = self._planes(i, v, wave)
                self._conv(ly, x, v.x_off, v.L_true, v.t0, v.n, resid, v.r_off, y, v.y_off)

    def _run(self, todo, final: bool, pads=None) -> dict:
        """todo: {row: n_new}; plans every row, executes once, counts what it hands out -> {row: samples}"""
        lys = self.plan.layers
        work = {"src": [], "shift": [[] for _ in self.bufs], "conv": [[] for _ in lys]}
        before = {r: self.rows[r].have[-1] for r in todo}
        for r, n in todo.items():
            self._advance(work, r, n, final)
        got = {r: self.rows[r].have[-1] - before[r] for r in todo}
        # the waveform of this call: plane r holds row r's new samples from column 0, then (flush) its zero pad
        width = max((got[r] + (pads[r] if pads else 0) for r in todo), default=0)
        wave = (torch.zeros if pads else torch.empty)((self.slots, 1, max(width, 1)), dtype=self.dtype, device=self.device)
        self.last_plan, self._ops = work, {}
        self._execute(work, wave)
        out = {r: wave[r, 0, :got[r] + (pads[r] if pads else 0)] for r in todo}
        for r, a in out.items():
            self.rows[r].samples += a.shape[0]
            self.rows[r].closed = final                # (push lets only open rows through)
        return out

    def push(self, n_new) -> dict:
        """n_new: more latent frames per row (`slots` ints; 0: the row is idle in this push) -> {row: new samples (1-D tensor)} for
        the rows with frames"""
        n_new = [int(v) for v in n_new]
        assert len(n_new) == self.slots and min(n_new) >= 0
        for r, n in enumerate(n_new):
            if n and self.rows[r].closed:
                raise ValueError(f"row {r} was flushed already (reset it for the next request)")
        return self._run({r: n for r, n in enumerate(n_new) if n}, False)

    def flush(self, rows, min_duration=None) -> dict:
        """The rest of each row's waveform: the true right edge (a decode of T frames has plan.out_len(T) samples), then the zero pad
        Dac.decode appends when the audio is shorter than min_duration seconds -> {row: samples (1-D tensor)}"""
        rows = [rows] if isinstance(rows, int) else list(rows)
        pads = {}
        for r in rows:
            st = self.rows[r]
            if st.closed:
                raise ValueError(f"row {r} was flushed already")
            # (known before the windows run: the pad is part of the wave tensor they write into)
            pads[r] = min_duration_pad(self.plan.out_len(st.have[0]) if st.have[0] else 0, self.model.sample_rate, min_duration)
        return self._run({r: 0 for r in rows}, True, pads)

    def reset(self, row: int):
        """row `row` (flushed, or never used) starts over: the next push is frame 0 of a new sequence"""
        self.rows[row] = _Timeline(len(self.plan.layers))


class DelayedRowsSource(_DelayedSource):
    """The source of DacRowStreamDecoder: every row reads the token buffer on its own clock.  t_valid[row]: the row's local step + 1
    at the last state read (serve.final_frames).  Under the ragged executor the requests of a read are one table section and one
    umoe_rvq_from_delayed_rows launch; called directly (the grouped executor) it is one umoe_rvq_from_delayed per row."""
    table_words = len(RVQ_ROW_FIELDS)

    def __init__(self, engine, model: DacModel):
        super().__init__(engine, model)
        self._refuse_missing_codebooks()
        self.t_valid = [0] * engine.tokens.shape[0]
        self._row_ids = torch.arange(engine.tokens.shape[0], dtype=torch.int32, device=engine.tokens.device)

    def _prefill(self):
        """the rows' prefill steps on the device: words [3B, 4B) of the engine's state, which admissions keep current"""
        B = self.engine.tokens.shape[0]
        return self.engine.state[3 * B:4 * B]

    def fill_table(self, sec: torch.Tensor, requests, slab: torch.Tensor):
        for row, f0, n, col in requests:
            sec[row] = torch.tensor([row, f0, n, self.t_valid[row], slab[row].data_ptr(), col, slab.shape[2], 0])

    def run_table(self, table, requests, slab: torch.Tensor):
        host, dev = table
        eng = self.engine
        B, Tmax, NQ = eng.tokens.shape
        cb, ow, ob = self._weights()
        _lib_call("umoe_rvq_from_delayed_rows", C.c_void_p(eng.tokens.data_ptr()), B, Tmax, NQ, C.c_void_p(self._prefill().data_ptr()),
                  C.c_void_p(self.delay.data_ptr()), self.pad, C.c_void_p(host.data_ptr()), C.c_void_p(dev.data_ptr()), host.shape[0],
                  max((n for _, _, n, _ in requests), default=0), _dev_f32(cb), _dev_f32(ow), _dev_f32(ob), cb.shape[1], cb.shape[2],
                  ow.shape[1], _stream())

    def __call__(self, requests, slab: torch.Tensor):
        weights = self._weights()
        for row, f0, n, col in requests:
            self._from_delayed(weights, prefill=self._prefill(), t_valid=self.t_valid[row], rows=self._row_ids[row:], n_rows=1, f0=f0, n=n,
                               out=slab[row], col=col)
