"""The mRoPE cos / sin tables the decode kernels read (ops.rope_tables) against the reference's rotary embedding as oracle/decode.py
restates it (rope_cos_sin + mrope_select), on the host.  The fused decode kernel (umoe_attn.hip, rope32) and the append kernel
(rope_append_kernel) index these tables by position and half-dim, and pick the position stream of a dim by the section rule
restated below; both must land on exactly the entries the reference multiplies by."""
import torch

from oracle import decode as OD
from unimoe_audio_amd import ops

HD, THETA, SECTIONS = 128, 1e6, (16, 24, 24)


def _kernel_stream(i, sec):
    """umoe_attn.hip: half-dim i < sec0 -> stream 0, < sec0 + sec1 -> stream 1, else stream 2 (dim i + 64 shares dim i's stream)"""
    return 0 if i < sec[0] else (1 if i < sec[0] + sec[1] else 2)


def test_rope_tables_equal_reference_rotary_at_every_engine_position():
    # the engine sizes its tables for Lmax + 4104 positions (DecodeEngine._pack_weights); Lmax of the benchmark's headline run:
    # 300-token prompt + 510 steps + 8
    Lmax = 300 + 510 + 8
    n = Lmax + 4104
    cos_t, sin_t = ops.rope_tables(n, HD, THETA, "cpu")
    assert cos_t.dtype == torch.bfloat16 and cos_t.shape[0] >= n and cos_t.shape[1] == HD // 2
    pos = torch.arange(cos_t.shape[0]).view(1, 1, -1)
    cos_r, sin_r = OD.rope_cos_sin(pos, HD, THETA, torch.bfloat16)       # [1, 1, n, 128]
    cos_r, sin_r = cos_r[0, 0], sin_r[0, 0]
    for tab, ref in ((cos_t, cos_r), (sin_t, sin_r)):
        # bit for bit, both halves of the reference's cat((freqs, freqs)) -- the kernels read dim i + 64 from column i
        assert torch.equal(tab.view(torch.int16), ref[:, : HD // 2].contiguous().view(torch.int16))
        assert torch.equal(tab.view(torch.int16), ref[:, HD // 2:].contiguous().view(torch.int16))
    # a table built for a shorter length is a prefix of the long one (the engine and the module path build different sizes)
    c2, s2 = ops.rope_tables(300, HD, THETA, "cpu")
    assert torch.equal(c2, cos_t[: c2.shape[0]]) and torch.equal(s2, sin_t[: s2.shape[0]])


def test_kernel_section_rule_selects_the_reference_mrope_entries():
    """Three distinct, large position streams per token: the table entry the kernels' section rule picks for every dim equals
    mrope_select of the reference's per-stream cos / sin."""
    Lmax = 300 + 510 + 8
    cos_t, sin_t = ops.rope_tables(Lmax + 4104, HD, THETA, "cpu")
    top = Lmax + 4104 - 1
    g = torch.Generator().manual_seed(5)
    T = 64
    pos3 = torch.randint(0, top + 1, (3, 1, T), generator=g)
    pos3[:, 0, 0] = torch.tensor([top, top - 1, 0])
    pos3[:, 0, 1] = torch.tensor([0, top, 4321])
    for sec in (SECTIONS, (8, 32, 24), (24, 16, 24)):
        cos3, sin3 = OD.rope_cos_sin(pos3, HD, THETA, torch.bfloat16)
        cos_r, sin_r = OD.mrope_select(cos3, list(sec))[0], OD.mrope_select(sin3, list(sec))[0]    # [T, 128]
        half = HD // 2
        stream = torch.tensor([_kernel_stream(i, sec) for i in range(half)])
        p = pos3[:, 0].T[:, stream]                                   # [T, 64]: the position each half-dim reads
        col = torch.arange(half).expand(T, -1)
        for tab, ref in ((cos_t, cos_r), (sin_t, sin_r)):
            got = tab[p, col]
            assert torch.equal(got.view(torch.int16), ref[:, :half].contiguous().view(torch.int16)), sec
            assert torch.equal(got.view(torch.int16), ref[:, half:].contiguous().view(torch.int16)), sec
