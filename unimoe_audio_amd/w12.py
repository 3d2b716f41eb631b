"""WP12: bf16 expert weights of the flat expert launch in 12 bits per weight, lossless (include/umoe.h "WP12").

A bf16 weight's high byte (sign + exponent bits 7..1) carries under 3 bits of information in a trained or initialised matrix; its low byte
(exponent bit 0 + mantissa) is noise.  WP12 keeps the low byte raw and codes the high byte in 4 bits: sign + a 3-bit offset into a
window of 8 consecutive high-byte exponents (16 binades), one window base per 16-row block.  A value whose high byte lies outside the
window (zeros, denormals, inf / NaN, outliers, tiny values) keeps its true bf16 in the block's exception list, which the kernel patches
into the decoded operand.  A block with more than CAP exceptions makes the matrix "not packable": the layer runs the bf16 launch.

Device-agnostic torch code: the CPU tests and the engine's load-time pack run the same functions.  Input and output of pack / unpack is
the WP16 tensor (umoe_pack_weight / umoe_pack_gate_up), so the operand a lane rebuilds is the WP16 one by construction."""
from typing import Optional, Tuple

import torch

CAP = 32            # exceptions per 16-row block
META = 40           # u32 per block: entries [0, CAP] (sentinel-terminated, the rest sentinels), window base in word META - 1;
                    # an entry: k-step << 25 | lane << 19 | element << 16 | bf16 bits (the sentinel reads as k-step 127)
SENTINEL = 0xFFFFFFFF


def wp16_from_rows(W: torch.Tensor) -> torch.Tensor:
    """WP16 order of a row-major bf16 matrix [N][K] (N % 16 == 0, K % 32 == 0) as int16 [N/16 * K/32 * 64 * 8] (include/umoe.h)."""
    N, K = W.shape
    assert N % 16 == 0 and K % 32 == 0, (N, K)
    v = W.contiguous().view(torch.int16).view(N // 16, 16, 4, K // 32, 8)      # [nb][r][h][i][j]
    return v.permute(0, 3, 2, 1, 4).contiguous().view(-1)                      # [nb][i][h][r][j]: lane = 16 h + r


def rows_from_wp16(p: torch.Tensor, N: int, K: int) -> torch.Tensor:
    v = p.view(N // 16, K // 32, 4, 16, 8).permute(0, 3, 2, 1, 4).contiguous()
    return v.view(N, K).view(torch.bfloat16)


def wp16_gate_up(Wg: torch.Tensor, Wu: torch.Tensor) -> torch.Tensor:
    """gate / up blocks interleaved per 16 rows (umoe_pack_gate_up)."""
    I, K = Wg.shape
    both = torch.stack([Wg.view(I // 16, 16, K), Wu.view(I // 16, 16, K)], 1).reshape(2 * I, K)
    return wp16_from_rows(both)


def steps_per_chunk(KB: int) -> int:
    """k-steps a lane's register stage holds: 2 (16 low bytes + 8 code bytes) when KB is even, else 1 (8 + 4)."""
    return 2 if KB % 2 == 0 else 1


def block_bytes(KB: int) -> int:
    return KB * 768


def pack(wp16: torch.Tensor, KB: int, cap: int = CAP) -> Optional[Tuple[torch.Tensor, torch.Tensor]]:
    """WP16 (int16, [NB * KB * 64 * 8]) -> (data uint8 [NB * KB * 768], meta int32 [NB * META]), or None when a block has more than
    `cap` exceptions (not packable).  Block nb of `data`: the low bytes of its KB * 512 values in WP16 order -- chunked so that a lane's
    CS = steps_per_chunk(KB) k-steps are 8 CS contiguous bytes: [chunk][lane][step][8] -- then its code words [chunk][lane][step] (u32:
    byte b holds value (0, 1, 4, 5)[b] in its low nibble and value (2, 3, 6, 7)[b] in its high one)."""
    assert cap <= CAP and wp16.dtype == torch.int16 and wp16.numel() % (KB * 512) == 0 and 0 < KB < 127
    NB = wp16.numel() // (KB * 512)
    CS = steps_per_chunk(KB)
    v = wp16.view(NB, KB, 64, 8).to(torch.int32) & 0xFFFF
    lo, hb = v & 0xFF, v >> 8
    e7, sg = hb & 0x7F, hb >> 7
    # the window of 8 high-byte exponents that covers most of the block (ties: the lowest base)
    hist = torch.zeros(NB, 129, dtype=torch.int64, device=v.device)
    hist[:, 1:].scatter_add_(1, e7.view(NB, -1).to(torch.int64), torch.ones(1, dtype=torch.int64, device=v.device).expand(NB, KB * 512))
    cum = hist.cumsum(1)
    wb = (cum[:, 8:] - cum[:, :-8]).argmax(1).to(torch.int32)                  # base in [0, 120]
    off = e7 - wb.view(NB, 1, 1, 1)
    inwin = (off >= 0) & (off < 8)
    code = torch.where(inwin, (sg << 3) | off, torch.zeros_like(off))
    exc = (~inwin).nonzero()                                                   # rows (nb, i, lane, j), ascending: by k-step within a block
    meta = torch.full((NB, META), -1, dtype=torch.int64, device=v.device)
    if exc.shape[0]:
        cnt = torch.bincount(exc[:, 0], minlength=NB)
        if int(cnt.max()) > cap:
            return None
        first = cnt.cumsum(0) - cnt
        rank = torch.arange(exc.shape[0], device=v.device) - first[exc[:, 0]]
        val = v[exc[:, 0], exc[:, 1], exc[:, 2], exc[:, 3]].to(torch.int64)
        meta[exc[:, 0], rank] = (exc[:, 1] << 25) | (exc[:, 2] << 19) | (exc[:, 3] << 16) | val
    meta[:, META - 1] = wb.to(torch.int64)
    meta = torch.where(meta >= 2 ** 31, meta - 2 ** 32, meta).to(torch.int32)      # (the u32 bits in an int32 tensor)
    cb = torch.stack([code[..., 0] | (code[..., 2] << 4), code[..., 1] | (code[..., 3] << 4),
                      code[..., 4] | (code[..., 6] << 4), code[..., 5] | (code[..., 7] << 4)], -1)       # [NB][KB][64][4]
    lows = lo.view(NB, KB // CS, CS, 64, 8).permute(0, 1, 3, 2, 4).reshape(NB, KB * 512)
    codes = cb.view(NB, KB // CS, CS, 64, 4).permute(0, 1, 3, 2, 4).reshape(NB, KB * 256)
    data = torch.cat([lows, codes], 1).to(torch.uint8).contiguous().view(-1)
    return data, meta.contiguous().view(-1)


def unpack(data: torch.Tensor, meta: torch.Tensor, KB: int) -> torch.Tensor:
    """The WP16 tensor (int16) that pack() was given."""
    NB = meta.numel() // META
    CS = steps_per_chunk(KB)
    d = data.view(NB, KB * 768).to(torch.int32)
    lo = d[:, : KB * 512].view(NB, KB // CS, 64, CS, 8).permute(0, 1, 3, 2, 4).reshape(NB, KB, 64, 8)
    cb = d[:, KB * 512:].view(NB, KB // CS, 64, CS, 4).permute(0, 1, 3, 2, 4).reshape(NB, KB, 64, 4)
    l4, h4 = cb & 0xF, cb >> 4
    code = torch.stack([l4[..., 0], l4[..., 1], h4[..., 0], h4[..., 1], l4[..., 2], l4[..., 3], h4[..., 2], h4[..., 3]], -1)
    m = meta.view(NB, META).to(torch.int64) & 0xFFFFFFFF
    wb = m[:, META - 1].to(torch.int32).view(NB, 1, 1, 1)
    v = (((code & 8) << 4) | ((code & 7) + wb)) << 8 | lo
    ent = m[:, : CAP + 1]
    nb, r = (ent != SENTINEL).nonzero(as_tuple=True)
    en = ent[nb, r]
    v[nb, (en >> 25) & 0x7F, (en >> 19) & 63, (en >> 16) & 7] = (en & 0xFFFF).to(torch.int32)
    return torch.where(v >= 0x8000, v - 0x10000, v).to(torch.int16).view(-1)


def exceptions_per_block(meta: torch.Tensor) -> torch.Tensor:
    m = meta.view(-1, META).to(torch.int64) & 0xFFFFFFFF
    return (m[:, : CAP + 1] != SENTINEL).sum(1)
