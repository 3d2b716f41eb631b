"""Weight-only FP8 (OCP e4m3) expert weights for the decode engine.

Format: every output row of an expert weight W[N][K] gets a power-of-two scale 2^e (int8 e, the MX E8M0 idea applied per row) and
elements q = fp8_e4m3fn(W / 2^e), rounded to nearest even.  e = ceil(log2(amax_row / 448)), so |W / 2^e| <= 448 and no element ever
needs saturation; an all-zero row has e = 0.  Because the scale is a power of two, q * 2^e is exactly representable in bf16: the
quantized model IS an ordinary bf16 model with weights W_deq = q * 2^e.  quantize_experts_ overwrites the expert parameters with W_deq,
so prefill, the module-level forward and training run the unchanged bf16 kernels on the numbers the fp8 decode launch
(moe_flat_fp8_kernel) converts to -- its outputs are bit-identical to the bf16 engine run on W_deq.

fp8-only (quantize_experts_(keep_bf16=False)): the expert parameters are RELEASED once their WP8 copy exists (`p.data` becomes an
empty tensor, shapes stay in `_fp8["shape"]`), and an engine built on such a model holds the WP8 copy of every expert and nothing else:
its prefill runs the tiled GEMM on the e4m3 blocks (umoe_tiled_gemm_wp8).  The module forward, training and state_dict saving of such a
model raise; dequantize_experts_ restores W_deq exactly.

Load-time only (torch ops, CPU or GPU): not a hot path.  WP8 layout: include/umoe.h.
"""
from typing import Tuple

import torch

FP8_MAX = 448.0
E_MIN, E_MAX = -117, 127      # 2^e stays a normal float32 / bf16 scale and q * 2^e (q >= 2^-9) stays a normal bf16


def quantize_fp8_rows(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """w [N, K] (any float dtype) -> (q uint8 [N, K] = e4m3fn bits, e int8 [N]).  Refuses inf / NaN."""
    if w.dim() != 2:
        raise ValueError(f"quantize_fp8_rows: expected a 2-D weight, got shape {tuple(w.shape)}")
    wf = w.detach().float()
    if not bool(torch.isfinite(wf).all()):
        raise ValueError("quantize_fp8_rows: the weight holds inf or NaN")
    amax = wf.abs().amax(1).double()
    nz = amax > 0
    safe = torch.where(nz, amax, torch.ones_like(amax))
    e = torch.ceil(torch.log2(safe / FP8_MAX))
    # exact correction of log2's rounding: the smallest e with amax <= 448 * 2^e
    e = e + (safe > FP8_MAX * torch.exp2(e)).double() - (safe <= FP8_MAX * torch.exp2(e - 1)).double()
    e = torch.where(nz, e, torch.zeros_like(e)).clamp(E_MIN, E_MAX)
    scaled = wf * torch.exp2(-e).float()[:, None]          # exact: a power-of-two scale of a normal value
    assert float(scaled.abs().max()) <= FP8_MAX if scaled.numel() else True
    q = scaled.to(torch.float8_e4m3fn).view(torch.uint8)     # in range: round to nearest even, never the cast's out-of-range NaN
    return q, e.to(torch.int8)


def dequantize_fp8_rows(q: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    """(q uint8 [N, K], e int8 [N]) -> W_deq = q * 2^e, bf16 [N, K] (exact)."""
    return (q.view(torch.float8_e4m3fn).float() * torch.exp2(e.float())[:, None]).to(torch.bfloat16)


def wp8_bytes(N: int, K: int) -> int:
    kb2 = (K // 32 + 1) // 2
    return -(-N // 16) * kb2 * 64 * 16


def pack_wp8(q: torch.Tensor, e: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """WP8 blocks of one weight: packed[((nb*KB2 + i)*64 + lane)*16 + j] = q[nb*16 + (lane&15)][(lane>>4)*(K/4) + 16*i + j]
    (zero past a K quarter and in padded rows) and exps[nb*16 + r] (0 for padded rows).  -> (uint8 [NB*KB2*1024], int8 [NB*16])."""
    N, K = q.shape
    if K % 32:
        raise ValueError(f"pack_wp8: K must be a multiple of 32 (got {K})")
    KB2, Q, NB = (K // 32 + 1) // 2, K // 4, -(-N // 16)
    qq = torch.zeros(NB * 16, 4, KB2 * 16, dtype=torch.uint8, device=q.device)
    qq[:N, :, :Q] = q.reshape(N, 4, Q)
    packed = qq.view(NB, 16, 4, KB2, 16).permute(0, 3, 2, 1, 4).contiguous().view(-1)     # (nb, i, h, r, j): lane = 16 h + r
    ex = torch.zeros(NB * 16, dtype=torch.int8, device=q.device)
    ex[:N] = e
    return packed, ex


def pack_wp8_gate_up(qg, eg, qu, eu) -> Tuple[torch.Tensor, torch.Tensor]:
    """gate / up of one SwiGLU expert, blocks interleaved as umoe_pack_gate_up (block 2i = gate i, 2i+1 = up i)."""
    if qg.shape != qu.shape or qg.shape[0] % 16:
        raise ValueError(f"pack_wp8_gate_up: gate {tuple(qg.shape)} / up {tuple(qu.shape)} (rows a multiple of 16)")
    pg, xg = pack_wp8(qg, eg)
    pu, xu = pack_wp8(qu, eu)
    NB = qg.shape[0] // 16
    return (torch.stack([pg.view(NB, -1), pu.view(NB, -1)], 1).reshape(-1),
            torch.stack([xg.view(NB, 16), xu.view(NB, 16)], 1).reshape(-1))


def unpack_wp8(packed: torch.Tensor, ex: torch.Tensor, N: int, K: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Inverse of pack_wp8: (q uint8 [N, K], e int8 [N])."""
    KB2, Q, NB = (K // 32 + 1) // 2, K // 4, -(-N // 16)
    qq = packed.view(NB, KB2, 4, 16, 16).permute(0, 3, 2, 1, 4).reshape(NB * 16, 4, KB2 * 16)
    return qq[:N, :, :Q].reshape(N, K).contiguous(), ex[:N].clone()


_PROJ = ("gate_proj", "up_proj", "down_proj")


def expert_modules(layer):
    """(routed experts, shared experts) of one decoder layer: the modules with gate_proj / up_proj / down_proj."""
    return list(layer.mlp.dynamic_real_moe.deepspeed_moe.experts.deepspeed_experts), list(layer.mlp.fixed_real_moe)


def _released_msg(what: str) -> str:
    return (f"{what}: this model holds its expert weights as fp8 only (quantize_experts_(keep_bf16=False) released the bf16 parameters); "
            "the decode engine runs on them (expert_weights='fp8-only') -- call unimoe_audio_amd.quant.dequantize_experts_(model) to get "
            "the bf16 parameters back (exact: W_deq)")


def _refuse_state_dict(module, prefix, keep_vars):
    from . import _lib as L
    raise L.UmoeError(_released_msg(f"state_dict of {prefix or 'an expert'}"))


def _release(m):
    """Drops the three bf16 parameters of a quantized expert module (the WP8 copy stays) and makes saving it an error."""
    for name in _PROJ:
        p = getattr(m, name).weight
        p.data = torch.empty(0, dtype=p.dtype, device=p.device)
    m._fp8["released"] = True
    if m._fp8.get("hook") is None:
        m._fp8["hook"] = m.register_state_dict_pre_hook(_refuse_state_dict)


def is_released(m) -> bool:
    """True for an expert module (or a DCMoE block / a model holding one) whose bf16 parameters were released."""
    st = getattr(m, "_fp8", None)
    if st is not None:
        return bool(st.get("released"))
    return any(bool(getattr(x, "_fp8", None) and x._fp8.get("released")) for x in m.modules())


@torch.no_grad()
def quantize_expert_(m, keep_bf16: bool = True):
    """One expert module (gate_proj / up_proj / down_proj): the e4m3 copy in WP8 layout on `m._fp8`; the parameters become W_deq, or,
    with keep_bf16=False, are released as soon as the copy exists."""
    if is_released(m):
        if keep_bf16:
            from . import _lib as L
            raise L.UmoeError(_released_msg("quantize_experts_(keep_bf16=True)"))
        return m
    qe, ver = {}, {}
    for name in _PROJ:
        p = getattr(m, name).weight
        q, e = quantize_fp8_rows(p)
        if keep_bf16:
            p.copy_(dequantize_fp8_rows(q, e).to(p.dtype))
        qe[name] = (q.to(p.device), e.to(p.device))
        ver[name] = (p._version, p.data_ptr())
    m._fp8 = dict(gu=pack_wp8_gate_up(*qe["gate_proj"], *qe["up_proj"]), dn=pack_wp8(*qe["down_proj"]), ver=ver,
                  shape={n: tuple(getattr(m, n).weight.shape) for n in _PROJ}, released=False, hook=None)
    if not keep_bf16:
        _release(m)
    return m


@torch.no_grad()
def quantize_experts_(model, fmt: str = "fp8", keep_bf16: bool = True):
    """Quantizes the gate / up / down weights of the routed AND shared experts of every layer in place: each parameter becomes W_deq.
    The e4m3 copies are kept on the expert module ONCE, already in the engine's WP8 layout (`_fp8["gu"]` gate/up interleaved, `_fp8["dn"]`:
    (packed, exponents)), with every parameter's version (a later change is detected by check_quantized).  Router gate, attention, codec
    head and embeddings stay bf16.  Idempotent.
    keep_bf16=False: each expert's three parameters are released as soon as its WP8 copy exists (the peak is ONE expert's bf16) and
    model._expert_weights becomes "fp8-only": the decode engine runs on the WP8 copies alone, everything else that needs the bf16
    parameters raises (dequantize_experts_ restores them)."""
    if fmt != "fp8":
        raise ValueError(f"quantize_experts_: unknown format {fmt!r} (only 'fp8')")
    for layer in model.language_model.layers:
        routed, shared = expert_modules(layer)
        for m in routed + shared:
            quantize_expert_(m, keep_bf16)
    model._expert_weights = "fp8" if keep_bf16 else "fp8-only"
    if not keep_bf16:
        _drop_packs(model)
    return model


def _drop_packs(model):
    """The WP16 packs (model.packed(), each block's prepare()) and an engine built on them hold the bytes the release is about."""
    from .checkpoint import invalidate_packed
    invalidate_packed(model)


@torch.no_grad()
def dequantize_experts_(model):
    """Restores W_deq = q * 2^e into every expert parameter from its WP8 copy (exact), released or not: an fp8-only model becomes the
    model quantize_experts_(keep_bf16=True) leaves -- forward, training, saving and bf16 / fp8 engines work again."""
    for layer in model.language_model.layers:
        routed, shared = expert_modules(layer)
        for m in routed + shared:
            st = getattr(m, "_fp8", None)
            if st is None:
                from . import _lib as L
                raise L.UmoeError("dequantize_experts_: an expert has no fp8 weights (quantize_experts_ first)")
            for name in _PROJ:
                p = getattr(m, name).weight
                q, e = expert_qe(m, name)
                w = dequantize_fp8_rows(q, e).to(device=p.device, dtype=p.dtype)
                if tuple(p.shape) == tuple(w.shape):
                    p.copy_(w)
                else:
                    p.data = w.contiguous()
                st["ver"][name] = (p._version, p.data_ptr())
            st["released"] = False
            if st.get("hook") is not None:
                st["hook"].remove()
                st["hook"] = None
    model._expert_weights = "fp8"
    _drop_packs(model)
    return model


def expert_qe(m, name: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """(q, e) of one projection of a quantized expert module, unpacked from its WP8 copy."""
    st = m._fp8
    N, K = st["shape"][name]
    if name == "down_proj":
        return unpack_wp8(*st["dn"], N, K)
    packed, ex = st["gu"]
    NB = N // 16
    half = 1 if name == "up_proj" else 0
    return unpack_wp8(packed.view(NB, 2, -1)[:, half].reshape(-1), ex.view(NB, 2, 16)[:, half].reshape(-1), N, K)


def expert_format(model) -> str:
    """"bf16", "fp8" (quantized, bf16 parameters kept as W_deq) or "fp8-only" (quantized, bf16 parameters released)."""
    return getattr(model, "_expert_weights", "bf16")


def is_quantized(model) -> bool:
    return expert_format(model) in ("fp8", "fp8-only")


def check_quantized(model):
    """Raises UmoeError when an expert weight changed after quantize_experts_ (a training step, load_state_dict, ...): its fp8 copy
    would be stale."""
    from . import _lib as L
    for li, layer in enumerate(model.language_model.layers):
        routed, shared = expert_modules(layer)
        for xi, m in enumerate(routed + shared):
            store = getattr(m, "_fp8", None)
            if store is None:
                raise L.UmoeError(f"layer {li} expert {xi} has no fp8 weights: call quantize_experts_('fp8')")
            if store.get("released"):
                continue               # no bf16 parameter that could differ from the fp8 copy
            for name in _PROJ:
                p = getattr(m, name).weight
                ver, ptr = store["ver"][name]
                if p._version == ver and p.data_ptr() == ptr:
                    continue
                # moved (model.to) or written: still W_deq?
                q, e = expert_qe(m, name)
                if torch.equal(p.detach(), dequantize_fp8_rows(q.to(p.device), e.to(p.device)).to(p.dtype)):
                    store["ver"][name] = (p._version, p.data_ptr())
                else:
                    raise L.UmoeError(f"layer {li} expert {xi} {name}: the weight changed after quantize_experts_('fp8') -- its fp8 copy is "
                                      "stale; quantize again")
