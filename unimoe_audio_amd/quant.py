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

w12-only (quantize_experts_("w12", keep_bf16=False)): the same release for the LOSSLESS 12-bit copies (w12.py) that bf16 engines
already decode from.  Each expert's WP12 copies are built from its parameters (`_w12` on the module) and the parameters released; an engine
built on such a model holds the WP12 copies and nothing else (prefill: umoe_tiled_gemm_w12).  No bit of any result changes, and
dequantize_experts_ restores the parameters bit for bit.  A layer with a matrix that is not packable keeps its parameters.

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


def _released_msg(what: str, w12: bool = False) -> str:
    if w12:
        return (f"{what}: this model holds its expert weights as the lossless 12-bit copies only (quantize_experts_('w12', keep_bf16=False) "
                "released the bf16 parameters); the decode engine runs on them (expert_weights='w12-only') -- call "
                "unimoe_audio_amd.quant.dequantize_experts_(model) to get the bf16 parameters back (bit for bit)")
    return (f"{what}: this model holds its expert weights as fp8 only (quantize_experts_(keep_bf16=False) released the bf16 parameters); "
            "the decode engine runs on them (expert_weights='fp8-only') -- call unimoe_audio_amd.quant.dequantize_experts_(model) to get "
            "the bf16 parameters back (exact: W_deq)")


def _refuse_state_dict(module, prefix, keep_vars):
    from . import _lib as L
    raise L.UmoeError(_released_msg(f"state_dict of {prefix or 'an expert'}", hasattr(module, "_w12")))


def released_w12(m) -> bool:
    """True for a module (or anything holding one) whose expert parameters were released in favour of their WP12 copies."""
    return any(bool(getattr(x, "_w12", None) and x._w12.get("released")) for x in m.modules())


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
    for attr in ("_fp8", "_w12"):
        st = getattr(m, attr, None)
        if st is not None:
            return bool(st.get("released"))
    return any(bool(getattr(x, a, None) and getattr(x, a).get("released")) for x in m.modules() for a in ("_fp8", "_w12"))


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
    if fmt == "w12":
        return _w12_experts_(model, keep_bf16)
    if fmt != "fp8":
        raise ValueError(f"quantize_experts_: unknown format {fmt!r} ('fp8' or 'w12')")
    if expert_format(model) == "w12-only":
        from . import _lib as L
        raise L.UmoeError(_released_msg("quantize_experts_('fp8')", True))
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
    if expert_format(model) == "w12-only" or any(hasattr(x, "_w12") for x in model.modules()):
        for layer in model.language_model.layers:
            _w12_restore_layer(layer)
        model._expert_weights = "bf16"
        _drop_packs(model)
        return model
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
    """"bf16", "fp8" (quantized, bf16 parameters kept as W_deq), "fp8-only" (quantized, bf16 parameters released) or "w12-only" (bf16
    parameters released in favour of their lossless WP12 copies)."""
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


# ------------------------------------------------------------------------------------------------ w12-only
@torch.no_grad()
def w12_expert_(m) -> bool:
    """One expert module: its WP12 copies (gate/up interleaved in WP16 order, down) on `m._w12`, the three parameters released as soon as
    the copies exist.  False, and the module untouched, when one of its matrices is not packable (a block over the exception cap)."""
    from . import w12
    if getattr(m, "_w12", None) is not None and m._w12.get("released"):
        return True
    wg, wu, wd = (getattr(m, n).weight.detach() for n in _PROJ)
    I, D = wg.shape
    if wg.dtype != torch.bfloat16 or I % 16 or D % 32 or I % 32 or D // 32 >= 127 or I // 32 >= 127:
        return False
    # On a device the copies get their storage FIRST, at their exact sizes and from an empty cache: served from the blocks that the
    # packer's temporaries and the released parameters leave behind, each would carry an unsplit remainder of up to 1 MiB that nothing
    # else can use.  The parameters' blocks go back to the driver as soon as they are released.
    cuda = wg.is_cuda
    if cuda:
        torch.cuda.empty_cache()
        NBg, NBd = 2 * I // 16, D // 16
        room = [(torch.empty(NBg * w12.block_bytes(D // 32), dtype=torch.uint8, device=wg.device),
                 torch.empty(NBg * w12.META, dtype=torch.int32, device=wg.device)),
                (torch.empty(NBd * w12.block_bytes(I // 32), dtype=torch.uint8, device=wg.device),
                 torch.empty(NBd * w12.META, dtype=torch.int32, device=wg.device))]
    gu = w12.pack(w12.wp16_gate_up(wg.contiguous(), wu.contiguous()), D // 32)
    dn = w12.pack(w12.wp16_from_rows(wd.contiguous()), I // 32) if gu is not None else None
    if gu is None or dn is None:
        return False
    if cuda:
        for dst, src in zip(room, (gu, dn)):
            dst[0].copy_(src[0]), dst[1].copy_(src[1])
        gu, dn = room
    m._w12 = dict(gu=gu, dn=dn, shape={n: tuple(getattr(m, n).weight.shape) for n in _PROJ}, released=True, hook=None)
    for name in _PROJ:
        p = getattr(m, name).weight
        p.data = torch.empty(0, dtype=p.dtype, device=p.device)
    m._w12["hook"] = m.register_state_dict_pre_hook(_refuse_state_dict)
    if cuda:
        del wg, wu, wd
        torch.cuda.empty_cache()
    return True


@torch.no_grad()
def w12_restore_expert_(m):
    """The three parameters of a released expert module back from its WP12 copies, bit for bit; the copies are dropped."""
    from . import w12
    st = getattr(m, "_w12", None)
    if st is None:
        return m
    (I, D) = st["shape"]["gate_proj"]
    both = w12.rows_from_wp16(w12.unpack(st["gu"][0], st["gu"][1], D // 32), 2 * I, D).view(I // 16, 2, 16, D)      # (the inverse of wp16_gate_up)
    vals = dict(gate_proj=both[:, 0].reshape(I, D), up_proj=both[:, 1].reshape(I, D),
                down_proj=w12.rows_from_wp16(w12.unpack(st["dn"][0], st["dn"][1], I // 32), D, I))
    for name in _PROJ:
        p = getattr(m, name).weight
        p.data = vals[name].to(device=p.device, dtype=p.dtype).contiguous()
    if st.get("hook") is not None:
        st["hook"].remove()
    del m._w12
    m.__dict__.pop("_unallocated", None)
    return m


def _w12_restore_layer(layer):
    routed, shared = expert_modules(layer)
    for m in routed + shared:
        w12_restore_expert_(m)


def w12_settle_layers_(model):
    """A layer is w12-only as a whole or not at all (the engine's layers are): where one expert of a layer kept its parameters (not
    packable), the layer's released experts get theirs back."""
    for layer in model.language_model.layers:
        routed, shared = expert_modules(layer)
        if any(getattr(m, "_w12", None) is None for m in routed + shared):
            _w12_restore_layer(layer)


@torch.no_grad()
def _w12_experts_(model, keep_bf16: bool):
    from . import _lib as L
    if keep_bf16:
        raise L.UmoeError("quantize_experts_('w12', keep_bf16=True): nothing to do -- bf16 engines already stream the lossless WP12 copies of "
                          "the expert weights (DESIGN 4k, 4l); keep_bf16=False releases the bf16 parameters in their favour ('w12-only')")
    if expert_format(model) in ("fp8", "fp8-only"):
        raise L.UmoeError(f"quantize_experts_('w12'): this model's experts are {expert_format(model)!r}; dequantize_experts_ first")
    for layer in model.language_model.layers:
        routed, shared = expert_modules(layer)
        if all(getattr(m, "_w12", None) is not None for m in routed + shared):
            continue                      # idempotent
        for m in routed + shared:         # (each expert released as soon as its copies exist: the peak is one expert's bf16)
            if not w12_expert_(m):
                _w12_restore_layer(layer)     # not packable: the whole layer stays as it was
                break
    model._expert_weights = "w12-only"
    _drop_packs(model)
    return model


def w12_layer_copies(layer, device=None):
    """dict(gu=[(blocks, records)], dn=[...]) over the routed, then the shared experts of a released layer (None: the layer kept its
    parameters).  The copies live in a plain dict on the expert module, which nn.Module.to() does not move: with `device` a copy that
    is elsewhere (a model released on the host, then moved) is moved there first, once, in the module's own store."""
    routed, shared = expert_modules(layer)
    mods = routed + shared
    if not mods or any(getattr(m, "_w12", None) is None for m in mods):
        return None
    if device is not None:
        device = torch.device(device)
        for m in mods:
            for k in ("gu", "dn"):
                if any(t.device != device for t in m._w12[k]):
                    m._w12[k] = tuple(t.to(device) for t in m._w12[k])
    return dict(gu=[m._w12["gu"] for m in mods], dn=[m._w12["dn"] for m in mods])
