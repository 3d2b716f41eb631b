"""AdamW with fp32 master weights and global-norm clipping on the HIP kernels of csrc/umoe_optim.hip (include/umoe.h "optimizer step").

The model's parameters are bf16 because the kernels read bf16 weights as stored; an update of 1e-5 on bf16 weights of size 0.03 is lost on
nine weights in ten.  The reference trains under DeepSpeed's bf16 mode (AdamW on fp32 master weights, gradient clipping:
UniMoEV2-Preview/deepspeed_zero2.conf, script/training.sh:61-72, moe_trainer.py:691-703); this is that step for one device: every
tensor of every parameter group goes through one chunked launch per stage --

    stage 1  sum of squared gradients per chunk (fixed order, no atomics)          2 bytes per bf16 parameter
    stage 2  norm, clip coefficient, bias corrections, skip flag (one workgroup)
    stage 3  the update: master, m, v read and written, gradient read, parameter written        28 bytes per bf16 parameter

-- enqueued on the current stream without a host sync.  A step whose gradients hold inf / NaN is skipped on the device (nothing is
written, `skipped_steps` advances, `steps` does not).  The arithmetic is torch.optim.AdamW (decoupled decay, no amsgrad) behind
torch.nn.utils.clip_grad_norm_; amsgrad / maximize / capturable are not offered.

Expert parallel (ep_size > 1): the norm of stage 1 / 2 is the local rank's.  Pass max_grad_norm=None and reduce / clip outside.

No CPU fallback: CPU tensors raise.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, Optional, Sequence

import numpy as np
import torch

from . import _lib as L

MAX_GROUPS = 16            # UMOE_OPTIM_MAX_GROUPS
CHUNK_ELEMS = 16384        # elements a workgroup owns at a time: 8 iterations of 256 threads x 8 elements
# the records of include/umoe.h (tests/test_optim_cpu.py compares them with the header through a compiled probe)
TENSOR_DTYPE = np.dtype([("p", "<u8"), ("g", "<u8"), ("master", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i8"), ("group", "<i4"),
                         ("p_fp32", "<i4")], align=True)
# p_fp32 is a flag word: bit 0 the parameter is fp32 (its own master), bit 1 the gradient is fp32 (an fp32 main gradient of a bf16 parameter)
P_FP32, G_FP32 = 1, 2
FOLD_DTYPE = np.dtype([("g", "<u8"), ("main", "<u8"), ("n", "<i8")], align=True)      # umoe_optim_fold_tensor
CHUNK_DTYPE = np.dtype([("tensor", "<i8"), ("first", "<i8")], align=True)
RECORD_DTYPE = np.dtype([("norm", "<f4"), ("clip", "<f4"), ("skip", "<i4"), ("reserved", "<i4"), ("bc1", "<f4", (MAX_GROUPS,)),
                         ("bc2", "<f4", (MAX_GROUPS,))], align=True)
RECORD_WORDS = RECORD_DTYPE.itemsize // 4


class OptimHyper(C.Structure):
    """umoe_optim_hyper: per-group settings, read by the library at every call"""
    _fields_ = [("num_groups", C.c_int32), ("reserved", C.c_int32), ("max_norm", C.c_double)] + \
               [(n, C.c_double * MAX_GROUPS) for n in ("lr", "beta1", "beta2", "eps", "wd")]


def build_chunk_table(sizes: Sequence[int], chunk_elems: int = CHUNK_ELEMS) -> np.ndarray:
    """(tensor index, first element) of every chunk, tensors in order: tensor i of sizes[i] elements gets ceil(sizes[i] / chunk_elems)
    chunks starting at multiples of chunk_elems, so every element is covered once and no chunk crosses a tensor; an empty tensor gets
    none.  -> CHUNK_DTYPE [n_chunks]."""
    if chunk_elems <= 0 or chunk_elems % 8:
        raise ValueError(f"chunk_elems must be a positive multiple of 8 (got {chunk_elems})")
    sizes = np.asarray(list(sizes), dtype=np.int64)
    if (sizes < 0).any():
        raise ValueError("negative tensor size")
    counts = -(-sizes // chunk_elems)
    table = np.zeros(int(counts.sum()), dtype=CHUNK_DTYPE)
    table["tensor"] = np.repeat(np.arange(len(sizes), dtype=np.int64), counts)
    starts = np.cumsum(counts) - counts
    table["first"] = (np.arange(len(table), dtype=np.int64) - np.repeat(starts, counts)) * chunk_elems
    return table


def make_hyper(groups: Sequence[dict], max_grad_norm: Optional[float]) -> OptimHyper:
    """param_groups (lr, betas, eps, weight_decay) -> umoe_optim_hyper"""
    if not 1 <= len(groups) <= MAX_GROUPS:
        raise L.UmoeError(f"AdamW: {len(groups)} parameter groups (1..{MAX_GROUPS}: the settings travel by value in the kernel argument)")
    h = OptimHyper(num_groups=len(groups), max_norm=-1.0 if max_grad_norm is None else float(max_grad_norm))
    for i, g in enumerate(groups):
        h.lr[i], h.beta1[i], h.beta2[i], h.eps[i], h.wd[i] = float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), \
            float(g["weight_decay"])
    return h


def _head(ptr: int, esize: int) -> int:
    """elements in front of the first 16-byte boundary (what umoe_optim.hip's head_of computes)"""
    return ((-ptr) & 15) // esize


def main_grad_offsets(ptrs_and_sizes) -> tuple:
    """where each tensor's run starts in one flat fp32 buffer, by the rule of AdamW._allocate: 4-element (16-byte) slots, shifted so that the
    run is 16-byte aligned after as many elements as its bf16 parameter (a view at an odd element offset keeps its vectors).
    ptrs_and_sizes: (data_ptr, element_size, numel) per parameter -> (offsets, total elements)"""
    offs, cur = [], 0
    for ptr, esize, n in ptrs_and_sizes:
        h = _head(ptr, esize) % 4
        o = -(-cur // 4) * 4 + (-h) % 4
        offs.append(o)
        cur = o + n
    return offs, cur


def _check_main_grad(mg, p: torch.Tensor, i: int):
    if not isinstance(mg, torch.Tensor) or mg.dtype != torch.float32:
        raise L.UmoeError(f"AdamW: main_grad of parameter {i} is {getattr(mg, 'dtype', type(mg).__name__)}; a main gradient is fp32")
    if mg.shape != p.shape or not mg.is_contiguous():
        raise L.UmoeError(f"AdamW: main_grad of parameter {i} has shape {tuple(mg.shape)} (strides {mg.stride()}), the parameter {tuple(p.shape)}")
    if not mg.is_cuda or mg.device != p.device:
        raise L.UmoeError(f"AdamW: main_grad of parameter {i} is on {mg.device}, the parameter on {p.device}; there is no CPU fallback")


def _check_param(p: torch.Tensor, name: str):
    if not isinstance(p, torch.Tensor):
        raise TypeError(f"AdamW: {name} is a {type(p).__name__}, not a tensor")
    if p.numel() == 0 and (hasattr(p, "allreduce") or hasattr(p, "group_name")):
        raise L.UmoeError(f"AdamW: {name} is a released expert parameter (expert_weights 'fp8-only' / 'w12-only'): inference only: "
                          "`quant.dequantize_experts_` first")
    if p.dtype not in (torch.bfloat16, torch.float32):
        raise L.UmoeError(f"AdamW: {name} is {p.dtype}; parameters are bf16 (fp32 master weights are kept here) or fp32")
    if not p.is_cuda:
        raise L.UmoeError(f"AdamW: {name} is a CPU tensor; there is no CPU fallback")
    if not p.is_contiguous():
        raise L.UmoeError(f"AdamW: {name} is not contiguous (shape {tuple(p.shape)}, strides {p.stride()})")


class AdamW(torch.optim.Optimizer):
    """AdamW(params_or_groups, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None, check_finite=True)

    params_or_groups: parameters or torch-style groups (train.moe_param_groups); a group may carry its own lr / betas / eps /
    weight_decay, read at every step, so torch LR schedulers work.  At most 16 groups.
    max_grad_norm: clip the global 2-norm of all gradients to it (clip_grad_norm_'s rule); None: off.
    check_finite: skip the step on the device when a gradient is inf / NaN.  With max_grad_norm=None and check_finite=False only the
    update kernel is enqueued (no norm pass; `grad_norm` stays NaN and the step counter is kept on the host as well).

    bf16 parameters get fp32 master weights, allocated with m and v on the first step() as three flat buffers (12 bytes per bf16
    parameter); an fp32 parameter is its own master.  `grad_norm` (fp32), `steps` and `skipped_steps` (int64) are device tensors:
    reading them is the caller's sync.  A parameter whose .grad is None is left out of that step.

    A parameter that carries an fp32 `main_grad` (train.attach_main_grads) is updated from it: the gradient arrives without a bf16
    rounding, `.grad` is ignored for that parameter (it must be None or all zero after MainGrads.fold()), and zero_grad() zeroes the
    main gradients as well."""

    def __init__(self, params, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 max_grad_norm: Optional[float] = None, check_finite: bool = True, chunk_elems: int = CHUNK_ELEMS):
        if isinstance(params, torch.nn.Module):
            raise TypeError("AdamW: pass model.parameters() or parameter groups (train.moe_param_groups(model)), not the module")
        if not (isinstance(lr, (int, float)) and lr >= 0.0):
            raise ValueError(f"AdamW: lr {lr!r}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"AdamW: betas {betas!r}")
        if eps < 0.0 or weight_decay < 0.0 or (max_grad_norm is not None and not max_grad_norm >= 0.0):
            raise ValueError(f"AdamW: eps {eps!r}, weight_decay {weight_decay!r}, max_grad_norm {max_grad_norm!r}")
        if chunk_elems <= 0 or chunk_elems % 8:
            raise ValueError(f"AdamW: chunk_elems must be a positive multiple of 8 (got {chunk_elems})")
        super().__init__(params, dict(lr=float(lr), betas=tuple(betas), eps=float(eps), weight_decay=float(weight_decay)))
        self.param_groups = [g for g in self.param_groups if g["params"]] or self.param_groups[:1]      # a group without parameters needs no slot
        self.max_grad_norm = max_grad_norm
        self.check_finite = bool(check_finite)
        self.chunk_elems = int(chunk_elems)
        make_hyper(self.param_groups, max_grad_norm)                                      # refuses more than 16 groups
        self._params = [(gi, p) for gi, g in enumerate(self.param_groups) for p in g["params"]]
        for i, (gi, p) in enumerate(self._params):
            _check_param(p, f"parameter {i} (group {gi}, shape {tuple(p.shape)})")
        devs = {p.device for _, p in self._params}
        if len(devs) > 1:
            raise L.UmoeError(f"AdamW: parameters on several devices {sorted(map(str, devs))}")
        self._dev = next(iter(devs)) if devs else None
        self._flat = None                 # master, m, v flat fp32 buffers
        self._key = None                  # the (p, grad) pointers the device tensor table was packed from
        self._host_t = 0                  # the step counter as the host knows it (exact when nothing can be skipped)
        self._uploaded = None
        self._counters = None             # [steps, skipped_steps] on the device

    # ------------------------------------------------------------------------------------------------------------ state
    @property
    def _uses_record(self) -> bool:
        return self.max_grad_norm is not None or self.check_finite

    def _allocate(self):
        """master / m / v as three flat fp32 buffers; each tensor's run starts where it is 16-byte aligned after as many elements as
        its parameter, so the update kernel's vectors line up across the streams of a tensor"""
        dev = self._dev
        offs, cur_s, cur_w = [], 0, 0
        for _, p in self._params:
            h = _head(p.data_ptr(), p.element_size()) % 4
            o_s = -(-cur_s // 4) * 4 + (-h) % 4
            cur_s = o_s + p.numel()
            o_w = None
            if p.dtype == torch.bfloat16:
                o_w = -(-cur_w // 4) * 4 + (-h) % 4
                cur_w = o_w + p.numel()
            offs.append((o_s, o_w))
        self._flat = dict(master=torch.empty(cur_w, dtype=torch.float32, device=dev), m=torch.zeros(cur_s, dtype=torch.float32, device=dev),
                          v=torch.zeros(cur_s, dtype=torch.float32, device=dev))
        for (_, p), (o_s, o_w) in zip(self._params, offs):
            st = self.state[p]
            n = p.numel()
            st["exp_avg"] = self._flat["m"][o_s:o_s + n].view(p.shape)
            st["exp_avg_sq"] = self._flat["v"][o_s:o_s + n].view(p.shape)
            if o_w is not None:
                st["master"] = self._flat["master"][o_w:o_w + n].view(p.shape)
                st["master"].copy_(p.detach())
        self._chunks_host = build_chunk_table([p.numel() for _, p in self._params], self.chunk_elems)
        n_chunks = len(self._chunks_host)
        self._chunks = torch.from_numpy(self._chunks_host.view(np.int64).reshape(-1, 2).copy()).to(dev)
        self._tensors_host = np.zeros(max(len(self._params), 1), dtype=TENSOR_DTYPE)
        self._staging = torch.empty(self._tensors_host.nbytes, dtype=torch.uint8).pin_memory()
        self._tensors = torch.zeros(self._tensors_host.nbytes, dtype=torch.uint8, device=dev)
        self._uploaded = torch.cuda.Event()
        self._partial = torch.zeros(max(n_chunks, 1), dtype=torch.float32, device=dev)
        self._flags = torch.zeros(max(n_chunks, 1), dtype=torch.int32, device=dev)
        self._rec = torch.zeros(RECORD_WORDS, dtype=torch.float32, device=dev)
        if not self._uses_record:
            self._rec[0] = float("nan")
        if self._counters is None:
            self._counters = torch.zeros(2, dtype=torch.int64, device=dev)

    def state_bytes(self) -> int:
        """bytes of master + m + v (0 before the first step)"""
        return 0 if self._flat is None else sum(t.numel() * 4 for t in self._flat.values())

    @property
    def grad_norm(self) -> torch.Tensor:
        """global 2-norm of the gradients of the last step() before clipping (device, fp32)"""
        self._need_state()
        return self._rec[0]

    @property
    def steps(self) -> torch.Tensor:
        self._need_state()
        return self._counters[0]

    @property
    def skipped_steps(self) -> torch.Tensor:
        self._need_state()
        return self._counters[1]

    def _need_state(self):
        if self._flat is None:
            if self._dev is None:
                raise L.UmoeError("AdamW: no parameters")
            self._allocate()

    # ------------------------------------------------------------------------------------------------------------- step
    def _sync_table(self) -> bool:
        """re-packs and uploads the tensor table when some p / grad / main-grad pointer changed; True when it did"""
        key = []
        for i, (gi, p) in enumerate(self._params):
            mg = getattr(p, "main_grad", None)
            if mg is not None:
                _check_main_grad(mg, p, i)
                key.append((p.data_ptr(), mg.data_ptr(), mg.data_ptr()))
                continue
            g = p.grad
            if g is not None:
                if g.dtype != p.dtype:
                    raise L.UmoeError(f"AdamW: the gradient of parameter {i} is {g.dtype}, the parameter {p.dtype}")
                if not g.is_cuda or g.device != p.device:
                    raise L.UmoeError(f"AdamW: the gradient of parameter {i} is on {g.device}; there is no CPU fallback")
                if not g.is_contiguous() or g.shape != p.shape:
                    raise L.UmoeError(f"AdamW: the gradient of parameter {i} is not contiguous (shape {tuple(g.shape)}, strides {g.stride()})")
            key.append((p.data_ptr(), 0 if g is None else g.data_ptr(), 0))
        key = tuple(key)
        if key == self._key:
            return False
        t = self._tensors_host
        for i, ((gi, p), (pp, gp, mp)) in enumerate(zip(self._params, key)):
            st = self.state[p]
            if not p.is_contiguous():
                raise L.UmoeError(f"AdamW: parameter {i} is no longer contiguous")
            t[i] = (pp, gp, st["master"].data_ptr() if "master" in st else 0, st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel(), gi,
                    (P_FP32 if p.dtype == torch.float32 else 0) | (G_FP32 if mp else 0))
        self._uploaded.synchronize()              # the previous upload (if any) has read the staging buffer
        self._staging.numpy()[:] = t.view(np.uint8).reshape(-1)
        self._tensors.copy_(self._staging, non_blocking=True)
        self._uploaded.record()
        self._key = key
        return True

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        has_grad = lambda p: p.grad is not None or getattr(p, "main_grad", None) is not None      # noqa: E731
        if not any(has_grad(p) for _, p in self._params):      # nothing to update: no step is counted, as in torch
            return loss
        self._need_state()
        hyper = make_hyper(self.param_groups, self.max_grad_norm)
        fresh = self._sync_table()
        n_chunks = len(self._chunks_host)
        if n_chunks == 0:
            return loss
        lib, stream = L.lib(), C.c_void_p(torch.cuda.current_stream(self._dev).cuda_stream)
        # the host copies are handed over with a freshly packed table only: the library checks every record of them before it enqueues
        ht = self._tensors_host.ctypes.data if fresh else None
        hc = self._chunks_host.ctypes.data if fresh else None
        nt = len(self._params)
        if self._uses_record:
            L.check(lib.umoe_optim_sqsum(self._tensors.data_ptr(), nt, self._chunks.data_ptr(), n_chunks, self.chunk_elems, ht, hc, hyper.num_groups,
                                         0, self._partial.data_ptr(), self._flags.data_ptr(), stream), "umoe_optim_sqsum")
            L.check(lib.umoe_optim_scalars(self._partial.data_ptr(), self._flags.data_ptr(), n_chunks, C.byref(hyper), self._counters.data_ptr(),
                                           self._rec.data_ptr(), stream), "umoe_optim_scalars")
            L.check(lib.umoe_optim_adamw(self._tensors.data_ptr(), nt, self._chunks.data_ptr(), n_chunks, self.chunk_elems, ht, hc, 0,
                                         C.byref(hyper), self._rec.data_ptr(), -1, self._counters.data_ptr(), stream), "umoe_optim_adamw")
        else:
            L.check(lib.umoe_optim_adamw(self._tensors.data_ptr(), nt, self._chunks.data_ptr(), n_chunks, self.chunk_elems, ht, hc, 0,
                                         C.byref(hyper), None, self._host_t, self._counters.data_ptr(), stream), "umoe_optim_adamw")
        self._host_t += 1
        # every pack cache of the package is keyed on (data_ptr, _version): the kernels wrote behind autograd's back
        torch.autograd.graph.increment_version([p for _, p in self._params if has_grad(p)])
        return loss

    @torch.no_grad()
    def zero_grad(self, set_to_none: bool = True):
        """torch's zero_grad, and the fp32 main gradients zeroed as well: one zero_() per flat buffer they are views of"""
        super().zero_grad(set_to_none=set_to_none)
        seen = {}
        for _, p in self._params:
            mg = getattr(p, "main_grad", None)
            if mg is not None:
                base = mg._base if mg._base is not None else mg
                seen[id(base)] = base
        for base in seen.values():
            base.zero_()

    # ------------------------------------------------------------------------------------------------------ checkpointing
    def state_dict(self):
        """torch's layout ("state" by parameter index, "param_groups") with master / exp_avg / exp_avg_sq as tensors of their own, plus
        "counters" = [steps, skipped_steps]"""
        sd = super().state_dict()
        sd["state"] = {k: {n: (t.detach().clone() if isinstance(t, torch.Tensor) else t) for n, t in st.items()} for k, st in sd["state"].items()}
        sd["counters"] = None if self._counters is None else self._counters.detach().clone()
        return sd

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """restores master, m, v and the counters bit for bit, the groups' settings, and re-derives every bf16 parameter from its master"""
        groups = state_dict["param_groups"]
        if len(groups) != len(self.param_groups) or any(len(a["params"]) != len(b["params"]) for a, b in zip(groups, self.param_groups)):
            raise ValueError("AdamW.load_state_dict: the parameter groups differ from the saved ones")
        for saved, own in zip(groups, self.param_groups):
            own.update({k: v for k, v in saved.items() if k != "params"})
        make_hyper(self.param_groups, self.max_grad_norm)
        if state_dict["state"]:
            self._need_state()
            for idx, (_, p) in enumerate(self._params):
                saved = state_dict["state"].get(idx)
                if saved is None:
                    continue
                st = self.state[p]
                for name in ("exp_avg", "exp_avg_sq") + (("master",) if "master" in st else ()):
                    if saved[name].shape != st[name].shape or saved[name].dtype != torch.float32:
                        raise ValueError(f"AdamW.load_state_dict: {name} of parameter {idx}: {tuple(saved[name].shape)} {saved[name].dtype}")
                    st[name].copy_(saved[name])
                if "master" in st:
                    p.copy_(st["master"])               # round to nearest even, what the kernel stores
        if state_dict.get("counters") is not None:
            self._need_state()
            self._counters.copy_(state_dict["counters"])
            self._host_t = int(state_dict["counters"][0])
