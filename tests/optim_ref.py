"""What the optimizer tests share (tests/test_optim_cpu.py, tests/test_gpu_optim.py): the fp64 restatement of the step, an fp32
emulation of the kernels' operation order (csrc/umoe_optim.hip), the error bounds derived from that order, and a thin driver of the
three launch entries on raw tables.  No test lives here.

Bounds (u = 2^-24, gamma_k = k u / (1 - k u); every fp32 operation of the kernel is one correctly rounded operation: the build has
-ffp-contract=off and correctly rounded division and square root).  The restatement gets the kernel's own fp32 inputs -- w, m, v, the
gradient, clip, bc1, bc2 -- and the settings as the doubles the caller passed, so the roundings counted are the kernel's alone:

  g^ = fl(g clip)                                                               1 rounding
  m' = fl(fl(b1 m) + fl(omb1 g^)),  b1 = fl(beta1), omb1 = fl(1 - beta1)        first term 3 roundings (b1, product, sum), second 4
       (omb1, g^, product, sum)                          |m^ - m'| <= gamma_4 (|beta1 m| + |(1 - beta1) g|)
  v' = fl(fl(b2 v) + fl(fl(omb2 g^) g^))                                        first term 3, second 6 (omb2, g^ twice, two products,
       sum); every term is >= 0, so                      |v^ - v'| <= gamma_6 v'
  decay = fl(1 - fl(fl(lr) fl(wd)))                                             |decay^ - decay| <= u (3 lr wd + 1)   (decay <= 1)
  A = fl(w decay^)                                                              |A^ - A| <= u |w| (2 + 3 lr wd)
  step = fl(fl(lr) / bc1), num = fl(step m^)                                    3 roundings relative to |step m'|, plus m^'s own error
  den = fl(fl(fl(sqrt(v^)) / fl(sqrt(bc2))) + fl(eps))                          sqrt halves v^'s 6, + sqrt 1, + sqrt(bc2) 1, + division 1 = 6
       on the quotient; eps 1; the sum 1 more on both:   |den^ - den| <= 7 u den
  upd = fl(num / den)                                                           3 + 7 + 1 = 11 roundings relative to |upd|
  w' = fl(A - upd)                                                              1 rounding on |w'| <= |w| + |upd|
       |w^ - w'| <= u ((3 + 3 lr wd) |w| + 12 |upd|) + gamma_4 (|beta1 m| + |(1 - beta1) g|) (lr / bc1) / den
  written with gamma_k for k u below.  The data of the tests keeps every intermediate a normal fp32 number (or an exact zero).

  stage 1: a thread adds at most n_t = 8 ceil(ceil(CH / 8) / 256) + 1 squares (1 rounding each, then n_t - 1 sums), the butterfly adds 6
  roundings, the waves 3: a partial is within gamma_(n_t + 9) of its exact value, all terms >= 0.  Stage 2 sums in fp64 (n 2^-53,
  covered by 2^-40) -- so the sum of squares is within gamma_(n_t + 9) + 2^-40, the square root halves that, and its rounding to fp32
  adds u.   clip = fl(fl(max_norm) / fl(norm + fl(1e-6))): 4 roundings.   bc = fp32(1 - beta^(t+1)) in fp64: u + 2^-40.
"""
import ctypes as C

import numpy as np

U = 2.0 ** -24
f32 = np.float32


def gamma(k):
    return k * U / (1.0 - k * U)


# ------------------------------------------------------------------------------------------------------------ fp64 restatement
def adamw_fp64(w, m, v, g, *, lr, beta1, beta2, eps, wd, clip, bc1, bc2):
    """one step of the issue's formulas in fp64 on numpy arrays; -> (w', m', v', parts) with parts for the bounds"""
    w, m, v, g = (np.asarray(a, dtype=np.float64) for a in (w, m, v, g))
    clip, bc1, bc2 = float(clip), float(bc1), float(bc2)
    gc = g * clip
    m1 = beta1 * m + (1.0 - beta1) * gc
    v1 = beta2 * v + (1.0 - beta2) * gc * gc
    den = np.sqrt(v1) / np.sqrt(bc2) + eps
    upd = (lr / bc1) * m1 / den
    w1 = w * (1.0 - lr * wd) - upd
    parts = dict(m_mag=np.abs(beta1 * m) + np.abs((1.0 - beta1) * gc), v1=v1, den=den, upd=upd, w=w)
    return w1, m1, v1, parts


def adamw_bounds(parts, *, lr, wd, bc1):
    """(bound_w, bound_m, bound_v) of the derivation above"""
    bm = gamma(4) * parts["m_mag"]
    bv = gamma(6) * parts["v1"]
    bw = gamma(3) * (1.0 + lr * wd) * np.abs(parts["w"]) + gamma(12) * np.abs(parts["upd"]) + bm * (lr / float(bc1)) / parts["den"]
    return bw, bm, bv


def scalars_fp64(grads, max_norm, betas, t):
    """stage 1 + 2 in fp64: norm, clip (1 with max_norm None), [(bc1, bc2)] per group, at step counter t"""
    tot = sum(float(np.sum(np.asarray(g, dtype=np.float64) ** 2)) for g in grads)
    norm = float(np.sqrt(tot))
    clip = 1.0 if max_norm is None else min(1.0, max_norm / (norm + 1e-6))
    return norm, clip, [(1.0 - b1 ** (t + 1), 1.0 - b2 ** (t + 1)) for b1, b2 in betas]


def norm_rel_bound(chunk_elems):
    n_t = 8 * (-(-(-(-chunk_elems // 8)) // 256)) + 1
    return 0.5 * (gamma(n_t + 9) + 2.0 ** -40) * (1.0 + 2.0 ** -20) + U


CLIP_REL_BOUND = gamma(4)
BC_REL_BOUND = U + 2.0 ** -40


# ------------------------------------------------------------------------------------------------------------ fp32 emulation
def bf16_rne(x):
    """fp32 array -> bf16 bit patterns (uint16), round to nearest even (finite inputs)"""
    b = np.asarray(x, dtype=f32).view(np.uint32)
    return ((b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def bf16_to_f32(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(f32)


def adamw_emulated(w, m, v, g, *, lr, beta1, beta2, eps, wd, clip, bc1, bc2, plant=None):
    """the kernel's fp32 operation order on numpy float32 arrays; plant = one of the errors the bounds must reject:
    "no_bias_correction", "l2_decay", "no_clip", "eps_in_sqrt", "bf16_master" (w is rounded to bf16 before the update)"""
    w, m, v, g = (np.asarray(a, dtype=f32) for a in (w, m, v, g))
    clip, bc1, bc2 = f32(clip), f32(bc1), f32(bc2)
    lr_f, b1, omb1, b2, omb2, eps_f, wd_f = f32(lr), f32(beta1), f32(1.0 - beta1), f32(beta2), f32(1.0 - beta2), f32(eps), f32(wd)
    if plant == "no_bias_correction":
        bc1 = bc2 = f32(1.0)
    if plant == "no_clip":
        clip = f32(1.0)
    if plant == "bf16_master":
        w = bf16_to_f32(bf16_rne(w))
    gc = g * clip
    if plant == "l2_decay":
        gc = gc + wd_f * w
    m1 = b1 * m + omb1 * gc
    v1 = b2 * v + (omb2 * gc) * gc
    decay = f32(1.0) if plant == "l2_decay" else f32(1.0) - lr_f * wd_f
    step, sq = lr_f / bc1, np.sqrt(bc2)
    den = np.sqrt(v1 + eps_f * eps_f) / sq if plant == "eps_in_sqrt" else np.sqrt(v1) / sq + eps_f
    w1 = w * decay - (step * m1) / den
    return w1.astype(f32), m1.astype(f32), v1.astype(f32)


def sqsum_emulated(g, chunk_elems):
    """stage 1 on one aligned tensor (head 0): the partial of every chunk in the kernel's order"""
    g = np.asarray(g, dtype=f32)
    out = []
    for first in range(0, len(g), chunk_elems):
        x = g[first:first + chunk_elems]
        sq = x * x
        nvec = len(x) // 8
        iters = -(-nvec // 256) if nvec else 0
        body = np.zeros(iters * 256 * 8, dtype=f32)
        body[:nvec * 8] = sq[:nvec * 8]
        body = body.reshape(iters, 256, 8)
        acc = np.zeros(256, dtype=f32)
        for i in range(iters):
            for j in range(8):
                acc = acc + body[i, :, j]          # a thread without a vector in this iteration adds an exact 0
        tail = np.zeros(256, dtype=f32)
        tail[:len(x) - nvec * 8] = sq[nvec * 8:]
        acc = (acc + tail).reshape(4, 64)
        lane = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, lane ^ off]
        s = acc[0, 0]
        for wv in range(1, 4):
            s = s + acc[wv, 0]
        out.append(s)
    return np.array(out, dtype=f32)


def total_emulated(partials, fp32_sum=False):
    """stage 2's order: 256 contiguous runs in ascending order, then the runs in ascending order; fp32_sum = the planted error"""
    dt = f32 if fp32_sum else np.float64
    p = np.asarray(partials, dtype=f32).astype(dt)
    per = -(-len(p) // 256)
    pad = np.zeros(per * 256, dtype=dt)
    pad[:len(p)] = p
    runs = np.cumsum(pad.reshape(256, per), axis=1, dtype=dt)[:, -1] if per else np.zeros(256, dtype=dt)
    return float(np.cumsum(runs, dtype=dt)[-1])


# ------------------------------------------------------------------------------------------------------------ GPU driver
class Tables:
    """device tables over a list of dicts(p, g, master (None for an fp32 p), m, v, group): what optim.AdamW packs, on raw tensors"""

    def __init__(self, tensors, chunk_elems, num_groups, chunks=None):
        import torch
        from unimoe_audio_amd import optim as O
        self.tensors, self.ch, self.num_groups = tensors, chunk_elems, num_groups
        dev = tensors[0]["p"].device if tensors else torch.device("cuda:0")
        th = np.zeros(max(len(tensors), 1), dtype=O.TENSOR_DTYPE)
        for i, t in enumerate(tensors):
            th[i] = (t["p"].data_ptr(), 0 if t.get("g") is None else t["g"].data_ptr(), 0 if t.get("master") is None else t["master"].data_ptr(),
                     t["m"].data_ptr(), t["v"].data_ptr(), t["p"].numel(), t["group"], int(t["p"].dtype == torch.float32))
        self.th = th
        self.chh = O.build_chunk_table([t["p"].numel() for t in tensors], chunk_elems) if chunks is None else chunks
        self.n_chunks = len(self.chh)
        self.td = torch.from_numpy(th.view(np.uint8).reshape(-1).copy()).to(dev)
        self.cd = torch.from_numpy(self.chh.view(np.int64).reshape(-1).copy()).to(dev) if self.n_chunks else torch.zeros(2, dtype=torch.int64, device=dev)
        self.partial = torch.full((max(self.n_chunks, 1),), -7.0, dtype=torch.float32, device=dev)
        self.flags = torch.full((max(self.n_chunks, 1),), -7, dtype=torch.int32, device=dev)
        self.rec = torch.full((O.RECORD_WORDS,), -7.0, dtype=torch.float32, device=dev)
        self.counters = torch.zeros(2, dtype=torch.int64, device=dev)

    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def sqsum(self, grid_cap=0, host=True, **over):
        from unimoe_audio_amd import _lib as L
        a = dict(tensors=self.td.data_ptr(), n_tensors=len(self.tensors), chunks=self.cd.data_ptr(), n_chunks=self.n_chunks, chunk_elems=self.ch,
                 ht=self.th.ctypes.data if host else None, hc=self.chh.ctypes.data if host else None, num_groups=self.num_groups,
                 partial=self.partial.data_ptr(), flags=self.flags.data_ptr())
        a.update(over)
        return L.lib().umoe_optim_sqsum(a["tensors"], a["n_tensors"], a["chunks"], a["n_chunks"], a["chunk_elems"], a["ht"], a["hc"], a["num_groups"],
                                        grid_cap, a["partial"], a["flags"], self._stream())

    def scalars(self, hy, **over):
        from unimoe_audio_amd import _lib as L
        a = dict(partial=self.partial.data_ptr(), flags=self.flags.data_ptr(), n_chunks=self.n_chunks, hyper=C.byref(hy),
                 counters=self.counters.data_ptr(), rec=self.rec.data_ptr())
        a.update(over)
        return L.lib().umoe_optim_scalars(a["partial"], a["flags"], a["n_chunks"], a["hyper"], a["counters"], a["rec"], self._stream())

    def adamw(self, hy, grid_cap=0, host=True, t_host=-1, **over):
        from unimoe_audio_amd import _lib as L
        a = dict(tensors=self.td.data_ptr(), n_tensors=len(self.tensors), chunks=self.cd.data_ptr(), n_chunks=self.n_chunks, chunk_elems=self.ch,
                 ht=self.th.ctypes.data if host else None, hc=self.chh.ctypes.data if host else None, hyper=C.byref(hy),
                 rec=self.rec.data_ptr() if t_host < 0 else None, counters=self.counters.data_ptr())
        a.update(over)
        return L.lib().umoe_optim_adamw(a["tensors"], a["n_tensors"], a["chunks"], a["n_chunks"], a["chunk_elems"], a["ht"], a["hc"], grid_cap,
                                        a["hyper"], a["rec"], t_host, a["counters"], self._stream())

    def record(self):
        from unimoe_audio_amd import optim as O
        return self.rec.cpu().numpy().view(O.RECORD_DTYPE)[0]
