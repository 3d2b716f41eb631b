"""Host-side packing of the per-request settings table of a decode batch (umoe_row_params, include/umoe.h).

Each sampling setting of DecodeEngine.start_decode may be one value for the whole batch or a sequence with one value per batch entry.
All scalars: no table (the engine's scalar path, unchanged).  Any sequence: the rest is broadcast and one record per entry is packed
into a numpy structured array whose layout is the C struct's; the engine copies it to the device as it is.  Plain functions on host
values: no device, no library."""
from __future__ import annotations

from typing import Optional

import numpy as np

from ._lib import UmoeError

# the layout of umoe_row_params (tests/test_row_params_cpu.py compares it with the header through a compiled probe)
ROW_DTYPE = np.dtype([("cfg_scale", "<f4"), ("temperature", "<f4"), ("top_p", "<f4"), ("eos_mul", "<f4"), ("top_k", "<i4"),
                      ("do_sample", "<i4"), ("min_tokens", "<i4"), ("max_tokens", "<i4"), ("seed", "<u8")], align=True)
SETTINGS = ("cfg_scale", "temperature", "top_p", "top_k", "eos_mul", "do_sample", "seed", "min_tokens", "max_tokens")
_NONE_IS_MINUS_ONE = ("top_k", "min_tokens")


def is_sequence(v) -> bool:
    """list / tuple / numpy array / tensor with at least one axis; a str or a 0-d array is a scalar"""
    if isinstance(v, (list, tuple)):
        return True
    return hasattr(v, "tolist") and getattr(v, "ndim", 0) > 0


def _values(v):
    return list(v.tolist()) if hasattr(v, "tolist") else list(v)


def largest(v) -> int:
    """the value an engine is sized by: the setting itself, or the largest of its per-row values"""
    return max(int(x) for x in _values(v)) if is_sequence(v) else int(v)


def scaled(v, factor: int):
    """seconds -> tokens, element by element for a sequence"""
    return [int(x) * factor for x in _values(v)] if is_sequence(v) else v * factor


def pack_row_params(batch: int, **settings) -> Optional[np.ndarray]:
    """settings: every name of SETTINGS, each a scalar or a sequence of length `batch`.  Returns None when all are scalars, else the
    table [batch] of ROW_DTYPE: sequences element by element, scalars broadcast, top_k / min_tokens None -> -1, seed modulo 2^64.
    A sequence of another length raises UmoeError naming the argument."""
    if set(settings) != set(SETTINGS):
        raise TypeError(f"pack_row_params takes exactly {SETTINGS}, got {tuple(sorted(settings))}")
    if not any(is_sequence(v) for v in settings.values()):
        return None
    table = np.zeros(batch, dtype=ROW_DTYPE)
    for name in SETTINGS:
        v = settings[name]
        if is_sequence(v):
            vals = _values(v)
            if len(vals) != batch:
                raise UmoeError(f"{name}: a sequence of {len(vals)} values for a batch of {batch} (one value per batch entry, or a scalar)")
        else:
            vals = [v] * batch
        for b, x in enumerate(vals):
            if x is None:
                if name not in _NONE_IS_MINUS_ONE:
                    raise UmoeError(f"{name}: None is not a value (entry {b})")
                x = -1
            if name == "seed":
                x = int(x) % (1 << 64)
            elif name == "do_sample":
                x = int(bool(x))
            table[name][b] = x
    return table
