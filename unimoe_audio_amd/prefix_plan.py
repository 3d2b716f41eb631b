"""Host-side plan of an admission behind a cached prefix (umoe_engine_admit_prefix).

A CFG pair's prompts are left padded to one length T and both begin with the same P tokens (a voice prompt).  Row r has first_r pad
columns; its prefix token i sits in cache slot first_r + i at rope position i.  The prefix store holds the roped K / V of tokens
0 .. P - 1, so

    install   store tokens [0, max(P - first_r, 0))  ->  slots [first_r, P) of row r
    compute   columns [P, T) of both rows: kv slot = the column, positions from the FULL mask (cumsum - 1, masked -> 1), q_pos0 = P

In the shorter row the computed columns [P, P + first_r) hold its last first_r prefix tokens again; they are recomputed.
Plain functions on host values: no device, no library."""
from __future__ import annotations

from typing import List, NamedTuple, Sequence, Tuple

from ._lib import UmoeError


class PrefixPlan(NamedTuple):
    T: int
    P: int
    first: List[int]                            # pad columns per row
    install: List[Tuple[int, int, int]]         # per row (i0, s0, n): store tokens [i0, i0 + n) -> slots [s0, s0 + n)
    kv_pos: List[List[int]]                     # per row, per computed column j: the cache slot
    pos3: List[List[int]]                       # per row, per computed column j: the rope position (all three planes)
    q_pos0: List[int]                           # per row: keys [kv_start, q_pos0 + j] are visible to computed column j
    valid_count: List[int]                      # per row: rope position of the first generated token


def _rows(valid) -> List[List[int]]:
    rows = valid.tolist() if hasattr(valid, "tolist") else [list(r) for r in valid]
    return [[int(bool(v)) for v in r] for r in rows]


def prefix_plan(valid, P: int) -> PrefixPlan:
    """valid [R][T]: the left-padded mask of the full rows (R = 2 for a CFG pair); P: tokens of the cached prefix.  Raises UmoeError for
    what umoe_engine_admit_prefix refuses on the mask: P < 1, fewer than 2 columns behind the prefix, a row that is not left padded or
    empty."""
    rows = _rows(valid)
    if not rows or any(len(r) != len(rows[0]) for r in rows):
        raise UmoeError("prefix_plan: valid is [rows][T]")
    T, P = len(rows[0]), int(P)
    if P < 1:
        raise UmoeError(f"prefix_plan: a prefix of {P} tokens (need 1 <= P)")
    if T - P < 2:
        raise UmoeError(f"prefix_plan: {T - P} columns behind a prefix of {P} tokens (need 2 <= T - P; clamp P to T - 2)")
    first, install, kv_pos, pos3, q0, vc = [], [], [], [], [], []
    for r, m in enumerate(rows):
        cnt = sum(m)
        f = T - cnt
        if cnt == 0:
            raise UmoeError(f"prefix_plan: row {r} has no valid token")
        if any(m[:f]) or not all(m[f:]):
            raise UmoeError(f"prefix_plan: row {r} is not left-padded")
        first.append(f)
        install.append((0, f, max(P - f, 0)))
        kv_pos.append(list(range(P, T)))
        pos3.append([t - f if t >= f else 1 for t in range(P, T)])
        q0.append(P)
        vc.append(cnt)
    return PrefixPlan(T, P, first, install, kv_pos, pos3, q0, vc)


def common_prefix_len(*seqs: Sequence[int]) -> int:
    """length of the longest common prefix of the token id sequences"""
    n = 0
    for col in zip(*seqs):
        if any(c != col[0] for c in col):
            break
        n += 1
    return n


def split_point(neg_ids: Sequence[int], pos_ids: Sequence[int], voice_ids: Sequence[int], T: int) -> int:
    """P of a request: the longest common prefix of the pair's UNPADDED id rows and the voice's prefix ids, clamped to T - 2 (the engine
    runs at least 2 columns behind the prefix).  0 or less: no split admission for this request."""
    return min(common_prefix_len(neg_ids, pos_ids, voice_ids), int(T) - 2)
