"""CPU suite: the decode engine's per-layer decision -- launch form of the MoE half, weight format of its expert launches, refusal --
pinned as a literal table through umoe_engine_plan_probe (csrc/umoe_engine_plan.h; no GPU, no engine).

The table was written from the code BEFORE the decision was one function: the enqueue side (moe_form, wide_mode, dense_mode, the flat block
of run_layer, experts_tiled, experts_wide) and the checking side (fp8_only_check, w12_only_check, fp8_step_check).  A cell is what a pass
ran there, per layer, or the substring of the refusal the GPU tests match.  Reference shape: 9 + 2 router columns (8 routed + 2 shared
experts), hidden 2048, intermediate 2752 / 1376.  On 256 compute units the flat expert launch has a schedule in every weight format up to
16 rows, on 100 it has none (tests/test_flat_plan_cpu.py, test_fp8_cpu.py, test_w12_cpu.py pin that)."""
import ctypes as C

import pytest

# forms (umoe_plan_out.form) and formats (UMOE_FMT_*)
TILED, RAGGED, FLAT, RIDERS, ROUTER, WIDE = range(6)
WP16, WP8, WP12, RM = range(4)
PREFILL, ADMISSION, DECODE = range(3)
SET, BF16, RM_EXP, RM_ATTN, H_WP8, H_WP12 = 1, 2, 4, 8, 16, 32

# what a layer holds
H_BF16 = SET | BF16 | RM_EXP | RM_ATTN            # the WP16 packs and the row-major tensors
H_BF16_NORM = SET | BF16                          # ... without the row-major tensors
H_BF16_W12 = H_BF16 | H_WP12                      # ... with WP12 copies (what a bf16 engine of at most 16 rows packs)
H_FP8_KEPT = H_BF16 | H_WP8                       # fp8 with the bf16 weights kept
H_FP8_ONLY = SET | RM_ATTN | H_WP8
H_W12_ONLY = SET | RM_ATTN | H_WP12
ENGINES = {
    "bf16": [H_BF16] * 2,
    "bf16_norm": [H_BF16_NORM] * 2,
    "bf16_w12": [H_BF16_W12] * 2,
    "fp8": [H_FP8_KEPT] * 2,
    "fp8_only": [H_FP8_ONLY] * 2,
    "w12_only": [H_W12_ONLY] * 2,
    "mixed": [H_W12_ONLY, H_BF16, H_W12_ONLY],    # one layer that was not packable among w12-only layers
}

# passes: (kind, rows of the engine, tokens)
PASSES = {
    "prefill24": (PREFILL, 2, 24), "prefill128": (PREFILL, 2, 128), "prompt1x2": (PREFILL, 2, 2), "admit2x12": (ADMISSION, 16, 24),
    "step2": (DECODE, 2, 2), "step16": (DECODE, 16, 16), "step18": (DECODE, 18, 18), "step32": (DECODE, 32, 32), "step64": (DECODE, 64, 64),
}

MISSING = "no bf16 expert weights"
LAYOUT = "fp8 expert weights need the dense decode layout"
FP8 = "fp8"


def plan(engine, pass_name, **kw):
    """-> [(form, format)] per layer, or the text of the first layer's refusal"""
    from unimoe_audio_amd import _lib as L
    kind, rows, n_tok = PASSES[pass_name]
    holds = ENGINES[engine]
    p = L.PlanIn(rows=rows, hidden=2048, inter_dyn=2752, inter_shared=1376, n_dyn=9, n_real=8, n_fix=2, ep_size=1, n_cu=256, tiled_prefill=1,
                 fuse_router=1, dense_min_rows=2, fp8_wide=0, w12_wide=0, flat_moe=-1, flat_w12=-1, wide_w12=-1, wide_decode=-1, kind=kind, n_tok=n_tok,
                 n_layers=len(holds))
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    arr = (C.c_uint8 * len(holds))(*holds)
    p.holds = C.cast(arr, C.POINTER(C.c_uint8))
    out = (L.PlanOut * len(holds))()
    rc = (C.c_int32 * len(holds))()
    msg = C.create_string_buffer(1024 * len(holds))
    assert L.lib().umoe_engine_plan_probe(C.byref(p), C.sizeof(p), out, rc, msg, 1024) == 0, L.lib().umoe_last_error()
    for l in range(len(holds)):
        if rc[l]:
            text = msg.raw[1024 * l:1024 * (l + 1)].split(b"\0")[0].decode()
            assert text.startswith("umoe_engine: "), text
            return text
    return [(out[l].form, out[l].format) for l in range(len(holds))]


def both(cell):
    return [cell, cell]


def mixed(w12_cell, bf16_cell):
    return [w12_cell, bf16_cell, w12_cell]


# (engine, pass, switches) -> the cell.  A string is a refusal: the message contains it.
TABLE = [
    # ---- the defaults, 256 compute units
    ("bf16", "prefill24", {}, both((RAGGED, WP16))), ("bf16", "prefill128", {}, both((TILED, RM))), ("bf16", "prompt1x2", {}, both((FLAT, WP16))),
    ("bf16", "admit2x12", {}, both((RAGGED, WP16))), ("bf16", "step2", {}, both((FLAT, WP16))), ("bf16", "step16", {}, both((FLAT, WP16))),
    ("bf16", "step18", {}, both((RAGGED, WP16))), ("bf16", "step32", {}, both((WIDE, WP16))), ("bf16", "step64", {}, both((WIDE, WP16))),
    ("bf16_norm", "prefill24", {}, both((RAGGED, WP16))), ("bf16_norm", "prefill128", {}, both((RAGGED, WP16))),
    ("bf16_w12", "prefill24", {}, both((RAGGED, WP16))), ("bf16_w12", "prefill128", {}, both((TILED, RM))), ("bf16_w12", "prompt1x2", {}, both((FLAT, WP12))),
    ("bf16_w12", "admit2x12", {}, both((RAGGED, WP16))), ("bf16_w12", "step2", {}, both((FLAT, WP12))), ("bf16_w12", "step16", {}, both((FLAT, WP12))),
    ("bf16_w12", "step18", {}, both((RAGGED, WP16))), ("bf16_w12", "step32", {}, both((WIDE, WP16))), ("bf16_w12", "step64", {}, both((WIDE, WP16))),
    ("fp8", "prefill24", {}, both((RAGGED, WP16))), ("fp8", "prefill128", {}, both((TILED, RM))), ("fp8", "prompt1x2", {}, both((FLAT, WP8))),
    ("fp8", "admit2x12", {}, both((RAGGED, WP16))), ("fp8", "step2", {}, both((FLAT, WP8))), ("fp8", "step16", {}, both((FLAT, WP8))),
    ("fp8", "step18", {}, LAYOUT), ("fp8", "step32", {}, LAYOUT), ("fp8", "step64", {}, LAYOUT),
    ("fp8_only", "prefill24", {}, both((TILED, WP8))), ("fp8_only", "prefill128", {}, both((TILED, WP8))), ("fp8_only", "prompt1x2", {}, both((FLAT, WP8))),
    ("fp8_only", "admit2x12", {}, both((TILED, WP8))), ("fp8_only", "step2", {}, both((FLAT, WP8))), ("fp8_only", "step16", {}, both((FLAT, WP8))),
    ("fp8_only", "step18", {}, MISSING), ("fp8_only", "step32", {}, MISSING), ("fp8_only", "step64", {}, MISSING),
    ("w12_only", "prefill24", {}, both((TILED, WP12))), ("w12_only", "prefill128", {}, both((TILED, WP12))), ("w12_only", "prompt1x2", {}, both((FLAT, WP12))),
    ("w12_only", "admit2x12", {}, both((TILED, WP12))), ("w12_only", "step2", {}, both((FLAT, WP12))), ("w12_only", "step16", {}, both((FLAT, WP12))),
    ("w12_only", "step18", {}, MISSING), ("w12_only", "step32", {}, MISSING), ("w12_only", "step64", {}, MISSING),
    ("mixed", "prefill24", {}, mixed((TILED, WP12), (RAGGED, WP16))), ("mixed", "prefill128", {}, mixed((TILED, WP12), (TILED, RM))),
    ("mixed", "prompt1x2", {}, mixed((FLAT, WP12), (FLAT, WP16))), ("mixed", "admit2x12", {}, mixed((TILED, WP12), (RAGGED, WP16))),
    ("mixed", "step2", {}, mixed((FLAT, WP12), (FLAT, WP16))), ("mixed", "step16", {}, mixed((FLAT, WP12), (FLAT, WP16))),
    ("mixed", "step18", {}, MISSING), ("mixed", "step32", {}, MISSING),
    # ---- umoe_engine_set_fp8_wide / umoe_engine_set_w12_wide: read by steps of 17..64 rows
    ("fp8", "step18", dict(fp8_wide=1), both((WIDE, WP8))), ("fp8", "step32", dict(fp8_wide=1), both((WIDE, WP8))), ("fp8", "step64", dict(fp8_wide=1), both((WIDE, WP8))),
    ("fp8", "step16", dict(fp8_wide=1), both((FLAT, WP8))),
    ("fp8_only", "step18", dict(fp8_wide=1), both((WIDE, WP8))), ("fp8_only", "step32", dict(fp8_wide=1), both((WIDE, WP8))),
    ("fp8_only", "step64", dict(fp8_wide=1), both((WIDE, WP8))),
    ("bf16_w12", "step18", dict(w12_wide=1), both((RAGGED, WP16))), ("bf16_w12", "step32", dict(w12_wide=1), both((WIDE, WP12))),
    ("bf16_w12", "step64", dict(w12_wide=1), both((WIDE, WP12))), ("bf16", "step32", dict(w12_wide=1), both((WIDE, WP16))),
    ("w12_only", "step18", dict(w12_wide=1), both((WIDE, WP12))), ("w12_only", "step32", dict(w12_wide=1), both((WIDE, WP12))),
    ("w12_only", "step64", dict(w12_wide=1), both((WIDE, WP12))),
    ("mixed", "step18", dict(w12_wide=1), mixed((WIDE, WP12), (WIDE, WP16))), ("mixed", "step32", dict(w12_wide=1), mixed((WIDE, WP12), (WIDE, WP16))),
    # ---- UMOE_FLAT_MOE=0: read by the dense layout
    ("bf16", "step16", dict(flat_moe=0), both((RIDERS, WP16))), ("bf16", "prompt1x2", dict(flat_moe=0), both((RIDERS, WP16))),
    ("bf16_w12", "step2", dict(flat_moe=0), both((RIDERS, WP16))), ("fp8", "step16", dict(flat_moe=0), FP8), ("fp8", "prompt1x2", dict(flat_moe=0), FP8),
    ("fp8_only", "step16", dict(flat_moe=0), MISSING), ("w12_only", "step16", dict(flat_moe=0), MISSING), ("w12_only", "prompt1x2", dict(flat_moe=0), MISSING),
    ("mixed", "step2", dict(flat_moe=0), MISSING), ("bf16", "step32", dict(flat_moe=0), both((WIDE, WP16))), ("bf16", "prefill24", dict(flat_moe=0), both((RAGGED, WP16))),
    ("bf16", "step16", dict(flat_moe=1), both((FLAT, WP16))),
    # ---- UMOE_FUSE_ROUTER=0
    ("bf16", "step16", dict(fuse_router=0), both((ROUTER, WP16))), ("bf16_w12", "step2", dict(fuse_router=0), both((ROUTER, WP16))),
    ("bf16", "prompt1x2", dict(fuse_router=0), both((ROUTER, WP16))), ("fp8", "step16", dict(fuse_router=0), FP8), ("fp8_only", "step2", dict(fuse_router=0), MISSING),
    ("w12_only", "step16", dict(fuse_router=0), MISSING), ("mixed", "step16", dict(fuse_router=0), MISSING),
    ("fp8", "step32", dict(fuse_router=0, fp8_wide=1), both((WIDE, WP8))),
    # ---- UMOE_FLAT_W12=0: read by the flat launch of a layer with WP12 copies
    ("bf16_w12", "step16", dict(flat_w12=0), both((FLAT, WP16))), ("bf16_w12", "prompt1x2", dict(flat_w12=0), both((FLAT, WP16))),
    ("bf16_w12", "step2", dict(flat_w12=1), both((FLAT, WP12))), ("bf16", "step16", dict(flat_w12=0), both((FLAT, WP16))),
    ("fp8", "step16", dict(flat_w12=0), both((FLAT, WP8))), ("w12_only", "step16", dict(flat_w12=0), MISSING), ("mixed", "step2", dict(flat_w12=0), MISSING),
    ("w12_only", "prefill24", dict(flat_w12=0), both((TILED, WP12))), ("w12_only", "step32", dict(flat_w12=0, w12_wide=1), both((WIDE, WP12))),
    # ---- UMOE_WIDE_W12=0: read by the wide form of a layer with WP12 copies
    ("bf16_w12", "step32", dict(w12_wide=1, wide_w12=0), both((WIDE, WP16))), ("bf16_w12", "step32", dict(w12_wide=1, wide_w12=1), both((WIDE, WP12))),
    ("w12_only", "step32", dict(w12_wide=1, wide_w12=0), MISSING), ("mixed", "step18", dict(w12_wide=1, wide_w12=0), MISSING),
    ("w12_only", "step16", dict(w12_wide=1, wide_w12=0), both((FLAT, WP12))),
    # ---- UMOE_WIDE_DECODE: 0 never wide (64 rows with the row-major tensors: the tiled kernels), 1 at every size
    ("bf16", "step32", dict(wide_decode=0), both((RAGGED, WP16))), ("bf16", "step64", dict(wide_decode=0), both((TILED, RM))),
    ("bf16_norm", "step64", dict(wide_decode=0), both((RAGGED, WP16))), ("bf16", "step18", dict(wide_decode=1), both((WIDE, WP16))),
    ("bf16_w12", "step18", dict(wide_decode=1, w12_wide=1), both((WIDE, WP12))), ("bf16", "step16", dict(wide_decode=1), both((FLAT, WP16))),
    ("fp8", "step32", dict(wide_decode=0, fp8_wide=1), LAYOUT), ("fp8", "step18", dict(wide_decode=1), LAYOUT), ("fp8", "step64", dict(wide_decode=0, fp8_wide=1), LAYOUT),
    ("fp8_only", "step32", dict(wide_decode=0, fp8_wide=1), MISSING), ("w12_only", "step32", dict(wide_decode=0, w12_wide=1), MISSING),
    ("mixed", "step18", dict(wide_decode=0, w12_wide=1), MISSING), ("w12_only", "step18", dict(wide_decode=1, w12_wide=1), both((WIDE, WP12))),
    # ---- UMOE_TILED_PREFILL=0: read by prefills (and by a step of 64 rows that is not wide)
    ("bf16", "prefill128", dict(tiled_prefill=0), both((RAGGED, WP16))), ("fp8", "prefill128", dict(tiled_prefill=0), both((RAGGED, WP16))),
    ("bf16", "step64", dict(tiled_prefill=0, wide_decode=0), both((RAGGED, WP16))),
    ("fp8_only", "prefill24", dict(tiled_prefill=0), MISSING), ("fp8_only", "prefill128", dict(tiled_prefill=0), MISSING),
    ("fp8_only", "admit2x12", dict(tiled_prefill=0), MISSING), ("w12_only", "prefill24", dict(tiled_prefill=0), MISSING),
    ("w12_only", "admit2x12", dict(tiled_prefill=0), MISSING), ("mixed", "prefill128", dict(tiled_prefill=0), MISSING),
    ("fp8_only", "step16", dict(tiled_prefill=0), both((FLAT, WP8))), ("w12_only", "prompt1x2", dict(tiled_prefill=0), both((FLAT, WP12))),
    # ---- UMOE_DENSE_MIN_ROWS=4: 2 rows leave the dense layout
    ("bf16", "step2", dict(dense_min_rows=4), both((RAGGED, WP16))), ("bf16", "prompt1x2", dict(dense_min_rows=4), both((RAGGED, WP16))),
    ("fp8", "step2", dict(dense_min_rows=4), LAYOUT), ("fp8", "prompt1x2", dict(dense_min_rows=4), both((RAGGED, WP16))),
    ("fp8_only", "step2", dict(dense_min_rows=4), MISSING), ("fp8_only", "prompt1x2", dict(dense_min_rows=4), both((TILED, WP8))),
    ("w12_only", "step2", dict(dense_min_rows=4), MISSING), ("w12_only", "prompt1x2", dict(dense_min_rows=4), both((TILED, WP12))),
    ("bf16", "step16", dict(dense_min_rows=4), both((FLAT, WP16))),
    # ---- 100 compute units: no flat schedule in any format
    ("bf16", "step16", dict(n_cu=100), both((RIDERS, WP16))), ("bf16", "prompt1x2", dict(n_cu=100), both((RIDERS, WP16))), ("bf16_w12", "step2", dict(n_cu=100), both((RIDERS, WP16))),
    ("fp8", "step16", dict(n_cu=100), FP8), ("fp8", "prompt1x2", dict(n_cu=100), FP8), ("fp8_only", "step2", dict(n_cu=100), FP8),
    ("w12_only", "step16", dict(n_cu=100), MISSING), ("w12_only", "prompt1x2", dict(n_cu=100), MISSING), ("mixed", "step16", dict(n_cu=100), MISSING),
    ("bf16", "step16", dict(n_cu=100, fuse_router=0), both((ROUTER, WP16))), ("bf16", "step16", dict(n_cu=0), both((RIDERS, WP16))),
    ("bf16", "prefill24", dict(n_cu=100), both((RAGGED, WP16))), ("bf16", "prefill128", dict(n_cu=100), both((TILED, RM))), ("bf16", "admit2x12", dict(n_cu=100), both((RAGGED, WP16))),
    ("bf16", "step18", dict(n_cu=100), both((RAGGED, WP16))), ("bf16", "step32", dict(n_cu=100), both((WIDE, WP16))), ("bf16", "step64", dict(n_cu=100), both((WIDE, WP16))),
    ("fp8", "step32", dict(n_cu=100, fp8_wide=1), both((WIDE, WP8))), ("fp8_only", "prefill24", dict(n_cu=100), both((TILED, WP8))),
    ("fp8_only", "step32", dict(n_cu=100, fp8_wide=1), both((WIDE, WP8))), ("w12_only", "prefill128", dict(n_cu=100), both((TILED, WP12))),
    ("w12_only", "admit2x12", dict(n_cu=100), both((TILED, WP12))), ("w12_only", "step32", dict(n_cu=100, w12_wide=1), both((WIDE, WP12))),
    ("mixed", "step32", dict(n_cu=100, w12_wide=1), mixed((WIDE, WP12), (WIDE, WP16))),
    # ---- a shape outside the router riders (8 router columns + 2): the router launch up to 16 rows, never wide
    ("bf16", "step16", dict(n_dyn=8), both((ROUTER, WP16))), ("bf16_w12", "step2", dict(n_dyn=8), both((ROUTER, WP16))), ("bf16", "prompt1x2", dict(n_dyn=8), both((ROUTER, WP16))),
    ("bf16", "step32", dict(n_dyn=8), both((RAGGED, WP16))), ("bf16", "step64", dict(n_dyn=8), both((TILED, RM))), ("bf16", "prefill128", dict(n_dyn=8), both((TILED, RM))),
    ("fp8", "step16", dict(n_dyn=8), LAYOUT), ("fp8_only", "step16", dict(n_dyn=8), LAYOUT), ("fp8", "step32", dict(n_dyn=8, fp8_wide=1), LAYOUT),
    ("w12_only", "step16", dict(n_dyn=8), MISSING), ("w12_only", "step32", dict(n_dyn=8, w12_wide=1), MISSING), ("w12_only", "prefill24", dict(n_dyn=8), both((TILED, WP12))),
    # ---- 11 routed + 2 shared experts: more groups than the tiled and the flat launch have
    ("bf16", "prefill128", dict(n_dyn=12, n_real=11), both((RAGGED, WP16))), ("bf16", "step16", dict(n_dyn=12, n_real=11), both((ROUTER, WP16))),
    ("bf16", "step16", dict(n_real=8, n_dyn=9, n_fix=2), both((FLAT, WP16))),
    ("fp8_only", "prefill24", dict(n_dyn=12, n_real=11), MISSING), ("fp8_only", "admit2x12", dict(n_dyn=12, n_real=11), MISSING),
    ("w12_only", "prefill24", dict(n_dyn=12, n_real=11), MISSING), ("w12_only", "step16", dict(n_dyn=12, n_real=11), MISSING),
    ("bf16", "step32", dict(n_dyn=12, n_real=11), both((RAGGED, WP16))),
]


def test_the_table_covers_every_engine_and_pass():
    assert {(e, p) for e, p, kw, _ in TABLE if not kw} >= {(e, p) for e in ENGINES if e != "bf16_norm" for p in PASSES} - {("mixed", "step64")}
    assert len({(e, p, tuple(sorted(kw.items()))) for e, p, kw, _ in TABLE}) == len(TABLE)          # no cell twice


@pytest.mark.parametrize("cus", ["256", "fewer"])
def test_every_cell_of_the_table(cus):
    """the cells on 256 compute units, then the cells that set another count (100; 0: the count is unknown)"""
    bad = []
    n = 0
    for engine, pass_name, kw, want in TABLE:
        if ("n_cu" in kw) != (cus == "fewer"):
            continue
        n += 1
        got = plan(engine, pass_name, **kw)
        ok = (isinstance(got, str) and want in got) if isinstance(want, str) else got == want
        if not ok:
            bad.append((engine, pass_name, kw, want, got))
    assert n > 20 and not bad, bad


def test_a_refusal_names_the_form_the_switch_and_the_missing_weights():
    text = plan("w12_only", "step16", flat_w12=0)
    assert "layer 0" in text and "UMOE_FLAT_W12=0" in text and "WP16" in text and MISSING in text and "w12-only" in text
    text = plan("fp8_only", "step32")
    assert "32 rows" in text and "umoe_engine_set_fp8_wide" in text and "MOE_RAGGED" in text and MISSING in text and "fp8-only" in text
    text = plan("mixed", "step16", n_cu=100)
    assert "100 compute units" in text and "MOE_RIDERS" in text and MISSING in text
    text = plan("fp8", "step16", n_cu=100)
    assert "100 compute units" in text and FP8 in text and MISSING not in text          # (it kept its bf16 weights: the fp8 rule alone refuses)


def test_expert_parallel_is_outside_the_decision_and_refuses_packed_holdings():
    from unimoe_audio_amd import _lib as L
    assert plan("bf16", "step16", ep_size=2) == both((6, WP16))          # the expert-parallel decode half (run_moe_ep)
    assert plan("bf16", "prefill128", ep_size=2) == both((TILED, RM))    # its prefill runs replicated on the tiled path
    for engine in ("fp8", "fp8_only", "w12_only", "bf16_w12"):
        assert "expert parallel" in plan(engine, "step16", ep_size=2)
    p = L.PlanIn(n_layers=1)
    out, rc, msg = (L.PlanOut * 1)(), (C.c_int32 * 1)(), C.create_string_buffer(64)
    assert L.lib().umoe_engine_plan_probe(C.byref(p), C.sizeof(p), out, rc, msg, 64) != 0          # no holdings
    arr = (C.c_uint8 * 1)(H_BF16)
    p.holds = C.cast(arr, C.POINTER(C.c_uint8))
    assert L.lib().umoe_engine_plan_probe(C.byref(p), C.sizeof(p) - 4, out, rc, msg, 64) != 0      # a mirror of another size
