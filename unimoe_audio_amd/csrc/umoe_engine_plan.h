// Decode engine: which launch form a layer's MoE half takes in a pass, which weight format its expert launches stream, and whether the
// pass is refused because the layer does not hold that format -- ONE pure function of a POD (umoe_plan_in, include/umoe.h).  The engine
// runs it for every layer before anything is enqueued (plan_pass) and again in run_layer, which switches on the result: a check cannot
// disagree with the enqueue, because there is no second copy of the rules.  Plain C++, no HIP: tests/test_engine_plan_cpu.py pins the
// table through umoe_engine_plan_probe without a GPU.
#pragma once
#include <stdio.h>

#include "umoe.h"

// Does a schedule of the flat expert launch exist for this decode shape, streamed in `format` (UMOE_FMT_WP16 / WP8 / WP12), on n_wg
// workgroups?  (umoe_moe_flat.hip, host code.  The answer is kept per format for the last shape: the decision asks before every layer of
// every eager step, and a plan search costs the host milliseconds.)
bool umoe_flat_feasible(int format, int n_wg, int S, int D, int I_dyn, int I_sh, int n_real, int n_fix);

// What a layer's router and experts are enqueued as: each form is one block of run_layer with no fall-through into another.
enum MoeForm {
    MOE_TILED,     // prefill: router + dispatch tables, tiled MFMA GEMMs (row-major bf16 at >= 64 rows; WP8 / WP12 at every row count)
    MOE_RAGGED,    // router + dispatch tables, weight-streaming GEMMs over the experts' ragged row lists
    MOE_FLAT,      // dense decode, ONE launch: router riders, RMSNorm, gate/up and down, one workgroup per CU (umoe_moe_flat.hip)
    MOE_RIDERS,    // dense decode, launch per kernel: RMSNorm | gate/up with the router riding in it | down
    MOE_ROUTER,    // dense decode, launch per kernel: router | gate/up | down
    MOE_WIDE,      // dense decode of 17..64 rows: router | RMSNorm + re-lay | gate/up | down, each weight streamed once for all row tiles
    MOE_EP,        // expert parallel decode (run_moe_ep): outside this decision, named so that every layer of every pass has a form
};

// why the form / format is what it is: only a refusal turns it into text (the decision itself formats nothing)
enum PlanWhy {
    WHY_DEFAULT,
    WHY_DEC_NO_FP8_WIDE, WHY_DEC_WIDE_OFF, WHY_DEC_NOT_DENSE,          // a decode step outside the dense layout and not wide: MOE_RAGGED
    WHY_PRE_TILED_OFF, WHY_PRE_GROUPS, WHY_PRE_DIMS,                   // a prefill whose experts cannot run tiled: MOE_RAGGED
    WHY_ROUTER_OFF, WHY_ROUTER_SHAPE,                                  // MOE_ROUTER
    WHY_FLAT_OFF, WHY_FLAT_NO_SCHEDULE,                                // MOE_RIDERS (or, format WP8, the fp8 flat launch without a schedule)
    WHY_FLAT_W12_OFF, WHY_FLAT_W12_NO_SCHEDULE,                        // MOE_FLAT on WP16 although the layer has WP12 copies
    WHY_WIDE_W12_OFF,                                                  // MOE_WIDE on WP16 although the layer has WP12 copies
};

struct umoe_plan_facts {     // what the decision reads of the OTHER layers
    bool fp8;                // some layer has WP8 weights: every decode layer of the engine runs on WP8 (flat or wide) or the step is refused
    bool w12_only;           // some layer holds the WP12 copies and nothing else: steps of 17..64 rows are wide at every size
};

static inline bool plan_w12_only(uint8_t h) { return (h & UMOE_HOLD_SET) && !(h & UMOE_HOLD_BF16) && (h & UMOE_HOLD_WP12) && !(h & UMOE_HOLD_WP8); }

static inline umoe_plan_facts umoe_plan_engine_facts(const umoe_plan_in& p) {
    umoe_plan_facts f{false, false};
    for (int l = 0; l < p.n_layers; ++l) {
        f.fp8 |= (p.holds[l] & UMOE_HOLD_WP8) != 0;
        f.w12_only |= plan_w12_only(p.holds[l]);
    }
    return f;
}

static inline bool umoe_plan_ep_decode(const umoe_plan_in& p) { return p.ep_size > 1 && p.n_tok == p.rows; }

// the dense-expert layout (every expert computes all rows; no dispatch tables): expert parallel decode IS it; an admission prefill of
// `rows` tokens is a prefill, ragged dispatch
static inline bool umoe_plan_dense(const umoe_plan_in& p) {
    if (umoe_plan_ep_decode(p)) return true;
    return p.kind != UMOE_PASS_ADMISSION && p.n_tok == p.rows && p.n_tok <= 16 && p.n_tok >= p.dense_min_rows;
}

// the shapes the wide form (umoe_gemm_wide.hip) is written for: 17..64 rows on one GPU, the router shapes of the 16-row step
static inline bool umoe_plan_wide_shape(const umoe_plan_in& p) {
    return p.kind != UMOE_PASS_ADMISSION && p.n_tok == p.rows && p.n_tok > 16 && p.n_tok <= 64 && p.ep_size == 1 && p.n_dyn == 9 && p.n_fix == 2 &&
           p.hidden == 2048 && p.n_real + p.n_fix <= 12;
}

// A decode step (never a prefill, whatever its token count) takes the wide form: on a bf16 engine at the sizes where it was MEASURED faster
// than the ragged path of the same process by more than the run-to-run spread (profiles/wide_decode.json; ms/step ragged | wide,
// 36 layers: batch 9 4.554 | 4.553 and 12 4.625 | 4.619 inside the spread -> ragged; 16 5.072 | 4.661, 24 6.099 | 5.544, 32 8.122 | 5.929
// -> wide; between the measured sizes only what the figures bound: 4 tiles cost at most the 5.929 of 32 and the ragged path at least the
// 6.099 of 24; batch 13..15 and 17..23 have no such bound and stay ragged), UMOE_WIDE_DECODE=1 at every size, =0 never.  An fp8 engine
// (with umoe_engine_set_fp8_wide) and an engine with w12-only layers have no other path above 16 rows: wide at EVERY size unless
// UMOE_WIDE_DECODE=0 -- and then their step is refused.
static inline bool umoe_plan_wide(const umoe_plan_in& p, const umoe_plan_facts& f) {
    if (p.kind != UMOE_PASS_DECODE || !umoe_plan_wide_shape(p)) return false;
    if (f.w12_only) return p.wide_decode != 0;
    if (f.fp8) return p.fp8_wide && p.wide_decode != 0;
    if (p.wide_decode < 0) return p.rows == 32 || (p.rows >= 48 && p.rows <= 64);
    return p.wide_decode != 0;
}

// workgroups of the flat expert launch: one per CU.  Its in-launch hand-offs need every workgroup RESIDENT at once (a waiting workgroup
// never yields its CU), so a device that exposes fewer CUs than a schedule needs (partition, CU mask, UMOE_FAKE_CUS) takes the
// launch-per-kernel form instead of discovering it by a timeout.
static inline int umoe_plan_flat_wgs(const umoe_plan_in& p) { return p.n_cu < 256 ? p.n_cu : 256; }

static inline bool plan_flat_feasible(const umoe_plan_in& p, int format) {
    const int n_wg = umoe_plan_flat_wgs(p);
    return n_wg > 0 && umoe_flat_feasible(format, n_wg, p.n_tok, p.hidden, p.inter_dyn, p.inter_shared, p.n_real, p.n_fix);
}

// the tiled GEMM on packed expert weights: 32-wide K granules; WP12 exception records address K / 32 < 127 granules
static inline bool plan_tiled_dims(const umoe_plan_in& p, int format) {
    const bool m32 = p.hidden % 32 == 0 && p.inter_dyn % 32 == 0 && (p.n_fix == 0 || p.inter_shared % 32 == 0);
    return m32 && (format != UMOE_FMT_WP12 || (p.hidden / 32 < 127 && p.inter_dyn / 32 < 127 && p.inter_shared / 32 < 127));
}

// what the pass would run and why, by PlanWhy; %d: the engine's rows ('r'), the experts per layer ('g') or the compute units ('c')
struct PlanWhyText { const char* text; char arg; };
static const PlanWhyText kPlanWhy[] = {
    /* WHY_DEFAULT */ {nullptr, 0},
    /* WHY_DEC_NO_FP8_WIDE */ {"a decode step of %d rows without the fp8 wide form (umoe_engine_set_fp8_wide, UMOE_WIDE_DECODE) takes MOE_RAGGED over WP16 packs", 'r'},
    /* WHY_DEC_WIDE_OFF */ {"UMOE_WIDE_DECODE=0 sends a decode step of %d rows to MOE_RAGGED over WP16 packs", 'r'},
    /* WHY_DEC_NOT_DENSE */ {"a decode step of %d rows outside the dense layout takes MOE_RAGGED over WP16 packs", 'r'},
    /* WHY_PRE_TILED_OFF */ {"UMOE_TILED_PREFILL=0 runs the experts of a prefill on the weight-streaming GEMM (MOE_RAGGED) over WP16 packs", 0},
    /* WHY_PRE_GROUPS */ {"a prefill of %d experts per layer takes MOE_RAGGED over WP16 packs (the tiled launch has 12 groups)", 'g'},
    /* WHY_PRE_DIMS */ {"the tiled GEMM on packed expert weights needs hidden and intermediate sizes that are multiples of 32 (WP12: below 4064), so this prefill takes MOE_RAGGED over WP16 packs", 0},
    /* WHY_ROUTER_OFF */ {"UMOE_FUSE_ROUTER=0 selects the launch-per-kernel form MOE_ROUTER over WP16 packs", 0},
    /* WHY_ROUTER_SHAPE */ {"this shape selects the launch-per-kernel form MOE_ROUTER over WP16 packs (the flat expert launch is written for 9 + 2 experts at hidden 2048 / 4096)", 0},
    /* WHY_FLAT_OFF */ {"UMOE_FLAT_MOE=0 selects the launch-per-kernel forms (MOE_RIDERS / MOE_ROUTER) over WP16 packs", 0},
    /* WHY_FLAT_NO_SCHEDULE */ {"the flat expert launch has no schedule on %d compute units (on WP16 packs MOE_RIDERS runs instead)", 'c'},
    /* WHY_FLAT_W12_OFF */ {"UMOE_FLAT_W12=0 runs the flat expert launch on the WP16 packs", 0},
    /* WHY_FLAT_W12_NO_SCHEDULE */ {"the flat expert launch on the WP12 copies has no schedule on %d compute units and runs on the WP16 packs", 'c'},
    /* WHY_WIDE_W12_OFF */ {"UMOE_WIDE_W12=0 (or umoe_engine_set_w12_wide off) runs the wide form of %d rows on the WP16 packs", 'r'},
};
// one text per holding: what the layer has instead of the weights the pass would stream
static inline const char* plan_holding_text(uint8_t h) {
    if (h & UMOE_HOLD_BF16) return "this engine runs its decode steps on fp8 expert weights and this layer has none (umoe_engine_set_layer_fp8)";
    if (h & UMOE_HOLD_WP8) return "this layer holds no bf16 expert weights (fp8-only: exp_gu / exp_dn / sh_gu / sh_dn and rm_exp_* / rm_sh_* were not given)";
    if (h & UMOE_HOLD_WP12) return "this layer holds no bf16 expert weights (w12-only: exp_gu / exp_dn / sh_gu / sh_dn and rm_exp_* / rm_sh_* were not given: the WP12 copies are all there is)";
    return "this layer holds no expert weights at all (no bf16 expert weights were given, and neither umoe_engine_set_layer_fp8 nor umoe_engine_set_layer_w12 was called)";
}

// fp8_rule: an fp8 engine decodes on its WP8 weights only, whatever else the layer holds; missing: the layer does not hold `format`
static inline void plan_refusal_text(const umoe_plan_in& p, int l, int why, int format, bool fp8_rule, bool missing, char* msg, size_t n) {
    static const char* const names[4] = {"WP16", "WP8", "WP12", "row-major bf16"};
    const PlanWhyText& t = kPlanWhy[why];
    char what[256], head[128];
    if (t.text) snprintf(what, sizeof(what), t.text, t.arg == 'r' ? p.rows : t.arg == 'g' ? p.n_real + p.n_fix : p.n_cu);
    else snprintf(what, sizeof(what), "this pass streams %s expert weights", names[format & 3]);
    const bool layout = why <= WHY_DEC_NOT_DENSE || why == WHY_ROUTER_SHAPE;
    if (fp8_rule) snprintf(head, sizeof(head), "fp8 expert weights need the %s (layer %d)", layout ? "dense decode layout of the flat expert launch, or the fp8 wide form" : "flat expert launch with its router riders", l);
    else snprintf(head, sizeof(head), "layer %d", l);
    snprintf(msg, n, "umoe_engine: %s: %s%s%s", head, what, missing ? ", and " : "", missing ? plan_holding_text(p.holds[l]) : "");
}

// The decision for layer l.  Returns 0 and fills `out`, or -1 with the refusal in msg: the pass would stream a format the layer does not
// hold (out still names what the pass would have run).
static inline int umoe_plan_layer(const umoe_plan_in& p, const umoe_plan_facts& f, int l, umoe_plan_out* out, char* msg, size_t msg_len) {
    const uint8_t h = p.holds[l];
    const int G = p.n_real + p.n_fix;
    out->form = MOE_EP; out->format = UMOE_FMT_WP16; out->attn = UMOE_ATTN_STREAM;
    if (!(h & UMOE_HOLD_SET)) {
        snprintf(msg, msg_len, "umoe_engine: layer %d has no weights", l);
        return -1;
    }
    if (p.ep_size > 1 && (!(h & UMOE_HOLD_BF16) || (h & (UMOE_HOLD_WP8 | UMOE_HOLD_WP12)))) {
        snprintf(msg, msg_len, "umoe_engine: layer %d: fp8 / WP12 expert weights and layers with no bf16 expert weights are not supported expert parallel (ep_size %d)", l, p.ep_size);
        return -1;
    }
    const bool bf16 = (h & UMOE_HOLD_BF16) != 0, has_rm = (h & UMOE_HOLD_RM_EXP) && (h & UMOE_HOLD_RM_ATTN);
    const bool wide = umoe_plan_wide(p, f), dense = umoe_plan_dense(p);
    // many rows (prefill): the attention GEMMs on the compute-bound tiled MFMA kernel over the row-major weights (a layer without bf16
    // expert weights has no rm_exp_*)
    out->attn = wide ? UMOE_ATTN_WIDE : ((bf16 ? has_rm : (h & UMOE_HOLD_RM_ATTN) != 0) && p.n_tok >= 64 && p.tiled_prefill) ? UMOE_ATTN_TILED : UMOE_ATTN_STREAM;
    if (umoe_plan_ep_decode(p)) return 0;
    int why = WHY_DEFAULT;
    // 1. the form, from the pass, the shape and the switches
    if (wide) {
        out->form = MOE_WIDE;
    } else if (!dense) {
        // a layer without bf16 expert weights: the tiled kernel on its WP8 blocks / WP12 copies at EVERY row count of a prefill (nothing
        // else reads them outside the decode launches)
        const int packed = (h & UMOE_HOLD_WP8) ? UMOE_FMT_WP8 : UMOE_FMT_WP12;
        const bool tiled = bf16 ? has_rm && p.n_tok >= 64 && p.tiled_prefill && G <= 12
                                : p.kind != UMOE_PASS_DECODE && p.tiled_prefill && G <= 12 && plan_tiled_dims(p, packed);
        out->form = tiled ? MOE_TILED : MOE_RAGGED;
        if (!tiled)
            why = p.kind == UMOE_PASS_DECODE ? (!umoe_plan_wide_shape(p) ? WHY_DEC_NOT_DENSE : f.fp8 && !f.w12_only ? WHY_DEC_NO_FP8_WIDE : WHY_DEC_WIDE_OFF)
                                             : (!p.tiled_prefill ? WHY_PRE_TILED_OFF : G > 12 ? WHY_PRE_GROUPS : bf16 ? WHY_DEFAULT : WHY_PRE_DIMS);
    } else if (!(p.fuse_router && p.n_dyn == 9 && p.n_fix == 2 && (p.hidden == 2048 || p.hidden == 4096))) {
        out->form = MOE_ROUTER;      // not the shapes the router riders are written for (router4_body<9, 2>; dense: <= 16 rows)
        why = p.fuse_router ? WHY_ROUTER_SHAPE : WHY_ROUTER_OFF;
    } else if (p.flat_moe != 0 && plan_flat_feasible(p, UMOE_FMT_WP16)) {
        out->form = MOE_FLAT;
    } else {
        out->form = MOE_RIDERS;
        why = p.flat_moe != 0 ? WHY_FLAT_NO_SCHEDULE : WHY_FLAT_OFF;
    }
    // 2. the format its expert launches stream
    switch (out->form) {
        case MOE_TILED:
            out->format = bf16 ? UMOE_FMT_RM : (h & UMOE_HOLD_WP8) ? UMOE_FMT_WP8 : UMOE_FMT_WP12;
            break;
        case MOE_FLAT:
            if (f.fp8) {
                out->format = UMOE_FMT_WP8;
                if (!plan_flat_feasible(p, UMOE_FMT_WP8)) {
                    plan_refusal_text(p, l, WHY_FLAT_NO_SCHEDULE, UMOE_FMT_WP8, true, !(h & UMOE_HOLD_WP8), msg, msg_len);
                    return -1;
                }
            } else if (h & UMOE_HOLD_WP12) {      // the same launch on the WP12 copies: the same outputs, 0.75 of the bytes
                const bool ok = p.flat_w12 != 0 && plan_flat_feasible(p, UMOE_FMT_WP12);
                out->format = ok ? UMOE_FMT_WP12 : UMOE_FMT_WP16;
                if (!ok) why = p.flat_w12 != 0 ? WHY_FLAT_W12_NO_SCHEDULE : WHY_FLAT_W12_OFF;
            }
            break;
        case MOE_WIDE:
            if (f.fp8) {
                out->format = UMOE_FMT_WP8;
            } else if (h & UMOE_HOLD_WP12) {      // a layer without copies (not packable) runs the WP16 launches
                const bool ok = p.w12_wide && p.wide_w12 != 0;
                out->format = ok ? UMOE_FMT_WP12 : UMOE_FMT_WP16;
                if (!ok) why = WHY_WIDE_W12_OFF;
            }
            break;
        default: break;      // MOE_RAGGED, MOE_RIDERS, MOE_ROUTER: WP16
    }
    // 3. the layer holds it; and an fp8 engine decodes on its WP8 weights and nothing else: no silent fall-back to the bf16 copies it may
    //    have kept (a one-token prompt in the dense layout is refused like a decode step; every other prefill keeps the bf16 weights)
    const int need = out->format == UMOE_FMT_RM ? UMOE_HOLD_RM_EXP : out->format == UMOE_FMT_WP8 ? UMOE_HOLD_WP8 : out->format == UMOE_FMT_WP12 ? UMOE_HOLD_WP12 : UMOE_HOLD_BF16;
    const bool missing = !(h & need), fp8_rule = f.fp8 && (p.kind == UMOE_PASS_DECODE || dense) && out->format != UMOE_FMT_WP8;
    if (missing || fp8_rule) {
        plan_refusal_text(p, l, why, out->format, fp8_rule, missing, msg, msg_len);
        return -1;
    }
    return 0;
}
