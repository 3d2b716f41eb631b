/*
 * umoe.h -- C-ABI of libumoe_hip.so, the MI355X (gfx950) implementation of the
 * UniMoE-Audio hot path: DCMoE transformer forward + DAC-token decode loop.
 *
 * The reference (foggy-frost-forest/UniMoE-Audio) is 100% Python and has no FFI; this ABI
 * is what the repo's Python host modules (the .py files of unimoe_audio_amd, which mirror the reference
 * module API) bind with ctypes.  Each entry point cites the reference code it replaces
 * (paths relative to the reference root).  See INTEGRATION.md for the reference-side stub.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error (message: umoe_last_error()).
 *   - pointers are DEVICE pointers unless named host_*; nothing is allocated or freed
 *     behind the caller's back except inside umoe_engine_* (which owns its workspace).
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued, never synchronised.
 *   - bf16 tensors are uint16_t bit patterns; "T" means bf16 when `*_bf16` is 1 else fp32.
 *   - row-major everywhere; [S] tokens, [D] hidden, [E] = n_dyn + n_fix router columns.
 */
#ifndef UMOE_H
#define UMOE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* umoe_stream_t;

const char* umoe_last_error(void);
int umoe_abi_version(void);
/* sizeof of an argument struct of this header AS THE LIBRARY WAS BUILT ("umoe_router_args", "umoe_gemm_args", ...; 0 = unknown name).
 * Every struct here is passed by pointer and read whole, and they grow at the end between versions: a binding checks its mirrors
 * against this at load time (unimoe_audio_amd/_lib.py does) instead of letting a stale build read past a shorter struct. */
size_t umoe_struct_size(const char* name);

/* ------------------------------------------------------------------ weight layout
 * nn.Linear weights W[N][K] (bf16) are re-laid once at load time into the MFMA operand
 * order used by every weight-streaming kernel ("WP16"): 16-row x 32-col fragments of
 * v_mfma_f32_16x16x32_bf16, stored so that one wave-instruction reads 1 KiB contiguous.
 * K is split into 4 equal quarters, lane-group h = lane>>4 owns quarter h:
 *   packed[((nb*KB + i)*64 + lane)*8 + j] = W[nb*16 + (lane&15)][(lane>>4)*(K/4) + i*8 + j]
 * with KB = K/32, N padded up to a multiple of 16 with zero rows.  Requires K % 32 == 0.
 */
size_t umoe_packed_elems(int N, int K);
int umoe_pack_weight(const uint16_t* W, int N, int K, uint16_t* packed, umoe_stream_t stream);
/* gate_proj / up_proj of one SwiGLU expert interleaved per 16-row block (block 2i = gate i,
 * block 2i+1 = up i) so one wave produces silu(g)*u without a round trip.  N_packed = 2*I. */
int umoe_pack_gate_up(const uint16_t* Wg, const uint16_t* Wu, int I, int K, uint16_t* packed, umoe_stream_t stream);
/* FP8 expert weights ("WP8", the decode engine's opt-in weight-only fp8: umoe_engine_set_layer_fp8).  Elements are OCP float8_e4m3fn
 * q[N][K], one power-of-two scale 2^e per output row (int8 e), so that q * 2^e is exact in bf16.  One 16-byte lane load carries TWO
 * k-steps of the WP16 order:
 *   packed[((nb*KB2 + i)*64 + lane)*16 + j] = q[nb*16 + (lane&15)][(lane>>4)*(K/4) + 16*i + j]
 * with KB2 = ceil(KB/2), KB = K/32; bytes past the end of a K quarter (K/4 % 16 == 8, e.g. K = 1376) and padded rows are zero.
 * Exponents: 16 per block, exps[nb*16 + r] (0 for padded rows).  Gate/up blocks are interleaved as in umoe_pack_gate_up.  Packed on
 * the host side (unimoe_audio_amd/quant.py). */
/* bf16 expert weights in 12 bits, lossless ("WP12", the default of the flat expert launch: umoe_engine_set_layer_w12).  Same blocks,
 * lanes and K quarters as WP16; per lane and k-step the 8 LOW bytes raw and a 4-bit code of each HIGH byte (sign + exponent bits 7..1):
 * sign << 3 | (high & 0x7f) - base, with one window base per 16-row block (8 consecutive values, 16 binades).  Block nb takes KB * 768
 * bytes: the low bytes, then the code words.  CS = 2 k-steps per chunk when KB is even, else 1:
 *   low [((c*64 + lane)*CS + s)*8 + j] = low byte of WP16[((nb*KB + c*CS + s)*64 + lane)*8 + j]
 *   code[((c*64 + lane)*CS + s)*4 + b] = code of element (0,1,4,5)[b] | code of element (2,3,6,7)[b] << 4
 * so `c & 0x0f0f0f0f` and `(c >> 4) & 0x0f0f0f0f` hold four codes in byte lanes and one v_perm_b32 per operand dword joins high and
 * low bytes.  Block record: 40 u32 per block -- words 0..32 the exceptions (values whose high byte is outside the window: zeros,
 * denormals, inf / NaN, outliers), sorted by k-step, k-step << 25 | lane << 19 | element << 16 | bf16 bits, terminated and padded by
 * 0xffffffff; word 39 the window base.  At most 32 exceptions per block: a matrix with more is not packable and its layer runs the WP16
 * launch.  KB < 127.  Packed and unpacked on the host side (unimoe_audio_amd/w12.py). */

/* ------------------------------------------------------------------ router
 * Replaces utils/UniMoE_Audio_core.py:246-291,331-339 (gate GEMM, Top-P count :157-167,
 * sparse mixer :94-154 + driver loop :262-282, renormalise / padding / shared-on :284-291,
 * global weights :178-193) and the `router_weight * expert_mask` of :447.
 * Integer outputs are bit-exact w.r.t. oracle/router_oracle.c given identical logits.
 */
typedef struct {
    /* inputs: either (x, gate_w) or logits_in */
    const uint16_t* x;        /* [S][D] bf16 hidden states (post-norm unless norm_w given), or NULL */
    const uint16_t* gate_w;   /* [E][D] bf16, reference `gate.weight` */
    const uint16_t* norm_w;   /* optional [D]: fuse RMSNorm (model.py:240) in front of the gate */
    uint16_t* h_out;          /* optional [S][D]: normalised hidden states written for the experts */
    const void* logits_in;    /* optional [S][E] T: skip the gate GEMM (parity tests) */
    const uint8_t* attn_mask; /* optional [S] 0/1 padding mask (core.py:286-288) */
    int S, D;
    int n_dyn, n_real, n_fix; /* 9, 8, 2 */
    int logits_bf16;          /* 1: eval (bf16 gate, core.py:251); 0: fp32 gate (core.py:249) */
    float top_p;              /* 0 => fixed_top_k for every token (core.py:254-257) */
    int fixed_top_k;
    double jitter_eps;        /* router_jitter_noise */
    float rms_eps;
    /* outputs (any may be NULL except expert_mask / moe_w / slot tables) */
    void* logits_out;         /* [S][E] T */
    int64_t* top_k;           /* [S] */
    int32_t* sel;             /* [S][n_dyn] expert picked at round j, -1 beyond k */
    int32_t* expert_mask;     /* [S][E] */
    float* routing_w;         /* [S][n_dyn] T-rounded values held in fp32 */
    float* global_w;          /* [S][E]     T-rounded values held in fp32 */
    float* moe_w;             /* [S][n_real] = global_w * mask */
    int norm_only;            /* 1: only h_out = RMSNorm(x) with the router's own arithmetic (x, norm_w, h_out; S <= 256, D 2048 / 4096):
                               * the launch the decode engine puts in front of the expert GEMM when the router itself rides inside
                               * that GEMM's launch (umoe_gemm_args.fused_router) */
    /* training branch of the mixer (core.py:111-137; `training and not ignore_differentiable_router`), taken when `gumbel` is set:
     * round j selects arg-max(masked_gates + gumbel[s][j][:]) instead of the arg-max, and its weight is the softmax multiplier times
     * mask_for_one = 1 if (selected == arg-max of the softmaxed gates or rand_u[s][j] > 0.75) else 0.3333.  The noise is an INPUT
     * (the reference draws gumbel_rsample / torch.rand_like per call): the host supplies it, tests inject the reference's draws. */
    const float* gumbel;      /* optional [S][n_dyn][n_dyn] fp32 Gumbel(0,1) noise, round-major per token */
    const float* rand_u;      /* [S][n_dyn] fp32 uniform [0,1) draws, one per (token, round); required with gumbel */
    float* round_factor;      /* optional out [S][n_dyn]: mask_for_one of round j as 1 / 0.3333 (T-rounded), 0 beyond k; kept for
                               * umoe_router_bwd_ex (AudioMoERoutingFunction.backward, core.py:64-91) */
    /* training-time input jitter with the fp32 gate (core.py:240-249: `hidden_states.float()` times U(1-eps, 1+eps) noise, then the
     * fp32 gate GEMM): the gate sees float(x[s][d]) * x_noise[s][d] with NO rounding to bf16 in between.  The noise is an INPUT like
     * the mixer's.  Needs x / gate_w, excludes norm_w / h_out / logits_in. */
    const float* x_noise;     /* optional [S][D] fp32 */
} umoe_router_args;
int umoe_router_fwd(const umoe_router_args* a, umoe_stream_t stream);

/* aux load-balancing loss (core.py:361-389): n_dyn * sum_e mean_s(mask) * mean_s(softmax(masked logits)); token_weight
 * (optional [S]) = aux_balance_weight expanded per token (core.py:380-385).  out = one fp32 scalar. */
int umoe_aux_loss_fwd(const void* logits, int logits_bf16, const int32_t* expert_mask, const float* token_weight, int S, int E,
                      int n_dyn, float* out, umoe_stream_t stream);
/* the same result from two launches (64 workgroups over contiguous token ranges, fixed-order partial sums in `ws`, then one small
 * workgroup): for many tokens (training).  ws: umoe_aux_loss_workspace_floats() floats, caller-owned.  Sums are re-associated, so
 * the value can differ from umoe_aux_loss_fwd in the last bits. */
int umoe_aux_loss_fwd_ws(const void* logits, int logits_bf16, const int32_t* expert_mask, const float* token_weight, int S, int E,
                         int n_dyn, float* out, float* ws, umoe_stream_t stream);
size_t umoe_aux_loss_workspace_floats(void);

/* Token drop (core.py:302-329; `capacity` = _audio_expert_capacity, core.py:170-175, computed by the host in the reference's
 * float32 arithmetic).  policy 0 "probs": per dynamic column keep the `capacity` selected tokens with the largest logits (the
 * reference's topk(dim=0) over the column, :305-314; shared columns untouched); policy 1 "position": keep the first `capacity`
 * selected tokens of EVERY column in token order (:321-323; the reference's cumsum runs over the shared columns too).  Dropped
 * entries leave routing_w, which is renormalised (:328-329); global_w / moe_w are recomputed over the kept columns (:178-193) with
 * the router's arithmetic.  Ties at the capacity boundary keep the lowest token indices (torch.topk leaves them unspecified).
 * Integer outputs are bit-exact w.r.t. the reference wherever the boundary is not tied. */
int umoe_token_drop(const void* logits, int logits_bf16, const int32_t* expert_mask_in, const float* routing_w_in, int S, int n_dyn,
                    int n_real, int n_fix, int capacity, int policy, int32_t* expert_mask_out, float* routing_w_out, float* global_w,
                    float* moe_w, umoe_stream_t stream);

/* Ragged dispatch tables from the 0/1 mask: the build's replacement for the dense
 * compress_matrix / decompress_matrix pair (utils/UniMoE_Audio_utils.py:436-523) and the
 * capacity MAX of core.py:455-457.  Wavefront ballot + prefix sums, token order preserved.
 *   counts[n_real], offsets[n_real+1], slot_token[S*n_real], slot_of[S][n_real] (-1 = unrouted) */
int umoe_dispatch_build(const int32_t* expert_mask, int S, int ld_mask, int n_real, int32_t* counts,
                        int32_t* offsets, int32_t* slot_token, int32_t* slot_of, umoe_stream_t stream);
/* same tables with every expert's slot range starting on a multiple of `align` (power of two): offsets[e] % align == 0,
 * offsets[n_real] = padded total, padding slots carry token 0 and are not counted.  slot_token needs
 * S*n_real + n_real*(align-1) entries.  Used by training: the weight-gradient GEMMs contract over slot columns of
 * transposed buffers in 16-byte chunks. */
int umoe_dispatch_build_aligned(const int32_t* expert_mask, int S, int ld_mask, int n_real, int align, int32_t* counts,
                                int32_t* offsets, int32_t* slot_token, int32_t* slot_of, umoe_stream_t stream);

/* router + dispatch tables in one call: a single fused launch when S <= 16 (decode), two launches otherwise */
int umoe_router_dispatch_fwd(const umoe_router_args* a, int32_t* counts, int32_t* offsets, int32_t* slot_token,
                             int32_t* slot_of, umoe_stream_t stream);

/* permute: out[slot] = x[slot_token[slot]]  (the gather half of compress_matrix);
 * bwd of unpermute.  rows = offsets[n_real] read on device. */
int umoe_permute_fwd(const uint16_t* x, int D, const int32_t* slot_token, const int32_t* total_slots, int max_slots,
                     uint16_t* out, umoe_stream_t stream);

/* ------------------------------------------------------------------ grouped weight-streaming GEMM
 * One launch covers any number of groups (routed experts with ragged row lists, shared
 * experts with all rows, plain dense layers with one group).
 */
typedef struct {
    const uint16_t* w;        /* WP16-packed weights of this group */
    const float* bias;        /* optional [N] fp32 */
    const int32_t* rows;      /* optional gather list (token index per row); NULL = identity */
    const int32_t* row_off;   /* optional device scalar added to the row number (offsets[e]) */
    const int32_t* count;     /* optional device scalar: number of rows; NULL => static_count */
    int static_count;
    int a_row_base;           /* identity mode: A row = a_row_base + r */
    int out_row_base;         /* output row = out_row_base + (row_off ? *row_off : 0) + r */
    int n_blocks;             /* N/16 (2*I/16 for gate/up pairs) */
    int k;                    /* K */
    int a_col_off;            /* element offset added to every A row of this group (EP receive buffers) */
    int reserved;
} umoe_group_t;

enum { UMOE_PRO_PLAIN = 0, UMOE_PRO_RMSNORM = 1 };
enum {
    UMOE_EPI_BF16 = 0,      /* y = bf16(acc + bias) */
    UMOE_EPI_BF16_RESID = 1, /* y = bf16(resid + bf16(acc + bias)) */
    UMOE_EPI_SWIGLU = 2,     /* pairs: y = bf16(bf16(silu(bf16 g)) * bf16 u)   core.py:31,49 */
    UMOE_EPI_F32 = 3,        /* y = float(bf16(acc))   (codec_head(...).float(), model.py:982) */
    UMOE_EPI_F32_RAW = 4     /* y = acc (fp32, unrounded) */
};

typedef struct {
    const umoe_group_t* groups; /* device array */
    int num_groups;
    int max_rows;             /* upper bound of rows per group (grid sizing; no host sync) */
    int max_n_blocks;         /* max over groups */
    int max_k;
    const uint16_t* a;        /* [*, lda] bf16 activations */
    int lda;
    const uint16_t* norm_w;   /* UMOE_PRO_RMSNORM: [K] */
    float rms_eps;
    const uint16_t* resid;    /* UMOE_EPI_BF16_RESID: [*, ldo] */
    void* out;                /* bf16 or fp32 [*, ldo] */
    int ldo;
    int n_valid;              /* columns >= n_valid are not stored (N not multiple of 16) */
    int prologue, epilogue;
    int nt;                   /* n-blocks per workgroup: 0 = auto, else 1/2/4/5/6/8, SwiGLU also 14 (tuning knob) */
    int waves;                /* waves per workgroup: 0 = auto, 4, 8 (8 only with nt = 8; tuning knob) */
    int ksplit;               /* >1 (<= 4): K split over workgroups; needs UMOE_EPI_F32_RAW: slab s at out + s*part_stride holds the
                               * product over k-steps [KB*s/ksplit, KB*(s+1)/ksplit) of every K quarter (KB = K/32; a slice of no
                               * steps stores exact zeros).  A group's bias is added in slab 0 ONLY, so the sum of the slabs is
                               * acc + bias */
    long part_stride;         /* elements between fp32 partial slabs */
    const umoe_group_t* groups_host; /* optional HOST copy of `groups`: with num_groups <= UMOE_GROUPS_INLINE the
                               * descriptors travel in the kernel arguments (one dependent HBM round trip less per launch) */
    int cache_policy;         /* reserved (0): the weight stream is always non-temporal -- a default-policy variant and an
                               * Infinity Cache warm-up were measured and bought nothing */
    const umoe_router_args* fused_router; /* optional HOST pointer (SwiGLU, nt = 14, <= 16 rows, n_dyn 9 / n_fix 2, D 2048 / 4096, S <= 16):
                               * the router of these tokens runs INSIDE this launch as S extra workgroups (its outputs are complete when
                               * the launch is); the GEMM itself must not depend on them (dense-expert decode: h_out NULL, see norm_only) */
    const void* rider_pub;    /* decode engine only, with fused_router: HOST pointer to the hand-off descriptor (epoch and error words) of
                               * the flat expert launch, which takes these arguments; umoe_grouped_gemm refuses anything but NULL */
} umoe_gemm_args;
#define UMOE_GROUPS_INLINE 12

/* Warm the Infinity Cache (256 MiB, memory side) with `bytes` at `p`: plain loads, nothing stored.  `wgs` workgroups of 256
 * threads, 8 x 16 B per thread in flight.  Used to pull the next weight-streaming kernel's first bytes out of HBM while
 * a latency-bound kernel leaves the memory idle. */
int umoe_prefetch(const void* p, size_t bytes, int wgs, umoe_stream_t stream);
int umoe_grouped_gemm(const umoe_gemm_args* a, umoe_stream_t stream);

/* ------------------------------------------------------------------ wide decode GEMM (17..64 rows, every weight streamed once)
 * Y[tile t][16, N(g)] = epilogue(A[tile t][16, K(g)] * W_g^T) for tiles = ceil(rows / 16) in {2, 3, 4}: one pass over the WP16 weights of
 * every group serves all row tiles (umoe_grouped_gemm re-reads a weight per 16-row tile).  The activations come as operand-order tiles
 * (umoe_pack_rows; WP16 of a [16][K] matrix, tile t of group g at host_b[g] + t * 16 * K(g), pad rows zero).  The K split over the
 * `waves` waves of a workgroup and the reduction order are those of the 16-row kernel with `u`-step chunks, so a (row, feature) product
 * is bit-identical to the one umoe_grouped_gemm computes for a 16-row tile with the same (waves, u).  One (epilogue, waves, u) triple per
 * GEMM of the decode step; anything else is refused:
 *   UMOE_EPI_BF16 (+ host_bias), 4, 16      QKV          UMOE_EPI_BF16_RESID (+ host_resid), 4, 16    o_proj
 *   UMOE_EPI_SWIGLU, 8, 1                   gate/up      UMOE_EPI_BF16, 8, 2                          down
 *   UMOE_EPI_F32, 4, 16 | 8 | 2             codec head (the 16-row launch's split by block count: < 512, < 1024, more)
 * host_* are HOST arrays of num_groups (<= 12) entries; groups may differ in n_blocks and K.  Row-major outputs: host_out[g] is
 * [rows][ldo] (bf16, fp32 for UMOE_EPI_F32), columns >= min(n_valid, 16 n_blocks(g)) and pad rows are not stored, ldo % 4 == 0.  UMOE_EPI_SWIGLU: host_out[g]
 * receives the tiles of silu(g) * u in operand order, [tiles][16 * I(g)], I = 8 * n_blocks (n_blocks % 4 == 0), pad rows included (zero
 * rows in, zero rows out): the input of the down projection.  host_bias / host_resid may be NULL, or hold NULL entries (bias).  Weights, input tiles, outputs and
 * residuals are 16-byte aligned. */
int umoe_gemm_wide(const uint16_t* const* host_w, const int* host_n_blocks, const int* host_k, int num_groups, int rows,
                   const uint16_t* const* host_b, void* const* host_out, int ldo, int n_valid, const float* const* host_bias,
                   const uint16_t* const* host_resid, int epilogue, int waves, int u, umoe_stream_t stream);
/* The gate/up and the down launch of the wide step on WP8 weights (above): host_w8[g] holds the WP8 blocks of group g, host_exps[g] their
 * row exponents (16 per block), everything else is umoe_gemm_wide's -- tiles, K split, reduction order, epilogue, operand-order tiles in
 * and (SwiGLU) out.  The e4m3 bytes are converted to the bf16 MFMA operand with the row's 2^e right in front of the MFMAs, so every output
 * is bit-identical to umoe_gemm_wide on the dequantized weights q * 2^e.  Accepts exactly (UMOE_EPI_SWIGLU, 8, 1) and (UMOE_EPI_BF16, 8, 2);
 * no bias, no residual.  A group with an even K / 32 streams 16-byte lane loads of two k-steps, one with an odd K / 32 (u = 2 only) one
 * 8-byte load per k-step; groups of both kinds may share a launch.  The gate/up launch (u = 1) needs K % 512 == 0, the K at which its
 * wave slices are whole 16-byte chunks: no padded k-step is ever computed.  Weights, input tiles and outputs are 16-byte aligned. */
int umoe_gemm_wide_fp8(const uint8_t* const* host_w8, const int8_t* const* host_exps, const int* host_n_blocks, const int* host_k,
                       int num_groups, int rows, const uint16_t* const* host_b, void* const* host_out, int ldo, int n_valid,
                       int epilogue, int waves, int u, umoe_stream_t stream);
/* The gate/up and the down launch of the wide step on WP12 weights (above, "WP12": the bf16 bits in 12 bits per weight): host_w12[g] holds
 * the WP12 blocks of group g (K / 32 * 768 bytes per 16-row block, gate/up blocks interleaved as in umoe_pack_gate_up), host_meta[g] their
 * block records (40 u32 per block); everything else is umoe_gemm_wide's -- tiles, K split, reduction order, epilogue, operand-order tiles in
 * and (SwiGLU) out.  A lane rebuilds the WP16 operand of a (block, k-step) once, in front of the MFMAs of all row tiles, so every output
 * is bit-identical to umoe_gemm_wide on the WP16 weights the blocks were packed from.  Accepts exactly (UMOE_EPI_SWIGLU, 8, 1) and
 * (UMOE_EPI_BF16, 8, 2); no bias, no residual; 17..64 rows.  A group with an even K / 32 streams 2-step chunks (16 low bytes + 8 code bytes
 * per lane), one with an odd K / 32 (u = 2 only) 1-step chunks (8 + 4), as the packer lays them; groups of both kinds may share a launch.
 * K % 32 == 0, K / 32 < 127; the gate/up launch (u = 1) needs K % 512 == 0 (every wave slice whole chunks) and n_blocks % 4 == 0.
 * Weights, input tiles and outputs are 16-byte aligned, records 4-byte aligned.  Anything else is refused with nothing launched. */
int umoe_gemm_wide_w12(const uint8_t* const* host_w12, const uint32_t* const* host_meta, const int* host_n_blocks, const int* host_k,
                       int num_groups, int rows, const uint16_t* const* host_b, void* const* host_out, int ldo, int n_valid,
                       int epilogue, int waves, int u, umoe_stream_t stream);
/* rows [rows][lda] (row-major, the first k columns) -> operand-order tiles for umoe_gemm_wide: packed holds ceil(rows / 16) * 16 * k
 * elements, pad rows of the last tile are written as zeros and their source is not read.  norm_w != NULL (k 2048 / 4096): RMSNorm in
 * front, values bit-identical to umoe_router_fwd(norm_only).  x, packed and norm_w are 16-byte aligned, lda % 8 == 0. */
int umoe_pack_rows(const uint16_t* x, int lda, int rows, int k, const uint16_t* norm_w, float rms_eps, uint16_t* packed,
                   umoe_stream_t stream);

/* ------------------------------------------------------------------ tiled MFMA GEMM (prefill / training shapes)
 * Y[rows(g), N(g)] = epilogue( A[rows(g), K] * W_g^T ) with W_g ROW-MAJOR [N][K] bf16 (the reference's nn.Linear layout,
 * core.py:21-28,39-46; no packing: training updates these tensors every step).  Compute-bound counterpart of
 * umoe_grouped_gemm: 128x128x64 tiles through LDS, v_mfma_f32_16x16x32_bf16, fp32 accumulation, the same ragged-group
 * conventions (gather list / device-side count and offset) and the same rounding points in the epilogues.
 * UMOE_EPI_SWIGLU takes gate rows from `w` and up rows from `w2` (N = intermediate size). */
typedef struct {
    const uint16_t* w;        /* [N][ldw] row-major */
    const uint16_t* w2;       /* SwiGLU only: up_proj [N][ldw] */
    const float* bias;        /* optional [N] fp32 */
    const int32_t* rows;      /* optional gather list; NULL = identity */
    const int32_t* row_off;   /* optional device scalar added to the row number */
    const int32_t* count;     /* optional device scalar: rows of this group; NULL => static_count */
    int static_count;
    int a_row_base, out_row_base;
    int n, k, ldw;            /* output features, contraction length (k % 8 == 0), elements between weight rows */
    int a_col_off;
    const int32_t* k_off;     /* optional device scalars: contract over columns [*k_off, *k_off + roundup8(*k_count)) of BOTH */
    const int32_t* k_count;   /* operands instead of [0, k) -- weight gradients over one expert's (8-aligned) slot range */
    int out_col_off;          /* element offset added to every output row of this group (attention heads side by side) */
    int k_compact_a;          /* with k_off / k_count: > 0 = the activation operand is laid out in per-group COMPACT blocks (what
                               * umoe_transpose_slots_compact writes): this group's block starts at element *k_off * k_compact_a (the
                               * operand's total row count) and its rows are roundup8(*k_count) apart, columns [0, roundup8(*k_count)) */
    int k_compact_w;          /* the same for the weight operand (total rows of `w`) */
    int w_kmajor;             /* != 0: `w` is row-major [K][ldw] with the CONTRACTION index as its row and n columns (Y = A W): the input
                               * gradient dX = dY W on an nn.Linear weight as stored, no transposed copy.  UMOE_EPI_BF16 only, every group of
                               * the launch alike, n % 8 == 0, no bias / K window; the launch runs whatever its size on 256 x 256 tiles */
    int k_w1;                 /* w_kmajor with w2 != NULL: rows [0, k_w1) of the contraction come from w, rows [k_w1, k) from w2 (same ldw, */
                              /* k_w1 % 32 == 0): (dG | dU) against Wg then Wu */
} umoe_tgroup_t;

typedef struct {
    const umoe_tgroup_t* groups;  /* HOST array (descriptors travel in the kernel arguments), num_groups <= 12 */
    int num_groups;
    int max_rows;             /* upper bound of rows in any group (grid sizing) */
    const uint16_t* a;        /* [*, lda] bf16 */
    int lda;
    const uint16_t* resid;    /* UMOE_EPI_BF16_RESID: [*, ldo] */
    void* out;                /* bf16 (or fp32 for UMOE_EPI_F32 / _RAW) [*, ldo] */
    int ldo;
    int epilogue;             /* UMOE_EPI_* */
    uint16_t* aux_out;        /* UMOE_EPI_SWIGLU with aux_out != NULL (training): also store the bf16 pre-activations, */
    int ld_aux;               /* gate at aux_out[row][col], up at aux_out[row][n + col] (what autograd would save) */
} umoe_tgemm_args;
int umoe_tiled_gemm(const umoe_tgemm_args* a, umoe_stream_t stream);
/* The same GEMM on WP8 weights (above; prefill of an engine that holds its experts as e4m3 only): host_w8[g] holds the WP8 blocks of
 * group g's weight [n][k] and host_exps[g] their row exponents (16 per block); with UMOE_EPI_SWIGLU host_w8[g] is the interleaved
 * gate/up pair (n = intermediate size, n % 16 == 0) and serves gate and up.  The groups' w / w2 / ldw are not read.  tgemm_kernel's
 * register-staging form with the e4m3 granules converted on their way into the LDS image, everything behind it shared: every output is
 * bit-identical to umoe_tiled_gemm's small-tile kernel on the dequantized weights q * 2^e (128- and 256-token tiles by the same rule;
 * there is no 256 x 256 ping-pong form).  UMOE_EPI_SWIGLU (no aux_out) and UMOE_EPI_BF16; gather list, device-side count and row offset
 * as umoe_tiled_gemm; k % 32 == 0.  Refused: w_kmajor, K windows (k_off / k_count / k_compact_*), bias, the other epilogues. */
int umoe_tiled_gemm_wp8(const umoe_tgemm_args* a, const uint8_t* const* host_w8, const int8_t* const* host_exps, umoe_stream_t stream);
/* The same GEMM on WP12 weights ("WP12" below; prefill of an engine that holds its bf16 experts as the lossless 12-bit copies only):
 * host_w12[g] holds the WP12 blocks of group g's weight [n][k] (16-byte aligned) and host_meta[g] their block records (40 words per
 * block, 4-byte aligned); with UMOE_EPI_SWIGLU host_w12[g] is the interleaved gate/up pair (n = intermediate size, n % 16 == 0) and
 * serves gate and up.  The groups' w / w2 / ldw are not read.  tgemm_kernel's register-staging form with the granules rebuilt on their
 * way into the LDS image and the blocks' exceptions patched into it, everything behind it shared: every output is bit-identical to
 * umoe_tiled_gemm's small-tile kernel on the row-major weights (128- and 256-token tiles by the same rule; no ping-pong form).
 * UMOE_EPI_SWIGLU (no aux_out) and UMOE_EPI_BF16; gather list, device-side count and row offset as umoe_tiled_gemm; k % 32 == 0,
 * k / 32 < 127.  Refused: w_kmajor, K windows (k_off / k_count / k_compact_*), bias, the other epilogues. */
int umoe_tiled_gemm_w12(const umoe_tgemm_args* a, const uint8_t* const* host_w12, const uint32_t* const* host_meta, umoe_stream_t stream);

/* Weight-gradient form of the tiled GEMM: both operands are row-major with the CONTRACTION index as the row (tokens / expert slots), as
 * autograd holds activations and their gradients -- dW = dY^T X without transposed copies (torch.nn.functional.linear backward,
 * core.py:21-49 through the expert MLPs and every nn.Linear of model.py:672-871):
 *   out_g[m][n] = sum over k in the group's window of  P[k][p_col_off + m] * Q[k][q_col_off + n]      (bf16 in, fp32 sum, bf16 out)
 * The window is static (k_off, k) or read on the device (k_off_dev / k_count_dev: an expert's slot range from
 * umoe_dispatch_build_aligned).  k_split > 1 (static windows, groups that tile one dense [rows][ldo] output with n == ldo): the window is
 * cut into k_split parts whose fp32 partial outputs (ws, part_stride floats apart, umoe_tiled_gemm_tn_workspace_bytes) are summed in
 * fixed order -- for products with too few 256 x 256 output tiles to fill the chip. */
typedef struct {
    const uint16_t* p; int ldp;   /* optional per-group operands (NULL: the launch's) */
    const uint16_t* q; int ldq;
    void* out;                    /* optional per-group output base (NULL: the launch's) */
    int p_col_off, q_col_off;     /* column of P that is output row 0 / column of Q that is output column 0 (multiples of 8) */
    int m, n;                     /* output rows / columns (multiples of 8) */
    int k_off, k;                 /* static window [k_off, k_off + k) */
    const int32_t* k_off_dev;     /* device scalars, both or neither */
    const int32_t* k_count_dev;
    int out_row_base, out_col_off;
} umoe_tn_group_t;
typedef struct {
    const umoe_tn_group_t* groups;   /* HOST array, num_groups <= 24 */
    int num_groups;
    const uint16_t* p; int ldp;      /* [rows][ldp] bf16: its columns become output ROWS */
    const uint16_t* q; int ldq;      /* [rows][ldq] bf16: its columns become output COLUMNS */
    void* out; int ldo;              /* bf16 [*, ldo] (umoe_tiled_gemm_tn_acc: fp32 [*, ldo], 16-byte aligned) */
    int k_split;                     /* 0 / 1: none; > 1: that many parts; < 0: chosen by the library (1..8, from the tile count and K) */
    void* ws; long part_stride;      /* k_split > 1 or < 0: fp32 workspace (umoe_tiled_gemm_tn_workspace_bytes), part_stride = rows * ldo of the output */
} umoe_tgemm_tn_args;
size_t umoe_tiled_gemm_tn_workspace_bytes(const umoe_tgemm_tn_args* a);
int umoe_tiled_gemm_tn_split(const umoe_tgemm_tn_args* a);      /* the K split the call would use (k_split < 0: the library's choice) */
int umoe_tiled_gemm_tn(const umoe_tgemm_tn_args* a, umoe_stream_t stream);
/* Accumulate form (fp32 main gradients): the same arguments and structs, but `out` and every group's `out` are FP32, 16-byte
 * aligned, and every element umoe_tiled_gemm_tn would store becomes out = out + sum (one fp32 add on the unrounded fp32 sum).  Rows at or
 * beyond m and columns at or beyond n are neither read nor written.  No K split: the tile's owner loads its float4, adds and stores -- no
 * atomics, bitwise reproducible.  K split (same rule and workspace): s = part 0 + part 1 + ... in the bf16 entry's order, then
 * out = out + s -- s has the bits the bf16 entry rounds.  A group whose window is empty (device k_count 0: an expert no token reached)
 * leaves its output bit for bit as it was.  Refusals: those of umoe_tiled_gemm_tn, and an fp32 output that is not 16-byte aligned;
 * a refused call enqueues nothing. */
int umoe_tiled_gemm_tn_acc(const umoe_tgemm_tn_args* a, umoe_stream_t stream);

/* Named wrappers required by the scope table; thin calls of umoe_grouped_gemm.
 * umoe_grouped_swiglu_fwd: routed experts, core.py:406-416 + :34-49 on ragged rows.
 * umoe_shared_swiglu_fwd : shared experts, core.py:344-351 + :16-31. */
int umoe_grouped_swiglu_fwd(const umoe_group_t* gateup_groups, const umoe_group_t* down_groups, int num_groups,
                            int max_rows, const uint16_t* x, int D, int I, uint16_t* h_ws, uint16_t* y_slots,
                            umoe_stream_t stream);

int umoe_shared_swiglu_fwd(const umoe_group_t* gateup_groups, const umoe_group_t* down_groups, int n_fix, int S,
                           const uint16_t* x, int D, int I, uint16_t* h_ws, uint16_t* y_shared, umoe_stream_t stream);

/* combine: out[s] = resid[s] + ( sum_e moe_w[s][e] * y[slot_of[s][e]]  (+ shared_i[s] * global_w[s][n_dyn+i]) )
 * with the reference's rounding points (einsum core.py:488, adds :342,:351, residual model.py:242). */
typedef struct {
    const uint16_t* y_slots;  /* [slots][D] routed expert outputs (bf16), or NULL when y_parts is used */
    const int32_t* slot_of;   /* [S][n_real] */
    const float* moe_w;       /* [S][n_real] */
    const uint16_t* y_shared; /* [n_fix][S][D] or NULL */
    const float* global_w;    /* [S][E] */
    const uint16_t* resid;    /* [S][D] or NULL */
    uint16_t* out;            /* [S][D] */
    int S, D, n_real, n_dyn, n_fix;
    const float* y_parts;     /* optional fp32 partial slabs [n_parts][rows][D] of a K-split down GEMM: y = bf16(sum) */
    int n_parts;
    long part_stride;
    int shared_row0;          /* >= 0: the shared experts' rows live in the slabs too, at shared_row0 + i*S + s */
    const uint16_t* norm_w;   /* optional [D]: also write norm_out = RMSNorm(out) * norm_w (next layer's input norm) */
    uint16_t* norm_out;       /* [S][D] */
    float rms_eps;
    const int32_t* expert_mask; /* dense-expert layout (slot_of == NULL): expert e's output row of token s is e*dense_rows + s, */
    int mask_ld, dense_rows;    /* used iff expert_mask[s*mask_ld + e] != 0 (every expert computed all rows; decode, S <= 16) */
    const void* ep_xfer;        /* decode engine only (NULL otherwise): HOST pointer to the exchange descriptor of an expert-parallel
                                 * step -- y_slots is then this rank's return slab and the kernel waits for the peers' rows itself */
} umoe_combine_args;
int umoe_unpermute_combine_fwd(const umoe_combine_args* a, umoe_stream_t stream);

/* ------------------------------------------------------------------ expert-parallel exchange (RCCL over xGMI)
 * The all-to-all of DeepSpeed's _AllToAll in the reference (core.py:467,480; utils.py:332-335).  `comm` is an opaque
 * ncclComm_t; librccl is resolved at first use.  Every rank exchanges slabs of equal size (fixed per-destination capacity
 * of unimoe_audio_amd/ep.py): send + p*bytes goes to peer p, peer p's slab lands at recv + p*bytes; enqueued on `stream`.
 * umoe_ep_unique_id (rank 0, 128 bytes to broadcast out of band) + umoe_ep_comm_create build a communicator where the
 * caller has none to pass in. */
int umoe_ep_unique_id(void* out128);
int umoe_ep_comm_create(const void* uid128, int rank, int nranks, void** comm_out);
int umoe_ep_comm_destroy(void* comm);
int umoe_ep_all_to_all(void* comm, const void* send, void* recv, size_t bytes_per_peer, int nranks, umoe_stream_t stream);

/* Peer exchange of the expert-parallel DECODE engine (umoe_engine_cfg.ep_size > 1): xGMI peer stores inside the captured step
 * graph instead of a collective call.  Every rank owns one exchange REGION (uncached device memory: flags + the dispatch slab
 * [ep][rows][D] + the return slab [n_real][rows][D]); ranks map each other's regions through HIP IPC handles once, at connect
 * time.  Per layer: rank r pushes its normalised rows into tile r of every peer's dispatch slab (the DENSE form of the
 * reference's first all-to-all, core.py:467: at <= 16 rows per rank every expert is hit anyway, so every rank receives every
 * row and the routing result is only needed by the combine), computes its local experts on all ep*rows rows, and pushes the
 * outputs for rank t's rows into the return slab of rank t (second all-to-all, core.py:480).  Payload and flags are
 * system-scope write-through stores (sc0 sc1), drained per wave before ONE lane publishes the epoch; receivers poll with
 * system-scope loads (bounded spin: a timeout sets the engine's error word, see umoe_engine_ep_error) and copy the slab into
 * ordinary device memory for the GEMMs.  Epoch = decode step * layers + layer + 1, counted on the device: graph replays need
 * no host value.  All ranks must run the same sequence of decode steps. */
#define UMOE_MAX_EP 8
int umoe_ep_ipc_export(const void* dev_ptr, void* handle64_out);      /* hipIpcGetMemHandle: 64 opaque bytes */
int umoe_ep_ipc_open(const void* handle64, void** dev_ptr_out);       /* hipIpcOpenMemHandle (lazy peer access) */
int umoe_ep_ipc_close(void* dev_ptr);

/* ------------------------------------------------------------------ backward pieces (training, BASELINE config 3)
 * The contractions run on umoe_tiled_gemm (operands K-contiguous): dX = dY * W uses a transposed weight copy, dW = dY^T X
 * contracts over the slot columns of transposed, 8-aligned, zero-padded buffers built by umoe_transpose_slots
 * (umoe_dispatch_build_aligned + umoe_tgroup_t.k_off / k_count).  Everything below is per-token / elementwise. */

/* dst[c][off_g + r] = src[row(off_g + r)][c], r < counts[g]; zeros up to the next multiple of 8.  row(s) = rows ? rows[s] : s.
 * counts/offsets NULL: one group of max_rows rows at offset 0 (plain transpose).  Replaces autograd's implicit
 * transposes in Linear.backward (core.py:21-49 via torch.nn.functional.linear). */
int umoe_transpose_slots(const uint16_t* src, int ld_src, int C, const int32_t* rows, const int32_t* counts,
                         const int32_t* offsets, int n_groups, int max_rows, uint16_t* dst, int ld_dst, umoe_stream_t stream);
/* the same transpose into per-group COMPACT blocks: group g's block starts at dst + offsets[g] * C and holds C rows of roundup8(counts[g])
 * elements (zero padded) -- a weight-gradient product then walks rows 5.6 KB apart instead of 50 KB (umoe_tgroup_t.k_compact_*).
 * counts / offsets required; dst needs (sum of roundup8 counts) * C elements. */
int umoe_transpose_slots_compact(const uint16_t* src, int ld_src, int C, const int32_t* rows, const int32_t* counts,
                                 const int32_t* offsets, int n_groups, int max_rows, uint16_t* dst, umoe_stream_t stream);

/* SwiGLU backward, core.py:31,49: gu [rows][2I] = (gate | up) pre-activations saved by the forward
 * (umoe_tgemm_args.aux_out), dh [rows][I] -> dgu [rows][2I] = (dgate | dup).  total_rows: device scalar or NULL. */
/* y[i] = bf16(float(x[i]) * noise[i]): the training-time input jitter on the gate's copy of the rows (core.py:240-244: the reference
 * multiplies a float copy and casts back) in one pass instead of three elementwise launches.  n % 8 == 0; n == 0: the pointers may be null. */
int umoe_mul_noise(const uint16_t* x, const float* noise, long n, uint16_t* y, umoe_stream_t stream);
int umoe_swiglu_bwd(const uint16_t* dh, int ld_dh, const uint16_t* gu, int ld_gu, int I, const int32_t* total_rows,
                    int max_rows, uint16_t* dgu, int ld_dgu, umoe_stream_t stream);

/* backward of umoe_unpermute_combine_fwd (einsum core.py:488, shared adds :349-351): per selected (token, expert)
 * dy[slot] = bf16(w * dout[s]) and d_moe_w[s][e] = <dout[s], y[slot]>; same for the shared experts with global_w. */
int umoe_unpermute_combine_bwd(const uint16_t* dout, const umoe_combine_args* a, uint16_t* dy_slots, uint16_t* dy_shared,
                               float* d_moe_w, float* d_gw_shared, umoe_stream_t stream);

/* backward of the dispatch gather (compress_matrix, utils.py:436-485): dx[s] = sum of the slot rows of token s
 * (+ the shared experts' input gradients [n_fix][S][D], + an optional extra [S][D] term), fp32 accumulate, one rounding. */
int umoe_permute_bwd(const uint16_t* dxe, const int32_t* slot_of, int n_real, const uint16_t* dx_shared, int n_fix, int S, int D,
                     const uint16_t* extra, uint16_t* dx, umoe_stream_t stream);

/* router backward, shipped configuration (ignore_differentiable_router, core.py:272): d(moe_w), d(shared global weights)
 * -> d_logits [S][E] fp32 through the per-round softmax multipliers (core.py:115-119), the renormalisation (:284) and the
 * global softmax (:178-193).  sel / top_k / expert_mask are the forward's integer outputs; d_logits_in is added (aux loss). */
int umoe_router_bwd(const void* logits, int logits_bf16, const int32_t* sel, const int64_t* top_k, const int32_t* expert_mask,
                    const float* d_moe_w, const float* d_gw_shared, const float* d_logits_in, int S, int n_dyn, int n_real,
                    int n_fix, double jitter_eps, float* d_logits, umoe_stream_t stream);
/* general form: token_drop as in umoe_router_bwd_drop; round_factor (optional [S][n_dyn], umoe_router_args.round_factor) = the
 * differentiable-router training branch: the forward weights carry mask_for_one, the gradient is AudioMoERoutingFunction.backward
 * (core.py:64-91: grad * multiplier * (onehot(selected) - masked_gates), mask_for_one not differentiated) */
int umoe_router_bwd_ex(const void* logits, int logits_bf16, const int32_t* sel, const int64_t* top_k, const int32_t* expert_mask,
                       const float* d_moe_w, const float* d_gw_shared, const float* d_logits_in, int S, int n_dyn, int n_real,
                       int n_fix, double jitter_eps, int token_drop, const float* round_factor, float* d_logits, umoe_stream_t stream);
/* the same with the token-drop branch in the graph (core.py:328-329): `expert_mask` is then the mask AFTER the drop and the routing
 * weights pass through r2 = (r * mask) / (sum(r * mask) + 1e-6) before the global weights */
int umoe_router_bwd_drop(const void* logits, int logits_bf16, const int32_t* sel, const int64_t* top_k, const int32_t* expert_mask,
                         const float* d_moe_w, const float* d_gw_shared, const float* d_logits_in, int S, int n_dyn, int n_real,
                         int n_fix, double jitter_eps, float* d_logits, umoe_stream_t stream);

/* Backward of the expert MLPs down(silu(gate x) * up x), core.py:16-49,406-416, over up to 12 groups per call:
 *   dH = dY Wd ; (dG | dU) = SwiGLU'(G, U, dH) ; dX_slots = dG Wg + dU Wu ; dWd = dY^T H ; dWg = dG^T X ; dWu = dU^T X.
 * umoe_grouped_swiglu_bwd: routed experts, ragged rows (counts/offsets from umoe_dispatch_build_aligned with align 8,
 * slot_token = gather list of x).  umoe_shared_swiglu_bwd: shared experts, counts/offsets NULL, group g owns slot rows
 * [row_base + g*max_rows, +max_rows) (both multiples of 8) and reads x by identity.  All weights row-major (nn.Linear). */
typedef struct {
    int num_groups;
    const uint16_t* const* w_gate;   /* host arrays [num_groups] of device pointers: [I][D], [I][D], [D][I] */
    const uint16_t* const* w_up;
    const uint16_t* const* w_down;
    int D, I;
    const int32_t* counts;           /* device [num_groups] or NULL */
    const int32_t* offsets;          /* device [num_groups + 1] (8-aligned, last = padded total) or NULL */
    const int32_t* slot_token;       /* device gather list (slot -> token) or NULL */
    int max_rows;                    /* tokens S: upper bound of rows per group */
    int slot_rows;                   /* rows of the slot buffers (h, gu, dy, dx_slots) */
    int row_base;                    /* static groups: first slot row of group 0 */
    const uint16_t* x;  int ldx;     /* [S][D] block input */
    const uint16_t* h;  int ldh;     /* [slot_rows][I] forward silu(g)*u */
    const uint16_t* gu; int ldgu;    /* [slot_rows][2I] forward pre-activations (umoe_tgemm_args.aux_out) */
    const uint16_t* dy; int lddy;    /* [slot_rows][D] gradient of the expert outputs */
    uint16_t* dx_slots; int lddx;    /* out [slot_rows][D]: gradient of the gathered inputs (-> umoe_permute_bwd) */
    uint16_t* const* dw_gate;        /* host arrays [num_groups] of device pointers, outputs [I][D], [I][D], [D][I] */
    uint16_t* const* dw_up;
    uint16_t* const* dw_down;
    void* ws; size_t ws_bytes;       /* umoe_swiglu_bwd_workspace_bytes() */
    const uint16_t* w_down_T;        /* optional, both or neither, read ONLY when I % 32 != 0 (otherwise the input gradients read the weights */
    const uint16_t* w_gateup_T;      /* as stored, umoe_tgroup_t.w_kmajor): transposed weight copies of the caller, group g's Wd^T [I][roundup8(D)]
                                      * at w_down_T + g*I*roundup8(D), (Wg^T | Wu^T) [D][2I] at w_gateup_T + g*D*2I -- what the composite
                                      * builds per call itself otherwise */
} umoe_swiglu_bwd_args;
size_t umoe_swiglu_bwd_workspace_bytes(const umoe_swiglu_bwd_args* a);
int umoe_grouped_swiglu_bwd(const umoe_swiglu_bwd_args* a, umoe_stream_t stream);
int umoe_shared_swiglu_bwd(const umoe_swiglu_bwd_args* a, umoe_stream_t stream);
/* The same composites with fp32 main gradients: dw_gate / dw_up / dw_down hold FP32 device pointers (16-byte aligned) that the three
 * weight-gradient products add into (umoe_tiled_gemm_tn_acc); the K-split rule of the shared experts tests for a stacked slab in fp32
 * elements.  dx_slots and everything on the input-gradient chain are bit-identical to the bf16 composites. */
int umoe_grouped_swiglu_bwd_acc(const umoe_swiglu_bwd_args* a, umoe_stream_t stream);
int umoe_shared_swiglu_bwd_acc(const umoe_swiglu_bwd_args* a, umoe_stream_t stream);

/* backward of umoe_aux_loss_fwd (core.py:361-389): d_logits [S][E] fp32 = *d_aux * d aux / d logits (zero on the columns the
 * mask removed and on the shared columns); ws: 17 floats of scratch (per-expert token fractions, weight sum). */
int umoe_aux_loss_bwd(const void* logits, int logits_bf16, const int32_t* expert_mask, const float* token_weight, int S, int E,
                      int n_dyn, const float* d_aux, float* d_logits, float* ws, umoe_stream_t stream);

/* Qwen2RMSNorm backward (model.py:206-207): h [S][D] the normalised tensor's input, dy the gradient of w * bf16(h * rs);
 * dh = rs * (dy*w - xh * mean(dy*w*xh)) + dsum (gradient arriving on h through the residual path, optional), dw [D].
 * ws: fp32 scratch of min(S,512)*D floats. */
int umoe_rmsnorm_residual_bwd(const uint16_t* h, const uint16_t* w, const uint16_t* dy, const uint16_t* dsum, float eps, int S,
                              int D, uint16_t* dh, uint16_t* dw, float* ws, size_t ws_floats, umoe_stream_t stream);


/* ------------------------------------------------------------------ norm / rope / attention
 * umoe_rmsnorm_residual_fwd: y = w * bf16((x [+ r]) * rsqrt(mean((x+r)^2) + eps)); also writes x+r.
 * Replaces transformers Qwen2RMSNorm (model.py:206-207,227,240,428) + residual adds (:238,:242). */
int umoe_rmsnorm_residual_fwd(const uint16_t* x, const uint16_t* r, const uint16_t* w, float eps, int S, int D,
                              uint16_t* sum_out, uint16_t* y, umoe_stream_t stream);

/* mRoPE + KV append.  qkv [rows*T][(H+2*KVH)*hd] bf16 (bias already added).  cos/sin tables
 * [max_pos][hd/2] bf16 built by the host exactly as Qwen2_5_VLRotaryEmbedding does; pos3 [3][rows*T]
 * position streams; sections = mrope_section (channel block i uses stream i%3).
 * Writes rotated q to q_out [rows*T][H*hd] and rotated k / v into the cache at kv_pos[row*T+t]:
 * cache layout [rows][KVH][Lmax][hd].  Replaces apply_multimodal_rotary_pos_emb + DynamicCache.update. */
typedef struct {
    const uint16_t* qkv;
    const uint16_t* cos_tab;
    const uint16_t* sin_tab;
    const int32_t* pos3;      /* [3][n_tok] */
    const int32_t* kv_pos;    /* [n_tok] cache slot of each token */
    int n_tok, T;             /* n_tok = rows*T; token i belongs to row i / T */
    int H, KVH, hd;
    int sec0, sec1, sec2;
    int Lmax;
    uint16_t* q_out;
    uint16_t* k_cache;
    uint16_t* v_cache;
} umoe_rope_args;
int umoe_qkv_mrope_kvappend(const umoe_rope_args* a, umoe_stream_t stream);

/* Attention backward, training path (reference: eager_attention_forward of the transformers dependency called at
 * model.py:228-237; fp32 softmax, probabilities cast to bf16).  The contractions run on umoe_tiled_gemm over materialised
 * score tiles; these are the row-wise pieces.  scores [heads*Tp][ld] fp32 raw Q K^T, row h*Tp + t sees keys [kv_start, t]:
 * p_out = bf16(softmax(scale * scores)), zero elsewhere (including the padding columns up to ld_p).
 * backward: ds = bf16(scale * p o (dp - sum_j dp_j p_j)). */
int umoe_attn_softmax_fwd(const float* scores, int ld, int heads, int T, int Tp, int kv_start, float scale, uint16_t* p_out,
                          int ld_p, umoe_stream_t stream);
int umoe_attn_softmax_bwd(const uint16_t* p, const uint16_t* dp, int ld, int heads, int T, int Tp, float scale, uint16_t* ds,
                          umoe_stream_t stream);
/* backward of umoe_attn_prefill_fwd over full sequences (nq == T queries per row, one per key position; keys
 * [kv_start[row], t] visible to query t): dq [rows*T][H*hd], dk / dv in cache layout (positions [0, T) written).
 * "Unfused" first version: scores are materialised per (row, kv head) group in the workspace (up to 16 heads per kv head).
 * Pinned by tests/test_gpu_attn_train.py: every dq row and dk / dv positions [0, T) are written, slots [T, Lmax) are not
 * touched; the dq rows of queries that see no key (t < kv_start) and the dk / dv rows below kv_start are exactly zero; the
 * visible outputs do not depend on what the masked slots (K / V below kv_start, q / d_out rows of padded queries) hold,
 * PROVIDED those values are finite: the kernels stage the 64-key step that holds kv_start whole and give its masked keys a
 * zero probability, and 0 x NaN in the matrix core is NaN (umoe_qkv_mrope_kvappend writes every slot of [0, T), so both
 * callers keep this).  Two calls on the same inputs give the same bits. */
typedef struct {
    const uint16_t* q;             /* [rows*T][H*hd] rotated queries (umoe_qkv_mrope_kvappend q_out) */
    const uint16_t* k_cache;       /* [rows][KVH][Lmax][hd] */
    const uint16_t* v_cache;
    const int32_t* kv_start_host;  /* HOST [rows] */
    const uint16_t* d_out;         /* [rows*T][H*hd] gradient of the attention output */
    int rows, T, H, KVH, hd, Lmax;
    float scale;
    uint16_t* dq;
    uint16_t* dk_cache;
    uint16_t* dv_cache;
    void* ws; size_t ws_bytes;     /* umoe_attn_prefill_bwd_workspace_bytes() */
    const uint16_t* out;           /* optional: the forward's output [rows*T][H*hd] and its log-sum-exp [rows*T][H] (fp32,        */
    const float* lse;              /* umoe_attn_args.lse_out).  Both given (hd 128, <= 8 heads per kv head): fused flash-style     */
                                   /* backward, no score matrices in memory; otherwise the unfused composite.                    */
} umoe_attn_bwd_args;
size_t umoe_attn_prefill_bwd_workspace_bytes(const umoe_attn_bwd_args* a);
int umoe_attn_prefill_bwd(const umoe_attn_bwd_args* a, umoe_stream_t stream);
/* backward of umoe_qkv_mrope_kvappend: dq [n_tok][H*hd], dk / dv in cache layout -> d(qkv) [n_tok][(H+2KVH)*hd] */
int umoe_qkv_mrope_bwd(const umoe_rope_args* a, const uint16_t* dq, const uint16_t* dk_cache, const uint16_t* dv_cache,
                       uint16_t* dqkv, umoe_stream_t stream);



/* Attention over the cache for nq query tokens per row (nq=1 decode, nq=T causal prefill).
 * q [rows*nq][H*hd]; query t of a row sees cache slots [kv_start[row], q_pos0[row] + t].
 * Split over keys (flash-decoding) + umoe_attn_combine.  out [rows*nq][H*hd] bf16.
 * Replaces Qwen2_5_VLAttention's sdpa/eager core (model.py:228-237). */
typedef struct {
    const uint16_t* q;
    const uint16_t* k_cache;
    const uint16_t* v_cache;
    const int32_t* kv_start;  /* [rows] first valid slot (left padding) */
    const int32_t* q_pos0;    /* [rows] cache slot of this call's first query */
    int rows, nq, H, KVH, hd, Lmax;
    int splits;               /* key splits per (row, kv head, query) */
    float scale;
    float* part_o;            /* [rows*nq][H][splits][hd] */
    float* part_ml;           /* [rows*nq][H][splits][2]  */
    uint16_t* out;
    /* decode fusion (nq == 1): when qkv_raw is set the kernel applies mRoPE to q and to the new k itself, appends the
     * new K/V to the cache slot q_pos0[row] (the caches are then written) and `q` is ignored */
    const uint16_t* qkv_raw;  /* [rows][(H+2*KVH)*hd] bias-added QKV of the new token */
    const uint16_t* cos_tab;
    const uint16_t* sin_tab;
    const int32_t* pos3;      /* [3][rows] */
    int sec0, sec1, sec2;
    float* lse_out;           /* optional (umoe_attn_prefill_fwd, MFMA path): log-sum-exp per (query, head) [rows*nq][H], +inf for
                               * queries that see no key (their out row is exactly zero); kept for umoe_attn_prefill_bwd.
                               * MFMA path: slots below kv_start inside the 64-slot step that holds it are loaded and must be
                               * finite; slots behind q_pos0 + nq - 1 are never read */
} umoe_attn_args;
int umoe_attn_decode(const umoe_attn_args* a, umoe_stream_t stream);
/* causal prefill (nq = T queries per row) over keys already appended by umoe_qkv_mrope_kvappend */
int umoe_attn_prefill_fwd(const umoe_attn_args* a, umoe_stream_t stream);

/* ------------------------------------------------------------------ codec side
 * codec_embedding (model.py:655-661): out[r] = sum_c Emb_c[tok[r][c]], bf16 adds in channel order.
 * emb [C][V][D].  Ids outside [0, V - 1] are clamped into the table.  rows == 0: a success that touches nothing (the pointers may be null). */
int umoe_codec_embed_sum(const int32_t* tok, const uint16_t* emb, int rows, int C, int V, int D, uint16_t* out,
                         umoe_stream_t stream);
/* backward of the same (the reference's autograd of the C nn.Embedding gathers, model.py:655-661): d_emb[c][v] = sum over the rows r
 * with tok[r][c] == v of d_out[r], fp32 accumulation in ASCENDING row order (deterministic), one rounding to bf16; rows of the table
 * nobody selected are written as zeros; ids outside [0, V - 1] contribute nowhere (they are NOT clamped: placeholder positions carry
 * id -1).  D % 8 == 0, D <= 2048 * 8.  rows == 0: tok and d_out may be null, d_emb is all zeros. */
int umoe_codec_embed_sum_bwd(const int32_t* tok, const uint16_t* d_out, int rows, int C, int V, int D, uint16_t* d_emb,
                             umoe_stream_t stream);

/* CFG + masks + sampling on codec-head logits (model.py:991-1017, 873-916).
 * logits [2B][C*V] fp32 (row 2b = uncond, 2b+1 = cond).  temperature 0 or do_sample 0 => arg-max.
 * probs_out optional [B*C][V] (post-filter probabilities, for parity).  rng: Philox-free counter
 * hash seeded by (seed, step, row). */
/* Per-request settings of one batch entry b (a CFG pair): a table of B of them in DEVICE memory replaces the scalar members of the
 * same names in umoe_sample_args / umoe_decode_io (and the one max_tokens of umoe_delay_step) when `row_params` is set there.  The
 * kernels read the table at every launch, so a captured step graph records the POINTER: the values may be rewritten between
 * requests.  8-byte aligned. */
typedef struct {
    float cfg_scale, temperature, top_p, eos_mul;
    int32_t top_k;        /* <= 0: none */
    int32_t do_sample;
    int32_t min_tokens;   /* -1 = None */
    int32_t max_tokens;   /* this row's max_tokens (delay step only) */
    uint64_t seed;
} umoe_row_params;

typedef struct {
    const float* logits;
    int B, C, V;
    float cfg_scale, temperature, top_p, eos_mul;
    int top_k;                /* <=0: none */
    int eos;
    int enable_eos;           /* host flag; or enable_eos_from_step >= 0: enabled iff *step >= that */
    int min_tokens;           /* -1 = None */
    const int32_t* step;      /* device scalar dec_step (may be NULL) */
    int do_sample;
    uint64_t seed;
    int64_t* pred;            /* [B][C] */
    float* probs_out;
    const int32_t* row_clock;          /* device int32 [2B] {step_off[b], t_prompt[b]} or NULL (= the one clock *step).  Set: workgroup (b, c)
                                        * lives on row b's local clock, local = *step - step_off[b]: min_tokens is compared with `local`
                                        * and the draw is u(seed, local, b * C + c) (the sampler reads step_off only) */
    const umoe_row_params* row_params; /* device [B] or NULL.  Set: workgroup (b, c) takes cfg_scale, temperature, top_p, eos_mul, top_k,
                                        * do_sample, min_tokens and seed from row_params[b]; the draw of row (b, c) stays
                                        * u(seed, step, b * C + c), what it is in a launch whose one seed is row_params[b].seed */
} umoe_sample_args;
int umoe_codec_head_cfg_sample(const umoe_sample_args* a, umoe_stream_t stream);

/* One step of generate()'s token bookkeeping on device (model.py:1173-1203 + DecoderOutput.update_one,
 * utils/UniMoE_Audio_utils.py:290-298): EOS detection on channel 0, countdown, forced EOS/PAD by delay
 * pattern, BOS masking, append into tokens[B][Tmax][C], advance *step.  state = int32[4*B + 8]:
 * eos_detected[B], countdown[B], finished[B], prefill_step[B], then {step, max_tokens, all_done, bos_over,
 * step0 (dec_step of the first decode call), 3 reserved}. */
int umoe_delay_step(int64_t* pred, int32_t* tokens, int32_t* state, const int32_t* delay, int B, int C, int Tmax,
                    int eos, int pad, int max_delay, umoe_stream_t stream);
/* the same with per-row lengths: row b is forced to end at cur >= row_params[b].max_tokens - max_delay (device table [B]; NULL = the
 * one max_tokens of the state, i.e. umoe_delay_step).  The loop bound state[4B + 1] stays one number: the host sets it to the
 * largest row value. */
int umoe_delay_step_rows(int64_t* pred, int32_t* tokens, int32_t* state, const int32_t* delay, int B, int C, int Tmax,
                         int eos, int pad, int max_delay, const umoe_row_params* row_params, umoe_stream_t stream);
/* the same on per-row clocks: row_clock = device int32 [2B] {step_off[b], t_prompt[b]} (NULL = umoe_delay_step_rows).  Row b lives at
 * cur_b = (step - step_off[b]) + 1: its forced ending, finished[b], its term of bos_over and the slot tokens[b][cur_b] it writes use
 * cur_b.  A row whose countdown is 0 at entry (ended, or never used) writes no token.  "Every countdown is 0" still ends a run;
 * step >= max_tokens does not (rows come and go, each ends by its own max_tokens).  The step word advances by one per launch. */
int umoe_delay_step_clock(int64_t* pred, int32_t* tokens, int32_t* state, const int32_t* delay, int B, int C, int Tmax,
                          int eos, int pad, int max_delay, const umoe_row_params* row_params, const int32_t* row_clock,
                          umoe_stream_t stream);

/* Per-channel codec cross-entropy of the training loss (model.py:830-847) on already shifted logits [N][C][V] fp32 and
 * labels [N][C] int64 (-100 = ignore): ch_loss[c] = mean nll over valid labels, total = ch_loss[0] + sum of channels with
 * at least one valid label.  probs (optional [N][C][V]) keeps the softmax rows for umoe_codec_ce_bwd:
 * dlogits = grad * (softmax - onehot) / count_c.  Fixed-order reductions, no atomics. */
int umoe_codec_ce_fwd(const float* logits, const int64_t* labels, int N, int C, int V, float* nll_ws, float* probs,
                      float* ch_loss, int32_t* ch_count, float* total, umoe_stream_t stream);
int umoe_codec_ce_bwd(const float* probs, const int64_t* labels, const int32_t* ch_count, int N, int C, int V, float grad,
                      float* dlogits, umoe_stream_t stream);

/* RVQ (third-party descript-audio-codec 1.0.0 ResidualVectorQuantize, call sites
 * utils/UniMoE_Audio_utils.py:113,123): from_codes = sum_q out_proj_q(codebook_q[code]); nearest = per level
 * in_proj, L2-normalised nearest neighbour, subtract.  All DAC dims are load-time parameters. */
int umoe_rvq_from_codes(const int32_t* codes, const float* codebooks, const float* out_w, const float* out_b, int NQ,
                        int CB, int cd, int Dl, int T, float* z, umoe_stream_t stream);
/* from_delayed: the same sums for frames [f0, f0 + n) of Bz rows, the codes read from the decode engine's delayed token buffer
 * tokens [B][Tmax][NQ]: z row r is token row rows[r] (rows == NULL: r), frame t's code of level q is
 * tokens[row][prefill_step[row] + t + delay[q]][q]; positions at or past t_valid read as `pad`.  prefill_step [B], delay [NQ] and rows
 * [Bz] are device arrays.  z [Bz][Dl][Lz], frame t written to column t - f0 + z_off. */
int umoe_rvq_from_delayed(const int32_t* tokens, int B, int Tmax, int NQ, const int32_t* prefill_step, const int32_t* delay, int t_valid,
                          int pad, const int32_t* rows, int Bz, int f0, int n, const float* codebooks, const float* out_w, const float* out_b,
                          int CB, int cd, int Dl, float* z, int z_off, int Lz, umoe_stream_t stream);
int umoe_rvq_nearest(const float* z, const float* codebooks, const float* in_w, const float* in_b, const float* out_w,
                     const float* out_b, int NQ, int CB, int cd, int Dl, int T, int32_t* codes, float* resid_ws,
                     umoe_stream_t stream);

/* DAC conv stacks (third-party descript-audio-codec 1.0.0 DAC.encode / DAC.decode behind utils/UniMoE_Audio_utils.py:112-113,123-124;
 * restated from the published architecture, PARITY UNPINNED, every dimension a load-time parameter).  fp32, [B][C][L] layout.
 * The Snake activation of the PRECEDING layer (x + sin(alpha x)^2 / (alpha + 1e-9), per input channel) is fused into the input
 * load when snake_alpha != NULL; bias, the residual add of a ResidualUnit (resid, same shape as y) and the decoder's final tanh
 * (act = 1) into the store.  Weights are the weight-normalised tensors already folded (g * v / |v|, done once at load time).
 *   umoe_dac_conv1d:            w [Cout][Cin][K], Lout = floor((L + 2 pad - dilation (K - 1) - 1) / stride) + 1; a receptive
 *                               field wider than the padded input (negative numerator) is an empty output and is refused
 *   umoe_dac_conv_transpose1d:  w [Cin][Cout][K], Lout = (L - 1) stride - 2 pad + K + out_pad */
int umoe_dac_conv1d(const float* x, const float* w, const float* bias, const float* snake_alpha, const float* resid, int B, int Cin,
                    int L, int Cout, int K, int stride, int dilation, int pad, int act, float* y, int* Lout_out, umoe_stream_t stream);
int umoe_dac_conv_transpose1d(const float* x, const float* w, const float* bias, const float* snake_alpha, int B, int Cin, int L,
                              int Cout, int K, int stride, int pad, int out_pad, float* y, int* Lout_out, umoe_stream_t stream);
/* Windowed twins for streaming decode: outputs [t_begin, t_begin + n) (absolute positions) of the convolution of a sequence of true
 * length L, with the full convolution's zero padding outside [0, L).  x holds input positions [x_off, x_off + Lx) ([B][Cin][Lx]),
 * resid positions [r_off, r_off + Lr), y positions [y_off, y_off + Ly).  Every input position inside [0, L) that the requested outputs
 * read must lie in the x buffer (checked).  Each output is bit-identical to the same position of umoe_dac_conv1d /
 * umoe_dac_conv_transpose1d on the whole sequence. */
int umoe_dac_conv1d_win(const float* x, int x_off, int Lx, const float* w, const float* bias, const float* snake_alpha, const float* resid,
                        int r_off, int Lr, int B, int Cin, int L, int Cout, int K, int stride, int dilation, int pad, int act, int t_begin,
                        int n, float* y, int y_off, int Ly, umoe_stream_t stream);
int umoe_dac_conv_transpose1d_win(const float* x, int x_off, int Lx, const float* w, const float* bias, const float* snake_alpha, int B,
                                  int Cin, int L, int Cout, int K, int stride, int pad, int out_pad, int t_begin, int n, float* y, int y_off,
                                  int Ly, umoe_stream_t stream);
/* Per-row window tables (the per-row streaming decoder of dac.py: one launch per layer for rows that are each on a timeline of their
 * own).  A table is a flat array of int64 words, a fixed number per row, built by the host (unimoe_audio_amd.dac.DAC_ROW_FIELDS and its
 * siblings name the words in this order); it is no C struct.  Every entry point takes it twice: `host`, which the checks read, and
 * `table`, the 8-byte aligned device copy the kernel reads (a caller uploads the tables of all layers of a read in one copy).
 *
 * UMOE_DAC_ROW_WORDS words per row of umoe_dac_conv1d_win_rows / umoe_dac_conv_transpose1d_win_rows:
 *   0 x       plane [Cin][Lx] of the row's input window (a device address)
 *   1 resid   plane [Cout][Lr] of its residual window, 0 = none (umoe_dac_conv_transpose1d_win_rows does not read it)
 *   2 y       plane [Cout][Ly] of its output window
 *   3 x_off   4 Lx   5 r_off   6 Lr   7 y_off   8 Ly   9 t_begin   10 n      as the arguments of the _win entries
 *   11 L      the true length of the row's sequence at this layer's input
 * Grid (ceil(max_n / 64), ceil(Cout / 64), rows); a workgroup whose tile starts at or past its row's n returns at once, so n = 0 makes a
 * row idle (its other words are not read).  Every row with n > 0 passes the checks of the _win entry and has n <= max_n; nothing is
 * enqueued unless all rows pass.  The kernels are the _win kernels' bodies, so an output is bit-identical to umoe_dac_conv1d_win /
 * umoe_dac_conv_transpose1d_win on that row's window.
 *
 * UMOE_RVQ_ROW_WORDS words per row of umoe_rvq_from_delayed_rows (umoe_rvq_from_delayed with a record per z row):
 *   0 row     the token row   1 f0   2 n   3 t_valid (the row's own: its local step + 1)
 *   4 z       plane [Dl][Lz] (a device address)   5 col: frame f0's column   6 Lz   7 reserved
 *
 * UMOE_SHIFT_ROW_WORDS words per row of umoe_dac_shift_rows (the left context of a slab, moved in place):
 *   0 plane   [C][W] (a device address)   1 W   2 shift   3 count: columns [shift, shift + count) move to [0, count); 0 = leave alone */
#define UMOE_DAC_ROW_WORDS 12
#define UMOE_RVQ_ROW_WORDS 8
#define UMOE_SHIFT_ROW_WORDS 4
int umoe_dac_conv1d_win_rows(const int64_t* host, const int64_t* table, int rows, int max_n, const float* w, const float* bias,
                             const float* snake_alpha, int Cin, int Cout, int K, int stride, int dilation, int pad, int act,
                             umoe_stream_t stream);
int umoe_dac_conv_transpose1d_win_rows(const int64_t* host, const int64_t* table, int rows, int max_n, const float* w, const float* bias,
                                       const float* snake_alpha, int Cin, int Cout, int K, int stride, int pad, int out_pad,
                                       umoe_stream_t stream);
int umoe_dac_shift_rows(const int64_t* host, const int64_t* table, int rows, int C, umoe_stream_t stream);
/* The six convolution entries above on the f32-input MFMA (v_mfma_f32_16x16x4_f32; csrc/umoe_dac_mfma.hip): the argument list of the
 * direct sibling with w replaced by wt, the k-major copy [Cin][K][Cout] of the folded weight (conv1d: w.permute(1, 2, 0); transposed:
 * w.permute(0, 2, 1)).  Same function, same windows, same per-row tables (UMOE_DAC_ROW_WORDS, same words), same int64 window checks,
 * same refusals by name with nothing written (bad arguments, an empty output); max_n == 0 and idle rows enqueue nothing.  fp32 in,
 * fp32 accumulate: each output is an fmaf chain over (ci, k) ascending in steps of 4, so results differ from the direct kernels in
 * the last bits and stay inside the same float64 bounds; among themselves the six are bit-identical per output position (the order
 * never depends on the tile, window, row or batch index).  Grid (ceil(n / 64), ceil(Cout / 64), B or rows) for conv1d; the transposed
 * form tiles 64 positions per phase, grid x = ceil(nq / 64) * stride with nq the values (t + pad) / stride takes over the window.
 * Staging limit: none that depends on the geometry -- LDS is a fixed 20 480 bytes (two [32][80] fp32 images), so the direct
 * kernels' "tile needs ... bytes of LDS" refusal has no counterpart; refused instead: Cin * taps beyond an int, and a grid beyond
 * the launch limits (Cout > 64 * 65535, B > 65535). */
int umoe_dac_conv1d_mfma(const float* x, const float* wt, const float* bias, const float* snake_alpha, const float* resid, int B, int Cin,
                         int L, int Cout, int K, int stride, int dilation, int pad, int act, float* y, int* Lout_out, umoe_stream_t stream);
int umoe_dac_conv_transpose1d_mfma(const float* x, const float* wt, const float* bias, const float* snake_alpha, int B, int Cin, int L,
                                   int Cout, int K, int stride, int pad, int out_pad, float* y, int* Lout_out, umoe_stream_t stream);
int umoe_dac_conv1d_win_mfma(const float* x, int x_off, int Lx, const float* wt, const float* bias, const float* snake_alpha,
                             const float* resid, int r_off, int Lr, int B, int Cin, int L, int Cout, int K, int stride, int dilation, int pad,
                             int act, int t_begin, int n, float* y, int y_off, int Ly, umoe_stream_t stream);
int umoe_dac_conv_transpose1d_win_mfma(const float* x, int x_off, int Lx, const float* wt, const float* bias, const float* snake_alpha, int B,
                                       int Cin, int L, int Cout, int K, int stride, int pad, int out_pad, int t_begin, int n, float* y,
                                       int y_off, int Ly, umoe_stream_t stream);
int umoe_dac_conv1d_win_rows_mfma(const int64_t* host, const int64_t* table, int rows, int max_n, const float* wt, const float* bias,
                                  const float* snake_alpha, int Cin, int Cout, int K, int stride, int dilation, int pad, int act,
                                  umoe_stream_t stream);
int umoe_dac_conv_transpose1d_win_rows_mfma(const int64_t* host, const int64_t* table, int rows, int max_n, const float* wt,
                                            const float* bias, const float* snake_alpha, int Cin, int Cout, int K, int stride, int pad,
                                            int out_pad, umoe_stream_t stream);
int umoe_rvq_from_delayed_rows(const int32_t* tokens, int B, int Tmax, int NQ, const int32_t* prefill_step, const int32_t* delay, int pad,
                               const int64_t* host, const int64_t* table, int rows, int max_n, const float* codebooks, const float* out_w,
                               const float* out_b, int CB, int cd, int Dl, umoe_stream_t stream);
/* windowed-sinc resampling to the codec's rate (torchaudio.transforms.Resample as used at utils.py:101-110, restated): with o / n =
 * orig / new frequency over their gcd, kern [n][2 width + o] the filter bank (built by the host from the published formula),
 * y[b][frame * n + phase] = sum_t kern[phase][t] * x[b][frame * o - width + t] (zero outside [0, L)). */
int umoe_dac_resample(const float* x, const float* kern, int B, int L, int o, int n, int width, int Lout, float* y, umoe_stream_t stream);

/* Vision tower pieces (reference utils/UniMoE_Audio_utils.py:756-900 over the third-party transformers vision block /
 * attention / MLP / patch merger).  The projections run on umoe_tiled_gemm; these are the rest.
 *   umoe_vision_rope: apply_rotary_pos_emb_vision on q and k inside the fused qkv buffer [S][3][H][hd] (fp32 arithmetic, one rounding);
 *                     cos / sin [S][hd] fp32.
 *   umoe_vision_attn: non-causal attention of token s over the keys [seg_lo[s], seg_hi[s]) of its cu_seqlens segment; out [S][H*hd].
 *   umoe_swiglu_pair: gu [S][2I] = (gate | up) with biases -> h [S][ldh] = bf16(bf16(silu(g)) * u), columns [I, ldh) zero.
 *   umoe_gelu:        exact GELU in place (patch merger). */
int umoe_vision_rope(uint16_t* qkv, const float* cos_t, const float* sin_t, int S, int H, int hd, umoe_stream_t stream);
int umoe_vision_attn(const uint16_t* qkv, const int32_t* seg_lo, const int32_t* seg_hi, int S, int H, int hd, float scale, uint16_t* out,
                     umoe_stream_t stream);
int umoe_swiglu_pair(const uint16_t* gu, int S, int I, int ldh, uint16_t* h, umoe_stream_t stream);
int umoe_gelu(uint16_t* x, long n, umoe_stream_t stream);

/* ------------------------------------------------------------------ decode engine
 * Owns workspace + KV cache and enqueues a whole decode step (36 layers + head + sampler + delay
 * bookkeeping) from one host call, optionally replayed as a hipGraph.  Restates
 * generate()/_decoder_step() control flow (model.py:918-1231) without per-step host syncs. */
typedef struct {
    int hidden, layers, heads, kv_heads, head_dim;
    int n_dyn, n_real, n_fix, inter_dyn, inter_shared;
    int codec_channels, codec_vocab, eos, pad, bos;
    int mrope0, mrope1, mrope2;
    float rms_eps, top_p;
    int fixed_top_k;
    double jitter_eps;
    int rows;                 /* 2 * batch (CFG pairs) */
    int Lmax;                 /* KV slots per row */
    int Tmax;                 /* token buffer length */
    int attn_splits;
    int ep_rank, ep_size;     /* expert parallel decode: this rank owns experts [rank*n_real/size, ...); ep_size in {1,2,4,8},
                               * rows <= 16 per rank; see umoe_engine_ep_connect */
} umoe_engine_cfg;

typedef struct {
    const uint16_t* in_norm;      /* [D] */
    const uint16_t* qkv_w;        /* WP16 of cat(q,k,v) [H*hd + 2*KVH*hd][D] */
    const float* qkv_b;           /* [H*hd + 2*KVH*hd] fp32 */
    const uint16_t* o_w;          /* WP16 [D][H*hd] */
    const uint16_t* post_norm;    /* [D] */
    const uint16_t* gate_w;       /* [E][D] plain bf16 */
    const uint16_t* const* exp_gu; /* host array [n_real] of device ptrs: WP16 gate/up pairs */
    const uint16_t* const* exp_dn; /* host array [n_real]: WP16 down */
    const uint16_t* const* sh_gu;  /* host array [n_fix] */
    const uint16_t* const* sh_dn;  /* host array [n_fix] */
    /* optional ROW-MAJOR copies (the reference's own nn.Linear tensors) for the tiled MFMA path of the prefill; all or none.
     * rm_qkv = cat(q,k,v) [QKV][D], rm_o [D][H*hd]; per expert gate/up [I][D] and down [D][I]. */
    const uint16_t* rm_qkv;
    const uint16_t* rm_o;
    const uint16_t* const* rm_exp_gate;  /* host arrays [n_real] */
    const uint16_t* const* rm_exp_up;
    const uint16_t* const* rm_exp_down;
    const uint16_t* const* rm_sh_gate;   /* host arrays [n_fix] */
    const uint16_t* const* rm_sh_up;
    const uint16_t* const* rm_sh_down;
} umoe_layer_weights;

typedef struct umoe_engine umoe_engine;
int umoe_engine_create(const umoe_engine_cfg* cfg, umoe_engine** out);
void umoe_engine_destroy(umoe_engine* e);
int umoe_engine_set_layer(umoe_engine* e, int layer, const umoe_layer_weights* w);
/* fp8 expert weights of one layer (after umoe_engine_set_layer): host arrays [n_real + n_fix] (routed experts, then shared) of device
 * pointers to WP8 gate/up pairs, their exponents, WP8 down blocks and theirs.  An engine with fp8 weights runs every dense decode layer's
 * experts through the fp8 flat launch (or, above 16 rows with umoe_engine_set_fp8_wide, the wide form on WP8) and nothing else: a decode step it cannot run that way (the launch-per-kernel form UMOE_FLAT_MOE=0
 * UMOE_FUSE_CQ=0, UMOE_FUSE_ROUTER=0, too few compute units for a schedule) is refused before anything is enqueued; expert parallel engines (ep_size > 1) are refused here.
 * umoe_engine_info(e, "expert_fp8") = 1 when the last dense decode layer ran the fp8 launch.  Prefill keeps the bf16 weights.
 * FP8-ONLY layers: umoe_engine_set_layer may be given NO bf16 expert weight at all (exp_gu, exp_dn, sh_gu, sh_dn and every rm_exp_* /
 * rm_sh_* NULL; rm_qkv and rm_o present) when this call follows.  The experts of a prefill or admission of such an engine run on the
 * WP8 blocks at every row count (umoe_tiled_gemm_wp8), decode as above, and every pass that would stream a bf16 expert weight (the
 * ragged streaming GEMM, the launch-per-kernel decode forms, the bf16 wide form, UMOE_TILED_PREFILL=0) is refused on the host before
 * anything is enqueued.  umoe_engine_info: "expert_bf16_resident" 0 / 1; "prefill_fp8" 1 when the last prefill / admission ran its
 * experts on WP8. */
int umoe_engine_set_layer_fp8(umoe_engine* e, int layer, const uint8_t* const* gu8, const int8_t* const* gu_e, const uint8_t* const* dn8,
                              const int8_t* const* dn_e);
/* on != 0: a decode step of 17..64 rows of an fp8 engine takes the wide form with umoe_gemm_wide_fp8 for gate/up and down (QKV, o_proj,
 * router, re-lay, combine and head are the bf16 wide launches) at EVERY such size -- the engine has no other path there, so the table of
 * sizes at which the bf16 wide form was measured faster does not apply; UMOE_WIDE_DECODE=0 makes the step refuse as with the switch off.
 * umoe_engine_info then gives "expert_launch" 4, "expert_fp8" 1, "row_tiles" = tiles.  Steps of 16 rows or fewer take the fp8 flat launch
 * either way.  Default off: a directly constructed fp8 engine of more than 16 rows refuses its decode step as before. */
int umoe_engine_set_fp8_wide(umoe_engine* e, int on);
/* WP12 copies of one layer's bf16 expert weights (after umoe_engine_set_layer with the WP16 packs; ep_size 1, no fp8 weights): host
 * arrays [n_real + n_fix] (routed experts, then shared) of device pointers to WP12 gate/up pairs, their block records, WP12 down blocks
 * and theirs.  The flat expert launch of this layer then streams them (moe_flat_w12_kernel; the same outputs bit for bit, 0.75 of the
 * bytes), and so does the wide form with umoe_engine_set_w12_wide; every other form keeps reading the WP16 packs.  UMOE_FLAT_W12=0 selects the WP16 launch.  umoe_engine_info(e, "expert_w12")
 * = 1 when the last dense decode layer ran the WP12 launch.
 * After umoe_engine_set_layer with EVERY bf16 expert pointer NULL (the layer shape of fp8-only) the layer becomes a w12-only layer: the
 * WP12 copies are all it has.  Its experts run a prefill / admission of any row count on them (umoe_tiled_gemm_w12), its decode is the
 * WP12 flat launch up to 16 rows and the WP12 wide form at every row count 17..64 (umoe_engine_set_w12_wide must be on); every pass or
 * switch that would stream a bf16 expert weight is refused on the host before anything is enqueued, with a message that names the missing
 * weights.  Layers may be mixed with layers that kept their bf16 weights.  umoe_engine_info: "w12_only_layers", "prefill_w12" (1: the last
 * prefill or admission ran experts on WP12), "expert_bf16_resident" (0 only when no layer holds bf16 expert weights). */
int umoe_engine_set_layer_w12(umoe_engine* e, int layer, const uint8_t* const* gu12, const uint32_t* const* gu_m, const uint8_t* const* dn12,
                              const uint32_t* const* dn_m);
/* on != 0: the wide form of a decode step of 17..64 rows (whether a step is wide, and the size table behind that, are untouched: the switch changes which kernel a
 * wide step runs, not whether the step is wide) runs the gate/up and down launches of every layer that has WP12 copies
 * (umoe_engine_set_layer_w12 stores them at any row count) through umoe_gemm_wide_w12: the same outputs bit for bit, 0.75 of the expert
 * bytes.  A layer without copies (not packable) and an fp8 engine keep their launches.  UMOE_WIDE_W12=0, read per enqueue, forces the WP16
 * launches on such an engine.  umoe_engine_info(e, "expert_w12") = 1 when the last layer's wide expert launches ran on WP12;
 * "expert_launch" stays 4 and "row_tiles" the tile count.  Default off. */
int umoe_engine_set_w12_wide(umoe_engine* e, int on);
/* What the engine decides per layer of a pass -- the launch form of the MoE half, the weight format its expert launches stream, how the
 * attention GEMMs run -- is one pure function of this POD (csrc/umoe_engine_plan.h).  The engine fills it once per pass, before anything
 * is enqueued, and refuses the pass when a layer does not hold the format it would stream. */
enum { UMOE_PASS_PREFILL = 0, UMOE_PASS_ADMISSION = 1, UMOE_PASS_DECODE = 2 };       /* umoe_plan_in.kind */
enum { UMOE_FMT_WP16 = 0, UMOE_FMT_WP8 = 1, UMOE_FMT_WP12 = 2, UMOE_FMT_RM = 3 };    /* umoe_plan_out.format; RM: row-major bf16 (the bf16 tiled form) */
enum { UMOE_ATTN_STREAM = 0, UMOE_ATTN_TILED = 1, UMOE_ATTN_WIDE = 2 };              /* umoe_plan_out.attn */
/* what a layer holds (umoe_plan_in.holds[layer]): the WP16 expert packs, the row-major expert / attention tensors, WP8 blocks, WP12 copies */
enum { UMOE_HOLD_SET = 1, UMOE_HOLD_BF16 = 2, UMOE_HOLD_RM_EXP = 4, UMOE_HOLD_RM_ATTN = 8, UMOE_HOLD_WP8 = 16, UMOE_HOLD_WP12 = 32 };
typedef struct umoe_plan_in {
    int32_t rows, hidden, inter_dyn, inter_shared, n_dyn, n_real, n_fix, ep_size;    /* of umoe_engine_cfg */
    int32_t n_cu;                                           /* compute units (UMOE_FAKE_CUS overrides) */
    int32_t tiled_prefill, fuse_router, dense_min_rows;     /* UMOE_TILED_PREFILL, UMOE_FUSE_ROUTER, UMOE_DENSE_MIN_ROWS: read when the engine is created */
    int32_t fp8_wide, w12_wide;                             /* umoe_engine_set_fp8_wide, umoe_engine_set_w12_wide */
    int32_t flat_moe, flat_w12, wide_w12, wide_decode;      /* UMOE_FLAT_MOE, UMOE_FLAT_W12, UMOE_WIDE_W12, UMOE_WIDE_DECODE, read once per pass: -1 unset, 0, 1 */
    int32_t kind, n_tok;                                    /* the pass: UMOE_PASS_*, and its token count (a decode step: rows) */
    int32_t n_layers;
    const uint8_t* holds;                                   /* [n_layers] masks of UMOE_HOLD_* */
} umoe_plan_in;
typedef struct umoe_plan_out {
    int32_t form;        /* 0 tiled, 1 ragged, 2 flat, 3 launch per kernel with router riders, 4 launch per kernel with the router launch, 5 wide,
                          * 6 the expert-parallel decode half (outside the decision) */
    int32_t format;      /* UMOE_FMT_* of the expert launches */
    int32_t attn;        /* UMOE_ATTN_* */
} umoe_plan_out;
/* test hook (no GPU needed): the decision for every layer of a caller-filled pass.  in_bytes = sizeof(umoe_plan_in) as the caller sees it;
 * rc [n_layers]: 0, or -1 = the pass is refused for this layer with the reason in msg + layer * msg_len (out still names what the pass
 * would have run).  Returns 0, or -1 for a bad argument. */
int umoe_engine_plan_probe(const umoe_plan_in* in, int in_bytes, umoe_plan_out* out, int32_t* rc, char* msg, int msg_len);
/* test hook: the fp8 launch's conversion path over a row-major e4m3 matrix q [N][K] (K % 8 == 0) with one exponent per row:
 * out[r][k] = bf16 bits of q[r][k] * 2^e[r] */
int umoe_fp8_convert_probe(const uint8_t* q, const int8_t* e, int N, int K, uint16_t* out, umoe_stream_t stream);
/* final norm [D], codec embeddings [C][V][D], WP16 codec head [C*V][D], rope tables [max_pos][hd/2] */
int umoe_engine_set_globals(umoe_engine* e, const uint16_t* final_norm, const uint16_t* codec_emb,
                            const uint16_t* codec_head_w, const uint16_t* cos_tab, const uint16_t* sin_tab, int max_pos,
                            const int32_t* delay_pattern_host);
size_t umoe_engine_workspace_bytes(const umoe_engine* e);
/* prefill: x [rows*T][D] input embeddings (host builds them: text embed + codec scatter, model.py:663-670),
 * valid [rows][T] 0/1 attention mask (left padded). Fills the KV cache. */
int umoe_engine_prefill(umoe_engine* e, const uint16_t* x, const uint8_t* valid_host, int T, umoe_stream_t stream);
/* the same with explicit rotary positions (multimodal prompts, reference get_rope_index model.py:513-652): pos3_host [3][rows][T]
 * int32 (NULL = from the mask as above), next_pos_host [rows] = position of the first generated token of each row = max position + 1
 * (the reference's cache_position + rope_deltas; NULL = number of valid tokens) */
int umoe_engine_prefill_pos(umoe_engine* e, const uint16_t* x, const uint8_t* valid_host, int T, const int32_t* pos3_host,
                            const int32_t* next_pos_host, umoe_stream_t stream);
/* the prompt was run outside the engine (an expert-parallel rank that holds ONLY its local experts -- core.py:505,
 * deepspeed_ep_param_aggregation.py:16-48 -- prefills through the module-level forward, whose DCMoE blocks exchange rows between the ranks)
 * and the caller copied the roped K / V of every layer into slots [0, T) of the cache buffers (umoe_engine_buffer "k_cache" / "v_cache",
 * [layer][row][kv_head][Lmax][head_dim]): sets the decode state only (arguments as umoe_engine_prefill_pos) */
int umoe_engine_prefill_external(umoe_engine* e, const uint8_t* valid_host, int T, const int32_t* pos3_host, const int32_t* next_pos_host,
                                 umoe_stream_t stream);
/* decode bookkeeping state + token buffer (device, owned by caller) */
typedef struct {
    int32_t* tokens;          /* [B][Tmax][C], -1 = to be generated */
    int32_t* state;           /* see umoe_delay_step */
    float cfg_scale, temperature, top_p, eos_mul;
    int top_k, do_sample, min_tokens;
    uint64_t seed;
    int32_t* row_clock;       /* device int32 [rows] {step_off[b], t_prompt[b]} per batch entry, or NULL (= one clock for the batch: the
                               * step word, its first value state[4B + 4] and the prompt length of the last prefill).  Set: row b
                               * decodes on its local clock step - step_off[b] behind a prompt of t_prompt[b] cache slots, and a row
                               * whose countdown is 0 is parked (attends to one key).  umoe_engine_admit writes the entries. */
    const umoe_row_params* row_params; /* device [rows / 2] or NULL (= the scalar members above): per-request sampling settings and
                                        * max_tokens, handed to the sampler and the delay step of every step */
} umoe_decode_io;
int umoe_engine_decode_step(umoe_engine* e, const umoe_decode_io* io, umoe_stream_t stream);
/* graph capture of one decode step; replays read all step-dependent scalars from device memory */
int umoe_engine_capture(umoe_engine* e, const umoe_decode_io* io, umoe_stream_t stream);
int umoe_engine_replay(umoe_engine* e, umoe_stream_t stream);
/* one eager step with a hipEvent (on `stream`) after every kernel class; accumulates into ms[13] / launches[13]:
 * {qkv, rope, attn, oproj, router, dispatch, gateup, down, combine, embed, head, sample, delay} */
int umoe_engine_profile_step(umoe_engine* e, const umoe_decode_io* io, umoe_stream_t stream, float* ms, int* launches,
                             int n);
/* Admission of a request into a free row of a batch that is decoding (io->row_clock set; ep_size 1; 1-D positions).
 * umoe_engine_reserve: sizes the workspace for prompts of up to n_tok tokens (2 * T of the longest admitted prompt) and puts the group
 *   table into decode shape.  The workspace is re-allocated (and zeroed) here and never afterwards by an admission, so a captured step
 *   graph stays valid across admissions: call it once when serving starts, before the first admission.
 * umoe_engine_admit: prefills the CFG pair x [2 * T][D] (valid_host [2][T], left padded) into cache rows 2b, 2b + 1 -- the prefill body
 *   of umoe_engine_prefill over 2 rows -- and resets batch entry b on the device, in stream order and without a host read of the state:
 *   row_clock[b] = {step - (prefill_step - 1), T}, eos_detected 0, countdown -1, finished -1, prefill_step, tokens[b][t >= prefix_len]
 *   = -1 (the caller has written the request's prefix tokens[b][0 .. prefix_len) -- the buffer of the reference's _prepare_audio_prompt,
 *   prefill_step <= prefix_len, with its own -1 entries -- and row_params[b] before the call).  Of the engine's
 *   persistent state only kv_start / valid_count of rows 2b, 2b + 1 and the cache slabs of those rows change.  Refuses (before anything
 *   is enqueued) a prompt beyond the reservation, an expert parallel engine, a row outside the batch.
 * umoe_engine_admit_external: the caller has written slots [0, T) of rows 2b, 2b + 1 of the K / V slabs; sets the state only. */
int umoe_engine_reserve(umoe_engine* e, int n_tok);
int umoe_engine_admit(umoe_engine* e, const umoe_decode_io* io, int b, const uint16_t* x, const uint8_t* valid_host, int T,
                      int prefill_step, int prefix_len, umoe_stream_t stream);
int umoe_engine_admit_external(umoe_engine* e, const umoe_decode_io* io, int b, const uint8_t* valid_host, int T, int prefill_step,
                               int prefix_len, umoe_stream_t stream);
/* Prefix reuse across admissions (ep_size 1).  A prefix STORE is a caller-owned bf16 device buffer [layers][2 (K, V)][kv_heads][P][head_dim]:
 * the roped keys and the values of prompt tokens 0 .. P - 1 at rope positions 0 .. P - 1.
 * umoe_kv_prefix_copy: ONE launch over all layers, K and V and every kv head, in 16-byte pieces (head_dim % 8 == 0).  jobs_host holds
 *   n_jobs (1..8) records {row, i0, s0, n}.  extract == 0 (install): store tokens [i0, i0 + n) -> slots [s0, s0 + n) of cache row `row`;
 *   extract != 0: the other way.  The caches are [layers][rows][kv_heads][Lmax][head_dim].  Every range is checked on the host (0 <= i0,
 *   i0 + n <= P, 0 <= s0, s0 + n <= Lmax, 0 <= row < rows, n >= 0; no two installs overlap in a row, no two extracts in the store);
 *   nothing outside the named ranges is written.
 * umoe_engine_prefix_build: runs x_prefix [P][D] ALONE as one row of P tokens (kv_start 0, positions 0 .. P - 1) through the prefill body
 *   -- tiled at P >= 64, ragged below, as the token count selects everywhere -- into cache row 2b of the FREE pair b, then extracts slots
 *   [0, P) into `store`.  The store's bits depend on the prefix and the engine's weights only.  kv_start of row 2b becomes 0.
 *   The host cannot see whether pair b is free: building through a pair that is decoding overwrites its keys and corrupts it.
 * umoe_engine_admit_prefix: umoe_engine_admit of a pair whose rows both begin with the store's P tokens.  valid_host [2][T] is the mask
 *   of the FULL pair (row r: first_r pad columns, its prefix token i in slot first_r + i); x_suffix [2 * (T - P)][D] are columns [P, T)
 *   of the pair's embeddings.  Per row, store tokens [0, max(P - first_r, 0)) are installed into slots [first_r, P); columns [P, T) of
 *   both rows then run the prefill body behind the cached keys (kv slot P + j, positions from the full mask, q_pos0 P) -- in the shorter
 *   row these columns begin with its last first_r prefix tokens, recomputed -- and batch entry b is reset as umoe_engine_admit resets it.
 *   Refused before anything is enqueued: T - P < 2, P < 1, a NULL store, P or 2 * (T - P) beyond the reservation, and whatever
 *   umoe_engine_admit refuses -- a row that is not left padded among it, which is what keeps every installed prefix token valid and
 *   below column P. */
int umoe_kv_prefix_copy(uint16_t* k_cache, uint16_t* v_cache, uint16_t* store, int layers, int rows, int kv_heads, int Lmax, int head_dim,
                        int P, const int32_t* jobs_host, int n_jobs, int extract, umoe_stream_t stream);
int umoe_engine_prefix_build(umoe_engine* e, const umoe_decode_io* io, int b, const uint16_t* x_prefix, int P, uint16_t* store,
                             umoe_stream_t stream);
int umoe_engine_admit_prefix(umoe_engine* e, const umoe_decode_io* io, int b, const uint16_t* store, int P, const uint16_t* x_suffix,
                             const uint8_t* valid_host, int T, int prefill_step, int prefix_len, umoe_stream_t stream);
/* Expert parallel decode (ep_size > 1).  umoe_engine_set_layer then takes exp_gu / exp_dn of the n_real / ep_size LOCAL experts
 * (global ids [ep_rank * E_loc, (ep_rank + 1) * E_loc), core.py:505) and EITHER the row-major tensors of ALL n_real experts (the
 * engine then prefills replicated on its tiled path) OR no row-major expert tensors at all (rm_exp_* NULL: the rank holds its local
 * experts only; prefill through umoe_engine_prefill_external).
 * umoe_engine_ep_region: this rank's exchange region (export with umoe_ep_ipc_export).
 * umoe_engine_ep_connect: peers[p] = rank p's region as mapped in this process (peers[ep_rank] = own base).
 *   mode UMOE_EP_PEER: xGMI peer stores; UMOE_EP_LOOPBACK: single-GPU emulation of ONE rank of an ep_size job for timing
 *   (every peer is this engine itself: tile p of the local slabs stands for rank p; results are not the model's);
 *   UMOE_EP_RCCL: `rccl_comm` (ncclComm_t) carries the same exchange as ncclAllGather + grouped ncclSend/ncclRecv.
 * umoe_engine_ep_error: synchronises `stream` and returns the sticky error word (0 = none; 1 = a receive timed out). */
enum { UMOE_EP_PEER = 0, UMOE_EP_LOOPBACK = 1, UMOE_EP_RCCL = 2 };
int umoe_engine_ep_region(umoe_engine* e, void** base_out, size_t* bytes_out);
int umoe_engine_ep_connect(umoe_engine* e, void* const* peers, void* rccl_comm, int mode);
int umoe_engine_ep_error(umoe_engine* e, umoe_stream_t stream, int* code_out);
/* per-layer probe for parity tests (EAGER decode steps only; capture refuses it).  teach_x [layers][rows][D] bf16 replaces the residual
 * stream at the START of every layer (the layer's input RMSNorm is recomputed from it), so each layer is checked on the oracle's input
 * of that layer without compounding (model.py:210-256 one layer at a time); dump_x1 / dump_x [layers][rows][D] receive the stream after
 * attention + o_proj and after the MoE block, dump_logits [layers][rows][E] the router logits (bf16).  Any pointer may be NULL; all
 * NULL switches the probe off.  With a probe the layer's combine runs as its own launch (it cannot ride in a QKV launch whose input
 * is replaced); every other launch is the decode step's own. */
int umoe_engine_set_probe(umoe_engine* e, const uint16_t* teach_x, uint16_t* dump_x1, uint16_t* dump_x, uint16_t* dump_logits);
/* router dump of ADMISSION passes for parity tests (umoe_engine_admit, umoe_engine_prefix_build, umoe_engine_admit_prefix): after every
 * layer of a pass of at most cap_tok tokens, the expert masks [tokens][E] int32 and the bf16 gate logits [tokens][E] of the pass's tokens
 * are copied to mask_out / logits_out [layers][cap_tok][E] (either may be NULL).  cap_tok 0 switches it off. */
int umoe_engine_set_admit_dump(umoe_engine* e, int32_t* mask_out, uint16_t* logits_out, int cap_tok);
/* host-side facts about the engine: "expert_launch" = what the last dense decode layer enqueued for its experts (0 gate/up and down as
 * two launches, 2 the flat launch moe_flat_kernel, 3 the one-launch expert-parallel MoE half moe_ep_kernel; 1 was the box-grid fused
 * launch, which no longer exists, and is never returned), "n_cu" = compute units the co-residency guards assume; -1 for an unknown key */
int umoe_engine_info(umoe_engine* e, const char* key);
/* introspection for parity tests: device pointers into the workspace */
const void* umoe_engine_buffer(umoe_engine* e, const char* name, size_t* bytes);

/* ------------------------------------------------------------------ optimizer step (umoe_optim.hip; unimoe_audio_amd/optim.py)
 * AdamW with decoupled decay (torch.optim.AdamW, no amsgrad) behind torch.nn.utils.clip_grad_norm_'s rule, on fp32 master weights
 * of bf16 parameters (the reference trains under DeepSpeed's bf16 mode: UniMoEV2-Preview/deepspeed_zero2.conf, script/training.sh:61-72,
 * moe_trainer.py:691-703).  All tensors of all parameter groups go through ONE chunked launch per stage; nothing syncs with the host.
 *
 * Tables (device arrays, packed on the host as plain records: unimoe_audio_amd/optim.py TENSOR_DTYPE / int64 pairs):
 *   umoe_optim_tensor [n_tensors]  one record per parameter tensor, 56 bytes, 8-byte aligned:
 *       p_fp32  a flag word: bit 0 (UMOE_OPTIM_P_FP32) the parameter is fp32 and its own master; bit 1 (UMOE_OPTIM_G_FP32) the gradient
 *               is fp32 whatever the parameter is (an fp32 main gradient of a bf16 parameter: DESIGN 4s).  0 and 1 mean what they did.
 *       p       the parameter: bf16 (bit 0 clear) or fp32 (bit 0 set) [n]
 *       g       its gradient [n], of the parameter's dtype unless bit 1 says fp32; NULL = the tensor is left out of this step (torch:
 *               .grad is None)
 *       master  fp32 master weights [n] (bit 0 clear); ignored for an fp32 parameter, which is updated in place
 *       m, v    fp32 first / second moments [n]
 *       n       element count;  group  index into the per-group settings of umoe_optim_hyper (0 .. num_groups - 1)
 *   umoe_optim_chunk [n_chunks]    (tensor index, first element): the chunk covers elements [first, min(first + chunk_elems, n)) of that
 *       tensor, first a multiple of chunk_elems below n -- so a chunk never crosses its tensor.  chunk_elems: a positive multiple of 8.
 *   The launch entries take the device tables and, optionally, the host arrays they were uploaded from (host_tensors / host_chunks,
 *   both or neither): given, every record is checked before anything is enqueued -- a chunk that crosses its tensor (tensor index out
 *   of range, first < 0, first >= n or not a multiple of chunk_elems), a group index outside the groups, n < 0 are refused.  The
 *   kernels themselves skip a chunk whose record fails these bounds, so a table that was never checked cannot send a workgroup
 *   outside [0, n) of a tensor either.
 * Streams of a tensor that are 16-byte aligned together after the same number of leading elements take 16-byte vector loads and
 * stores with a scalar head and tail (a view at an odd element offset); streams that are not co-aligned take the scalar path whole.
 *
 * Stage 1  umoe_optim_sqsum: partial[c] = sum of squares of chunk c's gradients, fp32, in a fixed order (per thread sequentially over
 *   its 8-element vectors then its head / tail element, xor butterfly within the wave, waves added in order): no atomics, bitwise
 *   reproducible, independent of grid_cap.  flags[c] = 1 when a gradient element (or the fp32 sum) is not finite.  A left-out tensor's
 *   chunks write 0 / 0.
 * Stage 2  umoe_optim_scalars: one workgroup adds the partials in fp64 (thread i its contiguous run of chunks in ascending order,
 *   then the 256 runs in ascending order), reads the step counter t = counters[0] and writes the record:
 *       norm = fp32(sqrt(sum)),  clip = min(1, fp32(max_norm) / (norm + 1e-6f)) in fp32 (1 when max_norm < 0: clipping off),
 *       bc1[g] = fp32(1 - beta1[g]^(t+1)),  bc2[g] = fp32(1 - beta2[g]^(t+1))  (fp64 arithmetic),
 *       skip = 1 when the sum or any flag is not finite.
 *   skip 0: counters[0] = t + 1.  skip 1: counters[1] += 1 and t stays.   partial / flags may be NULL with n_chunks 0.
 * Stage 3  umoe_optim_adamw: reads the record once per workgroup; skip set: returns having written nothing.  Otherwise per element,
 *   fp32, no contraction, correctly rounded division and square root, with b1 = fp32(beta1), omb1 = fp32(1 - beta1) (the difference in
 *   fp64), likewise b2 / omb2, decay = 1 - lr * wd, step = lr / bc1, sq = sqrt(bc2) computed once per workgroup in fp32:
 *       g  = float(grad) * clip
 *       m' = b1 * m + omb1 * g
 *       v' = b2 * v + (omb2 * g) * g
 *       w' = w * decay - (step * m') / (sqrt(v') / sq + eps)
 *   stores w' (master, or the fp32 parameter itself), m', v' and p = bf16_rne(w').
 *   rec NULL (no stage 1 / 2 ran: clipping off and no finite check): t_host >= 0 is the step counter kept by the caller; the bias
 *   corrections are computed from it on the host the same way, clip = 1, nothing is skipped, and counters[0] = t_host + 1 is written
 *   by the launch (counters may be NULL).
 * Refusals (error return, nothing enqueued): NULL tables / outputs, num_groups outside 1..UMOE_OPTIM_MAX_GROUPS, chunk_elems <= 0 or
 * not a multiple of 8, a host table record out of bounds (above).  n_chunks == 0 (an empty table) is a no-op returning 0.
 * grid_cap: most workgroups launched, each striding over the chunk table; 0 = the default (2048). */
#define UMOE_OPTIM_MAX_GROUPS 16
#define UMOE_OPTIM_P_FP32 1
#define UMOE_OPTIM_G_FP32 2
typedef struct {
    void* p;
    const void* g;
    float* master;
    float* m;
    float* v;
    int64_t n;
    int32_t group;
    int32_t p_fp32;
} umoe_optim_tensor;
typedef struct {
    int64_t tensor;
    int64_t first;
} umoe_optim_chunk;
/* what stage 2 leaves for stage 3 (device, 144 bytes) */
typedef struct {
    float norm;
    float clip;
    int32_t skip;
    int32_t reserved;
    float bc1[UMOE_OPTIM_MAX_GROUPS];
    float bc2[UMOE_OPTIM_MAX_GROUPS];
} umoe_optim_record;
/* per-group settings (host; read at every call, so a learning-rate schedule is just another value) */
typedef struct {
    int32_t num_groups;
    int32_t reserved;
    double max_norm;                      /* < 0: clipping off */
    double lr[UMOE_OPTIM_MAX_GROUPS], beta1[UMOE_OPTIM_MAX_GROUPS], beta2[UMOE_OPTIM_MAX_GROUPS], eps[UMOE_OPTIM_MAX_GROUPS],
        wd[UMOE_OPTIM_MAX_GROUPS];
} umoe_optim_hyper;
int umoe_optim_sqsum(const umoe_optim_tensor* tensors, int n_tensors, const umoe_optim_chunk* chunks, int64_t n_chunks, int chunk_elems,
                     const umoe_optim_tensor* host_tensors, const umoe_optim_chunk* host_chunks, int num_groups, int grid_cap,
                     float* partial, int32_t* flags, umoe_stream_t stream);
int umoe_optim_scalars(const float* partial, const int32_t* flags, int64_t n_chunks, const umoe_optim_hyper* hyper, int64_t* counters,
                       umoe_optim_record* rec, umoe_stream_t stream);
int umoe_optim_adamw(const umoe_optim_tensor* tensors, int n_tensors, const umoe_optim_chunk* chunks, int64_t n_chunks, int chunk_elems,
                     const umoe_optim_tensor* host_tensors, const umoe_optim_chunk* host_chunks, int grid_cap,
                     const umoe_optim_hyper* hyper, const umoe_optim_record* rec, int64_t t_host, int64_t* counters,
                     umoe_stream_t stream);

/* Fold of the bf16 gradients autograd still produces (norm weights, biases, the router gate, the embedding tables) into fp32 main
 * gradients, one chunked launch over a table of 24-byte records and a chunk table built as above:
 *       main[i] = main[i] + float(g[i])     (one fp32 add; the bf16 -> fp32 conversion is exact)
 *       g[i]    = +0                        (the same pass clears what it folded)
 * g NULL: the tensor is left out (its main gradient is untouched).  16-byte loads and stores where g and main are 16-byte aligned together
 * after the same number of leading elements, a scalar head and tail, the scalar path whole otherwise.  Each element belongs to one
 * thread, so the result does not depend on grid_cap.  Refusals as for the stages above (host tables checked when given, a record with g
 * but no main included); a refused call enqueues nothing. */
typedef struct {
    uint16_t* g;       /* bf16 [n], or NULL */
    float* main;       /* fp32 [n] */
    int64_t n;
} umoe_optim_fold_tensor;
int umoe_optim_fold(const umoe_optim_fold_tensor* tensors, int n_tensors, const umoe_optim_chunk* chunks, int64_t n_chunks, int chunk_elems,
                    const umoe_optim_fold_tensor* host_tensors, const umoe_optim_chunk* host_chunks, int grid_cap, umoe_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* UMOE_H */
