// Weight-streaming GEMM for a decode step of 17 to 64 rows on ONE GPU: 2, 3 or 4 sixteen-row tiles per pass over a weight.
//
//   Y[tile t][16, N(g)] = epilogue( A[tile t][16, K(g)] * W_g^T )   tile t = rows [16 t, min(16 t + 16, rows)), weights read ONCE
//
// Design (MI355X / gfx950), relative to wstream_gemm (umoe_gemm.hip) and wstream_mt (umoe_gemm_mt.hip):
//  * the WP16 weight stream goes straight into VGPRs (non-temporal 1 KiB wave-loads); there is NO grid dimension over row tiles, every
//    workgroup serves all tiles of the launch with the weight fragments it holds;
//  * the activation tiles arrive in MFMA operand order (pack_rows below re-lays row-major rows, the SwiGLU epilogue writes operand
//    order for the down projection), so a B fragment is one contiguous 1 KiB wave-load from L2: 64 rows at K 2752 are 344 KiB, more
//    than the LDS holds, and no staging pass or barrier stands in front of the stream;
//  * the K split over the WV waves of a workgroup and the fixed-order LDS reduction (wave 0 first) are those of
//    wstream_gemm<.., U, .., WV>: a wave runs its k-steps in ascending order into one accumulator per (tile, block), so every
//    (row, feature) product is BIT-IDENTICAL to the one the 16-row launch with the same (WV, U) computes (tests/test_gpu_wide_gemm.py);
//  * at most 16 (tile, block) accumulators per wave.  Three tiles run the four-tile instantiation: the fourth tile re-reads the third
//    one's fragments from L2 and is never stored (an MT = 3 loop would need block counts per workgroup of its own);
//  * every guard around an MFMA is a scalar branch (wave and slice bounds pinned into SGPRs; tests/test_wide_cpu.py scans the assembly);
//  * groups carry their own n_blocks and K (routed and shared experts in one launch): the grid is a box over the widest group.
// Pad rows of a partial last tile are zero on input (pack_rows, and silu(0) * 0 = 0 behind it) and are never stored row-major.
// Roofline: HBM.  Algorithmic bytes per launch = sum over groups of N*K*2.
//
// One body (wide_body: prologue, K split, fragment pointers, reduction, epilogues), three weight sources.  A source is the argument
// block of its kernel, the blocks a workgroup opens in it, the bias it can supply, and its weight stream: the loop that runs a wave's
// k-steps [i0, i1) in ascending order into acc.  Ring depths, clamps, refill order and the order in which (tile, block) MFMAs issue
// are each source's own.
//  * wide_wp16 (wstream_wide, umoe_gemm_wide): bf16 weights in WP16 order, every launch of the wide step.
//  * wide_wp8 (wstream_wide_f8, umoe_gemm_wide_fp8: the gate/up and down launches of an fp8 engine): WP8 blocks (include/umoe.h).  The
//    rings hold e4m3 bytes, converted to the bf16 MFMA operand right in front of the MFMAs with the row's 2^e (flat_f8_frag), so every
//    output is bit-identical to the bf16 form run on the dequantized weights.  A group with an even number of k-steps streams 16-byte
//    lane loads of two k-steps; a group with an odd number (the shared experts' down projection, 43 k-steps: wave slices start and end
//    on either half of a chunk) streams one 8-byte load per k-step.  The form is a scalar branch per group, so routed and shared groups
//    share one down launch.  No padded k-step is loaded or computed.
//  * wide_wp12 (wstream_wide_w12, umoe_gemm_wide_w12: the same two launches on the lossless 12-bit copies of the bf16 expert weights,
//    include/umoe.h "WP12", unimoe_audio_amd/w12.py).  A register stage holds CS k-steps of one block: 8 CS low bytes + 4 CS code bytes
//    per lane (CS = 2 for an even number of k-steps, 1 for an odd one: the packer chunks by the parity of KB).  The operand is rebuilt
//    ONCE per (block, k-step) and feeds the MFMAs of all row tiles; it is the WP16 operand bit for bit, so every output is the bf16 form's.
#include "umoe_flat_dev.h"      // (umoe_common.h; flat_f8_frag / flat_f8_scale; flat_w12_frag / flat_w12_base4 / flat_w12_cursor / flat_w12_patch)
#include <string.h>

#define UMOE_WIDE_MAXG 12
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

struct wide_args {
    const uint16_t* w[UMOE_WIDE_MAXG];      // WP16 weights of group g (gate/up blocks interleaved for SwiGLU)
    const uint16_t* b[UMOE_WIDE_MAXG];      // operand-order tiles of group g: tile t at b[g] + t * 16 * k[g]
    void* out[UMOE_WIDE_MAXG];              // row-major [rows][ldo] (bf16 / fp32), or operand-order tiles [tiles][16 * I] (SwiGLU)
    const float* bias[UMOE_WIDE_MAXG];      // optional [N] fp32
    const uint16_t* resid[UMOE_WIDE_MAXG];  // UMOE_EPI_BF16_RESID: [rows][ldo]
    int n_blocks[UMOE_WIDE_MAXG], k[UMOE_WIDE_MAXG];
    int num_groups, rows, tiles, ldo, n_valid;
};
struct wide_f8_args {
    const uint8_t* w[UMOE_WIDE_MAXG];       // WP8 weights of group g (gate/up blocks interleaved for SwiGLU)
    const int8_t* exps[UMOE_WIDE_MAXG];     // row exponents, 16 per weight block
    const uint16_t* b[UMOE_WIDE_MAXG];      // operand-order tiles, as wide_args
    void* out[UMOE_WIDE_MAXG];
    int n_blocks[UMOE_WIDE_MAXG], k[UMOE_WIDE_MAXG];
    int num_groups, rows, tiles, ldo, n_valid;
};
struct wide_w12_args {
    const uint8_t* w[UMOE_WIDE_MAXG];       // WP12 blocks of group g (gate/up blocks interleaved for SwiGLU), KB * 768 bytes each
    const uint32_t* meta[UMOE_WIDE_MAXG];   // block records, FLAT_W12_META words per block
    const uint16_t* b[UMOE_WIDE_MAXG];      // operand-order tiles, as wide_args
    void* out[UMOE_WIDE_MAXG];
    int n_blocks[UMOE_WIDE_MAXG], k[UMOE_WIDE_MAXG];
    int num_groups, rows, tiles, ldo, n_valid;
};

// k-step ii of every row tile's fragments: one stage of the fragment ring (L2) that all three weight streams keep
template <int MT>
__device__ __forceinline__ void wide_load_b(u32x4_t (&d)[MT], const u32x4_t* const (&bp)[MT], int ii) {
#pragma unroll
    for (int m = 0; m < MT; ++m) d[m] = bp[m][(size_t)ii * 64];
}

// ---- the weight sources.  open(): the workgroup's blocks nb0 .. nb0 + NT - 1 of group g; stream(): this wave's k-steps [i0, i1) of them
struct wide_wp16 {
    using args = wide_args;
    template <int NT>
    struct blocks { const u32x4_t* wp[NT]; };
    template <int NT>
    static __device__ __forceinline__ blocks<NT> open(const args p, const int g, const int nb0, const int n_blocks, const int KB, const int lane) {
        blocks<NT> w;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int nb = min(nb0 + t, n_blocks - 1);   // tail blocks re-read the last one; never stored
            w.wp[t] = reinterpret_cast<const u32x4_t*>(p.w[g]) + ((size_t)nb * KB) * 64 + lane;
        }
        return w;
    }
    static __device__ __forceinline__ const float* bias(const args p, int g) { return p.bias[g]; }

    template <int NT, int MT, int U, int RW, int RB, bool WREFILL>
    static __device__ __forceinline__ void stream(const blocks<NT> w, const int nb0, const int n_blocks, const int KB, const int lane, const int i0, const int i1,
                                                  const u32x4_t* const (&bp)[MT], f32x4_t (&acc)[MT][NT]) {
        // register rings as in wstream_mt: RW k-steps of weights (HBM) and RB k-steps of fragments (L2) in flight, the fragment refill
        // issued before the weight refill; every load is unconditional with its index clamped into the wave's slice (a wave without
        // k-steps reads step 0 and runs no MFMA)
        u32x4_t wr[RW][NT], br[RB][MT];
        auto load_w = [&](u32x4_t (&d)[NT], int ii) {
#pragma unroll
            for (int t = 0; t < NT; ++t) d[t] = __builtin_nontemporal_load(w.wp[t] + (size_t)ii * 64);
        };
        const int il = max(i1 - 1, 0);
#pragma unroll
        for (int r = 0; r < RB; ++r) wide_load_b(br[r], bp, min(i0 + r, il));
#pragma unroll
        for (int r = 0; r < RW; ++r) load_w(wr[r], min(i0 + r, il));
        __builtin_amdgcn_sched_barrier(0);
        for (int base = i0; base < i1; base += RW) {
#pragma unroll
            for (int r = 0; r < RW; ++r) {
                const int ii = base + r;
                if (ii < i1) {
#pragma unroll
                    for (int m = 0; m < MT; ++m) {
                        const bf16x8_t bfrag = __builtin_bit_cast(bf16x8_t, br[r % RB][m]);
#pragma unroll
                        for (int t = 0; t < NT; ++t)
                            acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, wr[r][t]), bfrag, acc[m][t], 0, 0, 0);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
                wide_load_b(br[r % RB], bp, min(ii + RB, il));
                if constexpr (WREFILL) load_w(wr[r], min(ii + RW, il));   // (WREFILL false: the whole K slice of a wave fits the ring)
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
};

// RW: k-steps the weight ring holds (RW / 2 stages of 16 bytes, or RW stages of 8 bytes for an odd number of k-steps)
struct wide_wp8 {
    using args = wide_f8_args;
    template <int NT>
    struct blocks {
        const u32x4_t* wp[NT];      // the block's first 16-byte chunk (two k-steps)
        const int8_t* ex;           // this lane's row exponent of block 0
    };
    template <int NT>
    static __device__ __forceinline__ blocks<NT> open(const args p, const int g, const int nb0, const int n_blocks, const int KB, const int lane) {
        blocks<NT> w;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int nb = min(nb0 + t, n_blocks - 1);   // tail blocks re-read the last one; never stored
            w.wp[t] = reinterpret_cast<const u32x4_t*>(p.w[g]) + ((size_t)nb * ((KB + 1) >> 1)) * 64 + lane;
        }
        w.ex = p.exps[g] + (lane & 15);
        return w;
    }
    static __device__ __forceinline__ const float* bias(const args, int) { return nullptr; }

    template <int NT, int MT, int U, int RW, int RB, bool WREFILL>
    static __device__ __forceinline__ void stream(const blocks<NT> w, const int nb0, const int n_blocks, const int KB, const int lane, const int i0, const int i1,
                                                  const u32x4_t* const (&bp)[MT], f32x4_t (&acc)[MT][NT]) {
        // the rings of wide_wp16 with e4m3 bytes in the weight stages: CS k-steps per stage (2: one 16-byte load, 1: one 8-byte load).  The fragment
        // ring, the refill order and the clamps are the same; the row exponents are requested behind the first weight stages
        u32x4_t br[RB][MT];
        auto stream = [&](auto cs) {
            constexpr int CS = decltype(cs)::value;
            using WT = std::conditional_t<CS == 2, u32x4_t, flat_u32x2>;
            WT wr[RW / CS][NT];
            auto load_w = [&](WT (&d)[NT], int ii) {      // the stage that starts at k-step ii (CS == 2: ii is even)
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const WT* c = reinterpret_cast<const WT*>(w.wp[t]);
                    d[t] = __builtin_nontemporal_load(CS == 2 ? c + (size_t)(ii >> 1) * 64 : c + (size_t)(ii >> 1) * 128 + (ii & 1));
                }
            };
            const int il = max(i1 - 1, 0), ilw = max(i1 - CS, 0);
#pragma unroll
            for (int r = 0; r < RB; ++r) wide_load_b(br[r], bp, min(i0 + r, il));
#pragma unroll
            for (int r = 0; r < RW / CS; ++r) load_w(wr[r], min(i0 + CS * r, ilw));
            float sc[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) sc[t] = flat_f8_scale(w.ex[min(nb0 + t, n_blocks - 1) * 16]);
            __builtin_amdgcn_sched_barrier(0);
            for (int base = i0; base < i1; base += RW) {
#pragma unroll
                for (int r = 0; r < RW; ++r) {
                    const int ii = base + r;
                    if (ii < i1) {
                        bf16x8_t wf[NT];
#pragma unroll
                        for (int t = 0; t < NT; ++t) wf[t] = flat_f8_frag(wr[r / CS][t][2 * (r % CS)], wr[r / CS][t][2 * (r % CS) + 1], sc[t]);
#pragma unroll
                        for (int m = 0; m < MT; ++m) {
                            const bf16x8_t bfrag = __builtin_bit_cast(bf16x8_t, br[r % RB][m]);
#pragma unroll
                            for (int t = 0; t < NT; ++t) acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[t], bfrag, acc[m][t], 0, 0, 0);
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    wide_load_b(br[r % RB], bp, min(ii + RB, il));
                    if constexpr (WREFILL)
                        if (r % CS == CS - 1) load_w(wr[r / CS], min(ii - (CS - 1) + RW, ilw));
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        };
        // (U == 1: the host admits only K whose wave slices are whole chunks)
        if (U == 2 && (KB & 1)) stream(std::integral_constant<int, 1>{});
        else stream(std::integral_constant<int, 2>{});
    }
};

// RW: k-steps the weight ring holds (RW / 2 stages of 16 + 8 bytes, or RW stages of 8 + 4 bytes for an odd number of k-steps)
struct wide_wp12 {
    using args = wide_w12_args;
    template <int NT>
    struct blocks {
        const char* wp[NT];         // the block: KB * 512 low bytes, then KB * 256 code bytes
        uint32_t mt[NT];            // the block records: lane l holds word min(l, 39)
    };
    template <int NT>
    static __device__ __forceinline__ blocks<NT> open(const args p, const int g, const int nb0, const int n_blocks, const int KB, const int lane) {
        blocks<NT> w;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int nb = min(nb0 + t, n_blocks - 1);   // tail blocks re-read the last one (weights and record); never stored
            w.wp[t] = reinterpret_cast<const char*>(p.w[g]) + (size_t)nb * ((size_t)KB * 768);
            w.mt[t] = p.meta[g][(size_t)nb * FLAT_W12_META + min(lane, FLAT_W12_META - 1)];      // (in front of the first stage: the first MFMA needs it)
        }
        return w;
    }
    static __device__ __forceinline__ const float* bias(const args, int) { return nullptr; }

    template <int NT, int MT, int U, int RW, int RB, bool WREFILL>
    static __device__ __forceinline__ void stream(const blocks<NT> w, const int nb0, const int n_blocks, const int KB, const int lane, const int i0, const int i1,
                                                  const u32x4_t* const (&bp)[MT], f32x4_t (&acc)[MT][NT]) {
        static_assert(RW % 2 == 0, "whole 2-step stages");
        // the rings of wide_wp16 with WP12 stages in the weight ring: 3 dwords per block and k-step.  The fragment ring, the refill order
        // and the clamps are the same
        u32x4_t br[RB][MT];
        auto stream = [&](auto cs) {
            constexpr int CS = decltype(cs)::value;
            using WT = std::conditional_t<CS == 2, u32x4_t, flat_u32x2>;      // the low bytes of a stage
            using CT = std::conditional_t<CS == 2, flat_u32x2, uint32_t>;     // its code words
            WT wr[RW / CS][NT];
            CT wc[RW / CS][NT];
            const size_t code0 = (size_t)KB * 512;
            auto load_w = [&](WT (&d)[NT], CT (&c)[NT], int ii) {             // the stage that starts at k-step ii (CS == 2: ii is even)
                const size_t slot = (size_t)(ii / CS) * 64 + lane;            // [chunk][lane]: 8 CS low bytes, 4 CS code bytes
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    d[t] = __builtin_nontemporal_load(reinterpret_cast<const WT*>(w.wp[t]) + slot);
                    c[t] = __builtin_nontemporal_load(reinterpret_cast<const CT*>(w.wp[t] + code0) + slot);
                }
            };
            const int il = max(i1 - 1, 0), ilw = max(i1 - CS, 0);
#pragma unroll
            for (int r = 0; r < RB; ++r) wide_load_b(br[r], bp, min(i0 + r, il));
#pragma unroll
            for (int r = 0; r < RW / CS; ++r) load_w(wr[r], wc[r], min(i0 + CS * r, ilw));
            // the exception cursor (entries of k-steps below the wave's i0 skipped) and the window base of every block: scalar registers
            uint32_t xs[NT], wb4[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                xs[t] = flat_w12_cursor(w.mt[t], i0, lane);
                wb4[t] = flat_w12_base4(w.mt[t]);
            }
            __builtin_amdgcn_sched_barrier(0);
            for (int base = i0; base < i1; base += RW) {
#pragma unroll
                for (int r = 0; r < RW; ++r) {
                    const int ii = base + r;
                    if (ii < i1) {
#pragma unroll
                        for (int t = 0; t < NT; ++t) {
                            uint32_t cw;
                            if constexpr (CS == 2) cw = wc[r / CS][t][r % CS]; else cw = wc[r][t];
                            flat_u32x4 o = flat_w12_frag(wr[r / CS][t][2 * (r % CS)], wr[r / CS][t][2 * (r % CS) + 1], cw, wb4[t]);
                            if ((xs[t] & 0xffu) == (uint32_t)ii) flat_w12_patch(o, w.mt[t], xs[t], (uint32_t)ii, lane);
                            const bf16x8_t wf = __builtin_bit_cast(bf16x8_t, o);
#pragma unroll
                            for (int m = 0; m < MT; ++m)
                                acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, __builtin_bit_cast(bf16x8_t, br[r % RB][m]), acc[m][t], 0, 0, 0);
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    wide_load_b(br[r % RB], bp, min(ii + RB, il));
                    if constexpr (WREFILL)
                        if (r % CS == CS - 1) load_w(wr[r / CS], wc[r / CS], min(ii - (CS - 1) + RW, ilw));
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        };
        // (U == 1: the host admits only K whose wave slices are whole chunks)
        if (U == 2 && (KB & 1)) stream(std::integral_constant<int, 1>{});
        else stream(std::integral_constant<int, 2>{});
    }
};

// ---- the body of every wide kernel: what decides the bits around a source's weight stream
template <class SRC, int NT, int MT, int U, int WV, int EPI, int RW, int RB, bool WREFILL>
__device__ __forceinline__ void wide_body(const typename SRC::args p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int g = blockIdx.z, nb0 = blockIdx.x * NT;
    const int n_blocks = p.n_blocks[g];
    if (nb0 >= n_blocks) return;
    const int K = p.k[g], KB = K >> 5;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar: every guard around an MFMA must be a scalar branch
    // K split of wstream_gemm<.., U, .., WV>: whole U-step chunks per wave when they divide, single steps otherwise
    int i0, i1;
    if (KB % U == 0) {
        const int units = KB / U;
        i0 = U * ((units * wave) / WV);
        i1 = U * ((units * (wave + 1)) / WV);
    } else {
        i0 = (KB * wave) / WV;
        i1 = (KB * (wave + 1)) / WV;
    }
    i0 = __builtin_amdgcn_readfirstlane(i0);
    i1 = __builtin_amdgcn_readfirstlane(i1);
    // (the source opens its blocks here, beside p.b[g] and p.tiles, so that one wait covers the scalar loads of the prologue -- read where
    // the stream first uses them the group's pointers cost two more round trips, 0.4 us on the 10 us QKV and o_proj launches -- and a
    // WP12 record is requested first of all)
    const auto w = SRC::template open<NT>(p, g, nb0, n_blocks, KB, lane);
    const u32x4_t* bp[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int mm = min(m, p.tiles - 1);          // (three tiles: the fourth re-reads the third; never stored)
        bp[m] = reinterpret_cast<const u32x4_t*>(p.b[g]) + ((size_t)mm * KB) * 64 + lane;
    }
    f32x4_t acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[m][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    SRC::template stream<NT, MT, U, RW, RB, WREFILL>(w, nb0, n_blocks, KB, lane, i0, i1, bp, acc);
    // ---- fixed-order cross-wave reduction (wave 0 first, as in wstream_gemm) --------------------------------------------
    f32x4_t* red = reinterpret_cast<f32x4_t*>(smem);
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int t = 0; t < NT; ++t) red[((wave * MT + m) * NT + t) * 64 + lane] = acc[m][t];
    __syncthreads();
    auto reduced = [&](int m, int t) -> f32x4_t {
        f32x4_t s = red[(m * NT + t) * 64 + lane];
#pragma unroll
        for (int w = 1; w < WV; ++w) {
            const f32x4_t v = red[((w * MT + m) * NT + t) * 64 + lane];
            s[0] += v[0]; s[1] += v[1]; s[2] += v[2]; s[3] += v[3];
        }
        return s;
    };
    const int h = lane >> 4, mm = lane & 15;   // lane (h, mm) owns features 4h..4h+3 of token row mm of every tile
    if constexpr (EPI == UMOE_EPI_SWIGLU) {
        const int I = n_blocks * 8, Q = I >> 2;             // intermediate size and its K-quarter for the down projection
        for (int q = wave; q < MT * (NT / 2); q += WV) {
            const int m = q / (NT / 2), pq = q % (NT / 2);
            if (m >= p.tiles || nb0 + 2 * pq >= n_blocks) continue;
            const f32x4_t ga = reduced(m, 2 * pq), ua = reduced(m, 2 * pq + 1);
            uint16_t y[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float gt = rbf(ga[j]);
                const float up = rbf(ua[j]);
                const float si = rbf(gt / (1.0f + expf(-gt)));
                y[j] = f2bf(si * up);
            }
            // feature f..f+3 of row mm -> operand order of the [16][I] tile: fragment (k-step i, lane = quarter*16 + row), element j
            // (pad rows of the last tile are written too: zero rows in give silu(0) * 0 = 0, the down projection reads zeros)
            const int f = (nb0 / 2 + pq) * 16 + 4 * h;
            const int qq = f / Q, r = f % Q;
            uint16_t* o = reinterpret_cast<uint16_t*>(p.out[g]) + (size_t)m * 16 * I + ((size_t)(r >> 3) * 64 + qq * 16 + mm) * 8 + (r & 7);
            *reinterpret_cast<uint2*>(o) = make_uint2((uint32_t)y[0] | ((uint32_t)y[1] << 16), (uint32_t)y[2] | ((uint32_t)y[3] << 16));
        }
    } else {
        // (read once: with p.n_valid in every guard the compiler does not see that `fast` excludes the per-element stores, and splits the
        // 8-byte store of the fast path into a dword and two shorts)
        const int n_valid = p.n_valid;
        const float* gbias = SRC::bias(p, g);   // (a source without bias: a compile-time null, the sum below is a4[j] + 0.f)
        for (int q = wave; q < MT * NT; q += WV) {
            const int m = q / NT, t = q % NT;
            const int row = m * 16 + mm;
            if (m >= p.tiles || nb0 + t >= n_blocks || row >= p.rows) continue;      // pad rows are never stored
            const f32x4_t a4 = reduced(m, t);
            const int n = (nb0 + t) * 16 + 4 * h;
            if (n >= n_valid) continue;
            const bool fast = n + 3 < n_valid;
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = a4[j] + ((gbias && n + j < n_valid) ? gbias[n + j] : 0.f);   // (+ 0.f without bias, as the 16-row kernel: -0 -> +0)
            const size_t off = (size_t)row * p.ldo + n;
            if constexpr (EPI == UMOE_EPI_F32) {
                float* o = reinterpret_cast<float*>(p.out[g]) + off;
                if (fast) {
                    *reinterpret_cast<float4*>(o) = make_float4(rbf(v[0]), rbf(v[1]), rbf(v[2]), rbf(v[3]));
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (n + j < n_valid) o[j] = rbf(v[j]);
                }
            } else {
                uint16_t* o = reinterpret_cast<uint16_t*>(p.out[g]) + off;
                uint16_t y[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float x = rbf(v[j]);
                    if constexpr (EPI == UMOE_EPI_BF16_RESID)
                        if (n + j < n_valid) x = bf2f(p.resid[g][off + j]) + x;
                    y[j] = f2bf(x);
                }
                if (fast) {
                    *reinterpret_cast<uint2*>(o) = make_uint2((uint32_t)y[0] | ((uint32_t)y[1] << 16), (uint32_t)y[2] | ((uint32_t)y[3] << 16));
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (n + j < n_valid) o[j] = y[j];
                }
            }
        }
    }
}

template <int NT, int MT, int U, int WV, int EPI, int RW, int RB, bool WREFILL>
__global__ __launch_bounds__(WV * 64, 1) void wstream_wide(const wide_args p) {
    wide_body<wide_wp16, NT, MT, U, WV, EPI, RW, RB, WREFILL>(p);
}
template <int NT, int MT, int U, int WV, int EPI, int RW, int RB, bool WREFILL>
__global__ __launch_bounds__(WV * 64, 1) void wstream_wide_f8(const wide_f8_args p) {
    static_assert(EPI == UMOE_EPI_SWIGLU || EPI == UMOE_EPI_BF16, "the fp8 form runs the gate/up and the down launch");
    wide_body<wide_wp8, NT, MT, U, WV, EPI, RW, RB, WREFILL>(p);
}
template <int NT, int MT, int U, int WV, int EPI, int RW, int RB, bool WREFILL>
__global__ __launch_bounds__(WV * 64, 1) void wstream_wide_w12(const wide_w12_args p) {
    static_assert(EPI == UMOE_EPI_SWIGLU || EPI == UMOE_EPI_BF16, "the WP12 form runs the gate/up and the down launch");
    wide_body<wide_wp12, NT, MT, U, WV, EPI, RW, RB, WREFILL>(p);
}

template <int NT, int MT, int U, int WV, int EPI, int RW, int RB, bool WREFILL, typename ARGS>
static int launch_wide_v(const ARGS& a, int max_nb, hipStream_t s) {
    const size_t lds = (size_t)WV * MT * NT * 64 * 16;
    void (*kernel)(const ARGS);
    if constexpr (std::is_same_v<ARGS, wide_f8_args>) kernel = &wstream_wide_f8<NT, MT, U, WV, EPI, RW, RB, WREFILL>;
    else if constexpr (std::is_same_v<ARGS, wide_w12_args>) kernel = &wstream_wide_w12<NT, MT, U, WV, EPI, RW, RB, WREFILL>;
    else kernel = &wstream_wide<NT, MT, U, WV, EPI, RW, RB, WREFILL>;
    static bool configured = false;
    if (!configured) {
        UMOE_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        configured = true;
    }
    const dim3 grid((unsigned)ceil_div(max_nb, NT), 1, (unsigned)a.num_groups);
    kernel<<<grid, WV * 64, lds, s>>>(a);
    UMOE_LAUNCH_CHECK();
    return 0;
}

template <int NT, int MT, int U, int WV, int EPI, int RW, int RB, typename ARGS>
static int launch_wide(const ARGS& a, hipStream_t s) {
    // k-steps of the longest wave slice over the groups: no weight refill when the ring holds them all
    int longest = 0, max_nb = 0;
    for (int g = 0; g < a.num_groups; ++g) {
        const int KB = a.k[g] >> 5;
        const int l = (KB % U == 0) ? U * ceil_div(KB / U, WV) : ceil_div(KB, WV);
        longest = l > longest ? l : longest;
        max_nb = a.n_blocks[g] > max_nb ? a.n_blocks[g] : max_nb;
    }
    if (longest <= RW) return launch_wide_v<NT, MT, U, WV, EPI, RW, RB, false>(a, max_nb, s);
    return launch_wide_v<NT, MT, U, WV, EPI, RW, RB, true>(a, max_nb, s);
}

// What the three entries refuse alike, and the fields of the argument block they fill alike.  fn: the entry point; w_name: its weight
// argument (host_w / host_w8 / host_w12), of which host_w is the pointer list; small: whose launch 16 rows and fewer are.
template <typename ARGS, typename W>
static int wide_fill(ARGS& a, const char* fn, const char* w_name, const char* small, const W* const* host_w, const int* host_n_blocks, const int* host_k,
                     int num_groups, int rows, const uint16_t* const* host_b, void* const* host_out, int ldo, int n_valid, bool swiglu) {
    UMOE_REQUIRE(host_w && host_n_blocks && host_k && host_b && host_out, "%s: null argument", fn);
    UMOE_REQUIRE(num_groups >= 1 && num_groups <= UMOE_WIDE_MAXG, "%s: 1..%d groups (got %d)", fn, UMOE_WIDE_MAXG, num_groups);
    UMOE_REQUIRE(rows > 16 && rows <= 64, "%s: 17..64 rows (got %d): 16 rows and fewer are %s", fn, rows, small);
    memset(&a, 0, sizeof(a));
    a.num_groups = num_groups; a.rows = rows; a.tiles = ceil_div(rows, 16); a.ldo = ldo; a.n_valid = n_valid;
    for (int g = 0; g < num_groups; ++g) {
        a.w[g] = host_w[g]; a.b[g] = host_b[g]; a.out[g] = host_out[g];
        a.n_blocks[g] = host_n_blocks[g]; a.k[g] = host_k[g];
        UMOE_REQUIRE(a.w[g], "%s: group %d: %s holds a null pointer", fn, g, w_name);
        UMOE_REQUIRE(a.b[g] && a.out[g], "%s: group %d lacks input tiles (host_b) or an output (host_out)", fn, g);
        UMOE_REQUIRE(((uintptr_t)a.w[g] & 15) == 0, "%s: group %d: %s must be 16-byte aligned (16-byte vector loads)", fn, g, w_name);
        UMOE_REQUIRE((((uintptr_t)a.b[g] | (uintptr_t)a.out[g]) & 15) == 0,
                     "%s: group %d: input tiles (host_b) and output (host_out) must be 16-byte aligned (16-byte vector accesses)", fn, g);
        UMOE_REQUIRE(a.k[g] > 0 && a.k[g] % 32 == 0 && a.n_blocks[g] > 0, "%s: group %d: host_k %% 32 == 0, host_n_blocks > 0 (K=%d n_blocks=%d)", fn, g, a.k[g],
                     a.n_blocks[g]);
        UMOE_REQUIRE(!swiglu || a.n_blocks[g] % 4 == 0, "%s: SwiGLU needs gate/up block pairs and I %% 32 == 0 (group %d: host_n_blocks %d)", fn, g, a.n_blocks[g]);
        UMOE_REQUIRE(swiglu || (ldo % 4 == 0 && n_valid > 0 && n_valid <= ldo), "%s: row-major outputs need ldo %% 4 == 0 and 0 < n_valid <= ldo (ldo=%d n_valid=%d)",
                     fn, ldo, n_valid);
    }
    return 0;
}

// blocks per workgroup (NT) by epilogue and tiles: the launcher's choice, restated by tests/test_gpu_wide_gemm.py
extern "C" int umoe_gemm_wide(const uint16_t* const* host_w, const int* host_n_blocks, const int* host_k, int num_groups, int rows,
                              const uint16_t* const* host_b, void* const* host_out, int ldo, int n_valid, const float* const* host_bias,
                              const uint16_t* const* host_resid, int epilogue, int waves, int u, umoe_stream_t stream) {
    const bool swiglu = epilogue == UMOE_EPI_SWIGLU;
    wide_args a;
    if (const int rc = wide_fill(a, "umoe_gemm_wide", "host_w", "umoe_grouped_gemm's", host_w, host_n_blocks, host_k, num_groups, rows, host_b, host_out, ldo,
                                 n_valid, swiglu))
        return rc;
    for (int g = 0; g < num_groups; ++g) {
        a.bias[g] = host_bias ? host_bias[g] : nullptr;
        a.resid[g] = host_resid ? host_resid[g] : nullptr;
        UMOE_REQUIRE(((uintptr_t)a.resid[g] & 15) == 0 && ((uintptr_t)a.bias[g] & 3) == 0,
                     "umoe_gemm_wide: group %d: the residual must be 16-byte aligned (16-byte vector accesses), the bias 4-byte aligned", g);
        UMOE_REQUIRE(epilogue != UMOE_EPI_BF16_RESID || a.resid[g], "umoe_gemm_wide: residual epilogue needs resid (group %d)", g);
    }
    hipStream_t s = (hipStream_t)stream;
    const bool two = a.tiles == 2;
    // one instantiation per (epilogue, WV, U) of the 16-row decode step (launch_gemm_nt / the SwiGLU switch of umoe_grouped_gemm)
    if (waves == 4 && u == 16 && epilogue == UMOE_EPI_BF16)         // QKV (+ bias)
        return two ? launch_wide<1, 2, 16, 4, UMOE_EPI_BF16, 16, 4>(a, s) : launch_wide<1, 4, 16, 4, UMOE_EPI_BF16, 16, 4>(a, s);
    if (waves == 4 && u == 16 && epilogue == UMOE_EPI_BF16_RESID)   // o_proj (+ residual)
        return two ? launch_wide<1, 2, 16, 4, UMOE_EPI_BF16_RESID, 16, 4>(a, s) : launch_wide<1, 4, 16, 4, UMOE_EPI_BF16_RESID, 16, 4>(a, s);
    if (waves == 4 && u == 8 && epilogue == UMOE_EPI_F32)           // codec head (512..1023 blocks in the 16-row launch: 2 per workgroup)
        return two ? launch_wide<2, 2, 8, 4, UMOE_EPI_F32, 8, 4>(a, s) : launch_wide<2, 4, 8, 4, UMOE_EPI_F32, 8, 4>(a, s);
    if (waves == 4 && u == 16 && epilogue == UMOE_EPI_F32)          // a small head (< 512 blocks: 1 per workgroup there)
        return two ? launch_wide<1, 2, 16, 4, UMOE_EPI_F32, 16, 4>(a, s) : launch_wide<1, 4, 16, 4, UMOE_EPI_F32, 16, 4>(a, s);
    if (waves == 4 && u == 2 && epilogue == UMOE_EPI_F32)           // a large head (>= 1024 blocks: 8 per workgroup there)
        return two ? launch_wide<2, 2, 2, 4, UMOE_EPI_F32, 8, 4>(a, s) : launch_wide<2, 4, 2, 4, UMOE_EPI_F32, 8, 4>(a, s);
    if (waves == 8 && u == 1 && swiglu)                             // gate/up
        return two ? launch_wide<8, 2, 1, 8, UMOE_EPI_SWIGLU, 4, 2>(a, s) : launch_wide<4, 4, 1, 8, UMOE_EPI_SWIGLU, 8, 2>(a, s);
    if (waves == 8 && u == 2 && epilogue == UMOE_EPI_BF16)          // down
        return two ? launch_wide<2, 2, 2, 8, UMOE_EPI_BF16, 8, 4>(a, s) : launch_wide<1, 4, 2, 8, UMOE_EPI_BF16, 8, 4>(a, s);
    UMOE_REQUIRE(false,
                 "umoe_gemm_wide: (epilogue, waves, u) must be one of the decode step's: (bf16 | bf16+resid, 4, 16), (fp32, 4, 16 | 8 | 2), (SwiGLU, 8, 1), "
                 "(bf16, 8, 2) (got %d, %d, %d)",
                 epilogue, waves, u);
}

// The gate/up and down launches of the wide step on WP8 weights: (SwiGLU, 8, 1) and (bf16, 8, 2), tiles and K split as above.  Ring depths
// (DESIGN 4i): a k-step is half the registers of the bf16 form's, so the rings of down (12 k-steps) and of gate/up at three or four tiles
// (8) hold a wave's whole K slice of the decode shapes and are never refilled; gate/up at two tiles (8 blocks per workgroup) keeps the
// bf16 form's 4 k-steps -- 6 and 8 spill.
extern "C" int umoe_gemm_wide_fp8(const uint8_t* const* host_w8, const int8_t* const* host_exps, const int* host_n_blocks, const int* host_k,
                                  int num_groups, int rows, const uint16_t* const* host_b, void* const* host_out, int ldo, int n_valid,
                                  int epilogue, int waves, int u, umoe_stream_t stream) {
    UMOE_REQUIRE(host_exps, "umoe_gemm_wide_fp8: null argument");
    const bool swiglu = epilogue == UMOE_EPI_SWIGLU && waves == 8 && u == 1, down = epilogue == UMOE_EPI_BF16 && waves == 8 && u == 2;
    UMOE_REQUIRE(swiglu || down, "umoe_gemm_wide_fp8: (epilogue, waves, u) must be the gate/up or the down launch's: (SwiGLU, 8, 1), (bf16, 8, 2) (got %d, %d, %d)",
                 epilogue, waves, u);
    wide_f8_args a;
    if (const int rc = wide_fill(a, "umoe_gemm_wide_fp8", "host_w8", "the fp8 flat expert launch's", host_w8, host_n_blocks, host_k, num_groups, rows, host_b,
                                 host_out, ldo, n_valid, swiglu))
        return rc;
    for (int g = 0; g < num_groups; ++g) {
        a.exps[g] = host_exps[g];
        UMOE_REQUIRE(a.exps[g], "umoe_gemm_wide_fp8: group %d lacks exponents (host_exps)", g);
        // u = 1 splits K in single steps: only when every wave boundary K / 32 * w / 8 is even is a slice whole 16-byte chunks (u = 2 serves
        // every K: whole chunks for an even number of k-steps, 8-byte loads for an odd one)
        UMOE_REQUIRE(!swiglu || a.k[g] % 512 == 0, "umoe_gemm_wide_fp8: the gate/up launch needs K %% 512 == 0 (group %d: K=%d): no padded k-step is computed", g,
                     a.k[g]);
    }
    hipStream_t s = (hipStream_t)stream;
    const bool two = a.tiles == 2;
    if (swiglu) return two ? launch_wide<8, 2, 1, 8, UMOE_EPI_SWIGLU, 4, 2>(a, s) : launch_wide<4, 4, 1, 8, UMOE_EPI_SWIGLU, 8, 2>(a, s);
    return two ? launch_wide<2, 2, 2, 8, UMOE_EPI_BF16, 12, 4>(a, s) : launch_wide<1, 4, 2, 8, UMOE_EPI_BF16, 12, 4>(a, s);
}

// The gate/up and down launches of the wide step on WP12 weights: (SwiGLU, 8, 1) and (bf16, 8, 2), tiles and K split as above.  Blocks per
// workgroup and ring depths: a k-step is 3 dwords per block, so gate/up takes 4 blocks per workgroup at every tile count and a
// ring of 8 k-steps (a wave's whole K slice at K 2048: never refilled there; measured against 8 blocks with a refilled ring of 4 k-steps
// at two tiles: 44.3 vs 45.6 us per launch); down keeps the bf16 form's blocks with a ring of 12 k-steps (a wave's whole slice of 86 k-steps).
extern "C" int umoe_gemm_wide_w12(const uint8_t* const* host_w12, const uint32_t* const* host_meta, const int* host_n_blocks, const int* host_k,
                                  int num_groups, int rows, const uint16_t* const* host_b, void* const* host_out, int ldo, int n_valid,
                                  int epilogue, int waves, int u, umoe_stream_t stream) {
    UMOE_REQUIRE(host_meta, "umoe_gemm_wide_w12: null argument");
    const bool swiglu = epilogue == UMOE_EPI_SWIGLU && waves == 8 && u == 1, down = epilogue == UMOE_EPI_BF16 && waves == 8 && u == 2;
    UMOE_REQUIRE(swiglu || down, "umoe_gemm_wide_w12: (epilogue, waves, u) must be the gate/up or the down launch's: (SwiGLU, 8, 1), (bf16, 8, 2) (got %d, %d, %d)",
                 epilogue, waves, u);
    wide_w12_args a;
    if (const int rc = wide_fill(a, "umoe_gemm_wide_w12", "host_w12", "the WP12 flat expert launch's", host_w12, host_n_blocks, host_k, num_groups, rows, host_b,
                                 host_out, ldo, n_valid, swiglu))
        return rc;
    for (int g = 0; g < num_groups; ++g) {
        a.meta[g] = host_meta[g];
        UMOE_REQUIRE(a.meta[g], "umoe_gemm_wide_w12: group %d: host_meta holds a null pointer", g);
        UMOE_REQUIRE(((uintptr_t)a.meta[g] & 3) == 0, "umoe_gemm_wide_w12: group %d: host_meta must be 4-byte aligned", g);
        UMOE_REQUIRE(a.k[g] / 32 < 127, "umoe_gemm_wide_w12: group %d: host_k / 32 < 127 (K=%d): a block record counts k-steps in 7 bits", g, a.k[g]);
        // u = 1 splits K in single steps: only when every wave boundary K / 32 * w / 8 is even is a slice whole 2-step chunks (u = 2 serves
        // every K: whole chunks for an even number of k-steps, 1-step chunks for an odd one)
        UMOE_REQUIRE(!swiglu || a.k[g] % 512 == 0, "umoe_gemm_wide_w12: the gate/up launch needs host_k %% 512 == 0 (group %d: K=%d): every wave slice whole chunks", g,
                     a.k[g]);
    }
    hipStream_t s = (hipStream_t)stream;
    const bool two = a.tiles == 2;
    if (swiglu) return two ? launch_wide<4, 2, 1, 8, UMOE_EPI_SWIGLU, 8, 2>(a, s) : launch_wide<4, 4, 1, 8, UMOE_EPI_SWIGLU, 8, 2>(a, s);
    return two ? launch_wide<2, 2, 2, 8, UMOE_EPI_BF16, 12, 4>(a, s) : launch_wide<1, 4, 2, 8, UMOE_EPI_BF16, 12, 4>(a, s);
}

// ------------------------------------------------------------------------------------ operand-order producers
// Rows [rows][K] row-major -> WP16 tiles of [16][K] (include/umoe.h): tile t at packed + t * 16 * K, pad rows of the last tile ZERO (their
// source is never read).  One workgroup of 256 threads per tile row.  NORM: the RMSNorm of router4_body (umoe_router_dev.h) in front,
// the same arithmetic bit for bit -- thread (wave, lane) holds the 16-byte chunks (4 n + wave) * 64 + lane, sums their squares in element
// order, xor-butterfly 32 .. 1, the four wave sums added in order, value = bf16(w * bf16(x * rs)).
template <bool NORM>
__global__ __launch_bounds__(256) void pack_rows_kernel(const uint16_t* __restrict__ x, int lda, int rows, int K, const uint16_t* __restrict__ norm_w,
                                                        float rms_eps, uint16_t* __restrict__ packed) {
    __shared__ float ss_part[4];
    const int r = blockIdx.x, t = r >> 4, m = r & 15, tid = threadIdx.x;
    const int KB = K >> 5;      // 16-byte chunks per K-quarter
    uint16_t* dst = packed + (size_t)t * 16 * K;
    auto chunk_dst = [&](int c) { return dst + ((size_t)(c % KB) * 64 + (c / KB) * 16 + m) * 8; };
    if (r >= rows) {            // (uniform per workgroup)
        for (int c = tid; c < 4 * KB; c += 256) st16(chunk_dst(c), make_uint4(0, 0, 0, 0));
        return;
    }
    const uint16_t* xr = x + (size_t)r * lda;
    if constexpr (!NORM) {
        for (int c = tid; c < 4 * KB; c += 256) st16(chunk_dst(c), ld16(xr + c * 8));
    } else {
        const int lane = tid & 63, wave = tid >> 6;
        const int nch = K >> 11;    // chunks per thread: 1 or 2
        uint4 xv[2], nw[2];
#pragma unroll
        for (int n = 0; n < 2; ++n)
            if (n < nch) {
                const int c = (n * 4 + wave) * 64 + lane;
                xv[n] = ld16(xr + c * 8);
                nw[n] = ld16(norm_w + c * 8);
            }
        float ss = 0.f;
#pragma unroll
        for (int n = 0; n < 2; ++n)
            if (n < nch) {
                float f[8];
                unpack8(xv[n], f);
#pragma unroll
                for (int j = 0; j < 8; ++j) ss += f[j] * f[j];
            }
        ss = wave_sum(ss);
        if (lane == 0) ss_part[wave] = ss;
        __syncthreads();
        ss = ((ss_part[0] + ss_part[1]) + ss_part[2]) + ss_part[3];
        const float rs = rsqrtf(ss / (float)K + rms_eps);
#pragma unroll
        for (int n = 0; n < 2; ++n)
            if (n < nch) {
                const int c = (n * 4 + wave) * 64 + lane;
                float f[8], w[8];
                unpack8(xv[n], f);
                unpack8(nw[n], w);
#pragma unroll
                for (int j = 0; j < 8; ++j) f[j] = rbf(w[j] * rbf(f[j] * rs));
                st16(chunk_dst(c), pack8(f));
            }
    }
}

extern "C" int umoe_pack_rows(const uint16_t* x, int lda, int rows, int k, const uint16_t* norm_w, float rms_eps, uint16_t* packed,
                              umoe_stream_t stream) {
    UMOE_REQUIRE(x && packed && rows > 0 && rows <= 65535 * 16 && k > 0 && k % 32 == 0 && lda >= k && lda % 8 == 0,
                 "umoe_pack_rows: need rows > 0, K %% 32 == 0, lda >= K, lda %% 8 == 0 (rows=%d K=%d lda=%d)", rows, k, lda);
    UMOE_REQUIRE((((uintptr_t)x | (uintptr_t)packed | (uintptr_t)norm_w) & 15) == 0, "umoe_pack_rows: x, packed and norm_w must be 16-byte aligned");
    UMOE_REQUIRE(!norm_w || k == 2048 || k == 4096, "umoe_pack_rows: the RMSNorm form needs K 2048 or 4096 (got %d)", k);
    const dim3 grid((unsigned)(ceil_div(rows, 16) * 16));
    if (norm_w) pack_rows_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>(x, lda, rows, k, norm_w, rms_eps, packed);
    else pack_rows_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>(x, lda, rows, k, nullptr, 0.f, packed);
    UMOE_LAUNCH_CHECK();
    return 0;
}
