// Device side of the flat expert launch (umoe_moe_flat.hip) shared with the expert-parallel flat launch (umoe_moe_ep.hip): the argument
// block, the LDS tile layout, the bounded flag wait and the two slice bodies (gate/up SwiGLU, down projection) whose tiles, K split and
// reduction order are those of wstream_body<14, 1, PLAIN, SWIGLU, 8> / <6, 2, PLAIN, BF16, 8> (umoe_gemm.hip) -- bit-identical outputs whichever launch computes a tile.
#pragma once
#include "umoe_common.h"
#include "umoe_router_dev.h"

#include <type_traits>

#define FLAT_MAXG UMOE_GROUPS_INLINE
#define FLAT_MAXWG 256
#define FLAT_NP_MIN 4
#define FLAT_NP_MAX 7
#define FLAT_ND_MAX2 6      // blocks of one down slice, 2-step chunks (even number of k-steps: the routed experts)
#define FLAT_ND_MAX1 10     // ... 1-step chunks (odd number of k-steps: the shared experts, half the bytes per block)
#define FLAT_SLICES 2       // down slices per workgroup

struct flat_args {
    // (what the first weight request needs sits at the front: one batch of kernel-argument loads)
    const uint16_t* a;                  // raw rows x1 [S][lda] (the residual stream after attention); every workgroup normalises them itself
    const uint16_t* norm_w;             // post-attention RMSNorm weights [D]
    float rms_eps;
    int lda, S, G;                      // row stride, rows (<= 16), groups
    int pair0[FLAT_MAXG + 1];           // first flat pair of gate/up group i (pair0[G] = all pairs)
    const uint16_t* w_gu[FLAT_MAXG];    // WP16 gate/up weights (blocks interleaved) per group
    uint16_t* h;                        // silu(g)*u rows [.][ldh]: written by the gate/up phase, read by the down phase of this launch
    uint16_t* y;                        // down-projection outputs [.][ldy]
    uint32_t* flags;                    // one word per workgroup: its gate/up slice is published
    unsigned long long* dbg;            // diagnostics only (NULL otherwise): [workgroup][16] wall-clock stamps (100 MHz)
    int ldh, ldy, kb_gu;                // k-steps (K / 32) of the gate/up GEMMs (64: see flat_gateup)
    const uint16_t* w_dn[FLAT_MAXG];    // WP16 down weights per group
    int h_row[FLAT_MAXG];               // gate/up group i writes rows h_row[i] + r of h
    int dn_kb[FLAT_MAXG];               // k-steps of down group i
    int dn_a_row[FLAT_MAXG];            // down group i reads rows dn_a_row[i] + r of h ...
    int dn_y_row[FLAT_MAXG];            // ... and writes rows dn_y_row[i] + r of y
    int dn_nb[FLAT_MAXG];               // 16-feature blocks of down group i
    int prod_base[FLAT_MAXG];           // producers of down group i's rows: workgroups [prod_base, prod_base + prod_n)
    int prod_n[FLAT_MAXG];
    uint32_t gu[FLAT_MAXWG];            // per workgroup: first flat pair | pairs << 11 | (rider token + 1) << 16 (0: not a rider)
    uint32_t dn[FLAT_MAXWG];            // per workgroup: TWO down slices, 16 bits each (low half first): group | first block << 4 | blocks << 12
};                                      //   (blocks 0 = no slice; see FLAT_ND_*)

__device__ __forceinline__ int flat_lds_chunk_off(int QS, int h, int i, int m) {
    // 16-byte chunk i of K-quarter h, row m: 256-byte segments, slot rotated by the row index (umoe_gemm.hip lds_chunk_off)
    return h * QS + (i >> 4) * 256 + (((i & 15) + m) & 15) * 16;
}

// bounded wait of ONE lane for an epoch flag; `code` lands in the sticky error word only on this lane's OWN timeout (a word that is
// already set -- an earlier cause, e.g. an expert-parallel receive -- ends the wait and is kept)
__device__ __forceinline__ void flat_wait(uint32_t* flag, uint32_t epoch, uint32_t* err_word, uint32_t code) {
    umoe_gu32* f = reinterpret_cast<umoe_gu32*>(reinterpret_cast<uintptr_t>(flag));
    umoe_gu32* err = reinterpret_cast<umoe_gu32*>(reinterpret_cast<uintptr_t>(err_word));
    const unsigned long long t0 = wall_clock64();
    for (unsigned spins = 0;; ++spins) {
        if ((int32_t)(__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - epoch) >= 0) break;
        __builtin_amdgcn_s_sleep(1);
        if ((spins & 1023u) == 1023u) {
            if (__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) break;
            if (wall_clock64() - t0 > 200000000ull) {      // 2 s
                uint32_t zero = 0u;
                __hip_atomic_compare_exchange_strong(err, &zero, code, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
        }
    }
}

// diagnostics: thread 0 keeps up to 16 stamps in registers and stores them at exit (scalar branch on a kernel argument)
// (the instrumented build only -- make tl, scripts/flat_timeline.py; the product kernel carries no stamp)
#ifdef UMOE_TIMELINE
struct flat_stamps { unsigned long long t[16]; };
#define FSTAMP(k) do { if (A.dbg) st.t[k] = wall_clock64(); } while (0)
#else
struct flat_stamps {};
#define FSTAMP(k) do { } while (0)
#endif

typedef uint32_t flat_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t flat_u32x2 __attribute__((ext_vector_type(2)));

// ---- FP8 expert weights (moe_flat_fp8_kernel): WP8 blocks (include/umoe.h) -- one 16-byte lane load carries TWO k-steps of OCP e4m3 --
// and one power-of-two exponent per output row.  The conversion v_cvt_scalef32_pk_bf16_fp8 with the scale 2^e yields exactly the bf16 bits
// of q * 2^e, so the MFMAs below see the operands of the bf16 kernel run on the dequantized weights: same tiles, K split, MFMA order.
struct flat_f8 {                        // a kernel argument of its own (flat_args stays as it is)
    const int8_t* e_gu[FLAT_MAXG];      // exponents of the gate/up blocks, 16 per block, blocks interleaved like the weights
    const int8_t* e_dn[FLAT_MAXG];      // exponents of the down blocks
};
typedef __bf16 flat_bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float flat_f8_scale(int e) { return __uint_as_float((uint32_t)(e + 127) << 23); }     // 2^e, |e| <= 126
// 8 e4m3 values (one k-step of a lane) -> one MFMA operand
__device__ __forceinline__ bf16x8_t flat_f8_frag(uint32_t lo, uint32_t hi, float sc) {
    const flat_bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, sc, false), b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, sc, true);
    const flat_bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, sc, false), d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, sc, true);
    return bf16x8_t{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

// ---- WP12 expert weights (moe_flat_w12_kernel): bf16 weights in 12 bits, lossless (include/umoe.h "WP12").  Per lane and k-step 8 raw
// low bytes + 8 four-bit codes of the high bytes (sign + offset into the block's window of 8 high-byte exponents); values outside the
// window sit in the block's sorted exception list and are patched into the decoded operand.  The operand is the WP16 one, bit for bit,
// so the MFMAs below are the bf16 kernel's: same tiles, K split, MFMA order.
#define FLAT_W12_META 40                // u32 per block: exceptions [0, 32] (sentinel-terminated), window base in the last word
struct flat_w12 {                       // a kernel argument of its own (flat_args stays as it is)
    const uint32_t* m_gu[FLAT_MAXG];    // block records of the gate/up blocks (blocks interleaved like the weights)
    const uint32_t* m_dn[FLAT_MAXG];    // ... of the down blocks
};
// one k-step of a lane (low bytes l0 = values 0..3, l1 = 4..7; code word c: byte b = value (0,1,4,5)[b] | value (2,3,6,7)[b] << 4)
// -> the MFMA operand.  wb4 = the window base in every byte (base + offset <= 127: no carry between bytes).
__device__ __forceinline__ flat_u32x4 flat_w12_frag(uint32_t l0, uint32_t l1, uint32_t c, uint32_t wb4) {
    const uint32_t hl = (((c & 0x07070707u) + wb4) | ((c & 0x08080808u) << 4));
    const uint32_t hh = ((((c >> 4) & 0x07070707u) + wb4) | (c & 0x80808080u));
    // v_perm_b32: selector bytes 0..3 pick from the second operand, 4..7 from the first
    return flat_u32x4{__builtin_amdgcn_perm(hl, l0, 0x05010400u), __builtin_amdgcn_perm(hh, l0, 0x05030402u),
                      __builtin_amdgcn_perm(hl, l1, 0x07010600u), __builtin_amdgcn_perm(hh, l1, 0x07030602u)};
}
// A tile's exception cursor: `m` holds the block record (lane l = word min(l, 39)), st = cursor << 8 | k-step of the entry under it
// (127: the sentinel).  Entry: k-step << 25 | lane << 19 | element << 16 | bf16 bits.
__device__ __forceinline__ uint32_t flat_w12_cursor(uint32_t m, int i0, int lane) {
    const uint32_t cur = (uint32_t)__builtin_popcountll(__ballot((int)(m >> 25) < i0 && lane <= 32));      // (sorted by k-step)
    return cur << 8 | (uint32_t)__builtin_amdgcn_readlane(m, cur) >> 25;
}
__device__ __forceinline__ uint32_t flat_w12_base4(uint32_t m) { return ((uint32_t)__builtin_amdgcn_readlane(m, FLAT_W12_META - 1) & 0xffu) * 0x01010101u; }
// the rare path (scalar branch taken when the entry under the cursor is of this k-step): every entry of k-step ii into the operand
__device__ __forceinline__ void flat_w12_patch(flat_u32x4& op, uint32_t m, uint32_t& st, uint32_t ii, int lane) {
    uint32_t cur = st >> 8, nx;
    do {
        const uint32_t en = (uint32_t)__builtin_amdgcn_readlane(m, cur);
        const uint32_t sh = ((en >> 16) & 1u) * 16u, d = (en >> 17) & 3u;
        const bool mine = (uint32_t)lane == ((en >> 19) & 63u);
#pragma unroll
        for (int q = 0; q < 4; ++q) op[q] = (mine && d == (uint32_t)q) ? ((op[q] & ~(0xffffu << sh)) | ((en & 0xffffu) << sh)) : op[q];
        ++cur;
        nx = (uint32_t)__builtin_amdgcn_readlane(m, cur) >> 25;
    } while (nx == ii);
    st = cur << 8 | nx;
}

// ---- gate/up SwiGLU slice: NP pairs of the flat list starting at fp0 (arithmetic of wstream_body<14, 1, PLAIN, SWIGLU, 8> per tile) ----
// The workgroup normalises the 16 rows ITSELF while it stages them (post-attention RMSNorm, model.py:240): the raw rows exist when the
// launch starts, so nothing is waited for -- rows requested first, the weight stream right behind them, and the ~2 us of row arithmetic
// hide under the first chunk's flight.  The sum of squares follows the router body's tree (umoe_router_dev.h router4_body: lane l of wave
// h sums the 8 squares of chunk 64 h + l, xor-butterfly 32 .. 1, the four wave sums added in order), so the rows are bit-identical to
// the rows the router launches write.  K = 2048 only (one staging round, thread (row m, sub) holds chunks sub and sub + 32 of a quarter).
__device__ __forceinline__ uint32_t flat_epoch(const umoe_rider_pub& pub) {
    // the step word lives in device memory: read it where it is first needed (a load the compiler may not hoist in front of the
    // kernel's first weight request -- it was one more dependent scalar round trip there)
    asm volatile("" ::: "memory");
    return __builtin_nontemporal_load(pub.step) * (uint32_t)pub.layers + (uint32_t)pub.layer + 1u;
}

// F8: WP8 weights (w_gu holds WP8 addresses, F their exponents): one 16-byte chunk = two k-steps; every chunk index below counts chunks.
// W12: WP12 weights (w_gu holds WP12 addresses, Wm the block records): a register stage is a 2-step chunk (16 low bytes + 8 code bytes
// per lane), ONE stage per tile that is requested again as soon as its two MFMAs are issued -- two whole stages would be 168 registers.
template <int NP, bool PUBLISH = true, bool F8 = false, bool W12 = false>
__device__ __forceinline__ void flat_gateup(const flat_args& A, const umoe_rider_pub& pub, const int fp0, const unsigned b, char* smem, flat_stamps& st,
                                            const int tid_in, const flat_f8* F = nullptr, const flat_w12* Wm = nullptr) {      // tid_in = threadIdx.x (a caller that loops over slices passes an opaque copy: see umoe_moe_ep.hip)
    static_assert(!(F8 && W12), "one weight format");
    constexpr int NT = 2 * NP, WV = 8, KB = 64;
    const int tid = tid_in, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // scalar: every guard around an MFMA is a scalar branch
    constexpr int QS = (KB * 16 + 255) & ~255, RS = QS * 4;
    const int i0 = __builtin_amdgcn_readfirstlane((KB * wave) / WV), i1 = __builtin_amdgcn_readfirstlane((KB * (wave + 1)) / WV);
    constexpr int CS = (F8 || W12) ? 2 : 1;          // k-steps per 16-byte chunk (a wave's 8 steps are whole chunks either way)
    const int c0 = i0 / CS, c1 = i1 / CS;
    // the slice straddles at most two groups (a group has far more than 7 pairs).  Every table read is a kernel-argument read with a
    // compile-time offset + a scalar select: ONE batch of scalar loads in front of the first request, no dependent second one
    int g0 = 0;
#pragma unroll
    for (int i = 1; i < FLAT_MAXG; ++i) g0 += (fp0 >= A.pair0[i] && i < A.G) ? 1 : 0;      // (pair0 ascends: the count IS the index)
    const int p0 = A.pair0[g0], cut = A.pair0[g0 + 1];
    const uint16_t *wg0 = A.w_gu[g0], *wg1 = A.w_gu[g0 + 1 < FLAT_MAXG ? g0 + 1 : g0];
    const int g1 = min(g0 + 1, A.G - 1);      // pairs >= cut belong to group g1
    f32x4_t acc[NT];
    const flat_u32x4* wp[NT];
    [[maybe_unused]] const int8_t* ep[F8 ? NT : 1];
    [[maybe_unused]] int ev[F8 ? NT : 1];
    // (W12: wp = the block's low bytes, 16 per lane and chunk; cp = its code words, 8 per lane and chunk; mp = this lane's record word)
    [[maybe_unused]] const flat_u32x2* cp[W12 ? NT : 1];
    [[maybe_unused]] const uint32_t* mp[W12 ? NT : 1];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        const int pp = fp0 + (t >> 1);
        const bool second = pp >= cut;
        const int lp = pp - (second ? cut : p0);
        if constexpr (W12) {
            const int blk = 2 * lp + (t & 1);
            const char* base = reinterpret_cast<const char*>(second ? wg1 : wg0) + (size_t)blk * (KB * 768);
            wp[t] = reinterpret_cast<const flat_u32x4*>(base) + lane;
            cp[t] = reinterpret_cast<const flat_u32x2*>(base + KB * 512) + lane;
            mp[t] = (second ? Wm->m_gu[g0 + 1 < FLAT_MAXG ? g0 + 1 : g0] : Wm->m_gu[g0]) + blk * FLAT_W12_META + min(lane, FLAT_W12_META - 1);
        } else if constexpr (F8) {
            const int blk = 2 * lp + (t & 1);
            wp[t] = reinterpret_cast<const flat_u32x4*>(second ? wg1 : wg0) + ((size_t)blk * (KB / 2)) * 64 + lane;
            ep[t] = (second ? F->e_gu[g0 + 1 < FLAT_MAXG ? g0 + 1 : g0] : F->e_gu[g0]) + blk * 16 + (lane & 15);
        } else {
            wp[t] = reinterpret_cast<const flat_u32x4*>(second ? wg1 : wg0) + ((size_t)(2 * lp + (t & 1)) * KB) * 64 + lane;
        }
    }
    // the row scales: requested behind the first weight chunk (never a round trip in front of it), needed at its first MFMA
    auto load_scales = [&]() {
        if constexpr (F8) {
#pragma unroll
            for (int t = 0; t < NT; ++t) ev[t] = *ep[t];
        }
    };
    [[maybe_unused]] flat_u32x2 wc[W12 ? NT : 1];      // W12: the code words of the stage w0; mt: the block records
    [[maybe_unused]] uint32_t mt[W12 ? NT : 1];
    auto w12_load_tile = [&](flat_u32x4 (&dst)[NT], int t, int ic) {
        if constexpr (W12) {
            dst[t] = __builtin_nontemporal_load(wp[t] + (size_t)ic * 64);
            wc[t] = __builtin_nontemporal_load(cp[t] + (size_t)ic * 64);
        }
    };
    flat_u32x4 w0[NT], w1[NT];
    auto load_chunk = [&](flat_u32x4 (&dst)[NT], int ii) {
        const int ic = min(ii, c1 - 1);
#pragma unroll
        for (int t = 0; t < NT; ++t) dst[t] = __builtin_nontemporal_load(wp[t] + (size_t)ic * 64);
    };
    const int count = A.S;
    // ---- rows first (they exist: the previous launch wrote them), then the weight stream; normalise while the chunk flies ----
    {
        constexpr int TPR = WV * 4;      // threads per row
        const int m = tid / TPR, sub = tid % TPR;
        const bool valid = m < count;
        const uint16_t* src = A.a + (size_t)(valid ? m : 0) * A.lda;
        char* dst = smem + m * RS;
        char* nw_lds = smem + 16 * RS;
        // normalise + stage the 16 rows from the slices the threads hold (`buf`, `nw1`: the row chunks and the norm weights of this thread)
        // (a lambda called once: written out in place, it changed the scalar register allocation of moe_ep_kernel)
        auto norm_stage = [&](uint4 (&buf)[8], const uint4 nw1) {
            st16(nw_lds + (tid & (4 * KB - 1)) * 16, nw1);      // (both halves of the workgroup store the same 4 KiB)
            float q4[4];
#pragma unroll
            for (int hq = 0; hq < 4; ++hq) {
                float c2[2];
#pragma unroll
                for (int k2 = 0; k2 < 2; ++k2) {
                    float f[8];
                    unpack8(buf[hq * 2 + k2], f);
                    float cs = 0.f;
#pragma unroll
                    for (int j = 0; j < 8; ++j) cs += f[j] * f[j];
                    c2[k2] = cs;
                }
                float v = c2[0] + c2[1];
#pragma unroll
                for (int o = 16; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
                q4[hq] = v;
            }
            const float ss = ((q4[0] + q4[1]) + q4[2]) + q4[3];
            const float rs = rsqrtf(ss / (float)(KB * 32) + A.rms_eps);
            __syncthreads();
            FSTAMP(2);
            // keep the row slice packed (32 registers) between the sum of squares and the scaling
#pragma unroll
            for (int n = 0; n < 8; ++n) asm volatile("" : "+v"(buf[n].x), "+v"(buf[n].y), "+v"(buf[n].z), "+v"(buf[n].w));
#pragma unroll
            for (int n = 0; n < 8; ++n) {
                const int h = n >> 1, i = sub + TPR * (n & 1);
                float f[8], w[8];
                unpack8(buf[n], f);
                unpack8(*reinterpret_cast<const uint4*>(nw_lds + (h * KB + i) * 16), w);
#pragma unroll
                for (int j = 0; j < 8; ++j) f[j] = w[j] * rbf(f[j] * rs);
                if (valid) st16(dst + flat_lds_chunk_off(QS, h, i, m), pack8(f));
            }
        };
        uint4 buf[8];
#pragma unroll
        for (int n = 0; n < 8; ++n) buf[n] = ld16(src + ((n >> 1) * KB + sub + TPR * (n & 1)) * 8);
        // (straight-line loads only: a branch around a load makes hipcc wait for vmcnt(0), i.e. for the weight chunk behind the rows)
        const uint4 nw1 = ld16(A.norm_w + (tid & (4 * KB - 1)) * 8);
        // (measured and rejected: BOTH register stages requested here.  A CU issues about 1 KiB of vector loads per 100 cycles, so the
        //  second stage's 14 requests per wave only delayed the point where the rows are staged -- 8.6 -> 12.1 us -- and bought nothing:
        //  3.020 vs 3.015 ms/step.  The launch runs at the CU's request rate from its first request on.)
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (W12) {
            // the block records in FRONT of the stage (256 bytes a tile): behind it they would return last, and the first MFMA needs them
#pragma unroll
            for (int t = 0; t < NT; ++t) mt[t] = *mp[t];
#pragma unroll
            for (int t = 0; t < NT; ++t) w12_load_tile(w0, t, c0);
        } else {
            load_chunk(w0, c0);
            load_scales();
        }
        __builtin_amdgcn_sched_barrier(0);
        FSTAMP(1);
        norm_stage(buf, nw1);
    }
    __syncthreads();
    FSTAMP(3);
    // ---- stream: 1-step chunks, double-buffered in registers, the 8 waves split K ----
    const int h = lane >> 4, mm = lane & 15;
    const char* bbase = smem + mm * RS;
    auto compute_chunk = [&](const flat_u32x4 (&src)[NT], int ii) {
        if (ii < c1) {
            if constexpr (F8) {
                // k-steps 2 ii and 2 ii + 1: every tile's MFMA of the first step, then of the second (the bf16 kernel's order per tile)
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const uint4 bv = *reinterpret_cast<const uint4*>(bbase + flat_lds_chunk_off(QS, h, 2 * ii + k, mm));
                    const bf16x8_t bfrag = __builtin_bit_cast(bf16x8_t, bv);
#pragma unroll
                    for (int t = 0; t < NT; ++t)
                        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(flat_f8_frag(src[t][2 * k], src[t][2 * k + 1], flat_f8_scale(ev[t])), bfrag, acc[t], 0, 0, 0);
                }
            } else {
                const uint4 bv = *reinterpret_cast<const uint4*>(bbase + flat_lds_chunk_off(QS, h, ii, mm));
                const bf16x8_t bfrag = __builtin_bit_cast(bf16x8_t, bv);
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, src[t]), bfrag, acc[t], 0, 0, 0);
            }
        }
    };
    if constexpr (W12) {
        // chunk ic of every tile: decode, patch (a scalar compare per tile and k-step), the two MFMAs; REFILL: the tile's next chunk is
        // requested right behind them (straight-line: the last chunk is the same body without the requests)
        uint32_t xs[NT], wb4[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            xs[t] = flat_w12_cursor(mt[t], i0, lane);
            wb4[t] = flat_w12_base4(mt[t]);
        }
        auto w12_chunk = [&](int ic, auto refill) {
            const uint4 bv0 = *reinterpret_cast<const uint4*>(bbase + flat_lds_chunk_off(QS, h, 2 * ic, mm));
            const uint4 bv1 = *reinterpret_cast<const uint4*>(bbase + flat_lds_chunk_off(QS, h, 2 * ic + 1, mm));
            const bf16x8_t bf0 = __builtin_bit_cast(bf16x8_t, bv0), bf1 = __builtin_bit_cast(bf16x8_t, bv1);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                flat_u32x4 o0 = flat_w12_frag(w0[t][0], w0[t][1], wc[t][0], wb4[t]);
                if ((xs[t] & 0xffu) == (uint32_t)(2 * ic)) flat_w12_patch(o0, mt[t], xs[t], (uint32_t)(2 * ic), lane);
                flat_u32x4 o1 = flat_w12_frag(w0[t][2], w0[t][3], wc[t][1], wb4[t]);
                if ((xs[t] & 0xffu) == (uint32_t)(2 * ic + 1)) flat_w12_patch(o1, mt[t], xs[t], (uint32_t)(2 * ic + 1), lane);
                if constexpr (decltype(refill)::value) w12_load_tile(w0, t, ic + 1);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, o0), bf0, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, o1), bf1, acc[t], 0, 0, 0);
            }
        };
        for (int ic = c0; ic < c1 - 1; ++ic) w12_chunk(ic, std::true_type{});
        w12_chunk(c1 - 1, std::false_type{});
    } else {
        for (int i = c0; i < c1; i += 2) {
            if (i + 1 < c1) load_chunk(w1, i + 1);
            compute_chunk(w0, i);
            if (i + 2 < c1) load_chunk(w0, i + 2);
            if (i + 1 < c1) compute_chunk(w1, i + 1);
        }
    }
    // ---- fixed-order cross-wave reduction through the (now free) staging area ----
    FSTAMP(4);
    __syncthreads();
    FSTAMP(5);
    f32x4_t* red = reinterpret_cast<f32x4_t*>(smem);
#pragma unroll
    for (int t = 0; t < NT; ++t) red[(wave * NT + t) * 64 + lane] = acc[t];
    __syncthreads();
    auto reduced = [&](int t) -> f32x4_t {
        f32x4_t s = red[t * 64 + lane];
#pragma unroll
        for (int w = 1; w < WV; ++w) {
            const f32x4_t v = red[(w * NT + t) * 64 + lane];
            s[0] += v[0]; s[1] += v[1]; s[2] += v[2]; s[3] += v[3];
        }
        return s;
    };
    // ---- SwiGLU epilogue: lane (h, mm) owns features 4h..4h+3 of row mm; pairs spread over the waves; write-through stores ----
    const auto orsrc = __builtin_amdgcn_make_buffer_rsrc(A.h, 0, 0x7fffffff, 0x00020000);
    for (int q = wave; q < NP; q += WV) {
        const int pp = fp0 + q;
        const int grp = pp >= cut ? g1 : g0;
        const int col = (pp - A.pair0[grp]) * 16 + 4 * h;
        const long orow = (long)A.h_row[grp] + mm;
        const f32x4_t ga = reduced(2 * q), ua = reduced(2 * q + 1);
        uint16_t yv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float gt = rbf(ga[j]);
            const float up = rbf(ua[j]);
            const float si = rbf(gt / (1.0f + expf(-gt)));
            yv[j] = f2bf(si * up);
        }
        const flat_u32x2 v2 = {(uint32_t)yv[0] | ((uint32_t)yv[1] << 16), (uint32_t)yv[2] | ((uint32_t)yv[3] << 16)};
        if (mm < count) __builtin_amdgcn_raw_buffer_store_b64(v2, orsrc, (int)((orow * A.ldh + col) * 2), 0, 16);
    }
    // publish: every storing wave drains, the workgroup meets, one lane raises this workgroup's flag
    // (PUBLISH false: a workgroup with several slices of one phase raises its flag once, behind the last of them -- the caller does)
    if constexpr (PUBLISH) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0)
            __hip_atomic_store(reinterpret_cast<umoe_gu32*>(reinterpret_cast<uintptr_t>(A.flags + b)), flat_epoch(pub), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    FSTAMP(6);
}

// ---- down-projection slice: blocks [nb0, nb0 + ND) of group grp (arithmetic of wstream_body<6, 2, PLAIN, BF16, 8> per tile) ----
// U = 2 for an even number of k-steps (whole 2-step chunks per wave), U = 1 for an odd one: the K split of the 2-step launch does not
// depend on U then, and a 1-step stream has no clamped duplicate step at the end of a wave's slice.
// F8: WP8 weights (w_dn holds WP8 addresses, F their exponents).  U = 2: one 16-byte load per lane carries the chunk's two k-steps;
// U = 1 (an odd number of k-steps per K quarter: a wave's slice starts or ends on either half of a 16-byte chunk): one 8-byte load per
// k-step.  Either way exactly the bf16 kernel's MFMAs -- no padded step is computed.
// W12: WP12 weights (w_dn holds WP12 addresses, Wm the block records): a register stage holds U k-steps -- 8 U low bytes + 4 U code bytes
// per lane, two loads -- and the stages are double-buffered like the bf16 ones (the packer chunks by the parity of KB, as U is chosen).
template <int ND, int U, bool F8 = false, bool W12 = false>
__device__ __forceinline__ void flat_down(const flat_args& A, const umoe_rider_pub& pub, const int grp, const int nb0, char* smem, flat_stamps& st,
                                          const int sb, const int tid_in, const flat_f8* F = nullptr, const flat_w12* Wm = nullptr) {
    static_assert(!(F8 && W12), "one weight format");
    constexpr int NT = ND, WV = 8;
    const int tid = tid_in, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int KB = A.dn_kb[grp];
    const int QS = (KB * 16 + 255) & ~255, RS = QS * 4;
    int i0, i1;
    if (KB % 2 == 0) {      // whole 2-step chunks per wave when the slice divides (U == 2 here)
        const int units = KB / 2;
        i0 = 2 * ((units * wave) / WV);
        i1 = 2 * ((units * (wave + 1)) / WV);
    } else {
        i0 = (KB * wave) / WV;
        i1 = (KB * (wave + 1)) / WV;
    }
    i0 = __builtin_amdgcn_readfirstlane(i0);
    i1 = __builtin_amdgcn_readfirstlane(i1);
    f32x4_t acc[NT];
    // (F8: a register stage holds U k-steps of e4m3 -- 8 bytes per step -- in ONE load: x4 for U = 2, x2 for U = 1)
    using FW = std::conditional_t<U == 2, flat_u32x4, flat_u32x2>;
    constexpr int UL = (F8 || W12) ? 1 : U;          // loads per register stage and tile (W12: + one of the code words)
    using WT = std::conditional_t<F8 || W12, FW, flat_u32x4>;
    using CT = std::conditional_t<U == 2, flat_u32x2, uint32_t>;      // W12: the code words of a stage
    const WT* wp[NT];
    [[maybe_unused]] int ev[F8 ? NT : 1];
    [[maybe_unused]] const CT* cp[W12 ? NT : 1];
    [[maybe_unused]] uint32_t mt[W12 ? NT : 1];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        if constexpr (W12) {
            const char* base = reinterpret_cast<const char*>(A.w_dn[grp]) + (size_t)(nb0 + t) * ((size_t)KB * 768);
            wp[t] = reinterpret_cast<const WT*>(base) + lane;
            cp[t] = reinterpret_cast<const CT*>(base + (size_t)KB * 512) + lane;
            mt[t] = Wm->m_dn[grp][(nb0 + t) * FLAT_W12_META + min(lane, FLAT_W12_META - 1)];      // (in front of the first stage, like flat_gateup)
        } else if constexpr (F8) {
            const int KB2 = (KB + 1) >> 1;           // 16-byte chunks per K quarter (the last one half used when KB is odd)
            wp[t] = reinterpret_cast<const WT*>(reinterpret_cast<const flat_u32x4*>(A.w_dn[grp]) + ((size_t)(nb0 + t) * KB2) * 64 + lane);
        } else {
            wp[t] = reinterpret_cast<const flat_u32x4*>(A.w_dn[grp]) + ((size_t)(nb0 + t) * KB) * 64 + lane;
        }
    }
    WT w0[NT][UL], w1[NT][UL];
    [[maybe_unused]] CT c0[W12 ? NT : 1], c1[W12 ? NT : 1];
    auto load_chunk = [&](WT (&dst)[NT][UL], int ibase) {
        if constexpr (W12) {
            const int ii = min(ibase, i1 - U) / U;   // (the stage is chunk ii of the block: U = 2 on even KB only, i0 and i1 even)
            CT(&cd)[W12 ? NT : 1] = (&dst == &w0) ? c0 : c1;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                dst[t][0] = __builtin_nontemporal_load(wp[t] + (size_t)ii * 64);
                cd[t] = __builtin_nontemporal_load(cp[t] + (size_t)ii * 64);
            }
        } else if constexpr (F8) {
            const int ii = min(ibase, i1 - U);       // (U = 2: ibase and i1 even -- the stage is the whole chunk ii / 2)
#pragma unroll
            for (int t = 0; t < NT; ++t)
                dst[t][0] = __builtin_nontemporal_load(U == 2 ? wp[t] + (size_t)(ii >> 1) * 64 : wp[t] + (size_t)(ii >> 1) * 128 + (ii & 1));
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int ii = min(ibase + u, i1 - 1);
#pragma unroll
                for (int t = 0; t < NT; ++t) dst[t][u] = __builtin_nontemporal_load(wp[t] + (size_t)ii * 64);
            }
        }
    };
    if (i0 < i1) load_chunk(w0, i0);
    if constexpr (F8) {      // the row scales behind the first weight stage
        const int8_t* e = F->e_dn[grp] + nb0 * 16 + (lane & 15);
#pragma unroll
        for (int t = 0; t < NT; ++t) ev[t] = e[t * 16];
    }
    const int count = A.S;
    // wait for the workgroups of THIS launch that produced this group's rows: lane i of wave 0 polls producer i (bounded)
    if (tid < A.prod_n[grp]) flat_wait(A.flags + A.prod_base[grp] + tid, flat_epoch(pub), pub.err, 3u);
    __syncthreads();
    FSTAMP(sb);
    {
        constexpr int TPR = WV * 4;
        const int m = tid / TPR, sub = tid % TPR;
        const bool valid = m < count;
        const long arow = (long)A.dn_a_row[grp] + (valid ? m : 0);
        char* dst = smem + m * RS;
        const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(A.h, 0, 0x7fffffff, 0x00020000);
        for (int ib0 = 0; ib0 < KB; ib0 += 4 * TPR) {
            uint4 buf[16];
#pragma unroll
            for (int n = 0; n < 16; ++n) {
                const int h = n >> 2, i = min(ib0 + sub + TPR * (n & 3), KB - 1);
                const flat_u32x4 t4 = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)((arow * A.ldh + (h * KB + i) * 8) * 2), 0, 16);
                buf[n] = make_uint4(t4[0], t4[1], t4[2], t4[3]);
            }
            if (ib0 == 0) {     // the second register stage right behind the rows (returns: first stage, rows, second stage)
                __builtin_amdgcn_sched_barrier(0);
                if (i0 + U < i1) load_chunk(w1, i0 + U);
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int n = 0; n < 16; ++n) {
                const int h = n >> 2, i = ib0 + sub + TPR * (n & 3);
                if (valid && i < KB) st16(dst + flat_lds_chunk_off(QS, h, i, m), buf[n]);
            }
        }
    }
    __syncthreads();
    FSTAMP(sb + 1);
    const int h = lane >> 4, mm = lane & 15;
    const char* bbase = smem + mm * RS;
    [[maybe_unused]] uint32_t xs[W12 ? NT : 1], wb4[W12 ? NT : 1];
    if constexpr (W12) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            xs[t] = flat_w12_cursor(mt[t], i0, lane);
            wb4[t] = flat_w12_base4(mt[t]);
        }
    }
    auto compute_chunk = [&](const WT (&src)[NT][UL], int ibase) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int ii = ibase + u;
            if (ii < i1) {
                const uint4 bv = *reinterpret_cast<const uint4*>(bbase + flat_lds_chunk_off(QS, h, ii, mm));
                const bf16x8_t bfrag = __builtin_bit_cast(bf16x8_t, bv);
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    if constexpr (W12) {
                        const CT(&cs)[NT] = (&src == &w0) ? c0 : c1;
                        uint32_t cw;
                        if constexpr (U == 2) cw = cs[t][u]; else cw = cs[t];
                        flat_u32x4 o = flat_w12_frag(src[t][0][2 * u], src[t][0][2 * u + 1], cw, wb4[t]);
                        if ((xs[t] & 0xffu) == (uint32_t)ii) flat_w12_patch(o, mt[t], xs[t], (uint32_t)ii, lane);
                        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, o), bfrag, acc[t], 0, 0, 0);
                    } else if constexpr (F8)
                        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(flat_f8_frag(src[t][0][2 * u], src[t][0][2 * u + 1], flat_f8_scale(ev[t])), bfrag, acc[t], 0, 0, 0);
                    else
                        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, src[t][u]), bfrag, acc[t], 0, 0, 0);
                }
            }
        }
    };
    for (int i = i0; i < i1; i += 2 * U) {
        if (i + U < i1 && i != i0) load_chunk(w1, i + U);
        compute_chunk(w0, i);
        if (i + 2 * U < i1) load_chunk(w0, i + 2 * U);
        if (i + U < i1) compute_chunk(w1, i + U);
    }
    FSTAMP(sb + 2);
    __syncthreads();
    FSTAMP(sb + 3);
    f32x4_t* red = reinterpret_cast<f32x4_t*>(smem);
#pragma unroll
    for (int t = 0; t < NT; ++t) red[(wave * NT + t) * 64 + lane] = acc[t];
    __syncthreads();
    if (mm >= count) return;
    // tile t is finished by wave t % 8
    for (int t = wave; t < NT; t += WV) {
        f32x4_t s = red[t * 64 + lane];
#pragma unroll
        for (int w = 1; w < WV; ++w) {
            const f32x4_t v = red[(w * NT + t) * 64 + lane];
            s[0] += v[0]; s[1] += v[1]; s[2] += v[2]; s[3] += v[3];
        }
        const int n = (nb0 + t) * 16 + 4 * h;
        uint16_t yv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) yv[j] = f2bf(rbf(s[j] + 0.f));      // (+ 0.f: the bias slot of the generic epilogue; -0 -> +0 like there)
        uint16_t* o = A.y + ((long)A.dn_y_row[grp] + mm) * A.ldy + n;
        *reinterpret_cast<uint2*>(o) = make_uint2((uint32_t)yv[0] | ((uint32_t)yv[1] << 16), (uint32_t)yv[2] | ((uint32_t)yv[3] << 16));
    }
}
