// The WP12 form of the wide decode GEMM (umoe_gemm_wide.hip): the gate/up and down launches of a decode step of 17 to 64 rows on the
// lossless 12-bit copies of the bf16 expert weights (include/umoe.h "WP12", unimoe_audio_amd/w12.py).  A file of its own: umoe_gemm_wide.hip
// and every device symbol in it stay byte for byte what they were.
#include "umoe_flat_dev.h"      // (umoe_common.h; flat_w12_frag / flat_w12_base4 / flat_w12_cursor / flat_w12_patch)
#include <string.h>

#define UMOE_WIDE_MAXG 12       // (as in umoe_gemm_wide.hip)

// wstream_wide_w12: prologue, K split, reduction and the two epilogues are wstream_wide's, restated as for the fp8 form; only the
// weight stream is new.  A register stage holds CS k-steps of one block: 8 CS low bytes + 4 CS code bytes per lane (CS = 2 for an even
// number of k-steps, 1 for an odd one: the packer chunks by the parity of KB).  The operand is rebuilt ONCE per (block, k-step) and feeds
// the MFMAs of all row tiles; it is the WP16 operand bit for bit, so every output is the bf16 form's.
struct wide_w12_args {                      // the WP12 form's own argument block (wide_args stays as it is)
    const uint8_t* w[UMOE_WIDE_MAXG];       // WP12 blocks of group g (gate/up blocks interleaved for SwiGLU), KB * 768 bytes each
    const uint32_t* meta[UMOE_WIDE_MAXG];   // block records, FLAT_W12_META words per block
    const uint16_t* b[UMOE_WIDE_MAXG];      // operand-order tiles, as wide_args
    void* out[UMOE_WIDE_MAXG];
    int n_blocks[UMOE_WIDE_MAXG], k[UMOE_WIDE_MAXG];
    int num_groups, rows, tiles, ldo, n_valid;
};

// RW: k-steps the weight ring holds (RW / 2 stages of 16 + 8 bytes, or RW stages of 8 + 4 bytes for an odd number of k-steps)
template <int NT, int MT, int U, int WV, int EPI, int RW, int RB, bool WREFILL>
__global__ __launch_bounds__(WV * 64, 1) void wstream_wide_w12(const wide_w12_args p) {
    static_assert(EPI == UMOE_EPI_SWIGLU || EPI == UMOE_EPI_BF16, "the WP12 form runs the gate/up and the down launch");
    static_assert(RW % 2 == 0, "whole 2-step stages");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
    const int g = blockIdx.z, nb0 = blockIdx.x * NT;
    const int n_blocks = p.n_blocks[g];
    if (nb0 >= n_blocks) return;
    const int K = p.k[g], KB = K >> 5;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
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
    const char* wp[NT];         // the block: KB * 512 low bytes, then KB * 256 code bytes
    uint32_t mt[NT];            // the block records: lane l holds word min(l, 39)
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int nb = min(nb0 + t, n_blocks - 1);   // tail blocks re-read the last one (weights and record); never stored
        wp[t] = reinterpret_cast<const char*>(p.w[g]) + (size_t)nb * ((size_t)KB * 768);
        mt[t] = p.meta[g][(size_t)nb * FLAT_W12_META + min(lane, FLAT_W12_META - 1)];      // (in front of the first stage: the first MFMA needs it)
    }
    const u32x4_t* bp[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int mm = min(m, p.tiles - 1);
        bp[m] = reinterpret_cast<const u32x4_t*>(p.b[g]) + ((size_t)mm * KB) * 64 + lane;
    }
    f32x4_t acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[m][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    // the rings of wstream_wide with WP12 stages in the weight ring: 3 dwords per block and k-step.  The fragment ring, the refill order
    // and the clamps are the same
    u32x4_t br[RB][MT];
    auto load_b = [&](u32x4_t (&d)[MT], int ii) {
#pragma unroll
        for (int m = 0; m < MT; ++m) d[m] = bp[m][(size_t)ii * 64];
    };
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
                d[t] = __builtin_nontemporal_load(reinterpret_cast<const WT*>(wp[t]) + slot);
                c[t] = __builtin_nontemporal_load(reinterpret_cast<const CT*>(wp[t] + code0) + slot);
            }
        };
        const int il = max(i1 - 1, 0), ilw = max(i1 - CS, 0);
#pragma unroll
        for (int r = 0; r < RB; ++r) load_b(br[r], min(i0 + r, il));
#pragma unroll
        for (int r = 0; r < RW / CS; ++r) load_w(wr[r], wc[r], min(i0 + CS * r, ilw));
        // the exception cursor (entries of k-steps below the wave's i0 skipped) and the window base of every block: scalar registers
        uint32_t xs[NT], wb4[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            xs[t] = flat_w12_cursor(mt[t], i0, lane);
            wb4[t] = flat_w12_base4(mt[t]);
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
                        if ((xs[t] & 0xffu) == (uint32_t)ii) flat_w12_patch(o, mt[t], xs[t], (uint32_t)ii, lane);
                        const bf16x8_t wf = __builtin_bit_cast(bf16x8_t, o);
#pragma unroll
                        for (int m = 0; m < MT; ++m)
                            acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, __builtin_bit_cast(bf16x8_t, br[r % RB][m]), acc[m][t], 0, 0, 0);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
                load_b(br[r % RB], min(ii + RB, il));
                if constexpr (WREFILL)
                    if (r % CS == CS - 1) load_w(wr[r / CS], wc[r / CS], min(ii - (CS - 1) + RW, ilw));
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    // (U == 1: the host admits only K whose wave slices are whole chunks)
    if (U == 2 && (KB & 1)) stream(std::integral_constant<int, 1>{});
    else stream(std::integral_constant<int, 2>{});
    // ---- fixed-order cross-wave reduction (wave 0 first) ----
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
    const int h = lane >> 4, mm = lane & 15;
    if constexpr (EPI == UMOE_EPI_SWIGLU) {
        const int I = n_blocks * 8, Q = I >> 2;
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
            const int f = (nb0 / 2 + pq) * 16 + 4 * h;
            const int qq = f / Q, r = f % Q;
            uint16_t* o = reinterpret_cast<uint16_t*>(p.out[g]) + (size_t)m * 16 * I + ((size_t)(r >> 3) * 64 + qq * 16 + mm) * 8 + (r & 7);
            *reinterpret_cast<uint2*>(o) = make_uint2((uint32_t)y[0] | ((uint32_t)y[1] << 16), (uint32_t)y[2] | ((uint32_t)y[3] << 16));
        }
    } else {
        for (int q = wave; q < MT * NT; q += WV) {
            const int m = q / NT, t = q % NT;
            const int row = m * 16 + mm;
            if (m >= p.tiles || nb0 + t >= n_blocks || row >= p.rows) continue;      // pad rows are never stored
            const f32x4_t a4 = reduced(m, t);
            const int n = (nb0 + t) * 16 + 4 * h;
            if (n >= p.n_valid) continue;
            uint16_t* o = reinterpret_cast<uint16_t*>(p.out[g]) + (size_t)row * p.ldo + n;
            uint16_t y[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) y[j] = f2bf(rbf(a4[j] + 0.f));      // (+ 0.f: the bias slot of wstream_wide; -0 -> +0 like there)
            if (n + 3 < p.n_valid) {
                *reinterpret_cast<uint2*>(o) = make_uint2((uint32_t)y[0] | ((uint32_t)y[1] << 16), (uint32_t)y[2] | ((uint32_t)y[3] << 16));
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (n + j < p.n_valid) o[j] = y[j];
            }
        }
    }
}

template <int NT, int MT, int U, int WV, int EPI, int RW, int RB, bool WREFILL>
static int launch_wide_w12_v(const wide_w12_args& a, int max_nb, hipStream_t s) {
    const size_t lds = (size_t)WV * MT * NT * 64 * 16;
    void (*kernel)(const wide_w12_args) = &wstream_wide_w12<NT, MT, U, WV, EPI, RW, RB, WREFILL>;
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

template <int NT, int MT, int U, int WV, int EPI, int RW, int RB>
static int launch_wide_w12(const wide_w12_args& a, hipStream_t s) {
    // k-steps of the longest wave slice over the groups: no weight refill when the ring holds them all
    int longest = 0, max_nb = 0;
    for (int g = 0; g < a.num_groups; ++g) {
        const int KB = a.k[g] >> 5;
        const int l = (KB % U == 0) ? U * ceil_div(KB / U, WV) : ceil_div(KB, WV);
        longest = l > longest ? l : longest;
        max_nb = a.n_blocks[g] > max_nb ? a.n_blocks[g] : max_nb;
    }
    if (longest <= RW) return launch_wide_w12_v<NT, MT, U, WV, EPI, RW, RB, false>(a, max_nb, s);
    return launch_wide_w12_v<NT, MT, U, WV, EPI, RW, RB, true>(a, max_nb, s);
}

// The gate/up and down launches of the wide step on WP12 weights: (SwiGLU, 8, 1) and (bf16, 8, 2), tiles and K split as above.  Blocks per
// workgroup and ring depths: a k-step is 3 dwords per block, so gate/up takes 4 blocks per workgroup at every tile count and a
// ring of 8 k-steps (a wave's whole K slice at K 2048: never refilled there; measured against 8 blocks with a refilled ring of 4 k-steps
// at two tiles: 44.3 vs 45.6 us per launch); down keeps the bf16 form's blocks with a ring of 12 k-steps (a wave's whole slice of 86 k-steps).
extern "C" int umoe_gemm_wide_w12(const uint8_t* const* host_w12, const uint32_t* const* host_meta, const int* host_n_blocks, const int* host_k,
                                  int num_groups, int rows, const uint16_t* const* host_b, void* const* host_out, int ldo, int n_valid,
                                  int epilogue, int waves, int u, umoe_stream_t stream) {
    UMOE_REQUIRE(host_w12 && host_meta && host_n_blocks && host_k && host_b && host_out, "umoe_gemm_wide_w12: null argument");
    UMOE_REQUIRE(num_groups >= 1 && num_groups <= UMOE_WIDE_MAXG, "umoe_gemm_wide_w12: 1..%d groups (got %d)", UMOE_WIDE_MAXG, num_groups);
    UMOE_REQUIRE(rows > 16 && rows <= 64, "umoe_gemm_wide_w12: 17..64 rows (got %d): 16 rows and fewer are the WP12 flat expert launch's", rows);
    const bool swiglu = epilogue == UMOE_EPI_SWIGLU && waves == 8 && u == 1, down = epilogue == UMOE_EPI_BF16 && waves == 8 && u == 2;
    UMOE_REQUIRE(swiglu || down, "umoe_gemm_wide_w12: (epilogue, waves, u) must be the gate/up or the down launch's: (SwiGLU, 8, 1), (bf16, 8, 2) (got %d, %d, %d)",
                 epilogue, waves, u);
    wide_w12_args a;
    memset(&a, 0, sizeof(a));
    a.num_groups = num_groups; a.rows = rows; a.tiles = ceil_div(rows, 16); a.ldo = ldo; a.n_valid = n_valid;
    for (int g = 0; g < num_groups; ++g) {
        a.w[g] = host_w12[g]; a.meta[g] = host_meta[g]; a.b[g] = host_b[g]; a.out[g] = host_out[g];
        a.n_blocks[g] = host_n_blocks[g]; a.k[g] = host_k[g];
        UMOE_REQUIRE(a.w[g] && a.meta[g], "umoe_gemm_wide_w12: group %d: host_w12 / host_meta hold a null pointer (weights %p, records %p)", g,
                     (const void*)a.w[g], (const void*)a.meta[g]);
        UMOE_REQUIRE(a.b[g] && a.out[g], "umoe_gemm_wide_w12: group %d lacks input tiles (host_b) or an output (host_out)", g);
        UMOE_REQUIRE(((uintptr_t)a.w[g] & 15) == 0, "umoe_gemm_wide_w12: group %d: host_w12 must be 16-byte aligned (16-byte vector loads)", g);
        UMOE_REQUIRE(((uintptr_t)a.meta[g] & 3) == 0, "umoe_gemm_wide_w12: group %d: host_meta must be 4-byte aligned", g);
        UMOE_REQUIRE((((uintptr_t)a.b[g] | (uintptr_t)a.out[g]) & 15) == 0,
                     "umoe_gemm_wide_w12: group %d: input tiles (host_b) and output (host_out) must be 16-byte aligned (16-byte vector accesses)", g);
        UMOE_REQUIRE(a.k[g] > 0 && a.k[g] % 32 == 0 && a.n_blocks[g] > 0, "umoe_gemm_wide_w12: group %d: host_k %% 32 == 0, host_n_blocks > 0 (K=%d n_blocks=%d)", g,
                     a.k[g], a.n_blocks[g]);
        UMOE_REQUIRE(a.k[g] / 32 < 127, "umoe_gemm_wide_w12: group %d: host_k / 32 < 127 (K=%d): a block record counts k-steps in 7 bits", g, a.k[g]);
        UMOE_REQUIRE(!swiglu || a.n_blocks[g] % 4 == 0, "umoe_gemm_wide_w12: SwiGLU needs gate/up block pairs and I %% 32 == 0 (group %d: host_n_blocks %d)", g,
                     a.n_blocks[g]);
        // u = 1 splits K in single steps: only when every wave boundary K / 32 * w / 8 is even is a slice whole 2-step chunks (u = 2 serves
        // every K: whole chunks for an even number of k-steps, 1-step chunks for an odd one)
        UMOE_REQUIRE(!swiglu || a.k[g] % 512 == 0, "umoe_gemm_wide_w12: the gate/up launch needs host_k %% 512 == 0 (group %d: K=%d): every wave slice whole chunks", g,
                     a.k[g]);
        UMOE_REQUIRE(swiglu || (ldo % 4 == 0 && n_valid > 0 && n_valid <= ldo),
                     "umoe_gemm_wide_w12: row-major outputs need ldo %% 4 == 0 and 0 < n_valid <= ldo (ldo=%d n_valid=%d)", ldo, n_valid);
    }
    hipStream_t s = (hipStream_t)stream;
    const bool two = a.tiles == 2;
    if (swiglu) return two ? launch_wide_w12<4, 2, 1, 8, UMOE_EPI_SWIGLU, 8, 2>(a, s) : launch_wide_w12<4, 4, 1, 8, UMOE_EPI_SWIGLU, 8, 2>(a, s);
    return two ? launch_wide_w12<2, 2, 2, 8, UMOE_EPI_BF16, 12, 4>(a, s) : launch_wide_w12<1, 4, 2, 8, UMOE_EPI_BF16, 12, 4>(a, s);
}
