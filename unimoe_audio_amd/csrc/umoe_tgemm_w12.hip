// The tiled MFMA GEMM (umoe_tgemm.hip, tgemm_kernel) with a WP12 weight source: prefill on the lossless 12-bit expert weights.
//
//   Y[rows(g), N] = epilogue( A[rows(g), K] * W_g^T ),  W_g = bf16 weights held as WP12 blocks + block records (include/umoe.h "WP12")
//
// The twin of tgemm_wp8_kernel (umoe_tgemm_wp8.hip): the register-staging form of tgemm_kernel with another weight source.  Where the
// bf16 kernel loads a 16-byte chunk (8 bf16 of one weight row), this one loads the granule's 8 raw low bytes and its one code word from
// the WP12 block, rebuilds the 16 bytes with flat_w12_frag (umoe_flat_dev.h: 12 VALU, exact) and stores them at the same LDS offset.
// Everything behind the store is shared code or the same code -- the LDS image (tg_off), the ds_read_b128 operand reads, the MFMA
// order, the K loop, tg_epilogue -- so the output is BIT-IDENTICAL to tgemm_kernel run on the row-major weights.
//
// Granule addressing (K % 32 == 0, KB = K / 32, Q = K / 4; follows w12.pack): column k of weight row n lies in quarter h = k / Q at
// o = k - h Q, k-step i = o / 8, lane 16 h + (n & 15) of block nb = n / 16, which starts at byte nb KB 768.  With CS = 2 for even KB,
// else 1 (k-steps per chunk): u = ((i / CS) 64 + lane) CS + i % CS; the low bytes are at u 8, the code word at KB 512 + u 4.
// SwiGLU: gate row n sits in block 2 (n / 16), up row n in block 2 (n / 16) + 1 of the interleaved pair.  The window base is word 39 of
// the block's 40-word record, read once per tile row, before the K loop.  Only n < N and k < K are ever addressed.
//
// Exceptions (at most 32 per block, k-step << 25 | lane << 19 | element << 16 | bits): a K tile walks columns in ascending k, which is
// not the record's k-step order (the quarter sits in the lane field), so the flat kernels' cursor does not carry over.  Here thread
// (b = tid / 32, x = tid % 32) keeps entry x of the tile row's block b in a register, with the K tile it falls in and its byte offset in
// the LDS image; a bit mask of the K tiles that hold an entry is built once in LDS and kept in SGPRs.  On a flagged K tile -- a branch
// that is uniform for the workgroup -- a barrier separates the granule stores from the 2-byte patches, and the barrier that publishes
// the buffer follows as in every tile.  An unflagged tile runs the WP8 twin's sequence.  No hand-off other than __syncthreads.
//
// Weight traffic: the 256 threads fetch a 128-row x 64-column tile as 8-byte + 4-byte loads, 0.75 of the bytes of the bf16 tile.
#include <string.h>

#include "umoe_tgemm_dev.h"
#include "umoe_flat_dev.h"      // flat_w12_frag, FLAT_W12_META

struct tg_w12 {                         // a kernel argument of its own (umoe_tgroup_t stays as it is)
    const uint8_t* w[TG_MAXG];          // WP12 blocks of group g (SwiGLU: the interleaved gate/up pair)
    const uint32_t* m[TG_MAXG];         // their block records, FLAT_W12_META words per block
};

// MI / BKC as tgemm_kernel: (4, 8) 128-token tiles, K steps of 64; (8, 4) 256-token tiles, K steps of 32.  Two LDS buffers.
template <int EPI, int MI, int BKC>
__global__ __launch_bounds__(256, 2) void tgemm_w12_kernel(const umoe_tgemm_args p, const tg_pack gp, const tg_w12 f) {
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [2 buffers][A tile | W tile]
    __shared__ uint32_t flg[4];         // bit t: K tile t holds an exception of this tile row (K / 32 < 127: at most 126 K tiles)
    constexpr int TM = 32 * MI;
    constexpr int RPP = 256 / BKC;
    constexpr int APS = TM / RPP, WPS = 128 / RPP;
    constexpr int ABYTES = TM * BKC * 16, WBYTES = 128 * BKC * 16, BUF = ABYTES + WBYTES;
    constexpr int KS = BKC / 4;
    constexpr int BK = BKC * 8;
    const umoe_tgroup_t g = gp.g[blockIdx.z];
    const int count = g.count ? *g.count : g.static_count;
    const int roff = g.row_off ? *g.row_off : 0;
    const int row0 = blockIdx.y * TM;
    if (row0 >= count) return;
    constexpr bool SW = EPI == UMOE_EPI_SWIGLU;
    constexpr int NTILE = SW ? 64 : 128;
    const int n0 = blockIdx.x * NTILE;
    if (n0 >= g.n) return;
    const int K = g.k;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const uint8_t* const wbase = f.w[blockIdx.z];
    const uint32_t* const mbase = f.m[blockIdx.z];

    // thread (lr = tid / BKC, ch = tid % BKC) owns granule ch of tile rows lr + RPP * pass, of both operands
    const int lr = tid / BKC, ch = tid % BKC;
    const uint16_t* ap[APS];
    bool aok[APS];
#pragma unroll
    for (int ps = 0; ps < APS; ++ps) {
        const int r = row0 + lr + RPP * ps;
        aok[ps] = r < count;
        long arow = 0;
        if (aok[ps]) arow = g.rows ? (long)g.rows[roff + r] : (long)(g.a_row_base + roff + r);
        ap[ps] = p.a + arow * (long)p.lda + g.a_col_off + ch * 8;
    }
    // weight rows: byte offset of the row's lane slot inside its block, and the block's window base -- read once, before the K loop
    const int Q = K >> 2, KB = K >> 5;
    const int sh = (KB & 1) ? 0 : 1;    // log2 of the k-steps per chunk
    uint32_t wo[WPS], wc[WPS], wb4[WPS];      // byte offsets of the row's low bytes and code words at u = 0; the window base in every byte
    bool wok[WPS];
#pragma unroll
    for (int ps = 0; ps < WPS; ++ps) {
        const int tr = lr + RPP * ps;   // tile row 0..127
        const int n = n0 + (SW ? (tr & 63) : tr);
        wok[ps] = n < g.n;
        const int nn = wok[ps] ? n : 0;
        const int blk = SW ? 2 * (nn >> 4) + (tr >= 64 ? 1 : 0) : (nn >> 4);
        const uint32_t boff = (uint32_t)blk * (uint32_t)KB * 768u, rs = (uint32_t)((nn & 15) << sh);
        wo[ps] = boff + rs * 8u;
        wc[ps] = boff + (uint32_t)KB * 512u + rs * 4u;
        wb4[ps] = (mbase[blk * FLAT_W12_META + FLAT_W12_META - 1] & 0xffu) * 0x01010101u;
    }
    // this thread's exception entry: entry (tid % 32) of block (tid / 32) of the tile row (a record holds at most 32 and a sentinel)
    int ekt = -1, eoff = 0;             // the K tile it falls in (-1: none) and its byte offset in the W image
    uint32_t ebits = 0;
    {
        const int b = tid >> 5, x = tid & 31;
        const int nblk = n0 + (SW ? (b & 3) : b) * 16;          // first weight row (feature) of the block
        if (nblk < g.n) {
            const int blk = SW ? 2 * (nblk >> 4) + (b >> 2) : (nblk >> 4);
            const uint32_t en = mbase[blk * FLAT_W12_META + x];
            const int ks = (int)(en >> 25), el = (int)((en >> 19) & 63u), ej = (int)((en >> 16) & 7u);
            const int n = nblk + (el & 15), col = (el >> 4) * Q + ks * 8 + ej;
            if (ks != 127 && n < g.n && ks * 8 < Q) {           // (the sentinel reads as k-step 127; rows behind N are never patched)
                const int trow = (SW ? (b >> 2) * 64 + (b & 3) * 16 : b * 16) + (el & 15);
                ekt = col / BK;
                eoff = tg_off<BKC>(trow, (col % BK) >> 3) + (col & 7) * 2;
                ebits = en & 0xffffu;
            }
        }
    }
    uint4 ra[APS];
    uint2 rl[WPS];                      // the granule as loaded: 8 low bytes and
    uint32_t rc[WPS];                   // its code word (rebuilt on the way into LDS)
    bool rk = false;                    // the loaded K tile's granule lies inside K
    auto gload = [&](int k0) {
        const int k = k0 + ch * 8;
        const bool kok = k < K;         // K % 8 == 0: a granule is entirely inside or outside
        const int h = (k >= Q ? 1 : 0) + (k >= 2 * Q ? 1 : 0) + (k >= 3 * Q ? 1 : 0);
        const int i = (k - h * Q) >> 3;
        const uint32_t u = (uint32_t)((((i >> sh) << 6) + 16 * h) << sh) + (uint32_t)(i & sh);      // (the row's term is in wo / wc)
        rk = kok;
#pragma unroll
        for (int ps = 0; ps < APS; ++ps) {
            ra[ps] = make_uint4(0, 0, 0, 0);
            if (kok && aok[ps]) ra[ps] = ld16(ap[ps] + k0);
        }
#pragma unroll
        for (int ps = 0; ps < WPS; ++ps) {
            rl[ps] = make_uint2(0, 0);
            rc[ps] = 0;
            if (kok && wok[ps]) {
                rl[ps] = *reinterpret_cast<const uint2*>(wbase + wo[ps] + u * 8u);
                rc[ps] = *reinterpret_cast<const uint32_t*>(wbase + wc[ps] + u * 4u);
            }
        }
    };
    auto lstore = [&](int buf) {
        char* A = smem + buf * BUF;
        char* W = A + ABYTES;
#pragma unroll
        for (int ps = 0; ps < APS; ++ps) st16(A + tg_off<BKC>(lr + RPP * ps, ch), ra[ps]);
#pragma unroll
        for (int ps = 0; ps < WPS; ++ps) {
            const flat_u32x4 v = flat_w12_frag(rl[ps].x, rl[ps].y, rc[ps], wb4[ps]);
            const bool ok = rk && wok[ps];      // a chunk outside the tile is bf16 zeros, as in tgemm_kernel (code 0 is not value 0)
            st16(W + tg_off<BKC>(lr + RPP * ps, ch), make_uint4(ok ? v[0] : 0u, ok ? v[1] : 0u, ok ? v[2] : 0u, ok ? v[3] : 0u));
        }
    };
    auto patch = [&](int buf, int kt) {     // this thread's exception into the W image of K tile kt
        if (ekt == kt) *reinterpret_cast<uint16_t*>(smem + buf * BUF + ABYTES + eoff) = (uint16_t)ebits;
    };

    gload(0);
    if (tid < 4) flg[tid] = 0u;
    __syncthreads();
    if (ekt >= 0) atomicOr(&flg[ekt >> 5], 1u << (ekt & 31));
    lstore(0);
    __syncthreads();
    const uint64_t flo = (uint64_t)__builtin_amdgcn_readfirstlane(flg[0]) | (uint64_t)__builtin_amdgcn_readfirstlane(flg[1]) << 32;
    const uint64_t fhi = (uint64_t)__builtin_amdgcn_readfirstlane(flg[2]) | (uint64_t)__builtin_amdgcn_readfirstlane(flg[3]) << 32;
    auto flagged = [flo, fhi](int t) { return (((t < 64 ? flo : fhi) >> (t & 63)) & 1u) != 0u; };
    if (flagged(0)) {
        patch(0, 0);
        __syncthreads();
    }

    f32x4_t acc[4][MI];   // [weight sub-tile j][token sub-tile i]
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < MI; ++i) acc[j][i] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    const int h = lane >> 4, c16 = lane & 15;
    int wrow[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) wrow[j] = SW ? ((j < 2 ? 0 : 64) + 32 * wn + 16 * (j & 1)) : (64 * wn + 16 * j);

    const int KT = (K + BK - 1) / BK;
    for (int kt = 0; kt < KT; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < KT) gload((kt + 1) * BK);
        const char* A = smem + buf * BUF;
        const char* W = A + ABYTES;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            bf16x8_t af[MI], wf[4];
#pragma unroll
            for (int i = 0; i < MI; ++i)
                af[i] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(A + tg_off<BKC>(16 * MI * wm + 16 * i + c16, s * 4 + h)));
#pragma unroll
            for (int j = 0; j < 4; ++j)
                wf[j] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(W + tg_off<BKC>(wrow[j] + c16, s * 4 + h)));
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < MI; ++i) acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], af[i], acc[j][i], 0, 0, 0);
        }
        if (kt + 1 < KT) {
            lstore(buf ^ 1);                   // buffer buf^1 was last read in iteration kt-1, behind a barrier
            if (flagged(kt + 1)) {             // uniform: the granule stores of every thread land before the patches
                __syncthreads();
                patch(buf ^ 1, kt + 1);
            }
        }
        __syncthreads();
    }

    int fbase[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) fbase[j] = n0 + (SW ? 32 * wn + 16 * (j & 1) : wrow[j]);
    tg_epilogue<EPI, MI>(p, g, acc, count, roff, row0 + 16 * MI * wm, fbase, lane);
}

template <int EPI, int MI, int BKC>
static int launch_tgemm_w12(const umoe_tgemm_args* a, const tg_w12& f, int max_n, hipStream_t s) {
    tg_pack gp;
    memset(&gp, 0, sizeof(gp));
    memcpy(gp.g, a->groups, sizeof(umoe_tgroup_t) * a->num_groups);
    constexpr int lds = 2 * (32 * MI * BKC * 16 + 128 * BKC * 16);
    static bool configured = false;
    if (!configured) {
        UMOE_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&tgemm_w12_kernel<EPI, MI, BKC>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        configured = true;
    }
    const int ntile = EPI == UMOE_EPI_SWIGLU ? 64 : 128;
    dim3 grid((unsigned)ceil_div(max_n, ntile), (unsigned)ceil_div(a->max_rows, 32 * MI), (unsigned)a->num_groups);
    tgemm_w12_kernel<EPI, MI, BKC><<<grid, 256, lds, s>>>(*a, gp, f);
    UMOE_LAUNCH_CHECK();
    return 0;
}

extern "C" int umoe_tiled_gemm_w12(const umoe_tgemm_args* a, const uint8_t* const* host_w12, const uint32_t* const* host_meta, umoe_stream_t stream) {
    UMOE_REQUIRE(a && a->groups && a->a && a->out && host_w12 && host_meta, "umoe_tiled_gemm_w12: null argument");
    UMOE_REQUIRE(a->num_groups > 0 && a->num_groups <= TG_MAXG, "umoe_tiled_gemm_w12: 1..%d groups per launch (got %d)", TG_MAXG, a->num_groups);
    UMOE_REQUIRE(a->max_rows > 0 && ceil_div(a->max_rows, 128) <= 65535, "umoe_tiled_gemm_w12: bad max_rows %d", a->max_rows);
    UMOE_REQUIRE((a->lda & 7) == 0, "umoe_tiled_gemm_w12: lda must be a multiple of 8");
    UMOE_REQUIRE(a->epilogue == UMOE_EPI_SWIGLU || a->epilogue == UMOE_EPI_BF16, "umoe_tiled_gemm_w12: epilogue %d (UMOE_EPI_SWIGLU or UMOE_EPI_BF16 only)",
                 a->epilogue);
    UMOE_REQUIRE(!a->aux_out, "umoe_tiled_gemm_w12: no aux_out (the pre-activations are a training output; train on bf16 weights)");
    tg_w12 f;
    memset(&f, 0, sizeof(f));
    int max_n = 0;
    for (int i = 0; i < a->num_groups; ++i) {
        const umoe_tgroup_t& g = a->groups[i];
        UMOE_REQUIRE(host_w12[i] && host_meta[i], "umoe_tiled_gemm_w12: group %d: host_w12 / host_meta hold a null pointer (WP12 blocks %p, block records %p)", i,
                     (const void*)host_w12[i], (const void*)host_meta[i]);
        UMOE_REQUIRE(((uintptr_t)host_w12[i] & 15) == 0, "umoe_tiled_gemm_w12: group %d: host_w12 must be 16-byte aligned", i);
        UMOE_REQUIRE(((uintptr_t)host_meta[i] & 3) == 0, "umoe_tiled_gemm_w12: group %d: host_meta must be 4-byte aligned", i);
        UMOE_REQUIRE(!g.w_kmajor && !g.k_off && !g.k_count && !g.k_compact_a && !g.k_compact_w && !g.bias,
                     "umoe_tiled_gemm_w12: group %d: no K-major weights (w_kmajor), K windows (k_off / k_count / k_compact_*) or bias on WP12 weights", i);
        UMOE_REQUIRE(g.n > 0 && g.k > 0 && g.k % 32 == 0 && (g.a_col_off & 7) == 0, "umoe_tiled_gemm_w12: group %d: need n > 0, k %% 32 == 0 (n=%d k=%d)", i,
                     g.n, g.k);
        UMOE_REQUIRE(g.k / 32 < 127, "umoe_tiled_gemm_w12: group %d: k / 32 < 127 (k=%d): a block record counts k-steps in 7 bits", i, g.k);
        UMOE_REQUIRE(a->epilogue != UMOE_EPI_SWIGLU || g.n % 16 == 0, "umoe_tiled_gemm_w12: group %d: SwiGLU needs n %% 16 == 0 (interleaved blocks; n=%d)", i, g.n);
        f.w[i] = host_w12[i];
        f.m[i] = host_meta[i];
        if (g.n > max_n) max_n = g.n;
    }
    hipStream_t s = (hipStream_t)stream;
    const bool big = umoe_tgemm_tm(a) == 256;
    if (a->epilogue == UMOE_EPI_SWIGLU)
        return big ? launch_tgemm_w12<UMOE_EPI_SWIGLU, 8, 4>(a, f, max_n, s) : launch_tgemm_w12<UMOE_EPI_SWIGLU, 4, 8>(a, f, max_n, s);
    return big ? launch_tgemm_w12<UMOE_EPI_BF16, 8, 4>(a, f, max_n, s) : launch_tgemm_w12<UMOE_EPI_BF16, 4, 8>(a, f, max_n, s);
}
