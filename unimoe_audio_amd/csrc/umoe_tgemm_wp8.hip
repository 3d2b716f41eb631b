// The tiled MFMA GEMM (umoe_tgemm.hip, tgemm_kernel) with a WP8 weight source: prefill on e4m3 expert weights.
//
//   Y[rows(g), N] = epilogue( A[rows(g), K] * W_g^T ),  W_g = q * 2^e held as WP8 blocks (include/umoe.h) + one int8 exponent per row
//
// The register-staging form of tgemm_kernel with one change: where the bf16 kernel loads a 16-byte chunk (8 bf16 of one weight row)
// and stores it into the swizzled LDS image, this one loads the 8 e4m3 BYTES of the same granule straight from the WP8 blocks, converts
// them with the row's 2^e (flat_f8_frag: v_cvt_scalef32_pk_bf16_fp8, exact) and stores the resulting 16 bytes at the same LDS offset.
// Everything behind the store is shared code or the same code -- the LDS image (tg_off), the ds_read_b128 operand reads, the MFMA order,
// the K loop, tg_epilogue -- so the output is BIT-IDENTICAL to tgemm_kernel run on the dequantized weights.
//
// Granule addressing (K % 32 == 0, so a K quarter Q = K / 4 is a multiple of 8 and an 8-element granule never straddles one): column k
// of weight row n lies in quarter h = k / Q at o = k - h Q, i.e. chunk i = o / 16, byte j0 = o % 16 (0 or 8) of lane 16 h + (n & 15) of
// block nb = n / 16:  byte ((nb KB2 + i) 64 + 16 h + (n & 15)) 16 + j0,  KB2 = ceil(K / 64).  The zero bytes behind a quarter's end
// (Q % 16 == 8, e.g. K = 1376) and the padded rows of the last block are never read: o < Q and n < N for every load.
// SwiGLU: gate row n sits in block 2 (n / 16), up row n in block 2 (n / 16) + 1 of the interleaved pair; exponents 16 per block.
//
// Weight traffic: the 256 threads fetch a 128-row x 64-column tile as 8-byte loads, 8 rows x 16 bytes contiguous per k-chunk
// (128-byte lines), half the bytes of the bf16 tile.  Roofline as tgemm_kernel (MFMA); an admission prefill of ~100 rows is bound by the
// expert weight bytes, which this halves.
#include <string.h>

#include "umoe_tgemm_dev.h"
#include "umoe_flat_dev.h"      // flat_f8_frag, flat_f8_scale

struct tg_f8 {                          // a kernel argument of its own (umoe_tgroup_t stays as it is)
    const uint8_t* w8[TG_MAXG];         // WP8 blocks of group g (SwiGLU: the interleaved gate/up pair)
    const int8_t* ex[TG_MAXG];          // their exponents, 16 per block
};

// MI / BKC as tgemm_kernel: (4, 8) 128-token tiles, K steps of 64; (8, 4) 256-token tiles, K steps of 32.  Two LDS buffers.
template <int EPI, int MI, int BKC>
__global__ __launch_bounds__(256, 2) void tgemm_wp8_kernel(const umoe_tgemm_args p, const tg_pack gp, const tg_f8 f8) {
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [2 buffers][A tile | W tile]
    constexpr int TM = 32 * MI;
    constexpr int RPP = 256 / BKC;
    constexpr int APS = TM / RPP, WPS = 128 / RPP;
    constexpr int ABYTES = TM * BKC * 16, WBYTES = 128 * BKC * 16, BUF = ABYTES + WBYTES;
    constexpr int KS = BKC / 4;
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
    // weight rows: lane address of the row inside its block, and the row's scale -- read once, before the K loop
    const int Q = K >> 2, KB2 = (K + 63) >> 6;
    const uint8_t* wp[WPS];
    float wsc[WPS];
    bool wok[WPS];
#pragma unroll
    for (int ps = 0; ps < WPS; ++ps) {
        const int tr = lr + RPP * ps;   // tile row 0..127
        const int n = n0 + (SW ? (tr & 63) : tr);
        wok[ps] = n < g.n;
        const int nn = wok[ps] ? n : 0;
        const int blk = SW ? 2 * (nn >> 4) + (tr >= 64 ? 1 : 0) : (nn >> 4);
        wp[ps] = f8.w8[blockIdx.z] + ((long)blk * KB2 * 64 + (nn & 15)) * 16;
        wsc[ps] = flat_f8_scale(wok[ps] ? (int)f8.ex[blockIdx.z][blk * 16 + (nn & 15)] : 0);
    }
    uint4 ra[APS];
    uint2 rw[WPS];                      // the granule as loaded: 8 e4m3 bytes (converted on the way into LDS)
    auto gload = [&](int k0) {
        const int k = k0 + ch * 8;
        const bool kok = k < K;         // K % 8 == 0: a granule is entirely inside or outside
        const int h = (k >= Q ? 1 : 0) + (k >= 2 * Q ? 1 : 0) + (k >= 3 * Q ? 1 : 0);
        const int o = k - h * Q;
        const int woff = (o >> 4) * 1024 + h * 256 + (o & 15);
#pragma unroll
        for (int ps = 0; ps < APS; ++ps) {
            ra[ps] = make_uint4(0, 0, 0, 0);
            if (kok && aok[ps]) ra[ps] = ld16(ap[ps] + k0);
        }
#pragma unroll
        for (int ps = 0; ps < WPS; ++ps) {
            rw[ps] = make_uint2(0, 0);  // e4m3 zeros convert to bf16 zeros: the image of a chunk outside the tile
            if (kok && wok[ps]) rw[ps] = *reinterpret_cast<const uint2*>(wp[ps] + woff);
        }
    };
    auto lstore = [&](int buf) {
        char* A = smem + buf * BUF;
        char* W = A + ABYTES;
#pragma unroll
        for (int ps = 0; ps < APS; ++ps) st16(A + tg_off<BKC>(lr + RPP * ps, ch), ra[ps]);
#pragma unroll
        for (int ps = 0; ps < WPS; ++ps)
            st16(W + tg_off<BKC>(lr + RPP * ps, ch), __builtin_bit_cast(uint4, flat_f8_frag(rw[ps].x, rw[ps].y, wsc[ps])));
    };

    f32x4_t acc[4][MI];   // [weight sub-tile j][token sub-tile i]
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < MI; ++i) acc[j][i] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    const int h = lane >> 4, c16 = lane & 15;
    int wrow[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) wrow[j] = SW ? ((j < 2 ? 0 : 64) + 32 * wn + 16 * (j & 1)) : (64 * wn + 16 * j);

    constexpr int BK = BKC * 8;
    const int KT = (K + BK - 1) / BK;
    gload(0);
    lstore(0);
    __syncthreads();
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
        if (kt + 1 < KT) lstore(buf ^ 1);      // buffer buf^1 was last read in iteration kt-1, behind a barrier
        __syncthreads();
    }

    int fbase[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) fbase[j] = n0 + (SW ? 32 * wn + 16 * (j & 1) : wrow[j]);
    tg_epilogue<EPI, MI>(p, g, acc, count, roff, row0 + 16 * MI * wm, fbase, lane);
}

template <int EPI, int MI, int BKC>
static int launch_tgemm_wp8(const umoe_tgemm_args* a, const tg_f8& f8, int max_n, hipStream_t s) {
    tg_pack gp;
    memset(&gp, 0, sizeof(gp));
    memcpy(gp.g, a->groups, sizeof(umoe_tgroup_t) * a->num_groups);
    constexpr int lds = 2 * (32 * MI * BKC * 16 + 128 * BKC * 16);
    static bool configured = false;
    if (!configured) {
        UMOE_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&tgemm_wp8_kernel<EPI, MI, BKC>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        configured = true;
    }
    const int ntile = EPI == UMOE_EPI_SWIGLU ? 64 : 128;
    dim3 grid((unsigned)ceil_div(max_n, ntile), (unsigned)ceil_div(a->max_rows, 32 * MI), (unsigned)a->num_groups);
    tgemm_wp8_kernel<EPI, MI, BKC><<<grid, 256, lds, s>>>(*a, gp, f8);
    UMOE_LAUNCH_CHECK();
    return 0;
}

extern "C" int umoe_tiled_gemm_wp8(const umoe_tgemm_args* a, const uint8_t* const* host_w8, const int8_t* const* host_exps, umoe_stream_t stream) {
    UMOE_REQUIRE(a && a->groups && a->a && a->out && host_w8 && host_exps, "umoe_tiled_gemm_wp8: null argument");
    UMOE_REQUIRE(a->num_groups > 0 && a->num_groups <= TG_MAXG, "umoe_tiled_gemm_wp8: 1..%d groups per launch (got %d)", TG_MAXG, a->num_groups);
    UMOE_REQUIRE(a->max_rows > 0 && ceil_div(a->max_rows, 128) <= 65535, "umoe_tiled_gemm_wp8: bad max_rows %d", a->max_rows);
    UMOE_REQUIRE((a->lda & 7) == 0, "umoe_tiled_gemm_wp8: lda must be a multiple of 8");
    UMOE_REQUIRE(a->epilogue == UMOE_EPI_SWIGLU || a->epilogue == UMOE_EPI_BF16, "umoe_tiled_gemm_wp8: epilogue %d (UMOE_EPI_SWIGLU or UMOE_EPI_BF16 only)",
                 a->epilogue);
    UMOE_REQUIRE(!a->aux_out, "umoe_tiled_gemm_wp8: no aux_out (the pre-activations are a training output; train on bf16 weights)");
    tg_f8 f8;
    memset(&f8, 0, sizeof(f8));
    int max_n = 0;
    for (int i = 0; i < a->num_groups; ++i) {
        const umoe_tgroup_t& g = a->groups[i];
        UMOE_REQUIRE(host_w8[i] && host_exps[i], "umoe_tiled_gemm_wp8: group %d: null WP8 blocks or exponents", i);
        UMOE_REQUIRE(!g.w_kmajor && !g.k_off && !g.k_count && !g.k_compact_a && !g.k_compact_w && !g.bias,
                     "umoe_tiled_gemm_wp8: group %d: no K-major weights, K windows or bias on WP8 weights", i);
        UMOE_REQUIRE(g.n > 0 && g.k > 0 && g.k % 32 == 0 && (g.a_col_off & 7) == 0, "umoe_tiled_gemm_wp8: group %d: need n > 0, k %% 32 == 0 (n=%d k=%d)", i,
                     g.n, g.k);
        UMOE_REQUIRE(a->epilogue != UMOE_EPI_SWIGLU || g.n % 16 == 0, "umoe_tiled_gemm_wp8: group %d: SwiGLU needs n %% 16 == 0 (interleaved blocks; n=%d)", i, g.n);
        f8.w8[i] = host_w8[i];
        f8.ex[i] = host_exps[i];
        if (g.n > max_n) max_n = g.n;
    }
    hipStream_t s = (hipStream_t)stream;
    const bool big = umoe_tgemm_tm(a) == 256;
    if (a->epilogue == UMOE_EPI_SWIGLU)
        return big ? launch_tgemm_wp8<UMOE_EPI_SWIGLU, 8, 4>(a, f8, max_n, s) : launch_tgemm_wp8<UMOE_EPI_SWIGLU, 4, 8>(a, f8, max_n, s);
    return big ? launch_tgemm_wp8<UMOE_EPI_BF16, 8, 4>(a, f8, max_n, s) : launch_tgemm_wp8<UMOE_EPI_BF16, 4, 8>(a, f8, max_n, s);
}
