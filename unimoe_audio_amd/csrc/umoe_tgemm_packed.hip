// The tiled MFMA GEMM (umoe_tgemm.hip, tgemm_kernel) on packed expert weights: prefill on e4m3 (WP8) and on the lossless 12-bit (WP12)
// copies of the bf16 weights.
//
//   Y[rows(g), N] = epilogue( A[rows(g), K] * W_g^T )
//      WP8:  W_g = q * 2^e held as WP8 blocks (include/umoe.h) + one int8 exponent per row
//      WP12: W_g = bf16 weights held as WP12 blocks + block records (include/umoe.h "WP12")
//
// One body (tg_rs_body), the register-staging form of tgemm_kernel with one change: where the bf16 kernel loads a 16-byte chunk (8 bf16 of
// one weight row) and stores it into the swizzled LDS image, a weight source loads the same granule in its packed form, rebuilds the 16
// bytes exactly and the body stores them at the same LDS offset.  Everything behind the store is shared code or the same code -- the LDS
// image (tg_off), the ds_read_b128 operand reads, the MFMA order, the K loop, tg_epilogue -- so the output is BIT-IDENTICAL to
// tgemm_kernel run on the dequantized (WP8) or row-major (WP12) weights.
//
// A source holds the state of this thread's weight rows (set once, before the K loop), load(k, kok) of the granule at column k of each of
// them, image(ps): the 16 bytes of row pass ps for LDS, and two hooks: first_loaded() behind the first load, and stored(W, kt) behind
// the granule stores of K tile kt into the W image, in front of the barrier that publishes the buffer.  Both hooks are uniform for the
// workgroup.
//
// K % 32 == 0, so a K quarter Q = K / 4 is a multiple of 8 and an 8-element granule never straddles one: column k of weight row n lies in
// quarter h = k / Q at o = k - h Q, in lane 16 h + (n & 15) of block nb = n / 16.  SwiGLU: gate row n sits in block 2 (n / 16), up row n
// in block 2 (n / 16) + 1 of the interleaved pair.  Only n < N and k < K are ever addressed.
//
// Roofline as tgemm_kernel (MFMA); an admission prefill of ~100 rows is bound by the expert weight bytes: the 256 threads fetch a
// 128-row x 64-column tile as 8-byte loads (WP8, 8 rows x 16 bytes contiguous per k-chunk, half the bytes of the bf16 tile) or as 8-byte +
// 4-byte loads (WP12, 0.75 of them).
#include <string.h>

#include "umoe_tgemm_dev.h"
#include "umoe_flat_dev.h"      // flat_f8_frag, flat_f8_scale; flat_w12_frag, FLAT_W12_META

struct tg_f8 {                          // the kernel argument beside umoe_tgroup_t
    const uint8_t* w8[TG_MAXG];         // WP8 blocks of group g (SwiGLU: the interleaved gate/up pair)
    const int8_t* ex[TG_MAXG];          // their exponents, 16 per block
};
struct tg_w12 {
    const uint8_t* w[TG_MAXG];          // WP12 blocks of group g (SwiGLU: the interleaved gate/up pair)
    const uint32_t* m[TG_MAXG];         // their block records, FLAT_W12_META words per block
};

// tile row tr (0..127) of the weight tile at feature n0 -> block blk and weight row nn (0 behind N) of the group; true: the row is below N
template <bool SW>
__device__ __forceinline__ bool tg_wrow(int tr, int n0, int N, int& blk, int& nn) {
    const int n = n0 + (SW ? (tr & 63) : tr);
    const bool ok = n < N;
    nn = ok ? n : 0;
    blk = SW ? 2 * (nn >> 4) + (tr >= 64 ? 1 : 0) : (nn >> 4);
    return ok;
}
// the K quarter of column k
__device__ __forceinline__ int tg_quarter(int k, int Q) { return (k >= Q ? 1 : 0) + (k >= 2 * Q ? 1 : 0) + (k >= 3 * Q ? 1 : 0); }

// ---- WP8: chunk i = o / 16, byte j0 = o % 16 (0 or 8):  byte ((nb KB2 + i) 64 + 16 h + (n & 15)) 16 + j0,  KB2 = ceil(K / 64); exponents
// 16 per block.  The zero bytes behind a quarter's end (Q % 16 == 8, e.g. K = 1376) and the padded rows of the last block are never
// read: o < Q and n < N for every load.  The granule becomes bf16 with the row's 2^e (flat_f8_frag: v_cvt_scalef32_pk_bf16_fp8, exact).
template <bool SW, int BKC>
struct tg_wp8 {
    using args = tg_f8;
    static constexpr int RPP = 256 / BKC, WPS = 128 / RPP;
    int Q;
    const uint8_t* wp[WPS];             // lane address of the row inside its block
    float wsc[WPS];                     // the row's scale
    bool wok[WPS];
    uint2 rw[WPS];                      // the granule as loaded: 8 e4m3 bytes (converted on the way into LDS)

    __device__ __forceinline__ void rows(const args f, const int N, const int K, const int n0, const int tid) {
        const int lr = tid / BKC, KB2 = (K + 63) >> 6;
        Q = K >> 2;
#pragma unroll
        for (int ps = 0; ps < WPS; ++ps) {
            int blk, nn;
            wok[ps] = tg_wrow<SW>(lr + RPP * ps, n0, N, blk, nn);
            wp[ps] = f.w8[blockIdx.z] + ((long)blk * KB2 * 64 + (nn & 15)) * 16;
            wsc[ps] = flat_f8_scale(wok[ps] ? (int)f.ex[blockIdx.z][blk * 16 + (nn & 15)] : 0);
        }
    }
    __device__ __forceinline__ void load(const int k, const bool kok) {
        const int h = tg_quarter(k, Q);
        const int o = k - h * Q;
        const int woff = (o >> 4) * 1024 + h * 256 + (o & 15);
#pragma unroll
        for (int ps = 0; ps < WPS; ++ps) {
            rw[ps] = make_uint2(0, 0);  // e4m3 zeros convert to bf16 zeros: the image of a chunk outside the tile
            if (kok && wok[ps]) rw[ps] = *reinterpret_cast<const uint2*>(wp[ps] + woff);
        }
    }
    __device__ __forceinline__ uint4 image(const int ps) const { return __builtin_bit_cast(uint4, flat_f8_frag(rw[ps].x, rw[ps].y, wsc[ps])); }
    __device__ __forceinline__ void first_loaded() {}
    template <bool FIRST>
    __device__ __forceinline__ void stored(char*, int) {}
};

// ---- WP12 (follows w12.pack): KB = K / 32, k-step i = o / 8; a block starts at byte nb KB 768.  With CS = 2 for even KB, else 1
// (k-steps per chunk): u = ((i / CS) 64 + lane) CS + i % CS; the low bytes are at u 8, the code word at KB 512 + u 4.  The window base is
// word 39 of the block's 40-word record.  The granule's 8 raw low bytes and its one code word become the 16 bytes with flat_w12_frag
// (umoe_flat_dev.h: 12 VALU, exact).
//
// Exceptions (at most 32 per block, k-step << 25 | lane << 19 | element << 16 | bits): a K tile walks columns in ascending k, which is
// not the record's k-step order (the quarter sits in the lane field), so the flat kernels' cursor does not carry over.  Here thread
// (b = tid / 32, x = tid % 32) keeps entry x of the tile row's block b in a register, with the K tile it falls in and its byte offset in
// the LDS image; a bit mask of the K tiles that hold an entry is built once in LDS and kept in SGPRs.  On a flagged K tile -- a branch
// that is uniform for the workgroup -- a barrier separates the granule stores from the 2-byte patches, and the barrier that publishes
// the buffer follows as in every tile.  An unflagged tile runs the WP8 source's sequence.  No hand-off other than __syncthreads.
template <bool SW, int BKC>
struct tg_wp12 {
    using args = tg_w12;
    static constexpr int RPP = 256 / BKC, WPS = 128 / RPP, BK = BKC * 8;
    int Q, sh, tid;                     // sh: log2 of the k-steps per chunk
    const uint8_t* wbase;
    uint32_t wo[WPS], wc[WPS], wb4[WPS];      // byte offsets of the row's low bytes and code words at u = 0; the window base in every byte
    bool wok[WPS];
    int ekt, eoff;                      // this thread's exception entry: the K tile it falls in (-1: none) and its byte offset in the W image
    uint32_t ebits;
    uint2 rl[WPS];                      // the granule as loaded: 8 low bytes and
    uint32_t rc[WPS];                   // its code word (rebuilt on the way into LDS)
    bool rk;                            // the loaded K tile's granule lies inside K
    uint64_t flo, fhi;                  // bit t: K tile t holds an exception of this tile row (K / 32 < 127: at most 126 K tiles)

    static __device__ __forceinline__ uint32_t* flags() {
        __shared__ uint32_t flg[4];
        return flg;
    }
    __device__ __forceinline__ void rows(const args f, const int N, const int K, const int n0, const int tid_) {
        const int lr = tid_ / BKC, KB = K >> 5;
        const uint32_t* const mbase = f.m[blockIdx.z];
        wbase = f.w[blockIdx.z];
        tid = tid_;
        Q = K >> 2;
        sh = (KB & 1) ? 0 : 1;
#pragma unroll
        for (int ps = 0; ps < WPS; ++ps) {
            int blk, nn;
            wok[ps] = tg_wrow<SW>(lr + RPP * ps, n0, N, blk, nn);
            const uint32_t boff = (uint32_t)blk * (uint32_t)KB * 768u, rs = (uint32_t)((nn & 15) << sh);
            wo[ps] = boff + rs * 8u;
            wc[ps] = boff + (uint32_t)KB * 512u + rs * 4u;
            wb4[ps] = (mbase[blk * FLAT_W12_META + FLAT_W12_META - 1] & 0xffu) * 0x01010101u;
        }
        // entry (tid % 32) of block (tid / 32) of the tile row (a record holds at most 32 and a sentinel)
        ekt = -1; eoff = 0; ebits = 0;
        const int b = tid >> 5, x = tid & 31;
        const int nblk = n0 + (SW ? (b & 3) : b) * 16;          // first weight row (feature) of the block
        if (nblk < N) {
            const int blk = SW ? 2 * (nblk >> 4) + (b >> 2) : (nblk >> 4);
            const uint32_t en = mbase[blk * FLAT_W12_META + x];
            const int ks = (int)(en >> 25), el = (int)((en >> 19) & 63u), ej = (int)((en >> 16) & 7u);
            const int n = nblk + (el & 15), col = (el >> 4) * Q + ks * 8 + ej;
            if (ks != 127 && n < N && ks * 8 < Q) {             // (the sentinel reads as k-step 127; rows behind N are never patched)
                const int trow = (SW ? (b >> 2) * 64 + (b & 3) * 16 : b * 16) + (el & 15);
                ekt = col / BK;
                eoff = tg_off<BKC>(trow, (col % BK) >> 3) + (col & 7) * 2;
                ebits = en & 0xffffu;
            }
        }
    }
    __device__ __forceinline__ void load(const int k, const bool kok) {
        const int h = tg_quarter(k, Q);
        const int i = (k - h * Q) >> 3;
        const uint32_t u = (uint32_t)((((i >> sh) << 6) + 16 * h) << sh) + (uint32_t)(i & sh);      // (the row's term is in wo / wc)
        rk = kok;
#pragma unroll
        for (int ps = 0; ps < WPS; ++ps) {
            rl[ps] = make_uint2(0, 0);
            rc[ps] = 0;
            if (kok && wok[ps]) {
                rl[ps] = *reinterpret_cast<const uint2*>(wbase + wo[ps] + u * 8u);
                rc[ps] = *reinterpret_cast<const uint32_t*>(wbase + wc[ps] + u * 4u);
            }
        }
    }
    __device__ __forceinline__ uint4 image(const int ps) const {
        const flat_u32x4 v = flat_w12_frag(rl[ps].x, rl[ps].y, rc[ps], wb4[ps]);
        const bool ok = rk && wok[ps];      // a chunk outside the tile is bf16 zeros, as in tgemm_kernel (code 0 is not value 0)
        return make_uint4(ok ? v[0] : 0u, ok ? v[1] : 0u, ok ? v[2] : 0u, ok ? v[3] : 0u);
    }
    __device__ __forceinline__ void first_loaded() {
        uint32_t* flg = flags();
        if (tid < 4) flg[tid] = 0u;
        __syncthreads();
        if (ekt >= 0) atomicOr(&flg[ekt >> 5], 1u << (ekt & 31));
    }
    template <bool FIRST>
    __device__ __forceinline__ void stored(char* W, const int kt) {
        if constexpr (FIRST) {          // the first tile's barrier publishes the flag words too; the mask stays in SGPRs
            __syncthreads();
            const uint32_t* flg = flags();
            flo = (uint64_t)__builtin_amdgcn_readfirstlane(flg[0]) | (uint64_t)__builtin_amdgcn_readfirstlane(flg[1]) << 32;
            fhi = (uint64_t)__builtin_amdgcn_readfirstlane(flg[2]) | (uint64_t)__builtin_amdgcn_readfirstlane(flg[3]) << 32;
        }
        if ((((kt < 64 ? flo : fhi) >> (kt & 63)) & 1u) != 0u) {      // uniform: the granule stores of every thread land before the patches
            if constexpr (!FIRST) __syncthreads();
            if (ekt == kt) *reinterpret_cast<uint16_t*>(W + eoff) = (uint16_t)ebits;
        }
    }
};

// MI / BKC as tgemm_kernel: (4, 8) 128-token tiles, K steps of 64; (8, 4) 256-token tiles, K steps of 32.  Two LDS buffers.
template <template <bool, int> class SRC, int EPI, int MI, int BKC>
__device__ __forceinline__ void tg_rs_body(const umoe_tgemm_args p, const tg_pack gp, const typename SRC<EPI == UMOE_EPI_SWIGLU, BKC>::args f) {
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
    SRC<SW, BKC> src;
    src.rows(f, g.n, K, n0, tid);
    uint4 ra[APS];
    auto gload = [&](int k0) {
        const int k = k0 + ch * 8;
        const bool kok = k < K;         // K % 8 == 0: a granule is entirely inside or outside
#pragma unroll
        for (int ps = 0; ps < APS; ++ps) {
            ra[ps] = make_uint4(0, 0, 0, 0);
            if (kok && aok[ps]) ra[ps] = ld16(ap[ps] + k0);
        }
        src.load(k, kok);
    };
    auto lstore = [&](int buf) {
        char* A = smem + buf * BUF;
        char* W = A + ABYTES;
#pragma unroll
        for (int ps = 0; ps < APS; ++ps) st16(A + tg_off<BKC>(lr + RPP * ps, ch), ra[ps]);
#pragma unroll
        for (int ps = 0; ps < WPS; ++ps) st16(W + tg_off<BKC>(lr + RPP * ps, ch), src.image(ps));
    };

    gload(0);
    src.first_loaded();
    lstore(0);
    src.template stored<true>(smem + ABYTES, 0);
    __syncthreads();

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
            src.template stored<false>(smem + (buf ^ 1) * BUF + ABYTES, kt + 1);
        }
        __syncthreads();
    }

    int fbase[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) fbase[j] = n0 + (SW ? 32 * wn + 16 * (j & 1) : wrow[j]);
    tg_epilogue<EPI, MI>(p, g, acc, count, roff, row0 + 16 * MI * wm, fbase, lane);
}

template <int EPI, int MI, int BKC>
__global__ __launch_bounds__(256, 2) void tgemm_wp8_kernel(const umoe_tgemm_args p, const tg_pack gp, const tg_f8 f8) {
    tg_rs_body<tg_wp8, EPI, MI, BKC>(p, gp, f8);
}
template <int EPI, int MI, int BKC>
__global__ __launch_bounds__(256, 2) void tgemm_w12_kernel(const umoe_tgemm_args p, const tg_pack gp, const tg_w12 f) {
    tg_rs_body<tg_wp12, EPI, MI, BKC>(p, gp, f);
}

template <int EPI, int MI, int BKC, typename ARGS>
static int launch_tgemm_packed(const umoe_tgemm_args* a, const ARGS& f, int max_n, hipStream_t s) {
    tg_pack gp;
    memset(&gp, 0, sizeof(gp));
    memcpy(gp.g, a->groups, sizeof(umoe_tgroup_t) * a->num_groups);
    constexpr int lds = 2 * (32 * MI * BKC * 16 + 128 * BKC * 16);
    void (*kernel)(const umoe_tgemm_args, const tg_pack, const ARGS);
    if constexpr (std::is_same_v<ARGS, tg_f8>) kernel = &tgemm_wp8_kernel<EPI, MI, BKC>;
    else kernel = &tgemm_w12_kernel<EPI, MI, BKC>;
    static bool configured = false;
    if (!configured) {
        UMOE_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        configured = true;
    }
    const int ntile = EPI == UMOE_EPI_SWIGLU ? 64 : 128;
    dim3 grid((unsigned)ceil_div(max_n, ntile), (unsigned)ceil_div(a->max_rows, 32 * MI), (unsigned)a->num_groups);
    kernel<<<grid, 256, lds, s>>>(*a, gp, f);
    UMOE_LAUNCH_CHECK();
    return 0;
}

template <typename ARGS>
static int dispatch_tgemm_packed(const umoe_tgemm_args* a, const ARGS& f, int max_n, hipStream_t s) {
    const bool big = umoe_tgemm_tm(a) == 256;
    if (a->epilogue == UMOE_EPI_SWIGLU)
        return big ? launch_tgemm_packed<UMOE_EPI_SWIGLU, 8, 4>(a, f, max_n, s) : launch_tgemm_packed<UMOE_EPI_SWIGLU, 4, 8>(a, f, max_n, s);
    return big ? launch_tgemm_packed<UMOE_EPI_BF16, 8, 4>(a, f, max_n, s) : launch_tgemm_packed<UMOE_EPI_BF16, 4, 8>(a, f, max_n, s);
}

// What both entries refuse alike.  fn: the entry point; fmt: its weight format; w_name, x_name: its two pointer lists, host_w and host_x.
// max_n: the widest group.
static int tg_packed_check(const umoe_tgemm_args* a, const char* fn, const char* fmt, const char* w_name, const char* x_name, const void* const* host_w,
                           const void* const* host_x, int* max_n) {
    UMOE_REQUIRE(a && a->groups && a->a && a->out && host_w && host_x, "%s: null argument", fn);
    UMOE_REQUIRE(a->num_groups > 0 && a->num_groups <= TG_MAXG, "%s: 1..%d groups per launch (got %d)", fn, TG_MAXG, a->num_groups);
    UMOE_REQUIRE(a->max_rows > 0 && ceil_div(a->max_rows, 128) <= 65535, "%s: bad max_rows %d", fn, a->max_rows);
    UMOE_REQUIRE((a->lda & 7) == 0, "%s: lda must be a multiple of 8", fn);
    UMOE_REQUIRE(a->epilogue == UMOE_EPI_SWIGLU || a->epilogue == UMOE_EPI_BF16, "%s: epilogue %d (UMOE_EPI_SWIGLU or UMOE_EPI_BF16 only)", fn, a->epilogue);
    UMOE_REQUIRE(!a->aux_out, "%s: no aux_out (the pre-activations are a training output; train on bf16 weights)", fn);
    *max_n = 0;
    for (int i = 0; i < a->num_groups; ++i) {
        const umoe_tgroup_t& g = a->groups[i];
        UMOE_REQUIRE(host_w[i] && host_x[i], "%s: group %d: %s / %s hold a null pointer (%p, %p)", fn, i, w_name, x_name, host_w[i], host_x[i]);
        UMOE_REQUIRE(!g.w_kmajor && !g.k_off && !g.k_count && !g.k_compact_a && !g.k_compact_w && !g.bias,
                     "%s: group %d: no K-major weights (w_kmajor), K windows (k_off / k_count / k_compact_*) or bias on %s weights", fn, i, fmt);
        UMOE_REQUIRE(g.n > 0 && g.k > 0 && g.k % 32 == 0 && (g.a_col_off & 7) == 0, "%s: group %d: need n > 0, k %% 32 == 0 (n=%d k=%d)", fn, i, g.n, g.k);
        UMOE_REQUIRE(a->epilogue != UMOE_EPI_SWIGLU || g.n % 16 == 0, "%s: group %d: SwiGLU needs n %% 16 == 0 (interleaved blocks; n=%d)", fn, i, g.n);
        if (g.n > *max_n) *max_n = g.n;
    }
    return 0;
}

extern "C" int umoe_tiled_gemm_wp8(const umoe_tgemm_args* a, const uint8_t* const* host_w8, const int8_t* const* host_exps, umoe_stream_t stream) {
    int max_n;
    if (const int rc = tg_packed_check(a, "umoe_tiled_gemm_wp8", "WP8", "host_w8", "host_exps", reinterpret_cast<const void* const*>(host_w8),
                                       reinterpret_cast<const void* const*>(host_exps), &max_n))
        return rc;
    tg_f8 f8;
    memset(&f8, 0, sizeof(f8));
    for (int i = 0; i < a->num_groups; ++i) {
        f8.w8[i] = host_w8[i];
        f8.ex[i] = host_exps[i];
    }
    return dispatch_tgemm_packed(a, f8, max_n, (hipStream_t)stream);
}

extern "C" int umoe_tiled_gemm_w12(const umoe_tgemm_args* a, const uint8_t* const* host_w12, const uint32_t* const* host_meta, umoe_stream_t stream) {
    int max_n;
    if (const int rc = tg_packed_check(a, "umoe_tiled_gemm_w12", "WP12", "host_w12", "host_meta", reinterpret_cast<const void* const*>(host_w12),
                                       reinterpret_cast<const void* const*>(host_meta), &max_n))
        return rc;
    tg_w12 f;
    memset(&f, 0, sizeof(f));
    for (int i = 0; i < a->num_groups; ++i) {
        UMOE_REQUIRE(((uintptr_t)host_w12[i] & 15) == 0, "umoe_tiled_gemm_w12: group %d: host_w12 must be 16-byte aligned", i);
        UMOE_REQUIRE(((uintptr_t)host_meta[i] & 3) == 0, "umoe_tiled_gemm_w12: group %d: host_meta must be 4-byte aligned", i);
        UMOE_REQUIRE(a->groups[i].k / 32 < 127, "umoe_tiled_gemm_w12: group %d: k / 32 < 127 (k=%d): a block record counts k-steps in 7 bits", i, a->groups[i].k);
        f.w[i] = host_w12[i];
        f.m[i] = host_meta[i];
    }
    return dispatch_tgemm_packed(a, f, max_n, (hipStream_t)stream);
}
