// DAC convolutions on the f32-input MFMA (v_mfma_f32_16x16x4_f32): the opt-in conv_form="mfma" of dac.py.  Same function as the direct
// kernels of umoe_dac.hip (Snake of the preceding layer fused into the input staging, zero outside [0, L), bias / tanh / residual in the
// store, tanh before the residual), same windows and per-row tables; fp32 in, fp32 accumulate: an MFMA is bit for bit a k-ordered fmaf
// chain, so this is exact f32 arithmetic in another summation order, not a reduced-precision path.
//
// Implicit GEMM.  M = output channels, N = output positions, reduction index r:
//   conv1d            r = ci K + k                       B[r][t] = snake?(x[ci][t stride - pad + k dil])        A[r][co] = wt[ci][k][co]
//   conv_transpose1d  per phase ph = (t + pad) mod stride, q = (t + pad) / stride, M = ceil(K / stride) taps k = ph + m stride:
//                     r = ci M + m                       B[r][q] = snake?(x[ci][q - m])                         A[r][co] = wt[ci][k][co], 0 where k >= K
// wt is the k-major copy [Cin][K][Cout] of the folded weight (dac.py makes it once), so a row of A is contiguous in co.
// Tile: 64 channels x 64 positions per 256-thread workgroup, reduction in chunks of KC = 32 (8 MFMA k-steps of 4).  Both operands are
// staged as [KC][64] images with a row stride of LS = 80 floats: a ds_read_b32 serves lanes {0-31} in one cycle, lanes 0-15 read row g
// and lanes 16-31 row g + 1 of a k-step, and 80 = 16 mod 32 puts them on disjoint banks.  Wave w owns the 32 x 32 quarter
// (w & 1, w >> 1): 2 x 2 MFMA tiles = 4 independent accumulators (16 VGPRs), 4 LDS reads per 4 MFMAs.  Wave w stages rows w, w + 4, ...
// of a chunk, so (ci, k) of a staged row is wave-uniform and lane l loads column l: every global load is one 256-byte row segment.
// LDS is a fixed 2 x 32 x 80 x 4 = 20 480 bytes whatever the geometry: there is no tile these kernels cannot stage, and several
// workgroups share a CU.  The global loads of chunk c + 1 (16 dwords per thread, into registers) are issued before the MFMAs of
// chunk c and consumed after them: one round trip per chunk, hidden behind the matrix work even where a layer fills few CUs.
// Roofline: f32 matrix peak 157 TF; per chunk and workgroup 32 MFMAs per wave (1024 cycles of issue) against 16 global dwords per thread.
//
// Order contract (the bit-identity of the full, windowed and per-row forms rests on it): every stored output passes through k-steps
// r = 0, 4, 8, ... in ascending order, each step summing its 4 terms in ascending r, up to the end of the last chunk; terms with
// r >= R, with k >= K (transposed) or whose input position lies outside [0, L) enter as fma(0, 0, acc) or fma(0, w, acc), which is
// exact.  r counts from 0 for every tile, window start, row and batch index, so the sequence never depends on them.
// MFMA ignores EXEC: every operand is staged for all 64 x 64 x KC cells (zero fill), every branch around an MFMA is on wave-uniform
// values, and only the stores are guarded per lane.
#include "umoe_common.h"
#include "umoe_dac_host.h"
#include "umoe_dac_snake.h"

namespace {
constexpr int TM = 64, TN = 64, KC = 32, LS = 80;

// Window of a WIN instantiation (absolute positions), as DacWin of umoe_dac.hip.
struct MfmaWin {
    int x_off, Lx, r_off, Lr, y_off, Ly, t_begin, n;
};

struct MfmaArgs {
    const float *x, *wt, *bias, *alpha, *resid;
    float* y;
    int Cin, L, Cout, K, stride, dil, pad, Lout, act;
};

__device__ __forceinline__ void mfma_chunk(const float* wl, const float* xl, int wm, int wn, int lane, f32x4_t (&acc)[2][2]) {
    const int c = lane & 15, g = lane >> 4;
#pragma unroll
    for (int ks = 0; ks < KC / 4; ++ks) {
        const int row = (ks * 4 + g) * LS;
        const float a0 = wl[row + wm + c], a1 = wl[row + wm + 16 + c];
        const float b0 = xl[row + wn + c], b1 = xl[row + wn + 16 + c];
        acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
    }
}

// y[b][co][t] = act( bias[co] + sum_r A[r][co] B[r][t] ) (+ resid[b][co][t]) for the tile at (t0, co0) of plane b
template <bool WIN>
__device__ __forceinline__ void conv1d_tile(const MfmaArgs& a, const MfmaWin& win, int t0, int co0, int b) {
    __shared__ float wl[KC * LS], xl[KC * LS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int Lx = WIN ? win.Lx : a.L, x_off = WIN ? win.x_off : 0;
    const float* xb = a.x + (size_t)b * a.Cin * Lx;
    const int R = a.Cin * a.K, K = a.K;
    const long long pbase = ((long long)t0 + lane) * a.stride - a.pad;      // input position of tap 0 of this lane's staging column
    const bool co_ok = co0 + lane < a.Cout;
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
    f32x4_t acc[2][2] = {};
    // a chunk's operands on their way: fetch() only issues the loads (nothing waits on them), stage() applies Snake and writes LDS
    float xr[KC / 4], wr[KC / 4], ar[KC / 4];
    unsigned live = 0;                                                       // bit j: xr[j] is an input value (Snake applies), not fill
    auto fetch = [&](int r0) {
        int r = r0 + wave, ci = r / K, k = r - ci * K;                       // wave-uniform
        live = 0;
#pragma unroll
        for (int j = 0; j < KC / 4; ++j) {
            xr[j] = 0.f, wr[j] = 0.f, ar[j] = 0.f;
            if (r < R) {
                const long long pos = pbase + (long long)k * a.dil;
                // (WIN: a position outside the buffer feeds only outputs past the window; the entry point checks the window's own)
                if (pos >= 0 && pos < a.L && (!WIN || (pos >= x_off && pos < (long long)x_off + Lx))) {
                    xr[j] = xb[(size_t)ci * Lx + (size_t)(pos - x_off)];
                    live |= 1u << j;
                }
                if (co_ok) wr[j] = a.wt[(size_t)r * a.Cout + co0 + lane];
                if (a.alpha) ar[j] = a.alpha[ci];
            }
            r += 4;
            k += 4;
            while (k >= K) {
                k -= K;
                ++ci;
            }
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int j = 0; j < KC / 4; ++j) {
            float xv = xr[j];
            if (a.alpha && (live >> j & 1)) xv = snake(xv, ar[j]);
            xl[(wave + 4 * j) * LS + lane] = xv;
            wl[(wave + 4 * j) * LS + lane] = wr[j];
        }
    };
    fetch(0);
    for (int r0 = 0; r0 < R; r0 += KC) {
        stage();
        __syncthreads();
        if (r0 + KC < R) fetch(r0 + KC);                                     // in flight while the MFMAs of this chunk run
        mfma_chunk(wl, xl, wm, wn, lane, acc);
        __syncthreads();
    }
    const int t_end = WIN ? win.t_begin + win.n : a.Lout;
    const int Ly = WIN ? win.Ly : a.Lout, y_off = WIN ? win.y_off : 0;
    const int Lr = WIN ? win.Lr : a.Lout, r_off = WIN ? win.r_off : 0;
    const int c = lane & 15, g = lane >> 4;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int co = co0 + wm + i * 16 + g * 4 + e;
            if (co >= a.Cout) continue;
            const float bv = a.bias ? a.bias[co] : 0.f;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const long long t = (long long)t0 + wn + j * 16 + c;
                if (t >= t_end) continue;
                float v = acc[i][j][e] + bv;
                if (a.act == 1) v = tanhf(v);
                if (a.resid) v += a.resid[((size_t)b * a.Cout + co) * Lr + (size_t)(t - r_off)];
                a.y[((size_t)b * a.Cout + co) * Ly + (size_t)(t - y_off)] = v;
            }
        }
}

// ConvTranspose1d, one phase per tile: blockIdx.x = tile * stride + phase; column n of the tile is q = q0 + n, output t = q stride + ph - pad.
// Outputs [t_lo, t_end) are stored (a tile's first q may lie before the window's first output of its phase).
template <bool WIN>
__device__ __forceinline__ void convt1d_tile(const MfmaArgs& a, const MfmaWin& win, long long q0, int ph, int co0, int b) {
    __shared__ float wl[KC * LS], xl[KC * LS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int Lx = WIN ? win.Lx : a.L, x_off = WIN ? win.x_off : 0;
    const float* xb = a.x + (size_t)b * a.Cin * Lx;
    const int K = a.K, M = (K + a.stride - 1) / a.stride, R = a.Cin * M;
    const long long qs = q0 + lane;                                         // q of this lane's staging column
    const bool co_ok = co0 + lane < a.Cout;
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
    f32x4_t acc[2][2] = {};
    float xr[KC / 4], wr[KC / 4], ar[KC / 4];                                // as in conv1d_tile
    unsigned live = 0;
    auto fetch = [&](int r0) {
        int r = r0 + wave, ci = r / M, m = r - ci * M;                       // wave-uniform
        live = 0;
#pragma unroll
        for (int j = 0; j < KC / 4; ++j) {
            xr[j] = 0.f, wr[j] = 0.f, ar[j] = 0.f;
            const int k = ph + m * a.stride;
            if (r < R && k < K) {
                const long long pos = qs - m;
                if (pos >= 0 && pos < a.L && (!WIN || (pos >= x_off && pos < (long long)x_off + Lx))) {
                    xr[j] = xb[(size_t)ci * Lx + (size_t)(pos - x_off)];
                    live |= 1u << j;
                }
                if (co_ok) wr[j] = a.wt[((size_t)ci * K + k) * a.Cout + co0 + lane];
                if (a.alpha) ar[j] = a.alpha[ci];
            }
            r += 4;
            m += 4;
            while (m >= M) {
                m -= M;
                ++ci;
            }
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int j = 0; j < KC / 4; ++j) {
            float xv = xr[j];
            if (a.alpha && (live >> j & 1)) xv = snake(xv, ar[j]);
            xl[(wave + 4 * j) * LS + lane] = xv;
            wl[(wave + 4 * j) * LS + lane] = wr[j];
        }
    };
    fetch(0);
    for (int r0 = 0; r0 < R; r0 += KC) {
        stage();
        __syncthreads();
        if (r0 + KC < R) fetch(r0 + KC);
        mfma_chunk(wl, xl, wm, wn, lane, acc);
        __syncthreads();
    }
    const long long t_lo = WIN ? win.t_begin : 0, t_end = WIN ? (long long)win.t_begin + win.n : a.Lout;
    const int Ly = WIN ? win.Ly : a.Lout, y_off = WIN ? win.y_off : 0;
    const int c = lane & 15, g = lane >> 4;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int co = co0 + wm + i * 16 + g * 4 + e;
            if (co >= a.Cout) continue;
            const float bv = a.bias ? a.bias[co] : 0.f;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const long long t = (q0 + wn + j * 16 + c) * a.stride + ph - a.pad;
                if (t >= t_lo && t < t_end) a.y[((size_t)b * a.Cout + co) * Ly + (size_t)(t - y_off)] = acc[i][j][e] + bv;
            }
        }
}

// q tiles of a transposed window: outputs [t_begin, t_begin + n) cover q = (t + pad) / stride from q_first on, nq values
__host__ __device__ inline long long convt_q_first(int t_begin, int pad, int stride) { return ((long long)t_begin + pad) / stride; }
__host__ __device__ inline long long convt_q_count(int t_begin, int n, int pad, int stride) {
    return ((long long)t_begin + n - 1 + pad) / stride - ((long long)t_begin + pad) / stride + 1;
}

template <bool WIN>
__global__ __launch_bounds__(256) void dac_conv1d_mfma_kernel(MfmaArgs a, MfmaWin win) {
    conv1d_tile<WIN>(a, win, (WIN ? win.t_begin : 0) + (int)blockIdx.x * TN, (int)blockIdx.y * TM, (int)blockIdx.z);
}

template <bool WIN>
__global__ __launch_bounds__(256) void dac_convt1d_mfma_kernel(MfmaArgs a, MfmaWin win) {
    const int tile = (int)(blockIdx.x / (unsigned)a.stride), ph = (int)(blockIdx.x % (unsigned)a.stride);
    convt1d_tile<WIN>(a, win, convt_q_first(WIN ? win.t_begin : 0, a.pad, a.stride) + (long long)tile * TN, ph, (int)blockIdx.y * TM, (int)blockIdx.z);
}

// ---- every row of the launch (blockIdx.z) on a window of its own, read from row blockIdx.z of the table (umoe.h "Per-row window
// tables"; the same words as the direct kernels read).  The addresses depend on blockIdx.z alone, so the values are wave-uniform; a
// workgroup whose tile starts past its row's work (n = 0: the row is idle) leaves before the first barrier.
#define DAC_ROW_WIN(r) MfmaWin{(int)(r)[3], (int)(r)[4], (int)(r)[5], (int)(r)[6], (int)(r)[7], (int)(r)[8], (int)(r)[9], (int)(r)[10]}

__global__ __launch_bounds__(256) void dac_conv1d_rows_mfma_kernel(const int64_t* __restrict__ table, MfmaArgs a) {
    const int64_t* row = table + (size_t)blockIdx.z * UMOE_DAC_ROW_WORDS;
    const MfmaWin win = DAC_ROW_WIN(row);
    if ((int)(blockIdx.x * TN) >= win.n) return;
    a.x = reinterpret_cast<const float*>(row[0]);
    a.resid = reinterpret_cast<const float*>(row[1]);
    a.y = reinterpret_cast<float*>(row[2]);
    a.L = (int)row[11];
    conv1d_tile<true>(a, win, win.t_begin + (int)blockIdx.x * TN, (int)blockIdx.y * TM, 0);      // (plane 0: the planes are the row's own)
}

__global__ __launch_bounds__(256) void dac_convt1d_rows_mfma_kernel(const int64_t* __restrict__ table, MfmaArgs a) {
    const int64_t* row = table + (size_t)blockIdx.z * UMOE_DAC_ROW_WORDS;
    const MfmaWin win = DAC_ROW_WIN(row);
    const int tile = (int)(blockIdx.x / (unsigned)a.stride), ph = (int)(blockIdx.x % (unsigned)a.stride);
    if (win.n <= 0 || (long long)tile * TN >= convt_q_count(win.t_begin, win.n, a.pad, a.stride)) return;
    a.x = reinterpret_cast<const float*>(row[0]);
    a.y = reinterpret_cast<float*>(row[2]);
    a.L = (int)row[11];
    convt1d_tile<true>(a, win, convt_q_first(win.t_begin, a.pad, a.stride) + (long long)tile * TN, ph, (int)blockIdx.y * TM, 0);
}
#undef DAC_ROW_WIN

// What these kernels cannot launch (their LDS use is fixed, so no geometry is too large to stage): a reduction length or a grid
// that does not fit the launch's integers.
int mfma_limits(const char* who, int B, int Cin, int Cout, int taps, long long x_tiles) {
    UMOE_REQUIRE((long long)Cin * taps <= 0x7fffffffLL, "%s: reduction length %lld does not fit an int", who, (long long)Cin * taps);
    UMOE_REQUIRE(ceil_div(Cout, TM) <= 65535 && B <= 65535 && x_tiles <= 0x7fffffffLL, "%s: grid (%lld, %d, %d) is beyond the launch limits", who,
                 x_tiles, ceil_div(Cout, TM), B);
    return 0;
}

long long convt_x_tiles(long long nq, int stride) { return (nq + TN - 1) / TN * stride; }
}  // namespace

extern "C" int umoe_dac_conv1d_mfma(const float* x, const float* wt, const float* bias, const float* snake_alpha, const float* resid, int B,
                                    int Cin, int L, int Cout, int K, int stride, int dilation, int pad, int act, float* y, int* Lout_out,
                                    umoe_stream_t stream) {
    const char* who = "umoe_dac_conv1d_mfma";
    UMOE_REQUIRE(x && wt && B > 0 && Cin > 0 && Cout > 0 && K > 0 && stride > 0 && dilation > 0 && pad >= 0 && L > 0, "%s: bad argument", who);
    const int Lout = (int)dac_conv_out_len(L, K, stride, dilation, pad);
    UMOE_REQUIRE(Lout > 0, "%s: empty output (L=%d K=%d stride=%d dilation=%d pad=%d)", who, L, K, stride, dilation, pad);
    UMOE_REQUIRE(y, "%s: bad argument", who);
    if (int rc = mfma_limits(who, B, Cin, Cout, K, ceil_div(Lout, TN))) return rc;
    if (Lout_out) *Lout_out = Lout;
    dim3 grid((unsigned)ceil_div(Lout, TN), (unsigned)ceil_div(Cout, TM), (unsigned)B);
    const MfmaArgs a{x, wt, bias, snake_alpha, resid, y, Cin, L, Cout, K, stride, dilation, pad, Lout, act};
    dac_conv1d_mfma_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>(a, MfmaWin{});
    UMOE_LAUNCH_CHECK();
    return 0;
}

extern "C" int umoe_dac_conv_transpose1d_mfma(const float* x, const float* wt, const float* bias, const float* snake_alpha, int B, int Cin,
                                              int L, int Cout, int K, int stride, int pad, int out_pad, float* y, int* Lout_out,
                                              umoe_stream_t stream) {
    const char* who = "umoe_dac_conv_transpose1d_mfma";
    UMOE_REQUIRE(x && wt && y && B > 0 && Cin > 0 && Cout > 0 && K > 0 && stride > 0 && pad >= 0 && out_pad >= 0 && L > 0, "%s: bad argument", who);
    const long long Lout = ((long long)L - 1) * stride - 2LL * pad + K + out_pad;
    UMOE_REQUIRE(Lout > 0 && Lout <= 0x7fffffffLL, "%s: empty output", who);
    const long long xt = convt_x_tiles(convt_q_count(0, (int)Lout, pad, stride), stride);
    if (int rc = mfma_limits(who, B, Cin, Cout, (K + stride - 1) / stride, xt)) return rc;
    if (Lout_out) *Lout_out = (int)Lout;
    dim3 grid((unsigned)xt, (unsigned)ceil_div(Cout, TM), (unsigned)B);
    const MfmaArgs a{x, wt, bias, snake_alpha, nullptr, y, Cin, L, Cout, K, stride, 1, pad, (int)Lout, 0};
    dac_convt1d_mfma_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>(a, MfmaWin{});
    UMOE_LAUNCH_CHECK();
    return 0;
}

extern "C" int umoe_dac_conv1d_win_mfma(const float* x, int x_off, int Lx, const float* wt, const float* bias, const float* snake_alpha,
                                        const float* resid, int r_off, int Lr, int B, int Cin, int L, int Cout, int K, int stride,
                                        int dilation, int pad, int act, int t_begin, int n, float* y, int y_off, int Ly, umoe_stream_t stream) {
    const char* who = "umoe_dac_conv1d_win_mfma";
    UMOE_REQUIRE(x && wt && y && B > 0 && Cin > 0 && Cout > 0 && K > 0 && stride > 0 && dilation > 0 && pad >= 0 && L > 0 && Lx > 0 && Ly > 0 &&
                 t_begin >= 0 && n > 0, "%s: bad argument", who);
    if (int rc = dac_conv1d_win_check(who, x_off, Lx, resid != nullptr, r_off, Lr, L, K, stride, dilation, pad, t_begin, n, y_off, Ly)) return rc;
    if (int rc = mfma_limits(who, B, Cin, Cout, K, ceil_div(n, TN))) return rc;
    dim3 grid((unsigned)ceil_div(n, TN), (unsigned)ceil_div(Cout, TM), (unsigned)B);
    const MfmaArgs a{x, wt, bias, snake_alpha, resid, y, Cin, L, Cout, K, stride, dilation, pad, (int)dac_conv_out_len(L, K, stride, dilation, pad), act};
    dac_conv1d_mfma_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>(a, MfmaWin{x_off, Lx, r_off, Lr, y_off, Ly, t_begin, n});
    UMOE_LAUNCH_CHECK();
    return 0;
}

extern "C" int umoe_dac_conv_transpose1d_win_mfma(const float* x, int x_off, int Lx, const float* wt, const float* bias, const float* snake_alpha,
                                                  int B, int Cin, int L, int Cout, int K, int stride, int pad, int out_pad, int t_begin, int n,
                                                  float* y, int y_off, int Ly, umoe_stream_t stream) {
    const char* who = "umoe_dac_conv_transpose1d_win_mfma";
    UMOE_REQUIRE(x && wt && y && B > 0 && Cin > 0 && Cout > 0 && K > 0 && stride > 0 && pad >= 0 && out_pad >= 0 && L > 0 && Lx > 0 && Ly > 0 &&
                 t_begin >= 0 && n > 0, "%s: bad argument", who);
    if (int rc = dac_convt1d_win_check(who, x_off, Lx, L, K, stride, pad, out_pad, t_begin, n, y_off, Ly)) return rc;
    const long long xt = convt_x_tiles(convt_q_count(t_begin, n, pad, stride), stride);
    if (int rc = mfma_limits(who, B, Cin, Cout, (K + stride - 1) / stride, xt)) return rc;
    dim3 grid((unsigned)xt, (unsigned)ceil_div(Cout, TM), (unsigned)B);
    const MfmaArgs a{x, wt, bias, snake_alpha, nullptr, y, Cin, L, Cout, K, stride, 1, pad, 0, 0};
    dac_convt1d_mfma_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>(a, MfmaWin{x_off, Lx, 0, 0, y_off, Ly, t_begin, n});
    UMOE_LAUNCH_CHECK();
    return 0;
}

extern "C" int umoe_dac_conv1d_win_rows_mfma(const int64_t* host, const int64_t* table, int rows, int max_n, const float* wt, const float* bias,
                                             const float* snake_alpha, int Cin, int Cout, int K, int stride, int dilation, int pad, int act,
                                             umoe_stream_t stream) {
    const char* who = "umoe_dac_conv1d_win_rows_mfma";
    UMOE_REQUIRE(wt && Cin > 0 && Cout > 0 && K > 0 && stride > 0 && dilation > 0 && pad >= 0, "%s: bad argument", who);
    if (int rc = dac_rows_common(who, host, table, rows, max_n)) return rc;
    for (int r = 0; r < rows; ++r) {
        const int64_t* d = host + (size_t)r * UMOE_DAC_ROW_WORDS;
        if (d[10] == 0) continue;
        if (int rc = dac_conv1d_win_check(who, (int)d[3], (int)d[4], d[1] != 0, (int)d[5], (int)d[6], (int)d[11], K, stride, dilation, pad, (int)d[9],
                                          (int)d[10], (int)d[7], (int)d[8]))
            return rc;
    }
    if (int rc = mfma_limits(who, rows, Cin, Cout, K, ceil_div(max_n, TN))) return rc;
    if (max_n == 0) return 0;
    dim3 grid((unsigned)ceil_div(max_n, TN), (unsigned)ceil_div(Cout, TM), (unsigned)rows);
    const MfmaArgs a{nullptr, wt, bias, snake_alpha, nullptr, nullptr, Cin, 0, Cout, K, stride, dilation, pad, 0, act};
    dac_conv1d_rows_mfma_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(table, a);
    UMOE_LAUNCH_CHECK();
    return 0;
}

extern "C" int umoe_dac_conv_transpose1d_win_rows_mfma(const int64_t* host, const int64_t* table, int rows, int max_n, const float* wt,
                                                       const float* bias, const float* snake_alpha, int Cin, int Cout, int K, int stride,
                                                       int pad, int out_pad, umoe_stream_t stream) {
    const char* who = "umoe_dac_conv_transpose1d_win_rows_mfma";
    UMOE_REQUIRE(wt && Cin > 0 && Cout > 0 && K > 0 && stride > 0 && pad >= 0 && out_pad >= 0, "%s: bad argument", who);
    if (int rc = dac_rows_common(who, host, table, rows, max_n)) return rc;
    long long nq = 0;
    for (int r = 0; r < rows; ++r) {
        const int64_t* d = host + (size_t)r * UMOE_DAC_ROW_WORDS;
        if (d[10] == 0) continue;
        if (int rc = dac_convt1d_win_check(who, (int)d[3], (int)d[4], (int)d[11], K, stride, pad, out_pad, (int)d[9], (int)d[10], (int)d[7], (int)d[8]))
            return rc;
        const long long q = convt_q_count((int)d[9], (int)d[10], pad, stride);
        nq = q > nq ? q : nq;
    }
    const long long xt = convt_x_tiles(nq, stride);
    if (int rc = mfma_limits(who, rows, Cin, Cout, (K + stride - 1) / stride, xt)) return rc;
    if (max_n == 0 || nq == 0) return 0;
    dim3 grid((unsigned)xt, (unsigned)ceil_div(Cout, TM), (unsigned)rows);
    const MfmaArgs a{nullptr, wt, bias, snake_alpha, nullptr, nullptr, Cin, 0, Cout, K, stride, 1, pad, 0, 0};
    dac_convt1d_rows_mfma_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(table, a);
    UMOE_LAUNCH_CHECK();
    return 0;
}
