// DAC waveform <-> latent conv stacks (reference utils/UniMoE_Audio_utils.py:112-113,123-124 call the third-party
// descript-audio-codec 1.0.0 `DAC.encode` / `DAC.decode`; the package is absent offline, so the layers are restated from the
// published architecture -- PARITY UNPINNED -- with every dimension a load-time parameter):
//   Snake1d(x) = x + sin(alpha x)^2 / (alpha + 1e-9)  ->  (weight-normalised) Conv1d / ConvTranspose1d, residual units x + y,
//   tanh on the last decoder layer.  fp32 like the reference model.
// One direct kernel per conv flavour, the Snake of the PRECEDING layer fused into the input load (the DAC graph is always
// Snake -> conv), bias, residual add and tanh fused into the store.  Output tile 64 channels x 64 positions per 256-thread
// workgroup, 4 x 4 outputs per thread, input channels in chunks of 8 staged through LDS together with their weight slices.
// Roofline: fp32 VALU / LDS; ~450 GFLOP per 10 s of audio, once per request (not on the per-step path).
// Windowed twins (umoe_dac_conv1d_win / umoe_dac_conv_transpose1d_win, the streaming decoder of dac.py): the same kernel bodies
// instantiated with WIN = true compute output positions [t_begin, t_begin + n) of a sequence of true length L from buffers that
// hold only a window of the input / residual / output.  Only the addressing differs: every output goes through the same loads
// (zero outside [0, L)), the same accumulation order (channel chunk, channel, tap) and the same epilogue, so it depends on the
// input values alone and never on the window or the tile start.
// Per-row twins (umoe_dac_conv1d_win_rows / umoe_dac_conv_transpose1d_win_rows, the per-row streaming decoder of dac.py): the WIN
// bodies a third time, each row of the launch on a window of its own read from a table (umoe.h "Per-row window tables").  The bodies
// are include files (umoe_dac_conv1d_body.h, umoe_dac_convt1d_body.h) so that every kernel compiles the same token stream.
// snake() lives in umoe_dac_snake.h and the host-side geometry / window checks in umoe_dac_host.h, both shared with umoe_dac_mfma.hip.
#include "umoe_common.h"
#include "umoe_dac_host.h"
#include "umoe_dac_snake.h"

namespace {
constexpr int TO = 64, TP = 64, CC = 8;

// Window of a WIN instantiation (absolute positions): x holds input positions [x_off, x_off + Lx), resid [r_off, r_off + Lr),
// y [y_off, y_off + Ly); outputs [t_begin, t_begin + n) are computed.  Ignored by the full-sequence instantiation.
struct DacWin {
    int x_off, Lx, r_off, Lr, y_off, Ly, t_begin, n;
};

// y[b][co][t] = act( bias[co] + sum_ci sum_k snake?(x[b][ci][t*stride - pad + k*dil]) * w[co][ci][k] ) (+ resid[b][co][t])
template <bool WIN>
__global__ __launch_bounds__(256) void dac_conv1d_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                         const float* __restrict__ alpha, const float* __restrict__ resid, int Cin, int L,
                                                         int Cout, int K, int stride, int dil, int pad, int Lout, int act, int XW,
                                                         float* __restrict__ y, DacWin win) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* xl = sm;                       // [CC][XW]
    float* wl = sm + CC * XW;             // [CC][K][TO]
    const int t0 = (WIN ? win.t_begin : 0) + blockIdx.x * TP, co0 = blockIdx.y * TO, b = blockIdx.z, tid = threadIdx.x;
#include "umoe_dac_conv1d_body.h"
}

// ConvTranspose1d, gather form: y[b][co][t] = bias[co] + sum_ci sum_{k == (t + pad) mod stride, k < K} snake?(x[b][ci][(t + pad - k) / stride]) * w[ci][co][k]
template <bool WIN>
__global__ __launch_bounds__(256) void dac_convt1d_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                          const float* __restrict__ alpha, int Cin, int L, int Cout, int K, int stride, int pad,
                                                          int Lout, int XW, float* __restrict__ y, DacWin win) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* xl = sm;                       // [CC][XW]
    float* wl = sm + CC * XW;             // [CC][K][TO]
    const int t0 = (WIN ? win.t_begin : 0) + blockIdx.x * TP, co0 = blockIdx.y * TO, b = blockIdx.z, tid = threadIdx.x;
#include "umoe_dac_convt1d_body.h"
}

// ---- the WIN bodies once more, every row of the launch (blockIdx.z) on a window of its own: the row's plane pointers, its DacWin
// and its L come from row blockIdx.z of a table (umoe.h "Per-row window tables").  Every word is read at an address that depends on
// blockIdx.z alone, so the loads are scalar and the values wave-uniform.  A workgroup whose tile starts at or past its row's n
// (n = 0: the row is idle in this launch) leaves before the first barrier; all threads of a workgroup take the same way.
#define DAC_ROW_WIN(r) DacWin{(int)(r)[3], (int)(r)[4], (int)(r)[5], (int)(r)[6], (int)(r)[7], (int)(r)[8], (int)(r)[9], (int)(r)[10]}

__global__ __launch_bounds__(256) void dac_conv1d_rows_kernel(const int64_t* __restrict__ table, const float* __restrict__ w,
                                                              const float* __restrict__ bias, const float* __restrict__ alpha, int Cin, int Cout,
                                                              int K, int stride, int dil, int pad, int act, int XW) {
    const int64_t* row = table + (size_t)blockIdx.z * UMOE_DAC_ROW_WORDS;
    const DacWin win = DAC_ROW_WIN(row);
    if ((int)(blockIdx.x * TP) >= win.n) return;
    constexpr bool WIN = true;
    const float* __restrict__ x = reinterpret_cast<const float*>(row[0]);
    const float* __restrict__ resid = reinterpret_cast<const float*>(row[1]);
    float* __restrict__ y = reinterpret_cast<float*>(row[2]);
    const int L = (int)row[11], Lout = 0;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* xl = sm;                       // [CC][XW]
    float* wl = sm + CC * XW;             // [CC][K][TO]
    const int t0 = win.t_begin + blockIdx.x * TP, co0 = blockIdx.y * TO, b = 0, tid = threadIdx.x;      // (b: the planes are the row's own)
#include "umoe_dac_conv1d_body.h"
}

__global__ __launch_bounds__(256) void dac_convt1d_rows_kernel(const int64_t* __restrict__ table, const float* __restrict__ w,
                                                               const float* __restrict__ bias, const float* __restrict__ alpha, int Cin, int Cout,
                                                               int K, int stride, int pad, int XW) {
    const int64_t* row = table + (size_t)blockIdx.z * UMOE_DAC_ROW_WORDS;
    const DacWin win = DAC_ROW_WIN(row);
    if ((int)(blockIdx.x * TP) >= win.n) return;
    constexpr bool WIN = true;
    const float* __restrict__ x = reinterpret_cast<const float*>(row[0]);
    float* __restrict__ y = reinterpret_cast<float*>(row[2]);
    const int L = (int)row[11], Lout = 0;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* xl = sm;                       // [CC][XW]
    float* wl = sm + CC * XW;             // [CC][K][TO]
    const int t0 = win.t_begin + blockIdx.x * TP, co0 = blockIdx.y * TO, b = 0, tid = threadIdx.x;
#include "umoe_dac_convt1d_body.h"
}
#undef DAC_ROW_WIN

// Left context of the per-row decoder's slabs, all rows of a layer in one launch: row r's plane [C][W] moves its columns
// [shift, shift + count) to [0, count) in place.  One workgroup per (16 channels, row); a channel's columns go 256 at a time from the
// left.  A batch is read by all threads before any of it is written (the barrier), and it lands left of everything still to be read
// (shift > 0), so no column is overwritten before it was moved.
__global__ __launch_bounds__(256) void dac_shift_rows_kernel(const int64_t* __restrict__ table, int C) {
    const int64_t* r = table + (size_t)blockIdx.y * UMOE_SHIFT_ROW_WORDS;
    float* plane = reinterpret_cast<float*>(r[0]);
    const int W = (int)r[1], shift = (int)r[2], count = (int)r[3];
    if (count <= 0 || shift <= 0) return;
    for (int c = blockIdx.x * 16; c < min(C, (int)blockIdx.x * 16 + 16); ++c) {
        float* p = plane + (size_t)c * W;
        for (int j0 = 0; j0 < count; j0 += 256) {
            const int j = j0 + threadIdx.x;
            const float v = j < count ? p[j + shift] : 0.f;
            __syncthreads();
            if (j < count) p[j] = v;
        }
    }
}
// polyphase windowed-sinc resampler (torchaudio.transforms.Resample's default algorithm, reference utils.py:101-110): output sample
// j = frame * n + phase reads K = 2 width + o taps of filter `phase` from the zero-padded input at frame * o - width
__global__ __launch_bounds__(256) void dac_resample_kernel(const float* __restrict__ x, const float* __restrict__ kern, int L, int o, int n,
                                                           int width, int K, int Lout, float* __restrict__ y) {
    const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (j >= Lout) return;
    const int fr = j / n, ph = j % n;
    const float* k = kern + (size_t)ph * K;
    const float* xb = x + (size_t)b * L;
    const int p0 = fr * o - width;
    float acc = 0.f;
    for (int t = 0; t < K; ++t) {
        const int p = p0 + t;
        if (p >= 0 && p < L) acc += k[t] * xb[p];
    }
    y[(size_t)b * Lout + j] = acc;
}
}  // namespace

extern "C" int umoe_dac_resample(const float* x, const float* kern, int B, int L, int o, int n, int width, int Lout, float* y,
                                 umoe_stream_t stream) {
    UMOE_REQUIRE(x && kern && y && B > 0 && L > 0 && o > 0 && n > 0 && width >= 0 && Lout > 0, "umoe_dac_resample: bad argument");
    dac_resample_kernel<<<dim3((unsigned)ceil_div(Lout, 256), (unsigned)B), 256, 0, (hipStream_t)stream>>>(x, kern, L, o, n, width, 2 * width + o, Lout, y);
    UMOE_LAUNCH_CHECK();
    return 0;
}

extern "C" int umoe_dac_conv1d(const float* x, const float* w, const float* bias, const float* snake_alpha, const float* resid, int B,
                               int Cin, int L, int Cout, int K, int stride, int dilation, int pad, int act, float* y, int* Lout_out,
                               umoe_stream_t stream) {
    UMOE_REQUIRE(x && w && B > 0 && Cin > 0 && Cout > 0 && K > 0 && stride > 0 && dilation > 0 && pad >= 0 && L > 0,
                 "umoe_dac_conv1d: bad argument");
    const int Lout = (int)dac_conv_out_len(L, K, stride, dilation, pad);
    UMOE_REQUIRE(Lout > 0, "umoe_dac_conv1d: empty output (L=%d K=%d stride=%d dilation=%d pad=%d)", L, K, stride, dilation, pad);
    UMOE_REQUIRE(y, "umoe_dac_conv1d: bad argument");
    if (Lout_out) *Lout_out = Lout;
    const int XW = (TP - 1) * stride + (K - 1) * dilation + 1;
    const size_t lds = ((size_t)CC * XW + (size_t)CC * K * TO) * sizeof(float);
    UMOE_REQUIRE(lds <= 64 * 1024, "umoe_dac_conv1d: tile needs %zu bytes of LDS", lds);
    dim3 grid((unsigned)ceil_div(Lout, TP), (unsigned)ceil_div(Cout, TO), (unsigned)B);
    dac_conv1d_kernel<false><<<grid, 256, lds, (hipStream_t)stream>>>(x, w, bias, snake_alpha, resid, Cin, L, Cout, K, stride, dilation, pad, Lout, act,
                                                                      XW, y, DacWin{});
    UMOE_LAUNCH_CHECK();
    return 0;
}

extern "C" int umoe_dac_conv_transpose1d(const float* x, const float* w, const float* bias, const float* snake_alpha, int B, int Cin, int L,
                                         int Cout, int K, int stride, int pad, int out_pad, float* y, int* Lout_out, umoe_stream_t stream) {
    UMOE_REQUIRE(x && w && y && B > 0 && Cin > 0 && Cout > 0 && K > 0 && stride > 0 && pad >= 0 && out_pad >= 0 && L > 0,
                 "umoe_dac_conv_transpose1d: bad argument");
    const int Lout = (L - 1) * stride - 2 * pad + K + out_pad;
    UMOE_REQUIRE(Lout > 0, "umoe_dac_conv_transpose1d: empty output");
    if (Lout_out) *Lout_out = Lout;
    const int M = (K + stride - 1) / stride;
    const int XW = (TP - 1 + stride - 1) / stride + M + 1;
    const size_t lds = ((size_t)CC * XW + (size_t)CC * K * TO) * sizeof(float);
    UMOE_REQUIRE(lds <= 64 * 1024, "umoe_dac_conv_transpose1d: tile needs %zu bytes of LDS", lds);
    dim3 grid((unsigned)ceil_div(Lout, TP), (unsigned)ceil_div(Cout, TO), (unsigned)B);
    dac_convt1d_kernel<false><<<grid, 256, lds, (hipStream_t)stream>>>(x, w, bias, snake_alpha, Cin, L, Cout, K, stride, pad, Lout, XW, y, DacWin{});
    UMOE_LAUNCH_CHECK();
    return 0;
}

// ---- windowed entry points (streaming decode).  Absolute positions; int64 index arithmetic in the checks so that no window,
// however large its offsets, can make a kernel read or write outside the buffers it was given.
extern "C" int umoe_dac_conv1d_win(const float* x, int x_off, int Lx, const float* w, const float* bias, const float* snake_alpha,
                                   const float* resid, int r_off, int Lr, int B, int Cin, int L, int Cout, int K, int stride,
                                   int dilation, int pad, int act, int t_begin, int n, float* y, int y_off, int Ly, umoe_stream_t stream) {
    UMOE_REQUIRE(x && w && y && B > 0 && Cin > 0 && Cout > 0 && K > 0 && stride > 0 && dilation > 0 && pad >= 0 && L > 0 && Lx > 0 &&
                 Ly > 0 && t_begin >= 0 && n > 0, "umoe_dac_conv1d_win: bad argument");
    if (int rc = dac_conv1d_win_check("umoe_dac_conv1d_win", x_off, Lx, resid != nullptr, r_off, Lr, L, K, stride, dilation, pad, t_begin, n, y_off, Ly))
        return rc;
    const int XW = (TP - 1) * stride + (K - 1) * dilation + 1;
    const size_t lds = ((size_t)CC * XW + (size_t)CC * K * TO) * sizeof(float);
    UMOE_REQUIRE(lds <= 64 * 1024, "umoe_dac_conv1d_win: tile needs %zu bytes of LDS", lds);
    dim3 grid((unsigned)ceil_div(n, TP), (unsigned)ceil_div(Cout, TO), (unsigned)B);
    const DacWin win{x_off, Lx, r_off, Lr, y_off, Ly, t_begin, n};
    dac_conv1d_kernel<true><<<grid, 256, lds, (hipStream_t)stream>>>(x, w, bias, snake_alpha, resid, Cin, L, Cout, K, stride, dilation, pad,
                                                                     (int)dac_conv_out_len(L, K, stride, dilation, pad), act, XW, y, win);
    UMOE_LAUNCH_CHECK();
    return 0;
}

extern "C" int umoe_dac_conv_transpose1d_win(const float* x, int x_off, int Lx, const float* w, const float* bias, const float* snake_alpha,
                                             int B, int Cin, int L, int Cout, int K, int stride, int pad, int out_pad, int t_begin, int n,
                                             float* y, int y_off, int Ly, umoe_stream_t stream) {
    UMOE_REQUIRE(x && w && y && B > 0 && Cin > 0 && Cout > 0 && K > 0 && stride > 0 && pad >= 0 && out_pad >= 0 && L > 0 && Lx > 0 &&
                 Ly > 0 && t_begin >= 0 && n > 0, "umoe_dac_conv_transpose1d_win: bad argument");
    if (int rc = dac_convt1d_win_check("umoe_dac_conv_transpose1d_win", x_off, Lx, L, K, stride, pad, out_pad, t_begin, n, y_off, Ly)) return rc;
    const long long Lout = ((long long)L - 1) * stride - 2 * pad + K + out_pad;
    const int M = (K + stride - 1) / stride;
    const int XW = (TP - 1 + stride - 1) / stride + M + 1;
    const size_t lds = ((size_t)CC * XW + (size_t)CC * K * TO) * sizeof(float);
    UMOE_REQUIRE(lds <= 64 * 1024, "umoe_dac_conv_transpose1d_win: tile needs %zu bytes of LDS", lds);
    dim3 grid((unsigned)ceil_div(n, TP), (unsigned)ceil_div(Cout, TO), (unsigned)B);
    const DacWin win{x_off, Lx, 0, 0, y_off, Ly, t_begin, n};
    dac_convt1d_kernel<true><<<grid, 256, lds, (hipStream_t)stream>>>(x, w, bias, snake_alpha, Cin, L, Cout, K, stride, pad, (int)Lout, XW, y, win);
    UMOE_LAUNCH_CHECK();
    return 0;
}

// ---- one window per row (the per-row streaming decoder of dac.py): `host` is the table the checks read, `table` the device copy the
// kernel reads (the caller uploads the tables of all layers of a read in one copy).  Every row with n > 0 passes the checks of the _win
// entry; a row with n == 0 is idle and only its n is read.  Nothing is enqueued unless every row passes.
extern "C" int umoe_dac_conv1d_win_rows(const int64_t* host, const int64_t* table, int rows, int max_n, const float* w, const float* bias,
                                        const float* snake_alpha, int Cin, int Cout, int K, int stride, int dilation, int pad, int act,
                                        umoe_stream_t stream) {
    const char* who = "umoe_dac_conv1d_win_rows";
    UMOE_REQUIRE(w && Cin > 0 && Cout > 0 && K > 0 && stride > 0 && dilation > 0 && pad >= 0, "%s: bad argument", who);
    if (int rc = dac_rows_common(who, host, table, rows, max_n)) return rc;
    for (int r = 0; r < rows; ++r) {
        const int64_t* d = host + (size_t)r * UMOE_DAC_ROW_WORDS;
        if (d[10] == 0) continue;
        if (int rc = dac_conv1d_win_check(who, (int)d[3], (int)d[4], d[1] != 0, (int)d[5], (int)d[6], (int)d[11], K, stride, dilation, pad, (int)d[9],
                                          (int)d[10], (int)d[7], (int)d[8]))
            return rc;
    }
    if (max_n == 0) return 0;
    const int XW = (TP - 1) * stride + (K - 1) * dilation + 1;
    const size_t lds = ((size_t)CC * XW + (size_t)CC * K * TO) * sizeof(float);
    UMOE_REQUIRE(lds <= 64 * 1024, "%s: tile needs %zu bytes of LDS", who, lds);
    dim3 grid((unsigned)ceil_div(max_n, TP), (unsigned)ceil_div(Cout, TO), (unsigned)rows);
    dac_conv1d_rows_kernel<<<grid, 256, lds, (hipStream_t)stream>>>(table, w, bias, snake_alpha, Cin, Cout, K, stride, dilation, pad, act, XW);
    UMOE_LAUNCH_CHECK();
    return 0;
}

extern "C" int umoe_dac_conv_transpose1d_win_rows(const int64_t* host, const int64_t* table, int rows, int max_n, const float* w,
                                                  const float* bias, const float* snake_alpha, int Cin, int Cout, int K, int stride, int pad,
                                                  int out_pad, umoe_stream_t stream) {
    const char* who = "umoe_dac_conv_transpose1d_win_rows";
    UMOE_REQUIRE(w && Cin > 0 && Cout > 0 && K > 0 && stride > 0 && pad >= 0 && out_pad >= 0, "%s: bad argument", who);
    if (int rc = dac_rows_common(who, host, table, rows, max_n)) return rc;
    for (int r = 0; r < rows; ++r) {
        const int64_t* d = host + (size_t)r * UMOE_DAC_ROW_WORDS;
        if (d[10] == 0) continue;
        if (int rc = dac_convt1d_win_check(who, (int)d[3], (int)d[4], (int)d[11], K, stride, pad, out_pad, (int)d[9], (int)d[10], (int)d[7], (int)d[8]))
            return rc;
    }
    if (max_n == 0) return 0;
    const int M = (K + stride - 1) / stride;
    const int XW = (TP - 1 + stride - 1) / stride + M + 1;
    const size_t lds = ((size_t)CC * XW + (size_t)CC * K * TO) * sizeof(float);
    UMOE_REQUIRE(lds <= 64 * 1024, "%s: tile needs %zu bytes of LDS", who, lds);
    dim3 grid((unsigned)ceil_div(max_n, TP), (unsigned)ceil_div(Cout, TO), (unsigned)rows);
    dac_convt1d_rows_kernel<<<grid, 256, lds, (hipStream_t)stream>>>(table, w, bias, snake_alpha, Cin, Cout, K, stride, pad, XW);
    UMOE_LAUNCH_CHECK();
    return 0;
}

// table rows of UMOE_SHIFT_ROW_WORDS words {plane, W, shift, count}: columns [shift, shift + count) of each row's [C][W] plane move to
// [0, count); count == 0 or shift == 0: the row is left alone
extern "C" int umoe_dac_shift_rows(const int64_t* host, const int64_t* table, int rows, int C, umoe_stream_t stream) {
    const char* who = "umoe_dac_shift_rows";
    UMOE_REQUIRE(host && table && rows > 0 && rows <= 65535 && C > 0, "%s: bad argument", who);
    UMOE_REQUIRE(((size_t)table & 7) == 0, "%s: the device table must be 8-byte aligned", who);
    bool any = false;
    for (int r = 0; r < rows; ++r) {
        const int64_t* d = host + (size_t)r * UMOE_SHIFT_ROW_WORDS;
        UMOE_REQUIRE(dac_word_is_int(d[1]) && dac_word_is_int(d[2]) && dac_word_is_int(d[3]), "%s: row %d has a word that is not a non-negative int", who, r);
        if (d[3] == 0 || d[2] == 0) continue;
        UMOE_REQUIRE(d[0], "%s: row %d has a null plane", who, r);
        UMOE_REQUIRE(d[2] + d[3] <= d[1], "%s: row %d moves columns [%lld, %lld) of a plane %lld wide", who, r, (long long)d[2],
                     (long long)(d[2] + d[3]), (long long)d[1]);
        any = true;
    }
    if (!any) return 0;
    dac_shift_rows_kernel<<<dim3((unsigned)ceil_div(C, 16), (unsigned)rows), 256, 0, (hipStream_t)stream>>>(table, C);
    UMOE_LAUNCH_CHECK();
    return 0;
}
