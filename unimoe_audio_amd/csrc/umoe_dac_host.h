// Host-side geometry and window checks of the DAC convolution entry points, shared by the direct kernels (umoe_dac.hip) and the MFMA
// kernels (umoe_dac_mfma.hip): both families take the same windows and the same per-row tables (umoe.h "Per-row window tables") and
// refuse the same arguments.  Host code only; int64 index arithmetic so that no window, however large its offsets, can make a kernel
// read or write outside the buffers it was given.
#pragma once
#include "umoe_common.h"

namespace {
// floor((L + 2 pad - dilation (K - 1) - 1) / stride) + 1, and 0 where the receptive field is wider than the padded input: C division
// truncates toward zero, which turned a numerator in (-stride, 0) into one output position that does not exist
[[maybe_unused]] long long dac_conv_out_len(int L, int K, int stride, int dilation, int pad) {
    const long long num = (long long)L + 2LL * pad - (long long)dilation * (K - 1) - 1;
    return num < 0 ? 0 : num / stride + 1;
}

// [lo, hi] of the input positions inside [0, L) that outputs [t0, t1) read; false when they read none
[[maybe_unused]] bool dac_needed(long long lo, long long hi, int L, long long* a, long long* b) {
    *a = lo < 0 ? 0 : lo;
    *b = hi > (long long)L - 1 ? (long long)L - 1 : hi;
    return *a <= *b;
}

// the checks of one window, shared by the _win entries (one window for all planes) and the _rows entries (one per row)
[[maybe_unused]] int dac_conv1d_win_check(const char* who, int x_off, int Lx, bool has_resid, int r_off, int Lr, int L, int K, int stride, int dilation,
                                          int pad, int t_begin, int n, int y_off, int Ly) {
    UMOE_REQUIRE(L > 0 && Lx > 0 && Ly > 0 && t_begin >= 0 && n > 0, "%s: bad argument", who);
    const long long Lout = dac_conv_out_len(L, K, stride, dilation, pad);
    UMOE_REQUIRE(Lout > 0, "%s: empty output (L=%d K=%d stride=%d dilation=%d pad=%d)", who, L, K, stride, dilation, pad);
    UMOE_REQUIRE((long long)t_begin + n <= Lout, "%s: outputs [%d, %d) past the sequence's %lld", who, t_begin, t_begin + n, Lout);
    long long a, b;
    if (dac_needed((long long)t_begin * stride - pad, (long long)(t_begin + n - 1) * stride - pad + (long long)(K - 1) * dilation, L, &a, &b))
        UMOE_REQUIRE(a >= x_off && b < (long long)x_off + Lx, "%s: outputs [%d, %d) read input [%lld, %lld], the buffer holds [%d, %d)", who,
                     t_begin, t_begin + n, a, b, x_off, x_off + Lx);
    UMOE_REQUIRE(t_begin >= y_off && (long long)t_begin + n <= (long long)y_off + Ly, "%s: output buffer [%d, %d) misses [%d, %d)", who, y_off,
                 y_off + Ly, t_begin, t_begin + n);
    if (has_resid)
        UMOE_REQUIRE(Lr > 0 && t_begin >= r_off && (long long)t_begin + n <= (long long)r_off + Lr, "%s: residual buffer [%d, %d) misses [%d, %d)",
                     who, r_off, r_off + Lr, t_begin, t_begin + n);
    return 0;
}

[[maybe_unused]] int dac_convt1d_win_check(const char* who, int x_off, int Lx, int L, int K, int stride, int pad, int out_pad, int t_begin, int n,
                                           int y_off, int Ly) {
    UMOE_REQUIRE(L > 0 && Lx > 0 && Ly > 0 && t_begin >= 0 && n > 0, "%s: bad argument", who);
    const long long Lout = ((long long)L - 1) * stride - 2 * pad + K + out_pad;
    UMOE_REQUIRE((long long)t_begin + n <= Lout, "%s: outputs [%d, %d) past the sequence's %lld", who, t_begin, t_begin + n, Lout);
    // output t reads inputs i with i * stride + k == t + pad, 0 <= k < K
    const long long lo = ((long long)t_begin + pad - K + stride + (long long)stride * K) / stride - K;   // ceil((t_begin + pad - K + 1) / stride)
    long long a, b;
    if (dac_needed(lo, ((long long)t_begin + n - 1 + pad) / stride, L, &a, &b))
        UMOE_REQUIRE(a >= x_off && b < (long long)x_off + Lx, "%s: outputs [%d, %d) read input [%lld, %lld], the buffer holds [%d, %d)", who,
                     t_begin, t_begin + n, a, b, x_off, x_off + Lx);
    UMOE_REQUIRE(t_begin >= y_off && (long long)t_begin + n <= (long long)y_off + Ly, "%s: output buffer [%d, %d) misses [%d, %d)", who, y_off,
                 y_off + Ly, t_begin, t_begin + n);
    return 0;
}

// a table word that must be an int (offsets, lengths, positions)
[[maybe_unused]] bool dac_word_is_int(int64_t v) { return v >= 0 && v <= 0x7fffffffLL; }

// ---- one window per row (the per-row streaming decoder of dac.py): `host` is the table the checks read, `table` the device copy the
// kernel reads (the caller uploads the tables of all layers of a read in one copy).  Every row with n > 0 passes the checks of the _win
// entry; a row with n == 0 is idle and only its n is read.  Nothing is enqueued unless every row passes.
[[maybe_unused]] int dac_rows_common(const char* who, const int64_t* host, const int64_t* table, int rows, int max_n) {
    UMOE_REQUIRE(host && table && rows > 0 && rows <= 65535 && max_n >= 0, "%s: bad argument", who);
    UMOE_REQUIRE(((size_t)table & 7) == 0, "%s: the device table must be 8-byte aligned", who);
    for (int r = 0; r < rows; ++r) {
        const int64_t* d = host + (size_t)r * UMOE_DAC_ROW_WORDS;
        UMOE_REQUIRE(d[10] >= 0 && d[10] <= max_n, "%s: row %d has n = %lld, max_n is %d", who, r, (long long)d[10], max_n);
        if (d[10] == 0) continue;
        UMOE_REQUIRE(d[0] && d[2], "%s: row %d has a null plane", who, r);
        for (int k = 3; k < UMOE_DAC_ROW_WORDS; ++k)
            UMOE_REQUIRE(dac_word_is_int(d[k]), "%s: row %d, word %d (%lld) is not a non-negative int", who, r, k, (long long)d[k]);
    }
    return 0;
}
}  // namespace
