// The body of the transposed-conv kernels of umoe_dac.hip (see umoe_dac_conv1d_body.h).  Names it expects in scope: WIN, x, w, bias,
// alpha, Cin, L, Cout, K, stride, pad, Lout, XW, y, win, and the kernel's own first lines (sm / xl / wl, t0, co0, b, tid).
    const int tx = tid & 15, ty = tid >> 4;
    const int Lx = WIN ? win.Lx : L, x_off = WIN ? win.x_off : 0;
    const float* xb = x + (size_t)b * Cin * Lx;
    const int M = (K + stride - 1) / stride;                 // taps per output position
    const int ibase = (t0 + pad) / stride - (M - 1);         // input index of LDS column 0
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int c0 = 0; c0 < Cin; c0 += CC) {
        for (int i = tid; i < CC * XW; i += 256) {
            const int c = i / XW, p = i % XW, ci = c0 + c, pos = ibase + p;
            float v = 0.f;
            if (ci < Cin && pos >= 0 && pos < L && (!WIN || (pos >= x_off && pos < x_off + Lx))) {
                v = xb[(size_t)ci * Lx + (pos - x_off)];
                if (alpha) v = snake(v, alpha[ci]);
            }
            xl[i] = v;
        }
        for (int i = tid; i < CC * K * TO; i += 256) {
            const int o = i % TO, k = (i / TO) % K, c = i / (TO * K), ci = c0 + c, co = co0 + o;
            wl[i] = (ci < Cin && co < Cout) ? w[((size_t)ci * Cout + co) * K + k] : 0.f;
        }
        __syncthreads();
        for (int c = 0; c < CC; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int tp = t0 + tx + 16 * j + pad;
                const int k0 = tp % stride, i0 = tp / stride - ibase;
                for (int m = 0; m < M; ++m) {
                    const int k = k0 + m * stride;
                    if (k >= K) break;
                    const float xv = xl[c * XW + i0 - m];
                    const float4 wv = *reinterpret_cast<const float4*>(wl + (c * K + k) * TO + ty * 4);
                    acc[0][j] += wv.x * xv;
                    acc[1][j] += wv.y * xv;
                    acc[2][j] += wv.z * xv;
                    acc[3][j] += wv.w * xv;
                }
            }
        __syncthreads();
    }
    const int t_end = WIN ? win.t_begin + win.n : Lout;
    const int Ly = WIN ? win.Ly : Lout, y_off = WIN ? win.y_off : 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int co = co0 + ty * 4 + i;
        if (co >= Cout) continue;
        const float bv = bias ? bias[co] : 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = t0 + tx + 16 * j;
            if (t < t_end) y[((size_t)b * Cout + co) * Ly + (t - y_off)] = acc[i][j] + bv;
        }
    }
