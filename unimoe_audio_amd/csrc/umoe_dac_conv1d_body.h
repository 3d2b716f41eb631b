// The body of the conv1d kernels of umoe_dac.hip, included inside each of them behind the kernel's own first lines (sm / xl / wl, t0,
// co0, b, tid).  Names it expects in scope: WIN, x, w, bias, alpha, resid, Cin, L, Cout, K, stride, dil, pad, Lout, act, XW, y, win.
// An include and not a device function: the full-sequence and windowed kernels keep the token stream they always had, so their
// instruction text does not change when a third kernel shares the body.
    const int tx = tid & 15, ty = tid >> 4;
    const int Lx = WIN ? win.Lx : L, x_off = WIN ? win.x_off : 0;
    const float* xb = x + (size_t)b * Cin * Lx;
    const int in0 = t0 * stride - pad;    // input position of LDS column 0
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int c0 = 0; c0 < Cin; c0 += CC) {
        for (int i = tid; i < CC * XW; i += 256) {
            const int c = i / XW, p = i % XW, ci = c0 + c, pos = in0 + p;
            float v = 0.f;
            // (WIN: a position outside the buffer feeds only outputs past the window; the entry point checks the window's own)
            if (ci < Cin && pos >= 0 && pos < L && (!WIN || (pos >= x_off && pos < x_off + Lx))) {
                v = xb[(size_t)ci * Lx + (pos - x_off)];
                if (alpha) v = snake(v, alpha[ci]);
            }
            xl[i] = v;
        }
        for (int i = tid; i < CC * K * TO; i += 256) {
            const int o = i % TO, k = (i / TO) % K, c = i / (TO * K), ci = c0 + c, co = co0 + o;
            wl[i] = (ci < Cin && co < Cout) ? w[((size_t)co * Cin + ci) * K + k] : 0.f;
        }
        __syncthreads();
        for (int c = 0; c < CC; ++c)
            for (int k = 0; k < K; ++k) {
                const float4 wv = *reinterpret_cast<const float4*>(wl + (c * K + k) * TO + ty * 4);
                const float* xr = xl + c * XW + k * dil;
                float xv[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) xv[j] = xr[(tx + 16 * j) * stride];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[0][j] += wv.x * xv[j];
                    acc[1][j] += wv.y * xv[j];
                    acc[2][j] += wv.z * xv[j];
                    acc[3][j] += wv.w * xv[j];
                }
            }
        __syncthreads();
    }
    const int t_end = WIN ? win.t_begin + win.n : Lout;
    const int Ly = WIN ? win.Ly : Lout, y_off = WIN ? win.y_off : 0;
    const int Lr = WIN ? win.Lr : Lout, r_off = WIN ? win.r_off : 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int co = co0 + ty * 4 + i;
        if (co >= Cout) continue;
        const float bv = bias ? bias[co] : 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = t0 + tx + 16 * j;
            if (t >= t_end) continue;
            float v = acc[i][j] + bv;
            if (act == 1) v = tanhf(v);
            if (resid) v += resid[((size_t)b * Cout + co) * Lr + (t - r_off)];
            y[((size_t)b * Cout + co) * Ly + (t - y_off)] = v;
        }
    }
