// Optimizer step (include/umoe.h "optimizer step"): AdamW on fp32 master weights of bf16 parameters behind a global-norm clip, every
// tensor of every parameter group in one chunked launch per stage.
//   optim_sqsum_kernel    per-chunk sum of squared gradients, fixed order, no atomics
//   optim_scalars_kernel  one workgroup: fp64 sum of the partials -> norm, clip, bias corrections, skip; advances the counters
//   optim_adamw_kernel    the update: 28 bytes per bf16 parameter (master, m, v read and written, gradient read, parameter written)
// A workgroup owns a chunk at a time and strides over the chunk table.  Within a chunk the streams move as 16-byte vectors, eight
// elements per thread and iteration; a tensor whose streams reach 16-byte alignment together after `head` elements (a view at an odd
// element offset) takes those and the tail one element per thread; streams that never align together take the chunk scalar.
#include <math.h>

#include "umoe_common.h"

#define OPT_THREADS 256
#define OPT_DEFAULT_GRID 2048      // cdna_hip_programming.md Guideline 11: cap a memory-bound grid at ~256 CU x 8 and stride the rest

static_assert(sizeof(umoe_optim_fold_tensor) == 24, "umoe.h record layout");
static_assert(sizeof(umoe_optim_tensor) == 56 && sizeof(umoe_optim_chunk) == 16 && sizeof(umoe_optim_record) == 144, "umoe.h record layout");

struct optim_group_k { float lr, b1, omb1, b2, omb2, eps, wd, bc1, bc2; };
struct optim_kargs {
    optim_group_k g[UMOE_OPTIM_MAX_GROUPS];
    long long t_host;     // >= 0: no record; bc1 / bc2 above, clip 1, and counters[0] = t_host + 1
};

// what one chunk is: the tensor's record, the run [first, first + len) and how its streams align
struct chunk_view {
    umoe_optim_tensor t;
    long first;
    int len;      // 0: nothing to do (left-out tensor or a record out of bounds)
    int head;     // scalar elements in front of the vectors; len = all scalar
};

__device__ __forceinline__ int head_of(const void* p, long first, int esize) {      // elements until 16-byte alignment, < 16 / esize
    const uintptr_t a = (uintptr_t)p + (uintptr_t)first * esize;
    return (int)(((16u - (unsigned)(a & 15u)) & 15u) / esize);
}
__device__ __forceinline__ bool aligned_after(const void* p, long first, int head, int esize) {
    return (((uintptr_t)p + (uintptr_t)(first + head) * esize) & 15u) == 0;
}

// with_state: the update's view (p, master, m, v must co-align with g); else stage 1's (g alone)
__device__ __forceinline__ chunk_view chunk_open(const umoe_optim_tensor* tensors, int n_tensors, const umoe_optim_chunk* chunks, long c,
                                                 int chunk_elems, bool with_state) {
    chunk_view cv;
    cv.t = umoe_optim_tensor{};
    cv.len = 0;
    cv.head = 0;
    cv.first = 0;
    const long ti = chunks[c].tensor, first = chunks[c].first;
    if (ti < 0 || ti >= n_tensors) return cv;
    cv.t = tensors[ti];
    if (!cv.t.g || first < 0 || first >= cv.t.n) return cv;
    cv.first = first;
    const long left = cv.t.n - first;
    cv.len = (int)(left < chunk_elems ? left : chunk_elems);
    // p_fp32 is a flag word: bit 0 the parameter is fp32 (its own master), bit 1 the gradient is fp32 (a main gradient of a bf16 parameter)
    const int es = (cv.t.p_fp32 & UMOE_OPTIM_P_FP32) ? 4 : 2;
    const int eg = (cv.t.p_fp32 & (UMOE_OPTIM_P_FP32 | UMOE_OPTIM_G_FP32)) ? 4 : 2;
    // the head is the parameter's where the parameter moves too (its elements are the widest apart in bytes per 16: a bf16 parameter
    // needs up to 7, which its fp32 streams then share); the same number as the gradient's whenever the two have one type and co-align
    int head = with_state ? head_of(cv.t.p, first, es) : head_of(cv.t.g, first, eg);
    bool ok = (((uintptr_t)cv.t.g) & (eg - 1)) == 0;
    if (with_state) {
        ok = ok && aligned_after(cv.t.g, first, head, eg) && aligned_after(cv.t.m, first, head, 4) && aligned_after(cv.t.v, first, head, 4);
        if (!(cv.t.p_fp32 & UMOE_OPTIM_P_FP32)) ok = ok && aligned_after(cv.t.master, first, head, 4);
    }
    cv.head = ok ? (head < cv.len ? head : cv.len) : cv.len;
    return cv;
}

// The tensors' pointers come out of a table in memory, so the compiler knows no address space for them and would emit flat
// instructions; they are global memory by contract, and the casts below say so (global_load / global_store).
#define OPT_GLOBAL __attribute__((address_space(1)))
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;      // plain vector types: HIP's float4 / uint4 classes copy through generic references
typedef OPT_GLOBAL const f32x4_t* gc_f4;
typedef OPT_GLOBAL f32x4_t* g_f4;
typedef OPT_GLOBAL const u32x4_t* gc_u4;
typedef OPT_GLOBAL u32x4_t* g_u4;
typedef OPT_GLOBAL const float* gc_f1;
typedef OPT_GLOBAL float* g_f1;
typedef OPT_GLOBAL const uint16_t* gc_h1;
typedef OPT_GLOBAL uint16_t* g_h1;

__device__ __forceinline__ void load8(const void* base, long i, bool f32, float* x) {      // 16-byte aligned at element i
    if (f32) {
        const f32x4_t a = *(gc_f4)((const float*)base + i), b = *(gc_f4)((const float*)base + i + 4);
        x[0] = a[0]; x[1] = a[1]; x[2] = a[2]; x[3] = a[3]; x[4] = b[0]; x[5] = b[1]; x[6] = b[2]; x[7] = b[3];
    } else {
        const u32x4_t r = *(gc_u4)((const uint16_t*)base + i);
        unpack8(make_uint4(r[0], r[1], r[2], r[3]), x);
    }
}
__device__ __forceinline__ void store8f(float* base, long i, const float* x) {
    *(g_f4)(base + i) = f32x4_t{x[0], x[1], x[2], x[3]};
    *(g_f4)(base + i + 4) = f32x4_t{x[4], x[5], x[6], x[7]};
}
__device__ __forceinline__ float load1(const void* base, long i, bool f32) {
    return f32 ? *(gc_f1)((const float*)base + i) : bf2f(*(gc_h1)((const uint16_t*)base + i));
}
__device__ __forceinline__ void store1f(float* base, long i, float x) { *(g_f1)(base + i) = x; }

// ---------------------------------------------------------------------------------------------------------------- stage 1
__global__ __launch_bounds__(OPT_THREADS) void optim_sqsum_kernel(const umoe_optim_tensor* __restrict__ tensors, int n_tensors,
                                                                  const umoe_optim_chunk* __restrict__ chunks, long n_chunks, int chunk_elems,
                                                                  float* __restrict__ partial, int32_t* __restrict__ flags) {
    __shared__ float wave_sum[OPT_THREADS / 64];
    const int tid = threadIdx.x;
    for (long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const chunk_view cv = chunk_open(tensors, n_tensors, chunks, c, chunk_elems, false);
        const bool f32 = (cv.t.p_fp32 & (UMOE_OPTIM_P_FP32 | UMOE_OPTIM_G_FP32)) != 0;      // the gradient's type
        float acc = 0.0f;
        const int nvec = (cv.len - cv.head) >> 3, tail0 = cv.head + (nvec << 3), nscal = cv.head + (cv.len - tail0);
        for (int i = tid; i < nvec; i += OPT_THREADS) {
            float x[8];
            load8(cv.t.g, cv.first + cv.head + ((long)i << 3), f32, x);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc = acc + x[j] * x[j];
        }
        for (int i = tid; i < nscal; i += OPT_THREADS) {
            const float x = load1(cv.t.g, cv.first + (i < cv.head ? i : tail0 + (i - cv.head)), f32);
            acc = acc + x * x;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc = acc + __shfl_xor(acc, off);
        if ((tid & 63) == 0) wave_sum[tid >> 6] = acc;
        __syncthreads();
        if (tid == 0) {
            float s = wave_sum[0];
#pragma unroll
            for (int w = 1; w < OPT_THREADS / 64; ++w) s = s + wave_sum[w];
            partial[c] = s;
            flags[c] = (fabsf(s) <= 3.402823466e38f) ? 0 : 1;      // squares are >= 0: a non-finite element (or an overflow) makes the sum inf or NaN
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------- stage 2
__global__ __launch_bounds__(OPT_THREADS) void optim_scalars_kernel(const float* __restrict__ partial, const int32_t* __restrict__ flags,
                                                                    long n_chunks, umoe_optim_hyper hy, int64_t* __restrict__ counters,
                                                                    umoe_optim_record* __restrict__ rec) {
    __shared__ double run_sum[OPT_THREADS];
    __shared__ int run_bad[OPT_THREADS];
    const int tid = threadIdx.x;
    const long per = (n_chunks + OPT_THREADS - 1) / OPT_THREADS;
    const long lo = tid * per, hi = lo + per < n_chunks ? lo + per : n_chunks;
    double s = 0.0;
    int bad = 0;
    for (long c = lo; c < hi; ++c) {
        s = s + (double)partial[c];
        bad |= flags[c];
    }
    run_sum[tid] = s;
    run_bad[tid] = bad;
    __syncthreads();
    if (tid < UMOE_OPTIM_MAX_GROUPS && tid < hy.num_groups) {          // t is read here, before thread 0 advances it behind the barrier
        const double tp1 = (double)(counters[0] + 1);
        rec->bc1[tid] = (float)(1.0 - pow(hy.beta1[tid], tp1));
        rec->bc2[tid] = (float)(1.0 - pow(hy.beta2[tid], tp1));
    }
    __syncthreads();
    if (tid == 0) {
        double tot = 0.0;
        int any = 0;
        for (int i = 0; i < OPT_THREADS; ++i) {
            tot = tot + run_sum[i];
            any |= run_bad[i];
        }
        const float norm = (float)sqrt(tot);
        const int skip = (any != 0 || !(fabs(tot) <= 1.7976931348623157e308)) ? 1 : 0;
        float clip = 1.0f;
        if (hy.max_norm >= 0.0) {
            clip = (float)hy.max_norm / (norm + 1e-6f);
            clip = clip < 1.0f ? clip : 1.0f;
        }
        rec->norm = norm;
        rec->clip = clip;
        rec->skip = skip;
        rec->reserved = 0;
        if (skip) counters[1] = counters[1] + 1;
        else counters[0] = counters[0] + 1;
    }
}

// ---------------------------------------------------------------------------------------------------------------- stage 3
struct optim_scal { float clip, b1, omb1, b2, omb2, eps, decay, step, sq; };

__device__ __forceinline__ void adamw_elem(float& w, float& m, float& v, float g, const optim_scal& s) {
    g = g * s.clip;
    m = s.b1 * m + s.omb1 * g;
    v = s.b2 * v + (s.omb2 * g) * g;
    const float den = sqrtf(v) / s.sq + s.eps;
    w = w * s.decay - (s.step * m) / den;
}

__global__ __launch_bounds__(OPT_THREADS) void optim_adamw_kernel(const umoe_optim_tensor* __restrict__ tensors, int n_tensors,
                                                                  const umoe_optim_chunk* __restrict__ chunks, long n_chunks, int chunk_elems,
                                                                  optim_kargs ka, const umoe_optim_record* __restrict__ rec,
                                                                  int64_t* __restrict__ counters) {
    const int tid = threadIdx.x;
    float clip = 1.0f;
    if (ka.t_host < 0) {
        if (rec->skip) return;
        clip = rec->clip;
    } else if (blockIdx.x == 0 && tid == 0 && counters) {
        counters[0] = ka.t_host + 1;
    }
    for (long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const chunk_view cv = chunk_open(tensors, n_tensors, chunks, c, chunk_elems, true);
        if (cv.len == 0) continue;
        const int gi = (cv.t.group >= 0 && cv.t.group < UMOE_OPTIM_MAX_GROUPS) ? cv.t.group : 0;
        const optim_group_k gk = ka.g[gi];
        const float bc1 = ka.t_host < 0 ? rec->bc1[gi] : gk.bc1, bc2 = ka.t_host < 0 ? rec->bc2[gi] : gk.bc2;
        optim_scal s;
        s.clip = clip; s.b1 = gk.b1; s.omb1 = gk.omb1; s.b2 = gk.b2; s.omb2 = gk.omb2; s.eps = gk.eps;
        s.decay = 1.0f - gk.lr * gk.wd;
        s.step = gk.lr / bc1;
        s.sq = sqrtf(bc2);
        const bool f32 = (cv.t.p_fp32 & UMOE_OPTIM_P_FP32) != 0;
        const bool gf32 = (cv.t.p_fp32 & (UMOE_OPTIM_P_FP32 | UMOE_OPTIM_G_FP32)) != 0;
        float* wbase = f32 ? (float*)cv.t.p : cv.t.master;
        const int nvec = (cv.len - cv.head) >> 3, tail0 = cv.head + (nvec << 3), nscal = cv.head + (cv.len - tail0);
        for (int i = tid; i < nvec; i += OPT_THREADS) {
            const long e = cv.first + cv.head + ((long)i << 3);
            float g[8], w[8], m[8], v[8];
            load8(cv.t.g, e, gf32, g);
            load8(wbase, e, true, w);
            load8(cv.t.m, e, true, m);
            load8(cv.t.v, e, true, v);
#pragma unroll
            for (int j = 0; j < 8; ++j) adamw_elem(w[j], m[j], v[j], g[j], s);
            store8f(wbase, e, w);
            store8f(cv.t.m, e, m);
            store8f(cv.t.v, e, v);
            if (!f32) {
                const uint4 r = pack8(w);
                *(g_u4)((uint16_t*)cv.t.p + e) = u32x4_t{r.x, r.y, r.z, r.w};
            }
        }
        for (int i = tid; i < nscal; i += OPT_THREADS) {
            const long e = cv.first + (i < cv.head ? i : tail0 + (i - cv.head));
            float w = load1(wbase, e, true), m = load1(cv.t.m, e, true), v = load1(cv.t.v, e, true);
            adamw_elem(w, m, v, load1(cv.t.g, e, gf32), s);
            store1f(wbase, e, w);
            store1f(cv.t.m, e, m);
            store1f(cv.t.v, e, v);
            if (!f32) *(g_h1)((uint16_t*)cv.t.p + e) = f2bf(w);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- fold
// main += float(g), g = +0 over the bf16 gradients autograd still produces (umoe.h "umoe_optim_fold"); the chunk walk of the stages above
__global__ __launch_bounds__(OPT_THREADS) void optim_fold_kernel(const umoe_optim_fold_tensor* __restrict__ tensors, int n_tensors,
                                                                 const umoe_optim_chunk* __restrict__ chunks, long n_chunks, int chunk_elems) {
    const int tid = threadIdx.x;
    for (long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const long ti = chunks[c].tensor, first = chunks[c].first;
        if (ti < 0 || ti >= n_tensors) continue;
        const umoe_optim_fold_tensor t = tensors[ti];
        if (!t.g || !t.main || first < 0 || first >= t.n) continue;
        const long left = t.n - first;
        const int len = (int)(left < chunk_elems ? left : chunk_elems);
        int head = head_of(t.g, first, 2);
        const bool ok = (((uintptr_t)t.g) & 1) == 0 && aligned_after(t.main, first, head, 4);
        head = ok ? (head < len ? head : len) : len;
        const int nvec = (len - head) >> 3, tail0 = head + (nvec << 3), nscal = head + (len - tail0);
        for (int i = tid; i < nvec; i += OPT_THREADS) {
            const long e = first + head + ((long)i << 3);
            float g[8], m[8];
            load8(t.g, e, false, g);
            load8(t.main, e, true, m);
#pragma unroll
            for (int j = 0; j < 8; ++j) m[j] = m[j] + g[j];
            store8f(t.main, e, m);
            *(g_u4)(t.g + e) = u32x4_t{0u, 0u, 0u, 0u};
        }
        for (int i = tid; i < nscal; i += OPT_THREADS) {
            const long e = first + (i < head ? i : tail0 + (i - head));
            store1f(t.main, e, load1(t.main, e, true) + load1(t.g, e, false));
            *(g_h1)(t.g + e) = (uint16_t)0;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
static int optim_check_tables(const char* who, const void* tensors, int n_tensors, const void* chunks, int64_t n_chunks, int chunk_elems,
                              const umoe_optim_tensor* ht, const umoe_optim_chunk* hc, int num_groups, int grid_cap) {
    UMOE_REQUIRE(n_tensors >= 0 && n_chunks >= 0 && grid_cap >= 0, "%s: negative count", who);
    UMOE_REQUIRE(chunk_elems > 0 && chunk_elems % 8 == 0, "%s: chunk_elems must be a positive multiple of 8 (got %d)", who, chunk_elems);
    UMOE_REQUIRE(num_groups >= 1 && num_groups <= UMOE_OPTIM_MAX_GROUPS, "%s: %d parameter groups (1..%d)", who, num_groups, UMOE_OPTIM_MAX_GROUPS);
    if (n_chunks == 0) return 0;
    UMOE_REQUIRE(tensors && chunks && n_tensors > 0, "%s: NULL table", who);
    UMOE_REQUIRE((ht == nullptr) == (hc == nullptr), "%s: host_tensors and host_chunks go together", who);
    if (!ht) return 0;
    for (int i = 0; i < n_tensors; ++i) {
        UMOE_REQUIRE(ht[i].n >= 0 && ht[i].group >= 0 && ht[i].group < num_groups, "%s: tensor %d: n %lld, group %d of %d", who, i,
                     (long long)ht[i].n, ht[i].group, num_groups);
        UMOE_REQUIRE(ht[i].n == 0 || !ht[i].g || (ht[i].p && ht[i].m && ht[i].v && ((ht[i].p_fp32 & UMOE_OPTIM_P_FP32) || ht[i].master)),
                     "%s: tensor %d: NULL p / master / m / v", who, i);
    }
    for (int64_t c = 0; c < n_chunks; ++c) {
        const int64_t ti = hc[c].tensor, first = hc[c].first;
        UMOE_REQUIRE(ti >= 0 && ti < n_tensors, "%s: chunk %lld names tensor %lld of %d", who, (long long)c, (long long)ti, n_tensors);
        UMOE_REQUIRE(first >= 0 && first < ht[ti].n && first % chunk_elems == 0,
                     "%s: chunk %lld crosses its tensor (first %lld, n %lld, chunk_elems %d)", who, (long long)c, (long long)first,
                     (long long)ht[ti].n, chunk_elems);
    }
    return 0;
}

static unsigned optim_grid(int64_t n_chunks, int grid_cap) {
    const int64_t cap = grid_cap > 0 ? grid_cap : OPT_DEFAULT_GRID;
    return (unsigned)(n_chunks < cap ? n_chunks : cap);
}

extern "C" int umoe_optim_sqsum(const umoe_optim_tensor* tensors, int n_tensors, const umoe_optim_chunk* chunks, int64_t n_chunks,
                                int chunk_elems, const umoe_optim_tensor* host_tensors, const umoe_optim_chunk* host_chunks, int num_groups,
                                int grid_cap, float* partial, int32_t* flags, umoe_stream_t stream) {
    if (int rc = optim_check_tables("umoe_optim_sqsum", tensors, n_tensors, chunks, n_chunks, chunk_elems, host_tensors, host_chunks,
                                    num_groups, grid_cap))
        return rc;
    if (n_chunks == 0) return 0;
    UMOE_REQUIRE(partial && flags, "umoe_optim_sqsum: NULL partial / flags");
    optim_sqsum_kernel<<<dim3(optim_grid(n_chunks, grid_cap)), OPT_THREADS, 0, (hipStream_t)stream>>>(tensors, n_tensors, chunks, (long)n_chunks,
                                                                                                     chunk_elems, partial, flags);
    UMOE_LAUNCH_CHECK();
    return 0;
}

static int optim_check_hyper(const char* who, const umoe_optim_hyper* hy) {
    UMOE_REQUIRE(hy, "%s: NULL hyper", who);
    UMOE_REQUIRE(hy->num_groups >= 1 && hy->num_groups <= UMOE_OPTIM_MAX_GROUPS, "%s: %d parameter groups (1..%d)", who, hy->num_groups,
                 UMOE_OPTIM_MAX_GROUPS);
    return 0;
}

extern "C" int umoe_optim_scalars(const float* partial, const int32_t* flags, int64_t n_chunks, const umoe_optim_hyper* hyper,
                                  int64_t* counters, umoe_optim_record* rec, umoe_stream_t stream) {
    if (int rc = optim_check_hyper("umoe_optim_scalars", hyper)) return rc;
    UMOE_REQUIRE(n_chunks >= 0, "umoe_optim_scalars: negative count");
    if (n_chunks == 0) return 0;
    UMOE_REQUIRE(partial && flags && counters && rec, "umoe_optim_scalars: NULL partial / flags / counters / rec");
    optim_scalars_kernel<<<dim3(1), OPT_THREADS, 0, (hipStream_t)stream>>>(partial, flags, (long)n_chunks, *hyper, counters, rec);
    UMOE_LAUNCH_CHECK();
    return 0;
}

extern "C" int umoe_optim_adamw(const umoe_optim_tensor* tensors, int n_tensors, const umoe_optim_chunk* chunks, int64_t n_chunks,
                                int chunk_elems, const umoe_optim_tensor* host_tensors, const umoe_optim_chunk* host_chunks, int grid_cap,
                                const umoe_optim_hyper* hyper, const umoe_optim_record* rec, int64_t t_host, int64_t* counters,
                                umoe_stream_t stream) {
    if (int rc = optim_check_hyper("umoe_optim_adamw", hyper)) return rc;
    if (int rc = optim_check_tables("umoe_optim_adamw", tensors, n_tensors, chunks, n_chunks, chunk_elems, host_tensors, host_chunks,
                                    hyper->num_groups, grid_cap))
        return rc;
    if (n_chunks == 0) return 0;
    UMOE_REQUIRE((rec != nullptr) != (t_host >= 0), "umoe_optim_adamw: pass the record of stage 2 (t_host < 0) or t_host >= 0 (rec NULL), not both");
    optim_kargs ka;
    ka.t_host = rec ? -1 : (long long)t_host;
    for (int g = 0; g < UMOE_OPTIM_MAX_GROUPS; ++g) {
        const bool on = g < hyper->num_groups;
        optim_group_k& k = ka.g[g];
        k.lr = on ? (float)hyper->lr[g] : 0.0f;
        k.b1 = on ? (float)hyper->beta1[g] : 0.0f;
        k.omb1 = on ? (float)(1.0 - hyper->beta1[g]) : 0.0f;
        k.b2 = on ? (float)hyper->beta2[g] : 0.0f;
        k.omb2 = on ? (float)(1.0 - hyper->beta2[g]) : 0.0f;
        k.eps = on ? (float)hyper->eps[g] : 1.0f;
        k.wd = on ? (float)hyper->wd[g] : 0.0f;
        k.bc1 = (on && !rec) ? (float)(1.0 - pow(hyper->beta1[g], (double)(t_host + 1))) : 1.0f;
        k.bc2 = (on && !rec) ? (float)(1.0 - pow(hyper->beta2[g], (double)(t_host + 1))) : 1.0f;
    }
    optim_adamw_kernel<<<dim3(optim_grid(n_chunks, grid_cap)), OPT_THREADS, 0, (hipStream_t)stream>>>(tensors, n_tensors, chunks, (long)n_chunks,
                                                                                                     chunk_elems, ka, rec, counters);
    UMOE_LAUNCH_CHECK();
    return 0;
}

extern "C" int umoe_optim_fold(const umoe_optim_fold_tensor* tensors, int n_tensors, const umoe_optim_chunk* chunks, int64_t n_chunks,
                               int chunk_elems, const umoe_optim_fold_tensor* host_tensors, const umoe_optim_chunk* host_chunks, int grid_cap,
                               umoe_stream_t stream) {
    const char* who = "umoe_optim_fold";
    UMOE_REQUIRE(n_tensors >= 0 && n_chunks >= 0 && grid_cap >= 0, "%s: negative count", who);
    UMOE_REQUIRE(chunk_elems > 0 && chunk_elems % 8 == 0, "%s: chunk_elems must be a positive multiple of 8 (got %d)", who, chunk_elems);
    if (n_chunks == 0) return 0;
    UMOE_REQUIRE(tensors && chunks && n_tensors > 0, "%s: NULL table", who);
    UMOE_REQUIRE((host_tensors == nullptr) == (host_chunks == nullptr), "%s: host_tensors and host_chunks go together", who);
    if (host_tensors) {
        for (int i = 0; i < n_tensors; ++i) {
            UMOE_REQUIRE(host_tensors[i].n >= 0, "%s: tensor %d: n %lld", who, i, (long long)host_tensors[i].n);
            UMOE_REQUIRE(host_tensors[i].n == 0 || !host_tensors[i].g || host_tensors[i].main, "%s: tensor %d: a gradient without a main gradient", who, i);
            UMOE_REQUIRE((reinterpret_cast<size_t>(host_tensors[i].g) & 1) == 0 && (reinterpret_cast<size_t>(host_tensors[i].main) & 3) == 0,
                         "%s: tensor %d: misaligned g / main", who, i);
        }
        for (int64_t c = 0; c < n_chunks; ++c) {
            const int64_t ti = host_chunks[c].tensor, first = host_chunks[c].first;
            UMOE_REQUIRE(ti >= 0 && ti < n_tensors, "%s: chunk %lld names tensor %lld of %d", who, (long long)c, (long long)ti, n_tensors);
            UMOE_REQUIRE(first >= 0 && first < host_tensors[ti].n && first % chunk_elems == 0,
                         "%s: chunk %lld crosses its tensor (first %lld, n %lld, chunk_elems %d)", who, (long long)c, (long long)first,
                         (long long)host_tensors[ti].n, chunk_elems);
        }
    }
    optim_fold_kernel<<<dim3(optim_grid(n_chunks, grid_cap)), OPT_THREADS, 0, (hipStream_t)stream>>>(tensors, n_tensors, chunks, (long)n_chunks,
                                                                                                    chunk_elems);
    UMOE_LAUNCH_CHECK();
    return 0;
}
