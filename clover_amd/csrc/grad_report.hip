// Overflow report: which parameters hold the non-finite gradients behind a skipped optimizer step.
//
// The reference finds an overflow with one host synchronisation per parameter (LossScaler.has_overflow / _has_inf_or_nan,
// mmaction/core/hooks/fp16_utils.py:328-349) and announces every one of them (mmcv_Fp16OptimizerHook.py:123-141: "Check
// overflow, currently only support static/dynamic loss scale").  Here the skip decision lives on the device (clv_optim_prep,
// optim_state.hpp), so the report is taken there too: two plain launches over one gradient buffer — an fp32 slab, or the 16-bit
// wire copy of a data-parallel job — that exit at once on a step that is not skipped (mode 0).
//
// Both walk a TABLE (device memory, built once by the host: ops.grad_report_table), the pattern of clv_ema_update:
//   n_params x ParamRec {first chunk, chunks}     one per parameter
//   n_chunks x ChunkRec {parameter, start, count} one per 256-thread block of pass 1: <= CLV_SUMSQ_CHUNK elements of ONE
//                                                 parameter, start counted in elements from the buffer's first
// and write the REPORT (device memory, CLV_GRAD_REPORT_HEADER_BYTES + 16 bytes per parameter + 16 bytes per chunk):
//   header   {int32 t, skipped; float loss_scale; int32 n_params; 4 x int32 0}
//   n_params x Stat   the parameter's {int32 nonfinite; float max_abs; float sumsq; float norm = sqrt(sumsq)}
//   n_chunks x Stat   pass 1's partial records (pass 2's input)
// max_abs, sumsq and norm cover the FINITE elements only, in the units the buffer holds (loss scale and all).
//
// Pass 1: one block per chunk.  16-byte loads from the first 16-byte boundary on, the elements before it and the < 16 bytes
// behind the last full vector one by one; every thread folds its elements in index order, then a fixed xor tree over the
// wave and a fixed sum over the four waves.  Pass 2: one wave per parameter, lane l folds chunks l, l + 64, ... in index
// order, then the same tree.  No atomics anywhere: the report is a pure function of buffer and table, bit-reproducible,
// and every word of it is rewritten by every reporting call.
#include "common.hpp"
#include "../../include/clover_hip.h"
#include "optim_state.hpp"

namespace {

struct ParamRec {
    int64_t first;         // index of the parameter's first chunk record
    int64_t chunks;        // how many follow (0: an empty parameter)
};

struct ChunkRec {
    int64_t param;
    int64_t start;         // elements from the buffer's first
    int64_t count;         // 1 .. CLV_SUMSQ_CHUNK
};

struct Stat {
    int32_t nonfinite;
    uint32_t max_abs;      // the bits of an fp32 >= 0: ordered like the values, so the maximum is an integer maximum
    float sumsq;
    float norm;
};

struct Header {
    int32_t t, skipped;
    float loss_scale;
    int32_t n_params;
    int32_t zero[4];
};

static_assert(sizeof(ParamRec) == CLV_GRAD_REPORT_PARAM_BYTES, "table layout is part of the ABI");
static_assert(sizeof(ChunkRec) == CLV_GRAD_REPORT_CHUNK_BYTES, "table layout is part of the ABI");
static_assert(sizeof(Stat) == CLV_GRAD_REPORT_STAT_BYTES, "report layout is part of the ABI");
static_assert(sizeof(Header) == CLV_GRAD_REPORT_HEADER_BYTES, "report layout is part of the ABI");
static_assert(CLV_SUMSQ_CHUNK % (8 * 256) == 0, "a full chunk is a whole number of 16-byte rounds of one block");

// The buffer is global memory (the host hands over a device tensor): say so, and the loads are global_load_dwordx4.
#define CLV_GLOBAL __attribute__((address_space(1)))
typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));

struct Acc {
    uint32_t nonfinite = 0, max_abs = 0;
    float sumsq = 0.f;
};

// one element: (is it finite, |g| as bits, g^2), the last two 0 for a NaN / an infinity
__device__ __forceinline__ float fold_one(float g, Acc& a) {
    const uint32_t mag = __float_as_uint(g) & 0x7fffffffu;
    const bool finite = mag < 0x7f800000u;
    a.nonfinite += finite ? 0u : 1u;
    a.max_abs = max(a.max_abs, finite ? mag : 0u);
    const float v = finite ? g : 0.f;
    return v * v;
}

template <typename T> struct Vec;
template <> struct Vec<float> {
    static constexpr int N = 4;
    static __device__ __forceinline__ float one(const CLV_GLOBAL float* g, int i) { return g[i]; }
    static __device__ __forceinline__ void fold(u32x4v u, Acc& a) {
        const float s0 = fold_one(__uint_as_float(u.x), a), s1 = fold_one(__uint_as_float(u.y), a);
        const float s2 = fold_one(__uint_as_float(u.z), a), s3 = fold_one(__uint_as_float(u.w), a);
        a.sumsq += (s0 + s1) + (s2 + s3);
    }
};
template <> struct Vec<bf16_t> {
    static constexpr int N = 8;
    static __device__ __forceinline__ float one(const CLV_GLOBAL bf16_t* g, int i) { return bf2f(g[i]); }
    static __device__ __forceinline__ void fold(u32x4v u, Acc& a) {
        const float s0 = fold_one(half_lo(u.x), a), s1 = fold_one(half_hi(u.x), a);
        const float s2 = fold_one(half_lo(u.y), a), s3 = fold_one(half_hi(u.y), a);
        const float s4 = fold_one(half_lo(u.z), a), s5 = fold_one(half_hi(u.z), a);
        const float s6 = fold_one(half_lo(u.w), a), s7 = fold_one(half_hi(u.w), a);
        a.sumsq += ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7));
    }
};

__device__ __forceinline__ void wave_fold(Acc& a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a.nonfinite += (uint32_t)__shfl_xor((int)a.nonfinite, o, 64);
        a.max_abs = max(a.max_abs, (uint32_t)__shfl_xor((int)a.max_abs, o, 64));
        a.sumsq += __shfl_xor(a.sumsq, o, 64);
    }
}

template <typename T>
__global__ void __launch_bounds__(256) grad_report_chunks_kernel(const T* __restrict__ base, const ChunkRec* __restrict__ chunks,
                                                                 const OptimState* __restrict__ st, Stat* __restrict__ partial,
                                                                 int mode) {
    if (mode == 0 && st->skip == 0) return;            // a step that was taken: nothing to report, the last report stays
    constexpr int N = Vec<T>::N;
    constexpr int ROUNDS = CLV_SUMSQ_CHUNK / (N * 256);
    __shared__ uint32_t sh_nf[4], sh_mx[4];
    __shared__ float sh_ss[4];
    const ChunkRec c = chunks[blockIdx.x];
    const int cnt = (int)c.count;
    const CLV_GLOBAL T* g = (const CLV_GLOBAL T*)(base + c.start);
    const int off = (int)(((uintptr_t)g) & 15);
    int head = off ? (16 - off) / (int)sizeof(T) : 0;  // elements in front of the first 16-byte boundary
    if (head > cnt) head = cnt;
    const int nvec = (cnt - head) / N;
    const CLV_GLOBAL u32x4v* g4 = (const CLV_GLOBAL u32x4v*)(g + head);
    Acc a;
    if ((int)threadIdx.x < head) a.sumsq += fold_one(Vec<T>::one(g, threadIdx.x), a);
    if (nvec == ROUNDS * 256) {                        // the common case, a full aligned chunk: every load in flight at once
        u32x4v v[ROUNDS];
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) v[r] = g4[r * 256 + threadIdx.x];
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) Vec<T>::fold(v[r], a);
    } else {
        for (int i = threadIdx.x; i < nvec; i += 256) Vec<T>::fold(g4[i], a);
    }
    const int tail = head + nvec * N + (int)threadIdx.x;       // < 16 bytes behind the last vector
    if (tail < cnt) a.sumsq += fold_one(Vec<T>::one(g, tail), a);
    wave_fold(a);
    if ((threadIdx.x & 63) == 0) {
        sh_nf[threadIdx.x >> 6] = a.nonfinite;
        sh_mx[threadIdx.x >> 6] = a.max_abs;
        sh_ss[threadIdx.x >> 6] = a.sumsq;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        Stat s;
        s.nonfinite = (int32_t)((sh_nf[0] + sh_nf[1]) + (sh_nf[2] + sh_nf[3]));
        s.max_abs = max(max(sh_mx[0], sh_mx[1]), max(sh_mx[2], sh_mx[3]));
        s.sumsq = (sh_ss[0] + sh_ss[1]) + (sh_ss[2] + sh_ss[3]);
        s.norm = sqrtf(s.sumsq);
        partial[blockIdx.x] = s;
    }
}

__global__ void __launch_bounds__(256) grad_report_params_kernel(const ParamRec* __restrict__ params,
                                                                 const OptimState* __restrict__ st, Header* __restrict__ header,
                                                                 Stat* __restrict__ stats, const Stat* __restrict__ partial,
                                                                 int n_params, int mode) {
    if (mode == 0 && st->skip == 0) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        Header h;
        h.t = st->t;
        h.skipped = st->skipped;
        // mode 0 runs behind clv_optim_prep, which may have moved a dynamic scale already: it kept the old one
        h.loss_scale = mode == 0 ? st->grad_loss_scale : st->loss_scale;
        h.n_params = n_params;
        h.zero[0] = h.zero[1] = h.zero[2] = h.zero[3] = 0;
        *header = h;
    }
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= n_params) return;
    const ParamRec r = params[p];
    Acc a;
    for (int64_t i = threadIdx.x & 63; i < r.chunks; i += 64) {
        const Stat s = partial[r.first + i];
        a.nonfinite += (uint32_t)s.nonfinite;
        a.max_abs = max(a.max_abs, s.max_abs);
        a.sumsq += s.sumsq;
    }
    wave_fold(a);
    if ((threadIdx.x & 63) == 0) {
        Stat s;
        s.nonfinite = (int32_t)a.nonfinite;
        s.max_abs = a.max_abs;
        s.sumsq = a.sumsq;
        s.norm = sqrtf(a.sumsq);
        stats[p] = s;
    }
}

}  // namespace

extern "C" int clv_grad_report(const void* buf, int32_t elem, const void* table, int32_t n_params, int32_t n_chunks,
                               const void* state, void* report, int32_t mode, void* stream) {
    if (!buf || !table || !state || !report || n_params < 0 || n_chunks < 0 || (mode != 0 && mode != 1) ||
        (elem != CLV_GRAD_REPORT_F32 && elem != CLV_GRAD_REPORT_HALF))
        return CLV_ERR_ARG;
    if ((((uintptr_t)table) & 7) || (((uintptr_t)state) & 3) || (((uintptr_t)report) & 15)) return CLV_ERR_ARG;
    if (((uintptr_t)buf) & (elem == CLV_GRAD_REPORT_F32 ? 3 : 1)) return CLV_ERR_ARG;
    if (n_params == 0 && n_chunks > 0) return CLV_ERR_ARG;
    const ParamRec* params = (const ParamRec*)table;
    const ChunkRec* chunks = (const ChunkRec*)(params + n_params);
    Header* header = (Header*)report;
    Stat* stats = (Stat*)(header + 1);
    Stat* partial = stats + n_params;
    const OptimState* st = (const OptimState*)state;
    if (n_chunks > 0) {
        if (elem == CLV_GRAD_REPORT_F32)
            hipLaunchKernelGGL(grad_report_chunks_kernel<float>, dim3((unsigned)n_chunks), dim3(256), 0, (hipStream_t)stream,
                               (const float*)buf, chunks, st, partial, (int)mode);
        else
            hipLaunchKernelGGL(grad_report_chunks_kernel<bf16_t>, dim3((unsigned)n_chunks), dim3(256), 0, (hipStream_t)stream,
                               (const bf16_t*)buf, chunks, st, partial, (int)mode);
        const int rc = clv_check_launch();
        if (rc != CLV_OK) return rc;
    }
    hipLaunchKernelGGL(grad_report_params_kernel, dim3((unsigned)((n_params + 3) / 4 > 0 ? (n_params + 3) / 4 : 1)), dim3(256), 0,
                       (hipStream_t)stream, params, st, header, stats, partial, (int)n_params, (int)mode);
    return clv_check_launch();
}
