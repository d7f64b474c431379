// Activation report: which forward output went non-finite first, and how close the others are to the 16-bit limit.
//
// The gradient report (grad_report.hip) names the parameters whose gradients were non-finite.  When the overflow is in the
// FORWARD pass — an fp16 activation above 65504 is stored as inf, everything behind it is NaN — that list is the whole
// model.  The reference has nothing better: LossScaler.has_overflow / _has_inf_or_nan (mmaction/core/hooks/fp16_utils.py:
// 328-349) looks at gradients only, and mmcv_Fp16OptimizerHook.py:123-141 announces "Check overflow" without a place.  Here
// every watched module's output is folded into one 16-byte RECORD on the device, inside the step's hipGraphs:
//   Slot {int32 nonfinite; uint32 max_abs; int32 calls; int32 zero}
// nonfinite counts the NaN / infinite elements, max_abs holds the bits of the largest FINITE |x| as fp32 (ordered like an
// integer: the convention of Stat in grad_report.hip), calls counts the launches folded in since the record was cleared.
//
// clv_act_report: one launch, a bounded grid with a grid-stride loop of 16-byte loads from the first 16-byte boundary on,
// the elements before it and the < 16 bytes behind the last full vector one by one (block 0); an xor tree over the wave,
// a fold over the block's four waves, then at most one integer atomicAdd and one integer atomicMax per block on the record.
// Integer add and max commute, so the record is a pure function of what was folded in, whatever order the blocks finish in.
// No float is ever accumulated.
//
// clv_act_report_latch: one small launch behind clv_optim_prep that returns at once on a step that was taken (mode 0 of the
// gradient report) and otherwise copies the live records behind a header of the gradient report's layout.
#include "common.hpp"
#include "../../include/clover_hip.h"
#include "optim_state.hpp"

namespace {

struct Slot {
    int32_t nonfinite;
    uint32_t max_abs;      // the bits of an fp32 >= 0: ordered like the values, so the maximum is an integer maximum
    int32_t calls;
    int32_t zero;
};

struct Header {            // the Header of grad_report.hip, n_slots in its n_params word
    int32_t t, skipped;
    float loss_scale;
    int32_t n_slots;
    int32_t zero[4];
};

static_assert(sizeof(Slot) == CLV_ACT_REPORT_SLOT_BYTES, "record layout is part of the ABI");
static_assert(sizeof(Header) == CLV_GRAD_REPORT_HEADER_BYTES, "report layout is part of the ABI");

#define CLV_GLOBAL __attribute__((address_space(1)))
typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));

constexpr int ACT_THREADS = 256;
constexpr int ACT_UNROLL = 2;          // 16-byte loads one thread keeps in flight
constexpr int ACT_MAX_BLOCKS = 256;    // one block per CU: the grid never grows with the tensor beyond this (2 MiB a pass)

struct Acc {
    uint32_t nonfinite = 0, max_abs = 0;
};

__device__ __forceinline__ void fold_one(float x, Acc& a) {
    const uint32_t mag = __float_as_uint(x) & 0x7fffffffu;
    const bool finite = mag < 0x7f800000u;
    a.nonfinite += finite ? 0u : 1u;
    a.max_abs = max(a.max_abs, finite ? mag : 0u);
}

template <typename T> struct Vec;
template <> struct Vec<float> {
    static constexpr int N = 4;
    static __device__ __forceinline__ float one(const CLV_GLOBAL float* g, int i) { return g[i]; }
    static __device__ __forceinline__ void fold(u32x4v u, Acc& a) {
        fold_one(__uint_as_float(u.x), a);
        fold_one(__uint_as_float(u.y), a);
        fold_one(__uint_as_float(u.z), a);
        fold_one(__uint_as_float(u.w), a);
    }
};
template <> struct Vec<bf16_t> {
    static constexpr int N = 8;
    static __device__ __forceinline__ float one(const CLV_GLOBAL bf16_t* g, int i) { return bf2f(g[i]); }
    static __device__ __forceinline__ void fold(u32x4v u, Acc& a) {
        fold_one(half_lo(u.x), a);
        fold_one(half_hi(u.x), a);
        fold_one(half_lo(u.y), a);
        fold_one(half_hi(u.y), a);
        fold_one(half_lo(u.z), a);
        fold_one(half_hi(u.z), a);
        fold_one(half_lo(u.w), a);
        fold_one(half_hi(u.w), a);
    }
};

// head: elements in front of the first 16-byte boundary (< Vec<T>::N, clamped to count by the host); nvec: full vectors
template <typename T>
__global__ void __launch_bounds__(ACT_THREADS) act_report_kernel(const T* __restrict__ base, int count, int head, int nvec,
                                                                 Slot* __restrict__ slot) {
    constexpr int N = Vec<T>::N;
    __shared__ uint32_t sh_nf[ACT_THREADS / 64], sh_mx[ACT_THREADS / 64];
    const CLV_GLOBAL T* g = (const CLV_GLOBAL T*)base;
    const CLV_GLOBAL u32x4v* g4 = (const CLV_GLOBAL u32x4v*)(g + head);
    Acc a;
    if (blockIdx.x == 0) {
        if ((int)threadIdx.x < head) fold_one(Vec<T>::one(g, threadIdx.x), a);
        const int done = head + nvec * N;                      // < 16 bytes are left behind the last vector
        if ((int)threadIdx.x < count - done) fold_one(Vec<T>::one(g, done + (int)threadIdx.x), a);
    }
    const int stride = (int)gridDim.x * ACT_THREADS;
    int i = (int)blockIdx.x * ACT_THREADS + (int)threadIdx.x;
    for (; i + (ACT_UNROLL - 1) * stride < nvec; i += ACT_UNROLL * stride) {
        u32x4v v[ACT_UNROLL];
#pragma unroll
        for (int r = 0; r < ACT_UNROLL; ++r) v[r] = g4[i + r * stride];
#pragma unroll
        for (int r = 0; r < ACT_UNROLL; ++r) Vec<T>::fold(v[r], a);
    }
    for (; i < nvec; i += stride) Vec<T>::fold(g4[i], a);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a.nonfinite += (uint32_t)__shfl_xor((int)a.nonfinite, o, 64);
        a.max_abs = max(a.max_abs, (uint32_t)__shfl_xor((int)a.max_abs, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        sh_nf[threadIdx.x >> 6] = a.nonfinite;
        sh_mx[threadIdx.x >> 6] = a.max_abs;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t nf = (sh_nf[0] + sh_nf[1]) + (sh_nf[2] + sh_nf[3]);
        const uint32_t mx = max(max(sh_mx[0], sh_mx[1]), max(sh_mx[2], sh_mx[3]));
        // adding 0 and maxing with 0 change nothing (max_abs >= 0): a block that has nothing to say stays off the record
        if (nf) atomicAdd(&slot->nonfinite, (int)nf);
        if (mx) atomicMax(&slot->max_abs, mx);
        if (blockIdx.x == 0) atomicAdd(&slot->calls, 1);
    }
}

__global__ void __launch_bounds__(256) act_report_latch_kernel(const OptimState* __restrict__ st,
                                                               const uint32_t* __restrict__ live, Header* __restrict__ header,
                                                               int n_slots) {
    if (st->skip == 0) return;             // a step that was taken: nothing to report, the last report stays
    if (threadIdx.x == 0) {
        Header h;
        h.t = st->t;
        h.skipped = st->skipped;
        h.loss_scale = st->grad_loss_scale;    // behind clv_optim_prep a dynamic scale has moved already: it kept the old one
        h.n_slots = n_slots;
        h.zero[0] = h.zero[1] = h.zero[2] = h.zero[3] = 0;
        *header = h;
    }
    uint32_t* out = (uint32_t*)(header + 1);
    const int words = n_slots * (int)(sizeof(Slot) / sizeof(uint32_t));
    for (int i = threadIdx.x; i < words; i += 256) out[i] = live[i];
}

}  // namespace

extern "C" int clv_act_report(const void* x, int64_t count, int32_t elem, void* slot, void* stream) {
    if (!slot || (((uintptr_t)slot) & 15) || count < 0 || (elem != CLV_GRAD_REPORT_F32 && elem != CLV_GRAD_REPORT_HALF))
        return CLV_ERR_ARG;
    if (count > 0x7fffffffLL) return CLV_ERR_UNSUPPORTED;
    const int esize = elem == CLV_GRAD_REPORT_F32 ? 4 : 2;
    if (count > 0 && (!x || (((uintptr_t)x) & (uintptr_t)(esize - 1)))) return CLV_ERR_ARG;
    const int n = (int)count, per = 16 / esize;
    const int off = (int)(((uintptr_t)x) & 15);
    int head = off ? (16 - off) / esize : 0;
    if (head > n) head = n;
    const int nvec = (n - head) / per;
    int blocks = (nvec + ACT_THREADS * ACT_UNROLL - 1) / (ACT_THREADS * ACT_UNROLL);
    blocks = blocks < 1 ? 1 : (blocks > ACT_MAX_BLOCKS ? ACT_MAX_BLOCKS : blocks);
    if (elem == CLV_GRAD_REPORT_F32)
        hipLaunchKernelGGL(act_report_kernel<float>, dim3((unsigned)blocks), dim3(ACT_THREADS), 0, (hipStream_t)stream,
                           (const float*)x, n, head, nvec, (Slot*)slot);
    else
        hipLaunchKernelGGL(act_report_kernel<bf16_t>, dim3((unsigned)blocks), dim3(ACT_THREADS), 0, (hipStream_t)stream,
                           (const bf16_t*)x, n, head, nvec, (Slot*)slot);
    return clv_check_launch();
}

extern "C" int clv_act_report_latch(const void* state, const void* live, void* latched, int32_t n_slots, void* stream) {
    if (!state || !live || !latched || n_slots < 0 || n_slots > (1 << 24)) return CLV_ERR_ARG;
    if ((((uintptr_t)state) & 3) || (((uintptr_t)live) & 15) || (((uintptr_t)latched) & 15)) return CLV_ERR_ARG;
    hipLaunchKernelGGL(act_report_latch_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const OptimState*)state,
                       (const uint32_t*)live, (Header*)latched, (int)n_slots);
    return clv_check_launch();
}
