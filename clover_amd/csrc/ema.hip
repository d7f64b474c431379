// Exponential moving average of the weights (the reference's ema_hook, mmaction/core/hooks/ema.py) on the engine's flat
// fp32 slabs: one launch updates the average of the whole model, one launch exchanges average and weights in place.
// Pure HBM streaming like optim.hip: 16 B per lane where an entry allows it, no atomics, every element has one writer.
//
// Both kernels walk a TABLE (device memory, built once by the host: ops.ema_table), the pattern of clv_sumsq_ranges:
//   n_entries x Entry            what to work on: pointers + length of one slab or one loose tensor
//   n_blocks  x EmaBlock         one record per 256-thread block: which entry, and where its chunk of <= CLV_EMA_CHUNK
//                                floats starts (a multiple of CLV_EMA_CHUNK, so a chunk is 16-byte aligned iff its entry is)
// A chunk whose pointers are 16-byte aligned moves float4s and finishes the < 4 floats of an entry's tail one by one; any
// other chunk (a loose tensor that starts off a 16-byte boundary) goes element by element.
#include "common.hpp"
#include "../../include/clover_hip.h"

namespace {

struct EmaUpdateEntry {
    const float* p;
    float* ema;
    int64_t n;
};

struct EmaSwapEntry {
    float* p;
    float* ema;
    bf16_t* shadow;        // 16-bit compute copy of p (null: none)
    int64_t n;
};

struct EmaBlock {
    int64_t entry;
    int64_t start;
};

static_assert(sizeof(EmaUpdateEntry) == CLV_EMA_UPDATE_ENTRY_BYTES, "table layout is part of the ABI");
static_assert(sizeof(EmaSwapEntry) == CLV_EMA_SWAP_ENTRY_BYTES, "table layout is part of the ABI");
static_assert(sizeof(EmaBlock) == CLV_EMA_BLOCK_BYTES, "table layout is part of the ABI");
static_assert(CLV_EMA_CHUNK % (4 * 256) == 0, "a full chunk is a whole number of float4 rounds of one block");

constexpr int ROUNDS = CLV_EMA_CHUNK / (4 * 256);      // float4s per thread in a full chunk

// The pointers come out of the table, so the compiler cannot know that they are global memory and would address them as
// flat; they always are (the host builds the table from device tensors): say so, and the accesses are global_load / _store.
#define CLV_GLOBAL __attribute__((address_space(1)))
typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2v __attribute__((ext_vector_type(2)));
template <typename T, typename S>
__device__ __forceinline__ CLV_GLOBAL T* global_ptr(S* p) { return (CLV_GLOBAL T*)(p); }

// ema <- (1 - m) ema + m p: the product (1 - m) ema rounded, then ONE fused multiply-add (buf.mul_(1 - m).add_(p, alpha=m)
// with its last two roundings merged)
__device__ __forceinline__ float ema_one(float e, float p, float m, float om) { return fmaf(m, p, om * e); }

__global__ void __launch_bounds__(256) ema_update_kernel(const EmaUpdateEntry* __restrict__ entries,
                                                         const EmaBlock* __restrict__ blocks, float m, float om) {
    const EmaBlock b = blocks[blockIdx.x];
    const EmaUpdateEntry e = entries[b.entry];
    const int64_t left = e.n - b.start;
    const int cnt = (int)(left < CLV_EMA_CHUNK ? left : CLV_EMA_CHUNK);
    const CLV_GLOBAL float* __restrict__ p = global_ptr<const float>(e.p + b.start);
    CLV_GLOBAL float* __restrict__ q = global_ptr<float>(e.ema + b.start);
    if (((((uintptr_t)p) | ((uintptr_t)q)) & 15) == 0) {
        const int n4 = cnt >> 2;
        const CLV_GLOBAL f32x4v* p4 = (const CLV_GLOBAL f32x4v*)p;
        CLV_GLOBAL f32x4v* q4 = (CLV_GLOBAL f32x4v*)q;
        if (cnt == CLV_EMA_CHUNK) {                    // the common case: every load in flight before the first store
            f32x4v pv[ROUNDS], ev[ROUNDS];
#pragma unroll
            for (int r = 0; r < ROUNDS; ++r) {
                pv[r] = p4[r * 256 + threadIdx.x];
                ev[r] = q4[r * 256 + threadIdx.x];
            }
#pragma unroll
            for (int r = 0; r < ROUNDS; ++r) {
                f32x4v o;
                o.x = ema_one(ev[r].x, pv[r].x, m, om);
                o.y = ema_one(ev[r].y, pv[r].y, m, om);
                o.z = ema_one(ev[r].z, pv[r].z, m, om);
                o.w = ema_one(ev[r].w, pv[r].w, m, om);
                q4[r * 256 + threadIdx.x] = o;
            }
            return;
        }
        for (int i = threadIdx.x; i < n4; i += 256) {
            const f32x4v pv = p4[i];
            f32x4v ev = q4[i];
            ev.x = ema_one(ev.x, pv.x, m, om);
            ev.y = ema_one(ev.y, pv.y, m, om);
            ev.z = ema_one(ev.z, pv.z, m, om);
            ev.w = ema_one(ev.w, pv.w, m, om);
            q4[i] = ev;
        }
        const int i = n4 * 4 + (int)threadIdx.x;       // the entry's tail: < 4 floats
        if (i < cnt) q[i] = ema_one(q[i], p[i], m, om);
    } else {
        for (int i = threadIdx.x; i < cnt; i += 256) q[i] = ema_one(q[i], p[i], m, om);
    }
}

// p <-> ema, bit for bit (moved as integers: no floating-point instruction touches a NaN payload), and the 16-bit copy of
// the NEW p by the conversion the AdamW kernel writes its shadow with (pack2bf / f2bf of common.hpp).
__global__ void __launch_bounds__(256) ema_swap_kernel(const EmaSwapEntry* __restrict__ entries,
                                                       const EmaBlock* __restrict__ blocks) {
    const EmaBlock b = blocks[blockIdx.x];
    const EmaSwapEntry e = entries[b.entry];
    const int64_t left = e.n - b.start;
    const int cnt = (int)(left < CLV_EMA_CHUNK ? left : CLV_EMA_CHUNK);
    CLV_GLOBAL uint32_t* __restrict__ p = global_ptr<uint32_t>(e.p + b.start);
    CLV_GLOBAL uint32_t* __restrict__ q = global_ptr<uint32_t>(e.ema + b.start);
    CLV_GLOBAL bf16_t* __restrict__ s = e.shadow ? global_ptr<bf16_t>(e.shadow + b.start) : nullptr;
    const bool vec = ((((uintptr_t)p) | ((uintptr_t)q)) & 15) == 0 && (((uintptr_t)s) & 7) == 0;
    if (vec) {
        const int n4 = cnt >> 2;
        CLV_GLOBAL u32x4v* p4 = (CLV_GLOBAL u32x4v*)p;
        CLV_GLOBAL u32x4v* q4 = (CLV_GLOBAL u32x4v*)q;
        for (int i = threadIdx.x; i < n4; i += 256) {
            const u32x4v pv = p4[i];
            const u32x4v ev = q4[i];
            p4[i] = ev;
            q4[i] = pv;
            if (s) {
                u32x2v o;
                o.x = pack2bf(__uint_as_float(ev.x), __uint_as_float(ev.y));
                o.y = pack2bf(__uint_as_float(ev.z), __uint_as_float(ev.w));
                ((CLV_GLOBAL u32x2v*)s)[i] = o;
            }
        }
        const int i = n4 * 4 + (int)threadIdx.x;
        if (i < cnt) {
            const uint32_t pv = p[i], ev = q[i];
            p[i] = ev;
            q[i] = pv;
            if (s) s[i] = f2bf(__uint_as_float(ev));
        }
    } else {
        for (int i = threadIdx.x; i < cnt; i += 256) {
            const uint32_t pv = p[i], ev = q[i];
            p[i] = ev;
            q[i] = pv;
            if (s) s[i] = f2bf(__uint_as_float(ev));
        }
    }
}

bool table_ok(const void* table, int32_t n_entries, int32_t n_blocks) {
    return table && n_entries >= 0 && n_blocks >= 0 && !(((uintptr_t)table) & 7) && (n_entries > 0 || n_blocks == 0);
}

}  // namespace

extern "C" int clv_ema_update(const void* table, int32_t n_entries, int32_t n_blocks, double momentum, void* stream) {
    if (!table_ok(table, n_entries, n_blocks) || !(momentum >= 0.0 && momentum <= 1.0)) return CLV_ERR_ARG;
    if (n_blocks == 0) return CLV_OK;
    const EmaUpdateEntry* entries = (const EmaUpdateEntry*)table;
    const EmaBlock* blocks = (const EmaBlock*)(entries + n_entries);
    // 1 - m in double, THEN to fp32: what buf.mul_(1 - momentum) multiplies by
    hipLaunchKernelGGL(ema_update_kernel, dim3((unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream, entries, blocks,
                       (float)momentum, (float)(1.0 - momentum));
    return clv_check_launch();
}

extern "C" int clv_ema_swap(const void* table, int32_t n_entries, int32_t n_blocks, void* stream) {
    if (!table_ok(table, n_entries, n_blocks)) return CLV_ERR_ARG;
    if (n_blocks == 0) return CLV_OK;
    const EmaSwapEntry* entries = (const EmaSwapEntry*)table;
    const EmaBlock* blocks = (const EmaBlock*)(entries + n_entries);
    hipLaunchKernelGGL(ema_swap_kernel, dim3((unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream, entries, blocks);
    return clv_check_launch();
}
