// Clip preparation: decoded uint8 frames -> the normalised clip tensor the recognizers take (include/clover_hip.h,
// "clip preparation").  One launch restates the reference's train / test image steps per output pixel:
//   RandomResizedCrop / CenterCrop (a box per sample) -> Resize(S, bilinear) -> Flip -> Normalize -> FormatShape('NCTHW_TSN')
// (mmaction/datasets/pipelines/augmentations.py, formating.py).  Memory bound: 1 byte per source channel in, 4 (or 2) bytes
// per output element out, ~20 flops per output pixel.  No LDS, no atomics, no cross-lane traffic.
//
// Work split: a workgroup owns a strip of output rows of ONE frame (b, t); a lane owns 8 adjacent output x in all three
// channel planes, so every store is a 16-byte vector (fp32: two per plane and row, 16-bit: one).  The eight x taps
// (two source columns and one weight each) are computed once per lane and reused for every row of the strip; the y taps
// once per row.  Source bytes are read with plain byte loads — the three channels of a pixel are adjacent, the lanes of a
// row walk the source row left to right, so a wave's loads of one tap fall into a few consecutive cache lines.
//
// Arithmetic of one output element, in THIS order (the exact test of tests/test_clip_prep_gpu.py restates it in torch):
//   xe = flip ? S - 1 - x : x
//   sx = clamp(fma(xe + 0.5f, (float)bw / (float)S, -0.5f), 0, bw - 1);  x0 = floor(sx), fx = sx - x0, x1 = min(x0 + 1, bw - 1)
//   (sy, y0, y1, fy likewise with bh)        — neighbours clamped to the CROP, then the crop's columns / rows to the frame
//   top = fma(p01 - p00, fx, p00);  bot = fma(p11 - p10, fx, p10);  v = fma(bot - top, fy, top)         (fp32)
//   out = (v - mean[c]) * inv_std[c]                                  (a subtract, then a multiply; rounded once on store)
// For a box of exactly S x S: sx = x, fx = 0 and v = p00 exactly, so out = ((float)u8 - mean[c]) * inv_std[c] bit for bit.
#include "common.hpp"
#include "../../include/clover_hip.h"

namespace {

constexpr int CP_BLOCK = 256;      // threads of a strip workgroup
constexpr int CP_PX = 8;           // adjacent output x per lane
constexpr int CP_PASSES = 2;       // row passes of a strip workgroup (x taps reused across them)

// What a shape launches: clv_clip_prep_plan reports it and clv_clip_prep takes its grid from it, so the two cannot drift.
bool clip_launch(int64_t frames, int S, ClvClipPrepPlan* o) {
    const int lpr = S / CP_PX;                         // lanes per output row
    o->lanes_per_row = lpr;
    if (lpr * S <= CP_BLOCK) {                         // the whole S x S plane in one pass of one workgroup (S <= 40)
        o->cls = CLV_CLIP_CLASS_PLANE;
        o->block = (lpr * S + 63) / 64 * 64;
        o->rows_per_pass = S;
        o->passes = 1;
        o->strips = 1;
        o->tail_rows = 0;
    } else {
        o->cls = CLV_CLIP_CLASS_STRIPS;
        o->block = CP_BLOCK;
        o->rows_per_pass = lpr <= CP_BLOCK ? CP_BLOCK / lpr : 0;
        if (o->rows_per_pass < 1) return false;        // S > 2048: a row does not fit one workgroup
        o->passes = CP_PASSES;
        const int rows = o->rows_per_pass * CP_PASSES;
        o->strips = (S + rows - 1) / rows;
        o->tail_rows = S % rows;                       // rows of the last strip when it is a partial one (0: none is)
    }
    o->idle_lanes = o->block - lpr * o->rows_per_pass;
    const int64_t grid = frames * o->strips;
    if (grid > 0x7fffffff) return false;
    o->grid = (int32_t)grid;
    return true;
}

struct Taps {
    int i0, i1;     // byte offsets of the two source pixels inside their row (x) / row indices (y)
    float f;
};

// The two taps and the weight of output index `i` over a crop of `n` source pixels starting at `lo`, inside a frame of
// `lim` pixels.  `n` >= 1; the returned indices lie in [0, lim - 1] whatever the box says.
__device__ __forceinline__ Taps taps_of(int i, float scale, int lo, int n, int lim) {
    float s = fmaf((float)i + 0.5f, scale, -0.5f);
    s = fminf(fmaxf(s, 0.f), (float)(n - 1));
    const float fl = floorf(s);
    const int a = (int)fl;
    const int b = min(a + 1, n - 1);
    Taps t;
    t.i0 = min(max(lo + a, 0), lim - 1);
    t.i1 = min(max(lo + b, 0), lim - 1);
    t.f = s - fl;
    return t;
}

template <bool HALF>
__global__ void __launch_bounds__(CP_BLOCK)
clip_prep_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ boxes, const uint8_t* __restrict__ flips,
                 const float* __restrict__ mean, const float* __restrict__ inv_std, void* __restrict__ out,
                 int T, int Hs, int Ws, int S, int lpr, int rows_per_pass, int passes, int strips) {
    const int strip = blockIdx.x % strips;
    const int frame = blockIdx.x / strips;             // b * T + t
    const int b = frame / T, t = frame - b * T;
    const int xg = threadIdx.x % lpr;
    const int rlane = threadIdx.x / lpr;
    if (rlane >= rows_per_pass) return;                // the idle lanes behind the last whole row

    // the box, made safe: inside the frame and at least one pixel each way (the binding refuses such boxes; this keeps a
    // bad one from reading outside src)
    const int left = min(max(boxes[b * 4 + 0], 0), Ws - 1), top = min(max(boxes[b * 4 + 1], 0), Hs - 1);
    const int bw = min(max(boxes[b * 4 + 2], left + 1), Ws) - left, bh = min(max(boxes[b * 4 + 3], top + 1), Hs) - top;
    const bool flip = flips[b] != 0;
    const float xscale = (float)bw / (float)S, yscale = (float)bh / (float)S;

    int c0[CP_PX], c1[CP_PX];
    float fx[CP_PX];
#pragma unroll
    for (int j = 0; j < CP_PX; ++j) {
        const int x = xg * CP_PX + j;
        const Taps tx = taps_of(flip ? S - 1 - x : x, xscale, left, bw, Ws);
        c0[j] = tx.i0 * 3;
        c1[j] = tx.i1 * 3;
        fx[j] = tx.f;
    }
    const float m0 = mean[0], m1 = mean[1], m2 = mean[2];
    const float s0 = inv_std[0], s1 = inv_std[1], s2 = inv_std[2];
    const uint8_t* fsrc = src + (int64_t)frame * Hs * Ws * 3;
    const int64_t plane = (int64_t)S * S;
    const int64_t obase = ((int64_t)b * 3 * T + t) * plane;          // channel c adds c * T * plane

    for (int p = 0; p < passes; ++p) {
        const int y = (strip * passes + p) * rows_per_pass + rlane;
        if (y >= S) return;
        const Taps ty = taps_of(y, yscale, top, bh, Hs);
        const uint8_t* r0 = fsrc + (int64_t)ty.i0 * Ws * 3;
        const uint8_t* r1 = fsrc + (int64_t)ty.i1 * Ws * 3;
        float v[3][CP_PX];
#pragma unroll
        for (int j = 0; j < CP_PX; ++j) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float p00 = (float)r0[c0[j] + c], p01 = (float)r0[c1[j] + c];
                const float p10 = (float)r1[c0[j] + c], p11 = (float)r1[c1[j] + c];
                const float tp = fmaf(p01 - p00, fx[j], p00);
                const float bt = fmaf(p11 - p10, fx[j], p10);
                const float val = fmaf(bt - tp, ty.f, tp);
                v[c][j] = (val - (c == 0 ? m0 : c == 1 ? m1 : m2)) * (c == 0 ? s0 : c == 1 ? s1 : s2);
            }
        }
        const int64_t o = obase + (int64_t)y * S + xg * CP_PX;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int64_t oc = o + (int64_t)c * T * plane;
            if (HALF) {
                uint4 w = make_uint4(pack2bf(v[c][0], v[c][1]), pack2bf(v[c][2], v[c][3]), pack2bf(v[c][4], v[c][5]),
                                     pack2bf(v[c][6], v[c][7]));
                *reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(out) + oc) = w;
            } else {
                float4* dst = reinterpret_cast<float4*>(reinterpret_cast<float*>(out) + oc);
                dst[0] = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
                dst[1] = make_float4(v[c][4], v[c][5], v[c][6], v[c][7]);
            }
        }
    }
}

}  // namespace

extern "C" int clv_clip_prep_supported(int32_t C, int32_t Hs, int32_t Ws, int32_t S, int32_t box_w, int32_t box_h) {
    if (C != 3) return CLV_CLIP_BAD_CHANNELS;
    if (Hs < 1 || Ws < 1) return CLV_CLIP_BAD_FRAME;
    if (S < 8 || S % 8 != 0 || S > 2048) return CLV_CLIP_BAD_SIZE;
    if (box_w < 1 || box_w > Ws || box_h < 1 || box_h > Hs) return CLV_CLIP_BAD_BOX;
    return 0;
}

extern "C" int clv_clip_prep_plan(const ClvClipPrepGeom* g, ClvClipPrepPlan* out) {
    if (!g || !out || g->B < 1 || g->T < 1) return CLV_ERR_ARG;
    if (g->out_dtype != CLV_CLIP_OUT_F32 && g->out_dtype != CLV_CLIP_OUT_HALF) return CLV_ERR_ARG;
    if (clv_clip_prep_supported(g->C, g->Hs, g->Ws, g->S, 1, 1) != 0) return CLV_ERR_UNSUPPORTED;
    return clip_launch((int64_t)g->B * g->T, g->S, out) ? CLV_OK : CLV_ERR_UNSUPPORTED;
}

extern "C" int clv_clip_prep(const uint8_t* src, const int32_t* boxes, const uint8_t* flips, const float* mean,
                             const float* inv_std, void* out, const ClvClipPrepGeom* g, void* stream) {
    if (!src || !boxes || !flips || !mean || !inv_std || !out || !g) return CLV_ERR_ARG;
    if ((((uintptr_t)out) & 15) || (((uintptr_t)boxes) & 3)) return CLV_ERR_ARG;
    ClvClipPrepPlan pl;
    const int rc = clv_clip_prep_plan(g, &pl);
    if (rc != CLV_OK) return rc;
    if (g->boxes_host) {                               // the caller's host copy of `boxes`: checked here, without a sync
        for (int b = 0; b < g->B; ++b) {
            const int32_t* q = g->boxes_host + 4 * b;
            if (q[0] < 0 || q[1] < 0 || q[2] > g->Ws || q[3] > g->Hs) return CLV_ERR_ARG;
            if (clv_clip_prep_supported(g->C, g->Hs, g->Ws, g->S, q[2] - q[0], q[3] - q[1]) != 0) return CLV_ERR_UNSUPPORTED;
        }
    }
    auto kernel = g->out_dtype == CLV_CLIP_OUT_HALF ? clip_prep_kernel<true> : clip_prep_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(pl.grid), dim3(pl.block), 0, (hipStream_t)stream, src, boxes, flips, mean, inv_std, out,
                       g->T, g->Hs, g->Ws, g->S, pl.lanes_per_row, pl.rows_per_pass, pl.passes, pl.strips);
    return clv_check_launch();
}
