// PatchEmbed3D (conv3d as an MFMA GEMM over patches gathered straight from the fp32 [B,3,T,H,W] clip) fused with
// bias + LayerNorm(C) + the SimMIM-style mask-token blend, writing channels-last bf16 tokens for the clean and the
// masked pass from ONE read of the clip.  Two GEMM front ends feed one epilogue (pe_epilogue):
//
// patch = stride = (2,4,4), patch_embed_fwd_kernel: K = 3*2*4*4 = 96 is walked as 3 MFMA k-steps (one per input
// channel): inside a k-step the lane group g = lane>>4 owns (dt, dy-pair) = (g>>1, g&1) and its 8 k-values are two
// float4 rows of the clip, so a wave's A-operand load is 16 consecutive tokens x 16 B = 256 B contiguous per lane group
// (coalesced [B,3,T,H,W] reads).  The C x 96 weight lives in registers as B-operand fragments for the whole grid-stride
// loop.
//
// Any patch size and stride of the supported set (clv_patch_embed_gen_supported), patch_embed_gen_fwd_kernel:
// K = 3*pt*ph*pw (<= 384) in the weight's own column order (c, dt, dy, dx), walked in k-steps of 32 with the last step
// zero-filled.  Lane l of a wave holds token row l & 15 and k = 8 (l >> 4) + j of the step.  What keeps the gather
// general is a per-k offset table in LDS (c*T*H*W + dt*H*W + dy*W + dx) plus one base offset per token
// (b*3*T*H*W + t'*st*H*W + h'*sh*W + w'*sw): a lane's 8 k-values are two float4 loads where pw, sw and W are multiples of
// 4 (4 consecutive k are then 16 aligned bytes of one clip row), 8 scalar loads elsewhere.  The C x K weight sits in LDS
// as 16-bit B-operand rows (128 x 392 x 2 B = 98 KB at the largest; with the output tiles 150.5 KB of LDS, one workgroup
// per CU) for the whole grid-stride loop.  K = 96, the (2,4,4) geometry, runs the same three k-steps over the same k
// order as the register-weight kernel: bit-identical.
#include "common.hpp"
#include "../../include/clover_hip.h"

namespace {

constexpr int PE_THREADS = 256;
constexpr int PE_WAVES = PE_THREADS / 64;
constexpr int PG_KMAX = 384;

struct PEGrid {
    int B, Tp, Hp, Wp;     // token grid
    int mh, mw, ch, cw;    // mask grid and cell size (Hp/mh, Wp/mw)
    int64_t M;             // tokens
};

struct PEShape {
    PEGrid G;
    int T, H, W;           // input clip dims (T even, H,W multiples of 4)
};

struct PGShape {
    PEGrid G;                  // (T - pt) / st + 1, ...
    int T, H, W;               // clip dims
    int pt, ph, pw, st, sh, sw;
    int K, KS;                 // 3*pt*ph*pw and its k-steps of 32
    int vec;                   // 4 consecutive k are 16 aligned bytes of the clip
};

__device__ __forceinline__ void tok_coords(const PEGrid& G, int64_t m, int& b, int& tp, int& hp, int& wp) {
    wp = (int)(m % G.Wp);
    int64_t r = m / G.Wp;
    hp = (int)(r % G.Hp);
    r /= G.Hp;
    tp = (int)(r % G.Tp);
    b = (int)(r / G.Tp);
}

// 1 where the video mask [B][mh][mw] covers token m
__device__ __forceinline__ int64_t tok_mask(const PEGrid& G, const int64_t* __restrict__ vmask, int64_t m) {
    int b, tp, hp, wp;
    tok_coords(G, m, b, tp, hp, wp);
    return vmask[((int64_t)b * G.mh + hp / G.ch) * G.mw + wp / G.cw];
}

bool make_grid(PEGrid& G, int B, int Tp, int Hp, int Wp, int mh, int mw) {
    if (B <= 0 || Tp <= 0 || Hp <= 0 || Wp <= 0) return false;
    G.B = B; G.Tp = Tp; G.Hp = Hp; G.Wp = Wp;
    G.M = (int64_t)B * Tp * Hp * Wp;
    G.mh = mh > 0 ? mh : 1;
    G.mw = mw > 0 ? mw : 1;
    if (Hp % G.mh || Wp % G.mw) return false;
    G.ch = Hp / G.mh;
    G.cw = Wp / G.mw;
    return true;
}

// ------------------------------------------------------------------ the shared tail of the forward kernels
// a lane's NT = C/16 entries of bias / gamma / beta / mask_token: column n = nt*16 + lr
template <int NT>
__device__ __forceinline__ void lane_params(const float* __restrict__ bias, const float* __restrict__ gamma,
                                            const float* __restrict__ beta, const float* __restrict__ mask_token,
                                            bool blend, int lr, float (&bi)[NT], float (&ga)[NT], float (&be)[NT],
                                            float (&mt)[NT]) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        bi[nt] = bias[nt * 16 + lr];
        ga[nt] = gamma ? gamma[nt * 16 + lr] : 1.f;
        be[nt] = beta ? beta[nt * 16 + lr] : 0.f;
        mt[nt] = (blend && mask_token) ? mask_token[nt * 16 + lr] : 0.f;
    }
}

// acc[nt][r] = z[token m0 + lg*4 + r][n = nt*16 + lr]  (before bias) -> bias, LayerNorm (norm), the mask-token blend,
// mean / rstd, and the wave's 16 rows of out_clean / out_masked / z_out through its three wave-private LDS tiles
// (16 x (C + 8) elements each).
template <int C>
__device__ __forceinline__ void pe_epilogue(const f32x4_t (&acc)[C / 16], const float (&bi)[C / 16],
                                            const float (&ga)[C / 16], const float (&be)[C / 16],
                                            const float (&mt)[C / 16], bool norm, const int64_t* __restrict__ vmask,
                                            bf16_t* __restrict__ out_clean, bf16_t* __restrict__ out_masked,
                                            bf16_t* __restrict__ z_out, float* __restrict__ mean,
                                            float* __restrict__ rstd, const PEGrid& G, float eps, int64_t m0,
                                            bf16_t* tile0, bf16_t* tile1, bf16_t* tile2, int lane, int lg, int lr) {
    constexpr int NT = C / 16, LDO = C + 8;
    const float invC = 1.0f / (float)C;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t m = m0 + lg * 4 + r;
        float zs[NT], sum = 0.f;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            zs[nt] = acc[nt][r] + bi[nt];
            sum += zs[nt];
        }
        float mu = 0.f, rs = 1.f;
        if (norm) {
            mu = row16_sum(sum) * invC;
            float vs = 0.f;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) vs += (zs[nt] - mu) * (zs[nt] - mu);
            rs = rsqrtf(row16_sum(vs) * invC + eps);
        }
        float wgt = 0.f;
        if (out_masked && m < G.M) wgt = (float)tok_mask(G, vmask, m);
        if (m < G.M && lr == 0) {
            if (mean) mean[m] = mu;
            if (rstd) rstd[m] = rs;
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const float yv = norm ? (zs[nt] - mu) * rs * ga[nt] + be[nt] : zs[nt];
            const int off = (lg * 4 + r) * LDO + nt * 16 + lr;
            tile0[off] = f2bf(yv);
            tile1[off] = f2bf(yv * (1.f - wgt) + mt[nt] * wgt);
            tile2[off] = f2bf(zs[nt]);
        }
    }
    // the wave's own tile: write full rows, 16 B per lane  (wave-private LDS, no block barrier)
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
    __builtin_amdgcn_wave_barrier();
    constexpr int CH = C / 8;
    for (int idx = lane; idx < 16 * CH; idx += 64) {
        const int tr = idx / CH, c8 = idx - tr * CH;
        const int64_t m = m0 + tr;
        if (m < G.M) {
            if (out_clean)
                *reinterpret_cast<uint4*>(out_clean + m * C + c8 * 8) =
                    *reinterpret_cast<const uint4*>(&tile0[tr * LDO + c8 * 8]);
            if (out_masked)
                *reinterpret_cast<uint4*>(out_masked + m * C + c8 * 8) =
                    *reinterpret_cast<const uint4*>(&tile1[tr * LDO + c8 * 8]);
            if (z_out)
                *reinterpret_cast<uint4*>(z_out + m * C + c8 * 8) =
                    *reinterpret_cast<const uint4*>(&tile2[tr * LDO + c8 * 8]);
        }
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
}

// ------------------------------------------------------------------ (2,4,4 | 2,4,4): weights in registers
// A-operand fragment (8 k-values of channel c) of token m for lane group g.
__device__ __forceinline__ Frag8 patch_frag(const float* __restrict__ x, const PEShape& S, int64_t m, bool valid,
                                            int c, int g) {
    Frag8 f;
    if (!valid) {
        f.u4 = make_uint4(0, 0, 0, 0);
        return f;
    }
    int b, tp, hp, wp;
    tok_coords(S.G, m, b, tp, hp, wp);
    const int t = 2 * tp + (g >> 1), y = 4 * hp + 2 * (g & 1);
    const float* p = x + ((((int64_t)b * 3 + c) * S.T + t) * S.H + y) * S.W + 4 * wp;
    const float4 r0 = *reinterpret_cast<const float4*>(p);
    const float4 r1 = *reinterpret_cast<const float4*>(p + S.W);
    f.u[0] = pack2bf(r0.x, r0.y);
    f.u[1] = pack2bf(r0.z, r0.w);
    f.u[2] = pack2bf(r1.x, r1.y);
    f.u[3] = pack2bf(r1.z, r1.w);
    return f;
}

// fp8 variant (BASELINE config 5, "fp8 MFMA ... patch-proj path"): the same 8 k-values per lane, kept in fp32 until the
// token's 96 patch values are all in hand (its row maximum sits in the 4 lane groups x 3 channel steps of lane lr), then
// scaled by 448 / max and converted to OCP e4m3; the product runs on v_mfma_f32_16x16x32_fp8_fp8 (same lane -> k map as
// the bf16 instruction, 8 bytes per lane) and is rescaled by row scale x per-output-channel weight scale afterwards.
__device__ __forceinline__ void patch_frag_f32(const float* __restrict__ x, const PEShape& S, int64_t m, bool valid, int c,
                                               int g, float (&v)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0.f;
    if (!valid) return;
    int b, tp, hp, wp;
    tok_coords(S.G, m, b, tp, hp, wp);
    const int t = 2 * tp + (g >> 1), y = 4 * hp + 2 * (g & 1);
    const float* p = x + ((((int64_t)b * 3 + c) * S.T + t) * S.H + y) * S.W + 4 * wp;
    const float4 r0 = *reinterpret_cast<const float4*>(p);
    const float4 r1 = *reinterpret_cast<const float4*>(p + S.W);
    v[0] = r0.x; v[1] = r0.y; v[2] = r0.z; v[3] = r0.w; v[4] = r1.x; v[5] = r1.y; v[6] = r1.z; v[7] = r1.w;
}
__device__ __forceinline__ long pack8_fp8(const float (&v)[8], float inv) {
    int lo = 0, hi = 0;
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(v[0] * inv, v[1] * inv, lo, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(v[2] * inv, v[3] * inv, lo, true);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(v[4] * inv, v[5] * inv, hi, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(v[6] * inv, v[7] * inv, hi, true);
    return (long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

template <int C, bool FP8 = false>
__global__ void __launch_bounds__(PE_THREADS) patch_embed_fwd_kernel(
    const float* __restrict__ x, const bf16_t* __restrict__ w, const float* __restrict__ bias,
    const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ mask_token,
    const int64_t* __restrict__ vmask, bf16_t* __restrict__ out_clean, bf16_t* __restrict__ out_masked,
    bf16_t* __restrict__ z_out, float* __restrict__ mean, float* __restrict__ rstd, PEShape S, float eps,
    const unsigned char* __restrict__ w8 = nullptr, const float* __restrict__ wscale = nullptr) {
    constexpr int NT = C / 16, LDO = C + 8;
    __shared__ __attribute__((aligned(16))) bf16_t tile[PE_WAVES][3][16 * LDO];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lg = lane >> 4, lr = lane & 15;
    // weight fragments: B[k = s*32 + lg*8 + j][n = nt*16 + lr] = W[n][k]
    Frag8 wf[3][NT];
    long wf8[3][NT];
    float ws[NT];
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            if constexpr (FP8) wf8[s][nt] = *reinterpret_cast<const long*>(w8 + (nt * 16 + lr) * 96 + s * 32 + lg * 8);
            else wf[s][nt].u4 = *reinterpret_cast<const uint4*>(w + (nt * 16 + lr) * 96 + s * 32 + lg * 8);
        }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) ws[nt] = FP8 ? wscale[nt * 16 + lr] : 1.f;
    float bi[NT], ga[NT], be[NT], mt[NT];
    lane_params<NT>(bias, gamma, beta, mask_token, out_masked != nullptr, lr, bi, ga, be, mt);
    const int64_t ntiles = (S.G.M + 15) / 16;
    const int64_t wave = (int64_t)blockIdx.x * PE_WAVES + wv, nwaves = (int64_t)gridDim.x * PE_WAVES;
    for (int64_t tileid = wave; tileid < ntiles; tileid += nwaves) {
        const int64_t m0 = tileid * 16;
        f32x4_t acc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
        if constexpr (FP8) {
            float pv[3][8], amax = 0.f;
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                patch_frag_f32(x, S, m0 + lr, m0 + lr < S.G.M, s, lg, pv[s]);
#pragma unroll
                for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(pv[s][e]));
            }
            amax = grp4_max(amax);                               // the token's 96 values: 4 lane groups x 3 steps
            const float inv = amax > 0.f ? 448.0f / amax : 1.0f, rsc = amax > 0.f ? amax * (1.0f / 448.0f) : 1.0f;
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const long a8 = pack8_fp8(pv[s], inv);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a8, wf8[s][nt], acc[nt], 0, 0, 0);
            }
            // acc[nt][r] belongs to token m0 + lg*4 + r: its row scale lives in the lanes with lr = lg*4 + r
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float sr = __shfl(rsc, lg * 4 + r, 64);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[nt][r] *= sr * ws[nt];
            }
        } else {
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const Frag8 a = patch_frag(x, S, m0 + lr, m0 + lr < S.G.M, s, lg);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[nt] = mfma16(a, wf[s][nt], acc[nt]);
            }
        }
        pe_epilogue<C>(acc, bi, ga, be, mt, gamma != nullptr, vmask, out_clean, out_masked, z_out, mean, rstd, S.G, eps, m0,
                       &tile[wv][0][0], &tile[wv][1][0], &tile[wv][2][0], lane, lg, lr);
    }
}

// ------------------------------------------------------------------ any geometry: weight and offset table in LDS
// offset of patch element k = ((c*pt + dt)*ph + dy)*pw + dx from its token's first clip element (fits int: make_shape)
__device__ __forceinline__ int k_offset(const PGShape& S, int k) {
    const int dx = k % S.pw;
    int r = k / S.pw;
    const int dy = r % S.ph;
    r /= S.ph;
    const int dt = r % S.pt, c = r / S.pt;
    return ((c * S.T + dt) * S.H + dy) * S.W + dx;
}

// first clip element of token m: channel 0, (t'*st, h'*sh, w'*sw)
__device__ __forceinline__ int64_t tok_base(const PGShape& S, int64_t m) {
    int b, tp, hp, wp;
    tok_coords(S.G, m, b, tp, hp, wp);
    return ((((int64_t)b * 3 * S.T + tp * S.st) * S.H + hp * S.sh) * S.W) + wp * S.sw;
}

__device__ __forceinline__ uint4 pack8(const float (&v)[8]) {
    return make_uint4(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7]));
}

// the 8 patch values k0 .. k0+7 (k0 % 8 == 0; K % 8 == 0, so the group is inside K or wholly beyond it) of the token at xb
template <class OffsetOf>
__device__ __forceinline__ uint4 gather8(const float* __restrict__ xb, const PGShape& S, int k0, bool valid, OffsetOf off) {
    if (!valid || k0 >= S.K) return make_uint4(0, 0, 0, 0);
    float v[8];
    if (S.vec) {
        const float4 r0 = *reinterpret_cast<const float4*>(xb + off(k0));
        const float4 r1 = *reinterpret_cast<const float4*>(xb + off(k0 + 4));
        v[0] = r0.x; v[1] = r0.y; v[2] = r0.z; v[3] = r0.w; v[4] = r1.x; v[5] = r1.y; v[6] = r1.z; v[7] = r1.w;
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = xb[off(k0 + j)];
    }
    return pack8(v);
}

__host__ __device__ constexpr int pg_kp(int KS) { return KS * 32 + 8; }                 // weight row stride in LDS (elements)
__host__ __device__ constexpr int pg_lds_bytes(int C, int KS) {
    return KS * 32 * 4 + C * pg_kp(KS) * 2 + PE_WAVES * 3 * 16 * (C + 8) * 2;           // offsets, weight, output tiles
}

template <int C>
__global__ void __launch_bounds__(PE_THREADS) patch_embed_gen_fwd_kernel(
    const float* __restrict__ x, const bf16_t* __restrict__ w, const float* __restrict__ bias,
    const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ mask_token,
    const int64_t* __restrict__ vmask, bf16_t* __restrict__ out_clean, bf16_t* __restrict__ out_masked,
    bf16_t* __restrict__ z_out, float* __restrict__ mean, float* __restrict__ rstd, PGShape S, float eps) {
    constexpr int NT = C / 16, LDO = C + 8;
    extern __shared__ __attribute__((aligned(16))) unsigned char pg_smem[];
    const int KP = pg_kp(S.KS);
    int* koff = reinterpret_cast<int*>(pg_smem);                                         // [KS*32]
    bf16_t* wl = reinterpret_cast<bf16_t*>(pg_smem + S.KS * 32 * 4);                     // [C][KP], columns >= K zero
    bf16_t* tiles = wl + C * KP;                                                         // [PE_WAVES][3][16*LDO]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lg = lane >> 4, lr = lane & 15;
    for (int k = threadIdx.x; k < S.KS * 32; k += PE_THREADS) koff[k] = k < S.K ? k_offset(S, k) : 0;
    const int kc = S.KS * 4;                                                             // 16-byte chunks per weight row
    for (int i = threadIdx.x; i < C * kc; i += PE_THREADS) {
        const int n = i / kc, k = (i - n * kc) * 8;
        *reinterpret_cast<uint4*>(wl + n * KP + k) =
            k < S.K ? *reinterpret_cast<const uint4*>(w + n * S.K + k) : make_uint4(0, 0, 0, 0);
    }
    __syncthreads();
    bf16_t* tile0 = tiles + (wv * 3 + 0) * 16 * LDO;
    bf16_t* tile1 = tiles + (wv * 3 + 1) * 16 * LDO;
    bf16_t* tile2 = tiles + (wv * 3 + 2) * 16 * LDO;
    float bi[NT], ga[NT], be[NT], mt[NT];
    lane_params<NT>(bias, gamma, beta, mask_token, out_masked != nullptr, lr, bi, ga, be, mt);
    const int64_t ntiles = (S.G.M + 15) / 16;
    const int64_t wave = (int64_t)blockIdx.x * PE_WAVES + wv, nwaves = (int64_t)gridDim.x * PE_WAVES;
    for (int64_t tileid = wave; tileid < ntiles; tileid += nwaves) {
        const int64_t m0 = tileid * 16;
        const bool valid = m0 + lr < S.G.M;
        const float* xb = x + (valid ? tok_base(S, m0 + lr) : 0);
        f32x4_t acc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < S.KS; ++s) {
            Frag8 a;
            a.u4 = gather8(xb, S, s * 32 + lg * 8, valid, [&](int k) { return koff[k]; });
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                Frag8 b;
                b.u4 = *reinterpret_cast<const uint4*>(wl + (nt * 16 + lr) * KP + s * 32 + lg * 8);
                acc[nt] = mfma16(a, b, acc[nt]);
            }
        }
        pe_epilogue<C>(acc, bi, ga, be, mt, gamma != nullptr, vmask, out_clean, out_masked, z_out, mean, rstd, S.G, eps, m0,
                       tile0, tile1, tile2, lane, lg, lr);
    }
}

// ------------------------------------------------------------------ backward
// im2col of the clip into 16-bit patches [M][K], k in the weight's column order (c, dt, dy, dx), the operand of the
// weight-gradient GEMM dW = dZᵀ · patches: one thread = 8 consecutive k of a token.
__global__ void __launch_bounds__(256) im2col_kernel(const float* __restrict__ x, bf16_t* __restrict__ patches,
                                                     PGShape S) {
    const int k8 = S.K / 8;
    const int64_t total = S.G.M * k8;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t m = i / k8;
        const int k0 = (int)(i - m * k8) * 8;
        *reinterpret_cast<uint4*>(patches + m * S.K + k0) =
            gather8(x + tok_base(S, m), S, k0, true, [&](int k) { return k_offset(S, k); });
    }
}

// Backward of the mask-token blend (swin_transformer_3d.py:222-230): out_masked = y (1 - w) + mask_token w and
// out_clean = y, so  dy = d_clean + d_masked (1 - w)  and  d mask_token = sum over tokens of d_masked w
// (w in {0,1} per token, from the [B][mh][mw] video mask).  One pass: each thread owns 8 channels of a row
// stripe; the mask-token sum is folded per block through LDS and added with one atomic per channel.
template <int CV>
__global__ void __launch_bounds__(256) blend_bwd_kernel(const bf16_t* __restrict__ dclean,
                                                        const bf16_t* __restrict__ dmasked,
                                                        const int64_t* __restrict__ vmask, bf16_t* __restrict__ dy,
                                                        float* __restrict__ dmt, PEGrid G) {
    constexpr int CH = CV / 8;                    // 16-byte chunks per row
    constexpr int RPB = 256 / CH;                 // rows per block pass
    __shared__ float red[RPB][CV];
    const int t = threadIdx.x, rl = t / CH, ck = t - rl * CH;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    if (rl < RPB) {
        for (int64_t m = (int64_t)blockIdx.x * RPB + rl; m < G.M; m += (int64_t)gridDim.x * RPB) {
            const bool masked = dmasked && tok_mask(G, vmask, m) != 0;
            Frag8 c, d, o;
            c.u4 = dclean ? *reinterpret_cast<const uint4*>(dclean + m * CV + ck * 8) : make_uint4(0, 0, 0, 0);
            d.u4 = dmasked ? *reinterpret_cast<const uint4*>(dmasked + m * CV + ck * 8) : make_uint4(0, 0, 0, 0);
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float dm = bf2f(d.h[e]);
                v[e] = bf2f(c.h[e]) + (masked ? 0.f : dm);
                if (masked) acc[e] += dm;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) o.u[e] = pack2bf(v[2 * e], v[2 * e + 1]);
            *reinterpret_cast<uint4*>(dy + m * CV + ck * 8) = o.u4;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) red[rl][ck * 8 + e] = acc[e];
    }
    __syncthreads();
    if (dmt && t < CV) {
        float sum = 0.f;
        for (int r = 0; r < RPB; ++r) sum += red[r][t];
        if (sum != 0.f) atomicAdd(dmt + t, sum);
    }
}

// ------------------------------------------------------------------ host side
// what every forward entry refuses with CLV_ERR_ARG before it looks at the geometry
bool fwd_args_ok(const float* x, const void* w, const float* bias, const float* gamma, const float* beta,
                 const float* mask_token, const int64_t* vmask, const void* out_clean, const void* out_masked) {
    if (!x || !w || !bias || (!out_clean && !out_masked)) return false;
    if ((gamma == nullptr) != (beta == nullptr)) return false;
    return !out_masked || (vmask && mask_token);
}

// the register-weight kernels' clip: T even, H and W multiples of 4 (their float4 loads rest on it)
bool make_shape(PEShape& S, int B, int T, int H, int W, int mh, int mw) {
    if (T <= 0 || H <= 0 || W <= 0 || (T & 1) || (H & 3) || (W & 3)) return false;
    S.T = T; S.H = H; S.W = W;
    return make_grid(S.G, B, T / 2, H / 4, W / 4, mh, mw);
}

int pe_fwd_grid(const PEShape& S) {
    const int64_t ntiles = (S.G.M + 15) / 16, grid = (ntiles + PE_WAVES - 1) / PE_WAVES;
    return (int)(grid > 1024 ? 1024 : grid);
}

bool make_shape(PGShape& S, const float* x, int B, int T, int H, int W, int pt, int ph, int pw, int st, int sh, int sw,
                int C, int mh, int mw) {
    if (clv_patch_embed_gen_supported(pt, ph, pw, st, sh, sw, C) != 0) return false;
    if (B <= 0 || T < pt || H < ph || W < pw) return false;
    if ((int64_t)3 * T * H * W > INT32_MAX) return false;           // the per-k offsets are 32-bit
    S.T = T; S.H = H; S.W = W;
    S.pt = pt; S.ph = ph; S.pw = pw; S.st = st; S.sh = sh; S.sw = sw;
    S.K = 3 * pt * ph * pw;
    S.KS = (S.K + 31) / 32;
    S.vec = (pw % 4 == 0 && sw % 4 == 0 && W % 4 == 0 && ((uintptr_t)x & 15) == 0) ? 1 : 0;
    return make_grid(S.G, B, (T - pt) / st + 1, (H - ph) / sh + 1, (W - pw) / sw + 1, mh, mw);
}

template <int C>
int launch_gen_fwd(const float* x, const void* w, const float* bias, const float* gamma, const float* beta,
                   const float* mask_token, const int64_t* vmask, void* out_clean, void* out_masked, void* z_out,
                   float* mean, float* rstd, const PGShape& S, float eps, hipStream_t st) {
    // dynamic LDS = offsets + weight + the four waves' output tiles (pg_lds_bytes), and the total bounds occupancy: C = 128
    // 52 224 B of tiles alone, above 64 KB from K > 32 on, 154 112 B at K = 384 (one workgroup per CU); C = 96 above 64 KB
    // from K > 96 on, 116 736 B at K = 384; C = 48 at most 60 672 B.  Opted into once per process, for the largest K
    static const bool attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&patch_embed_gen_fwd_kernel<C>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 pg_lds_bytes(C, PG_KMAX / 32)) == hipSuccess;
    if (!attr) return CLV_ERR_LAUNCH;
    const int64_t ntiles = (S.G.M + 15) / 16;
    int grid = (int)((ntiles + PE_WAVES - 1) / PE_WAVES);
    if (grid > 512) grid = 512;                                     // every workgroup stages the weight once
    hipLaunchKernelGGL((patch_embed_gen_fwd_kernel<C>), dim3(grid), dim3(PE_THREADS), (size_t)pg_lds_bytes(C, S.KS), st, x,
                       (const bf16_t*)w, bias, gamma, beta, mask_token, vmask, (bf16_t*)out_clean, (bf16_t*)out_masked,
                       (bf16_t*)z_out, mean, rstd, S, eps);
    return clv_check_launch();
}

}  // namespace

extern "C" int clv_patch_embed_fwd(const float* x, const void* w, const float* bias, const float* gamma,
                                   const float* beta, const float* mask_token, const int64_t* vmask,
                                   void* out_clean, void* out_masked, void* z_out, float* mean, float* rstd,
                                   int32_t B, int32_t T, int32_t H, int32_t W, int32_t C, int32_t mh, int32_t mw,
                                   float eps, void* stream) {
    PEShape S;
    if (!fwd_args_ok(x, w, bias, gamma, beta, mask_token, vmask, out_clean, out_masked)) return CLV_ERR_ARG;
    if (!make_shape(S, B, T, H, W, out_masked ? mh : 1, out_masked ? mw : 1)) return CLV_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int grid = pe_fwd_grid(S);
#define PE_LAUNCH(CV)                                                                                          \
    hipLaunchKernelGGL((patch_embed_fwd_kernel<CV>), dim3(grid), dim3(PE_THREADS), 0, st, x, (const bf16_t*)w, \
                       bias, gamma, beta, mask_token, vmask, (bf16_t*)out_clean, (bf16_t*)out_masked,          \
                       (bf16_t*)z_out, mean, rstd, S, eps)
    switch (C) {
        case 48: PE_LAUNCH(48); break;
        case 96: PE_LAUNCH(96); break;
        case 128: PE_LAUNCH(128); break;
        default: return CLV_ERR_UNSUPPORTED;
    }
#undef PE_LAUNCH
    return clv_check_launch();
}

extern "C" int clv_patch_embed_fwd_fp8(const float* x, const void* w8, const float* wscale, const float* bias,
                                       const float* gamma, const float* beta, const float* mask_token,
                                       const int64_t* vmask, void* out_clean, void* out_masked, void* z_out, float* mean,
                                       float* rstd, int32_t B, int32_t T, int32_t H, int32_t W, int32_t C, int32_t mh,
                                       int32_t mw, float eps, void* stream) {
    PEShape S;
    if (!wscale || !fwd_args_ok(x, w8, bias, gamma, beta, mask_token, vmask, out_clean, out_masked)) return CLV_ERR_ARG;
    if (!make_shape(S, B, T, H, W, out_masked ? mh : 1, out_masked ? mw : 1)) return CLV_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int grid = pe_fwd_grid(S);
#define PE_LAUNCH8(CV)                                                                                              \
    hipLaunchKernelGGL((patch_embed_fwd_kernel<CV, true>), dim3(grid), dim3(PE_THREADS), 0, st, x, (const bf16_t*)nullptr, \
                       bias, gamma, beta, mask_token, vmask, (bf16_t*)out_clean, (bf16_t*)out_masked,              \
                       (bf16_t*)z_out, mean, rstd, S, eps, (const unsigned char*)w8, wscale)
    switch (C) {
        case 48: PE_LAUNCH8(48); break;
        case 96: PE_LAUNCH8(96); break;
        case 128: PE_LAUNCH8(128); break;
        default: return CLV_ERR_UNSUPPORTED;
    }
#undef PE_LAUNCH8
    return clv_check_launch();
}

extern "C" int clv_patch_embed_gen_supported(int32_t pt, int32_t ph, int32_t pw, int32_t st, int32_t sh, int32_t sw,
                                             int32_t C) {
    if (pt < 1 || ph < 1 || pw < 1) return CLV_PE_GEN_BAD_PATCH;
    if (st < 1 || sh < 1 || sw < 1 || st > pt || sh > ph || sw > pw) return CLV_PE_GEN_BAD_STRIDE;
    if ((int64_t)pt * ph * pw % 8 != 0) return CLV_PE_GEN_BAD_VOLUME;
    if ((int64_t)3 * pt * ph * pw > PG_KMAX) return CLV_PE_GEN_BAD_K;
    if (C != 48 && C != 96 && C != 128) return CLV_PE_GEN_BAD_WIDTH;
    return 0;
}

extern "C" int clv_patch_embed_gen_fwd(const float* x, const void* w, const float* bias, const float* gamma,
                                       const float* beta, const float* mask_token, const int64_t* vmask, void* out_clean,
                                       void* out_masked, void* z_out, float* mean, float* rstd, int32_t B, int32_t T,
                                       int32_t H, int32_t W, int32_t C, int32_t mh, int32_t mw, int32_t pt, int32_t ph,
                                       int32_t pw, int32_t st, int32_t sh, int32_t sw, float eps, void* stream) {
    PGShape S;
    if (!fwd_args_ok(x, w, bias, gamma, beta, mask_token, vmask, out_clean, out_masked)) return CLV_ERR_ARG;
    if ((((uintptr_t)w) | ((uintptr_t)out_clean) | ((uintptr_t)out_masked) | ((uintptr_t)z_out)) & 15) return CLV_ERR_ARG;
    if (clv_patch_embed_gen_supported(pt, ph, pw, st, sh, sw, C) != 0) return CLV_ERR_UNSUPPORTED;
    if (!make_shape(S, x, B, T, H, W, pt, ph, pw, st, sh, sw, C, out_masked ? mh : 1, out_masked ? mw : 1))
        return CLV_ERR_ARG;
    hipStream_t hs = (hipStream_t)stream;
    switch (C) {
        case 48: return launch_gen_fwd<48>(x, w, bias, gamma, beta, mask_token, vmask, out_clean, out_masked, z_out, mean, rstd, S, eps, hs);
        case 96: return launch_gen_fwd<96>(x, w, bias, gamma, beta, mask_token, vmask, out_clean, out_masked, z_out, mean, rstd, S, eps, hs);
        case 128: return launch_gen_fwd<128>(x, w, bias, gamma, beta, mask_token, vmask, out_clean, out_masked, z_out, mean, rstd, S, eps, hs);
        default: return CLV_ERR_UNSUPPORTED;
    }
}

extern "C" int clv_im2col_patches(const float* x, void* patches, int32_t B, int32_t T, int32_t H, int32_t W, int32_t pt,
                                  int32_t ph, int32_t pw, int32_t st, int32_t sh, int32_t sw, void* stream) {
    PGShape S;
    if (!x || !patches || (((uintptr_t)patches) & 15)) return CLV_ERR_ARG;
    if (clv_patch_embed_gen_supported(pt, ph, pw, st, sh, sw, 96) != 0) return CLV_ERR_UNSUPPORTED;
    if (!make_shape(S, x, B, T, H, W, pt, ph, pw, st, sh, sw, 96, 1, 1)) return CLV_ERR_ARG;
    const int64_t total = S.G.M * (S.K / 8);
    int grid = (int)((total + 255) / 256);
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(im2col_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, (bf16_t*)patches, S);
    return clv_check_launch();
}

extern "C" int clv_patch_embed_blend_bwd(const void* dclean, const void* dmasked, const int64_t* vmask, void* dy,
                                         float* dmask_token, int32_t B, int32_t Tp, int32_t Hp, int32_t Wp, int32_t C,
                                         int32_t mh, int32_t mw, void* stream) {
    PEGrid G;
    if (!dy || (!dclean && !dmasked) || (dmasked && (!vmask || !dmask_token))) return CLV_ERR_ARG;
    if ((((uintptr_t)dclean) | ((uintptr_t)dmasked) | ((uintptr_t)dy)) & 15) return CLV_ERR_ARG;
    if (!make_grid(G, B, Tp, Hp, Wp, dmasked ? mh : 1, dmasked ? mw : 1)) return CLV_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
#define BB_LAUNCH(CV)                                                                                             \
    {                                                                                                             \
        const int rpb = 256 / (CV / 8);                                                                           \
        int64_t g = (G.M + rpb - 1) / rpb;                                                                        \
        if (g > 2048) g = 2048;                                                                                   \
        hipLaunchKernelGGL((blend_bwd_kernel<CV>), dim3((unsigned)g), dim3(256), 0, st, (const bf16_t*)dclean,    \
                           (const bf16_t*)dmasked, vmask, (bf16_t*)dy, dmask_token, G);                           \
    }
    switch (C) {
        case 48: BB_LAUNCH(48) break;
        case 96: BB_LAUNCH(96) break;
        case 128: BB_LAUNCH(128) break;
        default: return CLV_ERR_UNSUPPORTED;
    }
#undef BB_LAUNCH
    return clv_check_launch();
}
