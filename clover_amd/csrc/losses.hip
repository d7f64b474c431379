// Fused losses of the Clover pre-training step (fp32 math, as the reference's @force_fp32):
//   * focal masked-LM cross entropy over the vocabulary (one pass over the logits);
//   * exclusive tri-modal InfoNCE + margin ranking on the all-gathered embeddings
//     (normalise -> f32-MFMA similarity GEMMs -> one-block loss -> analytic backward).
#include "common.hpp"
#include "../../include/clover_hip.h"

namespace {

// =========================================================================== focal CE
constexpr int FC_THREADS = 256;

template <bool BF16>
__device__ __forceinline__ float ld_logit(const void* p, int64_t i) {
    if (BF16) return bf2f(reinterpret_cast<const bf16_t*>(p)[i]);
    return reinterpret_cast<const float*>(p)[i];
}

__device__ __forceinline__ float block_reduce(float v, float* sh, bool is_max) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    v = is_max ? wave_max(v) : wave_sum(v);
    __syncthreads();
    if (lane == 0) sh[wv] = v;
    __syncthreads();
    float r = sh[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r = is_max ? fmaxf(r, sh[w]) : r + sh[w];
    return r;
}

template <bool BF16>
__global__ void __launch_bounds__(FC_THREADS) focal_fwd_kernel(
    const void* __restrict__ logits, const int64_t* __restrict__ labels, float* __restrict__ row_ce,
    float* __restrict__ row_lse, float* __restrict__ sum_acc, float* __restrict__ cnt_acc, int V, int64_t ld, float gamma) {
    __shared__ float sh[8];
    const int64_t row = blockIdx.x;
    const int64_t lab = labels[row];
    if (lab < 0) {                       // label == -100: not a masked position
        if (threadIdx.x == 0) { row_ce[row] = 0.f; row_lse[row] = 0.f; }
        return;
    }
    const int64_t base = row * ld;
    float m = -INFINITY;
    for (int j = threadIdx.x; j < V; j += FC_THREADS) m = fmaxf(m, ld_logit<BF16>(logits, base + j));
    m = block_reduce(m, sh, true);
    float s = 0.f;
    for (int j = threadIdx.x; j < V; j += FC_THREADS) s += __expf(ld_logit<BF16>(logits, base + j) - m);
    s = block_reduce(s, sh, false);
    if (threadIdx.x == 0) {
        const float lse = m + __logf(s);
        const float ce = lse - ld_logit<BF16>(logits, base + lab);
        const float pt = __expf(-ce);
        row_ce[row] = ce;
        row_lse[row] = lse;
        atomicAdd(sum_acc, powf(1.f - pt, gamma) * ce);
        atomicAdd(cnt_acc, 1.0f);
    }
}

__global__ void focal_finish_kernel(float* __restrict__ loss, const float* __restrict__ count) {
    loss[0] = loss[0] / count[0];        // mean over the masked rows (NaN when there are none, as torch)
}

template <bool BF16>
__global__ void __launch_bounds__(FC_THREADS) focal_bwd_kernel(
    const void* __restrict__ logits, const int64_t* __restrict__ labels, const float* __restrict__ row_ce,
    const float* __restrict__ row_lse, const float* __restrict__ count, const float* __restrict__ dloss,
    void* __restrict__ dlogits, int V, int64_t ld, float gamma) {
    const int64_t row = blockIdx.x;
    const int64_t lab = labels[row];
    const int64_t base = row * ld;
    float coef = 0.f, lse = 0.f;
    if (lab >= 0) {
        const float ce = row_ce[row], pt = __expf(-ce), om = 1.f - pt;
        // d/dce [(1-pt)^g * ce] = g (1-pt)^(g-1) pt ce + (1-pt)^g
        const float dl = (gamma == 0.f) ? 1.f : gamma * powf(om, gamma - 1.f) * pt * ce + powf(om, gamma);
        coef = dloss[0] * dl / count[0];
        lse = row_lse[row];
    }
    for (int j = threadIdx.x; j < (int)ld; j += FC_THREADS) {     // columns [V, ld) are padding: zero
        float g = 0.f;
        if (lab >= 0 && j < V) {
            const float p = __expf(ld_logit<BF16>(logits, base + j) - lse);
            g = coef * (p - (j == lab ? 1.f : 0.f));
        }
        if (BF16) reinterpret_cast<bf16_t*>(dlogits)[base + j] = f2bf(g);
        else reinterpret_cast<float*>(dlogits)[base + j] = g;
    }
}

// bf16 logits with an even vocabulary (30522): a row is 4-byte aligned, so a thread moves PAIRS (one 4-byte access), 1024
// threads per row, and the forward keeps a running (max, sum) per thread — one pass over the row, 15 independent loads
// per thread instead of two passes of 120 dependent 2-byte ones (43 -> ~10 us for the ~40 masked rows of a step, which
// sit at the tail of the forward graph and at the head of the backward graph).
constexpr int FC_WIDE = 1024;

__global__ void __launch_bounds__(FC_WIDE) focal_fwd_pairs_kernel(
    const unsigned* __restrict__ logits2, const int64_t* __restrict__ labels, float* __restrict__ row_ce,
    float* __restrict__ row_lse, float* __restrict__ sum_acc, float* __restrict__ cnt_acc, int V, int64_t ld, float gamma) {
    __shared__ float shm[FC_WIDE / 64], shs[FC_WIDE / 64];
    const int64_t row = blockIdx.x;
    const int64_t lab = labels[row];
    if (lab < 0) {
        if (threadIdx.x == 0) { row_ce[row] = 0.f; row_lse[row] = 0.f; }
        return;
    }
    const int V2 = V >> 1;
    const unsigned* r2 = logits2 + row * (ld >> 1);
    float m = -INFINITY, sum = 0.f;
    for (int j = threadIdx.x; j < V2; j += FC_WIDE) {
        const unsigned w = r2[j];
        const float a = bf2f((bf16_t)(w & 0xffff)), b = bf2f((bf16_t)(w >> 16));
        const float mn = fmaxf(m, fmaxf(a, b));
        sum = sum * __expf(m - mn) + __expf(a - mn) + __expf(b - mn);     // first trip: 0 * exp(-inf) = 0
        m = mn;
    }
    // (m, sum) pairs: wave, then block
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float wm = wave_max(m);
    sum = wave_sum(m == -INFINITY ? 0.f : sum * __expf(m - wm));          // a lane (or a whole wave) without elements
    if (lane == 0) { shm[wv] = wm; shs[wv] = sum; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float bm = shm[0];
        for (int w = 1; w < FC_WIDE / 64; ++w) bm = fmaxf(bm, shm[w]);
        float bs = 0.f;
        for (int w = 0; w < FC_WIDE / 64; ++w)
            if (shm[w] != -INFINITY) bs += shs[w] * __expf(shm[w] - bm);
        const float lse = bm + __logf(bs);
        const unsigned w = r2[lab >> 1];
        const float ce = lse - bf2f((bf16_t)((lab & 1) ? (w >> 16) : (w & 0xffff)));
        const float pt = __expf(-ce);
        row_ce[row] = ce;
        row_lse[row] = lse;
        atomicAdd(sum_acc, powf(1.f - pt, gamma) * ce);
        atomicAdd(cnt_acc, 1.0f);
    }
}

__global__ void __launch_bounds__(FC_WIDE) focal_bwd_pairs_kernel(
    const unsigned* __restrict__ logits2, const int64_t* __restrict__ labels, const float* __restrict__ row_ce,
    const float* __restrict__ row_lse, const float* __restrict__ count, const float* __restrict__ dloss,
    unsigned* __restrict__ dlogits2, int V, int64_t ld, float gamma) {
    const int64_t row = blockIdx.x;
    const int64_t lab = labels[row];
    const int V2 = V >> 1, L2 = (int)(ld >> 1);
    unsigned* d2 = dlogits2 + row * L2;
    if (lab < 0) {
        for (int j = threadIdx.x; j < L2; j += FC_WIDE) d2[j] = 0u;
        return;
    }
    for (int j = V2 + threadIdx.x; j < L2; j += FC_WIDE) d2[j] = 0u;      // padding columns [V, ld)
    const float ce = row_ce[row], pt = __expf(-ce), om = 1.f - pt;
    const float dl = (gamma == 0.f) ? 1.f : gamma * powf(om, gamma - 1.f) * pt * ce + powf(om, gamma);
    const float coef = dloss[0] * dl / count[0], lse = row_lse[row];
    const unsigned* r2 = logits2 + row * L2;
    const int labp = (int)(lab >> 1);
    for (int j = threadIdx.x; j < V2; j += FC_WIDE) {
        const unsigned w = r2[j];
        float ga = coef * __expf(bf2f((bf16_t)(w & 0xffff)) - lse), gb = coef * __expf(bf2f((bf16_t)(w >> 16)) - lse);
        if (j == labp) {
            if (lab & 1) gb -= coef;
            else ga -= coef;
        }
        d2[j] = pack2bf(ga, gb);
    }
}

// =========================================================================== the work area of a contrastive loss
// One layout for every loss below, with nb score blocks against the first embedding (InfoNCE: 3, NormSoftmax and the
// dual-softmax loss: 1).  In floats, in this order:
//   en   [nb+1][G][Dm]  normalised embeddings
//   enT  [Dm][nb+1][G]  their transpose (contraction index (k, j) contiguous)
//   den  [nb+1][G][Dm]  d loss / d normalised embeddings
//   invn [nb+1][G]      1/max(|e|, eps); NormSoftmax and the dual-softmax loss set its sign bit on the clamped rows
//   sim  [nb][G][G]     en0 . en_{k+1}^T / temperature (the dual-softmax loss: the cosine)
//   dsim [G][nb][G]     d loss / d sim, row-major in (i, k, j)
//   dsimT[nb][G][G]     transposed per block: [k][j][i]
//   lser [nb][G]        row log-sum-exp (InfoNCE: of the three exclusive [G,3G] rows)
//   lsec [nb][G]        column log-sum-exp (t2v)
//   16 spare
//   term [2 nb][G]      multi-workgroup path only: diag - lse of every (exclusive) row, then of every column
// loss_work_off is the one statement of it: the carve, the float count and the plan entries (which need the operand
// addresses modulo 16 only) all read it.
struct LossWork {
    float *en, *enT, *den, *invn, *sim, *dsim, *dsimT, *lser, *lsec, *term;
};
struct LossWorkOff {
    int64_t en, enT, den, invn, sim, dsim, dsimT, lser, lsec, term;
};
__host__ __device__ inline LossWorkOff loss_work_off(int nb, int G, int Dm) {
    const int64_t emb = (int64_t)(nb + 1) * G * Dm, blk = (int64_t)nb * G * G;
    LossWorkOff o;
    int64_t w = 0;
    o.en = w; w += emb;
    o.enT = w; w += emb;
    o.den = w; w += emb;
    o.invn = w; w += (nb + 1) * G;
    o.sim = w; w += blk;
    o.dsim = w; w += blk;
    o.dsimT = w; w += blk;
    o.lser = w; w += nb * G;
    o.lsec = w; w += nb * G;
    w += 16;
    o.term = w;
    return o;
}
__host__ __device__ inline int64_t loss_work_floats(int nb, int G, int Dm) {
    return loss_work_off(nb, G, Dm).term + (int64_t)2 * nb * G;
}
__host__ __device__ inline LossWork loss_carve(float* w, int nb, int G, int Dm) {
    const LossWorkOff o = loss_work_off(nb, G, Dm);
    return {w + o.en,   w + o.enT,   w + o.den,  w + o.invn, w + o.sim,
            w + o.dsim, w + o.dsimT, w + o.lser, w + o.lsec, w + o.term};
}

// one wave per row: en = e / max(|e|, eps) of NE embeddings with row stride ld.  InfoNCE: eps 1e-8 (cos_norm,
// contrastive_loss.py:20-25); NormSoftmax: F.normalize's 1e-12 (:51-52) or sim_matrix's 1e-8 (:10-18).  MARK: the sign bit of
// invn marks the clamped rows (nrm < eps) for the backward; without it the backward tests invn >= 1e8.  The two tests differ
// at |e| == eps exactly, and each loss keeps its own.
template <int NE, bool MARK>
__device__ __forceinline__ void normalize_body(const float* e0, const float* e1, const float* e2, const float* e3,
                                               const LossWork& W, int G, int Dm, int ld, float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= NE * G) return;
    const int k = row / G, i = row - k * G;
    const float* e = (k == 0 ? e0 : (NE == 2 || k == 1) ? e1 : k == 2 ? e2 : e3) + (int64_t)i * ld;
    float s = 0.f;
    for (int d = lane; d < Dm; d += 64) s += e[d] * e[d];
    const float nrm = sqrtf(wave_sum(s));
    const float inv = 1.0f / fmaxf(nrm, eps);
    if (lane == 0) W.invn[row] = (!MARK || nrm >= eps) ? inv : -inv;
    for (int d = lane; d < Dm; d += 64) {
        const float v = e[d] * inv;
        W.en[(int64_t)row * Dm + d] = v;
        W.enT[((int64_t)d * NE + k) * G + i] = v;
    }
}

// =========================================================================== InfoNCE
// The recognizer evaluates the loss TWICE per step on slots of one packed [G, k, Dm] tensor (video -> text and text -> video,
// multimodal_transformer_pretrain.py:151,161): the *_pair kernels run both evaluations ("directions") in the same launches —
// blockIdx.y (or the batch index of the GEMMs) is the direction, each with its own work area — so that the loss section
// is 3 + 4 dependent launches instead of 6 + 8 (+ the zero fills and the add of the two gradients).  The forward of the
// four-tensor entries is the same host sequence with one direction (direction 0 of an NcePair) on thin kernels of its own
// over the shared bodies: through the *_pair kernels that form measured slower than before (profiles/loss_refactor.txt).
struct NcePair {
    LossWork w[2];
    const float* e[2][4];
    const float* dout[4];      // backward: device scalars, the upstream gradients of {nce_0, rank_0, nce_1, rank_1} (null: 0)
    int slot[2][4];            // the packed form's norm backward only
};
__global__ void __launch_bounds__(256) nce_normalize_kernel(const float* e0, const float* e1, const float* e2,
                                                            const float* e3, LossWork W, int G, int Dm, int ld) {
    normalize_body<4, false>(e0, e1, e2, e3, W, G, Dm, ld, 1e-8f);
}
__global__ void __launch_bounds__(256) nce_pair_normalize_kernel(NcePair P, int G, int Dm, int ld) {
    const int d = blockIdx.y;
    normalize_body<4, false>(P.e[d][0], P.e[d][1], P.e[d][2], P.e[d][3], P.w[d], G, Dm, ld, 1e-8f);
}

// C[i][j] (ldc) = alpha * sum_k A[i][k] * B[j][k]   — exact-f32 MFMA 16x16x4, one 16x16 tile per workgroup.
// K multiple of 16 is NOT required (tail guarded); rows/cols guarded.  NW waves split the contraction (partial tiles meet in
// LDS): the similarity GEMMs have G x G outputs — a handful of tiles — and Dm = 768 to contract: one wave per tile walked 48
// dependent load rounds (20 us); the gradient GEMMs contract over <= 3 G and keep one wave.
__host__ __device__ inline int sgemm_kchunk(int K, int nw) {      // per wave, a multiple of 16 (clv_loss_gemm_plan reports it)
    return ((K + nw * 16 - 1) / (nw * 16)) * 16;
}

template <int NW>
__global__ void __launch_bounds__(64 * NW) sgemm_nt_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                      float* __restrict__ C, int M, int N, int K, int lda, int ldb,
                                                      int ldc, int64_t sA, int64_t sB, int64_t sC, float alpha,
                                                      int zb, int64_t s2) {
    // batch index z = z1 * zb + z0: operand offsets (sA, sB, sC) * z0 + s2 * z1 (the pair form: z1 = direction, one work
    // area of s2 floats each)
    __shared__ float red[NW > 1 ? NW - 1 : 1][64][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lg = lane >> 4, lr = lane & 15;
    const int z1 = blockIdx.z / zb, z0 = blockIdx.z - z1 * zb;
    A += sA * z0 + s2 * z1;
    B += sB * z0 + s2 * z1;
    C += sC * z0 + s2 * z1;
    const int i = blockIdx.y * 16 + lr, j = blockIdx.x * 16 + lr;
    const float* ap = A + (int64_t)(i < M ? i : 0) * lda;
    const float* bp = B + (int64_t)(j < N ? j : 0) * ldb;
    const bool av = i < M, bv = j < N;
    const int kchunk = sgemm_kchunk(K, NW);
    const int kb = wave * kchunk, ke = min(K, kb + kchunk);
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = kb; k0 < ke; k0 += 16) {
        float a[4], b[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int k = k0 + lg * 4 + e;
            a[e] = (av && k < ke) ? ap[k] : 0.f;
            b[e] = (bv && k < ke) ? bp[k] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[e], acc, 0, 0, 0);
    }
    if (NW > 1) {
        if (wave > 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) red[wave - 1][lane][r] = acc[r];
        }
        __syncthreads();
        if (wave > 0) return;
#pragma unroll
        for (int w = 0; w < NW - 1; ++w)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] += red[w][lane][r];
    }
    // acc[r] = C[row blockIdx.y*16 + lg*4 + r][col blockIdx.x*16 + lr]
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int ci = blockIdx.y * 16 + lg * 4 + r;
        if (ci < M && j < N) C[(int64_t)ci * ldc + j] = alpha * acc[r];
    }
}

__device__ __forceinline__ float nce_entry(const float* sim, int G, int kx, int i, int k, int j) {
    // value of column (k, j) in the exclusive row of variant kx for sample i
    // (contrastive_loss.py:130-132: other blocks' diagonals become x - (x + 10000))
    const float x = sim[((int64_t)k * G + i) * G + j];
    if (k != kx && j == i) return x - (x + 10000.f);
    return x;
}

// single block: all log-sum-exps, the two losses.
__device__ __forceinline__ void nce_loss_body(const LossWork& W, float* __restrict__ out, int G, float margin) {
    __shared__ float sh[16];
    const float* sim = W.sim;
    float part_v = 0.f, part_t = 0.f, part_r = 0.f;
    // 3G exclusive rows + 3G columns, one thread each (G <= 512 in practice: 3G*G work per thread is tiny)
    for (int t = threadIdx.x; t < 6 * G; t += blockDim.x) {
        if (t < 3 * G) {
            const int kx = t / G, i = t - kx * G;
            float m = -INFINITY;
            for (int k = 0; k < 3; ++k)
                for (int j = 0; j < G; ++j) m = fmaxf(m, nce_entry(sim, G, kx, i, k, j));
            float s = 0.f;
            for (int k = 0; k < 3; ++k)
                for (int j = 0; j < G; ++j) s += __expf(nce_entry(sim, G, kx, i, k, j) - m);
            const float lse = m + __logf(s);
            W.lser[t] = lse;
            part_v += sim[((int64_t)kx * G + i) * G + i] - lse;          // diag of the own block
        } else {
            const int u = t - 3 * G, k = u / G, j = u - k * G;
            float m = -INFINITY;
            for (int i = 0; i < G; ++i) m = fmaxf(m, sim[((int64_t)k * G + i) * G + j]);
            float s = 0.f;
            for (int i = 0; i < G; ++i) s += __expf(sim[((int64_t)k * G + i) * G + j] - m);
            const float lse = m + __logf(s);
            W.lsec[u] = lse;
            part_t += sim[((int64_t)k * G + j) * G + j] - lse;
        }
    }
    for (int i = threadIdx.x; i < G; i += blockDim.x) {
        const float a = sim[((int64_t)0 * G + i) * G + i], b = sim[((int64_t)1 * G + i) * G + i];
        part_r += fmaxf(0.f, -(a - b) + margin);
    }
    const float sv = block_reduce(part_v, sh, false);
    const float stt = block_reduce(part_t, sh, false);
    const float sr = block_reduce(part_r, sh, false);
    if (threadIdx.x == 0) {
        const float loss_v = -(sv / (float)G);
        const float loss_t = -(stt / (float)(3 * G));
        out[0] = loss_v + loss_t;
        out[1] = sr / (float)G;
    }
}
__global__ void __launch_bounds__(1024) nce_loss_kernel(LossWork W, float* __restrict__ out, int G, float margin) {
    nce_loss_body(W, out, G, margin);
}
__global__ void __launch_bounds__(1024) nce_pair_loss_kernel(NcePair P, float* __restrict__ out, int G, float margin) {
    nce_loss_body(P.w[blockIdx.x], out + 2 * blockIdx.x, G, margin);
}

// elementwise: d loss / d sim[k][i][j]
__device__ __forceinline__ void nce_dsim_body(const LossWork& W, const float gn, const float gr, int G, float margin) {
    const int64_t total = (int64_t)3 * G * G;
    const float invG = 1.0f / (float)G, inv3G = 1.0f / (float)(3 * G);
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int k = (int)(idx / ((int64_t)G * G));
        const int rem = (int)(idx - (int64_t)k * G * G);
        const int i = rem / G, j = rem - i * G;
        const float x = W.sim[idx];
        float g = 0.f;
        // v2t: three exclusive rows of sample i
        for (int kx = 0; kx < 3; ++kx) {
            if (k != kx && j == i) continue;                    // excluded entry: x-(x+1e4) has zero slope
            const float p = __expf(x - W.lser[kx * G + i]);
            g += -invG * gn * ((k == kx && j == i ? 1.f : 0.f) - p);
        }
        // t2v: column softmax over i
        g += -inv3G * gn * ((i == j ? 1.f : 0.f) - __expf(x - W.lsec[k * G + j]));
        // ranking: mean_i max(0, margin - (vt_ii - vtm_ii))
        if (i == j && k < 2) {
            const float a = W.sim[((int64_t)0 * G + i) * G + i], b = W.sim[((int64_t)1 * G + i) * G + i];
            if (-(a - b) + margin > 0.f) g += (k == 0 ? -1.f : 1.f) * invG * gr;
        }
        W.dsim[((int64_t)i * 3 + k) * G + j] = g;
        W.dsimT[((int64_t)k * G + j) * G + i] = g;
    }
}
__global__ void __launch_bounds__(256) nce_dsim_kernel(LossWork W, const float* __restrict__ dout, int G, float margin) {
    nce_dsim_body(W, dout[0], dout[1], G, margin);
}
__global__ void __launch_bounds__(256) nce_pair_dsim_kernel(NcePair P, int G, float margin) {
    const float* gn = P.dout[2 * blockIdx.y];
    const float* gr = P.dout[2 * blockIdx.y + 1];
    nce_dsim_body(P.w[blockIdx.y], gn ? *gn : 0.f, gr ? *gr : 0.f, G, margin);
}

// d e = invn * (d en - en * <en, d en>)   (valid while |e| >= eps; below eps: d e = d en * invn) into NE separate gradients
// with row stride ldd; NE and MARK as normalize_body.
template <int NE, bool MARK>
__global__ void __launch_bounds__(256) norm_bwd_kernel(LossWork W, float* d0, float* d1, float* d2, float* d3, int G,
                                                       int Dm, int ldd) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= NE * G) return;
    const int k = row / G, i = row - k * G;
    float* d = (k == 0 ? d0 : (NE == 2 || k == 1) ? d1 : k == 2 ? d2 : d3) + (int64_t)i * ldd;
    const float* en = W.en + (int64_t)row * Dm;
    const float* de = W.den + (int64_t)row * Dm;
    float s = 0.f;
    for (int c = lane; c < Dm; c += 64) s += en[c] * de[c];
    s = wave_sum(s);
    const float inv = W.invn[row];
    const bool clamped = MARK ? inv < 0.f : inv >= 1e8f;
    for (int c = lane; c < Dm; c += 64) d[c] = clamped ? de[c] * (MARK ? -inv : inv) : inv * (de[c] - en[c] * s);
}

// The packed pair form writes the WHOLE packed gradient [G][k][Dm]: one wave per (row i, slot s) sums d en over the (direction,
// position) pairs that read slot s (video and text are read by both directions; the map d e = invn (d en - en <en, d en>) is
// linear in d en and en / invn of a slot are the same numbers in both work areas), a slot nobody read gets zeros.
__global__ void __launch_bounds__(256) nce_pair_norm_bwd_kernel(NcePair P, float* __restrict__ dp, int G, int k, int Dm) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= k * G) return;
    const int i = row / k, sl = row - i * k;
    float* d = dp + (int64_t)row * Dm;
    const float* en = nullptr;
    const float* de[2] = {nullptr, nullptr};
    float inv = 0.f;
    int n = 0;
#pragma unroll
    for (int dir = 0; dir < 2; ++dir)
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (P.slot[dir][q] == sl && n < 2) {
                const int64_t r = (int64_t)q * G + i;
                if (!n) {
                    en = P.w[dir].en + r * Dm;
                    inv = P.w[dir].invn[r];
                }
                de[n++] = P.w[dir].den + r * Dm;
            }
    if (!n) {
        for (int c = lane; c < Dm; c += 64) d[c] = 0.f;
        return;
    }
    float s = 0.f;
    for (int c = lane; c < Dm; c += 64) s += en[c] * (de[0][c] + (n > 1 ? de[1][c] : 0.f));
    s = wave_sum(s);
    const bool clamped = inv >= 1e8f;
    for (int c = lane; c < Dm; c += 64) {
        const float g = de[0][c] + (n > 1 ? de[1][c] : 0.f);
        d[c] = clamped ? g * inv : inv * (g - en[c] * s);
    }
}


// =========================================================================== NormSoftmaxLoss
// (mmaction/models/losses/contrastive_loss.py:26-68): x = normalise(video) . normalise(text)^T / t,
// loss = -mean_i diag(log_softmax(x, 1)) - mean_j diag(log_softmax(x^T, 1)).
// The work area is the common one with nb = 1.
__global__ void __launch_bounds__(256) ns_normalize_kernel(const float* e0, const float* e1, LossWork W, int G, int Dm,
                                                           float eps) {
    normalize_body<2, true>(e0, e1, nullptr, nullptr, W, G, Dm, Dm, eps);
}

// single block: G row + G column log-sum-exps (one thread each), then the loss.
__global__ void __launch_bounds__(1024) ns_loss_kernel(LossWork W, const float* __restrict__ sim, float* __restrict__ out,
                                                       int G) {
    __shared__ float sh[16];
    float part = 0.f;
    for (int t = threadIdx.x; t < 2 * G; t += blockDim.x) {
        const bool col = t >= G;
        const int u = col ? t - G : t;
        const int64_t base = col ? u : (int64_t)u * G, step = col ? G : 1;
        float m = -INFINITY;
        for (int j = 0; j < G; ++j) m = fmaxf(m, sim[base + j * step]);
        float s = 0.f;
        for (int j = 0; j < G; ++j) s += __expf(sim[base + j * step] - m);
        const float lse = m + __logf(s);
        (col ? W.lsec : W.lser)[u] = lse;
        part += sim[(int64_t)u * G + u] - lse;
    }
    const float tot = block_reduce(part, sh, false);
    if (threadIdx.x == 0) out[0] = -(tot / (float)G);
}

__global__ void __launch_bounds__(256) ns_dsim_kernel(LossWork W, const float* __restrict__ sim,
                                                      const float* __restrict__ dout, float* __restrict__ dsim_out,
                                                      int G) {
    const int64_t total = (int64_t)G * G;
    const float g = -dout[0] / (float)G;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int i = (int)(idx / G), j = (int)(idx - (int64_t)i * G);
        const float x = sim[idx];
        const float d = g * ((i == j ? 2.f : 0.f) - __expf(x - W.lser[i]) - __expf(x - W.lsec[j]));
        dsim_out[idx] = d;
        if (dsim_out == W.dsim) W.dsimT[(int64_t)j * G + i] = d;
    }
}

// =========================================================================== the loss section at a global batch
// The one-workgroup kernels above serve a device batch (G <= ~100).  With virtual ranks G is the GLOBAL batch (1024 at the
// reference's headline configuration): 6 G log-sum-exps over G or 3 G scores each, 19 M exponentials on one CU.  The kernels
// below spread them over the device and keep the result reproducible — no float atomics, every sum in a fixed order:
//   lse_rows_kernel : one wave per exclusive row; its NB rows of G scores are contiguous, lanes stride them; ONE pass with a
//                     running (max, sum) per lane (as focal_fwd_pairs_kernel), merged across the wave
//   lse_cols_kernel : 64 adjacent columns per workgroup (a lane = a column: every global read is contiguous across the
//                     wave), 16 waves share the G rows; the 16 (max, sum) pairs of a column meet in LDS in wave order
//   *_finish_kernel : one workgroup sums the per-row terms diag - lse in a fixed order and writes the losses
// lser / lsec are written exactly as the one-workgroup kernels write them: the backward kernels are shared.
constexpr int LSE_COL_WAVES = 16;

__device__ __forceinline__ void lse_push(float& m, float& s, float x) {
    const float mn = fmaxf(m, x);
    if (mn == -INFINITY) return;
    s = s * __expf(m - mn) + __expf(x - mn);                  // first value: 0 * exp(-inf) = 0
    m = mn;
}

template <int NB>
__device__ __forceinline__ void lse_rows_body(const float* __restrict__ sim, float* __restrict__ lser,
                                              float* __restrict__ term, int G) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= NB * G) return;
    const int kx = t / G, i = t - kx * G;
    float m = -INFINITY, s = 0.f;
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        const float* row = sim + ((int64_t)k * G + i) * G;
        for (int j = lane; j < G; j += 64) {
            float x = row[j];
            if (k != kx && j == i) x = x - (x + 10000.f);     // nce_entry: the other blocks' diagonals
            lse_push(m, s, x);
        }
    }
    const float wm = wave_max(m);
    s = wave_sum(m == -INFINITY ? 0.f : s * __expf(m - wm));  // a lane without elements (G < 64)
    if (lane == 0) {
        const float lse = wm + __logf(s);
        lser[t] = lse;
        term[t] = sim[((int64_t)kx * G + i) * G + i] - lse;
    }
}

__device__ __forceinline__ void lse_cols_body(const float* __restrict__ sim, float* __restrict__ lsec,
                                              float* __restrict__ term, int G) {
    __shared__ float shm[LSE_COL_WAVES][64], shs[LSE_COL_WAVES][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int k = blockIdx.y, j = blockIdx.x * 64 + lane;
    const float* blk = sim + (int64_t)k * G * G;
    float m = -INFINITY, s = 0.f;
    if (j < G)
        for (int i = wv; i < G; i += LSE_COL_WAVES) lse_push(m, s, blk[(int64_t)i * G + j]);
    shm[wv][lane] = m;
    shs[wv][lane] = s;
    __syncthreads();
    if (wv != 0 || j >= G) return;
    float bm = shm[0][lane];
#pragma unroll
    for (int w = 1; w < LSE_COL_WAVES; ++w) bm = fmaxf(bm, shm[w][lane]);
    float bs = 0.f;
#pragma unroll
    for (int w = 0; w < LSE_COL_WAVES; ++w)
        if (shm[w][lane] != -INFINITY) bs += shs[w][lane] * __expf(shm[w][lane] - bm);
    const float lse = bm + __logf(bs);
    lsec[k * G + j] = lse;
    term[k * G + j] = blk[(int64_t)j * G + j] - lse;
}

__device__ __forceinline__ void nce_finish_body(const LossWork& W, float* __restrict__ out, int G, float margin) {
    __shared__ float sh[16];
    float part_v = 0.f, part_t = 0.f, part_r = 0.f;
    for (int t = threadIdx.x; t < 3 * G; t += blockDim.x) {
        part_v += W.term[t];
        part_t += W.term[3 * G + t];
    }
    for (int i = threadIdx.x; i < G; i += blockDim.x) {
        const float a = W.sim[((int64_t)0 * G + i) * G + i], b = W.sim[((int64_t)1 * G + i) * G + i];
        part_r += fmaxf(0.f, -(a - b) + margin);
    }
    const float sv = block_reduce(part_v, sh, false);
    const float stt = block_reduce(part_t, sh, false);
    const float sr = block_reduce(part_r, sh, false);
    if (threadIdx.x == 0) {
        out[0] = -(sv / (float)G) + -(stt / (float)(3 * G));
        out[1] = sr / (float)G;
    }
}

__global__ void __launch_bounds__(256) nce_lse_rows_kernel(LossWork W, int G) {
    lse_rows_body<3>(W.sim, W.lser, W.term, G);
}
__global__ void __launch_bounds__(256) nce_pair_lse_rows_kernel(NcePair P, int G) {
    const LossWork& W = P.w[blockIdx.y];
    lse_rows_body<3>(W.sim, W.lser, W.term, G);
}
__global__ void __launch_bounds__(64 * LSE_COL_WAVES) nce_lse_cols_kernel(LossWork W, int G) {
    lse_cols_body(W.sim, W.lsec, W.term + 3 * G, G);
}
__global__ void __launch_bounds__(64 * LSE_COL_WAVES) nce_pair_lse_cols_kernel(NcePair P, int G) {
    const LossWork& W = P.w[blockIdx.z];
    lse_cols_body(W.sim, W.lsec, W.term + 3 * G, G);
}
__global__ void __launch_bounds__(256) nce_finish_kernel(LossWork W, float* __restrict__ out, int G, float margin) {
    nce_finish_body(W, out, G, margin);
}
__global__ void __launch_bounds__(256) nce_pair_finish_kernel(NcePair P, float* __restrict__ out, int G, float margin) {
    nce_finish_body(P.w[blockIdx.x], out + 2 * blockIdx.x, G, margin);
}
__global__ void __launch_bounds__(256) ns_lse_rows_kernel(LossWork W, const float* __restrict__ sim, int G) {
    lse_rows_body<1>(sim, W.lser, W.term, G);
}
__global__ void __launch_bounds__(64 * LSE_COL_WAVES) ns_lse_cols_kernel(LossWork W, const float* __restrict__ sim, int G) {
    lse_cols_body(sim, W.lsec, W.term + G, G);
}
__global__ void __launch_bounds__(256) ns_finish_kernel(LossWork W, float* __restrict__ out, int G) {
    __shared__ float sh[16];
    float part = 0.f;
    for (int t = threadIdx.x; t < 2 * G; t += blockDim.x) part += W.term[t];
    const float tot = block_reduce(part, sh, false);
    if (threadIdx.x == 0) out[0] = -(tot / (float)G);
}

// C[i][j] (ldc) = alpha * sum_k A[i][k] * B[j][k], batched like sgemm_nt_kernel, as 64 x 64 x 16 LDS tiles (4 waves, 32 x 32
// each, exact-f32 MFMA 16x16x4; the tile loop of parity.hip's sgemm_tiled_kernel).  sgemm_nt_kernel gives every 16 x 16 tile
// a wave of its own, which re-reads each operand row from L2 once per tile across: G / 16 = 64 times at G = 1024.
constexpr int LT_BM = 64, LT_BN = 64, LT_BK = 16, LT_LD = LT_BK + 1;

template <bool VEC>
__global__ void __launch_bounds__(256) sgemm_nt_tiled_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                             float* __restrict__ C, int M, int N, int K, int lda, int ldb,
                                                             int ldc, int64_t sA, int64_t sB, int64_t sC, float alpha,
                                                             int zb, int64_t s2) {
    __shared__ float As[LT_BM * LT_LD], Bs[LT_BN * LT_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lg = lane >> 4, lr = lane & 15;
    const int z1 = blockIdx.z / zb, z0 = blockIdx.z - z1 * zb;
    A += sA * z0 + s2 * z1;
    B += sB * z0 + s2 * z1;
    C += sC * z0 + s2 * z1;
    const int m0 = blockIdx.y * LT_BM, n0 = blockIdx.x * LT_BN;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
    f32x4_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    const int srow = tid >> 2, sk = (tid & 3) * 4;            // staging: four floats of A and of B per thread
    const int am = m0 + srow, bn = n0 + srow;
    for (int k0 = 0; k0 < K; k0 += LT_BK) {
        float4 av = make_float4(0.f, 0.f, 0.f, 0.f), bv = av;
        if (VEC) {
            if (am < M) av = *reinterpret_cast<const float4*>(A + (int64_t)am * lda + k0 + sk);
            if (bn < N) bv = *reinterpret_cast<const float4*>(B + (int64_t)bn * ldb + k0 + sk);
        } else {
            float* a4 = reinterpret_cast<float*>(&av);
            float* b4 = reinterpret_cast<float*>(&bv);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int kk = k0 + sk + e;
                if (am < M && kk < K) a4[e] = A[(int64_t)am * lda + kk];
                if (bn < N && kk < K) b4[e] = B[(int64_t)bn * ldb + kk];
            }
        }
        __syncthreads();                                      // the previous step's fragment reads are done
        float* as = As + srow * LT_LD + sk;
        float* bs = Bs + srow * LT_LD + sk;
        as[0] = av.x; as[1] = av.y; as[2] = av.z; as[3] = av.w;
        bs[0] = bv.x; bs[1] = bv.y; bs[2] = bv.z; bs[3] = bv.w;
        __syncthreads();
#pragma unroll
        for (int k4 = 0; k4 < LT_BK; k4 += 4) {
            float a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                a[i] = As[(wr + i * 16 + lr) * LT_LD + k4 + lg];
                b[i] = Bs[(wc + i * 16 + lr) * LT_LD + k4 + lg];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }
    // acc[i][j][r] = C[m0 + wr + i*16 + lg*4 + r][n0 + wc + j*16 + lr]
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int cn = n0 + wc + j * 16 + lr;
            if (cn >= N) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int cm = m0 + wr + i * 16 + lg * 4 + r;
                if (cm < M) C[(int64_t)cm * ldc + cn] = alpha * acc[i][j][r];
            }
        }
}

// =========================================================================== dual-softmax loss (DSL)
// NormSoftmaxLoss under the dual-softmax prior (the training half of retrieval.hip's re-scoring; not in the reference).  With
// c = en_v . en_t^T (the cosine, held in `sim`: the score GEMM runs with alpha 1), x = T c and a = G / temperature:
//   Pr = softmax over i of x      yr = (a c) Pr     (video -> text logits; its log-sum-exp runs along a row)
//   Pc = softmax over j of x      yc = (a c) Pc     (text -> video logits; its log-sum-exp runs down a column)
//   loss = -(sum_i (yr[i][i] - lse_j yr[i][j]) + sum_j (yc[j][j] - lse_i yc[i][j])) / G
// Every exponential takes an argument that a maximum or a log-sum-exp of its own row / column was subtracted from, so T = 100
// (most priors underflow to 0) stays finite.  y is formed on the fly from c and the prior statistics: no second G x G matrix.
// Backward, with gr = softmax_j(yr) - [i == j], gc = softmax_i(yc) - [i == j] (the 1 / G is folded into the scale):
//   u[j] = sum_i (gr c) Pr      w[i] = sum_j (gc c) Pc
//   d loss / d c = dout / temperature * ( Pr (gr (1 + x) - T u[j]) + Pc (gc (1 + x) - T w[i]) )
// work layout: that of NormSoftmax (LossWork with nb = 1; lser / lsec hold the log-sums of yr / yc), then the prior statistics
// pc.m, pc.l, pr.m, pr.l, the maxima yr.m, yc.m, and w, u: [G] each.  The backward reads only what the forward
// left there, and both forms leave the same numbers in the same places: either backward accepts either forward's work.
// The arithmetic of this section is written with contraction off, one rounding per operation, so that tests/dsl_loss_ref.py
// can repeat it (lse_push keeps its fused multiply-add, as loss_ref models it).
// A log-sum-exp kept in two parts: the maximum m and l = log sum exp(. - m).  exp((v - m) - l) then rounds differences of
// order 1, where exp(v - (m + l)) would carry the rounding of a sum of the logits' magnitude (G / temperature at worst)
// into every probability of the row.
struct DslStat {
    float *m, *l;
};
struct DslWork {
    LossWork ns;
    DslStat pc, pr, yr, yc;          // of x per row i / per column j; of yr per row i / of yc per column j
    float *w, *u;
};
__host__ __device__ inline int64_t dsl_work_floats(int G, int Dm) { return loss_work_floats(1, G, Dm) + (int64_t)8 * G; }
__host__ __device__ inline DslWork dsl_carve(float* w, int G, int Dm) {
    DslWork W;
    W.ns = loss_carve(w, 1, G, Dm);
    float* x = w + loss_work_floats(1, G, Dm);
    const int64_t g = G;
    W.pc = {x, x + g};
    W.pr = {x + 2 * g, x + 3 * g};
    W.yr = {x + 4 * g, W.ns.lser};
    W.yc = {x + 5 * g, W.ns.lsec};
    W.w = x + 6 * g;
    W.u = x + 7 * g;
    return W;
}

// l = log(s), correctly rounded (the fp64 logarithm rounded once): 4 G of them per evaluation.  A last-bit difference of a
// prior's l moves every logit of its column by a c P 2^-24 l, hundreds of ulps of a probability at a = G / temperature, so
// the hardware's 1-ulp log2 is not used here (tests/DSL_LOSS_ERROR_BUDGET.md, "the logarithm").
__device__ __forceinline__ float dsl_log(float s) { return (float)log((double)s); }
__device__ __forceinline__ float dsl_x(float c, float T) {
#pragma clang fp contract(off)
    return T * c;
}
// exp((v - m) - l): a prior from x, a probability from y
__device__ __forceinline__ float dsl_p(float v, float m, float l) {
#pragma clang fp contract(off)
    return __expf((v - m) - l);
}
// the logit of one entry: (pm, pl) is the prior statistic of the entry's column (yr) or row (yc)
__device__ __forceinline__ float dsl_y(float c, float T, float a, float pm, float pl) {
#pragma clang fp contract(off)
    return (a * c) * dsl_p(T * c, pm, pl);
}
// gr c Pr (prior of column j, statistic of yr's row i) or gc c Pc (prior of row i, statistic of yc's column j) of one entry
__device__ __forceinline__ float dsl_gcp(float c, bool diag, float T, float a, float pm, float pl, float ym, float yl) {
#pragma clang fp contract(off)
    const float p = dsl_p(T * c, pm, pl);
    const float g = dsl_p((a * c) * p, ym, yl) - (diag ? 1.f : 0.f);
    return (g * c) * p;
}

// single block: G row + G column prior statistics (one thread each), then G row + G column log-sum-exps of y, then the loss.
__global__ void __launch_bounds__(1024) dsl_loss_kernel(DslWork W, float* __restrict__ out, int G, float T, float a) {
#pragma clang fp contract(off)
    __shared__ float sh[16];
    const float* c = W.ns.sim;
    for (int t = threadIdx.x; t < 2 * G; t += blockDim.x) {
        const bool col = t >= G;
        const int u = col ? t - G : t;
        const int64_t base = col ? u : (int64_t)u * G, step = col ? G : 1;
        float m = -INFINITY;
        for (int j = 0; j < G; ++j) m = fmaxf(m, dsl_x(c[base + j * step], T));
        float s = 0.f;
        for (int j = 0; j < G; ++j) s += __expf(dsl_x(c[base + j * step], T) - m);
        const DslStat& st = col ? W.pr : W.pc;
        st.m[u] = m;
        st.l[u] = dsl_log(s);
    }
    __syncthreads();                                          // the statistics of the other axis are read below
    float part = 0.f;
    for (int t = threadIdx.x; t < 2 * G; t += blockDim.x) {
        const bool col = t >= G;
        const int u = col ? t - G : t;
        const int64_t base = col ? u : (int64_t)u * G, step = col ? G : 1;
        const DslStat& p = col ? W.pc : W.pr;                 // a row walks columns j: pr[j]; a column walks rows i: pc[i]
        float m = -INFINITY;
        for (int j = 0; j < G; ++j) m = fmaxf(m, dsl_y(c[base + j * step], T, a, p.m[j], p.l[j]));
        float s = 0.f;
        for (int j = 0; j < G; ++j) s += __expf(dsl_y(c[base + j * step], T, a, p.m[j], p.l[j]) - m);
        const float l = dsl_log(s);
        const DslStat& st = col ? W.yc : W.yr;
        st.m[u] = m;
        st.l[u] = l;
        part += (dsl_y(c[(int64_t)u * G + u], T, a, p.m[u], p.l[u]) - m) - l;
    }
    const float tot = block_reduce(part, sh, false);
    if (threadIdx.x == 0) out[0] = -(tot / (float)G);
}

// The multi-workgroup forward: lse_rows_body / lse_cols_body with the value formed on the fly.  YPASS false: the prior
// statistics of x = T c; true: the log-sum-exp of y and the term (diag - m) - l for ns_finish_kernel.
template <bool YPASS>
__global__ void __launch_bounds__(256) dsl_rows_kernel(DslWork W, int G, float T, float a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= G) return;
    const float* row = W.ns.sim + (int64_t)i * G;
    float m = -INFINITY, s = 0.f;
    for (int j = lane; j < G; j += 64) lse_push(m, s, YPASS ? dsl_y(row[j], T, a, W.pr.m[j], W.pr.l[j]) : dsl_x(row[j], T));
    const float wm = wave_max(m);
    s = wave_sum(m == -INFINITY ? 0.f : s * __expf(m - wm));  // a lane without elements (G < 64)
    if (lane == 0) {
        const float l = dsl_log(s);
        const DslStat& st = YPASS ? W.yr : W.pc;
        st.m[i] = wm;
        st.l[i] = l;
        if (YPASS) W.ns.term[i] = (dsl_y(row[i], T, a, W.pr.m[i], W.pr.l[i]) - wm) - l;
    }
}

template <bool YPASS>
__global__ void __launch_bounds__(64 * LSE_COL_WAVES) dsl_cols_kernel(DslWork W, int G, float T, float a) {
#pragma clang fp contract(off)
    __shared__ float shm[LSE_COL_WAVES][64], shs[LSE_COL_WAVES][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + lane;
    const float* c = W.ns.sim;
    float m = -INFINITY, s = 0.f;
    if (j < G)
        for (int i = wv; i < G; i += LSE_COL_WAVES) {
            const float v = c[(int64_t)i * G + j];
            lse_push(m, s, YPASS ? dsl_y(v, T, a, W.pc.m[i], W.pc.l[i]) : dsl_x(v, T));
        }
    shm[wv][lane] = m;
    shs[wv][lane] = s;
    __syncthreads();
    if (wv != 0 || j >= G) return;
    float bm = shm[0][lane];
#pragma unroll
    for (int w = 1; w < LSE_COL_WAVES; ++w) bm = fmaxf(bm, shm[w][lane]);
    float bs = 0.f;
#pragma unroll
    for (int w = 0; w < LSE_COL_WAVES; ++w)
        if (shm[w][lane] != -INFINITY) bs = __builtin_fmaf(shs[w][lane], __expf(shm[w][lane] - bm), bs);
    const float l = dsl_log(bs);
    const DslStat& st = YPASS ? W.yc : W.pr;
    st.m[j] = bm;
    st.l[j] = l;
    if (YPASS) W.ns.term[G + j] = (dsl_y(c[(int64_t)j * G + j], T, a, W.pc.m[j], W.pc.l[j]) - bm) - l;
}

// backward reductions, one-workgroup form's order: one thread per row (w) / column (u) adds its G terms one after the other
__global__ void __launch_bounds__(64) dsl_uw_kernel(DslWork W, int G, float T, float a) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= 2 * G) return;
    const float* c = W.ns.sim;
    const bool col = t >= G;
    const int u = col ? t - G : t;
    const int64_t base = col ? u : (int64_t)u * G, step = col ? G : 1;
    const DslStat& p = col ? W.pr : W.pc;                     // u[j]: Pr of column j, yr of row i;  w[i]: Pc of row i, yc of column j
    const DslStat& y = col ? W.yr : W.yc;
    const float pm = p.m[u], pl = p.l[u];
    float s = 0.f;
    for (int k = 0; k < G; ++k) s += dsl_gcp(c[base + k * step], k == u, T, a, pm, pl, y.m[k], y.l[k]);
    (col ? W.u : W.w)[u] = s;
}

// the same at a global batch: one wave per row, lanes stride the columns, wave_sum
__global__ void __launch_bounds__(256) dsl_w_rows_kernel(DslWork W, int G, float T, float a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= G) return;
    const float* row = W.ns.sim + (int64_t)i * G;
    const float pm = W.pc.m[i], pl = W.pc.l[i];
    float s = 0.f;
    for (int j = lane; j < G; j += 64) s += dsl_gcp(row[j], j == i, T, a, pm, pl, W.yc.m[j], W.yc.l[j]);
    s = wave_sum(s);
    if (lane == 0) W.w[i] = s;
}

// 64 adjacent columns per workgroup, 16 waves share the rows, the 16 partial sums of a column meet in LDS in wave order
__global__ void __launch_bounds__(64 * LSE_COL_WAVES) dsl_u_cols_kernel(DslWork W, int G, float T, float a) {
#pragma clang fp contract(off)
    __shared__ float shs[LSE_COL_WAVES][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + lane;
    float s = 0.f;
    if (j < G) {
        const float pm = W.pr.m[j], pl = W.pr.l[j];
        for (int i = wv; i < G; i += LSE_COL_WAVES)
            s += dsl_gcp(W.ns.sim[(int64_t)i * G + j], i == j, T, a, pm, pl, W.yr.m[i], W.yr.l[i]);
    }
    shs[wv][lane] = s;
    __syncthreads();
    if (wv != 0 || j >= G) return;
    float bs = 0.f;
#pragma unroll
    for (int w = 0; w < LSE_COL_WAVES; ++w) bs += shs[w][lane];
    W.u[j] = bs;
}

// elementwise: d loss / d c, and its transpose for the second gradient GEMM
__global__ void __launch_bounds__(256) dsl_dsim_kernel(DslWork W, const float* __restrict__ dout, int G, float T, float a,
                                                       float invt) {
#pragma clang fp contract(off)
    const int64_t total = (int64_t)G * G;
    const float scale = dout[0] * invt;                       // dout a / G
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int i = (int)(idx / G), j = (int)(idx - (int64_t)i * G);
        const float c = W.ns.sim[idx], dg = i == j ? 1.f : 0.f;
        const float x = T * c, ac = a * c;
        const float pr = dsl_p(x, W.pr.m[j], W.pr.l[j]), pc = dsl_p(x, W.pc.m[i], W.pc.l[i]);
        const float gr = dsl_p(ac * pr, W.yr.m[i], W.yr.l[i]) - dg, gc = dsl_p(ac * pc, W.yc.m[j], W.yc.l[j]) - dg;
        const float k = 1.f + x;
        const float d = scale * (pr * (gr * k - T * W.u[j]) + pc * (gc * k - T * W.w[i]));
        W.ns.dsim[idx] = d;
        W.ns.dsimT[(int64_t)j * G + i] = d;
    }
}

}  // namespace

// Which focal kernels serve a row layout: the launches below and clv_focal_plan read the same record.
static void focal_plan(bool is16, int V, int64_t ld, uintptr_t logits_addr, uintptr_t dlogits_addr, ClvFocalPlan& p) {
    const bool even = is16 && !(V & 1) && !(ld & 1);
    p.fwd_kernel = !is16 ? 0 : (even && !(logits_addr & 3)) ? 2 : 1;
    p.bwd_kernel = !is16 ? 0 : (even && !((logits_addr | dlogits_addr) & 3)) ? 2 : 1;
    p.fwd_threads = p.fwd_kernel == 2 ? FC_WIDE : FC_THREADS;
    p.bwd_threads = p.bwd_kernel == 2 ? FC_WIDE : FC_THREADS;
    const int n = p.fwd_kernel == 2 ? V >> 1 : V;                      // accesses per row
    p.fwd_trips = (n + p.fwd_threads - 1) / p.fwd_threads;
    const int waves = p.fwd_threads / 64, busy = (n + 63) / 64;
    p.fwd_waves_with_work = busy < waves ? busy : waves;
}

extern "C" int clv_focal_plan(int32_t is_16bit, int32_t V, int64_t ld, int32_t logits_align, int32_t dlogits_align,
                              ClvFocalPlan* out) {
    if (!out || V <= 0 || ld < V || logits_align < 0 || dlogits_align < 0) return CLV_ERR_ARG;
    focal_plan(is_16bit != 0, V, ld, (uintptr_t)logits_align, (uintptr_t)dlogits_align, *out);
    return 0;
}

static int focal_fwd_impl(const void* logits, int32_t is_bf16, const int64_t* labels, float* row_ce, float* row_lse,
                          float* loss, float* count, int64_t rows, int32_t V, int64_t ld, float gamma, void* stream) {
    if (!logits || !labels || !row_ce || !row_lse || !loss || !count || rows <= 0 || V <= 0 || ld < V) return CLV_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    ClvFocalPlan pl;
    focal_plan(is_bf16 != 0, V, ld, reinterpret_cast<uintptr_t>(logits), 0, pl);
    // (loss, count) double as the {sum, count} accumulators (caller zeroes both); normalised in place
    // by the finish kernel
    if (pl.fwd_kernel == 2)
        hipLaunchKernelGGL(focal_fwd_pairs_kernel, dim3((unsigned)rows), dim3(FC_WIDE), 0, st, (const unsigned*)logits,
                           labels, row_ce, row_lse, loss, count, (int)V, ld, gamma);
    else if (pl.fwd_kernel == 1)
        hipLaunchKernelGGL((focal_fwd_kernel<true>), dim3((unsigned)rows), dim3(FC_THREADS), 0, st, logits, labels,
                           row_ce, row_lse, loss, count, (int)V, ld, gamma);
    else
        hipLaunchKernelGGL((focal_fwd_kernel<false>), dim3((unsigned)rows), dim3(FC_THREADS), 0, st, logits, labels,
                           row_ce, row_lse, loss, count, (int)V, ld, gamma);
    int rc = clv_check_launch();
    if (rc) return rc;
    hipLaunchKernelGGL(focal_finish_kernel, dim3(1), dim3(1), 0, st, loss, (const float*)count);
    return clv_check_launch();
}

static int focal_bwd_impl(const void* logits, int32_t is_bf16, const int64_t* labels, const float* row_ce,
                          const float* row_lse, const float* count, const float* dloss, void* dlogits, int64_t rows, int32_t V,
                          int64_t ld, float gamma, void* stream) {
    if (!logits || !labels || !row_ce || !row_lse || !count || !dloss || !dlogits || rows <= 0 || V <= 0 || ld < V)
        return CLV_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    ClvFocalPlan pl;
    focal_plan(is_bf16 != 0, V, ld, reinterpret_cast<uintptr_t>(logits), reinterpret_cast<uintptr_t>(dlogits), pl);
    if (pl.bwd_kernel == 2)
        hipLaunchKernelGGL(focal_bwd_pairs_kernel, dim3((unsigned)rows), dim3(FC_WIDE), 0, st, (const unsigned*)logits,
                           labels, row_ce, row_lse, count, dloss, (unsigned*)dlogits, (int)V, ld, gamma);
    else if (pl.bwd_kernel == 1)
        hipLaunchKernelGGL((focal_bwd_kernel<true>), dim3((unsigned)rows), dim3(FC_THREADS), 0, st, logits, labels,
                           row_ce, row_lse, count, dloss, dlogits, (int)V, ld, gamma);
    else
        hipLaunchKernelGGL((focal_bwd_kernel<false>), dim3((unsigned)rows), dim3(FC_THREADS), 0, st, logits, labels,
                           row_ce, row_lse, count, dloss, dlogits, (int)V, ld, gamma);
    return clv_check_launch();
}

extern "C" int clv_focal_ce_fwd(const void* logits, int32_t is_bf16, const int64_t* labels, float* row_ce,
                                float* row_lse, float* loss, float* count, int64_t rows, int32_t V, float gamma,
                                void* stream) {
    return focal_fwd_impl(logits, is_bf16, labels, row_ce, row_lse, loss, count, rows, V, V, gamma, stream);
}

extern "C" int clv_focal_ce_bwd(const void* logits, int32_t is_bf16, const int64_t* labels, const float* row_ce,
                                const float* row_lse, const float* count, const float* dloss, void* dlogits,
                                int64_t rows, int32_t V, float gamma, void* stream) {
    return focal_bwd_impl(logits, is_bf16, labels, row_ce, row_lse, count, dloss, dlogits, rows, V, V, gamma, stream);
}

// The same on rows of stride ld >= V elements (logits and dlogits alike): the padded [rows, ld] score buffer the MLM decoder
// GEMM writes (V = 30522 is not a multiple of 8; ld = 30528 is).  The backward ZEROES the padding columns [V, ld) of dlogits,
// so that the decoder's input- and weight-gradient GEMMs can contract over ld.
extern "C" int clv_focal_ce_fwd_ld(const void* logits, int32_t is_bf16, const int64_t* labels, float* row_ce,
                                   float* row_lse, float* loss, float* count, int64_t rows, int32_t V, int64_t ld,
                                   float gamma, void* stream) {
    return focal_fwd_impl(logits, is_bf16, labels, row_ce, row_lse, loss, count, rows, V, ld, gamma, stream);
}

extern "C" int clv_focal_ce_bwd_ld(const void* logits, int32_t is_bf16, const int64_t* labels, const float* row_ce,
                                   const float* row_lse, const float* count, const float* dloss, void* dlogits,
                                   int64_t rows, int32_t V, int64_t ld, float gamma, void* stream) {
    return focal_bwd_impl(logits, is_bf16, labels, row_ce, row_lse, count, dloss, dlogits, rows, V, ld, gamma, stream);
}

extern "C" int64_t clv_infonce_work_floats(int32_t G, int32_t Dm) { return loss_work_floats(3, G, Dm); }

// one thread per exclusive row / column (6 G of them): whole waves, at most the kernel's 1024 (a per-rank batch of 8 needs one)
static int nce_loss_threads(int G) {
    const int t = (6 * G + 63) / 64 * 64;
    return t < 64 ? 64 : (t > 1024 ? 1024 : t);
}

// The loss section at and above this many rows takes the multi-workgroup path (log-sum-exp kernels over the device, LDS-tiled
// GEMMs); below it the one-workgroup kernels, unchanged.  Measured (tools/virtual_ranks_bench.py, DESIGN section 5: forward +
// backward of the pair form, Dm = 768, old / new): as one hipGraph replay 0.89 x at G = 16, 1.02 x at 32, 1.17 x at 64,
// 1.83 x at 128, 4.2 x at 256, 19 x at 1024; issued eagerly, as the engine's loss section issues it (the new forward is five
// launches where the old one is three), 0.98 x at 32, 0.96 x at 64, 1.25 x at 128, 3.3 x at 256, 19 x at 1024.  The crossover
// of the eager form lies between 64 and 128: the threshold is the smallest size measured at which both forms are ahead.
constexpr int NCE_LARGE_MIN_G = 128;

// Which kernel a GEMM of the loss section takes: nce_gemm launches by this record and clv_loss_gemm_plan returns it.
static void loss_gemm_plan(int M, int N, int K, int lda, int ldb, int batch, int64_t sA, int64_t sB, int64_t s2,
                           uintptr_t a_addr, uintptr_t b_addr, bool tiled, ClvLossGemmPlan& p) {
    p.k_tail = K % 16;
    if (tiled) {
        p.gx = (N + LT_BN - 1) / LT_BN;
        p.gy = (M + LT_BM - 1) / LT_BM;
        const bool vec = K % LT_BK == 0 && lda % 4 == 0 && ldb % 4 == 0 && sA % 4 == 0 && sB % 4 == 0 && s2 % 4 == 0 &&
                         a_addr % 16 == 0 && b_addr % 16 == 0;
        p.kernel = vec ? 2 : 3;
        p.waves = p.waves_with_work = 4;
        p.kchunk = LT_BK;
    } else {
        p.gx = (N + 15) / 16;
        p.gy = (M + 15) / 16;
        // few tiles (per evaluation), long contraction: 8 waves share a tile
        const bool wide = K >= 256 && (int64_t)p.gx * p.gy * batch <= 512;
        p.kernel = wide ? 1 : 0;
        p.waves = wide ? 8 : 1;
        p.kchunk = sgemm_kchunk(K, p.waves);
        const int busy = (K + p.kchunk - 1) / p.kchunk;
        p.waves_with_work = busy < p.waves ? busy : p.waves;
    }
    p.tiles = (int32_t)((int64_t)p.gx * p.gy * batch);
}

extern "C" int clv_loss_gemm_plan(int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldb, int32_t batch, int64_t sA,
                                  int64_t sB, int64_t s2, int32_t a_align, int32_t b_align, int32_t tiled,
                                  ClvLossGemmPlan* out) {
    if (!out || M <= 0 || N <= 0 || K <= 0 || lda < K || ldb < K || batch <= 0 || a_align < 0 || b_align < 0)
        return CLV_ERR_ARG;
    loss_gemm_plan(M, N, K, lda, ldb, batch, sA, sB, s2, (uintptr_t)a_align, (uintptr_t)b_align, tiled != 0, *out);
    return 0;
}

static int nce_gemm(const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc,
                    int batch, int64_t sA, int64_t sB, int64_t sC, float alpha, hipStream_t st, int outer = 1,
                    int64_t s2 = 0, bool tiled = false) {
    ClvLossGemmPlan pl;
    loss_gemm_plan(M, N, K, lda, ldb, batch, sA, sB, s2, reinterpret_cast<uintptr_t>(A), reinterpret_cast<uintptr_t>(B),
                   tiled, pl);
    const dim3 grid(pl.gx, pl.gy, batch * outer);
    if (pl.kernel == 2)
        hipLaunchKernelGGL(sgemm_nt_tiled_kernel<true>, grid, dim3(256), 0, st, A, B, C, M, N, K, lda, ldb, ldc, sA, sB,
                           sC, alpha, batch, s2);
    else if (pl.kernel == 3)
        hipLaunchKernelGGL(sgemm_nt_tiled_kernel<false>, grid, dim3(256), 0, st, A, B, C, M, N, K, lda, ldb, ldc, sA, sB,
                           sC, alpha, batch, s2);
    else if (pl.kernel == 1)
        hipLaunchKernelGGL(sgemm_nt_kernel<8>, grid, dim3(512), 0, st, A, B, C, M, N, K, lda, ldb, ldc, sA, sB, sC, alpha,
                           batch, s2);
    else
        hipLaunchKernelGGL(sgemm_nt_kernel<1>, grid, dim3(64), 0, st, A, B, C, M, N, K, lda, ldb, ldc, sA, sB, sC, alpha,
                           batch, s2);
    return clv_check_launch();
}

// The three GEMMs of an evaluation on a carved work area with nb score blocks.  which: 0 the
// scores en0 . en_{k+1}^T, 1 d en0 = dsim . en_{1..nb} (contraction nb * G), 2 d en_{k+1} = dsimT[k] . en0 (contraction G).
// The launches and the plan entries both come through here.
struct LossGemmArgs {
    int64_t oA, oB, oC;                        // operand offsets (floats) from the start of the work area
    int M, N, K, lda, ldb, ldc, batch;
    int64_t sA, sB, sC;
};
static LossGemmArgs loss_gemm_args(int which, int nb, int G, int Dm) {
    const LossWorkOff o = loss_work_off(nb, G, Dm);
    const int64_t GD = (int64_t)G * Dm, GG = (int64_t)G * G;
    const bool many = nb > 1;
    if (which == 0) return {o.en, o.en + GD, o.sim, G, G, Dm, Dm, Dm, G, nb, 0, many ? GD : 0, many ? GG : 0};
    // d en0[i][d] = sum_{k,j} dsim[i][(k,j)] * en_{k+1}[j][d] / T :  A = dsim [G][nb G], B = enT[d][(k+1, j)]
    if (which == 1) return {o.dsim, o.enT + G, o.den, G, Dm, nb * G, nb * G, (nb + 1) * G, Dm, 1, 0, 0, 0};
    // d en_{k+1}[j][d] = sum_i dsimT[k][j][i] * en0[i][d] / T   :  A = dsimT[k] [G][G], B = enT[d][(0, i)]
    return {o.dsimT, o.enT, o.den + GD, G, Dm, G, G, (nb + 1) * G, Dm, nb, many ? GG : 0, 0, many ? GD : 0};
}
static int loss_gemm(const LossWork& W, int which, int nb, int G, int Dm, float alpha, hipStream_t st, int outer,
                     int64_t s2, bool tiled) {
    const LossGemmArgs a = loss_gemm_args(which, nb, G, Dm);
    float* work = W.en;                        // the work area starts with en
    return nce_gemm(work + a.oA, work + a.oB, work + a.oC, a.M, a.N, a.K, a.lda, a.ldb, a.ldc, a.batch, a.sA, a.sB, a.sC,
                    alpha, st, outer, s2, tiled);
}

// The grid of an elementwise d loss / d sim kernel over nb G x G scores (256 threads, grid-stride above 1024 workgroups).
static int loss_dsim_grid(int nb, int G) {
    const int64_t grid = ((int64_t)nb * G * G + 255) / 256;
    return grid > 1024 ? 1024 : (int)grid;
}

// The two gradient GEMMs after d loss / d sim: d en0 (GEMM 1), d en_{k+1} (GEMM 2).  outer / s2: as nce_gemm.
static int loss_bwd_gemms(const LossWork& W, int nb, int G, int Dm, float alpha, hipStream_t st, int outer, int64_t s2,
                          bool large) {
    const int rc = loss_gemm(W, 1, nb, G, Dm, alpha, st, outer, s2, large);
    return rc ? rc : loss_gemm(W, 2, nb, G, Dm, alpha, st, outer, s2, large);
}

// The backward tail of one evaluation: the two GEMMs, then the strided norm backward into NE gradients of row stride ldd
// (InfoNCE: <4, false>; NormSoftmax and the dual-softmax loss: <2, true>, d2 and d3 unused).
template <int NE, bool MARK>
static int loss_bwd_tail(const LossWork& W, int G, int Dm, float alpha, hipStream_t st, bool large, float* d0, float* d1,
                         float* d2, float* d3, int ldd) {
    const int rc = loss_bwd_gemms(W, NE - 1, G, Dm, alpha, st, 1, 0, large);
    if (rc) return rc;
    hipLaunchKernelGGL((norm_bwd_kernel<NE, MARK>), dim3((NE * G + 3) / 4), dim3(256), 0, st, W, d0, d1, d2, d3, G, Dm, ldd);
    return clv_check_launch();
}

// Launch shapes of the loss kernels between the GEMMs; the forwards below launch by this record.
static void loss_kernels_plan(int G, int nb, bool large, ClvLossPlan& p) {
    p.large = large;
    p.loss_threads = p.loss_trips = p.rows_grid = p.cols_gx = p.cols_gy = p.finish_threads = p.cols_last = 0;
    p.idle_row_lanes = p.idle_col_waves = 0;
    if (!large) {
        p.loss_threads = nb == 3 ? nce_loss_threads(G) : 1024;
        p.loss_trips = (2 * nb * G + p.loss_threads - 1) / p.loss_threads;
        return;
    }
    p.rows_grid = (nb * G + 3) / 4;
    p.cols_gx = (G + 63) / 64;
    p.cols_gy = nb;
    p.finish_threads = 256;
    p.cols_last = G - 64 * (p.cols_gx - 1);
    p.idle_row_lanes = G < 64 ? 64 - G : 0;
    p.idle_col_waves = G < LSE_COL_WAVES ? LSE_COL_WAVES - G : 0;
}

// For a work area at a 16-byte boundary: operand addresses modulo 16 follow from the offsets.
static void loss_section_plan(int nb, int G, int Dm, int64_t s2, bool large, bool gemms, ClvLossPlan& p) {
    loss_kernels_plan(G, nb, large, p);
    ClvLossGemmPlan* g[3] = {&p.fwd, &p.bwd0, &p.bwd1};
    for (int which = 0; which < 3; ++which) {
        *g[which] = ClvLossGemmPlan{};
        if (!gemms) continue;
        const LossGemmArgs a = loss_gemm_args(which, nb, G, Dm);
        loss_gemm_plan(a.M, a.N, a.K, a.lda, a.ldb, a.batch, a.sA, a.sB, s2, (uintptr_t)(a.oA * 4), (uintptr_t)(a.oB * 4),
                       large, *g[which]);
    }
}

// The GEMM batch stride between the work areas of InfoNCE's nd directions (1: the four-tensor entries, 2: the pair entries).
static int64_t nce_dir_stride(int nd, int G, int Dm) { return nd > 1 ? loss_work_floats(3, G, Dm) : 0; }

// ld is checked as the entry checks it; no launch class depends on it
extern "C" int clv_infonce_plan(int32_t G, int32_t Dm, int32_t ld, int32_t pair, int32_t large, ClvLossPlan* out) {
    if (!out || G <= 0 || Dm <= 0 || ld < Dm) return CLV_ERR_ARG;
    loss_section_plan(3, G, Dm, nce_dir_stride(pair ? 2 : 1, G, Dm), large != 0, true, *out);
    return 0;
}

extern "C" int clv_normsoftmax_plan(int32_t G, int32_t Dm, int32_t sim_mat, int32_t large, ClvLossPlan* out) {
    if (!out || G <= 0 || (!sim_mat && Dm <= 0)) return CLV_ERR_ARG;
    loss_section_plan(1, G, Dm > 0 ? Dm : 1, 0, large != 0, !sim_mat, *out);
    return 0;
}

extern "C" int32_t clv_infonce_large_min_g(void) { return NCE_LARGE_MIN_G; }

// The launches of InfoNCE on nd directions: 1 for the four-tensor entries (direction 0 of P alone), 2 for the packed pair
// entries.
static int infonce_fwd_impl(const NcePair& P, int nd, float* out, int G, int Dm, int ld, float temperature, float margin,
                            hipStream_t st, bool large) {
    const LossWork& W = P.w[0];
    const bool one = nd == 1;
    if (one)
        hipLaunchKernelGGL(nce_normalize_kernel, dim3((4 * G + 3) / 4), dim3(256), 0, st, P.e[0][0], P.e[0][1], P.e[0][2],
                           P.e[0][3], W, G, Dm, ld);
    else
        hipLaunchKernelGGL(nce_pair_normalize_kernel, dim3((4 * G + 3) / 4, nd), dim3(256), 0, st, P, G, Dm, ld);
    int rc = clv_check_launch();
    if (rc) return rc;
    // sim[k] = en0 . en_{k+1}^T / temperature
    rc = loss_gemm(W, 0, 3, G, Dm, 1.0f / temperature, st, nd, nce_dir_stride(nd, G, Dm), large);
    if (rc) return rc;
    ClvLossPlan pl;
    loss_kernels_plan(G, 3, large, pl);
    if (!large) {
        if (one) hipLaunchKernelGGL(nce_loss_kernel, dim3(1), dim3(pl.loss_threads), 0, st, W, out, G, margin);
        else hipLaunchKernelGGL(nce_pair_loss_kernel, dim3(nd), dim3(pl.loss_threads), 0, st, P, out, G, margin);
        return clv_check_launch();
    }
    if (one) hipLaunchKernelGGL(nce_lse_rows_kernel, dim3(pl.rows_grid), dim3(256), 0, st, W, G);
    else hipLaunchKernelGGL(nce_pair_lse_rows_kernel, dim3(pl.rows_grid, nd), dim3(256), 0, st, P, G);
    if ((rc = clv_check_launch())) return rc;
    const dim3 colt(64 * LSE_COL_WAVES);
    if (one) hipLaunchKernelGGL(nce_lse_cols_kernel, dim3(pl.cols_gx, pl.cols_gy), colt, 0, st, W, G);
    else hipLaunchKernelGGL(nce_pair_lse_cols_kernel, dim3(pl.cols_gx, pl.cols_gy, nd), colt, 0, st, P, G);
    if ((rc = clv_check_launch())) return rc;
    if (one) hipLaunchKernelGGL(nce_finish_kernel, dim3(1), dim3(pl.finish_threads), 0, st, W, out, G, margin);
    else hipLaunchKernelGGL(nce_pair_finish_kernel, dim3(nd), dim3(pl.finish_threads), 0, st, P, out, G, margin);
    return clv_check_launch();
}

static int infonce_single_fwd(const float* e0, const float* e1, const float* e2, const float* e3, float* out,
                              float* work, int32_t G, int32_t Dm, int32_t ld, float temperature, float margin,
                              void* stream, bool large) {
    if (!e0 || !e1 || !e2 || !e3 || !out || !work || G <= 0 || Dm <= 0 || ld < Dm || temperature <= 0.f)
        return CLV_ERR_ARG;
    NcePair P{};                               // direction 0 alone
    P.w[0] = loss_carve(work, 3, G, Dm);
    P.e[0][0] = e0;
    P.e[0][1] = e1;
    P.e[0][2] = e2;
    P.e[0][3] = e3;
    return infonce_fwd_impl(P, 1, out, G, Dm, ld, temperature, margin, (hipStream_t)stream, large);
}

extern "C" int clv_infonce_fwd(const float* e0, const float* e1, const float* e2, const float* e3, float* out,
                               float* work, int32_t G, int32_t Dm, int32_t ld, float temperature, float margin,
                               void* stream) {
    return infonce_single_fwd(e0, e1, e2, e3, out, work, G, Dm, ld, temperature, margin, stream, false);
}
extern "C" int clv_infonce_fwd_large(const float* e0, const float* e1, const float* e2, const float* e3, float* out,
                                     float* work, int32_t G, int32_t Dm, int32_t ld, float temperature, float margin,
                                     void* stream) {
    return infonce_single_fwd(e0, e1, e2, e3, out, work, G, Dm, ld, temperature, margin, stream, true);
}

static int infonce_single_bwd(const float* dout, const float* work, float* d0, float* d1, float* d2, float* d3, int32_t G,
                              int32_t Dm, int32_t ldd, float temperature, float margin, void* stream, bool large) {
    if (!dout || !work || !d0 || !d1 || !d2 || !d3 || G <= 0 || Dm <= 0 || ldd < Dm) return CLV_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const LossWork W = loss_carve(const_cast<float*>(work), 3, G, Dm);
    hipLaunchKernelGGL(nce_dsim_kernel, dim3(loss_dsim_grid(3, G)), dim3(256), 0, st, W, dout, (int)G, margin);
    const int rc = clv_check_launch();
    if (rc) return rc;
    return loss_bwd_tail<4, false>(W, G, Dm, 1.0f / temperature, st, large, d0, d1, d2, d3, ldd);
}

extern "C" int clv_infonce_bwd(const float* e0, const float* e1, const float* e2, const float* e3, const float* dout,
                               const float* work, float* d0, float* d1, float* d2, float* d3, int32_t G, int32_t Dm,
                               int32_t ldd, float temperature, float margin, void* stream) {
    return infonce_single_bwd(dout, work, d0, d1, d2, d3, G, Dm, ldd, temperature, margin, stream, false);
}
extern "C" int clv_infonce_bwd_large(const float* e0, const float* e1, const float* e2, const float* e3, const float* dout,
                                     const float* work, float* d0, float* d1, float* d2, float* d3, int32_t G, int32_t Dm,
                                     int32_t ldd, float temperature, float margin, void* stream) {
    return infonce_single_bwd(dout, work, d0, d1, d2, d3, G, Dm, ldd, temperature, margin, stream, true);
}

static bool nce_pair_setup(NcePair& P, const float* packed, float* work, const int32_t* slots, int G, int k, int Dm) {
    const int64_t ws = loss_work_floats(3, G, Dm);
    for (int d = 0; d < 2; ++d) {
        P.w[d] = loss_carve(work + d * ws, 3, G, Dm);
        for (int q = 0; q < 4; ++q) {
            const int sl = slots[d * 4 + q];
            if (sl < 0 || sl >= k) return false;
            for (int r = 0; r < q; ++r)
                if (slots[d * 4 + r] == sl) return false;               // the four slots of a direction are distinct
            P.slot[d][q] = sl;
            P.e[d][q] = packed ? packed + (int64_t)sl * Dm : nullptr;
        }
    }
    for (int q = 0; q < 4; ++q) P.dout[q] = nullptr;
    return true;
}

static int infonce_pair_fwd(const float* packed, const int32_t* slots, float* out, float* work, int32_t G, int32_t k,
                            int32_t Dm, float temperature, float margin, void* stream, bool large) {
    if (!packed || !slots || !out || !work || G <= 0 || k < 4 || Dm <= 0 || temperature <= 0.f) return CLV_ERR_ARG;
    NcePair P;
    if (!nce_pair_setup(P, packed, work, slots, G, k, Dm)) return CLV_ERR_ARG;
    return infonce_fwd_impl(P, 2, out, G, Dm, k * Dm, temperature, margin, (hipStream_t)stream, large);
}

extern "C" int clv_infonce_pair_fwd(const float* packed, const int32_t* slots, float* out, float* work, int32_t G,
                                    int32_t k, int32_t Dm, float temperature, float margin, void* stream) {
    return infonce_pair_fwd(packed, slots, out, work, G, k, Dm, temperature, margin, stream, false);
}
extern "C" int clv_infonce_pair_fwd_large(const float* packed, const int32_t* slots, float* out, float* work, int32_t G,
                                          int32_t k, int32_t Dm, float temperature, float margin, void* stream) {
    return infonce_pair_fwd(packed, slots, out, work, G, k, Dm, temperature, margin, stream, true);
}

static int infonce_pair_bwd(const float* const* dout, const float* work, const int32_t* slots, float* dpacked, int32_t G,
                            int32_t k, int32_t Dm, float temperature, float margin, void* stream, bool large) {
    if (!dout || !work || !slots || !dpacked || G <= 0 || k < 4 || Dm <= 0 || temperature <= 0.f) return CLV_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    NcePair P;
    if (!nce_pair_setup(P, nullptr, const_cast<float*>(work), slots, G, k, Dm)) return CLV_ERR_ARG;
    for (int q = 0; q < 4; ++q) P.dout[q] = dout[q];
    hipLaunchKernelGGL(nce_pair_dsim_kernel, dim3(loss_dsim_grid(3, G), 2), dim3(256), 0, st, P, (int)G, margin);
    int rc = clv_check_launch();
    if (rc) return rc;
    rc = loss_bwd_gemms(P.w[0], 3, G, Dm, 1.0f / temperature, st, 2, nce_dir_stride(2, G, Dm), large);
    if (rc) return rc;
    hipLaunchKernelGGL(nce_pair_norm_bwd_kernel, dim3((k * G + 3) / 4), dim3(256), 0, st, P, dpacked, (int)G, (int)k,
                       (int)Dm);
    return clv_check_launch();
}

extern "C" int clv_infonce_pair_bwd(const float* const* dout, const float* work, const int32_t* slots, float* dpacked,
                                    int32_t G, int32_t k, int32_t Dm, float temperature, float margin, void* stream) {
    return infonce_pair_bwd(dout, work, slots, dpacked, G, k, Dm, temperature, margin, stream, false);
}
extern "C" int clv_infonce_pair_bwd_large(const float* const* dout, const float* work, const int32_t* slots,
                                          float* dpacked, int32_t G, int32_t k, int32_t Dm, float temperature, float margin,
                                          void* stream) {
    return infonce_pair_bwd(dout, work, slots, dpacked, G, k, Dm, temperature, margin, stream, true);
}

extern "C" int64_t clv_normsoftmax_work_floats(int32_t G, int32_t Dm) { return loss_work_floats(1, G, Dm > 0 ? Dm : 1); }

static int normsoftmax_fwd_impl(const float* video, const float* text, const float* sim_mat, float* out,
                                float* work, int32_t G, int32_t Dm, float temperature, float eps, void* stream,
                                bool large) {
    if (!out || !work || G <= 0) return CLV_ERR_ARG;
    if (!sim_mat && (!video || !text || Dm <= 0 || temperature <= 0.f || eps <= 0.f)) return CLV_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    LossWork W = loss_carve(work, 1, G, Dm > 0 ? Dm : 1);
    if (!sim_mat) {
        hipLaunchKernelGGL(ns_normalize_kernel, dim3((2 * G + 3) / 4), dim3(256), 0, st, video, text, W, (int)G, (int)Dm,
                           eps);
        int rc = clv_check_launch();
        if (rc) return rc;
        rc = loss_gemm(W, 0, 1, G, Dm, 1.0f / temperature, st, 1, 0, large);
        if (rc) return rc;
    }
    const float* sim = sim_mat ? sim_mat : (const float*)W.sim;
    ClvLossPlan pl;
    loss_kernels_plan(G, 1, large, pl);
    if (!large) {
        hipLaunchKernelGGL(ns_loss_kernel, dim3(1), dim3(pl.loss_threads), 0, st, W, sim, out, (int)G);
        return clv_check_launch();
    }
    hipLaunchKernelGGL(ns_lse_rows_kernel, dim3(pl.rows_grid), dim3(256), 0, st, W, sim, (int)G);
    int rc = clv_check_launch();
    if (rc) return rc;
    hipLaunchKernelGGL(ns_lse_cols_kernel, dim3(pl.cols_gx, pl.cols_gy), dim3(64 * LSE_COL_WAVES), 0, st, W, sim, (int)G);
    if ((rc = clv_check_launch())) return rc;
    hipLaunchKernelGGL(ns_finish_kernel, dim3(1), dim3(pl.finish_threads), 0, st, W, out, (int)G);
    return clv_check_launch();
}

extern "C" int clv_normsoftmax_fwd(const float* video, const float* text, const float* sim_mat, float* out,
                                   float* work, int32_t G, int32_t Dm, float temperature, float eps, void* stream) {
    return normsoftmax_fwd_impl(video, text, sim_mat, out, work, G, Dm, temperature, eps, stream, false);
}
extern "C" int clv_normsoftmax_fwd_large(const float* video, const float* text, const float* sim_mat, float* out,
                                         float* work, int32_t G, int32_t Dm, float temperature, float eps, void* stream) {
    return normsoftmax_fwd_impl(video, text, sim_mat, out, work, G, Dm, temperature, eps, stream, true);
}

static int normsoftmax_bwd_impl(const float* sim_mat, const float* dout, const float* work, float* dvideo,
                                float* dtext, float* dsim, int32_t G, int32_t Dm, float temperature, void* stream,
                                bool large) {
    if (!dout || !work || G <= 0) return CLV_ERR_ARG;
    if (sim_mat ? !dsim : (!dvideo || !dtext || Dm <= 0 || temperature <= 0.f)) return CLV_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    LossWork W = loss_carve(const_cast<float*>(work), 1, G, Dm > 0 ? Dm : 1);
    hipLaunchKernelGGL(ns_dsim_kernel, dim3(loss_dsim_grid(1, G)), dim3(256), 0, st, W,
                       sim_mat ? sim_mat : (const float*)W.sim, dout, sim_mat ? dsim : W.dsim, (int)G);
    const int rc = clv_check_launch();
    if (rc || sim_mat) return rc;
    // d en_v[i][d] = sum_j dsim[i][j] en_t[j][d] / t ;  d en_t[j][d] = sum_i dsim[i][j] en_v[i][d] / t
    return loss_bwd_tail<2, true>(W, G, Dm, 1.0f / temperature, st, large, dvideo, dtext, nullptr, nullptr, Dm);
}

extern "C" int clv_normsoftmax_bwd(const float* sim_mat, const float* dout, const float* work, float* dvideo,
                                   float* dtext, float* dsim, int32_t G, int32_t Dm, float temperature,
                                   void* stream) {
    return normsoftmax_bwd_impl(sim_mat, dout, work, dvideo, dtext, dsim, G, Dm, temperature, stream, false);
}
extern "C" int clv_normsoftmax_bwd_large(const float* sim_mat, const float* dout, const float* work, float* dvideo,
                                         float* dtext, float* dsim, int32_t G, int32_t Dm, float temperature,
                                         void* stream) {
    return normsoftmax_bwd_impl(sim_mat, dout, work, dvideo, dtext, dsim, G, Dm, temperature, stream, true);
}

// ------------------------------------------------------------------------------------------------- dual-softmax loss
extern "C" int64_t clv_dsl_loss_work_floats(int32_t G, int32_t Dm) { return dsl_work_floats(G, Dm > 0 ? Dm : 1); }

// The launch shapes and the three GEMM classes are those of NormSoftmax on embeddings: the same record.
extern "C" int clv_dsl_loss_plan(int32_t G, int32_t Dm, int32_t large, ClvLossPlan* out) {
    if (!out || G <= 0 || Dm <= 0) return CLV_ERR_ARG;
    loss_section_plan(1, G, Dm, 0, large != 0, true, *out);
    return 0;
}

static bool dsl_prior_ok(float T) { return T >= 0.f && T <= 3.4e38f; }      // false for NaN and inf

static int dsl_fwd_impl(const float* video, const float* text, float* out, float* work, int32_t G, int32_t Dm,
                        float temperature, float eps, float T, void* stream, bool large) {
    if (!video || !text || !out || !work || G <= 0 || Dm <= 0 || temperature <= 0.f || eps <= 0.f || !dsl_prior_ok(T))
        return CLV_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    DslWork W = dsl_carve(work, G, Dm);
    hipLaunchKernelGGL(ns_normalize_kernel, dim3((2 * G + 3) / 4), dim3(256), 0, st, video, text, W.ns, (int)G, (int)Dm, eps);
    int rc = clv_check_launch();
    if (rc) return rc;
    rc = loss_gemm(W.ns, 0, 1, G, Dm, 1.0f, st, 1, 0, large);             // the cosine: 1 / temperature is folded into a
    if (rc) return rc;
    const float a = (float)G / temperature;
    ClvLossPlan pl;
    loss_kernels_plan(G, 1, large, pl);
    if (!large) {
        hipLaunchKernelGGL(dsl_loss_kernel, dim3(1), dim3(pl.loss_threads), 0, st, W, out, (int)G, T, a);
        return clv_check_launch();
    }
    const dim3 cols(pl.cols_gx, pl.cols_gy), colt(64 * LSE_COL_WAVES);
    hipLaunchKernelGGL(dsl_rows_kernel<false>, dim3(pl.rows_grid), dim3(256), 0, st, W, (int)G, T, a);
    if ((rc = clv_check_launch())) return rc;
    hipLaunchKernelGGL(dsl_cols_kernel<false>, cols, colt, 0, st, W, (int)G, T, a);
    if ((rc = clv_check_launch())) return rc;
    hipLaunchKernelGGL(dsl_rows_kernel<true>, dim3(pl.rows_grid), dim3(256), 0, st, W, (int)G, T, a);
    if ((rc = clv_check_launch())) return rc;
    hipLaunchKernelGGL(dsl_cols_kernel<true>, cols, colt, 0, st, W, (int)G, T, a);
    if ((rc = clv_check_launch())) return rc;
    hipLaunchKernelGGL(ns_finish_kernel, dim3(1), dim3(pl.finish_threads), 0, st, W.ns, out, (int)G);
    return clv_check_launch();
}

extern "C" int clv_dsl_loss_fwd(const float* video, const float* text, float* out, float* work, int32_t G, int32_t Dm,
                                float temperature, float eps, float dual_softmax, void* stream) {
    return dsl_fwd_impl(video, text, out, work, G, Dm, temperature, eps, dual_softmax, stream, false);
}
extern "C" int clv_dsl_loss_fwd_large(const float* video, const float* text, float* out, float* work, int32_t G,
                                      int32_t Dm, float temperature, float eps, float dual_softmax, void* stream) {
    return dsl_fwd_impl(video, text, out, work, G, Dm, temperature, eps, dual_softmax, stream, true);
}

static int dsl_bwd_impl(const float* dout, const float* work, float* dvideo, float* dtext, int32_t G, int32_t Dm,
                        float temperature, float T, void* stream, bool large) {
    if (!dout || !work || !dvideo || !dtext || G <= 0 || Dm <= 0 || temperature <= 0.f || !dsl_prior_ok(T))
        return CLV_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    DslWork W = dsl_carve(const_cast<float*>(work), G, Dm);
    const float a = (float)G / temperature;
    ClvLossPlan pl;
    loss_kernels_plan(G, 1, large, pl);
    int rc;
    if (!large) {
        hipLaunchKernelGGL(dsl_uw_kernel, dim3((2 * G + 63) / 64), dim3(64), 0, st, W, (int)G, T, a);
        if ((rc = clv_check_launch())) return rc;
    } else {
        hipLaunchKernelGGL(dsl_w_rows_kernel, dim3(pl.rows_grid), dim3(256), 0, st, W, (int)G, T, a);
        if ((rc = clv_check_launch())) return rc;
        hipLaunchKernelGGL(dsl_u_cols_kernel, dim3(pl.cols_gx, pl.cols_gy), dim3(64 * LSE_COL_WAVES), 0, st, W, (int)G, T, a);
        if ((rc = clv_check_launch())) return rc;
    }
    hipLaunchKernelGGL(dsl_dsim_kernel, dim3(loss_dsim_grid(1, G)), dim3(256), 0, st, W, dout, (int)G, T, a,
                       1.0f / temperature);
    if ((rc = clv_check_launch())) return rc;
    // d en_v[i][d] = sum_j dc[i][j] en_t[j][d] ;  d en_t[j][d] = sum_i dc[i][j] en_v[i][d]
    return loss_bwd_tail<2, true>(W.ns, G, Dm, 1.0f, st, large, dvideo, dtext, nullptr, nullptr, Dm);
}

extern "C" int clv_dsl_loss_bwd(const float* dout, const float* work, float* dvideo, float* dtext, int32_t G, int32_t Dm,
                                float temperature, float dual_softmax, void* stream) {
    return dsl_bwd_impl(dout, work, dvideo, dtext, G, Dm, temperature, dual_softmax, stream, false);
}
extern "C" int clv_dsl_loss_bwd_large(const float* dout, const float* work, float* dvideo, float* dtext, int32_t G,
                                      int32_t Dm, float temperature, float dual_softmax, void* stream) {
    return dsl_bwd_impl(dout, work, dvideo, dtext, G, Dm, temperature, dual_softmax, stream, true);
}
