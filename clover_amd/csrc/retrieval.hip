// Text -> video retrieval ranks on the device (gfx950): for every query the 0-based position of its ground-truth
// gallery row in the stable descending order of its cosine scores, and optionally the first K rows of that order —
// without ever writing the [Nq, Ng] score matrix.  Restates the host metric of the reference's evaluation stage
// (mmaction/core/evaluation/accuracy.py:430-462: normalise, dot, argsort, position of the diagonal;
// mmaction/utils/numpy_norm.py:5-8: all-zero rows stay zero), which needs one number per query and no sort:
//     rank[i] = #{j : s[i][j] > s[i][g]} + #{j < g : s[i][j] == s[i][g]},   g = gt[i].
//
// Three launches (+ one for top-K), all on fp32:
//   1. retrieval_normalize_kernel: one wave per row, query and gallery rows to unit L2 norm into the work area
//      (IEEE sqrt and division: a norm of 8 gives exactly 0.125).
//   2. retrieval_score_kernel<RT_GT>: the score of every query against ITS ground-truth row.  It is the same tile code as
//      pass 3 with the gallery operand gathered through gt (tile column c holds gallery row gt[m0 + c]; the diagonal of
//      the tile is what is kept).  v_mfma_f32_16x16x4_f32 is an fmaf chain over k per output element, so a score is a
//      function of the two rows and of the order of k alone — which both passes share — and gt_score[i] is bit-equal to
//      the s[i][g] pass 3 computes.  Pass 3 still excludes j == g by index, so even a difference could not count g itself.
//   3. retrieval_score_kernel<RT_COUNT | RT_TOPK>: a workgroup owns 64 queries and walks a contiguous chunk of the gallery
//      in 64-row tiles (both operands staged through LDS, 64 x 64 x 16 steps, 4 waves x 32 x 32, as sgemm_tiled_kernel of
//      parity.hip).  Scores stay in the MFMA accumulators; the epilogue compares them with the row's gt_score and adds up
//      int32 counts in registers, which meet across the chunks of a long gallery through atomicAdd on int32 (integer
//      adds commute: deterministic).  With top-K the tile's scores additionally pass through LDS, where one thread per
//      query inserts them in ascending column order into the query's running list (strict >: ties keep the lower index).
//   4. retrieval_topk_merge_kernel: one thread per query selects the K best of its chunk lists in the total order
//      (score descending, index ascending).
// Padded rows and columns (Nq, Ng not multiples of 64; D not a multiple of 16) are staged as zeros and masked by index
// in every epilogue: they never count and never enter a list.
//
// clv_retrieval_group_best (zero-shot multiple choice, accuracy.py:396-427; the video -> text direction of a many-caption
// test set) asks another question of the same scores: the best gallery row inside a per-query range [lo, hi), without
// the N x C N matrix whose block diagonal the reference keeps.  retrieval_score_kernel<RT_BEST> is pass 3's tile loop
// over the tiles that meet the ranges of the workgroup's 64 queries; the tile's scores pass through LDS as for top-K and
// one thread per query keeps the first maximum of its range.  retrieval_best_merge_kernel joins the chunks; the rank of
// that row in the whole gallery, when asked for, is passes 2 and 3 with gt = best_idx.  Rows are scaled by
// 1 / max(norm, eps) (sim_matrix, accuracy.py:385-394); eps = 0 is the normalisation above.
//
// Dual-softmax re-scoring (clv_retrieval_col_stats + clv_retrieval_rank_prior): s'[i][j] = s[i][j] * softmax_i(T s[i][j]),
// the softmax taken down the QUERY axis, so every query is coupled to every other one through the column statistics
//     m_j = max_i T s[i][j],   l_j = sum_i exp(T s[i][j] - m_j).
// retrieval_score_kernel<RT_STATS> is pass 3's tile loop with the operands swapped: its "queries" are the gallery rows (a
// workgroup owns 64 of them) and it walks the query set in 64-row tiles.  fmaf(a, b, c) == fmaf(b, a, c) and the order of k
// is the same, so the transposed score is bit-equal to s[i][j].  Every lane keeps a running (m, l) for its 8 rows; they
// meet over the 16 lanes of a row by xor shuffles, over the two waves of a row through LDS, and over the chunks of a long
// query set in retrieval_stats_merge_kernel, which joins the partials in chunk order: no float atomics, one fixed order.
// clv_retrieval_rank_prior is passes 1-4 with PRIOR = true: wherever a score leaves the accumulators it becomes
// rt_prior(s, m_j, l_j, T) first — in pass 2 for gt_score, in pass 3 for the counts and the lists — by one inlined
// function without contraction, so pass 3 meets pass 2's gt_score bit for bit as before.
#include "common.hpp"
#include "../../include/clover_hip.h"

namespace {

constexpr int RT_BM = 64, RT_BN = 64, RT_BK = 16;
// row stride 18: lanes (lr, lg) of a 32-lane half read word lr * 18 + lg — 16 distinct even banks + their odd
// neighbours of the 32 ds_read_b32 banks; 17 would put (15, 1) on (0, 0)'s bank
constexpr int RT_LD = RT_BK + 2;
constexpr int RT_SLD = RT_BN + 1;          // score tile: thread t walks row t
constexpr int RT_KMAX = 16, RT_LLD = RT_KMAX + 1;
constexpr int RT_MAX_CHUNKS = 64;          // bounds the top-K partial table: chunks x Nq x K x 8 bytes
constexpr int RT_WANT_GROUPS = 512;        // two workgroups per CU before the gallery stops being split

enum { RT_GT = 0, RT_COUNT = 1, RT_TOPK = 2, RT_BEST = 3, RT_STATS = 4 };
constexpr const int32_t* RT_ALL = nullptr;   // lo / hi of the modes that have no ranges
constexpr const float* RT_PLAIN = nullptr;   // col_max / col_sum of the launches without the prior

struct RtPlan {
    int nqb, tiles, tiles_per_chunk, chunks;
};

inline RtPlan rt_plan(int64_t Nq, int64_t Ng) {
    RtPlan p;
    p.nqb = (int)((Nq + RT_BM - 1) / RT_BM);
    p.tiles = (int)((Ng + RT_BN - 1) / RT_BN);
    int want = (RT_WANT_GROUPS + p.nqb - 1) / p.nqb;
    if (want > p.tiles) want = p.tiles;
    if (want > RT_MAX_CHUNKS) want = RT_MAX_CHUNKS;
    p.tiles_per_chunk = (p.tiles + want - 1) / want;
    p.chunks = (p.tiles + p.tiles_per_chunk - 1) / p.tiles_per_chunk;
    return p;
}

// one wave per row; rows [0, Nq) are the queries, [Nq, Nq + Ng) the gallery.  out is packed [Nq + Ng][D].
__global__ void __launch_bounds__(256) retrieval_normalize_kernel(const float* __restrict__ query,
                                                                  const float* __restrict__ gallery,
                                                                  float* __restrict__ out, int64_t Nq, int64_t Ng, int D,
                                                                  int64_t ldq, int64_t ldg, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= Nq + Ng) return;
    const float* e = row < Nq ? query + row * ldq : gallery + (row - Nq) * ldg;
    float s = 0.f;
    for (int d = lane; d < D; d += 64) s += e[d] * e[d];
    float nrm = fmaxf(sqrtf(wave_sum(s)), eps);             // accuracy.py:391 — max(norm, eps); eps = 0 changes nothing
    if (nrm == 0.f) nrm = 1.f;                              // numpy_norm.py:7 — l2[l2 == 0] = 1
    float* o = out + row * D;
    for (int d = lane; d < D; d += 64) o[d] = e[d] / nrm;
}

// (m, l) <- (m, l) joined with (m2, l2), both an online max / sum of exponentials: l counts exp(x - m).  An empty side is
// (-inf, 0); two empty sides stay empty (no inf - inf).
__device__ __forceinline__ void rt_stat_join(float& m, float& l, float m2, float l2) {
#pragma clang fp contract(off)
    const float mm = fmaxf(m, m2);
    if (mm == -INFINITY) return;
    l = l * expf(m - mm) + l2 * expf(m2 - mm);
    m = mm;
}

// two more exponents (-inf: a masked column) into a lane's running (m, l)
__device__ __forceinline__ void rt_stat_add2(float& m, float& l, float x0, float x1) {
#pragma clang fp contract(off)
    const float mm = fmaxf(m, fmaxf(x0, x1));
    if (mm == -INFINITY) return;
    l = l * expf(m - mm) + expf(x0 - mm) + expf(x1 - mm);
    m = mm;
}

// the re-scored value: one rounding per operation (T * s is the product col_stats took the maximum of)
__device__ __forceinline__ float rt_prior(float s, float m, float l, float T) {
#pragma clang fp contract(off)
    const float x = T * s;
    return s * expf(x - m) / l;
}

// qn [Nq][D], gn [Ng][D] packed unit rows.  Grid: (query blocks, gallery chunks); RT_GT: (query blocks, 1).
// RT_BEST reads lo / hi [Nq] (both null: the whole gallery) and writes part_score / part_idx [chunks][Nq]: the first
// maximum of query m over the columns of this chunk inside [lo[m], hi[m]), or -inf / -1 when there is none.
// PRIOR (RT_GT, RT_COUNT, RT_TOPK): col_max / col_sum [Ng] and T turn every score into rt_prior(...) before it is kept,
// compared or listed.  RT_STATS is launched with the operands swapped (qn = the gallery's rows, Nq = their number; gn =
// the queries) and writes part_score [chunks][Nq][2]: (max, sum) of T * s over the columns of this chunk.
template <int MODE, bool PRIOR = false>
__global__ void __launch_bounds__(256) retrieval_score_kernel(const float* __restrict__ qn, const float* __restrict__ gn,
                                                              const int32_t* __restrict__ gt, int32_t* __restrict__ rank,
                                                              float* __restrict__ gt_score, float* __restrict__ part_score,
                                                              int32_t* __restrict__ part_idx, int Nq, int Ng, int D,
                                                              int tiles_per_chunk, int topk,
                                                              const int32_t* __restrict__ lo,
                                                              const int32_t* __restrict__ hi,
                                                              const float* __restrict__ col_max,
                                                              const float* __restrict__ col_sum, float T) {
    __shared__ float As[RT_BM * RT_LD], Bs[RT_BN * RT_LD];
    __shared__ float Ss[(MODE == RT_TOPK || MODE == RT_BEST) ? RT_BM * RT_SLD : 1];
    __shared__ int Span[MODE == RT_BEST ? 2 : 1];
    __shared__ float Ls[MODE == RT_TOPK ? RT_BM * RT_LLD : 1];
    __shared__ int32_t Li[MODE == RT_TOPK ? RT_BM * RT_LLD : 1];
    __shared__ float Sm[MODE == RT_STATS ? 2 * RT_BM : 1], Sl[MODE == RT_STATS ? 2 * RT_BM : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lg = lane >> 4, lr = lane & 15;
    const int m0 = blockIdx.x * RT_BM;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
    const int srow = tid >> 2, sk = (tid & 3) * 4;           // staging: one float4 of each operand per thread

    // the ground truth of query m: gt[m], or m itself; -1 when the query has none (or it lies outside the gallery)
    auto truth = [&](int m) -> int {
        if (m >= Nq) return -1;
        const int g = gt ? gt[m] : m;
        return (g >= 0 && g < Ng) ? g : -1;
    };

    const float* asrc = (m0 + srow < Nq) ? qn + (int64_t)(m0 + srow) * D : nullptr;

    // per-lane view of the accumulators: acc[i][j][r] = s[m0 + wr + i*16 + lg*4 + r][n0 + wc + j*16 + lr]
    float gs[2][4];
    int g[2][4], cnt[2][4];
    if (MODE == RT_COUNT || MODE == RT_TOPK) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wr + i * 16 + lg * 4 + r;
                g[i][r] = truth(m);
                gs[i][r] = g[i][r] >= 0 ? gt_score[m] : 0.f;
                cnt[i][r] = 0;
            }
    }
    float sm[2][4], sl[2][4];                                // RT_STATS: the lane's running (m, l) of its 8 rows
    if (MODE == RT_STATS) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                sm[i][r] = -INFINITY;
                sl[i][r] = 0.f;
            }
    }
    if (MODE == RT_TOPK) {
        for (int e = tid; e < RT_BM * RT_LLD; e += 256) {
            Ls[e] = -INFINITY;
            Li[e] = -1;
        }
    }

    // RT_BEST: thread t < 64 (wave 0) owns query m0 + t; a range that is empty or leaves [0, Ng] holds no column
    int qlo = 0, qhi = 0, bidx = -1;
    float bscore = -INFINITY;
    if (MODE == RT_BEST) {
        if (tid < RT_BM) {
            if (m0 + tid < Nq) {
                qlo = lo ? lo[m0 + tid] : 0;
                qhi = hi ? hi[m0 + tid] : Ng;
                if (qlo < 0 || qhi > Ng || qlo >= qhi) qlo = qhi = 0;
            }
            int smin = qlo < qhi ? qlo : 0x7fffffff, smax = qlo < qhi ? qhi : 0;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                smin = min(smin, __shfl_xor(smin, o, 64));
                smax = max(smax, __shfl_xor(smax, o, 64));
            }
            if (tid == 0) {
                Span[0] = smin;
                Span[1] = smax;
            }
        }
        __syncthreads();
    }

    int tile0 = MODE == RT_GT ? 0 : blockIdx.y * tiles_per_chunk;
    int tile1 = MODE == RT_GT ? 1 : min(tile0 + tiles_per_chunk, (Ng + RT_BN - 1) / RT_BN);
    if (MODE == RT_BEST) {                                    // only the tiles that meet [min lo, max hi) of the 64 queries
        tile0 = max(tile0, Span[0] / RT_BN);
        tile1 = min(tile1, (Span[1] + RT_BN - 1) / RT_BN);
    }
    for (int tile = tile0; tile < tile1; ++tile) {
        const int n0 = tile * RT_BN;
        const float* bsrc;
        if (MODE == RT_GT) {
            const int gg = truth(m0 + srow);
            bsrc = gg >= 0 ? gn + (int64_t)gg * D : nullptr;
        } else {
            bsrc = (n0 + srow < Ng) ? gn + (int64_t)(n0 + srow) * D : nullptr;
        }
        f32x4_t acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

        const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
        // D % 4 == 0: a float4 at k is wholly inside the row or wholly outside
        float4 av = (asrc && sk < D) ? *reinterpret_cast<const float4*>(asrc + sk) : zero4;
        float4 bv = (bsrc && sk < D) ? *reinterpret_cast<const float4*>(bsrc + sk) : zero4;
        for (int k0 = 0; k0 < D; k0 += RT_BK) {
            __syncthreads();                                  // the previous step's fragment reads are done
            float* as = As + srow * RT_LD + sk;
            float* bs = Bs + srow * RT_LD + sk;
            as[0] = av.x; as[1] = av.y; as[2] = av.z; as[3] = av.w;
            bs[0] = bv.x; bs[1] = bv.y; bs[2] = bv.z; bs[3] = bv.w;
            __syncthreads();
            const int kn = k0 + RT_BK + sk;                   // the next step's operands travel under this step's MFMAs
            av = (asrc && kn < D) ? *reinterpret_cast<const float4*>(asrc + kn) : zero4;
            bv = (bsrc && kn < D) ? *reinterpret_cast<const float4*>(bsrc + kn) : zero4;
#pragma unroll
            for (int k4 = 0; k4 < RT_BK; k4 += 4) {
                float a[2], b[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    a[i] = As[(wr + i * 16 + lr) * RT_LD + k4 + lg];
                    b[i] = Bs[(wc + i * 16 + lr) * RT_LD + k4 + lg];
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
            }
        }

        if (MODE == RT_GT) {
            // tile column c holds gallery row gt[m0 + c]: the diagonal is s[m][gt[m]]
            if (wr == wc) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int m = m0 + wr + i * 16 + lg * 4 + r;
                        if (lg * 4 + r == lr && m < Nq) {
                            const int gg = truth(m);
                            const bool ok = gg >= 0;
                            float s = acc[i][i][r];
                            if (PRIOR && ok) s = rt_prior(s, col_max[gg], col_sum[gg], T);
                            gt_score[m] = ok ? s : __builtin_nanf("");
                            rank[m] = ok ? 0 : -1;
                        }
                    }
            }
        } else if (MODE == RT_STATS) {
            // the columns of this launch are the queries: Ng is their number, and a padded one adds nothing
            const bool in0 = n0 + wc + lr < Ng, in1 = n0 + wc + 16 + lr < Ng;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    rt_stat_add2(sm[i][r], sl[i][r], in0 ? T * acc[i][0][r] : -INFINITY,
                                 in1 ? T * acc[i][1][r] : -INFINITY);
        } else if (MODE == RT_BEST) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        Ss[(wr + i * 16 + lg * 4 + r) * RT_SLD + wc + j * 16 + lr] = acc[i][j][r];
            __syncthreads();
            if (tid < RT_BM) {
                // ascending columns, strict >: the first maximum.  qhi <= Ng keeps the padded columns out.
                const int c1 = min(RT_BN, qhi - n0);
                for (int c = max(0, qlo - n0); c < c1; ++c) {
                    const float s = Ss[tid * RT_SLD + c];
                    if (bidx < 0 || s > bscore) {
                        bscore = s;
                        bidx = n0 + c;
                    }
                }
            }
            // the next tile writes Ss only after the syncs of its k loop (D >= 4: at least one step)
        } else {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int jg = n0 + wc + j * 16 + lr;
                    const float cm = (PRIOR && jg < Ng) ? col_max[jg] : 0.f;
                    const float cl = (PRIOR && jg < Ng) ? col_sum[jg] : 1.f;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float s = PRIOR ? rt_prior(acc[i][j][r], cm, cl, T) : acc[i][j][r];
                        const bool ahead = s > gs[i][r] || (s == gs[i][r] && jg < g[i][r]);
                        cnt[i][r] += (jg < Ng && jg != g[i][r] && ahead) ? 1 : 0;
                        if (MODE == RT_TOPK) Ss[(wr + i * 16 + lg * 4 + r) * RT_SLD + wc + j * 16 + lr] = s;
                    }
                }
            if (MODE == RT_TOPK) {
                __syncthreads();
                if (tid < RT_BM && m0 + tid < Nq) {
                    float* ls = Ls + tid * RT_LLD;
                    int32_t* li = Li + tid * RT_LLD;
                    float thr = ls[topk - 1];
                    const int nc = min(RT_BN, Ng - n0);
                    for (int c = 0; c < nc; ++c) {
                        const float s = Ss[tid * RT_SLD + c];
                        if (s > thr) {                        // a tie with the list's last entry loses: its index is higher
                            int p = topk - 1;
                            while (p > 0 && ls[p - 1] < s) {
                                ls[p] = ls[p - 1];
                                li[p] = li[p - 1];
                                --p;
                            }
                            ls[p] = s;
                            li[p] = n0 + c;
                            thr = ls[topk - 1];
                        }
                    }
                }
                // the next tile writes Ss only after the syncs of its k loop (D >= 4: at least one step)
            }
        }
    }

    if (MODE == RT_STATS) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int o = 1; o < 16; o <<= 1)              // the 16 lanes that share the row: both partners get the same sum
                    rt_stat_join(sm[i][r], sl[i][r], __shfl_xor(sm[i][r], o, 64), __shfl_xor(sl[i][r], o, 64));
                if (lr == 0) {
                    Sm[(wave & 1) * RT_BM + wr + i * 16 + lg * 4 + r] = sm[i][r];
                    Sl[(wave & 1) * RT_BM + wr + i * 16 + lg * 4 + r] = sl[i][r];
                }
            }
        __syncthreads();
        if (tid < RT_BM && m0 + tid < Nq) {                   // columns 0..31 of every tile, then columns 32..63
            float m = Sm[tid], l = Sl[tid];
            rt_stat_join(m, l, Sm[RT_BM + tid], Sl[RT_BM + tid]);
            const int64_t at = ((int64_t)blockIdx.y * Nq + m0 + tid) * 2;
            part_score[at] = m;
            part_score[at + 1] = l;
        }
    }
    if (MODE == RT_BEST) {
        if (tid < RT_BM && m0 + tid < Nq) {
            part_score[(int64_t)blockIdx.y * Nq + m0 + tid] = bscore;
            part_idx[(int64_t)blockIdx.y * Nq + m0 + tid] = bidx;
        }
    }
    if (MODE == RT_COUNT || MODE == RT_TOPK) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                int c = cnt[i][r];
                c += __shfl_xor(c, 1, 64);
                c += __shfl_xor(c, 2, 64);
                c += __shfl_xor(c, 4, 64);
                c += __shfl_xor(c, 8, 64);
                const int m = m0 + wr + i * 16 + lg * 4 + r;
                if (lr == 0 && g[i][r] >= 0 && c != 0) atomicAdd(rank + m, c);
            }
    }
    if (MODE == RT_TOPK) {
        __syncthreads();
        if (tid < RT_BM && m0 + tid < Nq) {
            const int64_t base = ((int64_t)blockIdx.y * Nq + (m0 + tid)) * topk;
            for (int p = 0; p < topk; ++p) {
                part_score[base + p] = Ls[tid * RT_LLD + p];
                part_idx[base + p] = Li[tid * RT_LLD + p];
            }
        }
    }
}

// one thread per query: the K best of chunks x K candidates in the order (score descending, index ascending).  Indices are
// distinct, so the order is total and "the best candidate after the previous pick" needs no bookkeeping.
__global__ void __launch_bounds__(256) retrieval_topk_merge_kernel(const float* __restrict__ part_score,
                                                                   const int32_t* __restrict__ part_idx,
                                                                   int32_t* __restrict__ topk_idx,
                                                                   float* __restrict__ topk_score, int Nq, int chunks,
                                                                   int topk) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Nq) return;
    float ps = INFINITY;
    int pi = -1;
    for (int p = 0; p < topk; ++p) {
        float bs = -INFINITY;
        int bi = -1;
        for (int c = 0; c < chunks; ++c) {
            const int64_t base = ((int64_t)c * Nq + i) * topk;
            for (int e = 0; e < topk; ++e) {
                const int ci = part_idx[base + e];
                if (ci < 0) break;                            // a list is filled from the front
                const float cs = part_score[base + e];
                const bool after_prev = cs < ps || (cs == ps && ci > pi);
                const bool better = bi < 0 || cs > bs || (cs == bs && ci < bi);
                if (after_prev && better) {
                    bs = cs;
                    bi = ci;
                }
            }
        }
        topk_idx[(int64_t)i * topk + p] = bi;
        topk_score[(int64_t)i * topk + p] = bi >= 0 ? bs : -INFINITY;
        if (bi < 0) {                                         // fewer than K gallery rows: the rest is padding
            for (int q = p + 1; q < topk; ++q) {
                topk_idx[(int64_t)i * topk + q] = -1;
                topk_score[(int64_t)i * topk + q] = -INFINITY;
            }
            return;
        }
        ps = bs;
        pi = bi;
    }
}

// one thread per query: the best of its chunk partials in the order (score descending, index ascending); -1 / NaN when
// no chunk held a column of the query's range.
__global__ void __launch_bounds__(256) retrieval_best_merge_kernel(const float* __restrict__ part_score,
                                                                   const int32_t* __restrict__ part_idx,
                                                                   int32_t* __restrict__ best_idx,
                                                                   float* __restrict__ best_score, int Nq, int chunks) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Nq) return;
    float bs = 0.f;
    int bi = -1;
    for (int c = 0; c < chunks; ++c) {
        const int ci = part_idx[(int64_t)c * Nq + i];
        if (ci < 0) continue;
        const float cs = part_score[(int64_t)c * Nq + i];
        if (bi < 0 || cs > bs || (cs == bs && ci < bi)) {
            bs = cs;
            bi = ci;
        }
    }
    best_idx[i] = bi;
    best_score[i] = bi >= 0 ? bs : __builtin_nanf("");
}

// one thread per gallery row: the chunk partials (max, sum) joined in chunk order.  Every chunk holds at least one query,
// so every partial is finite and col_sum >= 1.
__global__ void __launch_bounds__(256) retrieval_stats_merge_kernel(const float* __restrict__ part, float* __restrict__ col_max,
                                                                    float* __restrict__ col_sum, int Ng, int chunks) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= Ng) return;
    float m = -INFINITY, l = 0.f;
    for (int c = 0; c < chunks; ++c) {
        const int64_t at = ((int64_t)c * Ng + j) * 2;
        rt_stat_join(m, l, part[at], part[at + 1]);
    }
    col_max[j] = m;
    col_sum[j] = l;
}

inline bool rt_supported(int64_t Nq, int64_t Ng, int32_t D, int32_t topk) {
    return Nq >= 1 && Ng >= 1 && Nq <= 0x7fffffff - RT_BM && Ng <= 0x7fffffff - RT_BN && D >= 4 && D <= 4096 &&
           D % 4 == 0 && topk >= 0 && topk <= RT_KMAX;
}

// T finite and >= 0 (a NaN fails both)
inline bool rt_temperature_ok(float T) { return T >= 0.f && T <= 3.402823466e38f; }

// clv_retrieval_rank (PRIOR = false: col_max, col_sum and T are not read) and clv_retrieval_rank_prior: the same launches
template <bool PRIOR>
int rt_rank(const float* query, const float* gallery, const int32_t* gt, int32_t* rank, float* gt_score, int32_t* topk_idx,
            float* topk_score, void* work, int64_t Nq, int64_t Ng, int32_t D, int64_t ldq, int64_t ldg, int32_t topk,
            const float* col_max, const float* col_sum, float T, void* stream) {
    if (!rt_supported(Nq, Ng, D, topk)) return CLV_ERR_UNSUPPORTED;
    if (!query || !gallery || !rank || !gt_score || !work || ldq < D || ldg < D) return CLV_ERR_ARG;
    if (topk > 0 && (!topk_idx || !topk_score)) return CLV_ERR_ARG;
    if (!gt && Nq > Ng) return CLV_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(work) % 16 != 0) return CLV_ERR_ARG;
    if (PRIOR && (!col_max || !col_sum || !rt_temperature_ok(T))) return CLV_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const RtPlan p = rt_plan(Nq, Ng);
    float* qn = (float*)work;
    float* gn = qn + Nq * (int64_t)D;
    float* part_score = gn + Ng * (int64_t)D;
    int32_t* part_idx = (int32_t*)(part_score + (int64_t)p.chunks * Nq * topk);
    const int64_t rows = Nq + Ng;
    hipLaunchKernelGGL(retrieval_normalize_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, query, gallery, qn,
                       Nq, Ng, (int)D, ldq, ldg, 0.f);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(retrieval_score_kernel<RT_GT, PRIOR>), dim3(p.nqb, 1), dim3(256), 0, st, qn, gn, gt,
                       rank, gt_score, (float*)nullptr, (int32_t*)nullptr, (int)Nq, (int)Ng, (int)D, 1, 0, RT_ALL, RT_ALL,
                       col_max, col_sum, T);
    if (topk > 0) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(retrieval_score_kernel<RT_TOPK, PRIOR>), dim3(p.nqb, p.chunks), dim3(256), 0, st,
                           qn, gn, gt, rank, gt_score, part_score, part_idx, (int)Nq, (int)Ng, (int)D, p.tiles_per_chunk,
                           (int)topk, RT_ALL, RT_ALL, col_max, col_sum, T);
        hipLaunchKernelGGL(retrieval_topk_merge_kernel, dim3((unsigned)((Nq + 255) / 256)), dim3(256), 0, st, part_score,
                           part_idx, topk_idx, topk_score, (int)Nq, p.chunks, (int)topk);
    } else {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(retrieval_score_kernel<RT_COUNT, PRIOR>), dim3(p.nqb, p.chunks), dim3(256), 0, st,
                           qn, gn, gt, rank, gt_score, (float*)nullptr, (int32_t*)nullptr, (int)Nq, (int)Ng, (int)D,
                           p.tiles_per_chunk, 0, RT_ALL, RT_ALL, col_max, col_sum, T);
    }
    return clv_check_launch();
}

}  // namespace

extern "C" int64_t clv_retrieval_work_bytes(int64_t Nq, int64_t Ng, int32_t D, int32_t topk) {
    if (!rt_supported(Nq, Ng, D, topk)) return CLV_ERR_UNSUPPORTED;
    const RtPlan p = rt_plan(Nq, Ng);
    return (Nq + Ng) * (int64_t)D * 4 + (int64_t)p.chunks * Nq * topk * 8;
}

extern "C" int clv_retrieval_rank(const float* query, const float* gallery, const int32_t* gt, int32_t* rank,
                                  float* gt_score, int32_t* topk_idx, float* topk_score, void* work, int64_t Nq,
                                  int64_t Ng, int32_t D, int64_t ldq, int64_t ldg, int32_t topk, void* stream) {
    return rt_rank<false>(query, gallery, gt, rank, gt_score, topk_idx, topk_score, work, Nq, Ng, D, ldq, ldg, topk, RT_PLAIN,
                          RT_PLAIN, 0.f, stream);
}

extern "C" int64_t clv_retrieval_col_stats_work_bytes(int64_t Nq, int64_t Ng, int32_t D) {
    if (!rt_supported(Nq, Ng, D, 0)) return CLV_ERR_UNSUPPORTED;
    const RtPlan p = rt_plan(Ng, Nq);                         // the gallery rows own the workgroups, the queries are walked
    return (Nq + Ng) * (int64_t)D * 4 + (int64_t)p.chunks * Ng * 8;
}

extern "C" int clv_retrieval_col_stats(const float* query, const float* gallery, int64_t Nq, int64_t Ng, int32_t D,
                                       int64_t ldq, int64_t ldg, float T, float* col_max, float* col_sum, void* work,
                                       void* stream) {
    if (!rt_supported(Nq, Ng, D, 0)) return CLV_ERR_UNSUPPORTED;
    if (!query || !gallery || !col_max || !col_sum || !work || ldq < D || ldg < D) return CLV_ERR_ARG;
    if (!rt_temperature_ok(T) || reinterpret_cast<uintptr_t>(work) % 16 != 0) return CLV_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const RtPlan p = rt_plan(Ng, Nq);
    float* qn = (float*)work;
    float* gn = qn + Nq * (int64_t)D;
    float* part = gn + Ng * (int64_t)D;
    const int64_t rows = Nq + Ng;
    hipLaunchKernelGGL(retrieval_normalize_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, query, gallery, qn,
                       Nq, Ng, (int)D, ldq, ldg, 0.f);
    hipLaunchKernelGGL(retrieval_score_kernel<RT_STATS>, dim3(p.nqb, p.chunks), dim3(256), 0, st, (const float*)gn,
                       (const float*)qn, (const int32_t*)nullptr, (int32_t*)nullptr, (float*)nullptr, part,
                       (int32_t*)nullptr, (int)Ng, (int)Nq, (int)D, p.tiles_per_chunk, 0, RT_ALL, RT_ALL, RT_PLAIN, RT_PLAIN, T);
    hipLaunchKernelGGL(retrieval_stats_merge_kernel, dim3((unsigned)((Ng + 255) / 256)), dim3(256), 0, st, (const float*)part,
                       col_max, col_sum, (int)Ng, p.chunks);
    return clv_check_launch();
}

extern "C" int64_t clv_retrieval_rank_prior_work_bytes(int64_t Nq, int64_t Ng, int32_t D, int32_t topk) {
    return clv_retrieval_work_bytes(Nq, Ng, D, topk);
}

extern "C" int clv_retrieval_rank_prior(const float* query, const float* gallery, const int32_t* gt, int32_t* rank,
                                        float* gt_score, int32_t* topk_idx, float* topk_score, void* work, int64_t Nq,
                                        int64_t Ng, int32_t D, int64_t ldq, int64_t ldg, int32_t topk, const float* col_max,
                                        const float* col_sum, float T, void* stream) {
    return rt_rank<true>(query, gallery, gt, rank, gt_score, topk_idx, topk_score, work, Nq, Ng, D, ldq, ldg, topk, col_max,
                         col_sum, T, stream);
}

extern "C" int64_t clv_retrieval_group_work_bytes(int64_t Nq, int64_t Ng, int32_t D) {
    if (!rt_supported(Nq, Ng, D, 0)) return CLV_ERR_UNSUPPORTED;
    const RtPlan p = rt_plan(Nq, Ng);
    return (Nq + Ng) * (int64_t)D * 4 + (int64_t)p.chunks * Nq * 8;
}

extern "C" int clv_retrieval_group_best(const float* query, const float* gallery, const int32_t* lo, const int32_t* hi,
                                        int32_t* best_idx, float* best_score, int32_t* rank, void* work, int64_t Nq,
                                        int64_t Ng, int32_t D, int64_t ldq, int64_t ldg, float eps, void* stream) {
    if (!rt_supported(Nq, Ng, D, 0)) return CLV_ERR_UNSUPPORTED;
    if (!query || !gallery || !best_idx || !best_score || !work || ldq < D || ldg < D) return CLV_ERR_ARG;
    if ((lo == nullptr) != (hi == nullptr) || !(eps >= 0.f)) return CLV_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(work) % 16 != 0) return CLV_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const RtPlan p = rt_plan(Nq, Ng);
    float* qn = (float*)work;
    float* gn = qn + Nq * (int64_t)D;
    float* part_score = gn + Ng * (int64_t)D;
    int32_t* part_idx = (int32_t*)(part_score + (int64_t)p.chunks * Nq);
    const int64_t rows = Nq + Ng;
    hipLaunchKernelGGL(retrieval_normalize_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, query, gallery, qn,
                       Nq, Ng, (int)D, ldq, ldg, eps);
    hipLaunchKernelGGL(retrieval_score_kernel<RT_BEST>, dim3(p.nqb, p.chunks), dim3(256), 0, st, qn, gn,
                       (const int32_t*)nullptr, (int32_t*)nullptr, (float*)nullptr, part_score, part_idx, (int)Nq, (int)Ng,
                       (int)D, p.tiles_per_chunk, 0, lo, hi, RT_PLAIN, RT_PLAIN, 0.f);
    hipLaunchKernelGGL(retrieval_best_merge_kernel, dim3((unsigned)((Nq + 255) / 256)), dim3(256), 0, st, part_score,
                       part_idx, best_idx, best_score, (int)Nq, p.chunks);
    if (rank) {
        // clv_retrieval_rank's passes 2 and 3 with gt = best_idx.  Pass 2 rewrites best_score with s[i][best_idx[i]]: the
        // same two rows in the same k order, so the same bits (and NaN where best_idx = -1).
        hipLaunchKernelGGL(retrieval_score_kernel<RT_GT>, dim3(p.nqb, 1), dim3(256), 0, st, qn, gn, (const int32_t*)best_idx,
                           rank, best_score, (float*)nullptr, (int32_t*)nullptr, (int)Nq, (int)Ng, (int)D, 1, 0, RT_ALL,
                           RT_ALL, RT_PLAIN, RT_PLAIN, 0.f);
        hipLaunchKernelGGL(retrieval_score_kernel<RT_COUNT>, dim3(p.nqb, p.chunks), dim3(256), 0, st, qn, gn,
                           (const int32_t*)best_idx, rank, best_score, (float*)nullptr, (int32_t*)nullptr, (int)Nq, (int)Ng,
                           (int)D, p.tiles_per_chunk, 0, RT_ALL, RT_ALL, RT_PLAIN, RT_PLAIN, 0.f);
    }
    return clv_check_launch();
}
