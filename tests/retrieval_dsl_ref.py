"""Reference side of the dual-softmax (DSL) retrieval tests, shared by tests/test_retrieval_dsl_cpu.py and
tests/test_retrieval_dsl_gpu.py: the fp64 reference, the a-priori error bounds of tests/RETRIEVAL_DSL_ERROR_BUDGET.md, the
rank windows they give, and the numpy fp32 restatement that has to stay inside them on its own.

    s'[i][j] = s[i][j] * p[i][j],   p[i][j] = exp(T s[i][j] - m_j) / l_j,   m_j = max_i T s[i][j],  l_j = sum_i exp(T s[i][j] - m_j)
"""
import functools
import math

import numpy as np

U = 2.0 ** -24                    # unit roundoff of fp32
TINY = 4 * 2.0 ** -149            # underflow floor: exp, the product and the quotient each round to a subnormal grid
EXP_ULP = 3                       # expf: at most 3 ulp (the OpenCL / HIP device-library bound), 1 ulp = 2 U

# (Nq, Ng, D, captions per video, topk, seed) of the windowed rank tests, each run at both temperatures
TEMPERATURES = (20.0, 100.0)
WINDOW_CASES = [(333, 333, 64, 1, 10, 2395), (515, 103, 96, 5, 10, 3701), (17, 5, 8, 1, 10, 127)]
WIDE_CASE = (1000, 1000, 768, 1, 5, 75)        # the seed: see test_numpy_fp32_restatement_stays_inside_the_windows
WIDE_CAP = 0.05


def eps_s(D):
    """|device score - fp64 score| for unit rows (tests/test_retrieval_gpu.py): 2 (D + 4) 2^-24."""
    return 2 * (D + 4) * U


def rescales(Nq):
    """How often a term of l_j can be multiplied by a rescaling factor exp(m_old - m_new) on its way to col_sum: once per
    64-query tile of its chunk, four lane shuffles, one join of the two waves, once per chunk (tiles per chunk + chunks
    <= tiles + 1)."""
    return (Nq + 63) // 64 + 6


def eps_x(es, T):
    """Absolute error of the exponent fl(fl(T s) - m_j) against T s64 - m64_j, es the bound of the scores."""
    return 2 * T * es + 4 * T * U


def rho_l(Nq, es, T):
    """log of the relative error factor of col_sum[j] (RETRIEVAL_DSL_ERROR_BUDGET.md, section 2)."""
    return eps_x(es, T) + (2 * EXP_ULP + (Nq - 1) + rescales(Nq) * (2 * EXP_ULP + 1 + 2 * T)) * U


def eps_l(Nq, es, T):
    return math.expm1(rho_l(Nq, es, T))


def eps_r(Nq, es, T):
    """Relative error of the device prior times the two roundings of s * e / l (section 3)."""
    return math.expm1(eps_x(es, T) + 2 * EXP_ULP * U + rho_l(Nq, es, T) + 2 * U)


def norm64(x):
    x = np.asarray(x, dtype=np.float64)
    n = np.linalg.norm(x, axis=1, keepdims=True)
    n[n == 0] = 1
    return x / n


def ref64(q, gal, T):
    """-> s64, m64 [Ng], l64 [Ng], p64, s'64, all float64."""
    s = norm64(q) @ norm64(gal).T
    x = T * s
    m = x.max(axis=0)
    e = np.exp(x - m[None, :])
    l = e.sum(axis=0)
    p = e / l[None, :]
    return s, m, l, p, s * p


def bound(s64, p64, Nq, es, T):
    """e_ij = p_ij (eps_s + |s64_ij| eps_r) + the underflow floor."""
    return p64 * (es + np.abs(s64) * eps_r(Nq, es, T)) + TINY


def windows(sp64, e, gt):
    """lo = #{j : certainly above gt}, hi = #{j != g : possibly above or tied}, with a per-element bound e (an array like
    sp64, or one number)."""
    Nq = len(sp64)
    e = np.broadcast_to(np.asarray(e, dtype=np.float64), sp64.shape)
    rows = np.arange(Nq)
    up_g, dn_g = (sp64 + e)[rows, gt], (sp64 - e)[rows, gt]
    others = np.ones_like(sp64, dtype=bool)
    others[rows, gt] = False
    lo = ((sp64 - e > up_g[:, None]) & others).sum(1)
    hi = ((sp64 + e >= dn_g[:, None]) & others).sum(1)
    return lo, hi


def restate32(q, gal, T):
    """The numpy fp32 restatement: evaluation.normalize_fn, one fp32 matmul, evaluation.dual_softmax_scores -> s32, s'32."""
    from clover_amd.evaluation import dual_softmax_scores, normalize_fn
    s32 = np.dot(normalize_fn(np.asarray(q, np.float32)), normalize_fn(np.asarray(gal, np.float32)).T)
    sp32 = dual_softmax_scores(s32, T)
    assert s32.dtype == np.float32 and sp32.dtype == np.float32
    return s32, sp32


def stable_ranks(sp, gt):
    order = np.argsort(-sp, axis=1, kind='stable')
    return np.where(order == np.asarray(gt)[:, None])[1]


def make(Nq, Ng, D, caps, seed):
    """The inputs of tests/test_retrieval_gpu.py::_make."""
    from test_retrieval_gpu import _make
    return _make(Nq, Ng, D, caps, seed)


@functools.lru_cache(maxsize=None)
def window_case(case, T):
    """One windowed case, computed once per process: inputs, fp64 reference, bound and windows."""
    Nq, Ng, D, caps, topk, seed = case
    q, gal, gt = make(Nq, Ng, D, caps, seed)
    s64, m64, l64, p64, sp64 = ref64(q, gal, T)
    es = eps_s(D)
    if case == WIDE_CASE:
        # D = 768, where the a-priori eps_s makes too many windows wide: as test_real_width_random, eps_s is measured on the
        # reference arithmetic, 8 x max|numpy fp32 score - fp64 score|, and goes into the same formulas for eps_r and e_ij
        s32, _ = restate32(q, gal, T)
        es = 8 * float(np.abs(s32.astype(np.float64) - s64).max())
    e = bound(s64, p64, Nq, es, T)
    lo, hi = windows(sp64, e, gt)
    for a in (q, gal, gt, s64, p64, sp64, lo, hi):
        a.setflags(write=False)
    return dict(q=q, gal=gal, gt=gt, s64=s64, m64=m64, l64=l64, p64=p64, sp64=sp64, e=e, lo=lo, hi=hi,
                wide=float(np.mean(hi > lo)), topk=topk, D=D, T=T, eps_s=es)
