"""Reference, floor and case table of the dual-softmax loss (csrc/losses.hip clv_dsl_loss_*).  Built on tests/loss_ref.py
(imported, not edited): its ``Arith``, ``_normalise`` / ``_normalise_bwd``, ``_matmul_nt`` and the parts of its ordered
log-sum-exp helpers (``_push``, ``_tree64``, ``_fma``).  tests/DSL_LOSS_ERROR_BUDGET.md explains the bounds.

``dsl_ref`` evaluates, with c the cosine matrix, x = T c and a = G / temperature,

    Pr = softmax over i of x      Pc = softmax over j of x      yr = (a c) Pr      yc = (a c) Pc
    loss = -mean_i log_softmax_j(yr)[i][i] - mean_j log_softmax_i(yc)[j][j]

and the analytic gradient (gr = exp(yr - lse_j yr) - I, gc = exp(yc - lse_i yc) - I; the 1 / G folded into the scale)

    u[j] = sum_i (gr c) Pr        w[i] = sum_j (gc c) Pc
    d loss / d c = g / temperature * (Pr (gr (1 + x) - T u[j]) + Pc (gc (1 + x) - T w[i])).

With ``FP64`` and no ``order`` it is the reference.  With ``DSL32`` and the ``order`` record of the path's plan it is the floor:
the same operations, one fp32 rounding each, in the order the kernels add — the kernels' arithmetic is compiled with
contraction off so that this holds operation for operation; ``lse_push`` keeps its fused multiply-add, as loss_ref models it.
"""
import ctypes as C
import functools

import torch

import loss_ref as lr
from loss_ref import FP64



class _DslArith(lr.Arith):
    """loss_ref's fp32 arithmetic with the logarithm of the DSL kernels: dsl_log, the fp64 logarithm rounded once."""

    def log(self, x):
        return torch.log(x.double()).to(self.dtype)


DSL32 = _DslArith(torch.float32, True)
DSL_TS = (0.0, 20.0, 100.0)
DSL_DLOSS = 1.7

# (G, Dm, path, what it reaches).  paths: 'small' / 'large' pinned, 'auto' by the row count.
DSL_CASES = [
    (1, 16, 'auto', 'one tile; loss and gradients 0'),
    (3, 40, 'auto', 'K % 16 != 0'),
    (33, 257, 'auto', '8-wave forward'),
    (64, 768, 'auto', 'the fine-tuning width'),
    (127, 64, 'auto', 'last small G'),
    (128, 64, 'auto', 'first large G'),
    (65, 64, 'large', 'ragged column group, G just over a wave'),
    (131, 80, 'large', '3 columns in the last group'),
    (256, 64, 'small', 'busiest one-workgroup walk'),
]


def dsl_claims():
    """{(G, Dm, large): predicate on the record of clv_dsl_loss_plan} — what each case was written to reach."""
    G1, G8, GV, GG = lr.G_ONE, lr.G_EIGHT, lr.G_VEC, lr.G_GUARD
    return {
        (1, 16, 0): lambda p: p.fwd.kernel == G1 and p.fwd.tiles == 1 and p.loss_threads == 1024 and p.loss_trips == 1,
        (3, 40, 0): lambda p: p.fwd.kernel == G1 and p.fwd.k_tail == 8,
        (33, 257, 0): lambda p: p.fwd.kernel == G8 and p.fwd.waves_with_work == 6,
        (64, 768, 0): lambda p: p.fwd.kernel == G8 and p.fwd.waves_with_work == 8 and p.fwd.k_tail == 0,
        (127, 64, 0): lambda p: p.large == 0 and p.loss_trips == 1 and p.fwd.kernel == G1,
        (128, 64, 1): lambda p: (p.large == 1 and p.cols_gx == 2 and p.cols_last == 64 and p.rows_grid == 32
                                 and p.fwd.kernel == GV and p.bwd0.kernel == GV and p.bwd1.kernel == GV),
        (65, 64, 1): lambda p: p.cols_gx == 2 and p.cols_last == 1 and p.fwd.kernel == GV and p.bwd0.kernel == GG,
        (131, 80, 1): lambda p: p.cols_gx == 3 and p.cols_last == 3 and p.fwd.kernel == GV and p.bwd0.kernel == GG,
        (256, 64, 0): lambda p: (p.large == 0 and p.loss_threads == 1024 and p.loss_trips == 1 and p.bwd0.kernel == G8
                                 and p.bwd1.kernel == G8 and p.fwd.kernel == G1),
    }


def dsl_plan(lib, G, Dm, large):
    from clover_amd import _lib
    p = _lib.ClvLossPlan()
    assert lib.clv_dsl_loss_plan(G, Dm, int(large), C.byref(p)) == 0
    return p


# ------------------------------------------------------------------------------------------ plain sums in the kernels' order
def _sum_seq(x):
    """Rows of x [R, n] added element after element by one thread (dsl_uw_kernel)."""
    s = x.new_zeros(x.shape[0])
    for c in range(x.shape[1]):
        s = s + x[:, c]
    return s


def _sum_rows_multi(x):
    """dsl_w_rows_kernel: lane l adds elements l, l + 64, ... of its row in turn, then wave_sum."""
    R, n = x.shape
    pad = (-n) % 64
    x = torch.cat([x, x.new_zeros(R, pad)], 1).view(R, -1, 64)
    acc = x.new_zeros(R, 64)
    for c in range(x.shape[1]):
        acc = acc + x[:, c]
    return lr._tree64(acc)


def _sum_cols_multi(x, waves=16):
    """dsl_u_cols_kernel: wave w adds rows w, w + 16, ... of a column; the 16 partial sums are added in wave order."""
    G, n = x.shape
    pad = (-G) % waves
    x = torch.cat([x, x.new_zeros(pad, n)], 0).view(-1, waves, n)
    acc = x.new_zeros(waves, n)
    for r in range(x.shape[0]):
        acc = acc + x[r]
    s = x.new_zeros(n)
    for w in range(waves):
        s = s + acc[w]
    return s


def _sum_rows(x, order):
    if order is None:
        return x.sum(1)
    return _sum_rows_multi(x) if order['large'] else _sum_seq(x)


def _sum_cols(x, order):
    if order is None:
        return x.sum(0)
    return _sum_cols_multi(x) if order['large'] else _sum_seq(x.t().contiguous())


# --------------------------------------------------------------------- log-sum-exps in two parts, in the kernels' order
# The kernels keep a log-sum-exp as (m, l): the maximum and l = log sum exp(. - m), and form exp((v - m) - l).  loss_ref's
# ordered helpers return m + l rounded to one number; these are the same walks (its _push, _tree64 and _fma) with the two
# parts returned apart.
def _stat_seq(x, ar):
    """loss_ref._lse_seq: rows of x [R, n], the maximum, then `s += exp(x - m)` element after element."""
    m = x.max(1).values
    s = torch.zeros_like(m)
    for c in range(x.shape[1]):
        s = s + ar.exp(x[:, c] - m)
    return m, ar.log(s)


def _stat_rows_multi(x, ar):
    """loss_ref._lse_rows_multi on one block."""
    R, G = x.shape
    m = torch.full((R, 64), lr.NEG_INF, dtype=ar.dtype)
    s = torch.zeros(R, 64, dtype=ar.dtype)
    lanes = torch.arange(64)
    for c in range(0, G, 64):
        v = torch.full((R, 64), lr.NEG_INF, dtype=ar.dtype)
        n = min(64, G - c)
        v[:, :n] = x[:, c:c + n]
        m, s = lr._push(m, s, v, (lanes < n)[None, :].expand(R, 64), ar)
    wm = m.max(1).values
    t = torch.where(m == lr.NEG_INF, torch.zeros_like(s), s * ar.exp(m - wm[:, None]))
    return wm, ar.log(lr._tree64(t))


def _stat_cols_multi(x, ar, waves=16):
    """loss_ref._lse_cols_multi."""
    G = x.shape[0]
    m = torch.full((waves, G), lr.NEG_INF, dtype=ar.dtype)
    s = torch.zeros(waves, G, dtype=ar.dtype)
    ws = torch.arange(waves)
    for r in range(0, G, waves):
        v = torch.full((waves, G), lr.NEG_INF, dtype=ar.dtype)
        n = min(waves, G - r)
        v[:n] = x[r:r + n]
        m, s = lr._push(m, s, v, (ws < n)[:, None].expand(waves, G), ar)
    bm = m.max(0).values
    bs = torch.zeros(G, dtype=ar.dtype)
    for w in range(waves):
        live = m[w] != lr.NEG_INF
        bs = torch.where(live, lr._fma(s[w], ar.exp(m[w] - bm), bs), bs)
    return bm, ar.log(bs)


def _stat_rows(x, ar, order):
    if order is None:
        m = x.max(1).values
        return m, ar.log(ar.exp(x - m[:, None]).sum(1))
    return _stat_rows_multi(x, ar) if order['large'] else _stat_seq(x, ar)


def _stat_cols(x, ar, order):
    if order is None:
        m, l = _stat_rows(x.t(), ar, None)
        return m, l
    return _stat_cols_multi(x, ar) if order['large'] else _stat_seq(x.t().contiguous(), ar)


# ------------------------------------------------------------------------------------------------------- the loss
def dsl_cos_ref(c, temperature, T, g, ar=FP64, order=None):
    """The loss on a given cosine matrix c [G, G].  -> dict(loss, dc, yr, yc)."""
    c = c.to(ar.dtype)
    G = c.shape[0]
    tt = lambda v: torch.tensor(v, dtype=ar.dtype)                            # noqa: E731
    a = tt(float(G)) / tt(temperature)
    Tt = tt(T)
    idx = torch.arange(G)
    eye = torch.eye(G, dtype=ar.dtype)
    x = c * Tt
    (prm, prl), (pcm, pcl) = _stat_cols(x, ar, order), _stat_rows(x, ar, order)
    pr, pc = ar.exp((x - prm[None, :]) - prl[None, :]), ar.exp((x - pcm[:, None]) - pcl[:, None])
    ac = c * a
    yr, yc = ac * pr, ac * pc
    (yrm, yrl), (ycm, ycl) = _stat_rows(yr, ar, order), _stat_cols(yc, ar, order)
    loss = -((((yr[idx, idx] - yrm) - yrl).sum() + ((yc[idx, idx] - ycm) - ycl).sum()) / G)
    gr = ar.exp((yr - yrm[:, None]) - yrl[:, None]) - eye
    gc = ar.exp((yc - ycm[None, :]) - ycl[None, :]) - eye
    u, w = _sum_cols((gr * c) * pr, order), _sum_rows((gc * c) * pc, order)
    k = 1 + x
    scale = tt(g) * (tt(1.0) / tt(temperature))
    dc = (pr * (gr * k - Tt * u[None, :]) + pc * (gc * k - Tt * w[:, None])) * scale
    return dict(loss=loss, dc=dc, yr=yr, yc=yc, parts=dict(c=c, pcm=pcm, pcl=pcl, prm=prm, prl=prl, yrm=yrm, yrl=yrl, ycm=ycm,
                                                           ycl=ycl, w=w, u=u))


def _normalise(e, eps, ar, order):
    """loss_ref._normalise with a correctly rounded square root in the floor.  ns_normalize_kernel's sqrtf IS correctly
    rounded (the compiler's fix-up sequence after the hardware estimate); torch's vectorised fp32 sqrt on the host is not
    on about one row in a hundred (found on four dumped work areas: with the fp64 square root rounded once, 1 / norm agrees
    with the kernel on every row).  One ulp of a norm is one ulp of a whole row of cosines, which this loss multiplies by up
    to G / temperature; the plain loss never noticed."""
    if order is None:
        return lr._normalise(e, eps, ar, order)
    n = lr._lane_dot(e, e).double().sqrt().to(ar.dtype)[:, None]
    inv = 1.0 / n.clamp_min(eps)
    return e * inv, inv, n >= eps


def dsl_ref(video, text, temperature, eps, T, g, ar=FP64, order=None):
    """The dual-softmax loss with the norm clamp eps and upstream gradient g.  -> dict(loss, dvideo, dtext, yr, yc)."""
    v, t = video.to(ar.dtype), text.to(ar.dtype)
    vn, vinv, vlive = _normalise(v, eps, ar, order)
    tn, tinv, tlive = _normalise(t, eps, ar, order)
    r = dsl_cos_ref(lr._matmul_nt(vn, tn, ar, order, 0), temperature, T, g, ar, order)
    dv = lr._matmul_nt(r['dc'], tn.t(), ar, order, 1)
    dt = lr._matmul_nt(r['dc'].t(), vn.t(), ar, order, 2)
    return dict(loss=r['loss'], dvideo=lr._normalise_bwd(vn, dv, vinv, vlive, order),
                dtext=lr._normalise_bwd(tn, dt, tinv, tlive, order), yr=r['yr'], yc=r['yc'], dc=r['dc'], parts=r['parts'])


def dsl_autograd(video, text, temperature, eps, T, g):
    """The plain formulation under fp64 autograd (priors not detached).  -> dict(loss, dvideo, dtext)."""
    v = video.double().clone().requires_grad_()
    t = text.double().clone().requires_grad_()
    G = v.shape[0]
    vn = v / v.norm(dim=1, keepdim=True).clamp_min(eps)
    tn = t / t.norm(dim=1, keepdim=True).clamp_min(eps)
    c = vn @ tn.t()
    yr = (G / temperature) * c * torch.softmax(T * c, 0)
    yc = (G / temperature) * c * torch.softmax(T * c, 1)
    loss = -torch.log_softmax(yr, 1).diag().mean() - torch.log_softmax(yc, 0).diag().mean()
    (g * loss).backward()
    return dict(loss=loss.detach(), dvideo=v.grad, dtext=t.grad)


# ------------------------------------------------------------------------------------------------------- inputs
def dsl_inputs(G, Dm, hub=False):
    """loss_ref.ns_inputs with its clamp rows (zero and sub-eps norms) from G = 4 on.  hub: video 0 is the mean of all text
    rows — a video every text query scores high on, the case the prior over the queries is made for."""
    v, t = lr.ns_inputs(G, Dm, clamp=G >= 4)
    if hub:
        v = v.clone()
        v[0] = t.mean(0)
    return v, t


def dsl_clamp_rows(G):
    """{tensor name: rows whose gradient is compared against its own maximum} — the rows of norm 3e-10 / 3e-9 (and the zero
    row), whose reference gradients are many orders above the others'."""
    rows = {'dvideo': [], 'dtext': []}
    if G >= 4:
        for name, row in lr.NS_CLAMP_ROWS:
            rows[name].append(row)
    return rows


def _lib_handle():
    from clover_amd import _lib
    return _lib.lib()


@functools.lru_cache(maxsize=None)
def dsl_case_refs(G, Dm, temperature, eps, T, large=None, hub=False):
    """(video, text, fp64 reference, fp32 floor in the order of the path's kernels); shared by the tests, never modified."""
    v, t = dsl_inputs(G, Dm, hub)
    order = None if large is None else lr.plan_order(dsl_plan(_lib_handle(), G, Dm, large))
    return (v, t, dsl_ref(v, t, temperature, eps, T, DSL_DLOSS, FP64),
            dsl_ref(v, t, temperature, eps, T, DSL_DLOSS, DSL32, order))


def hub_pairs():
    """The hub case written out: four orthonormal texts e_j; video j = e_j + 2 e_(4+j), cosine 1 / sqrt(5) = 0.447 with its
    own text and 0 with the others; video 0 = the mean of all text rows, cosine 0.5 with EVERY text.  Plain scores rank the
    hub above the true video for texts 1..3; its prior along the text axis is 1 / 4, the true videos' is about 1."""
    t = torch.eye(4, 8, dtype=torch.float64)
    v = torch.eye(4, 8, dtype=torch.float64)
    for j in range(4):
        v[j, 4 + j] = 2.0
    v[0] = t.mean(0)
    return v, t
