"""References, floors, input builders and case tables for the loss kernels of csrc/losses.hip (focal masked-LM cross entropy,
exclusive InfoNCE + ranking, NormSoftmaxLoss).  tests/LOSS_ERROR_BUDGET.md explains the bounds.

* ``*_ref`` with ``FP64``: the formulas written out plainly in fp64, forward and analytic backward.  They do not call
  ``oracle.model``; tests/test_loss_ref_cpu.py compares the two.
* the same functions with ``FP32``: the floor — the same formulas in fp32 with what the kernels do and nothing else:
  exp(x) as exp2(fl(x * log2 e)) and log(x) as fl(log2(x) * ln 2) (what __expf / __logf compile to), the temperature as a
  multiplication by fl(1 / T), 16-bit logits and 16-bit rounding of dlogits on the 16-bit focal paths, and — for InfoNCE
  and NormSoftmax, given an ``order`` record — the order in which the kernels of a path add (see _gemm_nt, _lse_seq,
  _lse_rows_multi, _lse_cols_multi, _lane_dot).
* builders whose conditions (both kinds of hinge row, a hinge no closer than 0.02 to its threshold, finite gradients)
  tests/test_loss_ref_cpu.py asserts on the fp64 reference, and the case tables with the launch class each case was
  written to reach, which the same test asserts through clv_focal_plan / clv_infonce_plan / clv_normsoftmax_plan.
"""
import ctypes as C
import functools
import math

import torch

LOG2E, LN2 = 1.4426950408889634, 0.6931471805599453


class Arith:
    """A number format and its exp / log."""

    def __init__(self, dtype, fast):
        self.dtype, self.fast = dtype, fast

    def exp(self, x):
        if not self.fast:
            return torch.exp(x)
        return torch.exp2(x * torch.tensor(LOG2E, dtype=self.dtype))

    def log(self, x):
        if not self.fast:
            return torch.log(x)
        return torch.log2(x) * torch.tensor(LN2, dtype=self.dtype)

    def lse(self, x, dim):
        m = x.max(dim, keepdim=True).values
        return (m + self.log(self.exp(x - m).sum(dim, keepdim=True))).squeeze(dim)


FP64, FP32 = Arith(torch.float64, False), Arith(torch.float32, True)


# ------------------------------------------------------------------------------------------------------------ statistics
def rms_rel(got, ref):
    """RMS error over the RMS of the reference (inf when the reference is all zero and `got` is not)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    den = ref.pow(2).mean().sqrt().item()
    num = (got - ref).pow(2).mean().sqrt().item()
    if den == 0.0:
        return 0.0 if num == 0.0 else math.inf
    return num / den


def row_stat(got, ref):
    """The largest per-row max error over that row's max; a row whose max is below 1e-3 of the tensor's is normalised by
    that fraction of the tensor's max (the rule of NORM_ACT_ERROR_BUDGET.md)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    got, ref = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    top = ref.abs().max().item()
    err = (got - ref).abs().max(1).values
    if top == 0.0:
        return 0.0 if err.max().item() == 0.0 else math.inf
    return (err / ref.abs().max(1).values.clamp_min(1e-3 * top)).max().item()


def scalar_rel(got, ref):
    return abs(float(got) - float(ref)) / max(1.0, abs(float(ref)))


def vec_rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return ((got - ref).abs() / ref.abs().clamp_min(1.0)).max().item() if ref.numel() else 0.0


ULP32 = 2.0 ** -23


# ----------------------------------------------------------------------------------------------------------------- focal
def focal_ref(logits, labels, gamma, dloss, ld=None, ar=FP64, round_to=None):
    """logits [R, V] (the values the kernel reads), labels int64 [R] (< 0: ignored).  -> dict(lse [R], ce [R] (0 on ignored
    rows, as the kernel stores them), loss, count, dlogits [R, ld] with zeros on ignored rows and padding columns).
    round_to: the 16-bit type dlogits is stored in."""
    x = logits.to(ar.dtype)
    R, V = x.shape
    ld = V if ld is None else ld
    act = labels >= 0
    lab = labels.clamp_min(0)
    lse = ar.lse(x, 1)
    ce = lse - x.gather(1, lab[:, None])[:, 0]
    pt = ar.exp(-ce)
    om = 1 - pt
    if gamma == 0:
        f, dl = ce, torch.ones_like(ce)
    else:
        f = om ** gamma * ce
        dl = gamma * om ** (gamma - 1) * pt * ce + om ** gamma
    n = int(act.sum())
    zero = torch.zeros_like(ce)
    loss = torch.where(act, f, zero).sum() / n if n else torch.tensor(float('nan'), dtype=ar.dtype)
    coef = torch.where(act, dloss * dl / max(n, 1), zero)
    onehot = torch.zeros_like(x).scatter_(1, lab[:, None], 1.0)
    d = torch.zeros(R, ld, dtype=ar.dtype)
    d[:, :V] = torch.where(act[:, None], coef[:, None] * (ar.exp(x - lse[:, None]) - onehot), torch.zeros_like(x))
    if round_to is not None:
        d = d.to(round_to).to(ar.dtype)
    return dict(lse=torch.where(act, lse, zero), ce=torch.where(act, ce, zero), loss=loss, count=n, dlogits=d)


GAMMAS = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0)
FOCAL_DLOSS = 1.7
# kernel classes of clv_focal_plan
F_FP32, F_HALF, F_PAIRS = 0, 1, 2


def focal_inputs(rows, V, gamma, seed):
    """fp32 logits [rows, V] and labels.  rows == 9: ignored rows first, in between and last; an ascending-sorted row with
    the label at column 0, a descending one with the label at 1, a constant row with the label at V - 2, a row with one
    dominant logit (+40) under its label V - 1 (pt -> 1; for gamma < 1, where the reference has no finite gradient at
    pt == 1, a random row instead), two random rows.  rows == 1: one random row with the label at V - 1."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, V, generator=g) * 2.0
    col = lambda c: min(max(c, 0), V - 1)                                  # noqa: E731
    if rows == 1:
        return x, torch.tensor([V - 1])
    assert rows == 9
    labels = torch.tensor([-100, col(0), col(1), col(V - 2), -100, col(V - 1), int(torch.randint(0, V, (1,), generator=g)),
                           col(V // 2), -100])
    x[1] = x[1].sort().values
    x[2] = x[2].sort(descending=True).values
    x[3] = 0.75
    if gamma >= 1 or gamma == 0:
        x[5, V - 1] += 40.0
    return x, labels


def focal_gammas(V):
    """V == 1 is a saturated row (pt == 1) by itself: gamma < 1 has no finite reference gradient there (gamma == 0 is the
    special case d = 1)."""
    return tuple(g for g in GAMMAS if V > 1 or g >= 1 or g == 0)


def _focal_cases():
    out = []

    def add(cls, is16, V, ld, off=0, doff=0, fwd=None, bwd=None):
        out.append(dict(name=f'{cls}-V{V}-ld{ld}', cls=cls, is16=is16, V=V, ld=ld, off=off, doff=doff, fwd=fwd, bwd=bwd))

    for V in (1, 255, 257, 513, 30522):                                   # fp32: 256 threads
        add('fp32', 0, V, V, fwd=F_FP32, bwd=F_FP32)
        add('fp32', 0, V, V + 3, fwd=F_FP32, bwd=F_FP32)
    for V in (2, 6, 130, 2050, 30522):                                    # 16-bit pairs: 1024 threads
        add('pairs', 1, V, V, fwd=F_PAIRS, bwd=F_PAIRS)
        add('pairs', 1, V, V + 6, fwd=F_PAIRS, bwd=F_PAIRS)
    for V in (1, 255, 257, 513):                                          # 2-byte fallback: odd V
        add('odd_v', 1, V, V, fwd=F_HALF, bwd=F_HALF)
        add('odd_v', 1, V, V + 3, fwd=F_HALF, bwd=F_HALF)
    for V in (2, 256, 514, 30522):                                        # 2-byte fallback: even V on an odd stride
        add('odd_ld', 1, V, V + 1, fwd=F_HALF, bwd=F_HALF)
    for V in (2, 130, 514, 30522):                                        # 2-byte fallback: base pointer at an odd element
        add('odd_base', 1, V, V, off=1, doff=1, fwd=F_HALF, bwd=F_HALF)
        add('odd_base', 1, V, V + 6, off=1, doff=1, fwd=F_HALF, bwd=F_HALF)
    add('odd_dbase', 1, 130, 130, off=0, doff=1, fwd=F_PAIRS, bwd=F_HALF)   # only the gradient buffer is off: pairs forward
    add('odd_dbase', 1, 2050, 2056, off=0, doff=1, fwd=F_PAIRS, bwd=F_HALF)
    return out


FOCAL_CASES = _focal_cases()
FOCAL_ROWS = (1, 9)


# -------------------------------------------------------------------------------------------- cos-normalisation, forward and back
# The floor also ADDS IN THE KERNELS' ORDER where an `order` record is given (the fp64 reference never takes one).  Summation
# order is an operation the kernels really perform, and at temperature 0.05 it is the largest term of their error: a
# one-thread sum of 3 G exponentials, a per-lane running (max, sum), a contraction walked sixteen elements at a time.
#   order = dict(large=<multi-workgroup path>, nw=(waves that split the contraction of the score GEMM, of d en0, of d en_k))
# csrc/losses.hip: normalize_body (lane-strided sum of squares, wave_sum), sgemm_nt_kernel and
# sgemm_nt_tiled_kernel (fused multiply-adds in the order of the MFMA steps, the partial tiles of the waves added in wave
# order), nce_loss_body / ns_loss_kernel (`s += __expf(..)` over a row or a column by one thread), lse_push / lse_rows_body /
# lse_cols_body (running maximum with a rescaled sum per lane or wave, then the merge), norm_bwd_kernel (lane-strided
# dot product).
NEG_INF = float('-inf')


def _fma(a, b, c):
    """fl(a * b + c) with one rounding: exact in fp64 for fp32 operands, then rounded once."""
    return (a.double() * b.double() + c.double()).float()


def _tree64(t):
    """wave_sum (common.hpp): lanes l and l ^ 32, then ^ 16, ... ^ 1."""
    n = 64
    while n > 1:
        n //= 2
        t = t[..., :n] + t[..., n:2 * n]
    return t[..., 0]


def _lane_dot(x, y):
    """sum_d x[r][d] y[r][d] as a wave computes it: lane l takes d = l, l + 64, ... in order, then wave_sum."""
    R, n = x.shape
    pad = (-n) % 64
    x = torch.cat([x, x.new_zeros(R, pad)], 1).view(R, -1, 64)
    y = torch.cat([y, y.new_zeros(R, pad)], 1).view(R, -1, 64)
    acc = x.new_zeros(R, 64)
    for c in range(x.shape[1]):
        acc = _fma(x[:, c], y[:, c], acc)
    return _tree64(acc)


def _gemm_nt(A, B, nw, tiled):
    """A [M, K] . B [N, K]^T in the kernels' order: nw waves take kchunk elements each (a multiple of 16), a wave walks its
    elements as the MFMA steps do (sgemm_nt_kernel: step e of a 16-block contracts k0 + {0, 4, 8, 12} + e; the tiled kernel:
    four adjacent elements a step), the partial tiles are added in wave order."""
    M, K = A.shape
    kchunk = ((K + nw * 16 - 1) // (nw * 16)) * 16
    A64, B64 = A.double(), B.double()
    total = None
    for w in range(nw):
        kb, ke = w * kchunk, min(K, (w + 1) * kchunk)
        acc = torch.zeros(M, B.shape[0], dtype=torch.float32)
        for k0 in range(kb, ke, 16):
            ks = range(k0, k0 + 16) if tiled else [k0 + lg * 4 + e for e in range(4) for lg in range(4)]
            for k in ks:
                if k < ke:
                    acc = (acc.double() + A64[:, k, None] * B64[None, :, k]).float()
        total = acc if total is None else total + acc
    return total


def _matmul_nt(A, B, ar, order, which):
    if order is None:
        return A @ B.t()
    return _gemm_nt(A.contiguous(), B.contiguous(), 1 if order['large'] else order['nw'][which], order['large'])


def _lse_seq(x, ar):
    """Rows of x [R, n]: the maximum, then `s += exp(x - m)` element after element (one thread per row)."""
    m = x.max(1).values
    s = torch.zeros_like(m)
    for c in range(x.shape[1]):
        s = s + ar.exp(x[:, c] - m)
    return m + ar.log(s)


def _push(m, s, x, valid, ar):
    """lse_push on every (row, lane) where `valid`: a running maximum and the sum rescaled to it."""
    mn = torch.maximum(m, x)
    ok = valid & (mn > NEG_INF)
    s2 = _fma(s, ar.exp(m - mn), ar.exp(x - mn))
    return torch.where(ok, mn, m), torch.where(ok, s2, s)


def _lse_rows_multi(blocks, ar):
    """lse_rows_body: one wave per row; lane l pushes elements l, l + 64, ... of each block in turn; the 64 (max, sum) pairs
    are merged by wave_max / wave_sum."""
    R, G = blocks[0].shape
    m = torch.full((R, 64), NEG_INF, dtype=ar.dtype)
    s = torch.zeros(R, 64, dtype=ar.dtype)
    lanes = torch.arange(64)
    for blk in blocks:
        for c in range(0, G, 64):
            x = torch.full((R, 64), NEG_INF, dtype=ar.dtype)
            n = min(64, G - c)
            x[:, :n] = blk[:, c:c + n]
            m, s = _push(m, s, x, (lanes < n)[None, :].expand(R, 64), ar)
    wm = m.max(1).values
    t = torch.where(m == NEG_INF, torch.zeros_like(s), s * ar.exp(m - wm[:, None]))
    return wm + ar.log(_tree64(t))


def _lse_cols_multi(blk, ar, waves=16):
    """lse_cols_body: a lane per column; wave w pushes rows w, w + 16, ...; the 16 pairs of a column meet in wave order."""
    G = blk.shape[0]
    m = torch.full((waves, G), NEG_INF, dtype=ar.dtype)
    s = torch.zeros(waves, G, dtype=ar.dtype)
    ws = torch.arange(waves)
    for r in range(0, G, waves):
        x = torch.full((waves, G), NEG_INF, dtype=ar.dtype)
        n = min(waves, G - r)
        x[:n] = blk[r:r + n]
        m, s = _push(m, s, x, (ws < n)[:, None].expand(waves, G), ar)
    bm = m.max(0).values
    bs = torch.zeros(G, dtype=ar.dtype)
    for w in range(waves):
        live = m[w] != NEG_INF
        bs = torch.where(live, _fma(s[w], ar.exp(m[w] - bm), bs), bs)
    return bm + ar.log(bs)


def _lse_rows(blocks, ar, order):
    if order is None:
        return ar.lse(torch.cat(blocks, 1), 1)
    return _lse_rows_multi(blocks, ar) if order['large'] else _lse_seq(torch.cat(blocks, 1), ar)


def _lse_cols(blk, ar, order):
    if order is None:
        return ar.lse(blk, 0)
    return _lse_cols_multi(blk, ar) if order['large'] else _lse_seq(blk.t(), ar)


def _normalise(e, eps, ar, order=None):
    n = (e.pow(2).sum(1) if order is None else _lane_dot(e, e)).sqrt()[:, None]
    inv = 1.0 / n.clamp_min(eps)
    return e * inv, inv, n >= eps


def _normalise_bwd(en, den, inv, live, order=None):
    """d e = inv (d en - en <en, d en>) where |e| >= eps; below eps the clamp rule d e = d en / eps."""
    dot = ((en * den).sum(1) if order is None else _lane_dot(en, den))[:, None]
    return torch.where(live, inv * (den - en * dot), den * inv)


# --------------------------------------------------------------------------------------------------------------- InfoNCE
def nce_ref(es, temperature, margin, gn, gr, ar=FP64, eps=1e-8, order=None):
    """ExclusiveNCEwithRankingLoss on four [G, Dm] tensors (video, text, masked text, reconstruction) with upstream
    gradients gn (nce) and gr (rank).  -> dict(nce, rank, grads [4 x [G, Dm]], hinge [G] = margin - (a - b))."""
    es = [e.to(ar.dtype) for e in es]
    G = es[0].shape[0]
    nrm = [_normalise(e, eps, ar, order) for e in es]
    en = [t[0] for t in nrm]
    it = torch.tensor(1.0 / temperature, dtype=ar.dtype)
    sim = [_matmul_nt(en[0], en[k + 1], ar, order, 0) * it for k in range(3)]
    idx = torch.arange(G)
    eye = torch.eye(G, dtype=torch.bool)
    diag = [s[idx, idx] for s in sim]
    gone = [torch.where(eye, s - (s + 10000.0), s) for s in sim]          # the other blocks' diagonals: x - (x + 10000)
    dsim = [torch.zeros_like(s) for s in sim]
    loss_v = torch.zeros((), dtype=ar.dtype)
    for kx in range(3):
        blocks = [sim[k] if k == kx else gone[k] for k in range(3)]
        row = torch.cat(blocks, 1)                                                      # [G, 3G]
        lse = _lse_rows(blocks, ar, order)
        loss_v = loss_v - (diag[kx] - lse).sum() / G
        p = ar.exp(row - lse[:, None])
        for k in range(3):
            blk = p[:, k * G:(k + 1) * G]
            if k == kx:
                dsim[k] = dsim[k] + (-gn / G) * (eye.to(ar.dtype) - blk)
            else:
                dsim[k] = dsim[k] + (-gn / G) * torch.where(eye, torch.zeros_like(blk), -blk)      # excluded: zero slope
    loss_t = torch.zeros((), dtype=ar.dtype)
    for k in range(3):
        lse = _lse_cols(sim[k], ar, order)
        loss_t = loss_t - (diag[k] - lse).sum() / (3 * G)
        dsim[k] = dsim[k] + (-gn / (3 * G)) * (eye.to(ar.dtype) - ar.exp(sim[k] - lse[None, :]))
    hinge = margin - (diag[0] - diag[1])
    rank = hinge.clamp_min(0).sum() / G
    on = (hinge > 0).to(ar.dtype) * (gr / G)
    dsim[0] = dsim[0] - torch.diag(on)
    dsim[1] = dsim[1] + torch.diag(on)
    den = [_matmul_nt(torch.cat(dsim, 1), torch.cat(en[1:], 0).t(), ar, order, 1) * it]
    den += [_matmul_nt(dsim[k].t(), en[0].t(), ar, order, 2) * it for k in range(3)]
    grads = [_normalise_bwd(en[q], den[q], nrm[q][1], nrm[q][2], order) for q in range(4)]
    return dict(nce=loss_v + loss_t, rank=rank, grads=grads, hinge=hinge, den=den, norm=nrm)


SA, SB = (0, 1, 2, 3), (1, 0, 4, 5)            # the two evaluations of the step on a packed [G, 6, Dm] tensor
NCE_MARGIN = 5.0
WEIGHTS = {'distinct': (1.3, 0.7, 0.9, 1.1), 'nce_only': (1.3, None, 0.9, None), 'rank_only': (None, 0.7, None, 1.1)}


def nce_pair_ref(packed, temperature, wts, ar=FP64, margin=NCE_MARGIN, order=None):
    """Both evaluations on slots SA and SB of packed [G, k, Dm]; wts: upstream gradients of (nce_a, rank_a, nce_b, rank_b),
    None = 0.  -> dict(losses [4], grad [G, k, Dm] (zeros in slots nobody reads), grad_a, grad_b, hinge_a, hinge_b)."""
    w = [0.0 if v is None else v for v in wts]
    out = dict(losses=[])
    total = torch.zeros(packed.shape, dtype=ar.dtype)
    for tag, slots, gn, gr in (('a', SA, w[0], w[1]), ('b', SB, w[2], w[3])):
        r = nce_ref([packed[:, s] for s in slots], temperature, margin, gn, gr, ar, order=order)
        g = torch.zeros(packed.shape, dtype=ar.dtype)
        for q, s in enumerate(slots):
            g[:, s] = r['grads'][q]
        out['grad_' + tag], out['hinge_' + tag] = g, r['hinge']
        out['losses'] += [r['nce'].item(), r['rank'].item()]
        out['parts_' + tag] = r
        total = total + g
    if order is not None:
        # nce_pair_norm_bwd_kernel: a slot both evaluations read gets the SUM of the two d en before the normalisation's
        # Jacobian (en and 1 / norm of a slot are the same numbers in both work areas)
        for s in set(SA) & set(SB):
            ra, rb, qa, qb = out['parts_a'], out['parts_b'], SA.index(s), SB.index(s)
            en, inv, live = ra['norm'][qa]
            total[:, s] = _normalise_bwd(en, ra['den'][qa] + rb['den'][qb], inv, live, order)
    del out['parts_a'], out['parts_b']
    out['grad'] = total
    return out


def nce_packed(G, Dm, k=6, seed=None):
    """packed fp32 [G, k, Dm]: positives correlated; every third row's masked-text slot flipped (slots 2 and 4, offset by a
    row), so that the ranking hinge of both evaluations is active on some rows and inactive on others."""
    seed = 1000 + G + Dm if seed is None else seed
    for _ in range(16):                       # reseed until no row of either evaluation sits within HINGE_GAP of its threshold
        p = mixed_hinge_(torch.randn(G, k, Dm, generator=torch.Generator().manual_seed(seed)))
        if min(hinge_gap(p, slots, t) for slots in (SA, SB) for t in NCE_TEMPS) >= HINGE_GAP:
            return p
        seed += 10007
    raise AssertionError('no seed keeps the hinges away from the threshold')


def hinge_rows(video, text, text_mask, temperature=0.05, margin=5.0):
    """margin - (a - b) per row in fp64: > 0 where the ranking hinge is active."""
    e = [torch.nn.functional.normalize(t.detach().double().cpu(), dim=1, eps=1e-8) for t in (video, text, text_mask)]
    return margin - ((e[0] * e[1]).sum(1) - (e[0] * e[2]).sum(1)) / temperature


def hinge_gap(p, slots, temperature, margin=5.0):
    """min over rows of |margin - (a - b)| of the evaluation on `slots`."""
    return hinge_rows(*[p[:, s] for s in slots[:3]], temperature, margin).abs().min().item()


def assert_mixed_hinge(video, text, text_mask, temperature=0.05, margin=5.0):
    """Both kinds of row exist (from three rows on): the active and the inactive branch of the hinge both run."""
    h = hinge_rows(video, text, text_mask, temperature, margin)
    if len(h) >= 3:
        assert int((h > 0).sum()) > 0 and int((h <= 0).sum()) > 0, (int((h > 0).sum()), int((h <= 0).sum()))


def mixed_hinge_(p):
    p[:, 1] = p[:, 0] * 0.7 + p[:, 1] * 0.5
    p[:, 2] = p[:, 0] * 0.6 + p[:, 2] * 0.6
    p[:, 4] = p[:, 1] * 0.6 + p[:, 4] * 0.6
    p[0::3, 2] = -p[0::3, 2]
    p[1::3, 4] = -p[1::3, 4]
    return p


HINGE_GAP = 0.02          # min |margin - (a - b)|: several thousand fp32 ulps of a similarity of about 20


def hinge_kinds(hinge):
    """(active, inactive) row counts and the smallest distance of a row from the threshold."""
    return int((hinge > 0).sum()), int((hinge <= 0).sum()), hinge.abs().min().item()


CLAMP_G, CLAMP_DM = 5, 40
CLAMP_ROWS = ((1, 0, 0.0), (2, 1, 3e-10), (3, 4, 3e-9))      # (row, slot, norm): all below InfoNCE's eps 1e-8


def nce_clamp_packed():
    """An all-zero row, a row of norm 3e-10 and a row of norm 3e-9, in three different slots."""
    p = nce_packed(CLAMP_G, CLAMP_DM)
    for row, slot, norm in CLAMP_ROWS:
        p[row, slot] = p[row, slot] / p[row, slot].norm() * norm
    return p


# (G, Dm, paths, what the case reaches).  paths: 'small' / 'large' pinned with NCE_FORCE_LARGE, 'auto' by the row count.
def nce_cases(T):
    return [
        (1, 16, ('small', 'large'), 'guards, empty lanes and waves'),
        (3, 40, ('small', 'large'), 'guards, empty lanes and waves, Dm % 16 != 0 in the tiled forward'),
        (17, 300, ('small', 'large'), '8-wave forward, ragged kchunk, idle waves'),
        (33, 257, ('small',), 'waves with kb >= K'),
        (65, 64, ('large',), 'ragged column group'),
        (96, 768, ('small',), '8-wave backward, K = 288'),
        (171, 48, ('small',), 'second trip of the loss kernel'),
        (256, 64, ('small',), '8-wave batch-3 backward, K = G'),
        (131, 80, ('auto',), 'as today'),
        (T, 80, ('auto',), 'as today'),
    ]


NCE_TEMPS = (0.05, 1.0)


# ----------------------------------------------------------------------------------------------------------- NormSoftmax
def ns_ref(video, text, temperature, eps, g, ar=FP64, order=None):
    """NormSoftmaxLoss with the norm clamp eps (1e-12: F.normalize, 1e-8: cos_sim) and upstream gradient g.
    -> dict(loss, dvideo, dtext)."""
    v, t = video.to(ar.dtype), text.to(ar.dtype)
    vn, vinv, vlive = _normalise(v, eps, ar, order)
    tn, tinv, tlive = _normalise(t, eps, ar, order)
    it = torch.tensor(1.0 / temperature, dtype=ar.dtype)
    r = ns_sim_ref(_matmul_nt(vn, tn, ar, order, 0) * it, g, ar, order)
    dv = _matmul_nt(r['dsim'], tn.t(), ar, order, 1) * it
    dt = _matmul_nt(r['dsim'].t(), vn.t(), ar, order, 2) * it
    return dict(loss=r['loss'], dvideo=_normalise_bwd(vn, dv, vinv, vlive, order),
                dtext=_normalise_bwd(tn, dt, tinv, tlive, order))


def ns_sim_ref(x, g, ar=FP64, order=None):
    """The sim_mat entry: the loss on a given [G, G] score matrix.  -> dict(loss, dsim)."""
    x = x.to(ar.dtype)
    G = x.shape[0]
    idx = torch.arange(G)
    lser, lsec = _lse_rows([x], ar, order), _lse_cols(x, ar, order)
    loss = -((x[idx, idx] - lser).sum() + (x[idx, idx] - lsec).sum()) / G
    dsim = (-g / G) * (2 * torch.eye(G, dtype=ar.dtype) - ar.exp(x - lser[:, None]) - ar.exp(x - lsec[None, :]))
    return dict(loss=loss, dsim=dsim)


def ns_inputs(G, Dm, clamp=False):
    g = torch.Generator().manual_seed(7 + G + Dm)
    v, t = torch.randn(G, Dm, generator=g), torch.randn(G, Dm, generator=g)
    t = 0.5 * v + t
    if clamp:                                     # zero, 3e-10 (below both eps), 3e-9 (between 1e-12 and 1e-8)
        v[1] = 0.0
        t[2] = t[2] / t[2].norm() * 3e-10
        v[3] = v[3] / v[3].norm() * 3e-9
    return v, t


NS_CLAMP_ROWS = (('dvideo', 1), ('dtext', 2), ('dvideo', 3))
NS_NORMS = ((0.07, 1e-12), (0.05, 1e-8))         # (temperature, eps): F.normalize and cos_sim
NS_DLOSS = 1.7
# (G, Dm, path, what it reaches)
NS_CASES = [
    (1, 16, 'auto', 'one tile, 15 idle rows and columns'),
    (3, 40, 'auto', 'K % 16 != 0'),
    (33, 257, 'auto', '8-wave forward, waves with kb >= K'),
    (64, 768, 'auto', '8-wave forward, eight full waves'),
    (256, 64, 'small', '8-wave backward, K = G'),
    (65, 64, 'large', 'ragged column group, tiled GEMMs'),
]
NS_SIM_G = (1, 6, 65)


# -------------------------------------------------------------------------------------------------------------- the plans
G_ONE, G_EIGHT, G_VEC, G_GUARD = 0, 1, 2, 3       # kernel classes of clv_loss_gemm_plan


def focal_plan(c, lib):
    from clover_amd import _lib
    p = _lib.ClvFocalPlan()
    es = 2 if c['is16'] else 4
    rc = lib.clv_focal_plan(c['is16'], c['V'], c['ld'], (c['off'] * es) % 4, (c['doff'] * es) % 4, C.byref(p))
    assert rc == 0, (c, rc)
    return p


def nce_plan(lib, G, Dm, pair, large):
    from clover_amd import _lib
    p = _lib.ClvLossPlan()
    assert lib.clv_infonce_plan(G, Dm, Dm, int(pair), int(large), C.byref(p)) == 0
    return p


def ns_plan(lib, G, Dm, sim_mat, large):
    from clover_amd import _lib
    p = _lib.ClvLossPlan()
    assert lib.clv_normsoftmax_plan(G, Dm, int(sim_mat), int(large), C.byref(p)) == 0
    return p


def nce_claims(T):
    """{(G, Dm, large): predicate on the plan of the four-tensor / packed entries} — what each case of nce_cases was
    written to reach."""
    return {
        (1, 16, 0): lambda p: p.fwd.kernel == G_ONE and p.loss_threads == 64 and p.loss_trips == 1,
        (1, 16, 1): lambda p: p.fwd.kernel == G_VEC and p.idle_row_lanes == 63 and p.idle_col_waves == 15 and p.cols_last == 1,
        (3, 40, 0): lambda p: p.fwd.kernel == G_ONE and p.fwd.k_tail == 8,
        (3, 40, 1): lambda p: (p.fwd.kernel == G_GUARD and p.fwd.k_tail == 8 and p.idle_row_lanes == 61
                                and p.idle_col_waves == 13 and p.bwd0.kernel == G_GUARD),
        (17, 300, 0): lambda p: p.fwd.kernel == G_EIGHT and p.fwd.kchunk == 48 and p.fwd.waves_with_work == 7 and p.fwd.k_tail,
        (17, 300, 1): lambda p: p.fwd.kernel == G_GUARD and p.idle_row_lanes == 47 and p.idle_col_waves == 0,
        (33, 257, 0): lambda p: p.fwd.kernel == G_EIGHT and p.fwd.kchunk == 48 and p.fwd.waves_with_work == 6,
        (65, 64, 1): lambda p: p.cols_gx == 2 and p.cols_last == 1 and p.fwd.kernel == G_VEC and p.bwd0.kernel == G_GUARD,
        (96, 768, 0): lambda p: (p.fwd.kernel == G_EIGHT and p.fwd.waves_with_work == 8 and p.bwd0.kernel == G_EIGHT
                                  and p.bwd0.kchunk == 48 and p.bwd0.waves_with_work == 6 and p.bwd1.kernel == G_ONE),
        (171, 48, 0): lambda p: p.loss_threads == 1024 and p.loss_trips == 2,
        (256, 64, 0): lambda p: (p.bwd1.kernel == G_EIGHT and p.bwd1.tiles == 192 and p.bwd0.kernel == G_EIGHT
                                  and p.fwd.kernel == G_ONE),
        (131, 80, 1): lambda p: p.large == 1 and p.fwd.kernel == G_VEC and p.bwd0.kernel == G_GUARD and p.cols_last == 3,
        (T, 80, 1): lambda p: p.large == 1 and p.fwd.kernel == G_VEC and p.bwd0.kernel == G_VEC and p.bwd1.kernel == G_VEC,
    }


def ns_claims():
    return {
        (1, 16, 0): lambda p: p.fwd.kernel == G_ONE and p.fwd.tiles == 1 and p.loss_threads == 1024,
        (3, 40, 0): lambda p: p.fwd.kernel == G_ONE and p.fwd.k_tail == 8,
        (33, 257, 0): lambda p: p.fwd.kernel == G_EIGHT and p.fwd.waves_with_work == 6,
        (64, 768, 0): lambda p: p.fwd.kernel == G_EIGHT and p.fwd.waves_with_work == 8 and p.fwd.k_tail == 0,
        (256, 64, 0): lambda p: p.bwd0.kernel == G_EIGHT and p.bwd1.kernel == G_EIGHT and p.fwd.kernel == G_ONE,
        (65, 64, 1): lambda p: p.cols_last == 1 and p.fwd.kernel == G_VEC and p.bwd0.kernel == G_GUARD,
    }


def path_is_large(path, G, T):
    return {'small': False, 'large': True, 'auto': G >= T}[path]


def force_of(path):
    return {'small': False, 'large': True, 'auto': None}[path]


# --------------------------------------------------------------------------------------------- references, computed once
def plan_order(p):
    """The `order` record of a floor from a ClvLossPlan: the path and the waves that split each contraction."""
    return dict(large=bool(p.large), nw=tuple(g.waves if g.kernel in (G_ONE, G_EIGHT) else 1 for g in (p.fwd, p.bwd0, p.bwd1)))


def _lib_handle():
    from clover_amd import _lib
    return _lib.lib()


@functools.lru_cache(maxsize=None)
def nce_case_refs(G, Dm, temperature, weights, clamp=False, large=None):
    """(packed, fp64 reference, fp32 floor) of the pair form on one case; shared by the tests, never modified.  large: None =
    the floor in torch's own summation order, False / True = in the order of that path's kernels."""
    p = nce_clamp_packed() if clamp else nce_packed(G, Dm)
    order = None if large is None else plan_order(nce_plan(_lib_handle(), G, Dm, 1, large))
    return (p, nce_pair_ref(p, temperature, WEIGHTS[weights], FP64),
            nce_pair_ref(p, temperature, WEIGHTS[weights], FP32, order=order))


@functools.lru_cache(maxsize=None)
def ns_case_refs(G, Dm, temperature, eps, clamp=False, large=None):
    v, t = ns_inputs(G, Dm, clamp)
    order = None if large is None else plan_order(ns_plan(_lib_handle(), G, Dm, 0, large))
    return v, t, ns_ref(v, t, temperature, eps, NS_DLOSS, FP64), ns_ref(v, t, temperature, eps, NS_DLOSS, FP32, order)


@functools.lru_cache(maxsize=None)
def ns_sim_refs(G, large=None):
    x = torch.randn(G, G, generator=torch.Generator().manual_seed(90 + G)) * 3
    order = None if large is None else dict(large=bool(large), nw=(1, 1, 1))
    return x, ns_sim_ref(x, NS_DLOSS, FP64), ns_sim_ref(x, NS_DLOSS, FP32, order)
