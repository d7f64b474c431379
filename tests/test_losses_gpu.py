"""Every launch class of the loss kernels (csrc/losses.hip: focal masked-LM cross entropy, exclusive InfoNCE + ranking,
NormSoftmaxLoss) through the C entries, and once each through clover_amd.ops.  Each test first asserts, through the plan
entries, the class its case was written to reach, then compares with the fp64 reference of tests/loss_ref.py.  The
bounds are multiples of the fp32 floor of the same module (the same formulas in fp32, added in the order of the path's
kernels) — 2 x its RMS error, 4 x its per-row error, 4 x its loss error plus 2^-23 sqrt(n) for a one-workgroup sum of n
terms — never a figure taken from the kernels; tests/LOSS_ERROR_BUDGET.md has the reasoning and the measured table.
`-m gpu` only."""
import ctypes as C
import math

import pytest
import torch

import loss_ref as lr

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SENTINEL, TAIL = -7.0e30, 1024                  # floats beyond the work buffer, on the same allocation
RMS_X, ROW_X, LOSS_X = 2.0, 4.0, 4.0           # margins over the floor


def L():
    from clover_amd import _lib
    return _lib.lib()


def half():
    from clover_amd import _lib
    return _lib.half_dtype()


def T():
    return int(L().clv_infonce_large_min_g())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Budget:
    """Collects (statistic, measured, allowed), prints the worst of each statistic, then asserts all of them."""

    def __init__(self, name):
        self.name, self.worst, self.bad = name, {}, []

    def check(self, stat, got, allowed, where=''):
        ratio = got / allowed if allowed > 0 else (0.0 if got == 0 else math.inf)
        if stat not in self.worst or ratio > self.worst[stat][0]:
            self.worst[stat] = (ratio, got, allowed)
        if not got <= allowed:
            self.bad.append((stat, where, got, allowed))

    def grad(self, stat, got, ref, floor, where=''):
        self.check(stat + '.rms', lr.rms_rel(got, ref), RMS_X * lr.rms_rel(floor, ref), where)
        self.check(stat + '.row', lr.row_stat(got, ref), ROW_X * lr.row_stat(floor, ref), where)

    def loss(self, stat, got, ref, floor, n, where=''):
        self.check(stat, lr.scalar_rel(got, ref), LOSS_X * lr.scalar_rel(floor, ref) + lr.ULP32 * math.sqrt(n), where)

    def done(self):
        print('LOSSBUDGET', self.name, ' '.join(f'{k}={g:.3e}/{a:.3e}({r:.2f})' for k, (r, g, a) in sorted(self.worst.items())))
        assert not self.bad, self.bad[:8]


# =================================================================================================================== focal
def focal_run(c, rows, gamma, x, labels, bud):
    """One forward + backward of case c on the values x (already in the storage type); checks everything."""
    lib, V, ld = L(), c['V'], c['ld']
    dt = x.dtype
    where = (rows, gamma)
    buf = torch.full((c['off'] + rows * ld,), float('nan'), dtype=dt, device=DEV)            # padding columns hold NaN
    lg = buf[c['off']:].view(rows, ld)
    lg[:, :V] = x.to(DEV)
    dbuf = torch.full((c['doff'] + rows * ld,), float('nan'), dtype=dt, device=DEV)
    dlg = dbuf[c['doff']:].view(rows, ld)
    es = x.element_size()
    p = lr.focal_plan(c, lib)
    assert lg.data_ptr() % 4 == (c['off'] * es) % 4 and dlg.data_ptr() % 4 == (c['doff'] * es) % 4
    assert (p.fwd_kernel, p.bwd_kernel) == (c['fwd'], c['bwd'])
    lab = labels.to(DEV)
    row_ce = torch.full((rows,), float('nan'), device=DEV)
    row_lse = torch.full((rows,), float('nan'), device=DEV)
    acc = torch.zeros(2, device=DEV)
    dloss = torch.tensor([lr.FOCAL_DLOSS], device=DEV)
    is16 = int(c['is16'])
    if ld == V:
        assert lib.clv_focal_ce_fwd(ptr(lg), is16, ptr(lab), ptr(row_ce), ptr(row_lse), ptr(acc[0:1]), ptr(acc[1:2]), rows,
                                    V, gamma, stream()) == 0
        assert lib.clv_focal_ce_bwd(ptr(lg), is16, ptr(lab), ptr(row_ce), ptr(row_lse), ptr(acc[1:2]), ptr(dloss), ptr(dlg),
                                    rows, V, gamma, stream()) == 0
    else:
        assert lib.clv_focal_ce_fwd_ld(ptr(lg), is16, ptr(lab), ptr(row_ce), ptr(row_lse), ptr(acc[0:1]), ptr(acc[1:2]),
                                       rows, V, ld, gamma, stream()) == 0
        assert lib.clv_focal_ce_bwd_ld(ptr(lg), is16, ptr(lab), ptr(row_ce), ptr(row_lse), ptr(acc[1:2]), ptr(dloss),
                                       ptr(dlg), rows, V, ld, gamma, stream()) == 0
    torch.cuda.synchronize()
    rt = dt if is16 else None
    ref = lr.focal_ref(x, labels, gamma, lr.FOCAL_DLOSS, ld)
    floor = lr.focal_ref(x, labels, gamma, lr.FOCAL_DLOSS, ld, ar=lr.FP32, round_to=rt)
    n = ref['count']
    assert acc[1].item() == n, where
    ignored = labels < 0
    got = dlg.float().cpu()
    assert not torch.isnan(got).any(), where                                   # every element written
    assert (got[ignored] == 0).all() and (got[:, V:] == 0).all(), where
    assert (row_ce.cpu()[ignored] == 0).all() and (row_lse.cpu()[ignored] == 0).all(), where
    if c['off']:
        assert torch.isnan(buf[:c['off']]).all()
    if c['doff']:
        assert torch.isnan(dbuf[:c['doff']]).all()                             # nothing in front of the view was written
    if n == 0:
        assert math.isnan(acc[0].item()) and (got == 0).all()
        return
    bud.loss('loss', acc[0].item(), ref['loss'].item(), floor['loss'].item(), n, where)
    bud.check('lse', lr.vec_rel(row_lse, ref['lse']), LOSS_X * lr.vec_rel(floor['lse'], ref['lse']) + lr.ULP32, where)
    bud.check('ce', lr.vec_rel(row_ce, ref['ce']), LOSS_X * lr.vec_rel(floor['ce'], ref['ce']) + lr.ULP32, where)
    bud.grad('dlogits', got, ref['dlogits'], floor['dlogits'], where)


@pytest.mark.parametrize('c', lr.FOCAL_CASES, ids=[c['name'] for c in lr.FOCAL_CASES])
def test_focal(c):
    dt = half() if c['is16'] else torch.float32
    bud = Budget('focal ' + c['name'])
    for rows in lr.FOCAL_ROWS:
        for gamma in lr.focal_gammas(c['V']):
            x, labels = lr.focal_inputs(rows, c['V'], gamma, 40 + rows)
            focal_run(c, rows, gamma, x.to(dt), labels, bud)
    bud.done()


@pytest.mark.parametrize('name', ['fp32-V257-ld260', 'pairs-V130-ld136', 'odd_v-V255-ld255', 'odd_ld-V514-ld515',
                                  'odd_base-V130-ld130', 'odd_dbase-V2050-ld2056'])
def test_focal_all_rows_ignored(name):
    c = {k['name']: k for k in lr.FOCAL_CASES}[name]
    x, _ = lr.focal_inputs(9, c['V'], 2.0, 3)
    focal_run(c, 9, 2.0, x.to(half() if c['is16'] else torch.float32), torch.full((9,), -100), Budget('ignored'))


def test_focal_through_ops():
    """ops.focal_ce_masked on the [rows, V] view of a padded score buffer, as the MLM decoder hands it over."""
    from clover_amd import ops
    V, ld, gamma = 2050, 2056, 2.0
    p = lr.focal_plan(dict(is16=1, V=V, ld=ld, off=0, doff=0), L())
    assert (p.fwd_kernel, p.bwd_kernel, p.fwd_trips) == (lr.F_PAIRS, lr.F_PAIRS, 2)      # ops allocates both buffers aligned
    x, labels = lr.focal_inputs(9, V, gamma, 49)
    x = x.to(half())
    buf = torch.full((9, ld), float('nan'), dtype=half(), device=DEV)
    buf[:, :V] = x.to(DEV)
    lg = buf[:, :V].requires_grad_()
    loss = ops.focal_ce_masked(lg, labels.to(DEV), gamma)
    (lr.FOCAL_DLOSS * loss).backward()
    ref = lr.focal_ref(x, labels, gamma, lr.FOCAL_DLOSS)
    floor = lr.focal_ref(x, labels, gamma, lr.FOCAL_DLOSS, ar=lr.FP32, round_to=half())
    bud = Budget('focal ops')
    bud.loss('loss', loss.item(), ref['loss'].item(), floor['loss'].item(), ref['count'])
    bud.grad('dlogits', lg.grad.float().cpu(), ref['dlogits'], floor['dlogits'])
    bud.done()


# ================================================================================================================= InfoNCE
def work_buffer(floats):
    """NaN where the kernels work, a sentinel in the TAIL floats behind it, one allocation."""
    w = torch.full((floats + TAIL,), float('nan'), device=DEV)
    w[floats:] = SENTINEL
    return w


def tail_untouched(w):
    return bool((w[-TAIL:] == SENTINEL).all())


def nce_four(es, ld, G, Dm, temperature, wts, large, ds=None, ldd=None):
    """clv_infonce_fwd / _bwd(_large) on four row-strided tensors.  -> (losses [2], the four gradients)."""
    lib = L()
    fwd = lib.clv_infonce_fwd_large if large else lib.clv_infonce_fwd
    bwd = lib.clv_infonce_bwd_large if large else lib.clv_infonce_bwd
    work = work_buffer(lib.clv_infonce_work_floats(G, Dm))
    out = torch.full((2,), float('nan'), device=DEV)
    assert fwd(*[ptr(e) for e in es], ptr(out), ptr(work), G, Dm, ld, temperature, lr.NCE_MARGIN, stream()) == 0
    dout = torch.tensor([0.0 if w is None else w for w in wts], device=DEV)
    if ds is None:
        ds, ldd = [torch.full((G, Dm), float('nan'), device=DEV) for _ in range(4)], Dm
    assert bwd(None, None, None, None, ptr(dout), ptr(work), *[ptr(d) for d in ds], G, Dm, ldd, temperature,
               lr.NCE_MARGIN, stream()) == 0
    torch.cuda.synchronize()
    assert tail_untouched(work)
    return out.cpu().tolist(), ds


def nce_pair(p7, G, Dm, temperature, wts, large):
    """clv_infonce_pair_fwd / _bwd(_large) on packed [G, 7, Dm].  -> (losses [4], dpacked)."""
    lib = L()
    fwd = lib.clv_infonce_pair_fwd_large if large else lib.clv_infonce_pair_fwd
    bwd = lib.clv_infonce_pair_bwd_large if large else lib.clv_infonce_pair_bwd
    k = p7.shape[1]
    slots = (C.c_int32 * 8)(*(lr.SA + lr.SB))
    work = work_buffer(2 * lib.clv_infonce_work_floats(G, Dm))
    out = torch.full((4,), float('nan'), device=DEV)
    assert fwd(ptr(p7), slots, ptr(out), ptr(work), G, k, Dm, temperature, lr.NCE_MARGIN, stream()) == 0
    ws = [None if w is None else torch.tensor([w], device=DEV) for w in wts]
    dout = (C.c_void_p * 4)(*[None if w is None else w.data_ptr() for w in ws])         # NULL: no gradient arrives
    dp = torch.full(p7.shape, float('nan'), device=DEV)
    assert bwd(dout, ptr(work), slots, ptr(dp), G, k, Dm, temperature, lr.NCE_MARGIN, stream()) == 0
    torch.cuda.synchronize()
    assert tail_untouched(work)
    return out.cpu().tolist(), dp


def poisoned7(p):
    """[G, 6, Dm] -> [G, 7, Dm] on the device with NaN in the slot nobody reads."""
    G, _, Dm = p.shape
    return torch.cat([p, torch.full((G, 1, Dm), float('nan'))], 1).to(DEV).contiguous()


def nce_check(G, Dm, large, bud, clamp=False, weights=tuple(lr.WEIGHTS), temps=lr.NCE_TEMPS):
    for temperature in temps:
        for wname in weights:
            wts = lr.WEIGHTS[wname]
            where = (temperature, wname)
            p, ref, floor = lr.nce_case_refs(G, Dm, temperature, wname, clamp, bool(large))
            p7 = poisoned7(p)
            # ---- the pair entry: both evaluations, the whole packed gradient
            losses, dp = nce_pair(p7, G, Dm, temperature, wts, large)
            for q, (got, r, f) in enumerate(zip(losses, ref['losses'], floor['losses'])):
                bud.loss('nce' if q % 2 == 0 else 'rank', got, r, f, 6 * G if q % 2 == 0 else G, where)
            assert (dp[:, 6] == 0).all(), where                              # a slot nobody reads: zeros, NaN input or not
            nce_grad_check(bud, 'pair', dp[:, :6].cpu(), ref['grad'], floor['grad'], clamp, where)
            if large:                                                        # fixed-order sums: bit for bit from run to run
                losses2, dp2 = nce_pair(p7, G, Dm, temperature, wts, large)
                assert losses2 == losses and torch.equal(dp2[:, :6], dp[:, :6]), where
            # ---- four tensors (evaluation a) and four slots of the packed tensor (a and b)
            es = [p[:, s].contiguous().to(DEV) for s in lr.SA]
            la, da = nce_four(es, Dm, G, Dm, temperature, wts[:2], large)
            assert la == losses[:2], where                                   # the pair form's losses bit for bit
            ga = torch.stack(da, 1).cpu()
            nce_grad_check(bud, 'four', ga, ref['grad_a'][:, list(lr.SA)], floor['grad_a'][:, list(lr.SA)], clamp, where,
                           slots=lr.SA)
            for tag, slots, w2, l2 in (('a', lr.SA, wts[:2], losses[:2]), ('b', lr.SB, wts[2:], losses[2:])):
                dpk = torch.full(p7.shape, float('nan'), device=DEV)
                lp, _ = nce_four([p7[:, s] for s in slots], 7 * Dm, G, Dm, temperature, w2, large,
                                 ds=[dpk[:, s] for s in slots], ldd=7 * Dm)
                assert lp == l2, where
                others = [s for s in range(7) if s not in slots]
                assert torch.isnan(dpk[:, others]).all(), where              # only the four slots are written
                if tag == 'a':
                    assert torch.equal(dpk[:, list(slots)], torch.stack(da, 1)), where      # strided == contiguous, bit for bit
                else:
                    gb = dpk[:, :6].cpu().nan_to_num(0.0)
                    nce_grad_check(bud, 'packed', gb, ref['grad_b'], floor['grad_b'], clamp, where)


def nce_grad_check(bud, stat, got, ref, floor, clamp, where, slots=None):
    """got / ref / floor [G, k, Dm].  The clamp rows (gradients about 1e8 times the others) are compared against their own
    row max, the other rows among themselves."""
    if not clamp:
        bud.grad(stat, got, ref, floor, where)
        return
    mask = torch.zeros(got.shape[:2], dtype=torch.bool)
    for row, slot, _ in lr.CLAMP_ROWS:
        if slots is None:
            mask[row, slot] = True
        elif slot in slots:
            mask[row, slots.index(slot)] = True
    bud.grad(stat, got[~mask], ref[~mask], floor[~mask], where)
    for i, j in mask.nonzero().tolist():
        assert torch.isfinite(got[i, j]).all()
        bud.check(stat + '.clamp', lr.row_stat(got[i, j][None], ref[i, j][None]),
                  ROW_X * lr.row_stat(floor[i, j][None], ref[i, j][None]), where + (i, j))


def _nce_ids():
    return [(G, Dm, path) for G, Dm, paths, _ in lr.nce_cases(128) for path in paths]


@pytest.mark.parametrize('G,Dm,path', _nce_ids())
def test_infonce(G, Dm, path):
    if (G, Dm) == (128, 80):
        G = T()
    large = lr.path_is_large(path, G, T())
    p = lr.nce_plan(L(), G, Dm, 0, large)
    assert lr.nce_claims(T())[(G, Dm, int(large))](p), (G, Dm, path)
    # the pair form: the same classes, but on the tiled path a second work area off a 16-byte boundary takes guarded staging
    q = lr.nce_plan(L(), G, Dm, 1, large)
    if large and L().clv_infonce_work_floats(G, Dm) % 4:
        assert (q.fwd.kernel, q.bwd0.kernel, q.bwd1.kernel) == (lr.G_GUARD,) * 3, (G, Dm, path)
    else:
        assert [g.kernel for g in (q.fwd, q.bwd0, q.bwd1)] == [g.kernel for g in (p.fwd, p.bwd0, p.bwd1)], (G, Dm, path)
    bud = Budget(f'infonce G{G} Dm{Dm} {"multi" if large else "one"}')
    nce_check(G, Dm, large, bud)
    bud.done()


@pytest.mark.parametrize('large', [False, True])
def test_infonce_clamp_rows(large):
    """An all-zero row and rows of norm 3e-10 and 3e-9 (all below eps = 1e-8): d e = d en / eps, finite."""
    bud = Budget(f'infonce clamp {"multi" if large else "one"}')
    nce_check(lr.CLAMP_G, lr.CLAMP_DM, large, bud, clamp=True, weights=('distinct',))
    bud.done()


WORK_FILL = 0x4B3C2D1E                          # a finite float (about 1.2e7): what no kernel wrote stays comparable


def filled(floats):
    return torch.full((floats,), WORK_FILL, dtype=torch.int32, device=DEV).view(torch.float32)


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize('G,Dm,large', [(17, 80, False), (17, 80, True), (65, 48, True)])
def test_infonce_single_is_one_direction_of_pair(G, Dm, large):
    """The four-tensor entry on the slots of a direction leaves, bit for bit, the losses and the WHOLE work area that the
    pair entry leaves for that direction: after the forward, and again after the backward (d sim, its transpose, d en).
    G = 65 on the multi-workgroup form: a second, one-lane trip of the row kernel and a second, one-column workgroup of
    the column kernel."""
    lib, sfx = L(), '_large' if large else ''
    pl = lr.nce_plan(lib, G, Dm, 0, large)
    assert pl.large == int(large)
    if G == 65:
        assert pl.cols_gx == 2 and pl.cols_last == 1 and pl.rows_grid == (3 * G + 3) // 4
        assert (G + 63) // 64 == 2 and G % 64 == 1          # a row's 64 lanes stride its G scores: a second trip of one lane
    p = lr.nce_packed(G, Dm).to(DEV)
    k, wf = p.shape[1], lib.clv_infonce_work_floats(G, Dm)
    temperature, wts = 0.05, lr.WEIGHTS['distinct']
    slots = (C.c_int32 * 8)(*(lr.SA + lr.SB))
    pwork, pout = filled(2 * wf), torch.full((4,), float('nan'), device=DEV)
    assert getattr(lib, 'clv_infonce_pair_fwd' + sfx)(ptr(p), slots, ptr(pout), ptr(pwork), G, k, Dm, temperature,
                                                        lr.NCE_MARGIN, stream()) == 0
    single = []
    for d, sl in enumerate((lr.SA, lr.SB)):
        work, out = filled(wf), torch.full((2,), float('nan'), device=DEV)
        es = [C.c_void_p(p.data_ptr() + 4 * Dm * s) for s in sl]
        assert getattr(lib, 'clv_infonce_fwd' + sfx)(*es, ptr(out), ptr(work), G, Dm, k * Dm, temperature, lr.NCE_MARGIN,
                                                      stream()) == 0
        torch.cuda.synchronize()
        assert same_bits(out, pout[2 * d:2 * d + 2]), (d, out.tolist(), pout.tolist())
        assert same_bits(work, pwork[d * wf:(d + 1) * wf]), ('forward', d)
        single.append(work)
    ws = [torch.tensor([w], device=DEV) for w in wts]
    dout = (C.c_void_p * 4)(*[w.data_ptr() for w in ws])
    dp = torch.empty(G, k, Dm, device=DEV)
    assert getattr(lib, 'clv_infonce_pair_bwd' + sfx)(dout, ptr(pwork), slots, ptr(dp), G, k, Dm, temperature,
                                                        lr.NCE_MARGIN, stream()) == 0
    for d, work in enumerate(single):
        d2 = torch.tensor(wts[2 * d:2 * d + 2], device=DEV)
        ds = [torch.empty(G, Dm, device=DEV) for _ in range(4)]
        assert getattr(lib, 'clv_infonce_bwd' + sfx)(None, None, None, None, ptr(d2), ptr(work), *[ptr(g) for g in ds], G, Dm,
                                                      Dm, temperature, lr.NCE_MARGIN, stream()) == 0
        torch.cuda.synchronize()
        assert same_bits(work, pwork[d * wf:(d + 1) * wf]), ('backward', d)


@pytest.mark.parametrize('G,Dm,force', [(17, 300, False), (17, 300, True), (131, 80, None), (96, 768, None)])
def test_infonce_through_ops(G, Dm, force):
    from clover_amd import ops
    large = (G >= T()) if force is None else force
    assert lr.nce_plan(L(), G, Dm, 1, large).large == int(large)
    assert lr.nce_claims(T())[(G, Dm, int(large))](lr.nce_plan(L(), G, Dm, 0, large))
    p, ref, floor = lr.nce_case_refs(G, Dm, 0.05, 'distinct', False, bool(large))
    bud = Budget(f'infonce ops G{G} Dm{Dm} {"multi" if large else "one"}')
    ops.NCE_FORCE_LARGE = force
    try:
        pg = p.to(DEV).requires_grad_()
        outs = ops.exclusive_infonce_rank_pair(pg, lr.SA, lr.SB, 0.05, lr.NCE_MARGIN)
        sum(w * o for w, o in zip(lr.WEIGHTS['distinct'], outs)).backward()
        es = [p[:, s].contiguous().to(DEV).requires_grad_() for s in lr.SA]
        nce, rank = ops.exclusive_infonce_rank(*es, 0.05, lr.NCE_MARGIN)
        (lr.WEIGHTS['distinct'][0] * nce + lr.WEIGHTS['distinct'][1] * rank).backward()
        pk = p.to(DEV).requires_grad_()
        nce2, rank2 = ops.exclusive_infonce_rank_packed(pk, lr.SA, 0.05, lr.NCE_MARGIN)
        (lr.WEIGHTS['distinct'][0] * nce2 + lr.WEIGHTS['distinct'][1] * rank2).backward()
    finally:
        ops.NCE_FORCE_LARGE = None
    for q, (got, r, f) in enumerate(zip(outs, ref['losses'], floor['losses'])):
        bud.loss('nce' if q % 2 == 0 else 'rank', got.item(), r, f, 6 * G if q % 2 == 0 else G)
    bud.grad('pair', pg.grad.cpu(), ref['grad'], floor['grad'])
    assert (nce.item(), rank.item()) == (outs[0].item(), outs[1].item()) == (nce2.item(), rank2.item())
    ga = torch.stack([e.grad for e in es], 1)
    bud.grad('four', ga.cpu(), ref['grad_a'][:, list(lr.SA)], floor['grad_a'][:, list(lr.SA)])
    assert torch.equal(pk.grad[:, list(lr.SA)], ga) and (pk.grad[:, [4, 5]] == 0).all()
    bud.done()


# ============================================================================================================= NormSoftmax
def ns_run(v, t, x, G, Dm, temperature, eps, large):
    """clv_normsoftmax_fwd / _bwd(_large): embeddings (x None) or a given score matrix.  -> (loss, dvideo, dtext, dsim)."""
    lib = L()
    fwd = lib.clv_normsoftmax_fwd_large if large else lib.clv_normsoftmax_fwd
    bwd = lib.clv_normsoftmax_bwd_large if large else lib.clv_normsoftmax_bwd
    work = work_buffer(lib.clv_normsoftmax_work_floats(G, Dm))
    out = torch.full((1,), float('nan'), device=DEV)
    assert fwd(ptr(v), ptr(t), ptr(x), ptr(out), ptr(work), G, Dm, temperature, eps, stream()) == 0
    dout = torch.tensor([lr.NS_DLOSS], device=DEV)
    dv = dt = dsim = None
    if x is None:
        dv, dt = torch.full((G, Dm), float('nan'), device=DEV), torch.full((G, Dm), float('nan'), device=DEV)
    else:
        dsim = torch.full((G, G), float('nan'), device=DEV)
    assert bwd(ptr(x), ptr(dout), ptr(work), ptr(dv), ptr(dt), ptr(dsim), G, Dm, temperature, stream()) == 0
    torch.cuda.synchronize()
    assert tail_untouched(work)
    return out.item(), dv, dt, dsim


def ns_check(G, Dm, large, bud, clamp=False):
    for temperature, eps in lr.NS_NORMS:
        where = (temperature, eps)
        v, t, ref, floor = lr.ns_case_refs(G, Dm, temperature, eps, clamp, bool(large))
        loss, dv, dt, _ = ns_run(v.to(DEV), t.to(DEV), None, G, Dm, temperature, eps, large)
        bud.loss('loss', loss, ref['loss'].item(), floor['loss'].item(), 2 * G, where)
        if large:
            again = ns_run(v.to(DEV), t.to(DEV), None, G, Dm, temperature, eps, large)
            assert again[0] == loss and torch.equal(again[1], dv) and torch.equal(again[2], dt)
        for name, got in (('dvideo', dv.cpu()), ('dtext', dt.cpu())):
            assert torch.isfinite(got).all(), (name, where)
            # below eps = 1e-12 only the zero row is clamped; the two tiny rows are huge all the same: each against itself
            special = [row for n, row in lr.NS_CLAMP_ROWS if n == name] if clamp else []
            keep = torch.ones(G, dtype=torch.bool)
            keep[special] = False
            bud.grad(name, got[keep], ref[name][keep], floor[name][keep], where)
            for row in special:
                bud.check(name + '.clamp', lr.row_stat(got[row][None], ref[name][row][None]),
                          ROW_X * lr.row_stat(floor[name][row][None], ref[name][row][None]), where + (row,))


@pytest.mark.parametrize('G,Dm,path', [c[:3] for c in lr.NS_CASES])
def test_normsoftmax(G, Dm, path):
    large = lr.path_is_large(path, G, T())
    assert lr.ns_claims()[(G, Dm, int(large))](lr.ns_plan(L(), G, Dm, 0, large))
    bud = Budget(f'normsoftmax G{G} Dm{Dm} {"multi" if large else "one"}')
    ns_check(G, Dm, large, bud)
    bud.done()


@pytest.mark.parametrize('large', [False, True])
def test_normsoftmax_clamp_rows(large):
    bud = Budget(f'normsoftmax clamp {"multi" if large else "one"}')
    ns_check(lr.CLAMP_G, lr.CLAMP_DM, large, bud, clamp=True)
    bud.done()


@pytest.mark.parametrize('large', [False, True])
@pytest.mark.parametrize('G', lr.NS_SIM_G)
def test_normsoftmax_sim_mat(G, large):
    p = lr.ns_plan(L(), G, 0, 1, large)
    assert p.large == int(large) and p.fwd.waves == 0 and (p.cols_last == (G - 1) % 64 + 1 if large else p.loss_trips == 1)
    x, ref, floor = lr.ns_sim_refs(G, bool(large))
    loss, _, _, dsim = ns_run(None, None, x.to(DEV), G, 0, 1.0, 1.0, large)
    bud = Budget(f'normsoftmax sim_mat G{G} {"multi" if large else "one"}')
    bud.loss('loss', loss, ref['loss'].item(), floor['loss'].item(), 2 * G)
    bud.grad('dsim', dsim.cpu(), ref['dsim'], floor['dsim'])
    bud.done()


def test_normsoftmax_through_ops():
    from clover_amd import ops
    G, Dm = 33, 257
    assert G < T() and lr.ns_claims()[(G, Dm, 0)](lr.ns_plan(L(), G, Dm, 0, False))       # dispatched to the one-workgroup path
    bud = Budget('normsoftmax ops')
    for temperature, eps in lr.NS_NORMS:
        v, t, ref, floor = lr.ns_case_refs(G, Dm, temperature, eps, False, False)
        vg, tg = v.to(DEV).requires_grad_(), t.to(DEV).requires_grad_()
        loss = ops.norm_softmax_loss(vg, tg, temperature=temperature, eps=eps)
        (lr.NS_DLOSS * loss).backward()
        bud.loss('loss', loss.item(), ref['loss'].item(), floor['loss'].item(), 2 * G)
        bud.grad('dvideo', vg.grad.cpu(), ref['dvideo'], floor['dvideo'])
        bud.grad('dtext', tg.grad.cpu(), ref['dtext'], floor['dtext'])
    bud.done()
