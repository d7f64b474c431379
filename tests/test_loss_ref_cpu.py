"""tests/loss_ref.py itself, without a GPU: the plan entries of csrc/losses.hip say what every case of the tables was written
to reach and every class of clv_focal_plan and of the three GEMMs of clv_infonce_plan is reached by some case (the NormSoftmax
shapes reach the subset test_normsoftmax_cases_reach_their_classes lists: no guarded forward, no vector-staged backward —
the same kernels, which the InfoNCE cases run); the input builders keep their conditions (both kinds of
hinge row, a hinge away from its threshold, a saturated focal row, finite reference gradients); the fp64 references agree
with ``oracle.model`` under autograd to 1e-12; the fp32 floor is a rounding distance away from them."""
import ctypes as C
import os
import re

import pytest
import torch

import loss_ref as lr
from clover_amd import _lib
from oracle import model as om

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('clv_loss_gemm_plan', 'clv_focal_plan', 'clv_infonce_plan', 'clv_normsoftmax_plan')


def L():
    return _lib.lib()


def T():
    return int(L().clv_infonce_large_min_g())


def rel(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300)).item()


# --------------------------------------------------------------------------------------------------------------- symbols
def test_symbols_binding_and_abi_version():
    hdr = open(os.path.join(ROOT, 'include', 'clover_hip.h')).read()
    assert re.search(r'#define CLV_ABI_VERSION 20\b', hdr) and _lib.ABI_VERSION == 20        # new symbols only
    for name in NEW:
        assert re.search(r'\b%s\(' % name, hdr) and name in _lib.SIGNATURES, name
    for fname in ('libclover_hip.so', 'libclover_hip_f16.so'):
        so = C.CDLL(os.path.join(ROOT, 'clover_amd', fname))
        for name in NEW:
            assert hasattr(so, name), (fname, name)
        so.clv_abi_version.restype = C.c_int
        assert so.clv_abi_version() == 20, fname
    assert C.sizeof(_lib.ClvLossGemmPlan) == 32 and C.sizeof(_lib.ClvFocalPlan) == 24
    assert C.sizeof(_lib.ClvLossPlan) == 3 * 32 + 40


def test_plan_entries_reject_what_the_launches_reject():
    g, f, p = _lib.ClvLossGemmPlan(), _lib.ClvFocalPlan(), _lib.ClvLossPlan()
    assert L().clv_loss_gemm_plan(4, 4, 0, 4, 4, 1, 0, 0, 0, 0, 0, 0, C.byref(g)) == -1
    assert L().clv_loss_gemm_plan(4, 4, 4, 4, 4, 1, 0, 0, 0, 0, 0, 0, None) == -1
    assert L().clv_focal_plan(1, 8, 7, 0, 0, C.byref(f)) == -1 and L().clv_focal_plan(1, 0, 8, 0, 0, C.byref(f)) == -1
    assert L().clv_infonce_plan(0, 8, 8, 0, 0, C.byref(p)) == -1 and L().clv_infonce_plan(4, 8, 7, 0, 0, C.byref(p)) == -1
    assert L().clv_normsoftmax_plan(4, 0, 0, 0, C.byref(p)) == -1 and L().clv_normsoftmax_plan(4, 0, 1, 0, C.byref(p)) == 0
    assert p.fwd.waves == 0 and p.bwd0.waves == 0 and p.loss_threads == 1024            # sim_mat: no GEMM runs


# ----------------------------------------------------------------------------------------------------------- GEMM classes
def gemm_plan(M, N, K, lda, ldb, batch=1, sA=0, sB=0, s2=0, a=0, b=0, tiled=0):
    p = _lib.ClvLossGemmPlan()
    assert L().clv_loss_gemm_plan(M, N, K, lda, ldb, batch, sA, sB, s2, a, b, tiled, C.byref(p)) == 0
    return p


def test_loss_gemm_plan_classes_and_wave_split():
    p = gemm_plan(17, 17, 255, 255, 255)
    assert (p.kernel, p.waves, p.kchunk, p.waves_with_work, p.k_tail) == (lr.G_ONE, 1, 256, 1, 15)
    p = gemm_plan(17, 17, 256, 256, 256)
    assert (p.kernel, p.waves, p.kchunk, p.waves_with_work, p.tiles) == (lr.G_EIGHT, 8, 32, 8, 4)
    p = gemm_plan(17, 17, 257, 257, 257)                     # kchunk 48: waves 6 and 7 start at or beyond K
    assert (p.kernel, p.kchunk, p.waves_with_work, p.k_tail) == (lr.G_EIGHT, 48, 6, 1)
    assert gemm_plan(96, 768, 288, 288, 384).tiles == 288 and gemm_plan(96, 768, 288, 288, 384).kernel == lr.G_EIGHT
    assert gemm_plan(200, 768, 600, 600, 800).kernel == lr.G_ONE           # 13 x 48 = 624 tiles > 512
    assert gemm_plan(128, 128, 768, 768, 768, batch=3).tiles == 192        # the limit counts one evaluation's tiles
    for kw, want in [(dict(), lr.G_VEC), (dict(K=80), lr.G_VEC), (dict(K=40), lr.G_GUARD), (dict(lda=82), lr.G_GUARD),
                     (dict(ldb=81), lr.G_GUARD), (dict(sA=2), lr.G_GUARD), (dict(sB=6), lr.G_GUARD), (dict(s2=1), lr.G_GUARD),
                     (dict(a=4), lr.G_GUARD), (dict(b=8), lr.G_GUARD)]:
        args = dict(M=130, N=70, K=64, lda=80, ldb=80, batch=3, tiled=1)
        args.update(kw)
        p = gemm_plan(**args)
        assert (p.kernel, p.waves, p.kchunk, p.gx, p.gy) == (want, 4, 16, 2, 3), kw


# ---------------------------------------------------------------------------------------------------------- case tables
def test_focal_cases_reach_their_classes():
    seen = set()
    for c in lr.FOCAL_CASES:
        p = lr.focal_plan(c, L())
        assert (p.fwd_kernel, p.bwd_kernel) == (c['fwd'], c['bwd']), c
        assert p.fwd_threads == (1024 if c['fwd'] == lr.F_PAIRS else 256), c
        assert p.bwd_threads == (1024 if c['bwd'] == lr.F_PAIRS else 256), c
        seen.add((c['cls'], c['ld'] > c['V']))
    by = {c['name']: lr.focal_plan(c, L()) for c in lr.FOCAL_CASES}
    assert by['pairs-V2-ld2'].fwd_waves_with_work == 1                   # 15 of 16 waves empty
    assert by['pairs-V130-ld130'].fwd_waves_with_work == 2 and by['pairs-V130-ld130'].fwd_trips == 1
    assert by['pairs-V2050-ld2050'].fwd_trips == 2                       # the first width where a thread rescales its sum
    assert by['pairs-V30522-ld30528'].fwd_trips == 15
    assert by['fp32-V255-ld255'].fwd_trips == 1 and by['fp32-V257-ld257'].fwd_trips == 2
    assert by['odd_v-V513-ld513'].fwd_trips == 3 and by['odd_v-V1-ld1'].fwd_waves_with_work == 1
    # every class dense and padded (an odd stride is padded by construction)
    for cls in ('fp32', 'pairs', 'odd_v', 'odd_base', 'odd_dbase'):
        assert (cls, False) in seen and (cls, True) in seen, cls
    assert ('odd_ld', True) in seen
    kernels = {(c['fwd'], c['bwd']) for c in lr.FOCAL_CASES}
    assert kernels == {(0, 0), (1, 1), (2, 2), (2, 1)}
    for cls, want in [('fp32', {1, 255, 257, 513, 30522}), ('pairs', {2, 6, 130, 2050, 30522})]:
        assert {c['V'] for c in lr.FOCAL_CASES if c['cls'] == cls} == want
    assert {c['V'] for c in lr.FOCAL_CASES if c['fwd'] == lr.F_HALF} >= {1, 255, 257, 513, 30522}


def test_infonce_cases_reach_their_classes():
    claims = lr.nce_claims(T())
    used, gemms, trips, ragged, lanes = set(), set(), set(), set(), set()
    for G, Dm, paths, _ in lr.nce_cases(T()):
        for path in paths:
            large = int(lr.path_is_large(path, G, T()))
            p = lr.nce_plan(L(), G, Dm, 0, large)
            assert p.large == large and claims[(G, Dm, large)](p), (G, Dm, path)
            used.add((G, Dm, large))
            for pair in (0, 1):
                q = lr.nce_plan(L(), G, Dm, pair, large)
                gemms |= {(n, getattr(q, n).kernel) for n in ('fwd', 'bwd0', 'bwd1')}
            if large:
                ragged.add(p.cols_last < 64)
                lanes.add((p.idle_row_lanes > 0, p.idle_col_waves > 0))
                assert (p.rows_grid, p.cols_gx, p.cols_gy, p.finish_threads) == ((3 * G + 3) // 4, (G + 63) // 64, 3, 256)
            else:
                trips.add(p.loss_trips)
                assert p.loss_threads == min(1024, max(64, (6 * G + 63) // 64 * 64))
    assert used == set(claims)                                           # no claim without its case
    # every class of every GEMM of the section; both trip counts; ragged and full column groups; idle lanes / waves or none
    assert gemms >= {('fwd', k) for k in range(4)} | {('bwd0', k) for k in range(4)} | {('bwd1', k) for k in range(4)}
    assert trips == {1, 2} and ragged == {True, False}
    assert lanes == {(True, True), (True, False), (False, False)}
    # the pair form of an odd G: the second work area is not 16-byte aligned
    assert lr.nce_plan(L(), T() + 3, 80, 1, 1).fwd.kernel == lr.G_GUARD and lr.nce_plan(L(), T(), 80, 1, 1).fwd.kernel == lr.G_VEC


def test_normsoftmax_cases_reach_their_classes():
    claims = lr.ns_claims()
    used, gemms = set(), set()
    for G, Dm, path, _ in lr.NS_CASES:
        large = int(lr.path_is_large(path, G, T()))
        p = lr.ns_plan(L(), G, Dm, 0, large)
        assert claims[(G, Dm, large)](p), (G, Dm, path)
        used.add((G, Dm, large))
        gemms |= {(n, getattr(p, n).kernel) for n in ('fwd', 'bwd0', 'bwd1')}
        if large:
            assert (p.rows_grid, p.cols_gx, p.cols_gy) == ((G + 3) // 4, (G + 63) // 64, 1)
        else:
            assert (p.loss_threads, p.loss_trips) == (1024, (2 * G + 1023) // 1024)
    assert used == set(claims)
    assert gemms >= {('fwd', lr.G_ONE), ('fwd', lr.G_EIGHT), ('fwd', lr.G_VEC), ('bwd0', lr.G_ONE), ('bwd0', lr.G_EIGHT),
                     ('bwd0', lr.G_GUARD), ('bwd1', lr.G_EIGHT), ('bwd1', lr.G_GUARD)}
    assert lr.CLAMP_G < T() and all(g in (1, 6, 65) for g in lr.NS_SIM_G)


# ------------------------------------------------------------------------------------------------------ input conditions
def test_infonce_inputs_have_both_kinds_of_hinge_row():
    cases = [(G, Dm) for G, Dm, _, _ in lr.nce_cases(T())] + [(8, 64), (64, 768), (200, 768), (1024, 768)]
    for G, Dm in cases:
        p = lr.nce_packed(G, Dm)
        for temperature in lr.NCE_TEMPS if G <= 256 else (0.05,):
            r = lr.nce_pair_ref(p, temperature, lr.WEIGHTS['distinct'])
            for tag in 'ab':
                on, off, gap = lr.hinge_kinds(r['hinge_' + tag])
                assert gap >= lr.HINGE_GAP, (G, Dm, temperature, tag, gap)
                if temperature == 0.05 and G >= 3:                       # at T = 1 a - b <= 2 < margin: every row is active
                    assert on > 0 and off > 0, (G, Dm, tag, on, off)
                if temperature == 1.0:
                    assert off == 0
    r = lr.nce_pair_ref(lr.nce_packed(96, 768), 0.05, lr.WEIGHTS['distinct'])
    assert lr.hinge_kinds(r['hinge_a'])[:2] == (64, 32)
    # the recipe the older tests used never switches a hinge off
    g = torch.Generator().manual_seed(5)
    old = torch.randn(64, 6, 128, generator=g)
    old[:, 1] = old[:, 0] * 0.7 + old[:, 1] * 0.5
    old[:, 2] = old[:, 0] * 0.6 + old[:, 2] * 0.6
    assert lr.hinge_kinds(lr.nce_pair_ref(old, 0.05, lr.WEIGHTS['distinct'])['hinge_a'])[1] == 0


def test_clamp_rows_have_finite_gradients_far_above_the_others():
    for temperature in lr.NCE_TEMPS:
        p, ref, floor = lr.nce_case_refs(lr.CLAMP_G, lr.CLAMP_DM, temperature, 'distinct', True)
        assert torch.isfinite(ref['grad']).all() and torch.isfinite(floor['grad']).all()
        assert min(lr.hinge_kinds(ref['hinge_' + t])[2] for t in 'ab') >= lr.HINGE_GAP
        mask = torch.zeros(p.shape[:2], dtype=torch.bool)
        for row, slot, norm in lr.CLAMP_ROWS:
            assert abs(p[row, slot].norm().item() - norm) <= 1e-6 * norm and norm < 1e-8
            mask[row, slot] = True
        rest = ref['grad'][~mask].abs().max().item()
        for row, slot, _ in lr.CLAMP_ROWS:
            assert ref['grad'][row, slot].abs().max().item() > 1e6 * rest
    for temperature, eps in lr.NS_NORMS:
        v, t, ref, floor = lr.ns_case_refs(lr.CLAMP_G, lr.CLAMP_DM, temperature, eps, True)
        assert all(torch.isfinite(ref[k]).all() and torch.isfinite(floor[k]).all() for k in ('dvideo', 'dtext'))
        assert v[1].norm() == 0 and 1e-12 < t[2].norm() < 1e-9 < v[3].norm() < 1e-8     # between the two eps values
        for name, row in lr.NS_CLAMP_ROWS:
            assert ref[name][row].abs().max().item() > 1e6 * ref['dvideo'][0].abs().max().item()


@pytest.mark.parametrize('V', [1, 2, 6, 255, 2050])
def test_focal_inputs_keep_their_rows(V):
    for gamma in lr.GAMMAS:
        x, labels = lr.focal_inputs(9, V, gamma, 3)
        assert labels[0] < 0 and labels[4] < 0 and labels[8] < 0 and int((labels >= 0).sum()) == 6
        assert [int(v) for v in labels[[1, 2, 3, 5]]] == [0, min(1, V - 1), max(V - 2, 0), V - 1]
        assert (x[1].diff() >= 0).all() and (x[2].diff() <= 0).all() and (x[3] == x[3, 0]).all()
        r = lr.focal_ref(x, labels, gamma, lr.FOCAL_DLOSS, V + 3)
        if gamma not in lr.focal_gammas(V):
            assert not torch.isfinite(r['dlogits']).all()                # why the combination is left out
            continue
        assert torch.isfinite(r['dlogits']).all() and torch.isfinite(r['loss'])
        if V > 1 and (gamma >= 1 or gamma == 0):
            assert r['ce'][5] < 1e-12                                    # the saturated row: pt -> 1
        assert (r['dlogits'][:, V:] == 0).all() and (r['dlogits'][labels < 0] == 0).all()
    x, labels = lr.focal_inputs(1, V, 2.0, 3)
    assert labels.tolist() == [V - 1]
    r = lr.focal_ref(x, torch.tensor([-100]), 2.0, 1.0)
    assert r['count'] == 0 and torch.isnan(r['loss']) and (r['dlogits'] == 0).all()


def test_a_saturated_row_has_no_finite_reference_gradient_below_gamma_one():
    x = torch.zeros(1, 8)
    x[0, 7] = 40.0
    assert not torch.isfinite(lr.focal_ref(x, torch.tensor([7]), 0.5, 1.0)['dlogits']).all()
    assert torch.isfinite(lr.focal_ref(x, torch.tensor([7]), 1.0, 1.0)['dlogits']).all()


# ------------------------------------------------------------------------------------------- references against the oracle
@pytest.mark.parametrize('gamma', lr.GAMMAS)
@pytest.mark.parametrize('V', [2, 6, 257])
def test_focal_reference_equals_oracle_autograd(V, gamma):
    x, labels = lr.focal_inputs(9, V, gamma, 11)
    rows = torch.where(labels >= 0)[0]
    xr = x.double().requires_grad_()
    loss = om.focal_loss_multiclass(xr[rows], labels[rows], gamma)
    (lr.FOCAL_DLOSS * loss).backward()
    r = lr.focal_ref(x, labels, gamma, lr.FOCAL_DLOSS)
    assert abs(r['loss'].item() - loss.item()) <= 1e-12 * max(1.0, abs(loss.item()))
    assert lr.row_stat(r['dlogits'], xr.grad) <= 1e-12
    ce = torch.nn.functional.cross_entropy(x.double()[rows], labels[rows], reduction='none')
    assert (r['ce'][rows] - ce).abs().max() <= 1e-12 and r['count'] == 6
    assert (r['lse'][rows] - torch.logsumexp(x.double()[rows], 1)).abs().max() <= 1e-12


def oracle_pair(p, temperature, wts):
    pr = p.double().requires_grad_()
    la = om.exclusive_nce_rank_loss(*[pr[:, s] for s in lr.SA], temperature=temperature, margin=lr.NCE_MARGIN, gather=False)
    lb = om.exclusive_nce_rank_loss(*[pr[:, s] for s in lr.SB], temperature=temperature, margin=lr.NCE_MARGIN, gather=False)
    losses = [la['nce_loss'], la['rank_t_tm_loss'], lb['nce_loss'], lb['rank_t_tm_loss']]
    sum(w * l for w, l in zip(wts, losses) if w is not None).backward()
    return [l.item() for l in losses], pr.grad


@pytest.mark.parametrize('weights', list(lr.WEIGHTS))
@pytest.mark.parametrize('G,Dm', [(1, 16), (3, 40), (17, 300), (33, 257)])
def test_infonce_reference_equals_oracle_autograd(G, Dm, weights):
    for temperature in lr.NCE_TEMPS:
        p, ref, _ = lr.nce_case_refs(G, Dm, temperature, weights)
        losses, grad = oracle_pair(p, temperature, lr.WEIGHTS[weights])
        for a, b in zip(ref['losses'], losses):
            assert abs(a - b) <= 1e-12 * max(1.0, abs(b)), (a, b)
        assert lr.row_stat(ref['grad'], grad) <= 1e-12, lr.row_stat(ref['grad'], grad)
        assert (ref['grad'][:, 6:] == 0).all()


def test_infonce_reference_equals_oracle_autograd_on_the_clamp_rows():
    for temperature in lr.NCE_TEMPS:
        p, ref, _ = lr.nce_case_refs(lr.CLAMP_G, lr.CLAMP_DM, temperature, 'distinct', True)
        losses, grad = oracle_pair(p, temperature, lr.WEIGHTS['distinct'])
        for a, b in zip(ref['losses'], losses):
            assert abs(a - b) <= 1e-12 * max(1.0, abs(b))
        for row in range(lr.CLAMP_G):                        # every (row, slot) against its own max: d e = d en / eps
            for slot in range(6):
                assert rel(ref['grad'][row, slot], grad[row, slot]) <= 1e-12, (row, slot)


@pytest.mark.parametrize('clamp', [False, True])
@pytest.mark.parametrize('G,Dm', [(1, 16), (3, 40), (5, 40), (33, 257)])
def test_normsoftmax_reference_equals_oracle_autograd(G, Dm, clamp):
    if clamp and G != lr.CLAMP_G:
        return
    for temperature, eps in lr.NS_NORMS:
        v, t, ref, _ = lr.ns_case_refs(G, Dm, temperature, eps, clamp)
        vr, tr = v.double().requires_grad_(), t.double().requires_grad_()
        loss = om.norm_softmax_loss(vr, tr, temperature=temperature, cos_sim=eps == 1e-8, gather=False)
        (lr.NS_DLOSS * loss).backward()
        assert abs(ref['loss'].item() - loss.item()) <= 1e-12 * max(1.0, abs(loss.item()))
        for got, want in ((ref['dvideo'], vr.grad), (ref['dtext'], tr.grad)):
            for row in range(G):
                assert (got[row] - want[row]).abs().max() <= 1e-12 * max(want[row].abs().max().item(), 1e-3 * float(
                    want[0].abs().max())), row


@pytest.mark.parametrize('G', lr.NS_SIM_G)
def test_sim_mat_reference_equals_oracle_autograd(G):
    x, ref, _ = lr.ns_sim_refs(G)
    xr = x.double().requires_grad_()
    loss = om.norm_softmax_loss(sim_mat=xr)
    (lr.NS_DLOSS * loss).backward()
    assert abs(ref['loss'].item() - loss.item()) <= 1e-12 * max(1.0, abs(loss.item()))
    assert lr.row_stat(ref['dsim'], xr.grad) <= 1e-12


# ------------------------------------------------------------------------------------------------------------ the floor
def test_the_floor_is_a_rounding_distance_from_the_reference():
    """The floor is fp32 arithmetic and nothing else: its distance from fp64 is a few fp32 roundings — four orders below
    the bounds the older tests use (2e-4 on a loss, 2e-3 of the largest gradient element)."""
    for G, Dm in [(3, 40), (17, 300), (96, 768)]:
        p, ref, floor = lr.nce_case_refs(G, Dm, 0.05, 'distinct')
        assert 0 < lr.rms_rel(floor['grad'], ref['grad']) < 2e-6 and lr.row_stat(floor['grad'], ref['grad']) < 2e-5
        assert all(lr.scalar_rel(a, b) < 4e-6 for a, b in zip(floor['losses'], ref['losses']))
    for temperature, eps in lr.NS_NORMS:
        _, _, ref, floor = lr.ns_case_refs(33, 257, temperature, eps)
        # (at T = 0.05 the positives saturate the softmax: the gradient is the small difference 1 - p, an order less exact)
        assert 0 < lr.rms_rel(floor['dvideo'], ref['dvideo']) < 2e-5 and lr.scalar_rel(floor['loss'], ref['loss']) < 4e-6
    half = _lib.half_dtype()
    x, labels = lr.focal_inputs(9, 2050, 2.0, 5)
    ref = lr.focal_ref(x, labels, 2.0, lr.FOCAL_DLOSS)
    floor = lr.focal_ref(x, labels, 2.0, lr.FOCAL_DLOSS, ar=lr.FP32)
    assert 0 < lr.rms_rel(floor['dlogits'], ref['dlogits']) < 2e-6 and lr.vec_rel(floor['lse'], ref['lse']) < 1e-6
    xh = x.to(half)
    ref = lr.focal_ref(xh, labels, 2.0, lr.FOCAL_DLOSS)
    floor = lr.focal_ref(xh, labels, 2.0, lr.FOCAL_DLOSS, ar=lr.FP32, round_to=half)
    u = 2.0 ** -8 if half == torch.bfloat16 else 2.0 ** -11                 # half an ulp of the stored gradient
    assert 0.1 * u < lr.rms_rel(floor['dlogits'], ref['dlogits']) < u
