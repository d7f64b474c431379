"""The reference of the dual-softmax loss (tests/dsl_loss_ref.py) without a GPU: against torch autograd on the plain
formulation, against loss_ref.ns_ref at T = 0, a hand-computed G = 2 case, the hub case, the plan records of the GPU cases
through the host-only clv_dsl_loss_plan, the refusals, the loss class's kwarg and the config, and — for every GPU case — that
the fp64 gradient is not zero and the fp32 floor is close to it, so that no bound of tests/test_dsl_loss_gpu.py is a ratio of
two zeros."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

import dsl_loss_ref as dr
import loss_ref as lr
from loss_ref import FP64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def L():
    from clover_amd import _lib
    return _lib.lib()


def T128():
    return int(L().clv_infonce_large_min_g())


def _close(got, want, tol=1e-10):
    top = want.abs().max().item()
    assert (got - want).abs().max().item() <= tol * max(top, 1e-300), ((got - want).abs().max().item(), top)


@pytest.mark.parametrize('T', dr.DSL_TS + (3.0,))
@pytest.mark.parametrize('G,Dm,hub', [(2, 5, False), (7, 12, False), (7, 12, True), (33, 40, True)])
def test_reference_equals_autograd(G, Dm, hub, T):
    for temperature, eps in lr.NS_NORMS:
        v, t = dr.dsl_inputs(G, Dm, hub)
        ref = dr.dsl_ref(v, t, temperature, eps, T, dr.DSL_DLOSS, FP64)
        ag = dr.dsl_autograd(v, t, temperature, eps, T, dr.DSL_DLOSS)
        assert abs(ref['loss'].item() - ag['loss'].item()) <= 1e-10 * max(1.0, abs(ag['loss'].item()))
        _close(ref['dvideo'], ag['dvideo'])
        _close(ref['dtext'], ag['dtext'])


@pytest.mark.parametrize('G,Dm', [(1, 16), (5, 40), (33, 257)])
def test_without_a_prior_it_is_normsoftmax(G, Dm):
    """T = 0: P = 1 / G, the logits are c / temperature."""
    for temperature, eps in lr.NS_NORMS:
        v, t = dr.dsl_inputs(G, Dm)
        ref = dr.dsl_ref(v, t, temperature, eps, 0.0, dr.DSL_DLOSS, FP64)
        ns = lr.ns_ref(v, t, temperature, eps, dr.DSL_DLOSS, FP64)
        assert abs(ref['loss'].item() - ns['loss'].item()) <= 1e-12 * max(1.0, abs(ns['loss'].item()))
        for k in ('dvideo', 'dtext'):
            if ns[k].abs().max().item() == 0.0:
                assert ref[k].abs().max().item() == 0.0
            else:
                _close(ref[k], ns[k], 1e-11)


def test_two_pairs_by_hand():
    """Unit vectors with c = [[0.6, 0], [0.96, 0.6]]; T = ln 3 / 0.36, so that column 0 (0.6 against 0.96) has the priors
    (1/4, 3/4); G / temperature = 2 / 0.5 = 4.  Every entry is written out with math.exp / math.log."""
    T, temperature = math.log(3) / 0.36, 0.5
    v = torch.tensor([[1.0, 0.0], [0.8, 0.6]], dtype=torch.float64)
    t = torch.tensor([[0.6, 0.8], [0.0, 1.0]], dtype=torch.float64)
    cc = [[0.6, 0.0], [0.96, 0.6]]
    assert torch.allclose(v @ t.t(), torch.tensor(cc, dtype=torch.float64), atol=1e-15)
    e = math.exp
    pr = [[e(T * cc[i][j]) / (e(T * cc[0][j]) + e(T * cc[1][j])) for j in range(2)] for i in range(2)]     # down a column
    pc = [[e(T * cc[i][j]) / (e(T * cc[i][0]) + e(T * cc[i][1])) for j in range(2)] for i in range(2)]     # along a row
    assert abs(pr[0][0] - 0.25) < 1e-12 and abs(pr[1][0] - 0.75) < 1e-12
    a = 2 / temperature
    yr = [[a * cc[i][j] * pr[i][j] for j in range(2)] for i in range(2)]
    yc = [[a * cc[i][j] * pc[i][j] for j in range(2)] for i in range(2)]
    assert abs(yr[0][0] - 0.6) < 1e-12 and abs(yr[1][0] - 2.88) < 1e-12 and yr[0][1] == 0.0 == yc[0][1]
    lse = lambda p, q: math.log(e(p) + e(q))                                       # noqa: E731
    want = (-0.5 * ((yr[0][0] - lse(yr[0][0], yr[0][1])) + (yr[1][1] - lse(yr[1][0], yr[1][1])))
            - 0.5 * ((yc[0][0] - lse(yc[0][0], yc[1][0])) + (yc[1][1] - lse(yc[0][1], yc[1][1]))))
    ref = dr.dsl_ref(v, t, temperature, 1e-8, T, 1.0, FP64)
    assert abs(ref['loss'].item() - want) < 1e-12
    assert torch.allclose(ref['yr'], torch.tensor(yr, dtype=torch.float64), atol=1e-12)
    assert torch.allclose(ref['yc'], torch.tensor(yc, dtype=torch.float64), atol=1e-12)


def test_hub_video_loses_to_the_true_pair_under_the_prior():
    """Video 0 is the mean of all text rows: plain scores put it above the true video of texts 1..3; the text -> video logits of
    the dual-softmax loss (the scores `dual_softmax_scores` ranks by) put the true pair above it, and the loss says so."""
    v, t = dr.hub_pairs()
    plain = dr.dsl_ref(v, t, 0.05, 1e-8, 0.0, 1.0, FP64)
    dsl = dr.dsl_ref(v, t, 0.05, 1e-8, 20.0, 1.0, FP64)
    for j in (1, 2, 3):
        assert plain['yc'][0, j] > plain['yc'][j, j]              # the hub wins text j
        assert dsl['yc'][j, j] > dsl['yc'][0, j]                  # the true pair wins
        assert int(plain['yc'][:, j].argmax()) == 0 and int(dsl['yc'][:, j].argmax()) == j
    # the same matrix through the inference form
    import numpy as np
    from clover_amd.evaluation import dual_softmax_scores
    vn, tn = torch.nn.functional.normalize(v, dim=1), torch.nn.functional.normalize(t, dim=1)
    s = dual_softmax_scores((tn @ vn.t()).numpy(), 20.0)          # [text queries, video gallery]
    assert np.allclose(s.T * (4 / 0.05), dsl['yc'].numpy(), atol=1e-9)
    assert list(s.argmax(1)) == [0, 1, 2, 3]
    assert dsl['loss'].item() < plain['loss'].item()


def _gpu_cases():
    out = []
    for G, Dm, path, _ in dr.DSL_CASES:
        out.append((G, Dm, lr.path_is_large(path, G, T128()), False))
    out += [(T128(), 64, False, False), (33, 257, False, True), (65, 64, True, True)]      # threshold pair, hub cases
    return out


def test_plan_records_of_the_gpu_cases():
    lib = L()
    claims = dr.dsl_claims()
    for G, Dm, path, _ in dr.DSL_CASES:
        large = lr.path_is_large(path, G, T128())
        p = dr.dsl_plan(lib, G, Dm, large)
        assert claims[(G, Dm, int(large))](p), (G, Dm, large)
        # the record of NormSoftmax on embeddings: same launch shapes, same three GEMMs
        q = lr.ns_plan(lib, G, Dm, 0, large)
        assert bytes(p) == bytes(q)
    assert T128() == 128 and lr.path_is_large('auto', 127, T128()) is False and lr.path_is_large('auto', 128, T128()) is True
    from clover_amd import _lib
    p = _lib.ClvLossPlan()
    assert lib.clv_dsl_loss_plan(0, 16, 0, C.byref(p)) != 0 and lib.clv_dsl_loss_plan(4, 0, 0, C.byref(p)) != 0
    assert lib.clv_dsl_loss_plan(4, 16, 0, None) != 0
    # work: NormSoftmax's area and eight vectors of G
    for G, Dm in ((1, 16), (65, 64), (1024, 768)):
        assert lib.clv_dsl_loss_work_floats(G, Dm) == lib.clv_normsoftmax_work_floats(G, Dm) + 8 * G


@pytest.mark.parametrize('case', range(12))
def test_gpu_cases_have_a_gradient_and_a_close_floor(case):
    """Every (case, normalisation, T) of the GPU test: non-zero RMS of the fp64 gradient (the clamp rows apart, as the GPU
    test compares them) and an fp32 floor within 1e-3 of it RMS-relative.  G = 1 is the case the table lists as 'loss and
    gradients 0': there the reference AND the floor must be exactly zero, and the GPU test asks the kernels for zeros."""
    G, Dm, large, hub = _gpu_cases()[case]
    rows = dr.dsl_clamp_rows(G)
    for temperature, eps in lr.NS_NORMS:
        for T in dr.DSL_TS:
            v, t, ref, floor = dr.dsl_case_refs(G, Dm, temperature, eps, T, bool(large), hub)
            assert math.isfinite(ref['loss'].item()) and math.isfinite(floor['loss'].item())
            for name in ('dvideo', 'dtext'):
                assert torch.isfinite(ref[name]).all() and torch.isfinite(floor[name]).all()
                if G == 1:
                    assert not ref[name].any() and not floor[name].any() and ref['loss'].item() == 0.0 == floor['loss'].item()
                    continue
                keep = torch.ones(G, dtype=torch.bool)
                keep[rows[name]] = False
                assert ref[name][keep].pow(2).mean().sqrt().item() > 0.0, (name, temperature, T)
                assert lr.rms_rel(floor[name][keep], ref[name][keep]) < 1e-3, (name, temperature, T)
                for row in rows[name]:
                    assert ref[name][row].abs().max().item() > 0.0
                    assert lr.row_stat(floor[name][row][None], ref[name][row][None]) < 1e-3, (name, row, temperature, T)


def test_gpu_case_count():
    assert len(_gpu_cases()) == 12


def test_refusals():
    from clover_amd import ops
    from clover_amd.evaluation import dual_softmax_scores
    from clover_amd.losses import NormSoftmaxLoss
    import numpy as np
    for bad in (-1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError) as e_eval:
            dual_softmax_scores(np.eye(2), bad)
        with pytest.raises(ValueError) as e_ops:
            ops.norm_softmax_loss(torch.zeros(2, 4), torch.zeros(2, 4), dual_softmax=bad)
        assert str(e_ops.value) == str(e_eval.value)                   # the same message rule
        with pytest.raises(ValueError, match='T must be finite and >= 0'):
            NormSoftmaxLoss(0.05, True, dual_softmax=bad)
    with pytest.raises(ValueError, match='sim_mat together with dual_softmax'):
        ops.norm_softmax_loss(sim_mat=torch.eye(3), dual_softmax=20.0)
    with pytest.raises(ValueError, match='sim_mat together with dual_softmax'):
        NormSoftmaxLoss(0.05, True, dual_softmax=20.0)(sim_mat=torch.eye(3))
    # no CPU fallback: the kernel path refuses host tensors as every op does
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.norm_softmax_loss(torch.zeros(2, 4), torch.zeros(2, 4), dual_softmax=20.0)


def test_loss_class_kwarg_and_config():
    from clover_amd.builder import build_loss
    from clover_amd.runner import Config, EvalHook
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    plain = build_loss(dict(type='NormSoftmaxLoss', cos_sim=True, temperature=0.05))
    assert plain.dual_softmax is None
    loss = build_loss(dict(type='NormSoftmaxLoss', cos_sim=True, temperature=0.05, dual_softmax=20))
    assert loss.dual_softmax == 20.0 and isinstance(loss.dual_softmax, float) and loss.t == 0.05 and loss.equal_batch
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'finetune_retrieval_dsl_train_synthetic.py'))
    base = Config.fromfile(os.path.join(ROOT, 'configs', 'finetune_retrieval_dsl_synthetic.py'))
    assert dict(cfg.model['loss_type']) == dict(type='NormSoftmaxLoss', cos_sim=True, temperature=0.05, dual_softmax=20.0)
    ev = dict(cfg.evaluation)
    assert ev['dual_softmax'] == 20.0 and ev['save_best'] == 'DSL_Recall@1' and ev == dict(base.evaluation)
    model, bmodel = dict(cfg.model), dict(base.model)
    model.pop('loss_type'), bmodel.pop('loss_type')
    assert model == bmodel and cfg.data == base.data and cfg.optimizer == base.optimizer
    assert build_loss(dict(cfg.model['loss_type'])).dual_softmax == 20.0
    assert EvalHook([], **ev).dual_softmax == 20.0
