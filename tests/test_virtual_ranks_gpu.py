"""CloverEngine(virtual_ranks=k): one optimizer step on k micro-batches with the global batch's negatives.

The step must compute what a k-rank DDP job of the reference computes.  tests/golden/g_dist.npz holds the reference's own
W = 1, 2, 4 DDP runs on one global batch of 4 (six losses, 13 packed gradients each): test_matches_reference_ddp holds the
engine to them, eager and through the hipGraphs; the other tests pin the mechanism (slices, 1/k, recomputation under the
same dropout masks, the optimizer's counters) and the refusals.  `-m gpu` only."""
import numpy as np
import pytest
import torch

import closed_form as cf
import gutil
from test_step_gpu import LOSS_KEYS, LOSS_TOL, grad_tol, rel_packed

pytestmark = pytest.mark.gpu
DEV = 'cuda'
PRETRAIN_KEYS = ('token_ids', 'input_mask', 'mlm_label', 'v_token_mask')


def make_model(cfg=None, train=False):
    import clover_amd
    m = clover_amd.build_model(cfg or cf.tiny_model_cfg())
    sd = {k: v for k, v in cf.cf_state(gutil.manifest()).items() if k in m.state_dict()}
    m.load_state_dict(sd, strict=False)
    m = m.to(DEV)
    return m.train() if train else m.eval()


def split(batch, k):
    n = len(batch['imgs'])
    assert n % k == 0
    B = n // k
    return [{name: v[j * B:(j + 1) * B].to(DEV) for name, v in batch.items()} for j in range(k)]


def engine(model, micro, k, graph=False, **kw):
    from clover_amd.engine import CloverEngine
    kw = dict(dict(lr=1e-4, weight_decay=0.005, grad_clip=15.0, max_iters=10 ** 6), **kw)
    eng = CloverEngine(model, micro[0], virtual_ranks=k, **kw)
    assert eng.first_touch_params == 0 and eng._norm_tables is None      # every producer adds into the slabs
    if graph:
        assert eng.capture(micro[0])
    return eng


def live_graphs(model, micro):
    """The definition, by plain autograd on a model no engine owns: all k encode graphs alive, ONE contrastive_losses on
    the concatenation, the k rank-local losses added, one backward; gradients divided by k -> ({name: grad}, log values)."""
    k = len(micro)
    keys = tuple(getattr(model, 'CLV_ENCODE_KEYS', PRETRAIN_KEYS))
    model.zero_grad(set_to_none=True)
    outs = [model.encode(b['imgs'], **{n: b[n] for n in keys}) for b in micro]
    E = torch.cat([e for e, _ in outs], 0)
    if outs[0][1] is not None:
        local = torch.stack([m.float().reshape(()) for _, m in outs]).sum()
        losses = model.contrastive_losses(None, local, gathered=E)
    else:
        losses = model.contrastive_losses(E, None)
    loss, lv = model._parse_losses(losses)
    loss.backward()
    grads = {n: (p.grad.detach().float() / k if p.grad is not None else None) for n, p in model.named_parameters()}
    return grads, {n: float(v) for n, v in lv.items()}


def compare_with_live_graphs(eng, model, ref_model, micro):
    k = len(micro)
    out = eng.forward_backward(micro)
    ref, ref_lv = live_graphs(ref_model, micro)
    scale = eng.loss_scale * k
    named = dict(model.named_parameters())
    unused = set(eng.unused_names)
    worst = 0.0
    for n, r in ref.items():
        if r is None:
            assert n in unused, n
            continue
        assert n not in unused, n
        err = float((named[n].grad / scale - r).abs().max() / r.abs().max().clamp_min(1e-30))
        worst = max(worst, err)
        assert err <= 1e-4, (n, err)
    assert sorted(n for n, r in ref.items() if r is None) == sorted(unused)
    print('virtual ranks vs live graphs: worst gradient error', k, worst)
    return out, ref_lv


# ----------------------------------------------------------------------------- 1. the reference's own DDP runs
@pytest.mark.parametrize('mode', ['eager', 'graph'])
@pytest.mark.parametrize('k', [2, 4])
def test_matches_reference_ddp(k, mode):
    g = gutil.load('g_dist.npz')
    model = make_model()
    micro = split(cf.cf_batch(4, tag='dist'), k)
    eng = engine(model, micro, k, graph=mode == 'graph')
    out = eng.forward_backward(micro)
    assert out['num_samples'] == 4
    lv = {n: float(out['log_vars'][n]) for n in LOSS_KEYS}
    errs = {n: abs(lv[n] - float(g[f'W{k}.{n}'])) for n in LOSS_KEYS}
    print(f'virtual ranks k = {k} ({mode}) loss errors', errs)
    for n in LOSS_KEYS:
        assert errs[n] <= LOSS_TOL[n], (n, lv[n], float(g[f'W{k}.{n}']))
    named = dict(model.named_parameters())
    scale = eng.loss_scale * k
    pre = f'W{k}.grad.'
    names = [n[len(pre):-4] for n in g.files if n.startswith(pre) and n.endswith('.sub')]
    assert len(names) == 13
    worst = {n: rel_packed(g, pre + n, named[n].grad / scale) for n in names}
    print(f'virtual ranks k = {k} ({mode}) grad rel errors', worst)
    for n, e in worst.items():
        assert e < grad_tol(n), (n, e)
    # teeth: W = k is told from W = 1 (the goldens' norms differ by more than 10 %: the 1/W of the local-slice gather)
    key = 'backbone.patch_embed.proj.weight'
    assert rel_packed(g, 'W1.grad.' + key, named[key].grad / scale) > grad_tol(key)


# ----------------------------------------------------------------------------- 2. slices and 1/k
@pytest.mark.parametrize('k', [2, 3])
def test_equals_live_graphs(k):
    """Both sides run the same kernels and differ in fp32 accumulation order and in store versus add: every parameter
    gradient within 1e-4 of its max — ~100 x fp32 summation noise and ~300 x below the 16-bit tolerances, so a misplaced
    slice or a missing 1/k cannot hide."""
    model, ref_model = make_model(), make_model()
    micro = split(cf.cf_batch(2 * k, tag=f'vr{k}'), k)
    eng = engine(model, micro, k)
    out, ref_lv = compare_with_live_graphs(eng, model, ref_model, micro)
    lv = out['log_vars']
    for n in ('nce_loss', 'rank_t_tm_loss', 'v_nce_loss', 'rank_v_vm_loss'):
        assert abs(float(lv[n]) - ref_lv[n]) <= 1e-5 * max(1.0, abs(ref_lv[n])), (n, float(lv[n]), ref_lv[n])
    assert abs(float(lv['mlm_loss']) - ref_lv['mlm_loss'] / k) <= 1e-5 * max(1.0, ref_lv['mlm_loss'])   # the mean of the k


# ----------------------------------------------------------------------------- 3. recomputation draws the same masks
@pytest.mark.parametrize('mode', ['eager', 'graph'])
def test_recompute_draws_the_same_masks(mode):
    """Train mode, dropout and DropPath on, k = 3 micro-batches holding the SAME samples: what tells their embeddings
    apart is the masks alone.  Every recomputed forward must reproduce its pass-1 embeddings bit for bit (each under its
    own RNG state), the three micro-batches must differ, and the next step must draw new masks."""
    k = 3
    torch.manual_seed(3)
    model = make_model(cf.tiny_model_cfg(drop=0.1), train=True)
    one = split(cf.cf_batch(2, tag='vrmask'), 1)[0]
    micro = [one, {n: v.clone() for n, v in one.items()}, {n: v.clone() for n, v in one.items()}]
    eng = engine(model, micro, k, graph=mode == 'graph')
    eng._vr_keep_recomputed = True
    eng.forward_backward(micro)
    first = [e.clone() for e in eng._vr_emb]
    assert sorted(eng._vr_emb_recomputed) == [0, 1]
    for j in (0, 1):
        assert torch.equal(eng._vr_emb_recomputed[j], first[j]), j
    assert not torch.equal(first[0], first[1]) and not torch.equal(first[1], first[2])
    eng.zero_grads()
    eng.forward_backward(micro)
    for j in range(k):
        assert all(not torch.equal(eng._vr_emb[j], f) for f in first), j
    for j in (0, 1):
        assert torch.equal(eng._vr_emb_recomputed[j], eng._vr_emb[j]), j
    model.eval()


# ----------------------------------------------------------------------------- 4. the optimizer's counters
def test_step_trajectory():
    """Five step() calls, k = 2, a dynamic scaler that starts too high: 2**120 overflows, one division by 2**108 leaves
    2**12, three taken steps grow it back to 2**120, which overflows again.  Scale, Adam's count and step_count follow
    oracle/loss_scaler.py driven by the overflow flags the device reports; a skipped step leaves the weights bit-identical;
    the LR index and step_count advance once per call, not once per micro-batch."""
    from clover_amd import ops
    from oracle.loss_scaler import LossScaler
    k = 2
    micro = split(cf.cf_batch(4, tag='vrtraj'), k)
    kw = dict(init_scale=2.0 ** 120, mode='dynamic', scale_factor=2.0 ** 108, scale_window=3)
    eng = engine(make_model(), micro, k, lr=2e-4, weight_decay=0.0, loss_scale=kw)
    ref = LossScaler(**kw)
    taken = skipped = 0
    for it in range(5):
        assert eng.loss_scale == ref.loss_scale
        p0 = [sg.flat_p.clone() for sg in eng.segments]
        out = eng.step(micro)
        st = ops.optim_state_read(eng.optim_state)
        ref.update_scale(bool(st['skip']))
        assert st['loss_scale'] == ref.loss_scale and st['scale_iter'] == ref.cur_iter, (it, st, ref.state_dict())
        same = all(torch.equal(sg.flat_p, q) for sg, q in zip(eng.segments, p0))
        assert same == bool(st['skip']), (it, st)
        taken += 0 if st['skip'] else 1
        skipped += st['skip']
        assert st['t'] == taken and st['skipped'] == skipped
        assert eng.step_count == it + 1 and eng.lr_iter == it + 1
        assert np.isfinite(float(out['log_vars']['loss']))
        assert all(float(sg.flat_g.abs().max()) == 0.0 for sg in eng.segments)       # cleared for the next k backwards
    print('virtual-rank trajectory: taken', taken, 'skipped', skipped, 'scale', eng.loss_scale)
    assert skipped >= 1 and taken >= 1


# ----------------------------------------------------------------------------- 5. retrieval fine-tuning
def test_retrieval_finetune_virtual_ranks():
    """CloverFinetune(task='retrieval'), k = 2: NormSoftmaxLoss on the 2 B rows.  There is no multi-rank golden of the
    reference for this recognizer, so loss and gradients are held to the live-graphs formulation (test_equals_live_graphs)."""
    k = 2
    model, ref_model = make_model(cf.tiny_finetune_cfg()), make_model(cf.tiny_finetune_cfg())
    batch = cf.cf_batch(4, tag='vrft')
    micro = split({n: batch[n] for n in ('imgs', 'label', 'token_ids', 'segment_ids', 'input_mask')}, k)
    eng = engine(model, micro, k)
    out, ref_lv = compare_with_live_graphs(eng, model, ref_model, micro)
    assert set(out['log_vars']) == {'retrieval_nce_loss', 'loss'}
    got = float(out['log_vars']['loss'])
    assert abs(got - ref_lv['loss']) <= 1e-5 * max(1.0, abs(ref_lv['loss'])), (got, ref_lv['loss'])
    # ... and it is the loss of the global batch, not of a micro-batch
    with torch.no_grad():
        one = ref_model.train_step(micro[0], None)['log_vars']['loss']
    assert abs(got - float(one)) > 1e-3


# ----------------------------------------------------------------------------- 6. the refusals
def test_refusals(monkeypatch):
    import clover_amd
    import qa_cases
    from clover_amd import engine as E
    micro = split(cf.cf_batch(4, tag='vrref'), 2)
    with pytest.raises(ValueError, match='virtual_ranks must be >= 1'):
        E.CloverEngine(make_model(), micro[0], virtual_ranks=0)
    monkeypatch.setattr(E, 'collectives_active', lambda: True)
    with pytest.raises(NotImplementedError, match='data-parallel'):
        E.CloverEngine(make_model(), micro[0], virtual_ranks=2)
    monkeypatch.undo()
    cfg = cf.tiny_model_cfg()
    cfg['mlm_ssl_head']['T']['text_bn'] = True
    with pytest.raises(NotImplementedError, match='BatchNorm1d'):
        E.CloverEngine(clover_amd.build_model(cfg).to(DEV), micro[0], virtual_ranks=2)
    qa = clover_amd.build_model(qa_cases.tiny_qa_cfg('mc')).to(DEV)
    qb = {n: v.to(DEV) for n, v in qa_cases.qa_batch('mc', 2, 'vrqa').items()}
    with pytest.raises(NotImplementedError, match='video_qa / FIB'):
        E.CloverEngine(qa, qb, virtual_ranks=2)
    eng = engine(make_model(), micro, 2)
    with pytest.raises(ValueError, match='sequence of 2 micro-batches, got 3'):
        eng.step(micro + micro[:1])
    with pytest.raises(ValueError, match='sequence of 2 micro-batches, got one batch dict'):
        eng.step(micro[0])
    short = {n: v[:1] for n, v in micro[1].items()}
    with pytest.raises(ValueError, match='another geometry'):
        eng.step([micro[0], short])
    assert eng.step_count == 0                                  # nothing above took a step
    eng.step(micro)
    assert eng.step_count == 1 and eng.adam_steps() == 1
