"""Retrieval fine-tuning with the dual-softmax loss through the engine: one step of CloverFinetune(task='retrieval') whose
loss is NormSoftmaxLoss(dual_softmax=20), eager and captured, alone and with virtual_ranks = 2.  Loss and gradients are held
to the live-autograd formulation — the pattern and the bounds of test_virtual_ranks_gpu.py::
test_retrieval_finetune_virtual_ranks, whose helpers are imported: every gradient within 1e-4 of its maximum of plain autograd
on a model no engine owns (same kernels, so the 16-bit backward rounds the same numbers), the loss within 1e-5 relative.
The loss VALUE is held, at the same 1e-5, to the formulation written in plain torch operations on the same embeddings too.
The strict run (no library GEMM) uses the model of configs/finetune_retrieval_dsl_train_synthetic.py: the tiny model's
backbone widths lie outside the HIP GEMM kernels' coverage with or without this loss.  `-m gpu` only."""
import pytest
import torch

import closed_form as cf
from test_virtual_ranks_gpu import DEV, compare_with_live_graphs, engine, make_model, split

pytestmark = pytest.mark.gpu
T_DSL, TEMP = 20.0, 0.05
KEYS = ('imgs', 'label', 'token_ids', 'segment_ids', 'input_mask')


class TorchDualSoftmax(torch.nn.Module):
    """The plain formulation in torch operations (cos_sim normalisation, eps 1e-8)."""

    def forward(self, video_embd, text_embd):
        v, t = video_embd.float(), text_embd.float()
        G = v.shape[0]
        vn = v / v.norm(dim=1, keepdim=True).clamp_min(1e-8)
        tn = t / t.norm(dim=1, keepdim=True).clamp_min(1e-8)
        c = vn @ tn.t()
        yr = (G / TEMP) * c * torch.softmax(T_DSL * c, 0)
        yc = (G / TEMP) * c * torch.softmax(T_DSL * c, 1)
        return -torch.log_softmax(yr, 1).diag().mean() - torch.log_softmax(yc, 0).diag().mean()


def dsl_cfg():
    cfg = cf.tiny_finetune_cfg()
    cfg['loss_type'] = dict(cfg['loss_type'], dual_softmax=T_DSL)
    assert cfg['loss_type']['temperature'] == TEMP and cfg['loss_type']['cos_sim'] is True
    return cfg


def torch_loss(model, micro):
    """The plain formulation on the embeddings of all micro-batches."""
    keys = tuple(model.CLV_ENCODE_KEYS)
    with torch.no_grad():
        emb = torch.cat([model.encode(b['imgs'], **{n: b[n] for n in keys})[0] for b in micro], 0)
        return float(TorchDualSoftmax()(emb[:, 0], emb[:, 1]))


def micro_batches(k, tag):
    batch = cf.cf_batch(4, tag=tag)
    return split({n: batch[n] for n in KEYS}, k)


def check_step(k, graph, tag):
    from clover_amd.engine import CloverEngine
    model, ref_model = make_model(dsl_cfg()), make_model(dsl_cfg())
    assert model.loss_func.dual_softmax == T_DSL == ref_model.loss_func.dual_softmax
    micro = micro_batches(k, tag)
    if k == 1:                                    # (the helper `engine` asserts what holds under virtual ranks only)
        eng = CloverEngine(model, micro[0], lr=1e-4, weight_decay=0.005, grad_clip=15.0, max_iters=10 ** 6)
        if graph:
            assert eng.capture(micro[0])
    else:
        eng = engine(model, micro, k, graph=graph)
    out, ref_lv = compare_with_live_graphs(eng, model, ref_model, micro)       # every gradient within 1e-4 of its maximum
    assert set(out['log_vars']) == {'retrieval_nce_loss', 'loss'}
    got = float(out['log_vars']['loss'])
    assert abs(got - ref_lv['loss']) <= 1e-5 * max(1.0, abs(ref_lv['loss'])), (got, ref_lv['loss'])
    want = torch_loss(ref_model, micro)
    assert abs(got - want) <= 1e-5 * max(1.0, abs(want)), (got, want)
    return got, ref_model, micro


@pytest.mark.parametrize('mode', ['eager', 'graph'])
def test_one_step(mode):
    got, ref_model, micro = check_step(1, mode == 'graph', 'dslft')
    # the prior is in the loss: the plain NormSoftmaxLoss of the same batch is another number
    plain = make_model(cf.tiny_finetune_cfg())
    with torch.no_grad():
        other = float(plain.train_step(micro[0], None)['log_vars']['loss'])
    assert abs(got - other) > 1e-3, (got, other)


@pytest.mark.parametrize('mode', ['eager', 'graph'])
def test_virtual_ranks(mode):
    got, ref_model, micro = check_step(2, mode == 'graph', 'dslvr')
    # ... and it is the loss of the global batch, not of a micro-batch
    with torch.no_grad():
        one = ref_model.train_step(micro[0], None)['log_vars']['loss']
    assert abs(got - float(one)) > 1e-3


@pytest.mark.usefixtures('strict_own_gemm')
def test_own_gemms_only():
    """CLOVER_STRICT_OWN_GEMM=1 (a library GEMM raises; the fixture asserts the call table empty at the end): two optimizer
    steps of the new config's model, virtual_ranks = 2, every loss finite."""
    import math
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    import clover_amd
    from clover_amd import ops
    from clover_amd.engine import CloverEngine
    from clover_amd.runner import Config
    cfg = Config.fromfile(os.path.join(root, 'configs', 'finetune_retrieval_dsl_train_synthetic.py'))
    torch.manual_seed(31)
    model = clover_amd.build_model(cfg.model).to(DEV).eval()
    assert model.loss_func.dual_softmax == 20.0
    micro = split(bench.synthetic_batch(4, 8, 32, seed=13), 2)
    eng = CloverEngine(model, micro[0], virtual_ranks=2, lr=1e-5, weight_decay=0.01, grad_clip=5.0, max_iters=10 ** 6)
    for _ in range(2):
        assert math.isfinite(float(eng.step(micro)['log_vars']['loss']))
    assert not ops.LIBRARY_GEMM_CALLS
