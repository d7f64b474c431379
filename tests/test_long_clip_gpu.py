"""64-frame clips: the fusion encoder's sequence is 32 x 49 + 32 = 1600 tokens, which ops.seq_attention runs on the own kernels
as four parts of 400 staged tokens (tests/test_seq_parts_gpu.py holds the kernels to their references).  Here the step, the
engine's captured step and the retrieval test loop run at that geometry — VideoSwin-T + BERT-base + 3-layer fusion, 224^2,
32 text tokens, one clip — with every GEMM on the HIP kernels.

There is no CPU-oracle run at 64 frames (minutes of host time), and parity mode stops at 1024 keys (clv_attn_f32_*): the
step-level witness is the unfused GEMM + row-softmax path on the same weights and batch, a second 16-bit estimate of the same
fp32 value.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from test_step_gpu import LOSS_KEYS, LOSS_TOL          # noqa: E402

DEV = 'cuda'
FRAMES, TOKENS = 64, 32
FUSION_TOKENS = FRAMES // 2 * 49 + TOKENS                # 1600


@pytest.fixture(scope='module')
def long_clip():
    """One seeded model (eval mode) and one batch, shared by the tests of this file and never modified."""
    import bench
    import clover_amd
    torch.manual_seed(640)
    m = clover_amd.build_model(bench.model_cfg('T', FRAMES)).eval().to(DEV)
    batch = {k: v.to(DEV) for k, v in bench.synthetic_batch(1, FRAMES, TOKENS, seed=64).items()}
    return m, batch


def seq_lengths_seen(monkeypatch):
    """Record the sequence lengths ops.seq_attention is called with."""
    from clover_amd import ops
    seen, real = [], ops.seq_attention

    def spy(qkv, *a, **kw):
        seen.append(qkv.shape[1])
        return real(qkv, *a, **kw)
    monkeypatch.setattr(ops, 'seq_attention', spy)
    return seen


@pytest.mark.usefixtures('strict_own_gemm')
def test_strict_long_clip_step(long_clip, monkeypatch):
    from clover_amd import ops
    m, batch = long_clip
    assert FUSION_TOKENS == 1600 and 896 < FUSION_TOKENS <= ops.SEQ_FUSED_MAX_KEYS
    seen = seq_lengths_seen(monkeypatch)
    with torch.no_grad():
        lv = m.train_step(batch, None)['log_vars']
    assert FUSION_TOKENS in seen, sorted(set(seen))
    assert len(LOSS_KEYS) == 6
    for k in LOSS_KEYS:
        assert np.isfinite(lv[k]), (k, lv)
    assert not ops.LIBRARY_GEMM_CALLS


def test_own_path_equals_unfused_path_at_the_step(long_clip, monkeypatch):
    """The six losses with the fusion attention on the own four-part kernels and on the unfused library path
    (SEQ_FUSED_MAX_KEYS set back to 896) differ by at most LOSS_TOL."""
    import warnings
    from clover_amd import ops
    m, batch = long_clip
    saved = dict(ops.LIBRARY_GEMM_CALLS)
    with torch.no_grad():
        own = m.train_step(batch, None)['log_vars']
    assert ops.LIBRARY_GEMM_CALLS == saved                       # the own path made no library call
    monkeypatch.setattr(ops, 'SEQ_FUSED_MAX_KEYS', 896)
    try:
        with warnings.catch_warnings(), torch.no_grad():
            warnings.simplefilter('ignore', RuntimeWarning)
            lib = m.train_step(batch, None)['log_vars']
        assert [k for k in ops.LIBRARY_GEMM_CALLS if k[0].startswith('seq_attention') and k[1][2] == FUSION_TOKENS]
    finally:
        ops.LIBRARY_GEMM_CALLS.clear()
        ops.LIBRARY_GEMM_CALLS.update(saved)
    diffs = {k: abs(own[k] - lib[k]) for k in LOSS_KEYS}
    print('64-frame step, own four-part path vs unfused path: loss differences', diffs, {k: own[k] for k in LOSS_KEYS})
    for k in LOSS_KEYS:
        assert diffs[k] <= LOSS_TOL[k], (k, own[k], lib[k])


@pytest.mark.usefixtures('strict_own_gemm')
def test_engine_graph_mode_long_clip():
    """CloverEngine with captured hipGraphs, B = 1, train mode (dropout inside the kernels), three steps: one capture for the
    one geometry, finite losses, no library call — the scratch of the four-part attention is allocated inside the autograd
    function and lives in the graphs' pool."""
    import bench
    import clover_amd
    from clover_amd import ops
    from clover_amd.engine import CloverEngine
    torch.manual_seed(641)
    m = clover_amd.build_model(bench.model_cfg('T', FRAMES)).to(DEV)
    m.train()
    batch = {k: v.to(DEV) for k, v in bench.synthetic_batch(1, FRAMES, TOKENS, seed=65).items()}
    eng = CloverEngine(m, batch, lr=1e-4, weight_decay=0.005, grad_clip=15.0, max_iters=10 ** 6)
    eng.capture(batch)
    assert eng.graph is not None
    for _ in range(3):
        lv = eng.step(batch)['log_vars']
        vals = {k: float(v) for k, v in lv.items()}
        assert all(np.isfinite(v) for v in vals.values()), vals
    torch.cuda.synchronize()
    assert len(eng._captures) == 1
    assert not ops.LIBRARY_GEMM_CALLS
    m.eval()


def test_retrieval_test_loop_long_clip():
    """CloverFinetune(task='retrieval').forward_test at 64 frames (the towers only: a guard for the config)."""
    import bench
    import clover_amd
    pre = bench.model_cfg('T', FRAMES)
    cfg = dict(type='CloverFinetune', freeze_stage=None, separate_test=True, backbone=pre['backbone'],
               freeze_text_backbone=None, text_vocab_size=30522, mm_backbone=pre['mm_backbone'],
               text_backbone=pre['text_backbone'], cls_head=None, task='retrieval', ssl_head=pre['ssl_head'],
               itm_head=None, loss_type=dict(type='NormSoftmaxLoss', cos_sim=True, temperature=0.05),
               train_cfg=dict(aux_info=['token_ids', 'segment_ids', 'input_mask']), test_cfg=dict(feature_extraction=False))
    torch.manual_seed(642)
    m = clover_amd.build_model(cfg).eval().to(DEV)
    B = 2
    batch = {k: v.to(DEV) for k, v in bench.synthetic_batch(B, FRAMES, TOKENS, seed=66).items()}
    with torch.no_grad():
        v, t = m.forward_test(batch['imgs'], token_ids=batch['token_ids'], segment_ids=batch['segment_ids'],
                              input_mask=batch['input_mask'])
    D = pre['ssl_head']['vts_embed_dim']
    assert tuple(v.shape) == (B, D) and tuple(t.shape) == (B, D), (v.shape, t.shape)
    assert torch.isfinite(v).all() and torch.isfinite(t).all()
