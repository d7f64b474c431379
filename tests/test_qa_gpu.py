"""GPU tests of the video-QA / fill-in-the-blank path: the csrc/qa.hip kernels against fp32 torch on the same 16-bit
inputs, the choice broadcast of the fusion encoder against expand + cat, the three task variants through the model and
the engine, and tools/train.py + tools/test.py on the synthetic QA configs.  `-m gpu` only."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import closed_form as cf

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _half():
    from clover_amd import _lib
    return _lib.half_dtype()


def _rel(a, b, floor=1e-12):
    """max|a - b| / max|b|; ``floor`` bounds the denominator from below (a gradient that is zero in exact arithmetic, such
    as the multiple-choice score bias: softmax - onehot sums to zero over each sample's candidates)."""
    a, b = a.detach().float(), b.detach().float()
    return float((a - b).abs().max()) / max(float(b.abs().max()), floor)


def _head_params(D, H, K, seed):
    g = torch.Generator().manual_seed(seed)
    w1 = (torch.rand(H, D, generator=g) * 2 - 1) * D ** -0.5
    b1 = (torch.rand(H, generator=g) * 2 - 1) * 0.1
    gm = 1 + (torch.rand(H, generator=g) * 2 - 1) * 0.1
    bt = (torch.rand(H, generator=g) * 2 - 1) * 0.1
    w2 = (torch.rand(K, H, generator=g) * 2 - 1) * H ** -0.5
    b2 = (torch.rand(K, generator=g) * 2 - 1) * 0.1
    return [t.to(DEV).requires_grad_() for t in (w1, b1, gm, bt, w2, b2)]


def _torch_head(x, params, eps=1e-5):
    w1, b1, gm, bt, w2, b2 = params
    z = x @ w1.t() + b1
    y = F.layer_norm(z, (z.shape[-1],), gm, bt, eps)
    return F.gelu(y) @ w2.t() + b2


def _rows_problem(N, S, D, seed):
    g = torch.Generator().manual_seed(seed)
    h = (torch.randn(N, S, D, generator=g)).to(DEV, _half()).requires_grad_()
    pos = torch.randint(0, S, (N,), generator=g)
    rows = (torch.arange(N) * S + pos).to(DEV, torch.int32)
    return h, rows


def test_answer_rows_cls_and_mask():
    from clover_amd import ops
    ids = torch.randint(1000, 2000, (6, 12), device=DEV)
    ids[0, 3] = 103
    ids[1, 0] = 103
    ids[1, 7] = 103            # two: the first counts, count 2
    ids[3, 11] = 103
    ids[4, 5] = 103
    ids[5, 2] = 103
    rows, counts = ops.qa_answer_rows(ids, 20, 8, answer_mask=True)
    n = torch.arange(6, device=DEV) * 20 + 8
    assert rows.tolist() == (n + torch.tensor([3, 0, 0, 11, 5, 2], device=DEV)).tolist()
    assert counts.tolist() == [1, 2, 0, 1, 1, 1]
    rows, counts = ops.qa_answer_rows(ids, 20, 7, answer_mask=False)
    assert rows.tolist() == (n - 1).tolist() and counts.tolist() == [1] * 6


@pytest.mark.parametrize('D,H,K,M', [(768, 384, 1540, 80), (768, 384, 908, 333), (768, 256, 1, 80), (128, 64, 37, 5),
                                     (128, 256, 1, 1), (768, 384, 1000, 16), (128, 64, 37, 4096)])
def test_qa_head_matches_fp32_torch(D, H, K, M):
    from clover_amd import ops
    S = 3
    h, rows = _rows_problem(M, S, D, seed=D + H + K + M)
    params = _head_params(D, H, K, seed=K)
    logits = ops.qa_head(h, rows, *params, drop_p=0.0)
    ref_params = [p.detach().clone().requires_grad_() for p in params]
    hr = h.detach().float().clone().requires_grad_()
    ref = _torch_head(hr.view(-1, D)[rows.long()], ref_params)
    assert _rel(logits, ref) <= 2e-4
    dl = torch.randn(M, K, device=DEV)
    logits.backward(dl)
    ref.backward(dl)
    dh_ref = hr.grad.view(-1, D)
    dh = h.grad.view(-1, D).float()
    assert _rel(dh[rows.long()], dh_ref[rows.long()]) <= 5e-3        # 16-bit storage of d h
    mask = torch.ones(dh.shape[0], dtype=torch.bool, device=DEV)
    mask[rows.long()] = False
    assert float(dh[mask].abs().max()) == 0.0                      # untouched rows stay zero
    for p, r in zip(params, ref_params):
        assert _rel(p.grad, r.grad) <= 1e-3, (p.shape, _rel(p.grad, r.grad))


@pytest.mark.parametrize('C,B', [(5, 16), (5, 1), (3, 7)])
def test_mc_head_with_softmax_ce_over_candidates(C, B):
    from clover_amd import ops
    D, H = 768, 256
    M = B * C
    h, rows = _rows_problem(M, 2, D, seed=C * 100 + B)
    params = _head_params(D, H, 1, seed=7)
    labels = torch.randint(0, C, (B,), device=DEV)
    loss = ops.qa_head(h, rows, *params, drop_p=0.0, labels=labels, num_choices=C)
    ref_params = [p.detach().clone().requires_grad_() for p in params]
    hr = h.detach().float().clone().requires_grad_()
    ref = F.cross_entropy(_torch_head(hr.view(-1, D)[rows.long()], ref_params).view(-1, C), labels)
    assert abs(float(loss) - float(ref)) <= 1e-4
    (loss * 3.0).backward()
    (ref * 3.0).backward()
    assert _rel(h.grad.view(-1, D)[rows.long()], hr.grad.view(-1, D)[rows.long()]) <= 5e-3
    for p, r in zip(params, ref_params):
        assert _rel(p.grad, r.grad, floor=1e-3) <= 1e-3


def test_dropout_keep_rate_scale_same_mask_and_seed_determinism():
    """W1 = I (D = H = 128): the input gradient at the answer rows is dz * mask / (1 - p), so its zeros ARE the dropped
    inputs.  The forward with that mask applied by hand must equal the kernel's forward (same mask in both passes)."""
    from clover_amd import ops
    D = H = 128
    K, M, p = 37, 512, 0.5
    h, rows = _rows_problem(M, 2, D, seed=3)
    params = _head_params(D, H, K, seed=11)
    with torch.no_grad():
        params[0].copy_(torch.eye(D, device=DEV))
    torch.manual_seed(0)
    ops.dropout_seeds_end(DEV)
    seed = ops.next_dropout_seed(DEV)
    y = ops._QAHead.apply(h, rows, *params, seed, p, 1e-5, None, 1)
    y2 = ops._QAHead.apply(h.detach(), rows, *[q.detach() for q in params], seed, p, 1e-5, None, 1)
    assert torch.equal(y.detach(), y2)                                  # same seed -> same mask
    dl = torch.randn(M, K, device=DEV)
    y.backward(dl)
    dxr = h.grad.view(-1, D)[rows.long()].float()
    ref_params = [q.detach().clone().requires_grad_() for q in params]
    xr = h.detach().view(-1, D)[rows.long()].float()
    ref0 = _torch_head(xr, ref_params)
    ref0.backward(dl)
    del ref0
    keep = dxr != 0
    rate = float(keep.float().mean())
    assert abs(rate - (1 - p)) < 0.02, rate
    m = keep.float() / (1 - p)
    ref_params = [q.detach().clone().requires_grad_() for q in params]
    xin = (xr * m).requires_grad_()
    ref = _torch_head(xin, ref_params)
    assert _rel(y, ref) <= 2e-4
    ref.backward(dl)
    assert _rel(dxr, xin.grad * m) <= 5e-3                            # 1/(1-p) scale, same mask
    for q, r in zip(params, ref_params):
        assert _rel(q.grad, r.grad) <= 1e-3
    seed2 = ops.next_dropout_seed(DEV)
    y3 = ops._QAHead.apply(h.detach(), rows, *[q.detach() for q in params], seed2, p, 1e-5, None, 1)
    assert not torch.equal(y3, y2)


@pytest.mark.parametrize('N,S,nH,hd', [(4, 396, 12, 64), (2, 61, 2, 64), (3, 1040, 12, 64)])
def test_attention_probs_mean(N, S, nH, hd):
    from clover_amd import ops
    C = nH * hd
    qkv = (torch.randn(N, S, 3 * C, device=DEV) * 0.5).to(_half())
    m = torch.ones(N, S, device=DEV)
    m[:, S - S // 5:] = 0
    km = (1.0 - m) * -10000.0
    out = ops.attn_probs_mean(qkv, km, nH)
    q, k, _ = qkv.float().view(N, S, 3, nH, hd).unbind(2)
    sc = torch.einsum('nqhd,nkhd->nhqk', q, k) * hd ** -0.5 + km[:, None, None, :]
    ref = sc.softmax(-1).mean(1)
    assert float((out - ref).abs().max()) <= 1e-5


# ----------------------------------------------------------------------------------------------- model level
def _tiny_qa_cfg(kind):
    cfg = cf.tiny_finetune_cfg()
    cfg.update(separate_test=False, ssl_head=None, loss_type=dict(type='CrossEntropyLoss'))
    if kind == 'mc':
        cfg.update(task='video_qa', answer_cls=True, qa_head=dict(type='QA_MC_head', hidden_dim=128, dropout_ratio=0.5))
    elif kind == 'oe':
        cfg.update(task='video_qa', answer_cls=True,
                   qa_head=dict(type='QA_OE_Head', hidden_dim=128, dropout_ratio=0.1, num_labels=37))
    else:
        cfg['mm_backbone'] = dict(cfg['mm_backbone'], use_text_cls=False)
        cfg.update(task='FIB', answer_mask=True, itm_head=dict(type='ITMHead', hidden_dim=128, dropout_ratio=0.5),
                   qa_head=dict(type='QA_OE_Head', hidden_dim=128, dropout_ratio=0.1, num_labels=37))
    return cfg


def _tiny_qa_batch(kind, B=2, seed=5):
    from clover_amd.utils.qa_synthetic import qa_batch
    spec = dict(mc=dict(num_choices=5), oe=dict(num_labels=37), fib=dict(num_labels=37, fib=True))[kind]
    b = qa_batch(B, 16, 4, seed, size=112, **spec)
    b['token_ids'] = b['token_ids'] % 1024                     # tiny vocabulary
    b['token_ids'][b['token_ids'] == 103 % 1024] = 7
    if kind == 'fib':
        b['token_ids'][:, :, 2] = 103
    b['token_ids'][:, :, 0] = 101
    return {k: v.to(DEV) for k, v in b.items()}


def _tiny_model(kind):
    import clover_amd
    torch.manual_seed(0)
    return clover_amd.build_model(_tiny_qa_cfg(kind)).to(DEV)


def _reference_step(model, batch, kind):
    """The reference's forward_train (:87-123) on the model's own modules, in torch where the QA path has its kernels:
    expand the video tokens over the candidates, fusion encoder, answer row by torch.where / the CLS row, the head chain
    in fp32, CrossEntropyLoss."""
    imgs = batch['imgs'].reshape((-1,) + batch['imgs'].shape[2:])
    ids = batch['token_ids'].reshape(-1, batch['token_ids'].shape[-1])
    mask = batch['input_mask'].reshape(-1, batch['input_mask'].shape[-1])
    B = batch['token_ids'].shape[0]
    text = model.text_backbone(ids, mask)['last_hidden_state']
    vis = model.backbone.forward_tokens(imgs)
    _, T, hh, ww, Dv = vis.shape
    vis = vis.reshape(B, T, hh * ww, Dv)
    C = ids.shape[0] // B
    if C > 1:
        vis = vis.unsqueeze(1).expand(-1, C, -1, -1, -1).flatten(0, 1)
    out = model.multimodal_backbone(visual_token=vis, text_input_mask=mask, text_input_embeds=text)
    if kind == 'fib':
        x = out['t_last_hidden_state'][torch.where(ids == 103)]
    else:
        x = out['t_last_hidden_state'][:, 0]
    seq = model.qa_head.classifier
    p = [seq[1].weight, seq[1].bias, seq[2].weight, seq[2].bias, seq[4].weight, seq[4].bias]
    logits = _torch_head(x.float(), p).view(-1, C if C > 1 else p[4].shape[0])
    return F.cross_entropy(logits, batch['label'].view(-1))


@pytest.mark.parametrize('kind', ['mc', 'oe', 'fib'])
def test_qa_model_step_matches_the_reference_formulation(kind):
    """eval mode (dropout off): loss and gradients of the fused path vs the reference's formulation on the same modules
    (expand + cat, torch.where answer rows, torch head)."""
    m = _tiny_model(kind).eval()
    b = _tiny_qa_batch(kind)
    out = m.train_step(b)
    out['loss'].backward()
    got = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    loss = float(out['log_vars']['qa_loss'])
    m.zero_grad(set_to_none=True)
    ref = _reference_step(m, b, kind)
    from clover_amd import _lib
    (ref * _lib.LOSS_SCALE).backward()
    assert abs(loss - float(ref)) <= 5e-3, (loss, float(ref))
    refg = {n: p.grad.detach().clone() / _lib.LOSS_SCALE for n, p in m.named_parameters() if p.grad is not None}
    # (the reference backward runs outside the root-scale node: the unscale hooks divide by 1, so it is divided here)
    checked = 0
    for n in refg:
        # (key biases are left out: their exact gradient is zero — the softmax over keys ignores a per-query constant)
        if (n.startswith('qa_head.') or n.startswith('multimodal_backbone.fc_in') or 'layer.1.' in n) \
                and not n.endswith('key.bias'):
            assert n in got, n
            # (floor: the multiple-choice score bias has an exactly-zero gradient as well — softmax - onehot sums to 0)
            assert _rel(got[n], refg[n], floor=1e-5) <= 5e-2, (n, _rel(got[n], refg[n], floor=1e-5))
            checked += 1
    assert checked >= 8
    unused = [n for n, p in m.named_parameters() if p.requires_grad and n not in got]
    if kind == 'fib':
        assert any(n.startswith('itm_head.') for n in unused)
    assert not any(n.startswith('qa_head.') for n in unused)


@pytest.mark.parametrize('kind', ['mc', 'oe', 'fib'])
def test_qa_forward_test_result_and_attention(kind):
    m = _tiny_model(kind).eval()
    b = _tiny_qa_batch(kind, B=3, seed=9)
    with torch.no_grad():
        out = m(return_loss=False, imgs=b['imgs'], token_ids=b['token_ids'], input_mask=b['input_mask'],
                segment_ids=b['segment_ids'])
    B = 3
    C = 5 if kind == 'mc' else 37
    assert out['result'].shape == (B, C) and out['result'].dtype == torch.float32
    Ntot = B * (5 if kind == 'mc' else 1)
    att = out['attention']
    assert att.shape[0] == Ntot and att.shape[1] == att.shape[2]
    assert float((att.sum(-1) - 1).abs().max()) <= 1e-4
    # the padded caption tokens get no probability
    L = b['token_ids'].shape[-1]
    km = b['input_mask'].reshape(Ntot, L) == 0
    assert float(att[:, :, -L:][km[:, None, :].expand(-1, att.shape[1], -1)].abs().max()) <= 1e-6


def test_choice_broadcast_equals_expand_and_cat():
    m = _tiny_model('mc').eval()
    fus = m.multimodal_backbone
    B, C, L, T, S = 2, 3, 16, 2, 196
    g = torch.Generator().manual_seed(1)
    vis = torch.randn(B, T, S, 96, generator=g).to(DEV, _half()).requires_grad_()
    text = torch.randn(B * C, L, 128, generator=g).to(DEV, _half()).requires_grad_()
    mask = torch.ones(B * C, L, dtype=torch.long, device=DEV)
    mask[:, -3:] = 0
    out = fus(visual_token=vis, text_input_mask=mask, text_input_embeds=text, num_choices=C)['last_hidden_state']
    vis2 = vis.detach().clone().requires_grad_()
    text2 = text.detach().clone().requires_grad_()
    ref = fus(visual_token=vis2.unsqueeze(1).expand(-1, C, -1, -1, -1).flatten(0, 1), text_input_mask=mask,
              text_input_embeds=text2)['last_hidden_state']
    assert _rel(out, ref) <= 1e-2
    d = torch.randn_like(out.float()).to(out.dtype)
    out.backward(d)
    ref.backward(d)
    assert _rel(vis.grad, vis2.grad) <= 2e-2
    assert _rel(text.grad, text2.grad) <= 2e-2


def test_fib_eager_rejects_zero_or_two_masks():
    m = _tiny_model('fib').train()
    b = _tiny_qa_batch('fib')
    for bad in ('zero', 'two'):
        bb = {k: v.clone() for k, v in b.items()}
        if bad == 'zero':
            bb['token_ids'][0, 0, 2] = 7
        else:
            bb['token_ids'][1, 0, 5] = 103
        with pytest.raises(ValueError):
            m.train_step(bb)


@pytest.mark.parametrize('kind', ['mc', 'oe', 'fib'])
def test_qa_engine_graph_equals_eager(kind):
    """eval mode (no dropout): the replayed hipGraph step follows the eager trajectory."""
    from clover_amd.engine import CloverEngine
    b = _tiny_qa_batch(kind, B=2, seed=21)
    traj = {}
    for mode in ('eager', 'graph'):
        m = _tiny_model(kind).eval()
        eng = CloverEngine(m, b, lr=2e-4, weight_decay=0.0, grad_clip=15.0, max_iters=10 ** 9)
        if kind == 'fib':
            assert any(n.startswith('itm_head.') for n in eng.unused_names)
        eng.step(b)
        run = b
        if mode == 'graph':
            assert eng.capture(b)
            run = eng.input_buffers()
        traj[mode] = [float(eng.step(run)['log_vars']['qa_loss']) for _ in range(3)]
    # the first replay and the eager step see the same weights: equal to 1e-5.  Later steps follow AdamW updates whose
    # early moments normalise gradients of ~1e-8 (atomic-order rounding then flips whole lr-sized steps): 1e-3
    assert abs(traj['eager'][0] - traj['graph'][0]) <= 1e-5 * max(1.0, abs(traj['eager'][0])), traj
    for a, g in zip(traj['eager'], traj['graph']):
        assert abs(a - g) <= 1e-3 * max(1.0, abs(a)), traj


@pytest.mark.parametrize('kind', ['mc', 'fib'])
def test_qa_engine_train_mode_replay_draws_fresh_dropout(kind):
    """train mode: the captured step takes its dropout seeds from the pool refreshed inside the graph, so replays draw new
    masks — a finite trajectory that is not constant on a fixed batch, and the head's parameters move."""
    from clover_amd.engine import CloverEngine
    b = _tiny_qa_batch(kind, B=2, seed=23)
    m = _tiny_model(kind).train()
    eng = CloverEngine(m, b, lr=0.0, weight_decay=0.0, grad_clip=15.0, max_iters=10 ** 9)
    eng.step(b)
    assert eng.capture(b)
    run = eng.input_buffers()
    losses = [float(eng.step(run)['log_vars']['qa_loss']) for _ in range(4)]
    assert all(np.isfinite(v) for v in losses), losses
    assert len(set(losses)) > 1, losses          # lr = 0: only the dropout masks change between replays


def test_parity_mode_refuses_the_qa_head():
    from clover_amd import ops, parity
    h, rows = _rows_problem(4, 2, 128, seed=1)
    params = _head_params(128, 64, 37, seed=1)
    with parity.mode(), pytest.raises(NotImplementedError):
        ops.qa_head(h, rows, *params)


# ----------------------------------------------------------------------------------------------- tools
TOOLS_CASES = {'qa_mc': ("{'num_choices': 5}", 100, 'video_qa_mc', 'acc:'),
               'qa_oe': ("{'num_labels': 1540}", 40, 'video_qa_oe', 'overall_acc:'),
               'fib': ("{'num_labels': 908, 'fib': True}", 200, 'video_qa_oe', 'overall_acc:')}


@pytest.fixture(scope='module')
def pretrain_ckpt(tmp_path_factory):
    import bench
    import clover_amd
    pre = clover_amd.build_model(bench.model_cfg('B', 8))
    ck = tmp_path_factory.mktemp('pre') / 'epoch_1.pth'
    torch.save({'state_dict': pre.state_dict(), 'meta': {}}, ck)
    return ck


@pytest.mark.usefixtures('strict_own_gemm')
@pytest.mark.parametrize('name', list(TOOLS_CASES))
def test_train_then_test_config(name, tmp_path, pretrain_ckpt):
    """tools/train.py on each synthetic QA config (two short epochs, from a pre-training checkpoint), then tools/test.py
    on the checkpoint it wrote: prints the config's metric."""
    qa, tokens, metric, printed = TOOLS_CASES[name]
    cfg = os.path.join(ROOT, 'configs', f'finetune_{name}_synthetic.py')
    wd = tmp_path / 'work'
    opts = ['videos_per_gpu=2', "log_config={'interval': 1}",
            f"data.synthetic=[{{'length': 2, 'frames': 8, 'tokens': {tokens}, 'qa': {qa}}}]",
            f"data.synthetic_test={{'pairs': 4, 'frames': 8, 'tokens': {tokens}, 'qa': {qa}}}"]
    env = dict(os.environ, CLOVER_STRICT_OWN_GEMM='1')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'train.py'), cfg, '--launcher', 'none',
                        '--load-from', str(pretrain_ckpt), '--work_dir', str(wd), '--cfg-options', *opts],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'qa_loss' in r.stdout
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'test.py'), cfg, str(wd / 'epoch_2.pth'),
                        '--eval', metric, '--out', str(tmp_path / 'res.json'), '--cfg-options', *opts],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert printed in r.stdout, r.stdout[-2000:]


def test_bf16_build_runs_the_qa_head_in_a_child_process():
    code = ('import sys; sys.path[:0] = ["tests", "tests/golden"]; import torch, test_qa_gpu as t; '
            't.test_qa_head_matches_fp32_torch(768, 384, 908, 80); t.test_mc_head_with_softmax_ce_over_candidates(5, 4); '
            'print("bf16 ok")')
    env = dict(os.environ, CLOVER_HALF='bf16')
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'bf16 ok' in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
