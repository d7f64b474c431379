"""Parity mode (fp32 storage + fp32 arithmetic on the HIP kernels) over every fine-tuning task: the video-QA /
fill-in-the-blank step and forward_test and the retrieval fine-tuning step against the numbers the REFERENCE itself
produced (tests/golden/g_qa.npz, g_finetune.npz), at the tolerances parity mode holds for pre-training
(tests/test_parity_gpu.py): losses 1e-3 (north star), gradients and feature maps 1e-4 of the tensor's max; and the fp32
instantiations of the QA kernels (csrc/qa.hip) alone against fp64 restatements at 1e-5 forward / 2e-5 backward.
Every measured error is printed (DESIGN.md §2 quotes the maxima).  `-m gpu` only."""
import ctypes
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import closed_form as cf
import gutil
import qa_cases as Q

pytestmark = pytest.mark.gpu
DEV = 'cuda'
G = gutil.load('g_qa.npz')
PARITY_TOL = 1e-3          # losses: the north-star number
MAP_TOL = 1e-4             # gradients and feature maps against the reference, of the tensor's max
K_FWD, K_BWD = 1e-5, 2e-5  # an fp32 kernel alone against an fp64 restatement, of the tensor's max
ZERO_GRAD_ABS = 5e-7       # a gradient that is zero in exact arithmetic (the multiple-choice score bias: softmax - onehot
#                            sums to zero per sample): absolute, what tests/test_qa_golden_gpu.py enforces (5e-2 x 1e-5)
MC_BIAS = 'qa_head.mc_vqa_classifier.4.bias'
QA_MAXSUB = 1024           # make_goldens_qa.pack


def sub(t):
    a = t.detach().float().cpu().double().numpy().reshape(-1)
    return a[::max(1, a.size // QA_MAXSUB)][:QA_MAXSUB]


def err_scale(a, ref):
    """(max|a - ref|, max|ref|) in float64."""
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    ref = ref.detach().double().cpu().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref, dtype=np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return float(np.abs(a - ref).max()), float(np.abs(ref).max())


def within(a, ref, tol, what, log=None):
    e, s = err_scale(a, ref)
    if log is not None:
        log[what] = e / s if s > 0 else e
    assert e <= tol * s, (what, e, s, e / max(s, 1e-300))


# ------------------------------------------------------------------------------- 1. QA / FIB against the reference
_QA_MODELS = {}


def qa_model(kind):
    """As tests/test_qa_golden_gpu.py::model, built (once per kind) under parity mode."""
    import clover_amd
    from clover_amd import parity
    if kind not in _QA_MODELS:
        with parity.mode():
            m = clover_amd.build_model(Q.tiny_qa_cfg(kind))
            manifest = json.loads(str(G[f'{kind}.manifest']))
            missing, unexpected = m.load_state_dict(cf.cf_state(manifest), strict=False)
            assert not unexpected and all('relative_position_index' in k for k in missing), (missing, unexpected)
            _QA_MODELS[kind] = m.to(DEV).eval()
    return _QA_MODELS[kind]


@pytest.mark.parametrize('B', [2, 4])
@pytest.mark.parametrize('kind', Q.KINDS)
def test_parity_qa_step_and_forward_test_vs_reference(kind, B):
    from clover_amd import parity
    m = qa_model(kind)
    m.zero_grad(set_to_none=True)
    batch = {k: v.to(DEV) for k, v in Q.qa_batch(kind, B, f'qa.{kind}.B{B}').items()}
    pre = f'{kind}.B{B}.'
    with parity.mode():
        out = m.train_step(batch)
        out['loss'].backward()
        with torch.no_grad():
            res = m(return_loss=False, imgs=batch['imgs'], token_ids=batch['token_ids'],
                    segment_ids=batch['segment_ids'], input_mask=batch['input_mask'])
    loss_err = abs(float(out['log_vars']['qa_loss']) - float(G[pre + 'qa_loss']))
    named = dict(m.named_parameters())
    keys = [k[len(pre + 'grad.'):-len('.sub')] for k in G.files if k.startswith(pre + 'grad.') and k.endswith('.sub')]
    assert len(keys) in (13, 14), keys
    worst, bad = {}, []
    for k in keys:
        assert named[k].grad is not None, k
        assert named[k].grad.dtype == torch.float32
        e, s = err_scale(sub(named[k].grad), G[pre + f'grad.{k}.sub'])
        if k == MC_BIAS:
            worst[k + ' (abs)'] = e
            ok = e <= ZERO_GRAD_ABS
        else:
            worst[k] = e / s
            ok = e <= MAP_TOL * s
        if not ok:
            bad.append((k, e, s))
    ref = G[pre + 'result']
    got = res['result'].cpu().numpy()
    re_, rs = err_scale(got, ref)
    ae, as_ = err_scale(sub(res['attention']), G[pre + 'attention.sub'])
    print(f'parity qa {kind} B={B}: |qa_loss - ref| {loss_err:.2e}; result {re_ / rs:.2e}; attention {ae / as_:.2e}; '
          f'worst grad {max(v for k, v in worst.items() if not k.endswith("(abs)")):.2e}', worst)
    assert loss_err <= PARITY_TOL
    assert not bad, bad
    assert sum(p.grad is None for p in named.values()) == int(G[pre + 'n_unused'])
    assert got.shape == ref.shape and got.dtype == np.float32
    assert re_ <= MAP_TOL * rs, (re_, rs)
    assert ae <= MAP_TOL * as_, (ae, as_)
    m.zero_grad(set_to_none=True)


# ------------------------------------------------------------------------------- 2. heads alone at D = 768
@pytest.mark.parametrize('M,K', Q.HEAD_CASES)
def test_parity_heads_alone_at_bert_base_width(M, K):
    from clover_amd import parity
    from clover_amd.builder import build_head
    head = build_head(dict(type='QA_MC_head', hidden_dim=768) if K == 1
                      else dict(type='QA_OE_Head', hidden_dim=768, num_labels=K))
    head.load_state_dict(cf.cf_state({k: list(v.shape) for k, v in head.state_dict().items()}))
    head = head.to(DEV).eval()
    tag = f'head.M{M}.K{K}'
    x = cf.cf_float(tag + '.x', (M, 768), 1.0).to(DEV).requires_grad_()
    log = {}
    with parity.mode():
        y = head(x)
        y.backward(cf.cf_float(tag + '.dy', tuple(y.shape), 1.0).to(DEV))
    assert y.dtype == torch.float32 and x.grad.dtype == torch.float32
    try:
        within(sub(y), G[tag + '.y.sub'], MAP_TOL, 'y', log)
        within(sub(x.grad), G[tag + '.dx.sub'], MAP_TOL, 'dx', log)
        for n, p in head.named_parameters():
            within(sub(p.grad), G[f'{tag}.grad.{n}.sub'], MAP_TOL, n, log)
    finally:
        print(f'parity head M={M} K={K}', {k: f'{v:.1e}' for k, v in log.items()})


# ------------------------------------------------------------------------------- 3. the head kernel at its edges
def head_params(D, H, K, seed):
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g) * 2 - 1       # noqa: E731
    ps = (u(H, D) * D ** -0.5, u(H) * 0.1, 1 + u(H) * 0.1, u(H) * 0.1, u(K, H) * H ** -0.5, u(K) * 0.1)
    return [t.to(DEV).requires_grad_() for t in ps]


def head_f64(x, params, eps=1e-5):
    w1, b1, gm, bt, w2, b2 = params
    z = x @ w1.t() + b1
    return F.gelu(F.layer_norm(z, (z.shape[-1],), gm, bt, eps)) @ w2.t() + b2


def rows_problem(N, S, D, seed):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(N, S, D, generator=g).to(DEV).requires_grad_()
    rows = (torch.arange(N) * S + torch.randint(0, S, (N,), generator=g)).to(DEV, torch.int32)
    return h, rows


PARAM_NAMES = ('dW1', 'db1', 'dgamma', 'dbeta', 'dW2', 'db2')


def f64_twin(h, params):
    return h.detach().double().requires_grad_(), [p.detach().double().requires_grad_() for p in params]


# D not a multiple of the 16-wide chunk nor of 256; a partial second row block (17 rows); both limits of
# clv_qa_head_supported (D = 1024, H = 512)
@pytest.mark.parametrize('N,S,D,H,K', [(4, 2, 40, 64, 37), (17, 3, 300, 320, 1), (1, 1, 1024, 512, 5)])
def test_head_kernel_f32_vs_fp64(N, S, D, H, K):
    from clover_amd import ops, parity
    assert ops._lib.lib().clv_qa_head_supported(D, H, K)
    h, rows = rows_problem(N, S, D, seed=N + S + D + H + K)
    params = head_params(D, H, K, seed=K)
    dl = torch.randn(N, K, generator=torch.Generator().manual_seed(5)).to(DEV)
    with parity.mode():
        logits = ops.qa_head(h, rows, *params, drop_p=0.0)
        logits.backward(dl)
    h64, p64 = f64_twin(h, params)
    ref = head_f64(h64.view(-1, D)[rows.long()], p64)
    ref.backward(dl.double())
    log = {}
    try:
        assert logits.dtype == torch.float32 and h.grad.dtype == torch.float32
        within(logits, ref, K_FWD, 'logits', log)
        within(h.grad, h64.grad, K_BWD, 'dh', log)
        off = torch.ones(N * S, dtype=torch.bool, device=DEV)
        off[rows.long()] = False
        assert float(h.grad.view(-1, D)[off].abs().sum()) == 0.0          # exactly zero off the answer rows
        for n, p, r in zip(PARAM_NAMES, params, p64):
            within(p.grad, r.grad, K_BWD, n, log)
    finally:
        print(f'head f32 N={N} S={S} D={D} H={H} K={K}', {k: f'{v:.1e}' for k, v in log.items()})


@pytest.mark.parametrize('C,B', [(1, 4), (5, 3)])
def test_head_kernel_f32_folded_cross_entropy_vs_fp64(C, B):
    """K = 1 with ``labels``: the softmax-CE over each sample's C scores rides in the head.  The loss is a difference of
    logits (lse - logit[label]), so its error is bounded in units of the logits' max; with C = 1 loss and gradients are
    exactly zero on both sides.  d b2 is zero in exact arithmetic (see ZERO_GRAD_ABS): absolute bound."""
    from clover_amd import ops, parity
    D, H, S = 300, 320, 3
    M = B * C
    h, rows = rows_problem(M, S, D, seed=100 * C + B)
    params = head_params(D, H, 1, seed=7)
    labels = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(C)).to(DEV)
    with parity.mode():
        loss = ops.qa_head(h, rows, *params, drop_p=0.0, labels=labels, num_choices=C)
        loss.backward()
    h64, p64 = f64_twin(h, params)
    lg = head_f64(h64.view(-1, D)[rows.long()], p64)
    ref = F.cross_entropy(lg.view(-1, C), labels)
    ref.backward()
    log = dict(loss=abs(float(loss.detach()) - float(ref.detach())))
    try:
        assert log['loss'] <= K_FWD * float(lg.detach().abs().max())
        within(h.grad, h64.grad, K_BWD, 'dh', log)
        for n, p, r in zip(PARAM_NAMES, params, p64):
            if n == 'db2':
                log[n + ' (abs)'] = err_scale(p.grad, r.grad)[0]
                assert log[n + ' (abs)'] <= ZERO_GRAD_ABS
            else:
                within(p.grad, r.grad, K_BWD, n, log)
    finally:
        print(f'head f32 CE C={C} B={B}', {k: f'{v:.1e}' for k, v in log.items()})


# ------------------------------------------------------------------------------- 4. dispatch contract
def test_dispatch_is_by_mode_and_dtype():
    from clover_amd import ops, parity
    half = ops.BF16
    h32, rows = rows_problem(4, 2, 128, seed=1)
    params = head_params(128, 64, 37, seed=1)
    qkv32 = torch.randn(2, 6, 3 * 2 * 8, device=DEV)
    vis32, text32 = torch.randn(2, 3, 16, device=DEV), torch.randn(4, 2, 16, device=DEV)
    with parity.mode():
        with pytest.raises(NotImplementedError):
            ops.qa_head(h32.detach().to(half), rows, *params)
        with pytest.raises(NotImplementedError):
            ops.attn_probs_mean(qkv32.to(half), None, 2)
        with pytest.raises(TypeError):
            ops.choice_assemble(vis32.to(half), text32.to(half), 2)
        with pytest.raises(TypeError):
            ops.choice_assemble(vis32, text32.to(half), 2)
        y = ops.qa_head(h32, rows, *params)
        y.sum().backward()
        assert y.dtype == torch.float32 and h32.grad.dtype == torch.float32
        assert ops.attn_probs_mean(qkv32, None, 2).dtype == torch.float32
        feat = ops.choice_assemble(vis32, text32, 2)
        assert feat.dtype == torch.float32
        dv, dt = ops.choice_assemble_bwd(feat, (2, 2, 3, 2, 16))
        assert dv.dtype == torch.float32 and dt.dtype == torch.float32
    # outside parity mode fp32 activations keep raising, 16-bit ones run
    with pytest.raises(NotImplementedError):
        ops.attn_probs_mean(qkv32, None, 2)
    with pytest.raises(NotImplementedError):
        ops.qa_head(h32.detach(), rows, *params)
    with pytest.raises(TypeError):
        ops.choice_assemble(vis32, text32, 2)
    assert ops.attn_probs_mean(qkv32.to(half), None, 2).dtype == torch.float32
    assert ops.choice_assemble(vis32.to(half), text32.to(half), 2).dtype == half


# ------------------------------------------------------------------------------- 5. choice assembly in fp32
@pytest.mark.parametrize('B,C,n_vis,L,D', [(2, 5, 3, 2, 12), (1, 1, 1, 1, 4), (3, 2, 7, 5, 768)])
def test_choice_assemble_f32(B, C, n_vis, L, D):
    from clover_amd import ops, parity
    g = torch.Generator().manual_seed(B * 1000 + D)
    vis = torch.randn(B, n_vis, D, generator=g).to(DEV)
    text = torch.randn(B * C, L, D, generator=g).to(DEV)
    d = torch.randn(B * C, n_vis + L, D, generator=g).to(DEV)
    with parity.mode():
        feat = ops.choice_assemble(vis, text, C)
        dv, dt = ops.choice_assemble_bwd(d, (B, C, n_vis, L, D))
    assert feat.dtype == torch.float32
    assert torch.equal(feat, torch.cat([vis.repeat_interleave(C, 0), text], 1))
    ref = d.double()[:, :n_vis].reshape(B, C, n_vis, D).sum(1)
    e, s = err_scale(dv, ref)
    print(f'choice assemble f32 {(B, C, n_vis, L, D)}: d visual {e / s:.1e}')
    assert dv.dtype == torch.float32 and e <= 1e-6 * s
    assert torch.equal(dt, d[:, n_vis:])


def test_choice_assemble_f32_needs_whole_16_byte_groups():
    from clover_amd import _lib
    B, C, n_vis, L, D = 2, 3, 2, 2, 10
    vis, text = torch.zeros(B, n_vis, D, device=DEV), torch.zeros(B * C, L, D, device=DEV)
    feat = torch.zeros(B * C, n_vis + L, D, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())        # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L_ = _lib.lib()
    assert _lib.ERRORS[-2].startswith('CLV_ERR_UNSUPPORTED')
    assert L_.clv_qa_choice_assemble_f32(p(vis), p(text), p(feat), B, C, n_vis, L, D, st) == -2
    assert L_.clv_qa_choice_assemble_f32_bwd(p(feat), p(vis), p(text), B, C, n_vis, L, D, st) == -2
    torch.cuda.synchronize()
    assert float(feat.abs().sum()) == 0.0          # nothing was launched


# ------------------------------------------------------------------------------- 6. attention map in fp32
@pytest.mark.parametrize('N,S,nH,hd,masked', [(2, 5, 2, 2, True), (1, 300, 3, 64, True), (3, 212, 12, 64, True),
                                             (2, 5, 2, 2, False)])
def test_attention_probs_mean_f32(N, S, nH, hd, masked):
    from clover_amd import ops, parity
    Cd = nH * hd
    qkv = torch.randn(N, S, 3 * Cd, generator=torch.Generator().manual_seed(S + nH)).to(DEV) * 0.5
    km = None
    if masked:                                   # ragged padding: sequence n keeps S - (n + 1) * max(1, S // 5) keys
        keep = torch.ones(N, S, device=DEV)
        for n in range(N):
            keep[n, S - (n + 1) * max(1, S // 5):] = 0
        km = (1.0 - keep) * -10000.0
    with parity.mode():
        out = ops.attn_probs_mean(qkv, km, nH)
    q, k, _ = qkv.double().view(N, S, 3, nH, hd).unbind(2)
    sc = torch.einsum('nqhd,nkhd->nhqk', q, k) * hd ** -0.5
    if masked:
        sc = sc + km.double()[:, None, None, :]
    ref = sc.softmax(-1).mean(1)
    e, s = err_scale(out, ref)
    rowsum = float((out.double().sum(-1) - 1).abs().max())
    print(f'attention map f32 {(N, S, nH, hd)} masked={masked}: {e / s:.1e} of max, |row sum - 1| {rowsum:.1e}')
    assert out.dtype == torch.float32 and tuple(out.shape) == (N, S, S)
    assert e <= K_FWD * s
    assert rowsum <= 1e-5
    if masked:
        assert float(out[(keep == 0)[:, None, :].expand(-1, S, -1)].abs().max()) == 0.0


# ------------------------------------------------------------------------------- 7. many-candidate fusion, BERT-base width
def test_parity_many_candidate_fusion_equals_expansion():
    """num_choices = 5 (fc_in / norm once per video, clv_qa_choice_assemble_f32, its backward's sum over the candidates)
    against the reference's own formulation on the same module: tokens expanded over the candidates by torch,
    num_choices = 1 (fc_in / norm per candidate)."""
    from clover_amd import parity
    from clover_amd.builder import build_backbone
    torch.manual_seed(1234)
    B, C, T, S, L = 2, 5, 2, 9, 8
    fus = build_backbone(dict(type='CrossModalTransformerFromPretrained', pretrained_model='bert-base-uncased',
                              num_hidden_layers=3, img_in_size=1024, hidden_size=768, num_frames=T, spacial_tokens=S,
                              token_types=2, layer_norm_eps=1e-12)).to(DEV).eval()
    g = torch.Generator().manual_seed(7)
    vis = torch.randn(B, T, S, 1024, generator=g).to(DEV).requires_grad_()
    text = torch.randn(B * C, L, 768, generator=g).to(DEV).requires_grad_()
    mask = torch.ones(B * C, L, dtype=torch.long, device=DEV)
    for i in range(B * C):                      # ragged: caption i ends in i % 4 padded positions
        if i % 4:
            mask[i, L - i % 4:] = 0
    n_tot = T * S + 1 + L
    d = torch.randn(B * C, n_tot, 768, generator=g).to(DEV)
    with parity.mode():
        out = fus(visual_token=vis, text_input_mask=mask, text_input_embeds=text, num_choices=C, return_attention=True)
        assert out['last_hidden_state'].dtype == torch.float32
        out['last_hidden_state'].backward(d)
        got = (out['last_hidden_state'].detach(), out['attention'], vis.grad, text.grad, fus.fc_in.weight.grad.clone())
        fus.zero_grad(set_to_none=True)
        vis2, text2 = vis.detach().clone().requires_grad_(), text.detach().clone().requires_grad_()
        ref = fus(visual_token=vis2.unsqueeze(1).expand(-1, C, -1, -1, -1).flatten(0, 1), text_input_mask=mask,
                  text_input_embeds=text2, return_attention=True)
        ref['last_hidden_state'].backward(d)
    want = (ref['last_hidden_state'].detach(), ref['attention'], vis2.grad, text2.grad, fus.fc_in.weight.grad)
    log = {}
    try:
        for n, a, b, tol in zip(('last_hidden_state', 'attention', 'd visual', 'd text', 'd fc_in.weight'), got, want,
                                (K_FWD, K_FWD, K_BWD, K_BWD, K_BWD)):
            within(a, b, tol, n, log)
    finally:
        print('many-candidate fusion (parity) vs expansion', {k: f'{v:.1e}' for k, v in log.items()})


# ------------------------------------------------------------------------------- 8. retrieval fine-tuning
FT_AUX = ['token_ids', 'segment_ids', 'input_mask']


@pytest.fixture(scope='module')
def ft_model():
    """As tests/test_step_gpu.py::ft_model."""
    import clover_amd
    m = clover_amd.build_model(cf.tiny_finetune_cfg())
    sd = {k: v for k, v in cf.cf_state(gutil.manifest()).items() if k in m.state_dict()}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert all('relative_position_index' in k for k in missing) and not unexpected
    return m.to(DEV).eval()


@pytest.mark.parametrize('B', [2, 4])
def test_parity_retrieval_finetune_step_vs_reference(ft_model, B):
    from clover_amd import parity
    g = gutil.load('g_finetune.npz')
    batch = {k: v.to(DEV) for k, v in cf.cf_batch(B, tag=f'ft{B}').items()}
    ft_model.zero_grad(set_to_none=True)
    with parity.mode():
        out = ft_model.train_step({k: batch[k] for k in ['imgs', 'label'] + FT_AUX}, None)
        out['loss'].backward()
    lv = out['log_vars']
    assert set(lv) == {'retrieval_nce_loss', 'loss'}
    loss_err = abs(lv['loss'] - float(g[f'train.B{B}.loss']))
    named = dict(ft_model.named_parameters())
    worst = {}
    pre = f'train.B{B}.grad.'
    for k in [n[len(pre):-4] for n in g.files if n.startswith(pre) and n.endswith('.sub')]:
        s, stats = gutil.packed(named[k].grad)
        assert g[pre + k + '.stats'][2] == stats[2]
        e, sc = err_scale(s, g[pre + k + '.sub'])
        worst[k] = e / sc
    print(f'parity retrieval fine-tuning B={B}: |loss - ref| {loss_err:.2e}, grad rel errors', worst)
    assert loss_err <= PARITY_TOL
    assert len(worst) == 7
    for k, e in worst.items():
        assert e <= MAP_TOL, (k, e)
    assert sum(p.grad is None for p in named.values()) == int(g[f'train.B{B}.n_unused'])
    ft_model.zero_grad(set_to_none=True)


def test_parity_retrieval_separate_test_vs_reference(ft_model):
    """forward_test(separate_test=True): one clip per sample and two (the clip average), the recall metrics of the
    embeddings, and the caption encoder on its side stream against the same pass on the main stream."""
    from clover_amd import parity
    from clover_amd.evaluation import recall_for_video_text_retrieval
    g = gutil.load('g_finetune.npz')
    batch = {k: v.to(DEV) for k, v in cf.cf_batch(4, tag='ft_test').items()}
    with parity.mode(), torch.no_grad():
        v, t = ft_model(batch['imgs'], None, return_loss=False, **{k: batch[k] for k in FT_AUX})
        imgs2 = batch['imgs'].reshape((2, 2) + tuple(batch['imgs'].shape[2:]))
        v2, t2 = ft_model.forward_test(imgs2, **{k: batch[k][:2] for k in FT_AUX})
        ft_model.overlap_text = False
        try:
            v3, t3 = ft_model(batch['imgs'], None, return_loss=False, **{k: batch[k] for k in FT_AUX})
        finally:
            del ft_model.overlap_text
    log = {}
    try:
        assert v.dtype == torch.float32 and t.dtype == torch.float32
        within(v, g['test.clips1.visual_emb'], MAP_TOL, 'clips1.visual_emb', log)
        within(t, g['test.clips1.text_emb'], MAP_TOL, 'clips1.text_emb', log)
        within(v2, g['test.clips2.visual_emb'], MAP_TOL, 'clips2.visual_emb', log)
        within(t2, g['test.clips2.text_emb'], MAP_TOL, 'clips2.text_emb', log)
    finally:
        print('parity retrieval forward_test', {k: f'{x:.1e}' for k, x in log.items()})
    assert recall_for_video_text_retrieval(v, t) == recall_for_video_text_retrieval(g['test.clips1.visual_emb'],
                                                                                  g['test.clips1.text_emb'])
    assert torch.equal(v, v3) and torch.equal(t, t3)          # the same kernels on the same data, on another stream
