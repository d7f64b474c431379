"""Video-text retrieval metrics of the reference's evaluation stage
(mmaction/core/evaluation/accuracy.py:430-462, ``normalize_fn`` mmaction/utils/numpy_norm.py:5-8).

This is the HOST post-processing the reference's dataset ``evaluate()`` runs in numpy once per epoch on the
embeddings ``forward_test(separate_test=True)`` returned (N x D, N = test-set size, MSRVTT: 1000); it stays host
code here too — the device work is the two encoders that produce the embeddings.

``recall_on_device`` is the same metric for callers that evaluate inside a training job (runner.EvalHook): the ranks
come from ``ops.retrieval_rank`` (csrc/retrieval.hip — no score matrix, no sort) and only they cross to the host.

Zero-shot multiple choice (``acc_for_msrvtt_mc``, accuracy.py:396-427) and the many-caption protocol
(``recall_for_video_text_retrieval_varied``, accuracy.py:465-523, with its test loop my_eval_hook.py:115-215) are here the
same way: a numpy restatement for host results, and ``mc_acc_on_device`` / ``recall_varied_on_device`` on
``ops.retrieval_group_best`` / ``ops.retrieval_rank`` for device results.

Dual-softmax re-scoring at inference (``dual_softmax=T``; NOT in the reference): every score is multiplied by a softmax
prior taken over all queries for its gallery item, ``s' = s * softmax(T * s, axis=0)``, which damps hub videos.  It is an
opt-in that ADDS ``DSL_*`` keys next to the plain ones: ``dual_softmax_scores`` for host results,
``ops.retrieval_rank(..., dual_softmax=T)`` for device results.
"""
import numpy as np


def normalize_fn(x, axis=-1, order=2):
    """Rows scaled to unit L2 norm; all-zero rows are left untouched (numpy_norm.py:5-8)."""
    x = np.asarray(x)
    l2 = np.atleast_1d(np.linalg.norm(x, ord=order, axis=axis))
    l2[l2 == 0] = 1
    return x / np.expand_dims(l2, axis=axis)


def dual_softmax_scores(scores, T):
    """``s'[i][j] = s[i][j] * softmax_i(T * s[i][j])`` for a host score matrix [Nq, Ng]: the softmax runs down the QUERY
    axis (axis 0), the column maximum is subtracted before ``exp``.  Computed in the dtype of ``scores``."""
    s = np.asarray(scores)
    T = float(T)
    if not (T >= 0 and np.isfinite(T)):
        raise ValueError(f'dual_softmax: T must be finite and >= 0 (got {T})')
    x = s * s.dtype.type(T)
    e = np.exp(x - x.max(axis=0, keepdims=True))
    return s * e / e.sum(axis=0, keepdims=True)


def _dsl_ranks(scores, gt, T):
    """Ranks of the ground truth under the re-scored matrix, ties by index (the device path's rule)."""
    order = np.argsort(-dual_softmax_scores(scores, T), axis=1, kind='stable')
    return np.where(order == np.asarray(gt)[:, None])[1]


def _dsl_keys(ind, with_all=False):
    out = _recall_keys(ind, 'DSL_')
    if with_all:
        out['DSL_Recall@all'] = out['DSL_Recall@1'] + out['DSL_Recall@5'] + out['DSL_Recall@10'] - out['DSL_MR']
    return out


def recall_for_video_text_retrieval(video_embd=None, text_embd=None, input_scores=None, use_sim=False, texts=None,
                                    dual_softmax=None):
    """R@1 / R@5 / R@10 (percent), median rank (1-based) and ``Recall@all`` = R1 + R5 + R10 - MR of
    text -> video retrieval; query i's ground truth is video i.  ``use_sim`` is accepted and ignored, as in the
    reference (accuracy.py:438 overwrites it with False); ``texts`` is unused there too.  ``dual_softmax = T`` adds the
    same five keys with the prefix ``DSL_``, from ``dual_softmax_scores(scores, T)``; the plain keys do not change."""
    if input_scores is not None:
        scores = np.asarray(input_scores)
    else:
        scores = np.dot(normalize_fn(_host(text_embd)), normalize_fn(_host(video_embd)).T)
    order = np.argsort(-scores, axis=1)
    gt = np.arange(len(scores))
    ind = np.where(order == gt[:, None])[1]
    metrics = {
        'Recall@1': float(np.sum(ind == 0)) / len(ind) * 100,
        'Recall@5': float(np.sum(ind < 5)) / len(ind) * 100,
        'Recall@10': float(np.sum(ind < 10)) / len(ind) * 100,
        'MR': np.median(ind) + 1,
    }
    metrics['Recall@all'] = metrics['Recall@1'] + metrics['Recall@5'] + metrics['Recall@10'] - metrics['MR']
    if dual_softmax is not None:
        metrics.update(_dsl_keys(_dsl_ranks(scores, gt, dual_softmax), with_all=True))
    return metrics


def recall_on_device(video_embd, text_embd, gt=None, topk=0, dual_softmax=None):
    """``recall_for_video_text_retrieval`` with the scoring on the device: the same five keys, from the ranks
    ``ops.retrieval_rank`` returns; only that [Nq] int32 vector (and the [Nq, topk] indices asked for) crosses to the
    host, the median and the counts stay numpy.  ``video_embd`` fp32 [N, D] is the gallery; ``text_embd`` [Nq, D] the
    queries, or [N, C, D] — C captions per video — which means Nq = N * C queries with ``gt = i // C``.  ``gt`` None:
    query i's ground truth is video i.  Ties rank by index (the stable order); queries with ``gt < 0`` are left out.
    With ``topk`` the result also carries ``'topk'``: int array [Nq, topk], the retrieved video indices per query.
    ``dual_softmax = T`` runs the ranks a second time under the dual-softmax prior (``ops.retrieval_rank(...,
    dual_softmax=T)``: the prior spans all Nq queries of this call) and ADDS ``DSL_Recall@1/5/10``, ``DSL_MR`` and
    ``DSL_Recall@all``, with ``topk`` also ``'dsl_topk'``; every plain key, ``'topk'`` included, stays what it is."""
    import torch
    from .. import ops
    v, t = torch.as_tensor(video_embd), torch.as_tensor(text_embd)
    if t.dim() == 3:
        if gt is not None:
            raise ValueError('text_embd [N, C, D] fixes gt = i // C; pass 2-D queries with an explicit gt')
        caps = t.shape[1]
        t = t.reshape(-1, t.shape[-1])
        gt = torch.arange(t.shape[0], device=t.device, dtype=torch.int32) // caps
    elif gt is not None:
        gt = torch.as_tensor(gt).to(device=t.device, dtype=torch.int32)
    rank, _, tidx, _ = ops.retrieval_rank(t.float(), v.float(), gt=gt, topk=topk)
    ind = rank.cpu().numpy()
    ind = ind[ind >= 0]
    metrics = {
        'Recall@1': float(np.sum(ind == 0)) / len(ind) * 100,
        'Recall@5': float(np.sum(ind < 5)) / len(ind) * 100,
        'Recall@10': float(np.sum(ind < 10)) / len(ind) * 100,
        'MR': np.median(ind) + 1,
    }
    metrics['Recall@all'] = metrics['Recall@1'] + metrics['Recall@5'] + metrics['Recall@10'] - metrics['MR']
    if topk:
        metrics['topk'] = tidx.cpu().numpy()
    if dual_softmax is not None:
        drank, _, didx, _ = ops.retrieval_rank(t.float(), v.float(), gt=gt, topk=topk, dual_softmax=dual_softmax)
        dind = drank.cpu().numpy()
        metrics.update(_dsl_keys(dind[dind >= 0], with_all=True))
        if topk:
            metrics['dsl_topk'] = didx.cpu().numpy()
    return metrics


def sim_matrix(a, b, eps=1e-8):
    """Cosine scores with rows scaled by 1 / max(norm, eps) (accuracy.py:385-394), in the inputs' precision."""
    a, b = np.asarray(a), np.asarray(b)
    a_n = np.maximum(np.linalg.norm(a, axis=1, keepdims=True), eps).astype(a.dtype)
    b_n = np.maximum(np.linalg.norm(b, axis=1, keepdims=True), eps).astype(b.dtype)
    return np.dot(a / a_n, (b / b_n).T)


def _recall_keys(ind, prefix=''):
    return {f'{prefix}Recall@1': float(np.sum(ind == 0)) / len(ind) * 100,
            f'{prefix}Recall@5': float(np.sum(ind < 5)) / len(ind) * 100,
            f'{prefix}Recall@10': float(np.sum(ind < 10)) / len(ind) * 100,
            f'{prefix}MR': np.median(ind) + 1}


def acc_for_msrvtt_mc(video_embd, text_embd, label, use_sim=True):
    """MSRVTT / LSMDC multiple choice (accuracy.py:396-427): ``video_embd`` [N, D], ``text_embd`` [N * C, D] (video i's
    candidates are rows i*C .. i*C + C - 1), ``label`` [N] in [0, C) -> ``{'acc'}``, the float32 mean of
    ``argmax == label``.  The full [N, N * C] matrix, its (b_v, b_v, ans_num) reshape and the diagonal are kept as there
    (:413-418); ``use_sim`` selects ``sim_matrix`` (what ``evaluate`` passes, video_dataset.py:182) over the plain dot.
    The first of equal candidates wins (``argmax``).  The reference's prints and its two ``np.save`` calls are left out."""
    video_embd, text_embd = _host(video_embd), _host(text_embd)
    b_v = video_embd.shape[0]
    text_embd = text_embd.reshape(-1, video_embd.shape[-1])
    scores = sim_matrix(video_embd, text_embd) if use_sim else np.dot(video_embd, text_embd.T)
    ans_num = scores.shape[1] // b_v
    scores = scores.reshape(b_v, b_v, ans_num)
    ans_diag = np.diagonal(scores, axis1=0, axis2=1).T                                # (C, N) -> (N, C)
    ans = np.argmax(ans_diag, axis=-1)
    label = _host_int(label).reshape(-1)
    return {'acc': float((ans == label).astype(np.float32).mean())}


def recall_for_video_text_retrieval_varied(video_embd, text_embd, tid, dual_softmax=None):
    """Text -> video R@1 / R@5 / R@10 (percent) and median rank (1-based) when video i has ``len(tid[i])`` captions
    (accuracy.py:465-523): ``text_embd`` [sum of the lengths, D] holds the captions video by video, every caption's ground
    truth is its video; scores by ``sim_matrix``.  Of ``tid`` only the per-video lengths are used (an int sequence of
    counts is taken as it is).  No ``Recall@all``, as there.  Equal scores rank by video index (a stable sort, which
    is also the device path's rule; the reference's ``np.argsort`` leaves their order open).  ``dual_softmax = T`` adds
    ``DSL_Recall@1/5/10`` and ``DSL_MR`` from ``dual_softmax_scores(scores, T)`` (the prior over all captions)."""
    counts = np.array([t if np.ndim(t) == 0 else len(t) for t in tid], dtype=np.int64)
    scores = sim_matrix(_host(text_embd), _host(video_embd))
    order = np.argsort(-scores, axis=1, kind='stable')
    gt = np.repeat(np.arange(len(counts)), counts)
    ind = np.where(order == gt[:, None])[1]
    out = _recall_keys(ind)
    if dual_softmax is not None:
        out.update(_dsl_keys(_dsl_ranks(scores, gt, dual_softmax)))
    return out


_NO_DSL_MC = ('dual_softmax is not defined for multiple choice (video_qa_mc / mc_acc_on_device): every video scores its own '
              'candidates only, and a prior over candidates that belong to different videos has no meaning')
_NO_DSL_V2T = ('dual_softmax does not cover the V2T_* keys of recall_varied_on_device: video -> text would need the prior '
               'inside clv_retrieval_group_best; ask for v2t without dual_softmax (the V2T_* keys are plain scores)')


def mc_acc_on_device(video_embd, text_embd, label, return_pred=False, dual_softmax=None):
    """``acc_for_msrvtt_mc`` with the scoring on the device: one ``ops.retrieval_group_best`` call in which video i
    looks at the text rows [i*C, (i+1)*C) only (``eps = 1e-8`` as ``sim_matrix``), so of the N x N*C scores the reference
    computes only the N x C it keeps are; ``pred = best_idx - i*C`` [N] is all that crosses to the host.  ``text_embd``
    fp32 [N, C, D] or [N*C, D].  -> ``{'acc'}`` (the float32 mean, as there), with ``return_pred`` also ``'pred'``.
    ``dual_softmax`` is refused: it is not defined here."""
    if dual_softmax is not None:
        raise ValueError(_NO_DSL_MC)
    import torch
    from .. import ops
    v, t = torch.as_tensor(video_embd).float(), torch.as_tensor(text_embd).float()
    N = v.shape[0]
    t = t.reshape(-1, v.shape[-1])
    if t.shape[0] % N:
        raise ValueError(f'{t.shape[0]} candidate captions for {N} videos')
    C = t.shape[0] // N
    lo = torch.arange(N, device=v.device, dtype=torch.int32) * C
    best, _, _ = ops.retrieval_group_best(v, t, lo, lo + C, eps=1e-8)
    pred = (best - lo).cpu().numpy()
    out = {'acc': float((pred == _host_int(label).reshape(-1)).astype(np.float32).mean())}
    if return_pred:
        out['pred'] = pred
    return out


def recall_varied_on_device(video_embd, text_embd, counts, v2t=False, dual_softmax=None):
    """``recall_for_video_text_retrieval_varied`` with the scoring on the device.  ``video_embd`` fp32 [N, D],
    ``text_embd`` [sum(counts), D] video by video, ``counts`` int [N].  Text -> video (the reference's four keys) comes
    from ``ops.retrieval_rank`` with ``gt = repeat_interleave(arange(N), counts)``; rows are normalised as ``normalize_fn``
    there (``sim_matrix`` differs only for rows of norm below 1e-8).

    With ``v2t`` the result also holds ``V2T_Recall@1/5/10`` and ``V2T_MR``: per video the rank, among all texts, of the
    best of its own captions (``ops.retrieval_group_best(video, text, lo, hi, want_rank=True)``, the ranges from
    ``cumsum(counts)``).  That is the usual best-caption protocol of video -> text retrieval (the minimum rank over a
    video's valid descriptions); it has NO counterpart in the reference, whose function scores text -> video only.
    Only the int32 rank vectors cross to the host.

    ``dual_softmax = T`` ADDS ``DSL_Recall@1/5/10`` and ``DSL_MR`` (text -> video under the prior over all captions,
    ``ops.retrieval_rank(..., dual_softmax=T)``); the plain keys stay.  Together with ``v2t`` it is refused."""
    if dual_softmax is not None and v2t:
        raise ValueError(_NO_DSL_V2T)
    import torch
    from .. import ops
    v, t = torch.as_tensor(video_embd).float(), torch.as_tensor(text_embd).float()
    counts = torch.as_tensor(counts).to(device=v.device, dtype=torch.int64).reshape(-1)
    if counts.shape[0] != v.shape[0] or int(counts.sum()) != t.shape[0]:
        raise ValueError(f'counts [{counts.shape[0]}] summing to {int(counts.sum())} for {v.shape[0]} videos and '
                         f'{t.shape[0]} texts')
    gt = torch.repeat_interleave(torch.arange(v.shape[0], device=v.device), counts).to(torch.int32)
    rank, _, _, _ = ops.retrieval_rank(t, v, gt=gt)
    out = _recall_keys(rank.cpu().numpy())
    if dual_softmax is not None:
        drank, _, _, _ = ops.retrieval_rank(t, v, gt=gt, dual_softmax=dual_softmax)
        out.update(_dsl_keys(drank.cpu().numpy()))
    if v2t:
        hi = torch.cumsum(counts, 0)
        _, _, vrank = ops.retrieval_group_best(v, t, hi - counts, hi, want_rank=True)
        ind = vrank.cpu().numpy()
        out.update(_recall_keys(ind[ind >= 0], 'V2T_'))
    return out


def _host_int(x):
    if hasattr(x, 'detach'):
        x = x.detach().cpu().numpy()
    return np.asarray(x)


def _host(x):
    if hasattr(x, 'detach'):
        x = x.detach().float().cpu().numpy()
    return np.asarray(x)


def multi_gpu_test_retrieval(model, data_loader, gpu_collect=True, to_host=True, with_label=False):
    """Embed a test set with ``forward_test(separate_test=True)`` on every rank and collect the embeddings on all
    ranks in dataset order (mmaction/core/hooks/my_eval_hook.py:20-100).  Each batch carries ``index`` (the
    samples' positions in the test set); several clips per sample are averaged, several captions per video are
    grouped, as there (:58-63).  Returns ``dict(video_embd=[N x D], text_embd=[N x ...])`` of numpy arrays, or with
    ``to_host=False`` the same collected, de-duplicated tensors still on the device (for ``recall_on_device``).
    ``with_label`` (multiple choice): the batches' ``label`` [B] travels with the embeddings — ordered and de-duplicated
    like them — into ``results['label']`` (the reference reads it from the metas, video_dataset.py:176).

    Collection is one ``all_gather`` of the stacked per-rank embeddings (+ indices) instead of the reference's
    pickle-through-uint8-tensor exchange; a 1-rank run has nothing to collect."""
    import torch
    import torch.distributed as dist
    was_training = model.training
    model.eval()
    vids, txts, idxs, labels = [], [], [], []
    with torch.no_grad():
        for data in data_loader:
            data = dict(data)
            idxs.append(data.pop('index').reshape(-1).to(torch.int64))
            data.pop('img_metas', None)
            label = data.pop('label', None)
            if with_label:
                if label is None:
                    raise KeyError('with_label: the batch has no label')
                labels.append(label.reshape(-1).to(torch.int64))
            v, t = model(return_loss=False, **data)
            if v.shape[0] > t.shape[0]:                                               # :58-60
                v = v.view(t.shape[0], -1, t.shape[1]).mean(dim=1)
            elif v.shape[0] < t.shape[0]:                                             # :61-63 (multiple choice)
                t = t.view(v.shape[0], -1, t.shape[1])
            vids.append(v.float())
            txts.append(t.float())
    model.train(was_training)
    v, t, ix = torch.cat(vids), torch.cat(txts), torch.cat(idxs).to(vids[0].device)
    lb = torch.cat(labels).to(v.device) if with_label else None
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        W = dist.get_world_size()
        n = torch.tensor([v.shape[0]], device=v.device)
        ns = [torch.zeros_like(n) for _ in range(W)]
        dist.all_gather(ns, n)
        mx = int(max(x.item() for x in ns))

        def gather(x):
            pad = x.new_zeros((mx,) + tuple(x.shape[1:]))
            pad[:x.shape[0]] = x
            out = [torch.empty_like(pad) for _ in range(W)]
            dist.all_gather(out, pad)
            return torch.cat([o[:int(k.item())] for o, k in zip(out, ns)])
        v, t, ix = gather(v), gather(t), gather(ix)
        lb = gather(lb) if with_label else None
    # dataset order; a DistributedSampler pads the last ranks with repeated samples: keep the first of each index
    order = torch.argsort(ix, stable=True)
    ix, v, t = ix[order], v[order], t[order]
    keep = torch.ones_like(ix, dtype=torch.bool)
    keep[1:] = ix[1:] != ix[:-1]
    res = dict(video_embd=v[keep], text_embd=t[keep], index=ix[keep])
    if with_label:
        res['label'] = lb[order][keep]
    return res if not to_host else {k: x.cpu().numpy() for k, x in res.items()}


def multi_gpu_test_retrieval_varied(model, data_loader, to_host=True):
    """The test loop of a set whose videos have several captions each, in unequal numbers (my_eval_hook.py:115-215): every
    batch is ONE video (``index`` [1]) with its c_i captions (``token_ids`` [1, c_i, L]), as the reference's loop assumes
    (:150-164); the clips of the video are averaged (:162-164).  Returns ``video_embd`` [N, D], the flat ``text_embd``
    [sum c_i, D] video by video and ``counts`` [N] (what the reference keeps as one name list per video, :150-152), plus
    ``index`` — numpy arrays, or device tensors with ``to_host=False``.  Collected over the ranks with the padded
    all-gather of ``multi_gpu_test_retrieval`` (texts padded to the longest rank's total), ordered by ``index`` and
    de-duplicated."""
    import torch
    import torch.distributed as dist
    was_training = model.training
    model.eval()
    vids, txts, idxs, cnts = [], [], [], []
    with torch.no_grad():
        for data in data_loader:
            data = dict(data)
            ix = data.pop('index').reshape(-1).to(torch.int64)
            if ix.numel() != 1:
                raise ValueError(f'the varied test loop takes one video per batch (got index {ix.tolist()})')
            data.pop('img_metas', None)
            data.pop('label', None)
            v, t = model(return_loss=False, **data)
            v = v.unsqueeze(0) if v.dim() == 1 else v                                 # :158-159
            t = t.reshape(-1, t.shape[-1])                                            # :160-161, flat instead of [1, c, D]
            if v.shape[0] > 1:                                                        # :162-164
                v = v.mean(dim=0, keepdim=True)
            idxs.append(ix)
            vids.append(v.float())
            txts.append(t.float())
            cnts.append(t.shape[0])
    model.train(was_training)
    dev = vids[0].device
    v, t, ix = torch.cat(vids), torch.cat(txts), torch.cat(idxs).to(dev)
    c = torch.tensor(cnts, device=dev, dtype=torch.int64)
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        W = dist.get_world_size()

        def gather(x):
            n = torch.tensor([x.shape[0]], device=dev)
            ns = [torch.zeros_like(n) for _ in range(W)]
            dist.all_gather(ns, n)
            pad = x.new_zeros((int(max(k.item() for k in ns)),) + tuple(x.shape[1:]))
            pad[:x.shape[0]] = x
            out = [torch.empty_like(pad) for _ in range(W)]
            dist.all_gather(out, pad)
            return torch.cat([o[:int(k.item())] for o, k in zip(out, ns)])
        v, t, ix, c = gather(v), gather(t), gather(ix), gather(c)
    # dataset order, first of each repeated index; the texts follow their videos
    order = torch.argsort(ix, stable=True)
    keep = torch.ones_like(ix, dtype=torch.bool)
    keep[1:] = ix[order][1:] != ix[order][:-1]
    order = order[keep]
    start = torch.cumsum(c, 0) - c
    rows = torch.cat([torch.arange(int(start[i]), int(start[i] + c[i]), device=dev) for i in order.tolist()])
    res = dict(video_embd=v[order], text_embd=t[rows], counts=c[order], index=ix[order])
    return res if not to_host else {k: x.cpu().numpy() for k, x in res.items()}


RETRIEVAL_METRICS = ('recall_for_video_text_retrieval', 'video_qa_mc', 'recall_for_video_text_retrieval_varied')


def evaluate_retrieval(results, metrics=('recall_for_video_text_retrieval',), topk=0, with_pred=False, v2t=False,
                       dual_softmax=None):
    """The embedding-similarity branches of ``VideoDataset.evaluate`` (mmaction/datasets/video_dataset.py:173-182
    ``video_qa_mc``, needs ``results['label']``; :189-195 ``recall_for_video_text_retrieval``; :196-203
    ``recall_for_video_text_retrieval_varied``, needs ``results['counts']``).  Results that hold device tensors (the
    test loops with ``to_host=False``) are scored on the device (``recall_on_device``, which is also what ``topk``
    needs; ``mc_acc_on_device``, which is what ``with_pred`` — the chosen candidate per video as ``'pred'`` — needs;
    ``recall_varied_on_device``, which is what ``v2t`` needs); numpy results take the reference's host path.
    ``dual_softmax = T`` adds the ``DSL_*`` keys of the two recall metrics on either path (with ``topk`` also
    ``'dsl_topk'``); ``video_qa_mc`` and ``v2t`` refuse it."""
    out = {}
    names = [metrics] if isinstance(metrics, str) else list(metrics)
    if dual_softmax is not None and 'video_qa_mc' in names:
        raise ValueError(_NO_DSL_MC)
    if dual_softmax is not None and v2t:
        raise ValueError(_NO_DSL_V2T)
    v = results['video_embd']
    on_device = getattr(v, 'is_cuda', False)
    if (topk or with_pred or v2t) and not on_device:
        raise ValueError('topk, with_pred and v2t need device results (the test loop with to_host=False)')
    for metric in ([metrics] if isinstance(metrics, str) else metrics):
        if metric not in RETRIEVAL_METRICS:
            raise KeyError(f'metric {metric} is not supported')                      # video_dataset.py:163-165
        if metric == 'video_qa_mc':
            if on_device:
                out.update(mc_acc_on_device(v, results['text_embd'], results['label'], return_pred=with_pred))
            else:
                out.update(acc_for_msrvtt_mc(np.stack(list(v)), np.stack(list(results['text_embd'])),
                                             results['label'], use_sim=True))
            continue
        if metric == 'recall_for_video_text_retrieval_varied':
            if on_device:
                out.update(recall_varied_on_device(v, results['text_embd'], results['counts'], v2t=v2t,
                                                   dual_softmax=dual_softmax))
            else:
                out.update(recall_for_video_text_retrieval_varied(np.stack(list(v)), results['text_embd'],
                                                                  results['counts'], dual_softmax=dual_softmax))
            continue
        if on_device:
            out.update(recall_on_device(v, results['text_embd'], topk=topk, dual_softmax=dual_softmax))
            continue
        out.update(recall_for_video_text_retrieval(np.stack(list(results['video_embd'])),
                                                   np.stack(list(results['text_embd'])), dual_softmax=dual_softmax))
    return out
