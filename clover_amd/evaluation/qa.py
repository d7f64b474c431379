"""Video-QA evaluation: the test loop ``multi_gpu_test_itm_finetune`` (mmaction/core/hooks/my_eval_hook.py:317-380,
selected by ``evaluation.test_fn='use_itm_head_fn'``) and the accuracy metrics of ``VideoDataset.evaluate``
(mmaction/datasets/video_dataset.py:304-343): ``video_qa_mc`` -> ``acc``, ``video_qa_oe`` -> ``overall_acc``, both
argmax accuracy of the per-sample scores against the labels (host numpy, as there)."""
import numpy as np

QA_METRICS = ('video_qa_mc', 'video_qa_oe')


def multi_gpu_test_itm_finetune(model, data_loader):
    """Score a test set with ``forward_test`` (task video_qa / FIB) on every rank and collect the scores and labels on
    all ranks in dataset order.  Each batch carries ``index`` (positions in the test set) and ``label``.  Returns
    dict(result=[N x C or N x num_labels] fp32, label=[N], index=[N]) as numpy arrays; collection is the all-gather of
    the retrieval test (evaluation.retrieval.multi_gpu_test_retrieval)."""
    import torch
    import torch.distributed as dist
    was_training = model.training
    model.eval()
    res, labs, idxs = [], [], []
    with torch.no_grad():
        for data in data_loader:
            data = dict(data)
            idxs.append(data.pop('index').reshape(-1).to(torch.int64))
            labs.append(data.pop('label').reshape(-1).to(torch.int64))
            data.pop('img_metas', None)
            out = model(return_loss=False, **data)
            res.append(out['result'].float())
    model.train(was_training)
    r, lab, ix = torch.cat(res), torch.cat(labs).to(res[0].device), torch.cat(idxs).to(res[0].device)
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        W = dist.get_world_size()
        n = torch.tensor([r.shape[0]], device=r.device)
        ns = [torch.zeros_like(n) for _ in range(W)]
        dist.all_gather(ns, n)
        mx = int(max(x.item() for x in ns))

        def gather(x):
            pad = x.new_zeros((mx,) + tuple(x.shape[1:]))
            pad[:x.shape[0]] = x
            out = [torch.empty_like(pad) for _ in range(W)]
            dist.all_gather(out, pad)
            return torch.cat([o[:int(k.item())] for o, k in zip(out, ns)])
        r, lab, ix = gather(r), gather(lab), gather(ix)
    order = torch.argsort(ix, stable=True)
    ix, r, lab = ix[order], r[order], lab[order]
    keep = torch.ones_like(ix, dtype=torch.bool)
    keep[1:] = ix[1:] != ix[:-1]
    return dict(result=r[keep].cpu().numpy(), label=lab[keep].cpu().numpy(), index=ix[keep].cpu().numpy())


def qa_accuracy(scores, labels):
    """Fraction of samples whose argmax score is the label (video_dataset.py:304-343)."""
    scores = np.asarray(scores)
    labels = np.asarray(labels).reshape(-1)
    if scores.ndim != 2 or scores.shape[0] != labels.shape[0]:
        raise ValueError(f'scores {scores.shape} do not match labels {labels.shape}')
    return float(np.mean(np.argmax(scores, axis=1) == labels)) if len(labels) else 0.0


def evaluate_qa(results, metrics=('video_qa_mc',)):
    """results: dict(result=[N x C], label=[N]) of multi_gpu_test_itm_finetune -> {'acc'} (video_qa_mc) and / or
    {'overall_acc'} (video_qa_oe)."""
    out = {}
    for metric in ([metrics] if isinstance(metrics, str) else metrics):
        if metric == 'video_qa_mc':
            out['acc'] = qa_accuracy(results['result'], results['label'])
        elif metric == 'video_qa_oe':
            out['overall_acc'] = qa_accuracy(results['result'], results['label'])
        else:
            raise KeyError(f'metric {metric} is not supported')
    return out
