"""Synthetic test sets with the batch layout of the reference's test pipeline (the dataset side — decoding,
tokenisation, augmentation — is outside this project's scope).  Shared by ``tools/test.py`` and the validation loader of
``tools/train.py --validate``; the batches come from the benchmark's generator (``bench.synthetic_batch``) and
``utils.qa_synthetic.qa_batch``."""
import torch


class SyntheticTestLoader:
    """This rank's shard of a synthetic test set: batches with ``index`` as the reference's test pipeline emits."""

    def __init__(self, pairs, batch, frames, tokens, rank, world, device, seed=4242, qa=None):
        import bench
        from .qa_synthetic import qa_batch
        self.batches = []
        mine = list(range(rank, pairs, world))
        keys = ('imgs', 'token_ids', 'segment_ids', 'input_mask') + (('label',) if qa is not None else ())
        for s in range(0, len(mine), batch):
            idx = mine[s:s + batch]
            b = (qa_batch(len(idx), tokens, frames, seed + idx[0], **qa) if qa is not None
                 else bench.synthetic_batch(len(idx), frames, tokens, seed + idx[0]))
            b = {k: b[k].to(device) for k in keys}
            b['index'] = torch.tensor(idx, device=device)
            self.batches.append(b)

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)
