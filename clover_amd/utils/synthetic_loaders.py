"""Synthetic test sets with the batch layout of the reference's test pipeline (the dataset side — decoding,
tokenisation, augmentation — is outside this project's scope).  Shared by ``tools/test.py`` and the validation loader of
``tools/train.py --validate``; the batches come from the benchmark's generator (``bench.synthetic_batch``) and
``utils.qa_synthetic.qa_batch``."""
import torch


class SyntheticTestLoader:
    """This rank's shard of a synthetic test set: batches with ``index`` as the reference's test pipeline emits.

    ``candidates=C`` (zero-shot multiple choice, ``data.test = dict(is_mc=True)`` there): every video comes with C
    captions, ``token_ids / segment_ids / input_mask`` [B, C, L], and ``label`` [B] in [0, C).
    ``captions=<int | sequence>`` (the many-caption test sets): video i comes with ``captions[i % len]`` captions,
    [B, c, L]; with unequal counts every batch is one video, as the reference's varied test loop assumes.
    ``size`` / ``vocab`` fit these two to a small model: the clips' side length, and token ids folded into [1, vocab)."""

    def __init__(self, pairs, batch, frames, tokens, rank, world, device, seed=4242, qa=None, candidates=None,
                 captions=None, size=224, vocab=None):
        import bench
        from .qa_synthetic import qa_batch
        if sum(x is not None for x in (qa, candidates, captions)) > 1:
            raise ValueError('qa, candidates and captions are three different test sets')
        self.batches = []
        mine = list(range(rank, pairs, world))
        per_video = None
        if candidates is not None:
            per_video = [int(candidates)] * pairs
        elif captions is not None:
            caps = [int(captions)] if isinstance(captions, int) else [int(c) for c in captions]
            per_video = [caps[i % len(caps)] for i in range(pairs)]
            if len(set(per_video)) > 1:
                batch = 1
        if per_video is not None and min(per_video, default=1) < 1:
            raise ValueError('every video needs at least one caption')
        labelled = qa is not None or candidates is not None
        keys = ('imgs', 'token_ids', 'segment_ids', 'input_mask') + (('label',) if labelled else ())
        for s in range(0, len(mine), batch):
            idx = mine[s:s + batch]
            if per_video is not None:
                b = self._many_captions(bench, idx, per_video[idx[0]], frames, tokens, seed, candidates is not None,
                                        size, vocab)
            elif qa is not None:
                b = qa_batch(len(idx), tokens, frames, seed + idx[0], **qa)
            else:
                b = bench.synthetic_batch(len(idx), frames, tokens, seed + idx[0])
            b = {k: b[k].to(device) for k in keys}
            b['index'] = torch.tensor(idx, device=device)
            self.batches.append(b)

    @staticmethod
    def _many_captions(bench, idx, c, frames, tokens, seed, with_label, size, vocab):
        """The clips of ``synthetic_batch(len(idx), ...)`` with c captions each: caption j > 0 of the batch is the caption
        row of the same generator at seed + 7919 j."""
        b = bench.synthetic_batch(len(idx), frames, tokens, seed + idx[0], size=size)
        more = [bench.synthetic_batch(len(idx), 1, tokens, seed + idx[0] + 7919 * j, size=8) for j in range(1, c)]
        for k in ('token_ids', 'segment_ids', 'input_mask'):
            b[k] = torch.cat([b[k]] + [m[k] for m in more], dim=1)
        if vocab is not None:
            ids = b['token_ids']
            b['token_ids'] = torch.where(ids >= vocab, 1 + ids % (vocab - 1), ids)
        if with_label:
            g = torch.Generator().manual_seed(seed + idx[0] + 31)
            b['label'] = torch.randint(0, c, (len(idx),), generator=g)
        return b

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)
