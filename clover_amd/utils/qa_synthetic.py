"""Synthetic video-QA / fill-in-the-blank batches with the layout of the reference's collated QA batch
(configs/_base_/datasets_local/tgif_action_mc.py, tgif_frame_oe.py, lsmdc_FIB.py pipelines): N(0, 1) clips, captions
``[B, C, L]`` as ``[CLS] ids [SEP] pad`` (C candidates for multiple choice, C = 1 otherwise), labels in range, and in
fill-in-the-blank exactly one ``[MASK]`` (id 103) per caption.  The real datasets and tokenisers are out of scope."""
import torch

CLS_ID, SEP_ID, MASK_ID = 101, 102, 103


def qa_batch(B, L, frames, seed, num_choices=1, num_labels=None, fib=False, size=224):
    """-> dict(imgs [B, 1, 3, frames, size, size], label [B], token_ids / segment_ids / input_mask [B, C, L]).
    Multiple choice (num_labels None): label in [0, num_choices); otherwise label in [0, num_labels)."""
    if num_labels is None and num_choices < 2:
        raise ValueError('multiple choice needs num_choices >= 2; open-ended / FIB need num_labels')
    if L < 4:
        raise ValueError('captions need room for [CLS] x [SEP]')
    C = num_choices if num_labels is None else 1
    g = torch.Generator().manual_seed(seed)
    imgs = torch.randn(B, 1, 3, frames, size, size, generator=g)
    ids = torch.zeros(B, C, L, dtype=torch.long)
    for b in range(B):
        for c in range(C):
            n = int(torch.randint(2, L - 1, (1,), generator=g))
            ids[b, c, 0] = CLS_ID
            ids[b, c, 1:1 + n] = torch.randint(1000, 30000, (n,), generator=g)
            ids[b, c, 1 + n] = SEP_ID
            if fib:
                ids[b, c, int(torch.randint(1, 1 + n, (1,), generator=g))] = MASK_ID
    hi = num_choices if num_labels is None else num_labels
    label = torch.randint(0, hi, (B,), generator=g)
    return dict(imgs=imgs, label=label, token_ids=ids, segment_ids=torch.zeros_like(ids), input_mask=(ids != 0).long())

