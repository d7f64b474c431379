"""The video-QA / fill-in-the-blank cases shared by make_goldens_qa.py (which runs the reference on them) and the GPU
tests that read g_qa.npz: tiny-width model configs in the reference's format and closed-form (RNG-free) batches."""
import torch

import closed_form as cf

KINDS = ('mc', 'oe', 'fib')
NUM_CHOICES = 5
NUM_LABELS = 37
L = 16
# gradients recorded per variant (besides every qa_head.* parameter): the last fusion layer, fc_in, one text-encoder and
# one Swin parameter
GRAD_KEYS = ['multimodal_backbone.bert_encoder.layer.1.attention.self.query.weight',
             'multimodal_backbone.bert_encoder.layer.1.output.dense.weight',
             'multimodal_backbone.bert_encoder.layer.1.output.LayerNorm.weight',
             'multimodal_backbone.fc_in.weight', 'multimodal_backbone.fc_in.bias',
             'text_backbone.bert.encoder.layer.1.attention.self.query.weight',
             'backbone.layers.1.blocks.1.attn.qkv.weight']
# (rows, K) of the heads alone at D = 768 (closed-form inputs): K = 1 is QA_MC_head, the others QA_OE_Head
HEAD_CASES = [(1, 1), (80, 1), (5, 908), (333, 1540), (80, 1540), (1, 908)]


def tiny_qa_cfg(kind):
    """CloverFinetune at the tiny widths of closed_form.tiny_finetune_cfg, shaped as finetune_tgif_action.py (mc),
    finetune_tgif_frameqa.py (oe) and finetune_lsmdc_FIB.py (fib)."""
    cfg = cf.tiny_finetune_cfg()
    cfg.update(separate_test=False, ssl_head=None, loss_type=dict(type='CrossEntropyLoss'))
    if kind == 'mc':
        cfg.update(task='video_qa', answer_cls=True, qa_head=dict(type='QA_MC_head', hidden_dim=128, dropout_ratio=0.5))
    elif kind == 'oe':
        cfg.update(task='video_qa', answer_cls=True,
                   qa_head=dict(type='QA_OE_Head', hidden_dim=128, dropout_ratio=0.1, num_labels=NUM_LABELS))
    elif kind == 'fib':
        cfg['mm_backbone'] = dict(cfg['mm_backbone'], use_text_cls=False)
        cfg.update(task='FIB', answer_mask=True,
                   itm_head=dict(type='ITMHead', hidden_dim=128, dropout_ratio=0.5, finetune=True),
                   qa_head=dict(type='QA_OE_Head', hidden_dim=128, dropout_ratio=0.1, num_labels=NUM_LABELS))
    else:
        raise KeyError(kind)
    return cfg


def qa_batch(kind, B, tag):
    """Closed-form batch: clips [B, 1, 3, 4, 112, 112]; captions [B, C, L] = [CLS] ids [SEP] pad (no 103 except the one
    [MASK] per FIB caption); labels in range."""
    C = NUM_CHOICES if kind == 'mc' else 1
    imgs = cf.cf_float(f'{tag}.imgs', (B, 1, 3, 4, 112, 112), 1.7)
    ids = cf.cf_int(f'{tag}.ids', (B, C, L), 5, 1024)
    ids[ids == 103] = 104
    ids[:, :, 0] = 101
    mask = torch.ones(B, C, L, dtype=torch.long)
    for b in range(B):
        for c in range(C):
            npad = (2 * b + c + 3) % (L // 2)
            if npad:
                ids[b, c, L - npad:] = 0
                mask[b, c, L - npad:] = 0
            ids[b, c, L - npad - 1] = 102
            if kind == 'fib':
                ids[b, c, 2 + (b + c) % 3] = 103
    hi = NUM_CHOICES if kind == 'mc' else NUM_LABELS
    label = torch.tensor([(7 * b + 3) % hi for b in range(B)], dtype=torch.long)
    return dict(imgs=imgs, label=label, token_ids=ids, segment_ids=torch.zeros_like(ids), input_mask=mask)
