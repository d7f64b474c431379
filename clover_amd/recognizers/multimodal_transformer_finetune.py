"""``CloverFinetune`` — downstream fine-tuning on the pre-trained encoders
(mmaction/models/recognizers/multimodal_transformer_finetune.py:9-215), same constructor kwargs and ``losses`` keys.

``task='retrieval'`` (:83-86 train, :146-148 test): the two uni-modal encoders of the pre-training step (the HIP Swin +
BERT paths) feeding the contrastive projections and ``NormSoftmaxLoss``.

``task='video_qa'`` / ``'FIB'`` (:87-123 train, :157-193 test): video tokens + caption hidden states through the fusion
encoder, the answer row of every sequence (the text CLS row with ``answer_cls``, the ``[MASK]`` row with
``answer_mask``) into the QA head, CrossEntropyLoss as ``qa_loss``.  Multiple choice (a head without ``num_labels``) runs
C = token_ids.shape[1] candidate captions per video; the fusion encoder's per-token input layers run once per video
(``num_choices``).  The answer rows come from a device row table (ops.qa_answer_rows) and the head reads them in place
(ops.qa_head), so the step has no data-dependent shape and is captured by the engine like the pre-training step; the CE
is rank-local and rides in ``encode``.  The branches of the reference that call ``itm_head`` (answer_cls + itm_head, no
qa_head) are refused at construction: no shipped config runs them.
"""
import torch

from .. import ops
from ..builder import RECOGNIZERS, build_backbone, build_head, build_loss
from .base import BaseRecognizer


@RECOGNIZERS.register_module()
class CloverFinetune(BaseRecognizer):
    def __init__(self, mm_backbone, text_backbone=None, freeze_text_backbone=None, loss_type=None, task=None,
                 ssl_head=None, itm_head=None, answer_mask=False, answer_cls=False, qa_head=None,
                 from_scratch=False, text_vocab_size=30522, separate_test=False, **kwargs):
        super().__init__(**kwargs)
        # the reference builds the fusion encoder for every task (:28) although retrieval never runs it; keeping
        # it keeps pre-training checkpoints loadable with strict=True
        self.multimodal_backbone = build_backbone(mm_backbone)
        self.text_backbone = build_backbone(text_backbone)
        self.text_vocab_size = text_vocab_size
        self.from_scratch = from_scratch
        self.separate_test = separate_test
        self.task = task
        if task == 'retrieval':
            self.ssl_head = build_head(ssl_head)
            self.loss_func = build_loss(loss_type)
        elif task in ('video_qa', 'FIB'):
            if qa_head is None:
                raise NotImplementedError(f'task={task!r} without qa_head: the reference then scores with itm_head '
                                          '(:115-121, :185-187), a branch no shipped config uses and this path refuses')
            if not answer_mask and not answer_cls:
                raise NotImplementedError(f'task={task!r} with neither answer_mask nor answer_cls: the reference then runs '
                                          'itm_head on the fusion CLS row (:110-112), a branch no shipped config uses')
            if answer_cls and not answer_mask and itm_head is not None:
                raise NotImplementedError('answer_cls with itm_head: the reference feeds the ITM head output into qa_head '
                                          '(:108-109), a branch no shipped config uses and this path refuses')
            self.answer_mask = answer_mask
            self.answer_cls = answer_cls
            self.itm_head = build_head(itm_head) if itm_head is not None else None     # built, never called (FIB)
            self.qa_head = build_head(qa_head)
            self.loss_func = build_loss(loss_type)
            self.loss_type = loss_type['type']
            if self.loss_type != 'CrossEntropyLoss':
                raise NotImplementedError(f'task={task!r} with loss_type {self.loss_type}: the QA configs use '
                                          'CrossEntropyLoss')
        else:
            raise NotImplementedError('must have head to do downstream finetuning')       # :45-46
        self.fp16_enabled = False

    def extract_visual_feat(self, imgs):
        return self.backbone(imgs)

    # ---- the engine's split of the step (same contract as CloverPretrain): ``encode`` is everything that touches
    # only this rank's samples (captured as hipGraphs), ``contrastive_losses`` holds the all-gather + the loss
    EMB_NAMES = ('visual_emb', 'text_emb')

    @property
    def CLV_ENCODE_KEYS(self):
        return ('token_ids', 'input_mask', 'label') if self.task in ('video_qa', 'FIB') else ('token_ids', 'input_mask')

    @property
    def is_qa(self):
        return self.task in ('video_qa', 'FIB')

    # ---- video QA / FIB
    def _qa_fusion(self, imgs, token_ids, input_mask, video_cut=None, text_cut=None, test=False):
        """-> (fusion output h [N, Ltot, D], answer rows int32 [N], mask counts int32 [N], C, attention or None)."""
        if token_ids.dim() != 3:
            raise ValueError('video_qa / FIB take captions as [B, C, L] (C = 1 for open-ended and FIB; the reference '
                             'flattens them with token_ids.reshape, :67-70)')
        if self.training and imgs.is_cuda:
            ops.dropout_seeds_begin(imgs.device)
        imgs = imgs.reshape((-1,) + imgs.shape[2:])                                   # :62 / :159
        if self.from_scratch:
            imgs = imgs / 255.0
        B = token_ids.shape[0]
        ids = token_ids.reshape((-1,) + token_ids.shape[2:])                          # :67-70
        mask = input_mask.reshape((-1,) + input_mask.shape[2:])
        C = 1 if getattr(self.qa_head, 'num_labels', None) is not None else ids.shape[0] // B     # :91-95
        if C * B != ids.shape[0]:
            raise ValueError(f'{ids.shape[0]} captions for {B} videos')
        text = self.text_backbone(ids, mask)['last_hidden_state']                    # :78-79
        if text_cut is not None:
            leaf = text.detach().requires_grad_()
            text_cut.append((text, leaf))
            text = leaf
        vis = self.backbone.forward_tokens(imgs, mid_cut=video_cut)                   # channels-last [B', T', h, w, Dv]
        if video_cut is not None:
            cut = (vis, vis.detach().requires_grad_())
            video_cut.append(cut)
            vis = cut[1]
        if vis.shape[0] != B:                                                         # :73-75 clip average
            vis = vis.reshape((B, -1) + vis.shape[1:]).float().mean(dim=1)
        _, T, hh, ww, Dv = vis.shape
        fusion = self.multimodal_backbone(visual_token=vis.reshape(B, T, hh * ww, Dv),
                                          text_input_mask=mask, text_input_embeds=text, num_choices=C,
                                          return_attention=test)
        h = fusion['last_hidden_state']
        Ltot = h.shape[1]
        n_vis = Ltot - ids.shape[1]
        if self.answer_mask:                                                          # :100-102
            base = n_vis
        else:                                                                         # :103-107
            base = n_vis - 1 if 'cls_last_hidden_state' in fusion else n_vis
        rows, counts = ops.qa_answer_rows(ids, Ltot, base, self.answer_mask)
        return h, rows, counts, C, fusion.get('attention')

    def _check_masks(self, counts):
        """Eager fill-in-the-blank calls: every caption must hold exactly one [MASK] (the reference's
        ``t_last_hidden_state[torch.where(token_ids == 103)]`` otherwise yields a row count that matches no label).  The
        engine skips this host check (it would sync inside a capture) and uses the first [MASK] of each caption."""
        if not self.answer_mask or (counts.is_cuda and torch.cuda.is_current_stream_capturing()):
            return
        c = counts.cpu()
        if bool((c != 1).any()):
            bad = [i for i, v in enumerate(c.tolist()) if v != 1]
            raise ValueError(f'FIB: captions {bad[:8]} hold {[c[i].item() for i in bad[:8]]} [MASK] tokens (exactly one '
                             'is required)')

    def _qa_encode(self, imgs, token_ids, input_mask, label, video_cut=None, text_cut=None):
        if label is None:
            raise ValueError('video_qa / FIB training needs label')
        h, rows, counts, C, _ = self._qa_fusion(imgs, token_ids, input_mask, video_cut, text_cut)
        self._check_masks(counts)
        if C > 1:                                                                     # :115-121, K = 1 + CE over C
            loss = self.qa_head(h, rows, labels=label.reshape(-1), num_choices=C)
        else:
            logits = self.qa_head(h, rows)
            loss = self.loss_func(logits, label.reshape(-1))
        return loss.float().reshape(1, 1), None


    def _embeddings(self, imgs, token_ids, input_mask, video_cut=None, text_cut=None):
        """Shared by train and test (:61-81 / :128-147): video tokens (mean over the clips of a sample when
        there are several), caption hidden states, then the two projections."""
        if self.training and imgs.is_cuda:
            ops.dropout_seeds_begin(imgs.device)
        imgs = imgs.reshape((-1,) + imgs.shape[2:])                                   # :62
        if self.from_scratch:
            imgs = imgs / 255.0
        B_text = token_ids.shape[0]
        token_ids = token_ids.reshape((-1,) + token_ids.shape[2:])                    # :67-69
        input_mask = input_mask.reshape((-1,) + input_mask.shape[2:])

        def text_side():
            text = self.text_backbone(token_ids, input_mask)['last_hidden_state']     # :78-79
            if text_cut is not None:
                leaf = text.detach().requires_grad_()
                text_cut.append((text, leaf))
                text = leaf
            return self.ssl_head.forward_text(text, input_mask, token_ids)
        # the caption encoder's kernels are tiny (B x L tokens) and independent of the video encoder: run them on
        # a side stream underneath the Swin kernels, as in the pre-training step
        side = self._text_stream(imgs.device) if imgs.is_cuda and getattr(self, 'overlap_text', True) else None
        if side is not None:
            main = torch.cuda.current_stream()
            side.wait_stream(main)
            with torch.cuda.stream(side):
                text_emb = text_side()
        vis = self.backbone.forward_tokens(imgs, mid_cut=video_cut)                   # channels-last [B,T',h,w,D]
        if video_cut is not None:            # engine graph mode: see CloverPretrain.encode
            cut = (vis, vis.detach().requires_grad_())
            video_cut.append(cut)
            vis = cut[1]
        if B_text != vis.shape[0]:                                                    # :73-75
            vis = vis.reshape((B_text, -1) + vis.shape[1:]).float().mean(dim=1)
        if side is not None:
            main.wait_stream(side)
            text_emb.record_stream(main)
        else:
            text_emb = text_side()
        return self.ssl_head.forward_vision(vis, channels_last=True), text_emb

    def _text_stream(self, device):
        st = getattr(self, '_txt_stream', None)
        if st is None or st.device != device:
            st = torch.cuda.Stream(device=device)
            object.__setattr__(self, '_txt_stream', st)
        return st

    def encode(self, imgs, token_ids=None, input_mask=None, video_cut=None, text_cut=None, label=None, **kwargs):
        """-> (emb fp32 [B, 2, D] in EMB_NAMES order, None): the retrieval step has no rank-local loss.
        video_qa / FIB: (the rank-local qa_loss as fp32 [1, 1], None) — there is nothing to gather across ranks."""
        if self.is_qa:
            return self._qa_encode(imgs, token_ids, input_mask, label, video_cut, text_cut)
        v, t = self._embeddings(imgs, token_ids, input_mask, video_cut, text_cut)
        return torch.stack([v, t], dim=1).float(), None

    def contrastive_losses(self, emb, _local_loss=None):
        if self.is_qa:
            return {'qa_loss': emb.reshape(())}                                      # :122-123
        return {'retrieval_nce_loss': self.loss_func(emb[:, 0], emb[:, 1])}           # :84-86

    def forward_train(self, imgs, label=None, token_ids=None, segment_ids=None, input_mask=None, ans_ids=None,
                      ans_mask=None, **kwargs):
        return self.contrastive_losses(*self.encode(imgs, token_ids=token_ids, input_mask=input_mask, label=label))

    def forward_test(self, imgs, token_ids=None, segment_ids=None, input_mask=None, ans_ids=None, ans_mask=None,
                     **kwargs):
        if self.is_qa and not self.separate_test:                                     # :162-193
            h, rows, counts, C, attention = self._qa_fusion(imgs, token_ids, input_mask, test=True)
            self._check_masks(counts)
            scores = self.qa_head(h, rows)
            return {'result': scores.view(-1, scores.shape[1] if C == 1 else C).float(), 'attention': attention}
        if not self.separate_test:
            raise NotImplementedError('not implement the finetune test method')       # :203-204
        return self._embeddings(imgs, token_ids, input_mask)                          # :146-148

    def forward_gradcam(self, imgs, token_ids=None, segment_ids=None, input_mask=None):
        return self.forward_test(imgs, token_ids, segment_ids, input_mask)
