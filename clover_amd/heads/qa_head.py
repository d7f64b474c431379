"""Video-QA heads, registered as ``QA_MC_head`` and ``QA_OE_Head`` (mmaction/models/heads/qa_head.py:8-85), with the
reference's kwargs, parameter names (``mc_vqa_classifier.{1,2,4}`` / ``vqa_classifier.{1,2,4}``) and xavier / zero init.

The ``nn.Sequential`` only holds the parameters: the whole chain — Dropout -> Linear(D, H) -> LayerNorm(H) -> GELU ->
Linear(H, K) — runs as the fused HIP head (ops.qa_head, csrc/qa.hip), which reads its input rows through a row table
straight out of the fusion encoder's output and, for multiple choice, folds the softmax-CE over the candidates in."""
import torch
import torch.nn as nn

from .. import ops
from ..builder import HEADS
from ..nn import to_bf16


def init_qa_weights(module):
    """qa_head.py:23-32 / :64-73: xavier-uniform Linear weights, zero biases, LayerNorm (1, 0)."""
    for m in module.modules():
        if isinstance(m, nn.Linear):
            nn.init.xavier_uniform_(m.weight)
            if m.bias is not None:
                m.bias.data.zero_()
        elif isinstance(m, nn.LayerNorm):
            m.bias.data.zero_()
            m.weight.data.fill_(1.0)


class _FusedQAHead(nn.Module):
    """Common forward of the two heads over ``self.classifier`` (the reference's Sequential)."""

    def _run(self, x, rows=None, labels=None, num_choices=None):
        seq = self.classifier
        drop, fc1, ln, fc2 = seq[0], seq[1], seq[2], seq[4]
        if rows is None:                       # plain [..., D] rows (the reference's call: qa_head(itm_output))
            x = x.reshape(-1, 1, x.shape[-1])
            rows = torch.arange(x.shape[0], device=x.device, dtype=torch.int32)
        x = to_bf16(x)                         # the path's storage type: fp32 in parity mode
        return ops.qa_head(x, rows, fc1.weight, fc1.bias, ln.weight, ln.bias, fc2.weight, fc2.bias,
                           drop_p=drop.p if self.training else 0.0, eps=ln.eps, labels=labels, num_choices=num_choices)


@HEADS.register_module()
class QA_MC_head(_FusedQAHead):
    """Multiple choice: one score per (video, candidate) row, hidden width 256 (qa_head.py:8-40)."""

    def __init__(self, hidden_dim, dropout_ratio=0.1):
        super().__init__()
        self.mc_vqa_classifier = nn.Sequential(nn.Dropout(dropout_ratio), nn.Linear(hidden_dim, 256), nn.LayerNorm(256),
                                               nn.GELU(), nn.Linear(256, 1))
        init_qa_weights(self)
        self.fp16_enabled = False

    @property
    def classifier(self):
        return self.mc_vqa_classifier

    def forward(self, x, rows=None, labels=None, num_choices=None):
        """x [..., D] -> scores fp32 [M, 1]; or x = the fusion output [N, S, D] with ``rows`` int32 [N] (its answer rows).
        With ``labels`` [N / num_choices]: the CrossEntropyLoss of the scores viewed [-1, num_choices] (:109-121)."""
        return self._run(x, rows, labels, num_choices)


@HEADS.register_module()
class QA_OE_Head(_FusedQAHead):
    """Open-ended answers (and fill-in-the-blank): ``num_labels`` classes, hidden width hidden_dim // 2 (qa_head.py:43-85)."""

    def __init__(self, hidden_dim=768, dropout_ratio=0.5, num_labels=None, **kwargs):
        super().__init__()
        self.num_labels = num_labels
        self.vqa_classifier = nn.Sequential(nn.Dropout(dropout_ratio), nn.Linear(hidden_dim, hidden_dim // 2),
                                            nn.LayerNorm(hidden_dim // 2), nn.GELU(),
                                            nn.Linear(hidden_dim // 2, self.num_labels))
        init_qa_weights(self)
        self.fp16_enabled = False

    @property
    def classifier(self):
        return self.vqa_classifier

    def forward(self, x, rows=None):
        """x [..., D] (or the fusion output [N, S, D] with ``rows``) -> logits fp32 [M, num_labels]."""
        return self._run(x, rows)
