# Multiple-choice video QA (TGIF-Action / TGIF-Transition / LSMDC-MC) in the reference's config format
# (configs/exp_local/finetune_tgif_action.py): Swin-B + BERT-base, 3-layer fusion encoder on the text CLS row, QA_MC_head
# over 5 candidates x 100 tokens.  The TGIF loaders are replaced by a synthetic batch stream of the same layout
# (clover_amd/utils/qa_synthetic.py); `--load-from` takes a pre-training checkpoint written by tools/train.py.
_base_ = ['_base_default_runtime.py']
videos_per_gpu = 16
num_frames = 8
weight_decay = 0.01
import bench as _bench                                   # noqa: E402  (repo root is on sys.path under tools/train.py)
_pre = _bench.model_cfg('B', num_frames)                 # Swin-B: fc_in 1024 -> 768 (img_in_size=1024)
base_lr = 5e-6 / 128
_qa = dict(num_choices=5)
model = dict(type='CloverFinetune', freeze_stage=None, separate_test=False, backbone=_pre['backbone'],
             freeze_text_backbone=False, text_vocab_size=30522,
             mm_backbone=dict(_pre['mm_backbone'], use_text_cls=True),
             text_backbone=_pre['text_backbone'], cls_head=None, task='video_qa', ssl_head=None,
             itm_head=None, answer_cls=True,
             qa_head=dict(type='QA_MC_head', hidden_dim=768, dropout_ratio=0.5),
             loss_type=dict(type='CrossEntropyLoss'),
             train_cfg=dict(aux_info=['token_ids', 'segment_ids', 'input_mask']))
del _pre
data = dict(videos_per_gpu=videos_per_gpu, synthetic=[dict(length=20, frames=num_frames, tokens=100, qa=_qa)],
            synthetic_test=dict(pairs=64, frames=num_frames, tokens=100, qa=_qa))           # tools/test.py
evaluation = dict(interval=1, metrics=['video_qa_mc'], gpu_collect=True, test_fn='use_itm_head_fn')
optimizer = dict(type='AdamW', base_lr=base_lr, betas=(0.9, 0.98), eps=1e-8, weight_decay=weight_decay,
                 paramwise_cfg=dict(norm_decay_mult=0.0, bias_decay_mult=0.0,
                                    custom_keys={'qa_head': dict(lr_mult=10)}))
optimizer_config = dict(grad_clip=dict(max_norm=50))
fp16 = dict(loss_scale='dynamic')
lr_config = dict(policy='CosineAnnealing', min_lr_ratio=1e-3, by_epoch=False, warmup='linear', warmup_iters=1,
                 warmup_ratio=0.0001, warmup_by_epoch=True)
total_epochs = 2
workflow = [('train', 1)]
