# configs/pretrain_synthetic.py at 32-frame clips with the window of the public 32-frame VideoSwin checkpoints:
# window_size = (16, 7, 7), 784 tokens per window (the 16 temporal positions of a 32-frame clip in ONE window, where the
# default (8, 7, 7) cuts them in two).  VideoSwin-T + BERT-base + 3-layer fusion, all five losses.  Windows beyond 448
# tokens run on the own attention kernels as two parts of 400 staged tokens (ops.window_attention), the
# 816-token fusion sequence as two parts as well, so the config also runs with CLOVER_STRICT_OWN_GEMM=1.  Stages 2 and 3
# (16 x 14 x 14 and 16 x 7 x 7 tokens) keep the 784-token window; the 1-frame image stream clips it to (1, 7, 7).
_base_ = ['_base_default_runtime.py']
videos_per_gpu = 2
base_lr = 5e-5 / 1024
weight_decay = 0.005
fp16 = dict(loss_scale='dynamic')                       # as the reference (pretrain_webvid_cc3m.py:21): the engine's device-resident scaler
import bench as _bench                                   # noqa: E402  (repo root is on sys.path under tools/train.py)
model = _bench.model_cfg('T', 32)
model['backbone'].update(window_size=(16, 7, 7))
data = dict(videos_per_gpu=videos_per_gpu,
            # lengths: the reference's interleave (clover_runner.py:76-93) needs long <= 1.5 * short, else its restarted
            # iterator runs dry mid-epoch (StopIteration there and here)
            synthetic=[dict(length=8, frames=32, tokens=32), dict(length=6, frames=1, tokens=32)])
optimizer = dict(type='AdamW', base_lr=base_lr, betas=(0.9, 0.98), eps=1e-8, weight_decay=weight_decay,
                 paramwise_cfg=dict(norm_decay_mult=0.0, bias_decay_mult=0.0,
                                    custom_keys={'absolute_pos_embed': dict(decay_mult=0.),
                                                 'relative_position_bias_table': dict(decay_mult=0.)}))
optimizer_config = dict(grad_clip=dict(max_norm=15))
lr_config = dict(policy='CosineAnnealing', min_lr_ratio=1e-3, by_epoch=False, warmup='linear', warmup_iters=2,
                 warmup_ratio=0.001, warmup_by_epoch=True)
total_epochs = 2
