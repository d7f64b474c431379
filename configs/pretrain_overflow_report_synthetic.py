# configs/pretrain_synthetic.py with the overflow report: every optimizer step also launches the two "on skip" kernels of
# clv_grad_report over the gradients (they return at once unless the step was skipped), and an OverflowHook reads the
# optimizer's device record every `interval` steps — loss_scale, grad_norm and skipped go into its records, a skipped step
# prints the `top` parameters that held the non-finite gradients, and `max_consecutive_skips` skipped steps in a row stop
# the run with their names (a static scale that overflows would otherwise skip every step in silence).
_base_ = ['_base_default_runtime.py']
videos_per_gpu = 8
base_lr = 5e-5 / 1024
weight_decay = 0.005
fp16 = dict(loss_scale='dynamic')                       # as the reference (pretrain_webvid_cc3m.py:21): the engine's device-resident scaler
overflow_report = dict(interval=4, top=5, max_consecutive_skips=64)     # (the dynamic scale starts at 2^32: ~20 skips to settle)
import bench as _bench                                   # noqa: E402  (repo root is on sys.path under tools/train.py)
model = _bench.model_cfg('T', 8)
data = dict(videos_per_gpu=videos_per_gpu,
            # lengths: the reference's interleave (clover_runner.py:76-93) needs long <= 1.5 * short, else its restarted
            # iterator runs dry mid-epoch (StopIteration there and here)
            synthetic=[dict(length=16, frames=8, tokens=32), dict(length=12, frames=1, tokens=32)])
optimizer = dict(type='AdamW', base_lr=base_lr, betas=(0.9, 0.98), eps=1e-8, weight_decay=weight_decay,
                 paramwise_cfg=dict(norm_decay_mult=0.0, bias_decay_mult=0.0,
                                    custom_keys={'absolute_pos_embed': dict(decay_mult=0.),
                                                 'relative_position_bias_table': dict(decay_mult=0.)}))
optimizer_config = dict(grad_clip=dict(max_norm=15))
lr_config = dict(policy='CosineAnnealing', min_lr_ratio=1e-3, by_epoch=False, warmup='linear', warmup_iters=4,
                 warmup_ratio=0.001, warmup_by_epoch=True)
total_epochs = 2
