# configs/pretrain_synthetic.py at 64-frame clips: VideoSwin-T + BERT-base + 3-layer fusion, all five losses.  The fusion
# encoder sees 32 temporal positions x 49 spatial tokens + 32 text tokens = 1600 tokens per sample (model_cfg: num_frames =
# 32): its self-attention runs on the own kernels as four parts of 400 staged tokens (ops.seq_attention),
# so the config also runs with CLOVER_STRICT_OWN_GEMM=1.  The synthetic sets are a 64-frame video stream and a 1-frame
# image stream; the engine keeps one set of hipGraphs per batch geometry.
_base_ = ['_base_default_runtime.py']
videos_per_gpu = 2
base_lr = 5e-5 / 1024
weight_decay = 0.005
fp16 = dict(loss_scale='dynamic')                       # as the reference (pretrain_webvid_cc3m.py:21): the engine's device-resident scaler
import bench as _bench                                   # noqa: E402  (repo root is on sys.path under tools/train.py)
model = _bench.model_cfg('T', 64)
data = dict(videos_per_gpu=videos_per_gpu,
            # lengths: the reference's interleave (clover_runner.py:76-93) needs long <= 1.5 * short, else its restarted
            # iterator runs dry mid-epoch (StopIteration there and here)
            synthetic=[dict(length=8, frames=64, tokens=32), dict(length=6, frames=1, tokens=32)])
optimizer = dict(type='AdamW', base_lr=base_lr, betas=(0.9, 0.98), eps=1e-8, weight_decay=weight_decay,
                 paramwise_cfg=dict(norm_decay_mult=0.0, bias_decay_mult=0.0,
                                    custom_keys={'absolute_pos_embed': dict(decay_mult=0.),
                                                 'relative_position_bias_table': dict(decay_mult=0.)}))
optimizer_config = dict(grad_clip=dict(max_norm=15))
lr_config = dict(policy='CosineAnnealing', min_lr_ratio=1e-3, by_epoch=False, warmup='linear', warmup_iters=2,
                 warmup_ratio=0.001, warmup_by_epoch=True)
total_epochs = 2
