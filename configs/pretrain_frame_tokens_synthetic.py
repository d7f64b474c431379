# configs/pretrain_synthetic.py with per-frame tokens: PatchEmbed3D patch_size = stride = (1, 4, 4).  An 8-frame clip gives the
# captions 8 temporal positions instead of 4 (mm_backbone.num_frames = the frame count), a one-frame image is one temporal
# position without a zero-padded second frame, and a 2-D Swin checkpoint inflates without the 1 / patch_t averaging.  Any
# geometry but (2,4,4 | 2,4,4) runs the general patch-embed kernel (clv_patch_embed_gen_fwd); the other
# supported ones — patch_size = stride = (4, 4, 4), or stride = (1, 4, 4) under patch_size = (2, 4, 4) (overlapping tubelets,
# num_frames = frames - 1) — are set the same way.
_base_ = ['_base_default_runtime.py']
videos_per_gpu = 2
base_lr = 5e-5 / 1024
weight_decay = 0.005
fp16 = dict(loss_scale='dynamic')                       # as the reference (pretrain_webvid_cc3m.py:21): the engine's device-resident scaler
frames = 8
import bench as _bench                                   # noqa: E402  (repo root is on sys.path under tools/train.py)
model = _bench.model_cfg('T', frames)
model['backbone'].update(patch_size=(1, 4, 4), stride=(1, 4, 4))
model['mm_backbone'].update(num_frames=frames)
data = dict(videos_per_gpu=videos_per_gpu,
            synthetic=[dict(length=8, frames=frames, tokens=32), dict(length=6, frames=1, tokens=32)])
optimizer = dict(type='AdamW', base_lr=base_lr, betas=(0.9, 0.98), eps=1e-8, weight_decay=weight_decay,
                 paramwise_cfg=dict(norm_decay_mult=0.0, bias_decay_mult=0.0,
                                    custom_keys={'absolute_pos_embed': dict(decay_mult=0.),
                                                 'relative_position_bias_table': dict(decay_mult=0.)}))
optimizer_config = dict(grad_clip=dict(max_norm=15))
lr_config = dict(policy='CosineAnnealing', min_lr_ratio=1e-3, by_epoch=False, warmup='linear', warmup_iters=2,
                 warmup_ratio=0.001, warmup_by_epoch=True)
total_epochs = 2
