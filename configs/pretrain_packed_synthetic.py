# configs/pretrain_synthetic.py reading packed uint8 clips instead of pre-made tensors: an 8-frame video stream and a
# one-frame image stream, as WebVid + CC3M.  Run
#     python tools/pack_synthetic_clips.py work_dirs/packed_synthetic --image-clips 48
# first (random frames, no download).  The reference's train pipeline (pretrain_webvid_cc3m.py: RandomResizedCrop ->
# Resize(224) -> Flip(0.5) -> Normalize -> FormatShape) runs on the device as one kernel per batch (ops.clip_prep); each
# stream's loader writes into the static input of its own captured geometry.
_base_ = ['pretrain_synthetic.py']
data = dict(videos_per_gpu=8,
            packed=dict(path='work_dirs/packed_synthetic',
                        train=[dict(split='train', flip_ratio=0.5, size=224), dict(split='image', flip_ratio=0.5, size=224)]))
