# configs/finetune_retrieval_synthetic.py reading packed uint8 clips instead of pre-made tensors.  Run
#     python tools/pack_synthetic_clips.py work_dirs/packed_synthetic
# first: it writes the train / test splits below (random 8 x 256 x 340 frames, no download).  The reference's train pipeline
# (finetune_msrvtt_retrieval.py: RandomResizedCrop -> Resize(224) -> Flip(0.5) -> Normalize -> FormatShape) and its test
# pipeline (Resize(-1, 224) -> CenterCrop(224) -> ...) run on the device as one kernel per batch (ops.clip_prep), writing
# into the static input of the captured step.
_base_ = ['finetune_retrieval_synthetic.py']
data = dict(videos_per_gpu=16,
            packed=dict(path='work_dirs/packed_synthetic',
                        train=dict(split='train', flip_ratio=0.5, area_range=(0.08, 1.0), size=224),
                        test=dict(split='test', size=224)))
