#!/usr/bin/env python
"""Write a small packed-clip directory for the `data.packed` configs (clover_amd/utils/packed_loader.py), no download:

    python tools/pack_synthetic_clips.py work_dirs/packed_synthetic
    python tools/train.py configs/finetune_retrieval_packed_synthetic.py --launcher none --validate

<dir>/train and <dir>/test (and <dir>/image with --image-clips: one-frame clips, the pre-training image stream) each hold
frames.npy (uint8 [N, T, Hs, Ws, 3]: random frames, except clip 0 = flat grey and clip 1 = a ramp in x and y — the two
images whose resampled values are known in closed form), text.npz (token ids, masks and labels in the layout of
bench.synthetic_batch) and meta.json (mean, std, channel order)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)     # the reference's img_norm_cfg (RGB order)


def write_split(path, clips, frames, height, width, tokens, seed):
    import bench
    os.makedirs(path, exist_ok=True)
    rng = np.random.default_rng(seed)
    out = np.lib.format.open_memmap(os.path.join(path, 'frames.npy'), mode='w+', dtype=np.uint8,
                                    shape=(clips, frames, height, width, 3))
    for i in range(clips):
        out[i] = rng.integers(0, 256, size=(frames, height, width, 3), dtype=np.uint8)
    if clips > 0:
        out[0] = 128
    if clips > 1:
        y, x = np.mgrid[0:height, 0:width]
        ramp = (255.0 * (x / max(width - 1, 1) + y / max(height - 1, 1)) / 2.0).astype(np.uint8)
        out[1] = ramp[None, :, :, None]
    out.flush()
    del out
    b = bench.synthetic_batch(clips, 1, tokens, seed, size=8)
    np.savez(os.path.join(path, 'text.npz'), **{k: b[k].numpy() for k in
                                                ('token_ids', 'segment_ids', 'input_mask', 'mlm_label', 'v_token_mask', 'label')})
    with open(os.path.join(path, 'meta.json'), 'w') as f:
        json.dump(dict(mean=list(MEAN), std=list(STD), channel_order='rgb'), f)


def main():
    p = argparse.ArgumentParser(description='write a synthetic packed-clip directory')
    p.add_argument('out', help='directory to write (train/, test/ and optionally image/ below it)')
    p.add_argument('--train-clips', type=int, default=48)
    p.add_argument('--test-clips', type=int, default=32)
    p.add_argument('--image-clips', type=int, default=0, help='also write image/: this many one-frame clips')
    p.add_argument('--frames', type=int, default=8)
    p.add_argument('--height', type=int, default=256)
    p.add_argument('--width', type=int, default=340)
    p.add_argument('--tokens', type=int, default=32)
    p.add_argument('--seed', type=int, default=0)
    a = p.parse_args()
    write_split(os.path.join(a.out, 'train'), a.train_clips, a.frames, a.height, a.width, a.tokens, a.seed)
    write_split(os.path.join(a.out, 'test'), a.test_clips, a.frames, a.height, a.width, a.tokens, a.seed + 1)
    if a.image_clips:
        write_split(os.path.join(a.out, 'image'), a.image_clips, 1, a.height, a.width, a.tokens, a.seed + 2)
    print(f'wrote {a.out}: train {a.train_clips}, test {a.test_clips}, image {a.image_clips} clips of '
          f'{a.frames} x {a.height} x {a.width}')


if __name__ == '__main__':
    main()
