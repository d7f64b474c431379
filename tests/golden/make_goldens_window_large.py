"""Golden-vector generator for windows beyond 448 tokens — BUILD-CONTAINER ONLY (beside make_goldens.py).

Runs the REAL reference SwinTransformer3D (imported from /root/reference through ref_harness.py) with
window_size = (16, 7, 7) on a 32-frame clip and writes tests/golden/g_window_large.npz:

    python tests/golden/make_goldens_window_large.py

Model: SwinTransformer3D(embed_dim=48, depths=[2, 2], num_heads=[3, 6], window_size=(16, 7, 7), pretrained2d=False) on one
closed-form 1 x 3 x 32 x 56 x 56 clip: 16 x 14 x 14 tokens, stage 0 = four 784-token windows per sample with shift (0, 3, 3)
in the second block, stage 1 (16 x 7 x 7) = one window without shift.  (The reference computes the second extent of the
window from the grid too, so a (16, 7, 7) table serves both.)

The state dict is the closed-form one (closed_form.cf_state over the reference's own parameter names and shapes): its 398k
fp32 values would be 1.6 MB, beyond what a committed file may hold, and they are a pure function of the names — so the fixture
stores the manifest (names and shapes, as JSON text) and the tests rebuild the values from it, as every other fixture here
does with manifest_tiny.json.  Stored in full: the output (75k values, 0.3 MB), the seeded output gradient's tag, and the
gradients of the first block's relative_position_bias_table and qkv.weight and of the patch-embed weight.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import closed_form as cf  # noqa: E402
import ref_harness as H  # noqa: E402

CFG = dict(embed_dim=48, depths=[2, 2], num_heads=[3, 6], window_size=(16, 7, 7), pretrained2d=False)
CLIP = (1, 3, 32, 56, 56)
GRADS = ['layers.0.blocks.0.attn.relative_position_bias_table', 'layers.0.blocks.0.attn.qkv.weight', 'patch_embed.proj.weight']


def main():
    H.install_shims()
    import mmaction.models.backbones.swin_transformer_3d as S
    torch.manual_seed(0)
    bb = S.SwinTransformer3D(**CFG)
    bb.eval()
    manifest = {k: list(v.shape) for k, v in bb.state_dict().items() if 'relative_position_index' not in k}
    missing, unexpected = bb.load_state_dict(cf.cf_state(manifest), strict=False)
    assert all('relative_position_index' in k for k in missing) and not unexpected, (missing, unexpected)
    x = cf.cf_float('window_large.clip', CLIP, 1.0)
    y = bb(x)
    assert tuple(y.shape) == (1, 96, 16, 7, 7), y.shape
    gw = cf.cf_float('window_large.gw', tuple(y.shape), 1.0)
    bb.zero_grad()
    (y * gw).sum().backward()
    named = dict(bb.named_parameters())
    out = {'manifest': np.array(json.dumps(manifest)), 'out': y.detach().numpy()}
    for k in GRADS:
        out['grad.' + k] = named[k].grad.detach().numpy()
    path = os.path.join(HERE, 'g_window_large.npz')
    np.savez_compressed(path, **out)
    print(f'wrote g_window_large.npz: {len(out)} arrays, {os.path.getsize(path) / 1024:.1f} KiB')


if __name__ == '__main__':
    main()
