#!/usr/bin/env python
"""Timings behind the patch-embed rows of DESIGN section 4 (profiles/patch_embed_general.txt, profiles/patch_embed_refactor.txt):
prints one JSON row per kernel.

    python tools/patch_embed_bench.py

The forward kernels at the config-2 clip (B = 8, 3 x 8 x 224 x 224 fp32, C = 96, 7 x 7 mask, every output): the fast
(2,4,4 | 2,4,4) kernel, the general kernel at the same geometry, and the general kernel at (1,4,4), (2,4,4 | 1,4,4) and
(4,4,4); and the two backward kernels of the (2,4,4 | 2,4,4) geometry on the same clip, clv_im2col_patches and
clv_patch_embed_blend_bwd (both gradients in).  Device events around 400 back-to-back launches, 7 repeats with the variants alternating inside every repeat, 30
warm-up launches per shape.  Clip and output buffers rotate over 10 sets (385 MB of clips alone, more than the 256 MB
Infinity Cache), so every launch reads its clip from HBM.  Algorithmic bytes = clip read once + clean, masked and z written
+ mean, rstd (im2col: clip read + patches written; blend backward: two gradients read + dy written); roof = bytes / 8 TB/s.
Needs a GPU: there is no CPU leg."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

assert torch.cuda.is_available(), 'tools/patch_embed_bench.py times kernels on the GPU'
from clover_amd import _lib, ops  # noqa: E402
L = _lib.lib(); p = ops._ptr; HALF = _lib.half_dtype(); DEV = 'cuda'
B, T, H, W, C = 8, 8, 224, 224, 96
NBUF = 10
g = torch.Generator().manual_seed(0)
clips = [torch.randn(B, 3, T, H, W, generator=g).to(DEV) for _ in range(NBUF)]
vm = (torch.rand(B, 7, 7, generator=g) > 0.8).long().to(DEV)
def setup(kind, patch, stride):
    K = 3 * patch[0] * patch[1] * patch[2]
    w = (torch.randn(C, K, generator=g) * 0.1).to(DEV, HALF)
    vec = [torch.randn(C, generator=g).to(DEV) for _ in range(4)]
    Tp, Hp, Wp = ops.patch_grid(T, H, W, patch, stride)
    M = B * Tp * Hp * Wp
    outs = [(torch.empty(2 * M, C, device=DEV, dtype=HALF), torch.empty(M, C, device=DEV, dtype=HALF),
             torch.empty(M, device=DEV), torch.empty(M, device=DEV)) for _ in range(NBUF)]
    if kind == 'im2col':
        outs = [torch.empty(M, K, device=DEV, dtype=HALF) for _ in range(NBUF)]
    elif kind == 'blend_bwd':
        outs = [(torch.randn(2, M, C, device=DEV).to(HALF), torch.empty(M, C, device=DEV, dtype=HALF)) for _ in range(NBUF)]
        vec = torch.zeros(C, device=DEV)                 # d mask_token, accumulated into
    return w, vec, (Tp, Hp, Wp), outs
def launch(kind, patch, stride, st, i):
    w, vec, (Tp, Hp, Wp), outs = st
    M = B * Tp * Hp * Wp
    x = clips[i % NBUF]
    if kind == 'im2col':
        rc = L.clv_im2col_patches(p(x), p(outs[i % NBUF]), B, T, H, W, *patch, *stride, ops._stream())
        assert rc == 0, rc
        return
    if kind == 'blend_bwd':
        d, dy = outs[i % NBUF]
        rc = L.clv_patch_embed_blend_bwd(p(d[0]), p(d[1]), p(vm), p(dy), p(vec), B, Tp, Hp, Wp, C, 7, 7, ops._stream())
        assert rc == 0, rc
        return
    both, z, mean, rstd = outs[i % NBUF]
    if kind == 'fast':
        rc = L.clv_patch_embed_fwd(p(x), p(w), p(vec[0]), p(vec[1]), p(vec[2]), p(vec[3]), p(vm), p(both[:M]), p(both[M:]), p(z),
                                   p(mean), p(rstd), B, T, H, W, C, 7, 7, 1e-5, ops._stream())
    else:
        rc = L.clv_patch_embed_gen_fwd(p(x), p(w), p(vec[0]), p(vec[1]), p(vec[2]), p(vec[3]), p(vm), p(both[:M]), p(both[M:]), p(z),
                                       p(mean), p(rstd), B, T, H, W, C, 7, 7, *patch, *stride, 1e-5, ops._stream())
    assert rc == 0, rc
cases = [('fast', (2, 4, 4), (2, 4, 4)), ('gen', (2, 4, 4), (2, 4, 4)), ('gen', (1, 4, 4), (1, 4, 4)), ('gen', (2, 4, 4), (1, 4, 4)),
         ('gen', (4, 4, 4), (4, 4, 4)), ('im2col', (2, 4, 4), (2, 4, 4)), ('blend_bwd', (2, 4, 4), (2, 4, 4))]
states = [setup(k, pa, s) for k, pa, s in cases]
ITERS, REPS = 400, 7
for ci, (k, pa, s) in enumerate(cases):                      # warm-up of every shape
    for i in range(30):
        launch(k, pa, s, states[ci], i)
torch.cuda.synchronize()
times = {ci: [] for ci in range(len(cases))}
for rep in range(REPS):                                      # alternate the variants inside every repeat
    for ci, (k, pa, s) in enumerate(cases):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(ITERS):
            launch(k, pa, s, states[ci], i)
        e1.record(); torch.cuda.synchronize()
        times[ci].append(e0.elapsed_time(e1) * 1e3 / ITERS)   # us per launch (enqueue overlapped: launches are back to back)
res = []
for ci, (k, pa, s) in enumerate(cases):
    M = B * states[ci][2][0] * states[ci][2][1] * states[ci][2][2]
    byt = {'im2col': B * 3 * T * H * W * 4 + M * 3 * pa[0] * pa[1] * pa[2] * 2, 'blend_bwd': 3 * M * C * 2}.get(
        k, B * 3 * T * H * W * 4 + 3 * M * C * 2 + 2 * M * 4)
    ts = sorted(times[ci]); med = ts[len(ts) // 2]
    row = dict(kernel=k, patch=pa, stride=s, tokens=M, us_median=round(med, 2), us_min=round(ts[0], 2), us_max=round(ts[-1], 2),
               algorithmic_MB=round(byt / 1e6, 2), hbm_roof_us=round(byt / 8.0e12 * 1e6, 2), frac_of_hbm_roof=round(byt / 8.0e12 * 1e6 / med, 3))
    print(json.dumps(row)); res.append(row)
