#!/usr/bin/env python
"""Timings behind profiles/clip_prep.txt (bench geometry: 8 clips x 8 frames, 256 x 340 uint8 -> 224 x 224).

    python tools/clip_prep_bench.py --cpu                       # the four steps restated with torch on 16 CPU threads
    python tools/clip_prep_bench.py --kernel                    # clv_clip_prep (fp32 and 16-bit output) and the uint8 H2D copy
    python tools/clip_prep_bench.py --steps <packed dir>        # step time of the retrieval fine-tuning config fed by
                                                                # PackedClipLoader next to the same engine on resident batches

Device times are device events around back-to-back launches after a warm-up, ended by a synchronise; bytes are computed
from the shapes (the crop's source bytes in, the output's bytes out)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, T, HS, WS, S = 8, 8, 256, 340, 224
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
HBM_ROOF = 6.29e12          # bytes / s, the measured float4-copy rate of the MI355X


def inputs(seed=0):
    from clover_amd.utils.packed_loader import random_resized_crop_boxes
    rng = np.random.default_rng(seed)
    src = torch.from_numpy(rng.integers(0, 256, size=(B, T, HS, WS, 3), dtype=np.uint8))
    boxes = random_resized_crop_boxes(rng, B, (HS, WS))
    flips = (rng.random(B) < 0.5).astype(np.uint8)
    return src, boxes, flips


def cpu(threads=16, reps=5):
    """RandomResizedCrop -> Resize(224, bilinear) -> Flip -> Normalize -> FormatShape for one batch, torch on the CPU."""
    import torch.nn.functional as F
    torch.set_num_threads(threads)
    src, boxes, flips = inputs()
    mean, inv = torch.tensor(MEAN).view(1, 3, 1, 1), 1.0 / torch.tensor(STD).view(1, 3, 1, 1)

    def run():
        out = torch.empty(B, 1, 3, T, S, S)
        for b in range(B):
            l, t, r, bt = boxes[b].tolist()
            crop = src[b, :, t:bt, l:r].permute(0, 3, 1, 2).float()                  # [T, 3, h, w]
            v = F.interpolate(crop, size=(S, S), mode='bilinear', align_corners=False)
            if flips[b]:
                v = v.flip(-1)
            out[b, 0] = ((v - mean) * inv).permute(1, 0, 2, 3)
        return out
    run()
    t0 = time.perf_counter()
    for _ in range(reps):
        run()
    dt = (time.perf_counter() - t0) / reps
    print(f'cpu torch restatement, {threads} threads: {dt * 1e3:.1f} ms per batch of {B * T} frames = '
          f'{B * T / dt:.0f} frames/s')


def _timed(fn, warm=20, reps=200):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e-3


def kernel():
    from clover_amd import _lib, ops
    src, boxes, flips = inputs()
    dev = torch.device('cuda')
    pinned = src.pin_memory()
    dsrc = torch.empty_like(src, device=dev)
    t_h2d = _timed(lambda: dsrc.copy_(pinned, non_blocking=True), warm=5, reps=50)
    print(f'H2D uint8 batch ({src.numel() / 1e6:.1f} MB, pinned): {t_h2d * 1e6:.0f} us = {src.numel() / t_h2d / 1e9:.1f} GB/s; '
          f'the same batch as fp32 would be {4 * src.numel() / 1e6:.1f} MB')
    crop_bytes = int(sum((r - l) * (b - t) for l, t, r, b in boxes.tolist())) * T * 3
    full = ops.clip_prep_plan(B, T, HS, WS, S)
    print(f'plan: {full}')
    db = torch.from_numpy(boxes).to(dev)
    df = torch.from_numpy(flips).to(dev)
    mean_d, inv_d = ops.clip_prep_constants(MEAN, STD, dev)
    import ctypes as C
    for dtype in (torch.float32, _lib.half_dtype()):
        out = torch.empty(B, 1, 3, T, S, S, device=dev, dtype=dtype)
        g = _lib.ClvClipPrepGeom(B=B, T=T, Hs=HS, Ws=WS, C=3, S=S, out_dtype=int(dtype != torch.float32), pad=0, boxes_host=None)
        L, st = _lib.lib(), ops._stream()

        def launch():           # the launcher alone: the binding's host-side checks and uploads are not kernel time
            _lib.check(L.clv_clip_prep(ops._ptr(dsrc), ops._ptr(db), ops._ptr(df), ops._ptr(mean_d), ops._ptr(inv_d),
                                       ops._ptr(out), C.byref(g), st), 'clv_clip_prep')
        t = _timed(launch)
        moved = crop_bytes + out.numel() * out.element_size()
        print(f'clv_clip_prep -> {dtype}: {t * 1e6:.1f} us per launch ({B * T} frames: {B * T / t / 1e6:.2f} M frames/s); '
              f'must move {moved / 1e6:.1f} MB (crops {crop_bytes / 1e6:.1f} + out {out.numel() * out.element_size() / 1e6:.1f}) '
              f'= {moved / t / 1e12:.2f} TB/s = {100 * moved / t / HBM_ROOF:.0f} % of the {HBM_ROOF / 1e12:.2f} TB/s HBM roof')
        t = _timed(lambda: ops.clip_prep(dsrc, boxes, flips, MEAN, STD, out=out), warm=5, reps=50)
        print(f'ops.clip_prep -> {dtype} (host checks + box / flip upload + launch): {t * 1e6:.1f} us per call')


def steps(path, n_epochs=8):
    import clover_amd
    from clover_amd.engine import CloverEngine
    from clover_amd.runner import Config
    from clover_amd.utils.packed_loader import packed_loaders
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from train import SyntheticLoader, engine_kwargs
    dev = torch.device('cuda')
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'finetune_retrieval_packed_synthetic.py'))
    vpg = cfg.get('videos_per_gpu', 16)
    spec = dict(cfg.data['packed'])
    spec['path'] = path
    for mode in ('synthetic', 'packed'):
        torch.manual_seed(0)
        model = clover_amd.build_model(dict(cfg.model)).to(dev)
        model.train()
        if mode == 'packed':
            ld = packed_loaders(spec, 'train', vpg, dev)[0]
        else:
            ld = SyntheticLoader(len(packed_loaders(spec, 'train', vpg, dev)[0]), vpg, 8, 32, 1000, dev)
        first = next(iter(ld))
        eng = CloverEngine(model, first, **engine_kwargs(cfg, 1e-6, clover_amd._lib.HALF_F16))
        eng.dry_step(first)
        eng.capture(first)
        if mode == 'packed':
            ld.engine = eng
        for batch in ld:                    # warm-up epoch
            eng.step(batch)
        torch.cuda.synchronize()
        t0, n = time.perf_counter(), 0
        for _ in range(n_epochs):
            for batch in ld:
                eng.step(batch)
                n += 1
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / n
        print(f'{mode} loader, {vpg} clips x 8 frames per step, hipGraph replay: {dt * 1e3:.2f} ms per step over {n} steps '
              f'= {vpg * 8 / dt:.0f} frames/s')
        del eng, model


if __name__ == '__main__':
    p = argparse.ArgumentParser()
    p.add_argument('--cpu', action='store_true')
    p.add_argument('--kernel', action='store_true')
    p.add_argument('--steps', metavar='DIR', default=None)
    a = p.parse_args()
    if a.cpu:
        cpu()
    if a.kernel:
        kernel()
    if a.steps:
        steps(a.steps)
