#!/usr/bin/env python
"""Time of ops.window_attention at Swin-B shapes of a 32-frame 224-pixel clip (B = 2): the (16, 7, 7) window — 784 tokens, the
part path of csrc/attention.hip — beside the (8, 7, 7) window on the same tokens (392 tokens, the one-part kernels).
Forward and forward + backward with the table gradient, device events around each warmed run, the median of `--iters`
runs; the fraction is algorithmic flops (ops._attn_work: 4 / 14 N^2 hd per (window, head)) over 2.5 PFLOP/s.
Informational: one JSON line per (stage, window).

    python tools/window_attention_bench.py [--iters 20] [--warmup 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 2.5e15
STAGES = {'stage0': (16, 56, 56, 128, 4), 'stage2': (16, 14, 14, 512, 16)}       # Swin-B: D', H', W', C, heads (hd 32)


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=2)
    a = ap.parse_args()
    from clover_amd import _lib, ops
    from clover_amd.backbones.swin_transformer_3d import window_geometry
    dev, B = 'cuda', a.batch
    for stage, (D, H, W, C, nH) in STAGES.items():
        for tw, shift in (((16, 7, 7), (8, 3, 3)), ((8, 7, 7), (4, 3, 3))):
            for shifted in (False, True):
                ws, ss, rid = window_geometry((D, H, W), tw, shift if shifted else (0, 0, 0), dev)
                N, hd = ws[0] * ws[1] * ws[2], C // nH
                groups = B * (D // ws[0]) * (H // ws[1]) * (W // ws[2])
                g = torch.Generator(device=dev).manual_seed(1)
                qkv = torch.randn(B, D, H, W, 3 * C, generator=g, device=dev).to(_lib.half_dtype()).requires_grad_()
                table = (0.5 * torch.randn((2 * tw[0] - 1) * (2 * tw[1] - 1) * (2 * tw[2] - 1), nH, generator=g,
                                           device=dev)).requires_grad_()
                do = torch.randn(B, D, H, W, C, generator=g, device=dev).to(_lib.half_dtype())
                use_rid = rid if any(ss) else None

                def fwd():
                    with torch.no_grad():
                        return ops.window_attention(qkv, table, use_rid, ws, ss, nH, table_window=tw)

                def fwd_bwd():
                    qkv.grad = table.grad = None
                    ops.window_attention(qkv, table, use_rid, ws, ss, nH, table_window=tw).backward(do)
                per = groups * nH * N * N * hd
                f_ms, b_ms = timed(fwd, a.warmup, a.iters), timed(fwd_bwd, a.warmup, a.iters)
                print(json.dumps(dict(
                    stage=stage, window=list(ws), shift=list(ss), tokens_per_window=N, groups=groups, heads=nH, hd=hd,
                    fwd_ms=round(f_ms[0], 4), fwd_min_max_ms=[round(f_ms[1], 4), round(f_ms[2], 4)],
                    fwd_bwd_ms=round(b_ms[0], 4), fwd_bwd_min_max_ms=[round(b_ms[1], 4), round(b_ms[2], 4)],
                    fwd_flop_frac=round(4 * per / (f_ms[0] * 1e-3) / PEAK, 4),
                    fwd_bwd_flop_frac=round(14 * per / (b_ms[0] * 1e-3) / PEAK, 4), iters=a.iters)), flush=True)
                del qkv, table, do
                torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
