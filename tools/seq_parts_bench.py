#!/usr/bin/env python
"""Device time and peak memory of sequence attention beyond 896 keys, the two ways the tree has:

  own      ops.seq_attention: the fused kernels of csrc/attention.hip as P = ceil(ceil(S / 16) / 28) parts of staged tokens
           + the merge kernels (no library GEMM, O(S) activation memory: o, lse and the P-part scratch)
  unfused  ops._LongSeqAttention: four batched library GEMMs around the HIP row-softmax kernels, three [B, nH, S, S]
           16-bit tensors kept for the backward (the path of S > 4096, and of S > 896 before the P-part form)

Shapes: S in {1030, 1600, 2048, 4096}, 16 sequences x 12 heads x head dim 64 (the fusion encoder's batch; 1600 is the
64-frame fusion sequence), a key mask on one sample, no dropout.  Forward (under no_grad) and forward + backward are timed
with device events around `iters` back-to-back calls after `warmup` calls, the two ways alternating, three rounds each (the
minimum and every round are reported).  Peak memory is torch's peak allocated bytes over one forward + backward above what
is allocated before it.  The outputs of the two ways are compared on the same inputs.  One JSON line per size.

    python tools/seq_parts_bench.py [--iters 10] [--warmup 3] [--sizes 1030,1600,2048,4096] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch                                            # noqa: E402


def _timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--iters', type=int, default=10)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--sizes', default='1030,1600,2048,4096')
    p.add_argument('--out', default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('seq_parts_bench.py needs an MI355X (no CPU fallback)')
    from clover_amd import _lib, ops
    warnings.simplefilter('ignore', RuntimeWarning)         # the unfused path announces its library GEMMs: that is the point here
    dev = torch.device('cuda', 0)
    B, nH, hd = 16, 12, 64
    Hd = nH * hd
    half = _lib.half_dtype()
    lines = []
    for S in [int(s) for s in args.sizes.split(',')]:
        assert 896 < S <= ops.SEQ_FUSED_MAX_KEYS, S
        g = torch.Generator(device=dev).manual_seed(S)
        qkv = torch.randn(B, S, 3 * Hd, generator=g, device=dev).to(half).requires_grad_()
        do = torch.randn(B, S, Hd, generator=g, device=dev).to(half)
        km = torch.zeros(B, S, device=dev)
        km[0, S - 37:] = -10000.0
        geom = _lib.ClvAttnGeom(mode=0, groups=B, N=S, nH=nH, hd=hd, ldq=3 * Hd, ldk=3 * Hd, ldv=3 * Hd, ldo=Hd,
                                scale=hd ** -0.5, dropout_p=0.0)
        parts = _lib.lib().clv_attn_seq_parts(C.byref(geom))

        def own_fwd():
            with torch.no_grad():
                return ops.seq_attention(qkv, km, nH)

        def lib_fwd():
            with torch.no_grad():
                return ops._LongSeqAttention.apply(qkv, km, nH, 0.0, None)

        def own_fb():
            qkv.grad = None
            ops.seq_attention(qkv, km, nH).backward(do)

        def lib_fb():
            qkv.grad = None
            ops._LongSeqAttention.apply(qkv, km, nH, 0.0, None).backward(do)

        before = dict(ops.LIBRARY_GEMM_CALLS)
        own_fb()
        assert ops.LIBRARY_GEMM_CALLS == before, 'the own path called the library'
        o_own, g_own = own_fwd().float(), qkv.grad.float().clone()
        lib_fb()
        o_lib, g_lib = lib_fwd().float(), qkv.grad.float().clone()
        rel = lambda a, b: float((a - b).abs().max() / b.abs().max())      # noqa: E731
        agree = dict(o=rel(o_own, o_lib), dqkv=rel(g_own, g_lib))
        del o_own, g_own, o_lib, g_lib
        for _ in range(args.warmup):
            own_fwd(), lib_fwd(), own_fb(), lib_fb()
        torch.cuda.synchronize()
        t = dict(own_fwd=[], lib_fwd=[], own_fb=[], lib_fb=[])
        for _ in range(3):                                # alternate the two ways
            t['own_fwd'].append(_timed(own_fwd, args.iters))
            t['lib_fwd'].append(_timed(lib_fwd, args.iters))
            t['own_fb'].append(_timed(own_fb, args.iters))
            t['lib_fb'].append(_timed(lib_fb, args.iters))
        qkv.grad = None
        peak_own, peak_lib = _peak(own_fb), _peak(lib_fb)
        qkv.grad = None
        flops_f = 4 * B * nH * S * S * hd                   # 2 matmuls forward, 5 backward (ops._attn_work)
        lines.append(dict(S=S, sequences=B, heads=nH, hd=hd, parts=parts,
                          own_fwd_ms=min(t['own_fwd']), unfused_fwd_ms=min(t['lib_fwd']),
                          own_fwd_bwd_ms=min(t['own_fb']), unfused_fwd_bwd_ms=min(t['lib_fb']),
                          own_fwd_tflops=flops_f / min(t['own_fwd']) / 1e9,
                          own_fwd_bwd_tflops=3.5 * flops_f / min(t['own_fb']) / 1e9,
                          own_peak_mib=peak_own / 2 ** 20, unfused_peak_mib=peak_lib / 2 ** 20,
                          runs={k: v for k, v in t.items()}, max_rel_diff=agree, iters=args.iters, warmup=args.warmup,
                          device=torch.cuda.get_device_name(0), half='f16' if _lib.HALF_F16 else 'bf16',
                          torch=torch.__version__, hip=torch.version.hip))
        print(json.dumps(lines[-1]), flush=True)
        del qkv, do, km
        torch.cuda.empty_cache()
    ops.LIBRARY_GEMM_CALLS.clear()
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(json.dumps(ln) for ln in lines) + '\n')


if __name__ == '__main__':
    main()
