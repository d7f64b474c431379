#!/usr/bin/env python
"""Device time of the retrieval loss section, forward + backward, the two losses a fine-tuning config can name:

  plain  ops.norm_softmax_loss(v, t)                    NormSoftmaxLoss (clv_normsoftmax_*)
  dsl    ops.norm_softmax_loss(v, t, dual_softmax=20)   the dual-softmax loss (clv_dsl_loss_*)

Shapes: (G, Dm) = (128, 768), the reference's 8 x 16 fine-tuning batch, and (1024, 768), a virtual-rank global batch; each in
the one-workgroup and in the multi-workgroup form where that form applies (the one-workgroup form is not timed at G = 1024:
it exists for device batches).  The normalisation, the three GEMMs and the normalisation's backward are the same launches
in both losses, so `extra_fwd_bwd_ms` = dsl - plain is the cost of the added passes over the G x G matrix (2 -> 4 in the
forward, 1 -> 3 in the backward) and of their launches; the GEMM time is not measured apart (that takes a kernel trace).

Timed with device events around `iters` back-to-back calls after `warmup` calls — forward + backward, and the forward alone
under no_grad — the two losses alternating, five rounds each (the minimum and every round are reported); a call takes
0.05 .. 2 ms, so iters defaults to 200.  Issued eagerly through clover_amd.ops, as the engine's loss section issues them:
the figures include the launch overhead of 7 (plain) or 8 .. 13 (dsl) dependent launches.  One JSON line per (shape, form).

    python tools/dsl_loss_bench.py [--iters 200] [--warmup 20] [--out FILE]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch                                            # noqa: E402

T_DSL, TEMP, EPS = 20.0, 0.05, 1e-8
SHAPES = ((128, 768, (False, True)), (1024, 768, (True,)))


def _timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--iters', type=int, default=200)
    p.add_argument('--warmup', type=int, default=20)
    p.add_argument('--out', default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('dsl_loss_bench.py needs an MI355X (no CPU fallback)')
    from clover_amd import _lib, ops
    dev = torch.device('cuda', 0)
    lines = []
    for G, Dm, forms in SHAPES:
        g = torch.Generator(device=dev).manual_seed(G)
        v = torch.randn(G, Dm, generator=g, device=dev)
        t = (0.5 * v + torch.randn(G, Dm, generator=g, device=dev)).requires_grad_()
        v.requires_grad_()
        for large in forms:
            ops.NCE_FORCE_LARGE = large

            def run(dual):
                v.grad = t.grad = None
                loss = ops.norm_softmax_loss(v, t, temperature=TEMP, eps=EPS, dual_softmax=dual)
                loss.backward()
                return loss

            def fwd(dual):
                with torch.no_grad():
                    return ops.norm_softmax_loss(v, t, temperature=TEMP, eps=EPS, dual_softmax=dual)

            before = dict(ops.LIBRARY_GEMM_CALLS)
            losses = dict(plain=float(run(None)), dsl=float(run(T_DSL)), dsl_T0=float(run(0.0)))
            assert ops.LIBRARY_GEMM_CALLS == before, 'the loss section called the library'
            for _ in range(args.warmup):
                run(None), run(T_DSL), fwd(None), fwd(T_DSL)
            torch.cuda.synchronize()
            tm = dict(plain_fb=[], dsl_fb=[], plain_fwd=[], dsl_fwd=[])
            for _ in range(5):                            # alternate the two losses
                tm['plain_fb'].append(_timed(lambda: run(None), args.iters))
                tm['dsl_fb'].append(_timed(lambda: run(T_DSL), args.iters))
                tm['plain_fwd'].append(_timed(lambda: fwd(None), args.iters))
                tm['dsl_fwd'].append(_timed(lambda: fwd(T_DSL), args.iters))
            best = {k: min(x) for k, x in tm.items()}
            lines.append(dict(G=G, Dm=Dm, form='multi' if large else 'one', dual_softmax=T_DSL, temperature=TEMP,
                              plain_fwd_bwd_ms=best['plain_fb'], dsl_fwd_bwd_ms=best['dsl_fb'],
                              plain_fwd_ms=best['plain_fwd'], dsl_fwd_ms=best['dsl_fwd'],
                              ratio_fwd_bwd=best['dsl_fb'] / best['plain_fb'], ratio_fwd=best['dsl_fwd'] / best['plain_fwd'],
                              extra_fwd_bwd_ms=best['dsl_fb'] - best['plain_fb'],
                              launches=dict(plain_fwd=3 if not large else 5, dsl_fwd=3 if not large else 7,
                                            plain_bwd=4, dsl_bwd=5 if not large else 6),
                              losses=losses, runs=tm, iters=args.iters, warmup=args.warmup,
                              device=torch.cuda.get_device_name(0), half='f16' if _lib.HALF_F16 else 'bf16',
                              torch=torch.__version__, hip=torch.version.hip))
            print(json.dumps(lines[-1]), flush=True)
    ops.NCE_FORCE_LARGE = None
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(json.dumps(ln) for ln in lines) + '\n')


if __name__ == '__main__':
    main()
