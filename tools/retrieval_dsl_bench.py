#!/usr/bin/env python
"""Device time of dual-softmax re-scored retrieval ranks, ops.retrieval_rank(..., dual_softmax=T), at
(Nq, Ng, D) = (1000, 1000, 768) and (10000, 10000, 768), next to

  plain   ops.retrieval_rank without the option (what the evaluation ran before the option existed)
  torch   what a user would write without it: the normalised [Nq, Ng] score matrix, softmax down dim 0, multiply,
          argsort, position of the ground truth — with its peak device memory

Times are device events around `iters` back-to-back calls after `warmup` calls, the three ways alternating, the best of
three rounds; the DSL ranks of the two ways are compared on the same seeded inputs.  Peak memory is
torch.cuda.max_memory_allocated over one call, minus what was allocated before it.  One JSON line per size.

    python tools/retrieval_dsl_bench.py [--iters 20] [--warmup 3] [--temperature 20] [--out FILE]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch                                            # noqa: E402


def _timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters, out


def _peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - base


def _unit(x):
    n = x.norm(dim=1, keepdim=True)
    return x / torch.where(n == 0, torch.ones_like(n), n)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--iters', type=int, default=20)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--temperature', type=float, default=20.0)
    p.add_argument('--sizes', type=int, nargs='+', default=[1000, 10000])
    p.add_argument('--out', default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('retrieval_dsl_bench.py needs an MI355X (no CPU fallback)')
    from clover_amd import _lib, ops
    dev = torch.device('cuda', 0)
    T, D = args.temperature, 768
    lines = []
    for N in args.sizes:
        g = torch.Generator().manual_seed(N)
        gal = torch.randn(N, D, generator=g)
        a = torch.exp(torch.empty(N, 1).uniform_(-3.9, 0.0, generator=g))          # as the tests' inputs: ranks from 0 into the bulk
        q = (a * gal + torch.randn(N, D, generator=g)).to(dev)
        gal = gal.to(dev)
        gt = torch.arange(N, device=dev)

        def plain():
            return ops.retrieval_rank(q, gal)[0]

        def dsl():
            return ops.retrieval_rank(q, gal, dual_softmax=T)[0]

        def matrix():
            s = torch.matmul(_unit(q), _unit(gal).T)
            sp = s * torch.softmax(T * s, dim=0)
            order = torch.argsort(-sp, dim=1, stable=True)
            return (order == gt[:, None]).int().argmax(dim=1)

        for _ in range(args.warmup):
            plain(), dsl(), matrix()
        torch.cuda.synchronize()
        runs = dict(plain=[], dsl=[], torch=[])
        for _ in range(3):                                # alternate the three ways
            for name, fn in (('plain', plain), ('dsl', dsl), ('torch', matrix)):
                ms, out = _timed(fn, args.iters)
                runs[name].append(ms)
                if name == 'dsl':
                    r_dsl = out
                elif name == 'torch':
                    r_torch = out
        best = {k: min(v) for k, v in runs.items()}
        lines.append(dict(Nq=N, Ng=N, D=D, T=T, plain_ms=best['plain'], dsl_ms=best['dsl'], torch_matrix_ms=best['torch'],
                          dsl_over_plain=best['dsl'] / best['plain'], dsl_over_torch=best['dsl'] / best['torch'],
                          plain_peak_bytes=_peak(plain), dsl_peak_bytes=_peak(dsl), torch_matrix_peak_bytes=_peak(matrix),
                          ranks_agree=float((r_dsl.long() == r_torch.long()).float().mean()),
                          max_rank_difference=int((r_dsl.long() - r_torch.long()).abs().max()),
                          runs_ms=runs, iters=args.iters, device=torch.cuda.get_device_name(0),
                          half='f16' if _lib.HALF_F16 else 'bf16', torch=torch.__version__, hip=torch.version.hip))
    for ln in lines:
        print(json.dumps(ln))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(json.dumps(ln) for ln in lines) + '\n')


if __name__ == '__main__':
    main()
