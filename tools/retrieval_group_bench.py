#!/usr/bin/env python
"""Device time of ops.retrieval_group_best at the two sizes it was written for, next to the full score matrix that gives
the same answer (torch.matmul of the normalised operands, then the diagonal / argsort, as the reference's host code does):

  mc    MSRVTT multiple choice: 2 990 videos x 5 candidates, D = 768 (accuracy.py:396-427)
  msvd  MSVD video -> text: 670 videos against 27 763 texts in ranges of unequal length, best caption and its rank

Times are device events around `iters` back-to-back calls after `warmup` calls, the two ways alternating; the answers of
the two ways are compared on the same seeded inputs.  One JSON line per size.

    python tools/retrieval_group_bench.py [--iters 20] [--warmup 3] [--out FILE]
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


def _unit(x, eps=1e-8):
    return x / torch.clamp(x.norm(dim=1, keepdim=True), min=eps)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--iters', type=int, default=20)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--out', default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('retrieval_group_bench.py needs an MI355X (no CPU fallback)')
    from clover_amd import _lib, ops
    dev = torch.device('cuda', 0)
    g = torch.Generator().manual_seed(0)
    lines = []

    # ---- multiple choice
    N, C, D = 2990, 5, 768
    v = torch.randn(N, D, generator=g).to(dev)
    t = (torch.randn(N * C, D, generator=g) + 0.3 * v.cpu().repeat_interleave(C, 0) *
         (torch.rand(N * C, 1, generator=g) < 0.2)).to(dev)
    lo = torch.arange(N, device=dev, dtype=torch.int32) * C

    def mc_group():
        return ops.retrieval_group_best(v, t, lo, lo + C, eps=1e-8)[0] - lo

    def mc_matrix():
        s = torch.matmul(_unit(v), _unit(t).T).reshape(N, N, C)
        return torch.argmax(torch.diagonal(s, dim1=0, dim2=1).T, dim=-1)

    # ---- MSVD video -> text
    Nv, Nt = 670, 27763
    gcount = torch.Generator().manual_seed(1)
    cuts = torch.sort(torch.randperm(Nt - 1, generator=gcount)[:Nv - 1] + 1).values
    hi = torch.cat([cuts, torch.tensor([Nt])])
    counts = hi - torch.cat([torch.tensor([0]), cuts])
    vv = torch.randn(Nv, D, generator=g).to(dev)
    tt = (torch.randn(Nt, D, generator=g) + 0.3 * vv.cpu().repeat_interleave(counts, 0)).to(dev)
    hi_d = hi.to(dev)
    lo_d = hi_d - counts.to(dev)
    col = torch.arange(Nt, device=dev)[None, :]

    def msvd_group():
        idx, _, rank = ops.retrieval_group_best(vv, tt, lo_d, hi_d, want_rank=True, eps=1e-8)
        return idx, rank

    def msvd_matrix():
        s = torch.matmul(_unit(vv), _unit(tt).T)
        inside = (col >= lo_d[:, None]) & (col < hi_d[:, None])
        best = s.masked_fill(~inside, float('-inf')).argmax(dim=1)
        order = torch.argsort(-s, dim=1, stable=True)
        return best, (order == best[:, None]).int().argmax(dim=1)

    for name, own, full, shape in (('mc', mc_group, mc_matrix, dict(N=N, C=C, D=D)),
                                   ('msvd', msvd_group, msvd_matrix, dict(videos=Nv, texts=Nt, D=D, want_rank=True))):
        for _ in range(args.warmup):
            own()
            full()
        torch.cuda.synchronize()
        t_own, t_full = [], []
        for _ in range(3):                                # alternate the two ways
            ms, a = _timed(own, args.iters)
            t_own.append(ms)
            ms, b = _timed(full, args.iters)
            t_full.append(ms)
        a = a if isinstance(a, tuple) else (a,)
        b = b if isinstance(b, tuple) else (b,)
        agree = [float((x.long() == y.long()).float().mean()) for x, y in zip(a, b)]
        lines.append(dict(case=name, **shape, group_best_ms=min(t_own), full_matrix_ms=min(t_full),
                          group_best_ms_runs=t_own, full_matrix_ms_runs=t_full, agree=agree, iters=args.iters,
                          device=torch.cuda.get_device_name(0), half='f16' if _lib.HALF_F16 else 'bf16',
                          torch=torch.__version__, hip=torch.version.hip))
    for ln in lines:
        print(json.dumps(ln))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(json.dumps(ln) for ln in lines) + '\n')


if __name__ == '__main__':
    main()
