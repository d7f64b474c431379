#!/usr/bin/env python
"""Measurements behind virtual ranks: prints ONE JSON object.

    python tools/virtual_ranks_bench.py                      # both tables
    python tools/virtual_ranks_bench.py --only loss          # (a) alone; --only step: (b) alone

(a) loss section: forward + backward of ops.exclusive_infonce_rank_pair on a packed [G, 6, 768] tensor, G in 16 .. 1024,
    the one-workgroup kernels against the multi-workgroup ones on the same box in the same process, samples alternating
    between the two.  Each sample is one replay of a hipGraph of the forward + backward (GPU time between two events, no
    host pacing), and once more issued eagerly, as the engine's loss section issues it (host-paced at small G); the table
    gives the medians of 20 after warm-up, the ratios, and the largest difference of the four losses and of the gradient.
    The dispatch threshold (NCE_LARGE_MIN_G, csrc/losses.hip) belongs at the smallest G from which the new path wins in
    both; --G takes other sizes when the crossover lies outside the default list.
(b) step: pairs/s of the captured config-2 step (VideoSwin-T, 8 clips x 8 frames per micro-batch) for k = 1, 2, 4, 8 virtual
    ranks, next to the cost model (k (F + B) + (k - 1) F + L + O) / k built from phase_ms() of the k = 1 run (F forward
    graph, B backward graphs, L loss section, O optimizer): k - 1 micro-batches are recomputed, L and O are paid once.

Every GPU leg is a child process under its own `timeout`; the first leg that fails ends the run (nothing more is started
on the device) and the JSON says which."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOSS_G = (16, 32, 64, 128, 256, 512, 1024)
STEP_K = (1, 2, 4, 8)


def leg_loss(args):
    import torch
    from clover_amd import ops
    dev = torch.device('cuda', 0)
    sa, sb, wts = (0, 1, 2, 3), (1, 0, 4, 5), (1.3, 0.7, 0.9, 1.1)
    rows = []
    for G in args.G:
        g = torch.Generator().manual_seed(G)
        p = torch.randn(G, 6, 768, generator=g)
        p[:, 1] = p[:, 0] * 0.7 + p[:, 1] * 0.5
        p[:, 4] = p[:, 1] * 0.6 + p[:, 4] * 0.6
        packed = p.to(dev)
        graphs, outs = {}, {}
        for name, large in (('old', False), ('new', True)):
            ops.NCE_FORCE_LARGE = large
            leaf = packed.clone().requires_grad_()

            def run(leaf=leaf):
                leaf.grad = None
                o = ops.exclusive_infonce_rank_pair(leaf, sa, sb, 0.05, 5.0)
                sum(w * x for w, x in zip(wts, o)).backward()
                return torch.stack([x.detach() for x in o])
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    run()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                res = run()
            graphs[name], outs[name] = gr, (res, leaf, run)
        ops.NCE_FORCE_LARGE = None
        for _ in range(5):
            for gr in graphs.values():
                gr.replay()
        torch.cuda.synchronize()
        ms = {'old': [], 'new': []}
        for _ in range(args.samples):
            for name in ('old', 'new'):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                graphs[name].replay()
                b.record()
                b.synchronize()
                ms[name].append(a.elapsed_time(b))
        med = {n: statistics.median(v) for n, v in ms.items()}
        # the same launches issued eagerly, as the engine's loss section issues them: at small G the host paces them, and
        # the new path's forward is five launches where the old one's is three
        eager = {'old': [], 'new': []}
        for it in range(5 + args.samples):
            for name, large in (('old', False), ('new', True)):
                ops.NCE_FORCE_LARGE = large
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                outs[name][2]()
                b.record()
                b.synchronize()
                if it >= 5:
                    eager[name].append(a.elapsed_time(b))
        ops.NCE_FORCE_LARGE = None
        emed = {n: statistics.median(v) for n, v in eager.items()}
        dl = float((outs['old'][0] - outs['new'][0]).abs().max())
        go, gn = outs['old'][1].grad, outs['new'][1].grad
        dg = float((go - gn).abs().max() / go.abs().max())
        rows.append(dict(G=G, old_ms=round(med['old'], 4), new_ms=round(med['new'], 4),
                         old_over_new=round(med['old'] / med['new'], 3), old_min_ms=round(min(ms['old']), 4),
                         new_min_ms=round(min(ms['new']), 4), eager_old_ms=round(emed['old'], 4),
                         eager_new_ms=round(emed['new'], 4), eager_old_over_new=round(emed['old'] / emed['new'], 3),
                         max_loss_diff=dl, grad_rel_diff=dg))
    print(json.dumps(dict(leg='loss', Dm=768, samples=args.samples, dispatch_min_g=ops.nce_large_min_g(), rows=rows)))


def leg_step(args):
    import torch
    import bench
    import clover_amd
    from clover_amd import ops
    from clover_amd.engine import CloverEngine
    k, B = args.k, 8
    dev = torch.device('cuda', 0)
    torch.manual_seed(1234)
    model = clover_amd.build_model(bench.model_cfg('T', 8)).to(dev)
    model.train()
    micro = [{n: v.to(dev) for n, v in bench.synthetic_batch(B, 8, 32, 1000 + j).items()} for j in range(k)]
    scaler = dict(init_scale=1024.0, mode='dynamic') if clover_amd._lib.HALF_F16 else None
    eng = CloverEngine(model, micro[0], lr=5e-5 / 1024 * B * k, weight_decay=0.005, grad_clip=15.0, max_iters=100000,
                       loss_scale=scaler, virtual_ranks=k)
    feed = micro[0] if k == 1 else micro
    eng.step(feed)
    eng.capture(micro[0])
    for _ in range(args.warmup):
        eng.step(feed)
    torch.cuda.synchronize()
    skipped0 = ops.optim_state_read(eng.optim_state)['skipped']
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = eng.step(feed)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    res = dict(leg='step', k=k, B=B, steps=args.steps, step_ms=round(dt / args.steps * 1e3, 3),
               pairs_per_s=round(k * B * args.steps / dt, 2), loss=float(out['log_vars']['loss']),
               steps_skipped=ops.optim_state_read(eng.optim_state)['skipped'] - skipped0,
               peak_mem_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))
    if k == 1:
        eng.start_phase_timing()
        for _ in range(args.steps):
            eng.step(feed)
        torch.cuda.synchronize()
        res['phases_ms'] = {n: round(v, 3) for n, v in eng.phase_ms().items()}
    print(json.dumps(res))


def child(argv, limit):
    """One GPU leg under its own time limit -> its JSON line, or a dict that says how it ended."""
    cmd = ['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__)] + argv
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        return dict(failed=argv, exit=r.returncode, stderr=r.stderr[-2000:])
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', choices=['loss', 'step'], default=None)
    ap.add_argument('--leg', choices=['loss', 'step'], default=None, help=argparse.SUPPRESS)
    ap.add_argument('--G', type=int, nargs='+', default=list(LOSS_G))
    ap.add_argument('--ks', type=int, nargs='+', default=list(STEP_K))
    ap.add_argument('--k', type=int, default=1, help=argparse.SUPPRESS)
    ap.add_argument('--samples', type=int, default=20)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None, help='also write the JSON object to this file')
    args = ap.parse_args()
    if args.leg == 'loss':
        return leg_loss(args)
    if args.leg == 'step':
        return leg_step(args)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('tools/virtual_ranks_bench.py needs an MI355X (no CPU fallback)')
    res, ok = {}, True
    if args.only in (None, 'loss'):
        res['loss'] = child(['--leg', 'loss', '--samples', str(args.samples), '--G'] + [str(g) for g in args.G], 240)
        ok = 'failed' not in res['loss']
    if ok and args.only in (None, 'step'):
        res['step'] = []
        for k in args.ks:
            r = child(['--leg', 'step', '--k', str(k), '--steps', str(args.steps), '--warmup', str(args.warmup)], 300)
            res['step'].append(r)
            if 'failed' in r:
                ok = False
                break
        base = res['step'][0]
        if ok and base.get('k') == 1 and base.get('phases_ms'):
            ph = base['phases_ms']
            F, Bw, L, O = ph.get('forward', 0.0), ph.get('backward', 0.0), ph.get('loss', 0.0), ph.get('optimizer', 0.0)
            for r in res['step']:
                k = r['k']
                model_ms = k * (F + Bw) + (k - 1) * F + L + O
                r['model_step_ms'] = round(model_ms, 3)
                r['model_pairs_per_s'] = round(k * r['B'] / model_ms * 1e3, 2)
    res['ok'] = ok
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    print(line)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
