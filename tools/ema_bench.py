#!/usr/bin/env python
"""Cost of the weight EMA on the config-2 model (VideoSwin-T + BERT-base, 8 clips x 8 frames).

    python tools/ema_bench.py                              # ema_update / ema_swap against the framework restatement
    python tools/ema_bench.py --with-step                  # + the captured step with and without the update behind it
    python tools/ema_bench.py --out profiles/ema_update.txt

Prints a small table and ONE JSON line:

* ``ema_update``: one launch for the whole model (slabs + loose tensors), 12 B per parameter (p and ema read, ema written);
* the same arithmetic as ``torch._foreach_mul_(ema, 1 - m)`` + ``torch._foreach_add_(ema, p, alpha=m)`` over the same slabs
  (20 B per parameter: ema read + written, then p and ema read, ema written);
* ``ema_swap``: the kernel alone (16 B per parameter + 2 B per 16-bit copy) and ``engine.ema_swap()`` with the W^T refresh.

Every figure is GPU time between two device events around ``--launches`` back-to-back launches (>= 50) after warm-up, the
median of ``--samples`` such windows; the candidates alternate window by window, in one process on one device.  Rates are
the algorithm's bytes over that time, next to the float4-copy rate of the chip (6.29 TB/s)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE_TBS = 6.29          # measured float4 copy on an MI355X: the streaming rate to hold an elementwise kernel against


def window_ms(fn, launches):
    """GPU milliseconds per call over `launches` back-to-back calls."""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / launches


def alternate(cands, launches, samples, warmup=3):
    """{name: [ms per call, one per window]} with the candidates taking turns."""
    out = {n: [] for n in cands}
    for it in range(warmup + samples):
        for n, fn in cands.items():
            ms = window_ms(fn, launches)
            if it >= warmup:
                out[n].append(ms)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=50, help='launches per timed window (>= 50)')
    ap.add_argument('--samples', type=int, default=7)
    ap.add_argument('--momentum', type=float, default=0.0002)
    ap.add_argument('--with-step', action='store_true', help='also time the captured step without / with ema_update')
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--out', default=None, help='also write the table and the JSON line to this file')
    args = ap.parse_args()
    if args.launches < 50 or args.launches % 2:
        raise SystemExit('--launches: an even number >= 50 (an even count of swaps leaves the weights where they were)')
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('tools/ema_bench.py needs an MI355X (no CPU fallback)')
    import bench
    import clover_amd
    from clover_amd import ops
    from clover_amd.engine import CloverEngine
    dev = torch.device('cuda', 0)
    torch.manual_seed(1234)
    B = 8
    model = clover_amd.build_model(bench.model_cfg('T', 8)).to(dev)
    model.train()
    batch = {n: v.to(dev) for n, v in bench.synthetic_batch(B, 8, 32, 1000).items()}
    scaler = dict(init_scale=1024.0, mode='dynamic') if clover_amd._lib.HALF_F16 else None
    eng = CloverEngine(model, batch, lr=5e-5 / 1024 * B, weight_decay=0.005, grad_clip=15.0, max_iters=100000,
                       loss_scale=scaler)
    eng.ema_enable()
    tab = eng._ema_table
    m = args.momentum
    slabs_p = [sg.flat_p for sg in eng.segments]
    slabs_e = [sg.ema for sg in eng.segments]
    slab_elems = sum(t.numel() for t in slabs_p)

    def ours():
        ops.ema_update(tab, m)

    def foreach():
        torch._foreach_mul_(slabs_e, 1 - m)
        torch._foreach_add_(slabs_e, slabs_p, alpha=m)

    upd = alternate(dict(ema_update=ours, foreach=foreach), args.launches, args.samples)
    swp = alternate(dict(swap_kernel=lambda: ops.ema_swap(tab), engine_swap=eng.ema_swap), args.launches, args.samples)
    assert not eng.ema_swapped
    med = {n: statistics.median(v) for n, v in {**upd, **swp}.items()}
    lo = {n: min(v) for n, v in {**upd, **swp}.items()}
    upd_bytes, fe_bytes = 12 * tab.numel, 20 * slab_elems
    swap_bytes = 16 * tab.numel + 2 * tab.shadow_numel
    rate = lambda nbytes, ms: nbytes / (ms * 1e-3) / 1e12                                        # noqa: E731
    res = dict(model='config 2 (VideoSwin-T + BERT-base, 8 x 8 frames)', half='f16' if clover_amd._lib.HALF_F16 else 'bf16',
               elements=tab.numel, slab_elements=slab_elems, entries=tab.n_entries, blocks=tab.n_blocks,
               launches_per_window=args.launches, windows=args.samples, momentum=m,
               ema_update_ms=round(med['ema_update'], 4), ema_update_min_ms=round(lo['ema_update'], 4),
               ema_update_bytes=upd_bytes, ema_update_tbs=round(rate(upd_bytes, med['ema_update']), 3),
               ema_update_share_of_copy_rate=round(rate(upd_bytes, med['ema_update']) / COPY_RATE_TBS, 3),
               foreach_ms=round(med['foreach'], 4), foreach_min_ms=round(lo['foreach'], 4), foreach_bytes=fe_bytes,
               foreach_tbs=round(rate(fe_bytes, med['foreach']), 3),
               foreach_over_ema_update=round(med['foreach'] / med['ema_update'], 3),
               swap_kernel_ms=round(med['swap_kernel'], 4), swap_kernel_bytes=swap_bytes,
               swap_kernel_tbs=round(rate(swap_bytes, med['swap_kernel']), 3),
               engine_swap_ms=round(med['engine_swap'], 4))
    if args.with_step:
        eng.step(batch)
        eng.capture(batch)
        for _ in range(5):
            eng.step(batch)
            eng.ema_update(m)
        torch.cuda.synchronize()

        def steps(with_ema):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                eng.step(batch)
                if with_ema:
                    eng.ema_update(m)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / args.steps * 1e3
        plain, with_ema = [], []
        for _ in range(args.samples):
            plain.append(steps(False))
            with_ema.append(steps(True))
        res.update(step_ms=round(statistics.median(plain), 3), step_with_ema_ms=round(statistics.median(with_ema), 3),
                   step_ms_spread=[round(min(plain), 3), round(max(plain), 3)],
                   step_with_ema_ms_spread=[round(min(with_ema), 3), round(max(with_ema), 3)], steps_per_window=args.steps)
    lines = [f"weight EMA on {res['model']}, {res['half']} build: {tab.numel} elements in {tab.n_entries} entries / "
             f"{tab.n_blocks} blocks; {args.samples} windows of {args.launches} launches, medians (min)",
             f"  ema_update            {res['ema_update_ms']:8.4f} ms ({res['ema_update_min_ms']:.4f})  {upd_bytes / 1e6:9.1f} MB"
             f"  {res['ema_update_tbs']:.3f} TB/s = {100 * res['ema_update_share_of_copy_rate']:.1f} % of the {COPY_RATE_TBS} TB/s copy rate",
             f"  _foreach_mul_ + _add_ {res['foreach_ms']:8.4f} ms ({res['foreach_min_ms']:.4f})  {fe_bytes / 1e6:9.1f} MB"
             f"  {res['foreach_tbs']:.3f} TB/s   ({res['foreach_over_ema_update']:.2f} x ema_update's time, slabs only)",
             f"  ema_swap kernel       {res['swap_kernel_ms']:8.4f} ms            {swap_bytes / 1e6:9.1f} MB  {res['swap_kernel_tbs']:.3f} TB/s",
             f"  engine.ema_swap()     {res['engine_swap_ms']:8.4f} ms   (kernel + the W^T refresh of every segment)"]
    if args.with_step:
        lines.append(f"  captured step         {res['step_ms']:8.3f} ms {res['step_ms_spread']}   with ema_update behind it "
                     f"{res['step_with_ema_ms']:8.3f} ms {res['step_with_ema_ms_spread']}  ({args.steps} steps per window, host clock)")
    text = '\n'.join(lines) + '\n' + json.dumps(res) + '\n'
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
