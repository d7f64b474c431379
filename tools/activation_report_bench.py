#!/usr/bin/env python
"""Cost of the activation report at the bench's shapes (the model of configs/pretrain_synthetic.py, B = 8, 8 frames, 32 tokens):
TWO engines in one process, built alike but for activation_report, each with its own copy of the model and its own captured
step, timed in interleaved windows; what the switch adds to a step (launches, bytes scanned); and one clv_act_report over a
tensor of the largest watched output's size, as GB/s.  Results: profiles/activation_report.txt.

    python tools/activation_report_bench.py"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
import clover_amd  # noqa: E402
from clover_amd import ops  # noqa: E402
from clover_amd.engine import CloverEngine  # noqa: E402


def say(s):
    print(s, flush=True)


dev = torch.device('cuda', 0)
models = {}
for on in (False, True):                       # the same seed: two copies of the same weights
    torch.manual_seed(1234)
    models[on] = clover_amd.build_model(bench.model_cfg('T', 8)).to(dev)
    models[on].train()
batch0 = {k: v.to(dev) for k, v in bench.synthetic_batch(8, 8, 32, 1000).items()}

# every scan the engine issues while it captures the forward graph = the launches a replay holds
scans = []
real_scan = ops.act_report


def counting_scan(t, slot_view):
    if torch.cuda.is_current_stream_capturing():
        scans.append((t.numel(), t.element_size(), str(t.dtype)))
    real_scan(t, slot_view)


ops.act_report = counting_scan
eng, batch = {}, {}
for on in (False, True):
    eng[on] = CloverEngine(models[on], batch0, lr=5e-5 / 1024 * 8, weight_decay=0.005, grad_clip=15.0, max_iters=100000,
                           loss_scale=dict(init_scale=1024.0, mode='dynamic'), overflow_report=True, activation_report=on)
    eng[on].step(batch0)
    assert eng[on].capture(batch0)
    batch[on] = eng[on].input_buffers()
    for _ in range(10):
        eng[on].step(batch[on])
ops.act_report = real_scan
torch.cuda.synchronize()
act = eng[True]._act
nbytes = sum(n * e for n, e, _ in scans)
say(f'watched modules {len(act.names)} (of {len(act.watched)} hooked), scans per forward graph {len(scans)}, '
    f'bytes scanned per step {nbytes} ({nbytes / 1e6:.1f} MB)')
say(f'added launches per step: {len(scans)} scans in the forward graph + 1 eager clear of the table + 1 latch behind '
    f'clv_optim_prep = {len(scans) + 2}')


def timed(e, b, steps=30):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        e.step(b)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


res = {False: [], True: []}
for rnd in range(4):
    for on in (False, True):
        res[on].append(timed(eng[on], batch[on]))
med = {}
for on in (False, True):
    v = sorted(res[on])
    med[on] = (v[1] + v[2]) / 2
    say(f'step, activation_report {"on " if on else "off"}: ms per step over 4 interleaved rounds of 30: '
        + ' '.join(f'{x:.3f}' for x in res[on]) + f'  | median {v[1]:.3f} .. {v[2]:.3f}')
say(f'added time per step: {med[True] - med[False]:+.3f} ms ({(med[True] / med[False] - 1) * 100:+.2f} %)')
for on in (False, True):
    st = eng[on].step_stats()
    say(f'activation_report {"on " if on else "off"}: skipped in all steps {st["skipped"]} (taken {st["t"]})')

# the headroom view after the last step: the five outputs closest to the limit
stats = eng[True].activation_stats()
top = sorted(stats['rows'], key=lambda r: -r[4])[:5]
say(f'limit {stats["limit"]:g}; largest finite outputs: ' + '; '.join(f'{r[0]} {r[4]:.4g}' for r in top))
assert all(r[3] == 0 for r in stats['rows'])

# one clv_act_report over a tensor like the largest watched one
numel, esize, dtype = max(scans, key=lambda s: s[0] * s[1])
x = torch.randn(numel, device=dev).to(ops.BF16 if esize == 2 else torch.float32)
live, _ = ops.act_report_new(1, dev)
ev = []
for rep in range(12):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    ops.act_report(x, live[0])
    b.record()
    ev.append((a, b))
torch.cuda.synchronize()
us = sorted(a.elapsed_time(b) * 1e3 for a, b in ev[2:])
say(f'clv_act_report over the largest watched tensor ({numel} x {dtype}, {numel * esize / 1e6:.1f} MB): {us[len(us) // 2]:.1f} us '
    f'(median of 10; min {us[0]:.1f}, max {us[-1]:.1f}) = {numel * esize / (us[len(us) // 2] * 1e-6) / 1e9:.0f} GB/s')
small = torch.randn(4096, device=dev).to(ops.BF16)
ev = []
for rep in range(12):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    ops.act_report(small, live[0])
    b.record()
    ev.append((a, b))
torch.cuda.synchronize()
us = sorted(a.elapsed_time(b) * 1e3 for a, b in ev[2:])
say(f'clv_act_report over 4096 elements (the launch alone, eager): {us[len(us) // 2]:.1f} us')
