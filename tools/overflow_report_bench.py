#!/usr/bin/env python
"""Cost of the overflow report at the bench's shapes (the model of configs/pretrain_synthetic.py, B = 8, 8 frames, 32 tokens):
the captured step with the switch off and on — ONE engine built with overflow_report=True whose switch is flipped between
interleaved windows, so both legs share weights, graphs and clocks —, the two launches alone on a record that says "taken"
and on one that says "skipped", and the eager optimizer part of a skipped step.  Results: profiles/overflow_report.txt.

    python tools/overflow_report_bench.py"""
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
torch.manual_seed(1234)
model = clover_amd.build_model(bench.model_cfg('T', 8)).to(dev)
model.train()
batch = {k: v.to(dev) for k, v in bench.synthetic_batch(8, 8, 32, 1000).items()}
eng = CloverEngine(model, batch, lr=5e-5 / 1024 * 8, weight_decay=0.005, grad_clip=15.0, max_iters=100000,
                   loss_scale=dict(init_scale=1024.0, mode='dynamic'), overflow_report=True)
eng.step(batch)
assert eng.capture(batch)
batch = eng.input_buffers()
for _ in range(10):
    eng.step(batch)
torch.cuda.synchronize()
tabs = eng._grad_report_tables()
say(f'parameters {eng.num_params}, slabs {[sg.flat_g.numel() for sg in eng.segments]}, '
    f'report blocks {[t.n_chunks for t in tabs]}, report parameters {[t.n_params for t in tabs]}')


def timed(steps=30):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.step(batch)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


res = {False: [], True: []}
for rnd in range(4):
    for on in (False, True):
        eng._overflow_report = on
        res[on].append(timed())
for on in (False, True):
    say(f'step, switch {"on " if on else "off"}: ms per step over 4 interleaved rounds of 30: '
        + ' '.join(f'{v:.3f}' for v in res[on]) + f'  | median {sorted(res[on])[len(res[on]) // 2 - 1]:.3f} .. {sorted(res[on])[len(res[on]) // 2]:.3f}')
st = eng.step_stats()
say(f'skipped in the timed steps: {st["skipped"]} (taken {st["t"]})')

# the two launches alone, on a state that says "taken" (what every enabled step pays) and on one that says "skipped"
state = eng.optim_state.clone()
outs = [ops.grad_report_new(t, dev) for t in tabs]
grads = [sg.flat_g for sg in eng.segments]
for skip in (0, 1):
    state[4] = skip
    ev = []
    for rep in range(12):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for g, t, o in zip(grads, tabs, outs):
            ops.grad_report(g, t, state, o, 0)
        b.record()
        ev.append((a, b))
    torch.cuda.synchronize()
    us = sorted(a.elapsed_time(b) * 1e3 for a, b in ev[2:])
    nbytes = sum(g.numel() * 4 for g in grads)
    say(f'clv_grad_report over all slabs, mode 0, skip = {skip}: {us[len(us) // 2]:.1f} us (median of 10; min {us[0]:.1f}, max {us[-1]:.1f})'
        + (f'  = {nbytes / (us[len(us) // 2] * 1e-6) / 1e12:.2f} TB/s over {nbytes / 1e6:.0f} MB' if skip else ''))
# a whole reporting step: an inf in one slot, then the optimizer step (eager part of the step), with and without the switch
for on in (False, True):
    eng._overflow_report = on
    ev = []
    for rep in range(4):
        eng.forward_backward(batch)
        eng.segments[-1].flat_g[3] = float('inf')
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        eng.optimizer_step()
        b.record()
        torch.cuda.synchronize()
        ev.append(a.elapsed_time(b) * 1e3)
    say(f'optimizer_step of a SKIPPED step, switch {"on " if on else "off"}: us ' + ' '.join(f'{v:.0f}' for v in ev))
eng._overflow_report = True
rep = eng.overflow_report()
say(f'report: skipped {rep["skipped"]}, loss_scale {rep["loss_scale"]}, rows {rep["rows"][:3]}')
