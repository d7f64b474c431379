"""Window attention beyond 448 tokens (csrc/attention.hip: a window run as P parts of at most 25 staged tiles, template MODE 2)
through ops.window_attention, forward and backward with the relative-position-table gradient.

The method is tests/test_attention_gpu.py's, unchanged: the kernels are held to RMS_MARGIN / SLICE_MARGIN times the error of
a FLOOR reference (fp64 arithmetic, a 16-bit round trip wherever the kernels store one) against the exact fp64 reference,
per tensor and per (group, head) slice, with the same DEGENERATE_SLICE rule (hold_to_floor).  The floor of a window in parts
is tests/window_ref.py attn_core_nparts.  Measured ratios: tests/WINDOW_LARGE_ERROR_BUDGET.md.
"""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from clover_amd import _lib                                                           # noqa: E402
from test_attention_gpu import DEV, HALF, half_rt, hold_to_floor, ident, ops, rnd     # noqa: E402
from window_ref import LargeWindowGeom, attn_core_nparts, part_plan                   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (B, D, H, W, C, nH, table window, configured shift, with a table); the effective window / shift follow from the
# grid as in the model (get_window_size): a window extent that covers the grid is clipped to it and its shift zeroed
CASES = {
    'a': (2, 16, 7, 7, 64, 2, (16, 7, 7), (0, 0, 0), True),       # 784 tokens, 49 tiles, 2 parts of 25 + 24: the headline case
    'b': (1, 32, 14, 7, 64, 2, (16, 7, 7), (8, 3, 3), True),      # four windows, effective shift (8, 3, 0): mask across parts
    'c': (1, 10, 7, 7, 64, 2, (10, 7, 7), (0, 0, 0), True),       # 490 tokens, 31 tiles: pad keys in the last tile
    'd': (1, 10, 10, 10, 32, 2, (5, 10, 10), (2, 5, 5), True),    # 500 tokens, hd 16, effective shift (2, 0, 0)
    'e': (1, 12, 7, 7, 64, 2, (16, 7, 7), (0, 0, 0), True),       # 588 tokens clipped under a (16, 7, 7) table: the band
    'f': (1, 8, 8, 8, 128, 2, (8, 8, 8), (0, 0, 0), True),        # 512 tokens, exact tiles, hd 64
    'g': (1, 16, 8, 8, 64, 2, (16, 8, 8), (0, 0, 0), True),       # 1024 tokens: the bound, 3 parts of 22 + 22 + 20 tiles
    'h': (2, 16, 7, 7, 64, 2, (16, 7, 7), (0, 0, 0), False),      # case a without a table and without a mask
    'i': (1, 2, 30, 15, 32, 2, (2, 15, 15), (0, 7, 7), True),     # 450 tokens, 29 tiles: parts of 15 tiles on the 16-tile kernels
}
EXPECT = {      # name -> (window, shift, N, hd, groups, (parts, part tokens, instantiation))
    'a': ((16, 7, 7), (0, 0, 0), 784, 32, 2, (2, 400, 25)), 'b': ((16, 7, 7), (8, 3, 0), 784, 32, 4, (2, 400, 25)),
    'c': ((10, 7, 7), (0, 0, 0), 490, 32, 1, (2, 256, 16)), 'd': ((5, 10, 10), (2, 0, 0), 500, 16, 2, (2, 256, 16)),
    'e': ((12, 7, 7), (0, 0, 0), 588, 32, 1, (2, 304, 25)), 'f': ((8, 8, 8), (0, 0, 0), 512, 64, 1, (2, 256, 16)),
    'g': ((16, 8, 8), (0, 0, 0), 1024, 32, 1, (3, 352, 25)), 'h': ((16, 7, 7), (0, 0, 0), 784, 32, 2, (2, 400, 25)),
    'i': ((2, 15, 15), (0, 7, 0), 450, 16, 2, (2, 240, 16)),
}
_REF = {}


def case_inputs(name):
    """Geometry, seeded inputs and both references of a case: computed once, shared by the tests, never modified."""
    if name not in _REF:
        B, D, H, W, Cc, nH, tw, cfg_ss, with_table = CASES[name]
        wg = LargeWindowGeom(B, D, H, W, Cc, nH, tw, cfg_ss)
        ws, ss, N, hd, groups, plan = EXPECT[name]
        assert (tuple(wg.ws), tuple(wg.ss), wg.N, wg.hd, wg.groups, wg.plan) == (ws, ss, N, hd, groups, plan)
        seed = 40 + 10 * sorted(CASES).index(name)
        qkv = rnd(B, D, H, W, 3 * Cc, seed=seed + 1).to(HALF)
        table = rnd(wg.rows, nH, scale=0.5, seed=seed + 2) if with_table else None
        do = rnd(B, D, H, W, Cc, seed=seed + 3).to(HALF)
        exact = wg.reference(qkv, table, do, ident, parts=False)
        floor = wg.reference(qkv, table, do, half_rt)
        for d in (exact, floor):
            if with_table:
                d['dtable'] = d['dtable'].t().unsqueeze(0)           # [1, nH, rows]: one slice per head
        _REF[name] = (wg, qkv, table, do, exact, floor)
    return _REF[name]


def check_plan(wg, with_table):
    """The dispatch the case is there for, read back from the C ABI."""
    L = _lib.lib()
    g = wg.clv_geom(table=with_table)
    P, pt, _ = wg.plan
    assert (L.clv_attn_seq_parts(C.byref(g)), L.clv_attn_part_tokens(C.byref(g))) == (P, pt)
    assert L.clv_attn_seq_work_bytes(C.byref(g)) > 0


def run_window(name, wg, qkv, table, do):
    """-> (got dict in window layout, the raw dqkv) of one forward + backward through ops.window_attention."""
    from clover_amd.backbones.swin_transformer_3d import window_geometry
    B, D, H, W, Cc, nH, tw, cfg_ss, with_table = CASES[name]
    ws, ss, rid = window_geometry((D, H, W), tw, cfg_ss, DEV)
    assert tuple(ws) == tuple(wg.ws) and tuple(ss) == tuple(wg.ss) and (rid is not None) == any(ss)
    qg = qkv.to(DEV, copy=True).requires_grad_()
    tg = table.to(DEV, copy=True).requires_grad_() if table is not None else None
    o = ops().window_attention(qg, tg, rid, ws, ss, nH, table_window=tw)
    o.backward(do.to(DEV))
    torch.cuda.synchronize()
    dq, dk, dv = wg.windows(qg.grad.cpu(), 3)
    got = dict(o=wg.windows(o.detach().cpu(), 1)[0], dq=dq, dk=dk, dv=dv)
    if tg is not None:
        got['dtable'] = tg.grad.cpu().t().unsqueeze(0)
    return got, qg.grad


@pytest.mark.parametrize('name', sorted(CASES))
def test_large_window(name):
    wg, qkv, table, do, exact, floor = case_inputs(name)
    with_table = table is not None
    check_plan(wg, with_table)
    ops().LIBRARY_GEMM_CALLS.clear()
    got, _ = run_window(name, wg, qkv, table, do)
    assert not ops().LIBRARY_GEMM_CALLS, ops().LIBRARY_GEMM_CALLS
    zeros = None
    if with_table:
        # rows of the table the window cannot reach (a clipped window: temporal offsets beyond its depth) get exactly 0
        tw = wg.tw
        assert int(wg.used_rows.sum()) == (2 * wg.ws[0] - 1) * (2 * tw[1] - 1) * (2 * tw[2] - 1)
        if name == 'e':
            assert int((~wg.used_rows).sum()) == 8 * 13 * 13
        zeros = dict(dtable=(~wg.used_rows)[None, None, :].expand(1, wg.nH, wg.rows))
    hold_to_floor(f'large window {name} N={wg.N} hd={wg.hd} groups={wg.groups} shift={tuple(wg.ss)} parts={wg.plan[0]}', got,
                  exact, floor, zeros)


def test_nparts_floor_equals_the_one_part_reference_without_rounding():
    """attn_core_nparts with the identity hook is attn_core for any number of parts; with two parts and the 16-bit hook it is
    attn_core(.., pt=)."""
    from test_attention_gpu import attn_core
    G, nH, N, hd = 2, 2, 72, 16
    q, k, v, do = (rnd(G, nH, N, hd, seed=s).double() for s in (1, 2, 3, 4))
    bias = rnd(1, nH, N, N, scale=0.5, seed=5).double()
    add = lambda g0, g1: bias                                                      # noqa: E731
    one = attn_core(q, k, v, do, hd ** -0.5, add, ident)
    for pt, P in ((48, 2), (32, 3), (16, 5)):
        gen = attn_core_nparts(q, k, v, do, hd ** -0.5, add, ident, pt, P)
        for a, b in zip(gen, one):
            assert ((a - b).abs().max() / b.abs().max()).item() < 1e-10
    two = attn_core(q.to(HALF).double(), k.to(HALF).double(), v.to(HALF).double(), do.to(HALF).double(), hd ** -0.5, add,
                    half_rt, pt=48)
    gen = attn_core_nparts(q.to(HALF).double(), k.to(HALF).double(), v.to(HALF).double(), do.to(HALF).double(), hd ** -0.5,
                           add, half_rt, 48, 2)
    for a, b in zip(gen, two):
        assert ((a - b).abs().max() / b.abs().max()).item() < 1e-12
    assert part_plan(448) == (1, 448, 28) and part_plan(449) == (2, 240, 16) and part_plan(1025) is None


def test_backward_host_forms_agree():
    """Case a's backward through the three host forms of _Attention.backward: eager (stage mask 0 = 7 in one call), the
    deferred gather of a backward segment (15 + clv_attn_dbias_gather_entry, with a gradient sink) and the profiled form
    (1, 2, 4 as separate calls).  dq / dk / dv bit for bit; the table gradient within the floor margin of the exact one (the
    order of the partial sums differs)."""
    name = 'a'
    wg, qkv, table, do, exact, floor = case_inputs(name)
    from clover_amd.backbones.swin_transformer_3d import window_geometry
    B, D, H, W, Cc, nH, tw, cfg_ss, _ = CASES[name]
    ws, ss, rid = window_geometry((D, H, W), tw, cfg_ss, DEV)
    o_ = ops()

    def run(form):
        qg = qkv.to(DEV, copy=True).requires_grad_()
        tg = table.to(DEV, copy=True).requires_grad_()
        if form != 'eager':
            tg._clv_grad = torch.zeros(wg.rows, nH, device=DEV)            # an engine-style gradient sink
            tg._clv_ready = lambda: None
        if form == 'deferred':
            with o_.defer_folds():
                o_.window_attention(qg, tg, rid, ws, ss, nH, table_window=tw).backward(do.to(DEV))
                assert len(o_.SEGMENT.dbias) == 1
        elif form == 'profiled':
            o_.PROF = {}
            try:
                o_.window_attention(qg, tg, rid, ws, ss, nH, table_window=tw).backward(do.to(DEV))
                keys = set(o_.PROF)
            finally:
                o_.PROF = None
            assert keys == {'attn_fwd_kernel<32, 25, false, 2>', 'attn_bwd_dq_kernel<32, 25, false, 2>',
                            'attn_bwd_dkv_kernel<32, 26, false, 2>'}, keys
        else:
            o_.window_attention(qg, tg, rid, ws, ss, nH, table_window=tw).backward(do.to(DEV))
        torch.cuda.synchronize()
        dt = tg.grad if form == 'eager' else tg._clv_grad
        return qg.grad.clone(), dt.detach().clone()
    ref_dqkv, ref_dt = run('eager')
    unused = (~wg.used_rows)[None, None, :].expand(1, nH, wg.rows)
    for form in ('eager', 'deferred', 'profiled'):
        dqkv, dt = run(form)
        assert torch.equal(dqkv, ref_dqkv), form
        hold_to_floor(f'large window a, backward form {form}', dict(dtable=dt.cpu().t().unsqueeze(0)),
                      dict(dtable=exact['dtable']), dict(dtable=floor['dtable']), dict(dtable=unused))


def test_large_window_in_the_bf16_build():
    """Case a in a child process with CLOVER_HALF=bf16, started as tests/test_seq_parts_gpu.py starts its child."""
    env = dict(os.environ, CLOVER_HALF='bf16')
    r = subprocess.run([sys.executable, '-m', 'pytest', '-x', '-q', '-m', 'gpu',
                        'tests/test_window_large_gpu.py::test_large_window[a]'], env=env, capture_output=True, text=True,
                       cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert '1 passed' in r.stdout, r.stdout[-2000:]
