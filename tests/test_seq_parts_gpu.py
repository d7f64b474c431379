"""Sequence attention beyond 896 keys on the own kernels: the P-part form of csrc/attention.hip (mode 0, tiles = ceil(S / 16) >
56: P = ceil(tiles / 28) parts of ceil(tiles / P) * 16 staged tokens, tsplit = P, up to clv_attn_seq_max_keys() = 4096 keys).

The method is tests/test_attention_gpu.py's: the kernels are held to multiples (RMS_MARGIN, SLICE_MARGIN, unchanged) of the
error of a FLOOR reference — fp64 arithmetic with a round trip through the 16-bit type wherever the kernels store one — against
the exact fp64 reference.  `attn_core(.., pt=)` there models two parts; `attn_core_parts` below is its P-part form, first
proved equal to it for P = 2.  The references of these lengths run in fp64 on the device.
"""
import ctypes as C
import os
import subprocess
import sys
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

from clover_amd import _lib                                         # noqa: E402
from test_attention_gpu import (DEV, HALF, LOG2E, NKTS, half_rt, hold_to_floor, ident, ops, rnd,    # noqa: E402
                                seq_reference)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_KEYS = 4096


def predict_parts(S):
    """(nkt, tsplit, nparts) of a long sequence as attention.hip's make_geom / pick_nkt choose them: P = ceil(tiles / 28),
    parts of ceil(tiles / P) tiles, tsplit = P, the smallest instantiated tile count that holds a part."""
    tiles = (S + 15) // 16
    assert 28 < tiles and S <= MAX_KEYS
    P = (tiles + 27) // 28
    need = (tiles + P - 1) // P
    return next(o for o in NKTS if o >= need), P, P


def part_tokens(S):
    tiles = (S + 15) // 16
    P = (tiles + 27) // 28
    return (tiles + P - 1) // P * 16, P


def geom(B, S, nH, hd, p=0.0):
    Hd = nH * hd
    return _lib.ClvAttnGeom(mode=0, groups=B, N=S, nH=nH, hd=hd, ldq=3 * Hd, ldk=3 * Hd, ldv=3 * Hd, ldo=Hd, scale=hd ** -0.5,
                            dropout_p=p)


# ----------------------------------------------------------------------------- the P-part floor reference
def attn_core_parts(q, k, v, do, scale, add, r, pt, nparts):
    """tests/test_attention_gpu.py attn_core(.., pt=) with `nparts` parts of `pt` tokens (the last one shorter): the hook r is
    applied to each part's stored contribution — o_p, dq_p (key parts), dk_p, dv_p (query parts) — and to the merged value,
    as seq_combine_fwd_kernel / seq_combine_bwd_kernel round them.  The parts are summed in ascending order, as the
    kernels' `for p < G.nparts` loops do.  -> o, dq, dk, dv [G, nH, N, hd]."""
    G, nH, N, hd = q.shape
    o, dq, dk, dv = (torch.empty_like(q) for _ in range(4))
    step = max(1, (1 << 24) // (nH * N * N))
    parts = [slice(i * pt, min(N, (i + 1) * pt)) for i in range(nparts)]
    assert parts[-1].start < N and parts[-1].stop == N
    T = lambda x: x.transpose(-1, -2)                                   # noqa: E731
    for g0 in range(0, G, step):
        s = slice(g0, min(G, g0 + step))
        S = scale * (q[s] @ T(k[s])) + add(s.start, s.stop)
        P = S.softmax(-1)
        O = r(sum(P[..., p].sum(-1, keepdim=True) * r(r(S[..., p].softmax(-1)) @ v[s][:, :, p]) for p in parts))
        delta = (do[s] * O).sum(-1, keepdim=True)
        dP = do[s] @ T(v[s])
        dS = r(P * (dP - delta))
        qs = r(q[s] * (scale * LOG2E)) / LOG2E
        Pkv = (qs @ T(k[s]) + add(s.start, s.stop) - S.logsumexp(-1, keepdim=True)).exp()
        dSkv, Pkvr = r(Pkv * (dP - delta)), r(Pkv)
        o[s] = O
        dq[s] = r(sum(r(scale * (dS[..., p] @ k[s][:, :, p])) for p in parts))
        dk[s] = r(sum(r(T(dSkv[:, :, p]) @ qs[:, :, p]) for p in parts))
        dv[s] = r(sum(r(T(Pkvr[:, :, p]) @ do[s][:, :, p]) for p in parts))
    return o, dq, dk, dv


def split_heads(qkv, do, nH):
    B, S, C3 = qkv.shape
    hd = C3 // 3 // nH
    q, k, v = qkv.double().view(B, S, 3, nH, hd).permute(2, 0, 3, 1, 4)
    return q, k, v, do.double().view(B, S, nH, hd).permute(0, 2, 1, 3), hd


def parts_reference(qkv, kmask, do, nH, r, pt, nparts):
    q, k, v, dow, hd = split_heads(qkv, do, nH)
    km = kmask.double()
    o, dq, dk, dv = attn_core_parts(q, k, v, dow, hd ** -0.5, lambda g0, g1: km[g0:g1, None, None, :], r, pt, nparts)
    return dict(o=o, dq=dq, dk=dk, dv=dv)


def test_parts_reference_equals_two_part_reference():
    """attn_core_parts with P = 2 is attn_core(.., pt=): with the identity hook and with the 16-bit round trip."""
    B, S, nH, hd, pt = 3, 72, 2, 16, 48
    qkv, do = rnd(B, S, 3 * nH * hd, seed=4, device=DEV).to(HALF), rnd(B, S, nH * hd, seed=5, device=DEV).to(HALF)
    keep = torch.ones(B, S, device=DEV)
    keep[0, 17:] = 0
    keep[1, 20:53] = 0
    kmask = (1.0 - keep) * -10000.0
    for r in (ident, half_rt):
        two = seq_reference(qkv, kmask, do, nH, r, pt)
        gen = parts_reference(qkv, kmask, do, nH, r, pt, 2)
        for name in two:
            d = ((gen[name] - two[name]).abs().max() / two[name].abs().max()).item()
            assert d < 1e-10, (r.__name__, name, d)
    one = seq_reference(qkv, kmask, do, nH, ident)                      # without rounding three parts are the same function
    gen = parts_reference(qkv, kmask, do, nH, ident, 32, 3)
    for name in one:
        assert ((gen[name] - one[name]).abs().max() / one[name].abs().max()).item() < 1e-10, name


# ----------------------------------------------------------------------------- dispatch
def test_max_keys():
    assert _lib.lib().clv_attn_seq_max_keys() == MAX_KEYS
    assert ops().SEQ_FUSED_MAX_KEYS == MAX_KEYS


@pytest.mark.parametrize('S,parts', [(448, 1), (449, 2), (896, 2), (897, 3), (1344, 3), (1345, 4), (1600, 4), (4096, 10),
                                     (4097, 0)])
def test_parts_dispatch(S, parts):
    L = _lib.lib()
    B, nH, hd = 2, 2, 64
    g = geom(B, S, nH, hd)
    assert L.clv_attn_seq_parts(C.byref(g)) == parts
    wb = L.clv_attn_seq_work_bytes(C.byref(g))
    assert (wb > 0) == (parts > 1)
    if parts > 1:                 # [part][o] + [part][lse] forward, [part][dq | dk | dv][tokens][C] backward: the larger
        tc = B * S * nH * hd
        assert wb == max(parts * (tc * 2 + B * nH * S * 4), parts * 3 * tc * 2)


# ----------------------------------------------------------------------------- accuracy
def parts_keep(S, full=True):
    """One sample per mask pattern: no masked key; valid length 17; valid length 1; keys 20..52 masked; valid keys ending 5
    before the end of part 0 (parts 1..P-1 fully masked); valid keys ending inside the first tile of the last part.
    full=False: the first and the fifth only."""
    pt16, P = part_tokens(S)
    rows = [torch.ones(S)]
    for n in (17, 1):
        v = torch.zeros(S)
        v[:n] = 1
        rows.append(v)
    v = torch.ones(S)
    v[20:53] = 0
    rows.append(v)
    v = torch.zeros(S)
    v[:pt16 - 5] = 1
    rows.append(v)
    v = torch.zeros(S)
    assert (P - 1) * pt16 + 7 <= S
    v[:(P - 1) * pt16 + 7] = 1
    rows.append(v)
    return torch.stack(rows if full else [rows[0], rows[4]])


def run_parts_case(keep, nH, hd, seed, expect):
    B, S = keep.shape
    Hd = nH * hd
    nkt, tsplit, nparts = expect
    assert predict_parts(S) == (nkt, tsplit, nparts)
    g = geom(B, S, nH, hd)
    assert _lib.lib().clv_attn_seq_parts(C.byref(g)) == nparts
    # the launch names carry the instantiation of the PART (the dK / dV kernel runs the next even tile count)
    assert ops()._kname('attn_fwd_kernel', g) == f'attn_fwd_kernel<{hd}, {nkt}, false, 0>'
    assert ops()._kname('attn_bwd_dkv_kernel', g) == f'attn_bwd_dkv_kernel<{hd}, {(nkt + 1) & ~1}, false, 0>'
    pt16, P = part_tokens(S)
    assert P == nparts and pt16 <= nkt * 16
    keep = keep.to(DEV)
    qkv = rnd(B, S, 3 * Hd, seed=seed, device=DEV).to(HALF)
    do = rnd(B, S, Hd, seed=seed + 1, device=DEV).to(HALF)
    kmask = ((1.0 - keep) * -10000.0).float().contiguous()
    exact = seq_reference(qkv, kmask, do, nH, ident)
    floor = parts_reference(qkv, kmask, do, nH, half_rt, pt16, nparts)
    qg = qkv.clone().requires_grad_()
    o = ops().seq_attention(qg, kmask, nH)
    o.backward(do)
    torch.cuda.synchronize()
    dq, dk, dv = qg.grad.view(B, S, 3, nH, hd).permute(2, 0, 3, 1, 4)
    got = dict(o=o.detach().view(B, S, nH, hd).permute(0, 2, 1, 3), dq=dq, dk=dk, dv=dv)
    masked = (keep == 0)[:, None, :, None].expand(B, nH, S, hd)
    zeros = dict(dk=masked, dv=masked) if masked.any() else None
    hold_to_floor(f'seq S={S} hd={hd} pairs={B * nH} nkt={nkt} tsplit={tsplit} parts={nparts}', got, exact, floor, zeros)


# 897: the first 3-part length, the last tile holds one key; 1344: three full parts, looped tiles = 28 * 3 exactly; 1345: one
# key beyond; 1600: the 64-frame fusion sequence; 4096: the maximum
PART_LENGTHS = [(897, 25, 3, 3), (1344, 28, 3, 3), (1345, 25, 4, 4), (1600, 25, 4, 4), (4096, 28, 10, 10)]


@pytest.mark.parametrize('S,nkt,tsplit,nparts', PART_LENGTHS)
def test_parts_lengths(S, nkt, tsplit, nparts):
    run_parts_case(parts_keep(S, full=S < MAX_KEYS), 2, 64, 500 + S, (nkt, tsplit, nparts))


@pytest.mark.parametrize('hd', [32, 16])
def test_parts_head_sizes(hd):
    run_parts_case(parts_keep(897), 2, hd, 600 + hd, (25, 3, 3))


@pytest.mark.parametrize('B,nH', [(1, 2), (16, 12)])
def test_parts_few_and_many_pairs(B, nH):
    """S = 1030 (3 parts): grids of P^2 = 9 workgroups per (sample, head) with 2 and with 192 pairs."""
    base = parts_keep(1030)
    keep = base[(torch.arange(B) + 3) % base.shape[0]]
    run_parts_case(keep, nH, 64, 700 + B, (25, 3, 3))


# ----------------------------------------------------------------------------- dropout
@pytest.mark.parametrize('S', [1030, 2100])
def test_parts_dropout_equals_unfused_path(S, monkeypatch):
    """The dropout mask is the hash of (seed, group, head, query row, GLOBAL key index) whatever the number of parts, so for
    one seed ops.seq_attention (three parts at S = 1030) equals the unfused GEMM + row-softmax path, which materialises the same mask:
    forward and the q / k / v gradients, with a key mask on one sample.  The bounds are those of
    test_split_seq_attention_dropout_equals_unfused_path.  S = 2100 (five parts): the unfused path's row-softmax kernels walk rows
    of more than 2048 keys from memory (softmax.hip *_stream_kernel), forward and backward, with the same mask hash."""
    o_ = ops()
    B, nH, hd, pdrop = 2, 4, 64, 0.2
    Hd = nH * hd
    seed = torch.tensor([1234567], device=DEV, dtype=torch.int64)
    qkv = rnd(B, S, 3 * Hd, seed=141, device=DEV).to(HALF)
    do = rnd(B, S, Hd, seed=142, device=DEV).to(HALF)
    km = torch.zeros(B, S, device=DEV)
    km[1, S - 50:] = -10000.0
    q1 = qkv.clone().requires_grad_()
    calls = dict(o_.LIBRARY_GEMM_CALLS)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        o1 = o_._LongSeqAttention.apply(q1, km, nH, pdrop, seed)
    o1.backward(do)
    o_.LIBRARY_GEMM_CALLS.clear()
    o_.LIBRARY_GEMM_CALLS.update(calls)                                 # the direct call above is not a finding
    monkeypatch.setattr(o_, 'next_dropout_seed', lambda device: seed)
    q2 = qkv.clone().requires_grad_()
    o2 = o_.seq_attention(q2, km, nH, dropout_p=pdrop)
    o2.backward(do)
    assert o_.LIBRARY_GEMM_CALLS == calls                               # the own kernels ran
    rel = lambda a, b: ((a.float() - b.float()).abs().max() / b.float().abs().max()).item()      # noqa: E731
    print(f'dropout S={S}: o', rel(o2, o1), 'dqkv', rel(q2.grad, q1.grad))
    assert rel(o2, o1) < 2e-2, rel(o2, o1)
    assert rel(q2.grad, q1.grad) < 3e-2, rel(q2.grad, q1.grad)


# ----------------------------------------------------------------------------- strict mode, beyond the maximum
@pytest.mark.usefixtures('strict_own_gemm')
@pytest.mark.parametrize('S', [1030, 1600])
def test_parts_run_in_strict_mode(S):
    B, nH, hd = 2, 12, 64
    qg = rnd(B, S, 3 * nH * hd, seed=150 + S, device=DEV).to(HALF).requires_grad_()
    km = torch.zeros(B, S, device=DEV)
    km[0, S - 37:] = -10000.0
    o = ops().seq_attention(qg, km, nH)
    o.backward(rnd(B, S, nH * hd, seed=151, device=DEV).to(HALF))
    torch.cuda.synchronize()
    assert torch.isfinite(o).all() and torch.isfinite(qg.grad).all()
    assert not ops().LIBRARY_GEMM_CALLS


def test_beyond_the_maximum_is_the_counted_refused_path(monkeypatch):
    o_ = ops()
    B, S, nH, hd = 1, 4100, 1, 16
    g = geom(B, S, nH, hd)
    assert _lib.lib().clv_attn_seq_parts(C.byref(g)) == 0
    qkv = rnd(B, S, 3 * nH * hd, seed=160, device=DEV).to(HALF)
    saved = dict(o_.LIBRARY_GEMM_CALLS)
    o_.LIBRARY_GEMM_CALLS.clear()
    try:
        monkeypatch.delenv('CLOVER_STRICT_OWN_GEMM', raising=False)
        qg = qkv.clone().requires_grad_()
        with pytest.warns(RuntimeWarning, match='ROCm library GEMM'):
            o = o_.seq_attention(qg, None, nH)
        o.backward(torch.ones_like(o))
        torch.cuda.synchronize()
        assert torch.isfinite(o).all() and torch.isfinite(qg.grad).all()
        qr = qkv.float().requires_grad_()                               # and computes attention: against fp32 torch
        q, k, v = qr.view(B, S, 3, nH, hd).permute(2, 0, 3, 1, 4)
        o_ref = ((q @ k.transpose(-1, -2) / hd ** 0.5).softmax(-1) @ v).permute(0, 2, 1, 3).reshape(B, S, nH * hd)
        o_ref.backward(torch.ones_like(o_ref))
        rel = lambda a, b: ((a.float() - b).abs().max() / b.abs().max()).item()      # noqa: E731
        assert rel(o, o_ref) < 2e-2 and rel(qg.grad, qr.grad) < 3e-2, (rel(o, o_ref), rel(qg.grad, qr.grad))
        assert [k for k in o_.LIBRARY_GEMM_CALLS if k[0].startswith('seq_attention') and k[1] == (B, nH, S, hd)]
        monkeypatch.setenv('CLOVER_STRICT_OWN_GEMM', '1')
        with pytest.raises(RuntimeError, match='CLV_ERR_UNSUPPORTED'):
            o_.seq_attention(qkv, None, nH)
    finally:
        o_.LIBRARY_GEMM_CALLS.clear()
        o_.LIBRARY_GEMM_CALLS.update(saved)


# ----------------------------------------------------------------------------- the bf16 build
@pytest.mark.skipif(os.environ.get('CLOVER_HALF', 'f16').lower() == 'bf16', reason='this process already runs the bf16 build')
def test_parts_in_the_bf16_build():
    """One case (S = 897, hd = 64) in a child process with CLOVER_HALF=bf16, started as tests/test_bf16_build_gpu.py does."""
    env = dict(os.environ, CLOVER_HALF='bf16')
    r = subprocess.run([sys.executable, '-m', 'pytest', '-x', '-q', '-m', 'gpu', 'tests/test_seq_parts_gpu.py', '-k',
                        'test_parts_lengths and 897'], env=env, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert '1 passed' in r.stdout, r.stdout[-2000:]
