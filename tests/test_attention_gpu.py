"""Every dispatch path of csrc/attention.hip against an fp64 reference, bounded by what the 16-bit element type alone costs.

One plain-torch attention (`attn_core`: explicit forward and backward formulas, fp64) is evaluated twice per case: with the
rounding hook r = identity it is the EXACT reference, with r = a round trip through the library's 16-bit type it is the FLOOR.
The kernels are held to multiples of the floor's own error (RMS_MARGIN, SLICE_MARGIN), never to an absolute number, so the same
file serves the fp16 and the bf16 build.  The measured ratios and every rounding the floor models: tests/ATTENTION_ERROR_BUDGET.md.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import indexing as ix          # noqa: E402
from oracle import model as om             # noqa: E402
from clover_amd import _lib                # noqa: E402

DEV = 'cuda'
HALF = _lib.half_dtype()
TABLE_WINDOW = (8, 7, 7)
TABLE_ROWS = 15 * 13 * 13
# kernel error <= margin x floor error.  2: the roundings the emulation does not model (K staged as K.scale.log2e and rounded
# again, exp2 for exp, fp32 for fp64 accumulation).  4: the slice statistic is a maximum over 1e5..1e6 elements, and one more
# 16-bit rounding of an element next to a binade edge doubles it.  Neither may be raised.
RMS_MARGIN, SLICE_MARGIN = 2.0, 4.0
# A (group, head) slice whose exact values are below this fraction of the tensor's maximum is not data but the cancellation
# residue of the reference's own arithmetic (a sample with ONE valid key: P = 1, dS = dP - delta = 0 in exact arithmetic, so
# its dq / dk are 1e-16 in fp64 and 1e-7 in any fp32 kernel); such a slice is normalised by this fraction of the tensor's
# maximum.  Seeded normal inputs put every other slice's maximum within a factor of 3 of the tensor's.
DEGENERATE_SLICE = 1e-3
NKTS = (2, 8, 13, 14, 15, 16, 25, 28)
LOG2E = 1.4426950408889634


def ops():
    from clover_amd import ops as o
    return o


def rnd(*shape, scale=1.0, seed=0, device='cpu'):
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=device) * scale


def ident(t):
    return t


def half_rt(t):
    """Round trip through the library's 16-bit element type (fp16, or bf16 in the bf16 build)."""
    return t.to(HALF).to(t.dtype)


def predict(mode, groups, nH, N):
    """(nkt, tsplit, nparts, table-gradient slices) as attention.hip's make_geom / pick_nkt / dbias_splits choose them."""
    tiles, pairs = (N + 15) // 16, groups * nH
    ts = 1
    while ts < 4 and pairs * ts < 384 and tiles >= 8 * ts:
        ts *= 2
    nparts, need = 1, tiles
    if mode == 0 and 28 < tiles <= 56:
        nparts, need, ts = 2, (tiles + 1) // 2, 2
    nkt = next((o for o in NKTS if o >= need), -1)
    return nkt, ts, nparts, min(32, max(1, groups // 64))


# ----------------------------------------------------------------------------- the reference
def attn_core(q, k, v, do, scale, add, r, pt=None):
    """Attention forward + backward by explicit formulas.  q, k, v, do: [G, nH, N, hd] (fp64); add(g0, g1): the additive term
    (bias + mask) of groups [g0, g1), broadcastable to [g1 - g0, nH, N, N]; r: the rounding hook.
    pt: the two-part sequence path (make_geom: nparts == 2, parts of pt tokens).  Its kernels store every part's o, dq, dk
    and dv in 16 bits and the combine kernels round the merged value again — seq_combine_fwd_kernel `o_part` / `pack2bf(acc..)`,
    seq_combine_bwd_kernel `part` / `pack2bf(acc..)` — so the hook is applied to each part's contribution and to their sum
    (key parts for o and dq, query parts for dk and dv).  With r = identity this is the same function as pt = None.
    -> o, dq, dk, dv [G, nH, N, hd] and the sum of r(dS) over the groups [nH, N, N]."""
    G, nH, N, hd = q.shape
    o, dq, dk, dv = (torch.empty_like(q) for _ in range(4))
    ds_sum = torch.zeros(nH, N, N, dtype=q.dtype, device=q.device)
    step = max(1, (1 << 24) // (nH * N * N))
    parts = [slice(0, N)] if pt is None else [slice(0, pt), slice(pt, N)]
    T = lambda x: x.transpose(-1, -2)
    for g0 in range(0, G, step):
        s = slice(g0, min(G, g0 + step))
        S = scale * (q[s] @ T(k[s])) + add(s.start, s.stop)
        P = S.softmax(-1)
        Pr = r(P)
        if pt is None:
            O = r(Pr @ v[s])
        else:           # o_p = softmax over the part's keys . V_p (stored), weighted by the part's share of the row
            O = r(sum(P[..., p].sum(-1, keepdim=True) * r(r(S[..., p].softmax(-1)) @ v[s][:, :, p]) for p in parts))
        delta = (do[s] * O).sum(-1, keepdim=True)
        dP = do[s] @ T(v[s])
        dS = r(P * (dP - delta))
        # The dK / dV kernels do not read P: they recompute it from Q staged as Q.scale.log2e in 16 bits —
        # attn_bwd_dkv_kernel `stage<HD, NK, true>(row_s, q, ..)`, attn_bwd_one_kernel's staged Q' — against the forward's
        # lse, and contract dS with that Q'.  A probability near 1 (a row with one valid key) then carries the rounding of
        # Q' where r(P) alone is exact.  With r = identity Skv = S and Pkv = P.
        qs = r(q[s] * (scale * LOG2E)) / LOG2E
        Pkv = (qs @ T(k[s]) + add(s.start, s.stop) - S.logsumexp(-1, keepdim=True)).exp()
        dSkv, Pkvr = r(Pkv * (dP - delta)), r(Pkv)
        o[s] = O
        if pt is None:
            dq[s] = r(scale * (dS @ k[s]))
            dk[s] = r(T(dSkv) @ qs)
            dv[s] = r(T(Pkvr) @ do[s])
        else:
            dq[s] = r(sum(r(scale * (dS[..., p] @ k[s][:, :, p])) for p in parts))
            dk[s] = r(sum(r(T(dSkv[:, :, p]) @ qs[:, :, p]) for p in parts))
            dv[s] = r(sum(r(T(Pkvr[:, :, p]) @ do[s][:, :, p]) for p in parts))
        ds_sum += dS.sum(0)
    return o, dq, dk, dv, ds_sum


class WindowGeom:
    """Roll / partition / region mask / table index of one window-attention geometry, from the oracle's helpers."""

    def __init__(self, B, D, H, W, C, nH, cfg_ss):
        self.shape, self.nH, self.hd = (B, D, H, W, C), nH, C // nH
        self.ws, self.ss = ix.get_window_size((D, H, W), TABLE_WINDOW, cfg_ss)
        self.N = self.ws[0] * self.ws[1] * self.ws[2]
        self.nW = (D // self.ws[0]) * (H // self.ws[1]) * (W // self.ws[2])
        self.groups = B * self.nW
        self.idx = torch.from_numpy(ix.relative_position_index(TABLE_WINDOW)[:self.N, :self.N].reshape(-1).copy()).long()
        self.mask = torch.from_numpy(ix.compute_mask(D, H, W, self.ws, self.ss)).double() if any(self.ss) else None
        self.used_rows = torch.zeros(TABLE_ROWS, dtype=torch.bool)
        self.used_rows[self.idx] = True

    def windows(self, x, parts):
        """natural layout [B, D, H, W, parts * C] -> `parts` tensors [groups, nH, N, hd] (roll(-shift) + partition)"""
        ss = self.ss
        if any(ss):
            x = torch.roll(x, shifts=(-ss[0], -ss[1], -ss[2]), dims=(1, 2, 3))
        xw = om._t_window_partition(x, self.ws).reshape(self.groups, self.N, parts, self.nH, self.hd)
        return tuple(xw.permute(2, 0, 3, 1, 4))

    def reference(self, qkv, table, do, r):
        """-> dict of o, dq, dk, dv in window layout and dtable [rows, nH]; on the device of the inputs."""
        dev = qkv.device
        q, k, v = self.windows(qkv.double(), 3)
        dow, = self.windows(do.double(), 1)
        idx = self.idx.to(dev)
        bias = table.double()[idx].reshape(self.N, self.N, self.nH).permute(2, 0, 1)
        mask = self.mask.to(dev) if self.mask is not None else None

        def add(g0, g1):
            if mask is None:
                return bias.unsqueeze(0)
            return bias.unsqueeze(0) + mask[torch.arange(g0, g1, device=dev) % self.nW].unsqueeze(1)
        o, dq, dk, dv, ds_sum = attn_core(q, k, v, dow, self.hd ** -0.5, add, r)
        dtab = torch.zeros(TABLE_ROWS, self.nH, dtype=torch.float64, device=dev)
        dtab.index_add_(0, idx, ds_sum.permute(1, 2, 0).reshape(self.N * self.N, self.nH))
        return dict(o=o, dq=dq, dk=dk, dv=dv, dtable=dtab)

    def clv_geom(self, **kw):
        B, D, H, W, Cc = self.shape
        ws, ss = self.ws, self.ss
        return _lib.ClvAttnGeom(mode=1, groups=self.groups, N=self.N, nH=self.nH, hd=self.hd, D=D, H=H, W=W, wd=ws[0], wh=ws[1],
                                ww=ws[2], sd=ss[0], sh=ss[1], sw=ss[2], ldq=3 * Cc, ldk=3 * Cc, ldv=3 * Cc, ldo=Cc, bwd=8, bwh=7,
                                bww=7, scale=self.hd ** -0.5, dropout_p=0.0, **kw)


def seq_reference(qkv, kmask, do, nH, r, pt=None):
    B, S, C3 = qkv.shape
    hd = C3 // 3 // nH
    q, k, v = qkv.double().view(B, S, 3, nH, hd).permute(2, 0, 3, 1, 4)
    dow = do.double().view(B, S, nH, hd).permute(0, 2, 1, 3)
    km = kmask.double()
    o, dq, dk, dv, _ = attn_core(q, k, v, dow, hd ** -0.5, lambda g0, g1: km[g0:g1, None, None, :], r, pt)
    return dict(o=o, dq=dq, dk=dk, dv=dv)


# ----------------------------------------------------------------------------- the assertions
def _slices(t):
    """[G, nH, ...] -> [G * nH, rest]"""
    return t.reshape(t.shape[0] * t.shape[1], -1)


def rms_err(a, b):
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt().clamp_min(1e-300)).item()


def slice_err(a, b):
    a, b = _slices(a), _slices(b)
    norm = b.abs().amax(1).clamp_min(DEGENERATE_SLICE * b.abs().max())
    return ((a - b).abs().amax(1) / norm).max().item()


OLD_BOUND = dict(o=2e-2)          # tests/test_kernels_gpu.py rel(): beyond it a case is a bug, whatever the floor says


def hold_to_floor(case, got, exact, floor, zeros=None):
    """got / exact / floor: dicts of tensors [G, nH, ...] (the table gradient as [1, nH, rows]).  zeros: {name: bool mask of the
    entries that are structurally zero}.  Prints every figure, then asserts all of them at once."""
    bad = []
    for name, e in exact.items():
        g, f = got[name].to(e.device).double(), floor[name]
        assert g.shape == e.shape, (name, g.shape, e.shape)
        assert torch.isfinite(g).all(), f'{case} {name}: non-finite values'
        fr, kr = rms_err(f, e), rms_err(g, e)
        fs, ks = slice_err(f, e), slice_err(g, e)
        old = ((g - e).abs().max() / e.abs().max()).item()
        print(f'ATTN_BUDGET | {case} | {name} | floor rms {fr:.3e} kernel/floor {kr / fr:.2f} | floor slice {fs:.3e} '
              f'kernel/floor {ks / fs:.2f} | max/max {old:.2e}')
        if kr > RMS_MARGIN * fr:
            bad.append(f'{name}: RMS error {kr:.3e} = {kr / fr:.2f} x floor {fr:.3e} (allowed {RMS_MARGIN})')
        if ks > SLICE_MARGIN * fs:
            bad.append(f'{name}: slice error {ks:.3e} = {ks / fs:.2f} x floor {fs:.3e} (allowed {SLICE_MARGIN})')
        if old > OLD_BOUND.get(name, 3e-2):
            bad.append(f'{name}: max/max {old:.3e} beyond the old bound (kernel/floor RMS {kr / fr:.2f})')
        if zeros and name in zeros:
            z = zeros[name].to(e.device)
            assert (e[z] == 0).all(), f'{case} {name}: the reference is not zero where the test expects it'
            nz = int((g[z] != 0).sum())
            if nz:
                bad.append(f'{name}: {nz} nonzero values (max {g[z].abs().max().item():.3e}) where the reference is exactly 0 '
                           f'(kernel/floor RMS {kr / fr:.2f})')
    assert not bad, f'{case}: ' + '; '.join(bad)


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


# ----------------------------------------------------------------------------- the reference itself
def test_reference_backward_equals_autograd():
    """attn_core's explicit backward (r = identity) against torch autograd of the existing restatements, in fp64."""
    from test_kernels_gpu import ref_window_attention
    B, D, H, W, Cc, nH = 2, 4, 14, 14, 48, 3
    wg = WindowGeom(B, D, H, W, Cc, nH, (4, 3, 3))
    qkv, table, do = rnd(B, D, H, W, 3 * Cc, seed=1).double(), rnd(TABLE_ROWS, nH, scale=0.5, seed=2).double(), \
        rnd(B, D, H, W, Cc, seed=3).double()
    qr, tr = qkv.clone().requires_grad_(), table.clone().requires_grad_()
    o_ref = ref_window_attention(qr, tr, ix.relative_position_index(TABLE_WINDOW), TABLE_WINDOW, (4, 3, 3), nH)
    o_ref.backward(do)
    ex = wg.reference(qkv, table, do, ident)
    dq, dk, dv = wg.windows(qr.grad, 3)
    assert _rel(ex['o'], wg.windows(o_ref.detach(), 1)[0]) < 1e-10
    for name, t in (('dq', dq), ('dk', dk), ('dv', dv), ('dtable', tr.grad)):
        assert _rel(ex[name], t) < 1e-10, (name, _rel(ex[name], t))

    B, S, nH, hd = 3, 40, 2, 16
    qkv, do = rnd(B, S, 3 * nH * hd, seed=4).double(), rnd(B, S, nH * hd, seed=5).double()
    keep = torch.ones(B, S)
    keep[0, 17:] = 0
    keep[1, 20:30] = 0
    ext = om.extended_mask(keep).double()
    qr = qkv.clone().requires_grad_()
    q, k, v = qr.view(B, S, 3, nH, hd).permute(2, 0, 3, 1, 4)
    p = (q @ k.transpose(-1, -2) / hd ** 0.5 + ext).softmax(-1)
    o_ref = (p @ v).permute(0, 2, 1, 3).reshape(B, S, nH * hd)
    o_ref.backward(do)
    ex = seq_reference(qkv, ext.reshape(B, S), do, nH, ident)
    g = qr.grad.view(B, S, 3, nH, hd).permute(2, 0, 3, 1, 4)
    assert _rel(ex['o'], o_ref.detach().view(B, S, nH, hd).permute(0, 2, 1, 3)) < 1e-10
    for i, name in enumerate(('dq', 'dk', 'dv')):
        assert _rel(ex[name], g[i]) < 1e-10, (name, _rel(ex[name], g[i]))
    two = seq_reference(qkv, ext.reshape(B, S), do, nH, ident, pt=16)     # the two-part form without rounding: the same function
    for name in ex:
        assert _rel(two[name], ex[name]) < 1e-10, (name, _rel(two[name], ex[name]))


# ----------------------------------------------------------------------------- sequence mode
def seq_keep(S, nparts):
    """The valid-key masks of one batch, one sample each: none; valid length 17; valid length 1; keys 20..52 masked (tile
    32..47 whole); on the two-part path one more whose valid keys end inside the first part (the second: all masked).
    Lengths too short for a pattern clip it (S = 7: valid length 5, no block; S = 32, 33: the block runs to the end)."""
    rows = [torch.ones(S)]
    v = torch.zeros(S)
    v[:17 if S > 17 else S - 2] = 1
    rows.append(v)
    v = torch.zeros(S)
    v[:1] = 1
    rows.append(v)
    if S > 21:
        v = torch.ones(S)
        v[20:min(53, S)] = 0
        rows.append(v)
    if nparts > 1:
        pt16 = ((S + 15) // 16 + 1) // 2 * 16
        v = torch.zeros(S)
        v[:pt16 - 5] = 1
        rows.append(v)
    return torch.stack(rows)


_SEQ_REF = {}


def run_seq_case(keep, nH, hd, seed, expect):
    B, S = keep.shape
    Hd = nH * hd
    nkt, tsplit, nparts = expect
    assert predict(0, B, nH, S)[:3] == (nkt, tsplit, nparts)
    g = _lib.ClvAttnGeom(mode=0, groups=B, N=S, nH=nH, hd=hd, ldq=3 * Hd, ldk=3 * Hd, ldv=3 * Hd, ldo=Hd, scale=hd ** -0.5,
                         dropout_p=0.0)
    assert (_lib.lib().clv_attn_seq_work_bytes(C.byref(g)) > 0) == (nparts == 2)
    qkv = rnd(B, S, 3 * Hd, seed=seed).to(HALF)
    do = rnd(B, S, Hd, seed=seed + 1).to(HALF)
    kmask = ((1.0 - keep) * -10000.0).float()
    pt = ((S + 15) // 16 + 1) // 2 * 16 if nparts == 2 else None
    exact = seq_reference(qkv, kmask, do, nH, ident)
    floor = seq_reference(qkv, kmask, do, nH, half_rt, pt)
    qg = qkv.to(DEV).requires_grad_()
    o = ops().seq_attention(qg, kmask.to(DEV).contiguous(), nH)
    o.backward(do.to(DEV))
    torch.cuda.synchronize()
    dq, dk, dv = qg.grad.cpu().view(B, S, 3, nH, hd).permute(2, 0, 3, 1, 4)
    got = dict(o=o.detach().cpu().view(B, S, nH, hd).permute(0, 2, 1, 3), dq=dq, dk=dk, dv=dv)
    masked = (keep == 0)[:, None, :, None].expand(B, nH, S, hd)
    zeros = dict(dk=masked, dv=masked) if masked.any() else None
    hold_to_floor(f'seq S={S} hd={hd} pairs={B * nH} nkt={nkt} tsplit={tsplit} parts={nparts}', got, exact, floor, zeros)


SEQ_LENGTHS = [(7, 2, 1, 1), (32, 2, 1, 1), (33, 8, 1, 1), (128, 8, 2, 1), (129, 13, 2, 1), (208, 13, 2, 1), (209, 14, 2, 1),
               (224, 14, 2, 1), (225, 15, 2, 1), (240, 15, 2, 1), (241, 16, 4, 1), (256, 16, 4, 1), (257, 25, 4, 1),
               (400, 25, 4, 1), (401, 28, 4, 1), (448, 28, 4, 1), (449, 15, 2, 2), (895, 28, 2, 2), (896, 28, 2, 2)]


@pytest.mark.parametrize('S,nkt,tsplit,nparts', SEQ_LENGTHS)
def test_seq_lengths(S, nkt, tsplit, nparts):
    """Every instantiated key-tile count at its exact fit and one key beyond, the one-part / two-part switch (448 / 449), the
    largest fused length; per-sample masks (seq_keep)."""
    assert S <= ops().SEQ_FUSED_MAX_KEYS
    run_seq_case(seq_keep(S, nparts), 2, 64, 100 + S, (nkt, tsplit, nparts))


@pytest.mark.parametrize('hd', [32, 16])
@pytest.mark.parametrize('S,nkt,tsplit,nparts', [(33, 8, 1, 1), (225, 15, 2, 1), (449, 15, 2, 2)])
def test_seq_head_sizes(S, nkt, tsplit, nparts, hd):
    run_seq_case(seq_keep(S, nparts), 2, hd, 200 + S + hd, (nkt, tsplit, nparts))


@pytest.mark.parametrize('pairs,tsplit', [(2, 4), (200, 2), (384, 1)])
def test_seq_query_splits(pairs, tsplit):
    """S = 256, hd 16: 4, 2 or 1 workgroups per (sample, head), chosen from B * nH (make_geom)."""
    base = seq_keep(256, 1)
    keep = base[torch.arange(pairs // 2) % base.shape[0]]
    run_seq_case(keep, 2, 16, 300 + pairs, (16, tsplit, 1))


# ----------------------------------------------------------------------------- window mode
_WIN_REF = {}


def window_inputs(case, device='cpu'):
    """Seeded inputs + both references of a window case, computed once and shared by its parametrisations (never modified)."""
    key = (case, device)
    if key not in _WIN_REF:
        B, D, H, W, Cc, nH, shifted = case
        wg = WindowGeom(B, D, H, W, Cc, nH, (4, 3, 3) if shifted else (0, 0, 0))
        qkv = rnd(B, D, H, W, 3 * Cc, seed=11, device=device).to(HALF)
        table = rnd(TABLE_ROWS, nH, scale=0.5, seed=12, device=device)
        do = rnd(B, D, H, W, Cc, seed=13, device=device).to(HALF)
        exact = wg.reference(qkv, table, do, ident)
        floor = wg.reference(qkv, table, do, half_rt)
        for d in (exact, floor):
            d['dtable'] = d['dtable'].t().unsqueeze(0)           # [1, nH, rows]: one slice per head
        _WIN_REF[key] = (wg, qkv, table, do, exact, floor)
    return _WIN_REF[key]


def window_expectations(wg, bwd_one_env=None):
    """The dispatch the case is there for, read back from the C ABI where it is exposed."""
    L = _lib.lib()
    nkt, tsplit, nparts, splits = predict(1, wg.groups, wg.nH, wg.N)
    g = wg.clv_geom()
    nt = (wg.N + 15) // 16
    assert L.clv_attn_dbias_index_count(C.byref(g)) == TABLE_ROWS * nkt * 16
    assert L.clv_attn_dbias_partial_bytes(C.byref(g)) == splits * wg.nH * nt * nkt * 1024
    one = L.clv_attn_bwd_one_kernel(C.byref(g))
    if bwd_one_env is not None:
        want = bwd_one_env == '2' and wg.hd == 32 and nt in (13, 25) and nkt == nt
        assert one == int(want), (one, want)
    return nkt, tsplit, splits, one


def run_window_case(case, label, device='cpu', bwd_one_env=None):
    wg, qkv, table, do, exact, floor = window_inputs(case, device)
    window_expectations(wg, bwd_one_env)
    from clover_amd.backbones.swin_transformer_3d import window_geometry
    B, D, H, W, Cc, nH, shifted = case
    ws, ss, rid = window_geometry((D, H, W), TABLE_WINDOW, (4, 3, 3) if shifted else (0, 0, 0), DEV)
    assert tuple(ws) == tuple(wg.ws) and tuple(ss) == tuple(wg.ss)
    qg = qkv.to(DEV, copy=True).requires_grad_()
    tg = table.to(DEV, copy=True).requires_grad_()
    o = ops().window_attention(qg, tg, rid, ws, ss, nH, table_window=TABLE_WINDOW)
    o.backward(do.to(DEV))
    torch.cuda.synchronize()
    dq, dk, dv = wg.windows(qg.grad.to(device), 3)
    got = dict(o=wg.windows(o.detach().to(device), 1)[0], dq=dq, dk=dk, dv=dv, dtable=tg.grad.to(device).t().unsqueeze(0))
    assert int(wg.used_rows.sum()) == (2 * wg.ws[0] - 1) * 13 * 13        # the temporal band of a window of depth ws[0]
    unused = (~wg.used_rows)[None, None, :].expand(1, nH, TABLE_ROWS)
    hold_to_floor(label, got, exact, floor, dict(dtable=unused))


WIN_SHAPES = {        # (hd, N) -> (B, D, H, W, C, nH)
    (16, 49): (2, 1, 14, 14, 32, 2), (32, 49): (2, 1, 14, 14, 64, 2), (64, 49): (2, 1, 14, 14, 128, 2),
    (16, 98): (1, 2, 14, 14, 48, 3), (32, 98): (2, 2, 14, 14, 64, 2), (64, 98): (1, 2, 14, 14, 128, 2),
    (16, 196): (2, 4, 14, 14, 48, 3), (32, 196): (1, 4, 14, 21, 96, 3), (64, 196): (1, 4, 14, 14, 128, 2),
    (16, 392): (1, 8, 14, 14, 48, 3), (32, 392): (1, 16, 14, 14, 64, 2), (64, 392): (1, 8, 14, 14, 128, 2),
}


@pytest.mark.parametrize('shifted', [False, True])
@pytest.mark.parametrize('hd,N', list(WIN_SHAPES))
def test_window_head_size_by_window_size(hd, N, shifted):
    """hd 16 / 32 / 64 x the four window sizes of table window (8, 7, 7): one frame (1, 7, 7) — 13 of the table's 15 temporal
    bands unused —, two, four and eight frames; block shift off and on (the temporal shift is zeroed where the window covers
    the clip, the in-plane shift stays)."""
    case = WIN_SHAPES[(hd, N)] + (shifted,)
    wg = window_inputs(case)[0]
    assert (wg.hd, wg.N) == (hd, N)
    run_window_case(case, f'window hd={hd} N={N} groups={wg.groups} shift={wg.ss}')


PRODUCTION = (2, 4, 56, 56, 96, 3)        # stage 0 of Swin: 128 groups, 384 (group, head) pairs


@pytest.mark.parametrize('bwd_one', ['2', '0'])           # backward: the one-kernel form / dQ + dK/dV kernels
@pytest.mark.parametrize('dbias_index', ['1', '0'])       # table gradient: precomputed offset table / index arithmetic
@pytest.mark.parametrize('shifted', [False, True])
def test_window_production_split(shifted, dbias_index, bwd_one, monkeypatch):
    """One workgroup per (group, head) (tsplit == 1) and two group slices of the table gradient (dbias_splits == 2)."""
    monkeypatch.setenv('CLOVER_DBIAS_INDEX', dbias_index)
    monkeypatch.setenv('CLV_ATTN_BWD_ONE', bwd_one)
    case = PRODUCTION + (shifted,)
    wg = window_inputs(case)[0]
    assert (wg.groups, wg.groups * wg.nH, wg.N) == (128, 384, 196)
    assert predict(1, wg.groups, wg.nH, wg.N) == (13, 1, 1, 2)
    run_window_case(case, f'window production shift={int(shifted)} index={dbias_index} one={bwd_one}', bwd_one_env=bwd_one)


# groups * E * 2 > DBIAS_CHUNK_MB << 20 with E = nH * 13 * 13 * 64, groups and slices even: with 24 heads 384 groups are
# the fewest (256 give 127 MiB): 6 clips of 4 x 56 x 56 tokens, two chunks of 192 groups and 3 slices each
CHUNKED = (6, 4, 56, 56, 768, 24, True)


@pytest.mark.parametrize('bwd_one', ['2', '0'])
def test_window_chunked_table_gradient(bwd_one, monkeypatch):
    """launch_bwd's chunked dQ + dbias_sum loop (nch > 1).  The references of this case run in fp64 on the device, a few
    windows at a time (attn_core's group loop)."""
    monkeypatch.setenv('CLV_ATTN_BWD_ONE', bwd_one)
    wg = window_inputs(CHUNKED, DEV)[0]
    nkt, tsplit, nparts, splits = predict(1, wg.groups, wg.nH, wg.N)
    E = wg.nH * 13 * nkt * 64
    nch = 1
    while nch < 8 and (wg.groups // nch) * E * 2 > 128 << 20 and wg.groups % (2 * nch) == 0 and splits % (2 * nch) == 0:
        nch *= 2
    assert (wg.groups, splits, tsplit, nch) == (384, 6, 1, 2)
    run_window_case(CHUNKED, f'window chunked one={bwd_one}', device=DEV, bwd_one_env=bwd_one)
    if bwd_one == '0':
        _WIN_REF.pop((CHUNKED, DEV))                      # the last user: release the device copies


def test_window_deferred_gather_with_split_slices():
    """ops.defer_folds() with a geometry of 128 groups: its entry has nsplit == 2, so dbias_split_sum_batch_kernel runs
    before the batched gather.  The sinks are held to the exact reference, and equal what the immediate path leaves."""
    from clover_amd.backbones.swin_transformer_3d import window_geometry
    cases = [PRODUCTION + (True,), (1, 8, 14, 14, 64, 2, False)]
    assert predict(1, 128, 3, 196)[3] == 2

    def run(deferred):
        sinks = []

        def body():
            for case in cases:
                wg, qkv, table, do, _, _ = window_inputs(case)
                B, D, H, W, Cc, nH, shifted = case
                ws, ss, rid = window_geometry((D, H, W), TABLE_WINDOW, (4, 3, 3) if shifted else (0, 0, 0), DEV)
                t = table.to(DEV).requires_grad_()
                t._clv_grad = torch.zeros(TABLE_ROWS, nH, device=DEV)      # an engine-style gradient sink
                t._clv_ready = lambda: None
                sinks.append(t._clv_grad)
                q = qkv.to(DEV).requires_grad_()
                ops().window_attention(q, t, rid, ws, ss, nH, table_window=TABLE_WINDOW).backward(do.to(DEV))
        if deferred:
            with ops().defer_folds():
                body()
                pend = ops().SEGMENT.dbias
                assert [e.entry.nsplit for e in pend] == [2, 1]
        else:
            body()
        torch.cuda.synchronize()
        return sinks
    now, later = run(False), run(True)
    for case, a, b in zip(cases, now, later):
        wg, _, _, _, exact, floor = window_inputs(case)
        assert _rel(b.double(), a.double()) < 1e-5
        unused = (~wg.used_rows)[None, None, :].expand(1, wg.nH, TABLE_ROWS)
        hold_to_floor(f'window deferred groups={wg.groups}', dict(dtable=b.cpu().t().unsqueeze(0)), dict(dtable=exact['dtable']),
                      dict(dtable=floor['dtable']), dict(dtable=unused))
