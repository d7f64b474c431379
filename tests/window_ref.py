"""References for window attention beyond 448 tokens (csrc/attention.hip: a window run as P parts of staged tokens).

tests/test_attention_gpu.py's `attn_core` is the exact reference (hook = identity) and, with the 16-bit round trip as hook, the
floor of the one-part kernels; its `pt=` argument models two parts and its `WindowGeom` one table window, (8, 7, 7).  Here:

  attn_core_nparts   the floor of a window (or sequence) run as ANY number of parts, with the table gradient's dS sum:
                     every part's stored o / dq / dk / dv takes the hook, and so does the merged value (seq_combine_fwd_kernel
                     `o_part` -> pack2bf, seq_combine_bwd_kernel `part` -> pack2bf); the parts are added in ascending order;
  part_plan          (parts, part tokens, staged tiles of the instantiation) as make_geom / pick_nkt choose them for a window;
  LargeWindowGeom    WindowGeom for any table window, whose reference() takes the part plan.

Nothing here touches the GPU; the tensors stay on the device of the inputs.
"""
import torch

from oracle import indexing as ix
from oracle import model as om
from clover_amd import _lib
from test_attention_gpu import LOG2E, NKTS, attn_core

WIN_PART_TILES = 25          # attention.hip WIN_ONE_PART_TILES: the table band shares the LDS with the staged part
WIN_MAX_TOKENS = 1024


def part_plan(N):
    """-> (parts, tokens per part, tiles of the instantiation); one part up to 448 tokens; None beyond 1024."""
    tiles = (N + 15) // 16
    if tiles <= 28:
        return 1, tiles * 16, next(o for o in NKTS if o >= tiles)
    if N > WIN_MAX_TOKENS:
        return None
    P = (tiles + WIN_PART_TILES - 1) // WIN_PART_TILES
    per = (tiles + P - 1) // P
    return P, per * 16, 16 if per <= 16 else 25          # attention.hip plan_nkt: the two instantiations of template MODE 2


def attn_core_nparts(q, k, v, do, scale, add, r, pt, nparts):
    """attn_core(.., pt=) for `nparts` parts of `pt` tokens, the last one shorter.  q, k, v, do [G, nH, N, hd] fp64; add(g0, g1)
    the additive term of groups [g0, g1); r the rounding hook.  -> o, dq, dk, dv and the sum of r(dS) over the groups
    [nH, N, N].  dS itself is rounded once per element whatever the part (the dQ kernel packs it for the MFMA and stores
    that same value to the scratch), so the table gradient's operand does not depend on the part plan."""
    if nparts == 1:
        return attn_core(q, k, v, do, scale, add, r)
    G, nH, N, hd = q.shape
    o, dq, dk, dv = (torch.empty_like(q) for _ in range(4))
    ds_sum = torch.zeros(nH, N, N, dtype=q.dtype, device=q.device)
    step = max(1, (1 << 24) // (nH * N * N))
    parts = [slice(i * pt, min(N, (i + 1) * pt)) for i in range(nparts)]
    assert parts[-1].start < N and parts[-1].stop == N
    T = lambda x: x.transpose(-1, -2)                                   # noqa: E731

    def total(terms):
        acc = None
        for t in terms:                                                 # ascending parts, as the combine kernels' loops
            acc = t if acc is None else acc + t
        return acc
    for g0 in range(0, G, step):
        s = slice(g0, min(G, g0 + step))
        S = scale * (q[s] @ T(k[s])) + add(s.start, s.stop)
        P = S.softmax(-1)
        O = r(total(P[..., p].sum(-1, keepdim=True) * r(r(S[..., p].softmax(-1)) @ v[s][:, :, p]) for p in parts))
        delta = (do[s] * O).sum(-1, keepdim=True)
        dP = do[s] @ T(v[s])
        dS = r(P * (dP - delta))
        qs = r(q[s] * (scale * LOG2E)) / LOG2E                          # see attn_core: dK / dV recompute P from the staged Q'
        Pkv = (qs @ T(k[s]) + add(s.start, s.stop) - S.logsumexp(-1, keepdim=True)).exp()
        dSkv, Pkvr = r(Pkv * (dP - delta)), r(Pkv)
        o[s] = O
        dq[s] = r(total(r(scale * (dS[..., p] @ k[s][:, :, p])) for p in parts))
        dk[s] = r(total(r(T(dSkv[:, :, p]) @ qs[:, :, p]) for p in parts))
        dv[s] = r(total(r(T(Pkvr[:, :, p]) @ do[s][:, :, p]) for p in parts))
        ds_sum += dS.sum(0)
    return o, dq, dk, dv, ds_sum


class LargeWindowGeom:
    """Roll / partition / region mask / table index of one window-attention geometry with ANY table window, from the oracle's
    helpers (tests/test_attention_gpu.py WindowGeom has (8, 7, 7) built in)."""

    def __init__(self, B, D, H, W, C, nH, table_window, cfg_ss):
        self.shape, self.nH, self.hd, self.tw = (B, D, H, W, C), nH, C // nH, tuple(table_window)
        self.ws, self.ss = ix.get_window_size((D, H, W), self.tw, cfg_ss)
        self.N = self.ws[0] * self.ws[1] * self.ws[2]
        self.nW = (D // self.ws[0]) * (H // self.ws[1]) * (W // self.ws[2])
        self.groups = B * self.nW
        self.rows = (2 * self.tw[0] - 1) * (2 * self.tw[1] - 1) * (2 * self.tw[2] - 1)
        self.idx = torch.from_numpy(ix.relative_position_index(self.tw)[:self.N, :self.N].reshape(-1).copy()).long()
        self.mask = torch.from_numpy(ix.compute_mask(D, H, W, self.ws, self.ss)).double() if any(self.ss) else None
        self.used_rows = torch.zeros(self.rows, dtype=torch.bool)
        self.used_rows[self.idx] = True
        self.plan = part_plan(self.N)

    def windows(self, x, parts):
        """natural layout [B, D, H, W, parts * C] -> `parts` tensors [groups, nH, N, hd] (roll(-shift) + partition)"""
        ss = self.ss
        if any(ss):
            x = torch.roll(x, shifts=(-ss[0], -ss[1], -ss[2]), dims=(1, 2, 3))
        xw = om._t_window_partition(x, self.ws).reshape(self.groups, self.N, parts, self.nH, self.hd)
        return tuple(xw.permute(2, 0, 3, 1, 4))

    def reference(self, qkv, table, do, r, parts=True):
        """-> dict of o, dq, dk, dv in window layout (+ dtable [rows, nH] with a table).  parts=False: the one-part
        arithmetic whatever N (the exact reference does not care; the floor must use the kernels' plan)."""
        dev = qkv.device
        q, k, v = self.windows(qkv.double(), 3)
        dow, = self.windows(do.double(), 1)
        idx = self.idx.to(dev)
        zero = torch.zeros(1, 1, 1, 1, dtype=torch.float64, device=dev)
        bias = table.double()[idx].reshape(self.N, self.N, self.nH).permute(2, 0, 1).unsqueeze(0) if table is not None else zero
        mask = self.mask.to(dev) if self.mask is not None else None

        def add(g0, g1):
            if mask is None:
                return bias
            return bias + mask[torch.arange(g0, g1, device=dev) % self.nW].unsqueeze(1)
        P, pt, _ = self.plan if parts else (1, None, None)
        o, dq, dk, dv, ds_sum = attn_core_nparts(q, k, v, dow, self.hd ** -0.5, add, r, pt, P)
        out = dict(o=o, dq=dq, dk=dk, dv=dv)
        if table is not None:
            dtab = torch.zeros(self.rows, self.nH, dtype=torch.float64, device=dev)
            dtab.index_add_(0, idx, ds_sum.permute(1, 2, 0).reshape(self.N * self.N, self.nH))
            out['dtable'] = dtab
        return out

    def clv_geom(self, table=True, **kw):
        B, D, H, W, Cc = self.shape
        ws, ss = self.ws, self.ss
        tw = self.tw if table else (0, 0, 0)
        return _lib.ClvAttnGeom(mode=1, groups=self.groups, N=self.N, nH=self.nH, hd=self.hd, D=D, H=H, W=W, wd=ws[0], wh=ws[1],
                                ww=ws[2], sd=ss[0], sh=ss[1], sw=ss[2], ldq=3 * Cc, ldk=3 * Cc, ldv=3 * Cc, ldo=Cc, bwd=tw[0],
                                bwh=tw[1], bww=tw[2], scale=self.hd ** -0.5, dropout_p=0.0, **kw)
