"""Plain-torch references of the operations in csrc/norm_act.hip: no GPU code, any device, fp64 unless a caller casts.

`ln_core` is LayerNorm forward + backward by explicit formulas with a rounding hook r: r = identity is the EXACT reference,
r = a round trip through the library's 16-bit type is the FLOOR (what the element type alone costs).  Every 16-bit rounding
the kernels make is in it — the stored y, the stored sum, the stored dx / dres, and the re-read of the stored sum by a
backward that runs with x_is_sum — so tests/test_norm_act_gpu.py holds the kernels to small multiples of the floor's own
error.  tests/test_norm_ref_cpu.py checks these functions against torch autograd; tests/NORM_ACT_ERROR_BUDGET.md has the
measured figures."""
import math

import numpy as np
import torch


def ident(t):
    return t


def _opt(v, like, fill):
    """None -> the neutral element; a tensor (or number) -> fp64 on `like`'s device."""
    if v is None:
        return torch.full((), fill, dtype=torch.float64, device=like.device)
    return torch.as_tensor(v, device=like.device).double()


def ln_core(x, res, k, gamma, beta, eps, dy, dy2, dsum, r, x_is_sum):
    """x, res, dy, dy2, dsum: [rows, C] (res, dy2, dsum may be None); k: the multiplier on x (dropout keep / (1 - p) times the
    per-sample scale), broadcastable to [rows, C], or None for 1; gamma, beta [C]; r: the rounding hook.
    x_is_sum: the backward re-reads the stored (rounded) sum against the forward's unrounded statistics, as the kernels do for
    a LayerNorm that returned its sum.
    -> dict of y, s (= r(x.k + res)), mean, rstd [rows], dgamma, dbeta [C], dx, dres — all fp64."""
    x = x.double()
    k, res, dy2, dsum = _opt(k, x, 1.0), _opt(res, x, 0.0), _opt(dy2, x, 0.0), _opt(dsum, x, 0.0)
    gamma, beta, dy = gamma.double().to(x.device), beta.double().to(x.device), dy.double()
    t = x * k + res
    mu = t.mean(-1, keepdim=True)
    var = (t - mu).pow(2).mean(-1, keepdim=True)
    rstd = (var + eps).rsqrt()
    y = r((t - mu) * rstd * gamma + beta)
    s = r(t)
    tb = s if x_is_sum else t
    xh = (tb - mu) * rstd
    d = dy + dy2
    dgamma, dbeta = (d * xh).sum(0), d.sum(0)
    g = d * gamma
    dt = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True)) + dsum
    return dict(y=y, s=s, mean=mu.squeeze(-1), rstd=rstd.squeeze(-1), dgamma=dgamma, dbeta=dbeta, dres=r(dt),
                dx=r(dt * k))


# ------------------------------------------------------------------------------ PatchMerging gather
def merge_gather(x):
    """[B, D, H, W, C] (H, W even) -> [B * D * H/2 * W/2, 4C] in the order of oracle.indexing.patch_merging_gather:
    (even h, even w), (odd h, even w), (even h, odd w), (odd h, odd w)."""
    C = x.shape[-1]
    return torch.cat([x[:, :, 0::2, 0::2], x[:, :, 1::2, 0::2], x[:, :, 0::2, 1::2], x[:, :, 1::2, 1::2]], -1).reshape(-1, 4 * C)


def merge_scatter(g, shape):
    """The inverse of merge_gather: [rows, 4C] -> `shape` = (B, D, H, W, C); every element is written exactly once."""
    B, D, H, W, C = shape
    g = g.reshape(B, D, H // 2, W // 2, 4, C)
    out = torch.empty(shape, dtype=g.dtype, device=g.device)
    out[:, :, 0::2, 0::2], out[:, :, 1::2, 0::2] = g[..., 0, :], g[..., 1, :]
    out[:, :, 0::2, 1::2], out[:, :, 1::2, 1::2] = g[..., 2, :], g[..., 3, :]
    return out


# ------------------------------------------------------------------------------ the dropout mask of the vector LayerNorm
_M32 = 0xFFFFFFFF


def _mul32(x, c):
    """(x * c) mod 2^32 on int64 tensors holding values below 2^32, without leaving the int64 range."""
    return (x * (c & 0xFFFF) + (((x * (c >> 16)) & _M32) << 16)) & _M32


def ln_keep_mask(seed, rows, C, p, device='cpu'):
    """Bool [rows, C], True = kept: `ln_keep` of norm_act.hip in integer arithmetic — a pure function of (seed, row, column).
    seed: the 64-bit value the kernel reads; p: the dropout probability as the C ABI carries it (a float)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    thresh = int(float(np.float32(p)) * 4294967296.0) & _M32
    row = torch.arange(rows, dtype=torch.int64, device=device)[:, None]
    col = torch.arange(C, dtype=torch.int64, device=device)[None, :]
    x = _mul32(row, 0x9E3779B1) ^ _mul32(col, 0x85EBCA77) ^ (seed & _M32)
    x = x ^ (x >> 16)
    x = _mul32(x, 0x7feb352d)
    x = x ^ (x >> 15)
    x = _mul32(x, 0x846ca68b)
    x = x ^ (x >> 16)
    x = (x + (seed >> 32)) & _M32
    x = x ^ (x >> 15)
    x = _mul32(x, 0x2c1b3c6d)
    x = x ^ (x >> 12)
    return x >= thresh


def inv_keep(p):
    """1 / (1 - p) as make_lnx computes it: in float."""
    p = np.float32(p)
    return float(np.float32(1.0) / (np.float32(1.0) - p))


# ------------------------------------------------------------------------------ GELU
def gelu64(x):
    """x Phi(x) with Phi through erfc, which keeps the negative tail exact (1 + erf cancels there)."""
    x = x.double()
    return x * 0.5 * torch.special.erfc(-x * math.sqrt(0.5))


def gelu_grad64(x):
    """Phi(x) + x phi(x)."""
    x = x.double()
    return 0.5 * torch.special.erfc(-x * math.sqrt(0.5)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def spacing16(v, dtype):
    """The distance between neighbouring values of the 16-bit `dtype` at the magnitude of v (fp64 tensor)."""
    mant, emin = (10, -14) if dtype == torch.float16 else (7, -126)
    e = (torch.frexp(v.double().abs().clamp_min(2.0 ** emin))[1] - 1).clamp_min(emin)
    return torch.exp2((e - mant).double())
