"""fp64 restatement of PatchEmbed3D + LayerNorm + mask-token blend for any patch size and stride, forward and backward,
with the error budget of tests/PATCH_EMBED_ERROR_BUDGET.md.  Plain torch on the CPU; tests/test_patch_embed_ref_cpu.py
checks it against torch.nn.functional.conv3d(stride=...) and fp64 autograd."""
import torch

F64 = torch.float64

# (patch, stride) of the general-kernel tests
GEOMETRIES = [((1, 4, 4), (1, 4, 4)), ((4, 4, 4), (4, 4, 4)), ((2, 4, 4), (1, 4, 4)), ((2, 4, 4), (2, 2, 2)),
              ((2, 8, 8), (2, 8, 8)), ((2, 4, 4), (2, 4, 4))]


def grid(T, H, W, patch, stride):
    """Token grid of a clip that is already padded to multiples of the patch: floor((n - p) / s) + 1 per axis."""
    return tuple((n - p) // s + 1 for n, p, s in zip((T, H, W), patch, stride))


def pad_to_patch(x, patch):
    """Zero-pad back / bottom / right to multiples of the patch (what PatchEmbed3D.pad does)."""
    T, H, W = x.shape[2:]
    return torch.nn.functional.pad(x, (0, -W % patch[2], 0, -H % patch[1], 0, -T % patch[0]))


def im2col_index(B, T, H, W, patch, stride):
    """int64 [M, K]: flat index into the [B,3,T,H,W] clip of patch element k = ((c*pt + dt)*ph + dy)*pw + dx of token
    m = ((b*T' + t')*H' + h')*W' + w' — a per-token base plus a per-k offset."""
    pt, ph, pw = patch
    st, sh, sw = stride
    Tp, Hp, Wp = grid(T, H, W, patch, stride)
    ar = torch.arange
    base = (ar(B).view(B, 1, 1, 1) * 3 * T * H * W + ar(Tp).view(1, Tp, 1, 1) * st * H * W
            + ar(Hp).view(1, 1, Hp, 1) * sh * W + ar(Wp).view(1, 1, 1, Wp) * sw).reshape(-1)
    koff = (ar(3).view(3, 1, 1, 1) * T * H * W + ar(pt).view(1, pt, 1, 1) * H * W + ar(ph).view(1, 1, ph, 1) * W
            + ar(pw).view(1, 1, 1, pw)).reshape(-1)
    return base[:, None] + koff[None, :]


def token_weight(vmask, Tp, Hp, Wp):
    """float64 [M]: 1 on masked tokens.  vmask [B, mh, mw]; one cell covers H'/mh x W'/mw tokens of every frame."""
    B, mh, mw = vmask.shape
    assert Hp % mh == 0 and Wp % mw == 0
    w = vmask.reshape(B, 1, mh, 1, mw, 1).expand(B, Tp, mh, Hp // mh, mw, Wp // mw)
    return w.reshape(-1).to(F64)


class Ref:
    """Forward of one case in fp64, every intermediate kept; .backward() for the gradients; .budget_*() for the bounds."""

    def __init__(self, x, w, bias, gamma, beta, mask_token, vmask, patch, stride, eps=1e-5):
        B, _, T, H, W = x.shape
        self.C, self.K = w.shape[0], w[0].numel()
        self.grid = grid(T, H, W, patch, stride)
        self.P = x.to(F64).reshape(-1)[im2col_index(B, T, H, W, patch, stride)]          # [M, K]
        self.W2 = w.to(F64).reshape(self.C, self.K)
        self.M = self.P.shape[0]
        self.bias = bias.to(F64)
        self.z = self.P @ self.W2.t() + self.bias
        self.absdot = self.P.abs() @ self.W2.abs().t() + self.bias.abs()                 # sum_k |a_k w_k| + |bias|
        self.gamma = gamma.to(F64) if gamma is not None else None
        if gamma is not None:
            self.mean = self.z.mean(1)
            var = ((self.z - self.mean[:, None]) ** 2).mean(1)
            self.rstd = (var + eps) ** -0.5
            self.xhat = (self.z - self.mean[:, None]) * self.rstd[:, None]
            self.y = self.xhat * self.gamma + beta.to(F64)
        else:
            self.mean, self.rstd = torch.zeros(self.M, dtype=F64), torch.ones(self.M, dtype=F64)
            self.xhat, self.y = self.z, self.z
        self.wgt = token_weight(vmask, *self.grid) if vmask is not None else None
        if vmask is not None:
            self.mt = mask_token.to(F64).reshape(-1)
            self.ym = self.y * (1 - self.wgt[:, None]) + self.mt[None, :] * self.wgt[:, None]

    def backward(self, dclean, dmasked):
        """dclean / dmasked [M, C] (either None) -> dict of dW [C,K], dbias, dgamma, dbeta, dmask_token, dz, dy."""
        zero = torch.zeros(self.M, self.C, dtype=F64)
        dc = dclean.to(F64).reshape(self.M, self.C) if dclean is not None else zero
        out = {}
        if dmasked is not None:
            dm = dmasked.to(F64).reshape(self.M, self.C)
            dy = dc + dm * (1 - self.wgt[:, None])
            out['dmask_token'] = (dm * self.wgt[:, None]).sum(0)
        else:
            dy = dc
        if self.gamma is not None:
            out['dgamma'] = (dy * self.xhat).sum(0)
            out['dbeta'] = dy.sum(0)
            g = dy * self.gamma
            dz = self.rstd[:, None] * (g - g.mean(1, keepdim=True) - self.xhat * (g * self.xhat).mean(1, keepdim=True))
        else:
            dz = dy
        out.update(dy=dy, dz=dz, dW=dz.t() @ self.P, dbias=dz.sum(0))
        return out

    # ---- error budget (tests/PATCH_EMBED_ERROR_BUDGET.md); u16 = half an ulp of the 16-bit type, relative ----
    U32 = 2.0 ** -24

    def budget_z32(self):
        """|z as the kernel holds it in fp32 - z|: K products accumulated in fp32, then the bias add."""
        return (self.K + 1) * self.U32 * self.absdot

    @staticmethod
    def round16(v, e, u16, tiny):
        """Bound on |r16(v + d) - v| for |d| <= e: the error carried in, plus half an ulp at the rounded magnitude."""
        return e + u16 * (v.abs() + e) + tiny

    def budget_y32(self):
        """|LayerNorm output in fp32 - y|: the carried z error through the normalisation, plus the fp32 statistics."""
        if self.gamma is None:
            return self.budget_z32()
        # a uniform bound E on |dz| per row: the accumulation term, plus the fp32 sum of C values for the mean
        E = self.budget_z32().max(1).values + (self.C + 2) * self.U32 * self.z.abs().max(1).values
        amp = 2 * E * self.rstd                                                     # |d xhat| <= amp (1 + |xhat|)
        # variance sum of C fp32 squares, the hardware reciprocal square root (1 ulp) and the final fma: (C + 8) u32 relative
        return self.gamma.abs() * (amp[:, None] * (1 + self.xhat.abs()) + (self.C + 8) * self.U32 * self.xhat.abs()) \
            + 4 * self.U32 * self.y.abs()

    def budget_grads(self, dclean, dmasked, u16):
        """Bounds on the kernel chain's dW, dbias, dgamma, dbeta against .backward(): the chain stores z, dy (when it blends)
        and dz in the 16-bit type and accumulates over the M tokens in fp32."""
        r = self.backward(dclean, dmasked)
        U, M, so = self.U32, self.M, 1 + 8 * u16                                   # so: covers the second-order terms
        ddy = u16 * r['dy'].abs() if dmasked is not None else torch.zeros_like(r['dy'])
        out = {}
        if self.gamma is not None:
            # xhat as the backward rebuilds it, (z16 - mean32) rstd32: the stored z re-read, and the forward's fp32 statistics
            E = self.budget_z32().max(1).values + (self.C + 2) * U * self.z.abs().max(1).values
            drs = (2 * E * self.rstd + (self.C + 8) * U)[:, None]                  # |d rstd| / rstd
            dxh = (self.round16(self.z, self.budget_z32(), u16, 2.0 ** -25) + E[:, None]) * self.rstd[:, None] \
                + self.xhat.abs() * drs
            g, dg = r['dy'] * self.gamma, ddy * self.gamma.abs()
            c2 = (g * self.xhat).mean(1, keepdim=True)
            dc2 = (dg * self.xhat.abs() + g.abs() * dxh).mean(1, keepdim=True)
            ddz32 = self.rstd[:, None] * (dg + dg.mean(1, keepdim=True) + dxh * c2.abs() + self.xhat.abs() * dc2) \
                + r['dz'].abs() * drs \
                + (2 * self.C + 16) * U * self.rstd[:, None] * (g.abs() + g.abs().mean(1, keepdim=True)
                                                              + self.xhat.abs() * (g.abs() * self.xhat.abs()).mean(1, keepdim=True))
            out['dgamma'] = so * ((ddy * self.xhat.abs() + r['dy'].abs() * dxh).sum(0)
                                  + (M + 2) * U * (r['dy'].abs() * self.xhat.abs()).sum(0))
            out['dbeta'] = so * (ddy.sum(0) + (M + 2) * U * r['dy'].abs().sum(0))
            ddz = self.round16(r['dz'], ddz32, u16, 2.0 ** -25)
        else:
            ddz = ddy
        adz = r['dz'].abs() + ddz
        out['dW'] = so * (ddz.t() @ self.P.abs() + (M + 2) * U * (adz.t() @ self.P.abs()))
        out['dbias'] = so * (ddz.sum(0) + (M + 2) * U * adz.sum(0))
        return r, out
