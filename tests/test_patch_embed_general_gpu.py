"""clv_patch_embed_gen_fwd / clv_patch_embed_fwd / clv_im2col_patches / clv_patch_embed_blend_bwd: bit-exact on integer data,
and held to the derived budget of tests/PATCH_EMBED_ERROR_BUDGET.md on random data, against the fp64 reference of
tests/patch_embed_ref.py.  `-m gpu` only."""
import functools

import pytest
import torch

import patch_embed_ref as pr

pytestmark = pytest.mark.gpu

from clover_amd import _lib  # noqa: E402

DEV = 'cuda'
HALF = _lib.half_dtype()
U16 = 2.0 ** -11 if _lib.HALF_F16 else 2.0 ** -8            # half an ulp of the 16-bit type, relative
TINY = 2.0 ** -25 if _lib.HALF_F16 else 0.0                 # half the subnormal spacing (fp16; bf16 has fp32's range)
F64 = torch.float64
FAST = ((2, 4, 4), (2, 4, 4))
COUTS = [48, 96, 128]


def ops():
    from clover_amd import ops as o
    return o


def clip_dims(patch, stride, masked):
    """B = 2, T' = 3 (odd).  Unmasked: 28 x 36 (H != W; M % 16 != 0: a tail tile), padded to the patch.  Masked: a 7 x 7
    mask needs H' % 7 == W' % 7 == 0 — 56 x 56 (two tokens per cell at stride 4, one at 8), 44 x 44 at stride 2 (three)."""
    T = (3 - 1) * stride[0] + patch[0]
    if not masked:
        return T, 28 + (-28 % patch[1]), 36 + (-36 % patch[2])
    return (T, 44, 44) if stride[1] == 2 else (T, 56, 56)


def asym_mask(B):
    vm = torch.zeros(B, 7, 7, dtype=torch.long)
    vm[0, 0, 1:4] = 1
    vm[0, 2:, 5] = 1
    vm[0, 6, 0] = 1
    vm[1, 1, :] = 1
    vm[1, 3:5, 2] = 1
    assert not torch.equal(vm[0], vm[0].t()) and not torch.equal(vm[0], vm[1])
    return vm


def gen_fwd(x, w, bias, gamma, beta, mt, vm, patch, stride, fast=False, stacked=False, want_clean=True):
    """One direct call of the C entry.  -> dict of clean, masked [M, C], z [M, C], mean, rstd (CPU tensors)."""
    o = ops()
    B, _, T, H, W = x.shape
    C = w.shape[0]
    Tp, Hp, Wp = pr.grid(T, H, W, patch, stride)
    M = B * Tp * Hp * Wp
    d = lambda t, dt=torch.float32: t.to(DEV, dt).contiguous() if t is not None else None
    xd, wd, bd, gd, bed, mtd = d(x), d(w.reshape(C, -1), HALF), d(bias), d(gamma), d(beta), d(mt)
    vmd = d(vm, torch.long)
    both = torch.full((2 * M, C), float('nan'), device=DEV, dtype=HALF)
    clean = both[:M] if want_clean else None
    masked = (both[M:] if stacked else torch.full((M, C), float('nan'), device=DEV, dtype=HALF)) if vm is not None else None
    z = torch.full((M, C), float('nan'), device=DEV, dtype=HALF)
    mean, rstd = torch.full((M,), float('nan'), device=DEV), torch.full((M,), float('nan'), device=DEV)
    mh, mw = (vm.shape[1], vm.shape[2]) if vm is not None else (1, 1)
    p = o._ptr
    L = _lib.lib()
    if fast:
        rc = L.clv_patch_embed_fwd(p(xd), p(wd), p(bd), p(gd), p(bed), p(mtd), p(vmd), p(clean), p(masked), p(z), p(mean),
                                   p(rstd), B, T, H, W, C, mh, mw, 1e-5, o._stream())
    else:
        rc = L.clv_patch_embed_gen_fwd(p(xd), p(wd), p(bd), p(gd), p(bed), p(mtd), p(vmd), p(clean), p(masked), p(z),
                                       p(mean), p(rstd), B, T, H, W, C, mh, mw, *patch, *stride, 1e-5, o._stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    c = lambda t: t.cpu() if t is not None else None
    return dict(clean=c(clean), masked=c(masked), z=c(z), mean=c(mean), rstd=c(rstd))


# ----------------------------------------------------------------------------- integer data: bit-exact
@functools.lru_cache(maxsize=None)
def int_case(patch, stride, C, masked):
    """Clip in {-1,0,1}; weight in {-1,0,1}, a different column pattern for every k and no symmetry between rows; for
    K = 384 every other column is zero, so at most 192 products are non-zero and |z| <= 192 + 2 < 256: exact in fp32,
    fp16 and bf16 whatever the order of the sum."""
    g = torch.Generator().manual_seed(1000 + 7 * C + sum(patch) + 3 * sum(stride) + int(masked))
    T, H, W = clip_dims(patch, stride, masked)
    K = 3 * patch[0] * patch[1] * patch[2]
    x = torch.randint(-1, 2, (2, 3, T, H, W), generator=g).float()
    w = torch.randint(-1, 2, (C, K), generator=g).float()
    if K == 384:
        w[:, 1::2] = 0
    live = w.t()[(w != 0).any(0)]
    assert len({tuple(col.tolist()) for col in live}) == len(live) >= K // 2      # every live column its own pattern
    assert len({tuple(row.tolist()) for row in w}) == C                          # and every output channel
    w = w.reshape(C, 3, *patch)
    bias = torch.randint(-2, 3, (C,), generator=g).float()
    gamma = 1 + 0.25 * torch.randint(-2, 3, (C,), generator=g).float()
    beta = 0.125 * torch.randint(-4, 5, (C,), generator=g).float()
    mt = 0.0625 * torch.randint(-8, 9, (C,), generator=g).float()           # exact in both 16-bit types
    vm = asym_mask(2) if masked else None
    ref = pr.Ref(x, w, bias, gamma, beta, mt, vm, patch, stride)
    assert ref.z.abs().max() <= 256 and ref.absdot.max() <= 256               # the exactness argument, checked
    assert ref.grid[0] == 3 and (masked or ref.M % 16 != 0)
    return x, w, bias, gamma, beta, mt, vm, ref


@pytest.mark.parametrize('C', COUTS)
@pytest.mark.parametrize('patch,stride', pr.GEOMETRIES)
def test_forward_exact_on_integers(patch, stride, C):
    for masked in (False, True):
        x, w, bias, gamma, beta, mt, vm, ref = int_case(patch, stride, C, masked)
        out = gen_fwd(x, w, bias, gamma, beta, mt, vm, patch, stride, stacked=masked)
        assert torch.equal(out['z'].double(), ref.z), (out['z'].double() - ref.z).abs().max()
        assert (out['mean'].double() - ref.mean).abs().max() <= 1e-5 * ref.mean.abs().max().clamp_min(1)
        assert ((out['rstd'].double() - ref.rstd).abs() <= 1e-5 * ref.rstd).all()
        assert torch.isfinite(out['clean'].float()).all()
        assert (out['clean'].double() - ref.y).abs().max() <= 2 * U16 * ref.y.abs().max()       # loose here; test 3 bounds it
        if masked:
            m = ref.wgt.bool()
            assert m.any() and not m.all()
            assert torch.equal(out['masked'][m], mt.to(HALF).expand(int(m.sum()), C))            # the mask token, exactly
            assert torch.equal(out['masked'][~m], out['clean'][~m])                              # clean elsewhere, exactly
        if (patch, stride) == FAST:                       # the general entry at the fast geometry: bit for bit the fast kernel
            fast = gen_fwd(x, w, bias, gamma, beta, mt, vm, patch, stride, fast=True, stacked=masked)
            for k in ('clean', 'masked', 'z', 'mean', 'rstd'):
                if out[k] is not None:
                    assert torch.equal(out[k], fast[k]), k


@pytest.mark.parametrize('patch,stride', pr.GEOMETRIES[:5])
def test_masked_only_and_no_norm_outputs(patch, stride):
    """want_clean=False (out_clean NULL) and gamma = beta = NULL: the outputs that are asked for do not change."""
    x, w, bias, gamma, beta, mt, vm, ref = int_case(patch, stride, 96, True)
    full = gen_fwd(x, w, bias, gamma, beta, mt, vm, patch, stride)
    only = gen_fwd(x, w, bias, gamma, beta, mt, vm, patch, stride, want_clean=False)
    assert torch.equal(only['masked'], full['masked']) and torch.equal(only['z'], full['z'])
    raw = gen_fwd(x, w, bias, None, None, mt, vm, patch, stride)
    assert torch.equal(raw['clean'], raw['z']) and torch.equal(raw['z'], full['z'])


@pytest.mark.parametrize('C', COUTS)
@pytest.mark.parametrize('patch,stride', pr.GEOMETRIES)
def test_backward_exact_on_integers(patch, stride, C):
    """No LayerNorm (gamma = beta = None), so dz = d_clean + d_masked (1 - w) is an integer: dW, dbias and d mask_token
    are sums of small integers, below 2^24 in magnitude — exact in fp32 in any order."""
    x, w, bias, _, _, mt, vm, _ = int_case(patch, stride, C, True)
    ref = pr.Ref(x, w, bias, None, None, mt, vm, patch, stride)
    g = torch.Generator().manual_seed(5)
    dc = torch.randint(-3, 4, (ref.M, C), generator=g).float()
    dm = torch.randint(-3, 4, (ref.M, C), generator=g).float()
    r = ref.backward(dc, dm)
    assert max(r['dW'].abs().max(), r['dbias'].abs().max(), r['dmask_token'].abs().max()) < 2 ** 24
    assert (ref.M * 6 * 1) < 2 ** 24                          # every partial sum too: |dz| <= 6, |patch| <= 1
    wg, bg, mg = (t.to(DEV).requires_grad_() for t in (w, bias, mt.reshape(1, C, 1, 1, 1)))
    clean, masked = ops().patch_embed(x.to(DEV), wg, bg, None, None, mg, vm.to(DEV), True, 1e-5, patch, stride)
    shape = clean.shape
    assert tuple(shape) == (2, *ref.grid, C)
    ((clean.float() * dc.to(DEV).view(shape)).sum() + (masked.float() * dm.to(DEV).view(shape)).sum()).backward()
    assert torch.equal(wg.grad.cpu().double().reshape(C, -1), r['dW'])
    assert torch.equal(bg.grad.cpu().double(), r['dbias'])
    assert torch.equal(mg.grad.cpu().double().reshape(-1), r['dmask_token'])


def test_im2col_gen_is_the_index_map():
    o = ops()
    for patch, stride in pr.GEOMETRIES:
        x, *_ = int_case(patch, stride, 48, False)
        B, _, T, H, W = x.shape
        idx = pr.im2col_index(B, T, H, W, patch, stride)
        xs = (torch.arange(x.numel()) % 2039 - 1019).float().view_as(x) / 8        # exact in fp16; distinct neighbours
        xs = xs.to(HALF).float()
        out = torch.empty(idx.shape, device=DEV, dtype=HALF)
        xd = xs.to(DEV)
        rc = _lib.lib().clv_im2col_patches(o._ptr(xd), o._ptr(out), B, T, H, W, *patch, *stride, o._stream())
        assert rc == 0
        assert torch.equal(out.cpu().float(), xs.reshape(-1)[idx])


@pytest.mark.parametrize('C', COUTS)
def test_blend_backward_entry_exact_on_integers(C):
    """clv_patch_embed_blend_bwd alone, with the asymmetric 7 x 7 mask.  A block pass covers 42 / 21 / 16 rows at
    C = 48 / 96 / 128 (at 48 the 42 rows leave 4 of the 256 threads idle).  Token grid (2, 3, 14, 14): M = 1176 = 28 * 42 =
    56 * 21 fills whole passes at 48 and 96 and leaves a tail at 128 (73.5 passes); token grid (2, 1, 7, 7): M = 98, a tail
    at every width.  Integer gradients in [-3, 3]: dy (|dy| <= 6) and d mask_token (|sum| <= 3 M) are exact in any order."""
    o, L = ops(), _lib.lib()
    p = o._ptr
    for B, Tp, Hp, Wp in ((2, 3, 14, 14), (2, 1, 7, 7)):
        M = B * Tp * Hp * Wp
        assert M in (1176, 98) and M % 16 and (M == 1176 or all(M % (256 // (c // 8)) for c in COUTS))
        vm = asym_mask(B)
        wgt = pr.token_weight(vm, Tp, Hp, Wp)[:, None]
        g = torch.Generator().manual_seed(11 + C)
        dc = torch.randint(-3, 4, (M, C), generator=g).double()
        dm = torch.randint(-3, 4, (M, C), generator=g).double()
        dcd, dmd, vmd = dc.to(DEV, HALF), dm.to(DEV, HALF), vm.to(DEV)
        for clean in (dcd, None):
            dy = torch.full((M, C), float('nan'), device=DEV, dtype=HALF)
            dmt = torch.zeros(C, device=DEV)
            rc = L.clv_patch_embed_blend_bwd(p(clean), p(dmd), p(vmd), p(dy), p(dmt), B, Tp, Hp, Wp, C, 7, 7, o._stream())
            torch.cuda.synchronize()
            assert rc == 0, rc
            want = (dc if clean is not None else 0) + dm * (1 - wgt)           # patch_embed_ref.Ref.backward
            assert torch.equal(dy.cpu().double(), want)
            assert torch.equal(dmt.cpu().double(), (dm * wgt).sum(0))
    rc = L.clv_patch_embed_blend_bwd(p(dcd), p(dmd), p(vmd), p(dy), p(dmt), 2, 1, 7, 12, C, 7, 7, o._stream())
    assert rc == -1                                                            # 12 % 7 != 0: CLV_ERR_ARG


# ----------------------------------------------------------------------------- random data: the derived budget
@functools.lru_cache(maxsize=None)
def rnd_case(patch, stride, C):
    g = torch.Generator().manual_seed(2000 + C + sum(patch) + 3 * sum(stride))
    T, H, W = clip_dims(patch, stride, True)
    x = torch.randn(2, 3, T, H, W, generator=g).to(HALF).float()                          # the 16-bit-rounded clip
    w = (torch.randn(C, 3, *patch, generator=g) * 0.1).to(HALF).float()                   # and weight
    bias, gamma = 0.1 * torch.randn(C, generator=g), 1 + 0.1 * torch.randn(C, generator=g)
    beta, mt = 0.1 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    vm = asym_mask(2)
    ref = pr.Ref(x, w, bias, gamma, beta, mt, vm, patch, stride)
    dc = torch.randn(ref.M, C, generator=g).to(HALF).float()
    dm = torch.randn(ref.M, C, generator=g).to(HALF).float()
    return x, w, bias, gamma, beta, mt, vm, ref, dc, dm


def check(name, got, want, bound):
    err = (got.double() - want).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f'{name}: max err {err.max().item():.3e}, worst err/bound {worst:.3f}')
    assert worst <= 1.0, (name, worst)


def forward_within_budget(patch, stride, C, fast):
    x, w, bias, gamma, beta, mt, vm, ref, _, _ = rnd_case(patch, stride, C)
    out = gen_fwd(x, w, bias, gamma, beta, mt, vm, patch, stride, fast=fast)
    check('z', out['z'], ref.z, pr.Ref.round16(ref.z, ref.budget_z32(), U16, TINY))
    y32 = ref.budget_y32()
    check('clean', out['clean'], ref.y, pr.Ref.round16(ref.y, y32, U16, TINY))
    blend = y32 * (1 - ref.wgt[:, None]) + 4 * pr.Ref.U32 * ref.ym.abs()
    check('masked', out['masked'], ref.ym, pr.Ref.round16(ref.ym, blend, U16, TINY))
    E = ref.budget_z32().max(1).values + (C + 2) * pr.Ref.U32 * ref.z.abs().max(1).values
    check('mean', out['mean'], ref.mean, E + pr.Ref.U32 * ref.mean.abs())
    check('rstd', out['rstd'], ref.rstd, ref.rstd * (2 * E * ref.rstd + (C + 8) * pr.Ref.U32))


def backward_within_budget(patch, stride, C):
    x, w, bias, gamma, beta, mt, vm, ref, dc, dm = rnd_case(patch, stride, C)
    r, bound = ref.budget_grads(dc, dm, U16)
    leaves = [t.to(DEV).requires_grad_() for t in (w, bias, gamma, beta, mt.reshape(1, C, 1, 1, 1))]
    wg, bg, gg, beg, mg = leaves
    clean, masked = ops().patch_embed(x.to(DEV), wg, bg, gg, beg, mg, vm.to(DEV), True, 1e-5, patch, stride)
    shape = clean.shape
    ((clean.float() * dc.to(DEV).view(shape)).sum() + (masked.float() * dm.to(DEV).view(shape)).sum()).backward()
    check('dW', wg.grad.cpu().reshape(C, -1), r['dW'], bound['dW'])
    check('dbias', bg.grad.cpu(), r['dbias'], bound['dbias'])
    check('dgamma', gg.grad.cpu(), r['dgamma'], bound['dgamma'])
    check('dbeta', beg.grad.cpu(), r['dbeta'], bound['dbeta'])


@pytest.mark.parametrize('C', COUTS)
@pytest.mark.parametrize('patch,stride', pr.GEOMETRIES)
def test_forward_within_budget(patch, stride, C):
    forward_within_budget(patch, stride, C, fast=False)


@pytest.mark.parametrize('C', COUTS)
@pytest.mark.parametrize('patch,stride', pr.GEOMETRIES[:5])
def test_backward_within_budget(patch, stride, C):
    backward_within_budget(patch, stride, C)


@pytest.mark.parametrize('C', COUTS)
def test_fast_kernel_meets_the_same_budget(C):
    """Sanity of the budget itself: the existing (2,4,4) kernel and its backward chain are held to it too."""
    forward_within_budget(*FAST, C, fast=True)
    backward_within_budget(*FAST, C)


# ----------------------------------------------------------------------------- refusals at the first call
def test_mask_grid_must_divide_the_token_grid():
    x = torch.zeros(1, 3, 2, 28, 36, device=DEV)                               # (1,4,4): tokens 7 x 9; 9 % 7 != 0
    w, b = torch.zeros(48, 3, 1, 4, 4, device=DEV), torch.zeros(48, device=DEV)
    mt, vm = torch.zeros(1, 48, 1, 1, 1, device=DEV), torch.zeros(1, 7, 7, dtype=torch.long, device=DEV)
    with pytest.raises(ValueError, match='does not divide the token grid'):
        ops().patch_embed(x, w, b, None, None, mt, vm, True, 1e-5, (1, 4, 4), (1, 4, 4))
    p = ops()._ptr
    out = torch.empty(2 * 63, 48, device=DEV, dtype=HALF)
    rc = _lib.lib().clv_patch_embed_gen_fwd(p(x), p(w.to(HALF)), p(b), None, None, p(mt), p(vm), None, p(out), None, None, None,
                                            1, 2, 28, 36, 48, 7, 7, 1, 4, 4, 1, 4, 4, 1e-5, ops()._stream())
    assert rc == -1                                                            # CLV_ERR_ARG from the entry itself
    rc = _lib.lib().clv_patch_embed_gen_fwd(p(x), p(w.to(HALF)), p(b), None, None, None, None, p(out), None, None, None, None,
                                            1, 2, 28, 36, 48, 1, 1, 1, 4, 4, 2, 4, 4, 1e-5, ops()._stream())
    assert rc == -2                                                            # stride > patch: CLV_ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError, match='stride'):
        ops().patch_embed(x, w, b, None, None, None, None, True, 1e-5, (1, 4, 4), (2, 4, 4))


def test_unpadded_clip_and_wrong_weight_are_refused_with_the_reason():
    w, b = torch.zeros(48, 3, 2, 4, 4, device=DEV), torch.zeros(48, device=DEV)
    with pytest.raises(ValueError, match='not padded'):
        ops().patch_embed(torch.zeros(1, 3, 3, 28, 36, device=DEV), w, b, None, None, None, None, True, 1e-5, (2, 4, 4), (1, 4, 4))
    with pytest.raises(ValueError, match='patch size'):
        ops().patch_embed(torch.zeros(1, 3, 4, 28, 36, device=DEV), w, b, None, None, None, None, True, 1e-5, (1, 4, 4), (1, 4, 4))


def test_fast_geometry_is_refused_with_the_same_reasons():
    w, b = torch.zeros(48, 3, 2, 4, 4, device=DEV), torch.zeros(48, device=DEV)
    with pytest.raises(ValueError, match='not padded'):
        ops().patch_embed(torch.zeros(1, 3, 3, 28, 36, device=DEV), w, b, None, None, None, None, True, 1e-5, *FAST)
    mt, vm = torch.zeros(1, 48, 1, 1, 1, device=DEV), torch.zeros(1, 7, 7, dtype=torch.long, device=DEV)
    with pytest.raises(ValueError, match='does not divide the token grid'):            # tokens 7 x 9; 9 % 7 != 0
        ops().patch_embed(torch.zeros(1, 3, 2, 28, 36, device=DEV), w, b, None, None, mt, vm, True, 1e-5, *FAST)
