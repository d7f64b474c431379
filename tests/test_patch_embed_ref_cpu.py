"""The fp64 patch-embed reference (tests/patch_embed_ref.py) against torch's conv3d(stride=...) + layer_norm + blend and
fp64 autograd, the output-grid formula, and the refusals of the general kernel's supported set (host only: no GPU)."""
import os

import pytest
import torch
import torch.nn.functional as F

import patch_embed_ref as pr

F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def case(patch, stride, C=16, seed=0):
    g = torch.Generator().manual_seed(seed)
    B, T, H, W = 2, 3 * patch[0], 28, 36
    x = pr.pad_to_patch(torch.randn(B, 3, T, H, W, generator=g, dtype=F64), patch)
    w = torch.randn(C, 3, *patch, generator=g, dtype=F64) * 0.2
    vec = [torch.randn(C, generator=g, dtype=F64) for _ in range(4)]
    return x, w, vec[0], 1 + 0.1 * vec[1], 0.1 * vec[2], vec[3], g


@pytest.mark.parametrize('patch,stride', pr.GEOMETRIES)
@pytest.mark.parametrize('norm', [True, False])
def test_reference_equals_conv3d_and_autograd(patch, stride, norm):
    x, w, bias, gamma, beta, mt, g = case(patch, stride)
    B, _, T, H, W = x.shape
    Tp, Hp, Wp = pr.grid(T, H, W, patch, stride)
    vmask = (torch.rand(B, Hp, 1, generator=g) > 0.5).long().expand(B, Hp, Wp).contiguous()   # one cell per token
    vmask[0, 0, 0], vmask[0, 0, 1] = 1, 0
    leaves = [t.clone().requires_grad_() for t in (w, bias, gamma, beta, mt)]
    wl, bl, gl, bel, mtl = leaves
    z = F.conv3d(x, wl, bl, stride=stride)
    assert tuple(z.shape[2:]) == (Tp, Hp, Wp)                                  # the grid formula is conv3d's
    z = z.permute(0, 2, 3, 4, 1).reshape(-1, w.shape[0])
    y = F.layer_norm(z, (w.shape[0],), gl, bel, 1e-5) if norm else z
    wt = vmask.reshape(B, 1, Hp, Wp).expand(B, Tp, Hp, Wp).reshape(-1, 1).to(F64)
    ym = y * (1 - wt) + mtl[None, :] * wt
    dc, dm = torch.randn(*y.shape, generator=g, dtype=F64), torch.randn(*y.shape, generator=g, dtype=F64)
    ((y * dc).sum() + (ym * dm).sum()).backward()

    ref = pr.Ref(x, w, bias, gamma if norm else None, beta if norm else None, mt, vmask, patch, stride)
    assert ref.grid == (Tp, Hp, Wp) and ref.M == z.shape[0]
    for got, want in ((ref.z, z), (ref.y, y), (ref.ym, ym)):
        assert (got - want.detach()).abs().max() <= 1e-12 * want.abs().max()
    r = ref.backward(dc, dm)
    pairs = [('dW', wl), ('dbias', bl), ('dmask_token', mtl)] + ([('dgamma', gl), ('dbeta', bel)] if norm else [])
    for name, leaf in pairs:
        want = leaf.grad.reshape(r[name].shape)
        assert (r[name] - want).abs().max() <= 1e-11 * want.abs().max(), name


def test_two_cells_per_token_weight():
    vm = torch.tensor([[[1, 0], [0, 1]]])
    w = pr.token_weight(vm, 2, 4, 4).reshape(2, 4, 4)
    assert torch.equal(w[0], w[1])
    assert torch.equal(w[0], torch.tensor([[1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 1, 1], [0, 0, 1, 1]], dtype=F64))


@pytest.mark.parametrize('dims,patch,stride,want', [
    ((8, 224, 224), (2, 4, 4), (2, 4, 4), (4, 56, 56)), ((8, 224, 224), (1, 4, 4), (1, 4, 4), (8, 56, 56)),
    ((8, 224, 224), (2, 4, 4), (1, 4, 4), (7, 56, 56)), ((6, 28, 36), (2, 4, 4), (2, 2, 2), (3, 13, 17)),
    ((1, 30, 33), (2, 8, 8), (2, 8, 8), (1, 4, 5)), ((5, 30, 33), (2, 4, 4), (1, 4, 4), (5, 8, 9))])
def test_output_grid(dims, patch, stride, want):
    """ops.patch_grid pads to multiples of the patch first, as PatchEmbed3D.pad does, and equals conv3d's grid."""
    from clover_amd import ops
    assert ops.patch_grid(*dims, patch, stride) == want
    x = pr.pad_to_patch(torch.zeros(1, 3, *dims), patch)
    assert pr.grid(*x.shape[2:], patch, stride) == want
    assert tuple(F.conv3d(x, torch.zeros(1, 3, *patch), stride=stride).shape[2:]) == want


def test_supported_set():
    from clover_amd import _lib, ops
    sup = _lib.lib().clv_patch_embed_gen_supported
    for patch, stride in pr.GEOMETRIES:
        for C in (48, 96, 128):
            assert sup(*patch, *stride, C) == 0
            assert ops.patch_embed_refusal(patch, stride, 3, C) is None
    assert sup(1, 1, 8, 1, 1, 1, 96) == 0 and sup(2, 8, 8, 1, 1, 1, 48) == 0        # K = 24, the smallest; K = 384, the largest
    refused = [((2, 4, 4), (4, 4, 4), 3, 96, 'stride'), ((2, 4, 4), (2, 5, 4), 3, 96, 'stride'),
               ((2, 4, 4), (2, 0, 4), 3, 96, 'stride'), ((1, 2, 2), (1, 2, 2), 3, 96, 'multiple of 8'),
               ((3, 4, 4), (3, 4, 4), 3, 96, None), ((2, 3, 3), (2, 3, 3), 3, 96, 'multiple of 8'),
               ((4, 8, 8), (4, 8, 8), 3, 96, 'exceeds 384'), ((2, 8, 16), (2, 8, 16), 3, 96, 'exceeds 384'),
               ((2, 4, 4), (1, 4, 4), 3, 192, 'embed_dim'), ((2, 4, 4), (1, 4, 4), 1, 96, 'in_chans'),
               ((0, 4, 4), (1, 4, 4), 3, 96, 'patch extent')]
    for patch, stride, cin, C, word in refused:
        why = ops.patch_embed_refusal(patch, stride, cin, C)
        if word is None:                                                    # (3,4,4): 48 % 8 == 0, K = 144: covered
            assert why is None
        else:
            assert why is not None and word in why, (patch, stride, cin, C, why)


def test_module_refuses_at_construction_with_the_reason():
    from clover_amd.backbones.swin_transformer_3d import PatchEmbed3D, SwinTransformer3D
    for kw, word in [(dict(patch_size=(2, 4, 4), stride=(4, 4, 4)), 'stride'), (dict(patch_size=(1, 2, 2), stride=(1, 2, 2)), 'multiple of 8'),
                     (dict(in_chans=1), 'in_chans'), (dict(patch_size=(4, 8, 8), stride=(4, 8, 8)), 'exceeds 384'),
                     (dict(patch_size=(1, 4, 4), stride=(1, 4, 4), embed_dim=192), 'embed_dim'), (dict(embed_dim=192), 'embed_dim')]:
        with pytest.raises(NotImplementedError, match=word):
            PatchEmbed3D(**kw)
    with pytest.raises(NotImplementedError, match='stride'):
        SwinTransformer3D(patch_size=(2, 4, 4), stride=(3, 4, 4), depths=[1, 1], num_heads=[3, 6])
    m = PatchEmbed3D(patch_size=(2, 4, 4), stride=(1, 4, 4), embed_dim=48)
    assert m.proj.stride == (1, 4, 4) and m.proj.kernel_size == (2, 4, 4)


@pytest.mark.parametrize('pt', [1, 4])
def test_inflate_state_dict_closed_form(pt):
    from clover_amd.backbones.swin_transformer_3d import SwinTransformer3D
    m = SwinTransformer3D(patch_size=(pt, 4, 4), stride=(pt, 4, 4), embed_dim=48, depths=[1, 1], num_heads=[3, 6],
                          window_size=(2, 7, 7))
    sd2d = {'patch_embed.proj.weight': torch.randn(48, 3, 4, 4, generator=torch.Generator().manual_seed(pt))}
    w3 = m.inflate_state_dict(sd2d)['patch_embed.proj.weight']
    assert tuple(w3.shape) == (48, 3, pt, 4, 4) == tuple(m.patch_embed.proj.weight.shape)
    for dt in range(pt):
        assert torch.equal(w3[:, :, dt], sd2d['patch_embed.proj.weight'] / pt)
    assert torch.allclose(w3.sum(2), sd2d['patch_embed.proj.weight'], rtol=0, atol=1e-6)   # a still clip sees the 2-D filter


def test_config_sets_frame_tokens():
    from clover_amd.runner import Config
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'pretrain_frame_tokens_synthetic.py'))
    bb, mm = cfg.model['backbone'], cfg.model['mm_backbone']
    assert tuple(bb['patch_size']) == tuple(bb['stride']) == (1, 4, 4)
    assert mm['num_frames'] == cfg.data['synthetic'][0]['frames'] == 8
