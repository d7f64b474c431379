"""PatchEmbed3D geometries other than (2,4,4 | 2,4,4) at the module and the engine level: SwinTransformer3D against the
fp32 oracle (16-bit path and parity mode), and CloverEngine — eager step = captured step, the loss falls, no library GEMM —
on the model of configs/pretrain_frame_tokens_synthetic.py with the depths cut down.  `-m gpu` only."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEV = 'cuda'


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-20)).item()


# ----------------------------------------------------------------------------- SwinTransformer3D vs the oracle
@pytest.fixture(scope='module', params=[(1, 4, 4), (4, 4, 4)], ids=['p144', 'p444'])
def swin_case(request):
    """A two-stage backbone with patch = stride, one seeded clip whose frame count is NOT a multiple of the patch depth
    (PatchEmbed3D.pad runs), a 7 x 7 mask over 14 x 14 tokens, and the oracle's outputs — computed once."""
    from clover_amd.backbones.swin_transformer_3d import SwinTransformer3D
    from oracle import model as om
    patch = request.param
    torch.manual_seed(144 + patch[0])
    m = SwinTransformer3D(patch_size=patch, stride=patch, embed_dim=48, depths=[2, 2], num_heads=[3, 6],
                          window_size=(8, 7, 7), drop_path_rate=0.0, mask_token=True, pretrained2d=False)
    m.eval()
    with torch.no_grad():                                 # LayerNorm gains / biases and the mask token away from 1 / 0
        for n, p in m.named_parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p))
    T = 3 if patch[0] == 1 else 6                          # (4,4,4): 6 frames are padded to 8
    x = torch.randn(2, 3, T, 56, 56)
    vm = torch.zeros(2, 1, 7, 7, dtype=torch.long)
    vm[0, 0, 1:4, 2:6] = 1
    vm[1, 0, 4:, 0:3] = 1
    vm[1, 0, 0, 6] = 1
    P = {'backbone.' + k: v.detach().float() for k, v in m.state_dict().items() if 'relative_position_index' not in k}
    ocfg = dict(patch_size=patch, embed_dim=48, depths=[2, 2], num_heads=[3, 6], window_size=(8, 7, 7))
    with torch.no_grad():
        ref = om.swin_forward(P, 'backbone.', x, ocfg)
        refm, refw = om.swin_forward(P, 'backbone.', x, ocfg, mask=vm)
    return m.to(DEV), x.to(DEV), vm.to(DEV), ref, refm, refw, patch


def test_swin_forward_matches_oracle(swin_case):
    """The bound of the Swin forward tests on the 16-bit path (tests/test_step_gpu.py::test_swin_backbone,
    test_swin_padded_sizes): 3e-2 of the largest reference value."""
    m, x, vm, ref, refm, refw, patch = swin_case
    with torch.no_grad():
        y = m(x)
        ym, w = m(x.clone(), vm)
        yb = m.forward_both(x, vm)
    Tp = -(-x.shape[2] // patch[0])
    assert tuple(y.shape) == tuple(ref.shape) and y.shape[2] == Tp
    assert rel(y, ref) < 3e-2, rel(y, ref)
    assert rel(ym, refm) < 3e-2, rel(ym, refm)
    assert torch.equal(w.float().cpu(), refw.float())                          # the blend map, bit for bit
    assert torch.equal(yb, torch.cat([y, ym], 0).permute(0, 2, 3, 4, 1))       # the stacked pass is the two passes


def test_swin_forward_parity_mode(swin_case):
    """The same in parity mode (fp32 HIP kernels) at the parity bound of tests/test_parity_gpu.py: 1e-4 of max."""
    from clover_amd import parity
    m, x, vm, ref, refm, refw, _ = swin_case
    with parity.mode(), torch.no_grad():
        y = m(x)
        ym, w = m(x.clone(), vm)
    assert rel(y, ref) < 1e-4, rel(y, ref)
    assert rel(ym, refm) < 1e-4, rel(ym, refm)
    assert torch.equal(w.float().cpu(), refw.float())


def test_patch_embed_module_overlap_parity_and_16bit():
    """stride (1,4,4) under patch (2,4,4) at the module: the 16-bit kernel and the parity path (unfold) against conv3d.
    Bounds: 2e-2 of max, what tests/test_kernels_gpu.py::test_patch_embed holds the (2,4,4) kernel's tokens to against the
    oracle; 1e-4 in parity mode (tests/test_parity_gpu.py::test_parity_modules_vs_reference)."""
    import torch.nn.functional as F
    from clover_amd import parity
    from clover_amd.backbones.swin_transformer_3d import PatchEmbed3D
    torch.manual_seed(7)
    pe = PatchEmbed3D(patch_size=(2, 4, 4), stride=(1, 4, 4), embed_dim=96).to(DEV)
    x = torch.randn(2, 3, 5, 28, 36, device=DEV)                               # 5 frames: padded to 6, T' = 5
    ref = F.conv3d(pe.pad(x).double(), pe.proj.weight.double(), pe.proj.bias.double(), stride=(1, 4, 4))
    assert tuple(ref.shape[2:]) == (5, 7, 9)
    with torch.no_grad():
        y = pe(x)
        with parity.mode():
            yp = pe(x)
    assert tuple(y.shape) == tuple(ref.shape)
    assert rel(y, ref) < 2e-2 and rel(yp, ref) < 1e-4, (rel(y, ref), rel(yp, ref))


# ----------------------------------------------------------------------------- the engine
def frame_token_model(patch, stride, frames, seed):
    """The model of configs/pretrain_frame_tokens_synthetic.py (Swin-T widths, BERT-base widths) with the depths cut down."""
    import bench
    import clover_amd
    from clover_amd.ops import patch_grid
    cfg = bench.model_cfg('T', frames)
    cfg['backbone'].update(patch_size=patch, stride=stride, depths=[1, 1, 1, 1], drop_path_rate=0.0)
    cfg['mm_backbone'].update(num_frames=patch_grid(frames, 224, 224, patch, stride)[0], num_hidden_layers=1)
    cfg['text_backbone'].update(num_hidden_layers=2)
    torch.manual_seed(seed)
    return clover_amd.build_model(cfg).to(DEV).eval()      # eval: dropout off -> deterministic trajectories


@pytest.mark.usefixtures('strict_own_gemm')
@pytest.mark.parametrize('patch,stride,frames', [((1, 4, 4), (1, 4, 4), 4), ((2, 4, 4), (1, 4, 4), 4), ((4, 4, 4), (4, 4, 4), 8)],
                         ids=['p144', 'p244s144', 'p444'])
def test_engine_graph_equals_eager_and_loss_decreases(patch, stride, frames):
    """As tests/test_engine_gpu.py::test_graph_capture_equals_eager_and_loss_decreases: the captured step follows the eager
    one within 5 % per step, and the loss falls; every GEMM, the conv weight gradient included, on the HIP kernels.
    num_frames = T' in every case ((4,4,4): 8 frames, T' = 2), and the fusion encoder's inputs prepared beside the text tower
    are built for that T' — the ones its forward then uses (their key matches), not rebuilt."""
    import bench
    from clover_amd import ops
    from clover_amd.engine import CloverEngine
    Tp = ops.patch_grid(frames, 224, 224, patch, stride)[0]
    b = {k: v.to(DEV) for k, v in bench.synthetic_batch(2, frames, 32, seed=21).items()}
    traj = {}
    for mode in ('eager', 'graph'):
        m = frame_token_model(patch, stride, frames, seed=300)
        assert m.backbone.patch_embed.proj.weight.shape[2:] == patch and m.backbone.patch_embed.stride == stride
        mb, keys = m.multimodal_backbone, []
        assert mb.num_frames == Tp
        real_prepare = mb.prepare

        def spy(*a, _real=real_prepare, _keys=keys):
            out = _real(*a)
            _keys.append(out['key'])
            return out
        mb.prepare = spy
        eng = CloverEngine(m, b, lr=2e-4, weight_decay=0.0, grad_clip=15.0, max_iters=10 ** 9)
        eng.step(b)
        if mode == 'graph':
            assert eng.capture(b)
            b_run = eng.input_buffers()
            assert b_run is not None
        else:
            b_run = b
        losses = []
        for _ in range(5):
            losses.append(float(eng.step(b_run)['log_vars']['loss']))
        traj[mode] = losses
        assert keys and all(k == (4, Tp, mb.spacial_tokens) for k in keys), (keys, Tp)     # 2B clips, T', 49
        del eng, m, mb
    print(patch, stride, traj)
    assert all(np.isfinite(v) for v in traj['eager'] + traj['graph']), traj
    for a, g in zip(traj['eager'], traj['graph']):
        assert abs(a - g) < 0.05 * max(1.0, abs(a)), traj
    assert traj['graph'][-1] < traj['graph'][0] and traj['eager'][-1] < traj['eager'][0], traj
    assert not ops.LIBRARY_GEMM_CALLS
