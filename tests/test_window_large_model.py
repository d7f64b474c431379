"""SwinTransformer3D(window_size=(16, 7, 7)) on a 32-frame clip — 784-token windows, the 16-bit kernels' part path — against
the REAL reference's numbers (tests/golden/g_window_large.npz, written by tests/golden/make_goldens_window_large.py), and one
CloverEngine step of the tiny pre-training model with that window, eager and captured, against the oracle.

Geometry of the fixture: 16 x 14 x 14 tokens; stage 0 = four 784-token windows with shift (0, 3, 3) in its second block;
stage 1 (16 x 7 x 7 tokens) = one window, no shift.  The oracle test runs without a GPU; the others are marked `gpu`.
Tolerances are the ones the same comparisons have elsewhere: the oracle against a reference fixture as
tests/test_oracle_golden.py::test_swin (1e-4 forward, 2e-4 gradients); the module as tests/test_patch_embed_module_gpu.py and
tests/test_step_gpu.py (3e-2 of max on the 16-bit path, forward and backbone gradients: grad_tol) and 1e-4 in parity mode
(tests/test_parity_gpu.py, forward and gradients); the step's losses as tests/test_step_gpu.py LOSS_TOL.
"""
import json

import numpy as np
import pytest
import torch

import closed_form as cf
import gutil

DEV = 'cuda'
CFG = dict(embed_dim=48, depths=[2, 2], num_heads=[3, 6], window_size=(16, 7, 7))
GRADS = ['layers.0.blocks.0.attn.relative_position_bias_table', 'layers.0.blocks.0.attn.qkv.weight', 'patch_embed.proj.weight']
_CASE = {}


def fixture():
    """-> (golden, closed-form state rebuilt from the stored manifest, clip, output gradient); loaded once, never modified."""
    if not _CASE:
        g = gutil.load('g_window_large.npz')
        manifest = json.loads(str(g['manifest']))
        _CASE['v'] = (g, cf.cf_state(manifest), cf.cf_float('window_large.clip', (1, 3, 32, 56, 56), 1.0),
                      cf.cf_float('window_large.gw', (1, 96, 16, 7, 7), 1.0))
    return _CASE['v']


def rel(a, b):
    a = a.detach().float().cpu().numpy().astype(np.float64).reshape(-1)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-20)


def test_oracle_matches_the_reference_fixture():
    from oracle import indexing as ix
    from oracle import model as om
    g, sd, x, gw = fixture()
    assert ix.get_window_size((16, 14, 14), (16, 7, 7), (8, 3, 3)) == ((16, 7, 7), (0, 3, 3))       # stage 0, second block
    assert ix.get_window_size((16, 7, 7), (16, 7, 7), (8, 3, 3)) == ((16, 7, 7), (0, 0, 0))         # stage 1
    P = {'backbone.' + k: v.clone().requires_grad_() for k, v in sd.items()}
    y = om.swin_forward(P, 'backbone.', x, dict(patch_size=(2, 4, 4), **CFG))
    gutil.assert_close(y, g['out'], name='out')
    (y * gw).sum().backward()
    for k in GRADS:
        gutil.assert_close(P['backbone.' + k].grad, g['grad.' + k], rtol=2e-4, name='grad.' + k)
    # the first block's table: every row is reachable by a full (16, 7, 7) window
    assert int((g['grad.' + GRADS[0]] != 0).all(axis=1).sum()) == 31 * 13 * 13


def build_module():
    from clover_amd.backbones.swin_transformer_3d import SwinTransformer3D
    g, sd, x, gw = fixture()
    m = SwinTransformer3D(drop_path_rate=0.0, pretrained2d=False, **CFG)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert all('relative_position_index' in k for k in missing) and not unexpected, (missing, unexpected)
    m.eval()
    return m.to(DEV), g, x.to(DEV), gw.to(DEV)


@pytest.mark.gpu
def test_module_matches_the_reference_fixture():
    from clover_amd import ops
    m, g, x, gw = build_module()
    ops.LIBRARY_GEMM_CALLS.clear()
    y = m(x)
    assert tuple(y.shape) == g['out'].shape
    (y.float() * gw).sum().backward()
    torch.cuda.synchronize()
    errs = {'out': rel(y, g['out'])}
    named = dict(m.named_parameters())
    for k in GRADS:
        errs[k] = rel(named[k].grad, g['grad.' + k])
    print('window_large module rel errors', errs)
    for k, e in errs.items():
        assert e < 3e-2, (k, e)


@pytest.mark.gpu
def test_module_parity_mode_matches_the_reference_fixture():
    from clover_amd import parity
    m, g, x, gw = build_module()
    with parity.mode():
        y = m(x)
        (y.float() * gw).sum().backward()
    torch.cuda.synchronize()
    errs = {'out': rel(y, g['out'])}
    named = dict(m.named_parameters())
    for k in GRADS:
        errs[k] = rel(named[k].grad, g['grad.' + k])
    print('window_large parity rel errors', errs)
    for k, e in errs.items():
        assert e < 1e-4, (k, e)


# ----------------------------------------------------------------------------- the engine
def wide_window_cfg(which):
    cfg = cf.tiny_model_cfg() if which == 'tiny' else cf.mid_model_cfg()
    cfg['backbone'].update(window_size=(16, 7, 7))
    cfg['mm_backbone'].update(num_frames=16)                   # 32 frames / patch depth 2
    return cfg


_ORACLE = {}


def oracle_losses(which):
    if which not in _ORACLE:
        import clover_amd
        from oracle import model as om
        cfg = wide_window_cfg(which)
        manifest = {k: list(v.shape) for k, v in clover_amd.build_model(cfg).state_dict().items()}
        sd = cf.cf_state(manifest)
        batch = cf.cf_batch(2, frames=32, tag='window_large')
        with torch.no_grad():
            _, lv = om.parse_losses(om.forward_train(sd, batch, cf.oracle_cfg_from(cfg), gather=False))
        _ORACLE[which] = (cfg, sd, batch, {k: float(v) for k, v in lv.items()})
    return _ORACLE[which]


@pytest.mark.gpu
@pytest.mark.parametrize('which', ['tiny', 'mid'])
def test_engine_step_eager_and_captured(which, monkeypatch):
    """One CloverEngine step of the tiny pre-training model (tests/golden/closed_form.py tiny_model_cfg) with window_size =
    (16, 7, 7) on 32-frame 112-pixel clips — stage 0: sixteen 784-token windows per clip — eager and as replayed hipGraphs.
    The six losses of both are finite, within tests/test_step_gpu.py's LOSS_TOL of the oracle's, and within the same
    tolerance of each other (the same kernels on the same data: what differs is the order of the loss kernels' atomic sums).
    The step reaches every parameter it reaches with the (8, 7, 7) window: the unused ones are the seven the reference itself
    never uses (tests/golden/unused_params_tiny.json, what tests/test_engine_gpu.py pins), none of them in the backbone.

    Library GEMMs: the tiny model's widths (48 / 96, no multiples of 64) send its Linear layers to the ROCm library whatever
    the window (closed_form.mid_model_cfg's docstring), so `LIBRARY_GEMM_CALLS` cannot be empty there; what is asserted for
    it is that no entry is an attention fallback.  'mid' is the same model at the widths the HIP
    GEMMs take (mid_model_cfg: 96 / 192), run with CLOVER_STRICT_OWN_GEMM=1: there the table is empty."""
    import clover_amd
    from clover_amd import ops
    from clover_amd.engine import CloverEngine
    from test_step_gpu import LOSS_KEYS, LOSS_TOL
    cfg, sd, batch, lv_ref = oracle_losses(which)
    b = {k: v.to(DEV) for k, v in batch.items()}
    if which == 'mid':
        monkeypatch.setenv('CLOVER_STRICT_OWN_GEMM', '1')
    ops.LIBRARY_GEMM_CALLS.clear()
    got = {}
    for mode in ('eager', 'graph'):
        m = clover_amd.build_model(cfg)
        missing, unexpected = m.load_state_dict(sd, strict=False)
        assert all('relative_position_index' in k for k in missing) and not unexpected
        m = m.to(DEV).eval()
        eng = CloverEngine(m, b, lr=1e-4, weight_decay=0.005, grad_clip=15.0, max_iters=10 ** 6)
        assert sorted(eng.unused_names) == gutil.unused_params()
        assert not any(n.startswith('backbone.') for n in eng.unused_names)
        if mode == 'graph':
            assert eng.capture(b)
            out = eng._graphed_forward_backward(b)
        else:
            eng._ft.done.clear()
            out = m.train_step(b, None)
            eng._backward(lambda: out['loss'].backward())
        eng.finish_backward()
        torch.cuda.synchronize()
        got[mode] = {k: float(out['log_vars'][k]) for k in LOSS_KEYS}
        del eng, m
    print('window_large engine losses', got, 'oracle', {k: lv_ref[k] for k in LOSS_KEYS})
    for mode, lv in got.items():
        for k in LOSS_KEYS:
            assert np.isfinite(lv[k]), (mode, k, lv)
            assert abs(lv[k] - lv_ref[k]) <= LOSS_TOL[k], (mode, k, lv[k], lv_ref[k])
    for k in LOSS_KEYS:
        assert abs(got['eager'][k] - got['graph'][k]) <= LOSS_TOL[k], (k, got)
    if which == 'mid':
        assert not ops.LIBRARY_GEMM_CALLS, ops.LIBRARY_GEMM_CALLS
    else:
        assert not any('attention' in site for site, _ in ops.LIBRARY_GEMM_CALLS), ops.LIBRARY_GEMM_CALLS
    ops.LIBRARY_GEMM_CALLS.clear()
