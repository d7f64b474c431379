"""CPU-only checks of the host side: registry / plugin API, state_dict compatibility, the
index/geometry helpers against the reference goldens (bit-exact), the C ABI surface, and the
no-CPU-fallback rule."""
import ctypes
import os
import sys
import re

import numpy as np
import pytest
import torch

import closed_form as cf
import gutil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_registry_builds_reference_config_and_state_dict_matches_reference():
    import clover_amd
    from clover_amd.builder import MODELS
    for name in ['SwinTransformer3D', 'BertFromPretrained', 'CrossModalTransformerFromPretrained', 'NCEHeadForMM',
                 'NCEHeadForVision', 'NCEHeadForText', 'MLMHead', 'ExclusiveNCEwithRankingLoss',
                 'SoftmaxFocalLossMultiClass', 'CrossEntropyLoss', 'CloverPretrain']:
        assert name in MODELS, name
    m = clover_amd.build_model(cf.tiny_model_cfg())
    sd = m.state_dict()
    man = gutil.manifest()                     # names/shapes of the REFERENCE model's state_dict
    assert set(sd) == set(man)
    for k, shp in man.items():
        assert list(sd[k].shape) == shp, k
    assert m.aux_info == cf.AUX and m.fp16_enabled is False
    with pytest.raises(KeyError):
        clover_amd.build_backbone(dict(type='NoSuchBackbone'))
    with pytest.raises(ValueError):
        m(torch.zeros(1), None, return_loss=True)          # 'Label should not be None.'


FS = [(4, 56, 56), (8, 56, 56), (16, 56, 56), (2, 28, 28), (2, 14, 14), (4, 7, 7), (16, 7, 7), (16, 14, 14), (3, 10, 12)]


@pytest.mark.parametrize('fs', FS)
def test_window_geometry_bit_exact(fs):
    from clover_amd.backbones import swin_transformer_3d as S
    g = gutil.load('g_idx.npz')
    tag = '%d_%d_%d' % fs
    ws, ss = S.get_window_size(fs, (8, 7, 7), (4, 3, 3))
    assert list(ws) + list(ss) == g['gws_' + tag].tolist()
    ws2, ss2, rid = S.window_geometry(fs, (8, 7, 7), (4, 3, 3), 'cpu')
    assert (ws2, ss2) == (ws, ss)
    mask = g['mask_' + tag]
    if any(ss):
        r = rid.numpy()
        assert r.dtype == np.int32
        assert np.array_equal((r[:, :, None] != r[:, None, :]).astype(np.int8), mask)
    else:
        assert rid is None and not mask.any()


def _tok_row(D, H, W, ws, ss, wi, n):
    """Python transcription of the kernel's token addressing (attention.hip tok_row)."""
    nWh, nWw = H // ws[1], W // ws[2]
    wz, wr = divmod(wi, nWh * nWw)
    wy, wx = divmod(wr, nWw)
    tz, tr = divmod(n, ws[1] * ws[2])
    ty, tx = divmod(tr, ws[2])
    d = (wz * ws[0] + tz + ss[0]) % D
    h = (wy * ws[1] + ty + ss[1]) % H
    w = (wx * ws[2] + tx + ss[2]) % W
    return (d * H + h) * W + w


@pytest.mark.parametrize('fs', [(4, 56, 56), (16, 14, 14), (2, 28, 28), (4, 7, 7)])
def test_kernel_token_addressing_matches_roll_partition(fs):
    from clover_amd.backbones import swin_transformer_3d as S
    g = gutil.load('g_idx.npz')
    ws, ss = S.get_window_size(fs, (8, 7, 7), (4, 3, 3))
    part = g['part_%d_%d_%d' % fs]                      # reference roll(-shift) + window_partition of arange
    nW, N = part.shape
    for wi in list(range(0, nW, max(1, nW // 7))) + [nW - 1]:
        rows = [_tok_row(fs[0], fs[1], fs[2], ws, ss, wi, n) for n in range(N)]
        assert rows == part[wi].tolist()


def test_relative_position_index_and_blend_and_merge_order():
    from clover_amd.backbones import swin_transformer_3d as S
    g = gutil.load('g_idx.npz')
    for ws in [(8, 7, 7), (4, 7, 7), (2, 7, 7)]:
        assert np.array_equal(S.build_relative_position_index(ws).numpy(), g['rpi_%d_%d_%d' % ws])
    w = S.mask_blend_weight(torch.from_numpy(g['blend_mask']), 2, 28, 28)
    assert np.array_equal(w.numpy().astype(np.int8), g['blend_w'])
    cat = S.PatchMerging.merge_gather(torch.from_numpy(g['merge_in']))
    assert np.array_equal(cat.numpy(), g['merge_cat'])
    tid = torch.from_numpy(g['ssl_token_ids'])[:, 0]
    lab = torch.from_numpy(g['ssl_mlm_label'])[:, 0]
    assert np.array_equal(torch.where(lab == -100, tid, lab).numpy(), g['ssl_ids'])


def test_c_abi_exports_every_declared_symbol():
    from clover_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'clover_hip.h')).read()
    declared = set(re.findall(r'\b(clv_[a-z0-9_]+)\s*\(', hdr))
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    # both builds of the one ABI (fp16 element type = the default, bf16): every declared symbol, the same version, and each
    # says which element type it computes in (no compute call: there is no GPU here)
    pkg = os.path.dirname(_lib.LIB_PATH)
    for fname, half in (('libclover_hip_f16.so', 1), ('libclover_hip.so', 0)):
        so = ctypes.CDLL(os.path.join(pkg, fname))
        for name in declared:
            assert hasattr(so, name), (fname, name)
        assert so.clv_abi_version() == _lib.ABI_VERSION, fname
        assert so.clv_half_type() == half, fname
    assert os.path.basename(_lib.LIB_PATH) == ('libclover_hip_f16.so' if _lib.HALF_F16 else 'libclover_hip.so')
    assert _lib.lib().clv_abi_version() == _lib.ABI_VERSION
    from clover_amd import ops
    assert ops.OPTIM_STATE_BYTES == int(re.search(r'#define CLV_OPTIM_STATE_BYTES (\d+)', hdr).group(1))
    assert ctypes.sizeof(_lib.ClvAttnGeom) == 23 * 4 + 4 + 8 + 8  # 21 int32 + scale + dropout_p, padding, dbias_index + work pointers
    assert ctypes.sizeof(_lib.ClvWgradEntry) == 88                # ... + overwrite / pad (first-touch gradient sinks)
    assert ctypes.sizeof(_lib.ClvLnExtra) == 80                   # ... + q8 / qscale pointers (round 3)


def test_env_variable_census():
    """The environment variables the product reads are exactly the table of INTEGRATION.md section 4: every name handed to
    os.environ.get / os.environ[...] / os.getenv in clover_amd/**/*.py and to getenv (or the one helper around it,
    clv_env_int) in clover_amd/csrc/*.{hip,hpp}.  CLV_GEMM_TILE is allowed only inside the #ifdef GN_LAB block of
    gemm_nt.hip, which the shipped libraries do not compile."""
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    sect = doc[doc.index('## 4. Environment variables'):]
    documented = set(re.findall(r'^\| `((?:CLOVER|CLV)_[A-Z0-9_]+)` \|', sect, re.M))
    assert len(documented) == 19, sorted(documented)

    read, env_calls = set(), 0
    py_name = re.compile(r'''(?:os\.environ\.get\(|os\.environ\[|os\.getenv\(|environ\.get\(|getenv\()\s*(['"])([^'"]+)\1''')
    for dirpath, _, files in os.walk(os.path.join(ROOT, 'clover_amd')):
        for f in files:
            if f.endswith('.py'):
                src = open(os.path.join(dirpath, f)).read()
                src = re.sub(r'^\s*#.*$', '', src, flags=re.M)
                names = [m.group(2) for m in py_name.finditer(src)]
                # every access to the environment names its variable literally, so none escapes the census
                env_calls = len(re.findall(r'\benviron\b(?!\w)|\bgetenv\b', src))
                assert env_calls == len(names), (f, env_calls, names)
                read |= set(names)
    csrc = os.path.join(ROOT, 'clover_amd', 'csrc')
    c_name = re.compile(r'\b(?:getenv|clv_env_int)\s*\(\s*"([^"]+)"')
    for f in sorted(os.listdir(csrc)):
        if not f.endswith(('.hip', '.hpp')):
            continue
        lab = 0
        for line in open(os.path.join(csrc, f)):
            s = line.strip()
            if lab:                                             # inside #ifdef GN_LAB (the blocks hold no nested #if)
                lab = 0 if s.startswith('#endif') else 1
            elif s.startswith('#ifdef GN_LAB'):
                lab = 1
            code = line.split('//')[0]
            for name in c_name.findall(code):
                if name == 'CLV_GEMM_TILE':
                    assert lab and f == 'gemm_nt.hip', (f, line)
                else:
                    assert not lab, (f, line)
                    read.add(name)
            # getenv with a computed name: only inside the helper itself
            if re.search(r'\bgetenv\s*\(\s*[^"\s]', code):
                assert f == 'common.hpp' and 'getenv(name)' in code, (f, line)
    assert read == documented, (sorted(read - documented), sorted(documented - read))
    # the Makefile builds the shipped libraries without the lab macro
    assert 'GN_LAB' not in open(os.path.join(csrc, 'Makefile')).read()


def test_no_cpu_fallback_and_no_oracle_in_product():
    from clover_amd import ops
    x = torch.randn(4, 96)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.layer_norm(x, torch.ones(96), torch.zeros(96))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.gelu(x)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.linear(x, torch.randn(8, 96), None)
    for dirpath, _, files in os.walk(os.path.join(ROOT, 'clover_amd')):
        for f in files:
            if f.endswith('.py'):
                src = open(os.path.join(dirpath, f)).read()
                assert 'import oracle' not in src and 'from oracle' not in src, f


def test_optimizer_param_groups_and_lr_schedule():
    import clover_amd
    from clover_amd.engine import cosine_lr, paramwise_weight_decay
    m = clover_amd.build_model(cf.tiny_model_cfg())
    wd = paramwise_weight_decay(m, 0.005, 0.0, 0.0, {'absolute_pos_embed': dict(decay_mult=0.),
                                                    'relative_position_bias_table': dict(decay_mult=0.)})
    assert wd['backbone.layers.0.blocks.0.attn.relative_position_bias_table'] == 0.0      # custom key
    assert wd['backbone.layers.0.blocks.0.norm1.weight'] == 0.0                            # norm layer
    assert wd['backbone.layers.0.blocks.0.attn.qkv.bias'] == 0.0                           # bias
    assert wd['backbone.layers.0.blocks.0.attn.qkv.weight'] == 0.005
    assert wd['text_backbone.bert.embeddings.word_embeddings.weight'] == 0.005
    assert wd['multimodal_backbone.vis_space_pos'] == 0.005
    base = 1e-3
    assert abs(cosine_lr(base, 0, 100) - base) < 1e-12
    assert abs(cosine_lr(base, 100, 100) - base * 1e-3) < 1e-12
    assert abs(cosine_lr(base, 50, 100) - (base * 1e-3 + 0.5 * (base - base * 1e-3))) < 1e-12
    lr0 = cosine_lr(base, 0, 1000, warmup_iters=10, warmup_ratio=0.001)
    assert abs(lr0 - cosine_lr(base, 0, 1000) * 0.001) < 1e-12
    assert cosine_lr(base, 10, 1000, warmup_iters=10) == cosine_lr(base, 10, 1000)


def test_paramwise_lr_mult_and_fractional_decay():
    """mmcv DefaultOptimizerConstructor: custom_keys carry lr_mult AND decay_mult (any value), bias_lr_mult applies to
    non-norm biases; a custom-key hit switches the norm / bias rules off."""
    import clover_amd
    from clover_amd.engine import paramwise_options
    m = clover_amd.build_model(cf.tiny_model_cfg())
    o = paramwise_options(m, 0.01, dict(norm_decay_mult=0.0, bias_decay_mult=0.0, bias_lr_mult=2.0, custom_keys={
        'backbone.layers': dict(lr_mult=0.1, decay_mult=0.5), 'relative_position_bias_table': dict(decay_mult=0.)}))
    assert o['backbone.layers.0.blocks.0.attn.relative_position_bias_table'] == (0.0, 1.0)   # longest key wins
    assert o['backbone.layers.0.blocks.0.attn.qkv.weight'] == (0.005, 0.1)
    assert o['backbone.layers.0.blocks.0.attn.qkv.bias'] == (0.005, 0.1)          # custom key: bias rule is off
    assert o['backbone.layers.0.blocks.0.norm1.weight'] == (0.005, 0.1)           # ... and the norm rule
    assert o['text_backbone.bert.encoder.layer.0.output.dense.bias'] == (0.0, 2.0)
    assert o['text_backbone.bert.encoder.layer.0.output.LayerNorm.bias'] == (0.0, 1.0)
    assert o['text_backbone.bert.encoder.layer.0.output.dense.weight'] == (0.01, 1.0)


def test_lr_follows_runner_iter_in_two_loader_mode():
    """the reference's LR hook reads runner.iter, which the two-loader runner advances once per batch
    INDEX (clover_runner.py:76-91), so both loaders' steps of an index share one LR, the first step uses iter 0 and
    warm-up lasts warmup_epochs x len(longest loader) indices.  Checked against mmcv's formula written out."""
    import math
    from clover_amd.runner import CloverRunner, LrUpdaterHook

    class Stepper(_FakeStepper):
        def __init__(self):
            super().__init__()
            self.lrs = []

        def set_lr(self, lr):
            self._lr = lr

        def train_step(self, batch, opt):
            self.lrs.append(self._lr)
            return super().train_step(batch, opt)
    A, B = [f'a{i}' for i in range(6)], [f'b{i}' for i in range(4)]
    base, epochs, warm_epochs = 1e-3, 3, 1
    st = Stepper()
    r = CloverRunner(st, max_epochs=epochs)
    r.register_hook(LrUpdaterHook(base, min_lr_ratio=1e-3, warmup='linear', warmup_iters=warm_epochs,
                                  warmup_ratio=0.001, warmup_by_epoch=True))
    r.run([A, B], [('train', 1)], epochs)
    max_iters, warm = epochs * len(A), warm_epochs * len(A)

    def mmcv_lr(it):
        end = base * 1e-3
        lr = end + 0.5 * (base - end) * (1 + math.cos(math.pi * it / max_iters))          # annealing_cos
        if it < warm:
            k = (1 - it / warm) * (1 - 0.001)                                                # get_warmup_lr 'linear'
            lr = lr * (1 - k)
        return lr
    want = [mmcv_lr(i) for i in range(max_iters) for _ in range(2)]                         # two steps per index
    assert len(st.lrs) == len(want) == 36
    assert max(abs(a - b) for a, b in zip(st.lrs, want)) < 1e-15
    assert st.lrs[0] == mmcv_lr(0) and st.lrs[0] < base * 2e-3                              # iter 0, not 1
    assert st.lrs[2 * warm] == mmcv_lr(warm) and st.lrs[-1] > base * 1e-3                   # never clamped early


def test_bert_loader_maps_legacy_checkpoint_names(tmp_path, monkeypatch):
    """the stock bert-base-uncased file names LayerNorm params gamma / beta and the MLM output bias
    ``cls.predictions.bias``; from_pretrained (bert_from_hugface.py:13-15, mlm_itm_head.py:33-35) renames / ties
    them.  A fake checkpoint in the OLD naming must initialise every parameter; a partial one must raise."""
    from clover_amd.backbones.bert_from_hugface import BertFromPretrained
    from clover_amd.backbones.cross_transformer import CrossModalTransformerFromPretrained
    from clover_amd.heads.mlm_itm_head import MLMHead
    bc = dict(vocab_size=50, hidden_size=16, num_hidden_layers=2, num_attention_heads=2, intermediate_size=32,
              max_position_embeddings=24)
    src = BertFromPretrained(None, bert_config=bc, num_hidden_layers=2)
    g = torch.Generator().manual_seed(3)
    new = {'bert.' + k: torch.randn(v.shape, generator=g) for k, v in src.bert.state_dict().items()}
    new.update({'cls.predictions.transform.dense.weight': torch.randn(16, 16, generator=g),
                'cls.predictions.transform.dense.bias': torch.randn(16, generator=g),
                'cls.predictions.transform.LayerNorm.weight': torch.randn(16, generator=g),
                'cls.predictions.transform.LayerNorm.bias': torch.randn(16, generator=g),
                'cls.predictions.bias': torch.randn(50, generator=g)})                     # no decoder.* keys at all
    old = {k.replace('LayerNorm.weight', 'LayerNorm.gamma').replace('LayerNorm.bias', 'LayerNorm.beta'): v
           for k, v in new.items()}
    assert any('gamma' in k for k in old)
    d = tmp_path / 'bert-base-uncased'
    d.mkdir()
    import json
    (d / 'config.json').write_text(json.dumps(bc))
    torch.save(old, str(d / 'pytorch_model.bin'))
    monkeypatch.chdir(tmp_path)                             # the MLM head's hard-coded 'bert-base-uncased' (:33)
    text = BertFromPretrained('bert-base-uncased', num_hidden_layers=2)
    for k, v in text.bert.state_dict().items():
        assert torch.equal(v, new['bert.' + k]), k
    fuse = CrossModalTransformerFromPretrained('bert-base-uncased', hidden_size=16, img_in_size=16, num_frames=2,
                                               spacial_tokens=4, num_hidden_layers=1, use_text_cls=True)
    assert torch.equal(fuse.bert_encoder.layer[0].output.LayerNorm.weight,
                       new['bert.encoder.layer.0.output.LayerNorm.weight'])
    assert torch.equal(fuse.bert_embedding.LayerNorm.bias, new['bert.embeddings.LayerNorm.bias'])
    head = MLMHead(16, 50)
    assert torch.equal(head.predictions.decoder.bias, new['cls.predictions.bias'])          # tied bias
    assert torch.equal(head.predictions.decoder.weight, new['bert.embeddings.word_embeddings.weight'])   # tied weight
    assert torch.equal(head.predictions.transform.LayerNorm.weight, new['cls.predictions.transform.LayerNorm.weight'])
    # a checkpoint that lacks a parameter must not load silently
    broken = {k: v for k, v in old.items() if 'layer.1.output.LayerNorm.beta' not in k}
    torch.save(broken, str(d / 'pytorch_model.bin'))
    with pytest.raises(RuntimeError, match='not found in the checkpoint'):
        BertFromPretrained('bert-base-uncased', num_hidden_layers=2)


def test_lazy_log_vars_and_parse_losses():
    from clover_amd.recognizers.base import BaseRecognizer, LazyLogVars
    lv = LazyLogVars(['a_loss', 'b'], torch.tensor([1.5, 2.0]))
    assert list(lv.keys()) == ['a_loss', 'b'] and lv['a_loss'] == 1.5 and dict(lv.items())['b'] == 2.0

    class R(BaseRecognizer):
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.lazy_log_vars = False

        def forward_train(self, *a, **k):
            pass

        def forward_test(self, *a, **k):
            pass
    loss, log_vars = R()._parse_losses({'mlm_loss': torch.tensor(1.0), 'acc': torch.tensor(0.5),
                                        'x_loss': [torch.tensor([1.0, 3.0])]})
    assert float(loss) == 3.0 and log_vars['loss'] == 3.0 and log_vars['acc'] == 0.5     # 'acc' not summed


def test_swin_2d_to_3d_inflation_matches_reference():
    """SwinTransformer3D.inflate_weights vs the reference's own function run on the same synthetic 2-D
    checkpoint (tests/golden/make_goldens.py::gen_inflate): patch-embed repeat / patch_t, table tiling (2wd-1),
    bicubic 23x23 -> 13x13 resize, dropped buffers, head-count mismatch skipped at load."""
    import clover_amd
    from clover_amd.builder import build_backbone
    g = gutil.load('g_inflate.npz')
    cfg = cf.tiny_model_cfg()['backbone']
    bb = build_backbone(dict(cfg))
    sd = bb.inflate_state_dict(cf.inflate_checkpoint_2d())
    assert sorted(sd) == sorted(str(k) for k in g['__keys__'])
    for k in sd:
        ref = g[k]
        assert tuple(sd[k].shape) == ref.shape, k
        assert np.abs(sd[k].numpy() - ref).max() <= 1e-6 * max(1.0, np.abs(ref).max()), k
    before = bb.layers[1].blocks[1].attn.relative_position_bias_table.detach().clone()
    missing, unexpected, bad = bb.inflate_weights(cf.inflate_checkpoint_2d())
    assert bad == ['layers.1.blocks.1.attn.relative_position_bias_table'] and not unexpected
    assert torch.equal(bb.layers[1].blocks[1].attn.relative_position_bias_table, before)       # left untouched
    assert torch.allclose(bb.layers[1].blocks[0].attn.relative_position_bias_table,
                          torch.from_numpy(g['layers.1.blocks.0.attn.relative_position_bias_table']), atol=1e-6)
    assert torch.allclose(bb.patch_embed.proj.weight, torch.from_numpy(g['patch_embed.proj.weight']), atol=1e-7)


# ----------------------------------------------------------------------------- runner / config
def test_config_base_merge_and_cfg_options(tmp_path):
    from clover_amd.runner import Config, parse_cfg_options, scaled_lr
    (tmp_path / 'base.py').write_text("model = dict(type='X', backbone=dict(depth=2, width=8), head=dict(a=1))\n"
                                      "total_epochs = 3\nlog_config = dict(interval=10)\n")
    (tmp_path / 'child.py').write_text("_base_ = ['base.py']\nvideos_per_gpu = 4\n"
                                       "model = dict(backbone=dict(depth=4), head=dict(_delete_=True, b=2))\n"
                                       "optimizer = dict(type='AdamW', base_lr=1e-4, weight_decay=0.1)\n")
    cfg = Config.fromfile(str(tmp_path / 'child.py'))
    assert cfg.model.type == 'X' and cfg.model.backbone == dict(depth=4, width=8)      # recursive merge
    assert cfg.model.head == dict(b=2)                                                # _delete_ replaces
    assert cfg.total_epochs == 3 and cfg.log_config.interval == 10
    cfg.merge_from_dict(parse_cfg_options(['model.backbone.width=16', 'total_epochs=1', 'tag=run7', 'x.y=[1,2]']))
    assert cfg.model.backbone.width == 16 and cfg.total_epochs == 1 and cfg.tag == 'run7' and cfg.x.y == [1, 2]
    # linear scaling rule, tools/train.py:160-166: base_lr is popped, lr = base_lr * videos_per_gpu * world_size
    assert abs(scaled_lr(cfg, 8) - 1e-4 * 4 * 8) < 1e-12 and 'base_lr' not in cfg.optimizer
    assert scaled_lr(cfg, 2) == cfg.optimizer['lr']                                   # second call: nothing to scale


class _FakeStepper(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.seen = []

    def train_step(self, batch, optimizer):
        self.seen.append(batch)
        return dict(loss=torch.tensor(float(len(self.seen))), log_vars=dict(loss=float(len(self.seen))), num_samples=1)


def test_runner_multi_loader_interleave_and_hooks(tmp_path):
    """clover_runner.py:60-96: one step per loader per batch index; once the shorter loader runs out it is
    restarted and from then on EVERY slot of a row draws from the restarted iterator (the longer loader's own batch
    of that row is dropped) — reproduced, it decides which samples the reference trains on."""
    from clover_amd.runner import CheckpointHook, CloverRunner, Hook, LogHook
    A, B = [f'a{i}' for i in range(5)], [f'b{i}' for i in range(3)]
    calls = []

    class Spy(Hook):
        def before_run(self, r): calls.append('before_run')
        def before_train_epoch(self, r): calls.append('before_epoch')
        def before_train_iter(self, r): calls.append('bi')
        def after_train_iter(self, r): calls.append('ai')
        def after_train_epoch(self, r): calls.append('after_epoch')
        def after_run(self, r): calls.append('after_run')
    m = _FakeStepper()
    r = CloverRunner(m, max_epochs=1, work_dir=str(tmp_path))
    log = LogHook(interval=1)
    for h in (Spy(), log, CheckpointHook(str(tmp_path))):
        r.register_hook(h)
    r.run([A, B], [('train', 1)], 1)
    assert m.seen == ['a0', 'b0', 'a1', 'b1', 'a2', 'b2', 'a3', 'b0', 'b1', 'b2']
    assert r.iter == 5 and r.epoch == 1                      # :91 counts batch indices
    assert calls == ['before_run', 'before_epoch'] + ['bi', 'ai'] * 10 + ['after_epoch', 'after_run']
    assert [rec['loss'] for rec in log.records] == [float(i) for i in range(1, 11)]
    # single loader mode (:17-35) and the checkpoint layout {'meta','state_dict','optimizer'?}
    m2 = _FakeStepper()
    r2 = CloverRunner(m2, max_epochs=2, work_dir=str(tmp_path))
    r2.run([A], [('train', 1)])
    assert m2.seen == A + A and r2.iter == 10 and r2.epoch == 2
    ck = torch.load(str(tmp_path / 'epoch_1.pth'))
    assert set(ck) >= {'meta', 'state_dict'} and ck['meta']['epoch'] == 1 and 'w' in ck['state_dict']
    r3 = CloverRunner(_FakeStepper(), max_epochs=3)
    r3.resume(str(tmp_path / 'epoch_1.pth'))
    assert r3.epoch == 1 and r3.iter == 5


def test_runner_short_loader_runs_dry_like_the_reference():
    """With too short a second loader the restarted iterator is exhausted mid-epoch and `next()` raises — the
    reference has no guard (clover_runner.py:80-82) and neither has the drop-in."""
    from clover_amd.runner import CloverRunner
    r = CloverRunner(_FakeStepper(), max_epochs=1)
    with pytest.raises(StopIteration):
        r.run([['a0', 'a1', 'a2'], ['b0']], [('train', 1)])


# ----------------------------------------------------------------------------- retrieval metrics
def test_recall_for_video_text_retrieval_goldens():
    """clover_amd.evaluation against the reference's own metric values (g_finetune.npz; accuracy.py:430-462)."""
    from clover_amd.evaluation import normalize_fn, recall_for_video_text_retrieval
    g = gutil.load('g_finetune.npz')
    keys = ['Recall@1', 'Recall@5', 'Recall@10', 'MR', 'Recall@all']
    for N, D in ((1, 8), (7, 16), (50, 32), (200, 64)):
        ve = cf.cf_float(f'recall.N{N}.v', (N, D), 1.0).numpy()
        te = (0.35 * ve + cf.cf_float(f'recall.N{N}.t', (N, D), 1.0).numpy()).astype(np.float32)
        if N == 7:
            te[3] = 0
        m = recall_for_video_text_retrieval(ve, te)
        np.testing.assert_allclose([m[k] for k in keys], g[f'recall.N{N}'], rtol=0, atol=1e-9)
        mt = recall_for_video_text_retrieval(torch.from_numpy(ve), torch.from_numpy(te))      # tensors accepted
        assert mt == m
    sc = cf.cf_float('recall.scores', (12, 12), 1.0).numpy()
    m = recall_for_video_text_retrieval(input_scores=sc)
    np.testing.assert_allclose([m[k] for k in keys], g['recall.scores'], rtol=0, atol=1e-9)
    z = normalize_fn(np.array([[3.0, 4.0], [0.0, 0.0]]))
    assert np.array_equal(z, np.array([[0.6, 0.8], [0.0, 0.0]]))


def test_finetune_registered_and_refuses_without_gpu():
    """CloverFinetune / NormSoftmaxLoss are registry entries with the reference's constructor kwargs; the loss has
    no CPU path."""
    import clover_amd
    from clover_amd.builder import LOSSES, RECOGNIZERS
    assert 'CloverFinetune' in RECOGNIZERS.module_dict and 'NormSoftmaxLoss' in LOSSES.module_dict
    m = clover_amd.build_model(cf.tiny_finetune_cfg())
    assert m.task == 'retrieval' and m.loss_func.use_cos_similarity and m.loss_func.t == 0.05
    assert not any(k.startswith(('mlm_head', 'mlm_ssl')) for k in m.state_dict())
    with pytest.raises(RuntimeError):
        m.loss_func(torch.randn(4, 8), torch.randn(4, 8))


def test_tools_cli_host_side():
    """tools/train.py and tools/test.py: the reference's argument names parse, and the synthetic test loader shards the
    test set rank-major without losing or duplicating a pair (no GPU involved)."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mods = {}
    for name in ('train', 'test'):
        spec = importlib.util.spec_from_file_location(f'clv_tools_{name}', os.path.join(root, 'tools', f'{name}.py'))
        mods[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mods[name])
    argv = sys.argv
    try:
        sys.argv = ['train.py', 'cfg.py', '--work_dir', 'w', '--resume-from', 'a.pth', '--seed', '3', '--launcher', 'none',
                    '--cfg-options', 'total_epochs=1', 'optimizer.base_lr=0.1']
        a = mods['train'].parse_args()
        assert (a.config, a.work_dir, a.resume_from, a.seed, a.launcher) == ('cfg.py', 'w', 'a.pth', 3, 'none')
        assert a.cfg_options == ['total_epochs=1', 'optimizer.base_lr=0.1']
        sys.argv = ['test.py', 'cfg.py', 'ckpt.pth', '--eval', 'recall_for_video_text_retrieval', '--gpu-collect',
                    '--out', 'o.json']
        t = mods['test'].parse_args()
        assert (t.config, t.checkpoint, t.eval, t.out) == ('cfg.py', 'ckpt.pth', ['recall_for_video_text_retrieval'], 'o.json')
    finally:
        sys.argv = argv
    seen = []
    for rank in range(3):
        ld = mods['test'].SyntheticTestLoader(pairs=10, batch=2, frames=2, tokens=8, rank=rank, world=3, device='cpu')
        for b in ld:
            assert b['imgs'].shape[0] == b['index'].numel() == b['token_ids'].shape[0]
            seen += b['index'].tolist()
    assert sorted(seen) == list(range(10))


def test_grouped_weight_gradient_chunking():
    """ops.wgrad_chunks: <= 80 problems per launch, and two in-place problems (few rows, or a large 256-divisible output)
    with the same dW never in one launch — the in-place kernels add without atomics."""
    import torch
    from clover_amd import ops, _lib
    L = _lib.lib()
    assert L.clv_linear_wgrad_in_place(512, 768, 3072) == 1 and L.clv_linear_wgrad_in_place(3648, 768, 3072) == 1
    assert L.clv_linear_wgrad_in_place(12544, 384, 1536) == 0 and L.clv_linear_wgrad_in_place(3136, 768, 768) == 0
    assert L.clv_linear_wgrad_class(12544, 384, 384) == 0 and L.clv_linear_wgrad_class(3136, 768, 768) == 1
    assert L.clv_linear_wgrad_class(512, 768, 768) == 0                       # few-row problems stay on 128 x 128 tiles
    shared = torch.zeros(768, 768)
    other = [torch.zeros(768, 768) for _ in range(3)]
    item = lambda dw, M: ops.WgradItem(None, None, dw, None, M, 768, 768)
    # partial-mode uses of a shared dW may sit together in the GEMM launch (each writes its own partial buffer; their
    # folds are separated below) ...
    assert [len(c) for c in ops.wgrad_chunks([item(shared, 12544), item(shared, 12544), item(other[0], 512)])] == [3]
    # ... two in-place uses may not; an in-place + a partial-mode use may
    assert [len(c) for c in ops.wgrad_chunks([item(shared, 512), item(other[0], 512), item(shared, 640),
                                              item(shared, 12544), item(other[1], 512)])] == [2, 3]
    many = [item(torch.zeros(8, 8), 12544) for _ in range(175)]
    assert [len(c) for c in ops.wgrad_chunks(many)] == [80, 80, 15]
    # the folds of two partial-mode uses of ONE dW (or db) never share a launch: the fold kernel adds without atomics
    w = [torch.zeros(4) for _ in range(4)]
    fold = lambda dw, db=None: ops.FoldItem(torch.zeros(1), dw, db, 2, 2, 4)
    assert [len(c) for c in ops.fold_chunks([fold(shared), fold(other[0]), fold(shared), fold(other[1])])] == [2, 2]
    assert [len(c) for c in ops.fold_chunks([fold(other[0], w[0]), fold(other[1], w[0]), fold(other[2], w[1])])] == [1, 2]
    assert [len(c) for c in ops.fold_chunks([fold(torch.zeros(2, 2)) for _ in range(130)])] == [64, 64, 2]


def test_chunker_properties():
    """ops._chunks, the one rule that keeps the no-atomics batched kernels race-free, on seeded random item lists: the chunks
    concatenate to the input, none exceeds the cap, no conflict key appears twice in one, and the split is greedy (a chunk
    starts only where its first item would have broken the cap or met a key of the chunk before it)."""
    import random
    from clover_amd import ops
    rng = random.Random(20)
    for trial in range(400):
        cap = 1 + trial % 5
        items = [(i, frozenset(rng.sample('abcd', rng.choice((0, 0, 1, 1, 2))))) for i in range(rng.randrange(0, 24))]
        chunks = ops._chunks(items, cap, lambda it: it[1])
        assert [it for c in chunks for it in c] == items and all(chunks)
        for j, c in enumerate(chunks):
            assert len(c) <= cap
            keys = [k for it in c for k in it[1]]
            assert len(keys) == len(set(keys)), (trial, c)
            if j:
                before = chunks[j - 1]
                assert len(before) == cap or c[0][1] & {k for it in before for k in it[1]}, (trial, before, c[0])
    assert ops._chunks([], 3, lambda it: ()) == []


def test_segment_lifecycle(monkeypatch):
    """ops.defer_folds(): one open segment in ops.SEGMENT; a nested one flushes its own items at ITS exit and restores the
    outer one; a body that raises flushes nothing and restores the previous state; a clean exit runs grouped weight
    gradients, all folds (the ones those produced included), the post callables, LayerNorm reductions, table gathers — in
    that order; CLOVER_GROUP_WGRAD=0 leaves `wgrads` None and the other lists in place."""
    from clover_amd import ops
    log = []
    monkeypatch.setattr(ops, 'flush_wgrads', lambda p: (log.append(('wgrads', list(p))), ['made:%s' % i for i in p])[1])
    for name in ('flush_folds', 'flush_ln_reduces', 'flush_dbias_gathers'):
        monkeypatch.setattr(ops, name, lambda p, name=name: log.append((name[6:], list(p))))
    monkeypatch.delenv('CLOVER_GROUP_WGRAD', raising=False)

    def fill(tag):
        seg = ops.SEGMENT
        seg.dbias.append(tag + 'd'), seg.ln_reduces.append(tag + 'l'), seg.post.append(lambda: log.append(('post', tag)))
        seg.folds.append(tag + 'f'), seg.wgrads.append(tag + 'w')

    def flushed(tag):
        return [('wgrads', [tag + 'w']), ('folds', [tag + 'f', 'made:' + tag + 'w']), ('post', tag),
                ('ln_reduces', [tag + 'l']), ('dbias_gathers', [tag + 'd'])]
    assert ops.SEGMENT is None
    with ops.defer_folds():
        outer = ops.SEGMENT
        assert isinstance(outer, ops.Segment)
        fill('o')
        with ops.defer_folds():
            assert ops.SEGMENT is not outer and ops.SEGMENT.folds == []
            fill('i')
        assert ops.SEGMENT is outer and log == flushed('i')
        del log[:]
        with pytest.raises(KeyError):
            with ops.defer_folds():
                fill('x')
                raise KeyError('body')
        assert ops.SEGMENT is outer and log == []
    assert ops.SEGMENT is None and log == flushed('o')
    del log[:]
    with pytest.raises(KeyError):
        with ops.defer_folds():
            fill('x')
            raise KeyError('body')
    assert ops.SEGMENT is None and log == []
    monkeypatch.setenv('CLOVER_GROUP_WGRAD', '0')
    with ops.defer_folds():
        seg = ops.SEGMENT
        assert seg.wgrads is None and (seg.folds, seg.post, seg.ln_reduces, seg.dbias) == ([], [], [], [])
    assert [k for k, _ in log] == ['wgrads', 'folds', 'ln_reduces', 'dbias_gathers'] and all(p == [] for _, p in log)


def _sink_param(shape=(4, 8), sink_dtype=torch.float32):
    """A CPU parameter carrying the engine's attributes by hand: a zeroed sink and a counting ``_clv_ready``."""
    p = torch.nn.Parameter(torch.zeros(shape))
    p._clv_grad = torch.zeros(shape, dtype=sink_dtype)
    p.calls = []
    p._clv_ready = lambda: p.calls.append(1)
    return p


def test_gradient_sink_group_decision():
    """ops._sinks: all or nothing over a group — the ATTRIBUTE OBJECTS (aligned with the parameters, None for an absent
    one) when every present parameter has an fp32, contiguous sink, else None; the pad variant reads ``_clv_pad_grad``;
    ops._sink is the one-parameter form; a sink comes back still carrying its first-touch state."""
    from clover_amd import ops
    w, b, g = _sink_param(), _sink_param((4,)), _sink_param((8,))
    got = ops._sinks(w, None, b, g)
    assert isinstance(got, tuple) and len(got) == 4
    assert got[0] is w._clv_grad and got[1] is None and got[2] is b._clv_grad and got[3] is g._clv_grad
    assert ops._sinks(w) == (w._clv_grad,) and ops._sinks(w)[0] is w._clv_grad and ops._sinks() == () and ops._sinks(None) == (None,)
    assert ops._sink(w) is w._clv_grad and ops._sink(None) is None
    plain = torch.nn.Parameter(torch.zeros(4))
    assert ops._sinks(w, plain) is None and ops._sinks(plain, w) is None and ops._sink(plain) is None
    unset = _sink_param((4,))
    unset._clv_grad = None
    assert ops._sinks(w, unset) is None
    for dt in (torch.float16, torch.bfloat16):
        half = _sink_param((4,), dt)
        assert ops._sinks(w, half, g) is None and ops._sink(half) is None
    strided = _sink_param()
    strided._clv_grad = torch.zeros(8, 4).t()
    assert strided._clv_grad.shape == (4, 8) and not strided._clv_grad.is_contiguous()
    assert ops._sinks(w, b, strided) is None and ops._sink(strided) is None
    # identity: what hangs on the sink object is still there on what the helper hands out
    st = ops.FirstTouch()
    st.on = True
    w._clv_grad._clv_ft = st
    w._clv_grad._clv_ssq = ops.NormSlots(torch.zeros(1), torch.zeros(1), ops.FusedNormState())
    sk = ops._sinks(w, b)[0]
    assert sk._clv_ft is st and sk._clv_ssq.state.dirty is False and ops._sink(w)._clv_ft is st
    assert ops.first_touch(sk) and not ops.first_touch(ops._sink(w))          # one state: the second touch accumulates
    assert not ops.first_touch(w._clv_grad.view(8, 4))                           # (a view opts out: it carries no state)
    # the phantom-padded variant reads the padded view and nothing else
    assert ops._sinks(w, b, pad=True) is None
    w._clv_pad_grad, b._clv_pad_grad = torch.zeros(6, 8), torch.zeros(6)
    got = ops._sinks(w, b, pad=True)
    assert got[0] is w._clv_pad_grad and got[1] is b._clv_pad_grad and ops._sinks(w, b)[0] is w._clv_grad
    b._clv_pad_grad = torch.zeros(6, dtype=torch.bfloat16)
    assert ops._sinks(w, b, pad=True) is None


def test_gradient_sinks_delivered_once_each():
    """ops._delivered: ``_clv_ready`` of every present parameter exactly once, None skipped; a fused view's (as
    engine._Segment.fused_view builds it) reaches each member once."""
    from clover_amd import ops
    w, b, g = _sink_param(), _sink_param((4,)), _sink_param((8,))
    ops._delivered(w, None, b)
    assert (len(w.calls), len(b.calls), len(g.calls)) == (1, 1, 0)
    ops._delivered()
    ops._delivered(None, None)
    assert (len(w.calls), len(b.calls), len(g.calls)) == (1, 1, 0)
    q, k, v = _sink_param(), _sink_param(), _sink_param()
    f = torch.nn.Parameter(torch.zeros(12, 8))
    f._clv_grad = torch.zeros(12, 8)
    f._clv_members = [q, k, v]
    f._clv_ready = lambda ms=f._clv_members: [m._clv_ready() for m in ms] and None
    assert ops._sinks(f, None) == (f._clv_grad, None)
    ops._delivered(f, g)
    assert [len(m.calls) for m in (q, k, v, g)] == [1, 1, 1, 1]


def test_gradient_sink_census():
    """Only the helpers read the sink attributes: in the code of clover_amd/ops.py — comments and docstrings aside —
    ``_clv_grad`` appears in _sinks alone and ``_clv_ready`` in _delivered alone."""
    import ast
    import io
    import tokenize
    src = open(os.path.join(ROOT, 'clover_amd', 'ops.py')).read()
    tree = ast.parse(src)
    skip = set()                                # lines of docstrings
    for node in ast.walk(tree):
        if isinstance(node, (ast.Module, ast.ClassDef, ast.FunctionDef)) and ast.get_docstring(node, clean=False) is not None:
            skip.update(range(node.body[0].lineno, node.body[0].end_lineno + 1))
    owner = {}                                  # line -> name of the top-level function it lies in
    for node in tree.body:
        if isinstance(node, ast.FunctionDef):
            owner.update((ln, node.name) for ln in range(node.lineno, node.end_lineno + 1))
    found = {'_clv_grad': set(), '_clv_ready': set()}
    for tok in tokenize.generate_tokens(io.StringIO(src).readline):
        if tok.type == tokenize.COMMENT or tok.start[0] in skip:
            continue
        for name in found:
            if re.search(r'(?<![A-Za-z0-9])%s(?![A-Za-z0-9_])' % name, tok.string):
                found[name].add(owner.get(tok.start[0], '<module>:%d' % tok.start[0]))
    assert found == {'_clv_grad': {'_sinks'}, '_clv_ready': {'_delivered'}}, found


def test_segment_take_stream_wgrads(monkeypatch):
    """Segment.take_stream_wgrads (the by-stream split behind ops.flush_stream_wgrads): the items of one stream leave in
    their order, the others — those without a stream included — keep theirs; an absent stream takes nothing."""
    from clover_amd import ops
    monkeypatch.delenv('CLOVER_GROUP_WGRAD', raising=False)
    a, b = 0x7f00, 0
    seg = ops.Segment()
    items = [ops.WgradItem(None, None, None, None, 8 + i, 8, 8, stream=s) for i, s in enumerate((a, b, None, a, b))]
    seg.wgrads.extend(items)
    held = seg.wgrads
    assert seg.take_stream_wgrads(0x1234) == [] and seg.wgrads == items
    took = seg.take_stream_wgrads(a)
    assert len(took) == 2 and took[0] is items[0] and took[1] is items[3]
    assert seg.wgrads is held and len(held) == 3 and all(x is y for x, y in zip(held, (items[1], items[2], items[4])))
    assert seg.take_stream_wgrads(a) == [] and len(seg.wgrads) == 3
    assert items[2].stream is None and items[2].flags == 0 and ops.FoldItem(None, None, None, 2, 2, 4).flags == 0


def test_batch_caps_match_the_kernel_sources():
    """The per-launch caps the host chunks by (_lib.py) are the table sizes of the kernels: the #defines of
    include/clover_hip.h and WG_GROUP_MAX of gemm_wgrad.hip."""
    from clover_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'clover_hip.h')).read()
    defines = {k: int(v) for k, v in re.findall(r'^#define\s+(CLV_\w+_MAX)\s+(\d+)\s*$', header, re.M)}
    assert _lib.FOLD_MAX == defines['CLV_FOLD_MAX']
    assert _lib.LN_REDUCE_MAX == defines['CLV_LN_REDUCE_MAX']
    assert _lib.DBIAS_GATHER_MAX == defines['CLV_DBIAS_GATHER_MAX']
    wgrad = open(os.path.join(ROOT, 'clover_amd', 'csrc', 'gemm_wgrad.hip')).read()
    assert _lib.WGRAD_GROUP_MAX == int(re.search(r'constexpr int WG_GROUP_MAX = (\d+);', wgrad).group(1))


def test_fusion_text_outputs_and_token_mean_equal_autograd():
    """ops.fusion_text_outputs (one autograd node for the MLM decoder's input + the two reconstruction heads' CLS rows,
    multimodal_transformer_pretrain.py:129,148-149,156-157) and ops.token_mean (the vision head's spatial average,
    ssl_head.py:88-94) against the plain slice / unbind / select / mean expressions they replace: values and gradients, with
    both consumers, with either one alone (the ablation switches), in fp32 and bf16."""
    import torch
    from clover_amd import ops
    torch.manual_seed(3)
    B, S, L, D = 3, 11, 4, 8
    for dtype in (torch.float32, torch.bfloat16):
        h0 = torch.randn(2 * B, S, D).to(dtype)
        wt, wc = torch.randn(B, L, D), torch.randn(2, B, D)
        for use_t, use_c in ((True, True), (True, False), (False, True)):
            h = h0.clone().requires_grad_()
            t_last, cls = ops.fusion_text_outputs(h, S - L)
            assert t_last.is_contiguous() and t_last.dtype == dtype and cls.dtype == torch.float32
            loss = (t_last.float() * wt).sum() * use_t + (cls * wc).sum() * use_c
            loss.backward()
            hr = h0.clone().requires_grad_()
            t_all = hr[:, S - L:]
            tl, vf = t_all.unflatten(0, (2, B)).unbind(0)
            cr = torch.stack([tl[:, 0].float(), vf[:, 0].float()])
            lr = (tl.float() * wt).sum() * use_t + (cr * wc).sum() * use_c
            lr.backward()
            assert torch.equal(t_last, tl) and torch.equal(cls, cr)
            tol = 0.0 if dtype == torch.float32 else 2e-2       # (bf16: the CLS rows are added in fp32 here, in bf16 there)
            assert (h.grad.float() - hr.grad.float()).abs().max().item() <= tol * hr.grad.float().abs().max().item() + 1e-6
    for dtype in (torch.float32, torch.bfloat16):
        x0 = torch.randn(4, 2, 3, 3, D).to(dtype)
        w = torch.randn(4, D)
        x = x0.clone().requires_grad_()
        y = ops.token_mean(x)
        ((y * w).sum() + (x.float() ** 2).sum()).backward()     # a second consumer, as the fusion encoder is
        xr = x0.clone().requires_grad_()
        yr = xr.float().mean(dim=(1, 2, 3))
        ((yr * w).sum() + (xr.float() ** 2).sum()).backward()
        assert y.dtype == torch.float32 and (y - yr).abs().max().item() < 1e-6
        assert (x.grad.float() - xr.grad.float()).abs().max().item() <= 2e-2 * xr.grad.float().abs().max().item()


def test_sumsq_range_table_host_logic():
    """ops.sumsq_range_table (the block table of clv_sumsq_ranges): ranges are cut into blocks of <= CLV_SUMSQ_CHUNK floats,
    nothing is lost or counted twice, an empty list gives zero blocks."""
    from clover_amd import ops
    hdr = open(os.path.join(ROOT, 'include', 'clover_hip.h')).read()
    assert ops.SUMSQ_CHUNK == int(re.search(r'#define CLV_SUMSQ_CHUNK (\d+)', hdr).group(1))
    assert ops.SUMSQ_SLOTS == int(re.search(r'#define CLV_SUMSQ_SLOTS (\d+)', hdr).group(1))
    ranges = [(0, 7), (8, 8), (16, 40000), (40004, 40005), (100000, 300000)]
    tab, n = ops.sumsq_range_table(ranges, 'cpu')
    assert tab.shape == (n, 2) and int(tab[:, 1].max()) <= ops.SUMSQ_CHUNK
    covered = torch.zeros(300000, dtype=torch.int32)
    for off, cnt in tab.tolist():
        assert off % 4 == 0
        covered[off:off + cnt] += 1
    want = torch.zeros_like(covered)
    for a, b in ranges:
        want[a:b] = 1
    assert torch.equal(covered, want)
    tab0, n0 = ops.sumsq_range_table([], 'cpu')
    assert n0 == 0


@pytest.mark.parametrize('spans,total,want', [
    ([], 10, [(0, 10)]),                                             # no span: everything is left over
    ([], 0, []),
    ([(0, 3), (7, 10)], 10, [(3, 7)]),                               # spans touching both ends
    ([(2, 4), (4, 6), (9, 12)], 16, [(0, 2), (6, 9), (12, 16)]),     # adjacent spans leave no empty range between them
    ([(1, 8), (3, 5), (6, 11), (11, 11)], 14, [(0, 1), (11, 14)]),   # overlapping, nested and empty spans
    ([(0, 10)], 10, []),                                             # one span covering everything
])
def test_complement_of_spans_tiles_the_slab(spans, total, want):
    """engine._complement (the zero views of the first-touch scheme, the range tables of the fused norm): the ranges and
    the spans together cover every element of [0, total), no element lies in a range and a span or in two ranges, the
    ranges are in order and none is empty."""
    from clover_amd.engine import _complement
    ranges = _complement(spans, total)
    assert ranges == want
    assert all(0 <= a < b <= total for a, b in ranges)
    assert all(b0 < a1 for (_, b0), (a1, _) in zip(ranges, ranges[1:]))      # ordered, and not merely split in two
    in_span, in_range = np.zeros(total, dtype=np.int64), np.zeros(total, dtype=np.int64)
    for a, b in spans:
        in_span[a:b] = 1
    for a, b in ranges:
        in_range[a:b] += 1
    assert np.array_equal(in_span + in_range, np.ones(total, dtype=np.int64))


def test_bench_dump_outputs_fixed_sample(tmp_path):
    """bench.py --dump-outputs: the losses and the gradient norm as float64 scalars, the parameters and AdamW moments as
    float32 samples at indices fixed by the parameter names — the same arrays for two slab layouts of the same weights,
    within the size bound."""
    from types import SimpleNamespace
    sys.path.insert(0, ROOT)
    import bench
    g = torch.Generator().manual_seed(5)
    params = {'a.weight': torch.randn(300, 40, generator=g), 'b.bias': torch.randn(24, generator=g),
              'c.weight': torch.randn(8, 8, generator=g)}

    def engine(order):
        offs, n = [], 0
        for name in order:
            offs.append(n)
            n += (params[name].numel() + 7) // 8 * 8
        seg = SimpleNamespace(names=list(order), params=[params[k] for k in order], offsets=offs,
                              flat_p=torch.zeros(n), exp_avg=torch.zeros(n), exp_avg_sq=torch.zeros(n))
        for k, off in zip(order, offs):
            m = params[k].numel()
            seg.flat_p[off:off + m] = params[k].reshape(-1)
            seg.exp_avg[off:off + m] = 0.1 * params[k].reshape(-1)
            seg.exp_avg_sq[off:off + m] = params[k].reshape(-1) ** 2
        return SimpleNamespace(segments=[seg])
    out = dict(loss=torch.tensor(3.5), log_vars={'mlm_loss': 1.25, 'loss': 3.5})
    bench.dump_outputs(str(tmp_path / 'x'), engine(['a.weight', 'b.bias', 'c.weight']), out, 7.0)
    bench.dump_outputs(str(tmp_path / 'y'), engine(['c.weight', 'a.weight', 'b.bias']), out, 7.0)
    names = sorted(os.listdir(tmp_path / 'x'))
    assert names == sorted(os.listdir(tmp_path / 'y')) == sorted(
        ['loss.npy', 'log_mlm_loss.npy', 'log_loss.npy', 'grad_norm.npy', 'params.npy', 'exp_avg.npy', 'exp_avg_sq.npy'])
    for f in names:
        a, b = np.load(tmp_path / 'x' / f), np.load(tmp_path / 'y' / f)
        assert a.dtype == (np.float32 if f.startswith(('params', 'exp_avg')) else np.float64), f
        assert np.array_equal(a, b), f
    assert float(np.load(tmp_path / 'x' / 'log_mlm_loss.npy')) == 1.25 and float(np.load(tmp_path / 'x' / 'grad_norm.npy')) == 7.0
    p = np.load(tmp_path / 'x' / 'params.npy')
    assert p.size == min(12000, bench.DUMP_PER_PARAM) + 24 + 64
    assert np.isin(p[:bench.DUMP_PER_PARAM], params['a.weight'].numpy()).all()          # names in order: a, b, c
    assert np.array_equal(p[bench.DUMP_PER_PARAM:], torch.cat([params['b.bias'], params['c.weight'].reshape(-1)]).numpy())
    assert np.allclose(np.load(tmp_path / 'x' / 'exp_avg.npy'), 0.1 * p)
