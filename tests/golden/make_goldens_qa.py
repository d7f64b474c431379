"""Golden vectors of the video-QA / fill-in-the-blank path — BUILD-CONTAINER ONLY.
Runs the REAL reference CloverFinetune(task='video_qa' / 'FIB') (imported through ref_harness.py) on the closed-form
weights and batches of qa_cases.py and writes g_qa.npz next to this file:

  per variant (mc: QA_MC_head over 5 candidates, oe: QA_OE_Head over 37 labels, fib: QA_OE_Head on the [MASK] row + the
  never-called ITMHead) and B in {2, 4}, in eval mode (dropout off): qa_loss, the gradients of qa_head.* and of
  qa_cases.GRAD_KEYS (strided subsamples, pack()), the count of parameters without a gradient, forward_test's result
  (full) and attention (subsample; transformers 5.x ignores output_attentions: the last fusion layer's eager attention
  weights are captured by a forward hook and averaged over heads, as 4.6.1's output['attentions'][-1].mean(dim=1)),
  and the reference's state_dict manifest;
  the heads alone at D = 768 on closed-form inputs: outputs and input / weight gradients for qa_cases.HEAD_CASES.

    python tests/golden/make_goldens_qa.py

The archive is written with fixed zip timestamps, so a rerun reproduces it byte for byte."""
import io
import json
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import closed_form as cf  # noqa: E402
import make_goldens as MG  # noqa: E402
import qa_cases as Q  # noqa: E402
import ref_harness as H  # noqa: E402


MAXSUB = 1024          # values per strided subsample (the fixture stays under 1 MiB)


def pack(out, name, t):
    """make_goldens.pack with MAXSUB values: a strided subsample + [sum, l2, numel]."""
    a = t.detach().cpu().double().numpy().reshape(-1)
    stride = max(1, a.size // MAXSUB)
    out[name + '.sub'] = a[::stride][:MAXSUB].astype(np.float32)
    out[name + '.stats'] = np.array([a.sum(), np.sqrt((a * a).sum()), a.size], dtype=np.float64)


def save_reproducible(fname, out):
    """np.savez_compressed with a fixed timestamp per member (byte-identical reruns)."""
    path = os.path.join(HERE, fname)
    with zipfile.ZipFile(path, 'w', compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(out[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())
    print(f'wrote {fname}: {len(out)} arrays, {os.path.getsize(path) / 1024:.1f} KiB')


def ref_qa_model(kind):
    H.install_shims()
    H.init_dist_single()
    import mmaction.models.heads.qa_head  # noqa: F401  (registers QA_MC_head / QA_OE_Head)
    m, manifest = MG.ref_model(cfg=Q.tiny_qa_cfg(kind))
    return m, manifest


def attention_hook(m):
    """Capture the last fusion layer's attention probabilities (eager attention, transformers 5.x)."""
    enc = m.multimodal_backbone.bert_encoder
    for mod in enc.modules():
        cfg = getattr(mod, 'config', None)
        if cfg is not None:
            cfg._attn_implementation = 'eager'
    store = {}

    def hook(_mod, _inp, output):
        store['p'] = output[1]
    enc.layer[-1].attention.self.register_forward_hook(hook)

    def enc_hook(_mod, _inp, output):      # what 4.6.1 returns with output_attentions=True (the last layer is read)
        output['attentions'] = (store['p'],)
        return output
    enc.register_forward_hook(enc_hook)
    return store


def gen_models(out):
    aux = ['token_ids', 'segment_ids', 'input_mask']
    for kind in Q.KINDS:
        m, manifest = ref_qa_model(kind)
        out[f'{kind}.manifest'] = np.array(json.dumps(manifest, sort_keys=True))
        store = attention_hook(m)
        m.eval()
        named = dict(m.named_parameters())
        for B in (2, 4):
            batch = Q.qa_batch(kind, B, f'qa.{kind}.B{B}')
            m.zero_grad(set_to_none=True)
            losses = m(batch['imgs'], batch['label'], return_loss=True, **{k: batch[k] for k in aux})
            losses['qa_loss'].backward()
            out[f'{kind}.B{B}.qa_loss'] = np.float64(losses['qa_loss'].item())
            for k in [n for n in named if n.startswith('qa_head.')] + Q.GRAD_KEYS:
                pack(out, f'{kind}.B{B}.grad.{k}', named[k].grad)
            out[f'{kind}.B{B}.n_unused'] = np.int64(sum(p.grad is None for p in named.values()))
            with torch.no_grad():
                res = m.forward_test(batch['imgs'], **{k: batch[k] for k in aux})
            MG.full(out, f'{kind}.B{B}.result', res['result'])
            pack(out, f'{kind}.B{B}.attention', store['p'].mean(dim=1))


def gen_heads(out):
    H.install_shims()
    from mmaction.models.heads.qa_head import QA_MC_head, QA_OE_Head
    for M, K in Q.HEAD_CASES:
        tag = f'head.M{M}.K{K}'
        head = QA_MC_head(768) if K == 1 else QA_OE_Head(768, num_labels=K)
        sd = cf.cf_state({k: list(v.shape) for k, v in head.state_dict().items()})
        head.load_state_dict(sd)
        head.eval()
        x = cf.cf_float(tag + '.x', (M, 768), 1.0).requires_grad_()
        y = head(x)
        dy = cf.cf_float(tag + '.dy', tuple(y.shape), 1.0)
        y.backward(dy)
        pack(out, tag + '.y', y)
        pack(out, tag + '.dx', x.grad)
        for n, p in head.named_parameters():
            pack(out, f'{tag}.grad.{n}', p.grad)


if __name__ == '__main__':
    torch.set_num_threads(8)
    torch.use_deterministic_algorithms(True)
    out = {}
    gen_models(out)
    gen_heads(out)
    save_reproducible('g_qa.npz', out)
