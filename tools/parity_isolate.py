"""Error isolation for the 1e-3 loss target: per-loss |delta| of the step against the reference
goldens (config 1, B = 4) and against the oracle at BASELINE config 2's shapes (B = 2), for
  fast            the bf16 training path,
  parity          fp32 storage + fp32 arithmetic (clover_amd/parity.py),
  parity+<kind>   parity mode with ONE bf16 rounding source re-injected (act / stream / weight / prob / input),
  parity+all      all five re-injected (should land near `fast`).
Writes gpurun_out/parity_isolate.json and prints a markdown table (pasted into DESIGN.md §2).

The fine-tuning losses get the same variants, all against the reference goldens (tests/golden/g_qa.npz, g_finetune.npz):
|qa_loss - reference| and max|result - reference| (forward_test's scores) for multiple choice / open-ended /
fill-in-the-blank at B = 2 and 4, and |retrieval_nce_loss - reference| at B = 2 and 4.  They are further entries of the
same JSON file and further tables (a `finetune` run alone is recorded as profiles/parity_isolate_finetune.json).
    python tools/parity_isolate.py [pretrain | finetune | all]           # on the GPU box; default: all
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

import torch  # noqa: E402

LOSS_KEYS = ['mlm_loss', 'nce_loss', 'rank_t_tm_loss', 'v_nce_loss', 'rank_v_vm_loss', 'loss']


def variants():
    from clover_amd import parity
    return [('fast', None), ('parity', ())] + [(f'parity+{k}', (k,)) for k in parity.ROUND_KINDS] + \
           [('parity+all', parity.ROUND_KINDS)]


def pretrain(out):
    import bench
    import closed_form as cf
    import gutil
    import clover_amd
    from clover_amd import parity
    from oracle import model as om
    dev = 'cuda'

    def run(model, batch, ref, tag):
        rows = {}
        for name, rounds in variants():
            with torch.no_grad():
                if rounds is None:
                    lv = model.train_step(batch, None)['log_vars']
                else:
                    with parity.mode(round=rounds):
                        lv = model.train_step(batch, None)['log_vars']
            rows[name] = {k: abs(lv[k] - ref[k]) for k in LOSS_KEYS}
        out[tag] = rows

    # config 1: reference goldens
    m = clover_amd.build_model(cf.tiny_model_cfg())
    m.load_state_dict(cf.cf_state(gutil.manifest()), strict=False)
    m = m.to(dev).eval()
    g = gutil.load('g_step.npz')
    for B in (1, 2, 4):
        batch = {k: v.to(dev) for k, v in cf.cf_batch(B, tag=f'step{B}').items()}
        run(m, batch, {k: float(g[f'B{B}.{k}']) for k in LOSS_KEYS}, f'config1_B{B}_vs_reference')

    # config 2 shapes: oracle
    torch.manual_seed(4321)
    cfg = bench.model_cfg('T', 8)
    m = clover_amd.build_model(cfg).eval()
    P = {k: v.detach().float() for k, v in m.state_dict().items() if 'relative_position_index' not in k}
    batch = bench.synthetic_batch(2, 8, 32, seed=77)
    torch.set_num_threads(max(1, min(32, len(os.sched_getaffinity(0)))))
    with torch.no_grad():
        _, ref = om.parse_losses(om.forward_train(P, batch, bench.oracle_cfg(cfg), gather=False))
    m = m.to(dev)
    run(m, {k: v.to(dev) for k, v in batch.items()}, ref, 'config2_shapes_B2_vs_oracle')



def finetune(out):
    """The fine-tuning tasks on the closed-form weights and batches of the goldens (eval mode: dropout off)."""
    import contextlib
    import numpy as np
    import closed_form as cf
    import gutil
    import qa_cases as Q
    import clover_amd
    from clover_amd import parity
    dev = 'cuda'
    aux = ['token_ids', 'segment_ids', 'input_mask']
    out.update({t: {name: {} for name, _ in variants()} for t in ('qa_loss_vs_reference', 'qa_result_vs_reference',
                                                                  'retrieval_nce_loss_vs_reference')})

    def each_variant():
        for name, rounds in variants():
            with torch.no_grad(), (contextlib.nullcontext() if rounds is None else parity.mode(round=rounds)):
                yield name

    g = gutil.load('g_qa.npz')
    for kind in Q.KINDS:
        m = clover_amd.build_model(Q.tiny_qa_cfg(kind))
        m.load_state_dict(cf.cf_state(json.loads(str(g[f'{kind}.manifest']))), strict=False)
        m = m.to(dev).eval()
        for B in (2, 4):
            batch = {k: v.to(dev) for k, v in Q.qa_batch(kind, B, f'qa.{kind}.B{B}').items()}
            col = f'{kind} B={B}'
            for name in each_variant():
                loss = float(m.train_step(batch)['log_vars']['qa_loss'])
                res = m(return_loss=False, imgs=batch['imgs'], **{k: batch[k] for k in aux})['result']
                out['qa_loss_vs_reference'][name][col] = abs(loss - float(g[f'{kind}.B{B}.qa_loss']))
                out['qa_result_vs_reference'][name][col] = float(
                    np.abs(res.double().cpu().numpy() - g[f'{kind}.B{B}.result']).max())

    g = gutil.load('g_finetune.npz')
    m = clover_amd.build_model(cf.tiny_finetune_cfg())
    m.load_state_dict({k: v for k, v in cf.cf_state(gutil.manifest()).items() if k in m.state_dict()}, strict=False)
    m = m.to(dev).eval()
    for B in (2, 4):
        batch = {k: v.to(dev) for k, v in cf.cf_batch(B, tag=f'ft{B}').items()}
        for name in each_variant():
            lv = m.train_step({k: batch[k] for k in ['imgs', 'label'] + aux}, None)['log_vars']
            out['retrieval_nce_loss_vs_reference'][name][f'B={B}'] = abs(lv['retrieval_nce_loss'] -
                                                                         float(g[f'train.B{B}.loss']))


def main(which='all'):
    assert which in ('pretrain', 'finetune', 'all'), which
    out = {}                                   # {tag: {variant: {column: |delta|}}}
    if which in ('pretrain', 'all'):
        pretrain(out)
    if which in ('finetune', 'all'):
        finetune(out)
    os.makedirs(os.path.join(ROOT, 'gpurun_out'), exist_ok=True)
    json.dump(out, open(os.path.join(ROOT, 'gpurun_out', 'parity_isolate.json'), 'w'), indent=1)
    for tag, rows in out.items():
        cols = list(next(iter(rows.values())))
        print(f'\n### {tag}\n| variant | ' + ' | '.join(cols) + ' |\n|---|' + '---|' * len(cols))
        for name, e in rows.items():
            print(f'| {name} | ' + ' | '.join(f'{e[k]:.1e}' for k in cols) + ' |')


if __name__ == '__main__':
    main(*sys.argv[1:2])
