"""clv_clip_prep on the MI355X, through ops.clip_prep: the exact class bit for bit, the general class against the fp64
reference of tests/clip_prep_ref.py within the bound of tests/CLIP_PREP_ERROR_BUDGET.md, independence of the samples, the
refusals, and a captured engine fed by PackedClipLoader through its static input buffer.  `-m gpu` only."""
import json
import os

import numpy as np
import pytest
import torch

import clip_prep_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
from clover_amd import _lib as _clv_lib  # noqa: E402
HALF = _clv_lib.half_dtype()
UNIT = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
MEAN, INV = R.constants()


def prep(src, boxes, flips, **kw):
    from clover_amd import ops
    return ops.clip_prep(torch.from_numpy(src).to(DEV), boxes, flips, R.MEAN, R.STD, **kw)


# ------------------------------------------------------------------------------------------------- exact class
@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('flip', [0, 1])
def test_box_of_exactly_s_by_s_is_bit_equal_to_torch(T, flip):
    """fx = fy = 0: the blend returns the tap itself, and the kernel's (v - mean[c]) * inv_std[c] — a subtract, then a
    multiply, both fp32 — is what torch computes below from the same fp32 constants."""
    S = 16
    rng = np.random.default_rng([11, T, flip])
    src = R.random_frames(rng, 2, T, 37, 53)
    boxes = np.asarray([(5, 7, 21, 23), (37, 21, 53, 37)], np.int32)             # different boxes per sample
    out = prep(src, boxes, [flip, flip], size=S)
    assert out.shape == (2, 1, 3, T, S, S) and out.dtype == torch.float32
    mean, inv = torch.from_numpy(MEAN).to(DEV), torch.from_numpy(INV).to(DEV)
    for b, (l, t, r, bt) in enumerate(boxes.tolist()):
        crop = torch.from_numpy(src[b, :, t:bt, l:r]).to(DEV).float()            # [T, S, S, 3]
        want = ((crop - mean) * inv).permute(3, 0, 1, 2)                         # [3, T, S, S]
        if flip:
            want = want.flip(-1)
        assert torch.equal(out[b, 0], want), (b, float((out[b, 0] - want).abs().max()))


# ------------------------------------------------------------------------------------------------- general class
_REF = {}


def _case(case):
    """Inputs and fp64 reference of a CASES entry, computed once and shared by both output types."""
    if case[0] not in _REF:
        src, boxes, flips = R.case_inputs(case)
        _REF[case[0]] = (src, boxes, flips, R.clip_prep_ref(src, boxes, flips, MEAN, INV, case[3]))
    return _REF[case[0]]


@pytest.mark.parametrize('dtype', [torch.float32, HALF], ids=['f32', 'half'])
@pytest.mark.parametrize('case', R.CASES, ids=[c[0] for c in R.CASES])
def test_general_class_within_the_derived_bound(case, dtype):
    src, boxes, flips, ref = _case(case)
    out = prep(src, boxes, flips, size=case[3], dtype=dtype)
    assert out.dtype == dtype and out.shape == ref.shape
    err = np.abs(out.double().cpu().numpy() - ref)
    tol = R.bound(ref, boxes, INV, UNIT[dtype])
    worst = float((err / tol).max())
    print(f'{case[0]} {dtype}: max |err| {err.max():.3e}, max err / bound {worst:.3f}')
    assert np.isfinite(err).all() and worst <= 1.0, (case[0], dtype, float(err.max()), worst)


def test_out_is_written_in_place_and_both_types_agree():
    case = R.CASES[1]
    src, boxes, flips, ref = _case(case)
    B, T, S = len(boxes), case[4], case[3]
    buf = torch.full((B, 1, 3, T, S, S), float('nan'), device=DEV)
    got = prep(src, boxes, flips, out=buf)
    assert got is buf and torch.equal(buf, prep(src, boxes, flips, size=S))
    half = prep(src, boxes, flips, size=S, dtype=HALF)
    assert torch.equal(half, buf.to(HALF))                                       # the same fp32 value, rounded once on store


# ------------------------------------------------------------------------------------------------- independence
def test_a_sample_does_not_depend_on_its_neighbours_box_or_flip():
    rng = np.random.default_rng(21)
    src = R.random_frames(rng, 2, 2, 37, 53)
    box1 = (3, 2, 50, 31)
    base = prep(src, [(0, 0, 53, 37), box1], [0, 1], size=16)
    for box0, flip0 in (((10, 5, 11, 30), 0), ((0, 0, 53, 37), 1), ((20, 20, 36, 36), 1)):
        out = prep(src, [box0, box1], [flip0, 1], size=16)
        assert torch.equal(out[1], base[1])
        assert not torch.equal(out[0], base[0])


# ------------------------------------------------------------------------------------------------- refusals
def test_refusals_are_raised_before_any_launch():
    rng = np.random.default_rng(22)
    src = R.random_frames(rng, 1, 1, 37, 53)
    with pytest.raises(NotImplementedError, match='CLV_CLIP_BAD_SIZE'):
        prep(src, [(0, 0, 53, 37)], [0], size=12)
    for box in ((0, 0, 54, 37), (-1, 0, 20, 20), (0, 0, 53, 38), (0, -2, 53, 37)):
        with pytest.raises(ValueError, match='leaves the 37 x 53 frame'):
            prep(src, [box], [0], size=16)
    with pytest.raises(NotImplementedError, match='CLV_CLIP_BAD_BOX'):
        prep(src, [(9, 9, 9, 20)], [0], size=16)
    with pytest.raises(NotImplementedError, match='CLV_CLIP_BAD_CHANNELS'):
        from clover_amd import ops
        ops.clip_prep(torch.zeros(1, 1, 8, 8, 4, dtype=torch.uint8, device=DEV), [(0, 0, 8, 8)], [0], R.MEAN, R.STD, size=8)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- engine path
def _write_dataset(path, batch, N, T, Hs, Ws):
    """N clips whose text rows are the closed-form batch of the engine tests."""
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, 'frames.npy'), R.random_frames(np.random.default_rng(31), N, T, Hs, Ws))
    np.savez(os.path.join(path, 'text.npz'), **{k: v.numpy() for k, v in batch.items() if k != 'imgs'})
    with open(os.path.join(path, 'meta.json'), 'w') as f:
        json.dump(dict(mean=list(R.MEAN), std=list(R.STD), channel_order='rgb'), f)


def test_engine_trains_from_the_static_buffer_exactly_as_from_eager_clips(tmp_path):
    """Two captured engines on identical models: one is fed by a PackedClipLoader that writes into the graph's static
    `imgs` buffer, the other gets the same clips as fresh tensors (ops.clip_prep without `out`) and runs the engine's own
    staging copy.  Same clips, same losses, bit for bit."""
    import closed_form as cf
    import gutil
    import clover_amd
    from clover_amd.engine import CloverEngine
    from clover_amd.utils.packed_loader import PackedClipDataset, PackedClipLoader
    B, T, S = 2, 4, 112
    text = cf.cf_batch(2 * B, frames=T, size=8, tag='packed')
    _write_dataset(str(tmp_path), text, 2 * B, T, 120, 136)
    ds = PackedClipDataset(str(tmp_path))
    losses = {}
    for mode in ('static', 'eager'):
        m = clover_amd.build_model(cf.tiny_model_cfg())
        m.load_state_dict(cf.cf_state(gutil.manifest()), strict=False)
        m = m.to(DEV).eval()                                                     # eval: no dropout, deterministic steps
        ld = PackedClipLoader(ds, B, DEV, train=True, seed=5, size=S)
        first = next(iter(ld))
        assert first['imgs'].shape == (B, 1, 3, T, S, S) and first['imgs'].dtype == torch.float32
        eng = CloverEngine(m, first, lr=2e-4, weight_decay=0.0, grad_clip=0.0, max_iters=10 ** 9)
        eng.dry_step(first)
        assert eng.capture(first)
        if mode == 'static':
            ld.engine = eng
        got = []
        for batch in ld:
            if mode == 'static':
                assert batch['imgs'] is eng.input_buffers()['imgs']
            else:
                assert batch['imgs'] is not eng.input_buffers()['imgs']
            got.append(eng.step(batch)['loss'].detach().clone())
        assert len(got) == 2 and ld.epoch == 1
        losses[mode] = torch.stack(got).cpu()
    print(losses)
    assert torch.isfinite(losses['static']).all() and torch.isfinite(losses['eager']).all()
    assert torch.equal(losses['static'], losses['eager']), losses
    assert float(losses['static'][0]) != float(losses['static'][1])              # two different batches were trained on
