"""Clip preparation without a GPU: the fp64 reference of tests/clip_prep_ref.py against closed forms, the crop boxes of
clover_amd/utils/packed_loader.py, the host-only plan / supported entries of the C ABI, and the packed dataset and loader
with the reference standing in for ops.clip_prep."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import clip_prep_ref as R
from clover_amd.utils import packed_loader as PL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, INV = R.constants()


def _norm(v):
    """(v - mean) * inv_std over the last (channel) axis of [..., 3], moved to the front as the clip layout has it."""
    return np.moveaxis((v.astype(np.float64) - MEAN.astype(np.float64)) * INV.astype(np.float64), -1, 0)


# ------------------------------------------------------------------------------------------------- the reference itself
def test_box_of_exactly_s_by_s_is_normalisation_alone():
    rng = np.random.default_rng(1)
    src = R.random_frames(rng, 2, 3, 37, 53)
    boxes = np.asarray([(5, 7, 21, 23), (37, 0, 53, 16)])
    out = R.clip_prep_ref(src, boxes, [0, 0], MEAN, INV, 16)
    for b, (l, t, r, bt) in enumerate(boxes.tolist()):
        for f in range(3):
            assert np.array_equal(out[b, 0, :, f], _norm(src[b, f, t:bt, l:r]))


def test_constant_frame_gives_constant_output():
    src = np.full((1, 2, 30, 41, 3), 77, np.uint8)
    for box in [(0, 0, 41, 30), (3, 4, 20, 29), (8, 8, 9, 9)]:
        out = R.clip_prep_ref(src, [box], [1], MEAN, INV, 24)
        want = _norm(np.full((1, 1, 3), 77))
        assert np.allclose(out[0, 0, :, 0], want, rtol=0, atol=1e-13) and np.allclose(out[0, 0, :, 1], want, rtol=0, atol=1e-13)


def test_affine_frame_is_reproduced_in_the_interior_and_clamped_at_the_border():
    ax, ay, c0 = 2, 3, 5
    src = R.ramp_frame(40, 60, ax, ay, c0)[None, None]
    l, t, r, b, S = 4, 6, 52, 30, 16                      # 48 x 24 -> 16 x 16: scale 3 in x, 1.5 in y
    out = R.clip_prep_ref(src, [(l, t, r, b)], [0], MEAN, INV, S)[0, 0, :, 0]
    sx = np.clip((np.arange(S) + 0.5) * (r - l) / S - 0.5, 0, r - l - 1) + l          # the CLAMPED sample positions
    sy = np.clip((np.arange(S) + 0.5) * (b - t) / S - 0.5, 0, b - t - 1) + t
    want = c0 + ax * sx[None, :] + ay * sy[:, None]
    for c in range(3):
        assert np.allclose(out[c], ((want + c) - float(MEAN[c])) * float(INV[c]), rtol=0, atol=1e-12)
    # an upscale: the outermost positions fall outside the first / last pixel centre and are clamped to them
    out = R.clip_prep_ref(src, [(10, 10, 14, 14)], [0], MEAN, INV, 16)[0, 0, 0, 0]
    raw = (np.arange(16) + 0.5) * 4 / 16 - 0.5
    assert raw[0] < 0 and raw[-1] > 3
    want = c0 + ax * (np.clip(raw, 0, 3)[None, :] + 10) + ay * (np.clip(raw, 0, 3)[:, None] + 10)
    assert np.allclose(out, (want - float(MEAN[0])) * float(INV[0]), rtol=0, atol=1e-12)
    assert out[0, 0] == out[0, 1] == out[1, 0] and out[0, 2] > out[0, 1]            # the clamp, and the ramp behind it


def test_flip_is_the_mirrored_output_and_twice_is_the_identity():
    rng = np.random.default_rng(2)
    src = R.random_frames(rng, 1, 2, 23, 31)
    box = [(2, 1, 29, 20)]
    plain = R.clip_prep_ref(src, box, [0], MEAN, INV, 8)
    flipped = R.clip_prep_ref(src, box, [1], MEAN, INV, 8)
    assert np.array_equal(flipped, plain[..., ::-1])
    assert np.array_equal(flipped[..., ::-1][..., ::-1], flipped) and np.array_equal(flipped[..., ::-1], plain)
    # the same through the source: a mirrored frame with the mirrored box, flipped, is the plain result
    msrc = np.ascontiguousarray(src[:, :, :, ::-1])
    mbox = [(31 - 29, 1, 31 - 2, 20)]
    assert np.allclose(R.clip_prep_ref(msrc, mbox, [1], MEAN, INV, 8), plain, rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------- boxes
@pytest.mark.parametrize('hw, S', [((27, 45), 24), ((45, 27), 24), ((63, 99), 56)])
def test_center_crop_box_equals_resize_then_center_crop(hw, S):
    """Resize(-1, S) + CenterCrop(S) as two fp64 resamples == ONE resample of center_crop_box (odd landscape / portrait
    frames whose rescaled long side and margins are whole numbers, S <= short side: the conditions of the docstring)."""
    h, w = hw
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    short = min(h, w)
    nh, nw = (S, w * S // h) if h <= w else (h * S // w, S)
    assert nw * h == w * S or nh * w == h * S                                 # a whole number
    resized = R.resample(img, (0, 0, w, h), (nh, nw))                         # Resize(-1, S): the whole frame
    oy, ox = (nh - S) // 2, (nw - S) // 2
    assert (nh - S) % 2 == 0 and (nw - S) % 2 == 0
    two_step = resized[oy:oy + S, ox:ox + S]                                  # CenterCrop(S)
    box = PL.center_crop_box(hw)
    assert box == ((w - short) // 2, (h - short) // 2, (w - short) // 2 + short, (h - short) // 2 + short)
    one_step = R.resample(img, box, (S, S))
    assert np.allclose(one_step, two_step, rtol=0, atol=1e-10)


def test_random_resized_crop_boxes_lie_in_the_frame_and_in_their_ranges():
    rng = np.random.default_rng(4)
    h, w = 256, 340
    area_range, ar_range = (0.08, 1.0), (3 / 4, 4 / 3)
    boxes = PL.random_resized_crop_boxes(rng, 500, (h, w), area_range, ar_range)
    assert boxes.dtype == np.int32 and boxes.shape == (500, 4)
    l, t, r, b = boxes.T
    assert (l >= 0).all() and (t >= 0).all() and (r <= w).all() and (b <= h).all() and (r > l).all() and (b > t).all()
    bw, bh = (r - l).astype(np.float64), (b - t).astype(np.float64)
    fallback = (bw == h) & (bh == h) & (l == (w - h) // 2) & (t == 0)
    acc = ~fallback
    assert acc.sum() > 400
    # np.round moves each side by at most 0.5: (bw +- 0.5)(bh +- 0.5) brackets the drawn area, likewise the ratio
    assert ((bw[acc] + 0.5) * (bh[acc] + 0.5) >= area_range[0] * h * w).all()
    assert ((bw[acc] - 0.5) * (bh[acc] - 0.5) <= area_range[1] * h * w).all()
    assert ((bw[acc] + 0.5) / (bh[acc] - 0.5) >= ar_range[0]).all() and ((bw[acc] - 0.5) / (bh[acc] + 0.5) <= ar_range[1]).all()
    assert len({tuple(q) for q in boxes.tolist()}) > 400                      # it is random


def test_random_resized_crop_fallback_is_the_centre_square():
    rng = np.random.default_rng(5)
    boxes = PL.random_resized_crop_boxes(rng, 20, (8, 400), area_range=(0.9, 1.0))        # no candidate is <= 8 high
    assert (boxes == np.asarray([196, 0, 204, 8])).all()
    boxes = PL.random_resized_crop_boxes(rng, 20, (400, 9), area_range=(0.9, 1.0))
    assert (boxes == np.asarray([0, 195, 9, 204])).all()


def test_random_resized_crop_same_seed_same_boxes():
    a = PL.random_resized_crop_boxes(np.random.default_rng(6), 50, (256, 340))
    b = PL.random_resized_crop_boxes(np.random.default_rng(6), 50, (256, 340))
    c = PL.random_resized_crop_boxes(np.random.default_rng(7), 50, (256, 340))
    assert np.array_equal(a, b) and not np.array_equal(a, c)


# ------------------------------------------------------------------------------------------------- the C ABI, host only
def test_symbols_in_header_binding_and_both_builds():
    from clover_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'clover_hip.h')).read()
    assert re.search(r'#define CLV_ABI_VERSION 20\b', hdr) and _lib.ABI_VERSION == 20          # new symbols only
    for name in ('clv_clip_prep_supported', 'clv_clip_prep_plan', 'clv_clip_prep'):
        assert re.search(r'\bint %s\(' % name, hdr) and name in _lib.SIGNATURES, name
        for fname in ('libclover_hip.so', 'libclover_hip_f16.so'):
            assert hasattr(C.CDLL(os.path.join(ROOT, 'clover_amd', fname)), name), (fname, name)
    assert C.sizeof(_lib.ClvClipPrepGeom) == 40 and C.sizeof(_lib.ClvClipPrepPlan) == 36
    from clover_amd import ops
    for rc, text in ops.CLIP_REASONS.items():
        name = text.split(':')[0]
        assert re.search(r'#define %s %d\b' % (name, rc), hdr), name


def test_plan_reaches_each_launch_class_at_the_sizes_of_the_gpu_test():
    from clover_amd import ops
    used = {case[3] for case in R.CASES} | {112}
    assert used == set(R.PLAN_CLASSES)
    for S, (cls, tail) in R.PLAN_CLASSES.items():
        for half in (False, True):
            pl = ops.clip_prep_plan(2, 3, 37, 53, S, half=half)
            assert (pl['cls'], pl['tail_rows']) == (cls, tail), (S, pl)
            assert pl['lanes_per_row'] == S // 8 and pl['block'] % 64 == 0 and pl['grid'] == 2 * 3 * pl['strips']
            assert pl['idle_lanes'] == pl['block'] - pl['lanes_per_row'] * pl['rows_per_pass'] >= 0
            rows = pl['rows_per_pass'] * pl['passes']
            assert (pl['strips'] - 1) * rows < S <= pl['strips'] * rows            # the strips cover the plane, none is empty
    assert {c for c, _ in R.PLAN_CLASSES.values()} == {R.PLANE, R.STRIPS}
    assert {t > 0 for c, t in R.PLAN_CLASSES.values() if c == R.STRIPS} == {True, False}
    pl = ops.clip_prep_plan(8, 8, 256, 340, 224)                                   # the bench geometry
    assert (pl['cls'], pl['block'], pl['lanes_per_row'], pl['rows_per_pass'], pl['passes'], pl['strips'], pl['grid'],
            pl['idle_lanes']) == (R.STRIPS, 256, 28, 9, 2, 13, 8 * 8 * 13, 4)
    assert ops.clip_prep_plan(1, 1, 9, 9, 8)['block'] == 64 and ops.clip_prep_plan(1, 1, 9, 9, 40)['block'] == 256
    assert ops.clip_prep_plan(1, 1, 9, 9, 40)['cls'] == R.PLANE and ops.clip_prep_plan(1, 1, 9, 9, 48)['cls'] == R.STRIPS


def test_supported_names_each_reason_and_the_entries_refuse():
    from clover_amd import _lib, ops
    lib = _lib.lib()
    assert lib.clv_clip_prep_supported(3, 37, 53, 16, 53, 37) == 0
    assert ops.clip_prep_refusal(4, 37, 53, 16).startswith('CLV_CLIP_BAD_CHANNELS')
    assert ops.clip_prep_refusal(3, 0, 53, 16).startswith('CLV_CLIP_BAD_FRAME')
    assert ops.clip_prep_refusal(3, 37, 0, 16).startswith('CLV_CLIP_BAD_FRAME')
    for S in (12, 0, 4, 2056):
        assert ops.clip_prep_refusal(3, 37, 53, S).startswith('CLV_CLIP_BAD_SIZE'), S
    for bw, bh in ((0, 5), (54, 5), (5, 0), (5, 38), (-3, 5)):
        assert ops.clip_prep_refusal(3, 37, 53, 16, bw, bh).startswith('CLV_CLIP_BAD_BOX'), (bw, bh)
    assert ops.clip_prep_refusal(3, 37, 53, 2048) is None and ops.clip_prep_refusal(3, 1, 1, 8, 1, 1) is None
    # the plan and the launcher refuse before anything is dereferenced or launched
    pl = _lib.ClvClipPrepPlan()
    g = _lib.ClvClipPrepGeom(B=1, T=1, Hs=37, Ws=53, C=3, S=12, out_dtype=0, pad=0, boxes_host=None)
    assert lib.clv_clip_prep_plan(C.byref(g), C.byref(pl)) == -2
    one = C.c_void_p(16)
    assert lib.clv_clip_prep(one, one, one, one, one, one, C.byref(g), None) == -2
    g.S, g.out_dtype = 16, 2
    assert lib.clv_clip_prep_plan(C.byref(g), C.byref(pl)) == -1
    g.out_dtype, g.B = 0, 0
    assert lib.clv_clip_prep_plan(C.byref(g), C.byref(pl)) == -1
    g.B = 1
    assert lib.clv_clip_prep_plan(C.byref(g), None) == -1 and lib.clv_clip_prep(None, one, one, one, one, one, C.byref(g), None) == -1
    assert lib.clv_clip_prep(one, one, one, one, one, C.c_void_p(8), C.byref(g), None) == -1          # out not 16-byte aligned
    # a host copy of the boxes: a box outside the frame is CLV_ERR_ARG, an empty one CLV_ERR_UNSUPPORTED, before any launch
    for box, rc in (((0, 0, 54, 37), -1), ((-1, 0, 5, 5), -1), ((5, 5, 5, 9), -2)):
        hb = (C.c_int32 * 4)(*box)
        g.boxes_host = C.cast(hb, C.c_void_p)
        assert lib.clv_clip_prep(one, one, one, one, one, one, C.byref(g), None) == rc, box


# ------------------------------------------------------------------------------------------------- dataset and loader
def _write_dataset(path, N=11, T=2, Hs=20, Ws=28, L=12, seed=0):
    import bench
    os.makedirs(path, exist_ok=True)
    rng = np.random.default_rng(seed)
    frames = R.random_frames(rng, N, T, Hs, Ws)
    frames[:, :, 0, 0, 0] = np.arange(N, dtype=np.uint8)[:, None]               # sample i carries i in its corner pixel
    np.save(os.path.join(path, 'frames.npy'), frames)
    b = bench.synthetic_batch(N, 1, L, seed, size=8)
    b['token_ids'][:, 0, 1] = 1000 + torch.arange(N)                             # ... and in its second token
    np.savez(os.path.join(path, 'text.npz'), **{k: v.numpy() for k, v in b.items() if k != 'imgs'})
    with open(os.path.join(path, 'meta.json'), 'w') as f:
        json.dump(dict(mean=list(R.MEAN), std=list(R.STD), channel_order='rgb'), f)
    return frames


def _ref_prep(calls):
    def prep(src, boxes, flips, mean, std, out=None, size=224, dtype=None):
        m, s = R.constants(mean, std)
        calls.append((src.numpy().copy(), np.asarray(boxes).copy(), np.asarray(flips).copy()))
        v = torch.from_numpy(R.clip_prep_ref(src.numpy(), np.asarray(boxes), np.asarray(flips), m, s, size)).float()
        if out is not None:
            return out.copy_(v)
        return v
    return prep


def test_packed_loader_batches_have_the_layout_of_the_synthetic_batch(tmp_path):
    import bench
    frames = _write_dataset(str(tmp_path), N=11, T=2, L=12)
    ds = PL.PackedClipDataset(str(tmp_path))
    assert len(ds) == 11 and isinstance(ds.frames, np.memmap) and ds.mean == R.MEAN and ds.std == R.STD
    calls = []
    ld = PL.PackedClipLoader(ds, 4, 'cpu', train=True, seed=3, size=16, prep=_ref_prep(calls))
    assert len(ld) == 2                                                          # 11 // 4: the last partial batch is dropped
    batches = list(ld)
    assert len(batches) == 2 and ld.epoch == 1
    want = bench.synthetic_batch(4, 2, 12, 0, size=16)
    for b in batches:
        assert set(b) == set(want)
        for k, v in want.items():
            assert b[k].shape == v.shape and b[k].dtype == v.dtype, k
    # the frames handed to the kernel are the samples the text rows belong to, and the boxes lie in the frame
    seen = []
    for b, (src, boxes, flips) in zip(batches, calls):
        ids = (b['token_ids'][:, 0, 1] - 1000).tolist()
        assert src[:, 0, 0, 0, 0].tolist() == ids and np.array_equal(src, frames[ids])
        assert boxes.shape == (4, 4) and (boxes[:, 0] >= 0).all() and (boxes[:, 2] <= 28).all() and (boxes[:, 3] <= 20).all()
        assert flips.shape == (4,) and set(flips.tolist()) <= {0, 1}
        seen += ids
    assert len(set(seen)) == 8
    # a second epoch draws another permutation; the same seed replays the first
    again = [b['token_ids'][:, 0, 1].tolist() for b in PL.PackedClipLoader(ds, 4, 'cpu', seed=3, size=16, prep=_ref_prep([]))]
    assert again == [b['token_ids'][:, 0, 1].tolist() for b in batches]
    assert [b['token_ids'][:, 0, 1].tolist() for b in ld] != again and ld.epoch == 2


def test_packed_loader_ranks_are_disjoint_and_the_test_split_keeps_order(tmp_path):
    _write_dataset(str(tmp_path), N=11)
    ds = PL.PackedClipDataset(str(tmp_path))
    per_rank = []
    for rank in range(2):
        ld = PL.PackedClipLoader(ds, 2, 'cpu', train=True, seed=9, rank=rank, world=2, size=8, prep=_ref_prep([]))
        assert len(ld) == 2                                                      # 11 // 2 = 5 per rank -> 2 batches of 2
        per_rank.append([int(i) - 1000 for b in ld for i in b['token_ids'][:, 0, 1]])
    assert len(per_rank[0]) == len(per_rank[1]) == 4 and not set(per_rank[0]) & set(per_rank[1])
    # train=False: every sample once, in order, centre box, no flip, `index`, the partial batch kept
    calls = []
    got = []
    for rank in range(2):
        ld = PL.PackedClipLoader(ds, 4, 'cpu', train=False, rank=rank, world=2, size=8, prep=_ref_prep(calls))
        for b in ld:
            assert (b['token_ids'][:, 0, 1] - 1000).tolist() == b['index'].tolist()
            got.append(b['index'].tolist())
    assert got == [[0, 2, 4, 6], [8, 10], [1, 3, 5, 7], [9]]
    for src, boxes, flips in calls:
        assert (boxes == np.asarray(PL.center_crop_box((20, 28)))).all() and not flips.any()
    assert PL.center_crop_box((20, 28)) == (4, 0, 24, 20)
    with pytest.raises(ValueError):
        PL.PackedClipLoader(ds, 16, 'cpu', train=True, prep=_ref_prep([]))       # not one whole batch
