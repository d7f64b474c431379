"""Training and evaluation on packed uint8 clips: the host side of ``ops.clip_prep``.

A packed directory holds pre-decoded frames (decoding is out of scope: no decoder is a dependency of this project):

    frames.npy   uint8 [N, T, Hs, Ws, 3], opened with mmap_mode='r'; frames pre-resized to the short side of the reference's
                 pipeline (256), so the device kernel does exactly the reference's single Resize to 224 on the crop
    text.npz     token_ids, segment_ids, input_mask [N, 1, L] (+ mlm_label, v_token_mask, label where the task needs them)
    meta.json    {"mean": [3], "std": [3], "channel_order": "rgb" | "bgr"} — mean / std in the stored channel order

The host draws one crop box and one flip flag per sample (the reference's RandomResizedCrop / Flip, or the centre box of
its test pipeline) and ``ops.clip_prep`` does crop, resize, flip, normalise and layout in one launch — into the captured
graph's static ``imgs`` buffer when the loader is bound to a captured ``CloverEngine``.
(Reference: mmaction/datasets/pipelines/augmentations.py RandomResizedCrop :863-1020, Resize :1202-1330, Flip :1385-1530,
Normalize :1532-1615, CenterCrop :1715-1812; formating.py FormatShape.)"""
import json
import os

import numpy as np
import torch

TEXT_KEYS = ('token_ids', 'segment_ids', 'input_mask')
OPTIONAL_KEYS = ('mlm_label', 'v_token_mask', 'label')


def random_resized_crop_boxes(rng, n, img_hw, area_range=(0.08, 1.0), aspect_ratio_range=(3 / 4, 4 / 3), max_attempts=10):
    """n crop boxes (left, top, right, bottom), int32 [n, 4]: RandomResizedCrop.get_crop_bbox (augmentations.py:894-942) per
    sample — `max_attempts` candidates with log-uniform aspect ratio and uniform area, w = round(sqrt(area * ratio)),
    h = round(sqrt(area / ratio)); the first candidate that fits the frame is placed uniformly; if none fits, the centred
    square of the short side.  `rng` is a numpy.random.Generator the caller owns (the reference draws from the global
    np.random / random state: the distribution and the fallback are restated, not the stream)."""
    assert 0 < area_range[0] <= area_range[1] <= 1 and 0 < aspect_ratio_range[0] <= aspect_ratio_range[1]
    img_h, img_w = int(img_hw[0]), int(img_hw[1])
    area = img_h * img_w
    out = np.empty((n, 4), np.int32)
    for k in range(n):
        ratios = np.exp(rng.uniform(np.log(aspect_ratio_range[0]), np.log(aspect_ratio_range[1]), size=max_attempts))
        areas = rng.uniform(area_range[0], area_range[1], size=max_attempts) * area
        cw = np.round(np.sqrt(areas * ratios)).astype(np.int32)
        ch = np.round(np.sqrt(areas / ratios)).astype(np.int32)
        for w, h in zip(cw.tolist(), ch.tolist()):
            if 1 <= h <= img_h and 1 <= w <= img_w:
                x = int(rng.integers(0, img_w - w + 1))
                y = int(rng.integers(0, img_h - h + 1))
                out[k] = (x, y, x + w, y + h)
                break
        else:
            s = min(img_h, img_w)
            x, y = (img_w - s) // 2, (img_h - s) // 2
            out[k] = (x, y, x + s, y + s)
    return out


def center_crop_box(img_hw):
    """The box of the test pipeline, Resize(-1, S) + CenterCrop(S): the centred square of the short side.

    Identity: resizing an h x w frame (h <= w) to S x w' with w' = w S / h and cutting columns [o, o + S), o = (w' - S) / 2,
    reads output column x at source position (o + x + 0.5) h / S - 0.5 = (w - h) / 2 + (x + 0.5) h / S - 0.5 — exactly ONE
    resample of the columns [(w - h) / 2, (w - h) / 2 + h) to S.  It holds to the bit when w' and both margins are whole
    numbers and h >= S (a downscale never reaches across the box edge); otherwise the reference's own rounding of w' and
    of the two margins moves the positions by less than one source pixel.  (Portrait frames likewise, rows for columns.)
    tests/test_clip_prep_ref_cpu.py pins it against a two-step fp64 resample."""
    h, w = int(img_hw[0]), int(img_hw[1])
    s = min(h, w)
    x, y = (w - s) // 2, (h - s) // 2
    return (x, y, x + s, y + s)


class PackedClipDataset:
    """A packed directory (module docstring): `frames` is the memory map, `text` the arrays of text.npz in memory."""

    def __init__(self, path):
        self.path = path
        self.frames = np.load(os.path.join(path, 'frames.npy'), mmap_mode='r')
        if self.frames.dtype != np.uint8 or self.frames.ndim != 5 or self.frames.shape[-1] != 3:
            raise ValueError(f'{path}/frames.npy: uint8 [N, T, Hs, Ws, 3] expected, got {self.frames.dtype} '
                             f'{self.frames.shape}')
        with np.load(os.path.join(path, 'text.npz')) as z:
            self.text = {k: np.asarray(z[k]) for k in z.files}
        with open(os.path.join(path, 'meta.json')) as f:
            self.meta = json.load(f)
        for k in TEXT_KEYS:
            if k not in self.text or self.text[k].shape[0] != len(self):
                raise ValueError(f'{path}/text.npz: `{k}` [N, 1, L] is required for all {len(self)} clips')
        self.mean, self.std = tuple(self.meta['mean']), tuple(self.meta['std'])

    def __len__(self):
        return self.frames.shape[0]


class PackedClipLoader:
    """Batches of a PackedClipDataset with the keys of tools/train.py's SyntheticLoader: imgs [B, 1, 3, T, size, size],
    label, token_ids, segment_ids, input_mask, mlm_label, v_token_mask (those the dataset holds; `label` defaults to
    zeros); with train=False imgs, the three text keys and `index`, as SyntheticTestLoader.

    train=True: one permutation per epoch (the same on every rank, seeded by (seed, epoch)), rank r takes every world-th
    sample, and the last partial batch is dropped — the engine's geometry is static.  Boxes come from
    random_resized_crop_boxes, flips with probability flip_ratio, both from one generator per (seed, rank, epoch).
    train=False: samples rank, rank + world, ... in order, the centre box, no flip, the last partial batch kept.

    Per batch: the frames are gathered from the memory map into one of TWO pinned uint8 staging tensors, copied
    `non_blocking` into the matching device uint8 buffer, and `prep` (ops.clip_prep) writes the clip — into the static
    `imgs` buffer of `engine`'s capture of this geometry when there is one (the batch's `imgs` IS that buffer, so the
    engine's `batch[k] is not v` check skips its staging copy), else into a new tensor.  The two staging / device pairs
    alternate, so the host gathers batch n + 1 while step n runs, and the copy goes to a stream of its own, so it runs
    under step n as well; events per pair order copy and kernel and keep the host from overwriting a staging tensor
    whose copy is still in flight.  No worker processes, no GPU work from threads.

    `prep(src_u8, boxes, flips, mean, std, out=..., size=..., dtype=...)` defaults to ops.clip_prep; a test hands in a
    host statement of it and device='cpu'."""

    def __init__(self, dataset, batch, device, train=True, flip_ratio=0.5, seed=0, rank=0, world=1, size=224, engine=None,
                 prep=None, dtype=None, area_range=(0.08, 1.0), aspect_ratio_range=(3 / 4, 4 / 3)):
        self.dataset, self.batch, self.device, self.train = dataset, int(batch), torch.device(device), bool(train)
        self.flip_ratio, self.seed, self.rank, self.world, self.size = float(flip_ratio), int(seed), int(rank), int(world), int(size)
        self.engine, self.dtype = engine, dtype
        self.area_range, self.aspect_ratio_range = tuple(area_range), tuple(aspect_ratio_range)
        if prep is None:
            from .. import ops
            prep = ops.clip_prep
        self.prep = prep
        self.epoch = 0
        n = len(dataset)
        if self.train:
            self.per_rank = n // self.world
            self.length = self.per_rank // self.batch
        else:
            self.per_rank = len(range(self.rank, n, self.world))
            self.length = -(-self.per_rank // self.batch)
        if self.length < 1:
            raise ValueError(f'{dataset.path}: {n} clips give rank {rank} of {world} no batch of {batch}')
        _, T, Hs, Ws, _ = dataset.frames.shape
        on_gpu = self.device.type == 'cuda'
        self._staging = [torch.empty(self.batch, T, Hs, Ws, 3, dtype=torch.uint8, pin_memory=on_gpu) for _ in range(2)]
        self._dev = [torch.empty(self.batch, T, Hs, Ws, 3, dtype=torch.uint8, device=self.device) for _ in range(2)] if on_gpu \
            else self._staging
        self._copied = [None, None]            # per pair: the event behind its host-to-device copy ...
        self._read = [None, None]              # ... and behind the kernel that read the device buffer
        self._copy_stream = torch.cuda.Stream(self.device) if on_gpu else None
        self._slot = 0

    def __len__(self):
        return self.length

    def indices(self, epoch):
        """This rank's sample indices of an epoch, in batch order (whole batches only with train=True)."""
        n = len(self.dataset)
        if not self.train:
            return np.arange(self.rank, n, self.world)
        perm = np.random.default_rng([self.seed, epoch]).permutation(n)
        return perm[self.rank:self.per_rank * self.world:self.world][:self.length * self.batch]

    def _static_imgs(self, shapes):
        """The static `imgs` tensor of the engine's capture of this batch geometry, or None."""
        if self.engine is None or getattr(self.engine, 'graph', None) is None:
            return None
        bufs = self.engine.input_buffers(shapes)
        return None if bufs is None else bufs['imgs']

    def _make(self, idx, boxes, flips):
        ds, B = self.dataset, len(idx)
        slot, self._slot = self._slot, self._slot ^ 1
        if self._copied[slot] is not None:
            self._copied[slot].synchronize()              # the copy that last read this staging tensor has finished
        stage = self._staging[slot][:B]
        order = np.argsort(idx, kind='stable')            # ascending reads of the memory map
        stage_np = stage.numpy()
        for j in order.tolist():
            stage_np[j] = ds.frames[int(idx[j])]
        if self.device.type == 'cuda':
            # the copy runs on a stream of its own, under the step the compute stream is still working on; it starts
            # once the kernel that last read this device buffer (two batches ago) is done, and the kernel waits for it
            src = self._dev[slot][:B]
            main = torch.cuda.current_stream(self.device)
            with torch.cuda.stream(self._copy_stream):
                if self._read[slot] is not None:
                    self._copy_stream.wait_event(self._read[slot])
                src.copy_(stage, non_blocking=True)
                self._copied[slot] = torch.cuda.Event()
                self._copied[slot].record(self._copy_stream)
            main.wait_event(self._copied[slot])
        else:
            src = stage
        keys = TEXT_KEYS + OPTIONAL_KEYS if self.train else TEXT_KEYS       # (the test pipeline emits the text keys and `index`)
        text = {k: torch.from_numpy(np.ascontiguousarray(v[idx])).to(self.device) for k, v in ds.text.items() if k in keys}
        if self.train and 'label' not in text:
            text['label'] = torch.zeros(B, dtype=torch.long, device=self.device)
        T = ds.frames.shape[1]
        shape = (B, 1, 3, T, self.size, self.size)
        shapes = {k: tuple(v.shape) for k, v in text.items()}
        shapes['imgs'] = shape
        out = self._static_imgs(shapes) if self.train else None
        imgs = self.prep(src, boxes, flips, ds.mean, ds.std, out=out, size=self.size, dtype=self.dtype)
        if self.device.type == 'cuda':
            self._read[slot] = torch.cuda.Event()
            self._read[slot].record()
        batch = dict(imgs=imgs, **text)
        if not self.train:
            batch['index'] = torch.from_numpy(np.asarray(idx, np.int64)).to(self.device)
        return batch

    def __iter__(self):
        epoch = self.epoch
        idx = self.indices(epoch)
        hw = self.dataset.frames.shape[2:4]
        rng = np.random.default_rng([self.seed, self.rank, epoch, 1])
        for s in range(0, len(idx), self.batch):
            part = idx[s:s + self.batch]
            if self.train:
                boxes = random_resized_crop_boxes(rng, len(part), hw, self.area_range, self.aspect_ratio_range)
                flips = (rng.random(len(part)) < self.flip_ratio).astype(np.uint8)
            else:
                boxes = np.tile(np.asarray(center_crop_box(hw), np.int32), (len(part), 1))
                flips = np.zeros(len(part), np.uint8)
            yield self._make(part, boxes, flips)
        if self.train:
            self.epoch = epoch + 1                         # a finished pass: the next one draws a new permutation


def packed_loaders(spec, which, batch, device, rank=0, world=1, seed=0, **common):
    """The loaders of `data.packed = dict(path=<dir>, train=dict(split='train', ...) | [dict, ...], test=dict(split='test',
    ...))` (tools/train.py, tools/test.py): one PackedClipLoader per entry of `which` ('train' | 'test') over
    <dir>/<split>; the other keys of an entry (flip_ratio, size, area_range, aspect_ratio_range, seed) go to the loader,
    and so does `common` (prep, dtype) for every entry."""
    entries = spec[which]
    entries = [entries] if isinstance(entries, dict) else list(entries)
    loaders = []
    for i, e in enumerate(entries):
        e = dict(common, **e)
        ds = PackedClipDataset(os.path.join(spec['path'], e.pop('split', which)))
        e.setdefault('seed', seed + 1000 * (i + 1))
        loaders.append(PackedClipLoader(ds, batch, device, train=which == 'train', rank=rank, world=world, **e))
    return loaders
