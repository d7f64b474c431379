"""fp64 NumPy statement of clv_clip_prep's per-pixel definition (include/clover_hip.h, "clip preparation"), written from
that definition and not from the kernel, plus the input builders and the error bound the GPU test shares with
tests/test_clip_prep_ref_cpu.py.  tests/CLIP_PREP_ERROR_BUDGET.md derives the bound."""
import numpy as np

MEAN = (123.675, 116.28, 103.53)            # the reference's img_norm_cfg (configs/exp_local/pretrain_webvid_cc3m.py)
STD = (58.395, 57.12, 57.375)


def constants(mean=MEAN, std=STD):
    """(mean, inv_std) as the fp32 numbers the kernel is handed: inv_std = fp32(1 / fp64(std)) (mmcv.imnormalize)."""
    return np.asarray(mean, np.float64).astype(np.float32), (1.0 / np.asarray(std, np.float64)).astype(np.float32)


def taps(n_out, lo, n):
    """Source indices and weight of each of n_out output positions over a crop of n pixels that starts at lo: half-pixel
    centres, the coordinate clamped to the crop's first and last pixel centre, the right neighbour clamped to the crop."""
    s = (np.arange(n_out, dtype=np.float64) + 0.5) * (float(n) / float(n_out)) - 0.5
    s = np.clip(s, 0.0, float(n - 1))
    i0 = np.floor(s).astype(np.int64)
    i1 = np.minimum(i0 + 1, n - 1)
    return lo + i0, lo + i1, s - i0


def resample(img, box, out_hw):
    """Bilinear resample (fp64) of the crop `box` = (left, top, right, bottom) of img [H, W, C] to out_hw = (h, w):
    mmcv.imresize(crop, 'bilinear') without the rounding to uint8."""
    l, t, r, b = (int(v) for v in box)
    y0, y1, fy = taps(out_hw[0], t, b - t)
    x0, x1, fx = taps(out_hw[1], l, r - l)
    im = img.astype(np.float64)
    fx, fy = fx[None, :, None], fy[:, None, None]
    top = im[y0][:, x0] * (1 - fx) + im[y0][:, x1] * fx
    bot = im[y1][:, x0] * (1 - fx) + im[y1][:, x1] * fx
    return top * (1 - fy) + bot * fy


def clip_prep_ref(src, boxes, flips, mean, inv_std, S):
    """src uint8 [B, T, Hs, Ws, 3], boxes [B, 4], flips [B], mean / inv_std [3] -> fp64 [B, 1, 3, T, S, S]."""
    B, T = src.shape[:2]
    m, s = np.asarray(mean, np.float64), np.asarray(inv_std, np.float64)
    out = np.empty((B, 1, 3, T, S, S), np.float64)
    for b in range(B):
        for t in range(T):
            v = resample(src[b, t], boxes[b], (S, S))
            if flips[b]:
                v = v[:, ::-1]
            out[b, 0, :, t] = ((v - m) * s).transpose(2, 0, 1)
    return out


def bound(ref, boxes, inv_std, unit):
    """|kernel - ref| allowed per element (tests/CLIP_PREP_ERROR_BUDGET.md): `unit` is the output type's unit roundoff
    (2^-24 fp32, 2^-11 fp16, 2^-8 bf16); boxes [B, 4]; ref [B, 1, 3, T, S, S]."""
    u = 2.0 ** -24
    ext = np.asarray([(r - l) + (b - t) for l, t, r, b in np.asarray(boxes).tolist()], np.float64)
    level = 255.0 * u * (2.0 * ext + 6.0)                                  # in uint8 levels, per sample
    return level[:, None, None, None, None, None] * float(np.max(inv_std)) + np.abs(ref) * (2.0 * u + unit)


PLANE, STRIPS = 0, 1                          # CLV_CLIP_CLASS_* of include/clover_hip.h
# output size -> (launch class, rows of the partial last strip) the GPU tests rely on; tests/test_clip_prep_ref_cpu.py
# asserts them against clv_clip_prep_plan.  8 / 16: one workgroup writes the plane (8 and 32 busy lanes of 64);
# 64: two whole passes, no partial strip; 112 (the engine test's clips) and 224: strips with a partial last one.
PLAN_CLASSES = {8: (PLANE, 0), 16: (PLANE, 0), 64: (STRIPS, 0), 112: (STRIPS, 4), 224: (STRIPS, 8)}

# The general-class cases of tests/test_clip_prep_gpu.py: (name, Hs, Ws, S, T, boxes); sample b is flipped when b is odd.
_B3753 = [(0, 0, 20, 17),       # touches the left and top frame edges
          (33, 20, 53, 37),     # touches the right and bottom edges
          (0, 0, 53, 37),       # the full frame
          (10, 5, 11, 30),      # one pixel wide: both x taps coincide
          (4, 9, 40, 10),       # one pixel high
          (7, 3, 8, 4)]         # a single pixel
_B6464 = [(0, 0, 64, 64), (0, 13, 31, 64), (17, 0, 64, 29), (5, 7, 21, 23)]
_B96128 = [(0, 0, 128, 96),     # 8 x / 6 x downscale: taps skip source pixels
           (3, 5, 99, 77)]
CASES = [('37x53-S8', 37, 53, 8, 2, _B3753), ('37x53-S16', 37, 53, 16, 2, _B3753),
         ('64x64-S16', 64, 64, 16, 1, _B6464), ('64x64-S64', 64, 64, 64, 1, _B6464),
         ('96x128-S16', 96, 128, 16, 2, _B96128), ('96x128-S8', 96, 128, 8, 1, _B96128),
         ('96x128-S224', 96, 128, 224, 1, [(7, 3, 120, 96)])]          # S = 224: one frame only


def case_inputs(case, seed=0):
    """(src uint8 [B, T, Hs, Ws, 3], boxes int32 [B, 4], flips uint8 [B]) of a CASES entry."""
    name, Hs, Ws, S, T, boxes = case
    rng = np.random.default_rng([seed, Hs, Ws, S])
    B = len(boxes)
    return random_frames(rng, B, T, Hs, Ws), np.asarray(boxes, np.int32), (np.arange(B) % 2).astype(np.uint8)


def ramp_frame(Hs, Ws, ax=2, ay=3, c0=5):
    """uint8 [Hs, Ws, 3]: value = c0 + ax * x + ay * y + channel (an affine image; must stay <= 255)."""
    y, x = np.mgrid[0:Hs, 0:Ws]
    v = c0 + ax * x + ay * y
    f = np.stack([v, v + 1, v + 2], -1)
    assert f.max() <= 255
    return f.astype(np.uint8)


def random_frames(rng, B, T, Hs, Ws):
    return rng.integers(0, 256, size=(B, T, Hs, Ws, 3), dtype=np.uint8)
