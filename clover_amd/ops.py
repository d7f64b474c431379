"""torch.autograd.Function wrappers over the C ABI (include/clover_hip.h).

These own every tensor, pass ``data_ptr()`` + the current HIP stream through ctypes, and
are what the registered nn.Modules call.  No CPU path exists: a non-HIP tensor raises.
"""
import ctypes as C
import functools
import os
from typing import Any, NamedTuple, Optional

import torch

from . import _lib, parity
from ._lib import ClvAttnGeom, check

BF16 = _lib.half_dtype()          # the 16-bit storage type: bf16, or fp16 with CLOVER_HALF=f16 (the name is historical)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError('clover_amd ops run only on a HIP device (MI355X); there is no CPU fallback — '
                               'got a tensor on %s' % t.device)


LIBRARY_GEMM_CALLS = {}     # {(site, shape): calls} of every GEMM that left the own kernels for the ROCm library (below)


def _library_gemm(site, shape):
    """Every GEMM of the Clover configs runs on the own kernels, and no switch routes one elsewhere; only a shape they do
    not take (a contraction that is not a multiple of 64 such as the 48-wide tiny model, a sequence beyond
    clv_attn_seq_max_keys() = 4096 keys, ...) goes to the ROCm library, and only THROUGH HERE: counted in
    LIBRARY_GEMM_CALLS (bench.py prints the table, the step tests assert it stays empty), announced once per shape, and
    refused with CLOVER_STRICT_OWN_GEMM=1 — never silent."""
    key = (site, tuple(int(v) for v in shape))
    n = LIBRARY_GEMM_CALLS.get(key, 0)
    LIBRARY_GEMM_CALLS[key] = n + 1
    if os.environ.get('CLOVER_STRICT_OWN_GEMM') == '1':
        raise RuntimeError(f'CLV_ERR_UNSUPPORTED: {site} {key[1]} is not covered by the HIP GEMM kernels '
                           f'(CLOVER_STRICT_OWN_GEMM=1 refuses the library fallback)')
    if n == 0:
        import warnings
        warnings.warn(f'clover_amd: {site} with shape {key[1]} runs on the ROCm library GEMM, not on the HIP kernels '
                      f'(shape outside their coverage)', RuntimeWarning, stacklevel=3)


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


def _half_rows(t, cols):
    """t as contiguous rows [-1, cols] of the 16-bit storage type (an upstream gradient on its way into a kernel)."""
    t = t.reshape(-1, cols)
    return _c(t if t.dtype == BF16 else t.to(BF16))


ACTIVE_LOSS_SCALE = [1.0]    # the loss scale of the backward pass that is RUNNING (set by _ScaleGrad at its root, reset at its end)


class _ScaleGrad(torch.autograd.Function):
    """Identity whose backward multiplies the gradient by a constant: the loss scale at the root of a 16-bit backward
    (_lib.LOSS_SCALE).  It also publishes the scale for the duration of that backward pass (ACTIVE_LOSS_SCALE), so that the
    recognizer's per-parameter hooks divide it out of exactly the gradients that carry it — a backward that does not start
    from the recognizer's loss (a test differentiating a feature map) is left alone."""

    @staticmethod
    def forward(ctx, x, s):
        ctx.s = float(s)
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        ACTIVE_LOSS_SCALE[0] = ctx.s
        torch.autograd.Variable._execution_engine.queue_callback(_reset_active_scale)
        return g * ctx.s, None


def _reset_active_scale():
    ACTIVE_LOSS_SCALE[0] = 1.0


def unscale_hook(g):
    """Gradient hook of a plain-autograd parameter: divide the running backward's loss scale out (a power of two: exact)."""
    s = ACTIVE_LOSS_SCALE[0]
    return g if s == 1.0 else g * (1.0 / s)


def scale_grad(x, s):
    return _ScaleGrad.apply(x, s) if (s != 1.0 and x.requires_grad) else x


class _ScaleGradDev(torch.autograd.Function):
    """_ScaleGrad with the scale held in DEVICE memory (the engine's loss scaler, clv_optim_prep moves it): the multiply
    reads it when the kernel runs, so a captured backward follows a dynamic scale without re-capture.  The engine's
    optimizer kernels divide the same device value out again."""

    @staticmethod
    def forward(ctx, x, s):
        ctx.s = s
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.s, None


def scale_grad_dev(x, s):
    return _ScaleGradDev.apply(x, s) if x.requires_grad else x


# --------------------------------------------------------------------------- in-process kernel timing
# bench.py sets PROF = {} for the timed region: every attention launch is then bracketed by HIP
# events recorded on the launch stream (no synchronisation), and the elapsed times are read after
# the final sync.  key -> dict(events=[(start, end)], flops=.., bytes=..) per launch.
PROF = None


class _Timed:
    def __init__(self, key, flops, nbytes):
        self.key, self.flops, self.nbytes = key, flops, nbytes

    def __enter__(self):
        if PROF is not None:
            self.s = torch.cuda.Event(enable_timing=True)
            self.e = torch.cuda.Event(enable_timing=True)
            self.s.record()
        return self

    def __exit__(self, *a):
        if PROF is not None:
            self.e.record()
            PROF.setdefault(self.key, []).append((self.s, self.e, self.flops, self.nbytes))


_DBIAS_INDEX = {}


def _dbias_index(g, device):
    """Device pointer of the (bias-table row, key) -> dS-fragment offset table of this window geometry, built on first
    use (outside hipGraph captures) and kept for the life of the process; None = the kernel does the index arithmetic."""
    if os.environ.get('CLOVER_DBIAS_INDEX', '1') != '1':
        return None
    key = (str(device), g.N, g.bwd, g.bwh, g.bww)
    t = _DBIAS_INDEX.get(key)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            return None
        L = _lib.lib()
        n = L.clv_attn_dbias_index_count(C.byref(g))
        if n <= 0:
            return None
        t = torch.empty(n, device=device, dtype=torch.int32)
        check(L.clv_attn_dbias_index(C.byref(g), _ptr(t), _stream()), 'clv_attn_dbias_index')
        _DBIAS_INDEX[key] = t
    return t.data_ptr()


def _kname(kernel, g):
    """Device-kernel name as rocprofv3 prints it: template <HD, NKT, DROP, MODE> (attention.hip CLV_PICK)."""
    need = (g.N + 15) // 16
    mode = g.mode
    if need > 28 and (g.mode == 0 or g.N <= WINDOW_MAX_TOKENS):
        # a long sequence, or a window beyond 448 tokens, runs as P parts of staged tokens (attention.hip make_geom): the
        # instantiation is chosen from the PART's tiles, not from N; a window's parts hold at most 25 tiles (the table band
        # shares the LDS) and run the instantiations of template MODE 2
        per = 28 if g.mode == 0 else 25
        parts = (need + per - 1) // per
        need = (need + parts - 1) // parts
        mode = 0 if g.mode == 0 else 2
    nkt = next((o for o in ((16, 25) if mode == 2 else (2, 8, 13, 14, 15, 16, 25, 28)) if o >= need), need)   # > 28: UNSUPPORTED
    drop = 'true' if (g.dropout_p > 0 and g.mode == 0) else 'false'
    if kernel == 'attn_bwd_dkv_kernel':
        nkt = (nkt + 1) & ~1                  # the dK / dV kernel runs the next even tile count (attention.hip launch_bwd)
    return f'{kernel}<{g.hd}, {nkt}, {drop}, {mode}>'


def _attn_work(g, backward):
    """Algorithmic work of one attention call: 2 flops/MAC over the
    N x N x hd products (2 matmuls forward, 5 backward); bytes = q,k,v read + o written
    (forward) or q,k,v,o,do read + dq,dk,dv written (backward), bf16.  A sequence or a window run as P parts does the same N x N
    products (every part set walks all looped tiles against its own part of the staged ones); the P-fold re-staging and
    the partial results in the scratch are the implementation's traffic, not counted here."""
    per = g.groups * g.nH * g.N * g.N * g.hd
    flops = (10 if backward else 4) * per
    tok = g.groups * g.N * g.nH * g.hd * 2
    nbytes = (8 if backward else 4) * tok
    return flops, nbytes


def roofline_from_prof(prof, steps):
    """-> (roofline dict of the dominant instrumented KERNEL, per-kernel table, roofline dict of the runner-up).  Keys are device
    kernel names (as rocprofv3 --stats prints them); a kernel launched with many shapes is aggregated:
    achieved = sum(algorithmic work) / sum(duration), avg_us = mean launch duration."""
    rows = []
    for key, evs in prof.items():
        ms = [s.elapsed_time(e) for s, e, _, _ in evs]
        rows.append(dict(kernel=key, launches_per_step=len(ms) / steps, avg_us=1e3 * sum(ms) / len(ms),
                         total_ms_per_step=sum(ms) / steps, secs=sum(ms) * 1e-3,
                         flops=sum(f for _, _, f, _ in evs), bytes=sum(b for _, _, _, b in evs)))
    rows.sort(key=lambda r: -r['total_ms_per_step'])

    def roof_of(top):
        n = len(prof[top['kernel']])
        t_hbm, t_mfma = top['bytes'] / 8.0e12, top['flops'] / 2.5e15
        if t_hbm >= t_mfma:
            roof = dict(bound='hbm', achieved=round(top['bytes'] / top['secs'] / 1e9, 1), peak=8000.0, unit='GB/s',
                        frac=round(top['bytes'] / top['secs'] / 8.0e12, 4), traffic=None)
        else:
            roof = dict(bound='mfma', achieved=round(top['flops'] / top['secs'] / 1e12, 2), peak=2500.0, unit='TFLOP/s',
                        frac=round(top['flops'] / top['secs'] / 2.5e15, 4), traffic=None)
        roof['kernel'] = top['kernel']
        roof['avg_us'] = round(top['avg_us'], 2)
        roof['launches_per_step'] = round(top['launches_per_step'], 2)
        roof['ms_per_step'] = round(top['total_ms_per_step'], 3)
        roof['algorithmic_bytes_per_launch'] = int(top['bytes'] / n)
        roof['algorithmic_flops_per_launch'] = int(top['flops'] / n)
        return roof
    roof = roof_of(rows[0])
    # the runner-up too (bench.py prints it as `roofline_2`): the two largest kernels of the step are 2 % apart (the grouped
    # weight-gradient launch and AdamW), so which one leads flips from box to box — a reader comparing rounds sees both
    roof2 = roof_of(rows[1]) if len(rows) > 1 else None
    def frac_of(r):       # the same roofline arithmetic for every instrumented kernel: which roof bounds it, what fraction it reaches
        hb, mf = r['bytes'] / 8.0e12, r['flops'] / 2.5e15
        return ('hbm', round(r['bytes'] / r['secs'] / 8.0e12, 4)) if hb >= mf else ('mfma', round(r['flops'] / r['secs'] / 2.5e15, 4))
    table = [dict(kernel=r['kernel'], launches_per_step=round(r['launches_per_step'], 2),
                  avg_us=round(r['avg_us'], 2), ms_per_step=round(r['total_ms_per_step'], 3),
                  bound=frac_of(r)[0], frac=frac_of(r)[1]) for r in rows[:14]]
    return roof, table, roof2


# --------------------------------------------------------------------------- Linear
def _wgrad_custom(M, N, K):
    """Shapes the split-M weight-gradient kernels take: every Linear whose widths are multiples of 8 (16-byte row groups)
    — token-parallel ones (huge M, small N x K), few-row ones (M <= 1024: one M-slice accumulated straight into the fp32
    gradient), the 256 x 256-tile class for the large stage-3 / fusion outputs, and everything between them on M-slices
    of >= 256 rows of the 128 x 128 tiles."""
    return N % 8 == 0 and K % 8 == 0


FRESH_LOG = None            # census (engine set-up): {data_ptr: [calls, numel]} of every sink linear_wgrad writes


class FusedNormState:
    """Shared by the sinks of one engine's fused gradient norm: dirty = the norm slots do not describe the slabs this step."""

    def __init__(self):
        self.dirty = False


class NormSlots(NamedTuple):
    """``_clv_ssq`` of a sink in fused-norm mode (engine._setup_fused_norm)."""
    acc: Any                # the engine's sum-of-squares accumulator (an explicit pass over the sink adds to it)
    slots: Any              # the CLV_SUMSQ_SLOTS partial sums the grouped / fold kernels add to
    state: FusedNormState


class FirstTouch:
    """State of an engine's first-touch gradient sinks (engine._setup_first_touch): ``on`` and the set of sinks already
    written since the engine last "cleared" the gradients.  The sink tensors (``param._clv_grad``) carry it as
    ``_clv_ft``, so whoever runs a backward over these parameters — the engine or plain ``loss.backward()`` — sees the
    same state."""

    def __init__(self):
        self.on = False
        self.done = set()


def first_touch(dw_out):
    """True when dw_out is a sink whose previous content is STALE (a weight the engine does not zero: its first weight
    gradient of a step overwrites instead of accumulating — 8 bytes of HBM traffic per parameter and step less: no
    zero-fill, no read-modify-write).  Every later gradient of the same step accumulates as usual."""
    if dw_out is None:
        return False
    if FRESH_LOG is not None:
        ent = FRESH_LOG.setdefault(dw_out.data_ptr(), [0, dw_out.numel()])
        ent[0] += 1
        if ent[1] != dw_out.numel():
            ent[0] += 1 << 20                              # two sinks of different extent at one address: never first-touch
    st = getattr(dw_out, '_clv_ft', None)
    if st is None or not st.on or id(dw_out) in st.done:
        return False
    st.done.add(id(dw_out))
    return True


def _sinks(*params, pad=False):
    """The gradient sinks of a GROUP of parameters whose gradients one backward produces together: a tuple aligned with
    `params` (None where the parameter is None: an absent bias) when EVERY present one has a usable sink — the backward
    then writes straight into them, calls _delivered() and returns None to autograd — else None: it allocates
    temporaries and returns them.  All or nothing, so a group never splits between the two routes.

    A sink is the engine's fp32 slab view ``param._clv_grad`` (pad=True: ``_clv_pad_grad``, the phantom-padded view the
    MLM decoder's kernels write).  It is usable when it is fp32 and contiguous: the kernels write fp32 through the raw
    pointer, so any other tensor was never a correct target, and the engine never produces one (engine._Segment).
    What comes back is the ATTRIBUTE OBJECT, never a view of it: the first-touch state (``_clv_ft``, keyed on id() in
    first_touch()) and the fused-norm slots (``_clv_ssq``) hang on that object, and a view carries neither.

    Groups: (weight, bias) of a Linear — _LinearF32, _param_grads (_Linear, _MlpGelu, both _FusedMLP bodies), _MLMDecoder
    (pad); (weight, bias, gamma, beta) of a LayerNorm-folded projection — _unfold_grads, _wgrad_folded; (gamma, beta) —
    _LayerNorm, _MergeLayerNorm; (weight, bias, gamma, beta, mask_token) — _PatchEmbed.  One parameter at a time
    (_sink): _Embedding, the table of _Attention, each of the six parameters of _QAHead."""
    attr = '_clv_pad_grad' if pad else '_clv_grad'
    out = []
    for p in params:
        sk = getattr(p, attr, None)
        if p is not None and (sk is None or sk.dtype != torch.float32 or not sk.is_contiguous()):
            return None
        out.append(sk)
    return tuple(out)


def _sink(param):
    """The usable sink of ONE parameter (see _sinks), or None."""
    sks = _sinks(param)
    return sks[0] if sks is not None else None


def _delivered(*params):
    """The gradients of `params` (None entries skipped) are complete in their sinks: the bucket countdown of the gradient
    all-reduce (``_clv_ready``; a fused view's fans out to its members), once per parameter."""
    for p in params:
        if p is not None:
            p._clv_ready()


def linear_wgrad(dy2, x2, want_bias, dw_out=None, db_out=None, xstats=None):
    """dW fp32 [N,K] and db fp32 [N] of y = x W^T + b for bf16 dy2 [M,N], x2 [M,K].
    With dw_out / db_out (fp32, e.g. views of the engine's flat gradient slab) the result is
    ACCUMULATED into them in place and (None, None) is returned — dW is STORED instead when the sink is a first-touch
    one (first_touch()).  xstats = (mean, rstd): the GEMM
    operand is the row-standardised x (the LayerNorm output a fused forward never stored)."""
    M, N = dy2.shape
    K = x2.shape[1]
    sink = dw_out is not None
    first = first_touch(dw_out)
    # fused gradient norm (engine, one rank): this sink's sum of squares is delivered by whoever WRITES it — the grouped /
    # fold kernels through their norm slots (DELIVER_SUMSQ), every other path by an explicit pass over the sink right here
    ssq = getattr(dw_out, '_clv_ssq', None) if sink else None
    if ssq is not None and not first:
        # a SECOND gradient for a sink whose sum of squares rode on its first one (a caller running two backward passes
        # between optimizer steps): the fused sums no longer describe the slab — the engine recomputes the whole norm
        ssq.state.dirty = True
        ssq = None
    if xstats is not None and not _wgrad_custom(M, N, K):
        x2 = ((x2.float() - xstats[0][:, None]) * xstats[1][:, None]).to(BF16)
        xstats = None
    if _wgrad_custom(M, N, K):
        L = _lib.lib()
        if SEGMENT is not None and SEGMENT.wgrads is not None and sink and xstats is None:
            # nothing reads a weight gradient before the optimizer: this launch joins the grouped one that closes the
            # backward segment (dy2 / x2 stay alive in the list until then)
            SEGMENT.wgrads.append(WgradItem(dy2, x2, dw_out, db_out if want_bias else None, M, N, K,
                                            (STORE_DW if first else 0) | (DELIVER_SUMSQ if ssq is not None else 0),
                                            torch.cuda.current_stream().cuda_stream))
            return None, None
        if first:
            dw_out.zero_()                     # the stand-alone launches only accumulate
        dw = dw_out if sink else torch.zeros(N, K, device=dy2.device, dtype=torch.float32)
        db = (db_out if sink else torch.zeros(N, device=dy2.device, dtype=torch.float32)) if want_bias else None
        work = torch.empty(L.clv_linear_wgrad_work_floats(M, N, K), device=dy2.device, dtype=torch.float32)
        args = (_ptr(dy2), _ptr(x2), _ptr(dw), _ptr(db), _ptr(work), M, N, K, dy2.stride(0), x2.stride(0),
                _ptr(xstats[0] if xstats else None), _ptr(xstats[1] if xstats else None))
        slices = L.clv_linear_wgrad_splits(M, N, K)
        needs_fold = slices > 1 or xstats is not None       # one slice without standardisation: atomics straight into dW
        if PROF is None:
            if SEGMENT is not None and sink and needs_fold:
                # partial kernel now, its fold in the segment's ONE batched launch (a stale dw was zeroed above: += is =)
                check(L.clv_linear_wgrad(*args, 1, _stream()), 'clv_linear_wgrad')
                SEGMENT.folds.append(FoldItem(work, dw, db, N, K, slices, DELIVER_SUMSQ if ssq is not None else 0))
            else:
                check(L.clv_linear_wgrad(*args, 0, _stream()), 'clv_linear_wgrad')
                if ssq is not None:
                    sumsq_accumulate(dw, ssq.acc)
        else:                                  # one event pair per device kernel
            kname = 'wgrad_kernel' if xstats else f"wgrad_dma2_kernel<{'true' if slices == 1 else 'false'}>"
            with _Timed(kname, 2 * M * N * K, M * (N + K) * 2):
                check(L.clv_linear_wgrad(*args, 1, _stream()), 'clv_linear_wgrad')
            check(L.clv_linear_wgrad(*args, 2, _stream()), 'clv_linear_wgrad')
            if ssq is not None:
                sumsq_accumulate(dw, ssq.acc)
        return (None, None) if sink else (dw, db)
    # library GEMM with fp32 output: accumulated in place into the gradient slab view (beta = 1) — no bf16 rounding
    # of dW and no separate fp32 add
    db = None
    if want_bias:
        db = db_out if sink else torch.zeros(N, device=dy2.device, dtype=torch.float32)
        if N % 8 == 0 and dy2.stride(0) % 8 == 0:
            check(_lib.lib().clv_colsum(_ptr(dy2), _ptr(db), M, N, dy2.stride(0), _stream()), 'clv_colsum')
        else:
            db.add_(dy2.sum(0, dtype=torch.float32))
    _library_gemm('linear_wgrad', (M, N, K))
    if sink:
        if first:
            torch.mm(dy2.t(), x2, out_dtype=torch.float32, out=dw_out)
        else:
            torch.addmm(dw_out, dy2.t(), x2, out_dtype=torch.float32, out=dw_out)
        if ssq is not None:
            sumsq_accumulate(dw_out.reshape(-1), ssq.acc)
        return None, None
    return torch.mm(dy2.t(), x2, out_dtype=torch.float32), db


# Flag bits of a deferred item: the `overwrite` fields of ClvWgradEntry / ClvFoldEntry (include/clover_hip.h)
STORE_DW = 1                # dW is stored, not added: a first-touch sink, or an uninitialised temporary
STORE_DB = 2                # ... and db too (folds only)
DELIVER_SUMSQ = 4           # whoever writes dW adds its sum of squares to the sink's norm slots (fused gradient norm)


class WgradItem(NamedTuple):        # a deferred dw += dy^T x, db += colsum(dy); dy and x stay alive in it until the launch
    dy: Any
    x: Any
    dw: Any
    db: Any
    M: int
    N: int
    K: int
    flags: int = 0
    stream: Optional[int] = None    # raw handle of the stream it was queued from; None: waits for the segment's end


class FoldItem(NamedTuple):         # a deferred fold of `splits` fp32 partial slabs [N*K dW | N db] into dw / db
    partial: Any
    dw: Any
    db: Any
    N: int
    K: int
    splits: int
    flags: int = 0


# a deferred reduction of a LayerNorm backward's per-block partials [2][nblk][C] into dgamma / dbeta, and a deferred
# relative-position-table gather: the planned ClvDbiasGather and the tensors it points into
LnReduceItem = NamedTuple('LnReduceItem', [('partial', Any), ('dgamma', Any), ('dbeta', Any), ('nblk', int), ('C', int)])
DbiasItem = NamedTuple('DbiasItem', [('entry', Any), ('partial', Any), ('dtable', Any), ('index', Any)])


class Segment:
    """Context (ops.defer_folds()): what a backward segment postpones to its end — the engine wraps whole backward segments,
    nobody reads these gradients before the optimizer.  Weight-gradient launches (`wgrads`; None with CLOVER_GROUP_WGRAD=0:
    they go out at once), the `folds` of their partials (ONE launch instead of ~44 launch-bound 5-7 us fold kernels per pass),
    the LayerNorm un-folds that consume them (`post`, callables), LayerNorm reductions (`ln_reduces`), table gathers (`dbias`)."""

    def __init__(self):
        self.wgrads = [] if os.environ.get('CLOVER_GROUP_WGRAD', '1') == '1' else None
        self.folds, self.post, self.ln_reduces, self.dbias = [], [], [], []

    def __enter__(self):
        global SEGMENT
        self.prev, SEGMENT = SEGMENT, self
        return self

    def __exit__(self, *exc):
        global SEGMENT
        SEGMENT = self.prev
        if exc[0] is None:                 # (a backward segment that raised launches nothing that it deferred)
            flush_folds(self.folds + flush_wgrads(self.wgrads or []))    # (the folds those produced included)
            for fn in self.post:
                fn()
            flush_ln_reduces(self.ln_reduces)
            flush_dbias_gathers(self.dbias)

    def take_stream_wgrads(self, stream):
        """Remove and return the weight gradients queued from `stream` (a raw handle); the others keep their order."""
        mine = [it for it in self.wgrads if it.stream == stream]
        self.wgrads[:] = [it for it in self.wgrads if it.stream != stream]
        return mine


defer_folds = Segment       # the name its users know: `with ops.defer_folds(): <backward segment>`
SEGMENT = None              # the open Segment; one plain global: autograd runs one device's backward on one thread


def flush_stream_wgrads():
    """Launch NOW, on the current stream, the deferred weight gradients that were queued from it (and the folds of their
    partials), leaving the others pending.  The text tower's backward runs on a side stream beside the video tower's: at
    its end (`flush_point` on the embedding output) its 48 few-row weight gradients go out there, under the rest of the
    video backward, instead of as the last grouped launch of the step on the main stream.
    (The same for the heads' / fusion encoder's gradients on an auxiliary stream was measured and dropped: same-box
    11.09 / 11.16 -> 11.28 / 11.33 ms — MFMA-heavy grouped launches beside the video chain take the CUs and the HBM that
    chain is bound by, as the early video launches of round 4 did.)"""
    if SEGMENT is not None and SEGMENT.wgrads:
        flush_folds(flush_wgrads(SEGMENT.take_stream_wgrads(torch.cuda.current_stream().cuda_stream)))


class _FlushPoint(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        flush_stream_wgrads()
        return g


def flush_point(x):
    """Identity whose backward flushes the deferred weight gradients of the stream it runs on (see flush_stream_wgrads)."""
    if x.requires_grad and x.is_cuda:
        return _FlushPoint.apply(x)
    return x


def _chunks(items, cap, keys):
    """Split `items`, in order, into launches of <= cap of them in which no conflict key appears twice (keys(item): the
    addresses its launch adds into WITHOUT atomics, possibly none).  Greedy: a launch closes when it is full or the next
    item's keys meet it; successive launches on a stream are ordered, which keeps those kernels race-free."""
    chunks, seen = [], set()
    for item in items:
        k = keys(item)
        if not chunks or len(chunks[-1]) == cap or not seen.isdisjoint(k):
            chunks.append([])
            seen = set()
        chunks[-1].append(item)
        seen.update(k)
    return chunks


def wgrad_chunks(pending):
    """The deferred weight gradients in launches of <= WGRAD_GROUP_MAX problems.  In-place problems (few rows / very large
    outputs: clv_linear_wgrad_in_place) add into dW without atomics: two with the SAME dW never share a launch."""
    in_place = _lib.lib().clv_linear_wgrad_in_place
    return _chunks(pending, _lib.WGRAD_GROUP_MAX, lambda it: (it.dw.data_ptr(),) if in_place(it.M, it.N, it.K) else ())


def flush_wgrads(pending):
    """The deferred weight gradients as grouped launches (clv_linear_wgrad_batch); returns the FoldItems of their partials."""
    folds = []
    L = _lib.lib()
    for chunk in wgrad_chunks(pending):
        arr = (_lib.ClvWgradEntry * len(chunk))()
        for e, it in zip(arr, chunk):
            e.dy, e.x, e.M, e.N, e.K = it.dy.data_ptr(), it.x.data_ptr(), it.M, it.N, it.K
            e.ldy, e.ldx, e.want_bias = it.dy.stride(0), it.x.stride(0), int(it.db is not None)
        check(L.clv_linear_wgrad_batch_plan(arr, len(chunk)), 'clv_linear_wgrad_batch_plan')
        work = torch.empty(max(1, sum(e.work_floats for e in arr)), device=chunk[0].dy.device, dtype=torch.float32)
        off = 0
        slots = None                                 # norm slots of the sinks whose sum of squares the kernels deliver
        for e, it in zip(arr, chunk):
            if it.flags & DELIVER_SUMSQ:
                slots = it.dw._clv_ssq.slots
            if e.work_floats == 0:                   # few-row problem: accumulated in place, nothing to fold
                e.dw, e.db = it.dw.data_ptr(), (it.db.data_ptr() if it.db is not None else None)
                e.overwrite = it.flags & (STORE_DW | DELIVER_SUMSQ)
                continue
            w = work[off:off + e.work_floats]
            e.work = w.data_ptr()
            folds.append(FoldItem(w, it.dw, it.db, it.N, it.K, e.splits, it.flags))
            off += e.work_floats
        if PROF is None:
            check(L.clv_linear_wgrad_batch_ss(arr, len(chunk), _ptr(slots), _stream()), 'clv_linear_wgrad_batch')
        else:                                        # one event pair per device kernel: the tile classes one by one
            for cls, kname in ((0, 'wgrad_dma2_group_kernel'), (1, 'wgrad_big_group_kernel<2, 2>')):
                sub = [e for e in arr if L.clv_linear_wgrad_class(e.M, e.N, e.K) == cls]
                if not sub:
                    continue
                sarr = (_lib.ClvWgradEntry * len(sub))(*sub)
                with _Timed(kname, sum(2 * e.M * e.N * e.K for e in sub), sum(e.M * (e.N + e.K) * 2 for e in sub)):
                    check(L.clv_linear_wgrad_batch_ss(sarr, len(sub), _ptr(slots), _stream()), 'clv_linear_wgrad_batch')
    return folds


def fold_chunks(pending):
    """The deferred folds in launches of <= FOLD_MAX entries in which no dW (and no db) appears twice: fold_batch_kernel
    adds with a plain load / add / store, every entry from its own blocks, so two entries with one target in ONE launch
    would race (a Linear applied twice inside a backward segment on the partial path — ADVICE r2)."""
    return _chunks(pending, _lib.FOLD_MAX,
                   lambda it: (it.dw.data_ptr(),) if it.db is None else (it.dw.data_ptr(), it.db.data_ptr()))


def flush_folds(pending):
    for chunk in fold_chunks(pending):
        arr = (_lib.ClvFoldEntry * len(chunk))()
        slots = None
        for e, it in zip(arr, chunk):
            e.partial, e.dw, e.db = it.partial.data_ptr(), it.dw.data_ptr(), (it.db.data_ptr() if it.db is not None else None)
            e.nk, e.e2, e.splits, e.overwrite = it.N * it.K, it.N * it.K + it.N, it.splits, it.flags
            if it.flags & DELIVER_SUMSQ:             # the fold delivers this sink's sum of squares (fused gradient norm)
                slots = it.dw._clv_ssq.slots
        check(_lib.lib().clv_wgrad_fold_batch_ss(arr, len(chunk), _ptr(slots), _stream()), 'clv_wgrad_fold_batch')


def flush_dbias_gathers(pending):
    """The deferred table-gradient gathers (DbiasItem) as launches of <= DBIAS_GATHER_MAX blocks; two gathers into the
    SAME table (a module applied twice in the segment) never share a launch — each adds without atomics."""
    for chunk in _chunks(pending, _lib.DBIAS_GATHER_MAX, lambda it: (it.dtable.data_ptr(),)):
        arr = (_lib.ClvDbiasGather * len(chunk))(*[it.entry for it in chunk])
        check(_lib.lib().clv_attn_dbias_gather_batch(arr, len(chunk), _stream()), 'clv_attn_dbias_gather_batch')


def flush_ln_reduces(pending):
    for chunk in _chunks(pending, _lib.LN_REDUCE_MAX, lambda it: ()):      # (the kernel adds with atomics: no key)
        arr = (_lib.ClvLnReduceEntry * len(chunk))()
        for e, it in zip(arr, chunk):
            e.partial, e.dgamma, e.dbeta = it.partial.data_ptr(), it.dgamma.data_ptr(), it.dbeta.data_ptr()
            e.nblk, e.C = it.nblk, it.C
        check(_lib.lib().clv_ln_reduce_batch(arr, len(chunk), _stream()), 'clv_ln_reduce_batch')


def _rowgemm_fwd_ok(x, N, K):
    """Forward y = x W^T: the row-streaming kernel wins for K <= 128 (stage-0 Swin widths)."""
    return x.is_cuda and K <= 128 and x.stride(-1) == 1 and rowgemm_supported(N, K)


# Widest output clv_gemm_nt is handed by the Linear wrappers.  Up to 3072 columns the bias row sits in LDS; wider outputs
# (VideoSwin-B's stage-3 MLP: 4096; round 6 — they used to fall to the library) read it from global memory in the epilogue,
# as the MLM decoder's 30 528 columns always did.
OWN_GEMM_MAX_N = 65536


def own_gemm_ok(a, N, K):
    """Shapes that run on clv_gemm_nt (forward: a = x [M, K], N outputs; input gradient: a = dy, contraction = the layer's
    output width): every forward / input-gradient GEMM of a Linear whose shape the kernel takes — Swin stages 1-3,
    PatchMerging, the text tower, the fusion encoder, fc_in, the MLM transform — from one row up (a 3-caption
    text batch has 48).  Device-side durations against the tuned library GEMM: tools/probes/gemm_bench.py and
    tools/probes/gemm_tiles.py."""
    return (a.is_cuda and a.dtype == BF16 and a.shape[0] >= 1 and K % 64 == 0 and K >= 64
            and 64 <= N <= OWN_GEMM_MAX_N and N % 8 == 0 and a.stride(1) == 1 and a.stride(0) % 8 == 0
            and a.data_ptr() % 16 == 0)


def wants_transposed(out_features, in_features):
    """Does the input gradient of a Linear(in, out) run on a kernel that takes W^T as a K-contiguous operand
    (linear_dgrad: the row-streaming GEMM of the stage-0 widths, clv_gemm_nt otherwise)?  Modules flag such weights
    (``_clv_want_t``) and the engine keeps their bf16 transposes fresh."""
    return (out_features % 64 == 0 and 64 <= in_features <= OWN_GEMM_MAX_N and in_features % 8 == 0) or \
           (in_features <= 128 and out_features <= 384)


# --------------------------------------------------------------------------- fp8 forward GEMMs (BASELINE config 5)
FP8 = os.environ.get('CLOVER_FP8', '0') == '1'


def fp8_ok(a, N, K):
    """CLOVER_FP8=1: forward GEMMs whose contraction is a multiple of 128 run on e4m3 operands (clv_gemm_nt_fp8) — QKV,
    attention-output / FFN / PatchMerging projections of Swin stages 1-3 (stage 0 and the patch projection contract over
    96-128 inputs: their row-streaming / fused kernels are bound by the activation traffic, not the matrix pipe), the text
    tower and the fusion encoder.  Gradients stay bf16."""
    # wide outputs only (CLOVER_FP8_MIN_N, default 1024): the row-wise quantisation of the activation is an extra pass
    # over [M, K]; it pays where the GEMM does >= ~1000 MACs per activation element (measured)
    return (FP8 and a.is_cuda and a.dtype == BF16 and a.shape[0] >= 64 and K % 128 == 0 and 256 <= K <= 4096
            and int(os.environ.get('CLOVER_FP8_MIN_N', '1024')) <= N <= 3072 and N >= 64 and N % 8 == 0 and a.stride(1) == 1 and a.stride(0) % 8 == 0 and a.data_ptr() % 16 == 0)


def quant_fp8_rows(x2):
    """(q uint8 [M,K] e4m3 bytes, scale fp32 [M]) with q = x / scale, scale = rowmax|x| / 448."""
    _need_gpu(x2)
    assert x2.dtype == BF16 and x2.dim() == 2 and x2.stride(1) == 1
    M, K = x2.shape
    q = torch.empty(M, K, device=x2.device, dtype=torch.uint8)
    sc = torch.empty(M, device=x2.device, dtype=torch.float32)
    check(_lib.lib().clv_quant_fp8_rows(_ptr(x2), _ptr(q), _ptr(sc), M, K, x2.stride(0), K, _stream()), 'clv_quant_fp8_rows')
    return q, sc


def gemm_nt_fp8(a, b, bias=None, epilogue=None, aq8=None):
    """c bf16 [M,N] = a [M,K] . b [N,K]^T (+ bias, GELU) with both bf16 operands quantised row-wise to e4m3 on the way
    (raw launcher, no autograd).  aq8 = (q uint8 [M,K], scale fp32 [M]): a's quantised form when its producer already
    wrote it (the LayerNorm kernel).  Returns c, or (c, GELU'(pre)) for GEMM_EPI_BIAS_GELU_D."""
    if epilogue is None:
        epilogue = GEMM_EPI_BIAS if bias is not None else GEMM_EPI_NONE
    if aq8 is not None and tuple(aq8[0].shape) == tuple(a.shape):
        aq, asc = aq8
    else:
        aq, asc = quant_fp8_rows(a)
    bq, bsc = quant_fp8_rows(b)
    M, K = a.shape
    N = b.shape[0]
    c = torch.empty(M, N, device=a.device, dtype=BF16)
    c2 = torch.empty_like(c) if epilogue == GEMM_EPI_BIAS_GELU_D else None
    if bias is not None and bias.dtype != torch.float32:
        bias = bias.float()
    args = (_ptr(aq), _ptr(bq), _ptr(asc), _ptr(bsc), _ptr(bias), _ptr(c), _ptr(c2), M, N, K, K, K, N, int(epilogue), _stream())
    if PROF is None:
        check(_lib.lib().clv_gemm_nt_fp8(*args), 'clv_gemm_nt_fp8')
    else:
        nout = 2 if c2 is not None else 1
        with _Timed(_gemm_kname(M, N, K // 2, int(epilogue), True), 2 * M * N * K, M * K + N * K + nout * M * N * 2):
            check(_lib.lib().clv_gemm_nt_fp8(*args), 'clv_gemm_nt_fp8')
    return (c, c2) if c2 is not None else c


def _raw_bf16(p):
    """The 16-bit copy of a parameter (None for None): the engine's shadow (kept fresh by the AdamW kernel) or a cast on
    the spot."""
    if p is None:
        return None
    pb = getattr(p, '_clv_shadow', None)
    return pb if pb is not None else p.detach().to(BF16)


def _wt(weight, wb):
    """bf16 W^T [K,N]: the engine's transposed shadow (refreshed once per step) or a transpose on the spot."""
    wt = getattr(weight, '_clv_shadow_t', None) if weight is not None else None
    return wt if wt is not None else wb.t().contiguous()


def linear_dgrad(dy2, wb, weight=None, pre=None):
    """dx [M,K] = dy [M,N] . W [N,K] (pre: times GELU'(pre), the fc2 input gradient of an MLP): as a row-streaming GEMM
    over the contraction N when that is short (<= 288) or the output is narrow (K <= 128); the LDS-tiled HIP GEMM with
    W^T as its K-contiguous B operand for every other shape it takes (own_gemm_ok), with GELU' fused into its epilogue;
    a shape outside both goes through _library_gemm."""
    N, K = wb.shape
    if pre is None and dy2.is_cuda and (N <= 288 or K <= 128 and N <= 384) and rowgemm_supported(K, N) and dy2.stride(1) == 1:
        return rowgemm(dy2, _wt(weight, wb), None)['y']
    if own_gemm_ok(dy2, K, N):
        return gemm_nt(dy2, _wt(weight, wb), aux=pre, epilogue=GEMM_EPI_DGELU if pre is not None else GEMM_EPI_NONE)
    _library_gemm('linear_dgrad', (dy2.shape[0], K, N))
    dx = torch.mm(dy2, wb)
    if pre is not None:
        out = torch.empty_like(dx)
        check(_lib.lib().clv_gelu_bwd(_ptr(dx), _ptr(pre), _ptr(out), dx.numel(), 0, _stream()), 'clv_gelu_bwd')
        return out
    return dx


# --------------------------------------------------------------------------- fp32 Linear of the projection heads
def _sgemm_strided(A, sa, B, sb, bias, Cout, M, N, K, accumulate):
    check(_lib.lib().clv_sgemm_strided(_ptr(A), _ptr(B), _ptr(bias), _ptr(Cout), M, N, K, sa[0], sa[1], sb[0], sb[1],
                                       Cout.stride(0) if Cout.dim() == 2 else 1, int(accumulate), _stream()),
          'clv_sgemm_strided')


_ONES = {}


def _ones_f32(n, device):
    """A cached all-ones fp32 vector (the bias gradient of a few-row layer is a GEMM against it): no fill kernel per use."""
    key = (int(n), str(device))
    if key not in _ONES:
        if torch.cuda.is_current_stream_capturing():
            return torch.ones(n, device=device, dtype=torch.float32)
        _ONES[key] = torch.ones(n, device=device, dtype=torch.float32)
    return _ONES[key]


class _LinearF32(torch.autograd.Function):
    """y = x W^T + b in fp32 storage and exact-f32 MFMA arithmetic (clv_sgemm_strided) for the [batch, D]-sized projection
    heads: the contrastive logits are cosines / 0.05, so these few-row GEMMs stay fp32 (the reference forces fp32 there too,
    contrastive_loss.py:102).  Forward, input gradient and weight / bias gradient are the same kernel with different
    strides; engine-managed parameters receive their gradients straight in the fp32 slab (accumulate)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        _need_gpu(x, weight)
        K = weight.shape[1]
        x2 = _c(x.float().reshape(-1, K))
        w = _c(weight.detach().float())
        M, N = x2.shape[0], w.shape[0]
        y = torch.empty(M, N, device=x.device, dtype=torch.float32)
        bf = _c(bias.detach().float()) if bias is not None else None
        _sgemm_strided(x2, (K, 1), w, (K, 1), bf, y, M, N, K, False)
        ctx.save_for_backward(x2, w)
        ctx.refs = (weight, bias)
        ctx.xshape = x.shape
        return y.view(x.shape[:-1] + (N,))

    @staticmethod
    def backward(ctx, dy):
        x2, w = ctx.saved_tensors
        weight, bias = ctx.refs
        N, K = w.shape
        dy2 = _c(dy.float().reshape(-1, N))
        M = dy2.shape[0]
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(M, K, device=dy2.device, dtype=torch.float32)
            _sgemm_strided(dy2, (N, 1), w, (1, K), None, dx, M, K, N, False)          # dx[m][k] = sum_n dy[m][n] W[n][k]
            dx = dx.view(ctx.xshape)
        sinks = _sinks(weight, bias)
        sink = sinks is not None
        if sink:
            dw, db = sinks
        else:
            dw = torch.empty(N, K, device=dy2.device, dtype=torch.float32)
            db = torch.empty(N, device=dy2.device, dtype=torch.float32) if bias is not None else None
        if bias is not None and M <= 96:
            # dW[n][k] (+)= sum_m dy[m][n] x[m][k] and db[n] (+)= sum_m dy[m][n] in ONE launch (the row sums of the A operand)
            check(_lib.lib().clv_sgemm_strided_rowsum(_ptr(dy2), _ptr(x2), _ptr(dw), _ptr(db), N, K, M, 1, N, 1, K,
                                                      dw.stride(0), int(sink), _stream()), 'clv_sgemm_strided_rowsum')
        else:
            _sgemm_strided(dy2, (1, N), x2, (1, K), None, dw, N, K, M, sink)          # dW[n][k] (+)= sum_m dy[m][n] x[m][k]
            if bias is not None:
                ones = _ones_f32(M, dy2.device)
                _sgemm_strided(dy2, (1, N), ones, (0, 1), None, db.view(N, 1), N, 1, M, sink)   # db[n] (+)= sum_m dy[m][n]
        if sink:
            _delivered(weight, bias)
            return dx, None, None
        return dx, dw.to(weight.dtype), (db.to(bias.dtype) if db is not None else None)


def linear_f32(x, weight, bias=None):
    return _LinearF32.apply(x, weight, bias)


class _Linear(torch.autograd.Function):
    """y = x W^T + b with fp32 master parameters and bf16 MFMA operands.  The forward and the
    input-gradient GEMMs are plain library GEMMs (hipBLASLt through torch); the weight/bias
    gradient of the token-parallel layers is the split-M HIP kernel (clv_linear_wgrad), in fp32.

    Engine-managed parameters carry ``_clv_shadow`` (bf16 copy kept fresh by the AdamW kernel — no
    per-step cast), ``_clv_grad`` (fp32 view of the flat gradient slab — gradients are accumulated
    there directly, no autograd AccumulateGrad add) and ``_clv_ready`` (bucket countdown of the
    gradient all-reduce)."""

    @staticmethod
    def forward(ctx, x, weight, bias, xq=None):
        _need_gpu(x, weight)
        xb = x if x.dtype == BF16 else x.to(BF16)
        wb = _raw_bf16(weight)
        N, K = wb.shape
        x2 = xb.reshape(-1, K)
        if _rowgemm_fwd_ok(xb, N, K):
            bf = bias if bias is not None and bias.dtype == torch.float32 else (bias.float() if bias is not None else None)
            y = rowgemm(x2, wb, bf)['y'].view(xb.shape[:-1] + (N,))
        elif fp8_ok(x2, N, K):
            y = gemm_nt_fp8(x2, wb, bias.detach() if bias is not None else None, aq8=xq).view(xb.shape[:-1] + (N,))
        elif own_gemm_ok(x2, N, K):
            y = gemm_nt(x2, wb, bias.detach() if bias is not None else None,
                        epilogue=GEMM_EPI_BIAS if bias is not None else GEMM_EPI_NONE).view(xb.shape[:-1] + (N,))
        else:
            _library_gemm('linear', (x2.shape[0], N, K))
            y = torch.nn.functional.linear(xb, wb, _raw_bf16(bias))
        ctx.save_for_backward(xb, wb)
        ctx.wref, ctx.bref = weight, bias
        return y

    @staticmethod
    def backward(ctx, dy):
        xb, wb = ctx.saved_tensors
        N, K = wb.shape
        dy2 = _half_rows(dy, N)
        x2 = _c(xb.reshape(-1, K))
        dx = linear_dgrad(dy2, wb, ctx.wref).view(xb.shape) if ctx.needs_input_grad[0] else None
        dw, db = (None, None)
        if ctx.needs_input_grad[1] or (ctx.bref is not None and ctx.needs_input_grad[2]):
            dw, db = _param_grads(dy2, x2, ctx.wref, ctx.bref)
        return dx, dw, db, None


_NOAFFINE_CONST = {}


def _ln_bwd_noaffine(dxhat, x, mean, rstd, dsum, gamma=None, xscale=None, rows_per_sample=1):
    """dx = LayerNorm-backward of dxhat w.r.t. x for the affine-free standardisation (+ dsum).  gamma: dxhat is the
    gradient w.r.t. the AFFINE output (taken through the raw, un-folded weight): the kernel applies gamma itself —
    d xhat = (dy W) * gamma == dy (W * gamma), so the backward needs no transpose of the folded weight."""
    rows, C_ = x.shape
    L = _lib.lib()
    nblk = L.clv_layernorm_bwd_blocks(rows, C_)
    dev = x.device
    partial = torch.empty(2 * nblk * C_, device=dev, dtype=torch.float32)
    key = (C_, str(dev))
    if key not in _NOAFFINE_CONST:          # gamma = 1 and a never-read dgamma / dbeta dump, allocated once
        _NOAFFINE_CONST[key] = (torch.ones(C_, device=dev, dtype=torch.float32),
                                torch.zeros(2 * C_, device=dev, dtype=torch.float32))
    ones, junk = _NOAFFINE_CONST[key]
    if gamma is not None:
        ones = _c(gamma.detach().float())
    dx = torch.empty_like(x)
    ds2 = _half_rows(dsum, C_) if dsum is not None else None
    # xscale: x is the saved SUM t = xscale * a + r (x_is_sum); dx then receives d t times the factor (the gradient of a)
    # and dres d t itself (the gradient of r) — both from the one kernel
    dres = torch.empty_like(x) if xscale is not None else None
    ex = _lib.ClvLnExtra(_ptr(xscale), int(rows_per_sample), 0.0, None, None, _ptr(dres), 1 if xscale is not None else 0,
                         0, 0, 0, 0)
    ex.no_reduce = 1                        # nobody reads dgamma / dbeta of the affine-free norm: skip their reduction launch
    check(L.clv_layernorm_bwd(_ptr(dxhat), _ptr(x), _ptr(None), _ptr(ones), _ptr(mean), _ptr(rstd), _ptr(ds2),
                              _ptr(dx), _ptr(junk), C.c_void_p(junk.data_ptr() + 4 * C_), _ptr(partial), rows, C_, 0,
                              C.byref(ex), _stream()), 'clv_layernorm_bwd')
    return dx if xscale is None else (dx, dres)


def fold_layernorm(weight, bias, gamma, beta):
    """LayerNorm's affine part folded into the following Linear:
    (xhat*gamma + beta) W^T + b  ==  xhat (W*gamma)^T + (b + W beta).  -> (wf bf16 [N,K], bf fp32 [N]), one kernel."""
    N, K = weight.shape
    wf = torch.empty(N, K, device=weight.device, dtype=BF16)
    bf = torch.empty(N, device=weight.device, dtype=torch.float32)
    check(_lib.lib().clv_ln_fold_fwd(_ptr(_c(weight.detach().float())), _ptr(_c(bias.detach().float())) if bias is not None else None,
                                     _ptr(_c(gamma.detach().float())), _ptr(_c(beta.detach().float())), _ptr(wf), _ptr(bf),
                                     N, K, _stream()), 'clv_ln_fold_fwd')
    return wf, bf


def _unfold_grads(dwf, dbf, weight, bias, gamma, beta):
    """Backward of fold_layernorm: (d wf, d bf) -> gradients of (weight, bias, gamma, beta), accumulated straight into
    the engine's slab views when all four are engine-managed (returns Nones), else returned."""
    N, K = weight.shape
    sinks = _sinks(weight, bias, gamma, beta)
    if sinks is not None:
        dw, db, dg, dbt = sinks
    else:
        dw = torch.zeros(N, K, device=dwf.device, dtype=torch.float32)
        db = torch.zeros(N, device=dwf.device, dtype=torch.float32) if bias is not None else None
        dg = torch.zeros(K, device=dwf.device, dtype=torch.float32)
        dbt = torch.zeros_like(dg)
    check(_lib.lib().clv_ln_fold_bwd(_ptr(dwf), _ptr(dbf), _ptr(_c(weight.detach().float())),
                                     _ptr(_c(gamma.detach().float())), _ptr(_c(beta.detach().float())), _ptr(dw), _ptr(db),
                                     _ptr(dg), _ptr(dbt), N, K, _stream()), 'clv_ln_fold_bwd')
    if sinks is not None:
        _delivered(weight, bias, gamma, beta)
        return None, None, None, None
    return (dw.to(weight.dtype), db.to(bias.dtype) if bias is not None else None, dg.to(gamma.dtype),
            dbt.to(beta.dtype))


def _wgrad_folded(dy2, xhat, xs, mean, rstd, weight, bias, gamma, beta):
    """Weight gradient of a LayerNorm-folded projection and its un-fold into (d weight, d bias, d gamma, d beta).  Inside
    defer_folds() with engine-managed parameters both are deferred: the GEMM joins the grouped launch (into a zeroed
    temporary), the un-fold kernel runs after the folds."""
    if (SEGMENT is not None and SEGMENT.wgrads is not None and xhat is not None
            and _sinks(weight, bias, gamma, beta) is not None):
        (M, N), K = dy2.shape, xhat.shape[1]
        if _wgrad_custom(M, N, K):
            in_place = bool(_lib.lib().clv_linear_wgrad_in_place(M, N, K))
            # partial slices + fold: the fold STORES into the temporary (no zero-fill launch); one in-place slice adds
            tmp = (torch.zeros if in_place else torch.empty)(N * K + N, device=dy2.device, dtype=torch.float32)
            dwf, dbf = tmp[:N * K].view(N, K), tmp[N * K:]
            SEGMENT.wgrads.append(WgradItem(dy2, xhat, dwf, dbf, M, N, K, 0 if in_place else STORE_DW | STORE_DB))
            SEGMENT.post.append(lambda: _unfold_grads(dwf, dbf, weight, bias, gamma, beta))
            return None, None, None, None
    dwf, dbf = linear_wgrad(dy2, xhat, True) if xhat is not None else linear_wgrad(dy2, xs, True, xstats=(mean, rstd))
    return _unfold_grads(dwf, dbf, weight, bias, gamma, beta)


class _FusedLNLinear(torch.autograd.Function):
    """(y, s) = (Linear(LayerNorm(a [+ r])),  a + r) in ONE row-streaming kernel: residual add, LayerNorm statistics +
    standardisation and the projection, the norm's affine part folded into the weights (swin_transformer_3d.py:450
    + :376).  Takes the raw parameters; the fold and its backward are one small kernel each."""

    @staticmethod
    def forward(ctx, a, r, ln_weight, ln_bias, weight, bias, eps, stream_out=False):
        _need_gpu(a, weight)
        K = a.shape[-1]
        N = weight.shape[0]
        a2 = _c(a).view(-1, K)
        r2 = _c(r).view(-1, K) if r is not None else None
        wt, bf = fold_layernorm(weight, bias, ln_weight, ln_bias)
        out = rowgemm(a2, wt, bf, res=r2, standardise=True, eps=eps, want_xhat=any(ctx.needs_input_grad))
        xs = out['sum'] if r is not None else a2
        ctx.save_for_backward(xs, out['mean'], out['rstd'], wt, out['xhat'])
        ctx.has_res = r is not None
        ctx.shape = a.shape
        ctx.prefs = (weight, bias, ln_weight, ln_bias)
        y = out['y'].view(a.shape[:-1] + (N,))
        if r is None and stream_out:
            # the input doubles as the residual stream of the block (first block of a stage): handing it out HERE makes the
            # stream's gradient arrive as ds and fold into dx in the LayerNorm-backward kernel — no autograd add kernel
            return y, a2.view(a.shape)
        return y, (out['sum'].view(a.shape) if r is not None else None)

    @staticmethod
    def backward(ctx, dy, ds):
        xs, mean, rstd, wt, xhat = ctx.saved_tensors
        N, K = wt.shape
        dy2 = _half_rows(dy, N)
        weight, bias, gamma, beta = ctx.prefs
        # through the raw weight (the engine keeps its transpose fresh); the norm's gamma is applied by the LN backward
        dxhat = linear_dgrad(dy2, _raw_bf16(weight), weight)
        dx = _ln_bwd_noaffine(dxhat, xs, mean, rstd, ds, gamma=gamma).view(ctx.shape)
        # the forward kept the standardised rows: the weight gradient runs on the LDS-DMA kernel
        dw, db, dg, dbt = _wgrad_folded(dy2, xhat, xs, mean, rstd, weight, bias, gamma, beta)
        return dx, (dx if ctx.has_res else None), dg, dbt, dw, db, None, None


def ln_linear(a, r, ln_weight, ln_bias, weight, bias, eps=1e-5, stream_out=False):
    """y = Linear(LayerNorm(a [+ r])), s = a + r (None without r; a itself with stream_out)."""
    return _FusedLNLinear.apply(a, r, ln_weight, ln_bias, weight, bias, eps, stream_out)


def mlp_fused_shape(C_, hidden):
    """Widths of the one-kernel MLP (clv_mlp_fused_*: both weight matrices resident in LDS): VideoSwin-T's stage 0."""
    return C_ == 96 and hidden == 384


def mlp_fused_ok(a2, hidden):
    """The one-kernel forward / backward of norm2 + Mlp (round 6) for a contiguous bf16 [M, 96] operand; CLOVER_FUSED_MLP=0
    restores the two-kernel forward (LayerNorm + fc1 + GELU, fc2) that writes the hidden activations."""
    return (os.environ.get('CLOVER_FUSED_MLP', '1') == '1' and not parity.enabled() and a2.is_cuda and a2.dtype == BF16
            and a2.dim() == 2 and a2.is_contiguous() and mlp_fused_shape(a2.shape[1], hidden)
            and a2.data_ptr() % 16 == 0)


def mlp_fused_fwd(a2, r2, w1f, b1f, w2b, b2, eps=1e-5, xscale=None, rows_per_sample=1):
    """Raw launcher of clv_mlp_fused_fwd (no autograd) -> dict(out, sum, mean, rstd)."""
    _need_gpu(a2, w1f, w2b)
    M, C_ = a2.shape
    Hd = w1f.shape[0]
    assert a2.dtype == BF16 and a2.is_contiguous() and w1f.is_contiguous() and w2b.is_contiguous()
    assert w1f.shape == (Hd, C_) and w2b.shape == (C_, Hd) and b1f.dtype == torch.float32
    out = torch.empty_like(a2)
    ssum = torch.empty_like(a2) if r2 is not None else None
    mean = torch.empty(M, device=a2.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    b2f = _c(b2.detach().float()) if b2 is not None else None
    with _Timed('mlp96_fwd_kernel', 4 * M * C_ * Hd, M * C_ * 2 * (4 if r2 is not None else 2) + 8 * M):
        check(_lib.lib().clv_mlp_fused_fwd(_ptr(a2), _ptr(r2), _ptr(ssum), _ptr(mean), _ptr(rstd), _ptr(w1f), _ptr(b1f),
                                           _ptr(w2b), _ptr(b2f), _ptr(out), M, C_, Hd, float(eps), _ptr(xscale),
                                           int(rows_per_sample), _stream()), 'clv_mlp_fused_fwd')
    return dict(out=out, sum=ssum, mean=mean, rstd=rstd)


def mlp_fused_bwd(ts, mean, rstd, do2, ds2, w1f, b1f, w2t, xscale=None, rows_per_sample=1, want_dres=False, want_xhat=True):
    """Raw launcher of clv_mlp_fused_bwd (no autograd) -> dict(da, dres, act, dpre, xhat)."""
    _need_gpu(ts, do2, w1f, w2t)
    M, C_ = ts.shape
    Hd = w1f.shape[0]
    assert ts.is_contiguous() and do2.is_contiguous() and w2t.is_contiguous() and w2t.shape == (Hd, C_)
    da = torch.empty_like(ts)
    dres = torch.empty_like(ts) if want_dres else None
    act = torch.empty(M, Hd, device=ts.device, dtype=BF16)
    dpre = torch.empty_like(act)
    xhat = torch.empty_like(ts) if want_xhat else None
    nb = M * C_ * 2 * (3 + (1 if ds2 is not None else 0) + (1 if want_dres else 0) + (1 if want_xhat else 0)) + 2 * M * Hd * 2
    with _Timed('mlp96_bwd_kernel', 10 * M * C_ * Hd, nb + 8 * M):
        check(_lib.lib().clv_mlp_fused_bwd(_ptr(ts), _ptr(mean), _ptr(rstd), _ptr(do2), _ptr(ds2), _ptr(w1f), _ptr(b1f),
                                           _ptr(w2t), _ptr(da), _ptr(dres), _ptr(act), _ptr(dpre), _ptr(xhat), M, C_, Hd,
                                           _ptr(xscale), int(rows_per_sample), _stream()), 'clv_mlp_fused_bwd')
    return dict(da=da, dres=dres, act=act, dpre=dpre, xhat=xhat)


class _FusedMLP(torch.autograd.Function):
    """(out, s) = (fc2(GELU(fc1(LN(a + r)))),  a + r): kernel 1 = residual add + LayerNorm + fc1 + bias +
    GELU (pre-activation kept), kernel 2 = fc2; backward: fc2 input-gradient GEMM with the GELU
    backward in its epilogue, split-M weight gradients (fc1's on the re-standardised rows), LayerNorm
    backward with the residual-path gradient folded in (swin_transformer_3d.py:482-483,262-268,503)."""

    @staticmethod
    def forward(ctx, a, r, ln_weight, ln_bias, w1, b1, w2, b2, eps, x_scale=None):
        _need_gpu(a, w1)
        K = a.shape[-1]
        a2 = _c(a).view(-1, K)
        r2 = _c(r).view(-1, K) if r is not None else None
        wt1, bf1 = fold_layernorm(w1, b1, ln_weight, ln_bias)
        # x_scale fp32 [B]: the per-sample DropPath factor of the branch a — folded into the residual add of the kernel's
        # prologue (t = x_scale * a + r) and, in the backward, into the LayerNorm-backward kernel (round 5: the block
        # multiplied a 19 M-element tensor by it with an elementwise pass each way, 2 x 18 us on the critical path)
        assert x_scale is None or r is not None
        xsc = _c(x_scale.detach().float()) if x_scale is not None else None
        rps = a2.shape[0] // a.shape[0]
        ctx.xsc, ctx.rps = xsc, rps
        w2b = _raw_bf16(w2)
        ctx.has_res = r is not None
        ctx.shape = a.shape
        ctx.w2ref, ctx.b2ref = w2, b2
        ctx.prefs = (w1, b1, ln_weight, ln_bias)
        ctx.one_kernel = mlp_fused_ok(a2, w1.shape[0]) and (r2 is None or (r2.is_contiguous() and r2.data_ptr() % 16 == 0))
        if ctx.one_kernel:
            # norm2 + fc1 + GELU + fc2 in ONE kernel, both weight matrices in LDS: the [M, 4C] hidden tensors (activation,
            # pre-activation) are never written — the backward recomputes them from the residual stream (clv_mlp_fused_bwd)
            o = mlp_fused_fwd(a2, r2, wt1, bf1, _c(w2b), b2, eps, xsc, rps)
            xs = o['sum'] if r is not None else a2
            ctx.save_for_backward(xs, o['mean'], o['rstd'], wt1, bf1, w2b)
            return o['out'].view(a.shape), (o['sum'].view(a.shape) if r is not None else None)
        o1 = rowgemm(a2, wt1, bf1, res=r2, standardise=True, epilogue=1, eps=eps, want_xhat=any(ctx.needs_input_grad),
                     xscale=xsc, rows_per_sample=rps)
        xs = o1['sum'] if r is not None else a2
        if own_gemm_ok(o1['y'], w2b.shape[0], w2b.shape[1]):     # fc2 of the stage-0 block (200 704 x 96 x 384)
            out = gemm_nt(o1['y'], w2b, b2.detach() if b2 is not None else None,
                          epilogue=GEMM_EPI_BIAS if b2 is not None else GEMM_EPI_NONE)
        else:
            _library_gemm('fused_mlp fc2', (o1['y'].shape[0], w2b.shape[0], w2b.shape[1]))
            out = torch.nn.functional.linear(o1['y'], w2b, _raw_bf16(b2))
        ctx.save_for_backward(xs, o1['mean'], o1['rstd'], wt1, o1['pre'], o1['y'], w2b, o1['xhat'])
        return out.view(a.shape), (o1['sum'].view(a.shape) if r is not None else None)

    @staticmethod
    def backward(ctx, dout, ds):
        if ctx.one_kernel:
            return _FusedMLP._backward_one_kernel(ctx, dout, ds)
        xs, mean, rstd, wt1, pre, act, w2b, xhat = ctx.saved_tensors
        C_, Hd = w2b.shape                              # fc2: [C, 4C]
        do2 = _half_rows(dout, C_)
        # d pre = (d out . W2) * gelu'(pre)
        if rowgemm_supported(Hd, C_) and C_ <= 288:
            dpre = rowgemm(do2, _wt(ctx.w2ref, w2b), None, epilogue=2, pre_in=pre)['y']
        else:
            _library_gemm('fused_mlp fc2 dgrad', (do2.shape[0], Hd, C_))
            dact = torch.mm(do2, w2b)
            dpre = torch.empty_like(dact)
            check(_lib.lib().clv_gelu_bwd(_ptr(dact), _ptr(pre), _ptr(dpre), dact.numel(), 0, _stream()), 'clv_gelu_bwd')
        dw2, db2 = _param_grads(do2, act, ctx.w2ref, ctx.b2ref)
        # fc1 + LayerNorm
        w1, b1, gamma, beta = ctx.prefs
        dxhat = linear_dgrad(dpre, _raw_bf16(w1), w1)
        if ctx.xsc is not None:
            dx, dr = _ln_bwd_noaffine(dxhat, xs, mean, rstd, ds, gamma=gamma, xscale=ctx.xsc, rows_per_sample=ctx.rps)
            dx, dr = dx.view(ctx.shape), dr.view(ctx.shape)
        else:
            dx = _ln_bwd_noaffine(dxhat, xs, mean, rstd, ds, gamma=gamma).view(ctx.shape)
            dr = dx
        dw1, db1, dg, dbt = _wgrad_folded(dpre, xhat, xs, mean, rstd, w1, b1, gamma, beta)
        return dx, (dr if ctx.has_res else None), dg, dbt, dw1, db1, dw2, db2, None, None

    @staticmethod
    def _backward_one_kernel(ctx, dout, ds):
        """clv_mlp_fused_bwd: recompute of the hidden activations, both input-gradient GEMMs, the GELU backward and the
        LayerNorm backward (with the stream's gradient and the DropPath factor) in one kernel; it leaves act, d pre and xhat
        for the (grouped, deferred) weight-gradient launches."""
        xs, mean, rstd, wt1, bf1, w2b = ctx.saved_tensors
        C_, Hd = w2b.shape
        do2 = _half_rows(dout, C_)
        ds2 = _half_rows(ds, C_) if ds is not None else None
        w2, b2 = ctx.w2ref, ctx.b2ref
        o = mlp_fused_bwd(xs, mean, rstd, do2, ds2, wt1, bf1, _c(_wt(w2, w2b)), ctx.xsc, ctx.rps,
                          want_dres=ctx.xsc is not None and ctx.has_res)
        dx = o['da'].view(ctx.shape)
        dr = o['dres'].view(ctx.shape) if o['dres'] is not None else dx
        dw2, db2 = _param_grads(do2, o['act'], w2, b2)
        w1, b1, gamma, beta = ctx.prefs
        dw1, db1, dg, dbt = _wgrad_folded(o['dpre'], o['xhat'], xs, mean, rstd, w1, b1, gamma, beta)
        return dx, (dr if ctx.has_res else None), dg, dbt, dw1, db1, dw2, db2, None, None


def fused_mlp(a, r, ln_weight, ln_bias, w1, b1, w2, b2, eps=1e-5, x_scale=None):
    """out = fc2(GELU(fc1(LayerNorm(x_scale * a [+ r])))), s = x_scale * a + r (x_scale fp32 [B] per sample, or None)."""
    return _FusedMLP.apply(a, r, ln_weight, ln_bias, w1, b1, w2, b2, eps, x_scale)


def fused_block_supported(C_, hidden):
    """Widths for which the fused LN+projection / MLP kernels are used (stage-0 Swin-T/B: 96, 128)."""
    return (not parity.enabled() and C_ <= 128 and rowgemm_supported(3 * C_, C_, True) and rowgemm_supported(hidden, C_, True)
            and hidden % 32 == 0)


def _fp8_side(x):
    """(q8, scale) the producing LayerNorm left on x, if x has not been written since."""
    side = getattr(x, '_clv_fp8', None) if FP8 else None
    if side is None:
        return None
    if len(side) == 3:
        if side[2] != x._version:
            return None
        side = side[:2]
    return side


def linear(x, weight, bias=None):
    if parity.enabled():
        return parity.linear(x, weight, bias)
    return _Linear.apply(x, weight, bias, _fp8_side(x))


def _param_grads(dy2, x2, weight, bias):
    """dW / db of one Linear into the engine's slab views (-> None, None) or returned to autograd."""
    sinks = _sinks(weight, bias)
    if sinks is not None:
        linear_wgrad(dy2, x2, bias is not None, *sinks)
        _delivered(weight, bias)
        return None, None
    dw, db = linear_wgrad(dy2, x2, bias is not None)
    return dw.to(weight.dtype), (db.to(bias.dtype) if db is not None else None)


class _MlpGelu(torch.autograd.Function):
    """out = fc2(GELU(fc1(x))) (Mlp.forward, swin_transformer_3d.py:262-268, no dropout) with the activation inside the
    GEMMs: fc1 = clv_gemm_nt with the bias + GELU epilogue (pre-activation kept for backward), fc2's input gradient =
    clv_gemm_nt with the GELU-backward epilogue — the two standalone GELU passes over the [M, 4C] tensor are gone."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, xq=None):
        K = x.shape[-1]
        x2 = x.reshape(-1, K)
        w1b, w2b = _raw_bf16(w1), _raw_bf16(w2)
        # the second output is GELU'(pre) rather than pre when fc2's input gradient runs on clv_gemm_nt too: its
        # epilogue then is one multiply per element (no erf / exp in the backward)
        Hd, C_ = w1b.shape[0], w2b.shape[0]
        ctx.dgelu_saved = own_gemm_ok(x2, Hd, C_)
        if ctx.dgelu_saved and fp8_ok(x2, Hd, C_):
            act, pre = gemm_nt_fp8(x2, w1b, b1.detach(), epilogue=GEMM_EPI_BIAS_GELU_D, aq8=xq)
        else:
            act, pre = gemm_nt(x2, w1b, b1.detach(),
                               epilogue=GEMM_EPI_BIAS_GELU_D if ctx.dgelu_saved else GEMM_EPI_BIAS_GELU)
        if fp8_ok(act, C_, Hd):
            out = gemm_nt_fp8(act, w2b, b2.detach() if b2 is not None else None)
        elif own_gemm_ok(act, C_, Hd):
            out = gemm_nt(act, w2b, b2.detach() if b2 is not None else None,
                          epilogue=GEMM_EPI_BIAS if b2 is not None else GEMM_EPI_NONE)
        else:
            _library_gemm('mlp_gelu fc2', (act.shape[0], C_, Hd))
            out = torch.nn.functional.linear(act, w2b, _raw_bf16(b2))
        ctx.save_for_backward(x2, pre, act, w1b, w2b)
        ctx.refs = (w1, b1, w2, b2)
        ctx.xshape = x.shape
        return out.view(x.shape[:-1] + (C_,))

    @staticmethod
    def backward(ctx, dout):
        x2, pre, act, w1b, w2b = ctx.saved_tensors
        w1, b1, w2, b2 = ctx.refs
        do2 = _half_rows(dout, w2b.shape[0])
        if ctx.dgelu_saved:                                  # pre holds GELU'(pre)
            dpre = gemm_nt(do2, _wt(w2, w2b), aux=pre, epilogue=GEMM_EPI_MUL)
        else:
            dpre = linear_dgrad(do2, w2b, w2, pre=pre)       # (d out . W2) * GELU'(pre)
        dw2, db2 = _param_grads(do2, act, w2, b2)
        dx = linear_dgrad(dpre, w1b, w1).view(ctx.xshape) if ctx.needs_input_grad[0] else None
        dw1, db1 = _param_grads(dpre, x2, w1, b1)
        return dx, dw1, db1, dw2, db2, None


def mlp_gelu_ok(x, hidden):
    """The fused-activation MLP is used where its fc1 GEMM (contraction C, 4C outputs) is one of clv_gemm_nt's shapes."""
    x2 = x.reshape(-1, x.shape[-1])
    return not parity.enabled() and x.is_cuda and x.dtype == BF16 and own_gemm_ok(x2, hidden, x.shape[-1])


def mlp_gelu(x, w1, b1, w2, b2):
    return _MlpGelu.apply(x, w1, b1, w2, b2, _fp8_side(x))


# --------------------------------------------------------------------------- LDS-tiled GEMM with fused epilogues
GEMM_EPI_NONE, GEMM_EPI_BIAS, GEMM_EPI_BIAS_GELU, GEMM_EPI_DGELU, GEMM_EPI_BIAS_GELU_D, GEMM_EPI_MUL = 0, 1, 2, 3, 4, 5


def _gemm_kname(M, N, K, epi, fp8, split=False):
    """Device-kernel name as rocprofv3 prints it (gemm_nt.hip gn_plan: tile class by rows / tile count / contraction; K in
    2-byte units for the fp8 entry point).  split: the K-slice launch (epilogue 6 = fp32 partials; its reduce kernel rides in
    the same event bracket)."""
    t128 = ((M + 127) // 128) * ((N + 127) // 128)
    t64 = ((M + 63) // 64) * ((N + 127) // 128)
    if not fp8 and M <= 1024 and K >= 512 and t64 <= 256 and N <= 3072:          # N <= GN_MAX_BIAS (gemm_nt.hip gn_plan)
        return f"gemm_ws_kernel<64, 128, 2, 2, 2, 4, {6 if split else epi}>"
    if not fp8 and t128 <= 256 and K >= 1536 and N <= 3072:
        return f"gemm_ws_kernel<128, 128, 2, 4, 2, 4, {6 if split else epi}>"
    if not fp8 and N % 192 == 0 and N <= 576 and M >= 8192:
        if ((M + 127) // 128) * (N // 192) <= 256:
            return f"gemm_nt_kernel<64, 192, 2, 2, 2, {epi}, false>"                     # 4 waves of 32 x 96, ring of 2
        return f"gemm_nt_kernel<128, 192, 4, 2, 3, {epi}, false>"                        # 8 waves of 32 x 96, ring of 3
    if K >= 512 and t128 <= 384:
        return f"gemm_nt_kernel<64, 128, 2, 2, 3, {epi}, {'true' if fp8 else 'false'}>"
    return f"gemm_nt_kernel<128, 128, 2, 4, 2, {epi}, {'true' if fp8 else 'false'}>"     # 8 waves (2 x 4), ring of 2


def gemm_nt_supported(M, N, K):
    return bool(_lib.lib().clv_gemm_nt_supported(int(M), int(N), int(K)))


def gemm_nt(a, b, bias=None, aux=None, epilogue=GEMM_EPI_NONE, out=None):
    """Raw launcher of clv_gemm_nt (no autograd): c [M,N] = a [M,K] . b [N,K]^T with the epilogue fused.
    a, b bf16 with unit inner stride; bias fp32 [N]; aux bf16 [M,N] contiguous (DGELU: the pre-activation).
    Returns c, or (c, c2) for GEMM_EPI_BIAS_GELU (c2 = pre-activation) / GEMM_EPI_BIAS_GELU_D (c2 = GELU'(pre))."""
    _need_gpu(a, b)
    M, K = a.shape
    N = b.shape[0]
    assert a.dtype == BF16 and b.dtype == BF16 and a.stride(1) == 1 and b.stride(1) == 1 and b.shape[1] == K
    c = out if out is not None else torch.empty(M, N, device=a.device, dtype=BF16)
    # c2 is addressed with c's row stride: for an `out` that is a column slice, empty_like would hand back a dense [M, N]
    # and the kernel would write past its end
    c2 = (torch.empty_strided(c.shape, c.stride(), device=c.device, dtype=BF16)
          if epilogue in (GEMM_EPI_BIAS_GELU, GEMM_EPI_BIAS_GELU_D) else None)
    if bias is not None and bias.dtype != torch.float32:
        bias = bias.float()
    if aux is not None:
        assert aux.dtype == BF16 and aux.shape == (M, N) and aux.stride(1) == 1 and aux.stride(0) == c.stride(0)
    L = _lib.lib()
    wbytes = L.clv_gemm_nt_work_bytes(M, N, K)              # > 0: the contraction runs as slices (fp32 partials + a reduce)
    work = torch.empty(wbytes, device=a.device, dtype=torch.uint8) if wbytes > 0 else None
    args = (_ptr(a), _ptr(b), _ptr(bias), _ptr(aux), _ptr(c), _ptr(c2), M, N, K, a.stride(0), b.stride(0), c.stride(0),
            int(epilogue), _ptr(work), wbytes, _stream())
    if PROF is None:
        check(L.clv_gemm_nt_ex(*args), 'clv_gemm_nt_ex')
    else:
        nout = 2 if epilogue in (GEMM_EPI_BIAS_GELU, GEMM_EPI_BIAS_GELU_D) else 1
        nin = 1 if epilogue in (GEMM_EPI_DGELU, GEMM_EPI_MUL) else 0
        with _Timed(_gemm_kname(M, N, K, int(epilogue), False, split=wbytes > 0), 2 * M * N * K,
                    (M * K + N * K + (nout + nin) * M * N) * 2):
            check(L.clv_gemm_nt_ex(*args), 'clv_gemm_nt_ex')
    return (c, c2) if epilogue in (GEMM_EPI_BIAS_GELU, GEMM_EPI_BIAS_GELU_D) else c


def transpose_batch(src_base, dst_base, table, n_entries, total_tiles):
    _need_gpu(src_base, dst_base, table)
    check(_lib.lib().clv_transpose_batch(_ptr(src_base), _ptr(dst_base), _ptr(table), int(n_entries), int(total_tiles),
                                         _stream()), 'clv_transpose_batch')


def transpose_table(entries, device):
    """entries: [(src_off, dst_off, rows, cols)] in elements -> (device table, n_entries, total_tiles) for
    transpose_batch (include/clover_hip.h: CLV_TRANSPOSE_ENTRY_BYTES layout)."""
    import struct
    raw, tile = b'', 0
    for src_off, dst_off, rows, cols in entries:
        tr, tc = (rows + 63) // 64, (cols + 63) // 64
        raw += struct.pack('<qqiiii', src_off, dst_off, rows, cols, tile, tc)
        tile += tr * tc
    t = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)
    return t, len(entries), tile


# --------------------------------------------------------------------------- row-streaming GEMM
def rowgemm_supported(N, K, standardise=False):
    return bool(_lib.lib().clv_rowgemm_supported(int(N), int(K), int(bool(standardise))))


def rowgemm(x, wt, bias=None, res=None, standardise=False, epilogue=0, pre_in=None, eps=1e-5, want_xhat=False,
            xscale=None, rows_per_sample=1):
    """Raw launcher of clv_rowgemm (no autograd).  x bf16 [M,K]; wt bf16 [N,K]; bias fp32 [N] | None.
    xscale fp32 [M / rows_per_sample]: per-sample factor on x inside the residual-add prologue (x * xscale + res).
    Returns dict(y, sum, mean, rstd, pre) (entries None when not produced)."""
    _need_gpu(x, wt)
    M, K = x.shape
    N = wt.shape[0]
    assert x.dtype == BF16 and wt.dtype == BF16 and x.stride(1) == 1 and wt.is_contiguous()
    y = torch.empty(M, N, device=x.device, dtype=BF16)
    ssum = torch.empty_like(x) if res is not None else None
    mean = torch.empty(M, device=x.device, dtype=torch.float32) if standardise else None
    rstd = torch.empty_like(mean) if standardise else None
    pre = torch.empty_like(y) if epilogue == 1 else None
    bf = _c(bias.float()) if bias is not None else None
    xhat = torch.empty_like(x) if (want_xhat and standardise) else None
    if xscale is not None:
        check(_lib.lib().clv_rowgemm_xs(_ptr(x), _ptr(res), _ptr(ssum), _ptr(mean), _ptr(rstd), _ptr(xhat), _ptr(wt), _ptr(bf),
                                        _ptr(pre_in), _ptr(y), _ptr(pre), M, N, K, x.stride(0), N, int(bool(standardise)),
                                        int(epilogue), float(eps), _ptr(xscale), int(rows_per_sample), _stream()),
              'clv_rowgemm_xs')
    else:
        check(_lib.lib().clv_rowgemm(_ptr(x), _ptr(res), _ptr(ssum), _ptr(mean), _ptr(rstd), _ptr(xhat), _ptr(wt), _ptr(bf),
                                     _ptr(pre_in), _ptr(y), _ptr(pre), M, N, K, x.stride(0), N, int(bool(standardise)),
                                     int(epilogue), float(eps), _stream()), 'clv_rowgemm')
    return dict(y=y, sum=ssum, mean=mean, rstd=rstd, pre=pre, xhat=xhat)


# --------------------------------------------------------------------------- LayerNorm
def _ln_extra(xscale, rows_per_sample, drop_p, seed, dy2=None, dres=None, x_is_sum=False, q8=None, qscale=None):
    """ClvLnExtra for the C call, or None when nothing is requested (keeps its tensors alive via the caller)."""
    if xscale is None and not drop_p and dy2 is None and dres is None and q8 is None:
        return None
    return _lib.ClvLnExtra(_ptr(xscale), int(rows_per_sample), float(drop_p or 0.0), _ptr(seed), _ptr(dy2),
                           _ptr(dres), int(x_is_sum), 0, 0, 0, 0, _ptr(q8), _ptr(qscale))


_LN_FP8_OUT = None          # side channel: the (q8, scale) pair the last _LayerNorm.forward produced (read by layer_norm)


def ln_emits_fp8(C_, f32):
    """CLOVER_FP8=1: LayerNorms whose width an fp8 GEMM can contract over also write their output as e4m3 + row scales
    (the activation operand of the QKV / FFN-in GEMM that follows: no separate quantisation pass over the activation)."""
    return FP8 and not f32 and C_ % 128 == 0 and 256 <= C_ <= 3072


class _LayerNorm(torch.autograd.Function):
    """y = LN(f(x) [+ res]); with want_sum also returns s = f(x) + res (the updated residual stream), and the
    backward folds the gradient arriving on s into dx — the Swin residual adds never run as kernels.
    f = the transforms that sit between the sub-layer and the norm in the model, applied while the row is
    loaded instead of as elementwise kernels: nn.Dropout(p) (BertSelfOutput / BertOutput) and the per-sample
    DropPath factor xscale [B] (swin_transformer_3d.py:498,503).  fork: y is returned twice (two autograd
    edges, one storage) and the backward reads both upstream gradients itself instead of autograd adding them.
    Engine-managed gamma/beta receive their gradients directly in the flat slab (atomics)."""

    @staticmethod
    def forward(ctx, x, res, gamma, beta, eps, want_sum, xscale, drop_p, fork):
        _need_gpu(x, gamma)
        C_ = x.shape[-1]
        x2 = _c(x).view(-1, C_)
        r2 = _c(res).view(-1, C_) if res is not None else None
        f32 = x2.dtype == torch.float32            # fp32 storage (projection heads) or bf16 storage
        if not f32 and x2.dtype != BF16:
            x2 = x2.to(BF16)
        if r2 is not None and r2.dtype != x2.dtype:
            r2 = r2.to(x2.dtype)
        g = _c(gamma.float())
        b = _c(beta.float())
        rows = x2.shape[0]
        y = torch.empty_like(x2)
        # want_sum without a residual or an operand transform: the "sum" IS the input — hand it out as a view (no copy), so
        # that the gradient of the stream arrives as dsum and is folded into dx by the backward kernel
        alias = bool(want_sum) and res is None and xscale is None and not drop_p
        ssum = torch.empty_like(x2) if (want_sum and not alias) else None
        mean = torch.empty(rows, device=x.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        xs = rps = seed = None
        if xscale is not None:
            xs = _c(xscale.reshape(-1).float())
            rps = rows // xs.numel()
            assert rps * xs.numel() == rows, 'xscale must have one entry per leading-dim sample'
        if drop_p:
            seed = next_dropout_seed(x.device)
        global _LN_FP8_OUT
        q8 = qs = None
        if ln_emits_fp8(C_, f32):
            q8 = torch.empty(rows, C_, device=x.device, dtype=torch.uint8)
            qs = torch.empty(rows, device=x.device, dtype=torch.float32)
        _LN_FP8_OUT = (q8, qs) if q8 is not None else None
        ex = _ln_extra(xs, rps or 1, drop_p, seed, q8=q8, qscale=qs)
        check(_lib.lib().clv_layernorm_fwd(_ptr(x2), _ptr(r2), _ptr(g), _ptr(b), _ptr(y), _ptr(ssum), _ptr(mean),
                                           _ptr(rstd), rows, C_, float(eps), int(f32),
                                           C.byref(ex) if ex is not None else None, _stream()),
              'clv_layernorm_fwd')
        if alias:
            ssum = x2
        if want_sum:
            ctx.save_for_backward(ssum, None, g, mean, rstd, xs, seed)    # f(x) + res is all the backward needs
        else:
            ctx.save_for_backward(x2, r2, g, mean, rstd, xs, seed)
        ctx.x_is_sum = bool(want_sum)
        ctx.rps, ctx.drop_p = rps or 1, float(drop_p or 0.0)
        ctx.has_res = res is not None
        ctx.xshape = x.shape
        ctx.gdtype = gamma.dtype
        ctx.gref, ctx.bref = gamma, beta
        yv = y.view(x.shape)
        return yv, (ssum.view(x.shape) if want_sum else None), (yv.view_as(yv) if fork else None)

    @staticmethod
    def backward(ctx, dy, dsum, dyf):
        x2, r2, g, mean, rstd, xs, seed = ctx.saved_tensors
        rows, C_ = x2.shape

        def prep(t):
            if t is None:
                return None
            t = _c(t).view(rows, C_)
            return t if t.dtype == x2.dtype else t.to(x2.dtype)
        dy2, ds2, dyf2 = prep(dy), prep(dsum), prep(dyf)
        if dy2 is None:
            dy2, dyf2 = dyf2, None
        if dy2 is None:
            dy2 = torch.zeros_like(x2)
        L = _lib.lib()
        nblk = L.clv_layernorm_bwd_blocks(rows, C_)
        partial = torch.empty(2 * nblk * C_, device=x2.device, dtype=torch.float32)
        dx = torch.empty_like(x2)
        xform = xs is not None or ctx.drop_p > 0
        dres = torch.empty_like(x2) if (xform and ctx.has_res) else None
        sinks = _sinks(ctx.gref, ctx.bref)
        sink = sinks is not None
        if sink:
            dg, db = sinks
        else:
            dg = torch.zeros(C_, device=x2.device, dtype=torch.float32)
            db = torch.zeros_like(dg)
        ex = _ln_extra(xs, ctx.rps, ctx.drop_p, seed, dyf2, dres, ctx.x_is_sum)
        if SEGMENT is not None and sink and L.clv_layernorm_bwd_needs_reduce(rows, C_):
            # leave the per-block partials; ONE batched launch reduces them when the backward segment closes
            if ex is None:
                ex = _lib.ClvLnExtra(None, 1, 0.0, None, None, None, int(ctx.x_is_sum), 0, 0, 0, 0)
            ex.no_reduce = 1
            SEGMENT.ln_reduces.append(LnReduceItem(partial, dg, db, nblk, C_))
        check(L.clv_layernorm_bwd(_ptr(dy2), _ptr(x2), _ptr(r2), _ptr(g), _ptr(mean), _ptr(rstd), _ptr(ds2),
                                  _ptr(dx), _ptr(dg), _ptr(db), _ptr(partial), rows, C_,
                                  int(x2.dtype == torch.float32), C.byref(ex) if ex is not None else None,
                                  _stream()), 'clv_layernorm_bwd')
        dxv = dx.view(ctx.xshape)
        drv = None
        if ctx.has_res:
            drv = dres.view(ctx.xshape) if dres is not None else dxv
        if sink:
            _delivered(ctx.gref, ctx.bref)
            return dxv, drv, None, None, None, None, None, None, None
        return dxv, drv, dg.to(ctx.gdtype), db.to(ctx.gdtype), None, None, None, None, None


def layer_norm(x, weight, bias, eps=1e-5, residual=None, return_sum=False, x_scale=None, x_dropout_p=0.0,
               fork=False):
    """y = LayerNorm(f(x) [+ residual]) over the last dim; bf16 (or fp32) in/out, fp32 statistics.
    f: optional dropout(p = x_dropout_p) then per-sample factor x_scale [B] on x (fused, see _LayerNorm).
    return_sum=True -> (y, f(x) + residual);  fork=True -> y is returned twice (y, y2 share storage; use one
    for each consumer and their gradients meet inside the LayerNorm backward kernel)."""
    if parity.enabled():                      # fp32 storage: the same kernels (forward and backward) in their fp32 instantiation
        y, s, _ = _LayerNorm.apply(x.float(), residual.float() if residual is not None else None, weight, bias, eps,
                                   bool(return_sum), x_scale, float(x_dropout_p), False)
        y = parity.rnd('act', y)
        s = parity.rnd('stream', s) if return_sum else None
        out = (y,) + ((s,) if return_sum else ()) + ((y,) if fork else ())
        return out if len(out) > 1 else y
    global _LN_FP8_OUT
    _LN_FP8_OUT = None
    y, s, y2 = _LayerNorm.apply(x, residual, weight, bias, eps, bool(return_sum), x_scale, float(x_dropout_p), bool(fork))
    if _LN_FP8_OUT is not None:               # the consumer GEMM (ops.linear / ops.mlp_gelu) picks the operand up from here
        # ... bound to the tensor's VERSION: an in-place write to y between the LayerNorm and its Linear (dropout_, add_, a
        # mask) bumps it, and _fp8_side() then drops the quantised copy instead of multiplying stale data
        y._clv_fp8 = _LN_FP8_OUT + (y._version,)
        if y2 is not None:
            y2._clv_fp8 = _LN_FP8_OUT + (y2._version,)
        _LN_FP8_OUT = None
    out = (y,) + ((s,) if return_sum else ()) + ((y2,) if fork else ())
    return out if len(out) > 1 else y


class _MergeLayerNorm(torch.autograd.Function):
    """PatchMerging's gather + LayerNorm (swin_transformer_3d.py:531-541) as ONE kernel each way, with the pending
    residual of the stage's last block folded in: y = LN(gather(xscale[b] * x + res)) over rows of 4C, where
    gather concatenates the (2h, 2w), (2h+1, 2w), (2h, 2w+1), (2h+1, 2w+1) neighbours.  x / res stay in their
    natural [B, D, H, W, C] layout — the kernels address the four source rows themselves, forward (loads) and
    backward (each gradient element is written exactly once) — so neither the strided gather copy, nor the residual
    add, nor the DropPath multiply runs as a kernel."""

    @staticmethod
    def forward(ctx, x, res, gamma, beta, eps, xscale):
        _need_gpu(x, gamma)
        B, D, H, W, Cs = x.shape
        assert H % 2 == 0 and W % 2 == 0 and Cs % 8 == 0
        x2 = _c(x if x.dtype == BF16 else x.to(BF16))
        r2 = _c(res if res.dtype == BF16 else res.to(BF16)) if res is not None else None
        g, b = _c(gamma.float()), _c(beta.float())
        H2, W2 = H // 2, W // 2
        rows = B * D * H2 * W2
        y = torch.empty(B, D, H2, W2, 4 * Cs, device=x.device, dtype=BF16)
        mean = torch.empty(rows, device=x.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        xs = _c(xscale.reshape(-1).float()) if xscale is not None else None
        assert xs is None or xs.numel() == B
        ex = _lib.ClvLnExtra(_ptr(xs), D * H2 * W2, 0.0, None, None, None, 0, Cs, H2, W2)
        check(_lib.lib().clv_layernorm_fwd(_ptr(x2), _ptr(r2), _ptr(g), _ptr(b), _ptr(y), None, _ptr(mean), _ptr(rstd),
                                           rows, 4 * Cs, float(eps), 0, C.byref(ex), _stream()), 'clv_layernorm_fwd')
        ctx.save_for_backward(x2, r2, g, mean, rstd, xs)
        ctx.geom = (B, D, H2, W2, Cs)
        ctx.gref, ctx.bref, ctx.gdtype = gamma, beta, gamma.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        x2, r2, g, mean, rstd, xs = ctx.saved_tensors
        B, D, H2, W2, Cs = ctx.geom
        rows, C_ = B * D * H2 * W2, 4 * Cs
        dy2 = _half_rows(dy, C_)
        L = _lib.lib()
        nblk = L.clv_layernorm_bwd_blocks(rows, C_)
        partial = torch.empty(2 * nblk * C_, device=x2.device, dtype=torch.float32)
        dx = torch.empty_like(x2)
        dres = torch.empty_like(x2) if (xs is not None and r2 is not None) else None
        sinks = _sinks(ctx.gref, ctx.bref)
        sink = sinks is not None
        if sink:
            dg, db = sinks
        else:
            dg = torch.zeros(C_, device=x2.device, dtype=torch.float32)
            db = torch.zeros_like(dg)
        ex = _lib.ClvLnExtra(_ptr(xs), D * H2 * W2, 0.0, None, None, _ptr(dres), 0, Cs, H2, W2)
        check(L.clv_layernorm_bwd(_ptr(dy2), _ptr(x2), _ptr(r2), _ptr(g), _ptr(mean), _ptr(rstd), None, _ptr(dx),
                                  _ptr(dg), _ptr(db), _ptr(partial), rows, C_, 0, C.byref(ex), _stream()),
              'clv_layernorm_bwd')
        drv = None if r2 is None else (dres if dres is not None else dx)
        if sink:
            _delivered(ctx.gref, ctx.bref)
            return dx, drv, None, None, None, None
        return dx, drv, dg.to(ctx.gdtype), db.to(ctx.gdtype), None, None


def merge_layer_norm(x, weight, bias, eps=1e-5, residual=None, x_scale=None):
    """LayerNorm(PatchMerging-gather(x_scale[b] * x + residual)): x, residual bf16 [B, D, H, W, C] (H, W even, C % 8 == 0)
    -> bf16 [B, D, H/2, W/2, 4C] in the reference's concat order."""
    assert not parity.enabled(), 'parity mode takes the unfused PatchMerging route'
    return _MergeLayerNorm.apply(x, residual, weight, bias, eps, x_scale)


# --------------------------------------------------------------------------- GELU
class _Gelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _need_gpu(x)
        xc = _c(x)
        if xc.dtype not in (BF16, torch.float32):
            xc = xc.to(BF16)
        y = torch.empty_like(xc)
        check(_lib.lib().clv_gelu_fwd(_ptr(xc), _ptr(y), xc.numel(), int(xc.dtype == torch.float32), _stream()),
              'clv_gelu_fwd')
        ctx.save_for_backward(xc)
        return y

    @staticmethod
    def backward(ctx, dy):
        (xc,) = ctx.saved_tensors
        dyc = _c(dy)
        if dyc.dtype != xc.dtype:
            dyc = dyc.to(xc.dtype)
        dx = torch.empty_like(xc)
        check(_lib.lib().clv_gelu_bwd(_ptr(dyc), _ptr(xc), _ptr(dx), xc.numel(), int(xc.dtype == torch.float32),
                                      _stream()), 'clv_gelu_bwd')
        return dx


def gelu(x):
    """erf GELU (nn.GELU / HF 'gelu'), bf16 or fp32 storage."""
    if parity.enabled():
        return parity.rnd('act', _Gelu.apply(x.float()))
    return _Gelu.apply(x)


# --------------------------------------------------------------------------- embedding
class _BatchNorm1d(torch.autograd.Function):
    """nn.BatchNorm1d on [B, D] fp32 (the BatchNorm variants of the projection heads, ssl_head.py:50-66,175-186,252-262)
    on clv_batchnorm1d_fwd / _bwd; running statistics are updated in place in training mode."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, training, momentum, eps):
        _need_gpu(x)
        x2 = _c(x.float())
        if x2.dim() != 2:
            raise ValueError('BatchNorm1d of the projection heads takes [B, D] rows')
        B, D = x2.shape
        if training and B < 2:
            raise ValueError('Expected more than 1 value per channel when training')     # torch's own check
        y = torch.empty_like(x2)
        mean = torch.empty(D, device=x2.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        check(_lib.lib().clv_batchnorm1d_fwd(_ptr(x2), _ptr(weight), _ptr(bias), _ptr(running_mean), _ptr(running_var),
                                             _ptr(y), _ptr(mean), _ptr(rstd), B, D, float(eps), float(momentum),
                                             int(bool(training)), _stream()), 'clv_batchnorm1d_fwd')
        ctx.save_for_backward(x2, weight, mean, rstd)
        ctx.training = bool(training)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x2, weight, mean, rstd = ctx.saved_tensors
        B, D = x2.shape
        dy2 = _c(dy.float())
        dx = torch.empty_like(x2) if ctx.needs_input_grad[0] else None
        dg = torch.empty(D, device=x2.device, dtype=torch.float32) if weight is not None else None
        db = torch.empty(D, device=x2.device, dtype=torch.float32) if ctx.has_bias else None
        check(_lib.lib().clv_batchnorm1d_bwd(_ptr(dy2), _ptr(x2), _ptr(weight), _ptr(mean), _ptr(rstd), _ptr(dx), _ptr(dg),
                                             _ptr(db), B, D, int(ctx.training), _stream()), 'clv_batchnorm1d_bwd')
        return dx, dg, db, None, None, None, None, None


def batch_norm1d(x, weight, bias, running_mean, running_var, training, momentum=0.1, eps=1e-5):
    return _BatchNorm1d.apply(x, weight, bias, running_mean, running_var, training, momentum, eps)


class _TokenMean(torch.autograd.Function):
    """Mean over the token dimensions (all but the first and the last) of a channels-last feature map, fp32 out: the spatial
    average of the vision projection head (ssl_head.py:88-94).  ``x.float().mean(dims)`` writes an fp32 copy of the map (38 MB
    at B = 8) and its backward an fp32 broadcast of the gradient plus a cast; here the forward is one reduction reading the
    bf16 map and the backward hands autograd the [N, C] gradient / n as an EXPANDED view — the accumulation with the map's
    other gradient (it also feeds the fusion encoder) is then one broadcast add."""

    @staticmethod
    def forward(ctx, x):
        ctx.shape, ctx.dtype = x.shape, x.dtype
        return x.mean(dim=tuple(range(1, x.dim() - 1)), dtype=torch.float32)

    @staticmethod
    def backward(ctx, g):
        shape = ctx.shape
        n = 1
        for d in shape[1:-1]:
            n *= d
        gs = (g * (1.0 / n)).to(ctx.dtype)
        return gs.view((shape[0],) + (1,) * (len(shape) - 2) + (shape[-1],)).expand(shape)


def token_mean(x):
    """[N, ..., C] -> fp32 [N, C]: mean over the middle dimensions (a [N, C] input has none: returned as fp32)."""
    if x.dim() < 3:
        return x.float()
    return _TokenMean.apply(x)


class _Embedding(torch.autograd.Function):
    """weight[ids] with the gradient scattered straight into the engine's gradient slab (index_add_ of the few
    hundred looked-up rows) instead of a dense [vocab, H] zero-fill + scatter + fp32 add of 94 MB each.
    Rows of padding_idx receive no gradient (as nn.Embedding)."""

    @staticmethod
    def forward(ctx, ids, weight, padding_idx):
        ctx.save_for_backward(ids)
        ctx.wref, ctx.pad = weight, padding_idx
        return weight.detach()[ids]

    @staticmethod
    def backward(ctx, dy):
        (ids,) = ctx.saved_tensors
        w = ctx.wref
        sink = _sink(w)
        flat = ids.reshape(-1)
        d = dy.reshape(-1, dy.shape[-1])
        if ctx.pad is not None:
            d = d.masked_fill((flat == ctx.pad)[:, None], 0)
        if sink is not None:
            sink.index_add_(0, flat, d.float())
            _delivered(w)
            return None, None, None
        return None, torch.zeros_like(w).index_add_(0, flat, d.to(w.dtype)), None


def embedding(ids, weight, padding_idx=None):
    """nn.Embedding forward + sink-aware backward."""
    return _Embedding.apply(ids, weight, padding_idx)


# --------------------------------------------------------------------------- attention
class _Attention(torch.autograd.Function):
    """qkv: bf16 [..tokens.., 3*nH*hd] with q|k|v packed along the last dim.  table (window mode): the module's
    relative_position_bias_table fp32 [rows, nH], read into LDS by the kernels; its gradient (the per-window dS summed over the
    windows and scattered to the table rows) goes straight into the engine's gradient slab when the parameter is engine-managed."""

    @staticmethod
    def forward(ctx, qkv, table, rid, kmask, geom_kw, seed):
        _need_gpu(qkv)
        assert qkv.dtype == BF16 and qkv.is_contiguous()
        g = ClvAttnGeom(**geom_kw)
        assert g.dropout_p == 0.0 or seed is not None
        Cdim = g.nH * g.hd
        assert qkv.shape[-1] == 3 * Cdim
        g.ldq = g.ldk = g.ldv = 3 * Cdim
        g.ldo = Cdim
        tab = None
        if table is not None:
            assert table.shape == ((2 * g.bwd - 1) * (2 * g.bwh - 1) * (2 * g.bww - 1), g.nH), table.shape
            tab = _c(table.detach().float())
        o = torch.empty(qkv.shape[:-1] + (Cdim,), device=qkv.device, dtype=BF16)
        lse = torch.empty(g.groups * g.nH * g.N, device=qkv.device, dtype=torch.float32)
        wbytes = _lib.lib().clv_attn_seq_work_bytes(C.byref(g))        # > 0: a sequence beyond the LDS, run as several parts
        seq_work = torch.empty(wbytes, device=qkv.device, dtype=torch.uint8) if wbytes > 0 else None
        g.work = seq_work.data_ptr() if seq_work is not None else None
        base = qkv.data_ptr()
        with _Timed(_kname('attn_fwd_kernel', g), *_attn_work(g, False)):
            check(_lib.lib().clv_attn_fwd(C.c_void_p(base), C.c_void_p(base + 2 * Cdim),
                                          C.c_void_p(base + 4 * Cdim), _ptr(o), _ptr(lse), _ptr(tab), _ptr(rid),
                                          _ptr(kmask), _ptr(seed), C.byref(g), _stream()), 'clv_attn_fwd')
        ctx.save_for_backward(qkv, o, lse, tab, rid, kmask, seed)
        ctx.geom = g
        ctx.tref = table
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse, tab, rid, kmask, seed = ctx.saved_tensors
        g = ctx.geom
        Cdim = g.nH * g.hd
        doc = _c(do)
        if doc.dtype != BF16:
            doc = doc.to(BF16)
        dqkv = torch.empty_like(qkv)
        dsum = torch.empty_like(lse)
        L = _lib.lib()
        wbytes = L.clv_attn_seq_work_bytes(C.byref(g))
        seq_work = torch.empty(wbytes, device=qkv.device, dtype=torch.uint8) if wbytes > 0 else None
        g.work = seq_work.data_ptr() if seq_work is not None else None
        dtab = work = sink = None
        if tab is not None:
            sink = _sink(ctx.tref)
            dtab = sink if sink is not None else torch.zeros_like(tab)
            work = torch.empty(L.clv_attn_bwd_work_bytes(C.byref(g)), device=qkv.device, dtype=torch.uint8)
            g.dbias_index = _dbias_index(g, qkv.device)
        b, d = qkv.data_ptr(), dqkv.data_ptr()
        args = (C.c_void_p(b), C.c_void_p(b + 2 * Cdim), C.c_void_p(b + 4 * Cdim), _ptr(o), _ptr(doc), _ptr(lse),
                _ptr(tab), _ptr(rid), _ptr(kmask), C.c_void_p(d), C.c_void_p(d + 2 * Cdim),
                C.c_void_p(d + 4 * Cdim), _ptr(dtab), _ptr(dsum), _ptr(work), _ptr(seed))
        if PROF is None and SEGMENT is not None and sink is not None:
            # nothing reads a table gradient before the optimizer: leave the slices' partial sums in `work` (stage bit 8) and
            # gather every attention block of this backward segment in ONE launch when it closes (flush_dbias_gathers)
            # The partial sums go to a buffer of their own (ClvAttnGeom.work): only that stays alive until the gather — the dS
            # scratch in `work` (2.5-10 GB per block at 32 frames) is released with this backward node
            part = torch.empty(L.clv_attn_dbias_partial_bytes(C.byref(g)), device=qkv.device, dtype=torch.uint8)
            g.work = part.data_ptr()
            check(L.clv_attn_bwd(*args, 15, C.byref(g), _stream()), 'clv_attn_bwd')
            ent = _lib.ClvDbiasGather()
            check(L.clv_attn_dbias_gather_entry(C.byref(g), _ptr(work), _ptr(dtab), C.byref(ent)), 'clv_attn_dbias_gather_entry')
            g.work = None
            SEGMENT.dbias.append(DbiasItem(ent, part, dtab, g.dbias_index))
        elif PROF is None:
            check(L.clv_attn_bwd(*args, 0, C.byref(g), _stream()), 'clv_attn_bwd')
        elif tab is not None and L.clv_attn_bwd_one_kernel(C.byref(g)) == 1:
            fl, by = _attn_work(g, True)           # dQ / dK / dV as one kernel (stage mask 5), then the table gradient (2)
            with _Timed(f'attn_bwd_one_kernel<{g.hd}, {(g.N + 15) // 16}>', fl, by):
                check(L.clv_attn_bwd(*args, 5, C.byref(g), _stream()), 'clv_attn_bwd')
            check(L.clv_attn_bwd(*args, 2, C.byref(g), _stream()), 'clv_attn_bwd')
        else:                                  # one event pair per device kernel (work split 2:3 of the 5 matmuls)
            fl, by = _attn_work(g, True)
            with _Timed(_kname('attn_bwd_dq_kernel', g), fl * 0.4, by * 0.5):
                check(L.clv_attn_bwd(*args, 1, C.byref(g), _stream()), 'clv_attn_bwd')
            check(L.clv_attn_bwd(*args, 2, C.byref(g), _stream()), 'clv_attn_bwd')
            with _Timed(_kname('attn_bwd_dkv_kernel', g), fl * 0.6, by * 0.5):
                check(L.clv_attn_bwd(*args, 4, C.byref(g), _stream()), 'clv_attn_bwd')
        if sink is not None:
            _delivered(ctx.tref)
            dtab = None
        elif dtab is not None:
            dtab = dtab.to(ctx.tref.dtype)
        return dqkv, dtab, None, None, None, None


# the largest window of the 16-bit kernels and of the fp32 parity kernel alike (attention.hip WIN_MAX_TOKENS, F32_MAXT * 64)
WINDOW_MAX_TOKENS = _lib.lib().clv_attn_window_max_tokens()
_WIN_REASONS = {1: 'a window extent below 1', 2: 'head dim must be 16, 32 or 64',
                3: 'more than %d tokens per window' % WINDOW_MAX_TOKENS,
                4: 'the window has more tokens than the window its relative-position table was built for',
                5: 'the staged part of the window and its table band exceed the 160 KB of LDS'}


@functools.lru_cache(maxsize=None)
def _window_refusal(window, table_window, hd):
    rc = _lib.lib().clv_attn_window_supported(*window, *table_window, hd)
    if rc == 0:
        return None
    n = window[0] * window[1] * window[2]
    return (f'window {window} = {n} tokens (table window {table_window}, head dim {hd}): {_WIN_REASONS.get(rc, rc)}; '
            f'the attention kernels take windows of up to {WINDOW_MAX_TOKENS} tokens')


def window_attention_refusal(window, table_window, hd):
    """None when the HIP window-attention kernels (16-bit and parity alike) cover the window, else the reason as text.
    window: the effective window of the call; table_window: the window the relative-position table was built for (None:
    no table).  The set itself is stated once, in clv_attn_window_supported (host only: no GPU needed)."""
    tw = tuple(int(v) for v in table_window) if table_window is not None else (0, 0, 0)
    return _window_refusal(tuple(int(v) for v in window), tw, int(hd))


def window_attention(qkv, table, rid, window, shift, num_heads, table_window=None):
    """3-D shifted-window MHA on the natural token layout.

    qkv bf16 [B,D,H,W,3C]; table fp32 [rows, nH] = the module's relative_position_bias_table built for
    `table_window` (default: `window`; pass the configured full window when `window` is a clipped one — the
    reference then uses relative_position_index[:N,:N] of the full window, swin_transformer_3d.py:386);
    rid int32 [nW,N] region ids (None = no shift mask).
    Returns o bf16 [B,D,H,W,C] already window-reversed and un-rolled.
    """
    B, D, H, W, C3 = qkv.shape
    Cdim = C3 // 3
    hd = Cdim // num_heads
    N = window[0] * window[1] * window[2]
    nW = (D // window[0]) * (H // window[1]) * (W // window[2])
    tw = tuple(table_window or window) if table is not None else (0, 0, 0)
    why = window_attention_refusal(window, tw if table is not None else None, hd)
    if why is not None:
        raise NotImplementedError(f'window attention: {why}')
    kw = dict(mode=1, groups=B * nW, N=N, nH=num_heads, hd=hd, D=D, H=H, W=W, wd=window[0], wh=window[1],
              ww=window[2], sd=shift[0], sh=shift[1], sw=shift[2], bwd=tw[0], bwh=tw[1], bww=tw[2],
              scale=float(hd) ** -0.5)
    if parity.enabled():
        return parity.attention(qkv, table, rid, None, kw)
    return _Attention.apply(qkv, table, rid, None, kw, None)


_DROPOUT_COUNTER = {}


_SEED_STRIDE = 0x9E3779B97F4A7C15 - (1 << 64)          # odd 64-bit stride (wraps)
_SEED_POOL = {}


def _dev_key(device):
    d = torch.device(device)
    return f'cuda:{torch.cuda.current_device() if d.index is None else d.index}' if d.type == 'cuda' else str(d)


def _wrap64(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= (1 << 63) else v


def dropout_seeds_begin(device, n=128):
    """Refresh the step's pool of dropout seeds: ONE kernel writes n fresh device-resident uint64 seeds and
    one advances the counter; every next_dropout_seed() until the next begin() is then a free slice.  Call
    it inside the captured region (start of the forward), so each hipGraph replay draws new masks."""
    key = _dev_key(device)
    ctr = _dropout_counter(device)
    pool = _SEED_POOL.get(key)
    if pool is None or pool['seeds'].numel() != n:
        pool = dict(seeds=torch.empty(n, device=device, dtype=torch.int64),
                    steps=torch.arange(n, device=device, dtype=torch.int64) * _SEED_STRIDE, idx=0)
        _SEED_POOL[key] = pool
    torch.add(pool['steps'], ctr, out=pool['seeds'])
    ctr.add_(_wrap64(n * _SEED_STRIDE))
    pool['idx'] = 0


def dropout_seeds_end(device):
    """Back to one counter update per seed (ops used outside a step)."""
    _SEED_POOL.pop(_dev_key(device), None)


def _dropout_counter(device):
    key = _dev_key(device)
    if key not in _DROPOUT_COUNTER:
        init = int(torch.randint(1, 2 ** 62, (1,)).item())
        _DROPOUT_COUNTER[key] = torch.tensor([init], device=device, dtype=torch.int64)
    return _DROPOUT_COUNTER[key]


def next_dropout_seed(device):
    """A fresh device-resident uint64 seed per dropout site, derived from a device counter that is
    advanced by a (capturable) kernel — so every hipGraph replay draws new masks without host traffic.
    The counter starts from torch's seeded CPU generator (torch.manual_seed controls it)."""
    pool = _SEED_POOL.get(_dev_key(device))
    if pool is not None and pool['idx'] < pool['seeds'].numel():
        i = pool['idx']
        pool['idx'] = i + 1
        return pool['seeds'][i:i + 1]
    ctr = _dropout_counter(device)
    seed = ctr.clone()
    ctr.add_(_SEED_STRIDE)
    return seed


# fused kernels: up to 448 keys staged at once, longer sequences as ceil(tiles / 28) parts + a merge, up to 4096 keys (the
# 32-frame fusion sequence has 816 tokens, the 64-frame one 1600).  Read at call time: a test sets it back to 896 to get the
# unfused path below for comparison.
SEQ_FUSED_MAX_KEYS = _lib.lib().clv_attn_seq_max_keys()


class _LongSeqAttention(torch.autograd.Function):
    """Self-attention for sequences beyond the fused kernels' reach (SEQ_FUSED_MAX_KEYS): batched library GEMMs for
    Q.K^T / P.V and their gradients, the HIP row-softmax kernels (mask + softmax + dropout, and the backward) between them."""

    @staticmethod
    def forward(ctx, qkv, kmask, num_heads, dropout_p, seed):
        _need_gpu(qkv)
        assert qkv.dtype == BF16
        B, S, C3 = qkv.shape
        Cdim = C3 // 3
        hd = Cdim // num_heads
        q, k, v = (qkv[..., i * Cdim:(i + 1) * Cdim].view(B, S, num_heads, hd).permute(0, 2, 1, 3) for i in range(3))
        _library_gemm('seq_attention (more than %d keys)' % SEQ_FUSED_MAX_KEYS, (B, num_heads, S, hd))
        scores = torch.matmul(q, k.transpose(-1, -2))                         # [B, nH, S, S] bf16
        p = torch.empty_like(scores)
        pd = torch.empty_like(scores) if dropout_p > 0 else None
        km = _c(kmask.float()) if kmask is not None else None
        scale = float(hd) ** -0.5
        check(_lib.lib().clv_softmax_rows_fwd(_ptr(scores), _ptr(km), _ptr(p), _ptr(pd), _ptr(seed),
                                              B * num_heads * S, S, S, num_heads * S, scale, float(dropout_p),
                                              _stream()), 'clv_softmax_rows_fwd')
        o = torch.matmul(pd if pd is not None else p, v)                      # [B, nH, S, hd]
        ctx.save_for_backward(qkv, p, pd, seed)
        ctx.cfg = (num_heads, hd, scale, float(dropout_p))
        return o.permute(0, 2, 1, 3).reshape(B, S, Cdim)

    @staticmethod
    def backward(ctx, do):
        qkv, p, pd, seed = ctx.saved_tensors
        num_heads, hd, scale, dropout_p = ctx.cfg
        B, S, C3 = qkv.shape
        Cdim = C3 // 3
        q, k, v = (qkv[..., i * Cdim:(i + 1) * Cdim].view(B, S, num_heads, hd).permute(0, 2, 1, 3) for i in range(3))
        doh = do.to(BF16).view(B, S, num_heads, hd).permute(0, 2, 1, 3)
        dqkv = torch.empty_like(qkv)
        dq, dk, dv = (dqkv[..., i * Cdim:(i + 1) * Cdim].view(B, S, num_heads, hd).permute(0, 2, 1, 3) for i in range(3))
        dv.copy_(torch.matmul((pd if pd is not None else p).transpose(-1, -2), doh))
        ds = torch.matmul(doh, v.transpose(-1, -2))                           # dPd, turned into dS in place
        check(_lib.lib().clv_softmax_rows_bwd(_ptr(p), _ptr(ds), _ptr(ds), _ptr(seed), B * num_heads * S, S, S,
                                              scale, dropout_p, _stream()), 'clv_softmax_rows_bwd')
        dq.copy_(torch.matmul(ds, k))
        dk.copy_(torch.matmul(ds.transpose(-1, -2), q))
        return dqkv, None, None, None, None


def seq_attention(qkv, kmask, num_heads, dropout_p=0.0):
    """BERT self-attention. qkv bf16 [B,S,3H]; kmask fp32 [B,S] additive ((1-m)*-10000) or None;
    dropout_p: dropout on the attention probabilities (HF attention_probs_dropout_prob).
    Up to SEQ_FUSED_MAX_KEYS (4096) tokens: the fused LDS-resident kernels (beyond 448 as parts of at most 448 staged
    tokens + a merge); longer sequences: the unfused library GEMM + row-softmax path (counted, refused in strict mode)."""
    B, S, C3 = qkv.shape
    hd = C3 // 3 // num_heads
    if parity.enabled():
        return parity.attention(qkv, None, None, kmask, dict(mode=0, groups=B, N=S, nH=num_heads, hd=hd,
                                                            scale=float(hd) ** -0.5, dropout_p=float(dropout_p)))
    if S > SEQ_FUSED_MAX_KEYS:
        seed = next_dropout_seed(qkv.device) if dropout_p > 0 else None
        return _LongSeqAttention.apply(qkv, kmask, num_heads, float(dropout_p), seed)
    kw = dict(mode=0, groups=B, N=S, nH=num_heads, hd=hd, scale=float(hd) ** -0.5, dropout_p=float(dropout_p))
    seed = next_dropout_seed(qkv.device) if dropout_p > 0 else None
    return _Attention.apply(qkv, None, None, kmask, kw, seed)


# --------------------------------------------------------------------------- patch embed
PE_FAST = ((2, 4, 4), (2, 4, 4))      # the geometry of clv_patch_embed_fwd (and its fp8 form); every other one: the general kernel
_PE_REASONS = {1: 'a patch extent below 1', 2: 'stride must satisfy 1 <= stride <= patch on every axis (no gaps between patches)',
               3: 'pt*ph*pw must be a multiple of 8 (K = 3*pt*ph*pw feeds the weight-gradient kernels in 16-byte groups)',
               4: 'K = 3*pt*ph*pw exceeds 384', 5: 'embed_dim must be 48, 96 or 128'}


def patch_embed_refusal(patch, stride, in_chans, Cout):
    """None when the HIP patch-embed kernels cover the geometry, else the reason as text.  The set itself is stated once,
    in clv_patch_embed_gen_supported (host only: no GPU needed)."""
    if in_chans != 3:
        return f'in_chans = {in_chans}: the kernels read 3-channel clips'
    rc = _lib.lib().clv_patch_embed_gen_supported(*(int(v) for v in patch), *(int(v) for v in stride), int(Cout))
    return None if rc == 0 else f'patch {tuple(patch)} stride {tuple(stride)} embed_dim {Cout}: {_PE_REASONS.get(rc, rc)}'


def patch_grid(T, H, W, patch=PE_FAST[0], stride=PE_FAST[1]):
    """Token grid (T', H', W') of PatchEmbed3D for a clip of T x H x W: each extent is padded up to a multiple of the
    PATCH (PatchEmbed3D.pad, the reference's :674-680), then (extent - patch) // stride + 1."""
    return tuple((-(-n // p) * p - p) // s + 1 for n, p, s in zip((T, H, W), patch, stride))


class _PatchEmbed(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, mask_token, vmask, want_clean, eps, stacked=False,
                patch=PE_FAST[0], stride=PE_FAST[1]):
        _need_gpu(x, weight)
        B, Cin, T, H, W = x.shape
        Cout = weight.shape[0]
        patch, stride = tuple(int(v) for v in patch), tuple(int(v) for v in stride)
        K = 3 * patch[0] * patch[1] * patch[2]
        why = patch_embed_refusal(patch, stride, Cin, Cout)
        if why is not None:
            raise NotImplementedError(f'patch embed: {why}')
        if tuple(weight.shape[1:]) != (3,) + patch:
            raise ValueError(f'patch embed: weight {tuple(weight.shape)} does not have the patch size {patch}')
        if T % patch[0] or H % patch[1] or W % patch[2]:
            raise ValueError(f'patch embed: clip {(T, H, W)} is not padded to multiples of the patch {patch} '
                             f'(PatchEmbed3D.pad)')
        xc = _c(x.float())
        w2 = _c(weight.reshape(Cout, K).to(BF16))
        bf = _c(bias.float())
        gf = _c(gamma.float()) if gamma is not None else None
        bef = _c(beta.float()) if beta is not None else None
        want_masked = vmask is not None
        mt = _c(mask_token.reshape(-1).float()) if want_masked else None
        vm = _c(vmask.reshape(B, vmask.shape[-2], vmask.shape[-1]).long()) if want_masked else None
        Tp, Hp, Wp = patch_grid(T, H, W, patch, stride)
        if want_masked and (Hp % vm.shape[1] or Wp % vm.shape[2]):
            raise ValueError(f'patch embed: the mask grid {tuple(vm.shape[1:])} does not divide the token grid '
                             f'{(Hp, Wp)} (the reference expands a mask cell over H\' // mh x W\' // mw tokens)')
        M = B * Tp * Hp * Wp
        dev = x.device
        need_grad = any(t is not None and t.requires_grad for t in (weight, bias, gamma, beta, mask_token))
        both = None
        if stacked:                      # clean and masked tokens as the two halves of ONE [2B, ...] tensor
            assert want_clean and want_masked
            both = torch.empty(2 * B, Tp, Hp, Wp, Cout, device=dev, dtype=BF16)
            clean, masked = both[:B], both[B:]
        else:
            clean = torch.empty(B, Tp, Hp, Wp, Cout, device=dev, dtype=BF16) if want_clean else None
            masked = torch.empty(B, Tp, Hp, Wp, Cout, device=dev, dtype=BF16) if want_masked else None
        z = torch.empty(M, Cout, device=dev, dtype=BF16) if need_grad else None
        mean = torch.empty(M, device=dev, dtype=torch.float32) if need_grad else None
        rstd = torch.empty(M, device=dev, dtype=torch.float32) if need_grad else None
        mh, mw = (vm.shape[1], vm.shape[2]) if want_masked else (1, 1)
        if (patch, stride) != PE_FAST:           # any other geometry: the general kernel, in the 16-bit type (no fp8 form)
            check(_lib.lib().clv_patch_embed_gen_fwd(_ptr(xc), _ptr(w2), _ptr(bf), _ptr(gf), _ptr(bef), _ptr(mt), _ptr(vm),
                                                     _ptr(clean), _ptr(masked), _ptr(z), _ptr(mean), _ptr(rstd), B, T, H, W,
                                                     Cout, mh, mw, *patch, *stride, float(eps), _stream()),
                  'clv_patch_embed_gen_fwd')
        elif FP8:                                # BASELINE config 5: the patch projection on the fp8 matrix instruction
            w8, wsc = quant_fp8_rows(w2)
            check(_lib.lib().clv_patch_embed_fwd_fp8(_ptr(xc), _ptr(w8), _ptr(wsc), _ptr(bf), _ptr(gf), _ptr(bef), _ptr(mt),
                                                     _ptr(vm), _ptr(clean), _ptr(masked), _ptr(z), _ptr(mean), _ptr(rstd),
                                                     B, T, H, W, Cout, mh, mw, float(eps), _stream()),
                  'clv_patch_embed_fwd_fp8')
        else:
            check(_lib.lib().clv_patch_embed_fwd(_ptr(xc), _ptr(w2), _ptr(bf), _ptr(gf), _ptr(bef), _ptr(mt), _ptr(vm),
                                                 _ptr(clean), _ptr(masked), _ptr(z), _ptr(mean), _ptr(rstd), B, T, H, W,
                                                 Cout, mh, mw, float(eps), _stream()), 'clv_patch_embed_fwd')
        ctx.save_for_backward(xc, z, mean, rstd, gf, vm)
        ctx.prefs = (weight, bias, gamma, beta, mask_token)
        ctx.meta = (B, T, H, W, Cout, want_clean, want_masked, weight.shape,
                    mask_token.shape if mask_token is not None else None)
        ctx.stacked = bool(stacked)
        ctx.geom = (patch, stride)
        if stacked:
            return both, x.new_empty(0)
        outs = (clean if want_clean else x.new_empty(0), masked if want_masked else x.new_empty(0))
        return outs

    @staticmethod
    def backward(ctx, dclean, dmasked):
        xc, z, mean, rstd, gf, vm = ctx.saved_tensors
        B, T, H, W, Cout, want_clean, want_masked, wshape, mtshape = ctx.meta
        patch, stride = ctx.geom
        K = 3 * patch[0] * patch[1] * patch[2]
        Tp, Hp, Wp = patch_grid(T, H, W, patch, stride)
        M = B * Tp * Hp * Wp
        L = _lib.lib()

        def bf(t):
            return _half_rows(t, Cout) if t is not None else None
        if ctx.stacked:                  # dclean holds the gradient of the stacked [2B, ...] output
            dclean, dmasked = (dclean[:B], dclean[B:]) if dclean is not None else (None, None)
        dc = bf(dclean) if want_clean else None
        dm = bf(dmasked) if want_masked else None
        dmt = None
        # engine-managed parameters: every gradient goes straight into its fp32 slab view (the conv weight's through the
        # deferred grouped launch) — this backward closes the video encoder's chain, and a dozen zero-fill / add kernels of
        # autograd's AccumulateGrad sat on the critical path here
        weight, bias, gamma, beta, mask_token = ctx.prefs
        ps = (weight, bias, gamma, beta, mask_token if dm is not None else None)
        sinks = _sinks(*ps)
        sink = sinks is not None
        if sink:
            wsink, bsink, gsink, besink, msink = sinks
        if dm is None:
            dyb = dc
        else:
            # dy = d_clean + d_masked (1 - w), d mask_token = sum d_masked w — one kernel (clv_patch_embed_blend_bwd)
            dyb = torch.empty(M, Cout, device=xc.device, dtype=BF16)
            dmt = msink.view(-1) if sink else torch.zeros(Cout, device=xc.device, dtype=torch.float32)
            check(L.clv_patch_embed_blend_bwd(_ptr(dc), _ptr(dm), _ptr(vm), _ptr(dyb), _ptr(dmt), B, Tp, Hp, Wp, Cout,
                                              vm.shape[1], vm.shape[2], _stream()), 'clv_patch_embed_blend_bwd')
            dmt = None if sink else dmt.reshape(mtshape)
        if gf is not None:
            nblk = L.clv_layernorm_bwd_blocks(M, Cout)
            partial = torch.empty(2 * nblk * Cout, device=xc.device, dtype=torch.float32)
            dz = torch.empty_like(z)
            if sink:
                dg, db = gsink.view(-1), besink.view(-1)
            else:
                dg = torch.zeros(Cout, device=xc.device, dtype=torch.float32)
                db = torch.zeros_like(dg)
            check(L.clv_layernorm_bwd(_ptr(dyb), _ptr(z), _ptr(None), _ptr(gf), _ptr(mean), _ptr(rstd), _ptr(None), _ptr(dz),
                                      _ptr(dg), _ptr(db), _ptr(partial), M, Cout, 0, None, _stream()),
                  'clv_layernorm_bwd')
            if sink:
                dg = db = None
        else:
            dz, dg, db = dyb, None, None
        patches = torch.empty(M, K, device=xc.device, dtype=BF16)
        check(L.clv_im2col_patches(_ptr(xc), _ptr(patches), B, T, H, W, *patch, *stride, _stream()), 'clv_im2col_patches')
        if sink:
            # the conv weight's sink goes in as its [Cout, K] VIEW, not as the attribute object: a view carries neither
            # first-touch state nor norm slots (_sinks), so this gradient always accumulates into a cleared slot and the
            # norm pass reads it.  Kept as it was: engine._setup_first_touch finds the slot non-finite in its poisoned
            # pass and goes on clearing it
            linear_wgrad(dz, patches, True, wsink.view(Cout, K), bsink.view(-1))
            _delivered(*ps)
            return (None,) * 12
        dw, dbias = linear_wgrad(dz, patches, True)
        dw = dw.reshape(wshape)
        return (None, dw, dbias, dg, db, dmt) + (None,) * 6


def patch_embed(x, weight, bias, gamma, beta, mask_token=None, vmask=None, want_clean=True, eps=1e-5,
                patch=PE_FAST[0], stride=PE_FAST[1]):
    """PatchEmbed3D + LN + mask-token blend. x fp32 [B,3,T,H,W] (already padded).
    Returns (clean, masked) bf16 [B,T',H',W',C] channels-last, (T',H',W') = patch_grid(...) (masked None without vmask).
    patch = stride = (2,4,4): clv_patch_embed_fwd; any other geometry of the supported set: clv_patch_embed_gen_fwd."""
    if parity.enabled():
        return parity.patch_embed(x, weight, bias, gamma, beta, mask_token, vmask, want_clean, eps, stride=stride)
    clean, masked = _PatchEmbed.apply(x, weight, bias, gamma, beta, mask_token, vmask, want_clean, eps, False, patch, stride)
    return (clean if want_clean else None), (masked if vmask is not None else None)


def patch_embed_stacked(x, weight, bias, gamma, beta, mask_token, vmask, eps=1e-5, patch=PE_FAST[0], stride=PE_FAST[1]):
    """As patch_embed, but the clean and the masked tokens are written as the two halves of one bf16
    [2B,T',H',W',C] tensor (clean first) — the layout the doubled Swin pass consumes, without a cat."""
    if parity.enabled():
        return parity.patch_embed(x, weight, bias, gamma, beta, mask_token, vmask, True, eps, stacked=True, stride=stride)
    return _PatchEmbed.apply(x, weight, bias, gamma, beta, mask_token, vmask, True, eps, True, patch, stride)[0]


# --------------------------------------------------------------------------- MLM decoder (vocabulary projection)
MLM_DECODER_STATS = dict(in_place=0, copied=0)      # which way _MLMDecoder.backward took its gradient (tests read it)


class _MLMDecoder(torch.autograd.Function):
    """scores [R, V] = x [R, H] . W[V, H]^T + b — BertLMPredictionHead.decoder (mlm_itm_head.py:38-41; V = 30522) on the
    step's own GEMM kernels.  V is not a multiple of 8, so every operand is used in its PHANTOM-PADDED form (engine:
    ``_clv_pad_rows``): Vp = 30528 weight rows / bias entries, the phantom ones zero.  The scores are written into a
    [R, Vp] buffer and handed out as its [R, V] view; the focal loss reads that view in place and returns its gradient the
    same way, padding columns zeroed, so that
        dx  = d scores [R, Vp] . W^T-shadow [H, Vp]^T      (clv_gemm_nt, K slices: the contraction is the vocabulary)
        dW += d scores^T x                                  (the few-row weight-gradient kernel, into the padded slab view)
    run over Vp with no edge code and no copy.  Engine-managed parameters carry the padded views (slab slots with phantom
    rows); for a model WITHOUT an engine (round 6: the parity tests, tools/test.py) the padded bf16 operands are built per
    call and the gradients come back to autograd as the [V, H] / [V] slices of padded fp32 temporaries — the same kernels
    either way, never the library GEMM."""

    @staticmethod
    def forward(ctx, x2, weight, bias):
        _need_gpu(x2, weight)
        V = weight.shape[0]
        ctx.engine = _pad_managed(weight, bias)
        if ctx.engine:
            Wp, bp = weight._clv_pad_shadow, bias._clv_pad_weight
        else:
            Vp_ = V + (-V % 64)
            Wp = torch.zeros(Vp_, weight.shape[1], device=weight.device, dtype=BF16)
            Wp[:V].copy_(weight.detach())
            bp = torch.zeros(Vp_, device=weight.device, dtype=torch.float32)
            bp[:V].copy_(bias.detach())
        Vp = Wp.shape[0]
        R = x2.shape[0]
        xb = _c(x2 if x2.dtype == BF16 else x2.to(BF16))
        buf = torch.empty(R, Vp, device=x2.device, dtype=BF16)
        gemm_nt(xb, Wp, bp, epilogue=GEMM_EPI_BIAS, out=buf)
        ctx.save_for_backward(xb, *(() if ctx.engine else (Wp,)))
        ctx.refs = (weight, bias)
        ctx.Vp = Vp
        return buf[:, :V]

    @staticmethod
    def backward(ctx, dy):
        xb, *rest = ctx.saved_tensors
        weight, bias = ctx.refs
        Vp, V = ctx.Vp, weight.shape[0]
        R = xb.shape[0]
        base = getattr(dy, '_base', None)
        if (dy.dtype == BF16 and dy.stride() == (Vp, 1) and dy.storage_offset() == 0 and base is not None
                and tuple(base.shape) == (R, Vp) and getattr(base, '_clv_dscores_pad', 0) == Vp):
            # the [R, V] view of the [R, Vp] gradient buffer the focal backward allocated for THIS purpose (it marks the
            # buffer: ``_clv_dscores_pad``; ADVICE r5 — any other [R, Vp]-strided view, e.g. one of the live scores buffer,
            # takes the copy path below and is never written): contract over it in place, padding columns cleared here
            dyp = base
            MLM_DECODER_STATS['in_place'] += 1
            if Vp > V:
                dyp[:, V:].zero_()
        else:
            MLM_DECODER_STATS['copied'] += 1
            dyp = torch.zeros(R, Vp, device=dy.device, dtype=BF16)
            dyp[:, :V].copy_(dy)
        if ctx.engine:
            dx = gemm_nt(dyp, weight._clv_pad_shadow_t) if ctx.needs_input_grad[0] else None
            linear_wgrad(dyp, xb, True, *_sinks(weight, bias, pad=True))
            _delivered(weight, bias)
            return dx, None, None
        Wp = rest[0]
        dx = gemm_nt(dyp, Wp.t().contiguous()) if ctx.needs_input_grad[0] else None
        dwp, dbp = linear_wgrad(dyp, xb, True)           # no sink: never deferred, autograd gets these gradients now
        return dx, dwp[:V].to(weight.dtype), dbp[:V].to(bias.dtype)


def _pad_managed(weight, bias):
    """Do both parameters carry the engine's phantom-padded views — the 16-bit weight and its transpose, the fp32 bias,
    and a usable padded gradient sink each (_sinks)?"""
    return (all(hasattr(weight, a) for a in ('_clv_pad_shadow', '_clv_pad_shadow_t')) and hasattr(bias, '_clv_pad_weight')
            and _sinks(weight, bias, pad=True) is not None)


def mlm_decoder_ok(x, weight, bias):
    """The own-kernel decoder: engine-managed parameters bring their phantom-padded views; without an engine the padded
    operands are built per call (hidden width a multiple of 64: whole GEMM stages).  Not the parity path."""
    if parity.enabled() or not x.is_cuda or bias is None:
        return False
    if _pad_managed(weight, bias):
        return True
    return (not hasattr(weight, '_clv_pad_shadow') and weight.shape[1] % 64 == 0 and weight.shape[1] >= 64
            and x.shape[-1] == weight.shape[1])


def mlm_decoder(x, weight, bias):
    """x [..., H] -> scores [..., V] (a view of a [rows, Vp] buffer)."""
    y = _MLMDecoder.apply(x.reshape(-1, x.shape[-1]), weight, bias)
    return y.view(x.shape[:-1] + (weight.shape[0],))


# --------------------------------------------------------------------------- fusion encoder output -> MLM decoder / reconstruction heads
class _FusionTextOut(torch.autograd.Function):
    """h [2B, S, D], the fusion encoder's output (rows [n_vis:] of a sample are its caption tokens) -> (the caption rows of
    the first B samples, [B, L, D] contiguous: the MLM decoder's input; the caption-CLS row of all 2B samples as fp32
    [2, B, D]: the two reconstruction heads' inputs).  ONE backward node that writes d h once — zeros, the caption rows, the
    CLS rows added in fp32 — where autograd's slice / unbind / select chain on the step's critical path took two zero fills,
    three copies, two casts, two adds and a cat (multimodal_transformer_pretrain.py:119-157 reads the same rows)."""

    @staticmethod
    def forward(ctx, h, n_vis):
        B2, S, D = h.shape
        ctx.cfg = (B2, S, D, int(n_vis), h.dtype)
        t_last = h[:B2 // 2, n_vis:].contiguous()
        cls = h[:, n_vis].float().reshape(2, B2 // 2, D)
        return t_last, cls

    @staticmethod
    def backward(ctx, d_t, d_cls):
        B2, S, D, n_vis, dtype = ctx.cfg
        ref = d_t if d_t is not None else d_cls
        dh = torch.zeros(B2, S, D, device=ref.device, dtype=dtype)
        if d_t is not None:
            dh[:B2 // 2, n_vis:].copy_(d_t)
        if d_cls is not None:
            dh[:, n_vis].add_(d_cls.reshape(B2, D))
        return dh, None


def fusion_text_outputs(h, n_vis):
    assert h.dim() == 3 and h.shape[0] % 2 == 0 and 0 <= n_vis < h.shape[1]
    return _FusionTextOut.apply(h, int(n_vis))


# --------------------------------------------------------------------------- focal MLM loss


class _FocalCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, gamma):
        _need_gpu(logits, labels)
        assert logits.dim() == 2 and logits.dtype in (BF16, torch.float32)
        # a [rows, V] view of a padded [rows, ld] score buffer (the MLM decoder's, ld = V rounded up to 8) is read in place
        strided = logits.stride(1) == 1 and logits.stride(0) > logits.shape[1] and logits.stride(0) % 2 == 0
        lg = logits if strided else _c(logits)
        lab = _c(labels.long())
        rows, V = lg.shape
        ld = lg.stride(0)
        dev = lg.device
        row_ce = torch.empty(rows, device=dev, dtype=torch.float32)
        row_lse = torch.empty_like(row_ce)
        acc = torch.zeros(2, device=dev, dtype=torch.float32)          # one fill for the two accumulators
        loss, count = acc[0:1], acc[1:2]
        check(_lib.lib().clv_focal_ce_fwd_ld(_ptr(lg), int(lg.dtype == BF16), _ptr(lab), _ptr(row_ce), _ptr(row_lse),
                                             _ptr(loss), _ptr(count), rows, V, ld, float(gamma), _stream()),
              'clv_focal_ce_fwd_ld')
        ctx.save_for_backward(lg, lab, row_ce, row_lse, count)
        ctx.gamma = float(gamma)
        return loss[0]

    @staticmethod
    def backward(ctx, dloss):
        lg, lab, row_ce, row_lse, count = ctx.saved_tensors
        rows, V = lg.shape
        ld = lg.stride(0)
        dl = _c(dloss.float().reshape(1))
        buf = torch.empty(rows, ld, device=lg.device, dtype=lg.dtype)         # same row stride as the scores
        if ld > V:
            buf._clv_dscores_pad = ld          # "a padded d-scores buffer nobody else reads": _MLMDecoder.backward may use it in place
        check(_lib.lib().clv_focal_ce_bwd_ld(_ptr(lg), int(lg.dtype == BF16), _ptr(lab), _ptr(row_ce), _ptr(row_lse),
                                             _ptr(count), _ptr(dl), _ptr(buf), rows, V, ld, ctx.gamma, _stream()),
              'clv_focal_ce_bwd_ld')
        return buf[:, :V], None, None      # (the kernel also zeroes the padding columns [V, ld))


def focal_ce_masked(logits, labels, gamma=2.0):
    """mean over rows with label != -100 of (1-pt)^gamma * CE(logits, label)."""
    return _FocalCE.apply(logits, labels, gamma)


# --------------------------------------------------------------------------- InfoNCE + rank
# The loss section has two sets of kernels (csrc/losses.hip): one workgroup per evaluation for a device batch, and from
# clv_infonce_large_min_g() rows on — the global batch of a virtual-rank step — log-sum-exp kernels spread over the device
# with LDS-tiled GEMMs.  NCE_FORCE_LARGE: None = dispatch by the row count; True / False pins one set (the timing tool and
# the tests that compare the two).
NCE_FORCE_LARGE = None


def nce_large_min_g():
    return int(_lib.lib().clv_infonce_large_min_g())


def _nce_fn(name, G):
    """(forward entry, backward entry) of loss `name` at G rows: both of the same set."""
    large = NCE_FORCE_LARGE if NCE_FORCE_LARGE is not None else G >= nce_large_min_g()
    L, tail = _lib.lib(), '_large' if large else ''
    return getattr(L, name + '_fwd' + tail), getattr(L, name + '_bwd' + tail)


class _InfoNCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, e0, e1, e2, e3, temperature, margin):
        _need_gpu(e0)
        es = [_c(e.float()) for e in (e0, e1, e2, e3)]
        G, Dm = es[0].shape
        L = _lib.lib()
        work = torch.empty(L.clv_infonce_work_floats(G, Dm), device=e0.device, dtype=torch.float32)
        out = torch.empty(2, device=e0.device, dtype=torch.float32)
        fwd, ctx.bwd = _nce_fn('clv_infonce', G)
        check(fwd(_ptr(es[0]), _ptr(es[1]), _ptr(es[2]), _ptr(es[3]), _ptr(out), _ptr(work), G, Dm, Dm,
                  float(temperature), float(margin), _stream()), 'clv_infonce_fwd')
        ctx.save_for_backward(*es, work)
        ctx.cfg = (G, Dm, float(temperature), float(margin), [e.dtype for e in (e0, e1, e2, e3)])
        return out[0], out[1]

    @staticmethod
    def backward(ctx, dnce, drank):
        e0, e1, e2, e3, work = ctx.saved_tensors
        G, Dm, temp, margin, dts = ctx.cfg
        dout = torch.stack([dnce.float().reshape(()), drank.float().reshape(())]).contiguous()
        ds = [torch.empty_like(e0) for _ in range(4)]
        check(ctx.bwd(_ptr(e0), _ptr(e1), _ptr(e2), _ptr(e3), _ptr(dout), _ptr(work), _ptr(ds[0]), _ptr(ds[1]), _ptr(ds[2]),
                      _ptr(ds[3]), G, Dm, Dm, temp, margin, _stream()), 'clv_infonce_bwd')
        return ds[0].to(dts[0]), ds[1].to(dts[1]), ds[2].to(dts[2]), ds[3].to(dts[3]), None, None


class _InfoNCEPacked(torch.autograd.Function):
    """The same loss on four slots of ONE packed fp32 [G, k, Dm] tensor (the layout the feature all-gather
    delivers): the kernels read the slots in place (row stride k*Dm) and write the gradient straight into the
    matching slots of a [G, k, Dm] gradient — no per-embedding copies either way."""

    @staticmethod
    def forward(ctx, packed, slots, temperature, margin):
        _need_gpu(packed)
        assert packed.dtype == torch.float32 and packed.dim() == 3 and packed.is_contiguous() and len(slots) == 4
        G, k, Dm = packed.shape
        L = _lib.lib()
        work = torch.empty(L.clv_infonce_work_floats(G, Dm), device=packed.device, dtype=torch.float32)
        out = torch.empty(2, device=packed.device, dtype=torch.float32)
        base = packed.data_ptr()
        es = [C.c_void_p(base + 4 * Dm * int(sl)) for sl in slots]
        fwd, ctx.bwd = _nce_fn('clv_infonce', G)
        check(fwd(*es, _ptr(out), _ptr(work), G, Dm, k * Dm, float(temperature), float(margin), _stream()),
              'clv_infonce_fwd')
        ctx.save_for_backward(work)
        ctx.cfg = (G, k, Dm, tuple(int(sl) for sl in slots), float(temperature), float(margin))
        return out[0], out[1]

    @staticmethod
    def backward(ctx, dnce, drank):
        work, = ctx.saved_tensors
        G, k, Dm, slots, temp, margin = ctx.cfg
        dout = torch.stack([dnce.float().reshape(()), drank.float().reshape(())]).contiguous()
        dp = torch.zeros(G, k, Dm, device=work.device, dtype=torch.float32)
        base = dp.data_ptr()
        ds = [C.c_void_p(base + 4 * Dm * sl) for sl in slots]
        check(ctx.bwd(None, None, None, None, _ptr(dout), _ptr(work), *ds, G, Dm, k * Dm, temp, margin, _stream()),
              'clv_infonce_bwd')
        return dp, None, None, None


class _InfoNCEPair(torch.autograd.Function):
    """Both evaluations of the step (video -> text, text -> video) on slots of one packed fp32 [G, k, Dm] tensor in the same
    launches (clv_infonce_pair_fwd / _bwd): 3 + 4 dependent kernels instead of 6 + 8, no zero fill of the gradient and no
    add of two partial gradients — the backward writes the whole [G, k, Dm] gradient."""

    @staticmethod
    def forward(ctx, packed, slots_a, slots_b, temperature, margin):
        _need_gpu(packed)
        assert packed.dtype == torch.float32 and packed.dim() == 3 and packed.is_contiguous()
        assert len(slots_a) == 4 and len(slots_b) == 4
        G, k, Dm = packed.shape
        L = _lib.lib()
        slots = (C.c_int32 * 8)(*[int(v) for v in tuple(slots_a) + tuple(slots_b)])
        work = torch.empty(2 * L.clv_infonce_work_floats(G, Dm), device=packed.device, dtype=torch.float32)
        out = torch.empty(4, device=packed.device, dtype=torch.float32)
        fwd, ctx.bwd = _nce_fn('clv_infonce_pair', G)
        check(fwd(_ptr(packed), slots, _ptr(out), _ptr(work), G, k, Dm, float(temperature), float(margin), _stream()),
              'clv_infonce_pair_fwd')
        ctx.save_for_backward(work)
        ctx.cfg = (G, k, Dm, slots, float(temperature), float(margin))
        return out[0], out[1], out[2], out[3]

    @staticmethod
    def backward(ctx, *douts):
        work, = ctx.saved_tensors
        G, k, Dm, slots, temp, margin = ctx.cfg
        # the four upstream gradients are read where autograd left them (no stack kernel): device pointers, NULL = 0
        ds = [d if d is None or d.dtype == torch.float32 else d.float() for d in douts]
        dout = (C.c_void_p * 4)(*[None if d is None else d.data_ptr() for d in ds])
        dp = torch.empty(G, k, Dm, device=work.device, dtype=torch.float32)
        check(ctx.bwd(dout, _ptr(work), slots, _ptr(dp), G, k, Dm, temp, margin, _stream()), 'clv_infonce_pair_bwd')
        return dp, None, None, None, None


def exclusive_infonce_rank_pair(packed, slots_a, slots_b, temperature=0.05, margin=5.0):
    """(nce_a, rank_a, nce_b, rank_b): exclusive_infonce_rank_packed on slots_a and on slots_b of the same packed tensor."""
    assert len(set(int(v) for v in slots_a)) == 4 and len(set(int(v) for v in slots_b)) == 4
    return _InfoNCEPair.apply(packed, tuple(slots_a), tuple(slots_b), temperature, margin)


def exclusive_infonce_rank_packed(packed, slots, temperature=0.05, margin=5.0):
    """(nce_loss, rank_t_tm_loss) with (video, text, text_mask, text_recon) = packed[:, slots[i]]; packed fp32
    [G, k, Dm] already gathered.  Slots must be distinct."""
    assert len(set(int(s) for s in slots)) == 4
    return _InfoNCEPacked.apply(packed, tuple(slots), temperature, margin)


def exclusive_infonce_rank(video, text, text_mask, text_recon, temperature=0.05, margin=5.0):
    """(nce_loss, rank_t_tm_loss) of ExclusiveNCEwithRankingLoss on already-gathered [G,Dm] embeddings."""
    return _InfoNCE.apply(video, text, text_mask, text_recon, temperature, margin)


class _NormSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, video, text, sim_mat, temperature, eps):
        L = _lib.lib()
        if sim_mat is not None:
            _need_gpu(sim_mat)
            x = _c(sim_mat.float())
            G, Dm = x.shape[0], 0
            if x.dim() != 2 or x.shape[1] != G:
                raise ValueError('NormSoftmaxLoss: sim_mat must be square (the diagonals are the positives)')
            v = t = None
        else:
            _need_gpu(video, text)
            v, t = _c(video.float()), _c(text.float())
            G, Dm = v.shape
            if t.shape != v.shape:
                raise ValueError(f'NormSoftmaxLoss: video {tuple(v.shape)} vs text {tuple(t.shape)}')
            x = None
        dev = (x if x is not None else v).device
        work = torch.empty(L.clv_normsoftmax_work_floats(G, Dm), device=dev, dtype=torch.float32)
        out = torch.empty(1, device=dev, dtype=torch.float32)
        fwd, ctx.bwd = _nce_fn('clv_normsoftmax', G)
        check(fwd(_ptr(v), _ptr(t), _ptr(x), _ptr(out), _ptr(work), G, Dm, float(temperature), float(eps), _stream()),
              'clv_normsoftmax_fwd')
        ctx.save_for_backward(work, *([x] if x is not None else []))
        ctx.cfg = (G, Dm, float(temperature), None if x is not None else (video.dtype, text.dtype),
                   sim_mat.dtype if x is not None else None)
        return out[0]

    @staticmethod
    def backward(ctx, dloss):
        work, *rest = ctx.saved_tensors
        G, Dm, temp, dts, sdt = ctx.cfg
        dout = _c(dloss.float().reshape(1))
        if rest:
            dsim = torch.empty_like(rest[0])
            check(ctx.bwd(_ptr(rest[0]), _ptr(dout), _ptr(work), None, None, _ptr(dsim), G, Dm, temp, _stream()),
                  'clv_normsoftmax_bwd')
            return None, None, dsim.to(sdt), None, None
        dv = torch.empty(G, Dm, device=work.device, dtype=torch.float32)
        dt = torch.empty_like(dv)
        check(ctx.bwd(None, _ptr(dout), _ptr(work), _ptr(dv), _ptr(dt), None, G, Dm, temp, _stream()),
              'clv_normsoftmax_bwd')
        return dv.to(dts[0]), dt.to(dts[1]), None, None, None


class _DualSoftmaxLoss(torch.autograd.Function):
    """NormSoftmaxLoss under the dual-softmax prior (csrc/losses.hip clv_dsl_loss_*): dtype handling as _NormSoftmax."""

    @staticmethod
    def forward(ctx, video, text, temperature, eps, T):
        L = _lib.lib()
        _need_gpu(video, text)
        v, t = _c(video.float()), _c(text.float())
        if v.dim() != 2 or t.shape != v.shape:
            raise ValueError(f'NormSoftmaxLoss: video {tuple(v.shape)} vs text {tuple(t.shape)}')
        G, Dm = v.shape
        work = torch.empty(L.clv_dsl_loss_work_floats(G, Dm), device=v.device, dtype=torch.float32)
        out = torch.empty(1, device=v.device, dtype=torch.float32)
        fwd, ctx.bwd = _nce_fn('clv_dsl_loss', G)
        check(fwd(_ptr(v), _ptr(t), _ptr(out), _ptr(work), G, Dm, float(temperature), float(eps), T, _stream()),
              'clv_dsl_loss_fwd')
        ctx.save_for_backward(work)
        ctx.cfg = (G, Dm, float(temperature), T, video.dtype, text.dtype)
        return out[0]

    @staticmethod
    def backward(ctx, dloss):
        work, = ctx.saved_tensors
        G, Dm, temp, T, vdt, tdt = ctx.cfg
        dout = _c(dloss.float().reshape(1))
        dv = torch.empty(G, Dm, device=work.device, dtype=torch.float32)
        dt = torch.empty_like(dv)
        check(ctx.bwd(_ptr(dout), _ptr(work), _ptr(dv), _ptr(dt), G, Dm, temp, T, _stream()), 'clv_dsl_loss_bwd')
        return dv.to(vdt), dt.to(tdt), None, None, None


def dual_softmax_temperature(T, sim_mat=False):
    """The checked ``dual_softmax`` of a loss: a finite float >= 0 (the rule and the message of
    ``evaluation.dual_softmax_scores``); refused together with a given score matrix."""
    T = float(T)
    if not 0 <= T < float('inf'):                             # false for NaN too
        raise ValueError(f'dual_softmax: T must be finite and >= 0 (got {T})')
    if sim_mat:
        raise ValueError('NormSoftmaxLoss: sim_mat together with dual_softmax is refused: that matrix is already divided by '
                         'a temperature, so the scale of the prior softmax(T * cosine) is undefined; pass the embeddings')
    return T


def norm_softmax_loss(video=None, text=None, sim_mat=None, temperature=0.07, eps=1e-12, dual_softmax=None):
    """NormSoftmaxLoss (contrastive_loss.py:26-68) on already-gathered [G,Dm] embeddings or a [G,G] sim_mat.
    ``dual_softmax = T`` (not in the reference): the same loss on the logits (G / temperature) c softmax(T c) with the prior
    down the video axis (video -> text) and along the text axis (text -> video), c the cosine — the loss whose inference
    form ``retrieval_rank(..., dual_softmax=T)`` is; T = 0 is the plain loss.  Embeddings only."""
    if dual_softmax is None:
        return _NormSoftmax.apply(video, text, sim_mat, temperature, eps)
    T = dual_softmax_temperature(dual_softmax, sim_mat is not None)
    return _DualSoftmaxLoss.apply(video, text, temperature, eps, T)


# --------------------------------------------------------------------------- optimizer primitives
def sumsq_accumulate(flat_grad, acc):
    """acc += sum(g^2); g fp32, or the bf16 wire copy of a data-parallel job."""
    _need_gpu(flat_grad, acc)
    if flat_grad.dtype == BF16:
        check(_lib.lib().clv_sumsq_bf16(_ptr(flat_grad), _ptr(acc), flat_grad.numel(), _stream()), 'clv_sumsq_bf16')
    else:
        check(_lib.lib().clv_sumsq(_ptr(flat_grad), _ptr(acc), flat_grad.numel(), _stream()), 'clv_sumsq')


def pack_bf16(src, dst):
    """dst (bf16) = src (fp32), the wire copy of a gradient-slab slice (clv_pack_bf16)."""
    _need_gpu(src, dst)
    assert src.dtype == torch.float32 and dst.dtype == BF16 and src.numel() == dst.numel()
    check(_lib.lib().clv_pack_bf16(_ptr(src), _ptr(dst), src.numel(), _stream()), 'clv_pack_bf16')


def adamw_step(p, g, m, v, shadow, sumsq, lr, beta1, beta2, eps, weight_decay, step, max_norm, grad_scale=1.0):
    _need_gpu(p, g, m, v)
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    check(_lib.lib().clv_adamw_step(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(shadow), _ptr(sumsq), p.numel(),
                                    float(lr), float(beta1), float(beta2), float(eps), float(weight_decay),
                                    float(bc1), float(bc2), float(max_norm), float(grad_scale), _stream()),
          'clv_adamw_step')


OPTIM_STATE_BYTES = 64


def optim_state_new(device):
    """Device-resident optimizer scalars (include/clover_hip.h: CLV_OPTIM_STATE_BYTES), zero-initialised."""
    return torch.zeros(OPTIM_STATE_BYTES // 4, device=device, dtype=torch.int32)


def optim_state_read(state):
    """Host copy (syncs): dict(coef, bc1, bc2_sqrt, norm, skip, t, skipped) + the loss scaler's fields."""
    raw = state.detach().cpu()
    f = raw.view(torch.float32)
    return dict(coef=float(f[0]), bc1=float(f[1]), bc2_sqrt=float(f[2]), norm=float(f[3]), skip=int(raw[4]),
                t=int(raw[5]), skipped=int(raw[6]), loss_scale=float(f[8]), scale_factor=float(f[9]),
                scale_window=int(raw[10]), scale_iter=int(raw[11]), last_overflow=int(raw[12]), dynamic=int(raw[13]))


def optim_state_set_scaler(state, init_scale, dynamic, scale_factor=2.0, scale_window=1000, scale_iter=0, last_overflow=-1):
    """Write the loss scaler's half of the state (LossScaler.__init__ / load_state_dict, fp16_utils.py:314-327,375-385)."""
    f = state.view(torch.float32)
    f[8] = float(init_scale)
    f[9] = float(scale_factor)
    state[10] = int(scale_window)
    state[11] = int(scale_iter)
    state[12] = int(last_overflow)
    state[13] = 1 if dynamic else 0


def optim_prep(sumsq, state, beta1, beta2, max_norm, grad_scale=1.0, slots=None):
    """slots: the CLV_SUMSQ_SLOTS norm slots the weight-gradient kernels filled (fused gradient norm): added in and re-zeroed."""
    _need_gpu(sumsq, state)
    check(_lib.lib().clv_optim_prep_slots(_ptr(sumsq), _ptr(slots), _ptr(state), float(beta1), float(beta2), float(max_norm),
                                          float(grad_scale), _stream()), 'clv_optim_prep')


SUMSQ_SLOTS, SUMSQ_CHUNK = 64, 16384         # include/clover_hip.h: CLV_SUMSQ_SLOTS, CLV_SUMSQ_CHUNK


def sumsq_range_table(ranges, device):
    """Device table for clv_sumsq_ranges: the (start, end) element ranges of one fp32 buffer cut into blocks of <= SUMSQ_CHUNK
    floats (starts must be multiples of 4: slab slots are 8-element aligned).  -> (int64 tensor [blocks][2], blocks)."""
    rows = []
    for a, b in ranges:
        assert a % 4 == 0 and b >= a
        while a < b:
            n = min(SUMSQ_CHUNK, b - a)
            rows.append((a, n))
            a += n
    t = torch.tensor(rows if rows else [(0, 0)], dtype=torch.int64, device=device)
    return t, len(rows)


def sumsq_ranges(base, table, n_blocks, acc):
    """acc[0] += sum of squares of base over the table's ranges, one launch."""
    _need_gpu(base, acc)
    if n_blocks:
        check(_lib.lib().clv_sumsq_ranges(_ptr(base), _ptr(table), int(n_blocks), _ptr(acc), _stream()), 'clv_sumsq_ranges')


def adamw_step_dev(p, g, m, v, shadow, state, lr, beta1, beta2, eps, weight_decay):
    _need_gpu(p, g, m, v, state)
    # algorithmic traffic: p, g, m, v read + p, m, v written (fp32) + the bf16 compute copy
    fn = _lib.lib().clv_adamw_step_dev_bf16g if g.dtype == BF16 else _lib.lib().clv_adamw_step_dev
    gbytes = 2 if g.dtype == BF16 else 4
    with _Timed('adamw_dev_kernel', 12 * p.numel(), (24 + gbytes + (2 if shadow is not None else 0)) * p.numel()):
        check(fn(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(shadow), _ptr(state), p.numel(),
                 float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), _stream()), 'clv_adamw_step_dev')


# --------------------------------------------------------------------------- weight EMA (csrc/ema.hip)
EMA_CHUNK = 4096                           # include/clover_hip.h: CLV_EMA_CHUNK


class EmaTable(NamedTuple):
    """Device tables of clv_ema_update / clv_ema_swap over one list of (p, ema, shadow) tensors (ema_table)."""
    update: torch.Tensor                   # int64: n_entries x {p, ema, n}, then n_blocks x {entry, start}
    swap: torch.Tensor                     # int64: n_entries x {p, ema, shadow, n}, then the same block records
    n_entries: int
    n_blocks: int
    numel: int                             # elements of all entries
    shadow_numel: int                      # ... of the entries with a 16-bit copy
    tensors: tuple                         # the tensors the tables point into (kept alive with them)


def ema_table(entries, device):
    """Tables for ema_update / ema_swap.  ``entries``: (p, ema) or (p, ema, shadow) tuples — fp32 tensors of equal size,
    contiguous, on ``device``; ``shadow`` (or None) is the 16-bit compute copy of ``p`` that a swap rewrites.  A whole slab
    is ONE entry; a loose tensor may have any length and any (4-byte) alignment.  Every entry is cut into chunks of
    EMA_CHUNK floats, one 256-thread block each."""
    device = torch.device(device)
    rows_u, rows_s, blocks, keep, total, shadowed = [], [], [], [], 0, 0
    for i, ent in enumerate(entries):
        p, ema = ent[0], ent[1]
        shadow = ent[2] if len(ent) > 2 else None
        _need_gpu(p, ema, shadow)
        n = p.numel()
        for t, dt, what in ((p, torch.float32, 'p'), (ema, torch.float32, 'ema'), (shadow, BF16, 'shadow')):
            if t is None:
                continue
            if t.dtype != dt or t.numel() != n or not t.is_contiguous() or t.device != p.device:
                raise ValueError(f'ema_table: entry {i}: {what} must be a contiguous {dt} tensor of {n} elements on '
                                 f'{p.device}, got {t.dtype} {tuple(t.shape)} on {t.device}')
        if p.data_ptr() == ema.data_ptr() and n:
            raise ValueError(f'ema_table: entry {i}: p and ema are the same memory')
        rows_u.append((p.data_ptr(), ema.data_ptr(), n))
        rows_s.append((p.data_ptr(), ema.data_ptr(), shadow.data_ptr() if shadow is not None else 0, n))
        starts = torch.arange(0, n, EMA_CHUNK, dtype=torch.int64)
        blocks.append(torch.stack([torch.full_like(starts, i), starts], 1))
        keep += [p, ema] + ([shadow] if shadow is not None else [])
        total += n
        shadowed += n if shadow is not None else 0
    blk = torch.cat(blocks).reshape(-1) if blocks else torch.zeros(0, dtype=torch.int64)

    def table(rows, width):
        head = torch.tensor(rows, dtype=torch.int64).reshape(-1) if rows else torch.zeros(0, dtype=torch.int64)
        assert head.numel() == width * len(rows)
        t = torch.cat([head, blk])
        return (t if t.numel() else torch.zeros(1, dtype=torch.int64)).to(device)

    return EmaTable(table(rows_u, 3), table(rows_s, 4), len(rows_u), blk.numel() // 2, total, shadowed, tuple(keep))


def ema_update(table, momentum):
    """ema = (1 - momentum) * ema + momentum * p over every entry of the table: one launch, fp32, on the current stream.
    ``momentum`` is a launch argument: it may change every call at no cost."""
    momentum = float(momentum)
    if not 0.0 <= momentum <= 1.0:
        raise ValueError(f'ema_update: momentum must lie in [0, 1], got {momentum}')
    with _Timed('ema_update_kernel', 3 * table.numel, 12 * table.numel):
        check(_lib.lib().clv_ema_update(_ptr(table.update), table.n_entries, table.n_blocks, momentum, _stream()),
              'clv_ema_update')


def ema_swap(table):
    """Exchange p and ema of every entry in place, bit for bit, and rewrite the 16-bit copies of the new p: one launch."""
    with _Timed('ema_swap_kernel', 0, 16 * table.numel + 2 * table.shadow_numel):
        check(_lib.lib().clv_ema_swap(_ptr(table.swap), table.n_entries, table.n_blocks, _stream()), 'clv_ema_swap')


# --------------------------------------------------------------------------- overflow report (csrc/grad_report.hip)
GRAD_REPORT_HEADER_WORDS, GRAD_REPORT_STAT_WORDS = 8, 4      # include/clover_hip.h: CLV_GRAD_REPORT_HEADER_BYTES / _STAT_BYTES


class GradReportTable(NamedTuple):
    """Device table of clv_grad_report over the parameters of one gradient buffer (grad_report_table)."""
    table: torch.Tensor                    # int64: n_params x {first chunk, chunks}, then n_chunks x {parameter, start, count}
    n_params: int
    n_chunks: int
    extent: int                            # one past the last element a chunk covers: what a buffer must hold at least
    numels: tuple                          # elements per parameter
    numel: int                             # ... of all of them


def grad_report_chunks(params_offsets):
    """The host half of grad_report_table.  ``params_offsets``: one (offset, numel) pair per parameter, in elements of the
    buffer.  -> (rows {first chunk, chunks} per parameter, rows {parameter, start, count} per chunk): every parameter cut
    into chunks of <= SUMSQ_CHUNK elements, its chunks adjacent and in order; an empty parameter has none."""
    prows, crows = [], []
    for i, (off, n) in enumerate(params_offsets):
        off, n = int(off), int(n)
        if off < 0 or n < 0 or n >= 2 ** 31:
            raise ValueError(f'grad_report_table: parameter {i}: offset {off}, numel {n} (need offset >= 0, 0 <= numel < 2^31)')
        prows.append((len(crows), (n + SUMSQ_CHUNK - 1) // SUMSQ_CHUNK))
        crows += [(i, off + a, min(SUMSQ_CHUNK, n - a)) for a in range(0, n, SUMSQ_CHUNK)]
    return prows, crows


def grad_report_table(params_offsets, device):
    """Table for grad_report over one gradient buffer (an fp32 slab or its 16-bit wire copy: the offsets are elements, so one
    table serves both).  Offsets of any alignment are legal; 8-element aligned ones, as the slabs lay parameters out, put
    every chunk on a 16-byte boundary."""
    device = torch.device(device)
    if device.type != 'cuda':
        raise RuntimeError('clover_amd ops run only on a HIP device (MI355X); there is no CPU fallback — '
                           'got device %s' % device)
    prows, crows = grad_report_chunks(params_offsets)
    flat = [v for r in prows for v in r] + [v for r in crows for v in r]
    t = torch.tensor(flat if flat else [0], dtype=torch.int64).to(device)
    return GradReportTable(t, len(prows), len(crows), max((s + c for _, s, c in crows), default=0),
                           tuple(int(n) for _, n in params_offsets), sum(int(n) for _, n in params_offsets))


def grad_report_new(table, device):
    """A zeroed report buffer for ``table`` (int32 words: header, one record per parameter, one per chunk)."""
    words = GRAD_REPORT_HEADER_WORDS + GRAD_REPORT_STAT_WORDS * (table.n_params + table.n_chunks)
    return torch.zeros(words, dtype=torch.int32, device=device)


def grad_report(buf, table, state, out, mode):
    """Per-parameter {non-finite count, largest finite |g|, sum of squares of the finite g} of the gradient buffer ``buf``
    (fp32, or the 16-bit storage type) into ``out``: two launches on the current stream, no host sync, capturable.
    ``mode`` 0: only when ``state`` says the step was skipped — otherwise both kernels return at once and ``out`` keeps the
    last skipped step's report; 1: always."""
    _need_gpu(buf, table.table, state, out)
    if buf.dtype not in (torch.float32, BF16) or not buf.is_contiguous():
        raise ValueError(f'grad_report: buf must be a contiguous fp32 or {BF16} tensor, got {buf.dtype}')
    if buf.numel() < table.extent:
        raise ValueError(f'grad_report: the table covers {table.extent} elements, buf holds {buf.numel()}')
    words = GRAD_REPORT_HEADER_WORDS + GRAD_REPORT_STAT_WORDS * (table.n_params + table.n_chunks)
    if out.dtype != torch.int32 or out.numel() < words or not out.is_contiguous():
        raise ValueError(f'grad_report: out must be a contiguous int32 tensor of >= {words} words (grad_report_new)')
    if state.dtype != torch.int32 or state.numel() * 4 < OPTIM_STATE_BYTES:
        raise ValueError('grad_report: state is the int32 record of optim_state_new')
    if mode not in (0, 1):
        raise ValueError(f'grad_report: mode is 0 (on skip) or 1 (always), got {mode!r}')
    gbytes = 2 if buf.dtype == BF16 else 4
    with _Timed('grad_report_kernel', 3 * table.numel, gbytes * table.numel):
        check(_lib.lib().clv_grad_report(_ptr(buf), 1 if buf.dtype == BF16 else 0, _ptr(table.table), table.n_params,
                                         table.n_chunks, _ptr(state), _ptr(out), int(mode), _stream()), 'clv_grad_report')


def grad_report_read(out, table):
    """Host copy of a report (syncs): dict(t, skipped, loss_scale, n_params, nonfinite, max_abs, sumsq, norm), the last four
    one CPU tensor each with one entry per parameter, in the buffer's units.  n_params == 0: no call has reported yet."""
    raw = out.detach().cpu()
    f = raw.view(torch.float32)
    a, b = GRAD_REPORT_HEADER_WORDS, GRAD_REPORT_HEADER_WORDS + GRAD_REPORT_STAT_WORDS * table.n_params
    return dict(t=int(raw[0]), skipped=int(raw[1]), loss_scale=float(f[2]), n_params=int(raw[3]), nonfinite=raw[a:b:4].clone(),
                max_abs=f[a + 1:b:4].clone(), sumsq=f[a + 2:b:4].clone(), norm=f[a + 3:b:4].clone())


# --------------------------------------------------------------------------- activation report (csrc/act_report.hip)
ACT_REPORT_SLOT_WORDS = 4                 # include/clover_hip.h: CLV_ACT_REPORT_SLOT_BYTES


def act_report_new(n_slots, device):
    """Zeroed activation-report buffers for ``n_slots`` records -> (live, latched), int32 words: ``live`` is the table
    act_report folds into (row i = slot i: {nonfinite, max_abs bits, calls, 0}), ``latched`` a header plus a copy of it."""
    device = torch.device(device)
    if device.type != 'cuda':
        raise RuntimeError('clover_amd ops run only on a HIP device (MI355X); there is no CPU fallback — '
                           'got device %s' % device)
    if int(n_slots) < 0:
        raise ValueError(f'act_report_new: n_slots {n_slots}')
    live = torch.zeros(max(int(n_slots), 1), ACT_REPORT_SLOT_WORDS, dtype=torch.int32, device=device)
    latched = torch.zeros(GRAD_REPORT_HEADER_WORDS + ACT_REPORT_SLOT_WORDS * int(n_slots), dtype=torch.int32, device=device)
    return live, latched


def act_report(t, slot_view):
    """Fold the contiguous fp32 / 16-bit tensor ``t`` into one record (``slot_view``: a row of act_report_new's live
    table): nonfinite += its NaN / inf count, max_abs = max(max_abs, largest finite |t|), calls += 1.  One launch on the
    current stream, no host sync, capturable; integer atomics only, so the record does not depend on block order."""
    _need_gpu(t, slot_view)
    if t.dtype not in (torch.float32, BF16) or not t.is_contiguous():
        raise ValueError(f'act_report: t must be a contiguous fp32 or {BF16} tensor, got {t.dtype}'
                         f'{"" if t.is_contiguous() else " (not contiguous)"}')
    if slot_view.dtype != torch.int32 or slot_view.numel() != ACT_REPORT_SLOT_WORDS or not slot_view.is_contiguous():
        raise ValueError(f'act_report: slot_view is one record of {ACT_REPORT_SLOT_WORDS} int32 words (a row of act_report_new)')
    n = t.numel()
    with _Timed('act_report_kernel', 2 * n, t.element_size() * n):
        check(_lib.lib().clv_act_report(_ptr(t) if n else None, n, 1 if t.dtype == BF16 else 0, _ptr(slot_view), _stream()),
              'clv_act_report')


def act_report_latch(state, live, latched, n_slots):
    """Behind optim_prep: if ``state`` says the step was skipped, ``latched`` = header {t, skipped, loss_scale of those
    gradients, n_slots} + a copy of the first ``n_slots`` records of ``live``; otherwise nothing is written.  One launch."""
    _need_gpu(state, live, latched)
    n_slots = int(n_slots)
    if live.dtype != torch.int32 or not live.is_contiguous() or live.numel() < ACT_REPORT_SLOT_WORDS * n_slots:
        raise ValueError(f'act_report_latch: live must be a contiguous int32 table of >= {n_slots} records')
    words = GRAD_REPORT_HEADER_WORDS + ACT_REPORT_SLOT_WORDS * n_slots
    if latched.dtype != torch.int32 or not latched.is_contiguous() or latched.numel() < words:
        raise ValueError(f'act_report_latch: latched must be a contiguous int32 tensor of >= {words} words (act_report_new)')
    if state.dtype != torch.int32 or state.numel() * 4 < OPTIM_STATE_BYTES:
        raise ValueError('act_report_latch: state is the int32 record of optim_state_new')
    check(_lib.lib().clv_act_report_latch(_ptr(state), _ptr(live), _ptr(latched), n_slots, _stream()), 'clv_act_report_latch')


def act_report_read(buf, n_slots, latched):
    """Host copy (syncs) of act_report_new's ``latched`` buffer (latched=True) or ``live`` table (False): dict(t, skipped,
    loss_scale, n_slots — all None for the live table; n_slots == 0 in a latched buffer: nothing was latched yet —
    nonfinite, max_abs, calls: one CPU tensor each with an entry per slot; max_abs fp32)."""
    raw = buf.detach().cpu().reshape(-1)
    n_slots = int(n_slots)
    head = dict(t=None, skipped=None, loss_scale=None, n_slots=None)
    a = 0
    if latched:
        head = dict(t=int(raw[0]), skipped=int(raw[1]), loss_scale=float(raw.view(torch.float32)[2]), n_slots=int(raw[3]))
        a = GRAD_REPORT_HEADER_WORDS
    rec = raw[a:a + ACT_REPORT_SLOT_WORDS * n_slots].reshape(n_slots, ACT_REPORT_SLOT_WORDS)
    return dict(head, nonfinite=rec[:, 0].clone(), max_abs=rec[:, 1].clone().view(torch.float32), calls=rec[:, 2].clone())


# --------------------------------------------------------------------------- video QA / fill-in-the-blank (csrc/qa.hip)
QA_MASK_ID = 103         # BERT [MASK]: the answer row of fill-in-the-blank (multimodal_transformer_finetune.py:100-102)


def qa_answer_rows(token_ids, seq_len, base, answer_mask, mask_id=QA_MASK_ID):
    """The QA head's row table into a fusion output [N, seq_len, D] viewed as [N * seq_len, D], built on the device (no
    host sync, capturable): row n * seq_len + base (answer_cls), or + the first ``mask_id`` position of caption n
    (answer_mask).  -> (rows int32 [N], counts int32 [N]: how many ``mask_id`` tokens caption n holds; 1 for answer_cls)."""
    _need_gpu(token_ids)
    ids = _c(token_ids.reshape(token_ids.shape[0], -1).long())
    N, L = ids.shape
    out = torch.empty(2, N, device=ids.device, dtype=torch.int32)
    check(_lib.lib().clv_qa_answer_rows(_ptr(ids), N, L, int(seq_len), int(base), int(bool(answer_mask)), int(mask_id),
                                        _ptr(out[0]), _ptr(out[1]), _stream()), 'clv_qa_answer_rows')
    return out[0], out[1]


_QA_F32 = {'clv_qa_head_fwd': 'clv_qa_head_f32_fwd', 'clv_qa_head_bwd': 'clv_qa_head_f32_bwd',
           'clv_attn_probs_mean': 'clv_attn_probs_mean_f32', 'clv_qa_choice_assemble': 'clv_qa_choice_assemble_f32',
           'clv_qa_choice_assemble_bwd': 'clv_qa_choice_assemble_f32_bwd'}


def _qa_entry(name, t, what):
    """(function, its name) of the QA entry point for activation ``t``: ``name`` on 16-bit storage outside parity mode,
    its fp32-storage instantiation (_QA_F32) on fp32 storage inside it.  A mismatch raises: a 16-bit
    activation inside parity mode means a producer rounded where it should not have, and an fp32 one outside it that a
    producer left the 16-bit path.  None of these ops is a rounding source of parity.ROUND_KINDS, so there is nothing to
    re-inject (parity.rnd) here: the head's logits are fp32 on the 16-bit path too, choice assembly is a copy, and the
    attention map is computed in fp32 from the stored q / k."""
    want = torch.float32 if parity.enabled() else BF16
    if t.dtype != want:
        where = 'in fp32 parity mode (CLOVER_PARITY)' if parity.enabled() else 'on the 16-bit path'
        raise NotImplementedError(f'{what} takes {want} activations {where}, got {t.dtype}')
    name = _QA_F32[name] if parity.enabled() else name
    return getattr(_lib.lib(), name), name


def _qa_grad_out(p):
    """(fp32 buffer the head's backward ADDS the gradient of p into, whether it is the engine's slab sink)."""
    sink = _sink(p)
    if sink is not None:
        return sink, True
    return torch.zeros(p.shape, device=p.device, dtype=torch.float32), False


class _QAHead(torch.autograd.Function):
    """QA_MC_head / QA_OE_Head (qa_head.py:8-85) on the rows ``rows`` of h [N, S, D]: dropout -> Linear(D, H) -> LayerNorm
    -> erf-GELU -> Linear(H, K) as clv_qa_head_fwd (1 launch for K = 1, 2 otherwise), optionally followed by the
    multiple-choice CrossEntropyLoss over groups of ``C`` rows (clv_qa_mc_ce_fwd, 1 launch).  Backward: one zero fill of
    d h, clv_qa_head_bwd (2 launches: d h scattered at the rows, the parameter gradients added into the engine's slab sinks
    or into fresh buffers)."""

    @staticmethod
    def forward(ctx, h, rows, w1, b1, gamma, beta, w2, b2, seed, drop_p, eps, labels, C):
        _need_gpu(h, rows)
        fwd, fwd_name = _qa_entry('clv_qa_head_fwd', h, 'the QA head')
        ctx.bwd = _qa_entry('clv_qa_head_bwd', h, 'the QA head')
        h = _c(h)
        D = h.shape[-1]
        H, K = w1.shape[0], w2.shape[0]
        M = rows.numel()
        if not _lib.lib().clv_qa_head_supported(D, H, K):
            raise RuntimeError(f'CLV_ERR_UNSUPPORTED: QA head D={D} H={H} K={K} (D <= 1024, H <= 512)')
        dev = h.device
        ws = [_c(t.detach().float()) for t in (w1, b1, gamma, beta, w2, b2)]
        zg = torch.empty(2, M, H, device=dev, dtype=torch.float32)
        stats = torch.empty(2, M, device=dev, dtype=torch.float32)
        logits = torch.empty(M, K, device=dev, dtype=torch.float32)
        L = _lib.lib()
        check(fwd(_ptr(h), _ptr(rows), *[_ptr(t) for t in ws], _ptr(seed), float(drop_p), float(eps), _ptr(zg[0]),
                  _ptr(zg[1]), _ptr(stats[0]), _ptr(stats[1]), _ptr(logits), M, D, H, K, _stream()), fwd_name)
        ctx.cfg = (h.shape, M, D, H, K, float(drop_p))
        ctx.params = (w1, b1, gamma, beta, w2, b2)
        if labels is None:
            ctx.save_for_backward(h, rows, zg, stats, seed, *ws)
            ctx.mc = False
            return logits
        B = M // C
        dprob = torch.empty(M, device=dev, dtype=torch.float32)
        out = torch.empty(2, device=dev, dtype=torch.float32)
        check(L.clv_qa_mc_ce_fwd(_ptr(logits), _ptr(_c(labels.reshape(-1).long())), _ptr(dprob), _ptr(out), B, C,
                                 _stream()), 'clv_qa_mc_ce_fwd')
        ctx.save_for_backward(h, rows, zg, stats, seed, *ws, dprob, out)
        ctx.mc = True
        return out[0]

    @staticmethod
    def backward(ctx, dout):
        shape, M, D, H, K, drop_p = ctx.cfg
        saved = ctx.saved_tensors
        h, rows, zg, stats, seed = saved[:5]
        w1, b1, gamma, beta, w2, b2 = saved[5:11]
        if ctx.mc:
            dprob, out = saved[11:]
            dl, s1, s2 = dprob, out[1:2], _c(dout.float().reshape(1))
        else:
            dl, s1, s2 = _c(dout.float()), None, None
        dev = h.device
        dh = torch.zeros(shape, device=dev, dtype=h.dtype)
        scratch = torch.empty(2, M, H, device=dev, dtype=torch.float32)
        outs = [_qa_grad_out(p) for p in ctx.params]
        bwd, bwd_name = ctx.bwd
        check(bwd(_ptr(h), _ptr(rows), _ptr(w1), _ptr(gamma), _ptr(beta), _ptr(w2), _ptr(zg[0]), _ptr(zg[1]),
                  _ptr(stats[0]), _ptr(stats[1]), _ptr(dl), _ptr(s1), _ptr(s2), _ptr(seed), drop_p, _ptr(scratch[0]),
                  _ptr(scratch[1]), _ptr(dh), *[_ptr(t) for t, _ in outs], M, D, H, K, _stream()), bwd_name)
        _delivered(*[p for p, (_, is_sink) in zip(ctx.params, outs) if is_sink])
        grads = [None if is_sink else t.to(p.dtype) for p, (t, is_sink) in zip(ctx.params, outs)]
        return (dh, None, *grads, None, None, None, None, None)


def qa_head(h, rows, w1, b1, gamma, beta, w2, b2, drop_p=0.0, eps=1e-5, labels=None, num_choices=None):
    """h [N, S, D] 16-bit (fp32 in parity mode: the same kernels in fp32 storage, d h returned in fp32), e.g. the fusion
    output, rows int32 [M] into h viewed as [N * S, D] -> logits fp32 [M, K]; with ``labels`` (multiple choice, K = 1): the
    CrossEntropyLoss of the logits viewed [M / num_choices, num_choices]."""
    seed = next_dropout_seed(h.device) if drop_p > 0 else None
    if labels is not None:
        assert w2.shape[0] == 1 and num_choices and rows.numel() % num_choices == 0
    return _QAHead.apply(h, rows, w1, b1, gamma, beta, w2, b2, seed, float(drop_p), float(eps), labels,
                         int(num_choices or 1))


def choice_assemble(visual, text, C):
    """visual 16-bit [B, n_vis, D] (fp32 in parity mode), text [B*C, L, D] -> the multiple-choice fusion input
    [B*C, n_vis + L, D] (one launch)."""
    _need_gpu(visual, text)
    if visual.dtype != text.dtype:
        raise TypeError(f'choice_assemble takes rows of one type, got {visual.dtype} / {text.dtype}')
    try:
        fn, name = _qa_entry('clv_qa_choice_assemble', visual, 'choice_assemble')
    except NotImplementedError as e:
        raise TypeError(str(e)) from None
    visual, text = _c(visual), _c(text)
    B, n_vis, D = visual.shape
    BC, L, _ = text.shape
    assert BC == B * C and text.shape[2] == D, (visual.shape, text.shape, C)
    feat = torch.empty(BC, n_vis + L, D, device=visual.device, dtype=visual.dtype)
    check(fn(_ptr(visual), _ptr(text), _ptr(feat), B, int(C), n_vis, L, D, _stream()), name)
    return feat


def choice_assemble_bwd(dfeat, cfg):
    """-> (d visual [B, n_vis, D]: the sum over the C candidates, d text [B*C, L, D]) (one launch)."""
    B, C, n_vis, L, D = cfg
    d = _c(dfeat.to(torch.float32 if parity.enabled() else BF16))
    fn, name = _qa_entry('clv_qa_choice_assemble_bwd', d, 'choice_assemble_bwd')
    dv = torch.empty(B, n_vis, D, device=d.device, dtype=d.dtype)
    dt = torch.empty(B * C, L, D, device=d.device, dtype=d.dtype)
    check(fn(_ptr(d), _ptr(dv), _ptr(dt), B, C, n_vis, L, D, _stream()), name)
    return dv, dt


def attn_probs_mean(qkv, kmask, num_heads):
    """forward_test's attention map: qkv 16-bit (fp32 in parity mode) [N, S, 3 C] of a BERT layer, kmask fp32 additive
    [N, S] (or None) -> fp32 [N, S, S] = softmax(q k^T / sqrt(hd) + kmask) averaged over the heads (inference only: no
    autograd)."""
    _need_gpu(qkv)
    fn, name = _qa_entry('clv_attn_probs_mean', qkv, 'attn_probs_mean')
    qkv = _c(qkv.detach())
    N, S, C3 = qkv.shape
    hd = C3 // 3 // num_heads
    out = torch.empty(N, S, S, device=qkv.device, dtype=torch.float32)
    km = _c(kmask.detach().float()) if kmask is not None else None
    check(fn(_ptr(qkv), _ptr(km), _ptr(out), N, S, num_heads, hd, float(hd) ** -0.5, _stream()), name)
    return out


def retrieval_rank(query, gallery, gt=None, topk=0, dual_softmax=None):
    """Retrieval ranks on the device (clv_retrieval_rank; accuracy.py:430-462 without the score matrix or the sort).
    query fp32 [Nq, D], gallery fp32 [Ng, D] (rows are normalised inside, all-zero rows stay zero), gt int [Nq] = each
    query's ground-truth gallery row (None: query i <-> row i) ->
    (rank int32 [Nq]: 0-based position of the ground truth in the stable descending order of the query's scores, -1 where
    gt < 0;  gt_score fp32 [Nq];  topk_idx int32 [Nq, topk] and topk_score fp32 [Nq, topk], or None, None with topk = 0).
    dual_softmax = T (a float >= 0): the order, gt_score and topk_score are those of the re-scored
    s'[i][j] = s[i][j] * softmax_i(T * s[i][j]) — the softmax over ALL queries of this call, per gallery row
    (clv_retrieval_col_stats, then clv_retrieval_rank_prior; O(Ng) extra memory).  None: the plain scores.
    Inference only: no autograd."""
    _need_gpu(query, gallery, gt)
    if query.dtype != torch.float32 or gallery.dtype != torch.float32:
        raise TypeError(f'retrieval_rank takes fp32 embeddings (got {query.dtype}, {gallery.dtype})')
    if query.dim() != 2 or gallery.dim() != 2 or query.shape[1] != gallery.shape[1]:
        raise ValueError(f'retrieval_rank: query [Nq, D] and gallery [Ng, D] (got {tuple(query.shape)}, {tuple(gallery.shape)})')
    q, g = query.detach(), gallery.detach()
    q = q if q.stride(1) == 1 or q.shape[1] == 1 else q.contiguous()
    g = g if g.stride(1) == 1 or g.shape[1] == 1 else g.contiguous()
    Nq, D = q.shape
    Ng, topk = g.shape[0], int(topk)
    if gt is not None:
        if gt.shape != (Nq,):
            raise ValueError(f'retrieval_rank: gt must be [{Nq}] (got {tuple(gt.shape)})')
        gt = _c(gt.detach().to(torch.int32))
    elif Nq > Ng:
        raise ValueError(f'retrieval_rank: without gt query i is matched with gallery row i, but Nq = {Nq} > Ng = {Ng}')
    L = _lib.lib()
    nbytes = L.clv_retrieval_work_bytes(Nq, Ng, D, topk)
    check(min(nbytes, 0), 'clv_retrieval_work_bytes')
    if dual_softmax is not None:                       # one area serves the statistics pass and then the rank pass
        sbytes = L.clv_retrieval_col_stats_work_bytes(Nq, Ng, D)
        check(min(sbytes, 0), 'clv_retrieval_col_stats_work_bytes')
        nbytes = max(nbytes, sbytes)
    dev = q.device
    work = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    rank = torch.empty(Nq, device=dev, dtype=torch.int32)
    gscore = torch.empty(Nq, device=dev, dtype=torch.float32)
    tidx = torch.empty(Nq, topk, device=dev, dtype=torch.int32) if topk else None
    tscore = torch.empty(Nq, topk, device=dev, dtype=torch.float32) if topk else None
    if dual_softmax is not None:
        T = float(dual_softmax)
        cmax = torch.empty(Ng, device=dev, dtype=torch.float32)
        csum = torch.empty(Ng, device=dev, dtype=torch.float32)
        ldq, ldg = max(q.stride(0), D), max(g.stride(0), D)
        check(L.clv_retrieval_col_stats(_ptr(q), _ptr(g), Nq, Ng, D, ldq, ldg, T, _ptr(cmax), _ptr(csum), _ptr(work),
                                        _stream()), 'clv_retrieval_col_stats')
        check(L.clv_retrieval_rank_prior(_ptr(q), _ptr(g), _ptr(gt), _ptr(rank), _ptr(gscore), _ptr(tidx), _ptr(tscore),
                                         _ptr(work), Nq, Ng, D, ldq, ldg, topk, _ptr(cmax), _ptr(csum), T, _stream()),
              'clv_retrieval_rank_prior')
        return rank, gscore, tidx, tscore
    check(L.clv_retrieval_rank(_ptr(q), _ptr(g), _ptr(gt), _ptr(rank), _ptr(gscore), _ptr(tidx), _ptr(tscore), _ptr(work),
                               Nq, Ng, D, max(q.stride(0), D), max(g.stride(0), D), topk, _stream()), 'clv_retrieval_rank')
    return rank, gscore, tidx, tscore


def retrieval_col_stats(query, gallery, T):
    """The column statistics of the dual-softmax prior (clv_retrieval_col_stats): for every gallery row j, over all
    queries, (col_max fp32 [Ng] = max_i T * s[i][j],  col_sum fp32 [Ng] = sum_i exp(T * s[i][j] - col_max[j])), s the
    scores retrieval_rank compares.  query fp32 [Nq, D], gallery fp32 [Ng, D], T a float >= 0.  Inference only."""
    _need_gpu(query, gallery)
    if query.dtype != torch.float32 or gallery.dtype != torch.float32:
        raise TypeError(f'retrieval_col_stats takes fp32 embeddings (got {query.dtype}, {gallery.dtype})')
    if query.dim() != 2 or gallery.dim() != 2 or query.shape[1] != gallery.shape[1]:
        raise ValueError(f'retrieval_col_stats: query [Nq, D] and gallery [Ng, D] (got {tuple(query.shape)}, '
                         f'{tuple(gallery.shape)})')
    q, g = query.detach(), gallery.detach()
    q = q if q.stride(1) == 1 or q.shape[1] == 1 else q.contiguous()
    g = g if g.stride(1) == 1 or g.shape[1] == 1 else g.contiguous()
    Nq, D = q.shape
    Ng = g.shape[0]
    L = _lib.lib()
    nbytes = L.clv_retrieval_col_stats_work_bytes(Nq, Ng, D)
    check(min(nbytes, 0), 'clv_retrieval_col_stats_work_bytes')
    work = torch.empty(nbytes, device=q.device, dtype=torch.uint8)
    cmax = torch.empty(Ng, device=q.device, dtype=torch.float32)
    csum = torch.empty(Ng, device=q.device, dtype=torch.float32)
    check(L.clv_retrieval_col_stats(_ptr(q), _ptr(g), Nq, Ng, D, max(q.stride(0), D), max(g.stride(0), D), float(T),
                                    _ptr(cmax), _ptr(csum), _ptr(work), _stream()), 'clv_retrieval_col_stats')
    return cmax, csum


def retrieval_group_best(query, gallery, lo=None, hi=None, want_rank=False, eps=0.0):
    """The best gallery row inside a per-query range (clv_retrieval_group_best; accuracy.py:396-427 without the score
    matrix).  query fp32 [Nq, D], gallery fp32 [Ng, D] (rows are scaled by 1 / max(norm, eps) inside; eps = 0: all-zero
    rows stay zero, as retrieval_rank), lo / hi int [Nq]: query i looks at gallery rows [lo[i], hi[i]) (both None: at the
    whole gallery) ->
    (best_idx int32 [Nq]: the first row of the range with the highest score, -1 where the range is empty or leaves the
    gallery;  best_score fp32 [Nq] (NaN there);  rank int32 [Nq] with want_rank, else None: the 0-based position of
    best_idx in the stable descending order of the query's scores over the WHOLE gallery).  Inference only: no autograd."""
    _need_gpu(query, gallery, lo, hi)
    if query.dtype != torch.float32 or gallery.dtype != torch.float32:
        raise TypeError(f'retrieval_group_best takes fp32 embeddings (got {query.dtype}, {gallery.dtype})')
    if query.dim() != 2 or gallery.dim() != 2 or query.shape[1] != gallery.shape[1]:
        raise ValueError(f'retrieval_group_best: query [Nq, D] and gallery [Ng, D] (got {tuple(query.shape)}, '
                         f'{tuple(gallery.shape)})')
    if (lo is None) != (hi is None):
        raise ValueError('retrieval_group_best: lo and hi come together')
    q, g = query.detach(), gallery.detach()
    q = q if q.stride(1) == 1 or q.shape[1] == 1 else q.contiguous()
    g = g if g.stride(1) == 1 or g.shape[1] == 1 else g.contiguous()
    Nq, D = q.shape
    Ng = g.shape[0]
    if lo is not None:
        if lo.shape != (Nq,) or hi.shape != (Nq,):
            raise ValueError(f'retrieval_group_best: lo and hi must be [{Nq}] (got {tuple(lo.shape)}, {tuple(hi.shape)})')
        lo, hi = _c(lo.detach().to(torch.int32)), _c(hi.detach().to(torch.int32))
    L = _lib.lib()
    nbytes = L.clv_retrieval_group_work_bytes(Nq, Ng, D)
    check(min(nbytes, 0), 'clv_retrieval_group_work_bytes')
    dev = q.device
    work = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    bidx = torch.empty(Nq, device=dev, dtype=torch.int32)
    bscore = torch.empty(Nq, device=dev, dtype=torch.float32)
    rank = torch.empty(Nq, device=dev, dtype=torch.int32) if want_rank else None
    check(L.clv_retrieval_group_best(_ptr(q), _ptr(g), _ptr(lo), _ptr(hi), _ptr(bidx), _ptr(bscore), _ptr(rank), _ptr(work),
                                     Nq, Ng, D, max(q.stride(0), D), max(g.stride(0), D), float(eps), _stream()),
          'clv_retrieval_group_best')
    return bidx, bscore, rank


# --------------------------------------------------------------------------- clip preparation (csrc/clip_prep.hip)
CLIP_REASONS = {1: 'CLV_CLIP_BAD_CHANNELS: the kernel reads 3-channel frames',
                2: 'CLV_CLIP_BAD_FRAME: the frame needs at least one pixel each way',
                3: 'CLV_CLIP_BAD_SIZE: the output size must be a multiple of 8 in [8, 2048]',
                4: 'CLV_CLIP_BAD_BOX: a crop box needs 1 <= right - left <= Ws and 1 <= bottom - top <= Hs'}
_CLIP_CONSTANTS = {}


def clip_prep_refusal(C_, Hs, Ws, S, box_w=1, box_h=1):
    """None when clv_clip_prep covers the shape (and a box of box_w x box_h), else the named reason.  The set is stated
    once, in clv_clip_prep_supported (host only: no GPU needed)."""
    rc = _lib.lib().clv_clip_prep_supported(int(C_), int(Hs), int(Ws), int(S), int(box_w), int(box_h))
    return None if rc == 0 else CLIP_REASONS.get(rc, str(rc))


def clip_prep_plan(B, T, Hs, Ws, S, half=False):
    """The launch of clv_clip_prep for a shape (clv_clip_prep_plan, host only) as a dict of the plan's fields."""
    g = _lib.ClvClipPrepGeom(B=B, T=T, Hs=Hs, Ws=Ws, C=3, S=S, out_dtype=int(half), pad=0, boxes_host=None)
    pl = _lib.ClvClipPrepPlan()
    check(_lib.lib().clv_clip_prep_plan(C.byref(g), C.byref(pl)), 'clv_clip_prep_plan')
    return {n: getattr(pl, n) for n, _ in pl._fields_}


def clip_prep_constants(mean, std, device):
    """(mean, inv_std) as fp32 [3] tensors on `device`: inv_std = 1 / float64(std) rounded to fp32, mmcv.imnormalize's
    `stdinv` (the reference multiplies by it: Normalize, augmentations.py:1563-1600).  Cached per (mean, std, device)."""
    key = (tuple(float(v) for v in mean), tuple(float(v) for v in std), _dev_key(device))
    if key not in _CLIP_CONSTANTS:
        if len(key[0]) != 3 or len(key[1]) != 3:
            raise ValueError('clip_prep: mean and std have one value per channel (3)')
        m = torch.tensor(key[0], dtype=torch.float64).to(torch.float32)
        s = (1.0 / torch.tensor(key[1], dtype=torch.float64)).to(torch.float32)
        _CLIP_CONSTANTS[key] = (m.to(device), s.to(device))
    return _CLIP_CONSTANTS[key]


def clip_prep(src_u8, boxes, flips, mean, std, out=None, size=224, dtype=None):
    """Decoded frames -> the normalised clip [B, 1, 3, T, size, size] in one launch (clv_clip_prep): per sample a crop box,
    a bilinear resize of the crop to size x size (half-pixel centres, neighbours clamped to the crop), an optional
    horizontal flip, (v - mean[c]) / std[c] and the NCTHW layout — the reference's RandomResizedCrop / CenterCrop, Resize,
    Flip, Normalize and FormatShape.

    src_u8 uint8 [B, T, Hs, Ws, 3] on the device, channel order as stored; boxes int [B, 4] (left, top, right, bottom;
    right / bottom exclusive) ON THE HOST (array or CPU tensor: checked here, then uploaded — a device tensor is copied
    back first, which synchronises); flips [B] (host or device, non-zero = mirror); mean / std 3 numbers each.
    With `out` given ([B, 1, 3, T, size, size], fp32 or the 16-bit element type, contiguous) the clip is written in
    place — a captured engine's static `imgs` buffer goes here; otherwise a new tensor of `dtype` (default fp32).
    No autograd: inputs carry no gradient.  A box outside the frame raises ValueError before any launch; a shape or box
    extent outside the kernel's set raises NotImplementedError with the named reason of clv_clip_prep_supported."""
    _need_gpu(src_u8, out)
    if src_u8.dtype != torch.uint8 or src_u8.dim() != 5:
        raise TypeError(f'clip_prep: src is uint8 [B, T, Hs, Ws, 3] (got {src_u8.dtype} {tuple(src_u8.shape)})')
    B, T, Hs, Ws, Cin = src_u8.shape
    if out is not None:
        size, dtype = out.shape[-1], out.dtype
    dtype = torch.float32 if dtype is None else dtype
    S = int(size)
    why = clip_prep_refusal(Cin, Hs, Ws, S)
    if why is not None:
        raise NotImplementedError(f'clip_prep: {why}')
    if dtype not in (torch.float32, BF16):
        raise TypeError(f'clip_prep: the output is fp32 or {BF16} (got {dtype})')
    hb = torch.as_tensor(boxes).detach().cpu().to(torch.int32).contiguous()
    if hb.shape != (B, 4):
        raise ValueError(f'clip_prep: boxes must be [{B}, 4] (got {tuple(hb.shape)})')
    for b, (l, t, r, bt) in enumerate(hb.tolist()):
        if l < 0 or t < 0 or r > Ws or bt > Hs:
            raise ValueError(f'clip_prep: box {b} = {(l, t, r, bt)} leaves the {Hs} x {Ws} frame')
        why = clip_prep_refusal(Cin, Hs, Ws, S, r - l, bt - t)
        if why is not None:
            raise NotImplementedError(f'clip_prep: box {b} = {(l, t, r, bt)}: {why}')
    dev = src_u8.device
    fl = torch.as_tensor(flips)
    if fl.shape != (B,):
        raise ValueError(f'clip_prep: flips must be [{B}] (got {tuple(fl.shape)})')
    fl = _c((fl != 0).to(torch.uint8).to(dev, non_blocking=True))
    db = hb.to(dev, non_blocking=True)
    mean_d, inv_std_d = clip_prep_constants(mean, std, dev)
    if out is None:
        out = torch.empty(B, 1, 3, T, S, S, device=dev, dtype=dtype)
    elif tuple(out.shape) != (B, 1, 3, T, S, S) or not out.is_contiguous():
        raise ValueError(f'clip_prep: out must be contiguous [{B}, 1, 3, {T}, {S}, {S}] (got {tuple(out.shape)})')
    g = _lib.ClvClipPrepGeom(B=B, T=T, Hs=Hs, Ws=Ws, C=Cin, S=S, out_dtype=int(dtype != torch.float32), pad=0,
                             boxes_host=hb.data_ptr())
    check(_lib.lib().clv_clip_prep(_ptr(_c(src_u8)), _ptr(db), _ptr(fl), _ptr(mean_d), _ptr(inv_std_d), _ptr(out),
                                   C.byref(g), _stream()), 'clv_clip_prep')
    return out
