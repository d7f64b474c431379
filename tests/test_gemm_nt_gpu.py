"""Every launch class of csrc/gemm_nt.hip through the C entries, bit-exact on integer data.

The four one-kernel classes of gemm_nt_kernel (128 x 128, 64 x 128, 128 x 192, 64 x 192), the two wave-specialised classes of
gemm_ws_kernel, with and without K slices, gemm_nt_kernel<PARTIAL>, splitk_reduce_kernel, the rotated K walk and
clv_gemm_nt_fp8 run on the inputs of tests/gemm_ref.py, whose caps make fp32 accumulation independent of its order: c, the
pre-activation c2 and the MUL epilogue are compared bit for bit with the fp64 result converted once to the 16-bit type, the
values behind GELU / GELU' within the allowances of NORM_ACT_ERROR_BUDGET.md.  Every case first asserts, through
clv_gemm_nt_plan, the launch it was written for (gemm_ref.CASES): a retuned planner fails the claim instead of moving the case
to another kernel.

Buffers: operands are column slices (lda, ldb != K) of wider NaN-filled tensors with NaN rows after M / N; c, c2 and aux share
an ldc > N (aux is padded with ones: a store past an edge that multiplied by it would otherwise put NaN on NaN), the padding columns and TAIL_ROWS rows after M of c / c2 are NaN and must stay NaN; `work` is NaN with a NaN tail
of three slabs, and after a sliced launch its slabs must add up to the exact a b^T.  A read past an edge or a write past a
buffer shows in the comparison instead of in somebody else's memory.

One random-data case per kernel class holds the kernels to two bounds that are not fitted to them (test_random_data); measured
ratios: tests/GEMM_ERROR_BUDGET.md (GEMM_BUDGET lines under `pytest -s`)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_ref as gr                      # noqa: E402
import norm_ref as nr                      # noqa: E402
from clover_amd import _lib                # noqa: E402

DEV = 'cuda'
HALF = _lib.half_dtype()
NAN = float('nan')
GUARD_ROWS = 128                           # operand rows past M / N: a whole tile of rows
TAIL_ROWS = 128                            # NaN rows after M in c / c2: a whole tile of rows
ERR_ARG, ERR_UNSUPPORTED = -1, -2
EPI_WITH_C2 = (gr.EPI_GELU, gr.EPI_GELUD)
GELU_DATA = (gr.EPI_GELU, gr.EPI_GELUD, gr.EPI_DGELU)


def L():
    return _lib.lib()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ----------------------------------------------------------------------------- guarded buffers
class Operand:
    """A read-only matrix [R][W] as a column slice of a wider `fill`-filled tensor with GUARD_ROWS `fill` rows after it."""

    def __init__(self, t, pad=16, off=8, fill=NAN):
        R, W = t.shape
        self.buf = torch.full((R + GUARD_ROWS, W + pad), fill, dtype=t.dtype, device=DEV)
        self.view = self.buf[:R, off:off + W]
        self.view.copy_(t)
        self.before = self.buf.clone()
        self.ld = W + pad

    def ptr(self):
        return C.c_void_p(self.view.data_ptr())

    def check(self, what):
        n = self.buf.element_size()
        it = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[n]
        assert torch.equal(self.buf.view(it), self.before.view(it)), f'{what}: an operand was written'


class Out16:
    """A 16-bit output [M][N] inside a NaN-filled [M + TAIL_ROWS][ldc]."""

    def __init__(self, M, N, ldc):
        self.M, self.N = M, N
        self.buf = torch.full((M + TAIL_ROWS, ldc), NAN, dtype=HALF, device=DEV)
        self.view = self.buf[:M, :N]

    def ptr(self):
        return C.c_void_p(self.buf.data_ptr())

    def check(self, what):
        assert torch.isnan(self.buf[:self.M, self.N:]).all(), f'{what}: padding columns [N, ldc) written'
        assert torch.isnan(self.buf[self.M:]).all(), f'{what}: rows past M written'


class Vec:
    """fp32 vector / work buffer of n floats followed by a tail (NaN for what a kernel writes; 1 for bias and scales: with a NaN
    there, a store past N or M that went with the read past it would put NaN on NaN and stay unseen)."""

    def __init__(self, n, fill, tail=4096, tail_fill=NAN):
        self.n = n
        self.buf = torch.full((n + tail,), tail_fill, dtype=torch.float32, device=DEV)
        if isinstance(fill, torch.Tensor):
            self.buf[:n].copy_(fill.reshape(-1))
        else:
            self.buf[:n].fill_(fill)
        self.t = self.buf[:n]
        self.before = self.buf.clone()

    def ptr(self):
        return C.c_void_p(self.buf.data_ptr())

    def check_tail(self, what):
        assert torch.isnan(self.buf[self.n:]).all(), f'{what}: written past its end'

    def check_unchanged(self, what):
        assert torch.equal(self.buf.view(torch.int32), self.before.view(torch.int32)), f'{what}: written'


def same(got, want64, what):
    """bit-exact: a 16-bit device tensor against the fp64 expectation converted once to the 16-bit type"""
    w = want64.to(HALF)
    if not torch.equal(got, w):
        bad = (got != w) | torch.isnan(got)
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact reference '
                             f'({int(torch.isnan(got).sum())} NaN), first at {idx}: got {got[tuple(idx)].item()}, '
                             f'exact {want64[tuple(idx)].item()}')


def within(got, want64, allow, what):
    g = got.double()
    assert torch.isfinite(g).all(), f'{what}: non-finite values'
    over = (g - want64).abs() - allow
    if (over > 0).any():
        idx = over.argmax().item()
        m, n = divmod(idx, got.shape[1])
        raise AssertionError(f'{what}: {int((over > 0).sum())} elements over the allowance, worst at ({m}, {n}): got '
                             f'{g[m, n].item()}, reference {want64[m, n].item()}, allowed {allow[m, n].item():.3e}')


# ----------------------------------------------------------------------------- one launch, checked
def launch(spec, epi, a_, b_, bias_, aux_, ldc_pad=24, work_short=False, expect_plan=None):
    """clv_gemm_nt_ex on guarded buffers under the spec's environment -> (c Out16, c2 Out16 or None, work Vec, splitk)."""
    M, N, K = spec.M, spec.N, spec.K
    a, b = Operand(a_, 16, 8), Operand(b_, 24, 16)
    ldc = N + ldc_pad
    c = Out16(M, N, ldc)
    c2 = Out16(M, N, ldc) if epi in EPI_WITH_C2 else None
    aux = None
    if epi in (gr.EPI_DGELU, gr.EPI_MUL):
        aux = Operand(aux_, ldc_pad, 0, fill=1.0)      # finite: a store past M / N that multiplied by it must not be NaN on NaN
        assert aux.ld == ldc
    bias = Vec(N, bias_, tail=64, tail_fill=1.0) if epi in (gr.EPI_BIAS, gr.EPI_GELU, gr.EPI_GELUD) else None
    with gr.env(spec.force, spec.rot):
        pl = gr.plan(M, N, K, with_work=not work_short)
        assert pl == (expect_plan or spec.claim), f'{pl} (claimed {expect_plan or spec.claim})'
        wb = L().clv_gemm_nt_work_bytes(M, N, K)
        slab = M * N
        work = Vec(wb // 4, NAN, tail=3 * slab + 4096) if wb else Vec(0, NAN, tail=4096)
        rc = L().clv_gemm_nt_ex(a.ptr(), b.ptr(), bias.ptr() if bias else None, aux.ptr() if aux else None, c.ptr(),
                                c2.ptr() if c2 else None, M, N, K, a.ld, b.ld, ldc, epi, work.ptr(),
                                wb - 1 if work_short else (wb if wb else 4096 * 4), stream())
    torch.cuda.synchronize()
    assert rc == 0, f'clv_gemm_nt_ex = {rc}'
    what = f'{M}x{N}x{K} {gr.EPI_NAMES[epi]}'
    for o in (a, b) + ((aux,) if aux else ()):
        o.check(what)
    if bias:
        bias.check_unchanged(what + ' bias')
    for o in (c,) + ((c2,) if c2 else ()):
        o.check(what)
    return c, c2, work, pl.splitk


def check_work(work, splitk, spec, acc, what):
    if splitk == 1:
        assert torch.isnan(work.buf).all(), f'{what}: a one-pass launch wrote to the work buffer'
        return
    slabs = work.t.view(splitk, spec.M, spec.N)
    assert torch.isfinite(slabs).all(), f'{what}: a slab element was not written'
    assert torch.equal(slabs.double().sum(0), acc), f'{what}: the fp32 slabs do not add up to the exact a b^T'
    assert torch.equal(slabs.sum(0).double(), acc)
    work.check_tail(f'{what}: work (past {splitk} slabs)')


def run_exact(name, epi, work_short=False, expect_plan=None):
    spec = gr.assert_plan(name)
    # the GELU data (pre-activations within 16, shapes checked by tests/test_gemm_ref_cpu.py) on the all-epilogue cases; DGELU
    # elsewhere takes the integer data, whose aux in {0, +-1/2, +-1, +-2} goes through GELU' all the same
    case = gr.exact_case(spec.M, spec.N, spec.K, gelu=epi in GELU_DATA and name in gr.ALL_EPI, device=DEV)
    c, c2, work, splitk = launch(spec, epi, case.a, case.b, case.bias, case.aux, work_short=work_short, expect_plan=expect_plan)
    what = f'{name} {spec.M}x{spec.N}x{spec.K} {gr.EPI_NAMES[epi]}'
    bias, aux = case.bias.double().to(DEV), case.aux.double().to(DEV)
    want, want2 = gr.expected(epi, case.acc, bias, aux)
    al, al2 = gr.allowance(epi, case.acc, bias, aux)
    if al is None:
        same(c.view, want, what + ': c')
    else:
        within(c.view, want, al, what + ': c')
    if c2 is not None:
        if al2 is None:
            same(c2.view, want2, what + ': c2')
        else:
            within(c2.view, want2, al2, what + ': c2')
    check_work(work, splitk, spec, case.acc, what)
    return c, c2


# ----------------------------------------------------------------------------- the case table
@pytest.mark.parametrize('epi', range(6), ids=gr.EPI_NAMES)
@pytest.mark.parametrize('name', gr.ALL_EPI)
def test_every_epilogue(name, epi):
    """All six epilogues on one case per kernel class and once through the reduce kernel."""
    run_exact(name, epi)


_REST = [n for n in gr.CASES if n not in gr.ALL_EPI]


@pytest.mark.parametrize('name', _REST)
def test_case_bias(name):
    run_exact(name, gr.EPI_BIAS)


@pytest.mark.parametrize('name,epi', [(n, (gr.EPI_MUL, gr.EPI_DGELU)[i % 2]) for i, n in enumerate(_REST)],
                         ids=[f'{n}-{("MUL", "DGELU")[i % 2]}' for i, n in enumerate(_REST)])
def test_case_aux(name, epi):
    """MUL / DGELU in turn: aux read with ldc on every remaining case."""
    run_exact(name, epi)


@pytest.mark.parametrize('name', ['nt128-second-tile-1-stage', 'nt192-one-second-tile-1-stage', 'ws128-second-tile',
                                  'ws64-4-slices-second-unit'])
def test_launched_twice(name):
    """The same launch again on fresh buffers: nothing may be left in a ring or a slab."""
    for _ in range(2):
        run_exact(name, gr.EPI_NONE)


@pytest.mark.parametrize('rot', list(gr.ROT_PAIRS))
@pytest.mark.parametrize('epi', [gr.EPI_NONE, gr.EPI_BIAS], ids=['NONE', 'BIAS'])
def test_rotation(rot, epi):
    """CLV_GEMM_ROT=1 on the three routes that take it: the plan says rot = 1, and on integer data the result equals the
    unrotated one (and the exact one) bit for bit."""
    assert gr.CASES[rot].claim.rot == 1
    c_rot, _ = run_exact(rot, epi)
    c_plain, _ = run_exact(gr.ROT_PAIRS[rot], epi)
    assert torch.equal(c_rot.view.view(torch.int16), c_plain.view.view(torch.int16))


def test_short_work_buffer_runs_in_one_pass():
    """work_bytes one byte short: the call must run as without a work buffer and leave `work` alone."""
    spec = gr.CASES['ws64-4-slices']
    with gr.env():
        one_pass = gr.plan(spec.M, spec.N, spec.K, with_work=False)
    assert one_pass.splitk == 1 and one_pass.kernel == 2 and spec.claim.splitk == 4
    spec = gr.assert_plan('ws64-4-slices')
    case = gr.exact_case(spec.M, spec.N, spec.K, device=DEV)
    c, _, work, _ = launch(spec, gr.EPI_BIAS, case.a, case.b, case.bias, case.aux, work_short=True, expect_plan=one_pass)
    same(c.view, gr.expected(gr.EPI_BIAS, case.acc, case.bias.double().to(DEV), None)[0], 'short work buffer: c')
    assert torch.isnan(work.buf).all(), 'a launch whose work buffer is too small wrote to it'


# ----------------------------------------------------------------------------- the bias is rounded to 16 bits
@pytest.mark.parametrize('name', ['nt128-two-row-blocks', 'nt128-pc8-global-bias', 'nt64-over-ws-limit', 'ws64-one-row',
                                  'ws128-ragged', 'ws64-2-slices-one-row', 'forced-nt-partial'])
def test_bias_is_rounded_to_16_bits(name):
    """LDS path, global-memory path, both wave-specialised classes and the reduce kernel: c = round16(acc + round16(bias)).
    The bias values are not 16-bit values; every fourth column has acc = 1 and a bias that sits just above half a 16-bit
    spacing at 1: added unrounded the sum rounds UP to the next 16-bit value, rounded first it is a tie and goes to 1."""
    spec = gr.assert_plan(name)
    M, N, K = spec.M, spec.N, spec.K
    g = torch.Generator().manual_seed(N)
    a = gr._tern(g, 0.5, M, K)
    b = gr._tern(g, 0.5, N, K)
    a[:, 0] = 1
    b[::4] = 0
    b[::4, 0] = 1
    bias = torch.randn(N, generator=g)
    bias = bias + torch.sign(bias) * 0.5                       # |bias| >= 1/2: acc + round16(bias) stays exact in fp32
    mant = 10 if HALF == torch.float16 else 7
    bias[::4] = 2.0 ** -(mant + 1) + 2.0 ** -(mant + 13)
    b16 = bias.to(HALF).double()
    assert (b16 != bias.double()).sum() > N // 2 and torch.equal(b16[::4], torch.full_like(b16[::4], 2.0 ** -(mant + 1)))
    acc = gr.acc64(a, b, DEV)
    assert acc.abs().max() <= 128 and torch.equal(acc[:, ::4], torch.ones_like(acc[:, ::4]))
    want = acc + b16.to(DEV)
    assert torch.equal(want.float().double(), want)            # the fp32 addition is exact: one rounding, to 16 bits
    unrounded = (acc + bias.double().to(DEV)).to(HALF)
    assert (unrounded != want.to(HALF)).float().mean() >= 0.25  # (what a kernel without the rounding would store)
    c, _, _, _ = launch(spec, gr.EPI_BIAS, a.to(HALF), b.to(HALF), bias, None)
    same(c.view, want, f'{name}: c')


# ----------------------------------------------------------------------------- argument checks (no launch)
def test_argument_checks():
    t = torch.zeros(1 << 16, dtype=HALF, device=DEV)
    f = torch.zeros(4096, dtype=torch.float32, device=DEV)
    p, pf = t.data_ptr(), f.data_ptr()
    v = C.c_void_p

    def call(M=128, N=64, K=64, lda=64, ldb=64, ldc=64, epi=gr.EPI_NONE, a=p, b=p, bias=None, aux=None, c=p + 65536, c2=None):
        return L().clv_gemm_nt_ex(v(a), v(b), v(bias) if bias else None, v(aux) if aux else None, v(c), v(c2) if c2 else None, M,
                                  N, K, lda, ldb, ldc, epi, None, 0, stream())
    assert call() == 0
    assert call(N=68, ldc=72) == ERR_UNSUPPORTED               # N % 8
    assert call(K=96, lda=96, ldb=96) == ERR_UNSUPPORTED       # K % 64
    assert call(N=56) == ERR_UNSUPPORTED                       # N < 64
    for kw in (dict(a=p + 2), dict(b=p + 8), dict(c=p + 65540), dict(epi=gr.EPI_BIAS, bias=pf + 4), dict(epi=gr.EPI_MUL, aux=p + 2),
               dict(epi=gr.EPI_GELU, bias=pf, c2=p + 6)):
        assert call(**kw) == ERR_ARG, kw                       # misaligned pointers
    for kw in (dict(lda=56), dict(ldb=56), dict(ldc=56), dict(lda=68), dict(ldc=68)):
        assert call(**kw) == ERR_ARG, kw                       # ld below the width, or not a multiple of 8
    for epi in (gr.EPI_BIAS, gr.EPI_GELU, gr.EPI_GELUD):
        assert call(epi=epi, c2=p) == ERR_ARG                  # no bias
    for epi in (gr.EPI_GELU, gr.EPI_GELUD):
        assert call(epi=epi, bias=pf) == ERR_ARG               # no c2
    for epi in (gr.EPI_DGELU, gr.EPI_MUL):
        assert call(epi=epi) == ERR_ARG                        # no aux
    assert call(epi=6) == ERR_UNSUPPORTED and call(epi=-1) == ERR_UNSUPPORTED
    assert call(M=0) == ERR_ARG and call(a=None) == ERR_ARG
    torch.cuda.synchronize()
    assert not t.any()


# ----------------------------------------------------------------------------- clv_gemm_nt_fp8
@pytest.mark.parametrize('epi', [gr.EPI_NONE, gr.EPI_BIAS, gr.EPI_GELUD], ids=['NONE', 'BIAS', 'BIAS_GELU_D'])
@pytest.mark.parametrize('M,N,K', gr.FP8_SHAPES)
def test_fp8(M, N, K, epi):
    """e4m3 bytes of {-1, 0, 1}, power-of-two row scales: acc * sa * sb (+ bias) is exact in fp32 and in 16 bits.  The tile
    class (64 x 128 for K >= 1024 bytes) has no host entry: gr.fp8_class is a copy of the rule."""
    assert gr.fp8_class(M, N, K) == (64 if K >= 1024 else 128)
    a_, b_, sa_, sb_, bias_, pre = gr.fp8_case(M, N, K, device=DEV)
    a, b = Operand(gr.e4m3(a_), 16, 16, fill=0x7f), Operand(gr.e4m3(b_), 32, 16, fill=0x7f)     # 0x7f: e4m3 NaN
    sa, sb, bias = (Vec(M, sa_, tail=GUARD_ROWS, tail_fill=1.0), Vec(N, sb_, tail=64, tail_fill=1.0),
                    Vec(N, bias_, tail=64, tail_fill=1.0))
    ldc = N + 24
    c, c2 = Out16(M, N, ldc), (Out16(M, N, ldc) if epi == gr.EPI_GELUD else None)
    rc = L().clv_gemm_nt_fp8(a.ptr(), b.ptr(), sa.ptr(), sb.ptr(), bias.ptr() if epi else None, c.ptr(),
                             c2.ptr() if c2 else None, M, N, K, a.ld, b.ld, ldc, epi, stream())
    torch.cuda.synchronize()
    assert rc == 0
    what = f'fp8 {M}x{N}x{K} {gr.EPI_NAMES[epi]}'
    bd = bias_.double().to(DEV)
    if epi == gr.EPI_NONE:
        same(c.view, pre - bd, what)
    elif epi == gr.EPI_BIAS:
        same(c.view, pre, what)
    else:
        within(c.view, nr.gelu64(pre), nr.spacing16(nr.gelu64(pre), HALF) + gr.GELU_TERM * pre.abs(), what + ': c')
        within(c2.view, nr.gelu_grad64(pre), nr.spacing16(nr.gelu_grad64(pre), HALF) + gr.GELU_GRAD_TERM * (1 + pre.abs()),
               what + ': c2')
    for o in (a, b):
        o.check(what)
    for o in (sa, sb, bias):
        o.check_unchanged(what)
    for o in (c,) + ((c2,) if c2 else ()):
        o.check(what)


def test_fp8_argument_checks():
    t = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    f = torch.zeros(4096, dtype=torch.float32, device=DEV)
    p, pf, v = t.data_ptr(), f.data_ptr(), C.c_void_p

    def call(M=64, N=64, K=128, lda=128, ldb=128, ldc=64, epi=gr.EPI_NONE, a=p, bias=None, c2=None):
        return L().clv_gemm_nt_fp8(v(a), v(p), v(pf), v(pf), v(bias) if bias else None, v(p + 32768), v(c2) if c2 else None, M, N, K,
                                   lda, ldb, ldc, epi, stream())
    assert call() == 0
    assert call(K=64, lda=64, ldb=64) == ERR_UNSUPPORTED and call(N=68, ldc=72) == ERR_UNSUPPORTED and call(N=56) == ERR_UNSUPPORTED
    assert call(a=p + 8) == ERR_ARG and call(lda=120) == ERR_ARG and call(lda=136) == ERR_ARG and call(ldc=56) == ERR_ARG
    assert call(epi=gr.EPI_BIAS) == ERR_ARG and call(epi=gr.EPI_GELUD, bias=pf) == ERR_ARG
    assert call(epi=gr.EPI_GELU, bias=pf, c2=p) == ERR_UNSUPPORTED
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- ops level
def test_ops_gemm_nt_into_a_column_slice():
    """ops.gemm_nt(..., out = a column slice) leaves the neighbouring columns alone, and the c2 it allocates for the GELU
    epilogues has the row stride the kernel addresses it with."""
    from clover_amd import ops
    spec = gr.CASES['nt128-two-row-blocks']
    M, N, K = spec.M, spec.N, spec.K
    case = gr.exact_case(M, N, K, gelu=True, device=DEV)
    a, b, bias = case.a.to(DEV), case.b.to(DEV), case.bias.to(DEV)
    pre = case.acc + case.bias.double().to(DEV)
    wide = torch.full((M + TAIL_ROWS, N + 32), NAN, dtype=HALF, device=DEV)
    out = wide[:M, 16:16 + N]
    assert ops.gemm_nt(a, b, bias, epilogue=ops.GEMM_EPI_BIAS, out=out) is out
    torch.cuda.synchronize()
    same(out, pre, 'ops.gemm_nt into a column slice')
    assert torch.isnan(wide[:, :16]).all() and torch.isnan(wide[:, 16 + N:]).all() and torch.isnan(wide[M:]).all()
    wide.fill_(NAN)
    act, c2 = ops.gemm_nt(a, b, bias, epilogue=ops.GEMM_EPI_BIAS_GELU, out=out)
    torch.cuda.synchronize()
    assert act is out and c2.shape == (M, N) and c2.stride() == out.stride()
    same(c2, pre, 'ops.gemm_nt into a column slice: c2')
    within(act, nr.gelu64(pre), nr.spacing16(nr.gelu64(pre), HALF) + gr.GELU_TERM * pre.abs(), 'ops.gemm_nt: GELU')
    assert torch.isnan(wide[:, :16]).all() and torch.isnan(wide[:, 16 + N:]).all() and torch.isnan(wide[M:]).all()


# ----------------------------------------------------------------------------- random data: two bounds, neither fitted
@pytest.mark.parametrize('epi', [gr.EPI_BIAS, gr.EPI_MUL, gr.EPI_DGELU], ids=['BIAS', 'MUL', 'DGELU'])
@pytest.mark.parametrize('name', gr.RANDOM)
def test_random_data(name, epi):
    """Gaussian operands against the fp64 reference (the device's fp64 matmul: independent of these kernels).
    Per element: |err| <= spacing16(ref) + (K + splitk + 2) 2^-23 (|a||b|^T + |bias|), the summation bound for ANY order plus
    one 16-bit rounding; for MUL / DGELU the second term times |aux| / |g'(aux)|, plus the GELU' allowance times |acc|.
    Per tensor: max |err| <= one 16-bit spacing at max |ref|."""
    spec = gr.assert_plan(name)
    M, N, K = spec.M, spec.N, spec.K
    a_, b_, bias_, aux_ = gr.gauss_case(M, N, K)
    c, _, work, splitk = launch(spec, epi, a_, b_, bias_, aux_)
    acc = gr.acc64(a_, b_, DEV)
    absdot = a_.to(DEV).double().abs() @ b_.to(DEV).double().abs().t()
    bias, aux = bias_.double().to(DEV), aux_.double().to(DEV)
    ref, _ = gr.expected(epi, acc, bias, aux)
    summ = (K + splitk + 2) * gr.U * (absdot + (bias.abs() if epi == gr.EPI_BIAS else 0))
    if epi == gr.EPI_MUL:
        summ = summ * aux.abs()
    elif epi == gr.EPI_DGELU:
        g = nr.gelu_grad64(aux)
        summ = summ * g.abs() + (nr.spacing16(g, HALF) + gr.GELU_GRAD_TERM * (1 + aux.abs())) * acc.abs()
    bound = nr.spacing16(ref, HALF) + summ
    got = c.view.double()
    assert torch.isfinite(got).all()
    err = (got - ref).abs()
    elem = (err / bound).max().item()
    top = ref.abs().max()
    tens = (err.max() / nr.spacing16(top, HALF)).item()
    print(f'GEMM_BUDGET | {name} {M}x{N}x{K} splitk {splitk} | {gr.EPI_NAMES[epi]} | per element {elem:.3f} of the bound | '
          f'max error {tens:.3f} of a spacing at max|ref| = {top.item():.3f}')
    assert elem <= 1, f'{name}: an element is off by {elem:.3f} x its bound'
    assert tens <= 1, f'{name}: max error is {tens:.3f} spacings at max|ref|'
    if splitk > 1:
        work.check_tail(name)
    else:
        assert torch.isnan(work.buf).all()
