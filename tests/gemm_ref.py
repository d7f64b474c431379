"""References, input generators and planning claims for the tests of csrc/gemm_nt.hip (tests/test_gemm_ref_cpu.py,
tests/test_gemm_nt_gpu.py).  Plain torch; the only library calls are the HOST entries clv_gemm_nt_plan / _work_bytes.

    acc[m][n] = sum_k a[m][k] b[n][k]          c = epilogue(acc, bias, aux)

Exactness.  The exact generators produce operands in {-1, 0, 1} (GELU cases: b in {-1/8, 0, 1/8}), a bias of integers in
[-8, 8] (GELU cases: multiples of 1/16 in [-2, 2]) and aux in {0, +-1/2, +-1, +-2}.  With q the common unit (1, or 1/16) they
assert, on the inputs and the fp64 reference alone,
    (max |a| |b|^T + |bias|) / q < 2^24    every partial sum, in any order and any grouping (MFMA blocks, K slices, the reduce
                                           kernel), is a multiple of q below 2^24 q: exact in fp32, so is every fp32 addition
    max |acc + bias| <= 256 q              every such multiple of q is a value of bf16 (8 significant bits) and of fp16: one
                                           dropped or doubled product changes the STORED result
and pick the largest density of non-zeros among 2/3, 1/2, 1/3, 1/4 for which both hold.  These are caps on the inputs, not
tolerances.  The expected c (and c2 of BIAS_GELU, and MUL) is then the fp64 result converted ONCE to the 16-bit type and is
compared bit for bit; the values that pass through GELU / GELU' get the allowances of tests/NORM_ACT_ERROR_BUDGET.md.

Claims.  Every case names the launch it was written for as a literal ClvGemmPlan; assert_plan compares it with what the
library's host entry says, so a retuned planner fails the claim instead of moving the case to another kernel.  The tile class
of clv_gemm_nt_fp8 has no host entry: fp8_class() is a hand-written COPY of its two-line rule (see GEMM_ERROR_BUDGET.md).
"""
import functools
import os
from contextlib import contextmanager
from typing import NamedTuple, Optional

import torch

import norm_ref as nr
from clover_amd import _lib

HALF = _lib.half_dtype()
CAP = 1 << 24
TOP = 256                       # max |acc + bias| in units of q: integers up to 2^8 are bf16 values (fp16: 2^11)
DENSITIES = (2 / 3, 1 / 2, 1 / 3, 1 / 4)
EPI_NONE, EPI_BIAS, EPI_GELU, EPI_DGELU, EPI_GELUD, EPI_MUL = range(6)
EPI_NAMES = ('NONE', 'BIAS', 'BIAS_GELU', 'DGELU', 'BIAS_GELU_D', 'MUL')
GELU_TERM, GELU_GRAD_TERM = 3e-7, 3e-7      # NORM_ACT_ERROR_BUDGET.md: + 3e-7 |x|, + 3e-7 (1 + |x|)
U = 2.0 ** -23                  # unit roundoff of the summation bound (WGRAD_ERROR_BUDGET.md: rounding mode of the MFMA unverified)


# ----------------------------------------------------------------------------------------------- planning claims
class Plan(NamedTuple):
    kernel: int                 # 0 gemm_nt_kernel, 1 gemm_ws_kernel 128 x 128, 2 gemm_ws_kernel 64 x 128
    BM: int
    BN: int
    waves: int
    ring: int
    splitk: int
    rot: int
    pc: int
    grid: int
    units: int                  # units_max_xcd
    slots: int                  # slots_xcd
    bias_lds: int


@contextmanager
def env(splitk=None, rot=None):
    """CLV_GEMM_SPLITK / CLV_GEMM_ROT for the calls inside (the library reads both per call), restored afterwards."""
    old = {k: os.environ.get(k) for k in ('CLV_GEMM_SPLITK', 'CLV_GEMM_ROT')}
    try:
        for k, v in (('CLV_GEMM_SPLITK', splitk), ('CLV_GEMM_ROT', rot)):
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def plan(M, N, K, with_work=True):
    """clv_gemm_nt_plan under the current environment -> Plan"""
    p = _lib.ClvGemmPlan()
    rc = _lib.lib().clv_gemm_nt_plan(M, N, K, int(with_work), p)
    assert rc == 0, f'clv_gemm_nt_plan({M}, {N}, {K}) = {rc}'
    return Plan(p.kernel, p.BM, p.BN, p.waves, p.ring, p.splitk, p.rot, p.pc, p.grid, p.units_max_xcd, p.slots_xcd, p.bias_in_lds)


class Spec(NamedTuple):
    M: int
    N: int
    K: int
    claim: Plan
    force: Optional[int] = None     # CLV_GEMM_SPLITK for the launch (None: unset, the planner's own choice)
    rot: Optional[int] = None       # CLV_GEMM_ROT
    note: str = ''


def _nt(BM, BN, waves, ring, pc, units, slots, splitk=1, rot=0, lds=1):
    return Plan(0, BM, BN, waves, ring, splitk, rot, pc, 8 * min(units, slots), units, slots, lds if splitk == 1 else 0)


def _ws(BM, pc, units, splitk=1):
    return Plan(1 if BM == 128 else 2, BM, 128, 10 if BM == 128 else 6, 4, splitk, 0, pc, 8 * min(units, 32), units, 32,
                int(splitk == 1))


# name -> Spec.  M x N x K.  `units` on `slots`: more units than slots = some workgroup runs a second tile / unit.
CASES = {
    # gemm_nt_kernel 128 x 128, 8 waves, ring 2
    'nt128-one-row': Spec(1, 64, 64, _nt(128, 128, 8, 2, 1, 1, 64), note='7 of 8 workgroups return early'),
    'nt128-two-row-blocks': Spec(130, 64, 64, _nt(128, 128, 8, 2, 1, 1, 64)),
    'nt128-pc8-global-bias': Spec(40, 3080, 64, _nt(128, 128, 8, 2, 8, 4, 64, lds=0), note='last column tile 8 wide'),
    'nt128-under-192-rule': Spec(8191, 192, 64, _nt(128, 128, 8, 2, 1, 16, 64)),
    'nt128-second-tile-1-stage': Spec(4200, 2056, 64, _nt(128, 128, 8, 2, 2, 81, 64), note='M tail 104'),
    'nt128-second-tile-2-stages': Spec(4200, 2048, 128, _nt(128, 128, 8, 2, 2, 72, 64)),
    'nt128-second-tile-3-stages': Spec(4097, 2056, 192, _nt(128, 128, 8, 2, 2, 81, 64), note='M tail 1'),
    'nt128-pc4-wide': Spec(2100, 4104, 512, _nt(128, 128, 8, 2, 4, 81, 64, lds=0)),
    # gemm_nt_kernel 64 x 128, ring 3
    'nt64-over-ws-limit': Spec(1025, 264, 512, _nt(64, 128, 4, 3, 2, 10, 64)),
    'nt64-wide': Spec(1100, 3080, 1536, _nt(64, 128, 4, 3, 4, 63, 64, lds=0)),
    'nt64-pc8-second-tile': Spec(1000, 4104, 512, _nt(64, 128, 4, 3, 8, 80, 64, lds=0)),
    # gemm_nt_kernel 128 x 192, ring 3
    'nt192-one-second-tile-1-stage': Spec(32800, 192, 64, _nt(128, 192, 8, 3, 1, 33, 32), note='257 tiles on 256 workgroups'),
    'nt192-one-second-tile-2-stages': Spec(32800, 192, 128, _nt(128, 192, 8, 3, 1, 33, 32)),
    'nt192-two-columns': Spec(16400, 384, 128, _nt(128, 192, 8, 3, 1, 34, 32)),
    'nt192-three-tiles': Spec(33000, 576, 192, _nt(128, 192, 8, 3, 1, 99, 32)),
    # gemm_nt_kernel 64 x 192, ring 2
    'nt64x192': Spec(8192, 192, 64, _nt(64, 192, 4, 2, 1, 16, 64)),
    'nt64x192-tail-8': Spec(8200, 192, 64, _nt(64, 192, 4, 2, 1, 17, 64)),
    'nt64x192-two-columns': Spec(8200, 384, 128, _nt(64, 192, 4, 2, 1, 34, 64)),
    # gemm_ws_kernel 128 x 128
    'ws128-ragged': Spec(1030, 200, 1536, _ws(128, 1, 4), note='18 tiles, last column tile 72 wide'),
    'ws128-second-tile': Spec(2100, 1912, 1536, _ws(128, 2, 40)),
    'ws128-odd-stages': Spec(2100, 1912, 1600, _ws(128, 2, 40), note='25 stages: the fragment pair ends on the other buffer'),
    # gemm_ws_kernel 64 x 128, one pass
    'ws64-one-row': Spec(1, 64, 512, _ws(64, 1, 1)),
    'ws64-1000': Spec(1000, 264, 512, _ws(64, 2, 8)),
    'ws64-1024': Spec(1024, 264, 512, _ws(64, 2, 8)),
    # gemm_ws_kernel 64 x 128, the planner's slices + splitk_reduce_kernel
    'ws64-2-slices-one-row': Spec(1, 64, 1536, _ws(64, 1, 2, splitk=2)),
    'ws64-2-slices': Spec(70, 72, 1536, _ws(64, 1, 2, splitk=2)),
    'ws64-4-slices': Spec(520, 264, 3072, _ws(64, 2, 24, splitk=4)),
    'ws64-4-slices-second-unit': Spec(1024, 768, 3072, _ws(64, 2, 48, splitk=4)),
    'ws64-12-slices-pc8': Spec(128, 1024, 9216, _ws(64, 8, 24, splitk=12)),
    # slices forced through CLV_GEMM_SPLITK
    'forced-12-slices': Spec(300, 200, 1536, _ws(64, 2, 24, splitk=12), force=12, note='2-stage units in a ring of 4'),
    'forced-5-slices': Spec(300, 200, 1536, _ws(64, 2, 10, splitk=5), force=5, note='4, 5, 5, 5, 5 stages'),
    'forced-ws128-8-slices': Spec(1030, 200, 1536, _ws(128, 1, 32, splitk=8), force=8),
    'forced-nt-partial': Spec(300, 3080, 1536, _nt(128, 128, 8, 2, 8, 36, 64, splitk=3, lds=0), force=3,
                              note='the only route to gemm_nt_kernel<PARTIAL>'),
    # the K walk rotated (CLV_GEMM_ROT=1)
    'rot-nt128': Spec(4097, 2056, 192, _nt(128, 128, 8, 2, 2, 81, 64, rot=1), rot=1),
    'rot-nt64': Spec(1100, 3080, 1536, _nt(64, 128, 4, 3, 4, 63, 64, rot=1, lds=0), rot=1),
    'rot-nt-partial': Spec(300, 3080, 1536, _nt(128, 128, 8, 2, 8, 36, 64, splitk=3, rot=1, lds=0), force=3, rot=1),
}
ROT_PAIRS = {'rot-nt128': 'nt128-second-tile-3-stages', 'rot-nt64': 'nt64-wide', 'rot-nt-partial': 'forced-nt-partial'}
# all six epilogues: one case per kernel class, and one through the reduce kernel
ALL_EPI = ('nt128-two-row-blocks', 'nt64-over-ws-limit', 'nt192-one-second-tile-2-stages', 'nt64x192-tail-8', 'ws128-ragged',
           'ws64-1000', 'ws64-2-slices')
# the five shapes of test_kernels_gpu.py::test_gemm_nt_split_k_and_rotation and its (splitk, rot) settings
OLD_ROT_SHAPES = ((3136, 768, 3072), (512, 768, 3072), (3648, 768, 3072), (300, 200, 1536), (1000, 136, 2048))
OLD_ROT_SETTINGS = (('0', '1'), ('2', '0'), ('5', '1'), ('8', '1'), ('1', '1'))
FP8_SHAPES = ((64, 64, 128), (777, 136, 256), (520, 264, 1024))
RANDOM = ('nt128-second-tile-3-stages', 'nt64-over-ws-limit', 'nt192-two-columns', 'nt64x192-two-columns', 'ws128-ragged',
          'ws64-1000', 'ws64-4-slices')


def assert_plan(name, with_work=True):
    """The claim of CASES[name] against the library's host entry, under the case's own environment -> the Spec."""
    s = CASES[name]
    with env(s.force, s.rot):
        got = plan(s.M, s.N, s.K, with_work)
        wb = _lib.lib().clv_gemm_nt_work_bytes(s.M, s.N, s.K)
    assert got == s.claim, f'{name} {s.M}x{s.N}x{s.K}: the planner moved this case off its path: {got} (claimed {s.claim})'
    assert wb == (s.claim.splitk * s.M * s.N * 4 if s.claim.splitk > 1 else 0), f'{name}: work bytes {wb}'
    return s


def unit_stages(K, splitk):
    """stage counts of the K slices of one tile (unit_span of the kernels)"""
    nst = K // 64
    return [nst * (z + 1) // splitk - nst * z // splitk for z in range(splitk)]


def fp8_class(M, N, K):
    """BM of clv_gemm_nt_fp8: a COPY of its rule (K in bytes), which no host entry reports."""
    return 64 if (K >= 1024 and -(-M // 128) * -(-N // 128) <= 384) else 128


# ----------------------------------------------------------------------------------------------- references
def acc64(a, b, device='cpu'):
    """fp64 a b^T on `device` (exact on the generators' data)"""
    return a.to(device).double() @ b.to(device).double().t()


def acc_int64(a, b, scale, rows):
    """independent reference of some rows of the accumulator: int64 arithmetic on the operands times `scale`"""
    ai = (a[rows].double() * scale[0])
    bi = (b.double() * scale[1])
    assert torch.equal(ai, ai.round()) and torch.equal(bi, bi.round())
    return ai.to(torch.int64) @ bi.to(torch.int64).t()


def round16(t):
    return t.to(HALF).double()


def expected(epi, acc, bias, aux):
    """fp64 (c, c2) of an epilogue; bias enters ROUNDED to the 16-bit type, as in every kernel path.  acc, bias [N], aux
    [M][N]: fp64 on one device.  c2 is None where the epilogue leaves none."""
    if epi == EPI_NONE:
        return acc, None
    if epi == EPI_MUL:
        return acc * aux, None
    if epi == EPI_DGELU:
        return acc * nr.gelu_grad64(aux), None
    pre = acc + round16(bias)
    if epi == EPI_BIAS:
        return pre, None
    if epi == EPI_GELU:
        return nr.gelu64(pre), pre
    return nr.gelu64(pre), nr.gelu_grad64(pre)


def allowance(epi, acc, bias, aux):
    """(allowance on c, allowance on c2) as fp64 tensors, None = bit-exact (the fp64 result converted once)."""
    if epi in (EPI_NONE, EPI_BIAS, EPI_MUL):
        return None, None
    if epi == EPI_DGELU:
        g = nr.gelu_grad64(aux)
        return (nr.spacing16(g, HALF) + GELU_GRAD_TERM * (1 + aux.abs())) * acc.abs(), None
    pre = acc + round16(bias)
    fwd = nr.spacing16(nr.gelu64(pre), HALF) + GELU_TERM * pre.abs()
    if epi == EPI_GELU:
        return fwd, None
    return fwd, nr.spacing16(nr.gelu_grad64(pre), HALF) + GELU_GRAD_TERM * (1 + pre.abs())


# ----------------------------------------------------------------------------------------------- generators
class Case(NamedTuple):
    a: torch.Tensor             # HALF [M][K] (CPU)
    b: torch.Tensor             # HALF [N][K]
    bias: torch.Tensor          # fp32 [N]
    aux: torch.Tensor           # HALF [M][N]
    acc: torch.Tensor           # fp64 [M][N] on the device the case was made for: the exact a b^T
    density: float
    q: float                    # the unit all values are multiples of


def check_caps(a, b, bias, acc, q):
    """The two caps (module docstring), on the inputs and the reference alone.  |a| |b|^T is bounded per element by
    min(max_m sum_k |a| * max |b|, max |a| * max_n sum_k |b|), so no second product is needed."""
    for t in (a, b):
        assert t.dtype == HALF
    for t in (a.double(), b.double(), bias.double(), acc):
        assert torch.equal(t / q, (t / q).round()), f'a value is not a multiple of {q}: the exact reference takes none such'
    ad, bd = a.double().abs(), b.double().abs()
    absdot = min(ad.sum(1).max().item() * bd.max().item(), ad.max().item() * bd.sum(1).max().item()) + bias.abs().max().item()
    assert absdot / q < CAP, f'|a||b|^T + |bias| may reach {absdot / q} units >= 2^24: fp32 accumulation would depend on the order'
    top = (acc + bias.double().to(acc.device)).abs().max().item()
    top = max(top, acc.abs().max().item())
    assert top / q <= TOP, f'max |acc + bias| is {top / q} units > {TOP}: not every sum is a 16-bit value'


def _tern(g, dens, *shape):
    keep = torch.rand(shape, generator=g) < dens
    return ((torch.randint(0, 2, shape, generator=g) * 2 - 1) * keep).float()


@functools.lru_cache(maxsize=None)
def exact_case(M, N, K, gelu=False, device='cpu', seed=0):
    """Ternary operands at the largest density that meets the caps.  gelu: b in {0, +-1/8}, bias multiples of 1/16 in
    [-2, 2] — the pre-activation is then a multiple of 1/16 of magnitude <= 16, exact in both 16-bit types, and spans the
    curved part of GELU; aux (the DGELU operand) multiples of 1/16 in [-4, 4].  Otherwise aux in {0, +-1/2, +-1, +-2}."""
    q = 1 / 16 if gelu else 1.0
    why = None
    for i, dens in enumerate(DENSITIES):
        g = torch.Generator().manual_seed(1000003 * seed + 7919 * M + 31 * N + K + 104729 * i + int(gelu))
        a = _tern(g, dens, M, K).to(HALF)
        b = (_tern(g, dens, N, K) * (0.125 if gelu else 1.0)).to(HALF)
        if gelu:
            bias = torch.randint(-32, 33, (N,), generator=g).float() / 16
            aux = (torch.randint(-64, 65, (M, N), generator=g).float() / 16).to(HALF)
        else:
            bias = torch.randint(-8, 9, (N,), generator=g).float()
            aux = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0])[torch.randint(0, 7, (M, N), generator=g)].to(HALF)
        acc = acc64(a, b, device)
        try:
            check_caps(a, b, bias, acc, q)
        except AssertionError as e:
            why = e
            continue
        return Case(a, b, bias, aux, acc, dens, q)
    raise AssertionError(f'{M}x{N}x{K}: no density meets the caps ({why})')


@functools.lru_cache(maxsize=None)
def gauss_case(M, N, K, seed=0):
    """Gaussian 16-bit operands (a b^T of unit variance), a bias already rounded to 16 bits, aux ~ N(0, 1) -> (a, b, bias, aux)"""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * M + 31 * N + K + 3)
    r = lambda *s: torch.randn(*s, generator=g)
    return r(M, K).to(HALF), (r(N, K) * K ** -0.5).to(HALF), (r(N) * 0.5).to(HALF).float(), r(M, N).to(HALF)


# ----------------------------------------------------------------------------------------------- fp8
def e4m3(t):
    """OCP e4m3 bytes of a tensor of {-1, 0, 1}: 0x38 = 1.0, 0xb8 = -1.0, 0 = 0."""
    assert set(t.unique().tolist()) <= {-1.0, 0.0, 1.0}
    return torch.where(t > 0, 0x38, torch.where(t < 0, 0xb8, 0)).to(torch.uint8)


@functools.lru_cache(maxsize=None)
def fp8_case(M, N, K, device='cpu', seed=0):
    """Ternary e4m3 operands, power-of-two per-row scales sa in {1/8, 1/4}, sb in {1/2, 1}, a bias of multiples of 1/16 in
    [-2, 2]: pre = acc * sa * sb + bias is a multiple of 1/16 and must stay within 16 (256 units: a 16-bit value, on the
    curved part of GELU) -> (a, b, sa, sb, bias, pre fp64)."""
    why = None
    for i, dens in enumerate(DENSITIES):
        g = torch.Generator().manual_seed(1000003 * seed + 7919 * M + 31 * N + K + 104729 * i + 5)
        a, b = _tern(g, dens, M, K), _tern(g, dens, N, K)
        sa = torch.tensor([0.125, 0.25])[torch.randint(0, 2, (M,), generator=g)]
        sb = torch.tensor([0.5, 1.0])[torch.randint(0, 2, (N,), generator=g)]
        bias = torch.randint(-32, 33, (N,), generator=g).float() / 16
        acc = acc64(a, b, device)
        pre = acc * sa.double().to(device)[:, None] * sb.double().to(device)[None, :] + bias.double().to(device)
        assert (a.abs().sum(1).max().item() + 2) * 16 < CAP
        if max(pre.abs().max().item(), (pre - bias.double().to(device)).abs().max().item()) * 16 <= TOP:
            return a, b, sa, sb, bias, pre
        why = f'max |pre| {pre.abs().max().item()}'
    raise AssertionError(f'fp8 {M}x{N}x{K}: no density meets the caps ({why})')
