"""tests/gemm_ref.py without a GPU: every generator meets the caps that make fp32 accumulation order-independent at every
shape tests/test_gemm_nt_gpu.py uses, an independent int64 reference reproduces the fp64 one, and the planning facts the
cases claim hold through the library's own host entry clv_gemm_nt_plan (a retuned planner fails HERE, on the claim, not
quietly on another kernel)."""
import ctypes as C

import pytest
import torch

import gemm_ref as gr
from clover_amd import _lib


def L():
    return _lib.lib()


SHAPES = sorted({(s.M, s.N, s.K) for s in gr.CASES.values()})
GELU_SHAPES = sorted({(gr.CASES[n].M, gr.CASES[n].N, gr.CASES[n].K) for n in gr.ALL_EPI})


def _rows(M):
    g = torch.Generator().manual_seed(M)
    return torch.unique(torch.cat([torch.tensor([0, M - 1]), torch.randint(0, M, (30,), generator=g)]))


@pytest.mark.parametrize('M,N,K', SHAPES)
def test_exact_generator_meets_its_caps(M, N, K):
    """The generator asserts the caps itself; here additionally: the value sets, and 32 rows of the fp64 accumulator against
    int64 arithmetic."""
    c = gr.exact_case(M, N, K)
    assert c.density in gr.DENSITIES and c.q == 1.0
    assert set(c.a.unique().tolist()) <= {-1.0, 0.0, 1.0} and set(c.b.unique().tolist()) <= {-1.0, 0.0, 1.0}
    assert c.bias.abs().max() <= 8 and torch.equal(c.bias, c.bias.round())
    assert set(c.aux.unique().tolist()) <= {0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0}
    gr.check_caps(c.a, c.b, c.bias, c.acc, 1.0)
    assert (c.acc + c.bias.double()).abs().max() <= gr.TOP and c.acc.abs().max() > 8      # (and the sums are not trivial)
    r = _rows(M)
    assert torch.equal(gr.acc_int64(c.a, c.b, (1, 1), r).double(), c.acc[r])
    # the 16-bit conversion of every expected output is the identity, or a single rounding of an exactly known value
    for epi in (gr.EPI_NONE, gr.EPI_BIAS):
        want, _ = gr.expected(epi, c.acc, c.bias.double(), c.aux.double())
        assert torch.equal(gr.round16(want), want)
    mul, _ = gr.expected(gr.EPI_MUL, c.acc, c.bias.double(), c.aux.double())
    assert torch.equal(mul.float().double(), mul) and mul.abs().max() <= 2 * gr.TOP


@pytest.mark.parametrize('M,N,K', GELU_SHAPES)
def test_gelu_generator_meets_its_caps(M, N, K):
    c = gr.exact_case(M, N, K, gelu=True)
    assert c.q == 1 / 16 and set((c.b.double() * 8).unique().tolist()) <= {-1.0, 0.0, 1.0}
    pre = c.acc + c.bias.double()
    assert pre.abs().max() <= 16 and torch.equal(gr.round16(pre), pre) and torch.equal(pre * 16, (pre * 16).round())
    assert pre.abs().max() >= 2, 'the pre-activation does not span the curved part of GELU'
    assert c.aux.double().abs().max() <= 4 and torch.equal(c.aux.double() * 16, (c.aux.double() * 16).round())
    r = _rows(M)
    assert torch.equal(gr.acc_int64(c.a, c.b, (1, 8), r).double() / 8, c.acc[r])


def test_density_claims_of_the_budget_file():
    """the three figures quoted in GEMM_ERROR_BUDGET.md: which density the generator lands on at the three heaviest shapes"""
    assert gr.exact_case(128, 1024, 9216).density == 1 / 2 and gr.exact_case(1024, 768, 3072).density >= 1 / 2
    assert gr.exact_case(2100, 1912, 1536).density == 2 / 3


def test_caps_are_enforced():
    """Inputs that break a cap must raise, not hand out data for which a bit-exact comparison proves nothing."""
    a = torch.full((8, 4096), 64.0).to(gr.HALF)
    with pytest.raises(AssertionError, match='2\\^24'):
        gr.check_caps(a, a, torch.zeros(8), gr.acc64(a, a), 1.0)
    ones = torch.ones(8, 320).to(gr.HALF)
    with pytest.raises(AssertionError, match='not every sum is a 16-bit value'):
        gr.check_caps(ones, ones, torch.zeros(8), gr.acc64(ones, ones), 1.0)
    with pytest.raises(AssertionError, match='not every sum is a 16-bit value'):          # the bias counts
        gr.check_caps(ones[:, :250], ones[:, :250], torch.full((8,), 8.0), gr.acc64(ones[:, :250], ones[:, :250]), 1.0)
    half = torch.full((8, 64), 0.5).to(gr.HALF)
    with pytest.raises(AssertionError, match='not a multiple'):
        gr.check_caps(half, ones[:, :64], torch.zeros(8), gr.acc64(half, ones[:, :64]), 1.0)
    gr.check_caps(ones[:, :248], ones[:, :248], torch.full((8,), 8.0), gr.acc64(ones[:, :248], ones[:, :248]), 1.0)


@pytest.mark.parametrize('name', list(gr.CASES))
def test_plans(name):
    s = gr.assert_plan(name)
    p = s.claim
    assert p.grid == 8 * min(p.units, p.slots) and (p.splitk == 1 or p.bias_lds == 0)
    # without a work buffer nothing is sliced, whatever the environment says
    with gr.env(s.force, s.rot):
        assert gr.plan(s.M, s.N, s.K, with_work=False).splitk == 1
    if p.splitk > 1:
        st = gr.unit_stages(s.K, p.splitk)
        assert sum(st) == s.K // 64 and min(st) >= 2


def test_plans_name_the_geometries():
    """The facts the cases were chosen for, stated on the claims (which test_plans holds against the library)."""
    c = {n: s.claim for n, s in gr.CASES.items()}
    classes = {(p.kernel, p.BM, p.BN, p.waves, p.ring) for p in c.values()}
    assert classes == {(0, 128, 128, 8, 2), (0, 64, 128, 4, 3), (0, 128, 192, 8, 3), (0, 64, 192, 4, 2), (1, 128, 128, 10, 4),
                       (2, 64, 128, 6, 4)}
    second = lambda n: c[n].units > c[n].slots
    # a second tile after 1, 2 and 3 stages in the ring-2 class, after 1 and 2 (< R - 1 = 2: the drain) in the 128 x 192 class
    for n, stages in (('nt128-second-tile-1-stage', 1), ('nt128-second-tile-2-stages', 2), ('nt128-second-tile-3-stages', 3),
                      ('nt192-one-second-tile-1-stage', 1), ('nt192-one-second-tile-2-stages', 2)):
        assert second(n) and gr.CASES[n].K // 64 == stages
    assert c['nt192-one-second-tile-1-stage'].units == c['nt192-one-second-tile-1-stage'].slots + 1     # exactly one workgroup
    assert -(-32800 // 128) == 257 and c['nt192-three-tiles'].units >= 3 * c['nt192-three-tiles'].slots
    assert second('nt128-pc4-wide') and c['nt128-pc4-wide'].pc == 4 and second('nt64-pc8-second-tile')
    assert (c['nt64-pc8-second-tile'].pc, c['nt64-pc8-second-tile'].units, c['nt64-pc8-second-tile'].slots) == (8, 80, 64)
    assert (c['ws128-second-tile'].pc, c['ws128-second-tile'].units, c['ws128-second-tile'].slots) == (2, 40, 32)
    assert gr.CASES['ws128-odd-stages'].K // 64 == 25
    assert (c['ws64-4-slices-second-unit'].splitk, c['ws64-4-slices-second-unit'].units) == (4, 48)
    assert (c['ws64-12-slices-pc8'].splitk, c['ws64-12-slices-pc8'].pc) == (12, 8)
    # the 64 x 192 class never has more units than slots: it is chosen only below 257 tiles of 128 rows, i.e. <= 512 of 64
    for n, p in c.items():
        if (p.BM, p.BN) == (64, 192):
            assert p.units <= p.slots, n
    assert gr.unit_stages(1536, 12) == [2] * 12 and gr.unit_stages(1536, 5) == [4, 5, 5, 5, 5]
    # both bias paths of the one-pass kernels, and the reduce kernel's
    assert {p.bias_lds for p in c.values() if p.splitk == 1 and p.kernel == 0} == {0, 1}
    assert c['forced-nt-partial'].kernel == 0 and c['forced-nt-partial'].splitk == 3
    assert c['forced-ws128-8-slices'].kernel == 1 and c['forced-ws128-8-slices'].splitk == 8
    for r, base in gr.ROT_PAIRS.items():
        assert c[r].rot == 1 and c[base].rot == 0 and c[r]._replace(rot=0) == c[base]
        assert gr.CASES[r][:3] == gr.CASES[base][:3]
    for names in (gr.ALL_EPI, gr.RANDOM):
        assert {(c[n].kernel, c[n].BM, c[n].BN) for n in names} == {(k, bm, bn) for k, bm, bn, _, _ in classes}
        assert any(c[n].splitk > 1 for n in names)


def test_the_old_rotation_test_reaches_no_rotating_kernel():
    """test_kernels_gpu.py::test_gemm_nt_split_k_and_rotation sets CLV_GEMM_ROT=1 on five shapes; every one of its 25
    settings plans to a wave-specialised kernel, which takes no rotation argument (recorded in GEMM_ERROR_BUDGET.md)."""
    for M, N, K in gr.OLD_ROT_SHAPES:
        for splitk, rot in gr.OLD_ROT_SETTINGS:
            with gr.env(splitk, rot):
                p = gr.plan(M, N, K)
            assert p.kernel in (1, 2) and p.rot == 0, (M, N, K, splitk, rot, p)
    # and none of them reaches gemm_nt_kernel<PARTIAL>
    with gr.env(3, 1):
        assert gr.plan(300, 3080, 1536) == gr.CASES['rot-nt-partial'].claim


def test_rotation_needs_three_stages_and_the_one_kernel_class():
    with gr.env(None, 1):
        assert gr.plan(4200, 2048, 128).rot == 0 and gr.plan(4097, 2056, 192).rot == 1
        assert gr.plan(1000, 264, 512).rot == 0                  # wave-specialised
        assert gr.plan(32800, 192, 192).rot == 1                 # the 192-column classes rotate too


def test_fp8_class_rule():
    """The copy of clv_gemm_nt_fp8's rule puts the three fp8 shapes where the GPU test says (no host entry pins it)."""
    assert [gr.fp8_class(*s) for s in gr.FP8_SHAPES] == [128, 128, 64]
    for M, N, K in gr.FP8_SHAPES:
        assert L().clv_gemm_nt_fp8_supported(M, N, K) == 1
        a, b, sa, sb, bias, pre = gr.fp8_case(M, N, K)
        assert torch.equal(gr.round16(pre), pre) and pre.abs().max() <= 16 and torch.equal(pre * 16, (pre * 16).round())
        assert set(gr.e4m3(a).unique().tolist()) <= {0, 0x38, 0xb8}


def test_plan_entry_refuses_what_the_gemm_refuses():
    p = _lib.ClvGemmPlan()
    assert L().clv_gemm_nt_plan(64, 64, 64, 1, None) == -1 and L().clv_gemm_nt_plan(0, 64, 64, 1, p) == -1
    for M, N, K in ((64, 68, 64), (64, 64, 96), (64, 56, 64), (64, 64, 32)):
        assert L().clv_gemm_nt_plan(M, N, K, 1, p) == -2 and L().clv_gemm_nt_supported(M, N, K) == 0
    assert C.sizeof(_lib.ClvGemmPlan) == 48


def test_a_retuned_planner_fails_the_claims(monkeypatch):
    """The claims are compared with what the library says, so a library that says something else must fail them."""
    real = L()

    class Retuned:
        def __getattr__(self, k):
            return getattr(real, k)

        def clv_gemm_nt_plan(self, M, N, K, w, out):
            rc = real.clv_gemm_nt_plan(M, N, K, w, out)
            out.ring += 1
            return rc

    monkeypatch.setattr(_lib, 'lib', lambda: Retuned())
    with pytest.raises(AssertionError, match='off its path'):
        gr.assert_plan('ws64-1000')
