"""The loss section at a global batch (virtual ranks): the multi-workgroup log-sum-exp kernels and LDS-tiled GEMMs of
csrc/losses.hip (clv_infonce_*_large, clv_normsoftmax_*_large) against the oracle in fp64, at the bounds
tests/test_kernels_gpu.py::test_infonce asserts for the one-workgroup kernels: 2e-4 relative loss, 2e-3 of the largest
gradient element.

Shapes: G = the dispatch threshold T and T + 3 with Dm = 80 (T + 3: ragged row blocks of 4 waves, a ragged last column group
of 64, partial 64 x 64 GEMM tiles; Dm = 80: a contraction that is no multiple of 64 and, with T + 3, operands that are not
16-byte aligned, so the guarded staging loads run); G = 1024 with Dm = 768 once (the reference's headline global batch:
vector staging loads, 16 x 16 tiles of the score matrices, 341 row blocks).  Entries: four tensors, four slots of a packed
tensor, the pair form; NormSoftmaxLoss at T + 3 and 1024.  `-m gpu` only."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import model as om             # noqa: E402

DEV = 'cuda'
LOSS_REL, GRAD_REL = 2e-4, 2e-3            # test_infonce's bounds
SA, SB = (0, 1, 2, 3), (1, 0, 4, 5)        # the two evaluations of the step on a packed [G, 6, Dm] tensor
WTS = (1.3, 0.7, 0.9, 1.1)                 # upstream gradients of (nce_a, rank_a, nce_b, rank_b)


def ops():
    from clover_amd import ops as o
    return o


def T():
    return ops().nce_large_min_g()


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-20)).item()


def close(got, ref):
    return abs(got - ref) < LOSS_REL * max(1.0, abs(ref))


@functools.lru_cache(maxsize=None)
def case(G, Dm):
    """packed fp32 [G, 6, Dm] (loss_ref.nce_packed: positives correlated and every third masked row flipped, so that the
    ranking hinge of both evaluations is active on some rows and inactive on others — asserted) and the fp64 oracle on it:
    the four losses of the two evaluations and the gradient of their WTS-weighted sum.  Computed once."""
    import loss_ref
    p = loss_ref.nce_packed(G, Dm)
    for s3 in (SA[:3], SB[:3]):
        loss_ref.assert_mixed_hinge(*[p[:, s] for s in s3])
    pr = p.double().requires_grad_()
    la = om.exclusive_nce_rank_loss(*[pr[:, s] for s in SA], temperature=0.05, margin=5.0, gather=False)
    lb = om.exclusive_nce_rank_loss(*[pr[:, s] for s in SB], temperature=0.05, margin=5.0, gather=False)
    ref = [la['nce_loss'], la['rank_t_tm_loss'], lb['nce_loss'], lb['rank_t_tm_loss']]
    ga, = torch.autograd.grad(WTS[0] * ref[0] + WTS[1] * ref[1], pr, retain_graph=True)
    gb, = torch.autograd.grad(WTS[2] * ref[2] + WTS[3] * ref[3], pr)
    return p, [r.item() for r in ref], ga, gb


def shapes():
    return [(T(), 80), (T() + 3, 80)]


@pytest.mark.parametrize('which', [0, 1])
def test_single_and_packed_entries(which):
    G, Dm = shapes()[which]
    assert G >= T()                                            # the dispatch takes the new path here
    p, ref, ga, _ = case(G, Dm)
    es = [p[:, s].contiguous().to(DEV).requires_grad_() for s in SA]
    nce, rank = ops().exclusive_infonce_rank(*es, 0.05, 5.0)
    (WTS[0] * nce + WTS[1] * rank).backward()
    print('single', G, Dm, nce.item() - ref[0], rank.item() - ref[1], [rel(e.grad, ga[:, s]) for e, s in zip(es, SA)])
    assert close(nce.item(), ref[0]) and close(rank.item(), ref[1]), (nce.item(), rank.item(), ref[:2])
    for e, s in zip(es, SA):
        assert rel(e.grad, ga[:, s]) < GRAD_REL, s
    pg = p.to(DEV).requires_grad_()
    nce2, rank2 = ops().exclusive_infonce_rank_packed(pg, SA, 0.05, 5.0)
    (WTS[0] * nce2 + WTS[1] * rank2).backward()
    # strided reads / strided gradient writes of the same numbers: bit for bit the four-tensor entry
    assert nce2.item() == nce.item() and rank2.item() == rank.item()
    for e, s in zip(es, SA):
        assert torch.equal(pg.grad[:, s], e.grad)
    assert pg.grad[:, [4, 5]].abs().max().item() == 0.0
    # two runs: bit-equal losses (fixed-order reductions, no float atomics)
    nce3, rank3 = ops().exclusive_infonce_rank_packed(p.to(DEV), SA, 0.05, 5.0)
    assert nce3.item() == nce2.item() and rank3.item() == rank2.item()


def _pair(G, Dm):
    p, ref, ga, gb = case(G, Dm)
    pg = p.to(DEV).requires_grad_()
    outs = ops().exclusive_infonce_rank_pair(pg, SA, SB, 0.05, 5.0)
    sum(w * o for w, o in zip(WTS, outs)).backward()
    got = [o.item() for o in outs]
    err = rel(pg.grad, ga + gb)
    print('pair', G, Dm, [a - b for a, b in zip(got, ref)], err)
    for a, b in zip(got, ref):
        assert close(a, b), (got, ref)
    assert err < GRAD_REL, err
    again = [o.item() for o in ops().exclusive_infonce_rank_pair(p.to(DEV), SA, SB, 0.05, 5.0)]
    assert again == got                                        # bit-reproducible from run to run


@pytest.mark.parametrize('which', [0, 1])
def test_pair_entry(which):
    _pair(*shapes()[which])


def test_pair_entry_at_the_headline_global_batch():
    _pair(1024, 768)


def test_dispatch_keeps_the_one_workgroup_kernels_below_the_threshold():
    """G = T - 1 runs the kernels it always ran (bit for bit what the pinned one-workgroup path gives); G = T the new ones,
    which agree with the old ones to fp32 rounding of a different summation order."""
    o = ops()
    G, Dm = T() - 1, 80
    p = case(T(), 80)[0][:G].contiguous().to(DEV)
    auto = [x.item() for x in o.exclusive_infonce_rank_pair(p, SA, SB, 0.05, 5.0)]
    o.NCE_FORCE_LARGE = False
    try:
        small = [x.item() for x in o.exclusive_infonce_rank_pair(p, SA, SB, 0.05, 5.0)]
        p2 = case(T(), 80)[0].to(DEV)
        small2 = [x.item() for x in o.exclusive_infonce_rank_pair(p2, SA, SB, 0.05, 5.0)]
    finally:
        o.NCE_FORCE_LARGE = None
    assert auto == small
    large2 = [x.item() for x in o.exclusive_infonce_rank_pair(p2, SA, SB, 0.05, 5.0)]
    for a, b in zip(large2, small2):
        assert abs(a - b) <= 1e-5 * max(1.0, abs(b)), (large2, small2)


def test_new_forward_feeds_the_old_backward():
    """At G = T: lser / lsec written by the new pass, read by the one-workgroup path's backward (clv_infonce_bwd: the shared
    nce_dsim / nce_norm_bwd kernels with the one-tile-per-wave GEMMs), give the gradients the oracle gives."""
    from clover_amd import _lib
    L = _lib.lib()
    G, Dm = shapes()[0]
    p, ref, ga, _ = case(G, Dm)
    es = [p[:, s].contiguous().to(DEV) for s in SA]
    out = torch.empty(2, device=DEV)
    work = torch.empty(L.clv_infonce_work_floats(G, Dm), device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.clv_infonce_fwd_large(*[e.data_ptr() for e in es], out.data_ptr(), work.data_ptr(), G, Dm, Dm, 0.05, 5.0,
                                   st) == 0
    assert close(out[0].item(), ref[0]) and close(out[1].item(), ref[1])
    dout = torch.tensor(WTS[:2], device=DEV)
    ds = [torch.empty_like(e) for e in es]
    assert L.clv_infonce_bwd(None, None, None, None, dout.data_ptr(), work.data_ptr(), *[d.data_ptr() for d in ds], G, Dm,
                             Dm, 0.05, 5.0, st) == 0
    torch.cuda.synchronize()
    for d, s in zip(ds, SA):
        assert rel(d, ga[:, s]) < GRAD_REL, s


@pytest.mark.parametrize('big', [False, True])
def test_norm_softmax_loss_large_path(big):
    G, Dm = (1024, 768) if big else (T() + 3, 80)
    g = torch.Generator().manual_seed(7 + G)
    v, t = torch.randn(G, Dm, generator=g), torch.randn(G, Dm, generator=g)
    t = 0.5 * v + t
    vr, tr = v.double().requires_grad_(), t.double().requires_grad_()
    lref = om.norm_softmax_loss(vr, tr, temperature=0.05, cos_sim=True, gather=False)
    lref.backward()
    vg, tg = v.to(DEV).requires_grad_(), t.to(DEV).requires_grad_()
    loss = ops().norm_softmax_loss(vg, tg, temperature=0.05, eps=1e-8)
    loss.backward()
    print('normsoftmax', G, Dm, loss.item() - lref.item(), rel(vg.grad, vr.grad), rel(tg.grad, tr.grad))
    assert close(loss.item(), lref.item()), (loss.item(), lref.item())
    assert rel(vg.grad, vr.grad) < GRAD_REL and rel(tg.grad, tr.grad) < GRAD_REL
    assert ops().norm_softmax_loss(v.to(DEV), t.to(DEV), temperature=0.05, eps=1e-8).item() == loss.item()
    # the sim_mat entry takes the same log-sum-exp kernels
    x = (torch.randn(G, G, generator=g) * 3).to(DEV).requires_grad_()
    xr = x.detach().double().cpu().requires_grad_()
    lx = ops().norm_softmax_loss(sim_mat=x)
    lx.backward()
    lxr = om.norm_softmax_loss(sim_mat=xr)
    lxr.backward()
    assert close(lx.item(), lxr.item()) and rel(x.grad, xr.grad) < GRAD_REL
