"""The two routes a parameter gradient takes out of a backward of clover_amd.ops — into the engine-style fp32 sink
(``_clv_grad`` + one ``_clv_ready`` call, nothing returned to autograd) or back to autograd — for every op family that
produces one, each at a small shape its own kernels take.  `-m gpu` only."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from clover_amd import _lib as _clv_lib  # noqa: E402

DEV = 'cuda'
HALF = _clv_lib.half_dtype()


def ops():
    from clover_amd import ops as o
    return o


def rnd(*shape, scale=1.0, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


class Case:
    """params: name -> seeded fp32 CPU tensor; groups: the parameters whose sinks the op decides on TOGETHER (all or
    nothing); run(P): forward + backward on fresh device leaves P of the same names, identical inputs every time."""

    per_param = False                   # True: the op decides parameter by parameter (the QA head)

    def __init__(self, params, groups, run):
        self.params, self.groups, self.run = params, groups, run

    def attach(self, P, names):
        """Zero-filled fp32 sinks on P[k] for k in names -> {k: the tensor to compare with the gradient}."""
        for k in names:
            P[k]._clv_grad = torch.zeros_like(P[k], dtype=torch.float32)
        return {k: P[k]._clv_grad for k in names}


def _dev(*ts):
    return [t.to(DEV) if t is not None else None for t in ts]


def case_linear():
    M, N, K = 3000, 96, 96                                   # tests/test_kernels_gpu.py test_linear_and_wgrad
    x, dy = _dev(rnd(M, K, seed=71).to(HALF), rnd(M, N, seed=74).to(HALF))

    def run(P):
        ops().linear(x.clone().requires_grad_(), P['w'], P['b']).backward(dy)
    return Case(dict(w=rnd(N, K, scale=0.05, seed=72), b=rnd(N, scale=0.1, seed=73)), [('w', 'b')], run)


def case_linear_f32():
    M, N, K = 3, 130, 70                                     # tests/test_parity_gpu.py test_linear_f32_heads
    x, dy = _dev(rnd(M, K, seed=51), rnd(M, N, seed=54))

    def run(P):
        ops().linear_f32(x.clone().requires_grad_(), P['w'], P['b']).backward(dy)
    return Case(dict(w=rnd(N, K, seed=52) * 0.05, b=rnd(N, seed=53)), [('w', 'b')], run)


def _block_inputs(C):                                        # tests/test_kernels_gpu.py test_fused_ln_linear_and_mlp
    M, Hd = 3000, 4 * C
    P = dict(g=1 + 0.1 * rnd(C, seed=123), b=0.1 * rnd(C, seed=124), wq=rnd(3 * C, C, scale=0.1, seed=125),
             bq=0.1 * rnd(3 * C, seed=126), w1=rnd(Hd, C, scale=0.1, seed=127), b1=0.1 * rnd(Hd, seed=128),
             w2=rnd(C, Hd, scale=0.05, seed=129), b2=0.1 * rnd(C, seed=130))
    a, r, dq, dm, ds = _dev(*[rnd(M, n, seed=s).to(HALF) for n, s in ((C, 121), (C, 122), (3 * C, 131), (C, 132), (C, 133))])
    return P, a, r, dq, dm, ds


def case_ln_linear():
    P, a, r, dq, _, ds = _block_inputs(96)

    def run(Q):
        q, s = ops().ln_linear(a.clone().requires_grad_(), r.clone().requires_grad_(), Q['g'], Q['b'], Q['wq'], Q['bq'])
        torch.autograd.backward([q, s], [dq, ds])
    return Case({k: P[k] for k in ('wq', 'bq', 'g', 'b')}, [('wq', 'bq', 'g', 'b')], run)


def _case_fused_mlp(C):
    P, a, r, _, dm, ds = _block_inputs(C)

    def run(Q):
        a2 = a.clone().requires_grad_()
        assert ops().mlp_fused_ok(a2, 4 * C) == (C == 96)    # 96: the one-kernel body; 128: the two-kernel one
        m, s = ops().fused_mlp(a2, r.clone().requires_grad_(), Q['g'], Q['b'], Q['w1'], Q['b1'], Q['w2'], Q['b2'])
        torch.autograd.backward([m, s], [dm, ds])
    return Case({k: P[k] for k in ('w1', 'b1', 'g', 'b', 'w2', 'b2')}, [('w1', 'b1', 'g', 'b'), ('w2', 'b2')], run)


def case_mlp_gelu():
    M, C, Hd = 8192, 192, 768                                # tests/test_kernels_gpu.py test_linear_and_mlp_on_the_hip_gemm
    x, dy = _dev(rnd(M, C, seed=321).to(HALF), rnd(M, C, seed=326).to(HALF))

    def run(P):
        xg = x.clone().requires_grad_()
        assert ops().mlp_gelu_ok(xg, Hd)
        ops().mlp_gelu(xg, P['w1'], P['b1'], P['w2'], P['b2']).backward(dy)
    return Case(dict(w1=rnd(Hd, C, scale=0.05, seed=322), b1=rnd(Hd, scale=0.1, seed=323),
                     w2=rnd(C, Hd, scale=0.05, seed=324), b2=rnd(C, scale=0.1, seed=325)), [('w1', 'b1'), ('w2', 'b2')], run)


def case_layer_norm():
    rows, C = 777, 192                                       # tests/test_kernels_gpu.py test_layernorm_shapes
    x, dy = _dev(rnd(rows, C, seed=91).to(HALF), rnd(rows, C, seed=92).to(HALF))

    def run(P):
        ops().layer_norm(x.clone().requires_grad_(), P['g'], P['b']).backward(dy)
    return Case(dict(g=1 + 0.1 * rnd(C, seed=93), b=0.1 * rnd(C, seed=94)), [('g', 'b')], run)


def case_merge_layer_norm():
    B, D, H, W, C = 2, 3, 6, 10, 128                         # tests/test_kernels_gpu.py test_merge_layer_norm
    x, r, dy = _dev(rnd(B, D, H, W, C, seed=141).to(HALF), rnd(B, D, H, W, C, seed=142).to(HALF),
                    rnd(B, D, H // 2, W // 2, 4 * C, seed=145).to(HALF))
    sc = torch.tensor([0.0, 1.25], device=DEV)

    def run(P):
        ops().merge_layer_norm(x.clone().requires_grad_(), P['g'], P['b'], 1e-5, residual=r.clone().requires_grad_(),
                               x_scale=sc).backward(dy)
    return Case(dict(g=1 + 0.1 * rnd(4 * C, seed=143), b=0.1 * rnd(4 * C, seed=144)), [('g', 'b')], run)


def case_embedding():
    V, Hh = 500, 64                  # BertEmbeddings' word lookup: ids with repeats and padding rows, a ragged [3, 17] batch
    ids = torch.randint(0, V, (3, 17), generator=torch.Generator().manual_seed(5))
    ids[:, -4:] = 0
    ids[1, 2] = ids[0, 2]
    ids, dy = _dev(ids, rnd(3, 17, Hh, seed=6))

    def run(P):
        ops().embedding(ids, P['w'], 0).backward(dy)
    return Case(dict(w=rnd(V, Hh, seed=7)), [('w',)], run)


def case_window_attention():
    from clover_amd.backbones.swin_transformer_3d import window_geometry
    B, D, H, W, C, nH = 2, 4, 7, 7, 64, 2                    # tests/test_kernels_gpu.py WIN_CASES (clamped window)
    ws, ss, rid = window_geometry((D, H, W), (8, 7, 7), (4, 3, 3), DEV)
    qkv, do = _dev(rnd(B, D, H, W, 3 * C, seed=11).to(HALF), rnd(B, D, H, W, C, seed=13).to(HALF))

    def run(P):
        ops().window_attention(qkv.clone().requires_grad_(), P['table'], rid, ws, ss, nH, table_window=(8, 7, 7)).backward(do)
    return Case(dict(table=rnd(15 * 13 * 13, nH, scale=0.5, seed=12)), [('table',)], run)


def case_patch_embed():
    C, B, T, HW = 128, 1, 4, 56                              # tests/test_kernels_gpu.py test_patch_embed
    x = rnd(B, 3, T, HW, HW, seed=31).to(DEV)
    vm = (rnd(B, 1, 7, 7, seed=37) > 0.5).long().to(DEV)
    g1, g2 = _dev(rnd(B, T // 2, HW // 4, HW // 4, C, seed=38).to(HALF), rnd(B, T // 2, HW // 4, HW // 4, C, seed=39).to(HALF))

    def run(P):
        clean, masked = ops().patch_embed(x, P['w'], P['b'], P['g'], P['beta'], P['mt'], vm)
        torch.autograd.backward([clean, masked], [g1, g2])
    names = ('w', 'b', 'g', 'beta', 'mt')
    return Case(dict(w=rnd(C, 3, 2, 4, 4, scale=0.1, seed=32), b=0.1 * rnd(C, seed=33), g=1 + 0.1 * rnd(C, seed=34),
                     beta=0.1 * rnd(C, seed=35), mt=rnd(1, C, 1, 1, 1, scale=0.3, seed=36)), [names], run)


def case_mlm_decoder():
    R, V, Hh = 64, 1003, 128                                 # tests/test_kernels_gpu.py test_mlm_decoder_padded_vocabulary
    Vp = V + (-V % 64)
    x, dy = _dev(rnd(R, Hh, seed=601).to(HALF), rnd(R, V, seed=605).to(HALF))

    def run(P):
        ops().mlm_decoder(x.clone().requires_grad_(), P['w'], P['b']).backward(dy)

    class Padded(Case):
        def attach(self, P, names):
            """The engine's phantom-padded views (engine._Segment): operands on both parameters, ``_clv_pad_grad`` on
            `names`; what is compared is the first V rows of the sink, and the phantom rows behind them stay zero."""
            wp = torch.zeros(Vp, Hh, device=DEV)
            wp[:V] = P['w'].detach()
            bp = torch.zeros(Vp, device=DEV)
            bp[:V] = P['b'].detach()
            P['w']._clv_pad_shadow, P['w']._clv_pad_shadow_t = wp.to(HALF), wp.to(HALF).t().contiguous()
            P['b']._clv_pad_weight = bp
            for k in names:
                P[k]._clv_pad_grad = torch.zeros((Vp, Hh) if k == 'w' else (Vp,), device=DEV)
            self.padded = [P[k]._clv_pad_grad for k in names]
            return {k: P[k]._clv_pad_grad[:V] for k in names}
    case = Padded(dict(w=rnd(V, Hh, scale=0.05, seed=602), b=rnd(V, scale=0.1, seed=603)), [('w', 'b')], run)
    case.V = V
    return case


def case_qa_head():
    D, Hh, K, M, S = 128, 64, 37, 5, 3                       # tests/test_qa_gpu.py test_qa_head_matches_fp32_torch
    g = torch.Generator().manual_seed(D + Hh + K + M)
    h = torch.randn(M, S, D, generator=g).to(DEV, HALF)
    rows = (torch.arange(M) * S + torch.randint(0, S, (M,), generator=g)).to(DEV, torch.int32)
    dl = rnd(M, K, seed=8).to(DEV)
    names = ('w1', 'b1', 'g', 'b', 'w2', 'b2')
    u = lambda *shape, seed: torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1    # noqa: E731

    def run(P):
        ops().qa_head(h.clone().requires_grad_(), rows, *[P[k] for k in names], drop_p=0.0).backward(dl)
    case = Case(dict(w1=u(Hh, D, seed=1) * D ** -0.5, b1=u(Hh, seed=2) * 0.1, g=1 + u(Hh, seed=3) * 0.1, b=u(Hh, seed=4) * 0.1,
                     w2=u(K, Hh, seed=5) * Hh ** -0.5, b2=u(K, seed=6) * 0.1), [names], run)
    case.per_param = True            # (`groups` only names the parameter (c) leaves without a sink: the last one)
    return case


CASES = dict(linear=case_linear, linear_f32=case_linear_f32, ln_linear=case_ln_linear,
             fused_mlp=lambda: _case_fused_mlp(96), fused_mlp_two_kernels=lambda: _case_fused_mlp(128),
             mlp_gelu=case_mlp_gelu, layer_norm=case_layer_norm, merge_layer_norm=case_merge_layer_norm,
             embedding=case_embedding, window_attention=case_window_attention, patch_embed=case_patch_embed,
             mlm_decoder=case_mlm_decoder, qa_head=case_qa_head)

# max |difference| / max |gradient| between two routes.  The routes run the same kernels on the same inputs and differ
# only in the buffer the gradient lands in, so what separates them is the order of fp32 atomic adds: the bound the
# project uses for that comparison (tests/test_parity_gpu.py test_linear_f32_heads, tests/test_kernels_gpu.py
# test_wgrad_accumulates_into_sink), 1e-5.  Measured on an MI355X on the commit BEFORE the sink helpers existed (this
# test runs there unchanged): fused_mlp 6.7e-7, its two-kernel form 3.6e-7, ln_linear 3.4e-7, patch_embed 2.1e-7,
# layer_norm 1.8e-7, merge_layer_norm 1.3e-7 (all in gamma / beta / mask token: atomics), every other op 0 — no op
# needs a bound of its own.
BOUND = 1e-5


def _route(case, sunk):
    """One forward + backward with sinks on the parameters `sunk` -> (leaves, sinks, ``_clv_ready`` calls per name)."""
    P = {k: v.to(DEV).requires_grad_() for k, v in case.params.items()}
    calls = {k: [] for k in sunk}
    sinks = case.attach(P, sunk) if sunk else {}
    for k in sunk:
        P[k]._clv_ready = lambda k=k: calls[k].append(1)
    case.run(P)
    torch.cuda.synchronize()
    return P, sinks, {k: len(v) for k, v in calls.items()}


@pytest.mark.parametrize('name', list(CASES))
def test_gradient_routes(name):
    """(a) no sinks: every gradient arrives in .grad.  (b) a sink on every parameter: nothing in .grad, each
    ``_clv_ready`` called exactly once, each sink holds the gradient of (a).  (c) the last parameter of every group
    WITHOUT a sink: the whole group goes back to autograd — every gradient in .grad as in (a), the attached sinks
    untouched, no ``_clv_ready`` call; the QA head decides per parameter instead: the one without a sink is returned,
    the other five are delivered as in (b).  A group of one parameter leaves nothing attached in (c): route (a) again,
    which must reproduce itself.

    On the commit before the helpers (c) of mlm_decoder raised AttributeError: a padded weight whose bias lacks the
    padded sink was taken for engine-managed."""
    torch.manual_seed(0)
    ops().LIBRARY_GEMM_CALLS.clear()
    case = CASES[name]()
    names = list(case.params)

    def same(tag, got, want):
        r = rel(got, want)
        print(f'{name} {tag}: {r:.3g}')
        assert r <= BOUND, (name, tag, r)

    Pa, _, _ = _route(case, ())
    ref = {k: Pa[k].grad for k in names}
    for k in names:
        assert ref[k] is not None and ref[k].dtype == torch.float32 and float(ref[k].abs().max()) > 0, k

    Pb, sinks, calls = _route(case, names)
    for k in names:
        assert Pb[k].grad is None, k
        assert calls[k] == 1, (k, calls)
        same(f'(b) {k}', sinks[k], ref[k])
    if hasattr(case, 'padded'):
        assert all(float(t[case.V:].abs().max()) == 0.0 for t in case.padded)

    dropped = [grp[-1] for grp in case.groups]
    kept = [k for k in names if k not in dropped]
    Pc, sinks, calls = _route(case, kept)
    for k in names:
        if case.per_param and k in kept:
            assert Pc[k].grad is None and calls[k] == 1, (k, calls)
            same(f'(c) {k}', sinks[k], ref[k])
        else:
            assert Pc[k].grad is not None, k
            same(f'(c) {k}', Pc[k].grad, ref[k])
            if k in kept:
                assert calls[k] == 0, (k, calls)
                assert float(sinks[k].abs().max()) == 0.0, k
    assert not ops().LIBRARY_GEMM_CALLS, ops().LIBRARY_GEMM_CALLS      # every case ran on the own kernels
