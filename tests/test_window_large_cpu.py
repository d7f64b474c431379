"""Window attention beyond 448 tokens, on the host: the part plan of csrc/attention.hip's make_geom as the C ABI reports it
(no GPU: clv_attn_seq_parts / clv_attn_part_tokens / clv_attn_window_supported compute from the geometry alone), the Python
refusal that speaks for it, and the module that raises it by name."""
import ctypes as C

import pytest
import torch

from clover_amd import _lib, ops
from clover_amd.backbones.swin_transformer_3d import SwinTransformerBlock3D, WindowAttention3D

WINDOWS = {49: (1, 7, 7), 98: (2, 7, 7), 196: (4, 7, 7), 392: (8, 7, 7), 448: (8, 8, 7), 490: (10, 7, 7), 500: (5, 10, 10),
           450: (2, 15, 15), 512: (8, 8, 8), 576: (4, 12, 12), 588: (12, 7, 7), 784: (16, 7, 7), 1024: (16, 8, 8), 1152: (8, 12, 12),
           1568: (32, 7, 7)}
# N -> (parts, tokens a part stages): P = ceil(tiles / 25) parts of ceil(tiles / P) tiles (make_geom, WIN_ONE_PART_TILES)
PLAN = {450: (2, 240), 490: (2, 256), 500: (2, 256), 512: (2, 256), 576: (2, 288), 588: (2, 304), 784: (2, 400), 1024: (3, 352)}


def geom(ws, tw, hd=32, groups=2, nH=2):
    N, Cc = ws[0] * ws[1] * ws[2], nH * hd
    return _lib.ClvAttnGeom(mode=1, groups=groups, N=N, nH=nH, hd=hd, D=ws[0], H=ws[1], W=ws[2], wd=ws[0], wh=ws[1], ww=ws[2],
                            ldq=3 * Cc, ldk=3 * Cc, ldv=3 * Cc, ldo=Cc, bwd=tw[0], bwh=tw[1], bww=tw[2], scale=hd ** -0.5,
                            dropout_p=0.0)


@pytest.mark.parametrize('hd', [16, 32, 64])
@pytest.mark.parametrize('N', [49, 98, 196, 392, 448])
def test_one_part_up_to_448_tokens(N, hd):
    L, ws = _lib.lib(), WINDOWS[N]
    for tw in (ws, (0, 0, 0)):
        g = geom(ws, tw, hd)
        assert L.clv_attn_seq_parts(C.byref(g)) == 1
        assert L.clv_attn_part_tokens(C.byref(g)) == (N + 15) // 16 * 16
        assert L.clv_attn_seq_work_bytes(C.byref(g)) == 0
    assert L.clv_attn_window_supported(*ws, *ws, hd) == 0
    assert ops.window_attention_refusal(ws, ws, hd) is None


@pytest.mark.parametrize('hd', [16, 32, 64])
@pytest.mark.parametrize('N', sorted(PLAN))
def test_part_plan_beyond_448_tokens(N, hd):
    L, ws = _lib.lib(), WINDOWS[N]
    parts, pt = PLAN[N]
    tiles = (N + 15) // 16
    assert parts == -(-tiles // 25) and pt == -(-tiles // parts) * 16 and (parts - 1) * pt < N <= parts * pt
    for tw in (ws, (0, 0, 0)):
        g = geom(ws, tw, hd)
        assert L.clv_attn_seq_parts(C.byref(g)) == parts
        assert L.clv_attn_part_tokens(C.byref(g)) == pt
        # the parts' partial results: forward [part][o] + [part][lse], backward [part][dq | dk | dv], rounded to 256 bytes
        tc = g.groups * N * g.nH * hd
        want = max(parts * (tc * 2 + g.groups * g.nH * N * 4), parts * 3 * tc * 2)
        assert L.clv_attn_seq_work_bytes(C.byref(g)) == -(-want // 256) * 256
    g = geom(ws, ws, hd)
    # the table gradient keeps its fragment order with ceil(N / 16) key tiles per query tile
    rows = (2 * ws[0] - 1) * (2 * ws[1] - 1) * (2 * ws[2] - 1)
    assert L.clv_attn_dbias_index_count(C.byref(g)) == rows * tiles * 16
    assert L.clv_attn_dbias_partial_bytes(C.byref(g)) == L.clv_attn_seq_work_bytes(C.byref(g)) + g.nH * tiles * tiles * 1024
    assert L.clv_attn_bwd_work_bytes(C.byref(g)) == g.groups * g.nH * tiles * tiles * 512 + 33 * g.nH * tiles * tiles * 1024
    assert L.clv_attn_bwd_one_kernel(C.byref(g)) != 1
    assert L.clv_attn_window_supported(*ws, *ws, hd) == 0
    assert ops.window_attention_refusal(ws, ws, hd) is None
    assert ops.window_attention_refusal(ws, None, hd) is None


@pytest.mark.parametrize('N', [1152, 1568])
def test_unsupported_beyond_1024_tokens(N):
    L, ws = _lib.lib(), WINDOWS[N]
    assert L.clv_attn_window_max_tokens() == 1024 == ops.WINDOW_MAX_TOKENS
    for hd in (16, 32, 64):
        g = geom(ws, ws, hd)
        assert L.clv_attn_seq_parts(C.byref(g)) == 0
        assert L.clv_attn_part_tokens(C.byref(g)) == 0
        assert L.clv_attn_window_supported(*ws, *ws, hd) == 3
        why = ops.window_attention_refusal(ws, ws, hd)
        assert why is not None and str(N) in why and '1024' in why and str(ws) in why


def test_clipped_window_and_the_other_refusals():
    L = _lib.lib()
    assert L.clv_attn_window_supported(12, 7, 7, 16, 7, 7, 32) == 0          # clipped under a larger table window
    g = geom((12, 7, 7), (16, 7, 7))
    assert (L.clv_attn_seq_parts(C.byref(g)), L.clv_attn_part_tokens(C.byref(g))) == PLAN[588]
    assert L.clv_attn_window_supported(16, 7, 7, 12, 7, 7, 32) == 4          # more tokens than the table's window
    assert L.clv_attn_window_supported(16, 7, 7, 16, 7, 7, 48) == 2
    assert L.clv_attn_window_supported(0, 7, 7, 16, 7, 7, 32) == 1
    assert 'head dim' in ops.window_attention_refusal((16, 7, 7), (16, 7, 7), 48)
    # the LDS statement: the largest band (a (16, 8, 8) table, 27.9 KB) beside 26 staged tiles at hd 64 still fits ...
    assert L.clv_attn_window_supported(16, 8, 8, 16, 8, 8, 64) == 0
    # ... and a band that does not is refused before any launch: 2 x 31 x 31 x 31 rows under a 2-frame clip of a (16,16,16) table
    assert L.clv_attn_window_supported(2, 16, 16, 16, 16, 16, 64) == 0       # 3 x 31 x 31 floats = 11.5 KB
    assert L.clv_attn_window_supported(4, 16, 16, 4, 64, 64, 64) == 5        # 7 x 127 x 127 floats = 452 KB


def test_kernel_names_of_the_parts():
    g = geom((16, 7, 7), (16, 7, 7), 32)
    assert ops._kname('attn_fwd_kernel', g) == 'attn_fwd_kernel<32, 25, false, 2>'
    assert ops._kname('attn_bwd_dq_kernel', g) == 'attn_bwd_dq_kernel<32, 25, false, 2>'
    assert ops._kname('attn_bwd_dkv_kernel', g) == 'attn_bwd_dkv_kernel<32, 26, false, 2>'
    g = geom((10, 7, 7), (10, 7, 7), 16)
    assert ops._kname('attn_fwd_kernel', g) == 'attn_fwd_kernel<16, 16, false, 2>'
    g = geom((2, 15, 15), (2, 15, 15), 16)                  # parts of 15 tiles run on the 16-tile kernels
    assert ops._kname('attn_bwd_dq_kernel', g) == 'attn_bwd_dq_kernel<16, 16, false, 2>'
    g = geom((8, 7, 7), (8, 7, 7), 32)
    assert ops._kname('attn_fwd_kernel', g) == 'attn_fwd_kernel<32, 25, false, 1>'
    fl, by = ops._attn_work(geom((16, 7, 7), (16, 7, 7), 32, groups=4, nH=3), True)
    assert fl == 10 * 4 * 3 * 784 * 784 * 32 and by == 8 * 4 * 784 * 3 * 32 * 2


def test_module_refuses_an_1152_token_window_by_name():
    attn = WindowAttention3D(64, (8, 12, 12), 2, qkv_bias=True)
    with pytest.raises(NotImplementedError) as e:
        attn.check_window((8, 12, 12))
    msg = str(e.value)
    assert '1024' in msg and '1152' in msg and '(8, 12, 12)' in msg and 'CLV_ERR' not in msg
    with pytest.raises(NotImplementedError, match='1024'):                    # forward: before any kernel (a CPU tensor here)
        attn(torch.zeros(1, 8, 12, 12, 64), (8, 12, 12), (0, 0, 0), None)
    attn.check_window((4, 12, 12))                                            # the same module on a shorter clip: 576 tokens
    blk = SwinTransformerBlock3D(64, 2, window_size=(8, 12, 12))
    with pytest.raises(NotImplementedError, match='1024'):
        blk.attn_part(torch.zeros(1, 8, 12, 12, 64))
    with pytest.raises(NotImplementedError, match='1024'):                    # the op itself, for a direct caller
        ops.window_attention(torch.zeros(1, 8, 12, 12, 192), None, None, (8, 12, 12), (0, 0, 0), 2)
