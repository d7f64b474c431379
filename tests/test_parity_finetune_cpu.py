"""The fp32-storage QA entry points of parity mode on the host side (no GPU): both builds of the library export them,
the ctypes table binds them with their 16-bit counterparts' argument lists, and the ABI version did not move."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_ENTRIES = {'clv_qa_head_f32_fwd': 'clv_qa_head_fwd', 'clv_qa_head_f32_bwd': 'clv_qa_head_bwd',
               'clv_attn_probs_mean_f32': 'clv_attn_probs_mean', 'clv_qa_choice_assemble_f32': 'clv_qa_choice_assemble',
               'clv_qa_choice_assemble_f32_bwd': 'clv_qa_choice_assemble_bwd'}


@pytest.mark.parametrize('fname', ['libclover_hip_f16.so', 'libclover_hip.so'])
def test_both_builds_export_the_f32_qa_entries(fname):
    so = ctypes.CDLL(os.path.join(ROOT, 'clover_amd', fname))
    for sym in F32_ENTRIES:
        assert hasattr(so, sym), (fname, sym)
    assert so.clv_abi_version() == 20


def test_lib_binds_the_f32_qa_entries_like_their_16_bit_counterparts():
    from clover_amd import _lib
    assert _lib.ABI_VERSION == 20
    for sym, twin in F32_ENTRIES.items():
        assert _lib.SIGNATURES[sym] == _lib.SIGNATURES[twin], sym
        fn = getattr(_lib.lib(), sym)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == list(_lib.SIGNATURES[sym][1])
    assert _lib.lib().clv_abi_version() == 20


def test_entry_selection_is_by_mode_and_dtype():
    """ops._qa_entry: the 16-bit entry outside parity mode, the _f32 one inside it, a raise on a mismatch."""
    import torch
    from clover_amd import ops, parity
    half, f32 = torch.empty(1, dtype=ops.BF16), torch.empty(1, dtype=torch.float32)
    names = list(F32_ENTRIES.values())
    assert [ops._qa_entry(n, half, 'x')[1] for n in names] == list(F32_ENTRIES.values())
    with pytest.raises(NotImplementedError):
        ops._qa_entry('clv_qa_head_fwd', f32, 'x')
    with parity.mode():
        assert [ops._qa_entry(n, f32, 'x')[1] for n in names] == list(F32_ENTRIES)
        with pytest.raises(NotImplementedError):
            ops._qa_entry('clv_qa_head_fwd', half, 'x')
