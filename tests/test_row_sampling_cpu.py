"""Per-request temperature / top_k / top_p in the lock-step loops: what needs no GPU - the ABI (two symbols, one struct; the
loops take the array as member row_params of sd_loop_opts), the refusals of sd_norm_batch_rows and the argument checks of the three Python entries."""
import ctypes as C

import pytest
import torch

import abi_header
from llmspeculativesampling_amd import _lib
from llmspeculativesampling_amd.sampling import (speculative_sampling_batch, speculative_sampling_queue,
                                                 speculative_sampling_queue_shared)

NEW = ("sd_norm_batch_rows", "sd_norm_batch_rows_debug")
REMOVED = ("sd_spec_batch_generate_rows", "sd_spec_queue_generate_rows")      # ABI 7: member row_params of sd_loop_opts
SYM = {name: (res, args) for name, res, args in _lib.SYMBOLS}


def test_new_symbols_are_exported_and_bound():
    for name in NEW:
        assert name in SYM, name
        assert SYM[name][0] is C.c_int
        fn = getattr(_lib.lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == list(SYM[name][1])
    protos, raw = abi_header.parse()[0], C.CDLL(_lib.LIB_PATH)
    for name in REMOVED:
        assert name not in protos and name not in SYM and not hasattr(raw, name), name


def test_row_sampling_struct_and_version():
    assert _lib.C_STRUCTS["sd_row_sampling"] is _lib.SdRowSampling
    assert C.sizeof(_lib.SdRowSampling) == 12
    assert [n for n, _ in _lib.SdRowSampling._fields_] == ["temperature", "top_k", "top_p"]
    assert _lib.lib.sd_version() == 7


def _norm_rows(params, n):
    """sd_norm_batch_rows on host memory: every refusal comes before a launch, so no GPU is needed."""
    buf = (C.c_float * 64)()
    rows = (_lib.SdNormRow * n)()
    for r in rows:
        r.probs_out = C.addressof(buf)
    _lib.check(_lib.lib.sd_norm_batch_rows(C.addressof(buf), n, 8, 8, params, 0, rows, 0, None, None), "sd_norm_batch_rows")


def test_norm_batch_rows_refusals_do_not_need_a_gpu():
    R = _lib.SdRowSampling
    with pytest.raises(ValueError, match="params"):
        _norm_rows(None, 3)
    with pytest.raises(ValueError, match=r"row 1: temperature"):
        _norm_rows((R * 3)(R(1.0, 0, 0.0), R(0.0, 0, 0.0), R(1.0, 0, 0.0)), 3)
    with pytest.raises(ValueError, match=r"row 2: top_k -1"):
        _norm_rows((R * 3)(R(1.0, 0, 0.0), R(1.0, 5, 0.0), R(1.0, -1, 0.0)), 3)


PROMPTS = [torch.ones((1, 3), dtype=torch.int64) for _ in range(3)]
ENTRIES = [(speculative_sampling_queue, {}), (speculative_sampling_queue_shared, {"shared_prefix": 2}),
           (speculative_sampling_batch, {})]


@pytest.mark.parametrize("fn,more", ENTRIES, ids=["queue", "queue_shared", "batch"])
@pytest.mark.parametrize("name,value", [
    ("temperature", [1.0, 0.7]), ("top_k", [20, 0, 1, 5]), ("top_p", [0.9]),                 # 3 prompts, other lengths
    ("temperature", [1.0, 0, 0.7]), ("temperature", [1.0, 0.0, 0.7]),                      # a zero temperature
    ("top_k", [20, -1, 0]), ("top_k", [20, 2.5, 0]),                                        # negative / non-integer top_k
], ids=["T_len", "k_len", "p_len", "T_zero_int", "T_zero", "k_negative", "k_fraction"])
def test_bad_sequences_raise_before_a_model_is_touched(fn, more, name, value):
    # None models: anything that reached as_specdec_model would raise TypeError instead
    with pytest.raises(ValueError, match=name):
        fn(PROMPTS, None, None, -1, None, 4, **{name: value}, **more)


@pytest.mark.parametrize("fn,more", ENTRIES, ids=["queue", "queue_shared", "batch"])
def test_good_sequences_reach_the_models(fn, more):
    # the checks pass (scalars and sequences mixed, tuples and tensors count as sequences): the call gets as far as the models
    with pytest.raises(TypeError):
        fn(PROMPTS, None, None, -1, None, 4, temperature=(1.0, 0.7, -1.0), top_k=torch.tensor([20, 0, 65]), top_p=0.9, **more)
