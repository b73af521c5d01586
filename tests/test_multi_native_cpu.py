"""Host-side checks of the native width-w loop: ABI of the new entry points, argument refusal, and the rule that decides
which loop multi_speculative_sampling takes.  No GPU needed."""
import ctypes as C
import re

import pytest


def multi_blocks(lib):
    # the argument blocks of a direct sd_spec_multi_generate call that hands over no buffer at all
    return (lib.SdSampling(temperature=1.0, top_k=0, top_p=0.0, V=128, ld=128, eos_token_id=2),
            lib.SdSpecScratch(max_rows_per_forward=80), lib.SdSeqState(T=10, max_iters=1))


def test_new_symbols_resolve_with_the_declared_argument_types():
    """(Argument counts and classes against the header: test_abi_cpu.py.)"""
    from llmspeculativesampling_amd import _lib
    assert C.sizeof(_lib.SdMultiAdoptItem) == 24 and C.sizeof(_lib.SdMultiReplica) == 40
    assert _lib.lib.sd_spec_multi_block_bytes(4, 4) == C.sizeof(_lib.SdMultiResult) + 4 * 4 * 13
    assert _lib.lib.sd_spec_multi_block_bytes(0, 4) == 0


def test_native_multi_entry_points_refuse_bad_limits_on_the_host():
    from llmspeculativesampling_amd import _lib
    from llmspeculativesampling_amd.sampling import multi
    sampling, scratch, state = multi_blocks(_lib)
    for width, gamma in ((17, 4), (0, 4), (4, 17), (4, 0)):
        rc = _lib.lib.sd_spec_multi_generate(None, width, gamma, 64, sampling, 0, None, scratch, None, None, state, None)
        assert rc == _lib.SD_ERR_INVALID
        assert re.search("width|gamma", _lib.lib.sd_last_error().decode())
        with pytest.raises(_lib.SpecDecError):
            multi._check_native(rc)
        assert _lib.lib.sd_multi_accept_resample(None, width, 128, 128, 3, gamma, None, 0, 0, 0, None, 0, None) == _lib.SD_ERR_INVALID
        assert _lib.lib.sd_multi_adopt(None, width, None, 3, gamma, 0, 0, 1, 8, 16, 1, 8, 16, 32, None) == _lib.SD_ERR_INVALID
    # ranges the device could derive must fit the arenas and the token buffers
    items = (_lib.SdMultiAdoptItem * 2)()
    res = (C.c_char * C.sizeof(_lib.SdMultiResult))()
    assert _lib.lib.sd_multi_adopt(items, 2, C.addressof(res), 6, 4, 5, 5, 1, 8, 16, 1, 16, 16, 32, None) == _lib.SD_ERR_INVALID
    assert "overruns" in _lib.lib.sd_last_error().decode()
    reps = (_lib.SdMultiReplica * 2)()
    for blocks in ((None, scratch, state), (sampling, None, state), (sampling, scratch, None)):   # a null block, limits in range
        assert _lib.lib.sd_spec_multi_generate(reps, 2, 4, 64, blocks[0], 0, None, blocks[1], None, None, blocks[2], None) \
            == _lib.SD_ERR_INVALID
        assert b"sd_spec_multi_generate: null argument" in _lib.lib.sd_last_error()
    multi._check_native(0)


def test_dispatch_rule_of_multi_speculative_sampling(monkeypatch):
    """Device RNG and not verbose take the native loop unless SD_MULTI_NATIVE=0 (read per call); ReplayNoise and the live
    torch generator never do."""
    from llmspeculativesampling_amd import noise
    from llmspeculativesampling_amd.sampling.multi import _takes_native_loop
    monkeypatch.delenv("SD_MULTI_NATIVE", raising=False)
    dev = noise.DeviceNoise(1)
    assert _takes_native_loop(dev, False) and not _takes_native_loop(dev, True)
    assert not _takes_native_loop(noise.ReplayNoise([], "cpu"), False)
    assert not _takes_native_loop(noise.HostTorchNoise("cpu"), False)
    monkeypatch.setenv("SD_MULTI_NATIVE", "0")
    assert not _takes_native_loop(dev, False)
    monkeypatch.setenv("SD_MULTI_NATIVE", "1")
    assert _takes_native_loop(dev, False)
