"""Host-side checks of the native width-w loop: ABI of the new entry points, argument refusal, and the rule that decides
which loop multi_speculative_sampling takes.  No GPU needed."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sd_multi_accept_resample", "sd_multi_adopt", "sd_spec_multi_block_bytes", "sd_spec_multi_generate"]


def _declared_arg_count(name):
    hdr = open(os.path.join(ROOT, "include", "specdec.h")).read()
    m = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, name
    return len([a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()])


def test_new_symbols_resolve_with_the_declared_argument_types():
    from llmspeculativesampling_amd import _lib
    bound = {n: (res, args) for n, res, args in _lib.SYMBOLS}
    for name in NEW:
        fn = getattr(_lib.lib, name)
        res, args = bound[name]
        assert fn.restype is res and list(fn.argtypes) == list(args)
        assert len(args) == _declared_arg_count(name), name
    assert C.sizeof(_lib.SdMultiAdoptItem) == 24 and C.sizeof(_lib.SdMultiReplica) == 40
    assert _lib.lib.sd_spec_multi_block_bytes(4, 4) == C.sizeof(_lib.SdMultiResult) + 4 * 4 * 13
    assert _lib.lib.sd_spec_multi_block_bytes(0, 4) == 0


def test_native_multi_entry_points_refuse_bad_limits_on_the_host():
    from llmspeculativesampling_amd import _lib
    from llmspeculativesampling_amd.sampling import multi
    for width, gamma in ((17, 4), (0, 4), (4, 17), (4, 0)):
        rc = _lib.lib.sd_spec_multi_generate(None, width, gamma, 1.0, 0, 0.0, 128, 128, 64, 0, 0, None, 0, None, 0, None, 80,
                                             None, None, None, None, 10, 2, 0, None, None, 0, None, None, None, 1, None, None,
                                             None, None, None, None, None, None)
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
