"""Host side of the shared-prefix attention (no GPU): sd_shared_attn_plan, the plan the launch path uses."""
import ctypes as C

import pytest

from llmspeculativesampling_amd import _lib

lib = _lib.lib


@pytest.mark.parametrize("D,Hq,Hkv", [(128, 40, 40), (128, 64, 8), (64, 8, 2), (128, 8, 1)])
def test_plan_covers_both_key_ranges_within_the_partial_buffer(D, Hq, Hkv):
    for rows, groups in ((2, 2), (15, 4), (80, 16), (80, 32)):
        for P, own in ((1, 1), (65, 75), (577, 9), (3840, 69), (100_000, 20_000)):
            t, ps, pc, ss, sc, lds = [C.c_int() for _ in range(5)] + [C.c_long()]
            _lib.check(lib.sd_shared_attn_plan(D, Hq, Hkv, P, P + own, rows, groups, 256, *(C.byref(x) for x in (t, ps, pc, ss, sc, lds))),
                       "sd_shared_attn_plan")
            t, ps, pc, ss, sc = (x.value for x in (t, ps, pc, ss, sc))
            assert pc % 64 == 0 and sc % 64 == 0 and ps >= 1 and ss >= 1 and groups * (ps + ss) <= 64, (rows, groups, P, own)
            assert (ps - 1) * pc < P <= ps * pc and (ss - 1) * sc < own <= ss * sc          # [0, P) and [P, s_max), no empty split
            assert (t - 1) * 64 < (Hq // Hkv) * rows <= t * 64 and 0 < lds.value <= 160 * 1024
            assert (ps == 1 or pc >= 256) and (ps - 1) * Hkv * t < 256                     # no split under 256 keys or past the CUs
    none = [None] * 6
    for bad in ((32, Hq, Hkv, 64, 70, 2, 2, 0), (D, 16 * Hkv, Hkv, 64, 70, 2, 2, 0), (D, Hq, Hkv, 0, 70, 2, 2, 0),
                (D, Hq, Hkv, 64, 64, 2, 2, 0), (D, Hq, Hkv, 64, 70, 81, 2, 0), (D, Hq, Hkv, 64, 70, 2, 3, 0),
                (D, Hq, Hkv, 64, 70, 40, 33, 0), (D, Hq, Hkv, 64, 70, 2, 2, -1)):
        assert lib.sd_shared_attn_plan(*bad, *none) == _lib.SD_ERR_INVALID and b"sd_shared_attn_plan" in lib.sd_last_error(), bad
