"""Host-side checks of the prompt queue's shared prompt prefix (speculative_sampling_queue_shared(shared_prefix=P),
sd_spec_queue_generate's donors, sd_session_copy_kv): the argument is refused before a model is built, the new symbols and
the copy item's layout match the header, and the native entry points refuse what needs no GPU to refuse.  No GPU needed."""
import ctypes as C
import re

import pytest
import torch

from test_spec_queue_cpu import queue_blocks

P = 5


def _prompts(lens=(5, 9, 7, 12)):
    """Prompts that share their first P tokens and differ behind them."""
    head = torch.arange(10, 10 + P, dtype=torch.int64)
    return [torch.cat([head[:L], torch.full((max(L - P, 0),), 100 + i, dtype=torch.int64)]).unsqueeze(0) for i, L in enumerate(lens)]


def _q(prefixes, **kw):
    """The models are None: anything that reached as_specdec_model raises TypeError, not ValueError."""
    import llmspeculativesampling_amd.sampling as S
    return S.speculative_sampling_queue_shared(prefixes, None, None, 2, None, 4, **kw)


def test_the_shared_queue_is_the_queue_plus_one_keyword():
    """speculative_sampling_queue keeps its parameter list; the shared entry point has the same one, then shared_prefix=0."""
    import inspect
    import llmspeculativesampling_amd.sampling as S
    assert callable(S.speculative_sampling_queue_shared) and "speculative_sampling_queue_shared" in S.__all__
    plain = inspect.signature(S.speculative_sampling_queue).parameters
    shared = inspect.signature(S.speculative_sampling_queue_shared).parameters
    assert "shared_prefix" not in plain
    assert list(shared) == list(plain) + ["shared_prefix"] and shared["shared_prefix"].default == 0
    assert all(shared[k].default == plain[k].default and shared[k].kind == plain[k].kind for k in plain)
    with pytest.raises(TypeError, match="shared_prefix"):         # the plain queue does not take the keyword
        S.speculative_sampling_queue(_prompts(), None, None, 2, None, 4, shared_prefix=P)


@pytest.mark.parametrize("bad", [True, False, -1, 2.0, 5.0, None, "5"], ids=repr)
def test_shared_prefix_must_be_a_non_bool_int_of_at_least_zero(bad):
    with pytest.raises(ValueError, match="shared_prefix"):
        _q(_prompts(), shared_prefix=bad)


def test_shared_prefix_longer_than_the_shortest_prompt_is_refused():
    with pytest.raises(ValueError, match=r"shared_prefix: 6 tokens, but the shortest prompt has 5"):
        _q(_prompts(), shared_prefix=P + 1)


def test_a_differing_token_is_named_by_prompt_and_position():
    ps = _prompts()
    ps[2][0, P - 1] += 1
    ps[3][0, 1] += 1                                              # (a later prompt differs earlier: the FIRST prompt is named)
    with pytest.raises(ValueError, match=rf"shared_prefix: prompt 2 differs from prompt 0 at position {P - 1}\b"):
        _q(ps, shared_prefix=P)
    ps[2][0, 0] += 1                                              # the first position of several that differ
    with pytest.raises(ValueError, match=r"prompt 2 differs from prompt 0 at position 0\b"):
        _q(ps, shared_prefix=P)
    with pytest.raises(TypeError):                                # behind the prefix the prompts may differ: prompts 0 .. 1 pass
        _q(ps[:2], shared_prefix=P)


def test_the_edge_shared_prefix_equal_to_the_shortest_prompt_is_accepted():
    with pytest.raises(TypeError):                                # well-formed: the call reaches the models
        _q(_prompts(), shared_prefix=P)
    with pytest.raises(TypeError):
        _q(_prompts(), shared_prefix=0)
    with pytest.raises(TypeError):
        _q(_prompts((1, 1)), shared_prefix=1)                     # one-token prompts: nothing can be shared, nothing is wrong


def test_the_other_checks_still_come_first():
    with pytest.raises(ValueError, match="slots"):
        _q(_prompts(), shared_prefix=-1, slots=0)
    with pytest.raises(ValueError, match=r"prefixes\[1\]"):
        _q([_prompts()[0], torch.ones(3, dtype=torch.int64)], shared_prefix=2)


# ----------------------------------------------------------------------------- ABI
def test_new_symbols_are_exported_and_declared():
    from llmspeculativesampling_amd import _lib
    bound = {n: (res, args) for n, res, args in _lib.SYMBOLS}
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("sd_session_copy_kv", "sd_spec_queue_generate"):
        assert hasattr(raw, name) and bound[name][0] is C.c_int, name
    # ABI 7: the queue has one entry, which takes the two donors and the row count ahead of its sd_loop_opts
    # (test_abi_cpu.py has the whole list)
    assert "sd_spec_queue_generate_shared" not in bound and not hasattr(raw, "sd_spec_queue_generate_shared")
    assert list(bound["sd_spec_queue_generate"][1][-4:]) == [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(_lib.SdLoopOpts)]


def test_copy_item_layout_matches_the_header():
    from llmspeculativesampling_amd import _lib
    assert [f for f, _ in _lib.SdKvCopyItem._fields_] == ["dst", "lo", "hi"]
    assert (_lib.SdKvCopyItem.lo.offset, _lib.SdKvCopyItem.hi.offset, C.sizeof(_lib.SdKvCopyItem)) == (8, 12, 16)


def test_copy_kv_refuses_null_arguments_and_item_counts_without_a_gpu():
    from llmspeculativesampling_amd import _lib
    lib = _lib.lib
    items = (_lib.SdKvCopyItem * 17)()
    fake = C.addressof((C.c_char * 64)())                         # never read: the count is checked before any item
    assert lib.sd_session_copy_kv(None, items, 1, None) == _lib.SD_ERR_INVALID and b"null argument" in lib.sd_last_error()
    assert lib.sd_session_copy_kv(fake, None, 1, None) == _lib.SD_ERR_INVALID and b"null argument" in lib.sd_last_error()
    for n in (0, 17, -1):
        assert lib.sd_session_copy_kv(fake, items, n, None) == _lib.SD_ERR_INVALID
        assert re.search(r"n_items -?\d+ outside 1\.\.16", lib.sd_last_error().decode())
    with pytest.raises(ValueError, match="sd_session_copy_kv"):
        _lib.check(_lib.SD_ERR_INVALID, "sd_session_copy_kv")


def test_shared_entry_point_refuses_bad_arguments_before_any_launch():
    from llmspeculativesampling_amd import _lib
    lib = _lib.lib
    buf = (C.c_char * 256)()
    p = C.addressof(buf)
    sampling, scratch, log = queue_blocks(p)
    slots = (_lib.SdBatchStream * 2)()
    prompts = (_lib.SdQueuePrompt * 2)()

    def call(donor_draft=None, donor_target=None, rows=0, n_slots=2, lg=log):
        return lib.sd_spec_queue_generate(slots, n_slots, 64, prompts, 2, 0, 4, sampling, 0, None, scratch, lg, None, None,
                                          donor_draft, donor_target, rows, None)

    for args in ((None, None, 3), (p, None, 3), (None, p, 3), (p, p, 0), (None, None, -1)):
        assert call(*args) == _lib.SD_ERR_INVALID
        assert re.search(r"sd_spec_queue_generate: shared_rows -?\d+ needs both donor sessions", lib.sd_last_error().decode())
    assert call(n_slots=17) == _lib.SD_ERR_INVALID and b"sd_spec_queue_generate: n_slots 17" in lib.sd_last_error()
    # without donors the checks are the same, under the same name
    assert call() == _lib.SD_ERR_INVALID and b"sd_spec_queue_generate: slot 0: null pointer" in lib.sd_last_error()
    assert call(lg=None) == _lib.SD_ERR_INVALID and b"sd_spec_queue_generate: null argument" in lib.sd_last_error()
    assert (log.n_iters, log.err) == (-7, -7)                     # nothing was written, nothing ran
