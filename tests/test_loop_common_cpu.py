"""The host-side steps the four decode-loop wrappers share (sampling/_loop_common.py), each against values written out
by hand.  No GPU needed."""
import importlib
import math

import numpy as np
import pytest
import torch

from llmspeculativesampling_amd import noise
from llmspeculativesampling_amd.sampling import _loop_common as LC

E = 9                                                              # the EOS id of the tables below

# (tokens, eos_token_id, ori_eos_cnt, expected)
EOS_TABLE = [
    ([1, 2, 3, 4], E, 0, [1, 2, 3, 4]),                            # no EOS at all
    ([1, E, 3, E], None, 0, [1, E, 3, E]),                         # eos_token_id=None
    ([E, 1, 2, 3], E, 1, [E, 1, 2, 3]),                            # EOS only in the prompt, ori = 1
    ([E, 1, E, 3], E, 2, [E, 1, E, 3]),                            # EOS only in the prompt, ori = 2
    ([1, 2, 3, E], E, 0, [1, 2, 3, E]),                            # the new EOS as the last token
    ([1, 2, E, 4, 5], E, 0, [1, 2, E]),                            # the new EOS followed by accepted tokens
    ([1, E, 3, E, 5], E, 0, [1, E]),                               # two new EOS in one commit: cut after the first
    ([1, E, 3, E, 5], E, 1, [1, E, 3, E]),                         # ori = 1: the new EOS comes after the old one's index
    ([E, 1, 2, E, E], E, 1, [E, 1, 2, E]),                         # ori = 1 and two new ones
    ([1, 2], E, 3, [1, 2]),                                        # fewer EOS than the prompt had (never cut)
]


@pytest.mark.parametrize("tokens,eos,ori,want", EOS_TABLE)
def test_cut_after_new_eos_hand_table(tokens, eos, ori, want):
    before = list(tokens)
    got = LC.cut_after_new_eos(tokens, eos, ori)
    assert got == want and isinstance(got, list) and tokens == before
    # the wrappers' loops break on "a new EOS was produced", which they read off the identity of the result
    new_eos = eos is not None and tokens.count(eos) > ori
    assert (got is tokens) == (not new_eos)


def test_cut_after_new_eos_with_the_new_eos_before_the_old_ones_index():
    """ori = 1 counts EOS, not positions: when the sequence has its first EOS earlier than the prompt's one sat (a caller
    that passes a count taken from another prefix), the cut still falls after EOS number ori + 1."""
    assert LC.cut_after_new_eos([E, 1, E, 2], E, 1) == [E, 1, E]
    assert LC.cut_after_new_eos([1, E, E, 2], E, 1) == [1, E, E]


def _reference_eos_rule(tokens, eos, ori):
    """Reference speculative_sampling.py:2033-2041 restated on a numpy row: keep while the running EOS count is below
    ori + 1, plus the one position after that (the new EOS itself)."""
    hit = np.asarray(tokens) == eos
    if int(hit.sum()) <= ori:
        return list(tokens)
    return list(tokens[:int((np.cumsum(hit) < ori + 1).sum()) + 1])


def test_cut_after_new_eos_equals_the_reference_rule_on_random_lists():
    rng = np.random.default_rng(2033)
    cut = 0
    for _ in range(200):
        tokens = rng.integers(0, 4, size=int(rng.integers(1, 41))).tolist()
        eos = int(rng.integers(0, 4))
        ori = tokens[:int(rng.integers(0, len(tokens) + 1))].count(eos)       # as a prompt that is a prefix would give
        want = _reference_eos_rule(tokens, eos, ori)
        assert LC.cut_after_new_eos(tokens, eos, ori) == want, (tokens, eos, ori)
        cut += len(want) < len(tokens)
    assert 50 < cut < 200                                                      # both outcomes really occur


def test_reseed_uniforms():
    assert LC.reseed_uniforms(0, 4, "cpu") is None and LC.reseed_uniforms(None, 4, "cpu") is None
    state = torch.get_rng_state()
    r = LC.reseed_uniforms(42, 5, "cpu")
    assert torch.equal(torch.get_rng_state(), state)               # the global generator is not touched
    want = torch.rand(1, generator=torch.Generator().manual_seed(42))
    assert r.shape == (5,) and r.dtype == torch.float32 and r.device.type == "cpu"
    assert torch.equal(r, want.repeat(5))
    assert torch.equal(LC.reseed_uniforms(42, 1, "cpu"), want)     # one draw, whatever n is
    assert not torch.equal(LC.reseed_uniforms(43, 1, "cpu"), want)


THIRD, SEVEN_TENTHS = np.float32(1 / 3), np.float32(0.7)


def test_accept_rates_f64_hand_table():
    """min(1, p / q) in float64 on float32 inputs (reference :1966-1971).  0 / 0 is nan and p / 0 clamps to 1: that is what
    the loops have always reported for a slot the scan never reached, and it stays."""
    p = np.array([0.5, 0.25, 0.25, 0.0, THIRD, 0.5], dtype=np.float32)
    q = np.array([0.25, 0.25, 0.5, 0.0, SEVEN_TENTHS, 0.0], dtype=np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        got = LC.accept_rates_f64(p, q)
    assert isinstance(got, list) and all(type(x) is float for x in got)
    assert got[:3] == [1.0, 1.0, 0.5] and math.isnan(got[3]) and got[5] == 1.0
    assert got[4] == float(THIRD) / float(SEVEN_TENTHS)             # the double quotient of the two float32 values
    assert type(np.mean(got)) is np.float64


def test_accept_rates_f32_zero_q_hand_table():
    """The width-w loop's form (reference :1597): the quotient is taken in float32, a ratio above 1 becomes the int 1, a
    zero q the int 0 (also for 0 / 0); everything else is the float32 quotient as a Python float."""
    p = np.array([0.5, 0.25, 0.25, 0.0, THIRD, 0.5], dtype=np.float32)
    q = np.array([0.25, 0.25, 0.5, 0.0, SEVEN_TENTHS, 0.0], dtype=np.float32)
    got = LC.accept_rates_f32_zero_q(p, q)
    assert isinstance(got, list) and [type(x) for x in got] == [int, float, float, int, float, int]
    assert got[:4] == [1, 1.0, 0.5, 0] and got[5] == 0
    f32_quotient = float(THIRD / SEVEN_TENTHS)
    assert got[4] == f32_quotient and f32_quotient != float(THIRD) / float(SEVEN_TENTHS)
    # a (replicas, gamma) block is read replica by replica
    assert LC.accept_rates_f32_zero_q(p.reshape(2, 3), q.reshape(2, 3)) == got
    assert LC.accept_rates_f32_zero_q(p[:0], q[:0]) == []


@pytest.mark.parametrize("q_fill,timed", [(1.0, True), (0.0, False)], ids=["ones_timed", "zeros_untimed"])
def test_loop_log_arrays_and_slices(q_fill, timed):
    log = LC.LoopLog([5, 6, 7], 12, 4, 3, q_fill=q_fill, timed=timed)
    assert log.host_seq.dtype == np.int32 and log.host_seq.tolist() == [5, 6, 7] + [0] * 9
    assert log.acc.dtype == np.int32 and log.acc.tolist() == [0] * 4
    assert log.p_at.dtype == np.float32 and log.p_at.tolist() == [0.0] * 12
    assert log.q_at.dtype == np.float32 and log.q_at.tolist() == [q_fill] * 12
    ptrs = log.ptrs()
    assert ptrs[:3] == (log.acc.ctypes.data, log.p_at.ctypes.data, log.q_at.ctypes.data) and len(ptrs) == 5
    if timed:
        assert log.draft_ms.dtype == log.target_ms.dtype == np.float32 and log.draft_ms.shape == log.target_ms.shape == (4,)
        assert ptrs[3:] == (log.draft_ms.ctypes.data, log.target_ms.ctypes.data)
    else:
        assert log.draft_ms is None and log.target_ms is None and ptrs[3:] == (None, None)
        assert log.phase_ns(3) == (0, 0)
    st = log.seq_state(3, 9, 1, (2, 1), noise.DeviceNoise(7), 4)   # the sequence's sd_seq_state: state in, this log's arrays out
    assert (st.host_seq, st.len, st.T, st.ori_eos_cnt, st.draft_len, st.target_len, st.seed, st.draw, st.max_iters, st.n_iters, st.err) \
        == (log.host_seq.ctypes.data, 3, 9, 1, 2, 1, 7, 0, 4, 0, 0)
    assert (st.acc_len_out, st.p_at_out, st.q_at_out, st.draft_ms_out, st.target_ms_out) == ptrs
    # what a native loop would leave after two iterations
    log.host_seq[3:8] = [8, 9, 10, 11, 12]
    log.acc[:2] = [3, 1]
    log.p_at[:6] = np.arange(6)
    log.q_at[:6] = 2.0
    assert log.tokens(8) == [5, 6, 7, 8, 9, 10, 11, 12] and all(type(t) is int for t in log.tokens(8))
    assert log.acc_len(2) == [3, 1] and log.acc_len(0) == []
    pa, qa = log.ratios(2)
    assert pa.tolist() == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0] and qa.tolist() == [2.0] * 6
    assert [a.size for a in log.ratios(4)] == [12, 12] and [a.size for a in log.ratios(0)] == [0, 0]
    assert log.ratios(3)[1].tolist() == [2.0] * 6 + [q_fill] * 3   # slots no iteration wrote keep the fill value


def test_loop_log_phase_ns_truncates_every_entry_before_summing():
    log = LC.LoopLog([1], 4, 3, 2, q_fill=1.0, timed=True)
    log.draft_ms[:] = [0.0000019, 0.0000019, 5.0]                   # 1.9 ns -> 1 ns each; summed first they would give 3
    log.target_ms[:] = [1.5, 0.25, 7.0]
    assert log.phase_ns(2) == (2, 1_750_000) and log.phase_ns(3) == (5_000_002, 8_750_000)
    assert log.phase_ns(0) == (0, 0) and all(type(v) is int for v in log.phase_ns(3))


def test_sampling_block_writes_the_conventions_once():
    for args, want in (((1, None, None, 128, 160, None), (1.0, 0, 0.0, 128, 160, -1)), ((0.5, 20, 0.5, 8, 8, 0), (0.5, 20, 0.5, 8, 8, 0))):
        s = LC.sampling_block(*args)                               # None: that filter is off / there is no EOS; token 0 is an EOS
        assert (s.temperature, s.top_k, s.top_p, s.V, s.ld, s.eos_token_id) == want


def test_spec_stream_and_bind_spec_slot_fill_the_same_eight_fields():
    """The device side of one speculative stream, from two stand-in KVCacheModels (a session handle and a probability arena each)."""
    from types import SimpleNamespace as NS
    from llmspeculativesampling_amd import _lib
    draft = NS(_session=NS(handle=0x1100), _probs=torch.zeros(4, 8))
    target = NS(_session=NS(handle=0x2200), _probs=torch.zeros(4, 8))
    seq32, err = torch.zeros(6, dtype=torch.int32), torch.zeros(13, dtype=torch.int32)
    want = (0x1100, 0x2200, seq32.data_ptr(), draft._probs.data_ptr(), target._probs.data_ptr(), err.data_ptr(), 0x3300, 0x4400)
    fields = ["draft", "target", "seq", "q_hist", "p_hist", "err_words", "res_dev", "res_host"]
    dev = LC.spec_stream(draft, target, seq32, err, 0x3300, 0x4400)
    assert type(dev) is _lib.SdSpecStream and tuple(getattr(dev, f) for f in fields) == want
    item = _lib.SdBatchStream(len=5, T=9)                            # the slot's own fields stay as they are
    LC.bind_spec_slot(item, draft, target, seq32, err, 0x3300, 0x4400)
    assert tuple(getattr(item, f) for f in fields) == want and (item.len, item.T, item.host_seq) == (5, 9, None)


def test_raise_loop_error_texts():
    LC.raise_loop_error(0)
    with pytest.raises(RuntimeError, match="^prob error$"):
        LC.raise_loop_error(1)
    with pytest.raises(RuntimeError, match="^norm logits error$"):
        LC.raise_loop_error(2)


def test_details_dict_keys_and_order():
    seven = ["approx_time", "target_time", "other_time", "acc_len", "acc_rate", "target_call_times", "approx_call_times"]
    d = LC.details_dict(1, 2, 3, [4], 0.5, 6, 7)
    assert list(d) == seven and list(d.values()) == [1, 2, 3, [4], 0.5, 6, 7]
    d = LC.details_dict(1, 2, 3, [4], 0.5, 6, 7, target_model_time=8, target_pre_cache_time=9, target_post_prob_time=10)
    assert list(d) == seven + ["target_model_time", "target_pre_cache_time", "target_post_prob_time"]
    assert (d["target_model_time"], d["target_pre_cache_time"], d["target_post_prob_time"]) == (8, 9, 10)


def test_make_noise_kinds_and_the_alias():
    ss = importlib.import_module("llmspeculativesampling_amd.sampling.speculative_sampling")   # (the package exports the function)
    assert ss._make_noise is LC.make_noise
    assert type(LC.make_noise(None, "cpu")) is noise.HostTorchNoise and type(LC.make_noise("host", "cpu")) is noise.HostTorchNoise
    dev = LC.make_noise("device", "cpu")
    assert type(dev) is noise.DeviceNoise and dev.seed == int(torch.initial_seed()) and dev.on_device
    mine = noise.ReplayNoise([], "cpu")
    assert LC.make_noise(mine, "cpu") is mine
