"""Host-side checks of the native single-stream loop (sd_spec_generate): its refusals, in the order include/specdec.h gives
them, each before anything is written, launched or a session dereferenced.  Placeholder pointers, no GPU needed.  (The ABI of
the entry and of sd_spec_stream: test_abi_cpu.py.)"""
import ctypes as C

import pytest

from llmspeculativesampling_amd import _lib

P = 0x1000                                                        # a placeholder pointer: every refusal comes before any use
STREAM_FIELDS = [f for f, _ in _lib.SdSpecStream._fields_]


def _blocks(gamma_rows=5):
    """Blocks that pass every refusal a placeholder can reach (gamma 4: a workspace of 5 rows holds the target's lists)."""
    dev = _lib.SdSpecStream(*[P] * 8)
    sampling = _lib.SdSampling(temperature=1.0, top_k=20, top_p=0.9, V=128, ld=128, eos_token_id=2)
    scratch = _lib.SdSpecScratch(_lib.SdHeadScratch(P, 128, 0), _lib.SdHeadScratch(P, 128, 0), P, gamma_rows)
    seq = _lib.SdSeqState(host_seq=P, len=9, T=12, max_iters=3, n_iters=-7, err=-7)
    return dev, sampling, scratch, seq


def _refused(text, dev, gamma, sampling, scratch, seq, random_seed=0, r_const=None, opts=None):
    lib = _lib.lib
    assert lib.sd_spec_generate(dev, gamma, sampling, scratch, seq, random_seed, r_const, None, opts) == _lib.SD_ERR_INVALID
    msg = lib.sd_last_error().decode()
    assert msg.startswith("sd_spec_generate:") and text in msg, msg


def test_spec_generate_refuses_a_null_block_or_pointer():
    dev, sampling, scratch, seq = _blocks()
    for i in range(4):                                            # each of the four blocks
        args = [dev, sampling, scratch, seq]
        args[i] = None
        _refused("null argument", args[0], 4, *args[1:])
    for f in STREAM_FIELDS:                                       # each pointer of the stream block
        d2 = _lib.SdSpecStream(*[P] * 8)
        setattr(d2, f, None)
        _refused("null argument", d2, 4, sampling, scratch, seq)
    for side in ("draft", "target"):                              # either head's logit rows
        _, _, s2, _ = _blocks()
        getattr(s2, side).logits = None
        _refused("null argument", dev, 4, sampling, s2, seq)
    q2 = _lib.SdSeqState(host_seq=None, len=9, T=12, max_iters=3, n_iters=-7, err=-7)
    _refused("null argument", dev, 4, sampling, scratch, q2)
    assert (seq.n_iters, seq.err, seq.len) == (-7, -7, 9) and (q2.n_iters, q2.err, q2.len) == (-7, -7, 9)


def test_spec_generate_refusals_come_in_the_documented_order():
    """A call that breaks every rule is refused for the first; mended rule by rule, it is refused for the next one.  The last
    rule, V against the models' vocabularies, reads the sessions and is left to the GPU tests."""
    dev, sampling, scratch, seq = _blocks(gamma_rows=4)           # (a workspace of 4 rows: one short of gamma 4 + 1)
    sampling.temperature = 0.0
    null_dev = _lib.SdSpecStream(*[P] * 8)
    null_dev.res_host = None
    _refused("null argument", null_dev, 17, sampling, scratch, seq, random_seed=5)
    for gamma in (17, 0, -1):
        _refused(f"gamma {gamma} outside 1..16", dev, gamma, sampling, scratch, seq, random_seed=5)
    _refused("random_seed needs its uniform (r_const)", dev, 4, sampling, scratch, seq, random_seed=5)
    _refused("temperature must be non-zero", dev, 4, sampling, scratch, seq, random_seed=5, r_const=P)
    _refused("temperature must be non-zero", dev, 4, sampling, scratch, seq)
    sampling.temperature = 0.5
    _refused("workspace of 4 rows", dev, 4, sampling, scratch, seq)
    _refused("workspace of 4 rows", dev, 16, sampling, scratch, seq)
    # the entry's own refusals come before anything in opts, and an empty block is a NULL one
    bad = _lib.SdLoopOpts(row_params=(_lib.SdRowSampling * 1)(), logprobs=C.pointer(_lib.SdLogprobBlock()))
    for opts in (bad, _lib.SdLoopOpts()):
        _refused("gamma 17 outside 1..16", dev, 17, sampling, scratch, seq, opts=opts)
        _refused("workspace of 4 rows", dev, 4, sampling, scratch, seq, opts=opts)
    assert (seq.n_iters, seq.err, seq.len) == (-7, -7, 9)         # nothing was written, nothing ran
    with pytest.raises(ValueError, match="sd_spec_generate"):
        _lib.check(_lib.SD_ERR_INVALID, "sd_spec_generate")


def test_spec_stream_is_the_head_of_a_batch_stream():
    assert _lib.SdBatchStream._fields_[:8] == _lib.SdSpecStream._fields_ and C.sizeof(_lib.SdSpecStream) == 64
