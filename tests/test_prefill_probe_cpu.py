"""The layouts of tests/prefill_probe_layouts.py, checked on the oracle alone (no GPU), the way test_attn_probe_cpu.py
checks attn_probe's: for each of the (model, dtype, arena) cases that test_gpu_prefill_attention_variants.py runs, the
same-dtype oracle (with the fp8 arena: models_ref._kv_fp8's emulation, the arena's scales folded in) is finite and passes the
GPU test's 1.5x rule against the fp32 oracle by itself, and losing the marker - or leaking a forbidden one into the probed
row - moves that row's fp32 logits by at least 20x the GPU test's tolerance.  20x is the condition of test_attn_probe_cpu.py,
not a fit (the measured figures are printed)."""
import functools

import pytest

import attn_probe as P
import prefill_probe_layouts as L
from prefill_probe_layouts import wide_models  # noqa: F401  (fixture)
from test_attn_probe_cpu import _check

pytestmark = pytest.mark.usefixtures("wide_models")


@functools.lru_cache(maxsize=None)
def _oracle(name, dt, kvq=None):
    return P.ProbeOracle(name, P.DTYPES[dt], kvq)


def test_layout_table():
    lays = L.layouts()
    assert len(lays) == 58 and len(set(lays)) == 58
    assert all(0 <= l.marker <= l.S and l.n - L.TAIL <= l.probe < l.n for l in lays)
    assert {(l.n, l.S - l.n) for l in L.edge_layouts()} == set(L.EDGE_CALLS)
    for n, pos0 in L.EDGE_CALLS:
        mine = [l for l in L.edge_layouts() if (l.n, l.S - l.n) == (n, pos0)]
        assert {l.marker for l in mine if l.cls == "chunk_edge"} == {k for k in L.V_CHUNK_EDGES if k < pos0 + n}
        assert {l.probe for l in mine if l.cls == "own"} == {n - 64, n - 17, n - 16, n - 1}
        assert {l.probe for l in mine if l.cls == "forbidden"} == {n - 64, n - 17, n - 16}
        assert all(l.marker == pos0 + l.probe + (l.cls == "forbidden") for l in mine if l.cls != "chunk_edge")


@pytest.mark.parametrize("name,dt,kvq", L.CASES, ids=L.CASE_IDS)
def test_prefill_layouts_discriminate_and_the_reference_alone_passes(name, dt, kvq):
    o32, o16 = _oracle(name, "fp32"), _oracle(name, dt, kvq)
    worst, e_max = float("inf"), 0.0
    for lay in L.layouts():
        r, e = _check(o32, o16, lay, P.discrimination, lambda o, l: o.logits(l))
        worst, e_max = min(worst, r), max(e_max, e)
    print(f"prefill variants {name} {dt} {kvq}: {len(L.layouts())} layouts, least discrimination {worst:.1f}x the tolerance, "
          f"reference error at most {e_max:.4f}")
    assert worst >= 20.0


def test_batched_prefill_streams_discriminate_a_foreign_scale_pointer():
    """The batched-prefill case of the GPU file (prefill_probe_layouts.batch_model: two layers, three streams, the second
    with K's and V's scales swapped): each stream's reference passes the 1.5x rule on the row fed after the prefill, and a
    prefill attention that multiplied by a NEIGHBOUR stream's scales - the arena rows stored with the stream's own (k_proj /
    v_proj folded with them), scores and output scaled with the other's (q_proj / o_proj), on the prefill rows only - moves
    that row's logits by d >= 4x the GPU test's tolerance.  Why 4: such a kernel's row lies d from the correct evaluation, which
    itself lies within the tolerance of the truth, so its error is at least d - tol; it fails the GPU test for certain once
    d > 2 tol, and 4 leaves a factor of two (random weights: no planted marker concentrates the row, so the planted
    layouts' 20x is not to be had here; measured on the oracle: 9.9x at the least)."""
    import oracle
    from test_gpu_production_parity import _assert_within_reference_error
    cfg, sd, ids = L.batch_model()
    o32 = oracle.RefCausalLM(cfg, sd)
    for i, n in enumerate(L.BATCH_ROWS):
        own = L.fold_scales(cfg, sd, L.stream_scales(i, cfg))
        other = L.fold_scales(cfg, sd, L.stream_scales(1 if i != 1 else 0, cfg))
        mixed = dict(own)
        for k in other:
            if "q_proj" in k or "o_proj" in k:
                mixed[k] = other[k]
        truth = o32(ids[i]).logits.float()[0, n:]
        o16 = oracle.RefCausalLM(cfg, P.cast_sd(own, P.DTYPES["bf16"]), kv_quant="fp8")
        ref16 = o16(ids[i]).logits.float()[0, n:]
        errs = P.errors(ref16, ref16, truth)
        _assert_within_reference_error(errs, f"stream {i}")
        right = oracle.RefCausalLM(cfg, own, kv_quant="fp8")
        wrong = oracle.RefCausalLM(cfg, mixed, kv_quant="fp8")
        good = right(ids[i]).logits.float()[0, n:]
        bad = right(ids[i][:, n:], past_key_values=wrong(ids[i][:, :n]).past_key_values).logits.float()[0]
        d = float((bad - good).abs().max())
        print(f"stream {i}: reference error {errs[1]:.4f}, a foreign scale pointer moves the row by {d:.3f} = {d / P.tol16(errs[1]):.1f}x the tolerance")
        assert d >= 4 * P.tol16(errs[1]), (i, d, errs[1])
