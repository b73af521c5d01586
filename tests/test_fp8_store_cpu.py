"""The e4m3 store definition on the host, and what the GPU test's inputs cover (needs no GPU).

  * fp8_store.e4m3_byte - integers alone, from the OCP format - against torch's float8_e4m3fn cast over all 65536 bf16 and
    all 65536 fp16 patterns at scale 1, three powers of two at either end of the tables' range, 0.3 and 1.7;
  * the two definitions, x * fl32(1 / s) and fl32(x / s), re-derived with the encoder: the 16-bit patterns on which they give
    different bytes at 0.3 and 1.7 (the GPU test plants them);
  * oracle.models_ref._kv_fp8 is the scale-1 case of the same function;
  * the coverage conditions of test_gpu_fp8_store.py, on the oracle's K / V rows alone.
"""
import numpy as np
import pytest
import torch

import fp8_store as F
from oracle import models_ref

POW2_ENDS = [2.0 ** k for k in (-12, -11, -10, 10, 11, 12)]
SCALES = [1.0] + POW2_ENDS + [0.3, 1.7]


def _torch_bytes(bits, dt, scale, divide=False):
    x = F.from_bits(bits, dt).float()
    s = torch.tensor(scale, dtype=torch.float32)
    v = x / s if divide else x * (torch.tensor(1.0, dtype=torch.float32) / s)
    return v.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("scale", SCALES)
def test_encoder_equals_torch_cast_on_every_16_bit_pattern(dt, scale):
    p = F.all_patterns()
    _, _, _, nan, _ = F.split16(p, dt)
    for divide, enc in ((False, F.e4m3_byte), (True, F.e4m3_byte_div)):
        mine, ref = enc(p, dt, scale), _torch_bytes(p, dt, scale, divide)
        assert ((mine & 0x7F) == 0x7F).tolist() == nan.tolist()            # NaN in, NaN out, and nothing else
        assert np.array_equal(mine & 0x7F, ref & 0x7F) and np.array_equal(mine[~nan], ref[~nan]), (dt, scale, divide)


def test_reciprocal_in_integers_is_the_fp32_quotient():
    rng = np.random.default_rng(0)
    for s in SCALES + [3.0, 1.0 / 3.0, 5.0, 6.0, 10.0] + (2.0 ** rng.uniform(-20, 20, size=2000)).tolist():
        m, e = F.rcp32(s)
        want = np.float32(1.0) / np.float32(s)
        assert float(m) * 2.0 ** e == float(want), s


def test_every_code_and_every_midpoint_at_scale_one():
    """Written from the format: every finite code encodes to itself; a midpoint goes to the even neighbour; half the smallest
    denormal goes to +-0 with the sign kept; 448 < x stays 448."""
    codes = np.arange(0, 0x7F)
    vals = F.e4m3_value(codes)
    assert vals[1] == 2.0 ** -9 and vals[8] == 2.0 ** -6 and vals[0x7E] == 448.0 and np.all(np.diff(vals) > 0)
    for sign in (0, 0x8000):
        b16 = F.to_bits(torch.tensor(vals, dtype=torch.float16)) | sign
        assert np.array_equal(F.e4m3_byte(b16, "fp16", 1.0), codes | (sign >> 8))
        mids = (vals[:-1] + vals[1:]) / 2
        b16 = F.to_bits(torch.tensor(mids, dtype=torch.float16)) | sign
        even = np.where(codes[:-1] % 2 == 0, codes[:-1], codes[1:])
        assert np.array_equal(F.e4m3_byte(b16, "fp16", 1.0), even | (sign >> 8))
    assert F.e4m3_byte([0x1400, 0x9400, 0x1401, 0x9401], "fp16", 1.0).tolist() == [0x00, 0x80, 0x01, 0x81]   # 2^-10 and the next
    assert F.e4m3_byte([0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x7E00, 0xFE00], "fp16", 1.0).tolist() == [0x7E, 0xFE, 0x7E, 0xFE, 0x7F, 0xFF]


def test_oracle_kv_fp8_is_the_scale_one_case():
    for dt in ("bf16", "fp16"):
        p = F.all_patterns()
        _, _, _, nan, _ = F.split16(p, dt)
        got = models_ref._kv_fp8(F.from_bits(p, dt)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
        mine = F.e4m3_byte(p, dt, 1.0)
        assert np.array_equal(got[~nan], mine[~nan]) and np.all((got[nan] & 0x7F) == 0x7F)


def test_the_two_definitions_differ_on_a_few_patterns():
    """The contract: the arena holds x * fl32(1 / scale).  At 0.3 and 1.7 the quotient fl32(x / scale) gives another byte on
    the patterns listed here (the product lands on the other side of an e4m3 rounding boundary); torch agrees with the
    encoder on both sides.  The GPU test plants exactly these."""
    found = {}
    for dt in ("bf16", "fp16"):
        for s in F.CONTRACT_SCALES:
            pats = F.contract_patterns(dt, s)
            found[(dt, s)] = pats
            b = np.array(pats, dtype=np.int64)
            if len(pats):
                assert np.array_equal(F.e4m3_byte(b, dt, s), _torch_bytes(b, dt, s))
                assert np.array_equal(F.e4m3_byte_div(b, dt, s), _torch_bytes(b, dt, s, divide=True))
            print(f"{dt} scale {s}: {len(pats)} patterns differ: {[hex(x) for x in pats[:8]]}")
        for s in (3.0, 1.0 / 3.0, 5.0, 6.0, 10.0, 0.5, 4.0):
            print(f"{dt} scale {s:.4f}: {len(F.contract_patterns(dt, s))} patterns differ")
    assert all(len(found[("bf16", s)]) > 0 for s in F.CONTRACT_SCALES), found   # (else the planted contract case would be empty)
    assert all(len(F.contract_patterns(dt, 2.0 ** k)) == 0 for dt in ("bf16", "fp16") for k in (-12, -3, 0, 5, 12))


# ----------------------------------------------------------------------------- coverage of the GPU test's inputs
def test_planted_sweep_reaches_every_class():
    """2 signs x 128 mantissas x 4 exponents under 24 power-of-two scales: every (sign, mantissa) meets every e4m3 binade, the
    denormal range, both flushes and both saturations; every tie direction occurs."""
    bits = F.planted_bf16()
    assert sorted(bits.ravel().tolist()) == sorted((s << 15) | (e << 7) | m for s in (0, 1) for e in F.PLANT_EXPS for m in range(128))
    scales = F.sweep_scales()
    first = F.e4m3_byte(bits.ravel(), "bf16", scales[0])
    last = F.e4m3_byte(bits.ravel(), "bf16", scales[-1])
    assert set(first.tolist()) == {0x00, 0x80} and set(last.tolist()) == {0x7E, 0xFE}
    seen = set()
    for s in scales:
        by = F.e4m3_byte(bits.ravel(), "bf16", s)
        seen |= {(int(b) & 0x7F, int(p) & 0x7F, int(p) >> 15) for b, p in zip(by, bits.ravel())}
    for sign in (0, 1):
        for man in range(128):
            binades = {b >> 3 for b, m, sg in seen if m == man and sg == sign}
            assert binades == set(range(16)), (sign, man, binades)
    assert {b for b, _, _ in seen} == set(range(0x7F))                  # every finite code is some value's byte
    up = dn = 0
    for s in scales:
        u, d = F.tie_counts(bits.reshape(1, 1, 1, -1), "bf16", np.full((1, 1, 1), s, dtype=np.float32))
        up, dn = up + u, dn + d
    assert up > 100 and dn > 100, (up, dn)


def test_planted_fp16_holds_every_boundary():
    bits = F.planted_fp16().ravel()
    have = set(bits.tolist())
    for b in F.fp16_boundaries() + [0x7BFF, 0x0001]:
        assert b in have and (b | 0x8000) in have
    _, _, _, nan, inf = F.split16(bits, "fp16")
    assert not nan.any() and not inf.any() and 0x8000 not in have
    by = F.e4m3_byte(bits, "fp16", 1.0)
    assert set(range(0x7F)) <= set((by & 0x7F).tolist())


GPU_MODELS = [(n, d) for n in F.TWIN_MODELS for d in ("bf16", "fp16")]


@pytest.mark.parametrize("name,dt", GPU_MODELS, ids=[f"{n}-{d}" for n, d in GPU_MODELS])
def test_tables_meet_the_coverage_conditions(name, dt):
    """On the oracle's K / V rows of the GPU test's 17-row pass (the twin session's rows differ from them by summation order
    only).  Asserted: every table's entries differ; `tight` has an element beyond +448 and one beyond -448 in every (layer,
    k|v, head) and saturates more than half of all elements; `loose` has a non-zero denormal, a +0 and a -0 in every one and
    nothing past the first normal binade; `pow2` meets exact ties that round up and ties that round down; a wrong table
    entry (K's for V's, another head's, another layer's) changes the byte of at least 95 % of the elements under `pow2`.

    Measured and printed, with a floor only, because the tables' own definitions rule the full condition out: exact ties
    under `real` (a non-power-of-two reciprocal leaves the 24-bit product on a tie with a probability of about 2^-20 per
    element; where they occur it is because the head's amax is a small multiple of 7 - the planted sweep and `pow2` carry
    the ties); the share of bytes a wrong entry changes under `real` (neighbouring heads' amax differ by a few per cent:
    34 .. 82 %), `tight` (most elements saturate under either entry: 2 .. 4 %) and `loose` (most are 0 or one or two quanta
    under either entry: 23 .. 45 %).  A mutant needs ONE byte to differ; 1 % of a plane is 20 bytes and more."""
    bits = F.oracle_kv_bits(name, dt, F.TABLE_ROWS)
    vals = F.bits_value(bits, dt)
    n_el = bits[0, 0, 0].size
    for kind in F.TABLES:
        tab = F.scale_table(name, dt, kind)
        assert tab.dtype == np.float32
        if kind == "pow2" and tab.size > 25:                       # 32 entries, 25 powers of two: different inside every layer
            assert all(len(set(t.ravel().tolist())) == t.size for t in tab) and (tab[0] != tab[1]).all()
        else:
            assert len(set(tab.ravel().tolist())) == tab.size
        want = F.e4m3_byte_table(bits, dt, tab)
        changed = {k: float((F.e4m3_byte_table(bits, dt, np.ascontiguousarray(t)) != want).mean())
                   for k, t in F.swapped_tables(tab).items()}
        up, dn = F.tie_counts(bits, dt, tab)
        print(f"{name} {dt} {kind}: ties up {up} down {dn}; bytes changed by a wrong entry "
              + ", ".join(f"{k} {v:.3f}" for k, v in changed.items()))
        q = vals / tab[..., None, None].astype(np.float64)
        if kind == "tight":
            assert (q > 448).any(axis=(-1, -2)).all() and (q < -448).any(axis=(-1, -2)).all()
            assert ((want & 0x7F) == 0x7E).mean() > 0.5
        if kind == "loose":
            den = ((want & 0x7F) > 0) & ((want & 0x7F) < 8)
            assert den.any(axis=(-1, -2)).all() and (want == 0x00).any(axis=(-1, -2)).all() and (want == 0x80).any(axis=(-1, -2)).all()
            assert ((want & 0x7F) < 0x10).all()                            # nothing past the first normal binade
        if kind == "pow2":
            assert up > 0 and dn > 0, (up, dn)
        # a wrong entry shows on an element unless both scales flush it, saturate it or leave it in one rounding cell (half a
        # quantum is 1 / 32 .. 1 / 16 of the value): `pow2` entries are at least a factor 2 apart, so nearly every element
        # shows it; the entries of the other three are near each other (and `tight` saturates, `loose` flushes most
        # elements under either entry), so only a floor is held
        floor = 0.95 if kind == "pow2" else 0.01
        assert all(v >= floor for v in changed.values()), (kind, changed)
    assert n_el == F.TABLE_ROWS * F.config(name).head_dim
