"""tests/philox_reference.py against the published known-answer vectors of Philox4x32-10, and the two variate maps of
csrc/sampling.hip: exact in float32, in range, and drawn from separate counter domains.  Needs no GPU."""
import numpy as np

import philox_reference as PR


def _scalar_philox(c, k):
    """The algorithm once more, one counter at a time in Python integers: a second opinion for the vectorised one."""
    c, k = list(c), list(k)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return tuple(c)


def test_known_answer_vectors():
    for ctr, key, want in PR.KAT:
        got = tuple(int(x) for x in PR.philox4x32(ctr, key)[0])
        print("philox4x32-10", " ".join(f"{x:08x}" for x in ctr), "/", " ".join(f"{x:08x}" for x in key), "->",
              " ".join(f"{x:08x}" for x in got))
        assert got == want
        assert _scalar_philox(ctr, key) == want


def test_vectorised_counters_equal_the_scalar_algorithm():
    rng = np.random.default_rng(0)
    ctr = rng.integers(0, 2 ** 32, size=(64, 4), dtype=np.uint64)
    key = (0x89ABCDEF, 0x01234567)
    got = PR.philox4x32((ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3]), key)
    for row, g in zip(ctr, got):
        assert tuple(int(x) for x in g) == _scalar_philox([int(x) for x in row], key)


def test_variate_maps_are_exact_in_fp32_and_in_range():
    seed, draw, V = 0x8000000500000007, 2 ** 40 + 3, 50272
    k = PR.exp_bits(seed, draw, V)
    assert k.min() >= 0 and k.max() < 2 ** 23
    u = PR.exp_u(seed, draw, V)
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)           # (k + 0.5) * 2^-23 needs 24 bits
    assert u.min() >= 2.0 ** -24 and u.max() <= 1.0 - 2.0 ** -24
    # the extreme codes too, whether or not this stream holds them
    for kk in (0, 2 ** 23 - 1):
        x = (kk + 0.5) * 2.0 ** -23
        assert float(np.float32(x)) == x and 0.0 < x < 1.0
    e = PR.exponential(seed, draw, V)
    assert e.min() > 0.0 and e.max() < 16.7                                     # -log(2^-24) = 16.64
    r = PR.uniform(seed, 2 ** 32 - 3, 600)                                      # the draws cross 2^32: the high word moves
    assert np.array_equal(r.astype(np.float32).astype(np.float64), r) and r.min() >= 0.0 and r.max() < 1.0
    assert float(np.float32((2 ** 24 - 1) * 2.0 ** -24)) < 1.0
    print(f"exp u in [{u.min():.3e}, {u.max():.9f}], mean {u.mean():.4f}; uniform mean {r.mean():.4f}")


def test_fields_every_word_of_the_counter_and_key_reaches_the_output():
    """What the GPU sweep relies on: elem & 3 picks the word, elem >> 2 / draw low / draw high / seed low / seed high each
    change the block, and the two domains do not share a counter."""
    base = PR.exp_bits(5, 9, 64)
    words = PR.philox4x32((np.arange(16, dtype=np.uint64), 9, 0, PR.EXP_DOMAIN), (5, 0))
    assert np.array_equal(base, (words.reshape(-1) >> np.uint32(9)).astype(np.int64))   # element 4j + w is word w of block j
    for seed, draw in ((5, 9 + 2 ** 32), (5 + 2 ** 32, 9), (6, 9), (5, 10), (5 + 2 ** 63, 9)):
        assert (PR.exp_bits(seed, draw, 64) != base).mean() > 0.9
    u0 = PR.uniform(5, 9, 1)[0]
    assert u0 != PR.uniform(5, 9 + 2 ** 32, 1)[0] and u0 != PR.uniform(5 + 2 ** 32, 9, 1)[0]
    w_exp = PR.philox4x32((0, 9, 0, PR.EXP_DOMAIN), (5, 0))[0]
    w_uni = PR.philox4x32((0, 9, 0, PR.UNI_DOMAIN), (5, 0))[0]
    assert not np.array_equal(w_exp, w_uni) and u0 == float(w_uni[0] >> np.uint32(8)) * 2.0 ** -24


def test_marginals_of_the_reference_itself():
    """A sanity check of the reference, not of the device: 2^16 exponentials and uniforms fit their laws (chi-square over 32
    equiprobable bins, bar at 1e-9)."""
    from scipy import stats
    u = np.concatenate([PR.exp_u(77, d, 8192) for d in range(8)])
    r = np.concatenate([PR.uniform(s, 0, 1024) for s in range(64)])
    bar = stats.chi2.isf(1e-9, 31)
    for name, x in (("exp", u), ("uniform", r)):
        obs = np.bincount((x * 32).astype(int), minlength=32)
        x2 = float(((obs - len(x) / 32) ** 2 / (len(x) / 32)).sum())
        print(f"{name}: X2 {x2:.1f} on 31 dof, bar {bar:.1f}")
        assert x2 < bar
