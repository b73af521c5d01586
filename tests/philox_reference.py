"""An independent Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) in plain
numpy, and the two variate maps the device RNG documents in csrc/sampling.hip, restated from its comments - not from its code:

  exponential: counter (elem >> 2, draw_lo, draw_hi, 0x5D5D), key (seed_lo, seed_hi); the output word is chosen by elem & 3;
               u = ((x >> 9) + 0.5) * 2^-23 lies strictly inside (0, 1); the variate is -log(u).
  uniform:     counter (0, draw_lo, draw_hi, 0xACCE), same key; u = (word 0 >> 8) * 2^-24 lies in [0, 1).

Everything is vectorised over the counter; integers are uint64 arrays masked to 32 bits, floats are float64 (both maps are
exact in float32, which test_philox_reference_cpu.py shows), so nothing here shares a rounding with the code under test.
Needs no GPU.  tests/philox_replay.py feeds the DEVICE's variates to the oracle; this file says what they have to be."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57            # the two round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85            # the key schedule (golden ratio, sqrt(3) - 1)
MASK = np.uint64(0xFFFFFFFF)
EXP_DOMAIN, UNI_DOMAIN = 0x5D5D, 0xACCE

# Known-answer vectors of the Random123 distribution (kat_vectors, philox4x32 10): counter, key, output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def _u64(x):
    return np.atleast_1d(np.asarray(x, dtype=np.uint64))


def philox4x32(counter, key, rounds=10):
    """counter: four arrays (or ints) of 32-bit words, key: two.  Returns an (n, 4) uint32 array."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[_u64(c) & MASK for c in counter])
    k0, k1 = (_u64(k) & MASK for k in key)
    for _ in range(rounds):
        p0 = np.uint64(M0) * c0                                   # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def _split(x):
    x = int(x) & 0xFFFFFFFFFFFFFFFF
    return x & 0xFFFFFFFF, x >> 32


def exp_bits(seed, draw, V):
    """The 23-bit integers k of elements 0..V-1 of exponential draw `draw` of stream `seed`: u = (k + 0.5) * 2^-23."""
    elem = np.arange(V, dtype=np.uint64)
    (slo, shi), (dlo, dhi) = _split(seed), _split(draw)
    words = philox4x32((elem >> np.uint64(2), dlo, dhi, EXP_DOMAIN), (slo, shi))
    x = words[np.arange(V), (elem & np.uint64(3)).astype(np.int64)]
    return (x >> np.uint32(9)).astype(np.int64)


def exp_u(seed, draw, V):
    """float64, exact: the open-interval uniforms under the exponential variates."""
    return (exp_bits(seed, draw, V).astype(np.float64) + 0.5) * 2.0 ** -23


def exponential(seed, draw, V):
    """float64 -log(u): what sd_philox_exp has to return up to the device's logf and one rounding to fp32."""
    return -np.log(exp_u(seed, draw, V))


def uniform(seed, draw, n=1):
    """float64, exact in float32: the uniforms of draws draw .. draw + n - 1 (sd_philox_uniform's `draw + i`, in 64 bits)."""
    slo, shi = _split(seed)
    d = [_split(int(draw) + i) for i in range(n)]
    words = philox4x32((0, np.array([a for a, _ in d], dtype=np.uint64), np.array([b for _, b in d], dtype=np.uint64), UNI_DOMAIN),
                       (slo, shi))
    return (words[:, 0] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
