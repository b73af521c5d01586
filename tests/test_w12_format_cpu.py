"""The 12-bit weight records' host reference (tests/w12_format.py) on its own: it round-trips every case the GPU test packs,
and N(0, 1 / sqrt(K)) weights escape as rarely as the format's design assumes."""
import numpy as np

import w12_format as F


def _round_trip(tiles):
    codes, meta, ok = F.pack(tiles)
    assert ok
    assert codes.shape == (len(tiles), 64, 3) and meta.shape == (len(tiles), 4)
    assert np.array_equal(F.unpack(codes, meta), tiles)
    return codes, meta


def test_planted_tiles_round_trip():
    t = F.planted_tiles()
    codes, meta = _round_trip(t)
    c = (meta[:, 0] >> 8) & 7
    assert c[0] == 0 and c[1] == 0 and c[3] == 0 and c[8] == 0 and c[9] == 0
    assert (c[2], c[4], c[5], c[6], c[7]) == (3, 2, 4, 6, 2)
    assert (meta[[0, 1, 3, 8], 0] & 0xFF).tolist() == [0, 0, 0, 0]            # base clamps to 0
    assert meta[5, 0] & 0xFF == 241                                           # Inf / NaN: base + code <= 255
    assert meta[7, 2] & 0x1FF == 0 and (meta[7, 2] >> 9) & 0x1FF == 511       # first and last element of the tile
    # the tile order is a permutation and its inverse
    w = F.from_tiles(t, F.PLANTED_N, F.PLANTED_K)
    assert w.shape == (32, 256) and np.array_equal(F.to_tiles(w), t)
    assert w[0, 0] == t[0, 0, 0] and w[17, 32 + 8 + 3] == t[8 + 1, 16 + 1, 3]


def test_plain_matrix_round_trip():
    _round_trip(F.normal_tiles(4 * 32, 1024, seed=5))                         # the GPU test's 64 x 1024 matrix


def test_seven_escapes_are_unpackable():
    codes, meta, ok = F.pack(F.seven_escape_tiles())
    assert not ok
    assert (meta[6, 0] >> 8) & 7 == 6                                         # the side record never overflows


def test_escape_statistic_of_normal_weights():
    """200,000 tiles of N(0, 1 / sqrt(5120)): 5.0-5.4 % of the tiles hold an escape (0.055 per tile: an element escapes when it
    lies 14 binades under the tile's maximum, |w| < ~2^-19 against sigma = 2^-6.2, 1.1e-4 per element, 512 elements), and
    none comes near the cap of six.  The bounds span that estimate and the measured interval, widened by 4 binomial
    standard deviations (0.0005) on either side."""
    n_esc = np.concatenate([F.escape_counts(F.normal_tiles(20000, 5120, seed=100 + i)) for i in range(10)])
    frac, mean = float((n_esc > 0).mean()), float(n_esc.mean())
    print(f"tiles with an escape {frac:.4f}, escapes per tile {mean:.4f}, max {int(n_esc.max())}")
    assert 0.048 <= frac <= 0.058
    assert 0.050 <= mean <= 0.060
    assert n_esc.max() <= F.MAX_ESC
    sub = F.normal_tiles(2000, 5120, seed=100)
    _round_trip(sub)
