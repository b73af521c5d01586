"""Host reference of the 12-bit weight records (csrc/w12.h is the device definition): a numpy packer
and decoder for the documented layout, and the planted tiles the CPU and the GPU tests share.

A matrix is handled as its streaming tiles: uint16 [T][64][8], tile (n / 16, k / 32), lane 16 * (k / 8 % 4) + n % 16,
element k % 8.  Records: codes uint32 [T][64][3], side records uint32 [T][4]."""
import numpy as np

SM = np.uint32(0x807F807F)
CM = np.uint32(0x07800780)
MAX_ESC = 6
WINDOW = 14                      # base = max(E_max - 14, 0): codes 0..14


def f32_to_bf16(a):
    """float32 -> bf16 bits (uint16), round to nearest even (finite inputs)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def to_tiles(w):
    """row-major uint16 [N][K] -> [T][64][8] (sd_pack_weight_bf16's order)."""
    N, K = w.shape
    return np.ascontiguousarray(w.reshape(N // 16, 16, K // 32, 4, 8).transpose(0, 2, 3, 1, 4)).reshape(-1, 64, 8)


def from_tiles(t, N, K):
    return np.ascontiguousarray(t.reshape(N // 16, K // 32, 4, 16, 8).transpose(0, 3, 1, 2, 4)).reshape(N, K)


def _rotl(x, s):
    return (x << np.uint32(s)) | (x >> np.uint32(32 - s))


def exponents(tiles):
    """(E [T][64][8], base [T]) of uint16 tiles."""
    E = (tiles.astype(np.uint32) >> np.uint32(7)) & np.uint32(0xFF)
    emax = E.reshape(len(E), -1).max(axis=1).astype(np.int64)
    return E, np.maximum(emax - WINDOW, 0).astype(np.uint32)


def escape_counts(tiles):
    E, base = exponents(tiles)
    return (E < base[:, None, None]).reshape(len(E), -1).sum(axis=1)


def pack(tiles):
    """-> (codes uint32 [T][64][3], meta uint32 [T][4], packable).  Tiles with more than six escapes make the matrix
    unpackable; their side record keeps the first six."""
    T = len(tiles)
    v = tiles.astype(np.uint32)
    E, base = exponents(tiles)
    esc = E < base[:, None, None]
    code = np.where(esc, np.uint32(0), E - base[:, None, None]).astype(np.uint32)
    o = v[:, :, 0::2] | (v[:, :, 1::2] << np.uint32(16))                     # [T][64][4]
    codes = np.zeros((T, 64, 3), np.uint32)
    codes[:, :, 0] = (o[:, :, 0] & SM) | _rotl(o[:, :, 1] & SM, 8)
    codes[:, :, 1] = (o[:, :, 2] & SM) | _rotl(o[:, :, 3] & SM, 8)
    for i in range(4):
        codes[:, :, 2] |= (code[:, :, 2 * i] << np.uint32(4 * i)) | (code[:, :, 2 * i + 1] << np.uint32(16 + 4 * i))
    meta = np.zeros((T, 4), np.uint32)
    meta[:, 0] = base
    n_esc = esc.reshape(T, -1).sum(axis=1)
    Ef = E.reshape(T, -1)
    for t in np.nonzero(n_esc)[0]:
        pos = np.nonzero(esc[t].reshape(-1))[0][:MAX_ESC]                    # ascending lane * 8 + element
        meta[t, 0] |= np.uint32(len(pos) << 8)
        for j, p in enumerate(pos):
            e = np.uint32(Ef[t, p])
            if j < 2:
                meta[t, 0] |= e << np.uint32(16 + 8 * j)
            else:
                meta[t, 1] |= e << np.uint32(8 * (j - 2))
            meta[t, 2 + j // 3] |= np.uint32(p) << np.uint32(9 * (j % 3))
    return codes, meta, bool((n_esc <= MAX_ESC).all())


def unpack(codes, meta):
    """-> uint16 tiles [T][64][8]."""
    T = len(codes)
    base = meta[:, 0] & np.uint32(0xFF)
    bb = (base * np.uint32(0x00800080))[:, None]
    p0, p1, p2 = codes[:, :, 0], codes[:, :, 1], codes[:, :, 2]
    sm = [p0 & SM, _rotl(p0, 24) & SM, p1 & SM, _rotl(p1, 24) & SM]
    sh = [p2 << np.uint32(7), p2 << np.uint32(3), p2 >> np.uint32(1), p2 >> np.uint32(5)]
    o = np.stack([(sm[i] | (sh[i] & CM)) + bb for i in range(4)], axis=2)    # [T][64][4]
    c = (meta[:, 0] >> np.uint32(8)) & np.uint32(7)
    for t in np.nonzero(c)[0]:
        for j in range(int(c[t])):
            e = (meta[t, 0] >> np.uint32(16 + 8 * j)) & np.uint32(0xFF) if j < 2 else (meta[t, 1] >> np.uint32(8 * (j - 2))) & np.uint32(0xFF)
            pos = int((meta[t, 2 + j // 3] >> np.uint32(9 * (j % 3))) & np.uint32(0x1FF))
            o[t, pos >> 3, (pos >> 1) & 3] -= (base[t] - e) << np.uint32(7 + 16 * (pos & 1))
    out = np.zeros((T, 64, 8), np.uint16)
    out[:, :, 0::2] = (o & np.uint32(0xFFFF)).astype(np.uint16)
    out[:, :, 1::2] = (o >> np.uint32(16)).astype(np.uint16)
    return out


def normal_tiles(n_tiles, K, seed):
    """n_tiles tiles of N(0, 1 / sqrt(K)) weights rounded to bf16."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(size=(n_tiles, 64, 8), dtype=np.float32) * np.float32(1.0 / np.sqrt(K))
    return f32_to_bf16(a)


def _bits(E, rng, shape):
    """random-sign, random-mantissa bf16 bits with exponent field(s) E."""
    return (rng.integers(0, 2, size=shape).astype(np.uint16) << 15) | (np.asarray(E, np.uint16) << 7) | rng.integers(0, 128, size=shape).astype(np.uint16)


PLANTED_N, PLANTED_K = 32, 256                  # 2 x 8 = 16 tiles


def planted_tiles():
    """The 16 tiles of the round-trip tests: [16][64][8] uint16, every one packable."""
    rng = np.random.default_rng(12)
    t = normal_tiles(16, PLANTED_K, seed=3)                                  # tiles 11.. stay plain
    body = lambda lo, hi: _bits(rng.integers(lo, hi + 1, size=(64, 8)), rng, (64, 8))
    t[0] = 0                                                                 # all zeros
    t[1] = 0x8000                                                            # all -0.0 (base 0, no escape)
    t[2] = body(118, 126); t[2, 5, 3] = 0x8000; t[2, 40, 0] = 0x8000; t[2, 41, 7] = 0x0000   # -0.0 / +0.0 under a large maximum
    t[3] = _bits(0, rng, (64, 8)) | 1                                        # all denormals (base 0)
    t[4] = body(120, 127); t[4, 7, 1] = 0x0001; t[4, 33, 6] = 0x807F         # denormals under a large maximum
    t[5] = body(243, 254)                                                    # Inf and NaN next to 2^-20
    t[5, 0, 1], t[5, 9, 2], t[5, 17, 4], t[5, 63, 0] = 0x7F80, 0xFF80, 0x7FC1, 0xFFFF
    for lane, el in ((1, 0), (2, 7), (30, 3), (62, 5)):
        t[5, lane, el] = (127 - 20) << 7
    t[6] = body(115, 127)                                                    # exactly six escapes
    for lane, el in ((3, 2), (3, 3), (19, 0), (31, 7), (32, 1), (60, 6)):
        t[6, lane, el] = _bits(int(rng.integers(1, 100)), rng, ())
    t[7] = body(113, 127); t[7, 0, 0] = 0x0000; t[7, 63, 7] = _bits(50, rng, ())   # escapes in the first and the last element
    t[8] = body(0, 13)                                                       # maximum exponent below 14: base clamps to 0
    t[9] = body(100, 114); t[9, 10, 4] = 114 << 7                            # the whole window in use (codes 0..14), no escape
    t[10] = body(241, 255)                                                   # base + code up to 255
    assert (escape_counts(t) <= MAX_ESC).all()
    assert escape_counts(t)[6] == 6 and escape_counts(t)[7] == 2 and escape_counts(t)[5] == 4
    return t


def seven_escape_tiles():
    """planted_tiles() with a seventh escape in tile 6: not packable."""
    t = planted_tiles()
    t[6, 61, 1] = 0x0000
    assert escape_counts(t)[6] == 7
    return t
