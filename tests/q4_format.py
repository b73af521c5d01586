"""Host definition of the 4-bit group-quantised weight records (csrc/q4.h is the device definition):
the weight w = bf16_rne(float(s) * float(q - z)) per group of 128 k of a row, the 1088-byte record layout, and the planted
groups the GPU tests use.  q uint8 [N][K], s uint16 (bf16 bits) [N][K / 128], z uint8 [N][K / 128]."""
import numpy as np

from w12_format import f32_to_bf16, to_tiles

GROUP = 128
REC_DWORDS = 272                 # 64 lanes x 4 dwords of codes, then 16 dwords s | z << 16


def weights(q, s, z):
    """-> bf16 bits uint16 [N][K] of w (the fp32 product is exact: 8 significant bits times at most 5)."""
    sf = (s.astype(np.uint32) << np.uint32(16)).view(np.float32)
    d = q.astype(np.int32) - np.repeat(z.astype(np.int32), GROUP, axis=1)
    return f32_to_bf16(np.repeat(sf, GROUP, axis=1) * d.astype(np.float32))


def records(q, s, z):
    """-> uint32 [N / 16 * K / 128][272]: record (n-tile, group); dword u of lane l holds the eight codes of
    W[n = l % 16][k = 32 u + 8 (l / 16) + e], code e in bits 4e .. 4e + 3."""
    N, K = q.shape
    c = q.astype(np.uint32).reshape(N // 16, 16, K // GROUP, 4, 4, 8)          # [nt][n][g][u][quad][e]
    dw = (c << (np.uint32(4) * np.arange(8, dtype=np.uint32))).sum(axis=-1, dtype=np.uint32)
    codes = dw.transpose(0, 2, 4, 1, 3).reshape(-1, 256)                        # [nt][g][quad][n][u]: lane = 16 quad + n
    sz = (s.astype(np.uint32) | (z.astype(np.uint32) << np.uint32(16))).reshape(N // 16, 16, K // GROUP)
    return np.concatenate([codes, sz.transpose(0, 2, 1).reshape(-1, 16)], axis=1)


def tiles(q, s, z):
    return to_tiles(weights(q, s, z))


def random_case(N, K, seed):
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 16, size=(N, K), dtype=np.uint8)
    z = rng.integers(0, 16, size=(N, K // GROUP), dtype=np.uint8)
    s = f32_to_bf16(rng.standard_normal(size=(N, K // GROUP), dtype=np.float32) * np.float32(0.01))
    return q, s, z


PLANTED_N, PLANTED_K = 32, 256


def planted_case():
    """random_case with planted groups in rows 0..7 (both groups of the row): codes 0 and 15 against zero points 0 and 15, a
    zero scale, a negative one, 0x3F81 times 3 (129 / 128 * 3 = 193.5 / 64 lies halfway between two bf16: to even, 194 / 64 = 0x4042) and
    a full mantissa times 15."""
    q, s, z = random_case(PLANTED_N, PLANTED_K, seed=4)
    q[0], z[0] = 0, 0
    q[1], z[1] = 15, 0
    q[2], z[2] = 0, 15
    q[3], z[3] = 15, 15
    s[4] = 0
    s[5] = 0xBC23
    s[6], z[6] = 0x3F81, 2
    q[6, ::2], q[6, 1::2] = 5, 4                                   # q - z = 3 and 2
    s[7], z[7] = 0x3CFF, 0
    q[7, ::3] = 15
    assert weights(q, s, z)[6, 0] == 0x4042 and weights(q, s, z)[6, 1] == 0x4001
    return q, s, z
