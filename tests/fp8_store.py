"""What an e4m3 KV arena must hold, byte for byte (helper of test_fp8_store_cpu.py and test_gpu_fp8_store.py; needs no GPU).

Both store paths of the engine - store4_fp8 (OPT's K / V rows, Llama's V rows) and to_fp8 (Llama's K rows, on the RoPE
pairs), in the fused QKV epilogue of the GEMMs (gemm_epilogue_fold); the stand-alone qkv_epilogue_kernel has no fp8 store,
an fp8 arena needs the fused layout - round the K / V element to the model's 16-bit type BEFORE they quantise it.  The stored byte is therefore a pure function of a 16-bit pattern, which a
16-bit arena of the same model would hold bit for bit, and of one fp32 scale:

    byte = e4m3( clamp( fl32( x * fl32(1 / scale) ), -448, 448 ) )         NaN stays NaN

`e4m3_byte` is that function in integer arithmetic alone, written from the OCP 8-bit floating point format (E4M3: bias 7,
3 mantissa bits, denormals, no infinity, S.1111.111 the only NaN, largest finite 448 = S.1111.110), round to nearest even.
`e4m3_byte_div` is the other definition the comments used to give, fl32(x / scale): the two differ on a handful of 16-bit
values at scales such as 0.3 and 1.7 (`contract_patterns`), and the arena holds the first.

The rest of the file is what the two tests share: the four scale tables, a GQA probe model, the probe models' weights with
every o_proj zero (a layer's K / V then depend on the tokens and positions alone, not on what attention read from the
arena), the oracle's K / V rows as 16-bit patterns, and the planted-bias sets of the exhaustive sweep.
"""
from __future__ import annotations

import functools
from typing import Dict, List, Tuple

import numpy as np
import torch

import oracle
import seam_probe as S
from llmspeculativesampling_amd.config import ModelConfig
from llmspeculativesampling_amd.synth import make_state_dict

NAN_BYTE, MAX_BYTE = 0x7F, 0x7E    # S.1111.111 / 448
E4M3_MAX = 448
NP16 = {"bf16": (8, 7, 127), "fp16": (5, 10, 15)}                  # exponent bits, mantissa bits, bias


# ----------------------------------------------------------------------------- the definition, in integers
def _bit_length(v: np.ndarray) -> np.ndarray:
    """Bits of the non-negative int64 values (0 for 0)."""
    v = v.copy()
    n = np.zeros(v.shape, dtype=np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        big = (v >> s) > 0
        n += np.where(big, s, 0)
        v = np.where(big, v >> s, v)
    return n + (v > 0)


def _rne_shift(v: np.ndarray, sh: np.ndarray) -> np.ndarray:
    """v / 2^sh (sh >= 0) rounded to the nearest integer, ties to even."""
    sh = np.minimum(sh, 62)
    q = v >> sh
    rem = v - (q << sh)
    half = np.where(sh > 0, np.int64(1) << np.maximum(sh - 1, 0), 0)
    up = (sh > 0) & ((rem > half) | ((rem == half) & ((q & 1) == 1)))
    return q + up


def split16(bits16, dtype: str):
    """16-bit patterns -> (sign, m, e, nan, inf) with |x| = m * 2^e exactly (m, e int64)."""
    eb, mb, bias = NP16[dtype]
    b = np.asarray(bits16).astype(np.int64) & 0xFFFF
    sign, ex, man = b >> 15, (b >> mb) & ((1 << eb) - 1), b & ((1 << mb) - 1)
    top = ex == (1 << eb) - 1
    m = np.where(ex == 0, man, man | (1 << mb))
    e = np.where(ex == 0, 1, ex) - bias - mb
    return sign, np.where(top, 0, m), e, top & (man != 0), top & (man == 0)


def split32(x: float) -> Tuple[int, int]:
    """A positive normal fp32 number -> (m, e) with x = m * 2^e, m a 24-bit integer."""
    b = int(np.array(x, dtype=np.float32).view(np.uint32))
    ex, man = (b >> 23) & 0xFF, b & 0x7FFFFF
    assert b >> 31 == 0 and 0 < ex < 255, ("a positive normal fp32 scale", x)
    return man | (1 << 23), ex - 127 - 23


def rcp32(scale: float) -> Tuple[int, int]:
    """fl32(1 / scale) as (m, e): the quotient 2^k / m_s to 26 bits and a sticky bit, rounded once to 24."""
    ms, es = split32(scale)
    num = 1 << 72
    q, r = divmod(num, ms)                                         # q has 49 or 50 bits
    q = (q << 1) | (r != 0)
    sh = q.bit_length() - 24
    half, rem, m = 1 << (sh - 1), q & ((1 << sh) - 1), q >> sh
    m += rem > half or (rem == half and m & 1)
    e = -es - 72 - 1 + sh
    if m == 1 << 24:
        m, e = m >> 1, e + 1
    assert -126 <= e + 23 <= 127, ("1 / scale is a normal fp32 number", scale)
    return m, e


def _encode(sign, q, E, nan, inf):
    """|v| = q * 2^E with more than 24 significant bits where it is inexact (the last bit set then: sticky).  Rounds once to
    fp32 (24 bits; below 2^-126 the result is far under half the smallest e4m3 denormal whatever fp32 does with it), clamps
    to 448, rounds to e4m3."""
    bl = _bit_length(q)
    q = _rne_shift(q, np.maximum(bl - 24, 0))
    E = E + np.maximum(bl - 24, 0)
    bl = _bit_length(q)                                            # (24, or 25 when the rounding carried)
    t = np.where(q > 0, bl - 1 + E, -1000)                         # floor(log2 |v|)
    # |v| > 448 = 7 * 2^6: certainly from 2^9 on, certainly not below 2^8; between, compare q * 2^E with 7 * 2^6 exactly
    Ec = np.clip(E, -40, 10)
    mid = np.where(Ec >= 0, (q << np.maximum(Ec, 0)) > E4M3_MAX, q > (np.int64(E4M3_MAX) << np.maximum(-Ec, 0)))
    sat = inf | (t >= 9) | ((t == 8) & mid)
    g = np.maximum(t - 3, -9)                                      # exponent of the quantum: 2^-9 in the denormal range
    sh = g - E
    r = np.where(sh <= 0, q << np.clip(-sh, 0, 20), _rne_shift(q, np.maximum(sh, 0)))
    r = np.where(q > 0, r, 0)
    byte = ((g + 9) << 3) + r                                      # normal: (t + 7) << 3 | (r - 8); a carry to r = 16 lands
    byte = np.where(t < -20, 0, byte)                              # on the next binade by itself; denormal: r
    byte = np.where(sat | (byte > MAX_BYTE), MAX_BYTE, byte)
    byte = np.where(nan, NAN_BYTE, byte)
    return (byte | (sign << 7)).astype(np.uint8)


def e4m3_byte(bits16, dtype: str, scale: float) -> np.ndarray:
    """The byte an e4m3 arena holds for the 16-bit pattern(s) under `scale`: e4m3(clamp(fl32(x * fl32(1 / scale))))."""
    sign, m, e, nan, inf = split16(bits16, dtype)
    mr, er = rcp32(scale)
    return _encode(sign, m * mr, e + er, nan, inf)                 # the product is exact: at most 11 + 24 bits


def e4m3_byte_div(bits16, dtype: str, scale: float) -> np.ndarray:
    """The same with fl32(x / scale) for the product - NOT what the arena holds (see contract_patterns)."""
    sign, m, e, nan, inf = split16(bits16, dtype)
    ms, es = split32(scale)
    num = m << 50                                                  # < 2^61; the quotient has at least 27 bits where m > 0
    q = num // ms
    q = (q << 1) | (num - q * ms != 0)
    return _encode(sign, q, e - es - 51, nan, inf)


def e4m3_byte_table(bits16: np.ndarray, dtype: str, table: np.ndarray) -> np.ndarray:
    """bits16 [L][2][Hkv][rows][D] under table [L][2][Hkv]."""
    out = np.empty(bits16.shape, dtype=np.uint8)
    for idx in np.ndindex(*table.shape):
        out[idx] = e4m3_byte(bits16[idx], dtype, float(table[idx]))
    return out


def e4m3_value(byte) -> np.ndarray:
    """The number a byte stands for (float64; NaN for S.1111.111) - for the tests' own bookkeeping."""
    b = np.asarray(byte).astype(np.int64)
    ex, man = (b >> 3) & 15, b & 7
    v = np.where(ex == 0, man * 2.0 ** -9, (8 + man) * 2.0 ** (ex - 10.0))
    v = np.where((b & 0x7F) == NAN_BYTE, np.nan, v)
    return np.where(b >> 7 == 1, -v, v)


def all_patterns() -> np.ndarray:
    return np.arange(65536, dtype=np.int64)


def to_bits(t: torch.Tensor) -> np.ndarray:
    """A bf16 / fp16 tensor's patterns (int64)."""
    assert t.dtype in (torch.bfloat16, torch.float16)
    return t.contiguous().view(torch.int16).numpy().astype(np.int64) & 0xFFFF


def from_bits(bits, dtype: str) -> torch.Tensor:
    a = np.asarray(bits).astype(np.uint16).view(np.int16)
    return torch.from_numpy(a.copy()).view(S.DTYPES[dtype])


def contract_patterns(dtype: str, scale: float) -> List[int]:
    """The finite 16-bit patterns whose byte differs between x * fl32(1 / scale) and fl32(x / scale)."""
    p = all_patterns()
    _, _, _, nan, inf = split16(p, dtype)
    diff = (e4m3_byte(p, dtype, scale) != e4m3_byte_div(p, dtype, scale)) & ~nan & ~inf
    return [int(x) for x in p[diff]]


CONTRACT_SCALES = (0.3, 1.7)


# ----------------------------------------------------------------------------- models
GQA = "llama_gqa"                  # 8 query heads on 2 KV heads, D = 32, 3 layers: head - Hq runs 0 .. 3, K heads then V heads
GQA_CFG = dict(arch="llama", vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=3,
               num_attention_heads=8, num_key_value_heads=2, max_position_embeddings=S.MAX_POS, rms_norm_eps=1e-5)
OPT = "opt_pre_h256"
TWIN_MODELS = ("llama_h1024", "llama_h256", OPT, GQA)


def config(name: str) -> ModelConfig:
    return ModelConfig(**GQA_CFG) if name == GQA else S.probe_config(name)


def _o_proj_names(cfg: ModelConfig) -> List[str]:
    if cfg.arch == "llama":
        return [f"model.layers.{l}.self_attn.o_proj.weight" for l in range(cfg.num_hidden_layers)]
    return [f"model.decoder.layers.{l}.self_attn.out_proj.weight" for l in range(cfg.num_hidden_layers)]


@functools.lru_cache(maxsize=None)
def state_dict(name: str) -> Dict[str, torch.Tensor]:
    """The probe weights (fp32 tensors of bf16 numbers) with every o_proj zero.  Shared: do not modify."""
    cfg = config(name)
    if name == GQA:
        sd = {k: v.to(torch.bfloat16).float() for k, v in make_state_dict(cfg, 47, head_gain=2.0).items()}
    else:
        sd = dict(S.probe_state_dict(name))
    for k in _o_proj_names(cfg):
        sd[k] = torch.zeros_like(sd[k])
    return sd


def tokens(n: int) -> Tuple[int, ...]:
    return tuple(S.ordinary(r) for r in range(n))


@functools.lru_cache(maxsize=None)
def oracle_kv_bits(name: str, dt: str, n: int, pos0: int = 0) -> np.ndarray:
    """[L][2][Hkv][n][D] patterns of the K (after RoPE) / V rows the 16-bit oracle appends for `tokens(n)` at pos0."""
    lm = oracle.RefCausalLM(config(name), S.cast_sd(state_dict(name), S.DTYPES[dt]))
    past = lm(torch.tensor([S.prefix_tokens(pos0)])).past_key_values if pos0 else None
    kv = lm(torch.tensor([list(tokens(n))]), past_key_values=past).past_key_values
    return np.stack([np.stack([to_bits(k[0, :, pos0:]), to_bits(v[0, :, pos0:])]) for k, v in kv])


def bits_value(bits: np.ndarray, dtype: str) -> np.ndarray:
    return from_bits(bits, dtype).double().numpy().reshape(np.shape(bits))


# ----------------------------------------------------------------------------- scale tables [L][2][Hkv], every entry different
TABLES = ("pow2", "real", "tight", "loose")
TABLE_ROWS = 17                    # rows of the oracle pass the `real` table is taken from


def scale_table(name: str, dt: str, kind: str) -> np.ndarray:
    cfg = config(name)
    shape = (cfg.num_hidden_layers, 2, cfg.num_key_value_heads)
    n = int(np.prod(shape))
    if kind == "pow2":                                             # 2^-12 .. 2^12, spread over the entries, all different
        if n > 25:                                                 # more entries than powers: all different inside a layer,
            per = 2 * cfg.num_key_value_heads                      # and from the same (k|v, head) entry of every other layer
            assert per <= 25 and cfg.num_hidden_layers <= 8
            ex = np.array([[(7 * i + 12 * l) % 25 - 12 for i in range(per)] for l in range(cfg.num_hidden_layers)])
            return (2.0 ** ex).astype(np.float32).reshape(shape)
        ex = np.round(np.linspace(-12, 12, n)).astype(np.int64)
        ex = ex[(np.arange(n) * 7) % n] if n % 7 else ex           # (neighbouring entries far apart)
        assert len(set(ex.tolist())) == n
        return (2.0 ** ex).astype(np.float32).reshape(shape)
    amax = np.abs(bits_value(oracle_kv_bits(name, dt, TABLE_ROWS), dt)).max(axis=(-1, -2))
    real = (amax.astype(np.float32) / np.float32(E4M3_MAX)).astype(np.float32)
    flat, seen = real.reshape(-1), {}
    for i, v in enumerate(flat.tolist()):                          # two heads with the same 16-bit amax: the k-th repeat gets
        k = seen.get(v, 0)                                         # (1 + k / 32) of head-room, so that every entry differs
        seen[v] = k + 1
        flat[i] = np.float32(v) * np.float32(1.0 + k / 32.0)
    assert real.shape == shape and len(set(real.ravel().tolist())) == n, (name, dt, "two entries of `real` are equal")
    if kind == "real":
        return real
    return real / np.float32(64.0) if kind == "tight" else real * np.float32(2.0 ** 14)


def swapped_tables(table: np.ndarray) -> Dict[str, np.ndarray]:
    """What a wrong index reads: K's and V's scales exchanged, two heads', two layers'."""
    return {"k<->v": table[:, ::-1], "heads": np.roll(table, 1, axis=2), "layers": np.roll(table, 1, axis=0)}


def tie_counts(bits16: np.ndarray, dtype: str, table: np.ndarray) -> Tuple[int, int]:
    """(ties that round up, ties that round down): elements whose fp32 product lies exactly between two e4m3 codes."""
    up = dn = 0
    for idx in np.ndindex(*table.shape):
        b = bits16[idx].ravel()
        sign, m, e, nan, inf = split16(b, dtype)
        mr, er = rcp32(float(table[idx]))
        q, E = m * mr, e + er
        bl = _bit_length(q)
        q, E = _rne_shift(q, np.maximum(bl - 24, 0)), E + np.maximum(bl - 24, 0)
        t = np.where(q > 0, _bit_length(q) - 1 + E, -1000)
        sh = np.maximum(t - 3, -9) - E
        ok = (q > 0) & (t <= 8) & (sh > 0) & (sh < 40) & ~nan & ~inf
        shc = np.clip(sh, 1, 40)
        tie = ok & ((q & ((np.int64(1) << shc) - 1)) == (np.int64(1) << (shc - 1)))
        odd = ((q >> shc) & 1) == 1
        up += int((tie & odd).sum())
        dn += int((tie & ~odd).sum())
    return up, dn


# ----------------------------------------------------------------------------- planted biases (OPT: k = v = 0 * h + bias)
PLANT_LAYERS, PLANT_HEADS, PLANT_D = 2, 4, 64                      # the OPT probe: 2 x 2 x 256 = 1024 planted values
PLANT_EXPS = (126, 127, 128, 129)  # four adjacent bf16 exponent fields: |x| in [0.5, 8)
PLANT_ROWS = (1, 5)


def planted_bf16() -> np.ndarray:
    """[L][2][H * D] bf16 patterns: 2 signs x 128 mantissas x 4 adjacent exponents, each once."""
    p = [(s << 15) | (e << 7) | m for s in (0, 1) for e in PLANT_EXPS for m in range(128)]
    rng = np.random.default_rng(5)
    return rng.permutation(np.array(p, dtype=np.int64)).reshape(PLANT_LAYERS, 2, PLANT_HEADS * PLANT_D)


def sweep_scales() -> List[float]:
    """One uniform power-of-two scale per step: from every planted value flushing to +-0 (8 / s <= 2^-10) to every one
    saturating (0.5 / s > 448)."""
    return [2.0 ** k for k in range(13, -11, -1)]


def fp16_boundaries() -> List[int]:
    """fp16 patterns (positive) at every boundary between two e4m3 codes at scale 1 - the midpoints of neighbouring codes,
    the half-denormal 2^-10 and the clamp edge 448 (all fp16 numbers) - each with its two fp16 neighbours."""
    vals = sorted({float(v) for v in e4m3_value(np.arange(0, MAX_BYTE + 1))})
    mids = [(a + b) / 2 for a, b in zip(vals[:-1], vals[1:])] + [448.0, 464.0, 480.0]
    out = []
    for v in mids:
        t = torch.tensor([v], dtype=torch.float16)
        assert float(t) == v, v
        b = int(to_bits(t)[0])
        out += [b - 1, b, b + 1]
    return sorted(set(out))


def planted_fp16() -> np.ndarray:
    """[L][2][H * D] fp16 patterns: every code boundary and its neighbours in both signs, +-65504, the smallest denormal,
    random finite patterns in the remaining slots."""
    pos = fp16_boundaries() + [0x7BFF, 0x0001]
    p = pos + [b | 0x8000 for b in pos]
    total = PLANT_LAYERS * 2 * PLANT_HEADS * PLANT_D
    assert len(p) <= total, len(p)
    rng = np.random.default_rng(6)
    fill = rng.integers(0, 65536, size=4 * total)
    fill = fill[(((fill >> 10) & 31) != 31) & (fill != 0x8000)][:total - len(p)]   # (0 + -0 is +0: the bias would not survive)
    return rng.permutation(np.concatenate([np.array(p, dtype=np.int64), fill])).reshape(PLANT_LAYERS, 2, PLANT_HEADS * PLANT_D)


def planted_state_dict(bits: np.ndarray, dt: str, n_layers: int = PLANT_LAYERS) -> Dict[str, torch.Tensor]:
    """The OPT probe's weights in `dt` with k_proj.weight = v_proj.weight = 0 and the K / V biases the given patterns
    [layers][2][H * D]: every stored element is rnd(0 + bias), the bias bit for bit, whatever the row."""
    cfg = planted_config(n_layers)
    sd = {k: v for k, v in S.cast_sd(S.probe_state_dict(OPT), S.DTYPES[dt]).items()
          if not k.startswith("model.decoder.layers.") or int(k.split(".")[3]) < n_layers}
    for l in range(cfg.num_hidden_layers):
        p = f"model.decoder.layers.{l}.self_attn."
        for j, n in enumerate("kv"):
            sd[p + f"{n}_proj.weight"] = torch.zeros_like(sd[p + f"{n}_proj.weight"])
            sd[p + f"{n}_proj.bias"] = from_bits(bits[l, j], dt)
    sd["lm_head.weight"] = sd["model.decoder.embed_tokens.weight"]
    return sd


def planted_config(n_layers: int = PLANT_LAYERS) -> ModelConfig:
    return ModelConfig(**dict(S.MODELS[OPT], num_hidden_layers=n_layers))


def planted_expected(bits: np.ndarray, dt: str, table: np.ndarray) -> np.ndarray:
    """[L][2][H][D] bytes of ONE arena row."""
    L = bits.shape[0]
    b = bits.reshape(L, 2, PLANT_HEADS, 1, PLANT_D)
    return e4m3_byte_table(b, dt, table)[:, :, :, 0, :]


SPECIALS = {"bf16": {"+inf": 0x7F80, "-inf": 0xFF80, "nan": 0x7FC0, "-nan": 0xFFC0, "nan_payload": 0x7F81},
            "fp16": {"+inf": 0x7C00, "-inf": 0xFC00, "nan": 0x7E00, "-nan": 0xFE00, "nan_payload": 0x7C01}}


def special_bits(dt: str) -> np.ndarray:
    """[1][2][H * D]: the specials at the first slots of every head (a 4-byte store group holds a NaN next to finite values
    and next to an infinity), ordinary values elsewhere."""
    base = (planted_bf16() if dt == "bf16" else planted_fp16())[:1].copy()
    sp = list(SPECIALS[dt].values())
    for j in range(2):
        for h in range(PLANT_HEADS):
            for i, b in enumerate(sp):
                base[0, j, h * PLANT_D + (i * 3 + h) % PLANT_D] = b
    return base
