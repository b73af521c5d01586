"""12-bit weight records on the GPU (`pytest -m gpu`): the packer and the expander against the host reference
(tests/w12_format.py), and the forward pass that streams records against the same model streaming bf16 - bit for bit, since
the records are decoded to the bf16 tile before the MFMA and nothing else changes."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import w12_format as F
from llmspeculativesampling_amd.config import ModelConfig

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import types
    from llmspeculativesampling_amd import _lib, engine
    return types.SimpleNamespace(lib=_lib.lib, L=_lib, engine=engine)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _pack(hip, tiles, N, K):
    """uint16 tiles [T][64][8] (the tiled layout as it lies in memory) -> (codes, meta, status, expanded tiles) off the GPU."""
    cb, mb = C.c_size_t(), C.c_size_t()
    hip.L.check(hip.lib.sd_w12_bytes(N, K, C.byref(cb), C.byref(mb)), "sd_w12_bytes")
    T = (N // 16) * (K // 32)
    assert (cb.value, mb.value) == (T * 768, T * 16) and tiles.shape == (T, 64, 8)
    w = torch.from_numpy(tiles.view(np.int16)).cuda()
    guard = 0x5A
    codes = torch.full((cb.value + 256,), guard, dtype=torch.uint8, device="cuda")
    meta = torch.full((mb.value + 256,), guard, dtype=torch.uint8, device="cuda")
    status = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    hip.L.check(hip.lib.sd_pack_weight_w12(w.data_ptr(), codes.data_ptr(), meta.data_ptr(), N, K, status.data_ptr(), _st()),
                "sd_pack_weight_w12")
    back = torch.full_like(w, -1)
    hip.L.check(hip.lib.sd_unpack_weight_w12(codes.data_ptr(), meta.data_ptr(), back.data_ptr(), N, K, _st()), "sd_unpack_weight_w12")
    torch.cuda.synchronize()
    assert bool((codes[cb.value:] == guard).all()) and bool((meta[mb.value:] == guard).all())     # nothing past the arrays
    c = codes[:cb.value].cpu().numpy().view(np.uint32).reshape(T, 64, 3)
    m = meta[:mb.value].cpu().numpy().view(np.uint32).reshape(T, 4)
    return c, m, int(status.item()), w, back


@pytest.mark.parametrize("case", ["planted", "plain"])
def test_pack_unpack_round_trip(hip, case):
    """sd_pack_weight_w12 -> sd_unpack_weight_w12 gives the input back, the GPU's records decode to the input with the
    host decoder, and they are the host packer's records byte for byte (one format, two definitions)."""
    if case == "planted":
        N, K, tiles = F.PLANTED_N, F.PLANTED_K, F.planted_tiles()
    else:
        N, K, tiles = 64, 1024, F.normal_tiles(4 * 32, 1024, seed=5)
    c, m, status, w, back = _pack(hip, tiles, N, K)
    assert status == 0
    assert torch.equal(back, w)
    assert torch.equal(torch.from_numpy(F.unpack(c, m).view(np.int16)), w.cpu())
    rc, rm, ok = F.pack(tiles)
    assert ok and np.array_equal(c, rc) and np.array_equal(m, rm)


def test_seven_escapes_report_unpackable(hip):
    c, m, status, _, _ = _pack(hip, F.seven_escape_tiles(), F.PLANTED_N, F.PLANTED_K)
    assert status == 1
    assert (m[6, 0] >> 8) & 7 == 6


# ---- the forward pass ------------------------------------------------------------------------------------------------
CFG = ModelConfig(arch="llama", vocab_size=4096, hidden_size=1024, intermediate_size=2816, num_hidden_layers=2,
                  num_attention_heads=8, num_key_value_heads=8, max_position_embeddings=512, rms_norm_eps=1e-5)
PREFILL, PASSES, WIDE = 37, (1, 2, 3, 4, 5, 8), 9


def _zero_at(t, r0, c0, cells):
    for r, c in cells:
        t[r0 + r, c0 + c] = 0
    return t


def _planted(name, t):
    """a tile with exactly six escapes and a zeroed 16-row strip inside w_down and w_gate_up of layer 0 (the fused gate/up
    layout interleaves 8 gate rows with the same 8 up rows: its tile row j is rows 8j..8j+7 of both)."""
    six = ((0, 0), (0, 7), (3, 8), (5, 16), (7, 24), (7, 31))
    if name == "model.layers.0.mlp.down_proj.weight":
        t[16:32] = 0
        _zero_at(t, 32, 64, six)
    if name in ("model.layers.0.mlp.gate_proj.weight", "model.layers.0.mlp.up_proj.weight"):
        t[16:24] = 0
    if name == "model.layers.0.mlp.gate_proj.weight":
        _zero_at(t, 40, 32, six)
    return t


def _seven(name, t):
    if name == "model.layers.0.mlp.down_proj.weight":
        _zero_at(t, 32, 64, ((0, 0), (0, 7), (3, 8), (5, 16), (7, 24), (7, 31), (15, 31)))
    return t


def _run(hip, w12, transform):
    """prefill, the <= 8-row passes, one 9-row pass: (logits, written KV rows) of every pass and the records-launch counter
    after each.  hidden 1024 is a width the small-model path (<= 4 rows, hidden <= 2048, bf16 weights only) would take:
    SD_SMALL_PATH=0, sampled when the session is created, keeps the 1..4-row passes on the route of the 13b target."""
    m = hip.engine.SpecDecModel.synthetic(CFG, seed=21, dtype=torch.bfloat16, max_pos=128, transform=transform, w12=w12)
    old = os.environ.get("SD_SMALL_PATH")
    os.environ["SD_SMALL_PATH"] = "0"
    try:
        ses = m.new_session(128)
    finally:
        if old is None:
            del os.environ["SD_SMALL_PATH"]
        else:
            os.environ["SD_SMALL_PATH"] = old
    ids = torch.from_numpy(np.random.default_rng(8).integers(3, CFG.vocab_size, size=128)).to(torch.int32).cuda()
    outs, counts, pos = [], [], 0
    for n in (PREFILL,) + PASSES + (WIDE,):
        logits = ses.forward(ids[pos:pos + n], min(n, 9)).clone()
        outs.append((logits, ses.kv[:, :, :, pos:pos + n, :].clone()))
        counts.append(ses.w12_launches())
        pos += n
    torch.cuda.synchronize()
    return m.w12_packed, outs, counts


@pytest.fixture(scope="module")
def bf16_runs(hip):
    return {name: _run(hip, False, tr) for name, tr in (("natural", None), ("planted", _planted), ("seven", _seven))}


def _same(a, b):
    for i, ((la, ka), (lb, kb)) in enumerate(zip(a, b)):
        assert torch.equal(la.view(torch.int32), lb.view(torch.int32)), f"logits of pass {i}"
        assert torch.equal(ka.view(torch.int16), kb.view(torch.int16)), f"KV rows of pass {i}"


@pytest.mark.parametrize("case", ["natural", "planted"])
def test_forward_on_records_is_bit_identical(hip, bf16_runs, case):
    """2 layers of hidden 1024 / intermediate 2816 (a ragged last k-group in the down projection): rows 1, 2, 3, 4 | 5 | 8
    reach the three conversion widths of the norm-on-load GEMM; every pass's logits and KV rows equal the bf16 model's.
    Records are read by QKV of layer 1, gate/up of both layers and down of layer 0: four launches per <= 8-row pass, none in
    the prefill, none in the 9-row pass, none on the bf16 model."""
    packed0, ref, counts0 = bf16_runs[case]
    assert packed0 == {} and counts0 == [0] * len(counts0)
    packed, got, counts = _run(hip, True, {"natural": None, "planted": _planted}[case])
    assert packed == {"qkv": [1], "gate_up": [0, 1], "down": [0]}
    _same(got, ref)
    assert counts[0] == 0                                                     # prefill reads bf16
    per_pass = np.diff(counts).tolist()
    assert per_pass[:len(PASSES)] == [4] * len(PASSES)
    assert per_pass[len(PASSES)] == 0                                         # 9 rows: bf16


def test_unpackable_matrix_stays_bf16(hip, bf16_runs):
    """A seven-escape tile in layer 0's down projection: that matrix keeps bf16, the others are packed, results the same."""
    _, ref, _ = bf16_runs["seven"]
    packed, got, counts = _run(hip, True, _seven)
    assert packed == {"qkv": [1], "gate_up": [0, 1]}
    _same(got, ref)
    assert np.diff(counts).tolist() == [3] * len(PASSES) + [0]
