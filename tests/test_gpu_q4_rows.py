"""The balanced GEMM on 4-bit weight records (gemm_q4_rows, `pytest -m gpu`): the stand-alone entry against a float64 product
of the format's definition - exactly - and the forward of a q4="rows" model against the same model on its bf16 copy."""
import ctypes as C

import numpy as np
import pytest
import torch

import q4_format as F
from sd_env import tunables
from test_gpu_w12 import CFG, _st, hip  # noqa: F401  (the w12 test's model)

pytestmark = pytest.mark.gpu
FILL = 12345.0
SHAPES = {(16 * 37, 128): 3, (16 * 300, 1024): 4, (1024, 2816): 5}        # (N, K) -> seed
ROWS = (1, 9, 16, 17, 40, 80)


@pytest.fixture(scope="module")
def operands(hip):
    """per (N, K): the records on the device, 80 rows of activations, and the float64 product of the definition"""
    out = {}
    for (N, K), seed in SHAPES.items():
        rng = np.random.default_rng(seed)
        q = rng.integers(0, 16, size=(N, K), dtype=np.uint8)
        z = rng.integers(0, 16, size=(N, K // 128), dtype=np.uint8)
        s = np.array([0x3E00, 0x3E80, 0x3F00, 0x3F80], dtype=np.uint16)[rng.integers(0, 4, size=(N, K // 128))]   # 2^-3 .. 1
        x = rng.integers(-4, 5, size=(80, K)).astype(np.float64)
        w = (F.weights(q, s, z).astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)
        nb = C.c_size_t()
        hip.L.check(hip.lib.sd_q4_bytes(N, K, C.byref(nb)), "sd_q4_bytes")
        rec = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
        tiled = torch.empty(N * K, dtype=torch.int16, device="cuda")
        dq, dz, ds = torch.from_numpy(q).cuda(), torch.from_numpy(z).cuda(), torch.from_numpy(s.view(np.int16)).cuda()
        hip.L.check(hip.lib.sd_pack_weight_q4(dq.data_ptr(), ds.data_ptr(), dz.data_ptr(), rec.data_ptr(), tiled.data_ptr(), N, K,
                                              _st()), "sd_pack_weight_q4")
        torch.cuda.synchronize()
        out[N, K] = (rec, torch.from_numpy(x).to(torch.bfloat16).cuda(), torch.from_numpy(x @ w.T))
    return out


# (slabs are whole records: the one-record shape has no cut in 4)
@pytest.mark.parametrize("M,N,K,slabs", [(M, N, K, S) for M in ROWS for N, K in SHAPES for S in (0, 1, 4) if S <= K // 128])
def test_gemm_is_integer_exact(hip, operands, M, N, K, slabs):
    """Products are multiples of 1/8 of magnitude <= 60 and K <= 2816: every fp32 partial sum is exact in any order, so the
    folded slabs EQUAL the float64 product.  Nothing is written past the slabs the plan chose or past out's M rows."""
    rec, x, want = operands[N, K]
    Mpad = (M + 15) // 16 * 16
    xt = torch.zeros(Mpad * K, dtype=torch.bfloat16, device="cuda")
    hip.L.check(hip.lib.sd_pack_activation_bf16(x[:M].contiguous().data_ptr(), xt.data_ptr(), M, K, _st()), "sd_pack_activation_bf16")
    cap = 16 * Mpad * N
    part = torch.full((cap + 4096,), FILL, dtype=torch.float32, device="cuda")
    out = torch.full((M * N + 4096,), FILL, dtype=torch.float32, device="cuda")
    splits = C.c_int(0)
    hip.L.check(hip.lib.sd_gemm_q4_rows(rec.data_ptr(), xt.data_ptr(), M, N, K, slabs, part.data_ptr(), cap, out.data_ptr(),
                                        C.byref(splits), _st()), "sd_gemm_q4_rows")
    torch.cuda.synchronize()
    S = splits.value
    assert 1 <= S <= 16 and (slabs == 0 or S == slabs)
    assert torch.equal(out[:M * N].cpu().double().reshape(M, N), want[:M])
    assert bool((out[M * N:] == FILL).all()) and bool((part[S * Mpad * N:] == FILL).all())


# ---- the forward pass ------------------------------------------------------------------------------------------------
PREFILL, SMALL, PASSES, WIDE = 7, (1, 5, 8), (9, 16, 17, 40, 64, 80), 96      # (a <= 8-row prefill: the same KV rows in every arm)
BAR_AT = (17, 40, 64)                     # the passes SD_GEMM_ROWS=0 sends another way on the bf16 copy
L = CFG.num_hidden_layers


def _run(model, **env):
    with tunables(SD_SMALL_PATH="0", **env):
        ses = model.new_session(512)
    ids = torch.from_numpy(np.random.default_rng(8).integers(3, CFG.vocab_size, size=512)).to(torch.int32).cuda()
    outs, counts, pos = {}, [0], 0
    for n in (PREFILL,) + SMALL + PASSES + (WIDE,):
        logits = ses.forward(ids[pos:pos + n], min(n, 9)).clone()
        outs[n] = (logits, ses.kv[:, :, :, pos:pos + n, :].float().clone())
        counts.append(ses.q4_launches())
        pos += n
    torch.cuda.synchronize()
    return outs, dict(zip((PREFILL,) + SMALL + PASSES + (WIDE,), np.diff(counts).tolist()))


def _gap(a, b):
    return tuple(float((a[i] - b[i]).abs().max()) for i in range(2))


@pytest.fixture(scope="module")
def arms(hip):
    mk = lambda q4: hip.engine.SpecDecModel.synthetic(CFG, seed=21, dtype=torch.bfloat16, max_pos=512, q4=q4)  # noqa: E731
    deq, rows = mk("dequantised"), mk("rows")
    ref, ref_n = _run(deq)
    alt, _ = _run(deq, SD_GEMM_ROWS="0")
    bar = tuple(max(_gap(ref[n], alt[n])[i] for n in BAR_AT) for i in range(2))
    print("bar (logits, KV):", bar)
    assert all(v == 0 for v in ref_n.values()) and bar[0] > 0 and bar[1] > 0
    return dict(deq=deq, rows=rows, ref=ref, bar=bar)


def test_forward_on_records(hip, arms):
    """q4="rows" against the same model under q4="dequantised": the same products in another order, so the bar is what the
    dequantised model shows between two of its OWN routes (default against SD_GEMM_ROWS=0, largest |difference| over the
    17-, 40- and 64-row passes), taken for logits and KV rows apart; the records arm stays within twice that at every pass.
    Measured (and printed on every run): bar 0.0625 on logits, 0.015625 on KV rows; the records arm differs by 0 / 0.0625 /
    0.0625 / 0.125 / 0.125 / 0.0625 on logits and 0 / 0.015625 / 0 / 0.015625 / 0.015625 / 0.015625 on KV rows at 9 / 16 / 17 /
    40 / 64 / 80 rows.
    Three record launches per layer on a 9..80-row pass, none on the 96-row prefill; the <= 8-row passes take what q4=True
    takes and give its logits bit for bit."""
    m = arms["rows"]
    assert m.q4_packed == {k: list(range(L)) for k in ("qkv", "gate_up", "down")} and m.w12_packed == {}
    got, n = _run(m)
    small, small_n = _run(hip.engine.SpecDecModel.synthetic(CFG, seed=21, dtype=torch.bfloat16, max_pos=512, q4=True))
    gaps = {p: _gap(got[p], arms["ref"][p]) for p in PASSES}
    print("records arm |difference| (logits, KV) per pass:", gaps, "bar:", arms["bar"])
    assert [n[p] for p in PASSES] == [3 * L] * len(PASSES) and n[WIDE] == 0
    for p in (PREFILL,) + SMALL:
        assert n[p] == small_n[p] > 0
        assert torch.equal(got[p][0].view(torch.int32), small[p][0].view(torch.int32)), f"logits of the {p}-row pass"
    for p in PASSES:
        assert gaps[p][0] <= 2 * arms["bar"][0] and gaps[p][1] <= 2 * arms["bar"][1], (p, gaps[p], arms["bar"])


def test_batch_forward_takes_the_route(hip, arms):
    """8 sessions x 5 rows = one 40-row pass: three record launches per layer (counted on the first session), same bar"""
    res = {}
    for arm in ("deq", "rows"):
        with tunables(SD_SMALL_PATH="0"):
            sess = [arms[arm].new_session(64) for _ in range(8)]
        seqs = [torch.from_numpy(np.random.default_rng(40 + i).integers(3, CFG.vocab_size, size=64)).to(torch.int32).cuda()
                for i in range(8)]
        for s, sq in zip(sess, seqs):
            s.forward(sq[:7], 0)                      # (<= 8 rows: both arms leave the same KV rows behind)
        n0 = sess[0].q4_launches()
        logits = hip.engine.batch_forward(sess, seqs, [5] * 8, [5] * 8).clone()
        kv = torch.stack([s.kv[:, :, :, 7:12, :].float() for s in sess])
        res[arm] = (logits, kv, sess[0].q4_launches() - n0)
    assert res["deq"][2] == 0 and res["rows"][2] == 3 * L
    gap = _gap(res["rows"], res["deq"])
    print("batch_forward |difference| (logits, KV):", gap, "bar:", arms["bar"])
    assert gap[0] <= 2 * arms["bar"][0] and gap[1] <= 2 * arms["bar"][1]
