"""4-bit group-quantised weight records on the GPU (`pytest -m gpu`): packer and expander against the host definition
(tests/q4_format.py), and the forward pass that streams records against the same model reading its bf16 copy - bit for bit,
since a record decodes to the bf16 tile before the MFMA and the k-steps keep their order."""
import ctypes as C

import numpy as np
import pytest
import torch

import q4_format as F
from sd_env import tunables
from test_gpu_w12 import CFG, PREFILL, PASSES, WIDE, _same, _st, hip  # noqa: F401  (the w12 test's model and passes)

pytestmark = pytest.mark.gpu
GUARD = 0x5A


@pytest.mark.parametrize("case", ["planted", "random"])
def test_pack_unpack_numpy(hip, case):
    q, s, z = F.planted_case() if case == "planted" else F.random_case(64, 1024, seed=9)
    N, K = q.shape
    nb = C.c_size_t()
    hip.L.check(hip.lib.sd_q4_bytes(N, K, C.byref(nb)), "sd_q4_bytes")
    assert nb.value == (N // 16) * (K // 128) * 1088
    dq, dz = torch.from_numpy(q).cuda(), torch.from_numpy(z).cuda()
    ds = torch.from_numpy(s.view(np.int16)).cuda()
    rec = torch.full((nb.value + 256,), GUARD, dtype=torch.uint8, device="cuda")
    tiled = torch.full((N * K + 128,), GUARD << 8 | GUARD, dtype=torch.int16, device="cuda")
    back = torch.full_like(tiled, GUARD << 8 | GUARD)
    hip.L.check(hip.lib.sd_pack_weight_q4(dq.data_ptr(), ds.data_ptr(), dz.data_ptr(), rec.data_ptr(), tiled.data_ptr(), N, K, _st()),
                "sd_pack_weight_q4")
    hip.L.check(hip.lib.sd_unpack_weight_q4(rec.data_ptr(), back.data_ptr(), N, K, _st()), "sd_unpack_weight_q4")
    torch.cuda.synchronize()
    want = torch.from_numpy(F.tiles(q, s, z).reshape(-1).view(np.int16))
    assert torch.equal(back[:N * K].cpu(), want)                               # the decoder's w is the definition's
    assert torch.equal(tiled, back)                                            # the packer's copy, and both guards
    assert bool((tiled[N * K:] == (GUARD << 8 | GUARD)).all()) and bool((rec[nb.value:] == GUARD).all())
    assert np.array_equal(rec[:nb.value].cpu().numpy().view(np.uint32).reshape(-1, F.REC_DWORDS), F.records(q, s, z))


def _run(hip, q4):
    """test_gpu_w12._run on a q4 model: (logits, written KV rows) and both records-launch counters after every pass."""
    m = hip.engine.SpecDecModel.synthetic(CFG, seed=21, dtype=torch.bfloat16, max_pos=128, q4=q4)
    with tunables(SD_SMALL_PATH="0"):
        ses = m.new_session(128)
    ids = torch.from_numpy(np.random.default_rng(8).integers(3, CFG.vocab_size, size=128)).to(torch.int32).cuda()
    outs, counts, pos = [], [], 0
    for n in (PREFILL,) + PASSES + (WIDE,):
        logits = ses.forward(ids[pos:pos + n], min(n, 9)).clone()
        outs.append((logits, ses.kv[:, :, :, pos:pos + n, :].clone()))
        counts.append((ses.q4_launches(), ses.w12_launches()))
        pos += n
    torch.cuda.synchronize()
    return m, outs, counts


def test_forward_on_records_is_bit_identical(hip):
    """hidden 1024 / intermediate 2816: the 32 k-steps of QKV and gate/up split evenly over the waves (every wave starts on a
    record), the down projection's 22 groups do not (partial records at slab and wave boundaries).  Rows 1..5 and 8 reach the
    three conversion widths; 9 rows and the prefill read the bf16 copy."""
    ref_m, ref, ref_counts = _run(hip, "dequantised")
    assert ref_m.q4_packed == {}
    assert all(c[0] == 0 for c in ref_counts)
    m, got, counts = _run(hip, True)
    assert m.q4_packed == {"qkv": [1], "gate_up": [0, 1], "down": [0]} and m.w12_packed == {}
    assert m.streamed_weight_bytes < m.weight_bytes == ref_m.weight_bytes
    _same(got, ref)
    q4n = [c[0] for c in counts]
    assert q4n[0] == 0 and np.diff(q4n).tolist() == [4] * len(PASSES) + [0]
    assert all(c[1] == 0 for c in counts)


def test_speculative_sampling_end_to_end(hip):
    """the tiny draft (at the target's vocabulary) and the q4 target: same seed, same token ids on records as on the bf16 copy"""
    import dataclasses
    from llmspeculativesampling_amd.sampling import speculative_sampling
    from llmspeculativesampling_amd.config import load_config
    dcfg = dataclasses.replace(load_config("tiny-llama-draft"), vocab_size=CFG.vocab_size)
    draft = hip.engine.SpecDecModel.synthetic(dcfg, seed=3, dtype=torch.bfloat16, max_pos=128)
    prompt = torch.from_numpy(np.random.default_rng(2).integers(3, 250, size=(1, 8))).cuda()
    out = []
    for q4 in (True, "dequantised"):
        target = hip.engine.SpecDecModel.synthetic(CFG, seed=21, dtype=torch.bfloat16, max_pos=128, q4=q4)
        torch.manual_seed(7)                           # (the host noise is torch's CPU generator: both arms from one state)
        with tunables(SD_SMALL_PATH="0"):
            out.append(speculative_sampling(prompt, draft, target, 2, 0, max_len=16, gamma=4, random_seed=7))
    assert torch.equal(out[0], out[1]) and out[0].shape[1] > prompt.shape[1]
