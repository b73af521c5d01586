"""Adversarial logit rows for the sampler kernels and what the oracle says about them (CPU only, no GPU needed).

Shared by tests/test_sampler_rows_cpu.py (the conditions on the inputs: cut margin, share of denominator-sensitive 16-bit
cases, coverage of the (route, family) table) and tests/test_gpu_sampler_routes.py (the kernels against these rows).
Nothing here comes from the kernels: rows are seeded, expectations are oracle.sampling_ref's."""
import numpy as np
import torch

import oracle
import oracle.sampling_ref as SR
from golden_io import logits_row

NEG = float("-inf")
DTYPES = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}
DT_MODE = {0: 0, 1: 16, 2: 32}                      # SD_NORM_DT_BF16 / SD_NORM_DT_F16

# route-word bits (include/specdec.h, SD_ROUTE_*)
A, B = 0x1, 0x2
A_CHUNK, A_TOTAL, B_TILE, B_CAND, A_SECOND = 0x4, 0x8, 0x10, 0x20, 0x40
PRE, PRE_CAP, BISECT, P_LIST, P_MASS, CUT_IDX, STAGED, ERROR, LIST = 0x80, 0x100, 0x200, 0x400, 0x800, 0x1000, 0x2000, 0x4000, 0x8000
ROUTE_NAMES = {A: "A", B: "B", A_CHUNK: "A_CHUNK_CAP", A_TOTAL: "A_TOTAL_CAP", B_TILE: "B_TILE_CAP", B_CAND: "B_CAND_CAP",
               A_SECOND: "A_SECOND", PRE: "PREFILTER", PRE_CAP: "PREFILTER_CAP", BISECT: "TOPK_BISECT", P_LIST: "TOPP_LIST",
               P_MASS: "TOPP_MASS", CUT_IDX: "CUT_IDX", STAGED: "STAGED", ERROR: "ERROR", LIST: "LIST"}
LDS_ROW_LIMIT = 35840


def route_str(w):
    return "|".join(n for b, n in ROUTE_NAMES.items() if w & b) + f"|kept={w >> 16}"


# --------------------------------------------------------------------------------------------- row families
def _rng(seed, V):
    return np.random.default_rng([seed, V, 77])


def gauss(seed, V, scale=3.0):
    """family 6: plain fp32 Gaussian rows (no two logits equal)"""
    return logits_row(seed, V, scale)


def bf16_valued(seed, V, scale=3.0):
    """family 1: the headline input - a bf16 head's logits widened to fp32 (many exact ties)"""
    return logits_row(seed, V, scale).to(torch.bfloat16).float()


def _ids(rng, V, n, where):
    """n distinct token ids: 'spread' over the row; 'chunk' inside ONE of the 16 chunks of the workspace kernel (chunk 7);
    'tiles' a run of whole 16-column tiles."""
    if where == "spread":
        return rng.choice(V, size=n, replace=False)
    csz = ((V // 4 + 15) // 16) * 4
    if where == "chunk":
        assert n <= csz
        return 7 * csz + rng.choice(csz, size=n, replace=False)
    start = (int(rng.integers(0, (V - n - 32) // 16)) * 16)
    return np.arange(start, start + n)


def plateau_max(seed, V, n, where="spread", top=9.0):
    """family 2a: n equal maxima over a Gaussian floor that stays below them"""
    rng = _rng(seed, V)
    x = np.minimum(logits_row(seed, V, 2.0).numpy()[0], np.float32(top - 2.5))
    x[_ids(rng, V, n, where)] = np.float32(top)
    return torch.from_numpy(x[None])


def plateau_kth(seed, V, n, k, where="spread"):
    """family 2b: k - 1 distinct larger values, then n equal values occupying ranks k .. k + n - 1"""
    rng = _rng(seed, V)
    x = np.minimum(logits_row(seed, V, 2.0).numpy()[0], np.float32(5.0))
    ids = _ids(rng, V, n, where)
    x[ids] = np.float32(8.0)
    free = np.setdiff1d(np.arange(V), ids)
    top = rng.choice(free, size=k - 1, replace=False)
    x[top] = (np.float32(8.5) + np.float32(0.125) * np.arange(k - 1, dtype=np.float32))
    return torch.from_numpy(x[None])


def masked(seed, V, kind):
    """family 3: 'filtered' = top_k_top_p_filter's own output (k = 20: V - 20 entries -inf); 'few' = 7 finite entries (the
    k-th largest is -inf for k > 7); 'half' = every second entry -inf (every fast entry still accepts the row); 'tail' = the last 1/16 of the row (last chunk and last tiles) all -inf"""
    x = logits_row(seed, V, 3.0)
    if kind == "filtered":
        return oracle.top_k_top_p_filter(x, 20, 0.0)
    if kind == "few":
        rng = _rng(seed, V)
        y = torch.full((1, V), NEG)
        ids = torch.from_numpy(rng.choice(V, size=7, replace=False))
        y[0, ids] = x[0, ids]
        return y
    y = x.clone()
    if kind == "half":
        y[0, ::2] = NEG
        return y
    y[0, V - ((V // 4 + 15) // 16) * 4:] = NEG
    return y


def same_slot(seed, V, n=20):
    """n strong tokens whose ids all agree modulo 1024 (one per-thread partial of the dense residual sum) over a low floor"""
    rng = _rng(seed, V)
    x = np.minimum(logits_row(seed, V, 2.0).numpy()[0], np.float32(3.0))
    ids = int(rng.integers(0, V % 1024 or 1024)) + 1024 * rng.choice(V // 1024, size=n, replace=False)
    x[ids] = np.float32(8.0) + rng.standard_normal(n).astype(np.float32)
    return torch.from_numpy(x[None])


def wide_range(seed, V, clip=True):
    """family 4: five kept entries more than 104 below the maximum - their probability underflows to 0 or a denormal.
    The floor is clipped, so that hundreds of equal values tie at the 20th rank (clip=False: a distinct floor, and k = 20
    keeps exactly 20 tokens, 8 of them with probability 0)"""
    rng = _rng(seed, V)
    x = logits_row(seed, V, 2.0).numpy()[0]
    x = (np.minimum(x, np.float32(4.0)) if clip else x) - np.float32(150.0)
    ids = rng.choice(V, size=12, replace=False)
    x[ids[:7]] = np.float32(20.0) - np.arange(7, dtype=np.float32)
    x[ids[7:]] = np.float32(20.0) - np.float32(100.0) - np.float32(1.5) * np.arange(5, dtype=np.float32)
    return torch.from_numpy(x[None])


def error_row(seed, V, what, where):
    """family 5: one NaN / one +inf at `where` (chunk0, chunk15, last, far_tile), or an all -inf row"""
    if what == "allneg":
        return torch.full((1, V), NEG)
    x = logits_row(seed, V, 3.0)
    csz = ((V // 4 + 15) // 16) * 4
    if where == "far_tile":
        pos = int(torch.argmin(x[0].view(-1, 16).max(1)[0])) * 16 + 5 if V % 16 == 0 else int(torch.argmin(x[0]))
    else:
        pos = {"chunk0": 3, "chunk15": 15 * csz + 1, "last": V - 1}[where]
    x[0, pos] = float("nan") if what == "nan" else float("inf")
    return x


# --------------------------------------------------------------------------------------------- oracle expectations
class stable_ties:
    def __init__(self, on=True):
        self.on = on

    def __enter__(self):
        self.old = SR.STABLE_TIES
        SR.STABLE_TIES = self.on

    def __exit__(self, *a):
        SR.STABLE_TIES = self.old


def as_dtype(x, dt):
    """the row as the kernel's dtype mode sees it: values of the 16-bit dtype, carried as fp32"""
    return x.to(DTYPES[dt])


def expected(x, T, k, p, dt, filter_only=False):
    """(stable, unstable) oracle results as fp32 rows, or None where the reference raises 'norm logits error'."""
    xd = as_dtype(x, dt)
    out = []
    for st in (True, False):
        with stable_ties(st):
            try:
                if filter_only:
                    out.append(oracle.top_k_top_p_filter(xd / T, k, p).float())
                else:
                    out.append(oracle.norm_logits(xd, T, k, p).float())
            except RuntimeError as e:
                assert "norm logits error" in str(e)
                return None
    return out[0], out[1]


def scaled(x, T, dt):
    return (as_dtype(x, dt) / T).float()


def cut_margin(x, T, k, p):
    """fp32 rows: distance of the fp64 cumulative mass from top_p on either side of the kept boundary (inf when no cut)"""
    if not p > 0:
        return float("inf")
    z = (x / T)[0]
    if k > 0:
        z = z.masked_fill(z < torch.topk(z, min(k, z.numel()))[0][-1], NEG)
    srt = torch.sort(z, descending=True, stable=True)[0].double()
    c = torch.cumsum(torch.softmax(srt, 0), 0)
    over = (c.float() > p).nonzero()
    if over.numel() == 0:
        return float("inf")
    j = int(over[0])                                   # first prefix past top_p: token j is the last one kept
    nfin = int(torch.isfinite(srt).sum())
    if j + 1 >= nfin or srt[j + 1] == srt[j]:          # nothing dropped, or the cut separates tokens of EQUAL probability
        return float("inf")
    d = abs(float(c[j]) - p)
    if j >= 1:
        d = min(d, abs(float(c[j - 1]) - p))
    return d


def lowprec_alternative(x, T, k, p, dt):
    """16-bit rows: the probability row the reference would give if its fp32 softmax denominator were one ulp lower / higher,
    where that moves the kept set (else None) - the device of fixture G10.  Stable ties."""
    if not p > 0:
        return None
    dtype = DTYPES[dt]
    z = (as_dtype(x, dt) / T)
    if k > 0:
        z = z.masked_fill(z < torch.topk(z, min(k, z.size(-1)))[0][:, -1:], NEG)
    srt, order = torch.sort(z, descending=True, stable=True)
    e = torch.exp(srt.float() - srt.float().max())
    d0 = e.sum(dim=-1, keepdim=True)
    with stable_ties(True):
        base = oracle.top_k_top_p_filter(z, 0, p)
    alts = []
    for d in (torch.nextafter(d0, torch.zeros_like(d0)), torch.nextafter(d0, torch.full_like(d0, float("inf")))):
        cs = torch.cumsum((e / d).to(dtype), dim=-1)
        rem = cs > p
        rem[..., 1:] = rem[..., :-1].clone()
        rem[..., 0] = False
        zz = z.clone()
        zz[0, order[rem]] = NEG
        if not torch.equal(torch.isfinite(zz), torch.isfinite(base)):
            alts.append(torch.log_softmax(zz, dim=1).exp().float())
    return alts or None


def tile_maxima(x):
    """[V / 16] maxima of the row's 16-column tiles, NaN where a tile holds one (what the head's epilogue leaves)"""
    t = x[0].view(-1, 16)
    m = t.max(1)[0]
    return torch.where(torch.isnan(t).any(1), torch.full_like(m, float("nan")), m)[None].contiguous()


# --------------------------------------------------------------------------------------------- the case table
# entry: how the launch is made - "ws" (workspace: route A where its conditions hold), "tile" (tile maxima: route B),
# "plain" (neither: route C for V <= 35840, D above).  Every case runs through every entry listed and the results must be
# bit-equal to each other.  want[entry] = (bits that must be set, bits that must be clear) in the row's route word.
HARNESS = (1.0, 20, 0.9)
FAST_ANY = A | B | PRE


def _fast(V, plain_only=False, k=20):
    """route expectations of a row that every fast entry accepts (k in 1..64, list top-p).  Every chunk of the workspace
    kernel keeps at least k candidates, so from k = 9 on (16 * k > 128) the second-level prefilter runs; at k = 1 a row
    without ties at its maximum gives 16.  At k = 64 the in-kernel prefilter's threshold is each wave's SMALLEST per-thread
    maximum: more than 1024 candidates pass on any Gaussian row and it hands over to the general top-k."""
    st = STAGED if V <= LDS_ROW_LIMIT else 0
    if k == 64:
        w = {"plain": (PRE | PRE_CAP | BISECT | P_LIST | st, A | B | P_MASS | (0 if st else STAGED))}
    else:
        w = {"plain": (PRE | P_LIST | st, A | B | PRE_CAP | BISECT | P_MASS | (0 if st else STAGED))}
    if not plain_only:
        sec = (A_SECOND, 0) if k >= 9 else (0, A_SECOND)
        w["ws"] = (A | P_LIST | sec[0], A_CHUNK | A_TOTAL | PRE | BISECT | P_MASS | STAGED | sec[1])
        if k == 64:                                   # 16 chunks x >= 64 candidates: past the total cap on any dense row
            w["ws"] = (A | A_TOTAL | w["plain"][0], A_CHUNK | P_MASS)
        w["tile"] = (B | P_LIST, B_TILE | B_CAND | PRE | BISECT | P_MASS | STAGED)
    return w


def _nop(want):
    """the same expectations for top_p == 0 (no top-p bit at all)"""
    return {e: (s & ~P_LIST, c | P_LIST | P_MASS) for e, (s, c) in want.items()}


CASES = []


def case(id, family, make, V, setting, dt=0, want=None, **kw):
    T, k, p = setting
    CASES.append(dict(id=id, family=family, make=make, V=V, T=T, k=k, p=p, dt=dt, want=want, **kw))


def _build():
    V0 = 32000
    # ---- families 1 and 6 through A / B / C (and D above the LDS limit), harness setting and the k-only settings
    for fam, mk, seeds in (("bf16_valued", bf16_valued, (100, 101, 102)), ("gauss", gauss, (103, 104, 100))):
        for V in (4096, 8192, 32000, 35840, 50272, 65536):
            for s in seeds[:2 if V != 32000 else 3]:
                for sc in ((3.0, 12.0) if V == 32000 and s == seeds[0] else (3.0,)):
                    case(f"{fam}_V{V}_s{s}_x{sc:g}", fam, lambda s=s, V=V, sc=sc, mk=mk: mk(s, V, sc), V, HARNESS, want=_fast(V))
        case(f"{fam}_k1", fam, lambda mk=mk, s=seeds[0]: mk(s, V0), V0, (1.0, 1, 0.0), want=_nop(_fast(V0, k=1)))
        case(f"{fam}_k64", fam, lambda mk=mk, s=seeds[1]: mk(s, V0), V0, (1.0, 64, 0.0), want=_nop(_fast(V0, k=64)))
        case(f"{fam}_k64_p05", fam, lambda mk=mk, s=seeds[1]: mk(s, V0), V0, (1.0, 64, 0.5), want=_fast(V0, k=64))
        # ---- sizes that keep a fast entry out: scalar loads (V % 4), V % 16 for the tiles, V > 65536
        for V in (4100, 32016, 35844, 65552):
            w = _fast(V)
            if V > 65536:
                w["ws"] = w["tile"] = w["plain"]
            elif V % 16:
                w["tile"] = w["plain"]                        # tiles declined: that launch has no workspace either
            case(f"{fam}_V{V}", fam, lambda mk=mk, s=seeds[0], V=V: mk(s, V), V, HARNESS, want=w)
        for V in (32001, 50257):
            w = _fast(V, plain_only=True)
            w["ws"] = w["plain"]
            case(f"{fam}_V{V}", fam, lambda mk=mk, s=seeds[0], V=V: mk(s, V), V, HARNESS, want=w)
        w = _fast(128256, plain_only=True)
        w["ws"] = w["plain"]
        case(f"{fam}_V128256", fam, lambda mk=mk, s=seeds[0]: mk(s, 128256), 128256, HARNESS, want=w)
        # ---- E: no top-k / k > 64
        for V in (32000, 50257, 128256):
            st = STAGED if V <= LDS_ROW_LIMIT else 0
            e = {"plain": (P_MASS | st, FAST_ANY | BISECT | P_LIST | (CUT_IDX if fam == "gauss" else 0))}
            e["ws"] = e["plain"]
            case(f"{fam}_E_mass_V{V}", fam, lambda mk=mk, s=seeds[2], V=V: mk(s, V), V, (0.7, 0, 0.9), want=e)
        e = {"plain": (BISECT | P_LIST | STAGED, FAST_ANY | P_MASS), "ws": (BISECT | P_LIST | STAGED, FAST_ANY | P_MASS)}
        case(f"{fam}_E_k65", fam, lambda mk=mk, s=seeds[0]: mk(s, V0), V0, (1.0, 65, 0.0), want=_nop(e))
        e = {"plain": (BISECT | P_LIST | STAGED, FAST_ANY | P_MASS)}
        case(f"{fam}_E_k65_p05", fam, lambda mk=mk, s=seeds[1]: mk(s, V0), V0, (1.0, 65, 0.5), want=e)
        e = {"plain": (BISECT | P_MASS | STAGED, FAST_ANY | P_LIST)}
        case(f"{fam}_E_k2000", fam, lambda mk=mk, s=seeds[0]: mk(s, V0), V0, (1.0, 2000, 0.99), want=e)
        e = {"plain": (STAGED, FAST_ANY | BISECT | P_LIST | P_MASS)}
        case(f"{fam}_E_none", fam, lambda mk=mk, s=seeds[0]: mk(s, V0), V0, (1.0, 0, 0.0), want=e)
        e = {"plain": (BISECT | STAGED, FAST_ANY | P_LIST | P_MASS)}
        case(f"{fam}_E_kV", fam, lambda mk=mk, s=seeds[0]: mk(s, 8192), 8192, (1.0, 8192, 0.0), want=e)

    # ---- family 2: plateaus.  n equal maxima (k = 20, p = 0.9): the k-th value IS the plateau, every member survives top-k
    # and the top-p cut falls inside the run.  What each entry does with n candidates >= its threshold:
    #   A spread: <= 192 per chunk; n <= 1024 in all -> A (second prefilter above 128), else total cap -> in-kernel prefilter
    #   A chunk : n > 192 in chunk 7 -> per-chunk cap -> in-kernel prefilter
    #   B       : n <= 1024 -> B; n > 1024 spread -> > 1024 tiles qualify (tile cap); packed tiles -> candidate cap
    #   in-kernel prefilter: n <= 1024 -> list; else cap -> general top-k; > 1024 finite survivors -> mass bisection + cut_idx
    for n in (2, 63, 64, 65, 127, 128, 129, 192, 193, 1024, 1025, 1500):
        for where in ("spread", "chunk", "tiles"):
            big = n > 1024
            st = STAGED
            plain = (PRE | P_LIST | st, PRE_CAP | BISECT | P_MASS) if not big else \
                    (PRE | PRE_CAP | BISECT | P_MASS | CUT_IDX | st, P_LIST | LIST)
            tail_set, tail_clr = plain
            if where != "spread" and n > 192:                  # (a run of whole tiles lies inside one chunk as well)
                ws = (A | A_CHUNK | tail_set, A_TOTAL | A_SECOND | tail_clr)
            elif big:
                ws = (A | A_TOTAL | tail_set, A_CHUNK | tail_clr)
            else:
                ws = (A | P_LIST | A_SECOND, A_CHUNK | A_TOTAL | PRE | BISECT | P_MASS)
            if not big:
                tile = (B | P_LIST, B_TILE | B_CAND | PRE | BISECT | P_MASS)
            else:
                # n members sit in at most 1024 tiles: the candidate cap, not the tile cap (that one needs a threshold of
                # -inf: the masked rows).  B works without a staged row; after it gives up the row is re-read from memory
                # (1500 ids drawn over the row's 2000 tiles do occupy more than 1024 of them)
                cap, other = (B_TILE, B_CAND) if (where == "spread" and n == 1500) else (B_CAND, B_TILE)
                tile = (B | cap | (tail_set & ~STAGED), other | tail_clr | STAGED)
            lowprec = (n in (64, 129, 1025) and where == "spread") or (n == 193 and where == "chunk") or (n == 1025 and where == "tiles")
            for dt in ((0, 1, 2) if lowprec else (0,)):
                case(f"plateau_max_n{n}_{where}_dt{dt}", "plateau", lambda n=n, where=where: plateau_max(500 + n, V0, n, where), V0,
                     HARNESS, dt=dt, want={"plain": plain, "ws": ws, "tile": tile})
    case("plateau_max_n64_D", "plateau", lambda: plateau_max(565, 50272, 64, "spread"), 50272, HARNESS, want=_fast(50272))
    big_d = (PRE | PRE_CAP | BISECT | P_MASS | CUT_IDX, STAGED | P_LIST | LIST)
    case("plateau_max_n1500_D", "plateau", lambda: plateau_max(564, 50272, 1500, "spread"), 50272, HARNESS,
         want={"plain": big_d, "ws": (A | A_TOTAL | big_d[0], big_d[1]), "tile": (B | B_TILE | big_d[0], big_d[1])})
    # n equal values at the k-th rank, p = 0: all n survive (ties at the k-th value stay), no top-p
    # (n = 108 / 109 / 110 keep 127 / 128 / 129 tokens: the last candidate list that is written, and the first that is not)
    for n in (2, 64, 65, 108, 109, 110, 128, 129, 193, 1024, 1025, 1500):
        for where in (("spread", "chunk") if n in (193, 1500) else ("spread",)):
            tot = n + 19
            big = tot > 1024
            plain = (PRE | STAGED, PRE_CAP | BISECT | P_LIST | P_MASS) if not big else (PRE | PRE_CAP | BISECT | STAGED, P_LIST | P_MASS | LIST)
            if where == "chunk" and n > 192:
                ws = (A | A_CHUNK | plain[0], A_TOTAL | plain[1])
            elif big:
                ws = (A | A_TOTAL | plain[0], A_CHUNK | plain[1])
            else:
                ws = (A | A_SECOND, A_CHUNK | A_TOTAL | PRE | BISECT | P_LIST | P_MASS)
            if not big:                                # the list is written up to 128 kept tokens and not beyond
                lst = (LIST, 0) if tot <= 128 else (0, LIST)
                plain = (plain[0] | lst[0], plain[1] | lst[1])
                if not (where == "chunk" and n > 192):
                    ws = (ws[0] | lst[0], ws[1] | lst[1])
            cap, other = (B_TILE, B_CAND) if (where == "spread" and n == 1500) else (B_CAND, B_TILE)
            tile = (B | lst[0], B_TILE | B_CAND | PRE | BISECT | lst[1]) if not big else (B | cap | PRE | PRE_CAP | BISECT, other | STAGED | LIST)
            for dt in ((0, 1) if n in (128, 1025) else (0,)):
                case(f"plateau_kth_n{n}_{where}_dt{dt}", "plateau", lambda n=n, where=where: plateau_kth(700 + n, V0, n, 20, where), V0,
                     (1.0, 20, 0.0), dt=dt, want={"plain": plain, "ws": ws, "tile": tile})
    # the same rows under the wide settings: list top-p in E, mass bisection with and without cut_idx
    # (without top-k a list needs <= 1024 FINITE entries - the masked rows below; a plateau gets one behind the general top-k)
    e = {"plain": (BISECT | P_LIST | STAGED, FAST_ANY | P_MASS | CUT_IDX)}
    case("plateau_E_list", "plateau", lambda: plateau_max(561, V0, 300, "spread"), V0, (1.0, 65, 0.5), want=e)
    e = {"plain": (BISECT | P_MASS | CUT_IDX | STAGED, FAST_ANY | P_LIST)}
    case("plateau_E_k2000_cut", "plateau", lambda: plateau_max(562, V0, 1500, "spread"), V0, (1.0, 2000, 0.99), want=e)
    e = {"plain": (P_MASS | CUT_IDX, FAST_ANY | P_LIST | STAGED | BISECT)}
    for dt in (0, 1, 2):
        case(f"plateau_E_mass_cut_D_dt{dt}", "plateau", lambda: plateau_max(563, 50272, 1500, "spread"), 50272, (0.7, 0, 0.9), dt=dt, want=e)

    # ---- family 3: masked rows
    fl = _fast(V0)
    # V - 20 entries are -inf: every chunk but a few holds only -inf, its threshold is -inf and it keeps its whole chunk
    # (per-chunk cap); most tile maxima are -inf and fewer than 20 per wave are finite, so > 1024 tiles qualify (tile cap);
    # the in-kernel prefilter's threshold is -inf as well (cap), and the general path then finds 20 finite survivors
    tail = (PRE | PRE_CAP | BISECT | P_LIST, P_MASS)
    w = {"plain": (tail[0] | STAGED, tail[1]), "ws": (A | A_CHUNK | tail[0] | STAGED, A_TOTAL | tail[1]),
         "tile": (B | B_TILE | tail[0], B_CAND | STAGED | tail[1])}
    for dt in (0, 1, 2):
        case(f"masked_filtered_dt{dt}", "masked", lambda: masked(301, V0, "filtered"), V0, HARNESS, dt=dt, want=w)
        case(f"masked_few_dt{dt}", "masked", lambda: masked(302, V0, "few"), V0, HARNESS, dt=dt, want=w)
        case(f"masked_tail_dt{dt}", "masked", lambda: masked(303, V0, "tail"), V0, HARNESS, dt=dt,
             want={"plain": fl["plain"], "ws": (A | A_CHUNK | fl["plain"][0], A_TOTAL | BISECT | P_MASS), "tile": fl["tile"]})
    for V in (V0, 50272):
        for dt in (0, 1):
            case(f"masked_half_V{V}_dt{dt}", "masked", lambda V=V: masked(306, V, "half"), V, HARNESS, dt=dt, want=_fast(V))
    e = {"plain": (P_LIST | STAGED, FAST_ANY | BISECT | P_MASS)}
    case("masked_filtered_E_p999", "masked", lambda: masked(301, V0, "filtered"), V0, (1.0, 0, 0.999), want=e)
    case("masked_few_E_k65", "masked", lambda: masked(302, V0, "few"), V0, (1.0, 65, 0.0),
         want={"plain": (BISECT | STAGED, FAST_ANY | P_LIST | P_MASS)})
    case("masked_tail_D", "masked", lambda: masked(304, 50272, "tail"), 50272, HARNESS,
         want={"plain": _fast(50272)["plain"], "tile": _fast(50272)["tile"]})
    case("masked_tail_E_mass", "masked", lambda: masked(305, 50272, "tail"), 50272, (0.7, 0, 0.9),
         want={"plain": (P_MASS, FAST_ANY | BISECT | P_LIST | STAGED)})

    # ---- family 4: wide dynamic range, extreme and negative temperature (route B must decline T < 0)
    case("wide_range_k20", "wide", lambda: wide_range(401, V0), V0, (1.0, 20, 0.0), want=_nop(_fast(V0)))
    case("T0.01", "wide", lambda: gauss(402, V0), V0, (0.01, 20, 0.9), want=_fast(V0))
    case("T100", "wide", lambda: gauss(403, V0), V0, (100.0, 20, 0.9), want=_fast(V0))
    w = _fast(V0)
    w["tile"] = w["plain"]
    case("T_negative", "wide", lambda: gauss(404, V0), V0, (-1.0, 20, 0.9), want=w)

    # ---- family 5: error rows at size
    for what in ("nan", "inf"):
        for where in ("chunk0", "chunk15", "last", "far_tile"):
            w = {"plain": (ERROR | STAGED, LIST | BISECT), "ws": (A | ERROR, LIST | BISECT), "tile": (B | ERROR, LIST | BISECT | STAGED)}
            case(f"error_{what}_{where}", "error", lambda what=what, where=where: error_row(600, V0, what, where), V0, HARNESS,
                 want=w, error=True)
    w = {"plain": (ERROR | STAGED, LIST), "ws": (A | A_CHUNK | ERROR | STAGED, LIST), "tile": (B | ERROR, LIST | STAGED)}
    case("error_allneg", "error", lambda: error_row(601, V0, "allneg", None), V0, HARNESS, want=w, error=True)
    case("error_nan_E", "error", lambda: error_row(602, 50257, "nan", "last"), 50257, (0.7, 0, 0.9),
         want={"plain": (ERROR, LIST | STAGED | FAST_ANY)}, error=True)

    # ---- 16-bit dtype modes on Gaussian rows (natural ties): every fast entry, C and D, E
    for dt in (1, 2):
        for V in (8192, 32000, 50272):
            for s in (800, 801, 802):
                case(f"lowprec_dt{dt}_V{V}_s{s}", "lowprec", lambda s=s, V=V: gauss(s, V), V, HARNESS, dt=dt, want=_fast(V))
        st = {"plain": (P_MASS | STAGED, FAST_ANY | BISECT | P_LIST)}
        case(f"lowprec_dt{dt}_E_mass", "lowprec", lambda: gauss(803, V0), V0, (0.7, 0, 0.9), dt=dt, want=st)
        case(f"lowprec_dt{dt}_k64_p05", "lowprec", lambda: gauss(804, V0), V0, (1.0, 64, 0.5), dt=dt, want=_fast(V0, k=64))


_build()
assert len({c["id"] for c in CASES}) == len(CASES)
FILTER_ONLY_IDS = ["bf16_valued_V32000_s100_x3", "gauss_V50272_s103_x3", "plateau_max_n129_spread_dt0", "plateau_max_n1500_spread_dt0",
                   "plateau_max_n1025_spread_dt1", "masked_filtered_dt0", "masked_few_dt2", "bf16_valued_E_mass_V32000",
                   "gauss_E_k2000", "plateau_E_mass_cut_D_dt0", "wide_range_k20", "lowprec_dt1_V32000_s800"]
SAMPLE_IDS = ["bf16_valued_V32000_s100_x3", "bf16_valued_V50272_s100_x3", "gauss_V32000_s103_x3", "gauss_V128256",
              "plateau_max_n64_spread_dt0", "plateau_max_n193_chunk_dt0", "plateau_max_n1500_spread_dt0", "plateau_max_n1025_spread_dt1",
              "masked_filtered_dt0", "masked_few_dt1", "bf16_valued_E_mass_V50257", "gauss_E_k2000", "lowprec_dt2_V32000_s801",
              "plateau_kth_n129_spread_dt0", "wide_range_k20"]
BY_ID = {c["id"]: c for c in CASES}
assert all(i in BY_ID for i in FILTER_ONLY_IDS + SAMPLE_IDS)

# (route, family) pairs the table must contain: label -> predicate on the (set, clear) expectation of some entry
REQUIRED_ROUTES = {
    "A": lambda s, c: s & A and not s & (A_CHUNK | A_TOTAL | A_SECOND | ERROR),
    "A+second": lambda s, c: s & A_SECOND,
    "A->chunk cap": lambda s, c: s & A_CHUNK,
    "A->total cap": lambda s, c: s & A_TOTAL,
    "B": lambda s, c: s & B and not s & (B_TILE | B_CAND | ERROR),
    "B->tile cap": lambda s, c: s & B_TILE,
    "B->cand cap": lambda s, c: s & B_CAND,
    "C": lambda s, c: s & PRE and s & STAGED and not s & (A | B | PRE_CAP),
    "C->E": lambda s, c: s & PRE_CAP and s & STAGED and not s & (A | B),
    "D": lambda s, c: s & PRE and c & STAGED and not s & (A | B | PRE_CAP),
    "D->E": lambda s, c: s & PRE_CAP and c & STAGED and not s & (A | B),
    "E list top-p": lambda s, c: s & P_LIST and c & PRE and c & A,
    "E mass": lambda s, c: s & P_MASS and c & CUT_IDX,
    "E mass+cut_idx": lambda s, c: s & P_MASS and s & CUT_IDX,
}
# families that must reach each of them (the issue's table: 1, 2, 3 and 6 wherever the family can take the route - a
# give-up needs a plateau or a mask by construction)
REQUIRED_PAIRS = [(r, f) for r in ("A+second", "B", "C", "D", "E list top-p") for f in ("bf16_valued", "gauss", "plateau", "masked")] + \
                 [("A", "bf16_valued"), ("A", "gauss")] + \
                 [(r, "plateau") for r in REQUIRED_ROUTES if r not in ("E mass", "A")] + \
                 [("A->chunk cap", "masked"), ("B->tile cap", "masked"), ("C->E", "masked"), ("E mass", "gauss")]
