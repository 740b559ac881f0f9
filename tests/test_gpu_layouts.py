"""The fixed-point flooding decoder at every check count where a kernel's lane layout changes, GPU vs
the CPU oracle, bit-exact (iterations, hard decisions, syndrome verdicts, posteriors).

The number of checks m decides which kernel choose_kernel (fpldpc_kernels.hip) picks and how that
kernel lays checks onto lanes.  Part A runs every p = 47 array code r = 1..47 on its default kernel,
part B the family's other kernels forced with FPLDPC_KERNEL at the ends of their envelopes, part C the
table and generic kernels at their own check-count edges on random codes with exact check degrees.

No case skips: a creation error fails the test.  Each case's describe() must start with the name the
rule tables below predict; the tables restate choose_kernel's conditions and are not run output:

  LDS bytes of a variant (variant_lds): (4 n + 20) * 4 posteriors and control words, + 2 * ceil(n / 32) * 4
  info masks, + m * tab_words * 4 (ldsoffs / mix: 25 words per check), + m * dc * 2 (flood_lds16's state);
  p = 47: 35,424 + 560 = 35,984 before the per-check terms.  A variant is taken only if it and every
  kernel of its fallback chain stay within 160 KiB = 163,840.
    flood_array2<P=47,W=3>            m <= 256                      r <= 5     chain flood_array<P=47>
    flood_array2<P=47,..,mix>         m <= 1152                     r <= 24    chain flood_lds16, flood_gmem<48>
    flood_array2<P=47,CPL=2,ldsoffs>  m <= 1536, 35,984 + 100 m     r <= 27    (m <= 1278), the same chain
    flood_array2<P=47,CPL=2>          m <= 1536, chain's flood_lds16 35,984 + 94 m, so m <= 1360: r = 28 only
    flood_lds16<P=47>                 m <= 2048, 35,984 + 94 m      r <= 28    chain flood_gmem<48>
    r = 29..32 (m = 1363..1504) fit the walked CPL=2 kernel but not its chain: flood_gmem<DC=48>, as r >= 33.
  Codes that are no p = 47 array code, by check degrees: the degree-sorted table kernel needs degrees 7..8 and
  at least 3 * 256 checks of degree 7, the table kernel degrees 7..8, both m <= 1024; flood_reg<DC,CPL> takes
  dc_max <= DC and m <= 256 CPL in the order <8,1>, <8,4>, <16,2>; all else the first flood_gmem<DC> with
  dc_max <= DC.  The int32 kernels need (4 n + 20) * 4 bytes of LDS, dynamic, and no other: n <= 10,235.

Kernels with a fallback chain (the int16 ones) must hand at least the full-range frames of the batch down
the chain (they are out of range from their load); kernels without one report (0, 0).
"""
import math
from collections import deque

import numpy as np
import pytest

from conftest import assert_same

pytestmark = pytest.mark.gpu

SEED = 123456789
MAX_ITER = 10

MIX = "flood_array2<P=47,CPL=2,ldsoffs,mix>"
LDSOFFS = "flood_array2<P=47,CPL=2,ldsoffs>"
CPL2 = "flood_array2<P=47,CPL=2>"
LDS16 = "flood_lds16<P=47>"
TAB_LO = "flood_tab2<DC=8,CPL=4,lo=3>"
TAB = "flood_tab2<DC=8,CPL=4>"
CHAINED = {"flood_array2<P=47,W=3>", MIX, LDSOFFS, CPL2, LDS16, TAB_LO, TAB}


def p47_default(r):
    """The rule table of the module docstring for the default kernel of Code.array(47, r)."""
    m, lds0 = 47 * r, (4 * 2209 + 20) * 4 + 2 * 70 * 4
    lds16_fits = lds0 + 94 * m <= 160 * 1024
    if m <= 256:
        return "flood_array2<P=47,W=3>"
    if m <= 1152 and lds0 + 100 * m <= 160 * 1024 and lds16_fits:
        return MIX
    if m <= 1536 and lds0 + 100 * m <= 160 * 1024 and lds16_fits:
        return LDSOFFS
    if m <= 1536 and lds16_fits:
        return CPL2
    return "flood_gmem<DC=48>"


def test_rule_table_spelled_out():
    """The derived table, spelled out: r <= 5 A, 6..24 mix, 25..27 ldsoffs, 28 CPL=2, 29.. global."""
    got = [p47_default(r) for r in range(1, 48)]
    assert got == (["flood_array2<P=47,W=3>"] * 5 + [MIX] * 19 + [LDSOFFS] * 3 + [CPL2] + ["flood_gmem<DC=48>"] * 19)


def p47_centre(r):
    """Centre (dB, channel SNR) of the three AWGN points c - 1, c, c + 1 of Code.array(47, r)."""
    for top, c in ((1, 8.5), (2, 8.0), (3, 7.5), (5, 7.0), (10, 6.5), (19, 6.0), (47, 5.5)):
        if r <= top:
            return c


def exact_alist(n, degs, seed):
    """alist text of a random H whose check c has degree degs[c] exactly: rows cut from concatenated random
    permutations of range(n) (a permutation that starts inside a row lists that row's variables last), so every
    variable is covered (sum(degs) >= n), no row repeats a variable, and variable degrees differ by at most 1."""
    degs = [int(d) for d in degs]
    assert sum(degs) >= n >= max(degs)
    rs = np.random.default_rng(seed)
    pool, rows = deque(), []
    for d in degs:
        row = []
        while len(row) < d:
            if not pool:
                perm = [int(x) for x in rs.permutation(n)]
                pool = deque([x for x in perm if x not in row] + [x for x in perm if x in row])
            row.append(pool.popleft())
        assert len(set(row)) == d
        rows.append(sorted(row))
    vl = [[] for _ in range(n)]
    for c, row in enumerate(rows):
        for v in row:
            vl[v].append(c)
    assert all(vl)
    out = [f"{n} {len(rows)}", f"{max(map(len, vl))} {max(degs)}", " ".join(str(len(x)) for x in vl),
           " ".join(map(str, degs))]
    out += [" ".join(map(str, x)) for x in vl] + [" ".join(map(str, x)) for x in rows]
    return "\n".join(out) + "\n"


def _mixed(m, lo, hi, seed):
    """m degrees covering lo..hi: every value at least once where m allows, in a random order."""
    rs = np.random.default_rng(seed)
    d = np.concatenate([np.arange(lo, hi + 1), rs.integers(lo, hi + 1, max(0, m - (hi - lo + 1)))])[:m]
    d[:2] = (hi, lo) if m >= 2 else d[:2]
    return [int(x) for x in rs.permutation(d)]


def _shuffled(degs, seed):
    return [int(x) for x in np.random.default_rng(seed).permutation(degs)]


# Part C: centre (dB) of each shape's AWGN points, found on the CPU with the oracle alone (the recipe of
# frames() below on a 0.5 dB grid, as for p = 47: the middle of the centres at which the condition holds)
CENTRES = {
    "lo3_m768": 1.5, "lo3_m769": 2.5, "lo3_m896": 2.5, "lo3_m1024_mixed": 3.0, "lo3_m1024_deg7": 2.0, "lo3_m1024_dv1": 8.0,
    "tab_m2": 4.5, "tab_m255": 3.0, "tab_m256": 3.0, "tab_m257": 3.0, "tab_m512": 3.0, "tab_m513": 3.5, "tab_m767": 3.5,
    "tab_m1024_n8192": 9.0, "reg8x1_m255": 4.0, "reg8x1_m256": 4.0, "reg8x4_m1023": 3.0, "reg8x4_m1024": 3.5,
    "reg16x2_m511": 4.5, "reg16x2_m512": 4.5, "gmem16_m513": 5.0, "gmem8_n10235": 4.0, "gmem32_m65": 5.5,
    "gmem32_m1025": 6.0, "gmem64_m65": 7.0, "gmem64_m1025": 7.0,
}
# name -> (n, check degrees, expected kernel, forced name or None)
SHAPES = {
    # the degree-sorted table kernel: at least 768 checks of degree 7
    "lo3_m768": (1201, [7] * 768, TAB_LO, None),
    "lo3_m769": (1536, _shuffled([7] * 768 + [8], 1), TAB_LO, None),
    "lo3_m896": (2000, [7] * 768 + _mixed(128, 7, 8, 2), TAB_LO, None),
    "lo3_m1024_mixed": (2400, _shuffled([7] * 768 + [8] * 256, 3), TAB_LO, None),
    "lo3_m1024_deg7": (1793, [7] * 1024, TAB_LO, None),
    "lo3_m1024_dv1": (7168, [7] * 1024, TAB_LO, None),
    # the table kernel: fewer than 768 of degree 7
    "tab_m2": (9, [7, 8], TAB, None),
    "tab_m255": (601, _mixed(255, 7, 8, 4), TAB, None),
    "tab_m256": (640, _mixed(256, 7, 8, 5), TAB, None),
    "tab_m257": (643, _mixed(257, 7, 8, 6), TAB, None),
    "tab_m512": (1280, _mixed(512, 7, 8, 7), TAB, None),
    "tab_m513": (1283, _mixed(513, 7, 8, 8), TAB, None),
    "tab_m767": (1917, _mixed(767, 7, 8, 9), TAB, None),
    "tab_m1024_n8192": (8192, [8] * 1024, TAB, None),
    # the generic int32 kernels at their own max_m
    "reg8x1_m255": (600, _mixed(255, 2, 8, 10), "flood_reg<DC=8,CPL=1>", "flood_reg<DC=8,CPL=1>"),
    "reg8x1_m256": (601, _mixed(256, 2, 8, 11), "flood_reg<DC=8,CPL=1>", "flood_reg<DC=8,CPL=1>"),
    "reg8x4_m1023": (2047, _mixed(1023, 2, 8, 12), "flood_reg<DC=8,CPL=4>", None),
    "reg8x4_m1024": (2048, _mixed(1024, 2, 8, 13), "flood_reg<DC=8,CPL=4>", None),
    "reg16x2_m511": (1533, _mixed(511, 2, 16, 14), "flood_reg<DC=16,CPL=2>", None),
    "reg16x2_m512": (1536, _mixed(512, 2, 16, 15), "flood_reg<DC=16,CPL=2>", None),
    "gmem16_m513": (1539, _mixed(513, 2, 16, 16), "flood_gmem<DC=16>", None),
    # the longest code any kernel takes: (4 n + 20) * 4 <= 160 KiB
    "gmem8_n10235": (10235, _mixed(5000, 2, 8, 17), "flood_gmem<DC=8>", None),
    "gmem32_m65": (401, _mixed(65, 2, 32, 18), "flood_gmem<DC=32>", None),
    "gmem32_m1025": (6001, _mixed(1025, 2, 32, 19), "flood_gmem<DC=32>", None),
    "gmem64_m65": (701, _mixed(65, 2, 64, 20), "flood_gmem<DC=64>", None),
    "gmem64_m1025": (10001, _mixed(1025, 2, 64, 21), "flood_gmem<DC=64>", None),
}


class Case:
    """A code, its oracle twin and the one frame recipe; the oracle's results per (mask, precheck), computed
    once per session and kept read-only."""

    def __init__(self, F, O, code, centre):
        self.code, self.O = code, O
        self.ocode = O.OracleCode.from_alist_text(code.write_alist())
        self.llr, self.kind = frames(O, code.n, centre)
        self.llr.setflags(write=False)
        self._ref = {}

    def ref(self, mask=0xFF, precheck=False):
        key = (mask, precheck)
        if key not in self._ref:
            r = self.O.decode_batch(self.ocode, self.llr, max_iter=MAX_ITER, mask=mask, precheck=precheck)
            for v in r.values():
                v.setflags(write=False)
            self._ref[key] = r
        return self._ref[key]


def frames(O, n, centre):
    """48 frames: 3 x 12 AWGN at centre - 1, centre, centre + 1 dB (first frames 0 / 1000 / 2000 of the channel
    stream), 4 uniform in +-2000, 2 uniform in +-3 (zeros occur), 2 noiseless (all 40), 2 uniform over the whole
    int16 range, 2 with |LLR| in 5000..8000 and random signs; in a fixed random order, so that frames of every
    kind share workgroups.  Returns the LLRs and each frame's kind."""
    rs = np.random.default_rng(n)
    parts, kind = [], []
    for i, x in enumerate((centre - 1, centre, centre + 1)):
        snr = math.pow(10.0, x / 10)
        parts.append(O.gen_llr(SEED, 1000 * i, 12, n, snr, math.sqrt(1 / snr), 4))
        kind += ["awgn"] * 12
    parts += [rs.integers(-2000, 2001, (4, n)), rs.integers(-3, 4, (2, n)), np.full((2, n), 40),
              rs.integers(-32768, 32768, (2, n)), rs.integers(5000, 8001, (2, n)) * rs.choice([-1, 1], (2, n))]
    kind += ["mid"] * 4 + ["small"] * 2 + ["clean"] * 2 + ["full"] * 2 + ["large"] * 2
    order = rs.permutation(len(kind))
    return np.concatenate(parts).astype(np.int32)[order], np.array(kind)[order]


_CASES = {}


def p47_case(F, O, r):
    if ("p47", r) not in _CASES:
        _CASES["p47", r] = Case(F, O, F.Code.array(47, r), p47_centre(r))
    return _CASES["p47", r]


def shape_case(F, O, name):
    if name not in _CASES:
        n, degs = SHAPES[name][:2]
        _CASES[name] = Case(F, O, F.Code.parse(exact_alist(n, degs, len(degs))), CENTRES[name])
    return _CASES[name]


def assert_awgn_not_trivial(case):
    """On the oracle's own result (mask 0xFF): the AWGN frames' iteration counts take at least three values,
    the cap and one <= 5 among them; with dv_max = 1 nothing changes after the first update, so the counts
    are 1 or the cap, and both occur."""
    it = case.ref()["iters"][case.kind == "awgn"]
    vals = set(int(x) for x in it)
    if case.code.dv_max == 1:
        assert vals == {1, MAX_ITER}, sorted(vals)
    else:
        assert len(vals) >= 3 and MAX_ITER in vals and min(vals) <= 5, sorted(vals)


def run(F, case, torch_dev, expect, mask=0xFF, precheck=False, tile=1, where=""):
    """Create the decoder (an error fails the test), check the kernel's name, decode the recipe (tiled `tile`
    times) and compare everything with the oracle; then the fallback counts."""
    import torch
    assert_awgn_not_trivial(case)
    dec = F.Decoder(case.code, max_iter=MAX_ITER, width_mask=mask, precheck=precheck)
    assert dec.describe().split(" ")[0] == expect, (where, dec.describe(), expect)
    ref, llr, kind = case.ref(mask, precheck), case.llr, case.kind
    if tile > 1:
        llr, kind = np.tile(llr, (tile, 1))[:600], np.tile(kind, tile)[:600]
        ref = {k: np.concatenate([v] * tile)[:600] for k, v in ref.items()}
    out = dec.decode_torch(torch.from_numpy(llr.astype(np.int16)).to(torch_dev), post=True)
    torch.cuda.synchronize()
    fb = dec.fallback_counts()
    gpu = {k: v.cpu().numpy() for k, v in out.items()}
    where = f"{where} mask {mask:#x} precheck {precheck} B={len(llr)} [{dec.describe()}] fallbacks={fb}"
    assert_same(gpu, ref, case.code.n, check_post=False, where=where)
    ran = ref["iters"] > 0  # (a frame the pre-check passes keeps its zero-initialised posteriors)
    assert (ref["iters"][kind == "clean"] == 0).all() if precheck else ran.all()
    bad = np.nonzero((gpu["post"][ran] != ref["post"][ran]).any(axis=1))[0]
    assert bad.size == 0 and (gpu["post"][~ran] == 0).all(), f"{where}: posterior mismatch at {np.nonzero(ran)[0][bad[:8]]}"
    if expect in CHAINED:
        assert fb[0] >= int((kind == "full").sum()), where
    else:
        assert fb == (0, 0), where
    return dec


# ---- A: the p = 47 family on its default kernel ----

BOUNDARIES = [1, 5, 6, 16, 17, 21, 22, 24, 25, 27, 28, 29, 32, 33, 47]


@pytest.mark.parametrize("r", range(1, 48))
def test_p47_default_kernel(F, O, torch_dev, r):
    run(F, p47_case(F, O, r), torch_dev, p47_default(r), where=f"p47 r{r}")


@pytest.mark.parametrize("r", BOUNDARIES)
def test_p47_boundary_mask_and_precheck(F, O, torch_dev, r):
    case = p47_case(F, O, r)
    run(F, case, torch_dev, p47_default(r), mask=0x3F, where=f"p47 r{r}")
    run(F, case, torch_dev, p47_default(r), mask=0x3F, precheck=True, where=f"p47 r{r}")
    run(F, case, torch_dev, p47_default(r), precheck=True, where=f"p47 r{r}")


@pytest.mark.parametrize("r", BOUNDARIES)
def test_p47_boundary_refills(F, O, torch_dev, monkeypatch, r):
    """600 frames (the recipe tiled) on one workgroup per CU: workgroups refill a frame half while the
    neighbouring lanes are idle or still decoding."""
    monkeypatch.setenv("FPLDPC_GRID_PER_CU", "1")
    run(F, p47_case(F, O, r), torch_dev, p47_default(r), tile=13, where=f"p47 r{r} refills")


# ---- B: the family's other kernels, forced, at the ends of their envelopes ----

FORCED = [(LDSOFFS, 6), (LDSOFFS, 16), (LDSOFFS, 17), (LDSOFFS, 27),
          (CPL2, 6), (CPL2, 17), (CPL2, 28),
          (LDS16, 1), (LDS16, 21), (LDS16, 22), (LDS16, 28),
          ("flood_array<P=47>", 1), ("flood_array<P=47>", 3),
          ("flood_reg<DC=47,CPL=1,regular>", 1), ("flood_reg<DC=47,CPL=1,regular>", 4),
          ("flood_gmem<DC=48>", 1), ("flood_gmem<DC=48>", 33), ("flood_gmem<DC=48>", 47),
          ("flood_gmem<DC=64>", 1), ("flood_gmem<DC=64>", 33), ("flood_gmem<DC=64>", 47)]


@pytest.mark.parametrize("name,r", FORCED)
def test_p47_forced_kernel(F, O, torch_dev, monkeypatch, name, r):
    monkeypatch.setenv("FPLDPC_KERNEL", name)
    run(F, p47_case(F, O, r), torch_dev, name, where=f"p47 r{r} forced")


# ldsoffs: 35,984 + 100 * 1316 > 163,840; flood_array: 282 checks > 256; flood_lds16: 35,984 + 94 * 1363 >
# 163,840; the walked CPL=2 kernel fits r = 29..32 itself, its chain's flood_lds16 does not
REFUSED = [(LDSOFFS, 28), ("flood_array<P=47>", 6), (LDS16, 29), (CPL2, 29), (CPL2, 32), (CPL2, 33)]


@pytest.mark.parametrize("name,r", REFUSED)
def test_p47_forced_kernel_refused(F, monkeypatch, name, r):
    monkeypatch.setenv("FPLDPC_KERNEL", name)
    with pytest.raises(F.FpldpcError) as e:
        F.Decoder(F.Code.array(47, r), max_iter=MAX_ITER)
    assert e.value.code == -4, e.value


# ---- C: table and generic kernels at their check-count edges ----

@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shape(F, O, torch_dev, monkeypatch, name):
    n, degs, expect, force = SHAPES[name]
    if force:
        monkeypatch.setenv("FPLDPC_KERNEL", force)
    case = shape_case(F, O, name)
    assert (case.code.n, case.code.m, case.code.dc_max) == (n, len(degs), max(degs))
    run(F, case, torch_dev, expect, where=name)
    run(F, case, torch_dev, expect, mask=0x3F, precheck=True, where=name)


@pytest.mark.parametrize("split", ["0", "1"])
@pytest.mark.parametrize("name", sorted(k for k, v in SHAPES.items() if v[2] == TAB))
def test_table_kernel_lone_frames(F, O, torch_dev, monkeypatch, name, split):
    """Batches of 1 and 3 frames (lone frames from the first step) with FPLDPC_SPLIT_TAIL 0 and 1."""
    import torch
    monkeypatch.setenv("FPLDPC_SPLIT_TAIL", split)
    case = shape_case(F, O, name)
    dec = F.Decoder(case.code, max_iter=MAX_ITER)
    assert dec.describe().split(" ")[0] == TAB, dec.describe()
    ref = case.ref()
    for first in (0, 7, 20):
        for B in (1, 3):
            sl = slice(first, first + B)
            out = dec.decode_torch(torch.from_numpy(case.llr[sl].astype(np.int16)).to(torch_dev), post=True)
            gpu = {k: v.cpu().numpy() for k, v in out.items()}
            assert_same(gpu, {k: v[sl] for k, v in ref.items()}, case.code.n, where=f"{name} split={split} frames {sl}")


def test_reg8x1_refuses_257_checks(F, monkeypatch):
    monkeypatch.setenv("FPLDPC_KERNEL", "flood_reg<DC=8,CPL=1>")
    with pytest.raises(F.FpldpcError) as e:
        F.Decoder(F.Code.parse(exact_alist(603, _mixed(257, 2, 8, 22), 257)), max_iter=MAX_ITER)
    assert e.value.code == -4, e.value


def test_longer_code_is_refused(F):
    """One past the longest code the kernels take (the gmem8_n10235 case: (4 n + 20) * 4 = 160 KiB exactly):
    unsupported, and said so."""
    code = F.Code.parse(exact_alist(10236, _mixed(5000, 2, 8, 17), 5000))
    with pytest.raises(F.FpldpcError, match="code length too large") as e:
        F.Decoder(code, max_iter=MAX_ITER)
    assert e.value.code == -4, e.value
