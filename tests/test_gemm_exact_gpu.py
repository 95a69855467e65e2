"""Every GEMM tile configuration, schedule and epilogue against the float64 reference of tests/gemm_reference.py with EXACT operands: small
integers whose products add exactly in fp32 in any order, so a correct kernel matches bit for bit whatever its tile, split or reduction
order (`assert_exact`), memory outside the operand views changes no bit (`embed` + guards), and only what a transcendental or the fold's
rsqrt touches is compared within derived bf16 ulps (`assert_ulps`, bounds in gemm_reference.ULPS).

Shapes come from the tile under test (edge bugs show at the smallest ragged sizes), every test loops over its shapes and reports all
failures at once.  tests/test_gemm_reference.py shows on the CPU that these checks reject what the tolerance tests accept.
"""
import json
from collections import namedtuple
from pathlib import Path

import pytest
import torch

from tests import gemm_reference as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
ANY = None

# The tile configurations of csrc/gemm_nt.hip (kTiles), literally: id, tile rows x columns, K tile (64: the 8-wave and 4-wave kernels, 32: the
# ring and the skinny kernel), K granularity, accepted K-extension widths (ANY: every multiple of 8), whether id + 100 (the hybrid schedule
# forced) exists, kernel family.  6 is the skinny kernel: no forced id, `tile = 0` takes it for N = 32, K <= 3072, M >= 512.
# test_table_names_every_configuration_of_the_dispatch_table ties the ids to tests/golden/gemm_dispatch_table.json.
Cfg = namedtuple("Cfg", "id BM BN BK kgran kext plus100 fam")
CONFIGS = [
    Cfg(1, 128, 128, 64, 8, ANY, True, "w8"), Cfg(2, 64, 128, 64, 8, ANY, True, "w8"),
    Cfg(5, 128, 32, 64, 8, ANY, True, "w8"),
    Cfg(10, 256, 256, 32, 8, ANY, False, "ring"), Cfg(11, 256, 128, 32, 8, ANY, False, "ring"), Cfg(12, 256, 128, 32, 8, ANY, False, "ring"),
    Cfg(13, 128, 256, 32, 8, ANY, False, "ring"), Cfg(14, 128, 128, 32, 8, ANY, False, "ring"), Cfg(15, 256, 256, 32, 8, ANY, False, "ring"),
    Cfg(20, 256, 256, 32, 8, ANY, False, "ring"), Cfg(21, 256, 256, 32, 8, ANY, False, "ring"),
    Cfg(16, 256, 256, 64, 8, ANY, True, "w8"), Cfg(17, 256, 256, 64, 8, ANY, True, "w8"),
    Cfg(18, 256, 256, 64, 64, (0, 32, 64, 96), True, "w4"), Cfg(22, 128, 256, 64, 64, (0, 32), True, "w4"),
    Cfg(6, 32, 32, 32, 8, (0,), False, "skinny"),
]
REMOVED_TILES = [3]                                                       # the 256x128 8-wave tile: no longer in kTiles
BY_ID = {c.id: c for c in CONFIGS}
FORCED = [c.id for c in CONFIGS if c.fam != "skinny"]                     # ids `tile=` accepts
PLUS100 = [c.id + 100 for c in CONFIGS if c.plus100]
EVERY_TILE = FORCED + PLUS100 + [0]                                       # 0 here = the skinny kernel through the auto path
FIXED_TILES = [1, 2, 5, 17, 18, 22]
FIXED_SPLITS = [1, 2, 3, 5, 8]
PLAIN_K = {"w8": (8, 56, 64, 72, 136, 520), "ring": (8, 24, 32, 40, 104, 520), "w4": (64, 128, 192, 448), "skinny": (8, 24, 32, 40, 104, 520)}


def cfg_of(tile):
    return BY_ID[6] if tile == 0 else BY_ID[tile % 100]


def tname(tile):
    return "skinny" if tile == 0 else f"t{tile}"


def shapes_mn(c):
    if c.fam == "skinny":      # N = 32 and M >= 512 are what makes `tile = 0` take it; 32 rows per workgroup
        return [512, 512 + c.BM - 1, 512 + c.BM + 1, 512 + 2 * c.BM + 37], [32]
    return [1, c.BM - 1, c.BM + 1, 2 * c.BM + 37], [8, c.BN - 8, c.BN + 8, 2 * c.BN + 24]


def ragged_mn(c):
    return (512 + c.BM + 5, 32) if c.fam == "skinny" else (c.BM + 37, c.BN + 24)


Failures = R.Failures


def resolved_family(ops, fn):
    """The kernel instance a launch ran, as the library's own decision code names it (ovla_gemm_resolved_tile through ops._gemm_family)."""
    prev, ops.PROFILE = ops.PROFILE, []
    try:
        out = fn()
        fams = [f for f, *_ in ops.PROFILE]
    finally:
        ops.PROFILE = prev
    return out, fams


def run_plain(ops, dev, tile, a, b, **kw):
    """One launch; for the skinny kernel the launch must have resolved to it."""
    if tile != 0:
        return ops.gemm(a, b, tile=tile, **kw)
    out, fams = resolved_family(ops, lambda: ops.gemm(a, b, tile=0, **kw))
    assert fams == ["gemm_nt_t6"], f"expected the skinny kernel, the launch resolved to {fams}"
    return out


# ---- the table -------------------------------------------------------------------------------------------------------------------------------
def test_table_names_every_configuration_of_the_dispatch_table():
    """The literal table covers the ids the recorded dispatch table knows (tests/golden/gemm_dispatch_table.json): a tile added to kTiles is
    re-recorded there and then fails here until it is added to CONFIGS -- and with that to every test below."""
    tiles = json.loads((Path(__file__).resolve().parent / "golden" / "gemm_dispatch_table.json").read_text())["tiles"]
    not_a_config = {0, 7, 103, 110, 1018} | set(REMOVED_TILES)   # auto, and the ids the recorded table keeps to pin the "unknown tile" errors
    assert set(tiles) - not_a_config == {c.id for c in CONFIGS} | set(PLUS100)
    assert len({c.id for c in CONFIGS}) == len(CONFIGS) and set(FIXED_TILES) <= set(FORCED)
    assert not set(REMOVED_TILES) & ({c.id for c in CONFIGS} | set(PLUS100))


@pytest.mark.parametrize("tile", REMOVED_TILES, ids=tname)
def test_removed_tile_ids_are_unknown(ops, dev, tile):
    """The id of a removed configuration (3: the 256x128 8-wave tile) is no configuration any more: a launch that names it is refused with the
    unknown-id message before anything runs, and the output keeps its bits."""
    g = R.rng(500 + tile)
    a, b = R.operand(g, 64, 64).to(dev), R.operand(g, 64, 64).to(dev)
    out = torch.full((64, 64), 7.0, dtype=BF, device=dev)
    with pytest.raises(RuntimeError, match=rf"unknown tile id {tile}\b"):
        ops.gemm(a, b, out=out, tile=tile)
    assert torch.equal(out, torch.full_like(out, 7.0)), f"tile {tile}: the refused launch wrote the output"


# ---- plain GEMM, every configuration -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", EVERY_TILE, ids=tname)
def test_plain_every_configuration(ops, dev, tile):
    """M on both sides of one and two row tiles, N likewise, K below the pipeline depth, exactly one K tile, ragged tails, odd and even tile
    counts.  Operands are views of one larger matrix, so columns past K hold live data a K tail must not read."""
    c, fails = cfg_of(tile), Failures()
    Ms, Ns = shapes_mn(c)
    Ks = PLAIN_K[c.fam]
    g = R.rng(1000 + tile)
    A, B = R.operand(g, max(Ms), max(Ks) + 8), R.operand(g, max(Ns), max(Ks) + 8)
    Ad, Bd = A.to(dev), B.to(dev)
    for K in Ks:
        ref = R.reference(A[:, :K], B[:, :K]).out.to(dev)
        for M in Ms:
            for N in Ns:
                out = run_plain(ops, dev, tile, Ad[:M, :K], Bd[:N, :K])
                fails.exact(out, ref[:M, :N], f"{tname(tile)} plain {M}x{N}x{K}", (c.BM, c.BN))
    fails.done()


# ---- isolation ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", EVERY_TILE, ids=tname)
def test_operand_and_output_isolation(ops, dev, tile):
    """Operands embedded in larger allocations whose guard rows and columns hold zeros, +-3e38, then NaN: the outputs are bit-identical across the
    three and exact, and no output guard element (rows above and below, columns left and right up to ldc) is written.  K has a ragged tail,
    M and N ragged edge tiles; the forward launch carries the K-extension, bias, the residual and C_pre, a second launch the backward epilogue."""
    c, fails = cfg_of(tile), Failures()
    M, N = ragged_mn(c)
    K = {"w8": 136, "ring": 104, "w4": 192, "skinny": 104}[c.fam]
    K2 = {"w8": 24, "ring": 24, "w4": 32, "skinny": 0}[c.fam]
    g = R.rng(2000 + tile)
    a, b, res, bias = R.operand(g, M, K), R.operand(g, N, K), R.bias_like(g, M, N), R.bias_like(g, N).to(dev)
    a2, b2 = (R.operand(g, M, K2), R.operand(g, N, K2)) if K2 else (None, None)
    z = (R.ints(g, (M, N), -24, 24).float() * 0.25).to(BF)
    fwd = R.reference(a, b, a2=a2, b2=b2, alpha=0.5, bias=bias.cpu(), residual=res) if K2 else R.reference(a, b, alpha=0.5)
    bwd = R.reference(a, b, dact=("act", z, R.ACT_RELU))
    first = {}
    for fill in R.GUARD_FILLS:
        e = {k: R.embed(v.to(dev), align=8, fill=fill) for k, v in dict(a=a, b=b, a2=a2, b2=b2).items() if v is not None}
        out = R.embed(BF, shape=(M, N), align=4, right=2, fill="sentinel", device=dev)
        if c.fam == "skinny":
            run_plain(ops, dev, 0, e["a"].view, e["b"].view, out=out.view, alpha=0.5)
        else:
            pre = R.embed(BF, shape=(M, N), align=4, right=2, fill="sentinel", device=dev)
            r_ = R.embed(res.to(dev), align=4, right=2, fill=fill)
            ops.gemm(e["a"].view, e["b"].view, a2=e["a2"].view, b2=e["b2"].view, alpha=0.5, bias=bias, residual=r_.view, c_pre=pre.view, out=out.view, tile=tile)
            fails.exact(pre.view, fwd.c_pre, f"{tname(tile)} C_pre, guards {fill}", (c.BM, c.BN))
            pre.assert_guards(f"{tname(tile)} C_pre, guards {fill}")
            z_ = R.embed(z.to(dev), align=4, right=2, fill=fill)
            out2 = R.embed(BF, shape=(M, N), align=4, right=2, fill="sentinel", device=dev)
            ops.gemm(e["a"].view, e["b"].view, dact=("act", z_.view, R.ACT_RELU), out=out2.view, tile=tile)
            fails.exact(out2.view, bwd.out, f"{tname(tile)} backward, guards {fill}", (c.BM, c.BN))
            out2.assert_guards(f"{tname(tile)} backward C, guards {fill}")
            fails.check(torch.equal(first.setdefault("bwd", out2.view.clone()), out2.view), f"{tname(tile)} backward: bits depend on the guards ({fill})")
        fails.exact(out.view, fwd.out, f"{tname(tile)} C, guards {fill}", (c.BM, c.BN))
        out.assert_guards(f"{tname(tile)} C, guards {fill}")
        fails.check(torch.equal(first.setdefault("fwd", out.view.clone()), out.view), f"{tname(tile)}: bits depend on the guards ({fill})")
    fails.done()


# ---- epilogues ---------------------------------------------------------------------------------------------------------------------------------
EPILOGUE_TILES = [1, 101, 2, 102, 5, 105, 16, 116, 17, 117, 18, 118, 22, 122, 10]     # every +100 configuration in both forms, one ring configuration
ACT_WORST = {}      # worst |err| / ulp per non-exact epilogue over the whole run (printed by the last test of the file)


def _note(key, worst):
    ACT_WORST[key] = max(ACT_WORST.get(key, 0.0), worst)


@pytest.mark.parametrize("tile", EPILOGUE_TILES, ids=tname)
def test_epilogues(ops, dev, tile):
    """bias; residual; bias + ReLU + colscale + residual + C_pre; FiLM with film_rows dividing neither BM nor M: exact.  The four activations
    within 1 bf16 ulp of float64 (erf-GELU: + 2e-7 |z|), their C_pre exact; pre-activations in about [-6, 6]."""
    c, fails = cfg_of(tile), Failures()
    M, N = 2 * c.BM + 37, c.BN + 24
    K = 64 if c.fam == "w4" else 72
    g = R.rng(3000 + tile)
    a, b = R.operand(g, M, K), R.operand(g, N, K)
    bias, res, cs = R.bias_like(g, N), R.bias_like(g, M, N), R.colscale_like(g, N)
    rows = 50
    gamma, beta = R.film_like(g, -(-M // rows), N)
    ad, bd, biasd, resd, csd, gd, btd = (t.to(dev) for t in (a, b, bias, res, cs, gamma, beta))
    tl = (c.BM, c.BN)
    for alpha in R.ALPHAS:
        fails.exact(ops.gemm(ad, bd, bias=biasd, alpha=alpha, tile=tile), R.reference(a, b, bias=bias, alpha=alpha).out, f"{tname(tile)} bias alpha {alpha}", tl)
    fails.exact(ops.gemm(ad, bd, residual=resd, tile=tile), R.reference(a, b, residual=res).out, f"{tname(tile)} residual", tl)
    pre = torch.full((M, N), float("nan"), dtype=BF, device=dev)
    ref = R.reference(a, b, bias=bias, act=R.ACT_RELU, colscale=cs, residual=res, alpha=0.5)
    fails.exact(ops.gemm(ad, bd, bias=biasd, act=R.ACT_RELU, colscale=csd, residual=resd, c_pre=pre, alpha=0.5, tile=tile), ref.out, f"{tname(tile)} bias+relu+colscale+residual", tl)
    fails.exact(pre, ref.c_pre, f"{tname(tile)} C_pre of bias+relu+colscale+residual", tl)
    pre = torch.full((M, N), float("nan"), dtype=BF, device=dev)
    ref = R.reference(a, b, residual=res, film=(gamma, beta, rows), alpha=0.5)
    fails.exact(ops.gemm(ad, bd, residual=resd, film=(gd, btd, rows), c_pre=pre, alpha=0.5, tile=tile), ref.out, f"{tname(tile)} FiLM rows {rows}", tl)
    fails.exact(pre, ref.c_pre, f"{tname(tile)} pre-FiLM C_pre", tl)
    sbias = (R.ints(g, (N,), -4, 4).float() * 0.25).to(BF)                 # z = 2^-5 acc + bias: standard deviation 1.2, a few elements out to +-6
    for act, name in [(R.ACT_GELU, "gelu"), (R.ACT_SILU, "silu"), (R.ACT_GELU_TANH, "gelu_tanh")]:
        pre = torch.full((M, N), float("nan"), dtype=BF, device=dev)
        ref = R.reference(a, b, bias=sbias, act=act, alpha=2.0 ** -5)
        out = ops.gemm(ad, bd, bias=sbias.to(dev), act=act, c_pre=pre, alpha=2.0 ** -5, tile=tile)
        fails.exact(pre, ref.c_pre, f"{tname(tile)} pre-activation of {name}", tl)
        floor = R.ERF_FLOOR * ref.z64.abs() if act == R.ACT_GELU else None
        _note(name, fails.ulps(out, ref.out64, R.ULPS[name], f"{tname(tile)} {name}", floor, tl))
        fails.check(float(ref.z64.abs().max()) <= 8.0 and float(ref.z64.abs().max()) >= 4.0, f"{name}: pre-activations span +-{float(ref.z64.abs().max())}, not about +-6")
    fails.done()


# ---- K-extension ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", FORCED + [118, 122], ids=tname)
def test_k_extension(ops, dev, tile):
    """K2 in {8, 16, 32, 64, 96} where the configuration takes it, ungrouped and grouped (group = BN with 2 groups, 2 BN with 3), A2 wider
    than its G * K2 columns (lda2 > G * K2).  What a configuration does not take is refused with its message."""
    c, fails = cfg_of(tile), Failures()
    K = 64 if c.fam == "w4" else 72
    g = R.rng(4000 + tile)
    for K2 in (8, 16, 32, 64, 96):
        for G, group in [(1, 0), (2, c.BN), (3, 2 * c.BN)]:
            M, N = c.BM + 1, (G * group if G > 1 else c.BN + 8)
            a, b, a2, b2 = R.operand(g, M, K), R.operand(g, N, K), R.operand(g, M, G * K2), R.operand(g, N, K2)
            wide = R.embed(a2.to(dev), align=8, top=0, bottom=0, left=0, right=2, fill="nan")
            kw = dict(a2=wide.view, b2=b2.to(dev), k2_group_n=group, alpha=0.5, tile=tile)
            if c.kext is not ANY and K2 not in c.kext:
                with pytest.raises(RuntimeError, match="K-extension of 0"):
                    ops.gemm(a.to(dev), b.to(dev), **kw)
                continue
            ref = R.reference(a, b, a2=a2, b2=b2, k2_group_n=group, alpha=0.5).out
            fails.exact(ops.gemm(a.to(dev), b.to(dev), **kw), ref, f"{tname(tile)} K2 {K2} groups {G} x {group} ({M}x{N}x{K})", (c.BM, c.BN))
    fails.done()


# ---- RoPE ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rope_cols", [128, 256])
def test_rope_epilogue_same_exact_bits_on_every_variant(ops, dev, rope_cols):
    """rope_S = 77 against M = 2 BM + 37 (positions wrap inside and across row tiles), rope_cols < N (the columns beyond are the plain
    projection), tables that differ in every (position, column): the four fused variants (1 and 18: one head per column tile; 16: one head
    per wave slab; 17: interior tiles, M and rope_cols multiples of 256; 22: the column map), their +100 forms and tile 2, which appends
    the ovla_rope launch, all give the reference's bits."""
    fails = Failures()
    N, K, S = 512, 128, 77
    g = R.rng(5000 + rope_cols)
    cos, sin = R.rope_tables(g, S + 3)
    cosd, sind = cos.to(dev), sin.to(dev)
    for tile in [1, 101, 16, 116, 17, 117, 18, 118, 22, 122, 2]:
        c = cfg_of(tile)
        for M in [2 * c.BM + 37] + ([512] if tile % 100 == 17 else []):
            a, b = R.operand(g, M, K), R.operand(g, N, K)
            ref = R.reference(a, b, rope=(cos, sin, S, rope_cols))
            out = ops.gemm(a.to(dev), b.to(dev), rope=(cosd, sind, S, rope_cols), tile=tile)
            fails.exact(out, ref.out, f"{tname(tile)} rope {M}x{N}x{K} cols {rope_cols}", (c.BM, c.BN))
            fails.exact(out[:, rope_cols:], ref.z64[:, rope_cols:].to(BF), f"{tname(tile)} columns beyond rope_cols", (c.BM, c.BN))
    fails.done()


# ---- RMSNorm fold -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [1, 101, 22, 122], ids=tname)
def test_rmsnorm_fold(ops, dev, tile):
    """Producer: rowsq_out exact (K = 64 keeps |out| <= 256, so every 64-column sum of squares is an exact fp32 integer; the reference asserts
    it).  Consumer: C within 1 ulp of bf16(rstd * acc) in float64, rowscale_r within 3 fp32 roundings of float64's rstd: the slot sums are
    exact integers, the division by K and the addition of eps round once each (their error is halved by the square root) and rsqrtf is good
    to 1 ulp = 2 units: (1 + 1) / 2 + 2 = 3 units of 2^-24, asserted as 2^-22.
    Consumer with alpha no power of two: given the rowscale_r the launch wrote, C is bf16(fp32(acc) * fp32(alpha * rowscale_r[m])) to the bit
    (one factor, one multiplication: gemm_reference.fold_orders), in the interior tile and the edge tiles alike; the inputs are chosen so that
    (acc * rstd) * alpha gives other bits in both regions (tests/test_gemm_reference.py counts them on the CPU; re-counted here)."""
    c, fails = cfg_of(tile), Failures()
    g = R.rng(6000 + tile)
    M, N, K = c.BM + 37, c.BN + 64, 64
    a, b, res = R.operand(g, M, K), R.operand(g, N, K), R.bias_like(g, M, N)
    ref = R.reference(a, b, residual=res, rowsq=True)
    part = torch.full((M, N // 64), float("nan"), device=dev)
    out = ops.gemm(a.to(dev), b.to(dev), residual=res.to(dev), rowsq_out=part, tile=tile)
    fails.exact(out, ref.out, f"{tname(tile)} producer output", (c.BM, c.BN))
    fails.exact(part, ref.rowsq, f"{tname(tile)} rowsq_out")
    M, N, K, eps = c.BM + 37, c.BN + 24, 512, 1e-5
    a, b = R.operand(g, M, K), R.operand(g, N, K)
    parts = R.ints(g, (M, K // 64), 100, 3000, dtype=torch.float32)
    ref = R.reference(a, b, rowscale=(parts, eps))
    rbuf = torch.full((M,), float("nan"), device=dev)
    out = ops.gemm(a.to(dev), b.to(dev), rowscale=(parts.to(dev), eps, rbuf), tile=tile)
    _note("rowscale", fails.ulps(out, ref.out64, R.ULPS["rowscale"], f"{tname(tile)} consumer", None, (c.BM, c.BN)))
    rel = ((rbuf.cpu().double() - ref.rstd) / ref.rstd).abs().max().item()
    _note("rowscale_r (units of 2^-24)", rel * 2 ** 24)
    fails.check(rel <= 2.0 ** -22, f"{tname(tile)} rowscale_r: relative error {rel:.3e} > 2^-22")
    for alpha in R.FOLD_ALPHAS:
        a, b, parts, eps = R.fold_alpha_case(tile, c.BM, c.BN, alpha)
        rbuf = torch.full((M,), float("nan"), device=dev)
        out = ops.gemm(a.to(dev), b.to(dev), rowscale=(parts.to(dev), eps, rbuf), alpha=alpha, tile=tile)
        want, other = R.fold_orders(R.accumulate(a, b)[0], rbuf, alpha)
        fails.exact(out, want, f"{tname(tile)} consumer, alpha {alpha}: bf16(acc * (alpha * rowscale_r[m]))", (c.BM, c.BN))
        inner, edge = R.fold_told_apart(want, other, c.BM, c.BN)
        fails.check(inner >= 1 and edge >= 1, f"{tname(tile)} alpha {alpha}: with the launch's rowscale_r the two orders differ in {inner} interior and {edge} edge elements")
    fails.done()


# ---- one epilogue body: the path a tile takes changes no bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [1, 101, 17, 117, 18, 118, 22, 122], ids=tname)
def test_same_bits_whatever_path_the_tile_took(ops, dev, tile):
    """Rows [0, BM), columns [0, N - 64) computed twice from the same operand rows: inside an N-column launch of whole tiles (the unrolled or
    fused read-back of an interior tile) and as an (N - 64)-column launch (an edge tile: the rolled read-back; RoPE: refused, so the plain
    projection and the rope kernel).  Bit-identical, with alpha no power of two wherever the epilogue takes one (RoPE requires alpha 1).
    N = BN and K = 128; the fold consumer needs K = 512 (eight slots).  RoPE runs on N = 2 BN against 2 BN - 64 with rope_cols = BN on every
    tile: tile 17 fuses it only when all of M, N and rope_cols are multiples of 256, and tile 1's BN - 64 would be narrower than one head."""
    c, fails = cfg_of(tile), Failures()
    g = R.rng(6600 + tile)
    M, N, tl = c.BM, c.BN, (c.BM, c.BN)
    a, b, bias, res = R.operand(g, M, 128), R.operand(g, N, 128), R.bias_like(g, N), R.bias_like(g, M, N)
    ad, bd, biasd, resd = a.to(dev), b.to(dev), bias.to(dev), res.to(dev)
    whole = ops.gemm(ad, bd, bias=biasd, residual=resd, alpha=0.3, tile=tile)
    part = ops.gemm(ad, bd[:N - 64], bias=biasd[:N - 64], residual=resd[:, :N - 64], alpha=0.3, tile=tile)
    fails.exact(part, whole[:, :N - 64], f"{tname(tile)} bias + residual, alpha 0.3: edge tile against interior tile", tl)
    if tile % 100 in (1, 22):
        a, b, parts = R.fold_alpha_problem(g, M, N, 512, 0.3, 1e-5)      # (row sums under which the two multiplication orders round differently)
        outs = [ops.gemm(a.to(dev), b.to(dev)[:n], rowscale=(parts.to(dev), 1e-5, torch.empty(M, device=dev)), alpha=0.3, tile=tile) for n in (N, N - 64)]
        fails.exact(outs[1], outs[0][:, :N - 64], f"{tname(tile)} fold consumer, alpha 0.3: edge tile against interior tile", tl)
    S, N2 = 77, 2 * c.BN
    cos, sin = (t.to(dev) for t in R.rope_tables(g, S + 3))
    a, b = R.operand(g, M, 128).to(dev), R.operand(g, N2, 128).to(dev)
    outs = [ops.gemm(a, b[:n], rope=(cos, sin, S, c.BN), tile=tile) for n in (N2, N2 - 64)]
    fails.exact(outs[1], outs[0][:, :N2 - 64], f"{tname(tile)} rope: refused (N = {N2 - 64}) against fused (N = {N2})", tl)
    fails.done()


# ---- SwiGLU pair epilogue -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [18, 118, 22, 122], ids=tname)
def test_swiglu_pair_epilogue(ops, dev, tile):
    """F in {128, 384}; on 18 / 118 with and without the 32-column K-extension, ungrouped -- and grouped by F at F = 256: a K-extension group must
    be whole column tiles there, so F = 128 and 384 grouped are refused, as is any K-extension on the 128x256 configuration.  C_pre = the
    [M, 2 F] projection is exact, C within 2 ulps."""
    c, fails = cfg_of(tile), Failures()
    g = R.rng(7000 + tile)
    K, alpha = 64, 2.0 ** -5
    for F, K2, group in [(F, K2, grp and F) for F in (128, 384) for K2, grp in [(0, 0), (32, 0), (32, 1)]] + [(256, 32, 256)]:
        M = c.BM + 37
        a, b = R.operand(g, M, K), R.operand(g, 2 * F, K)
        kw, rkw = {}, {}
        if K2:
            G = 2 if group else 1
            a2, b2 = R.operand(g, M, G * K2), R.operand(g, 2 * F, K2)
            kw, rkw = dict(a2=a2.to(dev), b2=b2.to(dev), k2_group_n=group), dict(a2=a2, b2=b2, k2_group_n=group)
        refusal = "takes no K-extension" if (K2 and tile % 100 == 22) else "the 4-wave configs need K % 64 == 0, a K-extension" if group % c.BN else None
        if refusal:
            with pytest.raises(RuntimeError, match=refusal):
                ops.gemm(a.to(dev), b.to(dev), act=R.ACT_SWIGLU, alpha=alpha, tile=tile, **kw)
            continue
        ref = R.reference(a, b, act=R.ACT_SWIGLU, alpha=alpha, **rkw)
        pre = torch.full((M, 2 * F), float("nan"), dtype=BF, device=dev)
        out = ops.gemm(a.to(dev), b.to(dev), act=R.ACT_SWIGLU, alpha=alpha, c_pre=pre, tile=tile, **kw)
        what = f"{tname(tile)} swiglu F {F} K2 {K2} group {group}"
        fails.exact(pre, ref.c_pre, what + " C_pre", (c.BM, c.BN))
        fails.check(out.shape == (M, F), what + f": shape {tuple(out.shape)}")
        _note("swiglu", fails.ulps(out, ref.out64, R.ULPS["swiglu"], what))
    fails.done()


# ---- backward epilogues ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [1, 101, 17, 10, 18], ids=tname)
def test_backward_epilogues(ops, dev, tile):
    """dact_mode 1 with each activation (ReLU exact, the others within 1 ulp; erf-GELU + 2e-7 |z|) and dact_mode 2 with ldc = ld_dact = 2 N + 8
    (within 2 ulps; guard columns untouched).  Saved pre-activations are multiples of 1/4 in [-6, 6], the incoming gradient 2^-5 acc stays below 8.
    Row 0 also holds the extreme pre-activations -2e13, -1e19, -3e38 and +3e38 (the derivative there is 0 or 1; an unclamped tanh-GELU' is 0 * inf)."""
    c, fails = cfg_of(tile), Failures()
    g = R.rng(8000 + tile)
    M, N, K, alpha = c.BM + 37, c.BN + 24, 64, 2.0 ** -5
    a, b = R.operand(g, M, K), R.operand(g, N, K)
    ad, bd = a.to(dev), b.to(dev)
    z = (R.ints(g, (M, N), -24, 24).float() * 0.25).to(BF)
    z[0, :4] = torch.tensor([-2e13, -1e19, -3e38, 3e38]).to(BF)
    for act, name in [(R.ACT_GELU, "gelu"), (R.ACT_RELU, "relu"), (R.ACT_SILU, "silu"), (R.ACT_GELU_TANH, "gelu_tanh")]:
        ref = R.reference(a, b, alpha=alpha, dact=("act", z, act))
        out = ops.gemm(ad, bd, alpha=alpha, dact=("act", z.to(dev), act), tile=tile)
        fails.check(float(ref.z64.abs().max()) <= 8.0, "incoming gradient beyond 8")
        if act == R.ACT_RELU:
            fails.exact(out, ref.out, f"{tname(tile)} dact relu", (c.BM, c.BN))
        else:
            floor = R.ERF_FLOOR * z.double().abs() if act == R.ACT_GELU else None
            _note(f"dact1 {name}", fails.ulps(out, ref.out64, R.ULPS["dact1"], f"{tname(tile)} dact {name}", floor, (c.BM, c.BN)))
    gu = (R.ints(g, (M, 2 * N), -24, 24).float() * 0.25).to(BF)
    src = R.embed(gu.to(dev), align=4, top=1, bottom=1, left=0, right=2, fill="nan")
    out = R.embed(BF, shape=(M, 2 * N), align=4, top=1, bottom=1, left=0, right=2, fill="sentinel", device=dev)
    assert src.view.stride(0) == 2 * N + 8 and out.view.stride(0) == 2 * N + 8
    ref = R.reference(a, b, alpha=alpha, dact=("swiglu", gu))
    ops.gemm(ad, bd, alpha=alpha, dact=("swiglu", src.view), out=out.view, tile=tile)
    _note("dact2", fails.ulps(out.view, ref.out64, R.ULPS["dact2"], f"{tname(tile)} dact swiglu"))
    out.assert_guards(f"{tname(tile)} dact swiglu")
    fails.done()


# ---- split-K ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", FORCED + PLUS100, ids=tname)
def test_split_k(ops, dev, tile):
    """split_k in {2, 3, 8} at ragged M and N with bias + ReLU, which then runs in the reduce kernel.  11 K tiles: no multiple of a split, and
    8 splits of 2 tiles leave the last two slabs empty; 5 K tiles with split_k = 8: the split is clamped to the tile count."""
    c, fails = cfg_of(tile), Failures()
    g = R.rng(9000 + tile)
    M, N = c.BM + 37, c.BN + 24
    for T, splits in [(11, 2), (11, 3), (11, 8), (5, 8)]:
        K = T * c.BK
        a, b, bias = R.operand(g, M, K), R.operand(g, N, K), R.bias_like(g, N)
        ref = R.reference(a, b, bias=bias, act=R.ACT_RELU, alpha=0.5).out
        out = ops.gemm(a.to(dev), b.to(dev), bias=bias.to(dev), act=R.ACT_RELU, alpha=0.5, split_k=splits, tile=tile)
        fails.exact(out, ref, f"{tname(tile)} split_k {splits} over {T} K tiles ({M}x{N}x{K})", (c.BM, c.BN))
    fails.done()


# ---- hybrid remainder ----------------------------------------------------------------------------------------------------------------------------------------
WS_SENTINEL = 0x7FA5A5A5


@pytest.mark.parametrize("tile", PLUS100, ids=tname)
def test_hybrid_remainder(ops, dev, tile):
    """9 tiles (far from a round of the chip) over 33 K tiles: the planner splits the remainder.  That a split RAN is established, not assumed:
    the fp32 workspace is filled with a sentinel and slab storage must have changed.  Separate reduce kernel and in-launch reduce give the
    reference's bits; the arrival counters are zero afterwards."""
    c, fails = cfg_of(tile), Failures()
    g = R.rng(10000 + tile)
    M, N, K = 2 * c.BM + 37, 2 * c.BN + 24, 33 * 64
    a, b, bias, res = R.operand(g, M, K), R.operand(g, N, K), R.bias_like(g, N), R.bias_like(g, M, N)
    a2, b2 = R.operand(g, M, 32), R.operand(g, N, 32)
    ref = R.reference(a, b, a2=a2, b2=b2, bias=bias, residual=res, alpha=0.5).out
    kw = dict(a2=a2.to(dev), b2=b2.to(dev), bias=bias.to(dev), residual=res.to(dev), alpha=0.5, tile=tile)
    ad, bd = a.to(dev), b.to(dev)
    ws = ops._workspace(dev, ops._WS_BYTES)
    prev = ops._HYB_INLAUNCH
    try:
        for inlaunch in (False, True):
            ops._HYB_INLAUNCH = inlaunch
            ws.view(torch.int32).fill_(WS_SENTINEL)
            out = ops.gemm(ad, bd, **kw)
            assert ops._workspace(dev, ops._WS_BYTES) is ws
            changed = int((ws.view(torch.int32) != WS_SENTINEL).sum().item())
            fails.check(changed >= 2 * c.BM * c.BN, f"{tname(tile)}: no K split ran at {M}x{N}x{K} ({changed} workspace floats written): not a test of the remainder schedule")
            fails.exact(out, ref, f"{tname(tile)} hybrid {'in-launch reduce' if inlaunch else 'reduce kernel'} {M}x{N}x{K}", (c.BM, c.BN))
        torch.cuda.synchronize()
        fails.check(int(ops._hybrid_counters(dev).abs().sum().item()) == 0, "arrival counters must be zero after the launches")
    finally:
        ops._HYB_INLAUNCH = prev
    fails.done()


# ---- the fixed schedule ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", FIXED_TILES, ids=tname)
def test_fixed_schedule_every_tile_and_split(ops, dev, tile):
    """ovla_gemm_bf16_fixed under every (tile, splits) it accepts: K = 64 (4 splits) + 64, the smallest K a split takes plus one tile (so the
    last slab is uneven), M in {8, BM + 1, 2 BM + 37}; plain, bias + residual and, where the tile fuses them, RoPE and SwiGLU -- refused with
    the library's message elsewhere, as is SwiGLU's C_pre.  All exact; rows [:8] have the same bits for the three M; splits * 4 > K tiles is refused."""
    c, fails = cfg_of(tile), Failures()
    g = R.rng(11000 + tile)
    tl = (c.BM, c.BN)
    Ms = [8, c.BM + 1, 2 * c.BM + 37]
    cos, sin = R.rope_tables(g, 80)
    for splits in FIXED_SPLITS:
        K = 64 * 4 * splits + 64
        sched = (tile, splits)
        N = c.BN + 24
        A, b, bias, RES = R.operand(g, max(Ms), K), R.operand(g, N, K), R.bias_like(g, N), R.bias_like(g, max(Ms), N)
        bR, bS = R.operand(g, 512, K), R.operand(g, 256, K)
        Ad, bd, biasd, RESd, bRd, bSd = (t.to(dev) for t in (A, b, bias, RES, bR, bS))
        first = {}
        for M in Ms:
            a, res, ad, resd = A[:M].contiguous(), RES[:M].contiguous(), Ad[:M].contiguous(), RESd[:M].contiguous()
            what = f"fixed ({tile}, {splits}) M {M} K {K}"
            outs = {}
            outs["plain"] = ops.gemm(ad, bd, schedule=sched)
            fails.exact(outs["plain"], R.reference(a, b).out, what + " plain", tl)
            outs["bias_res"] = ops.gemm(ad, bd, bias=biasd, residual=resd, alpha=0.5, schedule=sched)
            fails.exact(outs["bias_res"], R.reference(a, b, bias=bias, residual=res, alpha=0.5).out, what + " bias + residual", tl)
            rope_kw = dict(rope=(cos.to(dev), sin.to(dev), 77, 256), schedule=sched)
            if tile in (1, 18, 22):
                outs["rope"] = ops.gemm(ad, bRd, **rope_kw)
                fails.exact(outs["rope"], R.reference(a, bR, rope=(cos, sin, 77, 256)).out, what + " rope", tl)
            elif M == Ms[0]:
                with pytest.raises(RuntimeError, match="RoPE runs fused on tiles 1, 18 and 22 only"):
                    ops.gemm(ad, bRd, **rope_kw)
            if tile in (18, 22):
                ref = R.reference(a, bS, act=R.ACT_SWIGLU, alpha=2.0 ** -6)
                outs["swiglu"] = ops.gemm(ad, bSd, act=R.ACT_SWIGLU, alpha=2.0 ** -6, schedule=sched)
                if M == Ms[0]:      # C_pre (kept by training only) is not part of a fixed schedule on the 4-wave configurations
                    with pytest.raises(RuntimeError, match="take alpha, 16-byte aligned bias / residual"):
                        ops.gemm(ad, bSd, act=R.ACT_SWIGLU, c_pre=torch.empty((M, 256), dtype=BF, device=dev), schedule=sched)
                _note("swiglu", fails.ulps(outs["swiglu"], ref.out64, R.ULPS["swiglu"], what + " swiglu"))
            elif M == Ms[0]:
                with pytest.raises(RuntimeError, match="runs on the 4-wave configurations only"):
                    ops.gemm(ad, bSd, act=R.ACT_SWIGLU, schedule=sched)
            for k, o in outs.items():
                fails.check(torch.equal(first.setdefault(k, o[:8].clone()), o[:8]), what + f" {k}: rows [:8] differ from those of M = {Ms[0]}")
        if splits > 1:
            Kbad = 64 * 4 * splits - 64
            with pytest.raises(RuntimeError, match=f"{splits} splits need K >= {splits * 4 * 64}"):
                ops.gemm(Ad[:8, :Kbad].contiguous(), bd[:, :Kbad].contiguous(), schedule=sched)
    with pytest.raises(RuntimeError, match="is not a fixed schedule"):
        ops.gemm(Ad[:8], bd, schedule=(tile, 9))
    fails.done()


def test_fixed_schedule_refuses_other_tiles_and_modes(ops, dev):
    g = R.rng(12000)
    a, b = R.operand(g, 8, 320).to(dev), R.operand(g, 128, 320).to(dev)
    for tile in sorted(set(FORCED + PLUS100) - set(FIXED_TILES)):
        with pytest.raises(RuntimeError, match="is not a fixed schedule"):
            ops.gemm(a, b, schedule=(tile, 1))
    with pytest.raises(RuntimeError, match="the schedule replaces tile / split_k"):
        ops.gemm(a, b, schedule=(1, 1), tile=1)
    with pytest.raises(RuntimeError, match="the schedule replaces tile / split_k"):
        ops.gemm(a, b, schedule=(1, 1), dact=("act", torch.zeros((8, 128), dtype=BF, device=dev), R.ACT_RELU))
    with pytest.raises(RuntimeError, match="take alpha, 16-byte aligned bias / residual"):
        ops.gemm(a, b, schedule=(18, 1), act=R.ACT_RELU)


# ---- the auto path ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_auto_path_on_both_sides_of_every_threshold(ops, dev):
    """`tile = 0` on both sides of each special case of gemm_run, with the kernel instance the library says it ran: a threshold edit cannot
    quietly move a case onto another kernel."""
    fails = Failures()
    g = R.rng(13000)
    cases = [   # M, N, K, expected instance
        (512, 32, 3072, "gemm_nt_t6"), (511, 32, 3072, "gemm_nt_t5"), (512, 32, 3080, "gemm_nt_t5"),      # the skinny kernel: N = 32, K <= 3072, M >= 512
        (100, 32, 72, "gemm_nt_t5"), (100, 40, 72, "gemm_nt_t2"),                                          # N <= 32
        (64, 136, 72, "gemm_nt_t2"), (65, 128, 72, "gemm_nt_t2"), (65, 136, 72, None),                     # M <= 64 or N <= 128; beyond: the planner's pick
        (2285, 2048, 4096, "gemm_nt_t18k0"), (2285, 2048, 4032, "gemm_nt_t17"),                            # the 17 -> 18 upgrade at K >= 4096
    ]
    for M, N, K, want in cases:
        a, b = R.operand(g, M, K), R.operand(g, N, K)
        if want is None:
            want = f"gemm_nt_t{ops.gemm_plan(M, N, K)[0]}"
        if K >= 4032:
            fails.check(ops.gemm_plan(M, N, K)[0] == 17, f"the planner no longer gives {M}x{N}x{K} to the 256x256 tile: choose another shape")
        out, fams = resolved_family(ops, lambda: ops.gemm(a.to(dev), b.to(dev), alpha=0.5))
        fails.check(fams == [want], f"auto {M}x{N}x{K}: ran {fams}, expected {want}")
        fails.exact(out, R.reference(a, b, alpha=0.5).out, f"auto {M}x{N}x{K} ({want})")
    for gn, want in [(32, "gemm_nt_t5"), (128, "gemm_nt_t1")]:      # block-diagonal mode, 3 groups
        M, K, G = 165, 136, 3
        a, b = R.operand(g, M, G * K), R.operand(g, G * gn, K)
        out, fams = resolved_family(ops, lambda: ops.gemm(a.to(dev), b.to(dev), alpha=0.5, a_group_n=gn))
        fails.check(fams == [want], f"block-diagonal a_group_n {gn}: ran {fams}, expected {want}")
        fails.exact(out, R.reference(a, b, alpha=0.5, a_group_n=gn).out, f"block-diagonal a_group_n {gn}")
    fails.done()


def test_zz_report_worst_ulps():
    """Not a check of its own: prints the worst |err| / ulp each non-exact epilogue reached in this run (DESIGN.md section 5 records them)."""
    for k in sorted(ACT_WORST):
        print(f"worst |err|/ulp  {k}: {ACT_WORST[k]:.3f}")
