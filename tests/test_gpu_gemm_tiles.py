"""GPU: every tile of the GEMM family ALONE (linetr_debug_gemm_case) against a float64 reference at the shapes where its tiles end.

Tiles: the SplitTile kernels of lt_gemm_split.h / lt_gemm_split16.h / lt_gemm_small.h in the three split modes, the F32Tile kernels
of lt_gemm.h in f32, and the weight-stationary kernel of lt_gemm_ws.h.  Cases, input families and the bars are in gemm_cases.py; every
comparison asserts the kernel that ran (`tile_used`).  Shape grid notes: with M <= 769 and N <= 768 the tile counts 7 and 17 cannot be
factored for every tile; gemm_cases.count_shape then takes the nearest count with the same property (fewer tiles than XCDs; more
than two tiles per XCD with a remainder).  tools/gemm_unit_report.py runs the same cases and writes profiles/gemm_unit_errors.txt."""
import ctypes as C

import pytest
import torch

import gemm_cases as G

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
E_ARG = -1

TILE_MODE = [(t, m) for m in G.MODES for t in G.tiles_of(m)]
EPILOGUES = [(0, False), (1, True), (3, True)]       # (a) bias only, (b) bias + ReLU + residual, (c) distance epilogue + residual


@pytest.fixture(scope="module")
def eng():
    from linetr_amd.engine import Engine
    from workloads import synth
    e = Engine(synth.make_state_dict(0), "cuda:0")
    yield e
    e.set_precision("bf16x6")


def in_mode(eng, mode):
    eng.set_precision(mode)
    return eng


def exact_failures(eng, tile, p, want_tile=None, **kw):
    Y, used = G.launch(eng, p, tile, **kw)
    assert used == (want_tile or tile), (used, tile)
    ref64, _ = G.references(p, kw.get("act", 0), kw.get("residual", False))
    n, first = G.mismatches(Y, ref64)
    return [f"{used} {p['family']} M={p['M']} N={p['N']} K={p['K']} {kw}: {n} mismatches, first (g, row, col, got, want) {first}"] if n else []


def normal_failures(eng, mode, tile, p, want_tile=None, ref=None, **kw):
    Y, used = G.launch(eng, p, tile, **kw)
    assert used == (want_tile or tile), (used, tile)
    ref64, ref32 = G.references(p, kw.get("act", 0), kw.get("residual", False), kw.get("norm", 0), kw.get("add2", False))
    err = (Y.double() - ref64).abs().max().item()
    bar = G.bar(mode, ref64, ref32)
    print(f"{mode} {used} {p['family']} M={p['M']} N={p['N']} K={p['K']} {kw}: err {err:.3e} bar {bar:.3e} ratio {err / bar:.3f}")
    return ([] if err <= bar else [f"{mode} {used} M={p['M']} N={p['N']} K={p['K']} {kw}: error {err:.3e} > bar {bar:.3e}"]), Y


# ---- exact and onehot: bit for bit, every tile x every mode --------------------------------------------------------------------

@pytest.mark.parametrize("tile,mode", TILE_MODE)
def test_tile_exact(eng, tile, mode):
    """`exact` and `onehot` over the tile's shape grid with the three epilogues, contiguous and row-strided A / Y / R: bit for bit."""
    in_mode(eng, mode)
    bad = []
    for i, (M, N, K) in enumerate(G.shape_grid(tile, mode)):
        for family in ("exact", "onehot"):
            p = G.problem(family, M, N, K)
            for j, (act, res) in enumerate(EPILOGUES):
                for strided in (False, True):
                    bad += exact_failures(eng, tile, p, act=act, residual=res, strided=strided)
    assert not bad, "\n".join(bad[:20])


def test_ws_exact(eng):
    """the weight-stationary kernel (bf16x6, 128 -> 256, bias, none / ReLU) at M around its 64-row tile"""
    in_mode(eng, "bf16x6")
    bad = []
    for M, N, K in G.shape_grid(G.WS, "bf16x6"):
        for family in ("exact", "onehot"):
            for act in (0, 1):
                for strided in (False, True):
                    bad += exact_failures(eng, G.WS, G.problem(family, M, N, K), act=act, strided=strided)
    assert not bad, "\n".join(bad[:20])


# ---- normal and sentinel ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile,mode", TILE_MODE)
def test_tile_normal_and_sentinel(eng, tile, mode):
    """f32 and bf16x6: `normal` (tight views) and `sentinel` (row-strided views in +-1e4 surroundings) with all four activations and
    a residual, against the fp32-class bar; the two-plane modes: `normal` against their stated tolerances."""
    in_mode(eng, mode)
    bad = []
    grid = G.shape_grid(tile, mode)
    for i, (M, N, K) in enumerate(grid):
        for family in (("normal", "sentinel") if mode in ("f32", "bf16x6") else ("normal",)):
            for act in (0, 1, 2, 3):
                bad += normal_failures(eng, mode, tile, G.problem(family, M, N, K), act=act, residual=True,
                                       strided=family == "sentinel")[0]
    assert not bad, "\n".join(bad[:20])


def test_ws_normal_and_sentinel(eng):
    in_mode(eng, "bf16x6")
    bad = []
    for M, N, K in G.shape_grid(G.WS, "bf16x6"):
        for family in ("normal", "sentinel"):
            for act in (0, 1):
                bad += normal_failures(eng, "bf16x6", G.WS, G.problem(family, M, N, K), act=act, strided=family == "sentinel")[0]
    assert not bad, "\n".join(bad[:20])


# ---- the concatenated left operand [A | A2] -----------------------------------------------------------------------------------------

CONCAT_TILES = [(t, m) for t, m in TILE_MODE]          # every kernel of the family stages A through the same K1 switch


@pytest.mark.parametrize("tile,mode", CONCAT_TILES)
def test_tile_concat(eng, tile, mode):
    """[A | A2] with the split point K1 at 32, K - 32 and K / 2 (on and off a K-tile pair boundary), lda2 != lda: `exact` bit for bit
    against float64, i.e. also against the same tile on the materialised concatenation (test_tile_exact holds it to the same
    reference), which is launched once more here and compared directly."""
    in_mode(eng, mode)
    BM, BN = G.tile_dims(tile, mode)
    bad = []
    for K in ((128, 160, 544) if tile != "32x32k4" else (128, 160, 256, 544)):
        M, N = 2 * BM + 1, G.n_unit(tile, mode)
        p = G.problem("exact", M, N, K)
        whole, used = G.launch(eng, p, tile, act=1, residual=True)
        assert used == tile
        for K1 in sorted({32, K - 32, (K // 2 + 31) // 32 * 32, 64}):
            if not 0 < K1 < K:
                continue
            bad += exact_failures(eng, tile, p, act=1, residual=True, K1=K1)
            Y, _ = G.launch(eng, p, tile, act=1, residual=True, K1=K1, strided=False)
            if not torch.equal(Y, whole):
                bad.append(f"{tile} {mode} K={K} K1={K1}: differs from the same tile on torch.cat([A, A2], 1)")
    assert not bad, "\n".join(bad[:20])


# ---- grouped launches ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile,mode", [("128x64", "bf16x6"), ("64x64", "bf16x6"), ("32x32k4", "bf16x6"), ("128x64", "bf16x3"),
                                       ("64x64", "f16x3"), ("64x128", "f32"), ("128x64", "f32")])
@pytest.mark.parametrize("groups", [1, 2, 4])
def test_tile_groups(eng, tile, mode, groups):
    """1, 2 and 4 groups with a shared A (gA = 0) and with one A per group: `exact` bit for bit against float64 and against the
    ungrouped call on each group's slice; `sentinel`: every second group's operands hold +-1e4 and the other groups still meet the
    bar."""
    in_mode(eng, mode)
    BM, BN = G.tile_dims(tile, mode)
    bad = []
    for shared in (True, False):
        for M, K in ((BM + 1, 160), (2 * BM + 1, 544 if tile == "32x32k4" else 96)):
            N = G.n_unit(tile, mode)
            p = G.problem("exact", M, N, K, groups, shared)
            Y, used = G.launch(eng, p, tile, act=1)
            assert used == tile
            n, first = G.mismatches(Y, G.references(p, 1)[0])
            if n:
                bad.append(f"{tile} {mode} groups={groups} shared={shared} M={M} K={K}: {n} mismatches {first}")
            for gi in range(groups):
                one = dict(p, groups=1, shared_a=True, A=p["A"][gi if not shared else 0][None], W=p["W"][gi * N:(gi + 1) * N],
                           bias=p["bias"][gi * N:(gi + 1) * N])
                Y1, _ = G.launch(eng, one, tile, act=1)
                if not torch.equal(Y1[0], Y[gi]):
                    bad.append(f"{tile} {mode} groups={groups} shared={shared} group {gi}: differs from the ungrouped call")
            if groups > 1 and mode in ("f32", "bf16x6"):
                ps = G.problem("sentinel", M, N, K, groups, shared)
                odd = tuple(range(1, groups, 2))
                Ys, used = G.launch(eng, ps, tile, act=1, bad_groups=odd)
                r64, r32 = G.references(ps, 1)
                for gi in range(0, groups, 2):
                    err = (Ys[gi].double() - r64[gi]).abs().max().item()
                    if not err <= G.bar(mode, r64[gi], r32[gi]):
                        bad.append(f"{tile} {mode} groups={groups} sentinel group {gi}: error {err:.3e}")
    assert not bad, "\n".join(bad[:20])


# ---- the row normalisation fused into the 128x256 epilogue, and row_norm_kernel ------------------------------------------------------

@pytest.mark.parametrize("mode", ["bf16x6", "bf16x3", "f16x3"])
@pytest.mark.parametrize("norm", [1, 2])
def test_fused_norm(eng, mode, norm):
    """128x256, N = 256, M around the tile: LayerNorm and L2, with and without add2 and R, against float64 (a restatement of
    GemmArgs::norm) and against the row_norm_kernel path on the same inputs, within the same bar.  (This is the test that found
    row_norm_kernel dropping add2 behind the L2 normalisation: errors of 2.6 - 4.5 against bars of 2e-6 - 1e-4, every M and mode.)"""
    in_mode(eng, mode)
    bad = []
    for M in (1, 127, 128, 129, 257):
        for K in (96, 544):
            p = G.problem("normal", M, 256, K)
            for add2 in (False, True):
                for res in (False, True):
                    kw = dict(residual=res, norm=norm, add2=add2, strided=True)
                    f, Yf = normal_failures(eng, mode, "128x256", p, **kw)
                    r, Yr = normal_failures(eng, mode, "128x256", p, via_row_norm=True, **kw)
                    bad += f + r
                    r64, r32 = G.references(p, 0, res, norm, add2)
                    d = (Yf.double() - Yr.double()).abs().max().item()
                    if not d <= G.bar(mode, r64, r32):
                        bad.append(f"{mode} norm={norm} M={M} K={K}: fused and row_norm_kernel differ by {d:.3e}")
    assert not bad, "\n".join(bad[:20])


def test_row_norm_behind_every_f32_tile(eng):
    in_mode(eng, "f32")
    bad = []
    for tile in G.F32_TILES:
        for norm in (1, 2):
            bad += normal_failures(eng, "f32", tile, G.problem("normal", 129, 256, 96), residual=True, norm=norm, add2=True,
                                   via_row_norm=True)[0]
    assert not bad, "\n".join(bad)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------

def test_refusals(eng):
    """What a kernel is not written for is refused with LINETR_E_ARG (a NativeError with the message) and Y keeps its marker:
    gemm_cases.launch checks the whole marked output buffer when the call raises, before it passes the exception on."""
    from linetr_amd._native import NativeError
    bad = []

    def refused(what, mode, tile, p, **kw):
        in_mode(eng, mode)
        try:
            G.launch(eng, p, tile, **kw)
        except NativeError as e:
            if f"error {E_ARG}:" not in str(e):
                bad.append((what, str(e)))
        else:
            bad.append((what, "launched"))

    p = G.problem("normal", 129, 256, 128)
    for tile in ("64x64", "64x256", "128x128s", "32x32k4", "112x256"):
        refused(f"fused norm on {tile}", "bf16x3", tile, p, norm=1)
    refused("fused norm in f32", "f32", "128x128", p, norm=2)
    refused("fused norm on ws", "bf16x6", G.WS, p, norm=2)
    refused("ws with a residual", "bf16x6", G.WS, p, residual=True)
    refused("ws with GELU", "bf16x6", G.WS, p, act=2)
    refused("ws with A2", "bf16x6", G.WS, p, K1=64)
    refused("ws in bf16x3", "bf16x3", G.WS, p)
    refused("ws at K = 160", "bf16x6", G.WS, G.problem("normal", 129, 256, 160))
    refused("ws at N = 512", "bf16x6", G.WS, G.problem("normal", 129, 512, 128))
    refused("ws with groups", "bf16x6", G.WS, G.problem("normal", 65, 256, 128, 2))
    refused("112x256 with groups", "bf16x3", "112x256", G.problem("normal", 65, 256, 128, 2))
    refused("fused norm, N = 512", "bf16x6", "128x256", G.problem("normal", 129, 512, 128), norm=1)
    # K1 not a multiple of 32: straight through the C entry point (the wrapper takes K1 from A's shape)
    in_mode(eng, "bf16x6")
    from linetr_amd import _native as nat
    A = torch.zeros((8, 256), device="cuda:0")
    W = torch.zeros((64, 128), device="cuda:0")
    Y = torch.full((8, 64), G.MARKER, device="cuda:0")
    for K1 in (16, 48, 100, 0, 128):
        c = nat.GemmCase(A=A.data_ptr(), lda=256, A2=A.data_ptr() + 512, lda2=256, K1=K1, W=W.data_ptr(), bias=None, R=None,
                         Y=Y.data_ptr(), ldy=64, M=8, N=64, K=128, act=0, groups=1, gA=0, gY=0, norm=0, gamma=None, beta=None,
                         add2=None, eps=0.0, via_row_norm=0, tile=-1)
        code = eng._L.linetr_debug_gemm_case(eng._h, C.byref(c), None, None)
        text = eng._L.linetr_last_error().decode()
        if code != E_ARG or "K1" not in text:
            bad.append((f"K1 = {K1}", code, text))
    torch.cuda.synchronize()
    assert bool((Y == G.MARKER).all())
    assert not bad, bad


def test_launcher_fallbacks(eng):
    """tile_used is what launches: a 256-wide tile on N % 256 != 0 takes 64x128, any tile on N % 128 != 0 takes 128x64 (the
    K-split kernel keeps its 32-wide tiles), 256x256 is not built in the product; each fallback computes the exact result."""
    bad = []
    for mode, tile, N, want in [("bf16x6", "128x256", 384, "64x128"), ("bf16x6", "64x256", 128, "64x128"), ("bf16x3", "112x256", 384, "64x128"),
                                ("bf16x3", "112x256", 192, "128x64"), ("bf16x6", "128x128s", 192, "128x64"), ("bf16x6", "32x32k4", 192, "32x32k4"),
                                ("bf16x3", "256x256", 512, "64x128"), ("bf16x6", "256x256", 256, "64x128"), ("f32", "128x128", 192, "128x64")]:
        in_mode(eng, mode)
        assert eng.gemm_tile(129, N, 160, tile=tile) == want, (mode, tile, N)
        bad += exact_failures(eng, tile, G.problem("exact", 129, N, 160), want_tile=want, act=1, residual=True)
    assert not bad, "\n".join(bad)


# ---- the dispatch table ----------------------------------------------------------------------------------------------------------------

R, G2 = dict(residual=True), dict(act=2)
DISPATCH = [   # (mode, M, N, K, keywords of Engine.gemm_tile, kernel): both sides of every threshold
    # small_gemm_wins: fewer than 256 tiles of 64 x 64, K >= 128
    ("bf16x6", 64 * 255, 64, 128, {}, "32x32k4"), ("bf16x6", 64 * 255 + 1, 64, 128, {}, "128x64"), ("bf16x6", 64, 64, 96, {}, "128x64"),
    ("bf16x6", 8128, 128, 128, {}, "32x32k4"), ("bf16x6", 8192, 128, 128, {}, "64x64"), ("bf16x6", 64, 128, 128, dict(groups=128), "64x64"),
    ("bf16x6", 64, 128, 128, dict(groups=127), "32x32k4"), ("bf16x3", 398, 768, 256, {}, "32x32k4"), ("f16x3", 1, 64, 128, {}, "32x32k4"),
    # N % 128 != 0
    ("bf16x6", 70000, 64, 32, {}, "128x64"), ("bf16x6", 20000, 192, 256, {}, "128x64"), ("bf16x3", 20000, 192, 256, {}, "128x64"),
    # split16_wins (two-plane modes): one group, N % 256 == 0, at least 192 tiles of 128 x 256, a round of blocks saved
    ("bf16x3", 25472, 256, 512, {}, "112x256"), ("f16x3", 25472, 256, 512, {}, "112x256"), ("bf16x6", 25472, 256, 512, {}, "128x256"),
    ("bf16x3", 24448, 256, 512, {}, "128x256"), ("bf16x3", 24576, 256, 512, {}, "112x256"), ("bf16x3", 32768, 256, 512, {}, "128x256"),
    ("bf16x3", 25472, 768, 256, {}, "112x256"), ("bf16x3", 12736, 256, 512, dict(groups=2), "128x256"),
    # 128x128s (bf16x6): K <= 256, N >= 768, 400 tiles of 128 x 128 -- or K <= 128 and 1024 tiles
    ("bf16x6", 8576, 768, 256, {}, "128x128s"), ("bf16x6", 8448, 768, 256, {}, "128x256"), ("bf16x6", 8576, 768, 288, {}, "128x256"),
    ("bf16x6", 25472, 512, 256, {}, "128x256"), ("bf16x6", 65536, 256, 128, R, "128x128s"), ("bf16x6", 65408, 256, 128, R, "128x256"),
    ("bf16x6", 65536, 256, 160, R, "128x256"), ("bf16x3", 8576, 768, 256, {}, "112x256"),
    # 128x256: N % 256 == 0 and 140 tiles
    ("bf16x6", 17920, 256, 1024, {}, "128x256"), ("bf16x6", 17792, 256, 1024, {}, "64x256"),
    # 128x128s once more: K <= 512 and 140 tiles of 128 x 128
    ("bf16x6", 9584, 256, 512, {}, "128x128s"), ("bf16x6", 9584, 256, 544, {}, "64x64"), ("bf16x6", 8960, 256, 512, {}, "128x128s"),
    ("bf16x6", 8832, 256, 512, {}, "64x64"),
    # 256x128: N % 256 != 0 and 192 tiles of 256 x 128; 128x128 behind it
    ("bf16x6", 16384, 384, 1024, {}, "256x128"), ("bf16x6", 16128, 384, 1024, {}, "128x128"), ("bf16x3", 16384, 384, 1024, {}, "256x128"),
    # 64x64 up to 768 tiles, 64x128 up to 512, then 64x256
    ("bf16x6", 12288, 256, 1024, {}, "64x64"), ("bf16x6", 12289, 256, 1024, {}, "64x128"), ("bf16x6", 16384, 256, 1024, {}, "64x128"),
    ("bf16x6", 16385, 256, 1024, {}, "64x256"),
    # gemm_ws_takes: bf16x6, 128 -> 256, none / ReLU, no residual, M >= 16384
    ("bf16x6", 16384, 256, 128, {}, "ws64x256"), ("bf16x6", 16384, 256, 128, dict(act=1), "ws64x256"), ("bf16x6", 16383, 256, 128, {}, "128x128s"),
    ("bf16x6", 16384, 256, 128, R, "128x128s"), ("bf16x6", 16384, 256, 128, G2, "128x128s"), ("bf16x6", 16384, 256, 128, dict(concat=True), "128x128s"),
    ("bf16x3", 16384, 256, 128, {}, "64x128"), ("bf16x6", 291208, 256, 128, {}, "ws64x256"),
    # f32_tile: N % 128 != 0; 384 tiles of 128 x 128
    ("f32", 70000, 64, 32, {}, "128x64"), ("f32", 49152, 128, 64, {}, "128x128"), ("f32", 49024, 128, 64, {}, "64x128"),
    ("f32", 398, 768, 256, {}, "64x128"), ("f32", 6144, 128, 64, dict(groups=8), "128x128"),
    # the workloads' shapes: cfg3 (25 472 sub-lines), cfg2 (one pair), cfg5 (9 584)
    ("bf16x6", 25472, 768, 256, {}, "128x128s"), ("bf16x6", 25472, 256, 512, R, "128x256"), ("bf16x6", 25472, 512, 512, dict(concat=True, act=1), "128x256"),
    ("bf16x6", 25472, 1024, 256, G2, "128x128s"), ("bf16x6", 25472, 256, 1024, R, "128x256"), ("bf16x6", 25472, 256, 768, dict(concat=True), "128x256"),
    ("bf16x6", 25472, 256, 256, {}, "128x256"), ("bf16x6", 291208, 256, 128, R, "128x128s"), ("bf16x6", 25472, 64, 544, dict(groups=4), "128x64"),
    ("bf16x6", 398, 768, 256, {}, "32x32k4"), ("bf16x6", 398, 512, 512, dict(concat=True, act=1), "32x32k4"), ("bf16x6", 398, 1024, 768, dict(concat=True), "32x32k4"),
    ("bf16x6", 9584, 1024, 256, G2, "128x128s"), ("bf16x6", 9584, 512, 512, dict(concat=True, act=1), "128x256"), ("bf16x6", 9584, 256, 1024, R, "64x64"),
]


def test_dispatch_table(eng):
    """Engine.gemm_tile launches nothing: workload-sized shapes on both sides of every threshold of split_tile, small_gemm_wins,
    split16_wins, gemm_ws_takes and f32_tile."""
    got = []
    for mode, M, N, K, kw, want in DISPATCH:
        in_mode(eng, mode)
        got.append((mode, M, N, K, kw, eng.gemm_tile(M, N, K, **kw)))
    assert got == DISPATCH, [(g, w[-1]) for g, w in zip(got, DISPATCH) if g != w]


# ---- the dispatcher's own choice, launched -----------------------------------------------------------------------------------------------

OWN_CHOICE = [   # (mode, M, N, K, kernel): the smallest M at which the dispatcher picks the tile by itself at K = 64 (32x32k4: K = 128)
    ("bf16x6", 1, 64, 128, "32x32k4"), ("bf16x6", 1, 64, 64, "128x64"), ("bf16x6", 1, 128, 64, "64x64"),
    ("bf16x6", 2945, 768, 64, "128x128s"), ("bf16x6", 5889, 768, 64, "128x256"),
    ("bf16x3", 12289, 256, 64, "64x128"), ("bf16x3", 16385, 256, 64, "64x256"), ("bf16x3", 17793, 256, 64, "128x256"),
    ("bf16x3", 24449, 256, 64, "112x256"), ("bf16x3", 16129, 384, 64, "256x128"), ("bf16x3", 10881, 384, 64, "128x128"),
    ("f32", 1, 64, 64, "128x64"), ("f32", 1, 128, 64, "64x128"), ("f32", 49025, 128, 64, "128x128"),
]


@pytest.mark.parametrize("mode,M,N,K,want", OWN_CHOICE)
def test_dispatchers_own_choice(eng, mode, M, N, K, want):
    """tile = -1: one launch per tile at the smallest M for which the dispatcher takes it by itself (the only larger shapes of this
    file), `exact` with a residual and ReLU, bit for bit."""
    in_mode(eng, mode)
    assert eng.gemm_tile(M, N, K, act=1, residual=True) == want
    assert eng.gemm_tile(M - 1, N, K, act=1, residual=True) != want or M == 1
    p = G.problem("exact", M, N, K)
    bad = exact_failures(eng, -1, p, want_tile=want, act=1, residual=True, strided=False)
    assert not bad, "\n".join(bad)


def test_dispatchers_own_choice_weight_stationary(eng):
    """tile = -1 on the 128 -> 256 layer without a residual: from M = 16384 on the dispatcher takes the weight-stationary kernel."""
    in_mode(eng, "bf16x6")
    assert eng.gemm_tile(16384, 256, 128, act=1) == G.WS and eng.gemm_tile(16383, 256, 128, act=1) != G.WS
    bad = exact_failures(eng, -1, G.problem("exact", 16384, 256, 128), want_tile=G.WS, act=1, strided=False)
    assert not bad, "\n".join(bad)
