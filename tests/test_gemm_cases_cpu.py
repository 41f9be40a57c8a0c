"""CPU: the premise of the zero tolerance of tests/test_gpu_gemm_tiles.py -- for every `exact` / `onehot` case the plain float32
torch reference IS the float64 one -- and the properties of the shape grids the GPU tests rely on."""
import pytest
import torch

import gemm_cases as G

EPILOGUES = [(0, False), (1, True), (3, True)]


def all_exact_shapes():
    shapes = set()
    for mode in G.MODES:
        for tile in G.tiles_of(mode) + ((G.WS,) if mode == "bf16x6" else ()):
            shapes.update((M, N, K, 1, True) for M, N, K in G.shape_grid(tile, mode))
            if tile == G.WS:
                continue
            BM, BN = G.tile_dims(tile, mode)
            for K in (128, 160, 256, 544):                                   # test_tile_concat
                shapes.add((2 * BM + 1, G.n_unit(tile, mode), K, 1, True))
            for groups in (1, 2, 4):                                         # test_tile_groups
                for shared in (True, False):
                    for M, K in ((BM + 1, 160), (2 * BM + 1, 544), (2 * BM + 1, 96)):
                        shapes.add((M, G.n_unit(tile, mode), K, groups, shared))
    for N in (128, 192, 256, 384, 512):                                      # test_launcher_fallbacks
        shapes.add((129, N, 160, 1, True))
    return sorted(shapes)


def test_exact_cases_are_exact_in_float32():
    bad = []
    for M, N, K, groups, shared in all_exact_shapes():
        for family in ("exact", "onehot"):
            p = G.problem(family, M, N, K, groups, shared)
            assert p["A"].abs().max() <= 2 and p["W"].abs().max() <= 2 and bool((p["A"] * 4 == (p["A"] * 4).round()).all())
            for act, res in EPILOGUES:
                if not G.exact_is_exact(p, act, res):
                    bad.append((family, M, N, K, groups, act, res))
    assert not bad, bad


def test_dispatchers_own_choice_cases_are_exact():
    import test_gpu_gemm_tiles as T
    for mode, M, N, K, want in T.OWN_CHOICE + [("bf16x6", 16384, 256, 128, G.WS)]:
        assert G.exact_is_exact(G.problem("exact", M, N, K), 1, True), (M, N, K)


def test_exact_values_depend_on_row_and_column():
    a = G.problem("exact", 257, 128, 160)["A"][0]
    assert len(torch.unique(a)) == 17                                          # every integer in [-8, 8] times 2^-2
    assert len(torch.unique(a, dim=0)) == 257 and len(torch.unique(a.t().contiguous(), dim=0)) == 160   # no two rows / columns equal
    kt = a.view(257, 5, 32).transpose(0, 1).reshape(5, -1)
    assert len(torch.unique(kt, dim=0)) == 5                                   # no two K tiles equal


@pytest.mark.parametrize("mode", G.MODES)
def test_shape_grids_cover_the_tile_edges(mode):
    for tile in G.tiles_of(mode):
        BM, BN = G.tile_dims(tile, mode)
        grid = G.shape_grid(tile, mode)
        ms, ns, ks = {s[0] for s in grid}, {s[1] for s in grid}, {s[2] for s in grid}
        assert {1, BM - 1, BM, BM + 1, 2 * BM + 1} <= ms | {0}, tile
        assert ks == set(G.K_GRID_SMALL if tile == "32x32k4" else G.K_GRID), tile
        bn = G.n_unit(tile, mode)
        assert {bn, 2 * bn, 3 * bn} <= ns and all(n % bn == 0 for n in ns), tile
        counts = {-(-M // BM) * (N // BN) for M, N, K in grid}
        # fewer tiles than XCDs, one per XCD, one per XCD with a remainder, more than two per XCD with a remainder (tiles whose legal N
        # are multiples of twice their width only reach even counts: 10 then stands for 9, 18 for 17)
        assert 8 in counts and any(c < 8 for c in counts) and any(8 < c < 16 for c in counts) and any(c > 16 and c % 8 for c in counts), \
            (tile, sorted(counts))
        if tile == "32x32k4":      # every variant of the K-split kernel: 4 waves (K < 256), 8 waves, 4 waves with one staging buffer
            assert any(K < 256 for M, N, K in grid) and any(K >= 256 and G.small_blocks(M, N) <= 256 for M, N, K in grid)
            assert any(K >= 256 and 256 < G.small_blocks(M, N) <= 512 for M, N, K in grid)
        assert all(M <= G.M_CAP and N <= G.N_CAP and K <= G.K_CAP for M, N, K in grid)
