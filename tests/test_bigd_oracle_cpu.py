"""The oracles of bigd_oracle.py held against themselves on the CPU, so that
test_gpu_bigd_oracle.py cannot hide a failure: the table generator builds
what the kernels expect, the fp32 emulations meet the tolerances, and every
mutant (a plausible kernel mistake) misses them at the very inputs the GPU
file runs."""
import numpy as np
import pytest

import bigd_oracle as bo
from cuda_gmm_mpi_amd.ops import functional as F

ESTEP_KINDS_DS = ([("b16", d) for d in bo.ESTEP_B16_DS]
                  + [("f32", d) for d in bo.ESTEP_F32_DS])
MOMENTS_ALL = bo.MOMENTS_CASES + bo.MOMENTS_PIPE


@pytest.mark.parametrize("d", [12, 31, 32, 47, 48, 79, 80, 142])
def test_table_matches_mfac_shape(d):
    """Shape and column tier equal functional.mfac_shape; the content is
    [F | -F mu] inside the structural mask and exact zeros outside."""
    planes_n, rows, cols = F.mfac_shape(d)
    assert bo.table_shape(d) == (rows, cols)
    tier = {12: 2, 31: 2, 32: 3, 47: 3, 48: 5, 79: 5, 80: 9, 142: 9}[d]
    assert cols == 16 * tier and rows == 32 * ((d + 31) // 32)
    k = 3
    ft = bo.make_factor_table(np.random.default_rng(d), k, d)
    assert ft.table.shape == (k, rows, cols)
    assert ft.table.dtype == np.float32
    assert ft.planes.shape == (k, planes_n, rows, cols)
    mask = bo.structure_mask(d)
    assert not ft.table[:, ~mask].any() and not ft.planes[:, :, ~mask].any()
    assert (ft.table[:, mask] != 0).all()  # dense: no live cell is idle
    diag = ft.table[:, np.arange(d), np.arange(d)]
    assert (diag >= 0.5).all() and (diag <= 1.5).all()
    f64 = ft.table[:, :d, :d].astype(np.float64)
    aug = -np.einsum("kij,kj->ki", f64, ft.mu.astype(np.float64))
    np.testing.assert_allclose(ft.table[:, :d, d], aug, rtol=1e-6, atol=1e-6)
    # hi and lo are bf16 values and hi + lo is the table to 2^-16
    assert np.array_equal(bo.bf16_round(ft.planes), ft.planes)
    np.testing.assert_allclose(ft.planes.sum(axis=1), ft.table,
                               rtol=2.0 ** -15, atol=0)
    assert (ft.add >= -600).all() and (ft.add <= -50).all()


def test_bf16_round_matches_torch():
    import torch
    a = np.random.default_rng(0).standard_normal(4096).astype(np.float32)
    a[:4] = [0.0, -0.0, 1.00390625, 1.01171875]  # ties, both directions
    want = torch.from_numpy(a).to(torch.bfloat16).float().numpy()
    assert np.array_equal(bo.bf16_round(a), want)


def test_big2_tile_and_live_tiles():
    """BE = 256 up to D = 128, 128 beyond; the live tiles are those the
    kernel's skip rule keeps (kc <= 2 rt + 1, or the augmented tile) that
    hold a structural cell."""
    assert [bo.big2_tile(d) for d in (12, 80, 128, 129, 142)] == \
        [256, 256, 256, 128, 128]
    for d in bo.ESTEP_B16_DS:
        rows, cols = bo.table_shape(d)
        kept = {(rt, kc) for rt in range(rows // 32)
                for kc in range(cols // 16)
                if kc <= 2 * rt + 1 or kc == d >> 4}
        assert set(bo.live_tiles(d)) <= kept
    assert bo.live_tiles(12) == [(0, 0)]
    assert len(bo.live_tiles(142)) == 2 + 4 + 6 + 8 + 9 + 4


def test_gpu_grid_is_complete():
    """The shared case lists cover the whole grid: nothing is left out."""
    assert {c[0] for c in bo.ESTEP_B16_GRID} == set(bo.ESTEP_B16_DS)
    assert len(bo.ESTEP_B16_GRID) == len(bo.ESTEP_B16_DS) == 11
    assert all(k == 5 and n == 2 * bo.big2_tile(d) + 37
               for d, k, n in bo.ESTEP_B16_GRID)
    assert {(d, n) for d, _, n in bo.ESTEP_B16_EDGES if d != 80} == \
        {(48, 1), (48, 255), (48, 256), (48, 257),
         (142, 1), (142, 127), (142, 128), (142, 129)}
    assert (80, 1) in {(d, k) for d, k, _ in bo.ESTEP_B16_EDGES}
    assert {c[0] for c in bo.ESTEP_B16_MULTI} == {33, 80, 142}
    assert {c[0] for c in bo.ESTEP_F32_CASES} == set(bo.ESTEP_F32_DS)
    assert {c[1] for c in bo.ESTEP_F32_CASES} == {1, 5, 6}
    assert {c[2] for c in bo.ESTEP_F32_CASES} == {1, 127, 128, 129, 300}
    assert {c[0] for c in bo.MOMENTS_CASES} == set(bo.MOMENTS_DS)
    assert {c[1] for c in bo.MOMENTS_CASES} == {1, 2, 5}
    assert {c[2] for c in bo.MOMENTS_CASES} == {1, 63, 64, 65, 129, 200}
    for d in bo.MOMENTS_DS:
        mine = [c for c in bo.MOMENTS_CASES if c[0] == d]
        assert any(n % 2 for _, _, n in mine), d
        assert any(k % 2 for _, k, _ in mine), d
    assert bo.MOMENTS_PIPE == [(33, 5, 329), (96, 5, 329), (159, 5, 329)]
    assert len(bo.LSE_CASES) == 20


# ------------------------------------------------------------------ E-step
@pytest.mark.parametrize("kind,d", ESTEP_KINDS_DS)
def test_estep_emulation_within_tolerance(kind, d):
    c = bo.estep_case(kind, *bo.estep_canonical(kind, d))
    eps = bo.estep_eps(kind, d)
    # fp32 sums of a few hundred terms: a few 1e-7, as NUMERICS.md lists
    assert 1e-7 < eps < 1e-6, eps
    logw, _ = bo.logw_emulation_f32(c["table"], c["z"], c["add"])
    err = np.abs(logw.astype(np.float64) - c["logw"])
    tol = bo.logw_tolerance(eps, c["q"], c["logw"])
    assert (err <= tol).all(), float((err / tol).max())


def _exceeding(kind, d, mutation):
    """Share of (cluster, event) samples where the mutant oracle misses
    the tolerance, and the median of error / tolerance."""
    c = bo.estep_case(kind, *bo.estep_canonical(kind, d))
    tol = bo.logw_tolerance(bo.estep_eps(kind, d), c["q"], c["logw"])
    mut, _ = bo.logw_oracle(c["table"], c["z"], c["add"], mutation)
    ratio = np.abs(mut - c["logw"]) / tol
    return float((ratio > 1).mean()), float(np.median(ratio))


@pytest.mark.parametrize("kind,d", ESTEP_KINDS_DS)
def test_estep_mutants_exceed_tolerance(kind, d):
    """Dropped lo plane, ignored augmented column and every single zeroed
    live tile: each misses the tolerance on at least half of the samples."""
    mutants = [("tile", rt, kc) for rt, kc in bo.live_tiles(d)] + ["no_aug"]
    if kind == "b16":
        mutants.append("no_lo")
    worst = None
    for m in mutants:
        share, med = _exceeding(kind, d, m)
        assert share >= 0.5, (m, share, med)
        if worst is None or med < worst[1]:
            worst = (m, med)
    print(f"{kind} D={d}: {len(mutants)} mutants, least visible {worst[0]} "
          f"at a median of {worst[1]:.0f}x the tolerance")


def test_estep_mutation_of_emulation_agrees():
    """The emulation takes the same mutations as the oracle."""
    c = bo.estep_case("b16", 33, 5, 2 * 256 + 37)
    eps = bo.estep_eps("b16", 33)
    for m in ("no_lo", "no_aug", ("tile", 1, 2)):
        ref, q = bo.logw_oracle(c["table"], c["z"], c["add"], m)
        emu, _ = bo.logw_emulation_f32(c["table"], c["z"], c["add"], m)
        tol = bo.logw_tolerance(eps, q, ref)
        assert (np.abs(emu.astype(np.float64) - ref) <= tol).all(), m


# ----------------------------------------------------------------- moments
@pytest.mark.parametrize("d,k,n", MOMENTS_ALL)
def test_moments_emulation_and_mutants(d, k, n):
    """The bf16x3 emulation meets 4 eps_mom |ref| (by construction of
    eps_mom, with room), the packed layout is what moments_views reads,
    and dropping either cross product misses the tolerance on at least
    half of the entries."""
    import torch
    c = bo.moments_case(d, k, n)
    ref, eps = c["ref"], c["eps"]
    assert ref.shape == (k, (d + 1) * (d + 2) // 2)
    # worst case of the four 2^-16-sized terms (both z splits, the a
    # split, the dropped lo*lo) is 4 * 2^-16; sums average below that
    assert 1e-6 < eps < 4 * 2.0 ** -16, eps
    n_c, mean_num, s = F.moments_views(torch.from_numpy(ref), d)
    x64, w64 = c["x"].astype(np.float64), c["w"].astype(np.float64)
    np.testing.assert_allclose(n_c.numpy(), w64.sum(axis=1), rtol=1e-12)
    np.testing.assert_allclose(mean_num.numpy(), w64 @ x64.T, rtol=1e-12)
    np.testing.assert_allclose(
        s.numpy(), np.einsum("kn,in,jn->kij", w64, x64, x64), rtol=1e-12)
    tol = bo.moments_tolerance(eps, ref)
    assert (tol > 0).all()  # offset data: no entry cancels to nothing
    for m in ("no_hilo", "no_lohi"):
        ratio = np.abs(bo.moments_oracle(c["x"], c["w"], m) - ref) / tol
        share = float((ratio > 1).mean())
        print(f"D={d} K={k} n={n} {m}: {share:.0%} of entries exceed, "
              f"median {np.median(ratio):.1f}x")
        assert share >= 0.5, (m, share)
        emu = bo.moments_emulation_b16x3(c["x"], c["w"], m)
        assert float((np.abs(emu - ref) > tol).mean()) >= 0.5, m


# --------------------------------------------------------------------- lse
@pytest.mark.parametrize("k,n", bo.LSE_CASES)
def test_lse_inputs_and_mutant(k, n):
    c = bo.lse_case(k, n)
    logw, ref = c["logw"], c["ref"]
    assert logw.dtype == np.float32 and logw.shape == (k, n)
    assert float((logw.max(axis=0) - logw.min(axis=0)).max()) <= 3.001
    import torch
    np.testing.assert_allclose(
        ref, torch.logsumexp(torch.from_numpy(logw).double(), 0).numpy(),
        rtol=1e-13)
    tol = bo.lse_tolerance(logw, ref)
    mut = bo.lse_oracle(logw, "no_last")
    assert (np.abs(mut - ref) > tol).all()
    if n == 1100:
        # without the max subtraction the fp32 sum underflows
        naive = np.exp(logw).sum(axis=0)
        assert float((naive == 0).mean()) > 0.9
