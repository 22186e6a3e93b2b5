"""Float64 oracles, fp32 reference emulations and tolerance rules for the
big-D kernels (estep_logw_big, estep_logw_big_f32, estep_lse and
mstep_moments_big). Plain numpy on the CPU: no GPU, no extension import.

The oracles are fed the kernels' own inputs (the factor table, the data,
the offsets), so a comparison tests the kernel alone and not the Cholesky
or LU that produced a table.

Every oracle and emulation takes a `mutation`: a deliberately wrong variant
of the same computation, used by test_bigd_oracle_cpu.py to show that the
tolerances below would catch that mistake in a kernel.

  E-step   None | "no_lo" | "no_aug" | ("tile", rt, kc)
  moments  None | "no_hilo" | "no_lohi"
  lse      None | "no_last"

Tolerances. None of them is a measured kernel number; u = 2^-24.

  E-step   |logw - ref| <= 1/2 * 8 * eps_ref * q_ref + 2^-23 * |logw_ref|
           eps_ref is the largest relative error on q of the sequential fp32
           emulation against the oracle. The kernels sum in another order
           (inside the MFMA, and as row-tile partials), and eps_ref is a
           maximum over a few thousand samples: hence 8x. The second term is
           the rounding of q/2 into the much larger `add`.
  moments  |T - ref| <= 4 * eps_mom * |ref| per packed entry
           eps_mom is the largest relative error of the documented bf16x3
           algorithm, summed sequentially in fp32, against the oracle. Its
           dominant part, the dropped lo*lo product, does not depend on the
           order of the sum: hence only 4x. The data is offset so that no
           entry cancels.
  lse      see lse_tolerance.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

U = 2.0 ** -24          # fp32 unit roundoff
TILE_ROWS, TILE_COLS = 32, 16  # one MFMA tile of the factor table

# the D grids of test_gpu_bigd_oracle.py; test_bigd_oracle_cpu.py runs its
# mutant checks over exactly these
ESTEP_B16_DS = (12, 32, 33, 47, 48, 79, 80, 96, 128, 129, 142)
ESTEP_F32_DS = (32, 33, 47, 48, 79, 80, 128, 142)
MOMENTS_DS = (32, 33, 63, 64, 95, 96, 127, 128, 159)
LSE_KS = (1, 3, 5, 64)

FactorTable = namedtuple("FactorTable", "table planes mu add")


# --------------------------------------------------------------------------
# bf16 and table geometry
# --------------------------------------------------------------------------
def bf16_round(a) -> np.ndarray:
    """fp32 -> nearest-even bf16, returned as fp32 (finite inputs)."""
    bits = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    bias = ((bits >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF)
    return ((bits + bias) & np.uint32(0xFFFF0000)).view(np.float32)


def split_planes(a) -> tuple[np.ndarray, np.ndarray]:
    """hi = bf16(a), lo = bf16(a - hi), both as fp32."""
    a = np.asarray(a, dtype=np.float32)
    hi = bf16_round(a)
    return hi, bf16_round(a - hi)


def table_shape(d: int) -> tuple[int, int]:
    """(rows, cols) of the factor table, written out independently of
    functional.mfac_shape (the CPU tests hold the two against each other):
    rows pad d to 32, cols pad d + 1 to 16 and then up to a tier of 2, 3, 5
    or 9 column tiles."""
    rows = -(-d // TILE_ROWS) * TILE_ROWS
    kc = -(-(d + 1) // TILE_COLS)
    kct = next(t for t in (2, 3, 5, 9) if kc <= t)
    return rows, kct * TILE_COLS


def big2_tile(d: int) -> int:
    """Events per tile (BE) of estep_logw_big2_kernel: 256 where the table,
    the z tile and the row-tile partials fit 160 KiB of LDS, else 128."""
    rows, cols = table_shape(d)
    lds256 = (2 * rows + 256) * (cols + 8) * 2 + (rows // 32) * 256 * 4
    return 256 if lds256 <= 160 * 1024 else 128


def structure_mask(d: int) -> np.ndarray:
    """bool [rows, cols]: the cells a factor table may hold a non-zero in,
    {row < d, col <= row} and {row < d, col = d}."""
    rows, cols = table_shape(d)
    r = np.arange(rows)[:, None]
    c = np.arange(cols)[None, :]
    return (r < d) & ((c <= r) | (c == d))


def live_tiles(d: int) -> list[tuple[int, int]]:
    """(row-tile, column-tile) pairs with at least one structural cell."""
    m = structure_mask(d)
    rows, cols = m.shape
    return [(rt, kc)
            for rt in range(rows // TILE_ROWS)
            for kc in range(cols // TILE_COLS)
            if m[rt * TILE_ROWS:(rt + 1) * TILE_ROWS,
                 kc * TILE_COLS:(kc + 1) * TILE_COLS].any()]


def make_factor_table(rng, k: int, d: int) -> FactorTable:
    """A synthetic factor table [F | -F mu] in the kernels' layout.

    table  fp32 [K, rows, cols]: F dense lower-triangular with N(0,1)/sqrt(d)
           entries and a diagonal uniform in [0.5, 1.5]; column d = -F mu;
           every other cell an exact zero. Dense on purpose: every live
           32x16 tile moves q measurably.
    planes fp32 [K, 2, rows, cols] holding hi = bf16(table) and
           lo = bf16(table - hi).
    mu     fp32 [K, d], 2 * N(0,1).
    add    fp32 [K], uniform in [-600, -50]: the size of constant + ln pi
           at these D."""
    rows, cols = table_shape(d)
    f = np.tril(rng.standard_normal((k, d, d)) / np.sqrt(d))
    idx = np.arange(d)
    f[:, idx, idx] = rng.uniform(0.5, 1.5, (k, d))
    f = f.astype(np.float32)
    mu = (2.0 * rng.standard_normal((k, d))).astype(np.float32)
    table = np.zeros((k, rows, cols), dtype=np.float32)
    table[:, :d, :d] = f
    table[:, :d, d] = -np.einsum("kij,kj->ki", f.astype(np.float64),
                                 mu.astype(np.float64)).astype(np.float32)
    hi, lo = split_planes(table)
    add = rng.uniform(-600.0, -50.0, k).astype(np.float32)
    return FactorTable(table, np.stack([hi, lo], axis=1), mu, add)


def random_covariance_model(rng, k: int, d: int):
    """(means [K, d], R [K, d, d], pi [K]) of test_gpu_kernels.random_model:
    R = A A^T + d I, means 2 * N(0,1), pi Dirichlet(1)."""
    means = (rng.standard_normal((k, d)) * 2).astype(np.float32)
    rs = []
    for _ in range(k):
        a = rng.standard_normal((d, d))
        rs.append((a @ a.T + d * np.eye(d)).astype(np.float32))
    pi = rng.dirichlet(np.ones(k)).astype(np.float32)
    return means, np.stack(rs), pi


# --------------------------------------------------------------------------
# E-step: logw = add - q/2, q = sum_rows (T [z; 1])^2
# --------------------------------------------------------------------------
def _planes_of(table, mutation) -> list[np.ndarray]:
    """The table as a list of [K, rows, cols] planes with the mutation
    applied: [table] for an fp32 table, [hi, lo] for bf16 planes."""
    table = np.asarray(table)
    planes = ([table] if table.ndim == 3
              else [table[:, p] for p in range(table.shape[1])])
    if mutation is None:
        return planes
    if mutation == "no_lo":
        assert len(planes) == 2, "no_lo needs hi/lo planes"
        return planes[:1]
    if mutation == "no_aug":
        raise AssertionError("no_aug is applied to z, not to the table")
    kind, rt, kc = mutation
    assert kind == "tile"
    out = []
    for p in planes:
        p = p.copy()
        p[:, rt * TILE_ROWS:(rt + 1) * TILE_ROWS,
          kc * TILE_COLS:(kc + 1) * TILE_COLS] = 0
        out.append(p)
    return out


def _augment(z, cols: int, mutation, dtype) -> np.ndarray:
    """[z; 1; 0...] as [cols, n]; "no_aug" leaves the ones row out."""
    z = np.asarray(z)
    d, n = z.shape
    za = np.zeros((cols, n), dtype=dtype)
    za[:d] = z
    if mutation != "no_aug":
        za[d] = 1
    return za


def logw_oracle(table, z, add, mutation=None):
    """(logw, q) in float64, [K, n] each.

    bf16 kernel: `table` is the hi/lo planes [K, 2, rows, cols] (their
    float64 sum is the table) and z the bf16-rounded data. fp32 kernel:
    `table` is the fp32 table [K, rows, cols] and z the data."""
    tab_mut = None if mutation == "no_aug" else mutation
    t64 = sum(p.astype(np.float64) for p in _planes_of(table, tab_mut))
    za = _augment(z, t64.shape[2], mutation, np.float64)
    y = t64 @ za                                        # [K, rows, n]
    q = np.einsum("krn,krn->kn", y, y)
    logw = np.asarray(add, dtype=np.float64)[:, None] - 0.5 * q
    return logw, q


def logw_emulation_f32(table, z, add, mutation=None):
    """(logw, q) of the same sum in sequential fp32: per row the products
    are added k ascending, hi before lo; the squares rows ascending; then
    fl(add - q/2). A reference with fp32's error, not the kernel: the
    kernels sum in the MFMA's order and as row-tile partials."""
    tab_mut = None if mutation == "no_aug" else mutation
    planes = [np.asarray(p, dtype=np.float32)
              for p in _planes_of(table, tab_mut)]
    k, rows, cols = planes[0].shape
    za = _augment(z, cols, mutation, np.float32)
    y = np.zeros((k, rows, za.shape[1]), dtype=np.float32)
    for kk in range(cols):
        if not any(p[:, :, kk].any() for p in planes):
            continue  # an all-zero column adds an exact zero
        for p in planes:
            y = y + p[:, :, kk, None] * za[kk][None, None, :]
    q = np.zeros((k, za.shape[1]), dtype=np.float32)
    for r in range(rows):
        q = q + y[:, r] * y[:, r]
    logw = np.asarray(add, dtype=np.float32)[:, None] - np.float32(0.5) * q
    return logw, q


def eps_ref(table, z, add) -> float:
    """Largest relative error on q of the fp32 emulation against the
    oracle, over all clusters and events."""
    _, q64 = logw_oracle(table, z, add)
    _, q32 = logw_emulation_f32(table, z, add)
    return float(np.max(np.abs(q32.astype(np.float64) - q64) / q64))


def logw_tolerance(eps: float, q_ref, logw_ref) -> np.ndarray:
    """1/2 * 8 * eps * q_ref + 2^-23 * |logw_ref| (module docstring)."""
    return 0.5 * 8.0 * eps * np.asarray(q_ref) + 2.0 ** -23 * np.abs(logw_ref)


# --------------------------------------------------------------------------
# moments: T_c = sum_e w_ce [x; 1][x; 1]^T, packed lower triangle
# --------------------------------------------------------------------------
def _pack(t: np.ndarray) -> np.ndarray:
    """[K, dp, dp] -> [K, dp(dp+1)/2], entry (i, j <= i) at i(i+1)/2 + j:
    the layout functional.moments_views reads."""
    ii, jj = np.tril_indices(t.shape[1])
    return np.ascontiguousarray(t[:, ii, jj])


def _augment_x(x, dtype) -> np.ndarray:
    x = np.asarray(x)
    return np.concatenate([x.astype(dtype),
                           np.ones((1, x.shape[1]), dtype=dtype)], axis=0)


def _b16x3_terms(x, w):
    """The operands of the documented bf16x3 algorithm, all fp32:
    z = hi + lo of [x; 1] [dp, n]; a = fl(w * z) [K, dp, n] split into
    a_hi, a_lo; b_hi, b_lo the planes of z."""
    b_hi, b_lo = split_planes(_augment_x(x, np.float32))
    z = b_hi + b_lo
    a = np.asarray(w, dtype=np.float32)[:, None, :] * z[None, :, :]
    a_hi, a_lo = split_planes(a)
    return a_hi, a_lo, b_hi, b_lo


def moments_oracle(x, w, mutation=None) -> np.ndarray:
    """float64 packed [K, pp]. With a mutation: the float64 sum of the
    bf16x3 products with that one product left out (the mutant kernel,
    free of summation error)."""
    if mutation is None:
        xa = _augment_x(x, np.float64)
        t = np.einsum("kn,in,jn->kij", np.asarray(w, dtype=np.float64),
                      xa, xa, optimize=True)
        return _pack(t)
    a_hi, a_lo, b_hi, b_lo = (v.astype(np.float64)
                              for v in _b16x3_terms(x, w))
    t = np.einsum("kin,jn->kij", a_hi, b_hi, optimize=True)
    if mutation != "no_hilo":
        t += np.einsum("kin,jn->kij", a_hi, b_lo, optimize=True)
    if mutation != "no_lohi":
        t += np.einsum("kin,jn->kij", a_lo, b_hi, optimize=True)
    assert mutation in ("no_hilo", "no_lohi")
    return _pack(t)


def moments_emulation_b16x3(x, w, mutation=None) -> np.ndarray:
    """fp32 packed [K, pp] of the documented algorithm: per event, in event
    order, acc += a_hi*b_hi, acc += a_hi*b_lo, acc += a_lo*b_hi (products of
    two bf16 values are exact in fp32; every add rounds)."""
    assert mutation in (None, "no_hilo", "no_lohi")
    a_hi, a_lo, b_hi, b_lo = _b16x3_terms(x, w)
    k, dp, n = a_hi.shape
    acc = np.zeros((k, dp, dp), dtype=np.float32)
    for e in range(n):
        ah = a_hi[:, :, e, None]
        acc = acc + ah * b_hi[None, None, :, e]
        if mutation != "no_hilo":
            acc = acc + ah * b_lo[None, None, :, e]
        if mutation != "no_lohi":
            acc = acc + a_lo[:, :, e, None] * b_hi[None, None, :, e]
    return _pack(acc)


def eps_mom(x, w) -> float:
    """Largest relative error of the fp32 bf16x3 emulation against the
    oracle over all packed entries of these inputs."""
    ref = moments_oracle(x, w)
    emu = moments_emulation_b16x3(x, w).astype(np.float64)
    return float(np.max(np.abs(emu - ref) / np.abs(ref)))


def moments_tolerance(eps: float, ref) -> np.ndarray:
    """4 * eps * |ref| per packed entry (module docstring)."""
    return 4.0 * eps * np.abs(ref)


def moments_inputs(rng, d: int, k: int, n: int):
    """x = 2 N(0,1) + 3 [d, n], w ~ U(0,1) [K, n]: offset data, so that no
    entry of T is a cancelling sum."""
    x = (2.0 * rng.standard_normal((d, n)) + 3.0).astype(np.float32)
    w = rng.uniform(0.0, 1.0, (k, n)).astype(np.float32)
    return x, w


# --------------------------------------------------------------------------
# lse
# --------------------------------------------------------------------------
def lse_oracle(logw, mutation=None) -> np.ndarray:
    """float64 log-sum-exp over clusters, [n]; "no_last" leaves the last
    cluster out (-inf for K = 1)."""
    l64 = np.asarray(logw, dtype=np.float64)
    if mutation == "no_last":
        l64 = l64[:-1]
        if l64.shape[0] == 0:
            return np.full(l64.shape[1], -np.inf)
    else:
        assert mutation is None
    m = l64.max(axis=0)
    return m + np.log(np.exp(l64 - m[None, :]).sum(axis=0))


def lse_tolerance(logw, ref) -> np.ndarray:
    """u * (|m| + |ref|) + (3K + 4) * u with u = 2^-24, m = max_c logw.

    The kernel computes m exactly, t_c = fl(l_c - m) <= 0,
    s = sum_c __expf(t_c) in cluster order, lse = fl(m + __logf(s)).

    * The two roundings around m are the first term: fl(m + ln s) is off by
      at most u * |ref|, and fl(l_c - m), a difference of two values of
      size |m|, is granted u * |m| (it is exact when the two lie within a
      factor of two of each other, and otherwise moves its term by no more
      than |t| e^-|t| u <= 0.37 u).
    * __expf(t) is exp2(t * log2 e): the scaled argument carries a relative
      error of about u, which moves the result by |t| log2(e) e^-|t| u
      <= 0.53 u, and exp2 itself is good to one ulp of a value <= 1: every
      term is off by less than 2 u. The K - 1 additions add at most
      (K - 1) u * s. Since the largest term is e^0 = 1, s >= 1, and the
      error of ln s from the terms and the sum is at most
      2 K u / s + (K - 1) u <= 3 K u.
    * __logf(s) is log2(s) * ln 2: one ulp of the logarithm and half an ulp
      of the product, 1.5 ulp(ln s). For ln s < 2 that is at most 3 u, the
      "+ 4". For ln s >= 2, s >= 7.4 and the term errors shrink to
      2 K u / s <= 0.27 K u, while 1.5 ulp(ln s) <= 3 u ln K; the total
      1.27 K u + 3 u ln K stays below (3 K + 4) u for every K."""
    l64 = np.asarray(logw, dtype=np.float64)
    k = l64.shape[0]
    m = l64.max(axis=0)
    return U * (np.abs(m) + np.abs(ref)) + (3 * k + 4) * U


def lse_inputs(rng, k: int, n: int) -> np.ndarray:
    """fp32 logw [K, n]: clusters within +-3 of each other (each entry
    uniform in [-1.5, 1.5]) plus a per-event offset uniform in [-2000, 50].
    Without the max subtraction the sum underflows at most events, and a
    left-out cluster moves lse by about 1/K."""
    spread = rng.uniform(-1.5, 1.5, (k, n))
    offset = rng.uniform(-2000.0, 50.0, n)
    return (spread + offset[None, :]).astype(np.float32)


# --------------------------------------------------------------------------
# The cases of test_gpu_bigd_oracle.py, shared with test_bigd_oracle_cpu.py
# so that the CPU file checks the very inputs the GPU file runs. (d, k, n).
# --------------------------------------------------------------------------
def _be(d: int) -> int:
    return big2_tile(d)


# K = 5, two full tiles and a ragged third
ESTEP_B16_GRID = [(d, 5, 2 * _be(d) + 37) for d in ESTEP_B16_DS]
# n around one tile, and a single cluster
ESTEP_B16_EDGES = ([(d, 5, n) for d in (48, 142)
                    for n in (1, _be(d) - 1, _be(d), _be(d) + 1)]
                   + [(80, 1, 2 * _be(80) + 37)])
# four tiles, walked by 1, 2 or 4 blocks per cluster (GMM_BIG2_NCHUNK)
ESTEP_B16_MULTI = [(d, 5, 3 * _be(d) + 5) for d in (33, 80, 142)]
# K = 6: the second grid.y block of the fp32 kernel has two idle waves
ESTEP_F32_CASES = [(32, 5, 300), (33, 6, 129), (47, 1, 127), (48, 5, 128),
                   (48, 6, 1), (79, 6, 300), (80, 5, 1), (80, 1, 129),
                   (128, 6, 129), (128, 5, 127), (142, 5, 300),
                   (142, 1, 128)]
# every D once with an odd n and once with an odd K
MOMENTS_CASES = [(32, 1, 1), (32, 5, 65), (33, 2, 63), (33, 5, 129),
                 (63, 5, 64), (63, 1, 129), (64, 2, 65), (64, 5, 200),
                 (95, 1, 63), (95, 2, 200), (96, 5, 129), (96, 2, 64),
                 (127, 1, 65), (127, 2, 200), (128, 5, 1), (128, 2, 129),
                 (159, 5, 63), (159, 1, 200)]
# six 64-event tiles, the last ragged
MOMENTS_PIPE = [(d, 5, 64 * 5 + 9) for d in (33, 96, 159)]
LSE_CASES = [(k, n) for k in LSE_KS for n in (1, 255, 256, 257, 1100)]


def estep_canonical(kind: str, d: int) -> tuple[int, int, int]:
    """The case eps_ref(d) is taken from: K = 5 and enough events that the
    maximum runs over more than a thousand samples."""
    return (d, 5, 2 * _be(d) + 37) if kind == "b16" else (d, 5, 300)


@functools.lru_cache(maxsize=None)
def estep_case(kind: str, d: int, k: int, n: int) -> dict:
    """Seeded inputs and float64 reference of one E-step case, built once
    and shared read-only. kind "b16": table = hi/lo planes, z bf16-rounded;
    "f32": table = the fp32 table, z fp32."""
    assert kind in ("b16", "f32")
    rng = np.random.default_rng([int(kind == "f32"), d, k, n])
    ft = make_factor_table(rng, k, d)
    z = rng.standard_normal((d, n)).astype(np.float32)
    if kind == "b16":
        z = bf16_round(z)
    table = ft.planes if kind == "b16" else ft.table
    logw, q = logw_oracle(table, z, ft.add)
    return {"table": table, "z": z, "add": ft.add, "logw": logw, "q": q}


@functools.lru_cache(maxsize=None)
def estep_eps(kind: str, d: int) -> float:
    """eps_ref(d): the emulation's error on the canonical case of this D.
    Cases with few events (n = 1) use it too: a maximum over five samples
    would say little about the format."""
    c = estep_case(kind, *estep_canonical(kind, d))
    return eps_ref(c["table"], c["z"], c["add"])


@functools.lru_cache(maxsize=None)
def moments_case(d: int, k: int, n: int) -> dict:
    """Seeded inputs, float64 reference and eps_mom of one moments case."""
    rng = np.random.default_rng([2, d, k, n])
    x, w = moments_inputs(rng, d, k, n)
    return {"x": x, "w": w, "ref": moments_oracle(x, w),
            "eps": eps_mom(x, w)}


@functools.lru_cache(maxsize=None)
def lse_case(k: int, n: int) -> dict:
    rng = np.random.default_rng([3, k, n])
    logw = lse_inputs(rng, k, n)
    return {"logw": logw, "ref": lse_oracle(logw)}
