// MI355X (gfx950 / CDNA4) kernels for the GMM EM engine.
//
// Brand-new HIP implementations of the reference's kernel set
// (gaussian_kernel.cu — estep1/estep2/mstep_covariance1/constants_kernel),
// redesigned for CDNA4: 64-wide wavefronts, 256-thread workgroups, dynamic
// LDS (no NUM_DIMENSIONS=32 static cap — the reference silently corrupts
// for D > 32), packed-symmetric quadratic forms (half the FLOPs and LDS of
// the reference's full D^2 loop), grids >> 256 workgroups to fill 8 XCDs,
// and deterministic chunked reductions (no float atomics).
//
// Layouts (match the engine):
//   x     : [D, N] dimension-major (fp32 or bf16)
//   logw/w: [K, N] cluster-major
//   rinv packed: lower triangle, off-diagonal entries pre-summed with their
//                transpose so  q = sum_{i>j} p_ij dx_i dx_j + sum_i p_ii dx_i^2
//                == the reference's full double loop (gaussian_kernel.cu:435-439)
#include "gmm_common.h"

namespace gmm {

// map linear lower-triangle index t -> (row i, col j), j <= i
__device__ inline void tri_row_col(int t, int* i, int* j) {
  int r = (int)((sqrtf(8.0f * t + 1.0f) - 1.0f) * 0.5f);
  while ((r + 1) * (r + 2) / 2 <= t) ++r;
  while (r * (r + 1) / 2 > t) --r;
  *i = r;
  *j = t - r * (r + 1) / 2;
}

// k index held by lane group (l>>4) element u for mfma_f32_16x16x32_bf16
// A/B fragments. Verified on hardware by the mfma_probe test
// (tests/test_gpu_kernels.py::test_mfma_bf16_probe); flip to the split-K
// variant (4*(l>>4) + u%4 + 16*(u/4)) if the probe ever disagrees.
__device__ inline int mfma_b16_k(int group, int u) { return 8 * group + u; }

// k-chunk count rounded to the estep-big template tiers (D <= 143); the
// factor storage is allocated at the tier width with zero-filled padding
// so templated kernels can unroll a fixed chunk count.
__host__ __device__ inline int kc_tier(int kc) {
  return kc <= 2 ? 2 : kc == 3 ? 3 : kc <= 5 ? 5 : 9;
}

// Factor table shape per cluster and plane: mfac_rows(d) rows (RT row-tiles
// of 32) by mfac_kct(d) * 16 k-slots (the d + 1 augmented columns in 16-deep
// MFMA k-chunks, at the tier width).
__host__ __device__ inline int mfac_rows(int d) { return ((d + 31) / 32) * 32; }
__host__ __device__ inline int mfac_kct(int d) {
  return kc_tier((d + 1 + 15) / 16);
}

// Stage cluster c's means + packed/pre-symmetrized Rinv into LDS.
// lds layout: [0, d) means, [d, d + d(d+1)/2) packed rinv.
__device__ inline void stage_cluster_params(
    const float* __restrict__ means, const float* __restrict__ rinv,
    int c, int d, float* lds_means, float* lds_rp) {
  const int p = d * (d + 1) / 2;
  for (int t = threadIdx.x; t < d; t += NT) lds_means[t] = means[c * d + t];
  const float* rc = rinv + (int64_t)c * d * d;
  for (int t = threadIdx.x; t < p; t += NT) {
    int i, j;
    tri_row_col(t, &i, &j);
    lds_rp[t] = (i == j) ? rc[i * d + i] : (rc[i * d + j] + rc[j * d + i]);
  }
}

// ---------------------------------------------------------------------------
// E-step 1: log weighted likelihoods (replaces estep1, gaussian_kernel.cu:383)
//   logw[c, e] = -0.5 * (x_e - mu_c)^T Rinv_c (x_e - mu_c) + constant_c + ln pi_c
//
// Variant A (D <= DMAX <= 32): per-event dx cached in registers, fully
// unrolled triangle — VALU-bound, coalesced single pass over x.
// ---------------------------------------------------------------------------
template <int DMAX, typename T>
__global__ void __launch_bounds__(NT)
estep_logw_reg_kernel(const T* __restrict__ x, const float* __restrict__ means,
                      const float* __restrict__ rinv,
                      const float* __restrict__ constant,
                      const float* __restrict__ logpi,
                      float* __restrict__ logw, int d, int64_t n) {
  extern __shared__ float lds[];
  float* lds_means = lds;
  float* lds_rp = lds + d;
  const int c = blockIdx.y;
  stage_cluster_params(means, rinv, c, d, lds_means, lds_rp);
  __syncthreads();
  const float add = constant[c] + logpi[c];

  for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n;
       e += (int64_t)gridDim.x * NT) {
    float dx[DMAX];
#pragma unroll
    for (int i = 0; i < DMAX; ++i)
      dx[i] = (i < d) ? (load_x(x, (int64_t)i * n + e) - lds_means[i]) : 0.0f;
    float q = 0.0f;
    int t = 0;
#pragma unroll
    for (int i = 0; i < DMAX; ++i) {
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        // guard keeps padded lanes out of the LDS array without branching
        // on anything runtime-divergent (i,j,d are wave-uniform)
        if (i < d) q = fmaf(lds_rp[t] * dx[i], dx[j], q);
        ++t;
      }
    }
    logw[(int64_t)c * n + e] = -0.5f * q + add;
  }
}

// Variant B (any D): dx_j re-read from global (L1/L2-resident column tile).
template <typename T>
__global__ void __launch_bounds__(NT)
estep_logw_gen_kernel(const T* __restrict__ x, const float* __restrict__ means,
                      const float* __restrict__ rinv,
                      const float* __restrict__ constant,
                      const float* __restrict__ logpi,
                      float* __restrict__ logw, int d, int64_t n) {
  extern __shared__ float lds[];
  float* lds_means = lds;
  float* lds_rp = lds + d;
  const int c = blockIdx.y;
  stage_cluster_params(means, rinv, c, d, lds_means, lds_rp);
  __syncthreads();
  const float add = constant[c] + logpi[c];

  for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n;
       e += (int64_t)gridDim.x * NT) {
    float q = 0.0f;
    int t = 0;
    for (int i = 0; i < d; ++i) {
      const float dxi = load_x(x, (int64_t)i * n + e) - lds_means[i];
      float qi = 0.0f;
#pragma unroll 4
      for (int j = 0; j < i; ++j) {
        const float dxj = load_x(x, (int64_t)j * n + e) - lds_means[j];
        qi = fmaf(lds_rp[t + j], dxj, qi);  // pre-summed (R_ij + R_ji)
      }
      qi = fmaf(lds_rp[t + i], dxi, qi);    // diagonal term
      q = fmaf(qi, dxi, q);
      t += i + 1;
    }
    logw[(int64_t)c * n + e] = -0.5f * q + add;
  }
}

// Diagonal-only variant (DIAG_ONLY, gaussian_kernel.cu:430-433).
template <typename T>
__global__ void __launch_bounds__(NT)
estep_logw_diag_kernel(const T* __restrict__ x, const float* __restrict__ means,
                       const float* __restrict__ rinv,
                       const float* __restrict__ constant,
                       const float* __restrict__ logpi,
                       float* __restrict__ logw, int d, int64_t n) {
  extern __shared__ float lds[];
  float* lds_means = lds;
  float* lds_rd = lds + d;
  const int c = blockIdx.y;
  for (int t = threadIdx.x; t < d; t += NT) {
    lds_means[t] = means[(int64_t)c * d + t];
    lds_rd[t] = rinv[((int64_t)c * d + t) * d + t];
  }
  __syncthreads();
  const float add = constant[c] + logpi[c];
  for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n;
       e += (int64_t)gridDim.x * NT) {
    float q = 0.0f;
#pragma unroll 4
    for (int i = 0; i < d; ++i) {
      const float dx = load_x(x, (int64_t)i * n + e) - lds_means[i];
      q = fmaf(dx * dx, lds_rd[i], q);
    }
    logw[(int64_t)c * n + e] = -0.5f * q + add;
  }
}

// ---------------------------------------------------------------------------
// E-step 2: posteriors + likelihood (replaces estep2, gaussian_kernel.cu:446)
// In-place on logw: per event max over K, log-sum-exp, normalize; per-block
// partial sum of log P(x) written to partial[blockIdx.x] (deterministic
// torch.sum on the host side of the stream — no float atomics).
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(NT)
estep_posteriors_kernel(float* __restrict__ logw, float* __restrict__ partial,
                        int k, int64_t n) {
  float acc = 0.0f;
  for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n;
       e += (int64_t)gridDim.x * NT) {
    float m = logw[e];
#pragma unroll 4
    for (int c = 1; c < k; ++c) m = fmaxf(m, logw[(int64_t)c * n + e]);
    float s = 0.0f;
#pragma unroll 4
    for (int c = 0; c < k; ++c) s += __expf(logw[(int64_t)c * n + e] - m);
    const float denom = m + __logf(s);
#pragma unroll 4
    for (int c = 0; c < k; ++c) {
      const int64_t idx = (int64_t)c * n + e;
      logw[idx] = __expf(logw[idx] - denom);
    }
    acc += denom;
  }
  // wave reduction then LDS across the 4 waves
  __shared__ float wsum[NT / WAVE];
  for (int off = WAVE / 2; off > 0; off >>= 1)
    acc += __shfl_down(acc, off, WAVE);
  const int wid = threadIdx.x / WAVE;
  if ((threadIdx.x & (WAVE - 1)) == 0) wsum[wid] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float total = 0.0f;
    for (int wv = 0; wv < NT / WAVE; ++wv) total += wsum[wv];
    partial[blockIdx.x] = total;
  }
}

// ---------------------------------------------------------------------------
// Per-event log-sum-exp ONLY (no posterior write-back): reads logw [K, N],
// writes lse [N] + per-block likelihood partials. Pairs with the lse-aware
// M-step kernels (they apply exp(logw - lse) while staging w), which
// deletes the [K, N] posterior write+read round trip of the two-kernel
// E-step path entirely.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(NT)
estep_lse_kernel(const float* __restrict__ logw, float* __restrict__ lse,
                 float* __restrict__ partial, int k, int64_t n) {
  float acc = 0.0f;
  for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n;
       e += (int64_t)gridDim.x * NT) {
    float m = logw[e];
#pragma unroll 4
    for (int c = 1; c < k; ++c) m = fmaxf(m, logw[(int64_t)c * n + e]);
    float s = 0.0f;
#pragma unroll 4
    for (int c = 0; c < k; ++c) s += __expf(logw[(int64_t)c * n + e] - m);
    const float denom = m + __logf(s);
    lse[e] = denom;
    acc += denom;
  }
  __shared__ float wsum[NT / WAVE];
  for (int off = WAVE / 2; off > 0; off >>= 1)
    acc += __shfl_down(acc, off, WAVE);
  const int wid = threadIdx.x / WAVE;
  if ((threadIdx.x & (WAVE - 1)) == 0) wsum[wid] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float total = 0.0f;
    for (int wv = 0; wv < NT / WAVE; ++wv) total += wsum[wv];
    partial[blockIdx.x] = total;
  }
}

// ---------------------------------------------------------------------------
// Per-event training weights s_e >= 0: the lse-aware M-step kernels stage
// exp(logw - lse), so  s_e * posterior = exp(logw - (lse - ln s_e))  and a
// weighted M-step is the same kernels reading the shifted lse written here:
//   lse_w[e] = lse[e] - lns[e]     (lns = ln s, -inf where s == 0)
//   lse_w[e] = +inf where s[e] == 0, whatever lse holds (-inf - -inf is
//              NaN): the staged weight exp(logw - inf) is then an exact 0.
// With `partial` non-null each block also writes its share of the weighted
// log-likelihood sum_e s_e * lse_e to partial[blockIdx.x] (zero-weight
// terms skipped, not multiplied: 0 * inf is NaN) for reduce_scalar_kernel.
// Every thread walks a fixed set of events in a fixed order and block_sum
// is fixed-order: deterministic, no float atomics.
// Memory-bound (12 B read + 4 B written per event): the first nvec * 4
// events move as 16-byte vectors (the launcher passes nvec = 0 when a
// pointer is not 16-byte aligned), the rest as a scalar tail.
// ---------------------------------------------------------------------------
#define EW_VEC 4  // events per thread and grid-stride step

__device__ __forceinline__ float event_weight_one(float l, float s, float ls,
                                                  float* acc) {
  if (s == 0.0f) return INFINITY;
  *acc += s * l;
  return l - ls;
}

__global__ void __launch_bounds__(NT)
event_weight_lse_kernel(const float* __restrict__ lse,
                        const float* __restrict__ s,
                        const float* __restrict__ lns,
                        float* __restrict__ lse_w,
                        float* __restrict__ partial, int64_t nvec,
                        int64_t n) {
  float acc = 0.0f;
  const int64_t stride = (int64_t)gridDim.x * NT;
  const int64_t t0 = (int64_t)blockIdx.x * NT + threadIdx.x;
  const f32x4* lse4 = reinterpret_cast<const f32x4*>(lse);
  const f32x4* s4 = reinterpret_cast<const f32x4*>(s);
  const f32x4* lns4 = reinterpret_cast<const f32x4*>(lns);
  f32x4* out4 = reinterpret_cast<f32x4*>(lse_w);
  for (int64_t v = t0; v < nvec; v += stride) {
    const f32x4 l = lse4[v];
    const f32x4 sv = s4[v];
    const f32x4 ls = lns4[v];
    f32x4 o;
#pragma unroll
    for (int u = 0; u < EW_VEC; ++u)
      o[u] = event_weight_one(l[u], sv[u], ls[u], &acc);
    out4[v] = o;
  }
  for (int64_t e = nvec * EW_VEC + t0; e < n; e += stride)
    lse_w[e] = event_weight_one(lse[e], s[e], lns[e], &acc);
  if (partial != nullptr) {  // kernel argument: uniform over the block
    __shared__ float wsum[NT / WAVE];
    block_sum(acc, wsum, partial);
  }
}

// ---------------------------------------------------------------------------
// Uniform background component: the mixture (1 - pi0) sum_c pi_c N_c + pi0/V
// rides on the same contract. With b = ln(pi0 / (1 - pi0)) - ln V read from
// the device scalar bg[1] (so a captured graph follows its updates):
//   lse_b[e] = logaddexp(lse[e], b)   (b = -inf: lse_b == lse bit for bit;
//                                      both -inf: -inf)
//   r0[e]    = exp(b - lse_b[e])      background posterior (0 at b = -inf)
//   lse_m[e] = lse_b[e]               what the moments kernels then read
// With weights (W) it replaces event_weight_lse_kernel in the chain instead
// of following it: lse_m = lse_b - lns, +inf where s == 0 (bitwise that
// kernel applied to lse_b). lse_b is also stored when `lse_b` is non-null
// (a weighted fit needs it to normalise posteriors for output).
// Block partials: n0_part[blockIdx.x] = sum s_e r0_e on every call, and
// lik_part[blockIdx.x] = sum s_e lse_b_e when `lik_part` is non-null
// (zero-weight events skipped in both). Same geometry, vector / tail split
// and fixed summation order as event_weight_lse_kernel: deterministic.
// The accurate expf / log1pf (not the fast intrinsics): the correction term
// log1p(exp(-|lse - b|)) <= ln 2 is the whole effect at small pi0.
// ---------------------------------------------------------------------------
template <bool W>
__device__ __forceinline__ float background_one(float l, float b, float s,
                                                float ls, float* lb_out,
                                                float* n0, float* lik) {
  float lb = l, r0 = 0.0f;
  if (b != -INFINITY) {
    const float hi = fmaxf(l, b);
    lb = hi + log1pf(expf(-fabsf(l - b)));
    r0 = expf(b - lb);
  }
  *lb_out = lb;
  if (W) {
    if (s == 0.0f) return INFINITY;
    *n0 += s * r0;
    *lik += s * lb;
    return lb - ls;
  }
  *n0 += r0;
  *lik += lb;
  return lb;
}

template <bool W>
__global__ void __launch_bounds__(NT)
background_lse_kernel(const float* __restrict__ lse,
                      const float* __restrict__ bg,
                      const float* __restrict__ s,
                      const float* __restrict__ lns,
                      float* __restrict__ lse_m, float* __restrict__ lse_b,
                      float* __restrict__ n0_part,
                      float* __restrict__ lik_part, int64_t nvec,
                      int64_t n) {
  const float b = bg[1];
  float n0 = 0.0f, lik = 0.0f;
  const int64_t stride = (int64_t)gridDim.x * NT;
  const int64_t t0 = (int64_t)blockIdx.x * NT + threadIdx.x;
  const f32x4* lse4 = reinterpret_cast<const f32x4*>(lse);
  const f32x4* s4 = reinterpret_cast<const f32x4*>(s);
  const f32x4* lns4 = reinterpret_cast<const f32x4*>(lns);
  f32x4* m4 = reinterpret_cast<f32x4*>(lse_m);
  f32x4* b4 = reinterpret_cast<f32x4*>(lse_b);
  for (int64_t v = t0; v < nvec; v += stride) {
    const f32x4 l = lse4[v];
    f32x4 sv = {1.0f, 1.0f, 1.0f, 1.0f}, ls = {0.0f, 0.0f, 0.0f, 0.0f};
    if (W) {
      sv = s4[v];
      ls = lns4[v];
    }
    f32x4 o, ob;
#pragma unroll
    for (int u = 0; u < EW_VEC; ++u) {
      float lb;
      o[u] = background_one<W>(l[u], b, sv[u], ls[u], &lb, &n0, &lik);
      ob[u] = lb;
    }
    m4[v] = o;
    if (lse_b != nullptr) b4[v] = ob;
  }
  for (int64_t e = nvec * EW_VEC + t0; e < n; e += stride) {
    float lb;
    lse_m[e] = background_one<W>(lse[e], b, W ? s[e] : 1.0f,
                                 W ? lns[e] : 0.0f, &lb, &n0, &lik);
    if (lse_b != nullptr) lse_b[e] = lb;
  }
  __shared__ float wsum0[NT / WAVE];
  block_sum(n0, wsum0, n0_part);
  if (lik_part != nullptr) {  // kernel argument: uniform over the block
    __shared__ float wsum1[NT / WAVE];
    block_sum(lik, wsum1, lik_part);
  }
}

// One block: n0 = sum of the nparts background partials (the reduce_scalar
// order: fixed per lane, then wave order), then the new background state
//   bg[0] = pi0     = min(n0 / n_total, 1 - 1e-6)
//   bg[1] = b       = ln pi0 - ln(1 - pi0) - lnV   (-inf at pi0 == 0)
//   bg[2] = lik_add = n_total * ln(1 - pi0)
//   bg[3] = n0
// The scalar tail runs in double on one thread and rounds once per value.
// No host synchronisation: the E-step that follows reads bg[1] on device.
__global__ void __launch_bounds__(NT)
background_update_kernel(const float* __restrict__ n0_part, int64_t nparts,
                         double n_total, double ln_v,
                         float* __restrict__ bg) {
  float acc = 0.0f;
  for (int64_t i = threadIdx.x; i < nparts; i += NT) acc += n0_part[i];
  __shared__ float wsum[NT / WAVE];
  for (int off = WAVE / 2; off > 0; off >>= 1)
    acc += __shfl_down(acc, off, WAVE);
  if ((threadIdx.x & (WAVE - 1)) == 0) wsum[threadIdx.x / WAVE] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float n0 = 0.0f;
    for (int wv = 0; wv < NT / WAVE; ++wv) n0 += wsum[wv];
    double pi0 = (double)n0 / n_total;
    if (!(pi0 > 0.0)) pi0 = 0.0;
    if (pi0 > 1.0 - 1e-6) pi0 = 1.0 - 1e-6;
    const double l1m = log1p(-pi0);
    bg[0] = (float)pi0;
    bg[1] = pi0 > 0.0 ? (float)(log(pi0) - l1m - ln_v) : -INFINITY;
    bg[2] = (float)(n_total * l1m);
    bg[3] = n0;
  }
}

// ---------------------------------------------------------------------------
// Student-t mixture components (fixed degrees of freedom nu) on the lse
// contract: one pass over the Gaussian log-weights logw[c*n + e] =
// add_c - q/2 an lse-family E-step left, rewriting what the M-step reads.
// Per (cluster, event), with h = (nu + D) / 2 and delta(nu, D) the constant
// that turns the Gaussian normaliser into the t one:
//   q    = max(0, 2 (add_c - logw))             squared Mahalanobis distance
//   lt   = (add_c + delta) - h log1p(q / nu)    ln(pi_c t_c(x_e))
//   u    = (nu + D) / (nu + q)                  the latent scale's mean
// and per event lse_t = logsumexp_c lt by an online (max, sum) recurrence.
// TRAIN: logw <- lt + ln u, so exp(logw - lse_m) is s tau u, the weight of
//   the parameter-expanded M-step; lse_m = lse_t, or with weights (W)
//   lse_t - lns and +inf where s == 0 (bitwise event_weight_lse_kernel on
//   lse_t); lse_t itself is stored too. Block partials, written by every
//   launched block: n_part[blockIdx.x * k + c] = sum_e s_e exp(lt - lse_t)
//   (the true responsibilities: pi and N come from them, not from the
//   moments' corner) and, when lik_part is non-null, lik_part[blockIdx.x] =
//   sum_e s_e lse_t (zero-weight events skipped, not multiplied).
// !TRAIN (posterior): logw <- lt, lse_t stored, nothing else written.
// q = +inf gives lt = -inf and weight 0; an event whose lt are all -inf has
// lse_t = -inf and contributes exact zeros to n_part, never NaN.
//
// Geometry: a block walks tiles of NT * V events (tile = blockIdx.x,
// += gridDim.x), V = 4 events per thread as one 16-byte access over the
// first nvec * 4 events (the launcher passes nvec = 0 unless every pointer
// is 16-byte aligned and n % 4 == 0, which keeps every cluster row aligned)
// and V = 1 over the rest. Posterior mode sweeps a thread's column of logw
// once, storing lt as it goes. Train mode sweeps it twice per tile: once for
// lse_t (kept in registers with s), once to rewrite logw and sum
// exp(lt - lse_t), which needs the finished lse_t (lt + ln u alone would not
// let the second sweep recover lt); the tile's 1024 K floats were just
// read, so the second read is served by whatever cache still holds them. The
// per-cluster sums go wave-reduce -> this wave's row of the LDS table
// [NT / WAVE][k] (only that wave ever touches its row, tiles in order) ->
// one combine in wave order at the end: fixed event sets, fixed order, no
// float atomics. The accurate expf / logf / log1pf, as in background_lse:
// h log1p(q / nu) is the whole tail behaviour.
// ---------------------------------------------------------------------------
template <int V>
__device__ __forceinline__ void st_load(const float* p, float* o) {
  if constexpr (V == 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int u = 0; u < 4; ++u) o[u] = v[u];
  } else {
    o[0] = p[0];
  }
}

template <int V>
__device__ __forceinline__ void st_store(float* p, const float* o) {
  if constexpr (V == 4) {
    f32x4 v;
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = o[u];
    *reinterpret_cast<f32x4*>(p) = v;
  } else {
    p[0] = o[0];
  }
}

// One tile: this thread's V events start at e0 (`active` false past the
// end: the thread still takes part in the wave sums, adding zeros).
template <int V, bool W, bool TRAIN>
__device__ __forceinline__ void student_t_tile(
    float* __restrict__ logw, const float* __restrict__ add,
    const float* __restrict__ s, const float* __restrict__ lns,
    float* __restrict__ lse_m, float* __restrict__ lse_t, int k, int64_t n,
    int64_t e0, bool active, float nu, float nud, float delta,
    float* __restrict__ tab_row, float* lik) {
  const float h = 0.5f * nud;
  float lt_lse[V], sv[V];
#pragma unroll
  for (int u = 0; u < V; ++u) {
    lt_lse[u] = -INFINITY;
    sv[u] = 1.0f;
  }
  if (active) {
    float m[V], sum[V];
#pragma unroll
    for (int u = 0; u < V; ++u) {
      m[u] = -INFINITY;
      sum[u] = 0.0f;
    }
    for (int c = 0; c < k; ++c) {
      const float ac = add[c];
      const float a = ac + delta;
      float lw[V];
      st_load<V>(logw + (int64_t)c * n + e0, lw);
#pragma unroll
      for (int u = 0; u < V; ++u) {
        const float q = fmaxf(0.0f, 2.0f * (ac - lw[u]));
        const float lt = a - h * log1pf(q / nu);
        if (lt > m[u]) {
          // m == -inf: expf(-inf) = 0 and the sum restarts at 1
          sum[u] = sum[u] * expf(m[u] - lt) + 1.0f;
          m[u] = lt;
        } else if (lt != -INFINITY) {
          sum[u] += expf(lt - m[u]);
        }
        lw[u] = lt;
      }
      // posterior mode is done with this column after one sweep: lt does
      // not depend on lse_t
      if (!TRAIN) st_store<V>(logw + (int64_t)c * n + e0, lw);
    }
#pragma unroll
    for (int u = 0; u < V; ++u)
      lt_lse[u] = m[u] == -INFINITY ? -INFINITY : m[u] + logf(sum[u]);
    st_store<V>(lse_t + e0, lt_lse);
    if (TRAIN) {
      float lm[V];
      if (W) {
        float ls[V];
        st_load<V>(s + e0, sv);
        st_load<V>(lns + e0, ls);
#pragma unroll
        for (int u = 0; u < V; ++u)
          lm[u] = event_weight_one(lt_lse[u], sv[u], ls[u], lik);
      } else {
#pragma unroll
        for (int u = 0; u < V; ++u) {
          lm[u] = lt_lse[u];
          *lik += lt_lse[u];
        }
      }
      st_store<V>(lse_m + e0, lm);
    }
  }
  if (!TRAIN) return;
  // second sweep (train): rewrite logw, per-cluster sums of the
  // responsibilities exp(lt - lse_t), which need the finished lse_t
  for (int c = 0; c < k; ++c) {
    float acc = 0.0f;
    if (active) {
      const float ac = add[c];
      const float a = ac + delta;
      float lw[V];
      st_load<V>(logw + (int64_t)c * n + e0, lw);
#pragma unroll
      for (int u = 0; u < V; ++u) {
        const float q = fmaxf(0.0f, 2.0f * (ac - lw[u]));
        const float lt = a - h * log1pf(q / nu);
        lw[u] = lt + logf(nud / (nu + q));
        if (lt != -INFINITY && !(W && sv[u] == 0.0f)) {
          const float tau = expf(lt - lt_lse[u]);
          acc += W ? sv[u] * tau : tau;
        }
      }
      st_store<V>(logw + (int64_t)c * n + e0, lw);
    }
    for (int off = WAVE / 2; off > 0; off >>= 1)
      acc += __shfl_down(acc, off, WAVE);
    if ((threadIdx.x & (WAVE - 1)) == 0) tab_row[c] += acc;
  }
}

template <bool W, bool TRAIN>
__global__ void __launch_bounds__(NT)
student_t_lse_kernel(float* __restrict__ logw, const float* __restrict__ add,
                     const float* __restrict__ s,
                     const float* __restrict__ lns,
                     float* __restrict__ lse_m, float* __restrict__ lse_t,
                     float* __restrict__ n_part,
                     float* __restrict__ lik_part, int k, int64_t nvec,
                     int64_t n, float nu, float nud, float delta) {
  extern __shared__ float st_tab[];  // TRAIN: [NT / WAVE][k]
  float* tab_row = st_tab + (size_t)(threadIdx.x / WAVE) * k;
  if (TRAIN) {
    for (int c = threadIdx.x; c < (NT / WAVE) * k; c += NT) st_tab[c] = 0.0f;
    __syncthreads();
  }
  float lik = 0.0f;
  const int64_t vtiles = (nvec + NT - 1) / NT;
  for (int64_t t = blockIdx.x; t < vtiles; t += gridDim.x) {
    const int64_t v = t * NT + threadIdx.x;
    student_t_tile<EW_VEC, W, TRAIN>(logw, add, s, lns, lse_m, lse_t, k, n,
                                     v * EW_VEC, v < nvec, nu, nud, delta,
                                     tab_row, &lik);
  }
  const int64_t tail0 = nvec * EW_VEC;
  const int64_t ttiles = (n - tail0 + NT - 1) / NT;
  for (int64_t t = blockIdx.x; t < ttiles; t += gridDim.x) {
    const int64_t e = tail0 + t * NT + threadIdx.x;
    student_t_tile<1, W, TRAIN>(logw, add, s, lns, lse_m, lse_t, k, n, e,
                                e < n, nu, nud, delta, tab_row, &lik);
  }
  if (TRAIN) {
    __syncthreads();
    for (int c = threadIdx.x; c < k; c += NT) {
      float total = 0.0f;
      for (int wv = 0; wv < NT / WAVE; ++wv) total += st_tab[wv * k + c];
      n_part[(int64_t)blockIdx.x * k + c] = total;
    }
    if (lik_part != nullptr) {  // kernel argument: uniform over the block
      __shared__ float wsum[NT / WAVE];
      block_sum(lik, wsum, lik_part);
    }
  }
}

// One block, after finalize: the mixing weights and counts of a t fit from
// the reduced responsibilities n_c = sum_e s_e tau_ce (finalize derived its
// own from the moments' corner, which holds sum s tau u):
//   N[c] = n_c,  pi[c] = n_c < 0.5 ? 1e-10 : n_c / sum_c n_c
// with the sum taken in cluster order by one fp32 accumulator, as finalize
// does; add[c] = constant[c] + logf(pi[c]) when `add` is non-null.
__global__ void __launch_bounds__(NT)
student_t_pi_kernel(const float* __restrict__ n_c,
                    const float* __restrict__ constant,
                    float* __restrict__ n_out, float* __restrict__ pi,
                    float* __restrict__ add, int k) {
  __shared__ float total_sh;
  if (threadIdx.x == 0) {
    float total = 0.0f;
    for (int c = 0; c < k; ++c) total += n_c[c];
    total_sh = total;
  }
  __syncthreads();
  const float total = total_sh;
  for (int c = threadIdx.x; c < k; c += NT) {
    const float nc = n_c[c];
    const float p = nc < 0.5f ? 1e-10f : nc / total;
    n_out[c] = nc;
    pi[c] = p;
    if (add != nullptr) add[c] = constant[c] + logf(p);
  }
}

// Deterministic chunk reduction: out[j] = sum_i in[i*m + j] (fixed i
// order). Replaces torch's generic reduce_kernel (19.6 us for the
// [256, K*Pp] moments partials).
__global__ void __launch_bounds__(NT)
reduce_chunks_kernel(const float* __restrict__ in, float* __restrict__ out,
                     int c, int64_t m) {
  // 8 independent accumulators: m is only ~20k columns, so without ILP the
  // chunk loop serializes on memory latency (measured 78 us vs torch's
  // 19). The reassociation is FIXED (same order every run): acc[u] takes
  // chunks i == u (mod 8) in ascending order, then the tree below. The
  // main loop only puts 32 loads in flight before the first add (8 left
  // the kernel at 32 dependent round trips, 12.8 us for 21 MB); the adds
  // keep that order. One-wave blocks spread the columns over every CU.
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m;
       j += (int64_t)gridDim.x * blockDim.x) {
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int i = 0;
    for (; i + 32 <= c; i += 32) {
      float v[32];
#pragma unroll
      for (int u = 0; u < 32; ++u) v[u] = in[(int64_t)(i + u) * m + j];
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int u = 0; u < 8; ++u) acc[u] += v[8 * q + u];
    }
    for (; i + 8 <= c; i += 8) {
#pragma unroll
      for (int u = 0; u < 8; ++u) acc[u] += in[(int64_t)(i + u) * m + j];
    }
    for (; i < c; ++i) acc[0] += in[(int64_t)i * m + j];
    out[j] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) +
             ((acc[4] + acc[5]) + (acc[6] + acc[7]));
  }
}

// Scalar sum: out[0] = sum in[0..n) (single block, fixed order per lane
// then wave-order combine — deterministic).
__global__ void __launch_bounds__(NT)
reduce_scalar_kernel(const float* __restrict__ in, float* __restrict__ out,
                     int64_t n) {
  // each lane adds in[tid], in[tid + NT], ... in that order; the loads of
  // 16 terms are issued together so the chain is not one memory round
  // trip per term (31 of them at the flagship's 7813 partials)
  constexpr int U = 16;
  float acc = 0.0f;
  for (int64_t i = threadIdx.x; i < n; i += (int64_t)U * NT) {
    float v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t idx = i + (int64_t)u * NT;
      v[u] = in[idx < n ? idx : i];
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (i + (int64_t)u * NT < n) acc += v[u];
  }
  __shared__ float wsum[NT / WAVE];
  for (int off = WAVE / 2; off > 0; off >>= 1)
    acc += __shfl_down(acc, off, WAVE);
  if ((threadIdx.x & (WAVE - 1)) == 0) wsum[threadIdx.x / WAVE] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float total = 0.0f;
    for (int wv = 0; wv < NT / WAVE; ++wv) total += wsum[wv];
    out[0] = total;
  }
}

// ---------------------------------------------------------------------------
// M-step covariance: packed second moments S_c = sum_e w_ce x_e x_e^T
// (replaces mstep_covariance1, gaussian_kernel.cu:605 — but uncentered;
// the engine finalizes R = (S - N mu mu^T + G avgvar I)/N, identical math).
//
// Grid (K, NCHUNK); each block accumulates its chunk of event tiles into
// registers (PPT pairs per thread, compile-time) and writes
// partials[chunk, c, p] once — summed deterministically on the host side.
// Event tiles staged through LDS as float4 (conflict-free b128 groups with
// the +1 float4 row pad).
// ---------------------------------------------------------------------------
template <int PPT, typename T>
__global__ void __launch_bounds__(NT)
mstep_cov_kernel(const T* __restrict__ x, const float* __restrict__ w,
                 const float* __restrict__ lse,
                 float* __restrict__ partials, int d, int k, int64_t n,
                 int te, int nchunk) {
  // lds: xs[d][te + 4] floats (te multiple of 4), then wt[te]
  extern __shared__ float lds[];
  const int row = te + 4;
  float* xs = lds;
  float* wt = lds + (int64_t)d * row;

  const int c = blockIdx.x;
  const int chunk = blockIdx.y;
  const int p_total = d * (d + 1) / 2;

  int pr[PPT], pc[PPT];
#pragma unroll
  for (int u = 0; u < PPT; ++u) {
    const int t = threadIdx.x + u * NT;
    if (t < p_total) tri_row_col(t, &pr[u], &pc[u]);
    else { pr[u] = 0; pc[u] = 0; }
  }
  float acc[PPT];
#pragma unroll
  for (int u = 0; u < PPT; ++u) acc[u] = 0.0f;

  const int64_t tiles = (n + te - 1) / te;
  for (int64_t tile = chunk; tile < tiles; tile += nchunk) {
    const int64_t e0 = tile * te;
    const int cnt = (int)min((int64_t)te, n - e0);
    __syncthreads();
    // stage x tile (coalesced per dimension row) and w tile; branchless
    // when the tile is full (guide §5 trap 4c)
    // per-element runtime selects inside staging loops serialize every
    // load behind vmcnt(0) (guide §5 trap 4c) — the lse test is hoisted
    // into duplicated loops instead
    if (cnt == te) {
      for (int i = threadIdx.x; i < d * te; i += NT)
        xs[(i / te) * row + i % te] =
            load_x(x, (int64_t)(i / te) * n + e0 + i % te);
      if (lse) {
        for (int ei = threadIdx.x; ei < te; ei += NT)
          wt[ei] = __expf(w[(int64_t)c * n + e0 + ei] - lse[e0 + ei]);
      } else {
        for (int ei = threadIdx.x; ei < te; ei += NT)
          wt[ei] = w[(int64_t)c * n + e0 + ei];
      }
    } else {
      for (int i = threadIdx.x; i < d * te; i += NT) {
        const int di = i / te, ei = i % te;
        xs[di * row + ei] =
            (ei < cnt) ? load_x(x, (int64_t)di * n + e0 + ei) : 0.0f;
      }
      if (lse) {
        for (int ei = threadIdx.x; ei < te; ei += NT)
          wt[ei] = (ei < cnt)
              ? __expf(w[(int64_t)c * n + e0 + ei] - lse[e0 + ei]) : 0.0f;
      } else {
        for (int ei = threadIdx.x; ei < te; ei += NT)
          wt[ei] = (ei < cnt) ? w[(int64_t)c * n + e0 + ei] : 0.0f;
      }
    }
    __syncthreads();

#pragma unroll
    for (int u = 0; u < PPT; ++u) {
      if (threadIdx.x + u * NT >= p_total) continue;
      const float4* xi = (const float4*)(xs + pr[u] * row);
      const float4* xj = (const float4*)(xs + pc[u] * row);
      const float4* wv = (const float4*)wt;
      float a = acc[u];
#pragma unroll 2
      for (int e4 = 0; e4 < te / 4; ++e4) {
        const float4 vi = xi[e4], vj = xj[e4], vw = wv[e4];
        a = fmaf(vw.x * vi.x, vj.x, a);
        a = fmaf(vw.y * vi.y, vj.y, a);
        a = fmaf(vw.z * vi.z, vj.z, a);
        a = fmaf(vw.w * vi.w, vj.w, a);
      }
      acc[u] = a;
    }
  }
#pragma unroll
  for (int u = 0; u < PPT; ++u) {
    const int t = threadIdx.x + u * NT;
    if (t < p_total)
      partials[((int64_t)chunk * k + c) * p_total + t] = acc[u];
  }
}

// ---------------------------------------------------------------------------
// Constants: batched in-LDS no-pivot LU inversion + ln|det| + constant
// (replaces constants_kernel / device invert, gaussian_kernel.cu:107-259,
// parallelized instead of the reference's single-thread LU; dynamic LDS
// sized for D up to 128 — no NUM_DIMENSIONS cap).
// One workgroup per cluster. Crout-style: L keeps the diagonal, U unit.
// ---------------------------------------------------------------------------
// ---------------------------------------------------------------------------
// M-step finalize (one workgroup per cluster): from the all-reduced packed
// moments [K, Dp(Dp+1)/2] produce N, means, R and pi with the reference's
// exact rules (cov zero at N<1, G*avgvar on the diagonal,
// divide at N>0.5 else identity; means zero at N<=0.5; pi floor 1e-10).
// Replaces ~15 eager torch ops per iteration.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(NT)
mstep_finalize_kernel(const float* __restrict__ packed,
                      const float* __restrict__ avgvar, int world,
                      float* __restrict__ n_out, float* __restrict__ means,
                      float* __restrict__ r_out, float* __restrict__ pi,
                      int d, int k, int diag_only) {
  extern __shared__ float mu[];  // [d] this cluster's means
  const int c = blockIdx.x;
  const int dp = d + 1;
  const int pp = dp * (dp + 1) / 2;
  const int p = d * (d + 1) / 2;
  const float* row = packed + (int64_t)c * pp;
  const float n_c = row[pp - 1];
  const bool ge1 = n_c >= 1.0f;
  const bool gt05 = n_c > 0.5f;

  if (threadIdx.x == 0) {
    n_out[c] = n_c;
    // pi = N/sum(N) with the 1e-10 floor (compute_pi semantics)
    float total = 0.0f;
    for (int cc = 0; cc < k; ++cc) total += packed[(int64_t)cc * pp + pp - 1];
    pi[c] = (n_c < 0.5f) ? 1e-10f : n_c / total;
  }
  for (int i = threadIdx.x; i < d; i += NT) {
    const float m = gt05 ? row[p + i] / n_c : 0.0f;
    mu[i] = m;
    means[(int64_t)c * d + i] = m;
  }
  __syncthreads();
  const float reg = world * avgvar[c];
  for (int t = threadIdx.x; t < p; t += NT) {
    int i, j;
    tri_row_col(t, &i, &j);
    float cov = ge1 ? row[t] - n_c * mu[i] * mu[j] : 0.0f;
    if (diag_only && i != j) cov = 0.0f;
    if (i == j) cov += reg;
    float rv;
    if (gt05) rv = cov / n_c;
    else rv = (i == j) ? 1.0f : 0.0f;
    r_out[((int64_t)c * d + i) * d + j] = rv;
    if (i != j) r_out[((int64_t)c * d + j) * d + i] = rv;
  }
}

// Emit the fused-E-step factor M = [F | -F mu] with F = L^-1 where
// L L^T = R (lower Cholesky of the COVARIANCE, not of Rinv): then
// q = ||F z||^2 = z^T R^-1 z exactly. Factoring R — which is positive
// definite by construction (covariance + avgvar ridge; identity resets)
// — is stable where the previous chol(Rinv) exploded: a no-pivot fp32
// LU inverse of an ill-conditioned R loses positive-definiteness and
// clamped pivots cascade into ~1e15-scale factor rows whose quadratic
// forms overflow fp32 (K >> N/D regimes).
// acc - round(x * y): the empty asm makes the product a value of its own,
// so the compiler cannot contract the pair into one fused multiply-add.
__device__ __forceinline__ float unfused_mulsub(float acc, float x, float y) {
  float p = x * y;
  asm("" : "+v"(p));
  return acc - p;
}

// ---- the factor chain in registers, D <= 32 (wave 0 of the block) ----
// The general chain below meets at a workgroup barrier after every column
// and walks its sums through LDS; at D <= 32 one wave holds the whole
// matrix, a row or column per lane, and neither is needed. Both halves are
// right-looking: a finished value is applied at once to every element that
// still waits for it, so the updates of one step are independent of each
// other and only divide -> broadcast -> update is serial. Each element
// still receives the same operations in the same kk order as in the general
// chain, so the results are the same bits. DM is the unroll bound (register
// arrays need static indices); steps at or past d are skipped by a uniform
// branch, lanes and columns past d compute values nobody stores.
__device__ __forceinline__ float lane_bcast(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// Lower Cholesky of R in a [d*ldp] (lower triangle read), L written back
// over it, diagonal included. Lane i owns row i.
template <int DM>
__device__ __forceinline__ void chol_regs(float* a, int d, int ldp) {
  const int lane = threadIdx.x;
  const bool alive = lane < d;
  float* ri = a + (alive ? lane : 0) * ldp;
  float w[DM];
#pragma unroll
  for (int m = 0; m < DM; ++m) w[m] = (alive && m <= lane) ? ri[m] : 0.0f;
  // the pivot of row i is R[i][i] - sum_kk L[i][kk]^2 in kk order, kept as
  // a running sum of its own and frozen once column i - 1 is done
  float sd = alive ? ri[lane] : 0.0f;
  const float lo = fmaf(1e-8f, fabsf(sd), 1e-30f);
  float pv = sqrtf(fmaxf(sd, lo));
#pragma unroll
  for (int j = 0; j + 1 < DM; ++j) {
    if (j + 1 >= d) continue;
    const float l = w[j] / lane_bcast(pv, j);
    if (lane > j) {
      if (alive) ri[j] = l;
      sd = fmaf(-l, l, sd);
      pv = sqrtf(fmaxf(sd, lo));
    }
#pragma unroll
    for (int m = j + 1; m < DM; ++m) w[m] = fmaf(-l, lane_bcast(l, m), w[m]);
  }
  if (alive) ri[lane] = pv;
}

// F = L^-1 (lower) by forward substitution, L read from a, F written to o.
// Lane i owns column i and counts rows from its own diagonal: g[n] is
// F[i+n][i], xv[n] its running sum. With that numbering the split of a sum
// into fused head and unfused eights, (j - i) & 7 = n & 7 terms long, is the
// same for every lane and known at compile time. L[i+n][i+t] differs per
// lane, so it comes from LDS; none of those loads waits for the chain.
template <int DM>
__device__ __forceinline__ void inv_regs(const float* a, float* o, int d,
                                         int ldp) {
  const int lane = threadIdx.x;
  const int i = lane < d ? lane : 0;
  // lane's row i + n of L from column i on; rows past d read a[t], t < d
  int off[DM];
#pragma unroll
  for (int n = 0; n < DM; ++n)
    off[n] = (lane + n < d) ? (i + n) * ldp + i : 0;
  // the sums start from a +0 the compiler cannot see through: from a
  // literal it makes -p of 0 - p, which is -0 where the product is +0 (the
  // rows of an identity R), and the general chain subtracts from a register
  float zero = 0.0f;
  asm("" : "+v"(zero));
  float g[DM], xv[DM];
#pragma unroll
  for (int n = 0; n < DM; ++n) xv[n] = zero;
  g[0] = 1.0f / a[off[0]];
  if (lane < d) o[off[0]] = g[0];
#pragma unroll
  for (int t = 0; t + 1 < DM; ++t) {
    if (t + 1 >= d) continue;
#pragma unroll
    for (int n = t + 1; n < DM; ++n) {
      const float lv = a[off[n] + t];
      xv[n] = (t < (n & 7)) ? fmaf(-lv, g[t], xv[n])
                            : unfused_mulsub(xv[n], lv, g[t]);
    }
    g[t + 1] = xv[t + 1] / a[off[t + 1] + t + 1];
    if (lane + t + 1 < d) o[off[t + 1]] = g[t + 1];
  }
}

template <int DM>
__device__ __forceinline__ void chain_regs(float* a, float* o, int d,
                                           int ldp) {
  chol_regs<DM>(a, d, ldp);
  // lanes read what other lanes of this wave wrote: LDS serves one wave's
  // accesses in order, the fence keeps the compiler from moving them
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  inv_regs<DM>(a, o, d, ldp);
}

// `a` is scratch LDS [d*ldp] for R, factored in place into L (only the
// lower triangle is read); with r_global == nullptr the caller has put R
// there already, barrier included. `o` [d*ldp] receives F (lower triangle
// only); u0 [d] follows o. Thread i owns row i of L and column i of F, so
// d <= blockDim.x (the launchers check it; LDS stops at D = 142 anyway).
// Every element keeps the operations and the kk-ascending order of the
// straightforward column Cholesky / forward substitution; what changed is
// who computes them and how often the block meets at a barrier.
// (forced inline: as a call it takes runtime null checks and a stack frame)
__device__ __forceinline__ void emit_mfac(
    float* a, float* o, const float* __restrict__ r_global,
    const float* __restrict__ means, __hip_bfloat16* __restrict__ mfac,
    float* __restrict__ mfac32, int c, int d,
    const float* __restrict__ pi = nullptr,
    float* __restrict__ constant = nullptr,
    float* __restrict__ add = nullptr) {
  const int tid = threadIdx.x;
  // odd LDS row stride: stride-d column walks with gcd(d, 32) > 1 put
  // whole lane groups on one bank (8-way at d = 24)
  const int ldp = d | 1;
  float* u0 = o + d * ldp;
  if (r_global != nullptr) {
    for (int t = tid; t < d * d; t += blockDim.x)
      a[(t / d) * ldp + t % d] = r_global[(int64_t)c * d * d + t];
    __syncthreads();
  }
  // D <= 32: wave 0 runs both halves of the chain in registers (above) and
  // leaves L in a and F in o; the other waves wait for it here
  const bool regs = d <= 32;
  if (regs) {
    if (tid < WAVE) {
      if (d <= 8) chain_regs<8>(a, o, d, ldp);
      else if (d <= 16) chain_regs<16>(a, o, d, ldp);
      else if (d <= 24) chain_regs<24>(a, o, d, ldp);
      else chain_regs<32>(a, o, d, ldp);
    }
    __syncthreads();
  }
  // in-place lower Cholesky of R, one barrier per column. The pivot of
  // row i is R[i][i] - sum_kk L[i][kk]^2 in kk order: the row's owner
  // keeps that running sum in a register, subtracts each L[i][j] as it
  // produces it, and publishes the pivot together with L[i][i-1], one
  // column step before anyone reads it (a lone thread used to walk the
  // row through LDS for every pivot, between two barriers of its own).
  if (!regs) {
    const bool own = tid < d;
    float* ri = a + tid * ldp;
    float sd = 0.0f, diag0 = 0.0f;
    if (own) {
      sd = ri[tid];
      diag0 = fabsf(sd);
    }
    if (tid == 0) ri[0] = sqrtf(fmaxf(sd, fmaf(1e-8f, diag0, 1e-30f)));
    __syncthreads();
    for (int j = 0; j + 1 < d; ++j) {
      if (own && tid > j) {
        const float* rj = a + j * ldp;
        float s = ri[j];
#pragma unroll 8
        for (int kk = 0; kk < j; ++kk) s = fmaf(-ri[kk], rj[kk], s);
        const float l = s / rj[j];
        ri[j] = l;
        sd = fmaf(-l, l, sd);
        if (tid == j + 1)
          ri[tid] = sqrtf(fmaxf(sd, fmaf(1e-8f, diag0, 1e-30f)));
      }
      __syncthreads();
    }
  }
  // ln|R| = 2 sum ln diag(L): lets the EM iteration skip the LU kernel
  // entirely on the factor paths (constant = -D/2 ln 2pi - 0.5 ln|R|,
  // fp-equivalent to the LU determinant; the reference-faithful LU Rinv
  // is refreshed once per K for the merge/output path)
  if (constant != nullptr) {
    __shared__ float wsum_e[NT / WAVE];
    const int nw = (blockDim.x + WAVE - 1) / WAVE;
    float acc = 0.0f;
    for (int i = tid; i < d; i += blockDim.x)
      acc += __logf(a[i * ldp + i]);
    for (int off = WAVE / 2; off > 0; off >>= 1)
      acc += __shfl_down(acc, off, WAVE);
    if ((tid & (WAVE - 1)) == 0) wsum_e[tid / WAVE] = acc;
    __syncthreads();
    if (tid == 0) {
      const float ld2 = 2.0f * (wsum_e[0] + ((nw > 1) ? wsum_e[1] : 0.0f) +
                                ((nw > 2) ? wsum_e[2] : 0.0f) +
                                ((nw > 3) ? wsum_e[3] : 0.0f));
      const float cst = -d * 0.5f * 1.8378770664093453f - 0.5f * ld2;
      constant[c] = cst;
      if (add) add[c] = cst + __logf(pi[c]);
    }
    __syncthreads();
  }
  // F = L^-1 (lower) by forward substitution, L read from a and F written
  // to o (no snapshot copy: nothing is overwritten). Thread i owns column
  // i, serial down the rows; its own earlier F values come back from o.
  // The sum runs in kk order with the rounding the kernel has always had:
  // the first (j - i) % 8 terms as fused multiply-adds, the rest in eights
  // as a rounded product subtracted (unfused_mulsub keeps it that way).
  if (!regs && tid < d) {
    const int i = tid;
    for (int j = i; j < d; ++j) {
      const float* lj = a + j * ldp;
      float xv = 1.0f;
      if (i != j) {
        xv = 0.0f;
        int kk = i;
        for (const int head = i + ((j - i) & 7); kk < head; ++kk)
          xv = fmaf(-lj[kk], o[kk * ldp + i], xv);
        for (; kk < j; kk += 8) {
          float lv[8], fv[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            lv[u] = lj[kk + u];
            fv[u] = o[(kk + u) * ldp + i];
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) xv = unfused_mulsub(xv, lv[u], fv[u]);
        }
      }
      o[j * ldp + i] = xv / lj[j];
    }
  }
  __syncthreads();
  // u0 = -F mu (mu = centered cluster means; F lower: j <= i)
  if (tid < d) {
    const float* fi = o + tid * ldp;
    float s = 0.0f;
#pragma unroll 8
    for (int j = 0; j <= tid; ++j) s = fmaf(fi[j], means[c * d + j], s);
    u0[tid] = -s;
  }
  __syncthreads();
  // write hi/lo bf16 fragments: rows padded to RT*32, k-slots to KC*16
  // (RT = ceil(d/32) row-tiles, KC = ceil((d+1)/16) MFMA k-chunks; for
  // d <= 31 this is the original [32][32] layout). k-order is contiguous
  // (identity fragment map, hardware-verified by the probes). A work item
  // is 8 consecutive k-slots of one row (cols is a multiple of 16): built
  // in registers, stored as 16 bytes per bf16 plane and 32 bytes of fp32.
  const int rows = mfac_rows(d);
  const int cols = mfac_kct(d) * 16;
  const int cells = rows * cols;
  const int cpr = cols >> 3;  // items per row
  __hip_bfloat16* out = mfac + (int64_t)c * 2 * cells;
  float* out32 = mfac32 ? mfac32 + (int64_t)c * cells : nullptr;
  for (int g = tid; g < rows * cpr; g += blockDim.x) {
    const int i = g / cpr, kx0 = (g - i * cpr) << 3;
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = 0.0f;
    if (i < d && kx0 <= d) {
      const float* fi = o + i * ldp;
      const float ui = u0[i];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int kx = kx0 + u;
        // clamped address: the row's slots past the diagonal are not F
        const float f = fi[min(kx, i)];
        v[u] = (kx <= i) ? f : ((kx == d) ? ui : 0.0f);
      }
    }
    unsigned int ph[4], pl[4];
#pragma unroll
    for (int u = 0; u < 8; u += 2) {
      const __hip_bfloat16 h0 = __float2bfloat16(v[u]);
      const __hip_bfloat16 h1 = __float2bfloat16(v[u + 1]);
      const __hip_bfloat16 l0 = __float2bfloat16(v[u] - __bfloat162float(h0));
      const __hip_bfloat16 l1 =
          __float2bfloat16(v[u + 1] - __bfloat162float(h1));
      ph[u >> 1] = (unsigned int)__bfloat16_as_ushort(h0) |
                   ((unsigned int)__bfloat16_as_ushort(h1) << 16);
      pl[u >> 1] = (unsigned int)__bfloat16_as_ushort(l0) |
                   ((unsigned int)__bfloat16_as_ushort(l1) << 16);
    }
    const int t = g << 3;
    *(uint4*)(out + t) = make_uint4(ph[0], ph[1], ph[2], ph[3]);
    *(uint4*)(out + cells + t) = make_uint4(pl[0], pl[1], pl[2], pl[3]);
    if (out32) {
      *(float4*)(out32 + t) = make_float4(v[0], v[1], v[2], v[3]);
      *(float4*)(out32 + t + 4) = make_float4(v[4], v[5], v[6], v[7]);
    }
  }
}

// Fused M-step finalize + factor/constants emission (one block per
// cluster): the finalize's R lands in this block's L1, the emission
// reloads it without a kernel boundary, and the EM iteration drops one
// launch. Fast-path only (lazy-Rinv engines); the split kernels remain
// for the VALU/diag paths.
__global__ void __launch_bounds__(NT)
mstep_finalize_emit_kernel(const float* __restrict__ packed,
                           const float* __restrict__ avgvar, int world,
                           float* __restrict__ n_out,
                           float* __restrict__ means,
                           float* __restrict__ r_out,
                           float* __restrict__ pi,
                           float* __restrict__ constant,
                           float* __restrict__ add,
                           __hip_bfloat16* __restrict__ mfac,
                           float* __restrict__ mfac32, int d, int k) {
  extern __shared__ float lds[];
  const int ldp = d | 1;
  float* a = lds;                 // emit working buffer [d*ldp]
  float* o = a + d * ldp;         // emit snapshot [d*ldp] (+u0 [d])
  float* mu = o + d * ldp;        // borrow u0 space for mu during finalize
  const int c = blockIdx.x;
  const int dp = d + 1;
  const int pp = dp * (dp + 1) / 2;
  const int p = d * (d + 1) / 2;
  const float* row = packed + (int64_t)c * pp;
  const float n_c = row[pp - 1];
  const bool ge1 = n_c >= 1.0f;
  const bool gt05 = n_c > 0.5f;

  if (threadIdx.x < WAVE) {
    // pi denominator: sum of all N in cluster order, one fp32 accumulator.
    // Wave 0 loads 64 of them at a time, a lane each, and adds them lane
    // by lane (a single thread walking k strided loads one after the
    // other kept the other 255 waiting at the barrier below).
    float total = 0.0f;
    for (int base = 0; base < k; base += WAVE) {
      const int cc = min(base + (int)threadIdx.x, k - 1);
      const int nv = __float_as_int(packed[(int64_t)cc * pp + pp - 1]);
      const int cnt = min(WAVE, k - base);
      if (cnt == WAVE) {
#pragma unroll
        for (int l = 0; l < WAVE; ++l)
          total += __int_as_float(__builtin_amdgcn_readlane(nv, l));
      } else {
        for (int l = 0; l < cnt; ++l)
          total += __int_as_float(__builtin_amdgcn_readlane(nv, l));
      }
    }
    if (threadIdx.x == 0) {
      n_out[c] = n_c;
      pi[c] = (n_c < 0.5f) ? 1e-10f : n_c / total;
    }
  }
  for (int i = threadIdx.x; i < d; i += NT) {
    const float m = gt05 ? row[p + i] / n_c : 0.0f;
    mu[i] = m;
    means[(int64_t)c * d + i] = m;
  }
  __syncthreads();
  const float reg = world * avgvar[c];
  for (int t = threadIdx.x; t < p; t += NT) {
    int i, j;
    tri_row_col(t, &i, &j);
    // (n_c mu_i) rounded, then one fused multiply-add, as compiled so far
    float cov = ge1 ? fmaf(-(n_c * mu[i]), mu[j], row[t]) : 0.0f;
    if (i == j) cov += reg;
    float rv;
    if (gt05) rv = cov / n_c;
    else rv = (i == j) ? 1.0f : 0.0f;
    r_out[((int64_t)c * d + i) * d + j] = rv;
    if (i != j) r_out[((int64_t)c * d + j) * d + i] = rv;
    a[i * ldp + j] = rv;  // the factorization reads the lower triangle only
  }
  __syncthreads();
  // R is already where the factorization wants it (it used to be stored
  // and read back through global memory); means are reloaded through the
  // pointer this block has just written them to
  emit_mfac(a, o, nullptr, means, mfac, mfac32, c, d, pi, constant, add);
}

// NOTE (negative result, round 2): a wave-per-cluster constants variant
// (4 independent waves per block, zero workgroup barriers, cross-lane
// LDS ordering via the wave's own lgkmcnt) measured SLOWER than this
// block-per-cluster kernel: 64/103 us vs 47/77 us (LU-only / LU+emit,
// K=64 D=24). With one cluster per wave only K/4 blocks run (16 CUs at
// K=64 vs 64) and each serial chain has a quarter of the lanes and no
// co-resident waves to hide LDS latency; the ~100 __syncthreads of the
// block variant are cheaper than that. Kept here as a ledger entry —
// do not rediscover (full details in profiles/LADDER.md).
__global__ void __launch_bounds__(NT)
constants_lu_kernel(const float* __restrict__ r,
                    const float* __restrict__ means,
                    const float* __restrict__ pi, float* __restrict__ rinv,
                    float* __restrict__ logdet,
                    float* __restrict__ constant, float* __restrict__ add,
                    __hip_bfloat16* __restrict__ mfac,
                    float* __restrict__ mfac32, int d) {
  // lds: a[d*d] working buffer, o[d*d] read-only snapshot of the LU factor.
  // The reference's in-place triangular inversion reads a mix of original
  // and already-inverted entries in a serial order; parallelized across
  // columns/rows that order only survives if cross-thread reads come from
  // a snapshot (o) and each thread's own running values stay private (a).
  extern __shared__ float a[];
  const int c = blockIdx.x;
  const int tid = threadIdx.x;
  // odd LDS row stride (see emit_mfac): kills the gcd(d, 32)-way bank
  // conflicts of stride-d column walks
  const int ldp = d | 1;
  float* o = a + d * ldp;
  const float* rc = r + (int64_t)c * d * d;
  float* oc = rinv + (int64_t)c * d * d;

  for (int t = tid; t < d * d; t += blockDim.x)
    a[(t / d) * ldp + t % d] = rc[t];
  __syncthreads();

  if (d == 1) {
    if (tid == 0) {
      const float lg = __logf(a[0]);
      logdet[c] = lg;
      const float cst = -0.5f * 1.8378770664093453f - 0.5f * lg;  // ln(2pi)
      if (constant) constant[c] = cst;
      if (add) add[c] = cst + __logf(pi[c]);
      oc[0] = 1.0f / a[0];
      o[0] = oc[0];
    }
    __syncthreads();
    if (mfac != nullptr) emit_mfac(a, o, r, means, mfac, mfac32, c, 1);
    return;
  }

  // normalize row 0 (invert_matrix.cpp:42 / gaussian_kernel.cu:120)
  for (int j = 1 + tid; j < d; j += blockDim.x) a[j] /= a[0];
  __syncthreads();

  for (int i = 1; i < d; ++i) {
    // column i of L: rows j >= i in parallel
    for (int j = i + tid; j < d; j += blockDim.x) {
      float s = 0.0f;
#pragma unroll 8
      for (int kk = 0; kk < i; ++kk)
        s = fmaf(a[j * ldp + kk], a[kk * ldp + i], s);
      a[j * ldp + i] -= s;
    }
    __syncthreads();
    if (i == d - 1) break;
    // row i of U: cols j > i in parallel
    const float pivot = a[i * ldp + i];
    for (int j = i + 1 + tid; j < d; j += blockDim.x) {
      float s = 0.0f;
#pragma unroll 8
      for (int kk = 0; kk < i; ++kk)
        s = fmaf(a[i * ldp + kk], a[kk * ldp + j], s);
      a[i * ldp + j] = (a[i * ldp + j] - s) / pivot;
    }
    __syncthreads();
  }

  // ln|det| = sum ln|diag| (natural log, gaussian_kernel.cu:139)
  {
    __shared__ float wsum[NT / WAVE];
    const int nw = (blockDim.x + WAVE - 1) / WAVE;
    float acc = 0.0f;
    for (int i = tid; i < d; i += blockDim.x)
      acc += __logf(fabsf(a[i * ldp + i]));
    for (int off = WAVE / 2; off > 0; off >>= 1)
      acc += __shfl_down(acc, off, WAVE);
    if ((tid & (WAVE - 1)) == 0) wsum[tid / WAVE] = acc;
    __syncthreads();
    if (tid == 0) {
      float total = 0.0f;
      for (int wv = 0; wv < nw; ++wv) total += wsum[wv];
      logdet[c] = total;
      // constant = -D/2 ln(2pi) - 0.5 ln|R| (gaussian_kernel.cu:241)
      const float cst = -d * 0.5f * 1.8378770664093453f - 0.5f * total;
      if (constant) constant[c] = cst;
      if (add) add[c] = cst + __logf(pi[c]);
    }
  }
  __syncthreads();
  // snapshot the LU factor: the inversion below reads original L/U values
  // that the in-place writes would otherwise clobber across threads
  for (int t = tid; t < d * ldp; t += blockDim.x) o[t] = a[t];
  __syncthreads();

  // invert L: column i per thread, serial down rows; cross-column reads and
  // the diagonal divisor come from the snapshot (gaussian_kernel.cu:142-151:
  // data[j,k] for k>i and data[j,j] are pre-inversion values there)
  for (int i = tid; i < d; i += blockDim.x) {
    for (int j = i; j < d; ++j) {
      float xv = 1.0f;
      if (i != j) {
        xv = 0.0f;
#pragma unroll 8
        for (int kk = i; kk < j; ++kk)
          xv -= o[j * ldp + kk] * a[kk * ldp + i];
      }
      a[j * ldp + i] = xv / o[j * ldp + j];
    }
  }
  // invert U: row i per thread, serial across cols; column reads from the
  // snapshot (gaussian_kernel.cu:152-159: data[k,j] for k>i pre-inversion),
  // row reads from this thread's own inverted values. Disjoint from the L
  // writes (strict upper vs lower+diag) so no barrier is needed between.
  for (int i = tid; i < d; i += blockDim.x) {
    for (int j = i + 1; j < d; ++j) {
      float s = 0.0f;
#pragma unroll 8
      for (int kk = i; kk < j; ++kk)
        s += o[kk * ldp + j] * ((i == kk) ? 1.0f : a[i * ldp + kk]);
      a[i * ldp + j] = -s;
    }
  }
  __syncthreads();
  // final composition Rinv[j,i] = sum_{kk>=max(i,j)} Uinv[j,kk]*Linv[kk,i]
  // (gaussian_kernel.cu:160-166) — each output element independent; write
  // straight to global (reads see the pre-write LDS values, same as the
  // reference's read-before-write order)
  for (int t = tid; t < d * d; t += blockDim.x) {
    const int j = t / d, i = t % d;
    float s = 0.0f;
#pragma unroll 8
    for (int kk = (i > j ? i : j); kk < d; ++kk)
      s = fmaf((j == kk) ? 1.0f : a[j * ldp + kk], a[kk * ldp + i], s);
    oc[j * d + i] = s;
  }
  if (mfac != nullptr) {
    __syncthreads();
    // factor emission re-reads R from global and factors it directly
    emit_mfac(a, o, r, means, mfac, mfac32, c, d);
  }
}

// ---------------------------------------------------------------------------
// MFMA M-step: fused augmented moments  T_c = sum_e w_ce [x;1][x;1]^T
// via v_mfma_f32_16x16x4_f32 (exact f32 fmaf chain — bitwise an f32 VALU
// loop, guide §3) — one kernel produces S, the mean numerators AND N
// (replaces mstep_N + mstep_means + mstep_covariance1,
// gaussian_kernel.cu:522-677, and the separate rocBLAS GEMM).
//
// Packed output layout per cluster (lower triangle of (D+1)x(D+1)):
//   [0, P)        S rows 0..D-1   (P = D(D+1)/2)
//   [P, P+D)      mean numerators (row D, cols 0..D-1)
//   [P+D]         N               (row D, col D)
// Grid (ceil(K/4), nchunk): 4 waves per block, one cluster per wave, all
// sharing the LDS event tile. D <= 31 (Dp = D+1 <= 32: 2 row-tiles).
// f32 MFMA fragment maps (guide §3): A lane l -> A[i=l&15][k=l>>4],
// B lane l -> B[k=l>>4][j=l&15]; C/D: col=l&15, row=(l>>4)*4+reg.
// ---------------------------------------------------------------------------
#define MOM_BK 128

// When `lse` is non-null, `w` holds LOG weights and the effective weight is
// exp(w - lse[e]) computed while staging (bit-identical to the normalize
// pass it replaces — same __expf on the same operands). Pad events get 0.
template <typename T>
__global__ void __launch_bounds__(NT)
mstep_moments_kernel(const T* __restrict__ x, const float* __restrict__ w,
                     const float* __restrict__ lse,
                     float* __restrict__ partials, int d, int k, int64_t n,
                     int nchunk) {
  // Exact-fp32 augmented moments on v_mfma_f32_16x16x4_f32, with
  // double-buffered register-staged tiles (T14) like the bf16x3 kernel.
  // LDS per buffer: xs [d][MOM_BK+4] f32, wt [4][MOM_BK] f32.
  extern __shared__ float lds[];
  const int row = MOM_BK + 4;
  const int plane = d * row;
  float* xs0 = lds;
  float* wt0 = lds + plane;
  float* xs1 = wt0 + 4 * MOM_BK;
  float* wt1 = xs1 + plane;

  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int c = blockIdx.x * 4 + wave;
  const int chunk = blockIdx.y;
  const int dp = d + 1;
  const int rt2 = dp > 16;

  f32x4 acc00 = {0, 0, 0, 0}, acc10 = {0, 0, 0, 0}, acc11 = {0, 0, 0, 0};
  const int i_loc = lane & 15;
  const int kk = lane >> 4;              // event sub-index 0..3

  const int xq_total = d * (MOM_BK / 4);
  const int nxq = (xq_total + NT - 1) / NT;  // <= 4 at D <= 31
  const int64_t tiles = (n + MOM_BK - 1) / MOM_BK;
  const int64_t my_tiles =
      chunk < tiles ? (tiles - chunk + nchunk - 1) / nchunk : 0;

  float4 rx[4];
  float4 rw;
  auto issue_loads = [&](int64_t tile) {
    const int64_t e0 = tile * MOM_BK;
    const bool full = (n - e0) >= MOM_BK;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int q = threadIdx.x + s * NT;
      if (s < nxq && q < xq_total) {
        const int di = q / (MOM_BK / 4), eq = q % (MOM_BK / 4);
        const int64_t g = (int64_t)di * n + e0 + eq * 4;
        if (full || eq * 4 + 3 < (int)(n - e0)) {
          rx[s] = make_float4(load_x(x, g), load_x(x, g + 1),
                              load_x(x, g + 2), load_x(x, g + 3));
        } else {
          float v[4];
          for (int u = 0; u < 4; ++u)
            v[u] = (e0 + eq * 4 + u < n) ? load_x(x, g + u) : 0.0f;
          rx[s] = *(float4*)v;
        }
      }
    }
    if (threadIdx.x < 4 * (MOM_BK / 4)) {
      const int wv = threadIdx.x / (MOM_BK / 4);
      const int eq = threadIdx.x % (MOM_BK / 4);
      const int cw = blockIdx.x * 4 + wv;
      if (cw < k) {
        const int64_t g = (int64_t)cw * n + e0 + eq * 4;
        const int64_t ge = e0 + eq * 4;
        if (full && lse) {
          rw = *(const float4*)&w[g];
          const float4 lv = *(const float4*)&lse[ge];
          rw.x = __expf(rw.x - lv.x);
          rw.y = __expf(rw.y - lv.y);
          rw.z = __expf(rw.z - lv.z);
          rw.w = __expf(rw.w - lv.w);
        } else if (full) {
          rw = *(const float4*)&w[g];
        } else {
          float v[4];
          for (int u = 0; u < 4; ++u) {
            const bool ok = ge + u < n;
            v[u] = ok ? w[g + u] : 0.0f;
            if (lse) v[u] = ok ? __expf(v[u] - lse[ge + u]) : 0.0f;
          }
          rw = *(float4*)v;
        }
      } else {
        rw = (float4){0, 0, 0, 0};
      }
    }
  };
  auto write_buf = [&](float* xs, float* wt) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int q = threadIdx.x + s * NT;
      if (s < nxq && q < xq_total) {
        const int di = q / (MOM_BK / 4), eq = q % (MOM_BK / 4);
        *(float4*)(xs + di * row + eq * 4) = rx[s];
      }
    }
    if (threadIdx.x < 4 * (MOM_BK / 4))
      *(float4*)(wt + threadIdx.x * 4) = rw;
  };

  if (my_tiles > 0) {
    issue_loads(chunk);
    write_buf(xs0, wt0);
  }
  __syncthreads();

  int cur = 0;
  for (int64_t ti = 0; ti < my_tiles; ++ti) {
    if (ti + 1 < my_tiles) issue_loads(chunk + (ti + 1) * nchunk);
    const float* xs = cur ? xs1 : xs0;
    const float* wt = cur ? wt1 : wt0;

    for (int ks = 0; ks < MOM_BK / 4; ++ks) {
      const int e = ks * 4 + kk;
      const float we = wt[wave * MOM_BK + e];
      const int g0 = i_loc;             // row-tile 0 rows 0..15
      const int g1 = 16 + i_loc;        // row-tile 1 rows 16..31
      const float z0 = (g0 < d) ? xs[g0 * row + e] : (g0 == d ? 1.0f : 0.0f);
      const float z1 = (g1 < d) ? xs[g1 * row + e] : (g1 == d ? 1.0f : 0.0f);
      const float a0 = we * z0;
      acc00 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, z0, acc00, 0, 0, 0);
      if (rt2) {
        const float a1 = we * z1;
        acc10 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, z0, acc10, 0, 0, 0);
        acc11 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, z1, acc11, 0, 0, 0);
      }
    }
    // single barrier per tile: the write targets the buffer nobody reads
    // this iteration, and the previous barrier already ordered its readers
    if (ti + 1 < my_tiles) write_buf(cur ? xs0 : xs1, cur ? wt0 : wt1);
    __syncthreads();
    cur ^= 1;
  }

  if (c >= k) return;
  const int p_aug = dp * (dp + 1) / 2;
  float* out = partials + ((int64_t)chunk * k + c) * p_aug;
  // C/D layout: col = lane&15, row = (lane>>4)*4 + reg
  const int col = lane & 15;
  const int row0 = (lane >> 4) * 4;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    {  // tile (0,0): keep lower triangle
      const int gi = row0 + r, gj = col;
      if (gi < dp && gj <= gi) out[gi * (gi + 1) / 2 + gj] = acc00[r];
    }
    if (rt2) {
      const int gi = 16 + row0 + r;
      {  // tile (1,0)
        const int gj = col;
        if (gi < dp) out[gi * (gi + 1) / 2 + gj] = acc10[r];
      }
      {  // tile (1,1)
        const int gj = 16 + col;
        if (gi < dp && gj <= gi) out[gi * (gi + 1) / 2 + gj] = acc11[r];
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Split-precision (bf16x3) augmented moments: same packed output as
// mstep_moments_kernel but on v_mfma_f32_32x32x16_bf16 at ~15x the f32
// MFMA rate. Each operand is split into bf16 hi+lo parts; the three
// products hi*hi + hi*lo + lo*hi are accumulated in fp32 and the lo*lo
// term (relative magnitude ~2^-16 per element) is dropped — ~1e-5-class
// relative accuracy on S vs the exact-fp32 kernel.
//   A[i=dim][kk=event] = w[e] * z_i[e]   (split per cluster)
//   B[kk=event][j=dim] = z_j[e]          (split once, shared by 4 clusters)
// ---------------------------------------------------------------------------
#define MB_BK 128
#define MB_NT 512
#define MB_CPB 8  // clusters per block (one per wave; 8 halves x re-reads)

__global__ void __launch_bounds__(MB_NT)
mstep_moments_b16_kernel(const __hip_bfloat16* __restrict__ xhi,
                         const __hip_bfloat16* __restrict__ xlo,
                         const float* __restrict__ w,
                         const float* __restrict__ lse,
                         float* __restrict__ partials, int d, int k,
                         int64_t n, int nchunk) {
  // Split-precision moments with double-buffered, register-staged tiles
  // (guide T14): tile t+1's global loads are issued before tile t's MFMA
  // work and written to the other LDS buffer after it — the measured 52%
  // SQ_WAIT share was staging latency exposed at the tile barrier.
  // x arrives pre-split into persistent hi/lo bf16 planes.
  // LDS per buffer: zhi/zlo [32][136] bf16, wt [MB_CPB][MB_BK] f32.
  extern __shared__ float lds[];
  constexpr int ZBR = MB_BK + 8;
  constexpr int PLANE = 32 * ZBR;          // bf16 elements per z plane
  constexpr int BUFB = 2 * PLANE;          // zhi+zlo per buffer (bf16)
  __bf16* zbuf = (__bf16*)lds;             // [2][2*PLANE]
  float* wbuf = (float*)(zbuf + 2 * BUFB); // [2][MB_CPB*MB_BK]

  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int j32 = lane & 31;
  const int g2 = lane >> 5;
  const int c = blockIdx.x * MB_CPB + wave;
  const int chunk = blockIdx.y;
  const int dp = d + 1;

  // this thread's staging assignment: quads of 4 consecutive events
  // (x: d*MB_BK/4 quads; w: MB_CPB*MB_BK/4 float4, first quarter of threads)
  const int xq_total = d * (MB_BK / 4);
  const int nxq = (xq_total + MB_NT - 1) / MB_NT;  // <= 2 at D <= 31

  f32x16_t accA = (f32x16_t)(0.0f);   // hi*hi
  f32x16_t accB = (f32x16_t)(0.0f);   // hi*lo + lo*hi (shared accumulator)

  const int64_t tiles = (n + MB_BK - 1) / MB_BK;
  const int64_t my_tiles =
      chunk < tiles ? (tiles - chunk + nchunk - 1) / nchunk : 0;

  // ---- staging helpers -------------------------------------------------
  uint2 rxh[2], rxl[2];
  float4 rw;
  auto issue_loads = [&](int64_t tile) {
    const int64_t e0 = tile * MB_BK;
    const bool full = (n - e0) >= MB_BK;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int q = threadIdx.x + s * MB_NT;
      if (s < nxq && q < xq_total) {
        const int di = q / (MB_BK / 4), eq = q % (MB_BK / 4);
        const int64_t g = (int64_t)di * n + e0 + eq * 4;
        if (full || eq * 4 + 3 < (int)(n - e0)) {
          rxh[s] = *(const uint2*)&xhi[g];
          rxl[s] = *(const uint2*)&xlo[g];
        } else {  // tail tile: element-wise guarded
          __hip_bfloat16 h[4], l[4];
          for (int u = 0; u < 4; ++u) {
            const bool ok = e0 + eq * 4 + u < n;
            h[u] = ok ? xhi[g + u] : __hip_bfloat16(0.0f);
            l[u] = ok ? xlo[g + u] : __hip_bfloat16(0.0f);
          }
          rxh[s] = *(uint2*)h;
          rxl[s] = *(uint2*)l;
        }
      }
    }
    const int wq_total = MB_CPB * (MB_BK / 4);
    if (threadIdx.x < wq_total) {
      const int wv = threadIdx.x / (MB_BK / 4);
      const int eq = threadIdx.x % (MB_BK / 4);
      const int cw = blockIdx.x * MB_CPB + wv;
      if (cw < k) {
        const int64_t g = (int64_t)cw * n + e0 + eq * 4;
        const int64_t ge = e0 + eq * 4;
        if (full && lse) {
          rw = *(const float4*)&w[g];
          const float4 lv = *(const float4*)&lse[ge];
          rw.x = __expf(rw.x - lv.x);
          rw.y = __expf(rw.y - lv.y);
          rw.z = __expf(rw.z - lv.z);
          rw.w = __expf(rw.w - lv.w);
        } else if (full) {
          rw = *(const float4*)&w[g];
        } else {
          float v[4];
          for (int u = 0; u < 4; ++u) {
            const bool ok = ge + u < n;
            v[u] = ok ? w[g + u] : 0.0f;
            if (lse) v[u] = ok ? __expf(v[u] - lse[ge + u]) : 0.0f;
          }
          rw = *(float4*)v;
        }
      } else {
        rw = (float4){0, 0, 0, 0};
      }
    }
  };
  auto write_buf = [&](int buf) {
    __bf16* zh = zbuf + buf * BUFB;
    __bf16* zl = zh + PLANE;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int q = threadIdx.x + s * MB_NT;
      if (s < nxq && q < xq_total) {
        const int di = q / (MB_BK / 4), eq = q % (MB_BK / 4);
        *(uint2*)(zh + di * ZBR + eq * 4) = rxh[s];
        *(uint2*)(zl + di * ZBR + eq * 4) = rxl[s];
      }
    }
    if (threadIdx.x < MB_CPB * (MB_BK / 4))
      *(float4*)(wbuf + buf * MB_CPB * MB_BK + threadIdx.x * 4) = rw;
  };
  // constant rows (ones at d, zeros above) in BOTH buffers, written once;
  // a tail tile is always the globally last so no re-fix is needed
  for (int b = 0; b < 2; ++b) {
    __bf16* zh = zbuf + b * BUFB;
    __bf16* zl = zh + PLANE;
    for (int idx = d * MB_BK + threadIdx.x; idx < 32 * MB_BK; idx += blockDim.x) {
      const int di = idx / MB_BK, ei = idx % MB_BK;
      zh[di * ZBR + ei] = (__bf16)(di == d ? 1.0f : 0.0f);
      zl[di * ZBR + ei] = (__bf16)0.0f;
    }
  }

  if (my_tiles > 0) {
    issue_loads(chunk);
    write_buf(0);
  }
  __syncthreads();

  int cur = 0;
  for (int64_t ti = 0; ti < my_tiles; ++ti) {
    if (ti + 1 < my_tiles) issue_loads(chunk + (ti + 1) * nchunk);
    const __bf16* zh = zbuf + cur * BUFB;
    const __bf16* zl = zh + PLANE;
    const float* wt = wbuf + cur * MB_CPB * MB_BK;

#pragma unroll 2
    for (int ch = 0; ch < MB_BK / 16; ++ch) {
      const int eb = ch * 16 + 8 * g2;
      const bf16x8 b_hi = *(const bf16x8*)(zh + j32 * ZBR + eb);
      const bf16x8 b_lo = *(const bf16x8*)(zl + j32 * ZBR + eb);
      const float4 wv0 = *(const float4*)(wt + wave * MB_BK + eb);
      const float4 wv1 = *(const float4*)(wt + wave * MB_BK + eb + 4);
      const float wv[8] = {wv0.x, wv0.y, wv0.z, wv0.w,
                           wv1.x, wv1.y, wv1.z, wv1.w};
      bf16x8 a_hi, a_lo;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const float zf = (float)b_hi[u] + (float)b_lo[u];
        const float av = wv[u] * zf;
        const __bf16 hi = (__bf16)av;
        a_hi[u] = hi;
        a_lo[u] = (__bf16)(av - (float)hi);
      }
      accA = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, b_hi, accA, 0, 0, 0);
      accB = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, b_lo, accB, 0, 0, 0);
      accB = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_lo, b_hi, accB, 0, 0, 0);
    }
    // single barrier per tile: the write targets the buffer nobody reads
    // this iteration, and the previous barrier already ordered its readers
    if (ti + 1 < my_tiles) write_buf(cur ^ 1);
    __syncthreads();  // buf[cur^1] ready for the next iteration
    cur ^= 1;
  }

  if (c >= k) return;
  const int p_aug = dp * (dp + 1) / 2;
  float* out = partials + ((int64_t)chunk * k + c) * p_aug;
  // C/D layout: col = l&31, row = (reg&3) + 8*(reg>>2) + 4*(l>>5)
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int gi = (r & 3) + 8 * (r >> 2) + 4 * g2;
    const int gj = j32;
    if (gi < dp && gj <= gi)
      out[gi * (gi + 1) / 2 + gj] = accA[r] + accB[r];
  }
}

// ---------------------------------------------------------------------------
// Split-precision (bf16x3) moments regrouped as ONE GEMM over pair columns:
//   T_c[i,j] = sum_e w_ce (z_i z_j)_e   ->   C[K x PP] = W[K x N] . P[N x PP]
// with column p = i(i+1)/2 + j (j <= i) — exactly the packed row layout of
// partials[chunk][c][.], so there is no triangle masking and no wasted upper
// half. The per-(cluster, dim, event) rebuild + hi/lo split of A = w.z that
// bounds mstep_moments_b16_kernel is gone:
//   A[row=cluster][kk=event] = w        split ONCE by the staging thread
//   B[kk=event][col=pair]    = z_i z_j  built + split in registers, shared
//                                       by all 64 clusters of the block
// One block owns 16*NCT clusters (NCT 16-row A tiles; 64 clusters up to
// D = 26) and ALL pair tiles of its event chunk, so w (the 256 MB operand)
// is read once. Pair tiles are 16 columns wide on v_mfma_f32_16x16x32_bf16;
// wave v of 8 owns tiles v, v+8, ... (TPW per wave, statically indexed
// accumulators: 8*TPW*NCT registers). D >= 27 (TPW 4-5) runs NCT = 2 to
// stay inside the register file without spilling.
// LDS per buffer: z [32][MP_ZROW] f32 (hi+lo rebuilt once at staging),
// w hi / w lo [16*NCT][MP_WROW] bf16 — an A fragment is one ds_read_b128.
// ---------------------------------------------------------------------------
#define MP_BK 128
#define MP_NT 512
#define MP_WROW (MP_BK + 8)   // bf16 per staged w row
#define MP_ZROW (MP_BK + 4)   // f32 per staged z row
// bytes per LDS buffer for NCT 16-row cluster tiles per block
#define MP_BUF_BYTES(NCT) (32 * MP_ZROW * 4 + 2 * 16 * (NCT) * MP_WROW * 2)

template <int TPW, int NCT>
__global__ void __launch_bounds__(MP_NT)
mstep_moments_pair_b16_kernel(const __hip_bfloat16* __restrict__ xhi,
                              const __hip_bfloat16* __restrict__ xlo,
                              const float* __restrict__ w,
                              const float* __restrict__ lse,
                              float* __restrict__ partials, int d, int k,
                              int64_t n, int nchunk) {
  extern __shared__ float lds[];
  constexpr int CB = 16 * NCT;          // clusters per block
  constexpr int WPLANE = CB * MP_WROW;  // bf16 elements per w plane
  constexpr int BUFB = MP_BUF_BYTES(NCT);
  char* lds_b = (char*)lds;

  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const int lane = threadIdx.x & (WAVE - 1);
  const int r16 = lane & 15;
  const int g4 = lane >> 4;
  const int chunk = blockIdx.y;
  const int c0 = blockIdx.x * CB;
  const int dp = d + 1;
  const int pp = dp * (dp + 1) / 2;
  // live 16-row cluster tiles of this block (block-uniform)
  const int nct = (min(CB, k - c0) + 15) / 16;

  // this lane's pair column per owned tile: z rows (i, j), fixed for the
  // whole kernel. Columns >= PP (a whole dead tile included) compute on
  // row 0 and are never stored: no per-tile branch in the k-loop.
  int zoff_i[TPW], zoff_j[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int p = (wave + 8 * t) * 16 + r16;
    int i = 0, j = 0;
    if (p < pp) tri_row_col(p, &i, &j);
    zoff_i[t] = i * MP_ZROW + 8 * g4;
    zoff_j[t] = j * MP_ZROW + 8 * g4;
  }

  f32x4 accA[TPW][NCT], accB[TPW][NCT];  // hi*hi | hi*lo + lo*hi
#pragma unroll
  for (int t = 0; t < TPW; ++t)
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
      accA[t][ct] = (f32x4)(0.0f);
      accB[t][ct] = (f32x4)(0.0f);
    }

  const int64_t tiles = (n + MP_BK - 1) / MP_BK;
  // (the 64-bit divide runs on the VALU: readfirstlane keeps the tile
  // count, and every branch on it, scalar)
  const int my_tiles = __builtin_amdgcn_readfirstlane(
      chunk < tiles ? (int)((tiles - chunk + nchunk - 1) / nchunk) : 0);
  // the one partial tile is the globally last; it is this chunk's last
  const bool has_tail =
      (n % MP_BK) != 0 && my_tiles > 0 &&
      chunk + (int64_t)(my_tiles - 1) * nchunk == tiles - 1;

  // ---- staging: quads of 4 consecutive events --------------------------
  // x: d*32 quads over 2 x 512 slots, slots past the end repeat the last
  // quad (same value to the same address) so the path has no branch;
  // w: CB rows x 32 quads, each thread one event quad of rows cr, cr+16,
  // ... (lse shared); rows >= K load row K-1 and stage as zero.
  const int xq_last = d * (MP_BK / 4) - 1;
  const int eq = threadIdx.x % (MP_BK / 4);
  const int cr = threadIdx.x / (MP_BK / 4);
  int xdi[2], xeq[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int q = min((int)threadIdx.x + s * MP_NT, xq_last);
    xdi[s] = q / (MP_BK / 4);
    xeq[s] = q % (MP_BK / 4);
  }
  uint2 rxh[2], rxl[2];
  float4 rw[NCT], rl;
  rl = (float4){0, 0, 0, 0};
  // full tile: raw vector loads only, so nothing here waits on memory;
  // __expf(w - lse) and the hi/lo split happen in write_buf, after the
  // MFMA work of the current tile
  auto issue_full = [&](int64_t tile) {
    const int64_t e0 = tile * MP_BK;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int64_t g = (int64_t)xdi[s] * n + e0 + xeq[s] * 4;
      rxh[s] = *(const uint2*)&xhi[g];
      rxl[s] = *(const uint2*)&xlo[g];
    }
    const int64_t ge = e0 + eq * 4;
    if (lse) rl = *(const float4*)&lse[ge];
#pragma unroll
    for (int s = 0; s < NCT; ++s) {
      const int cw = min(c0 + cr + 16 * s, k - 1);
      rw[s] = *(const float4*)&w[(int64_t)cw * n + ge];
    }
  };
  // tail tile: element-wise guarded; pad events carry x = 0 and the w that
  // stages as 0 (-inf under lse, else 0)
  auto issue_tail = [&](int64_t tile) {
    const int64_t e0 = tile * MP_BK;
    const float wpad = lse ? -INFINITY : 0.0f;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int64_t ge = e0 + xeq[s] * 4;
      const int64_t g = (int64_t)xdi[s] * n + ge;
      __hip_bfloat16 h[4], l[4];
      for (int u = 0; u < 4; ++u) {
        const bool ok = ge + u < n;
        h[u] = ok ? xhi[g + u] : __hip_bfloat16(0.0f);
        l[u] = ok ? xlo[g + u] : __hip_bfloat16(0.0f);
      }
      rxh[s] = *(uint2*)h;
      rxl[s] = *(uint2*)l;
    }
    const int64_t ge = e0 + eq * 4;
    float lv[4] = {0, 0, 0, 0};
    if (lse)
      for (int u = 0; u < 4; ++u)
        if (ge + u < n) lv[u] = lse[ge + u];
    rl = *(float4*)lv;
#pragma unroll
    for (int s = 0; s < NCT; ++s) {
      const int cw = min(c0 + cr + 16 * s, k - 1);
      const int64_t g = (int64_t)cw * n + ge;
      float v[4];
      for (int u = 0; u < 4; ++u) v[u] = ge + u < n ? w[g + u] : wpad;
      rw[s] = *(float4*)v;
    }
  };
  auto write_buf = [&](int buf) {
    float* zf = (float*)(lds_b + buf * BUFB);
    __bf16* wh = (__bf16*)(zf + 32 * MP_ZROW);
    __bf16* wl = wh + WPLANE;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const __bf16* h = (const __bf16*)&rxh[s];
      const __bf16* l = (const __bf16*)&rxl[s];
      float4 z;
      z.x = (float)h[0] + (float)l[0];
      z.y = (float)h[1] + (float)l[1];
      z.z = (float)h[2] + (float)l[2];
      z.w = (float)h[3] + (float)l[3];
      *(float4*)(zf + xdi[s] * MP_ZROW + xeq[s] * 4) = z;
    }
    // w split into bf16 hi/lo ONCE here, not per consuming wave
#pragma unroll
    for (int s = 0; s < NCT; ++s) {
      float v[4] = {rw[s].x, rw[s].y, rw[s].z, rw[s].w};
      if (lse) {
        v[0] = __expf(v[0] - rl.x);
        v[1] = __expf(v[1] - rl.y);
        v[2] = __expf(v[2] - rl.z);
        v[3] = __expf(v[3] - rl.w);
      }
      const bool row_ok = c0 + cr + 16 * s < k;
      __bf16 h[4], l[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float vu = row_ok ? v[u] : 0.0f;
        h[u] = (__bf16)vu;
        l[u] = (__bf16)(vu - (float)h[u]);
      }
      const int off = (cr + 16 * s) * MP_WROW + eq * 4;
      *(uint2*)(wh + off) = *(const uint2*)h;
      *(uint2*)(wl + off) = *(const uint2*)l;
    }
  };
  // one staged tile: 4 k-steps of 32 events. ALLCT drops the per-cluster-
  // tile branch from the full-block path.
  auto compute = [&](auto allct, int buf) {
    constexpr bool ALLCT = decltype(allct)::value;
    const float* zf = (const float*)(lds_b + buf * BUFB);
    const __bf16* wh = (const __bf16*)(zf + 32 * MP_ZROW);
    const __bf16* wl = wh + WPLANE;
#pragma unroll 1
    for (int ks = 0; ks < MP_BK / 32; ++ks) {
      bf16x8 a_hi[NCT], a_lo[NCT];
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) {
        const int aoff = (ct * 16 + r16) * MP_WROW + ks * 32 + 8 * g4;
        a_hi[ct] = *(const bf16x8*)(wh + aoff);
        a_lo[ct] = *(const bf16x8*)(wl + aoff);
      }
#pragma unroll
      for (int t = 0; t < TPW; ++t) {
        // B fragment: 8 events of pair column (i, j), built in registers
        const float* zi = zf + zoff_i[t] + ks * 32;
        const float* zj = zf + zoff_j[t] + ks * 32;
        const float4 i0 = *(const float4*)zi;
        const float4 i1 = *(const float4*)(zi + 4);
        const float4 j0 = *(const float4*)zj;
        const float4 j1 = *(const float4*)(zj + 4);
        const float pr[8] = {i0.x * j0.x, i0.y * j0.y, i0.z * j0.z,
                             i0.w * j0.w, i1.x * j1.x, i1.y * j1.y,
                             i1.z * j1.z, i1.w * j1.w};
        bf16x8 b_hi, b_lo;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const __bf16 hi = (__bf16)pr[u];
          b_hi[u] = hi;
          b_lo[u] = (__bf16)(pr[u] - (float)hi);
        }
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
          if (ALLCT || ct < nct) {
            accA[t][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a_hi[ct], b_hi, accA[t][ct], 0, 0, 0);
            accB[t][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a_hi[ct], b_lo, accB[t][ct], 0, 0, 0);
            accB[t][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a_lo[ct], b_hi, accB[t][ct], 0, 0, 0);
          }
        }
      }
    }
  };
  // double-buffered, register-staged tiles (T14): tile t+1's loads are
  // issued before tile t's MFMA work and written to the other buffer after
  // it. One barrier per tile: the write targets the buffer nobody reads
  // this iteration, and the previous barrier already ordered its readers.
  // The tail tile runs after the loop, un-pipelined, so the loop holds
  // only the full-tile loads (ledger R3: a shared full/tail path makes the
  // compiler wait on the loads where they are issued).
  const int nfull = my_tiles - (has_tail ? 1 : 0);
  auto main_loop = [&](auto allct) {
    int cur = 0;
    for (int ti = 0; ti < nfull; ++ti) {
      const bool more = ti + 1 < nfull;
      if (more) issue_full(chunk + (int64_t)(ti + 1) * nchunk);
      compute(allct, cur);
      if (more) write_buf(cur ^ 1);
      __syncthreads();
      cur ^= 1;
    }
    if (has_tail) {  // every reader of both buffers is past a barrier
      issue_tail(tiles - 1);
      write_buf(cur);
      __syncthreads();
      compute(allct, cur);
    }
  };

  // constant z rows (ones at d, zeros above) in BOTH buffers, written once
  for (int b = 0; b < 2; ++b) {
    float* zf = (float*)(lds_b + b * BUFB);
    for (int idx = d * MP_BK + threadIdx.x; idx < 32 * MP_BK;
         idx += MP_NT) {
      const int di = idx / MP_BK, ei = idx % MP_BK;
      zf[di * MP_ZROW + ei] = di == d ? 1.0f : 0.0f;
    }
  }
  if (nfull > 0) {
    issue_full(chunk);
    write_buf(0);
  }
  __syncthreads();
  if (nct == NCT)
    main_loop(std::true_type{});
  else
    main_loop(std::false_type{});

  // C/D layout (16x16): col = l&15 (pair), row = 4*(l>>4) + reg (cluster)
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int p = (wave + 8 * t) * 16 + r16;
    if (p < pp) {
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = c0 + ct * 16 + 4 * g4 + r;
          if (c < k)
            partials[((int64_t)chunk * k + c) * pp + p] =
                accA[t][ct][r] + accB[t][ct][r];
        }
      }
    }
  }
}

// w[c, e] = __expf(logw[c, e] - lse[e]) materialised with the same intrinsic
// the moments kernels apply at staging (lets a test feed either form).
__global__ void __launch_bounds__(NT)
exp_sub_lse_kernel(const float* __restrict__ logw,
                   const float* __restrict__ lse, float* __restrict__ out,
                   int k, int64_t n) {
  const int64_t total = (int64_t)k * n;
  for (int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * NT)
    out[idx] = __expf(logw[idx] - lse[idx % n]);
}

}  // namespace gmm

// the five MFMA fused E-step kernels for D <= 31
#include "estep_fused.hip"
// the classify kernels (score new events): label / lse / pmax per event
#include "estep_classify.hip"
// greedy k-means++ seeding: sample / evaluate / choose / commit per round
#include "seed_kmeanspp.hip"

namespace gmm {

// ---------------------------------------------------------------------------
// Big-D split-precision moments (31 < D <= 159): same packed output as the
// small-D kernels. Row-tiles of 32 cover the padded (D+1) dims; the
// RT2*(RT2+1)/2 tile-pairs of the symmetric output are split across two
// waves per cluster (two clusters per block share the staged z tile).
// Grid (ceil(K/2), nchunk); BK = 64 events per tile.
// ---------------------------------------------------------------------------
#define MBB_BK 64
#define MBB_NT 1024  // 16 waves: 2 clusters x 8 pair-groups
#define MBB_CPB 2
#define MBB_PMAX 2  // tile-pairs per wave: acc[4] x f32x16 = 64 AGPRs
                    // spilled 72 B/lane in the chunk loop (measured);
                    // 2 pairs (32 acc regs) fits

__global__ void __launch_bounds__(MBB_NT)
mstep_moments_big_kernel(const float* __restrict__ x,
                         const float* __restrict__ w,
                         const float* __restrict__ lse,
                         float* __restrict__ partials, int d, int k,
                         int64_t n, int nchunk) {
  typedef __attribute__((ext_vector_type(16))) float f32x16;
  const int dp = d + 1;
  const int rt2 = (dp + 31) / 32;
  const int rows = rt2 * 32;
  const int tp = rt2 * (rt2 + 1) / 2;
  // Augmented-row split: when D % 32 == 0 the ones row (index d) is the
  // ONLY live row of the last row-tile, so the rt2-1 tile-pairs touching
  // it run full MFMA just to produce T[d, :] = [sum w z | sum w] (the
  // mean numerators and N). Drop those pairs from the MFMA set (at
  // D=128: 15 -> 10, one third of the MFMA + A-build work) and let the
  // waves they would have occupied accumulate that row directly from
  // the staged LDS planes with plain FMA (lane = event slot:
  // conflict-free, and far off the pair-waves' critical path).
  const bool aug_split = (d & 31) == 0;
  const int tp_mfma = aug_split ? (rt2 - 1) * rt2 / 2 : tp;
  const int pair_groups = (tp_mfma + MBB_PMAX - 1) / MBB_PMAX;
  const int zbr = MBB_BK + 8;  // bf16 row stride
  // DOUBLE-BUFFERED LDS (ablation: single-buffer T14 still exposed
  // ~37% of the kernel as staging+barrier time — the write pass sat
  // between two barriers on the critical path): per buffer
  // zhi/zlo [rows][zbr] bf16 + wt [MBB_CPB][MBB_BK] f32; one barrier
  // per tile. 93 KB at D=128 -> 1 block/CU of 16 waves (4 waves/SIMD).
  extern __shared__ float lds[];
  const int zplane = rows * zbr;               // bf16 elems per z plane
  const int bufsz_b = 2 * zplane;              // bf16 elems per buffer
  __bf16* zbuf = (__bf16*)lds;                 // [2][2*zplane]
  float* wbuf = (float*)(zbuf + 2 * bufsz_b);  // [2][MBB_CPB*MBB_BK]

  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int j32 = lane & 31;
  const int g2 = lane >> 5;
  const int cw = wave >> 3;              // which of the block's 2 clusters
  const int group = wave & 7;            // which eighth of the tile-pairs
  const int c = blockIdx.x * MBB_CPB + cw;
  const int chunk = blockIdx.y;
  const int p_lo = group * MBB_PMAX;
  const int p_hi = min(tp_mfma, p_lo + MBB_PMAX);
  const bool is_aug = aug_split && group >= pair_groups;
  // lane <-> dim mapping: each aug lane owns ONE dim of T[d, :] and
  // accumulates over every event serially (one scalar accumulator —
  // a per-lane dim ARRAY spilled 7 VGPRs and taxed every wave)
  const int augdim = (group - pair_groups) * WAVE + lane;
  // hoisted pair->tile mapping (tri_row_col has a sqrtf: keep it out of
  // the chunk loop)
  int ptr[MBB_PMAX], ptc[MBB_PMAX];
#pragma unroll
  for (int pp = 0; pp < MBB_PMAX; ++pp) {
    if (p_lo + pp < tp_mfma) tri_row_col(p_lo + pp, &ptr[pp], &ptc[pp]);
    else { ptr[pp] = 0; ptc[pp] = 0; }
  }

  f32x16 acc[MBB_PMAX];
#pragma unroll
  for (int pp = 0; pp < MBB_PMAX; ++pp) acc[pp] = (f32x16)(0.0f);

  float acc_aug = 0.0f;  // this lane's running sum for T[d, augdim]

  const int64_t tiles = (n + MBB_BK - 1) / MBB_BK;
  const int64_t my_tiles =
      chunk < tiles ? (tiles - chunk + nchunk - 1) / nchunk : 0;

  // T14 register staging: tile t+1's global loads are issued before tile
  // t's MFMA work; ONE LDS buffer with the write pass after the barrier
  // (double-buffering would halve occupancy at the D=128 LDS size).
  // Pad events need no z zero-fill: their w is staged as 0, so the
  // A-side fragments vanish regardless of what B holds.
  constexpr int MBB_NXQ = 3;  // ceil(159*16/1024)
  const int xq_total = d * (MBB_BK / 4);
  const int wq_total = MBB_CPB * (MBB_BK / 4);
  float4 rx[MBB_NXQ];
  float4 rw, rl;
  auto issue_loads = [&](int64_t ti) {
    const int64_t e0 = (chunk + ti * nchunk) * MBB_BK;
    const bool full = (n - e0) >= MBB_BK;
#pragma unroll
    for (int sq = 0; sq < MBB_NXQ; ++sq) {
      const int q = threadIdx.x + sq * MBB_NT;
      if (q < xq_total) {
        const int di = q / (MBB_BK / 4), eq = q % (MBB_BK / 4);
        const float* g = x + (int64_t)di * n + e0 + eq * 4;
        if (full) {
          rx[sq] = *(const float4*)g;
        } else {
          float v[4];
#pragma unroll
          for (int u = 0; u < 4; ++u)
            v[u] = (e0 + eq * 4 + u < n) ? g[u] : 0.0f;
          rx[sq] = *(float4*)v;
        }
      }
    }
    if (threadIdx.x < wq_total) {
      const int ci = blockIdx.x * MBB_CPB + threadIdx.x / (MBB_BK / 4);
      const int eq = threadIdx.x % (MBB_BK / 4);
      const int64_t ge = e0 + eq * 4;
      if (ci < k) {
        const float* g = w + (int64_t)ci * n + ge;
        if (full) {
          rw = *(const float4*)g;
          if (lse) rl = *(const float4*)&lse[ge];
        } else {
          float v[4], lv[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const bool ok = ge + u < n;
            // pad events carry w = 0 (plain) or logw = -inf-ish (lse
            // mode: exp gives 0) so their A fragments vanish
            v[u] = ok ? g[u] : (lse ? -3.0e38f : 0.0f);
            lv[u] = (ok && lse) ? lse[ge + u] : 0.0f;
          }
          rw = *(float4*)v;
          rl = *(float4*)lv;
        }
      } else {
        rw = (float4){lse ? -3.0e38f : 0.0f, lse ? -3.0e38f : 0.0f,
                      lse ? -3.0e38f : 0.0f, lse ? -3.0e38f : 0.0f};
        rl = (float4){0, 0, 0, 0};
      }
    }
  };
  auto write_buf = [&](int buf) {
    __bf16* zhi = zbuf + buf * bufsz_b;
    __bf16* zlo = zhi + zplane;
    float* wt = wbuf + buf * MBB_CPB * MBB_BK;
#pragma unroll
    for (int sq = 0; sq < MBB_NXQ; ++sq) {
      const int q = threadIdx.x + sq * MBB_NT;
      if (q < xq_total) {
        const int di = q / (MBB_BK / 4), ei4 = (q % (MBB_BK / 4)) * 4;
        const float v[4] = {rx[sq].x, rx[sq].y, rx[sq].z, rx[sq].w};
        __bf16 h[4], l[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          h[u] = (__bf16)v[u];
          l[u] = (__bf16)(v[u] - (float)h[u]);
        }
        *(uint2*)(zhi + di * zbr + ei4) = *(uint2*)h;
        *(uint2*)(zlo + di * zbr + ei4) = *(uint2*)l;
      }
    }
    if (threadIdx.x < wq_total) {
      float v[4] = {rw.x, rw.y, rw.z, rw.w};
      if (lse) {
        const float lv[4] = {rl.x, rl.y, rl.z, rl.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = __expf(v[u] - lv[u]);
      }
      *(float4*)(wt + threadIdx.x * 4) = *(float4*)v;
    }
  };

  // constant rows (ones at d, zeros above) in BOTH buffers, once;
  // visibility covered by the first barrier
  for (int bset = 0; bset < 2; ++bset) {
    __bf16* zhi = zbuf + bset * bufsz_b;
    __bf16* zlo = zhi + zplane;
    for (int idx = d * MBB_BK + threadIdx.x; idx < rows * MBB_BK;
         idx += MBB_NT) {
      const int di = idx / MBB_BK, ei = idx % MBB_BK;
      zhi[di * zbr + ei] = (__bf16)(di == d ? 1.0f : 0.0f);
      zlo[di * zbr + ei] = (__bf16)0.0f;
    }
  }
  if (my_tiles > 0) {
    issue_loads(0);
    write_buf(0);
  }
  __syncthreads();

  int cur = 0;
  for (int64_t ti = 0; ti < my_tiles; ++ti) {
    if (ti + 1 < my_tiles) issue_loads(ti + 1);
    const __bf16* zhi = zbuf + cur * bufsz_b;
    const __bf16* zlo = zhi + zplane;
    const float* wt = wbuf + cur * MBB_CPB * MBB_BK;

    if (p_lo < p_hi) {
#pragma unroll
    for (int ch = 0; ch < MBB_BK / 16; ++ch) {
      const int eb = ch * 16 + 8 * g2;
      const float4 wv0 = *(const float4*)(wt + cw * MBB_BK + eb);
      const float4 wv1 = *(const float4*)(wt + cw * MBB_BK + eb + 4);
      const float wv[8] = {wv0.x, wv0.y, wv0.z, wv0.w,
                           wv1.x, wv1.y, wv1.z, wv1.w};
      // the weighted A-side hi/lo split is per (row-tile, chunk) only:
      // hoist it across tile-pairs sharing tr (the quarter assignment
      // keeps same-tr pairs adjacent — ~2x less split VALU at RT2=5)
      int prev_tr = -1;
      bf16x8 a_hi, a_lo;
#pragma unroll
      for (int pp = 0; pp < MBB_PMAX; ++pp) {
        if (p_lo + pp >= p_hi) break;
        const int tr = ptr[pp], tc = ptc[pp];
        if (tr != prev_tr) {
          const bf16x8 zah =
              *(const bf16x8*)(zhi + (tr * 32 + j32) * zbr + eb);
          const bf16x8 zal =
              *(const bf16x8*)(zlo + (tr * 32 + j32) * zbr + eb);
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const float zf = (float)zah[u] + (float)zal[u];
            const float av = wv[u] * zf;
            const __bf16 hi = (__bf16)av;
            a_hi[u] = hi;
            a_lo[u] = (__bf16)(av - (float)hi);
          }
          prev_tr = tr;
        }
        const bf16x8 b_hi = *(const bf16x8*)(zhi + (tc * 32 + j32) * zbr + eb);
        const bf16x8 b_lo = *(const bf16x8*)(zlo + (tc * 32 + j32) * zbr + eb);
        acc[pp] =
            __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, b_hi, acc[pp], 0, 0, 0);
        acc[pp] =
            __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, b_lo, acc[pp], 0, 0, 0);
        acc[pp] =
            __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_lo, b_hi, acc[pp], 0, 0, 0);
      }
    }
    } else if (is_aug && augdim < dp) {
      // T[d, augdim] = sum_e w_e z[augdim, e] from the staged planes
      // (fixed order -> deterministic). b128 row reads: scalar b16
      // reads at the zbr=72 lane stride were 8-way bank-conflicted
      // (36 dwords = 4 mod 32; 12.5% LDSBankConflict on the final PMC);
      // one bf16x8 read covers 8 events at a 2-way worst case. These
      // waves sit well off the pair-waves' critical path either way.
      const __bf16* zh = zhi + augdim * zbr;
      const __bf16* zl = zlo + augdim * zbr;
      const float* wrow = wt + cw * MBB_BK;
      float a0 = 0.0f, a1 = 0.0f;
#pragma unroll
      for (int e8 = 0; e8 < MBB_BK; e8 += 8) {
        const bf16x8 vh = *(const bf16x8*)(zh + e8);
        const bf16x8 vl = *(const bf16x8*)(zl + e8);
#pragma unroll
        for (int u = 0; u < 8; u += 2) {
          a0 = fmaf(wrow[e8 + u], (float)vh[u] + (float)vl[u], a0);
          a1 = fmaf(wrow[e8 + u + 1],
                    (float)vh[u + 1] + (float)vl[u + 1], a1);
        }
      }
      acc_aug += a0 + a1;
    }
    // write the NEXT tile into the other buffer; single barrier per
    // tile (nobody reads that buffer this iteration)
    if (ti + 1 < my_tiles) write_buf(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }

  if (c >= k) return;
  const int p_aug = dp * (dp + 1) / 2;
  float* out = partials + ((int64_t)chunk * k + c) * p_aug;
#pragma unroll
  for (int pp = 0; pp < MBB_PMAX; ++pp) {
    if (p_lo + pp >= p_hi) break;
    const int tr = ptr[pp], tc = ptc[pp];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int gi = tr * 32 + (r & 3) + 8 * (r >> 2) + 4 * g2;
      const int gj = tc * 32 + j32;
      if (gi < dp && gj <= gi)
        out[gi * (gi + 1) / 2 + gj] = acc[pp][r];
    }
  }
  if (is_aug && augdim < dp)
    out[d * (d + 1) / 2 + augdim] = acc_aug;  // packed row d = T[d, :]
}

// ---------------------------------------------------------------------------
// Big-D MFMA E-step logw (31 < D <= 143): q = ||M_c z||^2 with the
// generalized factor layout [K][2][RT*32][KCT*16]. Writes logw to global
// (the separate posteriors kernel normalizes); replaces the VALU
// estep_logw_gen path which is L1/L2-latency-bound at D^2/2 re-reads.
// Grid (ceil(n/256), ceil(K/4)); 4 waves, one cluster per wave, 256 events
// staged transposed in LDS; per (cluster, row-tile) the KCT A-fragment
// pairs live in registers (compile-time KCT => no scratch).
// ---------------------------------------------------------------------------
#define ESB_BE 256

template <int KCT>
__global__ void __launch_bounds__(NT)
estep_logw_big_kernel(const __hip_bfloat16* __restrict__ z,
                      const __hip_bfloat16* __restrict__ mfac,
                      const float* __restrict__ add,
                      float* __restrict__ logw, int d, int k, int64_t n) {
  typedef __attribute__((ext_vector_type(16))) float f32x16;
  const int zrowk = KCT * 16 + 8;  // bf16 slots per transposed event row
  extern __shared__ float lds[];
  __bf16* zs = (__bf16*)lds;       // [ESB_BE][zrowk]

  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int j32 = lane & 31;
  const int g2 = lane >> 5;
  const int64_t e0 = (int64_t)blockIdx.x * ESB_BE;
  const int cnt = (int)min((int64_t)ESB_BE, n - e0);

  // transposed staging with ones-row and zero-pad baked in (branchless
  // for full tiles)
  if (cnt == ESB_BE) {
    for (int idx = threadIdx.x; idx < d * ESB_BE; idx += blockDim.x) {
      const int kk = idx / ESB_BE, ei = idx % ESB_BE;
      zs[ei * zrowk + kk] =
          (__bf16)__bfloat162float(z[(int64_t)kk * n + e0 + ei]);
    }
  } else {
    for (int idx = threadIdx.x; idx < d * ESB_BE; idx += blockDim.x) {
      const int kk = idx / ESB_BE, ei = idx % ESB_BE;
      zs[ei * zrowk + kk] = (__bf16)(
          (ei < cnt) ? __bfloat162float(z[(int64_t)kk * n + e0 + ei]) : 0.0f);
    }
  }
  for (int idx = threadIdx.x; idx < (KCT * 16 - d) * ESB_BE; idx += blockDim.x) {
    const int kk = d + idx / ESB_BE, ei = idx % ESB_BE;
    zs[ei * zrowk + kk] = (__bf16)((kk == d && ei < cnt) ? 1.0f : 0.0f);
  }
  __syncthreads();

  const int c = blockIdx.y * 4 + wave;
  if (c >= k) return;
  const int rt_n = (d + 31) / 32;
  const int cols = KCT * 16;
  const int64_t cells = (int64_t)rt_n * 32 * cols;
  const bf16x8* mf_hi =
      (const bf16x8*)(mfac + (int64_t)c * 2 * cells);
  const bf16x8* mf_lo = mf_hi + cells / 8;
  const float addc = add[c];

  float q[ESB_BE / 32];
#pragma unroll
  for (int t = 0; t < ESB_BE / 32; ++t) q[t] = 0.0f;

  for (int rt = 0; rt < rt_n; ++rt) {
    // A fragments for this row-tile: KCT chunks x hi/lo, in registers
    bf16x8 ah[KCT], al[KCT];
    const int row = rt * 32 + j32;
    const int rowfr = row * (cols / 8);
#pragma unroll
    for (int kc = 0; kc < KCT; ++kc) {
      ah[kc] = mf_hi[rowfr + kc * 2 + g2];
      al[kc] = mf_lo[rowfr + kc * 2 + g2];
    }
#pragma unroll 2
    for (int t = 0; t < ESB_BE / 32; ++t) {
      const __bf16* zrow = zs + (t * 32 + j32) * zrowk;
      f32x16 y = (f32x16)(0.0f);
#pragma unroll
      for (int kc = 0; kc < KCT; ++kc) {
        const bf16x8 b = *(const bf16x8*)(zrow + kc * 16 + 8 * g2);
        y = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[kc], b, y, 0, 0, 0);
        y = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[kc], b, y, 0, 0, 0);
      }
      float s = 0.0f;
#pragma unroll
      for (int r = 0; r < 16; ++r) s = fmaf(y[r], y[r], s);
      q[t] += s;
    }
  }
#pragma unroll
  for (int t = 0; t < ESB_BE / 32; ++t) {
    float s = q[t] + __shfl_xor(q[t], 32, WAVE);
    if (lane < 32) {
      const int64_t e = e0 + t * 32 + j32;
      if (e < n) logw[(int64_t)c * n + e] = -0.5f * s + addc;
    }
  }
}

// ---------------------------------------------------------------------------
// Big-D MFMA E-step v2 (round 2): ONE CLUSTER PER BLOCK with the whole
// factor table [2][RT*32][KCT*16] staged in LDS once and reused across
// MANY 128-event z tiles (tile-strided chunks). v1 re-read every
// cluster's fragments from L2/HBM per 256-event block (~295 GB/iter at
// config 4 by the round-1 ledger); v2's factor traffic is
// K * nchunk * |M_c| ~ 0.4 GB. 16 waves split the (row-tile, event-32)
// work; per-tile partials combine through LDS (fixed order:
// deterministic).
// ---------------------------------------------------------------------------
#define ESB2_NT 1024

template <int KCT, int BE>
__global__ void __launch_bounds__(ESB2_NT)
estep_logw_big2_kernel(const __hip_bfloat16* __restrict__ z,
                       const __hip_bfloat16* __restrict__ mfac,
                       const float* __restrict__ add,
                       float* __restrict__ logw, int d, int k, int64_t n,
                       int nchunk) {
  typedef __attribute__((ext_vector_type(16))) float f32x16;
  constexpr int COLS = KCT * 16;
  constexpr int AROW = COLS + 8;   // bf16 row stride (16-lane b128 groups
                                   // land on distinct banks: 76 = 12 mod 64)
  extern __shared__ float lds[];
  const int rt_n = (d + 31) / 32;
  const int rows = rt_n * 32;
  __bf16* ah = (__bf16*)lds;             // [rows][AROW]
  __bf16* al = ah + rows * AROW;
  __bf16* zs = al + rows * AROW;         // [BE][AROW]
  float* qpart = (float*)(zs + BE * AROW);  // [rt_n][BE]

  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int j32 = lane & 31;
  const int g2 = lane >> 5;
  const int c = blockIdx.y;
  const int chunk = blockIdx.x;
  const float addc = add[c];

  // stage this cluster's whole factor table (hi+lo planes) into padded
  // LDS rows; vectorized 8-bf16 copies, coalesced over the row-major
  // global layout [c][2][rows][cols]
  {
    const uint4* src_h =
        (const uint4*)(mfac + (int64_t)c * 2 * rows * COLS);
    const uint4* src_l = src_h + rows * COLS / 8;
    for (int q8 = threadIdx.x; q8 < rows * COLS / 8;
         q8 += (int)blockDim.x) {
      const int row = q8 / (COLS / 8), col8 = q8 % (COLS / 8);
      *(uint4*)(ah + row * AROW + col8 * 8) = src_h[q8];
      *(uint4*)(al + row * AROW + col8 * 8) = src_l[q8];
    }
  }

  const int64_t tiles = (n + BE - 1) / BE;
  for (int64_t tile = chunk; tile < tiles; tile += nchunk) {
    const int64_t e0 = tile * BE;
    const int cnt = (int)min((int64_t)BE, n - e0);
    __syncthreads();
    // transposed z staging: each thread gathers 4 consecutive k-slots of
    // one event (4 coalesced-by-wave global reads) and writes ONE 8-byte
    // ds_write_b64 — scalar b16 transpose writes were a 4-way bank
    // conflict (stride-AROW lanes 8 apart collide mod 32 for any 16B
    // row stride; 20% LDSBankConflict measured)
    {
      const int kq_total = ((d + 3) / 4) * BE;
      for (int idx = threadIdx.x; idx < kq_total;
           idx += (int)blockDim.x) {
        const int kk0 = (idx / BE) * 4, ei = idx % BE;
        __bf16 v[4];
        // kk0 is wave-uniform (BE >= WAVE): full quads take the
        // branchless path — per-element ternaries around loads would
        // serialize them behind vmcnt(0) (guide trap 4c, measured -15%)
        if (cnt == BE && kk0 + 3 < d) {
          const __hip_bfloat16* zp = z + (int64_t)kk0 * n + e0 + ei;
#pragma unroll
          for (int u = 0; u < 4; ++u) v[u] = (__bf16)(zp[(int64_t)u * n]);
        } else {
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int kk = kk0 + u;
            float vf = 0.0f;
            if (ei < cnt) {
              if (kk < d) vf = __bfloat162float(z[(int64_t)kk * n + e0 + ei]);
              else if (kk == d) vf = 1.0f;  // ones row inside the quad
            }
            v[u] = (__bf16)vf;
          }
        }
        *(uint2*)(zs + ei * AROW + kk0) = *(uint2*)v;
      }
      const int kpad0 = ((d + 3) / 4) * 4;
      for (int idx = threadIdx.x; idx < (COLS - kpad0) * BE;
           idx += (int)blockDim.x) {
        const int kk = kpad0 + idx / BE, ei = idx % BE;
        // d is only >= kpad0 when d % 4 == 0: the ones row then lives here
        zs[ei * AROW + kk] =
            (__bf16)((kk == d && ei < cnt) ? 1.0f : 0.0f);
      }
    }
    __syncthreads();

    // (row-tile, event-32-tile) tasks. Task cost falls with rt (the
    // zero-tile skip below), so enumerate tasks rt-DESCENDING and deal
    // them to waves in a zigzag: each wave's summed cost is near-uniform
    // and the post-loop barrier waits for the least-idle wave.
    const int etiles = BE / 32;
    const int T = rt_n * etiles;
    const int W = (int)(blockDim.x / WAVE);
    const int kaug = d >> 4;  // column-tile holding the augmented column
    for (int s2 = 0;; ++s2) {
      const int idx =
          (s2 & 1) ? ((s2 + 1) * W - 1 - wave) : (s2 * W + wave);
      if (idx >= T) break;
      const int rt = rt_n - 1 - idx / etiles;
      const int t = idx % etiles;
      // F = [chol(R)^-1 | -F mu] is lower-triangular + one augmented
      // column: row-tile rt's live column-tiles are 0..(64rt+31)/16 and
      // the augmented tile; the rest of the padded table is zeros
      // (emit_mfac) and MFMA accumulation of zeros is bitwise a no-op,
      // so skipping those tiles is exact
      const int kcmax = min(KCT - 1, 2 * rt + 1);
      const __bf16* arow = ah + (rt * 32 + j32) * AROW;
      const __bf16* lrow = al + (rt * 32 + j32) * AROW;
      const __bf16* zrow = zs + (t * 32 + j32) * AROW;
      f32x16 y = (f32x16)(0.0f);
#pragma unroll
      for (int kc = 0; kc < KCT; ++kc) {
        if (kc > kcmax && kc != kaug) continue;
        const bf16x8 b = *(const bf16x8*)(zrow + kc * 16 + 8 * g2);
        const bf16x8 fa = *(const bf16x8*)(arow + kc * 16 + 8 * g2);
        const bf16x8 fl = *(const bf16x8*)(lrow + kc * 16 + 8 * g2);
        y = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, b, y, 0, 0, 0);
        y = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fl, b, y, 0, 0, 0);
      }
      float s = 0.0f;
#pragma unroll
      for (int r = 0; r < 16; ++r) s = fmaf(y[r], y[r], s);
      s += __shfl_xor(s, 32, WAVE);
      if (lane < 32) qpart[rt * BE + t * 32 + j32] = s;
    }
    __syncthreads();
    // combine row-tile partials (fixed order) and write logw
    if (threadIdx.x < BE && threadIdx.x < cnt) {
      const int e = threadIdx.x;
      float q = qpart[e];
      for (int rt = 1; rt < rt_n; ++rt) q += qpart[rt * BE + e];
      logw[(int64_t)c * n + e0 + e] = -0.5f * q + addc;
    }
  }
}

// ---------------------------------------------------------------------------
// Exact-fp32 big-D MFMA E-step logw (31 < D <= 143): the fp32 counterpart
// of estep_logw_big_kernel on v_mfma_f32_32x32x2_f32, consuming the f32
// factor plane [K][RT*32][KCT*16]. Fills the fp32 + D > 31 quadrant that
// previously fell back to the latency-bound VALU estep_logw_gen path
// (reference estep1 covers its full D range at fp32 within its broken
// D <= 32 cap, gaussian_kernel.cu:383). 128-event tiles (f32 z LDS).
// ---------------------------------------------------------------------------
#define ESBF_BE 128

template <int KCT>
__global__ void __launch_bounds__(NT)
estep_logw_big_f32_kernel(const float* __restrict__ z,
                          const float* __restrict__ mfac32,
                          const float* __restrict__ add,
                          float* __restrict__ logw, int d, int k, int64_t n) {
  typedef __attribute__((ext_vector_type(16))) float f32x16;
  constexpr int ZR = KCT * 16 + 4;  // f32 slots per transposed event row
  extern __shared__ float lds[];
  float* zs = lds;                  // [ESBF_BE][ZR]

  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int j32 = lane & 31;
  const int g2 = lane >> 5;
  const int64_t e0 = (int64_t)blockIdx.x * ESBF_BE;
  const int cnt = (int)min((int64_t)ESBF_BE, n - e0);

  if (cnt == ESBF_BE) {
    for (int idx = threadIdx.x; idx < d * ESBF_BE; idx += blockDim.x) {
      const int kk = idx / ESBF_BE, ei = idx % ESBF_BE;
      zs[ei * ZR + kk] = z[(int64_t)kk * n + e0 + ei];
    }
  } else {
    for (int idx = threadIdx.x; idx < d * ESBF_BE; idx += blockDim.x) {
      const int kk = idx / ESBF_BE, ei = idx % ESBF_BE;
      zs[ei * ZR + kk] = (ei < cnt) ? z[(int64_t)kk * n + e0 + ei] : 0.0f;
    }
  }
  for (int idx = threadIdx.x; idx < (KCT * 16 - d) * ESBF_BE;
       idx += blockDim.x) {
    const int kk = d + idx / ESBF_BE, ei = idx % ESBF_BE;
    zs[ei * ZR + kk] = (kk == d && ei < cnt) ? 1.0f : 0.0f;
  }
  __syncthreads();

  const int c = blockIdx.y * 4 + wave;
  if (c >= k) return;
  const int rt_n = (d + 31) / 32;
  const int cols = KCT * 16;
  const float* mf = mfac32 + (int64_t)c * rt_n * 32 * cols;
  const float addc = add[c];

  float q[ESBF_BE / 32];
#pragma unroll
  for (int t = 0; t < ESBF_BE / 32; ++t) q[t] = 0.0f;

  for (int rt = 0; rt < rt_n; ++rt) {
    // A values for this row-tile: lane j32 holds row rt*32+j32, k-slots
    // 2*ch + g2 (v_mfma_f32_32x32x2_f32 operand map, guide §3).
    // F is lower-triangular + one augmented column: k-chunks past
    // chmax hold only zeros (emit_mfac pads), except the augmented
    // chunk — skipping them is exact (acc + 0*b is a bitwise no-op)
    // and cuts ~43% of the rate-limiting f32 MFMAs at D=128. rt is
    // wave-uniform, so the branches do not diverge.
    const int chmax = min(KCT * 8 - 1, 16 * rt + 15);
    const int chaug = d >> 1;  // k-chunk holding the augmented column
    float a[KCT * 8];
    const float* arow = mf + (rt * 32 + j32) * cols;
#pragma unroll
    for (int ch = 0; ch < KCT * 8; ++ch)
      a[ch] = (ch <= chmax || ch == chaug) ? arow[2 * ch + g2] : 0.0f;
#pragma unroll
    for (int t = 0; t < ESBF_BE / 32; ++t) {
      const float* zrow = zs + (t * 32 + j32) * ZR;
      f32x16 y = (f32x16)(0.0f);
#pragma unroll
      for (int ch = 0; ch < KCT * 8; ++ch) {
        if (ch > chmax && ch != chaug) continue;
        const float b = zrow[2 * ch + g2];
        y = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ch], b, y, 0, 0, 0);
      }
      float s = 0.0f;
#pragma unroll
      for (int r = 0; r < 16; ++r) s = fmaf(y[r], y[r], s);
      q[t] += s;
    }
  }
#pragma unroll
  for (int t = 0; t < ESBF_BE / 32; ++t) {
    float s = q[t] + __shfl_xor(q[t], 32, WAVE);
    if (lane < 32) {
      const int64_t e = e0 + t * 32 + j32;
      if (e < n) logw[(int64_t)c * n + e] = -0.5f * s + addc;
    }
  }
}

// Standalone factor emission from the covariance R (diag-only constants
// and the post-merge/resume refresh path).
__global__ void __launch_bounds__(NT)
emit_mfac_from_r_kernel(const float* __restrict__ r,
                        const float* __restrict__ means,
                        __hip_bfloat16* __restrict__ mfac,
                        float* __restrict__ mfac32, int d,
                        const float* __restrict__ pi,
                        float* __restrict__ constant,
                        float* __restrict__ add) {
  extern __shared__ float buf[];
  emit_mfac(buf, buf + d * (d | 1), r, means, mfac, mfac32,
            blockIdx.x, d, pi, constant, add);
}

// DIAG_ONLY constants (gaussian_kernel.cu:215-223)
__global__ void __launch_bounds__(NT)
constants_diag_kernel(const float* __restrict__ r, float* __restrict__ rinv,
                      float* __restrict__ logdet, int d) {
  const int c = blockIdx.x;
  const float* rc = r + (int64_t)c * d * d;
  float* oc = rinv + (int64_t)c * d * d;
  __shared__ float det;
  if (threadIdx.x == 0) {
    float dd = 1.0f;
    for (int i = 0; i < d; ++i) dd *= rc[i * d + i];
    det = __logf(dd);
    logdet[c] = det;
  }
  for (int t = threadIdx.x; t < d * d; t += NT) {
    const int i = t / d, j = t % d;
    oc[t] = (i == j) ? 1.0f / rc[t] : 0.0f;
  }
}

// Layout probe: D = A(16x32) @ B(32x16) in bf16 via one MFMA.
__global__ void mfma_probe_kernel(const __hip_bfloat16* __restrict__ a,
                                  const __hip_bfloat16* __restrict__ b,
                                  float* __restrict__ c) {
  const int lane = threadIdx.x & (WAVE - 1);
  bf16x8 av, bv;
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int kx = mfma_b16_k(lane >> 4, u);
    av[u] = (__bf16)__bfloat162float(a[(lane & 15) * 32 + kx]);
    bv[u] = (__bf16)__bfloat162float(b[kx * 16 + (lane & 15)]);
  }
  f32x4 acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
      av, bv, (f32x4){0, 0, 0, 0}, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 4; ++r)
    c[((lane >> 4) * 4 + r) * 16 + (lane & 15)] = acc[r];
}

// Layout probe for the 32x32x16 shape: D = A(32x16) @ B(16x32).
__global__ void mfma_probe32_kernel(const __hip_bfloat16* __restrict__ a,
                                    const __hip_bfloat16* __restrict__ b,
                                    float* __restrict__ c) {
  const int lane = threadIdx.x & (WAVE - 1);
  bf16x8 av, bv;
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int kx = 8 * (lane >> 5) + u;
    av[u] = (__bf16)__bfloat162float(a[(lane & 31) * 16 + kx]);
    bv[u] = (__bf16)__bfloat162float(b[kx * 32 + (lane & 31)]);
  }
  f32x16_t acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
      av, bv, (f32x16_t)(0.0f), 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 16; ++r)
    c[((r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * 32 + (lane & 31)] = acc[r];
}

}  // namespace gmm
