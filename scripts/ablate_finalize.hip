// Phase split of mstep_finalize_emit_kernel (K=64, D=24 by default).
// A copy of the kernel and of emit_mfac from ops/hip/gmm_kernels.hip with a
// clock read by thread 0 at every phase boundary; keep it in step with the
// original when that changes (helpers are taken from the original file).
// Prints, averaged over the blocks of the last launch, the share of each
// phase, next to the event-timed launch of the real kernel and of the copy.
//   hipcc -O3 --offload-arch=gfx950 scripts/ablate_finalize.hip \
//       -o scripts/ablate_finalize && scripts/ablate_finalize [K] [D]
#include "../cuda_gmm_mpi_amd/ops/hip/gmm_kernels.hip"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x)                                                            \
  do {                                                                   \
    hipError_t e_ = (x);                                                 \
    if (e_ != hipSuccess) {                                              \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));            \
      exit(1);                                                           \
    }                                                                    \
  } while (0)

namespace gmm {

constexpr int NSTAMP = 9;
static const char* kPhase[NSTAMP - 1] = {
    "pi + means", "R", "Cholesky", "ln det + constants", "inverse",
    "u0", "emission", "(tail barrier)"};
// D <= 32: the chain runs first, as a whole, on wave 0
static const char* kPhaseRegs[NSTAMP - 1] = {
    "pi + means", "R", "Cholesky", "inverse", "barrier, ln det + c.",
    "u0", "emission", "(tail barrier)"};

#define STAMP(n)                                                         \
  do {                                                                   \
    if (threadIdx.x == 0) stamps[blockIdx.x * NSTAMP + (n)] = clock64(); \
  } while (0)

// chain_regs with a stamp between its halves
template <int DM>
__device__ __forceinline__ void chain_regs_stamped(float* a, float* o, int d,
                                                   int ldp,
                                                   long long* stamps) {
  chol_regs<DM>(a, d, ldp);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  STAMP(3);
  inv_regs<DM>(a, o, d, ldp);
}

__global__ void __launch_bounds__(NT)
finalize_emit_stamped(const float* __restrict__ packed,
                      const float* __restrict__ avgvar, int world,
                      float* __restrict__ n_out, float* __restrict__ means,
                      float* __restrict__ r_out, float* __restrict__ pi,
                      float* __restrict__ constant, float* __restrict__ add,
                      __hip_bfloat16* __restrict__ mfac,
                      float* __restrict__ mfac32, int d, int k,
                      long long* __restrict__ stamps) {
  extern __shared__ float lds[];
  const int ldp = d | 1;
  float* a = lds;
  float* o = a + d * ldp;
  float* mu = o + d * ldp;
  const int c = blockIdx.x;
  const int dp = d + 1;
  const int pp = dp * (dp + 1) / 2;
  const int p = d * (d + 1) / 2;
  const float* row = packed + (int64_t)c * pp;
  STAMP(0);
  const float n_c = row[pp - 1];
  const bool ge1 = n_c >= 1.0f;
  const bool gt05 = n_c > 0.5f;

  if (threadIdx.x < WAVE) {
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
  STAMP(1);
  const float reg = world * avgvar[c];
  for (int t = threadIdx.x; t < p; t += NT) {
    int i, j;
    tri_row_col(t, &i, &j);
    float cov = ge1 ? fmaf(-(n_c * mu[i]), mu[j], row[t]) : 0.0f;
    if (i == j) cov += reg;
    float rv;
    if (gt05) rv = cov / n_c;
    else rv = (i == j) ? 1.0f : 0.0f;
    r_out[((int64_t)c * d + i) * d + j] = rv;
    if (i != j) r_out[((int64_t)c * d + j) * d + i] = rv;
    a[i * ldp + j] = rv;
  }
  __syncthreads();
  STAMP(2);

  // ---- emit_mfac, r_global == nullptr ----
  const int tid = threadIdx.x;
  float* u0 = o + d * ldp;
  const bool regs = d <= 32;
  if (regs) {
    // wave 0 (thread 0's wave) runs both halves of the chain in registers;
    // stamps 3 and 4 are taken in emit_mfac's order for this path: Cholesky,
    // inverse, then the barrier with ln det and the constants
    if (tid < WAVE) {
      if (d <= 8) chain_regs_stamped<8>(a, o, d, ldp, stamps);
      else if (d <= 16) chain_regs_stamped<16>(a, o, d, ldp, stamps);
      else if (d <= 24) chain_regs_stamped<24>(a, o, d, ldp, stamps);
      else chain_regs_stamped<32>(a, o, d, ldp, stamps);
      STAMP(4);
    }
    __syncthreads();
  }
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
  if (!regs) STAMP(3);
  {
    __shared__ float wsum_e[NT / WAVE];
    const int nw = (blockDim.x + WAVE - 1) / WAVE;
    float acc = 0.0f;
    for (int i = tid; i < d; i += blockDim.x) acc += __logf(a[i * ldp + i]);
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
      add[c] = cst + __logf(pi[c]);
    }
    __syncthreads();
  }
  if (!regs) STAMP(4);
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
  STAMP(5);
  if (tid < d) {
    const float* fi = o + tid * ldp;
    float s = 0.0f;
#pragma unroll 8
    for (int j = 0; j <= tid; ++j) s = fmaf(fi[j], means[c * d + j], s);
    u0[tid] = -s;
  }
  __syncthreads();
  STAMP(6);
  const int rows = mfac_rows(d);
  const int cols = mfac_kct(d) * 16;
  const int cells = rows * cols;
  const int cpr = cols >> 3;
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
  STAMP(7);
  __syncthreads();
  STAMP(8);
}

}  // namespace gmm

int main(int argc, char** argv) {
  const int k = argc > 1 ? atoi(argv[1]) : 64;
  const int d = argc > 2 ? atoi(argv[2]) : 24;
  if (k < 1 || d < 1 || d > 142) {
    fprintf(stderr, "need K >= 1 and 1 <= D <= 142\n");
    return 1;
  }
  const int dp = d + 1, pp = dp * (dp + 1) / 2, nev = 40 * d + 200;
  // moments of random data under random soft weights: R positive definite
  std::vector<double> x((size_t)nev * dp), acc((size_t)k * pp, 0.0);
  std::vector<float> w(k);
  unsigned s = 12345u;
  auto rnd = [&]() {
    s = s * 1664525u + 1013904223u;
    return (s >> 8) * (1.0 / 16777216.0);
  };
  for (int e = 0; e < nev; ++e) {
    for (int i = 0; i < d; ++i)
      x[(size_t)e * dp + i] = 3.0 * (rnd() + rnd() + rnd() - 1.5);
    x[(size_t)e * dp + d] = 1.0;
    double tot = 0.0;
    for (int c = 0; c < k; ++c) tot += (w[c] = (float)(rnd() + 0.01));
    for (int c = 0; c < k; ++c) {
      const double wc = w[c] / tot;
      double* row = &acc[(size_t)c * pp];
      int t = 0;
      for (int i = 0; i < dp; ++i)
        for (int j = 0; j <= i; ++j)
          row[t++] += wc * x[(size_t)e * dp + i] * x[(size_t)e * dp + j];
    }
  }
  std::vector<float> packed(acc.begin(), acc.end()), avgvar(k, 0.02f);
  const int rows = gmm::mfac_rows(d), cols = gmm::mfac_kct(d) * 16;
  float *dpk, *dav, *dn, *dmu, *dr, *dpi, *dc, *dadd, *dm32;
  __hip_bfloat16* dm;
  long long* dst;
  CK(hipMalloc(&dpk, packed.size() * 4));
  CK(hipMalloc(&dav, k * 4));
  CK(hipMalloc(&dn, k * 4));
  CK(hipMalloc(&dmu, (size_t)k * d * 4));
  CK(hipMalloc(&dr, (size_t)k * d * d * 4));
  CK(hipMalloc(&dpi, k * 4));
  CK(hipMalloc(&dc, k * 4));
  CK(hipMalloc(&dadd, k * 4));
  CK(hipMalloc(&dm, (size_t)k * 2 * rows * cols * 2));
  CK(hipMalloc(&dm32, (size_t)k * rows * cols * 4));
  CK(hipMalloc(&dst, (size_t)k * gmm::NSTAMP * 8));
  CK(hipMemcpy(dpk, packed.data(), packed.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(dav, avgvar.data(), k * 4, hipMemcpyHostToDevice));
  const size_t lds = sizeof(float) * (2 * (size_t)d * (d | 1) + d);
  if (lds > 64 * 1024) {
    CK(hipFuncSetAttribute(
        reinterpret_cast<const void*>(&gmm::mstep_finalize_emit_kernel),
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    CK(hipFuncSetAttribute(
        reinterpret_cast<const void*>(&gmm::finalize_emit_stamped),
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  const int warm = 300, reps = 200;
  for (int variant = 0; variant < 2; ++variant) {
    float ms = 0.0f;
    for (int it = 0; it < warm + reps; ++it) {
      if (it == warm) CK(hipEventRecord(e0));
      if (variant == 0)
        hipLaunchKernelGGL(gmm::mstep_finalize_emit_kernel, dim3(k), dim3(NT),
                           lds, 0, dpk, dav, 1, dn, dmu, dr, dpi, dc, dadd,
                           dm, nullptr, d, k);
      else
        hipLaunchKernelGGL(gmm::finalize_emit_stamped, dim3(k), dim3(NT), lds,
                           0, dpk, dav, 1, dn, dmu, dr, dpi, dc, dadd, dm,
                           nullptr, d, k, dst);
    }
    CK(hipEventRecord(e1));
    CK(hipDeviceSynchronize());
    CK(hipEventElapsedTime(&ms, e0, e1));
    printf("%s: %.2f us per launch (back to back, K=%d D=%d)\n",
           variant ? "stamped copy" : "kernel", ms * 1e3 / reps, k, d);
  }
  std::vector<long long> st((size_t)k * gmm::NSTAMP);
  CK(hipMemcpy(st.data(), dst, st.size() * 8, hipMemcpyDeviceToHost));
  double tot = 0.0, ph[gmm::NSTAMP - 1] = {};
  for (int c = 0; c < k; ++c) {
    const long long* b = &st[(size_t)c * gmm::NSTAMP];
    for (int q = 0; q + 1 < gmm::NSTAMP; ++q) ph[q] += double(b[q + 1] - b[q]);
    tot += double(b[gmm::NSTAMP - 1] - b[0]);
  }
  printf("in-kernel clock, mean over %d blocks: %.0f ticks\n", k, tot / k);
  for (int q = 0; q + 1 < gmm::NSTAMP; ++q)
    printf("  %-20s %8.0f ticks  %5.1f %%\n",
           (d <= 32 ? gmm::kPhaseRegs : gmm::kPhase)[q], ph[q] / k,
           100.0 * ph[q] / tot);
  float cst0 = 0.0f;
  CK(hipMemcpy(&cst0, dc, 4, hipMemcpyDeviceToHost));
  printf("constant[0] = %g\n", cst0);
  return 0;
}
