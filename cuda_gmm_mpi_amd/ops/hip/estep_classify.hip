// Classify kernels (D <= 31, any K): score new events against a fitted
// mixture and write 12 bytes per event, no [K, N] array.
//
//   estep_classify_kernel      bf16  256 events  label / lse / pmax
//   estep_classify_f32_kernel  f32   256 events  label / lse / pmax
//
// They are the online-softmax kernels of estep_fused.hip with the two ends
// changed, bodies written out per kernel as that file's header explains.
//  - Staging reads the caller's own layout: x is EVENT-major fp32 [N, D], so
//    a block's slab is one contiguous run of 256 d floats. Consecutive
//    threads walk consecutive floats (fully coalesced), carry (event, k)
//    incrementally, subtract the centre in fp32 and, in the bf16 kernel,
//    round to nearest even: the value the engine stages with
//    (shard - center).T.to(bfloat16). Ones row, zero pad and the partial
//    last block are as in estep_fused_kernel.
//  - The cluster loop and the cross-wave combine are copied expression for
//    expression, so logw and lse are bitwise what estep_fused /
//    estep_fused_f32 give for the same staged z. Next to its running max
//    each wave keeps the cluster that set it: a wave visits its clusters in
//    ascending order and updates on strict >, so that is its lowest argmax,
//    and the combine takes the smallest index among the waves that hold the
//    global max: the first argmax over all K. The index plane starts at
//    min(wave, k - 1), so a wave without clusters (K < 4) or an event whose
//    log-weights are all NaN still gives a label in [0, K).
//  - Each thread owns one event in the combine and writes label, lse and
//    pmax = __expf(m - lse) straight to global memory; there is no
//    likelihood partial (the host sums lse in float64).
// LDS: zs [EST_BE][ZROW], then m / s / index state [nwaves][EST_BE] each
// (32.0 KB bf16, 45.0 KB f32; K-independent), plus the 32-float centre.
#pragma once

#include "estep_fused.hip"

namespace gmm {

template <typename Fac>
constexpr size_t cls_lds_bytes() {
  return sizeof(float) *
         (z_tile_floats<Fac, EST_BE>() + 3 * (NT / WAVE) * EST_BE);
}

__global__ void __launch_bounds__(NT)
estep_classify_kernel(const float* __restrict__ x,       // [N][d] fp32
                      const float* __restrict__ center,  // [d]
                      const __hip_bfloat16* __restrict__ mfac,  // [K][2][32][32]
                      const float* __restrict__ add,            // const + ln pi
                      int* __restrict__ label_out,
                      float* __restrict__ lse_out,
                      float* __restrict__ pmax_out, int d, int k, int64_t n) {
  extern __shared__ float lds[];
  __hip_bfloat16* zs = (__hip_bfloat16*)lds;
  float* mstate = lds + (EST_BE * FacB16::ZROW) / 2;   // [nwaves][EST_BE]
  float* sstate = mstate + (NT / WAVE) * EST_BE;       // [nwaves][EST_BE]
  int* istate = (int*)(sstate + (NT / WAVE) * EST_BE); // [nwaves][EST_BE]
  __shared__ float cen[32];

  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t e0 = (int64_t)blockIdx.x * EST_BE;
  const int cnt = (int)min((int64_t)EST_BE, n - e0);
  const bool full = cnt == EST_BE;

  if (threadIdx.x < 32)
    cen[threadIdx.x] = (threadIdx.x < d) ? center[threadIdx.x] : 0.0f;
  __syncthreads();

  __bf16* zsb = (__bf16*)zs;
  {
    // slab walk: element idx of the slab is (event idx / d, k idx % d);
    // a step of NT elements moves that pair by (NT / d, NT % d)
    const float* slab = x + e0 * d;
    const int qs = NT / d, rs = NT % d;
    int ei = threadIdx.x / d, kk = threadIdx.x % d;
    if (full) {
      for (int idx = threadIdx.x; idx < d * EST_BE; idx += NT) {
        zsb[ei * FacB16::ZROW + kk] = (__bf16)(slab[idx] - cen[kk]);
        ei += qs;
        kk += rs;
        if (kk >= d) {
          kk -= d;
          ++ei;
        }
      }
    } else {
      const int live = cnt * d;  // floats of the slab that exist
      for (int idx = threadIdx.x; idx < d * EST_BE; idx += NT) {
        zsb[ei * FacB16::ZROW + kk] =
            (__bf16)((idx < live) ? slab[idx] - cen[kk] : 0.0f);
        ei += qs;
        kk += rs;
        if (kk >= d) {
          kk -= d;
          ++ei;
        }
      }
    }
  }
  for (int idx = threadIdx.x; idx < (32 - d) * EST_BE; idx += blockDim.x) {
    const int kk = d + idx / EST_BE, ei = idx % EST_BE;
    zsb[ei * FacB16::ZROW + kk] =
        (__bf16)((kk == d && ei < cnt) ? 1.0f : 0.0f);
  }
  for (int i = threadIdx.x; i < (NT / WAVE) * EST_BE; i += blockDim.x) {
    mstate[i] = -3.0e38f;
    sstate[i] = 0.0f;
    istate[i] = min(i / EST_BE, k - 1);
  }
  __syncthreads();

  // cluster loop [W]; per 16-deep chunk A lane l holds kk = 8*(l>>5)+u
  const int j32 = lane & 31;
  const int g2 = lane >> 5;
  const bf16x8* mf = (const bf16x8*)mfac;  // rows of 32 bf16 = 4 frags each
  const int fq0 = g2;      // chunk 0 covers k [0,16): slots {0,1}
  const int fq1 = 2 + g2;  // chunk 1 covers k [16,32): slots {2,3}
  const int nwaves = NT / WAVE;
  float* mrow = mstate + wave * EST_BE;
  float* srow = sstate + wave * EST_BE;
  int* irow = istate + wave * EST_BE;

  bf16x8 nx_h0, nx_l0, nx_h1, nx_l1;
  float nx_add;
  auto load_a = [&](int c) {
    const int64_t base = ((int64_t)c * 2) * 32 * 4;  // in bf16x8 units
    nx_h0 = mf[base + j32 * 4 + fq0];
    nx_l0 = mf[base + 32 * 4 + j32 * 4 + fq0];
    nx_h1 = mf[base + j32 * 4 + fq1];
    nx_l1 = mf[base + 32 * 4 + j32 * 4 + fq1];
    nx_add = add[c];
  };
  if (wave < k) load_a(wave);

  for (int c = wave; c < k; c += nwaves) {
    const bf16x8 a_h0 = nx_h0, a_l0 = nx_l0, a_h1 = nx_h1, a_l1 = nx_l1;
    const float addc = nx_add;
    if (c + nwaves < k) load_a(c + nwaves);
#pragma unroll
    for (int t = 0; t < EST_BE / 32; ++t) {
      // B fragments: contiguous 16 B of the transposed z row
      const bf16x8 b0 =
          *(const bf16x8*)(zs + (t * 32 + j32) * FacB16::ZROW + 8 * g2);
      const bf16x8 b1 =
          *(const bf16x8*)(zs + (t * 32 + j32) * FacB16::ZROW + 16 + 8 * g2);
      f32x16_t y = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
          a_h0, b0, (f32x16_t)(0.0f), 0, 0, 0);
      y = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_h1, b1, y, 0, 0, 0);
      y = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_l0, b0, y, 0, 0, 0);
      y = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_l1, b1, y, 0, 0, 0);
      float s = 0.0f;
#pragma unroll
      for (int r = 0; r < 16; ++r) s = fmaf(y[r], y[r], s);
      // the 32 Y rows live across the two lane halves: one cross-half sum
      s += __shfl_xor(s, 32, WAVE);
      if (lane < 32) {
        const int e = t * 32 + j32;
        const float lwv = -0.5f * s + addc;
        // lane j32 owns event e exclusively within this wave, so the
        // state update is race-free
        const float mo = mrow[e];
        if (lwv > mo) {
          srow[e] = srow[e] * __expf(mo - lwv) + 1.0f;
          mrow[e] = lwv;
          irow[e] = c;
        } else {
          srow[e] += __expf(lwv - mo);
        }
      }
    }
  }
  __syncthreads();

  // combine the per-wave (m, s, index) into the event's outputs
  // (EST_BE == NT: each thread owns one event)
  {
    const int e = threadIdx.x;
    float m = mstate[e];
#pragma unroll
    for (int wv = 1; wv < nwaves; ++wv)
      m = fmaxf(m, mstate[wv * EST_BE + e]);
    float ssum = 0.0f;
    {
      // the training kernels compile this sum to separately rounded
      // multiplies and adds (their fixtures pin that); here the compiler
      // would contract it to an fma chain, so contraction is switched off
#pragma clang fp contract(off)
#pragma unroll
      for (int wv = 0; wv < nwaves; ++wv)
        ssum += sstate[wv * EST_BE + e] * __expf(mstate[wv * EST_BE + e] - m);
    }
    const float lse = m + __logf(ssum);
    int best = k - 1;  // every stored index is <= k - 1
#pragma unroll
    for (int wv = 0; wv < nwaves; ++wv)
      if (mstate[wv * EST_BE + e] == m)
        best = min(best, istate[wv * EST_BE + e]);
    if (e < cnt) {
      label_out[e0 + e] = best;
      lse_out[e0 + e] = lse;
      pmax_out[e0 + e] = __expf(m - lse);
    }
  }
}

__global__ void __launch_bounds__(NT)
estep_classify_f32_kernel(const float* __restrict__ x,       // [N][d] fp32
                          const float* __restrict__ center,  // [d]
                          const float* __restrict__ mfac32,  // [K][32][32]
                          const float* __restrict__ add,
                          int* __restrict__ label_out,
                          float* __restrict__ lse_out,
                          float* __restrict__ pmax_out, int d, int k,
                          int64_t n) {
  constexpr int ZR = FacF32::ZROW;
  extern __shared__ float lds[];
  float* zs = lds;                                     // [EST_BE][ZR]
  float* mstate = lds + EST_BE * ZR;                   // [nwaves][EST_BE]
  float* sstate = mstate + (NT / WAVE) * EST_BE;       // [nwaves][EST_BE]
  int* istate = (int*)(sstate + (NT / WAVE) * EST_BE); // [nwaves][EST_BE]
  __shared__ float cen[32];

  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int j32 = lane & 31;
  const int g2 = lane >> 5;
  const int64_t e0 = (int64_t)blockIdx.x * EST_BE;
  const int cnt = (int)min((int64_t)EST_BE, n - e0);
  const bool full = cnt == EST_BE;

  if (threadIdx.x < 32)
    cen[threadIdx.x] = (threadIdx.x < d) ? center[threadIdx.x] : 0.0f;
  __syncthreads();

  {
    // slab walk as in estep_classify_kernel
    const float* slab = x + e0 * d;
    const int qs = NT / d, rs = NT % d;
    int ei = threadIdx.x / d, kk = threadIdx.x % d;
    if (full) {
      for (int idx = threadIdx.x; idx < d * EST_BE; idx += NT) {
        zs[ei * ZR + kk] = slab[idx] - cen[kk];
        ei += qs;
        kk += rs;
        if (kk >= d) {
          kk -= d;
          ++ei;
        }
      }
    } else {
      const int live = cnt * d;  // floats of the slab that exist
      for (int idx = threadIdx.x; idx < d * EST_BE; idx += NT) {
        zs[ei * ZR + kk] = (idx < live) ? slab[idx] - cen[kk] : 0.0f;
        ei += qs;
        kk += rs;
        if (kk >= d) {
          kk -= d;
          ++ei;
        }
      }
    }
  }
  for (int idx = threadIdx.x; idx < (32 - d) * EST_BE; idx += blockDim.x) {
    const int kk = d + idx / EST_BE, ei = idx % EST_BE;
    zs[ei * ZR + kk] = (kk == d && ei < cnt) ? 1.0f : 0.0f;
  }
  for (int i = threadIdx.x; i < (NT / WAVE) * EST_BE; i += blockDim.x) {
    mstate[i] = -3.0e38f;
    sstate[i] = 0.0f;
    istate[i] = min(i / EST_BE, k - 1);
  }
  __syncthreads();

  const int nwaves = NT / WAVE;
  float* mrow = mstate + wave * EST_BE;
  float* srow = sstate + wave * EST_BE;
  int* irow = istate + wave * EST_BE;

  // prefetched A rows: 16 f32 per lane (row j32, k-slots 2*ch + g2)
  float nx_a[16];
  float nx_add;
  auto load_a = [&](int c) {
    const float* row = mfac32 + ((int64_t)c * 32 + j32) * 32;
#pragma unroll
    for (int ch = 0; ch < 16; ++ch) nx_a[ch] = row[2 * ch + g2];
    nx_add = add[c];
  };
  if (wave < k) load_a(wave);

  for (int c = wave; c < k; c += nwaves) {
    float a[16];
#pragma unroll
    for (int ch = 0; ch < 16; ++ch) a[ch] = nx_a[ch];
    const float addc = nx_add;
    if (c + nwaves < k) load_a(c + nwaves);
    // columns past the augmented one (index d) are zero padding: skipping
    // them is exact (see estep_fused_f32_kernel)
    const int chmax = d >> 1;
#pragma unroll 2
    for (int t = 0; t < EST_BE / 32; ++t) {
      const float* zrow = zs + (t * 32 + j32) * ZR;
      f32x16_t y = (f32x16_t)(0.0f);
#pragma unroll
      for (int ch = 0; ch < 16; ++ch) {
        if (ch > chmax) continue;
        const float b = zrow[2 * ch + g2];
        y = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ch], b, y, 0, 0, 0);
      }
      float s = 0.0f;
#pragma unroll
      for (int r = 0; r < 16; ++r) s = fmaf(y[r], y[r], s);
      s += __shfl_xor(s, 32, WAVE);
      if (lane < 32) {
        const int e = t * 32 + j32;
        const float lwv = -0.5f * s + addc;
        const float mo = mrow[e];
        if (lwv > mo) {
          srow[e] = srow[e] * __expf(mo - lwv) + 1.0f;
          mrow[e] = lwv;
          irow[e] = c;
        } else {
          srow[e] += __expf(lwv - mo);
        }
      }
    }
  }
  __syncthreads();

  // cross-wave combine -> the event's outputs (EST_BE == NT)
  {
    const int e = threadIdx.x;
    float m = mstate[e];
#pragma unroll
    for (int wv = 1; wv < nwaves; ++wv)
      m = fmaxf(m, mstate[wv * EST_BE + e]);
    float ssum = 0.0f;
    {
      // the training kernels compile this sum to separately rounded
      // multiplies and adds (their fixtures pin that); here the compiler
      // would contract it to an fma chain, so contraction is switched off
#pragma clang fp contract(off)
#pragma unroll
      for (int wv = 0; wv < nwaves; ++wv)
        ssum += sstate[wv * EST_BE + e] * __expf(mstate[wv * EST_BE + e] - m);
    }
    const float lse = m + __logf(ssum);
    int best = k - 1;  // every stored index is <= k - 1
#pragma unroll
    for (int wv = 0; wv < nwaves; ++wv)
      if (mstate[wv * EST_BE + e] == m)
        best = min(best, istate[wv * EST_BE + e]);
    if (e < cnt) {
      label_out[e0 + e] = best;
      lse_out[e0 + e] = lse;
      pmax_out[e0 + e] = __expf(m - lse);
    }
  }
}

}  // namespace gmm
