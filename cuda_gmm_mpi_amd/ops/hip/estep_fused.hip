// MFMA fused E-step family (D <= 31): log-weights, softmax and likelihood
// in one kernel. The five kernels share the precision policies, the tile
// constants and LDS budgets (also used by the launchers), sqnorm and
// block_sum. Their bodies are written out per kernel on purpose: built
// from shared __forceinline__ pieces every kernel ran ~1 % slower at the
// same register counts (docs/KERNELS.md); as written their assembly equals
// that of the kernels before they moved to this file.
//
//   estep_fused_kernel          bf16  256 events  online softmax, any K
//   estep_fused_f32_kernel      f32   256 events  online softmax, any K
//   estep_fused_lds_kernel      bf16  128 events  lw in LDS (legacy v1)
//   estep_fused_lds2_kernel     bf16  128 events  lw in LDS (default)
//   estep_fused_f32_lds_kernel  f32   128 events  lw in LDS
//
// Math:  logw[c, e] = -0.5 * ||M_c z_e||^2 + add_c  with  M_c = [U_c | -U_c mu_c],
// U_c^T U_c = Rinv_c (Cholesky, emitted by the constants kernel), z_e the
// event augmented with a 1 in row d and zero-padded to 32 rows. The bf16
// kernels read M split into bf16 hi + lo parts, so accuracy matches a
// bf16-data fp32-VALU quadratic form; the f32 kernels run
// v_mfma_f32_32x32x2_f32, bitwise an fmaf chain (guide §3).
//
// Shared structure. [Z] the block's z tile is staged TRANSPOSED in LDS
// (one row of 32 k-slots + pad per event, ones-row and zero pad baked in),
// so a B fragment is one contiguous read. [W] One 32-row MFMA tile covers
// all of M and 32 events; WAVES SPLIT THE CLUSTER LOOP (c = wave, wave + 4,
// ...) so each cluster's factor fragments are fetched once per block, not
// once per wave: that L2 traffic is the measured E-step floor.
// 32x32 fragment maps: A lane l -> A[i = l&31][kk], B lane l ->
// B[kk][j = l&31], C/D col = l&31, row = (reg&3) + 8*(reg>>2) + 4*(l>>5).
#pragma once

#include "gmm_common.h"

namespace gmm {

// ---------------------------------------------------------------------------
// Precision policies: In = element type of z and of the factor table in
// global memory, Z = element type of the staged z tile, ZROW = its row pitch
// in elements, CELLS = table elements per cluster. FacB16 is also lds2's
// factor-fragment type: one cluster's fragments as one lane holds them, with
// j32 = lane & 31 (A row) and g2 = lane >> 5 (k half) passed in by the caller.
// ---------------------------------------------------------------------------
struct FacB16 {  // table [K][2 (hi, lo)][32][32] bf16
  using In = __hip_bfloat16;
  using Z = __bf16;
  static constexpr int ZROW = 40;  // 32 k-slots + pad
  static constexpr int CELLS = 2 * 32 * 32;  // table elements per cluster

  bf16x8 h0, l0, h1, l1;  // hi / lo, k-chunk 0 = k [0,16) / 1 = k [16,32)
  float add;              // constant_c + ln pi_c

  __device__ __forceinline__ void load(const In* mfac, const float* addv,
                                       int c, int j32, int g2) {
    const bf16x8* mf = (const bf16x8*)mfac;  // rows of 32 bf16 = 4 frags each
    const int64_t base = ((int64_t)c * 2) * 32 * 4;  // in bf16x8 units
    h0 = mf[base + j32 * 4 + g2];
    l0 = mf[base + 32 * 4 + j32 * 4 + g2];
    h1 = mf[base + j32 * 4 + 2 + g2];
    l1 = mf[base + 32 * 4 + j32 * 4 + 2 + g2];
    add = addv[c];
  }
};

struct FacF32 {  // table [K][32][32] f32
  using In = float;
  using Z = float;
  static constexpr int ZROW = 33;  // 32 k-slots + pad
  static constexpr int CELLS = 32 * 32;
};

// floats the staged z tile of BE events takes at the front of the LDS
template <typename Fac, int BE>
constexpr int z_tile_floats() {
  return BE * Fac::ZROW * (int)sizeof(typename Fac::Z) / 4;
}

// ||y||^2 of the accumulator rows this lane holds, as one fmaf chain over
// the first NL registers. Register r holds Y row (r & 3) + 8 (r >> 2) +
// 4 (lane >> 5) and the factor table is exactly zero from row d on, so with
// NL = 4 ceil(d / 8) the registers left out are +0 in every lane and
// fmaf(0, 0, s) == s: the sum is bitwise the 16-register one.
template <int NL>
__device__ __forceinline__ float sqnorm(const f32x16_t& y) {
  float s = 0.0f;
#pragma unroll
  for (int r = 0; r < NL; ++r) s = fmaf(y[r], y[r], s);
  return s;
}

// ---------------------------------------------------------------------------
// Online-softmax kernels (any K): 256-event blocks with NO logw-in-LDS
// buffer. Each wave walks its cluster slice keeping a running per-event
// (max, sum) pair in LDS; logw goes to w_out and stays there: the lse-aware
// M-step applies exp(logw - lse) while staging w, so there is no normalize
// pass and no posterior write + read round trip. After a cross-wave combine
// the block writes the per-event log-sum-exp and its likelihood partial.
// LDS: zs [EST_BE][ZROW], m / s state [nwaves][EST_BE] f32 each, lse
// [EST_BE] f32 (29.7 KB bf16, 42.8 KB f32; K-independent).
// ---------------------------------------------------------------------------
constexpr int EST_BE = 256;  // events per block; == NT (one event per thread)

template <typename Fac>
constexpr size_t est_lds_bytes() {
  return sizeof(float) *
         (z_tile_floats<Fac, EST_BE>() + (2 * (NT / WAVE) + 1) * EST_BE);
}

__global__ void __launch_bounds__(NT)
estep_fused_kernel(const __hip_bfloat16* __restrict__ z,
                   const __hip_bfloat16* __restrict__ mfac,  // [K][2][32][32]
                   const float* __restrict__ add,            // const + ln pi
                   float* __restrict__ w_out, float* __restrict__ lse_out,
                   float* __restrict__ partial, int d, int k, int64_t n) {
  // LDS: the z tile [Z], then the state listed above this kernel pair
  extern __shared__ float lds[];
  __hip_bfloat16* zs = (__hip_bfloat16*)lds;
  float* mstate = lds + (EST_BE * FacB16::ZROW) / 2;   // [nwaves][EST_BE]
  float* sstate = mstate + (NT / WAVE) * EST_BE;   // [nwaves][EST_BE]
  float* lse = sstate + (NT / WAVE) * EST_BE;      // [EST_BE]

  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t e0 = (int64_t)blockIdx.x * EST_BE;
  const int cnt = (int)min((int64_t)EST_BE, n - e0);
  const bool full = cnt == EST_BE;

  __bf16* zsb = (__bf16*)zs;
  if (full) {
    // branchless staging (guide §5 trap 4c): coalesced reads of the d data
    // rows, transposed scatter into LDS; then the constant rows
    for (int idx = threadIdx.x; idx < d * EST_BE; idx += blockDim.x) {
      const int kk = idx / EST_BE, ei = idx % EST_BE;
      zsb[ei * FacB16::ZROW + kk] =
          (__bf16)__bfloat162float(z[(int64_t)kk * n + e0 + ei]);
    }
  } else {
    for (int idx = threadIdx.x; idx < d * EST_BE; idx += blockDim.x) {
      const int kk = idx / EST_BE, ei = idx % EST_BE;
      zsb[ei * FacB16::ZROW + kk] = (__bf16)(
          (ei < cnt) ? __bfloat162float(z[(int64_t)kk * n + e0 + ei]) : 0.0f);
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
      // one accumulator chain: Y = (Mhi+Mlo)(chunk0+chunk1) summed by the
      // MFMAs themselves (the VALU epilogue was the measured bottleneck)
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
        // logw to w_out as scratch (this block's slab stays L2-hot for
        // the normalize pass); lane j32 owns event e exclusively within
        // this wave, so the state update is race-free
        if (full || e < cnt) w_out[(int64_t)c * n + e0 + e] = lwv;
        const float mo = mrow[e];
        if (lwv > mo) {
          srow[e] = srow[e] * __expf(mo - lwv) + 1.0f;
          mrow[e] = lwv;
        } else {
          srow[e] += __expf(lwv - mo);
        }
      }
    }
  }
  __syncthreads();

  // combine the per-wave (m, s) into the per-event log-sum-exp
  // (EST_BE == NT: each thread owns one event)
  {
    const int e = threadIdx.x;
    float m = mstate[e];
#pragma unroll
    for (int wv = 1; wv < nwaves; ++wv)
      m = fmaxf(m, mstate[wv * EST_BE + e]);
    float ssum = 0.0f;
#pragma unroll
    for (int wv = 0; wv < nwaves; ++wv)
      ssum += sstate[wv * EST_BE + e] * __expf(mstate[wv * EST_BE + e] - m);
    lse[e] = m + __logf(ssum);
  }
  __syncthreads();

  // likelihood partial + per-event lse out. w_out holds LOGW — the
  // lse-aware M-step applies exp(logw - lse) while staging w, so no
  // normalize pass and no posterior write+read round trip at all.
  {
    float acc = 0.0f;
    if (threadIdx.x < cnt) {
      acc = lse[threadIdx.x];
      lse_out[e0 + threadIdx.x] = acc;
    }
    __shared__ float wsum[NT / WAVE];
    block_sum(acc, wsum, partial);
  }
}

__global__ void __launch_bounds__(NT)
estep_fused_f32_kernel(const float* __restrict__ z,
                       const float* __restrict__ mfac32,  // [K][32][32]
                       const float* __restrict__ add,
                       float* __restrict__ w_out,
                       float* __restrict__ lse_out,
                       float* __restrict__ partial, int d, int k, int64_t n) {
  constexpr int ZR = FacF32::ZROW;
  extern __shared__ float lds[];
  float* zs = lds;                                 // [EST_BE][ZR]
  float* mstate = lds + EST_BE * ZR;               // [nwaves][EST_BE]
  float* sstate = mstate + (NT / WAVE) * EST_BE;   // [nwaves][EST_BE]
  float* lse = sstate + (NT / WAVE) * EST_BE;      // [EST_BE]

  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int j32 = lane & 31;
  const int g2 = lane >> 5;
  const int64_t e0 = (int64_t)blockIdx.x * EST_BE;
  const int cnt = (int)min((int64_t)EST_BE, n - e0);
  const bool full = cnt == EST_BE;

  if (full) {
    for (int idx = threadIdx.x; idx < d * EST_BE; idx += blockDim.x) {
      const int kk = idx / EST_BE, ei = idx % EST_BE;
      zs[ei * ZR + kk] = z[(int64_t)kk * n + e0 + ei];
    }
  } else {
    for (int idx = threadIdx.x; idx < d * EST_BE; idx += blockDim.x) {
      const int kk = idx / EST_BE, ei = idx % EST_BE;
      zs[ei * ZR + kk] =
          (ei < cnt) ? z[(int64_t)kk * n + e0 + ei] : 0.0f;
    }
  }
  for (int idx = threadIdx.x; idx < (32 - d) * EST_BE; idx += blockDim.x) {
    const int kk = d + idx / EST_BE, ei = idx % EST_BE;
    zs[ei * ZR + kk] = (kk == d && ei < cnt) ? 1.0f : 0.0f;
  }
  for (int i = threadIdx.x; i < (NT / WAVE) * EST_BE; i += blockDim.x) {
    mstate[i] = -3.0e38f;
    sstate[i] = 0.0f;
  }
  __syncthreads();

  const int nwaves = NT / WAVE;
  float* mrow = mstate + wave * EST_BE;
  float* srow = sstate + wave * EST_BE;

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
    // columns past the augmented one (index d) are zero padding and
    // f32 MFMA accumulation of zeros is bitwise a no-op: skipping them
    // is exact and cuts the 16-deep dependent MFMA chain to d/2+1
    // (13 at D=24). d is kernel-uniform, so no divergence.
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
        if (full || e < cnt) w_out[(int64_t)c * n + e0 + e] = lwv;
        const float mo = mrow[e];
        if (lwv > mo) {
          srow[e] = srow[e] * __expf(mo - lwv) + 1.0f;
          mrow[e] = lwv;
        } else {
          srow[e] += __expf(lwv - mo);
        }
      }
    }
  }
  __syncthreads();

  // cross-wave combine -> per-event log-sum-exp (EST_BE == NT)
  {
    const int e = threadIdx.x;
    float m = mstate[e];
#pragma unroll
    for (int wv = 1; wv < nwaves; ++wv)
      m = fmaxf(m, mstate[wv * EST_BE + e]);
    float ssum = 0.0f;
#pragma unroll
    for (int wv = 0; wv < nwaves; ++wv)
      ssum += sstate[wv * EST_BE + e] * __expf(mstate[wv * EST_BE + e] - m);
    lse[e] = m + __logf(ssum);
  }
  __syncthreads();

  // likelihood partial + per-event lse out (w_out holds LOGW; the
  // lse-aware M-step normalizes on the fly)
  {
    float acc = 0.0f;
    if (threadIdx.x < cnt) {
      acc = lse[threadIdx.x];
      lse_out[e0 + threadIdx.x] = acc;
    }
    __shared__ float wsum[NT / WAVE];
    block_sum(acc, wsum, partial);
  }
}

// ---------------------------------------------------------------------------
// Small-K kernels (lw-in-LDS): 128-event blocks, log-weights kept in LDS,
// posteriors + likelihood fused in-block: logw never touches HBM and the
// M-step reads plain posteriors (no exp at staging). Same-box A/B showed
// this beats the online-softmax variant by ~19 us/iter at the flagship
// K = 64 (the M-step's staging exp is on its VALU-bound critical path), so
// it is the preferred path when K fits; the kernels above cover the rest.
// LDS: zs [ESTL_BE][ZROW], then lw [k][ESTL_LROW] f32: K <= 104 bf16,
// K <= 85 f32 in 64 KB.
// ---------------------------------------------------------------------------
constexpr int ESTL_BE = 128;              // events per block
constexpr int ESTL_LROW = ESTL_BE + 4;    // lw row pitch

template <typename Fac>
constexpr size_t estl_lds_bytes(int k) {
  return sizeof(float) *
         (z_tile_floats<Fac, ESTL_BE>() + (size_t)k * ESTL_LROW);
}

// First version of the bf16 kernel; reachable as GMM_ESTEP_LDS=legacy.
__global__ void __launch_bounds__(NT)
estep_fused_lds_kernel(const __hip_bfloat16* __restrict__ z,
                   const __hip_bfloat16* __restrict__ mfac,  // [K][2][32][32]
                   const float* __restrict__ add,            // const + ln pi
                   float* __restrict__ w_out, float* __restrict__ partial,
                   int d, int k, int64_t n) {
  // LDS: the z tile [Z], then lw [k][ESTL_LROW] f32
  extern __shared__ float lds[];
  const int lrow = ESTL_LROW;
  __hip_bfloat16* zs = (__hip_bfloat16*)lds;
  float* lw = lds + (ESTL_BE * FacB16::ZROW) / 2;

  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t e0 = (int64_t)blockIdx.x * ESTL_BE;
  const int cnt = (int)min((int64_t)ESTL_BE, n - e0);

  __bf16* zsb = (__bf16*)zs;
  if (cnt == ESTL_BE) {
    // branchless staging (guide §5 trap 4c): coalesced reads of the d data
    // rows, transposed scatter into LDS; then the constant rows
    for (int idx = threadIdx.x; idx < d * ESTL_BE; idx += blockDim.x) {
      const int kk = idx / ESTL_BE, ei = idx % ESTL_BE;
      zsb[ei * FacB16::ZROW + kk] =
          (__bf16)__bfloat162float(z[(int64_t)kk * n + e0 + ei]);
    }
  } else {
    for (int idx = threadIdx.x; idx < d * ESTL_BE; idx += blockDim.x) {
      const int kk = idx / ESTL_BE, ei = idx % ESTL_BE;
      zsb[ei * FacB16::ZROW + kk] = (__bf16)(
          (ei < cnt) ? __bfloat162float(z[(int64_t)kk * n + e0 + ei]) : 0.0f);
    }
  }
  for (int idx = threadIdx.x; idx < (32 - d) * ESTL_BE; idx += blockDim.x) {
    const int kk = d + idx / ESTL_BE, ei = idx % ESTL_BE;
    zsb[ei * FacB16::ZROW + kk] =
        (__bf16)((kk == d && ei < cnt) ? 1.0f : 0.0f);
  }
  __syncthreads();

  // cluster loop [W]; per 16-deep chunk A lane l holds kk = 8*(l>>5)+u
  const int j32 = lane & 31;
  const int g2 = lane >> 5;
  const bf16x8* mf = (const bf16x8*)mfac;  // rows of 32 bf16 = 4 frags each
  const int fq0 = g2;      // chunk 0 covers k [0,16): slots {0,1}
  const int fq1 = 2 + g2;  // chunk 1 covers k [16,32): slots {2,3}
  const int nwaves = NT / WAVE;

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
    for (int t = 0; t < ESTL_BE / 32; ++t) {
      // B fragments: contiguous 16 B of the transposed z row
      const bf16x8 b0 =
          *(const bf16x8*)(zs + (t * 32 + j32) * FacB16::ZROW + 8 * g2);
      const bf16x8 b1 =
          *(const bf16x8*)(zs + (t * 32 + j32) * FacB16::ZROW + 16 + 8 * g2);
      // one accumulator chain: Y = (Mhi+Mlo)(chunk0+chunk1) summed by the
      // MFMAs themselves (the VALU epilogue was the measured bottleneck)
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
      if (lane < 32) lw[c * lrow + t * 32 + j32] = -0.5f * s + addc;
    }
  }
  __syncthreads();

  // pass 2: posteriors + likelihood, cluster loop split across BOTH
  // thread halves (the serial 64-deep store loop was 24% of the kernel —
  // store-issue-bound): threads t and t+ESTL_BE each handle half the
  // clusters of event t, combining max/sum through LDS.
  __shared__ float pmax[2][ESTL_BE];
  __shared__ float psum[2][ESTL_BE];
  float acc = 0.0f;
  {
    const int t = threadIdx.x & (ESTL_BE - 1);
    const int half = threadIdx.x >> 7;       // ESTL_BE == 128
    const int mid = (k + 1) / 2;   // half 0 never empty (K=1, odd K)
    const int c_lo = half * mid;
    const int c_hi = half ? k : mid;
    if (t < cnt && c_lo < c_hi) {
      float m = lw[c_lo * lrow + t];
#pragma unroll 4
      for (int c = c_lo + 1; c < c_hi; ++c)
        m = fmaxf(m, lw[c * lrow + t]);
      pmax[half][t] = m;
    } else if (t < ESTL_BE) {
      pmax[half][t] = -3.0e38f;
    }
    __syncthreads();
    const float m = fmaxf(pmax[0][t], pmax[1][t]);
    float s = 0.0f;
    if (t < cnt) {
#pragma unroll 4
      for (int c = c_lo; c < c_hi; ++c) {
        const float e = __expf(lw[c * lrow + t] - m);
        lw[c * lrow + t] = e;
        s += e;
      }
    }
    psum[half][t] = s;
    __syncthreads();
    const float total = psum[0][t] + psum[1][t];
    if (t < cnt && c_lo < c_hi) {
      const float inv = 1.0f / total;
#pragma unroll 4
      for (int c = c_lo; c < c_hi; ++c)
        w_out[(int64_t)c * n + e0 + t] = lw[c * lrow + t] * inv;
      if (half == 0) acc = m + __logf(total);
    }
  }
  __shared__ float wsum[NT / WAVE];
  block_sum(acc, wsum, partial);
}

__global__ void __launch_bounds__(NT)
estep_fused_f32_lds_kernel(const float* __restrict__ z,
                       const float* __restrict__ mfac32,  // [K][32][32]
                       const float* __restrict__ add,
                       float* __restrict__ w_out, float* __restrict__ partial,
                       int d, int k, int64_t n) {
  constexpr int ZR = FacF32::ZROW;
  extern __shared__ float lds[];
  float* zs = lds;                         // [ESTL_BE][ZR]
  const int lrow = ESTL_LROW;
  float* lw = lds + ESTL_BE * ZR;           // [k][lrow]

  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int j32 = lane & 31;
  const int g2 = lane >> 5;
  const int64_t e0 = (int64_t)blockIdx.x * ESTL_BE;
  const int cnt = (int)min((int64_t)ESTL_BE, n - e0);

  if (cnt == ESTL_BE) {
    // all of a thread's loads are issued before the first is used (one
    // wait per block, not one per row pair); rows >= d load row d-1 and
    // are not stored
    constexpr int NIT = 32 * ESTL_BE / NT;  // 16 row pairs cover d <= 31
    const int ei = threadIdx.x % ESTL_BE, k0 = threadIdx.x / ESTL_BE;
    float v[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it)
      v[it] = z[(int64_t)min(k0 + 2 * it, d - 1) * n + e0 + ei];
#pragma unroll
    for (int it = 0; it < NIT; ++it)
      if (k0 + 2 * it < d) zs[ei * ZR + k0 + 2 * it] = v[it];
  } else {
    for (int idx = threadIdx.x; idx < d * ESTL_BE; idx += blockDim.x) {
      const int kk = idx / ESTL_BE, ei = idx % ESTL_BE;
      zs[ei * ZR + kk] =
          (ei < cnt) ? z[(int64_t)kk * n + e0 + ei] : 0.0f;
    }
  }
  for (int idx = threadIdx.x; idx < (32 - d) * ESTL_BE; idx += blockDim.x) {
    const int kk = d + idx / ESTL_BE, ei = idx % ESTL_BE;
    zs[ei * ZR + kk] = (kk == d && ei < cnt) ? 1.0f : 0.0f;
  }
  __syncthreads();

  const int nwaves = NT / WAVE;

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
#pragma unroll 2
    for (int t = 0; t < ESTL_BE / 32; ++t) {
      const float* zrow = zs + (t * 32 + j32) * ZR;
      f32x16_t y = (f32x16_t)(0.0f);
#pragma unroll
      for (int ch = 0; ch < 16; ++ch) {
        if (ch > (d >> 1)) continue;  // zero padding past the aug column: exact skip
        const float b = zrow[2 * ch + g2];
        y = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ch], b, y, 0, 0, 0);
      }
      float s = 0.0f;
#pragma unroll
      for (int r = 0; r < 16; ++r) s = fmaf(y[r], y[r], s);
      s += __shfl_xor(s, 32, WAVE);
      if (lane < 32) lw[c * lrow + t * 32 + j32] = -0.5f * s + addc;
    }
  }
  __syncthreads();

  // pass 2: one thread per event walks all K clusters (not the two-half
  // split of estep_fused_lds_kernel: a different summation order)
  float acc = 0.0f;
  if (threadIdx.x < ESTL_BE && threadIdx.x < cnt) {
    const int t = threadIdx.x;
    float m = lw[t];
#pragma unroll 4
    for (int c = 1; c < k; ++c) m = fmaxf(m, lw[c * lrow + t]);
    float s = 0.0f;
#pragma unroll 4
    for (int c = 0; c < k; ++c) {
      const float e = __expf(lw[c * lrow + t] - m);
      lw[c * lrow + t] = e;
      s += e;
    }
    const float inv = 1.0f / s;
#pragma unroll 4
    for (int c = 0; c < k; ++c)
      w_out[(int64_t)c * n + e0 + t] = lw[c * lrow + t] * inv;
    acc = m + __logf(s);
  }
  __shared__ float wsum[NT / WAVE];
  block_sum(acc, wsum, partial);
}

// ---------------------------------------------------------------------------
// Second version of the small-K bf16 kernel (the default). Same contract,
// same LDS footprint and bitwise the same log-weights as
// estep_fused_lds_kernel; three things differ (134 VGPRs, no AGPRs, no
// scratch: 3 waves per SIMD, the limit the LDS sets anyway):
//  - staging: a work item is (event, k-octet). It issues its <= 8 coalesced
//    2-byte loads back to back, waits once, and writes one 16-byte LDS store
//    with the ones-row and the zero pad already in place;
//  - MFMA phase: the 8 B fragments of the block's 4 event tiles are read once
//    and held in registers; per cluster 4 independent accumulators (arch
//    VGPRs: the launch bound keeps the register budget under 256, so the
//    compiler does not pick the AGPR form) run with no LDS read in the loop,
//    and a permlane32_swap of two tiles' half sums lets all 64 lanes finish
//    and store a log-weight;
//  - pass 2: a thread owns 4 consecutive events of one cluster slice
//    (clusters s, s+8, ...), reads and rewrites lw as float4 and stores the
//    posteriors as float4 when n % 4 == 0. The 8 slices combine max and sum
//    through the z tile's LDS, which is dead by then.
// ---------------------------------------------------------------------------
constexpr int ESTL2_NS = 8;  // cluster slices in pass 2 (NT / 32)

template <int NL>  // live accumulator registers, 4 ceil(d / 8): see sqnorm
__global__ void __launch_bounds__(NT, 3)
estep_fused_lds2_kernel(const __hip_bfloat16* __restrict__ z,
                        const __hip_bfloat16* __restrict__ mfac,
                        const float* __restrict__ add,
                        float* __restrict__ w_out,
                        float* __restrict__ partial, int d, int k, int64_t n,
                        int vec4) {
  // the z tile's LDS is reused in pass 2 as cmax/csum [ESTL2_NS][ESTL_BE]
  extern __shared__ float lds[];
  constexpr int lrow = ESTL_LROW;
  constexpr int ZROW = FacB16::ZROW;
  __hip_bfloat16* zs = (__hip_bfloat16*)lds;
  float* lw = lds + z_tile_floats<FacB16, ESTL_BE>();

  // wave-uniform by construction; readfirstlane lets the compiler keep the
  // row and cluster indices (and their 64-bit address products) in SGPRs
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t e0 = (int64_t)blockIdx.x * ESTL_BE;
  const int cnt = (int)min((int64_t)ESTL_BE, n - e0);

  // staging: items (event e, octet o), 128 x 4 = 2 per thread; lanes run
  // along e. Octet slot i holds row 8o+i: data below d, the constant 1 at
  // d, zero above. Rows >= d load row d-1 (a valid address) and drop it, so
  // every load is issued before the first wait.
  {
    const unsigned short* zu = (const unsigned short*)z;
    const int e = threadIdx.x & (ESTL_BE - 1);
    const int o_lo = wave >> 1;  // items o_lo and o_lo + 2 (tid >> 7)
    unsigned short v[2][8];
    if (cnt == ESTL_BE) {
#pragma unroll
      for (int it = 0; it < 2; ++it)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int row = min(8 * (o_lo + 2 * it) + i, d - 1);
          v[it][i] = zu[(int64_t)row * n + e0 + e];
        }
    } else {
      const int ec = min(e, cnt - 1);
#pragma unroll
      for (int it = 0; it < 2; ++it)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int row = min(8 * (o_lo + 2 * it) + i, d - 1);
          const unsigned short x = zu[(int64_t)row * n + e0 + ec];
          v[it][i] = (e < cnt) ? x : (unsigned short)0;
        }
    }
    const unsigned short one = (e < cnt) ? 0x3F80 : 0;  // bf16 1.0
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int o = o_lo + 2 * it;
      unsigned int p[4];
#pragma unroll
      for (int i = 0; i < 8; i += 2) {
        const int r0 = 8 * o + i, r1 = r0 + 1;
        const unsigned int lo = r0 < d ? v[it][i] : (r0 == d ? one : 0);
        const unsigned int hi = r1 < d ? v[it][i + 1] : (r1 == d ? one : 0);
        p[i >> 1] = lo | (hi << 16);
      }
      *(uint4*)(zs + e * ZROW + 8 * o) = make_uint4(p[0], p[1], p[2], p[3]);
    }
  }
  __syncthreads();

  // MFMA phase: waves split the cluster loop as in [W]
  const int j32 = lane & 31;
  const int g2 = lane >> 5;
  const int nwaves = NT / WAVE;

  // the B fragments do not depend on the cluster: read them once
  bf16x8 b0[ESTL_BE / 32], b1[ESTL_BE / 32];
#pragma unroll
  for (int t = 0; t < ESTL_BE / 32; ++t) {
    b0[t] = *(const bf16x8*)(zs + (t * 32 + j32) * ZROW + 8 * g2);
    b1[t] = *(const bf16x8*)(zs + (t * 32 + j32) * ZROW + 16 + 8 * g2);
  }
  auto cluster = [&](const FacB16& f, int c) {
    // 4 independent chains, each in the order of estep_fused_lds_kernel
    // (hi.b0, hi.b1, lo.b0, lo.b1), issued tile-interleaved
    f32x16_t y[ESTL_BE / 32];
#pragma unroll
    for (int t = 0; t < ESTL_BE / 32; ++t)
      y[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
          f.h0, b0[t], (f32x16_t)(0.0f), 0, 0, 0);
#pragma unroll
    for (int t = 0; t < ESTL_BE / 32; ++t)
      y[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.h1, b1[t], y[t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < ESTL_BE / 32; ++t)
      y[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.l0, b0[t], y[t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < ESTL_BE / 32; ++t)
      y[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.l1, b1[t], y[t], 0, 0, 0);
    float s[ESTL_BE / 32];
#pragma unroll
    for (int t = 0; t < ESTL_BE / 32; ++t) s[t] = sqnorm<NL>(y[t]);
    // the 32 Y rows live across the two lane halves. Swap the upper half of
    // tile t with the lower half of tile t+1: lanes 0-31 then hold both
    // halves of tile t, lanes 32-63 both of tile t+1 (lower half first in
    // either, as in the __shfl_xor sum of estep_fused_lds_kernel), and every lane stores
#pragma unroll
    for (int t = 0; t < ESTL_BE / 32; t += 2) {
      const auto sw = __builtin_amdgcn_permlane32_swap(
          __float_as_uint(s[t]), __float_as_uint(s[t + 1]), false, false);
      const float st = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
      lw[c * lrow + (t + g2) * 32 + j32] = -0.5f * st + f.add;
    }
  };
  // one-deep factor prefetch over two register sets: the next cluster's
  // loads are issued before this cluster's MFMAs and first waited for a
  // whole cluster later (one set and a copy put the wait mid-cluster).
  // The prefetch is unconditional (past the end it re-loads cluster k-1):
  // a load under a branch makes the number of loads in flight depend on
  // the path, and the compiler then waits for all of them.
  FacB16 fa, fb;
  int c = wave;
  fa.load(mfac, add, min(c, k - 1), j32, g2);
  for (; c + nwaves < k; c += 2 * nwaves) {  // two clusters, one basic block
    // the scheduling barriers keep each prefetch ahead of the cluster it
    // overlaps and the two clusters' accumulators from being live together
    fb.load(mfac, add, c + nwaves, j32, g2);
    __builtin_amdgcn_sched_barrier(0);
    cluster(fa, c);
    __builtin_amdgcn_sched_barrier(0);
    fa.load(mfac, add, min(c + 2 * nwaves, k - 1), j32, g2);
    __builtin_amdgcn_sched_barrier(0);
    cluster(fb, c + nwaves);
    __builtin_amdgcn_sched_barrier(0);
  }
  if (c < k) cluster(fa, c);  // odd count: fa already holds cluster c
  __syncthreads();

  // pass 2: thread = (event group g: events 4g..4g+3, cluster slice sl).
  // An empty slice (sl >= k) contributes -3e38 to the max and 0 to the sum.
  float4* lw4 = (float4*)lw;                  // row stride lrow / 4 = 33
  float4* cmax = (float4*)lds;                // [ESTL2_NS][32]
  float4* csum = cmax + ESTL2_NS * 32;        // [ESTL2_NS][32]
  const int g = threadIdx.x & 31;
  const int sl = threadIdx.x >> 5;
  float4 m = make_float4(-3.0e38f, -3.0e38f, -3.0e38f, -3.0e38f);
#pragma unroll 4
  for (int c = sl; c < k; c += ESTL2_NS) {
    const float4 x = lw4[c * (lrow / 4) + g];
    m.x = fmaxf(m.x, x.x);
    m.y = fmaxf(m.y, x.y);
    m.z = fmaxf(m.z, x.z);
    m.w = fmaxf(m.w, x.w);
  }
  cmax[sl * 32 + g] = m;
  __syncthreads();
  m = cmax[g];
#pragma unroll
  for (int q = 1; q < ESTL2_NS; ++q) {
    const float4 x = cmax[q * 32 + g];
    m.x = fmaxf(m.x, x.x);
    m.y = fmaxf(m.y, x.y);
    m.z = fmaxf(m.z, x.z);
    m.w = fmaxf(m.w, x.w);
  }
  float4 sum = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll 4
  for (int c = sl; c < k; c += ESTL2_NS) {
    float4 x = lw4[c * (lrow / 4) + g];
    x.x = __expf(x.x - m.x);
    x.y = __expf(x.y - m.y);
    x.z = __expf(x.z - m.z);
    x.w = __expf(x.w - m.w);
    lw4[c * (lrow / 4) + g] = x;
    sum.x += x.x;
    sum.y += x.y;
    sum.z += x.z;
    sum.w += x.w;
  }
  csum[sl * 32 + g] = sum;
  __syncthreads();
  float4 total = csum[g];
#pragma unroll
  for (int q = 1; q < ESTL2_NS; ++q) {
    const float4 x = csum[q * 32 + g];
    total.x += x.x;
    total.y += x.y;
    total.z += x.z;
    total.w += x.w;
  }
  const float4 inv = make_float4(1.0f / total.x, 1.0f / total.y,
                                 1.0f / total.z, 1.0f / total.w);
  const int left = cnt - 4 * g;  // valid events of this group (may be <= 0)
  if (vec4) {
    // n % 4 == 0: cnt is a multiple of 4, a group is all valid or all pad
    if (left > 0) {
#pragma unroll 4
      for (int c = sl; c < k; c += ESTL2_NS) {
        const float4 x = lw4[c * (lrow / 4) + g];
        *(float4*)(w_out + (int64_t)c * n + e0 + 4 * g) =
            make_float4(x.x * inv.x, x.y * inv.y, x.z * inv.z, x.w * inv.w);
      }
    }
  } else {
#pragma unroll 2
    for (int c = sl; c < k; c += ESTL2_NS) {
      const float4 x = lw4[c * (lrow / 4) + g];
      float* dst = w_out + (int64_t)c * n + e0 + 4 * g;
      if (left > 0) dst[0] = x.x * inv.x;
      if (left > 1) dst[1] = x.y * inv.y;
      if (left > 2) dst[2] = x.z * inv.z;
      if (left > 3) dst[3] = x.w * inv.w;
    }
  }
  // likelihood: slice 0 is lanes 0-31 of wave 0 and holds all 128 events,
  // so one wave reduces it (not block_sum: a different summation order)
  if (wave == 0) {
    float acc = 0.0f;
    if (sl == 0) {
      if (left > 0) acc += m.x + __logf(total.x);
      if (left > 1) acc += m.y + __logf(total.y);
      if (left > 2) acc += m.z + __logf(total.z);
      if (left > 3) acc += m.w + __logf(total.w);
    }
    for (int off = WAVE / 2; off > 0; off >>= 1)
      acc += __shfl_down(acc, off, WAVE);
    if (lane == 0) partial[blockIdx.x] = acc;
  }
}

}  // namespace gmm
