// Greedy k-means++ seeding on the device (any D, any n): K rounds of
//
//   sample    1 block     the round's candidate rows, drawn from s * m
//   evaluate  n/256 blk   d_l = |x_e - x_cand_l|^2 for up to 8 candidates in
//                         one pass over x; min(m, d_l) into scratch [L, n],
//                         float64 block partials of s * min(m, d_l)
//   choose    1 block     fixed-order sum of the partials, lowest slot that
//                         attains the minimum potential
//   commit    n/256 blk   m <- the winner's scratch row, float64 block
//                         partials of s * m for the next draw
//
// Everything a round decides (candidate indices, winner slot) stays in device
// buffers that the next kernel reads, so the host enqueues all K rounds
// without a synchronisation and copies the trace back once. There are no
// atomics: every sum is a fixed tree over fixed slots, so two runs agree bit
// for bit.
//
// Numerics. Distances are sums of squared differences in fp32 (fmaf chain
// over the dimensions in ascending order); x_e == x_cand gives an exact 0.
// Every quantity that is summed over events (potentials, draw masses) is the
// exact float64 product of fp32 values, summed in float64.
//
// evaluate is the HBM-bound kernel (4 D bytes per event against 16 D VALU
// operations): x is event-major [n, D], a block's 256 events are staged into
// LDS in column chunks of up to 32. For D <= 32 that is the contiguous slab
// walk of estep_classify (consecutive threads, consecutive floats; a full
// block moves it as 16-byte vectors); above it each event contributes one
// contiguous run of 32 floats per chunk. The row pitch of 33 makes the
// per-event reads (lane stride 33) conflict-free. The chunk of the candidate
// rows sits next to it as [32][8], so a thread reads its eight candidates of
// one dimension as two broadcast 16-byte loads. Measured times, bytes and
// floors: docs/KERNELS.md.
#pragma once

#include "gmm_common.h"

namespace gmm {

constexpr int SEED_BE = NT;      // events per block, one per thread
constexpr int SEED_DC = 32;      // dimensions per staged chunk
constexpr int SEED_ZROW = SEED_DC + 1;
constexpr int SEED_LMAX = 8;     // candidates per round: 2 + floor(ln 512)

// Fixed-order block sum of NV doubles per thread: xor-butterfly inside each
// wave, then the waves in ascending order. Thread v < NV ends up holding the
// total of value v and stores it to out[v]. Only the first `live` values
// (uniform over the block) are summed; the others are stored as 0.
template <int NV>
__device__ __forceinline__ void seed_block_sum(double (&p)[NV], int live,
                                               double* __restrict__ red,
                                               double* __restrict__ out) {
  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    if (v >= live) break;
#pragma unroll
    for (int off = WAVE / 2; off >= 1; off >>= 1)
      p[v] += __shfl_xor(p[v], off, WAVE);
    if (lane == 0) red[wave * NV + v] = p[v];
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    double t = 0.0;
    if (threadIdx.x < live) {
      t = red[threadIdx.x];
#pragma unroll
      for (int w = 1; w < NT / WAVE; ++w) t += red[w * NV + threadIdx.x];
    }
    out[threadIdx.x] = t;
  }
}

// Block partials of the event weights, s_part[b] = sum of s over block b's
// events (the event count when s is null): the mass the first draw, and a
// draw at zero potential, samples from.
__global__ void __launch_bounds__(NT)
seed_weight_partials_kernel(const float* __restrict__ s,
                            double* __restrict__ s_part, int64_t n) {
  __shared__ double red[NT / WAVE];
  const int64_t e = (int64_t)blockIdx.x * SEED_BE + threadIdx.x;
  double p[1] = {e < n ? (s != nullptr ? (double)s[e] : 1.0) : 0.0};
  seed_block_sum<1>(p, 1, red, s_part + blockIdx.x);
}

// Sequential pick over the values at(0..cnt): the first i whose running sum,
// started at `run`, exceeds `target`; when rounding keeps the sum from
// crossing, the last i with a positive value (0 if there is none). `run`
// becomes the running sum in front of the returned i. Written without an
// early exit so that the loads of the unrolled loop are issued together.
template <typename At>
__device__ __forceinline__ int seed_scan_pick(At at, int cnt, double target,
                                              double& run) {
  int pick = 0;
  double base = run, r = run;
  bool open = true;
#pragma unroll 8
  for (int i = 0; i < cnt; ++i) {
    const double v = at(i);
    if (open && v > 0.0) {
      pick = i;
      base = r;
    }
    open = open && !(r + v > target);
    r += v;
  }
  run = base;
  return pick;
}

// Draw the round's `nl` candidates into cand[0..nl) (slots up to 8 repeat
// slot 0, so evaluate always reads valid rows). pick(p, u) is the first event
// whose running sum of p exceeds u * sum(p), found level by level: the 256
// segments of consecutive block partials, the blocks of that segment, the
// events of that block; the running sum is carried from level to level. The
// mass is s * m, or s alone when `by_weight` is set or s * m sums to zero
// (fewer distinct rows than clusters). A running sum that rounding keeps
// from crossing the target ends on the last segment / block / event with
// positive mass, so an event with zero mass is never returned. Lane l of
// wave 0 serves uniform l.
__global__ void __launch_bounds__(NT)
seed_sample_kernel(const float* __restrict__ s, const float* __restrict__ m,
                   const double* __restrict__ sm_part,
                   const double* __restrict__ s_part,
                   const double* __restrict__ u, int nl, int by_weight,
                   int64_t* __restrict__ cand, int64_t nblk, int64_t n) {
  constexpr int VROW = SEED_BE + 2;  // rows 4 banks apart: no lane conflicts
  __shared__ double seg_sum[NT];
  __shared__ double vals[SEED_LMAX * VROW];
  __shared__ double total_sh;
  __shared__ int64_t blk_sh[SEED_LMAX];

  const int tid = threadIdx.x;
  const int64_t seg = (nblk + NT - 1) / NT;  // blocks per segment
  const int64_t b0 = min((int64_t)tid * seg, nblk);
  const int64_t b1 = min(b0 + seg, nblk);

  const double* part = by_weight ? s_part : sm_part;
  bool weight_mode = by_weight != 0;
  for (int pass = 0; pass < 2; ++pass) {
    double acc = 0.0;
#pragma unroll 4
    for (int64_t b = b0; b < b1; ++b) acc += part[b];
    seg_sum[tid] = acc;
    __syncthreads();
    if (tid == 0) {
      double run = 0.0;
#pragma unroll 8
      for (int j = 0; j < NT; ++j) run += seg_sum[j];
      total_sh = run;
    }
    __syncthreads();
    if (weight_mode || total_sh != 0.0) break;
    // zero potential: every remaining row duplicates a chosen one
    part = s_part;
    weight_mode = true;
  }

  // levels 1 and 2: the segment, then the block inside it
  double run = 0.0, target = 0.0;
  if (tid < nl) {
    target = u[tid] * total_sh;
    const int j = seed_scan_pick([&](int q) { return seg_sum[q]; }, NT,
                                 target, run);
    const int64_t s0 = min((int64_t)j * seg, nblk - 1);
    const int64_t s1 = min(s0 + seg, nblk);
    blk_sh[tid] = s0 + seed_scan_pick([&](int i) { return part[s0 + i]; },
                                      (int)(s1 - s0), target, run);
  }
  __syncthreads();

  // level 3: the events of every slot's block, staged side by side
  for (int l = 0; l < nl; ++l) {
    const int64_t e = blk_sh[l] * SEED_BE + tid;
    double v = 0.0;
    if (e < n) {
      v = (s != nullptr) ? (double)s[e] : 1.0;
      if (!weight_mode) v *= (double)m[e];
    }
    vals[l * VROW + tid] = v;
  }
  __syncthreads();
  if (tid < nl) {
    const double* row = vals + tid * VROW;
    const int i = seed_scan_pick([&](int q) { return row[q]; }, SEED_BE,
                                 target, run);
    cand[tid] = min(blk_sh[tid] * SEED_BE + i, n - 1);
  }
  __syncthreads();
  if (tid >= nl && tid < SEED_LMAX) cand[tid] = cand[0];
}

// One pass over x: squared distances of a block's events to the candidate
// rows cand[0..8) (all eight are computed; slots >= nl repeat slot 0 and are
// not stored). `first` marks round 0, where m does not exist yet and the
// distance itself is stored.
__global__ void __launch_bounds__(NT)
seed_evaluate_kernel(const float* __restrict__ x,   // [n][d] event-major
                     const float* __restrict__ s,   // [n] or null
                     const float* __restrict__ m,   // [n]
                     const int64_t* __restrict__ cand,  // [8]
                     int nl, int first,
                     float* __restrict__ scratch,    // [nl][n]
                     double* __restrict__ pot_part,  // [nblk][8]
                     int vec,  // x is 16-byte aligned
                     int d, int64_t n) {
  __shared__ float zs[SEED_BE * SEED_ZROW];
  __shared__ __attribute__((aligned(16))) float cs[SEED_DC * SEED_LMAX];
  __shared__ double red[(NT / WAVE) * SEED_LMAX];

  const int tid = threadIdx.x;
  const int64_t e0 = (int64_t)blockIdx.x * SEED_BE;
  const int cnt = (int)min((int64_t)SEED_BE, n - e0);
  const float* slab = x + e0 * d;

  float acc[SEED_LMAX];
#pragma unroll
  for (int l = 0; l < SEED_LMAX; ++l) acc[l] = 0.0f;

  // this thread's element of the candidate chunk: dimension ck, slot cl
  const int ck = tid / SEED_LMAX, cl = tid % SEED_LMAX;
  // (clamped: a caller-written candidate can never index outside x)
  const float* crow = x + min(max(cand[cl], (int64_t)0), n - 1) * d;

  for (int c0 = 0; c0 < d; c0 += SEED_DC) {
    const int dc = min(SEED_DC, d - c0);
    if (c0 > 0) __syncthreads();  // the previous chunk has been consumed
    cs[tid] = (ck < dc) ? crow[c0 + ck] : 0.0f;
    if (vec && dc == d && cnt == SEED_BE) {
      // full block of whole rows: the slab is one 16-byte aligned run of
      // 256 d floats (64 d vectors), moved as 16-byte loads that the
      // unrolled loop issues back to back
      const f32x4* slab4 = reinterpret_cast<const f32x4*>(slab);
      const int nv = SEED_BE / 4 * d;
#pragma unroll 4
      for (int v = tid; v < nv; v += NT) {
        const f32x4 q = slab4[v];
        int ei = (4 * v) / d, kk = 4 * v - ei * d;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          zs[ei * SEED_ZROW + kk] = q[u];
          if (++kk == d) {
            kk = 0;
            ++ei;
          }
        }
      }
    } else {
      // chunk walk: element idx is (event idx / dc, column idx % dc); a step
      // of NT elements moves that pair by (NT / dc, NT % dc). With dc == d
      // the source offsets are idx itself: the contiguous slab
      const int live = cnt * dc;
      const int qs = NT / dc, rs = NT % dc;
      int ei = tid / dc, kk = tid % dc;
#pragma unroll 4
      for (int idx = tid; idx < live; idx += NT) {
        zs[ei * SEED_ZROW + kk] = slab[(int64_t)ei * d + c0 + kk];
        ei += qs;
        kk += rs;
        if (kk >= dc) {
          kk -= dc;
          ++ei;
        }
      }
    }
    __syncthreads();
    if (tid < cnt) {
      const float* zrow = zs + tid * SEED_ZROW;
      const f32x4* c4 = reinterpret_cast<const f32x4*>(cs);
#pragma unroll 4
      for (int kk = 0; kk < dc; ++kk) {
        const float v = zrow[kk];
        const f32x4 ca = c4[2 * kk], cb = c4[2 * kk + 1];
#pragma unroll
        for (int l = 0; l < 4; ++l) {
          const float da = v - ca[l], db = v - cb[l];
          acc[l] = fmaf(da, da, acc[l]);
          acc[4 + l] = fmaf(db, db, acc[4 + l]);
        }
      }
    }
  }

  double p[SEED_LMAX];
  {
    const bool live = tid < cnt;
    const float mo = (live && !first) ? m[e0 + tid] : INFINITY;
    const double sv = live ? (s != nullptr ? (double)s[e0 + tid] : 1.0) : 0.0;
#pragma unroll
    for (int l = 0; l < SEED_LMAX; ++l) {
      const float v = fminf(mo, acc[l]);
      const bool keep = live && l < nl;
      if (keep) scratch[(int64_t)l * n + e0 + tid] = v;
      p[l] = keep ? sv * (double)v : 0.0;
    }
  }
  seed_block_sum<SEED_LMAX>(p, nl, red,
                            pot_part + (int64_t)blockIdx.x * SEED_LMAX);
}

// Potentials of the round's candidates from the block partials (thread i
// sums blocks i, i + 256, ... in ascending order, then the block tree) and
// the winner: the lowest slot that attains the minimum. One block.
__global__ void __launch_bounds__(NT)
seed_choose_kernel(const double* __restrict__ pot_part,  // [nblk][8]
                   const int64_t* __restrict__ cand,     // [8]
                   int nl, int* __restrict__ winner,
                   int64_t* __restrict__ index,
                   double* __restrict__ pots,             // [8]
                   int64_t nblk) {
  __shared__ double red[(NT / WAVE) * SEED_LMAX];
  double p[SEED_LMAX];
#pragma unroll
  for (int l = 0; l < SEED_LMAX; ++l) p[l] = 0.0;
#pragma unroll 4
  for (int64_t b = threadIdx.x; b < nblk; b += NT) {
#pragma unroll
    for (int l = 0; l < SEED_LMAX; ++l) p[l] += pot_part[b * SEED_LMAX + l];
  }
  seed_block_sum<SEED_LMAX>(p, nl, red, pots);
  __syncthreads();
  if (threadIdx.x == 0) {
    int w = 0;
    for (int l = 1; l < nl; ++l)
      if (pots[l] < pots[w]) w = l;
    *winner = w;
    *index = cand[w];
  }
}

// m <- scratch[winner], and the float64 block partials of s * m that the
// next round's draw scans. x is not read.
__global__ void __launch_bounds__(NT)
seed_commit_kernel(const float* __restrict__ scratch,  // [nl][n]
                   const int* __restrict__ winner, int nl,
                   const float* __restrict__ s, float* __restrict__ m,
                   double* __restrict__ sm_part, int64_t n) {
  __shared__ double red[NT / WAVE];
  const int64_t e = (int64_t)blockIdx.x * SEED_BE + threadIdx.x;
  double p[1] = {0.0};
  if (e < n) {
    const int w = min(max(*winner, 0), nl - 1);
    const float v = scratch[(int64_t)w * n + e];
    m[e] = v;
    p[0] = (s != nullptr ? (double)s[e] : 1.0) * (double)v;
  }
  seed_block_sum<1>(p, 1, red, sm_part + blockIdx.x);
}

}  // namespace gmm
