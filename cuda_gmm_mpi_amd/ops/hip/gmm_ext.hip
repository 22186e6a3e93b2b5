// Host-side launchers + PyTorch bindings for the gfx950 GMM kernels.
#include <ATen/hip/HIPContext.h>
#include <torch/extension.h>

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#define HIP_CHECK(expr)                                                     \
  do {                                                                      \
    hipError_t _e = (expr);                                                 \
    TORCH_CHECK(_e == hipSuccess, "HIP error: ", hipGetErrorString(_e));    \
  } while (0)

#include "gmm_kernels.hip"

namespace {

constexpr int kNT = 256;

hipStream_t stream() { return at::hip::getCurrentHIPStream().stream(); }

void check_f32(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
                  t.scalar_type() == torch::kFloat32,
              name, " must be contiguous fp32 on device");
}

int grid_x_for(int64_t n) {
  // >> 256 workgroups to fill 8 XCDs x 32 CUs; cap so partial buffers and
  // tail-effect stay reasonable
  int64_t tiles = (n + kNT - 1) / kNT;
  return (int)std::min<int64_t>(tiles, 16384);
}


const float* lse_ptr(const torch::Tensor& lse, int64_t n) {
  if (lse.numel() == 0) return nullptr;
  TORCH_CHECK(lse.is_cuda() && lse.is_contiguous() &&
                  lse.scalar_type() == torch::kFloat32 && lse.numel() == n,
              "lse must be contiguous fp32 [N]");
  return lse.data_ptr<float>();
}

template <typename T>
const T* data_as(const torch::Tensor& t) {
  return reinterpret_cast<const T*>(t.data_ptr());
}

template <typename T>
void estep_logw_impl(const torch::Tensor& x, const torch::Tensor& means,
                     const torch::Tensor& rinv, const torch::Tensor& constant,
                     const torch::Tensor& logpi, torch::Tensor& logw,
                     bool diag_only) {
  const int d = (int)x.size(0);
  const int64_t n = x.size(1);
  const int k = (int)means.size(0);
  dim3 grid(grid_x_for(n), k);
  const int p = d * (d + 1) / 2;
  const size_t lds = sizeof(float) * (d + p);
  auto s = stream();
  const T* xp = data_as<T>(x);
  const float* mp = means.data_ptr<float>();
  const float* rp = rinv.data_ptr<float>();
  const float* cp = constant.data_ptr<float>();
  const float* lp = logpi.data_ptr<float>();
  float* op = logw.data_ptr<float>();

  if (diag_only) {
    const size_t lds_d = sizeof(float) * 2 * d;
    hipLaunchKernelGGL(gmm::estep_logw_diag_kernel<T>, grid, dim3(kNT), lds_d,
                       s, xp, mp, rp, cp, lp, op, d, n);
  } else if (d <= 8) {
    hipLaunchKernelGGL((gmm::estep_logw_reg_kernel<8, T>), grid, dim3(kNT),
                       lds, s, xp, mp, rp, cp, lp, op, d, n);
  } else if (d <= 16) {
    hipLaunchKernelGGL((gmm::estep_logw_reg_kernel<16, T>), grid, dim3(kNT),
                       lds, s, xp, mp, rp, cp, lp, op, d, n);
  } else if (d <= 24) {
    hipLaunchKernelGGL((gmm::estep_logw_reg_kernel<24, T>), grid, dim3(kNT),
                       lds, s, xp, mp, rp, cp, lp, op, d, n);
  } else if (d <= 32) {
    hipLaunchKernelGGL((gmm::estep_logw_reg_kernel<32, T>), grid, dim3(kNT),
                       lds, s, xp, mp, rp, cp, lp, op, d, n);
  } else {
    hipLaunchKernelGGL(gmm::estep_logw_gen_kernel<T>, grid, dim3(kNT), lds, s,
                       xp, mp, rp, cp, lp, op, d, n);
  }
  HIP_CHECK(hipGetLastError());
}

void estep_logw(torch::Tensor x, torch::Tensor means, torch::Tensor rinv,
                torch::Tensor constant, torch::Tensor logpi,
                torch::Tensor logw, bool diag_only) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous(), "x must be contiguous device");
  check_f32(means, "means");
  check_f32(rinv, "rinv");
  check_f32(constant, "constant");
  check_f32(logpi, "logpi");
  check_f32(logw, "logw");
  TORCH_CHECK(logw.size(0) == means.size(0) && logw.size(1) == x.size(1),
              "logw shape mismatch");
  if (x.scalar_type() == torch::kFloat32) {
    estep_logw_impl<float>(x, means, rinv, constant, logpi, logw, diag_only);
  } else if (x.scalar_type() == torch::kBFloat16) {
    estep_logw_impl<__hip_bfloat16>(x, means, rinv, constant, logpi, logw,
                                    diag_only);
  } else {
    TORCH_CHECK(false, "x must be fp32 or bf16");
  }
}

void estep_posteriors(torch::Tensor logw, torch::Tensor partial) {
  check_f32(logw, "logw");
  check_f32(partial, "partial");
  const int k = (int)logw.size(0);
  const int64_t n = logw.size(1);
  int grid = (int)std::min<int64_t>((n + kNT - 1) / kNT, partial.size(0));
  TORCH_CHECK(grid >= 1, "empty logw");
  // zero the tail of the partial buffer (grid may be < partial size)
  hipLaunchKernelGGL(gmm::estep_posteriors_kernel, dim3(grid), dim3(kNT), 0,
                     stream(), logw.data_ptr<float>(),
                     partial.data_ptr<float>(), k, n);
  HIP_CHECK(hipGetLastError());
}

void estep_lse(torch::Tensor logw, torch::Tensor lse,
               torch::Tensor partial) {
  check_f32(logw, "logw");
  check_f32(lse, "lse");
  check_f32(partial, "partial");
  const int k = (int)logw.size(0);
  const int64_t n = logw.size(1);
  TORCH_CHECK(lse.numel() == n, "lse must be [N]");
  int grid = (int)std::min<int64_t>((n + kNT - 1) / kNT, partial.size(0));
  TORCH_CHECK(grid >= 1, "empty logw");
  hipLaunchKernelGGL(gmm::estep_lse_kernel, dim3(grid), dim3(kNT), 0,
                     stream(), logw.data_ptr<float>(), lse.data_ptr<float>(),
                     partial.data_ptr<float>(), k, n);
  HIP_CHECK(hipGetLastError());
}

// Blocks event_weight_lse launches for n events: one per 4 * kNT events,
// capped (grid-stride beyond). The likelihood partial buffer has exactly
// this many slots, so reduce_scalar reads only slots a block has written.
int64_t event_weight_lse_blocks(int64_t n) {
  constexpr int64_t per_block = (int64_t)EW_VEC * kNT;
  return std::max<int64_t>(
      1, std::min<int64_t>((n + per_block - 1) / per_block, 2048));
}

void event_weight_lse(torch::Tensor lse, torch::Tensor s, torch::Tensor lns,
                      torch::Tensor lse_w, torch::Tensor partial) {
  check_f32(lse, "lse");
  check_f32(s, "s");
  check_f32(lns, "lns");
  check_f32(lse_w, "lse_w");
  check_f32(partial, "partial");
  const int64_t n = lse.numel();
  TORCH_CHECK(n >= 1, "empty lse");
  TORCH_CHECK(s.numel() == n && lns.numel() == n && lse_w.numel() == n,
              "s, lns and lse_w must be [N] like lse");
  const int64_t grid = event_weight_lse_blocks(n);
  // an empty partial switches the likelihood off (nothing is written)
  TORCH_CHECK(partial.numel() == 0 || partial.numel() == grid,
              "partial must be empty or [event_weight_lse_blocks(N)]");
  auto aligned = [](const torch::Tensor& t) {
    return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
  };
  const int64_t nvec = (aligned(lse) && aligned(s) && aligned(lns) &&
                        aligned(lse_w)) ? n / EW_VEC : 0;
  hipLaunchKernelGGL(gmm::event_weight_lse_kernel, dim3((unsigned)grid),
                     dim3(kNT), 0, stream(), lse.data_ptr<float>(),
                     s.data_ptr<float>(), lns.data_ptr<float>(),
                     lse_w.data_ptr<float>(),
                     partial.numel() ? partial.data_ptr<float>() : nullptr,
                     nvec, n);
  HIP_CHECK(hipGetLastError());
}

// background_lse: the geometry of event_weight_lse (one block per 4 * kNT
// events, capped). `bg` is the 4-float background state (bg[1] = b is read
// on the device); s / lns empty: unweighted; lse_b empty: not stored;
// partial is [blocks] (n0 only) or [2 * blocks] (n0, then the likelihood).
void background_lse(torch::Tensor lse, torch::Tensor bg, torch::Tensor s,
                    torch::Tensor lns, torch::Tensor lse_m,
                    torch::Tensor lse_b, torch::Tensor partial) {
  check_f32(lse, "lse");
  check_f32(bg, "bg");
  check_f32(s, "s");
  check_f32(lns, "lns");
  check_f32(lse_m, "lse_m");
  check_f32(lse_b, "lse_b");
  check_f32(partial, "partial");
  const int64_t n = lse.numel();
  TORCH_CHECK(n >= 1, "empty lse");
  TORCH_CHECK(bg.numel() == 4, "bg must be the 4-float background state");
  const bool weighted = s.numel() > 0;
  TORCH_CHECK(lse_m.numel() == n, "lse_m must be [N] like lse");
  TORCH_CHECK((!weighted && lns.numel() == 0) ||
                  (s.numel() == n && lns.numel() == n),
              "s and lns must both be empty or [N] like lse");
  TORCH_CHECK(lse_b.numel() == 0 || lse_b.numel() == n,
              "lse_b must be empty or [N] like lse");
  const int64_t grid = event_weight_lse_blocks(n);
  TORCH_CHECK(partial.numel() == grid || partial.numel() == 2 * grid,
              "partial must be [blocks] or [2 * blocks], blocks = "
              "event_weight_lse_blocks(N)");
  auto aligned = [](const torch::Tensor& t) {
    return t.numel() == 0 ||
           reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
  };
  const int64_t nvec = (aligned(lse) && aligned(s) && aligned(lns) &&
                        aligned(lse_m) && aligned(lse_b)) ? n / EW_VEC : 0;
  float* pp = partial.data_ptr<float>();
  float* lik_part = partial.numel() == 2 * grid ? pp + grid : nullptr;
  float* lbp = lse_b.numel() ? lse_b.data_ptr<float>() : nullptr;
  if (weighted) {
    hipLaunchKernelGGL(gmm::background_lse_kernel<true>,
                       dim3((unsigned)grid), dim3(kNT), 0, stream(),
                       lse.data_ptr<float>(), bg.data_ptr<float>(),
                       s.data_ptr<float>(), lns.data_ptr<float>(),
                       lse_m.data_ptr<float>(), lbp, pp, lik_part, nvec, n);
  } else {
    hipLaunchKernelGGL(gmm::background_lse_kernel<false>,
                       dim3((unsigned)grid), dim3(kNT), 0, stream(),
                       lse.data_ptr<float>(), bg.data_ptr<float>(),
                       (const float*)nullptr, (const float*)nullptr,
                       lse_m.data_ptr<float>(), lbp, pp, lik_part, nvec, n);
  }
  HIP_CHECK(hipGetLastError());
}

// bg <- (pi0, b, lik_add, n0) from the first `nparts` entries of n0_part.
void background_update(torch::Tensor n0_part, int64_t nparts, double n_total,
                       double ln_v, torch::Tensor bg) {
  check_f32(n0_part, "n0_part");
  check_f32(bg, "bg");
  TORCH_CHECK(bg.numel() == 4, "bg must be the 4-float background state");
  TORCH_CHECK(nparts >= 1 && nparts <= n0_part.numel(),
              "nparts must be in 1..n0_part.numel()");
  TORCH_CHECK(n_total > 0.0, "n_total must be positive");
  hipLaunchKernelGGL(gmm::background_update_kernel, dim3(1), dim3(kNT), 0,
                     stream(), n0_part.data_ptr<float>(), nparts, n_total,
                     ln_v, bg.data_ptr<float>());
  HIP_CHECK(hipGetLastError());
}

// Blocks student_t_lse launches for n events: one per tile of 4 * kNT
// events, capped (the blocks walk further tiles in order). n_part has
// exactly this many rows of K, lik_part this many slots.
int64_t student_t_lse_blocks(int64_t n) { return event_weight_lse_blocks(n); }

// student_t_lse over logw [K, N] in place. train: logw <- lt + ln u, lse_m,
// lse_t, n_part [blocks, K] and (unless empty) lik_part [blocks]; s / lns
// empty: unweighted. Posterior (train false): logw <- lt and lse_t only;
// s, lns, lse_m, n_part and lik_part must be empty.
void student_t_lse(torch::Tensor logw, torch::Tensor add, torch::Tensor s,
                   torch::Tensor lns, torch::Tensor lse_m,
                   torch::Tensor lse_t, torch::Tensor n_part,
                   torch::Tensor lik_part, double nu, int64_t d,
                   double delta, bool train) {
  check_f32(logw, "logw");
  check_f32(add, "add");
  check_f32(s, "s");
  check_f32(lns, "lns");
  check_f32(lse_m, "lse_m");
  check_f32(lse_t, "lse_t");
  check_f32(n_part, "n_part");
  check_f32(lik_part, "lik_part");
  TORCH_CHECK(logw.dim() == 2 && logw.numel() >= 1, "logw must be [K, N]");
  const int64_t k = logw.size(0);
  const int64_t n = logw.size(1);
  TORCH_CHECK(nu > 0.0 && std::isfinite(nu) && d >= 1 && std::isfinite(delta),
              "student_t_lse needs finite nu > 0, D >= 1 and a finite delta");
  // the LDS table of per-wave cluster sums: 4 rows of K floats
  TORCH_CHECK(k <= 2048, "student_t_lse supports K <= 2048, got ", k);
  TORCH_CHECK(add.numel() == k, "add must be [K]");
  TORCH_CHECK(lse_t.numel() == n, "lse_t must be [N]");
  const bool weighted = s.numel() > 0;
  const int64_t grid = student_t_lse_blocks(n);
  if (train) {
    TORCH_CHECK(lse_m.numel() == n, "lse_m must be [N]");
    TORCH_CHECK((!weighted && lns.numel() == 0) ||
                    (s.numel() == n && lns.numel() == n),
                "s and lns must both be empty or [N]");
    TORCH_CHECK(n_part.numel() == grid * k,
                "n_part must be [student_t_lse_blocks(N), K]");
    TORCH_CHECK(lik_part.numel() == 0 || lik_part.numel() == grid,
                "lik_part must be empty or [student_t_lse_blocks(N)]");
  } else {
    TORCH_CHECK(s.numel() == 0 && lns.numel() == 0 && lse_m.numel() == 0 &&
                    n_part.numel() == 0 && lik_part.numel() == 0,
                "posterior mode takes logw, add and lse_t only");
  }
  auto aligned = [](const torch::Tensor& t) {
    return t.numel() == 0 ||
           reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
  };
  // n % 4 == 0 keeps every cluster row of logw 16-byte aligned
  const int64_t nvec = (n % EW_VEC == 0 && aligned(logw) && aligned(s) &&
                        aligned(lns) && aligned(lse_m) && aligned(lse_t))
                           ? n / EW_VEC : 0;
  auto ptr = [](torch::Tensor& t) {
    return t.numel() ? t.data_ptr<float>() : (float*)nullptr;
  };
  const size_t lds = train ? sizeof(float) * (kNT / 64) * k : 0;
  const float nuf = (float)nu, nud = (float)(nu + (double)d),
              df = (float)delta;
#define ST_LAUNCH(W, TRAIN)                                                  \
  hipLaunchKernelGGL((gmm::student_t_lse_kernel<W, TRAIN>),                  \
                     dim3((unsigned)grid), dim3(kNT), lds, stream(),         \
                     logw.data_ptr<float>(), add.data_ptr<float>(), ptr(s),  \
                     ptr(lns), ptr(lse_m), lse_t.data_ptr<float>(),          \
                     ptr(n_part), ptr(lik_part), (int)k, nvec, n, nuf, nud,  \
                     df)
  if (!train) {
    ST_LAUNCH(false, false);
  } else if (weighted) {
    ST_LAUNCH(true, true);
  } else {
    ST_LAUNCH(false, true);
  }
#undef ST_LAUNCH
  HIP_CHECK(hipGetLastError());
}

// N and pi (and add = constant + ln pi unless `add` is empty) of a t fit
// from the reduced responsibilities n_c [K].
void student_t_pi(torch::Tensor n_c, torch::Tensor constant,
                  torch::Tensor n_out, torch::Tensor pi, torch::Tensor add) {
  check_f32(n_c, "n_c");
  check_f32(constant, "constant");
  check_f32(n_out, "n_out");
  check_f32(pi, "pi");
  check_f32(add, "add");
  const int64_t k = n_c.numel();
  TORCH_CHECK(k >= 1 && n_out.numel() == k && pi.numel() == k,
              "n_c, N and pi must be [K]");
  TORCH_CHECK(add.numel() == 0 || (add.numel() == k && constant.numel() == k),
              "add must be empty or [K] with constant [K]");
  hipLaunchKernelGGL(gmm::student_t_pi_kernel, dim3(1), dim3(kNT), 0,
                     stream(), n_c.data_ptr<float>(),
                     add.numel() ? constant.data_ptr<float>()
                                 : (const float*)nullptr,
                     n_out.data_ptr<float>(), pi.data_ptr<float>(),
                     add.numel() ? add.data_ptr<float>() : (float*)nullptr,
                     (int)k);
  HIP_CHECK(hipGetLastError());
}

template <typename T>
void mstep_cov_impl(const torch::Tensor& x, const torch::Tensor& w,
                    const torch::Tensor& lse, torch::Tensor& partials) {
  const int d = (int)x.size(0);
  const int64_t n = x.size(1);
  const int k = (int)w.size(0);
  const int nchunk = (int)partials.size(0);
  const int p = d * (d + 1) / 2;
  TORCH_CHECK(partials.size(1) == k && partials.size(2) == p,
              "partials must be [nchunk, K, D*(D+1)/2]");
  // largest event tile (multiple of 4) fitting the 64 KiB LDS budget:
  // d*(te+4) + te floats  <=  16384
  int te = (16384 - 4 * d) / (d + 1);
  te = std::min(te & ~3, 256);
  TORCH_CHECK(te >= 32, "D too large for covariance tile");
  const size_t lds = sizeof(float) * ((size_t)d * (te + 4) + te);
  dim3 grid(k, nchunk);
  auto s = stream();
  const int ppt = (p + kNT - 1) / kNT;
  const T* xp = data_as<T>(x);
  const float* wp = w.data_ptr<float>();
  const float* lp = lse_ptr(lse, n);
  float* pp = partials.data_ptr<float>();
#define LAUNCH_COV(PPT)                                                     \
  hipLaunchKernelGGL((gmm::mstep_cov_kernel<PPT, T>), grid, dim3(kNT), lds, \
                     s, xp, wp, lp, pp, d, k, n, te, nchunk)
  if (ppt <= 1) LAUNCH_COV(1);
  else if (ppt <= 2) LAUNCH_COV(2);
  else if (ppt <= 4) LAUNCH_COV(4);
  else if (ppt <= 8) LAUNCH_COV(8);
  else if (ppt <= 17) LAUNCH_COV(17);
  else if (ppt <= 33) LAUNCH_COV(33);
  else TORCH_CHECK(false, "D too large for covariance kernel (max 128)");
#undef LAUNCH_COV
  HIP_CHECK(hipGetLastError());
}

void mstep_covariance_partials(torch::Tensor x, torch::Tensor w,
                               torch::Tensor lse, torch::Tensor partials) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous(), "x must be contiguous device");
  check_f32(w, "w");
  check_f32(partials, "partials");
  if (x.scalar_type() == torch::kFloat32) {
    mstep_cov_impl<float>(x, w, lse, partials);
  } else if (x.scalar_type() == torch::kBFloat16) {
    mstep_cov_impl<__hip_bfloat16>(x, w, lse, partials);
  } else {
    TORCH_CHECK(false, "x must be fp32 or bf16");
  }
}

// The factor emission gives thread i row i of the factorization and stores
// 8 cells at a time: D within one block, 16-byte aligned factor tables.
void check_factor_out(const torch::Tensor& mfac, const torch::Tensor& mfac32,
                      int d) {
  TORCH_CHECK(d <= kNT, "factor emission needs D <= ", kNT);
  TORCH_CHECK(mfac.numel() == 0 ||
                  reinterpret_cast<uintptr_t>(mfac.data_ptr()) % 16 == 0,
              "mfac must be 16-byte aligned");
  TORCH_CHECK(mfac32.numel() == 0 ||
                  reinterpret_cast<uintptr_t>(mfac32.data_ptr()) % 16 == 0,
              "mfac32 must be 16-byte aligned");
}

void constants(torch::Tensor r, torch::Tensor means, torch::Tensor pi,
               torch::Tensor rinv, torch::Tensor logdet,
               torch::Tensor constant, torch::Tensor add, torch::Tensor mfac,
               torch::Tensor mfac32, bool diag_only) {
  check_f32(r, "r");
  check_f32(means, "means");
  check_f32(rinv, "rinv");
  check_f32(logdet, "logdet");
  const int k = (int)r.size(0);
  const int d = (int)r.size(1);
  const bool make_mfac = mfac.numel() > 0;
  __hip_bfloat16* mp = nullptr;
  float* mp32 = nullptr;
  if (mfac32.numel() > 0) {
    TORCH_CHECK(mfac32.is_cuda() && mfac32.is_contiguous() &&
                    mfac32.scalar_type() == torch::kFloat32,
                "mfac32 must be contiguous fp32");
    mp32 = mfac32.data_ptr<float>();
  }
  if (make_mfac) {
    const int rows = gmm::mfac_rows(d);
    const int kct = gmm::mfac_kct(d);
    TORCH_CHECK(mfac.is_cuda() && mfac.is_contiguous() &&
                    mfac.scalar_type() == torch::kBFloat16 &&
                    mfac.numel() == (int64_t)k * 2 * rows * kct * 16 &&
                    d <= 142,
                "mfac must be bf16 [K,2,RT*32,KCT*16] with D <= 142");
    mp = reinterpret_cast<__hip_bfloat16*>(mfac.data_ptr());
    check_factor_out(mfac, mfac32, d);
  }
  auto s = stream();
  float* pip = pi.numel() > 0 ? pi.data_ptr<float>() : nullptr;
  float* cst = constant.numel() > 0 ? constant.data_ptr<float>() : nullptr;
  float* addp = add.numel() > 0 ? add.data_ptr<float>() : nullptr;
  TORCH_CHECK(addp == nullptr || pip != nullptr, "add output requires pi");
  if (diag_only) {
    hipLaunchKernelGGL(gmm::constants_diag_kernel, dim3(k), dim3(kNT), 0, s,
                       r.data_ptr<float>(), rinv.data_ptr<float>(),
                       logdet.data_ptr<float>(), d);
    if (make_mfac) {
      // diag R is a valid input to the generic factor path (diagonal
      // Cholesky); emit from R via the standalone kernel
      hipLaunchKernelGGL(gmm::emit_mfac_from_r_kernel, dim3(k), dim3(kNT),
                         sizeof(float) * (2 * (size_t)d * (d | 1) + d), s,
                         r.data_ptr<float>(), means.data_ptr<float>(), mp,
                         mp32, d, nullptr, nullptr, nullptr);
    }
  } else {
    // working buffer + read-only LU snapshot (+ u0 scratch for the factor)
    const size_t lds = sizeof(float) * (2 * (size_t)d * (d | 1) + d);
    if (lds > 64 * 1024) {  // gfx950: 160 KiB LDS/CU; opt in past 64 KiB
      HIP_CHECK(hipFuncSetAttribute(
          reinterpret_cast<const void*>(&gmm::constants_lu_kernel),
          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    hipLaunchKernelGGL(gmm::constants_lu_kernel, dim3(k), dim3(kNT),
                       lds, s, r.data_ptr<float>(), means.data_ptr<float>(),
                       pip, rinv.data_ptr<float>(), logdet.data_ptr<float>(),
                       cst, addp, mp, mp32, d);
  }
  HIP_CHECK(hipGetLastError());
}

void mstep_moments(torch::Tensor x, torch::Tensor w, torch::Tensor lse,
                   torch::Tensor partials) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() &&
                  x.scalar_type() == torch::kFloat32,
              "x must be contiguous fp32 (exact M-step)");
  check_f32(w, "w");
  check_f32(partials, "partials");
  const int d = (int)x.size(0);
  const int64_t n = x.size(1);
  const int k = (int)w.size(0);
  const int nchunk = (int)partials.size(0);
  const int dp = d + 1;
  TORCH_CHECK(d <= 31, "mstep_moments fast path needs D <= 31");
  TORCH_CHECK(partials.size(1) == k &&
                  partials.size(2) == dp * (dp + 1) / 2,
              "partials must be [nchunk, K, Dp*(Dp+1)/2]");
  const size_t lds = 2 * sizeof(float) * ((size_t)d * (128 + 4) + 4 * 128);
  dim3 grid((k + 3) / 4, nchunk);
  hipLaunchKernelGGL((gmm::mstep_moments_kernel<float>), grid, dim3(kNT), lds,
                     stream(), x.data_ptr<float>(), w.data_ptr<float>(),
                     lse_ptr(lse, n), partials.data_ptr<float>(), d, k, n,
                     nchunk);
  HIP_CHECK(hipGetLastError());
}

void mstep_moments_b16(torch::Tensor xhi, torch::Tensor xlo,
                       torch::Tensor w, torch::Tensor lse,
                       torch::Tensor partials) {
  TORCH_CHECK(xhi.is_cuda() && xhi.is_contiguous() && xlo.is_contiguous() &&
                  xhi.scalar_type() == torch::kBFloat16 &&
                  xlo.scalar_type() == torch::kBFloat16,
              "xhi/xlo must be contiguous bf16 planes");
  check_f32(w, "w");
  check_f32(partials, "partials");
  const int d = (int)xhi.size(0);
  const int64_t n = xhi.size(1);
  const int k = (int)w.size(0);
  const int nchunk = (int)partials.size(0);
  const int dp = d + 1;
  TORCH_CHECK(d <= 31, "mstep_moments_b16 needs D <= 31");
  TORCH_CHECK(partials.size(1) == k &&
                  partials.size(2) == dp * (dp + 1) / 2,
              "partials must be [nchunk, K, Dp*(Dp+1)/2]");
  // two buffers x (zhi+zlo planes + w tiles for 8 clusters)
  const size_t lds = 2 * (2 * 32 * 136 * 2 + 8 * 128 * 4);
  dim3 grid((k + 7) / 8, nchunk);
  hipLaunchKernelGGL(gmm::mstep_moments_b16_kernel, grid, dim3(512), lds,
                     stream(),
                     reinterpret_cast<const __hip_bfloat16*>(xhi.data_ptr()),
                     reinterpret_cast<const __hip_bfloat16*>(xlo.data_ptr()),
                     w.data_ptr<float>(), lse_ptr(lse, n),
                     partials.data_ptr<float>(), d, k, n, nchunk);
  HIP_CHECK(hipGetLastError());
}

template <int TPW, int NCT>
void launch_moments_pair(int nchunk, const torch::Tensor& xhi,
                         const torch::Tensor& xlo, const torch::Tensor& w,
                         const float* lse, torch::Tensor& partials, int d,
                         int k, int64_t n) {
  constexpr size_t lds = 2 * MP_BUF_BYTES(NCT);  // double-buffered, > 64 KB
  dim3 grid((k + 16 * NCT - 1) / (16 * NCT), nchunk);
  HIP_CHECK(hipFuncSetAttribute(
      reinterpret_cast<const void*>(
          &gmm::mstep_moments_pair_b16_kernel<TPW, NCT>),
      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((gmm::mstep_moments_pair_b16_kernel<TPW, NCT>), grid,
                     dim3(MP_NT), lds, stream(),
                     reinterpret_cast<const __hip_bfloat16*>(xhi.data_ptr()),
                     reinterpret_cast<const __hip_bfloat16*>(xlo.data_ptr()),
                     w.data_ptr<float>(), lse, partials.data_ptr<float>(), d,
                     k, n, nchunk);
}

void mstep_moments_pair_b16(torch::Tensor xhi, torch::Tensor xlo,
                            torch::Tensor w, torch::Tensor lse,
                            torch::Tensor partials) {
  TORCH_CHECK(xhi.is_cuda() && xhi.is_contiguous() && xlo.is_cuda() &&
                  xlo.is_contiguous() &&
                  xhi.scalar_type() == torch::kBFloat16 &&
                  xlo.scalar_type() == torch::kBFloat16 &&
                  xlo.sizes() == xhi.sizes() && xhi.dim() == 2,
              "xhi/xlo must be contiguous bf16 [D, N] planes");
  check_f32(w, "w");
  check_f32(partials, "partials");
  const int d = (int)xhi.size(0);
  const int64_t n = xhi.size(1);
  const int k = (int)w.size(0);
  TORCH_CHECK(partials.dim() == 3 && partials.size(0) >= 1,
              "partials must be [nchunk, K, Dp*(Dp+1)/2]");
  const int nchunk = (int)partials.size(0);
  const int dp = d + 1;
  const int pp = dp * (dp + 1) / 2;
  TORCH_CHECK(d >= 1 && d <= 31, "mstep_moments_pair_b16 needs 1 <= D <= 31");
  TORCH_CHECK(w.dim() == 2 && w.size(1) == n && k >= 1 && n >= 1,
              "w must be [K, N]");
  TORCH_CHECK(partials.size(1) == k && partials.size(2) == pp,
              "partials must be [nchunk, K, Dp*(Dp+1)/2]");
  TORCH_CHECK(nchunk <= 65535, "nchunk must fit gridDim.y");
  const float* lp = lse_ptr(lse, n);
  // 16-column pair tiles over 8 waves: tiles per wave (<= 5 at D <= 31);
  // 64 clusters per block up to 3 tiles per wave, 32 above
  const int tpw = ((pp + 15) / 16 + 7) / 8;
  switch (tpw) {
    case 1: launch_moments_pair<1, 4>(nchunk, xhi, xlo, w, lp, partials, d, k, n); break;
    case 2: launch_moments_pair<2, 4>(nchunk, xhi, xlo, w, lp, partials, d, k, n); break;
    case 3: launch_moments_pair<3, 4>(nchunk, xhi, xlo, w, lp, partials, d, k, n); break;
    case 4: launch_moments_pair<4, 2>(nchunk, xhi, xlo, w, lp, partials, d, k, n); break;
    default: launch_moments_pair<5, 2>(nchunk, xhi, xlo, w, lp, partials, d, k, n); break;
  }
  HIP_CHECK(hipGetLastError());
}

void exp_sub_lse(torch::Tensor logw, torch::Tensor lse, torch::Tensor out) {
  check_f32(logw, "logw");
  check_f32(out, "out");
  TORCH_CHECK(logw.dim() == 2 && out.sizes() == logw.sizes(),
              "logw/out must be [K, N]");
  const int k = (int)logw.size(0);
  const int64_t n = logw.size(1);
  const float* lp = lse_ptr(lse, n);
  TORCH_CHECK(lp != nullptr, "lse must be [N]");
  hipLaunchKernelGGL(gmm::exp_sub_lse_kernel, dim3(grid_x_for((int64_t)k * n)),
                     dim3(kNT), 0, stream(), logw.data_ptr<float>(), lp,
                     out.data_ptr<float>(), k, n);
  HIP_CHECK(hipGetLastError());
}

// The five fused small-D E-step entry points: z [D,N] and the factor table
// in the precision of Fac, add [K], w_out [K,N], one partial per block of
// `tile` events.
struct FusedShape {
  int d, k;
  int64_t n, nblk;
};

template <typename Fac>
FusedShape check_fused(const char* name, const torch::Tensor& z,
                       const torch::Tensor& fac, const torch::Tensor& add,
                       const torch::Tensor& w_out,
                       const torch::Tensor& partial, int tile) {
  constexpr bool f32 = std::is_same<typename Fac::In, float>::value;
  const auto dt = f32 ? torch::kFloat32 : torch::kBFloat16;
  const char* dtn = f32 ? "fp32" : "bf16";
  TORCH_CHECK(z.is_cuda() && z.is_contiguous() && z.scalar_type() == dt &&
                  z.dim() == 2,
              name, ": z must be contiguous ", dtn, " [D,N] on device");
  TORCH_CHECK(fac.is_cuda() && fac.is_contiguous() && fac.scalar_type() == dt,
              name, ": factor table must be contiguous ", dtn, " on device");
  check_f32(add, "add");
  check_f32(w_out, "w_out");
  check_f32(partial, "partial");
  FusedShape s;
  s.d = (int)z.size(0);
  s.n = z.size(1);
  s.k = (int)add.size(0);
  s.nblk = (s.n + tile - 1) / tile;
  TORCH_CHECK(s.d >= 1 && s.d <= 31, name, " needs 1 <= D <= 31");
  TORCH_CHECK(s.k >= 1 && s.n >= 1, name, " needs K >= 1 and N >= 1");
  TORCH_CHECK(fac.numel() >= (int64_t)s.k * Fac::CELLS, name,
              ": factor table too small");
  TORCH_CHECK(w_out.dim() == 2 && w_out.size(0) == s.k &&
                  w_out.size(1) == s.n,
              name, ": w_out must be [K,N]");
  TORCH_CHECK(partial.size(0) >= s.nblk, name, ": partial buffer too small");
  return s;
}

// LDS bytes of the lw-in-LDS kernels at K clusters, checked against 64 KB
template <typename Fac>
size_t fused_lds_budget(const char* name, int k) {
  const size_t lds = gmm::estl_lds_bytes<Fac>(k);
  TORCH_CHECK(lds <= 64 * 1024, name, " LDS budget exceeded (K too big)");
  return lds;
}

template <typename Fac, typename Kernel>
void launch_fused_lse(const char* name, Kernel kernel, const torch::Tensor& z,
                      const torch::Tensor& fac, const torch::Tensor& add,
                      torch::Tensor& w_out, torch::Tensor& lse_out,
                      torch::Tensor& partial) {
  using In = typename Fac::In;
  const FusedShape s =
      check_fused<Fac>(name, z, fac, add, w_out, partial, gmm::EST_BE);
  check_f32(lse_out, "lse_out");
  TORCH_CHECK(lse_out.numel() == s.n, name, ": lse_out must be [N]");
  hipLaunchKernelGGL(kernel, dim3((uint32_t)s.nblk), dim3(kNT),
                     gmm::est_lds_bytes<Fac>(), stream(), data_as<In>(z),
                     data_as<In>(fac), add.data_ptr<float>(),
                     w_out.data_ptr<float>(), lse_out.data_ptr<float>(),
                     partial.data_ptr<float>(), s.d, s.k, s.n);
  HIP_CHECK(hipGetLastError());
}

void estep_fused(torch::Tensor z, torch::Tensor mfac, torch::Tensor add,
                 torch::Tensor w_out, torch::Tensor lse_out,
                 torch::Tensor partial) {
  launch_fused_lse<gmm::FacB16>("estep_fused", gmm::estep_fused_kernel, z,
                                mfac, add, w_out, lse_out, partial);
}

void estep_fused_f32(torch::Tensor z, torch::Tensor mfac32,
                     torch::Tensor add, torch::Tensor w_out,
                     torch::Tensor lse_out, torch::Tensor partial) {
  launch_fused_lse<gmm::FacF32>("estep_fused_f32",
                                gmm::estep_fused_f32_kernel, z, mfac32, add,
                                w_out, lse_out, partial);
}

template <typename Fac, typename Kernel>
void launch_fused_lds(const char* name, Kernel kernel, const torch::Tensor& z,
                      const torch::Tensor& fac, const torch::Tensor& add,
                      torch::Tensor& w_out, torch::Tensor& partial) {
  using In = typename Fac::In;
  const FusedShape s =
      check_fused<Fac>(name, z, fac, add, w_out, partial, gmm::ESTL_BE);
  const size_t lds = fused_lds_budget<Fac>(name, s.k);
  hipLaunchKernelGGL(kernel, dim3((uint32_t)s.nblk), dim3(kNT), lds,
                     stream(), data_as<In>(z), data_as<In>(fac),
                     add.data_ptr<float>(), w_out.data_ptr<float>(),
                     partial.data_ptr<float>(), s.d, s.k, s.n);
  HIP_CHECK(hipGetLastError());
}

void estep_fused_lds(torch::Tensor z, torch::Tensor mfac, torch::Tensor add,
                     torch::Tensor w_out, torch::Tensor partial) {
  launch_fused_lds<gmm::FacB16>("estep_fused_lds",
                                gmm::estep_fused_lds_kernel, z, mfac, add,
                                w_out, partial);
}

void estep_fused_f32_lds(torch::Tensor z, torch::Tensor mfac32,
                         torch::Tensor add, torch::Tensor w_out,
                         torch::Tensor partial) {
  launch_fused_lds<gmm::FacF32>("estep_fused_f32_lds",
                                gmm::estep_fused_f32_lds_kernel, z, mfac32,
                                add, w_out, partial);
}

// Same contract and LDS budget as estep_fused_lds; the default small-K path.
void estep_fused_lds2(torch::Tensor z, torch::Tensor mfac, torch::Tensor add,
                      torch::Tensor w_out, torch::Tensor partial) {
  const char* name = "estep_fused_lds2";
  const FusedShape s = check_fused<gmm::FacB16>(name, z, mfac, add, w_out,
                                                partial, gmm::ESTL_BE);
  // 16-byte posterior stores need every row start 16-byte aligned
  const int vec4 = s.n % 4 == 0 &&
                   reinterpret_cast<uintptr_t>(w_out.data_ptr()) % 16 == 0;
  const size_t lds = fused_lds_budget<gmm::FacB16>(name, s.k);
  // the kernel sums only the accumulator registers that hold factor rows
  // below d (groups of 8 rows): chosen here, so its cluster loop has no
  // branch on it
#define LAUNCH_LDS2(NL)                                                      \
  hipLaunchKernelGGL(gmm::estep_fused_lds2_kernel<NL>,                       \
                     dim3((uint32_t)s.nblk), dim3(kNT), lds, stream(),       \
                     data_as<__hip_bfloat16>(z),                             \
                     data_as<__hip_bfloat16>(mfac), add.data_ptr<float>(),   \
                     w_out.data_ptr<float>(), partial.data_ptr<float>(),     \
                     s.d, s.k, s.n, vec4)
  if (s.d <= 8) LAUNCH_LDS2(4);
  else if (s.d <= 16) LAUNCH_LDS2(8);
  else if (s.d <= 24) LAUNCH_LDS2(12);
  else LAUNCH_LDS2(16);
#undef LAUNCH_LDS2
  HIP_CHECK(hipGetLastError());
}

// The classify entry points: x event-major fp32 [N,D], center [D], the
// factor table in the precision of Fac, add [K]; label int32 [N], lse and
// pmax fp32 [N]. One block per 256 events, nothing else written.
template <typename Fac, typename Kernel>
void launch_classify(const char* name, Kernel kernel, const torch::Tensor& x,
                     const torch::Tensor& center, const torch::Tensor& fac,
                     const torch::Tensor& add, torch::Tensor& label,
                     torch::Tensor& lse, torch::Tensor& pmax) {
  using In = typename Fac::In;
  constexpr bool f32 = std::is_same<In, float>::value;
  const auto dt = f32 ? torch::kFloat32 : torch::kBFloat16;
  const char* dtn = f32 ? "fp32" : "bf16";
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() &&
                  x.scalar_type() == torch::kFloat32 && x.dim() == 2,
              name, ": x must be contiguous fp32 [N,D] on device");
  TORCH_CHECK(fac.is_cuda() && fac.is_contiguous() && fac.scalar_type() == dt,
              name, ": factor table must be contiguous ", dtn, " on device");
  check_f32(center, "center");
  check_f32(add, "add");
  check_f32(lse, "lse");
  check_f32(pmax, "pmax");
  TORCH_CHECK(label.is_cuda() && label.is_contiguous() &&
                  label.scalar_type() == torch::kInt32,
              name, ": label must be contiguous int32 on device");
  const int64_t n = x.size(0);
  const int64_t d64 = x.size(1);
  const int64_t k64 = add.numel();
  TORCH_CHECK(d64 >= 1 && d64 <= 31, name, " needs 1 <= D <= 31");
  TORCH_CHECK(k64 >= 1 && k64 <= INT32_MAX && n >= 1, name,
              " needs K >= 1 and N >= 1");
  TORCH_CHECK(center.numel() == d64, name, ": center must be [D]");
  TORCH_CHECK(fac.numel() >= k64 * Fac::CELLS, name,
              ": factor table too small");
  TORCH_CHECK(label.numel() == n && lse.numel() == n && pmax.numel() == n,
              name, ": label, lse and pmax must be [N]");
  const int64_t nblk = (n + gmm::EST_BE - 1) / gmm::EST_BE;
  TORCH_CHECK(nblk <= INT32_MAX, name, ": N too large for one launch");
  hipLaunchKernelGGL(kernel, dim3((uint32_t)nblk), dim3(kNT),
                     gmm::cls_lds_bytes<Fac>(), stream(),
                     x.data_ptr<float>(), center.data_ptr<float>(),
                     data_as<In>(fac), add.data_ptr<float>(),
                     label.data_ptr<int>(), lse.data_ptr<float>(),
                     pmax.data_ptr<float>(), (int)d64, (int)k64, n);
  HIP_CHECK(hipGetLastError());
}

void estep_classify(torch::Tensor x, torch::Tensor center, torch::Tensor mfac,
                    torch::Tensor add, torch::Tensor label, torch::Tensor lse,
                    torch::Tensor pmax) {
  launch_classify<gmm::FacB16>("estep_classify", gmm::estep_classify_kernel,
                               x, center, mfac, add, label, lse, pmax);
}

void estep_classify_f32(torch::Tensor x, torch::Tensor center,
                        torch::Tensor mfac32, torch::Tensor add,
                        torch::Tensor label, torch::Tensor lse,
                        torch::Tensor pmax) {
  launch_classify<gmm::FacF32>("estep_classify_f32",
                               gmm::estep_classify_f32_kernel, x, center,
                               mfac32, add, label, lse, pmax);
}

// Greedy k-means++ seeding (seed_kmeanspp.hip). One block per 256 events;
// the block-partial buffers have exactly this many rows.
int64_t seed_kmeanspp_blocks(int64_t n) {
  return (n + gmm::SEED_BE - 1) / gmm::SEED_BE;
}

// Stages of a round, as bits of `stages`.
constexpr int64_t kSeedSample = 1, kSeedEvaluate = 2, kSeedChoose = 4,
                  kSeedCommit = 8;

// Enqueue the selected stages of rounds [t0, t1) on the current stream; no
// synchronisation, nothing is read back. x fp32 [N,D] event-major, s fp32 [N]
// or empty (unweighted), u float64 [K,8] uniforms. Work buffers: m fp32 [N],
// scratch fp32 [L,N], pot_part float64 [blocks,8], sm_part / s_part float64
// [blocks]. Per-round record: cand int64 [K,8] (round t draws into row t, or
// the caller fills it when the sample stage is left out), winner int32 [K],
// index int64 [K], pots float64 [K,8]. Round 0 has one candidate; rounds
// >= 1 have L. With all stages, rounds [0, K) are the whole seeding.
void seed_kmeanspp_rounds(torch::Tensor x, torch::Tensor s, torch::Tensor u,
                          torch::Tensor m, torch::Tensor scratch,
                          torch::Tensor pot_part, torch::Tensor sm_part,
                          torch::Tensor s_part, torch::Tensor cand,
                          torch::Tensor winner, torch::Tensor index,
                          torch::Tensor pots, int64_t t0, int64_t t1,
                          int64_t stages) {
  auto check = [](const torch::Tensor& t, torch::ScalarType dt,
                  const char* name) {
    TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.scalar_type() == dt,
                "seed_kmeanspp: ", name,
                " must be contiguous on device with the documented dtype");
  };
  check(x, torch::kFloat32, "x");
  check(u, torch::kFloat64, "u");
  check(m, torch::kFloat32, "m");
  check(scratch, torch::kFloat32, "scratch");
  check(pot_part, torch::kFloat64, "pot_part");
  check(sm_part, torch::kFloat64, "sm_part");
  check(s_part, torch::kFloat64, "s_part");
  check(cand, torch::kInt64, "cand");
  check(winner, torch::kInt32, "winner");
  check(index, torch::kInt64, "index");
  check(pots, torch::kFloat64, "pots");
  TORCH_CHECK(x.dim() == 2 && x.size(0) >= 1 && x.size(1) >= 1 &&
                  x.size(1) <= INT32_MAX,
              "seed_kmeanspp: x must be [N,D] with N, D >= 1");
  const int64_t n = x.size(0);
  const int d = (int)x.size(1);
  const int64_t nblk = seed_kmeanspp_blocks(n);
  TORCH_CHECK(nblk <= INT32_MAX, "seed_kmeanspp: N too large for one launch");
  const float* sp = nullptr;
  if (s.numel() != 0) {
    check(s, torch::kFloat32, "s");
    TORCH_CHECK(s.numel() == n, "seed_kmeanspp: s must be [N]");
    sp = s.data_ptr<float>();
  }
  TORCH_CHECK(scratch.dim() == 2 && scratch.size(1) == n &&
                  scratch.size(0) >= 1 && scratch.size(0) <= gmm::SEED_LMAX,
              "seed_kmeanspp: scratch must be [L,N] with 1 <= L <= 8");
  const int nl = (int)scratch.size(0);
  const int64_t k = u.dim() == 2 ? u.size(0) : 0;
  TORCH_CHECK(k >= 1 && u.size(1) == gmm::SEED_LMAX,
              "seed_kmeanspp: u must be [K,8]");
  TORCH_CHECK(m.numel() == n, "seed_kmeanspp: m must be [N]");
  TORCH_CHECK(pot_part.numel() == nblk * gmm::SEED_LMAX &&
                  sm_part.numel() == nblk && s_part.numel() == nblk,
              "seed_kmeanspp: partial buffers must have "
              "seed_kmeanspp_blocks(N) rows");
  TORCH_CHECK(cand.numel() == k * gmm::SEED_LMAX &&
                  pots.numel() == k * gmm::SEED_LMAX && winner.numel() == k &&
                  index.numel() == k,
              "seed_kmeanspp: cand/pots must be [K,8], winner/index [K]");
  TORCH_CHECK(0 <= t0 && t0 <= t1 && t1 <= k,
              "seed_kmeanspp: rounds must satisfy 0 <= t0 <= t1 <= K");
  auto st = stream();
  const dim3 grid((uint32_t)nblk), one(1), nt(kNT);
  const int x_vec = reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0;
  if (t0 == 0 && t0 < t1 && (stages & kSeedSample))
    hipLaunchKernelGGL(gmm::seed_weight_partials_kernel, grid, nt, 0, st, sp,
                       s_part.data_ptr<double>(), n);
  for (int64_t t = t0; t < t1; ++t) {
    const int nlt = t == 0 ? 1 : nl;
    int64_t* cand_t = cand.data_ptr<int64_t>() + t * gmm::SEED_LMAX;
    if (stages & kSeedSample)
      hipLaunchKernelGGL(gmm::seed_sample_kernel, one, nt, 0, st, sp,
                         m.data_ptr<float>(), sm_part.data_ptr<double>(),
                         s_part.data_ptr<double>(),
                         u.data_ptr<double>() + t * gmm::SEED_LMAX, nlt,
                         (int)(t == 0), cand_t, nblk, n);
    if (stages & kSeedEvaluate)
      hipLaunchKernelGGL(gmm::seed_evaluate_kernel, grid, nt, 0, st,
                         x.data_ptr<float>(), sp, m.data_ptr<float>(), cand_t,
                         nlt, (int)(t == 0), scratch.data_ptr<float>(),
                         pot_part.data_ptr<double>(), x_vec, d, n);
    if (stages & kSeedChoose)
      hipLaunchKernelGGL(gmm::seed_choose_kernel, one, nt, 0, st,
                         pot_part.data_ptr<double>(), cand_t, nlt,
                         winner.data_ptr<int>() + t,
                         index.data_ptr<int64_t>() + t,
                         pots.data_ptr<double>() + t * gmm::SEED_LMAX, nblk);
    if (stages & kSeedCommit)
      hipLaunchKernelGGL(gmm::seed_commit_kernel, grid, nt, 0, st,
                         scratch.data_ptr<float>(),
                         winner.data_ptr<int>() + t, nlt, sp,
                         m.data_ptr<float>(), sm_part.data_ptr<double>(), n);
  }
  HIP_CHECK(hipGetLastError());
}

void estep_logw_big(torch::Tensor z, torch::Tensor mfac, torch::Tensor add,
                    torch::Tensor logw) {
  TORCH_CHECK(z.is_cuda() && z.is_contiguous() &&
                  z.scalar_type() == torch::kBFloat16,
              "z must be contiguous bf16 [D,N]");
  TORCH_CHECK(mfac.is_contiguous() && mfac.scalar_type() == torch::kBFloat16);
  check_f32(add, "add");
  check_f32(logw, "logw");
  const int d = (int)z.size(0);
  const int64_t n = z.size(1);
  const int k = (int)add.size(0);
  TORCH_CHECK(d >= 1 && d <= 142, "estep_logw_big supports D <= 143");
  TORCH_CHECK(logw.size(0) == k && logw.size(1) == n, "logw shape");
  const int kct = gmm::mfac_kct(d);
  const int rows = gmm::mfac_rows(d);
  const int rt_n = rows / 32;
  const int arow = kct * 16 + 8;
  // 256-event tiles where the LDS fits (gfx950: 160 KB/workgroup max),
  // else 128 (only D > 128, rows = 160, needs the smaller tile)
  const size_t lds256 = (size_t)(2 * rows + 256) * arow * 2 +
                        (size_t)rt_n * 256 * 4;
  const size_t lds128 = (size_t)(2 * rows + 128) * arow * 2 +
                        (size_t)rt_n * 128 * 4;
  const int be = lds256 <= 160 * 1024 ? 256 : 128;
  const size_t lds = be == 256 ? lds256 : lds128;
  const int64_t tiles = (n + be - 1) / be;
  // enough blocks to fill the chip; each block amortizes one staged
  // factor table over tiles/nchunk z tiles
  // 1024/K (4 chunk-streams at K=256): same-box A/B 3x alternating
  // showed 7.39 vs 7.26 it/s (+1.8%) over 2048/K on config 4 — fewer,
  // longer chunk walks keep same-XCD blocks closer to L2 lockstep
  int nchunk =
      (int)std::min<int64_t>(tiles, std::max<int64_t>(1, 1024 / k));
  if (const char* e = std::getenv("GMM_BIG2_NCHUNK"))
    nchunk = (int)std::min<int64_t>(tiles, std::max(1, atoi(e)));
  dim3 grid((uint32_t)nchunk, k);
  // block size matched to the (row-tile x event-tile) task count so no
  // waves idle at small rt_n
  const uint32_t nthreads = std::min<uint32_t>(
      1024, std::max<uint32_t>(256, rt_n * (be / 32) * 64));
  auto s = stream();
#define LAUNCH_ELB(KCT, BE)                                                 \
  do {                                                                      \
    if (lds > 64 * 1024) {                                                  \
      HIP_CHECK(hipFuncSetAttribute(                                        \
          reinterpret_cast<const void*>(                                    \
              &gmm::estep_logw_big2_kernel<KCT, BE>),                       \
          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));           \
    }                                                                       \
    hipLaunchKernelGGL((gmm::estep_logw_big2_kernel<KCT, BE>), grid,        \
                       dim3(nthreads), lds, s,                              \
                       reinterpret_cast<const __hip_bfloat16*>(             \
                           z.data_ptr()),                                   \
                       reinterpret_cast<const __hip_bfloat16*>(             \
                           mfac.data_ptr()),                                \
                       add.data_ptr<float>(), logw.data_ptr<float>(), d, k, \
                       n, nchunk);                                          \
  } while (0)
  if (kct == 2) LAUNCH_ELB(2, 256);
  else if (kct == 3) LAUNCH_ELB(3, 256);
  else if (kct == 5) LAUNCH_ELB(5, 256);
  else if (be == 256) LAUNCH_ELB(9, 256);
  else LAUNCH_ELB(9, 128);
#undef LAUNCH_ELB
  HIP_CHECK(hipGetLastError());
}

void estep_logw_big_f32(torch::Tensor z, torch::Tensor mfac32,
                        torch::Tensor add, torch::Tensor logw) {
  check_f32(z, "z");
  check_f32(mfac32, "mfac32");
  check_f32(add, "add");
  check_f32(logw, "logw");
  const int d = (int)z.size(0);
  const int64_t n = z.size(1);
  const int k = (int)add.size(0);
  TORCH_CHECK(d >= 1 && d <= 142, "estep_logw_big_f32 supports D <= 143");
  TORCH_CHECK(logw.size(0) == k && logw.size(1) == n, "logw shape");
  const int kct = gmm::mfac_kct(d);
  const int rows = gmm::mfac_rows(d);
  TORCH_CHECK(mfac32.numel() >= (int64_t)k * rows * kct * 16,
              "mfac32 too small for big-D layout");
  const size_t lds = sizeof(float) * (size_t)128 * (kct * 16 + 4);
  dim3 grid((uint32_t)((n + 127) / 128), (k + 3) / 4);
  auto s = stream();
#define LAUNCH_ELBF(KCT)                                                    \
  do {                                                                      \
    if (lds > 64 * 1024) {                                                  \
      HIP_CHECK(hipFuncSetAttribute(                                        \
          reinterpret_cast<const void*>(                                    \
              &gmm::estep_logw_big_f32_kernel<KCT>),                        \
          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));           \
    }                                                                       \
    hipLaunchKernelGGL((gmm::estep_logw_big_f32_kernel<KCT>), grid,         \
                       dim3(kNT), lds, s, z.data_ptr<float>(),              \
                       mfac32.data_ptr<float>(), add.data_ptr<float>(),     \
                       logw.data_ptr<float>(), d, k, n);                    \
  } while (0)
  if (kct == 2) LAUNCH_ELBF(2);
  else if (kct == 3) LAUNCH_ELBF(3);
  else if (kct == 5) LAUNCH_ELBF(5);
  else LAUNCH_ELBF(9);
#undef LAUNCH_ELBF
  HIP_CHECK(hipGetLastError());
}

void mstep_moments_big(torch::Tensor x, torch::Tensor w,
                       torch::Tensor lse, torch::Tensor partials) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() &&
                  x.scalar_type() == torch::kFloat32,
              "x must be contiguous fp32");
  check_f32(w, "w");
  check_f32(partials, "partials");
  const int d = (int)x.size(0);
  const int64_t n = x.size(1);
  const int k = (int)w.size(0);
  const int nchunk = (int)partials.size(0);
  const int dp = d + 1;
  TORCH_CHECK(d > 31 && d <= 159, "mstep_moments_big is the D > 31 path");
  TORCH_CHECK(partials.size(1) == k &&
                  partials.size(2) == dp * (dp + 1) / 2,
              "partials must be [nchunk, K, Dp*(Dp+1)/2]");
  const int rows = ((dp + 31) / 32) * 32;
  // double-buffered: 2 x (zhi+zlo planes + w tiles)
  const size_t lds =
      2 * ((size_t)2 * rows * (64 + 8) * 2 + 2 * 64 * 4);
  if (lds > 64 * 1024) {
    HIP_CHECK(hipFuncSetAttribute(
        reinterpret_cast<const void*>(&gmm::mstep_moments_big_kernel),
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  dim3 grid((k + 1) / 2, nchunk);
  hipLaunchKernelGGL(gmm::mstep_moments_big_kernel, grid, dim3(1024), lds,
                     stream(), x.data_ptr<float>(), w.data_ptr<float>(),
                     lse_ptr(lse, n), partials.data_ptr<float>(), d, k, n,
                     nchunk);
  HIP_CHECK(hipGetLastError());
}

void mfma_probe32(torch::Tensor a, torch::Tensor b, torch::Tensor c) {
  TORCH_CHECK(a.scalar_type() == torch::kBFloat16 && a.numel() == 32 * 16);
  TORCH_CHECK(b.scalar_type() == torch::kBFloat16 && b.numel() == 16 * 32);
  check_f32(c, "c");
  hipLaunchKernelGGL(gmm::mfma_probe32_kernel, dim3(1), dim3(64), 0, stream(),
                     reinterpret_cast<const __hip_bfloat16*>(a.data_ptr()),
                     reinterpret_cast<const __hip_bfloat16*>(b.data_ptr()),
                     c.data_ptr<float>());
  HIP_CHECK(hipGetLastError());
}

void reduce_chunks(torch::Tensor partials, torch::Tensor out) {
  check_f32(partials, "partials");
  check_f32(out, "out");
  const int c = (int)partials.size(0);
  const int64_t m = partials.numel() / c;
  TORCH_CHECK(out.numel() == m, "out shape");
  // a column per thread, one wave per block: ~20k columns at the flagship
  // shape make 325 blocks over the 256 CUs (82 four-wave blocks left two
  // thirds of them idle in a kernel that lives on loads in flight)
  constexpr int kRcNT = 64;
  const int grid = (int)std::min<int64_t>((m + kRcNT - 1) / kRcNT, 8192);
  hipLaunchKernelGGL(gmm::reduce_chunks_kernel, dim3(grid), dim3(kRcNT), 0,
                     stream(), partials.data_ptr<float>(),
                     out.data_ptr<float>(), c, m);
  HIP_CHECK(hipGetLastError());
}

void reduce_scalar(torch::Tensor in, torch::Tensor out) {
  check_f32(in, "in");
  check_f32(out, "out");
  TORCH_CHECK(out.numel() >= 1);
  hipLaunchKernelGGL(gmm::reduce_scalar_kernel, dim3(1), dim3(kNT), 0,
                     stream(), in.data_ptr<float>(), out.data_ptr<float>(),
                     in.numel());
  HIP_CHECK(hipGetLastError());
}

void mstep_finalize(torch::Tensor packed, torch::Tensor avgvar,
                    int64_t world, torch::Tensor n_out, torch::Tensor means,
                    torch::Tensor r_out, torch::Tensor pi, bool diag_only) {
  check_f32(packed, "packed");
  check_f32(avgvar, "avgvar");
  check_f32(n_out, "n_out");
  check_f32(means, "means");
  check_f32(r_out, "r_out");
  check_f32(pi, "pi");
  const int k = (int)means.size(0);
  const int d = (int)means.size(1);
  TORCH_CHECK(packed.size(0) == k &&
                  packed.size(1) == (d + 1) * (d + 2) / 2,
              "packed shape mismatch");
  hipLaunchKernelGGL(gmm::mstep_finalize_kernel, dim3(k), dim3(kNT),
                     sizeof(float) * d, stream(), packed.data_ptr<float>(),
                     avgvar.data_ptr<float>(), (int)world,
                     n_out.data_ptr<float>(), means.data_ptr<float>(),
                     r_out.data_ptr<float>(), pi.data_ptr<float>(), d, k,
                     diag_only ? 1 : 0);
  HIP_CHECK(hipGetLastError());
}

void mstep_finalize_emit(torch::Tensor packed, torch::Tensor avgvar,
                         int64_t world, torch::Tensor n_out,
                         torch::Tensor means, torch::Tensor r_out,
                         torch::Tensor pi, torch::Tensor constant,
                         torch::Tensor add, torch::Tensor mfac,
                         torch::Tensor mfac32) {
  check_f32(packed, "packed");
  check_f32(avgvar, "avgvar");
  check_f32(n_out, "n_out");
  check_f32(means, "means");
  check_f32(r_out, "r_out");
  check_f32(pi, "pi");
  check_f32(constant, "constant");
  check_f32(add, "add");
  const int k = (int)means.size(0);
  const int d = (int)means.size(1);
  TORCH_CHECK(packed.size(0) == k &&
                  packed.size(1) == (d + 1) * (d + 2) / 2,
              "packed shape mismatch");
  TORCH_CHECK(mfac.numel() > 0 && mfac.scalar_type() == torch::kBFloat16 &&
              mfac.is_contiguous());
  __hip_bfloat16* mp =
      reinterpret_cast<__hip_bfloat16*>(mfac.data_ptr());
  float* mp32 = nullptr;
  if (mfac32.numel() > 0) {
    check_f32(mfac32, "mfac32");
    mp32 = mfac32.data_ptr<float>();
  }
  check_factor_out(mfac, mfac32, d);
  const size_t lds = sizeof(float) * (2 * (size_t)d * (d | 1) + d);
  if (lds > 64 * 1024) {
    HIP_CHECK(hipFuncSetAttribute(
        reinterpret_cast<const void*>(&gmm::mstep_finalize_emit_kernel),
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  hipLaunchKernelGGL(gmm::mstep_finalize_emit_kernel, dim3(k), dim3(kNT),
                     lds, stream(), packed.data_ptr<float>(),
                     avgvar.data_ptr<float>(), (int)world,
                     n_out.data_ptr<float>(), means.data_ptr<float>(),
                     r_out.data_ptr<float>(), pi.data_ptr<float>(),
                     constant.data_ptr<float>(), add.data_ptr<float>(), mp,
                     mp32, d, k);
  HIP_CHECK(hipGetLastError());
}

void emit_factors(torch::Tensor r, torch::Tensor means,
                  torch::Tensor mfac, torch::Tensor mfac32,
                  torch::Tensor pi, torch::Tensor constant,
                  torch::Tensor add) {
  check_f32(r, "r");
  check_f32(means, "means");
  const int k = (int)r.size(0);
  const int d = (int)r.size(1);
  __hip_bfloat16* mp = nullptr;
  float* mp32 = nullptr;
  if (mfac.numel() > 0) {
    TORCH_CHECK(mfac.scalar_type() == torch::kBFloat16 && mfac.is_contiguous());
    mp = reinterpret_cast<__hip_bfloat16*>(mfac.data_ptr());
  }
  if (mfac32.numel() > 0) {
    check_f32(mfac32, "mfac32");
    mp32 = mfac32.data_ptr<float>();
  }
  check_factor_out(mfac, mfac32, d);
  const size_t lds = sizeof(float) * (2 * (size_t)d * (d | 1) + d);
  if (lds > 64 * 1024) {
    HIP_CHECK(hipFuncSetAttribute(
        reinterpret_cast<const void*>(&gmm::emit_mfac_from_r_kernel),
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  const float* pip = pi.numel() > 0 ? pi.data_ptr<float>() : nullptr;
  float* cst = constant.numel() > 0 ? constant.data_ptr<float>() : nullptr;
  float* addp = add.numel() > 0 ? add.data_ptr<float>() : nullptr;
  TORCH_CHECK(addp == nullptr || pip != nullptr, "add output requires pi");
  hipLaunchKernelGGL(gmm::emit_mfac_from_r_kernel, dim3(k), dim3(kNT),
                     lds, stream(), r.data_ptr<float>(),
                     means.data_ptr<float>(), mp, mp32, d, pip, cst, addp);
  HIP_CHECK(hipGetLastError());
}

void mfma_probe(torch::Tensor a, torch::Tensor b, torch::Tensor c) {
  TORCH_CHECK(a.scalar_type() == torch::kBFloat16 && a.numel() == 16 * 32);
  TORCH_CHECK(b.scalar_type() == torch::kBFloat16 && b.numel() == 32 * 16);
  check_f32(c, "c");
  hipLaunchKernelGGL(gmm::mfma_probe_kernel, dim3(1), dim3(64), 0, stream(),
                     reinterpret_cast<const __hip_bfloat16*>(a.data_ptr()),
                     reinterpret_cast<const __hip_bfloat16*>(b.data_ptr()),
                     c.data_ptr<float>());
  HIP_CHECK(hipGetLastError());
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("estep_logw", &estep_logw,
        "log weighted likelihoods [K,N] (gfx950 kernel)");
  m.def("estep_posteriors", &estep_posteriors,
        "in-place posteriors + per-block likelihood partials");
  m.def("estep_lse", &estep_lse,
        "per-event log-sum-exp + likelihood partials (no posterior "
        "write-back; pairs with the lse-aware M-step)");
  m.def("event_weight_lse", &event_weight_lse,
        "lse_w = lse - ln s (+inf at s == 0) + weighted likelihood partials");
  m.def("event_weight_lse_blocks", &event_weight_lse_blocks,
        "block (= likelihood partial) count of event_weight_lse for N events");
  m.def("background_lse", &background_lse,
        "uniform background: lse_b = logaddexp(lse, b), the moments' lse_m, "
        "block partials of n0 and (optionally) the likelihood");
  m.def("background_update", &background_update,
        "background state (pi0, b, lik_add, n0) from the n0 partials");
  m.def("student_t_lse", &student_t_lse,
        "Student-t components on the lse contract: logw [K, N] in place, "
        "lse_t, and in train mode lse_m plus block partials of N_c and the "
        "likelihood");
  m.def("student_t_lse_blocks", &student_t_lse_blocks,
        "block (= partial row) count of student_t_lse for N events");
  m.def("student_t_pi", &student_t_pi,
        "N, pi (and add) of a t fit from the reduced responsibilities");
  m.def("mstep_covariance_partials", &mstep_covariance_partials,
        "packed weighted second-moment partials [nchunk,K,P]");
  m.def("constants", &constants,
        "batched no-pivot LU inverse + ln|det| + bf16 Cholesky factors");
  m.def("estep_logw_big", &estep_logw_big,
        "big-D MFMA log-weights (31 < D <= 142)");
  m.def("estep_logw_big_f32", &estep_logw_big_f32,
        "exact-f32 big-D MFMA log-weights (31 < D <= 142)");
  m.def("mstep_moments_big", &mstep_moments_big,
        "big-D split-precision moments");
  m.def("mstep_moments_b16", &mstep_moments_b16,
        "split-precision bf16x3 augmented moments");
  m.def("mstep_moments", &mstep_moments,
        "fused augmented moments [S|mean_num|N] via f32 MFMA");
  m.def("mstep_moments_pair_b16", &mstep_moments_pair_b16,
        "split-precision bf16x3 moments as one W.P GEMM over pair columns");
  m.def("exp_sub_lse", &exp_sub_lse,
        "out[c, e] = __expf(logw[c, e] - lse[e]) (moments staging twin)");
  m.def("reduce_chunks", &reduce_chunks,
        "deterministic chunk-partials reduction out[j] = sum_i in[i][j]");
  m.def("reduce_scalar", &reduce_scalar,
        "deterministic scalar sum out[0] = sum(in)");
  m.def("mstep_finalize_emit", &mstep_finalize_emit,
        "fused M-step finalize + factor/constants emission (fast path)");
  m.def("mstep_finalize", &mstep_finalize,
        "finalize N/means/R/pi from all-reduced packed moments");
  m.def("emit_factors", &emit_factors,
        "re-emit E-step factors from the covariance R (post-merge/resume)");
  m.def("estep_fused_f32", &estep_fused_f32,
        "exact-f32 MFMA fused E-step (D <= 31)");
  m.def("estep_fused_lds", &estep_fused_lds,
        "small-K fused E-step (v1, lw in LDS, posteriors written)");
  m.def("estep_fused_lds2", &estep_fused_lds2,
        "small-K fused E-step (register B tiles, float4 pass 2; default)");
  m.def("estep_fused_f32_lds", &estep_fused_f32_lds,
        "small-K exact-f32 fused E-step (v1)");
  m.def("estep_fused", &estep_fused,
        "fused bf16-MFMA E-step: posteriors + likelihood partials");
  m.def("estep_classify", &estep_classify,
        "bf16-MFMA classify (D <= 31): label / lse / pmax per event");
  m.def("estep_classify_f32", &estep_classify_f32,
        "exact-f32 MFMA classify (D <= 31): label / lse / pmax per event");
  m.def("seed_kmeanspp_rounds", &seed_kmeanspp_rounds,
        "greedy k-means++ seeding: enqueue stages (1 sample | 2 evaluate | "
        "4 choose | 8 commit) of rounds [t0, t1)");
  m.def("seed_kmeanspp_blocks", &seed_kmeanspp_blocks,
        "block (= partial row) count of the seeding kernels for N events");
  m.def("mfma_probe", &mfma_probe, "bf16 MFMA fragment-layout probe");
  m.def("mfma_probe32", &mfma_probe32, "32x32x16 bf16 layout probe");
}
