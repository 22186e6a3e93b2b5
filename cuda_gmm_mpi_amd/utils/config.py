"""Runtime configuration for the MI355X-native GMM EM engine.

Every compile-time ``#define`` of the reference (``gaussian.h:10-42``) becomes a
runtime field here, with defaults equal to the reference values so that a
default run reproduces the reference behavior (including its quirks — see
``bug_compat``).
"""
from __future__ import annotations

import dataclasses
import math

# Reference: gaussian.h:10-16
MAX_CLUSTERS = 512
PI = 3.1415926535897931
COVARIANCE_DYNAMIC_RANGE = 1e3


@dataclasses.dataclass
class GmmConfig:
    """All knobs of the EM / MDL engine.

    Defaults reproduce the reference (`gaussian.h`) exactly:
    - ``min_iters == max_iters == 100`` makes the convergence epsilon dead
      (gaussian.cu:532 with gaussian.h:26-27) — every K runs 100 iterations.
    - ``bug_compat=True`` keeps the reference's log10/ln determinant mismatch
      in the merge path (invert_matrix.cpp:61 consumed as ln at
      gaussian.cu:1249) so MDL merge decisions match the reference bit-wise
      in spirit.
    """

    # Model-order loop (CLI positional args, gaussian.cu:1111-1166)
    num_clusters: int = 1
    target_num_clusters: int = 0  # 0 => sweep down to 1, keep best MDL score

    # EM loop (gaussian.h:26-27)
    min_iters: int = 100
    max_iters: int = 100

    # Numerics (gaussian.h:12, 23)
    covariance_dynamic_range: float = COVARIANCE_DYNAMIC_RANGE
    diag_only: bool = False

    # Faithful reproduction of reference quirks:
    #  - merge-path determinant accumulated in log10 but consumed as ln
    bug_compat: bool = True

    # Output toggles (gaussian.h:35-38). The reference defaults both to 0;
    # we default output ON because that is what end users need. The summary
    # file is always created (empty when output disabled), matching
    # gaussian.cu:1015-1040.
    enable_print: bool = False
    enable_output: bool = True

    # Compute dtype of the E-step data reads ("fp32" | "bf16"); accumulation
    # is always fp32. BASELINE.json config 2 names a bf16 E-step.
    estep_dtype: str = "fp32"

    # M-step sufficient-statistics precision: "fp32" = exact fp32 fmaf
    # chain (f32 MFMA, bitwise a VALU loop); "bf16x3" = split-precision
    # bf16 MFMA (~1e-5 relative on S, ~15x the instruction rate).
    mstep_precision: str = "fp32"

    # Internally center data by the global per-dimension mean before EM.
    # Translation-invariant math (covariance, quadratic forms) is unchanged;
    # output means get the center added back. This removes the catastrophic
    # cancellation in S - N*mu*mu^T and in the reference's own
    # E[x^2]-mean^2 variance (gaussian_kernel.cu:84-87).
    center_data: bool = True

    # Per-iteration likelihood logging on rank 0 (runtime replacement for
    # the reference's compile-time DEBUG printf macros, gaussian.h:44-54).
    verbose: bool = False

    # When the empty-cluster elimination jumps past target_num_clusters,
    # the reference keeps the FIRST saved model (K0). With this flag the
    # sweep instead saves the last completed K nearest the target.
    nearest_target: bool = False

    # Directory for MDL-sweep checkpoints (.npz per completed K); None
    # disables. Resume happens automatically when a checkpoint exists.
    checkpoint_dir: str | None = None

    # Where the K0 starting means come from: "strided" = the reference's
    # evenly-strided rows (gaussian.cu:108-123), which depend on the row
    # order of the file; "kmeans++" = a greedy k-means++ draw over the full
    # dataset (models.seed.seed_means_kmeanspp), reproducible from seed_rng.
    # A checkpoint resume ignores both.
    seed_method: str = "strided"
    seed_rng: int = 0

    # Uniform background component for outliers: the mixture becomes
    # (1 - pi0) * sum_c pi_c N_c(x) + pi0 / V with V the volume of the
    # data's bounding box (background_log_volume = ln V; None: computed from
    # the full data). It is switched on at pi0 = background_init after
    # background_warmup plain EM iterations at the starting K: from the
    # reference's R = I seeds the first quadratic forms are huge and a
    # background present from the first E-step takes every event for good.
    background: bool = False
    background_init: float = 0.01
    background_warmup: int = 5
    background_log_volume: float | None = None

    # Student-t mixture components with this many degrees of freedom (fixed,
    # not estimated); 0 = Gaussian components. Events in a population's tail
    # are down-weighted by u = (nu + D) / (nu + q) instead of inflating its
    # covariance. R is then the t scale matrix: the covariance is
    # nu / (nu - 2) * R for nu > 2.
    student_t_nu: float = 0.0

    def validate(self) -> None:
        if not (1 <= self.num_clusters <= MAX_CLUSTERS):
            raise ValueError(
                f"Invalid number of starting clusters (1..{MAX_CLUSTERS}): "
                f"{self.num_clusters}"
            )
        if self.target_num_clusters < 0:
            raise ValueError("target_num_clusters must be >= 0")
        if self.target_num_clusters > self.num_clusters:
            raise ValueError(
                "target_num_clusters must be less than equal to num_clusters"
            )
        if self.min_iters < 0 or self.max_iters < self.min_iters:
            raise ValueError(
                "need 0 <= min_iters <= max_iters: "
                f"{self.min_iters}..{self.max_iters}")
        if self.estep_dtype not in ("fp32", "bf16"):
            raise ValueError(f"estep_dtype must be fp32|bf16: {self.estep_dtype}")
        if self.mstep_precision not in ("fp32", "bf16x3"):
            raise ValueError(
                f"mstep_precision must be fp32|bf16x3: {self.mstep_precision}")
        if self.seed_method not in ("strided", "kmeans++"):
            raise ValueError(
                f"seed_method must be strided|kmeans++: {self.seed_method}")
        if (isinstance(self.seed_rng, bool)
                or not isinstance(self.seed_rng, int) or self.seed_rng < 0):
            raise ValueError(
                f"seed_rng must be an integer >= 0: {self.seed_rng!r}")
        if not (0.0 < float(self.background_init) < 1.0):
            raise ValueError(
                f"background_init must be in (0, 1): {self.background_init}")
        if (isinstance(self.background_warmup, bool)
                or not isinstance(self.background_warmup, int)
                or self.background_warmup < 0):
            raise ValueError("background_warmup must be an integer >= 0: "
                             f"{self.background_warmup!r}")
        if (self.background_log_volume is not None
                and not math.isfinite(float(self.background_log_volume))):
            raise ValueError("background_log_volume must be finite: "
                             f"{self.background_log_volume}")
        if self.background and self.checkpoint_dir:
            raise ValueError(
                "background cannot be combined with checkpoint_dir (the "
                "checkpoint does not hold the background's state)")

        if (isinstance(self.student_t_nu, bool)
                or not isinstance(self.student_t_nu, (int, float))
                or not math.isfinite(float(self.student_t_nu))
                or float(self.student_t_nu) < 0.0):
            raise ValueError("student_t_nu must be finite and >= 0 "
                             f"(0 = Gaussian components): "
                             f"{self.student_t_nu!r}")
        if self.student_t_nu > 0 and self.background:
            raise ValueError(
                "student_t_nu cannot be combined with background (the "
                "background pass and the t pass both rewrite the lse the "
                "M-step reads; combining them is not implemented)")
        if self.student_t_nu > 0 and self.checkpoint_dir:
            raise ValueError(
                "student_t_nu cannot be combined with checkpoint_dir (a "
                "checkpoint does not record the degrees of freedom)")

    @property
    def stop_number(self) -> int:
        """K at which the sweep stops (gaussian.cu:177-181)."""
        return 1 if self.target_num_clusters == 0 else self.target_num_clusters


def em_epsilon(num_dimensions: int, num_events: int) -> float:
    """Convergence epsilon (gaussian.cu:458).

    eps = (1 + D + 0.5*(D+1)*D) * ln(N*D) * 0.01
    Dead at reference defaults (min_iters == max_iters) but kept for
    configurable iteration counts.
    """
    d = num_dimensions
    return (1 + d + 0.5 * (d + 1) * d) * math.log(float(num_events) * d) * 0.01


def rissanen_score(likelihood: float, num_clusters: int, num_dimensions: int,
                   num_events: int, extra_params: int = 0) -> float:
    """Rissanen / MDL score (gaussian.cu:826).

    rissanen = -L + 0.5*(K*(1 + D + 0.5*(D+1)*D) - 1 + extra)*ln(N*D)

    ``extra_params`` counts free parameters beyond the Gaussians' (a
    background component adds one, its weight).
    """
    d = num_dimensions
    params_per_cluster = 1 + d + 0.5 * (d + 1) * d
    return float(
        -likelihood
        + 0.5 * (num_clusters * params_per_cluster - 1 + extra_params)
        * math.log(float(num_events) * d)
    )
