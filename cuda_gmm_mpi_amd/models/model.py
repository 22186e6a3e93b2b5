"""A fitted mixture as an object of its own: save it, load it, score new
data with it ("fit on one sample, gate the next twenty").

The means are stored in the engine's internal frame (`means_centered`,
relative to `center`): adding and then subtracting the centre is not exact
in fp32, and keeping the internal-frame values is what lets scoring the
training data reproduce the training run's memberships exactly. `constant`
is stored and used verbatim: after a merge under bug_compat it carries the
reference's log10 quirk, and the run's own .results is computed with it.

Scoring is single-process.
"""
from __future__ import annotations

import dataclasses
import os

import numpy as np
import torch

from ..ops import cpu_reference as cpu
from ..ops import functional as F
from .state import GmmState

FORMAT_VERSION = 1
# a model with a uniform background component: version 1 plus two scalars
FORMAT_VERSION_BACKGROUND = 2

_ARRAYS = ("center", "means_centered", "pi", "N", "constant", "avgvar",
           "R", "Rinv")
_FLAGS = ("diag_only", "bug_compat")
_KEYS = ("format_version",) + _ARRAYS + _FLAGS
_BACKGROUND = ("background_pi", "background_log_volume")
# a model with Student-t components: version 1 plus the degrees of freedom
FORMAT_VERSION_STUDENT_T = 3
_STUDENT_T = ("student_t_nu",)
_KEYS_BY_VERSION = {FORMAT_VERSION: _KEYS,
                    FORMAT_VERSION_BACKGROUND: _KEYS + _BACKGROUND,
                    FORMAT_VERSION_STUDENT_T: _KEYS + _STUDENT_T}


@dataclasses.dataclass
class Prediction:
    labels: np.ndarray         # int32 [N], first argmax of the posteriors;
    #                            -1 = the background (models that have one)
    log_prob: np.ndarray       # fp32 [N], ln p(x_e)
    max_posterior: np.ndarray  # fp32 [N], posterior of the assigned component
    log_likelihood: float      # float64 sum of log_prob
    counts: np.ndarray         # int64 [K], events per cluster label
    background_count: int = 0  # events labelled -1


def _as_events(data) -> torch.Tensor:
    """[N, D] fp32 contiguous CPU tensor from a numpy array or CPU tensor."""
    if isinstance(data, torch.Tensor):
        t = data.detach().to("cpu", torch.float32).contiguous()
    else:
        t = torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32))
    if t.dim() != 2:
        raise ValueError(f"data must be [N, D], got shape {tuple(t.shape)}")
    return t


@dataclasses.dataclass
class GmmModel:
    """Parameters of a fitted K-cluster, D-dimensional mixture (fp32 CPU
    tensors)."""
    center: torch.Tensor          # [D]
    means_centered: torch.Tensor  # [K, D], relative to center
    pi: torch.Tensor              # [K]
    N: torch.Tensor               # [K]
    constant: torch.Tensor        # [K], verbatim from the run
    avgvar: torch.Tensor          # [K]
    R: torch.Tensor               # [K, D, D]
    Rinv: torch.Tensor            # [K, D, D]
    diag_only: bool = False
    bug_compat: bool = True
    # uniform background: the mixture is (1 - background_pi) * sum_c pi_c
    # N_c + background_pi / V, ln V = background_log_volume; pi stays
    # normalised among the clusters. background_pi == 0: no background.
    background_pi: float = 0.0
    background_log_volume: float = 0.0
    # Student-t components with this many degrees of freedom (0: Gaussian).
    # R is then the scale matrix and `constant` stays the Gaussian one: the
    # t normaliser adds the same delta(nu, D) to every cluster.
    student_t_nu: float = 0.0

    def __post_init__(self):
        for name in _ARRAYS:
            setattr(self, name, torch.as_tensor(getattr(self, name))
                    .detach().to("cpu", torch.float32).contiguous())
        self.diag_only = bool(self.diag_only)
        self.bug_compat = bool(self.bug_compat)
        self.background_pi = float(self.background_pi)
        self.background_log_volume = float(self.background_log_volume)
        self.student_t_nu = float(self.student_t_nu)
        self._validate()

    def _validate(self) -> None:
        if self.means_centered.dim() != 2:
            raise ValueError("means_centered must be [K, D]")
        k, d = self.means_centered.shape
        want = {"center": (d,), "pi": (k,), "N": (k,), "constant": (k,),
                "avgvar": (k,), "R": (k, d, d), "Rinv": (k, d, d)}
        if k < 1 or d < 1:
            raise ValueError(f"model needs K >= 1 and D >= 1, got {k}x{d}")
        if not (0.0 <= self.background_pi < 1.0
                and np.isfinite(self.background_log_volume)):
            raise ValueError(
                f"inconsistent model: background_pi {self.background_pi} "
                f"must be in [0, 1) and background_log_volume "
                f"{self.background_log_volume} finite")
        if not (np.isfinite(self.student_t_nu) and self.student_t_nu >= 0.0):
            raise ValueError(
                f"inconsistent model: student_t_nu {self.student_t_nu} must "
                f"be finite and >= 0")
        if self.student_t_nu > 0.0 and self.background_pi > 0.0:
            raise ValueError(
                "inconsistent model: Student-t components cannot be combined "
                "with a background")
        for name, shape in want.items():
            got = tuple(getattr(self, name).shape)
            if got != shape:
                raise ValueError(
                    f"inconsistent model: {name} has shape {got}, expected "
                    f"{shape} for K={k}, D={d}")

    @property
    def num_clusters(self) -> int:
        return int(self.means_centered.shape[0])

    @property
    def num_dimensions(self) -> int:
        return int(self.means_centered.shape[1])

    @property
    def has_background(self) -> bool:
        return self.background_pi > 0.0

    @property
    def is_student_t(self) -> bool:
        return self.student_t_nu > 0.0

    @property
    def means(self) -> torch.Tensor:
        """Cluster means in the data's own frame."""
        return self.means_centered + self.center.unsqueeze(0)

    # ---------------------------------------------------------- construction

    @classmethod
    def from_state(cls, state: GmmState, center: torch.Tensor,
                   diag_only: bool = False,
                   bug_compat: bool = True, background_pi: float = 0.0,
                   background_log_volume: float = 0.0,
                   student_t_nu: float = 0.0) -> "GmmModel":
        """From an engine state whose means are in the centred frame."""
        return cls(center=center.clone(), means_centered=state.means.clone(),
                   pi=state.pi.clone(), N=state.N.clone(),
                   constant=state.constant.clone(),
                   avgvar=state.avgvar.clone(), R=state.R.clone(),
                   Rinv=state.Rinv.clone(), diag_only=diag_only,
                   bug_compat=bug_compat, background_pi=background_pi,
                   background_log_volume=(background_log_volume
                                          if background_pi > 0.0 else 0.0),
                   student_t_nu=student_t_nu)

    @classmethod
    def from_params(cls, means, R, pi, N=None, center=None,
                    diag_only: bool = False, background_pi: float = 0.0,
                    background_log_volume: float = 0.0,
                    student_t_nu: float = 0.0) -> "GmmModel":
        """From means [K, D] (data frame), covariances (scale matrices for a
        t model, ``student_t_nu`` > 0) and weights; Rinv and
        constant come from cpu_reference.compute_constants (natural log).
        The default centre is the pi-weighted mean of the means."""
        means = torch.as_tensor(means, dtype=torch.float32)
        r = torch.as_tensor(R, dtype=torch.float32)
        pi = torch.as_tensor(pi, dtype=torch.float32)
        k = means.shape[0]
        if center is None:
            center = ((pi.double().unsqueeze(1) * means.double()).sum(dim=0)
                      / pi.double().sum()).float()
        center = torch.as_tensor(center, dtype=torch.float32)
        rinv, constant = cpu.compute_constants(r.contiguous(), diag_only)
        return cls(center=center, means_centered=means - center.unsqueeze(0),
                   pi=pi, N=(torch.as_tensor(N, dtype=torch.float32)
                             if N is not None else torch.zeros(k)),
                   constant=constant, avgvar=torch.zeros(k), R=r, Rinv=rinv,
                   diag_only=diag_only, bug_compat=False,
                   background_pi=background_pi,
                   background_log_volume=background_log_volume,
                   student_t_nu=student_t_nu)

    @classmethod
    def from_summary(cls, path: str) -> "GmmModel":
        """From a .summary file (this project's or the reference's).

        LOSSY: .summary holds %.3f means and covariances and %f weights, so
        the model is the fitted one rounded to that; Rinv and constant are
        recomputed from the rounded R. Use save()/load() to keep a model
        exactly."""
        from ..utils.io import read_summary
        s = read_summary(path)
        pi0 = float(s.get("background_pi", 0.0))
        if pi0 <= 0.0:
            return cls.from_params(
                s["means"], s["R"], s["pi"], N=s["N"],
                student_t_nu=float(s.get("student_t_nu", 0.0)))
        # the cluster lines hold (1 - pi0) * pi_c: back to pi_c, normalised
        # among the clusters
        pi = s["pi"].astype(np.float64) / (1.0 - pi0)
        return cls.from_params(
            s["means"], s["R"], pi.astype(np.float32), N=s["N"],
            background_pi=pi0,
            background_log_volume=float(s["background_log_volume"]))

    # ------------------------------------------------------------- save/load

    def save(self, path: str) -> None:
        """One .npz, every field fp32, written atomically. A plain Gaussian
        model writes format version 1, one with a background version 2 (the
        two background scalars added, as float64), one with Student-t
        components version 3 (version 1 plus student_t_nu, as float64)."""
        version = (FORMAT_VERSION_BACKGROUND if self.has_background
                   else FORMAT_VERSION_STUDENT_T if self.is_student_t
                   else FORMAT_VERSION)
        payload = {"format_version": np.float32(version)}
        for name in _ARRAYS:
            payload[name] = getattr(self, name).numpy()
        for name in _FLAGS:
            payload[name] = np.float32(getattr(self, name))
        if self.has_background:
            for name in _BACKGROUND:
                payload[name] = np.float64(getattr(self, name))
        if self.is_student_t:
            # version 3: version 1 plus the degrees of freedom (float64)
            for name in _STUDENT_T:
                payload[name] = np.float64(getattr(self, name))
        # np.savez appends .npz when missing — keep the suffix on the temp name
        tmp = f"{path}.tmp.{os.getpid()}.npz"
        np.savez(tmp, **payload)
        os.replace(tmp, path)

    @classmethod
    def load(cls, path: str) -> "GmmModel":
        """Load a model written by save(). Raises ValueError when the file
        is not a readable .npz, misses keys, has another format version or
        holds arrays of inconsistent shapes (OSError when it is absent)."""
        if not os.path.exists(path):
            raise FileNotFoundError(f"model file not found: {path}")
        try:
            with np.load(path, allow_pickle=False) as z:
                have = set(z.files)
                # the key set is strict per format version
                version = (float(np.asarray(z["format_version"]))
                           if "format_version" in have else FORMAT_VERSION)
                keys = _KEYS_BY_VERSION.get(version, _KEYS)
                if have != set(keys):
                    missing = sorted(set(keys) - have)
                    extra = sorted(have - set(keys))
                    raise ValueError(
                        f"not a GmmModel file: missing keys {missing}, "
                        f"unexpected keys {extra}")
                fields = {name: np.asarray(z[name]) for name in keys}
        except ValueError as e:
            raise ValueError(f"cannot load model {path}: {e}") from None
        except Exception as e:  # noqa: BLE001 — truncated / not a zip
            raise ValueError(
                f"cannot load model {path}: unreadable .npz ({e})") from None
        version = float(fields["format_version"])
        if version not in _KEYS_BY_VERSION:
            raise ValueError(f"cannot load model {path}: format version "
                             f"{version:g}, this build reads "
                             f"{sorted(_KEYS_BY_VERSION)}")
        scalars = {name: float(fields[name])
                   for name in _BACKGROUND + _STUDENT_T if name in fields}
        try:
            return cls(**{name: torch.from_numpy(
                              fields[name].astype(np.float32))
                          for name in _ARRAYS},
                       diag_only=bool(fields["diag_only"]),
                       bug_compat=bool(fields["bug_compat"]), **scalars)
        except ValueError as e:
            raise ValueError(f"cannot load model {path}: {e}") from None

    # --------------------------------------------------------------- scoring

    def _check_data(self, data) -> torch.Tensor:
        x = _as_events(data)
        if x.shape[1] != self.num_dimensions:
            raise ValueError(
                f"data has D={x.shape[1]} but the model has "
                f"D={self.num_dimensions}")
        return x

    @staticmethod
    def _device(device) -> torch.device:
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        return torch.device(device)

    def _on(self, dev: torch.device) -> GmmState:
        """Internal-frame parameters on `dev`."""
        return GmmState(N=self.N, pi=self.pi, constant=self.constant,
                        avgvar=self.avgvar, means=self.means_centered,
                        R=self.R, Rinv=self.Rinv).to(dev)

    def _stage(self, chunk: torch.Tensor, center: torch.Tensor,
               estep_dtype: str) -> torch.Tensor:
        """The engine's resident E-step copy of a chunk: centred, [D, n]."""
        z = (chunk - center.unsqueeze(0)).T.contiguous()
        if estep_dtype == "bf16" and z.is_cuda:
            z = z.to(torch.bfloat16)
        return z

    def predict(self, data, device=None, estep_dtype: str = "fp32",
                chunk_events: int = 1 << 22) -> Prediction:
        """Cluster, ln p(x) and assigned posterior of every event of `data`
        ([N, D] numpy array or CPU tensor). Events go through the device in
        chunks of `chunk_events`, so N is bounded by host memory.

        cuda, D <= 31: the classify kernels (12 bytes per event come back);
        cuda, D > 31: the log-weight kernels per chunk, then estep_lse and
        a first-argmax; cpu: cpu_reference.classify."""
        if estep_dtype not in ("fp32", "bf16"):
            raise ValueError("estep_dtype must be 'fp32' or 'bf16'")
        if chunk_events < 1:
            raise ValueError("chunk_events must be >= 1")
        x = self._check_data(data)
        dev = self._device(device)
        n, d = x.shape
        k = self.num_clusters
        labels = np.empty(n, dtype=np.int32)
        log_prob = np.empty(n, dtype=np.float32)
        max_post = np.empty(n, dtype=np.float32)
        st = self._on(dev)
        center = self.center.to(dev)
        # a t model takes the [K, n]-buffer route at every D (the fused
        # classify kernel is Gaussian-only)
        fused = F.estep_classify_available(dev, d) and not self.is_student_t
        big = (not fused) and F.estep_big_available(dev, estep_dtype, d)
        if fused or big:  # factor tables: once per call
            fac, add = F.model_factor_tables(
                st.means, st.R, st.Rinv, st.constant, st.pi, self.diag_only,
                estep_dtype)
        for s in range(0, n, chunk_events):
            e = min(s + chunk_events, n)
            chunk = x[s:e].to(dev)
            if fused:
                lab, lse, pmax = F.estep_classify(chunk, center, fac, add,
                                                  estep_dtype)
            elif dev.type == "cuda":
                z = self._stage(chunk, center, estep_dtype)
                if big:
                    logw = torch.empty(k, e - s, dtype=torch.float32,
                                       device=dev)
                    (F.estep_logw_big_f32 if estep_dtype == "fp32"
                     else F.estep_logw_big)(z, fac, add, logw)
                else:
                    logw = F.estep_logw(z, st.means, st.Rinv, st.constant,
                                        st.pi, self.diag_only)
                if self.is_student_t:
                    # log-weights -> student_t_lse(posterior) -> argmax
                    logw, lse = F.student_t_posteriors(
                        logw, add if big else F.logw_offsets(st.constant,
                                                             st.pi),
                        self.student_t_nu, d)
                else:
                    lse = torch.empty(e - s, dtype=torch.float32, device=dev)
                    F.estep_lse(logw, lse, need_lik=False)
                m = logw.max(dim=0).values
                idx = torch.arange(k, dtype=torch.int32,
                                   device=dev).unsqueeze(1)
                lab = torch.where(logw == m.unsqueeze(0), idx,
                                  torch.full_like(idx, k)
                                  ).min(dim=0).values.clamp(max=k - 1)
                pmax = m if self.is_student_t else torch.exp(m - lse)
            elif self.is_student_t:
                logw = cpu.estep_logw(
                    self._stage(chunk, center, estep_dtype), st.means,
                    st.Rinv, st.constant, st.pi, self.diag_only)
                _, lse, tau = cpu.student_t_posteriors(
                    logw, F.logw_offsets(st.constant, st.pi),
                    self.student_t_nu, d)
                pmax = tau.max(dim=0).values
                idx = torch.arange(k, dtype=torch.int32).unsqueeze(1)
                lab = torch.where(tau == pmax.unsqueeze(0), idx,
                                  torch.full_like(idx, k)
                                  ).min(dim=0).values.clamp(max=k - 1)
            else:
                lab, lse, pmax = cpu.classify(
                    self._stage(chunk, center, estep_dtype), st.means,
                    st.Rinv, st.constant, st.pi, self.diag_only)
            if self.has_background:
                lab, lse, pmax = self._background_pass(lab, lse, pmax)
            labels[s:e] = lab.cpu().numpy()
            log_prob[s:e] = lse.cpu().numpy()
            max_post[s:e] = pmax.cpu().numpy()
        return Prediction(
            labels=labels, log_prob=log_prob, max_posterior=max_post,
            log_likelihood=float(log_prob.astype(np.float64).sum()),
            counts=np.bincount(labels[labels >= 0],
                               minlength=k).astype(np.int64),
            background_count=int((labels < 0).sum()))

    def _background_pass(self, lab: torch.Tensor, lse: torch.Tensor,
                         pmax: torch.Tensor
                         ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """The background on top of a Gaussian-only classification, from its
        12 bytes per event alone (a few elementwise ops; predict is bound by
        the host-to-device copy): with lse_b = logaddexp(lse, b) the
        background's posterior is r0 = exp(b - lse_b) and the largest
        cluster posterior pmax * exp(lse - lse_b) (the largest log-weight is
        lse + ln pmax). Label -1 where r0 is strictly the larger — or where
        the event is so far out that no cluster posterior is a number;
        log_prob = ln(1 - pi0) + lse_b."""
        _, b, _ = cpu.background_update(self.background_pi, 1.0,
                                        self.background_log_volume)
        bt = torch.full_like(lse, b)
        lse_b = torch.logaddexp(lse, bt)
        r0 = torch.exp(bt - lse_b)
        g = pmax * torch.exp(lse - lse_b)
        is_bg = ~(r0 <= g)
        lab = torch.where(is_bg, torch.full_like(lab, -1), lab)
        pmax = torch.where(is_bg, r0, g)
        return lab, lse_b + float(np.log1p(-self.background_pi)), pmax

    def score(self, data, device=None, estep_dtype: str = "fp32",
              chunk_events: int = 1 << 22) -> float:
        """Total log-likelihood ln p(data) under the model."""
        return self.predict(data, device, estep_dtype,
                            chunk_events).log_likelihood

    def posteriors(self, data, device=None, estep_dtype: str = "fp32",
                   chunk_events: int = 1 << 22) -> np.ndarray:
        """Full posterior matrix [K, N] (fp32), for .results-style output:
        per chunk the same ops EmEngine.recompute_memberships runs, so the
        training data gives the training run's memberships. A model with a
        background returns [K + 1, N], the background's row last."""
        x = self._check_data(data)
        dev = self._device(device)
        n = x.shape[0]
        rows = self.num_clusters + (1 if self.has_background else 0)
        out = np.empty((rows, n), dtype=np.float32)
        st = self._on(dev)
        center = self.center.to(dev)
        for s in range(0, n, chunk_events):
            e = min(s + chunk_events, n)
            z = self._stage(x[s:e].to(dev), center, estep_dtype)
            logw = F.estep_logw(z, st.means, st.Rinv, st.constant, st.pi,
                                self.diag_only)
            if self.is_student_t:
                w, _ = F.student_t_posteriors(
                    logw, F.logw_offsets(st.constant, st.pi),
                    self.student_t_nu, self.num_dimensions)
            elif self.has_background:
                w = F.background_posteriors(logw, self.background_pi,
                                            self.background_log_volume)
            else:
                w, _ = F.estep_posteriors(logw)
            out[:, s:e] = w.cpu().numpy()
        return out
