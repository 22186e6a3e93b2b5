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

_ARRAYS = ("center", "means_centered", "pi", "N", "constant", "avgvar",
           "R", "Rinv")
_FLAGS = ("diag_only", "bug_compat")
_KEYS = ("format_version",) + _ARRAYS + _FLAGS


@dataclasses.dataclass
class Prediction:
    labels: np.ndarray         # int32 [N], first argmax of the posteriors
    log_prob: np.ndarray       # fp32 [N], ln p(x_e)
    max_posterior: np.ndarray  # fp32 [N], posterior of the assigned cluster
    log_likelihood: float      # float64 sum of log_prob
    counts: np.ndarray         # int64 [K], events per label


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

    def __post_init__(self):
        for name in _ARRAYS:
            setattr(self, name, torch.as_tensor(getattr(self, name))
                    .detach().to("cpu", torch.float32).contiguous())
        self.diag_only = bool(self.diag_only)
        self.bug_compat = bool(self.bug_compat)
        self._validate()

    def _validate(self) -> None:
        if self.means_centered.dim() != 2:
            raise ValueError("means_centered must be [K, D]")
        k, d = self.means_centered.shape
        want = {"center": (d,), "pi": (k,), "N": (k,), "constant": (k,),
                "avgvar": (k,), "R": (k, d, d), "Rinv": (k, d, d)}
        if k < 1 or d < 1:
            raise ValueError(f"model needs K >= 1 and D >= 1, got {k}x{d}")
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
    def means(self) -> torch.Tensor:
        """Cluster means in the data's own frame."""
        return self.means_centered + self.center.unsqueeze(0)

    # ---------------------------------------------------------- construction

    @classmethod
    def from_state(cls, state: GmmState, center: torch.Tensor,
                   diag_only: bool = False,
                   bug_compat: bool = True) -> "GmmModel":
        """From an engine state whose means are in the centred frame."""
        return cls(center=center.clone(), means_centered=state.means.clone(),
                   pi=state.pi.clone(), N=state.N.clone(),
                   constant=state.constant.clone(),
                   avgvar=state.avgvar.clone(), R=state.R.clone(),
                   Rinv=state.Rinv.clone(), diag_only=diag_only,
                   bug_compat=bug_compat)

    @classmethod
    def from_params(cls, means, R, pi, N=None, center=None,
                    diag_only: bool = False) -> "GmmModel":
        """From means [K, D] (data frame), covariances and weights; Rinv and
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
                   diag_only=diag_only, bug_compat=False)

    @classmethod
    def from_summary(cls, path: str) -> "GmmModel":
        """From a .summary file (this project's or the reference's).

        LOSSY: .summary holds %.3f means and covariances and %f weights, so
        the model is the fitted one rounded to that; Rinv and constant are
        recomputed from the rounded R. Use save()/load() to keep a model
        exactly."""
        from ..utils.io import read_summary
        s = read_summary(path)
        return cls.from_params(s["means"], s["R"], s["pi"], N=s["N"])

    # ------------------------------------------------------------- save/load

    def save(self, path: str) -> None:
        """One .npz, every field fp32, written atomically."""
        payload = {"format_version": np.float32(FORMAT_VERSION)}
        for name in _ARRAYS:
            payload[name] = getattr(self, name).numpy()
        for name in _FLAGS:
            payload[name] = np.float32(getattr(self, name))
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
                if have != set(_KEYS):
                    missing = sorted(set(_KEYS) - have)
                    extra = sorted(have - set(_KEYS))
                    raise ValueError(
                        f"not a GmmModel file: missing keys {missing}, "
                        f"unexpected keys {extra}")
                fields = {name: np.asarray(z[name]) for name in _KEYS}
        except ValueError as e:
            raise ValueError(f"cannot load model {path}: {e}") from None
        except Exception as e:  # noqa: BLE001 — truncated / not a zip
            raise ValueError(
                f"cannot load model {path}: unreadable .npz ({e})") from None
        version = float(fields["format_version"])
        if version != FORMAT_VERSION:
            raise ValueError(f"cannot load model {path}: format version "
                             f"{version:g}, this build reads {FORMAT_VERSION}")
        try:
            return cls(**{name: torch.from_numpy(
                              fields[name].astype(np.float32))
                          for name in _ARRAYS},
                       diag_only=bool(fields["diag_only"]),
                       bug_compat=bool(fields["bug_compat"]))
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
        fused = F.estep_classify_available(dev, d)
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
                lse = torch.empty(e - s, dtype=torch.float32, device=dev)
                F.estep_lse(logw, lse, need_lik=False)
                m = logw.max(dim=0).values
                idx = torch.arange(k, dtype=torch.int32,
                                   device=dev).unsqueeze(1)
                lab = torch.where(logw == m.unsqueeze(0), idx,
                                  torch.full_like(idx, k)
                                  ).min(dim=0).values.clamp(max=k - 1)
                pmax = torch.exp(m - lse)
            else:
                lab, lse, pmax = cpu.classify(
                    self._stage(chunk, center, estep_dtype), st.means,
                    st.Rinv, st.constant, st.pi, self.diag_only)
            labels[s:e] = lab.cpu().numpy()
            log_prob[s:e] = lse.cpu().numpy()
            max_post[s:e] = pmax.cpu().numpy()
        return Prediction(
            labels=labels, log_prob=log_prob, max_posterior=max_post,
            log_likelihood=float(log_prob.astype(np.float64).sum()),
            counts=np.bincount(labels, minlength=k).astype(np.int64))

    def score(self, data, device=None, estep_dtype: str = "fp32",
              chunk_events: int = 1 << 22) -> float:
        """Total log-likelihood ln p(data) under the model."""
        return self.predict(data, device, estep_dtype,
                            chunk_events).log_likelihood

    def posteriors(self, data, device=None, estep_dtype: str = "fp32",
                   chunk_events: int = 1 << 22) -> np.ndarray:
        """Full posterior matrix [K, N] (fp32), for .results-style output:
        per chunk the same ops EmEngine.recompute_memberships runs, so the
        training data gives the training run's memberships."""
        x = self._check_data(data)
        dev = self._device(device)
        n = x.shape[0]
        out = np.empty((self.num_clusters, n), dtype=np.float32)
        st = self._on(dev)
        center = self.center.to(dev)
        for s in range(0, n, chunk_events):
            e = min(s + chunk_events, n)
            z = self._stage(x[s:e].to(dev), center, estep_dtype)
            logw = F.estep_logw(z, st.means, st.Rinv, st.constant, st.pi,
                                self.diag_only)
            w, _ = F.estep_posteriors(logw)
            out[:, s:e] = w.cpu().numpy()
        return out
