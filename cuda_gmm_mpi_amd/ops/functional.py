"""Device-dispatched EM ops: torch-CPU reference vs HIP/CDNA4 kernels.

The engine calls only these. CPU tensors -> ``cpu_reference`` (golden
semantics); CUDA tensors -> hand-written gfx950 kernels via the extension
(loud failure when unbuilt; no eager fallback).

GEMM-shaped cold ops (mean numerators = W @ [X;1]^T) go through rocBLAS via
torch.matmul, per the MI355X design rules (library GEMMs for plain GEMMs,
custom kernels for the fused hot ops).
"""
from __future__ import annotations

import os

import torch

from ..models import seed as seed_mod
from . import cpu_reference as cpu
from .backend import hip_ext


def estep_logw(x: torch.Tensor, means: torch.Tensor, rinv: torch.Tensor,
               constant: torch.Tensor, pi: torch.Tensor,
               diag_only: bool = False,
               out: torch.Tensor | None = None) -> torch.Tensor:
    """logw [K, N]; x may be fp32 or bf16 (bf16 reads, fp32 accumulate)."""
    if x.is_cuda:
        k, n = means.shape[0], x.shape[1]
        if out is None:
            out = torch.empty((k, n), dtype=torch.float32, device=x.device)
        hip_ext().estep_logw(
            x, means, rinv, constant, torch.log(pi), out, bool(diag_only)
        )
        return out
    logw = cpu.estep_logw(x.float(), means, rinv, constant, pi, diag_only)
    if out is not None:
        out.copy_(logw)
        return out
    return logw


def estep_posteriors(logw: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """In-place posteriors on CUDA; returns (w, likelihood scalar tensor)."""
    if logw.is_cuda:
        nblocks = 1024
        partial = torch.zeros(nblocks, dtype=torch.float32, device=logw.device)
        hip_ext().estep_posteriors(logw, partial)
        return logw, partial.sum()
    w, lik = cpu.estep_posteriors(logw)
    logw.copy_(w)  # in-place like the CUDA path: the buffer becomes posteriors
    return logw, lik


def estep_lse(logw: torch.Tensor, lse: torch.Tensor,
              need_lik: bool = True,
              lik_out: torch.Tensor | None = None) -> torch.Tensor | None:
    """Per-event log-sum-exp into lse [N] + likelihood scalar (CUDA),
    reduced into ``lik_out`` [1] when one is given.

    logw is NOT normalized — the lse-aware M-step kernels apply
    exp(logw - lse) while staging w, deleting the posterior write+read
    round trip of the two-kernel path."""
    nblocks = 1024
    partial = torch.zeros(nblocks, dtype=torch.float32, device=logw.device)
    hip_ext().estep_lse(logw, lse, partial)
    if not need_lik:
        return None
    lik = (lik_out if lik_out is not None
           else torch.empty(1, dtype=torch.float32, device=logw.device))
    hip_ext().reduce_scalar(partial, lik)
    return lik


def event_weight_lse(lse: torch.Tensor, s: torch.Tensor, lns: torch.Tensor,
                     lse_w: torch.Tensor, need_lik: bool = True,
                     lik_out: torch.Tensor | None = None
                     ) -> torch.Tensor | None:
    """Per-event training weights on the lse family (CUDA): writes
    lse_w [N] = lse - lns (+inf where s == 0), the shifted lse the lse-aware
    M-step kernels read so that they stage s * posterior. ``lns`` is ln s
    with -inf at s == 0. With ``need_lik`` returns the weighted
    log-likelihood sum_e s_e lse_e (zero-weight events skipped), reduced
    into ``lik_out`` [1] when one is given; fixed block partials, so it is
    deterministic. ``lse`` is left untouched."""
    ext = hip_ext()
    if not need_lik:
        ext.event_weight_lse(lse, s, lns, lse_w, lse.new_empty(0))
        return None
    # every launched block writes its partial slot: no zero-fill needed
    partial = torch.empty(ext.event_weight_lse_blocks(lse.numel()),
                          dtype=torch.float32, device=lse.device)
    ext.event_weight_lse(lse, s, lns, lse_w, partial)
    lik = (lik_out if lik_out is not None
           else torch.empty(1, dtype=torch.float32, device=lse.device))
    ext.reduce_scalar(partial, lik)
    return lik


def background_state(device) -> torch.Tensor:
    """The 4-float device state of a background component, switched off:
    [pi0, b, lik_add, n0] = [0, -inf, 0, 0] (pi0 = 0 is a fixed point)."""
    return torch.tensor([0.0, float("-inf"), 0.0, 0.0], dtype=torch.float32,
                        device=device)


def background_partial(n: int, device) -> torch.Tensor:
    """The persistent partial buffer of background_lse for n events: CUDA
    [2, blocks] (row 0 the n0 partials, row 1 the likelihood's); CPU [2, 1]
    holding the two sums themselves."""
    dev = torch.device(device)
    blocks = (int(hip_ext().event_weight_lse_blocks(n))
              if dev.type == "cuda" else 1)
    return torch.zeros((2, blocks), dtype=torch.float32, device=dev)


def background_lse(lse: torch.Tensor, bg: torch.Tensor,
                   s: torch.Tensor | None, lns: torch.Tensor | None,
                   lse_m: torch.Tensor, partial: torch.Tensor,
                   lse_b: torch.Tensor | None = None, need_lik: bool = True,
                   lik_out: torch.Tensor | None = None
                   ) -> torch.Tensor | None:
    """Uniform background on the lse family. ``bg`` is background_state
    (bg[1] = b is read on the device, so a captured graph follows it);
    writes lse_m [N], the lse the lse-aware M-step kernels read (lse_b =
    logaddexp(lse, b), shifted by -ln s and +inf at s == 0 with weights: it
    replaces event_weight_lse), lse_b itself when a buffer is given, and the
    n0 partials into ``partial`` (background_partial). With ``need_lik``
    returns sum_e s_e lse_b_e reduced into ``lik_out`` [1] when given.
    ``lse`` is left untouched. CPU tensors: the cpu_reference twin."""
    if not lse.is_cuda:
        lb, lm, n0, lik = cpu.background_lse(lse, float(bg[1]), s)
        lse_m.copy_(lm)
        if lse_b is not None:
            lse_b.copy_(lb)
        partial[0, 0] = n0
        if not need_lik:
            return None
        partial[1, 0] = lik
        out = lik_out if lik_out is not None else lse.new_empty(1)
        out.copy_(lik.reshape(1))
        return out
    ext = hip_ext()
    empty = lse.new_empty(0)
    ext.background_lse(lse, bg, s if s is not None else empty,
                       lns if s is not None else empty, lse_m,
                       lse_b if lse_b is not None else empty,
                       partial if need_lik else partial[0])
    if not need_lik:
        return None
    lik = (lik_out if lik_out is not None
           else torch.empty(1, dtype=torch.float32, device=lse.device))
    ext.reduce_scalar(partial[1], lik)
    return lik


def background_update(n0_part: torch.Tensor, n_total: float,
                      log_volume: float, bg: torch.Tensor) -> None:
    """bg <- [pi0, b, lik_add, n0] from the n0 partials (contract:
    cpu_reference.background_update); one block on CUDA, no host sync."""
    if not bg.is_cuda:
        n0 = n0_part.sum()
        pi0, b, lik_add = cpu.background_update(float(n0), n_total,
                                                log_volume)
        bg.copy_(torch.tensor([pi0, b, lik_add, float(n0)],
                              dtype=torch.float64))
        return
    hip_ext().background_update(n0_part, int(n0_part.numel()),
                                float(n_total), float(log_volume), bg)


background_update_host = cpu.background_update


def estep_posteriors_background(logw: torch.Tensor, bg: torch.Tensor,
                                s: torch.Tensor | None,
                                lse_b: torch.Tensor, partial: torch.Tensor
                                ) -> tuple[torch.Tensor,
                                           torch.Tensor | None, torch.Tensor]:
    """CPU engine path of a fit with a background: logw becomes
    exp(logw - lse_b) in place (the Gaussian posteriors); lse_b and the n0
    of ``partial`` are filled; returns (w, w * s for the M-step of a
    weighted fit or None, likelihood sum_e s_e lse_b_e)."""
    w, w_s, lb, n0, lik = cpu.estep_posteriors_background(
        logw, float(bg[1]), s)
    logw.copy_(w)
    lse_b.copy_(lb)
    partial[0, 0] = n0
    partial[1, 0] = lik
    return logw, w_s, lik


def background_log_volume(data, weights=None) -> float:
    """ln V of the bounding box of ``data`` [N, D]: float64
    sum_d ln(max_d - min_d) over the events with weight > 0 (all without
    weights). ValueError naming the dimension when a range is zero."""
    x = torch.as_tensor(data).double()
    if weights is not None:
        x = x[torch.as_tensor(weights).reshape(-1) > 0]
    if x.shape[0] == 0:
        raise ValueError("background volume: no event with weight > 0")
    rng = x.max(dim=0).values - x.min(dim=0).values
    bad = torch.nonzero(~(rng > 0)).reshape(-1)
    if bad.numel():
        raise ValueError(
            f"background volume: dimension {int(bad[0])} has zero range "
            f"(give background_log_volume explicitly)")
    return float(torch.log(rng).sum())


def background_posteriors(logw: torch.Tensor, pi0: float,
                          log_volume: float) -> torch.Tensor:
    """[K + 1, N] posteriors of a mixture with a background from the
    Gaussian log-weights (output path: the lse kernel or its CPU twin, then
    a few torch ops): rows 0..K-1 exp(logw - lse_b), the last row
    r0 = exp(b - lse_b)."""
    if logw.is_cuda:
        lse = torch.empty(logw.shape[1], dtype=torch.float32,
                          device=logw.device)
        estep_lse(logw, lse, need_lik=False)
    else:
        lse = cpu.estep_lse(logw)
    _, b, _ = cpu.background_update(pi0, 1.0, log_volume)
    bt = torch.full_like(lse, b)
    lse_b = torch.logaddexp(lse, bt)
    r0 = torch.exp(bt - lse_b) if b != float("-inf") else torch.zeros_like(lse)
    return torch.cat([torch.exp(logw - lse_b.unsqueeze(0)),
                      r0.unsqueeze(0)], dim=0)


student_t_delta = cpu.student_t_delta


def student_t_partials(n: int, k: int, device
                       ) -> tuple[torch.Tensor, torch.Tensor]:
    """(n_part [blocks, K], lik_part [blocks]) for student_t_lse over n
    events on ``device`` (CUDA). Every launched block writes its row and its
    slot, so they are never zero-filled."""
    blocks = int(hip_ext().student_t_lse_blocks(n))
    return (torch.empty((blocks, k), dtype=torch.float32, device=device),
            torch.empty(blocks, dtype=torch.float32, device=device))


def student_t_lse(logw: torch.Tensor, add: torch.Tensor, nu: float, d: int,
                  s: torch.Tensor | None, lns: torch.Tensor | None,
                  lse_m: torch.Tensor, lse_t: torch.Tensor,
                  n_part: torch.Tensor, lik_part: torch.Tensor,
                  n_c: torch.Tensor, need_lik: bool = True,
                  lik_out: torch.Tensor | None = None
                  ) -> torch.Tensor | None:
    """Student-t components on the lse family, train mode (CUDA). ``logw``
    [K, N] holds the Gaussian log-weights add_c - q/2 of any lse-family
    E-step and is rewritten in place to lt + ln u; writes lse_m [N] (what the
    lse-aware M-step kernels read: lse_t, with weights lse_t - lns and +inf
    at s == 0 — it replaces event_weight_lse), lse_t [N], and reduces the
    block partials of the responsibilities into n_c [K]. With ``need_lik``
    returns sum_e s_e lse_t reduced into ``lik_out`` [1] when given.
    Contract: cpu_reference.student_t_lse."""
    ext = hip_ext()
    empty = logw.new_empty(0)
    k = logw.shape[0]
    # a sweep shrinks K: the first blocks * K floats of the buffer, as rows
    part = n_part.reshape(-1)[:lik_part.numel() * k].view(-1, k)
    ext.student_t_lse(logw, add, s if s is not None else empty,
                      lns if s is not None else empty, lse_m, lse_t,
                      part, lik_part if need_lik else empty,
                      float(nu), int(d), student_t_delta(nu, d), True)
    ext.reduce_chunks(part, n_c)
    if not need_lik:
        return None
    lik = (lik_out if lik_out is not None
           else torch.empty(1, dtype=torch.float32, device=logw.device))
    ext.reduce_scalar(lik_part, lik)
    return lik


def student_t_posteriors(logw: torch.Tensor, add: torch.Tensor, nu: float,
                         d: int) -> tuple[torch.Tensor, torch.Tensor]:
    """(tau [K, N], lse_t [N]): the t posteriors and ln p(x_e) from Gaussian
    log-weights logw = add_c - q/2, which is overwritten (posterior mode of
    the kernel, then exp(lt - lse_t) in place). The output / scoring path."""
    if not logw.is_cuda:
        _, lse_t, tau = cpu.student_t_posteriors(logw, add, nu, d)
        logw.copy_(tau)
        return logw, lse_t
    lse_t = torch.empty(logw.shape[1], dtype=torch.float32,
                        device=logw.device)
    empty = logw.new_empty(0)
    hip_ext().student_t_lse(logw, add.contiguous(), empty, empty, empty,
                            lse_t, empty, empty, float(nu), int(d),
                            student_t_delta(nu, d), False)
    logw.sub_(lse_t.unsqueeze(0)).exp_()
    return logw, lse_t


def student_t_pi(n_c: torch.Tensor, constant: torch.Tensor | None,
                 n_out: torch.Tensor, pi: torch.Tensor,
                 add: torch.Tensor | None = None) -> None:
    """N <- n_c, pi <- n_c / sum n_c (1e-10 where n_c < 0.5) and, when
    ``add`` is given, add <- constant + ln pi: the mixing weights of a t fit
    come from the responsibilities, not from the moments' corner. One block
    on CUDA, no host sync. Contract: cpu_reference.student_t_pi."""
    if not n_c.is_cuda:
        n, p, a = cpu.student_t_pi(n_c, constant if add is not None else None)
        n_out.copy_(n)
        pi.copy_(p)
        if add is not None:
            add.copy_(a)
        return
    empty = n_c.new_empty(0)
    hip_ext().student_t_pi(n_c, constant if add is not None else empty,
                           n_out, pi, add if add is not None else empty)


def estep_posteriors_student_t(logw: torch.Tensor, add: torch.Tensor,
                               nu: float, d: int, s: torch.Tensor | None,
                               n_c: torch.Tensor
                               ) -> tuple[torch.Tensor, torch.Tensor,
                                          torch.Tensor]:
    """CPU engine path of a t fit: logw becomes tau in place, n_c [K] is
    filled; returns (tau, s tau u for the M-step, likelihood)."""
    tau, w_m, n, lik = cpu.estep_posteriors_student_t(logw, add, nu, d, s)
    logw.copy_(tau)
    n_c.copy_(n)
    return logw, w_m, lik


def estep_posteriors_weighted(logw: torch.Tensor, s: torch.Tensor
                              ) -> tuple[torch.Tensor, torch.Tensor,
                                         torch.Tensor]:
    """CPU engine path of a weighted fit: logw becomes the normalized
    posteriors in place (like estep_posteriors); returns (w, w * s for the
    M-step, weighted likelihood scalar tensor)."""
    w, w_s, lik = cpu.estep_posteriors_weighted(logw, s)
    logw.copy_(w)
    return logw, w_s, lik


def mstep_n_means(x_aug_t: torch.Tensor, w: torch.Tensor
                  ) -> tuple[torch.Tensor, torch.Tensor]:
    """(N [K], mean numerators [K, D]) via one rocBLAS GEMM.

    x_aug_t: [N, D+1] = [X^T | 1] (precomputed once). Fuses the reference's
    mstep_N and mstep_means kernels (gaussian_kernel.cu:522-577) into a
    single skinny GEMM: W @ X_aug^T -> [K, D+1].
    """
    nm = w @ x_aug_t                        # [K, D+1]
    return nm[:, -1].contiguous(), nm[:, :-1].contiguous()


_tri_cache: dict = {}


def _tri_unpack_index(d: int, device) -> torch.Tensor:
    """[D*D] gather index from packed lower-triangle to full matrix."""
    key = (d, str(device))
    idx = _tri_cache.get(key)
    if idx is None:
        full = torch.empty(d, d, dtype=torch.long)
        for i in range(d):
            for j in range(d):
                r, c = (i, j) if i >= j else (j, i)
                full[i, j] = r * (r + 1) // 2 + c
        idx = full.reshape(-1).to(device)
        _tri_cache[key] = idx
    return idx


def mstep_covariance_s(x: torch.Tensor, w: torch.Tensor,
                       out: torch.Tensor | None = None,
                       nchunk: int = 64,
                       lse: torch.Tensor | None = None) -> torch.Tensor:
    """Uncentered weighted second moments S [K, D, D].

    CUDA: custom LDS-tiled kernel (the covariance showpiece) producing
    deterministic per-chunk packed partials, summed + unpacked here; CPU:
    batched torch matmuls.
    """
    if x.is_cuda and x.shape[0] > 128:
        # past the covariance kernel's D cap: per-cluster rocBLAS GEMMs
        # (the exact-fp32 D>128 quadrant; ~K GEMMs of D x N x D)
        k, n = w.shape
        d = x.shape[0]
        if lse is not None and lse.numel() > 0:
            w = torch.exp(w - lse.unsqueeze(0))
        s = out if out is not None else torch.empty(
            (k, d, d), dtype=torch.float32, device=x.device)
        for c in range(k):
            s[c] = (x * w[c].unsqueeze(0)) @ x.T
        return s
    if x.is_cuda:
        k = w.shape[0]
        d = x.shape[0]
        n = x.shape[1]
        p = d * (d + 1) // 2
        te = min((16384 - 4 * d) // (d + 1) & ~3, 256)  # matches gmm_ext.hip
        tiles = (n + te - 1) // te
        nchunk = int(min(nchunk, tiles))
        partials = torch.empty((nchunk, k, p), dtype=torch.float32,
                               device=x.device)
        if lse is None:
            lse = torch.empty(0, dtype=torch.float32, device=x.device)
        hip_ext().mstep_covariance_partials(x, w, lse, partials)
        packed = torch.empty((k, p), dtype=torch.float32, device=x.device)
        hip_ext().reduce_chunks(partials, packed)         # [K, P]
        idx = _tri_unpack_index(d, x.device)
        s = packed[:, idx].view(k, d, d)
        if out is not None:
            out.copy_(s)
            return out
        return s
    k, n = w.shape
    d = x.shape[0]
    xf = x.float()
    s = out if out is not None else torch.empty((k, d, d), dtype=torch.float32)
    for c in range(k):
        s[c] = (xf * w[c].unsqueeze(0)) @ xf.T
    return s


def constants(r: torch.Tensor, means: torch.Tensor | None = None,
              diag_only: bool = False, mfac: torch.Tensor | None = None,
              mfac32: torch.Tensor | None = None,
              pi_add: tuple[torch.Tensor, torch.Tensor] | None = None,
              out: tuple[torch.Tensor, torch.Tensor] | None = None
              ) -> tuple[torch.Tensor, torch.Tensor]:
    """(Rinv [K,D,D], constant [K]) via no-pivot LU + ln|det|.

    On CUDA, when ``mfac`` (bf16 [K,2,32,32]) is given, the kernel also
    emits the fused-E-step factor M = [U | -U mu] (U^T U = Rinv) as bf16
    hi/lo fragment pairs — requires ``means`` and D <= 31.
    """
    k, d, _ = r.shape
    if r.is_cuda and d > 142:
        # the constants/emission kernels stage TWO d x (d|1) fp32 planes
        # + a d-float mu buffer in LDS (race-free LU snapshot /
        # triangular-inverse working set); that crosses gfx950's 160 KB
        # workgroup limit at exactly D = 143. Fall back to the CPU LU
        # (bit-faithful invert_cpu math) — the MFMA factor paths are
        # gated to D <= 142, so no caller needs mfac here.
        if mfac is not None and mfac.numel() > 0:
            raise ValueError("factor emission needs D <= 142 (LDS bound)")
        rinv_c, const_c = cpu.compute_constants(r.detach().cpu(), diag_only)
        rinv = out[0] if out is not None else torch.empty_like(r)
        rinv.copy_(rinv_c.to(r.device))
        const = const_c.to(r.device)
        if pi_add is not None:
            pi_t, add_t = pi_add
            const_t = (out[1] if out is not None
                       else torch.empty(k, dtype=torch.float32,
                                        device=r.device))
            const_t.copy_(const)
            add_t.copy_(const + torch.log(pi_t))
            return rinv, const_t
        if out is not None:
            out[1].copy_(const)
            return rinv, out[1]
        return rinv, const
    if r.is_cuda:
        rinv = out[0] if out is not None else torch.empty_like(r)
        logdet = torch.empty(k, dtype=torch.float32, device=r.device)
        if means is None:
            means = torch.zeros(k, d, dtype=torch.float32, device=r.device)
        if mfac is None:
            mfac = torch.empty(0, dtype=torch.bfloat16, device=r.device)
        if mfac32 is None:
            mfac32 = torch.empty(0, dtype=torch.float32, device=r.device)
        empty = torch.empty(0, dtype=torch.float32, device=r.device)
        if pi_add is not None:
            pi_t, add_t = pi_add
            const_t = (out[1] if out is not None
                       else torch.empty(k, dtype=torch.float32,
                                        device=r.device))
            hip_ext().constants(r, means, pi_t, rinv, logdet, const_t,
                                add_t, mfac, mfac32, bool(diag_only))
            if diag_only:  # diag kernel does not emit constant/add
                cval = -d * 0.5 * cpu.LOG_2PI - 0.5 * logdet
                if out is not None:
                    const_t.copy_(cval)
                else:
                    const_t = cval
                add_t.copy_(cval + torch.log(pi_t))
            return rinv, const_t
        hip_ext().constants(r, means, empty, rinv, logdet, empty, empty,
                            mfac, mfac32, bool(diag_only))
        const = -d * 0.5 * cpu.LOG_2PI - 0.5 * logdet
        if out is not None:
            out[1].copy_(const)
            const = out[1]
        return rinv, const
    rinv_c, const_c = cpu.compute_constants(r, diag_only)
    if out is not None:
        out[0].copy_(rinv_c)
        out[1].copy_(const_c)
        return out[0], out[1]
    return rinv_c, const_c


def _run_fused(entry: str, tile: int, z: torch.Tensor, fac: torch.Tensor,
               add: torch.Tensor, w_out: torch.Tensor, need_lik: bool,
               *lse: torch.Tensor, lik_out: torch.Tensor | None = None
               ) -> tuple[torch.Tensor, torch.Tensor | None]:
    """Launch one fused E-step entry point (`tile` events per block) and
    reduce its per-block likelihood partials, into `lik_out` [1] when the
    caller has a place for the scalar (saves it a device copy)."""
    ext = hip_ext()
    nblk = (z.shape[1] + tile - 1) // tile
    # every launched block writes its partial slot: no zero-fill needed
    partial = torch.empty(nblk, dtype=torch.float32, device=z.device)
    getattr(ext, entry)(z, fac, add, w_out, *lse, partial)
    if not need_lik:
        return w_out, None
    lik = (lik_out if lik_out is not None
           else torch.empty(1, dtype=torch.float32, device=z.device))
    ext.reduce_scalar(partial, lik)
    return w_out, lik


def estep_fused(z: torch.Tensor, mfac: torch.Tensor, add: torch.Tensor,
                w_out: torch.Tensor, lse: torch.Tensor,
                need_lik: bool = True, lik_out: torch.Tensor | None = None
                ) -> tuple[torch.Tensor, torch.Tensor | None]:
    """Fused bf16-MFMA E-step (CUDA only): LOG weights into w_out [K,N],
    per-event log-sum-exp into lse [N], returns (w_out, likelihood).
    Online-softmax over 256-event blocks; the lse-aware M-step applies
    exp(w_out - lse) on the fly — posteriors are never materialized."""
    return _run_fused("estep_fused", 256, z, mfac, add, w_out, need_lik, lse,
                      lik_out=lik_out)


def estep_fused_available(device: torch.device, dtype: str, d: int,
                          k: int) -> bool:
    """Fused path gate: D <= 31 (any K — the online-softmax redesign
    removed the K-sized logw LDS buffer)."""
    return device.type == "cuda" and d <= 31


def estep_fused_lds_available(device: torch.device, dtype: str, d: int,
                              k: int) -> bool:
    """v1 lw-in-LDS fast path: writes posteriors directly (the M-step
    then skips the exp at staging, which sits on its VALU-bound critical
    path — measured ~19 us/iter at K=64). LDS-bounded in K."""
    if device.type != "cuda" or d > 31:
        return False
    if dtype == "bf16":
        return 128 * 40 * 2 + 4 * k * 132 <= 64 * 1024   # K <= 104
    return 4 * (128 * 33 + k * 132) <= 64 * 1024         # K <= 85


def estep_fused_lds(z: torch.Tensor, mfac: torch.Tensor, add: torch.Tensor,
                    w_out: torch.Tensor, need_lik: bool = True,
                    lik_out: torch.Tensor | None = None
                    ) -> tuple[torch.Tensor, torch.Tensor | None]:
    """v1 fused bf16 E-step: POSTERIORS into w_out, likelihood scalar."""
    # GMM_ESTEP_LDS=legacy selects the first version of the kernel
    # (same-build A/B); the log-weights of the two are bitwise equal
    legacy = os.environ.get("GMM_ESTEP_LDS", "lds2") == "legacy"
    return _run_fused("estep_fused_lds" if legacy else "estep_fused_lds2",
                      128, z, mfac, add, w_out, need_lik, lik_out=lik_out)


def estep_fused_f32_lds(z: torch.Tensor, mfac32: torch.Tensor,
                        add: torch.Tensor, w_out: torch.Tensor,
                        need_lik: bool = True,
                        lik_out: torch.Tensor | None = None
                        ) -> tuple[torch.Tensor, torch.Tensor | None]:
    """v1 exact-f32 fused E-step: POSTERIORS into w_out."""
    return _run_fused("estep_fused_f32_lds", 128, z, mfac32, add, w_out,
                      need_lik, lik_out=lik_out)


def estep_fused_f32(z: torch.Tensor, mfac32: torch.Tensor, add: torch.Tensor,
                    w_out: torch.Tensor, lse: torch.Tensor,
                    need_lik: bool = True,
                    lik_out: torch.Tensor | None = None
                    ) -> tuple[torch.Tensor, torch.Tensor | None]:
    """Exact-f32 MFMA fused E-step (CUDA, D <= 31, any K): log weights
    into w_out, per-event log-sum-exp into lse."""
    return _run_fused("estep_fused_f32", 256, z, mfac32, add, w_out,
                      need_lik, lse, lik_out=lik_out)


def estep_big_available(device: torch.device, dtype: str, d: int) -> bool:
    """Big-D MFMA logw path gate (D <= 142, bf16 or exact-f32 MFMA; the
    factor-emission LDS working set crosses 160 KB at D = 143). The
    engine prefers the fused kernel for D <= 31."""
    return device.type == "cuda" and dtype in ("bf16", "fp32") and 1 <= d <= 142


def mfac_shape(d: int) -> tuple[int, int, int]:
    """Factor tensor shape [2, RT*32, KCT*16] for estep MFMA kernels."""
    rows = ((d + 31) // 32) * 32
    kc = (d + 1 + 15) // 16
    kct = 2 if kc <= 2 else 3 if kc == 3 else 5 if kc <= 5 else 9
    return 2, rows, kct * 16


def estep_logw_big(z: torch.Tensor, mfac: torch.Tensor, add: torch.Tensor,
                   out: torch.Tensor) -> torch.Tensor:
    """Big-D MFMA log-weights into out [K, N] (CUDA, bf16, D > 31)."""
    hip_ext().estep_logw_big(z, mfac, add, out)
    return out


def estep_logw_big_f32(z: torch.Tensor, mfac32: torch.Tensor,
                       add: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """Exact-f32 big-D MFMA log-weights into out [K, N] (CUDA, D > 31)."""
    hip_ext().estep_logw_big_f32(z, mfac32, add, out)
    return out


def emit_factor_tables(r: torch.Tensor, rinv: torch.Tensor,
                       means: torch.Tensor, diag_only: bool,
                       mfac: torch.Tensor | None,
                       mfac32: torch.Tensor | None) -> None:
    """Emit the MFMA E-step factor tables (CUDA) from the covariance R
    (Cholesky of R, stable for any PD covariance) into `mfac` (bf16) and
    `mfac32`, without touching the constants: after an MDL merge, a
    checkpoint resume or a model load the constant comes from the host path
    and must feed the E-step unchanged.

    DIAG parity through a merge: the reference's diag E-step reads
    diag(inv(R_merged_full)) — the host merge computed the FULL-matrix
    inverse and quirk #8 carries it into the next E-step — which is NOT
    inv(diag(R_full)). So with diag_only the factors come from the diagonal
    matrix with exactly that inverse; for an already-diagonal R (seed,
    resume, every iteration after the first M-step) this is identical to R.
    """
    if mfac is None and mfac32 is None:
        return
    r_src = r
    if diag_only:
        d_inv = rinv.diagonal(dim1=-2, dim2=-1)
        r_src = torch.diag_embed(1.0 / d_inv)
    empty_b = torch.empty(0, dtype=torch.bfloat16, device=r.device)
    empty_f = torch.empty(0, dtype=torch.float32, device=r.device)
    hip_ext().emit_factors(
        r_src.contiguous(), means.contiguous(),
        mfac if mfac is not None else empty_b,
        mfac32 if mfac32 is not None else empty_f,
        empty_f, empty_f, empty_f,  # constants NOT recomputed (quirk #8)
    )


def logw_offsets(constant: torch.Tensor, pi: torch.Tensor) -> torch.Tensor:
    """add [K] = constant + ln pi, the per-cluster offset of the factor-path
    E-step kernels; `constant` is taken verbatim (quirk #8)."""
    return constant + torch.log(pi)


def model_factor_tables(means: torch.Tensor, r: torch.Tensor,
                        rinv: torch.Tensor, constant: torch.Tensor,
                        pi: torch.Tensor, diag_only: bool, dtype: str
                        ) -> tuple[torch.Tensor, torch.Tensor]:
    """(factor table, add) of a parameter set on a CUDA device, D <= 142:
    what EmEngine._refresh_mfac and _sync_add leave in the engine's buffers.
    The table is bf16 [K, 2, rows, cols] for dtype "bf16" and fp32
    [K, rows, cols] for "fp32" (rows, cols from mfac_shape)."""
    k, d = means.shape
    shape = mfac_shape(d)
    mfac = torch.empty(k, *shape, dtype=torch.bfloat16, device=means.device)
    mfac32 = (torch.empty(k, *shape[1:], dtype=torch.float32,
                          device=means.device)
              if dtype == "fp32" else None)
    emit_factor_tables(r, rinv, means, diag_only, mfac, mfac32)
    return (mfac32 if mfac32 is not None else mfac,
            logw_offsets(constant, pi))


def estep_classify_available(device: torch.device, d: int) -> bool:
    """Classify kernel gate: D <= 31, any K."""
    return device.type == "cuda" and 1 <= d <= 31


def estep_classify(x_event_major: torch.Tensor, center: torch.Tensor,
                   fac: torch.Tensor, add: torch.Tensor, dtype: str
                   ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Score events against a mixture (CUDA, D <= 31): x fp32 [N, D] in the
    file's own event-major layout, center [D], the factor table and add of
    model_factor_tables. Returns (label int32 [N] = first argmax of the
    log-weights, lse fp32 [N] = ln p(x), pmax fp32 [N] = posterior of the
    assigned cluster). One kernel; no [K, N] array is written."""
    n = x_event_major.shape[0]
    dev = x_event_major.device
    label = torch.empty(n, dtype=torch.int32, device=dev)
    lse = torch.empty(n, dtype=torch.float32, device=dev)
    pmax = torch.empty(n, dtype=torch.float32, device=dev)
    entry = (hip_ext().estep_classify_f32 if dtype == "fp32"
             else hip_ext().estep_classify)
    entry(x_event_major, center, fac, add, label, lse, pmax)
    return label, lse, pmax


# stages of a seeding round (bits of seed_kmeanspp_rounds' `stages`)
SEED_SAMPLE, SEED_EVALUATE, SEED_CHOOSE, SEED_COMMIT = 1, 2, 4, 8
SEED_ALL = SEED_SAMPLE | SEED_EVALUATE | SEED_CHOOSE | SEED_COMMIT


def seed_kmeanspp_workspace(x_event_major: torch.Tensor, k: int,
                            seed_rng: int,
                            weights: torch.Tensor | None = None) -> dict:
    """Device buffers of one k-means++ seeding of x (CUDA fp32 [N, D],
    event-major): the uniforms (drawn on the host, uploaded once), the work
    buffers and the per-round record, keyed by the argument names of the
    extension's seed_kmeanspp_rounds. Nothing is launched."""
    ext = hip_ext()
    dev = x_event_major.device
    n = int(x_event_major.shape[0])
    nl = seed_mod.kmeanspp_num_candidates(k)
    nblk = int(ext.seed_kmeanspp_blocks(n))
    f32 = dict(dtype=torch.float32, device=dev)
    f64 = dict(dtype=torch.float64, device=dev)
    return {
        "x": x_event_major,
        "s": (weights.to(dev, torch.float32).reshape(-1).contiguous()
              if weights is not None else torch.empty(0, **f32)),
        "u": torch.from_numpy(seed_mod.kmeanspp_uniforms(k, seed_rng)).to(dev),
        "m": torch.empty(n, **f32),
        "scratch": torch.empty((nl, n), **f32),
        "pot_part": torch.empty((nblk, 8), **f64),
        "sm_part": torch.empty(nblk, **f64),
        "s_part": torch.empty(nblk, **f64),
        "cand": torch.zeros((k, 8), dtype=torch.int64, device=dev),
        "winner": torch.zeros(k, dtype=torch.int32, device=dev),
        "index": torch.zeros(k, dtype=torch.int64, device=dev),
        "pots": torch.zeros((k, 8), **f64),
    }


def seed_kmeanspp_rounds(ws: dict, t0: int, t1: int,
                         stages: int = SEED_ALL) -> None:
    """Enqueue the selected stages of seeding rounds [t0, t1) on the buffers
    of seed_kmeanspp_workspace; no host synchronisation."""
    hip_ext().seed_kmeanspp_rounds(
        ws["x"], ws["s"], ws["u"], ws["m"], ws["scratch"], ws["pot_part"],
        ws["sm_part"], ws["s_part"], ws["cand"], ws["winner"], ws["index"],
        ws["pots"], int(t0), int(t1), int(stages))


def seed_kmeanspp_trace(ws: dict) -> dict:
    """The per-round record of a finished seeding in the layout of
    models.seed.seed_means_kmeanspp's trace (host tensors)."""
    k = int(ws["u"].shape[0])
    nl = int(ws["scratch"].shape[0])
    cands = ws["cand"][:, :nl].cpu()
    pots = ws["pots"][:, :nl].cpu()
    if nl > 1:  # round 0 has a single candidate
        cands[0, 1:] = -1
        pots[0, 1:] = float("nan")
    return {"candidates": cands, "winner": ws["winner"].cpu().long(),
            "potentials": pots}


def seed_kmeanspp(data, k: int, seed_rng: int, weights=None,
                  device: torch.device | str = "cpu"
                  ) -> tuple[torch.Tensor, torch.Tensor, dict]:
    """Greedy k-means++ seeds of the full dataset ``data`` [N, D] (contract:
    models.seed.seed_means_kmeanspp). Returns host tensors (means fp32
    [K, D], indices int64 [K], trace).

    CPU: the float64 host implementation. CUDA: the data is uploaded once to
    ``device``, the gfx950 kernels run all K rounds without a host
    synchronisation, and the indices and the trace come back in one copy at
    the end; the upload is freed on return. The GPU draws from fp32
    distances, so a draw that lands within rounding of an interval boundary
    may differ from the CPU's; either is a valid k-means++ seeding."""
    device = torch.device(device)
    if device.type != "cuda":
        return seed_mod.seed_means_kmeanspp(data, k, seed_rng, weights)
    hip_ext()  # loud failure when unbuilt: no eager fallback
    host = torch.as_tensor(data).to(torch.float32).contiguous()
    w = None if weights is None else torch.as_tensor(weights)
    ws = seed_kmeanspp_workspace(host.to(device), k, seed_rng, w)
    seed_kmeanspp_rounds(ws, 0, k)
    idx = ws["index"].cpu()
    trace = seed_kmeanspp_trace(ws)
    return host[idx], idx, trace


def split_bf16_planes(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """Persistent hi/lo bf16 split of fp32 data (x = hi + lo + O(2^-18 x))."""
    hi = x.to(torch.bfloat16)
    lo = (x - hi.to(torch.float32)).to(torch.bfloat16)
    return hi.contiguous(), lo.contiguous()


# default chunk count of the pair-column bf16x3 moments kernel: one block per
# 64 clusters and chunk, so 256 chunks = one block per CU at K <= 64 (sweep
# 128..2048 in profiles/LADDER.md R33: 256 fastest, 512 +10%, 128 +70%)
PAIR_NCHUNK = 256


def mstep_moments(x: torch.Tensor, w: torch.Tensor,
                  nchunk: int | None = None,
                  precision: str = "fp32",
                  x_split: tuple[torch.Tensor, torch.Tensor] | None = None,
                  lse: torch.Tensor | None = None) -> torch.Tensor:
    """Fused augmented sufficient statistics, packed lower triangle of
    T_c = sum_e w_ce [x;1][x;1]^T per cluster: [K, Dp*(Dp+1)/2] with layout
    [S_tri (D rows) | mean numerators (row D) | N (corner)] — the single
    all-reduce payload of the M-step.

    CUDA fast path (D <= 31): one f32-MFMA kernel (exact fp32 fmaf chain).
    Otherwise composed from the covariance kernel + rocBLAS/torch ops.
    """
    k, n = w.shape
    d = x.shape[0]
    dp = d + 1
    pp = dp * (dp + 1) // 2
    p = d * (d + 1) // 2
    if x.is_cuda and d <= 31:
        tiles = (n + 127) // 128
        # bf16x3 runs the pair-column GEMM kernel; GMM_MOMENTS_B16=legacy
        # selects the per-cluster A = w.z kernel (same-build A/B)
        pair = (precision == "bf16x3"
                and os.environ.get("GMM_MOMENTS_B16", "pair") != "legacy")
        if nchunk is None:
            # enough chunk-parallelism to fill 8 XCDs x 32 CUs, capped so
            # the partial buffer stays <= 64 MB (measured sweeps: bf16x3
            # fastest at ~256 chunks, fp32 at ~512, K=64 N=1M)
            target = 256 if precision == "bf16x3" else 512
            if pair:
                # one block per 64 clusters and chunk (not one per 8)
                target = PAIR_NCHUNK
            nchunk = max(1, min(target, (64 << 20) // (4 * k * pp)))
        nchunk = int(min(nchunk, tiles))
        partials = torch.empty((nchunk, k, pp), dtype=torch.float32,
                               device=x.device)
        lse_t = (lse if lse is not None
                 else torch.empty(0, dtype=torch.float32, device=x.device))
        if precision == "bf16x3":
            if x_split is None:
                x_split = split_bf16_planes(x)
            kern = (hip_ext().mstep_moments_pair_b16 if pair
                    else hip_ext().mstep_moments_b16)
            kern(x_split[0], x_split[1], w, lse_t, partials)
        else:
            hip_ext().mstep_moments(x, w, lse_t, partials)
        out = torch.empty((k, pp), dtype=torch.float32, device=x.device)
        hip_ext().reduce_chunks(partials, out)
        return out
    if x.is_cuda and precision == "bf16x3" and d <= 159:
        tiles = (n + 63) // 64  # MBB_BK
        if nchunk is None and os.environ.get("GMM_MOMENTS_NCHUNK"):
            nchunk = int(os.environ["GMM_MOMENTS_NCHUNK"])
        if nchunk is None:
            # big-D packed rows are large (Pp ~ 8k at D=128): a small byte
            # cap starves chunk-parallelism (7 chunks = 448 blocks at
            # K=256). The partial buffer is cheap in 288 GB and its sum is
            # ~90 us/GB; keep >= 8 XCDs x 32 CUs of blocks instead.
            nchunk = max(1, min(256, (512 << 20) // (4 * k * pp)))
        nchunk = int(min(nchunk, tiles))
        partials = torch.empty((nchunk, k, pp), dtype=torch.float32,
                               device=x.device)
        lse_t = (lse if lse is not None
                 else torch.empty(0, dtype=torch.float32, device=x.device))
        hip_ext().mstep_moments_big(x, w, lse_t, partials)
        out = torch.empty((k, pp), dtype=torch.float32, device=x.device)
        hip_ext().reduce_chunks(partials, out)
        return out
    packed = torch.empty((k, pp), dtype=torch.float32, device=x.device)
    if x.is_cuda:
        if lse is not None:
            # fallback path mixes rocBLAS GEMMs that need materialized
            # posteriors. MUST be non-destructive: w holds the E-step's
            # logw, and an in-place normalize would corrupt the first
            # graph replay (the eager capture-warmup iteration would
            # leave posteriors where the replayed ops expect logw).
            w = torch.exp(w - lse.unsqueeze(0))
        s = mstep_covariance_s(x, w)        # custom kernel, [K, D, D]
        mean_num = w @ x.T                  # rocBLAS
        n_c = w.sum(dim=1)
    else:
        n_c, mean_num, s = cpu.mstep_sufficient_stats(x.float(), w)
    tri = torch.tril_indices(d, d, device=x.device)
    packed[:, :p] = s[:, tri[0], tri[1]]
    packed[:, p:p + d] = mean_num
    packed[:, -1] = n_c
    return packed


def moments_views(packed: torch.Tensor, d: int
                  ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(N [K], mean numerators [K,D], S [K,D,D]) from the packed layout."""
    k = packed.shape[0]
    p = d * (d + 1) // 2
    n_c = packed[:, -1]
    mean_num = packed[:, p:p + d]
    idx = _tri_unpack_index(d, packed.device)
    s = packed[:, :p][:, idx].view(k, d, d)
    return n_c, mean_num, s


finalize_means = cpu.finalize_means
finalize_covariance = cpu.finalize_covariance
compute_pi = cpu.compute_pi
