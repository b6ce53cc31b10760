"""NormalDistribution, GaussianProcess and sample (src/distributions.jl) on the device.

The reference draws ``s = N.Σ_ch.L * randn(rng, dim) .+ N.μ`` with ``Σ_ch = cholesky(Σ .+ 1e-7)``
-- the shift is a broadcast add to EVERY element of Σ, not to its diagonal
(src/distributions.jl:20-30).  Here μ and the factor stay on the device: the factor is the
upper triangle of a factor buffer (``gpr_mvn_factor`` / ``gpr_sample_prior``), the draws are
``S = μ 1ᵀ + Uᵀ Z`` for any number of columns at once (``gpr_mvn_sample``), and Z comes either
from the caller or from the library's counter-based generator (``gpr_randn``).
"""
from __future__ import annotations

import ctypes
from typing import Callable, Optional

import numpy as np
import torch

from . import _lib
from ._lib import PosDefException, lib
from .core import (EPS_DEFAULT, AbstractKernel, Context, GPRModel, GPRPredictCache, _dxp,
                   _fit_predict, _hp_arr, _kinds_arr, _ptr, default_context, dim_hp)

SHIFT_DEFAULT = 1e-7  # src/distributions.jl:21


class NormalDistribution:
    """NormalDistribution(μ, Σ) (src/distributions.jl:4-9,20-23): factors ``Σ .+ shift`` (every
    element shifted, as the reference) and keeps μ and the factor on the device.

    ``.mu`` and ``.Sigma`` are host arrays; ``.Sigma_ch`` is the upper factor U (Σ .+ shift =
    UᵀU, the reference's ``Σ_ch.U``) downloaded on demand.  A Σ .+ shift that is not positive
    definite raises ``PosDefException(info)`` like the reference's ``cholesky``."""

    def __init__(self, mu, Sigma, shift: float = SHIFT_DEFAULT, ctx: Optional[Context] = None):
        ctx = ctx or default_context()
        mu = np.asarray(mu, dtype=np.float64).reshape(-1)
        Sigma = np.asarray(Sigma, dtype=np.float64)
        n = mu.shape[0]
        if Sigma.shape != (n, n):
            raise ValueError("μ and Σ size mismatch.")
        self.ctx = ctx
        self.dim = n
        self.shift = float(shift)
        self._dmu = ctx.colmajor(mu)
        self._Sigma = Sigma
        self._sigma_fn = None
        self._fac = ctx.colmajor(Sigma)  # factor buffer: U above, Σ below the diagonal
        info = ctypes.c_int(0)
        rc = lib.gpr_mvn_factor(ctx.h, _ptr(self._fac), n, n, self.shift, ctypes.byref(info))
        if info.value != 0:
            raise PosDefException(info.value)
        ctx.check(rc, "gpr_mvn_factor")

    @classmethod
    def _from_factor(cls, ctx: Context, dmu: torch.Tensor, fac: torch.Tensor, shift: float,
                     sigma_fn: Callable[[], np.ndarray]) -> "NormalDistribution":
        """A distribution whose factor buffer the library already filled (gpr_sample_prior)."""
        self = cls.__new__(cls)
        self.ctx, self.dim, self.shift = ctx, dmu.shape[0], float(shift)
        self._dmu, self._fac, self._Sigma, self._sigma_fn = dmu, fac, None, sigma_fn
        return self

    @property
    def mu(self) -> np.ndarray:
        return self.ctx.host(self._dmu)

    @property
    def Sigma(self) -> np.ndarray:
        if self._Sigma is None:
            self._Sigma = self._sigma_fn()
        return self._Sigma

    @property
    def Sigma_ch(self) -> np.ndarray:
        return np.triu(self.ctx.host(self._fac))

    def _draw(self, dZ: torch.Tensor, ns: int) -> torch.Tensor:
        """S (dim x ns, device) = μ 1ᵀ + Uᵀ Z."""
        ctx, n = self.ctx, self.dim
        S = ctx.empty(ns, n)
        ctx.check(lib.gpr_mvn_sample(ctx.h, _ptr(self._fac), n, n, _ptr(self._dmu), _ptr(dZ), ns, n,
                                     _ptr(S), n), "gpr_mvn_sample")
        return S

    def __repr__(self):
        return f"NormalDistribution(dim={self.dim})"


class GaussianProcess:
    """GaussianProcess(f_μ, kernel) (src/distributions.jl:11-14,36-45)."""

    def __init__(self, f_mu: Callable, kernel: AbstractKernel):
        self.f_mu = f_mu
        self.kernel = kernel

    def __call__(self, x, theta=None, eps: float = EPS_DEFAULT, shift: float = SHIFT_DEFAULT,
                 ctx: Optional[Context] = None, rng=None) -> NormalDistribution:
        """gp(x, θ): μ = f_μ.(eachcol(x)), Σ = kernel(gp.kernel, θ, x), NormalDistribution(μ, Σ)
        (:41-45) -- K assembly, shift and factorisation in one device call, Σ never on the
        host.  gp(x): θ = rand(dim_hp(kernel, d)) (:36-39)."""
        ctx = ctx or default_context()
        x = np.asarray(x, dtype=np.float64)
        if x.ndim == 1:
            x = x[None, :]
        d, n = x.shape
        if theta is None:
            theta = (rng or np.random.default_rng()).random(dim_hp(self.kernel, d))
        theta = np.array(theta, dtype=np.float64)
        if theta.shape[0] != dim_hp(self.kernel, d):
            raise ValueError("Parameter size mismatch.")
        mu = np.array([self.f_mu(x[:, j]) for j in range(n)], dtype=np.float64)
        dx, dmu = ctx.colmajor(x), ctx.colmajor(mu)
        kinds, nk = _kinds_arr(self.kernel)
        _, hpp = _hp_arr(theta)
        fac, z0, s0 = ctx.empty(n, n), ctx.zeros(n), ctx.empty(n)
        info = ctypes.c_int(0)
        rc = lib.gpr_sample_prior(ctx.h, kinds, nk, hpp, d, _ptr(dx), n, _ptr(dmu), float(shift),
                                  float(eps), _ptr(z0), 1, n, _ptr(fac), n, _ptr(s0), n,
                                  ctypes.byref(info))
        if info.value != 0:
            raise PosDefException(info.value)
        ctx.check(rc, "gpr_sample_prior")
        cov = self.kernel

        def sigma():
            from .core import kernel as _kernel
            return _kernel(cov, theta, x, eps=eps, ctx=ctx)

        return NormalDistribution._from_factor(ctx, dmu, fac, shift, sigma)


def _normals(ctx: Context, dim: int, z, n_samples: Optional[int], seed: int):
    """(Z on the device as dim x ns column-major, ns, whether the result is a vector)."""
    if z is not None:
        z = np.asarray(z, dtype=np.float64)
        if z.shape[0] != dim or z.ndim > 2:
            raise ValueError(f"z must have length {dim} or shape ({dim}, n_samples)")
        if n_samples is not None and (z.ndim == 1 or z.shape[1] != n_samples):
            raise ValueError("z and n_samples disagree")
        ns = 1 if z.ndim == 1 else z.shape[1]
        if ns < 1:
            raise ValueError("n_samples must be >= 1")
        return ctx.colmajor(z), ns, z.ndim == 1
    ns = 1 if n_samples is None else int(n_samples)
    if ns < 1:
        raise ValueError("n_samples must be >= 1")
    Z = ctx.empty(ns, dim) if ns > 1 else ctx.empty(dim)
    ctx.check(lib.gpr_randn(ctx.h, int(seed) & (2 ** 64 - 1), 0, _ptr(Z), dim * ns), "gpr_randn")
    return Z, ns, n_samples is None


def sample(N, *args, z=None, n_samples: Optional[int] = None, seed: int = 1, **kw) -> np.ndarray:
    """sample(N) / sample(gp, x) / sample(gp, x, θ) (src/distributions.jl:25-33): Uᵀz + μ.

    With ``z`` (length dim, or dim x n_samples) the draw is exactly the reference's
    ``N.Σ_ch.L * z .+ N.μ`` for that z (one column per sample): this is the form on which
    parity with the reference holds.  Otherwise z comes from the library's counter-based
    generator, ``gpr_randn(seed, 0, ...)``: ``n_samples`` columns (a vector when it is None).
    The default ``seed=1`` mirrors the reference's fixed ``rng=Xoshiro(1)``: repeated calls
    return the same draw.  Julia's Xoshiro / ziggurat stream itself is NOT reproduced, so the
    numbers differ from the reference's unless z is supplied."""
    if isinstance(N, GaussianProcess):
        if not 1 <= len(args) <= 2:
            raise TypeError("sample(gp, x[, θ])")
        N = N(*args, **kw)
    elif args or kw:
        raise TypeError("sample(N; z, n_samples, seed)")
    if not isinstance(N, NormalDistribution):
        raise TypeError(f"cannot sample from {N!r}")
    dZ, ns, vec = _normals(N.ctx, N.dim, z, n_samples, seed)
    s = N.ctx.host(N._draw(dZ, ns))
    return s.reshape(-1) if vec else s.reshape(N.dim, ns)


def sample_posterior(md: GPRModel, xp, n_samples: int = 1, z=None, seed: int = 1,
                     shift: float = SHIFT_DEFAULT, jitter: float = 0.0,
                     eps: float = EPS_DEFAULT) -> np.ndarray:
    """Joint draws from the posterior at the test points xp (one step past the reference):
    (μp, Σp) = predict(md, xp) in full (src/predict.jl:14-25), Lp Lpᵀ = Σp .+ shift + jitter I,
    returns μp 1ᵀ + Lp Z (m x n_samples).  Z is ``z`` (m, or m x n_samples) or
    ``gpr_randn(seed, 0, ...)``.  Everything stays on the device until the return."""
    if md.y.ndim != 1:
        raise ValueError("sample_posterior needs a 1-D y")
    ctx = md.ctx
    pc = GPRPredictCache(md, 0)
    dxp = _dxp(md, xp)
    m = dxp.shape[0]
    mu, Sigma = ctx.empty(m), ctx.empty(m, m)
    _fit_predict(md, dxp, m, pc, mu, Sigma, False, eps)
    if jitter != 0.0:
        with torch.cuda.stream(ctx.stream):
            Sigma.diagonal().add_(float(jitter))
    info = ctypes.c_int(0)
    rc = lib.gpr_mvn_factor(ctx.h, _ptr(Sigma), m, m, float(shift), ctypes.byref(info))
    if info.value != 0:
        raise PosDefException(info.value)
    ctx.check(rc, "gpr_mvn_factor")
    dZ, ns, _ = _normals(ctx, m, z, None if z is not None else n_samples, seed)
    S = ctx.empty(ns, m)
    ctx.check(lib.gpr_mvn_sample(ctx.h, _ptr(Sigma), m, m, _ptr(mu), _ptr(dZ), ns, m, _ptr(S), m),
              "gpr_mvn_sample")
    return ctx.host(S).reshape(m, ns)
