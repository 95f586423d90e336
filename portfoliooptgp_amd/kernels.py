"""Covariance functions with the gpflow.kernels 2.9.1 constructor surface.

The objects only hold parameters and structure; they compile to a ``gpx_kernel_spec``
(include/gpx.h) that the HIP kernels evaluate on the device. Classes and defaults follow the
kernels the reference instantiates at GPR/main.py:105-114 (SE, Matern12, RationalQuadratic,
Exponential, SE+Matern12, Exponential+Periodic(SE)+Linear, Exponential+Periodic(SE),
SE*Matern12) and Multi-Input_GPR/main.py:118-135 (Exponential(active_dims) *
Exponential(active_dims)). Parameter order = GPflow's tf.Module flattening order
(sorted attribute names; Sum/Product kernels in list order).

ARD: the stationary kernels take ``lengthscales`` as a scalar or as a 1-D sequence with one entry
per active dim (``kernel.ard`` is then True, as in GPflow). The vector is one trainable variable;
in the θ row it is flattened where the scalar sits: ``[ℓ_0 … ℓ_{dn−1}, σ²]``, RationalQuadratic
``[α, ℓ_0 … ℓ_{dn−1}, σ²]``. Served by ``models.GPR`` (the dense route); see DESIGN.md §3h.

Coregion: ``Coregion(output_dim=P, rank=R, active_dims=[index column])`` is gpflow.kernels.Coregion,
the intrinsic coregionalisation model: ``K[i, j] = B[a_i, a_j]`` with ``B = W Wᵀ + diag(κ)`` and a the
integer output index in the one active column. ``W`` ([P, R], identity transform, signed) takes P·R θ
columns in row-major order, ``kappa`` ([P], positive) the P behind them. Alone or as one factor of a
flat ``Product``; served by ``models.GPR`` (the dense route); see DESIGN.md §3k.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native as N
from .parameter import ArrayParameter, Parameter, VectorParameter


def _normalise_active_dims(active_dims) -> Optional[Tuple[int, int]]:
    """Return (start, count) for a contiguous selection, None for 'all dims'."""
    if active_dims is None:
        return None
    if isinstance(active_dims, slice):
        if active_dims.step not in (None, 1):
            raise NotImplementedError("active_dims slices with a step are not supported")
        start = 0 if active_dims.start is None else int(active_dims.start)
        if active_dims.stop is None:
            return (start, -1)  # up to D, resolved at compile time
        return (start, int(active_dims.stop) - start)
    dims = [int(d) for d in list(active_dims)]
    if not dims or dims != list(range(dims[0], dims[0] + len(dims))):
        raise NotImplementedError("only contiguous active_dims are supported")
    return (dims[0], len(dims))


class Kernel:
    """Base class. ``parameters`` is the GPflow-ordered tuple of Parameter objects."""

    def __init__(self, active_dims=None, name: Optional[str] = None):
        self.active_dims = active_dims
        self._dims = _normalise_active_dims(active_dims)
        self.name = name or type(self).__name__.lower()

    # --- structure --------------------------------------------------------------------
    @property
    def parameters(self) -> Tuple[Parameter, ...]:
        raise NotImplementedError

    @property
    def trainable_parameters(self) -> Tuple[Parameter, ...]:
        return tuple(p for p in self.parameters if p.trainable)

    @property
    def trainable_variables(self):
        return tuple(p.unconstrained_variable for p in self.trainable_parameters)

    def _param_paths(self, prefix: str) -> List[Tuple[str, Parameter]]:
        raise NotImplementedError

    def _theta_slots(self) -> List[Tuple[object, Optional[int]]]:
        """The kernel's θ columns in order: (parameter, entry) per column — entry None for a
        scalar parameter, the index into its vector for an ARD lengthscale or a Coregion κ, the
        row-major index into a Coregion W."""
        out: List[Tuple[object, Optional[int]]] = []
        for p in self.parameters:
            if isinstance(p, VectorParameter):
                out.extend((p, e) for e in range(p.size))
            elif isinstance(p, ArrayParameter):
                out.extend((p, e) for e in range(int(np.prod(p.shape))))
            else:
                out.append((p, None))
        return out

    def theta_values(self) -> List[float]:
        """Constrained values of the θ columns (``_theta_slots`` order)."""
        out: List[float] = []
        for p in self.parameters:
            if isinstance(p, (VectorParameter, ArrayParameter)):
                out.extend(p.value.reshape(-1).tolist())
            else:
                out.append(p.value)
        return out

    def _terms(self) -> List["Kernel"]:
        return [self]

    def _combine(self) -> int:
        return N.GPX_SUM

    # --- algebra (gpflow.kernels.Kernel.__add__/__mul__) -------------------------------
    def __add__(self, other: "Kernel") -> "Sum":
        return Sum([self, other])

    def __mul__(self, other: "Kernel") -> "Product":
        return Product([self, other])

    def __repr__(self) -> str:
        def show(p):
            if isinstance(p, (VectorParameter, ArrayParameter)):
                return "[" + ", ".join(f"{v:.6g}" for v in p.value.reshape(-1).tolist()) + "]"
            return f"{p.value:.6g}"
        return f"<{type(self).__name__} " + ", ".join(
            f"{n}={show(p)}" for n, p in self._param_paths("")) + ">"


class _Term(Kernel):
    kind = 0
    ard = False

    def _active(self, D: int) -> Tuple[int, int]:
        if self._dims is None:
            start, count = 0, D
        else:
            start, count = self._dims
            if count < 0:
                count = D - start
        if start < 0 or count < 1 or start + count > D:
            raise ValueError(f"{self.name}: active_dims {self.active_dims} out of range for D={D}")
        return start, count

    def _spec_term(self, D: int, offset: int) -> N.GpxTerm:
        start, count = self._active(D)
        return N.GpxTerm(self.kind, start, count, offset)


class Stationary(_Term):
    """Stationary kernels of r = |x − x'| / ℓ: a scalar lengthscale (isotropic) or a vector with
    one entry per active dim (ARD); params ordered [lengthscales, variance]."""

    def __init__(self, variance=1.0, lengthscales=1.0, active_dims=None, name=None):
        super().__init__(active_dims=active_dims, name=name)
        self.variance = Parameter(variance, name="variance")
        if np.ndim(lengthscales) == 0:
            self.lengthscales = Parameter(lengthscales, name="lengthscales")
        else:
            if np.ndim(lengthscales) != 1:
                raise ValueError(f"{self.name}: ARD lengthscales must be a 1-D sequence, one entry per active dim")
            self.lengthscales = VectorParameter(lengthscales, name="lengthscales")
            # (an open-ended slice or 'all dims' is checked against D at compile_spec)
            if self._dims is not None and self._dims[1] >= 0 and self._dims[1] != self.lengthscales.size:
                raise ValueError(f"{self.name}: {self.lengthscales.size} lengthscales for "
                                 f"{self._dims[1]} active dims")

    @property
    def ard(self) -> bool:
        """True when ``lengthscales`` is a vector (gpflow.kernels.Stationary.ard)."""
        return isinstance(self.lengthscales, VectorParameter)

    def _spec_term(self, D: int, offset: int) -> N.GpxTerm:
        start, count = self._active(D)
        if not self.ard:
            return N.GpxTerm(self.kind, start, count, offset)
        if self.lengthscales.size != count:
            raise ValueError(f"{self.name}: {self.lengthscales.size} lengthscales for {count} active dims")
        # ARD over one active dim is the plain term (the same θ layout: it keeps the banded routes)
        return N.GpxTerm(self.kind | (N.GPX_TERM_ARD if count > 1 else 0), start, count, offset)

    @property
    def parameters(self):
        return (self.lengthscales, self.variance)

    def _param_paths(self, prefix):
        return [(prefix + "lengthscales", self.lengthscales), (prefix + "variance", self.variance)]


class SquaredExponential(Stationary):
    """σ² exp(−r²/2)."""
    kind = N.GPX_SE


RBF = SquaredExponential


class Matern12(Stationary):
    """σ² exp(−r)."""
    kind = N.GPX_MATERN12


class Matern32(Stationary):
    """σ² (1 + √3 r) exp(−√3 r)."""
    kind = N.GPX_MATERN32


class Matern52(Stationary):
    """σ² (1 + √5 r + 5r²/3) exp(−√5 r)."""
    kind = N.GPX_MATERN52


class Exponential(Stationary):
    """gpflow.kernels.Exponential: σ² exp(−r/2)."""
    kind = N.GPX_EXPONENTIAL


class RationalQuadratic(Stationary):
    """σ² (1 + r²/(2α))^(−α); params ordered [alpha, lengthscales, variance]."""
    kind = N.GPX_RQ

    def __init__(self, variance=1.0, lengthscales=1.0, alpha=1.0, active_dims=None, name=None):
        super().__init__(variance, lengthscales, active_dims, name)
        self.alpha = Parameter(alpha, name="alpha")

    @property
    def parameters(self):
        return (self.alpha, self.lengthscales, self.variance)

    def _param_paths(self, prefix):
        return [(prefix + "alpha", self.alpha)] + super()._param_paths(prefix)


class Linear(_Term):
    """σ² x·x' over the active dims; params [variance]."""
    kind = N.GPX_LINEAR

    def __init__(self, variance=1.0, active_dims=None, name=None):
        super().__init__(active_dims=active_dims, name=name)
        if np.ndim(variance) != 0:
            raise NotImplementedError("Linear takes a scalar variance (a vector, ARD, variance is not provided)")
        self.variance = Parameter(variance, name="variance")

    @property
    def parameters(self):
        return (self.variance,)

    def _param_paths(self, prefix):
        return [(prefix + "variance", self.variance)]


class Periodic(_Term):
    """gpflow.kernels.Periodic(base_kernel=SquaredExponential(), period=1.0):
    σ² exp(−½ Σ_d (sin(π(x_d−x'_d)/p)/ℓ)²); params [base.lengthscales, base.variance, period]."""
    kind = N.GPX_PERIODIC_SE

    def __init__(self, base_kernel: Optional[SquaredExponential] = None, period=1.0, name=None):
        base_kernel = base_kernel if base_kernel is not None else SquaredExponential()
        if type(base_kernel) is not SquaredExponential:
            raise NotImplementedError("Periodic is implemented for a SquaredExponential base kernel")
        if base_kernel.ard:
            raise NotImplementedError("Periodic over an ARD base kernel is not provided (scalar lengthscales only)")
        super().__init__(active_dims=base_kernel.active_dims, name=name)
        self.base_kernel = base_kernel
        self.period = Parameter(period, name="period")

    @property
    def parameters(self):
        return (self.base_kernel.lengthscales, self.base_kernel.variance, self.period)

    def _param_paths(self, prefix):
        return self.base_kernel._param_paths(prefix + "base_kernel.") + [(prefix + "period", self.period)]


class Coregion(_Term):
    """gpflow.kernels.Coregion(output_dim, rank, active_dims=[index column]): K[i, j] = B[a_i, a_j],
    B = W Wᵀ + diag(κ), a the integer output index held by the one active column. Params ordered
    [W, kappa] (tf.Module: attribute names in ASCII order); W [P, R] has the identity transform
    (default 0.1·ones, any sign), kappa [P] is positive (default ones)."""
    kind = N.GPX_COREGION

    def __init__(self, output_dim: int, rank: int, *, active_dims=None, name=None):
        super().__init__(active_dims=active_dims, name=name)
        P, R = int(output_dim), int(rank)
        if P < 1 or R < 1:
            raise ValueError(f"{self.name}: output_dim and rank must be >= 1")
        if self._dims is not None and self._dims[1] != 1:
            raise ValueError(f"{self.name}: Coregion acts on exactly one input column (the output index); "
                             f"active_dims {active_dims} selects {self._dims[1] if self._dims[1] >= 0 else 'several'}")
        self.output_dim, self.rank = P, R
        self.W = ArrayParameter(0.1 * np.ones((P, R)), name="W")
        self.W.summary_full = True  # (print_summary shows the whole matrix: at most 14 entries)
        self.kappa = VectorParameter(np.ones(P), name="kappa")

    def output_covariance(self) -> np.ndarray:
        """B = W Wᵀ + diag(κ), [P, P]."""
        W = self.W.value
        return W @ W.T + np.diag(self.kappa.value)

    def output_variance(self) -> np.ndarray:
        """diag(B) = Σ_r W_pr² + κ_p, [P]."""
        return np.sum(np.square(self.W.value), axis=1) + self.kappa.value

    def _spec_term(self, D: int, offset: int) -> N.GpxTerm:
        start, count = self._active(D)
        if count != 1:
            raise ValueError(f"{self.name}: Coregion acts on exactly one input column (the output index); "
                             f"active_dims {self.active_dims} selects {count} of D={D}")
        return N.GpxTerm(self.kind, start, 1, offset)

    def check_index(self, X, what: str = "X") -> None:
        """Every value of the index column must be an exact integer in [0, output_dim)."""
        X = np.asarray(X, dtype=np.float64)
        start, _ = self._active(X.shape[1])
        col = X[:, start]
        if not (np.all(np.isfinite(col)) and np.all(col == np.floor(col)) and np.all(col >= 0)
                and np.all(col < self.output_dim)):
            raise ValueError(f"{self.name}: column {start} of {what} must hold integer output indices in "
                             f"[0, {self.output_dim})")

    @property
    def parameters(self):
        return (self.W, self.kappa)

    def _param_paths(self, prefix):
        return [(prefix + "W", self.W), (prefix + "kappa", self.kappa)]


class Combination(Kernel):
    """Sum / Product; nested combinations of the same class are flattened like GPflow's
    Combination._set_kernels."""

    combine = N.GPX_SUM

    def __init__(self, kernels: Sequence[Kernel], name=None):
        super().__init__(name=name)
        flat: List[Kernel] = []
        for k in kernels:
            if not isinstance(k, Kernel):
                raise TypeError("can only combine Kernel instances")
            if isinstance(k, type(self)):
                flat.extend(k.kernels)
            else:
                flat.append(k)
        self.kernels = flat

    @property
    def parameters(self):
        return tuple(p for k in self.kernels for p in k.parameters)

    def _param_paths(self, prefix):
        out = []
        for i, k in enumerate(self.kernels):
            out.extend(k._param_paths(f"{prefix}kernels[{i}]."))
        return out

    def _terms(self):
        terms = []
        for k in self.kernels:
            if isinstance(k, Combination):
                raise NotImplementedError(
                    "nested Sum/Product mixes are not supported by the device spec; "
                    "use a flat Sum or a flat Product")
            terms.append(k)
        return terms

    def _combine(self):
        return self.combine


class Sum(Combination):
    combine = N.GPX_SUM


class Product(Combination):
    combine = N.GPX_PRODUCT


def compile_spec(kernel: Kernel, D: int) -> N.GpxKernelSpec:
    """Kernel object -> gpx_kernel_spec (parameter offsets in GPflow order)."""
    terms = kernel._terms()
    if len(terms) > N.GPX_MAX_TERMS:
        raise NotImplementedError(f"at most {N.GPX_MAX_TERMS} kernel terms are supported")
    spec = N.GpxKernelSpec()
    spec.n_terms = len(terms)
    spec.combine = kernel._combine()
    coreg = [k for k in terms if isinstance(k, Coregion)]
    if coreg:
        # one Coregion term, alone or as a factor of a flat product (include/gpx.h)
        if len(coreg) > 1:
            raise NotImplementedError("a kernel may hold one Coregion term (two Coregion factors are not provided)")
        if len(terms) > 1 and kernel._combine() != N.GPX_PRODUCT:
            raise NotImplementedError("Coregion inside a Sum is not provided: use it alone or as one factor of "
                                      "a flat Product (k_t * Coregion)")
        spec.reserved = coreg[0].output_dim | (coreg[0].rank << 8)
    off = 0
    for t, term in enumerate(terms):
        spec.terms[t] = term._spec_term(D, off)
        off += len(term._theta_slots())
    if off + 1 > N.GPX_THETA_STRIDE and not coreg:  # (a Coregion kernel: its own row rule below)
        raise NotImplementedError(
            f"too many kernel parameters: the θ row holds {N.GPX_THETA_STRIDE} values, this kernel needs "
            f"{off} + the noise variance")
    if any(spec.terms[t].kind & N.GPX_TERM_ARD for t in range(len(terms))):
        # an ARD spec leaves the row's last column free (include/gpx.h); the ARD kernels stage every
        # stationary term's scaled inputs in GPX_MAX_DIM values per row (plus D for Linear / Periodic)
        if off + 1 > N.GPX_THETA_STRIDE - 1:
            raise NotImplementedError(
                f"too many kernel parameters for an ARD kernel: the θ row holds {N.GPX_THETA_STRIDE} values, "
                f"of which an ARD kernel and the noise variance may use {N.GPX_THETA_STRIDE - 1}; this one "
                f"needs {off + 1}")
        staged = sum(spec.terms[t].dim_count for t, k in enumerate(terms) if isinstance(k, Stationary))
        if staged + (D if any(not isinstance(k, Stationary) for k in terms) else 0) > N.GPX_MAX_DIM:
            raise NotImplementedError(
                f"an ARD kernel's stationary terms may cover at most {N.GPX_MAX_DIM} input columns in total")
    if coreg:
        # the same row rule as an ARD spec; the Coregion kernels stage the partners' rows as the ARD
        # kernels do, plus the rows' output indices in one more column
        if off + 1 > N.GPX_THETA_STRIDE - 1:
            raise NotImplementedError(
                f"too many kernel parameters for a Coregion kernel: the θ row holds GPX_THETA_STRIDE = "
                f"{N.GPX_THETA_STRIDE} values, of which a Coregion kernel and the noise variance may use "
                f"{N.GPX_THETA_STRIDE - 1}; this one needs {off + 1} (P·R + P for W and kappa)")
        partners = [(t, k) for t, k in enumerate(terms) if not isinstance(k, Coregion)]
        staged = sum(spec.terms[t].dim_count for t, k in partners if isinstance(k, Stationary))
        if staged + (D if any(not isinstance(k, Stationary) for _, k in partners) else 0) + 1 > N.GPX_MAX_DIM:
            raise NotImplementedError(
                f"a Coregion kernel's partner terms may cover at most {N.GPX_MAX_DIM - 1} input columns in total")
    spec.n_params = off
    return spec


def has_coregion(kernel: Kernel) -> bool:
    """True when some term of ``kernel`` is a Coregion term."""
    def walk(k):
        if isinstance(k, Combination):
            return any(walk(c) for c in k.kernels)
        return isinstance(k, Coregion)
    return walk(kernel)


def coregion_term(kernel: Kernel) -> Optional["Coregion"]:
    """The Coregion term of a flat kernel, or None."""
    for k in kernel._terms():
        if isinstance(k, Coregion):
            return k
    return None


def signed_slot_mask(spec: N.GpxKernelSpec) -> int:
    """Bit p set: θ column p of ``spec`` is signed — a Coregion term's W entries, which may be any
    finite value. Every other kernel parameter (κ included) and the noise variance must be finite
    and > 0. The twin of signed_slot_mask in csrc/gpx_route.hip (gpx_spec_signed_mask)."""
    m = 0
    P, R = spec.reserved & 0xFF, (spec.reserved >> 8) & 0xFF
    for t in range(min(spec.n_terms, N.GPX_MAX_TERMS)):
        if spec.terms[t].kind != N.GPX_COREGION:
            continue
        for e in range(P * R):
            p = spec.terms[t].param_offset + e
            if 0 <= p < N.GPX_THETA_STRIDE:
                m |= 1 << p
    return m


def has_ard(kernel: Kernel) -> bool:
    """True when some term of ``kernel`` has vector lengthscales."""
    return any(getattr(k, "ard", False) for k in kernel._terms())
