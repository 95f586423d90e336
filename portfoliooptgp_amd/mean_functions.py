"""gpflow.functions / gpflow.mean_functions 2.9.1 surface for ``models.GPR(mean_function=...)``.

Reference call sites: ``Polynomial(2)`` (test_scripts/GPR.py:103, SVGP.py:208,
GPFlow_1_year.py:55), ``Linear()`` (GPFlow.py:189, :298), ``Constant()`` (GPR_Class.py:101).
One output column. Every parameter is trainable, carries the identity transform (GPflow's plain
``Parameter``), and is an ``ArrayParameter`` of GPflow's shape; the device evaluates the mean
(include/gpx.h gpx_batch_set_mean, csrc/gpx_mean.hip), ``__call__`` here is the same arithmetic
in numpy for inspection.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

from . import _native as N
from .parameter import ArrayParameter


class MeanFunction:
    """Base class: ``parameters`` in tf.Module order (attribute names sorted) and the flattened
    coefficient vector in the θ-row order of include/gpx.h (gpx_mean_spec)."""

    kind = N.GPX_MEAN_ZERO
    degree = 0

    @property
    def parameters(self) -> Tuple[ArrayParameter, ...]:
        return tuple(p for _, p in self._param_paths())

    def _param_paths(self):
        return []

    @property
    def n_coef(self) -> int:
        return sum(int(np.prod(p.shape)) for p in self.parameters)

    def coefficients(self) -> np.ndarray:
        ps = self.parameters
        return (np.concatenate([p.unconstrained.reshape(-1) for p in ps]) if ps else np.zeros(0))

    def spec(self) -> "N.GpxMeanSpec":
        return N.GpxMeanSpec(int(self.kind), int(self.degree), int(self.n_coef), 0)

    def _check_dim(self, D: int) -> None:
        pass

    def __call__(self, X) -> np.ndarray:
        X = np.asarray(X, dtype=np.float64)
        return np.zeros((X.shape[0], 1))


class Zero(MeanFunction):
    """m(x) = 0 (the same as ``mean_function=None``)."""


class Constant(MeanFunction):
    """m(x) = c; ``c`` has shape [1], default 0."""

    kind = N.GPX_MEAN_CONSTANT

    def __init__(self, c=None):
        c = np.zeros(1) if c is None else np.asarray(c, dtype=np.float64).reshape(-1)
        if c.shape != (1,):
            raise NotImplementedError("Constant mean: one output column (c must have one entry)")
        self.c = ArrayParameter(c, name="c")

    def _param_paths(self):
        return [("c", self.c)]

    def __call__(self, X):
        X = np.asarray(X, dtype=np.float64)
        return np.full((X.shape[0], 1), self.c.value[0])


class Linear(MeanFunction):
    """m(x) = xᵀA + b; ``A`` has shape [D, 1] and defaults to ones((1, 1)) (so the default serves
    D = 1 only), ``b`` has shape [1] and defaults to 0."""

    kind = N.GPX_MEAN_LINEAR

    def __init__(self, A=None, b=None):
        A = np.ones((1, 1)) if A is None else np.asarray(A, dtype=np.float64)
        if A.ndim == 1:
            A = A[:, None]
        b = np.zeros(1) if b is None else np.asarray(b, dtype=np.float64).reshape(-1)
        if A.ndim != 2 or A.shape[1] != 1 or b.shape != (1,):
            raise NotImplementedError("Linear mean: one output column (A must be [D, 1], b [1])")
        self.A = ArrayParameter(A, name="A")
        self.b = ArrayParameter(b, name="b")

    def _param_paths(self):
        return [("A", self.A), ("b", self.b)]

    def _check_dim(self, D: int) -> None:
        if self.A.shape[0] != D:
            raise ValueError(f"Linear mean: A has {self.A.shape[0]} rows, the inputs have {D} columns")

    def __call__(self, X):
        X = np.asarray(X, dtype=np.float64)
        X = X[:, None] if X.ndim == 1 else X
        A, b = self.A.value, self.b.value
        s = X[:, 0] * A[0, 0]
        for d in range(1, X.shape[1]):
            s = s + X[:, d] * A[d, 0]
        return (s + b[0])[:, None]


class Polynomial(MeanFunction):
    """m(x) = Σ_{k=0..degree} w_k x^k on one input column; ``w`` has shape [degree + 1, 1],
    degree <= 4.

    The default ``w`` here is ZEROS. GPflow's own default could not be checked when this was
    written (it is believed to be drawn at random), so a script that relies on GPflow's initial
    ``w`` must pass it explicitly."""

    kind = N.GPX_MEAN_POLYNOMIAL

    def __init__(self, degree: int, w=None):
        degree = int(degree)
        if not 0 <= degree <= 4:
            raise NotImplementedError("Polynomial mean: degree must be 0..4")
        self.degree = degree
        w = np.zeros((degree + 1, 1)) if w is None else np.asarray(w, dtype=np.float64)
        if w.ndim == 1:
            w = w[:, None]
        if w.shape != (degree + 1, 1):
            raise ValueError(f"Polynomial mean: w must have shape [{degree + 1}, 1]")
        self.w = ArrayParameter(w, name="w")

    def _param_paths(self):
        return [("w", self.w)]

    def _check_dim(self, D: int) -> None:
        if D != 1:
            raise NotImplementedError("Polynomial mean: one input column (D = 1) only")

    def __call__(self, X):
        x = np.asarray(X, dtype=np.float64).reshape(-1)
        w = self.w.value[:, 0]
        p = np.ones_like(x)
        s = np.full_like(x, w[0])
        for k in range(1, self.degree + 1):
            p = p * x
            s = s + w[k] * p
        return s[:, None]
