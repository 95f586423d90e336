"""gpflow.likelihoods.Gaussian: variance σn² with a 1e-6 lower bound
(``Gaussian(variance=1.0, variance_lower_bound=1e-6)``), and gpflow.likelihoods.StudentT
(``StudentT(scale=1.0, df=3.0)``: a positive scale parameter, a fixed df), which models.VGP takes, and
models.SVGP with ``per_point=True``."""
from __future__ import annotations

from .parameter import Parameter

DEFAULT_VARIANCE_LOWER_BOUND = 1e-6


class Gaussian:
    def __init__(self, variance: float = 1.0, variance_lower_bound: float = DEFAULT_VARIANCE_LOWER_BOUND):
        self.variance = Parameter(variance, lower=variance_lower_bound, name="variance")

    @property
    def parameters(self):
        return (self.variance,)

    @property
    def trainable_parameters(self):
        return tuple(p for p in self.parameters if p.trainable)

    @property
    def trainable_variables(self):
        return tuple(p.unconstrained_variable for p in self.trainable_parameters)


class StudentT:
    """Student-t noise: ``scale`` is a positive Parameter (softplus, lower bound 0), ``df`` a plain
    float that is neither a parameter nor trainable. The variance scale²·df/(df − 2) that
    predict_y adds exists for df > 2 only, so df <= 2 is refused here."""

    def __init__(self, scale: float = 1.0, df: float = 3.0):
        df = float(df)
        if not df > 2.0:
            raise ValueError(f"StudentT: df = {df} must be > 2 (the predictive variance is scale² df/(df − 2))")
        self.df = df
        self.scale = Parameter(scale, name="scale")

    @property
    def parameters(self):
        return (self.scale,)

    @property
    def trainable_parameters(self):
        return tuple(p for p in self.parameters if p.trainable)

    @property
    def trainable_variables(self):
        return tuple(p.unconstrained_variable for p in self.trainable_parameters)
