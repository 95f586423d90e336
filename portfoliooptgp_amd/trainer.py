"""Counterparts of the reference's callers of the GP hot path, batched on the device.

* ``ModelTrainer.train_model`` — GPR/model_trainer.py:10-26: for each kernel, GPR with the
  noise fixed at 1e-5, L-BFGS-B maxiter=100, predict_f at the training X, keep the minimum
  training MSE (strict ``<``, first wins). Here the kernel fits run concurrently in one
  lock-step batch; each is the same scipy trajectory it would be alone. Kernel objects are
  shared across calls exactly as in the reference (later fits warm-start from the
  previous optimum and earlier best models alias the mutated kernels).
* ``ModelTrainer.train_svgp_model`` — test_scripts/GPR.py:118-138: the same sweep with one SVGP per
  kernel (Gaussian(1e-4) frozen, inducing points X[:20]), fitted by ``Scipy().minimize_svgp_batch``.
* ``ModelTrainer.train_sgpr_model`` — the same sweep over the SGPR cell of test_scripts/SVGP.py:393-400
  (noise 1.0 and Z trainable, inducing points on a linspace grid), fitted by ``Scipy().minimize_sgpr_batch``.
* ``Predictor`` — GPR/predictor.py:4-51 (predict_single; predict_combined and
  upsample_predictions as host post-processing).
* ``MultiInputTrainer`` — Multi-Input_GPR/models/model_trainer.py:17-72 (train_model,
  train_likelihood with 4 noise restarts picking the lowest opt_logs.fun, train_best_model).
* ``BlendOptimizer`` — GPR/optimizer.py:5-28 (the α/β SLSQP of the timeframe blend).
* ``refit_steps`` — Multi-Input_GPR/main.py:414-456 (run_step_4's refit loop), batched.
"""
from __future__ import annotations

from copy import deepcopy
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import models as M
from .optimizers import Scipy
from .utilities import print_summary, set_trainable


def _np(a) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        return a.detach().cpu().numpy()
    return np.asarray(a)


def mean_squared_error(y_true, y_pred) -> float:
    """sklearn.metrics.mean_squared_error for [N,1] arrays (GPR/model_trainer.py:21)."""
    a, b = _np(y_true).reshape(len(_np(y_true)), -1), _np(y_pred).reshape(len(_np(y_pred)), -1)
    return float(np.average((a - b) ** 2, axis=0).mean())


def stack_assets(series):
    """Stack several assets' series into one data set for a Coregion kernel (GPflow's intrinsic
    coregionalisation layout): ``series`` is ``[(X_p [n_p, D], Y_p [n_p, 1])]``, one pair per asset,
    the counts n_p may differ. Returns ``(X_aug [Σn_p, D+1], Y_aug [Σn_p, 1], index_dim)``: the rows
    asset by asset, the asset's index p appended as column ``index_dim = D``::

        X, Y, idx = stack_assets(series)
        k = kernels.Exponential(active_dims=slice(0, idx)) * kernels.Coregion(len(series), 1, active_dims=[idx])
    """
    series = list(series)
    if not series:
        raise ValueError("stack_assets needs at least one (X, Y) pair")
    xs, ys, D = [], [], None
    for p, (X, Y) in enumerate(series):
        x = np.asarray(_np(X), dtype=np.float64)
        y = np.asarray(_np(Y), dtype=np.float64)
        x = x.reshape(-1, 1) if x.ndim == 1 else x
        y = y.reshape(-1, 1)
        if x.ndim != 2:
            raise ValueError(f"asset {p}: X must be [n, D], got shape {x.shape}")
        if x.shape[0] != y.shape[0]:
            raise ValueError(f"asset {p}: X has {x.shape[0]} rows, Y {y.shape[0]}")
        D = x.shape[1] if D is None else D
        if x.shape[1] != D:
            raise ValueError(f"asset {p}: X has {x.shape[1]} columns, asset 0 has {D}")
        xs.append(np.concatenate([x, np.full((x.shape[0], 1), float(p))], axis=1))
        ys.append(y)
    X_aug = np.concatenate(xs, axis=0)
    return X_aug, np.concatenate(ys, axis=0), X_aug.shape[1] - 1


def unstack_assets(values, X_aug, index_dim: int, n_assets: Optional[int] = None):
    """The inverse of stack_assets for anything with one row per stacked row (a prediction's mean or
    variance, [Σn_p, ...]): the list of per-asset arrays, rows in their stacked order. Works for any
    row order of ``X_aug`` (it selects by the index column); for stack_assets' own asset-by-asset
    order with every asset present the results are views of ``values``."""
    v = _np(values)
    idx = np.asarray(_np(X_aug), dtype=np.float64)[:, index_dim].astype(np.int64)
    if v.shape[0] != idx.shape[0]:
        raise ValueError(f"values has {v.shape[0]} rows, X_aug {idx.shape[0]}")
    P = int(idx.max()) + 1 if n_assets is None else int(n_assets)
    if np.all(np.diff(idx) >= 0):  # sorted by asset: contiguous slices (views)
        bounds = np.searchsorted(idx, np.arange(P + 1))
        return [v[bounds[p]:bounds[p + 1]] for p in range(P)]
    return [v[idx == p] for p in range(P)]


def sample_asset_paths(model, X_aug_new, index_dim: int, num_samples: int, **kw):
    """Joint posterior draws per asset and day from a multi-asset (Coregion) model: ``X_aug_new`` is
    a stack_assets-style Xnew, every asset with the same number H of rows; returns ``[S, H, P]``,
    column p holding asset p's rows in their stacked order (as unstack_assets groups them). The draws
    are ``model.predict_f_samples(X_aug_new, num_samples, **kw)`` regrouped — joint across assets
    and days with the default full_cov=True."""
    idx = np.asarray(_np(X_aug_new), dtype=np.float64)
    if idx.ndim != 2 or not (0 <= index_dim < idx.shape[1]):
        raise ValueError(f"X_aug_new must be [rows, D+1] with the asset index in column {index_dim}")
    idx = idx[:, index_dim].astype(np.int64)
    if idx.size == 0:
        raise ValueError("sample_asset_paths needs at least one row")
    counts = np.bincount(idx)
    if np.any(counts != counts[0]):
        raise ValueError(f"every asset must have the same number of rows, got {counts.tolist()}")
    samples = model.predict_f_samples(X_aug_new, num_samples, **kw)   # [S, rows, 1]
    S = samples.shape[0]
    # asset p's rows in stacked order: a stable sort by the index column
    order = torch.as_tensor(np.argsort(idx, kind="stable"), device=samples.device)
    return samples[:, order, 0].reshape(S, len(counts), int(counts[0])).transpose(1, 2).contiguous()


class ModelTrainer:
    def __init__(self, kernel_combinations: Sequence, device: Optional[int] = None):
        self.kernel_combinations = list(kernel_combinations)
        self.device = device
        self.last_results = []
        self.last_models = []

    def train_model(self, X_tf, Y_tf, maxiter: int = 100):
        models = []
        for kernel in self.kernel_combinations:
            model = M.GPR(data=(X_tf, Y_tf), kernel=kernel, device=self.device)
            model.likelihood.variance.assign(1e-5)
            set_trainable(model.likelihood.variance, False)
            models.append(model)
        self.last_results = Scipy().minimize_batch(models, options=dict(maxiter=maxiter))
        self.last_models = models
        preds = M.predict_f_batch(models, [m.data[0] for m in models])
        best_kernel, best_mse, best_model = None, float("inf"), None
        for kernel, model, (mean, _) in zip(self.kernel_combinations, models, preds):
            mse = mean_squared_error(Y_tf, _np(mean))
            if mse < best_mse:
                best_mse, best_kernel, best_model = mse, kernel, model
        return best_kernel, best_mse, best_model

    def train_svgp_model(self, X_tf, Y_tf, n_inducing: int = 20, maxiter: int = 100):
        """test_scripts/GPR.py:118-138: per kernel an SVGP with Gaussian(1e-4) frozen and the first
        ``n_inducing`` training inputs as inducing points (num_data left None), L-BFGS-B
        maxiter=100, predict_f at the training X, the minimum training MSE wins (strict ``<``,
        first wins). The kernel fits run in one lock-step batch, one device call per round."""
        from .likelihoods import Gaussian
        Z0 = _np(X_tf)
        Z0 = Z0.reshape(Z0.shape[0], -1)[:n_inducing]
        models = []
        for kernel in self.kernel_combinations:
            model = M.SVGP(kernel=kernel, likelihood=Gaussian(variance=1e-4), inducing_variable=Z0.copy(),
                           device=self.device)
            set_trainable(model.likelihood.variance, False)
            models.append(model)
        self.last_results = Scipy().minimize_svgp_batch(models, (X_tf, Y_tf), options=dict(maxiter=maxiter))
        self.last_models = models
        preds = M.predict_f_svgp_batch(models, [X_tf] * len(models))
        best_kernel, best_mse, best_model = None, float("inf"), None
        for kernel, model, (mean, _) in zip(self.kernel_combinations, models, preds):
            mse = mean_squared_error(Y_tf, _np(mean))
            if mse < best_mse:
                best_mse, best_kernel, best_model = mse, kernel, model
        return best_kernel, best_mse, best_model

    def train_sgpr_model(self, X_tf, Y_tf, n_inducing: int = 10, maxiter: int = 100):
        """The sparse sweep beside train_svgp_model, over the reference's SGPR cell
        (test_scripts/SVGP.py:393-400): per kernel an SGPR((X, Y), kernel, inducing_variable=Z0) with
        GPflow's defaults (noise variance 1.0 trainable, Z trainable). For one input column Z0 is the
        cell's layout, ``np.linspace(X.min(), X.max(), n_inducing)[:, None]``; for several, the rows of X
        at the indices ``np.linspace(0, N − 1, n_inducing).round()``. L-BFGS-B maxiter=100, predict_f
        at the training X, the minimum training MSE wins (strict ``<``, first wins). The kernel fits
        run in one lock-step batch, one device call per round."""
        Xn = _np(X_tf)
        Xn = Xn.reshape(Xn.shape[0], -1)
        if Xn.shape[1] == 1:
            Z0 = np.linspace(Xn.min(), Xn.max(), n_inducing)[:, None]
        else:
            Z0 = Xn[np.linspace(0, Xn.shape[0] - 1, n_inducing).round().astype(int)]
        models = [M.SGPR((X_tf, Y_tf), kernel, inducing_variable=np.array(Z0, dtype=np.float64),
                         device=self.device)
                  for kernel in self.kernel_combinations]
        self.last_results = Scipy().minimize_sgpr_batch(models, options=dict(maxiter=maxiter))
        self.last_models = models
        preds = M.predict_f_sgpr_batch(models, [X_tf] * len(models))
        best_kernel, best_mse, best_model = None, float("inf"), None
        for kernel, model, (mean, _) in zip(self.kernel_combinations, models, preds):
            mse = mean_squared_error(Y_tf, _np(mean))
            if mse < best_mse:
                best_mse, best_kernel, best_model = mse, kernel, model
        return best_kernel, best_mse, best_model


class Predictor:
    def predict_single(self, model, X):
        f_mean, f_var = model.predict_f(X, full_cov=False)
        y_mean, y_var = model.predict_y(X)
        return f_mean, f_var, y_mean, y_var

    def predict_combined(self, alpha, beta, daily_model, weekly_model, monthly_model, X_daily, X_weekly,
                         X_monthly):
        fd, vd, yd, yvd = self.predict_single(daily_model, X_daily)
        fw, vw, yw, yvw = self.predict_single(weekly_model, X_weekly)
        fm, vm, ym, yvm = self.predict_single(monthly_model, X_monthly)
        up = self.upsample_predictions
        fw, fm = up(X_daily, X_weekly, fw, "w"), up(X_daily, X_monthly, fm, "m")
        vw, vm = up(X_daily, X_weekly, vw, "w"), up(X_daily, X_monthly, vm, "m")
        yw, ym = up(X_daily, X_weekly, yw, "w"), up(X_daily, X_monthly, ym, "m")
        yvw, yvm = up(X_daily, X_weekly, yvw, "w"), up(X_daily, X_monthly, yvm, "m")
        g = 1.0 - alpha - beta
        return (alpha * fd + beta * fw + g * fm, alpha * vd + beta * vw + g * vm,
                alpha * yd + beta * yw + g * ym, alpha * yvd + beta * yvw + g * yvm)

    def upsample_predictions(self, X_daily_tf, X_tf, predictions, period="d"):
        """pandas Series(pred, index=X).reindex(X_daily).interpolate('linear') — positional
        linear interpolation over the reindexed rows, leading NaNs kept (GPR/predictor.py:35-51)."""
        if period not in ("w", "m"):
            return predictions
        import pandas as pd

        xd = _np(X_daily_tf).reshape(-1)
        xs = _np(X_tf).reshape(-1)
        p = _np(predictions).reshape(-1)
        s = pd.Series(p, index=xs).reindex(xd).interpolate(method="linear")
        return torch.as_tensor(s.values.reshape(-1, 1), dtype=torch.float64)


class BlendOptimizer:
    """Timeframe-blend weights (GPR/optimizer.py:5-28): SLSQP over (α, β) ∈ [0,1]², α + β ≤ 1,
    from (0.33, 0.33), minimising MSE(Y, α·f_d + β·f_w + (1−α−β)·f_m) + λ(|α| + |β|). Host
    code: two variables, evaluated on the blended device predictions."""

    def __init__(self, lambda_: float = 0.01):
        self.lambda_ = float(lambda_)
        self.initial_weights = [0.33, 0.33]
        self.bounds = [(0, 1), (0, 1)]
        self.constraints = {"type": "ineq", "fun": lambda w: 1 - sum(w)}

    def loss_fn(self, weights, Y, f_daily, f_weekly, f_monthly) -> float:
        a, b = weights
        y = _np(Y).reshape(len(_np(Y)), -1)
        blend = a * _np(f_daily) + b * _np(f_weekly) + (1.0 - a - b) * _np(f_monthly)
        return mean_squared_error(y, blend.reshape(y.shape)) + self.lambda_ * (abs(a) + abs(b))

    def optimize_weights(self, Y_tf, f_mean_daily, f_mean_weekly, f_mean_monthly) -> np.ndarray:
        import scipy.optimize
        res = scipy.optimize.minimize(
            lambda w: self.loss_fn(w, Y_tf, f_mean_daily, f_mean_weekly, f_mean_monthly),
            self.initial_weights, method="SLSQP", bounds=self.bounds, constraints=self.constraints)
        return res.x


class MultiInputTrainer:
    """Multi-Input_GPR/models/model_trainer.py (methods callable without an instance, as the
    reference calls them: ``ModelTrainer.train_model(model)``)."""

    def __init__(self, kernel_combinations: Sequence = ()):
        self.kernel_combinations = list(kernel_combinations)

    @staticmethod
    def train_model(model, verbose: bool = True):
        set_trainable(model.likelihood, False)
        Scipy().minimize(model.training_loss, model.trainable_variables)
        if verbose:
            print_summary(model)
        return model

    @staticmethod
    def train_likelihood(X, Y, composite_kernel, starting_variances=(1e-5, 1e-3, 1e-1, 1.0),
                         verbose: bool = True):
        """Four restarts with trainable noise, run as one lock-step batch; lowest final loss wins
        (strict ``<``, first wins, as Multi-Input_GPR/models/model_trainer.py:42-45)."""
        models = []
        for v in starting_variances:
            m = M.GPR((X, Y), kernel=deepcopy(composite_kernel), noise_variance=v)
            set_trainable(m.likelihood, True)
            models.append(m)
        logs = Scipy().minimize_batch(models)
        best_model, best_loss = None, float("inf")
        for m, r in zip(models, logs):
            if r.fun < best_loss:
                best_model, best_loss = m, r.fun
        if verbose:
            print("\nBest model:")
            print_summary(best_model)
            print(f"Best loss: {best_loss}")
        return best_model

    def train_best_model(self, X_tf, Y_tf):
        return ModelTrainer(self.kernel_combinations).train_model(X_tf, Y_tf)


def refit_steps(X_full, Y_full, n_train: int, composite_kernels: Sequence, is_fixed: bool = True,
                mean: float = 0.0, std: float = 1.0, noise_variance: float = 1e-3,
                starting_variances=(1e-5, 1e-3, 1e-1, 1.0)):
    """The iterative refit of Multi-Input_GPR/main.py:414-456 (``run_step_4``), batched.

    For every step i in [n_train, len(Y_full)) and every composite kernel, the reference fits a
    fresh GPR (``deepcopy(kernel)``) on the first i rows — noise fixed at 1e-3 and
    ``ModelTrainer.train_model`` (scipy defaults, no maxiter) when ``is_fixed``, else the
    4-restart ``train_likelihood`` — keeps the model of the LAST kernel of the loop, predicts
    f at the first i+1 rows and keeps the last row, de-normalised (mean·std + μ, var·std²).
    All (step × kernel × restart) fits are independent: here they run as ONE lock-step batch
    (ragged N = n_train … len−1), each the same scipy trajectory it would be alone.

    Returns (f_means, f_vars, actual_returns): lists of [1]-arrays, as run_step_4's first
    three outputs.
    """
    X_full = _np(X_full)
    Y_full = _np(Y_full).reshape(-1, 1)
    steps = list(range(n_train, len(Y_full)))
    kernels = list(composite_kernels)
    if not steps or not kernels:
        return [], [], []
    starts = [noise_variance] if is_fixed else list(starting_variances)
    models, index = [], []
    for si, i in enumerate(steps):
        for ki, k in enumerate(kernels):
            for v in starts:
                m = M.GPR((X_full[:i], Y_full[:i]), kernel=deepcopy(k), noise_variance=v)
                set_trainable(m.likelihood, not is_fixed)
                models.append(m)
                index.append((si, ki))
    logs = Scipy().minimize_batch(models)
    # per step: the last kernel's model (best restart by final loss, strict <, first wins)
    chosen = []
    for si in range(len(steps)):
        best, best_loss = None, float("inf")
        for m, r, (s, k) in zip(models, logs, index):
            if s == si and k == len(kernels) - 1 and r.fun < best_loss:
                best, best_loss = m, r.fun
        chosen.append(best)
    preds = M.predict_f_batch(chosen, [X_full[: i + 1] for i in steps])
    f_means, f_vars, actual = [], [], []
    for i, (fm, fv) in zip(steps, preds):
        fm, fv = _np(fm), _np(fv)
        f_means.append(fm[-1] * std + mean)
        f_vars.append(fv[-1] * std ** 2)
        actual.append(Y_full[i] * std + mean)
    return f_means, f_vars, actual
