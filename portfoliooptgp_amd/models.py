"""gpflow.models.GPR 2.9.1 surface backed by the HIP engine.

Reference call sites this serves: ``gpflow.models.GPR(data=(X_tf, Y_tf), kernel=kernel)``
(GPR/model_trainer.py:15), ``model.likelihood.variance.assign`` / ``set_trainable``
(:16-17), ``model.training_loss`` / ``model.trainable_variables`` (:19), ``model.predict_f``
(:20, GPR/predictor.py:6) and ``model.predict_y`` (GPR/predictor.py:7); and
``gpflow.models.GPR((X, Y), kernel=deepcopy(k), noise_variance=v)``
(Multi-Input_GPR/main.py:421-423, Multi-Input_GPR/models/model_trainer.py:31).

Arithmetic: every logML / gradient / prediction is computed by libgpx.so on the GPU. The
outputs are torch float64 tensors: on the CPU when the data came in as numpy / CPU tensors
(so ``.numpy()``, arithmetic and slicing work as on the tf tensors GPflow returns), else on
the GPU.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native as N
from .engine import DEFAULT_JITTER, Engine, check_jitter, default_device, solo_engine
from .kernels import Kernel, compile_spec, coregion_term, has_ard, has_coregion
from .likelihoods import Gaussian, StudentT
from .mean_functions import MeanFunction, Zero
from .parameter import ArrayParameter, Parameter, VectorParameter, sigmoid


def _refuse_ard(kernel: Kernel, model: str) -> None:
    """ARD lengthscales are served by models.GPR; the sparse / variational models evaluate K
    through the isotropic device functions."""
    if has_ard(kernel):
        raise NotImplementedError(f"{model} takes kernels with scalar lengthscales: ARD (vector) "
                                  "lengthscales are implemented for models.GPR")


def _refuse_coregion(kernel: Kernel, model: str) -> None:
    """Coregion kernels are served by models.GPR (the dense route's Coregion kernels); the sparse /
    variational models evaluate K through the isotropic device functions."""
    if has_coregion(kernel):
        raise NotImplementedError(f"{model} does not take kernels with a Coregion term: Coregion is "
                                  "implemented for models.GPR")


def _gaussian_log_density(model, data) -> torch.Tensor:
    """GPflow's GPModel.predict_log_density for a Gaussian likelihood: log N(Ynew | predict_y's mean,
    predict_y's variance), summed over the output column -> [N*]. Placed like predict_y's outputs."""
    if not isinstance(model.likelihood, Gaussian):
        raise NotImplementedError("predict_log_density is implemented for the Gaussian likelihood (GPflow "
                                  "integrates other likelihoods by quadrature)")
    Xnew, Ynew = data
    mean, var = model.predict_y(Xnew)
    y = Ynew if isinstance(Ynew, torch.Tensor) else torch.as_tensor(np.asarray(Ynew, dtype=np.float64))
    y = y.to(device=mean.device, dtype=torch.float64).reshape(-1, 1)
    if y.shape != mean.shape:
        raise ValueError(f"Ynew must have one row per row of Xnew ({mean.shape[0]}), got {tuple(y.shape)}")
    return (-0.5 * (np.log(2.0 * np.pi) + torch.log(var) + (y - mean) ** 2 / var)).sum(dim=-1)


def _nrows(x) -> int:
    return int(x.shape[0]) if hasattr(x, "shape") and len(x.shape) > 0 else len(x)


def _sample_args(Xnew, num_samples, white, jitter, full_cov: bool, full_output_cov: bool):
    """predict_f_samples' argument checks, before anything touches a device: (S, N*, white as a
    float64 tensor [S, N*] or None, jitter)."""
    if full_cov and full_output_cov:
        # GPflow 2.9 GPModel.predict_f_samples raises for this too
        raise NotImplementedError("The combination of both `full_cov` and `full_output_cov` is not permitted.")
    if num_samples is not None and (int(num_samples) != num_samples or num_samples <= 0):
        raise ValueError(f"num_samples must be a positive integer or None, got {num_samples}")
    S = 1 if num_samples is None else int(num_samples)
    jitter = DEFAULT_JITTER if jitter is None else check_jitter(jitter)
    nstar = _nrows(Xnew)
    if white is not None:
        w = white if isinstance(white, torch.Tensor) else torch.as_tensor(np.asarray(white, dtype=np.float64))
        want = (nstar, 1) if num_samples is None else (S, nstar, 1)
        if tuple(w.shape) != want:
            raise ValueError(f"white must have shape {want}, got {tuple(w.shape)}")
        white = w.detach().to(torch.float64).reshape(S, nstar)
    return S, nstar, white, jitter


class GPR:
    """Exact GP regression with a Gaussian likelihood and a zero or parametric mean function
    (mean_functions.Constant / Linear / Polynomial: the device factorises against y − m(X; β))."""

    def __init__(self, data: Tuple, kernel: Kernel, mean_function=None,
                 noise_variance: Optional[float] = None, likelihood: Optional[Gaussian] = None,
                 device: Optional[int] = None):
        if mean_function is not None and not isinstance(mean_function, MeanFunction):
            raise NotImplementedError("mean_function must be one of portfoliooptgp_amd.mean_functions "
                                      "(Zero, Constant, Linear, Polynomial) or None")
        X, Y = data
        self._out_cpu = not (isinstance(Y, torch.Tensor) and Y.is_cuda)
        Xt = X if isinstance(X, torch.Tensor) else torch.as_tensor(np.asarray(X, dtype=np.float64))
        Yt = Y if isinstance(Y, torch.Tensor) else torch.as_tensor(np.asarray(Y, dtype=np.float64))
        Xt = Xt.to(torch.float64)
        Yt = Yt.to(torch.float64)
        if Xt.ndim == 1:
            Xt = Xt[:, None]
        if Yt.ndim == 1:
            Yt = Yt[:, None]
        if Yt.shape[1] != 1:
            raise NotImplementedError("single-output GPR only (Y must be [N, 1])")
        if Xt.shape[0] != Yt.shape[0]:
            raise ValueError("X and Y must have the same number of rows")
        if Xt.shape[0] == 0:
            # GPflow would return the prior; the device engine needs at least one training point
            # (an empty factorisation has nothing to run on the GPU), so refuse it up front
            raise ValueError("GPR needs at least one training point (X has 0 rows)")
        self.data = (Xt, Yt)
        self.kernel = kernel
        if likelihood is None:
            likelihood = Gaussian(1.0 if noise_variance is None else noise_variance)
        elif noise_variance is not None:
            raise ValueError("give either noise_variance or likelihood")
        self.likelihood = likelihood
        # (Zero() is kept as given; it has no parameters and the device treats it as no mean)
        self.mean_function = mean_function
        self.num_latent_gps = 1
        self.device = default_device() if device is None else int(device)
        self._spec = compile_spec(kernel, Xt.shape[1])
        # a Coregion term: the index column of X must hold exact integers in [0, P)
        self._coreg = coregion_term(kernel)
        if self._coreg is not None:
            self._coreg.check_index(Xt.detach().cpu().numpy(), "X")
        self._mean = mean_function if mean_function is not None and mean_function.n_coef > 0 else None
        if self._mean is not None:
            self._mean._check_dim(int(Xt.shape[1]))
            if self._spec.n_params + 1 + self._mean.n_coef > N.GPX_THETA_STRIDE:
                raise ValueError(
                    f"the θ row holds {N.GPX_THETA_STRIDE} values: {self._spec.n_params} kernel parameters + the "
                    f"noise variance + {self._mean.n_coef} mean coefficients do not fit")
        self._engine: Optional[Engine] = None
        self._engine_index = 0

    # ---------------------------------------------------------------- structure -------
    @property
    def parameters(self) -> Tuple[Parameter, ...]:
        # GPR attributes sorted: kernel < likelihood < mean_function
        return (tuple(self.kernel.parameters) + tuple(self.likelihood.parameters)
                + (tuple(self._mean.parameters) if self._mean is not None else ()))

    @property
    def trainable_parameters(self) -> Tuple[Parameter, ...]:
        return tuple(p for p in self.parameters if p.trainable)

    @property
    def trainable_variables(self):
        return tuple(p.unconstrained_variable for p in self.trainable_parameters)

    def _param_paths(self):
        return ([("GPR.kernel." + n if n else "GPR.kernel", p) for n, p in self.kernel._param_paths("")]
                + [("GPR.likelihood.variance", self.likelihood.variance)]
                + ([("GPR.mean_function." + n, p) for n, p in self._mean._param_paths()]
                   if self._mean is not None else []))

    @property
    def n_kernel_params(self) -> int:
        return int(self._spec.n_params)

    def theta_row(self) -> np.ndarray:
        """Constrained θ in the gpx layout: kernel params, then σn² at index n_params, then the
        mean function's coefficients (gpx_mean_spec order)."""
        row = np.ones(N.GPX_THETA_STRIDE, dtype=np.float64)
        kv = self.kernel.theta_values()  # (an ARD lengthscale vector: one column per entry)
        row[:len(kv)] = kv
        row[len(kv)] = self.likelihood.variance.value
        if self._mean is not None:
            c = self._mean.coefficients()
            row[len(kv) + 1: len(kv) + 1 + len(c)] = c
        return row

    def mean_spec(self):
        """The slot's gpx_mean_spec (None: zero mean)."""
        return self._mean.spec() if self._mean is not None else None

    # ---------------------------------------------------------------- engine ----------
    def _attach(self, engine: Engine, index: int) -> None:
        self._engine, self._engine_index = engine, index
        if self._mean is not None or getattr(engine, "has_mean", False):
            engine.set_mean(index, self.mean_spec())

    def engine(self) -> Tuple[Engine, int]:
        """(engine, slot): the batch engine this model was attached to, else a pooled
        single-problem engine for its shape (engine.solo_engine)."""
        if self._engine is None:
            return solo_engine(self), 0
        return self._engine, self._engine_index

    def _wrap(self, t: torch.Tensor) -> torch.Tensor:
        t = t.reshape(-1, 1)
        return t.cpu() if self._out_cpu else t

    # ---------------------------------------------------------------- objective -------
    def _lml_and_grad_theta(self):
        eng, b = self.engine()
        row = self.theta_row()
        lml, grad, info = eng.lml_grad_row(b, row)
        if info == N.INFO_BAD_THETA:
            raise N.InvalidParameterError("hyperparameters out of range (every kernel parameter and the noise "
                                          f"finite and > 0, a Coregion W finite): {row[:eng.n_params[b] + 1]}")
        if info != 0:
            raise N.NotPositiveDefiniteError(
                f"Cholesky decomposition was not successful: pivot {int(info)} of K + noise I "
                "is not positive", info)
        return lml, grad

    def log_marginal_likelihood(self) -> torch.Tensor:
        return torch.tensor(self._lml_and_grad_theta()[0], dtype=torch.float64)

    def maximum_log_likelihood_objective(self) -> torch.Tensor:
        return self.log_marginal_likelihood()

    def training_loss(self) -> torch.Tensor:
        """−logML (no priors), the closure GPR/model_trainer.py:19 hands to Scipy."""
        return -self.log_marginal_likelihood()

    def training_loss_closure(self, compile: bool = True):
        def closure():
            return self.training_loss()
        closure._gpx_model = self
        return closure

    def _variable_map(self, variables):
        """(variables, θ-row index of each flattened variable entry, its Parameter, its entry
        index), cached for the variables object an optimiser passes on every call (kernel
        parameters, then σn² at n_params, then the mean function's coefficients). An array
        variable (a mean parameter, an ARD lengthscale vector) takes one consecutive column per
        entry, so ``rows`` follows the optimiser's flattened x; ``ents`` is the entry's index
        into a VectorParameter (None for every other parameter)."""
        cache = getattr(self, "_grad_map", None)
        if cache is None or cache[0] is not variables:
            pindex, nk = {}, 0  # parameter -> (first column, columns)
            for p in self.kernel.parameters:
                # (a Coregion W: one column per entry, row-major, the identity transform)
                cnt = (p.size if isinstance(p, VectorParameter)
                       else int(np.prod(p.shape)) if isinstance(p, ArrayParameter) else 1)
                pindex[id(p)] = (nk, cnt)
                nk += cnt
            mindex, o = {}, nk + 1
            for p in (self._mean.parameters if self._mean is not None else ()):
                mindex[id(p)] = (o, int(np.prod(p.shape)))
                o += mindex[id(p)][1]
            rows, params, ents = [], [], []
            for v in variables:
                p = v._param
                if p is self.likelihood.variance:
                    rows.append(nk)
                    params.append(p)
                    ents.append(None)
                elif id(p) in pindex:
                    c0, cnt = pindex[id(p)]
                    rows.extend(range(c0, c0 + cnt))
                    params.extend([p] * cnt)
                    ents.extend(range(cnt) if isinstance(p, VectorParameter) else [None] * cnt)
                elif id(p) in mindex:
                    c0, cnt = mindex[id(p)]
                    rows.extend(range(c0, c0 + cnt))
                    params.extend([p] * cnt)
                    ents.extend([None] * cnt)
                else:
                    raise ValueError(f"variable {v.name} is not a parameter of this model")
            cache = self._grad_map = (variables, rows, params, ents)
        return cache

    def theta_layout(self, variables, transforms: bool = False):
        """(cols int32 [P], lower float64 [P]): θ-row index and Shift of each flattened variable
        entry, for the batched driver's native θ / chain-rule helpers (gpx_host_theta_rows /
        _loss_grad_u). With ``transforms`` a third array, int32 [P]: the entry's transform code
        (0 softplus + Shift, 1 identity: a mean coefficient; gpx_host_theta_rows_t)."""
        _, rows, params, _ = self._variable_map(variables)
        cols = np.asarray(rows, dtype=np.int32)
        ident = [isinstance(p, ArrayParameter) for p in params]
        lower = np.asarray([0.0 if i else p.lower for p, i in zip(params, ident)], dtype=np.float64)
        if not transforms:
            return cols, lower
        return cols, lower, np.asarray([N.TRANSFORM_IDENTITY if i else N.TRANSFORM_SOFTPLUS for i in ident],
                                       dtype=np.int32)

    def loss_and_grad_unconstrained(self, variables=None, lml=None, grad_theta=None):
        """(−logML, ∂(−logML)/∂u) for ``variables`` (default: trainable_variables)."""
        if lml is None:
            lml, grad_theta = self._lml_and_grad_theta()
        variables = self.trainable_variables if variables is None else variables
        _, rows, params, ents = self._variable_map(variables)
        g = np.empty(len(rows), dtype=np.float64)
        for k, (r, p, e) in enumerate(zip(rows, params, ents)):
            if isinstance(p, ArrayParameter):  # (a mean coefficient's transform is the identity: ∂θ/∂u = 1)
                g[k] = -grad_theta[r]
            elif e is not None:                # (an ARD lengthscale: its own sigmoid(u_d))
                g[k] = -grad_theta[r] * sigmoid(p.unconstrained[e])
            else:
                g[k] = -grad_theta[r] * p.dtheta_du()
        return -float(lml), g

    # ---------------------------------------------------------------- prediction ------
    def predict_f(self, Xnew, full_cov: bool = False, full_output_cov: bool = False):
        """Posterior of the latent f: mean [N*,1] and var [N*,1], or with full_cov the
        covariance [1,N*,N*] (GPflow's layout with one latent GP; full_output_cov changes
        nothing for a single output)."""
        return self._predict(Xnew, add_noise=False, full_cov=full_cov)

    def predict_y(self, Xnew, full_cov: bool = False, full_output_cov: bool = False):
        if full_cov or full_output_cov:
            # GPflow 2.9 GPModel.predict_y raises for these too
            raise NotImplementedError("The predict_y method currently supports only the argument "
                                      "values full_cov=False and full_output_cov=False")
        return self._predict(Xnew, add_noise=True)

    def _predict(self, Xnew, add_noise: bool, full_cov: bool = False):
        if self._coreg is not None:  # (a Coregion term: Xnew's index column is checked like X's)
            xn = Xnew.detach().cpu().numpy() if isinstance(Xnew, torch.Tensor) else np.asarray(Xnew, dtype=np.float64)
            self._coreg.check_index(xn.reshape(xn.shape[0], -1) if xn.ndim != 2 else xn, "Xnew")
        eng, b = self.engine()
        theta = np.ones((eng.B, N.GPX_THETA_STRIDE))
        theta[b] = self.theta_row()
        cpu_out = not (isinstance(Xnew, torch.Tensor) and Xnew.is_cuda)
        m, v, _ = eng.predict([b], theta, [Xnew], add_noise, full_cov=full_cov)
        m = m[0].reshape(-1, 1)
        v = v[0].unsqueeze(0) if full_cov else v[0].reshape(-1, 1)
        if cpu_out:
            m, v = m.cpu(), v.cpu()
        return m, v

    def predict_log_density(self, data, full_cov: bool = False, full_output_cov: bool = False):
        """log p(Ynew | Xnew) per point, [N*]: the Gaussian log density of Ynew under predict_y."""
        if full_cov or full_output_cov:
            raise NotImplementedError("The predict_log_density method currently supports only the argument "
                                      "values full_cov=False and full_output_cov=False")
        return _gaussian_log_density(self, data)

    def predict_f_samples(self, Xnew, num_samples: Optional[int] = None, full_cov: bool = True,
                          full_output_cov: bool = False, *, white=None, generator=None, jitter=None):
        """Draws from the posterior of the latent f at Xnew: [S, N*, 1], or [N*, 1] when
        ``num_samples`` is None (GPflow's GPModel.predict_f_samples and its sample_mvn arithmetic).
        With full_cov the draws are joint, mean + chol(cov + jitter·I)·white on the device (the
        covariance never leaves it); without, mean + sqrt(var)·white per point (no jitter, no clamp).
        ``white``: the standard-normal input, [S, N*, 1] ([N*, 1] without num_samples); absent, it is
        drawn by torch.randn on the model's device with ``generator``. ``jitter``: None is GPflow's
        default 1e-6. Outputs are placed like predict_f's."""
        S, nstar, white, jitter = _sample_args(Xnew, num_samples, white, jitter, full_cov, full_output_cov)
        return _predict_f_samples([self], [Xnew], S, full_cov, [white], generator, jitter,
                                  squeeze=num_samples is None)[0]


def _predict_f_samples(models, Xnews, S: int, full_cov: bool, whites, generator, jitter: float,
                       squeeze: bool = False):
    """predict_f_samples of models that share one engine, after the argument checks: one device pass."""
    eng, _ = models[0].engine()
    idx = [m.engine()[1] for m in models]
    dev = f"cuda:{eng.device}"
    for m, x in zip(models, Xnews):
        if m._coreg is not None:  # (a Coregion term: Xnew's index column is checked like X's)
            xn = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x, dtype=np.float64)
            m._coreg.check_index(xn.reshape(xn.shape[0], -1) if xn.ndim != 2 else xn, "Xnew")
    whites = [torch.randn(S, _nrows(x), dtype=torch.float64, device=dev, generator=generator) if w is None
              else w.to(dev) for w, x in zip(whites, Xnews)]
    theta = np.ones((eng.B, N.GPX_THETA_STRIDE))
    for m, b in zip(models, idx):
        theta[b] = m.theta_row()
    out = [None] * len(models)
    live = [k for k, x in enumerate(Xnews) if _nrows(x) > 0]
    for k in set(range(len(models))) - set(live):
        out[k] = torch.empty(S, 0, dtype=torch.float64, device=dev)
    if live and full_cov:
        _, smp, _ = eng.predict_samples([idx[k] for k in live], theta, [Xnews[k] for k in live],
                                        [whites[k] for k in live], jitter)
        for k, s in zip(live, smp):
            out[k] = s
    elif live:
        ms, vs, _ = eng.predict([idx[k] for k in live], theta, [Xnews[k] for k in live], False)
        for k, m, v in zip(live, ms, vs):
            out[k] = m.reshape(1, -1) + torch.sqrt(v).reshape(1, -1) * whites[k]
    res = []
    for x, s in zip(Xnews, out):
        s = s.unsqueeze(-1)
        if squeeze:
            s = s[0]
        res.append(s.cpu() if not (isinstance(x, torch.Tensor) and x.is_cuda) else s)
    return res


def predict_f_samples_batch(models: Sequence[GPR], Xnews: Sequence, num_samples: int, full_cov: bool = True,
                            whites: Optional[Sequence] = None, generator=None, jitter=None):
    """predict_f_samples for several models in one device pass when they share an engine (fitted by
    Scipy().minimize_batch), like predict_f_batch; otherwise one by one. Ragged N* is padded per
    call; each model's draws equal its own predict_f_samples call bit for bit (same ``white``).
    ``whites``: one [S, N*_i, 1] per model, or None. Returns a list of [S, N*_i, 1]."""
    if num_samples is None:
        raise ValueError("predict_f_samples_batch needs num_samples")
    whites = [None] * len(models) if whites is None else list(whites)
    if len(Xnews) != len(models) or len(whites) != len(models):
        raise ValueError("predict_f_samples_batch needs one Xnew (and one white) per model")
    args = [_sample_args(x, num_samples, w, jitter, full_cov, False) for x, w in zip(Xnews, whites)]
    S, jit = args[0][0], args[0][3]
    shared = all(m._engine is not None for m in models) and len({id(m.engine()[0]) for m in models}) == 1
    if not shared:
        return [_predict_f_samples([m], [x], S, full_cov, [a[2]], generator, jit)[0]
                for m, x, a in zip(models, Xnews, args)]
    return _predict_f_samples(list(models), list(Xnews), S, full_cov, [a[2] for a in args], generator, jit)


def predict_f_batch(models: Sequence[GPR], Xnews: Sequence, add_noise: bool = False):
    """predict_f (or predict_y) for several models sharing one engine, in one device pass.
    Models not attached to a shared batch engine are predicted one by one."""
    if any(m._engine is None for m in models):
        return [(m.predict_y(x) if add_noise else m.predict_f(x)) for m, x in zip(models, Xnews)]
    eng, _ = models[0].engine()
    idx = []
    for m in models:
        e, b = m.engine()
        if e is not eng:
            raise ValueError("models must share an engine (fit them with Scipy().minimize_batch)")
        idx.append(b)
    theta = np.ones((eng.B, N.GPX_THETA_STRIDE))
    for m, b in zip(models, idx):
        theta[b] = m.theta_row()
    ms, vs, _ = eng.predict(idx, theta, Xnews, add_noise)
    out = []
    for x, m, v in zip(Xnews, ms, vs):
        cpu_out = not (isinstance(x, torch.Tensor) and x.is_cuda)
        m, v = m.reshape(-1, 1), v.reshape(-1, 1)
        out.append((m.cpu(), v.cpu()) if cpu_out else (m, v))
    return out


class SVGP:
    """gpflow.models.SVGP with a Gaussian or StudentT likelihood and GPflow's defaults (whiten=True,
    full q_sqrt, zero mean, one latent GP) — the cells at test_scripts/SVGP.py:461-478 and
    test_scripts/GPR.py:118-138::

        m = SVGP(kernel=k, likelihood=Gaussian(variance=1e-4), inducing_variable=Z, num_data=N)
        set_trainable(m.likelihood.variance, False)
        Scipy().minimize(m.training_loss_closure((X, Y)), m.trainable_variables,
                         options=dict(maxiter=100))
        mean, var = m.predict_f(X_test)

    ELBO, gradients and predictions come from libgpx.so (gpx_svgp_*); trainable variables
    are ordered as tf.Module flattens SVGP: inducing_variable.Z, kernel.*, likelihood.variance
    (likelihood.scale for StudentT), q_mu, q_sqrt (FillTriangular-unconstrained).

    ``per_point=True`` selects the per-point evaluation route (gpx_svgp_create_lik): the marginal of
    every data row and GPflow's variational expectation of it, for either likelihood. It is what
    serves ``likelihoods.StudentT(scale, df)`` (20-point Gauss–Hermite; predict_y adds
    scale²·df/(df − 2)), and it is opt-in::

        m = SVGP(kernel=k, likelihood=StudentT(), inducing_variable=Z, num_data=N, per_point=True)

    Without the keyword the model is what it was: the Gaussian likelihood by the closed-form route,
    and StudentT refused at construction (one more M×N device buffer and about a tenth more time
    per evaluation are not taken without being asked for)."""

    def __init__(self, kernel: Kernel, likelihood, inducing_variable, *, mean_function=None,
                 num_latent_gps: int = 1, q_diag: bool = False, q_mu=None, q_sqrt=None,
                 whiten: bool = True, num_data: Optional[int] = None, device: Optional[int] = None,
                 per_point: bool = False):
        from .inducing_variables import InducingPoints
        from .parameter import ArrayParameter
        if mean_function is not None:
            raise NotImplementedError("only the zero mean function (GPflow default) is supported")
        if num_latent_gps != 1 or q_diag or not whiten:
            raise NotImplementedError("SVGP supports GPflow's defaults: one latent GP, full q_sqrt, whiten=True")
        if not isinstance(likelihood, (Gaussian, StudentT)):
            raise NotImplementedError("SVGP supports the Gaussian and StudentT likelihoods")
        if isinstance(likelihood, StudentT) and not per_point:
            raise NotImplementedError("SVGP evaluates the StudentT likelihood by the per-point route only: pass "
                                      "per_point=True (the Gaussian and StudentT likelihoods are supported)")
        _refuse_ard(kernel, "SVGP")
        _refuse_coregion(kernel, "SVGP")
        self.kernel = kernel
        self.likelihood = likelihood
        self.inducing_variable = (inducing_variable if isinstance(inducing_variable, InducingPoints)
                                  else InducingPoints(inducing_variable))
        M = self.inducing_variable.num_inducing
        self.num_data = num_data
        self.num_latent_gps = 1
        self.whiten = True
        self.per_point = bool(per_point)
        self.q_mu = ArrayParameter(np.zeros((M, 1)) if q_mu is None else np.asarray(q_mu).reshape(M, 1),
                                   name="q_mu")
        self.q_sqrt = ArrayParameter(np.eye(M)[None] if q_sqrt is None else q_sqrt,
                                     transform="triangular", name="q_sqrt")
        self.device = default_device() if device is None else int(device)
        self._engines = {}

    # ---------------------------------------------------------------- structure -------
    @property
    def parameters(self):
        return ((self.inducing_variable.Z,) + tuple(self.kernel.parameters)
                + tuple(self.likelihood.parameters) + (self.q_mu, self.q_sqrt))

    @property
    def trainable_parameters(self):
        return tuple(p for p in self.parameters if p.trainable)

    @property
    def trainable_variables(self):
        return tuple(p.unconstrained_variable for p in self.trainable_parameters)

    @property
    def _lik_param(self) -> Parameter:
        return self.likelihood.scale if isinstance(self.likelihood, StudentT) else self.likelihood.variance

    def _engine_likelihood(self) -> dict:
        """The likelihood arguments of the SVGPEngine that serves this model."""
        if isinstance(self.likelihood, StudentT):
            return dict(likelihood=N.GPX_LIK_STUDENT_T, df=self.likelihood.df, per_point=True)
        return dict(likelihood=N.GPX_LIK_GAUSSIAN, per_point=self.per_point)

    def _param_paths(self):
        return ([("SVGP.inducing_variable.Z", self.inducing_variable.Z)]
                + [("SVGP.kernel." + n if n else "SVGP.kernel", p) for n, p in self.kernel._param_paths("")]
                + [("SVGP.likelihood." + self._lik_param.name, self._lik_param),
                   ("SVGP.q_mu", self.q_mu), ("SVGP.q_sqrt", self.q_sqrt)])

    @property
    def M(self) -> int:
        return self.inducing_variable.num_inducing

    def theta_row(self) -> np.ndarray:
        row = np.ones(N.GPX_THETA_STRIDE, dtype=np.float64)
        kp = self.kernel.parameters
        for i, p in enumerate(kp):
            row[i] = p.value
        row[len(kp)] = self._lik_param.value
        return row

    def _state(self):
        return (self.theta_row(), self.inducing_variable.Z.value, self.q_mu.value.reshape(-1),
                self.q_sqrt.value[0])

    # ---------------------------------------------------------------- engine ----------
    def engine(self, data=None) -> "SVGPEngine":
        from .engine import SVGPEngine
        if data is None:
            if self._engines:
                return next(iter(self._engines.values()))[0]
            Z = self.inducing_variable.Z.value
            data = (Z[:1], np.zeros((1, 1)))
        X, Y = data
        key = (id(X), id(Y))
        hit = self._engines.get(key)
        if hit is None or hit[1] is not X or hit[2] is not Y:
            Xa = X if isinstance(X, torch.Tensor) else np.asarray(X, dtype=np.float64)
            n = int(Xa.shape[0])
            D = 1 if Xa.ndim == 1 else int(Xa.shape[1])
            eng = SVGPEngine(X, Y, compile_spec(self.kernel, D), self.M,
                             num_data=float(self.num_data if self.num_data is not None else n),
                             device=self.device, **self._engine_likelihood())
            hit = (eng, X, Y)
            self._engines = {key: hit}
        return hit[0]

    # ---------------------------------------------------------------- objective -------
    def _elbo_and_grads(self, data):
        eng = self.engine(data)
        return eng.elbo_grad(*self._state())

    def elbo(self, data) -> torch.Tensor:
        return torch.tensor(self._elbo_and_grads(data)[0], dtype=torch.float64)

    def maximum_log_likelihood_objective(self, data) -> torch.Tensor:
        return self.elbo(data)

    def training_loss(self, data) -> torch.Tensor:
        return -self.elbo(data)

    def training_loss_closure(self, data, compile: bool = True):
        def closure():
            return self.training_loss(data)
        closure._gpx_model = self
        closure._gpx_loss_and_grad = lambda variables=None: self.loss_and_grad_unconstrained(data, variables)
        return closure

    def grads_to_unconstrained(self, variables, elbo, gth, gZ, gq, gR):
        """(−ELBO, ∂(−ELBO)/∂u flattened in ``variables`` order)."""
        kp = self.kernel.parameters
        pindex = {id(p): i for i, p in enumerate(kp)}
        parts = []
        for v in variables:
            p = v._param
            if p is self.inducing_variable.Z:
                parts.append(-np.asarray(gZ).ravel())
            elif p is self._lik_param:
                parts.append(np.array([-gth[len(kp)] * p.dtheta_du()]))
            elif id(p) in pindex:
                parts.append(np.array([-gth[pindex[id(p)]] * p.dtheta_du()]))
            elif p is self.q_mu:
                parts.append(-np.asarray(gq).ravel())
            elif p is self.q_sqrt:
                parts.append(-p.grad_to_unconstrained(gR).ravel())
            else:
                raise ValueError(f"variable {v.name} is not a parameter of this model")
        return -float(elbo), np.concatenate(parts)

    def loss_and_grad_unconstrained(self, data, variables=None):
        variables = self.trainable_variables if variables is None else variables
        return self.grads_to_unconstrained(variables, *self._elbo_and_grads(data))

    # ---------------------------------------------------------------- prediction ------
    def predict_f(self, Xnew, full_cov: bool = False, full_output_cov: bool = False):
        if full_cov or full_output_cov:
            raise NotImplementedError("SVGP.predict_f supports full_cov=False (marginals)")
        return self._predict(Xnew, False)

    def predict_log_density(self, data):
        """log p(Ynew | Xnew) per point, [N*], under predict_y (Gaussian likelihood; with StudentT
        GPflow integrates by quadrature: NotImplementedError)."""
        return _gaussian_log_density(self, data)

    def predict_y(self, Xnew, full_cov: bool = False, full_output_cov: bool = False):
        if full_cov or full_output_cov:
            raise NotImplementedError("The predict_y method currently supports only the argument "
                                      "values full_cov=False and full_output_cov=False")
        return self._predict(Xnew, True)

    def _predict(self, Xnew, add_noise: bool):
        cpu_out = not (isinstance(Xnew, torch.Tensor) and Xnew.is_cuda)
        m, v = self.engine().predict(*self._state(), Xnew, add_noise)
        m, v = m.reshape(-1, 1), v.reshape(-1, 1)
        if cpu_out:
            m, v = m.cpu(), v.cpu()
        return m, v


def predict_f_svgp_batch(models: Sequence[SVGP], Xnews: Sequence, add_noise: bool = False):
    """predict_f (or predict_y) of several SVGP models fitted by Scipy().minimize_svgp_batch, over the
    engine they are bound to (gpx_svgp_small_predict, one slot per model). A model that is not bound
    to one (over the fused path's limits, or never fitted in a batch) is predicted by its own
    predict_f / predict_y. Returns [(mean [Mn, 1], var [Mn, 1])] like the models' own methods."""
    out = []
    for m, x in zip(models, Xnews):
        bound = getattr(m, "_small", None)
        if bound is None:
            out.append(m.predict_y(x) if add_noise else m.predict_f(x))
            continue
        eng, b = bound
        mean, var = eng.predict(b, *m._state(), x, add_noise)
        mean = torch.from_numpy(mean).reshape(-1, 1)
        var = torch.from_numpy(var).reshape(-1, 1)
        if isinstance(x, torch.Tensor) and x.is_cuda:
            mean, var = mean.to(x.device), var.to(x.device)
        out.append((mean, var))
    return out


class SGPR:
    """gpflow.models.SGPR: sparse GP regression by the collapsed (Titsias) bound, Gaussian
    likelihood, zero mean, one output — the cell at test_scripts/SVGP.py:395-412::

        m = SGPR((X, Y), kernel=SquaredExponential(), inducing_variable=np.linspace(0, 360, 10)[:, None])
        Scipy().minimize(m.training_loss, m.trainable_variables)
        mean, var = m.predict_y(X_test)

    The bound, its gradients and the predictions come from libgpx.so (gpx_sgpr_*); trainable
    variables are ordered as tf.Module flattens SGPR: inducing_variable.Z, kernel.*,
    likelihood.variance. Not provided: mean functions, several output columns, other
    likelihoods, full_cov, upper_bound."""

    def __init__(self, data: Tuple, kernel: Kernel, inducing_variable, *, mean_function=None,
                 num_latent_gps: Optional[int] = None, noise_variance: Optional[float] = None,
                 likelihood: Optional[Gaussian] = None, device: Optional[int] = None):
        from .inducing_variables import InducingPoints
        if mean_function is not None and not isinstance(mean_function, Zero):
            raise NotImplementedError("SGPR supports only the zero mean function (GPflow's default)")
        if num_latent_gps not in (None, 1):
            raise NotImplementedError("SGPR supports one latent GP (Y must be [N, 1])")
        X, Y = data
        self._out_cpu = not (isinstance(Y, torch.Tensor) and Y.is_cuda)
        Xt = X if isinstance(X, torch.Tensor) else torch.as_tensor(np.asarray(X, dtype=np.float64))
        Yt = Y if isinstance(Y, torch.Tensor) else torch.as_tensor(np.asarray(Y, dtype=np.float64))
        Xt, Yt = Xt.to(torch.float64), Yt.to(torch.float64)
        if Xt.ndim == 1:
            Xt = Xt[:, None]
        if Yt.ndim == 1:
            Yt = Yt[:, None]
        if Yt.shape[1] != 1:
            raise NotImplementedError("single-output SGPR only (Y must be [N, 1])")
        if Xt.shape[0] != Yt.shape[0]:
            raise ValueError("X and Y must have the same number of rows")
        if Xt.shape[0] == 0:
            raise ValueError("SGPR needs at least one training point (X has 0 rows)")
        if likelihood is None:
            likelihood = Gaussian(1.0 if noise_variance is None else noise_variance)
        elif noise_variance is not None:
            raise ValueError("give either noise_variance or likelihood")
        if not isinstance(likelihood, Gaussian):
            raise NotImplementedError("SGPR supports the Gaussian likelihood")
        self.data = (Xt, Yt)
        _refuse_ard(kernel, "SGPR")
        _refuse_coregion(kernel, "SGPR")
        self.kernel = kernel
        self.likelihood = likelihood
        self.mean_function = mean_function
        self.inducing_variable = (inducing_variable if isinstance(inducing_variable, InducingPoints)
                                  else InducingPoints(inducing_variable))
        if self.inducing_variable.Z.shape[1] != Xt.shape[1]:
            raise ValueError("inducing points and X must have the same number of columns")
        self.num_latent_gps = 1
        self.device = default_device() if device is None else int(device)
        self._spec = compile_spec(kernel, Xt.shape[1])
        self._engine = None

    # ---------------------------------------------------------------- structure -------
    @property
    def parameters(self):
        return ((self.inducing_variable.Z,) + tuple(self.kernel.parameters) + tuple(self.likelihood.parameters))

    @property
    def trainable_parameters(self):
        return tuple(p for p in self.parameters if p.trainable)

    @property
    def trainable_variables(self):
        return tuple(p.unconstrained_variable for p in self.trainable_parameters)

    def _param_paths(self):
        return ([("SGPR.inducing_variable.Z", self.inducing_variable.Z)]
                + [("SGPR.kernel." + n if n else "SGPR.kernel", p) for n, p in self.kernel._param_paths("")]
                + [("SGPR.likelihood.variance", self.likelihood.variance)])

    @property
    def M(self) -> int:
        return self.inducing_variable.num_inducing

    def theta_row(self) -> np.ndarray:
        row = np.ones(N.GPX_THETA_STRIDE, dtype=np.float64)
        kp = self.kernel.parameters
        for i, p in enumerate(kp):
            row[i] = p.value
        row[len(kp)] = self.likelihood.variance.value
        return row

    def _state(self):
        return self.theta_row(), self.inducing_variable.Z.value

    # ---------------------------------------------------------------- engine ----------
    def engine(self) -> "SGPREngine":
        from .engine import SGPREngine
        if self._engine is None:
            self._engine = SGPREngine(self.data[0], self.data[1], self._spec, self.M, device=self.device)
        return self._engine

    # ---------------------------------------------------------------- objective -------
    def _elbo_and_grads(self):
        return self.engine().elbo_grad(*self._state())

    def elbo(self) -> torch.Tensor:
        return torch.tensor(self._elbo_and_grads()[0], dtype=torch.float64)

    def maximum_log_likelihood_objective(self) -> torch.Tensor:
        return self.elbo()

    def training_loss(self) -> torch.Tensor:
        """−F (no priors), the bound method the reference hands to Scipy().minimize."""
        return -self.elbo()

    def training_loss_closure(self, compile: bool = True):
        def closure():
            return self.training_loss()
        closure._gpx_model = self
        return closure

    def grads_to_unconstrained(self, variables, elbo, gth, gZ):
        """(−F, ∂(−F)/∂u flattened in ``variables`` order)."""
        kp = self.kernel.parameters
        pindex = {id(p): i for i, p in enumerate(kp)}
        parts = []
        for v in variables:
            p = v._param
            if p is self.inducing_variable.Z:
                parts.append(-np.asarray(gZ).ravel())
            elif p is self.likelihood.variance:
                parts.append(np.array([-gth[len(kp)] * p.dtheta_du()]))
            elif id(p) in pindex:
                parts.append(np.array([-gth[pindex[id(p)]] * p.dtheta_du()]))
            else:
                raise ValueError(f"variable {v.name} is not a parameter of this model")
        return -float(elbo), np.concatenate(parts)

    def loss_and_grad_unconstrained(self, variables=None):
        variables = self.trainable_variables if variables is None else variables
        return self.grads_to_unconstrained(variables, *self._elbo_and_grads())

    # ---------------------------------------------------------------- prediction ------
    def predict_f(self, Xnew, full_cov: bool = False, full_output_cov: bool = False):
        if full_cov or full_output_cov:
            raise NotImplementedError("SGPR.predict_f supports full_cov=False (marginals)")
        return self._predict(Xnew, False)

    def predict_log_density(self, data):
        """log p(Ynew | Xnew) per point, [N*]: the Gaussian log density of Ynew under predict_y."""
        return _gaussian_log_density(self, data)

    def predict_y(self, Xnew, full_cov: bool = False, full_output_cov: bool = False):
        if full_cov or full_output_cov:
            raise NotImplementedError("The predict_y method currently supports only the argument "
                                      "values full_cov=False and full_output_cov=False")
        return self._predict(Xnew, True)

    def _predict(self, Xnew, add_noise: bool):
        cpu_out = not (isinstance(Xnew, torch.Tensor) and Xnew.is_cuda)
        m, v = self.engine().predict(*self._state(), Xnew, add_noise)
        m, v = m.reshape(-1, 1), v.reshape(-1, 1)
        if cpu_out:
            m, v = m.cpu(), v.cpu()
        return m, v


def predict_f_sgpr_batch(models: Sequence[SGPR], Xnews: Sequence, add_noise: bool = False):
    """predict_f (or predict_y) of several SGPR models fitted by Scipy().minimize_sgpr_batch, over the
    engine they are bound to (gpx_sgpr_small_predict, one slot per model). A model that is not bound
    to one (over the fused path's limits, or never fitted in a batch) is predicted by its own
    predict_f / predict_y. Returns [(mean [Mn, 1], var [Mn, 1])] like the models' own methods."""
    out = []
    for m, x in zip(models, Xnews):
        bound = getattr(m, "_small", None)
        if bound is None:
            out.append(m.predict_y(x) if add_noise else m.predict_f(x))
            continue
        eng, b = bound
        mean, var = eng.predict(b, *m._state(), x, add_noise)
        mean = torch.from_numpy(mean).reshape(-1, 1)
        var = torch.from_numpy(var).reshape(-1, 1)
        if isinstance(x, torch.Tensor) and x.is_cuda:
            mean, var = mean.to(x.device), var.to(x.device)
        out.append((mean, var))
    return out


class VGP:
    """gpflow.models.VGP with GPflow's defaults (whitened, full q_sqrt, zero mean, one latent GP)
    and a Gaussian or StudentT likelihood — the cell at test_scripts/SVGP.py:402-437::

        m = VGP((X, Y), kernel=SquaredExponential(), likelihood=StudentT())
        Scipy().minimize(m.training_loss, m.trainable_variables)
        mean, var = m.predict_y(X_test)

    q_mu starts at zeros [N, 1], q_sqrt at the identity [1, N, N]. The ELBO (closed form for the
    Gaussian, GPflow's 20-point Gauss–Hermite rule for StudentT), its gradients and the predictions
    come from libgpx.so (gpx_vgp_*); trainable variables are ordered as tf.Module flattens VGP:
    kernel.*, likelihood.scale / likelihood.variance, q_mu, q_sqrt (FillTriangular-unconstrained).
    Not provided: mean functions, several output columns, other likelihoods, full_cov."""

    def __init__(self, data: Tuple, kernel: Kernel, likelihood, mean_function=None,
                 num_latent_gps: Optional[int] = None, device: Optional[int] = None):
        if mean_function is not None and not isinstance(mean_function, Zero):
            raise NotImplementedError("VGP supports only the zero mean function (GPflow's default)")
        if num_latent_gps not in (None, 1):
            raise NotImplementedError("VGP supports one latent GP (Y must be [N, 1])")
        if not isinstance(likelihood, (Gaussian, StudentT)):
            raise NotImplementedError("VGP supports the Gaussian and StudentT likelihoods")
        X, Y = data
        Xt = X if isinstance(X, torch.Tensor) else torch.as_tensor(np.asarray(X, dtype=np.float64))
        Yt = Y if isinstance(Y, torch.Tensor) else torch.as_tensor(np.asarray(Y, dtype=np.float64))
        Xt, Yt = Xt.to(torch.float64), Yt.to(torch.float64)
        if Xt.ndim == 1:
            Xt = Xt[:, None]
        if Yt.ndim == 1:
            Yt = Yt[:, None]
        if Yt.shape[1] != 1:
            raise NotImplementedError("single-output VGP only (Y must be [N, 1])")
        if Xt.shape[0] != Yt.shape[0]:
            raise ValueError("X and Y must have the same number of rows")
        if Xt.shape[0] == 0:
            raise ValueError("VGP needs at least one training point (X has 0 rows)")
        n = int(Xt.shape[0])
        self.data = (Xt, Yt)
        _refuse_ard(kernel, "VGP")
        _refuse_coregion(kernel, "VGP")
        self.kernel = kernel
        self.likelihood = likelihood
        self.mean_function = mean_function
        self.num_data = n
        self.num_latent_gps = 1
        self.q_mu = ArrayParameter(np.zeros((n, 1)), name="q_mu")
        self.q_sqrt = ArrayParameter(np.eye(n)[None], transform="triangular", name="q_sqrt")
        self.device = default_device() if device is None else int(device)
        self._spec = compile_spec(kernel, Xt.shape[1])
        self._engine = None

    # ---------------------------------------------------------------- structure -------
    @property
    def _lik_param(self) -> Parameter:
        return self.likelihood.scale if isinstance(self.likelihood, StudentT) else self.likelihood.variance

    @property
    def parameters(self):
        return tuple(self.kernel.parameters) + tuple(self.likelihood.parameters) + (self.q_mu, self.q_sqrt)

    @property
    def trainable_parameters(self):
        return tuple(p for p in self.parameters if p.trainable)

    @property
    def trainable_variables(self):
        return tuple(p.unconstrained_variable for p in self.trainable_parameters)

    def _param_paths(self):
        return ([("VGP.kernel." + n if n else "VGP.kernel", p) for n, p in self.kernel._param_paths("")]
                + [("VGP.likelihood." + self._lik_param.name, self._lik_param),
                   ("VGP.q_mu", self.q_mu), ("VGP.q_sqrt", self.q_sqrt)])

    def theta_row(self) -> np.ndarray:
        row = np.ones(N.GPX_THETA_STRIDE, dtype=np.float64)
        kp = self.kernel.parameters
        for i, p in enumerate(kp):
            row[i] = p.value
        row[len(kp)] = self._lik_param.value
        return row

    def _state(self):
        return self.theta_row(), self.q_mu.value.reshape(-1), self.q_sqrt.value[0]

    # ---------------------------------------------------------------- engine ----------
    def engine(self) -> "VGPEngine":
        from .engine import VGPEngine
        if self._engine is None:
            st = isinstance(self.likelihood, StudentT)
            self._engine = VGPEngine(self.data[0], self.data[1], self._spec,
                                     N.GPX_LIK_STUDENT_T if st else N.GPX_LIK_GAUSSIAN,
                                     df=self.likelihood.df if st else 3.0, device=self.device)
        return self._engine

    # ---------------------------------------------------------------- objective -------
    def _elbo_and_grads(self):
        row = self.theta_row()
        np_ = len(self.kernel.parameters)
        if not np.all(np.isfinite(row[:np_ + 1])) or not np.all(row[:np_ + 1] > 0.0):
            raise N.InvalidParameterError(f"hyperparameters out of (0, inf): {row[:np_ + 1]}")
        return self.engine().elbo_grad(*self._state())

    def elbo(self) -> torch.Tensor:
        return torch.tensor(self._elbo_and_grads()[0], dtype=torch.float64)

    def maximum_log_likelihood_objective(self) -> torch.Tensor:
        return self.elbo()

    def training_loss(self) -> torch.Tensor:
        """−ELBO (no priors), the bound method the reference hands to Scipy().minimize."""
        return -self.elbo()

    def training_loss_closure(self, compile: bool = True):
        def closure():
            return self.training_loss()
        closure._gpx_model = self
        return closure

    def grads_to_unconstrained(self, variables, elbo, gth, gq, gR):
        """(−ELBO, ∂(−ELBO)/∂u flattened in ``variables`` order)."""
        kp = self.kernel.parameters
        pindex = {id(p): i for i, p in enumerate(kp)}
        parts = []
        for v in variables:
            p = v._param
            if p is self._lik_param:
                parts.append(np.array([-gth[len(kp)] * p.dtheta_du()]))
            elif id(p) in pindex:
                parts.append(np.array([-gth[pindex[id(p)]] * p.dtheta_du()]))
            elif p is self.q_mu:
                parts.append(-np.asarray(gq).ravel())
            elif p is self.q_sqrt:
                parts.append(-p.grad_to_unconstrained(gR).ravel())
            else:
                raise ValueError(f"variable {v.name} is not a parameter of this model")
        return -float(elbo), np.concatenate(parts)

    def loss_and_grad_unconstrained(self, variables=None):
        variables = self.trainable_variables if variables is None else variables
        return self.grads_to_unconstrained(variables, *self._elbo_and_grads())

    # ---------------------------------------------------------------- prediction ------
    def predict_f(self, Xnew, full_cov: bool = False, full_output_cov: bool = False):
        if full_cov or full_output_cov:
            raise NotImplementedError("VGP.predict_f supports full_cov=False (marginals)")
        return self._predict(Xnew, False)

    def predict_log_density(self, data):
        """log p(Ynew | Xnew) per point, [N*], under predict_y (Gaussian likelihood; with StudentT
        GPflow integrates by quadrature: NotImplementedError)."""
        return _gaussian_log_density(self, data)

    def predict_y(self, Xnew, full_cov: bool = False, full_output_cov: bool = False):
        if full_cov or full_output_cov:
            raise NotImplementedError("The predict_y method currently supports only the argument "
                                      "values full_cov=False and full_output_cov=False")
        return self._predict(Xnew, True)

    def _predict(self, Xnew, predict_y: bool):
        cpu_out = not (isinstance(Xnew, torch.Tensor) and Xnew.is_cuda)
        m, v = self.engine().predict(*self._state(), Xnew, predict_y)
        m, v = m.reshape(-1, 1), v.reshape(-1, 1)
        if cpu_out:
            m, v = m.cpu(), v.cpu()
        return m, v
