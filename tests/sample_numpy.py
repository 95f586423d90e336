"""numpy restatement of GPflow 2.9.1's GPModel.predict_f_samples / sample_mvn(full_cov=True) for one
latent GP, the semantic contract of models.GPR.predict_f_samples and gpx_sample_mvn:

    mean, cov = predict_f(Xs, full_cov=True)            (the oracle's OGPR here)
    L = cholesky(cov + jitter·I)
    sample_s = mean + L @ white_s

with two routes to L — LAPACK's (np.linalg.cholesky) and an unblocked column-by-column Cholesky in
plain numpy — whose difference is the reference's own error. Shared by tests/test_samples_api.py (CPU)
and tests/test_samples_gpu.py."""
import numpy as np

from oracle import gp_oracle as O

U = 2.0 ** -53            # fp64 unit roundoff
JITTER = 1e-6             # GPflow's default_jitter()
MS = (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200)   # the smallest shapes that cross each block boundary
SS = (1, 3, 17, 64, 65)
N_TRAIN = 89


def chol_lapack(A):
    return np.linalg.cholesky(A)


def chol_columns(A):
    """Unblocked column Cholesky (the second route): raises LinAlgError with the 1-based pivot."""
    A = np.array(A, dtype=np.float64)
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        s = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not (s[0] > 0.0 and np.isfinite(s[0])):
            raise np.linalg.LinAlgError(f"pivot {j + 1} is not positive")
        L[j, j] = np.sqrt(s[0])
        L[j + 1:, j] = s[1:] / L[j, j]
    return L


def sample_mvn(mean, cov, white, jitter=JITTER, chol=chol_lapack):
    """mean [M], cov [M, M], white [S, M] -> [S, M]."""
    L = chol(np.asarray(cov, dtype=np.float64) + jitter * np.eye(len(mean)))
    return np.asarray(mean)[None, :] + np.asarray(white) @ L.T


def predict_f_samples(om, Xs, white, jitter=JITTER, chol=chol_lapack):
    """The oracle model's joint draws at Xs for white [S, N*]: [S, N*, 1]."""
    mean, cov = om.predict_f(Xs, full_cov=True)
    return sample_mvn(mean[:, 0], cov, white, jitter, chol)[:, :, None]


def factor_bound(A, c=1.0):
    """Higham's componentwise backward-error bound for the Cholesky factor of A (Accuracy and
    Stability of Numerical Algorithms, Thm 10.5 with |L||Lᵀ|_ij <= sqrt(A_ii A_jj) up to 1 + O(u)):
    |LLᵀ − A|_ij <= c·(M+1)·u·sqrt(A_ii A_jj)."""
    d = np.sqrt(np.diag(A))
    return c * (A.shape[0] + 1) * U * np.outer(d, d)


def sample_bound(A, L, white):
    """Per sample s: 2·κ₂(A)·(M+1)·u·‖L‖_F·‖white_s‖₂ — the first-order perturbation bound of the
    Cholesky factor under a backward error of (M+1)·u·‖A‖ (‖ΔL‖_F <~ κ₂(A)·‖L‖·ε), doubled because
    the device's factor and the reference's both carry it."""
    k = np.linalg.cond(A)
    return 2.0 * k * (A.shape[0] + 1) * U * np.linalg.norm(L) * np.linalg.norm(white, axis=1)


def xs_for(M):
    """The prediction inputs of the SE / Matern52 cases: cond(cov + 1e-6·I) <= 2.5e7 at every M of MS."""
    return np.linspace(80.0, 80.0 + M / 2.0, M)[:, None]


def train_data(n=N_TRAIN, seed=7):
    x = np.arange(n, dtype=np.float64)[:, None]
    return x, O.synthetic_series(n, seed=seed)[1]


def se_oracle():
    x, y = train_data()
    return O.OGPR(x, y, O.OSquaredExponential(lengthscales=5.0), noise_variance=1e-5)


def matern_oracle():
    x, y = train_data()
    return O.OGPR(x, y, O.OMatern52(lengthscales=3.0), noise_variance=1e-3)
