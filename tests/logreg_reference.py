"""A float64 NumPy restatement of the Newton iteration of gcc_amd/csrc/logreg.hip, the second yardstick of tests/logreg_check.py
(the first is sklearn's converged newton-cholesky fit): the minimiser of

    f(w, b) = 1/2 |w|^2 + rho 1/2 b^2 + C sum_r [log(1 + exp(z_r)) - t_r z_r],   z_r = w . x_r + b

from w = b = 0, by Cholesky of the exact Hessian and Armijo backtracking (constant 1e-4, step halving down to 2^-40), until
max|grad f| / C <= tol.  Also the top-k rule and the gradient norm the tests recompute."""
import numpy as np


def objective(A, t, w, C, R):
    z = A @ w
    return 0.5 * (R * w * w).sum() + C * (np.logaddexp(0.0, z) - t * z).sum()


def gradient(A, t, w, C, R):
    p = 0.5 * (1.0 + np.tanh(0.5 * (A @ w)))                      # the sigmoid, without overflow
    return R * w + C * (A.T @ (p - t)), p


def newton(X, t, C=1000.0, rho=0.0, tol=1e-9, iter_cap=200):
    """X [n, D] (any float type), t [n] in {0, 1} -> (w [D], b, iterations, max|g| / C)"""
    X = np.asarray(X, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    n, D = X.shape
    A = np.hstack([X, np.ones((n, 1))])
    R = np.ones(D + 1)
    R[D] = rho
    w = np.zeros(D + 1)
    for it in range(iter_cap + 1):
        g, p = gradient(A, t, w, C, R)
        gmax = float(np.abs(g).max()) / C
        if gmax <= tol or it == iter_cap:
            break
        H = np.diag(R) + C * (A.T * (p * (1.0 - p))) @ A
        L = np.linalg.cholesky(H)
        d = np.linalg.solve(L.T, np.linalg.solve(L, g))
        dec, f0, s = float(g @ d), objective(A, t, w, C, R), 1.0
        slack = 64.0 * np.finfo(np.float64).eps * abs(f0)          # the rounding of the two sums (see lr_search_kernel)
        while s >= 2.0 ** -40 and not objective(A, t, w - s * d, C, R) <= f0 - 1e-4 * s * dec + slack:
            s *= 0.5
        if s < 2.0 ** -40:
            raise RuntimeError("no decrease down to a step of 2^-40")
        w = w - s * d
    return w[:D], float(w[D]), it, gmax


def grad_norm(X, t, coef, intercept, C=1000.0, rho=0.0):
    """max|grad f| / C at (coef, intercept), in float64"""
    X = np.asarray(X, dtype=np.float64)
    A = np.hstack([X, np.ones((len(X), 1))])
    R = np.ones(X.shape[1] + 1)
    R[-1] = rho
    g, _ = gradient(A, np.asarray(t, dtype=np.float64), np.append(coef, intercept), C, R)
    return float(np.abs(g).max()) / C


def top_k(decision, y):
    """the rule of the device: per row the k classes that come first under (decision descending, class ascending), k = the row's
    label count, and every class for a row without labels -> uint8 [rows, classes]"""
    n, classes = decision.shape
    pred = np.zeros((n, classes), dtype=np.uint8)
    for r in range(n):
        k = int((y[r] != 0).sum())
        order = sorted(range(classes), key=lambda c: (-decision[r, c], c))
        pred[r, order[: k if k > 0 else classes]] = 1
    return pred


def counts(pred, y, fold, folds):
    """tp, fp, fn per fold over its held-out rows -> int64 [folds, 3]"""
    out = np.zeros((folds, 3), dtype=np.int64)
    p, t = pred != 0, y != 0
    for f in range(folds):
        m = fold == f
        out[f] = (p[m] & t[m]).sum(), (p[m] & ~t[m]).sum(), (~p[m] & t[m]).sum()
    return out
