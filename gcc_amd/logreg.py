"""One-vs-rest logistic regression on frozen embeddings, on the device: every fold of a cross-validation and every class in one
pass (gcc_logreg_setup / gcc_logreg_step / gcc_logreg_predict, gcc_amd/csrc/logreg.hip) -- what the reference's
gcc/tasks/node_classification.py:53-101 does with one ``TopKRanker(LogisticRegression(C=1000))`` fit per fold.

Every (fold, class) problem computes the minimiser of sklearn's objective

    f(w, b) = 1/2 |w|^2 + intercept_penalty 1/2 b^2 + C sum_{training rows} [log(1 + exp(z_r)) - t_r z_r],  z_r = w . x_r + b

by damped Newton steps in float64 until ``max|grad f| / C <= tol`` -- not sklearn's default iterate, which stops 2e-3 to 10 away
from it in decision value.  A held-out row is given the k classes of highest decision value, k = its label count (no label:
every class); ties go to the lower class.  A column that is constant on a fold's training side is not solved: decision -inf
(all zeros) or +inf (all ones), as sklearn's one-vs-rest predicts probability 0 or 1 there.  The result does not depend on how
the iterations are split over host reads.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _cabi
from ._engine import CabiEngine

STATUS_BITS = {_cabi.STATUS_LR_BAD_FOLD: "a fold id outside [0, folds)",
               _cabi.STATUS_LR_NONFINITE: "an embedding is NaN or infinite",
               _cabi.STATUS_LR_ITER_CAP: "a problem stopped at the iteration cap before tol was reached",
               _cabi.STATUS_LR_PIVOT: "a problem met a non-positive pivot in the Cholesky factorisation of its Hessian",
               _cabi.STATUS_LR_LINE_SEARCH: "a problem's line search found no decrease down to a step of 2^-40"}


class LogRegEngine(CabiEngine):
    """C-ABI calls of the classifier.  ``lib``/``ptr`` are injectable for the emulator tests only."""

    def fit_predict_folds(self, emb, y, fold_of_row, C=1000.0, tol=1e-9, intercept_penalty=0.0, iters_per_sync=4, iter_cap=200,
                          folds=None):
        """emb float32 [N, D] (a row stride larger than D is served); y [N, classes], non-zero = the row has the label;
        fold_of_row: N integers, the fold whose test side holds the row (``folds`` defaults to the largest entry + 1).
        -> dict(pred uint8 [N, classes]; decision float64 [N, classes]; counts int32 [folds, 3] = tp, fp, fn; coef float64
        [folds, classes, D]; intercept float64, iters int32, grad float64 (the final max|g| / C), state int32 [folds, classes];
        status int32 [1]; syncs, the host reads of the unfinished count).  Everything runs on torch's current stream; y and
        fold_of_row may be arrays or tensors."""
        a = _cabi.GccLogregArgs()
        a.emb, N, D, a.ld = self.table(emb)
        a.N, a.D = N, D
        dev = emb.device
        y_t = y if isinstance(y, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(y))
        fold_t = fold_of_row if isinstance(fold_of_row, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(fold_of_row))
        if y_t.dim() != 2 or y_t.shape[0] != N or fold_t.shape != (N,):
            raise ValueError(f"y must be [N, classes] and fold_of_row [N] with one row per row of emb ({N})")
        classes = int(y_t.shape[1])
        if folds is None:
            folds = int(fold_t.max()) + 1 if N else 0
        if not 1 <= int(iters_per_sync) < 2 ** 31 or not 1 <= int(iter_cap) < 2 ** 31:
            raise ValueError("iters_per_sync and iter_cap must be positive and below 2^31")
        nbytes = _cabi.size_query(self.lib, "gcc_logreg_workspace_bytes", N, D, classes, int(folds))
        y_d = (y_t != 0).to(torch.uint8).to(dev).contiguous()
        fold_d = fold_t.to(torch.int32).to(dev).contiguous()
        i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
        out = dict(pred=torch.empty((N, classes), dtype=torch.uint8, device=dev), decision=torch.empty((N, classes), **f64),
                   counts=torch.empty((folds, 3), **i32), coef=torch.empty((folds, classes, D), **f64),
                   intercept=torch.empty((folds, classes), **f64), iters=torch.empty((folds, classes), **i32),
                   grad=torch.empty((folds, classes), **f64), state=torch.empty((folds, classes), **i32),
                   status=torch.zeros(1, **i32))
        unfinished = torch.zeros(1, **i32)
        a.y, a.fold_of_row, a.classes, a.folds = self.ptr(y_d), self.ptr(fold_d), classes, int(folds)
        a.iters_per_sync, a.iter_cap = int(iters_per_sync), int(iter_cap)
        a.C, a.tol, a.intercept_penalty = float(C), float(tol), float(intercept_penalty)
        for name in ("pred", "decision", "counts", "coef", "intercept", "iters", "grad", "state"):
            setattr(a, name, self.ptr(out[name]))
        a.unfinished = self.ptr(unfinished)
        ws = self.workspace(nbytes, dev)
        call = lambda name: self.invoke(name, a, ws, out["status"])  # noqa: E731
        call("gcc_logreg_setup")
        # every problem ends at its iteration cap at the latest, so the host reads are bounded too
        syncs = 0
        for _ in range(int(iter_cap) // int(iters_per_sync) + 2):
            call("gcc_logreg_step")
            syncs += 1
            if int(unfinished.cpu()[0]) == 0:  # the one host read of a batch of iterations
                break
        else:
            raise RuntimeError("gcc_logreg_step: problems left unfinished past the iteration cap")
        call("gcc_logreg_predict")
        out["syncs"] = syncs
        return out

    @staticmethod
    def check_status(result, allow_iter_cap=False):
        """Raises and names the bits of the call's status word (one host read).  The iteration cap raises unless allowed: the
        result is then the solver's state at the cap."""
        CabiEngine.raise_status(result, "gcc_logreg", STATUS_BITS, _cabi.STATUS_LR_ITER_CAP if allow_iter_cap else 0)
