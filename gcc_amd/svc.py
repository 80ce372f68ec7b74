"""C-SVC on frozen embeddings, on the device: every fold of a cross-validation and every class pair in one pass
(gcc_svc_distances / gcc_svc_solve / gcc_svc_predict, gcc_amd/csrc/svc.hip) -- what the reference's
gcc/tasks/graph_classification.py:47-64 does with one ``sklearn.svm.SVC(C=100000)`` fit per fold.

The classifier is libsvm's: an RBF kernel with ``gamma = 1 / (D * var(training rows))`` per fold, one problem per class pair,
SMO with the second-order working-set choice until ``max_{I_up} - min_{I_low} < tol``, votes in (i < j) order with ties to the
lowest class.  A problem's rows are the fold's training rows of its two classes, the lower class first (its rows are +1);
a positive decision value votes for the lower class.  Ties of a selection go to the lowest row of the problem, so a run
is reproducible, and the result does not depend on how the iterations are split over launches.

``SVCEngine.search_fit_predict_folds`` is the same task's ``search=True``: sklearn's ``GridSearchCV`` over C per outer fold, every
inner problem solved side by side by the same kernels (gcc_svc_search_*), then the refit at each fold's winner.
"""
from __future__ import annotations

import time

import numpy as np
import torch

from . import _cabi
from ._engine import CabiEngine

STATUS_BITS = {_cabi.STATUS_SVC_BAD_LABEL: "a label outside [0, classes)",
               _cabi.STATUS_SVC_BAD_FOLD: "a fold id outside [0, folds)",
               _cabi.STATUS_SVC_MISSING_CLASS: "a fold's training side lacks a class that its test side has",
               _cabi.STATUS_SVC_NONFINITE: "an embedding is NaN or infinite",
               _cabi.STATUS_SVC_ITER_CAP: "a problem stopped at the iteration cap before tol was reached",
               _cabi.STATUS_SVC_OVERFLOW: "a problem has more rows than the workspace was sized for"}


def largest_problem(labels, fold_of_row, classes, folds):
    """rows of the largest (fold, class pair) problem: per fold, the two largest training classes (entries out of range train
    nothing)"""
    labels, fold_of_row = np.asarray(labels, dtype=np.int64), np.asarray(fold_of_row, dtype=np.int64)
    ok = (labels >= 0) & (labels < classes) & (fold_of_row >= 0) & (fold_of_row < folds)
    test = np.zeros((folds, classes), dtype=np.int64)
    np.add.at(test, (fold_of_row[ok], labels[ok]), 1)
    train = np.sort(test.sum(0)[None, :] - test, axis=1)
    return int((train[:, -1] + train[:, -2]).max())


class SVCEngine(CabiEngine):
    """C-ABI calls of the classifier.  ``lib``/``ptr`` are injectable for the emulator tests only."""

    def _emb_args(self, emb):
        a = _cabi.GccSvcArgs()
        a.emb, a.N, a.D, a.ld = self.table(emb)
        return a

    def distances(self, emb):
        """emb float32 [N, D] (a row stride larger than D is served) -> d2 float32 [N, N], a view of the engine's workspace"""
        a = self._emb_args(emb)
        a.classes, a.folds, a.max_rows = 2, 1, 0
        nbytes = _cabi.size_query(self.lib, "gcc_svc_workspace_bytes", a.N, a.D, 2, 1, 0)
        ws = self.workspace(nbytes, emb.device)
        status = torch.zeros(1, dtype=torch.int32, device=emb.device)
        self.invoke("gcc_svc_distances", a, ws, status)
        return ws[: a.N * a.N * 4].view(torch.float32).view(a.N, a.N), status

    def fit_predict_folds(self, emb, labels, fold_of_row, C=1e5, tol=1e-3, iters_per_launch=65536, iter_cap=0, classes=None,
                          folds=None):
        """emb float32 [N, D]; labels / fold_of_row: N integers each (array or tensor), fold_of_row[r] = the fold whose test
        side holds row r.  ``classes`` / ``folds`` default to the largest entry + 1.  ``iter_cap``: total iterations of one
        problem, 0 for libsvm's max(10^7, 100 rows).  -> dict(pred int32 [N]; decision float64 [N, pairs]; iters int32, rho,
        obj float64, n_free, n_bounded, problem_rows int32 [folds, pairs]; gamma float64 [folds]; alpha float64 and rows int32
        [folds, pairs, max_rows] (0 past problem_rows); first_rows int32 [folds, pairs], the rows of the lower class;
        status int32 [1]; launches, classes, folds, pairs).  Everything runs on torch's current stream.  labels and
        fold_of_row are host inputs (tensors are copied to the host: the problem sizes come from them); after that the solve
        loop reads one integer per launch, and the status word is read by check_status."""
        a = self._emb_args(emb)
        dev = emb.device
        lab_h = labels.cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
        fold_h = fold_of_row.cpu().numpy() if isinstance(fold_of_row, torch.Tensor) else np.asarray(fold_of_row)
        if lab_h.shape != (a.N,) or fold_h.shape != (a.N,):
            raise ValueError(f"labels and fold_of_row must hold one entry per row of emb ({a.N})")
        classes = int(lab_h.max()) + 1 if classes is None else int(classes)
        folds = int(fold_h.max()) + 1 if folds is None else int(folds)
        if classes < 2:
            raise ValueError("a classifier needs at least two classes")
        if iter_cap < 0 or iter_cap >= 2 ** 31 or not 1 <= iters_per_launch < 2 ** 31:
            raise ValueError("iters_per_launch must be positive, iter_cap not negative, both below 2^31")
        pairs = classes * (classes - 1) // 2
        max_rows = largest_problem(lab_h, fold_h, classes, folds) if 1 <= folds <= _cabi.SVC_MAX_FOLDS else 0
        nbytes = _cabi.size_query(self.lib, "gcc_svc_workspace_bytes", a.N, a.D, classes, folds, max_rows)
        lab_d = torch.from_numpy(np.ascontiguousarray(lab_h, dtype=np.int32)).to(dev)
        fold_d = torch.from_numpy(np.ascontiguousarray(fold_h, dtype=np.int32)).to(dev)
        x = emb.to(torch.float64)
        gamma = self._gamma_scale(x, fold_d, folds)
        i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
        out = dict(pred=torch.empty(a.N, **i32), decision=torch.empty((a.N, pairs), **f64),
                   iters=torch.empty((folds, pairs), **i32), rho=torch.empty((folds, pairs), **f64),
                   obj=torch.empty((folds, pairs), **f64), n_free=torch.empty((folds, pairs), **i32),
                   n_bounded=torch.empty((folds, pairs), **i32), problem_rows=torch.empty((folds, pairs), **i32),
                   first_rows=torch.zeros((folds, pairs), **i32), rows=torch.zeros((folds, pairs, max(max_rows, 1)), **i32),
                   alpha=torch.zeros((folds, pairs, max(max_rows, 1)), **f64),
                   status=torch.zeros(1, **i32), gamma=gamma, classes=classes, folds=folds, pairs=pairs)
        unfinished = torch.zeros(1, **i32)
        a.labels, a.fold_of_row, a.gamma = self.ptr(lab_d), self.ptr(fold_d), self.ptr(gamma)
        a.classes, a.folds, a.max_rows = classes, folds, max_rows
        a.iters_per_launch, a.iter_cap, a.C, a.eps = int(iters_per_launch), int(iter_cap), float(C), float(tol)
        for name in ("pred", "decision", "iters", "rho", "obj", "n_free", "n_bounded", "problem_rows"):
            setattr(a, name, self.ptr(out[name]))
        a.unfinished, a.first_rows = self.ptr(unfinished), self.ptr(out["first_rows"])
        a.rows_out, a.alpha_out = self.ptr(out["rows"]), self.ptr(out["alpha"])
        ws = self.workspace(nbytes, dev)
        call = lambda name: self.invoke(name, a, ws, out["status"])  # noqa: E731
        call("gcc_svc_distances")
        # every problem ends at its iteration cap at the latest, so the launches are bounded too
        cap = iter_cap if iter_cap > 0 else max(10 ** 7, 100 * max_rows)
        launches = 0
        for _ in range(cap // int(iters_per_launch) + 2):
            call("gcc_svc_solve")
            launches += 1
            if int(unfinished.cpu()[0]) == 0:  # the one host read of a launch
                break
        else:
            raise RuntimeError("gcc_svc_solve: problems left unfinished past the iteration cap")
        call("gcc_svc_predict")
        out["launches"] = launches
        return out

    def search_fit_predict_folds(self, emb, labels, fold_of_row, inner_of_row, Cs, tol=1e-3, iters_per_launch=65536, iter_cap=0,
                                 classes=None, folds=None, inner=None, profile=False):
        """The grid search over C of sklearn's ``GridSearchCV(SVC(), {"C": Cs}, cv=inner, scoring="accuracy")`` per outer fold
        and the refit at each fold's winner, every inner problem (outer fold, inner fold, class pair, candidate) side by side
        over one distance matrix.  ``inner_of_row`` int [folds, N]: the inner fold of row r on outer fold o's training side (-1 on
        its test side; see ``inner_fold_table``).  An inner problem trains on the rows with fold_of_row != o and inner_of_row[o]
        != i from alpha = 0, with gamma "scale" of exactly those rows.  A candidate's score is the mean over the inner folds of
        correct / fold size in float64 (``np.mean``, as sklearn); the winner is the first candidate with the largest score.
        -> everything ``fit_predict_folds`` returns, of the refit (``status`` holds the refit's bits), and C_of_fold float64
        [folds], best_index int64 [folds], correct int32 [folds, candidates, inner], inner_sizes int64 [folds, inner], mean_score
        float64 [folds, candidates] (the last four on the host), search_iters int32 and search_rho float64 [folds, inner, pairs,
        candidates], search_problem_rows and search_first_rows int32 [folds, inner, pairs], search_rows int32 [folds, inner, pairs,
        max_inner_rows], search_alpha float64 [folds, inner, pairs, candidates, max_inner_rows], inner_gamma float64 [folds,
        inner], search_status int32 [1] (the inner problems' bits), search_launches, workspace_bytes.  An inner training side
        with fewer than two classes is refused before any launch (sklearn scores NaN there).  Host reads: one integer per solve
        launch, and the count table between scoring and refit.  ``profile``: also phase_s, the seconds of setup / solve / score / refit
        (the refit's predictions included), each taken after a device synchronisation that the plain run does not make."""
        a = _cabi.GccSvcSearchArgs()
        a.emb, a.N, a.D, a.ld = self.table(emb)
        dev = emb.device
        to_host = lambda v: v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)  # noqa: E731
        lab_h, fold_h, inner_h = to_host(labels), to_host(fold_of_row), to_host(inner_of_row)
        Cs_h = np.atleast_1d(np.asarray(to_host(Cs), dtype=np.float64))
        if lab_h.shape != (a.N,) or fold_h.shape != (a.N,):
            raise ValueError(f"labels and fold_of_row must hold one entry per row of emb ({a.N})")
        classes = int(lab_h.max()) + 1 if classes is None else int(classes)
        folds = int(fold_h.max()) + 1 if folds is None else int(folds)
        inner = int(inner_h.max()) + 1 if inner is None else int(inner)
        if classes < 2:
            raise ValueError("a classifier needs at least two classes")
        if inner_h.shape != (folds, a.N):
            raise ValueError(f"inner_of_row must be [folds, N] = [{folds}, {a.N}], found {list(inner_h.shape)}")
        if Cs_h.ndim != 1 or Cs_h.size < 1 or not (np.isfinite(Cs_h).all() and (Cs_h > 0).all()):
            raise ValueError("Cs must be a list of positive finite candidates")
        if iter_cap < 0 or iter_cap >= 2 ** 31 or not 1 <= iters_per_launch < 2 ** 31:
            raise ValueError("iters_per_launch must be positive, iter_cap not negative, both below 2^31")
        cands, pairs = int(Cs_h.size), classes * (classes - 1) // 2
        sizes_ok = 1 <= folds <= _cabi.SVC_MAX_FOLDS and 2 <= inner <= _cabi.SVC_SEARCH_MAX_INNER
        max_rows = max_inner = 0
        inner_sizes = np.zeros((folds, max(inner, 1)), dtype=np.int64)
        sides = []                                                 # per outer fold: its training rows
        if sizes_ok:
            lab_ok = (lab_h >= 0) & (lab_h < classes)
            for o in range(folds):
                tr = np.nonzero((fold_h != o) & (fold_h >= 0) & (fold_h < folds))[0]
                ids = inner_h[o, tr]
                if ((ids < 0) | (ids >= inner)).any():
                    raise ValueError(f"inner_of_row[{o}] must hold an inner fold in [0, {inner}) for every row of outer fold {o}'s "
                                     "training side")
                for i in range(inner):
                    seen = np.unique(lab_h[tr][(ids != i) & lab_ok[tr]])
                    if len(seen) < 2:
                        raise ValueError(f"outer fold {o}, inner fold {i}: the inner training side holds {len(seen)} class(es); "
                                         "a classifier needs two (sklearn scores NaN for every candidate there)")
                inner_sizes[o] = np.bincount(ids, minlength=inner)
                max_inner = max(max_inner, largest_problem(lab_h[tr], ids, classes, inner))
                sides.append(tr)
            max_rows = largest_problem(lab_h, fold_h, classes, folds)
        nbytes = _cabi.size_query(self.lib, "gcc_svc_search_workspace_bytes", a.N, a.D, classes, folds, inner, cands, max_rows,
                                  min(max_inner, max_rows))
        max_inner = min(max_inner, max_rows)
        i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
        put = lambda h, dt: torch.from_numpy(np.ascontiguousarray(h, dtype=dt)).to(dev)  # noqa: E731
        lab_d, fold_d, inner_d, Cs_d = put(lab_h, np.int32), put(fold_h, np.int32), put(inner_h, np.int32), put(Cs_h, np.float64)
        x = emb.to(torch.float64)
        gamma = self._gamma_scale(x, fold_d, folds)
        # an inner side's gamma: what the plain call computes for the outer fold's training rows as a corpus of their own
        inner_gamma = torch.stack([self._gamma_scale(x.index_select(0, put(tr, np.int64)), put(inner_h[o, tr], np.int32), inner)
                                   for o, tr in enumerate(sides)])
        G, P, cap, icap = folds * inner * pairs, folds * inner * pairs * cands, max(max_rows, 1), max(max_inner, 1)
        out = dict(pred=torch.empty(a.N, **i32), decision=torch.empty((a.N, pairs), **f64),
                   iters=torch.empty((folds, pairs), **i32), rho=torch.empty((folds, pairs), **f64),
                   obj=torch.empty((folds, pairs), **f64), n_free=torch.empty((folds, pairs), **i32),
                   n_bounded=torch.empty((folds, pairs), **i32), problem_rows=torch.empty((folds, pairs), **i32),
                   first_rows=torch.zeros((folds, pairs), **i32), rows=torch.zeros((folds, pairs, cap), **i32),
                   alpha=torch.zeros((folds, pairs, cap), **f64), status=torch.zeros(1, **i32), gamma=gamma,
                   classes=classes, folds=folds, pairs=pairs, inner=inner, candidates=cands, inner_gamma=inner_gamma,
                   search_status=torch.zeros(1, **i32), search_iters=torch.empty((folds, inner, pairs, cands), **i32),
                   search_rho=torch.empty((folds, inner, pairs, cands), **f64),
                   search_problem_rows=torch.empty((folds, inner, pairs), **i32),
                   search_first_rows=torch.zeros((folds, inner, pairs), **i32),
                   search_rows=torch.zeros((folds, inner, pairs, icap), **i32),
                   search_alpha=torch.zeros((folds, inner, pairs, cands, icap), **f64),
                   inner_sizes=inner_sizes, workspace_bytes=nbytes)
        assert out["search_rows"].numel() == G * icap and out["search_alpha"].numel() == P * icap
        correct, unfinished, C_of_fold = torch.zeros((folds, cands, inner), **i32), torch.zeros(1, **i32), torch.ones(folds, **f64)
        a.labels, a.fold_of_row, a.inner_of_row = self.ptr(lab_d), self.ptr(fold_d), self.ptr(inner_d)
        a.gamma, a.inner_gamma, a.Cs, a.C_of_fold = self.ptr(gamma), self.ptr(inner_gamma), self.ptr(Cs_d), self.ptr(C_of_fold)
        a.classes, a.folds, a.inner, a.candidates, a.max_rows, a.max_inner_rows = classes, folds, inner, cands, max_rows, max_inner
        a.iters_per_launch, a.iter_cap, a.eps = int(iters_per_launch), int(iter_cap), float(tol)
        a.unfinished, a.correct = self.ptr(unfinished), self.ptr(correct)
        for name in ("search_status", "search_iters", "search_rho", "search_problem_rows", "search_first_rows", "search_rows",
                     "search_alpha", "pred", "decision", "iters", "rho", "obj", "n_free", "n_bounded", "problem_rows", "first_rows"):
            setattr(a, name, self.ptr(out[name]))
        a.rows_out, a.alpha_out = self.ptr(out["rows"]), self.ptr(out["alpha"])
        ws = self.workspace(nbytes, dev)
        call = lambda name: self.invoke(name, a, ws, out["status"])  # noqa: E731
        limit = (iter_cap if iter_cap > 0 else max(10 ** 7, 100 * max_rows)) // int(iters_per_launch) + 2

        def solve(name):
            for launch in range(limit):        # every problem ends at its iteration cap at the latest
                call(name)
                if int(unfinished.cpu()[0]) == 0:  # the one host read of a launch
                    return launch + 1
            raise RuntimeError(f"{name}: problems left unfinished past the iteration cap")

        marks = [time.perf_counter()]

        def mark():
            if profile:
                if dev.type == "cuda":
                    torch.cuda.synchronize(dev)
                marks.append(time.perf_counter())

        call("gcc_svc_search_setup")
        mark()
        out["search_launches"] = solve("gcc_svc_search_solve")
        mark()
        call("gcc_svc_search_score")
        out["correct"] = correct.cpu().numpy()                     # the one host read between scoring and refit
        with np.errstate(invalid="ignore", divide="ignore"):
            accuracy = out["correct"].astype(np.float64) / inner_sizes[:, None, :].astype(np.float64)
        out["mean_score"] = np.mean(np.ascontiguousarray(accuracy), axis=-1)   # (sklearn's own reduction over a candidate's folds)
        out["best_index"] = np.argmax(out["mean_score"], axis=1)    # the first of the largest: ties go to the earlier candidate
        out["C_of_fold"] = Cs_h[out["best_index"]]
        C_of_fold.copy_(put(out["C_of_fold"], np.float64))
        mark()
        out["launches"] = solve("gcc_svc_search_refit")
        call("gcc_svc_search_predict")
        mark()
        if profile:
            out["phase_s"] = dict(zip(("setup", "solve", "score", "refit"), np.diff(marks).tolist()))
        return out

    @staticmethod
    def _gamma_scale(x, fold_d, folds):
        """sklearn's gamma="scale" per fold, 1 / (D var) over all elements of the fold's training rows, in float64 and without
        a host read: per-row sums of the table (shifted by its mean, which the variance does not see) are added up per test
        fold in a fixed order, and a fold's training side is the total minus its own.  x float64 [N, D] -> float64 [folds]"""
        D = x.shape[1]
        # (a [folds, N] membership mask and row-wise sums, not index_add: its atomics would make gamma differ from run to run)
        m = (fold_d[None, :] == torch.arange(folds, dtype=fold_d.dtype, device=x.device)[:, None]).to(torch.float64)
        xc = x - (x * m.sum(0)[:, None]).sum() / (m.sum() * D).clamp(min=1.0)
        n, s1, s2 = m.sum(1) * D, (m * xc.sum(1)[None, :]).sum(1), (m * (xc * xc).sum(1)[None, :]).sum(1)
        n, s1, s2 = n.sum() - n, s1.sum() - s1, s2.sum() - s2
        var = s2 / n - (s1 / n) ** 2
        return torch.where(var > 0, 1.0 / (D * var), torch.ones_like(var))       # (an empty or constant side: 1, as sklearn)

    @staticmethod
    def check_status(result, allow_iter_cap=False):
        """Raises and names the bits of the call's status word (one host read).  The iteration cap raises unless allowed:
        libsvm only warns there, and the result is the solver's state at the cap."""
        allow = _cabi.STATUS_SVC_ITER_CAP if allow_iter_cap else 0
        CabiEngine.raise_status(result, "gcc_svc", STATUS_BITS, allow)
        if "search_status" in result:          # the inner problems of a search: a class that an inner training side lacks only
            # costs the candidate those rows, as in sklearn
            CabiEngine.raise_status(dict(status=result["search_status"]), "gcc_svc_search (inner problems)", STATUS_BITS,
                                    allow | _cabi.STATUS_SVC_MISSING_CLASS)


def inner_fold_table(labels, fold_of_row, inner, folds=None):
    """inner_of_row int32 [folds, N] of ``SVCEngine.search_fit_predict_folds``: per outer fold, sklearn's ``StratifiedKFold(inner)``
    without shuffle -- what ``cv=inner`` means for a classifier -- over the fold's training rows in ascending corpus order; -1 on
    the fold's test side"""
    from sklearn.model_selection import StratifiedKFold

    labels, fold_of_row = np.asarray(labels), np.asarray(fold_of_row)
    folds = int(fold_of_row.max()) + 1 if folds is None else int(folds)
    table = np.full((folds, len(labels)), -1, dtype=np.int32)
    for o in range(folds):
        tr = np.nonzero(fold_of_row != o)[0]
        for i, (_, held) in enumerate(StratifiedKFold(n_splits=inner).split(np.zeros(len(tr)), labels[tr])):
            table[o, tr[held]] = i
    return table
