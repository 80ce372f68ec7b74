"""Shared by tests/test_posemb_width_emu.py and tests/test_posemb_width_gpu.py: the positional-embedding solver
(gcc_amd/csrc/posemb.hip) at widths below 32, into output buffers that are NOT zero when the call starts, and on graphs with
more than one component or with nodes of degree 0 -- every solver class, against the dense float64 decomposition and the
invariants of tests/test_posemb_emu.py.  TEST INFRASTRUCTURE ONLY.  The CPU-only part (cases, float64 reference, assertions on
the cases themselves) needs no kernel; tests/test_posemb_width_emu.py runs it.

Bars: none are chosen here.  _check / _check_krylov of tests/test_posemb_emu.py keep theirs (2e-4 strict, 1e-3 Krylov, 5e-3
Gram, 1e-4 row norms); everything this file adds is exact (== 0, == SENTINEL, set equality).

Widths (WIDTHS): 2 is the smallest the C ABI takes; 5 makes 20-byte rows; 16 | 17 are the two sides of the one-wave teams' second
store; 30 is a value train.py users pick, 31 its odd neighbour; 32 is the baseline every other test runs.

Items per width (width_items): the k = min(n - 2, width) edge (n = 1, 2, 3, h + 1, h + 2, h + 3), one item per solver class by deflated
size, the degenerate spectra (star, K4, path), and the disconnected ones:
    iso40     20 + 15 + K2 + 3 isolated nodes (eigenvalue 1 three times)             one-wave team / small class
    two70     40 + 30                                                                65..128 class
    iso155    90 + 60 + path3 + 2 isolated nodes                                     block / slot class
    free5     5 nodes, no edge: M = 0, k = 3, every wanted eigenvalue is 0
    iso763    skewed_dense_graph(760) + 3 isolated nodes (ONE component with edges)  Krylov
    comm763   8 dense communities of 95 nodes, thinly linked, + 3 isolated nodes     Krylov
Every random item is the first of seed, seed + 100, ... whose float64 spectrum meets its conditions (connected_item,
disconnected_item): no kernel result enters the choice.

Output buffers (run_filled): every tensor of the DevicePosEmb's ring, ``evals`` and ``raw`` hold SENTINEL before the call and
have at least SPARE rows beyond node_off[B].  Afterwards every cell of a row < N has been written, the padding columns k.. are
exactly 0 in all three, rows >= N (and the ring's other tensors) still hold SENTINEL.

The Gram comparison only applies where the wanted subspace is unique; gram_applies() says so from float64 alone, the CPU-only
part pins which (item, width) pairs that is (UNMARKED lists every exception and why), and both tiers assert that the checker
compared exactly those.

The isolated-node rule (check_isolated).  A node i of degree 0 has (M u)_i = 0, hence u_i = 0 in every eigenvector with a non-zero
eigenvalue.  Neither the reference (sklearn's normalize of ARPACK's rounding noise is a unit row of noise) nor float64 eigh
defines the row, so it is asserted on its own: in every column whose float64 eigenvalue exceeds ISO_EIG = 0.1 in magnitude the
entries of degree-0 nodes are EXACTLY zero in ``raw`` and ``pos``; where every wanted eigenvalue does (ISO_WHOLE_ROWS: float64
says so at the widths listed there) their whole rows are.  Columns of eigenvalue 0 -- free5, and the wide cuts that reach the null
space -- carry only the existing invariants: there the isolated nodes' rows are part of a basis of the null space.
iso763 is the Krylov item the rule was first observed on, but the second eigenvalue of skewed_dense_graph(760) is 0.097: under
the 0.1 bar only its column of eigenvalue 1 is bound, at any width.  comm763 is the Krylov item on which the bar binds whole
rows: its eight community eigenvalues lie above 0.8 and the bulk of a 95-node community of density 0.5 ends near 0.2."""
import os

import numpy as np
import torch

from gcc_amd.graphgen import tiny_graphs
from oracle import posemb as P
from tests.test_posemb_emu import (DIRECT_MAX, SLOT_MAX, _dense_eigh, _sub, check_by_path, reduced_sizes,
                                   skewed_dense_graph)

WIDTHS = (2, 5, 16, 17, 30, 31, 32)
EMU_WIDTHS = (2, 5, 16, 17, 30, 31)
EMU_BIG_WIDTH = 6                 # the emulator's slowest items (385..704 class, Krylov) run at one narrow width only
SENTINEL = 7.25                   # finite, non-zero, exact in fp32 and outside [-1, 1]: no solver output can equal it
SPARE = 64
ISO_EIG = 0.1
GAP = 1e-3                        # _check's "wanted subspace unique" condition
BLOCK_EDGES = 12288               # directed edges the block class keeps in LDS; denser items are handed on (status word 3)
KNOBS = {"default": {}, "wave0": {"GCC_POSEMB_WAVE": "0"}, "pair0": {"GCC_POSEMB_PAIR": "0"},
         "cheb0": {"GCC_POSEMB_CHEB": "0"}}


# ---------------------------------------------------------------------------------------------------------------- the cases
def _view(n, edges):
    import scipy.sparse as sp

    e = np.array(sorted(set((min(i, j), max(i, j)) for i, j in edges)), dtype=np.int64).reshape(-1, 2)
    assert (e[:, 0] != e[:, 1]).all()
    a = sp.csr_matrix((np.ones(2 * len(e)), (np.r_[e[:, 0], e[:, 1]], np.r_[e[:, 1], e[:, 0]])), shape=(n, n))
    a.sort_indices()
    return dict(node_off=torch.tensor([0, n]), row_ptr=torch.from_numpy(a.indptr.astype(np.int64)),
                col_idx=torch.from_numpy(a.indices.astype(np.int64)))


def _csr_view(a):
    a.sort_indices()
    return dict(node_off=torch.tensor([0, a.shape[0]]), row_ptr=torch.from_numpy(a.indptr.astype(np.int64)),
                col_idx=torch.from_numpy(a.indices.astype(np.int64)))


def _ring_edges(n, p, rng, off=0):
    """a cycle (a path for n < 3) plus every other pair with probability p: connected, and no leaf for n >= 3"""
    if n == 1:
        return []
    edges = [(off + i, off + (i + 1) % n) for i in range(n if n >= 3 else n - 1)]
    edges += [(off + i, off + j) for i in range(n) for j in range(i + 1, n) if rng.rand() < p]
    return edges


def spectrum(view):
    """float64 eigh of the (one-item) view's normalised adjacency -> (ascending eigenvalues, eigenvectors)"""
    rp, ci = view["row_ptr"].numpy(), view["col_idx"].numpy()
    return _dense_eigh(P.normalized_adjacency(rp, ci).toarray())


def gram_applies(view, h):
    """float64's word on _check's ``gap_ok`` for a one-item view at width h (False where k <= 0: nothing is compared)"""
    n = int(view["node_off"][-1])
    k = min(n - 2, h)
    if k <= 0:
        return False
    s = spectrum(view)[0]
    return bool(n - k - 1 < 0 or s[-k] - s[-k - 1] > GAP)


def _first_seed(build, ok, seed):
    for t in range(50):
        v = build(np.random.RandomState(seed + 100 * t))
        if ok(v):
            return v
    raise AssertionError("no seed in 50 meets the float64 conditions")


def connected_item(n, p, seed, widths):
    """a connected random graph whose wanted subspace is unique (float64) at every width of ``widths``"""
    return _first_seed(lambda rng: _view(n, _ring_edges(n, p, rng)),
                       lambda v: all(gram_applies(v, h) or min(n - 2, h) <= 0 for h in widths), seed)


def disconnected_item(parts, isolated, p, seed, widths):
    """components of ``parts`` nodes (random, connected; 2 -> K2, 3 -> a path) followed by ``isolated`` nodes of degree 0"""
    def build(rng):
        edges, off = [], 0
        for m in parts:
            edges += [(off, off + 1), (off + 1, off + 2)] if m == 3 else _ring_edges(m, p, rng, off)
            off += m
        return _view(off + isolated, edges)
    return _first_seed(build, lambda v: all(gram_applies(v, h) for h in widths), seed)


def _tiny(name):
    rp, ci = tiny_graphs()[name]
    return dict(node_off=torch.tensor([0, len(rp) - 1]), row_ptr=torch.from_numpy(np.asarray(rp, dtype=np.int64)),
                col_idx=torch.from_numpy(np.asarray(ci, dtype=np.int64)))


_ITEMS = {}


def fixed_items():
    """the items that do not depend on the width, by name (built once, never modified)"""
    if not _ITEMS:
        import scipy.sparse as sp

        w = [h for h in WIDTHS]
        _ITEMS["wave40"] = connected_item(40, 0.12, 40, w)
        _ITEMS["wave60"] = connected_item(60, 0.08, 60, w)
        _ITEMS["mid110"] = connected_item(110, 0.04, 110, w)
        _ITEMS["sparse160"] = connected_item(160, 0.03, 160, w)
        _ITEMS["star40"] = _view(40, [(0, i) for i in range(1, 40)])
        _ITEMS["k4"] = _tiny("k4")
        _ITEMS["path5"] = _tiny("path5")
        # eigenvalue 1 three times: at width 2 the cut runs through it whatever the seed (UNMARKED)
        _ITEMS["iso40"] = disconnected_item((20, 15, 2), 3, 0.2, 1040, [h for h in w if h > 2])
        _ITEMS["two70"] = disconnected_item((40, 30), 0, 0.12, 1070, w)
        _ITEMS["iso155"] = disconnected_item((90, 60, 3), 2, 0.04, 1155, [h for h in w if h > 2])
        _ITEMS["free5"] = _view(5, [])
        _ITEMS["big400"] = _csr_view(skewed_dense_graph(400, seed=2))
        _ITEMS["kry760"] = _csr_view(skewed_dense_graph(760))
        _ITEMS["iso763"] = _csr_view(sp.block_diag([skewed_dense_graph(760), sp.csr_matrix((3, 3))], format="csr"))
        rng = np.random.RandomState(763)
        comm = np.arange(760) // 95
        up = np.triu(rng.rand(760, 760) < np.where(comm[:, None] == comm[None, :], 0.5, 0.01), 1)
        up[np.arange(759), np.arange(1, 760)] = True                  # connected
        _ITEMS["comm763"] = _csr_view(sp.block_diag([sp.csr_matrix((up | up.T).astype(np.float64)), sp.csr_matrix((3, 3))],
                                                    format="csr"))
    return _ITEMS


_KEDGE = {}


def kedge_items(h):
    """n = 1, 2, 3, h + 1, h + 2, h + 3: zeros, zeros, k = 1, k = h - 1 (one padding column), k = h = n - 2, k = h < n - 2"""
    if h not in _KEDGE:
        out = {}
        for n in (1, 2, 3, h + 1, h + 2, h + 3):
            out.setdefault("n%d" % n, connected_item(n, 0.3, 7000 + 10 * h + n, (h,)))
        _KEDGE[h] = out
    return _KEDGE[h]


CLASS_ITEMS = ("wave40", "wave60", "mid110", "sparse160")
DEGENERATE = ("star40", "k4", "path5")
DISCONNECTED = ("iso40", "two70", "iso155", "free5")
HEAVY = ("big400", "kry760", "iso763", "comm763")
KRYLOV = ("kry760", "iso763", "comm763")
WITH_ISOLATED = ("iso40", "iso155", "iso763", "comm763")
ISOLATED_NODES = {"iso40": 3, "iso155": 2, "iso763": 3, "comm763": 3, "free5": 5}

# (item, width) pairs where float64 says the Gram comparison does NOT apply, with the reason.  Everything else that takes the
# strict checker must be compared (test_cases_cpu_only pins both directions).
UNMARKED = {
    "star40": "eigenvalue 0 has multiplicity 38: every cut k >= 2 runs through it",
    "k4": "eigenvalue -1/3 three times, k = 2 takes one of them",
    "free5": "M = 0",
    "n1": "k <= 0: zeros", "n2": "k <= 0: zeros",
}
UNMARKED_AT = {("iso40", 2): "eigenvalue 1 three times (three components with edges), k = 2 takes two of them",
               ("iso155", 2): "eigenvalue 1 three times (three components with edges), k = 2 takes two of them"}


BIG400_MARKED = (2, 31)                      # float64: s[-k] - s[-k-1] > GAP at these widths only


def expected_marked(name, h):
    if h == 2 and name == "n2":              # (at width 2, "n2" is an item of two nodes: k <= 0)
        return False
    if name == "big400":                     # (a fixed graph: gaps of 2.4e-4 .. 2.5e-3 below its top eigenvalues)
        return h in BIG400_MARKED
    return name not in UNMARKED and (name, h) not in UNMARKED_AT and name not in KRYLOV


def solver_class(nr, n, knobs=()):
    """posemb_classify_kernel's rule: deflated size nr, n nodes, environment knobs -> the class an item is listed in first"""
    k = dict(knobs)
    wave, pair, cheb = (k.get("GCC_POSEMB_" + x, "1") != "0" for x in ("WAVE", "PAIR", "CHEB"))
    if n <= 2:
        return "zeros"
    if n > 1024:
        return "krylov"
    if wave and nr <= 64 and n <= 256:
        return "w48" if nr <= 48 else "w64"
    if nr <= 64:
        return "small"
    if nr <= 128:
        return "pair" if pair else "mid"
    if cheb:
        return "block"
    return "slot" if nr <= SLOT_MAX else "big" if nr <= DIRECT_MAX else "krylov"


def batch(named):
    """{name: one-item view} -> (names in order, one batched view)"""
    import scipy.sparse as sp

    names = list(named)
    mats, node_off = [], [0]
    for nm in names:
        v = named[nm]
        n = int(v["node_off"][-1])
        mats.append(sp.csr_matrix((np.ones(len(v["col_idx"])), v["col_idx"].numpy(), v["row_ptr"].numpy()), shape=(n, n)))
        node_off.append(node_off[-1] + n)
    a = sp.block_diag(mats, format="csr")
    a.sort_indices()
    return names, dict(node_off=torch.tensor(node_off), row_ptr=torch.from_numpy(a.indptr.astype(np.int64)),
                       col_idx=torch.from_numpy(a.indices.astype(np.int64)))


def width_items(h, heavy=False, only=None):
    """the named items of width h (``heavy``: with the 385..704 and Krylov items; ``only``: a subset by name)"""
    named = dict(kedge_items(h))
    f = fixed_items()
    for nm in CLASS_ITEMS + DEGENERATE + DISCONNECTED + (HEAVY if heavy else ()):
        named[nm] = f[nm]
    if only is not None:
        named = {nm: named[nm] for nm in only}
    return named


# ------------------------------------------------------------------------------------------- assertions on the cases themselves
def wanted_min(view, h):
    n = int(view["node_off"][-1])
    return float(spectrum(view)[0][-min(n - 2, h)])


# where float64 says EVERY wanted eigenvalue of an item with isolated nodes exceeds ISO_EIG (check_cases pins the list: the
# narrow widths, where the cut stays far above the null space; the wider cuts of iso40 and iso155 reach it)
ISO_WHOLE_ROWS = {"iso40": (2, 5, 6), "iso155": (2, 5, 6, 16, 17, 30, 31, 32), "iso763": (), "comm763": (2, 5, 6, 16, 17, 30, 31, 32)}


def check_cases():
    """The CPU-only part: the class every item reaches under every knob setting, the Gram-eligible set, the isolated-node
    condition.  float64 and the classify rule only."""
    f = fixed_items()
    red = {nm: int(reduced_sizes(v)[0]) for nm, v in f.items()}
    n = {nm: int(v["node_off"][-1]) for nm, v in f.items()}
    cls = {nm: {kn: solver_class(red[nm], n[nm], kv) for kn, kv in KNOBS.items()} for nm in f}
    assert cls["wave40"] == dict(default="w48", wave0="small", pair0="w48", cheb0="w48"), cls["wave40"]
    assert cls["wave60"] == dict(default="w64", wave0="small", pair0="w64", cheb0="w64"), cls["wave60"]
    assert cls["mid110"] == dict(default="pair", wave0="pair", pair0="mid", cheb0="pair"), cls["mid110"]
    assert cls["sparse160"] == dict(default="block", wave0="block", pair0="block", cheb0="slot"), cls["sparse160"]
    assert cls["big400"]["cheb0"] == "big" and all(cls[nm]["cheb0"] == "krylov" for nm in KRYLOV)
    assert cls["iso40"] == cls["wave40"] and cls["two70"] == cls["mid110"] and cls["iso155"] == cls["sparse160"]
    assert cls["free5"]["default"] == cls["star40"]["default"] == "w48" and cls["free5"]["wave0"] == "small"
    # with the block class on, the three dense items are listed there first and handed on: too many edges for its LDS list
    for nm in HEAVY:
        assert cls[nm]["default"] == "block" and len(f[nm]["col_idx"]) > BLOCK_EDGES, nm
    for nm in ("sparse160", "iso155"):
        assert len(f[nm]["col_idx"]) <= BLOCK_EDGES
    # components and isolated nodes
    for nm, comps, iso in (("iso40", 3, 3), ("two70", 2, 0), ("iso155", 3, 2), ("iso763", 1, 3), ("comm763", 1, 3),
                           ("free5", 0, 5)):
        deg = np.diff(f[nm]["row_ptr"].numpy())
        s = spectrum(f[nm])[0]
        assert int((deg == 0).sum()) == iso and int((np.abs(s - 1) < 1e-9).sum()) == comps, (nm, s[-4:])
    assert not spectrum(f["free5"])[0].any()
    # the Gram-eligible set, both directions
    assert gram_applies(f["big400"], EMU_BIG_WIDTH) == expected_marked("big400", EMU_BIG_WIDTH)
    for h in WIDTHS:
        for nm, v in width_items(h, heavy=True).items():
            if nm not in KRYLOV:                        # (Krylov invariants: no Gram comparison on that path)
                assert gram_applies(v, h) == expected_marked(nm, h), (nm, h)
        for nm in CLASS_ITEMS + ("two70", "path5") + tuple(k for k in kedge_items(h) if k not in ("n1", "n2")):
            assert expected_marked(nm, h), (nm, h)
        for nm in ("iso40", "iso155"):
            assert expected_marked(nm, h) == (h > 2)
        sizes = sorted(int(v["node_off"][-1]) for v in kedge_items(h).values())
        assert sizes == sorted({1, 2, 3, h + 1, h + 2, h + 3})
    # the isolated-node rule's condition
    for nm in WITH_ISOLATED:
        whole = tuple(h for h in sorted(WIDTHS + (EMU_BIG_WIDTH,)) if wanted_min(f[nm], h) > ISO_EIG)
        assert whole == ISO_WHOLE_ROWS[nm], (nm, whole, [round(wanted_min(f[nm], h), 4) for h in WIDTHS])
        assert nm == "iso763" or {2, 5, EMU_BIG_WIDTH}.issubset(whole)
    assert 0.09 < spectrum(f["iso763"])[0][-2] < ISO_EIG          # (why the bar binds one column of iso763 only)


# ------------------------------------------------------------------------------------------------------------------ the runner
class Knobs:
    """sets a KNOBS entry's environment variables for the duration of a call (posemb.hip reads them per call)"""

    def __init__(self, knob):
        self.env = KNOBS[knob]

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in ("GCC_POSEMB_WAVE", "GCC_POSEMB_PAIR", "GCC_POSEMB_CHEB")}
        for k in self.old:
            os.environ.pop(k, None)
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def node_capacity(view):
    """the Krylov class sizes its vectors as node_cap / batch_size; at least SPARE rows beyond node_off[B]"""
    sizes = np.diff(view["node_off"].numpy())
    cap = max(len(sizes) * (int(sizes.max()) + 1), int(sizes.sum()) + SPARE)
    assert cap >= int(sizes.sum()) + SPARE
    return cap


def run_filled(view, hid, make_batch, make_pe):
    """One call into buffers that hold SENTINEL.  ``make_batch(view, cap, hid)`` -> the batch object, ``make_pe(B, cap, hid)`` ->
    a DevicePosEmb with num_buffers=1.  Asserts what was and was not written -> (x, evals, raw, status words)."""
    B, N = len(view["node_off"]) - 1, int(view["node_off"][-1])
    cap = node_capacity(view)
    g = make_batch(view, cap, hid)
    pe = make_pe(B, cap, hid)
    dev = pe.status.device
    for t in pe._ring:
        assert t.shape == (cap, hid)
        t.fill_(SENTINEL)
    evals = torch.full((B + 4, hid), SENTINEL, device=dev)
    raw = torch.full((cap, hid), SENTINEL, device=dev)
    pe(g, evals=evals, raw=raw)
    if dev.type == "cuda":
        pe.check_status(strict=True)
    status = [int(v) for v in pe.status.cpu()]
    assert status[0] == 0, status
    out = g.pos_undirected
    assert out.data_ptr() == pe._ring[0].data_ptr()
    x, ev, rw = out.cpu().numpy(), evals.cpu().numpy(), raw.cpu().numpy()
    for t in pe._ring[1:]:
        assert bool((t == SENTINEL).all()), "a ring tensor the call was not given has been written"
    assert (x[N:] == SENTINEL).all() and (rw[N:] == SENTINEL).all(), "a row >= node_off[B] has been written"
    assert (ev[B:] == SENTINEL).all(), "an evals row >= B has been written"
    for name, t in (("pos", x[:N]), ("raw", rw[:N]), ("evals", ev[:B])):
        left = np.argwhere(t == SENTINEL)
        assert len(left) == 0, "%s: %d cells never written, first (row, column) %s" % (name, len(left), left[0])
    no = view["node_off"].numpy()
    for b in range(B):
        lo, hi = int(no[b]), int(no[b + 1])
        k = max(min(hi - lo - 2, hid), 0)
        assert not x[lo:hi, k:].any(), "pos: padding columns of item %d are not zero" % b
        assert not rw[lo:hi, k:].any(), "raw: padding columns of item %d are not zero" % b
        assert not ev[b, k:].any(), "evals: padding columns of item %d are not zero" % b
    return x[:N], ev[:B], rw[:N], status


def check_isolated(sub, x, raw, hid, whole):
    """the isolated-node rule on a one-item view: exact zeros in the columns of |float64 eigenvalue| > ISO_EIG; ``whole``:
    float64 says that is every wanted column (ISO_WHOLE_ROWS), so the rows are zero altogether -> number of isolated nodes"""
    n = int(sub["node_off"][-1])
    k = min(n - 2, hid)
    iso = np.where(np.diff(sub["row_ptr"].numpy()) == 0)[0]
    if k <= 0 or len(iso) == 0:
        return 0
    s = spectrum(sub)[0][-k:]                              # column c holds eigenvalue s[c] (ascending, _check / _check_krylov)
    cols = np.where(np.abs(s) > ISO_EIG)[0]
    assert whole == (len(cols) == k)
    norms = [float(np.linalg.norm(x[i, :k])) for i in iso]
    print("isolated nodes: |pos row| %s |raw row| %s" % (norms, [float(np.linalg.norm(raw[i, :k])) for i in iso]))
    assert not raw[np.ix_(iso, cols)].any(), "raw: entries of degree-0 nodes in columns of non-zero eigenvalue, |pos row| = %s" % norms
    assert not x[np.ix_(iso, cols)].any(), "pos: entries of degree-0 nodes in columns of non-zero eigenvalue, |pos row| = %s" % norms
    if whole:
        assert not x[iso].any() and not raw[iso].any(), "|pos row| = %s where 0 is required" % norms
    return len(iso)


def check_batch(names, view, hid, x, evals, raw):
    """the isolated-node rule (first: it is the sharper statement about a degree-0 row; the Gram comparison against the
    tightened float64 rows would only report the same row as a difference of 1), then strict / Krylov invariants by path and the
    Gram set"""
    for b, nm in enumerate(names):
        if nm in ISOLATED_NODES:
            lo, hi, sub = _sub(view, b)
            cnt = check_isolated(sub, x[lo:hi], raw[lo:hi], hid, nm in ISO_WHOLE_ROWS and hid in ISO_WHOLE_ROWS[nm])
            assert cnt == ISOLATED_NODES[nm]
    gram = []
    check_by_path(view, x, evals, raw, hid=hid, gram=gram)
    assert sorted(names[b] for b in gram) == sorted(nm for nm in names if expected_marked(nm, hid)), \
        "the Gram comparison ran on %s" % [names[b] for b in gram]


def expected_status(names, view, knob, status):
    """status words 2 (Arnoldi steps: the Krylov class ran) and 3 (items the block class handed on)"""
    red = reduced_sizes(view)
    sizes = np.diff(view["node_off"].numpy())
    cls = [solver_class(int(r), int(n), KNOBS[knob]) for r, n in zip(red, sizes)]
    handed = sum(1 for nm, c in zip(names, cls) if c == "block" and nm in HEAVY)
    krylov = any(nm in KRYLOV for nm in names)
    assert status[3] == handed, (status, cls)
    assert (status[2] > 0) == krylov, status
    return cls
