// gcc_amd/csrc/svc.hip -- C-SVC with an RBF kernel on frozen embeddings, every fold of a cross-validation in one call (gfx950).
//
// Replaces the fit / predict loop of GraphClassification.svc_classify (gcc/tasks/graph_classification.py:47-64 of the reference:
// StratifiedKFold, sklearn.svm.SVC(C=100000) per fold, i.e. libsvm's one-vs-one C-SVC).  The solver is the SMO of Fan, Chen and
// Lin (2005) with the second-order working-set choice (WSS 2), restated from the paper; no shrinking, no probability estimates.
//
//   svc_d2_kernel        64 x 64 tiles of d2[i, j] = sum_c (x_i[c] - x_j[c])^2: the differences themselves, one fmaf chain over
//       c = 0 .. D-1 per entry, so d2[i, j] and d2[j, i] are the same chain on negated differences (bitwise equal) and the
//       diagonal is exactly 0.  Flags non-finite embeddings.
//   svc_setup_kernel     one wave per row list (fold f, class pair ci < cj): the fold's training rows of the two classes in
//       libsvm's order (class ci's rows ascending, then class cj's), alpha = 0, G = -1; checks labels and fold ids.
//   svc_smo_kernel<W>    one workgroup of W waves per problem, alpha and G (float64) in LDS.  An iteration is two selections
//       (i = argmax over I_up of -y G; j = argmax over I_low of b^2 / a), each a wave butterfly under the total order (key
//       descending, row ascending) and one LDS slot per wave, the clipped two-variable update, and the gradient update from
//       the two kernel rows, formed as (float)exp(-gamma_f * d2) while the rows of the shared matrix are read.  The launch
//       runs at most `budget` iterations per problem, keeps alpha / G / the count in the workspace and counts the problems
//       that are not finished; a finished problem gets rho, its dual objective and its support-vector counts.
//   svc_predict_kernel   one workgroup per corpus row: for each class pair of the row's own fold, sum_t alpha_t y_t K(t, r) - rho
//       in float64 (one wave per pair, lanes strided, fixed order), then libsvm's vote (pairs in (i < j) order, ties to the
//       lowest class).
//   svc_score_kernel     the grid search: one workgroup per (corpus row, outer fold other than the row's own); the row's vote under
//       every candidate C from the problems of its inner fold (svc_predict_kernel's sum and vote), counted into correct[o, c, i]
//       with integer atomics.
// A problem is (fold, inner fold or none, class pair, candidate): problems p = g * cands + c of one row list g = (fold * ninner +
// inner) * pairs + pair share the list and differ in C; the plain call and the search's refit have ninner = cands = 1, so p = g =
// fold * pairs + pair.  gcc_svc_search_* solves the folds * inner * pairs * candidates problems of sklearn's
// GridSearchCV(SVC(), {"C": ...}, cv=inner) side by side over the one distance matrix, then the refit at each fold's winner.
// The entry points' scaffold (workspace carving, the NULL and workspace checks) is task_common.h's.
#include "task_common.h"

#include <float.h>
#include <math.h>

namespace {

constexpr int kTile = 64, kKc = 32, kD2Threads = 256;
constexpr int kPredictWaves = 4;
constexpr int kOneWaveRows = 512;             // problems up to this many rows run in one wave (no workgroup barrier at all)
constexpr double kTau = 1e-12;
enum { kRunning = 0, kConverged = 1, kCapped = 2, kSkipped = 3 };

struct SvcDev {
    const float *emb;
    long long ld;
    const int32_t *labels, *fold;
    const int32_t *inner;                     // [folds][N] the inner fold of a row on the fold's training side, or NULL (no inner folds)
    const double *gamma;                      // [folds * ninner]
    const double *Cs, *Cf;                    // [cands] the candidates' C / [folds] one C per fold; both NULL: C
    int32_t N, D, classes, folds, ninner, cands, pairs, groups, P, cap, budget, iter_cap;
    double C, eps;
    float *d2;                                // [N][N]
    int32_t *pn, *pni;                        // [groups]: rows, rows of the first class
    int32_t *pdone, *piter;                   // [P]: state, iterations so far
    int32_t *idx;                             // [groups][cap] corpus rows
    double *alpha, *G, *prho;                 // [P][cap], [P][cap], [P]
    int32_t *pred;
    double *decision;
    int32_t *iters;
    double *rho, *obj;
    int32_t *n_free, *n_bounded, *problem_rows, *first_rows, *rows_out;
    double *alpha_out;                        // [P][cap] or NULL; rows_out [groups][cap] or NULL
    int32_t *correct;                         // [folds][cands][ninner], svc_score_kernel
    int32_t *unfinished, *status;
};

// the box bound of problem p of row list g
__device__ __forceinline__ double problem_C(const SvcDev &a, int p, int g)
{
    return a.Cs ? a.Cs[p % a.cands] : a.Cf ? a.Cf[g / a.pairs] : a.C;
}

__global__ __launch_bounds__(kD2Threads) void svc_d2_kernel(SvcDev a)
{
    __shared__ float As[kTile][kKc + 1], Bs[kTile][kKc + 1];
    const int tid = (int)threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int i0 = (int)blockIdx.y * kTile, j0 = (int)blockIdx.x * kTile;
    float acc[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = 0.f;
    bool bad = false;
    for (int c0 = 0; c0 < a.D; c0 += kKc) {
        for (int e = tid; e < kTile * kKc; e += kD2Threads) {
            const int r = e / kKc, c = e % kKc;
            const bool cin = c0 + c < a.D;
            const float va = cin && i0 + r < a.N ? a.emb[(long long)(i0 + r) * a.ld + c0 + c] : 0.f;
            const float vb = cin && j0 + r < a.N ? a.emb[(long long)(j0 + r) * a.ld + c0 + c] : 0.f;
            bad |= !(fabsf(va) <= FLT_MAX);                      // (every row is the A side of the tiles of column 0)
            As[r][c] = va;
            Bs[r][c] = vb;
        }
        __syncthreads();
        for (int c = 0; c < kKc; ++c) {                             // columns past D hold zeros on both sides: fmaf(0, 0, acc) = acc
            float av[4], bv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { av[u] = As[ty * 4 + u][c]; bv[u] = Bs[tx * 4 + u][c]; }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const float d = av[u] - bv[v];
                    acc[u][v] = fmaf(d, d, acc[u][v]);
                }
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int i = i0 + ty * 4 + u, j = j0 + tx * 4 + v;
            if (i < a.N && j < a.N) a.d2[(long long)i * a.N + j] = acc[u][v];
        }
    if (bad) atomicOr(a.status, (int32_t)GCC_STATUS_SVC_NONFINITE);
}

// pair index -> (ci < cj) in libsvm's order (0,1), (0,2), ..., (1,2), ...
__device__ __forceinline__ void pair_classes(int pair, int classes, int &ci, int &cj)
{
    ci = 0;
    for (int c = 0; c < classes - 1; ++c) {
        const int width = classes - 1 - c;
        if (pair < width) { ci = c; break; }
        pair -= width;
    }
    cj = ci + 1 + pair;
}

// row r on the side of (fold f, inner fold in): 1 = trains, 2 = held out, 0 = neither.  Without inner folds the held-out side is
// the fold's own rows; with them it is the rows of the fold's training side whose inner fold is `in`.
__device__ __forceinline__ int row_side(const SvcDev &a, const int32_t *inner, int f, int in, int r, int fo)
{
    if (r >= a.N || fo < 0 || fo >= a.folds) return 0;
    if (!inner) return fo != f ? 1 : 2;
    if (fo == f) return 0;
    return inner[r] != in ? 1 : 2;
}

__global__ __launch_bounds__(64) void svc_setup_kernel(SvcDev a)
{
    const int g = (int)blockIdx.x, lane = lane_id();
    const int fi = g / a.pairs, f = fi / a.ninner, in = fi % a.ninner;
    const int32_t *inner = a.inner ? a.inner + (long long)f * a.N : nullptr;
    int ci, cj;
    pair_classes(g % a.pairs, a.classes, ci, cj);
    int ni = 0, nj = 0, ti = 0, tj = 0, bits = 0;
    for (int r0 = 0; r0 < a.N; r0 += 64) {
        const int r = r0 + lane;
        const int lab = r < a.N ? a.labels[r] : -1, fo = r < a.N ? a.fold[r] : -1;
        if (wave_ballot(r < a.N && (lab < 0 || lab >= a.classes))) bits |= GCC_STATUS_SVC_BAD_LABEL;     // (bits: wave-uniform)
        if (wave_ballot(r < a.N && (fo < 0 || fo >= a.folds))) bits |= GCC_STATUS_SVC_BAD_FOLD;
        const int side = row_side(a, inner, f, in, r, fo);
        if (wave_ballot(inner && side != 0 && (inner[r] < 0 || inner[r] >= a.ninner))) bits |= GCC_STATUS_SVC_BAD_FOLD;
        ni += __popcll(wave_ballot(side == 1 && lab == ci));
        nj += __popcll(wave_ballot(side == 1 && lab == cj));
        ti += __popcll(wave_ballot(side == 2 && lab == ci));
        tj += __popcll(wave_ballot(side == 2 && lab == cj));
    }
    if ((ni == 0 && ti > 0) || (nj == 0 && tj > 0)) bits |= GCC_STATUS_SVC_MISSING_CLASS;
    const int n = ni + nj;
    const bool fits = n <= a.cap;
    if (!fits) bits |= GCC_STATUS_SVC_OVERFLOW;                     // (the workspace was sized for smaller problems: nothing written)
    const bool solve = fits && ni > 0 && nj > 0;
    const long long gbase = (long long)g * a.cap;
    if (solve) {
        int bi = 0, bj = ni;
        for (int r0 = 0; r0 < a.N; r0 += 64) {
            const int r = r0 + lane;
            const int lab = r < a.N ? a.labels[r] : -1, fo = r < a.N ? a.fold[r] : -1;
            const bool train = row_side(a, inner, f, in, r, fo) == 1;
            const unsigned long long mi = wave_ballot(train && lab == ci), mj = wave_ballot(train && lab == cj);
            const long long at = gbase + (lab == ci ? bi + __popcll(mi & lanemask_lt()) : bj + __popcll(mj & lanemask_lt()));
            if (train && (lab == ci || lab == cj)) {
                a.idx[at] = r;
                if (a.rows_out) a.rows_out[at] = r;
            }
            bi += __popcll(mi);
            bj += __popcll(mj);
        }
    }
    for (int c = 0; c < a.cands; ++c) {                             // the problems of the row list: cold starts
        const int p = g * a.cands + c;
        const long long base = (long long)p * a.cap;
        if (solve)
            for (int t = lane; t < n; t += 64) { a.alpha[base + t] = 0.0; a.G[base + t] = -1.0; }
        if (lane == 0) {
            a.pdone[p] = solve ? kRunning : kSkipped;
            a.piter[p] = 0;
            a.prho[p] = 0.0;
            if (a.iters) a.iters[p] = 0;
            if (a.rho) a.rho[p] = 0.0;
            if (a.obj) a.obj[p] = 0.0;
            if (a.n_free) a.n_free[p] = 0;
            if (a.n_bounded) a.n_bounded[p] = 0;
        }
    }
    if (lane == 0) {
        a.pn[g] = solve ? n : 0;
        a.pni[g] = solve ? ni : 0;
        if (a.problem_rows) a.problem_rows[g] = n;
        if (a.first_rows) a.first_rows[g] = ni;
        if (bits) atomicOr(a.status, (int32_t)bits);
    }
}

// candidate a comes before candidate b: key descending, then row ascending; the empty candidate (-inf, -1) comes last
__device__ __forceinline__ bool better(double ka, int ia, double kb, int ib)
{
    return ka > kb || (ka == kb && (uint32_t)ia < (uint32_t)ib);
}
__device__ __forceinline__ void wave_best(double &k, int &i)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double ok = wave_shfl_xor(k, d);
        const int oi = wave_shfl_xor(i, d);
        if (better(ok, oi, k, i)) { k = ok; i = oi; }
    }
}
__device__ __forceinline__ double wave_max_f64(double v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const double o = wave_shfl_xor(v, d); v = o > v ? o : v; }
    return v;
}
__device__ __forceinline__ double wave_min_f64(double v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const double o = wave_shfl_xor(v, d); v = o < v ? o : v; }
    return v;
}

struct Slot1 { double key, alpha; int32_t idx, pad; };
struct Slot2 { double key, alpha, g; float q; int32_t idx; };

template <int kWaves> __device__ __forceinline__ void block_sync()
{
    if (kWaves == 1) wave_sync();
    else __syncthreads();
}
// op 0: sum, 1: max, 2: min -- wave butterfly, then the waves' values in wave order
template <int kWaves, int kOp> __device__ __forceinline__ double block_reduce(double v, double *red)
{
    v = kOp == 0 ? wave_sum(v) : kOp == 1 ? wave_max_f64(v) : wave_min_f64(v);
    if (kWaves == 1) return v;
    if (lane_id() == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = red[0];
    for (int w = 1; w < kWaves; ++w) r = kOp == 0 ? r + red[w] : kOp == 1 ? (red[w] > r ? red[w] : r) : (red[w] < r ? red[w] : r);
    __syncthreads();
    return r;
}

__host__ __device__ inline size_t smo_lds_bytes(int waves, int cap)
{
    return (size_t)cap * 24 + (size_t)waves * (sizeof(Slot1) + sizeof(Slot2) + 16);
}

template <int kWaves>
__global__ __launch_bounds__(64 * kWaves) void svc_smo_kernel(SvcDev a)
{
    constexpr int T = 64 * kWaves;
    DYN_SMEM(smem);
    const int cap = a.cap;
    double *alpha_s = reinterpret_cast<double *>(smem);            // [cap]
    double *G_s = alpha_s + cap;                                    // [cap]
    Slot1 *s1 = reinterpret_cast<Slot1 *>(G_s + cap);               // [kWaves] the waves' candidates for i
    Slot2 *s2 = reinterpret_cast<Slot2 *>(s1 + kWaves);             // [kWaves] ... for j
    double *gm2_s = reinterpret_cast<double *>(s2 + kWaves);        // [kWaves] the waves' max over I_low of y G
    double *red = gm2_s + kWaves;                                   // [kWaves]
    float *Qi_s = reinterpret_cast<float *>(red + kWaves);          // [cap] y_i y_t K(i, t) of this iteration's i
    int32_t *idx_s = reinterpret_cast<int32_t *>(Qi_s + cap);       // [cap]
    const int p = (int)blockIdx.x, tid = (int)threadIdx.x, lane = lane_id(), wv = tid >> 6;
    if (a.pdone[p] != kRunning) return;                             // (the whole workgroup)
    const int g = p / a.cands;                                      // the problem's row list
    const int n = a.pn[g], ni = a.pni[g], iter0 = a.piter[p];
    const double gamma = a.gamma[g / a.pairs], C = problem_C(a, p, g), eps = a.eps;
    const long long base = (long long)p * cap, gbase = (long long)g * cap;
    for (int t = tid; t < n; t += T) {
        alpha_s[t] = a.alpha[base + t];
        G_s[t] = a.G[base + t];
        idx_s[t] = a.idx[gbase + t];
    }
    block_sync<kWaves>();                                           // idx_s of the selected rows is read by every thread
    // libsvm's cap: max(10^7, 100 n) iterations, unless the caller passes its own
    const int cap_it = a.iter_cap > 0 ? a.iter_cap : (n > 100000 ? 100 * n : 10000000);
    const int budget = min(a.budget, cap_it - iter0);
    bool converged = false;
    int it = 0;
    for (; it < budget; ++it) {
        // ---- i = argmax over I_up of -y G (row t is thread t % T's: alpha_s, G_s, Qi_s entries have one reader and writer)
        double best = -INFINITY;
        int bi = -1;
        for (int t = tid; t < n; t += T) {
            const double al = alpha_s[t], g = G_s[t];
            const bool pos = t < ni;
            if (pos ? al < C : al > 0.0) {
                const double v = pos ? -g : g;
                if (v > best) { best = v; bi = t; }
            }
        }
        wave_best(best, bi);
        if (bi >= 0 ? (bi % T) == tid : lane == 0) {
            Slot1 s = {best, bi >= 0 ? alpha_s[bi] : 0.0, bi, 0};
            s1[wv] = s;
        }
        block_sync<kWaves>();
        double Gmax = s1[0].key, ai = s1[0].alpha;
        int i = s1[0].idx;
        for (int w = 1; w < kWaves; ++w)
            if (better(s1[w].key, s1[w].idx, Gmax, i)) { Gmax = s1[w].key; ai = s1[w].alpha; i = s1[w].idx; }
        if (i < 0) { converged = true; break; }                     // I_up is empty (workgroup-uniform)
        const bool ipos = i < ni;
        const double Gi = ipos ? -Gmax : Gmax;
        const float *rowi = a.d2 + (long long)idx_s[i] * a.N;
        // ---- j = argmin over I_low, b > 0, of -b^2 / a (a = K_ii + K_tt - 2 K_it = 2 - 2 K_it; a <= 0 -> tau), and max over I_low of y G
        double bestj = -INFINITY, gm2 = -INFINITY;
        int bj = -1;
        for (int t = tid; t < n; t += T) {
            const float kit = (float)exp(-gamma * (double)rowi[idx_s[t]]);
            const bool pos = t < ni;
            Qi_s[t] = pos == ipos ? kit : -kit;
            const double al = alpha_s[t], g = G_s[t];
            if (pos ? al > 0.0 : al < C) {
                const double yg = pos ? g : -g;
                gm2 = yg > gm2 ? yg : gm2;
                const double b = Gmax + yg;
                if (b > 0.0) {
                    double quad = 2.0 - 2.0 * (double)kit;
                    if (!(quad > 0.0)) quad = kTau;
                    const double key = b * b / quad;
                    if (key > bestj) { bestj = key; bj = t; }
                }
            }
        }
        wave_best(bestj, bj);
        gm2 = wave_max_f64(gm2);
        if (bj >= 0 ? (bj % T) == tid : lane == 0) {
            Slot2 s = {bestj, bj >= 0 ? alpha_s[bj] : 0.0, bj >= 0 ? G_s[bj] : 0.0, bj >= 0 ? Qi_s[bj] : 0.f, bj};
            s2[wv] = s;
        }
        if (lane == 0) gm2_s[wv] = gm2;
        block_sync<kWaves>();
        int j = s2[0].idx, jw = 0;
        double keyj = s2[0].key, Gmax2 = gm2_s[0];
        for (int w = 1; w < kWaves; ++w) {
            if (better(s2[w].key, s2[w].idx, keyj, j)) { keyj = s2[w].key; j = s2[w].idx; jw = w; }
            Gmax2 = gm2_s[w] > Gmax2 ? gm2_s[w] : Gmax2;
        }
        if (Gmax + Gmax2 < eps || j < 0) { converged = true; break; }
        const double aj = s2[jw].alpha, Gj = s2[jw].g, Qij = (double)s2[jw].q;
        const bool jpos = j < ni;
        // ---- the two-variable update with libsvm's clipping to the box [0, C]^2
        double ai_new = ai, aj_new = aj;
        if (ipos != jpos) {
            double quad = 2.0 + 2.0 * Qij;
            if (!(quad > 0.0)) quad = kTau;
            const double delta = (-Gi - Gj) / quad, diff = ai - aj;
            ai_new += delta;
            aj_new += delta;
            if (diff > 0.0) {
                if (aj_new < 0.0) { aj_new = 0.0; ai_new = diff; }
            } else {
                if (ai_new < 0.0) { ai_new = 0.0; aj_new = -diff; }
            }
            if (diff > 0.0) {                                       // (C_i = C_j: diff > C_i - C_j)
                if (ai_new > C) { ai_new = C; aj_new = C - diff; }
            } else {
                if (aj_new > C) { aj_new = C; ai_new = C + diff; }
            }
        } else {
            double quad = 2.0 - 2.0 * Qij;
            if (!(quad > 0.0)) quad = kTau;
            const double delta = (Gi - Gj) / quad, sum = ai + aj;
            ai_new -= delta;
            aj_new += delta;
            if (sum > C) {
                if (ai_new > C) { ai_new = C; aj_new = sum - C; }
            } else {
                if (aj_new < 0.0) { aj_new = 0.0; ai_new = sum; }
            }
            if (sum > C) {
                if (aj_new > C) { aj_new = C; ai_new = sum - C; }
            } else {
                if (ai_new < 0.0) { ai_new = 0.0; aj_new = sum; }
            }
        }
        const double dai = ai_new - ai, daj = aj_new - aj;
        // ---- G += Q_i d alpha_i + Q_j d alpha_j
        const float *rowj = a.d2 + (long long)idx_s[j] * a.N;
        for (int t = tid; t < n; t += T) {
            const float kjt = (float)exp(-gamma * (double)rowj[idx_s[t]]);
            const float qj = (t < ni) == jpos ? kjt : -kjt;
            G_s[t] += (double)Qi_s[t] * dai + (double)qj * daj;
        }
        if ((i % T) == tid) alpha_s[i] = ai_new;
        if ((j % T) == tid) alpha_s[j] = aj_new;
    }
    const int iters = iter0 + it;
    const bool capped = !converged && iters >= cap_it;
    for (int t = tid; t < n; t += T) {
        a.alpha[base + t] = alpha_s[t];
        a.G[base + t] = G_s[t];
    }
    if (!converged && !capped) {
        if (tid == 0) {
            a.piter[p] = iters;
            atomicAdd(a.unfinished, 1);
        }
        return;
    }
    // ---- finished: rho (the mean of y G over the free vectors, else the midpoint of the bounds), the dual objective, counts
    double sum_free = 0.0, n_free = 0.0, ub = INFINITY, lb = -INFINITY, obj = 0.0, n_sv = 0.0, n_bsv = 0.0;
    for (int t = tid; t < n; t += T) {
        const double al = alpha_s[t], g = G_s[t];
        const bool pos = t < ni;
        const double yg = pos ? g : -g;
        if (al >= C) {
            if (pos) lb = yg > lb ? yg : lb;
            else ub = yg < ub ? yg : ub;
        } else if (al <= 0.0) {
            if (pos) ub = yg < ub ? yg : ub;
            else lb = yg > lb ? yg : lb;
        } else {
            n_free += 1.0;
            sum_free += yg;
        }
        obj += al * (g - 1.0);
        n_sv += al > 0.0 ? 1.0 : 0.0;
        n_bsv += al >= C ? 1.0 : 0.0;
    }
    sum_free = block_reduce<kWaves, 0>(sum_free, red);
    n_free = block_reduce<kWaves, 0>(n_free, red);
    ub = block_reduce<kWaves, 2>(ub, red);
    lb = block_reduce<kWaves, 1>(lb, red);
    obj = block_reduce<kWaves, 0>(obj, red);
    n_sv = block_reduce<kWaves, 0>(n_sv, red);
    n_bsv = block_reduce<kWaves, 0>(n_bsv, red);
    if (a.alpha_out)
        for (int t = tid; t < n; t += T) a.alpha_out[base + t] = alpha_s[t];
    if (tid == 0) {
        const double r = n_free > 0.0 ? sum_free / n_free : (ub + lb) / 2.0;
        a.piter[p] = iters;
        a.pdone[p] = converged ? kConverged : kCapped;
        a.prho[p] = r;
        if (a.iters) a.iters[p] = iters;
        if (a.rho) a.rho[p] = r;
        if (a.obj) a.obj[p] = obj / 2.0;
        if (a.n_free) a.n_free[p] = (int32_t)(n_sv - n_bsv);
        if (a.n_bounded) a.n_bounded[p] = (int32_t)n_bsv;
        if (capped) atomicOr(a.status, (int32_t)GCC_STATUS_SVC_ITER_CAP);
    }
}

// sum_t alpha_t y_t K(t, row) - rho of problem p of row list g, `row` = the corpus row's distances: one wave, lanes strided, one
// fixed order (every lane gets the value)
__device__ __forceinline__ double decision_value(const SvcDev &a, int p, int g, const float *row, int lane)
{
    const int n = a.pn[g], ni = a.pni[g];
    const double gamma = a.gamma[g / a.pairs];
    const long long base = (long long)p * a.cap, gbase = (long long)g * a.cap;
    double s = 0.0;
    for (int t = lane; t < n; t += 64) {
        const double al = a.alpha[base + t];
        if (al > 0.0) s += (t < ni ? al : -al) * exp(-gamma * (double)row[a.idx[gbase + t]]);
    }
    return wave_sum(s) - a.prho[p];
}

// libsvm's vote over the solved pairs in (ci < cj) order, ties to the lowest class; -1 without a vote
__device__ __forceinline__ int vote_of(int classes, const double *dec, const int32_t *live)
{
    int votes[GCC_SVC_MAX_CLASSES];
    for (int c = 0; c < classes; ++c) votes[c] = 0;
    int pair = 0, any = 0;
    for (int ci = 0; ci < classes; ++ci)
        for (int cj = ci + 1; cj < classes; ++cj, ++pair)
            if (live[pair]) {
                ++votes[dec[pair] > 0.0 ? ci : cj];
                any = 1;
            }
    int bestc = 0;
    for (int c = 1; c < classes; ++c)
        if (votes[c] > votes[bestc]) bestc = c;
    return any ? bestc : -1;
}

__global__ __launch_bounds__(64 * kPredictWaves) void svc_predict_kernel(SvcDev a)
{
    DYN_SMEM(smem);
    double *dec_s = reinterpret_cast<double *>(smem);               // [pairs]
    int32_t *live_s = reinterpret_cast<int32_t *>(dec_s + a.pairs); // [pairs] 1 = the pair was solved
    const int r = (int)blockIdx.x, tid = (int)threadIdx.x, lane = lane_id(), wv = tid >> 6;
    const int f = a.fold[r];
    const bool served = f >= 0 && f < a.folds;                      // (workgroup-uniform)
    const float *row = a.d2 + (long long)r * a.N;
    for (int pair = wv; pair < a.pairs; pair += kPredictWaves) {
        double dec = 0.0;
        int live = 0;
        if (served) {
            const int p = f * a.pairs + pair;                       // (no inner folds, one candidate: the row list is p too)
            live = a.pdone[p] != kSkipped;
            if (live) dec = decision_value(a, p, p, row, lane);
        }
        if (lane == 0) {
            dec_s[pair] = dec;
            live_s[pair] = live;
            if (a.decision) a.decision[(long long)r * a.pairs + pair] = dec;
        }
    }
    __syncthreads();
    if (tid == 0 && a.pred) a.pred[r] = vote_of(a.classes, dec_s, live_s);
}

// grid (N, folds): row r as a held-out row of outer fold f's inner split -- its vote under every candidate, from the problems that
// left its inner fold out; a right vote adds 1 to correct[f][c][inner fold].  A row of fold f's own test side has no inner fold.
__global__ __launch_bounds__(64 * kPredictWaves) void svc_score_kernel(SvcDev a)
{
    DYN_SMEM(smem);
    const int items = a.cands * a.pairs;
    double *dec_s = reinterpret_cast<double *>(smem);               // [cands][pairs]
    int32_t *live_s = reinterpret_cast<int32_t *>(dec_s + items);   // [cands][pairs]
    const int r = (int)blockIdx.x, f = (int)blockIdx.y, tid = (int)threadIdx.x, lane = lane_id(), wv = tid >> 6;
    const int fo = a.fold[r], lab = a.labels[r];
    if (fo < 0 || fo >= a.folds || fo == f) return;                 // (the whole workgroup, as the next)
    const int in = a.inner[(long long)f * a.N + r];
    if (in < 0 || in >= a.ninner) return;
    const float *row = a.d2 + (long long)r * a.N;
    for (int item = wv; item < items; item += kPredictWaves) {
        const int c = item / a.pairs;
        const int g = (f * a.ninner + in) * a.pairs + item % a.pairs, p = g * a.cands + c;
        const int live = a.pdone[p] != kSkipped;
        const double dec = live ? decision_value(a, p, g, row, lane) : 0.0;
        if (lane == 0) {
            dec_s[item] = dec;
            live_s[item] = live;
        }
    }
    __syncthreads();
    if (tid < a.cands) {
        const int pred = vote_of(a.classes, dec_s + tid * a.pairs, live_s + tid * a.pairs);
        if (pred >= 0 && pred == lab) atomicAdd(a.correct + ((long long)f * a.cands + tid) * a.ninner + in, 1);
    }
}

// the state of a set of problems in the workspace: `groups` row lists of `cap` rows, `P` problems
struct Pieces {
    int32_t groups, P, cap;
    int64_t off_pn, off_pni, off_pdone, off_piter, off_prho, off_idx, off_alpha, off_G;
    void carve(Carve &cv, int32_t groups_, int32_t P_, int32_t max_rows)
    {
        groups = groups_;
        P = P_;
        cap = max_rows < 1 ? 1 : max_rows;
        off_pn = cv.take((int64_t)groups * 4);
        off_pni = cv.take((int64_t)groups * 4);
        off_pdone = cv.take((int64_t)P * 4);
        off_piter = cv.take((int64_t)P * 4);
        off_prho = cv.take((int64_t)P * 8);
        off_idx = cv.take((int64_t)groups * cap * 4);
        off_alpha = cv.take((int64_t)P * cap * 8);
        off_G = cv.take((int64_t)P * cap * 8);
    }
    void bind(SvcDev &d, void *workspace) const
    {
        d.groups = groups; d.P = P; d.cap = cap;
        d.pn = ws_at<int32_t>(workspace, off_pn); d.pni = ws_at<int32_t>(workspace, off_pni);
        d.pdone = ws_at<int32_t>(workspace, off_pdone); d.piter = ws_at<int32_t>(workspace, off_piter);
        d.prho = ws_at<double>(workspace, off_prho); d.idx = ws_at<int32_t>(workspace, off_idx);
        d.alpha = ws_at<double>(workspace, off_alpha); d.G = ws_at<double>(workspace, off_G);
    }
};

struct Plan { int32_t pairs; int64_t off_d2, total; Pieces pc; };

Plan make_plan(int32_t N, int32_t classes, int32_t folds, int32_t max_rows)
{
    Plan p;
    p.pairs = classes * (classes - 1) / 2;
    Carve cv;
    p.off_d2 = cv.take((int64_t)N * N * 4);
    p.pc.carve(cv, folds * p.pairs, folds * p.pairs, max_rows);
    p.total = cv.total();
    return p;
}

// the grid search: the refit's problems (folds * pairs, as the plain call's) and the inner problems
struct SearchPlan { int32_t pairs; int64_t off_d2, total; Pieces refit, inner; };

SearchPlan make_search_plan(int32_t N, int32_t classes, int32_t folds, int32_t inner, int32_t candidates, int32_t max_rows,
                            int32_t max_inner_rows)
{
    SearchPlan p;
    p.pairs = classes * (classes - 1) / 2;
    Carve cv;
    p.off_d2 = cv.take((int64_t)N * N * 4);
    p.refit.carve(cv, folds * p.pairs, folds * p.pairs, max_rows);
    p.inner.carve(cv, folds * inner * p.pairs, folds * inner * p.pairs * candidates, max_inner_rows);
    p.total = cv.total();
    return p;
}

int check_sizes(const char *who, int32_t N, int32_t D, int32_t classes, int32_t folds, int32_t max_rows)
{
    if (N < 1 || N > GCC_SVC_MAX_ROWS) {
        snprintf(g_err, kErrLen, "%s: N %d outside 1..GCC_SVC_MAX_ROWS (%d)", who, N, GCC_SVC_MAX_ROWS);
        return -2;
    }
    if (D < 1 || D > GCC_SVC_MAX_DIM) {
        snprintf(g_err, kErrLen, "%s: D %d outside 1..GCC_SVC_MAX_DIM (%d)", who, D, GCC_SVC_MAX_DIM);
        return -3;
    }
    if (classes < 2 || classes > GCC_SVC_MAX_CLASSES) {
        snprintf(g_err, kErrLen, "%s: classes %d outside 2..GCC_SVC_MAX_CLASSES (%d)", who, classes, GCC_SVC_MAX_CLASSES);
        return -4;
    }
    if (folds < 1 || folds > GCC_SVC_MAX_FOLDS) {
        snprintf(g_err, kErrLen, "%s: folds %d outside 1..GCC_SVC_MAX_FOLDS (%d)", who, folds, GCC_SVC_MAX_FOLDS);
        return -5;
    }
    if (max_rows < 0 || max_rows > GCC_SVC_MAX_PROBLEM_ROWS) {
        snprintf(g_err, kErrLen, "%s: max_rows %d outside 0..GCC_SVC_MAX_PROBLEM_ROWS (%d): a (fold, class pair) problem holds at most "
                 "that many training rows", who, max_rows, GCC_SVC_MAX_PROBLEM_ROWS);
        return -6;
    }
    return 0;
}

// the checks every entry point shares; fills d and pl; rc < 0 names the member in g_err
int prepare(const char *who, const gcc_svc_args *h, void *workspace, int64_t workspace_bytes, int32_t *status, bool need_labels,
            SvcDev &d, Plan &pl)
{
    int rc = null_member(who, {{h, "args"}});
    if (rc) return rc;
    if ((rc = check_sizes(who, h->N, h->D, h->classes, h->folds, h->max_rows))) return rc;
    if ((rc = null_member(who, {{status, "status"}, {h->labels, "labels", need_labels}, {h->fold_of_row, "fold_of_row", need_labels},
                                {h->gamma, "gamma", need_labels}})))
        return rc;
    pl = make_plan(h->N, h->classes, h->folds, h->max_rows);
    if ((rc = check_workspace(who, "gcc_svc_workspace_bytes", workspace, workspace_bytes, pl.total))) return rc;
    d = SvcDev();
    d.emb = h->emb; d.ld = h->ld; d.labels = h->labels; d.fold = h->fold_of_row; d.gamma = h->gamma;
    d.N = h->N; d.D = h->D; d.classes = h->classes; d.folds = h->folds; d.ninner = 1; d.cands = 1; d.pairs = pl.pairs;
    d.budget = h->iters_per_launch; d.iter_cap = h->iter_cap; d.C = h->C; d.eps = h->eps;
    d.d2 = ws_at<float>(workspace, pl.off_d2);
    pl.pc.bind(d, workspace);
    d.pred = h->pred; d.decision = h->decision; d.iters = h->iters; d.rho = h->rho; d.obj = h->obj;
    d.n_free = h->n_free; d.n_bounded = h->n_bounded; d.problem_rows = h->problem_rows; d.unfinished = h->unfinished;
    d.first_rows = h->first_rows; d.rows_out = h->rows_out; d.alpha_out = h->alpha_out;
    d.status = status;
    return 0;
}

template <int kWaves> void launch_smo(const SvcDev &d, hipStream_t s)
{
    const size_t lds = smo_lds_bytes(kWaves, d.cap);
#ifndef GCC_AMD_HIPEMU
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute((const void *)svc_smo_kernel<kWaves>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
#endif
    hipLaunchKernelGGL((svc_smo_kernel<kWaves>), dim3(d.P), dim3(64 * kWaves), lds, s, d);
}
// one launch of every unfinished problem of d: one wave or four by the capacity of a row list
void launch_solve(const SvcDev &d, hipStream_t s)
{
    (void)hipMemsetAsync(d.unfinished, 0, sizeof(int32_t), s);
    if (d.cap <= kOneWaveRows) launch_smo<1>(d, s);
    else launch_smo<4>(d, s);
}
void launch_predict(const SvcDev &d, hipStream_t s)
{
    hipLaunchKernelGGL(svc_predict_kernel, dim3(d.N), dim3(64 * kPredictWaves), (size_t)d.pairs * 12, s, d);
}
int check_solver(const char *who, int32_t iters_per_launch, int32_t iter_cap, double C, double eps)
{
    if (iters_per_launch < 1 || iter_cap < 0 || !(C > 0.0) || !(eps > 0.0)) {
        snprintf(g_err, kErrLen, "%s: iters_per_launch %d must be positive, iter_cap %d not negative, C %g and eps %g positive", who,
                 iters_per_launch, iter_cap, C, eps);
        return -7;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------------------ grid search
int check_search_sizes(const char *who, int32_t N, int32_t D, int32_t classes, int32_t folds, int32_t inner, int32_t candidates,
                       int32_t max_rows, int32_t max_inner_rows)
{
    const int rc = check_sizes(who, N, D, classes, folds, max_rows);
    if (rc) return rc;
    if (inner < 2 || inner > GCC_SVC_SEARCH_MAX_INNER) {
        snprintf(g_err, kErrLen, "%s: inner %d outside 2..GCC_SVC_SEARCH_MAX_INNER (%d)", who, inner, GCC_SVC_SEARCH_MAX_INNER);
        return -11;
    }
    if (candidates < 1 || candidates > GCC_SVC_SEARCH_MAX_CANDIDATES) {
        snprintf(g_err, kErrLen, "%s: candidates %d outside 1..GCC_SVC_SEARCH_MAX_CANDIDATES (%d)", who, candidates,
                 GCC_SVC_SEARCH_MAX_CANDIDATES);
        return -12;
    }
    if (max_inner_rows < 0 || max_inner_rows > max_rows) {
        snprintf(g_err, kErrLen, "%s: max_inner_rows %d outside 0..max_rows (%d): an inner problem is part of its fold's", who,
                 max_inner_rows, max_rows);
        return -13;
    }
    const int64_t problems = (int64_t)folds * inner * (classes * (classes - 1) / 2) * candidates;
    if (problems > GCC_SVC_SEARCH_MAX_PROBLEMS) {
        snprintf(g_err, kErrLen, "%s: %lld inner problems (folds * inner * class pairs * candidates) are more than "
                 "GCC_SVC_SEARCH_MAX_PROBLEMS (%d)", who, (long long)problems, GCC_SVC_SEARCH_MAX_PROBLEMS);
        return -14;
    }
    return 0;
}

// the checks every search entry point shares; fills rf (the refit's problems, as the plain call's) and in (the inner problems,
// whose bits go to search_status)
int prepare_search(const char *who, const gcc_svc_search_args *h, void *workspace, int64_t workspace_bytes, int32_t *status, SvcDev &rf,
                   SvcDev &in, SearchPlan &pl)
{
    int rc = null_member(who, {{h, "args"}});
    if (rc) return rc;
    if ((rc = check_search_sizes(who, h->N, h->D, h->classes, h->folds, h->inner, h->candidates, h->max_rows, h->max_inner_rows)))
        return rc;
    if ((rc = null_member(who, {{status, "status"}, {h->search_status, "search_status"}, {h->labels, "labels"},
                                {h->fold_of_row, "fold_of_row"}, {h->inner_of_row, "inner_of_row"}, {h->gamma, "gamma"},
                                {h->inner_gamma, "inner_gamma"}, {h->Cs, "Cs"}, {h->unfinished, "unfinished"}})))
        return rc;
    if ((rc = check_solver(who, h->iters_per_launch, h->iter_cap, 1.0, h->eps))) return rc;
    pl = make_search_plan(h->N, h->classes, h->folds, h->inner, h->candidates, h->max_rows, h->max_inner_rows);
    if ((rc = check_workspace(who, "gcc_svc_search_workspace_bytes", workspace, workspace_bytes, pl.total))) return rc;
    rf = SvcDev();
    rf.emb = h->emb; rf.ld = h->ld; rf.labels = h->labels; rf.fold = h->fold_of_row; rf.gamma = h->gamma; rf.Cf = h->C_of_fold;
    rf.N = h->N; rf.D = h->D; rf.classes = h->classes; rf.folds = h->folds; rf.ninner = 1; rf.cands = 1; rf.pairs = pl.pairs;
    rf.budget = h->iters_per_launch; rf.iter_cap = h->iter_cap; rf.C = 0.0; rf.eps = h->eps;
    rf.d2 = ws_at<float>(workspace, pl.off_d2);
    rf.unfinished = h->unfinished;
    in = rf;
    pl.refit.bind(rf, workspace);
    rf.pred = h->pred; rf.decision = h->decision; rf.iters = h->iters; rf.rho = h->rho; rf.obj = h->obj;
    rf.n_free = h->n_free; rf.n_bounded = h->n_bounded; rf.problem_rows = h->problem_rows;
    rf.first_rows = h->first_rows; rf.rows_out = h->rows_out; rf.alpha_out = h->alpha_out;
    rf.status = status;
    pl.inner.bind(in, workspace);
    in.inner = h->inner_of_row; in.gamma = h->inner_gamma; in.Cs = h->Cs; in.Cf = nullptr;
    in.ninner = h->inner; in.cands = h->candidates;
    in.iters = h->search_iters; in.rho = h->search_rho; in.problem_rows = h->search_problem_rows;
    in.first_rows = h->search_first_rows; in.rows_out = h->search_rows; in.alpha_out = h->search_alpha;
    in.correct = h->correct;
    in.status = h->search_status;
    return 0;
}

}  // namespace

extern "C" {

int64_t gcc_svc_workspace_bytes(int32_t N, int32_t D, int32_t classes, int32_t folds, int32_t max_rows)
{
    const int rc = check_sizes("gcc_svc_workspace_bytes", N, D, classes, folds, max_rows);
    if (rc) return rc;
    return make_plan(N, classes, folds, max_rows).total;
}

int32_t gcc_svc_distances(const gcc_svc_args *h, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream)
{
    const char *who = "gcc_svc_distances";
    SvcDev d;
    Plan pl;
    int rc = prepare(who, h, workspace, workspace_bytes, status, false, d, pl);
    if (rc) return rc;
    if ((rc = null_member(who, {{h->emb, "emb"}}))) return rc;
    if (h->ld < h->D) {
        snprintf(g_err, kErrLen, "%s: ld %lld must be at least D (%d)", who, (long long)h->ld, h->D);
        return -7;
    }
    if ((h->labels != nullptr) != (h->fold_of_row != nullptr)) {
        snprintf(g_err, kErrLen, "%s: labels and fold_of_row come together (both NULL: the distances only)", who);
        return -1;
    }
    const unsigned tiles = (unsigned)((h->N + kTile - 1) / kTile);
    hipLaunchKernelGGL(svc_d2_kernel, dim3(tiles, tiles), dim3(kD2Threads), 0, (hipStream_t)stream, d);
    if (h->labels) hipLaunchKernelGGL(svc_setup_kernel, dim3(d.groups), dim3(64), 0, (hipStream_t)stream, d);
    return launched();
}

int32_t gcc_svc_solve(const gcc_svc_args *h, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream)
{
    const char *who = "gcc_svc_solve";
    SvcDev d;
    Plan pl;
    int rc = prepare(who, h, workspace, workspace_bytes, status, true, d, pl);
    if (rc) return rc;
    if ((rc = null_member(who, {{h->unfinished, "unfinished"}}))) return rc;
    if ((rc = check_solver(who, h->iters_per_launch, h->iter_cap, h->C, h->eps))) return rc;
    launch_solve(d, (hipStream_t)stream);
    return launched();
}

int32_t gcc_svc_predict(const gcc_svc_args *h, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream)
{
    const char *who = "gcc_svc_predict";
    SvcDev d;
    Plan pl;
    const int rc = prepare(who, h, workspace, workspace_bytes, status, true, d, pl);
    if (rc) return rc;
    launch_predict(d, (hipStream_t)stream);
    return launched();
}

int64_t gcc_svc_search_workspace_bytes(int32_t N, int32_t D, int32_t classes, int32_t folds, int32_t inner, int32_t candidates,
                                       int32_t max_rows, int32_t max_inner_rows)
{
    const int rc = check_search_sizes("gcc_svc_search_workspace_bytes", N, D, classes, folds, inner, candidates, max_rows, max_inner_rows);
    if (rc) return rc;
    return make_search_plan(N, classes, folds, inner, candidates, max_rows, max_inner_rows).total;
}

int32_t gcc_svc_search_setup(const gcc_svc_search_args *h, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream)
{
    const char *who = "gcc_svc_search_setup";
    SvcDev rf, in;
    SearchPlan pl;
    int rc = prepare_search(who, h, workspace, workspace_bytes, status, rf, in, pl);
    if (rc) return rc;
    if ((rc = null_member(who, {{h->emb, "emb"}}))) return rc;
    if (h->ld < h->D) {
        snprintf(g_err, kErrLen, "%s: ld %lld must be at least D (%d)", who, (long long)h->ld, h->D);
        return -7;
    }
    hipStream_t s = (hipStream_t)stream;
    const unsigned tiles = (unsigned)((h->N + kTile - 1) / kTile);
    hipLaunchKernelGGL(svc_d2_kernel, dim3(tiles, tiles), dim3(kD2Threads), 0, s, rf);
    hipLaunchKernelGGL(svc_setup_kernel, dim3(rf.groups), dim3(64), 0, s, rf);
    hipLaunchKernelGGL(svc_setup_kernel, dim3(in.groups), dim3(64), 0, s, in);
    return launched();
}

int32_t gcc_svc_search_solve(const gcc_svc_search_args *h, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream)
{
    SvcDev rf, in;
    SearchPlan pl;
    const int rc = prepare_search("gcc_svc_search_solve", h, workspace, workspace_bytes, status, rf, in, pl);
    if (rc) return rc;
    launch_solve(in, (hipStream_t)stream);
    return launched();
}

int32_t gcc_svc_search_score(const gcc_svc_search_args *h, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream)
{
    const char *who = "gcc_svc_search_score";
    SvcDev rf, in;
    SearchPlan pl;
    int rc = prepare_search(who, h, workspace, workspace_bytes, status, rf, in, pl);
    if (rc) return rc;
    if ((rc = null_member(who, {{h->correct, "correct"}}))) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = (size_t)in.cands * in.pairs * 12;
#ifndef GCC_AMD_HIPEMU
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute((const void *)svc_score_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
#endif
    (void)hipMemsetAsync(h->correct, 0, sizeof(int32_t) * (size_t)h->folds * h->candidates * h->inner, s);
    hipLaunchKernelGGL(svc_score_kernel, dim3(h->N, h->folds), dim3(64 * kPredictWaves), lds, s, in);
    return launched();
}

int32_t gcc_svc_search_refit(const gcc_svc_search_args *h, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream)
{
    const char *who = "gcc_svc_search_refit";
    SvcDev rf, in;
    SearchPlan pl;
    int rc = prepare_search(who, h, workspace, workspace_bytes, status, rf, in, pl);
    if (rc) return rc;
    if ((rc = null_member(who, {{h->C_of_fold, "C_of_fold"}}))) return rc;
    launch_solve(rf, (hipStream_t)stream);
    return launched();
}

int32_t gcc_svc_search_predict(const gcc_svc_search_args *h, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream)
{
    SvcDev rf, in;
    SearchPlan pl;
    const int rc = prepare_search("gcc_svc_search_predict", h, workspace, workspace_bytes, status, rf, in, pl);
    if (rc) return rc;
    launch_predict(rf, (hipStream_t)stream);
    return launched();
}

}  // extern "C"
