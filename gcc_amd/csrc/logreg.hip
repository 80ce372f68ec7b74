// gcc_amd/csrc/logreg.hip -- L2-regularised logistic regression on frozen embeddings, one-vs-rest, every fold of a
// cross-validation and every class in one call (gfx950).
//
// Replaces the fit / predict loop of NodeClassification._evaluate (gcc/tasks/node_classification.py:53-101 of the reference:
// StratifiedKFold, TopKRanker(LogisticRegression(C=1000)) per fold, the k most probable classes per held-out row).  Problem
// p = fold * classes + class trains on the corpus rows whose fold id differs from its fold, against column `class` of the
// indicator matrix.  Every problem computes THE MINIMISER of
//     f(w, b) = 1/2 |w|^2 + rho 1/2 b^2 + C sum_{training rows} [log(1 + exp(z_r)) - t_r z_r],   z_r = w . x_r + b
// by damped Newton steps from w = b = 0: gradient, Hessian, Cholesky, objective and line search in float64, x float32 in memory.
//
//   lr_finite_kernel     flags NaN / infinite embeddings.
//   lr_setup_kernel      one wave per problem: positives and negatives of the training side (a constant column is not solved:
//       decision -inf / +inf), w = 0, the fold-id check.  Z = 0 by a memset.
//   lr_grad_kernel       grid (row split of its own, problem): from Z, q = m (p - t) and the Hessian weights s = m p (1 - p) (m: the training
//       mask) per row, and the split's part of X~^T q (X~ = [X | 1]), rows in ascending order.
//   lr_test_kernel       one wave per problem: g = R [w; b] + C sum of the parts in split order, the stop rule max|g| / C <= tol,
//       the iteration cap.
//   lr_hess_kernel       THE HOT PATH, grid (upper-triangle 16 x 16 tile, row split, problem): sum_r (s_r x~_r[i]) x~_r[j] on
//       v_mfma_f64_16x16x4_f64, four rows per instruction, the weight applied to the A operand; four waves take the row groups
//       round robin and are added in wave order.
//   lr_newton_kernel     one workgroup per running problem: H = R + C (parts in split order), Cholesky (in LDS up to D = 128, in
//       the workspace above), two triangular solves, the decrement g^T d.
//   lr_zd_kernel         one wave per (row, problem): Zd = X~ d.
//   lr_search_kernel     one workgroup per running problem: f(w - s d) for s = 1, 1/2, ... from Z and Zd alone (Armijo, constant
//       1e-4), then w -= s d, Z -= s Zd.
//   lr_predict_kernel    one workgroup per corpus row: decision values of the row's own fold from the final w (float64, lanes
//       strided), top-k under (decision descending, class ascending), tp / fp / fn per fold with integer atomics.
// No floating-point atomics: every sum has one fixed order, which depends on the sizes alone.  The workgroup sum, the Gram tile and
// the entry points' scaffold are task_common.h's.
#include "task_common.h"

#include <float.h>
#include <math.h>

namespace {

constexpr int kThreads = 256, kWaves = 4;
constexpr int kLdsDim = 128;                  // Cholesky in LDS up to this D ((D + 1)^2 float64 = 130 KiB), in the workspace above
constexpr double kArmijo = 1e-4, kMinStep = 1.0 / 1099511627776.0;        // 2^-40
constexpr double kRoundSlack = 64.0 * DBL_EPSILON;                        // of |f|: what the line search allows for rounding
static_assert(kWaves == kGramWaves, "lr_hess_kernel");
enum { kRunning = 0, kConverged = 1, kCapped = 2, kAllZero = 3, kAllOne = 4, kBadPivot = 5, kNoDecrease = 6, kNotRun = 7 };

struct LrDev {
    const float *emb;
    long long ld;
    const uint8_t *y;
    const int32_t *fold;
    int32_t N, D, classes, folds, P, Dp, Dpad, T, tiles, splits, rps, gsplits, grps, iter_cap, count;
    double C, tol, rho;
    double *Z, *Zd, *S;                       // [P][N]
    double *Hpart;                            // [P][splits][tiles][256], a tile in row-major order
    double *Hfull;                            // [P][Dp][Dp] (D > kLdsDim only)
    double *gpart;                            // [P][gsplits][Dpad]
    double *w, *g, *d;                        // [P][Dpad]; entry D is the intercept's
    double *gmax, *dec;                       // [P]
    int32_t *pstate, *piter;                  // [P]
    uint8_t *pred;
    double *decision;
    int32_t *counts;
    double *coef, *intercept, *grad_out;
    int32_t *iters_out, *state_out, *unfinished, *status;
};

__device__ __forceinline__ double sigmoid(double z)
{
    if (z >= 0.0) return 1.0 / (1.0 + exp(-z));
    const double e = exp(z);
    return e / (1.0 + e);
}
// log(1 + exp(z)) without overflow
__device__ __forceinline__ double log1pexp(double z) { return (z > 0.0 ? z : 0.0) + log1p(exp(-fabs(z))); }

__global__ __launch_bounds__(kThreads) void lr_finite_kernel(LrDev a)
{
    const int r0 = (int)blockIdx.x * 64;
    bool bad = false;
    for (int e = (int)threadIdx.x; e < 64 * a.D; e += kThreads) {
        const int r = r0 + e / a.D, c = e % a.D;
        if (r < a.N) bad |= !(fabsf(a.emb[(long long)r * a.ld + c]) <= FLT_MAX);
    }
    if (bad) atomicOr(a.status, (int32_t)GCC_STATUS_LR_NONFINITE);
}

__global__ __launch_bounds__(64) void lr_setup_kernel(LrDev a)
{
    const int p = (int)blockIdx.x, lane = lane_id();
    const int f = p / a.classes, c = p % a.classes;
    int npos = 0, nneg = 0, bits = 0;
    for (int r0 = 0; r0 < a.N; r0 += 64) {
        const int r = r0 + lane;
        const int fo = r < a.N ? a.fold[r] : 0;
        if (wave_ballot(fo < 0 || fo >= a.folds)) bits |= GCC_STATUS_LR_BAD_FOLD;       // (bits: wave-uniform)
        const bool train = r < a.N && fo >= 0 && fo < a.folds && fo != f;
        const bool pos = train && a.y[(long long)r * a.classes + c] != 0;
        npos += __popcll(wave_ballot(pos));
        nneg += __popcll(wave_ballot(train && !pos));
    }
    for (int j = lane; j < a.Dpad; j += 64) {
        a.w[(long long)p * a.Dpad + j] = 0.0;
        a.g[(long long)p * a.Dpad + j] = 0.0;
        a.d[(long long)p * a.Dpad + j] = 0.0;
    }
    if (lane == 0) {
        // (lr_finite_kernel ran before this launch: nothing is solved on a table with NaN or infinite entries)
        const bool finite = (load_fresh_i32(a.status) & GCC_STATUS_LR_NONFINITE) == 0;
        a.pstate[p] = !finite ? kNotRun : npos == 0 ? kAllZero : nneg == 0 ? kAllOne : kRunning;       // (no training row at all: all zeros)
        a.piter[p] = 0;
        a.gmax[p] = 0.0;
        a.dec[p] = 0.0;
        if (bits) atomicOr(a.status, (int32_t)bits);
    }
}

// entry c of the augmented row r: x[r][c], 1 in column D, 0 past it (the columns between D and ld are never read)
__device__ __forceinline__ double aug(const LrDev &a, int r, int c)
{
    return c < a.D ? (double)a.emb[(long long)r * a.ld + c] : c == a.D ? 1.0 : 0.0;
}

__global__ __launch_bounds__(kThreads) void lr_grad_kernel(LrDev a)
{
    __shared__ double q_s[kThreads], part_s[kThreads], red[kWaves];
    const int split = (int)blockIdx.x, p = (int)blockIdx.y, tid = (int)threadIdx.x;
    if (a.pstate[p] != kRunning) return;                            // (the whole workgroup)
    const int f = p / a.classes, c = p % a.classes;
    const int r0 = split * a.grps, r1 = min(a.N, r0 + a.grps);
    // thread (rg, j): column j of the rows rg, rg + G, ... of a chunk; nj = the power of two that holds the D columns
    int nj = 1;
    while (nj < a.D) nj <<= 1;
    const int G = kThreads / nj, j = tid % nj, rg = tid / nj;
    const long long pN = (long long)p * a.N;
    double acc = 0.0, qsum = 0.0;
    for (int c0 = r0; c0 < r1; c0 += kThreads) {
        const int r = c0 + tid;
        double q = 0.0;
        if (r < r1) {
            const int fo = a.fold[r];
            const bool train = fo >= 0 && fo < a.folds && fo != f;
            double s = 0.0;
            if (train) {
                const double pr = sigmoid(a.Z[pN + r]);
                q = pr - (a.y[(long long)r * a.classes + c] != 0 ? 1.0 : 0.0);
                s = pr * (1.0 - pr);
            }
            a.S[pN + r] = s;
        }
        q_s[tid] = q;
        qsum += q;
        __syncthreads();
        if (j < a.D) {
            const int n = min(kThreads, r1 - c0);
            for (int t = rg; t < n; t += G) acc = fma((double)a.emb[(long long)(c0 + t) * a.ld + j], q_s[t], acc);
        }
        __syncthreads();
    }
    const double qtot = block_sum<kWaves>(qsum, red);
    part_s[tid] = acc;
    __syncthreads();
    double *out = a.gpart + ((long long)p * a.gsplits + split) * a.Dpad;
    if (tid < a.D) {
        double s = part_s[tid];
        for (int k = 1; k < G; ++k) s += part_s[k * nj + tid];      // the row groups in order
        out[tid] = s;
    }
    if (tid == 0) out[a.D] = qtot;
}

__global__ __launch_bounds__(64) void lr_test_kernel(LrDev a)
{
    const int p = (int)blockIdx.x, lane = lane_id();
    if (a.pstate[p] != kRunning) return;
    const long long base = (long long)p * a.Dpad;
    double gm = 0.0;
    bool nan = false;
    for (int j = lane; j < a.Dp; j += 64) {
        double s = 0.0;
        for (int k = 0; k < a.gsplits; ++k) s += a.gpart[((long long)p * a.gsplits + k) * a.Dpad + j];
        const double gj = (j < a.D ? 1.0 : a.rho) * a.w[base + j] + a.C * s;
        a.g[base + j] = gj;
        nan |= !(fabs(gj) <= DBL_MAX);
        gm = fabs(gj) > gm ? fabs(gj) : gm;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const double o = wave_shfl_xor(gm, d); gm = o > gm ? o : gm; }
    const bool anynan = wave_ballot(nan) != 0;
    if (lane == 0) {
        const double rel = anynan ? (double)INFINITY : gm / a.C;
        a.gmax[p] = rel;
        if (rel <= a.tol) a.pstate[p] = kConverged;
        else if (a.piter[p] >= a.iter_cap) {
            a.pstate[p] = kCapped;
            atomicOr(a.status, (int32_t)GCC_STATUS_LR_ITER_CAP);
        } else if (a.count) atomicAdd(a.unfinished, 1);
    }
}

__global__ __launch_bounds__(kThreads) void lr_hess_kernel(LrDev a)
{
    __shared__ double red[kWaves][256];
    const int tile = (int)blockIdx.x, split = (int)blockIdx.y, p = (int)blockIdx.z, jl = lane_id() & 15;
    if (a.pstate[p] != kRunning) return;
    int ti, tj;
    tri_tile_of(tile, a.T, ti, tj);
    const int ca = 16 * ti + jl, cb = 16 * tj + jl;
    const int r0 = split * a.rps, r1 = min(a.N, r0 + a.rps);
    const double *S = a.S + (long long)p * a.N;
    // A[jl][q] = s x~[row q][ca], B[q][jl] = x~[row q][cb]; rows past the end read the last row, weight 0
    const double h = gram_tile_f64(
        r0, r1,
        [&](int r, bool in) {
            const int rc = in ? r : r1 - 1;
            const double s = in ? S[rc] : 0.0, x = aug(a, rc, ca);
            return s != 0.0 ? s * x : 0.0;
        },
        [&](int r, bool in) { return aug(a, in ? r : r1 - 1, cb); }, red);
    a.Hpart[(((long long)p * a.splits + split) * a.tiles + tile) * 256 + threadIdx.x] = h;
}

__global__ __launch_bounds__(kThreads) void lr_newton_kernel(LrDev a)
{
    DYN_SMEM(smem);
    __shared__ double red[kWaves];
    const int p = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (a.pstate[p] != kRunning) return;
    const int n = a.Dp;
    double *v_s = reinterpret_cast<double *>(smem);                 // [n] right-hand side of the solve in progress
    double *y_s = v_s + n;                                          // [n] its solution
    double *diag_s = y_s + n;                                       // [n] the diagonal of L
    double *M = a.D <= kLdsDim ? diag_s + n : a.Hfull + (long long)p * n * n;      // [n][n], lower triangle: L
    const long long base = (long long)p * a.Dpad;
    for (int e = tid; e < n * n; e += kThreads) {
        const int i = e / n, j = e % n;
        if (i > j) continue;
        const long long at = (long long)tri_tile_index(i >> 4, j >> 4, a.T) * 256 + (i & 15) * 16 + (j & 15);
        double s = 0.0;
        for (int k = 0; k < a.splits; ++k) s += a.Hpart[((long long)p * a.splits + k) * a.tiles * 256 + at];
        const double h = a.C * s + (i == j ? (i < a.D ? 1.0 : a.rho) : 0.0);
        M[i * n + j] = h;
        M[j * n + i] = h;
    }
    for (int j = tid; j < n; j += kThreads) v_s[j] = a.g[base + j];
    __syncthreads();
    // ---- Cholesky, right-looking: the pivots stay where they are and L's diagonal goes to diag_s
    bool ok = true;
    for (int k = 0; k < n; ++k) {
        const double piv = M[k * n + k];
        if (!(piv > 0.0) || !(piv <= DBL_MAX)) { ok = false; break; }         // (workgroup-uniform: every thread reads the same pivot)
        const double l = sqrt(piv);
        if (tid == 0) diag_s[k] = l;
        for (int i = k + 1 + tid; i < n; i += kThreads) M[i * n + k] /= l;
        __syncthreads();
        const int m = n - k - 1;
        for (int e = tid; e < m * m; e += kThreads) {
            const int i = k + 1 + e / m, j = k + 1 + e % m;
            if (j <= i) M[i * n + j] -= M[i * n + k] * M[j * n + k];
        }
        __syncthreads();
    }
    if (!ok) {
        if (tid == 0) {
            a.pstate[p] = kBadPivot;
            atomicOr(a.status, (int32_t)GCC_STATUS_LR_PIVOT);
        }
        return;
    }
    // ---- L y = g, then L^T d = y: one column of L per step
    for (int k = 0; k < n; ++k) {
        const double yk = v_s[k] / diag_s[k];
        if (tid == 0) y_s[k] = yk;
        for (int i = k + 1 + tid; i < n; i += kThreads) v_s[i] -= M[i * n + k] * yk;
        __syncthreads();
    }
    for (int k = n - 1; k >= 0; --k) {
        const double dk = y_s[k] / diag_s[k];
        if (tid == 0) v_s[k] = dk;                                  // (v_s[k] is dead: the forward solve is done)
        for (int j = tid; j < k; j += kThreads) y_s[j] -= M[k * n + j] * dk;
        __syncthreads();
    }
    double part = 0.0;
    for (int j = tid; j < n; j += kThreads) {
        a.d[base + j] = v_s[j];
        part += a.g[base + j] * v_s[j];
    }
    const double dec = block_sum<kWaves>(part, red);
    if (tid == 0) a.dec[p] = dec;
}

__global__ __launch_bounds__(kThreads) void lr_zd_kernel(LrDev a)
{
    const int p = (int)blockIdx.y, lane = lane_id(), wv = (int)threadIdx.x >> 6;
    if (a.pstate[p] != kRunning) return;
    const int f = p / a.classes;
    const double *d = a.d + (long long)p * a.Dpad;
    double dv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) dv[k] = lane + 64 * k < a.D ? d[lane + 64 * k] : 0.0;
    const double db = d[a.D];
    for (int t = 0; t < 16; ++t) {
        const int r = ((int)blockIdx.x * kWaves + wv) * 16 + t;
        if (r >= a.N) break;                                        // (wave-uniform)
        const int fo = a.fold[r];
        if (fo < 0 || fo >= a.folds || fo == f) continue;           // (held-out rows take no part in the search)
        const float *x = a.emb + (long long)r * a.ld;
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (lane + 64 * k < a.D) s = fma((double)x[lane + 64 * k], dv[k], s);
        s = wave_sum(s) + db;
        if (lane == 0) a.Zd[(long long)p * a.N + r] = s;
    }
}

__global__ __launch_bounds__(kThreads) void lr_search_kernel(LrDev a)
{
    __shared__ double red[kWaves];
    const int p = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (a.pstate[p] != kRunning) return;
    const int f = p / a.classes, c = p % a.classes;
    const long long base = (long long)p * a.Dpad, pN = (long long)p * a.N;
    const double dec = a.dec[p];
    // f(w - s d): the regulariser from w and d, the loss from Z - s Zd over the training rows (thread-strided, then block_sum)
    auto value = [&](double s) {
        double part = 0.0;
        for (int j = tid; j < a.Dp; j += kThreads) {
            const double wj = a.w[base + j] - s * a.d[base + j];
            part += 0.5 * (j < a.D ? 1.0 : a.rho) * wj * wj;
        }
        double loss = 0.0;
        for (int r = tid; r < a.N; r += kThreads) {
            const int fo = a.fold[r];
            if (fo < 0 || fo >= a.folds || fo == f) continue;
            const double z = a.Z[pN + r] - s * a.Zd[pN + r];
            loss += log1pexp(z) - (a.y[(long long)r * a.classes + c] != 0 ? z : 0.0);
        }
        return block_sum<kWaves>(part + a.C * loss, red);
    };
    // Armijo, with the rounding of the two sums allowed for: near the minimiser the decrease of a full Newton step (~ dec / 2) is
    // below the rounding of f itself, and a test on the bare values would halve good steps at random there
    const double f0 = value(0.0), slack = kRoundSlack * fabs(f0);
    double s = 1.0;
    bool found = false;
    for (; s >= kMinStep; s *= 0.5) {                               // (workgroup-uniform: block_sum hands every thread the same value)
        const double ft = value(s);
        if (ft <= f0 - kArmijo * s * dec + slack) { found = true; break; }
    }
    if (!found) {
        if (tid == 0) {
            a.pstate[p] = kNoDecrease;
            atomicOr(a.status, (int32_t)GCC_STATUS_LR_LINE_SEARCH);
        }
        return;
    }
    for (int j = tid; j < a.Dp; j += kThreads) a.w[base + j] -= s * a.d[base + j];
    for (int r = tid; r < a.N; r += kThreads) {
        const int fo = a.fold[r];
        if (fo < 0 || fo >= a.folds || fo == f) continue;
        a.Z[pN + r] -= s * a.Zd[pN + r];
    }
    if (tid == 0) a.piter[p] += 1;
}

__global__ __launch_bounds__(64) void lr_finish_kernel(LrDev a)
{
    const int p = (int)blockIdx.x, lane = lane_id();
    const int st = a.pstate[p];
    const bool solved = st != kAllZero && st != kAllOne;
    for (int j = lane; j < a.D; j += 64)
        if (a.coef) a.coef[(long long)p * a.D + j] = solved ? a.w[(long long)p * a.Dpad + j] : 0.0;
    if (lane == 0) {
        if (a.intercept) a.intercept[p] = solved ? a.w[(long long)p * a.Dpad + a.D] : st == kAllZero ? -(double)INFINITY : (double)INFINITY;
        if (a.iters_out) a.iters_out[p] = a.piter[p];
        if (a.grad_out) a.grad_out[p] = a.gmax[p];
        if (a.state_out) a.state_out[p] = st;
    }
}

__global__ __launch_bounds__(kThreads) void lr_predict_kernel(LrDev a)
{
    __shared__ double dec_s[GCC_LR_MAX_CLASSES];
    __shared__ int32_t cnt_s[4];
    const int r = (int)blockIdx.x, tid = (int)threadIdx.x, lane = lane_id(), wv = tid >> 6;
    const int f = a.fold[r];
    const bool served = f >= 0 && f < a.folds;                      // (workgroup-uniform)
    const float *x = a.emb + (long long)r * a.ld;
    if (tid < 4) cnt_s[tid] = 0;
    for (int c = wv; c < a.classes; c += kWaves) {
        double dec = 0.0;
        if (served) {
            const int p = f * a.classes + c, st = a.pstate[p];
            if (st == kAllZero) dec = -(double)INFINITY;
            else if (st == kAllOne) dec = (double)INFINITY;
            else {
                const double *w = a.w + (long long)p * a.Dpad;
                double s = 0.0;
                for (int j = lane; j < a.D; j += 64) s = fma((double)x[j], w[j], s);
                dec = wave_sum(s) + w[a.D];
            }
        }
        if (lane == 0) {
            dec_s[c] = dec;
            if (a.decision) a.decision[(long long)r * a.classes + c] = dec;
        }
    }
    __syncthreads();
    // class c is predicted when fewer than k classes come before it (decision descending, class ascending); k = the row's label
    // count, and no label means every class (the reference's argsort()[-0:])
    int k = 0;
    for (int c = 0; c < a.classes; ++c) k += a.y[(long long)r * a.classes + c] != 0;
    if (k == 0) k = a.classes;
    if (tid < a.classes) {
        const double mine = dec_s[tid];
        int before = 0;
        for (int c = 0; c < a.classes; ++c) before += dec_s[c] > mine || (dec_s[c] == mine && c < tid);
        const int pr = served && before < k, yy = a.y[(long long)r * a.classes + tid] != 0;
        a.pred[(long long)r * a.classes + tid] = (uint8_t)pr;
        if (served) {
            if (pr && yy) atomicAdd(&cnt_s[0], 1);
            if (pr && !yy) atomicAdd(&cnt_s[1], 1);
            if (!pr && yy) atomicAdd(&cnt_s[2], 1);
        }
    }
    __syncthreads();
    if (served && tid < 3 && cnt_s[tid] && a.counts) atomicAdd(a.counts + f * 3 + tid, cnt_s[tid]);
}

struct Plan {
    int32_t P, Dp, Dpad, T, tiles, splits, rps, gsplits, grps;
    int64_t off_Z, off_Zd, off_S, off_Hpart, off_Hfull, off_gpart, off_w, off_g, off_d, off_gmax, off_dec, off_state, off_iter, total;
};

// the row splits depend on the sizes alone, so a result does not depend on how the work was scheduled
Plan make_plan(int32_t N, int32_t D, int32_t classes, int32_t folds)
{
    Plan p;
    p.P = folds * classes;
    p.Dp = D + 1;
    p.Dpad = (p.Dp + 15) & ~15;
    p.T = p.Dpad / 16;
    p.tiles = p.T * (p.T + 1) / 2;
    const int64_t want = (1024 + (int64_t)p.P * p.tiles - 1) / ((int64_t)p.P * p.tiles), most = (N + 63) / 64;
    p.splits = (int32_t)(want < 1 ? 1 : want > 64 ? 64 : want);
    if (p.splits > most) p.splits = (int32_t)most;
    p.rps = (((N + p.splits - 1) / p.splits) + 31) & ~31;          // rows of a split: whole passes of the Hessian's four waves
    p.splits = (N + p.rps - 1) / p.rps;
    p.grps = (((N + 63) / 64) + 255) & ~255;                      // the gradient's own row splits: at most 64, whole chunks of 256 rows
    p.gsplits = (N + p.grps - 1) / p.grps;
    Carve cv;
    const int64_t PN = (int64_t)p.P * N * 8, vec = (int64_t)p.P * p.Dpad * 8;
    p.off_Z = cv.take(PN);
    p.off_Zd = cv.take(PN);
    p.off_S = cv.take(PN);
    p.off_Hpart = cv.take((int64_t)p.P * p.splits * p.tiles * 256 * 8);
    p.off_Hfull = cv.take((D > kLdsDim ? (int64_t)p.P * p.Dp * p.Dp * 8 : 0));
    p.off_gpart = cv.take(vec * p.gsplits);
    p.off_w = cv.take(vec);
    p.off_g = cv.take(vec);
    p.off_d = cv.take(vec);
    p.off_gmax = cv.take((int64_t)p.P * 8);
    p.off_dec = cv.take((int64_t)p.P * 8);
    p.off_state = cv.take((int64_t)p.P * 4);
    p.off_iter = cv.take((int64_t)p.P * 4);
    p.total = cv.total();
    return p;
}

int check_sizes(const char *who, int32_t N, int32_t D, int32_t classes, int32_t folds)
{
    if (N < 1 || N > GCC_LR_MAX_ROWS) {
        snprintf(g_err, kErrLen, "%s: N %d outside 1..GCC_LR_MAX_ROWS (%d)", who, N, GCC_LR_MAX_ROWS);
        return -2;
    }
    if (D < 1 || D > GCC_LR_MAX_DIM) {
        snprintf(g_err, kErrLen, "%s: D %d outside 1..GCC_LR_MAX_DIM (%d)", who, D, GCC_LR_MAX_DIM);
        return -3;
    }
    if (classes < 1 || classes > GCC_LR_MAX_CLASSES) {
        snprintf(g_err, kErrLen, "%s: classes %d outside 1..GCC_LR_MAX_CLASSES (%d)", who, classes, GCC_LR_MAX_CLASSES);
        return -4;
    }
    if (folds < 1 || folds > GCC_LR_MAX_FOLDS) {
        snprintf(g_err, kErrLen, "%s: folds %d outside 1..GCC_LR_MAX_FOLDS (%d)", who, folds, GCC_LR_MAX_FOLDS);
        return -5;
    }
    return 0;
}

// the checks every entry point shares; fills d and pl; rc < 0 names the member in g_err
int prepare(const char *who, const gcc_logreg_args *h, void *workspace, int64_t workspace_bytes, int32_t *status, LrDev &d, Plan &pl)
{
    int rc = null_member(who, {{h, "args"}});
    if (rc) return rc;
    if ((rc = check_sizes(who, h->N, h->D, h->classes, h->folds))) return rc;
    if ((rc = null_member(who, {{status, "status"}, {h->emb, "emb"}, {h->y, "y"}, {h->fold_of_row, "fold_of_row"}}))) return rc;
    if (h->ld < h->D) {
        snprintf(g_err, kErrLen, "%s: ld %lld must be at least D (%d)", who, (long long)h->ld, h->D);
        return -7;
    }
    if (!(h->C > 0.0) || !(h->tol > 0.0) || !(h->intercept_penalty >= 0.0) || h->iter_cap < 1 || h->iters_per_sync < 1) {
        snprintf(g_err, kErrLen, "%s: C %g and tol %g must be positive, intercept_penalty %g not negative, iter_cap %d and "
                 "iters_per_sync %d at least 1", who, h->C, h->tol, h->intercept_penalty, h->iter_cap, h->iters_per_sync);
        return -7;
    }
    pl = make_plan(h->N, h->D, h->classes, h->folds);
    if ((rc = check_workspace(who, "gcc_logreg_workspace_bytes", workspace, workspace_bytes, pl.total))) return rc;
    auto f64 = [&](int64_t off) { return ws_at<double>(workspace, off); };
    d = LrDev();
    d.emb = h->emb; d.ld = h->ld; d.y = h->y; d.fold = h->fold_of_row;
    d.N = h->N; d.D = h->D; d.classes = h->classes; d.folds = h->folds;
    d.P = pl.P; d.Dp = pl.Dp; d.Dpad = pl.Dpad; d.T = pl.T; d.tiles = pl.tiles; d.splits = pl.splits; d.rps = pl.rps;
    d.gsplits = pl.gsplits; d.grps = pl.grps;
    d.iter_cap = h->iter_cap; d.count = 0; d.C = h->C; d.tol = h->tol; d.rho = h->intercept_penalty;
    d.Z = f64(pl.off_Z); d.Zd = f64(pl.off_Zd); d.S = f64(pl.off_S); d.Hpart = f64(pl.off_Hpart); d.Hfull = f64(pl.off_Hfull);
    d.gpart = f64(pl.off_gpart); d.w = f64(pl.off_w); d.g = f64(pl.off_g); d.d = f64(pl.off_d);
    d.gmax = f64(pl.off_gmax); d.dec = f64(pl.off_dec);
    d.pstate = ws_at<int32_t>(workspace, pl.off_state); d.piter = ws_at<int32_t>(workspace, pl.off_iter);
    d.pred = h->pred; d.decision = h->decision; d.counts = h->counts; d.coef = h->coef; d.intercept = h->intercept;
    d.grad_out = h->grad; d.iters_out = h->iters; d.state_out = h->state; d.unfinished = h->unfinished;
    d.status = status;
    return 0;
}

// the gradient at the current w and the stop rule; count: add the problems that go on to *unfinished
void launch_grad_test(LrDev d, bool count, hipStream_t s)
{
    d.count = count ? 1 : 0;
    hipLaunchKernelGGL(lr_grad_kernel, dim3(d.gsplits, d.P), dim3(kThreads), 0, s, d);
    hipLaunchKernelGGL(lr_test_kernel, dim3(d.P), dim3(64), 0, s, d);
}

size_t newton_lds_bytes(const LrDev &d)
{
    return (size_t)d.Dp * 24 + (d.D <= kLdsDim ? (size_t)d.Dp * d.Dp * 8 : 0);
}

}  // namespace

extern "C" {

int64_t gcc_logreg_workspace_bytes(int32_t N, int32_t D, int32_t classes, int32_t folds)
{
    const int rc = check_sizes("gcc_logreg_workspace_bytes", N, D, classes, folds);
    if (rc) return rc;
    return make_plan(N, D, classes, folds).total;
}

int32_t gcc_logreg_setup(const gcc_logreg_args *h, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream)
{
    LrDev d;
    Plan pl;
    const int rc = prepare("gcc_logreg_setup", h, workspace, workspace_bytes, status, d, pl);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    (void)hipMemsetAsync(d.Z, 0, (size_t)pl.P * h->N * 8, s);
    hipLaunchKernelGGL(lr_finite_kernel, dim3((h->N + 63) / 64), dim3(kThreads), 0, s, d);
    hipLaunchKernelGGL(lr_setup_kernel, dim3(pl.P), dim3(64), 0, s, d);
    launch_grad_test(d, false, s);
    return launched();
}

int32_t gcc_logreg_step(const gcc_logreg_args *h, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream)
{
    const char *who = "gcc_logreg_step";
    LrDev d;
    Plan pl;
    int rc = prepare(who, h, workspace, workspace_bytes, status, d, pl);
    if (rc) return rc;
    if ((rc = null_member(who, {{h->unfinished, "unfinished"}}))) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = newton_lds_bytes(d);
#ifndef GCC_AMD_HIPEMU
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void *)lr_newton_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
#endif
    (void)hipMemsetAsync(h->unfinished, 0, sizeof(int32_t), s);
    for (int it = 0; it < h->iters_per_sync; ++it) {
        hipLaunchKernelGGL(lr_hess_kernel, dim3(pl.tiles, pl.splits, pl.P), dim3(kThreads), 0, s, d);
        hipLaunchKernelGGL(lr_newton_kernel, dim3(pl.P), dim3(kThreads), lds, s, d);
        hipLaunchKernelGGL(lr_zd_kernel, dim3((h->N + 16 * kWaves - 1) / (16 * kWaves), pl.P), dim3(kThreads), 0, s, d);
        hipLaunchKernelGGL(lr_search_kernel, dim3(pl.P), dim3(kThreads), 0, s, d);
        launch_grad_test(d, it == h->iters_per_sync - 1, s);
    }
    return launched();
}

int32_t gcc_logreg_predict(const gcc_logreg_args *h, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream)
{
    const char *who = "gcc_logreg_predict";
    LrDev d;
    Plan pl;
    int rc = prepare(who, h, workspace, workspace_bytes, status, d, pl);
    if (rc) return rc;
    if ((rc = null_member(who, {{h->pred, "pred"}}))) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (h->counts) (void)hipMemsetAsync(h->counts, 0, (size_t)h->folds * 3 * sizeof(int32_t), s);
    hipLaunchKernelGGL(lr_finish_kernel, dim3(pl.P), dim3(64), 0, s, d);
    hipLaunchKernelGGL(lr_predict_kernel, dim3(h->N), dim3(kThreads), 0, s, d);
    return launched();
}

}  // extern "C"
