// gcc_amd/csrc/prone.hip -- ProNE node embeddings of a parent graph (gfx950): the baseline the reference's node classification
// compares the pre-trained encoder against (gcc/models/emb/prone.py; `baseline.sh 64 prone usa_airport`).
//
// Input: a simple undirected graph as symmetric CSR, rows sorted, no self loops.  All arithmetic is float64, k = d + 10.
//   1. node terms (l.56-76): r_i = -log(deg_i), s_j = sum_{i in N(j)} 1 / deg_i, c_j = -log(s_j^0.75 / sum_j s_j^0.75).  The
//      factorised matrix F has A's pattern and the values r_i + c_j; it is never stored.
//   2. sklearn's randomized_svd(F, d, n_iter=5) from a given Omega (l.32-41): 11 products and orthonormalisations for the range Q,
//      B^T = F^T Q, the top d eigenpairs of B B^T, U = Q U^, svd_flip, U sqrt(Sigma), rows L2-normalised.
//   3. the Chebyshev-Gaussian propagation (l.78-108): 2 (step - 1) products with M = (1 - mu) I - D1^-1 A1, A1 = I + A, then
//      mm = A1 (a - conv), the eigenpairs of mm^T mm, emb = mm V Sigma^-1/2 with the same sign rule, rows L2-normalised.
//
//   pr_rows_kernel       checks row_ptr; lists the rows longer than a chunk and reserves their parts' slots (integer atomics).
//   pr_terms_kernel      one wave per row: s (lanes strided over the row, then the wave's sum), r, s^0.75; checks col_idx.
//   pr_norm_kernel       one workgroup: sum s^0.75, threads strided, then the workgroup's sum.     pr_c_kernel: c.
//   pr_spmm_kernel       THE HOT PATH, y = op x with the tail fused: a group of G = 16 / 32 / 64 lanes per row, lane = column (and
//       column + 64 for k > 64), the neighbours' rows of x gathered through col_idx.  A row's sum is ordered by the row alone (the
//       binary counter of include/gcc_amd.h over segments of 32 neighbours: SumCounter of task_common.h).
//   pr_spmm_long_kernel  one group per part of a row longer than a chunk -> the workspace.
//   pr_spmm_comb_kernel  one group per such row: its parts by the same counter, then the same tail.
//   pr_gram_kernel       grid (upper-triangle 16 x 16 tile, row split): x^T x on v_mfma_f64_16x16x4_f64, four rows per instruction;
//       four waves take the row groups round robin and are added in wave order.
//   pr_chol_kernel       one workgroup: the splits in order, Cholesky in LDS, R and R^-1 (a pivot that is not positive: RANK).
//   pr_right_kernel      out = x W for a small W in LDS (x R^-1 in place, Q U^, mm V), rows staged through LDS; per workgroup and
//       column the entry of largest magnitude, lowest row first.
//   pr_eig_kernel        one workgroup: cyclic Jacobi in round-robin order (m / 2 disjoint rotations per step, matrix and vectors in
//       LDS), eigenvalues descending, the top d.
//   pr_sign_kernel       the column signs from the workgroups' entries in order, sqrt(sigma) scaling, the singular-value check.
//   pr_finish_kernel     scaled rows, L2-normalised (a zero row stays zero) -> float64 and float32.
// No floating-point atomics: every sum has one fixed order, which depends on the sizes alone (and not on the chunk).  The counter, the
// CSR guards, the Gram tile and the entry points' scaffold are task_common.h's.
#include "task_common.h"

#include <float.h>
#include <limits.h>
#include <math.h>

namespace {

constexpr int kThreads = 256, kWaves = 4;
constexpr int kSeg = GCC_PRONE_SEGMENT;
constexpr int kLv = 8;                        // counter levels inside a part
constexpr int kLvParts = 27;                  // counter levels over the parts of a row: at most 2^31 / 32 parts
constexpr int kMaxK = GCC_PRONE_MAX_K;
constexpr int kPartStride = 80;               // float64 of one part's sums
constexpr int kRightRows = 128;               // rows of one pr_right_kernel workgroup
constexpr int kStage = 1536;                  // float64 of staged rows: (256 / dout) * kin for kin <= dout + 10
constexpr int kMaxSweeps = 40;
constexpr int kFatal = GCC_STATUS_PRONE_BAD_CSR | GCC_STATUS_PRONE_SPLIT_FULL | GCC_STATUS_PRONE_RANK | GCC_STATUS_PRONE_SINGULAR;
static_assert((kSeg << (kLv - 1)) == GCC_PRONE_MAX_CHUNK, "the counter holds one part");
static_assert(kMaxK <= kPartStride && kMaxK <= 128, "two columns per lane");
static_assert(kWaves == kGramWaves, "pr_gram_kernel");

struct PrDev {
    const int32_t *rp, *ci;
    int32_t n, nnz, k, chunk, mode, tail, G, slot_cap;
    double mu, alpha, beta;
    const double *r, *c;                      // what the products read
    double *rw, *cw, *tot;                    // what the node terms write
    const double *x, *z, *w;
    double *y, *conv;
    int32_t *cnt, *long_row, *long_first, *slot_row, *slot_part;
    double *part;
    int32_t *status;
};

__device__ __forceinline__ bool fatal(const int32_t *status) { return (load_fresh_i32(status) & kFatal) != 0; }

// entries [e0, e1) of row i (e0 on a segment boundary of the row) for the columns c0 and, if on1, c0 + 64
__device__ __forceinline__ void range_sum(const PrDev &a, int i, int e0, int e1, int c0, bool on1, double (&s)[2])
{
    const double ri = a.mode == GCC_PRONE_MODE_F ? a.r[i] : 0.0, ci = a.mode == GCC_PRONE_MODE_FT ? a.c[i] : 0.0;
    auto segment = [&](int f0, int f1, double &t0, double &t1) {
        t0 = t1 = 0.0;
        for (int e = f0; e < f1; ++e) {
            const int j = a.ci[e];
            if ((unsigned)j >= (unsigned)a.n) {                     // (never read out of x)
                atomicOr(a.status, (int32_t)GCC_STATUS_PRONE_BAD_CSR);
                continue;
            }
            const long long o = (long long)j * a.k + c0;
            double x0 = a.x[o], x1 = on1 ? a.x[o + 64] : 0.0;
            if (a.mode == GCC_PRONE_MODE_F || a.mode == GCC_PRONE_MODE_FT) {
                const double wt = a.mode == GCC_PRONE_MODE_F ? ri + a.c[j] : a.r[j] + ci;
                t0 = fma(wt, x0, t0);
                t1 = fma(wt, x1, t1);
            } else {
                if (a.mode == GCC_PRONE_MODE_A1) {
                    x0 -= a.z[o];
                    if (on1) x1 -= a.z[o + 64];
                }
                t0 += x0;
                t1 += x1;
            }
        }
    };
    const int nseg = (e1 - e0 + kSeg - 1) / kSeg;
    if (nseg <= 1) {
        segment(e0, e1, s[0], s[1]);
        return;
    }
    SumCounter<kLv, 2> cn;
    for (int t = 0; t < nseg; ++t) {
        double t0, t1;
        segment(e0 + t * kSeg, min(e0 + (t + 1) * kSeg, e1), t0, t1);
        cn.push(t, {t0, t1});
    }
    s[0] = s[1] = 0.0;
    cn.fold(nseg, false, s);
}

// entry (i, c) of y from the row's sum t: the row's own term and the tail
__device__ __forceinline__ void finish_entry(const PrDev &a, int i, int deg, int c, double t)
{
    const long long o = (long long)i * a.k + c;
    double y;
    if (a.mode == GCC_PRONE_MODE_F || a.mode == GCC_PRONE_MODE_FT) y = t;
    else if (a.mode == GCC_PRONE_MODE_A1) y = (a.x[o] - a.z[o]) + t;
    else {
        const double inv = 1.0 / (double)(deg + 1), dc = (1.0 - inv) - a.mu;
        // (every multiply-add is an explicit fma: pr_spmm_kernel and pr_spmm_comb_kernel must round alike)
        const double m = fma(dc, a.x[o], -(inv * t));
        if (a.tail == GCC_PRONE_TAIL_HALF) {
            const double zi = a.z[o];
            y = fma(0.5, m, -zi);
            a.conv[o] = fma(a.beta, y, a.alpha * zi);
        } else if (a.tail == GCC_PRONE_TAIL_CHEB) {
            y = fma(-2.0, a.z[o], m) - a.w[o];                       // (y may be w: read before the store below)
            a.conv[o] = fma(a.alpha, y, a.conv[o]);
        } else y = m;
    }
    a.y[o] = y;
}

__global__ __launch_bounds__(kThreads) void pr_rows_kernel(PrDev a)
{
    const long long i64 = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i64 >= a.n) return;
    const int i = (int)i64;
    int b, e;
    if (!csr_row_range(a.rp, a.nnz, i, b, e) || !csr_ends_ok(a.rp, a.n, a.nnz, i)) {
        atomicOr(a.status, (int32_t)GCC_STATUS_PRONE_BAD_CSR);
        return;
    }
    const int deg = e - b;
    if (deg <= a.chunk) return;
    const int parts = (deg + a.chunk - 1) / a.chunk;
    const int l = atomicAdd(a.cnt, 1), f = atomicAdd(a.cnt + 1, parts);
    if (l >= a.slot_cap || f > a.slot_cap - parts) {
        atomicOr(a.status, (int32_t)GCC_STATUS_PRONE_SPLIT_FULL);
        return;
    }
    a.long_row[l] = i;
    a.long_first[l] = f;
    for (int p = 0; p < parts; ++p) {
        a.slot_row[f + p] = i;
        a.slot_part[f + p] = p;
    }
}

__global__ __launch_bounds__(kThreads) void pr_terms_kernel(PrDev a)
{
    const int lane = lane_id(), wv = (int)threadIdx.x >> 6;
    const long long i64 = (long long)blockIdx.x * kWaves + wv;
    if (i64 >= a.n) return;                                         // (the whole wave)
    const int i = (int)i64;
    int b, e;
    csr_row_range(a.rp, a.nnz, i, b, e);
    double s = 0.0;
    int bits = 0;
    for (int e0 = b; e0 < e; e0 += 64) {
        const int q = e0 + lane;
        if (q >= e) continue;
        if (csr_entry_bad(a.ci, b, q, i, a.n)) {
            bits |= GCC_STATUS_PRONE_BAD_CSR;
            continue;
        }
        const int j = a.ci[q];
        if (q > b && a.ci[q - 1] == j) bits |= GCC_STATUS_PRONE_DUPLICATE;
        int jb, je;
        if (csr_row_range(a.rp, a.nnz, j, jb, je) && je > jb) s += 1.0 / (double)(je - jb);
    }
    if (bits) atomicOr(a.status, (int32_t)bits);
    s = wave_sum(s);
    if (lane == 0) {
        a.rw[i] = -log((double)(e - b));                            // (an isolated node: +inf, never read)
        a.cw[i] = pow(s, 0.75);
    }
}

__global__ __launch_bounds__(kThreads) void pr_norm_kernel(PrDev a)
{
    __shared__ double red[kWaves];
    double acc = 0.0;
    for (int i = (int)threadIdx.x; i < a.n; i += kThreads) acc += a.cw[i];
    const double tot = block_sum<kWaves>(acc, red);
    if (threadIdx.x == 0) a.tot[0] = tot;
}

__global__ __launch_bounds__(kThreads) void pr_c_kernel(PrDev a)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i < a.n) a.cw[i] = -log(a.cw[i] / a.tot[0]);
}

__global__ __launch_bounds__(kThreads) void pr_spmm_kernel(PrDev a)
{
    if (fatal(a.status)) return;
    const int tid = (int)threadIdx.x, c0 = tid % a.G;
    const long long i64 = (long long)blockIdx.x * (kThreads / a.G) + tid / a.G;
    if (i64 >= a.n || c0 >= a.k) return;
    const int i = (int)i64;
    int b, e;
    csr_row_range(a.rp, a.nnz, i, b, e);
    if (e - b > a.chunk) return;                                    // (pr_spmm_long_kernel / pr_spmm_comb_kernel)
    const bool on1 = c0 + 64 < a.k;
    double s[2];
    range_sum(a, i, b, e, c0, on1, s);
    finish_entry(a, i, e - b, c0, s[0]);
    if (on1) finish_entry(a, i, e - b, c0 + 64, s[1]);
}

__global__ __launch_bounds__(kThreads) void pr_spmm_long_kernel(PrDev a)
{
    if (fatal(a.status)) return;
    const int tid = (int)threadIdx.x, c0 = tid % a.G;
    const long long slot = (long long)blockIdx.x * (kThreads / a.G) + tid / a.G;
    if (slot >= a.slot_cap || c0 >= a.k) return;
    const int i = a.slot_row[slot];
    if (i < 0) return;
    int b, e;
    csr_row_range(a.rp, a.nnz, i, b, e);
    const int e0 = b + a.slot_part[slot] * a.chunk, e1 = min(e0 + a.chunk, e);
    const bool on1 = c0 + 64 < a.k;
    double s[2];
    range_sum(a, i, e0, e1, c0, on1, s);
    a.part[slot * kPartStride + c0] = s[0];
    if (on1) a.part[slot * kPartStride + c0 + 64] = s[1];
}

__global__ __launch_bounds__(kThreads) void pr_spmm_comb_kernel(PrDev a)
{
    if (fatal(a.status)) return;
    const int tid = (int)threadIdx.x, c0 = tid % a.G;
    const long long l = (long long)blockIdx.x * (kThreads / a.G) + tid / a.G;
    if (l >= a.slot_cap || c0 >= a.k) return;
    const int i = a.long_row[l];
    if (i < 0) return;
    int b, e;
    csr_row_range(a.rp, a.nnz, i, b, e);
    const int deg = e - b, full = deg / a.chunk;
    const bool ragged = deg % a.chunk != 0, on1 = c0 + 64 < a.k;
    const double *part = a.part + (long long)a.long_first[l] * kPartStride + c0;
    SumCounter<kLvParts, 2> cn;
    for (int p = 0; p < full; ++p) cn.push(p, {part[(long long)p * kPartStride], on1 ? part[(long long)p * kPartStride + 64] : 0.0});
    double s[2] = {0.0, 0.0};
    if (ragged) {
        s[0] = part[(long long)full * kPartStride];
        s[1] = on1 ? part[(long long)full * kPartStride + 64] : 0.0;
    }
    cn.fold(full, ragged, s);
    finish_entry(a, i, deg, c0, s[0]);
    if (on1) finish_entry(a, i, deg, c0 + 64, s[1]);
}

// part[split][tile][256] = the split's rows of x^T x, a tile in row-major order
__global__ __launch_bounds__(kThreads) void pr_gram_kernel(const double *X, int n, int k, int T, int rps, double *part, const int32_t *status)
{
    __shared__ double red[kWaves][256];
    if (fatal(status)) return;
    const int tile = (int)blockIdx.x, split = (int)blockIdx.y, jl = lane_id() & 15;
    int ti, tj;
    tri_tile_of(tile, T, ti, tj);
    const int ca = 16 * ti + jl, cb = 16 * tj + jl;
    const int r0 = split * rps, r1 = min(n, r0 + rps);
    // A[jl][q] = x[row q][ca], B[q][jl] = x[row q][cb]
    const double h = gram_tile_f64(
        r0, r1, [&](int r, bool in) { return in && ca < k ? X[(long long)r * k + ca] : 0.0; },
        [&](int r, bool in) { return in && cb < k ? X[(long long)r * k + cb] : 0.0; }, red);
    part[((long long)split * gridDim.x + tile) * 256 + threadIdx.x] = h;
}

// entry (i, j), i <= j, of the Gram matrix: the splits in order
__device__ __forceinline__ double gram_entry(const double *part, int splits, int T, int i, int j)
{
    const int tiles = T * (T + 1) / 2;
    const long long at = (long long)tri_tile_index(i >> 4, j >> 4, T) * 256 + (i & 15) * 16 + (j & 15);
    double s = 0.0;
    for (int sp = 0; sp < splits; ++sp) s += part[(long long)sp * tiles * 256 + at];
    return s;
}

// x^T x = R^T R -> rinv = R^-1 and rfac = R, both [k][k] row-major with zeros below the diagonal
__global__ __launch_bounds__(kThreads) void pr_chol_kernel(const double *part, int splits, int k, int T, double *rinv, double *rfac,
                                                           int32_t *status)
{
    __shared__ double M[kMaxK * kMaxK];                             // lower triangle: L
    __shared__ double diag_s[kMaxK];
    if (fatal(status)) return;
    const int tid = (int)threadIdx.x, n = k;
    for (int e = tid; e < n * n; e += kThreads) {
        const int i = e / n, j = e % n;
        if (i > j) continue;
        const double h = gram_entry(part, splits, T, i, j);
        M[i * n + j] = h;
        M[j * n + i] = h;
    }
    __syncthreads();
    double md = 0.0;
    for (int i = 0; i < n; ++i) md = M[i * n + i] > md ? M[i * n + i] : md;
    const double thr = 8.0 * n * DBL_EPSILON * md;                  // below it a pivot is rounding: the columns are dependent
    __syncthreads();
    bool ok = true;
    for (int c = 0; c < n; ++c) {
        const double piv = M[c * n + c];
        if (!(piv > thr) || !(piv <= DBL_MAX)) { ok = false; break; }         // (workgroup-uniform: every thread reads the same pivot)
        const double l = sqrt(piv);
        if (tid == 0) diag_s[c] = l;
        for (int i = c + 1 + tid; i < n; i += kThreads) M[i * n + c] /= l;
        __syncthreads();
        const int m = n - c - 1;
        for (int e = tid; e < m * m; e += kThreads) {
            const int i = c + 1 + e / m, j = c + 1 + e % m;
            if (j <= i) M[i * n + j] -= M[i * n + c] * M[j * n + c];
        }
        __syncthreads();
    }
    if (!ok) {
        if (tid == 0) atomicOr(status, (int32_t)GCC_STATUS_PRONE_RANK);
        return;
    }
    // R[i][m] = L[m][i]; column j of R^-1 by back substitution, one thread per column (it reads back its own stores)
    if (tid < n) {
        const int j = tid;
        for (int i = n - 1; i > j; --i) rinv[i * n + j] = 0.0;
        rinv[j * n + j] = 1.0 / diag_s[j];
        for (int i = j - 1; i >= 0; --i) {
            double s = 0.0;
            for (int m = i + 1; m <= j; ++m) s = fma(M[m * n + i], rinv[m * n + j], s);
            rinv[i * n + j] = -s / diag_s[i];
        }
    }
    for (int e = tid; e < n * n; e += kThreads) {
        const int i = e / n, j = e % n;
        rfac[e] = i == j ? diag_s[i] : i < j ? M[j * n + i] : 0.0;
    }
}

// out[n][dout] = X[n][kin] W[kin][dout] (out may be X when dout == kin); cm_*[workgroup][64]: per column the entry of largest
// magnitude among the workgroup's rows, the lowest row first
__global__ __launch_bounds__(kThreads) void pr_right_kernel(const double *X, int n, int kin, const double *W, int dout, double *out,
                                                            double *cm_abs, double *cm_val, int32_t *cm_row, const int32_t *status)
{
    __shared__ double W_s[kMaxK * kMaxK];
    __shared__ double ys[kStage];
    __shared__ double ba[kThreads], bv[kThreads];
    __shared__ int32_t br[kThreads];
    if (fatal(status)) return;
    const int tid = (int)threadIdx.x;
    for (int e = tid; e < kin * dout; e += kThreads) W_s[e] = W[e];
    const int rbat = kThreads / dout, rl = tid / dout, j = tid % dout;
    const int r0 = (int)blockIdx.x * kRightRows, r1 = min(n, r0 + kRightRows);
    double best_abs = -1.0, best_val = 0.0;
    int best_row = INT_MAX;
    for (int c0 = r0; c0 < r1; c0 += rbat) {
        const int nr = min(rbat, r1 - c0);
        __syncthreads();                                            // (W_s is there; the rows before are used up)
        for (int e = tid; e < nr * kin; e += kThreads) ys[e] = X[(long long)c0 * kin + e];
        __syncthreads();
        if (rl < nr) {
            double s = 0.0;
            for (int i = 0; i < kin; ++i) s = fma(ys[rl * kin + i], W_s[i * dout + j], s);
            out[(long long)(c0 + rl) * dout + j] = s;
            if (fabs(s) > best_abs) {                                // (the thread's rows ascend: a tie keeps the lower)
                best_abs = fabs(s);
                best_val = s;
                best_row = c0 + rl;
            }
        }
    }
    if (!cm_abs) return;
    __syncthreads();
    ba[tid] = best_abs;
    bv[tid] = best_val;
    br[tid] = best_row;
    __syncthreads();
    if (tid < dout) {
        for (int t = 1; t < rbat; ++t) {
            const int o = t * dout + tid;
            if (ba[o] > best_abs || (ba[o] == best_abs && br[o] < best_row)) {
                best_abs = ba[o];
                best_val = bv[o];
                best_row = br[o];
            }
        }
        cm_abs[(long long)blockIdx.x * 64 + tid] = best_abs;
        cm_val[(long long)blockIdx.x * 64 + tid] = best_val;
        cm_row[(long long)blockIdx.x * 64 + tid] = best_row;
    }
}

// the top `dtop` eigenpairs of the m x m Gram matrix in `part`: W[m][dtop] (columns = vectors), ev[dtop] descending
__global__ __launch_bounds__(kThreads) void pr_eig_kernel(const double *part, int splits, int m, int T, int dtop, double *W, double *ev,
                                                          int32_t *status)
{
    DYN_SMEM(smem);
    __shared__ double c_s[kMaxK / 2 + 1], s_s[kMaxK / 2 + 1];
    __shared__ int32_t p_s[kMaxK / 2 + 1], q_s[kMaxK / 2 + 1];
    __shared__ int32_t rot_s;
    if (fatal(status)) return;
    const int tid = (int)threadIdx.x, m2 = m + (m & 1), np = m2 / 2;          // (an odd size gets a row and column of zeros)
    double *A = reinterpret_cast<double *>(smem), *V = A + m2 * m2;
    for (int e = tid; e < m2 * m2; e += kThreads) {
        const int i = e / m2, j = e % m2;
        A[e] = i < m && j < m ? gram_entry(part, splits, T, min(i, j), max(i, j)) : 0.0;
        V[e] = i == j ? 1.0 : 0.0;
    }
    __syncthreads();
    bool done = false;
    for (int sweep = 0; sweep < kMaxSweeps && !done; ++sweep) {
        if (tid == 0) rot_s = 0;
        __syncthreads();
        // round st of a round-robin tournament of m2 players: np disjoint pairs, every pair once in m2 - 1 rounds
        for (int st = 0; st < m2 - 1; ++st) {
            if (tid < np) {
                int p = tid == 0 ? m2 - 1 : (st + tid) % (m2 - 1), q = tid == 0 ? st : (st - tid + (m2 - 1)) % (m2 - 1);
                if (p > q) { const int t = p; p = q; q = t; }
                const double app = A[p * m2 + p], aqq = A[q * m2 + q], apq = A[p * m2 + q];
                double c = 1.0, s = 0.0;
                if (fabs(apq) > DBL_EPSILON * sqrt(fabs(app) * fabs(aqq)) && fabs(apq) > DBL_MIN) {
                    const double theta = (aqq - app) / (2.0 * apq);
                    const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    c = 1.0 / sqrt(t * t + 1.0);
                    s = t * c;
                    rot_s = 1;
                }
                p_s[tid] = p; q_s[tid] = q; c_s[tid] = c; s_s[tid] = s;
            }
            __syncthreads();
            for (int e = tid; e < np * m2; e += kThreads) {        // columns p and q of A and of V
                const int pr = e / m2, i = e % m2, p = p_s[pr], q = q_s[pr];
                const double c = c_s[pr], s = s_s[pr];
                if (s == 0.0) continue;
                const double aip = A[i * m2 + p], aiq = A[i * m2 + q], vip = V[i * m2 + p], viq = V[i * m2 + q];
                A[i * m2 + p] = c * aip - s * aiq;
                A[i * m2 + q] = s * aip + c * aiq;
                V[i * m2 + p] = c * vip - s * viq;
                V[i * m2 + q] = s * vip + c * viq;
            }
            __syncthreads();
            for (int e = tid; e < np * m2; e += kThreads) {        // rows p and q of A
                const int pr = e / m2, j = e % m2, p = p_s[pr], q = q_s[pr];
                const double c = c_s[pr], s = s_s[pr];
                if (s == 0.0) continue;
                const double apj = A[p * m2 + j], aqj = A[q * m2 + j];
                A[p * m2 + j] = j == q ? 0.0 : c * apj - s * aqj;
                A[q * m2 + j] = j == p ? 0.0 : s * apj + c * aqj;
            }
            __syncthreads();
        }
        done = rot_s == 0;
        __syncthreads();
    }
    if (!done && tid == 0) atomicOr(status, (int32_t)GCC_STATUS_PRONE_SWEEPS);
    if (tid < m) {
        const double lam = A[tid * m2 + tid];
        int rank = 0;
        for (int j = 0; j < m; ++j) {
            const double o = A[j * m2 + j];
            rank += o > lam || (o == lam && j < tid);
        }
        if (rank < dtop) {
            ev[rank] = lam;
            for (int r = 0; r < m; ++r) W[r * dtop + rank] = V[r * m2 + tid];
        }
    }
}

// scale[j] = sign_j sqrt(sigma_j) (the factorisation) or sign_j / sqrt(sigma_j) (the propagation: U sqrt(s) = mm V / sqrt(s))
__global__ __launch_bounds__(64) void pr_sign_kernel(const double *cm_abs, const double *cm_val, const int32_t *cm_row, int wgs, const double *ev,
                                                     int d, int n, int divide, double *scale, double *sigma, int32_t *status)
{
    if (fatal(status)) return;
    const int j = (int)threadIdx.x;
    if (j >= d) return;
    double best_abs = -1.0, best_val = 0.0;
    int best_row = INT_MAX;
    for (int g = 0; g < wgs; ++g) {
        const double ab = cm_abs[(long long)g * 64 + j];
        const int row = cm_row[(long long)g * 64 + j];
        if (ab > best_abs || (ab == best_abs && row < best_row)) {
            best_abs = ab;
            best_val = cm_val[(long long)g * 64 + j];
            best_row = row;
        }
    }
    const double s1 = sqrt(ev[0] > 0.0 ? ev[0] : 0.0), sj = sqrt(ev[j] > 0.0 ? ev[j] : 0.0);
    if (sigma) sigma[j] = sj;
    if (!(sj > (double)n * DBL_EPSILON * s1) || !(sj <= DBL_MAX)) {
        atomicOr(status, (int32_t)GCC_STATUS_PRONE_SINGULAR);
        scale[j] = 0.0;
        return;
    }
    const double sg = best_val < 0.0 ? -1.0 : 1.0;
    scale[j] = divide ? sg / sqrt(sj) : sg * sqrt(sj);
}

__global__ __launch_bounds__(kThreads) void pr_finish_kernel(const double *Z, int n, int d, int G, const double *scale, double *emb, float *emb32,
                                                             const int32_t *status)
{
    if (fatal(status)) return;
    const int tid = (int)threadIdx.x, c = tid % G;
    const long long row = (long long)blockIdx.x * (kThreads / G) + tid / G;
    const bool in = row < n && c < d;
    const double v = in ? Z[row * d + c] * scale[c] : 0.0;
    double ss = v * v;
    for (int o = G >> 1; o >= 1; o >>= 1) ss += wave_shfl_xor(ss, o);
    const double nrm = sqrt(ss), out = nrm > 0.0 ? v / nrm : 0.0;    // (a zero row stays zero)
    if (in) {
        emb[row * d + c] = out;
        if (emb32) emb32[row * d + c] = (float)out;
    }
}

struct Plan {
    int32_t k, T, tiles, splits, rps, slot_cap, right_wgs;
    int64_t off_r, off_c, off_tot, off_cnt, off_long_row, off_long_first, off_slot_row, off_slot_part, off_part, off_gpart, off_rinv,
        off_rfac, off_W, off_ev, off_scale, off_cm_abs, off_cm_val, off_cm_row, off_Z, off_area, total;
};

int lanes_per_row(int k) { return k <= 16 ? 16 : k <= 32 ? 32 : 64; }

// the row splits depend on the sizes alone, so a result does not depend on how the work was scheduled
Plan make_plan(int64_t n, int64_t nnz, int32_t d)
{
    Plan p;
    p.k = d + GCC_PRONE_OVERSAMPLE;
    p.T = (p.k + 15) / 16;
    p.tiles = p.T * (p.T + 1) / 2;
    int64_t splits = (n + 511) / 512;
    splits = splits < 1 ? 1 : splits > 256 ? 256 : splits;
    p.rps = (int32_t)((((n + splits - 1) / splits) + 31) & ~(int64_t)31);
    p.splits = (int32_t)((n + p.rps - 1) / p.rps);
    p.slot_cap = (int32_t)(2 * (nnz / GCC_PRONE_CHUNK) + 64);
    p.right_wgs = (int32_t)((n + kRightRows - 1) / kRightRows);
    Carve cv;
    const int64_t nk = n * p.k, nd = n * d;
    p.off_r = cv.take(n * 8);
    p.off_c = cv.take(n * 8);
    p.off_tot = cv.take(8);
    p.off_cnt = cv.take(8);
    p.off_long_row = cv.take((int64_t)p.slot_cap * 4);
    p.off_long_first = cv.take((int64_t)p.slot_cap * 4);
    p.off_slot_row = cv.take((int64_t)p.slot_cap * 4);
    p.off_slot_part = cv.take((int64_t)p.slot_cap * 4);
    p.off_part = cv.take((int64_t)p.slot_cap * kPartStride * 8);
    p.off_gpart = cv.take((int64_t)p.splits * p.tiles * 256 * 8);
    p.off_rinv = cv.take((int64_t)kMaxK * kMaxK * 8);
    p.off_rfac = cv.take((int64_t)kMaxK * kMaxK * 8);
    p.off_W = cv.take((int64_t)kMaxK * kMaxK * 8);
    p.off_ev = cv.take((int64_t)kMaxK * 8);
    p.off_scale = cv.take((int64_t)kMaxK * 8);
    p.off_cm_abs = cv.take((int64_t)p.right_wgs * 64 * 8);
    p.off_cm_val = cv.take((int64_t)p.right_wgs * 64 * 8);
    p.off_cm_row = cv.take((int64_t)p.right_wgs * 64 * 4);
    p.off_Z = cv.take(nd * 8);
    p.off_area = cv.take((2 * nk > 5 * nd ? 2 * nk : 5 * nd) * 8);
    p.total = cv.total();
    return p;
}

int check_sizes(const char *who, int64_t n, int64_t nnz, int32_t d)
{
    if (d < 2 || d > GCC_PRONE_MAX_DIM) {
        snprintf(g_err, kErrLen, "%s: d %d outside 2..GCC_PRONE_MAX_DIM (%d)", who, d, GCC_PRONE_MAX_DIM);
        return -3;
    }
    if (n > INT32_MAX || nnz > INT32_MAX || nnz < 0) {
        snprintf(g_err, kErrLen, "%s: n %lld and nnz %lld must fit int32", who, (long long)n, (long long)nnz);
        return -2;
    }
    if (n < d + GCC_PRONE_OVERSAMPLE) {
        snprintf(g_err, kErrLen, "%s: n %lld is less than d + %d (%d): the range finder is wider than the graph", who, (long long)n,
                 GCC_PRONE_OVERSAMPLE, d + GCC_PRONE_OVERSAMPLE);
        return -2;
    }
    return 0;
}

struct Ws {
    void *base;
    Plan pl;
    double *f64(int64_t off) const { return ws_at<double>(base, off); }
    int32_t *i32(int64_t off) const { return ws_at<int32_t>(base, off); }
};

// the checks every entry point shares; fills d and ws; rc < 0 names the member in g_err
int prepare(const char *who, const gcc_prone_args *h, void *workspace, int64_t workspace_bytes, int32_t *status, PrDev &d, Ws &ws)
{
    int rc = null_member(who, {{h, "args"}});
    if (rc) return rc;
    if ((rc = check_sizes(who, h->n, h->nnz, h->d))) return rc;
    if ((rc = null_member(who, {{status, "status"}, {h->row_ptr, "row_ptr"}, {h->col_idx, "col_idx", h->nnz > 0}}))) return rc;
    int32_t chunk = h->chunk == 0 ? GCC_PRONE_CHUNK : h->chunk;
    if (chunk < GCC_PRONE_SEGMENT || chunk > GCC_PRONE_MAX_CHUNK || (chunk & (chunk - 1)) != 0) {
        snprintf(g_err, kErrLen, "%s: chunk %d must be 0 or GCC_PRONE_SEGMENT (%d) times a power of two, at most GCC_PRONE_MAX_CHUNK (%d)",
                 who, h->chunk, GCC_PRONE_SEGMENT, GCC_PRONE_MAX_CHUNK);
        return -4;
    }
    ws.pl = make_plan(h->n, h->nnz, h->d);
    if ((rc = check_workspace(who, "gcc_prone_workspace_bytes", workspace, workspace_bytes, ws.pl.total))) return rc;
    ws.base = workspace;
    const Plan &pl = ws.pl;
    d = PrDev();
    d.rp = h->row_ptr; d.ci = h->col_idx; d.n = (int32_t)h->n; d.nnz = (int32_t)h->nnz; d.chunk = chunk; d.slot_cap = pl.slot_cap;
    d.mu = h->mu; d.alpha = h->alpha; d.beta = h->beta;
    d.rw = h->r ? h->r : ws.f64(pl.off_r); d.cw = h->c ? h->c : ws.f64(pl.off_c); d.r = d.rw; d.c = d.cw; d.tot = ws.f64(pl.off_tot);
    d.cnt = ws.i32(pl.off_cnt); d.long_row = ws.i32(pl.off_long_row); d.long_first = ws.i32(pl.off_long_first);
    d.slot_row = ws.i32(pl.off_slot_row); d.slot_part = ws.i32(pl.off_slot_part); d.part = ws.f64(pl.off_part);
    d.status = status;
    return 0;
}

int check_k(const char *who, const gcc_prone_args *h)
{
    if (h->k < 1 || h->k > h->d + GCC_PRONE_OVERSAMPLE) {
        snprintf(g_err, kErrLen, "%s: k %d outside 1..d + %d (%d): the workspace is sized for d", who, h->k, GCC_PRONE_OVERSAMPLE,
                 h->d + GCC_PRONE_OVERSAMPLE);
        return -5;
    }
    return 0;
}

// row_ptr's checks and the lists of the rows longer than a chunk
void launch_rows(const PrDev &d, hipStream_t s)
{
    (void)hipMemsetAsync(d.cnt, 0, 8, s);
    (void)hipMemsetAsync(d.long_row, 0xFF, (size_t)d.slot_cap * 4, s);
    (void)hipMemsetAsync(d.slot_row, 0xFF, (size_t)d.slot_cap * 4, s);
    hipLaunchKernelGGL(pr_rows_kernel, dim3((d.n + kThreads - 1) / kThreads), dim3(kThreads), 0, s, d);
}

void launch_terms(const PrDev &d, hipStream_t s)
{
    hipLaunchKernelGGL(pr_terms_kernel, dim3((d.n + kWaves - 1) / kWaves), dim3(kThreads), 0, s, d);
    hipLaunchKernelGGL(pr_norm_kernel, dim3(1), dim3(kThreads), 0, s, d);
    hipLaunchKernelGGL(pr_c_kernel, dim3((d.n + kThreads - 1) / kThreads), dim3(kThreads), 0, s, d);
}

void launch_spmm(PrDev d, int mode, int tail, int k, const double *x, const double *z, const double *w, double *y, double *conv,
                 hipStream_t s)
{
    d.mode = mode; d.tail = tail; d.k = k; d.G = lanes_per_row(k);
    d.x = x; d.z = z; d.w = w; d.y = y; d.conv = conv;
    const int per = kThreads / d.G;
    hipLaunchKernelGGL(pr_spmm_kernel, dim3((d.n + per - 1) / per), dim3(kThreads), 0, s, d);
    hipLaunchKernelGGL(pr_spmm_long_kernel, dim3((d.slot_cap + per - 1) / per), dim3(kThreads), 0, s, d);
    hipLaunchKernelGGL(pr_spmm_comb_kernel, dim3((d.slot_cap + per - 1) / per), dim3(kThreads), 0, s, d);
}

void launch_gram(const Ws &ws, const double *X, int n, int k, int32_t *status, hipStream_t s)
{
    const int T = (k + 15) / 16;
    hipLaunchKernelGGL(pr_gram_kernel, dim3(T * (T + 1) / 2, ws.pl.splits), dim3(kThreads), 0, s, X, n, k, T, ws.pl.rps,
                       ws.f64(ws.pl.off_gpart), (const int32_t *)status);
}

void launch_right(const Ws &ws, const double *X, int n, int kin, const double *W, int dout, double *out, bool colmax, int32_t *status,
                  hipStream_t s)
{
    hipLaunchKernelGGL(pr_right_kernel, dim3(ws.pl.right_wgs), dim3(kThreads), 0, s, X, n, kin, W, dout, out,
                       colmax ? ws.f64(ws.pl.off_cm_abs) : (double *)nullptr, ws.f64(ws.pl.off_cm_val), ws.i32(ws.pl.off_cm_row),
                       (const int32_t *)status);
}

// CholeskyQR2 of Y [n][k] in place; rfac: [2][k][k] of the caller's or nullptr
void launch_orth(const Ws &ws, double *Y, int n, int k, double *rfac, int32_t *status, hipStream_t s)
{
    const int T = (k + 15) / 16;
    for (int pass = 0; pass < 2; ++pass) {
        launch_gram(ws, Y, n, k, status, s);
        hipLaunchKernelGGL(pr_chol_kernel, dim3(1), dim3(kThreads), 0, s, (const double *)ws.f64(ws.pl.off_gpart), ws.pl.splits, k, T,
                           ws.f64(ws.pl.off_rinv), rfac ? rfac + (size_t)pass * k * k : ws.f64(ws.pl.off_rfac), status);
        launch_right(ws, Y, n, k, ws.f64(ws.pl.off_rinv), k, Y, false, status, s);
    }
}

// the top d eigenpairs of S^T S for S [n][m], Z = X W for X [n][m], the signs and scales, the normalised rows
void launch_finish(const Ws &ws, const double *S, const double *X, int n, int m, int d, bool divide, double *sigma, double *emb,
                   float *emb32, int32_t *status, hipStream_t s)
{
    const int T = (m + 15) / 16, m2 = m + (m & 1);
    const size_t lds = (size_t)2 * m2 * m2 * sizeof(double);
    launch_gram(ws, S, n, m, status, s);
#ifndef GCC_AMD_HIPEMU
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void *)pr_eig_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
#endif
    hipLaunchKernelGGL(pr_eig_kernel, dim3(1), dim3(kThreads), lds, s, (const double *)ws.f64(ws.pl.off_gpart), ws.pl.splits, m, T, d,
                       ws.f64(ws.pl.off_W), ws.f64(ws.pl.off_ev), status);
    launch_right(ws, X, n, m, ws.f64(ws.pl.off_W), d, ws.f64(ws.pl.off_Z), true, status, s);
    hipLaunchKernelGGL(pr_sign_kernel, dim3(1), dim3(64), 0, s, (const double *)ws.f64(ws.pl.off_cm_abs),
                       (const double *)ws.f64(ws.pl.off_cm_val), (const int32_t *)ws.i32(ws.pl.off_cm_row), ws.pl.right_wgs,
                       (const double *)ws.f64(ws.pl.off_ev), d, n, divide ? 1 : 0, ws.f64(ws.pl.off_scale), sigma, status);
    const int G = lanes_per_row(d), per = kThreads / G;
    hipLaunchKernelGGL(pr_finish_kernel, dim3((n + per - 1) / per), dim3(kThreads), 0, s, (const double *)ws.f64(ws.pl.off_Z), n, d, G,
                       (const double *)ws.f64(ws.pl.off_scale), emb, emb32, (const int32_t *)status);
}

}  // namespace

extern "C" {

int64_t gcc_prone_workspace_bytes(int64_t n, int64_t nnz, int32_t d)
{
    const int rc = check_sizes("gcc_prone_workspace_bytes", n, nnz, d);
    if (rc) return rc;
    return make_plan(n, nnz, d).total;
}

int32_t gcc_prone_node_terms(const gcc_prone_args *h, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream)
{
    PrDev d;
    Ws ws;
    const int rc = prepare("gcc_prone_node_terms", h, workspace, workspace_bytes, status, d, ws);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    launch_rows(d, s);
    launch_terms(d, s);
    return launched();
}

int32_t gcc_prone_spmm(const gcc_prone_args *h, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream)
{
    const char *who = "gcc_prone_spmm";
    PrDev d;
    Ws ws;
    int rc = prepare(who, h, workspace, workspace_bytes, status, d, ws);
    if (rc) return rc;
    if ((rc = check_k(who, h))) return rc;
    if (h->mode < GCC_PRONE_MODE_F || h->mode > GCC_PRONE_MODE_A1 || h->tail < GCC_PRONE_TAIL_NONE || h->tail > GCC_PRONE_TAIL_CHEB ||
        (h->tail != GCC_PRONE_TAIL_NONE && h->mode != GCC_PRONE_MODE_M)) {
        snprintf(g_err, kErrLen, "%s: mode %d / tail %d: a tail goes with GCC_PRONE_MODE_M alone", who, h->mode, h->tail);
        return -6;
    }
    const bool need_z = h->mode == GCC_PRONE_MODE_A1 || h->tail != GCC_PRONE_TAIL_NONE, need_w = h->tail == GCC_PRONE_TAIL_CHEB;
    const bool need_conv = h->tail != GCC_PRONE_TAIL_NONE;
    if ((rc = null_member(who, {{h->x, "x"}, {h->y, "y"}, {h->z, "z", need_z}, {h->w, "w", need_w}, {h->conv, "conv", need_conv}}))) return rc;
    if (h->x == h->y) {
        snprintf(g_err, kErrLen, "%s: y must not be x (rows of x are gathered while y is written)", who);
        return -7;
    }
    hipStream_t s = (hipStream_t)stream;
    launch_rows(d, s);
    launch_spmm(d, h->mode, h->tail, h->k, h->x, h->z, h->w, h->y, h->conv, s);
    return launched();
}

int32_t gcc_prone_orthonormalize(const gcc_prone_args *h, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream)
{
    const char *who = "gcc_prone_orthonormalize";
    PrDev d;
    Ws ws;
    int rc = prepare(who, h, workspace, workspace_bytes, status, d, ws);
    if (rc) return rc;
    if ((rc = check_k(who, h))) return rc;
    if ((rc = null_member(who, {{h->y, "y"}}))) return rc;
    launch_orth(ws, h->y, d.n, h->k, h->rfac, status, (hipStream_t)stream);
    return launched();
}

int32_t gcc_prone_embed(const gcc_prone_args *h, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream)
{
    const char *who = "gcc_prone_embed";
    PrDev d;
    Ws ws;
    int rc = prepare(who, h, workspace, workspace_bytes, status, d, ws);
    if (rc) return rc;
    if (h->step < 1 || h->step > GCC_PRONE_MAX_STEP) {
        snprintf(g_err, kErrLen, "%s: step %d outside 1..GCC_PRONE_MAX_STEP (%d)", who, h->step, GCC_PRONE_MAX_STEP);
        return -6;
    }
    if ((rc = null_member(who, {{h->omega, "omega"}, {h->emb, "emb"}, {h->emb32, "emb32"}}))) return rc;
    hipStream_t s = (hipStream_t)stream;
    const Plan &pl = ws.pl;
    const int n = d.n, dd = h->d, k = pl.k;
    const int64_t nk = (int64_t)n * k, nd = (int64_t)n * dd;
    (void)hipMemsetAsync(h->emb, 0, (size_t)nd * 8, s);
    (void)hipMemsetAsync(h->emb32, 0, (size_t)nd * 4, s);
    if (h->sigma) (void)hipMemsetAsync(h->sigma, 0, (size_t)2 * dd * 8, s);
    launch_rows(d, s);
    launch_terms(d, s);
    // ---- the range of F: Q = Omega; five rounds of orth(F Q), orth(F^T Q); then orth(F Q)
    double *b0 = ws.f64(pl.off_area), *b1 = b0 + nk;
    const double *cur = h->omega;
    for (int it = 0; it < GCC_PRONE_POWER_ITERS; ++it) {
        launch_spmm(d, GCC_PRONE_MODE_F, 0, k, cur, nullptr, nullptr, b0, nullptr, s);
        launch_orth(ws, b0, n, k, nullptr, status, s);
        launch_spmm(d, GCC_PRONE_MODE_FT, 0, k, b0, nullptr, nullptr, b1, nullptr, s);
        launch_orth(ws, b1, n, k, nullptr, status, s);
        cur = b1;
    }
    launch_spmm(d, GCC_PRONE_MODE_F, 0, k, cur, nullptr, nullptr, b0, nullptr, s);
    launch_orth(ws, b0, n, k, nullptr, status, s);
    // ---- B^T = F^T Q; B B^T = U^ S^2 U^^T; U = Q U^
    launch_spmm(d, GCC_PRONE_MODE_FT, 0, k, b0, nullptr, nullptr, b1, nullptr, s);
    launch_finish(ws, b1, b0, n, k, dd, false, h->sigma, h->emb, h->emb32, status, s);
    if (h->step > 1) {
        // ---- the propagation (prone.py l.89-106); a = emb, and the iterates take the place of the range finder's
        double *t = ws.f64(pl.off_area), *la = t + nd, *lb = la + nd, *conv = lb + nd, *mm = conv + nd;
        const double *a = h->emb;
        launch_spmm(d, GCC_PRONE_MODE_M, GCC_PRONE_TAIL_NONE, dd, a, nullptr, nullptr, t, nullptr, s);
        d.alpha = h->bessel[0];
        d.beta = -2.0 * h->bessel[1];
        launch_spmm(d, GCC_PRONE_MODE_M, GCC_PRONE_TAIL_HALF, dd, t, a, nullptr, la, conv, s);
        const double *l0 = a;
        double *l1 = la;
        for (int i = 2; i < h->step; ++i) {
            launch_spmm(d, GCC_PRONE_MODE_M, GCC_PRONE_TAIL_NONE, dd, l1, nullptr, nullptr, t, nullptr, s);
            double *l2 = i == 2 ? lb : const_cast<double *>(l0);   // (a stays; later the oldest iterate is overwritten in place)
            d.alpha = (i % 2 == 0 ? 2.0 : -2.0) * h->bessel[i];
            launch_spmm(d, GCC_PRONE_MODE_M, GCC_PRONE_TAIL_CHEB, dd, t, l1, l0, l2, conv, s);
            l0 = l1;
            l1 = l2;
        }
        launch_spmm(d, GCC_PRONE_MODE_A1, 0, dd, a, conv, nullptr, mm, nullptr, s);
        launch_finish(ws, mm, mm, n, dd, dd, true, h->sigma ? h->sigma + dd : nullptr, h->emb, h->emb32, status, s);
    }
    return launched();
}

}  // extern "C"
