// gcc_amd/csrc/graphwave.hip -- GraphWave node embeddings of a parent graph (gfx950): the second baseline the reference's node
// classification and similarity search compare the pre-trained encoder against (gcc/models/emb/graphwave.py, as it is called there:
// automatic scales, Chebyshev order 30, two filters).
//
// Input: an undirected graph as symmetric CSR, rows sorted, no self loops; a repeated entry is a parallel edge.  All arithmetic is
// float64.  n = the rows that have an entry; an empty row is a node id outside the graph.
//   M = -D^-1/2 A D^-1/2;  H_i = sum_k coeff[i][k] T_k(M);  H_i = H_i > threshold / n ? H_i : 0;
//   chi[u][i 2T + 2j] = (sum_v cos(t_j H_i[v][u])) / n,  chi[u][i 2T + 2j + 1] = (sum_v sin(t_j H_i[v][u])) / n.
// Nothing of size n x n is kept: the source columns are taken in panels of W, [n_rows][W] row-major, lane = column.
//
//   gw_scale_kernel   one wave per row: checks row_ptr and col_idx, dinv_i = 1 / sqrt(row length), counts the live rows (integer atomic).
//   gw_init_kernel    orders 0 and 1 of a panel: X0 = the identity's columns, X1 = M's own columns (the multiplicity of u in row i by two
//       binary searches), Ha / Hb = c[0] X0 + c[1] X1.
//   gw_step_kernel    THE HOT PATH, one launch per order k >= 2: X_k = 2 M X_{k-1} - X_{k-2} written over X_{k-2} (a thread reads only
//       its own entry of it), the neighbours' rows of X_{k-1} gathered through col_idx, one coalesced read per neighbour and wave;
//       Ha += c_a[k] X_k, Hb += c_b[k] X_k in the same launch.  A row's sum is ordered by the row alone (the binary counter of
//       include/gcc_amd.h over segments of 32 neighbours: SumCounter of task_common.h).
//   gw_char_kernel    grid (column tile, block of 128 rows, filter x group of 8 time points): threshold, sincos per time point; a wave sums
//       32 rows left to right, the four waves are added as (0 + 1) + (2 + 3) -> the block's partial sums in the workspace.
//   gw_table_kernel   per column and table entry the blocks by the same counter, / n -> chi and, rounded once, chi32.
//   gw_heat_kernel    the two thresholded panels -> args.heat (the stage tests).
// No floating-point atomics: every sum has one fixed order, which depends on n_rows and the row alone (never on W or the grid).  The
// counter, the CSR guards and the entry points' scaffold are task_common.h's.
#include "task_common.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int kThreads = 256, kWaves = 4;
constexpr int kSeg = GCC_PRONE_SEGMENT;
constexpr int kLvRow = 27;                    // counter levels over a row's segments: at most 2^31 / 32 of them
constexpr int kLvBlocks = 10;                 // counter levels over the row blocks: at most 65,536 / 128 = 512 of them
constexpr int kOrder = GCC_GRAPHWAVE_ORDER;
constexpr int kMaxT = GCC_GRAPHWAVE_MAX_DIM / 4;
constexpr int kRowBlock = GCC_GRAPHWAVE_ROW_BLOCK, kRun = kRowBlock / kWaves;
constexpr int kTg = 8;                        // time points of one gw_char_kernel workgroup
constexpr int kDefaultMaxWidth = 2048;
constexpr int64_t kDefaultBudget = (int64_t)256 << 20;
static_assert(GCC_GRAPHWAVE_MAX_NODES <= (kRowBlock << (kLvBlocks - 1)), "the counter holds every row block");
static_assert(kRun == 32, "a wave's run of rows");

struct GwDev {
    const int32_t *rp, *ci;
    int32_t n_rows, nnz, W, col0, ncols;      // ncols: the panel's columns that are node ids
    double *dinv;
    int32_t *nlive;
    double *xa, *xb, *ha, *hb;                // xa: X_{k-2} in, X_k out; xb: X_{k-1}
    double ca, cb;                            // this order's coefficients
    int32_t *status;
};

struct GwInit {
    double c[2][2];
};

struct GwChar {
    double t[kMaxT];
    double threshold;
    int32_t T, d, groups;
    double *part;
};

__device__ __forceinline__ bool fatal(const int32_t *status) { return (load_fresh_i32(status) & GCC_STATUS_GRAPHWAVE_BAD_CSR) != 0; }

__global__ __launch_bounds__(kThreads) void gw_scale_kernel(GwDev a)
{
    const int lane = lane_id(), wv = (int)threadIdx.x >> 6;
    const long long i64 = (long long)blockIdx.x * kWaves + wv;
    if (i64 >= a.n_rows) return;                                    // (the whole wave)
    const int i = (int)i64;
    int b, e;
    const bool ok = csr_row_range(a.rp, a.nnz, i, b, e) && csr_ends_ok(a.rp, a.n_rows, a.nnz, i);
    int bits = ok ? 0 : GCC_STATUS_GRAPHWAVE_BAD_CSR;
    for (int e0 = b; e0 < e; e0 += 64) {
        const int q = e0 + lane;
        if (q >= e) continue;
        if (csr_entry_bad(a.ci, b, q, i, a.n_rows)) bits |= GCC_STATUS_GRAPHWAVE_BAD_CSR;
    }
    if (bits) atomicOr(a.status, (int32_t)bits);
    if (lane == 0) {
        const int deg = e - b;
        a.dinv[i] = deg > 0 ? 1.0 / sqrt((double)deg) : 0.0;
        if (deg > 0) atomicAdd(a.nlive, 1);
    }
}

// how often u stands in the sorted row [b, e)
__device__ __forceinline__ int multiplicity(const int32_t *ci, int b, int e, int u)
{
    int lo = b, hi = e;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ci[mid] < u) lo = mid + 1;
        else hi = mid;
    }
    const int first = lo;
    hi = e;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ci[mid] <= u) lo = mid + 1;
        else hi = mid;
    }
    return lo - first;
}

__global__ __launch_bounds__(kThreads) void gw_init_kernel(GwDev a, GwInit in)
{
    if (fatal(a.status)) return;
    const int c = (int)(blockIdx.x * 64 + (threadIdx.x & 63));
    const long long i64 = (long long)blockIdx.y * kWaves + (threadIdx.x >> 6);
    if (i64 >= a.n_rows || c >= a.ncols) return;
    const int i = (int)i64, u = a.col0 + c;
    int b, e;
    csr_row_range(a.rp, a.nnz, i, b, e);
    const double x0 = i == u ? 1.0 : 0.0;
    const int m = multiplicity(a.ci, b, e, u);
    const double x1 = m ? -(a.dinv[i] * ((double)m * a.dinv[u])) : 0.0;
    const long long o = (long long)i * a.W + c;
    a.xa[o] = x0;
    a.xb[o] = x1;
    a.ha[o] = fma(in.c[0][1], x1, in.c[0][0] * x0);
    a.hb[o] = fma(in.c[1][1], x1, in.c[1][0] * x0);
}

__global__ __launch_bounds__(kThreads) void gw_step_kernel(GwDev a)
{
    if (fatal(a.status)) return;
    const int c = (int)(blockIdx.x * 64 + (threadIdx.x & 63));
    const long long i64 = (long long)blockIdx.y * kWaves + (threadIdx.x >> 6);
    if (i64 >= a.n_rows) return;                                    // (the whole wave)
    const int i = wave_uniform((int)i64);                           // (a wave is one row: its entries and scales come by scalar loads)
    if (c >= a.ncols) return;
    int b, e;
    csr_row_range(a.rp, a.nnz, i, b, e);
    const double *x = a.xb + c;
    auto segment = [&](int f0, int f1) {
        double t = 0.0;
        for (int f = f0; f < f1; ++f) {
            const int j = a.ci[f];                                  // (in range: gw_scale_kernel checked every entry, or the call ended)
            t = fma(a.dinv[j], x[(long long)j * a.W], t);
        }
        return t;
    };
    const int nseg = (e - b + kSeg - 1) / kSeg;
    double s;
    if (nseg <= 1) s = segment(b, e);
    else {
        SumCounter<kLvRow, 1> cn;
        for (int t = 0; t < nseg; ++t) cn.push(t, {segment(b + t * kSeg, min(b + (t + 1) * kSeg, e))});
        s = cn.fold(nseg);
    }
    const long long o = (long long)i * a.W + c;
    const double xk = fma(-2.0 * a.dinv[i], s, -a.xa[o]);
    a.xa[o] = xk;
    a.ha[o] = fma(a.ca, xk, a.ha[o]);
    a.hb[o] = fma(a.cb, xk, a.hb[o]);
}

__global__ __launch_bounds__(kThreads) void gw_char_kernel(GwDev a, GwChar ch)
{
    __shared__ double red[kWaves][2 * kTg][64];
    if (fatal(a.status)) return;
    const int lane = lane_id(), wv = (int)threadIdx.x >> 6;
    const int c = (int)blockIdx.x * 64 + lane, rb = (int)blockIdx.y, filt = (int)blockIdx.z / ch.groups, j0 = ((int)blockIdx.z % ch.groups) * kTg;
    const int nlive = *a.nlive;
    const double thr = ch.threshold / (double)nlive;
    const double *h = filt ? a.hb : a.ha;
    const bool on = c < a.ncols && a.dinv[a.col0 + (c < a.ncols ? c : 0)] > 0.0;
    double cs[kTg], sn[kTg];
#pragma unroll
    for (int q = 0; q < kTg; ++q) cs[q] = sn[q] = 0.0;
    const int r0 = rb * kRowBlock + wv * kRun, r1 = min(r0 + kRun, a.n_rows);
    if (on) {
        for (int v = r0; v < r1; ++v) {
            if (!(a.dinv[v] > 0.0)) continue;                       // (a node id outside the graph: wave-uniform)
            double x = h[(long long)v * a.W + c];
            x = x > thr ? x : 0.0;
#pragma unroll
            for (int q = 0; q < kTg; ++q) {
                if (j0 + q >= ch.T) continue;
                double sv = 0.0, cv = 1.0;
                if (x != 0.0) sincos(ch.t[j0 + q] * x, &sv, &cv);
                cs[q] += cv;
                sn[q] += sv;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < kTg; ++q) {
        red[wv][2 * q][lane] = cs[q];
        red[wv][2 * q + 1][lane] = sn[q];
    }
    __syncthreads();
    if (!on) return;
    for (int q = wv; q < 2 * kTg; q += kWaves) {
        const int j = j0 + (q >> 1);
        if (j >= ch.T) continue;
        const double s = (red[0][q][lane] + red[1][q][lane]) + (red[2][q][lane] + red[3][q][lane]);
        const int entry = filt * 2 * ch.T + 2 * j + (q & 1);
        ch.part[((long long)rb * ch.d + entry) * a.W + c] = s;
    }
}

__global__ __launch_bounds__(kThreads) void gw_table_kernel(GwDev a, const double *part, int d, int blocks, double *chi, float *chi32)
{
    if (fatal(a.status)) return;
    const int c = (int)blockIdx.x * 64 + (int)(threadIdx.x & 63), entry = (int)blockIdx.y * kWaves + (int)(threadIdx.x >> 6);
    if (c >= a.ncols || entry >= d) return;
    const int u = a.col0 + c;
    if (!(a.dinv[u] > 0.0)) return;                                 // (its row keeps the zeros put there first)
    SumCounter<kLvBlocks, 1> cn;
    for (int rb = 0; rb < blocks; ++rb) cn.push(rb, {part[((long long)rb * d + entry) * a.W + c]});
    const double v = cn.fold(blocks) / (double)*a.nlive;
    chi[(long long)u * d + entry] = v;
    chi32[(long long)u * d + entry] = (float)v;
}

__global__ __launch_bounds__(kThreads) void gw_heat_kernel(GwDev a, double threshold, double *heat)
{
    if (fatal(a.status)) return;
    const int c = (int)(blockIdx.x * 64 + (threadIdx.x & 63));
    const long long i64 = (long long)blockIdx.y * kWaves + (threadIdx.x >> 6);
    if (i64 >= a.n_rows || c >= a.W) return;
    const int i = (int)i64;
    const double thr = threshold / (double)*a.nlive;
    const long long o = (long long)i * a.W + c, plane = (long long)a.n_rows * a.W;
    const bool on = c < a.ncols && a.dinv[i] > 0.0 && a.dinv[a.col0 + (c < a.ncols ? c : 0)] > 0.0;
    const double xa = on ? a.ha[o] : 0.0, xb = on ? a.hb[o] : 0.0;
    heat[o] = xa > thr ? xa : 0.0;
    heat[plane + o] = xb > thr ? xb : 0.0;
}

struct Plan {
    int32_t W, blocks;
    int64_t off_dinv, off_nlive, off_x, off_part, panel, total;
};

int64_t round64(int64_t x) { return (x + 63) & ~(int64_t)63; }

int check_sizes(const char *who, int64_t n_rows, int64_t nnz, int32_t d, int32_t width)
{
    if (d < 4 || d > GCC_GRAPHWAVE_MAX_DIM || d % 4 != 0) {
        snprintf(g_err, kErrLen, "%s: d %d must be a multiple of 4 in 4..GCC_GRAPHWAVE_MAX_DIM (%d)", who, d, GCC_GRAPHWAVE_MAX_DIM);
        return -3;
    }
    if (n_rows < 2 || n_rows > GCC_GRAPHWAVE_MAX_NODES) {
        snprintf(g_err, kErrLen, "%s: n_rows %lld outside 2..GCC_GRAPHWAVE_MAX_NODES (%d): the n_rows^2 work is not served above it", who,
                 (long long)n_rows, GCC_GRAPHWAVE_MAX_NODES);
        return -2;
    }
    if (nnz < 0 || nnz > INT32_MAX) {
        snprintf(g_err, kErrLen, "%s: nnz %lld must fit int32", who, (long long)nnz);
        return -2;
    }
    if (width < 0 || width > GCC_GRAPHWAVE_MAX_WIDTH || width % 64 != 0) {
        snprintf(g_err, kErrLen, "%s: width %d must be 0 or a multiple of 64 up to GCC_GRAPHWAVE_MAX_WIDTH (%d)", who, width,
                 GCC_GRAPHWAVE_MAX_WIDTH);
        return -4;
    }
    return 0;
}

int64_t row_blocks(int64_t n_rows) { return (n_rows + kRowBlock - 1) / kRowBlock; }

int32_t panel_width(int64_t n_rows, int32_t d, int32_t width)
{
    if (width) return width;
    const int64_t per_column = n_rows * 32 + row_blocks(n_rows) * d * 8;
    int64_t w = kDefaultBudget / per_column / 64 * 64;
    w = w < 64 ? 64 : w > kDefaultMaxWidth ? kDefaultMaxWidth : w;
    return (int32_t)(w < round64(n_rows) ? w : round64(n_rows));
}

Plan make_plan(int64_t n_rows, int32_t d, int32_t width)
{
    Plan p;
    p.W = panel_width(n_rows, d, width);
    p.blocks = (int32_t)row_blocks(n_rows);
    Carve cv;
    p.panel = n_rows * p.W * 8;
    p.off_dinv = cv.take(n_rows * 8);
    p.off_nlive = cv.take(8);
    p.off_x = cv.take(4 * p.panel);
    p.off_part = cv.take((int64_t)p.blocks * d * p.W * 8);
    p.total = cv.total();
    return p;
}

// the checks both entry points share; fills dv and pl; rc < 0 names the member in g_err
int prepare(const char *who, const gcc_graphwave_args *h, void *workspace, int64_t workspace_bytes, int32_t *status, GwDev &dv, Plan &pl)
{
    int rc = null_member(who, {{h, "args"}});
    if (rc) return rc;
    if ((rc = check_sizes(who, h->n_rows, h->nnz, h->d, h->width))) return rc;
    if ((rc = null_member(who, {{status, "status"}, {h->row_ptr, "row_ptr"}, {h->col_idx, "col_idx", h->nnz > 0}}))) return rc;
    pl = make_plan(h->n_rows, h->d, h->width);
    if ((rc = check_workspace(who, "gcc_graphwave_workspace_bytes", workspace, workspace_bytes, pl.total))) return rc;
    dv = GwDev();
    dv.rp = h->row_ptr; dv.ci = h->col_idx; dv.n_rows = (int32_t)h->n_rows; dv.nnz = (int32_t)h->nnz; dv.W = pl.W;
    dv.dinv = ws_at<double>(workspace, pl.off_dinv);
    dv.nlive = ws_at<int32_t>(workspace, pl.off_nlive);
    double *x = ws_at<double>(workspace, pl.off_x);
    const int64_t pe = pl.panel / 8;
    dv.xa = x; dv.xb = x + pe; dv.ha = x + 2 * pe; dv.hb = x + 3 * pe;
    dv.status = status;
    return 0;
}

void launch_scales(const GwDev &d, hipStream_t s)
{
    (void)hipMemsetAsync(d.nlive, 0, 8, s);
    hipLaunchKernelGGL(gw_scale_kernel, dim3((d.n_rows + kWaves - 1) / kWaves), dim3(kThreads), 0, s, d);
}

// the two heat sums of the panel of source columns [col0, col0 + W), before the threshold
void launch_panel(GwDev d, const gcc_graphwave_args *h, int col0, hipStream_t s)
{
    d.col0 = col0;
    d.ncols = d.n_rows - col0 < d.W ? d.n_rows - col0 : d.W;
    const dim3 grid((d.ncols + 63) / 64, (d.n_rows + kWaves - 1) / kWaves);
    GwInit in;
    for (int i = 0; i < 2; ++i) in.c[i][0] = h->coeff[i][0], in.c[i][1] = h->coeff[i][1];
    hipLaunchKernelGGL(gw_init_kernel, grid, dim3(kThreads), 0, s, d, in);
    for (int k = 2; k <= kOrder; ++k) {
        d.ca = h->coeff[0][k];
        d.cb = h->coeff[1][k];
        hipLaunchKernelGGL(gw_step_kernel, grid, dim3(kThreads), 0, s, d);
        double *t = d.xa;                                           // X_k took X_{k-2}'s place: it is X_{k-1} of the next order
        d.xa = d.xb;
        d.xb = t;
    }
}

}  // namespace

extern "C" {

int64_t gcc_graphwave_panel_width(int64_t n_rows, int32_t d, int32_t width)
{
    const int rc = check_sizes("gcc_graphwave_panel_width", n_rows, 0, d, width);
    if (rc) return rc;
    return panel_width(n_rows, d, width);
}

int64_t gcc_graphwave_workspace_bytes(int64_t n_rows, int64_t nnz, int32_t d, int32_t width)
{
    const int rc = check_sizes("gcc_graphwave_workspace_bytes", n_rows, nnz, d, width);
    if (rc) return rc;
    return make_plan(n_rows, d, width).total;
}

int32_t gcc_graphwave_heat(const gcc_graphwave_args *h, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream)
{
    const char *who = "gcc_graphwave_heat";
    GwDev d;
    Plan pl;
    int rc = prepare(who, h, workspace, workspace_bytes, status, d, pl);
    if (rc) return rc;
    if ((rc = null_member(who, {{h->heat, "heat"}}))) return rc;
    if (h->heat_chunk < 0 || (int64_t)h->heat_chunk * pl.W >= h->n_rows) {
        snprintf(g_err, kErrLen, "%s: heat_chunk %d outside the %lld panels of %d columns", who, h->heat_chunk,
                 (long long)((h->n_rows + pl.W - 1) / pl.W), pl.W);
        return -5;
    }
    hipStream_t s = (hipStream_t)stream;
    (void)hipMemsetAsync(h->heat, 0, (size_t)2 * pl.panel, s);
    launch_scales(d, s);
    launch_panel(d, h, h->heat_chunk * pl.W, s);
    d.col0 = h->heat_chunk * pl.W;
    d.ncols = d.n_rows - d.col0 < d.W ? d.n_rows - d.col0 : d.W;
    hipLaunchKernelGGL(gw_heat_kernel, dim3(d.W / 64, (d.n_rows + kWaves - 1) / kWaves), dim3(kThreads), 0, s, d, h->threshold, h->heat);
    return launched();
}

int32_t gcc_graphwave_embed(const gcc_graphwave_args *h, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream)
{
    const char *who = "gcc_graphwave_embed";
    GwDev d;
    Plan pl;
    int rc = prepare(who, h, workspace, workspace_bytes, status, d, pl);
    if (rc) return rc;
    if ((rc = null_member(who, {{h->chi, "chi"}, {h->chi32, "chi32"}}))) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int64_t nd = h->n_rows * h->d;
    (void)hipMemsetAsync(h->chi, 0, (size_t)nd * 8, s);
    (void)hipMemsetAsync(h->chi32, 0, (size_t)nd * 4, s);
    launch_scales(d, s);
    GwChar ch;
    ch.T = h->d / 4;
    ch.d = h->d;
    ch.groups = (ch.T + kTg - 1) / kTg;
    ch.threshold = h->threshold;
    for (int j = 0; j < kMaxT; ++j) ch.t[j] = j < ch.T ? h->time_points[j] : 0.0;
    ch.part = ws_at<double>(workspace, pl.off_part);
    for (int col0 = 0; col0 < d.n_rows; col0 += pl.W) {
        launch_panel(d, h, col0, s);
        d.col0 = col0;
        d.ncols = d.n_rows - col0 < d.W ? d.n_rows - col0 : d.W;
        const int tiles = (d.ncols + 63) / 64;
        // (30 orders from (xa, xb) leave the sums where they were: ha / hb do not move)
        hipLaunchKernelGGL(gw_char_kernel, dim3(tiles, pl.blocks, 2 * ch.groups), dim3(kThreads), 0, s, d, ch);
        hipLaunchKernelGGL(gw_table_kernel, dim3(tiles, (h->d + kWaves - 1) / kWaves), dim3(kThreads), 0, s, d, (const double *)ch.part, (int)h->d,
                           (int)pl.blocks, h->chi, h->chi32);
    }
    return launched();
}

}  // extern "C"
