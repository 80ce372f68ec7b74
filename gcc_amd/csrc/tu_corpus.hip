// gcc_amd/csrc/tu_corpus.hip -- the integers of a TU dataset's three files -> the resident corpus of gcc_pack_graphs (gfx950): what
// gcc_amd.ingest.read_tudataset and DeviceGraphCorpus.__init__ build on the host.  Integers only: the outputs are a function of the
// SET of lines of A.txt, whatever their order and whatever the grid.
//
//   tu_flag_kernel          flag[i] = node i opens a graph (its indicator differs from the one before it); a descent sets DESCENDS.
//   (scan)                  tu_tile_sum / tu_tile_scan / tu_scan_apply, the scan of graph_rows.h: the flags -> every node's graph number, G.
//   tu_first_kernel         G != L sets GRAPH_COUNT; counts[0]; node_first (only when neither bit is set: it has L + 1 words).
//   tu_degree_kernel        (not behind DESCENDS / GRAPH_COUNT) an id outside [1, N] sets BAD_ID; deg[u]++ for every line that is in
//                           range, no self loop and inside one graph: integer atomics gathered on chip first (Gather, graph_rows.h).
//   (scan)                  deg -> row_ptr, the number of entries and the longest row.
//   tu_scatter_kernel       (not behind BAD_ID) SELF_LOOP and CROSS_GRAPH; col_idx[row_ptr[u] + cursor[u]++] = v - node_first[graph of u].
//   tu_sort_wave / tu_sort_lds / tu_sort_chunks / tu_merge / tu_unique_large   the row classes of graph_rows.h, in place in col_idx
//                           (a long row's merge passes go through the workspace; tu_back_kernel brings it home).  A row that loses an
//                           entry to the removal of repeats is what REPEATED means (tu_rows_kernel, on a clean word only).
//   tu_sym_kernel           (clean word only) a thread per entry: its row by a binary search in row_ptr, its reverse entry by one in
//                           the other row; ASYMMETRIC.
//   tu_graph_kernel         a wave per graph: seed_local (the first maximum of the degrees), edge_first, the largest graph.
//   tu_label_* kernels      the L raw labels are sorted as ONE row by the same row classes, repeats removed: the distinct values
//                           ascending; a label's class is its rank among them.
//   tu_finish_kernel        counts[1 .. 7].
// Every launch is sized from N, m and L alone; the host reads nothing.  Entry offsets fit int32 (m < 2^31); global thread indices are
// formed in 64 bits.
#include "graph_rows.h"

namespace {

enum { TW_MAX_NODES, TW_MAX_ENTRIES, TW_SPARE, TW_WORDS = 8 };
enum { LW_DEG, LW_START, LW_UCOUNT, LW_LIST_LDS, LW_LIST_LARGE, LW_SC = 8, LW_WORDS = LW_SC + SC_WORDS };
constexpr int kEarly = GCC_STATUS_TU_DESCENDS | GCC_STATUS_TU_GRAPH_COUNT;

struct TuDev {
    GbDev g;                                          // the rows: n = N, start = row_ptr, tmp = col_idx
    GbDev l;                                          // the labels as one row of L slots
    const int32_t *indicator, *raw_labels;
    int32_t N, L;
    long long m;
    int32_t *flag, *gx;                               // [N]: a graph's first node; the node's graph number
    int32_t *tw;
    int32_t *node_first, *edge_first, *seed_local, *labels;
    int64_t *counts;
    int32_t *status;
};

// the scans and the row-sort classes of graph_rows.h as this file's kernels
__global__ __launch_bounds__(kThreads) void tu_tile_sum_kernel(const int32_t *v, int n, int32_t *tsum_a, int32_t *tsum_b, int32_t *tmax)
{
    gb_tile_sum_body(v, n, tsum_a, tsum_b, tmax);
}
__global__ __launch_bounds__(kThreads) void tu_tile_scan_kernel(int32_t *tsum_a, int32_t *tsum_b, const int32_t *tmax, int tiles, int32_t *total,
                                                                int32_t *maxword)
{
    gb_tile_scan_body(tsum_a, tsum_b, tmax, tiles, total, maxword);
}
__global__ __launch_bounds__(kThreads) void tu_scan_apply_kernel(const int32_t *v, int n, const int32_t *tsum_a, const int32_t *tsum_b, int32_t *out)
{
    gb_scan_apply_body(v, n, tsum_a, tsum_b, out, nullptr, nullptr);
}
__global__ __launch_bounds__(kThreads) void tu_sort_wave_kernel(GbDev a) { gb_sort_wave_body(a); }
__global__ __launch_bounds__(kThreads) void tu_sort_lds_kernel(GbDev a) { gb_sort_lds_body(a); }
__global__ __launch_bounds__(kThreads) void tu_sort_chunks_kernel(GbDev a) { gb_sort_chunks_body(a); }
__global__ __launch_bounds__(kThreads) void tu_merge_kernel(GbDev a, int pass) { gb_merge_body(a, pass); }
__global__ __launch_bounds__(kThreads) void tu_unique_large_kernel(GbDev a) { gb_unique_large_body(a); }

__global__ __launch_bounds__(kThreads) void tu_flag_kernel(TuDev a)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    bool down = false;
    if (i < a.N) {
        const int cur = a.indicator[i], prev = i > 0 ? a.indicator[i - 1] : cur;
        a.flag[i] = i == 0 || cur != prev;
        down = cur < prev;
    }
    if (wave_ballot(down) && lane_id() == 0) atomicOr(a.status, (int32_t)GCC_STATUS_TU_DESCENDS);
}

__global__ __launch_bounds__(kThreads) void tu_first_kernel(TuDev a)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    const int G = a.g.sc[SC_RAW_TOTAL];
    // (the flags count the distinct values only where the indicator never descends; the bit this kernel sets is not read)
    const bool climbs = (load_fresh_i32(a.status) & GCC_STATUS_TU_DESCENDS) == 0, sound = climbs && G == a.L;
    if (i < a.N) {
        const int f = a.flag[i], gi = a.gx[i] + f - 1;
        a.gx[i] = gi;
        if (sound && f) a.node_first[gi] = (int)i;
    }
    if (i == 0) {
        a.counts[0] = G;
        if (climbs && G != a.L) atomicOr(a.status, (int32_t)GCC_STATUS_TU_GRAPH_COUNT);
        if (sound) a.node_first[a.L] = a.N;
    }
}

// a line of A.txt: zero-based ids, whether it becomes an entry, and what else it is
struct TuLine {
    int u, v;
    bool on, bad, loop, cross;
};
__device__ __forceinline__ TuLine tu_line(const TuDev &a, long long i)
{
    TuLine l = {-1, -1, false, false, false, false};
    if (i < a.m) {
        const unsigned u = (unsigned)a.g.pairs[2 * i] - 1u, v = (unsigned)a.g.pairs[2 * i + 1] - 1u;
        l.bad = u >= (unsigned)a.N || v >= (unsigned)a.N;
        if (!l.bad) {                                 // (nothing is read through an unchecked id)
            l.u = (int)u;
            l.v = (int)v;
            l.loop = u == v;
            l.cross = a.gx[u] != a.gx[v];
            l.on = !l.loop && !l.cross;
        }
    }
    return l;
}

__global__ __launch_bounds__(kThreads) void tu_degree_kernel(TuDev a)
{
    __shared__ Gather g;
    if ((load_fresh_i32(a.status) & kEarly) != 0) return;          // (bits this kernel never sets: the whole grid agrees)
    gather_clear(g);
    bool bad = false;
#pragma unroll
    for (int j = 0; j < kLinesPer; ++j) {
        const TuLine l = tu_line(a, (long long)blockIdx.x * kLinesPerGroup + j * kThreads + threadIdx.x);
        bad = bad || l.bad;
        gather_add(g, a.g.deg, l.on, l.u);
    }
    if (wave_ballot(bad) && lane_id() == 0) atomicOr(a.status, (int32_t)GCC_STATUS_TU_BAD_ID);
    gather_flush(g, a.g.deg);
}

__global__ __launch_bounds__(kThreads) void tu_scatter_kernel(TuDev a)
{
    __shared__ Gather g;
    if ((load_fresh_i32(a.status) & (kEarly | GCC_STATUS_TU_BAD_ID)) != 0) return;
    gather_clear(g);
    TuLine l[kLinesPer];
    Place pu[kLinesPer];
    int bits = 0;
#pragma unroll
    for (int j = 0; j < kLinesPer; ++j) {
        l[j] = tu_line(a, (long long)blockIdx.x * kLinesPerGroup + j * kThreads + threadIdx.x);
        bits |= (l[j].loop ? GCC_STATUS_TU_SELF_LOOP : 0) | (l[j].cross ? GCC_STATUS_TU_CROSS_GRAPH : 0);
        pu[j] = gather_add(g, a.g.cursor, l[j].on, l[j].u);
    }
    if (bits) atomicOr(a.status, (int32_t)bits);
    gather_flush(g, a.g.cursor);
#pragma unroll
    for (int j = 0; j < kLinesPer; ++j) {
        if (!l[j].on) continue;                       // (a place is below deg[u]: the same lines counted the degree)
        a.g.tmp[a.g.start[l[j].u] + (pu[j].slot >= 0 ? g.base[pu[j].slot] : 0) + pu[j].rank] = l[j].v - a.node_first[a.gx[l[j].u]];
    }
}

// a long row whose last merge pass ended in the workspace comes home to col_idx
__global__ __launch_bounds__(kThreads) void tu_back_kernel(TuDev a)
{
    const int rows = min(a.g.sc[SC_N_LARGE], a.g.cap_large);
    for (int r = (int)blockIdx.x; r < rows; r += (int)gridDim.x) {
        const int i = a.g.list_large[r], d = a.g.deg[i], uc = a.g.ucount[i], b = a.g.start[i];
        if ((merge_passes(d) & 1) == 0) continue;
        for (int t = (int)threadIdx.x; t < uc; t += kThreads) a.g.tmp[b + t] = a.g.tmp2[b + t];
    }
}

// row_ptr's last word; a row that lost an entry when the repeats were removed
__global__ __launch_bounds__(kThreads) void tu_rows_kernel(TuDev a)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i == 0) a.g.start[a.N] = a.g.sc[SC_UNIQ_TOTAL];
    if (a.m == 0 || (load_fresh_i32(a.status) & ~GCC_STATUS_TU_REPEATED) != 0) return;       // (this kernel's own bit does not gate it)
    const bool twice = i < a.N && a.g.ucount[i] != a.g.deg[i];
    if (wave_ballot(twice) && lane_id() == 0) atomicOr(a.status, (int32_t)GCC_STATUS_TU_REPEATED);
}

// Runs only on a status word without any other bit: every line is an entry then, every row is sorted and names nodes of its own graph.
__global__ __launch_bounds__(kThreads) void tu_sym_kernel(TuDev a)
{
    if ((load_fresh_i32(a.status) & ~GCC_STATUS_TU_ASYMMETRIC) != 0) return;
    const long long q = (long long)blockIdx.x * kThreads + threadIdx.x;
    bool lone = false;
    if (q < a.m) {
        const int32_t *rp = a.g.start, *ci = a.g.tmp;
        const int i = bound_of<true>(rp, 0, a.N + 1, (int)q) - 1;  // the last row that begins at or below q: rows without entries are skipped
        const int first = a.node_first[a.gx[i]], j = first + ci[q], li = i - first;
        const int lo = bound_of<false>(ci, rp[j], rp[j + 1], li);
        lone = !(lo < rp[j + 1] && ci[lo] == li);
    }
    if (wave_ballot(lone) && lane_id() == 0) atomicOr(a.status, (int32_t)GCC_STATUS_TU_ASYMMETRIC);
}

// a wave per graph
__global__ __launch_bounds__(kThreads) void tu_graph_kernel(TuDev a)
{
    if ((load_fresh_i32(a.status) & kEarly) != 0) return;
    const int lane = lane_id();
    const long long waves = (long long)gridDim.x * kWaves;
    int most_nodes = 0, most_entries = 0;
    for (long long g64 = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6); g64 < a.L; g64 += waves) {
        const int g = wave_uniform((int)g64);
        const int n0 = wave_uniform(a.node_first[g]), n1 = wave_uniform(a.node_first[g + 1]);
        int best = -1, at = INT32_MAX;                // the largest degree and the lowest node that has it
        for (int i = n0 + lane; i < n1; i += 64) {
            const int d = a.g.deg[i];
            if (d > best) {
                best = d;
                at = i;
            }
        }
        for (int s = 32; s >= 1; s >>= 1) {
            const int ob = wave_shfl_xor(best, s), oa = wave_shfl_xor(at, s);
            if (ob > best || (ob == best && oa < at)) {
                best = ob;
                at = oa;
            }
        }
        const int e0 = a.g.start[n0], e1 = a.g.start[n1];
        if (lane == 0) {
            a.seed_local[g] = at - n0;
            a.edge_first[g] = e0;
            if (g == a.L - 1) a.edge_first[a.L] = e1;
        }
        most_nodes = n1 - n0 > most_nodes ? n1 - n0 : most_nodes;
        most_entries = e1 - e0 > most_entries ? e1 - e0 : most_entries;
    }
    if (lane == 0) {
        if (most_nodes > 0) atomicMax(&a.tw[TW_MAX_NODES], (int32_t)most_nodes);
        if (most_entries > 0) atomicMax(&a.tw[TW_MAX_ENTRIES], (int32_t)most_entries);
    }
}

__global__ __launch_bounds__(kThreads) void tu_label_init_kernel(TuDev a)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i < a.L) a.l.tmp[i] = a.raw_labels[i];
    if (i == 0) {
        a.l.deg[0] = a.L;                             // (start[0] is 0 from the memset)
        a.l.sc[SC_MAX_SLOTS] = a.L;
    }
}

// where the distinct values stand after the sort
__device__ __forceinline__ const int32_t *label_values(const TuDev &a) { return a.L > kLdsRow ? large_row(a.l, 0, a.L) : a.l.tmp; }

__global__ __launch_bounds__(kThreads) void tu_label_rank_kernel(TuDev a)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i < a.L) a.labels[i] = bound_of<false>(label_values(a), 0, a.l.ucount[0], a.raw_labels[i]);
}

__global__ void tu_finish_kernel(TuDev a)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    a.counts[1] = a.l.ucount[0];
    a.counts[2] = a.tw[TW_MAX_NODES];
    a.counts[3] = a.tw[TW_MAX_ENTRIES];
    a.counts[4] = a.g.sc[SC_MAX_SLOTS];
    a.counts[5] = a.counts[6] = a.counts[7] = 0;
}

// ---------------------------------------------------------------- host
struct Plan {
    int64_t off_deg, off_cursor, off_sc, off_tw, off_lw, zero_bytes;   // [off_deg, off_deg + zero_bytes): what a call zeroes first
    int64_t off_flag, off_gx, off_ucount, off_tsum_a, off_tsum_b, off_tmax, off_list_lds, off_list_large, off_tmp2, off_ltmp, off_ltmp2, total;
    int32_t tiles, cap_lds, cap_large, passes, label_passes;
};

int check_sizes(const char *who, int64_t n, int64_t m, int64_t l)
{
    if (n < 1 || n >= INT32_MAX) {
        snprintf(g_err, kErrLen, "%s: num_nodes %lld outside 1..2^31 - 2: node ids are int32 and row_ptr has one word more", who, (long long)n);
        return -2;
    }
    if (m < 0 || m > INT32_MAX) {
        snprintf(g_err, kErrLen, "%s: num_lines %lld outside 0..2^31 - 1: entry offsets are int32", who, (long long)m);
        return -2;
    }
    if (l < 1 || l >= INT32_MAX) {
        snprintf(g_err, kErrLen, "%s: num_labels %lld outside 1..2^31 - 2", who, (long long)l);
        return -2;
    }
    return 0;
}

int passes_of(int64_t slots)
{
    int p = 0;
    while (((int64_t)kLdsRow << p) < slots) ++p;
    return p;
}

Plan make_plan(int64_t n, int64_t m, int64_t l)
{
    Plan p;
    p.tiles = (int32_t)((n + kTile - 1) / kTile);
    // a row pushed to a list holds more than kWaveRow (kLdsRow) of the m slots
    p.cap_lds = (int32_t)(m / (kWaveRow + 1));
    p.cap_large = (int32_t)(m / (kLdsRow + 1));
    p.passes = passes_of(m);
    p.label_passes = passes_of(l);
    Carve cv;
    p.off_deg = cv.take(n * 4);
    p.off_cursor = cv.take(n * 4);
    p.off_sc = cv.take(SC_WORDS * 4);
    p.off_tw = cv.take(TW_WORDS * 4);
    p.off_lw = cv.take(LW_WORDS * 4);
    p.zero_bytes = cv.total() - p.off_deg;
    p.off_flag = cv.take(n * 4);
    p.off_gx = cv.take(n * 4);
    p.off_ucount = cv.take(n * 4);
    p.off_tsum_a = cv.take((int64_t)p.tiles * 4);
    p.off_tsum_b = cv.take((int64_t)p.tiles * 4);
    p.off_tmax = cv.take((int64_t)p.tiles * 4);
    p.off_list_lds = cv.take((int64_t)p.cap_lds * 4);
    p.off_list_large = cv.take((int64_t)p.cap_large * 4);
    p.off_tmp2 = cv.take(p.cap_large ? m * 4 : 0);
    p.off_ltmp = cv.take(l * 4);
    p.off_ltmp2 = cv.take(l > kLdsRow ? l * 4 : 0);
    p.total = cv.total();
    return p;
}

int grid_of(int64_t items, int per) { return (int)((items + per - 1) / per); }
int capped(int64_t g) { return (int)(g < 1 ? 1 : g > kListGrid ? kListGrid : g); }

// exclusive scan of v[0, N) -> out; the total -> total[0] (total[1]: the number of v > 0), the largest value -> *maxword
void launch_scan(const TuDev &d, const Plan &pl, const int32_t *v, int32_t *out, int32_t *total, int32_t *maxword, hipStream_t s)
{
    hipLaunchKernelGGL(tu_tile_sum_kernel, dim3(pl.tiles), dim3(kThreads), 0, s, v, d.N, d.g.tsum_a, d.g.tsum_b, d.g.tmax);
    hipLaunchKernelGGL(tu_tile_scan_kernel, dim3(1), dim3(kThreads), 0, s, d.g.tsum_a, d.g.tsum_b, (const int32_t *)d.g.tmax, (int)pl.tiles, total, maxword);
    hipLaunchKernelGGL(tu_scan_apply_kernel, dim3(pl.tiles), dim3(kThreads), 0, s, v, d.N, (const int32_t *)d.g.tsum_a, (const int32_t *)d.g.tsum_b, out);
}

// the row classes over the rows of `r`: `slots` entries in all, `passes` merge passes for its longest possible row
void launch_sorts(const GbDev &r, int64_t slots, int passes, hipStream_t s)
{
    const dim3 block(kThreads);
    hipLaunchKernelGGL(tu_sort_wave_kernel, dim3(grid_of(r.n, kWaves)), block, 0, s, r);
    if (r.cap_lds > 0) hipLaunchKernelGGL(tu_sort_lds_kernel, dim3(capped(r.cap_lds)), block, 0, s, r);
    if (r.cap_large > 0) {
        const int wide = capped(grid_of(slots, kLdsRow));
        hipLaunchKernelGGL(tu_sort_chunks_kernel, dim3(wide), block, 0, s, r);
        for (int pass = 0; pass < passes; ++pass) hipLaunchKernelGGL(tu_merge_kernel, dim3(wide), block, 0, s, r, pass);
        hipLaunchKernelGGL(tu_unique_large_kernel, dim3(capped(r.cap_large)), block, 0, s, r);
    }
}

}  // namespace

extern "C" {

int64_t gcc_tu_corpus_workspace_bytes(int64_t num_nodes, int64_t num_lines, int64_t num_labels)
{
    const int rc = check_sizes("gcc_tu_corpus_workspace_bytes", num_nodes, num_lines, num_labels);
    if (rc) return rc;
    return make_plan(num_nodes, num_lines, num_labels).total;
}

int32_t gcc_tu_corpus(const gcc_tu_corpus_args *h, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream)
{
    const char *who = "gcc_tu_corpus";
    int rc = null_member(who, {{h, "args"}});
    if (rc) return rc;
    const int64_t N = h->num_nodes, m = h->num_lines, L = h->num_labels;
    if ((rc = check_sizes(who, N, m, L))) return rc;
    if ((rc = null_member(who, {{status, "status"}, {h->pairs, "pairs", m > 0}, {h->indicator, "indicator"}, {h->graph_labels, "graph_labels"},
                                {h->node_first, "node_first"}, {h->edge_first, "edge_first"}, {h->row_ptr, "row_ptr"},
                                {h->col_idx, "col_idx", m > 0}, {h->seed_local, "seed_local"}, {h->labels, "labels"}, {h->counts, "counts"}})))
        return rc;
    const Plan pl = make_plan(N, m, L);
    if ((rc = check_workspace(who, "gcc_tu_corpus_workspace_bytes", workspace, workspace_bytes, pl.total))) return rc;
    TuDev d = TuDev();
    d.indicator = h->indicator; d.raw_labels = h->graph_labels;
    d.N = (int32_t)N; d.L = (int32_t)L; d.m = m;
    d.flag = ws_at<int32_t>(workspace, pl.off_flag); d.gx = ws_at<int32_t>(workspace, pl.off_gx); d.tw = ws_at<int32_t>(workspace, pl.off_tw);
    d.node_first = h->node_first; d.edge_first = h->edge_first; d.seed_local = h->seed_local; d.labels = h->labels;
    d.counts = h->counts; d.status = status;
    GbDev &g = d.g;
    g.pairs = h->pairs; g.n = (int32_t)N; g.m = (int32_t)m;
    g.deg = ws_at<int32_t>(workspace, pl.off_deg); g.cursor = ws_at<int32_t>(workspace, pl.off_cursor); g.sc = ws_at<int32_t>(workspace, pl.off_sc);
    g.start = h->row_ptr; g.ucount = ws_at<int32_t>(workspace, pl.off_ucount);
    g.tsum_a = ws_at<int32_t>(workspace, pl.off_tsum_a); g.tsum_b = ws_at<int32_t>(workspace, pl.off_tsum_b); g.tmax = ws_at<int32_t>(workspace, pl.off_tmax);
    g.list_lds = ws_at<int32_t>(workspace, pl.off_list_lds); g.list_large = ws_at<int32_t>(workspace, pl.off_list_large);
    g.tmp = h->col_idx; g.tmp2 = ws_at<int32_t>(workspace, pl.off_tmp2);
    g.cap_lds = pl.cap_lds; g.cap_large = pl.cap_large;
    g.status = status;
    GbDev &l = d.l;
    int32_t *lw = ws_at<int32_t>(workspace, pl.off_lw);
    l.n = 1; l.m = (int32_t)L;
    l.deg = lw + LW_DEG; l.start = lw + LW_START; l.ucount = lw + LW_UCOUNT; l.list_lds = lw + LW_LIST_LDS; l.list_large = lw + LW_LIST_LARGE;
    l.sc = lw + LW_SC;
    l.tmp = ws_at<int32_t>(workspace, pl.off_ltmp); l.tmp2 = ws_at<int32_t>(workspace, pl.off_ltmp2);
    l.cap_lds = L > kWaveRow; l.cap_large = L > kLdsRow;
    l.status = status;
    hipStream_t s = (hipStream_t)stream;
    const dim3 block(kThreads);
    const int node_grid = grid_of(N, kThreads), line_grid = grid_of(m, kLinesPerGroup), label_grid = grid_of(L, kThreads);
    (void)hipMemsetAsync(g.deg, 0, (size_t)pl.zero_bytes, s);
    hipLaunchKernelGGL(tu_flag_kernel, dim3(node_grid), block, 0, s, d);
    launch_scan(d, pl, d.flag, d.gx, g.sc + SC_RAW_TOTAL, d.tw + TW_SPARE, s);
    hipLaunchKernelGGL(tu_first_kernel, dim3(node_grid), block, 0, s, d);
    if (m > 0) hipLaunchKernelGGL(tu_degree_kernel, dim3(line_grid), block, 0, s, d);
    launch_scan(d, pl, g.deg, g.start, g.sc + SC_UNIQ_TOTAL, g.sc + SC_MAX_SLOTS, s);
    if (m > 0) {
        hipLaunchKernelGGL(tu_scatter_kernel, dim3(line_grid), block, 0, s, d);
        launch_sorts(g, m, pl.passes, s);
        if (pl.cap_large > 0) hipLaunchKernelGGL(tu_back_kernel, dim3(capped(pl.cap_large)), block, 0, s, d);
    }
    hipLaunchKernelGGL(tu_rows_kernel, dim3(node_grid), block, 0, s, d);
    if (m > 0) hipLaunchKernelGGL(tu_sym_kernel, dim3(grid_of(m, kThreads)), block, 0, s, d);
    hipLaunchKernelGGL(tu_graph_kernel, dim3(capped(grid_of(L, kWaves))), block, 0, s, d);
    hipLaunchKernelGGL(tu_label_init_kernel, dim3(label_grid), block, 0, s, d);
    launch_sorts(l, L, pl.label_passes, s);
    hipLaunchKernelGGL(tu_label_rank_kernel, dim3(label_grid), block, 0, s, d);
    hipLaunchKernelGGL(tu_finish_kernel, dim3(1), dim3(64), 0, s, d);
    return launched();
}

}  // extern "C"
