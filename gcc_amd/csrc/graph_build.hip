// gcc_amd/csrc/graph_build.hip -- raw undirected edge lines -> the contract CSR of the sampler, and the device form of the contract
// check (gfx950).  The rule is the reference converter's (gcc/utils/x2dgl.py, yuxiao_kdd17_graph_to_dgl): drop the lines u == v, insert
// both directions of the rest, keep one entry per non-zero, remove the nodes left without an entry, relabel the survivors in ascending
// old-id order, rows sorted ascending.  Integers only: the output is a function of the SET of lines, whatever their order.
//
//   gb_degree_kernel        ids outside [0, n) set GCC_STATUS_GRAPH_BUILD_BAD_ID and drop the line, u == v is counted and dropped,
//                           deg[u]++ / deg[v]++: integer atomics, gathered per run of equal ids in adjacent lanes and per id in
//                           the workgroup's 1,024 lines first (Gather: a hub's lines would otherwise all queue on one word).
//   gb_tile_sum / gb_tile_scan / gb_scan_apply   exclusive scan of (deg, deg > 0) in tiles of GCC_GRAPH_BUILD_SCAN_TILE: the rows' first
//                           slots in `tmp` and the new ids (node_map).  The same three kernels scan the rows' final lengths later.
//   gb_scatter_kernel       tmp[start[u] + cursor[u]++] = v and the reverse (returning atomics, gathered the same way); the arrival
//                           order in a row is arbitrary: the row is sorted next.
//   gb_sort_wave_kernel     a wave per row of up to GCC_GRAPH_BUILD_WAVE_ROW entries: bitonic network over the lanes, unique by a
//                           ballot, written back in place.  Longer rows are pushed to one of two lists (their order is arbitrary and
//                           immaterial: a row's result depends on the row alone).
//   gb_sort_lds_kernel      a workgroup per listed row of up to GCC_GRAPH_BUILD_LDS_ROW entries: bitonic sort in LDS, unique by a
//                           workgroup scan, written back in place.
//   gb_sort_chunks_kernel   longer rows: chunks of GCC_GRAPH_BUILD_LDS_ROW sorted in LDS, then
//   gb_merge_kernel         one launch per doubling of the run width: every element finds its place by a binary search in the sibling
//                           run (tmp <-> tmp2), and
//   gb_unique_large_kernel  a workgroup per long row removes the repeats in place.
//   gb_compact_kernel / gb_compact_large_kernel   col_idx[row_ptr[new(u)] + q] = new(entry q of row u).
//   gb_finish_kernel        row_ptr's last word and counts[6].
// Every launch is sized from n and m alone; the kernels read the live counts (list lengths, row lengths) on the device.  The host
// reads nothing.  Offsets: 2 m < 2^31 is required, so every slot index fits int32; global thread indices are formed in 64 bits.
//
//   gc_rows_kernel / gc_entries_kernel / gc_sym_kernel   gcc_graph_check: row_ptr, then every entry in its row (tiles of entries, so a
//                           hub row is no one's burden), then -- only when those found nothing: a binary search needs sorted rows
//                           in range -- the reverse entry of every entry.
#include "graph_rows.h"

namespace {

// the scans and the row-sort classes: their bodies live in graph_rows.h, which tu_corpus.hip shares
__global__ __launch_bounds__(kThreads) void gb_tile_sum_kernel(const int32_t *v, int n, int32_t *tsum_a, int32_t *tsum_b, int32_t *tmax)
{
    gb_tile_sum_body(v, n, tsum_a, tsum_b, tmax);
}
__global__ __launch_bounds__(kThreads) void gb_tile_scan_kernel(int32_t *tsum_a, int32_t *tsum_b, const int32_t *tmax, int tiles, int32_t *total,
                                                                int32_t *maxword)
{
    gb_tile_scan_body(tsum_a, tsum_b, tmax, tiles, total, maxword);
}
__global__ __launch_bounds__(kThreads) void gb_scan_apply_kernel(const int32_t *v, int n, const int32_t *tsum_a, const int32_t *tsum_b,
                                                                 int32_t *out_a, int32_t *out_b, int32_t *node_map)
{
    gb_scan_apply_body(v, n, tsum_a, tsum_b, out_a, out_b, node_map);
}
__global__ __launch_bounds__(kThreads) void gb_sort_wave_kernel(GbDev a) { gb_sort_wave_body(a); }
__global__ __launch_bounds__(kThreads) void gb_sort_lds_kernel(GbDev a) { gb_sort_lds_body(a); }
__global__ __launch_bounds__(kThreads) void gb_sort_chunks_kernel(GbDev a) { gb_sort_chunks_body(a); }
__global__ __launch_bounds__(kThreads) void gb_merge_kernel(GbDev a, int pass) { gb_merge_body(a, pass); }
__global__ __launch_bounds__(kThreads) void gb_unique_large_kernel(GbDev a) { gb_unique_large_body(a); }

// a line: its two ids, whether it is inserted, and what else it is
struct Line {
    int u, v;
    bool on, bad, loop;
};
__device__ __forceinline__ Line read_line(const GbDev &a, long long i)
{
    Line l = {-1, -1, false, false, false};
    if (i < a.m) {
        l.u = a.pairs[2 * i];
        l.v = a.pairs[2 * i + 1];
        l.bad = (unsigned)l.u >= (unsigned)a.n || (unsigned)l.v >= (unsigned)a.n;
        l.loop = !l.bad && l.u == l.v;
        l.on = !l.bad && !l.loop;
    }
    return l;
}

__global__ __launch_bounds__(kThreads) void gb_degree_kernel(GbDev a)
{
    __shared__ Gather g;
    gather_clear(g);
    int bad = 0, loops = 0;
#pragma unroll
    for (int j = 0; j < kLinesPer; ++j) {
        const Line l = read_line(a, (long long)blockIdx.x * kLinesPerGroup + j * kThreads + threadIdx.x);
        bad |= l.bad;
        loops += l.loop;
        gather_add(g, a.deg, l.on, l.u);
        gather_add(g, a.deg, l.on, l.v);
    }
    const unsigned long long any_bad = wave_ballot(bad != 0);
    loops = wave_scan_incl(loops);
    if (lane_id() == 63) {
        if (any_bad) atomicOr(a.status, (int32_t)GCC_STATUS_GRAPH_BUILD_BAD_ID);
        if (loops) atomicAdd(&a.sc[SC_SELF_LOOPS], (int32_t)loops);
    }
    gather_flush(g, a.deg);
}

__global__ __launch_bounds__(kThreads) void gb_scatter_kernel(GbDev a)
{
    __shared__ Gather g;
    gather_clear(g);
    Line l[kLinesPer];
    Place pu[kLinesPer], pv[kLinesPer];
#pragma unroll
    for (int j = 0; j < kLinesPer; ++j) {
        l[j] = read_line(a, (long long)blockIdx.x * kLinesPerGroup + j * kThreads + threadIdx.x);
        pu[j] = gather_add(g, a.cursor, l[j].on, l[j].u);
        pv[j] = gather_add(g, a.cursor, l[j].on, l[j].v);
    }
    gather_flush(g, a.cursor);
#pragma unroll
    for (int j = 0; j < kLinesPer; ++j) {
        if (!l[j].on) continue;                       // (a place is below deg[id]: the same lines counted the degree)
        a.tmp[a.start[l[j].u] + (pu[j].slot >= 0 ? g.base[pu[j].slot] : 0) + pu[j].rank] = l[j].v;
        a.tmp[a.start[l[j].v] + (pv[j].slot >= 0 ? g.base[pv[j].slot] : 0) + pv[j].rank] = l[j].u;
    }
}

__global__ __launch_bounds__(kThreads) void gb_compact_kernel(GbDev a)
{
    const int lane = lane_id();
    const long long i64 = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (i64 >= a.n) return;                                         // (the whole wave)
    const int i = wave_uniform((int)i64);
    const int d = wave_uniform(a.deg[i]);
    if (d == 0) return;
    const int ob = a.ustart[i];
    if (lane == 0) a.row_ptr[a.newid[i]] = ob;
    if (d > kLdsRow) return;                                        // (gb_compact_large_kernel moves its entries)
    const int uc = a.ucount[i], b = a.start[i];
    for (int q = lane; q < uc; q += 64) a.col_idx[ob + q] = a.newid[a.tmp[b + q]];
}

__global__ __launch_bounds__(kThreads) void gb_compact_large_kernel(GbDev a)
{
    const int rows = min(a.sc[SC_N_LARGE], a.cap_large);
    int before = 0;
    for (int r = 0; r < rows; ++r) {
        const int i = a.list_large[r], d = a.deg[i], uc = a.ucount[i], ob = a.ustart[i];
        const int32_t *buf = large_row(a, i, d);
        const int tiles = (uc + kThreads - 1) / kThreads, t_first = rotated(before);
        before = (before + tiles) % (int)gridDim.x;
        for (long long e = (long long)t_first * kThreads + threadIdx.x; e < uc; e += (long long)gridDim.x * kThreads)
            a.col_idx[ob + e] = a.newid[buf[e]];
    }
}

__global__ void gb_finish_kernel(GbDev a)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int kept = a.sc[SC_KEPT], entries = a.sc[SC_UNIQ_TOTAL];
    a.row_ptr[kept] = entries;
    a.counts[0] = kept;
    a.counts[1] = entries;
    a.counts[2] = a.sc[SC_SELF_LOOPS];
    a.counts[3] = (int64_t)a.sc[SC_RAW_TOTAL] - entries;
    a.counts[4] = (int64_t)a.n - kept;
    a.counts[5] = a.sc[SC_MAX_DEGREE];
}

// ---------------------------------------------------------------- the contract check
struct GcDev {
    const int32_t *rp, *ci;
    int32_t n, nnz, multigraph;
    int32_t *maxima, *status;
};

// a thread per row: row_ptr alone (its two ends, every row's extent and length)
__global__ __launch_bounds__(kThreads) void gc_rows_kernel(GcDev a)
{
    const long long threads = (long long)gridDim.x * kThreads;
    int bits = 0, maxdeg = 0;
    for (long long i64 = (long long)blockIdx.x * kThreads + threadIdx.x; i64 < a.n; i64 += threads) {
        const int i = (int)i64;
        if ((i == 0 && a.rp[0] != 0) || (i == a.n - 1 && a.rp[a.n] != a.nnz)) bits |= GCC_STATUS_GRAPH_CHECK_SPAN;
        const int b = a.rp[i], e = a.rp[i + 1];
        if (e <= b) bits |= GCC_STATUS_GRAPH_CHECK_ZERO_DEGREE;
        if (b < 0 || e > a.nnz) bits |= GCC_STATUS_GRAPH_CHECK_SPAN;
        else maxdeg = e - b > maxdeg ? e - b : maxdeg;
    }
    if (bits) atomicOr(a.status, (int32_t)bits);
    maxdeg = wave_max_i32(maxdeg);
    if (lane_id() == 0 && maxdeg > 0) atomicMax(&a.maxima[0], (int32_t)maxdeg);
}

// The two entry kernels work on tiles of kEntryTile ENTRIES, not on rows: a hub's row of 10^5 entries is spread over a hundred
// workgroups like any other stretch of col_idx.  They run only where gc_rows_kernel found row_ptr to climb strictly from 0 to nnz,
// so the row of entry q is the last i with rp[i] <= q: a binary search, over the rows of the whole graph for the tile's two ends
// (the same addresses in every lane) and over the tile's own rows (at most kEntryTile of them) for each entry.
constexpr int kEntryTile = 1024, kEntryGrid = 16384;
constexpr int kRowBits = GCC_STATUS_GRAPH_CHECK_SPAN | GCC_STATUS_GRAPH_CHECK_ZERO_DEGREE;

__device__ __forceinline__ int row_of(const int32_t *rp, int lo, int hi, int q)       // rows [lo, hi]
{
    return bound_of<true>(rp, lo, hi + 1, q) - 1;
}

struct EntryTile {
    int q0, q1, r0, r1;                               // entries [q0, q1), their rows within [r0, r1]
};
__device__ __forceinline__ EntryTile entry_tile(const GcDev &a, long long t)
{
    EntryTile e;
    e.q0 = (int)(t * kEntryTile);
    e.q1 = t * kEntryTile + kEntryTile < a.nnz ? (int)(t * kEntryTile + kEntryTile) : a.nnz;
    e.r0 = row_of(a.rp, 0, a.n - 1, e.q0);
    e.r1 = row_of(a.rp, e.r0, a.n - 1, e.q1 - 1);
    return e;
}

__global__ __launch_bounds__(kThreads) void gc_entries_kernel(GcDev a)
{
    if ((load_fresh_i32(a.status) & kRowBits) != 0) return;         // (bits this kernel never sets)
    int bits = 0;
    const long long tiles = ((long long)a.nnz + kEntryTile - 1) / kEntryTile;
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const EntryTile tl = entry_tile(a, t);
        for (int q = tl.q0 + (int)threadIdx.x; q < tl.q1; q += kThreads) {
            const int i = row_of(a.rp, tl.r0, tl.r1, q), b = a.rp[i], j = a.ci[q];
            if ((unsigned)j >= (unsigned)a.n) {
                bits |= GCC_STATUS_GRAPH_CHECK_RANGE;
                continue;
            }
            if (j == i) bits |= GCC_STATUS_GRAPH_CHECK_SELF_LOOP;
            if (q > b) {
                const int before = a.ci[q - 1];
                if (before > j) bits |= GCC_STATUS_GRAPH_CHECK_UNSORTED;
                if (before == j && !a.multigraph) bits |= GCC_STATUS_GRAPH_CHECK_DUPLICATE;
            }
        }
    }
    if (bits) atomicOr(a.status, (int32_t)bits);
}

// Runs only on a status word without any other bit: every row is then sorted and in range, so the reverse entry is found by a
// binary search.  Simple graphs: r must stand in row c.  Multigraphs: c in row r as often as r in row c.
__global__ __launch_bounds__(kThreads) void gc_sym_kernel(GcDev a)
{
    if ((load_fresh_i32(a.status) & ~GCC_STATUS_GRAPH_CHECK_ASYMMETRIC) != 0) return;       // (this kernel's own bit does not gate it)
    int bits = 0, copies = 0;
    const long long tiles = ((long long)a.nnz + kEntryTile - 1) / kEntryTile;
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const EntryTile tl = entry_tile(a, t);
        for (int q = tl.q0 + (int)threadIdx.x; q < tl.q1; q += kThreads) {
            const int i = row_of(a.rp, tl.r0, tl.r1, q), b = a.rp[i], e = a.rp[i + 1], c = a.ci[q];
            if (q > b && a.ci[q - 1] == c) continue;                // (a multigraph's copies: the first one speaks for them)
            const int here = a.multigraph ? bound_of<true>(a.ci, q, e, c) - q : 1;
            const int cb = a.rp[c], ce = a.rp[c + 1];
            const int lo = bound_of<false>(a.ci, cb, ce, i);
            const int there = a.multigraph ? bound_of<true>(a.ci, lo, ce, i) - lo : (lo < ce && a.ci[lo] == i);
            if (here != there) bits |= GCC_STATUS_GRAPH_CHECK_ASYMMETRIC;
            copies = here > copies ? here : copies;
        }
    }
    if (bits) atomicOr(a.status, (int32_t)bits);
    copies = wave_max_i32(copies);
    if (lane_id() == 0 && copies > 0) atomicMax(&a.maxima[1], (int32_t)copies);
}

// ---------------------------------------------------------------- host
struct Plan {
    int64_t off_deg, off_cursor, off_sc, zero_bytes;  // [off_deg, off_deg + zero_bytes): what a call zeroes first
    int64_t off_start, off_newid, off_ucount, off_ustart, off_tsum_a, off_tsum_b, off_tmax, off_list_lds, off_list_large, off_tmp, off_tmp2, total;
    int32_t tiles, cap_lds, cap_large, passes;
};

int check_sizes(const char *who, int64_t n, int64_t m)
{
    if (n < 1 || n > INT32_MAX) {
        snprintf(g_err, kErrLen, "%s: n %lld outside 1..2^31 - 1: node ids are int32", who, (long long)n);
        return -2;
    }
    if (m < 0 || 2 * m > INT32_MAX) {
        snprintf(g_err, kErrLen, "%s: m %lld: 2 m must stay below 2^31, entry offsets are int32", who, (long long)m);
        return -2;
    }
    return 0;
}

Plan make_plan(int64_t n, int64_t m)
{
    Plan p;
    p.tiles = (int32_t)((n + kTile - 1) / kTile);
    // a row pushed to a list holds more than kWaveRow (kLdsRow) of the 2 m slots
    p.cap_lds = (int32_t)(2 * m / (kWaveRow + 1));
    p.cap_large = (int32_t)(2 * m / (kLdsRow + 1));
    p.passes = 0;
    while (((int64_t)kLdsRow << p.passes) < m) ++p.passes;          // (a row holds at most m slots: a line gives each end one)
    Carve cv;
    p.off_deg = cv.take(n * 4);
    p.off_cursor = cv.take(n * 4);
    p.off_sc = cv.take(SC_WORDS * 4);
    p.zero_bytes = cv.total() - p.off_deg;
    p.off_start = cv.take(n * 4);
    p.off_newid = cv.take(n * 4);
    p.off_ucount = cv.take(n * 4);
    p.off_ustart = cv.take(n * 4);
    p.off_tsum_a = cv.take((int64_t)p.tiles * 4);
    p.off_tsum_b = cv.take((int64_t)p.tiles * 4);
    p.off_tmax = cv.take((int64_t)p.tiles * 4);
    p.off_list_lds = cv.take((int64_t)p.cap_lds * 4);
    p.off_list_large = cv.take((int64_t)p.cap_large * 4);
    p.off_tmp = cv.take(2 * m * 4);
    p.off_tmp2 = cv.take(p.cap_large ? 2 * m * 4 : 0);
    p.total = cv.total();
    return p;
}

int grid_of(int64_t items, int per) { return (int)((items + per - 1) / per); }
int capped(int64_t g) { return (int)(g < 1 ? 1 : g > kListGrid ? kListGrid : g); }

// exclusive scan of (v, v > 0) over n words -> out_a, out_b (may be NULL), node_map (may be NULL); the totals -> total[0 .. 1]
void launch_scan(const GbDev &d, const Plan &pl, const int32_t *v, int32_t *out_a, int32_t *out_b, int32_t *node_map, int32_t *total,
                 int32_t *maxword, hipStream_t s)
{
    hipLaunchKernelGGL(gb_tile_sum_kernel, dim3(pl.tiles), dim3(kThreads), 0, s, v, d.n, d.tsum_a, d.tsum_b, d.tmax);
    hipLaunchKernelGGL(gb_tile_scan_kernel, dim3(1), dim3(kThreads), 0, s, d.tsum_a, d.tsum_b, (const int32_t *)d.tmax, (int)pl.tiles, total, maxword);
    hipLaunchKernelGGL(gb_scan_apply_kernel, dim3(pl.tiles), dim3(kThreads), 0, s, v, d.n, (const int32_t *)d.tsum_a, (const int32_t *)d.tsum_b,
                       out_a, out_b, node_map);
}

}  // namespace

extern "C" {

int64_t gcc_graph_build_workspace_bytes(int64_t n, int64_t m)
{
    const int rc = check_sizes("gcc_graph_build_workspace_bytes", n, m);
    if (rc) return rc;
    return make_plan(n, m).total;
}

int32_t gcc_graph_build(const gcc_graph_build_args *h, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream)
{
    const char *who = "gcc_graph_build";
    int rc = null_member(who, {{h, "args"}});
    if (rc) return rc;
    if ((rc = check_sizes(who, h->n, h->m))) return rc;
    if ((rc = null_member(who, {{status, "status"}, {h->pairs, "pairs", h->m > 0}, {h->row_ptr, "row_ptr"}, {h->col_idx, "col_idx", h->m > 0},
                                {h->counts, "counts"}})))
        return rc;
    const Plan pl = make_plan(h->n, h->m);
    if ((rc = check_workspace(who, "gcc_graph_build_workspace_bytes", workspace, workspace_bytes, pl.total))) return rc;
    GbDev d = GbDev();
    d.pairs = h->pairs; d.n = (int32_t)h->n; d.m = (int32_t)h->m;
    d.deg = ws_at<int32_t>(workspace, pl.off_deg); d.cursor = ws_at<int32_t>(workspace, pl.off_cursor); d.sc = ws_at<int32_t>(workspace, pl.off_sc);
    d.start = ws_at<int32_t>(workspace, pl.off_start); d.newid = ws_at<int32_t>(workspace, pl.off_newid);
    d.ucount = ws_at<int32_t>(workspace, pl.off_ucount); d.ustart = ws_at<int32_t>(workspace, pl.off_ustart);
    d.tsum_a = ws_at<int32_t>(workspace, pl.off_tsum_a); d.tsum_b = ws_at<int32_t>(workspace, pl.off_tsum_b);
    d.tmax = ws_at<int32_t>(workspace, pl.off_tmax);
    d.list_lds = ws_at<int32_t>(workspace, pl.off_list_lds); d.list_large = ws_at<int32_t>(workspace, pl.off_list_large);
    d.tmp = ws_at<int32_t>(workspace, pl.off_tmp); d.tmp2 = ws_at<int32_t>(workspace, pl.off_tmp2);
    d.cap_lds = pl.cap_lds; d.cap_large = pl.cap_large;
    d.row_ptr = h->row_ptr; d.col_idx = h->col_idx; d.node_map = h->node_map; d.counts = h->counts; d.status = status;
    hipStream_t s = (hipStream_t)stream;
    const dim3 block(kThreads);
    const int line_grid = grid_of(h->m, kLinesPerGroup), row_grid = grid_of(h->n, kWaves);
    (void)hipMemsetAsync(d.deg, 0, (size_t)pl.zero_bytes, s);
    if (h->m > 0) hipLaunchKernelGGL(gb_degree_kernel, dim3(line_grid), block, 0, s, d);
    launch_scan(d, pl, d.deg, d.start, d.newid, d.node_map, d.sc + SC_RAW_TOTAL, d.sc + SC_MAX_SLOTS, s);
    if (h->m > 0) hipLaunchKernelGGL(gb_scatter_kernel, dim3(line_grid), block, 0, s, d);
    hipLaunchKernelGGL(gb_sort_wave_kernel, dim3(row_grid), block, 0, s, d);
    if (pl.cap_lds > 0) hipLaunchKernelGGL(gb_sort_lds_kernel, dim3(capped(pl.cap_lds)), block, 0, s, d);
    if (pl.cap_large > 0) {
        const int wide = capped(grid_of(2 * h->m, kLdsRow));
        hipLaunchKernelGGL(gb_sort_chunks_kernel, dim3(wide), block, 0, s, d);
        for (int pass = 0; pass < pl.passes; ++pass) hipLaunchKernelGGL(gb_merge_kernel, dim3(wide), block, 0, s, d, pass);
        hipLaunchKernelGGL(gb_unique_large_kernel, dim3(capped(pl.cap_large)), block, 0, s, d);
    }
    launch_scan(d, pl, d.ucount, d.ustart, nullptr, nullptr, d.sc + SC_UNIQ_TOTAL, d.sc + SC_MAX_DEGREE, s);
    hipLaunchKernelGGL(gb_compact_kernel, dim3(row_grid), block, 0, s, d);
    if (pl.cap_large > 0) hipLaunchKernelGGL(gb_compact_large_kernel, dim3(capped(grid_of(2 * h->m, kLdsRow))), block, 0, s, d);
    hipLaunchKernelGGL(gb_finish_kernel, dim3(1), dim3(64), 0, s, d);
    return launched();
}

int32_t gcc_graph_check(const gcc_graph_check_args *h, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream)
{
    const char *who = "gcc_graph_check";
    (void)workspace;
    (void)workspace_bytes;                            // (the check keeps nothing: a workspace is accepted and not used)
    int rc = null_member(who, {{h, "args"}});
    if (rc) return rc;
    if (h->n < 1 || h->n > INT32_MAX || h->nnz < 0 || h->nnz > INT32_MAX) {
        snprintf(g_err, kErrLen, "%s: n %lld / nnz %lld: 1 <= n and both must fit int32", who, (long long)h->n, (long long)h->nnz);
        return -2;
    }
    if ((rc = null_member(who, {{status, "status"}, {h->row_ptr, "row_ptr"}, {h->col_idx, "col_idx", h->nnz > 0}, {h->maxima, "maxima"}})))
        return rc;
    GcDev d = GcDev();
    d.rp = h->row_ptr; d.ci = h->col_idx; d.n = (int32_t)h->n; d.nnz = (int32_t)h->nnz; d.multigraph = h->multigraph != 0;
    d.maxima = h->maxima; d.status = status;
    hipStream_t s = (hipStream_t)stream;
    (void)hipMemsetAsync(d.maxima, 0, 8, s);
    hipLaunchKernelGGL(gc_rows_kernel, dim3(capped(grid_of(h->n, kThreads))), dim3(kThreads), 0, s, d);
    if (h->nnz > 0) {
        const int64_t tiles = (h->nnz + kEntryTile - 1) / kEntryTile;
        const dim3 grid((unsigned)(tiles < kEntryGrid ? tiles : kEntryGrid));
        hipLaunchKernelGGL(gc_entries_kernel, grid, dim3(kThreads), 0, s, d);
        hipLaunchKernelGGL(gc_sym_kernel, grid, dim3(kThreads), 0, s, d);
    }
    return launched();
}

}  // extern "C"
