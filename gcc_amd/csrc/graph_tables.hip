// gcc_amd/csrc/graph_tables.hip -- the sampler's tables from a CSR that is already in HBM (gfx950): the summary a DeviceGraph sizes
// itself with (longest row, sum d, sum d^2, rows of at least hub_degree entries), the seed cdf of d^0.75 per worker shard, and the
// hub index / hub-hub bitmap of gcc_graph.  What gcc_amd.graph.seed_cdf_table and hub_tables compute on the host.
//
//   gt_tile_sums_kernel     a workgroup per tile of GCC_GRAPH_TABLES_SCAN_TILE nodes (tiles never straddle a shard): the tile's total
//                           weight BY THE RULE BELOW, its number of hub rows, and the summary's integer sums (one atomic per
//                           workgroup and word).
//   gt_offsets_kernel       a wave per shard adds the shard's tile totals one after another (the tiles' offsets, the shard's total;
//                           a total that is zero or not finite sets GCC_STATUS_GRAPH_TABLES_EMPTY_SHARD); one more wave scans the
//                           tiles' hub counts.
//   gt_apply_kernel         the tile's prefixes again, the same bits: cdf = (offset + prefix) / shard total, and hub_index.
//   gt_hub_adj_kernel       gcc_graph_tables_hub_adj: tiles of GCC_GRAPH_TABLES_ENTRY_TILE ENTRIES, the row of an entry found by a
//                           binary search (as gc_entries_kernel of graph_build.hip: a hub's row of 10^5 entries is spread over a
//                           hundred workgroups), one integer atomic OR per hub-hub entry.
//
// THE CDF RULE.  rwr_walk_kernel's 256-ary search needs a cdf that never descends; a tree scan of positive floats does not promise
// that.  Here every level carries its offsets forward one after another and the next level's item IS the last prefix of the one
// below:  a lane adds its kPer weights in order (r_k); the lanes' offsets of a wave are o_0 = 0, o_{l+1} = o_l + r_last(l); the
// waves' offsets W_0 = 0, W_{v+1} = W_v + o_64(v); the tile's total is W_4; the tiles' offsets T_0 = 0, T_{j+1} = T_j + total_j.
// An element is T_j + (W_v + (o_l + r_k)).  Rounded addition is monotone in either operand, so within a lane, from a lane's last
// element (W_v + o_{l+1}) to the next lane's first, from a wave's last (W_{v+1}) to the next wave's first, and from a tile's last
// (T_{j+1}) to the next tile's first the value never falls; the shard's total is its last element, so the cdf ends in exactly 1.0.
// The order of additions depends on the tile grid alone: any grid size and any two calls give the same bits.  d^0.75 is
// sqrt(d) * sqrt(sqrt(d)) (correctly rounded square roots: 3.5 units of 2^-53 at most).
#include "task_common.h"

#include <limits.h>
#include <math.h>

#include <vector>

namespace {

constexpr int kThreads = 256, kWaves = 4;
constexpr int kTile = GCC_GRAPH_TABLES_SCAN_TILE, kPer = kTile / kThreads;
constexpr int kEntryTile = GCC_GRAPH_TABLES_ENTRY_TILE;
constexpr int kTileGrid = 4096, kEntryGrid = 16384, kMaxGrid = 65535;
static_assert(kTile == kThreads * kPer && kPer == 8, "a scan tile");

enum { SUM_MAX_DEGREE, SUM_D, SUM_D2, SUM_HUBS, SUM_STATUS, SUM_BAD_SHARD, SUM_WORDS = GCC_GRAPH_TABLES_SUMMARY_WORDS };

struct GtDev {
    const int32_t *rp;
    int32_t n, shards, tiles, hub_degree;
    const int64_t *shard_off, *tile_base;             // workspace copies of the host's tables, [shards + 1] each
    double *tile_sum, *tile_off, *shard_total;
    int32_t *tile_hubs;
    unsigned long long *summary;
    double *cdf;
    int32_t *hub_index, *status;
};

struct TileRef {
    int lo, hi, shard;                                // nodes [lo, hi)
};
// (every lane reads the same addresses)
__device__ __forceinline__ TileRef tile_ref(const GtDev &a, int t)
{
    int s = 0, above = a.shards;                      // the last s with tile_base[s] <= t
    while (above - s > 1) {
        const int mid = (s + above) >> 1;
        if (a.tile_base[mid] <= t) s = mid;
        else above = mid;
    }
    const long long b = a.shard_off[s] + (long long)(t - a.tile_base[s]) * kTile, end = a.shard_off[s + 1];
    TileRef r;
    r.lo = (int)b;
    r.hi = (int)(b + kTile < end ? b + kTile : end);
    r.shard = s;
    return r;
}

__device__ __forceinline__ double seed_weight(int d)
{
    if (d <= 0) return 0.0;
    const double x = sqrt((double)d);
    return x * sqrt(x);
}

// The tile's degrees and their prefixes by the rule above -> the tile's total (its last prefix; nodes past tl.hi weigh 0 and leave
// every value as it is).  All threads call; red: [kWaves] of LDS.
__device__ __forceinline__ double tile_prefix(const GtDev &a, const TileRef &tl, int (&d)[kPer], double (&p)[kPer], double *red)
{
    const int lane = lane_id(), wv = (int)threadIdx.x >> 6;
    const long long i0 = (long long)tl.lo + (long long)threadIdx.x * kPer;
    double r = 0.0;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        d[k] = i0 + k < tl.hi ? a.rp[i0 + k + 1] - a.rp[i0 + k] : 0;
        r = r + seed_weight(d[k]);
        p[k] = r;
    }
    double o = 0.0, mine = 0.0;
#pragma unroll 4                                      // (unrolled fully, the 64 lane values take 128 scalar registers at once and spill)
    for (int l = 0; l < 64; ++l) {
        if (lane == l) mine = o;
        o = o + wave_readlane(r, l);
    }
    if (lane == 0) red[wv] = o;
    __syncthreads();
    double W = 0.0, total = 0.0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        if (w == wv) W = total;
        total = total + red[w];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPer; ++k) p[k] = W + (mine + p[k]);
    return total;
}

__device__ __forceinline__ long long wave_sum_i64(long long v)
{
    for (int d = 32; d >= 1; d >>= 1) v += wave_shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ int wave_max_i32(int v)
{
    for (int d = 32; d >= 1; d >>= 1) {
        const int t = wave_shfl_xor(v, d);
        v = t > v ? t : v;
    }
    return v;
}

__device__ __forceinline__ int hub_rows(const GtDev &a, const int (&d)[kPer])
{
    int c = 0;
#pragma unroll
    for (int k = 0; k < kPer; ++k) c += d[k] >= a.hub_degree;
    return c;
}

__global__ __launch_bounds__(kThreads) void gt_tile_sums_kernel(GtDev a)
{
    __shared__ double red[kWaves];
    __shared__ long long redi[3][kWaves];
    __shared__ int redm[kWaves];
    const int lane = lane_id(), wv = (int)threadIdx.x >> 6;
    long long sd = 0, sd2 = 0;
    int mx = 0;
    for (int t = (int)blockIdx.x; t < a.tiles; t += (int)gridDim.x) {
        const TileRef tl = tile_ref(a, t);
        int d[kPer];
        double p[kPer];
        const double total = tile_prefix(a, tl, d, p, red);
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            sd += d[k];
            sd2 += (long long)d[k] * d[k];
            mx = d[k] > mx ? d[k] : mx;
        }
        const long long hubs = wave_sum_i64(hub_rows(a, d));
        if (lane == 0) redi[0][wv] = hubs;
        __syncthreads();
        if (threadIdx.x == 0) {
            a.tile_sum[t] = total;
            a.tile_hubs[t] = (int32_t)(redi[0][0] + redi[0][1] + redi[0][2] + redi[0][3]);
        }
        __syncthreads();
    }
    sd = wave_sum_i64(sd);
    sd2 = wave_sum_i64(sd2);
    mx = wave_max_i32(mx);
    if (lane == 0) {
        redi[1][wv] = sd;
        redi[2][wv] = sd2;
        redm[wv] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kWaves; ++w) {
            sd += redi[1][w];
            sd2 += redi[2][w];
            mx = redm[w] > mx ? redm[w] : mx;
        }
        atomicAdd(&a.summary[SUM_D], (unsigned long long)sd);
        atomicAdd(&a.summary[SUM_D2], (unsigned long long)sd2);
        atomicMax(&a.summary[SUM_MAX_DEGREE], (unsigned long long)mx);
    }
}

// workgroup s < shards (one wave): the offsets of shard s's tiles and its total; workgroup `shards`: the tiles' hub counts -> their
// exclusive prefixes in place, the number of hubs -> the summary
__global__ __launch_bounds__(64) void gt_offsets_kernel(GtDev a)
{
    const int lane = lane_id(), s = (int)blockIdx.x;
    if (s == a.shards) {
        int carry = 0;
        for (int base = 0; base < a.tiles; base += 64) {
            const int t = base + lane, x = t < a.tiles ? a.tile_hubs[t] : 0;
            const int incl = wave_scan_incl(x);
            if (t < a.tiles) a.tile_hubs[t] = carry + incl - x;
            carry += wave_last(incl);
        }
        if (lane == 0) a.summary[SUM_HUBS] = (unsigned long long)carry;
        return;
    }
    const int t0 = (int)a.tile_base[s], t1 = (int)a.tile_base[s + 1];
    double carry = 0.0;
    for (int base = t0; base < t1; base += 64) {
        const int t = base + lane;
        const double x = t < t1 ? a.tile_sum[t] : 0.0;
        double mine = 0.0;
#pragma unroll 4
        for (int l = 0; l < 64; ++l) {
            if (lane == l) mine = carry;
            carry = carry + wave_readlane(x, l);
        }
        if (t < t1) a.tile_off[t] = mine;
    }
    if (lane == 0) {
        a.shard_total[s] = carry;
        if (!(carry > 0.0 && carry < (double)INFINITY)) {
            atomicOr(a.status, (int32_t)GCC_STATUS_GRAPH_TABLES_EMPTY_SHARD);
            atomicOr(&a.summary[SUM_STATUS], (unsigned long long)GCC_STATUS_GRAPH_TABLES_EMPTY_SHARD);
            atomicMax(&a.summary[SUM_BAD_SHARD], (unsigned long long)(a.shards - s));       // (the lowest such shard wins)
        }
    }
}

__global__ __launch_bounds__(kThreads) void gt_apply_kernel(GtDev a)
{
    __shared__ double red[kWaves];
    __shared__ int redh[kWaves];
    const int lane = lane_id(), wv = (int)threadIdx.x >> 6;
    for (int t = (int)blockIdx.x; t < a.tiles; t += (int)gridDim.x) {
        const TileRef tl = tile_ref(a, t);
        int d[kPer];
        double p[kPer];
        tile_prefix(a, tl, d, p, red);
        const double off = a.tile_off[t], total = a.shard_total[tl.shard];
        const bool sound = total > 0.0 && total < (double)INFINITY;          // (else the status bit is set: 1.0, never a NaN)
        const long long i0 = (long long)tl.lo + (long long)threadIdx.x * kPer;
#pragma unroll
        for (int k = 0; k < kPer; ++k)
            if (i0 + k < tl.hi) a.cdf[i0 + k] = sound ? (off + p[k]) / total : 1.0;
        if (a.hub_index) {
            const int c = hub_rows(a, d), incl = wave_scan_incl(c);
            if (lane == 63) redh[wv] = incl;
            __syncthreads();
            int h = a.tile_hubs[t] + incl - c;
            for (int w = 0; w < wv; ++w) h += redh[w];
#pragma unroll
            for (int k = 0; k < kPer; ++k)
                if (i0 + k < tl.hi) a.hub_index[i0 + k] = d[k] >= a.hub_degree ? h++ : -1;
            __syncthreads();
        }
    }
}

// ---------------------------------------------------------------- the bitmap
struct GhDev {
    const int32_t *rp, *ci, *hub_index;
    uint32_t *adj;
    int32_t n, nnz, hubs, words;
};

// the last row of [lo, hi] that begins at or before entry q (lo when none does: a row_ptr that does not climb gives a wrong row,
// never one outside [lo, hi])
__device__ __forceinline__ int row_of(const int32_t *rp, int lo, int hi, int q)
{
    int b = lo, e = hi + 1;
    while (b < e) {
        const int mid = b + ((e - b) >> 1);
        if (rp[mid] <= q) b = mid + 1;
        else e = mid;
    }
    return b - 1 > lo ? b - 1 : lo;
}

__global__ __launch_bounds__(kThreads) void gt_hub_adj_kernel(GhDev a)
{
    const long long tiles = ((long long)a.nnz + kEntryTile - 1) / kEntryTile;
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int q0 = (int)(t * kEntryTile), q1 = t * kEntryTile + kEntryTile < a.nnz ? (int)(t * kEntryTile + kEntryTile) : a.nnz;
        const int r0 = row_of(a.rp, 0, a.n - 1, q0), r1 = row_of(a.rp, r0, a.n - 1, q1 - 1);
        for (int q = q0 + (int)threadIdx.x; q < q1; q += kThreads) {
            const int hr = a.hub_index[row_of(a.rp, r0, r1, q)];
            if ((unsigned)hr >= (unsigned)a.hubs) continue;          // (-1: not a hub)
            const int c = a.ci[q];
            if ((unsigned)c >= (unsigned)a.n) continue;
            const int hc = a.hub_index[c];
            if ((unsigned)hc >= (unsigned)a.hubs) continue;
            atomicOr(&a.adj[(size_t)hr * a.words + (hc >> 5)], 1u << (hc & 31));
        }
    }
}

// ---------------------------------------------------------------- host
struct Plan {
    int64_t off_table, off_tile_sum, off_tile_off, off_shard_total, off_tile_hubs, total;
    int64_t shards, tiles_cap;
};

int check_sizes(const char *who, int64_t n, int64_t nnz, int64_t num_shards)
{
    if (n < 1 || n > INT32_MAX || nnz < 0 || nnz > INT32_MAX) {
        snprintf(g_err, kErrLen, "%s: n %lld / nnz %lld: 1 <= n and both must fit int32", who, (long long)n, (long long)nnz);
        return -2;
    }
    if (num_shards < 0 || num_shards > n) {
        snprintf(g_err, kErrLen, "%s: num_shards %lld outside 0..n", who, (long long)num_shards);
        return -2;
    }
    return 0;
}

// (a shard ends in a tile of its own: at most one more tile per shard than the nodes fill)
Plan make_plan(int64_t n, int64_t num_shards)
{
    Plan p;
    p.shards = num_shards < 1 ? 1 : num_shards;
    p.tiles_cap = (n + kTile - 1) / kTile + p.shards;
    Carve cv;
    p.off_table = cv.take(2 * (p.shards + 1) * 8);
    p.off_tile_sum = cv.take(p.tiles_cap * 8);
    p.off_tile_off = cv.take(p.tiles_cap * 8);
    p.off_shard_total = cv.take(p.shards * 8);
    p.off_tile_hubs = cv.take(p.tiles_cap * 4);
    p.total = cv.total();
    return p;
}

int grid_for(int64_t items, int32_t asked, int cap)
{
    int64_t g = asked > 0 ? asked : (items < cap ? items : cap);
    return (int)(g < 1 ? 1 : g > kMaxGrid ? kMaxGrid : g);
}

int64_t hub_bytes_limit(const gcc_graph_tables_args *h) { return h->max_hub_bytes > 0 ? h->max_hub_bytes : (int64_t)1 << 30; }

#ifdef GCC_AMD_HIPEMU
constexpr int kHostToDevice = 1;                      // (the emulator's copy is a memcpy whatever the kind)
#else
constexpr hipMemcpyKind kHostToDevice = hipMemcpyHostToDevice;
#endif

// the shard table a call uploads; kept until the thread's next call
thread_local std::vector<int64_t> g_table;

}  // namespace

extern "C" {

int64_t gcc_graph_tables_workspace_bytes(int64_t n, int32_t num_shards)
{
    const int rc = check_sizes("gcc_graph_tables_workspace_bytes", n, 0, num_shards);
    if (rc) return rc;
    return make_plan(n, num_shards).total;
}

int32_t gcc_graph_tables(const gcc_graph_tables_args *h, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream)
{
    const char *who = "gcc_graph_tables";
    int rc = null_member(who, {{h, "args"}});
    if (rc) return rc;
    if ((rc = check_sizes(who, h->n, h->nnz, h->num_shards))) return rc;
    if ((rc = null_member(who, {{status, "status"}, {h->row_ptr, "row_ptr"}, {h->summary, "summary"}, {h->seed_cdf, "seed_cdf"},
                                {h->shard_off, "shard_off", h->num_shards > 1}})))
        return rc;
    if (h->hub_degree < 0) {
        snprintf(g_err, kErrLen, "%s: hub_degree %d is negative", who, (int)h->hub_degree);
        return -2;
    }
    const Plan pl = make_plan(h->n, h->num_shards);
    const int S = (int)pl.shards;
    g_table.assign(2 * (size_t)(S + 1), 0);
    int64_t *so = g_table.data(), *tb = so + S + 1;
    if (h->shard_off && h->num_shards >= 1) {
        bool ok = h->shard_off[0] == 0 && h->shard_off[S] == h->n;
        for (int s = 0; s < S && ok; ++s) ok = h->shard_off[s + 1] > h->shard_off[s];
        if (!ok) {
            snprintf(g_err, kErrLen, "%s: shard_off must be increasing node offsets from 0 to n (no empty shard)", who);
            return -2;
        }
        for (int s = 0; s <= S; ++s) so[s] = h->shard_off[s];
    } else {
        so[1] = h->n;
    }
    for (int s = 0; s < S; ++s) tb[s + 1] = tb[s] + (so[s + 1] - so[s] + kTile - 1) / kTile;
    if ((rc = check_workspace(who, "gcc_graph_tables_workspace_bytes", workspace, workspace_bytes, pl.total))) return rc;
    GtDev d = GtDev();
    d.rp = h->row_ptr; d.n = (int32_t)h->n; d.shards = S; d.tiles = (int32_t)tb[S];
    d.hub_degree = h->hub_degree > 0 ? h->hub_degree : GCC_GRAPH_TABLES_HUB_DEGREE;
    int64_t *table = ws_at<int64_t>(workspace, pl.off_table);
    d.shard_off = table; d.tile_base = table + S + 1;
    d.tile_sum = ws_at<double>(workspace, pl.off_tile_sum); d.tile_off = ws_at<double>(workspace, pl.off_tile_off);
    d.shard_total = ws_at<double>(workspace, pl.off_shard_total); d.tile_hubs = ws_at<int32_t>(workspace, pl.off_tile_hubs);
    d.summary = reinterpret_cast<unsigned long long *>(h->summary); d.cdf = h->seed_cdf; d.hub_index = h->hub_index; d.status = status;
    hipStream_t s = (hipStream_t)stream;
    (void)hipMemcpyAsync(table, g_table.data(), g_table.size() * 8, kHostToDevice, s);
    (void)hipMemsetAsync(d.summary, 0, SUM_WORDS * 8, s);
    const int grid = grid_for(d.tiles, h->grid, kTileGrid);
    hipLaunchKernelGGL(gt_tile_sums_kernel, dim3(grid), dim3(kThreads), 0, s, d);
    hipLaunchKernelGGL(gt_offsets_kernel, dim3(S + 1), dim3(64), 0, s, d);
    hipLaunchKernelGGL(gt_apply_kernel, dim3(grid), dim3(kThreads), 0, s, d);
    return launched();
}

int32_t gcc_graph_tables_hub_adj(const gcc_graph_tables_args *h, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream)
{
    const char *who = "gcc_graph_tables_hub_adj";
    (void)workspace;
    (void)workspace_bytes;                            // (the bitmap is the only thing written: a workspace is accepted and not used)
    int rc = null_member(who, {{h, "args"}});
    if (rc) return rc;
    if ((rc = check_sizes(who, h->n, h->nnz, 0))) return rc;
    if ((rc = null_member(who, {{status, "status"}, {h->row_ptr, "row_ptr"}, {h->col_idx, "col_idx", h->nnz > 0}, {h->hub_index, "hub_index"},
                                {h->hub_adj, "hub_adj"}})))
        return rc;
    if (h->num_hubs < 1 || h->num_hubs > h->n || h->hub_words != (h->num_hubs + 31) / 32) {
        snprintf(g_err, kErrLen, "%s: num_hubs %d / hub_words %d: 1 <= num_hubs <= n, hub_words = (num_hubs + 31) / 32", who, (int)h->num_hubs,
                 (int)h->hub_words);
        return -2;
    }
    const int64_t bytes = (int64_t)h->num_hubs * h->hub_words * 4;
    if (bytes > hub_bytes_limit(h)) {
        snprintf(g_err, kErrLen, "%s: the bitmap of %d hubs takes %lld bytes, max_hub_bytes is %lld", who, (int)h->num_hubs, (long long)bytes,
                 (long long)hub_bytes_limit(h));
        return -2;
    }
    GhDev d = GhDev();
    d.rp = h->row_ptr; d.ci = h->col_idx; d.hub_index = h->hub_index; d.adj = h->hub_adj;
    d.n = (int32_t)h->n; d.nnz = (int32_t)h->nnz; d.hubs = h->num_hubs; d.words = h->hub_words;
    hipStream_t s = (hipStream_t)stream;
    (void)hipMemsetAsync(d.adj, 0, (size_t)bytes, s);
    if (h->nnz > 0) {
        const int64_t tiles = (h->nnz + kEntryTile - 1) / kEntryTile;
        hipLaunchKernelGGL(gt_hub_adj_kernel, dim3(grid_for(tiles, h->grid, kEntryGrid)), dim3(kThreads), 0, s, d);
    }
    return launched();
}

}  // extern "C"
