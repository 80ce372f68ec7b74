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
#include "task_common.h"

#include <limits.h>

namespace {

constexpr int kThreads = 256, kWaves = 4;
constexpr int kWaveRow = GCC_GRAPH_BUILD_WAVE_ROW;
constexpr int kLdsRow = GCC_GRAPH_BUILD_LDS_ROW;
constexpr int kTile = GCC_GRAPH_BUILD_SCAN_TILE, kPer = kTile / kThreads;
constexpr int kPad = INT32_MAX;                       // above every node id (n <= INT32_MAX)
constexpr int kListGrid = 2048;                       // workgroups of a kernel that walks a list or strides over rows
static_assert(kWaveRow == 64, "a wave's row");
static_assert((kLdsRow & (kLdsRow - 1)) == 0 && kLdsRow >= 2 * kThreads, "the LDS sort works on a power of two");
static_assert(kTile == kThreads * kPer && kPer == 4, "a scan tile");

enum { SC_RAW_TOTAL, SC_KEPT, SC_UNIQ_TOTAL, SC_KEPT_AGAIN, SC_SELF_LOOPS, SC_MAX_DEGREE, SC_N_LDS, SC_N_LARGE, SC_MAX_SLOTS, SC_WORDS = 16 };

struct GbDev {
    const int32_t *pairs;
    int32_t n, m;
    int32_t *deg, *cursor, *sc;                       // zeroed by one memset at the start of a call
    int32_t *start, *newid, *ucount, *ustart, *tsum_a, *tsum_b, *tmax, *list_lds, *list_large, *tmp, *tmp2;
    int32_t cap_lds, cap_large;
    int32_t *row_ptr, *col_idx, *node_map;
    int64_t *counts;
    int32_t *status;
};

__device__ __forceinline__ int popc64(unsigned long long x) { return __builtin_popcountll(x); }

// The adds of a workgroup's lines to word[id], gathered on chip first: one word takes about 88 returning atomics per microsecond, and
// a hub of 10^5 lines would put that many on its one word.  Two steps of gathering:
//   * adjacent lanes with the same id form a run, and only the run's first lane goes on (a hub's lines in a sorted file fill whole
//     waves);
//   * the run enters a small hash table in LDS (LDS atomics: a compare-and-swap claims a slot for the id, two probes), so that the
//     lines of one id anywhere in the workgroup's kLinesPerGroup lines share ONE global atomic, issued by flush().  A run that finds
//     both slots taken by other ids adds to the global word itself.
// A lane keeps (slot, rank): after flush() its place is base[slot] + rank, or rank itself when slot < 0.
constexpr int kHashBits = 11, kHash = 1 << kHashBits;
constexpr int kLinesPer = 4, kLinesPerGroup = kThreads * kLinesPer;
struct Gather {
    int32_t key[kHash], cnt[kHash], base[kHash];
};
struct Place {
    int slot, rank;
};

__device__ __forceinline__ void gather_clear(Gather &g)
{
    for (int h = (int)threadIdx.x; h < kHash; h += kThreads) {
        g.key[h] = -1;
        g.cnt[h] = 0;
    }
    __syncthreads();
}

// every lane of the wave calls; `on`: the lane adds 1 to word[key]
__device__ __forceinline__ Place gather_add(Gather &g, int32_t *word, bool on, int key)
{
    const int lane = lane_id(), k = on ? key : -1;
    const int prev = wave_shfl_up(k, 1);
    const bool head = on && (lane == 0 || prev != k);
    const unsigned long long heads = wave_ballot(head), ons = wave_ballot(on);
    const unsigned long long upto = lanemask_lt() | (1ull << lane);
    const unsigned long long mine = heads & upto;
    const int first = mine ? 63 - __builtin_clzll(mine) : lane;
    const unsigned long long above = (heads | ~ons) & ~upto;
    const int end = above ? __builtin_ctzll(above) : 64;
    int slot = -1, rank = 0;
    if (head) {
        unsigned h = ((unsigned)k * 2654435761u) >> (32 - kHashBits);
        for (int probe = 0; probe < 2 && slot < 0; ++probe, h = (h + 1) & (kHash - 1)) {
            const int old = atomicCAS(&g.key[h], (int32_t)-1, (int32_t)k);
            if (old == -1 || old == k) slot = (int)h;
        }
        rank = slot >= 0 ? atomicAdd(&g.cnt[slot], (int32_t)(end - lane)) : atomicAdd(&word[k], (int32_t)(end - lane));
    }
    Place p;
    p.slot = wave_shfl(slot, first);
    p.rank = wave_shfl(rank, first) + (lane - first);
    return p;
}

// one global atomic per id the table holds; a barrier on both sides
__device__ __forceinline__ void gather_flush(Gather &g, int32_t *word)
{
    __syncthreads();
    for (int h = (int)threadIdx.x; h < kHash; h += kThreads)
        if (g.cnt[h]) g.base[h] = atomicAdd(&word[g.key[h]], g.cnt[h]);
    __syncthreads();
}

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

// exclusive prefix of (x, y) over the workgroup in thread order, and the totals; red: [2][kWaves] of LDS
__device__ __forceinline__ void block_scan2(int x, int y, int &ex, int &ey, int &tx, int &ty, int (*red)[kWaves])
{
    const int lane = lane_id(), wv = (int)threadIdx.x >> 6;
    const int ix = wave_scan_incl(x), iy = wave_scan_incl(y);
    if (lane == 63) {
        red[0][wv] = ix;
        red[1][wv] = iy;
    }
    __syncthreads();
    int bx = 0, by = 0;
    tx = ty = 0;
    for (int w = 0; w < kWaves; ++w) {
        if (w < wv) {
            bx += red[0][w];
            by += red[1][w];
        }
        tx += red[0][w];
        ty += red[1][w];
    }
    __syncthreads();
    ex = bx + ix - x;
    ey = by + iy - y;
}

__device__ __forceinline__ int wave_max_i32(int v)
{
    for (int d = 32; d >= 1; d >>= 1) {
        const int t = wave_shfl_xor(v, d);
        v = t > v ? t : v;
    }
    return v;
}

// the tile's sums of (v, v > 0) and its largest value
__global__ __launch_bounds__(kThreads) void gb_tile_sum_kernel(const int32_t *v, int n, int32_t *tsum_a, int32_t *tsum_b, int32_t *tmax)
{
    __shared__ int red[2][kWaves];
    __shared__ int redm[kWaves];
    const long long i0 = (long long)blockIdx.x * kTile + (long long)threadIdx.x * kPer;
    int x = 0, y = 0, mx = 0;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int d = i0 + k < n ? v[i0 + k] : 0;
        x += d;
        y += d > 0;
        mx = d > mx ? d : mx;
    }
    int ex, ey, tx, ty;
    block_scan2(x, y, ex, ey, tx, ty, red);
    if (threadIdx.x == 0) {
        tsum_a[blockIdx.x] = tx;
        tsum_b[blockIdx.x] = ty;
    }
    mx = wave_max_i32(mx);
    if (lane_id() == 0) redm[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kWaves; ++w) mx = redm[w] > mx ? redm[w] : mx;
        tmax[blockIdx.x] = mx;
    }
}

// one workgroup: the tiles' sums -> their exclusive prefixes, in place; the totals -> total[0], total[1]; the largest value -> *maxword
// (no atomic: one per tile on one word took as long as the scan itself at 10^7 nodes)
__global__ __launch_bounds__(kThreads) void gb_tile_scan_kernel(int32_t *tsum_a, int32_t *tsum_b, const int32_t *tmax, int tiles, int32_t *total,
                                                                int32_t *maxword)
{
    __shared__ int red[2][kWaves];
    __shared__ int redm[kWaves];
    int ca = 0, cb = 0, mx = 0;
    for (int base = 0; base < tiles; base += kThreads) {
        const int t = base + (int)threadIdx.x;
        const int x = t < tiles ? tsum_a[t] : 0, y = t < tiles ? tsum_b[t] : 0, m = t < tiles ? tmax[t] : 0;
        int ex, ey, tx, ty;
        block_scan2(x, y, ex, ey, tx, ty, red);
        if (t < tiles) {
            tsum_a[t] = ca + ex;
            tsum_b[t] = cb + ey;
        }
        ca += tx;
        cb += ty;
        mx = m > mx ? m : mx;
    }
    mx = wave_max_i32(mx);
    if (lane_id() == 0) redm[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kWaves; ++w) mx = redm[w] > mx ? redm[w] : mx;
        total[0] = ca;
        total[1] = cb;
        *maxword = mx;
    }
}

// out_a[i] = sum of v[< i], out_b[i] = the number of v[< i] > 0; node_map[i] = v[i] > 0 ? out_b[i] : -1
__global__ __launch_bounds__(kThreads) void gb_scan_apply_kernel(const int32_t *v, int n, const int32_t *tsum_a, const int32_t *tsum_b,
                                                                 int32_t *out_a, int32_t *out_b, int32_t *node_map)
{
    __shared__ int red[2][kWaves];
    const long long i0 = (long long)blockIdx.x * kTile + (long long)threadIdx.x * kPer;
    int d[kPer], x = 0, y = 0;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        d[k] = i0 + k < n ? v[i0 + k] : 0;
        x += d[k];
        y += d[k] > 0;
    }
    int ex, ey, tx, ty;
    block_scan2(x, y, ex, ey, tx, ty, red);
    int oa = tsum_a[blockIdx.x] + ex, ob = tsum_b[blockIdx.x] + ey;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        if (i0 + k < n) {
            out_a[i0 + k] = oa;
            if (out_b) out_b[i0 + k] = ob;
            if (node_map) node_map[i0 + k] = d[k] > 0 ? ob : -1;
        }
        oa += d[k];
        ob += d[k] > 0;
    }
}

__global__ __launch_bounds__(kThreads) void gb_sort_wave_kernel(GbDev a)
{
    const int lane = lane_id();
    const long long i64 = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (i64 >= a.n) return;                                         // (the whole wave)
    const int i = wave_uniform((int)i64);
    const int d = wave_uniform(a.deg[i]);
    if (d > kWaveRow) {
        if (lane == 0) {
            const bool lds = d <= kLdsRow;
            const int at = atomicAdd(&a.sc[lds ? SC_N_LDS : SC_N_LARGE], 1);
            if (at < (lds ? a.cap_lds : a.cap_large)) (lds ? a.list_lds : a.list_large)[at] = i;
        }
        return;
    }
    if (d == 0) {
        if (lane == 0) a.ucount[i] = 0;
        return;
    }
    const int b = a.start[i];
    int x = lane < d ? a.tmp[b + lane] : kPad;
    for (int k = 2; (k >> 1) < d; k <<= 1)                          // (lanes past the power of two hold the pad and stay put)
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int y = wave_shfl_xor(x, j);
            const bool up = (lane & k) == 0, low = (lane & j) == 0;
            x = (low == up) ? (x < y ? x : y) : (x > y ? x : y);
        }
    const int prev = wave_shfl_up(x, 1);
    const bool keep = lane < d && (lane == 0 || prev != x);
    const unsigned long long kept = wave_ballot(keep);
    if (keep) a.tmp[b + popc64(kept & lanemask_lt())] = x;          // (every lane holds its entry in a register by now)
    if (lane == 0) a.ucount[i] = popc64(kept);
}

// ascending sort of s[0, N), N a power of two, by the workgroup (a barrier must stand between the fill and this call)
__device__ __forceinline__ void lds_bitonic(int32_t *s, int N)
{
    for (int k = 2; k <= N; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = (int)threadIdx.x; t < N; t += kThreads) {
                const int p = t ^ j;
                if (p > t) {
                    const int x = s[t], y = s[p];
                    if ((x > y) == ((t & k) == 0)) {
                        s[t] = y;
                        s[p] = x;
                    }
                }
            }
            __syncthreads();
        }
}

__device__ __forceinline__ int pow2_at_least(int d)
{
    int N = 2;
    while (N < d) N <<= 1;
    return N;
}

__global__ __launch_bounds__(kThreads) void gb_sort_lds_kernel(GbDev a)
{
    __shared__ int32_t s[kLdsRow];
    __shared__ int red[2][kWaves];
    const int rows = min(a.sc[SC_N_LDS], a.cap_lds);
    for (int r = (int)blockIdx.x; r < rows; r += (int)gridDim.x) {
        const int i = a.list_lds[r], d = a.deg[i], b = a.start[i], N = pow2_at_least(d);
        for (int t = (int)threadIdx.x; t < N; t += kThreads) s[t] = t < d ? a.tmp[b + t] : kPad;
        __syncthreads();
        lds_bitonic(s, N);
        int carry = 0;
        for (int base = 0; base < d; base += kThreads) {
            const int t = base + (int)threadIdx.x;
            const int x = t < d ? s[t] : 0;
            const bool keep = t < d && (t == 0 || s[t - 1] != x);
            int ex, ey, tx, ty;
            block_scan2(keep, 0, ex, ey, tx, ty, red);
            if (keep) a.tmp[b + carry + ex] = x;
            carry += tx;
        }
        if (threadIdx.x == 0) a.ucount[i] = carry;
        __syncthreads();
    }
}

// the merge passes a row of d entries goes through: the smallest P with kLdsRow << P >= d
__device__ __forceinline__ int merge_passes(int d)
{
    int P = 0;
    while (((long long)kLdsRow << P) < d) ++P;
    return P;
}

// Every workgroup of a kernel over the long rows walks the whole list; the items of a row (chunks, tiles) go round the grid from
// where the row before it stopped, so that many rows of a few items each still spread over all workgroups.  -> this workgroup's
// first item of a row whose item 0 belongs to workgroup `before`
__device__ __forceinline__ int rotated(int before)
{
    const int g = (int)gridDim.x;
    return ((int)blockIdx.x - before + g) % g;
}

__global__ __launch_bounds__(kThreads) void gb_sort_chunks_kernel(GbDev a)
{
    __shared__ int32_t s[kLdsRow];
    const int rows = min(a.sc[SC_N_LARGE], a.cap_large);
    int before = 0;                                   // chunks of the rows so far, modulo the grid: the workgroup of a row's chunk 0
    for (int r = 0; r < rows; ++r) {
        const int i = a.list_large[r], d = a.deg[i], b = a.start[i];
        const int chunks = (d + kLdsRow - 1) / kLdsRow;
        const int c_first = rotated(before);
        before = (before + chunks) % (int)gridDim.x;
        for (int c = c_first; c < chunks; c += (int)gridDim.x) {
            const int c0 = c * kLdsRow, cnt = min(kLdsRow, d - c0);
            for (int t = (int)threadIdx.x; t < kLdsRow; t += kThreads) s[t] = t < cnt ? a.tmp[b + c0 + t] : kPad;
            __syncthreads();
            lds_bitonic(s, kLdsRow);
            for (int t = (int)threadIdx.x; t < cnt; t += kThreads) a.tmp[b + c0 + t] = s[t];
            __syncthreads();
        }
    }
}

// first index of [lo, hi) whose value is >= x (strict: > x)
template <bool kStrict> __device__ __forceinline__ int bound_of(const int32_t *p, int lo, int hi, int x)
{
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (kStrict ? p[mid] <= x : p[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// pass `pass`: runs of kLdsRow << pass entries merge in pairs; an element's place is its index in its own run plus its rank in
// the sibling (>= for the left run, > for the right one: equal values keep left before right)
__global__ __launch_bounds__(kThreads) void gb_merge_kernel(GbDev a, int pass)
{
    if (pass >= merge_passes(a.sc[SC_MAX_SLOTS])) return;          // (the launches are sized for a row of m slots; the longest one is done)
    const int rows = min(a.sc[SC_N_LARGE], a.cap_large);
    const long long w = (long long)kLdsRow << pass;
    int before = 0;
    for (int r = 0; r < rows; ++r) {
        const int i = a.list_large[r], d = a.deg[i];
        if (pass >= merge_passes(d)) continue;
        const int32_t *src = ((pass & 1) ? a.tmp2 : a.tmp) + a.start[i];
        int32_t *dst = ((pass & 1) ? a.tmp : a.tmp2) + a.start[i];
        const int tiles = (d + kThreads - 1) / kThreads, t_first = rotated(before);
        before = (before + tiles) % (int)gridDim.x;
        for (long long e = (long long)t_first * kThreads + threadIdx.x; e < d; e += (long long)gridDim.x * kThreads) {
            const long long a0 = e / (2 * w) * (2 * w), b0 = a0 + w < d ? a0 + w : d, b1 = a0 + 2 * w < d ? a0 + 2 * w : d;
            const int x = src[e];
            long long at;
            if (e < b0) at = e + (bound_of<false>(src, (int)b0, (int)b1, x) - b0);
            else at = a0 + (e - b0) + (bound_of<true>(src, (int)a0, (int)b0, x) - a0);
            dst[at] = x;
        }
    }
}

// where a long row stands after its merge passes
__device__ __forceinline__ int32_t *large_row(const GbDev &a, int i, int d) { return ((merge_passes(d) & 1) ? a.tmp2 : a.tmp) + a.start[i]; }

// A workgroup per long row drops the repeats in place, 256 entries at a time: an entry moves to an index at or below its own, and
// the one entry the next step reads back (the last of this step) is either untouched or overwritten by itself.
__global__ __launch_bounds__(kThreads) void gb_unique_large_kernel(GbDev a)
{
    __shared__ int red[2][kWaves];
    const int rows = min(a.sc[SC_N_LARGE], a.cap_large);
    for (int r = (int)blockIdx.x; r < rows; r += (int)gridDim.x) {
        const int i = a.list_large[r], d = a.deg[i];
        int32_t *buf = large_row(a, i, d);
        int carry = 0;
        for (int base = 0; base < d; base += kThreads) {
            const int t = base + (int)threadIdx.x;
            const int x = t < d ? buf[t] : 0;
            const bool keep = t < d && (t == 0 || buf[t - 1] != x);
            int ex, ey, tx, ty;
            block_scan2(keep, 0, ex, ey, tx, ty, red);              // (its barriers stand between this step's reads and writes)
            if (keep) buf[carry + ex] = x;
            carry += tx;
        }
        if (threadIdx.x == 0) a.ucount[i] = carry;
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
