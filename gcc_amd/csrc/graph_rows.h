// gcc_amd/csrc/graph_rows.h -- what graph_build.hip and tu_corpus.hip share: the on-chip gathering of same-address atomics, the
// tiled exclusive scan of (v, v > 0), and the three row-sort classes (a wave in registers, a workgroup in LDS, chunks merged in the
// workspace) with the removal of repeats, each as the body of a kernel: a file that includes this header wraps the bodies in
// kernels of its own (gb_*_kernel in graph_build.hip, whose head describes them; tu_*_kernel in tu_corpus.hip).  File-local like the rest of
// the kit: every source file that includes this header gets its own copy.
#pragma once
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
__device__ __forceinline__ void gb_tile_sum_body(const int32_t *v, int n, int32_t *tsum_a, int32_t *tsum_b, int32_t *tmax)
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
__device__ __forceinline__ void gb_tile_scan_body(int32_t *tsum_a, int32_t *tsum_b, const int32_t *tmax, int tiles, int32_t *total,
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
__device__ __forceinline__ void gb_scan_apply_body(const int32_t *v, int n, const int32_t *tsum_a, const int32_t *tsum_b,
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

__device__ __forceinline__ void gb_sort_wave_body(GbDev a)
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

__device__ __forceinline__ void gb_sort_lds_body(GbDev a)
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

__device__ __forceinline__ void gb_sort_chunks_body(GbDev a)
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
__device__ __forceinline__ void gb_merge_body(GbDev a, int pass)
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
__device__ __forceinline__ void gb_unique_large_body(GbDev a)
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

}  // namespace
