// gcc_amd/csrc/graph_batch.hip -- whole-graph batches assembled on the device (gfx950).
//
// Replaces, for GraphClassificationDataset / GraphClassificationDatasetLabeled (graph_dataset.py:306-385 of the reference,
// entire_graph=True), the host loop of gcc_amd/datasets.py: concatenating the selected graphs' rows and columns, graph_id,
// the gather of the cached positional rows, the multiplicity expansion and the host-to-device copies of all of them.
//
//   pack_prefix_kernel    ONE workgroup, one thread per batch row (B <= 1024): sizes of the selected graphs, two block scans
//       (nodes, entries * expand), node_off / edge_off, seed_local / labels, row_ptr[n].  A batch that does not fit the
//       capacities is cut at a graph boundary: the leading graphs that fit are kept, the others become empty graphs (offsets
//       stay monotone and within capacity, every column id points at a live row) and the status word says why.
//   pack_copy_kernel<V>   a flat space of tiles -- 256 output rows each, then 2048 output entries each -- walked by a fixed grid,
//       so a 3,800-node graph is 15 row tiles like 15 small batches' worth and never one workgroup's job.  A tile finds its
//       graphs by binary search in the batch offsets (staged in LDS; they already carry the cut above, so a dropped graph has
//       no tile).  Row tile: graph_id, row_ptr, then the positional rows as one linear destination run of 16-byte (P % 4 == 0)
//       or 8-byte lanes.  Entry tile: col_idx[p] = local id + node_off[b], every source entry `expand` times.
//       Plain vector stores only; the kernel boundary is the hand-off from the offsets to the copies.
#include "host_common.h"

namespace {

constexpr int kMaxB = GCC_PACK_GRAPHS_MAX_BATCH;
constexpr int kPrefixWaves = kMaxB / 64;
constexpr int kCopyThreads = 256;
constexpr int kRowTile = 256;             // output rows per tile
constexpr int kEntTile = 2048;            // output entries per tile
constexpr int kMaxGrid = 1024;            // workgroups of the copy kernel (tiles beyond that are walked)
constexpr int kUnroll = 4;                // positional lanes in flight per thread

struct PackDev {
    const int32_t *node_first, *rp, *ci, *seed, *labels;
    const float *pos;
    const int32_t *idx;
    int32_t G, P, B, expand;
    int32_t *node_off, *edge_off, *graph_id, *row_ptr, *col_idx;
    long long node_cap, edge_cap;
    float *pos_out;
    int32_t *seed_out, *labels_out, *status;
};

__device__ __forceinline__ long long wave_scan_incl_i64(long long v)
{
    const int l = lane_id();
    for (int d = 1; d < 64; d <<= 1) {
        const long long t = wave_shfl_up(v, d);
        if (l >= d) v += t;
    }
    return v;
}

// largest s in [lo, hi) with off[s] <= x, given off[lo] <= x < off[hi] (among equal offsets the last one: the others are empty)
__device__ __forceinline__ int find_slot(const int32_t *off, int lo, int hi, int x)
{
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kMaxB) void pack_prefix_kernel(PackDev a)
{
    __shared__ long long wn_s[kPrefixWaves], we_s[kPrefixWaves], live_s[2];
    __shared__ int32_t bits_s[kPrefixWaves];
    __shared__ int32_t keep_s[kMaxB + 1];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = (int)blockDim.x >> 6;
    const int B = a.B;
    int g = -1, bits = 0;
    if (tid < B) {
        g = a.idx[tid];
        if (g < -1 || g >= a.G) { bits |= GCC_STATUS_PACK_BAD_INDEX; g = -1; }
    }
    long long n = 0, e = 0;
    if (g >= 0) {
        const int f0 = a.node_first[g], f1 = a.node_first[g + 1];
        n = f1 - f0;
        e = (long long)(a.rp[f1] - a.rp[f0]) * a.expand;
    }
    const long long ni = wave_scan_incl_i64(n), ei = wave_scan_incl_i64(e);
    if (lane == 63) { wn_s[wave] = ni; we_s[wave] = ei; }
    if (tid == 0) { live_s[0] = 0; live_s[1] = 0; }
    __syncthreads();
    long long nincl = ni, eincl = ei;
    for (int w = 0; w < wave; ++w) { nincl += wn_s[w]; eincl += we_s[w]; }
    // the sums only grow with the row, so the rows that fit are a leading run of the batch
    const bool over_n = nincl > a.node_cap, over_e = eincl > a.edge_cap;
    const bool keep = tid < B && !over_n && !over_e;
    if (g >= 0) bits |= (over_n ? GCC_STATUS_PACK_NODE_OVERFLOW : 0) | (over_e ? GCC_STATUS_PACK_EDGE_OVERFLOW : 0);
    for (int d = 32; d >= 1; d >>= 1) bits |= wave_shfl_xor(bits, d);
    if (lane == 0) bits_s[wave] = bits;
    keep_s[tid] = keep ? 1 : 0;
    if (tid == 0) keep_s[blockDim.x] = 0;
    __syncthreads();
    if (keep && !keep_s[tid + 1]) { live_s[0] = nincl; live_s[1] = eincl; }       // the last row that fits: the live extents
    __syncthreads();
    const long long n_live = live_s[0], e_live = live_s[1];
    if (tid < B) {
        const long long ne = nincl - n, ee = eincl - e;
        a.node_off[tid] = (int32_t)(ne < n_live ? ne : n_live);
        a.edge_off[tid] = (int32_t)(ee < e_live ? ee : e_live);
        const bool live = keep && g >= 0;
        a.seed_out[tid] = live ? a.seed[g] : 0;
        if (a.labels_out) a.labels_out[tid] = live && a.labels ? a.labels[g] : -1;
    }
    if (tid == 0) {
        a.node_off[B] = (int32_t)n_live;
        a.edge_off[B] = (int32_t)e_live;
        a.row_ptr[n_live] = (int32_t)e_live;
        int all = 0;
        for (int w = 0; w < nwaves; ++w) all |= bits_s[w];
        if (all) atomicOr(a.status, (int32_t)all);           // (the caller's word, shared with its other calls)
    }
}

template <int kVec> struct PosLane;
template <> struct PosLane<4> { typedef u32x4 type; };
template <> struct PosLane<2> { typedef u32x2 type; };

template <int kVec>     // floats per lane of the positional rows: 4 (P % 4 == 0) or 2
__global__ __launch_bounds__(kCopyThreads) void pack_copy_kernel(PackDev a)
{
    typedef typename PosLane<kVec>::type V;
    __shared__ int32_t noff_s[kMaxB + 1], eoff_s[kMaxB + 1];
    __shared__ int32_t srow_s[kRowTile];
    const int tid = (int)threadIdx.x, B = a.B;
    const int n = a.node_off[B], e = a.edge_off[B];
    const int row_tiles = (n + kRowTile - 1) / kRowTile;
    const int tiles = row_tiles + (e + kEntTile - 1) / kEntTile;
    if ((int)blockIdx.x >= tiles) return;
    for (int i = tid; i <= B; i += kCopyThreads) { noff_s[i] = a.node_off[i]; eoff_s[i] = a.edge_off[i]; }
    __syncthreads();
    const int32_t *__restrict__ ci = a.ci;
    int32_t *__restrict__ col_out = a.col_idx;
    for (int t = (int)blockIdx.x; t < tiles; t += (int)gridDim.x) {
        if (t < row_tiles) {
            const int r0 = t * kRowTile, rows = min(kRowTile, n - r0);
            if (tid < rows) {
                const int r = r0 + tid;
                const int b = find_slot(noff_s, 0, B, r);
                const int f0 = a.node_first[a.idx[b]];
                const int src = f0 + (r - noff_s[b]);
                a.graph_id[r] = b;
                a.row_ptr[r] = eoff_s[b] + (a.rp[src] - a.rp[f0]) * a.expand;
                srow_s[tid] = src;
            }
            if (a.pos_out) {
                __syncthreads();
                const int lanes_per_row = a.P / kVec, total = rows * lanes_per_row;
                const V *__restrict__ from = reinterpret_cast<const V *>(a.pos);
                V *__restrict__ to = reinterpret_cast<V *>(a.pos_out) + (long long)r0 * lanes_per_row;   // one linear run
                for (int i0 = tid; i0 < total; i0 += kUnroll * kCopyThreads) {
                    V v[kUnroll];
#pragma unroll
                    for (int u = 0; u < kUnroll; ++u) {      // (the lanes past the end re-read the last one: no branch around a load)
                        const int i = min(i0 + u * kCopyThreads, total - 1);
                        const int row = i / lanes_per_row;
                        v[u] = from[(long long)srow_s[row] * lanes_per_row + (i - row * lanes_per_row)];
                    }
#pragma unroll
                    for (int u = 0; u < kUnroll; ++u) {
                        const int i = i0 + u * kCopyThreads;
                        if (i < total) to[i] = v[u];
                    }
                }
                __syncthreads();                             // (srow_s is the next row tile's)
            }
        } else {
            const int x0 = (t - row_tiles) * kEntTile, x1 = min(x0 + kEntTile, e);
            const int b0 = find_slot(eoff_s, 0, B, x0), b1 = find_slot(eoff_s, 0, B, x1 - 1);
            int b = -1, next = 0, first = 0, src0 = 0, base = 0;       // the graph of the previous entry of this thread
            for (int p = x0 + tid; p < x1; p += kCopyThreads) {
                if (b < 0 || p >= next) {
                    b = find_slot(eoff_s, b0, b1 + 1, p);
                    next = eoff_s[b + 1];
                    first = eoff_s[b];
                    src0 = a.rp[a.node_first[a.idx[b]]];
                    base = noff_s[b];
                }
                const int q = p - first;
                col_out[p] = ci[src0 + (a.expand == 1 ? q : q / a.expand)] + base;
            }
        }
    }
}

}  // namespace

extern "C" {

int32_t gcc_pack_graphs(const gcc_graph_corpus *c, const int32_t *idx, int32_t B, const gcc_batch_out *out, float *pos_out,
                        int32_t *seed_local_out, int32_t *labels_out, int32_t expand, int32_t *status, void *stream)
{
    if (!c || !idx || !out || !seed_local_out || !status || !c->node_first || !c->row_ptr || !c->col_idx || !c->seed_local ||
        !out->node_off || !out->edge_off || !out->graph_id || !out->row_ptr || (!out->col_idx && out->edge_cap > 0)) {
        snprintf(g_err, kErrLen, "gcc_pack_graphs: NULL argument");
        return -1;
    }
    if (B < 1 || B > kMaxB) {
        snprintf(g_err, kErrLen, "gcc_pack_graphs: batch size %d outside 1..GCC_PACK_GRAPHS_MAX_BATCH (%d)", B, kMaxB);
        return -2;
    }
    if (expand < 1) {
        snprintf(g_err, kErrLen, "gcc_pack_graphs: expand %d must be at least 1", expand);
        return -3;
    }
    if (c->num_graphs < 0 || out->node_cap < 0 || out->edge_cap < 0 || out->node_cap >= INT32_MAX || out->edge_cap > INT32_MAX) {
        snprintf(g_err, kErrLen, "gcc_pack_graphs: num_graphs %d / node_cap %lld / edge_cap %lld outside the int32 range",
                 c->num_graphs, (long long)out->node_cap, (long long)out->edge_cap);
        return -4;
    }
    const bool with_pos = pos_out && c->pos;
    if (with_pos && (c->pos_dim < 2 || (c->pos_dim & 1))) {
        snprintf(g_err, kErrLen, "gcc_pack_graphs: pos_dim %d must be even and at least 2", c->pos_dim);
        return -5;
    }
    const uintptr_t lane_bytes = with_pos && c->pos_dim % 4 == 0 ? 16 : 8;
    if (with_pos && (((uintptr_t)c->pos | (uintptr_t)pos_out) & (lane_bytes - 1))) {
        snprintf(g_err, kErrLen, "gcc_pack_graphs: pos / pos_out must be aligned to %d bytes", (int)lane_bytes);
        return -6;
    }
    PackDev a = {};
    a.node_first = c->node_first; a.rp = c->row_ptr; a.ci = c->col_idx; a.seed = c->seed_local; a.labels = c->labels;
    a.pos = with_pos ? c->pos : nullptr;
    a.idx = idx;
    a.G = c->num_graphs; a.P = c->pos_dim; a.B = B; a.expand = expand;
    a.node_off = out->node_off; a.edge_off = out->edge_off; a.graph_id = out->graph_id; a.row_ptr = out->row_ptr;
    a.col_idx = out->col_idx;
    a.node_cap = out->node_cap; a.edge_cap = out->edge_cap;
    a.pos_out = with_pos ? pos_out : nullptr;
    a.seed_out = seed_local_out; a.labels_out = labels_out; a.status = status;
    hipLaunchKernelGGL(pack_prefix_kernel, dim3(1), dim3((B + 63) / 64 * 64), 0, (hipStream_t)stream, a);
    const long long cap_tiles = (out->node_cap + kRowTile - 1) / kRowTile + (out->edge_cap + kEntTile - 1) / kEntTile;
    const int grid = (int)(cap_tiles < 1 ? 1 : (cap_tiles > kMaxGrid ? kMaxGrid : cap_tiles));
    if (with_pos && c->pos_dim % 4 == 0)
        hipLaunchKernelGGL(pack_copy_kernel<4>, dim3(grid), dim3(kCopyThreads), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(pack_copy_kernel<2>, dim3(grid), dim3(kCopyThreads), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

}  // extern "C"
