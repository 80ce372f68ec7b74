// gcc_amd/csrc/gin_wide.hip -- wide (hidden 256) GIN layers in bf16 on the matrix cores, one subgraph per
// workgroup, resident in LDS across all layers: BASELINE.json configs[4] ("GIN hid=256 layers=8 deg=32 bf16,
// SpMM+MFMA-MLP roofline run on batched subgraphs").  Reference: UnsupervisedGIN.forward gcc/models/gin.py:213-221
// with the modules of gin.py:42-58,107-116 in eval mode (generate.py:71); see include/gcc_amd.h.
//
// A subgraph has at most 128 nodes, so its adjacency (plus the identity: GINConv adds h_v itself, eps = 0) is a
// dense 128x128 block and all three products of a layer run on v_mfma_f32_16x16x32_bf16 with every operand read
// k-contiguous and every result stored 16 bytes at a time:
//     AGG [node][ch]  = sum_u  H^T[ch][u]  * ADJ[node][u]      A = H^T rows (LDS),  B = ADJ rows (64 registers, kept for all layers)
//     Z1  [node][ch]  = sum_k  W0[ch][k]   * AGG[node][k]      A = W0 rows (L2),    B = AGG rows (LDS)      + scale/shift/ReLU
//     H'^T[ch][node]  = sum_k  Z1[node][k] * W1[ch][k]         A = Z1 rows (LDS),   B = W1 rows (L2)        + 2x scale/shift/ReLU
// (D[row][col] = sum_k A[row][k] B[col][k]; a lane ends with 4 consecutive ROWS of one column, so the operand
// order of each product is chosen to make those values contiguous in the layout the next product reads.)
// The two LDS regions swap roles: H^T -> AGG in the other -> Z1 over H^T -> H'^T over AGG.
//
// Kernel shape: 256 threads = ONE wave per SIMD with up to 512 registers each, so that a wave's register tile is
// 64 channels x 128 nodes (Linear products) or 128 channels x 64 nodes (aggregation): every operand fragment read from
// LDS feeds FOUR matrix instructions, the weight fragments stream through a 4-deep register ring straight from L2 (each
// read once per workgroup, requested four k-steps = ~2000 cycles ahead across product boundaries), the adjacency is 16
// fragments in registers for all layers, and results are stored 16 bytes per lane: the rows of two adjacent A fragments
// are interleaved (row r of fragment e <-> index 2 r + e of a 32-block), so a lane's 4 + 4 accumulator rows are 8
// consecutive channels (or nodes).  Row strides per layout, from the LDS lane-group model of MI355X_MICROARCH.md (a
// 16-byte fragment read is serviced in 4 groups of 16 lanes): consecutive rows are conflict-free at 544 bytes,
// interleaved rows at 272 / 528 (blocks of four rows, the first try, are 2-way conflicted at every stride: 53 % of the
// LDS cycles in profiles/r3_pmc_gin_wide.json's first run).
//
// The stages of a layer are written once, as the inline functions below; two kernels call them: gin_wide2_kernel (a
// subgraph of at most 128 nodes, all layers in one launch) and gin_wide_big_kernel (a 128-row block of a larger one,
// one layer per launch).  gcc_ginw_embed puts them between a feature kernel and a readout kernel: the eval-mode embedding
// of a wide GIN encoder (GraphEncoder.resident_eval), one call per batch.
#include "host_common.h"

#include <mutex>

namespace {

constexpr int kD = GCC_GINW_HIDDEN;
constexpr int kNodes = GCC_GINW_MAX_NODES;
constexpr int kT = 256;
constexpr int kStrT = kNodes * 2 + 16;       // H^T, channel-major [256 ch][128 nodes]: read with interleaved rows (aggregation)
constexpr int kStrN = kD * 2 + 32;           // AGG, node-major [128 nodes][256 ch]: read with consecutive rows (first Linear)
constexpr int kStrZ = kD * 2 + 16;           // Z1,  node-major: read with interleaved rows (second Linear)
constexpr int kReg = kD * kStrT;             // 69,632 B = kNodes * kStrN
constexpr int kLds = 2 * kReg + (kNodes + 1 + 3) / 4 * 16;
static_assert(kNodes * kStrN <= kReg && kNodes * kStrZ <= kReg, "the node-major layouts must fit a region");
static_assert(kD == 256 && kNodes == 128, "the wave tilings below are written for 256 channels x 128 nodes");

struct WideArgs {
    const int32_t *node_off, *row_ptr, *col_idx;
    const uint16_t *x_in;
    uint16_t *x_out;
    float *pooled;
    int32_t *status;
    int32_t batch_size, num_layers;
    long long *ticks;                // diagnostics (gcc_ginw_debug_ticks): wall-clock ticks per phase, or NULL
    gcc_ginw_layer layers[GCC_GIN_MAX_LAYERS];
    // subgraphs over kNodes nodes (gin_wide_big_kernel): two [N, 256] bf16 ping-pong buffers and a work list
    // {count, -, (subgraph, row block) pairs}, or NULL: such subgraphs are refused (GCC_STATUS_GINW_TOO_LARGE)
    uint16_t *big0, *big1;
    int32_t *big_work;
    int32_t big_cap;                 // pairs the work list holds
    int32_t mult;                    // copies of every CSR entry in the graph the model saw (gcc_ginw_forward: 1; gcc_ginw_embed: edge_multiplicity)
};

long long *g_ticks = nullptr;

__device__ __forceinline__ void phase_tick(long long *row, int ph, long long &tick)
{
    if (row && threadIdx.x == 0) {
        const long long now = device_ticks();
        atomicAdd((unsigned long long *)&row[ph], (unsigned long long)(now - tick));
        tick = now;
    }
}

__device__ __forceinline__ u32x4 lds16(const unsigned char *p) { return *(const u32x4 *)p; }

__device__ __forceinline__ int perm8(int lr, int e) { return 2 * lr + e; }
__device__ __forceinline__ u32x4 pack8_bf16(const f32x4 &a, const f32x4 &b)
{
    u32x4 r;
    r[0] = pack2_bf16(a[0], b[0]);               // fragment 0 holds the even, fragment 1 the odd indices
    r[1] = pack2_bf16(a[1], b[1]);
    r[2] = pack2_bf16(a[2], b[2]);
    r[3] = pack2_bf16(a[3], b[3]);
    return r;
}
__device__ __forceinline__ float sum8_bf16(u32x4 v, float s = 0.f)
{
#pragma unroll
    for (int q = 0; q < 4; ++q) s = add2_bf16(v[q], s);
    return s;
}
// the 4 weight fragments of one k-step of a wave's 64 output channels.  kRowPerm: the fragments are A operands whose rows
// are interleaved in pairs (first Linear); else B operands, column lr = channel 16 m + lr (second Linear)
// kFrag: wmat is the fragment-major copy made by gcc_ginw_pack_weights (1 KiB contiguous per request)
template <bool kRowPerm, bool kFrag>
__device__ __forceinline__ void request_w(u32x4 (&dst)[4], const uint16_t *wmat, int w, int ks, int lr, int lg)
{
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        if (kFrag) {
            dst[m] = *(const u32x4 *)(wmat + (int64_t)((w * 4 + m) * 8 + ks) * 512 + (lg * 16 + lr) * 8);
        } else {
            const int ch = w * 64 + (kRowPerm ? (m >> 1) * 32 + perm8(lr, m & 1) : m * 16 + lr);
            dst[m] = *(const u32x4 *)(wmat + (int64_t)ch * kD + ks * 32 + lg * 8);
        }
    }
}

__global__ void ginw_pack_kernel(const uint16_t *w, uint16_t *wf, int which)
{
    const int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);      // one 16-byte piece: ((w * 4 + m) * 8 + ks) * 64 + lane
    if (idx >= kD * kD / 8) return;
    const int lane = idx & 63, ks = (idx >> 6) & 7, m = (idx >> 9) & 3, wb = idx >> 11, lr = lane & 15, lg = lane >> 4;
    const int row = wb * 64 + (which == 0 ? (m >> 1) * 32 + perm8(lr, m & 1) : m * 16 + lr);
    *(u32x4 *)(wf + (int64_t)idx * 8) = *(const u32x4 *)(w + (int64_t)row * kD + ks * 32 + lg * 8);
}

// =====================================================================================================================
// The stages of a layer, shared by the two kernels.  A "block" is what one workgroup holds in LDS: a whole subgraph
// (gin_wide2_kernel) or 128 rows / 128 columns of a larger one (gin_wide_big_kernel).  None of them has a barrier inside.

// nrows rows of `rows`, from global row row0 on -> P, channel-major; rows >= nrows of the block as zeros
// (4 nodes x 8 channels per work item: four 16-byte loads, eight 8-byte LDS writes; requesting all 16 loads of a
//  thread's four work items first was measured too: no gain)
__device__ __forceinline__ void load_rows_transposed(unsigned char *P, const uint16_t *rows, int row0, int nrows, int tid)
{
    for (int idx = tid; idx < (kNodes / 4) * (kD / 8); idx += kT) {
        const int chunk = idx & (kD / 8 - 1), node = 4 * (idx >> 5);
        u32x4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const u32x4 z = {0u, 0u, 0u, 0u};
            v[j] = node + j < nrows ? *(const u32x4 *)(rows + (int64_t)(row0 + node + j) * kD + chunk * 8) : z;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int sh = (e & 1) * 16;
            u32x2 o;
            o[0] = ((v[0][e >> 1] >> sh) & 0xFFFFu) | (((v[1][e >> 1] >> sh) & 0xFFFFu) << 16);
            o[1] = ((v[2][e >> 1] >> sh) & 0xFFFFu) | (((v[3][e >> 1] >> sh) & 0xFFFFu) << 16);
            *(u32x2 *)(P + (chunk * 8 + e) * kStrT + node * 2) = o;
        }
    }
}

// the block's rows (channel-major in P) back to node-major global memory, from global row row0 on
__device__ __forceinline__ void store_rows_transposed(const unsigned char *P, uint16_t *rows, int row0, int nrows, int tid)
{
    for (int idx = tid; idx < (kNodes / 4) * (kD / 8); idx += kT) {
        const int chunk = idx & (kD / 8 - 1), node = 4 * (idx >> 5);
        if (node < nrows) {
            u32x2 c[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) c[e] = *(const u32x2 *)(P + (chunk * 8 + e) * kStrT + node * 2);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (node + j < nrows) {
                    const int sh = (j & 1) * 16, h = j >> 1;
                    u32x4 v;
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        v[q] = ((c[2 * q][h] >> sh) & 0xFFFFu) | (((c[2 * q + 1][h] >> sh) & 0xFFFFu) << 16);
                    *(u32x4 *)(rows + (int64_t)(row0 + node + j) * kD + chunk * 8) = v;
                }
            }
        }
    }
}

// Neighbour counts of the block's nrows rows (row pointers staged in rp) towards the 128 columns of column block cblk of
// their subgraph (first node n0, n nodes) -> Q (zeroed by the caller; 16-bit counters, [row][column]).  Runs of 16
// consecutive edges per thread: one bisection of the row pointers per run, then the row advances with the edges (a
// bisection per edge was 9.8 us per subgraph).  A neighbour outside the subgraph is skipped in every column block and
// flagged in the first; one inside it but outside this column block belongs to another pass.  self_loop: + h_v itself
// (the column block that holds the rows' own nodes); it counts once, a CSR entry `mult` times (the edge multiplicity of the
// multigraph the CSR stands for).  A counter is 16 bits wide: a row with 65,536 / mult or more copies of ONE neighbour is
// outside the contract (it would carry into the next counter, or out of the word, unseen); what exceeds 256 below that
// is caught by flag_count_overflow.
__device__ __forceinline__ void count_neighbours(unsigned char *Q, const int32_t *rp, const int32_t *col_idx, int32_t *status, int n0,
                                                 int n, int nrows, int cblk, bool self_loop, uint32_t mult, int tid)
{
    const int e0 = rp[0], e1 = rp[nrows];
    for (int eb = e0 + 16 * tid; eb < e1; eb += 16 * kT) {
        int cols[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) cols[j] = eb + j < e1 ? col_idx[eb + j] : -1;
        int lo = 0, hi = nrows;                      // largest i with rp[i] <= eb
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (rp[mid] <= eb) lo = mid; else hi = mid;
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (eb + j >= e1) break;
            while (rp[lo + 1] <= eb + j) ++lo;       // (empty rows are skipped)
            const int ug = cols[j] - n0, u = ug - cblk * kNodes;
            if ((unsigned)ug >= (unsigned)n) { if (cblk == 0) atomicOr(status, (int32_t)GCC_STATUS_GINW_BAD_EDGE); }
            else if ((unsigned)u < (unsigned)kNodes) atomicAdd((uint32_t *)(Q + lo * kStrT + (u >> 1) * 4), (u & 1) ? mult << 16 : mult);
        }
    }
    if (self_loop && tid < nrows) atomicAdd((uint32_t *)(Q + tid * kStrT + (tid >> 1) * 4), (tid & 1) ? 0x10000u : 1u);
}

// channel tid's sum over the block's rows in P: hidden_rep[0] = the input (gin.py:216)
__device__ __forceinline__ float input_channel_sum(const unsigned char *P, int tid, float s)
{
    for (int j = 0; j < kNodes / 8; ++j) s += sum8_bf16(lds16(P + tid * kStrT + j * 16));
    return s;
}

// A count above kMaxCount has no exact bf16 value: it is reported (GCC_STATUS_GINW_COUNT_OVERFLOW), never left to round.
// A pass of its own over the finished counters (the padding bytes of a row are zeros), nine 16-byte reads per thread: in
// adjacency_fragments the test cost the block kernel 31 more spilled registers.
constexpr uint32_t kMaxCount = 256;          // integers up to 2^8 are exact in bf16 (8 significant bits)
__device__ __forceinline__ void flag_count_overflow(const unsigned char *Q, int32_t *status, int tid)
{
    uint32_t over = 0;
    for (int i = tid; i < kNodes * kStrT / 16; i += kT) {
        const u32x4 c = lds16(Q + i * 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) over |= (uint32_t)((c[q] & 0xFFFFu) > kMaxCount) | (uint32_t)((c[q] >> 16) > kMaxCount);
    }
    if (over) atomicOr(status, (int32_t)GCC_STATUS_GINW_COUNT_OVERFLOW);
}

// this wave's share of ADJ (its node half nh: 64 nodes x the block's 128 columns) as bf16 B fragments, from the counters in Q
__device__ __forceinline__ void adjacency_fragments(u32x4 (&adj)[4][4], const unsigned char *Q, int nh, int lr, int lg)
{
#pragma unroll
    for (int nf = 0; nf < 4; ++nf)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const u32x4 c = lds16(Q + (nh * 64 + nf * 16 + lr) * kStrT + (ks * 32 + lg * 8) * 2);
            u32x4 f;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                f[q] = pack2_bf16((float)(c[q] & 0xFFFFu), (float)(c[q] >> 16));
            adj[nf][ks] = f;
        }
}

// acc[ch][node] += sum_u H^T[ch][u] ADJ[node][u] over the block's 128 columns: 128 channels (half chh) x 64 nodes per wave
// (no branches on the block's size in here -- data-dependent branches around blocks of matrix instructions make the
// register allocator spill hundreds of values; rows and columns of padding nodes are zeros anyway)
__device__ __forceinline__ void aggregate(f32x4 (&acc)[8][4], const u32x4 (&adj)[4][4], const unsigned char *P, int chh, int lr, int lg)
{
    const unsigned char *src = P + (chh * 128) * kStrT + lg * 16;
    u32x4 buf[2][8];
#pragma unroll
    for (int m = 0; m < 8; ++m) buf[0][m] = lds16(src + ((m >> 1) * 32 + perm8(lr, m & 1)) * kStrT);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        if (ks + 1 < 4) {
#pragma unroll
            for (int m = 0; m < 8; ++m)
                buf[(ks + 1) & 1][m] = lds16(src + ((m >> 1) * 32 + perm8(lr, m & 1)) * kStrT + (ks + 1) * 64);
        }
        SCHED_FENCE();
#pragma unroll
        for (int m = 0; m < 8; ++m)
#pragma unroll
            for (int nf = 0; nf < 4; ++nf) acc[m][nf] = mfma_16x16x32_bf16(buf[ks & 1][m], adj[nf][ks], acc[m][nf]);
        SCHED_FENCE();
    }
}

// AGG[node][ch] -> Q (node-major), rounded to bf16 here and nowhere else
__device__ __forceinline__ void store_agg(unsigned char *Q, const f32x4 (&acc)[8][4], int nh, int chh, int lr, int lg)
{
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int nf = 0; nf < 4; ++nf)
            *(u32x4 *)(Q + (nh * 64 + nf * 16 + lr) * kStrN + (chh * 128 + p * 32 + lg * 8) * 2) =
                pack8_bf16(acc[2 * p][nf], acc[2 * p + 1][nf]);
}

// Z1[node][ch] = relu(s0 * (AGG W0^T) + t0): AGG in Q -> Z1 in P (both node-major); channels 64 w .. 64 w + 63, all nodes.
// The weight ring wr holds k-steps 0..3 of w0 on entry and k-steps 0..3 of w1 on exit.
template <bool kFrag>
__device__ __forceinline__ void linear0(const unsigned char *Q, unsigned char *P, u32x4 (&wr)[4][4], const gcc_ginw_layer &ly, int w,
                                        int lr, int lg)
{
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc[4][8];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int nf = 0; nf < 8; ++nf) acc[m][nf] = zero4;
    float4 sc[2][2], sh[2][2];                   // scale / shift of the lane's 8 channels per fragment pair
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            sc[p][e] = *(const float4 *)(ly.s0 + w * 64 + p * 32 + lg * 8 + e * 4);
            sh[p][e] = *(const float4 *)(ly.t0 + w * 64 + p * 32 + lg * 8 + e * 4);
        }
    const unsigned char *src = Q + lr * kStrN + lg * 16;
    u32x4 buf[2][8];
#pragma unroll
    for (int nf = 0; nf < 8; ++nf) buf[0][nf] = lds16(src + nf * 16 * kStrN);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
        if (ks + 1 < 8) {
#pragma unroll
            for (int nf = 0; nf < 8; ++nf) buf[(ks + 1) & 1][nf] = lds16(src + nf * 16 * kStrN + (ks + 1) * 64);
        }
        SCHED_FENCE();
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int nf = 0; nf < 8; ++nf) acc[m][nf] = mfma_16x16x32_bf16(wr[ks & 3][m], buf[ks & 1][nf], acc[m][nf]);
        SCHED_FENCE();
        if (ks < 4) request_w<true, kFrag>(wr[ks & 3], kFrag ? ly.w0_frag : ly.w0, w, ks + 4, lr, lg);
        else request_w<false, kFrag>(wr[ks & 3], kFrag ? ly.w1_frag : ly.w1, w, ks - 4, lr, lg);
        SCHED_FENCE();
    }
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int nf = 0; nf < 8; ++nf) {
            f32x4 lo = acc[2 * p][nf], hi = acc[2 * p + 1][nf];     // channels 8 lg + {0, 2, 4, 6} and + {1, 3, 5, 7}
            lo[0] = fmaxf(fmaf(lo[0], sc[p][0].x, sh[p][0].x), 0.f); hi[0] = fmaxf(fmaf(hi[0], sc[p][0].y, sh[p][0].y), 0.f);
            lo[1] = fmaxf(fmaf(lo[1], sc[p][0].z, sh[p][0].z), 0.f); hi[1] = fmaxf(fmaf(hi[1], sc[p][0].w, sh[p][0].w), 0.f);
            lo[2] = fmaxf(fmaf(lo[2], sc[p][1].x, sh[p][1].x), 0.f); hi[2] = fmaxf(fmaf(hi[2], sc[p][1].y, sh[p][1].y), 0.f);
            lo[3] = fmaxf(fmaf(lo[3], sc[p][1].z, sh[p][1].z), 0.f); hi[3] = fmaxf(fmaf(hi[3], sc[p][1].w, sh[p][1].w), 0.f);
            *(u32x4 *)(P + (nf * 16 + lr) * kStrZ + (w * 64 + p * 32 + lg * 8) * 2) = pack8_bf16(lo, hi);
        }
}

// H'^T[ch][node] = relu(s2 * relu(s1 * (Z1 W1^T) + t1) + t2): Z1 in P (node-major) -> H'^T in Q (channel-major), rows
// >= nrows of the block as 0 (the aggregation multiplies them by ADJ's zeros, which only works for finite values);
// SumPooling of the block's rows into pool[channel] (or NULL): stored, or with pool_atomic added (the row blocks of a big
// subgraph add up in arrival order: fp32 atomics on a row the fused kernel zeroed).  The weight ring holds k-steps 0..3 of
// w1 on entry; with request_next it holds k-steps 0..3 of wnext, the next layer's w0, on exit.
template <bool kFrag>
__device__ __forceinline__ void linear1(const unsigned char *P, unsigned char *Q, u32x4 (&wr)[4][4], const gcc_ginw_layer &ly,
                                        const uint16_t *wnext, bool request_next, float *pool, bool pool_atomic, int nrows, int w, int lr,
                                        int lg)
{
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc[8][4];
#pragma unroll
    for (int nf = 0; nf < 8; ++nf)
#pragma unroll
        for (int m = 0; m < 4; ++m) acc[nf][m] = zero4;
    // relu(s2 * relu(s1 * x + t1) + t2) as ONE multiply-add and ONE clamp per value: with A = s1 s2 and
    // B = s2 t1 + t2 it is max(A x + B, max(t2, 0)) for s2 >= 0 and min(max(A x + B, 0), max(t2, 0)) for s2 < 0
    float ea[4], eb[4], elo[4], ehi[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int c = w * 64 + m * 16 + lr;
        const float s1 = ly.s1[c], t1 = ly.t1[c], s2 = ly.s2[c], t2 = ly.t2[c];
        ea[m] = s1 * s2;
        eb[m] = fmaf(s2, t1, t2);
        elo[m] = s2 >= 0.f ? fmaxf(t2, 0.f) : 0.f;
        ehi[m] = s2 >= 0.f ? __uint_as_float(0x7F800000u) : fmaxf(t2, 0.f);
    }
    const unsigned char *src = P + lg * 16;
    u32x4 buf[2][8];
#pragma unroll
    for (int nf = 0; nf < 8; ++nf) buf[0][nf] = lds16(src + ((nf >> 1) * 32 + perm8(lr, nf & 1)) * kStrZ);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
        if (ks + 1 < 8) {
#pragma unroll
            for (int nf = 0; nf < 8; ++nf)
                buf[(ks + 1) & 1][nf] = lds16(src + ((nf >> 1) * 32 + perm8(lr, nf & 1)) * kStrZ + (ks + 1) * 64);
        }
        SCHED_FENCE();
#pragma unroll
        for (int nf = 0; nf < 8; ++nf)
#pragma unroll
            for (int m = 0; m < 4; ++m) acc[nf][m] = mfma_16x16x32_bf16(buf[ks & 1][nf], wr[ks & 3][m], acc[nf][m]);
        SCHED_FENCE();
        if (ks < 4) request_w<false, kFrag>(wr[ks & 3], kFrag ? ly.w1_frag : ly.w1, w, ks + 4, lr, lg);
        else if (request_next) request_w<true, kFrag>(wr[ks & 3], wnext, w, ks - 4, lr, lg);
        SCHED_FENCE();
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int c = w * 64 + m * 16 + lr;
        float psum = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int node = q * 32 + lg * 8;
            f32x4 lo = acc[2 * q][m], hi = acc[2 * q + 1][m];
#pragma unroll
            for (int r = 0; r < 4; ++r) {        // apply_func: relu(bn(mlp)), then relu(batch_norms[i](.))
                lo[r] = clamp_f32(fmaf(lo[r], ea[m], eb[m]), elo[m], ehi[m]);
                hi[r] = clamp_f32(fmaf(hi[r], ea[m], eb[m]), elo[m], ehi[m]);
            }
            if (q * 32 + 32 > nrows) {           // (block-uniform) this 32-block holds padding nodes: they stay 0
#pragma unroll
                for (int r = 0; r < 4; ++r) {        // (lo: nodes node + 0, 2, 4, 6; hi: + 1, 3, 5, 7)
                    lo[r] = node + 2 * r < nrows ? lo[r] : 0.f;
                    hi[r] = node + 2 * r + 1 < nrows ? hi[r] : 0.f;
                }
            }
            const u32x4 hv = pack8_bf16(lo, hi);
            psum = sum8_bf16(hv, psum);
            *(u32x4 *)(Q + c * kStrT + node * 2) = hv;
        }
        psum += wave_shfl_xor(psum, 16);
        psum += wave_shfl_xor(psum, 32);
        if (lg == 0 && pool) {
            if (pool_atomic) atomicAdd(&pool[c], psum);
            else pool[c] = psum;
        }
    }
}

// =====================================================================================================================
// Subgraphs of at most kNodes nodes: one per workgroup at a time, every layer in this launch
// (the "2" of the name: the second shape tried, and the name the records under profiles/ know it by)
template <bool kFrag>
__global__ __launch_bounds__(kT) void gin_wide2_kernel(WideArgs a)
{
    DYN_SMEM(smem);
    unsigned char *P = smem, *Q = smem + kReg;
    int32_t *rp = (int32_t *)(smem + 2 * kReg);              // [129] row pointers of the subgraph
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int lr = lane & 15, lg = lane >> 4;
    const int L = a.num_layers;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const int nh = w & 1, chh = w >> 1;                      // aggregation: node half x channel half

    for (int b = blockIdx.x; b < a.batch_size; b += gridDim.x) {
        __syncthreads();                                     // the previous subgraph's output pass is done with P
        long long tick = a.ticks ? device_ticks() : 0;
        const int n0 = a.node_off[b], n = a.node_off[b + 1] - n0;
        if (n <= 0 || n > kNodes) {                          // (uniform over the workgroup)
            if (n > kNodes && !a.big_work) {                 // (with scratch: gin_wide_big_kernel takes it, block by block)
                if (tid == 0) atomicOr(a.status, (int32_t)GCC_STATUS_GINW_TOO_LARGE);
                if (a.x_out)
                    for (int64_t i = tid; i < (int64_t)n * (kD / 2); i += kT) ((uint32_t *)(a.x_out + (int64_t)n0 * kD))[i] = 0u;
            }
            if (a.pooled)
                for (int i = tid; i < (L + 1) * kD; i += kT) a.pooled[(int64_t)b * (L + 1) * kD + i] = 0.f;
            continue;
        }
        // ---- the subgraph's input rows -> P, channel-major; neighbour counts -> Q (16-bit counters, [node][u])
        for (int i = tid; i < kNodes * kStrT / 4; i += kT) ((uint32_t *)Q)[i] = 0u;
        if (tid <= n) rp[tid] = a.row_ptr[n0 + tid];
        load_rows_transposed(P, a.x_in, n0, n, tid);
        __syncthreads();
        phase_tick(a.ticks, 0, tick);                        // rows in
        count_neighbours(Q, rp, a.col_idx, a.status, n0, n, n, 0, true, (uint32_t)a.mult, tid);
        __syncthreads();
        phase_tick(a.ticks, 1, tick);                        // neighbour counts
        flag_count_overflow(Q, a.status, tid);
        if (a.pooled) a.pooled[((int64_t)b * (L + 1)) * kD + tid] = input_channel_sum(P, tid, 0.f);
        u32x4 adj[4][4];                                     // kept in registers for every layer
        adjacency_fragments(adj, Q, nh, lr, lg);
        u32x4 wr[4][4];                                      // weight ring: slot = k-step & 3
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) request_w<true, kFrag>(wr[ks], kFrag ? a.layers[0].w0_frag : a.layers[0].w0, w, ks, lr, lg);
        lds_barrier();                                       // (not __syncthreads(): the requests stay in flight)
        phase_tick(a.ticks, 2, tick);                        // input pooling, adjacency fragments

        for (int layer = 0; layer < L; ++layer) {
            const gcc_ginw_layer ly = a.layers[layer];
            {
                f32x4 acc[8][4];
#pragma unroll
                for (int m = 0; m < 8; ++m)
#pragma unroll
                    for (int nf = 0; nf < 4; ++nf) acc[m][nf] = zero4;
                aggregate(acc, adj, P, chh, lr, lg);
                store_agg(Q, acc, nh, chh, lr, lg);
            }
            lds_barrier();
            phase_tick(a.ticks, 3, tick);                    // aggregation
            linear0<kFrag>(Q, P, wr, ly, w, lr, lg);
            lds_barrier();
            phase_tick(a.ticks, 4, tick);                    // first Linear
            {
                // (after the last layer the requests are dummies: no branch around them)
                const gcc_ginw_layer &lnext = a.layers[layer + 1 < L ? layer + 1 : layer];
                float *pool = a.pooled ? a.pooled + ((int64_t)b * (L + 1) + layer + 1) * kD : nullptr;
                linear1<kFrag>(P, Q, wr, ly, kFrag ? lnext.w0_frag : lnext.w0, true, pool, false, n, w, lr, lg);
            }
            lds_barrier();
            phase_tick(a.ticks, 5, tick);                    // second Linear
            unsigned char *t = P; P = Q; Q = t;
        }
        if (a.x_out) store_rows_transposed(P, a.x_out, n0, n, tid);
        phase_tick(a.ticks, 6, tick);                        // rows out
        if (a.ticks && tid == 0) atomicAdd((unsigned long long *)&a.ticks[15], 1ull);
    }
}

// =====================================================================================================================
// Subgraphs over kNodes nodes (ego-nets of the pre-training workload reach ~900 nodes: DESIGN.md section 6), one layer per
// launch, one (subgraph, block of 128 rows) per workgroup at a time.  The stages, LDS layouts and rounding points are the
// fused kernel's; what is this kernel's own is the aggregation's outer loop: the row block's adjacency is a [128 x n] strip,
// taken 128 columns at a time -- the column block's rows H_c^T come from global memory (the previous layer's output), the
// 16-bit neighbour counts of (row block, column block) are rebuilt, and the products ACCUMULATE into the same registers,
// so AGG is rounded to bf16 once, after the whole sum, exactly as for a small subgraph.  Rows travel through two global
// ping-pong buffers between the launches of consecutive layers (a layer needs every row block of the one before).
__global__ void ginw_classify_kernel(WideArgs a)
{
    __shared__ int32_t cnt;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    for (int b = threadIdx.x; b < a.batch_size; b += blockDim.x) {
        const int n = a.node_off[b + 1] - a.node_off[b];
        if (n <= kNodes) continue;
        const int nblk = (n + kNodes - 1) / kNodes;
        const int at = atomicAdd(&cnt, nblk);
        if (at + nblk > a.big_cap) {                         // no room: refused (status); the slots it reserved below the cap are
            atomicOr(a.status, (int32_t)GCC_STATUS_GINW_TOO_LARGE);      // marked so that the block kernel skips them instead of
            for (int r = 0; r < nblk && at + r < a.big_cap; ++r) a.big_work[2 + 2 * (at + r)] = -1;   // reading uninitialised pairs
            continue;
        }
        for (int r = 0; r < nblk; ++r) { a.big_work[2 + 2 * (at + r)] = b; a.big_work[3 + 2 * (at + r)] = r; }
    }
    __syncthreads();
    if (threadIdx.x == 0) a.big_work[0] = cnt < a.big_cap ? cnt : a.big_cap;
}

template <bool kFrag>
__global__ __launch_bounds__(kT) void gin_wide_big_kernel(WideArgs a, int layer, const uint16_t *hin, uint16_t *hout)
{
    DYN_SMEM(smem);
    unsigned char *P = smem, *Q = smem + kReg;
    int32_t *rp = (int32_t *)(smem + 2 * kReg);              // [129] row pointers of the row block
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int lr = lane & 15, lg = lane >> 4;
    const int L = a.num_layers;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const int nh = w & 1, chh = w >> 1;
    const gcc_ginw_layer ly = a.layers[layer];
    const int nitems = a.big_work[0];

    for (int it = blockIdx.x; it < nitems; it += gridDim.x) {
        const int b = a.big_work[2 + 2 * it], r = a.big_work[3 + 2 * it];
        if (b < 0) continue;                                 // (workgroup-uniform) a slot of a refused subgraph
        const int n0 = a.node_off[b], n = a.node_off[b + 1] - n0;
        const int nblk = (n + kNodes - 1) / kNodes;
        const int row0 = n0 + r * kNodes, nr = min(kNodes, n - r * kNodes);
        u32x4 wr[4][4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) request_w<true, kFrag>(wr[ks], kFrag ? ly.w0_frag : ly.w0, w, ks, lr, lg);
        f32x4 agg[8][4];
#pragma unroll
        for (int m = 0; m < 8; ++m)
#pragma unroll
            for (int nf = 0; nf < 4; ++nf) agg[m][nf] = zero4;
        float pool0 = 0.f;                                   // hidden_rep[0] of the subgraph (layer 0, row block 0: it sees every column block)
        for (int c = 0; c < nblk; ++c) {
            __syncthreads();                                 // the previous block's fragments / this item's predecessor are done with P, Q, rp
            const int col0 = n0 + c * kNodes, nc = min(kNodes, n - c * kNodes);
            for (int i = tid; i < kNodes * kStrT / 4; i += kT) ((uint32_t *)Q)[i] = 0u;
            if (tid <= nr) rp[tid] = a.row_ptr[row0 + tid];
            load_rows_transposed(P, hin, col0, nc, tid);     // H_c^T
            __syncthreads();
            count_neighbours(Q, rp, a.col_idx, a.status, n0, n, nr, c, c == r, (uint32_t)a.mult, tid);
            __syncthreads();
            if (layer == 0) flag_count_overflow(Q, a.status, tid);                               // (uniform; every layer sees the same counts)
            if (layer == 0 && r == 0 && a.pooled) pool0 = input_channel_sum(P, tid, pool0);      // (uniform)
            u32x4 adj[4][4];
            adjacency_fragments(adj, Q, nh, lr, lg);
            aggregate(agg, adj, P, chh, lr, lg);             // AGG += H_c^T ADJ(r, c)
        }
        if (layer == 0 && r == 0 && a.pooled) a.pooled[((int64_t)b * (L + 1)) * kD + tid] = pool0;
        __syncthreads();                                     // every wave is done with the last column block's P and Q
        store_agg(Q, agg, nh, chh, lr, lg);
        lds_barrier();
        linear0<kFrag>(Q, P, wr, ly, w, lr, lg);
        lds_barrier();
        float *pool = a.pooled ? a.pooled + ((int64_t)b * (L + 1) + layer + 1) * kD : nullptr;
        linear1<kFrag>(P, Q, wr, ly, nullptr, false, pool, true, nr, w, lr, lg);
        __syncthreads();
        store_rows_transposed(Q, hout, row0, nr, tid);
    }
}

// The caller's scratch, stated once: byte offsets of its regions and the total.  gcc_ginw_scratch_bytes returns `total`,
// gcc_ginw_forward checks the caller's size against it and binds WideArgs from the same object.
struct WideScratchLayout {
    int64_t rows[2];                 // [num_nodes][256] bf16 each: the ping-pong row buffers between the launches of two layers
    int64_t work;                    // int32 {count, -, cap x (subgraph, row block)}
    int64_t cap;                     // pairs the work list holds: every subgraph's row blocks, at most num_nodes / 128 + batch_size
    int64_t total;
};
WideScratchLayout wide_scratch_layout(int64_t num_nodes, int32_t batch_size)
{
    WideScratchLayout l;
    const int64_t rows = num_nodes * kD * 2;
    l.rows[0] = 0;
    l.rows[1] = rows;
    l.work = 2 * rows;
    l.cap = num_nodes / kNodes + batch_size;
    l.total = l.work + (2 + 2 * l.cap) * 4;
    return l;
}


// =====================================================================================================================
// The eval-mode embedding of a wide GIN encoder (gcc_ginw_embed): feature rows in, the layers above, the readout out.

// The feature rows of one view (graph_encoder.py:152-165): positional embedding | degree embedding | seed flag, as bf16 rows
// of kD channels; columns d_in.. are zero.  One subgraph per workgroup at a time, 8 channels (one 16-byte store) per work
// item; degree and seed flag as ginx_feat_kernel has them.  Rows from node_off[B] on are neither read nor written.
__global__ __launch_bounds__(kT) void ginw_feat_kernel(const int32_t *node_off, const int32_t *row_ptr, const int32_t *seed_local,
                                                       const float *pos, const float *emb, int B, int pos_dim, int de, int max_degree,
                                                       int mult, int node_cap, uint16_t *x)
{
    const int d_in = pos_dim + de + 1;
    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        const int n0 = max(node_off[b], 0), n1 = min(node_off[b + 1], node_cap);
        const int seed = node_off[b] + (seed_local ? seed_local[b] : 0);
        for (int i = (int)threadIdx.x; i < (n1 - n0) * (kD / 8); i += kT) {
            const int v = n0 + (i >> 5), c0 = (i & 31) * 8;
            int d = (row_ptr[v + 1] - row_ptr[v]) * mult;
            d = d < 0 ? 0 : (d > max_degree ? max_degree : d);
            float val[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int c = c0 + e;
                if (c < pos_dim) val[e] = pos[(int64_t)v * pos_dim + c];
                else if (c < pos_dim + de) val[e] = emb[(int64_t)d * de + (c - pos_dim)];
                else val[e] = (c == d_in - 1 && v == seed) ? 1.f : 0.f;
            }
            u32x4 o;
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] = pack2_bf16(val[2 * q], val[2 * q + 1]);
            *(u32x4 *)(x + (int64_t)v * kD + c0) = o;
        }
    }
}

// score[b] = sum_i (pred_w[i] pooled[b][i][:k_i] + pred_b[i]) per view (gin.py:226-230 in eval mode: dropout is the identity),
// normalised (graph_encoder.py:196), then the mean of the views (generate.py:52).  A workgroup of 16 waves takes kRoGraphs
// subgraphs, BOTH views at once, so that a prediction weight fetched from L2 feeds 2 x kRoGraphs accumulators.  A wave owns an
// output channel at a time: its lanes stride over (i, k) -- a hidden layer's row of up to 256 weights is ONE 16-byte load
// per lane when the rows are 16-byte aligned, so a channel's loads are all in flight together -- with one f32 accumulator
// per (view, subgraph), summed over the wave in a fixed order.  (The first shape, 4 waves x 64 channels each with scalar
// loads in a rolled loop, was a chain of ~2,000 L2 latencies per wave: 0.8 ms of a 1 ms call.)
constexpr int kRoGraphs = 2, kRoT = 1024;
struct ReadoutArgs {
    const float *pooled[2];
    const float *pred_w[GCC_GIN_MAX_LAYERS + 1], *pred_b[GCC_GIN_MAX_LAYERS + 1];
    float *out;
    int32_t B, L, d_in, hidden, out_dim, num_views, normalize;
    float norm_eps;
};
__global__ __launch_bounds__(kRoT) void ginw_readout_kernel(ReadoutArgs a)
{
    __shared__ __attribute__((aligned(16))) float P[2][kRoGraphs][(GCC_GIN_MAX_LAYERS + 1) * kD];   // 36 KiB: the pooled sums of this group
    __shared__ float S[2][kRoGraphs][kD];                                // scores per view
    __shared__ float R[2][kRoGraphs];                                    // max(||score||, eps), or 1
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int per = (a.L + 1) * kD;
    // (uniform) rows of the hidden layers' weights as 16-byte pieces: the row length and every base address allow it
    bool vec = (a.hidden & 3) == 0;
    for (int i = 1; i <= a.L; ++i) vec = vec && (((uintptr_t)a.pred_w[i]) & 15u) == 0;
    for (int g0 = (int)blockIdx.x * kRoGraphs; g0 < a.B; g0 += (int)gridDim.x * kRoGraphs) {
        __syncthreads();                                                 // the previous group is done with P, S and R
        for (int idx = tid; idx < 2 * kRoGraphs * per; idx += kRoT) {
            const int vg = idx / per, r = idx - vg * per, view = vg / kRoGraphs, g = vg - view * kRoGraphs;
            P[view][g][r] = (view < a.num_views && g0 + g < a.B) ? a.pooled[view][(int64_t)(g0 + g) * per + r] : 0.f;
        }
        __syncthreads();
        for (int o = w; o < a.out_dim; o += kRoT / 64) {                 // (wave-uniform)
            float acc[2][kRoGraphs], bias = 0.f;
#pragma unroll
            for (int v = 0; v < 2; ++v)
#pragma unroll
                for (int g = 0; g < kRoGraphs; ++g) acc[v][g] = 0.f;
            for (int i = 0; i <= a.L; ++i) {
                const int ki = i == 0 ? a.d_in : a.hidden;
                const float *wrow = a.pred_w[i] + (int64_t)o * ki;
                if (i > 0 && vec) {
                    for (int k = 4 * lane; k < ki; k += 256) {
                        const float4 wv = *(const float4 *)(wrow + k);
#pragma unroll
                        for (int v = 0; v < 2; ++v)
#pragma unroll
                            for (int g = 0; g < kRoGraphs; ++g) {
                                const float4 pv = *(const float4 *)&P[v][g][i * kD + k];
                                acc[v][g] = fmaf(wv.x, pv.x, fmaf(wv.y, pv.y, fmaf(wv.z, pv.z, fmaf(wv.w, pv.w, acc[v][g]))));
                            }
                    }
                } else {
#pragma unroll 4
                    for (int k = lane; k < ki; k += 64) {
                        const float wv = wrow[k];
#pragma unroll
                        for (int v = 0; v < 2; ++v)
#pragma unroll
                            for (int g = 0; g < kRoGraphs; ++g) acc[v][g] = fmaf(wv, P[v][g][i * kD + k], acc[v][g]);
                    }
                }
                bias += a.pred_b[i][o];
            }
#pragma unroll
            for (int v = 0; v < 2; ++v)
#pragma unroll
                for (int g = 0; g < kRoGraphs; ++g) {
                    const float t = wave_sum(acc[v][g]);
                    if (lane == 0) S[v][g][o] = t + bias;
                }
        }
        __syncthreads();
        for (int pr = w; pr < a.num_views * kRoGraphs; pr += kRoT / 64) {   // (wave-uniform) one wave per (view, subgraph)
            const int view = pr / kRoGraphs, g = pr - view * kRoGraphs;
            float ss = 0.f;
            for (int o = lane; o < a.out_dim; o += 64) ss = fmaf(S[view][g][o], S[view][g][o], ss);
            ss = wave_sum(ss);
            if (lane == 0) R[view][g] = a.normalize ? fmaxf(sqrtf(ss), a.norm_eps) : 1.f;
        }
        __syncthreads();
        for (int idx = tid; idx < kRoGraphs * a.out_dim; idx += kRoT) {
            const int g = idx / a.out_dim, o = idx - g * a.out_dim;
            if (g0 + g >= a.B) break;
            float f = S[0][g][o] / R[0][g];
            if (a.num_views == 2) f = (f + S[1][g][o] / R[1][g]) / 2;
            a.out[(int64_t)(g0 + g) * a.out_dim + o] = f;
        }
    }
}

// the layers of one batch from x_in: the fused launch for subgraphs of at most kNodes nodes, then -- with scratch -- the
// work list and one launch per layer for the larger ones (nothing to do, a few microseconds per launch, when there are none)
void launch_layers(const WideArgs &a, bool frag, const uint16_t *x_in, uint16_t *x_out, hipStream_t s)
{
#ifndef GCC_AMD_HIPEMU
    static std::once_flag lds_opt_in;                        // more than 64 KiB of dynamic LDS has to be opted into
    std::call_once(lds_opt_in, [] {
        for (const void *k : {(const void *)gin_wide2_kernel<false>, (const void *)gin_wide2_kernel<true>,
                              (const void *)gin_wide_big_kernel<false>, (const void *)gin_wide_big_kernel<true>})
            (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, kLds);
    });
#endif
    // one workgroup per CU (137 KB of LDS each), walking the subgraphs with a stride of the grid
    const dim3 grid(min(a.batch_size, 256)), block(kT);
    if (frag) hipLaunchKernelGGL((gin_wide2_kernel<true>), grid, block, kLds, s, a);
    else hipLaunchKernelGGL((gin_wide2_kernel<false>), grid, block, kLds, s, a);
    if (a.big_work) {
        hipLaunchKernelGGL(ginw_classify_kernel, dim3(1), dim3(256), 0, s, a);
        const uint16_t *hin = x_in;
        for (int l = 0; l < a.num_layers; ++l) {
            uint16_t *hout = (l == a.num_layers - 1 && x_out) ? x_out : ((l & 1) ? a.big1 : a.big0);
            if (frag) hipLaunchKernelGGL((gin_wide_big_kernel<true>), dim3(256), dim3(kT), kLds, s, a, l, hin, hout);
            else hipLaunchKernelGGL((gin_wide_big_kernel<false>), dim3(256), dim3(kT), kLds, s, a, l, hin, hout);
            hin = hout;
        }
    }
}

// the layer parameters into a.layers; returns through `frag` whether every layer carries the fragment-major copies.
// -1: a layer has a NULL parameter (its index in `bad`)
int bind_layers(WideArgs &a, const gcc_ginw_layer *layers, int num_layers, bool &frag, int &bad)
{
    frag = true;
    for (int i = 0; i < GCC_GIN_MAX_LAYERS; ++i) {
        a.layers[i] = layers[i];
        const gcc_ginw_layer &l = layers[i];
        if (i < num_layers && (!l.w0 || !l.w1 || !l.s0 || !l.t0 || !l.s1 || !l.t1 || !l.s2 || !l.t2)) { bad = i; return -1; }
        if (i < num_layers) frag = frag && l.w0_frag && l.w1_frag;
    }
    return 0;
}

void bind_scratch(WideArgs &a, void *scratch, const WideScratchLayout &sl)
{
    char *base = (char *)scratch;
    a.big0 = (uint16_t *)(base + sl.rows[0]);
    a.big1 = (uint16_t *)(base + sl.rows[1]);
    a.big_work = (int32_t *)(base + sl.work);
    a.big_cap = (int32_t)sl.cap;
}

// gcc_ginw_embed's workspace: the feature rows of the view in flight ([node_cap][256] bf16; the views run one after the
// other on the stream and share it), then the scratch of the layers
struct EmbedLayout {
    int64_t x, scratch, total;
    WideScratchLayout sl;
};
EmbedLayout embed_layout(int64_t node_cap, int32_t batch_size)
{
    EmbedLayout l;
    l.x = 0;
    l.scratch = node_cap * kD * 2;                           // (a multiple of 512: the scratch stays 16-byte aligned)
    l.sl = wide_scratch_layout(node_cap, batch_size);
    l.total = l.scratch + l.sl.total;
    return l;
}

}  // namespace

extern "C" void gcc_ginw_debug_ticks(long long *device_ticks64) { g_ticks = device_ticks64; }

extern "C" int32_t gcc_ginw_pack_weights(const uint16_t *w, uint16_t *w_frag, int32_t which, void *stream)
{
    if (!w || !w_frag || which < 0 || which > 1) {
        snprintf(g_err, kErrLen, "gcc_ginw_pack_weights: bad argument");
        return -1;
    }
    hipLaunchKernelGGL(ginw_pack_kernel, dim3(kD * kD / 8 / 256), dim3(256), 0, (hipStream_t)stream, w, w_frag, (int)which);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { snprintf(g_err, kErrLen, "gcc_ginw_pack_weights: %s", hipGetErrorString(e)); return -10; }
    return 0;
}

extern "C" int32_t gcc_ginw_forward(const gcc_ginw_args *g, int32_t *status, gcc_prof *prof, void *stream)
{
    if (!g || !status || !g->node_off || !g->row_ptr || !g->col_idx || !g->x_in || g->batch_size < 1 || g->num_layers < 1 ||
        g->num_layers > GCC_GIN_MAX_LAYERS || (!g->x_out && !g->pooled)) {
        snprintf(g_err, kErrLen, "gcc_ginw_forward: bad argument");
        return -1;
    }
    WideArgs a;
    a.node_off = g->node_off; a.row_ptr = g->row_ptr; a.col_idx = g->col_idx;
    a.x_in = g->x_in; a.x_out = g->x_out; a.pooled = g->pooled; a.status = status;
    a.batch_size = g->batch_size; a.num_layers = g->num_layers;
    a.ticks = g_ticks;
    a.big0 = a.big1 = nullptr; a.big_work = nullptr; a.big_cap = 0;
    a.mult = 1;
    if (g->scratch) {
        const WideScratchLayout sl = wide_scratch_layout(g->num_nodes, g->batch_size);
        if (g->num_nodes < 1 || g->scratch_bytes < sl.total || ((uintptr_t)g->scratch & 15u)) {
            snprintf(g_err, kErrLen, "gcc_ginw_forward: scratch of %lld bytes (16-byte aligned) needed for %lld nodes",
                     (long long)sl.total, (long long)g->num_nodes);
            return -3;
        }
        bind_scratch(a, g->scratch, sl);
    }
    bool frag;
    int bad = 0;
    if (bind_layers(a, g->layers, g->num_layers, frag, bad) != 0) {
        snprintf(g_err, kErrLen, "gcc_ginw_forward: layer %d has a NULL parameter", bad);
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    prof_mark(prof, 0, s);
    launch_layers(a, frag, g->x_in, g->x_out, s);
    prof_mark(prof, 1, s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { snprintf(g_err, kErrLen, "gcc_ginw_forward: %s", hipGetErrorString(e)); return -10; }
    return 0;
}

extern "C" int64_t gcc_ginw_scratch_bytes(int64_t num_nodes, int32_t batch_size)
{
    if (num_nodes < 1 || batch_size < 1) return -1;
    return wide_scratch_layout(num_nodes, batch_size).total;
}

extern "C" int64_t gcc_ginw_embed_workspace_bytes(int64_t node_cap, int32_t batch_size)
{
    if (node_cap < 1 || node_cap > INT32_MAX || batch_size < 1) {
        snprintf(g_err, kErrLen, "gcc_ginw_embed_workspace_bytes: bad argument");
        return -1;
    }
    return embed_layout(node_cap, batch_size).total;
}

extern "C" int32_t gcc_ginw_embed(const gcc_ginw_embed_args *e, int32_t *status, void *stream)
{
    if (!e || !status || e->num_views < 1 || e->num_views > 2 || e->batch_size < 1 || e->num_layers < 1 ||
        e->num_layers > GCC_GIN_MAX_LAYERS || e->pos_dim < 0 || e->deg_emb_dim < 0 || e->max_degree < 0 || e->edge_multiplicity < 1 ||
        e->node_cap < 1 || e->node_cap > INT32_MAX || !e->out || (e->deg_emb_dim > 0 && !e->degree_embedding)) {
        snprintf(g_err, kErrLen, "gcc_ginw_embed: bad argument");
        return -1;
    }
    const int d_in = e->pos_dim + e->deg_emb_dim + 1;
    if (d_in > kD || e->hidden < 1 || e->hidden > kD || e->out_dim < 1 || e->out_dim > kD) {
        snprintf(g_err, kErrLen, "gcc_ginw_embed: input / hidden / output widths of 1..%d are served (got %d / %d / %d)", kD, d_in,
                 e->hidden, e->out_dim);
        return -1;
    }
    for (int v = 0; v < e->num_views; ++v)
        if (!e->node_off[v] || !e->row_ptr[v] || !e->col_idx[v] || !e->pooled[v] || (e->pos_dim > 0 && !e->pos[v])) {
            snprintf(g_err, kErrLen, "gcc_ginw_embed: view %d has a NULL member", v);
            return -1;
        }
    for (int i = 0; i <= e->num_layers; ++i)
        if (!e->pred_w[i] || !e->pred_b[i]) {
            snprintf(g_err, kErrLen, "gcc_ginw_embed: prediction layer %d has a NULL parameter", i);
            return -1;
        }
    const EmbedLayout el = embed_layout(e->node_cap, e->batch_size);
    if (!e->workspace || e->workspace_bytes < el.total || ((uintptr_t)e->workspace & 15u)) {
        snprintf(g_err, kErrLen, "gcc_ginw_embed: workspace of %lld bytes (16-byte aligned) needed for %lld rows", (long long)el.total,
                 (long long)e->node_cap);
        return -3;
    }
    WideArgs a;
    bool frag;
    int bad = 0;
    if (bind_layers(a, e->layers, e->num_layers, frag, bad) != 0) {
        snprintf(g_err, kErrLen, "gcc_ginw_embed: layer %d has a NULL parameter", bad);
        return -1;
    }
    uint16_t *x = (uint16_t *)((char *)e->workspace + el.x);
    a.x_in = x; a.x_out = nullptr; a.status = status;
    a.batch_size = e->batch_size; a.num_layers = e->num_layers;
    a.ticks = g_ticks;
    a.mult = e->edge_multiplicity;
    bind_scratch(a, (char *)e->workspace + el.scratch, el.sl);
    hipStream_t s = (hipStream_t)stream;
    ReadoutArgs r;
    for (int v = 0; v < e->num_views; ++v) {
        hipLaunchKernelGGL(ginw_feat_kernel, dim3(min(e->batch_size, 1024)), dim3(kT), 0, s, e->node_off[v], e->row_ptr[v], e->seed_local[v],
                           e->pos[v], e->degree_embedding, (int)e->batch_size, (int)e->pos_dim, (int)e->deg_emb_dim, (int)e->max_degree,
                           (int)e->edge_multiplicity, (int)e->node_cap, x);
        a.node_off = e->node_off[v]; a.row_ptr = e->row_ptr[v]; a.col_idx = e->col_idx[v];
        a.pooled = e->pooled[v];
        launch_layers(a, frag, x, nullptr, s);
        r.pooled[v] = e->pooled[v];
    }
    if (e->num_views == 1) r.pooled[1] = nullptr;
    for (int i = 0; i <= GCC_GIN_MAX_LAYERS; ++i) { r.pred_w[i] = e->pred_w[i]; r.pred_b[i] = e->pred_b[i]; }
    r.out = e->out;
    r.B = e->batch_size; r.L = e->num_layers; r.d_in = d_in; r.hidden = e->hidden; r.out_dim = e->out_dim;
    r.num_views = e->num_views; r.normalize = e->normalize; r.norm_eps = e->norm_eps;
    hipLaunchKernelGGL(ginw_readout_kernel, dim3(min((e->batch_size + kRoGraphs - 1) / kRoGraphs, 1024)), dim3(kRoT), 0, s, r);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) { snprintf(g_err, kErrLen, "gcc_ginw_embed: %s", hipGetErrorString(err)); return -10; }
    return 0;
}
