// gcc_amd/csrc/simsearch.hip -- similarity search: cosine ranks, top-k and the counts behind Recall@k (gfx950).
//
// Replaces SimilaritySearch._evaluate (gcc/tasks/similarity_search.py:41-69 of the reference: two row normalisations, one
// emb_2.dot(v) and one argsort per query) for any number of queries; the [mq, mc] score matrix is never stored.
//
//   sim_prep_kernel      one wave per selected row: gather through q_idx / c_idx, L2 norm (wave sum in a fixed order, so equal
//       rows stay bitwise equal), the row zero-padded to Dpad columns into the workspace; flags absent rows, checks the targets.
//   sim_target_kernel    one wave per 16 queries: s_it with the tile kernel's own sequence of MFMAs (A = the 16 targets' rows,
//       B = the 16 queries, the diagonal of the tile), so the counts compare against the very value the tile pass produces.
//   sim_tile_kernel<NC>  grid (mq / 64 query tiles, S candidate splits); the model is nce_slice_kernel's forward.  A wave owns 16
//       queries (B operand, in registers); the split's candidate rows are staged through LDS in 64-row chunks shared by the 4
//       waves, the next chunk's loads in flight while this one is multiplied.  Per 16 x 16 tile a lane holds 4 candidates of one
//       query: the two counters stay in registers, a candidate that beats the query's current k-th entry (rare once the list has
//       warmed up: one ballot per 64 scores) is inserted into the query's sorted list in LDS by the whole wave (lane p holds entry
//       p: position by ballot, shift, write).  Dpad is one of 16 / 32 / 64 / 128 / 256 so that the operand registers are static.
//   sim_merge_kernel     one wave per query: sums the counters over the splits and merges the S sorted partial lists (lane s
//       holds the head of list s; k rounds of a wave arg-best under the total order score descending, column ascending).
// The entry point's scaffold (workspace carving, the NULL and workspace checks) is task_common.h's.
#include "task_common.h"

#include <math.h>

namespace {

constexpr int kThreads = 256;
constexpr int kQTile = 64;        // 4 waves x 16 queries
constexpr int kChunk = 64;        // candidate rows per staged chunk
constexpr int kSimWgs = 256;      // splits = 0: about one workgroup per CU when there are few query tiles
constexpr int kMinSplitRows = 256;

struct F4 { float x, y, z, w; };
__device__ __forceinline__ F4 ld4(const float *p)
{
    const float4 v = *reinterpret_cast<const float4 *>(p);
    F4 r = {v.x, v.y, v.z, v.w};
    return r;
}
__device__ __forceinline__ void st4(float *p, F4 v) { *reinterpret_cast<float4 *>(p) = make_float4(v.x, v.y, v.z, v.w); }

struct SimDev {
    const float *emb_q, *emb_c;
    long long rows_q, ld_q, rows_c, ld_c;
    const int32_t *q_idx, *c_idx, *target;
    int32_t mq, mc, D, Dpad, k, normalize, S, R;
    float *qn, *cn;                      // [mq][Dpad], [mc][Dpad]
    int32_t *qflag, *cflag, *tgt;        // [mq], [mc], [mq]: 1 = present; the checked target column or -1
    float *ts;                           // [mq] target scores
    int32_t *part_g, *part_e;            // [S][mq]
    float *part_ls;                      // [S][mq][k]
    int32_t *part_lc;
    int32_t *greater, *equal_before;
    float *target_score;
    int32_t *topk_col;
    float *topk_score;
    int32_t *status;
};

// (score, column) a precedes (score, column) b in a query's order; an empty entry (-inf, -1) follows everything
__device__ __forceinline__ bool precedes(float sa, int ca, float sb, int cb)
{
    return sa > sb || (sa == sb && (uint32_t)ca < (uint32_t)cb);
}

__global__ __launch_bounds__(kThreads) void sim_prep_kernel(SimDev a)
{
    const int lane = lane_id(), wv = (int)threadIdx.x >> 6;
    const long long row = (long long)blockIdx.x * (kThreads / 64) + wv;
    if (row >= (long long)a.mq + a.mc) return;                      // (the whole wave)
    const bool isq = row < a.mq;
    const int i = (int)(isq ? row : row - a.mq);
    const int32_t *idx = isq ? a.q_idx : a.c_idx;
    const float *emb = isq ? a.emb_q : a.emb_c;
    const long long rows = isq ? a.rows_q : a.rows_c, ld = isq ? a.ld_q : a.ld_c;
    const long long src = idx ? (long long)idx[i] : (long long)i;
    const bool ok = src >= 0 && src < rows;
    int bits = ok ? 0 : GCC_STATUS_SIM_BAD_INDEX;
    float v[4], ss = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int d = lane + 64 * u;
        v[u] = ok && d < a.D ? emb[src * ld + d] : 0.f;
        ss += v[u] * v[u];
    }
    ss = wave_sum(ss);
    if (a.normalize && ok) {
        if (ss == 0.f) bits |= GCC_STATUS_SIM_ZERO_ROW;
        else {
            const float norm = sqrtf(ss);
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = v[u] / norm;
        }
    }
    float *out = (isq ? a.qn : a.cn) + (long long)i * a.Dpad;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int d = lane + 64 * u;
        if (d < a.Dpad) out[d] = v[u];
    }
    if (lane == 0) {
        (isq ? a.qflag : a.cflag)[i] = ok ? 1 : 0;
        if (isq) {
            int t = a.target ? a.target[i] : -1;
            if (t < -1 || t >= a.mc) { bits |= GCC_STATUS_SIM_BAD_INDEX; t = -1; }
            a.tgt[i] = ok ? t : -1;
        }
        if (bits) atomicOr(a.status, (int32_t)bits);                // (the caller's word)
    }
}

// the products of one 16 x 16 tile: candidate rows (A, 4 floats of row j per 16-column block) x queries (B), k in the order
// 16 c + 4 q + {0, 1, 2, 3} -- the ONE sequence both the tile pass and the target scores run
__device__ __forceinline__ f32x4 tile_block(F4 cf, F4 qf, f32x4 acc)
{
    acc = mfma_16x16x4_f32(cf.x, qf.x, acc);
    acc = mfma_16x16x4_f32(cf.y, qf.y, acc);
    acc = mfma_16x16x4_f32(cf.z, qf.z, acc);
    acc = mfma_16x16x4_f32(cf.w, qf.w, acc);
    return acc;
}

__global__ __launch_bounds__(kThreads) void sim_target_kernel(SimDev a)
{
    const int lane = lane_id(), wv = (int)threadIdx.x >> 6, j = lane & 15, q = lane >> 4;
    const long long q0 = ((long long)blockIdx.x * (kThreads / 64) + wv) * 16;
    if (q0 >= a.mq) return;                                         // (the whole wave)
    const int qj = (int)q0 + j;
    const bool qvalid = qj < a.mq;
    int t = qvalid ? a.tgt[qj] : -1;
    if (t >= 0 && !a.cflag[t]) t = -1;                              // the target names an absent candidate
    const float *crow = a.cn + (long long)(t >= 0 ? t : 0) * a.Dpad;
    const float *qrow = a.qn + (long long)(qvalid ? qj : 0) * a.Dpad;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < a.Dpad / 16; ++c) acc = tile_block(ld4(crow + 16 * c + 4 * q), ld4(qrow + 16 * c + 4 * q), acc);
    // acc[r] = <target of query 4 q + r, query j>: the diagonal is in lane group q = j / 4, register j % 4
    const int r = j & 3;
    const float d = r == 0 ? acc[0] : r == 1 ? acc[1] : r == 2 ? acc[2] : acc[3];
    if (qvalid && q == (j >> 2)) {
        a.tgt[qj] = t;
        a.ts[qj] = t >= 0 ? d : NAN;
    }
}

template <int NC, bool kLists>
__global__ __launch_bounds__(kThreads) void sim_tile_kernel(SimDev a)
{
    constexpr int kDp = 16 * NC, kLd = kDp + 4;                      // LDS row stride: 16-byte aligned, rows 4 banks apart
    DYN_SMEM(smem);
    float *Cs = reinterpret_cast<float *>(smem);                    // [kChunk][kLd]
    int32_t *flag_s = reinterpret_cast<int32_t *>(Cs + kChunk * kLd);   // [kChunk] 1 = a live candidate of this split
    float *list_s = reinterpret_cast<float *>(flag_s + kChunk);     // [kQTile][k]
    int32_t *list_c = reinterpret_cast<int32_t *>(list_s + kQTile * a.k);
    const int tid = (int)threadIdx.x, lane = lane_id(), wv = tid >> 6, j = lane & 15, q = lane >> 4;
    const int s = (int)blockIdx.y, k = a.k;
    const long long qbase = (long long)blockIdx.x * kQTile + 16 * wv;
    const bool qin = qbase + j < a.mq;
    const int qj = qin ? (int)(qbase + j) : 0;
    const bool qvalid = qin && a.qflag[qj] != 0;
    F4 qf[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) qf[c] = ld4(a.qn + (long long)qj * kDp + 16 * c + 4 * q);
    const int t = qvalid ? a.tgt[qj] : -1;
    const float ts = t >= 0 ? a.ts[qj] : 0.f;
    int g = 0, e = 0;
    float thr_s = -INFINITY;                                        // the query's current k-th entry
    int thr_c = -1;
    float *my_ls = list_s + 16 * wv * k;
    int32_t *my_lc = list_c + 16 * wv * k;
    if (kLists) {
        for (int p = lane; p < 16 * k; p += 64) { my_ls[p] = -INFINITY; my_lc[p] = -1; }
        wave_sync();
    }
    const int row_beg = s * a.R, row_end = min(a.mc, row_beg + a.R);
    F4 nxt[NC];
    int nflag = 0;
    auto request = [&](int c0) {
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const int idx = tid + kThreads * i, row = idx / (4 * NC), c4 = (idx % (4 * NC)) * 4;
            nxt[i] = ld4(a.cn + (long long)min(c0 + row, a.mc - 1) * kDp + c4);
        }
        if (tid < kChunk) nflag = c0 + tid < row_end ? a.cflag[c0 + tid] : 0;
    };
    if (row_beg < row_end) request(row_beg);
    for (int c0 = row_beg; c0 < row_end; c0 += kChunk) {
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const int idx = tid + kThreads * i, row = idx / (4 * NC), c4 = (idx % (4 * NC)) * 4;
            st4(&Cs[row * kLd + c4], nxt[i]);
        }
        if (tid < kChunk) flag_s[tid] = nflag;
        __syncthreads();
        if (c0 + kChunk < row_end) request(c0 + kChunk);
        for (int tt = 0; tt < kChunk / 16; ++tt) {
            if (c0 + 16 * tt >= row_end) break;                     // block-uniform
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < NC; ++c) acc = tile_block(ld4(&Cs[(16 * tt + j) * kLd + 16 * c + 4 * q]), qf[c], acc);
            // acc[r] = <candidate col0 + r, query j>
            const int col0 = c0 + 16 * tt + 4 * q;
            const int4 fl = *reinterpret_cast<const int4 *>(&flag_s[16 * tt + 4 * q]);
            const float sc[4] = {acc[0], acc[1], acc[2], acc[3]};
            const bool live[4] = {fl.x != 0, fl.y != 0, fl.z != 0, fl.w != 0};
            if (t >= 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    g += live[r] && sc[r] > ts ? 1 : 0;
                    e += live[r] && sc[r] == ts && col0 + r < t ? 1 : 0;
                }
            }
            if (kLists) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int col = col0 + r;
                    unsigned long long hits = wave_ballot(qvalid && live[r] && precedes(sc[r], col, thr_s, thr_c));
                    while (hits) {                                  // wave-uniform
                        const int L = __ffsll(hits) - 1;
                        hits &= hits - 1;
                        const float ns = wave_readlane(sc[r], L);
                        const int nc = wave_readlane(col, L), qq = L & 15;
                        float *ls = my_ls + qq * k;
                        int32_t *lc = my_lc + qq * k;
                        const bool in = lane < k;
                        const float es = in ? ls[lane] : 0.f;
                        const int ec = in ? lc[lane] : 0;
                        // the list is sorted, so the entries that precede the newcomer are a leading run
                        const int pos = __popcll(wave_ballot(in && precedes(es, ec, ns, nc)));
                        if (pos < k) {                              // (an earlier hit of this tile may have raised the bar)
                            wave_sync();
                            if (in && lane >= pos && lane + 1 < k) { ls[lane + 1] = es; lc[lane + 1] = ec; }
                            if (lane == pos) { ls[pos] = ns; lc[pos] = nc; }
                            wave_sync();
                            // the new k-th entry, without waiting for the list: the newcomer itself, or the old entry k - 2
                            const float old_s = wave_readlane(es, k >= 2 ? k - 2 : 0);
                            const int old_c = wave_readlane(ec, k >= 2 ? k - 2 : 0);
                            if (j == qq) { thr_s = pos == k - 1 ? ns : old_s; thr_c = pos == k - 1 ? nc : old_c; }
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
    g += wave_shfl_xor(g, 16); g += wave_shfl_xor(g, 32);
    e += wave_shfl_xor(e, 16); e += wave_shfl_xor(e, 32);
    if (q == 0 && qin) {
        a.part_g[(long long)s * a.mq + qj] = g;
        a.part_e[(long long)s * a.mq + qj] = e;
    }
    if (kLists) {
        wave_sync();
        for (int p = lane; p < 16 * k; p += 64) {
            const long long qrow = qbase + p / k;
            if (qrow < a.mq) {
                const long long o = ((long long)s * a.mq + qrow) * k + p % k;
                a.part_ls[o] = my_ls[p];
                a.part_lc[o] = my_lc[p];
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void sim_merge_kernel(SimDev a)
{
    const int lane = lane_id(), wv = (int)threadIdx.x >> 6, k = a.k;
    const long long i = (long long)blockIdx.x * (kThreads / 64) + wv;
    if (i >= a.mq) return;                                          // (the whole wave)
    const bool live = lane < a.S;
    const int t = a.tgt[i];
    int g = live ? a.part_g[(long long)lane * a.mq + i] : 0, e = live ? a.part_e[(long long)lane * a.mq + i] : 0;
    for (int d = 32; d >= 1; d >>= 1) { g += wave_shfl_xor(g, d); e += wave_shfl_xor(e, d); }
    if (lane == 0) {
        if (a.greater) a.greater[i] = t >= 0 ? g : -1;
        if (a.equal_before) a.equal_before[i] = t >= 0 ? e : -1;
        if (a.target_score) a.target_score[i] = a.ts[i];
    }
    if (k == 0 || (!a.topk_col && !a.topk_score)) return;
    const float *ls = a.part_ls + ((long long)(live ? lane : 0) * a.mq + i) * k;
    const int32_t *lc = a.part_lc + ((long long)(live ? lane : 0) * a.mq + i) * k;
    int ptr = 0;
    float hs = live ? ls[0] : -INFINITY;
    int hc = live ? lc[0] : -1;
    for (int m = 0; m < k; ++m) {
        float bs = hs;
        int bc = hc, bl = lane;
        for (int d = 32; d >= 1; d >>= 1) {
            const float os = wave_shfl_xor(bs, d);
            const int oc = wave_shfl_xor(bc, d), ol = wave_shfl_xor(bl, d);
            // (two empty heads tie on score and column: the lower lane wins, so every lane ends with the same winner)
            if (precedes(os, oc, bs, bc) || (os == bs && oc == bc && ol < bl)) { bs = os; bc = oc; bl = ol; }
        }
        if (lane == 0) {
            if (a.topk_score) a.topk_score[i * k + m] = bs;
            if (a.topk_col) a.topk_col[i * k + m] = bc;
        }
        if (lane == bl && bc >= 0) {
            ++ptr;
            hs = ptr < k ? ls[ptr] : -INFINITY;
            hc = ptr < k ? lc[ptr] : -1;
        }
    }
}

struct Plan { int32_t Dpad, S, R, QB; int64_t off_qn, off_cn, off_qflag, off_cflag, off_tgt, off_ts, off_pg, off_pe, off_ls, off_lc, total; };

// sizes are checked by the caller: 0 <= mq, mc; 1 <= D <= GCC_SIM_MAX_DIM; 0 <= k <= GCC_SIM_MAX_K; 0 <= splits <= GCC_SIM_MAX_SPLITS
Plan make_plan(int32_t mq, int32_t mc, int32_t D, int32_t k, int32_t splits)
{
    Plan p;
    p.Dpad = 16;
    while (p.Dpad < D) p.Dpad *= 2;
    p.QB = (int32_t)(((int64_t)mq + kQTile - 1) / kQTile);
    int64_t s = splits;
    if (s == 0) {                            // every CU a workgroup when there are few query tiles, splits of >= 256 rows
        s = p.QB > 0 ? (kSimWgs + p.QB - 1) / p.QB : 1;
        const int64_t by_rows = ((int64_t)mc + kMinSplitRows - 1) / kMinSplitRows;
        if (s > by_rows) s = by_rows;
    }
    if (s > GCC_SIM_MAX_SPLITS) s = GCC_SIM_MAX_SPLITS;
    if (s < 1) s = 1;
    const int64_t r = ((((int64_t)mc + s - 1) / s) + 15) / 16 * 16;
    p.R = (int32_t)(r < 16 ? 16 : r);
    p.S = (int32_t)(((int64_t)mc + p.R - 1) / p.R);
    if (p.S < 1) p.S = 1;
    Carve cv;
    p.off_qn = cv.take((int64_t)mq * p.Dpad * 4);
    p.off_cn = cv.take((int64_t)mc * p.Dpad * 4);
    p.off_qflag = cv.take((int64_t)mq * 4);
    p.off_cflag = cv.take((int64_t)mc * 4);
    p.off_tgt = cv.take((int64_t)mq * 4);
    p.off_ts = cv.take((int64_t)mq * 4);
    p.off_pg = cv.take((int64_t)p.S * mq * 4);
    p.off_pe = cv.take((int64_t)p.S * mq * 4);
    p.off_ls = cv.take((int64_t)p.S * mq * k * 4);
    p.off_lc = cv.take((int64_t)p.S * mq * k * 4);
    p.total = cv.total();
    return p;
}

int check_sizes(const char *who, int32_t mq, int32_t mc, int32_t D, int32_t k, int32_t splits)
{
    if (mq < 0 || mc < 0) {
        snprintf(g_err, kErrLen, "%s: mq %d / mc %d must not be negative", who, mq, mc);
        return -2;
    }
    if (D < 1 || D > GCC_SIM_MAX_DIM) {
        snprintf(g_err, kErrLen, "%s: D %d outside 1..GCC_SIM_MAX_DIM (%d)", who, D, GCC_SIM_MAX_DIM);
        return -3;
    }
    if (k < 0 || k > GCC_SIM_MAX_K) {
        snprintf(g_err, kErrLen, "%s: k %d outside 0..GCC_SIM_MAX_K (%d)", who, k, GCC_SIM_MAX_K);
        return -4;
    }
    if (splits < 0 || splits > GCC_SIM_MAX_SPLITS) {
        snprintf(g_err, kErrLen, "%s: splits %d outside 0..GCC_SIM_MAX_SPLITS (%d)", who, splits, GCC_SIM_MAX_SPLITS);
        return -5;
    }
    return 0;
}

template <int NC, bool kLists> void launch_tiles(const SimDev &d, const Plan &pl, hipStream_t s)
{
    const size_t lds = ((size_t)kChunk * (16 * NC + 4) + kChunk) * 4 + (kLists ? (size_t)kQTile * d.k * 8 : 0);
#ifndef GCC_AMD_HIPEMU
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute((const void *)sim_tile_kernel<NC, kLists>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
#endif
    hipLaunchKernelGGL((sim_tile_kernel<NC, kLists>), dim3(pl.QB, pl.S), dim3(kThreads), lds, s, d);
}

template <bool kLists> void launch_tiles_nc(const SimDev &d, const Plan &pl, hipStream_t s)
{
    switch (pl.Dpad) {
    case 16: launch_tiles<1, kLists>(d, pl, s); break;
    case 32: launch_tiles<2, kLists>(d, pl, s); break;
    case 64: launch_tiles<4, kLists>(d, pl, s); break;
    case 128: launch_tiles<8, kLists>(d, pl, s); break;
    default: launch_tiles<16, kLists>(d, pl, s); break;
    }
}

}  // namespace

extern "C" {

int64_t gcc_sim_workspace_bytes(int32_t mq, int32_t mc, int32_t D, int32_t k, int32_t splits)
{
    const int rc = check_sizes("gcc_sim_workspace_bytes", mq, mc, D, k, splits);
    if (rc) return rc;
    return make_plan(mq, mc, D, k, splits).total;
}

int32_t gcc_sim_search(const gcc_sim_args *h, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream)
{
    const char *who = "gcc_sim_search";
    int rc = null_member(who, {{h, "args"}});
    if (rc) return rc;
    if ((rc = check_sizes(who, h->mq, h->mc, h->D, h->k, h->splits))) return rc;
    if ((rc = null_member(who, {{h->emb_q, "emb_q"}, {h->emb_c, "emb_c"}, {status, "status"}}))) return rc;
    if (h->rows_q < 0 || h->rows_c < 0 || h->ld_q < h->D || h->ld_c < h->D) {
        snprintf(g_err, kErrLen, "%s: rows_q %lld / rows_c %lld must not be negative, ld_q %lld / ld_c %lld must be at least D (%d)",
                 who, (long long)h->rows_q, (long long)h->rows_c, (long long)h->ld_q, (long long)h->ld_c, h->D);
        return -6;
    }
    if ((!h->q_idx && h->mq > h->rows_q) || (!h->c_idx && h->mc > h->rows_c)) {
        snprintf(g_err, kErrLen, "%s: mq %d / mc %d beyond rows_q %lld / rows_c %lld without q_idx / c_idx", who, h->mq, h->mc,
                 (long long)h->rows_q, (long long)h->rows_c);
        return -7;
    }
    if (h->mq == 0 || h->mc == 0) return 0;
    const Plan pl = make_plan(h->mq, h->mc, h->D, h->k, h->splits);
    if ((rc = check_workspace(who, "gcc_sim_workspace_bytes", workspace, workspace_bytes, pl.total))) return rc;
    SimDev d = {};
    d.emb_q = h->emb_q; d.emb_c = h->emb_c;
    d.rows_q = h->rows_q; d.ld_q = h->ld_q; d.rows_c = h->rows_c; d.ld_c = h->ld_c;
    d.q_idx = h->q_idx; d.c_idx = h->c_idx; d.target = h->target;
    d.mq = h->mq; d.mc = h->mc; d.D = h->D; d.Dpad = pl.Dpad; d.k = h->k; d.normalize = h->normalize; d.S = pl.S; d.R = pl.R;
    d.qn = ws_at<float>(workspace, pl.off_qn); d.cn = ws_at<float>(workspace, pl.off_cn);
    d.qflag = ws_at<int32_t>(workspace, pl.off_qflag); d.cflag = ws_at<int32_t>(workspace, pl.off_cflag);
    d.tgt = ws_at<int32_t>(workspace, pl.off_tgt); d.ts = ws_at<float>(workspace, pl.off_ts);
    d.part_g = ws_at<int32_t>(workspace, pl.off_pg); d.part_e = ws_at<int32_t>(workspace, pl.off_pe);
    d.part_ls = ws_at<float>(workspace, pl.off_ls); d.part_lc = ws_at<int32_t>(workspace, pl.off_lc);
    d.greater = h->greater; d.equal_before = h->equal_before; d.target_score = h->target_score;
    d.topk_col = h->topk_col; d.topk_score = h->topk_score;
    d.status = status;
    hipStream_t s = (hipStream_t)stream;
    const int wpb = kThreads / 64;
    const long long prep_rows = (long long)h->mq + h->mc;
    hipLaunchKernelGGL(sim_prep_kernel, dim3((unsigned)((prep_rows + wpb - 1) / wpb)), dim3(kThreads), 0, s, d);
    hipLaunchKernelGGL(sim_target_kernel, dim3((unsigned)((((long long)h->mq + 15) / 16 + wpb - 1) / wpb)), dim3(kThreads), 0, s, d);
    if (h->k > 0) launch_tiles_nc<true>(d, pl, s);
    else launch_tiles_nc<false>(d, pl, s);
    hipLaunchKernelGGL(sim_merge_kernel, dim3((unsigned)(((long long)h->mq + wpb - 1) / wpb)), dim3(kThreads), 0, s, d);
    return launched();
}

}  // extern "C"
