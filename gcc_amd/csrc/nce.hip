// gcc_amd/csrc/nce.hip -- MoCo / InfoNCE head (gfx950).
//
// Replaces MemoryMoCo.forward (gcc/contrastive/memory_moco.py:26-63: bmm/mm/cat/div/clone) and
// NCESoftmaxLoss / NCESoftmaxLossNS (gcc/contrastive/criterions.py:5-33: CrossEntropyLoss over
// [B, K+1]).  The queue's enqueue (index_copy_) and moment_update are step_tail.hip's.
//
//   (dtype GCC_NCE_BF16: the same kernels with q / k / queue rounded to bf16 on load -- the forward logits then run on
//   v_mfma_f32_16x16x32_bf16, 2 instructions per 16 x 16 tile instead of 16; accumulation and softmax stay fp32)
//   nce_slice_kernel<false>  grid (S slices of the queue, B/64 query blocks).  The slice's rows
//       are staged through LDS in 64-row chunks shared by the 4 waves; each wave owns 16 queries:
//       logits tile = exact-f32 MFMA (queue rows x queries), online row-softmax (running max /
//       sum) in registers; per-(slice, query) partials go to HBM.  K = 16384, B = 256: 537 MFLOP,
//       4 MiB of queue read once per query block.
//   nce_combine_kernel       merges the partials: lse, positive logit, mean loss, mean prob.
//   nce_slice_kernel<true>   backward: recomputes the logits tile, p = exp(l - lse), and feeds it
//       straight into a second MFMA (p^T x queue rows) -- the 4 logits a lane holds after the
//       first MFMA are exactly the B-operand values it must supply to the second, so P never
//       leaves registers.  Per-slice dq slabs are reduced in a fixed order by nce_dq_kernel.
// [B, K+1] is only materialised when the caller asks for it (train.py indexes out[:, 0]).
#include "host_common.h"

#include <math.h>

namespace {

constexpr int D = GCC_NCE_DIM;    // 64
constexpr int kLd = 72;           // LDS row stride (floats)
constexpr int kChunk = 64;        // queue rows per staged chunk
constexpr int kThreads = 256;
constexpr int kQPerBlock = 64;    // 4 waves x 16 queries

struct F4 { float x, y, z, w; };
__device__ __forceinline__ F4 ld4(const float *p)
{
    const float4 v = *reinterpret_cast<const float4 *>(p);
    F4 r = {v.x, v.y, v.z, v.w};
    return r;
}
__device__ __forceinline__ void st4(float *p, F4 v) { *reinterpret_cast<float4 *>(p) = make_float4(v.x, v.y, v.z, v.w); }

struct NceDev {
    const float *q, *k, *mem, *patch;
    int32_t patch_index, patch_rows, B, K, pos_mode;
    int32_t bf16;            // operands rounded to bf16 (f32 accumulation): gcc_nce_args.dtype
    int32_t defer;           // the means are formed in the backward call (gcc_nce_args.pos_mode 2; pos_mode here is 0 then)
    float inv_T;
    float *lse, *pos, *loss, *prob, *out_dense;
    int32_t S, R;             // slices and rows per slice (multiple of kChunk)
    float *pm, *ps;           // [S][B] partial max / sum
    float *slabs;             // [S][B][64] partial dq (backward)
    int32_t *ticket;          // arrival counter of nce_combine_kernel's workgroups (zeroed by the forward slice kernel)
    const float *dloss;
    int32_t by_mem_row;
    float *dq;
};

#ifndef GCC_NCE_WGS_DEFAULT
#define GCC_NCE_WGS_DEFAULT 256
#endif
constexpr int kNceWgs = GCC_NCE_WGS_DEFAULT;     // ~one workgroup per CU: enough to spread the queue, few enough slabs to reduce
struct Plan { int32_t S, R, QB; int64_t off_pm, off_ps, off_slabs, off_ticket, total; };

inline Plan make_plan(int32_t B, int32_t K)
{
    Plan p;
    p.QB = (B + kQPerBlock - 1) / kQPerBlock;
    static int wgs = 0;                      // workgroups of a slice launch (GCC_NCE_WGS: timing experiments)
    if (wgs == 0) { const char *e = getenv("GCC_NCE_WGS"); wgs = e ? atoi(e) : 0; if (wgs <= 0) wgs = kNceWgs; }
    int s = (wgs + p.QB - 1) / p.QB;
    const int maxs = (K + kChunk - 1) / kChunk;
    if (s > maxs) s = maxs;
    if (s < 1) s = 1;
    p.R = (((K + s - 1) / s) + kChunk - 1) / kChunk * kChunk;
    p.S = (K + p.R - 1) / p.R;
    auto al = [](int64_t x) { return (x + 255) & ~(int64_t)255; };
    int64_t o = 0;
    p.off_pm = o; o = al(o + (int64_t)p.S * B * 4);
    p.off_ps = o; o = al(o + (int64_t)p.S * B * 4);
    p.off_slabs = o; o = al(o + (int64_t)p.S * B * D * 4);
    p.off_ticket = o; o = al(o + 4);
    p.total = o;
    return p;
}

__device__ __forceinline__ float rnd_bf16(float x) { return bf16_bits_to_f32(f32_to_bf16_bits(x)); }
__device__ __forceinline__ F4 rnd4(F4 v, bool on)
{
    if (on) { v.x = rnd_bf16(v.x); v.y = rnd_bf16(v.y); v.z = rnd_bf16(v.z); v.w = rnd_bf16(v.w); }
    return v;
}
// two fp32 values that are exactly representable in bf16 -> one packed pair (low half = first)
__device__ __forceinline__ uint32_t pack_bf16(float lo, float hi) { return (__float_as_uint(lo) >> 16) | (__float_as_uint(hi) & 0xFFFF0000u); }

// One unconditional 16-byte load per call (the ADDRESS is selected, not the load: with the load under branches the compiler
// waited for each of a thread's four rows before requesting the next); rows >= K read row 0 and are zeroed by the caller.
__device__ __forceinline__ const float *mem_row_ptr(const NceDev &a, int r)
{
    const float *p = a.mem + (int64_t)(r < a.K ? r : 0) * D;
    if (a.patch) {                                   // (uniform) queue rows already overwritten by the enqueue
        int rel = r - a.patch_index;
        if (rel < 0) rel += a.K;
        if (r < a.K && rel < a.patch_rows) p = a.patch + (int64_t)rel * D;
    }
    return p;
}
// what follows a queue-row load once ALL loads of the batch have been requested: rows past the end are zeros, bf16 mode rounds
__device__ __forceinline__ F4 finish_mem4(const NceDev &a, F4 v, int r)
{
    if (r >= a.K) { F4 z = {0.f, 0.f, 0.f, 0.f}; v = z; }
    return rnd4(v, a.bf16 != 0);
}

template <bool kBwd, bool kBf16>
__global__ __launch_bounds__(kThreads) void nce_slice_kernel(NceDev a)
{
    TRAIN_STEP_WAVE_PRIORITY();
    __shared__ float Ms[kChunk * kLd];
    const int tid = (int)threadIdx.x, lane = lane_id(), wv = tid >> 6, j = lane & 15, q = lane >> 4;
    const int s = (int)blockIdx.x;
    if (!kBwd && s == 0 && blockIdx.y == 0 && tid == 0) *a.ticket = 0;     // arrival counter of nce_combine_kernel
    const int qj = (int)blockIdx.y * kQPerBlock + 16 * wv + j;
    const bool qvalid = qj < a.B;
    F4 qf[4];
    const float *qrow = a.q + (int64_t)(qvalid ? qj : 0) * D;      // (unconditional loads, masked afterwards)
#pragma unroll
    for (int c = 0; c < 4; ++c) qf[c] = ld4(qrow + 16 * c + 4 * q);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        F4 z = {0.f, 0.f, 0.f, 0.f};
        qf[c] = qvalid ? rnd4(qf[c], kBf16) : z;
    }
    // bf16 mode, forward logits on v_mfma_f32_16x16x32_bf16: lane (j, q) supplies 8 consecutive k of query j for the k-group q of
    // each 32-wide slab (the queue rows come from LDS the same way); the products of bf16 values are exact in fp32, so the
    // result differs from the fp32-MFMA path on the rounded operands (what the backward recomputes) by summation order only
    u32x4 qb[2];
    if (kBf16 && !kBwd) {
#pragma unroll
        for (int sl = 0; sl < 2; ++sl) {
            F4 z = {0.f, 0.f, 0.f, 0.f};
            const F4 lo = qvalid ? rnd4(ld4(a.q + (int64_t)qj * D + 32 * sl + 8 * q), true) : z;
            const F4 hi = qvalid ? rnd4(ld4(a.q + (int64_t)qj * D + 32 * sl + 8 * q + 4), true) : z;
            qb[sl][0] = pack_bf16(lo.x, lo.y); qb[sl][1] = pack_bf16(lo.z, lo.w);
            qb[sl][2] = pack_bf16(hi.x, hi.y); qb[sl][3] = pack_bf16(hi.z, hi.w);
        }
    }
    const int row_beg = s * a.R, row_end = min(a.K, row_beg + a.R);
    const int ld_out = a.K + (a.pos_mode == 0 ? 1 : 0), off_out = a.pos_mode == 0 ? 1 : 0;
    float m = -INFINITY, ssum = 0.f;
    float my_lse = 0.f;
    if (kBwd && !a.by_mem_row && qvalid) my_lse = a.lse[qj];
    f32x4 acc2[4];
    if (kBwd) {
#pragma unroll
        for (int db = 0; db < 4; ++db) { f32x4 z = {0.f, 0.f, 0.f, 0.f}; acc2[db] = z; }
    }
    // the next chunk of queue rows is requested while this one is being multiplied (a slice is 4 chunks: a round trip each)
    F4 nxt[4];
    auto request = [&](int c0) {                     // raw loads only: zeroing / rounding wait until the chunk is stored
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + kThreads * i, row = idx >> 4, c4 = (idx & 15) * 4;
            nxt[i] = ld4(mem_row_ptr(a, c0 + row) + c4);
        }
    };
    if (row_beg < row_end) request(row_beg);
    for (int c0 = row_beg; c0 < row_end; c0 += kChunk) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + kThreads * i, row = idx >> 4, c4 = (idx & 15) * 4;
            st4(&Ms[row * kLd + c4], finish_mem4(a, nxt[i], c0 + row));
        }
        __syncthreads();
        if (c0 + kChunk < row_end) request(c0 + kChunk);
        for (int t = 0; t < 4; ++t) {
            if (c0 + 16 * t >= row_end) break;      // block-uniform
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            if (kBf16 && !kBwd) {
#pragma unroll
                for (int sl = 0; sl < 2; ++sl) {
                    const F4 lo = ld4(&Ms[(16 * t + j) * kLd + 32 * sl + 8 * q]), hi = ld4(&Ms[(16 * t + j) * kLd + 32 * sl + 8 * q + 4]);
                    u32x4 mb;
                    mb[0] = pack_bf16(lo.x, lo.y); mb[1] = pack_bf16(lo.z, lo.w);
                    mb[2] = pack_bf16(hi.x, hi.y); mb[3] = pack_bf16(hi.z, hi.w);
                    acc = mfma_16x16x32_bf16(mb, qb[sl], acc);
                }
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const F4 mf = ld4(&Ms[(16 * t + j) * kLd + 16 * c + 4 * q]);
                    acc = mfma_16x16x4_f32(mf.x, qf[c].x, acc);
                    acc = mfma_16x16x4_f32(mf.y, qf[c].y, acc);
                    acc = mfma_16x16x4_f32(mf.z, qf[c].z, acc);
                    acc = mfma_16x16x4_f32(mf.w, qf[c].w, acc);
                }
            }
            // acc[r] = mem[row0 + r] . q[qj], row0 = c0 + 16 t + 4 q
            const int row0 = c0 + 16 * t + 4 * q;
            float lv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float l = acc[r] * a.inv_T;                      // torch.div(out, self.T), memory_moco.py:43
                const bool valid = row0 + r < row_end;
                if (!kBwd && a.out_dense && qvalid && valid) a.out_dense[(int64_t)qj * ld_out + off_out + row0 + r] = l;
                lv[r] = valid ? l : -INFINITY;
            }
            if (!kBwd) {
                const float tmax = fmaxf(fmaxf(lv[0], lv[1]), fmaxf(lv[2], lv[3]));
                if (tmax > -INFINITY) {
                    const float mn = fmaxf(m, tmax);
                    ssum = ssum * expf(m - mn) + expf(lv[0] - mn) + expf(lv[1] - mn) + expf(lv[2] - mn) + expf(lv[3] - mn);
                    m = mn;
                }
            } else {
                float lse_r[4] = {my_lse, my_lse, my_lse, my_lse};
                if (a.by_mem_row) {                          // (uniform) E2E: the softmax runs over the other view's rows
#pragma unroll
                    for (int r = 0; r < 4; ++r) lse_r[r] = a.lse[min(row0 + r, a.K - 1)];      // four loads requested together
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float p = 0.f;
                    if (qvalid && lv[r] > -INFINITY) p = expf(lv[r] - lse_r[r]);
                    // second GEMM: dq[query][d] += p[row][query] * mem[row][d]; this lane's p is the
                    // B operand (k = q <-> row 4q + r, column j = query)
#pragma unroll
                    for (int db = 0; db < 4; ++db)
                        acc2[db] = mfma_16x16x4_f32(Ms[(16 * t + 4 * q + r) * kLd + 16 * db + j], p, acc2[db]);
                }
            }
        }
        __syncthreads();
    }
    if (!kBwd) {
#pragma unroll
        for (int d = 16; d <= 32; d <<= 1) {
            const float m2 = wave_shfl_xor(m, d), s2 = wave_shfl_xor(ssum, d);
            const float mn = fmaxf(m, m2);
            ssum = mn > -INFINITY ? ssum * expf(m - mn) + s2 * expf(m2 - mn) : 0.f;
            m = mn;
        }
        if (q == 0 && qvalid) {
            a.pm[(int64_t)s * a.B + qj] = m;
            a.ps[(int64_t)s * a.B + qj] = ssum;
        }
    } else if (qvalid) {
#pragma unroll
        for (int db = 0; db < 4; ++db) {
            F4 o = {acc2[db][0], acc2[db][1], acc2[db][2], acc2[db][3]};
            st4(a.slabs + ((int64_t)s * a.B + qj) * D + 16 * db + 4 * q, o);
        }
    }
}

// Forward AND backward of the MoCo head (pos_mode 0, f32) in ONE pass over the queue -- flash-attention's identity applied to
// q . queue^T / T.  Per 16-row tile: logits on the MFMA as nce_slice_kernel<false>; the running maximum m of a query is made
// COMMON to its four lane groups before the tile's exp (in the second MFMA the reduction index runs over those groups, so their
// p~ = exp(l - m) must share one reference); p~ goes straight into the second MFMA (p~^T x queue rows, the operand identity of
// nce_slice_kernel<true>) and the accumulators are rescaled by exp(m_old - m_new) whenever the maximum rises.  No assumption
// about the size of the logits.  Per (slice, query): pm = m, ps = sum p~, slab = sum p~ row (unnormalised; nce_merge_kernel
// weighs it with exp(pm - lse)).
__global__ __launch_bounds__(kThreads) void nce_onepass_kernel(NceDev a)
{
    TRAIN_STEP_WAVE_PRIORITY();
    __shared__ float Ms[kChunk * kLd];
    const int tid = (int)threadIdx.x, lane = lane_id(), wv = tid >> 6, j = lane & 15, q = lane >> 4;
    const int s = (int)blockIdx.x;
    if (s == 0 && blockIdx.y == 0 && tid == 0) *a.ticket = 0;      // arrival counter of nce_merge_kernel
    const int qj = (int)blockIdx.y * kQPerBlock + 16 * wv + j;
    const bool qvalid = qj < a.B;
    F4 qf[4];
    const float *qrow = a.q + (int64_t)(qvalid ? qj : 0) * D;      // (unconditional loads, masked afterwards)
#pragma unroll
    for (int c = 0; c < 4; ++c) qf[c] = ld4(qrow + 16 * c + 4 * q);
#pragma unroll
    for (int c = 0; c < 4; ++c) {                    // (per component: a select between two F4 objects is a select of addresses -- scratch)
        qf[c].x = qvalid ? qf[c].x : 0.f; qf[c].y = qvalid ? qf[c].y : 0.f;
        qf[c].z = qvalid ? qf[c].z : 0.f; qf[c].w = qvalid ? qf[c].w : 0.f;
    }
    const int row_beg = s * a.R, row_end = min(a.K, row_beg + a.R);
    float m = -INFINITY, ssum = 0.f;                 // m: the same value in the four lane groups of a query
    f32x4 acc2[4];
#pragma unroll
    for (int db = 0; db < 4; ++db) { f32x4 z = {0.f, 0.f, 0.f, 0.f}; acc2[db] = z; }
    F4 nxt[4];
    auto request = [&](int c0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + kThreads * i, row = idx >> 4, c4 = (idx & 15) * 4;
            nxt[i] = ld4(mem_row_ptr(a, c0 + row) + c4);
        }
    };
    if (row_beg < row_end) request(row_beg);
    for (int c0 = row_beg; c0 < row_end; c0 += kChunk) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + kThreads * i, row = idx >> 4, c4 = (idx & 15) * 4;
            st4(&Ms[row * kLd + c4], finish_mem4(a, nxt[i], c0 + row));
        }
        __syncthreads();
        if (c0 + kChunk < row_end) request(c0 + kChunk);
        for (int t = 0; t < 4; ++t) {
            if (c0 + 16 * t >= row_end) break;      // block-uniform
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const F4 mf = ld4(&Ms[(16 * t + j) * kLd + 16 * c + 4 * q]);
                acc = mfma_16x16x4_f32(mf.x, qf[c].x, acc);
                acc = mfma_16x16x4_f32(mf.y, qf[c].y, acc);
                acc = mfma_16x16x4_f32(mf.z, qf[c].z, acc);
                acc = mfma_16x16x4_f32(mf.w, qf[c].w, acc);
            }
            // acc[r] = mem[row0 + r] . q[qj], row0 = c0 + 16 t + 4 q
            const int row0 = c0 + 16 * t + 4 * q;
            float lv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) lv[r] = row0 + r < row_end ? acc[r] * a.inv_T : -INFINITY;
            float tmax = fmaxf(fmaxf(lv[0], lv[1]), fmaxf(lv[2], lv[3]));
            tmax = fmaxf(tmax, wave_shfl_xor(tmax, 16));           // the tile's maximum over all 16 rows of the query
            tmax = fmaxf(tmax, wave_shfl_xor(tmax, 32));
            const float mn = fmaxf(m, tmax);
            const float sc = mn > -INFINITY ? expf(m - mn) : 1.f;  // (m = -inf before the first valid row: 0, and acc2 is 0)
            float p[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) p[r] = lv[r] > -INFINITY ? expf(lv[r] - mn) : 0.f;
            ssum = ssum * sc + ((p[0] + p[1]) + (p[2] + p[3]));
            m = mn;
#pragma unroll
            for (int db = 0; db < 4; ++db) acc2[db] *= sc;
            // second GEMM: slab[query][d] += p~[row][query] * mem[row][d]; this lane's p~ is the B operand (k = q <-> row
            // 4q + r, column j = query); the lane's accumulators all belong to query j, whose sc it holds
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int db = 0; db < 4; ++db)
                    acc2[db] = mfma_16x16x4_f32(Ms[(16 * t + 4 * q + r) * kLd + 16 * db + j], p[r], acc2[db]);
        }
        __syncthreads();
    }
    ssum += wave_shfl_xor(ssum, 16);                 // (one common m: the lane groups' sums simply add)
    ssum += wave_shfl_xor(ssum, 32);
    if (qvalid) {
        if (q == 0) {
            a.pm[(int64_t)s * a.B + qj] = m;
            a.ps[(int64_t)s * a.B + qj] = ssum;
        }
#pragma unroll
        for (int db = 0; db < 4; ++db) {
            F4 o = {acc2[db][0], acc2[db][1], acc2[db][2], acc2[db][3]};
            st4(a.slabs + ((int64_t)s * a.B + qj) * D + 16 * db + 4 * q, o);
        }
    }
}

// mean loss / mean positive logit by ONE workgroup, in index order (deterministic), from lse / pos that are visible to it: the
// workgroup that arrives last (nce_mean_by_last), or a workgroup of a later launch (nce_dq_kernel's extra one)
__device__ __forceinline__ void nce_means(const NceDev &a, double *red /* [8] */)
{
    const int tid = (int)threadIdx.x, lane = lane_id(), wv = tid >> 6;
    double lsum = 0.0, psum = 0.0;
    for (int i = tid; i < a.B; i += kThreads) {
        const float lse = load_fresh(a.lse + i), pos = load_fresh(a.pos + i);
        lsum += (double)(lse - pos);                             // CrossEntropyLoss row term
        psum += (double)pos;
    }
    lsum = wave_sum(lsum);
    psum = wave_sum(psum);
    if (lane == 0) { red[wv] = lsum; red[4 + wv] = psum; }
    __syncthreads();
    if (tid == 0) {
        a.loss[0] = (float)((red[0] + red[1] + red[2] + red[3]) / (double)a.B);    // reduction="mean"
        a.prob[0] = (float)((red[4] + red[5] + red[6] + red[7]) / (double)a.B);    // out[:, 0].mean(), train.py:394
    }
}

// nce_means by the workgroup that arrives last; every workgroup has written its lse / pos before it calls this
__device__ __forceinline__ void nce_mean_by_last(const NceDev &a, double *red, int *last)
{
    const int tid = (int)threadIdx.x;
    device_fence();                                              // lse / pos of this workgroup are visible device wide
    __syncthreads();
    if (tid == 0) *last = atomicAdd(a.ticket, 1) == (int)gridDim.x - 1;
    __syncthreads();
    if (!*last) return;
    device_fence();
    nce_means(a, red);
    if (tid == 0) *a.ticket = 0;
}

#ifndef NCE_MERGE_BATCH
#define NCE_MERGE_BATCH 32   // slabs requested per round
#endif
// nce_combine_kernel + nce_dq_kernel for nce_onepass_kernel's partials (pos_mode 0): one wave per query.  lse / pos exactly as
// nce_combine_kernel forms them; then dq[b] = dloss / (B T) * (sum_s exp(pm_s - lse) slab_s[b] + (exp(pos - lse) - 1) k[b]),
// slabs in slice order (lane = feature dim).  A slice without a valid row (pm = -inf) counts as zero, whatever its slab holds.
__global__ __launch_bounds__(kThreads) void nce_merge_kernel(NceDev a)
{
    TRAIN_STEP_WAVE_PRIORITY();
    __shared__ double red[8];
    __shared__ int last;
    const int tid = (int)threadIdx.x, lane = lane_id(), wv = tid >> 6;
    const int b = (int)blockIdx.x * (kThreads >> 6) + wv;
    if (b < a.B) {                                   // wave-uniform
        // one round trip: the query, the key, the first 64 slices' maxima and sums, dloss and the first batch of slabs
        const float qv = a.q[(int64_t)b * D + lane], kv = a.k[(int64_t)b * D + lane];
        const int s0 = min(lane, a.S - 1);
        const float pm0r = a.pm[(int64_t)s0 * a.B + b], ps0r = a.ps[(int64_t)s0 * a.B + b];
        const float dl = a.dloss[0];
        const float *sp = a.slabs + (int64_t)b * D + lane;
        const int64_t st = (int64_t)a.B * D;
        float v[NCE_MERGE_BATCH];
#pragma unroll
        for (int u = 0; u < NCE_MERGE_BATCH; ++u) v[u] = sp[(int64_t)min(u, a.S - 1) * st];
        const float pm0 = lane < a.S ? pm0r : -INFINITY;
        const float pos = wave_sum(qv * kv) * a.inv_T;
        float m = pm0;
        for (int s = lane + 64; s < a.S; s += 64) m = fmaxf(m, a.pm[(int64_t)s * a.B + b]);
        m = fmaxf(wave_max(m), pos);
        float sum = pm0 > -INFINITY ? ps0r * expf(pm0 - m) : 0.f;
        for (int s = lane + 64; s < a.S; s += 64) {
            const float pmv = a.pm[(int64_t)s * a.B + b], psv = a.ps[(int64_t)s * a.B + b];
            if (pmv > -INFINITY) sum += psv * expf(pmv - m);
        }
        sum = wave_sum(sum) + expf(pos - m);
        const float lse = m + logf(sum);
        if (lane == 0) {
            a.lse[b] = lse;
            a.pos[b] = pos;
        }
        float acc = 0.f;
        for (int base = 0; base < a.S; base += 64) {              // lane l holds the weight of slice base + l
            float pmv = pm0;
            if (base > 0) pmv = base + lane < a.S ? a.pm[(int64_t)(base + lane) * a.B + b] : -INFINITY;
            const float w = pmv > -INFINITY ? expf(pmv - lse) : 0.f;
            const int send = min(a.S, base + 64);
            for (int sl = base; sl < send; sl += NCE_MERGE_BATCH) {
                if (sl > 0) {
#pragma unroll
                    for (int u = 0; u < NCE_MERGE_BATCH; ++u) v[u] = sp[(int64_t)min(sl + u, a.S - 1) * st];
                }
#pragma unroll
                for (int u = 0; u < NCE_MERGE_BATCH; ++u) {
                    if (sl + u < send) {                           // wave-uniform
                        const float ws = wave_readlane(w, sl + u - base);
                        if (ws > 0.f) acc = fmaf(ws, v[u], acc);
                    }
                }
            }
        }
        const float coef = dl * a.inv_T / (float)a.B;
        a.dq[(int64_t)b * D + lane] = coef * (acc + (expf(pos - lse) - 1.f) * kv);
    }
    nce_mean_by_last(a, red, &last);
}

__global__ __launch_bounds__(kThreads) void nce_combine_kernel(NceDev a)
{
    TRAIN_STEP_WAVE_PRIORITY();
    // one wave per query (lanes over the 64 feature dims / the slices); the workgroup that arrives last adds the
    // per-query terms up in index order (deterministic) for the mean loss and the mean positive logit
    __shared__ double red[8];
    __shared__ int last;
    const int tid = (int)threadIdx.x, lane = lane_id(), wv = tid >> 6;
    const int ld_out = a.K + (a.pos_mode == 0 ? 1 : 0);
    const int b = (int)blockIdx.x * (kThreads >> 6) + wv;
    if (b < a.B) {
        const float *other = a.pos_mode == 0 ? a.k : a.mem;        // l_pos = bmm(q, k) | diagonal of k q^T
        // (the query, the key and the first 64 slices' maxima and sums in one round trip; more slices loop below)
        float qv = a.q[(int64_t)b * D + lane], ov = other[(int64_t)b * D + lane];
        const int s0 = min(lane, a.S - 1);
        const float pm0r = a.pm[(int64_t)s0 * a.B + b], ps0r = a.ps[(int64_t)s0 * a.B + b];
        const float pm0 = lane < a.S ? pm0r : -INFINITY;
        if (a.bf16) { qv = rnd_bf16(qv); ov = rnd_bf16(ov); }
        const float pos = wave_sum(qv * ov) * a.inv_T;
        float m = pm0;
        for (int s = lane + 64; s < a.S; s += 64) m = fmaxf(m, a.pm[(int64_t)s * a.B + b]);
        m = wave_max(m);
        if (a.pos_mode == 0) m = fmaxf(m, pos);
        float sum = pm0 > -INFINITY ? ps0r * expf(pm0 - m) : 0.f;
        for (int s = lane + 64; s < a.S; s += 64) {
            const float pmv = a.pm[(int64_t)s * a.B + b], psv = a.ps[(int64_t)s * a.B + b];
            if (pmv > -INFINITY) sum += psv * expf(pmv - m);
        }
        sum = wave_sum(sum);
        if (a.pos_mode == 0) sum += expf(pos - m);
        const float lse = m + logf(sum);
        if (lane == 0) {
            a.lse[b] = lse;
            a.pos[b] = pos;
            if (a.pos_mode == 0 && a.out_dense) a.out_dense[(int64_t)b * ld_out] = pos;
        }
    }
    // Nothing on the stream reads loss / prob before the step's meters.  Deferred: the kernel ends here and nce_dq_kernel's
    // extra workgroup forms the two means (the ticket, zeroed by the forward slice kernel, is not touched); otherwise the
    // workgroup that arrives last does -- a fence, a returning atomic and a second fence behind every workgroup's stores.
    if (a.defer) return;                                         // (uniform)
    nce_mean_by_last(a, red, &last);
}

#ifndef NCE_DQ_BATCH
#define NCE_DQ_BATCH 16      // slabs requested per round
#endif
__global__ __launch_bounds__(kThreads) void nce_dq_kernel(NceDev a)
{
    TRAIN_STEP_WAVE_PRIORITY();
    __shared__ double red[8];
    if (a.defer && blockIdx.x == gridDim.x - 1) {              // (block-uniform) the extra workgroup of a deferred head: the means
        nce_means(a, red);                                       // that nce_combine_kernel left out, beside the 16 that sum the slabs
        return;
    }
    const int gid = (int)blockIdx.x * kThreads + (int)threadIdx.x;
    const int b = gid >> 4, c4 = (gid & 15) * 4;
    if (b >= a.B) return;
    // everything the epilogue needs is requested first and the slabs 16 at a time: with 4 per round and the scalars
    // loaded at the end this was S / 4 + 3 = 19 dependent round trips for ~1 us of data
    const float dl = a.dloss[0];
    const float posb = a.pos_mode == 0 ? a.pos[b] : 0.f, lseb = a.pos_mode == 0 ? a.lse[b] : 0.f;     // (block-uniform branch)
    const F4 other = rnd4(ld4((a.pos_mode == 0 ? a.k : a.mem) + (int64_t)b * D + c4), a.bf16 != 0);
    F4 s = {0.f, 0.f, 0.f, 0.f};
    const float *sp = a.slabs + (int64_t)b * D + c4;
    const int64_t st = (int64_t)a.B * D;
    for (int sl = 0; sl < a.S; sl += NCE_DQ_BATCH) {  // fixed summation order: slab 0, 1, 2, ...
        F4 v[NCE_DQ_BATCH];
#pragma unroll
        for (int u = 0; u < NCE_DQ_BATCH; ++u) v[u] = ld4(sp + (int64_t)min(sl + u, a.S - 1) * st);
#pragma unroll
        for (int u = 0; u < NCE_DQ_BATCH; ++u)
            if (sl + u < a.S) { s.x += v[u].x; s.y += v[u].y; s.z += v[u].z; s.w += v[u].w; }
    }
    const int nrows = a.by_mem_row ? a.K : a.B;              // rows of the softmax that is averaged
    const float coef = dl * a.inv_T / (float)nrows;
    F4 o;
    if (a.pos_mode == 0) {
        const float pp = expf(posb - lseb) - 1.f;
        o.x = coef * (s.x + pp * other.x); o.y = coef * (s.y + pp * other.y);
        o.z = coef * (s.z + pp * other.z); o.w = coef * (s.w + pp * other.w);
    } else {
        o.x = coef * (s.x - other.x); o.y = coef * (s.y - other.y); o.z = coef * (s.z - other.z); o.w = coef * (s.w - other.w);
    }
    st4(a.dq + (int64_t)b * D + c4, o);
}

inline int fill_dev(const gcc_nce_args *a, void *workspace, int64_t workspace_bytes, NceDev &d, Plan &pl)
{
    if (!a || !a->q || !a->mem || a->B < 1 || a->K < 1 || (a->pos_mode != 1 && !a->k) ||
        (a->pos_mode == 1 && a->K < a->B) || !a->lse || !a->pos || a->pos_mode < 0 || a->pos_mode > GCC_NCE_POS_MOCO_DEFERRED ||
        (a->pos_mode == GCC_NCE_POS_MOCO_DEFERRED && (!a->loss || !a->prob || a->out_dense))) {
        snprintf(g_err, kErrLen, "gcc_nce: bad argument");
        return -1;
    }
    pl = make_plan(a->B, a->K);
    if (!workspace || workspace_bytes < pl.total) {
        snprintf(g_err, kErrLen, "gcc_nce: workspace %lld < %lld bytes", (long long)workspace_bytes, (long long)pl.total);
        return -3;
    }
    d.q = a->q; d.k = a->k; d.mem = a->mem; d.patch = a->patch;
    d.patch_index = a->patch_index; d.patch_rows = a->patch ? a->patch_rows : 0;
    d.defer = a->pos_mode == GCC_NCE_POS_MOCO_DEFERRED ? 1 : 0;
    d.B = a->B; d.K = a->K; d.pos_mode = d.defer ? 0 : a->pos_mode; d.inv_T = a->inv_T;
    d.bf16 = a->dtype == GCC_NCE_BF16 ? 1 : 0;
    d.lse = a->lse; d.pos = a->pos; d.loss = a->loss; d.prob = a->prob; d.out_dense = a->out_dense;
    d.S = pl.S; d.R = pl.R;
    char *base = (char *)workspace;
    d.pm = (float *)(base + pl.off_pm); d.ps = (float *)(base + pl.off_ps); d.slabs = (float *)(base + pl.off_slabs);
    d.ticket = (int32_t *)(base + pl.off_ticket);
    d.dloss = nullptr; d.by_mem_row = 0; d.dq = nullptr;
    return 0;
}

}  // namespace

extern "C" {

int64_t gcc_nce_workspace_bytes(int32_t B, int32_t K)
{
    if (B < 1 || K < 1) { snprintf(g_err, kErrLen, "gcc_nce_workspace_bytes: bad argument"); return -1; }
    return make_plan(B, K).total;
}

int32_t gcc_nce_forward(const gcc_nce_args *a, void *workspace, int64_t workspace_bytes, gcc_prof *prof, void *stream)
{
    NceDev d;
    Plan pl;
    int rc = fill_dev(a, workspace, workspace_bytes, d, pl);
    if (rc) return rc;
    if (!a->loss || !a->prob) { snprintf(g_err, kErrLen, "gcc_nce_forward: loss/prob are required"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    prof_mark(prof, 0, s);
    if (d.bf16) hipLaunchKernelGGL((nce_slice_kernel<false, true>), dim3(pl.S, pl.QB), dim3(kThreads), 0, s, d);
    else hipLaunchKernelGGL((nce_slice_kernel<false, false>), dim3(pl.S, pl.QB), dim3(kThreads), 0, s, d);
    hipLaunchKernelGGL(nce_combine_kernel, dim3((d.B + (kThreads >> 6) - 1) / (kThreads >> 6)), dim3(kThreads), 0, s, d);
    prof_mark(prof, 1, s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { snprintf(g_err, kErrLen, "gcc_nce_forward: %s", hipGetErrorString(e)); return -10; }
    return 0;
}

int32_t gcc_nce_backward(const gcc_nce_args *a, const float *dloss, int32_t by_mem_row, float *dq, void *workspace,
                         int64_t workspace_bytes, gcc_prof *prof, void *stream)
{
    NceDev d;
    Plan pl;
    int rc = fill_dev(a, workspace, workspace_bytes, d, pl);
    if (rc) return rc;
    if (!dloss || !dq || (by_mem_row && a->pos_mode != 1)) {
        snprintf(g_err, kErrLen, "gcc_nce_backward: bad argument");
        return -1;
    }
    d.dloss = dloss; d.by_mem_row = by_mem_row; d.dq = dq;
    hipStream_t s = (hipStream_t)stream;
    prof_mark(prof, 0, s);
    if (d.bf16) hipLaunchKernelGGL((nce_slice_kernel<true, true>), dim3(pl.S, pl.QB), dim3(kThreads), 0, s, d);
    else hipLaunchKernelGGL((nce_slice_kernel<true, false>), dim3(pl.S, pl.QB), dim3(kThreads), 0, s, d);
    hipLaunchKernelGGL(nce_dq_kernel, dim3((a->B * 16 + kThreads - 1) / kThreads + d.defer), dim3(kThreads), 0, s, d);
    prof_mark(prof, 1, s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { snprintf(g_err, kErrLen, "gcc_nce_backward: %s", hipGetErrorString(e)); return -10; }
    return 0;
}

int32_t gcc_nce_forward_backward(const gcc_nce_args *a, const float *dloss, float *dq, void *workspace,
                                 int64_t workspace_bytes, gcc_prof *prof_fwd, gcc_prof *prof_bwd, void *stream)
{
    NceDev d;
    Plan pl;
    int rc = fill_dev(a, workspace, workspace_bytes, d, pl);
    if (rc) return rc;
    if (!a->loss || !a->prob || !dloss || !dq) { snprintf(g_err, kErrLen, "gcc_nce_forward_backward: bad argument"); return -1; }
    if (a->pos_mode != 0 || a->out_dense || d.bf16) {
        snprintf(g_err, kErrLen, "gcc_nce_forward_backward: pos_mode 0, f32, no dense output (use gcc_nce_forward + gcc_nce_backward)");
        return -2;
    }
    d.dloss = dloss; d.dq = dq;
    hipStream_t s = (hipStream_t)stream;
    prof_mark(prof_fwd, 0, s);
    hipLaunchKernelGGL(nce_onepass_kernel, dim3(pl.S, pl.QB), dim3(kThreads), 0, s, d);
    prof_mark(prof_fwd, 1, s);
    prof_mark(prof_bwd, 0, s);
    hipLaunchKernelGGL(nce_merge_kernel, dim3((d.B + (kThreads >> 6) - 1) / (kThreads >> 6)), dim3(kThreads), 0, s, d);
    prof_mark(prof_bwd, 1, s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { snprintf(g_err, kErrLen, "gcc_nce_forward_backward: %s", hipGetErrorString(e)); return -10; }
    return 0;
}

}  // extern "C"
