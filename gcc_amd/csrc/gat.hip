// gcc_amd/csrc/gat.hip -- the GAT backbone of GraphEncoder(gnn_model="gat") (gfx950), forward and backward.
//
// Replaces gcc/models/gat.py (DGL GATLayer / GATConv, agg_mode "flatten") and the Set2Set / lin_readout / F.normalize
// tail of graph_encoder.py:189-196.  No BatchNorm anywhere: no two subgraphs of a batch are coupled, so
//   gat_forward_kernel   ONE workgroup per subgraph runs the whole forward: input features, L GAT layers, T Set2Set
//                        iterations of Lr LSTM layers, the readout and the normalisation.  Rows live in L2 (the pass's
//                        `saved` buffer: it is what the backward reads), so subgraphs of every size work.  Per layer:
//                        fc on the exact-f32 MFMA (W staged in LDS, one wave per 16-row block) with el / er in its
//                        epilogue, then the edge softmax per destination row with an online max / sum (one wave per
//                        row, lanes over channels); the log-sum-exp per (node, head) is saved.
//   gat_backward_kernel  ONE workgroup per subgraph: normalize / readout / Set2Set BPTT (LSTM gates and cells, alpha per
//                        (iteration, node) from `saved`), then the GAT layers from the last one down.  Attention is
//                        recomputed from el, er and the log-sum-exp; ds = a (da - <drst_v, rst_v>) times the leaky-ReLU
//                        slope.  The batch is symmetric (row u lists u's in-neighbours AND its out-neighbours), so
//                        every "scatter to the source" term (dft_u, del_u) is a gather over u's own row: no atomics.
//                        It leaves per-row / per-graph gradients dZ (dft, del, der, LSTM dz, readout dz) and dx0.
//   gat_wgrad_kernel     weight gradients as per-chunk partials sum_rows dZ^T X over fixed row chunks ...
//   gat_reduce_kernel    ... summed over the chunks in order (the project's rule: no float atomics, bit-identical runs).
// A backward is three launches; none of the counts depends on T or Lr.
#include "host_common.h"

#include <math.h>

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxD = 64;
constexpr int kLdw = 65;                 // LDS row stride of the staged 64 x 64 weight block and of the wave tiles
constexpr int kMaxL = GCC_GAT_MAX_LAYERS;
constexpr int kMaxLr = GCC_GAT_MAX_S2S_LAYERS;
constexpr int kChunksNode = 64;          // row chunks of the per-node weight gradients
constexpr int kChunksSeq = 16;           // ... of the LSTM weight gradients (T * B rows)
constexpr int kChunksGraph = 4;          // ... of the readout weight gradients (B rows)
constexpr int kMaxJobs = 3 * kMaxL + 2 * kMaxLr + 3;
constexpr int kRowBlk = 32;              // rows staged per round of gat_wgrad_kernel
constexpr int kEdgeJ = 8;                // CSR entries whose gathers are in flight together in the per-row loops

struct Dims {
    int32_t L, D, H, F, K0, Dout, T, Lr, pos, emb, maxdeg, cap, B, norm;
    float eps;
};

// float offsets into gcc_gat_pass.saved
struct Saved {
    int64_t x0, ft, rst, el, er, lse, alpha, gates, cst, hst, qstar, hid, opre, total;
};
// float offsets into the backward workspace
struct Work {
    int64_t dcur, drst, cvh, dft, del, der, dx0, dz, dhid, dz2, part, total;
};

Saved saved_layout(const Dims &d)
{
    Saved s = {};
    int64_t o = 0;
    const int64_t cap = d.cap, B = d.B;
    s.x0 = o; o += cap * d.K0;
    s.ft = o; o += (int64_t)d.L * cap * d.D;
    s.rst = o; o += (int64_t)d.L * cap * d.D;
    s.el = o; o += (int64_t)d.L * cap * d.H;
    s.er = o; o += (int64_t)d.L * cap * d.H;
    s.lse = o; o += (int64_t)d.L * cap * d.H;
    s.alpha = o; o += (int64_t)d.T * cap;
    s.gates = o; o += (int64_t)d.Lr * d.T * B * 4 * d.D;    // [Lr][T][B][4D] gate activations i, f, g, o
    s.cst = o; o += (int64_t)d.Lr * d.T * B * d.D;          // [Lr][T][B][D] cell states
    s.hst = o; o += (int64_t)d.Lr * d.T * B * d.D;          // [Lr][T][B][D] hidden states
    s.qstar = o; o += (int64_t)(d.T + 1) * B * 2 * d.D;     // [T + 1][B][2D]: q*_0 = 0 .. q*_T (the readout's input)
    s.hid = o; o += B * d.D;                                 // lin_readout.0 output (before the ReLU)
    s.opre = o; o += B * d.Dout;                             // lin_readout.2 output (before F.normalize)
    s.total = o;
    return s;
}

// ---- weight-gradient jobs: out[M][K] (+ bias[M]) = sum over rows r of dz[r][m] x[r][k]
enum { kJobGemm = 0, kJobDiag = 1, kJobEmb = 2 };
struct WJob {
    const float *dz, *x;
    float *part;                          // [chunks][size]
    int32_t type, ldz, ldx, xact;         // xact: 0 none, 1 leaky_relu(0.01), 2 relu
    int32_t M, K, rows, chunks;           // rows < 0: the batch's live node count node_off[B]
    int32_t bias, F;                      // bias: also column sums of dz; F: diag jobs, dz column = k / F
};
struct WArgs {
    WJob job[kMaxJobs];
    const int32_t *node_off, *row_ptr;
    int32_t B, mult, maxdeg, emb, pos, K0;
};
struct RJob {
    const float *part;
    float *dst, *dst_b, *dst_b2;          // dst [M * K]; bias [M] into dst_b (and dst_b2: the LSTM's b_hh)
    int32_t size, mk, chunks, reserved_;
};
struct RArgs {
    RJob job[kMaxJobs];
    int32_t accumulate;
};

__host__ __device__ inline int64_t job_size(const WJob &j)
{
    return j.type == kJobGemm ? (int64_t)j.M * j.K + (j.bias ? j.M : 0) : (int64_t)j.M * j.K;
}

Work work_layout(const Dims &d)
{
    Work w = {};
    int64_t o = 0;
    const int64_t cap = d.cap, B = d.B;
    w.dcur = o; o += cap * d.D;           // d(output of the current layer), per node
    w.drst = o; o += cap * d.D;           // d(aggregated rst) of the current layer
    w.cvh = o; o += cap * (d.H > 1 ? d.H : 1);    // <drst_v, rst_v> per (node, head); Set2Set: per-node scratch
    w.dft = o; o += (int64_t)d.L * cap * d.D;
    w.del = o; o += (int64_t)d.L * cap * d.H;
    w.der = o; o += (int64_t)d.L * cap * d.H;
    w.dx0 = o; o += cap * d.K0;
    w.dz = o; o += (int64_t)d.Lr * d.T * B * 4 * d.D;
    w.dhid = o; o += B * d.D;
    w.dz2 = o; o += B * d.Dout;
    w.part = o;
    w.total = o;                          // + the partials (gat_jobs)
    return w;
}

__device__ __forceinline__ float lrelu(float x, float s) { return x > 0.f ? x : s * x; }
__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }

struct FwdArgs {
    gcc_gat_weights w;
    const int32_t *node_off, *row_ptr, *col_idx, *seed_local;
    const float *pos;
    float *sv, *out;
    int32_t mult;
    Dims d;
    Saved s;
};

struct BwdArgs {
    gcc_gat_weights w;
    const int32_t *node_off, *row_ptr, *col_idx;
    const float *sv, *dout;
    float *ws;
    Dims d;
    Saved s;
    Work k;
};

// W [D][Kin] (row-major, nn.Linear.weight) -> Ws[64][kLdw], zero outside [D) x [Kin); attention vectors -> al / ar
__device__ __forceinline__ void stage_layer(const float *W, const float *attl, const float *attr, int D, int Kin, float *Ws,
                                            float *al, float *ar)
{
    const int tid = (int)threadIdx.x;
    for (int e = tid; e < 64 * 64; e += kThreads) {
        const int o = e >> 6, k = e & 63;
        Ws[o * kLdw + k] = (o < D && k < Kin) ? W[o * Kin + k] : 0.f;
    }
    if (tid < 64) {
        al[tid] = tid < D ? attl[tid] : 0.f;
        ar[tid] = tid < D ? attr[tid] : 0.f;
    }
}

// one wave: acc[cb][r] = Y[r0 + (lane >> 4) * 4 + r][16 cb + (lane & 15)] for a 16-row block.
// kTrans = false: Y = X W^T (X [rows][Kin], Ws[o][k]);  kTrans = true: Y = X W (X [rows][D], Ws[k][o]).
// X rows >= rend and columns >= kdim read as 0; act: leaky_relu(0.01) on X (the previous layer's activation).
template <bool kTrans>
__device__ __forceinline__ void mfma_rows16(const float *X, int ldx, int kdim, bool act, int r0, int rend, const float *Ws,
                                            int nb, f32x4 acc[4])
{
    const int lane = lane_id(), ar = r0 + (lane & 15), kq = lane >> 4, col = lane & 15;
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < kdim; k0 += 4) {
        const int k = k0 + kq;
        float a = 0.f;
        if (ar < rend && k < kdim) {
            a = X[(int64_t)ar * ldx + k];
            if (act) a = lrelu(a, 0.01f);
        }
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            if (cb < nb) {                       // (wave-uniform)
                const float b = kTrans ? Ws[k * kLdw + 16 * cb + col] : Ws[(16 * cb + col) * kLdw + k];
                acc[cb] = mfma_16x16x4_f32(a, b, acc[cb]);
            }
        }
    }
}

// sum / max over the workgroup (every thread calls; fixed order: wave reduction, then the waves in order)
__device__ __forceinline__ float block_sum(float v, float *red)
{
    const int tid = (int)threadIdx.x;
    v = wave_sum(v);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    float s = 0.f;
    for (int i = 0; i < kWaves; ++i) s += red[i];
    return s;
}
__device__ __forceinline__ float block_max(float v, float *red)
{
    const int tid = (int)threadIdx.x;
    v = wave_max(v);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    float m = red[0];
    for (int i = 1; i < kWaves; ++i) m = fmaxf(m, red[i]);
    return m;
}

// =====================================================================================================================
__global__ __launch_bounds__(kThreads) void gat_forward_kernel(FwdArgs a)
{
    TRAIN_STEP_WAVE_PRIORITY();
    __shared__ float Ws[64 * kLdw];
    __shared__ float tile[kWaves * 16 * kLdw];
    __shared__ float al[64], ar[64];
    __shared__ float qs[2 * kMaxD], hcur[kMaxLr * kMaxD], ccur[kMaxLr * kMaxD], gs[4 * kMaxD], red[4 * 64];
    const Dims &d = a.d;
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = a.node_off[b], n1 = a.node_off[b + 1], n = n1 - n0;
    const int D = d.D, H = d.H, F = d.F, cap = d.cap;
    float *sv = a.sv;

    // ---- input features (graph_encoder.py:152-165): [pos | degree_embedding(clamp(in_degree)) | seed]
    {
        const int seed = n0 + (a.seed_local ? a.seed_local[b] : 0);
        const int dtot = d.pos + d.emb;
        for (int e = tid; e < n * d.K0; e += kThreads) {
            const int v = n0 + e / d.K0, c = e - (e / d.K0) * d.K0;
            float x;
            if (c < d.pos) {
                x = a.pos[(int64_t)v * d.pos + c];
            } else if (c < dtot) {
                const int deg = (a.row_ptr[v + 1] - a.row_ptr[v]) * a.mult;
                x = a.w.degree_embedding[(int64_t)min(deg, d.maxdeg) * d.emb + (c - d.pos)];
            } else {
                x = v == seed ? 1.f : 0.f;
            }
            sv[a.s.x0 + (int64_t)v * d.K0 + c] = x;
        }
    }
    __syncthreads();

    for (int l = 0; l < d.L; ++l) {
        const int Kin = l == 0 ? d.K0 : D;
        const float *X = l == 0 ? sv + a.s.x0 : sv + a.s.rst + (int64_t)(l - 1) * cap * D;
        float *ft = sv + a.s.ft + (int64_t)l * cap * D, *rst = sv + a.s.rst + (int64_t)l * cap * D;
        float *el = sv + a.s.el + (int64_t)l * cap * H, *er = sv + a.s.er + (int64_t)l * cap * H;
        float *lse = sv + a.s.lse + (int64_t)l * cap * H;
        stage_layer(a.w.fc[l], a.w.attn_l[l], a.w.attn_r[l], D, Kin, Ws, al, ar);
        __syncthreads();
        // ---- ft = h W^T on the MFMA; el / er in the epilogue
        const int nb = (D + 15) >> 4;
        float *tw = tile + wave * 16 * kLdw;
        for (int rb = wave; rb * 16 < n; rb += kWaves) {
            const int r0 = n0 + rb * 16;
            f32x4 acc[4];
            mfma_rows16<false>(X, Kin, Kin, l > 0, r0, n1, Ws, nb, acc);
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
                if (cb < nb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) tw[((lane >> 4) * 4 + r) * kLdw + 16 * cb + (lane & 15)] = acc[cb][r];
            wave_sync();
            for (int r = 0; r < 16; ++r) {
                const int v = r0 + r;
                if (v < n1 && lane < D) ft[(int64_t)v * D + lane] = tw[r * kLdw + lane];
            }
            for (int p = lane; p < 16 * H; p += 64) {
                const int r = p / H, h = p - r * H, v = r0 + r;
                if (v < n1) {
                    float sl = 0.f, sr = 0.f;
                    for (int f = 0; f < F; ++f) {
                        const float x = tw[r * kLdw + h * F + f];
                        sl = fmaf(x, al[h * F + f], sl);
                        sr = fmaf(x, ar[h * F + f], sr);
                    }
                    el[(int64_t)v * H + h] = sl;
                    er[(int64_t)v * H + h] = sr;
                }
            }
            wave_sync();
        }
        __syncthreads();
        // ---- edge softmax over v's incoming edges (its CSR row) + aggregation: online max / sum, lanes over channels
        {
            const int j = lane < D ? lane : D - 1, h = j / F;
            for (int v = n0 + wave; v < n1; v += kWaves) {
                const int e0 = a.row_ptr[v], e1 = a.row_ptr[v + 1];
                const float erv = er[(int64_t)v * H + h];
                float m = -INFINITY, s = 0.f, acc = 0.f;
                auto step = [&](float x, float f) {
                    if (x > m) {
                        const float sc = expf(m - x);
                        s = fmaf(s, sc, 1.f);
                        acc = fmaf(acc, sc, f);
                        m = x;
                    } else {
                        const float p = expf(x - m);
                        s += p;
                        acc = fmaf(p, f, acc);
                    }
                };
                // kEdgeJ edges' loads in flight before the first (serial) update: one edge at a time, a hub row of a
                // thousand entries was a thousand dependent col_idx -> el / ft round trips
                int e = e0;
                for (; e + kEdgeJ <= e1; e += kEdgeJ) {
                    int u[kEdgeJ];
                    float x[kEdgeJ], f[kEdgeJ];
#pragma unroll
                    for (int i = 0; i < kEdgeJ; ++i) u[i] = a.col_idx[e + i];
#pragma unroll
                    for (int i = 0; i < kEdgeJ; ++i) {
                        x[i] = lrelu(el[(int64_t)u[i] * H + h] + erv, 0.2f);
                        f[i] = ft[(int64_t)u[i] * D + j];
                    }
#pragma unroll
                    for (int i = 0; i < kEdgeJ; ++i) step(x[i], f[i]);
                }
                for (; e < e1; ++e) {
                    const int u = a.col_idx[e];
                    step(lrelu(el[(int64_t)u * H + h] + erv, 0.2f), ft[(int64_t)u * D + j]);
                }
                if (lane < D) rst[(int64_t)v * D + lane] = s > 0.f ? acc / s : 0.f;      // no incoming edge: 0
                if (lane < D && lane == h * F) lse[(int64_t)v * H + h] = s > 0.f ? m + logf(s) : 0.f;
            }
        }
        __syncthreads();
    }

    // ---- Set2Set(D, T, Lr) over x = the last layer's output (no activation on the last layer)
    const float *xL = sv + a.s.rst + (int64_t)(d.L - 1) * cap * D;
    const int B = d.B, T = d.T, Lr = d.Lr;
    if (tid < 2 * D) {
        qs[tid] = 0.f;
        sv[a.s.qstar + (int64_t)b * 2 * D + tid] = 0.f;
    }
    for (int i = tid; i < Lr * kMaxD; i += kThreads) { hcur[i] = 0.f; ccur[i] = 0.f; }
    __syncthreads();
    for (int t = 0; t < T; ++t) {
        for (int k = 0; k < Lr; ++k) {
            const int in = k == 0 ? 2 * D : D;
            const float *xin = k == 0 ? qs : hcur + (k - 1) * kMaxD;
            const int64_t row = ((int64_t)k * T + t) * B + b;
            if (tid < 4 * D) {
                const float *wi = a.w.w_ih[k] + (int64_t)tid * in, *wh = a.w.w_hh[k] + (int64_t)tid * D;
                float z = a.w.b_ih[k][tid] + a.w.b_hh[k][tid];
                for (int i = 0; i < in; ++i) z = fmaf(wi[i], xin[i], z);
                for (int i = 0; i < D; ++i) z = fmaf(wh[i], hcur[k * kMaxD + i], z);
                const float g = (tid >= 2 * D && tid < 3 * D) ? tanhf(z) : sigm(z);
                gs[tid] = g;
                sv[a.s.gates + row * 4 * D + tid] = g;
            }
            __syncthreads();
            if (tid < D) {
                const float gi = gs[tid], gf = gs[D + tid], gg = gs[2 * D + tid], go = gs[3 * D + tid];
                const float c = fmaf(gf, ccur[k * kMaxD + tid], gi * gg);
                const float hh = go * tanhf(c);
                ccur[k * kMaxD + tid] = c;
                hcur[k * kMaxD + tid] = hh;
                sv[a.s.cst + row * D + tid] = c;
                sv[a.s.hst + row * D + tid] = hh;
            }
            __syncthreads();
        }
        const float *q = hcur + (Lr - 1) * kMaxD;
        float *alpha = sv + a.s.alpha + (int64_t)t * cap;
        float r_own = 0.f;
        if (n > 0) {                                          // (block-uniform) an empty graph reads out r = 0
            float mloc = -INFINITY;
            for (int v = n0 + tid; v < n1; v += kThreads) {
                float e = 0.f;
                for (int j = 0; j < D; ++j) e = fmaf(xL[(int64_t)v * D + j], q[j], e);
                alpha[v] = e;
                mloc = fmaxf(mloc, e);
            }
            const float m = block_max(mloc, red);
            float sloc = 0.f;
            for (int v = n0 + tid; v < n1; v += kThreads) sloc += expf(alpha[v] - m);
            const float ssum = block_sum(sloc, red);
            for (int v = n0 + tid; v < n1; v += kThreads) alpha[v] = expf(alpha[v] - m) / ssum;
            __syncthreads();
            if (lane < D) {
                float acc = 0.f;
                for (int v = n0 + wave; v < n1; v += kWaves) acc = fmaf(alpha[v], xL[(int64_t)v * D + lane], acc);
                red[wave * 64 + lane] = acc;
            }
            __syncthreads();
            if (tid < D) r_own = ((red[tid] + red[64 + tid]) + red[128 + tid]) + red[192 + tid];
        }
        __syncthreads();
        if (tid < D) {
            qs[tid] = q[tid];
            qs[D + tid] = r_own;
            float *qo = sv + a.s.qstar + ((int64_t)(t + 1) * B + b) * 2 * D;
            qo[tid] = q[tid];
            qo[D + tid] = r_own;
        }
        __syncthreads();
    }

    // ---- lin_readout: Linear(2D, D) -> ReLU -> Linear(D, out); F.normalize
    if (tid < D) {
        const float *w0 = a.w.ro0_w + (int64_t)tid * 2 * D;
        float z = a.w.ro0_b[tid];
        for (int i = 0; i < 2 * D; ++i) z = fmaf(w0[i], qs[i], z);
        sv[a.s.hid + (int64_t)b * D + tid] = z;
        gs[tid] = fmaxf(z, 0.f);
    }
    __syncthreads();
    if (wave == 0) {
        float o = 0.f;
        if (lane < d.Dout) {
            const float *w2 = a.w.ro2_w + (int64_t)lane * D;
            o = a.w.ro2_b[lane];
            for (int j = 0; j < D; ++j) o = fmaf(w2[j], gs[j], o);
            sv[a.s.opre + (int64_t)b * d.Dout + lane] = o;
        }
        float y = o;
        if (d.norm) {
            const float nrm = sqrtf(wave_sum(o * o));
            y = o / fmaxf(nrm, d.eps);
        }
        if (lane < d.Dout) a.out[(int64_t)b * d.Dout + lane] = y;
    }
}

// =====================================================================================================================
__global__ __launch_bounds__(kThreads) void gat_backward_kernel(BwdArgs a)
{
    TRAIN_STEP_WAVE_PRIORITY();
    __shared__ float Ws[64 * kLdw];
    __shared__ float tile[kWaves * 16 * kLdw];
    __shared__ float al[64], ar[64];
    __shared__ float dq[2 * kMaxD], dhin[2 * kMaxD], dhn[kMaxLr * kMaxD], dcn[kMaxLr * kMaxD], dzs[4 * kMaxD], qt[kMaxD],
        red[4 * 64];
    const Dims &d = a.d;
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = a.node_off[b], n1 = a.node_off[b + 1], n = n1 - n0;
    const int D = d.D, H = d.H, F = d.F, cap = d.cap, B = d.B, T = d.T, Lr = d.Lr;
    const float *sv = a.sv;
    float *ws = a.ws;
    float *dcur = ws + a.k.dcur;
    for (int e = tid; e < n * D; e += kThreads) dcur[(int64_t)n0 * D + e] = 0.f;

    // ---- F.normalize and lin_readout
    if (wave == 0) {
        const float o = lane < d.Dout ? sv[a.s.opre + (int64_t)b * d.Dout + lane] : 0.f;
        const float dy = lane < d.Dout ? a.dout[(int64_t)b * d.Dout + lane] : 0.f;
        float dO = dy;
        if (d.norm) {
            const float nrm = sqrtf(wave_sum(o * o));
            if (nrm > d.eps) {
                const float y = o / nrm;
                dO = (dy - y * wave_sum(dy * y)) / nrm;
            } else {
                dO = dy / d.eps;
            }
        }
        if (lane < d.Dout) ws[a.k.dz2 + (int64_t)b * d.Dout + lane] = dO;
        red[lane] = dO;
    }
    __syncthreads();
    if (tid < D) {
        float s = 0.f;
        for (int o = 0; o < d.Dout; ++o) s = fmaf(a.w.ro2_w[(int64_t)o * D + tid], red[o], s);
        const float dh = sv[a.s.hid + (int64_t)b * D + tid] > 0.f ? s : 0.f;
        ws[a.k.dhid + (int64_t)b * D + tid] = dh;
        dzs[tid] = dh;
    }
    __syncthreads();
    if (tid < 2 * D) {
        float s = 0.f;
        for (int j = 0; j < D; ++j) s = fmaf(a.w.ro0_w[(int64_t)j * 2 * D + tid], dzs[j], s);
        dq[tid] = s;
    }
    for (int i = tid; i < Lr * kMaxD; i += kThreads) { dhn[i] = 0.f; dcn[i] = 0.f; }
    __syncthreads();

    // ---- Set2Set, backwards through the T iterations
    const float *xL = sv + a.s.rst + (int64_t)(d.L - 1) * cap * D;
    // per-node scratch until the GAT layers: entry v * H of the cvh rows (a node's OWN row -- the other workgroups may
    // already be writing cvh of their nodes)
    float *tmp = ws + a.k.cvh;
    for (int t = T - 1; t >= 0; --t) {
        const float *alpha = sv + a.s.alpha + (int64_t)t * cap;
        if (tid < D) qt[tid] = sv[a.s.qstar + ((int64_t)(t + 1) * B + b) * 2 * D + tid];
        __syncthreads();
        float dqa = 0.f;
        if (n > 0) {                                          // (block-uniform)
            const float *dr = dq + D;
            float sloc = 0.f;
            for (int v = n0 + tid; v < n1; v += kThreads) {
                float da = 0.f;
                for (int j = 0; j < D; ++j) da = fmaf(dr[j], xL[(int64_t)v * D + j], da);
                tmp[(int64_t)v * H] = da;
                sloc = fmaf(alpha[v], da, sloc);
            }
            const float S = block_sum(sloc, red);
            for (int v = n0 + tid; v < n1; v += kThreads) tmp[(int64_t)v * H] = alpha[v] * (tmp[(int64_t)v * H] - S);
            __syncthreads();
            if (lane < D) {
                float acc = 0.f;
                const float drj = dr[lane], qj = qt[lane];
                for (int v = n0 + wave; v < n1; v += kWaves) {
                    const float de = tmp[(int64_t)v * H], x = xL[(int64_t)v * D + lane];
                    dcur[(int64_t)v * D + lane] += fmaf(alpha[v], drj, de * qj);
                    acc = fmaf(de, x, acc);
                }
                red[wave * 64 + lane] = acc;
            }
            __syncthreads();
            if (tid < D) dqa = ((red[tid] + red[64 + tid]) + red[128 + tid]) + red[192 + tid];
        }
        __syncthreads();
        if (tid < D) dhin[tid] = dq[tid] + dqa;
        __syncthreads();
        for (int k = Lr - 1; k >= 0; --k) {
            const int64_t row = ((int64_t)k * T + t) * B + b;
            if (tid < D) {
                const float *g = sv + a.s.gates + row * 4 * D;
                const float gi = g[tid], gf = g[D + tid], gg = g[2 * D + tid], go = g[3 * D + tid];
                const float c = sv[a.s.cst + row * D + tid];
                const float cprev = t > 0 ? sv[a.s.cst + (row - B) * D + tid] : 0.f;
                const float dh = dhin[tid] + dhn[k * kMaxD + tid];
                const float tc = tanhf(c);
                const float dO = dh * tc;
                const float dc = dcn[k * kMaxD + tid] + dh * go * (1.f - tc * tc);
                dcn[k * kMaxD + tid] = dc * gf;
                dzs[tid] = dc * gg * gi * (1.f - gi);
                dzs[D + tid] = dc * cprev * gf * (1.f - gf);
                dzs[2 * D + tid] = dc * gi * (1.f - gg * gg);
                dzs[3 * D + tid] = dO * go * (1.f - go);
            }
            __syncthreads();
            const int in = k == 0 ? 2 * D : D;
            if (tid < 4 * D) ws[a.k.dz + row * 4 * D + tid] = dzs[tid];
            float dx = 0.f;
            if (tid < in) {
                for (int g = 0; g < 4 * D; ++g) dx = fmaf(a.w.w_ih[k][(int64_t)g * in + tid], dzs[g], dx);
            }
            float dhp = 0.f;
            const int i2 = tid - 2 * kMaxD;
            if (i2 >= 0 && i2 < D) {
                for (int g = 0; g < 4 * D; ++g) dhp = fmaf(a.w.w_hh[k][(int64_t)g * D + i2], dzs[g], dhp);
            }
            __syncthreads();
            if (tid < in) {
                if (k > 0) dhin[tid] = dx;
                else dq[tid] = dx;                            // d q*_t: the previous iteration's [q, r]
            }
            if (i2 >= 0 && i2 < D) dhn[k * kMaxD + i2] = dhp;
            __syncthreads();
        }
    }

    // ---- the GAT layers, last to first.  dcur = d(layer output)
    float *drst = ws + a.k.drst, *cvh = ws + a.k.cvh;
    for (int l = d.L - 1; l >= 0; --l) {
        const int Kin = l == 0 ? d.K0 : D;
        const float *ft = sv + a.s.ft + (int64_t)l * cap * D, *rst = sv + a.s.rst + (int64_t)l * cap * D;
        const float *el = sv + a.s.el + (int64_t)l * cap * H, *er = sv + a.s.er + (int64_t)l * cap * H;
        const float *lse = sv + a.s.lse + (int64_t)l * cap * H;
        float *dft = ws + a.k.dft + (int64_t)l * cap * D;
        float *del = ws + a.k.del + (int64_t)l * cap * H, *der = ws + a.k.der + (int64_t)l * cap * H;
        stage_layer(a.w.fc[l], a.w.attn_l[l], a.w.attn_r[l], D, Kin, Ws, al, ar);
        float *scr = tile + wave * 16 * kLdw;                 // [256] per wave
        // phase 1: drst = dcur * activation'; c[v, h] = <drst_v, rst_v> per head
        for (int v = n0 + wave; v < n1; v += kWaves) {
            float p = 0.f;
            if (lane < D) {
                const float r = rst[(int64_t)v * D + lane];
                float dd = dcur[(int64_t)v * D + lane];
                if (l < d.L - 1 && !(r > 0.f)) dd *= 0.01f;   // F.leaky_relu between layers
                drst[(int64_t)v * D + lane] = dd;
                p = dd * r;
            }
            scr[lane] = p;
            wave_sync();
            if (lane < H) {
                float c = 0.f;
                for (int f = 0; f < F; ++f) c += scr[lane * F + f];
                cvh[(int64_t)v * H + lane] = c;
            }
            wave_sync();
        }
        __syncthreads();
        // phase 2: per node n: der (n as destination), del and the aggregation part of dft (n as source: gathered over
        // n's own row, which by symmetry lists n's out-neighbours)
        const int S = 64 / H, hs = lane % H, slot = lane / H;
        for (int nn = n0 + wave; nn < n1; nn += kWaves) {
            const int e0 = a.row_ptr[nn], e1 = a.row_ptr[nn + 1];
            float dr_acc = 0.f, dl_acc = 0.f;
            if (slot < S) {
                const float el_n = el[(int64_t)nn * H + hs], er_n = er[(int64_t)nn * H + hs];
                const float lse_n = lse[(int64_t)nn * H + hs], c_n = cvh[(int64_t)nn * H + hs];
                const float *drn = drst + (int64_t)nn * D + hs * F, *ftn = ft + (int64_t)nn * D + hs * F;
                for (int e = e0 + slot; e < e1; e += S) {
                    const int u = a.col_idx[e];
                    const float *fu = ft + (int64_t)u * D + hs * F, *du = drst + (int64_t)u * D + hs * F;
                    float da1 = 0.f, da2 = 0.f;
                    for (int f = 0; f < F; ++f) {
                        da1 = fmaf(drn[f], fu[f], da1);
                        da2 = fmaf(du[f], ftn[f], da2);
                    }
                    const float s1 = el[(int64_t)u * H + hs] + er_n;            // edge u -> n
                    const float a1 = expf(lrelu(s1, 0.2f) - lse_n);
                    dr_acc = fmaf(a1 * (da1 - c_n), s1 > 0.f ? 1.f : 0.2f, dr_acc);
                    const float s2 = el_n + er[(int64_t)u * H + hs];            // edge n -> u
                    const float a2 = expf(lrelu(s2, 0.2f) - lse[(int64_t)u * H + hs]);
                    dl_acc = fmaf(a2 * (da2 - cvh[(int64_t)u * H + hs]), s2 > 0.f ? 1.f : 0.2f, dl_acc);
                }
            }
            scr[lane] = dr_acc;
            scr[64 + lane] = dl_acc;
            wave_sync();
            if (lane < H) {
                float sr = 0.f, sl = 0.f;
                for (int s = 0; s < S; ++s) { sr += scr[s * H + lane]; sl += scr[64 + s * H + lane]; }
                der[(int64_t)nn * H + lane] = sr;
                del[(int64_t)nn * H + lane] = sl;
                scr[128 + lane] = sr;
                scr[192 + lane] = sl;
            }
            wave_sync();
            if (lane < D) {
                const int h = lane / F;
                const float el_n = el[(int64_t)nn * H + h];
                float acc = 0.f;
                int e = e0;
                for (; e + kEdgeJ <= e1; e += kEdgeJ) {           // (loads of kEdgeJ edges in flight, as in the forward)
                    int u[kEdgeJ];
                    float eu[kEdgeJ], lu[kEdgeJ], du[kEdgeJ];
#pragma unroll
                    for (int i = 0; i < kEdgeJ; ++i) u[i] = a.col_idx[e + i];
#pragma unroll
                    for (int i = 0; i < kEdgeJ; ++i) {
                        eu[i] = er[(int64_t)u[i] * H + h];
                        lu[i] = lse[(int64_t)u[i] * H + h];
                        du[i] = drst[(int64_t)u[i] * D + lane];
                    }
#pragma unroll
                    for (int i = 0; i < kEdgeJ; ++i) acc = fmaf(expf(lrelu(el_n + eu[i], 0.2f) - lu[i]), du[i], acc);
                }
                for (; e < e1; ++e) {
                    const int u = a.col_idx[e];
                    const float s2 = el_n + er[(int64_t)u * H + h];
                    const float a2 = expf(lrelu(s2, 0.2f) - lse[(int64_t)u * H + h]);
                    acc = fmaf(a2, drst[(int64_t)u * D + lane], acc);
                }
                dft[(int64_t)nn * D + lane] = fmaf(scr[192 + h], al[lane], fmaf(scr[128 + h], ar[lane], acc));
            }
            wave_sync();
        }
        __syncthreads();
        // phase 3: d(input) = dft W on the MFMA -> dcur (the previous layer's output) or dx0
        float *dst = l == 0 ? ws + a.k.dx0 : dcur;
        const int ldd = l == 0 ? d.K0 : D;
        const int nb = (Kin + 15) >> 4;
        for (int rb = wave; rb * 16 < n; rb += kWaves) {
            const int r0 = n0 + rb * 16;
            f32x4 acc[4];
            mfma_rows16<true>(dft, D, D, false, r0, n1, Ws, nb, acc);
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                const int c = 16 * cb + (lane & 15);
                if (cb < nb && c < Kin)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int v = r0 + (lane >> 4) * 4 + r;
                        if (v < n1) dst[(int64_t)v * ldd + c] = acc[cb][r];
                    }
            }
        }
        __syncthreads();
    }
}

// =====================================================================================================================
// blockIdx = (chunk, job, output tile of 64 x 64)
__global__ __launch_bounds__(kThreads) void gat_wgrad_kernel(WArgs a)
{
    TRAIN_STEP_WAVE_PRIORITY();
    __shared__ float Zs[kRowBlk * 64];
    __shared__ float Xs[kRowBlk * kLdw];
    const WJob &j = a.job[blockIdx.y];
    const int c = (int)blockIdx.x, tile = (int)blockIdx.z, tid = (int)threadIdx.x;
    if (c >= j.chunks) return;
    const int total = j.rows >= 0 ? j.rows : a.node_off[a.B];
    const int per = (total + j.chunks - 1) / j.chunks;
    const int r0 = min(c * per, total), r1 = min(r0 + per, total);
    const int64_t size = job_size(j);
    float *part = j.part + (int64_t)c * size;
    if (j.type == kJobEmb) {                                  // d emb[clamp(deg)][col] += dx0[r][pos + col]
        if (tile != 0) return;
        if (tid < a.emb) {
            for (int e = 0; e <= a.maxdeg; ++e) part[(int64_t)e * a.emb + tid] = 0.f;
            for (int r = r0; r < r1; ++r) {
                const int deg = (a.row_ptr[r + 1] - a.row_ptr[r]) * a.mult;
                part[(int64_t)min(deg, a.maxdeg) * a.emb + tid] += j.dz[(int64_t)r * a.K0 + a.pos + tid];
            }
        }
        return;
    }
    if (j.type == kJobDiag) {                                 // attn_l / attn_r: out[k] = sum_r dz[r][k / F] x[r][k]
        if (tile != 0) return;
        if (tid < j.K) {
            float s = 0.f;
            for (int r = r0; r < r1; ++r) s = fmaf(j.dz[(int64_t)r * j.ldz + tid / j.F], j.x[(int64_t)r * j.ldx + tid], s);
            part[tid] = s;
        }
        return;
    }
    const int kt = (j.K + 63) >> 6, mt = (j.M + 63) >> 6;
    if (tile >= mt * kt) return;
    const int m0 = (tile / kt) * 64, k0 = (tile % kt) * 64;
    const int mm = tid >> 2, kk0 = (tid & 3) * 16;
    float acc[16], bacc = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
    for (int rb = r0; rb < r1; rb += kRowBlk) {
        for (int e = tid; e < kRowBlk * 64; e += kThreads) {
            const int rr = e >> 6, col = e & 63, r = rb + rr;
            const bool live = r < r1;
            Zs[rr * 64 + col] = live && m0 + col < j.M ? j.dz[(int64_t)r * j.ldz + m0 + col] : 0.f;
            float x = live && k0 + col < j.K ? j.x[(int64_t)r * j.ldx + k0 + col] : 0.f;
            if (j.xact == 1) x = lrelu(x, 0.01f);
            else if (j.xact == 2) x = fmaxf(x, 0.f);
            Xs[rr * kLdw + col] = x;
        }
        __syncthreads();
        for (int rr = 0; rr < kRowBlk; ++rr) {
            const float z = Zs[rr * 64 + mm];
            bacc += z;
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[q] = fmaf(z, Xs[rr * kLdw + kk0 + q], acc[q]);
        }
        __syncthreads();
    }
    const int m = m0 + mm;
    if (m < j.M) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int k = k0 + kk0 + q;
            if (k < j.K) part[(int64_t)m * j.K + k] = acc[q];
        }
        if (j.bias && k0 == 0 && (tid & 3) == 0) part[(int64_t)j.M * j.K + m] = bacc;
    }
}

// blockIdx = (element block, job): the chunks' partials summed in order
__global__ __launch_bounds__(kThreads) void gat_reduce_kernel(RArgs a)
{
    TRAIN_STEP_WAVE_PRIORITY();
    const RJob &j = a.job[blockIdx.y];
    const int e = (int)blockIdx.x * kThreads + (int)threadIdx.x;
    if (e >= j.size) return;
    float s = 0.f;
    for (int c = 0; c < j.chunks; ++c) s += j.part[(int64_t)c * j.size + e];
    float *dst;
    if (e < j.mk) {
        dst = j.dst + e;
    } else {
        dst = j.dst_b + (e - j.mk);
        if (j.dst_b2) {
            float *d2 = j.dst_b2 + (e - j.mk);
            *d2 = a.accumulate ? *d2 + s : s;
        }
    }
    *dst = a.accumulate ? *dst + s : s;
}

// ---------------------------------------------------------------------------------------------------------------------
int make_dims(const char *who, const gcc_gat_weights *w, int32_t node_cap, int32_t B, Dims *d)
{
    if (!w) {
        snprintf(g_err, kErrLen, "%s: NULL weights", who);
        return -1;
    }
    const int K0 = w->pos_dim + w->deg_emb_dim + 1;
    if (w->hidden < 1 || w->hidden > kMaxD || w->heads < 1 || w->hidden % w->heads != 0) {
        snprintf(g_err, kErrLen, "%s: hidden %d with %d heads (supported: hidden <= %d, hidden %% heads == 0)", who, w->hidden,
                 w->heads, kMaxD);
        return -2;
    }
    if (w->out_dim < 1 || w->out_dim > kMaxD || K0 > kMaxD || w->pos_dim < 0 || w->deg_emb_dim < 0 || w->max_degree < 0) {
        snprintf(g_err, kErrLen, "%s: output %d / input %d (supported: both <= %d)", who, w->out_dim, K0, kMaxD);
        return -3;
    }
    if (w->num_layers < 1 || w->num_layers > kMaxL || w->s2s_layers < 1 || w->s2s_layers > kMaxLr || w->s2s_iters < 1) {
        snprintf(g_err, kErrLen, "%s: %d GAT layers / %d LSTM layers / %d Set2Set steps (supported: 1..%d / 1..%d / >= 1)", who,
                 w->num_layers, w->s2s_layers, w->s2s_iters, kMaxL, kMaxLr);
        return -4;
    }
    if (node_cap < 1 || B < 1) {
        snprintf(g_err, kErrLen, "%s: node_cap %d / batch size %d", who, node_cap, B);
        return -5;
    }
    *d = Dims{w->num_layers, w->hidden, w->heads, w->hidden / w->heads, K0, w->out_dim, w->s2s_iters, w->s2s_layers,
              w->pos_dim, w->deg_emb_dim, w->max_degree, node_cap, B, w->normalize ? 1 : 0, w->norm_eps};
    return 0;
}

int check_weights(const char *who, const gcc_gat_weights *w)
{
    bool ok = w->degree_embedding && w->ro0_w && w->ro0_b && w->ro2_w && w->ro2_b;
    for (int l = 0; l < w->num_layers; ++l) ok = ok && w->fc[l] && w->attn_l[l] && w->attn_r[l];
    for (int k = 0; k < w->s2s_layers; ++k) ok = ok && w->w_ih[k] && w->w_hh[k] && w->b_ih[k] && w->b_hh[k];
    if (!ok) snprintf(g_err, kErrLen, "%s: a weight pointer is NULL", who);
    return ok ? 0 : -1;
}

int check_pass(const char *who, const gcc_gat_pass *p, const Dims &d)
{
    const char *missing = !p ? "the pass itself"
                          : !p->node_off ? "node_off"
                          : !p->row_ptr ? "row_ptr"
                          : !p->col_idx ? "col_idx (an edge-free batch still passes one placeholder element)"
                          : !p->saved ? "saved"
                          : !p->out ? "out"
                          : (d.pos > 0 && !p->pos) ? "pos" : nullptr;
    if (missing) {
        snprintf(g_err, kErrLen, "%s: NULL pass member: %s", who, missing);
        return -1;
    }
    return 0;
}

// the weight-gradient jobs of a backward and the floats of their partials
int gat_jobs(const Dims &d, const Saved &s, const Work &k, const float *sv, float *ws, const gcc_gat_grads *g, WArgs *wa,
             RArgs *ra, int64_t *part_floats)
{
    int nj = 0;
    int64_t off = k.part;
    auto add = [&](WJob j, float *dst, float *dst_b, float *dst_b2) {
        j.part = ws ? ws + off : nullptr;
        const int64_t size = job_size(j);
        if (wa) wa->job[nj] = j;
        if (ra) ra->job[nj] = RJob{j.part, dst, dst_b, dst_b2, (int32_t)size, j.type == kJobGemm ? j.M * j.K : (int32_t)size,
                                  j.chunks, 0};
        off += size * j.chunks;
        ++nj;
    };
    const int64_t cap = d.cap, B = d.B, D = d.D;
    auto S = [&](int64_t o) { return sv ? sv + o : nullptr; };
    auto W = [&](int64_t o) { return ws ? ws + o : nullptr; };
    for (int l = 0; l < d.L; ++l) {
        const int Kin = l == 0 ? d.K0 : d.D;
        WJob j = {};
        j.type = kJobGemm; j.dz = W(k.dft + l * cap * D); j.ldz = d.D;
        j.x = l == 0 ? S(s.x0) : S(s.rst + (l - 1) * cap * D); j.ldx = Kin; j.xact = l == 0 ? 0 : 1;
        j.M = d.D; j.K = Kin; j.rows = -1; j.chunks = kChunksNode;
        add(j, g ? g->fc[l] : nullptr, nullptr, nullptr);
        WJob jl = {};
        jl.type = kJobDiag; jl.dz = W(k.del + l * cap * d.H); jl.ldz = d.H; jl.x = S(s.ft + l * cap * D); jl.ldx = d.D;
        jl.M = 1; jl.K = d.D; jl.F = d.F; jl.rows = -1; jl.chunks = kChunksNode;
        add(jl, g ? g->attn_l[l] : nullptr, nullptr, nullptr);
        WJob jr = jl;
        jr.dz = W(k.der + l * cap * d.H);
        add(jr, g ? g->attn_r[l] : nullptr, nullptr, nullptr);
    }
    for (int q = 0; q < d.Lr; ++q) {
        const int64_t TB = (int64_t)d.T * B;
        WJob j = {};
        j.type = kJobGemm; j.dz = W(k.dz + q * TB * 4 * D); j.ldz = 4 * d.D;
        j.x = q == 0 ? S(s.qstar) : S(s.hst + (q - 1) * TB * D); j.ldx = q == 0 ? 2 * d.D : d.D;
        j.M = 4 * d.D; j.K = j.ldx; j.rows = (int32_t)TB; j.chunks = kChunksSeq; j.bias = 1;
        add(j, g ? g->w_ih[q] : nullptr, g ? g->b_ih[q] : nullptr, g ? g->b_hh[q] : nullptr);
        WJob jh = {};                                         // h_prev of step t is h of step t - 1 (zero at t = 0)
        jh.type = kJobGemm; jh.dz = W(k.dz + q * TB * 4 * D + B * 4 * D); jh.ldz = 4 * d.D;
        jh.x = S(s.hst + q * TB * D); jh.ldx = d.D;
        jh.M = 4 * d.D; jh.K = d.D; jh.rows = (int32_t)((d.T - 1) * B); jh.chunks = kChunksSeq;
        add(jh, g ? g->w_hh[q] : nullptr, nullptr, nullptr);
    }
    {
        WJob j = {};
        j.type = kJobGemm; j.dz = W(k.dhid); j.ldz = d.D; j.x = S(s.qstar + (int64_t)d.T * B * 2 * D); j.ldx = 2 * d.D;
        j.M = d.D; j.K = 2 * d.D; j.rows = d.B; j.chunks = kChunksGraph; j.bias = 1;
        add(j, g ? g->ro0_w : nullptr, g ? g->ro0_b : nullptr, nullptr);
        WJob j2 = {};
        j2.type = kJobGemm; j2.dz = W(k.dz2); j2.ldz = d.Dout; j2.x = S(s.hid); j2.ldx = d.D; j2.xact = 2;
        j2.M = d.Dout; j2.K = d.D; j2.rows = d.B; j2.chunks = kChunksGraph; j2.bias = 1;
        add(j2, g ? g->ro2_w : nullptr, g ? g->ro2_b : nullptr, nullptr);
        WJob je = {};
        je.type = kJobEmb; je.dz = W(k.dx0); je.M = d.maxdeg + 1; je.K = d.emb; je.rows = -1; je.chunks = kChunksNode;
        add(je, g ? g->degree_embedding : nullptr, nullptr, nullptr);
    }
    *part_floats = off - k.part;
    return nj;
}

}  // namespace

extern "C" {

int64_t gcc_gat_saved_floats(const gcc_gat_weights *w, int32_t node_cap, int32_t batch_size)
{
    Dims d;
    const int rc = make_dims("gcc_gat_saved_floats", w, node_cap, batch_size, &d);
    return rc ? rc : saved_layout(d).total;
}

int64_t gcc_gat_backward_workspace_bytes(const gcc_gat_weights *w, int32_t node_cap, int32_t batch_size)
{
    Dims d;
    const int rc = make_dims("gcc_gat_backward_workspace_bytes", w, node_cap, batch_size, &d);
    if (rc) return rc;
    int64_t part = 0;
    const Work k = work_layout(d);
    gat_jobs(d, saved_layout(d), k, nullptr, nullptr, nullptr, nullptr, nullptr, &part);
    return (int64_t)sizeof(float) * (k.total + part);
}

int32_t gcc_gat_forward(const gcc_gat_pass *p, const gcc_gat_weights *w, void *stream)
{
    Dims d;
    int rc = make_dims("gcc_gat_forward", w, p ? p->node_cap : 0, p ? p->batch_size : 0, &d);
    if (rc) return rc;
    if ((rc = check_weights("gcc_gat_forward", w)) || (rc = check_pass("gcc_gat_forward", p, d))) return rc;
    FwdArgs a = {};
    a.w = *w;
    a.node_off = p->node_off; a.row_ptr = p->row_ptr; a.col_idx = p->col_idx; a.seed_local = p->seed_local; a.pos = p->pos;
    a.sv = p->saved; a.out = p->out;
    a.mult = p->edge_multiplicity > 1 ? p->edge_multiplicity : 1;
    a.d = d;
    a.s = saved_layout(d);
    hipLaunchKernelGGL(gat_forward_kernel, dim3(d.B), dim3(kThreads), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

int32_t gcc_gat_backward(const gcc_gat_pass *p, const gcc_gat_weights *w, const float *dout, const gcc_gat_grads *g,
                         int32_t accumulate, void *workspace, int64_t workspace_bytes, void *stream)
{
    Dims d;
    int rc = make_dims("gcc_gat_backward", w, p ? p->node_cap : 0, p ? p->batch_size : 0, &d);
    if (rc) return rc;
    if ((rc = check_weights("gcc_gat_backward", w)) || (rc = check_pass("gcc_gat_backward", p, d))) return rc;
    bool ok = dout && g && workspace && g->degree_embedding && g->ro0_w && g->ro0_b && g->ro2_w && g->ro2_b;
    for (int l = 0; ok && l < d.L; ++l) ok = g->fc[l] && g->attn_l[l] && g->attn_r[l];
    for (int k = 0; ok && k < d.Lr; ++k) ok = g->w_ih[k] && g->w_hh[k] && g->b_ih[k] && g->b_hh[k];
    if (!ok) {
        snprintf(g_err, kErrLen, "gcc_gat_backward: NULL dout / gradient / workspace");
        return -1;
    }
    const Saved s = saved_layout(d);
    const Work k = work_layout(d);
    int64_t part = 0;
    float *ws = (float *)workspace;
    WArgs wa = {};
    RArgs ra = {};
    const int nj = gat_jobs(d, s, k, p->saved, ws, g, &wa, &ra, &part);
    if ((int64_t)sizeof(float) * (k.total + part) > workspace_bytes) {
        snprintf(g_err, kErrLen, "gcc_gat_backward: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                 (long long)(sizeof(float) * (k.total + part)));
        return -6;
    }
    BwdArgs a = {};
    a.w = *w;
    a.node_off = p->node_off; a.row_ptr = p->row_ptr; a.col_idx = p->col_idx;
    a.sv = p->saved; a.dout = dout; a.ws = ws;
    a.d = d; a.s = s; a.k = k;
    hipLaunchKernelGGL(gat_backward_kernel, dim3(d.B), dim3(kThreads), 0, (hipStream_t)stream, a);
    wa.node_off = p->node_off; wa.row_ptr = p->row_ptr; wa.B = d.B;
    wa.mult = p->edge_multiplicity > 1 ? p->edge_multiplicity : 1;
    wa.maxdeg = d.maxdeg; wa.emb = d.emb; wa.pos = d.pos; wa.K0 = d.K0;
    int tiles = 1, maxsize = 1;
    for (int i = 0; i < nj; ++i) {
        const int t = ((wa.job[i].M + 63) / 64) * ((wa.job[i].K + 63) / 64);
        if (wa.job[i].type == kJobGemm && t > tiles) tiles = t;
        if (ra.job[i].size > maxsize) maxsize = ra.job[i].size;
    }
    hipLaunchKernelGGL(gat_wgrad_kernel, dim3(kChunksNode, nj, tiles), dim3(kThreads), 0, (hipStream_t)stream, wa);
    ra.accumulate = accumulate ? 1 : 0;
    hipLaunchKernelGGL(gat_reduce_kernel, dim3((maxsize + kThreads - 1) / kThreads, nj), dim3(kThreads), 0, (hipStream_t)stream,
                       ra);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

}  // extern "C"
