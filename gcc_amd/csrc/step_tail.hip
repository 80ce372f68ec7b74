// gcc_amd/csrc/step_tail.hip -- the tail of a training step over flat buffers: queue enqueue, gradient clip, optimizer update,
// EMA copy, meters, and the per-step scalars of a replayed step (gfx950).
//
// Replaces, in the reference's train.py: clip_grad_norm_ (:409) / clip_grad_value_ (:232-246), optimizer.step() of
// torch.optim.Adam / SGD / Adagrad (:417, :658-679), moment_update (:169-172), the loss / prob / gnorm / graph-size meters
// (:418-428) and the lr schedule's per-step values; and MemoryMoCo's index_copy_ of the new keys (memory_moco.py:57-62).
//
//   queue_enqueue_kernel      keys -> queue rows (index + i) mod K; the ring pointer by value or from gcc_step_scalars.
//   ema_kernel                ema = ema * m + (1 - m) * p over a flat buffer (the api path; the fused steps use the tail below).
//   gradnorm_kernel           sum of squares of the flat gradient in double, 32 partials added up in index order.
//   tail_norm_kernel<rule>    ONE launch: norm -> clip coefficient -> update (tail_update<rule>: Adam 0, GCC_OPT_SGD,
//       GCC_OPT_ADAGRAD) -> EMA copy past the live prefix -> one step of the meters by thread 0 of workgroup 0.  Adam only
//       (gcc_adam_ema_enqueue_step_scalars): the sum of squares from the backward's partials, the enqueue as extra workgroups.
//   tail_value_kernel<rule>   clip_grad_value_ + the same update: the fine-tuning tail, one launch, no norm pass.
//   step_meters_kernel        the meters as a launch of their own (the data-parallel and api paths).
//   step_scalars*_kernel      {lr, bias corrections, ring pointer, dropout key} into their device struct.
#include "encoder_common.h"      // F4 / ld4 / st4, kThreads

#include <math.h>

namespace {

constexpr int D = GCC_NCE_DIM;    // 64: a queue row
constexpr int kAdam = 0;          // the internal rule next to GCC_OPT_SGD (1) / GCC_OPT_ADAGRAD (2); not reachable through gcc_opt_*

__global__ __launch_bounds__(kThreads) void queue_enqueue_kernel(float *mem, int K, const float *keys, int nkeys,
                                                                 int index, float *saved, const gcc_step_scalars *sc)
{
    TRAIN_STEP_WAVE_PRIORITY();
    if (sc) index = sc->enqueue_index % K;                    // replayed step: the ring pointer lives on the device
    const int gid = (int)blockIdx.x * kThreads + (int)threadIdx.x;
    const int i = gid >> 4, c4 = (gid & 15) * 4;
    if (i >= nkeys) return;
    const int row = (index + i) % K;                          // torch.fmod(out_ids + index, queueSize)
    if (saved) st4(saved + (int64_t)i * D + c4, ld4(mem + (int64_t)row * D + c4));
    st4(mem + (int64_t)row * D + c4, ld4(keys + (int64_t)i * D + c4));
}

__global__ __launch_bounds__(kThreads) void ema_kernel(float *ema, const float *p, int64_t n, float m)
{
    TRAIN_STEP_WAVE_PRIORITY();
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride)
        ema[i] = ema[i] * m + (1.f - m) * p[i];               // p2.mul_(m).add_(1 - m, p1)
}

// ---- clip_grad_norm_ + the update over one flat buffer (train.py:409,417)
constexpr int kNormBlocks = 32;
// sum of squares of the flat gradient: kNormBlocks partial sums; the workgroup that arrives last adds them up in index
// order (deterministic).  scratch: [0] = result, [1] = ticket (as int), [2 .. 2 + kNormBlocks) = partials.
__global__ __launch_bounds__(kThreads) void gradnorm_kernel(const float *g, int64_t n, double *scratch)
{
    TRAIN_STEP_WAVE_PRIORITY();
    static_assert(kNormBlocks <= 64, "the last workgroup adds the partials up with one wave");
    __shared__ double red[kThreads / 64];
    __shared__ int last;
    const int tid = (int)threadIdx.x;
    double s = 0.0;
    // 8 independent loads per round (clamped address, masked afterwards): one element per round was a dependent round
    // trip per element, ~12 in a row for the 100 k parameters of the GIN encoder
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t base = (int64_t)blockIdx.x * kThreads + tid; base < n; base += 8 * stride) {
        float x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int64_t i = base + u * stride; x[u] = g[i < n ? i : n - 1]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) if (base + u * stride < n) s += (double)x[u] * (double)x[u];
    }
    s = wave_sum(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int i = 0; i < kThreads / 64; ++i) t += red[i];
        scratch[2 + blockIdx.x] = t;
        device_fence();
        last = atomicAdd((int *)(scratch + 1), 1) == (int)gridDim.x - 1;
    }
    __syncthreads();
    if (last && tid < 64) {                                  // block-uniform; one wave: the partials in one round trip, fixed tree
        device_fence();
        const double v = tid < (int)gridDim.x ? load_fresh_f64(scratch + 2 + tid) : 0.0;
        const double tot = wave_sum(v);
        if (tid == 0) {
            scratch[0] = tot;
            *(int *)(scratch + 1) = 0;
        }
    }
}

// ---- the update rules.  ``lr``: the step's rate (Adagrad: its clr = lr / (1 + (t - 1) lr_decay), formed by the host in double
// as torch forms it); ``hyper``: SGD's momentum / Adagrad's eps; the rest is Adam's.
struct TailHyper { float wd, hyper, lr, bc1, bc2_sqrt, b1, b2, eps; };      // (what every rule reads comes first: the unused rest of a
                                                                            // kernel's arguments then costs the SGD / Adagrad kernels no registers)

// gc: the clipped gradient; s0 / s1: Adam's exp_avg / exp_avg_sq, SGD's momentum buffer, Adagrad's sum of squares (s1: Adam
// only) -> the new parameter.  o0 / o1: where the new state goes -- the arrays' elements themselves, so that Adam's two stores are
// issued in front of its sqrt / divisions (their registers are free by then).
template <int kRule>
__device__ __forceinline__ float tail_update(float gc, float p0, float s0, float s1, const TailHyper &h, float &o0, float &o1)
{
    const float gi = fmaf(h.wd, p0, gc);                       // weight_decay: grad = grad + wd * param (after the clip, as torch)
    if constexpr (kRule == kAdam) {
        const float mi = fmaf(h.b1, s0, (1.f - h.b1) * gi);
        const float vi = fmaf(h.b2, s1, (1.f - h.b2) * gi * gi);
        o0 = mi;
        o1 = vi;
        const float denom = sqrtf(vi) / h.bc2_sqrt + h.eps;
        return p0 - (h.lr / h.bc1) * (mi / denom);
    } else if constexpr (kRule == GCC_OPT_SGD) {
        const float bi = fmaf(h.hyper, s0, gi);                // buf.mul_(momentum).add_(grad); buf = 0 gives torch's first step
        o0 = bi;
        return fmaf(-h.lr, bi, p0);                            // param.add_(buf, alpha=-lr)
    } else {
        const float si = fmaf(gi, gi, s0);                     // state_sum.addcmul_(grad, grad)
        o0 = si;
        return p0 - h.lr * gi / (sqrtf(si) + h.hyper);         // param.addcdiv_(grad, sqrt(sum) + eps, value=-clr): 0 / eps = 0
    }
}

// train.py:418-428's meters, one step (called by one thread)
__device__ __forceinline__ void meters_add(double *acc, int32_t *mx, const float *loss, const float *prob, float gnorm,
                                           const int32_t *node_off_q, const int32_t *edge_off_q, const int32_t *node_off_k, int32_t B)
{
    const int32_t nq = node_off_q[B], nk = node_off_k[B], eq = edge_off_q[B];
    acc[0] += (double)loss[0];
    acc[1] += (double)prob[0];
    acc[2] += (double)gnorm;
    acc[3] += (double)nq + (double)nk;
    acc[4] += 1.0;
    mx[0] = nq > mx[0] ? nq : mx[0];
    mx[1] = eq > mx[1] ? eq : mx[1];
}

// optional extras of the clip-by-norm launch: the EMA copy of the parameters and the per-step meters
struct TailExtras {
    float *ema; int64_t n_ema; float ema_m;
    const gcc_step_scalars *sc;      // replayed step: lr and the bias corrections come from here
    double *acc; int32_t *mx; const float *loss, *prob; const int32_t *node_off_q, *edge_off_q, *node_off_k; int32_t B;
    // gcc_adam_ema_enqueue_step_scalars (Adam only): the sum of squares as per-workgroup partials of gin_grad_final_kernel
    // (instead of sumsq[0] of a gradnorm_kernel launch), and the queue's enqueue as workgroups >= tail_blocks of this launch
    const double *parts; int32_t nparts;
    float *q_mem; const float *q_keys; int32_t q_K, q_nkeys, tail_blocks;
};

// s1: Adam's second state array; the other rules issue no load or store for it
template <int kRule>
__global__ __launch_bounds__(kThreads) void tail_norm_kernel(float *p, float *g, float *s, int64_t n, TailHyper h,
                                                             float max_norm, float grad_scale, const double *sumsq,
                                                             float *grad_norm, TailExtras x, float *s1)
{
    constexpr bool kTwo = kRule == kAdam, kFold = kRule == kAdam;
    TRAIN_STEP_WAVE_PRIORITY();
    int nblk = (int)gridDim.x;
    if constexpr (kFold) {
        if (x.q_mem) nblk = x.tail_blocks;
        if ((int)blockIdx.x >= nblk) {                         // (block-uniform) queue_enqueue_kernel's rows, ring pointer from the device
            const int gid = ((int)blockIdx.x - nblk) * kThreads + (int)threadIdx.x;
            const int i = gid >> 4, c4 = (gid & 15) * 4;
            if (i >= x.q_nkeys) return;
            const int row = (x.sc->enqueue_index % x.q_K + i) % x.q_K;                 // torch.fmod(out_ids + index, queueSize)
            st4(x.q_mem + (int64_t)row * D + c4, ld4(x.q_keys + (int64_t)i * D + c4));
            return;
        }
    }
    // grad_scale: the 1 / world of a summed (all-reduced) gradient, folded in here instead of a launch of its own
    double ss = 0.0;
    double pv[4] = {0.0, 0.0, 0.0, 0.0};
    const bool parts = kFold && x.parts;
    if (parts) {                                               // (uniform) the partials: one round trip, with the first element's
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = (int)threadIdx.x + kThreads * u;
            pv[u] = x.parts[idx < x.nparts ? idx : x.nparts - 1];
        }
    } else {
        ss = sumsq[0];
    }
    if (x.sc) {                                                // (uniform: one scalar load, in flight with the rest)
        h.lr = x.sc->lr;
        if constexpr (kRule == kAdam) { h.bc1 = x.sc->bias_corr1; h.bc2_sqrt = x.sc->bias_corr2_sqrt; }
    }
    // this thread's first element rides in the same round trip as the norm
    const int64_t stride = (int64_t)nblk * kThreads, i0 = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t ic = i0 < n ? i0 : n - 1;
    float g0 = g[ic], p0 = p[ic], a0 = s[ic], b0 = 0.f;
    if constexpr (kTwo) b0 = s1[ic];
    const float e0 = x.ema ? x.ema[i0 < x.n_ema ? i0 : x.n_ema - 1] : 0.f;      // (block-uniform branch)
    if constexpr (kFold) {
        if (parts) {
            // every workgroup adds ALL partials up in the same fixed order (thread t: partials t, t + 256, ..; wave tree; waves 0..3):
            // the same bits in every workgroup, no ticket and no last-arrival pass
            __shared__ double red[kThreads / 64];
            double t = 0.0;
#pragma unroll
            for (int u = 0; u < 4; ++u) if ((int)threadIdx.x + kThreads * u < x.nparts) t += pv[u];
            for (int idx = (int)threadIdx.x + 4 * kThreads; idx < x.nparts; idx += kThreads) t += x.parts[idx];
            t = wave_sum(t);
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
            __syncthreads();
            ss = (red[0] + red[1]) + (red[2] + red[3]);
        }
    }
    const float norm = grad_scale * (float)sqrt(ss);
    float coef = 1.f;
    if (max_norm > 0.f) {                                      // torch.nn.utils.clip_grad_norm_
        coef = max_norm / (norm + 1e-6f);
        coef = coef > 1.f ? 1.f : coef;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        grad_norm[0] = norm;
        if (x.acc) meters_add(x.acc, x.mx, x.loss, x.prob, norm, x.node_off_q, x.edge_off_q, x.node_off_k, x.B);
    }
    coef *= grad_scale;
    const int64_t nmax = x.ema && x.n_ema > n ? x.n_ema : n;
    for (int64_t i = i0; i < nmax; i += stride) {
        float pi, ei = 0.f;
        if (i != i0) {
            const int64_t j = i < n ? i : n - 1;
            g0 = g[j]; p0 = p[j]; a0 = s[j];
            if constexpr (kTwo) b0 = s1[j];
            if (x.ema) ei = x.ema[i < x.n_ema ? i : x.n_ema - 1];
        } else {
            ei = e0;
        }
        if (i < n) {
            const float gc = g0 * coef;
            g[i] = gc;                                         // the clipped gradient stays visible, as in torch
            pi = tail_update<kRule>(gc, p0, a0, b0, h, s[i], kTwo ? s1[i] : b0);
            p[i] = pi;
        } else {
            pi = p[i];                                         // parameters past the live prefix: only averaged
        }
        if (x.ema && i < x.n_ema) x.ema[i] = ei * x.ema_m + (1.f - x.ema_m) * pi;   // p2.mul_(m).add_(1 - m, p1), train.py:169-172
    }
}

// clip_grad_value_ + the same rules: the fine-tuning tail, one launch, no norm pass
template <int kRule>
__global__ __launch_bounds__(kThreads) void tail_value_kernel(float *p, float *g, float *s, int64_t n, float clip, float grad_scale,
                                                              TailHyper h, float *s1)
{
    TRAIN_STEP_WAVE_PRIORITY();
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
        float gc = g[i] * grad_scale;
        if (clip > 0.f) gc = gc < -clip ? -clip : (gc > clip ? clip : gc);   // clip_grad_value_ (NaN passes, as clamp_)
        g[i] = gc;                                           // the clipped gradient stays visible, as in torch
        const float p0 = p[i], a0 = s[i];
        float b0 = 0.f;
        if constexpr (kRule == kAdam) b0 = s1[i];
        p[i] = tail_update<kRule>(gc, p0, a0, b0, h, s[i], kRule == kAdam ? s1[i] : b0);
    }
}

// ---- the meters as a launch of their own: one thread
__global__ void step_meters_kernel(double *acc, int32_t *mx, const float *loss, const float *prob, const float *gnorm,
                                   const int32_t *node_off_q, const int32_t *edge_off_q, const int32_t *node_off_k,
                                   int32_t B)
{
    TRAIN_STEP_WAVE_PRIORITY();
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    meters_add(acc, mx, loss, prob, gnorm[0], node_off_q, edge_off_q, node_off_k, B);
}

__global__ void step_scalars_kernel(gcc_step_scalars *dev, gcc_step_scalars v) { *dev = v; }

// one thread: ring entry (*counter mod ring_len) of the host-pinned ring -> the device struct; the entry was written by plain
// host stores before this launch was submitted, and is read word by word with system-scope loads (the ring's lines are
// reused every ring_len steps: nothing may be served from a stale cache line)
__global__ void step_scalars_fetch_kernel(gcc_step_scalars *dev, const gcc_step_scalars *ring, int ring_len,
                                          unsigned long long *counter)
{
    const unsigned long long n = *counter;
    const uint32_t *src = (const uint32_t *)(ring + (n % (unsigned long long)ring_len));
    uint32_t *dst = (uint32_t *)dev;
#pragma unroll
    for (int i = 0; i < (int)(sizeof(gcc_step_scalars) / 4); ++i) dst[i] = load_system_u32(src + i);
    *counter = n + 1;
}

// the ONE copy of Adam's bias corrections: every by-value entry point and the scalars ring form them here
void fill_scalars(gcc_step_scalars &v, float lr, float beta1, float beta2, int32_t adam_step, int32_t enqueue_index,
                  uint64_t dropout_seed)
{
    v.lr = lr;
    v.bias_corr1 = 1.0f - powf(beta1, (float)adam_step);
    v.bias_corr2_sqrt = sqrtf(1.0f - powf(beta2, (float)adam_step));
    v.enqueue_index = enqueue_index;
    v.dropout_seed = dropout_seed;
}

// the host's hyper-parameters of one step: by value (``step`` >= 1), or lr / bias corrections left to the device struct
TailHyper tail_hyper(int32_t rule, bool scalars, float lr, float beta1, float beta2, float eps, float wd, int32_t step, float hyper)
{
    TailHyper h = {wd, hyper, scalars ? 0.f : lr, 1.f, 1.f, beta1, beta2, eps};
    if (rule == kAdam && !scalars) {
        gcc_step_scalars v;
        fill_scalars(v, lr, beta1, beta2, step, 0, 0);
        h.bc1 = v.bias_corr1; h.bc2_sqrt = v.bias_corr2_sqrt;
    }
    return h;
}

int tail_blocks(int64_t n)
{
    const int64_t blocks = (n + kThreads - 1) / kThreads;
    return blocks > 512 ? 512 : (int)blocks;
}

// the one argument check of both launchers (``rule`` is one of the three by now).  ``s1``: Adam's exp_avg_sq; ``step``: Adam's
// by-value step count (1 where there is none)
int32_t tail_check(const char *who, int32_t rule, const float *param, const float *grad, const float *s, const float *s1, int64_t n,
                   int32_t step, float grad_scale)
{
    if (n < 1) { snprintf(g_err, kErrLen, "%s: n = %lld, at least one element is needed", who, (long long)n); return -1; }
    if (!param || !grad || !s || (rule == kAdam && !s1)) {
        snprintf(g_err, kErrLen, "%s: %s is NULL", who,
                 !param ? "param" : !grad ? "grad" : rule != kAdam ? "state" : !s ? "exp_avg" : "exp_avg_sq");
        return -1;
    }
    if (step < 1) { snprintf(g_err, kErrLen, "%s: step = %d, steps count from 1", who, step); return -1; }
    if (!(grad_scale > 0.f)) { snprintf(g_err, kErrLen, "%s: grad_scale must be positive", who); return -1; }
    return 0;
}

// gcc_opt_*: rules 1 and 2 only -- Adam has entry points of its own
int32_t opt_rule_check(const char *who, int32_t rule)
{
    if (rule == GCC_OPT_SGD || rule == GCC_OPT_ADAGRAD) return 0;
    snprintf(g_err, kErrLen, "%s: unknown rule %d (GCC_OPT_SGD = 1, GCC_OPT_ADAGRAD = 2)", who, rule);
    return -2;
}

struct TailFold {            // gcc_adam_ema_enqueue_step_scalars
    const double *parts; int32_t nparts;
    float *q_mem; const float *q_keys; int32_t q_K, q_nkeys;
};

// every clip-by-norm entry point: [sum of squares] + tail_norm_kernel<rule>
int32_t norm_launch(const char *who, int32_t rule, float *param, float *grad, float *s, float *s1, int64_t n, const TailHyper &h,
                    int32_t step, float max_norm, float grad_scale, float *grad_norm, double *scratch, float *ema, int64_t n_ema,
                    float ema_m, const gcc_step_meters_args *meters, const gcc_step_scalars *scalars, void *stream,
                    const TailFold *fold = nullptr)
{
    const int32_t rc = tail_check(who, rule, param, grad, s, s1, n, step, grad_scale);
    if (rc) return rc;
    if (!grad_norm || !scratch || (ema && n_ema < n) ||
        (meters && (!meters->acc || !meters->mx || !meters->loss || !meters->prob || !meters->node_off_q ||
                    !meters->edge_off_q || !meters->node_off_k || meters->batch_size < 1))) {
        snprintf(g_err, kErrLen, "%s: bad argument (grad_norm / scratch NULL, n_ema < n, or an incomplete meters struct)", who);
        return -1;
    }
    hipStream_t st = (hipStream_t)stream;
    if (!fold || !fold->parts)
        hipLaunchKernelGGL(gradnorm_kernel, dim3(kNormBlocks), dim3(kThreads), 0, st, (const float *)grad, n, scratch);
    TailExtras x = {};
    x.sc = scalars;
    if (ema) { x.ema = ema; x.n_ema = n_ema; x.ema_m = ema_m; }
    if (meters) {
        x.acc = meters->acc; x.mx = meters->mx; x.loss = meters->loss; x.prob = meters->prob;
        x.node_off_q = meters->node_off_q; x.edge_off_q = meters->edge_off_q; x.node_off_k = meters->node_off_k;
        x.B = meters->batch_size;
    }
    const int blocks = tail_blocks(ema ? n_ema : n);
    int extra = 0;
    if (fold) {
        x.parts = fold->parts; x.nparts = fold->nparts;
        if (fold->q_mem) {
            x.q_mem = fold->q_mem; x.q_keys = fold->q_keys; x.q_K = fold->q_K; x.q_nkeys = fold->q_nkeys; x.tail_blocks = blocks;
            extra = (fold->q_nkeys * 16 + kThreads - 1) / kThreads;
        }
    }
    const dim3 grid(blocks + extra), block(kThreads);
    const double *sumsq = scratch;
    auto *kernel = rule == kAdam ? tail_norm_kernel<kAdam> : rule == GCC_OPT_SGD ? tail_norm_kernel<GCC_OPT_SGD> : tail_norm_kernel<GCC_OPT_ADAGRAD>;
    hipLaunchKernelGGL(kernel, grid, block, 0, st, param, grad, s, n, h, max_norm, grad_scale, sumsq, grad_norm, x, s1);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

// both clip-by-value entry points: tail_value_kernel<rule>
int32_t value_launch(const char *who, int32_t rule, float *param, float *grad, float *s, float *s1, int64_t n, const TailHyper &h,
                     int32_t step, float clip, float grad_scale, void *stream)
{
    const int32_t rc = tail_check(who, rule, param, grad, s, s1, n, step, grad_scale);
    if (rc) return rc;
    const dim3 grid(tail_blocks(n)), block(kThreads);
    hipStream_t st = (hipStream_t)stream;
    auto *kernel = rule == kAdam ? tail_value_kernel<kAdam> : rule == GCC_OPT_SGD ? tail_value_kernel<GCC_OPT_SGD> : tail_value_kernel<GCC_OPT_ADAGRAD>;
    hipLaunchKernelGGL(kernel, grid, block, 0, st, param, grad, s, n, clip, grad_scale, h, s1);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

}  // namespace

extern "C" {

int32_t gcc_queue_enqueue(float *mem, int32_t K, const float *keys, int32_t nkeys, int32_t index, float *saved,
                          void *stream)
{
    if (!mem || !keys || K < 1 || nkeys < 1 || nkeys > K || index < 0 || index >= K) {
        snprintf(g_err, kErrLen, "gcc_queue_enqueue: bad argument (K=%d n=%d index=%d)", K, nkeys, index);
        return -1;
    }
    hipLaunchKernelGGL(queue_enqueue_kernel, dim3((nkeys * 16 + kThreads - 1) / kThreads), dim3(kThreads), 0,
                       (hipStream_t)stream, mem, K, keys, nkeys, index, saved, (const gcc_step_scalars *)nullptr);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

int32_t gcc_queue_enqueue_scalars(float *mem, int32_t K, const float *keys, int32_t nkeys, const gcc_step_scalars *scalars,
                                  void *stream)
{
    if (!mem || !keys || !scalars || K < 1 || nkeys < 1 || nkeys > K) {
        snprintf(g_err, kErrLen, "gcc_queue_enqueue_scalars: bad argument (K=%d n=%d)", K, nkeys);
        return -1;
    }
    hipLaunchKernelGGL(queue_enqueue_kernel, dim3((nkeys * 16 + kThreads - 1) / kThreads), dim3(kThreads), 0,
                       (hipStream_t)stream, mem, K, keys, nkeys, 0, (float *)nullptr, scalars);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

void gcc_step_scalars_fill(gcc_step_scalars *host_entry, float lr, float beta1, float beta2, int32_t adam_step,
                           int32_t enqueue_index, uint64_t dropout_seed)
{
    gcc_step_scalars v;
    fill_scalars(v, lr, beta1, beta2, adam_step, enqueue_index, dropout_seed);
    memcpy(host_entry, &v, sizeof(v));
    __atomic_thread_fence(__ATOMIC_RELEASE);                      // visible before the launch that follows is submitted
}

int32_t gcc_step_scalars_fetch(gcc_step_scalars *dev, const gcc_step_scalars *ring, int32_t ring_len,
                               unsigned long long *counter, void *stream)
{
    if (!dev || !ring || !counter || ring_len < 1) {
        snprintf(g_err, kErrLen, "gcc_step_scalars_fetch: bad argument");
        return -1;
    }
    hipLaunchKernelGGL(step_scalars_fetch_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, dev, ring, (int)ring_len, counter);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

int32_t gcc_step_scalars_set(gcc_step_scalars *dev, float lr, float beta1, float beta2, int32_t adam_step,
                             int32_t enqueue_index, uint64_t dropout_seed, void *stream)
{
    if (!dev || adam_step < 1 || enqueue_index < 0) {
        snprintf(g_err, kErrLen, "gcc_step_scalars_set: bad argument");
        return -1;
    }
    gcc_step_scalars v;
    fill_scalars(v, lr, beta1, beta2, adam_step, enqueue_index, dropout_seed);
    hipLaunchKernelGGL(step_scalars_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, dev, v);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

int32_t gcc_adam_step(float *param, float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, float lr,
                      float beta1, float beta2, float eps, float weight_decay, int32_t step, float max_norm,
                      float grad_scale, float *grad_norm, double *scratch, void *stream)
{
    return norm_launch("gcc_adam_step", kAdam, param, grad, exp_avg, exp_avg_sq, n,
                       tail_hyper(kAdam, false, lr, beta1, beta2, eps, weight_decay, step, 0.f), step, max_norm, grad_scale,
                       grad_norm, scratch, nullptr, 0, 0.f, nullptr, nullptr, stream);
}

int32_t gcc_adam_ema_step(float *param, float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, float lr,
                          float beta1, float beta2, float eps, float weight_decay, int32_t step, float max_norm,
                          float grad_scale, float *grad_norm, double *scratch, float *ema, int64_t n_ema, float ema_m,
                          const gcc_step_meters_args *meters, void *stream)
{
    return norm_launch("gcc_adam_ema_step", kAdam, param, grad, exp_avg, exp_avg_sq, n,
                       tail_hyper(kAdam, false, lr, beta1, beta2, eps, weight_decay, step, 0.f), step, max_norm, grad_scale,
                       grad_norm, scratch, ema, n_ema, ema_m, meters, nullptr, stream);
}

int32_t gcc_adam_ema_step_scalars(float *param, float *grad, float *exp_avg, float *exp_avg_sq, int64_t n,
                                  float beta1, float beta2, float eps, float weight_decay, float max_norm,
                                  float grad_scale, float *grad_norm, double *scratch, float *ema, int64_t n_ema, float ema_m,
                                  const gcc_step_meters_args *meters, const gcc_step_scalars *scalars, void *stream)
{
    if (!scalars) { snprintf(g_err, kErrLen, "gcc_adam_ema_step_scalars: scalars is NULL"); return -1; }
    return norm_launch("gcc_adam_ema_step_scalars", kAdam, param, grad, exp_avg, exp_avg_sq, n,
                       tail_hyper(kAdam, true, 0.f, beta1, beta2, eps, weight_decay, 0, 0.f), 1, max_norm, grad_scale, grad_norm,
                       scratch, ema, n_ema, ema_m, meters, scalars, stream);
}

int32_t gcc_adam_ema_enqueue_step_scalars(float *param, float *grad, float *exp_avg, float *exp_avg_sq, int64_t n,
                                          float beta1, float beta2, float eps, float weight_decay, float max_norm,
                                          float grad_scale, float *grad_norm, double *scratch, float *ema, int64_t n_ema, float ema_m,
                                          const gcc_step_meters_args *meters, const gcc_step_scalars *scalars,
                                          const double *sumsq_parts, int32_t nparts, float *queue, int32_t K, const float *keys,
                                          int32_t nkeys, void *stream)
{
    const char *who = "gcc_adam_ema_enqueue_step_scalars";
    if (!scalars) { snprintf(g_err, kErrLen, "%s: scalars is NULL", who); return -1; }
    if ((sumsq_parts && nparts < 1) || (!sumsq_parts && nparts != 0) || (queue && (!keys || K < 1 || nkeys < 1 || nkeys > K)) ||
        (!sumsq_parts && !queue)) {
        snprintf(g_err, kErrLen, "%s: bad argument (nparts=%d K=%d n=%d)", who, nparts, K, nkeys);
        return -1;
    }
    const TailFold fold = {sumsq_parts, nparts, queue, keys, K, nkeys};
    return norm_launch(who, kAdam, param, grad, exp_avg, exp_avg_sq, n,
                       tail_hyper(kAdam, true, 0.f, beta1, beta2, eps, weight_decay, 0, 0.f), 1, max_norm, grad_scale, grad_norm,
                       scratch, ema, n_ema, ema_m, meters, scalars, stream, &fold);
}

int32_t gcc_adam_clipvalue_step(float *param, float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, float lr,
                                float beta1, float beta2, float eps, float weight_decay, int32_t step, float clip_value,
                                float grad_scale, void *stream)
{
    return value_launch("gcc_adam_clipvalue_step", kAdam, param, grad, exp_avg, exp_avg_sq, n,
                        tail_hyper(kAdam, false, lr, beta1, beta2, eps, weight_decay, step, 0.f), step, clip_value, grad_scale, stream);
}

int32_t gcc_opt_step(int32_t rule, float *param, float *grad, float *state, int64_t n, float lr, float hyper, float weight_decay,
                     float max_norm, float grad_scale, float *grad_norm, double *scratch, void *stream)
{
    if (const int32_t rc = opt_rule_check("gcc_opt_step", rule)) return rc;
    return norm_launch("gcc_opt_step", rule, param, grad, state, nullptr, n,
                       tail_hyper(rule, false, lr, 0.f, 0.f, 0.f, weight_decay, 1, hyper), 1, max_norm, grad_scale, grad_norm,
                       scratch, nullptr, 0, 0.f, nullptr, nullptr, stream);
}

int32_t gcc_opt_ema_step(int32_t rule, float *param, float *grad, float *state, int64_t n, float lr, float hyper, float weight_decay,
                         float max_norm, float grad_scale, float *grad_norm, double *scratch, float *ema, int64_t n_ema, float ema_m,
                         const gcc_step_meters_args *meters, void *stream)
{
    if (const int32_t rc = opt_rule_check("gcc_opt_ema_step", rule)) return rc;
    return norm_launch("gcc_opt_ema_step", rule, param, grad, state, nullptr, n,
                       tail_hyper(rule, false, lr, 0.f, 0.f, 0.f, weight_decay, 1, hyper), 1, max_norm, grad_scale, grad_norm,
                       scratch, ema, n_ema, ema_m, meters, nullptr, stream);
}

int32_t gcc_opt_ema_step_scalars(int32_t rule, float *param, float *grad, float *state, int64_t n, float hyper, float weight_decay,
                                 float max_norm, float grad_scale, float *grad_norm, double *scratch, float *ema, int64_t n_ema,
                                 float ema_m, const gcc_step_meters_args *meters, const gcc_step_scalars *scalars, void *stream)
{
    if (!scalars) { snprintf(g_err, kErrLen, "gcc_opt_ema_step_scalars: scalars is NULL"); return -1; }
    if (const int32_t rc = opt_rule_check("gcc_opt_ema_step_scalars", rule)) return rc;
    return norm_launch("gcc_opt_ema_step_scalars", rule, param, grad, state, nullptr, n,
                       tail_hyper(rule, true, 0.f, 0.f, 0.f, 0.f, weight_decay, 1, hyper), 1, max_norm, grad_scale, grad_norm,
                       scratch, ema, n_ema, ema_m, meters, scalars, stream);
}

int32_t gcc_opt_clipvalue_step(int32_t rule, float *param, float *grad, float *state, int64_t n, float lr, float hyper,
                               float weight_decay, float clip_value, float grad_scale, void *stream)
{
    if (const int32_t rc = opt_rule_check("gcc_opt_clipvalue_step", rule)) return rc;
    return value_launch("gcc_opt_clipvalue_step", rule, param, grad, state, nullptr, n,
                        tail_hyper(rule, false, lr, 0.f, 0.f, 0.f, weight_decay, 1, hyper), 1, clip_value, grad_scale, stream);
}

int32_t gcc_step_meters(double *acc, int32_t *mx, const float *loss, const float *prob, const float *grad_norm,
                        const int32_t *node_off_q, const int32_t *edge_off_q, const int32_t *node_off_k,
                        int32_t batch_size, void *stream)
{
    if (!acc || !mx || !loss || !prob || !grad_norm || !node_off_q || !edge_off_q || !node_off_k || batch_size < 1) {
        snprintf(g_err, kErrLen, "gcc_step_meters: bad argument");
        return -1;
    }
    hipLaunchKernelGGL(step_meters_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, acc, mx, loss, prob, grad_norm,
                       node_off_q, edge_off_q, node_off_k, batch_size);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

int32_t gcc_ema_update(float *ema, const float *p, int64_t n, float m, void *stream)
{
    if (!ema || !p || n < 1) { snprintf(g_err, kErrLen, "gcc_ema_update: bad argument"); return -1; }
    int blocks = (int)((n + kThreads - 1) / kThreads);
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(ema_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, ema, p, n, m);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

}  // extern "C"
