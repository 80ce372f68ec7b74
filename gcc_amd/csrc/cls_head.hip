// gcc_amd/csrc/cls_head.hip -- the fine-tuning head of train.py's --finetune path (gfx950).
//
// Replaces, for train_finetune / test_finetune (train.py:175-337 of the reference):
//   out = output_layer(feat_q)           nn.Linear(hidden, num_classes)
//   loss = CrossEntropyLoss()(out, y)     mean over the batch
//   loss.backward()                       d out, d W, d b, d feat_q (fed to the encoder's backward)
//   preds = out.argmax(1); f1_score(..., average="micro") = correct / rows
// (clip_grad_value_(params, v) + Adam.step() over the flat buffers: step_tail.hip).
//
//   cls_head_kernel<train>  ONE workgroup of 1024 threads (the problem is B <= 1024 rows x C <= 64 classes x D <= 256 features,
//       latency-bound).  W [C][D] and b sit in LDS.  Phase 1: every wave takes groups of R = 64 / C rows, one lane per
//       (row, class): logit = b + feat[r] . W[c] (feat read from L2, W from LDS: lanes of one class read the same word, lanes
//       of one row the same feat word -- broadcasts), the row's first lane does max / log-sum-exp / argmax over its C lanes'
//       logits in LDS, then every lane forms softmax - onehot; the group's dfeat rows follow with lanes over d.  Phase 2 (after
//       a workgroup barrier): dW / db as sums over rows 0..B-1 in order, one thread per element.  Loss and correct count: per
//       lane over its rows in order, then a fixed wave tree and the 16 waves in order -- no float atomics anywhere, two runs
//       are bit-identical.
#include "host_common.h"

#include <math.h>

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxC = 64;
constexpr int kMaxD = 256;
constexpr int kMaxB = 1 << 20;

struct HeadDev {
    const float *feat, *W, *b;
    const int32_t *labels;
    int32_t B, D, C, ld_feat, ld_dfeat;
    float *logits, *dlogits, *dW, *db, *dfeat, *loss;
    int32_t *correct;
    double *acc; int32_t *mx; const int32_t *node_off, *edge_off;
    double *eval_loss_sum; int32_t *eval_counts;
};

template <bool kTrain>
__global__ __launch_bounds__(kThreads) void cls_head_kernel(HeadDev a)
{
    TRAIN_STEP_WAVE_PRIORITY();
    DYN_SMEM(smem);
    const int C = a.C, D = a.D, B = a.B;
    double *wl_s = reinterpret_cast<double *>(smem);         // [kWaves] per-wave loss partials
    float *wc_s = reinterpret_cast<float *>(wl_s + kWaves);  // [kWaves] correct counts; [kWaves] valid counts
    float *lg_s = wc_s + 2 * kWaves;                         // [kWaves][64] logits of a row group, then its dlogits
    float *lse_s = lg_s + kWaves * 64;                       // [kWaves][64] per-row log-sum-exp (first lane of the row)
    int *pred_s = reinterpret_cast<int *>(lse_s + kWaves * 64);   // [kWaves][64] per-row argmax
    float *b_s = reinterpret_cast<float *>(pred_s + kWaves * 64);  // [C]
    float *w_s = b_s + kMaxC;                                // [C][D]
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;

    for (int e = tid; e < C * D; e += kThreads) w_s[e] = a.W[e];
    if (tid < C) b_s[tid] = a.b[tid];
    float nv = 0.f;
    for (int r = tid; r < B; r += kThreads) nv += a.labels[r] >= 0 ? 1.f : 0.f;
    nv = wave_readlane(wave_sum(nv), 0);                     // (exact: integers far below 2^24)
    if (lane == 0) wc_s[kWaves + wave] = nv;
    __syncthreads();
    float valid = 0.f;
    for (int w = 0; w < kWaves; ++w) valid += wc_s[kWaves + w];
    const float inv_valid = valid > 0.f ? 1.f / valid : 0.f;

    // ---- phase 1: row groups of R rows, lane = g * C + c
    const int R = 64 / C;
    const int g = lane / C, c = lane - g * C;
    const bool active = g < R;
    const int groups = (B + R - 1) / R;
    float *lg = lg_s + wave * 64, *lse_w = lse_s + wave * 64;
    int *pred_w = pred_s + wave * 64;
    double my_loss = 0.0;
    float my_correct = 0.f;
    for (int gi = wave; gi < groups; gi += kWaves) {
        const int r = gi * R + g;
        const bool live = active && r < B;
        const int y = live ? a.labels[r] : -1;
        float l = 0.f;
        if (live) {
            const float *f = a.feat + (int64_t)r * a.ld_feat;
            const float *w = w_s + c * D;
            float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
            int d = 0;
            for (; d + 4 <= D; d += 4) {
                s0 = fmaf(f[d], w[d], s0);
                s1 = fmaf(f[d + 1], w[d + 1], s1);
                s2 = fmaf(f[d + 2], w[d + 2], s2);
                s3 = fmaf(f[d + 3], w[d + 3], s3);
            }
            for (; d < D; ++d) s0 = fmaf(f[d], w[d], s0);
            l = ((s0 + s1) + (s2 + s3)) + b_s[c];
            lg[lane] = l;
            if (a.logits) a.logits[(int64_t)r * C + c] = l;
        }
        wave_sync();
        if (live && c == 0) {                                // the row's first lane: max / argmax / log-sum-exp over C logits
            float m = lg[lane];
            int am = 0;
            for (int j = 1; j < C; ++j) {
                const float v = lg[lane + j];
                if (v > m) { m = v; am = j; }                 // strict: ties keep the lowest index (torch.argmax)
            }
            float s = 0.f;
            for (int j = 0; j < C; ++j) s += expf(lg[lane + j] - m);
            const float lse = m + logf(s);
            lse_w[g] = lse;
            pred_w[g] = am;
            if (y >= 0) {
                // an out-of-range label gives NaN rather than a silently wrong loss
                const float ly = y < C ? lg[lane + y] : __uint_as_float(0x7fc00000u);
                my_loss += (double)(lse - ly);
                my_correct += am == y ? 1.f : 0.f;
            }
        }
        wave_sync();
        if (kTrain) {
            float dl = 0.f;
            if (live && y >= 0) {
                const float p = expf(l - lse_w[g]);
                dl = (p - (c == y ? 1.f : 0.f)) * inv_valid;
            }
            if (live) a.dlogits[(int64_t)r * C + c] = dl;
            wave_sync();                                     // (every lane has read its own logit before it is overwritten)
            if (active) lg[lane] = dl;
            wave_sync();
            // dfeat rows of this group: lanes over d, d < ld_dfeat (columns past D are written as zero)
            const int rows = min(R, B - gi * R);
            for (int gg = 0; gg < rows; ++gg) {
                const int rr = gi * R + gg;
                const float *dlr = lg + gg * C;
                for (int d = lane; d < a.ld_dfeat; d += 64) {
                    float s = 0.f;
                    if (d < D)
                        for (int j = 0; j < C; ++j) s = fmaf(dlr[j], w_s[j * D + d], s);
                    a.dfeat[(int64_t)rr * a.ld_dfeat + d] = s;
                }
            }
            wave_sync();
        }
    }
    // loss / correct: per-lane partials (rows in a fixed order) -> fixed wave tree -> waves in order
    const double wl = wave_readlane(wave_sum(my_loss), 0);
    const float wc = wave_readlane(wave_sum(my_correct), 0);
    if (lane == 0) { wl_s[wave] = wl; wc_s[wave] = wc; }
    __syncthreads();                                         // also publishes phase 1's dlogits to the whole workgroup

    if (kTrain) {
        // ---- phase 2: dW[c][d] = sum_r dlogits[r][c] feat[r][d], db[c] = sum_r dlogits[r][c]; rows in order
        for (int e = tid; e < C * D; e += kThreads) {
            const int cc = e / D, d = e - cc * D;
            float s = 0.f;
            for (int r = 0; r < B; ++r) s = fmaf(a.dlogits[(int64_t)r * C + cc], a.feat[(int64_t)r * a.ld_feat + d], s);
            a.dW[e] = s;
        }
        if (tid < C) {
            float s = 0.f;
            for (int r = 0; r < B; ++r) s += a.dlogits[(int64_t)r * C + tid];
            a.db[tid] = s;
        }
    }
    if (tid == 0) {
        double tl = 0.0;
        float tc = 0.f;
        for (int w = 0; w < kWaves; ++w) { tl += wl_s[w]; tc += wc_s[w]; }
        const int32_t ic = (int32_t)tc, iv = (int32_t)valid;
        if (kTrain) {
            const float mean = valid > 0.f ? (float)(tl / (double)valid) : 0.f;
            a.loss[0] = mean;
            if (a.correct) { a.correct[0] = ic; a.correct[1] = iv; }
            if (a.acc) {                                     // train.py:248-254's meters, accumulated on the device
                a.acc[0] += (double)mean * (double)valid;    // loss_meter.update(loss, bsz)
                a.acc[1] += (double)ic;                      // f1_meter.update(correct / bsz, bsz)
                a.acc[2] += (double)valid;
                a.acc[3] += a.node_off ? (double)a.node_off[B] : 0.0;
                a.acc[4] += 1.0;
                if (a.mx && a.node_off && a.edge_off) {
                    const int32_t n = a.node_off[B], m = a.edge_off[B];
                    a.mx[0] = n > a.mx[0] ? n : a.mx[0];
                    a.mx[1] = m > a.mx[1] ? m : a.mx[1];
                }
            }
        } else {
            a.eval_loss_sum[0] += tl;
            a.eval_counts[0] += ic;
            a.eval_counts[1] += iv;
        }
    }
}

size_t head_lds_bytes(int C, int D)
{
    return sizeof(float) * ((size_t)C * D + kMaxC + 2 * kWaves * 64) + sizeof(int) * kWaves * 64 + sizeof(double) * kWaves +
           sizeof(float) * 2 * kWaves;
}

int check_head(const char *who, const gcc_cls_head_args *h, bool train)
{
    if (!h || !h->feat || !h->W || !h->b || !h->labels) {
        snprintf(g_err, kErrLen, "%s: NULL argument", who);
        return -1;
    }
    if (h->C < 1 || h->C > kMaxC) {
        snprintf(g_err, kErrLen, "%s: num_classes %d outside 1..%d", who, h->C, kMaxC);
        return -2;
    }
    if (h->D < 1 || h->D > kMaxD || h->ld_feat < h->D) {
        snprintf(g_err, kErrLen, "%s: feature size %d (ld %d) outside 1..%d", who, h->D, h->ld_feat, kMaxD);
        return -3;
    }
    if (h->B < 1 || h->B > kMaxB) {
        snprintf(g_err, kErrLen, "%s: batch size %d outside 1..%d", who, h->B, kMaxB);
        return -4;
    }
    if (train && (!h->dlogits || !h->dW || !h->db || !h->dfeat || !h->loss || h->ld_dfeat < h->D)) {
        snprintf(g_err, kErrLen, "%s: dlogits / dW / db / dfeat / loss must be given (ld_dfeat >= D)", who);
        return -1;
    }
    if (!train && (!h->eval_loss_sum || !h->eval_counts)) {
        snprintf(g_err, kErrLen, "%s: eval_loss_sum / eval_counts must be given", who);
        return -1;
    }
    return 0;
}

template <bool kTrain>
int32_t launch_head(const char *who, const gcc_cls_head_args *h, void *stream)
{
    const int rc = check_head(who, h, kTrain);
    if (rc) return rc;
    HeadDev a = {};
    a.feat = h->feat; a.W = h->W; a.b = h->b; a.labels = h->labels;
    a.B = h->B; a.D = h->D; a.C = h->C; a.ld_feat = h->ld_feat; a.ld_dfeat = h->ld_dfeat;
    a.logits = h->logits; a.dlogits = h->dlogits; a.dW = h->dW; a.db = h->db; a.dfeat = h->dfeat; a.loss = h->loss;
    a.correct = h->correct;
    a.acc = h->meter_acc; a.mx = h->meter_max; a.node_off = h->node_off; a.edge_off = h->edge_off;
    a.eval_loss_sum = h->eval_loss_sum; a.eval_counts = h->eval_counts;
    const size_t lds = head_lds_bytes(h->C, h->D);
#ifndef GCC_AMD_HIPEMU
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute((const void *)cls_head_kernel<kTrain>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
#endif
    hipLaunchKernelGGL(cls_head_kernel<kTrain>, dim3(1), dim3(kThreads), lds, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

}  // namespace

extern "C" {

int32_t gcc_cls_head_train(const gcc_cls_head_args *args, void *stream)
{
    return launch_head<true>("gcc_cls_head_train", args, stream);
}

int32_t gcc_cls_head_eval(const gcc_cls_head_args *args, void *stream)
{
    return launch_head<false>("gcc_cls_head_eval", args, stream);
}

}  // extern "C"
