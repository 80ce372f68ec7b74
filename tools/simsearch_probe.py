"""Times gcc_sim_search on the MI355X against the plain-torch composition of the same search on the same GPU:

    F.normalize of both tables, mm, the comparison count against the target's score, topk

chunked over the queries where the [mq, mc] float32 score matrix would not fit the chunk budget.  Shapes (mq, mc, D), each
with k = 40: (2048, 2048, 64), the scale of the reference's co-author datasets, then (65536, 65536, 64) and (65536, 65536, 256).
Random non-zero Gaussian data, device-event pairs around each repetition after a warm-up call, the median of the repetitions.
Reported per shape: both times, their ratio, the fraction of the 157 TFLOP/s exact-f32 matrix peak that 2 mq mc D / time is,
the bytes of score matrix the composition would need unchunked (mq mc 4) and the bytes of the kernel's workspace.

    python tools/simsearch_probe.py [--out profiles/simsearch_probe.json] [--shape MQ MC D ...]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gcc_amd.simsearch import SimilarityEngine  # noqa: E402

SHAPES = ((2048, 2048, 64), (65536, 65536, 64), (65536, 65536, 256))
K = 40
PEAK_F32_MATRIX = 157e12
CHUNK_BYTES = 1 << 30            # score rows held at a time by the composition


def torch_search(emb_q, emb_c, target, k, chunk):
    qn, cn = F.normalize(emb_q, dim=1), F.normalize(emb_c, dim=1)
    greater, cols, scores = [], [], []
    for q0 in range(0, qn.shape[0], chunk):
        s = qn[q0: q0 + chunk] @ cn.t()
        st = s.gather(1, target[q0: q0 + chunk, None].long())
        greater.append((s > st).sum(1))
        top = s.topk(k, dim=1)
        cols.append(top.indices)
        scores.append(top.values)
    return torch.cat(greater), torch.cat(cols), torch.cat(scores)


def timed(fn, reps):
    fn()                                                         # warm-up: allocations, code objects, clocks
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "simsearch_probe.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shape", type=int, nargs=3, action="append", metavar=("MQ", "MC", "D"), help="instead of the three shapes")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.backends.cuda.matmul.allow_tf32 = False
    engine = SimilarityEngine()
    gen = torch.Generator(device=dev).manual_seed(0)
    results = []
    for mq, mc, D in (a.shape or SHAPES):
        emb_q = torch.randn(mq, D, device=dev, generator=gen)
        emb_c = torch.randn(mc, D, device=dev, generator=gen)
        target = torch.randint(0, mc, (mq,), device=dev, generator=gen, dtype=torch.int32)
        chunk = max(1, min(mq, CHUNK_BYTES // (mc * 4)))
        res = engine.search(emb_q, emb_c, target=target, k=K)
        engine.check_status(res)
        g_ref, c_ref, _ = torch_search(emb_q, emb_c, target, K, chunk)
        # the two sides round differently, so rank counts may differ where scores are within rounding of each other: reported
        rank_diff = int((res["greater"].long() - g_ref).abs().max())
        same_top1 = float((res["topk_col"][:, 0].long() == c_ref[:, 0]).float().mean())
        ms_kernel = timed(lambda: engine.search(emb_q, emb_c, target=target, k=K), a.reps)
        ms_torch = timed(lambda: torch_search(emb_q, emb_c, target, K, chunk), a.reps)
        mk, mt = float(np.median(ms_kernel)), float(np.median(ms_torch))
        row = dict(mq=mq, mc=mc, D=D, k=K, kernel_ms=[round(x, 3) for x in ms_kernel], torch_ms=[round(x, 3) for x in ms_torch],
                   kernel_ms_median=round(mk, 3), torch_ms_median=round(mt, 3), torch_over_kernel=round(mt / mk, 3),
                   kernel_fraction_of_f32_matrix_peak=round(2.0 * mq * mc * D / (mk * 1e-3) / PEAK_F32_MATRIX, 4),
                   torch_query_chunk=chunk, torch_score_matrix_bytes_unchunked=mq * mc * 4,
                   kernel_workspace_bytes=int(engine.lib.gcc_sim_workspace_bytes(mq, mc, D, K, 0)),
                   max_rank_count_difference=rank_diff, same_best_candidate=round(same_top1, 6))
        print(json.dumps(row), flush=True)
        results.append(row)
        del emb_q, emb_c, target, res, g_ref, c_ref
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), reps=a.reps, peak_f32_matrix_flops=PEAK_F32_MATRIX, results=results),
                  f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
