"""The backward tail's degree-embedding gradient (gin_bwd_emb_kernel, gin_grad_final_kernel: gcc_amd/csrc/encoder_bwd.hip) at its
shape edges, through the C ABI, for both tiers (tests/test_bwd_tail_emu.py: the wave64 emulator; tests/test_bwd_tail_gpu.py: the
device).

The scatter of a tile's rows into the workgroup's degree table and the final sums over the 448 partial tables and the 64 slabs
have a fixed order: a change that spreads the scatter over the workgroup, or that requests the partials of a sum earlier, moves no
addition.  Two such changes were built and measured against these cases (bit-identical, and not faster inside the pipeline:
profiles/head_tail_bench_ab.txt), so the kernels are the ones that wrote the recording; the cases stay as the pin for the next
attempt.  Every case must give the recorded bits of its tier (tests/golden/bwd_tail_bits_<tier>.npz,
tests/golden/make_bwd_tail_golden.py): the 448 partial tables as they lie in the workspace, the final degree_embedding gradient,
and three weight / bias gradients of the slab sums.  So that a wrong recording cannot hide a wrong kernel, the final gradient must
also be (a) the fixed tree of gin_grad_final_kernel over the partial tables, restated in numpy float32, bit for bit, and (b) the
float64 scatter of the input-feature gradient within the rounding of the f32 sums that make it up (worked out per cell below).

Cases: 1, 63, 64, 65 and 129 rows (one row, one short of a tile, a tile, a tile and one row, two tiles and one row); a batch
whose rows all have one degree (every addend of a tile lands in one cell of each column); a batch with degrees above and at
max_degree (the clamp); 8 and 16 embedding columns (the narrow form, with idle column lanes at 8) and 32 (the wide form)."""
import os

import numpy as np
import torch

from tests import gather_ring_check as K

TILE, H = K.TILE, K.H
MAX_DEGREE = 20                    # a small table keeps the 448 recorded partial tables small
EMB_BLOCKS, WG_CHUNKS = 448, 64    # encoder_bwd.hip: kEmbBlocks, kWgChunks


def _rows(rng, n, lo=0, hi=9):
    return rng.integers(lo, hi, n).astype(np.int64)


def _tiles(deg):
    return [deg[i:i + TILE] for i in range(0, len(deg), TILE)]


def views():
    """name -> view (degrees from 0 to 8 where nothing else is said)"""
    rng = np.random.default_rng(5)
    out = {}
    for n in (1, 63, 64, 65, 129):
        out["n%d" % n] = K.view_of(_tiles(_rows(rng, n)), 60 + n, graphs=min(n, 3))
    out["one_degree"] = K.view_of(_tiles(np.full(129, 5, dtype=np.int64)), 70, graphs=3)
    deg = _rows(rng, 65, 15, 41)                               # 15 .. 40: below, at and above MAX_DEGREE
    deg[:4] = (MAX_DEGREE, MAX_DEGREE + 1, MAX_DEGREE - 1, MAX_DEGREE)
    out["above_max_degree"] = K.view_of(_tiles(deg), 71, graphs=2)
    return out


def cases():
    """name -> (view name, embedding columns, positional columns); 32 embedding columns fit the 64-column input only behind a
    16-column positional embedding (the first 16 columns of the view's)"""
    out = {"%s_emb16" % v: (v, 16, 32) for v in views()}
    out.update({"%s_emb8" % v: (v, 8, 32) for v in ("n65", "n129", "one_degree", "above_max_degree")})
    out.update({"%s_emb32" % v: (v, 32, 16) for v in ("n129", "above_max_degree")})
    return out


def _model(dev, emb, pos):
    from gcc_amd.encoder import GraphEncoder

    torch.manual_seed(1)
    return GraphEncoder(positional_embedding_size=pos, max_node_freq=16, max_edge_freq=16, max_degree=MAX_DEGREE,
                        freq_embedding_size=16, degree_embedding_size=emb, output_dim=64, node_hidden_dim=64,
                        edge_hidden_dim=64, num_layers=5, num_step_set2set=6, num_layer_set2set=3,
                        norm=True, gnn_model="gin", degree_input=True).to(dev)


def _layout(cap, B, L):
    """float offsets of D, dpooled and the partial tables in the backward workspace (encoder_bwd.hip: bwd_layout)"""
    al = lambda x: (x + 255) // 256 * 256
    o, at = 0, {}
    for name, nbytes in (("U", cap * H * 4), ("V", cap * H * 4), ("Wt", cap * H * 4), ("D", cap * H * 4)) + \
            tuple(("dz%d" % i, cap * H * 4) for i in range(2 * L)) + \
            (("G", (L + 1) * B * H * 4), ("dpooled", (L + 1) * B * H * 4),
             ("slabs", (3 * L + 1) * WG_CHUNKS * H * H * 4), ("bias_slabs", (3 * L + 1) * WG_CHUNKS * H * 4), ("demb_parts", 0)):
        at[name] = o // 4
        o = al(o + nbytes)
    return at


def run_case(T, name):
    vname, emb, pos = cases()[name]
    view = dict(views()[vname])
    view["pos_undirected"] = view["pos_undirected"][:, :pos].contiguous()
    n, B = int(view["node_off"][-1]), len(view["node_off"]) - 1
    keep = (torch.rand(5, B, H, generator=torch.Generator().manual_seed(3)) > 0.5).float().to(T.dev)
    d = torch.randn(B, H, generator=torch.Generator().manual_seed(4)).to(T.dev)
    model = _model(T.dev, emb, pos)
    model.train()
    eng = T.engine()
    p, buf = eng.make_pass(model, T.batch(view), training=True, keep=keep)
    eng.forward([p])
    eng.backward(model, p, buf, d)
    wsf = next(v for k, v in eng._bufs.items() if k[0] == "bwd").view(torch.float32)
    cap, L = p.node_cap, len(model.gnn.ginlayers)
    at = _layout(cap, B, L)
    elems = (MAX_DEGREE + 1) * emb
    out = {"view": view, "emb": emb, "pos": pos}
    out["D"] = wsf[at["D"]:at["D"] + cap * H].view(cap, H)[:n].cpu().numpy().copy()
    out["dpooled0"] = wsf[at["dpooled"]:at["dpooled"] + B * H].view(B, H).cpu().numpy().copy()
    out["demb_parts"] = wsf[at["demb_parts"]:at["demb_parts"] + EMB_BLOCKS * elems].view(EMB_BLOCKS, elems).cpu().numpy().copy()
    g = lambda t: t.grad.detach().cpu().numpy().copy()
    out["demb"] = g(model.degree_embedding.weight)
    out["lin0_w"] = g(model.gnn.ginlayers[0].apply_func.mlp.linears[0].weight)        # section (1): a layer's slabs
    out["pred1_w"] = g(model.gnn.linears_prediction[1].weight)                        # section (1): a prediction layer's
    out["pred0_b"] = g(model.gnn.linears_prediction[0].bias)                          # section (3)
    return out


RECORDED = ("demb_parts", "demb", "lin0_w", "pred1_w", "pred0_b")


def record(res):
    return {k: K.bits(res[k]) for k in RECORDED}


def golden_path(tier):
    return os.path.join(os.path.dirname(__file__), "golden", "bwd_tail_bits_%s.npz" % tier)


def final_tree(parts):
    """gin_grad_final_kernel's section (5) in float32: 8 threads an element, each over 56 consecutive tables in batches of 8
    ((v0+v1)+(v2+v3))+((v4+v5)+(v6+v7)) added in order, then the shuffle tree over lanes xor 1, 2, 4"""
    p = parts.astype(np.float32).reshape(8, EMB_BLOCKS // 64, 8, -1)
    s = np.zeros((8, p.shape[-1]), dtype=np.float32)
    for b in range(p.shape[1]):
        v = p[:, b]
        s = s + (((v[:, 0] + v[:, 1]) + (v[:, 2] + v[:, 3])) + ((v[:, 4] + v[:, 5]) + (v[:, 6] + v[:, 7])))
    s = s[0::2] + s[1::2]
    s = s[0::2] + s[1::2]
    return s[0] + s[1]


def check_case(T, name):
    res = run_case(T, name)
    view, emb, pos = res["view"], res["emb"], res["pos"]
    rp, ci, no = view["row_ptr"].numpy(), view["col_idx"].numpy(), view["node_off"].numpy()
    n = len(rp) - 1
    deg = np.diff(rp)
    # (a) the final gradient is the fixed tree over the partial tables (the test models' gradients start at zero)
    tree = final_tree(res["demb_parts"]).reshape(MAX_DEGREE + 1, emb)
    assert np.array_equal(K.bits(tree), K.bits(res["demb"])), (name, "final tree")
    # tables of workgroups without a tile are zero; a tile's rows land in its workgroup's table and nowhere else
    tiles = (n + TILE - 1) // TILE
    assert np.count_nonzero(np.abs(res["demb_parts"]).sum(1)) <= tiles, name
    # (b) float64: dx0 = (I + A) D + dpooled0[graph]; d emb[min(deg, max)] += dx0[:, pos:pos + emb].  Every cell is a chain of f32
    # additions of its terms: at most (rows of the cell + longest row + 3 + 16 for the trees) roundings of 2^-24, each of
    # at most the sum of the terms' sizes.
    row = np.repeat(np.arange(n), deg)
    gid = np.repeat(np.arange(len(no) - 1), np.diff(no))
    D = res["D"].astype(np.float64)[:, pos:pos + emb]
    dp = res["dpooled0"].astype(np.float64)[gid][:, pos:pos + emb]
    nb, nb_abs = np.zeros((n, emb)), np.zeros((n, emb))
    np.add.at(nb, row, D[ci])
    np.add.at(nb_abs, row, np.abs(D[ci]))
    cell = np.minimum(deg, MAX_DEGREE)
    want, size = np.zeros((MAX_DEGREE + 1, emb)), np.zeros((MAX_DEGREE + 1, emb))
    np.add.at(want, cell, D + nb + dp)
    np.add.at(size, cell, np.abs(D) + nb_abs + np.abs(dp))
    ops = np.bincount(cell, minlength=MAX_DEGREE + 1)[:, None] + int(deg.max(initial=0)) + 3 + 16
    err = np.abs(res["demb"].astype(np.float64) - want)
    bound = ops * 2.0 ** -24 * (1.0 + ops * 2.0 ** -24) * size                      # (1 + u)^ops - 1 <= ops u (1 + ops u)
    print(name, "max error %.3g, largest bound %.3g" % (err.max(), bound.max()))
    assert np.all(err <= bound), (name, float(err.max()))
    assert np.abs(want).max() > 0 or n == 0, name
    # the recording of the commit before, bit for bit
    z = np.load(golden_path(T.tier))
    for k, v in record(res).items():
        w = z["%s__%s" % (name, k)]
        assert v.shape == w.shape and np.array_equal(v, w), (name, k, int((v != w).sum()), "entries differ")


def check_cases_are_what_they_are_named_for():
    vs = views()
    for n in (1, 63, 64, 65, 129):
        assert len(vs["n%d" % n]["row_ptr"]) - 1 == n
    d = np.diff(vs["one_degree"]["row_ptr"].numpy())
    assert len(d) == 129 and np.all(d == 5)
    d = np.diff(vs["above_max_degree"]["row_ptr"].numpy())
    assert (d > MAX_DEGREE).sum() > 8 and (d == MAX_DEGREE).sum() >= 2 and (d < MAX_DEGREE).sum() > 4
    embs = {e for _, e, _ in cases().values()}
    assert embs == {8, 16, 32}
