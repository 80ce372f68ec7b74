"""ctypes binding of libgcc_amd.so (include/gcc_amd.h).

This is the stub a maintainer of the reference would add: the
reference is pure Python, so the FFI is ctypes.  The product path has NO CPU
fallback: :func:`load` raises if the HIP library is missing, and every wrapper
in this package refuses non-CUDA tensors.
"""
from __future__ import annotations

import ctypes
import os
from collections import namedtuple

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libgcc_amd.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "gcc_amd.h")

c_i32p = ctypes.POINTER(ctypes.c_int32)
c_f32p = ctypes.POINTER(ctypes.c_float)
c_f64p = ctypes.POINTER(ctypes.c_double)

STATUS_SCRATCH_OVERFLOW = 1
STATUS_NODE_OVERFLOW = 2
STATUS_EDGE_OVERFLOW = 4


class GccGraph(ctypes.Structure):
    _fields_ = [
        ("row_ptr", ctypes.c_void_p),
        ("col_idx", ctypes.c_void_p),
        ("seed_cdf", ctypes.c_void_p),
        ("ltab", ctypes.c_void_p),
        ("num_nodes", ctypes.c_int64),
        ("num_edges", ctypes.c_int64),
        ("ltab_len", ctypes.c_int32),
        ("lmax", ctypes.c_int32),
        ("shard_off", ctypes.c_void_p),
        ("num_shards", ctypes.c_int32),
        ("flags", ctypes.c_int32),
        ("hub_index", ctypes.c_void_p), ("hub_adj", ctypes.c_void_p),
        ("num_hubs", ctypes.c_int32), ("hub_words", ctypes.c_int32),
        ("hub_table_degree", ctypes.c_int32), ("reserved_", ctypes.c_int32),
    ]


class GccSampleParams(ctypes.Structure):
    _fields_ = [
        ("run_seed", ctypes.c_uint64),
        ("first_sample_id", ctypes.c_int64),
        ("batch_size", ctypes.c_int32),
        ("restart_u32", ctypes.c_uint32),
        ("seeds", ctypes.c_void_p),
        ("prof", ctypes.c_void_p),
        ("hub_degree", ctypes.c_int32),
        ("max_hubs", ctypes.c_int32),
    ]


class GccPosembView(ctypes.Structure):
    _fields_ = [("g", ctypes.c_void_p), ("pos", ctypes.c_void_p), ("evals", ctypes.c_void_p), ("raw", ctypes.c_void_p)]


class GccBatchOut(ctypes.Structure):
    _fields_ = [
        ("node_off", ctypes.c_void_p),
        ("edge_off", ctypes.c_void_p),
        ("parent_nid", ctypes.c_void_p),
        ("graph_id", ctypes.c_void_p),
        ("row_ptr", ctypes.c_void_p),
        ("col_idx", ctypes.c_void_p),
        ("node_cap", ctypes.c_int64),
        ("edge_cap", ctypes.c_int64),
    ]


class GccGraphCorpus(ctypes.Structure):      # gcc_graph_corpus: every graph of a whole-graph dataset (csrc/graph_batch.hip)
    _fields_ = [
        ("num_graphs", ctypes.c_int32), ("pos_dim", ctypes.c_int32),
        ("node_first", ctypes.c_void_p), ("row_ptr", ctypes.c_void_p), ("col_idx", ctypes.c_void_p),
        ("seed_local", ctypes.c_void_p), ("labels", ctypes.c_void_p), ("pos", ctypes.c_void_p),
    ]


PACK_GRAPHS_MAX_BATCH = 1024
STATUS_PACK_NODE_OVERFLOW = 1                # gcc_pack_graphs' own status word
STATUS_PACK_EDGE_OVERFLOW = 2
STATUS_PACK_BAD_INDEX = 4

GIN_MAX_LAYERS = 8
GIN_HIDDEN = 64
_VP = ctypes.c_void_p


class GccBn(ctypes.Structure):
    _fields_ = [("weight", _VP), ("bias", _VP), ("running_mean", _VP), ("running_var", _VP),
                ("num_batches_tracked", _VP)]


class GccGinWeights(ctypes.Structure):
    _fields_ = [
        ("num_gin_layers", ctypes.c_int32), ("pos_dim", ctypes.c_int32), ("deg_emb_dim", ctypes.c_int32),
        ("max_degree", ctypes.c_int32),
        ("degree_embedding", _VP),
        ("lin0_w", _VP * GIN_MAX_LAYERS), ("lin0_b", _VP * GIN_MAX_LAYERS),
        ("lin1_w", _VP * GIN_MAX_LAYERS), ("lin1_b", _VP * GIN_MAX_LAYERS),
        ("bn_a", GccBn * GIN_MAX_LAYERS), ("bn_b", GccBn * GIN_MAX_LAYERS), ("bn_c", GccBn * GIN_MAX_LAYERS),
        ("pred_w", _VP * (GIN_MAX_LAYERS + 1)), ("pred_b", _VP * (GIN_MAX_LAYERS + 1)),
        ("bn_eps", ctypes.c_float), ("bn_momentum", ctypes.c_float), ("dropout_p", ctypes.c_float),
        ("norm_eps", ctypes.c_float),
        ("hidden", ctypes.c_int32),
    ]


class GccGinPass(ctypes.Structure):
    _fields_ = [
        ("node_off", _VP), ("row_ptr", _VP), ("col_idx", _VP), ("graph_id", _VP), ("pos", _VP),
        ("batch_size", ctypes.c_int32), ("training", ctypes.c_int32), ("update_running_stats", ctypes.c_int32),
        ("normalize", ctypes.c_int32),
        ("dropout_keep", _VP),
        ("dropout_seed", ctypes.c_uint64), ("dropout_philox", ctypes.c_int32),
        ("w", GccGinWeights),
        ("x0", _VP), ("agg", _VP * GIN_MAX_LAYERS), ("z1", _VP * GIN_MAX_LAYERS), ("z2", _VP * GIN_MAX_LAYERS),
        ("stats", _VP), ("pooled", _VP), ("score", _VP), ("feat", _VP),
        ("edge_multiplicity", ctypes.c_int32),
        ("bn_totals", _VP),
        ("seed_local", _VP),
        ("scalars", _VP),
        ("node_cap", ctypes.c_int64),
        ("rows_hint", ctypes.c_int64),
    ]


class GccGinxPass(ctypes.Structure):          # gcc_ginx_pass: the encoder at any width (csrc/ginx.hip)
    _fields_ = [
        ("node_off", _VP), ("row_ptr", _VP), ("col_idx", _VP), ("graph_id", _VP), ("pos", _VP), ("seed_local", _VP),
        ("batch_size", ctypes.c_int32), ("training", ctypes.c_int32), ("update_running_stats", ctypes.c_int32),
        ("normalize", ctypes.c_int32),
        ("dropout_keep", _VP),
        ("hidden", ctypes.c_int32), ("out_dim", ctypes.c_int32), ("edge_multiplicity", ctypes.c_int32),
        ("gemm_dtype", ctypes.c_int32),       # 0: f32, 1: bf16 operands of the per-node Linears (GEMM_DTYPES)
        ("node_cap", ctypes.c_int64),
        ("w", GccGinWeights),
        ("workspace", _VP), ("workspace_bytes", ctypes.c_int64),
        ("feat", _VP), ("pooled_out", _VP),
    ]


class GccGinGrads(ctypes.Structure):
    _fields_ = [
        ("degree_embedding", _VP),
        ("lin0_w", _VP * GIN_MAX_LAYERS), ("lin0_b", _VP * GIN_MAX_LAYERS),
        ("lin1_w", _VP * GIN_MAX_LAYERS), ("lin1_b", _VP * GIN_MAX_LAYERS),
        ("bn_a_w", _VP * GIN_MAX_LAYERS), ("bn_a_b", _VP * GIN_MAX_LAYERS),
        ("bn_b_w", _VP * GIN_MAX_LAYERS), ("bn_b_b", _VP * GIN_MAX_LAYERS),
        ("bn_c_w", _VP * GIN_MAX_LAYERS), ("bn_c_b", _VP * GIN_MAX_LAYERS),
        ("pred_w", _VP * (GIN_MAX_LAYERS + 1)), ("pred_b", _VP * (GIN_MAX_LAYERS + 1)),
    ]


class GccNceArgs(ctypes.Structure):
    _fields_ = [
        ("q", _VP), ("k", _VP), ("mem", _VP), ("patch", _VP),
        ("patch_index", ctypes.c_int32), ("patch_rows", ctypes.c_int32),
        ("B", ctypes.c_int32), ("K", ctypes.c_int32), ("pos_mode", ctypes.c_int32), ("inv_T", ctypes.c_float),
        ("lse", _VP), ("pos", _VP), ("loss", _VP), ("prob", _VP), ("out_dense", _VP),
        ("dtype", ctypes.c_int32),
    ]


class GccStepMetersArgs(ctypes.Structure):
    _fields_ = [("acc", _VP), ("mx", _VP), ("loss", _VP), ("prob", _VP), ("node_off_q", _VP), ("edge_off_q", _VP),
                ("node_off_k", _VP), ("batch_size", ctypes.c_int32)]


class GccGinwLayer(ctypes.Structure):
    _fields_ = [("w0", _VP), ("w1", _VP), ("s0", _VP), ("t0", _VP), ("s1", _VP), ("t1", _VP), ("s2", _VP), ("t2", _VP),
                ("w0_frag", _VP), ("w1_frag", _VP)]


class GccGinwArgs(ctypes.Structure):
    _fields_ = [
        ("node_off", _VP), ("row_ptr", _VP), ("col_idx", _VP), ("x_in", _VP), ("x_out", _VP), ("pooled", _VP),
        ("batch_size", ctypes.c_int32), ("num_layers", ctypes.c_int32),
        ("layers", GccGinwLayer * 8),
        ("scratch", _VP), ("scratch_bytes", ctypes.c_int64), ("num_nodes", ctypes.c_int64),
    ]


class GccGinwEmbedArgs(ctypes.Structure):     # gcc_ginw_embed_args: the eval-mode embedding of a wide GIN encoder (csrc/gin_wide.hip)
    _fields_ = [
        ("num_views", ctypes.c_int32), ("batch_size", ctypes.c_int32), ("num_layers", ctypes.c_int32),
        ("pos_dim", ctypes.c_int32), ("deg_emb_dim", ctypes.c_int32), ("max_degree", ctypes.c_int32),
        ("edge_multiplicity", ctypes.c_int32), ("hidden", ctypes.c_int32), ("out_dim", ctypes.c_int32),
        ("normalize", ctypes.c_int32), ("norm_eps", ctypes.c_float),
        ("node_cap", ctypes.c_int64),
        ("node_off", _VP * 2), ("row_ptr", _VP * 2), ("col_idx", _VP * 2), ("seed_local", _VP * 2), ("pos", _VP * 2),
        ("degree_embedding", _VP),
        ("layers", GccGinwLayer * 8),
        ("pred_w", _VP * (GIN_MAX_LAYERS + 1)), ("pred_b", _VP * (GIN_MAX_LAYERS + 1)),
        ("pooled", _VP * 2), ("out", _VP),
        ("workspace", _VP), ("workspace_bytes", ctypes.c_int64),
    ]


STATUS_GINW_TOO_LARGE = 32
STATUS_GINW_BAD_EDGE = 64
STATUS_GINW_COUNT_OVERFLOW = 128


class GccClsHeadArgs(ctypes.Structure):      # gcc_cls_head_args: the fine-tuning head (csrc/cls_head.hip)
    _fields_ = [
        ("feat", _VP), ("W", _VP), ("b", _VP), ("labels", _VP),
        ("B", ctypes.c_int32), ("D", ctypes.c_int32), ("C", ctypes.c_int32), ("ld_feat", ctypes.c_int32),
        ("ld_dfeat", ctypes.c_int32),
        ("logits", _VP), ("dlogits", _VP), ("dW", _VP), ("db", _VP), ("dfeat", _VP), ("loss", _VP), ("correct", _VP),
        ("meter_acc", _VP), ("meter_max", _VP), ("node_off", _VP), ("edge_off", _VP),
        ("eval_loss_sum", _VP), ("eval_counts", _VP),
    ]


class GccSimArgs(ctypes.Structure):          # gcc_sim_args: similarity search (csrc/simsearch.hip)
    _fields_ = [
        ("emb_q", _VP), ("rows_q", ctypes.c_int64), ("ld_q", ctypes.c_int64),
        ("emb_c", _VP), ("rows_c", ctypes.c_int64), ("ld_c", ctypes.c_int64),
        ("q_idx", _VP), ("c_idx", _VP), ("target", _VP),
        ("mq", ctypes.c_int32), ("mc", ctypes.c_int32), ("D", ctypes.c_int32), ("k", ctypes.c_int32),
        ("normalize", ctypes.c_int32), ("splits", ctypes.c_int32),
        ("greater", _VP), ("equal_before", _VP), ("target_score", _VP), ("topk_col", _VP), ("topk_score", _VP),
    ]


SIM_MAX_DIM = 256
SIM_MAX_K = 64
SIM_MAX_SPLITS = 64
STATUS_SIM_ZERO_ROW = 1                      # gcc_sim_search's own status word
STATUS_SIM_BAD_INDEX = 2



class GccSvcArgs(ctypes.Structure):          # gcc_svc_args: C-SVC on frozen embeddings (csrc/svc.hip)
    _fields_ = [
        ("emb", _VP), ("ld", ctypes.c_int64),
        ("labels", _VP), ("fold_of_row", _VP), ("gamma", _VP),
        ("N", ctypes.c_int32), ("D", ctypes.c_int32), ("classes", ctypes.c_int32), ("folds", ctypes.c_int32),
        ("max_rows", ctypes.c_int32), ("iters_per_launch", ctypes.c_int32), ("iter_cap", ctypes.c_int32),
        ("reserved_", ctypes.c_int32),
        ("C", ctypes.c_double), ("eps", ctypes.c_double),
        ("pred", _VP), ("decision", _VP), ("iters", _VP), ("rho", _VP), ("obj", _VP), ("n_free", _VP), ("n_bounded", _VP),
        ("problem_rows", _VP), ("unfinished", _VP), ("first_rows", _VP), ("rows_out", _VP), ("alpha_out", _VP),
    ]


SVC_MAX_ROWS = 16384
SVC_MAX_DIM = 256
SVC_MAX_PROBLEM_ROWS = 4096
SVC_MAX_CLASSES = 32
SVC_MAX_FOLDS = 64
STATUS_SVC_BAD_LABEL = 1                     # the gcc_svc_* calls' own status word
STATUS_SVC_BAD_FOLD = 2
STATUS_SVC_MISSING_CLASS = 4
STATUS_SVC_NONFINITE = 8
STATUS_SVC_ITER_CAP = 16
STATUS_SVC_OVERFLOW = 32


class GccSvcSearchArgs(ctypes.Structure):    # gcc_svc_search_args: the grid search over C (csrc/svc.hip)
    _fields_ = [
        ("emb", _VP), ("ld", ctypes.c_int64),
        ("labels", _VP), ("fold_of_row", _VP), ("inner_of_row", _VP), ("gamma", _VP), ("inner_gamma", _VP), ("Cs", _VP),
        ("C_of_fold", _VP),
        ("N", ctypes.c_int32), ("D", ctypes.c_int32), ("classes", ctypes.c_int32), ("folds", ctypes.c_int32),
        ("inner", ctypes.c_int32), ("candidates", ctypes.c_int32), ("max_rows", ctypes.c_int32), ("max_inner_rows", ctypes.c_int32),
        ("iters_per_launch", ctypes.c_int32), ("iter_cap", ctypes.c_int32),
        ("eps", ctypes.c_double),
        ("unfinished", _VP), ("search_status", _VP), ("correct", _VP), ("search_iters", _VP), ("search_rho", _VP),
        ("search_problem_rows", _VP), ("search_first_rows", _VP), ("search_rows", _VP), ("search_alpha", _VP),
        ("pred", _VP), ("decision", _VP), ("iters", _VP), ("rho", _VP), ("obj", _VP), ("n_free", _VP), ("n_bounded", _VP),
        ("problem_rows", _VP), ("first_rows", _VP), ("rows_out", _VP), ("alpha_out", _VP),
    ]


SVC_SEARCH_MAX_CANDIDATES = 16
SVC_SEARCH_MAX_INNER = 16
SVC_SEARCH_MAX_PROBLEMS = 32768


class GccLogregArgs(ctypes.Structure):       # gcc_logreg_args: logistic regression on frozen embeddings (csrc/logreg.hip)
    _fields_ = [
        ("emb", _VP), ("ld", ctypes.c_int64),
        ("y", _VP), ("fold_of_row", _VP),
        ("N", ctypes.c_int32), ("D", ctypes.c_int32), ("classes", ctypes.c_int32), ("folds", ctypes.c_int32),
        ("iters_per_sync", ctypes.c_int32), ("iter_cap", ctypes.c_int32),
        ("C", ctypes.c_double), ("tol", ctypes.c_double), ("intercept_penalty", ctypes.c_double),
        ("pred", _VP), ("decision", _VP), ("counts", _VP), ("coef", _VP), ("intercept", _VP), ("iters", _VP), ("grad", _VP),
        ("state", _VP), ("unfinished", _VP),
    ]


LR_MAX_ROWS = 65536
LR_MAX_DIM = 256
LR_MAX_CLASSES = 256
LR_MAX_FOLDS = 16
STATUS_LR_BAD_FOLD = 1                       # the gcc_logreg_* calls' own status word
STATUS_LR_NONFINITE = 2
STATUS_LR_ITER_CAP = 4
STATUS_LR_PIVOT = 8
STATUS_LR_LINE_SEARCH = 16
(LR_RUNNING, LR_CONVERGED, LR_CAPPED, LR_ALL_ZERO, LR_ALL_ONE, LR_BAD_PIVOT, LR_NO_DECREASE, LR_NOT_RUN) = range(8)   # a problem's state

PRONE_MAX_DIM = 64
PRONE_OVERSAMPLE = 10
PRONE_MAX_STEP = 32
PRONE_SEGMENT = 32
PRONE_CHUNK = 1024
PRONE_MAX_CHUNK = 4096
(PRONE_MODE_F, PRONE_MODE_FT, PRONE_MODE_M, PRONE_MODE_A1) = range(4)
(PRONE_TAIL_NONE, PRONE_TAIL_HALF, PRONE_TAIL_CHEB) = range(3)
STATUS_PRONE_BAD_CSR = 1                     # the gcc_prone_* calls' own status word
STATUS_PRONE_DUPLICATE = 2
STATUS_PRONE_SPLIT_FULL = 4
STATUS_PRONE_RANK = 8
STATUS_PRONE_SWEEPS = 16
STATUS_PRONE_SINGULAR = 32


class GccProneArgs(ctypes.Structure):        # gcc_prone_args: ProNE node embeddings of a parent graph (csrc/prone.hip)
    _fields_ = [
        ("row_ptr", _VP), ("col_idx", _VP),
        ("n", ctypes.c_int64), ("nnz", ctypes.c_int64),
        ("d", ctypes.c_int32), ("step", ctypes.c_int32), ("chunk", ctypes.c_int32),
        ("mode", ctypes.c_int32), ("tail", ctypes.c_int32), ("k", ctypes.c_int32),
        ("mu", ctypes.c_double), ("alpha", ctypes.c_double), ("beta", ctypes.c_double),
        ("bessel", ctypes.c_double * PRONE_MAX_STEP),
        ("r", _VP), ("c", _VP),
        ("x", _VP), ("z", _VP), ("w", _VP),
        ("y", _VP), ("conv", _VP),
        ("rfac", _VP),
        ("omega", _VP),
        ("emb", _VP), ("emb32", _VP),
        ("sigma", _VP),
    ]


GRAPHWAVE_ORDER = 30
GRAPHWAVE_MAX_DIM = 256
GRAPHWAVE_MAX_NODES = 65536
GRAPHWAVE_MAX_WIDTH = 4096
GRAPHWAVE_ROW_BLOCK = 128
STATUS_GRAPHWAVE_BAD_CSR = 1                 # the gcc_graphwave_* calls' own status word


class GccGraphwaveArgs(ctypes.Structure):    # gcc_graphwave_args: GraphWave node embeddings of a parent graph (csrc/graphwave.hip)
    _fields_ = [
        ("row_ptr", _VP), ("col_idx", _VP),
        ("n_rows", ctypes.c_int64), ("nnz", ctypes.c_int64),
        ("d", ctypes.c_int32), ("width", ctypes.c_int32), ("heat_chunk", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("coeff", (ctypes.c_double * (GRAPHWAVE_ORDER + 1)) * 2),
        ("time_points", ctypes.c_double * (GRAPHWAVE_MAX_DIM // 4)),
        ("threshold", ctypes.c_double),
        ("chi", _VP), ("chi32", _VP),
        ("heat", _VP),
    ]


GRAPH_BUILD_WAVE_ROW = 64                    # the row classes of gcc_graph_build and its scan tile (csrc/graph_build.hip)
GRAPH_BUILD_LDS_ROW = 2048
GRAPH_BUILD_SCAN_TILE = 1024
STATUS_GRAPH_BUILD_BAD_ID = 1                # gcc_graph_build's own status word
STATUS_GRAPH_CHECK_SPAN = 1                  # gcc_graph_check's own status word
STATUS_GRAPH_CHECK_ZERO_DEGREE = 2
STATUS_GRAPH_CHECK_RANGE = 4
STATUS_GRAPH_CHECK_UNSORTED = 8
STATUS_GRAPH_CHECK_SELF_LOOP = 16
STATUS_GRAPH_CHECK_DUPLICATE = 32
STATUS_GRAPH_CHECK_ASYMMETRIC = 64


class GccGraphBuildArgs(ctypes.Structure):   # gcc_graph_build_args: edge lines -> the contract CSR (csrc/graph_build.hip)
    _fields_ = [
        ("pairs", _VP),
        ("n", ctypes.c_int64), ("m", ctypes.c_int64),
        ("row_ptr", _VP), ("col_idx", _VP), ("node_map", _VP), ("counts", _VP),
    ]


class GccGraphCheckArgs(ctypes.Structure):   # gcc_graph_check_args: the contract check on the device (csrc/graph_build.hip)
    _fields_ = [
        ("row_ptr", _VP), ("col_idx", _VP),
        ("n", ctypes.c_int64), ("nnz", ctypes.c_int64),
        ("multigraph", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("maxima", _VP),
    ]


CLS_HEAD_MAX_CLASSES = 64
CLS_HEAD_MAX_DIM = 256

GEMM_DTYPES = {"f32": 0, "bf16": 1}      # gcc_ginx_pass.gemm_dtype / gcc_ncex_forward_dt
ABI_VERSION = 3          # GCC_AMD_ABI_VERSION of the include/gcc_amd.h these structs mirror (checked in load())
GRAPH_CONTRACT_CHECKED = 1   # gcc_graph.flags

GAT_MAX_LAYERS = 8
GAT_MAX_S2S_LAYERS = 8


class GccGatWeights(ctypes.Structure):       # gcc_gat_weights: GraphEncoder(gnn_model="gat") (csrc/gat.hip)
    _fields_ = [
        ("num_layers", ctypes.c_int32), ("hidden", ctypes.c_int32), ("heads", ctypes.c_int32), ("out_dim", ctypes.c_int32),
        ("pos_dim", ctypes.c_int32), ("deg_emb_dim", ctypes.c_int32), ("max_degree", ctypes.c_int32),
        ("s2s_iters", ctypes.c_int32), ("s2s_layers", ctypes.c_int32), ("normalize", ctypes.c_int32),
        ("norm_eps", ctypes.c_float),
        ("degree_embedding", _VP),
        ("fc", _VP * GAT_MAX_LAYERS), ("attn_l", _VP * GAT_MAX_LAYERS), ("attn_r", _VP * GAT_MAX_LAYERS),
        ("w_ih", _VP * GAT_MAX_S2S_LAYERS), ("w_hh", _VP * GAT_MAX_S2S_LAYERS),
        ("b_ih", _VP * GAT_MAX_S2S_LAYERS), ("b_hh", _VP * GAT_MAX_S2S_LAYERS),
        ("ro0_w", _VP), ("ro0_b", _VP), ("ro2_w", _VP), ("ro2_b", _VP),
    ]


class GccGatGrads(ctypes.Structure):
    _fields_ = [
        ("degree_embedding", _VP),
        ("fc", _VP * GAT_MAX_LAYERS), ("attn_l", _VP * GAT_MAX_LAYERS), ("attn_r", _VP * GAT_MAX_LAYERS),
        ("w_ih", _VP * GAT_MAX_S2S_LAYERS), ("w_hh", _VP * GAT_MAX_S2S_LAYERS),
        ("b_ih", _VP * GAT_MAX_S2S_LAYERS), ("b_hh", _VP * GAT_MAX_S2S_LAYERS),
        ("ro0_w", _VP), ("ro0_b", _VP), ("ro2_w", _VP), ("ro2_b", _VP),
    ]


class GccGatPass(ctypes.Structure):
    _fields_ = [
        ("node_off", _VP), ("row_ptr", _VP), ("col_idx", _VP), ("seed_local", _VP), ("pos", _VP),
        ("batch_size", ctypes.c_int32), ("node_cap", ctypes.c_int32), ("edge_multiplicity", ctypes.c_int32),
        ("reserved_", ctypes.c_int32),
        ("saved", _VP), ("out", _VP),
    ]


# name -> (restype, argtypes); the single source of truth for the symbol test
GRAPH_TABLES_SCAN_TILE = 2048                # the tiles of gcc_graph_tables (nodes) and gcc_graph_tables_hub_adj (entries)
GRAPH_TABLES_ENTRY_TILE = 1024
GRAPH_TABLES_HUB_DEGREE = 512
GRAPH_TABLES_SUMMARY_WORDS = 8
STATUS_GRAPH_TABLES_EMPTY_SHARD = 1


class GccGraphTablesArgs(ctypes.Structure):  # gcc_graph_tables_args: the sampler's tables on the device (csrc/graph_tables.hip)
    _fields_ = [
        ("row_ptr", _VP), ("col_idx", _VP),
        ("n", ctypes.c_int64), ("nnz", ctypes.c_int64),
        ("shard_off", _VP),
        ("num_shards", ctypes.c_int32), ("hub_degree", ctypes.c_int32),
        ("max_hub_bytes", ctypes.c_int64),
        ("grid", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("summary", _VP), ("seed_cdf", _VP), ("hub_index", _VP), ("hub_adj", _VP),
        ("num_hubs", ctypes.c_int32), ("hub_words", ctypes.c_int32),
    ]


TEXT_TILE_BYTES = 4096                       # a tile of gcc_text_ints / gcc_text_line_ends and the tiles of a scan pass (csrc/text_ingest.hip)
TEXT_SCAN_TILES = 1024
TEXT_MAX_QUERIES = 16
STATUS_TEXT_NOT_INTEGER = 1                  # gcc_text_ints' own status word
STATUS_TEXT_INT32_RANGE = 2
STATUS_TEXT_SHORT = 4


class GccTextLineEndsArgs(ctypes.Structure):  # gcc_text_line_ends_args: the newlines that end given lines (csrc/text_ingest.hip)
    _fields_ = [
        ("text", _VP),
        ("nbytes", ctypes.c_int64), ("capacity", ctypes.c_int64),
        ("lines", ctypes.POINTER(ctypes.c_int64)),
        ("num_lines", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("ends", _VP),
    ]


class GccTextIntsArgs(ctypes.Structure):     # gcc_text_ints_args: tokens of text -> int32 records (csrc/text_ingest.hip)
    _fields_ = [
        ("text", _VP),
        ("nbytes", ctypes.c_int64), ("capacity", ctypes.c_int64),
        ("first_byte", ctypes.c_int64), ("max_tokens", ctypes.c_int64),
        ("fields", ctypes.c_int32), ("keep", ctypes.c_int32),
        ("out", _VP), ("summary", _VP),
    ]


STATUS_TEXT_LINE_SHAPE = 8                   # gcc_text_ints_sep with line_records: a record does not sit on a line of its own


class GccTextIntsSepArgs(ctypes.Structure):  # gcc_text_ints_sep_args: gcc_text_ints with a seventh separator and records on lines
    _fields_ = [("ints", GccTextIntsArgs), ("extra_sep", ctypes.c_int32), ("line_records", ctypes.c_int32)]


STATUS_TU_DESCENDS = 1                       # gcc_tu_corpus' own status word: a bit per ValueError of ingest.read_tudataset, in its order
STATUS_TU_GRAPH_COUNT = 2
STATUS_TU_BAD_ID = 4
STATUS_TU_SELF_LOOP = 8
STATUS_TU_CROSS_GRAPH = 16
STATUS_TU_REPEATED = 32
STATUS_TU_ASYMMETRIC = 64


class GccTuCorpusArgs(ctypes.Structure):     # gcc_tu_corpus_args: a TU dataset's integers -> the resident corpus (csrc/tu_corpus.hip)
    _fields_ = [
        ("pairs", _VP), ("indicator", _VP), ("graph_labels", _VP),
        ("num_nodes", ctypes.c_int64), ("num_lines", ctypes.c_int64), ("num_labels", ctypes.c_int64),
        ("node_first", _VP), ("edge_first", _VP), ("row_ptr", _VP), ("col_idx", _VP), ("seed_local", _VP), ("labels", _VP),
        ("counts", _VP),
    ]


SIGNATURES = {
    "gcc_abi_version": (ctypes.c_int32, []),
    "gcc_last_error": (ctypes.c_char_p, []),
    "gcc_stream_create_cu_mask": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p)]),
    "gcc_stream_destroy": (ctypes.c_int32, [ctypes.c_void_p]),
    "gcc_prof_create": (ctypes.c_void_p, [ctypes.c_int32]),
    "gcc_prof_destroy": (None, [ctypes.c_void_p]),
    "gcc_prof_elapsed_ms": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, c_f32p]),
    "gcc_sampler_workspace_bytes": (ctypes.c_int64, [ctypes.POINTER(GccGraph), ctypes.c_int32, ctypes.c_int64]),
    "gcc_sampler_workspace_bytes_multi": (ctypes.c_int64, [ctypes.POINTER(GccGraph), ctypes.c_int32, ctypes.c_int32, ctypes.c_int64]),
    "gcc_sample_multi": (ctypes.c_int32, [
        ctypes.POINTER(GccGraph), ctypes.POINTER(GccSampleParams), ctypes.c_int32, ctypes.c_int64, ctypes.POINTER(GccBatchOut),
        ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "gcc_sample_batch": (ctypes.c_int32, [
        ctypes.POINTER(GccGraph), ctypes.POINTER(GccSampleParams), ctypes.POINTER(GccBatchOut),
        ctypes.POINTER(GccBatchOut), ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
        ctypes.c_void_p]),
    "gcc_posemb_workspace_bytes": (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int64, ctypes.c_int32]),
    "gcc_posemb_debug_ticks": (None, [ctypes.c_void_p]),
    "gcc_posemb_set_fork": (None, [ctypes.c_int32]),
    "gcc_sampler_debug_ticks": (None, [ctypes.c_void_p]),
    "gcc_sampler_debug_grids": (None, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    "gcc_debug_load": (ctypes.c_int32, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32,
                                        ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "gcc_gin_debug_ticks": (None, [ctypes.c_void_p]),
    "gcc_ginw_debug_ticks": (None, [ctypes.c_void_p]),
    "gcc_posemb_multi_workspace_bytes": (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32]),
    "gcc_posemb_multi": (ctypes.c_int32, [ctypes.POINTER(GccPosembView), ctypes.c_int32, ctypes.c_int32, ctypes.c_int64,
                                          ctypes.c_int32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p]),
    "gcc_posemb_multi_gated": (ctypes.c_int32, [ctypes.POINTER(GccPosembView), ctypes.c_int32, ctypes.c_int32, ctypes.c_int64,
                                          ctypes.c_int32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gcc_posemb": (ctypes.c_int32, [ctypes.POINTER(GccBatchOut), ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                    ctypes.c_void_p, ctypes.c_void_p]),
    "gcc_gin_forward": (ctypes.c_int32, [ctypes.POINTER(GccGinPass), ctypes.c_int32, ctypes.c_void_p,
                                         ctypes.c_void_p]),
    "gcc_gin_forward_fetch": (ctypes.c_int32, [ctypes.POINTER(GccGinPass), ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gcc_gin_backward_workspace_bytes": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]),
    "gcc_gin_backward": (ctypes.c_int32, [ctypes.POINTER(GccGinPass), ctypes.c_void_p, ctypes.POINTER(GccGinGrads),
                                          ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                          ctypes.c_void_p, ctypes.c_void_p]),
    "gcc_gin_backward_sumsq": (ctypes.c_int32, [ctypes.POINTER(GccGinPass), ctypes.c_void_p, ctypes.POINTER(GccGinGrads),
                                                ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int32,
                                                c_i32p, ctypes.c_void_p, ctypes.c_void_p]),
    "gcc_ginx_workspace_bytes": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    "gcc_ginx_forward": (ctypes.c_int32, [ctypes.POINTER(GccGinxPass), ctypes.c_void_p]),
    "gcc_ginx_backward": (ctypes.c_int32, [ctypes.POINTER(GccGinxPass), ctypes.c_void_p, ctypes.POINTER(GccGinGrads), ctypes.c_void_p]),
    "gcc_ncex_forward": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                          ctypes.c_float, ctypes.c_int32] + [ctypes.c_void_p] * 8),
    "gcc_ncex_forward_dt": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                             ctypes.c_float, ctypes.c_int32] + [ctypes.c_void_p] * 7 + [ctypes.c_int32, ctypes.c_void_p]),
    "gcc_queue_enqueue_x": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                             ctypes.c_void_p]),
    "gcc_ginw_forward": (ctypes.c_int32, [ctypes.POINTER(GccGinwArgs), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gcc_ginw_pack_weights": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]),
    "gcc_nce_workspace_bytes": (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int32]),
    "gcc_nce_forward": (ctypes.c_int32, [ctypes.POINTER(GccNceArgs), ctypes.c_void_p, ctypes.c_int64,
                                         ctypes.c_void_p, ctypes.c_void_p]),
    "gcc_nce_backward": (ctypes.c_int32, [ctypes.POINTER(GccNceArgs), ctypes.c_void_p, ctypes.c_int32,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                          ctypes.c_void_p]),
    "gcc_nce_forward_backward": (ctypes.c_int32, [ctypes.POINTER(GccNceArgs), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gcc_queue_enqueue": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                           ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]),
    "gcc_adam_step": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_int64, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                       ctypes.c_float, ctypes.c_int32, ctypes.c_float, ctypes.c_float, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_void_p]),
    "gcc_adam_ema_step": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_int64, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                           ctypes.c_float, ctypes.c_int32, ctypes.c_float, ctypes.c_float, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_float,
                                           ctypes.POINTER(GccStepMetersArgs), ctypes.c_void_p]),
    "gcc_adam_ema_step_scalars": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                   ctypes.c_int64, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                                   ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_void_p,
                                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_float,
                                                   ctypes.POINTER(GccStepMetersArgs), ctypes.c_void_p, ctypes.c_void_p]),
    "gcc_adam_ema_enqueue_step_scalars": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                           ctypes.c_int64, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                                           ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_void_p,
                                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_float,
                                                           ctypes.POINTER(GccStepMetersArgs), ctypes.c_void_p, ctypes.c_void_p,
                                                           ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                                           ctypes.c_int32, ctypes.c_void_p]),
    "gcc_queue_enqueue_scalars": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                                   ctypes.c_void_p, ctypes.c_void_p]),
    "gcc_ginw_scratch_bytes": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32]),
    "gcc_ginw_embed_workspace_bytes": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32]),
    "gcc_ginw_embed": (ctypes.c_int32, [ctypes.POINTER(GccGinwEmbedArgs), ctypes.c_void_p, ctypes.c_void_p]),
    "gcc_gin_eval_debug_ticks": (None, [ctypes.c_void_p]),
    "gcc_gin_eval_fused": (ctypes.c_int32, [ctypes.POINTER(GccGinPass), ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]),
    "gcc_step_scalars_fill": (None, [ctypes.c_void_p, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_int32,
                                      ctypes.c_int32, ctypes.c_uint64]),
    "gcc_step_scalars_fetch": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]),
    "gcc_step_scalars_set": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_int32,
                                              ctypes.c_int32, ctypes.c_uint64, ctypes.c_void_p]),
    "gcc_step_meters": (ctypes.c_int32, [ctypes.c_void_p] * 8 + [ctypes.c_int32, ctypes.c_void_p]),
    "gcc_ema_update": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_float,
                                        ctypes.c_void_p]),
    "gcc_gat_saved_floats": (ctypes.c_int64, [ctypes.POINTER(GccGatWeights), ctypes.c_int32, ctypes.c_int32]),
    "gcc_gat_forward": (ctypes.c_int32, [ctypes.POINTER(GccGatPass), ctypes.POINTER(GccGatWeights), ctypes.c_void_p]),
    "gcc_gat_backward_workspace_bytes": (ctypes.c_int64, [ctypes.POINTER(GccGatWeights), ctypes.c_int32, ctypes.c_int32]),
    "gcc_gat_backward": (ctypes.c_int32, [ctypes.POINTER(GccGatPass), ctypes.POINTER(GccGatWeights), ctypes.c_void_p,
                                          ctypes.POINTER(GccGatGrads), ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64,
                                          ctypes.c_void_p]),
    "gcc_cls_head_train": (ctypes.c_int32, [ctypes.POINTER(GccClsHeadArgs), ctypes.c_void_p]),
    "gcc_cls_head_eval": (ctypes.c_int32, [ctypes.POINTER(GccClsHeadArgs), ctypes.c_void_p]),
    "gcc_adam_clipvalue_step": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                 ctypes.c_int64, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                                 ctypes.c_float, ctypes.c_int32, ctypes.c_float, ctypes.c_float, ctypes.c_void_p]),
    # rule, param, grad, state, n, lr, hyper, weight_decay, max_norm, grad_scale, grad_norm, scratch, [ema, n_ema, ema_m, meters,] stream
    "gcc_opt_step": (ctypes.c_int32, [ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64] +
                     [ctypes.c_float] * 5 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gcc_opt_ema_step": (ctypes.c_int32, [ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64] +
                         [ctypes.c_float] * 5 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_float,
                                                 ctypes.POINTER(GccStepMetersArgs), ctypes.c_void_p]),
    "gcc_opt_ema_step_scalars": (ctypes.c_int32, [ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64] +
                                 [ctypes.c_float] * 4 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                                         ctypes.c_float, ctypes.POINTER(GccStepMetersArgs), ctypes.c_void_p,
                                                         ctypes.c_void_p]),
    "gcc_opt_clipvalue_step": (ctypes.c_int32, [ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64] +
                               [ctypes.c_float] * 5 + [ctypes.c_void_p]),
    "gcc_pack_graphs": (ctypes.c_int32, [ctypes.POINTER(GccGraphCorpus), ctypes.c_void_p, ctypes.c_int32,
                                         ctypes.POINTER(GccBatchOut), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]),
    "gcc_sim_workspace_bytes": (ctypes.c_int64, [ctypes.c_int32] * 5),
    "gcc_sim_search": (ctypes.c_int32, [ctypes.POINTER(GccSimArgs), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                        ctypes.c_void_p]),
    "gcc_svc_workspace_bytes": (ctypes.c_int64, [ctypes.c_int32] * 5),
    "gcc_svc_distances": (ctypes.c_int32, [ctypes.POINTER(GccSvcArgs), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                           ctypes.c_void_p]),
    "gcc_svc_solve": (ctypes.c_int32, [ctypes.POINTER(GccSvcArgs), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                       ctypes.c_void_p]),
    "gcc_svc_predict": (ctypes.c_int32, [ctypes.POINTER(GccSvcArgs), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                         ctypes.c_void_p]),
    "gcc_svc_search_workspace_bytes": (ctypes.c_int64, [ctypes.c_int32] * 8),
    **{name: (ctypes.c_int32, [ctypes.POINTER(GccSvcSearchArgs), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p])
       for name in ("gcc_svc_search_setup", "gcc_svc_search_solve", "gcc_svc_search_score", "gcc_svc_search_refit",
                    "gcc_svc_search_predict")},
    "gcc_logreg_workspace_bytes": (ctypes.c_int64, [ctypes.c_int32] * 4),
    "gcc_logreg_setup": (ctypes.c_int32, [ctypes.POINTER(GccLogregArgs), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                          ctypes.c_void_p]),
    "gcc_logreg_step": (ctypes.c_int32, [ctypes.POINTER(GccLogregArgs), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                         ctypes.c_void_p]),
    "gcc_logreg_predict": (ctypes.c_int32, [ctypes.POINTER(GccLogregArgs), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                            ctypes.c_void_p]),
    "gcc_prone_workspace_bytes": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32]),
    "gcc_prone_node_terms": (ctypes.c_int32, [ctypes.POINTER(GccProneArgs), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                              ctypes.c_void_p]),
    "gcc_prone_spmm": (ctypes.c_int32, [ctypes.POINTER(GccProneArgs), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                        ctypes.c_void_p]),
    "gcc_prone_orthonormalize": (ctypes.c_int32, [ctypes.POINTER(GccProneArgs), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                                  ctypes.c_void_p]),
    "gcc_prone_embed": (ctypes.c_int32, [ctypes.POINTER(GccProneArgs), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                         ctypes.c_void_p]),
    "gcc_graphwave_panel_width": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]),
    "gcc_graphwave_workspace_bytes": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]),
    "gcc_graphwave_heat": (ctypes.c_int32, [ctypes.POINTER(GccGraphwaveArgs), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                            ctypes.c_void_p]),
    "gcc_graphwave_embed": (ctypes.c_int32, [ctypes.POINTER(GccGraphwaveArgs), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                             ctypes.c_void_p]),
    "gcc_graph_build_workspace_bytes": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64]),
    "gcc_graph_build": (ctypes.c_int32, [ctypes.POINTER(GccGraphBuildArgs), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                         ctypes.c_void_p]),
    "gcc_graph_check": (ctypes.c_int32, [ctypes.POINTER(GccGraphCheckArgs), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                         ctypes.c_void_p]),
    "gcc_graph_tables_workspace_bytes": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32]),
    "gcc_graph_tables": (ctypes.c_int32, [ctypes.POINTER(GccGraphTablesArgs), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                          ctypes.c_void_p]),
    "gcc_graph_tables_hub_adj": (ctypes.c_int32, [ctypes.POINTER(GccGraphTablesArgs), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                                  ctypes.c_void_p]),
    "gcc_text_line_ends_workspace_bytes": (ctypes.c_int64, [ctypes.c_int64]),
    "gcc_text_ints_workspace_bytes": (ctypes.c_int64, [ctypes.c_int64]),
    "gcc_text_line_ends": (ctypes.c_int32, [ctypes.POINTER(GccTextLineEndsArgs), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                            ctypes.c_void_p]),
    "gcc_text_ints": (ctypes.c_int32, [ctypes.POINTER(GccTextIntsArgs), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                       ctypes.c_void_p]),
    "gcc_text_ints_sep": (ctypes.c_int32, [ctypes.POINTER(GccTextIntsSepArgs), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                           ctypes.c_void_p]),
    "gcc_tu_corpus_workspace_bytes": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64]),
    "gcc_tu_corpus": (ctypes.c_int32, [ctypes.POINTER(GccTuCorpusArgs), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                       ctypes.c_void_p]),
}
# symbols declared in the header but not built yet are listed here while the build is in progress
PENDING = set()


def declare(lib: ctypes.CDLL) -> ctypes.CDLL:
    """Attach restype/argtypes for every symbol of include/gcc_amd.h."""
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)   # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    return lib


_lib = None


def load() -> ctypes.CDLL:
    """Open the gfx950 library built in-tree by ``__graft_entry__.build()``."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  gcc_amd has no CPU fallback.")
        # PyTorch first: its wheel bundles its own libamdhip64.  If this library were opened before torch, the loader would
        # satisfy its libamdhip64 dependency from /opt/rocm and the process would hold TWO HIP runtimes -- kernels
        # registered with one, torch's streams and allocations owned by the other ("no ROCm-capable device is detected"
        # at the first launch; seen when build() and smoke() ran in one process).
        import torch  # noqa: F401

        lib = declare(ctypes.CDLL(LIB_PATH))
        got = lib.gcc_abi_version()
        if got != ABI_VERSION:             # the ctypes structs below mirror ONE layout of include/gcc_amd.h
            raise RuntimeError(f"{LIB_PATH} reports C-ABI version {got}, this binding was written for {ABI_VERSION}: "
                               "rebuild the library (python -c 'import __graft_entry__ as g; g.build()')")
        _lib = lib
    return _lib


def call(lib, name: str, *args) -> None:
    """``lib.<name>(*args)`` for a symbol that returns 0 on success.  ``lib`` is the library the CALLER holds (an engine's
    own ``self.lib``: the HIP library, or the emulator build a test injected), so the error text is that library's."""
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise RuntimeError(error_text(lib, name, rc))


def size_query(lib, name: str, *args, named=True) -> int:
    """``lib.<name>(*args)`` for a symbol that returns an int64 size, negative on error.  ``named=False``: the bare error text
    (what gcc_ginx_workspace_bytes has always raised)."""
    n = getattr(lib, name)(*args)
    if n < 0:
        raise RuntimeError(error_text(lib, name, n) if named else lib.gcc_last_error().decode())
    return n


def error_text(lib, name, rc):
    return f"{name} failed ({rc}): {lib.gcc_last_error().decode()}"


def node_cap(g) -> int:
    """rows of a batch's per-node arrays (a sampler batch carries ``parent_nid``, the hand-built ones only ``graph_id``)"""
    return g.parent_nid.numel() if hasattr(g, "parent_nid") else g.graph_id.numel()


# What an encoder call passes down of one batch (bind_batch): six addresses (None where absent), the scalars that go with them, and
# ``keep``: tensors the addresses point into that the batch itself does not hold (the col_idx stand-in)
BatchBinding = namedtuple("BatchBinding", "node_off row_ptr col_idx graph_id pos seed_local batch_size node_cap edge_multiplicity "
                                          "device keep")


def bind_batch(g, ptr, *, need_pos=True, need_graph_id=False, col_placeholder=False) -> BatchBinding:
    """The one place that turns a batch -- a :class:`gcc_amd.sampler.BatchedCSR`, or a hand-built object with its members -- into
    the fields of an encoder call's struct.  ``ptr`` maps a tensor to its address (an engine's ``self.ptr``).  Hand-built batches
    may lack ``parent_nid`` (the capacity is then ``graph_id``'s length), ``seed_local`` (None) and ``edge_multiplicity`` (1).
    Enforces the capacity rule from the tensors' shapes alone, without a host read of device memory: the
    kernels clamp a workgroup's first-tile loads to the capacity, not to the live node count; longer arrays are fine.
    ``col_placeholder``: some C calls refuse the null address of an empty ``col_idx``; one int32 element stands in for it."""
    pos = getattr(g, "pos_undirected", None)
    if need_pos and pos is None:
        raise RuntimeError("the batch has no pos_undirected (run the positional embedding first)")
    cap = node_cap(g)
    if g.row_ptr.numel() <= cap:
        _too_short("row_ptr", g.row_ptr.numel(), cap + 1, cap)
    if need_graph_id and g.graph_id.numel() < cap:
        _too_short("graph_id", g.graph_id.numel(), cap, cap)
    if need_pos and pos.shape[0] < cap:
        _too_short("pos_undirected", pos.shape[0], cap, cap)
    device = g.node_off.device
    col_idx, keep = g.col_idx, ()
    if col_placeholder and col_idx.numel() == 0:
        import torch

        col_idx = torch.zeros(1, dtype=torch.int32, device=device)
        keep = (col_idx,)
    seed_local = getattr(g, "seed_local", None)
    return BatchBinding(ptr(g.node_off), ptr(g.row_ptr), ptr(col_idx), ptr(g.graph_id) if need_graph_id else None,
                        ptr(pos) if need_pos else None, ptr(seed_local) if seed_local is not None else None, g.batch_size, cap,
                        int(getattr(g, "edge_multiplicity", 1)), device, keep)


def _too_short(name, have, need, cap):
    raise RuntimeError(f"the batch's {name} has {have} rows, its node capacity of {cap} needs at least {need}: row_ptr holds capacity + 1 "
                       "entries, graph_id and pos_undirected capacity rows (capacity = parent_nid.numel(), or graph_id.numel() without "
                       "parent_nid) -- the kernels' first-tile loads are clamped to the capacity, not to the live node count")


def batch_out(g, ptr, node_cap, csr_only=False) -> GccBatchOut:
    """gcc_batch_out of a batch's arrays: all six (the sampler's output buffers), or ``csr_only`` -- node_off, row_ptr and col_idx,
    what the positional embedding reads.  ``node_cap``: rows of the per-node arrays; edge_cap is ``col_idx``'s length."""
    rest = {} if csr_only else dict(edge_off=ptr(g.edge_off), parent_nid=ptr(g.parent_nid), graph_id=ptr(g.graph_id))
    return GccBatchOut(node_off=ptr(g.node_off), row_ptr=ptr(g.row_ptr), col_idx=ptr(g.col_idx), node_cap=node_cap,
                       edge_cap=g.col_idx.numel(), **rest)


def raw_stream(where):
    """the raw handle of torch's current stream on the device of ``where`` (a tensor or a device); None off the GPU"""
    import torch

    dev = where.device if isinstance(where, torch.Tensor) else torch.device(where)
    return torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None


def dev_ptr(t, dtype=None) -> int:
    """data_ptr() of a contiguous CUDA (HIP) tensor; anything else is refused."""
    import torch

    if t is None:
        return 0
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("gcc_amd kernels take device (HIP) tensors only; there is no CPU path")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError("tensor must be contiguous")
    return t.data_ptr()
