/*
 * include/gcc_amd.h -- C ABI of libgcc_amd.so, the MI355X-native GCC
 * pre-training hot path (RWR ego-net sampler -> batcher -> GIN encoder ->
 * MoCo/InfoNCE head).
 *
 * The reference (THUDM/GCC) is pure Python and has no FFI of its own
 * (SURVEY.md §8b), so there is no existing binding to match; each entry point
 * below names the reference call site whose native work it replaces.  The
 * reference-side glue is the ctypes stub in gcc_amd/_cabi.py (shown in
 * INTEGRATION.md).
 *
 * Conventions
 *   - plain pointers + sizes only; every pointer marked "device" is HBM memory
 *     owned by the caller (the Python host allocates it with torch and passes
 *     data_ptr()); the library allocates nothing and keeps no state.
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*;
 *     NULL = the null stream) and performs no host synchronisation.
 *   - return value 0 = launched; <0 = argument error (gcc_last_error()).
 *     Capacity overflows detected on the device are reported through the
 *     caller's `status` words (GCC_STATUS_*), never by writing out of bounds.
 */
#ifndef GCC_AMD_H
#define GCC_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3: gcc_gin_pass.{node_cap,rows_hint}.
 * 2: gcc_sample_params.{hub_degree,max_hubs}, gcc_gin_weights.hidden, gcc_gin_pass.scalars, gcc_ginw_args.{scratch,
 * scratch_bytes,num_nodes}, gcc_graph.{flags,hub_index,hub_adj,num_hubs,hub_words,hub_table_degree}.  A caller built against another version must not pass its structs:
 * compare gcc_abi_version() with the header's constant after loading (gcc_amd/_cabi.py does). */
#define GCC_AMD_ABI_VERSION 3

/* bits of the device status word */
#define GCC_STATUS_SCRATCH_OVERFLOW 1  /* induction scratch too small            */
#define GCC_STATUS_NODE_OVERFLOW    2  /* a view needs more than node_cap nodes  */
#define GCC_STATUS_EDGE_OVERFLOW    4  /* a view needs more than edge_cap edges  */

int32_t gcc_abi_version(void);
const char *gcc_last_error(void);

/* -------------------------------------------------------------- profiling ---
 * A ring of hipEvents the kernels' launch functions record between kernels
 * when a call's `prof` argument is non-NULL (bench.py's live per-kernel
 * durations; no counterpart in the reference, whose only timers are the
 * BT/DT wall-clock meters of train.py:367-368). */
typedef struct gcc_prof gcc_prof;
gcc_prof *gcc_prof_create(int32_t num_marks);
void gcc_prof_destroy(gcc_prof *p);
/* milliseconds between two recorded marks; synchronises on `to_mark`. */
int32_t gcc_prof_elapsed_ms(gcc_prof *p, int32_t from_mark, int32_t to_mark, float *ms);

/* -------------------------------------------------------------- streams ---
 * A HIP stream whose kernels may only run on the compute units set in
 * `cu_mask` (bit i of word i / 32; `words` 32-bit words, 256 CUs = 8 words).
 * The host layer gives the (few) data-pipeline streams a mask that leaves some
 * compute units to the training step alone (the reference gets this isolation
 * for free: its pipeline runs on CPU workers, train.py:577-586).
 * Returns 0 and the hipStream_t in *stream. */
int32_t gcc_stream_create_cu_mask(const uint32_t *cu_mask, int32_t words, void **stream);
/* diagnostics (tools/load_probe.py): a synthetic co-tenant -- `workgroups` workgroups of `threads` threads and `lds_bytes` of LDS that
 * spend `ticks` of the 100 MHz clock (at most max_iters rounds) on kind 0: barriers + LDS, 1: float4 reads streamed over buf, 2: FMA chains */
int32_t gcc_debug_load(int32_t kind, int32_t workgroups, int32_t threads, int32_t lds_bytes, int64_t ticks, int32_t max_iters,
                       const float *buf, int64_t buf_floats, float *sink, void *stream);
int32_t gcc_stream_destroy(void *stream);

/* ---------------------------------------------------------------- graph ---
 * The parent graph in the layout x2dgl.py:39-62 guarantees (symmetric, no self
 * loops, no duplicates, no zero-degree nodes, rows sorted), resident in HBM.
 * Replaces the per-worker dgl.data.utils.load_graphs copy of
 * gcc/datasets/graph_dataset.py:23-30. */
typedef struct gcc_graph {
    const int32_t *row_ptr;   /* device [num_nodes + 1]                               */
    const int32_t *col_idx;   /* device [num_edges]                                   */
    const double  *seed_cdf;  /* device [num_nodes]: cumsum(deg^0.75)/sum, float64    */
                              /*   (graph_dataset.py:86-90); with worker shards: each */
                              /*   shard's own cdf over its node range (ends at 1.0)  */
    const int32_t *ltab;      /* device [ltab_len]: max_nodes_per_seed by in-degree,  */
                              /*   index clamped to ltab_len-1 (graph_dataset.py:113-124) */
    int64_t num_nodes;
    int64_t num_edges;
    int32_t ltab_len;
    int32_t lmax;             /* max(ltab): sizes LDS and per-subgraph capacities     */
    /* Worker shards of LoadBalanceGraphDataset (graph_dataset.py:23-30,63-76): the corpus' graphs are laid out shard
     * by shard, shard s = nodes [shard_off[s], shard_off[s+1]); DataLoader batch i (= sample ids [i*bsz, (i+1)*bsz))
     * draws its seeds from shard i % num_shards only.  num_shards <= 1 (shard_off may be NULL): one shard = all. */
    const int64_t *shard_off; /* device [num_shards + 1] or NULL                      */
    int32_t num_shards;
    int32_t flags;            /* GCC_GRAPH_* bits                                     */
    /* Optional (NULL / 0: off): adjacency among the parent's high-degree rows, built once at upload.  The induction does not
     * scan a subgraph's hub rows; the edges BETWEEN two of them used to cost one search per pair in the shorter row (8-14
     * dependent loads; 55 of the walk launch's 120 us on the 1M-node graph) and are one bit probe with this table.  Used when
     * the call's effective hub_degree is >= hub_table_degree (every hub is in the table then). */
    const int32_t  *hub_index;        /* device [num_nodes]: index among the rows of degree >= hub_table_degree, -1 otherwise */
    const uint32_t *hub_adj;          /* device [num_hubs][hub_words]: bit (c & 31) of word c >> 5 of row a: hubs a, c adjacent */
    int32_t num_hubs, hub_words;      /* hub_words = (num_hubs + 31) / 32                                                      */
    int32_t hub_table_degree, reserved_;
} gcc_graph;
/* The caller has verified the contract above (symmetric, rows sorted ascending, no self loops, no duplicates).  Only
 * then may the induction skip hub rows (gcc_sample_params.hub_degree >= 0): their induced rows are rebuilt as mirror
 * images of the other rows' hits, which is the DGL-consistent subgraph on such a graph only.  Without the bit every
 * member row is scanned whatever hub_degree says (the result is then the induced subgraph of ANY sorted-row CSR).
 *
 * What an UNCHECKED parent may hold: a multigraph.  Parallel edges are repeated entries of a row; rows are sorted
 * non-decreasing, so the copies of an edge are adjacent; no self loops, no empty rows, and every pair has the same
 * number of copies in both directions (gcc_amd.graphgen.check_multigraph_contract).  A uniform draw over a row's
 * entries is then DGL's walk on the multigraph, the induction emits every copy (an induced row can hold MORE than
 * n - 1 entries: size edge_cap and the scratch for that, overflow sets the usual status bits), the positional
 * embedding's matrix is copies(i, j) / sqrt(d_i d_j) with d = row length, and the encoders take every entry as an
 * edge of its own.  Such a parent must never carry the bit: the hub-row short cut mirrors one hit per pair. */
#define GCC_GRAPH_CONTRACT_CHECKED 1

/* --------------------------------------------------------------- sampler ---
 * One call = one DataLoader batch of LoadBalanceGraphDataset
 * (graph_dataset.py:85-179 + data_util.py:26-32,218-239, minus the positional
 * embedding which is gcc_posemb_*): draw batch_size seeds, run two independent
 * random walks with restart per seed (views q and k), build both induced
 * subgraphs and emit two batched CSRs.  Bit-exact against
 * oracle/sampler_oracle.c for the RNG spec written there. */
typedef struct gcc_sample_params {
    uint64_t run_seed;         /* Philox key                                          */
    int64_t  first_sample_id;  /* global index of sample 0 of this batch              */
    int32_t  batch_size;       /* B samples -> 2B subgraphs                           */
    uint32_t restart_u32;      /* floor(restart_prob * 2^32)                          */
    const int32_t *seeds;      /* device [B] or NULL; non-NULL overrides the seed draw */
    gcc_prof *prof;            /* NULL, or marks 0..3 recorded around walk/induce/pack */
    int32_t hub_degree;        /* member rows of at least this parent degree are NOT scanned by the induction: the graph is
                                * symmetric, so their induced rows are the mirror images of the other rows' hits + one search
                                * per pair of hubs -- same result bit for bit, fewer bytes scanned on power-law graphs.
                                * 0 = default (512), < 0 = scan every row */
    int32_t max_hubs;          /* most such rows per subgraph (1..32; 0 = default, 32): with more rows over hub_degree the
                                * subgraph's own threshold rises to the power of two that leaves at most this many */
} gcc_sample_params;

/* One view's batched graph = dgl.batch(list of subgraphs), data_util.py:26-32.
 * Node i of subgraph b is global node node_off[b] + i; node_off[b] itself is
 * the seed (data_util.py:226,238). */
typedef struct gcc_batch_out {
    int32_t *node_off;    /* device [B + 1]                                           */
    int32_t *edge_off;    /* device [B + 1]                                           */
    int32_t *parent_nid;  /* device [node_cap]: id in the parent graph                */
    int32_t *graph_id;    /* device [node_cap]: subgraph index of each node           */
    int32_t *row_ptr;     /* device [node_cap + 1]                                    */
    int32_t *col_idx;     /* device [edge_cap]: global (batched) node ids             */
    int64_t  node_cap;
    int64_t  edge_cap;
} gcc_batch_out;

/* bytes of caller-provided workspace needed for batch_size samples with
 * scratch_entries int32 slots of induction scratch (one 1024-entry slot per unit of 256 aligned quads of the members'
 * parent rows: about the sum of the members' parent degrees over all subgraphs of the call). */
int64_t gcc_sampler_workspace_bytes(const gcc_graph *g, int32_t batch_size, int64_t scratch_entries);
/* ... for calls that cover num_steps consecutive DataLoader batches (gcc_sample_multi) */
#define GCC_SAMPLE_MAX_STEPS 16
int64_t gcc_sampler_workspace_bytes_multi(const gcc_graph *g, int32_t batch_size, int32_t num_steps, int64_t scratch_entries);

/* diagnostics: subsequent gcc_sample_batch calls add wall-clock ticks (100 MHz) of induce_kernel's phases into device
 * int64[16] ([0] prefix sums over the subgraphs, [1] hash map + row prefix sums, [2] segment scans, [15] workgroups). */
void gcc_sampler_debug_ticks(long long *device_ticks64);
/* tests only: cap the static grids of the two induce classes and of the big walk class (0 = the defaults), so that small
 * test batches exercise workgroups that walk through several virtual workgroups, subgraphs and list entries */
void gcc_sampler_debug_grids(int32_t small_grid, int32_t big_grid, int32_t walk_big_grid);

/* status: device int32[1], OR-ed with GCC_STATUS_* bits (caller zeroes it). */
int32_t gcc_sample_batch(const gcc_graph *g, const gcc_sample_params *p,
                         const gcc_batch_out *out_q, const gcc_batch_out *out_k,
                         void *workspace, int64_t workspace_bytes, int64_t scratch_entries,
                         int32_t *status, void *stream);

/* The batches of num_steps consecutive DataLoader steps in ONE launch set: step t samples the ids
 * p->first_sample_id + t * sample_id_stride + [0, batch_size) (stride = world * batch_size for a rank of a data-parallel
 * job) into outs[2 t] (view q) and outs[2 t + 1] (view k); p->seeds, if given, holds num_steps * batch_size seeds.
 * Every subgraph is the one gcc_sample_batch would produce for the same sample id (bit for bit); what changes is the
 * cost: the five kernels of a call are latency chains that a single step's 2 * batch_size subgraphs cannot fill the
 * GPU with (the reference's DataLoader prefetches whole batches ahead the same way, train.py:577-586).
 * num_steps <= GCC_SAMPLE_MAX_STEPS and 2 * batch_size * num_steps <= 16383; scratch_entries covers the whole call. */
int32_t gcc_sample_multi(const gcc_graph *g, const gcc_sample_params *p, int32_t num_steps, int64_t sample_id_stride,
                         const gcc_batch_out *outs, void *workspace, int64_t workspace_bytes, int64_t scratch_entries,
                         int32_t *status, void *stream);

/* --------------------------------------------------- positional embedding ---
 * _add_undirected_graph_positional_embedding + eigen_decomposision of
 * gcc/datasets/data_util.py:242-281 for every subgraph of a batched graph:
 * the k = min(n - 2, hidden) largest-algebraic eigenpairs of D^-1/2 A D^-1/2
 * (D = in-degree clipped at 1), eigenvalues ascending like scipy eigsh(which="LA"),
 * rows L2-normalised, zero-padded to `hidden` columns; k <= 0 gives zeros.
 * Twin leaves are deflated exactly first (their contrasts are null vectors).
 * Deflated size n' <= GCC_POSEMB_DIRECT_MAX: direct symmetric eigensolver
 * (tridiagonalisation, bisection, inverse iteration: exact multiplicities), the
 * matrix in LDS up to GCC_POSEMB_LDS_MAX and in a workspace slot above (a second
 * workspace class reaches GCC_POSEMB_BIG_MAX);
 * larger ones a thick-restart Krylov-Schur iteration
 * (single start vector, like ARPACK).  Eigenvectors are defined up to sign /
 * rotation inside degenerate eigenspaces; the reference's own output depends on
 * np.random.rand (data_util.py:248).  hidden <= 32. */
#define GCC_POSEMB_LDS_MAX 128
#define GCC_POSEMB_DIRECT_MAX 384
#define GCC_POSEMB_BIG_MAX 704      /* direct solver with the whole LDS of a CU up to this deflated size; Krylov-Schur above */
#define GCC_STATUS_POSEMB_NOT_CONVERGED 8
#define GCC_STATUS_POSEMB_TOO_LARGE 16   /* a subgraph with deflated size > GCC_POSEMB_DIRECT_MAX has more than
                                          * node_cap / batch_size nodes: zeros written (size node_cap accordingly) */
int64_t gcc_posemb_workspace_bytes(int32_t batch_size, int64_t node_cap, int32_t hidden);
/* pos: device [node_cap, hidden] out (rows >= node_off[B] untouched);
 * evals: device [B, hidden] out or NULL (eigenvalues, ascending, zero-padded);
 * raw:   device [node_cap, hidden] out or NULL (the eigenvectors before row normalisation);
 * seed: start vectors of the Krylov path are Philox(seed, subgraph) uniforms.
 * status: device int32[16]: [0] |= GCC_STATUS_*; diagnostics: [1] = most Krylov restart cycles / block filter rounds of
 *         an item, [2] += Arnoldi steps, [3] += items that left their first-choice solver (Krylov restart cap, block
 *         class handing on to the dense classes), [4] += items that set GCC_STATUS_POSEMB_NOT_CONVERGED, [5..9] = the
 *         first of them: item id (view * batch_size + subgraph), solver class, deflated size, reason, nodes. */
int32_t gcc_posemb(const gcc_batch_out *g, int32_t batch_size, int32_t hidden, float *pos, float *evals,
                   float *raw, uint64_t seed, void *workspace, int64_t workspace_bytes, int32_t *status, gcc_prof *prof,
                   void *stream);
/* The same for several batched graphs (views of several future steps) in ONE set of kernel launches: the
 * eigensolver kernels pull (view, subgraph) items from per-size-class work lists, so one call keeps the whole
 * GPU busy and its latency (bound by the slowest subgraph) is paid once.  All views share batch_size and node_cap. */
#define GCC_POSEMB_MAX_VIEWS 32
typedef struct gcc_posemb_view {
    const gcc_batch_out *g;
    float *pos, *evals, *raw;      /* as for gcc_posemb; evals/raw may be NULL */
} gcc_posemb_view;
int64_t gcc_posemb_multi_workspace_bytes(int32_t num_views, int32_t batch_size, int64_t node_cap, int32_t hidden);
int32_t gcc_posemb_multi(const gcc_posemb_view *views, int32_t num_views, int32_t batch_size, int64_t node_cap,
                         int32_t hidden, uint64_t seed, void *workspace, int64_t workspace_bytes, int32_t *status,
                         gcc_prof *prof, void *stream);
/* The same call with a GATE around its LDS-heavy launches (sparse block, Krylov and the 1024-thread dense classes:
 * workgroups that own most of a CU's LDS for milliseconds).  Several producer streams run such calls concurrently; with a
 * shared gate their heavy phases take turns, so that at most one call's heavy workgroups hold CUs at any time and the
 * rest of the GPU stays open to the training step's short kernels, while the light launches (classification, one-wave
 * teams) of all calls overlap freely.  heavy_wait: hipEvent_t the stream waits for before the first heavy launch (or
 * NULL); heavy_record: hipEvent_t recorded after the last one (or NULL). */
int32_t gcc_posemb_multi_gated(const gcc_posemb_view *views, int32_t num_views, int32_t batch_size, int64_t node_cap,
                               int32_t hidden, uint64_t seed, void *workspace, int64_t workspace_bytes, int32_t *status,
                               gcc_prof *prof, void *heavy_wait, void *heavy_record, void *stream);

/* How the solver classes of one gcc_posemb* call are issued.  0 (default): one after the other on the caller's stream -- next to a
 * training step that is what keeps the step's short kernels fed.  1: the one-wave teams and the 65..128 class on two side streams of the
 * caller's stream (same priority, created once per caller stream, joined before the call's end mark): half the latency of a call when
 * the pipeline has the GPU to itself (bench.py --mode sample-ready).  2: one side stream for everything but the block class.
 * -1: the environment variable GCC_POSEMB_FORK decides.  Process-wide; results do not depend on it. */
void gcc_posemb_set_fork(int32_t mode);

/* diagnostics: subsequent gcc_posemb* calls add wall-clock ticks (100 MHz) per solver class and phase into
 * device int64[GCC_POSEMB_TICK_CLASSES][16] -- EIGHT classes: small, mid, slot, Krylov, big, sparse block (Chebyshev),
 * one-wave teams n' <= 48, one-wave teams n' <= 64 (their ticks are WAVE time: 4 teams share a workgroup; the 'mid' class
 * runs on four-wave workgroups of 256 threads, three of which share a CU: its ticks are the time of one such workgroup);
 * phases of the dense classes 0..6 = matrix, tridiagonalise, bisect, inverse iteration, Gram-Schmidt, back-transform,
 * expand; [14] = executed f32 FLOPs; [15] = items; NULL switches it off.  A buffer sized for fewer classes is written
 * out of bounds. */
#define GCC_POSEMB_TICK_CLASSES 8
void gcc_posemb_debug_ticks(long long *device_ticks64);
/* the same for gin_in_kernel / gin_mid_kernel: device int64[3][16][2048] -- [kind 0 = gin_in first layer, 1 = gin_in other layers,
 * 2 = gin_mid][phase; 15 = tiles][workgroup = pass * 1024 + blockIdx.x]: every workgroup adds to its own slots (no shared counter) */
void gcc_gin_debug_ticks(long long *device_ticks64);

/* ------------------------------------------------------------ GIN encoder ---
 * GraphEncoder(gnn_model="gin", degree_input=True).forward of
 * gcc/models/graph_encoder.py:132-200 -> UnsupervisedGIN.forward gcc/models/gin.py:213-232
 * (DGL GINConv(sum, eps=0) + ApplyNodeFunc/MLP + BatchNorm1d + SumPooling +
 * linears_prediction + Dropout + F.normalize), and its backward.  The kernels
 * compute 64 channels (train.py:93 default); narrower models (gcc_gin_weights.hidden)
 * run zero-padded, exactly; d_in = pos_dim + deg_emb_dim + 1 <= 64.
 * All arithmetic is fp32 (f32 MFMA), BatchNorm / pooling sums accumulate in fp64. */
#define GCC_GIN_MAX_LAYERS 8     /* GIN message-passing layers = num_layers - 1 (train.py:79 -> 4) */
#define GCC_GIN_HIDDEN 64
#define GCC_GIN_STAT_REPLICAS 16  /* atomically accumulated rows are spread over this many copies (32 until ABI 3) */

typedef struct gcc_bn {          /* torch.nn.BatchNorm1d(64) */
    const float *weight, *bias;  /* device [64]                                           */
    float *running_mean, *running_var;   /* device [64], updated when update_running_stats */
    int64_t *num_batches_tracked;        /* device [1] or NULL                            */
} gcc_bn;

typedef struct gcc_gin_weights { /* state_dict of the reference GraphEncoder */
    int32_t num_gin_layers;      /* len(gnn.ginlayers)                                    */
    int32_t pos_dim, deg_emb_dim, max_degree;
    const float *degree_embedding;               /* [max_degree + 1, deg_emb_dim]          */
    const float *lin0_w[GCC_GIN_MAX_LAYERS];     /* ginlayers.i.apply_func.mlp.linears.0.weight [64, d_in|64] */
    const float *lin0_b[GCC_GIN_MAX_LAYERS];
    const float *lin1_w[GCC_GIN_MAX_LAYERS];     /* ...mlp.linears.1.weight [64, 64]       */
    const float *lin1_b[GCC_GIN_MAX_LAYERS];
    gcc_bn bn_a[GCC_GIN_MAX_LAYERS];             /* ...mlp.batch_norms.0                   */
    gcc_bn bn_b[GCC_GIN_MAX_LAYERS];             /* ginlayers.i.apply_func.bn              */
    gcc_bn bn_c[GCC_GIN_MAX_LAYERS];             /* gnn.batch_norms.i                      */
    const float *pred_w[GCC_GIN_MAX_LAYERS + 1]; /* gnn.linears_prediction.i.weight [64, d_in|64] */
    const float *pred_b[GCC_GIN_MAX_LAYERS + 1];
    float bn_eps, bn_momentum;   /* 1e-5, 0.1 (torch defaults, gin.py:51,104,189)          */
    float dropout_p;             /* 0.5 (graph_encoder.py:99)                              */
    float norm_eps;              /* 1e-5 (graph_encoder.py:196)                            */
    int32_t hidden;              /* --hidden-size (train.py:93) when it is below 64, 0 = 64: the COLUMN count of every weight
                                  * that reads a hidden representation (lin0_w of layers > 0, lin1_w, pred_w[i > 0]); the
                                  * kernels always compute 64 channels, so every weight keeps 64 ROWS and every per-channel
                                  * array 64 entries -- rows / entries >= hidden are zero padding owned by the caller (a zero
                                  * channel stays exactly zero through Linear, BatchNorm, ReLU and their backward, so the
                                  * padded model IS the narrow model).  Gradients come back in the same padded shapes. */
} gcc_gin_weights;

/* DEVICE-resident per-step scalars of a REPLAYED step.  A training step captured in a hipGraph replays the same
 * kernel arguments every time; what changes from step to step besides the data -- the learning rate (train.py:411-416),
 * Adam's bias corrections, the queue's ring pointer (memory_moco.py:55-61), the dropout key -- is read from this struct
 * by the kernels that need it (pass it where the `scalars` arguments below say; NULL = the by-value arguments), and
 * written by gcc_step_scalars_set, a one-thread launch issued in front of the replay. */
typedef struct gcc_step_scalars {
    float lr, bias_corr1, bias_corr2_sqrt;   /* Adam: lr, 1 - beta1^step, sqrt(1 - beta2^step) */
    int32_t enqueue_index;                   /* queue rows [index, index + nkeys) mod K are overwritten */
    uint64_t dropout_seed;                   /* Philox key of the pass's dropout masks (gcc_gin_pass.dropout_seed) */
} gcc_step_scalars;
int32_t gcc_step_scalars_set(gcc_step_scalars *dev, float lr, float beta1, float beta2, int32_t adam_step,
                             int32_t enqueue_index, uint64_t dropout_seed, void *stream);
/* The same without a launch between two replays: the HOST fills entry (n mod ring_len) of a ring in pinned, device-visible
 * host memory (gcc_step_scalars_fill: plain stores, no device work) before it launches the n-th step that uses the ring,
 * and the step's FIRST launch (gcc_step_scalars_fetch: one thread, part of the captured graph) copies entry
 * (*counter mod ring_len) into the device struct and increments the device-resident counter.  Host and device count the
 * same steps, so entry n is read by step n; the host must not run ring_len steps ahead of the device. */
void gcc_step_scalars_fill(gcc_step_scalars *host_entry, float lr, float beta1, float beta2, int32_t adam_step,
                           int32_t enqueue_index, uint64_t dropout_seed);
int32_t gcc_step_scalars_fetch(gcc_step_scalars *dev, const gcc_step_scalars *ring, int32_t ring_len,
                               unsigned long long *counter, void *stream);

typedef struct gcc_gin_pass {    /* one encoder invocation on one batched graph            */
    const int32_t *node_off, *row_ptr, *col_idx, *graph_id;   /* gcc_batch_out of the view */
    const float *pos;            /* device [node_cap, pos_dim]: ndata["pos_undirected"]    */
    int32_t batch_size;
    int32_t training;            /* 1: BatchNorm uses batch statistics (train.py:357-365)  */
    int32_t update_running_stats;/* 1: momentum update of running_mean/var                 */
    int32_t normalize;           /* graph_encoder.py:195 (train.py:83 default True)        */
    const float *dropout_keep;   /* device [num_gin_layers+1, B, 64] 0/1 keep masks, or NULL                    */
    uint64_t dropout_seed;       /* used when dropout_keep == NULL and dropout_philox != 0: keep(i, b, o) =     */
    int32_t dropout_philox;      /*   Philox4x32-10(key = seed, ctr = (b*64+o, i, 0xD50F, 0)).x >> 8 >= p * 2^24 */
    gcc_gin_weights w;
    /* activations, caller-allocated, kept for backward: */
    float *x0;                   /* [node_cap, 64] assembled input features (cols >= d_in are 0) */
    float *agg[GCC_GIN_MAX_LAYERS];   /* [node_cap, 64] h + sum_{u->v} h_u                */
    float *z1[GCC_GIN_MAX_LAYERS];    /* [node_cap, 64] linears.0 output                   */
    float *z2[GCC_GIN_MAX_LAYERS];    /* [node_cap, 64] linears.1 output                   */
    double *stats;               /* [num_gin_layers, 3, GCC_GIN_STAT_REPLICAS, 2, 64] column sum / sum of squares */
    double *pooled;              /* [num_gin_layers+1, B, 64] SumPooling of hidden_rep     */
    float *score;                /* [B, 64] score_over_layer before normalisation          */
    float *feat;                 /* [B, 64] output                                         */
    int32_t edge_multiplicity;   /* every edge of the CSR counts this many times (0 = 1): in-degree feature and
                                  * neighbour sum.  The reference's NodeClassificationDataset builds its DGL graph
                                  * with every undirected edge twice per direction (data_util.py:84-85 +
                                  * graph_dataset.py:301-302); forward only (backward requires 1). */
    double *bn_totals;           /* device [num_gin_layers][3][2][64] doubles, or NULL.  Training passes: gcc_gin_forward's
                                  * last kernel adds the 32 replicas of every BatchNorm's statistics up (in replica order:
                                  * the value each forward consumer computed for itself) and gcc_gin_backward's ~16 kernels
                                  * read these 2 numbers per channel instead of 64 before they can start. */
    const int32_t *seed_local;   /* device [B] or NULL: local index of the seed node of every graph (NULL: node 0, as the
                                  * sampler emits; graph classification marks g.out_degrees().argmax(),
                                  * data_util.py:236-237 with entire_graph=True) */
    const gcc_step_scalars *scalars;   /* device or NULL: with dropout_philox, the key is scalars->dropout_seed + dropout_seed
                                        * (read by the readout kernels of the forward AND the backward pass): dropout_seed is
                                        * then the pass's fixed offset -- 0, or the second pass's of an E2E step */
    int64_t node_cap;            /* (ABI 3) rows every per-node buffer of this pass holds (row_ptr: node_cap + 1 entries; graph_id, pos,
                                  * x0, agg, z1, z2: node_cap rows).  The tile kernels request a workgroup's first tile TOGETHER with the
                                  * live node count node_off[B] (one memory round trip instead of two dependent ones per kernel), clamped
                                  * to this capacity; rows past the live count are read and discarded.  Required (> 0). */
    int64_t rows_hint;           /* (ABI 3) 0, or an upper estimate of the live row count node_off[B] (e.g. 1.1 x the largest batch seen):
                                  * the tile kernels are launched with ceil(min(rows_hint, node_cap) / 64) workgroups per pass instead of
                                  * one per 64 rows of CAPACITY.  Any value is correct (workgroups walk on when there are more tiles);
                                  * workgroups without a tile cost what their speculative requests cost (0.63 vs 0.57 ms per step). */
} gcc_gin_pass;

/* Runs `npass` independent passes (e.g. query with model, key with model_ema)
 * in the same launches.  prof marks: 0 before, 1 after. */
int32_t gcc_gin_forward(const gcc_gin_pass *passes, int32_t npass, gcc_prof *prof, void *stream);
/* gcc_step_scalars_fetch + gcc_gin_forward without the fetch's launch: one thread of the forward's FIRST kernel copies ring
 * entry (*counter mod ring_len) into `dev` and increments the counter -- the same loads, the same count, once per call.  No
 * kernel of that first launch reads `dev`; the forward's readout (dropout key) and everything after it see the new entry.
 * An E2E step uses it for the first of its two forward calls only. */
int32_t gcc_gin_forward_fetch(const gcc_gin_pass *passes, int32_t npass, gcc_step_scalars *dev,
                              const gcc_step_scalars *ring, int32_t ring_len, unsigned long long *counter,
                              gcc_prof *prof, void *stream);

/* The eval-mode forward as ONE call (generate.py:33-53: model.eval(); feat_q = model(graph_q); feat_k = model(graph_k);
 * emb = (feat_q + feat_k) / 2): a workgroup carries a subgraph -- or a run of up to four subgraphs of at most 64 nodes --
 * through feature assembly, every GIN layer, the pooled readout and F.normalize with the hidden representation resident in
 * LDS (up to 320 nodes; larger ego-nets go through a second kernel that keeps up to 256 rows in LDS and gathers from the
 * L2-resident global copy above).  Every pass must have training = 0 (running statistics) and x0, z1[0], z2[0] ([node_cap,
 * 64] scratch: x0 holds the call's work list), score and feat; pooled is written when not NULL.  mean_out: device [B, 64]
 * or NULL -- receives the mean of the passes' feat (npass = 2: generate.py:52).  Same results as gcc_gin_forward in eval
 * mode to ~1e-6 (the neighbour sums run in another order). */
int32_t gcc_gin_eval_fused(const gcc_gin_pass *passes, int32_t npass, float *mean_out, void *stream);
/* diagnostics: device int64[2][16] -- per kernel of the call (subgraphs and runs of up to 320 nodes; the rest) 100 MHz ticks per
 * phase (features, pooling, weights, own rows / one wave's neighbour sums, gather / one wave's products, Linears / write-back,
 * mirror / barrier wait, readout; [8..11] = first start, last start, last end, longest stay of a workgroup; [15] = workgroups),
 * summed over every 4th (8th) workgroup of the following calls; NULL switches it off */
void gcc_gin_eval_debug_ticks(long long *device_ticks64);

typedef struct gcc_gin_grads {   /* same shapes as the weights; written (not accumulated)  */
    float *degree_embedding;
    float *lin0_w[GCC_GIN_MAX_LAYERS], *lin0_b[GCC_GIN_MAX_LAYERS];
    float *lin1_w[GCC_GIN_MAX_LAYERS], *lin1_b[GCC_GIN_MAX_LAYERS];
    float *bn_a_w[GCC_GIN_MAX_LAYERS], *bn_a_b[GCC_GIN_MAX_LAYERS];
    float *bn_b_w[GCC_GIN_MAX_LAYERS], *bn_b_b[GCC_GIN_MAX_LAYERS];
    float *bn_c_w[GCC_GIN_MAX_LAYERS], *bn_c_b[GCC_GIN_MAX_LAYERS];
    float *pred_w[GCC_GIN_MAX_LAYERS + 1], *pred_b[GCC_GIN_MAX_LAYERS + 1];
} gcc_gin_grads;

/* bytes of workspace gcc_gin_backward needs for a pass with this node capacity */
int64_t gcc_gin_backward_workspace_bytes(int64_t node_cap, int32_t batch_size, int32_t num_gin_layers);

/* Backward of one training-mode pass: dfeat [B, 64] -> grads (overwritten).
 * If `accumulate` != 0 the results are added to `grads` instead (E2E mode runs
 * two passes through the same weights, train.py:397-398).
 * Refused (-2, gcc_last_error names the sizes) when (max_degree + 1) * deg_emb_dim exceeds 10,240 floats: the degree-embedding
 * gradient keeps the table in LDS.  gcc_gin_forward serves such a table (a key encoder's forward-only training pass). */
int32_t gcc_gin_backward(const gcc_gin_pass *pass, const float *dfeat, const gcc_gin_grads *grads,
                         int32_t accumulate, void *workspace, int64_t workspace_bytes, int64_t node_cap,
                         gcc_prof *prof, void *stream);

/* gcc_gin_backward (accumulate = 0) whose last kernel also leaves the sum of squares of every gradient element it stored, as
 * `*nparts` fp64 partials (one per workgroup of that kernel, <= parts_cap or the call is refused with -3) in sumsq_parts --
 * the input of gcc_adam_ema_enqueue_step_scalars, which then needs no pass of its own over the gradient for the clip's norm.
 * The partials add up to the squared norm of the caller's flat gradient buffer if every element of that buffer is either a
 * target of `grads` or zero (zero-padded blocks of a hidden width below 64 are stored in full). */
int32_t gcc_gin_backward_sumsq(const gcc_gin_pass *pass, const float *dfeat, const gcc_gin_grads *grads, void *workspace,
                               int64_t workspace_bytes, int64_t node_cap, double *sumsq_parts, int32_t parts_cap,
                               int32_t *nparts, gcc_prof *prof, void *stream);

/* ------------------------------------- GIN encoder at any width (training) ---
 * The same encoder -- GraphEncoder(gnn_model="gin").forward, graph_encoder.py:132-200 -> gin.py:213-232 -- for hidden /
 * output sizes the 64-channel kernels above do not serve (`--hidden-size` above 64, train.py:93), forward in training
 * or eval mode and the full backward, fp32 on the matrix cores (gemm_dtype 0, the default) or with bf16 operands for the
 * per-node Linears (gemm_dtype 1, below).  Not fused: one launch per operator (CSR gather, strided
 * MFMA GEMM, fp64 column statistics, BatchNorm + ReLU passes, per-graph pooling); every activation is kept in the
 * caller's workspace for the backward pass.  Weights / gradients use gcc_gin_weights / gcc_gin_grads with the tensors'
 * own (unpadded) shapes: lin0_w[0] [hidden, d_in], lin0_w[i > 0] and lin1_w [hidden, hidden], pred_w[0] [out_dim, d_in],
 * pred_w[i > 0] [out_dim, hidden], per-channel arrays [hidden]; gcc_gin_weights.hidden is ignored.  Dropout: explicit
 * keep masks only (the host draws them, as torch.nn.Dropout does: gin.py:202,230).  The batched graph must be symmetric
 * (the sampler's output is): the gather is its own transpose in the backward pass. */
typedef struct gcc_ginx_pass {
    const int32_t *node_off, *row_ptr, *col_idx, *graph_id;   /* gcc_batch_out of the view                              */
    const float *pos;            /* device [node_cap, pos_dim]                                                          */
    const int32_t *seed_local;   /* device [B] or NULL (gcc_gin_pass.seed_local)                                        */
    int32_t batch_size;
    int32_t training;            /* 1: batch statistics; 0: running statistics (no backward)                            */
    int32_t update_running_stats;
    int32_t normalize;           /* graph_encoder.py:195                                                                */
    const float *dropout_keep;   /* device [num_gin_layers + 1, B, out_dim] 0 / 1 keep masks, or NULL: no dropout       */
    int32_t hidden, out_dim;     /* node_hidden_dim, output_dim: any positive size                                      */
    int32_t edge_multiplicity;   /* gcc_gin_pass.edge_multiplicity (forward; the backward pass requires 0 / 1)          */
    int32_t gemm_dtype;          /* (the former reserved_ field: 0 in every older caller) operands of the per-node Linears   */
                                 /* z1 / z2, their data gradients d a1 / d agg and weight gradients dW1 / dW0:          */
                                 /*   0: f32 on v_mfma_f32_16x16x4_f32 (parity mode);                                   */
                                 /*   1: C = alpha * sum_k bf16(A) * bf16(B) [+ bias] -- operands rounded to nearest    */
                                 /*      even as their tiles are staged, products and sums in fp32 on                   */
                                 /*      v_mfma_f32_16x16x32_bf16; memory stays fp32.  Gather, statistics, BatchNorm,   */
                                 /*      pooling, bias gradients, the [B, .] readout Linears and the normalisation are  */
                                 /*      f32 / fp64 in both modes.  Any other value: rc -5.                             */
    int64_t node_cap;            /* rows the launches are sized for (node_off[B] <= node_cap, read on the device)       */
    gcc_gin_weights w;
    void *workspace;             /* device, gcc_ginx_workspace_bytes(): activations of the forward pass (kept for the   */
    int64_t workspace_bytes;     /*   backward pass of the SAME struct) + backward scratch                              */
    float *feat;                 /* device [B, out_dim] out                                                             */
    float *pooled_out;           /* device [num_gin_layers, B, hidden] out or NULL: SumPooling of hidden_rep[1..]       */
} gcc_ginx_pass;
int64_t gcc_ginx_workspace_bytes(int64_t node_cap, int32_t batch_size, int32_t num_gin_layers, int32_t d_in, int32_t hidden,
                                 int32_t out_dim);
int32_t gcc_ginx_forward(const gcc_ginx_pass *p, void *stream);
/* dfeat: device [B, out_dim]; grads: written (not accumulated).  After gcc_ginx_forward of the same pass (training = 1). */
int32_t gcc_ginx_backward(const gcc_ginx_pass *p, const float *dfeat, const gcc_gin_grads *grads, void *stream);

/* MemoryMoCo.forward + NCESoftmaxLoss (mode 0: memory_moco.py:26-63, criterions.py:5-17) / the in-batch E2E head (mode 1:
 * out = rows mem^T / T with mem = the other view's features, K = B, labels on the diagonal: train.py:400, criterions.py:20-33)
 * at any feature size D, dense: out [B, K + 1] (mode 0: column 0 = <q, k> / T) or [B, B]; dlog: same shape, softmax - onehot;
 * grad_rows [B, D] = d loss / d rows and (mode 1) grad_mem [B, D] = d loss / d mem, both for a unit upstream gradient and
 * taken against the queue as it is NOW -- the caller enqueues afterwards; loss, prob: device scalars (mean CE; mean label
 * logit, train.py:394,401); acc: device double[2 + B * D] scratch (ABI 3: the B x D tail accumulates grad_rows, whose reduction runs
 * over the K queue rows and is split over workgroups). */
int32_t gcc_ncex_forward(const float *q, const float *k, const float *mem, int32_t B, int32_t K, int32_t D, float inv_T, int32_t mode,
                         float *out, float *dlog, float *grad_rows, float *grad_mem, float *loss, float *prob, double *acc, void *stream);
/* gcc_ncex_forward with the operand type of its three dense products -- the logits rows mem^T / T, d loss / d rows =
 * dlog mem / (T B) and (mode 1) d loss / d mem = dlog^T rows / (T B): gemm_dtype 0 = f32 (what gcc_ncex_forward calls),
 * 1 = operands rounded to bf16, fp32 products and sums (the rule of gcc_ginx_pass.gemm_dtype; `--nce-dtype bf16` above 64
 * features).  The positive logit <q, k> / T, the softmax and the positive's share of d loss / d q stay f32.  Other values: rc -5. */
int32_t gcc_ncex_forward_dt(const float *q, const float *k, const float *mem, int32_t B, int32_t K, int32_t D, float inv_T, int32_t mode,
                            float *out, float *dlog, float *grad_rows, float *grad_mem, float *loss, float *prob, double *acc,
                            int32_t gemm_dtype, void *stream);
/* memory.index_copy_(0, (arange(nkeys) + index) % K, keys) (memory_moco.py:55-61) for rows of D floats.  nkeys <= K is required
 * (rc -1 otherwise), as gcc_queue_enqueue requires it: with more keys than queue rows the indices collide and the reference's
 * index_copy_ result depends on the order its kernel happens to write in -- nothing a replacement could be bit-equal to. */
int32_t gcc_queue_enqueue_x(float *mem, int32_t K, int32_t D, const float *keys, int32_t nkeys, int32_t index, void *stream);

/* ------------------------------------------ wide GIN layers, bf16 (config 5) ---
 * BASELINE.json configs[4]: "GIN hid=256 layers=8 deg=32 bf16, SpMM+MFMA-MLP roofline run on batched
 * subgraphs".  The layer stack of UnsupervisedGIN.forward (gcc/models/gin.py:213-221) with hidden 256 and
 * BatchNorm in eval mode (generate.py:71 model.eval()), i.e. per layer
 *     agg = h + sum_{u in row v} h_u                                   (GINConv sum, eps = 0; gin.py:179-185)
 *     z1  = relu(s0 * (agg W0^T) + t0)                                 (mlp.linears.0 + mlp.batch_norms.0; gin.py:113-116)
 *     h'  = relu(s2 * relu(s1 * (z1 W1^T) + t1) + t2)                  (linears.1, apply_func.bn, gin.batch_norms; gin.py:55-57,219-220)
 * with the Linear biases and BatchNorm running statistics folded into the per-channel scale/shift pairs by
 * the caller.  Activations and weights are bf16 (stored as their 16 bits), every product accumulates in
 * f32 on the matrix cores, activations are rounded to bf16 (nearest even) where they are stored: agg, z1, h'.
 * One workgroup keeps one subgraph (<= 128 nodes) in LDS across all `num_layers` layers; pooled[b][i] is the
 * SumPooling of hidden_rep[i] (gin.py:205,228), i = 0 being the input. */
#define GCC_GINW_HIDDEN 256
#define GCC_GINW_MAX_NODES 128
#define GCC_STATUS_GINW_TOO_LARGE 32     /* a subgraph has more than GCC_GINW_MAX_NODES nodes and no scratch was given: its outputs are 0 */
#define GCC_STATUS_GINW_BAD_EDGE 64      /* a neighbour id outside its own subgraph was skipped                 */
typedef struct gcc_ginw_layer {
    const uint16_t *w0, *w1;             /* device [256, 256] bf16, torch Linear layout [out, in]               */
    const float *s0, *t0, *s1, *t1, *s2, *t2;   /* device [256] folded scale / shift                             */
    const uint16_t *w0_frag, *w1_frag;   /* device [256 * 256] bf16: the same weights re-laid by gcc_ginw_pack_weights
                                          * (which = 0 / 1), or NULL.  When every layer of a call has both, the kernel
                                          * requests 1 KiB-contiguous fragments instead of 16 rows x 64 B each (a wave
                                          * request over 16 rows costs ~3x the issue time; 13 % of the fused launch)  */
} gcc_ginw_layer;
typedef struct gcc_ginw_args {
    const int32_t *node_off;             /* device [B + 1]                                                       */
    const int32_t *row_ptr, *col_idx;    /* device batched CSR, global node ids; row v lists the in-neighbours   */
    const uint16_t *x_in;                /* device [N, 256] bf16                                                 */
    uint16_t *x_out;                     /* device [N, 256] bf16 output of the last layer, or NULL               */
    float *pooled;                       /* device [B, num_layers + 1, 256] or NULL                              */
    int32_t batch_size, num_layers;      /* 1 <= num_layers <= GCC_GIN_MAX_LAYERS                                */
    gcc_ginw_layer layers[GCC_GIN_MAX_LAYERS];
    /* Subgraphs over GCC_GINW_MAX_NODES nodes (ego-nets of the pre-training workload reach ~900): with scratch of
     * gcc_ginw_scratch_bytes(num_nodes, batch_size) bytes (device, 16-byte aligned) they run block by block -- one launch
     * per layer, one (subgraph, 128-row block) per workgroup, the block's adjacency strip taken 128 columns at a time with
     * the products accumulating in registers, rows through two global ping-pong buffers between layers -- with the same
     * rounding points as small subgraphs.  scratch == NULL: they are refused (GCC_STATUS_GINW_TOO_LARGE), as before. */
    void *scratch;
    int64_t scratch_bytes;
    int64_t num_nodes;                   /* rows of x_in (node_off[B] <= num_nodes); used with scratch only              */
} gcc_ginw_args;
int64_t gcc_ginw_scratch_bytes(int64_t num_nodes, int32_t batch_size);
/* status: device int32[1], OR of GCC_STATUS_GINW_* (zeroed by the caller).  prof marks: 0 before, 1 after. */
int32_t gcc_ginw_forward(const gcc_ginw_args *a, int32_t *status, gcc_prof *prof, void *stream);
/* Re-lays a [256, 256] bf16 Linear weight (torch layout) in the order gcc_ginw_forward's waves request it: fragment
 * (output block w < 4, fragment m < 4, k-step ks < 8) is 1 KiB contiguous at ((w * 4 + m) * 8 + ks) * 512 elements, lane
 * (16 lg + lr) holding W[row][32 ks + 8 lg .. + 7]; which = 0 (first Linear of a layer): row = 64 w + 32 (m / 2) +
 * 2 lr + m % 2 (the rows of two adjacent fragments interleaved), which = 1 (second Linear): row = 64 w + 16 m + lr.
 * Done once per model. */
int32_t gcc_ginw_pack_weights(const uint16_t *w, uint16_t *w_frag, int32_t which, void *stream);
/* diagnostics, as gcc_posemb_debug_ticks: device int64[16] (rows in, neighbour counts, fragments, aggregation, first
 * Linear, second Linear, rows out; [15] = subgraphs); NULL switches it off. */
void gcc_ginw_debug_ticks(long long *device_ticks64);

/* The eval-mode embedding of a wide GIN encoder in one call: generate.py:45-52, (f(graph_q) + f(graph_k)) / 2 (or f(graph_q)
 * with one view), on the resident layers above.  Per view:
 *     x      = bf16(positional embedding | degree embedding | seed flag), zero-padded to 256 columns (graph_encoder.py:152-165;
 *              in-degree = row length * edge_multiplicity, clamped to max_degree; seed = seed_local[b] or node 0)
 *     pooled = the SumPooling of x and of every layer's output, as gcc_ginw_forward computes them on the multigraph in which
 *              every CSR entry stands for edge_multiplicity edges (the self loop of GINConv counts once)
 *     score  = sum_i (pred_w[i] pooled[., i, :k_i] + pred_b[i]) in f32, k_0 = pos_dim + deg_emb_dim + 1, k_i = hidden;
 *              with `normalize`, score / max(||score||_2, norm_eps)                      (gin.py:226-230 in eval mode, graph_encoder.py:196)
 * The model's widths (input, hidden, output) are at most 256; `layers` holds the folded layer stack zero-padded to 256
 * channels (a padded channel has scale 0 and shift 0 and stays exactly 0), layer 0's [hidden, k_0] weight in the top left
 * corner of its [256, 256] block.  The rounding points are those of gcc_ginw_forward plus the rounding of x; the readout is f32.
 * Row counts are read on the device (node_off[batch_size]); nothing is read back by the host.  A count of one neighbour
 * (edge_multiplicity * copies in the CSR, + 1 on the diagonal) above 256 has no exact bf16 value: it is reported, never rounded --
 * up to the width of the 16-bit counters: a count of 65,536 or more wraps unseen, such a CSR is outside the contract. */
#define GCC_STATUS_GINW_COUNT_OVERFLOW 128   /* a neighbour occurs more than 256 times in one row: the results of its subgraph are wrong */
typedef struct gcc_ginw_embed_args {
    int32_t num_views;                   /* 1 or 2                                                               */
    int32_t batch_size, num_layers;      /* subgraphs per view; 1 <= num_layers <= GCC_GIN_MAX_LAYERS            */
    int32_t pos_dim, deg_emb_dim, max_degree, edge_multiplicity;
    int32_t hidden, out_dim;             /* 1..256 each, as pos_dim + deg_emb_dim + 1                            */
    int32_t normalize;
    float norm_eps;
    int64_t node_cap;                    /* rows the workspace is sized for: node_off[batch_size] <= node_cap    */
    const int32_t *node_off[2], *row_ptr[2], *col_idx[2];   /* per view, as gcc_ginw_args                        */
    const int32_t *seed_local[2];        /* device [B] or NULL (node 0 of every subgraph)                        */
    const float *pos[2];                 /* device [>= N, pos_dim]                                               */
    const float *degree_embedding;       /* device [max_degree + 1, deg_emb_dim]                                 */
    gcc_ginw_layer layers[GCC_GIN_MAX_LAYERS];
    const float *pred_w[GCC_GIN_MAX_LAYERS + 1], *pred_b[GCC_GIN_MAX_LAYERS + 1];   /* [out_dim, k_i], [out_dim] */
    float *pooled[2];                    /* device [B, num_layers + 1, 256] per view (written, then read by the readout) */
    float *out;                          /* device [B, out_dim]                                                  */
    void *workspace;                     /* device, 16-byte aligned, gcc_ginw_embed_workspace_bytes(node_cap, batch_size) */
    int64_t workspace_bytes;
} gcc_ginw_embed_args;
int64_t gcc_ginw_embed_workspace_bytes(int64_t node_cap, int32_t batch_size);
/* status: device int32[1], OR of GCC_STATUS_GINW_* (zeroed by the caller). */
int32_t gcc_ginw_embed(const gcc_ginw_embed_args *a, int32_t *status, void *stream);

/* ------------------------------------------------------- MoCo / InfoNCE head ---
 * MemoryMoCo.forward (gcc/contrastive/memory_moco.py:26-63, use_softmax=True) fused
 * with NCESoftmaxLoss (gcc/contrastive/criterions.py:12-17), and the E2E variant
 * out = feat_k feat_q^T / T with NCESoftmaxLossNS (train.py:400, criterions.py:27-33).
 * logits[b][j] = q_b . mem_j * inv_T; the positive is an extra column q_b . k_b
 * (pos_mode 0) or the diagonal column j == b (pos_mode 1).  The [B, K+1] logits are
 * only written when out_dense != NULL; loss/backward use an online row-softmax. */
#define GCC_NCE_DIM 64
typedef struct gcc_nce_args {
    const float *q;          /* device [B, 64] rows whose softmax is taken                      */
    const float *k;          /* device [B, 64] positives (pos_mode 0) or NULL                   */
    const float *mem;        /* device [K, 64] negatives: the queue, or the other view (E2E)    */
    const float *patch;      /* device [patch_rows, 64] or NULL: rows patch_index.. (mod K) of   */
    int32_t patch_index;     /*   mem are read from here (queue rows already overwritten by the */
    int32_t patch_rows;      /*   enqueue that follows the forward, memory_moco.py:55-61)       */
    int32_t B, K;
    int32_t pos_mode;        /* 0: MoCo, 1: E2E diagonal, GCC_NCE_POS_MOCO_DEFERRED: MoCo whose  */
                             /*   two means are formed by the backward call (below)             */
    float inv_T;             /* 1 / nce_t (train.py:87)                                         */
    float *lse, *pos;        /* device [B] out: row log-sum-exp and positive logit               */
    float *loss, *prob;      /* device [1] out: mean(lse - pos) and mean(pos) (train.py:394,407) */
    float *out_dense;        /* device [B, K + (pos_mode == 0)] or NULL                         */
    int32_t dtype;           /* GCC_NCE_F32: exact fp32 MFMA (parity mode, 1e-3 of the reference)  */
                             /* GCC_NCE_BF16: q, k and the queue rounded to bf16 on load, fp32     */
                             /*   accumulation and softmax (throughput mode of north_star; the     */
                             /*   queue itself stays fp32 in HBM / in the checkpoint)              */
} gcc_nce_args;
#define GCC_NCE_F32 0
#define GCC_NCE_BF16 1
/* pos_mode of a MoCo head (out_dense NULL) whose caller reads loss / prob only after the backward call: gcc_nce_forward ends
 * with lse / pos -- no arrival counter, no last workgroup -- and gcc_nce_backward's last launch forms loss[0] and prob[0] in
 * one extra workgroup, with the additions of pos_mode 0 in their order (the same bits).  Both calls take the same args. */
#define GCC_NCE_POS_MOCO_DEFERRED 2

int64_t gcc_nce_workspace_bytes(int32_t B, int32_t K);
int32_t gcc_nce_forward(const gcc_nce_args *a, void *workspace, int64_t workspace_bytes, gcc_prof *prof,
                        void *stream);
/* dq[b] = dloss / (B T) * (sum_j p_bj mem_j + [pos_mode 0] (p_b,pos - 1) k_b - [pos_mode 1] mem_b).
 * by_mem_row != 0 computes the gradient w.r.t. the OTHER operand of the E2E product instead:
 * call it with q/mem swapped; p is then normalised with lse[mem row] (args->lse has K entries). */
int32_t gcc_nce_backward(const gcc_nce_args *a, const float *dloss, int32_t by_mem_row, float *dq,
                         void *workspace, int64_t workspace_bytes, gcc_prof *prof, void *stream);
/* gcc_nce_forward + gcc_nce_backward of the MoCo head (pos_mode 0, GCC_NCE_F32, out_dense NULL; anything else is refused
 * with -2) as TWO launches instead of four, with ONE pass over the queue: the slice kernel keeps a running maximum per
 * query and feeds exp(logit - maximum) straight into the second product, rescaling its accumulators when the maximum
 * rises; the merge kernel forms lse / pos / loss / prob as gcc_nce_forward does and
 * dq[b] = dloss / (B T) * (sum_s exp(pm_s - lse) slab_s[b] + (p_b,pos - 1) k_b), slabs in slice order.  Same workspace;
 * same results up to summation order.  prof_fwd marks 0 / 1 bracket the slice launch, prof_bwd's the merge launch. */
int32_t gcc_nce_forward_backward(const gcc_nce_args *a, const float *dloss, float *dq, void *workspace,
                                 int64_t workspace_bytes, gcc_prof *prof_fwd, gcc_prof *prof_bwd, void *stream);

/* memory.index_copy_(0, (arange(n) + index) % K, keys) of memory_moco.py:55-61; when saved != NULL
 * the overwritten rows are first copied there (the `patch` of gcc_nce_args). */
int32_t gcc_queue_enqueue(float *mem, int32_t K, const float *keys, int32_t nkeys, int32_t index, float *saved,
                          void *stream);

/* clip_grad_norm_(max_norm) + Adam.step() of train.py:409,417 over one flat buffer (torch.optim.Adam
 * semantics: L2 weight decay added to the gradient, bias correction with `step` >= 1, eps outside the
 * sqrt).  grad_norm: device [1] out (the pre-clip norm); max_norm <= 0 disables clipping.
 * grad_scale > 0 multiplies the gradient first (1 / world for a gradient that was SUMMED over ranks:
 * norm, clipping and the stored clipped gradient all see grad * grad_scale); 1 on a single GPU.
 * scratch: device double[64], zeroed once by the caller (partial sums and an arrival counter that resets itself). */
int32_t gcc_adam_step(float *param, float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, float lr,
                      float beta1, float beta2, float eps, float weight_decay, int32_t step, float max_norm,
                      float grad_scale, float *grad_norm, double *scratch, void *stream);

/* The meters train.py:418-428 updates every step (loss, prob, gnorm, graph size; max nodes / edges of a q view),
 * accumulated on the device so that a step never synchronises with the host (the reference does, train.py:433):
 * acc: device double[5] += {loss, prob, grad_norm, nodes(q) + nodes(k), 1}; mx: device int32[2] = max with
 * {nodes(q), edges(q)}.  The caller reads and zeroes them when a log line is due. */
int32_t gcc_step_meters(double *acc, int32_t *mx, const float *loss, const float *prob, const float *grad_norm,
                        const int32_t *node_off_q, const int32_t *edge_off_q, const int32_t *node_off_k,
                        int32_t batch_size, void *stream);

/* moment_update of train.py:169-172 over one flat parameter buffer: ema = m * ema + (1 - m) * p */
int32_t gcc_ema_update(float *ema, const float *p, int64_t n, float m, void *stream);

/* The tail of a MoCo step (train.py:409,417-431) in the two launches of gcc_adam_step: clip + Adam over param[0, n),
 * then -- inside the Adam launch -- moment_update of ema[0, n_ema) from param[0, n_ema) (n_ema >= n: the live
 * parameters are a prefix of the flat buffer; the rest is only averaged, as the reference averages its unused
 * set2set / lin_readout weights) and one step of gcc_step_meters with this step's gradient norm.  ema == NULL and/or
 * meters == NULL leave that part out; with both NULL this is gcc_adam_step.  Same results as the three calls. */
typedef struct {
    double *acc;                 /* device double[5], as gcc_step_meters */
    int32_t *mx;                 /* device int32[2] */
    const float *loss, *prob;    /* device [1] each */
    const int32_t *node_off_q, *edge_off_q, *node_off_k;
    int32_t batch_size;
} gcc_step_meters_args;
int32_t gcc_adam_ema_step(float *param, float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, float lr,
                          float beta1, float beta2, float eps, float weight_decay, int32_t step, float max_norm,
                          float grad_scale, float *grad_norm, double *scratch, float *ema, int64_t n_ema, float ema_m,
                          const gcc_step_meters_args *meters, void *stream);
/* The same two launches and gcc_queue_enqueue with lr / bias corrections / ring pointer taken from a device-resident
 * gcc_step_scalars (a step captured in a hipGraph: see above).  Same results as the by-value calls. */
int32_t gcc_adam_ema_step_scalars(float *param, float *grad, float *exp_avg, float *exp_avg_sq, int64_t n,
                                  float beta1, float beta2, float eps, float weight_decay, float max_norm,
                                  float grad_scale, float *grad_norm, double *scratch, float *ema, int64_t n_ema, float ema_m,
                                  const gcc_step_meters_args *meters, const gcc_step_scalars *scalars, void *stream);
int32_t gcc_queue_enqueue_scalars(float *mem, int32_t K, const float *keys, int32_t nkeys,
                                  const gcc_step_scalars *scalars, void *stream);
/* The tail of a single-GPU MoCo step as ONE launch: gcc_adam_ema_step_scalars with
 *  - sumsq_parts / nparts (NULL / 0: the separate sum-of-squares launch stays): the partials of gcc_gin_backward_sumsq, valid
 *    when nothing touched the gradient since (no all-reduce, no accumulation); every workgroup adds them up in one fixed order,
 *    so grad_norm equals gcc_adam_ema_step_scalars' to fp64 reordering;
 *  - queue / K / keys / nkeys (queue NULL: none): gcc_queue_enqueue_scalars' copies as extra workgroups of the Adam launch.
 * At least one of the two must be given.  The clipped gradient is left in `grad` and grad_norm[0] written as before. */
int32_t gcc_adam_ema_enqueue_step_scalars(float *param, float *grad, float *exp_avg, float *exp_avg_sq, int64_t n,
                                          float beta1, float beta2, float eps, float weight_decay, float max_norm,
                                          float grad_scale, float *grad_norm, double *scratch, float *ema, int64_t n_ema, float ema_m,
                                          const gcc_step_meters_args *meters, const gcc_step_scalars *scalars,
                                          const double *sumsq_parts, int32_t nparts, float *queue, int32_t K, const float *keys,
                                          int32_t nkeys, void *stream);

/* --optimizer sgd / adagrad (train.py:658-679) on the same flat buffers, with torch.optim's float32 arithmetic:
 *   GCC_OPT_SGD      torch.optim.SGD(lr, momentum, weight_decay), dampening 0, no Nesterov: g' = g_clipped + wd p;
 *                    buf = momentum buf + g'; p -= lr buf.  state = buf, ZERO-initialised by the caller (which gives torch's
 *                    first step, buf = g', without a step counter); hyper = momentum.
 *   GCC_OPT_ADAGRAD  torch.optim.Adagrad(lr, lr_decay, weight_decay, eps): g' = g_clipped + wd p; sum += g' g';
 *                    p -= clr g' / (sqrt(sum) + eps).  state = sum, zero-initialised; hyper = eps; `lr` is THIS STEP's
 *                    clr = lr / (1 + (t - 1) lr_decay), which the caller forms in double as torch does.
 * gcc_opt_step / gcc_opt_ema_step / gcc_opt_ema_step_scalars are gcc_adam_step / gcc_adam_ema_step / gcc_adam_ema_step_scalars
 * with that update: the same clip (fixed-order double sum of squares, coef = min(1, max_norm / (norm + 1e-6)), grad_scale folded
 * in, the clipped gradient stored back, grad_norm[0] written, max_norm <= 0 = no clip), the same scratch, the same optional EMA
 * and meters inside the update launch; two launches.  With scalars, scalars->lr is the step's rate (Adagrad: its clr); the
 * bias-correction fields are not read.  gcc_opt_clipvalue_step is gcc_adam_clipvalue_step's twin (one launch).
 * An unknown rule, n < 1 and a NULL pointer are refused (rc < 0, gcc_last_error()). */
#define GCC_OPT_SGD 1
#define GCC_OPT_ADAGRAD 2
int32_t gcc_opt_step(int32_t rule, float *param, float *grad, float *state, int64_t n, float lr, float hyper,
                     float weight_decay, float max_norm, float grad_scale, float *grad_norm, double *scratch, void *stream);
int32_t gcc_opt_ema_step(int32_t rule, float *param, float *grad, float *state, int64_t n, float lr, float hyper,
                         float weight_decay, float max_norm, float grad_scale, float *grad_norm, double *scratch, float *ema,
                         int64_t n_ema, float ema_m, const gcc_step_meters_args *meters, void *stream);
int32_t gcc_opt_ema_step_scalars(int32_t rule, float *param, float *grad, float *state, int64_t n, float hyper,
                                 float weight_decay, float max_norm, float grad_scale, float *grad_norm, double *scratch,
                                 float *ema, int64_t n_ema, float ema_m, const gcc_step_meters_args *meters,
                                 const gcc_step_scalars *scalars, void *stream);
int32_t gcc_opt_clipvalue_step(int32_t rule, float *param, float *grad, float *state, int64_t n, float lr, float hyper,
                               float weight_decay, float clip_value, float grad_scale, void *stream);

/* ------------------------------------------------------- fine-tuning head ---
 * train.py --finetune (train_finetune / test_finetune of the reference, train.py:175-337): output_layer = nn.Linear(D, C),
 * CrossEntropyLoss (mean over the batch) and out.argmax(1), as ONE single-workgroup launch.  Rows whose label is < 0 are
 * padding (a partial last batch filled with empty subgraphs): they add nothing to the loss, the gradients or the counts.
 * Limits: 1 <= C <= 64, 1 <= D <= 256; anything else is refused (rc < 0, gcc_last_error()).  Every sum over rows runs in a
 * fixed order (no float atomics): two runs give bit-identical results. */
typedef struct gcc_cls_head_args {
    const float *feat;           /* device [B][ld_feat]: the encoder's embeddings, columns [0, D) used */
    const float *W;              /* device [C][D] (torch layout of nn.Linear.weight) */
    const float *b;              /* device [C] */
    const int32_t *labels;       /* device [B]: class index, < 0 = padding row */
    int32_t B, D, C, ld_feat, ld_dfeat;
    float *logits;               /* device [B][C] out, or NULL */
    float *dlogits;              /* train: device [B][C] out, (softmax - onehot) / valid rows, 0 on padding rows */
    float *dW, *db;              /* train: device [C][D], [C] out (may point into a flat gradient buffer) */
    float *dfeat;                /* train: device [B][ld_dfeat] out = dlogits W (columns past D written as 0) */
    float *loss;                 /* train: device [1] out, mean over the valid rows */
    int32_t *correct;            /* train: device [2] out {correct predictions, valid rows}, or NULL */
    double *meter_acc;           /* train, optional: device double[5] += {loss * valid, correct, valid, nodes, 1} */
    int32_t *meter_max;          /* train, optional: device int32[2] = max with {node_off[B], edge_off[B]} */
    const int32_t *node_off, *edge_off;   /* device [B + 1] of the batch (for the meters), or NULL */
    double *eval_loss_sum;       /* eval: device double[1] += sum over valid rows of the row's CE */
    int32_t *eval_counts;        /* eval: device int32[2] += {correct predictions, valid rows} */
} gcc_cls_head_args;
/* logits, loss, dlogits, dW, db, dfeat, correct count (+ meters) of one training batch */
int32_t gcc_cls_head_train(const gcc_cls_head_args *args, void *stream);
/* forward only (held-out fold): accumulates eval_loss_sum / eval_counts, so the eval loop reads them once at the end */
int32_t gcc_cls_head_eval(const gcc_cls_head_args *args, void *stream);

/* clip_grad_value_(params, clip_value) + Adam.step() over one flat buffer: g <- clamp(g * grad_scale, -clip_value, clip_value)
 * (stored back, as torch leaves the clipped gradient), then gcc_adam_step's update (L2 weight decay added to the clipped
 * gradient, bias correction with step >= 1, eps outside the sqrt).  clip_value <= 0 disables the clamp.  One launch. */
int32_t gcc_adam_clipvalue_step(float *param, float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, float lr,
                                float beta1, float beta2, float eps, float weight_decay, int32_t step, float clip_value,
                                float grad_scale, void *stream);

/* ------------------------------------------------------------ GAT backbone ---
 * GraphEncoder(gnn_model="gat") (gat.py + graph_encoder.py:152-196 of the reference): input features
 * [pos | degree_embedding(clamp(in_degree)) | seed], L GATLayers (fc without bias, per-head attention logits el / er,
 * leaky_relu(0.2) edge scores, softmax over each node's incoming edges, head-major flatten, F.leaky_relu between layers),
 * Set2Set(D, T, Lr) with PyTorch's LSTM gate order (i, f, g, o), lin_readout (Linear, ReLU, Linear) and F.normalize.
 * One workgroup per subgraph for the whole forward pass (one launch) and for the per-node / per-graph part of the
 * backward; weight gradients are per-chunk partials summed in a fixed order (no float atomics: two backward calls
 * give bit-identical gradients).  Limits: D = hidden <= 64 with D % heads == 0, out_dim <= 64,
 * pos_dim + deg_emb_dim + 1 <= 64, L <= GCC_GAT_MAX_LAYERS, Lr <= GCC_GAT_MAX_S2S_LAYERS, T >= 1.
 * The batch contract is symmetric (every CSR entry u in row v has an entry v in row u), as for the GIN kernels. */
#define GCC_GAT_MAX_LAYERS 8
#define GCC_GAT_MAX_S2S_LAYERS 8

typedef struct gcc_gat_weights {
    int32_t num_layers, hidden, heads, out_dim;       /* L, D, H, lin_readout output                     */
    int32_t pos_dim, deg_emb_dim, max_degree;
    int32_t s2s_iters, s2s_layers;                    /* T (--set2set-iter), Lr (--set2set-lstm-layer)    */
    int32_t normalize;                                /* F.normalize(p=2, dim=-1, eps=norm_eps) at the end */
    float norm_eps;
    const float *degree_embedding;                    /* [max_degree + 1][deg_emb_dim]                   */
    const float *fc[GCC_GAT_MAX_LAYERS];              /* gnn.layers.i.gnn.fc.weight [D][in]               */
    const float *attn_l[GCC_GAT_MAX_LAYERS];          /* gnn.layers.i.gnn.attn_l [1][H][D/H]              */
    const float *attn_r[GCC_GAT_MAX_LAYERS];
    const float *w_ih[GCC_GAT_MAX_S2S_LAYERS];        /* set2set.lstm.weight_ih_lk [4D][2D | D]           */
    const float *w_hh[GCC_GAT_MAX_S2S_LAYERS];        /* set2set.lstm.weight_hh_lk [4D][D]                */
    const float *b_ih[GCC_GAT_MAX_S2S_LAYERS];
    const float *b_hh[GCC_GAT_MAX_S2S_LAYERS];
    const float *ro0_w, *ro0_b;                       /* lin_readout.0 [D][2D], [D]                       */
    const float *ro2_w, *ro2_b;                       /* lin_readout.2 [out][D], [out]                    */
} gcc_gat_weights;

typedef struct gcc_gat_grads {                        /* device gradients, same shapes as the weights     */
    float *degree_embedding;
    float *fc[GCC_GAT_MAX_LAYERS], *attn_l[GCC_GAT_MAX_LAYERS], *attn_r[GCC_GAT_MAX_LAYERS];
    float *w_ih[GCC_GAT_MAX_S2S_LAYERS], *w_hh[GCC_GAT_MAX_S2S_LAYERS];
    float *b_ih[GCC_GAT_MAX_S2S_LAYERS], *b_hh[GCC_GAT_MAX_S2S_LAYERS];
    float *ro0_w, *ro0_b, *ro2_w, *ro2_b;
} gcc_gat_grads;

typedef struct gcc_gat_pass {
    const int32_t *node_off, *row_ptr, *col_idx;      /* the batch (gcc_gin_pass)                         */
    const int32_t *seed_local;                        /* device [B] or NULL (seed = first node)           */
    const float *pos;                                 /* device [node_cap][pos_dim]                       */
    int32_t batch_size, node_cap, edge_multiplicity, reserved_;
    float *saved;                                     /* device, gcc_gat_saved_floats() floats: activations the
                                                         backward reads (written by gcc_gat_forward)       */
    float *out;                                       /* device [B][out_dim]                              */
} gcc_gat_pass;

/* floats of gcc_gat_pass.saved for this model and batch capacity (< 0: refused, gcc_last_error()) */
int64_t gcc_gat_saved_floats(const gcc_gat_weights *w, int32_t node_cap, int32_t batch_size);
/* the forward pass: one launch, one workgroup per subgraph */
int32_t gcc_gat_forward(const gcc_gat_pass *p, const gcc_gat_weights *w, void *stream);
int64_t gcc_gat_backward_workspace_bytes(const gcc_gat_weights *w, int32_t node_cap, int32_t batch_size);
/* backward of a gcc_gat_forward pass (same p, w, unchanged saved): dout [B][out_dim] -> every parameter gradient,
 * written (accumulate = 0) or added (accumulate = 1).  Three launches. */
int32_t gcc_gat_backward(const gcc_gat_pass *p, const gcc_gat_weights *w, const float *dout, const gcc_gat_grads *g,
                         int32_t accumulate, void *workspace, int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------ whole-graph batches ---
 * GraphClassificationDataset / GraphClassificationDatasetLabeled of the reference (graph_dataset.py:306-385,
 * entire_graph=True): an item is a whole small graph in its own node order, a batch is dgl.batch of the selected graphs.
 * The corpus (every graph of the dataset, concatenated) is uploaded once; gcc_pack_graphs writes the batch of the graphs
 * idx[0..B) into caller-owned buffers -- what the host loop of gcc_amd/datasets.py (_batch_of, the positional-row gather,
 * _expand_multiplicity) assembles, bit for bit. */
typedef struct gcc_graph_corpus {
    int32_t num_graphs;          /* G                                                                        */
    int32_t pos_dim;             /* P: columns of pos, even and >= 2 (read only when pos is given)            */
    const int32_t *node_first;   /* device [G + 1]: first node of every graph in the concatenation            */
    const int32_t *row_ptr;      /* device [N_tot + 1]: GLOBAL entry offsets; graph g's own row_ptr is
                                    row_ptr[node_first[g] ..] - row_ptr[node_first[g]]                        */
    const int32_t *col_idx;      /* device [E_tot]: node ids local to their graph                             */
    const int32_t *seed_local;   /* device [G]: out_degrees().argmax(), first maximum (data_util.py:228-237)  */
    const int32_t *labels;       /* device [G] or NULL                                                        */
    const float *pos;            /* device [N_tot][P] or NULL: every graph's positional embedding; may be set
                                    after the eigensolver has run over all graphs                             */
} gcc_graph_corpus;
#define GCC_PACK_GRAPHS_MAX_BATCH 1024     /* graphs per call (one workgroup forms the batch offsets)          */
/* bits of gcc_pack_graphs' status word (a word of its own, not the sampler's) */
#define GCC_STATUS_PACK_NODE_OVERFLOW 1    /* the selected graphs have more than node_cap nodes                */
#define GCC_STATUS_PACK_EDGE_OVERFLOW 2    /* ... more than edge_cap entries (after `expand`)                  */
#define GCC_STATUS_PACK_BAD_INDEX     4    /* an index outside [-1, G): treated as padding                     */
/* idx: device [B], 1 <= B <= GCC_PACK_GRAPHS_MAX_BATCH; -1 = padding row (an empty graph, seed_local_out 0, labels_out -1);
 * an index may occur several times.  Written: out->node_off / edge_off [B + 1], and for the n = node_off[B] live rows
 * graph_id [n], row_ptr [n + 1] (batched entry offsets), col_idx [edge_off[B]] (batched node ids); out->parent_nid is not
 * touched.  pos_out (device [node_cap][P], or NULL): rows 0..n-1 = the graphs' rows of corpus->pos, when both are given.
 * seed_local_out device [B]; labels_out device [B] or NULL (-1 everywhere when the corpus has no labels).
 * expand >= 1: every entry is written `expand` times in a row and row_ptr / edge_off are multiplied by it (a uniform
 * multigraph as simple CSR).  Rows and entries past the live extents are unspecified.
 * Capacity: the leading graphs that fit node_cap and edge_cap form the batch, the others become empty graphs and
 * status (device int32[1], OR-ed, zeroed by the caller) reports why; nothing is written past either capacity.
 * Two launches (batch offsets; rows and entries by tiles), no workspace. */
int32_t gcc_pack_graphs(const gcc_graph_corpus *corpus, const int32_t *idx, int32_t B, const gcc_batch_out *out,
                        float *pos_out, int32_t *seed_local_out, int32_t *labels_out, int32_t expand, int32_t *status,
                        void *stream);

/* -------------------------------------------------------- similarity search ---
 * gcc/tasks/similarity_search.py:41-69 of the reference: the rows of two embedding tables are divided by their L2 norm,
 * every selected row of the first (the queries) is scored against every selected row of the second (the candidates),
 * and the rank of each query's true match decides Recall@k.  One call gives the rank counts and the k best candidates
 * of every query; the [mq, mc] score matrix is never stored.
 * Scores: s_ij = <q_i, c_j>, exact-f32 products and sums on v_mfma_f32_16x16x4_f32.
 * Order of a query's candidates: score descending, then column ascending (the reference's argsort leaves ties open).
 *   greater[i]      = #{j : s_ij > s_it}              t = target[i]
 *   equal_before[i] = #{j < t : s_ij == s_it}         query i is a hit at k  <=>  greater + equal_before < k
 *   target_score[i] = s_it, the very value the counts compare against (NaN without a target)
 *   topk_col / topk_score [i]: the first min(k, mc) candidates in that order, then -1 / -inf
 * Rows without a target (target NULL, -1 or refused) get greater = equal_before = -1.  Candidates and queries whose
 * index is refused are absent: an absent candidate is neither counted nor listed, an absent query has no target and an
 * empty list; a target that is refused, or that names an absent candidate, is no target (the list is still written).
 * Inputs are expected to be finite. */
#define GCC_SIM_MAX_DIM 256
#define GCC_SIM_MAX_K   64
#define GCC_SIM_MAX_SPLITS 64
#define GCC_STATUS_SIM_ZERO_ROW  1   /* normalize != 0 and a selected row has norm 0: it scores 0 against everything */
#define GCC_STATUS_SIM_BAD_INDEX 2   /* a q_idx / c_idx entry outside its table, or a target outside [-1, mc): row treated as absent */
typedef struct gcc_sim_args {
    const float *emb_q; int64_t rows_q, ld_q;   /* device [rows_q, ld_q], ld_q >= D */
    const float *emb_c; int64_t rows_c, ld_c;
    const int32_t *q_idx;      /* device [mq] rows of emb_q, or NULL = 0..mq-1; repeats allowed */
    const int32_t *c_idx;      /* device [mc] rows of emb_c, or NULL; repeats allowed */
    const int32_t *target;     /* device [mq]: candidate COLUMN (0..mc-1) of query i's true match, -1 = none; NULL = none */
    int32_t mq, mc, D, k;      /* 1 <= D <= 256; 0 <= k <= 64 (0: no lists) */
    int32_t normalize;         /* 1: rows divided by their L2 norm (similarity_search.py:49-50); 0: raw dot products */
    int32_t splits;            /* candidate ranges that are searched by separate workgroups and merged (at most
                                  GCC_SIM_MAX_SPLITS, and at most one per 16 candidates); 0 = chosen by the library */
    int32_t *greater, *equal_before;   /* device [mq] out, or NULL */
    float   *target_score;             /* device [mq] out, or NULL */
    int32_t *topk_col; float *topk_score;   /* device [mq, k] out, or NULL */
} gcc_sim_args;
/* bytes of workspace for a call of these sizes: O((mq + mc) * Dpad + splits * mq * k); negative on a bad size */
int64_t gcc_sim_workspace_bytes(int32_t mq, int32_t mc, int32_t D, int32_t k, int32_t splits);
/* status: device int32[1], OR-ed, zeroed by the caller.  D, k, splits or a size out of range, a NULL table, ld < D,
 * mq / mc beyond the table without an index list and a short workspace return rc < 0, name the member in
 * gcc_last_error() and launch nothing.  mq == 0 or mc == 0: rc 0, no launch, nothing written.  Four launches (gather
 * and normalise; target scores; tiles; merge of the splits), no host synchronisation. */
int32_t gcc_sim_search(const gcc_sim_args *a, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream);

/* ---------------------------------------------- C-SVC on frozen embeddings ---
 * gcc/tasks/graph_classification.py:47-64 of the reference: StratifiedKFold, then sklearn.svm.SVC(C=100000) per fold, which
 * is libsvm's one-vs-one C-SVC with an RBF kernel.  Here every (fold, class pair) is one problem -- the fold's training rows
 * of the two classes, class ci's rows first (+1), then class cj's (-1), each in corpus order -- and all problems of all
 * folds are solved side by side, one workgroup each, over ONE matrix of squared distances of the corpus:
 *   gcc_svc_distances   d2[i, j] = sum_c (x_i[c] - x_j[c])^2 (float32, bitwise symmetric, zero diagonal: the first N * N floats of
 *                       the workspace) and, with labels, the problems' row lists with alpha = 0, G = -1
 *   gcc_svc_solve       at most iters_per_launch SMO iterations of every unfinished problem (Fan, Chen, Lin 2005, WSS 2: alpha and
 *                       G float64, kernel values (float)exp(-gamma[fold] * d2), ties to the lowest row of the problem);
 *                       *unfinished = the number of problems that need another launch
 *   gcc_svc_predict     for every corpus row and every class pair of the row's own fold sum_t alpha_t y_t K(t, row) - rho in
 *                       float64 (positive: class ci), and libsvm's vote: pairs in (ci < cj) order, ties to the lowest class
 * The three calls share args and workspace; the workspace carries alpha, G and the iteration counts between them.  A pair
 * one of whose classes has no training row in the fold is not solved and does not vote. */
#define GCC_SVC_MAX_ROWS 16384
#define GCC_SVC_MAX_DIM 256
#define GCC_SVC_MAX_PROBLEM_ROWS 4096
#define GCC_SVC_MAX_CLASSES 32
#define GCC_SVC_MAX_FOLDS 64
#define GCC_STATUS_SVC_BAD_LABEL     1   /* a label outside [0, classes): the row trains nothing (it is still predicted) */
#define GCC_STATUS_SVC_BAD_FOLD      2   /* a fold id outside [0, folds): the row is left out, pred -1 */
#define GCC_STATUS_SVC_MISSING_CLASS 4   /* a fold's training side lacks a class that its test side has */
#define GCC_STATUS_SVC_NONFINITE     8   /* an embedding is NaN or infinite */
#define GCC_STATUS_SVC_ITER_CAP      16  /* a problem stopped at the iteration cap before eps was reached */
#define GCC_STATUS_SVC_OVERFLOW      32  /* a problem has more rows than max_rows: not solved */
typedef struct gcc_svc_args {
    const float *emb; int64_t ld;          /* device [N, ld], ld >= D */
    const int32_t *labels, *fold_of_row;   /* device [N]: class 0..classes-1; the fold whose TEST side holds the row */
    const double *gamma;                   /* device [folds]: 1 / (D * var(the fold's training rows)) for sklearn's "scale" */
    int32_t N, D, classes, folds;
    int32_t max_rows;                      /* the largest problem's rows, at most GCC_SVC_MAX_PROBLEM_ROWS */
    int32_t iters_per_launch;              /* gcc_svc_solve: SMO iterations of one launch per problem, >= 1 */
    int32_t iter_cap;                      /* total iterations of one problem; 0: libsvm's max(10^7, 100 rows) */
    int32_t reserved_;
    double C, eps;                         /* box bound; stop when max_{I_up} - min_{I_low} < eps */
    int32_t *pred;                         /* device [N] out or NULL: the voted class, -1 without a vote */
    double *decision;                      /* device [N, classes (classes - 1) / 2] out or NULL; 0 for a pair that was not solved */
    int32_t *iters;                        /* device [folds * pairs] out or NULL (problem = fold * pairs + pair), as the next five */
    double *rho, *obj;                     /* obj: the dual objective sum_t alpha_t (G_t - 1) / 2 */
    int32_t *n_free, *n_bounded;           /* support vectors with 0 < alpha < C / with alpha = C */
    int32_t *problem_rows;                 /* written by gcc_svc_distances, as first_rows and rows_out */
    int32_t *unfinished;                   /* device int32[1], gcc_svc_solve */
    int32_t *first_rows;                   /* device [folds * pairs] out or NULL: the problem's rows of class ci (they come first) */
    int32_t *rows_out;                     /* device [folds * pairs, max_rows] out or NULL: the problem's corpus rows in its order */
    double *alpha_out;                     /* device [folds * pairs, max_rows] out or NULL: alpha of a finished problem (gcc_svc_solve);
                                              entries past problem_rows are not written in either */
} gcc_svc_args;
/* bytes of workspace: N * N * 4 for the distances + O(folds * pairs * max_rows); negative on a size out of range, and
 * gcc_last_error() names it (max_rows beyond GCC_SVC_MAX_PROBLEM_ROWS among them) */
int64_t gcc_svc_workspace_bytes(int32_t N, int32_t D, int32_t classes, int32_t folds, int32_t max_rows);
/* status: device int32[1], OR-ed, zeroed by the caller.  A size out of range, a NULL member the call needs, ld < D and a short
 * workspace return rc < 0, name the member in gcc_last_error() and launch nothing.  No host synchronisation in any of them:
 * the caller reads *unfinished after a gcc_svc_solve and launches again while it is not 0.  labels == fold_of_row == NULL in
 * gcc_svc_distances: the distances only. */
int32_t gcc_svc_distances(const gcc_svc_args *a, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream);
int32_t gcc_svc_solve(const gcc_svc_args *a, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream);
int32_t gcc_svc_predict(const gcc_svc_args *a, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream);

/* The grid search over C of the same task (svc_classify(x, y, search=True): GridSearchCV(SVC(), {"C": [...]}, cv=inner,
 * scoring="accuracy") per outer fold, refit at the winner).  inner_of_row[o, r] is the inner fold of row r on outer fold o's
 * training side (-1 on its test side; the caller computes it, for the reference with StratifiedKFold(inner) over the
 * training rows in corpus order).  An inner problem is (outer fold o, inner fold i, class pair, candidate c): it trains on the rows
 * with fold_of_row != o and inner_of_row[o] != i, with C = Cs[c] and gamma = inner_gamma[o, i], from alpha = 0; problem index
 * ((o * inner + i) * pairs + pair) * candidates + c.  The candidates of one (o, i, pair) share their row list.  All of them are
 * solved side by side over the ONE distance matrix, one workgroup each, by the solver of gcc_svc_solve:
 *   gcc_svc_search_setup    the distances, the row lists and cold starts of the inner problems and of the refit's (fold, pair) problems
 *   gcc_svc_search_solve    at most iters_per_launch iterations of every unfinished inner problem; *unfinished as gcc_svc_solve
 *   gcc_svc_search_score    every row's vote (gcc_svc_predict's sum and vote) as a held-out row of each outer fold other than its
 *                           own, under every candidate: correct[o, c, i] = the right votes among the rows of inner fold i (integer
 *                           atomics; a row none of whose pairs was solved has no vote and counts as wrong).  The caller reads the
 *                           table, picks the winners and writes C_of_fold
 *   gcc_svc_search_refit    gcc_svc_solve on the (fold, pair) problems with C = C_of_fold[fold]; *unfinished likewise
 *   gcc_svc_search_predict  gcc_svc_predict on them
 * For a fold whose C_of_fold is C the refit's outputs are bit-identical to those of the gcc_svc_* calls with that C.  The bits that
 * the inner problems raise (MISSING_CLASS where an inner training side lacks a class, ITER_CAP, ...) go to *search_status, those of
 * the distances and the refit to *status.  Limits: at most GCC_SVC_SEARCH_MAX_CANDIDATES candidates, 2..GCC_SVC_SEARCH_MAX_INNER
 * inner folds, folds * inner * pairs * candidates <= GCC_SVC_SEARCH_MAX_PROBLEMS (one workgroup and 16 * max_inner_rows bytes of
 * workspace each), max_inner_rows <= max_rows <= GCC_SVC_MAX_PROBLEM_ROWS. */
#define GCC_SVC_SEARCH_MAX_CANDIDATES 16
#define GCC_SVC_SEARCH_MAX_INNER 16
#define GCC_SVC_SEARCH_MAX_PROBLEMS 32768
typedef struct gcc_svc_search_args {
    const float *emb; int64_t ld;          /* device [N, ld], ld >= D */
    const int32_t *labels, *fold_of_row;   /* device [N], as gcc_svc_args */
    const int32_t *inner_of_row;           /* device [folds, N] */
    const double *gamma;                   /* device [folds]: the refit's, as gcc_svc_args */
    const double *inner_gamma;             /* device [folds, inner] */
    const double *Cs;                      /* device [candidates], each > 0 */
    const double *C_of_fold;               /* device [folds], read by gcc_svc_search_refit only */
    int32_t N, D, classes, folds, inner, candidates;
    int32_t max_rows;                      /* the largest refit problem's rows */
    int32_t max_inner_rows;                /* the largest inner problem's rows */
    int32_t iters_per_launch, iter_cap;    /* as gcc_svc_args, per problem */
    double eps;
    int32_t *unfinished;                   /* device int32[1] */
    int32_t *search_status;                /* device int32[1], OR-ed, zeroed by the caller */
    int32_t *correct;                      /* device [folds, candidates, inner] out (gcc_svc_search_score zeroes it first) */
    int32_t *search_iters;                 /* device [folds, inner, pairs, candidates] out or NULL, as search_rho */
    double *search_rho;
    int32_t *search_problem_rows, *search_first_rows;   /* device [folds, inner, pairs] out or NULL */
    int32_t *search_rows;                  /* device [folds * inner * pairs, max_inner_rows] out or NULL */
    double *search_alpha;                  /* device [folds * inner * pairs * candidates, max_inner_rows] out or NULL */
    int32_t *pred;                         /* the refit's outputs, as gcc_svc_args: [N] */
    double *decision;
    int32_t *iters;
    double *rho, *obj;
    int32_t *n_free, *n_bounded, *problem_rows, *first_rows, *rows_out;
    double *alpha_out;
} gcc_svc_search_args;
/* bytes of workspace: N * N * 4 + O(folds * pairs * max_rows + folds * inner * pairs * candidates * max_inner_rows); negative on a
 * size out of range, and gcc_last_error() names the limit */
int64_t gcc_svc_search_workspace_bytes(int32_t N, int32_t D, int32_t classes, int32_t folds, int32_t inner, int32_t candidates,
                                       int32_t max_rows, int32_t max_inner_rows);
/* as the gcc_svc_* calls: rc < 0 and nothing launched on a size out of range, a NULL member or a short workspace; no host
 * synchronisation */
int32_t gcc_svc_search_setup(const gcc_svc_search_args *a, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream);
int32_t gcc_svc_search_solve(const gcc_svc_search_args *a, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream);
int32_t gcc_svc_search_score(const gcc_svc_search_args *a, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream);
int32_t gcc_svc_search_refit(const gcc_svc_search_args *a, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream);
int32_t gcc_svc_search_predict(const gcc_svc_search_args *a, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream);

/* ------------------------------- logistic regression on frozen embeddings ---
 * gcc/tasks/node_classification.py:53-101 of the reference: StratifiedKFold, then one-vs-rest LogisticRegression(C=1000) per fold
 * over the columns of an indicator matrix y [N, classes], and per held-out row the k classes of highest probability, k = the
 * row's label count (0 labels: every class).  Here every (fold, class) is one problem, p = fold * classes + class, over the corpus
 * rows whose fold id differs from its fold, and all problems run side by side.  A problem computes the minimiser of
 *   f(w, b) = 1/2 |w|^2 + intercept_penalty 1/2 b^2 + C sum_r [log(1 + exp(z_r)) - t_r z_r],  z_r = w . x_r + b
 * by damped Newton steps from 0 (exact Hessian on the fp64 matrix cores, Cholesky, Armijo backtracking with constant 1e-4 and
 * step halving, 64 eps |f| allowed for the rounding of f), everything in float64 on float32 rows, until max|grad f| / C <= tol.  A column that is constant on a fold's
 * training side is not solved: its decision value is -inf (all zeros) or +inf (all ones).
 *   gcc_logreg_setup     problem states, w = 0, the gradient at 0; flags fold ids out of range and non-finite embeddings
 *   gcc_logreg_step      iters_per_sync Newton iterations of every unfinished problem; *unfinished = the problems that need more
 *   gcc_logreg_predict   decision [N, classes] of every row's own fold, pred (top-k: decision descending, then class ascending),
 *                        counts [folds, 3] = tp, fp, fn, and the problems' coef / intercept / iters / grad / state
 * The calls share args and workspace.  Every sum has one fixed order that depends on the sizes alone (no floating-point atomics),
 * so every output is bit-identical for every iters_per_sync. */
#define GCC_LR_MAX_ROWS 65536
#define GCC_LR_MAX_DIM 256
#define GCC_LR_MAX_CLASSES 256
#define GCC_LR_MAX_FOLDS 16
#define GCC_STATUS_LR_BAD_FOLD    1   /* a fold id outside [0, folds): the row trains nothing, pred 0, decision 0 */
#define GCC_STATUS_LR_NONFINITE   2   /* an embedding is NaN or infinite */
#define GCC_STATUS_LR_ITER_CAP    4   /* a problem stopped at iter_cap before tol was reached */
#define GCC_STATUS_LR_PIVOT       8   /* a problem met a non-positive pivot in the Cholesky factorisation and stopped */
#define GCC_STATUS_LR_LINE_SEARCH 16  /* a problem's step shrank below 2^-40 without a decrease and the problem stopped */
/* state of a problem: 0 running, 1 converged, 2 at the iteration cap, 3 not solved (all zeros), 4 not solved (all ones),
 * 5 stopped at a pivot, 6 stopped in the line search, 7 not run (GCC_STATUS_LR_NONFINITE: w = 0) */
typedef struct gcc_logreg_args {
    const float *emb; int64_t ld;          /* device [N, ld], ld >= D */
    const uint8_t *y;                      /* device [N, classes]: non-zero = the row has the label */
    const int32_t *fold_of_row;            /* device [N]: the fold whose TEST side holds the row */
    int32_t N, D, classes, folds;
    int32_t iters_per_sync;                /* gcc_logreg_step: Newton iterations per call, >= 1 */
    int32_t iter_cap;                      /* total Newton iterations of one problem, >= 1 */
    double C, tol;
    double intercept_penalty;              /* rho: 0 = sklearn >= 0.22's objective (lbfgs), 1 = liblinear's */
    uint8_t *pred;                         /* device [N, classes] */
    double *decision;                      /* device [N, classes] or NULL */
    int32_t *counts;                       /* device [folds, 3] or NULL: tp, fp, fn over the fold's held-out rows */
    double *coef, *intercept;              /* device [folds * classes, D] / [folds * classes] or NULL */
    int32_t *iters;                        /* device [folds * classes] or NULL */
    double *grad;                          /* device [folds * classes] or NULL: the last max|grad f| / C */
    int32_t *state;                        /* device [folds * classes] or NULL */
    int32_t *unfinished;                   /* device int32[1], gcc_logreg_step */
} gcc_logreg_args;
/* bytes of workspace, with P = folds * classes, Dpad = D + 1 rounded up to 16, tiles = (Dpad / 16)(Dpad / 16 + 1) / 2 and
 * splits = min(64, ceil(1024 / (P tiles)), ceil(N / 64)) row splits (re-derived from their rows, a multiple of 32):
 *   3 P N 8 (Z, Zd, the Hessian weights) + P splits tiles 2048 (Hessian parts) + P (D + 1)^2 8 where D > 128 (the Cholesky
 *   that leaves LDS) + P (gsplits + 3) Dpad 8 (gradient parts in gsplits = ceil(N / (ceil(N / 64) rounded up to 256)) <= 64 row
 *   splits of their own, w, g, d) + 24 P, each array rounded up to 256 bytes.
 * Negative on a size out of range, and gcc_last_error() names it. */
int64_t gcc_logreg_workspace_bytes(int32_t N, int32_t D, int32_t classes, int32_t folds);
/* status: device int32[1], OR-ed, zeroed by the caller.  A size out of range, a NULL member the call needs, ld < D and a short
 * workspace return rc < 0, name the member in gcc_last_error() and launch nothing.  No host synchronisation in any of them: the
 * caller reads *unfinished after a gcc_logreg_step and calls again while it is not 0. */
int32_t gcc_logreg_setup(const gcc_logreg_args *a, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream);
int32_t gcc_logreg_step(const gcc_logreg_args *a, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream);
int32_t gcc_logreg_predict(const gcc_logreg_args *a, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream);

/* ---- ProNE node embeddings of a parent graph (csrc/prone.hip): the baseline of the reference's node classification
 * (gcc/models/emb/prone.py).  Input: a simple undirected graph as symmetric CSR in node-id order, rows sorted, no self loops.
 * Everything is float64; k = d + 10 is the width of the randomized range finder.
 *   node terms   r_i = -log(deg_i), s_j = sum_{i in N(j)} 1 / deg_i, c_j = -log(s_j^0.75 / sum_j s_j^0.75).  The factorised
 *                matrix F has A's pattern and the values F_ij = r_i + c_j; it is never stored.
 *   products     y = op x (+ tail) for x, y [n, k] row-major (gcc_prone_spmm), op one of GCC_PRONE_MODE_*.
 *   orthonormalisation  CholeskyQR2 of y [n, k] in place (gcc_prone_orthonormalize).
 *   the pipeline  sklearn's randomized_svd(F, d, n_iter=5) from a given Omega, svd_flip (per column the entry of largest
 *                magnitude positive, ties to the lowest row), U sqrt(Sigma), rows L2-normalised; then the Chebyshev-Gaussian
 *                propagation of `step` terms and the same finish on the thin SVD of its result (gcc_prone_embed).
 * ORDER OF A ROW'S SUM: the neighbours are taken in CSR order in segments of GCC_PRONE_SEGMENT; a segment is summed left to
 * right, the segment sums are added as a binary counter adds them (two sums of 2^l segments each make one of 2^(l+1); what is
 * left at the end is added from the lowest level up).  A row longer than `chunk` neighbours is split into parts of `chunk`, one
 * wave group each, whose sums go to the workspace and are added by the same rule; `chunk` is GCC_PRONE_SEGMENT times a power of
 * two, so every chunk gives the same bits.  No floating-point atomics anywhere: every sum depends on the sizes alone.  The one
 * implementation of the counter is SumCounter in gcc_amd/csrc/task_common.h; gcc_graphwave_* sums with it too. */
#define GCC_PRONE_MAX_DIM 64
#define GCC_PRONE_OVERSAMPLE 10
#define GCC_PRONE_MAX_K (GCC_PRONE_MAX_DIM + GCC_PRONE_OVERSAMPLE)
#define GCC_PRONE_MAX_STEP 32
#define GCC_PRONE_SEGMENT 32
#define GCC_PRONE_CHUNK 1024          /* neighbours of one part of a split row (args.chunk = 0) */
#define GCC_PRONE_MAX_CHUNK 4096
#define GCC_PRONE_POWER_ITERS 5       /* randomized_svd's n_iter */
#define GCC_PRONE_MODE_F  0           /* y_i = sum_{j in N(i)} (r_i + c_j) x_j */
#define GCC_PRONE_MODE_FT 1           /* y_i = sum_{j in N(i)} (r_j + c_i) x_j */
#define GCC_PRONE_MODE_M  2           /* m_i = ((1 - 1/(deg_i + 1)) - mu) x_i - (sum_{j in N(i)} x_j) / (deg_i + 1), then the tail */
#define GCC_PRONE_MODE_A1 3           /* y_i = (x_i - z_i) + sum_{j in N(i)} (x_j - z_j) */
#define GCC_PRONE_TAIL_NONE 0         /* y = m */
#define GCC_PRONE_TAIL_HALF 1         /* y = 0.5 m - z;  conv = alpha z + beta y      (prone.py l.91-94) */
#define GCC_PRONE_TAIL_CHEB 2         /* y = (m - 2 z) - w;  conv += alpha y          (prone.py l.97-102); y may be w */
#define GCC_STATUS_PRONE_BAD_CSR    1   /* row_ptr not ascending from 0 to nnz, a column outside [0, n), a self loop or an unsorted row */
#define GCC_STATUS_PRONE_DUPLICATE  2   /* a repeated entry in a row: a multigraph parent */
#define GCC_STATUS_PRONE_SPLIT_FULL 4   /* the split rows of this chunk do not fit the workspace */
#define GCC_STATUS_PRONE_RANK       8   /* orthonormalisation met a pivot that is not positive: the range lost rank */
#define GCC_STATUS_PRONE_SWEEPS    16   /* the eigensolver stopped at its sweep limit */
#define GCC_STATUS_PRONE_SINGULAR  32   /* a singular value not above n eps sigma_1 */
/* any of BAD_CSR, SPLIT_FULL, RANK and SINGULAR ends the call where it is met: the kernels after it return at once, and an output
 * that was not reached keeps what it held: the zeros gcc_prone_embed puts there first, or the factorisation's rows when the
 * propagation's decomposition is what failed.  No NaN is written. */
typedef struct gcc_prone_args {
    const int32_t *row_ptr, *col_idx;      /* device [n + 1], [nnz] */
    int64_t n, nnz;                        /* both within int32 */
    int32_t d;                             /* 2..GCC_PRONE_MAX_DIM; n >= d + 10 */
    int32_t step;                          /* gcc_prone_embed: 1..GCC_PRONE_MAX_STEP; 1 returns the factorisation's rows */
    int32_t chunk;                         /* 0: GCC_PRONE_CHUNK; else GCC_PRONE_SEGMENT 2^j up to GCC_PRONE_MAX_CHUNK */
    int32_t mode, tail, k;                 /* gcc_prone_spmm / gcc_prone_orthonormalize: columns of x and y, 1..GCC_PRONE_MAX_K */
    double mu;                             /* gcc_prone_embed, GCC_PRONE_MODE_M */
    double alpha, beta;                    /* gcc_prone_spmm: the tail's coefficients */
    double bessel[GCC_PRONE_MAX_STEP];     /* gcc_prone_embed: I_i(theta), i < step */
    double *r, *c;                         /* device [n] or NULL (then the workspace holds them) */
    const double *x, *z, *w;               /* gcc_prone_spmm: device [n, k]; y must not be x */
    double *y, *conv;                      /* gcc_prone_spmm out; gcc_prone_orthonormalize: y in place */
    double *rfac;                          /* gcc_prone_orthonormalize: device [2, k, k] or NULL: R of the two passes, y_in = q R2 R1 */
    const double *omega;                   /* gcc_prone_embed: device [n, d + 10] */
    double *emb; float *emb32;             /* gcc_prone_embed out: device [n, d] */
    double *sigma;                         /* gcc_prone_embed out: device [2, d] (factorisation, propagation) or NULL */
} gcc_prone_args;
/* bytes of workspace: r, c, the split rows' lists and partial sums (2 nnz / GCC_PRONE_CHUNK + 64 parts of 80 float64), the Gram
 * partials, the small factors, n d float64 of projected rows and max(2 n (d + 10), 5 n d) float64 of iterates.  Negative on a
 * size out of range, and gcc_last_error() names it. */
int64_t gcc_prone_workspace_bytes(int64_t n, int64_t nnz, int32_t d);
/* status: device int32[1], OR-ed, zeroed by the caller.  A size out of range, a NULL member the call needs and a short workspace
 * return rc < 0, name the member in gcc_last_error() and launch nothing.  No host synchronisation in any of them.  The calls share
 * args and workspace; gcc_prone_spmm in modes F / FT reads r and c (gcc_prone_node_terms, or the caller's own). */
int32_t gcc_prone_node_terms(const gcc_prone_args *a, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream);
int32_t gcc_prone_spmm(const gcc_prone_args *a, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream);
int32_t gcc_prone_orthonormalize(const gcc_prone_args *a, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream);
int32_t gcc_prone_embed(const gcc_prone_args *a, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream);

/* ---- GraphWave node embeddings of a parent graph (csrc/graphwave.hip): the second baseline of the reference's node
 * classification and similarity search (gcc/models/emb/graphwave.py), as the reference calls it.  Input: an undirected graph as
 * symmetric CSR in node-id order, rows sorted, no self loops; a repeated entry is a parallel edge and counts.  Everything is
 * float64.  With n the number of rows that have an entry (a row without one is a node id outside the graph: it takes part in no
 * mean and its row of the table is zero) and T = d / 4:
 *   operator     M = -D^-1/2 A D^-1/2, deg_i = the entries of row i, 1 / sqrt(deg_i) = 0 for an empty row.
 *   heat         H_i = sum_{k = 0..GCC_GRAPHWAVE_ORDER} coeff[i][k] T_k(M), T_0 = I, T_1 = M, T_k = 2 M T_{k-1} - T_{k-2}, computed
 *                on panels of W source columns ([n_rows, W] row-major), one launch per order; then x -> x > threshold / n ? x : 0.
 *   table        chi[u][i 2T + 2j] = (sum_v cos(time_points[j] H_i[v][u])) / n, chi[u][i 2T + 2j + 1] the same with sin.
 * ORDER OF THE SUMS: a row's product sum takes the neighbours in CSR order in segments of GCC_PRONE_SEGMENT, a segment left to
 * right, the segments as a binary counter adds them (see above).  A column's sum over the rows takes blocks of
 * GCC_GRAPHWAVE_ROW_BLOCK rows from row 0 (four runs of 32 rows, left to right, added as (0 + 1) + (2 + 3)), the blocks by the
 * same counter.  Neither depends on W or on the grid: every panel width gives the same bits.  No floating-point atomics. */
#define GCC_GRAPHWAVE_ORDER 30
#define GCC_GRAPHWAVE_MAX_DIM 256
#define GCC_GRAPHWAVE_MAX_NODES 65536
#define GCC_GRAPHWAVE_MAX_WIDTH 4096
#define GCC_GRAPHWAVE_ROW_BLOCK 128
#define GCC_STATUS_GRAPHWAVE_BAD_CSR 1  /* row_ptr not ascending from 0 to nnz, a column outside [0, n_rows), a self loop or an unsorted row */
/* GCC_STATUS_GRAPHWAVE_BAD_CSR ends the call where it is met: the kernels after it return at once and the outputs keep the zeros
 * the call puts there first.  No NaN is written. */
typedef struct gcc_graphwave_args {
    const int32_t *row_ptr, *col_idx;      /* device [n_rows + 1], [nnz] */
    int64_t n_rows, nnz;                   /* 2..GCC_GRAPHWAVE_MAX_NODES; nnz within int32 */
    int32_t d;                             /* a multiple of 4 in 4..GCC_GRAPHWAVE_MAX_DIM */
    int32_t width;                         /* columns of a panel: 0 (gcc_graphwave_panel_width's default) or a multiple of 64 */
    int32_t heat_chunk;                    /* gcc_graphwave_heat: the panel, columns [heat_chunk W, (heat_chunk + 1) W) */
    int32_t reserved;
    double coeff[2][GCC_GRAPHWAVE_ORDER + 1];          /* the Chebyshev coefficients of the two scales */
    double time_points[GCC_GRAPHWAVE_MAX_DIM / 4];     /* the first d / 4 are read */
    double threshold;                      /* divided by n on the device (the reference: 1e-4) */
    double *chi; float *chi32;             /* gcc_graphwave_embed out: device [n_rows, d] */
    double *heat;                          /* gcc_graphwave_heat out: device [2, n_rows, W], after the threshold; rows and columns
                                            * of empty rows and columns past n_rows are zero */
} gcc_graphwave_args;
/* the columns of one panel: `width` itself (a multiple of 64 up to GCC_GRAPHWAVE_MAX_WIDTH), or for 0 the widest multiple of 64
 * up to 2048 whose workspace stays within 256 MiB, at most n_rows rounded up to 64.  Negative on a size out of range. */
int64_t gcc_graphwave_panel_width(int64_t n_rows, int32_t d, int32_t width);
/* bytes of workspace: n_rows float64 of node scales, four panels [n_rows, W] (two Chebyshev iterates, two heat sums) and the
 * row blocks' partial sums [n_rows / GCC_GRAPHWAVE_ROW_BLOCK, d, W].  Negative on a size out of range, gcc_last_error() names it. */
int64_t gcc_graphwave_workspace_bytes(int64_t n_rows, int64_t nnz, int32_t d, int32_t width);
/* status: device int32[1], OR-ed, zeroed by the caller.  A size out of range, a NULL member the call needs and a short workspace
 * return rc < 0, name the member in gcc_last_error() and launch nothing.  No host synchronisation in either. */
int32_t gcc_graphwave_heat(const gcc_graphwave_args *a, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream);
int32_t gcc_graphwave_embed(const gcc_graphwave_args *a, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream);

/* ---- Raw edge lines -> the sampler's contract CSR, and the contract check on the device (csrc/graph_build.hip).  The rule is the
 * reference converter's (gcc/utils/x2dgl.py, yuxiao_kdd17_graph_to_dgl): the lines u == v are dropped, both directions of the rest
 * inserted, one entry kept per non-zero, the nodes without an entry removed, the survivors relabelled in ascending old-id order,
 * rows sorted ascending.  Integer arithmetic and integer atomics only: the output depends on the set of lines alone, so any order
 * of the lines and any two calls give the same bits.
 * ROW CLASSES: a row of up to GCC_GRAPH_BUILD_WAVE_ROW slots (before the repeats are removed) is sorted by one wave in registers,
 * one of up to GCC_GRAPH_BUILD_LDS_ROW by one workgroup in LDS, a longer one in chunks of GCC_GRAPH_BUILD_LDS_ROW that are merged
 * in the workspace.  The scans work on tiles of GCC_GRAPH_BUILD_SCAN_TILE words. */
#define GCC_GRAPH_BUILD_WAVE_ROW 64
#define GCC_GRAPH_BUILD_LDS_ROW 2048
#define GCC_GRAPH_BUILD_SCAN_TILE 1024
#define GCC_STATUS_GRAPH_BUILD_BAD_ID 1  /* a line names an id outside [0, n): the line was ignored */
typedef struct gcc_graph_build_args {
    const int32_t *pairs;                  /* device [m][2]: the lines' two ids, either order, repeats and u == v allowed */
    int64_t n, m;                          /* declared nodes 1..2^31 - 1; lines, 2 m < 2^31 */
    int32_t *row_ptr, *col_idx;            /* out, device: capacities [n + 1] and [2 m]; counts[0] + 1 and counts[1] words are written */
    int32_t *node_map;                     /* out, device [n] or NULL: old id -> new id, -1 for a removed node */
    int64_t *counts;                       /* out, device [6]: nodes kept, entries written, u == v lines dropped, repeated directed
                                            * slots dropped, nodes removed for having no entry, the longest row */
} gcc_graph_build_args;
/* bytes of workspace: six words per node, the scans' tile sums, the two row lists and one copy of the 2 m slots (two when a row
 * can exceed GCC_GRAPH_BUILD_LDS_ROW).  Negative on a size out of range, gcc_last_error() names it. */
int64_t gcc_graph_build_workspace_bytes(int64_t n, int64_t m);
/* status: device int32[1], OR-ed, zeroed by the caller.  A size out of range, a NULL member the call needs and a short workspace
 * return rc < 0, name the member in gcc_last_error() and launch nothing.  No host synchronisation: the caller reads counts and
 * status once and slices row_ptr / col_idx. */
int32_t gcc_graph_build(const gcc_graph_build_args *a, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream);

/* the contract a parent graph must obey, one bit per violation (gcc_amd.graphgen.check_contract / check_multigraph_contract) */
#define GCC_STATUS_GRAPH_CHECK_SPAN 1          /* row_ptr does not run from 0 to nnz within [0, nnz] */
#define GCC_STATUS_GRAPH_CHECK_ZERO_DEGREE 2   /* a row without an entry */
#define GCC_STATUS_GRAPH_CHECK_RANGE 4         /* a column outside [0, n) */
#define GCC_STATUS_GRAPH_CHECK_UNSORTED 8      /* a row that descends */
#define GCC_STATUS_GRAPH_CHECK_SELF_LOOP 16
#define GCC_STATUS_GRAPH_CHECK_DUPLICATE 32    /* a repeated entry (multigraph == 0 only) */
#define GCC_STATUS_GRAPH_CHECK_ASYMMETRIC 64   /* an entry without its reverse; multigraph: unequal copy counts in the two directions */
typedef struct gcc_graph_check_args {
    const int32_t *row_ptr, *col_idx;      /* device [n + 1], [nnz] */
    int64_t n, nnz;
    int32_t multigraph, reserved;          /* 1: repeated entries are parallel edges */
    int32_t *maxima;                       /* out, device int32[2]: the longest row, the most copies of one entry in a row */
} gcc_graph_check_args;
/* Writes status and maxima, nothing else; the workspace is not used and may be NULL.  Three steps, each run only on what the one
 * before it found sound (the status word must come in as 0): row_ptr (SPAN, ZERO_DEGREE, maxima[0]); every entry in its row, found
 * by a binary search in a row_ptr that climbs (RANGE, UNSORTED, SELF_LOOP, DUPLICATE); the reverse entries, found by a binary
 * search in sorted rows (ASYMMETRIC, maxima[1]).  The lowest bit set is the violation gcc_amd.graphgen.check_contract names. */
int32_t gcc_graph_check(const gcc_graph_check_args *a, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream);

/* ---- The sampler's tables from a CSR that is already in HBM (csrc/graph_tables.hip): what gcc_amd.graph builds on the host at
 * upload -- the summary a DeviceGraph sizes itself with, the seed cdf (deg^0.75 per worker shard) and the hub index / hub-hub
 * bitmap of gcc_graph.  Two calls, one host read between them: gcc_graph_tables fills summary, seed_cdf and hub_index; the caller
 * reads summary (GCC_GRAPH_TABLES_SUMMARY_WORDS int64), sizes hub_adj from summary[3] and calls gcc_graph_tables_hub_adj.
 * The integer outputs are exact.  THE CDF: float64 sums in an order the tile grid alone fixes (tiles of
 * GCC_GRAPH_TABLES_SCAN_TILE nodes that never straddle a shard; any grid size and any two calls give the same bits), carried
 * forward so that the cdf never descends within a shard, ends in exactly 1.0 and stays within (n_s + 64) * 2^-53 of the exact
 * cdf of a shard of n_s nodes.  The bitmap is built from tiles of GCC_GRAPH_TABLES_ENTRY_TILE entries. */
#define GCC_GRAPH_TABLES_SCAN_TILE 2048
#define GCC_GRAPH_TABLES_ENTRY_TILE 1024
#define GCC_GRAPH_TABLES_HUB_DEGREE 512      /* hub_degree == 0 */
#define GCC_GRAPH_TABLES_SUMMARY_WORDS 8
#define GCC_STATUS_GRAPH_TABLES_EMPTY_SHARD 1 /* a shard's total deg^0.75 weight is zero or not finite: its cdf is all 1.0 */
typedef struct gcc_graph_tables_args {
    const int32_t *row_ptr, *col_idx;      /* device [n + 1], [nnz] (col_idx: gcc_graph_tables_hub_adj only) */
    int64_t n, nnz;                        /* 1 <= n, both within int32 */
    const int64_t *shard_off;              /* HOST [num_shards + 1]: increasing from 0 to n; may be NULL when num_shards <= 1 */
    int32_t num_shards;                    /* <= 1: one shard covers all nodes */
    int32_t hub_degree;                    /* rows of at least this many entries are hubs; 0: GCC_GRAPH_TABLES_HUB_DEGREE */
    int64_t max_hub_bytes;                 /* gcc_graph_tables_hub_adj refuses a larger bitmap; 0: 1 GiB */
    int32_t grid, reserved;                /* workgroups of the tile kernels; 0: sized from the input (the outputs do not depend on it) */
    int64_t *summary;                      /* out, device [GCC_GRAPH_TABLES_SUMMARY_WORDS]: the longest row, sum d, sum d^2, hubs, the
                                            * status bits this call set, num_shards - (the lowest shard without weight), 0, 0 */
    double *seed_cdf;                      /* out, device [n] */
    int32_t *hub_index;                    /* out, device [n], or NULL (gcc_graph_tables: not built); in for gcc_graph_tables_hub_adj */
    uint32_t *hub_adj;                     /* out of gcc_graph_tables_hub_adj, device [num_hubs][hub_words] */
    int32_t num_hubs, hub_words;           /* gcc_graph_tables_hub_adj: summary[3] and (num_hubs + 31) / 32 */
} gcc_graph_tables_args;
/* bytes of workspace of gcc_graph_tables: three words per tile and the shard table.  Negative on a size out of range. */
int64_t gcc_graph_tables_workspace_bytes(int64_t n, int32_t num_shards);
/* status: device int32[1], OR-ed, zeroed by the caller.  A size out of range, a NULL member the call needs, a shard_off that does
 * not run from 0 to n in increasing order and a short workspace return rc < 0, name what is wrong in gcc_last_error() and launch
 * nothing.  No host synchronisation (shard_off is copied before the call returns). */
int32_t gcc_graph_tables(const gcc_graph_tables_args *a, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream);
/* hub_adj of the hubs hub_index numbers: zeroed, then one bit per entry of a hub's row that names a hub.  The workspace is not
 * used and may be NULL.  Refuses num_hubs < 1, a hub_words that does not fit and a bitmap above max_hub_bytes. */
int32_t gcc_graph_tables_hub_adj(const gcc_graph_tables_args *a, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream);

/* ---- Edge-list text that is already in HBM -> line ends and int32 records (csrc/text_ingest.hip): the first stage of
 * gcc_amd.ingest.read_lscc on the device.  THE TOKEN RULE is bytes.split()'s: the separators are the six bytes 9, 10, 11, 12, 13
 * and 32; a token starts at byte i >= first_byte when text[i] is no separator and (i == first_byte or text[i - 1] is one) and runs
 * to the next separator or the end of the text.  Token r, counted from first_byte, is field r % fields of record r / fields.  A
 * valid token is at most one '+' or '-' followed by one or more ASCII digits (leading zeros are fine, -0 is 0, an underscore is not
 * a digit); a token of any length is classified, never wrapped.
 * THE BUFFER: `text` is aligned to 16 bytes and has a capacity of at least nbytes rounded up to 16 (the kernels load 16 bytes at
 * a time and never a ragged tail); what the bytes at and above nbytes hold does not matter.
 * Work is cut into tiles of GCC_TEXT_TILE_BYTES bytes; one workgroup scans the tiles' counts, GCC_TEXT_SCAN_TILES tiles per pass.
 * Integer min and integer or are the only atomics: any grid and any two calls give the same words. */
#define GCC_TEXT_TILE_BYTES 4096
#define GCC_TEXT_SCAN_TILES 1024
#define GCC_TEXT_MAX_QUERIES 16
#define GCC_STATUS_TEXT_NOT_INTEGER 1   /* one of the first max_tokens tokens is not an integer: summary[1] */
#define GCC_STATUS_TEXT_INT32_RANGE 2   /* a kept token's value is outside int32: summary[2] */
#define GCC_STATUS_TEXT_SHORT 4         /* fewer than max_tokens tokens: summary[0] */
typedef struct gcc_text_line_ends_args {
    const uint8_t *text;                   /* device [capacity] */
    int64_t nbytes, capacity;              /* 1 <= nbytes <= 2^40; capacity >= nbytes rounded up to 16 */
    const int64_t *lines;                  /* HOST [num_lines]: zero-based line numbers, any order, repeats allowed */
    int32_t num_lines, reserved;           /* 0..GCC_TEXT_MAX_QUERIES */
    int64_t *ends;                         /* out, device [num_lines + 1]: the offset of the newline (byte 10) that ends line
                                            * lines[i], -1 where the text has fewer lines; ends[num_lines]: the newlines of the text */
} gcc_text_line_ends_args;
typedef struct gcc_text_ints_args {
    const uint8_t *text;                   /* device [capacity] */
    int64_t nbytes, capacity;
    int64_t first_byte;                    /* 0..nbytes: the bytes below it are not looked at */
    int64_t max_tokens;                    /* a multiple of fields; max_tokens / fields * keep < 2^31 */
    int32_t fields, keep;                  /* tokens per record 1..4; the leading fields of a record that are stored, 1..fields */
    int32_t *out;                          /* out, device [max_tokens / fields][keep]; a kept token that is no integer or outside
                                            * int32 stores 0; the words of tokens the text does not have are left alone */
    int64_t *summary;                      /* out, device [4]: tokens in [first_byte, nbytes) (uncapped); the offset of the lowest
                                            * of the first max_tokens tokens that is not an integer, or -1; the offset of the lowest
                                            * kept token outside int32, or -1; 0 */
} gcc_text_ints_args;
/* bytes of workspace: 24 per tile (a count and an int64 offset for the token starts and for the newlines).  Negative on a size out of range. */
int64_t gcc_text_line_ends_workspace_bytes(int64_t nbytes);
int64_t gcc_text_ints_workspace_bytes(int64_t nbytes);
/* A size out of range, a NULL member the call needs, a capacity below the padded size, a text off its alignment and a short
 * workspace return rc < 0, name what is wrong in gcc_last_error() and launch nothing.  No host synchronisation (`lines` is copied
 * before the call returns).  gcc_text_line_ends sets no status bit and accepts a NULL status; gcc_text_ints ORs its bits into
 * status (device int32[1], zeroed by the caller). */
int32_t gcc_text_line_ends(const gcc_text_line_ends_args *a, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream);
int32_t gcc_text_ints(const gcc_text_ints_args *a, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream);
/* gcc_text_ints with two knobs (the same kernels; gcc_text_ints is this call with both off).
 * extra_sep: 0, or one byte value in 1..255 that is none of the six separators and no digit, '+' or '-': a seventh separator
 * (TU's A.txt separates its two fields with ','; "1,,2" and "1 2" are then two fields as well).
 * line_records: with 1, token r counted from first_byte must be the first token on its line exactly when r % fields == 0.  "First
 * on its line": the separator run in front of it holds a byte 10, or it is the first token at or after first_byte; blank lines
 * pass, a line of more or fewer than `fields` tokens does not.  A violation among the first max_tokens tokens sets
 * GCC_STATUS_TEXT_LINE_SHAPE and summary[3] holds the offset of the lowest offending token, -1 when there is none (0 with
 * line_records == 0).  max_tokens == 0 with out == NULL counts the tokens (summary[0]) under the same separators.
 * The workspace is gcc_text_ints_workspace_bytes(nbytes). */
#define GCC_STATUS_TEXT_LINE_SHAPE 8    /* line_records: a record does not sit on a line of its own: summary[3] */
typedef struct gcc_text_ints_sep_args {
    gcc_text_ints_args ints;
    int32_t extra_sep, line_records;
} gcc_text_ints_sep_args;
int32_t gcc_text_ints_sep(const gcc_text_ints_sep_args *a, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream);

/* ---- TU dataset tables -> the resident corpus of gcc_pack_graphs (csrc/tu_corpus.hip): what gcc_amd.ingest.read_tudataset and
 * DeviceGraphCorpus.__init__ build on the host, from the integers of <NAME>_A.txt, _graph_indicator.txt and _graph_labels.txt.
 * Integer arithmetic and integer atomics only: the outputs are a function of the SET of lines, never of their order or the grid.
 * Graph ids need not start at 1 or be contiguous; a node or a graph without an entry is legal; label values may be negative or
 * sparse.  Rows of any length are served (the row classes of gcc_graph_build).
 * STATUS (device int32[1], zeroed by the caller, OR-ed): one bit per ValueError of the host reader, in the host's order, so the
 * lowest set bit names the error the host raises first.  A step runs only on what the steps before it found sound: DESCENDS and
 * GRAPH_COUNT stop everything behind them, BAD_ID stops the four behind it, SELF_LOOP and CROSS_GRAPH are found together,
 * REPEATED and ASYMMETRIC need the sorted rows and are looked for only on a clean word.  With any bit set the tables are not
 * promised; with GRAPH_COUNT set counts[0] still is. */
#define GCC_STATUS_TU_DESCENDS 1        /* graph_indicator descends somewhere */
#define GCC_STATUS_TU_GRAPH_COUNT 2     /* the distinct indicator values (counts[0]) are not num_labels many */
#define GCC_STATUS_TU_BAD_ID 4          /* a line of A.txt names an id outside [1, N] */
#define GCC_STATUS_TU_SELF_LOOP 8       /* a line u, u */
#define GCC_STATUS_TU_CROSS_GRAPH 16    /* a line joins nodes of two graphs */
#define GCC_STATUS_TU_REPEATED 32       /* a line stands twice */
#define GCC_STATUS_TU_ASYMMETRIC 64     /* a line u, v without its v, u */
typedef struct gcc_tu_corpus_args {
    const int32_t *pairs;                  /* device [m][2]: the 1-based ids as A.txt has them, any line order; NULL when m == 0 */
    const int32_t *indicator;              /* device [N]: the file's graph id of every node, in file order */
    const int32_t *graph_labels;           /* device [L]: the raw label values */
    int64_t num_nodes, num_lines, num_labels;  /* 1 <= N < 2^31 - 1, 0 <= m < 2^31, 1 <= L < 2^31 - 1 */
    int32_t *node_first;                   /* out, device [L + 1] */
    int32_t *edge_first;                   /* out, device [L + 1]: edge_first[g] = row_ptr[node_first[g]] */
    int32_t *row_ptr;                      /* out, device [N + 1]: global offsets */
    int32_t *col_idx;                      /* out, device [m]: ids local to their graph, every row ascending; NULL when m == 0 */
    int32_t *seed_local;                   /* out, device [L]: the first maximum of the degrees, 0 for a graph without entries */
    int32_t *labels;                       /* out, device [L]: 0..C-1 in ascending order of the distinct raw values */
    int64_t *counts;                       /* out, device [8]: G, C, the most nodes of a graph, the most entries of a graph, the
                                            * longest row, 0, 0, 0 */
} gcc_tu_corpus_args;
/* bytes of workspace; negative on a size out of range, gcc_last_error() names it */
int64_t gcc_tu_corpus_workspace_bytes(int64_t num_nodes, int64_t num_lines, int64_t num_labels);
/* A size out of range, a NULL member the call needs and a short workspace return rc < 0, name the member in gcc_last_error() and
 * launch nothing.  No host synchronisation: everything is enqueued on `stream`. */
int32_t gcc_tu_corpus(const gcc_tu_corpus_args *a, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GCC_AMD_H */
