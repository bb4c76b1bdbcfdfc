/* fmx.h -- C ABI of libfmx.so: the MI355X (gfx950) kernels behind the FM / DeepFM / NFM online hot path.
 *
 * The reference (haan6/fm-for-online-recommendation) has no FFI layer: its hot path is sequences of ATen ops
 * inside Python classes.  Each entry point below therefore cites the reference *op sequence* it replaces
 * (paths relative to the reference repository).  The Python classes in
 * fm-for-online-recommendation_amd/models/ bind these with ctypes (fm-for-online-recommendation_amd/fmx/_lib.py);
 * INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into caller-owned memory unless the comment says "host".  The data path allocates
 *     nothing: tables, batches, outputs and the per-step workspace (fmx_workspace_bytes) are the caller's.  What the library
 *     DOES own, per process: (a) per device, created on first use and never destroyed, two non-blocking HIP streams (one for
 *     the occurrence sorts that run beside the steps, one that stands in for the legacy default stream) and a handful of
 *     timing-disabled events ordering them against `stream`; (b) the tuning switches of fmx_set_option (process-wide, read
 *     by every call); (c) a launch sequence counter tagging the in-launch hand-offs; (d) fmx_fm_stream's MEASURING mode
 *     (kernel_ms != null) alone creates its HIP events and one temporary device buffer per call and frees them before it
 *     returns -- it synchronises the stream and is a benchmark facility, not part of the data path;
 *   - every other call is asynchronous on `stream` (a hipStream_t passed as void*) and performs no implicit
 *     synchronisation; work the library puts on its own streams is ordered behind what `stream` held at the call and
 *     `stream` is ordered behind it before the call returns.  Calls are safe to capture into a hipGraph except fmx_fm_stream
 *     (cross-stream events, optional timing); a capturing stream takes the paths without in-launch hand-offs.  A captured
 *     launch keeps the scalars the host computed at capture: under FMX_RULE_ADAM the step constants come from hyper->step on the
 *     host, so every replay repeats the captured step's constants -- an Adam step per replay needs a re-capture per step, or the
 *     *_stream / online entries, which advance the count themselves;
 *   - return value: 0 on success, a negative fmx_status otherwise; the message for the calling thread is
 *     available from fmx_last_error_string();
 *   - streams: fmx_fm_stream / fmx_deepfm_stream sort on a library-owned low-priority side stream beside the caller's stream.  HIP maps
 *     the streams of a process onto its hardware queues: a caller's stream that shares a queue with the side stream runs BEHIND the
 *     sorts (same results, 1.5 - 4 x the time per step).  Measured (tools/queue_alias.py): never with the runtime's default
 *     GPU_MAX_HW_QUEUES = 4; with 8 for the 4th and 11th stream a process creates, with 16 for every fourth.  Reuse one stream per
 *     loop.  The legacy default stream (NULL) is detoured through a library-owned one.
 *   - the library never throws.  Thread safety: calls on different tables / workspaces / streams may run concurrently;
 *     the mutable process state is (a)-(c) above plus the thread-local error string;
 *   - device-side conditions are reported through the caller's int32 error word (fmx_fwd_out_t.error and the `error`
 *     arguments): 1 = an index outside its field (that row is treated as absent), 2 = an in-launch hand-off of the update ran
 *     into its spin bound (the row update of that run was SKIPPED: the table is no longer the exact result).  2 means
 *     a dispatch-order assumption was violated; it has never been observed and is there so that a fault ends in a
 *     flag, not in a hang.
 *
 * Table layout in HBM (one flat buffer for all fields; field f owns rows [field_offsets[f], field_offsets[f+1])):
 *   FMX_LAYOUT_WEIGHTS  row = [ V[0..kp) | w | pad ]                                  row_stride >= kp + 4
 *   FMX_LAYOUT_FTRL     row = [ V[0..kp) | w, zw, nw, 0 | pad | zV[0..kp) | nV[0..kp) ]    zV at float z_offset,
 *                                                                                     row_stride >= z_offset + 2*kp
 *   FMX_LAYOUT_MOMENTS  row = [ V[0..kp) | w, mw, vw, 0 | pad | mV[0..kp) | vV[0..kp) ]    the FTRL geometry and checks;
 *                                                                                     mV at float z_offset
 * kp is k rounded up to 4, 8, 16, 32 or 64; the pad components must be zero (they then stay zero under every
 * rule).  row_stride and z_offset are in floats and multiples of 4 (16-byte pieces).  All layouts start with the
 * weights the forward pass reads, so a forward gather is ONE 64-byte request per row (k = 16) inside one 128-byte
 * line.  In the FTRL layout the state is (z, n); V and w are the weights derived from it,
 *     w = 0 if |z| <= l1 else -(z - sgn(z) l1) / ((beta + sqrt(n)) / alpha + l2)      (McMahan et al. 2013),
 * re-derived and stored by every update -- a cache, never an independent parameter: whoever writes (z, n) or changes
 * the hyper-parameters must rewrite V and w with the same formula.  In the MOMENTS layout the head of the row IS the
 * parameter and (m, v) are the first and second moments of FMX_RULE_ADAM (FMX_RULE_ADAGRAD keeps its sum of squared
 * gradients in the v slots and leaves the m slots untouched: zero).
 */
#ifndef FMX_H
#define FMX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FMX_VERSION 104 /* 0.1.4: fmx_deepfm_stream, fmx_fm_topk / fmx_fm_topk_workspace_bytes, fmx_mlp_topk /
                           fmx_mlp_topk_workspace_bytes; FMX_LAYOUT_MOMENTS, FMX_RULE_ADAGRAD / FMX_RULE_ADAM and the fields
                           appended to fmx_hyper_t, backward compatible as stated there; 0.1.3: fields as row-range pieces
                           of index columns -- field_cols / field_base / n_cols --, workspace_bytes arguments, fmx_owner_* */

typedef void *fmx_stream_t; /* hipStream_t */

enum fmx_status {
  FMX_OK = 0,
  FMX_ERR_ARG = -1,         /* null pointer / negative size / unknown enum */
  FMX_ERR_SHAPE = -2,       /* sizes inconsistent with each other (kp, row_stride, Bp, bbits ...) */
  FMX_ERR_ALIGN = -3,       /* a pointer that must be 16-byte aligned is not */
  FMX_ERR_LAUNCH = -4,      /* hipGetLastError() after a launch, or another HIP runtime error */
  FMX_ERR_UNSUPPORTED = -5  /* valid request the kernels do not cover (batch too large for the LDS sort, ...) */
};

enum fmx_layout { FMX_LAYOUT_WEIGHTS = 0, FMX_LAYOUT_FTRL = 1, FMX_LAYOUT_MOMENTS = 2 };

/* per-coordinate update rules (g = gradient summed over every occurrence of the row in the mini-batch) */
enum fmx_rule {
  FMX_RULE_SIGNADAM = 0, /* p -= lr * g / (|g| + eps): what a fresh torch.optim.Adam per call reduces to
                            (reference fm_adam.py:60,68 / :75,82).  FMX_LAYOUT_WEIGHTS */
  FMX_RULE_SGD = 1,      /* p -= lr * g (stale notebook prototypes only; parity unpinned).  FMX_LAYOUT_WEIGHTS */
  FMX_RULE_FTRL = 2,     /* FTRL-proximal on (z, n) (not in the reference; parity unpinned).  FMX_LAYOUT_FTRL */
  /* The persistent adaptive rules (not in the reference; torch.optim.Adagrad / torch.optim.SparseAdam on
     nn.Embedding(sparse=True)).  FMX_LAYOUT_MOMENTS.  Lazy: a row is touched when its index occurs in the batch, whatever
     its x (x = 0 included); untouched rows keep their bits.  The bias is one more coordinate, touched by every step. */
  FMX_RULE_ADAGRAD = 3,  /* G += g*g;  p -= lr * g / (sqrt(G) + eps)                    (lr_decay = weight_decay = 0) */
  FMX_RULE_ADAM = 4      /* m += (1-beta1)(g - m);  v += (1-beta2)(g*g - v);
                            p -= step_size * m / (sqrt(v) + eps),  step_size = lr sqrt(1 - beta2^t) / (1 - beta1^t),
                            t = fmx_hyper_t.step + 1 (torch.optim.SparseAdam's order of operations) */
};
/* The adaptive rules are taken by fmx_fm_update, fmx_fm_step, fmx_fm_stream and fmx_fm_online_run on a MOMENTS table.
 * fmx_deepfm_stream, fmx_online_run_mlp (fit mode), fmx_mlp_fit and fmx_owner_step return FMX_ERR_UNSUPPORTED for them.
 * DeepFM / NFM under these rules: fmx_deepfm_stream_opt (tables under any rule, the network under fmx_mlp_opt_t's) and
 * fmx_mlp_section_opt (the network's section alone) at mini-batch sizes; fmx_online_run_mlp_opt (the online predict-then-fit
 * loop) and fmx_mlp_fit_opt (its network step alone) one sample at a time, below.
 * A MOMENTS table is accepted wherever a table is only read (fmx_fm_forward, fmx_fm_forward_partial / _finish, the Hedge
 * mode of fmx_online_run_mlp): the bias weight is bias[0], as in the weights layout. */

/* loss applied to the FM logit z in the fused epilogue of fmx_fm_forward */
enum fmx_loss {
  FMX_LOSS_NONE = 0,
  FMX_LOSS_BCE_LOGITS = 1, /* BCEwl(z, y)            reference fm_adam.py:61,66 */
  FMX_LOSS_BCE_SIGMOID = 2 /* BCEwl(sigmoid(z), y)   reference fm_adam.py:76,80 (the "double sigmoid") */
};

typedef struct fmx_table {
  float *rows;                  /* [n_rows, row_stride] */
  const int64_t *field_offsets; /* [n_fields + 1] prefix sums of the per-field vocabulary sizes */
  float *bias;                  /* WEIGHTS: [1] = bias;  FTRL: [2] = (z, n) of the bias;  MOMENTS: [4] = (b, m_b, v_b, 0) */
  int64_t n_rows;
  int32_t n_fields;
  int32_t k;          /* embedding size */
  int32_t kp;         /* k padded to 4 / 8 / 16 / 32 / 64 */
  int32_t row_stride; /* floats */
  int32_t layout;     /* enum fmx_layout */
  int32_t z_offset;   /* FTRL / MOMENTS: float offset of zV / mV inside the row (multiple of 4, >= kp + 4); WEIGHTS: ignored */
  int64_t max_field_rows; /* largest per-field vocabulary (host copy; bounds the sort's composite keys) */
  /* SORT FIELDS (optional; n_sort_fields = 0: the fields themselves).  The occurrence lists and the update work per "sort
   * field".  An occurrence list packs (index, sample) into 32 bits, so a field of 176,373 rows (18 bits) leaves 14 bits for
   * the sample: 16,384 samples per exact step.  A field may therefore be cut into consecutive PIECES of at most
   * max_sort_field_rows rows, each sorted and updated as a field of its own (a sample appears in the list of the one piece
   * its index falls into): sort_offsets [n_sort_fields + 1] (host-built, device-resident) refines field_offsets,
   * sort_cols [n_sort_fields] names the field every piece belongs to.  The forward pass is unaffected. */
  const int64_t *sort_offsets;
  const int32_t *sort_cols;
  int32_t n_sort_fields;
  int32_t reserved;
  int64_t max_sort_field_rows;
  /* FIELDS AS PIECES OF INDEX COLUMNS (optional; all null / 0: field f holds every index of column f).  For the multi-GPU
   * field-owner mode a "field" of a table is a consecutive row range of one column of idx: field f reads column
   * field_cols[f] and holds its indices [field_base[f], field_base[f] + rows_f) -- a sample whose index lies outside belongs
   * to another piece (another field of this table, or a field of another owner's table) and contributes nothing here.  A
   * field may be EMPTY (0 rows): a hole in the forward tree.  The forward pass adds the fields in position order (lane
   * group f % SLOTS, pass f / SLOTS, SLOTS = 64 / (kp / 4)), so which piece sits at which field number decides the order
   * of the floating-point additions: tables that place the same pieces at the same positions give identical bits however
   * the positions are dealt over owners.  With pieces the kernels cannot tell a bad index from one of another piece:
   * device-side range errors (error word 1) are reported for unmapped tables only.
   * A table that ENDS in an empty field needs ONE READABLE ROW after n_rows (row_stride floats; their values do not matter): the
   * forward passes gather without a branch, and for a sample that has no row in a field they read the field's first row and
   * drop it -- for a trailing empty field that is row n_rows.  fmx.FlatTable allocates the spare row. */
  const int32_t *field_cols; /* [n_fields] or null */
  const int32_t *field_base; /* [n_fields] or null */
  int32_t n_cols;            /* columns of idx / xv; 0: n_fields */
  int32_t reserved2;
} fmx_table_t;

typedef struct fmx_hyper {
  float lr, eps;             /* SIGNADAM / SGD / ADAGRAD / ADAM */
  float alpha, beta, l1, l2; /* FTRL */
  /* APPENDED with the adaptive rules: the struct grew from 24 to 40 bytes.  The library reads them for FMX_RULE_ADAM only, so a
     caller compiled against the six-float struct keeps working with every other rule; FMX_RULE_ADAM needs the 40-byte form. */
  float beta1, beta2;        /* ADAM */
  int32_t step;              /* ADAM: steps this table has already taken; the call's first step is t = step + 1.
                                fmx_fm_stream: step s of the call uses t = step + s + 1; fmx_fm_online_run: sample i uses
                                t = step + i + 1.  The library never writes it back: the caller advances its count. */
  int32_t reserved;
} fmx_hyper_t;

/* Outputs of the forward pass.  Any pointer may be null except S when an update follows. */
typedef struct fmx_fwd_out {
  float *S;       /* [B, kp]  S_b = sum_f V[row_bf] * x_bf            (kept for the update)        */
  float *bi;      /* [B, kp]  0.5 * (S*S - sum_f e*e)                  reference second_order()     */
  float *first;   /* [B, F]   w[row_bf] * x_bf                         reference first_order()      */
  float *sfirst;  /* [B]      sum_f first                                                             */
  float *sbi;     /* [B]      sum_d bi                                                                */
  float *logit;   /* [B]      sfirst + sbi + bias                      reference forward_fm()       */
  float *loss;    /* [B]      per-sample loss (unscaled), needs y                                     */
  float *dz;      /* [B]      d(mean loss)/d logit = (...) * inv_b, needs y                           */
  int32_t *error; /* [1]      set to 1 when an index is outside its field (that row is treated as 0)  */
  int32_t sample_ld; /* 0: S, loss, dz are dense arrays as above.  > 0 (multiple of 4, >= kp): element b of S, of loss and
                        of dz lies sample_ld floats after element b-1 -- the three pointers then address fields of one
                        per-sample record, which a data-parallel caller all-gathers with ONE collective */
  int32_t reserved;
} fmx_fwd_out_t;

int fmx_version(void);
const char *fmx_last_error_string(void);

/* Process-wide tuning switches (mutable global state: see Conventions); returns the previous value (>= 0) or a negative
 * status for an unknown name.  Every switch changes HOW the same result is computed; results are identical bits.
 *   "inline_fixup" (default 1)  1: runs that cross 64-occurrence tiles are finished inside k_fm_update by an in-launch
 *                                hand-off; 0: by a second launch (k_fm_fixup).
 *   "upd_order"    (default 1)  the order in which k_fm_update's grid takes the table's sort fields (fmx_update_order below).
 *                                0: index order; 1: ascending row count, so that the small fields' tiles -- chains of dependent
 *                                round trips: list, sums, hand-off flags, records, one row -- enter the memory system ahead of
 *                                the large fields' burst of row lines; 2: descending, the adversarial order (large fields first,
 *                                every closing tile as late as possible), for tests.  The order of dispatch is not visible in any
 *                                result.  The library learns a table's row counts with one blocking copy of its offsets at the
 *                                table's first update (never while the stream is capturing) and keeps them per device, keyed by
 *                                (offsets pointer, sort fields, n_rows, largest sort field); a stale or missing entry, or a table
 *                                of more than 128 sort fields, gives index order or another order of the same tiles: it can cost
 *                                time, never correctness.
 *   "sort_ahead"   (default 16) most batches sorted per side-stream launch in fmx_fm_stream / fmx_deepfm_stream (1..16).
 *   "sort_resident" (default -1) most workgroups of a side-stream group sort of fmx_fm_stream / fmx_deepfm_stream, from a call's
 *                                third group on (they run beside a whole group of steps; their lists are needed a group later): min(batches x sort fields, value)
 *                                workgroups, rounded up to a multiple of 8, at most one per CU, each walking several (batch, sort
 *                                field) units -- the step's own kernels keep their wave slots on every CU beside the sort.  0: one
 *                                workgroup per unit, as the call's first two groups and every other sort are launched; -1 (any
 *                                negative value): the library's default for the device, half of its CUs.  This is the one
 *                                option whose previous value can be negative: -1 returned under this name is the default, not
 *                                a status.  Also FMX_SORT_RESIDENT in the environment.
 *   "sort_chunked" (default 1)  0: one workgroup per field at every width; 1: k_sort_chunk + k_sort_merge (1,024-composite
 *                                chunks spread over the chip, stable rank merge) from 8,192 composites per field on; 2: from 2,048 on.
 *   "mlp_chain"    (default 1)  0: fmx_mlp_section as separate GEMM launches instead of k_mlp_chain (forward + loss + dgrad chain
 *                                in one launch); same results up to summation order.
 *   "online_persistent" (default 1)  0: fmx_online_run_mlp as per-sample launches instead of one workgroup walking the stream. */
int fmx_set_option(const char *name, int value);

/* The order option "upd_order" = mode gives n sort fields of rows[i] rows each (host memory; nothing is launched): order[i] is
 * the field the grid takes i-th.  A permutation of 0..n-1 in ascending (1) or descending (2) row count, fields of equal count
 * in index order (empty fields count 0 rows: first when ascending); mode 0: 0..n-1.  Returns n, or 0 with nothing written for
 * n > 128: the launch carries one byte per field by value, and such a table is updated in index order.  Negative: bad argument. */
int fmx_update_order(const int64_t *rows, int32_t n, int32_t mode, uint8_t *order);

/* Smallest sort width for a batch: max(64, next power of two >= B); and log2 of it. */
int fmx_sorted_width(int B);
int fmx_sorted_bbits(int B);

/* Bytes of caller-owned device workspace a step of batch size B needs (16-byte aligned).  Layout:
 *   (F below: the number of SORT fields of the table, = n_fields unless large fields are split)
 *   sorted  uint32 [32][F, Bp]       occurrence lists: (local index << bbits) | sample, padded with 0xFFFFFFFF
 *                                    (a ring of 32: fmx_fm_stream sorts up to 16 batches ahead; single steps use the first)
 *   runs    uint32 [16][F, Bp]       Bp >= 2048 only: the chunk-sorted intermediate of the wide sort
 *   meta    int32  [F, Bp/64, 2]     per 64-entry tile: does a run come in from / go out to the neighbouring tile; with the
 *                                    in-launch hand-off word 0 is (launch sequence << 4 | states) and is polled by later tiles
 *   parts   float  [F, Bp/64, 2, 2*kp+4]  partial sums of the runs that cross a tile boundary
 * Every entry point that takes a workspace also takes its size in bytes and returns FMX_ERR_SHAPE when that is less than
 * fmx_workspace_bytes(table, B) NOW: the size depends on the table's sort fields, and a table whose fields were split for a
 * larger batch needs a larger workspace at every batch size.
 * The workspace must be ZERO-FILLED once before its first use (the hand-off's flag words are compared with a
 * non-zero launch sequence number; never-written words must not match one by accident).
 * Negative on a bad table. */
int64_t fmx_workspace_bytes(const fmx_table_t *table, int32_t B);

/* Gather + bi-interaction forward.
 * Replaces: first_order / second_order / forward_fm (reference deepfm_adam.py:46-77, fm_adam.py:35-53),
 * i.e. 2 x 39 nn.Embedding gathers, the two 39-term Python sums and the bi-interaction, plus (loss_kind != NONE)
 * the BCE-with-logits loss and its derivative (fm_adam.py:61,66 / :76,80).
 *   idx  [B, F] int32, per-field LOCAL indices exactly as the reference passes them (bit-exact; range-checked)
 *   xv   [B, F] fp32 feature values or null (== 1.0, the Criteo case)
 *   y    [B] fp32 labels or null (required when loss_kind != FMX_LOSS_NONE)
 *   inv_b  1 / (global batch size) folded into dz
 */
int fmx_fm_forward(const fmx_table_t *table, const fmx_hyper_t *hyper, const int32_t *idx, const float *xv,
                   const float *y, int32_t B, int32_t loss_kind, float inv_b, const fmx_fwd_out_t *out,
                   fmx_stream_t stream);

/* ---- the forward pass split over field owners (the model-parallel multi-GPU mode; fmx/owner.py, fmx/plan.py) ----
 * fmx_fm_forward sums a sample's rows in a fixed tree: lane group `slot` of SLOTS = 64 / (kp / 4) adds the fields slot,
 * SLOTS + slot, ... in order, then a butterfly over the lane groups.  The tree is cut into n_blocks BLOCKS of SL = SLOTS /
 * n_blocks consecutive lane groups (n_blocks a power of two <= SLOTS); an owner holds n_local_blocks of them as a table of its
 * own: with NP = n_fields / (n_local_blocks SL) passes, local field (lb NP + p) SL + s sits at position p SLOTS + (first + lb) SL + s
 * of the whole tree (fields are pieces of index columns: fmx_table_t.field_cols / field_base; empty fields fill the holes).
 * fmx_fm_forward_partial evaluates those sub-trees for every sample of the GLOBAL batch: parts_out [B / group][n_local_blocks][group,
 * 2 kp + 4] = per block and sample (S_part[kp], sum e*e part[kp], first-order part, 0, 0, 0); group (0: B) = the samples one rank
 * holds the labels of: their records lie together, block after block -- one contiguous message per destination.  The records of a sample meet on the rank
 * that holds its label; fmx_fm_forward_finish adds the n_blocks records in the order of the remaining butterfly levels --
 * block pairs, pairs of pairs, ... -- and applies fmx_fm_forward's epilogue (bias, loss, dlogit).  The outputs are
 * bit-identical to fmx_fm_forward on one device whose table has the same fields at the same positions.
 *   idx [B, n_cols] int32 (all columns; the owner's fields pick theirs), xv likewise or null; error as in fmx_fwd_out_t
 *   parts [n_blocks][B, 2 kp + 4], block r's records owner_stride floats after block r-1's; bias [1] or [2] as in fmx_table_t
 * Replaces: the same reference sites as fmx_fm_forward (deepfm_adam.py:46-77, fm_adam.py:35-53, :61,66 / :76,80). */
int fmx_fm_forward_partial(const fmx_table_t *table, const int32_t *idx, const float *xv, int32_t B, int32_t n_blocks,
                           int32_t n_local_blocks, int32_t group, float *parts_out, int32_t *error, fmx_stream_t stream);
int fmx_fm_forward_finish(const fmx_hyper_t *hyper, const float *bias, int32_t layout, int32_t kp, const float *parts,
                          int64_t owner_stride, int32_t n_owners, const float *y, int32_t B, int32_t loss_kind, float inv_b,
                          const fmx_fwd_out_t *out, fmx_stream_t stream);

/* ---- the field-owner step as ONE call per step, with the library's own RCCL communicator (one process per GPU) ----
 * What fmx/owner.py's FieldOwnerFM does with torch.distributed collectives between three ctypes calls -- 70 us of host time per
 * step -- as two entry points: fmx_owner_prefetch (weights-free, ahead of time, on the communicator's own stream: all-gather of
 * the ranks' index batches, occurrence sort of the owned pieces over the global batch) and fmx_owner_step (partial forward ->
 * all-to-all of the per-block records -> finish -> all-gather of (S, dlogit, loss) -> update of the owned rows), every launch
 * and both exchanges issued from C on `stream`.  RCCL is loaded at run time (librccl.so.1); with one rank nothing is exchanged
 * (flags bit 0 forces the calls: the RCCL path on a one-GPU box) and RCCL is not needed.
 *   fmx_comm_unique_id   rank 0 fills 2 x FMX_COMM_ID_BYTES bytes (two ncclUniqueId: the step's communicator and the prefetch
 *                        stream's -- operations of ONE RCCL communicator are serialised in issue order whatever their stream);
 *                        the host side broadcasts them (torch.distributed) and every rank calls fmx_comm_create
 *   block_count [world]  tree blocks per rank (fmx.plan.OwnerPlan.block_count; null: one each)
 * A slot (0 .. FMX_COMM_SLOTS-1) names one batch in flight: fmx_owner_prefetch(slot) orders itself behind `stream` as it is at
 * the call and behind the last fmx_owner_step that used the slot; fmx_owner_step(slot) waits for that prefetch.  The caller owns
 * every buffer: idx_all [world B, n_cols] and the workspace of the slot, parts_send [world][blocks of this rank][B, 2 kp + 4],
 * parts_recv [n_blocks][B, 2 kp + 4], rec_local [B, kp + 4], rec_all [world B, kp + 4] (with one rank and no forced collectives
 * parts_recv may be parts_send and rec_all rec_local, and nothing is copied: fmx_owner_prefetch sorts from idx_local, idx_all may be
 * null there, and the caller hands the same idx_local to fmx_owner_step as idx_all).  Same results, bit for bit, as the separate calls.
 * Replaces: reference fm_adam.py:56-69 (update_embedding: forward_fm, loss, backward, optimizer) on a batch sharded over ranks. */
#define FMX_COMM_ID_BYTES 128
#define FMX_COMM_MAX_WORLD 16
typedef struct fmx_comm fmx_comm_t;
typedef struct fmx_owner_bufs {
  float *parts_send, *parts_recv, *rec_local, *rec_all;
} fmx_owner_bufs_t;
int fmx_comm_unique_id(void *ids_out);
int fmx_comm_create(const void *ids, int32_t rank, int32_t world, const int32_t *block_count, int32_t flags, fmx_comm_t **out);
int fmx_comm_destroy(fmx_comm_t *comm);
int fmx_owner_prefetch(fmx_comm_t *comm, const fmx_table_t *table, const int32_t *idx_local, int32_t B, int32_t slot, int32_t *idx_all,
                       void *workspace, int64_t workspace_bytes, int32_t *error, fmx_stream_t stream);
int fmx_owner_step(fmx_comm_t *comm, const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, int32_t loss_kind,
                   const int32_t *idx_all, const float *y_local, int32_t B, int32_t slot, void *workspace, int64_t workspace_bytes,
                   const fmx_owner_bufs_t *bufs, float *loss_out, int32_t *error, fmx_stream_t stream);

/* Occurrence lists: for every field, the batch's (local index, sample) pairs sorted by index then sample.
 * Replaces: the duplicate-row summation embedding_dense_backward performs inside loss.backward()
 * (reference fm_adam.py:67,81) -- sorting is what makes "reduce per unique row, then
 * update once" deterministic.
 *   workspace: fmx_workspace_bytes(table, B) bytes; the lists land at its start as uint32 [F, Bp],
 *   entry = (local index << bbits) | sample, padded with 0xFFFFFFFF;
 *   Bp = fmx_sorted_width(B), bbits = fmx_sorted_bbits(B); requires (largest sort field - 1) < (0xFFFFFFFF >> bbits)
 *   and Bp <= 32768 (a field's composites are merged in one workgroup's LDS).
 */
int fmx_sort_occurrences(const fmx_table_t *table, const int32_t *idx, int32_t B, void *workspace, int64_t workspace_bytes, int32_t *error,
                         fmx_stream_t stream);

/* Row-reduced backward + fused per-row update.
 * Replaces: loss.backward() into 78 dense table gradients + optimizer.step() over all parameters
 * (reference fm_adam.py:67-68 / :81-82).  For every unique row of the batch:
 *     G[b,d]  = dz_bi[b] + gbi[b,d]                       (either term may be absent)
 *     dV[row] = sum_b x (S_b - x V_row) * G[b,:]          dw[row] = sum_b x dz_first[b]
 * summed in sample order, then ONE application of `rule` per coordinate.  The bias gets sum_b dz_first[b].
 *   workspace the one fmx_sort_occurrences filled for the same idx
 *   S         [B, kp] from fmx_fm_forward
 *   dz_first  [B] coefficient of the first-order weights and the bias
 *   dz_bi     [B] or null: scalar coefficient on every bi component (the FM term sum_d bi_d)
 *   gbi       [B, kp] or null: dL/dbi from a network on top of bi (DeepFM / NFM)
 *   loss_b    [B] or null with loss_out [1] or null: loss_out = inv_b * sum_b loss_b (deterministic order)
 *   sample_ld 0, or the record stride of fmx_fwd_out_t.sample_ld: applies to S, dz_first, dz_bi, loss_b and gbi (fields of one
 *             per-sample record, which a data-parallel caller all-gathers with ONE collective)
 */
int fmx_fm_update(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, void *workspace, int64_t workspace_bytes,
                  const float *xv, const float *S, const float *dz_first, const float *dz_bi, const float *gbi,
                  int32_t B, int32_t sample_ld, const float *loss_b, float inv_b, float *loss_out, fmx_stream_t stream);

/* The same row-reduced update from EXPLICIT per-occurrence gradients (a model whose embedding gradient is not of the form
 * x (S_b - x V) G_b: the attentional FM below).  For every unique row of the batch
 *     dV[row] = sum_b E[b, f]          dw[row] = sum_b x dz_first[b]
 * summed in sample order, then ONE application of `rule` per coordinate; the bias gets sum_b dz_first[b].  Same sort, runs,
 * hand-offs and rule arithmetic as fmx_fm_update (whose dV is the cV - V cA of its runs; here cV = sum E and cA = 0).
 *   workspace  the one fmx_sort_occurrences filled for the same idx (split large fields are honoured: a piece's occurrences read
 *              the slot of the field it belongs to)
 *   xv         [B, F] or null (== 1): the first-order weights' x
 *   occ_grad   [B, ld_occ]: E[b, f] = dL/dV_row of sample b's row of field f (x applied), kp floats at b * ld_occ + f * kp;
 *              ld_occ a multiple of 4, >= n_fields * kp; 16-byte aligned
 *   loss_b, inv_b, loss_out  as fmx_fm_update
 * Tables whose fields are pieces of index columns (field_cols / field_base) return FMX_ERR_UNSUPPORTED.
 * Replaces: the embedding part of loss.backward() + optimizer.step() of AFMAdam.fit (reference afm_adam.py:113-118). */
int fmx_fm_update_occ(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, void *workspace, int64_t workspace_bytes,
                      const float *xv, const float *dz_first, const float *occ_grad, int32_t ld_occ, int32_t B, const float *loss_b,
                      float inv_b, float *loss_out, fmx_stream_t stream);

/* One pure-FM mini-batch step = sort + forward(+loss) + update on one stream.
 * Replaces: FMAdam.update_embedding / FMAdam.fit (reference fm_adam.py:56-82) and every class's
 * update_embedding (deepfm_adam.py:91-104 etc.), which all train on forward_fm only.
 * workspace: fmx_workspace_bytes(table, B) bytes; fwd->S, fwd->loss, fwd->dz must be non-null. */
int fmx_fm_step(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, int32_t loss_kind,
                const int32_t *idx, const float *xv, const float *y, int32_t B, float inv_b, void *workspace, int64_t workspace_bytes,
                const fmx_fwd_out_t *fwd, float *loss_out, fmx_stream_t stream);

/* The online loop over a device-resident stream of mini-batches: step s uses batch (s mod n_pool).
 * Replaces: the driver loops reference main_experiment.py:92-105 (pre-training) and fm_adam.py:97-99
 * (run_experiment), batched.  idx_pool [n_pool, B, F], y_pool [n_pool, B]; loss_out [n_steps] or null.
 * kernel_ms (HOST pointer, [4]) or null: the measuring mode.  Everything runs on `stream` in groups of up to 8 steps: ONE
 * sort launch for the group's batches (as in production), the group's forwards back to back, then its updates back to
 * back, each block between two HIP events, every launch on a different batch of the pool (own sorted list, own
 * S / dz / loss in a temporary buffer) so that rows come from HBM / MALL as in production.  The forwards of a group all
 * read the table before the group's updates: the table is NOT the production run's.  After a stream synchronise
 * kernel_ms[0..2] = n_steps x the average per-launch milliseconds of {sort (up to 8 batches per launch), forward,
 * update (both launches of it when inline_fixup = 0)}, each with the cost of an empty event pair -- [3], same scaling --
 * subtracted. */
int fmx_fm_stream(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, int32_t loss_kind,
                  const int32_t *idx_pool, const float *y_pool, int32_t n_pool, int32_t B, float inv_b,
                  int32_t n_steps, void *workspace, int64_t workspace_bytes, const fmx_fwd_out_t *fwd, float *loss_out, float *kernel_ms,
                  fmx_stream_t stream);

/* The reference's online protocol for the pure-FM class on a device-resident stream of N samples: for every sample,
 * predict (pred_out[i] = sigmoid(logit) > 0.5 with the weights BEFORE the sample's update), then one fit step on that
 * sample alone (B = 1, inv_b = 1) under `rule` and `loss_kind`.  One wavefront walks the stream (the steps are sequential by
 * definition); the table and bias end bit-identical to N calls of fmx_fm_step with B = 1.  loss_out [N] may be null.
 * Needs n_fields <= 4 * (64 / (kp / 4)) (64 fields at kp = 16), else FMX_ERR_UNSUPPORTED.
 * Replaces: FMAdam.run_experiment's loop body (reference fm_adam.py:97-99: predict at :84-88, fit at :71-82). */
int fmx_fm_online_run(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, int32_t loss_kind,
                      const int32_t *idx, const float *xv, const float *y, int32_t N, uint8_t *pred_out, float *loss_out,
                      int32_t *error, fmx_stream_t stream);

/* ---- pairwise-ranking (BPR) training of the pure FM ----
 * A batch of B_pairs pairs is idx [2 B_pairs, F] (and xv [2 B_pairs, F] or null) in fmx_fm_forward's layout: row 2i is the
 * positive sample of pair i, row 2i + 1 the negative (typically the positive's row with the item columns replaced; nothing
 * requires that).  With d_i = z[2i] - z[2i + 1]: loss_i = -log(sigmoid(d_i) + margin), margin >= 0 and finite (0: BPR, in the
 * stable softplus form; the reference uses 0.1), g_i = d loss_i / d d_i = -sigmoid(d_i) sigmoid(-d_i) / (sigmoid(d_i) + margin).
 * Shared refusals: a null table / hyper / idx, a count < 1 and a bad margin are FMX_ERR_ARG; tables whose fields are pieces of
 * index columns (field_cols / field_base) FMX_ERR_UNSUPPORTED.  No labels are read.
 * Restates: the pair objective of reference models/models_meta_emb/meta_fm.py:145-169 for the FM logit. */

/* The forward pass of the 2 B_pairs rows with the pair epilogue: out->S / bi / first / sfirst / sbi / logit exactly as
 * fmx_fm_forward(FMX_LOSS_NONE) writes them for the same rows (bit-identical), and, where asked for,
 *   out->dz[2i] = g_i * inv_b, out->dz[2i + 1] = -out->dz[2i] (the same float negated: the two sum to exactly 0),
 *   out->loss[2i] = loss_i, out->loss[2i + 1] = 0.
 * With these fmx_fm_update(B = 2 B_pairs, dz_first = dz_bi = dz, loss_b = loss) is the exact step of inv_b * sum_i loss_i.
 * (reference meta_fm.py:145-169: out_pos, out_neg, -log(sigmoid(out_pos - out_neg) + margin).) */
int fmx_fm_pair_forward(const fmx_table_t *table, const fmx_hyper_t *hyper, const int32_t *idx, const float *xv, int32_t B_pairs,
                        float margin, float inv_b, const fmx_fwd_out_t *out, fmx_stream_t stream);

/* One pair step = fmx_sort_occurrences(2 B_pairs) + fmx_fm_pair_forward + fmx_fm_update(2 B_pairs) on one stream, under any rule
 * the table's layout takes; loss_out[0] = inv_b * sum_i loss_i.  workspace: fmx_workspace_bytes(table, 2 * B_pairs) bytes
 * (smaller: FMX_ERR_SHAPE); fwd->S, fwd->loss, fwd->dz must be non-null, sized for 2 B_pairs samples; 2 * B_pairs beyond the
 * sort's width is refused as fmx_sort_occurrences refuses it.
 * Replaces: the loss.backward() + optimizer.step() of the reference's pair objective (meta_fm.py:145-169). */
int fmx_fm_pair_step(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx, const float *xv,
                     int32_t B_pairs, float margin, float inv_b, void *workspace, int64_t workspace_bytes, const fmx_fwd_out_t *fwd,
                     float *loss_out, fmx_stream_t stream);

/* n_steps pair steps over a device-resident pool idx_pool [n_pool, 2 B_pairs, F] (every feature value 1): step s takes batch
 * (s mod n_pool) and, under FMX_RULE_ADAM, is step hyper->step + s + 1 of the table; loss_out [n_steps] or null.  The table ends
 * bit-identical to n_steps calls of fmx_fm_pair_step.  (The pair objective of reference meta_fm.py:145-169, batched as
 * fmx_fm_stream batches the pointwise one.) */
int fmx_fm_pair_stream(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx_pool, int32_t n_pool,
                       int32_t B_pairs, float margin, float inv_b, int32_t n_steps, void *workspace, int64_t workspace_bytes,
                       const fmx_fwd_out_t *fwd, float *loss_out, fmx_stream_t stream);

/* The online predict-then-fit protocol restated for pairs, on N device-resident pairs idx [2N, F]: for every pair,
 * pred_out[i] = z_pos > z_neg, logit_out[2i], logit_out[2i + 1] (or null) and loss_out[i] (or null) with the weights BEFORE the
 * pair's update, then one pair step on that pair alone (B_pairs = 1, inv_b = 1).  One wavefront walks the stream; the table and
 * bias end bit-identical to N calls of fmx_fm_pair_step with B_pairs = 1.  Under FMX_RULE_ADAM pair i is step
 * hyper->step + i + 1.  Needs n_fields <= 4 * (64 / (kp / 4)) as fmx_fm_online_run does (both samples' rows fit the wavefront's
 * registers), else FMX_ERR_UNSUPPORTED.  An out-of-range index sets *error to 1.
 * (The pair objective of reference meta_fm.py:145-169 under the protocol of fm_adam.py:90-119.) */
int fmx_fm_pair_online_run(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx, const float *xv,
                           int32_t N, float margin, uint8_t *pred_out, float *logit_out, float *loss_out, int32_t *error,
                           fmx_stream_t stream);

/* ---- listwise (sampled-softmax) training of the pure FM: one positive, G - 1 negatives ----
 * A batch of B_lists lists of G rows (2 <= G <= 16) is idx [B_lists G, F] (and xv of the same shape, or null) in fmx_fm_forward's
 * layout: row G i is the positive sample of list i, rows G i + 1 .. G i + G - 1 its negatives (typically the positive's row with
 * the item columns replaced; nothing requires that).  With z_j the FM logit of row G i + j, per list:
 *     m = max_j z_j,   e_j = exp(z_j - m),   s = e_0 + e_1 + ... + e_{G-1}  (added in that order),
 *     loss_i = log(s) - (z_0 - m)                                  softmax cross-entropy against position 0
 *     dz_j   = (e_j / s) inv_b                          for j >= 1
 *     dz_0   = -((e_1 + ... + e_{G-1}) / s) inv_b       the negatives' mass itself, not 1 - p_0, which loses its digits as p_0 -> 1
 * loss and dz are finite for every finite set of logits (the max is subtracted: exp's argument is <= 0 and s >= 1); every lane
 * of a list evaluates the same operands in the same order, so a list's result depends on its logits and G alone, never on its
 * place in the batch or the launch's geometry.  At G = 2 this is BPR (fmx_fm_pair_forward under margin 0) in other arithmetic.  No
 * labels are read; there is no temperature.  The log-Q correction for negatives that were not drawn uniformly: fmx_fm_list_*_q below.
 * The bias: a softmax does not move under a shift of all its logits, so the bias has no gradient, and the contract is the pair
 * family's -- a list step leaves the bias and its state (z / n, moments) BIT-UNCHANGED under every rule.  The dz of a list sum to
 * zero only up to rounding, so the step does not rely on the sum: the update's bias rule runs on 16 scratch bytes behind the
 * ordinary step workspace (fmx_fm_list_workspace_bytes), the forward reads the real bias.
 * The first-order weights of the columns every row of a list shares (the context) also have a gradient that is zero in exact
 * arithmetic; nothing shields them: they receive rounding-level gradients, which FMX_RULE_SIGNADAM normalises like any other
 * (g / (|g| + eps)), so under that rule they do move.
 * Shared refusals, each decided on the host before any launch and naming the entry point: a null table / hyper / idx,
 * B_lists < 1, G < 2, B_lists G beyond int32: FMX_ERR_ARG; G > 16 (a list's waves share one workgroup of at most 1024 threads):
 * FMX_ERR_UNSUPPORTED; tables whose fields are pieces of index columns (field_cols / field_base): FMX_ERR_UNSUPPORTED.
 * Replaces: nothing -- the reference has no listwise loss.  Its nearest counterpart is the pair objective of reference
 * models/models_meta_emb/meta_fm.py:145-169, which this generalises from one negative to G - 1. */

/* Bytes of caller-owned device workspace a list step of B_lists lists of G rows needs: fmx_workspace_bytes(table, B_lists G) plus
 * the 16 scratch bytes the bias rule runs on (at the end; 16-byte aligned).  Zero-fill once before the first use, as
 * fmx_workspace_bytes' buffer.  Negative on a bad table, B_lists < 1, G outside [2, 16] or B_lists G beyond int32.
 * Replaces: nothing in the reference (the pair objective of meta_fm.py:145-169 is its nearest counterpart; it has no listwise loss). */
int64_t fmx_fm_list_workspace_bytes(const fmx_table_t *table, int32_t B_lists, int32_t G);

/* The forward pass of the B_lists G rows with the list epilogue: out->S / bi / first / sfirst / sbi / logit exactly as
 * fmx_fm_forward(FMX_LOSS_NONE) writes them for the same rows (bit-identical), and, where asked for,
 *   out->loss[G i] = loss_i (unscaled), out->loss[G i + j] = 0 for j >= 1;   out->dz[G i + j] = dz_j as above.
 * G max(1, 4 / G) waves per workgroup (one row per wave): a workgroup holds whole lists.
 * Replaces: nothing in the reference, which has no listwise loss; nearest: the forward and loss of the pair objective
 * (meta_fm.py:145-169: out_pos, out_neg, -log(sigmoid(out_pos - out_neg) + margin)). */
int fmx_fm_list_forward(const fmx_table_t *table, const fmx_hyper_t *hyper, const int32_t *idx, const float *xv, int32_t B_lists,
                        int32_t G, float inv_b, const fmx_fwd_out_t *out, fmx_stream_t stream);

/* One list step = fmx_sort_occurrences(B_lists G) + fmx_fm_list_forward + fmx_fm_update(B_lists G, dz_first = dz_bi = dz) on one
 * stream, under any rule the table's layout takes: the step of inv_b sum_i loss_i; loss_out[0] = inv_b sum_i loss_i.  The table's
 * bias and its state are bit-unchanged (above).  workspace: fmx_fm_list_workspace_bytes(table, B_lists, G) bytes (null:
 * FMX_ERR_ARG, smaller: FMX_ERR_SHAPE); fwd->S, fwd->loss, fwd->dz must be non-null, sized for B_lists G samples; the rule against
 * the layout and FMX_RULE_ADAM's hyper-parameters are checked as fmx_fm_pair_step checks them; B_lists G beyond the sort's width is
 * refused as fmx_sort_occurrences refuses it.
 * Replaces: nothing in the reference, which has no listwise loss; nearest: the loss.backward() + optimizer.step() of the pair
 * objective (meta_fm.py:145-169). */
int fmx_fm_list_step(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx, const float *xv,
                     int32_t B_lists, int32_t G, float inv_b, void *workspace, int64_t workspace_bytes, const fmx_fwd_out_t *fwd,
                     float *loss_out, fmx_stream_t stream);

/* n_steps list steps over a device-resident pool idx_pool [n_pool, B_lists G, F] (every feature value 1): step s takes batch
 * (s mod n_pool) and, under FMX_RULE_ADAM, is step hyper->step + s + 1 of the table; loss_out [n_steps] or null.  The table ends
 * bit-identical to n_steps calls of fmx_fm_list_step.  n_pool < 1 and n_steps < 0 are FMX_ERR_ARG.
 * Replaces: nothing in the reference, which has no listwise loss; nearest: the pair objective of meta_fm.py:145-169, batched as
 * fmx_fm_stream batches the pointwise one. */
int fmx_fm_list_stream(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx_pool, int32_t n_pool,
                       int32_t B_lists, int32_t G, float inv_b, int32_t n_steps, void *workspace, int64_t workspace_bytes,
                       const fmx_fwd_out_t *fwd, float *loss_out, fmx_stream_t stream);

/* ---- the log-Q corrected list loss: sampled softmax under negatives that were not drawn uniformly ----
 * fmx_fm_list_forward / _step / _stream with one more array: corr [B_lists G] fp32 (the stream: corr_pool [n_pool, B_lists G], step
 * s reading the rows of batch s mod n_pool), one value per row, typically log Q(item of the row) of the sampler that drew the
 * negatives (fmx_alias_sample_negatives' neg_logq; the positive's item included).  With
 *     c_j = z_j - corr[G i + j]                    one fp32 subtraction per row
 * the loss and dz are the list family's formulas above with c in the place of z: m = max_j c_j, e_j = exp(c_j - m),
 * s = e_0 + ... + e_{G-1} added in that order, loss_i = log(s) - (c_0 - m), dz_j = (e_j / s) inv_b, dz_0 = minus the negatives'
 * mass times inv_b.  Without the correction an item is pushed down merely for being drawn often (Bengio & Senecal 2008; Yi et al.
 * 2019).  out->logit, S, bi, first, sfirst and sbi stay those of the UNCORRECTED forward, bit for bit: the logit is the serving score.
 * corr must be finite (the caller's contract; nothing checks it on the device).  A null corr / corr_pool is FMX_ERR_ARG.  Every other
 * refusal, the workspace (fmx_fm_list_workspace_bytes), the scratch the bias rule runs on and the bit-unchanged bias are the list
 * family's: the same host code.  With corr all +0 every output and the table are bit-identical to the uncorrected call (z - 0 is z).
 * The correction rides where the pointwise objective's label rides (one 4-byte load per row in the forward); nothing else of the
 * step changes.  fmx_fm_list_online_run has no corrected form.
 * Replaces: torch.log_softmax(z - log_q) on assembled rows and autograd through it; nothing in the reference, which has no listwise
 * loss and takes its negatives as given (meta_fm.py:145-169). */
int fmx_fm_list_forward_q(const fmx_table_t *table, const fmx_hyper_t *hyper, const int32_t *idx, const float *xv, const float *corr,
                          int32_t B_lists, int32_t G, float inv_b, const fmx_fwd_out_t *out, fmx_stream_t stream);
int fmx_fm_list_step_q(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx, const float *xv,
                       const float *corr, int32_t B_lists, int32_t G, float inv_b, void *workspace, int64_t workspace_bytes,
                       const fmx_fwd_out_t *fwd, float *loss_out, fmx_stream_t stream);
int fmx_fm_list_stream_q(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx_pool,
                         const float *corr_pool, int32_t n_pool, int32_t B_lists, int32_t G, float inv_b, int32_t n_steps,
                         void *workspace, int64_t workspace_bytes, const fmx_fwd_out_t *fwd, float *loss_out, fmx_stream_t stream);

/* The online predict-then-fit protocol restated for lists, on N device-resident lists idx [N G, F] (row G i the positive of list i,
 * as above; xv of the same shape, or null: every value 1).  For every list, with the weights BEFORE the list's update:
 *   rank_out[i]  (required) = the number of negatives of list i whose logit is >= the positive's -- 0: the positive is first; at
 *                G = 2, rank_out[i] == 0 is fmx_fm_pair_online_run's pred_out[i];
 *   logit_out[G i + j] (or null) = z_j;   loss_out[i] (or null) = loss_i, the bits of fmx_fm_list_step's loss_out[0] at B_lists = 1;
 * then one list step on that list alone.  One workgroup of G waves walks the stream (wave j holds row j of the list, as
 * fmx_fm_online_run's wavefront holds a sample).  The table ends bit-identical to N calls of fmx_fm_list_step with B_lists = 1,
 * inv_b = 1: the terms of a row several members of a list name are added in the order the table update adds them on the sorted
 * list of that step.  Under FMX_RULE_ADAM list i is step hyper->step + i + 1.
 * The bias is read once and never written: it and its state (z / n, moments) stay bit-unchanged, as a list step leaves them.
 * An out-of-range index sets *error to 1 and its occurrence is dropped, as in the step.
 * Refusals, each decided on the host before any launch and naming the entry point: the shared list refusals above with N in the
 * place of B_lists (N < 0: FMX_ERR_ARG), the rule against the layout and FMX_RULE_ADAM's hyper-parameters over N steps as
 * fmx_fm_list_step checks them, rank_out null: FMX_ERR_ARG; n_fields > 4 * (64 / (kp / 4)) (a wave holds its row's table rows in
 * registers, the field limit of fmx_fm_online_run): FMX_ERR_UNSUPPORTED; tables with a sort split (n_sort_fields > 0: the order of
 * the step's additions follows positions counted per piece): FMX_ERR_UNSUPPORTED -- walk such tables with fmx_fm_list_step.
 * N == 0 is FMX_OK, nothing is launched and the buffers may be null.
 * Replaces: nothing -- the reference has no listwise loss; nearest: the pair objective of meta_fm.py:145-169 under the online
 * protocol of fm_adam.py:90-119 (predict a sample, then fit on it). */
int fmx_fm_list_online_run(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx, const float *xv,
                           int32_t N, int32_t G, uint8_t *rank_out, float *logit_out, float *loss_out, int32_t *error,
                           fmx_stream_t stream);

/* ---- in-batch sampled-softmax training of the pure FM: a B x B list loss over the batch's own items ----
 * The list family above pays for every negative as a full table row.  Here the negatives of row i are the ITEMS of the batch's other
 * rows (Yi et al. 2019): a batch of B rows gives B - 1 negatives per positive and touches B F table rows, not B G F.
 * THE OBJECTIVE.  Split the F fields into item fields and context fields (the complement; it may be empty).  For the B rows:
 *     S_u[i], a_u[i]   what fmx_fm_forward gives for row i with the item fields masked (index 0, value 0): out->S, out->logit
 *                      (bias included);
 *     S_c[j], a_c[j]   what it gives for row j with the context fields masked: out->S, out->sfirst + out->sbi (one fp32 addition)
 * -- fmx/recommend.py: side_sums(want_bias=True / False) -- and
 *     score(i, j) = (a_u[i] + a_c[j]) + dot,  dot = fma(S_u[i, kp-1], S_c[j, kp-1], ... fma(S_u[i, 1], S_c[j, 1], S_u[i, 0] * S_c[j, 0]))
 * is fmx_fm_topk's score: the training logit IS the serving score, bit for bit (fmx_fm_topk's top_score for the same pair).
 *     key  [B] int32 or null: equal keys mean the same item.  E_i = {i} + {j != i : key[j] != key[i]} is row i's eligible set: a row
 *          that holds row i's own item (an accidental hit) is left out of row i's softmax.  key null: every j is eligible.
 *     corr [B] fp32, finite, or null: c_ij = score(i, j) - corr[j] (one fp32 subtraction; typically log Q(item of row j)).  corr
 *          null: c_ij = score(i, j); with corr all +0 every output is bit-identical to the null-corr call.
 *     m_i = max over E_i of c_ij,   e_ij = exp(c_ij - m_i),   s_i = sum over E_i of e_ij,   n_i = the same sum without j = i
 *     (accumulated on its own in the same order, as the list loss keeps the negatives' mass),
 *     loss_i = log(s_i) - (c_ii - m_i)
 *     g_ij = (e_ij / s_i) inv_b for eligible j != i,    g_ii = -(n_i / s_i) inv_b,    g_ij = 0 for ineligible j
 *     gSu[i, :] = sum_j g_ij S_c[j, :],    gSc[j, :] = sum_i g_ij S_u[i, :],    gac[j] = sum_i g_ij      (fma accumulation from +0)
 * The max is subtracted, so s_i >= 1 and the loss and the gradients are finite for all finite inputs.  There is no temperature.
 * THE ORDER OF EVERY SUM is fixed by B alone: with splits = min(32, ceil(B / 64)) and per = ceil(B / splits), the other side's rows
 * are cut into the ranges [p per, min(B, (p + 1) per)) (empty ranges dropped; fmx_fm_inbatch_splits returns how many remain: one up
 * to B = 64); a range is summed in ascending order from +0 and the ranges' sums are added in range order, m_i being the maximum over
 * all ranges.  No float atomics; two calls on the same inputs give the same bits.
 * THE TABLE GRADIENT per occurrence, with x the occurrence's value and v its table row (x applied, fmx_fm_update_occ's occ_grad):
 *     item field of row j:      E = x * fma(gac[j], S_c[j] - x * v, gSc[j])          (d a_c / d v = x (S_c - x v), d dot / d S_c = gSc)
 *     context field of row i:   E = x * gSu[i]
 * The row sum of g is zero in exact arithmetic and the step DEFINES it as zero: there is no gau term, so the bias and the context
 * fields' first-order weights get a gradient of exactly +0 (the step hands the update the item side's masked values: x = 0 in the
 * context columns), and an item field's first-order weight gets x gac[j].  The bias and its state stay BIT-UNCHANGED under every
 * rule: the update's bias rule runs on the list steps' scratch (16 bytes behind the step workspace), as in fmx_fm_list_step.  A
 * context row is touched (its V is updated) with a +0 first-order gradient; what the rules do with that: sgd, signadam
 * (0 / (0 + eps)), ftrl (z and n unchanged) and adagrad (v += 0, step 0) leave the first-order weight bit-unchanged; adam takes the
 * zero-gradient step of a touched row (m and v decay, the weight moves by lr_t m / (sqrt(v) + eps)).
 * B = 1 is legal: the loss is 0, every gradient is +-0 and the weights are bit-unchanged under sgd / signadam / ftrl.
 * Refusals, each decided on the host before any launch and naming the entry point: a null table / hyper / idx, B < 1, n_item_fields
 * outside [1, F], an item field out of range or repeated: FMX_ERR_ARG; kp not 4 / 8 / 16 / 32 / 64, tables whose fields are pieces of
 * index columns (field_cols / field_base), more than 512 fields: FMX_ERR_UNSUPPORTED; a null workspace FMX_ERR_ARG, one too small
 * FMX_ERR_SHAPE; the rule against the layout and FMX_RULE_ADAM's hyper-parameters as fmx_fm_list_step checks them; B beyond the
 * sort's width as fmx_sort_occurrences refuses it.  FMX_VERSION stays 104: probe for the symbols.
 * Replaces (every entry below): torch.log_softmax(S_u S_c^T + a_u + a_c^T - log_q) against the diagonal plus autograd through it and
 * through the two masked forwards; nothing in the reference, which has no listwise loss (nearest: meta_fm.py:145-169, one negative). */

/* The number of ranges the sums over the other side's rows are cut into (the formula above); negative on B < 1 or a bad kp.
 * Replaces: nothing -- it states the launch geometry of the calls that replace torch.log_softmax(S_u S_c^T + ... - log_q). */
int32_t fmx_fm_inbatch_splits(int32_t B, int32_t kp);

/* Bytes of the lse block the forward and the backward share: m [B], s [B], n [B] at its start (each padded to 256 bytes), the
 * splits' partial results behind them.  16-byte aligned, no initialisation needed.  Negative on B < 1 or a bad kp.
 * Replaces: the saved tensors of autograd's torch.log_softmax(S_u S_c^T + ... - log_q) node. */
int64_t fmx_fm_inbatch_lse_bytes(int32_t B, int32_t kp);

/* loss [B] = loss_i (unscaled) of the objective above from the two sides' sums (Su [B, ld_u], Sc [B, ld_c]: ld multiples of 4, >= kp,
 * 16-byte aligned; au, ac [B]), and (m, s, n) into the lse block for the backward.  inv_b is not read (the loss is unscaled; the
 * argument list is the backward's).  score_out [B, B] or null: score(i, j) at i B + j, uncorrected -- for tests that hold the logits
 * against fmx_fm_topk; the step passes null and no B x B array exists.
 * Replaces: torch.log_softmax(S_u S_c^T + a_u + a_c^T - log_q), masked, against the diagonal. */
int fmx_fm_inbatch_forward(const float *Su, int32_t ld_u, const float *au, const float *Sc, int32_t ld_c, const float *ac, int32_t B,
                           int32_t kp, const float *corr, const int32_t *key, float inv_b, void *lse, int64_t lse_bytes, float *loss,
                           float *score_out, fmx_stream_t stream);

/* gSu [B, kp], gSc [B, kp] (dense, 16-byte aligned) and gac [B] of inv_b sum_i loss_i from the same inputs and the lse block the
 * forward filled; g is recomputed from (m, s, n).  One launch of two roles (a thread per context row: gSu; a thread per item row:
 * gSc, gac) and, from two ranges on, one that adds the ranges' sums.
 * Replaces: autograd through torch.log_softmax(S_u S_c^T + a_u + a_c^T - log_q) to the side sums. */
int fmx_fm_inbatch_backward(const float *Su, int32_t ld_u, const float *au, const float *Sc, int32_t ld_c, const float *ac, int32_t B,
                            int32_t kp, const float *corr, const int32_t *key, float inv_b, void *lse, int64_t lse_bytes, float *gSu,
                            float *gSc, float *gac, fmx_stream_t stream);

/* occ_grad [B, ld_occ] in fmx_fm_update_occ's layout (field f's kp floats at b ld_occ + f kp; ld_occ a multiple of 4, >=
 * n_fields kp) from the side gradients: E as stated above; idx [B, F] and xv [B, F] (or null: 1) are the UNMASKED batch;
 * item_fields [n_item_fields] is a HOST array.  An index outside its field gives +0.
 * Replaces: autograd from the side sums' gradients through the two masked forwards to the embedding rows
 * (torch.log_softmax(S_u S_c^T + ... - log_q).backward()). */
int fmx_fm_inbatch_occ_grad(const fmx_table_t *table, const int32_t *idx, const float *xv, const int32_t *item_fields,
                            int32_t n_item_fields, const float *gSu, const float *gSc, const float *gac, const float *Sc, int32_t ld_c,
                            int32_t B, float *occ_grad, int32_t ld_occ, fmx_stream_t stream);

/* Bytes of caller-owned device workspace an in-batch step of B rows needs: fmx_workspace_bytes(table, B), the 16 scratch bytes of the
 * bias rule, and behind them the step's own buffers -- the masked (idx, xv) copies, both sides' sums, the side gradients, occ_grad
 * [B, F kp] and the lse block (whose partial sums are 2 splits B kp floats: 16 MiB at B = 4,096, kp = 16).  It does not depend on
 * n_item_fields beyond its check.  Zero-fill once before the first use, as fmx_workspace_bytes' buffer.  Negative on a bad argument.
 * Replaces: the temporaries of torch.log_softmax(S_u S_c^T + ... - log_q) and its autograd graph. */
int64_t fmx_fm_inbatch_workspace_bytes(const fmx_table_t *table, int32_t B, int32_t n_item_fields);

/* One in-batch step on one stream (capturable in a graph, like the other one-stream steps): the step of inv_b sum_i loss_i under any
 * rule the table's layout takes; loss_out[0] = inv_b sum_i loss_i (fmx_fm_update_occ's fixed order).  Bit-identical to this sequence
 * of public calls: the masked copies (idx_u, xv_u: item columns 0; idx_c, xv_c: context columns 0), fmx_sort_occurrences(idx),
 * fmx_fm_forward(idx_u, xv_u) -> S_u, a_u = logit, fmx_fm_forward(idx_c, xv_c) -> S_c, a_c = sfirst + sbi, fmx_fm_inbatch_forward,
 * fmx_fm_inbatch_backward, fmx_fm_inbatch_occ_grad(idx, xv), fmx_fm_update_occ(xv = xv_c, dz_first = gac, occ_grad, loss_b = loss)
 * on the table with its bias pointed at scratch.  The step builds the masked copies in the workspace and adds sfirst + sbi inside
 * the scans (the same fp32 addition).  item_fields is a HOST array.  fwd may be null; fwd->error (or null) receives the range-error
 * word of the sort and the forwards, fwd->loss (or null; 16-byte aligned) the per-row losses [B]; nothing else of it is read.
 * Replaces: torch.log_softmax(S_u S_c^T + ... - log_q) on the masked forwards + loss.backward() + optimizer.step(). */
int fmx_fm_inbatch_step(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx, const float *xv,
                        const int32_t *item_fields, int32_t n_item_fields, const float *corr, const int32_t *key, int32_t B, float inv_b,
                        void *workspace, int64_t workspace_bytes, const fmx_fwd_out_t *fwd, float *loss_out, fmx_stream_t stream);

/* n_steps in-batch steps over a device-resident pool idx_pool [n_pool, B, F] (every feature value 1) with corr_pool / key_pool
 * [n_pool, B] or null: step s takes batch (s mod n_pool) and, under FMX_RULE_ADAM, is step hyper->step + s + 1 of the table;
 * loss_out [n_steps] or null.  Bit-identical to n_steps calls of fmx_fm_inbatch_step: the same launches, queued from one call.
 * n_pool < 1 and n_steps < 0 are FMX_ERR_ARG.
 * Replaces: the training loop around torch.log_softmax(S_u S_c^T + ... - log_q) + backward + optimizer.step(). */
int fmx_fm_inbatch_stream(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx_pool,
                          const int32_t *item_fields, int32_t n_item_fields, const float *corr_pool, const int32_t *key_pool,
                          int32_t n_pool, int32_t B, float inv_b, int32_t n_steps, void *workspace, int64_t workspace_bytes,
                          const fmx_fwd_out_t *fwd, float *loss_out, fmx_stream_t stream);

/* ---- a cross-batch item bank for the in-batch loss: the items of earlier batches as further negatives ----
 * (Wang et al. 2021, "Cross-Batch Negative Sampling".)  The item-side sums (S_c, a_c) an in-batch step computes anyway are kept in a
 * device-resident ring of M slots, and every later row takes them as further negatives: one more scan over two small arrays, no
 * table row, no sort entry, no update.  The plain objective above stands as written; this is added to it.
 * THE BANK: caller-owned device memory and two host ints.  state[0] (head) is the next slot to write, in [0, M); state[1] (count)
 * the number of valid slots, in [0, M]; the valid slots are always the prefix [0, count) (the ring fills upwards from slot 0 and
 * is full from the first wrap on); a zeroed state is an empty bank.  The state lives on the device: a step is one-stream, reads
 * nothing back and can be captured in a graph (every replay advances the bank). */
typedef struct fmx_item_bank {
  float *S;          /* [capacity, kp] fp32, dense, 16-byte aligned: the kept items' S_c */
  float *a;          /* [capacity] fp32: the kept items' a_c */
  float *corr;       /* [capacity] fp32 or null: log Q of each kept item */
  int32_t *key;      /* [capacity] int32 or null: item keys, equal keys meaning the same item */
  int32_t *state;    /* device int32 [2]: head, count */
  int32_t capacity;  /* M >= 1, at most FMX_ITEM_BANK_MAX */
  int32_t kp;        /* the padded k, equal to the table's */
} fmx_item_bank_t;
#define FMX_ITEM_BANK_MAX 1048576 /* the largest capacity taken (2^20 slots) */
/* THE LOSS.  Row i's eligible set is E_i of the in-batch section plus Q_i = every slot q < count with key[i] != bank.key[q] (no
 * keys: every q < count).  c_iq = score(i, q) - bank.corr[q] with score(i, q) = (a_u[i] + bank.a[q]) + dot, the same product chain:
 * a banked item scores bit for bit what it scored in the batch it came from when the context side is the same.
 *     m_i = max over E_i and Q_i;   s_i and n_i also sum e_iq = exp(c_iq - m_i) over Q_i (every bank item is a negative: it counts
 *     in n);   loss_i and g_ii = -(n_i / s_i) inv_b keep their form;   g_iq = (e_iq / s_i) inv_b.
 * GRADIENTS.  Bank items take none (stale values, as in the paper):
 *     gSu[i] = sum_j g_ij S_c[j] + sum_q g_iq bank.S[q];   gSc and gac keep their definitions and change only through (m, s, n);
 * there is still no gau term: the bias and its state stay bit-unchanged under every rule.
 * THE ORDER OF EVERY SUM.  The batch's ranges come first, exactly as in the plain calls; the bank's follow: the slots [0, M) are cut
 * into splits_q = min(32, ceil(M / 64)) ranges of per_q = ceil(M / splits_q) slots (empty ranges dropped; fmx_fm_inbatch_bank_splits
 * returns how many remain) -- a function of M alone, not of count: a slot >= count is simply ineligible (and is not read).  Each
 * range ascends from +0 and the ranges are added in order behind the batch's; the maximum is taken over all ranges of both kinds
 * before any exponential.  No float atomics; two runs give the same bits.  With count = 0 every output of a bank call is
 * bit-identical to the plain call's (an empty range gives -inf to the maximum and +0 to a sum).
 * THE PUSH.  After the scans and the backward have read the bank a step writes its own B items to the slots (head + j) mod M,
 * j = 0 .. B - 1: S_c[j], a_c[j] as the scans used it, corr[j], key[j] -- the values of the weights BEFORE the update -- then
 * head <- (head + B) mod M, count <- min(M, count + B).  The push is a launch of its own behind the last reader of the bank.
 * Refusals, each decided on the host before any launch and naming the entry point: a null bank, S, a or state, capacity < 1:
 * FMX_ERR_ARG; bank->kp != the call's kp: FMX_ERR_SHAPE; S not 16-byte aligned: FMX_ERR_ALIGN; the call's corr null while bank->corr
 * is not, or the reverse, and the same for key: FMX_ERR_ARG; capacity > FMX_ITEM_BANK_MAX: FMX_ERR_UNSUPPORTED; in the calls that
 * push (push, step, stream) B > capacity: FMX_ERR_UNSUPPORTED; and whatever the plain call refuses, as it refuses it.
 * Replaces (every entry below): torch.log_softmax(cat([S_u S_c^T, S_u bank.S^T], 1) + a_u + cat([a_c, bank.a])^T - cat([log_q,
 * bank.corr])) against the diagonal, the bank detached, plus autograd through it; nothing in the reference. */

/* The number of ranges the bank's slots are cut into (the formula above); negative on M < 1, M > FMX_ITEM_BANK_MAX or a bad kp.
 * Replaces: nothing -- it states the launch geometry of the calls that replace the torch.log_softmax(cat(...)) above. */
int32_t fmx_fm_inbatch_bank_splits(int32_t M, int32_t kp);

/* Bytes of the lse block of the bank calls: m, s, n [B] at its start as in fmx_fm_inbatch_lse_bytes, the partial results of the
 * batch's and the bank's ranges behind them.  Negative on a bad argument.
 * Replaces: the saved tensors of autograd's torch.log_softmax(cat(...)) node. */
int64_t fmx_fm_inbatch_bank_lse_bytes(int32_t B, int32_t M, int32_t kp);

/* fmx_fm_inbatch_forward with the bank's slots as further negatives: loss [B], (m, s, n) into the lse block.  The bank is read only.
 * score_out [B, B] or null as there; bank_score_out [B, M] or null: the uncorrected score(i, q) at i M + q for q < count, slots
 * >= count left unwritten -- for tests.  B may exceed the capacity here.
 * Replaces: torch.log_softmax(cat([S_u S_c^T, S_u bank.S^T], 1) + ...) against the diagonal, the bank detached. */
int fmx_fm_inbatch_bank_forward(const float *Su, int32_t ld_u, const float *au, const float *Sc, int32_t ld_c, const float *ac,
                                int32_t B, int32_t kp, const float *corr, const int32_t *key, const fmx_item_bank_t *bank, float inv_b,
                                void *lse, int64_t lse_bytes, float *loss, float *score_out, float *bank_score_out,
                                fmx_stream_t stream);

/* fmx_fm_inbatch_backward from the lse block fmx_fm_inbatch_bank_forward filled: gSu with the bank's term, gSc and gac.  The item
 * role runs as in the plain call on the merged (m, s, n); one more launch walks the bank for gSu and one adds the ranges' sums.
 * Replaces: autograd through torch.log_softmax(cat([S_u S_c^T, S_u bank.S^T], 1) + ...) to the side sums, the bank detached. */
int fmx_fm_inbatch_bank_backward(const float *Su, int32_t ld_u, const float *au, const float *Sc, int32_t ld_c, const float *ac,
                                 int32_t B, int32_t kp, const float *corr, const int32_t *key, const fmx_item_bank_t *bank,
                                 float inv_b, void *lse, int64_t lse_bytes, float *gSu, float *gSc, float *gac, fmx_stream_t stream);

/* The push on its own: Sc [B, ld_c], a_c = ac (+ ac2 when it is not null: one fp32 addition), corr and key [B] (each null exactly
 * when the bank's is) to the slots (head + j) mod M; then the state advances.  One workgroup: its threads read the state, meet at
 * a barrier, one of them writes the new state and all of them the slots -- no second launch and no race.
 * Replaces: the torch.cat / index_copy_ of a cross-batch negative queue (torch.log_softmax(cat(...))'s bank side). */
int fmx_fm_inbatch_bank_push(const fmx_item_bank_t *bank, const float *Sc, int32_t ld_c, const float *ac, const float *ac2,
                             const float *corr, const int32_t *key, int32_t B, fmx_stream_t stream);

/* Bytes of a bank step's workspace: fmx_fm_inbatch_workspace_bytes' layout with the bank calls' lse block in the place of the
 * plain one.  Zero-fill once before the first use.  Negative on a bad argument.
 * Replaces: the temporaries of torch.log_softmax(cat(...)) and its autograd graph. */
int64_t fmx_fm_inbatch_bank_workspace_bytes(const fmx_table_t *table, int32_t B, int32_t M, int32_t n_item_fields);

/* fmx_fm_inbatch_step with the bank: one stream, capturable.  Bit-identical to this sequence of public calls: the masked copies,
 * fmx_sort_occurrences, the two fmx_fm_forward calls, fmx_fm_inbatch_bank_forward, fmx_fm_inbatch_bank_backward,
 * fmx_fm_inbatch_occ_grad, fmx_fm_update_occ on the table with its bias pointed at scratch, fmx_fm_inbatch_bank_push(S_c, sfirst,
 * sbi, corr, key).  With count = 0 the table, the moments, loss_out, the per-row losses and the error word are fmx_fm_inbatch_step's
 * bit for bit.  Four launches more than the plain step from two batch ranges on (B >= 65), five up to B = 64.
 * Replaces: torch.log_softmax(cat(...)) on the masked forwards + loss.backward() + optimizer.step() + the queue's update. */
int fmx_fm_inbatch_bank_step(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx, const float *xv,
                             const int32_t *item_fields, int32_t n_item_fields, const float *corr, const int32_t *key,
                             const fmx_item_bank_t *bank, int32_t B, float inv_b, void *workspace, int64_t workspace_bytes,
                             const fmx_fwd_out_t *fwd, float *loss_out, fmx_stream_t stream);

/* fmx_fm_inbatch_stream with the bank: bit-identical to n_steps calls of fmx_fm_inbatch_bank_step, the bank's contents and state at
 * the end included.
 * Replaces: the training loop around torch.log_softmax(cat(...)) + backward + optimizer.step() + the queue's update. */
int fmx_fm_inbatch_bank_stream(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const int32_t *idx_pool,
                               const int32_t *item_fields, int32_t n_item_fields, const float *corr_pool, const int32_t *key_pool,
                               const fmx_item_bank_t *bank, int32_t n_pool, int32_t B, float inv_b, int32_t n_steps, void *workspace,
                               int64_t workspace_bytes, const fmx_fwd_out_t *fwd, float *loss_out, fmx_stream_t stream);

/* ---- the small relu MLP on top of the bi-interaction vector (online steps of DeepFM / NFM and the ONN classes) ----
 * params: per layer W [out, in] row-major then b [out]; layer 0 maps k -> hidden, the others hidden -> hidden; the network's
 * contribution to the logit is the sum of the last activation (reference deepfm_adam.py:82-88: there is no output layer).
 * One workgroup per call; limits B <= 16, k <= 64 (63 for fit), hidden <= 64, layers <= 8, else FMX_ERR_UNSUPPORTED (larger
 * shapes stay on the caller's PyTorch path). */
typedef struct fmx_mlp {
  float *params;
  int32_t n_layers, k, hidden, reserved;
} fmx_mlp_t;

/* out [B] = base + sum_j x_L[j]  (may be null) ; layers_out [L, B] = sigmoid(base + sum_j x_l[j]) (may be null).
 * Replaces: the MLP part of forward() (reference deepfm_adam.py:79-89, deepfm_onn.py:88-102). */
int fmx_mlp_forward(const fmx_mlp_t *mlp, const float *bi, int32_t kp, const float *base, int32_t B, float *out,
                    float *layers_out, fmx_stream_t stream);

/* Forward, loss (fmx_loss on base + MLP), backward and the update of every hidden layer under `rule`
 * (FMX_RULE_SIGNADAM = the reference's fresh Adam, or FMX_RULE_SGD); emits what fmx_fm_update needs for the tables:
 * dz_out [B] = dL/dlogit and gbi_out [B, kp] = dL/dbi through the MLP.  loss_out [1] = mean loss (may be null).
 * Replaces: DeepFMAdam.fit / NFMAdam.fit minus the table part (reference deepfm_adam.py:106-119, nfm_adam.py:105-118). */
int fmx_mlp_fit(const fmx_mlp_t *mlp, const fmx_hyper_t *hyper, int32_t rule, int32_t loss_kind, const float *bi, int32_t kp,
                const float *base, const float *y, int32_t B, float inv_b, float *dz_out, float *gbi_out, float *loss_out,
                fmx_stream_t stream);

/* Hedge backprop (reference deepfm_onn.py:109-154): per-layer BCELoss(sigmoid(base + sum x_l), y), hidden layers updated by
 * lr * sum_{i >= j} alpha_i dloss_i/dlayer_j, then alpha_i <- max(alpha_i * hedge_b^loss_i, hedge_s / L) normalised.
 * alpha [L] is updated in place; losses_out [L] may be null.  The tables are not touched (as in the reference). */
int fmx_mlp_hedge_fit(const fmx_mlp_t *mlp, float lr, float hedge_b, float hedge_s, float *alpha, const float *bi, int32_t kp,
                      const float *base, const float *y, int32_t B, float *losses_out, fmx_stream_t stream);

/* The reference's online protocol for the classes with an MLP on a device-resident stream of N samples: per sample the
 * forward (pred_out[i] = what forward() returns: the logit for the Adam classes, sigmoid of the last layer's logit for
 * the ONN classes), then fit on that sample -- hedge = 0: fmx_mlp_fit + the table update (DeepFMAdam / NFMAdam.fit),
 * hedge = 1: fmx_mlp_hedge_fit (the ONN classes: hidden layers and alpha only; a table of any layout is read).  The fit mode
 * takes FMX_RULE_SIGNADAM / FMX_RULE_SGD, i.e. tables in the weights layout: any other pairing is FMX_ERR_ARG
 * (FMX_ERR_UNSUPPORTED for the adaptive rules).  fm_term: the FM logit is part of the
 * network's input logit (DeepFM) or only the first-order sum and the bias (NFM).  One workgroup walks the stream with the
 * network's parameters in LDS (k_online_mlp) when they are at most 8,192 floats, the fields fit one wavefront and the tables
 * are not FTRL tables under a fit step; otherwise the launches of all samples are queued without any host synchronisation
 * (2 per sample with Hedge, 4 otherwise).  Either way the parameters end bit-identical to per-sample calls.  workspace: fmx_workspace_bytes(table, 1);
 * fwd: S, bi, sfirst, logit of at least one sample; scratch: >= kp + 8 floats, 16-byte aligned.
 * Replaces: the loop body of run_experiment (reference deepfm_adam.py:128-130, deepfm_onn.py:178-180, ...). */
int fmx_online_run_mlp(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, int32_t loss_kind,
                       const fmx_mlp_t *mlp, int32_t hedge, int32_t fm_term, float hedge_b, float hedge_s, float *alpha,
                       const int32_t *idx, const float *xv, const float *y, int32_t N, void *workspace, int64_t workspace_bytes,
                       const fmx_fwd_out_t *fwd, float *scratch, float *pred_out, fmx_stream_t stream);

/* The same network at mini-batch sizes (BASELINE configs[3]: 3 x 256, B = 4096), any B / hidden / k, up to 8 layers:
 * forward, loss on (base + sum_j x_L[j]), backward -- fp32 MFMA GEMMs (v_mfma_f32_32x32x2_f32: exact f32 products and
 * accumulation), deterministic (split-K partials summed in a fixed order, no atomics).
 *   bi [B, ld_bi] (first k columns used), base [B], y [B];  logit_out [B] may be null
 *   dz_out [B] = dL/dlogit (inv_b folded in), gbi_out [B, ld_gbi] = dL/dbi through the MLP (columns k..ld_gbi-1 zeroed)
 *   grads: flat, the layout of mlp->params (W_l [out, in] then b_l [out] per layer); lr_apply != 0 also applies
 *   params -= lr_apply * grads in the same pass (single-rank SGD); loss_out [1] = inv_b * sum of the per-sample losses
 *   workspace: fmx_mlp_section_workspace_bytes(mlp, B) bytes, 16-byte aligned (activations, dH ping-pong, split partials)
 * Replaces: the MLP part of DeepFMAdam.fit / NFMAdam.fit at batch sizes the one-workgroup kernel does not take
 * (reference deepfm_adam.py:79-89,106-119; nfm_adam.py:78-88,105-118), i.e. nn.Linear + relu + autograd. */
/* Forward only at mini-batch sizes (predict / forward() of the MLP classes on whole batches, e.g. the accuracy print of
 * the pre-training loop, reference main_experiment.py:98): logit_out [B] = base + sum_j x_L[j] (may be null),
 * layers_out [L, B] = sigmoid(base + sum_j x_l[j]) per layer (may be null; what the ONN classes' forward() returns).
 * Same GEMMs and workspace as fmx_mlp_section. */
int fmx_mlp_forward_batch(const fmx_mlp_t *mlp, const float *bi, int32_t ld_bi, const float *base, int32_t B, void *workspace,
                          float *logit_out, float *layers_out, fmx_stream_t stream);
int64_t fmx_mlp_section_workspace_bytes(const fmx_mlp_t *mlp, int32_t B);
int fmx_mlp_section(const fmx_mlp_t *mlp, int32_t loss_kind, const float *bi, int32_t ld_bi, const float *base,
                    const float *y, int32_t B, float inv_b, void *workspace, float *logit_out, float *dz_out,
                    float *gbi_out, int32_t ld_gbi, float *grads, float lr_apply, float *loss_out, fmx_stream_t stream);

/* The mini-batch DeepFM loop over a device-resident stream of mini-batches (BASELINE configs[3]): step s uses batch (s mod n_pool);
 * per step the forward of the tables (S, bi, FM logit), fmx_mlp_section on bi with the FM logit as base (the SGD of the MLP applied in
 * its reduction: lr_mlp), then the row-reduced table update with dz_first = dz_bi = dL/dlogit and gbi = dL/dbi -- the launches of a
 * step issued back to back from one call, the occurrence sorts in groups on the library's side stream as in fmx_fm_stream.
 * idx_pool [n_pool, B, F], y_pool [n_pool, B]; fwd: S, bi, logit (dense, sample_ld = 0); dz [B], gbi [B, kp], grads (layout of
 * mlp->params) are scratch the call fills; loss_out [n_steps] or null; workspace: fmx_workspace_bytes(table, B), mlp_workspace:
 * fmx_mlp_section_workspace_bytes(mlp, B).  The result is the one of calling fmx_fm_forward, fmx_mlp_section, fmx_sort_occurrences
 * and fmx_fm_update per step.
 * fm_term: 1 = DeepFM (the FM logit is the network's base and dz also drives the FM term of the rows' gradient); 0 = NFM (base =
 * first-order sum + bias, written into fwd->logit's buffer; fwd->sfirst required; tables in the weights layout; the rows' gradient
 * comes through dL/dbi only -- reference nfm_adam.py:78-88,105-118).
 * Replaces: the mini-batch driver loop over DeepFMAdam.fit / NFMAdam.fit (reference main_experiment.py:92-105 with
 * deepfm_adam.py:106-119, nfm_adam.py:105-118). */
int fmx_deepfm_stream(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_mlp_t *mlp, int32_t loss_kind, int32_t fm_term,
                      const int32_t *idx_pool, const float *y_pool, int32_t n_pool, int32_t B, float inv_b, int32_t n_steps,
                      void *workspace, int64_t workspace_bytes, void *mlp_workspace, const fmx_fwd_out_t *fwd, float *dz, float *gbi,
                      float *grads, float lr_mlp, float *loss_out, fmx_stream_t stream);

/* ---- the network under a persistent rule of its own: fmx_mlp_section / fmx_deepfm_stream with a caller-owned optimizer state ----
 * m, v: flat fp32 device buffers in the layout of fmx_mlp_t.params (W_l [out, in] then b_l [out] per layer), 16-byte aligned.
 * The rule is applied to every parameter inside the fixed-order reduction of the weight gradients, in the pass that sums
 * them (no further launch, no atomics); `grads` receives the summed gradient g as in fmx_mlp_section.
 *   FMX_RULE_SGD      p -= lr * g                                               (m, v not touched; v must still be given)
 *   FMX_RULE_ADAGRAD  G += g*g;  p -= lr * g / (sqrt(G) + eps)                  (G in v; m may be null.  torch.optim.Adagrad,
 *                                                                               lr_decay = weight_decay = 0)
 *   FMX_RULE_ADAM     m += (1-beta1)(g - m);  v += (1-beta2)(g*g - v);
 *                     p -= step_size * m / (sqrt(v) + eps sqrt(1 - beta2^t)),  step_size = lr sqrt(1 - beta2^t) / (1 - beta1^t)
 *                     -- torch.optim.Adam, lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps), rearranged; it differs
 *                     from the tables' FMX_RULE_ADAM (SparseAdam) in where eps enters.  t = step + 1 for the call's first step.
 * step_size and eps sqrt(1 - beta2^t) are computed on the host in double, once per step (fmx_online_run_mlp_opt's one-workgroup
 * form: on the device, by the same function).  `step` is read, never written: the caller advances it by the steps a call took. */
typedef struct fmx_mlp_opt {
  float *m, *v;
  float lr, eps, beta1, beta2;
  int32_t rule; /* FMX_RULE_SGD, FMX_RULE_ADAGRAD or FMX_RULE_ADAM (fmx_afm_step_opt / fmx_afm_stream: FMX_RULE_SIGNADAM too) */
  int32_t step; /* FMX_RULE_ADAM: steps already taken */
} fmx_mlp_opt_t;

/* fmx_mlp_section with the network's update under opt->rule instead of lr_apply, and with the workspace's size.  grads,
 * dz_out, gbi_out, logit_out and loss_out are bit-identical to fmx_mlp_section with lr_apply = 0 on the same inputs; under
 * FMX_RULE_SGD params too are those of fmx_mlp_section(lr_apply = opt->lr).
 * Before anything is launched: opt null, an unknown rule, v null, m null under FMX_RULE_ADAM, a beta outside [0, 1), step < 0
 * or step + 1 beyond int32: FMX_ERR_ARG; mlp->params, grads, m or v not 16-byte aligned: FMX_ERR_ALIGN; workspace_bytes <
 * fmx_mlp_section_workspace_bytes(mlp, B): FMX_ERR_SHAPE. */
int fmx_mlp_section_opt(const fmx_mlp_t *mlp, int32_t loss_kind, const float *bi, int32_t ld_bi, const float *base,
                        const float *y, int32_t B, float inv_b, void *workspace, int64_t workspace_bytes, float *logit_out,
                        float *dz_out, float *gbi_out, int32_t ld_gbi, float *grads, const fmx_mlp_opt_t *opt, float *loss_out,
                        fmx_stream_t stream);

/* fmx_deepfm_stream with the network under opt->rule and the tables under ANY rule fmx_fm_stream takes, FMX_RULE_ADAGRAD /
 * FMX_RULE_ADAM on a MOMENTS table included.  Step s of the call is step t = hyper->step + s + 1 of the tables (as in
 * fmx_fm_stream) and t = opt->step + s + 1 of the network.  The result is the one of calling fmx_fm_forward,
 * fmx_mlp_section_opt, fmx_sort_occurrences and fmx_fm_update per step with both counts advanced by the caller, bit for bit.
 * fm_term = 0 (NFM) takes tables in the weights or the moments layout (bias[0] is the bias weight in both), not FTRL tables.
 * Every argument is checked before the first launch: fmx_deepfm_stream's checks, FMX_RULE_ADAM's hyper-parameters
 * (fmx_fm_stream), fmx_mlp_section_opt's checks of mlp, grads, opt (step + n_steps within int32) and mlp_workspace_bytes. */
int fmx_deepfm_stream_opt(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_mlp_t *mlp, int32_t loss_kind,
                          int32_t fm_term, const int32_t *idx_pool, const float *y_pool, int32_t n_pool, int32_t B, float inv_b,
                          int32_t n_steps, void *workspace, int64_t workspace_bytes, void *mlp_workspace, int64_t mlp_workspace_bytes,
                          const fmx_fwd_out_t *fwd, float *dz, float *gbi, float *grads, const fmx_mlp_opt_t *opt, float *loss_out,
                          fmx_stream_t stream);

/* ---- pairwise-ranking (BPR) training of DeepFM / NFM: the pair loss on the whole network's logit ----
 * The layout is fmx_fm_pair_forward's: B_pairs pairs are 2 B_pairs rows, row 2i the positive and row 2i + 1 the negative;
 * z_b = base_b + sum_j H_L[b, j] as the pointwise section sums it, d_i = z[2i] - z[2i + 1], loss_i = -log(sigmoid(d_i) + margin)
 * and g_i = d loss_i / d d_i as stated there (one device function evaluates both families).  No label is read.
 *
 * fmx_mlp_section on pairs: bi [2 B_pairs, ld_bi], base [2 B_pairs]; logit_out [2 B_pairs] (may be null) has the bits
 * fmx_mlp_section writes for the same bi / base;
 *   dz_out[2i] = g_i * inv_b, dz_out[2i + 1] = -dz_out[2i] (the same float negated: the two sum to exactly 0),
 *   gbi_out [2 B_pairs, ld_gbi] and grads as in fmx_mlp_section with that dz; loss_out [1] = inv_b * sum_i loss_i (may be null).
 * opt null: params -= lr_apply * grads in the same pass (lr_apply = 0 leaves the parameters alone); opt given: opt->rule as in
 * fmx_mlp_section_opt, this call being step t = opt->step + 1, and lr_apply is not read.  grads, dz_out, gbi_out and logit_out
 * do not depend on opt / lr_apply.  workspace: fmx_mlp_section_workspace_bytes for 2 * B_pairs rows (smaller: FMX_ERR_SHAPE).
 * Before anything is launched: B_pairs < 1 and a negative / NaN / infinite margin are FMX_ERR_ARG, then what fmx_mlp_section
 * refuses and, with opt, what fmx_mlp_section_opt refuses.
 * Replaces: nn.Linear + relu + autograd of DeepFMAdam.fit / NFMAdam.fit (reference deepfm_adam.py:79-89,106-119;
 * nfm_adam.py:78-88,105-118) under the pair objective of reference models/models_meta_emb/meta_fm.py:145-169. */
int fmx_mlp_pair_section(const fmx_mlp_t *mlp, const float *bi, int32_t ld_bi, const float *base, int32_t B_pairs, float margin,
                         float inv_b, void *workspace, int64_t workspace_bytes, float *logit_out, float *dz_out, float *gbi_out,
                         int32_t ld_gbi, float *grads, float lr_apply, const fmx_mlp_opt_t *opt, float *loss_out,
                         fmx_stream_t stream);

/* n_steps pair steps of DeepFM (fm_term = 1) / NFM (fm_term = 0) over a device-resident pool idx_pool [n_pool, 2 B_pairs, F]
 * (every feature value 1): step s takes batch (s mod n_pool).  opt null: the checks and rules of fmx_deepfm_stream (the network
 * under SGD by lr_mlp); opt given: those of fmx_deepfm_stream_opt (lr_mlp is not read; step s is step hyper->step + s + 1 of
 * the tables and opt->step + s + 1 of the network).  In front of them the refusals of the fmx_fm_pair_stream family: a null table /
 * hyper / idx_pool, B_pairs < 1, a bad margin: FMX_ERR_ARG; field_cols / field_base: FMX_ERR_UNSUPPORTED; 2 * B_pairs beyond the
 * sort's width: what fmx_sort_occurrences reports.  fwd, dz, gbi, workspace and mlp_workspace are sized for 2 * B_pairs rows;
 * mlp_workspace_bytes is checked under either rule.  fm_term = 1: base is the FM logit, the update takes dz_first = dz_bi = dz
 * and gbi; fm_term = 0: base is first-order sum + bias, the update takes dz_first = dz, no dz_bi, and gbi.
 * The result is, bit for bit, the one of calling fmx_fm_forward with FMX_LOSS_NONE on the 2 B_pairs rows, the NFM base add,
 * fmx_mlp_pair_section, fmx_sort_occurrences and fmx_fm_update per step, the counts advanced by the caller.  The bias gradient
 * sum_b dz_b is exactly +0, so FMX_RULE_SGD / SIGNADAM / FTRL / ADAGRAD leave the bias words as they are (FMX_RULE_ADAM decays its
 * moments).  loss_out [n_steps] or null.
 * Replaces: the mini-batch driver loop over DeepFMAdam.fit / NFMAdam.fit (reference main_experiment.py:92-105 with
 * deepfm_adam.py:106-119, nfm_adam.py:105-118) under the pair objective of reference meta_fm.py:145-169. */
int fmx_deepfm_pair_stream(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_mlp_t *mlp, int32_t fm_term,
                           const int32_t *idx_pool, int32_t n_pool, int32_t B_pairs, float margin, float inv_b, int32_t n_steps,
                           void *workspace, int64_t workspace_bytes, void *mlp_workspace, int64_t mlp_workspace_bytes,
                           const fmx_fwd_out_t *fwd, float *dz, float *gbi, float *grads, float lr_mlp, const fmx_mlp_opt_t *opt,
                           float *loss_out, fmx_stream_t stream);

/* ---- listwise (sampled-softmax) training of DeepFM / NFM: the list loss on the whole network's logit ----
 * The layout is fmx_fm_list_forward's: B_lists lists of G rows (2 <= G <= 16) are B_lists G rows, row G i the positive of list i
 * and rows G i + 1 .. G i + G - 1 its negatives; z_b = base_b + sum_j H_L[b, j] as the pointwise section sums it, and with
 * c_b = z_b - corr_b (corr: log Q of every row's item as in fmx_fm_list_forward_q, [B_lists G]; null: c_b = z_b, and a corr of
 * +0 gives the same bits) loss_i = -log softmax(c[G i .. G i + G - 1])[0], evaluated as stated at fmx_fm_list_forward (one
 * device formula for every list family).  No label is read.
 *
 * fmx_mlp_section on lists: bi [B_lists G, ld_bi], base [B_lists G]; logit_out [B_lists G] (may be null) is the UNCORRECTED z,
 * the serving score, with the bits fmx_mlp_forward_batch writes for the same bi / base;
 *   dz_out[G i + j] = inv_b * d loss_i / d z[G i + j]: negative for the positive, positive for every negative, summing to
 *   zero over a list up to rounding; gbi_out [B_lists G, ld_gbi] and grads as in fmx_mlp_section with that dz;
 *   loss_out [1] = inv_b * sum_i loss_i (may be null).
 * opt null: params -= lr_apply * grads in the same pass (lr_apply = 0 leaves the parameters alone); opt given: opt->rule as in
 * fmx_mlp_section_opt, this call being step t = opt->step + 1, and lr_apply is not read.  grads, dz_out, gbi_out and logit_out
 * do not depend on opt / lr_apply.  workspace: fmx_mlp_section_workspace_bytes for B_lists * G rows (smaller: FMX_ERR_SHAPE).
 * The section always runs as separate launches (the forward GEMMs, k_mlp_list_loss -- one wavefront per list --, the dgrad
 * GEMMs, the weight gradients, the reduction): fmx_set_option("mlp_chain", ...) does not change a bit of its results.
 * Before anything is launched: B_lists < 1, G < 2 and B_lists * G beyond int32 are FMX_ERR_ARG, G > 16 FMX_ERR_UNSUPPORTED,
 * then what fmx_mlp_section refuses (a null mlp / params / workspace / bi / base / dz_out / gbi_out / grads: FMX_ERR_ARG; ld_bi
 * or ld_gbi < k: FMX_ERR_SHAPE) and, with opt, what fmx_mlp_section_opt refuses.  Every message names fmx_mlp_list_section.
 * Replaces: nn.Linear + relu + autograd of DeepFMAdam.fit / NFMAdam.fit (reference deepfm_adam.py:79-89,106-119;
 * nfm_adam.py:78-88,105-118) under a softmax cross-entropy over the positive and its sampled negatives, which the reference
 * does not have (nearest: the pair objective of reference models/models_meta_emb/meta_fm.py:145-169). */
int fmx_mlp_list_section(const fmx_mlp_t *mlp, const float *bi, int32_t ld_bi, const float *base, const float *corr,
                         int32_t B_lists, int32_t G, float inv_b, void *workspace, int64_t workspace_bytes, float *logit_out,
                         float *dz_out, float *gbi_out, int32_t ld_gbi, float *grads, float lr_apply, const fmx_mlp_opt_t *opt,
                         float *loss_out, fmx_stream_t stream);

/* n_steps list steps of DeepFM (fm_term = 1) / NFM (fm_term = 0) over a device-resident pool idx_pool [n_pool, B_lists G, F]
 * (every feature value 1) with corr_pool [n_pool, B_lists G] or null beside it: step s takes batch (s mod n_pool).  opt null:
 * the checks and rules of fmx_deepfm_stream (the network under SGD by lr_mlp); opt given: those of fmx_deepfm_stream_opt (lr_mlp
 * is not read; step s is step hyper->step + s + 1 of the tables and opt->step + s + 1 of the network).  In front of them the
 * refusals of the fmx_fm_list_stream family: a null table / hyper / idx_pool, B_lists < 1, G < 2, B_lists * G beyond int32:
 * FMX_ERR_ARG; G > 16, field_cols / field_base: FMX_ERR_UNSUPPORTED; B_lists * G beyond the sort's width: what
 * fmx_sort_occurrences reports; n_pool < 1, n_steps < 0: FMX_ERR_ARG.  Every message names fmx_deepfm_list_stream, and
 * n_steps = 0 launches nothing.  fwd, dz, gbi and mlp_workspace are sized for B_lists * G rows; mlp_workspace_bytes is checked
 * under either rule (FMX_ERR_SHAPE).  workspace: fmx_fm_list_workspace_bytes(table, B_lists, G) bytes -- the step workspace and
 * the 16 bytes behind it on which the bias rule runs (smaller: FMX_ERR_SHAPE): the bias of a list step has no gradient but
 * rounding, so the table's bias and its state stay bit-unchanged under every rule, as in fmx_fm_list_step.
 * fm_term = 1: base is the FM logit, the update takes dz_first = dz_bi = dz and gbi; fm_term = 0: base is first-order sum + bias,
 * the update takes dz_first = dz, no dz_bi, and gbi.  The section's reduction rides in the table update's launch.
 * The result is, bit for bit, the one of calling fmx_fm_forward with FMX_LOSS_NONE on the B_lists G rows, the NFM base add,
 * fmx_mlp_list_section, fmx_sort_occurrences and fmx_fm_update (on a table struct whose bias points at scratch) per step, the
 * counts advanced by the caller.  loss_out [n_steps] or null.
 * Replaces: the mini-batch driver loop over DeepFMAdam.fit / NFMAdam.fit (reference main_experiment.py:92-105 with
 * deepfm_adam.py:106-119, nfm_adam.py:105-118) under the list objective above. */
int fmx_deepfm_list_stream(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_mlp_t *mlp, int32_t fm_term,
                           const int32_t *idx_pool, int32_t n_pool, int32_t B_lists, int32_t G, const float *corr_pool, float inv_b,
                           int32_t n_steps, void *workspace, int64_t workspace_bytes, void *mlp_workspace, int64_t mlp_workspace_bytes,
                           const fmx_fwd_out_t *fwd, float *dz, float *gbi, float *grads, float lr_mlp, const fmx_mlp_opt_t *opt,
                           float *loss_out, fmx_stream_t stream);

/* fmx_mlp_fit (the one-workgroup kernel: B <= 16, k <= 63, hidden <= 64, layers <= 8) with the hidden layers under opt->rule
 * (FMX_RULE_SGD, FMX_RULE_ADAGRAD, FMX_RULE_ADAM as stated at fmx_mlp_opt_t: the network's ADAM is torch.optim.Adam, the tables'
 * is SparseAdam) instead of `rule`: the thread that sums a parameter's gradient over the batch in sample order applies the rule to
 * (p, m, v) of that parameter.  This call is step t = opt->step + 1; opt->step is read and never written.  hyper is not read
 * (it may be null): the network's learning rate and eps are opt's.  dz_out, gbi_out and loss_out are bit-identical to
 * fmx_mlp_fit on the same inputs (the update does not feed them); under FMX_RULE_SGD params too are those of
 * fmx_mlp_fit(rule = FMX_RULE_SGD, lr = opt->lr).
 * Before anything is launched: fmx_mlp_fit's checks, then opt null, an unknown rule, v null, m null under FMX_RULE_ADAM, a beta
 * outside [0, 1), step < 0 or step + 1 beyond int32: FMX_ERR_ARG; mlp->params, m or v not 16-byte aligned: FMX_ERR_ALIGN.
 * Replaces: DeepFMAdam.fit / NFMAdam.fit minus the table part (reference deepfm_adam.py:106-119, nfm_adam.py:105-118) with a
 * persistent torch.optim.Adam / Adagrad over the hidden layers in place of the fresh Adam per call. */
int fmx_mlp_fit_opt(const fmx_mlp_t *mlp, const fmx_hyper_t *hyper, int32_t loss_kind, const float *bi, int32_t kp,
                    const float *base, const float *y, int32_t B, float inv_b, float *dz_out, float *gbi_out, float *loss_out,
                    const fmx_mlp_opt_t *opt, fmx_stream_t stream);

/* The fit mode of fmx_online_run_mlp (no Hedge: Hedge has a rule of its own) with the network under opt->rule and the tables
 * under ANY rule fmx_fm_online_run takes, FMX_RULE_ADAGRAD / FMX_RULE_ADAM on a MOMENTS table included; the two rules are
 * independent.  Sample i of the call is step t = hyper->step + i + 1 of the tables and t = opt->step + i + 1 of the network
 * (both counts are read, never written: the caller advances them by N).
 * One workgroup walks the stream (k_online_mlp) when the network has at most 8,192 parameters, the fields fit one wavefront and
 * the tables are not FTRL tables: the parameters AND the network's moments live in LDS for the length of the stream (4 bytes
 * per parameter, 8 under FMX_RULE_ADAGRAD, 12 under FMX_RULE_ADAM: at most 96 KB beside the kernel's 47 KB of static arrays, of
 * the CU's 160 KiB) and are written back at the end; ADAM's constants of a sample are derived on the device by the function the
 * host uses (same bits).  Otherwise, and with fmx_set_option("online_persistent", 0), the launches of all samples are queued
 * without any host synchronisation (forward, the network's step with the host's per-sample constants, sort, update).  Both forms
 * end in the bits of per-sample calls -- fmx_fm_forward, fmx_mlp_fit_opt, fmx_sort_occurrences, fmx_fm_update with hyper->step
 * and opt->step advanced by the caller: rows (moments included), bias words, params, m, v and pred_out.
 * Every argument is checked before the first launch (N = 0 included, which then launches nothing): fmx_online_run_mlp's checks,
 * fmx_mlp_fit_opt's checks of opt with step + N within int32, the pairing of rule and layout and FMX_RULE_ADAM's hyper-parameters
 * with step + N within int32 as in fmx_fm_online_run (FMX_ERR_ARG); fm_term = 0 on an FTRL table: FMX_ERR_UNSUPPORTED.
 * workspace, fwd, scratch: as for fmx_online_run_mlp.
 * Replaces: the loop body of run_experiment (reference deepfm_adam.py:128-130, nfm_adam.py:128-130) over predict and fit
 * (deepfm_adam.py:106-130, nfm_adam.py:105-130) with persistent optimizers in place of the fresh Adam per call. */
int fmx_online_run_mlp_opt(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, int32_t loss_kind,
                           const fmx_mlp_t *mlp, int32_t fm_term, const int32_t *idx, const float *xv, const float *y, int32_t N,
                           void *workspace, int64_t workspace_bytes, const fmx_fwd_out_t *fwd, float *scratch, float *pred_out,
                           const fmx_mlp_opt_t *opt, fmx_stream_t stream);

/* ---- the one-workgroup pair step and the online pair loop of DeepFM / NFM ----
 * fmx_mlp_fit / fmx_mlp_fit_opt on 2 * B_pairs rows under the pair loss: row 2i is the positive of pair i, row 2i + 1 its
 * negative, and no label is read.  z_b = base_b + sum_j x_L[b, j] summed as the pointwise modes sum it: logit_out [2 B_pairs]
 * (may be null) has the bits fmx_mlp_forward writes for the same bi / base.  d_i = z[2i] - z[2i + 1], loss_i and g_i as stated at
 * fmx_mlp_pair_section (one device function evaluates every pair family);
 *   dz_out[2i] = g_i * inv_b, dz_out[2i + 1] = the same float negated (the two sum to exactly +0),
 *   loss_out[0] (may be null) = inv_b * the ordered sum over the rows of loss_{2i} = loss_i, loss_{2i+1} = +0,
 *   gbi_out [2 B_pairs, kp] as fmx_mlp_fit writes it (columns k..kp-1 zeroed).
 * The backward pass and the parameter update are fmx_mlp_fit's: opt null -- `rule` (FMX_RULE_SIGNADAM / FMX_RULE_SGD) by hyper's
 * lr / eps; opt given -- opt->rule as in fmx_mlp_fit_opt, this call being step opt->step + 1 (read, never written), and hyper and
 * rule are not read.  dz_out, gbi_out, logit_out and loss_out do not depend on the rule.
 * Limits: fmx_mlp_fit's on 2 * B_pairs rows -- 1 <= B_pairs <= 8, k <= 63, hidden <= 64, layers <= 8, else FMX_ERR_UNSUPPORTED.
 * Before anything is launched: B_pairs < 1 and a negative / NaN / infinite margin are FMX_ERR_ARG, then fmx_mlp_fit's null
 * checks and, with opt, what fmx_mlp_fit_opt refuses.
 * Replaces: DeepFMAdam.fit / NFMAdam.fit minus the table part (reference deepfm_adam.py:106-119, nfm_adam.py:105-118) under the
 * pair objective of reference models/models_meta_emb/meta_fm.py:145-169. */
int fmx_mlp_pair_fit(const fmx_mlp_t *mlp, const fmx_hyper_t *hyper, int32_t rule, const float *bi, int32_t kp,
                     const float *base, int32_t B_pairs, float margin, float inv_b, float *logit_out, float *dz_out,
                     float *gbi_out, float *loss_out, const fmx_mlp_opt_t *opt, fmx_stream_t stream);

/* The online predict-then-fit protocol on N device-resident pairs idx [2N, F] (xv [2N, F] or null) through the whole network
 * of DeepFM (fm_term = 1) / NFM (fm_term = 0): for every pair, pred_out[i] = z_pos > z_neg, logit_out[2i], logit_out[2i + 1] (or
 * null) and loss_out[i] (or null) with the weights BEFORE the pair's update, then one pair step on that pair alone.  The
 * definition, bit for bit, is N times from outside: fmx_fm_forward(B = 2, FMX_LOSS_NONE), the NFM base add (sfirst + bias weight)
 * when fm_term = 0, fmx_mlp_pair_fit(B_pairs = 1, inv_b = 1), fmx_sort_occurrences(B = 2), fmx_fm_update(B = 2, dz_first = dz,
 * dz_bi = fm_term ? dz : null, gbi, inv_b = 1), the caller advancing hyper->step and opt->step -- rows (moments included), bias
 * words, params, m, v, pred_out, logit_out and loss_out.  Pair i is step hyper->step + i + 1 of the tables and opt->step + i + 1
 * of the network (both read, never written).
 * opt null: the pairing of fmx_online_run_mlp's fit mode (FMX_RULE_SIGNADAM / FMX_RULE_SGD on a weights table, the network under
 * the same rule); opt given: that of fmx_online_run_mlp_opt (any table rule, the network under opt->rule; fm_term = 0 on an FTRL
 * table: FMX_ERR_UNSUPPORTED).  The bias gradient dz[0] + dz[1] is exactly +0: only FMX_RULE_ADAM moves the bias words.
 * One workgroup walks the stream (k_online_mlp_pair: wave 0 holds both samples' rows, the parameters and the network's moments
 * live in LDS, at most 96 KB beside the kernel's 47 KB of static arrays) when the network has at most 8,192 parameters,
 * n_fields <= 4 * (64 / (kp / 4)) and the tables are not FTRL tables; otherwise, and with
 * fmx_set_option("online_persistent", 0), the four launches of every pair are queued without any host synchronisation.
 * Every argument is checked before the first launch, N = 0 included (which launches nothing; idx, xv and the three outputs may
 * then be null): a null table / hyper / idx / pred_out, N < 0, 2 * N beyond int32, a bad margin: FMX_ERR_ARG; field_cols /
 * field_base: FMX_ERR_UNSUPPORTED; then fmx_mlp_pair_fit's checks of mlp and opt (step + N within int32), the pairing of rule and
 * layout, FMX_RULE_ADAM's hyper-parameters.  workspace: fmx_workspace_bytes(table, 2) bytes (smaller: FMX_ERR_SHAPE); fwd: S, bi,
 * sfirst, logit of two samples, and fwd->error takes the index flag; scratch: >= 2 * kp + 8 floats (dz [2] at 0, gbi [2, kp]
 * at 8), 16-byte aligned.
 * Replaces: the loop body of run_experiment (reference deepfm_adam.py:128-130, nfm_adam.py:128-130) restated for the pair
 * objective of reference meta_fm.py:145-169. */
int fmx_online_run_mlp_pair(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_mlp_t *mlp,
                            int32_t fm_term, const int32_t *idx, const float *xv, int32_t N, float margin, void *workspace,
                            int64_t workspace_bytes, const fmx_fwd_out_t *fwd, float *scratch, uint8_t *pred_out,
                            float *logit_out, float *loss_out, const fmx_mlp_opt_t *opt, fmx_stream_t stream);

/* ---- the one-workgroup list step and the online list loop of DeepFM / NFM ----
 * fmx_mlp_fit / fmx_mlp_fit_opt on B_lists * G rows under the list loss of fmx_mlp_list_section: row G i is the positive of list
 * i, rows G i + 1 .. G i + G - 1 its negatives, and no label is read.  z_b = base_b + sum_j x_L[b, j] summed as the pointwise
 * modes sum it: logit_out [B_lists G] (may be null) has the bits fmx_mlp_forward writes for the same bi / base.  The softmax runs
 * on z_b - corr_b (corr [B_lists G]: log Q of every row's item; null: no correction, bit for bit a corr of +0) with the formula and
 * the operand order stated at fmx_fm_list_forward (one device function evaluates every list family); the logit stored is the
 * uncorrected z.
 *   dz_out [B_lists G] = dL/dlogit * inv_b (a list's sum to zero up to rounding; at G = 2 the two are exact negatives),
 *   loss_out[0] (may be null) = inv_b * the ordered sum over the rows of loss_{G i} = loss_i, +0 in the negatives' slots,
 *   gbi_out [B_lists G, kp] as fmx_mlp_fit writes it (columns k..kp-1 zeroed),
 *   rank_out[i] (uint8 [B_lists], may be null) = the negatives of list i with z_j >= z_0 on the uncorrected logits
 *   (fmx_fm_list_online_run's definition).
 * The backward pass and the parameter update are fmx_mlp_fit's: opt null -- `rule` (FMX_RULE_SIGNADAM / FMX_RULE_SGD) by hyper's
 * lr / eps; opt given -- opt->rule as in fmx_mlp_fit_opt, this call being step opt->step + 1 (read, never written), and hyper and
 * rule are not read.  dz_out, gbi_out, logit_out, loss_out and rank_out do not depend on the rule.
 * Limits: fmx_mlp_fit's on B_lists * G rows -- B_lists * G <= 16, 2 <= G <= 16, k <= 63, hidden <= 64, layers <= 8, else
 * FMX_ERR_UNSUPPORTED.  Before anything is launched: the list's shape as fmx_mlp_list_section refuses it, then fmx_mlp_pair_fit's
 * checks of mlp, rule and opt, and its null checks.
 * Replaces: DeepFMAdam.fit / NFMAdam.fit minus the table part (reference deepfm_adam.py:106-119, nfm_adam.py:105-118) under the
 * sampled-softmax objective.  Restates: fmx_mlp_list_section's loss at the one-workgroup step's loss site. */
int fmx_mlp_list_fit(const fmx_mlp_t *mlp, const fmx_hyper_t *hyper, int32_t rule, const float *bi, int32_t kp,
                     const float *base, const float *corr, int32_t B_lists, int32_t G, float inv_b, float *logit_out,
                     float *dz_out, float *gbi_out, float *loss_out, uint8_t *rank_out, const fmx_mlp_opt_t *opt,
                     fmx_stream_t stream);

/* The online predict-then-fit protocol on N device-resident lists idx [N G, F] (xv [N G, F] or null; corr [N G] or null) through
 * the whole network of DeepFM (fm_term = 1) / NFM (fm_term = 0): for every list, rank_out[i] = the negatives whose logit is >= the
 * positive's, logit_out[G i .. G i + G - 1] (or null; the uncorrected logits) and loss_out[i] (or null) with the weights BEFORE
 * the list's update, then one list step of tables and network on that list alone, inv_b = 1.  The definition, bit for bit, is N
 * times from outside: fmx_fm_forward(B = G, FMX_LOSS_NONE), the NFM base add (sfirst + bias weight) when fm_term = 0,
 * fmx_mlp_list_fit(B_lists = 1, inv_b = 1), fmx_sort_occurrences(B = G), fmx_fm_update(B = G, dz_first = dz, dz_bi = fm_term ? dz :
 * null, gbi, inv_b = 1) on the list steps' copy of the table struct, whose bias points at the scratch behind the step workspace
 * (fmx_fm_list_workspace_bytes), the caller advancing hyper->step and opt->step -- rows (moments included), params, m, v,
 * rank_out, logit_out and loss_out.  The table's bias and its state are read and never written.  List i is step
 * hyper->step + i + 1 of the tables and opt->step + i + 1 of the network (both read, never written).
 * opt null / given: the pairings of fmx_online_run_mlp_pair.
 * One workgroup of 64 max(G, 4) threads walks the stream (k_online_mlp_list: wave j holds row j of the list, the parameters and
 * the network's moments live in LDS, at most 96 KB beside the kernel's static arrays of at most 54.1 KB: the cap of
 * fmx_online_run_mlp_pair stands) when G <= 8, the network has at most 8,192 parameters, with or without moments,
 * n_fields <= min(4 * (64 / (kp / 4)), 128) and the tables are not FTRL tables; otherwise (longer lists among it: at 16 waves a
 * wave has 128 registers and the kernel would spill), and with fmx_set_option("online_persistent", 0), the four launches of every
 * list are queued without any host synchronisation.
 * Every argument is checked before the first launch, N = 0 included (which launches nothing; idx, xv, corr and the three outputs
 * may then be null): what fmx_fm_list_online_run refuses of table, hyper, idx, N and G (a sort split among it:
 * FMX_ERR_UNSUPPORTED), a null rank_out, then fmx_online_run_mlp_pair's checks of workspace, fwd, scratch, mlp, opt, rule and
 * layout.  workspace: fmx_fm_list_workspace_bytes(table, 1, G) bytes (smaller: FMX_ERR_SHAPE); fwd: S, bi, sfirst, logit of G
 * samples, and fwd->error takes the index flag; scratch: >= 16 + G * kp floats (dz [G] at 0, gbi [G, kp] at 16), 16-byte aligned.
 * Replaces: the loop body of run_experiment (reference deepfm_adam.py:128-130, nfm_adam.py:128-130) restated for the
 * sampled-softmax objective.  Restates: fmx_fm_list_online_run for the classes with a network. */
int fmx_online_run_mlp_list(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_mlp_t *mlp,
                            int32_t fm_term, const int32_t *idx, const float *xv, const float *corr, int32_t N, int32_t G,
                            void *workspace, int64_t workspace_bytes, const fmx_fwd_out_t *fwd, float *scratch,
                            uint8_t *rank_out, float *logit_out, float *loss_out, const fmx_mlp_opt_t *opt, fmx_stream_t stream);

/* Hedge backprop at mini-batch sizes (the ONN classes' fit() beyond 16 samples; reference deepfm_onn.py:109-154): per
 * layer BCELoss(sigmoid(base + sum_j x_l[j]), y), hidden layers updated by lr * sum_{i >= j} alpha_i dloss_i/dlayer_j (one
 * backward pass on the same GEMMs; `grads` receives that gradient), then alpha_i <- max(alpha_i * hedge_b^loss_i,
 * hedge_s / L) normalised, in place.  losses_out [L] may be null.  The tables are not touched, as in the reference. */
int fmx_mlp_hedge_section(const fmx_mlp_t *mlp, float lr, float hedge_b, float hedge_s, float *alpha, const float *bi,
                          int32_t ld_bi, const float *base, const float *y, int32_t B, void *workspace, float *grads,
                          float *losses_out, fmx_stream_t stream);

/* The sketched-FTRL family on a device-resident stream (hot path B's sketch classes): for every
 * sample predict y_hat = ||BP^T x||^2 - ||BN^T x||^2 (+ w^T x), then append sqrt(eta |s|) x to the sketch the gradient sign s
 * picks and shrink a full sketch (frequent directions).  fp64 like the reference, strictly sequential: ONE wavefront walks the
 * stream with both sketches in LDS; the shrink is a Jacobi eigen-decomposition of the d x d Gram matrix (same B B^T as the
 * reference's SVD of B^T B; the columns of B may differ by sign).
 *   X [N, D], y [N] fp64; the first d features enter the sketches (d = D: SFTRL_CCFM; d = D - 1 with w, g_w [D]: SFTRL_Vanila)
 *   BP, BN [d, 2 m] row-major and counts [2] (columns in use) are read and written back; task 0 = cls (+-1 predictions), 1 = reg
 *   status [2]: status[0] = 1 when the prediction of sample status[1] was NaN (the run stops there)
 * Limits: d <= 32, 2 m <= 128, D <= 64, else FMX_ERR_UNSUPPORTED (the caller's host path).
 * The count after a shrink is the exact rank logic on the d x d spectrum (never more than d); it can differ from the host
 * path's once the rounding noise of that path's 2m x 2m SVD (~ eps lambda_max: a sketch norm from about 1e4 at thres = 1e-12)
 * exceeds thres -- B B^T agrees either way ("Sketched FTRL").
 * Replaces: SFTRL_CCFM.online_learning / _GFD (reference models/models_online/SFTRL_CCFM.py:30-121), SFTRL_Vanila.py:30-130. */
int fmx_sftrl_run(const double *X, const double *y, int32_t N, int32_t D, int32_t d, int32_t m, double eta, double thres,
                  int32_t task, double *BP, double *BN, int32_t *counts, double *w, double *g_w, double *pred_out,
                  int32_t *status, fmx_stream_t stream);

/* A GRID of sketched-FTRL settings over the same stream in one launch: workgroup s runs (ms[s], etas[s]) -- one wavefront
 * per setting is latency-bound, 256 CUs run 256 settings in the time of one (the reference's notebooks try (eta, m) pairs one
 * run_experiment at a time).  ms [S] int32 (each <= m_max), etas [S] fp64 are device arrays.  Per setting s:
 *   BP, BN  [S][d * 2 * m_max]: setting s's sketch as [d, 2 ms[s]] row-major at the start of its slot;  counts [S, 2];
 *   w, g_w  [S, D] or both null;  pred_out [S, N];  status [S, 2]  -- everything else as fmx_sftrl_run, same limits;
 *   status[s][0] = 2: ms[s] = status[s][1] lies outside [1, m_max] (the launch is sized for m_max): setting s was not run.
 * Every setting's result is bit-identical to its own fmx_sftrl_run. */
int fmx_sftrl_grid(const double *X, const double *y, int32_t N, int32_t D, int32_t d, int32_t n_settings, const int32_t *ms,
                   const double *etas, int32_t m_max, double thres, int32_t task, double *BP, double *BN, int32_t *counts, double *w,
                   double *g_w, double *pred_out, int32_t *status, fmx_stream_t stream);

/* FM_FTRL on a device-resident stream (hot path B's dense baseline): per sample x (D features; x' = x without its last one)
 *     t = W2 x';  y_hat = w1 . x + t . t;  s = (-1 / (1 + exp(y_hat y))) y (task 0, cls) or 2 (y_hat - y) (task 1, reg);
 *     g_w1 += s x;  g_W2 += 2 t x'^T (no factor s: the reference's quirk);  w1 = -eta g_w1;  W2 = -eta g_W2.
 * fp64, strictly sequential: ONE wavefront walks the stream; g_W2 lives in LDS and W2 is derived from it element by element (one
 * multiplication, the host's rounding of -eta * g_W2) -- only the first sample reads the caller's W2.
 *   X [N, D], y [N];  m2 = 2 m rows of W2;  w1, g_w1 [D] and W2, g_W2 [m2, D - 1] row-major are read and written back: a caller
 *   continues a stream by passing them on (a run cut in two gives the bits of the uninterrupted run); a fresh stream passes
 *   g_w1 = g_W2 = 0.  pred_out [N] receives the RAW y_hat (the caller takes the sign for cls).
 *   status [2]: (1, i) when y_hat of sample i was NaN: the walk stops in front of that sample's update; else not written.
 * Order of the floating-point operations (no atomics; the same bits on every run):
 *   t_r = fma(W2[r][j], x[j], t_r), j ascending from t_r = 0;
 *   y_hat = the sum over lanes l = 0..63 of fma(t_{l+64}, t_{l+64}, fma(t_l, t_l, w1[l] * x[l])) (absent terms are 0), added by
 *   the xor butterfly l ^ 1, l ^ 2, l ^ 4, ..., l ^ 32;
 *   the state updates are one multiplication and one addition each, as written above (no fma).
 * Limits: 2 <= D <= 64, m2 even, 2 <= m2 <= 128; beyond 64 / 128: FMX_ERR_UNSUPPORTED (there is no host fallback).  N = 0 launches nothing.
 * Replaces: FM_FTRL.online_learning (reference models/models_online/FM_FTRL.py:61-80). */
int fmx_ftrl_dense_run(const double *X, const double *y, int32_t N, int32_t D, int32_t m2, double eta, int32_t task, double *w1,
                       double *W2, double *g_w1, double *g_W2, double *pred_out, int32_t *status, fmx_stream_t stream);

/* A GRID of FM_FTRL settings over the same stream in one launch: workgroup s runs (m2s[s], etas[s]) (the reference's notebooks run
 * one (eta, m) pair per FM_FTRL object, reference models/models_online/FM_FTRL.py:27-92).  m2s [S] int32, etas [S] fp64 are device
 * arrays.  Per setting s:
 *   w1, g_w1 [S, D];  W2, g_W2 [S][m2_max * (D - 1)]: setting s's matrix as [m2s[s], D - 1] row-major at the start of its slot;
 *   pred_out [S, N];  status [S, 2]  -- everything else as fmx_ftrl_dense_run, the limits applied to m2_max;
 *   status[s] = (2, m2s[s]): m2s[s] is odd or outside [2, m2_max] (the launch is sized for m2_max): setting s was not run and
 *   none of its slabs was written.
 * Every setting's result is bit-identical to its own fmx_ftrl_dense_run. */
int fmx_ftrl_dense_grid(const double *X, const double *y, int32_t N, int32_t D, int32_t n_settings, const int32_t *m2s, const double *etas,
                        int32_t m2_max, int32_t task, double *w1, double *W2, double *g_w1, double *g_W2, double *pred_out,
                        int32_t *status, fmx_stream_t stream);

/* RRF_Online (reparameterised random Fourier features) on a device-resident stream: per sample x, with eps [D, Ds] fixed,
 *     z = x (e^gamma * eps);  phi = [cos z, sin z];  y_hat = phi . w;  coef = -y (loss 0, logit) or y_hat - y (loss 1, l2);
 *     d_w = lr_w exp(w) + coef phi;  q_d = -sin z_d (coef w_d) + cos z_d (coef w_{Ds+d});
 *     d_gamma_n = (sum_d (x_n eps_nd) q_d) e^gamma_n;  w -= lr_w d_w;  gamma -= lr_gamma d_gamma.
 * fp64, ONE wavefront; eps in LDS, w and gamma in registers.  The device's exp / sin / cos are not the host libm's bit for bit.
 *   X [N, D], y [N];  eps [D, Ds] row-major (read only);  gamma [D], w [2 Ds] are read and written back;  pred_out [N] raw y_hat.
 *   A NaN y_hat leaves gamma and w untouched, writes NaN to that sample's pred_out and the walk goes on (the reference's loop skips
 *   the sample).  status [2] is always written: (number of NaN samples, the first of them or -1).
 * Order: z_d = fma(x_n, e^gamma_n * eps_nd, z_d), n ascending;  y_hat = the sum over lanes d of fma(sin z_d, w_{Ds+d}, cos z_d * w_d)
 * by the xor butterfly d ^ 1, ..., d ^ 32;  the sum of d_gamma_n = fma(x_n * eps_nd, q_d, .), d ascending;  the rest as written.
 * Limits: D <= 64, Ds <= 64, else FMX_ERR_UNSUPPORTED; the hinge and l1 losses are not implemented (FMX_ERR_ARG), as on the host.
 * Replaces: RRF_Online.online_learning (reference models/models_online/RRF_Online.py:70-123, :142-187). */
int fmx_rrf_run(const double *X, const double *y, int32_t N, int32_t D, int32_t Ds, double lr_w, double lr_gamma, int32_t loss,
                const double *eps, double *gamma, double *w, double *pred_out, int32_t *status, fmx_stream_t stream);

/* A GRID of RRF_Online settings over the same stream in one launch (reference RRF_Online.py:18-67 builds one setting per
 * object): workgroup s runs (Dss[s], lr_ws[s], lr_gammas[s]), device arrays of S elements.  Per setting s:
 *   eps [S][D * Ds_max]: setting s's matrix as [D, Dss[s]] row-major at the start of its slot;  gamma [S, D];
 *   w [S][2 * Ds_max]: setting s's 2 Dss[s] weights at the start of its slot;  pred_out [S, N];  status [S, 2].
 *   status[s] = (-2, Dss[s]): Dss[s] lies outside [1, Ds_max]: setting s was not run and none of its slabs was written.  (The
 *   refusal code 2 of the other grids, negated: a setting that ran reports its NaN count, >= 0, in status[s][0].)
 * Every setting's result is bit-identical to its own fmx_rrf_run. */
int fmx_rrf_grid(const double *X, const double *y, int32_t N, int32_t D, int32_t n_settings, const int32_t *Dss, const double *lr_ws,
                 const double *lr_gammas, int32_t Ds_max, int32_t loss, const double *eps, double *gamma, double *w, double *pred_out,
                 int32_t *status, fmx_stream_t stream);

/* ---- top-K recommendation over an FM table's candidates (fmx/recommend.py) ----
 * Replaces: the caller-side loop of forward() over assembled (context, candidate) samples followed by torch.topk; the reference
 * has no counterpart (no recommendation call).  Split a sample's fields into context fields and item fields; then
 *     logit(u + c) = a_u + a_c + <S_u, S_c>
 * with a_u the logit of u's context fields alone (bias included), a_c = sfirst + sbi of c's item fields alone, S_u / S_c their
 * sums of V x -- both come out of fmx_fm_forward with the other side's fields given xv = 0 (fmx/recommend.py).
 *   Su [U, ld_u], au [U]: context sums;  Sc [N, ld_c], ac [N]: candidate sums (ld_u, ld_c multiples of 4, >= kp; Su, Sc
 *   16-byte aligned);  kp 4 / 8 / 16 / 32 / 64;  1 <= K <= 256 (larger: FMX_ERR_UNSUPPORTED).
 *   excl_offsets [U + 1] / excl_pos: per user, the candidate positions never to return, CSR with each user's list ascending
 *   (binary-searched); both null: no exclusions.
 *   top_pos [U, K] int32, top_score [U, K] fp32: each row sorted by score descending, then position ascending (a total order:
 *   the result does not depend on scheduling); rows with fewer than K eligible candidates are padded with -1 / -inf.
 *   A NaN score and an excluded position are never returned; a score of -0 is returned as +0.
 * The score is one fixed function of (u, c), whatever U, N, the tile or the split of the pair:
 *     score(u, c) = (au[u] + ac[c]) + dot,  dot = fma(Su[kp-1], Sc[kp-1], ... fma(Su[1], Sc[1], Su[0] * Sc[0]) ...)
 * (fp32, one rounding per operation, d ascending).  One launch when a user tile's candidates are scanned by one workgroup,
 * else two (scan into per-split partial lists in the workspace, then a merge).  The workspace (16-byte aligned, no
 * initialisation needed) must hold fmx_fm_topk_workspace_bytes(U, N, K) bytes, else FMX_ERR_SHAPE; every argument is
 * checked before anything is launched. */
int64_t fmx_fm_topk_workspace_bytes(int32_t U, int32_t N, int32_t K);
int fmx_fm_topk(const float *Su, int32_t ld_u, const float *au, int32_t U, const float *Sc, int32_t ld_c, const float *ac, int32_t N,
                int32_t kp, const int32_t *excl_offsets, const int32_t *excl_pos, int32_t K, void *workspace, int64_t workspace_bytes,
                int32_t *top_pos, float *top_score, fmx_stream_t stream);

/* ---- top-K recommendation for the classes with an MLP (DeepFM / NFM, fmx/recommend.py) ----
 * Replaces: forward() over assembled (context, candidate) samples followed by torch.topk (reference deepfm_adam.py:79-89,
 * nfm_adam.py:78-88, deepfm_onn.py:88-104, nfm_onn.py:90-104 for the network).  The network does not split over the field
 * split, its input does: with both sides computed alone as for fmx_fm_topk,
 *     bi(u + c) = bi_u + bi_c + S_u (.) S_c
 * so the U x N forwards run on a k-vector built on the device.
 *   mlp: the network (params flat, W_l [hidden, in_l] then b_l [hidden] per layer, in_0 = k); fm_term = 1: DeepFM, 0: NFM
 *   Su, Bu [U, ld_u], au [U]: the contexts' S, bi and base;  Sc, Bc [N, ld_c], ac [N]: the candidates' (Bu / Bc share the
 *   strides of Su / Sc; ld_u, ld_c multiples of 4, >= kp; the four 16-byte aligned).  DeepFM: au = the logit of u alone (bias
 *   in), ac = sfirst_c + sbi_c;  NFM: au = sfirst_u + bias, ac = sfirst_c.
 *   kp, exclusions, K, top_pos / top_score: exactly as fmx_fm_topk (orders, -1 / -inf padding, NaN never returned, -0 as +0).
 * The score is one fixed function of (u, c), whatever U, N, the tile, the split or the candidate order (fp32, one rounding per
 * operation):
 *     x_0[d] = fma(Su[d], Sc[d], Bu[d] + Bc[d])                     d < k (columns k .. kp-1 are not read)
 *     x_l[j] = relu(acc),  acc = fma(x_{l-1}[in-1], W_l[j][in-1], ... fma(x_{l-1}[0], W_l[j][0], b_l[j]) ...)   (i ascending;
 *              relu(v) = v < 0 ? 0 : v, a NaN stays NaN)
 *     sum    = (... ((x_L[0] + x_L[1]) + x_L[2]) ... ) + x_L[hidden-1]
 *     base   = fm_term ? (au[u] + ac[c]) + dot : au[u] + ac[c]      dot: the fma chain of fmx_fm_topk over d < kp
 *     score  = base + sum
 * For the ONN classes this is the logit whose sigmoid forward() returns: the same order, without saturation ties.
 * Limits: kp 4 / 8 / 16 / 32 / 64, 1 <= k <= kp, 1 <= hidden <= 256, 1 <= n_layers <= 8, 1 <= K <= 256; anything outside:
 * FMX_ERR_UNSUPPORTED.  The workspace (16-byte aligned, no initialisation needed) holds a copy of the weights in the kernels'
 * operand order and the partial lists of a split scan: fmx_mlp_topk_workspace_bytes(mlp, U, N, K) bytes (monotone in U, N
 * and K), else FMX_ERR_SHAPE.  Three launches at most (the weight copy, the scan, the merge); every argument is checked before
 * anything is launched. */
int64_t fmx_mlp_topk_workspace_bytes(const fmx_mlp_t *mlp, int32_t U, int32_t N, int32_t K);
int fmx_mlp_topk(const fmx_mlp_t *mlp, int32_t fm_term, const float *Su, const float *Bu, int32_t ld_u, const float *au, int32_t U,
                 const float *Sc, const float *Bc, int32_t ld_c, const float *ac, int32_t N, int32_t kp,
                 const int32_t *excl_offsets, const int32_t *excl_pos, int32_t K, void *workspace, int64_t workspace_bytes,
                 int32_t *top_pos, float *top_score, fmx_stream_t stream);

/* ---- the attentional factorization machine (AFM, Xiao et al. 2017; models/models_online_deep/afm_adam.py) ----
 * Per sample, with e_f = x_f V[row_f] (k floats) and w_f the first-order weight, over the P = F (F - 1) / 2 pairs in the fixed
 * order i = 0 .. F-2, j = i+1 .. F-1:
 *     q_ij = e_i (.) e_j,   s_ij = h . relu(W q_ij + b),   a_ij = softmax over the sample's pairs of s_ij (max-subtracted)
 *     logit = bias + sum_f w_f x_f + p . sum_ij a_ij q_ij
 * params: ONE flat fp32 buffer [ W (t x k, row-major) | b (t) | h (t) | p (k) ] (the reference's attention_linear.weight / .bias,
 * H, P).  Limits: 2 <= n_fields <= 64, k <= 64 (the table's kp), 1 <= t <= 64; anything else: FMX_ERR_UNSUPPORTED.  Tables whose
 * fields are pieces of index columns: FMX_ERR_UNSUPPORTED.  Every sum is taken in a fixed order and no float is accumulated
 * with atomics: results are bit-identical run to run. */
typedef struct fmx_afm {
  float *params;
  int32_t k, t;
} fmx_afm_t;

/* Gather + attention forward: logit_out [B] (may be null); with loss_kind != FMX_LOSS_NONE and y, loss_out [B] = the per-sample
 * loss (unscaled; may be null).  error [1] or null: set to 1 when an index lies outside its field (that row is treated as absent).
 * Replaces: AFMAdam.forward (reference afm_adam.py:43-74), with the loss of :95,116. */
int fmx_afm_forward(const fmx_table_t *table, const fmx_afm_t *afm, const fmx_hyper_t *hyper, const int32_t *idx, const float *xv,
                    const float *y, int32_t B, int32_t loss_kind, float inv_b, float *logit_out, float *loss_out, int32_t *error,
                    fmx_stream_t stream);

/* Bytes of caller-owned device workspace an AFM step of batch size B needs: the table's step workspace (fmx_workspace_bytes), the
 * per-sample dlogit / loss, the per-occurrence embedding gradients [B, F, kp] and the attention partials of the workgroups.  It
 * must be ZERO-FILLED once before its first use, as fmx_workspace_bytes' is.  Negative on bad arguments. */
int64_t fmx_afm_workspace_bytes(const fmx_table_t *table, const fmx_afm_t *afm, int32_t B);

/* One AFM mini-batch step on one stream: occurrence sort -> forward with BCE-with-logits -> backward (per-occurrence embedding
 * gradients, dlogit, per-workgroup attention partials) -> the table update under `rule` (fmx_fm_update_occ) -> the fixed-order
 * reduction of the attention partials.  The attention parameters are NOT updated: attn_grad_out [t k + 2 t + k] receives the
 * gradient of the mean loss (inv_b folded in) in the layout of fmx_afm_t.params.  loss_out [1] = inv_b * sum of the per-sample
 * losses (may be null).  error [1] or null as in fmx_afm_forward.
 * Replaces: the body of AFMAdam.fit's batch loop (reference afm_adam.py:113-118: forward, loss, backward, optimizer.step on the
 * embeddings; the caller applies its rule to the attention parameters). */
int fmx_afm_step(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm, const int32_t *idx,
                 const float *xv, const float *y, int32_t B, float inv_b, void *workspace, int64_t workspace_bytes,
                 float *attn_grad_out, float *loss_out, int32_t *error, fmx_stream_t stream);

/* fmx_afm_step with the attention parameters under a rule of their own, applied inside the fixed-order reduction of the
 * attention partials: the thread that finishes summing column g of the workgroups' partials applies the rule to (params[g],
 * m[g], v[g]) and stores them (no further launch, no atomics).  opt: fmx_mlp_opt_t, with m, v flat fp32 device buffers in the
 * layout of fmx_afm_t.params (t k + 2 t + k floats), 16-byte aligned:
 *   FMX_RULE_SGD       p -= lr * g                                   (m, v may be null)
 *   FMX_RULE_SIGNADAM  p -= lr * g / (|g| + eps)                     (m, v may be null; a fresh Adam's first step.  The AFM calls
 *                                                                    alone take it in fmx_mlp_opt_t; the MLP calls refuse it)
 *   FMX_RULE_ADAGRAD   torch.optim.Adagrad, G in v                   (m may be null)
 *   FMX_RULE_ADAM      torch.optim.Adam as fmx_mlp_opt_t states it.  It is dense: every parameter's moments move on every
 *                      step, a zero gradient (a dead ReLU unit) included
 * The call is step t = opt->step + 1 of the attention parameters; opt->step is read, never written.  attn_grad_out, loss_out,
 * error and every table word (moments and bias words included) are bit-identical to fmx_afm_step on the same inputs: the
 * forward reads the parameters before the step's reduction writes them.
 * Before anything is launched, each naming this entry point in fmx_last_error_string(): fmx_afm_step's checks; opt null, an
 * unknown rule, v null under FMX_RULE_ADAGRAD / FMX_RULE_ADAM, m null under FMX_RULE_ADAM, a beta outside [0, 1), step < 0 or
 * step + 1 beyond int32 (of opt, and of hyper under the tables' FMX_RULE_ADAM): FMX_ERR_ARG; afm->params, m or v not 16-byte
 * aligned: FMX_ERR_ALIGN; the table and batch size as fmx_sort_occurrences checks them.
 * Replaces: the body of AFMAdam.fit's batch loop with the model's ONE persistent optimizer (reference afm_adam.py:93,113-118:
 * forward, loss, backward, optimizer.step) -- SparseAdam's form on the tables, the dense form on the attention parameters. */
int fmx_afm_step_opt(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm, const int32_t *idx,
                     const float *xv, const float *y, int32_t B, float inv_b, void *workspace, int64_t workspace_bytes,
                     float *attn_grad_out, const fmx_mlp_opt_t *opt, float *loss_out, int32_t *error, fmx_stream_t stream);

/* n_steps AFM steps over a device-resident pool, issued from one call without any host synchronisation: idx_pool [n_pool, B, F],
 * xv_pool [n_pool, B, F] or null (ones), y_pool [n_pool, B]; step s takes batch s mod n_pool and is step hyper->step + s + 1 of
 * the tables and opt->step + s + 1 of the attention parameters (both counts are read, never written: the caller advances them
 * by n_steps).  ADAM's constants of a step are computed on the host in double, once per step.  loss_out [n_steps] or null
 * receives each step's mean loss; attn_grad_out holds the last step's gradient.  workspace: fmx_afm_workspace_bytes(table, afm,
 * B) bytes (every batch is sorted on `stream` in front of its step; nothing is sorted ahead).  error [1] or null: set when any
 * index of any step lies outside its field.
 * The result is, bit for bit, the one of n_steps calls of fmx_afm_step_opt with both step counts advanced by the caller: rows,
 * moments, bias words, params, m, v and the per-step losses.  Every argument is checked before the first launch --
 * fmx_afm_step_opt's checks with step + n_steps within int32, n_pool >= 1, n_steps >= 0 -- and n_steps = 0 launches nothing.
 * Replaces: AFMAdam.fit's loop over the batches of an epoch (reference afm_adam.py:98-141, with the optimizer of :93). */
int fmx_afm_stream(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm, const int32_t *idx_pool,
                   const float *xv_pool, const float *y_pool, int32_t n_pool, int32_t B, float inv_b, int32_t n_steps, void *workspace,
                   int64_t workspace_bytes, float *attn_grad_out, const fmx_mlp_opt_t *opt, float *loss_out, int32_t *error,
                   fmx_stream_t stream);

/* The online predict-then-fit loop of the AFM on a device-resident stream, in one call: idx [N, F], xv [N, F] or null (ones),
 * y [N].  Sample i is predicted and then fitted on, one sample at a time: the call is N steps of fmx_afm_step_opt with B = 1 and
 * inv_b = 1, sample i being step hyper->step + i + 1 of the tables and step opt->step + i + 1 of the attention parameters (both
 * counts are read, never written: the caller advances them by N).  logit_out [N] or null receives each sample's logit under the
 * weights BEFORE its update (predict and fit share one forward); loss_out [N] or null its BCE-with-logits loss; attn_grad_out
 * [t k + 2 t + k] holds the last sample's attention gradient; error [1] or null is set to 1 when any index of the stream lies
 * outside its field (that row is absent for its sample; the walk goes on).  rule / opt->rule: every table rule fmx_afm_step_opt
 * takes, with its layout, and FMX_RULE_SGD / FMX_RULE_SIGNADAM / FMX_RULE_ADAGRAD / FMX_RULE_ADAM on the attention parameters.
 * workspace: fmx_afm_workspace_bytes(table, afm, 1) bytes.
 * One workgroup walks the stream and spreads each sample over its waves: the attention parameters (and their moments where they
 * fit) stay in LDS until the end of the stream, the bias words too; ADAM's constants of a sample are derived on the device by
 * the function the host uses for a launch.  A shape that does not leave room in the CU's 160 KiB of LDS for two pair tiles'
 * buffers beside the sample (the largest F, k and t together), or fmx_set_option("afm_online_persistent", 0), takes the
 * per-sample launches of fmx_afm_step_opt instead, queued without any host synchronisation.  No float is accumulated with
 * atomics; the result is deterministic run to run.
 * The result is, bit for bit, the one of N calls of fmx_afm_step_opt(B = 1, inv_b = 1) with both step counts advanced by the
 * caller, in either form: rows (moments and FTRL state included), bias words, params, m, v, the per-sample logits and losses,
 * the last attn_grad_out and the error word.
 * Limits: those of fmx_afm_step_opt (every shape it accepts is accepted).  Every argument is checked before the first launch,
 * each failure naming this entry point in fmx_last_error_string(): fmx_afm_step_opt's checks, with N < 0 and step + N beyond
 * int32 (of opt, and of hyper under the tables' FMX_RULE_ADAM): FMX_ERR_ARG; workspace_bytes too small: FMX_ERR_SHAPE; tables
 * whose fields are pieces of index columns: FMX_ERR_UNSUPPORTED.  N = 0 launches nothing and returns 0.
 * Replaces: a loop over the samples of AFMAdam.predict (reference afm_adam.py:170-191) followed by one fit step on the sample
 * (:113-118) -- the protocol of the other classes' run_experiment (reference fm_adam.py:90-119), which the reference's AFM lacks. */
int fmx_afm_online_run(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm, const int32_t *idx,
                       const float *xv, const float *y, int32_t N, void *workspace, int64_t workspace_bytes, float *attn_grad_out,
                       const fmx_mlp_opt_t *opt, float *logit_out, float *loss_out, int32_t *error, fmx_stream_t stream);

/* ---- pairwise-ranking (BPR) training of the AFM: the pair loss on the full attentional logit ----
 * The layout is fmx_fm_pair_forward's: B_pairs pairs are idx [2 B_pairs, F] (xv the same shape, or null: ones), row 2i the
 * positive sample of pair i and row 2i + 1 its negative, both full-width rows (typically the positive's row with the item columns
 * replaced; nothing assumes that).  With d_i = z[2i] - z[2i + 1] over the logit of fmx_afm_forward the loss is
 * loss_i = -log(sigmoid(d_i) + margin); margin 0 is BPR.  dL/dlogit of a row depends on its partner's logit, so one workgroup owns
 * the PAIR: it walks the pairs blockIdx.x, blockIdx.x + gridDim.x, ... and per pair runs the negative's forward, the positive's
 * forward, the loss, the positive's backward, then the negative's forward again (the same bits: the LDS has no room for two rows
 * at the largest shape) and its backward.
 * Order of the sums: the attention accumulators [ dW | db | dh | dp ] of a workgroup take a pair's positive tiles first, then its
 * negative tiles, each in the pair order of fmx_afm_step; pairs in the workgroup's walk order; the workgroups' partials in
 * workgroup order.  No float is accumulated with atomics; every sum has one fixed order that depends on (B_pairs, F, t, k) alone.
 * The table update is fmx_fm_update_occ on the 2 B_pairs rows: a row both samples of a pair name is a run of two occurrences, and
 * the bias gradient is the sum of dz, exactly +0 (dz[2i + 1] is dz[2i] negated): the bias word keeps its bits under every rule
 * but FMX_RULE_ADAM, where it moves along its decayed moments alone.
 * workspace of the step calls: fmx_afm_workspace_bytes(table, afm, 2 * B_pairs) bytes -- it covers dz, loss and E of the 2 B_pairs
 * rows and more partials than the pair launch's workgroups write (smaller: FMX_ERR_SHAPE; not 16-byte aligned: FMX_ERR_ALIGN).
 * Refused before anything is launched, each message naming the entry point: a null table / afm / hyper / idx / workspace /
 * attn_grad_out / opt, B_pairs < 1, 2 * B_pairs beyond int32, a negative / NaN / infinite margin: FMX_ERR_ARG; then what
 * fmx_afm_step / fmx_afm_step_opt refuse for 2 * B_pairs rows (the AFM's limits, the rule against the layout, the attention
 * rule's state, FMX_RULE_ADAM's hyper-parameters, the sort's geometry).  error [1] or null: set to 1 when an index lies outside
 * its field; that row is treated as absent, as in fmx_afm_step.
 * Restates: the pair objective of reference models/models_meta_emb/meta_fm.py:145-169 for the AFM logit. */

/* The forward pass of the 2 B_pairs rows with the pair epilogue.  logit_out [2 B_pairs]: the bits fmx_afm_forward(FMX_LOSS_NONE)
 * gives on the same rows; loss_out [2 B_pairs]: loss[2i] = loss_i (unscaled), loss[2i + 1] = +0; dz_out [2 B_pairs]:
 * dz[2i] = inv_b * d loss_i / d d_i, dz[2i + 1] = the same float negated.  Each of the three may be null.
 * Replaces: the forward and loss of the reference's pair objective (meta_fm.py:145-169) on AFMAdam.forward (afm_adam.py:43-74). */
int fmx_afm_pair_forward(const fmx_table_t *table, const fmx_afm_t *afm, const fmx_hyper_t *hyper, const int32_t *idx, const float *xv,
                         int32_t B_pairs, float margin, float inv_b, float *logit_out, float *loss_out, float *dz_out, int32_t *error,
                         fmx_stream_t stream);

/* One pair step on one stream: fmx_sort_occurrences(2 B_pairs) -> pair forward + backward -> fmx_fm_update_occ(2 B_pairs) under
 * `rule` -> the fixed-order reduction of the attention partials.  The attention parameters are NOT updated: attn_grad_out
 * [t k + 2 t + k] receives the gradient of inv_b * sum_i loss_i.  logit_out [2 B_pairs] or null: the logits before the update;
 * loss_out [1] = inv_b * sum_i loss_i (may be null).
 * Replaces: fmx_afm_step's BCE by the reference's pair objective (meta_fm.py:145-169): forward, loss, backward, the embeddings'
 * optimizer.step. */
int fmx_afm_pair_step(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm, const int32_t *idx,
                      const float *xv, int32_t B_pairs, float margin, float inv_b, void *workspace, int64_t workspace_bytes,
                      float *attn_grad_out, float *logit_out, float *loss_out, int32_t *error, fmx_stream_t stream);

/* fmx_afm_pair_step with the attention parameters under opt's rule inside the reduction, as fmx_afm_step_opt: the call is step
 * opt->step + 1 of the attention parameters (read, never written).  attn_grad_out, logit_out, loss_out, error and every table word
 * are bit-identical to fmx_afm_pair_step on the same inputs.
 * Replaces: fmx_afm_step_opt's BCE by the reference's pair objective (meta_fm.py:145-169) under the model's one optimizer. */
int fmx_afm_pair_step_opt(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm, const int32_t *idx,
                          const float *xv, int32_t B_pairs, float margin, float inv_b, void *workspace, int64_t workspace_bytes,
                          float *attn_grad_out, const fmx_mlp_opt_t *opt, float *logit_out, float *loss_out, int32_t *error,
                          fmx_stream_t stream);

/* n_steps pair steps over a device-resident pool idx_pool [n_pool, 2 B_pairs, F] (xv_pool the same shape, or null), issued from
 * one call as a plain queue of launches without any host synchronisation, as fmx_afm_stream: step s takes batch s mod n_pool and
 * is step hyper->step + s + 1 of the tables and opt->step + s + 1 of the attention parameters.  loss_out [n_steps] or null.
 * Also refused: n_pool < 1, n_steps < 0, step + n_steps beyond int32: FMX_ERR_ARG; n_steps = 0 launches nothing.
 * The result is, bit for bit, the one of n_steps calls of fmx_afm_pair_step_opt with both step counts advanced by the caller.
 * Replaces: fmx_afm_stream's BCE by the reference's pair objective (meta_fm.py:145-169), batched as AFMAdam.fit batches. */
int fmx_afm_pair_stream(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm, const int32_t *idx_pool,
                        const float *xv_pool, int32_t n_pool, int32_t B_pairs, float margin, float inv_b, int32_t n_steps,
                        void *workspace, int64_t workspace_bytes, float *attn_grad_out, const fmx_mlp_opt_t *opt, float *loss_out,
                        int32_t *error, fmx_stream_t stream);

/* The online predict-then-fit protocol restated for pairs on N_pairs device-resident pairs idx [2 N_pairs, F]: every pair is
 * predicted, then fitted on alone.  The contract: bit for bit N_pairs calls of fmx_afm_pair_step_opt(B_pairs = 1, inv_b = 1), pair
 * i being step hyper->step + i + 1 of the tables and opt->step + i + 1 of the attention parameters (both read, never written).
 * logit_out [2 N_pairs] or null: each pair's two logits BEFORE its update (the prediction is logit[2i] > logit[2i + 1]); loss_out
 * [N_pairs] or null: each pair's loss.  workspace: fmx_afm_workspace_bytes(table, afm, 2) bytes.  N_pairs < 0: FMX_ERR_ARG;
 * N_pairs = 0 launches nothing and returns 0.  Two forms, the same bits: one workgroup of 8 waves walks the stream with the
 * attention parameters resident in LDS (k_afm_pair_online, as fmx_afm_online_run's kernel) wherever at least min(2, tiles) tile
 * buffers fit beside a sample; otherwise, or under fmx_set_option("afm_pair_online_persistent", 0), the pairs' launches are queued
 * without any host synchronisation.  fmx_afm_pair_online_form says which form a shape takes.
 * Replaces: the protocol of reference fm_adam.py:90-119 under the pair objective of meta_fm.py:145-169, for the AFM. */
int fmx_afm_pair_online_run(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm, const int32_t *idx,
                            const float *xv, int32_t N_pairs, float margin, void *workspace, int64_t workspace_bytes,
                            float *attn_grad_out, const fmx_mlp_opt_t *opt, float *logit_out, float *loss_out, int32_t *error,
                            fmx_stream_t stream);

/* Which form fmx_afm_pair_online_run takes for this table and these attention parameters under the attention rule attn_rule
 * (FMX_RULE_SIGNADAM, FMX_RULE_SGD, FMX_RULE_ADAGRAD or FMX_RULE_ADAM; another: FMX_ERR_ARG): the number of tile buffers of the
 * one-workgroup kernel (> 0), or 0 for the queued pair steps (the shape leaves no room, or the option
 * "afm_pair_online_persistent" is 0).  moments_in_lds (or null) receives 1 when the attention moments stay in LDS for the call,
 * 0 when they stay in global memory or the rule has none.  The structs' shapes are read; no pointer in them is dereferenced and
 * no device call is made.  The table and the attention parameters are refused as fmx_afm_pair_online_run refuses them.
 * Replaces: nothing in the reference.  Restates: the dispatch of fmx_afm_pair_online_run, for callers and tests that must know
 * which kernel a result came from. */
int fmx_afm_pair_online_form(const fmx_table_t *table, const fmx_afm_t *afm, int32_t attn_rule, int32_t *moments_in_lds);

/* ---- listwise (sampled-softmax) training of the attentional FM: one positive, G - 1 negatives ----
 * The objective and the layout are fmx_fm_list_*'s (above fmx_fm_list_workspace_bytes) over the FULL attentional logit: a batch of
 * B_lists lists of G rows (2 <= G <= 16) is idx [B_lists G, F] (xv of the same shape, or null: ones), row G i the positive of list
 * i, rows G i + 1 .. G i + G - 1 its negatives; z_j is the logit fmx_afm_forward gives row G i + j (its bits), and
 *     loss_i = log sum_j exp(z_j - m) - (z_0 - m),   dz_j = p_j inv_b (j >= 1),   dz_0 = -(sum_{j>=1} p_j) inv_b
 * evaluated by the FM family's own formula on the same operands in the same order.  One workgroup of one wavefront owns a list
 * (k_afm_list): the negatives' forwards, then the positive's, the loss once, then the positive's backward and, after each
 * negative's forward AGAIN, its backward -- the recomputation of fmx_afm_pair_*, for its reason.
 * Order of the sums: the attention accumulators [ dW | db | dh | dp ] of a workgroup take a list's positive tiles first, then its
 * negatives' tiles in row order, each in the pair order of fmx_afm_step; lists in the workgroup's walk order; the workgroups'
 * partials in workgroup order.  No float is accumulated with atomics; every sum has one fixed order that depends on
 * (B_lists, G, F, t, k) alone.
 * The bias: as in fmx_fm_list_*, the table update's bias rule runs on 16 scratch bytes behind the step workspace; the forward reads
 * the real bias, and the bias and its state (z / n, moments) are BIT-UNCHANGED under every rule, FMX_RULE_ADAM included.
 * Refused before anything is launched, each message naming the entry point: fmx_fm_list_*'s shared refusals (a null table / hyper /
 * idx, B_lists < 1, G < 2, B_lists G beyond int32: FMX_ERR_ARG; G > 16 and tables whose fields are pieces of index columns:
 * FMX_ERR_UNSUPPORTED); then what fmx_afm_step / fmx_afm_step_opt refuse for B_lists G rows (the AFM's limits, a null workspace /
 * attn_grad_out / opt, the rule against the layout, the workspace's size and alignment, the attention rule's state,
 * FMX_RULE_ADAM's hyper-parameters, the sort's geometry).  error [1] or null: set to 1 when an index lies outside its field; that
 * row is treated as absent, as in fmx_afm_step.
 * Replaces: nothing -- the reference has no listwise loss.  Its nearest counterpart is the pair objective of reference
 * models/models_meta_emb/meta_fm.py:145-169, which this generalises from one negative to G - 1 for the AFM logit. */

/* Bytes of caller-owned device workspace a list step of B_lists lists of G rows needs: fmx_afm_workspace_bytes(table, afm,
 * B_lists G) plus the 16 scratch bytes the bias rule runs on (at the end; 16-byte aligned).  Negative on a bad table or afm,
 * B_lists < 1, G outside [2, 16] or B_lists G beyond int32.
 * Replaces: nothing in the reference (nearest: meta_fm.py:145-169).  Restates: fmx_fm_list_workspace_bytes for the AFM step. */
int64_t fmx_afm_list_workspace_bytes(const fmx_table_t *table, const fmx_afm_t *afm, int32_t B_lists, int32_t G);

/* The forward pass of the B_lists G rows with the list epilogue.  logit_out [B_lists G]: the bits fmx_afm_forward(FMX_LOSS_NONE)
 * gives on the same rows; loss_out [B_lists G]: loss[G i] = loss_i (unscaled), loss[G i + j] = +0 for j >= 1; dz_out [B_lists G]:
 * dz[G i + j] = dz_j as above.  Each of the three may be null.
 * Replaces: nothing in the reference, which has no listwise loss; nearest: the forward and loss of the pair objective
 * (meta_fm.py:145-169) on AFMAdam.forward (afm_adam.py:43-74). */
int fmx_afm_list_forward(const fmx_table_t *table, const fmx_afm_t *afm, const fmx_hyper_t *hyper, const int32_t *idx, const float *xv,
                         int32_t B_lists, int32_t G, float inv_b, float *logit_out, float *loss_out, float *dz_out, int32_t *error,
                         fmx_stream_t stream);

/* One list step on one stream: fmx_sort_occurrences(B_lists G) -> list forward + backward -> fmx_fm_update_occ(B_lists G) under
 * `rule` (its bias rule on the scratch) -> the fixed-order reduction of the attention partials.  The attention parameters are NOT
 * updated: attn_grad_out [t k + 2 t + k] receives the gradient of inv_b * sum_i loss_i.  logit_out [B_lists G] or null: the logits
 * before the update; loss_out [1] = inv_b * sum_i loss_i (may be null).  workspace: fmx_afm_list_workspace_bytes bytes.
 * Replaces: nothing in the reference; nearest: fmx_afm_pair_step's objective (meta_fm.py:145-169) with G - 1 negatives. */
int fmx_afm_list_step(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm, const int32_t *idx,
                      const float *xv, int32_t B_lists, int32_t G, float inv_b, void *workspace, int64_t workspace_bytes,
                      float *attn_grad_out, float *logit_out, float *loss_out, int32_t *error, fmx_stream_t stream);

/* fmx_afm_list_step with the attention parameters under opt's rule inside the reduction, as fmx_afm_step_opt: the call is step
 * opt->step + 1 of the attention parameters (read, never written).  attn_grad_out, logit_out, loss_out, error and every table word
 * are bit-identical to fmx_afm_list_step on the same inputs.
 * Replaces: nothing in the reference; nearest: fmx_afm_pair_step_opt's objective (meta_fm.py:145-169) with G - 1 negatives. */
int fmx_afm_list_step_opt(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm, const int32_t *idx,
                          const float *xv, int32_t B_lists, int32_t G, float inv_b, void *workspace, int64_t workspace_bytes,
                          float *attn_grad_out, const fmx_mlp_opt_t *opt, float *logit_out, float *loss_out, int32_t *error,
                          fmx_stream_t stream);

/* n_steps list steps over a device-resident pool idx_pool [n_pool, B_lists G, F] (xv_pool the same shape, or null), issued from one
 * call as a plain queue of launches without any host synchronisation, as fmx_afm_pair_stream: step s takes batch s mod n_pool and
 * is step hyper->step + s + 1 of the tables and opt->step + s + 1 of the attention parameters.  loss_out [n_steps] or null.
 * Also refused: n_pool < 1, n_steps < 0, step + n_steps beyond int32: FMX_ERR_ARG; n_steps = 0 launches nothing.
 * The result is, bit for bit, the one of n_steps calls of fmx_afm_list_step_opt with both step counts advanced by the caller.
 * Replaces: nothing in the reference; nearest: fmx_afm_pair_stream's objective (meta_fm.py:145-169) with G - 1 negatives. */
int fmx_afm_list_stream(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm, const int32_t *idx_pool,
                        const float *xv_pool, int32_t n_pool, int32_t B_lists, int32_t G, float inv_b, int32_t n_steps, void *workspace,
                        int64_t workspace_bytes, float *attn_grad_out, const fmx_mlp_opt_t *opt, float *loss_out, int32_t *error,
                        fmx_stream_t stream);

/* The online predict-then-fit protocol restated for lists on N device-resident lists idx [N G, F]: every list is predicted, then
 * fitted on alone.  The contract: bit for bit N calls of fmx_afm_list_step_opt(B_lists = 1, inv_b = 1), list i being step
 * hyper->step + i + 1 of the tables and opt->step + i + 1 of the attention parameters (both read, never written).  logit_out [N G]
 * or null: each list's logits BEFORE its update (the positive is ranked first when no negative's logit is >= logit[G i]); loss_out
 * [N] or null: each list's loss.  workspace: fmx_afm_list_workspace_bytes(table, afm, 1, G) bytes.  N < 0: FMX_ERR_ARG; N = 0
 * launches nothing and returns 0 (the buffers may be null).  One form: the lists' step launches queued without any host
 * synchronisation (there is no one-workgroup walker for lists).
 * Replaces: nothing in the reference; nearest: the protocol of fm_adam.py:90-119 under the pair objective of meta_fm.py:145-169. */
int fmx_afm_list_online_run(const fmx_table_t *table, const fmx_hyper_t *hyper, int32_t rule, const fmx_afm_t *afm, const int32_t *idx,
                            const float *xv, int32_t N, int32_t G, void *workspace, int64_t workspace_bytes, float *attn_grad_out,
                            const fmx_mlp_opt_t *opt, float *logit_out, float *loss_out, int32_t *error, fmx_stream_t stream);

/* ---- top-K recommendation under the AFM (fmx/recommend.py, AFMAdam.recommend) ----
 * Split the fields into context fields C and item fields I (at least one of each).  A combined sample's pairs are the C x C
 * pairs (u alone), the I x I pairs (c alone) and the |C| |I| cross pairs.  Each side's own pairs reduce to (lin, m, Z, R):
 * lin = the first-order sum (plus the bias on the context side), m = max s, Z = sum e^(s - m), R = sum e^(s - m) (p . q).
 * A side of one field has no pairs: m = -inf, Z = R = 0, and it adds exact zeros.  The other side's fields are NOT zeroed:
 * a zero field would still add pairs to the softmax.
 *
 * fmx_afm_side: (lin, m, Z, R) and the gathered embeddings of the n_sel selected fields of R full-width rows.
 *   idx / xv [R, F] (xv may be null: ones); fields: a HOST array of n_sel ascending field numbers; with_bias: 1 adds the
 *   table's bias to lin (the context side), 0 does not (the item side).
 *   E_out [R, n_sel, kp] = x V[row] of the selected fields (kp floats, as k_afm gathers them); stats_out [R, 4] = (lin, m, Z, R)
 *   over the selected fields' own pairs in the AFM's pair order, with fmx_afm_forward's arithmetic: lin = bias + w-sum (or the
 *   w-sum alone), m = the max, Z and R its max-subtracted sums.  Both 16-byte aligned.  error as in fmx_afm_forward.  A row's
 *   results do not depend on R or on the other rows; every table layout gives the weights fmx_afm_forward uses.
 * Replaces: nothing in the reference (it has no recommendation call); the AFM counterpart of fmx_fm_forward's masked sides. */
int fmx_afm_side(const fmx_table_t *table, const fmx_afm_t *afm, const fmx_hyper_t *hyper, const int32_t *idx, const float *xv,
                 int32_t R, const int32_t *fields, int32_t n_sel, int32_t with_bias, float *E_out, float *stats_out, int32_t *error,
                 fmx_stream_t stream);

/* fmx_afm_topk: exact top-K of the AFM logit over U contexts x N candidates.
 * Replaces: forward() over assembled (context, candidate) samples followed by torch.topk (reference afm_adam.py:43-74 for
 * the model).
 *   Eu [U, n_ctx, kp], stats_u [U, 4]: the contexts' fmx_afm_side with with_bias = 1;  Ec [N, n_item, kp], stats_c [N, 4]: the
 *   candidates' with with_bias = 0 (all four 16-byte aligned, rows dense).  afm: the parameters of fmx_afm_forward.
 *   kp, exclusions, K, top_pos / top_score: exactly as fmx_fm_topk (rows sorted by score descending then position ascending,
 *   -1 / -inf padding, a NaN score or an excluded position never returned, -0 returned as +0).
 * The score is one fixed function of (u, c), whatever U, N, the split or the candidate order (fp32, one rounding per operation):
 *     cross pairs in the order j = item field ascending, then i = context field ascending:
 *       q[d] = Eu[u][i][d] * Ec[c][j][d]                                    d < kp
 *       r    = fma(p[kp-1], q[kp-1], ... fma(p[0], q[0], 0) ...)             (p zero-padded past k)
 *       z_v  = fma(W[v][kp-1], q[kp-1], ... fma(W[v][0], q[0], b[v]) ...)    (W rows zero-padded past k)
 *       s    = fma(h[t-1], max(z_{t-1}, 0), ... fma(h[0], max(z_0, 0), 0) ...)
 *     folded into (mx, Zx, Rx), starting from (-inf, 0, 0), by online rescaling:
 *       s > mx:  e = exp(mx - s), Zx = fma(Zx, e, 1), Rx = fma(Rx, e, r), mx = s
 *       else:    e = exp(s - mx), Zx = Zx + e,        Rx = fma(e, r, Rx)
 *     M  = fmaxf(fmaxf(m_u, m_c), mx);  e_u = exp(m_u - M), e_c = exp(m_c - M), e_x = exp(mx - M)
 *     Z  = fma(Zx, e_x, fma(Z_c, e_c, Z_u * e_u)),  R = fma(Rx, e_x, fma(R_c, e_c, R_u * e_u))
 *     score = (lin_u + lin_c) + R / Z
 * It agrees with fmx_afm_forward on the assembled sample up to the order of the softmax's sums.
 * Limits: kp 4 / 8 / 16 / 32 / 64 and >= k, else FMX_ERR_SHAPE; n_ctx, n_item >= 1, else FMX_ERR_SHAPE; 1 <= t <= 64,
 * n_ctx + n_item <= 64, K <= 256, else FMX_ERR_UNSUPPORTED; U, N, K >= 1, else FMX_ERR_ARG.  The workspace (16-byte aligned, no
 * initialisation needed) holds the attention parameters padded to kp and the partial lists of a split scan:
 * fmx_afm_topk_workspace_bytes(afm, n_ctx, n_item, U, N, K) bytes (monotone in U, N and K, computed on the host; negative on
 * bad arguments), else FMX_ERR_SHAPE.  Three launches (the padded copy, the scan, the merge of the splits when there are
 * several); every argument is checked before anything is launched. */
int64_t fmx_afm_topk_workspace_bytes(const fmx_afm_t *afm, int32_t n_ctx, int32_t n_item, int32_t U, int32_t N, int32_t K);
int fmx_afm_topk(const fmx_afm_t *afm, const float *Eu, const float *stats_u, int32_t n_ctx, int32_t U, const float *Ec,
                 const float *stats_c, int32_t n_item, int32_t N, int32_t kp, const int32_t *excl_offsets, const int32_t *excl_pos,
                 int32_t K, void *workspace, int64_t workspace_bytes, int32_t *top_pos, float *top_score, fmx_stream_t stream);

/* ---- exact ranking evaluation: the rank of held-out targets among all candidates (fmx/recommend.py) ----
 * Replaces: recommending K = 256 and hoping the held-out item is inside, or forward() over U x N assembled samples followed
 * by a comparison count; the reference has no counterpart (utils/metric_manager.py keeps classification counts only).
 * One call per scoring family.  Each takes the arguments of the family's top-K call, with the same meaning and the same
 * limits (kp, k, hidden <= 256, n_layers <= 8, the AFM's t, n_ctx and n_item bounds), and K, top_pos, top_score replaced by
 *   targets [U, T] int32: candidate positions, 1 <= T <= 16 (larger: FMX_ERR_UNSUPPORTED; T < 1: FMX_ERR_ARG);  filtered: 0 or 1
 *   rank_out [U, T] int32;  score_out [U, T] fp32, may be null;  n_cand_out [U] int32, may be null.
 * Score: score(u, c) is the fixed function stated at the family's top-K call above (see there for the formula).  It gives the
 * same bits for a pair whatever U, N, T, the tile or the split, and the same bits that top-K call computes: the device code
 * of the score is shared, not restated.
 * Eligibility: candidate c is eligible for user u when 0 <= c < N, score(u, c) is not NaN and c is not in u's exclusion list --
 * exactly the candidates the top-K call may return.  n_cand_out[u] is their number.
 * Targets: a target p that is not eligible (-1 padding, p >= N, excluded, NaN score) gets rank -1 and score -inf.  Otherwise
 * score_out[u, t] = score(u, p) with -0 returned as +0, and rank_out[u, t] = the number of eligible c whose key is greater
 * than p's in the top-K order (score descending, then position ascending, -0 taken as +0): the 0-based index p would have in
 * an unbounded top-K row.  Hence p sits at index r of the family's top-K row exactly when rank = r < K.  filtered = 1: the
 * user's other eligible targets are not counted (the filtered rank of leave-n-out evaluation); filtered = 0: they count like
 * any candidate, and a target listed twice gets the same rank twice.
 * The workspace (16-byte aligned, no initialisation needed; the outputs need none either) holds the targets' keys and the
 * per-split partial counts, after the family's parameter copy: *_rank_workspace_bytes bytes (int64, monotone in U, N and T,
 * negative on bad sizes), else FMX_ERR_SHAPE.  Every argument is checked before anything is launched, with the codes the
 * top-K call returns for the same mistake.  Asynchronous on `stream`, safe under graph capture; the counts are integers, so the
 * result is identical run to run.  Launches: the parameter copy (network, AFM), the targets' keys, the counting scan, the
 * finishing step. */
int64_t fmx_fm_rank_workspace_bytes(int32_t U, int32_t N, int32_t T);
int fmx_fm_rank(const float *Su, int32_t ld_u, const float *au, int32_t U, const float *Sc, int32_t ld_c, const float *ac, int32_t N,
                int32_t kp, const int32_t *excl_offsets, const int32_t *excl_pos, const int32_t *targets, int32_t T, int32_t filtered,
                void *workspace, int64_t workspace_bytes, int32_t *rank_out, float *score_out, int32_t *n_cand_out,
                fmx_stream_t stream);
int64_t fmx_mlp_rank_workspace_bytes(const fmx_mlp_t *mlp, int32_t U, int32_t N, int32_t T);
int fmx_mlp_rank(const fmx_mlp_t *mlp, int32_t fm_term, const float *Su, const float *Bu, int32_t ld_u, const float *au, int32_t U,
                 const float *Sc, const float *Bc, int32_t ld_c, const float *ac, int32_t N, int32_t kp,
                 const int32_t *excl_offsets, const int32_t *excl_pos, const int32_t *targets, int32_t T, int32_t filtered,
                 void *workspace, int64_t workspace_bytes, int32_t *rank_out, float *score_out, int32_t *n_cand_out,
                 fmx_stream_t stream);
int64_t fmx_afm_rank_workspace_bytes(const fmx_afm_t *afm, int32_t n_ctx, int32_t n_item, int32_t U, int32_t N, int32_t T);
int fmx_afm_rank(const fmx_afm_t *afm, const float *Eu, const float *stats_u, int32_t n_ctx, int32_t U, const float *Ec,
                 const float *stats_c, int32_t n_item, int32_t N, int32_t kp, const int32_t *excl_offsets, const int32_t *excl_pos,
                 const int32_t *targets, int32_t T, int32_t filtered, void *workspace, int64_t workspace_bytes, int32_t *rank_out,
                 float *score_out, int32_t *n_cand_out, fmx_stream_t stream);

/* ---- hard negatives for pairwise (BPR) training: the best of n_draw drawn candidates per user (fmx/pairwise.py) ----
 * Replaces: uniform negatives (torch.randint with a redraw loop that reads a count back per round) followed, for dynamic
 * negative sampling (Zhang et al. 2013; Rendle & Freudenthaler 2014), by n_draw assembled forwards per positive and torch.max;
 * the reference has no counterpart (meta_fm.py:145-169 takes its negatives as given).
 *   Su, ld_u, au, U, Sc, ld_c, ac, N, kp, excl_offsets / excl_pos: exactly as fmx_fm_topk.  No workspace.
 *   own_pos [U] int32 or null: the position of the user's own (positive) item, never returned; -1: none.
 *   neg_pos [U, n_neg] int32, neg_score [U, n_neg] fp32.
 * Draws.  Draw j (0 <= j < n_draw) of user u is word j & 3 of Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl
 * constants 0x9E3779B9 / 0xBB67AE85) with
 *     key     = (seed & 0xffffffff, seed >> 32)
 *     counter = (offset & 0xffffffff, offset >> 32, (u_base + u) mod 2^32, j >> 2)
 * and the drawn position is (uint64(word) * N) >> 32: uniform over [0, N) up to a bias of at most N / 2^32 per position.  A
 * user's draws depend on (seed, offset, u_base + u, N) only -- not on U, nor on how a batch is cut into calls.
 * Eligibility.  A draw is eligible when its score is not NaN, its position is not own_pos[u], its position is not in the
 * user's exclusion list, and its position was not counted already (a position drawn twice counts once).
 * Score.  score(u, c) of fmx_fm_topk, the same bits: the device code of the score is shared, not restated.
 * Result.  Row u holds the n_neg best eligible drawn positions in fmx_fm_topk's order (score descending, then position
 * ascending, -0 returned as +0), padded with -1 / -inf: by definition what fmx_fm_topk with K = n_neg returns over the set of
 * that user's drawn, non-own candidates.
 * Limits.  kp 4 / 8 / 16 / 32 / 64, n_draw <= 1024, n_neg <= 16, else FMX_ERR_UNSUPPORTED; U, N, n_draw, n_neg >= 1 and
 * n_neg <= n_draw, non-null Su / au / Sc / ac / outputs, excl_offsets and excl_pos together, else FMX_ERR_ARG; ld_u, ld_c
 * multiples of 4 and Su, Sc 16-byte aligned, else FMX_ERR_ALIGN; ld_u, ld_c >= kp, else FMX_ERR_SHAPE.  Every argument is
 * checked before anything is launched.  One launch (a wavefront per user), asynchronous on `stream`, safe under graph
 * capture; no atomics and a total order, so the result is identical run to run. */
int fmx_fm_mine_negatives(const float *Su, int32_t ld_u, const float *au, int32_t U, const float *Sc, int32_t ld_c, const float *ac,
                          int32_t N, int32_t kp, const int32_t *excl_offsets, const int32_t *excl_pos, const int32_t *own_pos,
                          int32_t n_draw, int32_t n_neg, uint64_t seed, uint64_t offset, uint32_t u_base, int32_t *neg_pos,
                          float *neg_score, fmx_stream_t stream);

/* ---- popularity-sampled negatives: draws from an alias table, with log Q of every draw (fmx/pairwise.py) ----
 * Replaces: torch.multinomial(weights, n_neg, replacement=True) per batch, a redraw loop for the rows that drew their own item
 * (one count read back per round) and a gather of log q; the reference has no counterpart (meta_fm.py:145-169 takes its negatives
 * as given).  The cheap middle between uniform negatives, nearly all trivial on a long-tailed catalogue, and mined ones
 * (fmx_fm_mine_negatives), which cost a scoring pass.
 * Table (Walker's alias method, built on the host: fmx.pairwise.alias_table).  thresh [N] uint32 in [0, 2^24], alias [N] int32 in
 * [0, N), logq [N] fp32: the log of the REALISED probability of each position,
 *     q_i = (thresh_i + sum_{j: alias_j = i} (2^24 - thresh_j)) / (N 2^24),
 * or null (then neg_logq must be null too).
 * Draws.  Draw t (0 <= t < n_try) of row u takes two words of one Philox4x32-10 block (fmx_fm_mine_negatives' multipliers and Weyl
 * constants) with
 *     key     = (seed & 0xffffffff, seed >> 32)
 *     counter = (offset & 0xffffffff, offset >> 32, (u_base + u) mod 2^32, 0x80000000 + (t >> 1))
 *     a = word 2 (t & 1),  b = word 2 (t & 1) + 1,  p = (uint64(a) * N) >> 32,  position = (b >> 8) < thresh[p] ? p : alias[p]
 * The high bit of the fourth counter word keeps these streams apart from fmx_fm_mine_negatives' under the same (seed, offset).  p is
 * uniform over [0, N) up to the bias of at most N / 2^32 per position stated above; q is the law of a draw up to that bias.
 * Eligibility.  A draw is eligible when its position is not own_pos[u] (int32 [U] or null; -1: none), is not in the row's exclusion
 * list (excl_offsets [U + 1] / excl_pos: CSR as fmx_fm_topk takes it, each row's list ascending), and lies in [0, N): a corrupt alias
 * entry is dropped, never dereferenced.  Sampling is WITH replacement: a position drawn twice is returned twice.
 * Result.  Row u holds its first n_neg eligible draws in the order of t: neg_pos [U, n_neg] int32 padded with -1, neg_logq
 * [U, n_neg] fp32 = logq[position] padded with -inf (or null).  A row's result depends on (seed, offset, u_base + u, N, the table,
 * its own and excluded positions, n_neg, n_try) only -- not on U, nor on how a batch is cut into calls.
 * Limits, all decided on the host before the launch: U, N, n_neg >= 1, n_neg <= n_try, non-null thresh / alias / neg_pos, neg_logq
 * only with logq, excl_offsets and excl_pos together, else FMX_ERR_ARG; n_neg <= 16 and n_try <= 1024, else FMX_ERR_UNSUPPORTED.
 * One launch (a wavefront per row: in round r lane l evaluates draw 64 r + l, a ballot and a lane prefix count keep the eligible
 * draws in draw order; at most n_try / 64 rounds, no retry loop), no LDS, no atomics, asynchronous on `stream`, safe under graph
 * capture; the result is identical run to run. */
int fmx_alias_sample_negatives(const uint32_t *thresh, const int32_t *alias, const float *logq, int32_t N,
                               const int32_t *excl_offsets, const int32_t *excl_pos, const int32_t *own_pos, int32_t U,
                               int32_t n_neg, int32_t n_try, uint64_t seed, uint64_t offset, uint32_t u_base,
                               int32_t *neg_pos, float *neg_logq, fmx_stream_t stream);

/* Streaming read of `bytes` (multiple of 16) with 16-byte loads; sink [1] receives a checksum so the loads stay
 * live.  Used by bench.py to measure the HBM-read ceiling on the same GPU in the same run. */
int fmx_stream_read(const void *buf, int64_t bytes, float *sink, fmx_stream_t stream);

/* Random-row read probe (measurement aid, SURVEY.md section 8(d) "informational gather ceilings"): n_rows_read rows of row_bytes
 * (64 or 128) at hashed positions of buf, 16 bytes per lane -- the forward gather's access pattern alone. */
int fmx_gather_read(const void *buf, int64_t bytes, int32_t row_bytes, int64_t n_rows_read, uint32_t seed, float *sink, fmx_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FMX_H */
