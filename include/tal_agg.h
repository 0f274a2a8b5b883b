/*
 * tal_agg.h — C-ABI of the MI355X (gfx950) neighbor-model aggregation library.
 *
 * The reference (msakarvadia/topology_aware_learning) is pure Python: its hot path is the
 * inner loop shared by every aggregation app,
 *
 *     src/decentralized_client.py:399-413   (weighted_module_avg)
 *     src/decentralized_client.py:433-446   (unweighted_module_avg)
 *     src/decentralized_client.py:535-549   (sim_centrality_module_avg)
 *     src/decentralized_client.py:597-611   (centrality_module_avg)
 *     src/decentralized_client.py:630-645   (scale_agg)
 *
 *         avg[name]  = w_0 * clone(sd_0[name])            # fp32(w) * x, rounded to fp32
 *         avg[name] += w_i * clone(sd_i[name])  (i=1..M-1) # separate fp32 add, no FMA
 *         model.load_state_dict(avg)                       # int64 buffers: trunc toward 0
 *
 * and its caller, the round driver src/decentralized_app.py:605-641, which submits one such
 * call per simulated device.  The reference binds no native code, so there is no FFI to
 * mirror; the entry points below are what a ctypes binding of that loop would call (see
 * INTEGRATION.md).  They replace the torch CPU ops clone/mul/add_/copy_ on that path.
 *
 * Conventions
 *   - every function returns 0 (TAL_OK) or a TAL_ERR_* code; tal_last_error() gives a
 *     thread-local message for the last failure on the calling thread.
 *   - all data pointers are DEVICE pointers owned by the caller; host arrays are named *_host.
 *   - `stream` is a hipStream_t (NULL = the default stream); calls are stream-ordered and
 *     never synchronize the device; the library keeps no device memory of its own (the one
 *     allocation it makes is the stream-ordered scratch of a K1 call, freed in that call).
 *   - weights arrive as float64 (Python floats / numpy float64 in the reference) and are
 *     rounded to fp32 exactly as torch does for `python_float * fp32_tensor`.
 *   - mode: TAL_MODE_EXACT reproduces the reference bit for bit (ordered i=0..M-1,
 *     separate fp32 multiply and add).  TAL_MODE_FMA is one fused chain per element, in the same
 *     operand order: acc = fl32(w_0 * x_0), then acc = fma(w_i, x_i, acc) for i = 1..M-1 - the
 *     product is not rounded, each step rounds once, IEEE arithmetic with subnormals kept.  It
 *     is as deterministic as EXACT mode: every fp32 entry point and kernel form gives the same
 *     bits, pinned by the test oracle's oracle.agg_f32(exact=False) / round_f32(exact=False).
 *     Its distance to EXACT mode is at most M*2^-24*sum|w x|.
 */
#ifndef TAL_AGG_H
#define TAL_AGG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TAL_OK 0
#define TAL_ERR_INVALID 1   /* bad argument (null pointer, size, alias, plan mismatch) */
#define TAL_ERR_HIP 2       /* HIP runtime error (launch / attribute) */
#define TAL_ERR_CAPACITY 3  /* plan does not fit (a row has more sources than the LDS tile) */
#define TAL_ERR_COMM 4      /* RCCL error (multi-GPU halo exchange) */

#define TAL_MODE_FMA 0
#define TAL_MODE_EXACT 1

/* Thread-local text of the last error on this thread ("" if none). */
const char* tal_last_error(void);
/* ABI version (bumped on any signature change).  ABI 33 removed the round over
 * register-resident source groups (K3r) with its entry point: no plan the library picks ever
 * selected it.  ABI 34 added the column clique entries with per-source weights
 * (tal_agg_round_clique_col_w_*).  ABI 35 added the sequential round in one launch (K3q:
 * tal_seq_plan_*, tal_agg_round_seq_*). */
int32_t tal_abi_version(void);

/* ---- K1: one aggregation call over M flattened operands --------------------------------
 * out[e] = sum_{i<M} fp32(w_host[i]) * x[i][e]   for e < n  (fp32 segment)
 * Replaces decentralized_client.py:399-411 (+ the fp32 part of load_state_dict :413).
 * x_host: host array of M device pointers.  out may alias any x[i] (the reference's
 * aggregating client is itself the last operand, decentralized_app.py:625).  Any M >= 1:
 * past 256 operands further passes continue the ordered chain from out, or - when an operand
 * past the first 256 aliases out - from a stream-ordered fp32 scratch (as tal_agg_bf16).  */
int32_t tal_agg_f32(const float* const* x_host, const double* w_host, int32_t m,
                    float* out, int64_t n, int32_t mode, void* stream);

/* int64 buffers (num_batches_tracked): torch promotes `python_float * int64_tensor` to
 * fp32, accumulates in fp32 and load_state_dict's copy_ truncates toward zero
 * (decentralized_client.py:407-413).  NaN / out-of-range results give INT64_MIN, as the
 * x86 cvttss2si the reference runs on does.  Any m >= 1 (past 256 operands: passes through
 * an fp32 scratch, as tal_agg_bf16); out may alias any x[i]. */
int32_t tal_agg_i64(const int64_t* const* x_host, const double* w_host, int32_t m,
                    int64_t* out, int64_t n, void* stream);

/* One call over a whole model (fp32 + int64 segments) in ONE launch: the fp32 segment as
 * tal_agg_f32 and the int64 segment as tal_agg_i64, the same arithmetic bit for bit, but the
 * per-call path's vector, n % 4 tail and int64 launches fused (decentralized_client.py:406-413
 * over every state_dict entry of a ResNet: the num_batches_tracked counters ride along).
 * xi_host may be NULL when n_i == 0.  Fused when m <= 64, n_i <= 65536 and every fp32
 * pointer is 16-byte aligned; otherwise the two segment calls above run instead. */
int32_t tal_agg_model_f32(const float* const* x_host, const int64_t* const* xi_host,
                          const double* w_host, int32_t m, float* out, int64_t n,
                          int64_t* out_i, int64_t n_i, int32_t mode, void* stream);

/* bf16 buffers (uint16_t bit patterns; bf16 models).  mode TAL_MODE_EXACT: the reference's
 * own ops on bf16 tensors (decentralized_client.py:407-411 - `w * clone(v)` and `+=` each
 * round their fp32 result to bf16, nearest even), bit-identical to it; TAL_MODE_FMA: fp32
 * fused accumulation rounded to bf16 once (|error| <= 2^-8 |result| + M 2^-24 sum|w x|).  NaN
 * results are stored as 0xFFFF (torch's vectorized conversion).  Any m >= 1: past 256
 * operands the ordered chain runs in passes of 256 through an fp32 scratch of n elements,
 * allocated and freed in stream order (hipMallocAsync), carrying the same running value the
 * one-pass kernel keeps in registers; out may alias any x[i]. */
int32_t tal_agg_bf16(const uint16_t* const* x_host, const double* w_host, int32_t m,
                     uint16_t* out, int64_t n, int32_t mode, void* stream);

/* ---- K3: one whole aggregation round over a device-resident model pool -----------------
 * Row r of the round computes pool_out[out_row[r]][e] = sum_k fp32(w[k]) * pool_in[col[k]][e]
 * over k = row_ptr[r] .. row_ptr[r+1]-1 in that (reference) order, for e < n.  All rows read
 * the pool as it was before the round ("snapshot" semantics).
 *
 * The host first turns the CSR into a tile plan (rows grouped so that each group's distinct
 * sources fit one LDS tile); the plan is a flat int32 blob the caller copies to the device.
 */
typedef struct tal_round_plan_info {
  int32_t rows;          /* rows in the round */
  int32_t nnz;           /* operands over all rows */
  int32_t n_groups;      /* row groups */
  int32_t total_src;     /* staged sources summed over groups */
  int32_t max_src;       /* largest group source count (sizes the LDS tile) */
  int32_t max_rows;      /* largest group row count */
  int32_t max_nnz;       /* largest group operand count */
  int32_t c4;            /* float4 columns per staged source row per tile (16, 32, 64 or 128) */
  int32_t lds_bytes;     /* LDS per workgroup the round kernel will request */
  /* offsets (in int32 words) of the plan's arrays inside the blob */
  int32_t off_grp_row_ptr;  /* [n_groups+1] */
  int32_t off_grp_src_ptr;  /* [n_groups+1] */
  int32_t off_src_row;      /* [total_src]  pool_in row of each staged source */
  int32_t off_row_ptr;      /* [rows+1] */
  int32_t off_op_slot;      /* [nnz] staged-source slot of each operand (within its group) */
  int32_t off_op_w;         /* [nnz] fp32 weight bits */
  int32_t off_out_row;      /* [rows] pool_out row of each row */
  int32_t words;            /* total int32 words of the blob */
  /* dense row-block form (dense_rb > 0): a wavefront computes dense_rb rows per pass over its
   * group's staged sources, each LDS read serving every row that uses that source.  Valid
   * when every row lists its operands as sources in ascending order followed by the row's own
   * (reference order: sorted neighbors, then self). */
  int32_t dense_rb;         /* rows per block (0 = sparse form only) */
  int32_t n_blocks;         /* row blocks over all groups */
  int32_t off_grp_blk_ptr;  /* [n_groups+1] first block of each group */
  int32_t off_blk_tab;      /* [n_blocks] word offset of each block's table inside the blob */
  int32_t off_dense;        /* start of the tables (32-B aligned): per block {n_used, 7 pad words,
                             * slot[n_used] (staged slots
                             * the block's rows use, ascending), mask[n_used] (bit r = row r of
                             * the block uses that slot, own model excluded; bit 31 set
                             * when all those rows have the same fp32 weight, which then
                             * fills every w slot: one product w*x serves them all),
                             * w[n_used][dense_rb] fp32}; n_used padded to a multiple of 4
                             * with mask-0 entries */
  int32_t dense_reads;      /* LDS operand reads per column in the dense form (sparse: nnz) */
  /* streamed form (stream_cs > 0, built by tal_round_plan_build_stream): a workgroup of W
   * wavefronts (W = 8 or 16) owns a group of at most 8*W rows (one dense row block per
   * wavefront) and streams the group's staged sources through a ring of LDS chunks of
   * stream_cs = 2*W sources x 64 float4 columns (two 1 KiB global->LDS DMAs per wavefront per
   * chunk), so a group's source count is not bounded by LDS.  Each block's table lists its
   * entries chunk by chunk (including the rows' own models, flagged in mask bits 8..15), every
   * chunk's run padded to a multiple of 4 with mask-0 entries. */
  int32_t stream_cs;        /* sources per chunk (16 or 32); 0 = LDS-resident groups */
  /* narrow form (c4 16 / 32): each row's operands as (slot * c4, fp32 weight bits) pairs - its
   * first operand, then the rest padded to a multiple of 4 with (max_src * c4, 1.0f) pairs that
   * read a tile of -0.0 the kernel keeps in LDS slot max_src: fl(1 * -0) = -0 and x + -0 == x
   * for every x, so padding is an exact identity.  Rows of a group are ordered by operand count
   * (descending) so that the 64 / c4 rows a wavefront computes together have similar counts. */
  int32_t off_nrow_ptr;     /* [rows+1] pair offset of each row */
  int32_t off_npairs;       /* [npairs][2] int32 */
  int32_t npairs;           /* pairs over all rows (padded) */
  int32_t max_npairs;       /* largest group pair count */
  /* narrow_roww = 1 when every row's operands share one fp32 weight (the unweighted strategy,
   * scale_agg): the pairs are replaced by 16-bit slots (slot * c4, two per int32 word), each
   * row's run padded to a multiple of 4 with a zero-tile slot (slot ns: a -0.0 tile for a
   * row weight with the sign bit clear, slot ns + 1: +0.0 otherwise, so fl(w * 0) = -0 exactly),
   * the accumulator starts at -0.0 (-0 + y == y for every y), and the row weights are in
   * off_nrow_w.  off_nrow_ptr then counts slots; npairs counts slots. */
  int32_t narrow_roww;
  int32_t off_nrow_w;       /* [rows] fp32 weight bits (narrow_roww) */
  int32_t scalar_lds_bytes; /* LDS of the staged scalar tail kernel (the largest group; its
                             * tiles are c4 float4 wide, 16 for narrow plans) */
  /* broadcast form (narrow_bcast > 0, built by tal_round_plan_build_bcast; c4 16 / 32): the
   * LDS holds only the group's data tile and one -0.0 tile (slot max_src).  Each wavefront of
   * a workgroup runs a fixed program over the group's passes (4 rows computed together, 16
   * lanes each - one float4 chunk per lane at c4 = 16, chunks cl and cl + 16 at c4 = 32 - rows
   * ordered by operand count, descending), kept in VGPRs for the whole launch: a record
   * is 64 lanes x {LDS byte offset of the operand's tile column 0, fp32 weight bits} holding
   * operands 16c .. 16c+15 of every row of the pass (lane L: row L / 16, operand 16c + L % 16;
   * past a row's count: the -0.0 tile with weight 1.0, an exact identity); the kernel hands
   * operand u to the row's lanes by a DPP row broadcast from lane u, so no per-operand plan
   * read touches LDS.  Program of wavefront w of group g at word off_bc_prog[g * narrow_bcast +
   * w] (even): {n_rec, n_pass, data offset (words from the program, even), 5 x 0},
   * bc_rec_max descriptors {operands in the record (1..16) | last of its pass << 8 | pass << 16},
   * 4 output rows per pass (-1: none), then the n_rec records (128 words each). */
  int32_t narrow_bcast;     /* wavefronts per workgroup (8, 12 or 16); 0 = not this form */
  int32_t bc_rec_max;       /* records per wavefront (128 / narrow_bcast) */
  int32_t off_bc_prog;      /* [n_groups * narrow_bcast] program offsets */
  int32_t bc_records;       /* records over all programs */
  int32_t bc_wg_per_cu;     /* resident workgroups per CU the launch sizes registers for (1: 128
                             * VGPRs at 1024 threads, deeper read pipelining; 2: two groups' tiles
                             * overlap one's staging with the other's arithmetic) */
} tal_round_plan_info;

/* Blob size in int32 words of the sparse or narrow form for `rows` rows / `nnz` operands (an upper
 * bound); the dense tables come on top — tal_round_plan_build reports the exact need. */
int64_t tal_round_plan_words(int32_t rows, int64_t nnz);

/* Build the plan on the host.  row_ptr_host[rows+1], col_host[nnz], w_host[nnz] (float64),
 * out_row_host[rows].  c4 in {16,32,64,128} (16 / 32: narrow tiles, a wavefront computes 64/c4
 * rows at once, sparse form only); lds_bytes = LDS budget per workgroup (staged tile
 * 16*c4 B per source plus the plan slice the narrow and scalar kernels stage).  Rows keep their order; consecutive rows
 * share a group while the union of their sources fits; a group's staged sources are in
 * ascending pool row order.  dense_rb: 0 = sparse form, 8 = dense row blocks of 8 (falls back
 * to sparse if a row is not in reference order), -1 = dense when it cuts the LDS operand reads
 * to at most a quarter (one read serves >= 4 operands: cliques).  Returns
 * TAL_ERR_CAPACITY if one row alone has more distinct sources than fit, or if plan_capacity_words
 * is too small (info->words then holds the size needed). */
int32_t tal_round_plan_build(int32_t rows, const int32_t* row_ptr_host, const int32_t* col_host,
                             const double* w_host, const int32_t* out_row_host, int32_t c4,
                             int32_t lds_bytes, int32_t dense_rb, int32_t* plan_host,
                             int64_t plan_capacity_words, tal_round_plan_info* info);

/* Broadcast-form narrow plan (see narrow_bcast above): as tal_round_plan_build at c4 16 / 32,
 * with waves (8, 12 or 16) wavefronts per workgroup and wg_per_cu (1 or 2) resident workgroups per CU
 * (2 caps lds_bytes at 80 KiB; a c4 = 32 group of more than 128 sources at 1024 threads
 * launches only with wg_per_cu 1); a group also needs every wavefront's program
 * to fit 128 / waves records (TAL_ERR_CAPACITY for a row no group can take).  Per-operand
 * weights cost no LDS reads in this form (the centrality strategies on graphs whose degrees
 * differ: decentralized_client.py:572-611). */
int32_t tal_round_plan_build_bcast(int32_t rows, const int32_t* row_ptr_host, const int32_t* col_host,
                                   const double* w_host, const int32_t* out_row_host, int32_t c4,
                                   int32_t lds_bytes, int32_t waves, int32_t wg_per_cu, int32_t* plan_host,
                                   int64_t plan_capacity_words, tal_round_plan_info* info);

/* The broadcast form's staging limit: the most float4 staging loads per column tile (sources x
 * c4) one group of a (c4, waves, wg_per_cu) broadcast plan may need - the planner caps groups
 * at it and the launcher stages up to it (one table in the library for both).  -1 for a form
 * that does not exist. */
int64_t tal_round_bcast_max_loads(int32_t c4, int32_t waves, int32_t wg_per_cu);

/* Streamed plan (see stream_cs above).  Rows keep their order; consecutive rows share a group
 * while the group has at most max_group_rows rows (<= 128) and, if max_group_src > 0, at
 * most max_group_src distinct sources.  Every row must list its operands in reference order
 * (ascending distinct sources, then its own model, which does not occur before): otherwise
 * TAL_ERR_INVALID.  c4 is 64.  TAL_ERR_CAPACITY as for tal_round_plan_build. */
int32_t tal_round_plan_build_stream(int32_t rows, const int32_t* row_ptr_host,
                                    const int32_t* col_host, const double* w_host,
                                    const int32_t* out_row_host, int32_t max_group_rows,
                                    int32_t max_group_src, int32_t* plan_host,
                                    int64_t plan_capacity_words, tal_round_plan_info* info);

/* Execute the round on the fp32 segment (n elements per model; row stride ld_in / ld_out in
 * elements).  plan_dev = the blob copied to the device.  pool_out may equal pool_in only if
 * the plan has a single group (each workgroup stages every source of its tile in LDS before
 * it writes).  16-B aligned pools with ld % 4 == 0 take the float4 path; others the scalar
 * tiled path. */
int32_t tal_agg_round_f32(const float* pool_in, int64_t ld_in, float* pool_out, int64_t ld_out,
                          int64_t n, const int32_t* plan_dev, const tal_round_plan_info* info,
                          int32_t mode, void* stream);

/* The same round on the int64 segment (fp32 accumulate, truncation, as tal_agg_i64). */
int32_t tal_agg_round_i64(const int64_t* pool_in, int64_t ld_in, int64_t* pool_out,
                          int64_t ld_out, int64_t n, const int32_t* plan_dev,
                          const tal_round_plan_info* info, void* stream);

/* Clique rounds (K3c).  Rows of a round that form uniform-weight cliques — m <= 64 sources
 * s_0 < ... < s_{m-1} (pool rows) with one fp32 weight w, and for member i an output row whose
 * operands are, in reference order (decentralized_app.py:625), every other member ascending and
 * then s_i — are computed from one read of each source: the products are shared and each row's
 * in-order chain extends the shared prefix (bitwise the reference in EXACT mode; FMA mode as
 * tal_agg_f32's).  table_dev: n_cliques records of TAL_CLIQUE_WORDS int32
 *   {m, bits of w, n_att, 0, src_row[64], out_row[64], attached[4][12]}
 * (out_row -1: member without an output row) copied to the device.  An attached row (a
 * barbell's bridge node) has its own weight v and operands = members selected by a 64-bit
 * mask + at most two other rows + its own model, in reference order:
 *   {out_row, bits of v, mask lo, mask hi, self member index or -1, self pool row or -1,
 *    n_ext, ext_row[2], ext_pos[2] (members with a smaller pool row), 0}.
 * The other rows of the round run through a regular plan (a second call).  Out of place only; pools 8-B aligned with even ld.  mmax = the largest m (16, 32 or
 * 64 registers of products per lane). */
#define TAL_CLIQUE_WORDS 180
int32_t tal_agg_round_clique_f32(const float* pool_in, int64_t ld_in, float* pool_out, int64_t ld_out,
                                 int64_t n, const int32_t* table_dev, int32_t n_cliques, int32_t mmax,
                                 int32_t mode, void* stream);

/* The clique round on bf16 pools (ABI 30): the same table and the same checks, arithmetic as
 * tal_agg_bf16 per mode.  EXACT: the shared products are bf16(fl(w * x_j)) and every step of a
 * row's chain rounds its fp32 sum to bf16, so each row stays the reference's own left-to-right
 * chain on bf16 tensors; FMA: the fp32 entry's fused chains on the widened values, rounded once
 * by the store (NaN stored as 0xFFFF).  A column pair is one 32-bit word: pools 4-B aligned
 * with even ld, else TAL_ERR_INVALID. */
int32_t tal_agg_round_clique_bf16(const uint16_t* pool_in, int64_t ld_in, uint16_t* pool_out,
                                  int64_t ld_out, int64_t n, const int32_t* table_dev,
                                  int32_t n_cliques, int32_t mmax, int32_t mode, void* stream);

/* Clique rounds with per-source weights (ABI 31): the weighted and centrality apps on a clique.
 * Source s_j carries the same fp32 weight w_j in every row of the block (all members aggregate
 * over the same models, so the normaliser is common), hence the products p_j = fl(w_j * x_j) are
 * still shared and every row is the same in-order chain as above; only the multiply reads w_j.
 * EXACT: p_j = fl(w_j * x_j) (bf16: rounded to bf16, as is every step of a chain); FMA:
 * acc = fma(w_j, x_j, acc) along the same chains from -0.0.  Zero and negative weights are
 * ordinary values.  table_dev is the record above; its two weight words (bits of w, bits of v)
 * are ignored.  wtab_dev: n_cliques records of TAL_CLIQUE_WWORDS floats on the device,
 *   {w[64], attached[4]{v_member[64], v_ext[2], v_self}}
 * w[j] = the weight of s_j; for attached row q, v_member[j] = its weight for member position j
 * (used where its mask selects j), v_ext[k] = for ext_row[k], v_self = for its own model.  Every
 * slot not in use holds 1.0f: a padding step multiplies -0.0 by it (fl(1 * -0.0) = -0.0,
 * fma(1, -0.0, acc) = acc for every acc, -0.0 included).  Same checks and errors as the entries
 * above, and TAL_ERR_INVALID for a null wtab_dev. */
#define TAL_CLIQUE_WWORDS 332
#if defined(__cplusplus)
static_assert(TAL_CLIQUE_WWORDS == 64 + 4 * (64 + 2 + 1), "weight record: 64 members + 4 attached rows");
#else
_Static_assert(TAL_CLIQUE_WWORDS == 64 + 4 * (64 + 2 + 1), "weight record: 64 members + 4 attached rows");
#endif
int32_t tal_agg_round_clique_w_f32(const float* pool_in, int64_t ld_in, float* pool_out, int64_t ld_out,
                                   int64_t n, const int32_t* table_dev, int32_t n_cliques, int32_t mmax,
                                   int32_t mode, void* stream, const float* wtab_dev);
int32_t tal_agg_round_clique_w_bf16(const uint16_t* pool_in, int64_t ld_in, uint16_t* pool_out,
                                    int64_t ld_out, int64_t n, const int32_t* table_dev,
                                    int32_t n_cliques, int32_t mmax, int32_t mode, void* stream,
                                    const float* wtab_dev);

/* Clique rounds for blocks of up to 128 members (K3c1, ABI 32): uniform-weight blocks as above,
 * one element column per lane instead of a column pair, so the 128 product registers of a lane
 * hold up to 128 members (`unweighted_fl` over 66 or 100 clients is one such block).  The
 * arithmetic is the entries' above per column and per mode (EXACT: p_j = fl(w * x_j), on bf16
 * rounded to bf16 as is every step of a chain; FMA: fma(w, x_j, acc) along the same chains from
 * -0.0, bf16 rounded once at the store, NaN stored as 0xFFFF), each row its own in-order chain.
 * table_dev: n_cliques records of TAL_CLIQUE_COL_WORDS int32
 *   {m, bits of w, 0, 0, src_row[128], out_row[128]}
 * (out_row -1: member without an output row) copied to the device; no attached rows and no
 * per-source weights.  Blocks of any m <= 128 are legal (m <= 64 gives the bits of the entries
 * above).  Any ld >= n and element-aligned pools (4 B fp32, 2 B bf16): there is no column-pair
 * rule.  Out of place only.  TAL_ERR_INVALID, with no launch, for a null pointer, pool_out ==
 * pool_in, mmax outside 1..TAL_CLIQUE_COL_MAX, n_cliques outside 0..65535 or ld < n.  mmax = the
 * largest m (kernels for 68, 84, 100, 116 and 128 product registers per lane). */
#define TAL_CLIQUE_COL_MAX 128
#define TAL_CLIQUE_COL_WORDS 260
#if defined(__cplusplus)
static_assert(TAL_CLIQUE_COL_WORDS == 4 + 2 * TAL_CLIQUE_COL_MAX, "column-form record: header + 128 sources + 128 rows");
#else
_Static_assert(TAL_CLIQUE_COL_WORDS == 4 + 2 * TAL_CLIQUE_COL_MAX, "column-form record: header + 128 sources + 128 rows");
#endif
int32_t tal_agg_round_clique_col_f32(const float* pool_in, int64_t ld_in, float* pool_out, int64_t ld_out,
                                     int64_t n, const int32_t* table_dev, int32_t n_cliques, int32_t mmax,
                                     int32_t mode, void* stream);
int32_t tal_agg_round_clique_col_bf16(const uint16_t* pool_in, int64_t ld_in, uint16_t* pool_out,
                                      int64_t ld_out, int64_t n, const int32_t* table_dev,
                                      int32_t n_cliques, int32_t mmax, int32_t mode, void* stream);

/* K3c1 with per-source weights (ABI 34): the weighted and centrality apps on a clique of 65..128
 * members (`weighted_module_avg` over 66 or 100 clients is one such block).  The column entries'
 * chains with w_j in place of w: EXACT p_j = fl(w_j * x_j) (bf16: rounded to bf16, as is every
 * step of a chain), then row i = ((S_i + p_{i+1}) + ... + p_{m-1}) + p_i; FMA acc = fma(w_j, x_j,
 * acc) along the same chains from -0.0 (bf16 rounded once at the store, NaN stored as 0xFFFF).
 * Zero and negative weights are ordinary values.  table_dev is the TAL_CLIQUE_COL_WORDS record
 * above; its weight word is ignored.  wtab_dev: n_cliques records of TAL_CLIQUE_COL_WWORDS floats
 * on the device, w[j] = the weight of src_row[j]; every slot not in use holds 1.0f (a padding
 * step is x = -0.0 under weight 1.0 in both modes: fl(1 * -0.0) = -0.0, fma(1, -0.0, acc) = acc
 * for every acc, -0.0 included).  Blocks of any m <= 128 are legal (m <= 64 gives the bits of
 * tal_agg_round_clique_w_*; all weights equal gives those of tal_agg_round_clique_col_*).  Same
 * checks and errors as the column entries, and TAL_ERR_INVALID, with no launch, for a null
 * wtab_dev. */
#define TAL_CLIQUE_COL_WWORDS 128
#if defined(__cplusplus)
static_assert(TAL_CLIQUE_COL_WWORDS == TAL_CLIQUE_COL_MAX, "column-form weight record: one float per member");
#else
_Static_assert(TAL_CLIQUE_COL_WWORDS == TAL_CLIQUE_COL_MAX, "column-form weight record: one float per member");
#endif
int32_t tal_agg_round_clique_col_w_f32(const float* pool_in, int64_t ld_in, float* pool_out, int64_t ld_out,
                                       int64_t n, const int32_t* table_dev, int32_t n_cliques, int32_t mmax,
                                       int32_t mode, void* stream, const float* wtab_dev);
int32_t tal_agg_round_clique_col_w_bf16(const uint16_t* pool_in, int64_t ld_in, uint16_t* pool_out,
                                        int64_t ld_out, int64_t n, const int32_t* table_dev,
                                        int32_t n_cliques, int32_t mmax, int32_t mode, void* stream,
                                        const float* wtab_dev);

/* ---- K3q: a sequential round in one launch (ABI 35) -----------------------------------------
 * The reference's round under one aggregation thread: its apps overwrite the client models that
 * later apps of the same round read (decentralized_client.py:413, decentralized_app.py:606,629),
 * so clients go in order and each call sees the earlier calls' writes.  In place on one pool:
 *
 *   for r = 0 .. rows-1, in plan order:
 *     pool[out_row[r]][e] = chain over k = row_ptr[r] .. row_ptr[r+1]-1 of (fp32(w[k]), pool[col[k]][e])
 *
 * where pool is the state rows 0 .. r-1 of this call left (a row reads its own old value where it
 * lists itself).  The chain is tal_agg_f32 / tal_agg_bf16 / tal_agg_i64's per dtype and mode, from
 * the same device code, so row r has the bits of that call on the running pool: fp32 EXACT a
 * separate multiply and add per operand, FMA fl(w_0 x_0) then fma; bf16 EXACT every product and
 * sum rounded to bf16, FMA rounded once at the store (NaN stored as 0xFFFF); int64 operands
 * converted to fp32, accumulated in fp32 and truncated toward zero (NaN / out of range:
 * INT64_MIN).  The value later rows read is the stored one (bf16: the rounded value; int64: the
 * truncated integer).  Rows keep the caller's order - the order of the sweep - and operands the
 * caller's order; any operand order and count is legal and a source may occur twice in a row.
 * Pool rows the round does not write are not touched.
 *
 * The sweep is independent per element column: a wavefront owns a tile of 64 columns for the
 * whole round (one column per lane; each source row's piece staged into LDS once, each result
 * written to HBM and back into its LDS slot), so every model is read once and no spare pool is
 * needed.  One column per lane: any ld >= n, element-aligned pools.  At most TAL_SEQ_MAX_SRC
 * distinct source rows (a 64-column fp32 tile of 256 sources is 64 KiB of LDS for one wave).
 * The int64 entry runs one thread per column on global memory.
 *
 * Plan blob (int32 words, built on the host, copied to the device by the caller):
 *   {rows, nnz, n_src, words, max_row, max_ops, 0, 0}
 *   src_row[n_src]   the distinct pool rows that occur as operands, ascending; a row's slot is
 *                    its index here
 *   row_ptr[rows+1]
 *   op_slot[nnz]     slot of each operand
 *   op_w[nnz]        fp32 bits of (float)w
 *   out_row[rows]
 *   out_slot[rows]   slot of out_row[r], or -1 when no row reads it
 *   0 x 8            padding: the kernel reads the plan eight words at a time
 * tal_seq_plan_build: TAL_ERR_INVALID for a null array, rows <= 0, an empty row, a negative pool
 * row or an out_row listed twice; TAL_ERR_CAPACITY when n_src > TAL_SEQ_MAX_SRC, and when
 * plan_host is null or capacity_words too small (info->words then holds the size needed; info is
 * filled in both cases).  tal_seq_plan_words is an upper bound for any such round.
 *
 * tal_agg_round_seq_*: pool_rows = rows of the pool.  TAL_ERR_INVALID, with no launch, for a null
 * pointer, n < 0, ld < n or a plan row >= pool_rows (info->max_row); n == 0 returns TAL_OK
 * without a launch. */
#define TAL_SEQ_MAX_SRC 256
typedef struct tal_seq_plan_info {
  int32_t rows;          /* rows of the round */
  int32_t nnz;           /* operands over all rows */
  int32_t n_src;         /* distinct source rows (LDS slots) */
  int32_t max_row;       /* largest pool row read or written */
  int32_t max_ops;       /* operands of the longest row */
  /* offsets (int32 words) of the arrays inside the blob */
  int32_t off_src_row;
  int32_t off_row_ptr;
  int32_t off_op_slot;
  int32_t off_op_w;
  int32_t off_out_row;
  int32_t off_out_slot;
  int32_t reserved;
  int64_t words;         /* total int32 words of the blob */
} tal_seq_plan_info;
int64_t tal_seq_plan_words(int32_t rows, int64_t nnz);
int32_t tal_seq_plan_build(int32_t rows, const int32_t* row_ptr_host, const int32_t* col_host,
                           const double* w_host, const int32_t* out_row_host, int32_t* plan_host,
                           int64_t capacity_words, tal_seq_plan_info* info);
int32_t tal_agg_round_seq_f32(float* pool, int64_t ld, int64_t pool_rows, int64_t n, const int32_t* plan_dev,
                              const tal_seq_plan_info* info, int32_t mode, void* stream);
int32_t tal_agg_round_seq_bf16(uint16_t* pool, int64_t ld, int64_t pool_rows, int64_t n, const int32_t* plan_dev,
                               const tal_seq_plan_info* info, int32_t mode, void* stream);
int32_t tal_agg_round_seq_i64(int64_t* pool, int64_t ld, int64_t pool_rows, int64_t n, const int32_t* plan_dev,
                              const tal_seq_plan_info* info, void* stream);

/* tal_agg_round_f32's round on bf16 pools (arithmetic as tal_agg_bf16, per mode).  Takes sparse plans
 * (c4 64 / 128, dense_rb 0) and narrow plans (c4 16 / 32); TAL_ERR_INVALID for dense or
 * streamed plans.  A staged tile holds the sources' values as fp32 (c4 float4 per source). */
int32_t tal_agg_round_bf16(const uint16_t* pool_in, int64_t ld_in, uint16_t* pool_out,
                           int64_t ld_out, int64_t n, const int32_t* plan_dev,
                           const tal_round_plan_info* info, int32_t mode, void* stream);

/* The kernel tal_agg_round_f32 (bf16 != 0: tal_agg_round_bf16) runs over the float4 columns of
 * aligned pools for this plan, answered by the function the launch itself dispatches on (ABI 28):
 * "k_round_stream", "k_round_wide", "k_round_f32_narrow" (the broadcast form too),
 * "k_round_f32_persistent" or "k_round_f32_tiled"; "" for a null info.  A static string. */
const char* tal_round_kernel_name(const tal_round_plan_info* info, int32_t bf16);

/* ---- K2: cosine similarity of two models' parameters, bit for bit -------------------------
 * Reference: cosine_similarity, decentralized_client.py:661-681: for each parameter tensor
 * viewed as [A, I, B] (dim 1 = the reduced dim; 1-D tensors are unsqueezed to [n, 1]),
 * nn.CosineSimilarity(dim=1, eps=1e-6) gives A*B values whose mean is taken; the result is
 * the average of those means over tensors.  Every fp32 operation is the reference's, in the
 * order of the torch CPU kernels it runs on (vector_norm, the cascade sum, sum / numel; see
 * oracle/cosine_oracle.c, pinned bitwise by the reference's own values, near-ties included):
 * the result is the reference's fp32 value, so sim_centrality_module_avg's least-similar
 * neighbor (:511-516) is the reference's.  A tensor's mean over A*B >= 32768 outputs is, in
 * torch, a two-pass parallel sum whose order depends on the process's intra-op thread count T
 * (at::parallel_for chunks of ceil(n / min(T, ceil(n / 32768))) elements, then a T-entry
 * buffer summed); the plan carries T (tal_cosine_plan_set_threads, default 1 = serial), so the
 * result is torch's for that T.
 *
 * seg_host: 4*n_seg int64 {offset (elements into the flat parameter arena), A, I, B}.
 * The plan (int64 words, tal_cosine_plan_words; copied to the device by the caller, and the
 * host copy passed too) = {n_seg, n_outputs, threads, streamed chunks}, per tensor {offset, A,
 * I, B, first output, kind, outputs per chunk}, per workgroup chunk {tensor, first output, count,
 * streamed}.  Column tensors with B < 32 (3 x 3 convolutions) run streamed (ABI 25): every
 * model's norms in one launch, then each pair's products, both walking i in 16-element steps
 * through LDS; the others one thread (or 8 lanes) per output.
 *
 * a_ptrs_host / b_ptrs_host: n_pairs device pointers; pair j compares model a_j with b_j
 * (flat fp32 parameter arenas of the same layout).  scratch: device buffer of at least
 * tal_cosine_scratch_bytes(plan_host, n_pairs) bytes (ABI 25: 4 (3 n_outputs + n_seg) per pair
 * of a launch of up to 32 pairs).  out_dev: n_pairs fp32 results. */
int64_t tal_cosine_plan_words(const int64_t* seg_host, int32_t n_seg);
int32_t tal_cosine_plan_build(const int64_t* seg_host, int32_t n_seg, int64_t* plan_host,
                              int64_t plan_capacity_words, int32_t* n_chunks);
/* Set a built plan's thread word (1..1024; the calling process's torch.get_num_threads()). */
int32_t tal_cosine_plan_set_threads(int64_t* plan_host, int32_t threads);
int64_t tal_cosine_scratch_bytes(const int64_t* plan_host, int32_t n_pairs);
int32_t tal_cosine_params(const float* const* a_ptrs_host, const float* const* b_ptrs_host,
                          int32_t n_pairs, const int64_t* plan_dev, const int64_t* plan_host,
                          int32_t n_chunks, void* scratch, float* out_dev, void* stream);

/* ---- K2 on bf16 models (ABI 27) -------------------------------------------------------------
 * The reference has no bf16 path for cosine_similarity, so the definition is this project's:
 *
 *   the cosine similarity of two bf16 models is K2's fp32 result for the two models with every
 *   parameter widened exactly to fp32 - bit for bit what the reference's
 *   cosine_similarity(m1.float(), m2.float()) returns, for the plan's thread word.
 *
 * Only the loads differ: a bf16 bit pattern u becomes the fp32 value with bits u << 16.  Every
 * fp32 operation and its order stay K2's (vector_norm's FMA chains, the 1e-6 clamp, the two
 * quotients, the cascade sums, the per-tensor mean under the plan's thread word, the in-order
 * average over tensors), and the result is fp32.  It is not an op-by-op emulation of torch's bf16
 * CPU kernels: a result with 8 mantissa bits would make sim_centrality_module_avg's
 * least-similar-neighbor choice (decentralized_client.py:511-516) tie-prone, and those kernels'
 * reduction orders are not the fp32 ones K2 pins.
 *
 * The *_bf16 entry points (here, K2r's and the host forms' below) are their fp32 twins with
 * `const uint16_t*` models / pool (bf16 bit patterns; offsets and ld in elements, rows 2-byte
 * aligned): plans, round tables, scratch sizes, results and error codes are shared. */
int32_t tal_cosine_params_bf16(const uint16_t* const* a_ptrs_host, const uint16_t* const* b_ptrs_host,
                               int32_t n_pairs, const int64_t* plan_dev, const int64_t* plan_host,
                               int32_t n_chunks, void* scratch, float* out_dev, void* stream);

/* ---- K2r: K2 over a whole round's pair list (ABI 26) --------------------------------------
 * The `*_sim` strategies need the cosine of every client with every neighbor.  In a batched
 * round all models are rows of one pool segment (row r at pool + r ld), and the pairs of a round
 * share work that a per-client call cannot: a clamped norm belongs to a model, not to a pair, and
 * the value of a pair is bitwise symmetric (fl(x/n1) fl(y/n2) commutes and every sum runs in the
 * same order), so an undirected topology needs each edge once.  The round form computes every
 * norm once per model, every unique unordered pair once, and writes out_dev[j] for each of the
 * caller's ordered pairs, in the caller's order.  Every fp32 operation and its order are K2's
 * (the kernels share K2's device code), so out_dev[j] is bit for bit what tal_cosine_params
 * gives for (pool + row_a[j] ld, pool + row_b[j] ld) under the same plan, thread word included;
 * a NaN result is NaN for both orders (payload unspecified).
 *
 * The table (int32 words; built on the host by tal_cosine_round_build into a buffer of at least
 * tal_cosine_round_words(n_pairs) words, or exactly info->words, and copied to the device by the
 * caller, the host copy passed too):
 *   {n_pairs, n_unique, n_models, n_groups, max_group, pool_rows, words, 0}
 *   models[n_models]     the distinct rows referenced, ascending; a model's slot is its index here
 *   unique[n_unique][2]  the distinct unordered pairs as model slots {a, b}, a the row its
 *                        group shares (a == b, the self pair, is allowed), group after group
 *   groups[n_groups][3]  {slot a, first unique pair, count}: consecutive unique pairs that share
 *                        row a, at most 8 to a group (one streamed product workgroup holds a
 *                        and 8 others in LDS).  Each pair is given to one of its two rows so
 *                        that groups fill: the row with the most pairs still to place (8 or
 *                        more count alike, ties to the smaller row) takes up to 8 of them, until
 *                        none is left; a row with more partners than 8 gets several groups
 *   map[n_pairs]         the unique pair of each ordered pair
 * tal_cosine_round_build: TAL_ERR_INVALID for n_pairs <= 0, a null row array or a row outside
 * [0, pool_rows); TAL_ERR_CAPACITY, with the need in info->words, when table_host is null or
 * capacity_words is too small.  info carries the counts.
 *
 * Scratch (device, from the caller): 4 n_outputs per model (the norm table), 4 (n_outputs +
 * n_seg) per unique pair of a batch, 4 per unique pair.  tal_cosine_round_scratch_bytes picks
 * the largest batch of whole groups under budget_bytes (at most 32768 pairs), stores it in
 * info->batch_pairs with the number of batches in info->n_batches, and returns the bytes needed
 * (<= budget_bytes); -1 for bad arguments or when not even the largest group fits.
 * tal_cosine_round walks the groups in those batches.  It allocates nothing, runs every launch on
 * `stream`, and never synchronises.  plan_dev / plan_host / n_chunks: a plan of
 * tal_cosine_plan_build, as for tal_cosine_params; ld (elements) must cover the plan's tensors. */
typedef struct tal_cosine_round_info {
  int32_t n_pairs;     /* ordered pairs given */
  int32_t n_unique;    /* distinct unordered pairs */
  int32_t n_models;    /* distinct rows */
  int32_t n_groups;
  int32_t max_group;   /* pairs of the largest group (<= 8) */
  int32_t pool_rows;
  int32_t batch_pairs; /* set by tal_cosine_round_scratch_bytes: unique pairs per batch */
  int32_t n_batches;   /* set by tal_cosine_round_scratch_bytes */
  int64_t words;       /* table words */
} tal_cosine_round_info;
int64_t tal_cosine_round_words(int32_t n_pairs);
int32_t tal_cosine_round_build(const int32_t* row_a_host, const int32_t* row_b_host, int32_t n_pairs,
                               int32_t pool_rows, int32_t* table_host, int64_t capacity_words,
                               tal_cosine_round_info* info);
int64_t tal_cosine_round_scratch_bytes(const int64_t* plan_host, const int32_t* table_host,
                                       tal_cosine_round_info* info, int64_t budget_bytes);
int32_t tal_cosine_round(const float* pool, int64_t ld, const int64_t* plan_dev, const int64_t* plan_host,
                         int32_t n_chunks, const int32_t* table_dev, const int32_t* table_host,
                         const tal_cosine_round_info* info, void* scratch, int64_t scratch_bytes,
                         float* out_dev, void* stream);
/* K2r over a bf16 pool segment (ABI 27; semantics: "K2 on bf16 models" above). */
int32_t tal_cosine_round_bf16(const uint16_t* pool, int64_t ld, const int64_t* plan_dev, const int64_t* plan_host,
                              int32_t n_chunks, const int32_t* table_dev, const int32_t* table_host,
                              const tal_cosine_round_info* info, void* scratch, int64_t scratch_bytes,
                              float* out_dev, void* stream);

/* ---- FedProx proximal term ------------------------------------------------
 * Reference: local_train, tasks.py:277-286: loss += (prox_coeff / 2) * sum_t sum_p
 * ||w_p - wt_p||_2 over the neighbors t and the parameter tensors p.  Here the parameters are
 * segments of flat fp32 rows (a device ModelPool row per model).
 *
 * seg_host: 2*n_seg int64 {offset, length} of each parameter in the flat row.  The plan
 * (int64, copied to the device by the caller) cuts them into workgroup chunks.
 * tal_prox_norms: norms_out[t*n_seg + p] = ||w_p - wt_p||_2 (sums of squares per chunk in
 * fp32, combined in double in a fixed order: deterministic); scratch >=
 * tal_prox_scratch_bytes(n_chunks, k).
 * tal_prox_grad: gw = s * sum_t (w - wt) / ||w - wt||_p and, for each non-null gwt_host[t],
 * gwt[t] = -s * (w - wt) / ||w - wt||_p, with 0 where a norm is 0 (torch's norm backward);
 * s = *scale_dev (the upstream gradient, read on the device).  Only the parameter segments
 * of gw / gwt are written.
 * All four passes (these two and the _bf16 pair below) check every argument, each of the k
 * neighbor pointers included, before the first launch. */
int64_t tal_prox_plan_words(const int64_t* seg_host, int32_t n_seg);
int32_t tal_prox_plan_build(const int64_t* seg_host, int32_t n_seg, int64_t* plan_host,
                            int64_t plan_capacity_words, int32_t* n_chunks);
int64_t tal_prox_scratch_bytes(int32_t n_chunks, int32_t k);
int32_t tal_prox_norms(const float* w, const float* const* wt_host, int32_t k,
                       const int64_t* plan_dev, int32_t n_chunks, int32_t n_seg, void* scratch,
                       float* norms_out, void* stream);
int32_t tal_prox_grad(const float* w, const float* const* wt_host, int32_t k,
                      const int64_t* plan_dev, int32_t n_chunks, int32_t n_seg,
                      const float* norms, const float* scale_dev, float* gw,
                      float* const* gwt_host, void* stream);
/* K4 on bf16 models (ABI 29): w, wt, gw and gwt are bf16 rows (uint16_t bit patterns; a device
 * ModelPool's b16 segment), offsets and lengths in elements; plans, tal_prox_scratch_bytes and
 * the error codes are the fp32 entry points'.  This is the project's definition (the reference
 * has no pinned bf16 arithmetic for the term): every value x is the bf16 parameter widened
 * exactly to fp32 (bits u << 16).
 * tal_prox_norms_bf16: norms_out[t*n_seg + p] = ||w_p - wt_p||_2 in fp32: squares accumulated
 * per lane in fp32 with fmaf, lanes, wavefronts and chunks combined in double in a fixed order,
 * one sqrt, one cast.  Deterministic; not bit for bit tal_prox_norms on the widened rows (the
 * packed loads give a lane other elements).
 * tal_prox_grad_bf16: per element exactly tal_prox_grad's fp32 operations in its order
 * (c_t = norm_t > 0 ? s / norm_t : 0; d_t = (w - wt_t) * c_t; g = ((0 + d_0) + d_1) + ...);
 * g and -d_t are rounded to bf16 once, to nearest even, at the store.  For the same `norms` the
 * result is the nearest-even bf16 rounding of what tal_prox_grad writes for the widened rows, for
 * any k.  With k > 64 (more than one launch) the running sum stays fp32 between the launches in
 * acc_scratch, acc_elems fp32 elements indexed like the rows, which must cover every plan chunk's
 * [begin, begin + length); it may be NULL when k <= 64, and k > 64 with NULL or with fewer
 * elements than the plan has chunks is TAL_ERR_INVALID (a chunk past acc_elems is never
 * touched).  Only the parameter segments of gw / gwt are written.
 * Rows that are all 8-byte aligned (pool rows are) are read and written 8 bytes per lane, the up
 * to 3 elements before and after a chunk's whole 8-byte groups one by one; other rows go element
 * by element (the same gradient bit for bit; the norms by the same definition, summed in that
 * path's own fixed order).  That element path is the one the fp32 entry points run: the kernels
 * are one template over the storage type. */
int32_t tal_prox_norms_bf16(const uint16_t* w, const uint16_t* const* wt_host, int32_t k,
                            const int64_t* plan_dev, int32_t n_chunks, int32_t n_seg,
                            void* scratch, float* norms_out, void* stream);
int32_t tal_prox_grad_bf16(const uint16_t* w, const uint16_t* const* wt_host, int32_t k,
                           const int64_t* plan_dev, int32_t n_chunks, int32_t n_seg,
                           const float* norms, const float* scale_dev, uint16_t* gw,
                           uint16_t* const* gwt_host, float* acc_scratch, int64_t acc_elems,
                           void* stream);

/* ---- Host reduction: processes that see no GPU ------------------------------------------
 * BASELINE config 1 runs the reference's driver with CPU models and no GPU
 * (decentralized_client.py:399-413 on CPU tensors).  These compute the same arithmetic as
 * tal_agg_f32 / tal_agg_i64 / tal_agg_bf16 (EXACT: bitwise the reference; FMA as documented
 * there) on HOST pointers, elementwise in operand order, on up to 16 host threads.  out may
 * alias any x[i].  The package calls them only when torch sees no GPU; with a GPU visible
 * every aggregation runs the kernels above. */
int32_t tal_host_agg_f32(const float* const* x_host, const double* w_host, int32_t m, float* out,
                         int64_t n, int32_t mode);
int32_t tal_host_agg_i64(const int64_t* const* x_host, const double* w_host, int32_t m, int64_t* out,
                         int64_t n);
int32_t tal_host_agg_bf16(const uint16_t* const* x_host, const double* w_host, int32_t m, uint16_t* out,
                          int64_t n, int32_t mode);

/* K2's cosine similarity on HOST pointers (replaces the reference's cosine_similarity,
 * src/decentralized_client.py:661-681, where it runs: on CPU tensors inside
 * sim_centrality_module_avg, :482-490, in a process without a GPU).  out[j] = cosine of the
 * flat fp32 parameter rows a_host[j] / b_host[j] under a plan from tal_cosine_plan_build (its
 * thread word set by tal_cosine_plan_set_threads): the same fp32 operations in the same order
 * as tal_cosine_params, i.e. torch's CPU order, bit for bit.  Up to 16 host threads. */
int32_t tal_host_cosine(const float* const* a_host, const float* const* b_host, int32_t n_pairs,
                        const int64_t* plan_host, float* out);
/* tal_cosine_round on a HOST pool (no GPU visible): every unique pair of the table once through
 * tal_host_cosine's arithmetic, out[j] for each ordered pair. */
int32_t tal_host_cosine_round(const float* pool_host, int64_t ld, const int64_t* plan_host,
                              const int32_t* table_host, const tal_cosine_round_info* info, float* out);
/* The two host forms on bf16 rows / a bf16 host pool (ABI 27; "K2 on bf16 models" above): bit for
 * bit tal_cosine_params_bf16 / tal_cosine_round_bf16. */
int32_t tal_host_cosine_bf16(const uint16_t* const* a_host, const uint16_t* const* b_host, int32_t n_pairs,
                             const int64_t* plan_host, float* out);
int32_t tal_host_cosine_round_bf16(const uint16_t* pool_host, int64_t ld, const int64_t* plan_host,
                                   const int32_t* table_host, const tal_cosine_round_info* info, float* out);

/* ---- Synthetic pool rows (test / benchmark inputs) --------------------------
 * Not a reference interface: the reference trains its models; the benchmark and the full-size
 * parity tests need seeded models whose outputs the reference-generated sha256 fixtures pin
 * (tests/golden/full_round_c{3,4,5}_*.json).  Fills n_rows rows (pitch ld elements) of one pool
 * segment with synth.py's counter generator: element at generator position p of the row seeded
 * s is u = splitmix64(p ^ (s & 0xFFFFFFFF) << 40) turned into fp32 (dtype 0: sign bit 31,
 * exponent 121 + bits 23..25, mantissa bits 0..22; |v| + 0.5 in the running_var ranges), bf16
 * (dtype 1: that fp32 value rounded to nearest even) or int64 (dtype 2: u % hi).
 * table (int64, on the device; the host copy passed too): {n_rows, n, n_runs, n_rv, hi, 0, 0, 0},
 * seeds[n_rows], runs[n_runs] {generator position, first column, length} tiling columns
 * [0, n) in order, running_var ranges[n_rv] {first column, length} ascending (dtype 0 only).
 * One launch for the whole segment (the torch form took ~20 element-wise launches per 32 M
 * elements per row). */
int32_t tal_fill_counter(void* seg, int64_t ld, int32_t dtype, const int64_t* table_dev,
                         const int64_t* table_host, void* stream);

/* ---- Multi-GPU halo exchange (SURVEY §8(b) tal_halo_exchange, §8(e)) ---------------------
 * Reference: the models that cross workers are shipped by Parsl as Python objects
 * (decentralized_app.py:627-629, parsl_setup.py:191-203).  Sharded one process per GPU, each
 * rank needs the neighbor models other ranks own: per ordered pair (g -> h) the unique set of
 * g's rows that h's rows reference, sent once.  One RCCL communicator per process, made from a
 * unique id that rank 0 creates and the caller broadcasts (any channel: torch.distributed, a
 * file, MPI); tal_comm_init selects `device` for the communicator and restores the caller's
 * current device.
 *
 * tal_halo_pack gathers rows rows_dev[0..n_rows) (device int32, rows < pool_rows; others are
 * skipped) of a pool segment (row pitch ld_bytes) into buf, row_bytes each, back to back: the
 * message for one peer.  tal_halo_exchange posts in one RCCL group on `stream` a send of
 * send_bytes[p] bytes from send_bufs[p] and a receive of recv_bytes[p] bytes into recv_bufs[p]
 * for every peer p in [0, world) with a non-zero count (p == own rank: a local copy through
 * RCCL).  A peer's rows arrive back to back, so a contiguous block of ghost rows of the
 * receiving pool (its halo rows are grouped by owner) is a valid receive buffer and the round
 * kernels read it in place.  world must equal the communicator's size. */
#define TAL_COMM_ID_BYTES 128
int32_t tal_comm_unique_id(void* id_out);
int32_t tal_comm_init(void** comm_out, int32_t world, int32_t rank, const void* id, int32_t device);
int32_t tal_comm_destroy(void* comm);
int32_t tal_halo_pack(const void* pool, int64_t ld_bytes, int64_t pool_rows, const int32_t* rows_dev,
                      int32_t n_rows, int64_t row_bytes, void* buf, void* stream);
int32_t tal_halo_exchange(void* comm, int32_t world, const void* const* send_bufs,
                          const int64_t* send_bytes, void* const* recv_bufs,
                          const int64_t* recv_bytes, void* stream);

/* One process driving several GPUs (TAL_GPUS: the reference's single coordinator process,
 * decentralized_app.py:605-641 / parsl_setup.py:75-78, with its clients' models spread over the
 * node's GPUs).  tal_comm_init_local makes n communicators together, rank r on devices[r]
 * (ncclCommInitAll; distinct devices).  tal_halo_exchange_local posts, in ONE RCCL group (a thread
 * driving several ranks must group them), for every local rank r and peer p with a non-zero count:
 * a send of send_bytes[r n + p] bytes from send_bufs[r n + p] and a receive of recv_bytes[r n + p]
 * bytes into recv_bufs[r n + p], on rank r's stream streams[r].  The buffers obey
 * tal_halo_exchange's rules (a contiguous block of ghost rows is a valid receive buffer). */
int32_t tal_comm_init_local(void** comms_out, int32_t n, const int32_t* devices);
int32_t tal_halo_exchange_local(void* const* comms, int32_t n, const void* const* send_bufs,
                                const int64_t* send_bytes, void* const* recv_bufs,
                                const int64_t* recv_bytes, void* const* streams);

#ifdef __cplusplus
}
#endif

#endif /* TAL_AGG_H */
