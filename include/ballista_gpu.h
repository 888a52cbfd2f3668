/* ballista_gpu.h — C ABI of the MI355X-native Ballista stage-executor
 * library (libballista_gpu.so).
 *
 * This is the device boundary of SURVEY.md §8(b), seam 3: the thin
 * `extern "C"` FFI a Rust `GpuExecutionEngine` (implementing Ballista's
 * `ExecutionEngine` trait, ballista/executor/src/execution_engine.rs:53-103,
 * injected via `Executor::new` arg 8 / `ExecutorProcessConfig.
 * override_execution_engine`, executor_process.rs:319) binds to run the
 * executor-side physical-operator hot path on a gfx950 GPU.  The Rust-side
 * binding stub a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions:
 *  - All functions return BG_OK (0) or a negative bg_status code;
 *    bg_last_error() returns a thread-local message for the last failure.
 *  - Column buffers are Arrow C-Data-Interface-style: raw data pointer +
 *    optional validity bitmap (LSB bit order) + length.  Pointers named d_*
 *    are DEVICE pointers owned by the caller (allocated via bg_malloc);
 *    the library never frees caller memory.
 *  - There is no CPU fallback anywhere behind this ABI: every compute entry
 *    point requires an initialised HIP device and fails loudly otherwise.
 *
 * Reference interfaces each entry point replaces (file:line under
 * /root/reference):
 *  - bg_hash_columns / bg_partition_ids / bg_partition_indices:
 *      compute_partition_indices,
 *      ballista/core/src/execution_plans/sort_shuffle/writer.rs:1259-1279
 *      (evaluate key exprs -> create_hashes(REPARTITION_RANDOM_STATE) ->
 *       h % K -> per-partition row-index lists).
 *  - bg_eval_predicates / bg_mask_to_indices / bg_gather:
 *      DataFusion 55 FilterExec predicate eval + filter compaction and the
 *      sort-shuffle writer's interleave-gather
 *      (sort_shuffle/partitioned_batch_iterator.rs; SURVEY.md §8a rows 1,5).
 *  - bg_hash_repartition: the device half of
 *      SortShuffleWriterExec::execute_shuffle_write (writer.rs:564-753) —
 *      bucket rows by partition and materialise partition-major column
 *      buffers; IPC encode + file write stay host-side
 *      (write_task_consolidated writer.rs:810-895 + index.rs:21-33).
 *  - bg_q6_agg: the fused Filter+Partial-Aggregate stage of TPC-H q6
 *      (plan golden scheduler/tests/tpch_plan_stability/approved/q6.txt;
 *       SUM(Decimal128) exact i128 per DataFusion AggregateExec).
 *  - bg_q1_agg: the fused Filter+Partial-Aggregate stage of TPC-H q1
 *      (approved/q1.txt; grouped sums/counts, groups dictionary-encoded).
 */

#ifndef BALLISTA_GPU_H
#define BALLISTA_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status ---- */
typedef enum {
  BG_OK = 0,
  BG_ERR_HIP = -1,        /* HIP runtime failure (see bg_last_error) */
  BG_ERR_NO_GPU = -2,     /* no usable gfx950 device / not initialised */
  BG_ERR_INVALID = -3,    /* bad argument */
  BG_ERR_UNSUPPORTED = -4 /* dtype/op not yet accelerated */
} bg_status;

const char* bg_last_error(void);
int bg_version(void);
/* sha256 over the library's own sources, injected at compile time by the
 * build entry; "unverified-local-build" when compiled without it.  A CPU
 * test compares it against a fresh hash of the committed sources so a
 * stale committed binary is detected. */
const char* bg_source_hash(void);
/* duration (ms) of the most recent fused-aggregate kernel launch, measured
 * with hipEvents on the launch stream — roofline evidence for bench.py */
double bg_last_kernel_ms(void);

/* ---- device/session ---- */
int bg_init(int device_ordinal); /* fails loudly when no GPU is present */
int bg_device_count(int* out);
int bg_synchronize(void);

/* ---- device memory (caller-owned) ---- */
int bg_malloc(uint64_t bytes, void** d_ptr); /* pooled; see bg_pool_trim */
int bg_free(void* d_ptr);
int bg_memset(void* d_ptr, int value, uint64_t bytes);
int bg_memcpy_h2d(void* d_dst, const void* h_src, uint64_t bytes);
int bg_memcpy_d2h(void* h_dst, const void* d_src, uint64_t bytes);
int bg_memcpy_dtod(void* d_dst, const void* d_src, uint64_t bytes);
/* release the allocator pool's cached device memory back to HIP */
int bg_pool_trim(void);
/* allocator pool accounting (any out pointer may be NULL): live = buffers
 * handed out (bg_malloc included) and not yet released, cached = bytes
 * parked in the pool's free lists, which bg_pool_trim gives back */
int bg_pool_stats(int64_t* live_bytes, int64_t* live_buffers,
                  int64_t* cached_bytes);

/* ---- columns ---- */
typedef enum {
  BG_DT_INT32 = 1,
  BG_DT_INT64 = 2,
  BG_DT_DATE32 = 3,      /* Arrow Date32: i32 days since epoch */
  BG_DT_DECIMAL128 = 4,  /* Arrow Decimal128: 16-byte LE two's complement */
  BG_DT_DICT8 = 5,       /* dictionary codes as u8 (small Utf8 dictionaries) */
  BG_DT_UTF8 = 6,        /* Arrow Utf8: i32 offsets (d_offsets) + byte data */
  BG_DT_FLOAT64 = 7,     /* f64; predicates/aggregates at 1e-6 rel tolerance */
} bg_dtype;

typedef struct {
  int32_t dtype;          /* bg_dtype */
  int32_t precision;      /* decimals only */
  int32_t scale;          /* decimals only */
  int32_t _pad;
  const void* d_data;     /* device pointer; UTF8: byte data buffer */
  const uint8_t* d_validity; /* device pointer or NULL (all valid); LSB bits */
  const int32_t* d_offsets;  /* UTF8 only: n+1 Arrow offsets; else NULL */
  int64_t len;
} bg_column;

/* ---- predicates (FilterExec subset; ops shared with the oracle) ---- */
typedef enum {
  BG_PRED_GE_LT = 0,   /* lo <= x <  hi */
  BG_PRED_BETWEEN = 1, /* lo <= x <= hi */
  BG_PRED_LT = 2,      /* x <  hi */
  BG_PRED_EQ = 3,      /* x == lo */
  BG_PRED_GT = 4,      /* x >  lo */
} bg_pred_op;

typedef struct {
  int32_t column; /* index into the cols array */
  int32_t op;     /* bg_pred_op */
  /* bounds as i128 split into (lo64, hi64); narrower dtypes use the low part */
  int64_t lo_lo; int64_t lo_hi;
  int64_t hi_lo; int64_t hi_hi;
} bg_pred;

/* AND-fold `npreds` predicates over `cols` into an Arrow LSB bitmask
 * d_mask (ceil(n/64)*8 bytes, 8-byte aligned). Null input => false. */
int bg_eval_predicates(const bg_column* cols, int32_t ncols,
                       const bg_pred* preds, int32_t npreds,
                       int64_t n, uint8_t* d_mask);

/* Stable compaction: selection bitmask -> ascending row indices.
 * d_indices capacity n; *out_count receives the selected count. */
int bg_mask_to_indices(const uint8_t* d_mask, int64_t n, uint32_t* d_indices,
                       int64_t* out_count);

/* Row gather (take): d_dst[i] = d_src[d_idx[i]], elem_size in {1,2,4,8,16}. */
int bg_gather(const void* d_src, int64_t elem_size, const uint32_t* d_idx,
              int64_t m, void* d_dst);

/* Variable-length (Utf8/Binary) gather: m rows by index -> Arrow i32
 * offsets (m+1) + packed bytes (the writer's take/interleave for string
 * payload columns). */
int bg_gather_varlen(const void* d_src_data, const int32_t* d_src_offsets,
                     const uint32_t* d_idx, int64_t m,
                     int32_t* d_out_offsets, void* d_out_data,
                     int64_t out_data_cap, int64_t* out_total_bytes);

/* Arrow i32 offset rebase (writer-side partition slicing). */
int bg_sub_i32(const void* d_src, int64_t n, int32_t sub, void* d_out);

/* Validity-bitmap gather: out bit i = valid[idx[i]] (Arrow LSB order;
 * d_out_bits holds ceil(m/64)*8 bytes) — take for null-carrying columns. */
int bg_gather_bits(const uint8_t* d_valid, const uint32_t* d_idx, int64_t m,
                   uint8_t* d_out_bits);

/* LIKE / NOT LIKE over a Utf8 column, ANDed into an existing Arrow LSB
 * bitmask (q9/q13/q14/q16-class predicates: in-order literal fragments
 * with optional start/end anchors — the forms the reference's
 * approved plans use; no '_' wildcards there). */
int bg_eval_like(const bg_column* col, const char* const* terms,
                 const int32_t* term_lens, int32_t nterms,
                 int32_t anchor_prefix, int32_t anchor_suffix,
                 int32_t negate, int64_t n, uint8_t* d_mask);

/* CASE WHEN mask THEN a ELSE b: elementwise select (esz 1..16). */
int bg_select(const uint8_t* d_mask, const void* d_a, const void* d_b,
              int64_t esz, int64_t n, void* d_out);
/* constant fill (literal CASE branches): value as i128 (lo, hi). */
int bg_fill_const(void* d_out, int64_t n, int64_t esz, int64_t lo,
                  int64_t hi);

/* x IN {v0..v15} over integer/dict columns, ANDed into an existing
 * bitmask (q12/q19-class IN-lists). */
int bg_eval_in(const bg_column* col, const int64_t* values, int32_t nvalues,
               int64_t n, uint8_t* d_mask);
/* out = a OR b (disjunctive predicate groups, q19's OR-of-ANDs). */
int bg_bitmap_or(const uint8_t* d_a, const uint8_t* d_b, int64_t nbits,
                 uint8_t* d_out);

/* ---- scalar expressions beyond Decimal128 arithmetic and column-vs-
 * literal predicates.  Null semantics as everywhere: a predicate over a
 * NULL input is false; a projection leaves validity to the caller (share
 * the input's bitmap); value bytes under a NULL are unspecified. ---- */

/* date_part(part, Date32) -> Int32, as DataFusion 55's date_part on Date32
 * (approved/q7.txt:67, q8.txt:93, q9.txt:65: ProjectionExec
 * date_part(YEAR, o_orderdate) as o_year, then GROUP BY it).  Proleptic
 * Gregorian with floor division: exact for every int32 day number, before
 * 1970 and before year 0 included.  d_out: n x 4 B.  Other parts return
 * BG_ERR_UNSUPPORTED, a non-Date32 column BG_ERR_INVALID. */
#define BG_DATE_PART_YEAR 0
#define BG_DATE_PART_QUARTER 1
#define BG_DATE_PART_MONTH 2
#define BG_DATE_PART_DAY 3
#define BG_DATE_PART_DOY 4      /* 1..366 */
#define BG_DATE_PART_DOW 5      /* Sunday = 0, as DataFusion */
int bg_date_part(const bg_column* col /* DATE32 */, int32_t part, int64_t n,
                 int32_t* d_out);

/* substr(str, start[, count]) over a Utf8 column, as DataFusion's substr
 * (approved/q22.txt:3,13,16: substr(c_phone, 1, 2) as filter operand and
 * as the projected GROUP BY key cntrycode).  1-based, counted in UTF-8
 * CODE POINTS: with s = start-1 and e = has_count ? s+count : len the
 * result is code points [clamp(s,0,len), clamp(e,0,len)) — start <= 0
 * eats into the count, start > len gives ''.  count < 0 is refused
 * (BG_ERR_INVALID, "negative substring length not allowed").  NULL rows
 * produce zero bytes.  Outputs as bg_gather_varlen: Arrow i32 offsets
 * (n+1) + packed bytes; d_out_data == NULL is a sizing call returning
 * *out_total_bytes; a total above 2 GiB is BG_ERR_INVALID.  Cost per row
 * is O(start+count) bytes walked, not O(len). */
int bg_substr(const bg_column* col /* UTF8 */, int64_t start, int32_t has_count,
              int64_t count, int64_t n, int32_t* d_out_offsets /* n+1 */,
              void* d_out_data, int64_t out_data_cap, int64_t* out_total_bytes);

/* a <cmp> b between two COLUMNS, ANDed into an existing bitmask
 * (approved/q4.txt:8, q12.txt:3, q21.txt:7,53: FilterExec
 * l_receiptdate > l_commitdate, l_shipdate < l_commitdate on the lineitem
 * scan).  Same dtype on both sides, one of INT32/DATE32/INT64/DICT8/
 * DECIMAL128 (signed i128; equal scale required, the plan serialiser
 * presents coerced types); FLOAT64/UTF8 return BG_ERR_UNSUPPORTED.  Words
 * of d_mask that are already zero cost no column traffic, so run the
 * literal predicates first.  Bits at or beyond n come out 0. */
#define BG_CMP_LT 0
#define BG_CMP_LE 1
#define BG_CMP_GT 2
#define BG_CMP_GE 3
#define BG_CMP_EQ 4
#define BG_CMP_NE 5
int bg_eval_compare_cols(const bg_column* a, const bg_column* b, int32_t cmp,
                         int64_t n, uint8_t* d_mask);

/* x IN {v0..v15} over a Utf8 column by exact byte equality, ANDed into an
 * existing bitmask (approved/q22.txt:3,16: substr(c_phone, 1, 2) IN
 * ('13', '31', ...)).  1..16 literals of 1..64 bytes each. */
int bg_eval_in_utf8(const bg_column* col, const char* const* values,
                    const int32_t* value_lens, int32_t nvalues, int64_t n,
                    uint8_t* d_mask);

/* ---- CAST, Float64 arithmetic and Decimal128 division.  Some of these can
 * fail on a row, as they fail the query in DataFusion (casts run with
 * safe=false, decimal division raises DivideByZero).  A fallible call counts
 * the failing VALID rows, returns BG_ERR_INVALID with a message naming the
 * failure and the count ("cast: 3 of 1000 rows overflow Decimal128(19,6)",
 * "div: division by zero in 1 row") and stores the count to *out_failed
 * (may be NULL; 0 on success).  d_out is then unspecified.  Rows that are
 * NULL by the input validity are never examined: a zero divisor or garbage
 * under a NULL fails nothing.  The output's validity is the input's (the
 * AND of both inputs' for a binary call); the caller shares or combines
 * the bitmaps. ---- */

/* CAST(src AS to_dtype[(to_precision, to_scale)]).  d_out: n rows of the
 * target's width.  Pairs:
 *  - INT32 / INT64 / DECIMAL128(p,s) -> FLOAT64 (approved/q14.txt:22,
 *    q17.txt:27,33, q11.txt:70, q20.txt:49: CAST(sum(..) AS Float64)).
 *    Integers as (double)x; a decimal as (double)x / P10[s], where
 *    (double) of the i128 rounds once to nearest-even and P10 is the table
 *    of the correctly rounded doubles 1e0..1e38.  arrow-rs computes
 *    x as f64 / 10f64.powi(s): identical for s <= 22, where every power is
 *    exact; beyond that powi may differ from the table in the last bit,
 *    which has not been compared against a Rust build.
 *  - FLOAT64 -> DECIMAL128(p,s) (q17.txt:27, q11.txt:70):
 *    r = round(v * P10[s]) with C round() (half away from zero); a row
 *    fails when v is NaN or +-inf or |r| >= 10^p.
 *  - DECIMAL128(p1,s1) -> DECIMAL128(p2,s2) (q17.txt:19, q11.txt:74,
 *    q22.txt:18): x * 10^(s2-s1) for s2 >= s1, else x / 10^(s1-s2) rounded
 *    half away from zero (arrow-rs decimal-to-decimal); a row fails when
 *    |result| >= 10^p2.
 *  - INT32 / INT64 -> DECIMAL128(p,s): x * 10^s, same check.
 *  - INT32 -> INT64.
 * Any other pair returns BG_ERR_UNSUPPORTED before anything is allocated.
 * A conversion that cannot fail launches no failure counter and reads
 * nothing back: anything to FLOAT64, INT32 -> INT64, and a decimal target
 * wide enough for every input of the source's declared precision (10 and
 * 19 digits for INT32 / INT64; a source precision outside 1..38 counts as
 * unknown and is checked). */
int bg_cast(const bg_column* src, int32_t to_dtype, int32_t to_precision,
            int32_t to_scale, int64_t n, void* d_out, int64_t* out_failed);

/* Float64 arithmetic (q14.txt:22: 100 * a / b; q17.txt:33: a / 7;
 * q17.txt:27, q20.txt:49: 0.2 * a, 0.5 * a; q11.txt:70: a * 0.0001).  Each
 * result is exactly one IEEE-754 binary64 operation; division by zero
 * yields inf or NaN as arrow's float div does and is no failure.  The
 * column ops take a and b, the literal ops take a and lit (b ignored).  A
 * non-FLOAT64 column returns BG_ERR_INVALID. */
#define BG_F64_MUL 0     /* a * b */
#define BG_F64_ADD 1     /* a + b */
#define BG_F64_SUB 2     /* a - b */
#define BG_F64_DIV 3     /* a / b */
#define BG_F64_MUL_LIT 4 /* a * lit */
#define BG_F64_ADD_LIT 5 /* a + lit */
#define BG_F64_LIT_SUB 6 /* lit - a */
#define BG_F64_DIV_LIT 7 /* a / lit */
#define BG_F64_LIT_DIV 8 /* lit / a */
int bg_project_f64(int32_t op, const bg_column* a, const bg_column* b,
                   double lit, int64_t n, double* d_out);

/* Decimal128 / Decimal128 (q8.txt:103: sum(case..) / sum(volume) as
 * mkt_share), arrow-rs's decimal div: plain i128 division, truncated toward
 * zero, after aligning scales.  mul_pow >= 0: (a * 10^mul_pow) / b;
 * mul_pow < 0: a / (b * 10^-mul_pow); for a result of scale S over inputs
 * of scales s1 and s2, mul_pow = S - s1 + s2.  A valid row (valid in a AND
 * in b) fails when b == 0 or when the scaled operand leaves i128.  d_out:
 * n x 16 B.  |mul_pow| > 38 or a non-DECIMAL128 column: BG_ERR_INVALID. */
int bg_div_dec128(const bg_column* a, const bg_column* b, int32_t mul_pow,
                  int64_t n, void* d_out, int64_t* out_failed);

/* ---- hash repartition (SortShuffleWriterExec device half) ---- */

/* create_hashes restatement over the key columns (bg_ahash.h; parity
 * unpinned for the ahash seed constants — SURVEY.md §8c). */
int bg_hash_columns(const bg_column* key_cols, int32_t nkeys, int64_t n,
                    uint64_t* d_hashes);

/* pid[i] = hash[i] % k  (writer.rs:1274-1276) */
int bg_partition_ids(const uint64_t* d_hashes, int64_t n, uint32_t k,
                     uint32_t* d_pids);

/* Stable multi-split: partition-major row-index lists, ascending row order
 * inside each partition — the device equivalent of the Vec<Vec<u32>> that
 * compute_partition_indices returns.  d_indices: n entries; d_offsets: k+1
 * exclusive prefix (offsets[k] == n).  k <= 4096. */
int bg_partition_indices(const uint32_t* d_pids, int64_t n, uint32_t k,
                         uint32_t* d_indices, int64_t* d_offsets);

/* As bg_partition_indices, also emitting the inverse permutation
 * d_rank[row] = output position (coalesced write) — feeds
 * bg_scatter_rows so payload materialisation reads inputs sequentially. */
int bg_partition_indices_ex(const uint32_t* d_pids, int64_t n, uint32_t k,
                            uint32_t* d_indices, int64_t* d_offsets,
                            uint32_t* d_rank);

/* Scatter-materialise: d_dst[d_rank[i]] = d_src[i] (sequential reads,
 * partition-major writes — the write-side dual of bg_gather, avoiding the
 * gather's k-fold read amplification on permuted input). */
int bg_scatter_rows(const void* d_src, int64_t elem_size,
                    const uint32_t* d_rank, int64_t n, void* d_dst);

/* Fused convenience: hash + pids + stable split + gather every payload
 * column partition-major.  d_out[c] must hold len*elem_size(c) bytes; rows
 * of partition p for column c live at [offsets[p]*esz, offsets[p+1]*esz).
 * offsets (k+1, device) and the permutation d_indices are also returned so
 * the host can slice buffers for IPC encoding. */
int bg_hash_repartition(const bg_column* key_cols, int32_t nkeys,
                        const bg_column* payload_cols, int32_t ncols,
                        int64_t n, uint32_t k,
                        uint32_t* d_indices, int64_t* d_offsets,
                        void** d_out /* ncols device pointers */);

/* ---- HashJoinExec build/probe (INNER equi-join, Int64 keys) ----
 * Replaces DataFusion 55 HashJoinExec's build/probe arithmetic for
 * partitioned hash joins (planned when
 * `prefer_hash_join=true`, core/src/extension.rs:850-858 + the opt-in test
 * client/tests/context_checks.rs:1034-1063).  Contract: the emitted
 * (probe_idx, build_idx) pair MULTISET equals the reference's inner-join
 * result set; pairs are probe-major (ascending probe_idx, exact per-row
 * offsets from the count phase); chain order within one probe row is
 * unspecified, as in the reference (SQL does not pin intra-row order). */
int bg_hashjoin_build(const bg_column* build_keys, int64_t n_build,
                      void** out_handle);
int bg_hashjoin_probe_count(void* handle, const bg_column* probe_keys,
                            int64_t n_probe, int64_t* out_matches);
int bg_hashjoin_probe_fill(void* handle, const bg_column* probe_keys,
                           int64_t n_probe, uint32_t* d_out_probe,
                           uint32_t* d_out_build);
int bg_hashjoin_free(void* handle);

/* ---- generalized hash join (round 2): multi-column keys over
 * Int64/Int32/Date32/Decimal128/Utf8/dict8 and the probe-side join types
 * of DataFusion's HashJoinExec (q2/q9-class shapes).  Nodes store
 * {hash, next}; equality is the cross-table key compare.  Join null
 * semantics (null_equals_null=false): a row with ANY null key matches
 * nothing — excluded by INNER/SEMI, emitted by ANTI/OUTER_PROBE with
 * build id BG_JOIN_NULL_IDX.  The build-key device buffers must outlive
 * the handle (nodes reference them for compares). */
#define BG_JOIN_INNER 0
#define BG_JOIN_SEMI 1        /* probe rows with >=1 match, emitted once */
#define BG_JOIN_ANTI 2        /* probe rows with no match */
#define BG_JOIN_OUTER_PROBE 3 /* matches + unmatched probe rows */
#define BG_JOIN_NULL_IDX 0xFFFFFFFFu
int bg_hashjoin_build2(const bg_column* keys, int32_t nkeys, int64_t n,
                       void** out_handle);
int bg_hashjoin_probe_count2(void* handle, const bg_column* keys,
                             int32_t nkeys, int64_t n, int32_t join_type,
                             int64_t* out_matches);
int bg_hashjoin_probe_fill2(void* handle, const bg_column* keys,
                            int32_t nkeys, int64_t n, int32_t join_type,
                            uint32_t* d_out_probe, uint32_t* d_out_build);
int bg_hashjoin_free2(void* handle);

/* ---- build-side-preserving join types ----
 * DataFusion 55 HashJoinExec always builds on its LEFT input and tracks a
 * per-build-row "visited" bitmap for the types that preserve it
 * (joins/hash_join.rs: visited_left_side, emitted after the last probe
 * batch).  With build = DataFusion's left input these restate LeftSemi /
 * LeftAnti / Left / Full; SEMI/ANTI/OUTER_PROBE above are its RightSemi /
 * RightAnti / Right.  The handle owns one visited bit per build row (Arrow
 * LSB order, ((n_build+63)/64)*8 + 8 bytes), allocated and zeroed by the
 * first marking call, accumulated over every later one, released by
 * bg_hashjoin_free2.  Null semantics as above: a build row with any null
 * key is never inserted, so never marked (ANTI_BUILD / OUTER_BUILD /
 * OUTER_FULL emit it, SEMI_BUILD does not); a probe row with any null key
 * marks nothing. */
#define BG_JOIN_SEMI_BUILD  4  /* DataFusion LeftSemi: build rows with >=1 match, once */
#define BG_JOIN_ANTI_BUILD  5  /* DataFusion LeftAnti: build rows with no match        */
#define BG_JOIN_OUTER_BUILD 6  /* DataFusion Left:  inner pairs + unmatched build rows */
#define BG_JOIN_OUTER_FULL  7  /* DataFusion Full:  OUTER_PROBE pairs + unmatched build rows */
/* bg_hashjoin_probe_count2/_fill2 take types 6 and 7: the pairs are those
 * of INNER / OUTER_PROBE, and fill2 also marks every matched build row;
 * the unmatched build rows come from bg_hashjoin_build_rows2(matched=0)
 * after the last probe chunk.  Types 4 and 5 emit no pairs: count2/fill2
 * refuse them with BG_ERR_INVALID and point at bg_hashjoin_probe_mark2.
 * Every probe entry of this family, with or without a filter, refuses with
 * BG_ERR_INVALID, before anything is allocated or launched: a NULL handle
 * (bg_hashjoin_free2(NULL) stays BG_OK), probe keys whose count or dtypes
 * differ from the build's, and, in count and fill, a join_type outside
 * BG_JOIN_INNER .. BG_JOIN_OUTER_FULL. */

/* HashJoinExec's probe-side pass for LeftSemi/LeftAnti, where only the
 * visited bitmap matters: mark only; emits nothing (types 4/5 need no pair
 * buffers). Callable once per probe chunk. */
int bg_hashjoin_probe_mark2(void* handle, const bg_column* keys, int32_t nkeys,
                            int64_t n);

/* HashJoinExec's final build-side emission (get_final_indices_from_bit_map):
 * build rows whose visited bit == matched (0/1), ascending build index.
 * d_out_build == NULL: count only. Bits at or beyond n_build are never
 * reported. Valid before any marking call (then: nothing is matched). */
int bg_hashjoin_build_rows2(void* handle, int32_t matched, int64_t* out_count,
                            uint32_t* d_out_build);

/* ---- join residual filters ----
 * DataFusion 55 HashJoinExec with `filter: Some(JoinFilter)` (wire format:
 * JoinFilter, datafusion.proto:1402; HashJoinExecNode.filter = 8,
 * datafusion.proto:1189; approved/q21.txt:60-61, q7.txt, q19.txt).  A
 * CANDIDATE is a (build row, probe row) pair with equal non-NULL keys, as
 * above; it PASSES when the filter is TRUE (NULL counts as FALSE), and
 * every join type then reads "match" as "passing candidate": SEMI emits a
 * probe row with >=1 passing candidate (the walk goes on past failing
 * ones), ANTI one with none, the outer types extend rows without one, and
 * only passing candidates set a build row's visited bit.
 *
 * The filter is an OR of up to BG_JOIN_FILTER_MAX_GROUPS groups, each an
 * AND of its terms, handed over as a flat array of terms.  A group holds at
 * most one build mask, one probe mask and BG_JOIN_FILTER_MAX_CROSS cross
 * compares; group ids are dense from 0.  Single-side predicates are
 * evaluated by the caller into masks (bg_eval_predicates and its kin); a
 * cross compare follows bg_eval_compare_cols: equal dtypes among
 * Int32/Int64/Date32/Decimal128 (signed i128; equal scales are the
 * caller's to check)/dict8, a NULL on either side fails the term. */
#define BG_JOIN_FILTER_MAX_GROUPS 4
#define BG_JOIN_FILTER_MAX_CROSS 4
#define BG_JF_CROSS 0       /* d_build[build row] <cmp> d_probe[probe row] */
#define BG_JF_BUILD_MASK 1  /* d_build: Arrow LSB bitmap over the build rows */
#define BG_JF_PROBE_MASK 2  /* d_probe: Arrow LSB bitmap over THIS call's probe rows */
typedef struct {
  int32_t kind;   /* BG_JF_* */
  int32_t group;  /* 0 .. BG_JOIN_FILTER_MAX_GROUPS-1 */
  int32_t dtype;  /* BG_JF_CROSS: bg_dtype of both columns */
  int32_t cmp;    /* BG_JF_CROSS: BG_CMP_* */
  const void* d_build;             /* cross: build column data; build mask */
  const uint8_t* d_build_validity; /* cross: or NULL (all valid) */
  const void* d_probe;             /* cross: probe column data; probe mask */
  const uint8_t* d_probe_validity; /* cross: or NULL (all valid) */
} bg_join_filter_term;

/* bg_hashjoin_probe_count2 / _fill2 / _mark2 with a filter; join_type as
 * there (count/fill refuse types 4 and 5, mark serves them).  The fill
 * call must repeat the count call's terms.  nterms == 0 is BG_ERR_INVALID:
 * a join without a filter goes through the unfiltered entries. */
int bg_hashjoin_probe_count2_filtered(void* handle, const bg_column* keys,
                                      int32_t nkeys, int64_t n,
                                      int32_t join_type,
                                      const bg_join_filter_term* terms,
                                      int32_t nterms, int64_t* out_matches);
int bg_hashjoin_probe_fill2_filtered(void* handle, const bg_column* keys,
                                     int32_t nkeys, int64_t n,
                                     int32_t join_type,
                                     const bg_join_filter_term* terms,
                                     int32_t nterms, uint32_t* d_out_probe,
                                     uint32_t* d_out_build);
int bg_hashjoin_probe_mark2_filtered(void* handle, const bg_column* keys,
                                     int32_t nkeys, int64_t n,
                                     const bg_join_filter_term* terms,
                                     int32_t nterms);

/* ---- nested-loop join ----
 * DataFusion 55 NestedLoopJoinExec (wire format: NestedLoopJoinExecNode,
 * datafusion.proto:1359-1365; approved/q11.txt:69, q22.txt:14): a join
 * without equi-keys, so EVERY (build row, probe row) pair is a candidate and
 * the JoinFilter alone decides which pass.  Build = its left input, as in
 * the hash joins; join types, "match = passing candidate", the visited
 * bitmap and BG_JOIN_NULL_IDX read as in the bg_hashjoin_*2 family.  There
 * are no keys and so no key-NULL rule: the only NULL rule is the filter's
 * (a NULL on either side of a cross compare fails that term).
 *
 * PAIR ORDER is fixed: ascending probe row, and within a probe row ascending
 * build row (SEMI emits the lowest passing build row).  An unmatched probe
 * row (ANTI / OUTER_PROBE / OUTER_FULL) carries BG_JOIN_NULL_IDX.
 *
 * The handle holds no table, only the offsets between a count and its fill
 * and one visited bit per build row (layout and lifetime of
 * bg_hashjoin_build_rows2: lazily allocated by the first marking call,
 * accumulated over every later one, bits at or beyond n_build never
 * reported).  terms/nterms as in bg_hashjoin_probe_*2_filtered, with the
 * same limits and messages, except that nterms == 0 is allowed here: every
 * pair passes (CrossJoinExec).  The columns and masks the terms point at
 * carry the rows; the calls take only the row counts.
 *
 * Work is n_build candidates per probe row and parallel over probe rows
 * only: a one-row probe side against a large build side runs serially.
 * DataFusion puts the smaller input on the build side.
 *
 * Every entry refuses with BG_ERR_INVALID, before anything is allocated or
 * launched: a NULL handle (bg_nljoin_free(NULL) stays BG_OK), a negative
 * row count, n_build >= 2^32 - 1 (build rows travel as u32, the last value
 * is BG_JOIN_NULL_IDX), and, in count and fill, a join_type outside
 * BG_JOIN_INNER .. BG_JOIN_OUTER_FULL, types 4 and 5 (no pairs: call
 * bg_nljoin_mark, then bg_nljoin_build_rows) and a fill whose n_probe,
 * join_type or terms differ from the last count's. */
int bg_nljoin_open(int64_t n_build, void** out_handle);
int bg_nljoin_count(void* handle, int64_t n_probe, int32_t join_type,
                    const bg_join_filter_term* terms, int32_t nterms,
                    int64_t* out_matches);
int bg_nljoin_fill(void* handle, int64_t n_probe, int32_t join_type,
                   const bg_join_filter_term* terms, int32_t nterms,
                   uint32_t* d_out_probe, uint32_t* d_out_build);
/* types 4/5 (and any chunk whose pairs are not wanted): mark only */
int bg_nljoin_mark(void* handle, int64_t n_probe,
                   const bg_join_filter_term* terms, int32_t nterms);
/* as bg_hashjoin_build_rows2 */
int bg_nljoin_build_rows(void* handle, int32_t matched, int64_t* out_count,
                         uint32_t* d_out_build);
int bg_nljoin_free(void* handle);

/* Split an index vector carrying BG_JOIN_NULL_IDX sentinels (probe-outer
 * build side) into a clamped gather-safe vector + the validity bitmap of
 * non-sentinel slots. */
int bg_idx_sentinel(const uint32_t* d_idx, int64_t m, uint32_t* d_clamped,
                    uint8_t* d_valid_bits);
/* out = a AND b over ceil(nbits/8) bytes (combine validity bitmaps). */
int bg_bitmap_and(const uint8_t* d_a, const uint8_t* d_b, int64_t nbits,
                  uint8_t* d_out);

/* ---- general hash group-by (AggregateExec Partial/Single) ----
 * Arbitrary group cardinality (q3-class: millions of groups).  Aggregate
 * ops: 0 = SUM over Decimal128 (exact i128), 1 = SUM over Int64 (exact,
 * accumulated in i128).  COUNT(*) is always produced.  d_mask (optional,
 * Arrow LSB bitmask words) pre-filters rows (fused Filter+Aggregate).
 * Outputs are dense groups in ascending hash-slot order (deterministic for
 * a fixed max_groups): d_first_row[g] = first input row carrying the
 * group's key (gather key values from it), d_acc_out = i128 LE per
 * (group, agg), d_counts_out = i64 per group. */
#define BG_AGG_OP_SUM_DEC128 0
#define BG_AGG_OP_SUM_I64 1
#define BG_AGG_OP_MIN_I64 2 /* acc = order-preserving u64; host decodes */
#define BG_AGG_OP_MAX_I64 3
#define BG_AGG_OP_SUM_F64 4
#define BG_AGG_OP_MIN_F64 5 /* acc = totally-ordered u64 (IEEE sign flip) */
#define BG_AGG_OP_MAX_F64 6
#define BG_AGG_OP_MIN_I32 7 /* Int32/Date32; acc as MIN_I64 of the sign-extended value */
#define BG_AGG_OP_MAX_I32 8
#define BG_AGG_OP_MIN_ROW 9 /* Decimal128/Utf8 by agg_cols[i].dtype; acc word 0 = winning row+1, 0 = none */
#define BG_AGG_OP_MAX_ROW 10
/* MIN/MAX over a Decimal128 or Utf8 column (the ROW ops) keep the winning
 * INPUT ROW, not the value: no 128-bit atomic min/max exists and a string
 * has no fixed width.  Order: signed i128; bytewise unsigned lexicographic
 * with a proper prefix smaller ("" is a value, not NULL) — Arrow's orders,
 * the ones the reference's DataFusion Min/Max accumulators compare by.
 * Which of several tied rows wins is not deterministic; the value gathered
 * from it is.  Turn the records into a column with bg_agg_winner_rows +
 * bg_gather / bg_gather_varlen.  A ROW op over any other dtype, or an I32
 * op over anything but Int32/Date32, returns BG_ERR_UNSUPPORTED before any
 * device allocation. */
int bg_hashagg(const bg_column* key_cols, int32_t nkeys,
               const bg_column* agg_cols, const int32_t* agg_ops,
               int32_t naggs, const uint8_t* d_mask, int64_t n,
               int64_t max_groups, uint32_t* d_first_row,
               uint8_t* d_acc_out /* max_groups*naggs*16 */,
               int64_t* d_counts_out /* max_groups */,
               int64_t* out_ngroups);

/* As bg_hashagg, plus d_nncnt_out (max_groups*naggs i64): the per-
 * (group, aggregate) count of NON-NULL inputs.  NULL aggregate inputs are
 * always skipped (SQL semantics; the reference's accumulators in
 * datafusion/functions-aggregate treat null as no contribution); a group
 * whose inputs were all NULL has nncnt 0 and its SUM/MIN/MAX is NULL —
 * the accumulator value alone cannot encode that.  NULL group keys hash
 * as "no contribution" (hash_utils create_hashes) and group together
 * (NULL == NULL in GROUP BY). */
int bg_hashagg2(const bg_column* key_cols, int32_t nkeys,
                const bg_column* agg_cols, const int32_t* agg_ops,
                int32_t naggs, const uint8_t* d_mask, int64_t n,
                int64_t max_groups, uint32_t* d_first_row,
                uint8_t* d_acc_out, int64_t* d_counts_out,
                int64_t* d_nncnt_out, int64_t* out_ngroups);

/* ---- ProjectionExec expression subset: Decimal128 arithmetic ----
 * ops: 0 a*b, 1 a+b, 2 a-b, 3 lit-a, 4 a*lit, 5 a+lit (exact i128;
 * lit as (lo,hi) i128 halves).  d_out: n x 16 B. */
int bg_project_dec128(int32_t op, const bg_column* a, const bg_column* b,
                      int64_t lit_lo, int64_t lit_hi, int64_t n, void* d_out);

/* Multi-expression Decimal128 projection in one pass: stack bytecode
 * (PUSH_COL/PUSH_LIT/MUL/ADD/SUB) over <=8 input columns, <=6 output
 * dec128 columns; each input read once, intermediates in registers (the
 * q1-class expression chains cost ~77 GB of materialised intermediates
 * at SF100 without this). */
int bg_project_dec128_multi(const bg_column* cols, int32_t ncols,
                            const int32_t* ops, const int32_t* args,
                            int32_t nops, const int32_t* expr_end,
                            int32_t nexprs, const int64_t* lit_lo,
                            const int64_t* lit_hi, int32_t nlits, int64_t n,
                            void* const* d_outs);

/* ---- SortExec (stable multi-column ORDER BY) ----
 * d_perm (u32[n]) receives the stable row permutation realising ORDER BY
 * key_cols[0] [DESC], key_cols[1] [DESC], ...; Top-K = first K entries.
 * Keys: INT64/INT32/DATE32 (round 1). */
int bg_sort_rows(const bg_column* key_cols, const int32_t* descending,
                 int32_t nkeys, int64_t n, uint32_t* d_perm);

/* As bg_sort_rows with explicit per-key null ordering (1 = NULLS FIRST).
 * bg_sort_rows defaults to the SQL convention (ASC -> NULLS LAST,
 * DESC -> NULLS FIRST); null keys sort as one stable group and never
 * scramble by their undefined payload bytes. */
int bg_sort_rows2(const bg_column* key_cols, const int32_t* descending,
                  const int32_t* nulls_first, int32_t nkeys, int64_t n,
                  uint32_t* d_perm);

/* ---- SortMergeJoinExec (INNER, key-sorted Int64 inputs) ----
 * The reference's DEFAULT partitioned join (prefer_hash_join=false,
 * extension.rs:850-858; every approved/q*.txt join stage is SMJ).  Inputs
 * are key-sorted (bg_sort_rows); emits positions into the sorted orders,
 * probe-major with build ascending (fully deterministic).  Call once with
 * d_out_* NULL to size the output, then again with buffers. */
int bg_merge_join(const int64_t* d_build_sorted, int64_t nb,
                  const int64_t* d_probe_sorted, int64_t np,
                  int64_t* out_matches, uint32_t* d_out_probe,
                  uint32_t* d_out_build);

/* ---- GPU Parquet decode, stage 1: Snappy page decompression ----
 * (SURVEY.md §8f row 1).  One device thread decodes one independently-
 * compressed page; thousands of pages decode concurrently.  h_pages is a
 * host array of {src, dst, src_len, dst_cap} with DEVICE src/dst pointers;
 * h_out_lens receives decompressed lengths (-1 = malformed page). */
typedef struct {
  const uint8_t* d_src;
  uint8_t* d_dst;
  int64_t src_len;
  int64_t dst_cap;
} bg_snappy_page;
int bg_snappy_decompress(const bg_snappy_page* h_pages, int64_t npages,
                         int64_t* h_out_lens);

/* Parquet data-page extraction (PLAIN, no nulls): validates the def-level
 * block (optional columns) on device, copies the value bytes into the
 * column buffer at dst_byte_off; flba_reverse flips 16-B big-endian
 * decimals to Arrow LE.  Fails loudly on nulls/V2/dictionary pages. */
int bg_page_extract(const void* d_page, int64_t page_len, void* d_out,
                    int64_t dst_byte_off, int64_t nvals, int64_t src_esz,
                    int32_t has_def, int32_t flba_reverse);

/* Parquet dictionary-index expansion (PLAIN_DICTIONARY/RLE_DICTIONARY
 * data pages): one device thread expands one page's RLE/bit-packed index
 * block to u32 indices; materialise with bg_gather from the PLAIN-decoded
 * dictionary. */
int bg_dict_indices(const void* d_page, int64_t page_len, int64_t nvals,
                    int32_t has_def, uint32_t* d_out_idx);

/* Batched forms: the whole column's page list in one launch (chunks hold
 * few pages; per-page host loops starve the GPU). */
typedef struct {
  const uint8_t* d_page;
  uint8_t* d_out;
  int64_t page_len;
  int64_t nvals;
  int64_t src_esz;
  int32_t has_def;      /* 0 none, 1 validate-all-present, 2 nullable */
  int32_t flba_reverse;
  const uint32_t* d_vidx;      /* mode 2: slot -> value index, ~0u = NULL */
  const int64_t* d_n_present;  /* mode 2: values in this page */
} bg_page_extract_job;
int bg_page_extract_batch(const bg_page_extract_job* h_jobs, int64_t njobs);

typedef struct {
  const uint8_t* d_page;
  uint32_t* d_out_idx;
  int64_t page_len;
  int64_t nvals;
  int32_t has_def;      /* 0 none, 1 validate-all-present, 2 nullable */
  int32_t _pad;
  const uint32_t* d_vidx;      /* mode 2 */
  const int64_t* d_n_present;  /* mode 2 */
  uint32_t* d_dense;           /* mode 2: scratch, >= n_present u32 */
} bg_dict_indices_job;
int bg_dict_indices_batch(const bg_dict_indices_job* h_jobs, int64_t njobs);

/* OPTIONAL-column definition levels (max_def=1; the RLE/bit-packed hybrid
 * of the parquet spec, as decoded by the reference's parquet crate
 * rle.rs): per data page, decode [u32 len][levels] into the column's
 * Arrow validity bitmap (atomicOr into u32 words at bit_off — page
 * boundaries are not byte-aligned), the slot->value-index map vidx
 * (~0u = NULL), and n_present.  Feed vidx/n_present to the mode-2
 * extract/dict jobs above. */
typedef struct {
  const uint8_t* d_page;    /* page start ([u32 dlen][levels][values...]) */
  uint32_t* d_vidx;      /* u32[nvals] slice for this page */
  uint32_t* d_valid_out; /* column validity bitmap (u32 words, zeroed) */
  int64_t page_len;
  int64_t nvals;
  int64_t bit_off;       /* absolute bit position of this page's slot 0 */
  int64_t* d_n_present;
} bg_def_levels_job;
int bg_def_levels_batch(const bg_def_levels_job* h_jobs, int64_t njobs);

/* LIST columns (repetition levels, max_rep == 1; parquet-format.md
 * "Nested Encoding" / the reference's arrow-rs list reader).  A V1 page
 * body is [u32 rlen][rep][u32 dlen][def][values].  pass 1 fills
 * d_counts[4] = {rows, entries, present, rlen} per page; the host
 * prefix-sums bases and re-points the UNCHANGED mode-2 extract/dict
 * jobs at page + 4 + rlen.  pass 2 emits per-row entry counts (list
 * offsets = their prefix sum), the list/element validity bitmaps and
 * the page-local value index per entry.  Rows must not span pages. */
typedef struct {
  const uint8_t* d_page;   /* [u32 rlen][rep][u32 dlen][def][values] */
  int64_t page_len;
  int64_t nslots;       /* level entries (page header num_values) */
  int32_t max_def;
  int32_t def_entry;    /* min def meaning an element slot exists */
  int32_t def_valid;    /* min def meaning the LIST is non-null */
  int32_t _pad;
  int64_t row_base;     /* pass 2: column-global bases */
  int64_t entry_base;
  int64_t* d_counts;    /* pass 1 */
  int32_t* d_row_sizes; /* pass 2 (column-global) */
  uint32_t* d_list_valid;
  uint32_t* d_elem_valid;
  uint32_t* d_vidx;     /* pass 2: PAGE-LOCAL slice */
} bg_list_levels_job;
int bg_list_levels_batch(const bg_list_levels_job* h_jobs, int64_t njobs,
                         int32_t pass);

/* BYTE_ARRAY (Utf8/Binary) PLAIN pages (parquet spec PLAIN: [u32 len]
 * [bytes] per value; the reference's decoding.rs PlainDecoder):
 * per page, record each slot's length + absolute device source address
 * (NULL slots length 0); then ONE column-wide bg_ba_materialize scans the
 * lengths into Arrow i32 offsets and copies every slot's bytes.  Dict-
 * coded string pages bridge with bg_ba_from_dict (lengths/addresses from
 * the PLAIN-decoded dictionary through the expanded indices). */
typedef struct {
  const uint8_t* d_page;
  int64_t* d_lens_out;     /* i64[nvals] slice */
  int64_t* d_srcaddr_out;  /* i64[nvals] slice */
  int64_t page_len;
  int64_t nvals;
  int32_t has_def; /* 0 none, 2 nullable */
  int32_t _pad;
  const uint32_t* d_vidx;
  const int64_t* d_n_present;
} bg_ba_page_job;
int bg_ba_extract_batch(const bg_ba_page_job* h_jobs, int64_t njobs);
int bg_ba_from_dict(const uint32_t* d_idx, const int32_t* d_doffs,
                    const void* d_ddata, const uint32_t* d_vidx, int64_t n,
                    int64_t* d_lens_out, int64_t* d_srcaddr_out);
int bg_ba_materialize(const int64_t* d_lens, const int64_t* d_srcaddr,
                      int64_t n, int32_t* d_offs32 /* n+1 */,
                      uint8_t* d_data, int64_t data_cap, int64_t* out_total);

/* DELTA_BINARY_PACKED (encoding 5) INT32/INT64 pages — the reference's
 * parquet-rs DataPageV2 writer default for integers (spec Encodings.md
 * "Delta Encoding"; decoding.rs DeltaBitPackDecoder).  Lane-0 serial per
 * page (the prefix chain is sequential), pages concurrent across waves;
 * nullable slots scatter through the def-level vidx map. */
typedef struct {
  const uint8_t* d_page;
  uint8_t* d_out;        /* i32/i64 column slice */
  int64_t page_len;
  int64_t nvals;
  int64_t esz;           /* 4 or 8 */
  int32_t has_def;       /* 0 none, 2 nullable */
  int32_t _pad;
  const uint32_t* d_vidx;
  const int64_t* d_n_present;
} bg_delta_bp_job;
int bg_delta_bp_batch(const bg_delta_bp_job* h_jobs, int64_t njobs);

/* DELTA_LENGTH_BYTE_ARRAY (6) / DELTA_BYTE_ARRAY (7) string pages — the
 * reference's parquet-rs V2 writer defaults for BYTE_ARRAY (Encodings.md;
 * decoding.rs DeltaLengthByteArrayDecoder / DeltaByteArrayDecoder).
 * pass 1 fills slot lengths (+ source addresses for enc 6; 0 for enc 7);
 * after bg_ba_materialize lays out the column, pass 2 (enc 7 only)
 * rebuilds each string from its predecessor's prefix + its suffix. */
typedef struct {
  const uint8_t* d_page;
  int64_t* d_lens_out;
  int64_t* d_srcaddr_out;
  const int32_t* d_offs32;  /* pass 2 */
  uint8_t* d_data_out;      /* pass 2 */
  int64_t page_len;
  int64_t nvals;
  int32_t has_def;
  int32_t enc; /* 6 or 7 */
  const uint32_t* d_vidx;
  const int64_t* d_n_present;
} bg_delta_ba_job;
int bg_delta_ba_batch(const bg_delta_ba_job* h_jobs, int64_t njobs,
                      int32_t pass);

/* BYTE_STREAM_SPLIT (encoding 9, fixed-width): parallel byte transpose
 * of the k per-byte streams back into values (bg_page_extract_job fields;
 * flba_reverse unused). */
int bg_bss_batch(const bg_page_extract_job* h_jobs, int64_t njobs);

/* Device LZ4 block compression (the GPU shuffle codec's compress half,
 * SURVEY.md §8f row 3): 64 KiB blocks, one wave per block.  d_out_slots
 * holds nblocks slots of 65544 B; h_block_sizes[i] = compressed size, or
 * negative (-usize) when the block is stored raw.  Host glue frames the
 * blocks (constant header 04224d18 40 40 c0 + [u32 size] blocks + end
 * mark) into the LZ4_FRAME streams Arrow IPC carries. */
#define BG_LZ4_BLOCK 65536
#define BG_LZ4_SLOT_STRIDE 65544
int bg_lz4_compress(const void* d_src, int64_t len, void* d_out_slots,
                    int64_t* h_block_sizes, int64_t* out_nblocks);
/* flat batched compression over many buffers' blocks in one launch */
typedef struct {
  const uint8_t* d_src;
  uint8_t* d_dst_slot;
  int32_t blen;
  int32_t _pad;
} bg_lz4_block_job;
int bg_lz4_compress_flat(const bg_lz4_block_job* h_jobs, int64_t njobs,
                         int64_t* h_block_sizes);
/* LZ4-frame DECODE on device (shuffle-read ingest; mirror of the
 * compressor).  h_frames entries point at frame magic; h_out_lens[i] =
 * decompressed bytes or -1 on malformed input. */
typedef struct {
  const uint8_t* d_src;
  uint8_t* d_dst;
  int64_t src_len;
  int64_t dst_cap;
} bg_lz4_frame;
int bg_lz4_decompress(const bg_lz4_frame* h_frames, int64_t nframes,
                      int64_t* h_out_lens);
/* assemble [u32 size][block] sequences on device at precomputed offsets */
typedef struct {
  const uint8_t* d_src;
  uint8_t* d_dst;     /* at the 4-byte size word */
  int64_t nbytes;
  uint32_t size_word; /* high bit = stored block */
  uint32_t _pad;
} bg_pack_job;
int bg_pack_blocks(const bg_pack_job* h_jobs, int64_t njobs);

/* Fused repartition materialiser (k <= 64, <= 4 fixed-width payload
 * columns): one pass re-hashes keys, ranks rows per partition with
 * ballots, and write-combines k scattered payload streams through
 * per-partition LDS tiles (64-row flushes).  Same outputs and stable
 * order as bg_hash_repartition. */
int bg_hash_repartition_fused(const bg_column* key_cols, int32_t nkeys,
                              const bg_column* payload_cols, int32_t ncols,
                              int64_t n, uint32_t k, uint32_t* d_indices,
                              int64_t* d_offsets, uint32_t* d_rank,
                              void** d_out);

/* ---- stage-interpreter support (bg_execute_stage internals that are
 * also useful standalone) ---- */

/* Place nbits of an Arrow LSB bitmap at an arbitrary bit offset of a
 * destination bitmap (device shuffle-read: batch validity bitmaps land at
 * non-byte-aligned row cursors).  Boundary words use atomics. */
int bg_bitcopy(const uint8_t* d_src_bits, int64_t nbits, uint8_t* d_dst_bits,
               int64_t dst_bit_off);

/* Materialize bg_hashagg accumulator records into an Arrow column:
 * acc_stride in bytes between consecutive groups' records for this
 * aggregate; op = BG_AGG_OP_*; d_out element size 16 (SUM_DEC128), 4 (the
 * I32 ops) or 8.  With d_nncnt (stride bytes), groups whose non-null input
 * count is 0 get their bit cleared in d_valid_out (SQL: SUM/MIN/MAX of
 * all-NULL = NULL).  BG_ERR_INVALID for the ROW ops: their record names a
 * row of an input column this call never sees (bg_agg_winner_rows). */
int bg_agg_materialize(const void* d_acc, int64_t acc_stride, int32_t op,
                       int64_t ngroups, void* d_out, const int64_t* d_nncnt,
                       int64_t nncnt_stride, uint8_t* d_valid_out);

/* MIN_ROW/MAX_ROW records -> what a take needs: d_rows_out[g] = the
 * group's winning input row (0 where it had no non-NULL input, so the
 * index stays gather-safe) and bit g of d_valid_out (ceil(ngroups/8)
 * bytes, written whole) set exactly where word 0 of the record is
 * non-zero.  The value column is bg_gather (16-B elements) or
 * bg_gather_varlen of the aggregate's input by d_rows_out with this
 * validity — the Option-valued state of the reference's Min/Max
 * accumulators (datafusion/functions-aggregate min_max.rs), NULL for a
 * group whose inputs were all NULL. */
int bg_agg_winner_rows(const void* d_acc, int64_t acc_stride, int64_t ngroups,
                       uint32_t* d_rows_out, uint8_t* d_valid_out);

/* Strided i64 copy (COUNT materialisation from interleaved agg records). */
int bg_copy_i64_strided(const void* d_src, int64_t stride, int64_t n,
                        void* d_out);

/* AVG finalisation (AggregateExec Final for avg):
 * decimal — DataFusion's decimal AvgAccumulator: target scale = input
 * scale + 4, out = round-half-away-from-zero(sum * 10^scale_shift / count),
 * exact i128; f64 — IEEE sum/count.  count==0 clears the group's valid
 * bit. */
int bg_avg_finalize(const void* d_sum_acc, int64_t acc_stride, int32_t is_f64,
                    const void* d_cnt, int64_t cnt_stride,
                    int32_t scale_shift, int64_t ngroups, void* d_out,
                    uint8_t* d_valid_out);

/* ---- window functions over sorted input ----
 *
 * DataFusion's BoundedWindowAggExec / WindowAggExec with
 * InputOrderMode::Sorted (datafusion.proto WindowAggExecNode,
 * PhysicalWindowExprNode, WindowFrame); Ballista's
 * PartitionedBoundedWindowAggExec runs the former per partition.  The rows
 * are ALREADY sorted by (partition keys, order keys) — bg_sort_rows2
 * upstream — and, like the reference, nothing here verifies that: unsorted
 * input gives meaningless values, never an index outside [0, n].
 *
 * The work splits three ways: bounds once per window node, a frame once per
 * distinct frame, one rank or aggregate call per expression.  Row positions
 * are uint32_t; n > UINT32_MAX - 1 is BG_ERR_INVALID; n == 0 succeeds and
 * touches nothing.  Every temporary returns to the pool before the call
 * returns, on error paths too. */

/* Partition and peer-group extents by adjacent-row comparison of the key
 * columns (0-4 each; Utf8 by bytes; NULL equals NULL; Float64 by bit
 * pattern, so -0.0 and +0.0 differ and equal NaN patterns match).  Rows
 * are in one partition iff all part_cols are equal, and peers iff they
 * share a partition and all order_cols are equal.  Per row i the half-open
 * extents [d_part_start[i], d_part_end[i]) and [d_peer_start[i],
 * d_peer_end[i]); any output may be NULL. */
int bg_window_bounds(const bg_column* part_cols, int32_t npart,
                     const bg_column* order_cols, int32_t norder, int64_t n,
                     uint32_t* d_part_start, uint32_t* d_part_end,
                     uint32_t* d_peer_start, uint32_t* d_peer_end);

#define BG_WIN_ROW_NUMBER 0
#define BG_WIN_RANK 1
#define BG_WIN_DENSE_RANK 2
/* row_number / rank / dense_rank, 1-based, as INT64 (DataFusion types them
 * UInt64; same bits, values < 2^32).  d_peer_start may be NULL for
 * ROW_NUMBER; d_part_start NULL means one partition. */
int bg_window_rank(int32_t fn, const uint32_t* d_part_start,
                   const uint32_t* d_peer_start, int64_t n, int64_t* d_out);

#define BG_WIN_ROWS 0
#define BG_WIN_RANGE 1
#define BG_WIN_UNBOUNDED 0   /* preceding as a start, following as an end */
#define BG_WIN_CURRENT_ROW 1
#define BG_WIN_PRECEDING 2
#define BG_WIN_FOLLOWING 3
/* Resolve one frame to a half-open row range [d_lo[i], d_hi[i]) inside the
 * row's partition; always part_start <= lo <= hi <= part_end, and an empty
 * frame is legal.  ROWS offsets count rows.  RANGE: CURRENT_ROW is the peer
 * group's edge; an offset bound needs order_col, the single order key
 * (INT64, INT32, DATE32 in days, or FLOAT64 with the offset passed as f64
 * bits), and is found by a bounded binary search among the partition's
 * non-NULL keys, key +/- offset saturating at the i64 limits; a row whose
 * key is NULL keeps its NULL peer group as the offset side.  order_col is
 * NULL unless a RANGE offset bound is present; offsets are >= 0 and read
 * only for PRECEDING/FOLLOWING.  The peer arrays may be NULL for ROWS. */
int bg_window_frame(int32_t units, int32_t start_kind, int64_t start_off,
                    int32_t end_kind, int64_t end_off,
                    const bg_column* order_col, int32_t descending,
                    const uint32_t* d_part_start, const uint32_t* d_part_end,
                    const uint32_t* d_peer_start, const uint32_t* d_peer_end,
                    int64_t n, uint32_t* d_lo, uint32_t* d_hi);

#define BG_WIN_SUM 0
#define BG_WIN_COUNT 1
#define BG_WIN_MIN 2
#define BG_WIN_MAX 3
/* One aggregate over every row's frame [lo, hi), NULL inputs skipped (AVG
 * is SUM + COUNT + bg_avg_finalize with one "group" per row).  d_lo NULL
 * means "the frame starts at d_part_start", and is REQUIRED for MIN/MAX:
 * they are the segmented running extremum at hi - 1, and a sliding one is
 * BG_ERR_UNSUPPORTED.  val NULL is count(*).
 *   SUM   INT64 (wrapping) -> i64; DECIMAL128 (exact i128) -> 16 B;
 *         FLOAT64 -> f64, its running prefix restarted per partition
 *   COUNT -> i64, never NULL (d_valid_out unused, may be NULL)
 *   MIN/MAX over INT64, INT32, DATE32, FLOAT64 (IEEE total order),
 *         DECIMAL128 -> val's own width
 * SUM/MIN/MAX clear a row's bit in d_valid_out when its frame holds no
 * non-NULL input (the value written is 0); ceil(n/8) bytes are written
 * whole and none beyond. */
int bg_window_agg(int32_t fn, const bg_column* val,
                  const uint32_t* d_part_start, const uint32_t* d_lo,
                  const uint32_t* d_hi, int64_t n, void* d_out,
                  uint8_t* d_valid_out);

/* ---- stage interpreter (the product entry of SURVEY.md §8b seam 1) ----
 *
 * bg_execute_stage executes ONE whole query stage — the GPU analogue of
 * QueryStageExecutor::execute_query_stage (executor/src/execution_engine.
 * rs:78-103, default impl :127-212): operators are sequenced by a plan
 * tree, key EXPRESSIONS are evaluated before hashing (sort_shuffle/
 * writer.rs:1265), and the root writer produces the reference's exact
 * shuffle file bytes + ShuffleWritePartition summaries (proto :779-791).
 *
 * plan_json is a faithful JSON restatement of the decoded TaskDefinition
 * plan (the Rust host decodes task.plan with datafusion-proto exactly as
 * execution_loop.rs:364-367 does, then serialises the operator tree to
 * this schema — see INTEGRATION.md "Stage plan JSON").  Operators:
 * scan / filter / project / hash_join / nested_loop_join /
 * hash_aggregate / sort / limit / window / sort_shuffle_write /
 * passthrough_write / collect.
 *
 * On success *out_json receives a malloc'd result document:
 *   {"partitions": [{"partition_id", "path", "num_batches", "num_rows",
 *     "num_bytes"}...], "metrics": {...}, "rows": [...] (collect roots)}
 * Free it with bg_stage_free.  On failure returns a bg_status and
 * bg_last_error() describes the offending plan node. */
int bg_execute_stage(const char* plan_json, char** out_json);
void bg_stage_free(char* p);

/* Parse + type-check a stage plan without touching the GPU (host-side
 * validation; CPU tests cover the plan grammar through this). */
int bg_stage_validate(const char* plan_json, char** out_json);

/* Register a device-resident input table for "device" scan sources
 * (bench/tests feed synthetic in-HBM tables; the Rust host feeds decoded
 * ShuffleReaderExec batches the same way).  The caller owns the column
 * buffers; they must outlive the stage. */
int bg_stage_register_table(const char* name, const bg_column* cols,
                            const char* const* col_names, int32_t ncols,
                            int64_t n_rows);
int bg_stage_unregister_table(const char* name);

/* Deterministic synthetic fill (splitmix64 per element) for the
 * no-Python C++ examples/bench — test/bench infrastructure, not a query
 * path.  mode: 0 int64, 1 int32, 2 Decimal128 (LE pair).  Values uniform
 * in [lo, hi). */
int bg_fill_rand(void* d_out, int64_t n, uint64_t seed, int64_t lo,
                 int64_t hi, int32_t mode);

/* ---- fused filter+aggregate stages ---- */

/* TPC-H q6 stage 1 (scan+filter+aggregate, approved/q6.txt):
 *   sum(l_extendedprice * l_discount), count of qualifying rows.
 * shipdate: DATE32; discount/quantity/extendedprice: DECIMAL128.
 * Result is the exact i128 sum (scale 4). */
int bg_q6_agg(const bg_column* shipdate, const bg_column* discount,
              const bg_column* quantity, const bg_column* extendedprice,
              int32_t date_lo, int32_t date_hi, int64_t disc_lo,
              int64_t disc_hi, int64_t qty_lt,
              uint64_t* out_sum_lo, int64_t* out_sum_hi, int64_t* out_count);

/* TPC-H q1 stage 1 (filter + grouped partial aggregate, approved/q1.txt):
 * group = (rf_code<<4)|ls_code over u8 dictionary codes (<16 each);
 * per group: count + exact i128 sums of {qty, price, price*(100-disc),
 * price*(100-disc)*(100+tax), disc} — scales {2,2,4,6,2}.
 * h_counts: host i64[256]; h_sums: host bytes 256*5*16 (LE i128 each). */
int bg_q1_agg(const bg_column* rf, const bg_column* ls,
              const bg_column* quantity, const bg_column* extendedprice,
              const bg_column* discount, const bg_column* tax,
              const bg_column* shipdate, int32_t date_le,
              int64_t* h_counts, uint8_t* h_sums);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* BALLISTA_GPU_H */
