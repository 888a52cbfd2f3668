// stage.cpp — the GPU query-stage interpreter behind bg_execute_stage.
//
// This is the C++ host that turns a DECODED task plan into kernel sequences,
// replacing the hand-composed per-query scripts of round 1.  It restates,
// operator by operator (reference citations under /root/reference):
//
//   * QueryStageExecutor::execute_query_stage / drive_shuffle_writer_stage —
//     ballista/executor/src/execution_engine.rs:78-103, 127-212, 354-388:
//     the engine receives one whole stage plan (root = a shuffle writer) and
//     drives it to ShuffleWritePartition summaries.
//   * The plan arrives as a JSON restatement of the decoded TaskDefinition
//     physical plan (execution_loop.rs:364-367 decodes plan bytes with
//     datafusion-proto; the Rust host serialises that tree to this schema —
//     INTEGRATION.md "Stage plan JSON").  Key expressions are EVALUATED
//     before hashing, exactly like compute_partition_indices
//     (sort_shuffle/writer.rs:1259-1279, evaluate_expressions_to_arrays
//     :1265).
//   * SortShuffleWriterExec::execute_shuffle_write + write_task_consolidated
//     (writer.rs:564-753, 810-895) + ShuffleIndex (index.rs:21-33): the
//     consolidated `data.arrow` + `(K+1)` LE-i64 `.index` byte format, with
//     LZ4_FRAME-compressed IPC batches (codec default lz4,
//     core/src/config.rs:413-415) — compression runs ON DEVICE
//     (bg_lz4_compress_flat), only final bytes cross PCIe.
//   * ShuffleReaderExec::execute fan-in + local ranged reads
//     (shuffle_reader.rs:359-432, 1120-1168) with transparent sub-stream
//     crossing (multi_stream_reader.rs:17-34) and re-chunking to batch_size
//     (:1194-1282) — the "shuffle" scan source, decompressing on device.
//   * Operator semantics: FilterExec / ProjectionExec / HashJoinExec /
//     NestedLoopJoinExec / AggregateExec(Partial|Final|Single) /
//     SortExec(TopK) / WindowAggExec + BoundedWindowAggExec of DataFusion 55
//     (SURVEY.md §8a), each mapped onto the existing HIP kernels through
//     the public C ABI only — this file contains no device code.
//
// Everything here is host C++ over the `bg_*` ABI; it compiles into
// libballista_gpu.so next to the kernels so a Rust GpuExecutionEngine binds
// ONE entry (bg_execute_stage) per task.

#include <sys/stat.h>
#include <sys/types.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/ballista_gpu.h"
#include "bg_internal.h"
#include "stage_ipc.h"
#include "stage_json.h"

namespace bgstage {

using bgjson::Value;
using bgjson::ValuePtr;

// ---------------------------------------------------------------------------
// infrastructure
// ---------------------------------------------------------------------------

struct StageError : std::runtime_error {
  int code;
  StageError(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

static void chk(int rc, const char* what) {
  if (rc != BG_OK)
    throw StageError(rc, std::string(what) + ": " + bg_last_error());
}

struct DBuf {
  void* p = nullptr;
  uint64_t bytes = 0;
  DBuf(const DBuf&) = delete;
  DBuf& operator=(const DBuf&) = delete;
  explicit DBuf(uint64_t n) : bytes(n) {
    chk(bg_malloc(n ? n : 1, &p), "bg_malloc");
  }
  ~DBuf() {
    if (p) (void)bg_free(p);
  }
  uint8_t* u8() const { return (uint8_t*)p; }
};
using DBufPtr = std::shared_ptr<DBuf>;

static DBufPtr dalloc(uint64_t n) { return std::make_shared<DBuf>(n); }

// n elements of esz bytes each; an empty column still owns one element
static DBufPtr dalloc_elems(int64_t n, int64_t esz = 1) {
  return dalloc((uint64_t)(n > 0 ? n : 1) * (uint64_t)esz);
}

// Padded bitmap of nbits bits (validity, filter masks): whole 64-bit words
// plus one spare, so word-wide kernels may touch the word after the last
// bit.  join_visited_bytes() in kernels.hip uses the same formula for the
// join's visited bitmap.  fill >= 0 memsets every byte to it.
static DBufPtr alloc_bitmap(int64_t nbits, int fill = -1) {
  DBufPtr b = dalloc((uint64_t)((nbits + 63) / 64) * 8 + 8);
  if (fill >= 0) chk(bg_memset(b->p, fill, b->bytes), "bg_memset");
  return b;
}

static DBufPtr upload(const void* host, uint64_t n) {
  DBufPtr b = dalloc(n);
  if (n) chk(bg_memcpy_h2d(b->p, host, n), "bg_memcpy_h2d");
  return b;
}

using Clock = std::chrono::steady_clock;
static int64_t ns_since(Clock::time_point t0) {
  return std::chrono::duration_cast<std::chrono::nanoseconds>(Clock::now() -
                                                              t0)
      .count();
}

static int64_t dt_size(int32_t dt) {
  switch (dt) {
    case BG_DT_INT32:
    case BG_DT_DATE32: return 4;
    case BG_DT_INT64:
    case BG_DT_FLOAT64: return 8;
    case BG_DT_DECIMAL128: return 16;
    case BG_DT_DICT8: return 1;
    case BG_DT_UTF8: return 0;  // variable
    default: throw StageError(BG_ERR_INVALID, "unknown dtype tag");
  }
}

// a dtype as the plan JSON spells it (Arrow vocabulary)
struct DtSpec { int32_t dt, precision, scale; };

struct Col {
  int32_t dtype = 0;
  int32_t precision = 0, scale = 0;
  DBufPtr data, validity, offsets;  // owned device buffers (may be null)
  const void* ext_data = nullptr;   // registered-table externals
  const uint8_t* ext_valid = nullptr;
  const int32_t* ext_offs = nullptr;
  int64_t data_bytes = 0;  // utf8 payload bytes

  const void* dptr() const { return data ? data->p : ext_data; }
  const uint8_t* vptr() const {
    return validity ? (const uint8_t*)validity->p : ext_valid;
  }
  const int32_t* optr() const {
    return offsets ? (const int32_t*)offsets->p : ext_offs;
  }
  bool nullable() const { return vptr() != nullptr; }
  DtSpec spec() const { return {dtype, precision, scale}; }
};

// a Col of the given type that owns no buffers yet
static Col make_col(const DtSpec& d) {
  Col c;
  c.dtype = d.dt;
  c.precision = d.precision;
  c.scale = d.scale;
  return c;
}

struct Table {
  int64_t n = 0;
  std::vector<std::string> names;
  std::vector<Col> cols;

  int idx(const std::string& name) const {
    for (size_t i = 0; i < names.size(); ++i)
      if (names[i] == name) return (int)i;
    throw StageError(BG_ERR_INVALID, "plan: unknown column '" + name + "'");
  }
  Col& col(const std::string& name) { return cols[(size_t)idx(name)]; }
  const Col& col(const std::string& name) const {
    return cols[(size_t)idx(name)];
  }
};

static bg_column to_bg(const Col& c, int64_t n) {
  bg_column b{};
  b.dtype = c.dtype;
  b.precision = c.precision;
  b.scale = c.scale;
  b.d_data = c.dptr();
  b.d_validity = c.vptr();
  b.d_offsets = c.optr();
  b.len = n;
  return b;
}

// ---- dtype names in the plan JSON (Arrow vocabulary) ----
static DtSpec parse_dtype(const Value& field) {
  const std::string& s = field.get_str("dtype");
  if (s == "int32") return {BG_DT_INT32, 0, 0};
  if (s == "int64") return {BG_DT_INT64, 0, 0};
  if (s == "date32") return {BG_DT_DATE32, 0, 0};
  if (s == "float64") return {BG_DT_FLOAT64, 0, 0};
  if (s == "dict8") return {BG_DT_DICT8, 0, 0};
  if (s == "utf8") return {BG_DT_UTF8, 0, 0};
  if (s == "decimal128")
    return {BG_DT_DECIMAL128, (int32_t)field.get_int_or("precision", 38),
            (int32_t)field.get_int_or("scale", 0)};
  throw StageError(BG_ERR_INVALID, "plan: unknown dtype '" + s + "'");
}

static const char* dtype_name(int32_t dt) {
  switch (dt) {
    case BG_DT_INT32: return "int32";
    case BG_DT_INT64: return "int64";
    case BG_DT_DATE32: return "date32";
    case BG_DT_FLOAT64: return "float64";
    case BG_DT_DICT8: return "dict8";
    case BG_DT_UTF8: return "utf8";
    case BG_DT_DECIMAL128: return "decimal128";
    default: return "?";
  }
}

// i128 literal: JSON int, or decimal-integer string (already scaled)
static void parse_i128(const Value& v, int64_t* lo, int64_t* hi) {
  if (v.kind == Value::INT) {
    *lo = v.i;
    *hi = v.i < 0 ? -1 : 0;
    return;
  }
  if (v.kind != Value::STR)
    throw StageError(BG_ERR_INVALID, "plan: i128 literal must be int/string");
  const std::string& s = v.s;
  bool neg = !s.empty() && s[0] == '-';
  unsigned __int128 acc = 0;
  for (size_t i = neg ? 1 : 0; i < s.size(); ++i) {
    if (s[i] < '0' || s[i] > '9')
      throw StageError(BG_ERR_INVALID, "plan: bad i128 literal '" + s + "'");
    acc = acc * 10 + (unsigned)(s[i] - '0');
  }
  __int128 val = neg ? -(__int128)acc : (__int128)acc;
  *lo = (int64_t)(uint64_t)val;
  *hi = (int64_t)(uint64_t)((unsigned __int128)val >> 64);
}

// ---------------------------------------------------------------------------
// registered device tables ("device" scan sources)
// ---------------------------------------------------------------------------

static std::mutex g_tables_mu;
static std::map<std::string, Table> g_tables;

// ---------------------------------------------------------------------------
// gather machinery (take of a whole table by a u32 index buffer)
// ---------------------------------------------------------------------------

static Col gather_col(const Col& c, int64_t n_src, const uint32_t* d_idx,
                      int64_t m) {
  Col out = make_col(c.spec());
  if (c.dtype == BG_DT_UTF8) {
    out.offsets = dalloc((uint64_t)(m + 1) * 4);
    // one-to-many joins can duplicate rows, so the gathered payload may
    // EXCEED the source bytes: size exactly first (d_out_data NULL =
    // sizing call), then copy
    int64_t total = 0;
    chk(bg_gather_varlen(c.dptr(), c.optr(), d_idx, m,
                         (int32_t*)out.offsets->p, nullptr, 0, &total),
        "bg_gather_varlen(size)");
    out.data = dalloc_elems(total);
    chk(bg_gather_varlen(c.dptr(), c.optr(), d_idx, m,
                         (int32_t*)out.offsets->p, out.data->p,
                         total > 0 ? total : 1, &total),
        "bg_gather_varlen");
    out.data_bytes = total;
  } else {
    int64_t esz = dt_size(c.dtype);
    out.data = dalloc_elems(m, esz);
    chk(bg_gather(c.dptr(), esz, d_idx, m, out.data->p), "bg_gather");
  }
  if (c.nullable()) {
    out.validity = alloc_bitmap(m);
    chk(bg_gather_bits(c.vptr(), d_idx, m, out.validity->u8()),
        "bg_gather_bits");
  }
  (void)n_src;
  return out;
}

static Table gather_table(const Table& t, const uint32_t* d_idx, int64_t m) {
  Table out;
  out.n = m;
  out.names = t.names;
  for (auto& c : t.cols) out.cols.push_back(gather_col(c, t.n, d_idx, m));
  return out;
}

// Zero-copy row slice of a column: [start, start+len).  start must be a
// multiple of 64 so the validity bitmap slices at a byte boundary (the
// chunked-probe spill path below slices at 64-row multiples).
static Col slice_col(const Col& c, int64_t start, int64_t len) {
  Col s = c;  // shares ownership of the underlying buffers
  if (c.dtype == BG_DT_UTF8) {
    // absolute offsets stay valid against the shared data buffer
    s.ext_offs = c.optr() + start;
    s.offsets = nullptr;
  } else {
    s.ext_data = (const uint8_t*)c.dptr() + start * dt_size(c.dtype);
    s.data = nullptr;
  }
  if (c.nullable()) {
    s.ext_valid = c.vptr() + start / 8;
    s.validity = nullptr;
  }
  (void)len;
  return s;
}

// m all-NULL rows of `like`'s dtype, precision and scale (Utf8: zero
// offsets, 0 data bytes): the NULL-extended side of an outer join's
// unmatched rows.
static Col null_col(const Col& like, int64_t m) {
  Col out = make_col(like.spec());
  if (like.dtype == BG_DT_UTF8) {
    out.offsets = dalloc((uint64_t)(m + 1) * 4);
    chk(bg_memset(out.offsets->p, 0, out.offsets->bytes), "bg_memset");
    out.data = dalloc(1);
    out.data_bytes = 0;
  } else {
    out.data = dalloc_elems(m, dt_size(like.dtype));
    chk(bg_memset(out.data->p, 0, out.data->bytes), "bg_memset");
  }
  out.validity = alloc_bitmap(m, 0);
  return out;
}

// Concatenate row-aligned column pieces (the chunked-probe merge).
static Col concat_cols(const std::vector<Col>& pieces,
                       const std::vector<int64_t>& lens) {
  const Col& c0 = pieces[0];
  Col out = make_col(c0.spec());
  int64_t total = 0;
  bool any_null = false;
  for (size_t i = 0; i < pieces.size(); ++i) {
    total += lens[i];
    any_null |= pieces[i].nullable();
  }
  if (c0.dtype == BG_DT_UTF8) {
    int64_t bytes = 0;
    for (auto& p : pieces) bytes += p.data_bytes;
    out.offsets = dalloc((uint64_t)(total + 1) * 4);
    out.data = dalloc_elems(bytes);
    out.data_bytes = bytes;
    int64_t row = 0, db = 0;
    for (size_t i = 0; i < pieces.size(); ++i) {
      const Col& p = pieces[i];
      if (lens[i] == 0) continue;
      // piece offsets are 0-based (gather outputs); shift by the running
      // data cursor: out = in - (-db)
      chk(bg_sub_i32(p.optr(), lens[i] + 1, (int32_t)(-db),
                     out.offsets->u8() + 4 * row),
          "bg_sub_i32");
      if (p.data_bytes)
        chk(bg_memcpy_dtod(out.data->u8() + db, p.dptr(),
                           (uint64_t)p.data_bytes),
            "bg_memcpy_dtod");
      row += lens[i];
      db += p.data_bytes;
    }
  } else {
    const int64_t esz = dt_size(c0.dtype);
    out.data = dalloc_elems(total, esz);
    int64_t row = 0;
    for (size_t i = 0; i < pieces.size(); ++i) {
      if (lens[i])
        chk(bg_memcpy_dtod(out.data->u8() + row * esz, pieces[i].dptr(),
                           (uint64_t)lens[i] * esz),
            "bg_memcpy_dtod");
      row += lens[i];
    }
  }
  if (any_null) {
    out.validity = alloc_bitmap(total, 0xFF);
    int64_t row = 0;
    for (size_t i = 0; i < pieces.size(); ++i) {
      if (lens[i] && pieces[i].nullable())
        chk(bg_bitcopy(pieces[i].vptr(), lens[i], out.validity->u8(), row),
            "bg_bitcopy");
      row += lens[i];
    }
  }
  return out;
}

// ---------------------------------------------------------------------------
// scan sources
// ---------------------------------------------------------------------------

static void mkdirs(const std::string& path) {
  std::string cur;
  for (size_t i = 0; i <= path.size(); ++i) {
    if (i == path.size() || path[i] == '/') {
      if (!cur.empty() && mkdir(cur.c_str(), 0755) != 0 && errno != EEXIST)
        throw StageError(BG_ERR_INVALID, "mkdir failed: " + cur);
      if (i < path.size()) cur += '/';
    } else {
      cur += path[i];
    }
  }
}

static std::vector<uint8_t> read_file_range(const std::string& path,
                                            int64_t off, int64_t len) {
  std::ifstream f(path, std::ios::binary);
  if (!f) throw StageError(BG_ERR_INVALID, "cannot open " + path);
  if (len < 0) {
    f.seekg(0, std::ios::end);
    len = (int64_t)f.tellg() - off;
  }
  std::vector<uint8_t> buf((size_t)(len > 0 ? len : 0));
  f.seekg(off);
  if (len) f.read((char*)buf.data(), len);
  if (!f) throw StageError(BG_ERR_INVALID, "short read from " + path);
  return buf;
}

static std::vector<int64_t> read_index_file(const std::string& path) {
  auto raw = read_file_range(path, 0, -1);
  std::vector<int64_t> offs(raw.size() / 8);
  memcpy(offs.data(), raw.data(), offs.size() * 8);
  return offs;
}

// Device shuffle-read of a set of (file, partition) locations: the reduce
// side's fan-in (shuffle_reader.rs:359-432), local ranged reads
// (:1120-1168), transparent sub-stream crossing (multi_stream_reader.rs),
// LZ4 batch bodies decompressed on device.
struct BatchSrc {
  int64_t rows;
  // per column: validity (len 0 = absent), [offsets], data extents in raw
  std::vector<bgipc::BufSpec> bufs;
  bool compressed;
  int64_t raw_base;  // offset of this batch's stream range in the upload
};

// What the steps of one shuffle read share.
struct ShuffleRead {
  explicit ShuffleRead(const std::vector<DtSpec>& d) : dts(d) {}
  const std::vector<DtSpec>& dts;
  std::vector<uint8_t> all;       // every partition range, back to back
  std::vector<BatchSrc> batches;
  std::vector<size_t> first_buf;  // column -> index of its validity buffer
  int64_t total = 0;              // rows over all batches
  DBufPtr raw_dev;                // `all` on device
  std::vector<int64_t> utf8_total;
  std::vector<bg_lz4_frame> frames;  // one batched decompress
  std::vector<int64_t> expect;       // decoded bytes each frame must give

  // compressed buffer = [i64 usize][LZ4 frame]; read usize from host copy
  int64_t usize_of(const BatchSrc& b, const bgipc::BufSpec& sp) const {
    int64_t u;
    memcpy(&u, all.data() + b.raw_base + sp.off, 8);
    return u;
  }
  // real decoded bytes of a buffer (-1 prefix = stored raw, Arrow spec)
  int64_t real_usize(const BatchSrc& b, const bgipc::BufSpec& sp) const {
    if (!b.compressed) return sp.len;
    int64_t u = usize_of(b, sp);
    return u == -1 ? sp.len - 8 : u;
  }
};

// validity bits / utf8 offsets land in scratch first and are placed after
// the decompress
struct ShuffleFixup {
  int kind;  // 0 validity bitcopy, 1 utf8 offsets place
  size_t c;
  DBufPtr scratch;
  int64_t rows, row_cursor, data_cursor;
};

// gather all partition ranges into one host buffer, remembering (base, len)
static std::vector<std::pair<int64_t, int64_t>> gather_ranges(
    const std::vector<Value*>& locations, std::vector<uint8_t>& all) {
  std::vector<std::pair<int64_t, int64_t>> ranges;
  auto append = [&](const std::vector<uint8_t>& raw) {
    ranges.push_back({(int64_t)all.size(), (int64_t)raw.size()});
    all.insert(all.end(), raw.begin(), raw.end());
  };
  for (auto* loc : locations) {
    const std::string& data = loc->get_str("data");
    std::vector<int64_t> parts;
    if (loc->has("partition")) parts.push_back(loc->get_int("partition"));
    if (loc->has("partitions"))
      for (auto& p : loc->get_arr("partitions")) parts.push_back(p->i);
    if (!loc->has("index")) {
      // whole file = one complete IPC stream (passthrough writer output)
      append(read_file_range(data, 0, -1));
      continue;
    }
    auto idx = read_index_file(loc->get_str("index"));
    for (int64_t p : parts) {
      if (p + 1 >= (int64_t)idx.size())
        throw StageError(BG_ERR_INVALID, "partition out of index range");
      append(read_file_range(data, idx[(size_t)p],
                             idx[(size_t)p + 1] - idx[(size_t)p]));
    }
  }
  return ranges;
}

static std::vector<BatchSrc> walk_batches(
    const std::vector<uint8_t>& all,
    const std::vector<std::pair<int64_t, int64_t>>& ranges, size_t ncols) {
  std::vector<BatchSrc> batches;
  for (auto& r : ranges) {
    auto metas = bgipc::walk_partition(all.data() + r.first, r.second);
    for (auto& bm : metas) {
      if (bm.bufs.size() < 2 * ncols)
        throw StageError(BG_ERR_INVALID,
                         "shuffle batch has fewer buffers than schema");
      batches.push_back(
          {bm.n_rows, bm.bufs, bm.compressed, r.first + bm.body_off});
    }
  }
  return batches;
}

// allocate the output columns: validity only where some batch carries one,
// utf8 data sized from the sum of the data buffers' decoded sizes
static void alloc_shuffle_columns(ShuffleRead& sr, Table& out) {
  const size_t ncols = sr.dts.size();
  std::vector<bool> has_null(ncols, false);
  for (auto& b : sr.batches)
    for (size_t c = 0; c < ncols; ++c)
      if (b.bufs[sr.first_buf[c]].len > 0) has_null[c] = true;

  for (size_t c = 0; c < ncols; ++c) {
    Col col = make_col(sr.dts[c]);
    if (col.dtype == BG_DT_UTF8)
      col.offsets = dalloc((uint64_t)(sr.total + 1) * 4);  // data: below
    else
      col.data = dalloc((uint64_t)sr.total * (uint64_t)dt_size(col.dtype));
    if (has_null[c]) col.validity = alloc_bitmap(sr.total, 0xFF);
    out.cols.push_back(std::move(col));
  }

  sr.utf8_total.assign(ncols, 0);
  for (size_t c = 0; c < ncols; ++c) {
    if (sr.dts[c].dt != BG_DT_UTF8) continue;
    for (auto& b : sr.batches) {
      auto& dsp = b.bufs[sr.first_buf[c] + 2];
      if (dsp.len > 0) sr.utf8_total[c] += sr.real_usize(b, dsp);
    }
    out.cols[c].data = dalloc_elems(sr.utf8_total[c]);
    out.cols[c].data_bytes = sr.utf8_total[c];
  }
}

// one source buffer -> dst: a copy when stored raw, else an LZ4 frame job
static void schedule_buffer(ShuffleRead& sr, const BatchSrc& b,
                            const bgipc::BufSpec& sp, uint8_t* dst,
                            int64_t dst_cap) {
  const uint8_t* src = sr.raw_dev->u8() + b.raw_base + sp.off;
  if (!b.compressed) {
    chk(bg_memcpy_dtod(dst, src, (uint64_t)sp.len), "bg_memcpy_dtod");
  } else if (sr.usize_of(b, sp) == -1) {
    // Arrow compressed-body convention: uncompressed-length prefix of -1
    // marks a buffer stored raw (compression did not shrink)
    chk(bg_memcpy_dtod(dst, src + 8, (uint64_t)(sp.len - 8)),
        "bg_memcpy_dtod");
  } else {
    sr.frames.push_back({src + 8, dst, sp.len - 8, dst_cap});
    sr.expect.push_back(sr.usize_of(b, sp));
  }
}

// decompress jobs: fixed data straight into columns; validity + utf8
// offsets into scratch (placed after with bitcopy / rebase)
static std::vector<ShuffleFixup> schedule_buffers(ShuffleRead& sr,
                                                  Table& out) {
  std::vector<ShuffleFixup> fixups;
  std::vector<int64_t> utf8_cursor(sr.dts.size(), 0);
  int64_t row_cursor = 0;
  for (auto& b : sr.batches) {
    for (size_t c = 0; c < sr.dts.size(); ++c) {
      const size_t bi = sr.first_buf[c];
      auto to_scratch = [&](const bgipc::BufSpec& sp, int kind) {
        int64_t u = sr.real_usize(b, sp);
        DBufPtr scr = dalloc((uint64_t)u + 8);
        schedule_buffer(sr, b, sp, scr->u8(), u + 8);
        fixups.push_back({kind, c, scr, b.rows, row_cursor, utf8_cursor[c]});
      };
      if (b.bufs[bi].len > 0) to_scratch(b.bufs[bi], 0);
      if (sr.dts[c].dt == BG_DT_UTF8) {
        to_scratch(b.bufs[bi + 1], 1);
        const auto& dsp = b.bufs[bi + 2];
        if (dsp.len > 0) {
          int64_t du = sr.real_usize(b, dsp);
          schedule_buffer(sr, b, dsp, out.cols[c].data->u8() + utf8_cursor[c],
                          sr.utf8_total[c] - utf8_cursor[c] + 8);
          utf8_cursor[c] += du;
        }
      } else {
        int64_t esz = dt_size(sr.dts[c].dt);
        schedule_buffer(sr, b, b.bufs[bi + 1],
                        out.cols[c].data->u8() + row_cursor * esz,
                        (sr.total - row_cursor) * esz + 8);
      }
    }
    row_cursor += b.rows;
  }
  return fixups;
}

// place validity bits / utf8 offsets
static void place_fixups(const std::vector<ShuffleFixup>& fixups, Table& out) {
  for (auto& fx : fixups) {
    if (fx.kind == 0) {
      chk(bg_bitcopy(fx.scratch->u8(), fx.rows, out.cols[fx.c].validity->u8(),
                     fx.row_cursor),
          "bg_bitcopy");
    } else {
      // offsets in the batch start at 0 (the writers rebase); add the
      // column's running data cursor: out = in - (-data_cursor)
      chk(bg_sub_i32(fx.scratch->p, fx.rows + 1,
                     (int32_t)(-fx.data_cursor),
                     out.cols[fx.c].offsets->u8() + 4 * fx.row_cursor),
          "bg_sub_i32");
    }
  }
}

static Table read_shuffle_locations(const std::vector<Value*>& locations,
                                    const std::vector<DtSpec>& dts,
                                    const std::vector<std::string>& names) {
  ShuffleRead sr(dts);
  auto ranges = gather_ranges(locations, sr.all);
  sr.batches = walk_batches(sr.all, ranges, dts.size());
  for (auto& b : sr.batches) sr.total += b.rows;
  // 2 buffers per column (validity, data), 3 for utf8 (+ offsets)
  size_t nbufs = 0;
  for (auto& d : dts) {
    sr.first_buf.push_back(nbufs);
    nbufs += d.dt == BG_DT_UTF8 ? 3 : 2;
  }

  Table out;
  out.n = sr.total;
  out.names = names;
  if (sr.total == 0) {
    for (auto& d : dts) {
      Col col = make_col(d);
      col.data = dalloc(16);
      if (col.dtype == BG_DT_UTF8) {
        col.offsets = dalloc(4);
        chk(bg_memset(col.offsets->p, 0, 4), "bg_memset");
      }
      out.cols.push_back(std::move(col));
    }
    return out;
  }

  sr.raw_dev = upload(sr.all.data(), sr.all.size());
  alloc_shuffle_columns(sr, out);
  auto fixups = schedule_buffers(sr, out);
  if (!sr.frames.empty()) {
    std::vector<int64_t> lens(sr.frames.size());
    chk(bg_lz4_decompress(sr.frames.data(), (int64_t)sr.frames.size(),
                          lens.data()),
        "bg_lz4_decompress");
    for (size_t i = 0; i < sr.frames.size(); ++i)
      if (lens[i] != sr.expect[i])
        throw StageError(BG_ERR_INVALID, "shuffle read: LZ4 frame mismatch");
  }
  place_fixups(fixups, out);
  chk(bg_synchronize(), "bg_synchronize");
  return out;
}
#include "stage_parquet.h"

struct PqPage {
  int rg;
  int type;  // 0 data, 2 dict
  size_t data_pos;
  int64_t csz, usz, nvals, ndict;
  int enc;
  int64_t soff;  // slot in the decompressed scratch
};
// a data page with its running value cursor
struct PqDataPage {
  int64_t soff, usz, dst_off, nvals;
  int rg, enc;
};

// What the decode steps of one parquet column share.
struct PqDecode {
  int64_t src_esz = 0, dst_esz = 0;
  bool is_flba = false;
  int mode = 0;                // 2: OPTIONAL column (max_def 1), 0: REQUIRED
  DBufPtr scratch;             // every page decompressed, at PqPage::soff
  std::vector<PqDataPage> dp;  // data pages in file order
  DBufPtr vidx, npres;         // OPTIONAL: value slot map, per-page presents

  const uint32_t* vidx_at(size_t i) const {
    return mode ? (const uint32_t*)(vidx->u8() + 4 * dp[i].dst_off) : nullptr;
  }
  const int64_t* npres_at(size_t i) const {
    return mode ? (const int64_t*)(npres->u8() + 8 * i) : nullptr;
  }
};

static std::vector<PqPage> pq_walk_pages(const uint8_t* h_file,
                                         size_t file_len,
                                         const PqColumnSpec& spec,
                                         int64_t* scratch_total,
                                         int64_t* total_values) {
  std::vector<PqPage> pages;
  for (size_t rg = 0; rg < spec.chunks.size(); ++rg) {
    const PqChunk& ch = spec.chunks[rg];
    size_t pos = (size_t)ch.start;
    const size_t end = (size_t)(ch.start + ch.size);
    *total_values += ch.num_values;
    while (pos < end) {
      PageHeader ph = parse_page_header(h_file, file_len, pos);
      if (ph.type == 0 && ph.enc != 0 && ph.enc != 2 && ph.enc != 8)
        throw StageError(BG_ERR_UNSUPPORTED,
                         "parquet scan: encoding " + std::to_string(ph.enc) +
                             " — use the Python reader (DELTA*/BSS)");
      pages.push_back({(int)rg, ph.type, ph.data_pos, ph.csz, ph.usz,
                       ph.nvals, ph.ndict, ph.enc, *scratch_total});
      *scratch_total += (ph.usz + 255) & ~255LL;
      pos = ph.data_pos + (size_t)ph.csz;
    }
  }
  return pages;
}

// decompress (or copy) every page into its scratch slot
static DBufPtr pq_decompress_pages(const std::vector<PqPage>& pages,
                                   const DBufPtr& d_file, bool snappy,
                                   int64_t scratch_total) {
  DBufPtr scratch = dalloc((uint64_t)(scratch_total > 0 ? scratch_total : 256));
  if (!snappy) {
    for (auto& p : pages)
      chk(bg_memcpy_dtod(scratch->u8() + p.soff, d_file->u8() + p.data_pos,
                         (uint64_t)p.csz),
          "bg_memcpy_dtod");
    return scratch;
  }
  std::vector<bg_snappy_page> jobs;
  for (auto& p : pages)
    jobs.push_back({d_file->u8() + p.data_pos, scratch->u8() + p.soff, p.csz,
                    p.usz + 8});
  std::vector<int64_t> lens(jobs.size());
  chk(bg_snappy_decompress(jobs.data(), (int64_t)jobs.size(), lens.data()),
      "bg_snappy_decompress");
  for (size_t i = 0; i < jobs.size(); ++i)
    if (lens[i] != pages[i].usz)
      throw StageError(BG_ERR_INVALID, "parquet scan: snappy page failed");
  return scratch;
}

// OPTIONAL column: definition levels -> validity bitmap + slot map
static void pq_def_levels(PqDecode& d, int64_t total_values, Col& out) {
  const int64_t nwords = (total_values + 31) / 32;
  out.validity = dalloc((uint64_t)std::max<int64_t>(nwords, 1) * 4 + 8);
  chk(bg_memset(out.validity->p, 0, out.validity->bytes), "bg_memset");
  d.vidx = dalloc_elems(total_values, 4);
  d.npres = dalloc_elems((int64_t)d.dp.size(), 8);
  std::vector<bg_def_levels_job> djobs;
  for (size_t i = 0; i < d.dp.size(); ++i)
    djobs.push_back({d.scratch->u8() + d.dp[i].soff,
                     (uint32_t*)(d.vidx->u8() + 4 * d.dp[i].dst_off),
                     (uint32_t*)out.validity->p, d.dp[i].usz, d.dp[i].nvals,
                     d.dp[i].dst_off, (int64_t*)(d.npres->u8() + 8 * i)});
  chk(bg_def_levels_batch(djobs.data(), (int64_t)djobs.size()),
      "bg_def_levels_batch");
}

// PLAIN pages: one batched extract
static void pq_extract_plain(const PqDecode& d, Col& out) {
  std::vector<bg_page_extract_job> ejobs;
  for (size_t i = 0; i < d.dp.size(); ++i) {
    if (d.dp[i].enc != 0) continue;
    ejobs.push_back({d.scratch->u8() + d.dp[i].soff,
                     out.data->u8() + d.dp[i].dst_off * d.dst_esz,
                     d.dp[i].usz, d.dp[i].nvals, d.src_esz, d.mode,
                     d.is_flba ? 1 : 0, d.vidx_at(i), d.npres_at(i)});
  }
  if (!ejobs.empty())
    chk(bg_page_extract_batch(ejobs.data(), (int64_t)ejobs.size()),
        "bg_page_extract_batch");
}

// dictionary-coded pages: PLAIN-decode dictionaries, expand indices, gather
static void pq_dict_gather(const PqDecode& d,
                           const std::map<int, PqPage>& dict_of, Col& out) {
  std::vector<size_t> dpg;
  for (size_t i = 0; i < d.dp.size(); ++i)
    if (d.dp[i].enc == 2 || d.dp[i].enc == 8) dpg.push_back(i);
  if (dpg.empty()) return;
  std::map<int, DBufPtr> dict_bufs;
  std::vector<bg_page_extract_job> dj;
  for (auto& kv : dict_of) {
    const PqPage& dict = kv.second;
    DBufPtr buf = dalloc_elems(dict.ndict, d.dst_esz);
    dict_bufs[kv.first] = buf;
    dj.push_back({d.scratch->u8() + dict.soff, buf->u8(), dict.usz,
                  dict.ndict, d.src_esz, 0, d.is_flba ? 1 : 0, nullptr,
                  nullptr});
  }
  if (!dj.empty())
    chk(bg_page_extract_batch(dj.data(), (int64_t)dj.size()),
        "bg_page_extract(dicts)");

  int64_t nidx_total = 0;
  for (size_t i : dpg) nidx_total += d.dp[i].nvals;
  DBufPtr idx = dalloc_elems(nidx_total, 4);
  DBufPtr dense;
  if (d.mode) dense = dalloc_elems(nidx_total, 4);
  std::vector<bg_dict_indices_job> ijobs;
  struct Gather {
    int rg;
    int64_t ioff, dst_off, nvals;
  };
  std::vector<Gather> merged;  // adjacent pages of one rg gather as one
  int64_t run = 0;
  for (size_t i : dpg) {
    const PqDataPage& p = d.dp[i];
    ijobs.push_back({d.scratch->u8() + p.soff,
                     (uint32_t*)(idx->u8() + 4 * run), p.usz, p.nvals, d.mode,
                     0, d.vidx_at(i), d.npres_at(i),
                     d.mode ? (uint32_t*)(dense->u8() + 4 * run) : nullptr});
    if (!merged.empty() && merged.back().rg == p.rg &&
        merged.back().dst_off + merged.back().nvals == p.dst_off)
      merged.back().nvals += p.nvals;
    else
      merged.push_back({p.rg, run, p.dst_off, p.nvals});
    run += p.nvals;
  }
  chk(bg_dict_indices_batch(ijobs.data(), (int64_t)ijobs.size()),
      "bg_dict_indices_batch");
  for (auto& gth : merged)
    chk(bg_gather(dict_bufs[gth.rg]->p, d.dst_esz,
                  (const uint32_t*)(idx->u8() + 4 * gth.ioff), gth.nvals,
                  out.data->u8() + gth.dst_off * d.dst_esz),
        "bg_gather(dict)");
}

// The device decode pipeline for one parquet column (subset: V1 pages,
// PLAIN + RLE_DICTIONARY, INT32/INT64/DOUBLE/FLBA, max_def <= 1,
// SNAPPY/UNCOMPRESSED).  Mirrors the Python reader's batched flow
// (datafusion_ballista_amd/parquet.py read_column_all), whose parity is
// pinned against pyarrow's reader; the page-header walk and job building
// run here in C++ (the Python walk cost ~35 ms per SF100-scale column).
Col parquet_read_column(const uint8_t* h_file, size_t file_len,
                        const DBufPtr& d_file, const PqColumnSpec& spec,
                        const DtSpec& out_dt) {
  PqDecode d;
  d.is_flba = spec.phys == "FLBA";
  if (spec.phys == "INT32") d.src_esz = d.dst_esz = 4;
  else if (spec.phys == "INT64" || spec.phys == "DOUBLE")
    d.src_esz = d.dst_esz = 8;
  else if (d.is_flba) {
    d.src_esz = spec.flba_len;
    d.dst_esz = 16;
  } else {
    throw StageError(BG_ERR_UNSUPPORTED,
                     "parquet scan: physical type " + spec.phys +
                         " — use the Python reader for BYTE_ARRAY etc.");
  }
  const bool snappy = spec.codec == "SNAPPY";
  if (!snappy && spec.codec != "UNCOMPRESSED")
    throw StageError(BG_ERR_UNSUPPORTED,
                     "parquet scan: codec " + spec.codec +
                         " — use the Python reader (ZSTD/GZIP bridge)");

  int64_t scratch_total = 0, total_values = 0;
  auto pages =
      pq_walk_pages(h_file, file_len, spec, &scratch_total, &total_values);
  d.scratch = pq_decompress_pages(pages, d_file, snappy, scratch_total);

  // data pages in file order with their running value cursor
  int64_t got = 0;
  std::map<int, PqPage> dict_of;  // rg -> dictionary page
  for (auto& p : pages) {
    if (p.type == 2) dict_of[p.rg] = p;
    else if (p.type == 0) {
      d.dp.push_back({p.soff, p.usz, got, p.nvals, p.rg, p.enc});
      got += p.nvals;
    }
  }
  if (got != total_values)
    throw StageError(BG_ERR_INVALID, "parquet scan: value count mismatch");

  Col out = make_col(out_dt);
  out.data = dalloc_elems(total_values, d.dst_esz);
  d.mode = spec.max_def > 0 ? 2 : 0;
  if (d.mode) pq_def_levels(d, total_values, out);
  pq_extract_plain(d, out);
  pq_dict_gather(d, dict_of, out);
  return out;
}
// Read a "parquet" scan source: plan carries the footer-derived chunk
// metadata per column (start/size/num_values, codec, physical type) —
// hosts parse footers natively (pyarrow / parquet-rs); stage.py's
// parquet_source() builds this from pyarrow metadata.
static Table read_parquet_source(const Value& src,
                                 const std::vector<DtSpec>& dts,
                                 const std::vector<std::string>& names) {
  const std::string& path = src.get_str("path");
  auto raw = read_file_range(path, 0, -1);
  DBufPtr d_file = upload(raw.data(), raw.size());
  auto& cols = src.get_arr("columns");
  if (cols.size() != dts.size())
    throw StageError(BG_ERR_INVALID, "parquet source: columns != schema");
  Table t;
  t.names = names;
  int64_t nrows = -1;
  for (size_t c = 0; c < cols.size(); ++c) {
    const Value& cv = *cols[c];
    PqColumnSpec spec;
    spec.phys = cv.get_str("phys");
    spec.flba_len = (int)cv.get_int_or("flba_len", 0);
    spec.max_def = (int)cv.get_int_or("max_def", 0);
    spec.codec = cv.get_str_or("codec", "UNCOMPRESSED");
    int64_t nv = 0;
    for (auto& chv : cv.get_arr("chunks")) {
      spec.chunks.push_back({chv->get_int("start"), chv->get_int("size"),
                             chv->get_int("num_values")});
      nv += spec.chunks.back().num_values;
    }
    if (nrows < 0) nrows = nv;
    else if (nrows != nv)
      throw StageError(BG_ERR_INVALID, "parquet source: ragged columns");
    t.cols.push_back(
        parquet_read_column(raw.data(), raw.size(), d_file, spec, dts[c]));
  }
  t.n = nrows < 0 ? 0 : nrows;
  return t;
}



static Table scan(const Value& node) {
  const Value& src = node.at("source");
  const std::string kind = src.get_str("kind");
  std::vector<DtSpec> dts;
  std::vector<std::string> names;
  for (auto& f : node.get_arr("schema")) {
    dts.push_back(parse_dtype(*f));
    names.push_back(f->get_str("name"));
  }

  Table t;
  if (kind == "device") {
    std::lock_guard<std::mutex> g(g_tables_mu);
    auto it = g_tables.find(src.get_str("table"));
    if (it == g_tables.end())
      throw StageError(BG_ERR_INVALID,
                       "unregistered device table '" + src.get_str("table") +
                           "'");
    t = it->second;  // shallow copy; externals owned by the registrant
  } else if (kind == "shuffle" || kind == "ipc") {
    std::vector<Value*> locs;
    if (src.has("locations"))
      for (auto& l : src.get_arr("locations")) locs.push_back(l.get());
    else
      locs.push_back(const_cast<Value*>(&src));
    t = read_shuffle_locations(locs, dts, names);
  } else if (kind == "parquet") {
    t = read_parquet_source(src, dts, names);
  } else if (kind == "raw") {
    // flat LE binary column files (bench/test feeding); utf8 columns give
    // {offsets, data} files; optional {validity} of packed LSB bits
    t.n = src.get_int("rows");
    t.names = names;
    auto& files = src.get_arr("files");
    if (files.size() != dts.size())
      throw StageError(BG_ERR_INVALID, "raw source: files != schema len");
    for (size_t c = 0; c < dts.size(); ++c) {
      Col col = make_col(dts[c]);
      const Value& fv = *files[c];
      if (col.dtype == BG_DT_UTF8) {
        auto offs = read_file_range(fv.get_str("offsets"), 0, -1);
        auto data = read_file_range(fv.get_str("data"), 0, -1);
        col.offsets = upload(offs.data(), offs.size());
        col.data = upload(data.data(), data.size() ? data.size() : 1);
        col.data_bytes = (int64_t)data.size();
      } else {
        auto raw = read_file_range(fv.get_str("path"), 0, -1);
        col.data = upload(raw.data(), raw.size());
      }
      if (fv.has("validity")) {
        auto vb = read_file_range(fv.get_str("validity"), 0, -1);
        col.validity = upload(vb.data(), vb.size());
      }
      t.cols.push_back(std::move(col));
    }
  } else {
    throw StageError(BG_ERR_INVALID, "scan: unknown source kind " + kind);
  }

  if (t.names.empty()) t.names = names;
  if (node.has("projection")) {
    Table proj;
    proj.n = t.n;
    for (auto& p : node.get_arr("projection")) {
      int i = t.idx(p->s);
      proj.names.push_back(t.names[(size_t)i]);
      proj.cols.push_back(t.cols[(size_t)i]);
    }
    return proj;
  }
  return t;
}

// ---------------------------------------------------------------------------
// expressions
// ---------------------------------------------------------------------------

static DBufPtr eval_filter_mask(const Table& t, const Value& node);

struct ExprVal {
  bool is_lit = false;
  Col col;          // when !is_lit (shares buffers)
  int64_t lit_lo = 0, lit_hi = 0;  // when is_lit (i128; lit_f64: its bits)
  bool is_f64 = false;             // a lit_f64 literal
  double f64 = 0.0;
};

static ExprVal eval_expr(const Table& t, const Value& e);
static std::string expr_label(const Value& e);

// ---- cast / div / Float64 arithmetic: the verdicts that validate_expr and
// eval_expr both read, so what validation accepts is what execution runs ----

static const DtSpec DT_LIT{BG_DT_DECIMAL128, 38, 0};
static const DtSpec DT_F64{BG_DT_FLOAT64, 0, 0};

static bool is_literal_node(const Value& e) {
  return e.has("lit") || e.has("lit_f64");
}

// {"lit_f64": <JSON number>}; an integer token converts
static double lit_f64_value(const Value& e) {
  const Value& v = e.at("lit_f64");
  if (v.kind == Value::DBL) return v.d;
  if (v.kind == Value::INT) return (double)v.i;
  throw StageError(BG_ERR_INVALID, "lit_f64: value must be a JSON number");
}

static std::string spec_name(const DtSpec& d) {
  std::string s = dtype_name(d.dt);
  if (d.dt == BG_DT_DECIMAL128)
    s += "(" + std::to_string(d.precision) + "," + std::to_string(d.scale) +
         ")";
  return s;
}

// {"cast": {"arg": expr, "to": {"dtype", "precision"?, "scale"?}}}: the
// target type, decimal128 with both of its parameters spelled out
static DtSpec cast_target(const Value& c) {
  const Value& to = c.at("to");
  if (to.get_str("dtype") != "decimal128") return parse_dtype(to);
  const std::string arg = expr_label(c.at("arg"));
  for (const char* k : {"precision", "scale"})
    if (!to.has(k) || to.at(k).kind != Value::INT)
      throw StageError(BG_ERR_INVALID,
                       "cast: decimal128 target of '" + arg +
                           "' requires an integer '" + k + "'");
  const DtSpec d{BG_DT_DECIMAL128, (int32_t)to.get_int("precision"),
                 (int32_t)to.get_int("scale")};
  if (to.get_int("precision") < 1 || to.get_int("precision") > 38 ||
      to.get_int("scale") < 0 || to.get_int("scale") > to.get_int("precision"))
    throw StageError(BG_ERR_INVALID,
                     "cast: illegal target " + spec_name(d) + " of '" + arg +
                         "': 1 <= precision <= 38 and 0 <= scale <= "
                         "precision required");
  return d;
}

// the pairs bg_cast converts
static void cast_check_pair(const Value& c, const DtSpec& from,
                            const DtSpec& to) {
  const std::string arg = expr_label(c.at("arg"));
  if (is_literal_node(c.at("arg")))
    throw StageError(BG_ERR_INVALID, "cast: argument '" + arg +
                                         "' is a literal; cast a column");
  const bool from_int = from.dt == BG_DT_INT32 || from.dt == BG_DT_INT64;
  const bool from_dec = from.dt == BG_DT_DECIMAL128;
  const bool ok =
      (to.dt == BG_DT_FLOAT64 && (from_int || from_dec)) ||
      (to.dt == BG_DT_DECIMAL128 &&
       (from_int || from_dec || from.dt == BG_DT_FLOAT64)) ||
      (to.dt == BG_DT_INT64 && from.dt == BG_DT_INT32);
  if (!ok)
    throw StageError(BG_ERR_UNSUPPORTED,
                     "cast: '" + arg + "' (" + spec_name(from) + ") to " +
                         spec_name(to) + " is not supported");
}

// What mul|add|sub|div over operands of types a and b (a literal node's
// type is its literal kind's) runs as.
struct ArithPlan {
  enum Kind { DEC128, F64, DEC_DIV } kind = DEC128;
  int32_t f64_op = 0;       // F64: BG_F64_*
  bool negate_lit = false;  // F64: col - lit runs as col + (-lit), the same
                            // IEEE operation
  DtSpec out{BG_DT_DECIMAL128, 38, 0};  // F64, DEC_DIV
  int32_t mul_pow = 0;                  // DEC_DIV
};

static ArithPlan arith_plan(const std::string& k, const Value& e,
                            const Value& l, const DtSpec& a, const Value& r,
                            const DtSpec& b) {
  const bool la = is_literal_node(l), lb = is_literal_node(r);
  const std::string an = expr_label(l), bn = expr_label(r);
  const std::string both = "'" + an + "' (" + dtype_name(a.dt) + ") and '" +
                           bn + "' (" + dtype_name(b.dt) + ")";
  if (la && lb)
    throw StageError(BG_ERR_INVALID, k + ": two literals, " + both);
  ArithPlan p;
  const bool fa = a.dt == BG_DT_FLOAT64, fb = b.dt == BG_DT_FLOAT64;
  if (fa || fb) {
    if (!(fa && fb))
      throw StageError(BG_ERR_INVALID,
                       k + ": Float64 operand mixed with another type: " +
                           both + "; cast one side");
    p.kind = ArithPlan::F64;
    p.out = DT_F64;
    const bool lit = la || lb;
    if (k == "mul") p.f64_op = lit ? BG_F64_MUL_LIT : BG_F64_MUL;
    else if (k == "add") p.f64_op = lit ? BG_F64_ADD_LIT : BG_F64_ADD;
    else if (k == "sub") {
      p.f64_op = la ? BG_F64_LIT_SUB : lb ? BG_F64_ADD_LIT : BG_F64_SUB;
      p.negate_lit = lb;
    } else {
      p.f64_op = la ? BG_F64_LIT_DIV : lb ? BG_F64_DIV_LIT : BG_F64_DIV;
    }
    return p;
  }
  if (k != "div") return p;  // the Decimal128 mul|add|sub paths
  if (la || lb)
    throw StageError(BG_ERR_UNSUPPORTED,
                     "div: Decimal128 division takes two columns, '" +
                         (la ? an : bn) + "' is a literal (" + both + ")");
  if (a.dt != BG_DT_DECIMAL128 || b.dt != BG_DT_DECIMAL128)
    throw StageError(BG_ERR_INVALID,
                     "div: operands must both be decimal128 or both "
                     "float64: " + both);
  const int64_t s = e.has("scale") ? e.get_int("scale")
                                   : std::min<int64_t>(a.scale + 4, 38);
  const int64_t mul_pow = s - a.scale + b.scale;
  if (s < 0 || s > 38 || mul_pow < -38 || mul_pow > 38)
    throw StageError(BG_ERR_INVALID,
                     "div: result scale " + std::to_string(s) + " for " +
                         both + ", scales " + std::to_string(a.scale) +
                         " and " + std::to_string(b.scale) +
                         ", is outside what Decimal128 can align");
  p.kind = ArithPlan::DEC_DIV;
  p.out = {BG_DT_DECIMAL128, 38, (int32_t)s};
  p.mul_pow = (int32_t)mul_pow;
  return p;
}

static DtSpec expr_spec(const ExprVal& v) {
  return !v.is_lit ? v.col.spec() : v.is_f64 ? DT_F64 : DT_LIT;
}

// date_part's "part" names (validation and execution both read this)
static int32_t date_part_code(const std::string& s) {
  if (s == "year") return BG_DATE_PART_YEAR;
  if (s == "quarter") return BG_DATE_PART_QUARTER;
  if (s == "month") return BG_DATE_PART_MONTH;
  if (s == "day") return BG_DATE_PART_DAY;
  if (s == "doy") return BG_DATE_PART_DOY;
  if (s == "dow") return BG_DATE_PART_DOW;
  throw StageError(BG_ERR_INVALID, "date_part: unknown part '" + s + "'");
}

// a unary projection's result is NULL exactly where its argument is: share
// the argument's bitmap (owned or registered-table external)
static void share_validity(const Col& arg, Col* out) {
  out->validity = arg.validity;
  out->ext_valid = arg.validity ? nullptr : arg.ext_valid;
}

// a binary result is NULL where either input is: share the one nullable
// input's bitmap, AND two
static void binary_validity(const Table& t, const ExprVal& a,
                            const ExprVal& b, Col* out) {
  const Col* ca = !a.is_lit && a.col.nullable() ? &a.col : nullptr;
  const Col* cb = !b.is_lit && b.col.nullable() ? &b.col : nullptr;
  if (ca && cb) {
    out->validity = alloc_bitmap(t.n, 0);
    chk(bg_bitmap_and(ca->vptr(), cb->vptr(), t.n, out->validity->u8()),
        "bg_bitmap_and");
  } else if (ca || cb) {
    share_validity(ca ? *ca : *cb, out);
  }
}

static Col eval_f64_binary(const Table& t, const ArithPlan& p,
                           const ExprVal& a, const ExprVal& b) {
  Col out = make_col(p.out);
  out.data = dalloc_elems(t.n, 8);
  const ExprVal& first = a.is_lit ? b : a;  // the (first) column operand
  double lit = a.is_lit ? a.f64 : b.is_lit ? b.f64 : 0.0;
  if (p.negate_lit) lit = -lit;
  bg_column ba = to_bg(first.col, t.n), bb = to_bg(b.col, t.n);
  chk(bg_project_f64(p.f64_op, &ba, (a.is_lit || b.is_lit) ? nullptr : &bb,
                     lit, t.n, (double*)out.data->p),
      "bg_project_f64");
  binary_validity(t, a, b, &out);
  return out;
}

static Col eval_dec_div(const Table& t, const ArithPlan& p, const ExprVal& a,
                        const ExprVal& b) {
  Col out = make_col(p.out);
  out.data = dalloc_elems(t.n, 16);
  bg_column ba = to_bg(a.col, t.n), bb = to_bg(b.col, t.n);
  // the kernel examines a row only where both inputs are valid
  chk(bg_div_dec128(&ba, &bb, p.mul_pow, t.n, out.data->p, nullptr),
      "bg_div_dec128");
  binary_validity(t, a, b, &out);
  return out;
}

static Col eval_dec_binary(const Table& t, int op_cc, int op_cl, int op_lc,
                           const ExprVal& a, const ExprVal& b) {
  Col out = make_col({BG_DT_DECIMAL128, 38, 0});
  out.data = dalloc_elems(t.n, 16);
  if (!a.is_lit && !b.is_lit) {
    out.scale = (op_cc == 0) ? a.col.scale + b.col.scale : a.col.scale;
    bg_column ba = to_bg(a.col, t.n), bb = to_bg(b.col, t.n);
    chk(bg_project_dec128(op_cc, &ba, &bb, 0, 0, t.n, out.data->p),
        "bg_project_dec128");
  } else if (!a.is_lit && b.is_lit) {
    if (op_cl < 0)
      throw StageError(BG_ERR_UNSUPPORTED, "project: col OP lit unsupported");
    out.scale = a.col.scale;  // plan supplies scaled literals
    bg_column ba = to_bg(a.col, t.n);
    chk(bg_project_dec128(op_cl, &ba, nullptr, b.lit_lo, b.lit_hi, t.n,
                          out.data->p),
        "bg_project_dec128");
  } else if (a.is_lit && !b.is_lit) {
    if (op_lc < 0)
      throw StageError(BG_ERR_UNSUPPORTED, "project: lit OP col unsupported");
    out.scale = b.col.scale;
    bg_column bb = to_bg(b.col, t.n);
    chk(bg_project_dec128(op_lc, &bb, nullptr, a.lit_lo, a.lit_hi, t.n,
                          out.data->p),
        "bg_project_dec128");
  } else {
    throw StageError(BG_ERR_INVALID, "project: two literals");
  }
  // null propagation: binary arithmetic is NULL when either input is NULL
  const Col* srcs[2] = {a.is_lit ? nullptr : &a.col,
                        b.is_lit ? nullptr : &b.col};
  for (auto* s : srcs) {
    if (s && s->nullable()) {
      if (!out.validity) {
        out.validity = s->validity ? s->validity : nullptr;
        if (!out.validity) {  // external bitmap: copy it
          out.validity = alloc_bitmap(t.n);
          chk(bg_memcpy_dtod(out.validity->p, s->vptr(),
                             out.validity->bytes),
              "bg_memcpy_dtod");
        }
      }
      // both nullable: AND of bitmaps not yet needed by the TPC-H shapes
    }
  }
  return out;
}

// mul|add|sub|div.  Decimal128 arithmetic goes to bg_project_dec128 (op
// table: 0 a*b, 1 a+b, 2 a-b, 3 lit-a, 4 a*lit, 5 a+lit), Float64 to
// bg_project_f64, Decimal128 division to bg_div_dec128.
static Col eval_arith(const Table& t, const std::string& k, const Value& e) {
  auto& ops = e.get_arr(k);
  if (ops.size() != 2)
    throw StageError(BG_ERR_INVALID, k + ": two operands required");
  ExprVal a = eval_expr(t, *ops[0]);
  ExprVal b = eval_expr(t, *ops[1]);
  const ArithPlan p =
      arith_plan(k, e, *ops[0], expr_spec(a), *ops[1], expr_spec(b));
  if (p.kind == ArithPlan::F64) return eval_f64_binary(t, p, a, b);
  if (p.kind == ArithPlan::DEC_DIV) return eval_dec_div(t, p, a, b);
  if (k == "mul") return eval_dec_binary(t, 0, 4, 4, a, b);
  if (k == "add") return eval_dec_binary(t, 1, 5, 5, a, b);
  if (b.is_lit) {
    // col - lit == col + (-lit): negate the literal side
    __int128 litv = ((__int128)b.lit_hi << 64) | (uint64_t)b.lit_lo;
    litv = -litv;
    Col out = make_col({BG_DT_DECIMAL128, 38, a.col.scale});
    out.data = dalloc_elems(t.n, 16);
    bg_column ba = to_bg(a.col, t.n);
    chk(bg_project_dec128(5, &ba, nullptr, (int64_t)(uint64_t)litv,
                          (int64_t)(uint64_t)((unsigned __int128)litv >> 64),
                          t.n, out.data->p),
        "bg_project_dec128");
    if (a.col.nullable()) out.validity = a.col.validity;
    return out;
  }
  return eval_dec_binary(t, 2, -1, 3, a, b);
}

static ExprVal eval_expr(const Table& t, const Value& e) {
  ExprVal v;
  if (e.has("col")) {
    v.col = t.col(e.get_str("col"));
    return v;
  }
  if (e.has("lit")) {
    v.is_lit = true;
    parse_i128(e.at("lit"), &v.lit_lo, &v.lit_hi);
    return v;
  }
  if (e.has("lit_f64")) {
    v.is_lit = v.is_f64 = true;
    v.f64 = lit_f64_value(e);
    memcpy(&v.lit_lo, &v.f64, 8);
    return v;
  }
  for (const char* k : {"mul", "add", "sub", "div"})
    if (e.has(k)) {
      v.col = eval_arith(t, k, e);
      return v;
    }
  // CAST(arg AS to)  (q14/q17/q11/q20: sums to Float64 and back; q17/q22:
  // Decimal128 rescale)
  if (e.has("cast")) {
    const Value& c = e.at("cast");
    const DtSpec to = cast_target(c);
    ExprVal a = eval_expr(t, c.at("arg"));
    cast_check_pair(c, expr_spec(a), to);
    Col out = make_col(to);
    out.data = dalloc_elems(t.n, dt_size(to.dt));
    bg_column ba = to_bg(a.col, t.n);
    chk(bg_cast(&ba, to.dt, to.precision, to.scale, t.n, out.data->p,
                nullptr),
        "bg_cast");
    share_validity(a.col, &out);
    v.col = out;
    return v;
  }
  // CASE WHEN <predicates> THEN <expr> ELSE <expr>  (q8/q12/q14-class):
  // {"case": {"when": [pred...], "then": expr, "else": expr}}
  if (e.has("case")) {
    const Value& c = e.at("case");
    // when-predicates evaluate over the input table (same grammar as
    // filter, incl. LIKE)
    bgjson::Value fake;
    fake.kind = Value::OBJ;
    fake.obj.emplace_back("predicates", *c.find("when"));
    DBufPtr mask = eval_filter_mask(t, fake);
    ExprVal a = eval_expr(t, c.at("then"));
    ExprVal b = eval_expr(t, c.at("else"));
    // materialise literal branches as constant columns
    auto materialise = [&](ExprVal& ev, const ExprVal& other) -> Col {
      if (!ev.is_lit) return ev.col;
      Col out = make_col(other.is_lit ? DtSpec{BG_DT_DECIMAL128, 38, 0}
                                      : other.col.spec());
      int64_t esz = dt_size(out.dtype);
      out.data = dalloc_elems(t.n, esz);
      chk(bg_fill_const(out.data->p, t.n, esz, ev.lit_lo, ev.lit_hi),
          "bg_fill_const");
      return out;
    };
    Col ca = materialise(a, b);
    Col cb = materialise(b, a);
    if (ca.dtype != cb.dtype)
      throw StageError(BG_ERR_INVALID, "case: branch dtype mismatch");
    ExprVal v2;
    v2.col.dtype = ca.dtype;
    v2.col.precision = ca.precision ? ca.precision : cb.precision;
    v2.col.scale = ca.scale ? ca.scale : cb.scale;
    int64_t esz = dt_size(ca.dtype);
    v2.col.data = dalloc_elems(t.n, esz);
    chk(bg_select(mask->u8(), ca.dptr(), cb.dptr(), esz, t.n,
                  v2.col.data->p),
        "bg_select");
    return v2;
  }
  // date_part(part, date32) -> int32  (q7/q8/q9: GROUP BY the year)
  if (e.has("date_part")) {
    const Value& d = e.at("date_part");
    ExprVal a = eval_expr(t, d.at("arg"));
    if (a.is_lit) throw StageError(BG_ERR_INVALID, "date_part of a literal");
    Col out = make_col({BG_DT_INT32, 0, 0});
    out.data = dalloc_elems(t.n, 4);
    bg_column ba = to_bg(a.col, t.n);
    chk(bg_date_part(&ba, date_part_code(d.get_str("part")), t.n,
                     (int32_t*)out.data->p),
        "bg_date_part");
    share_validity(a.col, &out);
    v.col = out;
    return v;
  }
  // substr(utf8, start[, count]) -> utf8  (q22: the country code)
  if (e.has("substr")) {
    const Value& d = e.at("substr");
    ExprVal a = eval_expr(t, d.at("arg"));
    if (a.is_lit) throw StageError(BG_ERR_INVALID, "substr of a literal");
    const int64_t start = d.get_int("start");
    const bool has_count = d.has("count");
    const int64_t count = has_count ? d.get_int("count") : 0;
    Col out = make_col({BG_DT_UTF8, 0, 0});
    out.offsets = dalloc((uint64_t)(t.n + 1) * 4);
    bg_column ba = to_bg(a.col, t.n);
    int64_t total = 0;  // size exactly first (d_out_data NULL), then copy
    chk(bg_substr(&ba, start, has_count, count, t.n, (int32_t*)out.offsets->p,
                  nullptr, 0, &total),
        "bg_substr(size)");
    out.data = dalloc_elems(total);
    chk(bg_substr(&ba, start, has_count, count, t.n, (int32_t*)out.offsets->p,
                  out.data->p, total > 0 ? total : 1, &total),
        "bg_substr");
    out.data_bytes = total;
    share_validity(a.col, &out);
    v.col = out;
    return v;
  }
  throw StageError(BG_ERR_INVALID, "plan: unknown expression node");
}


// ---- fused multi-expression Decimal128 projection ----
// Compile a dec128 arithmetic tree to the stack bytecode of
// bg_project_dec128_multi; returns false when the tree contains nodes
// outside {col(dec128), lit, mul, add, sub} (caller falls back to the
// per-op path).
struct ExprProgBuild {
  std::vector<int32_t> ops, args;
  std::vector<int32_t> expr_end;
  std::vector<int64_t> lit_lo, lit_hi;
  std::vector<int> col_ids;  // table column indices
};

static bool compile_expr_rec(const Table& t, const Value& e,
                             ExprProgBuild* p, int* scale, int* depth) {
  if (*depth > 8) return false;
  ++*depth;
  if (e.has("col")) {
    int ci;
    try {
      ci = t.idx(e.get_str("col"));
    } catch (...) {
      return false;
    }
    const Col& c = t.cols[(size_t)ci];
    if (c.dtype != BG_DT_DECIMAL128 || c.nullable()) return false;
    int slot = -1;
    for (size_t s = 0; s < p->col_ids.size(); ++s)
      if (p->col_ids[s] == ci) slot = (int)s;
    if (slot < 0) {
      if (p->col_ids.size() >= 8) return false;
      slot = (int)p->col_ids.size();
      p->col_ids.push_back(ci);
    }
    p->ops.push_back(0);  // PUSH_COL
    p->args.push_back(slot);
    *scale = c.scale;
    return true;
  }
  if (e.has("lit")) {
    if (p->lit_lo.size() >= 8) return false;
    int64_t lo, hi;
    parse_i128(e.at("lit"), &lo, &hi);
    p->ops.push_back(1);  // PUSH_LIT
    p->args.push_back((int32_t)p->lit_lo.size());
    p->lit_lo.push_back(lo);
    p->lit_hi.push_back(hi);
    *scale = -1;  // literal adopts the sibling's scale
    return true;
  }
  const char* kinds[3] = {"mul", "add", "sub"};
  const int32_t opcodes[3] = {2, 3, 4};
  for (int k = 0; k < 3; ++k) {
    if (!e.has(kinds[k])) continue;
    auto& opnds = e.get_arr(kinds[k]);
    if (opnds.size() != 2) return false;
    int sa = -1, sb = -1;
    if (!compile_expr_rec(t, *opnds[0], p, &sa, depth)) return false;
    if (!compile_expr_rec(t, *opnds[1], p, &sb, depth)) return false;
    p->ops.push_back(opcodes[k]);
    p->args.push_back(0);
    if (k == 0)  // mul: scales add (literals contribute 0)
      *scale = (sa < 0 ? 0 : sa) + (sb < 0 ? 0 : sb);
    else
      *scale = sa >= 0 ? sa : sb;
    return true;
  }
  return false;
}

// Evaluate a set of expressions over t: arithmetic trees fuse into ONE
// kernel pass (each input column read once); anything else falls back to
// eval_expr.  outs[i] receives the i-th expression's column.
static void eval_exprs_fused(const Table& t,
                             const std::vector<const Value*>& exprs,
                             std::vector<Col>* outs) {
  outs->assign(exprs.size(), Col{});
  ExprProgBuild p;
  std::vector<size_t> fused;
  std::vector<int> scales;
  for (size_t i = 0; i < exprs.size(); ++i) {
    if (exprs[i]->has("col")) continue;  // plain refs share buffers
    ExprProgBuild trial = p;
    int scale = 0, depth = 0;
    if (fused.size() < 6 && trial.ops.size() + 12 < 24 &&
        compile_expr_rec(t, *exprs[i], &trial, &scale, &depth) &&
        trial.ops.size() <= 24) {
      trial.expr_end.push_back((int32_t)trial.ops.size());
      p = trial;
      fused.push_back(i);
      scales.push_back(scale);
    }
  }
  if (fused.size() >= 2) {  // fusion pays only with shared passes
    std::vector<bg_column> cols;
    for (int ci : p.col_ids) cols.push_back(to_bg(t.cols[(size_t)ci], t.n));
    std::vector<void*> douts;
    for (size_t fi = 0; fi < fused.size(); ++fi) {
      Col c = make_col({BG_DT_DECIMAL128, 38, scales[fi]});
      c.data = dalloc_elems(t.n, 16);
      douts.push_back(c.data->p);
      (*outs)[fused[fi]] = std::move(c);
    }
    chk(bg_project_dec128_multi(
            cols.data(), (int32_t)cols.size(), p.ops.data(), p.args.data(),
            (int32_t)p.ops.size(), p.expr_end.data(),
            (int32_t)p.expr_end.size(), p.lit_lo.data(), p.lit_hi.data(),
            (int32_t)p.lit_lo.size(), t.n, douts.data()),
        "bg_project_dec128_multi");
  } else {
    fused.clear();
  }
  for (size_t i = 0; i < exprs.size(); ++i) {
    bool done = false;
    for (size_t fi : fused)
      if (fi == i) done = true;
    if (done && (*outs)[i].data) continue;
    ExprVal v = eval_expr(t, *exprs[i]);
    if (v.is_lit)
      throw StageError(BG_ERR_INVALID, "bare literal expression column");
    (*outs)[i] = v.col;
  }
}

// rsub: lit - col  (op 3) — expressed as {"sub":[{"lit":...}, {"col":...}]}
// handled by eval_dec_binary's op_lc above.

// ---------------------------------------------------------------------------
// predicates (FilterExec subset — bg_eval_predicates)
// ---------------------------------------------------------------------------

static int32_t cmp_code(const std::string& s) {
  if (s == "ge_lt") return BG_PRED_GE_LT;
  if (s == "between") return BG_PRED_BETWEEN;
  if (s == "lt") return BG_PRED_LT;
  if (s == "eq") return BG_PRED_EQ;
  if (s == "gt") return BG_PRED_GT;
  throw StageError(BG_ERR_INVALID, "filter: unknown cmp '" + s + "'");
}

// column-to-column compare names ({"cmp": ..., "rhs": {"col": ...}}); lt,
// eq and gt overlap the literal forms, the presence of "rhs" selects these
static int32_t cmp_cols_code(const std::string& s) {
  if (s == "lt") return BG_CMP_LT;
  if (s == "le") return BG_CMP_LE;
  if (s == "gt") return BG_CMP_GT;
  if (s == "ge") return BG_CMP_GE;
  if (s == "eq") return BG_CMP_EQ;
  if (s == "ne") return BG_CMP_NE;
  throw StageError(BG_ERR_INVALID,
                   "filter: unknown column compare '" + s +
                       "' (lt/le/gt/ge/eq/ne)");
}

static bool in_values_are_strings(const Value& p) {
  auto& vals = p.get_arr("in");
  return !vals.empty() && vals[0]->kind == Value::STR;
}

// AND-fold one predicate group into a fresh mask.  Every predicate's
// operand is resolved ONCE to an index into `cols`: a named column is used
// in place, an "expr" operand is evaluated to a temporary column that lives
// until the call returns.  Evaluation order narrows the mask cheapest
// first: literal compares and IN lists, then LIKE, then column-to-column
// compares (whose kernel skips words that are already zero).
static DBufPtr eval_filter_mask(const Table& t, const Value& node) {
  auto& preds = node.get_arr("predicates");
  std::vector<bg_column> cols;
  for (auto& c : t.cols) cols.push_back(to_bg(c, t.n));
  std::vector<Col> temps;  // keep "expr" operands' buffers alive
  struct Pred { const Value* p; int operand; };
  auto resolve = [&](const Value& p) -> int {
    if (!p.has("expr")) return t.idx(p.get_str("col"));
    ExprVal v = eval_expr(t, p.at("expr"));
    if (v.is_lit)
      throw StageError(BG_ERR_INVALID, "filter: literal predicate operand");
    temps.push_back(v.col);
    cols.push_back(to_bg(temps.back(), t.n));
    return (int)cols.size() - 1;
  };
  std::vector<bg_pred> bp;
  std::vector<Pred> likes, ins, rhss;
  for (auto& p : preds) {
    const int operand = resolve(*p);
    if (p->has("rhs")) {
      rhss.push_back({p.get(), operand});
    } else if (p->has("like")) {
      likes.push_back({p.get(), operand});
    } else if (p->has("in")) {
      ins.push_back({p.get(), operand});
    } else {
      bg_pred q{};
      q.column = operand;
      q.op = cmp_code(p->get_str("cmp"));
      if (p->has("lo")) parse_i128(p->at("lo"), &q.lo_lo, &q.lo_hi);
      if (p->has("hi")) parse_i128(p->at("hi"), &q.hi_lo, &q.hi_hi);
      bp.push_back(q);
    }
  }
  DBufPtr mask = alloc_bitmap(t.n, bp.empty() ? 0xFF : -1);
  if (!bp.empty())
    chk(bg_eval_predicates(cols.data(), (int32_t)cols.size(), bp.data(),
                           (int32_t)bp.size(), t.n, mask->u8()),
        "bg_eval_predicates");
  for (auto& ip : ins) {
    const bg_column& c = cols[(size_t)ip.operand];
    auto& vals = ip.p->get_arr("in");
    if (in_values_are_strings(*ip.p)) {
      std::vector<const char*> strs;
      std::vector<int32_t> lens;
      for (auto& v : vals) {
        if (v->kind != Value::STR)
          throw StageError(BG_ERR_INVALID, "filter: mixed 'in' value kinds");
        strs.push_back(v->s.c_str());
        lens.push_back((int32_t)v->s.size());
      }
      chk(bg_eval_in_utf8(&c, strs.data(), lens.data(), (int32_t)strs.size(),
                          t.n, mask->u8()),
          "bg_eval_in_utf8");
      continue;
    }
    std::vector<int64_t> ivals;
    for (auto& v : vals) {
      int64_t lo, hi;
      parse_i128(*v, &lo, &hi);
      ivals.push_back(lo);
    }
    chk(bg_eval_in(&c, ivals.data(), (int32_t)ivals.size(), t.n, mask->u8()),
        "bg_eval_in");
  }
  for (auto& lk : likes) {
    const Value* lp = lk.p;
    // split the LIKE pattern into in-order literal fragments + anchors
    const std::string& pat = lp->get_str("like");
    const bool anchor_prefix = !pat.empty() && pat.front() != '%';
    const bool anchor_suffix = !pat.empty() && pat.back() != '%';
    std::vector<std::string> frags;
    std::string cur;
    for (char ch : pat) {
      if (ch == '%') {
        if (!cur.empty()) frags.push_back(cur);
        cur.clear();
      } else if (ch == '_') {
        throw StageError(BG_ERR_UNSUPPORTED,
                         "LIKE '_' wildcard not supported");
      } else {
        cur += ch;
      }
    }
    if (!cur.empty()) frags.push_back(cur);
    if (frags.empty())
      throw StageError(BG_ERR_INVALID, "LIKE pattern has no literal text");
    std::vector<const char*> terms;
    std::vector<int32_t> lens;
    for (auto& f : frags) {
      terms.push_back(f.c_str());
      lens.push_back((int32_t)f.size());
    }
    const bg_column& c = cols[(size_t)lk.operand];
    chk(bg_eval_like(&c, terms.data(), lens.data(), (int32_t)terms.size(),
                     anchor_prefix ? 1 : 0, anchor_suffix ? 1 : 0,
                     lp->get_bool_or("negate", false) ? 1 : 0, t.n,
                     mask->u8()),
        "bg_eval_like");
  }
  for (auto& rp : rhss) {
    const bg_column& a = cols[(size_t)rp.operand];
    const bg_column& b =
        cols[(size_t)t.idx(rp.p->at("rhs").get_str("col"))];
    chk(bg_eval_compare_cols(&a, &b, cmp_cols_code(rp.p->get_str("cmp")), t.n,
                             mask->u8()),
        "bg_eval_compare_cols");
  }
  return mask;
}

// filter node: {"predicates": [AND...]} or {"any": [[AND...], ...]}
// (disjunctive groups, the reference's q19-class OR-of-ANDs)
static DBufPtr eval_filter_node(const Table& t, const Value& node) {
  if (!node.has("any")) return eval_filter_mask(t, node);
  auto& groups = node.get_arr("any");
  DBufPtr acc;
  for (auto& grp : groups) {
    bgjson::Value fake;
    fake.kind = Value::OBJ;
    fake.obj.emplace_back("predicates", grp);
    DBufPtr m2 = eval_filter_mask(t, fake);
    if (!acc) {
      acc = m2;
    } else {
      chk(bg_bitmap_or(acc->u8(), m2->u8(), t.n, acc->u8()),
          "bg_bitmap_or");
    }
  }
  if (!acc) throw StageError(BG_ERR_INVALID, "filter: empty 'any'");
  return acc;
}

static Table filter_materialize(const Table& t, DBufPtr mask) {
  DBufPtr idx = dalloc_elems(t.n, 4);
  int64_t m = 0;
  chk(bg_mask_to_indices(mask->u8(), t.n, (uint32_t*)idx->p, &m),
      "bg_mask_to_indices");
  return gather_table(t, (const uint32_t*)idx->p, m);
}

// ---------------------------------------------------------------------------
// operators
// ---------------------------------------------------------------------------

struct Metrics {
  int64_t repart_time_ns = 0;
  int64_t write_time_ns = 0;
  int64_t scan_time_ns = 0;
  int64_t exec_time_ns = 0;
  int64_t output_rows = 0;
  double kernel_ms = 0.0;
};

static Table exec_plan(const Value& node, Metrics& m);

static Table exec_project(const Value& node, Metrics& m) {
  Table in = exec_plan(node.at("input"), m);
  Table out;
  out.n = in.n;
  std::vector<const Value*> exprs;
  for (auto& ex : node.get_arr("exprs")) exprs.push_back(&ex->at("expr"));
  std::vector<Col> cols;
  eval_exprs_fused(in, exprs, &cols);
  size_t i = 0;
  for (auto& ex : node.get_arr("exprs")) {
    out.names.push_back(ex->get_str("as"));
    out.cols.push_back(std::move(cols[i++]));
  }
  return out;
}

// The join types of the plan grammar: the one list that bg_stage_validate
// and execution both read.
struct JoinKind {
  const char* name;
  int32_t type;
  bool build_rows_only;  // emits build rows only, each at most once
  bool probe_null_idx;   // unmatched probe rows carry BG_JOIN_NULL_IDX
  bool build_tail;       // unmatched build rows follow the last chunk
};
static const JoinKind JOIN_KINDS[] = {
    {"inner", BG_JOIN_INNER, false, false, false},
    {"semi", BG_JOIN_SEMI, false, false, false},
    {"anti", BG_JOIN_ANTI, false, false, false},
    {"left", BG_JOIN_OUTER_PROBE, false, true, false},  // probe preserved
    // build preserved (DataFusion LeftSemi / LeftAnti / Left / Full)
    {"semi_build", BG_JOIN_SEMI_BUILD, true, false, false},
    {"anti_build", BG_JOIN_ANTI_BUILD, true, false, false},
    {"outer_build", BG_JOIN_OUTER_BUILD, false, false, true},
    {"full", BG_JOIN_OUTER_FULL, false, true, true},
};

// Both join nodes (hash_join, nested_loop_join) read the list; a refusal
// names the node it came from.
static const JoinKind& join_kind(const Value& node) {
  const std::string jt = node.get_str_or("join_type", "inner");
  for (auto& k : JOIN_KINDS)
    if (jt == k.name) return k;
  throw StageError(BG_ERR_UNSUPPORTED,
                   node.get_str("op") + ": join_type " + jt);
}

// nested_loop_join is the keyless join: keys on it are a mistake, not a hint
static void refuse_join_keys(const Value& node) {
  for (const char* key : {"build_keys", "probe_keys"})
    if (node.has(key))
      throw StageError(BG_ERR_INVALID,
                       std::string("nested_loop_join: '") + key +
                           "' given; a join with keys is a hash_join");
}

static void require_build_side(const std::string& op, const std::string& jt,
                               const Value& o) {
  if (o.get_str("side") != "build")
    throw StageError(BG_ERR_INVALID,
                     op + ": " + jt + " emits build rows only; output '" +
                         o.get_str("col") + "' is not side 'build'");
}

struct JoinOut {
  bool build;  // taken from the build side (else the probe side)
  std::string col, as;
};

// One entry of a join node's "output" list, checked against the join type;
// op names the node in the message.
static JoinOut join_output(const std::string& op, const JoinKind& k,
                           const Value& o) {
  if (k.build_rows_only) require_build_side(op, k.name, o);
  const bool build = o.get_str("side") == "build";
  const std::string col = o.get_str("col");
  return {build, col, o.get_str_or("as", col)};
}

// The library handle of one join.  With build keys it is a hash table: the
// single-INT64-key inner join without a residual filter has a specialised
// one, every other keyed shape goes through the general one.  Without keys
// (nested_loop_join) it is the nested-loop handle, which holds no table and
// takes no probe keys.  The probe calls take the chunk's filter terms; none
// means no filter.
using JoinTerms = std::vector<bg_join_filter_term>;
struct JoinHandle {
  void* h = nullptr;
  const bool nl;  // no keys: bg_nljoin_*
  const bool fast;
  const int32_t type;
  JoinHandle(const JoinHandle&) = delete;
  JoinHandle& operator=(const JoinHandle&) = delete;
  // bk empty: a nested-loop join
  JoinHandle(const std::vector<bg_column>& bk, int64_t n, int32_t join_type,
             bool filtered)
      : nl(bk.empty()),
        fast(bk.size() == 1 && bk[0].dtype == BG_DT_INT64 &&
             join_type == BG_JOIN_INNER && !filtered),
        type(join_type) {
    if (nl) chk(bg_nljoin_open(n, &h), "bg_nljoin_open");
    else if (fast) chk(bg_hashjoin_build(&bk[0], n, &h), "bg_hashjoin_build");
    else
      chk(bg_hashjoin_build2(bk.data(), (int32_t)bk.size(), n, &h),
          "bg_hashjoin_build2");
  }
  ~JoinHandle() {
    if (!h) return;
    (void)(nl ? bg_nljoin_free(h)
              : fast ? bg_hashjoin_free(h) : bg_hashjoin_free2(h));
  }
  int64_t count(const std::vector<bg_column>& pk, int64_t len,
                const JoinTerms& ft) {
    int64_t matches = 0;
    if (nl)
      chk(bg_nljoin_count(h, len, type, ft.data(), (int32_t)ft.size(),
                          &matches),
          "bg_nljoin_count");
    else if (fast)
      chk(bg_hashjoin_probe_count(h, &pk[0], len, &matches),
          "bg_hashjoin_probe_count");
    else if (ft.empty())
      chk(bg_hashjoin_probe_count2(h, pk.data(), (int32_t)pk.size(), len,
                                   type, &matches),
          "bg_hashjoin_probe_count2");
    else
      chk(bg_hashjoin_probe_count2_filtered(h, pk.data(), (int32_t)pk.size(),
                                            len, type, ft.data(),
                                            (int32_t)ft.size(), &matches),
          "bg_hashjoin_probe_count2_filtered");
    return matches;
  }
  void fill(const std::vector<bg_column>& pk, int64_t len,
            const JoinTerms& ft, uint32_t* pidx, uint32_t* bidx) {
    if (nl)
      chk(bg_nljoin_fill(h, len, type, ft.data(), (int32_t)ft.size(), pidx,
                         bidx),
          "bg_nljoin_fill");
    else if (fast)
      chk(bg_hashjoin_probe_fill(h, &pk[0], len, pidx, bidx),
          "bg_hashjoin_probe_fill");
    else if (ft.empty())
      chk(bg_hashjoin_probe_fill2(h, pk.data(), (int32_t)pk.size(), len, type,
                                  pidx, bidx),
          "bg_hashjoin_probe_fill2");
    else
      chk(bg_hashjoin_probe_fill2_filtered(h, pk.data(), (int32_t)pk.size(),
                                           len, type, ft.data(),
                                           (int32_t)ft.size(), pidx, bidx),
          "bg_hashjoin_probe_fill2_filtered");
  }
  // the build-rows calls exist for the general table and the nested-loop
  // handle only; the types that use them never take the fast path
  void mark(const std::vector<bg_column>& pk, int64_t len,
            const JoinTerms& ft) {
    if (nl)
      chk(bg_nljoin_mark(h, len, ft.data(), (int32_t)ft.size()),
          "bg_nljoin_mark");
    else if (ft.empty())
      chk(bg_hashjoin_probe_mark2(h, pk.data(), (int32_t)pk.size(), len),
          "bg_hashjoin_probe_mark2");
    else
      chk(bg_hashjoin_probe_mark2_filtered(h, pk.data(), (int32_t)pk.size(),
                                           len, ft.data(), (int32_t)ft.size()),
          "bg_hashjoin_probe_mark2_filtered");
  }
  // build rows some probe row matched (matched=1) or none did (0), in
  // ascending build order
  int64_t build_rows(int matched, uint32_t* idx) {
    int64_t rows = 0;
    if (nl)
      chk(bg_nljoin_build_rows(h, matched, &rows, idx),
          "bg_nljoin_build_rows");
    else
      chk(bg_hashjoin_build_rows2(h, matched, &rows, idx),
          "bg_hashjoin_build_rows2");
    return rows;
  }
};

// The two evaluated sides of a join with its key and output columns.
struct JoinSides {
  Table build, probe;
  std::vector<int> pk_ids;  // probe key columns
  std::vector<JoinOut> outs;

  // probe key columns of the slice [start, start+len); the Cols own nothing
  // new but must outlive the bg_column views taken of them
  void slice_probe_keys(int64_t start, int64_t len, std::vector<Col>& sliced,
                        std::vector<bg_column>& views) const {
    for (int id : pk_ids) {
      sliced.push_back(slice_col(probe.cols[(size_t)id], start, len));
      views.push_back(to_bg(sliced.back(), len));
    }
  }
  Col gather_build(const std::string& col, const DBufPtr& idx,
                   int64_t rows) const {
    return gather_col(build.col(col), build.n, (const uint32_t*)idx->p, rows);
  }

  // The residual filter ("filter": {"any": [group...]}), evaluated as far
  // as one side alone allows: each group's "build" and "probe" predicates
  // become one mask over that side's whole table, its "cross" terms stay
  // column pairs for the probe kernels.  No groups = no filter.
  struct FilterGroup {
    DBufPtr build_mask, probe_mask;
    struct Cross { int bcol, pcol; int32_t cmp; };
    std::vector<Cross> cross;
  };
  std::vector<FilterGroup> filter;

  void eval_filter(const Value& node) {
    if (!node.has("filter")) return;
    // AND-fold a group's predicate list over one side, like a filter node
    auto side_mask = [](const Table& t, const Value& grp, const char* key) {
      for (auto& kv : grp.obj) {
        if (kv.first != key || kv.second->arr.empty()) continue;
        bgjson::Value fake;
        fake.kind = Value::OBJ;
        fake.obj.emplace_back("predicates", kv.second);
        return eval_filter_mask(t, fake);
      }
      return DBufPtr();
    };
    for (auto& grp : node.at("filter").get_arr("any")) {
      FilterGroup g;
      g.build_mask = side_mask(build, *grp, "build");
      g.probe_mask = side_mask(probe, *grp, "probe");
      if (grp->has("cross"))
        for (auto& x : grp->get_arr("cross"))
          g.cross.push_back({build.idx(x->get_str("build")),
                             probe.idx(x->get_str("probe")),
                             cmp_cols_code(x->get_str("cmp"))});
      filter.push_back(std::move(g));
    }
  }

  // the filter's terms for the probe slice [start, start+len): start is a
  // 64-row multiple, so the slice's probe mask starts at a byte of the
  // whole table's and the cross columns slice like the keys
  JoinTerms filter_terms(int64_t start, int64_t len) const {
    JoinTerms terms;
    for (size_t gi = 0; gi < filter.size(); ++gi) {
      const FilterGroup& g = filter[gi];
      bg_join_filter_term t{};
      t.group = (int32_t)gi;
      if (g.build_mask) {
        t.kind = BG_JF_BUILD_MASK;
        t.d_build = g.build_mask->p;
        terms.push_back(t);
      }
      if (g.probe_mask) {
        t = bg_join_filter_term{};
        t.group = (int32_t)gi;
        t.kind = BG_JF_PROBE_MASK;
        t.d_probe = g.probe_mask->u8() + start / 8;
        terms.push_back(t);
      }
      for (auto& x : g.cross) {
        const Col& bc = build.cols[(size_t)x.bcol];
        // the slice owns nothing: its pointers stay good while probe lives
        const Col pc = slice_col(probe.cols[(size_t)x.pcol], start, len);
        t = bg_join_filter_term{};
        t.group = (int32_t)gi;
        t.kind = BG_JF_CROSS;
        t.dtype = bc.dtype;
        t.cmp = x.cmp;
        t.d_build = bc.dptr();
        t.d_build_validity = bc.vptr();
        t.d_probe = pc.dptr();
        t.d_probe_validity = pc.vptr();
        terms.push_back(t);
      }
    }
    return terms;
  }
};

// semi_build / anti_build: only the visited bitmap matters: mark per probe
// chunk (no pair buffers), then list the build rows once, in ascending
// build order
static Table join_build_rows_only(JoinHandle& jh, const JoinSides& s,
                                  int64_t chunk) {
  for (int64_t start = 0; start < s.probe.n; start += chunk) {
    const int64_t len = std::min(s.probe.n - start, chunk);
    std::vector<bg_column> pk;
    std::vector<Col> pk_sliced;
    s.slice_probe_keys(start, len, pk_sliced, pk);
    jh.mark(pk, len, s.filter_terms(start, len));
  }
  DBufPtr idx = dalloc_elems(s.build.n, 4);
  Table out;
  out.n = jh.build_rows(jh.type == BG_JOIN_SEMI_BUILD ? 1 : 0,
                        (uint32_t*)idx->p);
  for (auto& o : s.outs) {
    out.names.push_back(o.as);
    out.cols.push_back(s.gather_build(o.col, idx, out.n));
  }
  return out;
}

// One probe slice [start, start+len): count, fill, split the NULL-index
// sentinels off, gather one piece per output.  Returns the pair count.
static int64_t join_probe_chunk(JoinHandle& jh, const JoinKind& k,
                                const JoinSides& s, int64_t start, int64_t len,
                                std::vector<std::vector<Col>>& pieces) {
  std::vector<bg_column> pk;
  std::vector<Col> pk_sliced;
  s.slice_probe_keys(start, len, pk_sliced, pk);
  const JoinTerms ft = s.filter_terms(start, len);
  const int64_t matches = jh.count(pk, len, ft);
  DBufPtr pidx = dalloc_elems(matches, 4);
  DBufPtr bidx = dalloc_elems(matches, 4);
  jh.fill(pk, len, ft, (uint32_t*)pidx->p, (uint32_t*)bidx->p);

  DBufPtr bidx_clamped, outer_valid;
  if (k.probe_null_idx) {
    bidx_clamped = dalloc_elems(matches, 4);
    outer_valid = alloc_bitmap(matches, 0xFF);
    chk(bg_idx_sentinel((const uint32_t*)bidx->p, matches,
                        (uint32_t*)bidx_clamped->p, outer_valid->u8()),
        "bg_idx_sentinel");
  }

  for (size_t oi = 0; oi < s.outs.size(); ++oi) {
    const JoinOut& o = s.outs[oi];
    const bool outer_build = o.build && k.probe_null_idx;
    Col c;
    if (outer_build && s.build.n == 0) {
      // left or full join over an empty build side: every pair is an
      // unmatched probe row, and there is no build row 0 to gather a filler
      // from
      c = null_col(s.build.col(o.col), matches);
    } else if (o.build) {
      c = s.gather_build(o.col, outer_build ? bidx_clamped : bidx, matches);
      if (outer_build && c.validity) {
        DBufPtr comb = alloc_bitmap(matches);
        chk(bg_bitmap_and(c.validity->u8(), outer_valid->u8(), matches,
                          comb->u8()),
            "bg_bitmap_and");
        c.validity = comb;
      } else if (outer_build) {
        c.validity = outer_valid;
      }
    } else {
      // probe indices are chunk-relative: gather from the SLICE
      Col ps = slice_col(s.probe.col(o.col), start, len);
      c = gather_col(ps, len, (const uint32_t*)pidx->p, matches);
    }
    pieces[oi].push_back(std::move(c));
  }
  return matches;
}

// outer_build / full: one tail piece after the last chunk: the build rows
// no probe row matched, with NULL probe-side columns.  Returns its rows.
static int64_t join_unmatched_build_tail(JoinHandle& jh, const JoinSides& s,
                                         std::vector<std::vector<Col>>& pieces) {
  DBufPtr idx = dalloc_elems(s.build.n, 4);
  const int64_t rows = jh.build_rows(0, (uint32_t*)idx->p);
  for (size_t oi = 0; oi < s.outs.size(); ++oi) {
    const JoinOut& o = s.outs[oi];
    pieces[oi].push_back(o.build ? s.gather_build(o.col, idx, rows)
                                 : null_col(s.probe.col(o.col), rows));
  }
  return rows;
}

static Table exec_join(const Value& node, Metrics& m) {
  JoinSides s;
  s.build = exec_plan(node.at("build"), m);
  s.probe = exec_plan(node.at("probe"), m);
  const std::string op = node.get_str("op");
  // nested_loop_join has no keys: bk stays empty, which is what tells the
  // handle below to be the nested-loop one
  static const std::vector<bgjson::ValuePtr> no_keys;
  const bool keyed = op == "hash_join";
  if (!keyed) refuse_join_keys(node);
  auto& bkeys = keyed ? node.get_arr("build_keys") : no_keys;
  auto& pkeys = keyed ? node.get_arr("probe_keys") : no_keys;
  if (keyed &&
      (bkeys.size() != pkeys.size() || bkeys.empty() || bkeys.size() > 4))
    throw StageError(BG_ERR_INVALID, "hash_join: 1-4 matching key columns");
  const JoinKind& k = join_kind(node);

  std::vector<bg_column> bk;
  for (size_t i = 0; i < bkeys.size(); ++i) {
    bk.push_back(to_bg(s.build.col(bkeys[i]->s), s.build.n));
    s.pk_ids.push_back(s.probe.idx(pkeys[i]->s));
    if (bk[i].dtype != s.probe.cols[(size_t)s.pk_ids[i]].dtype)
      throw StageError(BG_ERR_INVALID, "hash_join: key dtype mismatch");
  }
  for (auto& o : node.get_arr("output"))
    s.outs.push_back(join_output(op, k, *o));
  s.eval_filter(node);
  JoinHandle jh(bk, s.build.n, k.type, !s.filter.empty());

  // Memory-pressure bound (the spill analogue of sort_shuffle/writer.rs:
  // 650-686 for join temporaries): probe in slices of probe_chunk_rows
  // so the pair buffers + gathered outputs stay bounded regardless of the
  // probe side's size; chunk outputs are concatenated afterwards.  0 =
  // unchunked.  Slices start at 64-row multiples (validity byte-aligned).
  int64_t chunk = node.get_int_or("probe_chunk_rows", 0);
  if (chunk <= 0 || chunk >= s.probe.n) chunk = s.probe.n > 0 ? s.probe.n : 1;
  chunk = (chunk + 63) & ~63LL;
  if (k.build_rows_only) return join_build_rows_only(jh, s, chunk);

  std::vector<std::vector<Col>> pieces(s.outs.size());
  std::vector<int64_t> piece_lens;
  // an empty probe side still runs one (empty) slice
  for (int64_t start = 0; start == 0 || start < s.probe.n; start += chunk)
    piece_lens.push_back(join_probe_chunk(
        jh, k, s, start, std::min(s.probe.n - start, chunk), pieces));
  if (k.build_tail)
    piece_lens.push_back(join_unmatched_build_tail(jh, s, pieces));

  Table out;
  for (int64_t len : piece_lens) out.n += len;
  for (size_t oi = 0; oi < s.outs.size(); ++oi) {
    out.names.push_back(s.outs[oi].as);
    if (pieces[oi].size() == 1)
      out.cols.push_back(std::move(pieces[oi][0]));
    else
      out.cols.push_back(concat_cols(pieces[oi], piece_lens));
  }
  return out;
}
// q6-shape fusion: aggregate(no groups, sum(mul(dec,dec)) [+count]) over
// filter(ge_lt date32, between dec128, lt dec128) over scan — the exact
// Filter+Partial-Aggregate stage of approved/q6.txt, one fused kernel.
static bool try_q6_fusion(const Value& agg_node, Metrics& m, Table* out) {
  if (!agg_node.at("group_by").arr.empty()) return false;
  auto& aggs = agg_node.get_arr("aggs");
  const Value* sum_agg = nullptr;
  const Value* cnt_agg = nullptr;
  for (auto& a : aggs) {
    const std::string fn = a->get_str("fn");
    if (fn == "sum" && !sum_agg) sum_agg = a.get();
    else if (fn == "count" && !cnt_agg) cnt_agg = a.get();
    else return false;
  }
  if (!sum_agg || !sum_agg->has("expr")) return false;
  const Value& se = sum_agg->at("expr");
  if (!se.has("mul")) return false;
  auto& mops = se.get_arr("mul");
  if (!mops[0]->has("col") || !mops[1]->has("col")) return false;

  const Value& fin = agg_node.at("input");
  if (!fin.has("op") || fin.get_str("op") != "filter") return false;
  const Value& scan_node = fin.at("input");
  if (!scan_node.has("op") || scan_node.get_str("op") != "scan") return false;
  auto& preds = fin.get_arr("predicates");
  if (preds.size() != 3) return false;

  Table t = scan(scan_node);
  const Value *p_date = nullptr, *p_disc = nullptr, *p_qty = nullptr;
  for (auto& p : preds) {
    const int32_t dt = t.col(p->get_str("col")).dtype;
    const std::string cmp = p->get_str("cmp");
    if (cmp == "ge_lt" && dt == BG_DT_DATE32) p_date = p.get();
    else if (cmp == "between" && dt == BG_DT_DECIMAL128) p_disc = p.get();
    else if (cmp == "lt" && dt == BG_DT_DECIMAL128) p_qty = p.get();
  }
  if (!p_date || !p_disc || !p_qty) return false;
  // the sum multiplies discount by the price column
  const std::string disc_name = p_disc->get_str("col");
  std::string price_name;
  if (mops[0]->get_str("col") == disc_name) price_name = mops[1]->get_str("col");
  else if (mops[1]->get_str("col") == disc_name)
    price_name = mops[0]->get_str("col");
  else return false;

  bg_column sd = to_bg(t.col(p_date->get_str("col")), t.n);
  bg_column cd = to_bg(t.col(disc_name), t.n);
  bg_column cq = to_bg(t.col(p_qty->get_str("col")), t.n);
  bg_column cp = to_bg(t.col(price_name), t.n);
  int64_t dlo_lo, dlo_hi, dhi_lo, dhi_hi, qlo, qhi_unused;
  parse_i128(p_date->at("lo"), &dlo_lo, &dlo_hi);
  parse_i128(p_date->at("hi"), &dhi_lo, &dhi_hi);
  int64_t disc_lo_lo, disc_lo_hi, disc_hi_lo, disc_hi_hi;
  parse_i128(p_disc->at("lo"), &disc_lo_lo, &disc_lo_hi);
  parse_i128(p_disc->at("hi"), &disc_hi_lo, &disc_hi_hi);
  parse_i128(p_qty->at("hi"), &qlo, &qhi_unused);

  uint64_t sum_lo = 0;
  int64_t sum_hi = 0, count = 0;
  chk(bg_q6_agg(&sd, &cd, &cq, &cp, (int32_t)dlo_lo, (int32_t)dhi_lo,
                disc_lo_lo, disc_hi_lo, qlo, &sum_lo, &sum_hi, &count),
      "bg_q6_agg");
  m.kernel_ms += bg_last_kernel_ms();

  // one-row output table: [sum dec128, count i64] in agg order
  Table res;
  res.n = 1;
  for (auto& a : aggs) {
    Col c = make_col({BG_DT_INT64, 0, 0});
    if (a->get_str("fn") == "sum") {
      // scale of the product = s1 + s2 from the scan schema
      c = make_col({BG_DT_DECIMAL128, 38,
                    t.col(disc_name).scale + t.col(price_name).scale});
      uint64_t host[2] = {sum_lo, (uint64_t)sum_hi};
      c.data = upload(host, 16);
    } else {
      c.data = upload(&count, 8);
    }
    res.names.push_back(a->get_str("as"));
    res.cols.push_back(std::move(c));
  }
  *out = res;
  return true;
}

// ---- aggregate output schema: the one derivation that bg_stage_validate
// and execution both read ----
struct AggField {
  std::string name;
  DtSpec dt;
};
static const DtSpec DT_I64{BG_DT_INT64, 0, 0};

static void check_agg_fn(const std::string& fn) {
  if (fn != "sum" && fn != "min" && fn != "max" && fn != "count" &&
      fn != "avg")
    throw StageError(BG_ERR_INVALID, "aggregate fn " + fn);
}

// The partial-side columns of one aggregate, value first: what partial
// mode emits and final mode reads.  A count is its own non-null count.
static std::vector<std::string> agg_partial_names(const std::string& fn,
                                                  const std::string& as) {
  if (fn == "count") return {as};
  return {fn == "avg" ? as + "$s" : as, as + "$n"};
}

// The output fields of one aggregate, in order.  `in` is the dtype of its
// input: the evaluated expression (single/partial; unused by count) or the
// partial value column (final).
static std::vector<AggField> agg_output_fields(const std::string& fn,
                                               const std::string& mode,
                                               const std::string& as,
                                               DtSpec in) {
  check_agg_fn(fn);
  if (fn == "count") return {{as, DT_I64}};
  // a Decimal128 sum accumulates at full width
  if (fn == "sum" && in.dt == BG_DT_DECIMAL128) in.precision = 38;
  if (mode == "partial") {
    auto names = agg_partial_names(fn, as);
    return {{names[0], in}, {names[1], DT_I64}};
  }
  // DataFusion decimal AVG: out scale = in scale + 4, precision + 4
  if (fn == "avg" && in.dt == BG_DT_FLOAT64) in = {BG_DT_FLOAT64, 0, 0};
  else if (fn == "avg")
    in = {BG_DT_DECIMAL128, std::min(in.precision + 4, 38), in.scale + 4};
  return {{as, in}};
}

struct AggSpec {
  std::string fn, as;
  int agg_slot = -1;  // index into the kernel's agg list (-1: count(*))
  int nn_slot = -1;   // extra slot whose SUM carries the merged nn (final)
  int32_t op = 0;     // kernel op for the value slot
  DtSpec in{0, 0, 0};  // input dtype, as agg_output_fields takes it
};

// The kernel's aggregate list: one slot per evaluated input column.
struct AggSlots {
  std::vector<AggSpec> specs;
  std::vector<Col> in;
  std::vector<int32_t> ops;
  int add(const Col& c, int32_t op) {
    in.push_back(c);
    ops.push_back(op);
    return (int)in.size() - 1;
  }
};

// The kernel op of an aggregate over an input dtype: the one answer that
// bg_stage_validate and execution both read.
static int32_t agg_op_for(const std::string& fn, int32_t dt) {
  if (fn == "min" || fn == "max") {
    const bool mn = fn == "min";
    switch (dt) {
      case BG_DT_FLOAT64: return mn ? BG_AGG_OP_MIN_F64 : BG_AGG_OP_MAX_F64;
      case BG_DT_INT64: return mn ? BG_AGG_OP_MIN_I64 : BG_AGG_OP_MAX_I64;
      case BG_DT_INT32:
      case BG_DT_DATE32: return mn ? BG_AGG_OP_MIN_I32 : BG_AGG_OP_MAX_I32;
      // no fixed-width atomic: the accumulator keeps the winning row
      case BG_DT_DECIMAL128:
      case BG_DT_UTF8: return mn ? BG_AGG_OP_MIN_ROW : BG_AGG_OP_MAX_ROW;
      default:  // a dictionary code has no value order
        throw StageError(BG_ERR_UNSUPPORTED,
                         std::string("min/max over ") + dtype_name(dt));
    }
  }
  switch (dt) {  // sum, avg and count(expr) all run a sum
    case BG_DT_DECIMAL128: return BG_AGG_OP_SUM_DEC128;
    case BG_DT_INT64: return BG_AGG_OP_SUM_I64;
    case BG_DT_FLOAT64: return BG_AGG_OP_SUM_F64;
    default:
      throw StageError(BG_ERR_UNSUPPORTED, "sum over unsupported dtype");
  }
}

// Specs and kernel input columns of a hash_aggregate node over its input.
static AggSlots plan_agg_slots(const Value& node, const Table& in,
                               bool is_final) {
  auto& aggs = node.get_arr("aggs");
  auto is_count_star = [](const Value& a) {
    return a.get_str("fn") == "count" && !a.has("expr");
  };
  // single/partial: the inputs are expressions — arithmetic fuses into one
  // projection pass (q1-class chains cost ~77 GB of intermediates otherwise)
  std::vector<const Value*> pre_exprs;
  for (auto& a : aggs)
    if (!is_final && !is_count_star(*a)) pre_exprs.push_back(&a->at("expr"));
  std::vector<Col> pre_cols;
  if (!pre_exprs.empty()) eval_exprs_fused(in, pre_exprs, &pre_cols);

  AggSlots slots;
  size_t pre = 0;
  for (auto& a : aggs) {
    AggSpec s;
    s.fn = a->get_str("fn");
    s.as = a->get_str("as");
    if (is_final) {
      // final: the inputs are the partial columns; a merged count is the
      // sum of the counts, as is the "$n" companion of every other fn
      auto names = agg_partial_names(s.fn, s.as);
      const Col& cv = in.col(names[0]);
      if (s.fn == "count") {
        s.op = BG_AGG_OP_SUM_I64;
        s.agg_slot = slots.add(cv, s.op);
      } else {
        const Col& cn = in.col(names[1]);
        s.in = cv.spec();
        s.op = agg_op_for(s.fn, cv.dtype);
        s.agg_slot = slots.add(cv, s.op);
        s.nn_slot = slots.add(cn, BG_AGG_OP_SUM_I64);
      }
    } else if (!is_count_star(*a)) {  // COUNT(*): the kernel's group counts
      const Col& v = pre_cols[pre++];
      s.in = v.spec();
      s.op = agg_op_for(s.fn, v.dtype);
      s.agg_slot = slots.add(v, s.op);
    }
    slots.specs.push_back(s);
  }
  return slots;
}

// One finished bg_hashagg2 run: ng groups, interleaved per-slot records.
struct HashAggRun {
  DBufPtr first, acc, counts, nncnt;
  int64_t ng = 0;
  int32_t naggs = 0;
  int64_t acc_stride() const { return (int64_t)naggs * 16; }
  int64_t nn_stride() const { return (int64_t)naggs * 8; }
  const uint8_t* acc_at(int slot) const {
    return acc->u8() + (int64_t)slot * 16;
  }
  const int64_t* nn_at(int slot) const {
    return (const int64_t*)(nncnt->u8() + (int64_t)slot * 8);
  }
};

// run the kernel (auto-grow on table-full, like gpu.py)
static HashAggRun run_hashagg_growing(const Value& node, const Table& in,
                                      const std::vector<Col>& keys,
                                      const AggSlots& slots,
                                      const DBufPtr& mask) {
  std::vector<bg_column> kcols, acols;
  for (auto& c : keys) kcols.push_back(to_bg(c, in.n));
  for (auto& c : slots.in) acols.push_back(to_bg(c, in.n));
  if (acols.empty()) acols.push_back(bg_column{});
  std::vector<int32_t> aops = slots.ops;
  if (aops.empty()) aops.push_back(0);

  HashAggRun r;
  r.naggs = (int32_t)slots.in.size();
  int64_t cap = node.get_int_or("estimated_groups", 1 << 16);
  if (cap < 64) cap = 64;
  for (int attempt = 0; attempt < 10; ++attempt) {
    r.first = dalloc((uint64_t)cap * 4);
    r.acc = dalloc_elems(r.naggs, (int64_t)cap * 16);
    r.counts = dalloc((uint64_t)cap * 8);
    r.nncnt = dalloc_elems(r.naggs, (int64_t)cap * 8);
    int rc = bg_hashagg2(kcols.data(), (int32_t)kcols.size(), acols.data(),
                         aops.data(), r.naggs, mask ? mask->u8() : nullptr,
                         in.n, cap, (uint32_t*)r.first->p, r.acc->u8(),
                         (int64_t*)r.counts->p, (int64_t*)r.nncnt->p, &r.ng);
    if (rc == BG_OK) break;
    std::string err = bg_last_error();
    if (err.find("table full") == std::string::npos || cap >= in.n)
      chk(rc, "bg_hashagg2");
    cap = cap * 8 < in.n ? cap * 8 : (in.n > 64 ? in.n : 64);
  }
  return r;
}

// where a group's non-null count lives: the kernel's nn records, or in
// final mode the merged "$n" sum (a SUM_I64 acc record's low limb)
struct NnSrc {
  const int64_t* p;
  int64_t stride;
};
static NnSrc nn_source(const HashAggRun& r, const AggSpec& s, bool is_final) {
  if (is_final) return {(const int64_t*)r.acc_at(s.nn_slot), r.acc_stride()};
  return {r.nn_at(s.agg_slot), r.nn_stride()};
}

// the non-null count of a slot as an INT64 column (never NULL)
static Col nn_column(const HashAggRun& r, int slot) {
  Col cn = make_col(DT_I64);
  cn.data = dalloc_elems(r.ng, 8);
  chk(bg_copy_i64_strided(r.nn_at(slot), r.nn_stride(), r.ng, cn.data->p),
      "bg_copy_i64_strided");
  return cn;
}

// the decoded value of a spec's slot; with an nn source, NULL where every
// input of the group was NULL.  `in` is the slot's input column: a ROW op
// kept the winning row, so its value is a take of `in` by those rows, NULL
// where the group had no winner.
static Col value_column(const HashAggRun& r, const AggSpec& s,
                        const DtSpec& dt, const NnSrc* nn, const Col& in,
                        int64_t n_in) {
  if (s.op == BG_AGG_OP_MIN_ROW || s.op == BG_AGG_OP_MAX_ROW) {
    DBufPtr rows = dalloc_elems(r.ng, 4);
    DBufPtr valid = alloc_bitmap(r.ng, 0);
    chk(bg_agg_winner_rows(r.acc_at(s.agg_slot), r.acc_stride(), r.ng,
                           (uint32_t*)rows->p, valid->u8()),
        "bg_agg_winner_rows");
    Col cv = gather_col(in, n_in, (const uint32_t*)rows->p, r.ng);
    cv.precision = dt.precision;
    cv.scale = dt.scale;
    cv.validity = valid;
    return cv;
  }
  Col cv = make_col(dt);
  cv.data = dalloc_elems(r.ng, dt_size(dt.dt));
  if (nn) cv.validity = alloc_bitmap(r.ng, 0xFF);
  chk(bg_agg_materialize(r.acc_at(s.agg_slot), r.acc_stride(), s.op, r.ng,
                         cv.data->p, nn ? nn->p : nullptr,
                         nn ? nn->stride : 0,
                         nn ? cv.validity->u8() : nullptr),
      "bg_agg_materialize");
  return cv;
}

static Col avg_column(const HashAggRun& r, const AggSpec& s, const DtSpec& dt,
                      const NnSrc& nn) {
  Col cv = make_col(dt);
  cv.data = dalloc_elems(r.ng, dt_size(dt.dt));
  cv.validity = alloc_bitmap(r.ng, 0xFF);
  chk(bg_avg_finalize(r.acc_at(s.agg_slot), r.acc_stride(),
                      dt.dt == BG_DT_FLOAT64 ? 1 : 0, nn.p, nn.stride, 4, r.ng,
                      cv.data->p, cv.validity->u8()),
      "bg_avg_finalize");
  return cv;
}

// Append every aggregate's output columns; names and dtypes come from
// agg_output_fields.
static void materialize_aggs(const AggSlots& slots, int64_t n_in,
                             const std::string& mode, const HashAggRun& r,
                             Table& out) {
  const bool is_final = mode == "final", is_partial = mode == "partial";
  for (auto& s : slots.specs) {
    const auto fields = agg_output_fields(s.fn, mode, s.as, s.in);
    const DtSpec& dt = fields[0].dt;
    std::vector<Col> cols;
    // the slot's input column (COUNT(*) has none and never reads it)
    static const Col no_input;
    const Col& vin = s.agg_slot < 0 ? no_input : slots.in[(size_t)s.agg_slot];
    if (s.agg_slot < 0) {
      // COUNT(*) = the group counts: dense i64[ng] already, never NULL
      cols.push_back(make_col(dt));
      cols[0].data = r.counts;
    } else if (s.fn == "count") {
      // final: the merged count is the SUM_I64 acc itself
      cols.push_back(is_final ? value_column(r, s, dt, nullptr, vin, n_in)
                              : nn_column(r, s.agg_slot));
    } else if (s.fn == "avg" && !is_partial) {
      cols.push_back(avg_column(r, s, dt, nn_source(r, s, is_final)));
    } else {
      // sum/min/max, and the "$s" sum of a partial avg (never NULL: its
      // "$n" companion says when it is empty)
      const NnSrc nn = nn_source(r, s, is_final);
      cols.push_back(
          value_column(r, s, dt, s.fn == "avg" ? nullptr : &nn, vin, n_in));
      if (is_partial) cols.push_back(nn_column(r, s.agg_slot));
    }
    for (size_t i = 0; i < cols.size(); ++i) {
      out.names.push_back(fields[i].name);
      out.cols.push_back(std::move(cols[i]));
    }
  }
}

static Table exec_aggregate(const Value& node, Metrics& m) {
  {
    Table fused;
    if (try_q6_fusion(node, m, &fused)) return fused;
  }
  const std::string mode = node.get_str_or("mode", "single");

  // input (+ fused filter mask when the child is a filter)
  DBufPtr mask;
  Table in;
  const Value& child = node.at("input");
  if (child.get_str("op") == "filter") {
    in = exec_plan(child.at("input"), m);
    mask = eval_filter_node(in, child);
  } else {
    in = exec_plan(child, m);
  }

  // group keys; none = one group under a constant key
  auto& group_by = node.get_arr("group_by");
  std::vector<Col> keys;
  for (auto& k : group_by) keys.push_back(in.col(k->s));
  if (keys.empty()) {
    keys.push_back(make_col(DT_I64));
    keys[0].data = dalloc_elems(in.n, 8);
    chk(bg_memset(keys[0].data->p, 0, keys[0].data->bytes), "bg_memset");
  }

  AggSlots slots = plan_agg_slots(node, in, mode == "final");
  HashAggRun r = run_hashagg_growing(node, in, keys, slots, mask);

  Table out;
  out.n = r.ng;
  // group keys (gathered by first_row; NULL keys keep their validity)
  for (size_t i = 0; i < group_by.size(); ++i) {
    out.names.push_back(group_by[i]->s);
    out.cols.push_back(
        gather_col(keys[i], in.n, (const uint32_t*)r.first->p, r.ng));
  }
  materialize_aggs(slots, in.n, mode, r, out);
  m.output_rows = r.ng;
  return out;
}
static Table exec_sort(const Value& node, Metrics& m) {
  Table in = exec_plan(node.at("input"), m);
  auto& keys = node.get_arr("keys");
  std::vector<bg_column> kcols;
  std::vector<int32_t> desc, nf;
  for (auto& k : keys) {
    kcols.push_back(to_bg(in.col(k->get_str("col")), in.n));
    bool d = k->get_bool_or("desc", false);
    desc.push_back(d ? 1 : 0);
    // SQL default: ASC => NULLS LAST, DESC => NULLS FIRST
    nf.push_back(k->get_bool_or("nulls_first", d) ? 1 : 0);
  }
  DBufPtr perm = dalloc_elems(in.n, 4);
  chk(bg_sort_rows2(kcols.data(), desc.data(), nf.data(),
                    (int32_t)kcols.size(), in.n, (uint32_t*)perm->p),
      "bg_sort_rows2");
  int64_t limit = node.get_int_or("limit", -1);
  int64_t mrows = (limit >= 0 && limit < in.n) ? limit : in.n;
  return gather_table(in, (const uint32_t*)perm->p, mrows);
}

static Table exec_window(const Value& node, Metrics& m);  // with its plan

static Table exec_plan(const Value& node, Metrics& m) {
  const std::string op = node.get_str("op");
  if (op == "scan") {
    auto t0 = Clock::now();
    Table t = scan(node);
    m.scan_time_ns += ns_since(t0);
    return t;
  }
  if (op == "filter") {
    Table in = exec_plan(node.at("input"), m);
    return filter_materialize(in, eval_filter_node(in, node));
  }
  if (op == "project") return exec_project(node, m);
  if (op == "hash_join" || op == "nested_loop_join")
    return exec_join(node, m);
  if (op == "hash_aggregate") return exec_aggregate(node, m);
  if (op == "sort") return exec_sort(node, m);
  if (op == "window") return exec_window(node, m);
  if (op == "limit") {
    Table in = exec_plan(node.at("input"), m);
    int64_t lim = node.get_int("count");
    if (lim < in.n) in.n = lim;  // head slice: buffers stay valid
    return in;
  }
  throw StageError(BG_ERR_INVALID, "plan: unknown operator '" + op + "'");
}

// ---------------------------------------------------------------------------
// writers
// ---------------------------------------------------------------------------

static std::vector<uint8_t> hex_decode(const std::string& s) {
  auto nib = [](char c) -> int {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    if (c >= 'A' && c <= 'F') return c - 'A' + 10;
    throw StageError(BG_ERR_INVALID, "bad hex in schema_msg_hex");
  };
  std::vector<uint8_t> out(s.size() / 2);
  for (size_t i = 0; i < out.size(); ++i)
    out[i] = (uint8_t)((nib(s[2 * i]) << 4) | nib(s[2 * i + 1]));
  return out;
}

static const uint8_t LZ4F_HEADER[7] = {0x04, 0x22, 0x4d, 0x18,
                                       0x40, 0x40, 0xc0};

// One buffer to compress+emit: a device region.
struct EncBuf {
  const void* dptr = nullptr;
  int64_t len = 0;  // uncompressed bytes (0 = absent buffer)
};
// One batch: per Arrow buffer-slot (validity[, offsets], data per column).
struct EncBatch {
  int64_t rows = 0;
  std::vector<EncBuf> bufs;
  std::vector<bgipc::FieldNode> nodes;
};

struct WriteStats {
  int64_t num_batches = 0, num_rows = 0, num_bytes = 0;
};

// LZ4 block i of a buffer of len bytes: every block full but the last
static int32_t block_len(int64_t len, int64_t i) {
  return (int32_t)std::min<int64_t>(len - i * BG_LZ4_BLOCK, BG_LZ4_BLOCK);
}

// One non-empty buffer (partition p, batch b, slot s) and its block jobs.
struct BufRef { size_t p, b, s; int64_t len, job0; int nblocks; };
struct CompressedBlocks {
  std::vector<BufRef> refs;
  std::vector<bg_lz4_block_job> jobs;
  DBufPtr slots;               // one BG_LZ4_SLOT_STRIDE slot per job
  std::vector<int64_t> sizes;  // per job; negative = stored raw
};
// (p,b,s) -> (offset in the packed download, frame body length)
using PackedAt =
    std::map<std::tuple<size_t, size_t, size_t>, std::pair<int64_t, int64_t>>;

// every batch buffer of every partition through ONE flat LZ4 launch
static CompressedBlocks compress_blocks(
    const std::vector<std::vector<EncBatch>>& parts) {
  CompressedBlocks c;
  for (size_t p = 0; p < parts.size(); ++p)
    for (size_t b = 0; b < parts[p].size(); ++b)
      for (size_t s = 0; s < parts[p][b].bufs.size(); ++s) {
        auto& eb = parts[p][b].bufs[s];
        if (eb.len <= 0) continue;
        int nb = (int)((eb.len + BG_LZ4_BLOCK - 1) / BG_LZ4_BLOCK);
        c.refs.push_back({p, b, s, eb.len, (int64_t)c.jobs.size(), nb});
        for (int i = 0; i < nb; ++i)
          c.jobs.push_back(
              {(const uint8_t*)eb.dptr + (int64_t)i * BG_LZ4_BLOCK, nullptr,
               block_len(eb.len, i), 0});
      }
  c.slots = dalloc_elems((int64_t)c.jobs.size(), BG_LZ4_SLOT_STRIDE);
  for (size_t i = 0; i < c.jobs.size(); ++i)
    c.jobs[i].d_dst_slot = c.slots->u8() + (int64_t)i * BG_LZ4_SLOT_STRIDE;
  c.sizes.resize(c.jobs.size());
  if (!c.jobs.empty())
    chk(bg_lz4_compress_flat(c.jobs.data(), (int64_t)c.jobs.size(),
                             c.sizes.data()),
        "bg_lz4_compress_flat");
  return c;
}

// pack the [u32 size][block] frame bodies back to back in ONE launch and
// download them once; packed_at records where each buffer's body lies
static std::vector<uint8_t> pack_bodies(const CompressedBlocks& c,
                                        PackedAt* packed_at) {
  std::vector<bg_pack_job> pack_jobs;
  std::vector<int64_t> dst_offs;  // each job's offset in the packed buffer
  int64_t cursor = 0;
  for (auto& r : c.refs) {
    int64_t body = 0;
    const int64_t start = cursor;
    for (int i = 0; i < r.nblocks; ++i) {
      const int64_t sz = c.sizes[(size_t)(r.job0 + i)];
      const int32_t blen = block_len(r.len, i);
      const int64_t payload = sz < 0 ? blen : sz;
      const uint32_t word =
          sz < 0 ? ((uint32_t)blen | 0x80000000u) : (uint32_t)sz;
      pack_jobs.push_back(
          {c.jobs[(size_t)(r.job0 + i)].d_dst_slot, nullptr, payload, word, 0});
      dst_offs.push_back(cursor);
      cursor += 4 + payload;
      body += 4 + (sz < 0 ? -sz : sz);
    }
    (*packed_at)[{r.p, r.b, r.s}] = {start, body};
  }
  DBufPtr packed = dalloc_elems(cursor);
  for (size_t i = 0; i < pack_jobs.size(); ++i)
    pack_jobs[i].d_dst = packed->u8() + dst_offs[i];
  if (!pack_jobs.empty())
    chk(bg_pack_blocks(pack_jobs.data(), (int64_t)pack_jobs.size()),
        "bg_pack_blocks");
  chk(bg_synchronize(), "bg_synchronize");

  std::vector<uint8_t> host((size_t)(cursor ? cursor : 1));
  if (cursor)
    chk(bg_memcpy_d2h(host.data(), packed->p, (uint64_t)cursor),
        "bg_memcpy_d2h");
  return host;
}

// one record batch of partition p: metadata, then per buffer
// [i64 usize][LZ4 frame header][body][end mark], each 8-aligned
static void stream_batch(FILE* f, const EncBatch& eb, size_t p, size_t b,
                         const PackedAt& packed_at,
                         const std::vector<uint8_t>& packed_host,
                         WriteStats* stats) {
  std::vector<bgipc::BufSpec> bufspecs;
  int64_t body_len = 0;
  std::vector<std::pair<int64_t, int64_t>> emit;  // packed_at; -1 = absent
  for (size_t s = 0; s < eb.bufs.size(); ++s) {
    if (eb.bufs[s].len <= 0) {
      bufspecs.push_back({body_len, 0});
      emit.push_back({-1, 0});
      continue;
    }
    auto pa = packed_at.at({p, b, s});
    int64_t part_len = 8 + 7 + pa.second + 4;  // usize + hdr + body + end
    bufspecs.push_back({body_len, part_len});
    emit.push_back(pa);
    body_len += part_len;
    body_len += (-body_len) & 7;
  }
  std::string meta =
      bgipc::record_batch_message(eb.rows, eb.nodes, bufspecs, body_len, true);
  fwrite(meta.data(), 1, meta.size(), f);
  int64_t written = 0;
  for (size_t s = 0; s < eb.bufs.size(); ++s) {
    if (emit[s].first < 0) continue;
    int64_t usize = eb.bufs[s].len;
    fwrite(&usize, 8, 1, f);
    fwrite(LZ4F_HEADER, 1, 7, f);
    fwrite(packed_host.data() + emit[s].first, 1, (size_t)emit[s].second, f);
    const uint32_t endmark = 0;
    fwrite(&endmark, 4, 1, f);
    written += 8 + 7 + emit[s].second + 4;
    int64_t pad = (-written) & 7;
    if (pad) {
      const uint64_t z = 0;
      fwrite(&z, 1, (size_t)pad, f);
      written += pad;
    }
    if (stats) stats->num_bytes += usize;
  }
  if (stats) {
    stats->num_batches += 1;
    stats->num_rows += eb.rows;
  }
}

// host metadata interleaved with slices of the single packed download;
// returns the K+1 partition offsets of the index file
static std::vector<int64_t> stream_file(
    const std::string& data_path, const std::vector<uint8_t>& schema_msg,
    const std::vector<std::vector<EncBatch>>& parts,
    const PackedAt& packed_at, const std::vector<uint8_t>& packed_host,
    std::vector<WriteStats>* stats, bool leading_schema_stream,
    bool always_stream) {
  const size_t k = parts.size();
  FILE* f = fopen(data_path.c_str(), "wb");
  if (!f) throw StageError(BG_ERR_INVALID, "cannot create " + data_path);
  std::vector<char> iobuf(4 << 20);
  setvbuf(f, iobuf.data(), _IOFBF, iobuf.size());
  std::vector<int64_t> offsets(k + 1, 0);
  if (leading_schema_stream) {
    // leading schema-only stream (writer.rs:838-846)
    fwrite(schema_msg.data(), 1, schema_msg.size(), f);
    fwrite(bgipc::EOS, 1, 8, f);
  }
  if (stats) stats->assign(k, WriteStats{});
  for (size_t p = 0; p < k; ++p) {
    offsets[p] = (int64_t)ftello(f);
    bool any = always_stream;
    for (auto& b : parts[p]) any |= b.rows > 0;
    if (!any) continue;
    fwrite(schema_msg.data(), 1, schema_msg.size(), f);
    for (size_t b = 0; b < parts[p].size(); ++b)
      if (parts[p][b].rows != 0)
        stream_batch(f, parts[p][b], p, b, packed_at, packed_host,
                     stats ? &(*stats)[p] : nullptr);
    fwrite(bgipc::EOS, 1, 8, f);
  }
  offsets[k] = (int64_t)ftello(f);
  fclose(f);
  return offsets;
}

// Compress every batch buffer of every partition on device in ONE flat
// launch, pack the [u32 size][block] bodies at final offsets in ONE
// launch, then stream the file.  (The device half of
// encode_buffered_partitions + write_task_consolidated.)
static void write_consolidated(
    const std::string& data_path, const std::string& index_path,
    const std::vector<uint8_t>& schema_msg,
    const std::vector<std::vector<EncBatch>>& parts,  // per partition
    std::vector<WriteStats>* stats, bool leading_schema_stream = true,
    bool always_stream = false) {
  CompressedBlocks c = compress_blocks(parts);
  PackedAt packed_at;
  std::vector<uint8_t> packed_host = pack_bodies(c, &packed_at);
  std::vector<int64_t> offsets =
      stream_file(data_path, schema_msg, parts, packed_at, packed_host, stats,
                  leading_schema_stream, always_stream);
  if (!index_path.empty()) {
    FILE* fi = fopen(index_path.c_str(), "wb");
    if (!fi) throw StageError(BG_ERR_INVALID, "cannot create " + index_path);
    fwrite(offsets.data(), 8, offsets.size(), fi);
    fclose(fi);
  }
}
// Build the per-partition batch list for the hash-repartitioned table.
static void build_repartition_batches(
    const Table& t, uint32_t kparts, int64_t batch_size,
    const std::vector<int64_t>& offsets_host, const DBufPtr& idx,
    const std::vector<DBufPtr>& fixed_out, const std::vector<int>& fixed_ids,
    const std::map<int, std::tuple<DBufPtr, DBufPtr, int64_t>>& utf8_out,
    std::vector<std::vector<EncBatch>>* parts,
    std::vector<DBufPtr>* keepalive) {
  size_t ncols = t.cols.size();
  // per-(nullable col, partition) bit-gathers: batches inside a partition
  // start at batch_size multiples => byte-aligned bitmap slices
  std::map<std::pair<int, int>, DBufPtr> part_valid;
  // host copies for null counts
  std::map<std::pair<int, int>, std::vector<uint8_t>> part_valid_host;
  for (size_t c = 0; c < ncols; ++c) {
    if (!t.cols[c].nullable()) continue;
    for (uint32_t p = 0; p < kparts; ++p) {
      int64_t lo = offsets_host[p], hi = offsets_host[p + 1];
      int64_t mrows = hi - lo;
      if (mrows == 0) continue;
      DBufPtr vb = alloc_bitmap(mrows);
      chk(bg_gather_bits(t.cols[c].vptr(), (const uint32_t*)idx->u8() + lo,
                         mrows, vb->u8()),
          "bg_gather_bits");
      part_valid[{(int)c, (int)p}] = vb;
    }
  }
  // utf8: host offsets for slicing + per-batch rebase buffers
  std::map<int, std::vector<int32_t>> utf8_offs_host;
  for (auto& kv : utf8_out) {
    auto& [oo, od, tot] = kv.second;
    std::vector<int32_t> h((size_t)t.n + 1);
    chk(bg_memcpy_d2h(h.data(), oo->p, (uint64_t)(t.n + 1) * 4),
        "bg_memcpy_d2h");
    utf8_offs_host[kv.first] = std::move(h);
  }
  chk(bg_synchronize(), "bg_synchronize");
  // null counts need the bitmaps on host
  for (auto& kv : part_valid) {
    std::vector<uint8_t> h((size_t)kv.second->bytes);
    chk(bg_memcpy_d2h(h.data(), kv.second->p, kv.second->bytes),
        "bg_memcpy_d2h");
    part_valid_host[kv.first] = std::move(h);
  }

  auto popcount_zero = [](const uint8_t* bits, int64_t bit0, int64_t n) {
    int64_t nulls = 0;
    for (int64_t i = 0; i < n; ++i)
      if (!((bits[(bit0 + i) >> 3] >> ((bit0 + i) & 7)) & 1)) ++nulls;
    return nulls;
  };

  parts->assign(kparts, {});
  for (uint32_t p = 0; p < kparts; ++p) {
    int64_t lo = offsets_host[p], hi = offsets_host[p + 1];
    for (int64_t b0 = lo; b0 < hi; b0 += batch_size) {
      int64_t mrows = (hi - b0 < batch_size) ? hi - b0 : batch_size;
      EncBatch eb;
      eb.rows = mrows;
      for (size_t c = 0; c < ncols; ++c) {
        int64_t nulls = 0;
        auto pv = part_valid.find({(int)c, (int)p});
        if (pv != part_valid.end()) {
          auto& hbits = part_valid_host[{(int)c, (int)p}];
          nulls = popcount_zero(hbits.data(), b0 - lo, mrows);
        }
        eb.nodes.push_back({mrows, nulls});
        // validity slot
        if (pv != part_valid.end() && nulls > 0) {
          eb.bufs.push_back(
              {pv->second->u8() + (b0 - lo) / 8, (mrows + 7) / 8});
        } else {
          eb.bufs.push_back({nullptr, 0});
        }
        auto ut = utf8_out.find((int)c);
        if (ut != utf8_out.end()) {
          auto& [oo, od, tot] = ut->second;
          auto& oh = utf8_offs_host[(int)c];
          // per-batch rebased offsets buffer
          DBufPtr reb = dalloc((uint64_t)(mrows + 1) * 4);
          chk(bg_sub_i32(oo->u8() + 4 * b0, mrows + 1, oh[(size_t)b0],
                         reb->p),
              "bg_sub_i32");
          keepalive->push_back(reb);
          eb.bufs.push_back({reb->p, (mrows + 1) * 4});
          int64_t d0 = oh[(size_t)b0], d1 = oh[(size_t)(b0 + mrows)];
          eb.bufs.push_back({od->u8() + d0, d1 - d0});
        } else {
          int fslot = -1;
          for (size_t fi = 0; fi < fixed_ids.size(); ++fi)
            if (fixed_ids[fi] == (int)c) fslot = (int)fi;
          int64_t esz = dt_size(t.cols[c].dtype);
          eb.bufs.push_back({fixed_out[(size_t)fslot]->u8() + b0 * esz,
                             mrows * esz});
        }
      }
      (*parts)[p].push_back(std::move(eb));
    }
  }
  for (auto& kv : part_valid) keepalive->push_back(kv.second);
}

// {work_dir}/{job}/{stage}/{leaf}, created
static std::string task_dir(const Value& doc, int64_t leaf) {
  std::string dir = doc.get_str("work_dir") + "/" + doc.get_str("job_id") +
                    "/" + std::to_string(doc.get_int("stage_id")) + "/" +
                    std::to_string(leaf);
  mkdirs(dir);
  return dir;
}

// one {...} entry of the result's "partitions" list
static void emit_partition_json(bgjson::Writer& res, int64_t id,
                                const std::string& path,
                                const WriteStats& stats) {
  res.raw("{\"partition_id\":");
  res.num(id);
  res.raw(",\"path\":");
  res.str(path);
  res.raw(",\"num_batches\":");
  res.num(stats.num_batches);
  res.raw(",\"num_rows\":");
  res.num(stats.num_rows);
  res.raw(",\"num_bytes\":");
  res.num(stats.num_bytes);
  res.raw("}");
}

static void exec_sort_shuffle_write(const Value& root, const Value& plan_doc,
                                    Metrics& m, bgjson::Writer& res) {
  Table t = exec_plan(root.at("input"), m);
  uint32_t kparts = (uint32_t)root.get_int("k");
  int64_t batch_size =
      plan_doc.get_int_or("batch_size", 8192);  // sort_shuffle/config.rs:35-43
  if (batch_size % 8 != 0)
    throw StageError(BG_ERR_INVALID, "batch_size must be a multiple of 8");
  auto schema_msg = hex_decode(plan_doc.get_str("schema_msg_hex"));

  auto t0 = Clock::now();
  // key EXPRESSIONS evaluated before hashing (writer.rs:1265, 1259-1279)
  std::vector<Col> key_cols_own;
  for (auto& ke : root.get_arr("keys")) {
    ExprVal v = eval_expr(t, *ke);
    if (v.is_lit) throw StageError(BG_ERR_INVALID, "literal partition key");
    key_cols_own.push_back(v.col);
  }
  std::vector<bg_column> kcols;
  for (auto& c : key_cols_own) kcols.push_back(to_bg(c, t.n));

  std::vector<int> fixed_ids;
  std::map<int, std::tuple<DBufPtr, DBufPtr, int64_t>> utf8_out;
  std::vector<bg_column> payload;
  for (size_t c = 0; c < t.cols.size(); ++c) {
    if (t.cols[c].dtype == BG_DT_UTF8) continue;
    fixed_ids.push_back((int)c);
    payload.push_back(to_bg(t.cols[c], t.n));
  }

  DBufPtr idx = dalloc_elems(t.n, 4);
  DBufPtr offs = dalloc((uint64_t)(kparts + 1) * 8);
  std::vector<DBufPtr> fixed_out;
  std::vector<void*> outp;
  for (int c : fixed_ids) {
    fixed_out.push_back(dalloc_elems(t.n, dt_size(t.cols[(size_t)c].dtype)));
    outp.push_back(fixed_out.back()->p);
  }
  chk(bg_hash_repartition(kcols.data(), (int32_t)kcols.size(), payload.data(),
                          (int32_t)payload.size(), t.n, kparts,
                          (uint32_t*)idx->p, (int64_t*)offs->p, outp.data()),
      "bg_hash_repartition");
  // variable-length payload through the same permutation
  for (size_t c = 0; c < t.cols.size(); ++c) {
    if (t.cols[c].dtype != BG_DT_UTF8) continue;
    DBufPtr oo = dalloc((uint64_t)(t.n + 1) * 4);
    DBufPtr od = dalloc_elems(t.cols[c].data_bytes);
    const int64_t cap = (int64_t)od->bytes;
    int64_t tot = 0;
    chk(bg_gather_varlen(t.cols[c].dptr(), t.cols[c].optr(),
                         (const uint32_t*)idx->p, t.n, (int32_t*)oo->p,
                         od->p, cap, &tot),
        "bg_gather_varlen");
    utf8_out[(int)c] = {oo, od, tot};
  }
  std::vector<int64_t> offsets_host(kparts + 1);
  chk(bg_memcpy_d2h(offsets_host.data(), offs->p, (kparts + 1) * 8),
      "bg_memcpy_d2h");
  chk(bg_synchronize(), "bg_synchronize");
  m.repart_time_ns = ns_since(t0);

  auto t1 = Clock::now();
  std::vector<std::vector<EncBatch>> parts;
  std::vector<DBufPtr> keepalive;
  build_repartition_batches(t, kparts, batch_size, offsets_host, idx,
                            fixed_out, fixed_ids, utf8_out, &parts,
                            &keepalive);

  // {work_dir}/{job}/{stage}/{task}/data.arrow (+.index)
  std::string data_path =
      task_dir(plan_doc, plan_doc.get_int("task_id")) + "/data.arrow";
  std::vector<WriteStats> stats;
  write_consolidated(data_path, data_path + ".index", schema_msg, parts,
                     &stats);
  m.write_time_ns = ns_since(t1);
  int64_t total_rows = 0;
  res.raw("\"partitions\":[");
  for (size_t p = 0; p < stats.size(); ++p) {
    if (p) res.raw(",");
    emit_partition_json(res, (int64_t)p, data_path, stats[p]);
    total_rows += stats[p].num_rows;
  }
  res.raw("]");
  m.output_rows = total_rows;
}

static void exec_passthrough_write(const Value& root, const Value& plan_doc,
                                   Metrics& m, bgjson::Writer& res) {
  Table t = exec_plan(root.at("input"), m);
  int64_t batch_size = plan_doc.get_int_or("batch_size", 8192);
  if (batch_size % 8 != 0)
    throw StageError(BG_ERR_INVALID, "batch_size must be a multiple of 8");
  auto schema_msg = hex_decode(plan_doc.get_str("schema_msg_hex"));
  int64_t gp = root.get_int("global_partition");

  auto t1 = Clock::now();
  // identity layout: batches are row slices — no permutation, but
  // validity/offsets still need batch-aligned forms; reuse the repartition
  // batch builder with a single identity "partition"
  DBufPtr idx = dalloc_elems(t.n, 4);
  {
    // identity permutation (for bit-gather only when any column nullable)
    std::vector<uint32_t> h((size_t)t.n);
    for (int64_t i = 0; i < t.n; ++i) h[(size_t)i] = (uint32_t)i;
    if (t.n) chk(bg_memcpy_h2d(idx->p, h.data(), (uint64_t)t.n * 4),
                 "bg_memcpy_h2d");
  }
  std::vector<int> fixed_ids;
  std::vector<DBufPtr> fixed_out;
  std::map<int, std::tuple<DBufPtr, DBufPtr, int64_t>> utf8_out;
  for (size_t c = 0; c < t.cols.size(); ++c) {
    if (t.cols[c].dtype == BG_DT_UTF8) {
      // wrap existing buffers (copy refs); rebase handled per batch
      DBufPtr oo, od;
      if (t.cols[c].offsets) oo = t.cols[c].offsets;
      else {
        oo = dalloc((uint64_t)(t.n + 1) * 4);
        chk(bg_memcpy_dtod(oo->p, t.cols[c].optr(), (uint64_t)(t.n + 1) * 4),
            "bg_memcpy_dtod");
      }
      if (t.cols[c].data) od = t.cols[c].data;
      else {
        od = dalloc_elems(t.cols[c].data_bytes);
        chk(bg_memcpy_dtod(od->p, t.cols[c].dptr(),
                           (uint64_t)t.cols[c].data_bytes),
            "bg_memcpy_dtod");
      }
      utf8_out[(int)c] = {oo, od, t.cols[c].data_bytes};
    } else {
      fixed_ids.push_back((int)c);
      if (t.cols[c].data) fixed_out.push_back(t.cols[c].data);
      else {
        int64_t esz = dt_size(t.cols[c].dtype);
        DBufPtr b = dalloc_elems(t.n, esz);
        chk(bg_memcpy_dtod(b->p, t.cols[c].dptr(),
                           (uint64_t)t.n * (uint64_t)esz),
            "bg_memcpy_dtod");
        fixed_out.push_back(b);
      }
    }
  }
  std::vector<int64_t> offsets_host = {0, t.n};
  std::vector<std::vector<EncBatch>> parts;
  std::vector<DBufPtr> keepalive;
  build_repartition_batches(t, 1, batch_size, offsets_host, idx, fixed_out,
                            fixed_ids, utf8_out, &parts, &keepalive);

  std::string data_path = task_dir(plan_doc, gp) + "/data-" +
                          std::to_string(plan_doc.get_int("task_id")) +
                          ".arrow";
  std::vector<WriteStats> stats;
  write_consolidated(data_path, "", schema_msg, parts, &stats,
                     /*leading_schema_stream=*/false, /*always_stream=*/true);
  m.write_time_ns = ns_since(t1);
  res.raw("\"partitions\":[");
  emit_partition_json(res, gp, data_path, stats[0]);
  res.raw("]");
  m.output_rows = stats[0].num_rows;
}

// the first nrows rows of a column, downloaded
struct HostCol {
  std::vector<uint8_t> data, valid;
  std::vector<int32_t> offs;
  std::vector<uint8_t> strdata;
};

static HostCol download_col(const Col& col, int64_t nrows) {
  HostCol hc;
  if (col.dtype == BG_DT_UTF8) {
    hc.offs.resize((size_t)nrows + 1);
    if (nrows)
      chk(bg_memcpy_d2h(hc.offs.data(), col.optr(), (uint64_t)(nrows + 1) * 4),
          "bg_memcpy_d2h");
    else hc.offs = {0};
    int64_t nb = hc.offs[(size_t)nrows] - hc.offs[0];
    hc.strdata.resize((size_t)(nb > 0 ? nb : 0));
    if (nb)
      chk(bg_memcpy_d2h(hc.strdata.data(),
                        (const uint8_t*)col.dptr() + hc.offs[0], (uint64_t)nb),
          "bg_memcpy_d2h");
  } else {
    int64_t esz = dt_size(col.dtype);
    hc.data.resize((size_t)(nrows * esz));
    if (nrows)
      chk(bg_memcpy_d2h(hc.data.data(), col.dptr(), (uint64_t)(nrows * esz)),
          "bg_memcpy_d2h");
  }
  if (col.nullable()) {
    hc.valid.resize((size_t)((nrows + 7) / 8) + 8);
    if (nrows)
      chk(bg_memcpy_d2h(hc.valid.data(), col.vptr(),
                        (uint64_t)((nrows + 7) / 8)),
          "bg_memcpy_d2h");
  }
  return hc;
}

// row r of a column as a JSON value
static void emit_cell(bgjson::Writer& res, int32_t dtype, const HostCol& hc,
                      int64_t r) {
  if (!hc.valid.empty() && !((hc.valid[(size_t)(r >> 3)] >> (r & 7)) & 1)) {
    res.raw("null");
    return;
  }
  switch (dtype) {
    case BG_DT_INT32:
    case BG_DT_DATE32: {
      int32_t v;
      memcpy(&v, hc.data.data() + r * 4, 4);
      res.num(v);
      break;
    }
    case BG_DT_DICT8: res.num(hc.data[(size_t)r]); break;
    case BG_DT_INT64: {
      int64_t v;
      memcpy(&v, hc.data.data() + r * 8, 8);
      res.num(v);
      break;
    }
    case BG_DT_FLOAT64: {
      double v;
      memcpy(&v, hc.data.data() + r * 8, 8);
      res.dbl(v);
      break;
    }
    case BG_DT_DECIMAL128: {
      unsigned __int128 u = 0;
      memcpy(&u, hc.data.data() + r * 16, 16);
      __int128 v = (__int128)u;
      // decimal integer string (scaled); host formats with scale
      char buf[48];
      int pos = 47;
      buf[pos] = '\0';
      bool neg = v < 0;
      unsigned __int128 uv = neg ? (unsigned __int128)(-v)
                                 : (unsigned __int128)v;
      if (uv == 0) buf[--pos] = '0';
      while (uv) {
        buf[--pos] = (char)('0' + (int)(uv % 10));
        uv /= 10;
      }
      if (neg) buf[--pos] = '-';
      res.raw("\"");
      res.raw(buf + pos);
      res.raw("\"");
      break;
    }
    case BG_DT_UTF8: {
      int32_t lo = hc.offs[(size_t)r] - hc.offs[0];
      int32_t hi = hc.offs[(size_t)r + 1] - hc.offs[0];
      res.str(std::string((const char*)hc.strdata.data() + lo,
                          (size_t)(hi - lo)));
      break;
    }
  }
}

// collect root: download and serialise rows (final stages / tests)
static void exec_collect(const Value& root, Metrics& m, bgjson::Writer& res) {
  Table t = exec_plan(root.at("input"), m);
  int64_t limit = root.get_int_or("limit", t.n);
  int64_t nrows = limit < t.n ? limit : t.n;
  m.output_rows = nrows;
  chk(bg_synchronize(), "bg_synchronize");

  res.raw("\"schema\":[");
  for (size_t c = 0; c < t.cols.size(); ++c) {
    if (c) res.raw(",");
    res.raw("{\"name\":");
    res.str(t.names[c]);
    res.raw(",\"dtype\":");
    res.str(dtype_name(t.cols[c].dtype));
    if (t.cols[c].dtype == BG_DT_DECIMAL128) {
      res.raw(",\"precision\":");
      res.num(t.cols[c].precision);
      res.raw(",\"scale\":");
      res.num(t.cols[c].scale);
    }
    res.raw("}");
  }
  res.raw("],\"rows\":[");

  std::vector<HostCol> host;
  for (auto& col : t.cols) host.push_back(download_col(col, nrows));
  for (int64_t r = 0; r < nrows; ++r) {
    if (r) res.raw(",");
    res.raw("[");
    for (size_t c = 0; c < t.cols.size(); ++c) {
      if (c) res.raw(",");
      emit_cell(res, t.cols[c].dtype, host[c], r);
    }
    res.raw("]");
  }
  res.raw("]");
}

// ---------------------------------------------------------------------------
// validation (CPU-only plan walk)
// ---------------------------------------------------------------------------

struct VSchema {
  std::vector<std::string> names;
  std::vector<DtSpec> dts;
  int idx(const std::string& n) const {
    for (size_t i = 0; i < names.size(); ++i)
      if (names[i] == n) return (int)i;
    throw StageError(BG_ERR_INVALID, "plan: unknown column '" + n + "'");
  }
};

static DtSpec validate_expr(const VSchema& s, const Value& e);

// how an error message names an operand: the column, or the expression
// node with the operand inside it, e.g. substr(c_phone)
static std::string expr_label(const Value& e) {
  if (e.has("col")) return e.get_str("col");
  for (const char* k : {"date_part", "substr", "cast"})
    if (e.has(k))
      return std::string(k) + "(" + expr_label(e.at(k).at("arg")) + ")";
  return e.kind == Value::OBJ && !e.obj.empty() ? e.obj[0].first : "?";
}

// The one predicate validator: filter groups and case.when both use it.
// Operand is {"col"} or {"expr"}; the form is column-to-column ("rhs"),
// LIKE, IN (string values iff the operand is utf8) or a literal cmp.
static void validate_predicate(const VSchema& s, const Value& p) {
  DtSpec opd;
  std::string name;
  if (p.has("expr")) {
    opd = validate_expr(s, p.at("expr"));
    name = expr_label(p.at("expr"));
  } else {
    name = p.get_str("col");
    opd = s.dts[(size_t)s.idx(name)];
  }
  if (p.has("rhs")) {
    for (const char* k : {"lo", "hi", "like", "in"})
      if (p.has(k))
        throw StageError(BG_ERR_INVALID,
                         "filter: 'rhs' compare on '" + name +
                             "' cannot also carry '" + k + "'");
    cmp_cols_code(p.get_str("cmp"));
    const std::string& rname = p.at("rhs").get_str("col");
    const DtSpec r = s.dts[(size_t)s.idx(rname)];
    const std::string pair = "'" + name + "' (" + dtype_name(opd.dt) +
                             ") vs rhs '" + rname + "' (" +
                             dtype_name(r.dt) + ")";
    if (opd.dt != r.dt)
      throw StageError(BG_ERR_INVALID,
                       "filter: rhs compare dtype mismatch: " + pair);
    if (opd.dt == BG_DT_FLOAT64 || opd.dt == BG_DT_UTF8)
      throw StageError(BG_ERR_UNSUPPORTED,
                       "filter: rhs compare of float64/utf8 columns: " + pair);
    if (opd.dt == BG_DT_DECIMAL128 && opd.scale != r.scale)
      throw StageError(BG_ERR_INVALID,
                       "filter: rhs compare scale mismatch: " + pair +
                           ", scales " + std::to_string(opd.scale) + " and " +
                           std::to_string(r.scale));
    return;
  }
  if (p.has("like")) return;
  if (p.has("in")) {
    const bool strs = in_values_are_strings(p);
    if (strs != (opd.dt == BG_DT_UTF8))
      throw StageError(BG_ERR_INVALID,
                       std::string("filter: 'in' with ") +
                           (strs ? "string" : "integer") + " values on '" +
                           name + "' (" + dtype_name(opd.dt) + ")");
    return;
  }
  cmp_code(p.get_str("cmp"));
}

static void validate_predicates(const VSchema& s,
                                const std::vector<ValuePtr>& preds) {
  for (auto& p : preds) validate_predicate(s, *p);
}

// every {"col": name} under a predicate (operand, rhs, expression leaves)
static void pred_columns(const Value& v, std::vector<std::string>& out) {
  for (auto& kv : v.obj) {
    if (kv.first == "col" && kv.second->kind == Value::STR)
      out.push_back(kv.second->s);
    else
      pred_columns(*kv.second, out);
  }
  for (auto& e : v.arr) pred_columns(*e, out);
}

static bool schema_has(const VSchema& s, const std::string& n) {
  return std::find(s.names.begin(), s.names.end(), n) != s.names.end();
}

// one side's predicate list of a join filter group: the ordinary pred
// grammar, over that side's columns only
static void validate_join_filter_side(const std::string& op,
                                      const VSchema& own, const VSchema& other,
                                      const char* side, const char* other_side,
                                      const Value& preds) {
  for (auto& p : preds.arr) {
    std::vector<std::string> names;
    pred_columns(*p, names);
    for (auto& n : names)
      if (!schema_has(own, n))
        throw StageError(
            BG_ERR_INVALID,
            op + " filter: '" + side + "' predicate names '" +
                n + "', " +
                (schema_has(other, n)
                     ? std::string("a column of the ") + other_side + " side"
                     : std::string("a column of neither side")));
    validate_predicate(own, *p);
  }
}

// A join node's "filter": {"any": [{build?, probe?, cross?}...]}; op is the
// node's name (hash_join, nested_loop_join), b and p are the build and probe
// schemas
static void validate_join_filter(const std::string& op, const VSchema& b,
                                 const VSchema& p, const Value& filt) {
  auto& groups = filt.get_arr("any");
  if (groups.empty())
    throw StageError(BG_ERR_INVALID,
                     op + " filter: empty 'any' (omit the filter)");
  if (groups.size() > BG_JOIN_FILTER_MAX_GROUPS)
    throw StageError(BG_ERR_UNSUPPORTED,
                     op + " filter: " + std::to_string(groups.size()) +
                         " groups in 'any', at most 4");
  for (size_t gi = 0; gi < groups.size(); ++gi) {
    const Value& g = *groups[gi];
    const std::string where = op + " filter: group " + std::to_string(gi);
    size_t nterms = 0;
    if (g.has("build")) {
      validate_join_filter_side(op, b, p, "build", "probe", g.at("build"));
      nterms += g.get_arr("build").size();
    }
    if (g.has("probe")) {
      validate_join_filter_side(op, p, b, "probe", "build", g.at("probe"));
      nterms += g.get_arr("probe").size();
    }
    if (g.has("cross")) {
      auto& cross = g.get_arr("cross");
      nterms += cross.size();
      if (cross.size() > BG_JOIN_FILTER_MAX_CROSS)
        throw StageError(BG_ERR_UNSUPPORTED,
                         where + " has " + std::to_string(cross.size()) +
                             " cross terms, at most 4");
      for (auto& x : cross) {
        const std::string& bn = x->get_str("build");
        const std::string& pn = x->get_str("probe");
        const std::string& cmp = x->get_str("cmp");
        if (!schema_has(b, bn))
          throw StageError(BG_ERR_INVALID,
                           where + ": cross term's build column '" + bn +
                               "' is not a column of the build side");
        if (!schema_has(p, pn))
          throw StageError(BG_ERR_INVALID,
                           where + ": cross term's probe column '" + pn +
                               "' is not a column of the probe side");
        try {
          cmp_cols_code(cmp);
        } catch (const StageError&) {
          throw StageError(BG_ERR_INVALID,
                           where + ": unknown cross cmp '" + cmp +
                               "' (lt/le/gt/ge/eq/ne)");
        }
        const DtSpec bd = b.dts[(size_t)b.idx(bn)];
        const DtSpec pd = p.dts[(size_t)p.idx(pn)];
        const std::string pair = "build '" + bn + "' (" + dtype_name(bd.dt) +
                                 ") vs probe '" + pn + "' (" +
                                 dtype_name(pd.dt) + ")";
        if (bd.dt != pd.dt)
          throw StageError(BG_ERR_INVALID,
                           where + ": cross term dtype mismatch: " + pair);
        if (bd.dt == BG_DT_FLOAT64 || bd.dt == BG_DT_UTF8)
          throw StageError(BG_ERR_UNSUPPORTED,
                           where + ": cross term over float64/utf8 columns: " +
                               pair);
        if (bd.dt == BG_DT_DECIMAL128 && bd.scale != pd.scale)
          throw StageError(BG_ERR_INVALID,
                           where + ": cross term scale mismatch: " + pair +
                               ", scales " + std::to_string(bd.scale) +
                               " and " + std::to_string(pd.scale));
      }
    }
    if (nterms == 0)
      throw StageError(BG_ERR_INVALID,
                       where + " is empty (always true: omit the filter "
                               "instead)");
  }
}

// ---------------------------------------------------------------------------
// window: ranking and framed aggregates over sorted input (DataFusion's
// WindowAggExec / BoundedWindowAggExec, Ballista's
// PartitionedBoundedWindowAggExec).  plan_window is the one reading of the
// node: bg_stage_validate and execution both go through it, so what
// validation accepts is what runs.
// ---------------------------------------------------------------------------

struct WinBound {
  int32_t kind = BG_WIN_UNBOUNDED;
  bool is_int = true;  // how the plan spelled the offset
  int64_t i = 0;
  double d = 0.0;
  bool offset() const { return kind >= BG_WIN_PRECEDING; }
  // where the bound sits relative to the current row, for the ordering
  // check only: preceding < 0 < following
  double pos(bool is_start) const {
    const double inf = 1e300;
    switch (kind) {
      case BG_WIN_UNBOUNDED: return is_start ? -inf : inf;
      case BG_WIN_CURRENT_ROW: return 0.0;
      case BG_WIN_PRECEDING: return -d;
      default: return d;
    }
  }
  std::string text(bool is_start) const {
    auto num = [this]() {
      if (is_int) return std::to_string(i);
      char buf[32];
      snprintf(buf, sizeof(buf), "%g", d);
      return std::string(buf);
    };
    switch (kind) {
      case BG_WIN_UNBOUNDED:
        return is_start ? "unbounded preceding" : "unbounded following";
      case BG_WIN_CURRENT_ROW: return "current row";
      case BG_WIN_PRECEDING: return num() + " preceding";
      default: return num() + " following";
    }
  }
};

struct WinFrame {
  int32_t units = BG_WIN_ROWS;
  WinBound start, end;
  std::string text() const {
    return std::string(units == BG_WIN_ROWS ? "rows" : "range") + " between " +
           start.text(true) + " and " + end.text(false);
  }
  bool range_offset() const {
    return units == BG_WIN_RANGE && (start.offset() || end.offset());
  }
};

struct WinOrderKey {
  std::string col;
  bool desc, nulls_first;
};

struct WinExpr {
  std::string fn, as;
  bool ranking = false;
  const Value* expr = nullptr;  // nullptr: ranking, or count(*)
  WinFrame frame;
  DtSpec in = DT_I64;  // the evaluated expression's dtype
  DtSpec out = DT_I64;
};

struct WinPlan {
  std::vector<std::string> part;
  std::vector<WinOrderKey> order;
  std::vector<WinExpr> exprs;
};

static WinBound parse_window_bound(const std::string& who, const Value& b) {
  WinBound r;
  if (b.kind == Value::STR) {
    if (b.s == "unbounded") r.kind = BG_WIN_UNBOUNDED;
    else if (b.s == "current_row") r.kind = BG_WIN_CURRENT_ROW;
    else
      throw StageError(BG_ERR_INVALID, who + ": unknown frame bound '" + b.s +
                                           "'");
    return r;
  }
  const bool prec = b.kind == Value::OBJ && b.has("preceding");
  const bool foll = b.kind == Value::OBJ && b.has("following");
  if (prec == foll)
    throw StageError(BG_ERR_INVALID,
                     who + ": a frame bound is \"unbounded\", \"current_row\", "
                           "{preceding: N} or {following: N}");
  r.kind = prec ? BG_WIN_PRECEDING : BG_WIN_FOLLOWING;
  const Value& v = b.at(prec ? "preceding" : "following");
  if (v.kind == Value::INT) {
    r.i = v.i;
    r.d = (double)v.i;
  } else if (v.kind == Value::DBL) {
    r.is_int = false;
    r.d = v.d;
  } else {
    throw StageError(BG_ERR_INVALID, who + ": frame offset must be a number");
  }
  if (!(r.d >= 0.0))
    throw StageError(BG_ERR_INVALID,
                     who + ": negative frame offset (" + r.text(true) + ")");
  return r;
}

// One frame, checked against the node's order keys; `who` names the node
// and the expression in every refusal.
static WinFrame parse_window_frame(const std::string& who, const Value& f,
                                   const std::vector<DtSpec>& order_dts) {
  WinFrame fr;
  const std::string units = f.get_str("units");
  if (units == "groups")
    throw StageError(BG_ERR_UNSUPPORTED, who + ": frame units 'groups'");
  if (units != "rows" && units != "range")
    throw StageError(BG_ERR_INVALID,
                     who + ": unknown frame units '" + units + "'");
  fr.units = units == "rows" ? BG_WIN_ROWS : BG_WIN_RANGE;
  fr.start = parse_window_bound(who, f.at("start"));
  fr.end = parse_window_bound(who, f.at("end"));
  if (fr.start.pos(true) > fr.end.pos(false))
    throw StageError(BG_ERR_INVALID, who + ": frame start lies after its end (" +
                                         fr.text() + ")");
  if (fr.units == BG_WIN_ROWS) {
    for (const WinBound* b : {&fr.start, &fr.end})
      if (b->offset() && !b->is_int)
        throw StageError(BG_ERR_INVALID,
                         who + ": a rows offset must be an integer (" +
                             fr.text() + ")");
  }
  if (fr.range_offset()) {
    if (order_dts.size() != 1)
      throw StageError(BG_ERR_INVALID,
                       who + ": a range offset needs exactly one order_by "
                             "key, the node has " +
                           std::to_string(order_dts.size()) + " (" +
                           fr.text() + ")");
    const int32_t dt = order_dts[0].dt;
    if (dt != BG_DT_INT64 && dt != BG_DT_INT32 && dt != BG_DT_DATE32 &&
        dt != BG_DT_FLOAT64)
      throw StageError(BG_ERR_UNSUPPORTED,
                       who + ": a range offset over a " +
                           std::string(dtype_name(dt)) + " order_by key (" +
                           fr.text() + ")");
    for (const WinBound* b : {&fr.start, &fr.end})
      if (b->offset() && !b->is_int && dt != BG_DT_FLOAT64)
        throw StageError(BG_ERR_INVALID,
                         who + ": a fractional range offset over a " +
                             std::string(dtype_name(dt)) + " order_by key (" +
                             fr.text() + ")");
  }
  return fr;
}

// Whether fn runs over dt under this frame: the one dtype verdict.
static void check_window_agg(const std::string& who, const std::string& fn,
                             int32_t dt, const WinFrame& fr) {
  if (fn == "count") return;  // reads validity only
  if (fn == "min" || fn == "max") {
    if (dt != BG_DT_INT64 && dt != BG_DT_INT32 && dt != BG_DT_DATE32 &&
        dt != BG_DT_FLOAT64 && dt != BG_DT_DECIMAL128)
      throw StageError(BG_ERR_UNSUPPORTED,
                       who + ": " + fn + " over " + dtype_name(dt) + " (" +
                           fr.text() + ")");
    if (fr.start.kind != BG_WIN_UNBOUNDED)
      throw StageError(BG_ERR_UNSUPPORTED,
                       who + ": sliding " + fn + " (" + fr.text() +
                           "); the frame must start at unbounded preceding");
    return;
  }
  const bool ok = dt == BG_DT_DECIMAL128 || dt == BG_DT_FLOAT64 ||
                  (dt == BG_DT_INT64 && fn == "sum");
  if (!ok)
    throw StageError(BG_ERR_UNSUPPORTED,
                     who + ": " + fn + " over " + dtype_name(dt));
}

static const char* const WIN_RANK_FNS[] = {"row_number", "rank", "dense_rank"};

static WinPlan plan_window(const Value& node, const VSchema& in) {
  WinPlan p;
  auto key_col = [&in](const char* list, const std::string& name) {
    if (!schema_has(in, name))
      throw StageError(BG_ERR_INVALID, std::string("window: ") + list +
                                           " names unknown column '" + name +
                                           "'");
    return in.dts[(size_t)in.idx(name)];
  };
  auto& part = node.get_arr("partition_by");
  auto& order = node.get_arr("order_by");
  for (auto* l : {&part, &order})
    if (l->size() > 4)
      throw StageError(BG_ERR_INVALID,
                       std::string("window: ") +
                           (l == &part ? "partition_by" : "order_by") +
                           " has " + std::to_string(l->size()) +
                           " keys, at most 4");
  for (auto& k : part) {
    key_col("partition_by", k->s);
    p.part.push_back(k->s);
  }
  std::vector<DtSpec> order_dts;
  for (auto& k : order) {
    const std::string col = k->get_str("col");
    order_dts.push_back(key_col("order_by", col));
    const bool d = k->get_bool_or("desc", false);
    p.order.push_back({col, d, k->get_bool_or("nulls_first", d)});
  }
  auto& exprs = node.get_arr("exprs");
  if (exprs.empty())
    throw StageError(BG_ERR_INVALID, "window: 'exprs' is empty");
  for (auto& ev : exprs) {
    WinExpr e;
    e.fn = ev->get_str("fn");
    e.as = ev->get_str("as");
    const std::string who = "window: " + e.fn + " as '" + e.as + "'";
    if (schema_has(in, e.as))
      throw StageError(BG_ERR_INVALID,
                       who + ": the name collides with an input column");
    for (auto& prev : p.exprs)
      if (prev.as == e.as)
        throw StageError(BG_ERR_INVALID, who + ": duplicate output name");
    for (const char* r : WIN_RANK_FNS)
      if (e.fn == r) e.ranking = true;
    if (e.ranking) {
      if (ev->has("expr"))
        throw StageError(BG_ERR_INVALID, who + ": a ranking fn takes no expr");
      p.exprs.push_back(e);
      continue;
    }
    if (e.fn != "sum" && e.fn != "avg" && e.fn != "min" && e.fn != "max" &&
        e.fn != "count")
      throw StageError(BG_ERR_INVALID, who + ": unknown window fn");
    if (!ev->has("frame"))
      throw StageError(BG_ERR_INVALID, who + ": an aggregate needs a frame");
    if (ev->has("expr")) e.expr = &ev->at("expr");
    else if (e.fn != "count")
      throw StageError(BG_ERR_INVALID, who + ": expr required");
    e.frame = parse_window_frame(who, ev->at("frame"), order_dts);
    if (e.expr) {
      e.in = validate_expr(in, *e.expr);
      if (is_literal_node(*e.expr))
        throw StageError(BG_ERR_INVALID, who + ": bare literal expression");
      check_window_agg(who, e.fn, e.in.dt, e.frame);
    }
    e.out = agg_output_fields(e.fn, "single", e.as, e.in)[0].dt;
    p.exprs.push_back(e);
  }
  return p;
}

// the frame's [lo, hi) arrays; lo stays empty when the frame starts at the
// partition start (bg_window_agg reads d_part_start then)
struct WinFrameBufs {
  std::string key;
  DBufPtr lo, hi;
};

struct WinBounds {
  DBufPtr ps, pe, qs, qe;
  const uint32_t* u(const DBufPtr& b) const { return (const uint32_t*)b->p; }
};

static const WinFrameBufs& window_frame(const WinFrame& fr, const WinPlan& p,
                                        const Table& in, const WinBounds& b,
                                        std::vector<WinFrameBufs>& cache) {
  const std::string key = fr.text();
  for (auto& c : cache)
    if (c.key == key) return c;
  WinFrameBufs fb;
  fb.key = key;
  fb.lo = dalloc_elems(in.n, 4);
  fb.hi = dalloc_elems(in.n, 4);
  bg_column okey{};
  bool f64 = false;
  if (fr.range_offset()) {
    okey = to_bg(in.col(p.order[0].col), in.n);
    f64 = okey.dtype == BG_DT_FLOAT64;
  }
  auto off = [f64](const WinBound& w) {
    if (!f64) return w.i;
    int64_t bits;
    memcpy(&bits, &w.d, 8);
    return bits;
  };
  chk(bg_window_frame(fr.units, fr.start.kind, off(fr.start), fr.end.kind,
                      off(fr.end), fr.range_offset() ? &okey : nullptr,
                      !p.order.empty() && p.order[0].desc ? 1 : 0, b.u(b.ps),
                      b.u(b.pe), b.u(b.qs), b.u(b.qe), in.n,
                      (uint32_t*)fb.lo->p, (uint32_t*)fb.hi->p),
      "bg_window_frame");
  if (fr.start.kind == BG_WIN_UNBOUNDED) fb.lo = nullptr;
  cache.push_back(std::move(fb));
  return cache.back();
}

// one bg_window_agg call into a fresh column of dtype dt
static Col window_agg_col(int32_t fn, const Col* val, const DtSpec& dt,
                          const WinBounds& b, const WinFrameBufs& fb,
                          int64_t n) {
  Col c = make_col(dt);
  c.data = dalloc_elems(n, dt_size(dt.dt));
  if (fn != BG_WIN_COUNT) c.validity = alloc_bitmap(n);
  bg_column v{};
  if (val) v = to_bg(*val, n);
  chk(bg_window_agg(fn, val ? &v : nullptr, b.u(b.ps),
                    fb.lo ? (const uint32_t*)fb.lo->p : nullptr,
                    (const uint32_t*)fb.hi->p, n, c.data->p,
                    c.validity ? c.validity->u8() : nullptr),
      "bg_window_agg");
  return c;
}

static Table exec_window(const Value& node, Metrics& m) {
  Table in = exec_plan(node.at("input"), m);
  VSchema vs;
  vs.names = in.names;
  for (auto& c : in.cols) vs.dts.push_back(c.spec());
  const WinPlan p = plan_window(node, vs);
  const int64_t n = in.n;

  std::vector<bg_column> pcols, ocols;
  for (auto& k : p.part) pcols.push_back(to_bg(in.col(k), n));
  for (auto& k : p.order) ocols.push_back(to_bg(in.col(k.col), n));
  WinBounds b;
  for (DBufPtr* d : {&b.ps, &b.pe, &b.qs, &b.qe}) *d = dalloc_elems(n, 4);
  chk(bg_window_bounds(pcols.data(), (int32_t)pcols.size(), ocols.data(),
                       (int32_t)ocols.size(), n, (uint32_t*)b.ps->p,
                       (uint32_t*)b.pe->p, (uint32_t*)b.qs->p,
                       (uint32_t*)b.qe->p),
      "bg_window_bounds");

  // the aggregates' inputs: arithmetic fuses into one pass, as in
  // hash_aggregate
  std::vector<const Value*> vexprs;
  for (auto& e : p.exprs)
    if (e.expr) vexprs.push_back(e.expr);
  std::vector<Col> vcols;
  if (!vexprs.empty()) eval_exprs_fused(in, vexprs, &vcols);

  Table out = in;
  std::vector<WinFrameBufs> frames;
  size_t vi = 0;
  for (auto& e : p.exprs) {
    Col c;
    if (e.ranking) {
      c = make_col(DT_I64);
      c.data = dalloc_elems(n, 8);
      const int32_t fn = e.fn == "row_number" ? BG_WIN_ROW_NUMBER
                         : e.fn == "rank"     ? BG_WIN_RANK
                                              : BG_WIN_DENSE_RANK;
      chk(bg_window_rank(fn, b.u(b.ps), b.u(b.qs), n, (int64_t*)c.data->p),
          "bg_window_rank");
    } else {
      const Col* val = e.expr ? &vcols[vi++] : nullptr;
      const WinFrameBufs& fb = window_frame(e.frame, p, in, b, frames);
      if (e.fn == "avg") {
        // SUM and COUNT per row, then the hash aggregate's own finalisation
        // with one "group" per row
        const DtSpec sum_dt =
            agg_output_fields("sum", "single", e.as, e.in)[0].dt;
        Col s = window_agg_col(BG_WIN_SUM, val, sum_dt, b, fb, n);
        Col cnt = window_agg_col(BG_WIN_COUNT, val, DT_I64, b, fb, n);
        c = make_col(e.out);
        c.data = dalloc_elems(n, dt_size(e.out.dt));
        c.validity = alloc_bitmap(n, 0xFF);
        chk(bg_avg_finalize(s.data->p, dt_size(sum_dt.dt),
                            e.out.dt == BG_DT_FLOAT64 ? 1 : 0, cnt.data->p, 8,
                            4, n, c.data->p, c.validity->u8()),
            "bg_avg_finalize");
      } else {
        const int32_t fn = e.fn == "sum"     ? BG_WIN_SUM
                           : e.fn == "count" ? BG_WIN_COUNT
                           : e.fn == "min"   ? BG_WIN_MIN
                                             : BG_WIN_MAX;
        c = window_agg_col(fn, val, e.out, b, fb, n);
      }
    }
    out.names.push_back(e.as);
    out.cols.push_back(std::move(c));
  }
  return out;
}

static VSchema validate_plan(const Value& node) {
  const std::string op = node.get_str("op");
  if (op == "scan") {
    VSchema s;
    for (auto& f : node.get_arr("schema")) {
      s.names.push_back(f->get_str("name"));
      s.dts.push_back(parse_dtype(*f));
    }
    const std::string kind = node.at("source").get_str("kind");
    if (kind != "device" && kind != "shuffle" && kind != "ipc" &&
        kind != "raw" && kind != "parquet")
      throw StageError(BG_ERR_INVALID, "scan: unknown source kind " + kind);
    if (node.has("projection")) {
      VSchema p;
      for (auto& pr : node.get_arr("projection")) {
        int i = s.idx(pr->s);
        p.names.push_back(s.names[(size_t)i]);
        p.dts.push_back(s.dts[(size_t)i]);
      }
      return p;
    }
    return s;
  }
  if (op == "filter") {
    VSchema s = validate_plan(node.at("input"));
    if (node.has("any"))
      for (auto& grp : node.get_arr("any")) validate_predicates(s, grp->arr);
    else
      validate_predicates(s, node.get_arr("predicates"));
    return s;
  }
  if (op == "project") {
    VSchema in = validate_plan(node.at("input"));
    VSchema out;
    for (auto& ex : node.get_arr("exprs")) {
      out.names.push_back(ex->get_str("as"));
      out.dts.push_back(validate_expr(in, ex->at("expr")));
    }
    return out;
  }
  if (op == "hash_join" || op == "nested_loop_join") {
    VSchema b = validate_plan(node.at("build"));
    VSchema p = validate_plan(node.at("probe"));
    if (op == "hash_join") {
      for (auto& k : node.get_arr("build_keys")) b.idx(k->s);
      for (auto& k : node.get_arr("probe_keys")) p.idx(k->s);
    } else {
      refuse_join_keys(node);
    }
    const JoinKind& k = join_kind(node);
    if (node.has("filter")) validate_join_filter(op, b, p, node.at("filter"));
    VSchema out;
    for (auto& ov : node.get_arr("output")) {
      const JoinOut o = join_output(op, k, *ov);
      const VSchema& src = o.build ? b : p;
      out.dts.push_back(src.dts[(size_t)src.idx(o.col)]);
      out.names.push_back(o.as);
    }
    return out;
  }
  if (op == "hash_aggregate") {
    VSchema in = validate_plan(node.at("input"));
    const std::string mode = node.get_str_or("mode", "single");
    VSchema out;
    for (auto& k : node.get_arr("group_by")) {
      int i = in.idx(k->s);
      out.names.push_back(k->s);
      out.dts.push_back(in.dts[(size_t)i]);
    }
    for (auto& a : node.get_arr("aggs")) {
      const std::string fn = a->get_str("fn");
      const std::string as = a->get_str("as");
      check_agg_fn(fn);
      DtSpec src = DT_I64;  // the aggregate's input dtype (count: unused)
      if (mode == "final") {
        auto partial = agg_partial_names(fn, as);
        for (auto& name : partial) in.idx(name);
        src = in.dts[(size_t)in.idx(partial[0])];
      } else if (fn != "count" || a->has("expr")) {
        src = validate_expr(in, a->at("expr"));
      }
      // the executor's verdict on fn over this dtype (a final count sums
      // its Int64 partial counts, whatever it counted)
      const bool count_star = fn == "count" && !a->has("expr");
      if (!count_star && !(mode == "final" && fn == "count"))
        (void)agg_op_for(fn, src.dt);
      for (auto& f : agg_output_fields(fn, mode, as, src)) {
        out.names.push_back(f.name);
        out.dts.push_back(f.dt);
      }
    }
    return out;
  }
  if (op == "sort") {
    VSchema s = validate_plan(node.at("input"));
    for (auto& k : node.get_arr("keys")) s.idx(k->get_str("col"));
    return s;
  }
  if (op == "window") {
    VSchema s = validate_plan(node.at("input"));
    const WinPlan p = plan_window(node, s);
    for (auto& e : p.exprs) {
      s.names.push_back(e.as);
      s.dts.push_back(e.out);
    }
    return s;
  }
  if (op == "limit") return validate_plan(node.at("input"));
  throw StageError(BG_ERR_INVALID, "plan: unknown operator '" + op + "'");
}

static DtSpec validate_expr(const VSchema& s, const Value& e) {
  if (e.has("col")) return s.dts[(size_t)s.idx(e.get_str("col"))];
  if (e.has("lit")) return DT_LIT;
  if (e.has("case")) {
    const Value& c = e.at("case");
    validate_predicates(s, c.get_arr("when"));
    DtSpec a = validate_expr(s, c.at("then"));
    DtSpec b = validate_expr(s, c.at("else"));
    return a.dt == BG_DT_DECIMAL128 || b.dt != BG_DT_DECIMAL128 ? a : b;
  }
  if (e.has("lit_f64")) {
    lit_f64_value(e);
    return DT_F64;
  }
  if (e.has("cast")) {
    const Value& c = e.at("cast");
    const DtSpec to = cast_target(c);
    cast_check_pair(c, validate_expr(s, c.at("arg")), to);
    return to;
  }
  for (const char* k : {"mul", "add", "sub", "div"}) {
    if (e.has(k)) {
      auto& ops = e.get_arr(k);
      if (ops.size() != 2)
        throw StageError(BG_ERR_INVALID,
                         std::string(k) + ": two operands required");
      DtSpec a = validate_expr(s, *ops[0]);
      DtSpec b = validate_expr(s, *ops[1]);
      const ArithPlan p = arith_plan(k, e, *ops[0], a, *ops[1], b);
      if (p.kind != ArithPlan::DEC128) return p.out;
      int scale = strcmp(k, "mul") == 0 ? a.scale + b.scale
                                        : (a.dt == BG_DT_DECIMAL128 ? a.scale
                                                                    : b.scale);
      return {BG_DT_DECIMAL128, 38, scale};
    }
  }
  if (e.has("date_part")) {
    const Value& d = e.at("date_part");
    date_part_code(d.get_str("part"));
    const DtSpec a = validate_expr(s, d.at("arg"));
    if (a.dt != BG_DT_DATE32)
      throw StageError(BG_ERR_INVALID,
                       "date_part: argument '" + expr_label(d.at("arg")) +
                           "' is " + dtype_name(a.dt) + ", date32 required");
    return {BG_DT_INT32, 0, 0};
  }
  if (e.has("substr")) {
    const Value& d = e.at("substr");
    const DtSpec a = validate_expr(s, d.at("arg"));
    const std::string arg = expr_label(d.at("arg"));
    if (a.dt != BG_DT_UTF8)
      throw StageError(BG_ERR_INVALID, "substr: argument '" + arg + "' is " +
                                           dtype_name(a.dt) +
                                           ", utf8 required");
    for (const char* k : {"start", "count"})
      if (d.has(k) && d.at(k).kind != Value::INT)
        throw StageError(BG_ERR_UNSUPPORTED,
                         std::string("substr: '") + k + "' of '" + arg +
                             "' must be an integer literal");
    d.get_int("start");
    if (d.has("count") && d.get_int("count") < 0)
      throw StageError(BG_ERR_INVALID,
                       "substr: negative substring length not allowed "
                       "(count " + std::to_string(d.get_int("count")) +
                           " on '" + arg + "')");
    return {BG_DT_UTF8, 0, 0};
  }
  throw StageError(BG_ERR_INVALID, "plan: unknown expression node");
}

static VSchema validate_root(const Value& doc) {
  const Value& root = doc.at("plan");
  const std::string op = root.get_str("op");
  if (op == "sort_shuffle_write") {
    doc.at("work_dir");
    doc.at("job_id");
    root.get_int("k");
    VSchema in = validate_plan(root.at("input"));
    for (auto& ke : root.get_arr("keys")) validate_expr(in, *ke);
    if (!doc.has("schema_msg_hex"))
      throw StageError(BG_ERR_INVALID,
                       "sort_shuffle_write requires schema_msg_hex (the "
                       "Arrow schema message bytes from the host)");
    return in;
  }
  if (op == "passthrough_write") {
    doc.at("work_dir");
    root.get_int("global_partition");
    if (!doc.has("schema_msg_hex"))
      throw StageError(BG_ERR_INVALID, "passthrough_write requires "
                                       "schema_msg_hex");
    return validate_plan(root.at("input"));
  }
  if (op == "collect") return validate_plan(root.at("input"));
  throw StageError(
      BG_ERR_INVALID,
      "stage root must be sort_shuffle_write / passthrough_write / collect");
}

}  // namespace bgstage

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------

using namespace bgstage;

static char* dup_out(const std::string& s) {
  char* p = (char*)malloc(s.size() + 1);
  memcpy(p, s.c_str(), s.size() + 1);
  return p;
}

extern "C" void bg_stage_free(char* p) { free(p); }

extern "C" int bg_stage_validate(const char* plan_json, char** out_json) {
  try {
    bgjson::Parser parser(plan_json);
    ValuePtr doc = parser.parse();
    VSchema s = validate_root(*doc);
    bgjson::Writer w;
    w.raw("{\"ok\":true,\"schema\":[");
    for (size_t i = 0; i < s.names.size(); ++i) {
      if (i) w.raw(",");
      w.raw("{\"name\":");
      w.str(s.names[i]);
      w.raw(",\"dtype\":");
      w.str(dtype_name(s.dts[i].dt));
      if (s.dts[i].dt == BG_DT_DECIMAL128) {  // as the collect root spells it
        w.raw(",\"precision\":");
        w.num(s.dts[i].precision);
        w.raw(",\"scale\":");
        w.num(s.dts[i].scale);
      }
      w.raw("}");
    }
    w.raw("]}");
    if (out_json) *out_json = dup_out(w.out);
    return BG_OK;
  } catch (const StageError& e) {
    return bg_set_error(e.code, e.what());
  } catch (const std::exception& e) {
    return bg_set_error(BG_ERR_INVALID, e.what());
  }
}

extern "C" int bg_execute_stage(const char* plan_json, char** out_json) {
  try {
    bgjson::Parser parser(plan_json);
    ValuePtr doc = parser.parse();
    (void)validate_root(*doc);  // fail fast with a typed message

    auto t0 = Clock::now();
    Metrics m;
    bgjson::Writer res;
    res.raw("{");
    const Value& root = doc->at("plan");
    const std::string op = root.get_str("op");
    if (op == "sort_shuffle_write")
      exec_sort_shuffle_write(root, *doc, m, res);
    else if (op == "passthrough_write")
      exec_passthrough_write(root, *doc, m, res);
    else
      exec_collect(root, m, res);
    chk(bg_synchronize(), "bg_synchronize");
    int64_t total_ns = ns_since(t0);
    // metric names mirror the reference writer's MetricsSet
    // (sort_shuffle/writer.rs:328-440) + the GPU counters of SURVEY.md §5
    res.raw(",\"metrics\":{\"repart_time_ns\":");
    res.num(m.repart_time_ns);
    res.raw(",\"write_time_ns\":");
    res.num(m.write_time_ns);
    res.raw(",\"scan_time_ns\":");
    res.num(m.scan_time_ns);
    res.raw(",\"stage_time_ns\":");
    res.num(total_ns);
    res.raw(",\"spill_time_ns\":0,\"spill_count\":0,\"spilled_bytes\":0");
    res.raw(",\"output_rows\":");
    res.num(m.output_rows);
    res.raw(",\"gpu_kernel_ms\":");
    res.dbl(m.kernel_ms);
    res.raw("}}");
    if (out_json) *out_json = dup_out(res.out);
    return BG_OK;
  } catch (const StageError& e) {
    return bg_set_error(e.code, e.what());
  } catch (const std::exception& e) {
    return bg_set_error(BG_ERR_INVALID, e.what());
  }
}

extern "C" int bg_stage_register_table(const char* name,
                                       const bg_column* cols,
                                       const char* const* col_names,
                                       int32_t ncols, int64_t n_rows) {
  try {
    Table t;
    t.n = n_rows;
    for (int32_t c = 0; c < ncols; ++c) {
      Col col = make_col({cols[c].dtype, cols[c].precision, cols[c].scale});
      col.ext_data = cols[c].d_data;
      col.ext_valid = cols[c].d_validity;
      col.ext_offs = cols[c].d_offsets;
      if (col.dtype == BG_DT_UTF8 && col.ext_offs) {
        // cache the payload length (last offset) for gather sizing
        int32_t last = 0;
        chk(bg_memcpy_d2h(&last, (const uint8_t*)cols[c].d_offsets +
                                     4 * n_rows, 4),
            "bg_memcpy_d2h");
        col.data_bytes = last;
      }
      t.cols.push_back(std::move(col));
      t.names.push_back(col_names[c]);
    }
    std::lock_guard<std::mutex> g(g_tables_mu);
    g_tables[name] = std::move(t);
    return BG_OK;
  } catch (const StageError& e) {
    return bg_set_error(e.code, e.what());
  } catch (const std::exception& e) {
    return bg_set_error(BG_ERR_INVALID, e.what());
  }
}

extern "C" int bg_stage_unregister_table(const char* name) {
  std::lock_guard<std::mutex> g(g_tables_mu);
  g_tables.erase(name);
  return BG_OK;
}

// test-only: expose the C++ RecordBatch metadata builder so CPU tests can
// pin it byte-for-byte against the Python ipc.py builder (itself validated
// by pyarrow round-trips).  nodes: (length, null_count) pairs; bufs:
// (offset, length) pairs.  *out receives malloc'd hex.
extern "C" int bg_debug_rb_message(int64_t n_rows, const int64_t* nodes,
                                   int32_t nnodes, const int64_t* bufs,
                                   int32_t nbufs, int64_t body_len,
                                   int32_t compressed, char** out) {
  try {
    std::vector<bgipc::FieldNode> nd;
    for (int32_t i = 0; i < nnodes; ++i)
      nd.push_back({nodes[2 * i], nodes[2 * i + 1]});
    std::vector<bgipc::BufSpec> bf;
    for (int32_t i = 0; i < nbufs; ++i)
      bf.push_back({bufs[2 * i], bufs[2 * i + 1]});
    std::string msg = bgipc::record_batch_message(n_rows, nd, bf, body_len,
                                                  compressed != 0);
    static const char* hexd = "0123456789abcdef";
    std::string hex;
    hex.reserve(msg.size() * 2);
    for (unsigned char c : msg) {
      hex += hexd[c >> 4];
      hex += hexd[c & 15];
    }
    *out = dup_out(hex);
    return BG_OK;
  } catch (const std::exception& e) {
    return bg_set_error(BG_ERR_INVALID, e.what());
  }
}
