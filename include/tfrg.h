/* tfrg.h — C-ABI of libtfrg, the MI355X TFRecord -> tf.train.Example -> Feature decode path.
 *
 * Plain pointers and sizes only (no torch / HIP types): the Python host mirror binds it with
 * ctypes (which releases the GIL), see INTEGRATION.md for the binding stubs. Every entry point
 * cites the reference interface (kmkolasinski/tfrecords-reader v1.1.0) whose work it replaces.
 *
 * Return convention: int functions return 0 on success and a negative TFRG_E_* code on a runtime
 * failure (HIP error, bad argument, allocation). Per-record DATA errors are never return codes:
 * they are the per-record int32 status column (include/tfrg_status.h), mirroring the exception the
 * reference would raise for that record.
 */
#ifndef TFRG_H
#define TFRG_H
#include <stdint.h>
#include "tfrg_status.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TFRG_ABI_VERSION 1

/* runtime error codes (return values) */
#define TFRG_E_ARG (-1)
#define TFRG_E_HIP (-2)
#define TFRG_E_NOMEM (-3)
#define TFRG_E_IO (-4)
#define TFRG_E_LIMIT (-5)

/* decode flags */
#define TFRG_FLAG_PAYLOAD_ONLY 1u /* ranges are bare Example payloads (decode(raw) semantics)   */
#define TFRG_FLAG_SPEC_VARINT 2u  /* protobuf-spec int64 varints instead of the reference's
                                     int-width shift (decoder.pyx:44)               */
#define TFRG_FLAG_NO_CRC 4u       /* skip the CRC-32C verdicts. Record-shape templates still apply:
                                     a record matching one under its mask takes it whatever its
                                     CRCs (verdict TFRG_V_LEN_MATCH)                              */
#define TFRG_FLAG_STRICT_CRC 8u   /* a record whose length field or either masked CRC-32C does not
                                     match fails with TFRG_ERR_CRC (no values) instead of only
                                     clearing its verdict bits; overrides TFRG_FLAG_NO_CRC      */
#define TFRG_FLAG_MATERIALIZE_BYTES 16u /* also gather every bytes_list element's payload into a
                                     contiguous device byte column (tfrg_columns.bytes_data) with
                                     u64 offsets (bytes_offsets); default: (offset, len) views  */

int tfrg_abi_version(void);
/* Per-record status (tfrg_status.h) -> the reference's exception: its Python type name ("Exception",
 * "UnicodeDecodeError", "AttributeError", "OSError", ...) and message text, literal for the
 * decoder.pyx:49-297 exceptions ("Unsupported wire type: <aux>" for TFRG_ERR_WIRE_TYPE). The
 * message pointer is thread-local storage, valid until the next call on the thread. */
const char* tfrg_status_exception(int status);
const char* tfrg_status_message(int status, int64_t aux);
/* message of the last runtime failure on this thread */
const char* tfrg_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * Host framing index (replaces cython/indexer.pyx:212-252 create_tfrecord_pointers_index).
 * Pointers are (start, end, example_size) u64 triples, end = start + 16 + size; bit-exact with the
 * reference, including its acceptance of a last record that runs past EOF.
 * ------------------------------------------------------------------------------------------- */
/* over an in-memory file image; writes up to cap triples, returns the record count */
int64_t tfrg_index_buffer(const uint8_t* file, uint64_t size, uint64_t* out_triples, int64_t cap);
/* mmap + index; *out_triples is malloc'd (free with tfrg_free) */
int tfrg_index_file(const char* path, uint64_t** out_triples, int64_t* n);
/* .idx cache file, indexer.pyx:260-328: native size_t n, then n x {u64 start, end, size} */
int tfrg_idx_save(const char* idx_path, const uint64_t* triples, int64_t n);
int tfrg_idx_load(const char* idx_path, uint64_t** out_triples, int64_t* n);
void tfrg_free(void* p);
/* Host staging of a selection (reader.py:212-247 load_records): copies the n byte ranges
 * [starts[i], ends[i]) of src back to back into dst (NULL: only sizes them); returns the total. */
uint64_t tfrg_gather_ranges(const uint8_t* src, const uint64_t* starts, const uint64_t* ends, int64_t n,
                            uint8_t* dst);
/* Key discovery before a device decode (no reference counterpart: the keys and kinds that
 * decoder.pyx:130-199 would meet). Parses the Example -> Features -> map entries of the n records
 * [start[i], end[i]) of bytes (framed, or bare payloads with TFRG_FLAG_PAYLOAD_ONLY) and writes up
 * to cap distinct (key offset, key length, kind) u64 triples: absolute key offsets into bytes, kind =
 * the field number of the entry's Feature (1 bytes_list, 2 float_list, 3 int64_list). Only canonical
 * records seed (Example = features fields, each map entry = key then value, each Feature = one list
 * field); any other record is left to the device decode's schema-miss pass, which follows the
 * reference's semantics. Returns the triple count. Seeding the key table with them spares a first
 * decode the exact walker's schema-miss pass. */
int64_t tfrg_scan_keys(const uint8_t* bytes, uint64_t nbytes, const uint64_t* start, const uint64_t* end, int64_t n,
                       uint32_t flags, uint64_t* out_triples, int64_t cap);

/* Compressed TFRecord files (TensorFlow TFRecordOptions "ZLIB" / "GZIP": the whole framed stream
 * deflated; claimed by the reference's README.md:14, not implemented there). tfrg_compression_of
 * classifies a file image: an image whose length chain tiles it exactly is uncompressed, else a
 * gzip / zlib header selects that format. tfrg_inflate decodes either (concatenated gzip members
 * included) into a malloc'd buffer (free with tfrg_free); the framing index is then built over it. */
#define TFRG_COMPRESSION_NONE 0
#define TFRG_COMPRESSION_ZLIB 1
#define TFRG_COMPRESSION_GZIP 2
int tfrg_compression_of(const uint8_t* image, uint64_t size);
int tfrg_inflate(const uint8_t* in, uint64_t size, uint8_t** out, uint64_t* out_len);

/* CRC-32C (Castagnoli) and the TFRecord mask (absent from the reference) */
uint32_t tfrg_crc32c(const uint8_t* p, uint64_t n);
uint32_t tfrg_masked_crc32c(const uint8_t* p, uint64_t n);
/* TFRecord writer framing: n payloads (concatenated, offsets[n+1]) -> framed bytes with spec CRCs
 * (crc != 0) or the zero CRCs the reference's test writers use (tests/utils.py:31-36).
 * Returns the framed size; writes only if out_cap suffices. */
int64_t tfrg_frame_records(const uint8_t* payloads, const uint64_t* offsets, int64_t n, int crc,
                           uint8_t* out, int64_t out_cap);

/* ---------------------------------------------------------------------------------------------
 * Device decode (replaces cython/decoder.pyx:107 example_from_bytes per record, batched).
 * One context per (device, host thread); calls on one context are serialised by the caller.
 * ------------------------------------------------------------------------------------------- */
typedef struct tfrg_ctx tfrg_ctx;

int tfrg_ctx_create(int device, tfrg_ctx** out);
int tfrg_ctx_destroy(tfrg_ctx* ctx);
/* records larger than lane_max bytes take the wavefront-per-record kernels (default 2048) */
int tfrg_ctx_set_lane_max(tfrg_ctx* ctx, uint32_t lane_max);
/* An upper bound on (end - start) of the records of the following tfrg_decode_device calls (0 =
 * unknown, the default). With a bound <= lane_max the batch has no large records and their count
 * kernel is not launched (a few microseconds per decode); a wrong bound still decodes correctly
 * (such records take the lane kernel's slower path). tfrg_decode_host derives it per call. */
int tfrg_ctx_set_record_bound(tfrg_ctx* ctx, uint64_t max_record_bytes);
/* Value-capacity hints: the int64 / float / bytes_list values the following decodes are expected to
 * produce at most (0 = unknown, the default: the worst case one int64 per input byte, one float per
 * 4 bytes, one bytes element per 2 -- about 13 x the batch's bytes of device memory). A decode whose
 * values exceed a hint is re-run with the worst case inside tfrg_result_info before it returns (the
 * results are always complete); tfrg_ctx_device_bytes counts those re-runs. */
int tfrg_ctx_set_value_caps(tfrg_ctx* ctx, uint64_t int64_values, uint64_t float_values, uint64_t bytes_values);
/* device memory held by the context (bytes) and the decodes re-run so far: a value-capacity hint was
 * too small, or an optimistic decode left records (tfrg_result_info) */
int tfrg_ctx_device_bytes(tfrg_ctx* ctx, uint64_t* bytes, uint64_t* hint_reruns);
/* wavefront records spanning <= nbytes are staged in LDS (clamped to the kernel's 12 KiB stage;
 * 0 routes every wavefront record to the streaming kernels). A tuning/testing knob. */
int tfrg_ctx_set_wave_stage(tfrg_ctx* ctx, uint32_t nbytes);
/* chunk size of tfrg_index_device: a power of two from 64 to 65536, 0 = the default (4096). A
 * tuning/testing knob: with small chunks small images exercise the multi-chunk logic. */
int tfrg_ctx_set_index_chunk(tfrg_ctx* ctx, uint32_t bytes);

/* Record-shape templates (no reference counterpart: a fast path under decoder.pyx:107-300). Up to
 * TFRG_TPL_MAX shapes of canonical records (payload <= TFRG_TPL_MAX_PAYLOAD bytes, at most
 * TFRG_TPL_MAX_ENTRIES feature entries) -- every byte fixed except list contents, incl. the
 * continuation bits of packed int64 lists -- are learned from up to TFRG_TPL_SAMPLE host records
 * spread over the batch, the most frequent shapes first (a shape seen once in a sample of >= 256 is
 * not kept; with payloads over 112 bytes the lane image holds at most 30, the LDS beside the CRC
 * tables). A framed record equal to a template under its mask, with matching length field and CRCs,
 * gets the template's dict without a walk (its values are still read from the record; k_tpl_lane,
 * schemas of <= TFRG_TPL_MAX_SLOTS slots); any other record takes the canonical walk. A shape is kept
 * per frame class (tfrg_template_frames): records whose two CRC fields are 0 match a template of
 * their own, and with TFRG_FLAG_NO_CRC the CRCs play no part in the match.
 * Learned automatically from the first tfrg_decode_host batch after each tfrg_set_schema; device-only
 * callers pass a host sample here. Returns the number of templates (0..TFRG_TPL_MAX). With no shape
 * kept, the slots that are one inline value in every sampled record (host decode) are still learned
 * for speculative placement (the optimistic decode of large single-value records).
 * tfrg_ctx_set_templates(ctx, 0) disables the match (env TFRG_TEMPLATES=0); the speculative
 * placement of slots that are one inline value in every learned shape stays on. */
#define TFRG_TPL_MAX 32
#define TFRG_TPL_MAX_PAYLOAD 240
#define TFRG_TPL_MAX_ENTRIES 16
#define TFRG_TPL_MAX_SLOTS 16
#define TFRG_TPL_SAMPLE 4096
int tfrg_learn_templates(tfrg_ctx* ctx, const uint8_t* h_bytes, uint64_t nbytes, const uint64_t* h_start,
                         const uint64_t* h_end, uint32_t n, uint32_t flags);
int tfrg_template_count(tfrg_ctx* ctx);
/* The frame classes of the kept templates, a bit mask: bit 0 -- spec-framed (length and data CRC
 * fields hold the spec masked CRC-32C), bit 1 -- unchecked-framed (both CRC fields 0, as the
 * reference's test writers leave them: such a record takes its template with verdict
 * TFRG_V_LEN_MATCH). A sample with both kinds keeps a shape once per class. 0: no templates. */
int tfrg_template_frames(tfrg_ctx* ctx);
/* The learned templates in their window form (u32 words, layout in csrc/tfrg_layout.h): up to cap
 * words into out, the window size W (words) into *window_words; returns the template count. For
 * checking a template against records on the host. */
int tfrg_template_words(tfrg_ctx* ctx, uint32_t* out, uint64_t cap, uint32_t* window_words);
/* Host only (no device): the templates tfrg_learn_templates would learn for the given key table
 * (as tfrg_set_schema) from the given records, in window form into out; returns their count. */
int tfrg_learn_templates_host(uint32_t n_keys, const uint8_t* key_blob, const uint64_t* key_offsets,
                              const uint32_t* key_flags, uint32_t n_slots, const uint32_t* slot_key,
                              const uint8_t* slot_kind, const uint8_t* h_bytes, uint64_t nbytes,
                              const uint64_t* h_start, const uint64_t* h_end, uint32_t n, uint32_t flags,
                              uint32_t* out, uint64_t cap, uint32_t* window_words);
int tfrg_ctx_set_templates(tfrg_ctx* ctx, int on);

/* Per-kernel timing: with profiling on, every decode records HIP events on its stream around
 * each kernel stage; tfrg_profile_last waits for the last decode and writes up to cap stage
 * durations (ms) and names, returning the stage count. */
int tfrg_ctx_set_profiling(tfrg_ctx* ctx, int on);
int tfrg_profile_last(tfrg_ctx* ctx, float* ms, const char** names, int cap);

/* Key table ("schema"): n_keys distinct key byte strings (key_blob[key_offsets[i]..[i+1]]),
 * key_flags bit0 = the bytes are not valid UTF-8 (decoder.pyx:164 would raise); n_slots columns,
 * slot s = (slot_key[s], slot_kind[s]) with kind 1 bytes_list, 2 float_list, 3 int64_list.
 * Records whose keys are not all in the table finish with status TFRG_ST_SCHEMA_MISS and list the
 * missing (key, kind) pairs (tfrg_result_misses): intern them and decode again. */
int tfrg_set_schema(tfrg_ctx* ctx, uint32_t n_keys, const uint8_t* key_blob, const uint64_t* key_offsets,
                    const uint32_t* key_flags, uint32_t n_slots, const uint32_t* slot_key,
                    const uint8_t* slot_kind);

/* ---------------------------------------------------------------------------------------------
 * Host decode of ONE payload (replaces cython/decoder.pyx:107 example_from_bytes for single
 * records: the "cython" decoder type, and the one-record calls decode(raw) / example_from_bytes /
 * ds[i] of the "hip" type, far below the device's launch latency). The reference's exact
 * semantics (error precedence, dict rules, varint compat mode unless TFRG_FLAG_SPEC_VARINT) on the
 * calling thread; no device, no schema. One context per host thread.
 * ------------------------------------------------------------------------------------------- */
typedef struct tfrg_host_ctx tfrg_host_ctx;
typedef struct tfrg_host_record {
  int32_t status;            /* tfrg_status of the record (0 = ok), as the device's status column */
  uint32_t n_entries;        /* dict entries (status 0), in the reference's dict order */
  int64_t aux;               /* error detail, as the device's aux column */
  const uint32_t* key_off;   /* entry e's key: payload bytes [key_off[e], key_off[e] + key_len[e]) */
  const uint32_t* key_len;
  const uint8_t* kind;       /* tfrg_kind of entry e */
  const uint32_t* val_off;   /* entry e's values: [val_off[e], val_off[e] + val_cnt[e]) of its kind's array */
  const uint32_t* val_cnt;
  const int64_t* i64;
  const uint32_t* f32;       /* raw bits */
  const uint32_t* b_off;     /* bytes elements: payload-relative (offset, length) */
  const uint32_t* b_len;
} tfrg_host_record;
int tfrg_host_ctx_create(tfrg_host_ctx** out);
int tfrg_host_ctx_destroy(tfrg_host_ctx* ctx);
/* Decodes payload[0, len) into *out (arrays owned by ctx, valid until its next call). Returns 0 or a
 * TFRG_E_* code; data errors are out->status. */
int tfrg_host_decode(tfrg_host_ctx* ctx, const uint8_t* payload, uint64_t len, uint32_t flags, tfrg_host_record* out);

/* Asynchronous decode of n records [start[i], end[i]) of a device buffer (framed TFRecords unless
 * TFRG_FLAG_PAYLOAD_ONLY). d_bytes must stay readable up to round_up(nbytes, 16) and nbytes must be
 * < 2^32 (split larger batches). d_start/d_end are device arrays. stream: hipStream_t or NULL for
 * the context's own stream. Results stay valid until the next decode on this context. */
int tfrg_decode_device(tfrg_ctx* ctx, const uint8_t* d_bytes, uint64_t nbytes, const uint64_t* d_start,
                       const uint64_t* d_end, uint32_t n, uint32_t flags, void* stream);
/* Same with 32-bit offsets (a batch is < 4 GiB, so offsets relative to d_bytes fit; the index's
 * (tfrecord_start, tfrecord_end) of indexer.pyx:212-252 rebased per batch). d_start32 == NULL: the
 * records lie back to back -- record 0 starts at first_start and record i > 0 where record i - 1
 * ends, as the framing index of a file image or a gathered selection always gives them -- and
 * only their u32 ends are read (4 bytes per record instead of 16). Results are those of
 * tfrg_decode_device on the same ranges. */
int tfrg_decode_device32(tfrg_ctx* ctx, const uint8_t* d_bytes, uint64_t nbytes, const uint32_t* d_start32,
                         const uint32_t* d_end32, uint32_t first_start, uint32_t n, uint32_t flags, void* stream);
/* Same from host memory: stages bytes/start/end into context-owned HBM (H2D on the stream). */
int tfrg_decode_host(tfrg_ctx* ctx, const uint8_t* h_bytes, uint64_t nbytes, const uint64_t* h_start,
                     const uint64_t* h_end, uint32_t n, uint32_t flags, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Framing index on the device (the walk of indexer.pyx:212-252, as tfrg_index_buffer runs it on the
 * host, for file images that are already in HBM). d_bytes[0, nbytes) holds n_pieces images back to
 * back (sum(piece_sizes) == nbytes < 2^32), readable to round_up(nbytes, 16) + 16. With fallback == 0
 * the rows written are bit for bit those of the host walk over every piece, shifted by the piece's
 * offset in the batch: a last record running past its piece is indexed, a tail of fewer than 8 bytes
 * ends a piece, a header of 8..11 bytes at the tail is a record, len + 4 is taken as int64 and a
 * seek that overflows or lands below 0 ends the piece after its record, start + 16 + len wraps in
 * u64. The one difference: a length whose seek lands at or before its own record's start reports
 * TFRG_INDEX_FB_SEEK (the host walk goes on from there and need not terminate).
 * The pieces are cut into chunks that are walked in parallel from guessed entries; the chain of
 * chunks from each piece's start is then verified and wrong guesses are re-walked, for a bounded
 * number of rounds (TFRG_INDEX_FB_ROUNDS if mismatches remain). Up to cap rows are written to
 * d_start / d_end / d_end32 (device, each may be NULL); piece_records (host, [n_pieces] or NULL)
 * receives the records per piece. One host synchronisation: the summary comes back in one small D2H
 * on stream (NULL: the context's). Scratch is the context's (tfrg_ctx_device_bytes counts it); the
 * last decode's result is untouched. TFRG_E_ARG: nbytes >= 2^32, sizes that do not sum to nbytes, a
 * NULL info. n_pieces == 0 or nbytes == 0: 0 records, nothing launched.
 * ------------------------------------------------------------------------------------------- */
#define TFRG_INDEX_FB_ROUNDS 1u
#define TFRG_INDEX_FB_SEEK 2u
typedef struct tfrg_index_info {
  uint64_t n_records;       /* records of all pieces (may exceed cap: only cap rows are written) */
  uint32_t fallback;        /* 0: the columns are exact. TFRG_INDEX_FB_ROUNDS: not proven within the
                               repair bound. TFRG_INDEX_FB_SEEK: a length field seeks backwards.
                               Nonzero: outputs undefined, index on the host */
  uint32_t tiled;           /* 1: start[i] == end[i-1] for every i > 0 and every end < 2^32
                               (d_end32 + first_start may drive tfrg_decode_device32 without starts) */
  uint32_t first_start;
  uint32_t n_chunks, repaired_chunks, repair_rounds;   /* diagnostics */
} tfrg_index_info;
int tfrg_index_device(tfrg_ctx* ctx, const uint8_t* d_bytes, uint64_t nbytes, const uint64_t* piece_sizes,
                      uint32_t n_pieces, uint64_t* d_start, uint64_t* d_end, uint32_t* d_end32, uint64_t cap,
                      uint64_t* piece_records, void* stream, tfrg_index_info* info);

typedef struct tfrg_info {
  uint32_t n_records;
  uint32_t n_slots;
  uint32_t n_errors;        /* records whose status is a decode error           */
  uint32_t first_error;     /* lowest such record index, 0xffffffff if none      */
  uint32_t n_miss_records;  /* records with TFRG_ST_SCHEMA_MISS                   */
  uint32_t n_miss_entries;  /* missing (key, kind) entries reported (may exceed the list capacity) */
  uint32_t n_big;           /* records decoded by the wavefront-per-record kernels */
  uint32_t scan_timeout;    /* must be 0                                          */
  uint64_t kind_totals[4];  /* values per kind: [1] bytes elements, [2] floats, [3] int64s */
  uint64_t nbytes;
  uint64_t bytes_data_len;  /* TFRG_FLAG_MATERIALIZE_BYTES: bytes in the byte column, else 0   */
  uint32_t tpl_groups_missed; /* 64-record groups with a record no record-shape template took */
  /* TFRG_IMPLICIT_* bits: columns an optimistic decode (tfrg_result_info) did not store because every
   * record of the batch took a record shape: STATUS -- every status 0 (aux unused) and every verdict
   * TFRG_V_LEN_MATCH | TFRG_V_LEN_CRC | TFRG_V_DATA_CRC; ORDER -- every slot's order word is the
   * same for every record (its key position in the shapes); BYTES_LEN -- every bytes_list slot holds
   * one element per record whose length is the same in every shape (the bytes_len column is that
   * constant; not with TFRG_FLAG_MATERIALIZE_BYTES). tfrg_result_fetch fills them into the
   * caller's buffers on the host (no copy), tfrg_result_device into the device columns (once per
   * decode, on the decode's stream, before it returns the view). */
  uint32_t implicit_cols;
  /* bit k: slot k (< 64) holds exactly one value per record, at row r of its column (final
   * speculative placement). Its row splits are the identity 0..n: the decode does not store them;
   * tfrg_result_fetch writes them into the caller's buffer, and tfrg_result_device into the device
   * columns (one small kernel on the decode's stream, before it returns the view). */
  uint64_t placed_slots;
  /* bit k: the last decode did not store slot k's bytes_off words. Slot k is a bytes_list slot that
   * holds one element per record at the same distance from the record's end in every record shape,
   * so element r of the slot's column is d_end32[r] + delta, with d_end32 the u32 ends the caller
   * passed to tfrg_decode_device32 and delta = tfrg_ctx_rel_off(ctx, k) (negative). Set only by an
   * optimistic decode (tfrg_result_info) with u32 offsets and without TFRG_FLAG_MATERIALIZE_BYTES;
   * a u64 or host decode, a re-run decode and env TFRG_IMPLICIT_OFF=0 at context creation store
   * every word (mask 0). tfrg_result_device writes the words into the device column (one small
   * kernel per masked slot on the decode's stream, once per decode) and tfrg_result_fetch copies
   * them from there; tfrg_result_dense / _dense_rows / _ragged_rows read d_end32 instead of the
   * column and write nothing.
   * Lifetime: while a result with a nonzero mask is read (tfrg_result_fetch, tfrg_result_device,
   * dense / dense_rows / ragged over a bytes slot), the d_end32 array of its decode must stay in
   * place and unchanged, until the next decode on the context -- exactly as d_bytes must stay for
   * the bytes views and for the confirmation of the decode. */
  uint64_t implicit_off_slots;
} tfrg_info;

/* The end-relative element offset of bytes slot `slot` in the context's learned record shapes
 * (tfrg_info.implicit_off_slots): *delta such that the slot's element of a record ending at e lies at
 * e + *delta. TFRG_E_ARG if the slot is not at one end-relative position in every learned shape. */
int tfrg_ctx_rel_off(const tfrg_ctx* ctx, uint32_t slot, int32_t* delta);

/* Waits for the last decode and returns its summary. Optimistic decodes: when the context's record
 * shapes took their whole learning sample, every slot is a single value and no record can exceed
 * lane_max (tfrg_ctx_set_record_bound), a decode is launched as the template pass alone plus one
 * bookkeeping kernel; this call confirms that every record took a shape, or re-runs the same decode
 * with every pass before it returns (its inputs must still be in place: the decode is not complete
 * before this call, tfrg_result_fetch or tfrg_result_device). Env TFRG_OPTIMISTIC=0 at context
 * creation turns it off. */
int tfrg_result_info(tfrg_ctx* ctx, tfrg_info* info);

/* Columnar result. Per record: status/aux/verdict. Per slot s (row-major [n_slots][n]):
 * order (0 absent, else 1 + the key's position in the record's dict), row_splits [n_slots][n+1]
 * (element offsets inside the slot's column), slot_base [n_slots] (column start inside its kind's
 * value array). Values: int64, float bits, bytes views (absolute offset into the input buffer,
 * length). miss: [min(n_miss_entries, cap)][4] = (record, kind, key offset, key length). */
typedef struct tfrg_columns {
  int32_t* status;
  int64_t* aux;
  uint8_t* verdict;
  uint16_t* order;
  uint32_t* row_splits;
  uint64_t* slot_base;
  int64_t* i64;
  uint32_t* f32;
  uint32_t* bytes_off;
  uint32_t* bytes_len;
  uint32_t* miss;
  /* TFRG_FLAG_MATERIALIZE_BYTES only: element e of the bytes values is
   * bytes_data[bytes_offsets[e] .. bytes_offsets[e + 1]) (kind_totals[1] + 1 offsets) */
  uint8_t* bytes_data;
  uint64_t* bytes_offsets;
} tfrg_columns;

/* device pointers of the last result (valid until the next decode / destroy). Asynchronous: the
 * columns are complete once the decode's stream reaches this call (it enqueues the identity row
 * splits of the placed slots there, once per decode). After an optimistic decode (tfrg_result_info)
 * it first synchronizes the decode's stream to confirm it, re-running it in full if needed. */
int tfrg_result_device(tfrg_ctx* ctx, tfrg_columns* cols);
/* copy the last result into caller host buffers sized from tfrg_info; NULL members are skipped */
int tfrg_result_fetch(tfrg_ctx* ctx, const tfrg_columns* host);

/* ---------------------------------------------------------------------------------------------
 * Dense device tensors from the last result (the tf.io.parse_example FixedLenFeature / padded VarLen
 * step the reference's users run after decoder.pyx:107; no reference counterpart). One kernel on the
 * decode's stream writes, for every spec, out[r][j] for r < n, j < width:
 *   int64_list / float_list slot: the record's value j if it has one, else fill (TFRG_DENSE_I64;
 *     TFRG_DENSE_I32: the low 32 bits of the int64; TFRG_DENSE_F32: the float's raw bits);
 *     lengths[r] = the record's value count;
 *   bytes_list slot (TFRG_DENSE_U8): byte j of element 0 of the record's list if it has one, else
 *     fill; lengths[r] = that element's byte length (0: the list is empty or absent).
 * d_stats (device, [n_specs][4] u32, or NULL; zeroed by the call on the stream): records whose
 * count (bytes: length) is > width (truncated), < width (padded), records without a value, and, for
 * bytes slots, records with more than one element.
 * The result is a function of the columns tfrg_result_fetch returns. An optimistic or hinted decode
 * is confirmed first, as by tfrg_result_device (the only host synchronisation); the implicit columns
 * and the identity row splits of placed slots are neither written nor read, and a later
 * tfrg_result_device / tfrg_result_fetch still gives the full view. Any number of calls per decode.
 * Stream order: the decode's stream waits for the work queued on consumer_stream so far (the
 * caller's allocator may have work pending on the outputs), and consumer_stream then waits for the
 * kernel; consumer_stream NULL is the decode's stream itself. n == 0 launches nothing.
 * TFRG_E_ARG (text in tfrg_last_error): no result, n_specs 0 or > TFRG_DENSE_MAX_SPECS, a slot >=
 * n_slots, a dtype that does not fit the slot's kind, a width outside 1..TFRG_DENSE_MAX_WIDTH, a NULL
 * out, a nonzero reserved.
 * ------------------------------------------------------------------------------------------- */
#define TFRG_DENSE_I64 0
#define TFRG_DENSE_I32 1
#define TFRG_DENSE_F32 2
#define TFRG_DENSE_U8 3
#define TFRG_DENSE_MAX_SPECS 64
#define TFRG_DENSE_MAX_WIDTH 4096
typedef struct tfrg_dense_spec {
  uint32_t slot;      /* column, as in tfrg_set_schema */
  uint32_t dtype;     /* TFRG_DENSE_* ; must fit the slot's kind */
  uint32_t width;     /* 1..TFRG_DENSE_MAX_WIDTH */
  uint32_t reserved;  /* 0 */
  uint64_t fill;      /* raw low bits of the pad value */
  void* out;          /* device, [n][width] row-major, caller-owned */
  int32_t* lengths;   /* device [n], or NULL */
} tfrg_dense_spec;
int tfrg_result_dense(tfrg_ctx* ctx, const tfrg_dense_spec* specs, uint32_t n_specs, uint32_t* d_stats,
                      void* consumer_stream);

/* Row-selected dense tensors: the same outputs for a list of records, a shuffled, sampled or filtered
 * minibatch of the last result. Outputs are [m][width], lengths [m]; output row k < m is record
 * g = d_rows[k] - row0 and holds exactly what tfrg_result_dense writes for row g. d_rows is a device
 * array of m int32 (TFRG_ROWS_I32) or int64 (TFRG_ROWS_I64) entries, ready on consumer_stream. An
 * entry with g outside [0, n) -- negative, INT64_MIN and INT64_MAX included -- is skipped: row k of
 * the outputs and lengths[k] are left as they were, no column is read for it, it counts in no d_stats
 * counter and adds 1 to d_skipped[spec] (device, [n_specs] u32, or NULL). d_stats and d_skipped are
 * zeroed by the call on the stream; lengths and d_stats are per output row written, so a record
 * drawn twice counts twice. row0 lets several contexts that hold consecutive runs of a row space
 * take one global row list: each writes the rows that are its own.
 * Confirmation of an optimistic or hinted decode (the only host synchronisation, once per decode),
 * stream order, any number of calls per decode and the full view afterwards are as for
 * tfrg_result_dense. m == 0 launches nothing; with n == 0 every row is skipped.
 * TFRG_E_ARG (text in tfrg_last_error): everything tfrg_result_dense refuses, a NULL d_rows with
 * m > 0, an unknown rows_dtype, m >= 2^31. */
#define TFRG_ROWS_I32 0
#define TFRG_ROWS_I64 1
int tfrg_result_dense_rows(tfrg_ctx* ctx, const tfrg_dense_spec* specs, uint32_t n_specs, const void* d_rows,
                           uint32_t rows_dtype, uint32_t m, int64_t row0, uint32_t* d_stats, uint32_t* d_skipped,
                           void* consumer_stream);

/* Ragged minibatches: packed values and offsets for a list of rows (the tf.io.parse_example
 * VarLenFeature / RaggedTensor side, next to the FixedLenFeature side above; the packed form varlen
 * attention, jagged tensors and EmbeddingBag take). Per spec and output row k < m, with
 * g = entry(k) - row0 and entry(k) = d_rows[k] (TFRG_ROWS_I32 / TFRG_ROWS_I64), or k itself when
 * d_rows is NULL (every record in order; rows_dtype is then ignored):
 *   L(k): record g's value count (int64_list / float_list slots), or the byte length of element 0 of
 *     its list, 0 if the list is empty or absent (bytes_list slots, TFRG_DENSE_U8);
 *   len(k): 0 where g is outside [0, n) (a skipped row, by tfrg_result_dense_rows's rule: INT64_MIN
 *     and INT64_MAX included); else L(k), or min(L(k), max_len) with max_len != 0;
 *   offsets[0] = 0, offsets[k + 1] = offsets[k] + len(k): all m + 1 are written, whatever cap is (a
 *     skipped row is an empty row here: a packed output has no row to leave alone);
 *   values[offsets[k] + j] for j < len(k): value j of record g, converted as by tfrg_result_dense
 *     (I32: the low 32 bits, F32: the raw bits, U8: byte j of element 0, zero past the readable input).
 *     Only positions < cap are stored and nothing else in values is written: with offsets[m] > cap the
 *     stored prefix is still correct, and the total shows the overflow.
 * d_totals (device, [n_specs] u64, or NULL): offsets[m] per spec. d_stats (device, [n_specs][4] u32, or
 * NULL; zeroed by the call on the stream): over the rows that are not skipped, rows with L > max_len
 * != 0 (truncated), rows without a value (empty), bytes rows with more than one element (multi); the
 * fourth counter is the skipped rows. A record drawn twice counts twice.
 * m == 0: offsets[0] = 0, totals 0, no kernel. n == 0: every row is skipped, all offsets are 0.
 * Three launches on the decode's stream (lengths per tile of rows, a scan of the tile sums, the
 * gather); no device value is read back. Stream order, confirmation of an optimistic or hinted decode
 * (the only host synchronisation, once per decode), the columns that are neither written nor read, the
 * full view afterwards and any number of calls per decode are as for tfrg_result_dense.
 * TFRG_E_ARG (text in tfrg_last_error): no context, no result, n_specs outside
 * 1..TFRG_RAGGED_MAX_SPECS, a slot >= n_slots, a dtype that does not fit the slot's kind, a NULL
 * offsets, values or offsets not aligned to their element size, a nonzero reserved, an unknown
 * rows_dtype with a non-NULL d_rows, m >= 2^31. */
#define TFRG_RAGGED_MAX_SPECS 64
typedef struct tfrg_ragged_spec {
  uint32_t slot;      /* column, as in tfrg_set_schema */
  uint32_t dtype;     /* TFRG_DENSE_*; must fit the slot's kind, as tfrg_dense_spec.dtype */
  uint32_t max_len;   /* 0: whole rows; else a row contributes at most max_len elements */
  uint32_t reserved;  /* 0 */
  uint64_t cap;       /* elements that values can hold */
  void* values;       /* device [cap] of the dtype, caller-owned; NULL: offsets and counters only */
  int64_t* offsets;   /* device [m + 1], caller-owned, not NULL */
} tfrg_ragged_spec;
int tfrg_result_ragged_rows(tfrg_ctx* ctx, const tfrg_ragged_spec* specs, uint32_t n_specs,
                            const void* d_rows, uint32_t rows_dtype, uint32_t m, int64_t row0,
                            uint64_t* d_totals, uint32_t* d_stats, void* consumer_stream);
/* rows per workgroup tile of tfrg_result_ragged_rows: a power of two from 64 to 4096, 0 = the default
 * (1024). A tuning/testing knob: with small tiles small row lists exercise the multi-tile logic. */
int tfrg_ctx_set_ragged_tile(tfrg_ctx* ctx, uint32_t rows);

/* Two-level ragged outputs: EVERY element of a bytes_list slot for a list of rows (the class strings
 * of a detection record, tags, several encoded frames), as three flat arrays: a list (rows) of lists
 * (elements) of byte strings. Rows (d_rows, rows_dtype, m, row0, a NULL d_rows as the identity list, the
 * rule for entries outside [0, n)) are exactly tfrg_result_ragged_rows's; a skipped row is an empty row.
 * Per spec and output row k < m, with g the row's record:
 *   C(k): record g's element count, 0 for a skipped row, an absent key or an empty list;
 *     cnt(k) = C(k), or min(C(k), max_elems) with max_elems != 0;
 *   row_offsets[0] = 0, row_offsets[k + 1] = row_offsets[k] + cnt(k): all m + 1 are written, whatever
 *     the capacities are. E = row_offsets[m];
 *   output element e, row_offsets[k] <= e < row_offsets[k + 1], is element e - row_offsets[k] of
 *     record g's list; L(e): its byte length; len(e) = L(e), or min(L(e), max_len) with max_len != 0;
 *   elem_offsets[0] = 0, elem_offsets[e + 1] = elem_offsets[e] + len(e) for e < E' = min(E, elem_cap):
 *     entries 0 .. E' are written and nothing else in the array;
 *   values[elem_offsets[e] + i] for e < E', i < len(e): byte i of element e, the byte
 *     tfrg_result_ragged_rows (TFRG_DENSE_U8) reads for an element (from the views into d_bytes, the
 *     materialized column, or the end-relative view of an implicit_off_slots slot; zero past the
 *     readable input). Only positions < cap are stored and nothing else in values is written.
 * d_totals (device, [n_specs][2] u64, or NULL): E, and B = the sum of len(e) over all E elements (not
 * only the first E'), so a first call without elem_offsets and values sizes both arrays exactly.
 * d_stats (device, [n_specs][4] u32, or NULL; zeroed by the call on the stream): rows with
 * C(k) > max_elems != 0; taken elements with L(e) > max_len != 0; rows that are not skipped and have
 * C(k) == 0; skipped rows. A record drawn twice counts twice.
 * m == 0: row_offsets[0] = 0, elem_offsets[0] = 0 where given, totals 0, no kernel. n == 0: every row
 * is skipped, all offsets and totals are 0. Two equal calls write equal bytes. With max_elems == 0 over
 * a decode whose records hold at most one element in the slot, values and B equal
 * tfrg_result_ragged_rows's (U8) values and total over the same rows, and
 * elem_offsets[row_offsets[k]] its offsets[k].
 * Four launches on the decode's stream (counts and byte sums per tile of rows, a scan of the tile
 * sums, the offsets, the copy); no device value is read back. Stream order, confirmation of an
 * optimistic or hinted decode (the only host synchronisation, once per decode), the implicit columns
 * that are neither written nor read, the full view afterwards and any number of calls per decode are
 * as for tfrg_result_ragged_rows; the rows per tile are tfrg_ctx_set_ragged_tile's.
 * TFRG_E_ARG (text in tfrg_last_error, nothing launched or written): no context, no result, n_specs
 * outside 1..TFRG_ELEMS_MAX_SPECS, a slot >= n_slots or not a bytes_list slot, a NULL row_offsets,
 * row_offsets or elem_offsets not 8-byte aligned, values without elem_offsets, a nonzero reserved, an
 * unknown rows_dtype with a non-NULL d_rows, m >= 2^31. */
#define TFRG_ELEMS_MAX_SPECS 32
typedef struct tfrg_elems_spec {
  uint32_t slot;         /* a bytes_list slot, as in tfrg_set_schema */
  uint32_t max_elems;    /* 0: every element of a row; else at most its first max_elems */
  uint32_t max_len;      /* 0: whole elements; else at most the first max_len bytes of each */
  uint32_t reserved;     /* 0 */
  uint64_t elem_cap;     /* elements that elem_offsets can describe (it holds elem_cap + 1 entries) */
  uint64_t cap;          /* bytes that values can hold */
  uint8_t* values;       /* device [cap], caller-owned; NULL: offsets and counters only */
  int64_t* elem_offsets; /* device [elem_cap + 1], caller-owned; NULL: row offsets and counters only */
  int64_t* row_offsets;  /* device [m + 1], caller-owned, not NULL */
} tfrg_elems_spec;       /* 56 bytes */
int tfrg_result_ragged_elems(tfrg_ctx* ctx, const tfrg_elems_spec* specs, uint32_t n_specs,
                             const void* d_rows, uint32_t rows_dtype, uint32_t m, int64_t row0,
                             uint64_t* d_totals, uint32_t* d_stats, void* consumer_stream);

/* Element ids: a bytes element as the integer a model takes (an embedding row, a class number), by a
 * hash into N buckets, by an exact lookup in a vocabulary, or by both.
 *
 * tfrg_hash64: one function of a byte string, computed identically by the host, the device and the
 * Python restatement in tfr_reader/ids.py (all arithmetic mod 2^64):
 *   h = 0xcbf29ce484222325
 *   for each 8-byte group w of the string, in order, read little-endian, the last one zero-padded:
 *     h = (h ^ w) * 0x100000001b3
 *   h ^= length
 *   h ^= h >> 33;  h *= 0xff51afd7ed558ccd;  h ^= h >> 33;  h *= 0xc4ceb9fe1a85ec53;  h ^= h >> 33
 * It is NOT TensorFlow's FarmHash (tf.strings.to_hash_bucket_fast gives other numbers): bucket numbers
 * are this library's own. They are stable across versions of the library, since callers may persist
 * them: the function above will not change. */
uint64_t tfrg_hash64(const uint8_t* p, uint64_t n);

/* A vocabulary: n_words distinct byte strings, each with an int64 id. Word i is
 * words[offsets[i] .. offsets[i + 1]) and its id is ids[i], or i when ids is NULL. device == -1 builds
 * the host table only: no HIP call is made, and tfrg_result_elem_ids refuses such a vocabulary.
 * device >= 0 also uploads the table to that device, once. The arguments are copied.
 * The table is an open-addressing table built on the host: capacity is the smallest power of two
 * >= max(16, 2 * n_words); a slot is a u32 word index, or 0xffffffff for empty; the words are inserted
 * in order, word i at tfrg_hash64(word i) & (capacity - 1) or, by linear probing, the first empty slot
 * after it (wrapping); max_probe is the largest displacement of any word from its home slot. Beside it:
 * the u32 word offsets, the word blob and the int64 ids. A match is byte equality: the hash picks the
 * home slot only. n_words == 0 is a valid vocabulary that nothing matches.
 * TFRG_E_ARG (text in tfrg_last_error): a word that occurs twice, n_words >= 2^31, words of 2^32
 * bytes or more in all (2^32 - 16 with device >= 0), offsets that descend, a NULL out.
 * tfrg_vocab_destroy synchronises the vocabulary's device before it frees the table, so work already
 * queued that reads it has finished; the caller keeps the object until the work that uses it has been
 * queued. NULL is accepted.
 * tfrg_vocab_info: any of the four pointers may be NULL; device_bytes is 0 for a host-only vocabulary.
 * tfrg_vocab_lookup_host: the id of the word equal to p[0 .. n), or `missing`. */
typedef struct tfrg_vocab tfrg_vocab;
int tfrg_vocab_create(int device, const uint8_t* words, const uint64_t* offsets, uint64_t n_words,
                      const int64_t* ids, tfrg_vocab** out);
int tfrg_vocab_destroy(tfrg_vocab* v);
int tfrg_vocab_info(const tfrg_vocab* v, uint64_t* n_words, uint64_t* capacity, uint32_t* max_probe,
                    uint64_t* device_bytes);
int64_t tfrg_vocab_lookup_host(const tfrg_vocab* v, const uint8_t* p, uint64_t n, int64_t missing);

/* The ids of EVERY element of a bytes_list slot for a list of rows: one int64 per element that
 * tfrg_result_ragged_elems would describe, in its order, with its row offsets. Rows (d_rows,
 * rows_dtype, m, row0, a NULL d_rows as the identity list, the rule for entries outside [0, n)) are
 * word for word tfrg_result_ragged_elems's; a skipped row is an empty row. Per spec:
 *   row_offsets[0 .. m] and the order of the elements are exactly those of tfrg_result_ragged_elems
 *     with the same max_elems, so ids[e] belongs to the element that call describes at e and the two
 *     outputs can be used side by side. All m + 1 row offsets are always written. E = row_offsets[m];
 *   the id of an element with bytes s: the id of the vocabulary's word equal to s, if there is one;
 *     else, with num_oov_buckets != 0, oov_base + (int64_t)(tfrg_hash64(s) % num_oov_buckets); else
 *     default_id. (Pure hashing: vocab NULL, oov_base 0. Out-of-vocabulary ids after the vocabulary:
 *     oov_base = n_words. Out-of-vocabulary ids first: ids[i] = i + k at tfrg_vocab_create, oov_base 0.)
 *   s is what tfrg_result_ragged_elems reads for the element: from the views into d_bytes, the
 *     materialized column, or the end-relative view of an implicit_off_slots slot with the constant
 *     length of TFRG_IMPLICIT_BYTES_LEN; bytes past the readable input read as zero. Columns an
 *     optimistic decode left implicit are neither read nor written.
 *   Only positions < elem_cap of ids are stored and nothing else in ids is written.
 * d_totals (device, [n_specs] u64, or NULL): E. d_stats (device, [n_specs][4] u32, or NULL; zeroed by
 * the call on the stream), counted over all E taken elements and not only the stored ones: rows with
 * more than max_elems != 0 elements; taken elements that matched no word (every element, with vocab
 * NULL); rows that are not skipped and have no element; skipped rows. A record drawn twice counts twice.
 * m == 0: row_offsets[0] = 0, totals 0, no kernel. n == 0: every row is skipped. Two equal calls write
 * equal bytes.
 * Three launches on the decode's stream (counts per tile of rows, the scan of the tile sums, then row
 * offsets and ids); no device value is read back. Stream order with consumer_stream, the single
 * confirmation of an optimistic or hinted decode, any number of calls per decode, the rows per tile
 * (tfrg_ctx_set_ragged_tile) and scratch from the context's arena are as for tfrg_result_ragged_elems.
 * Cost: an element is hashed, probed and compared by ONE lane, 8 bytes a step, so one very long element
 * holds its wave for its whole length (accepted, as tfrg_result_select_match's CONTAINS scan is: cap
 * such a slot's work with a vocabulary, below). An element longer than the vocabulary's longest word
 * under num_oov_buckets == 0 can match nothing and needs no hash: its bytes are not read at all.
 * Without d_stats, elements at or past elem_cap (all of them with ids NULL) are not read either: a
 * first call with ids NULL and d_stats NULL that sizes ids costs the row pass alone.
 * TFRG_E_ARG (text in tfrg_last_error prefixed "tfrg_result_elem_ids: ", nothing launched or
 * written): everything tfrg_result_ragged_elems refuses about the context, the rows and m; n_specs
 * outside 1..TFRG_IDS_MAX_SPECS; a slot >= n_slots or not a bytes_list slot; a NULL or misaligned
 * row_offsets, a misaligned ids; nonzero reserved words; vocab NULL with num_oov_buckets == 0; a
 * vocabulary built host-only or on another device than the context's. */
#define TFRG_IDS_MAX_SPECS 32
typedef struct tfrg_ids_spec {
  uint32_t slot;            /* a bytes_list slot, as in tfrg_set_schema */
  uint32_t max_elems;       /* 0: every element of a row; else at most its first max_elems */
  uint32_t reserved0;       /* 0 */
  uint32_t reserved1;       /* 0 */
  const tfrg_vocab* vocab;  /* NULL: hash buckets only */
  uint64_t num_oov_buckets; /* 0: an unmatched element gets default_id */
  int64_t oov_base;
  int64_t default_id;
  uint64_t elem_cap;        /* ids that `ids` can hold */
  int64_t* ids;             /* device [elem_cap], caller-owned; NULL: offsets and counters only */
  int64_t* row_offsets;     /* device [m + 1], caller-owned, not NULL */
} tfrg_ids_spec;            /* 72 bytes */
int tfrg_result_elem_ids(tfrg_ctx* ctx, const tfrg_ids_spec* specs, uint32_t n_specs,
                         const void* d_rows, uint32_t rows_dtype, uint32_t m, int64_t row0,
                         uint64_t* d_totals, uint32_t* d_stats, void* consumer_stream);

/* Filtered row lists: the WHERE clause over the last result, on the device. Predicates over the
 * decoded columns in, the compacted list of the passing rows in device memory out -- usable as it is
 * as d_rows of tfrg_result_dense_rows / tfrg_result_ragged_rows of the same context(s), with the same
 * row0, and with no host synchronisation in between.
 * Candidates: candidate k < m has entry(k) = d_rows[k] (TFRG_ROWS_I32 / TFRG_ROWS_I64), or k itself
 * when d_rows is NULL (rows_dtype is then ignored), and names record g = entry(k) - row0. A candidate
 * with g outside [0, n) -- INT64_MIN and INT64_MAX included, by tfrg_result_dense_rows's rule -- is
 * skipped: nothing indexed by g is read, it is never selected, and it adds 1 to d_stats[1].
 * A term is true or false for record g:
 *   TFRG_SEL_VALUE: false if the record has <= index values, whatever the op (NE included); else
 *     value[index] op operand;
 *   TFRG_SEL_ANY: true iff some value of the record's list satisfies the op (false for an empty or
 *     absent list);
 *   TFRG_SEL_COUNT, TFRG_SEL_BYTES_LEN, TFRG_SEL_STATUS: always defined (0 for an absent list),
 *     compared as signed int64.
 * int64_list slots compare as signed 64-bit integers. float_list slots compare the float32 VALUES, not
 * their bits: a NaN on either side is false under every op but NE, -0.0 == 0.0, and denormals are not
 * flushed (the smallest positive denormal is > 0.0).
 * Terms combine as an AND of OR-groups: record g passes iff every group that occurs among the terms
 * holds at least one true term. `label IN (1, 3)` is two EQ terms of one group, `10 <= x < 20` two
 * terms of two groups; n_terms == 0 selects every candidate that is not skipped.
 * Output: the entries entry(k) (not g) of the passing candidates, in candidate order, go to d_out from
 * position base on: base is 0, or with TFRG_SEL_APPEND the value of *d_count as the call's kernels find
 * it on the device. Only positions < cap are stored and nothing else in d_out is written;
 * *d_count = base + passing shows an overflow, as tfrg_result_ragged_rows's totals do. d_out NULL gives
 * the count alone. out_dtype (TFRG_ROWS_I32 / TFRG_ROWS_I64) is independent of rows_dtype. d_stats
 * (device, [2] u32, or NULL; zeroed by the call on the stream): candidates selected by this call,
 * candidates skipped. The output is a function of the inputs alone: two equal calls write equal bytes.
 * m == 0: no kernel; *d_count = 0, or unchanged with TFRG_SEL_APPEND. n == 0: every candidate is skipped.
 * Three launches on the decode's stream (verdicts per tile of candidates, kept as one bit each; a scan
 * of the tile sums; the write, which reads the bits and the entries alone); no device value is read
 * back. Stream order, confirmation of an optimistic or hinted decode (the only host synchronisation,
 * once per decode), the columns that are neither written nor read (identity row splits of placed
 * slots, the implicit lengths and statuses), the full view afterwards and any number of calls per
 * decode are as for tfrg_result_ragged_rows. Calls that share one consumer_stream are ordered with
 * each other, whatever their contexts: several contexts holding consecutive runs of a row space append
 * to one list, each with its own row0, the first without TFRG_SEL_APPEND.
 * TFRG_E_ARG (text in tfrg_last_error, prefixed "tfrg_result_select_rows: "): no context, no result,
 * n_terms > TFRG_SEL_MAX_TERMS, a slot >= n_slots, a subject that does not fit the slot's kind (VALUE /
 * ANY on a bytes_list slot, BYTES_LEN on another kind, STATUS with slot != 0), an unknown subject or
 * op, group >= 32, index != 0 outside VALUE, a nonzero reserved, a float operand with high bits set, an
 * unknown rows_dtype with a non-NULL d_rows, an unknown out_dtype, m >= 2^31, a NULL d_count, d_out or
 * d_count not aligned to their element size, a TFRG_ROWS_I32 output when [row0, row0 + n) does not fit
 * int32, unknown flag bits. (d_out non-NULL with cap == 0 is allowed.) */
#define TFRG_SEL_MAX_TERMS 32
/* subject of a term */
#define TFRG_SEL_VALUE 0      /* value `index` of the record's list (int64_list / float_list slot) */
#define TFRG_SEL_ANY 1        /* any value of the record's list (int64_list / float_list slot) */
#define TFRG_SEL_COUNT 2      /* the record's value count (any kind), compared as int64 */
#define TFRG_SEL_BYTES_LEN 3  /* byte length of element 0 of a bytes_list slot, 0 if empty or absent
                                 (tfrg_result_dense's lengths), compared as int64 */
#define TFRG_SEL_STATUS 4     /* the record's status (tfrg_status.h) as int64; slot must be 0 */
/* op */
#define TFRG_SEL_EQ 0
#define TFRG_SEL_NE 1
#define TFRG_SEL_LT 2
#define TFRG_SEL_LE 3
#define TFRG_SEL_GT 4
#define TFRG_SEL_GE 5
typedef struct tfrg_select_term {
  uint32_t slot;      /* column, as in tfrg_set_schema */
  uint32_t subject;   /* TFRG_SEL_VALUE .. TFRG_SEL_STATUS */
  uint32_t op;        /* TFRG_SEL_EQ .. TFRG_SEL_GE */
  uint32_t group;     /* < 32: terms of one group are ORed, the groups ANDed */
  uint32_t index;     /* TFRG_SEL_VALUE only, else 0 */
  uint32_t reserved;  /* 0 */
  uint64_t operand;   /* int64 raw bits; float_list VALUE / ANY: float bits in the low 32, high 32 zero */
} tfrg_select_term;   /* 32 bytes */
#define TFRG_SEL_APPEND 1u
int tfrg_result_select_rows(tfrg_ctx* ctx, const tfrg_select_term* terms, uint32_t n_terms,
                            const void* d_rows, uint32_t rows_dtype, uint32_t m, int64_t row0,
                            void* d_out, uint32_t out_dtype, uint64_t cap, uint64_t* d_count,
                            uint32_t* d_stats, uint32_t flags, void* consumer_stream);
/* candidates per workgroup tile of tfrg_result_select_rows: a power of two from 64 to 4096, 0 = the
 * default (1024). A tuning/testing knob, as tfrg_ctx_set_ragged_tile. */
int tfrg_ctx_set_select_tile(tfrg_ctx* ctx, uint32_t rows);

/* Filtered row lists with predicates on bytes features: `name = 'cat'`, `path LIKE 'train/%'`,
 * `name ~ 'rose'`, `id IN (...)` (the two queries of the reference's README.md filter on a string
 * feature). tfrg_result_select_match is tfrg_result_select_rows -- every parameter after patterns_len is
 * that call's, with the same meaning -- plus two subjects, three ops and the byte-string operands they
 * take. Candidates, skipped candidates, groups, output, d_count, d_stats, TFRG_SEL_APPEND, stream order,
 * the single confirmation of an optimistic or hinted decode, determinism (two equal calls write equal
 * bytes) and the m == 0 / n == 0 cases are exactly as documented there; the subjects and ops of
 * tfrg_result_select_rows work unchanged through this call and may be mixed with the new ones in one
 * term table. tfrg_result_select_rows itself still refuses the new subjects and ops.
 * Patterns: `patterns` is HOST memory, patterns_len <= TFRG_SEL_MAX_PATTERN_BYTES bytes holding the
 * operands back to back. It is consumed before the call returns (the caller may free or overwrite it at
 * once): the bytes travel to the kernel inside its launch argument, beside the term table, with no
 * device allocation, no copy on a stream and no host synchronisation. A pattern is a range of it of at
 * most TFRG_SEL_MAX_PATTERN bytes; terms may share a pattern, and patterns may overlap.
 * New subjects, on bytes_list slots only. For both, operand = pattern offset | (uint64_t)pattern
 * length << 32, with [offset, offset + length) inside [0, patterns_len):
 *   TFRG_SEL_BYTES: element `index` of the record's list. False, whatever the op (NE included), if the
 *     record has <= index elements (TFRG_SEL_VALUE's rule); else element op pattern;
 *   TFRG_SEL_BYTES_ANY: true iff some element of the record's list satisfies the op (false for an empty
 *     or absent list); index must be 0.
 * A failed record (status != 0) has no values: every bytes term is false for it.
 * Ops: TFRG_SEL_EQ .. TFRG_SEL_GE compare the element with the pattern as Python compares bytes objects:
 * byte by byte as unsigned values (0x80 > 0x7f), the first difference decides, and a proper prefix is
 * less than the longer string. TFRG_SEL_PREFIX / TFRG_SEL_SUFFIX / TFRG_SEL_CONTAINS (valid with the two
 * new subjects only): the element starts with / ends with / contains the pattern as a contiguous
 * substring. The empty pattern equals the empty element alone, and is a prefix, a suffix and a substring
 * of every element that is present (the empty one included).
 * An element's bytes are the ones tfrg_result_dense (TFRG_DENSE_U8) reads for it, from whichever source
 * the decode left: the (offset, length) views into d_bytes, the materialized byte column
 * (TFRG_FLAG_MATERIALIZE_BYTES), or for a slot of tfrg_info.implicit_off_slots the view at
 * d_end32[g] + tfrg_ctx_rel_off, with the constant length of TFRG_IMPLICIT_BYTES_LEN where that bit is
 * set; the columns an optimistic decode left implicit are neither read nor written. d_bytes and d_end32
 * must stay in place and unchanged as documented for tfrg_result_dense / tfrg_info.implicit_off_slots.
 * Nothing at or past round_up(nbytes, 16) of d_bytes (the byte column: its capacity) is touched: a byte
 * of a view that lies there reads as 0. An element of the last record that ends at nbytes, whatever
 * nbytes % 16 is, is compared in full.
 * Cost: EQ .. GE, PREFIX and SUFFIX read at most the pattern's length of an element, whatever its size
 * (a 512 KiB element compared for equality costs a length test), one lane per candidate. CONTAINS reads
 * an element until the first match: its lane walks an element of up to tfrg_ctx_set_select_scan bytes;
 * a longer one is streamed by the whole wave in coalesced 2 KiB chunks through LDS, pattern length - 1
 * bytes carried from chunk to chunk. A term table without a bytes subject runs the kernels of
 * tfrg_result_select_rows.
 * TFRG_E_ARG (text in tfrg_last_error, prefixed "tfrg_result_select_match: "): everything
 * tfrg_result_select_rows refuses, with subjects up to TFRG_SEL_BYTES_ANY and ops up to
 * TFRG_SEL_CONTAINS known; a bytes subject on a slot that is not a bytes_list; TFRG_SEL_PREFIX /
 * _SUFFIX / _CONTAINS with another subject; index != 0 outside TFRG_SEL_VALUE and TFRG_SEL_BYTES; a
 * pattern longer than TFRG_SEL_MAX_PATTERN; patterns_len > TFRG_SEL_MAX_PATTERN_BYTES; a pattern range
 * that is not inside [0, patterns_len); patterns NULL with patterns_len > 0. (patterns NULL with
 * patterns_len 0 is allowed: every pattern is then empty. As in tfrg_result_select_rows nothing is
 * launched or written when the call fails.) */
#define TFRG_SEL_MAX_PATTERN 256u
#define TFRG_SEL_MAX_PATTERN_BYTES 2048u
/* subjects of tfrg_result_select_match alone */
#define TFRG_SEL_BYTES 5      /* element `index` of the record's list (bytes_list slot) against a pattern */
#define TFRG_SEL_BYTES_ANY 6  /* any element of the record's list (bytes_list slot) against a pattern */
/* ops of tfrg_result_select_match alone, with the two subjects above */
#define TFRG_SEL_PREFIX 6
#define TFRG_SEL_SUFFIX 7
#define TFRG_SEL_CONTAINS 8
int tfrg_result_select_match(tfrg_ctx* ctx, const tfrg_select_term* terms, uint32_t n_terms,
                             const uint8_t* patterns, uint64_t patterns_len,
                             const void* d_rows, uint32_t rows_dtype, uint32_t m, int64_t row0,
                             void* d_out, uint32_t out_dtype, uint64_t cap, uint64_t* d_count,
                             uint32_t* d_stats, uint32_t flags, void* consumer_stream);
/* TFRG_SEL_CONTAINS: elements longer than `bytes` are scanned by their whole wave, shorter ones by the
 * candidate's lane: 4 to 65536, 0 = the default (256). The result does not depend on it. A
 * tuning/testing knob: with 4, elements of a few bytes exercise the wave scan. */
int tfrg_ctx_set_select_scan(tfrg_ctx* ctx, uint32_t bytes);

/* ---------------------------------------------------------------------------------------------
 * Double-buffered host -> HBM decode stream (replaces reader.py:212-247's per-record ThreadPool
 * read+decode for whole-dataset reads). Two slots, each with a pinned staging buffer of batch_bytes,
 * a device input buffer and its own decode context + stream. tfrg_stream_submit hands a batch (pieces:
 * file byte ranges or host memory, whole files or record-aligned runs of them) to the slot's worker
 * thread, which reads / copies it into the slot's pinned buffer (copy_threads threads), indexes every piece with the native framing walk
 * (or on the device after the H2D copy: tfrg_stream_set_device_index),
 * enqueues the H2D copies and tfrg_decode_device on the slot's stream, and returns at once; so the
 * next batch stages while this one decodes. tfrg_stream_wait blocks until the slot's batch is
 * enqueued and gives its record count (and records per piece); results are then read from
 * tfrg_stream_ctx(slot) with tfrg_result_info / _fetch / _device and stay valid until the next
 * submit to that slot. A slot is submitted again only after tfrg_stream_wait claimed its last batch
 * (else TFRG_E_ARG). The pieces' memory must stay valid until tfrg_stream_wait returns. Set the
 * key table on both contexts (tfrg_set_schema) while their slots are idle.
 * ------------------------------------------------------------------------------------------- */
typedef struct tfrg_stream tfrg_stream;
int tfrg_stream_create(int device, uint64_t batch_bytes, int copy_threads, tfrg_stream** out);
int tfrg_stream_destroy(tfrg_stream* s);
tfrg_ctx* tfrg_stream_ctx(tfrg_stream* s, int slot);
/* piece i: bytes [offsets[i], offsets[i] + sizes[i]) of file paths[i] (read with pread), or, where
 * paths is NULL or paths[i] is NULL, sizes[i] bytes of host memory at pieces[i] (e.g. the
 * decompressed stream of a ZLIB / GZIP file) */
int tfrg_stream_submit(tfrg_stream* s, int slot, const uint8_t* const* pieces, const char* const* paths,
                       const uint64_t* offsets, const uint64_t* sizes, int n_pieces, uint32_t flags);
/* stage_ms (NULL or 4 doubles): the batch's phases in ms, for the end-to-end report: file read /
 * copy into pinned memory, framing index, H2D + decode (synchronised), D2H of the columns */
int tfrg_stream_wait(tfrg_stream* s, int slot, uint64_t* n_records, uint64_t* nbytes, uint64_t* piece_records,
                     int cap, double* stage_ms);
/* the slot's decode summary and its result columns, already copied into pinned host memory by the
 * slot's worker (NULL members: aux when no record failed, bytes_off when bytes are materialised);
 * valid until the next submit to the slot. A summary with n_miss_records != 0 needs the key table
 * extended and the batch decoded again (tfrg_decode_host on the slot's context). */
int tfrg_stream_result(tfrg_stream* s, int slot, tfrg_info* info, tfrg_columns* host);
/* the slot's pinned copy of its batch (bytes_list views index into it) and its record ranges */
/* on != 0: the slot workers build the framing index on the device (tfrg_index_device over the bytes
 * just copied H2D; the (start, end) columns come back D2H beside the result columns) instead of
 * walking the pieces on the host; a batch that reports a fallback is indexed on the host as before.
 * Default 0. Call it while both slots are idle. stage_ms[1] is then the device index with its
 * synchronisation (the bytes' H2D included: the index waits for it). */
int tfrg_stream_set_device_index(tfrg_stream* s, int on);
const uint8_t* tfrg_stream_host_buffer(tfrg_stream* s, int slot);
int tfrg_stream_host_ranges(tfrg_stream* s, int slot, const uint64_t** starts, const uint64_t** ends);

/* Measurement helper (achievable HBM read bandwidth next to the 8 TB/s spec): one
 * streaming read of d_bytes[0, nbytes) (16 B nontemporal loads, nbytes a multiple of 16) on
 * `stream`, XOR-folded into the u32 at d_sink so the loads are live. variant 0..3 picks the loads in
 * flight per lane and the grid (4/16 blocks per CU, 8/8, 8/16, 16/4). Not part of the decode path. */
int tfrg_stream_read(const void* d_bytes, uint64_t nbytes, uint32_t* d_sink, void* stream, int variant);

/* Devices visible to libtfrg (hipGetDeviceCount); the multi-device host paths spread files over them. */
int tfrg_device_count(void);

#ifdef __cplusplus
}
#endif
#endif
