/*
 * dpquote.h — C ABI of libdpquote.so, the quote-aware CSV record index for the MI355X (gfx950).
 *
 * A library of its own next to libdpscan.so (dpscan.h): it shares the process, the HIP runtime and the
 * caller's device memory with it, so every entry point takes raw device pointers and an opaque
 * `void* stream` (= hipStream_t, e.g. the one dp_ctx_get_stream returns).  Status is returned as an int
 * (DQ_OK = 0, the codes mirror DP_*); the message of the last failure on the calling thread is available
 * from dq_last_error().  No C++ exception crosses this boundary.  Use one dq_ctx per host thread and
 * stream; at most one dq_records_async is in flight per ctx.
 *
 * Semantics.  Over object bytes d[begin, end), a quote byte q and an incoming state carry (1 = "inside a
 * quoted field at begin"): P(p) = (carry + #{x in [begin, p) : d[x] == q}) mod 2, and a byte d[p] == '\n'
 * is a RECORD END iff P(p) == 0.  An escaped quote "" toggles twice, so the parity rule is exact for
 * RFC 4180 input; for malformed input the parity rule is the definition.
 *
 * Escape-aware semantics (dq_records_esc_async, dq_records_esc_blocked_async): the dialect that writes a quote
 * inside a field as \" (Spark, Hive, MySQL INTO OUTFILE, Python csv with escapechar and doublequote=False).  With an
 * escape byte e (e != q, e != '\n') and an incoming esc_carry (1 = "the byte at begin is escaped"):
 *
 *     esc = esc_carry; inside = carry; toggles = 0
 *     for p in begin .. end-1:
 *         b = d[p]
 *         if esc:                      an escaped byte is literal, whatever it is (an escape byte included)
 *             esc = 0
 *             if b == '\n' and not inside and scope == QUOTED: record end at p
 *             continue
 *         if   b == e: esc = 1
 *         elif b == q: inside ^= 1; toggles += 1
 *         elif b == '\n' and not inside: record end at p
 *
 * A byte is escaped iff it follows a maximal run of not-escaped escape bytes of odd length.  Escaped quotes do not
 * toggle; "" still toggles twice.  Scope ALL (flags = 0, what Python's csv module and pandas do): the escape works
 * outside quoted fields too, an escaped '\n' never ends a record.  Scope QUOTED (DQ_ESC_SCOPE_QUOTED, what Spark /
 * univocity files need): a '\n' outside a quoted field always ends the record, so an unquoted field may end in the
 * escape byte.  On malformed input this state machine is the definition.
 * Runs of escape bytes up to DQ_ESCAPE_RUN_MAX bytes are exact.  A longer run may end the launch with
 * DQ_ERR_ESCAPE_RUN (the kernel walks back over a run only so far; it waits for nothing and never returns a wrong
 * index instead).
 *
 * Reference interface this stands in for (CLOUDLAB-URV/dataplug @ 2025-07-11): the row boundaries that
 * CSVSlice.get resolves byte by byte (formats/generic/csv.py:52-105).  The reference treats every '\n' as
 * a row end there, which cuts RFC 4180 records whose quoted fields hold line breaks; this index is the
 * set of '\n' that really end a record, as one sorted offset array.
 */
#ifndef DPQUOTE_H
#define DPQUOTE_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DQ_OK 0
#define DQ_ERR_INVALID 1   /* bad argument */
#define DQ_ERR_HIP 2       /* a HIP runtime call failed (message in dq_last_error) */
#define DQ_ERR_CAPACITY 3  /* output capacity too small; the required count is still returned */
#define DQ_ERR_OVERFLOW 4  /* a uint32 offset would be >= 2^32 */
#define DQ_ERR_TIMEOUT 5   /* an inter-workgroup wait hit its bound (results invalid) */
#define DQ_ERR_ESCAPE_RUN 6 /* a run of escape bytes longer than DQ_ESCAPE_RUN_MAX (results invalid) */

#define DQ_ESCAPE_RUN_MAX (1u << 20) /* runs of escape bytes up to this many bytes are exact */
#define DQ_ESC_SCOPE_QUOTED 1u       /* flags bit: the escape works inside quoted fields only */

typedef struct dq_ctx dq_ctx;

#define DQ_ABI_VERSION 1
int dq_abi_version(void);                                  /* returns DQ_ABI_VERSION of the build */
const char* dq_last_error(void);                           /* thread-local message of the last failure */

/* Binds `device` and `stream` (NULL: the device's default stream).  The ctx owns the tile ticket, the
 * look-back descriptor array (grow-only device memory) and a pinned result block; it does not own the
 * stream.  Fails with DQ_ERR_HIP (and a message) where there is no usable device. */
int dq_ctx_create(int device, void* stream, dq_ctx** out);
int dq_ctx_destroy(dq_ctx* ctx);                           /* waits for the stream first; NULL is a no-op */

/*
 * Record ends of object bytes [begin, end), enqueued on the ctx stream without waiting.
 *   d_buf[0 .. buf_len) (device memory, any alignment) holds object bytes [buf_base, buf_base + buf_len);
 *   buf_base <= begin <= end <= buf_base + buf_len.  quote: the quote byte (not '\n'); carry: 0 or 1.
 *   d_out receives the ascending OBJECT offsets of the record ends, uint32 (out_u64 = 0) or uint64; at
 *   most `cap` entries are written and nothing at or beyond d_out[cap].  cap = 0 with d_out = NULL is the
 *   count-only call.  One pass over the bytes: every 64 KiB tile is read once, its incoming state and
 *   output base come from a decoupled look-back over tile summaries.
 */
int dq_records_async(dq_ctx* ctx, const uint8_t* d_buf, uint64_t buf_len, uint64_t buf_base, uint64_t begin,
                     uint64_t end, uint32_t quote, uint32_t carry, void* d_out, int out_u64, uint64_t cap);
/*
 * The same record ends in the blocked form u16b (the form scan.objects.BlockedOffsets and formats/_lines.LineIndex
 * decode): a quarter of the bytes of the uint64 form, written by the kernel directly.  The additive entry point
 * of ABI version 1; collected by dq_records_result like dq_records_async.
 *   d_low receives, in ascending order, the low 16 bits of every record end's OBJECT offset (at most `cap`
 *   entries, nothing at or beyond d_low[cap]; cap = 0 with d_low = NULL counts only).
 *   d_table[j], j in 0 .. ntiles with ntiles = ((end - 1) >> 16) - (begin >> 16) + 1 (0 for an empty range),
 *   receives the number of record ends of THIS launch that lie before object offset ((begin >> 16) + j) << 16:
 *   d_table[0] = 0, and record end i lies in 64 KiB block (begin >> 16) + j for the largest j with
 *   d_table[j] <= i, so its offset is (((begin >> 16) + j) << 16) | d_low[i].  Exactly ntiles entries are written
 *   (whatever cap is) and nothing beyond them; table_cap is the room at d_table, in entries.
 *   The kernel's 64 KiB tiles lie on the object's 64 KiB grid here, so a table entry is the output base a tile's
 *   look-back resolves and a low word is the byte's position in its tile; no offset can overflow.
 * Alignment rule: the 16-byte loads need the tile grid 16-byte aligned in device memory, so the device address
 *   of object byte `begin`, d_buf + (begin - buf_base), must be congruent to `begin` mod 16 (the rule of
 *   dp_delim_ranges out_modes 3 and 4).  Only 16-byte chunks that hold a byte of [begin, end) are read.
 * DQ_ERR_INVALID: a non-empty range that breaks the alignment rule, table_cap < ntiles, d_table = NULL with a
 *   non-empty range, d_low not 2-byte or d_table not 8-byte aligned, and every check of dq_records_async.
 */
int dq_records_blocked_async(dq_ctx* ctx, const uint8_t* d_buf, uint64_t buf_len, uint64_t buf_base,
                             uint64_t begin, uint64_t end, uint32_t quote, uint32_t carry, uint16_t* d_low,
                             uint64_t cap, uint64_t* d_table, uint64_t table_cap);
/*
 * Waits for the launch and returns its counts: *n_out record ends (the full count even beyond cap),
 * *n_quotes bytes == quote, *n_newlines bytes == '\n' (kept or not) in [begin, end); each may be NULL.
 *   DQ_ERR_CAPACITY: n_out > cap (the counts are still returned; the first cap entries are valid);
 *   DQ_ERR_OVERFLOW: out_u64 = 0 and a record end lies at an offset >= 2^32;
 *   DQ_ERR_TIMEOUT:  a look-back wait exceeded its 20 s bound; the kernel ended, the output is invalid.
 */
int dq_records_result(dq_ctx* ctx, uint64_t* n_out, uint64_t* n_quotes, uint64_t* n_newlines);

/*
 * The escape-aware launches (additive entry points of ABI version 1; further instantiations of the same kernel).
 * Arguments as dq_records_async / dq_records_blocked_async, plus: escape, the escape byte; esc_carry, 0 or 1, 1 = the
 * byte at `begin` is escaped; flags, 0 (scope ALL) or DQ_ESC_SCOPE_QUOTED.  At most one launch of any kind is in
 * flight per ctx; collect with dq_records_esc_result (or dq_records_result).
 * DQ_ERR_INVALID: escape > 255, escape == quote, escape == '\n', esc_carry > 1, an unknown flags bit, and every check
 *   of the entry point they extend.
 */
int dq_records_esc_async(dq_ctx* ctx, const uint8_t* d_buf, uint64_t buf_len, uint64_t buf_base, uint64_t begin,
                         uint64_t end, uint32_t quote, uint32_t carry, uint32_t escape, uint32_t esc_carry,
                         uint32_t flags, void* d_out, int out_u64, uint64_t cap);
int dq_records_esc_blocked_async(dq_ctx* ctx, const uint8_t* d_buf, uint64_t buf_len, uint64_t buf_base,
                                 uint64_t begin, uint64_t end, uint32_t quote, uint32_t carry, uint32_t escape,
                                 uint32_t esc_carry, uint32_t flags, uint16_t* d_low, uint64_t cap,
                                 uint64_t* d_table, uint64_t table_cap);
/*
 * dq_records_result plus *n_toggles: the quote bytes that are not escaped, which is what a chain of launches over
 * consecutive ranges adds up into the next range's carry (for a plain launch: n_quotes).  After an escape-aware
 * launch *n_quotes still counts every byte == quote; *n_newlines counts the '\n' bytes that can end a record: all
 * of them under scope QUOTED, the ones that are not escaped under scope ALL.
 *   DQ_ERR_ESCAPE_RUN: a run of escape bytes longer than DQ_ESCAPE_RUN_MAX; the kernel ended, the output is invalid.
 */
int dq_records_esc_result(dq_ctx* ctx, uint64_t* n_out, uint64_t* n_quotes, uint64_t* n_newlines,
                          uint64_t* n_toggles);

/* Launch geometry (for tests/tuning): workgroups of the persistent grid, and bytes per tile. */
int dq_geometry(dq_ctx* ctx, int* grid, int* tile_bytes);

#ifdef __cplusplus
}
#endif
#endif /* DPQUOTE_H */
