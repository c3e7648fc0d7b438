/*
 * dpvpos.h — C ABI of libdpvpos.so: the per-line CHROM / POS parse behind the VCF position index on the MI355X
 * (gfx950).
 *
 * A fourth library next to libdpscan.so (dpscan.h), libdpquote.so (dpquote.h) and libdpfai.so (dpfai.h): it shares
 * the process, the HIP runtime and the caller's device memory with them, so every entry point takes raw device
 * pointers and the ctx binds an opaque `void* stream` (= hipStream_t).  Status is returned as an int (DVP_OK = 0); the
 * message of the last failure on the calling thread is available from dvp_last_error().  No C++ exception crosses this
 * boundary.  Every launch is asynchronous on the ctx stream and owns no state besides its output arrays: synchronize
 * the stream (or enqueue a copy on it) to read them.
 *
 * Definition of the index.  Let the object have `size` bytes and its body start at `body_offset`.
 *
 *   Lines.  Line 0 starts at body_offset.  A further line starts at p + 1 for every '\n' at p in the body with
 *   p + 1 < size.  A line ends before its '\n' or at size, so an unterminated last line is a line.  An empty body
 *   (body_offset >= size) has no lines.
 *
 *   Fields of a line that starts at s.  t1 is the first '\t' in the line and t2 the second.  CHROM is the bytes
 *   [s, t1) and POS the bytes (t1, t2).  The line is WELL FORMED iff
 *     both tabs exist and t2 - s < VPOS_PREFIX_MAX (1024);
 *     CHROM is non-empty;
 *     POS is 1 to 10 ASCII digits with a value of at most 2^31 - 1.
 *   Leading zeros are accepted.  Nothing after t2 is looked at.  Any byte value, 0x80 and above included, may occur
 *   in CHROM (a '\t' or '\n' ends it by definition).
 *
 *   Contig runs.  A run is a maximal sequence of consecutive lines with byte-equal CHROM.  The object is INDEXABLE
 *   iff every line is well formed, POS never decreases inside a run, and no CHROM has two runs (the lines of a
 *   contig are contiguous, as tabix requires).  The first offending line, in file order, is what an error names: a
 *   line is checked for malformed, then unsorted (same CHROM as the line before and a lower POS), then split contig
 *   (it starts a run whose CHROM had a run before).
 *
 *   Stored.  The POS of every line whose ordinal is a multiple of K (a power of two >= 1) as uint32 little-endian,
 *   and one text row per run in file order:  NAME\tFIRST_LINE\tNUM_LINES\tOFFSET\tEND\tMIN_POS\tMAX_POS\n  with OFFSET
 *   and END the byte offsets of the run's first byte and one past its last.
 *
 * What the launches compute, per line i < n of one launch (d_starts[i] ascending object offsets of line starts):
 *     pos[i]    the value of POS, 0 for a malformed line;
 *     clen[i]   the length of CHROM, 0 for a malformed line;
 *     flags[i]  bit 0 (VPOS_SAME): i > 0, line i is well formed, and the first field of line i - 1 -- its bytes up to
 *               its first '\t' -- equals CHROM of line i (whether or not line i - 1 is well formed);
 *               bit 1 (VPOS_MALFORMED): line i is not well formed.
 *   A prefix that reaches size, or the end of the buffer, with t2 unresolved is malformed, and so is a start outside
 *   the buffer.  Whatever d_starts holds, nothing is read outside d_buf[0 .. buf_len) rounded out to the aligned
 *   dwords that hold its first and last byte, and nothing is written outside the n entries of each output array.
 *
 * No workgroup of these kernels ever waits on another one: there is no look-back, no spin, no flag and no ticket.
 * The kernel boundary between parse and reduce is the only ordering; shared state is the output arrays and the
 * result words, initialised on the stream at every launch.
 */
#ifndef DPVPOS_H
#define DPVPOS_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVP_OK 0
#define DVP_ERR_INVALID 1 /* bad argument */
#define DVP_ERR_HIP 2     /* a HIP runtime call failed (message in dvp_last_error) */

#define VPOS_PREFIX_MAX 1024 /* t2 - s of a well-formed line is below this */
#define VPOS_POS_MAX 2147483647u
#define VPOS_SAME 1u
#define VPOS_MALFORMED 2u
#define DVP_NONE 0xFFFFFFFFFFFFFFFFull /* a lowest index of which there is none */

/* the result words of dvp_reduce_async (uint64 each) */
#define DVP_R_RUNS 0        /* run starts: lines with bit 0 clear (the full count, even beyond run_cap) */
#define DVP_R_MALFORMED 1   /* lines with bit 1 set */
#define DVP_R_UNSORTED 2    /* lines with bit 0 set and pos[i] < pos[i - 1] */
#define DVP_R_FIRST_POS 3   /* pos[0] */
#define DVP_R_LAST_POS 4    /* pos[n - 1] */
#define DVP_R_RUN_ENDS 5    /* run ends: lines i with i + 1 == n or bit 0 of line i + 1 clear (= DVP_R_RUNS) */
#define DVP_R_MIN_MALFORMED 6 /* the lowest malformed i, or DVP_NONE */
#define DVP_R_MIN_UNSORTED 7  /* the lowest unsorted i, or DVP_NONE */
#define DVP_R_WORDS 8

typedef struct dvp_ctx dvp_ctx;

#define DVP_ABI_VERSION 1
int dvp_abi_version(void);        /* returns DVP_ABI_VERSION of the build */
const char* dvp_last_error(void); /* thread-local message of the last failure */

/* Binds `device` and `stream` (NULL: the device's default stream); the ctx does not own the stream. */
int dvp_ctx_create(int device, void* stream, dvp_ctx** out);
int dvp_ctx_destroy(dvp_ctx* ctx); /* waits for the stream first; NULL is a no-op */

/*
 * Parse (vpos_parse_kernel, one lane per line).  d_buf[0 .. buf_len) (device memory, any alignment) holds object
 * bytes [buf_base, buf_base + buf_len) of an object of `size` bytes.  d_starts[n] (uint64, 8-byte aligned) are
 * ascending line starts as object offsets; n < 2^32.  Writes d_pos[n] (uint32), d_clen[n] (uint16), d_flags[n]
 * (uint8) as defined above.
 */
int dvp_parse_async(dvp_ctx* ctx, const uint8_t* d_buf, uint64_t buf_len, uint64_t buf_base, uint64_t size,
                    const uint64_t* d_starts, uint64_t n, uint32_t* d_pos, uint16_t* d_clen, uint8_t* d_flags);
/*
 * Reduce (vpos_reduce_kernel, one lane per line) over the parse outputs of n lines, of which line 0 has the global
 * ordinal `ordinal0`; `every` = K, a power of two.
 *   d_samples: pos[i] of every line with (ordinal0 + i) % K == 0, at slot (ordinal0 + i) / K - ceil(ordinal0 / K);
 *              the caller provides ceil((ordinal0 + n) / K) - ceil(ordinal0 / K) uint32 slots.
 *   d_runs, d_run_ends, d_run_clen (run_cap entries each; uint64, uint64, uint32): the slot of a run start is taken
 *              from a counter, so the entries are in no particular order -- sort them by their line index:
 *              d_runs[k] = i << 32 | pos[i] of a run start i with d_run_clen[k] = clen[i]; d_run_ends[k] =
 *              i << 32 | pos[i] of a run end i.  Nothing at or beyond run_cap is written; DVP_R_RUNS holds the
 *              full count, so a caller that finds it above run_cap launches again with that capacity.
 *   d_result:  DVP_R_WORDS uint64, initialised on the stream by this call.
 */
int dvp_reduce_async(dvp_ctx* ctx, const uint32_t* d_pos, const uint16_t* d_clen, const uint8_t* d_flags, uint64_t n,
                     uint64_t ordinal0, uint32_t every, uint32_t* d_samples, uint64_t* d_runs, uint64_t* d_run_ends,
                     uint32_t* d_run_clen, uint64_t run_cap, uint64_t* d_result);
/*
 * Names (vpos_name_kernel, one wave per name).  Copies the d_clen[d_lines[j]] CHROM bytes of line d_lines[j]
 * (uint32 line indices < n, j < m) to d_out + d_off[j]; d_off are the caller's exclusive sums of those lengths.
 * d_line_start[j] (uint64) receives d_starts[d_lines[j]], the byte offset of that line.  Nothing at or beyond
 * d_out[out_cap] is written and nothing outside the buffer is read.
 */
int dvp_names_async(dvp_ctx* ctx, const uint8_t* d_buf, uint64_t buf_len, uint64_t buf_base, const uint64_t* d_starts,
                    const uint16_t* d_clen, uint64_t n, const uint32_t* d_lines, const uint64_t* d_off, uint64_t m,
                    uint8_t* d_out, uint64_t out_cap, uint64_t* d_line_start);

/* Launch geometry (tests): the lines of one workgroup of the parse kernel and of the reduce kernel. */
int dvp_geometry(dvp_ctx* ctx, int* parse_lines, int* reduce_lines);

#ifdef __cplusplus
}
#endif
#endif /* DPVPOS_H */
