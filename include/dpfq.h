/*
 * dpfq.h — C ABI of libdpfq.so: the per-read lengths and cumulative bases behind the FASTQ read index on the MI355X
 * (gfx950).
 *
 * A fifth library next to libdpscan.so (dpscan.h), libdpquote.so (dpquote.h), libdpfai.so (dpfai.h) and libdpvpos.so
 * (dpvpos.h): it shares the process, the HIP runtime and the caller's device memory with them, so every entry point
 * takes raw device pointers and the ctx binds an opaque `void* stream` (= hipStream_t).  Status is returned as an int
 * (DFQ_OK = 0); the message of the last failure on the calling thread is available from dfq_last_error().  No C++
 * exception crosses this boundary.  Every launch is asynchronous on the ctx stream and owns no state besides its
 * output arrays: synchronize the stream (or enqueue a copy on it) to read them.
 *
 * Definition of the index.  Let the object have `size` bytes.
 *
 *   Lines.  Line 0 starts at 0 if size > 0.  A further line starts at p + 1 for every '\n' at p with p + 1 < size.
 *   Line i is the bytes [s_i, e_i), with e_i the offset of its '\n', or size for an unterminated last line.  Its
 *   content length c_i is e_i - s_i, less 1 if the line is non-empty and byte[e_i - 1] == '\r'.  L is the number of
 *   lines.
 *
 *   Reads.  Read r is the lines 4r .. 4r + 3 and R = L / 4 (rounded down).  Read boundaries come from the line count
 *   alone, so a quality line that begins with '@' is harmless.  Read r is WELL FORMED iff, checked in this order,
 *     c_{4r} >= 1 and byte[s_{4r}] == '@'                      else DFQ_BAD_HEADER;
 *     c_{4r+2} >= 1 and byte[s_{4r+2}] == '+'                  else DFQ_BAD_SEPARATOR;
 *     c_{4r+1} == c_{4r+3} and that length is below 2^32       else DFQ_LENGTH_MISMATCH.
 *   Nothing after the '+' is looked at.  A read of zero bases is well formed.  len_r = c_{4r+1}.
 *
 *   Indexable.  The object is INDEXABLE iff every read is well formed and L % 4 == 0.  With L % 4 != 0 the error is
 *   "truncated", attributed to read R at offset s_{4R}.  The first offending read, in file order, is what an error
 *   names, so a malformed read r < R comes before the truncation.  Wrapped FASTQ (a sequence or a quality string
 *   that spans several lines) is not supported: it surfaces as one of these errors.
 *
 *   Stored.  With K a power of two >= 1, S = ceil(R / K) and B the sum of all len_r: S + 1 pairs of little-endian
 *   uint64.  Pair j < S is (s_{4jK}, the sum of len_r over r < jK); the closing pair is (size, B).  An empty object
 *   stores the single pair (0, 0).
 *
 * What the launches compute.  d_starts holds ascending object offsets of line starts (uint64).  Read r < n of one
 * launch is the entries skip + 4r .. skip + 4r + 3; line j of it ends before entry skip + 4r + j + 1, and line 3 of
 * read n - 1 ends at `last_end` (the offset of its '\n', or size).  `skip` in 0..3 is the number of lines in front
 * that belong to a read begun before the launch's lines.
 *     len[r]    c of line 1, truncated to 32 bits;
 *     flags[r]  DFQ_WELL_FORMED (0) or the first of DFQ_BAD_HEADER, DFQ_BAD_SEPARATOR, DFQ_LENGTH_MISMATCH that holds.
 *   A byte the definition needs that lies outside the buffer or at or beyond size reads as 0 (so a header or a
 *   separator there is bad).  Whatever d_starts holds, nothing is read outside d_buf[0 .. buf_len), nothing outside
 *   d_starts[0 .. skip + 4n) rounded out to the aligned 16-byte words that hold its first and last entry, and nothing
 *   is written outside the output arrays.  With entries that do not ascend the lengths are unspecified.
 *
 * No workgroup of these kernels ever waits on another one: there is no look-back, no spin, no flag and no ticket.
 * The kernel boundaries between read, scan and sample are the only ordering; shared state is the output arrays and
 * the result words, initialised on the stream by dfq_reads_async.
 */
#ifndef DPFQ_H
#define DPFQ_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DFQ_OK 0
#define DFQ_ERR_INVALID 1 /* bad argument */
#define DFQ_ERR_HIP 2     /* a HIP runtime call failed (message in dfq_last_error) */

#define DFQ_WELL_FORMED 0u
#define DFQ_BAD_HEADER 1u
#define DFQ_BAD_SEPARATOR 2u
#define DFQ_LENGTH_MISMATCH 3u
#define DFQ_NONE 0xFFFFFFFFFFFFFFFFull /* a lowest index, or a minimum, of which there is none */

/* the result words (uint64 each) */
#define DFQ_R_MALFORMED 0     /* reads whose flag is not DFQ_WELL_FORMED */
#define DFQ_R_MAX_LEN 1       /* the largest len[r], 0 without reads */
#define DFQ_R_BASES 2         /* the sum of all len[r] (written by dfq_scan_async) */
#define DFQ_R_MIN_MALFORMED 3 /* the lowest malformed r, or DFQ_NONE */
#define DFQ_R_MIN_LEN 4       /* the smallest len[r], or DFQ_NONE without reads */
#define DFQ_R_WORDS 5

typedef struct dfq_ctx dfq_ctx;

#define DFQ_ABI_VERSION 1
int dfq_abi_version(void);        /* returns DFQ_ABI_VERSION of the build */
const char* dfq_last_error(void); /* thread-local message of the last failure */

/* Binds `device` and `stream` (NULL: the device's default stream); the ctx does not own the stream. */
int dfq_ctx_create(int device, void* stream, dfq_ctx** out);
int dfq_ctx_destroy(dfq_ctx* ctx); /* waits for the stream first; NULL is a no-op */

/*
 * Reads (fq_read_kernel, one lane per read).  d_buf[0 .. buf_len) (device memory, any alignment) holds object bytes
 * [buf_base, buf_base + buf_len) of an object of `size` bytes.  d_starts (uint64, 8-byte aligned) holds
 * skip + 4 * n entries; n < 2^32.  Writes d_len[n] (uint32), d_flags[n] (uint8) as defined above, d_block[w] (uint64)
 * = the sum of len[] over the reads of workgroup w (reads_per_wg of dfq_geometry each; ceil(n / reads_per_wg)
 * entries), and d_result (DFQ_R_WORDS uint64), initialised on the stream by this call, with n == 0 too.
 */
int dfq_reads_async(dfq_ctx* ctx, const uint8_t* d_buf, uint64_t buf_len, uint64_t buf_base, uint64_t size,
                    const uint64_t* d_starts, uint32_t skip, uint64_t n, uint64_t last_end, uint32_t* d_len,
                    uint8_t* d_flags, uint64_t* d_block, uint64_t* d_result);
/*
 * Scan (fq_scan_kernel, one workgroup): the exclusive sums of d_block[0 .. n_blocks) in place, in uint64, and their
 * total into d_result[DFQ_R_BASES] (no other result word is touched).
 */
int dfq_scan_async(dfq_ctx* ctx, uint64_t* d_block, uint64_t n_blocks, uint64_t* d_result);
/*
 * Sample (fq_sample_kernel, one lane per read) over len[] of n reads, of which read 0 has the global index `read0`;
 * `every` = K, a power of two.  d_block holds the scanned block sums.  For every read with (read0 + r) % K == 0 the
 * pair (d_starts[skip + 4r], the sum of len[] over the launch's reads before r) goes to slot
 * (read0 + r) / K - ceil(read0 / K) of d_samples (two uint64 per slot; the caller provides
 * ceil((read0 + n) / K) - ceil(read0 / K) slots).  len[] is an input like any other: its sums are made in uint64.
 */
int dfq_sample_async(dfq_ctx* ctx, const uint64_t* d_starts, uint32_t skip, const uint32_t* d_len,
                     const uint64_t* d_block, uint64_t n, uint64_t read0, uint32_t every, uint64_t* d_samples);

/* Launch geometry (tests): the reads of one workgroup of the read and sample kernels, the lanes of the scan's. */
int dfq_geometry(dfq_ctx* ctx, int* reads_per_wg, int* scan_lanes);

#ifdef __cplusplus
}
#endif
#endif /* DPFQ_H */
