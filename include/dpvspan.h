/*
 * dpvspan.h — C ABI of libdpvspan.so: where each record of a VCF body ends (rec_end), behind the record-end index
 * that lets a region query return every record whose interval [POS, rec_end] overlaps it, on the MI355X (gfx950).
 *
 * A sixth library next to libdpscan.so, libdpquote.so, libdpfai.so, libdpvpos.so (dpvpos.h) and libdpfq.so: it shares
 * the process, the HIP runtime and the caller's device memory with them, so every entry point takes raw device
 * pointers and the ctx binds an opaque `void* stream` (= hipStream_t).  Status is returned as an int (DVS_OK = 0); the
 * message of the last failure on the calling thread is available from dvs_last_error().  No C++ exception crosses this
 * boundary.  Every launch is asynchronous on the ctx stream and owns no state besides its output arrays: synchronize
 * the stream (or enqueue a copy on it) to read them.
 *
 * Definition.  Lines are those of dpvpos.h.  For a line [s, e), e its '\n' or `size`, field k (k = 1, 2, ...) is the
 * bytes between tab k - 1 and tab k, or up to e for the last field; POS is field 2 as dpvpos.h defines it.
 *
 *   reflen is the length of field 4.  A line with fewer than 4 fields, or with an empty field 4, is MISSING_REF.
 *   INFO is field 8 if the line has at least 8 fields; its entries are separated by ';'.
 *   The END entry is the first INFO entry that begins with the four bytes "END=" (it begins at INFO's first byte or
 *   directly behind a ';', so CIEND= and XEND= do not match).  Its end is a ';', a '\t' or e.
 *   The END value COUNTS iff the bytes behind '=' up to the entry's end are 1 to 10 ASCII digits, the value is at
 *   most 2^31 - 1, and the value is at least POS.
 *   rec_end is that value if it counts, and POS + reflen - 1 otherwise, saturated at 2^32 - 1.  So END=. , END= ,
 *   11 digits, a value above 2^31 - 1 or below POS and a non-digit in the value fall back to REF, and a later second
 *   END= entry is ignored whether or not the first one counts.  rec_end >= POS always holds.
 *
 *   Stored.  One uint32 little-endian per K-block, K = the position index's sampling step: slot j is the maximum
 *   rec_end over the body lines with ordinal in [jK, (j + 1)K); ceil(num_body_lines / K) slots, aligned with the
 *   samples of dpvpos.h.  Contig boundaries inside a block are not separated: a slot is a filter that may only
 *   over-include.
 *
 * What the span launch computes, per line i < n (d_starts[i] ascending object offsets of line starts, d_pos[i] the
 * parse output of dvp_parse_async for the same lines -- read, not recomputed):
 *     end[i]    rec_end, 0 for a line that is MISSING_REF or TRUNCATED;
 *     flags[i]  bit 0 (VSPAN_MISSING_REF);
 *               bit 1 (VSPAN_TRUNCATED): the buffer ends, below the object's end, before the walk has seen the end of
 *               field 8 (its '\t') or the line's end -- for a line with fewer than 8 fields that is before field 4's
 *               end or, with field 4 complete, before the '\n' that shows there is no field 8; a start outside the
 *               buffer is truncated too;
 *               bit 2 (VSPAN_FROM_END): the END value counted.
 *   At most one of bits 0 and 1 is set, and bit 2 only without them.  The walk stops at the first of: an empty field
 *   4, the end of field 8, the line's end, the buffer's end.  Whatever d_starts holds, nothing is read outside
 *   d_buf[0 .. buf_len) rounded out to the aligned dwords that hold its first and last byte, and nothing is written
 *   outside the n entries of each output array.
 *
 * No workgroup of these kernels ever waits on another one: no look-back, no spin, no flag, no ticket.  The kernel
 * boundary between span and block-max is the only ordering; shared state is the slots and the result words,
 * initialised on the stream at every launch.
 */
#ifndef DPVSPAN_H
#define DPVSPAN_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVS_OK 0
#define DVS_ERR_INVALID 1 /* bad argument */
#define DVS_ERR_HIP 2     /* a HIP runtime call failed (message in dvs_last_error) */

#define VSPAN_END_MAX 2147483647u /* an END value above this does not count */
#define VSPAN_MISSING_REF 1u
#define VSPAN_TRUNCATED 2u
#define VSPAN_FROM_END 4u
#define DVS_NONE 0xFFFFFFFFFFFFFFFFull /* a lowest index of which there is none */

/* the result words of dvs_blockmax_async (uint64 each) */
#define DVS_R_MISSING 0       /* lines with bit 0 set */
#define DVS_R_TRUNCATED 1     /* lines with bit 1 set */
#define DVS_R_FROM_END 2      /* lines with bit 2 set */
#define DVS_R_MAX_SPAN 3      /* the maximum of end[i] - pos[i] over the lines with neither bit 0 nor bit 1 */
#define DVS_R_MIN_MISSING 4   /* the lowest i with bit 0 set, or DVS_NONE */
#define DVS_R_MIN_TRUNCATED 5 /* the lowest i with bit 1 set, or DVS_NONE */
#define DVS_R_WORDS 6

typedef struct dvs_ctx dvs_ctx;

#define DVS_ABI_VERSION 1
int dvs_abi_version(void);        /* returns DVS_ABI_VERSION of the build */
const char* dvs_last_error(void); /* thread-local message of the last failure */

/* Binds `device` and `stream` (NULL: the device's default stream); the ctx does not own the stream. */
int dvs_ctx_create(int device, void* stream, dvs_ctx** out);
int dvs_ctx_destroy(dvs_ctx* ctx); /* waits for the stream first; NULL is a no-op */

/*
 * Span (vspan_span_kernel, one lane per line).  d_buf[0 .. buf_len) (device memory, any alignment) holds object
 * bytes [buf_base, buf_base + buf_len) of an object of `size` bytes.  d_starts[n] (uint64, 8-byte aligned) are
 * ascending line starts as object offsets; n < 2^32.  d_pos[n] (uint32) is read.  Writes d_end[n] (uint32) and
 * d_flags[n] (uint8) as defined above.
 */
int dvs_span_async(dvs_ctx* ctx, const uint8_t* d_buf, uint64_t buf_len, uint64_t buf_base, uint64_t size,
                   const uint64_t* d_starts, uint64_t n, const uint32_t* d_pos, uint32_t* d_end, uint8_t* d_flags);
/*
 * Block maxima (vspan_blockmax_kernel) over the span outputs of n lines, of which line 0 has the global ordinal
 * `ordinal0`; `every` = K, a power of two.
 *   d_blockmax: slot (ordinal0 + i) / K - ordinal0 / K receives the maximum of its lines' end[i]; the caller
 *               provides (ordinal0 + n - 1) / K - ordinal0 / K + 1 uint32 slots (none for n = 0), set to 0 on the
 *               stream by this call.  The first and the last slot may be partial blocks.
 *   d_result:   DVS_R_WORDS uint64, initialised on the stream by this call.
 */
int dvs_blockmax_async(dvs_ctx* ctx, const uint32_t* d_end, const uint8_t* d_flags, const uint32_t* d_pos, uint64_t n,
                       uint64_t ordinal0, uint32_t every, uint32_t* d_blockmax, uint64_t* d_result);

/* Launch geometry (tests): the lines of one workgroup of the span kernel and of the block-max kernel. */
int dvs_geometry(dvs_ctx* ctx, int* span_lines, int* blockmax_lines);

#ifdef __cplusplus
}
#endif
#endif /* DPVSPAN_H */
