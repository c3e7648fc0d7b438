/*
 * dpfai.h — C ABI of libdpfai.so: the per-sequence counts behind a faidx-compatible FASTA index (.fai) on the
 * MI355X (gfx950).
 *
 * A third library next to libdpscan.so (dpscan.h) and libdpquote.so (dpquote.h): it shares the process, the HIP
 * runtime and the caller's device memory with them, so every entry point takes raw device pointers and the ctx binds
 * an opaque `void* stream` (= hipStream_t).  Status is returned as an int (DFAI_OK = 0); the message of the last
 * failure on the calling thread is available from dfai_last_error().  No C++ exception crosses this boundary.  Every
 * launch is asynchronous on the ctx stream and owns no state besides its output arrays: synchronize the stream (or
 * enqueue a copy on it) to read them.
 *
 * Definition of the index.  Take the stored header pairs (start_i, end_i), i < H, of an object of `size` bytes.
 *
 *   Body.  The body of sequence i is [b_i, e_i), b_i = end_i, e_i = start_{i+1} (size for the last); B_i = e_i - b_i.
 *
 *   The GPU computes, per body, over its bytes:
 *     nl_i     the number of '\n' bytes,
 *     cr_i     the number of '\r' bytes,
 *     first_i  the lowest offset of a '\n', or none,
 *   and in a second launch that is given W_i:
 *     off_i      the number of '\n' at p with (p - b_i + 1) % W_i != 0,
 *     lastoff_i  the highest such p.
 *
 *   The host derives:
 *     OFFSET    = b_i
 *     LINEWIDTH = W_i = first_i - b_i + 1, or B_i when the body has no '\n'
 *     t_i, the terminator length: 1 if cr_i == 0; 2 if cr_i == nl_i > 0; anything else is mixed line endings
 *     LINEBASES = W_i - t_i (= B_i when there is no '\n')
 *     LENGTH    = B_i - nl_i - cr_i
 *     NAME      = the header bytes after '>' up to the first of space, tab, '\r', '\n'
 *
 *   Regular.  Sequence i is regular iff every line but the last has width W_i and no line is longer.  In the counts,
 *   with m = B_i / W_i (integer division) for W_i > 0, that is both of
 *     nl_i - off_i == m;
 *     off_i == 0, or off_i == 1 and lastoff_i == e_i - 1.
 *   A body without any '\n' is regular, and so is an empty body (all columns 0 except OFFSET).
 *
 *   Errors (as samtools faidx refuses such a file): an irregular sequence (mixed line endings included), a
 *   W_i >= 2^32, a duplicate NAME.
 *
 *   Scope.  Every body byte other than '\n' and '\r' counts as a base: spaces and tabs inside a body are bases here
 *   (htslib counts only graphic characters).  Which '>' is a header is not decided here: the pairs are taken as
 *   stored.
 *
 * Segments.  The launches know nothing about headers: they take n segments as device arrays lo[n], hi[n], origin[n]
 * of uint64 OBJECT offsets -- ascending, disjoint, lo <= hi, clipped by the caller to the buffer -- and count per
 * segment.  origin is the unclipped b_i, so the parts of a body that is cut over several buffers are counted
 * separately and merged by the caller: nl, cr, off add, first takes the minimum, lastoff the maximum.
 * Whatever the segment arrays hold, nothing is read outside d_buf[0 .. buf_len) and nothing is written outside the
 * n entries of each output array; segments that break the contract only yield wrong counts.
 *
 * No workgroup of these kernels ever waits on another one: there is no look-back, no spin and no flag, only atomics
 * on the output arrays and the memsets that initialise them at every launch.
 */
#ifndef DPFAI_H
#define DPFAI_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DFAI_OK 0
#define DFAI_ERR_INVALID 1 /* bad argument */
#define DFAI_ERR_HIP 2     /* a HIP runtime call failed (message in dfai_last_error) */

#define DFAI_NONE 0xFFFFFFFFFFFFFFFFull /* first[i] of a segment without any '\n' */

typedef struct dfai_ctx dfai_ctx;

#define DFAI_ABI_VERSION 1
int dfai_abi_version(void);      /* returns DFAI_ABI_VERSION of the build */
const char* dfai_last_error(void); /* thread-local message of the last failure */

/* Binds `device` and `stream` (NULL: the device's default stream); the ctx does not own the stream. */
int dfai_ctx_create(int device, void* stream, dfai_ctx** out);
int dfai_ctx_destroy(dfai_ctx* ctx); /* waits for the stream first; NULL is a no-op */

/*
 * Pass 1 (fai_count_kernel).  d_buf[0 .. buf_len) (device memory, any alignment) holds object bytes
 * [buf_base, buf_base + buf_len).  d_nl[i], d_cr[i] receive the '\n' and '\r' bytes of segment i, d_first[i] the
 * lowest object offset of a '\n' in it, or DFAI_NONE.  The three arrays (n uint64 each, 8-byte aligned) are
 * initialised on the stream by this call; every input byte is read at most once.
 */
int dfai_count_async(dfai_ctx* ctx, const uint8_t* d_buf, uint64_t buf_len, uint64_t buf_base, const uint64_t* d_lo,
                     const uint64_t* d_hi, const uint64_t* d_origin, uint64_t n, uint64_t* d_nl, uint64_t* d_cr,
                     uint64_t* d_first);
/*
 * Pass 2 (the second instantiation of fai_count_kernel).  d_width[i] (uint32) is W_i.  d_off[i] receives the number
 * of '\n' of segment i at an object offset p with (p - origin[i] + 1) % W_i != 0, d_lastoff[i] the highest such p,
 * or 0 when there is none.  A width of 0 counts every '\n' of the segment.  Both arrays are initialised by this call.
 */
int dfai_offgrid_async(dfai_ctx* ctx, const uint8_t* d_buf, uint64_t buf_len, uint64_t buf_base,
                       const uint64_t* d_lo, const uint64_t* d_hi, const uint64_t* d_origin, const uint32_t* d_width,
                       uint64_t n, uint64_t* d_off, uint64_t* d_lastoff);
/*
 * Names (fai_name_kernel, two launches).  Header i starts with its '>' at object offset d_start[i] and ends before
 * d_end[i], both clipped by the caller to the buffer (d_start[i] < d_end[i] <= buf_base + buf_len).
 * dfai_name_len_async: d_len[i] = the number of bytes after the '>' and before the first space, tab, '\r' or '\n',
 *   or before d_end[i].
 * dfai_name_copy_async: copies those d_len[i] bytes to d_out + d_off[i]; d_off are the caller's exclusive sums of
 *   d_len.  Nothing at or beyond d_out[out_cap] is written.
 */
int dfai_name_len_async(dfai_ctx* ctx, const uint8_t* d_buf, uint64_t buf_len, uint64_t buf_base,
                        const uint64_t* d_start, const uint64_t* d_end, uint64_t n, uint32_t* d_len);
int dfai_name_copy_async(dfai_ctx* ctx, const uint8_t* d_buf, uint64_t buf_len, uint64_t buf_base,
                         const uint64_t* d_start, const uint32_t* d_len, const uint64_t* d_off, uint64_t n,
                         uint8_t* d_out, uint64_t out_cap);

/* Launch geometry (tests, tuning): R, the bytes of the range a wave takes at a time; K, the per-wave segment slots
 * in LDS (a range that holds more segments sends the rest straight to global atomics); the waves of the grid. */
int dfai_geometry(dfai_ctx* ctx, int* range_bytes, int* slots, int* grid_waves);

#ifdef __cplusplus
}
#endif
#endif /* DPFAI_H */
