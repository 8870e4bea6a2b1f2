/*
 * muahuff_ingest.h -- C ABI of libmuahuff_ingest.so, the companion of libmuahuff.so: what stands around the codec.
 * In front of it, stage L0 of the reference's pipeline, spike time stamps -> binned counts; behind it, storage: the
 * per-segment CRC-32 of a compacted payload (mhi_seg_crc32), taken when a container is written and checked when it is
 * read.  All on the MI355X (gfx950).
 *
 * The reference bins per-channel spike times with histogram2 and uint8() (Data/Load_and_bin_Sabes_store_as_mat_file.m:
 * 30-54); its RTL counts detections per BIN_PERIOD clock ticks and holds at SPIKE_RATE_CLIP-1 (FPGA implementation/
 * 1_binner_final.v:19-21).  This library does the RTL's integer-tick form of it and writes either the byte-per-bin
 * channels the codec reads or, directly, the packed 2- / 4-bit chunk-blocked pieces of the stream path -- the
 * time-major block and mh_deinterleave_packed drop out of that path.
 *
 * Recordings arrive as ONE merged list of (time, channel) pairs in time order (the loaders' MUA_vec), not per channel:
 * mhi_aer_to_csr brings such a list, resident on the device, into the per-channel form mhi_bin_events reads -- a stable
 * partition by channel (count, scan, scatter), not a sort -- so that no stage in front of the codec runs on the host.
 *
 * And the way back: mhi_unbin_count / mhi_unbin_emit expand a matrix of counts -- a decoded recording -- into spike events
 * again, per channel (the input of mhi_bin_events) or as one merged pair list (the input of mhi_aer_to_csr).
 *
 * And the commonest query on a decoded recording: mhi_windows cuts the same window around many trigger times out of every
 * row in one call, re-binned on each window's own grid, stacked per trial or summed over the trials into a PSTH.
 *
 * Neither a binner nor a checksum is a codec operation, so they are not part of muahuff.h: that ABI is closed.  The conventions are the
 * same: every function returns MH_OK or a negative MH_ERR_* code of muahuff.h and never throws, mhi_last_error()
 * returns a thread-local message for the last failure on this thread, every argument check comes before any device
 * work, `stream` is a hipStream_t passed as void* (NULL = the default stream), the caller owns every buffer.  There
 * is no CPU fallback, no environment variable is read and nothing but the mhi_* functions is exported.
 */
#ifndef MUAHUFF_INGEST_H
#define MUAHUFF_INGEST_H

#include "muahuff.h"

#ifdef __cplusplus
extern "C" {
#endif

int mhi_version(void); /* == MH_VERSION of the muahuff.h this library was built with */
const char *mhi_last_error(void);

/* ticks: device, all channels' event time stamps back to back; channel c owns ticks[ev_off[c] .. ev_off[c+1]),
 * non-decreasing within the channel (duplicates allowed).  ev_off: device, C + 1 entries.
 * Bin b of a channel counts its events with origin + b*period <= tick < origin + (b+1)*period, b < T.
 * Events before origin or at/after origin + T*period are ignored.  period >= 1, T >= 1, 1 <= C < 2^31, ticks < 2^63;
 * origin + T*period must not exceed 2^63 (else MH_ERR_ARG: no tick could lie beyond it, and the bounds of every bin
 * then fit 64 bits without a wrap).
 * bits = 8: out + out_off[c] receives T bytes min(count, 255)                (MATLAB uint8(), Sabes loader :54)
 * bits = 4 / 2: ceil(T/16) pieces of 8 / 4 bytes holding min(count, 15) / min(count, 3), in EXACTLY the layout
 *   mh_deinterleave_packed writes: same bit order, cut last piece zero-padded and written whole, out_off[c] % 16 == 0,
 *   chunk_stride 0 = contiguous, else chunk j of channel c at out_off[c] + j * chunk_stride (same validity rules:
 *   a multiple of 16, at least one packed chunk; MH_ERR_ARG for any non-zero chunk_stride with bits = 8).
 * Every bin / piece of every channel is written (zeros included: no memset by the caller) and nothing else -- not
 * even the bytes up to the next multiple of 16 that mh_deinterleave_packed may touch.
 * out, out_off: device.  out_off % 16 is checked on the host where the table is host-readable as well (pinned or
 * managed memory); a host pointer the device cannot read is MH_ERR_ARG in any case; a table in device-only memory is
 * not read on the host, and a misaligned entry there is stored to as given.
 * Only enqueues on `stream`: no synchronisation, allocation or free, so it can be captured into a hipGraph.
 * Memory-safe on unsorted input: the counts are then unspecified, but no store leaves the channel's own bins. */
int mhi_bin_events(const uint64_t *ticks, const uint64_t *ev_off, uint32_t C, uint64_t origin, uint64_t period,
                   uint64_t T, uint32_t bits, uint8_t *out, const uint64_t *out_off, uint64_t chunk_stride,
                   void *stream);

/* The largest C of mhi_aer_to_csr: every wave keeps one 32-bit cursor per channel in LDS (64 KiB). */
#define MHI_AER_MAX_CHANNELS 16384

/* Bytes of scratch mhi_aer_to_csr needs for n pairs over C channels.  Host arithmetic only: no device is needed or
 * touched.  Non-decreasing in n for a fixed C, never 0.  MH_ERR_ARG: bytes NULL, C == 0, C > MHI_AER_MAX_CHANNELS,
 * n >= 2^32. */
int mhi_aer_scratch_bytes(uint64_t n, uint32_t C, uint64_t *bytes);

/* Stable partition of n (tick, channel) pairs by channel.  ticks: device, n entries; channels: device, n entries of
 * ch_bits = 16 or 32 bits, unsigned, pair i = (ticks[i], channels[i]).
 * out_ticks[ev_off[c] + k] is the tick of the k-th input pair, in input order, whose channel is c: with a list in time
 * order, (out_ticks, ev_off) is the input of mhi_bin_events.  ev_off[0] == 0 and ev_off[C] is the number of pairs kept.
 * A pair whose channel is >= C is dropped and counted: dropped[0] = the number of such pairs (0 when there are none).
 * Written: out_ticks[0 .. ev_off[C]), ev_off[0 .. C], dropped[0] and the scratch -- nothing at or after
 * out_ticks[ev_off[C]], nothing else.
 * Tick values are never inspected: a list that is not in time order gives the same stable partition, and no index
 * depends on data other than a channel that was compared with C first -- every store stays in the buffers above
 * whatever the list holds.
 * n == 0 is valid: ev_off all zero, dropped zero.  C >= 1.
 * MH_ERR_ARG, before any device work: a NULL pointer (with n == 0 as well), ch_bits other than 16 / 32, C == 0,
 * C > MHI_AER_MAX_CHANNELS, n >= 2^32 (output positions are 32-bit inside), scratch_bytes below what
 * mhi_aer_scratch_bytes(n, C) returns, scratch not 16-byte aligned, out_ticks[0 .. n) overlapping ticks[0 .. n).
 * out_ticks, ev_off, dropped: device, n / C + 1 / 1 entries.  scratch need not be zeroed or kept between calls.
 * Only enqueues on `stream`: no synchronisation, allocation or free, so it can be captured into a hipGraph, and two
 * calls in a row on the same scratch are ordered by the stream. */
int mhi_aer_to_csr(const uint64_t *ticks, const void *channels, uint32_t ch_bits, uint64_t n, uint32_t C,
                   uint64_t *out_ticks, uint64_t *ev_off, uint64_t *dropped, void *scratch, uint64_t scratch_bytes,
                   void *stream);

/* CRC-32 of directory segments of a payload, one value per segment: the zlib / IEEE 802.3 one (reflected polynomial
 * 0xEDB88320, initial value and final xor 0xFFFFFFFF, "123456789" -> 0xCBF43926) over the segment's stored words as
 * little-endian bytes -- zlib.crc32(payload[off : off + n].tobytes()).  A segment of 0 words has CRC 0.
 * payload: device, payload_words 32-bit words, 4-byte aligned -- segments may start at ANY word (mh_compact packs them
 * back to back).  seg_off / seg_words: device, n_segments entries, words.  seg_idx: device, n_idx directory indices
 * (the segments a range query uploaded; any order), or NULL: all n_segments.
 * crc: device, n_segments entries, written at the listed segments only; may be NULL when expect is given.
 * expect: NULL, or device, n_segments stored values -- the verify form: bad[0] += the number of listed segments whose
 * CRC differs from expect[segment], bad[1] = min(bad[1], index of each such segment).  The caller initialises bad
 * (device, 2 entries) to {0, UINT64_MAX}; several calls may share it.
 * No value read from device memory is trusted: a segment with seg_off + seg_words > payload_words (tested so that a
 * sum that wraps 64 bits fails too) is never read, counts as a mismatch and has 0 written to crc; a seg_idx entry
 * >= n_segments is skipped, counted in bad[0] and entered into bad[1] as it stands.
 * MH_ERR_ARG, before any device work: payload, seg_off or seg_words NULL; payload not 4-byte aligned; crc and expect
 * both NULL; expect without bad.  n_segments == 0 (or seg_idx with n_idx == 0) enqueues nothing.
 * Only enqueues on `stream`: no synchronisation, allocation or free, so it can be captured into a hipGraph. */
int mhi_seg_crc32(const void *payload, uint64_t payload_words, const uint64_t *seg_off, const uint64_t *seg_words,
                  uint64_t n_segments, const uint64_t *seg_idx, uint64_t n_idx, uint32_t *crc, const uint32_t *expect,
                  uint64_t *bad, void *stream);

/* ---- counts back to events: the inverse of mhi_bin_events ------------------------------------------------------------
 * A matrix of uint8 counts is walked in row-major order and element (i, j) with count k emits k entries, in two passes
 * with ONE read of a number between them: mhi_unbin_count writes total[0], the caller sizes the output from it, and
 * mhi_unbin_emit stores the events.  Any count up to 255 is expanded.
 * MHI_UNBIN_CSR: rows are channels, columns are bins.  Row i is the cols bytes at in + row_off[i] (row_off: device,
 *   rows entries, bytes; rows may start at ANY byte address and no byte outside a row is read).  An event of element
 *   (i, j) is the tick origin + j*period + phase; ev_off[0 .. rows] receives the rows' offsets, and (out_ticks, ev_off)
 *   is the input of mhi_bin_events.  out_ch and ch_bits are not used.
 * MHI_UNBIN_AER: rows are time steps, columns are channels, in = one contiguous [rows, cols] block, row_off = NULL.
 *   An event of element (i, j) is the pair (origin + i*period + phase, j): the tick goes to out_ticks, the channel to
 *   out_ch in ch_bits = 16 or 32 bits (16 needs cols <= 65536).  The list is in time order and in channel order within
 *   a tick: input for mhi_aer_to_csr.  ev_off is not used and may be NULL.
 * period >= 1, phase < period, rows >= 1, cols >= 1 (AER: cols <= 2^32), and the largest tick -- origin + (cols - 1) *
 * period + phase, with rows - 1 in the AER form -- is below 2^63.  The input is cut into tiles of 16 KiB (a CSR row
 * into ceil(cols / 16384) of them); more than 2^32 - 1 tiles are refused.
 * scratch: device, 16-byte aligned, at least mhi_unbin_scratch_bytes(form, rows, cols) bytes; it need not be zeroed,
 * and every cell of it that is read was written by the same mhi_unbin_count, so that calls chain on one scratch.
 * All three return MH_ERR_ARG, before any device work, for a NULL pointer that is used, an unknown form, a row_off that
 * does not fit the form, and any breach of the rules above.
 * count and emit only enqueue on `stream`: no synchronisation, allocation or free, so they can be captured into a
 * hipGraph. */
#define MHI_UNBIN_CSR 0u
#define MHI_UNBIN_AER 1u

/* Bytes of scratch for (form, rows, cols).  Host arithmetic only: no device is needed or touched.  Never 0. */
int mhi_unbin_scratch_bytes(uint32_t form, uint64_t rows, uint64_t cols, uint64_t *bytes);

/* First pass: total[0] = the number of events (device, 1 entry); CSR form: ev_off[0 .. rows] (device) as well.
 * Leaves the 64-bit output base of every tile in the scratch for mhi_unbin_emit. */
int mhi_unbin_count(uint32_t form, const uint8_t *in, const uint64_t *row_off, uint64_t rows, uint64_t cols,
                    uint64_t *ev_off, uint64_t *total, void *scratch, uint64_t scratch_bytes, void *stream);

/* Second pass, on the SAME (form, in, row_off, rows, cols, scratch) as the count before it: out_ticks[0 .. total) and,
 * in the AER form, out_ch[0 .. total).  capacity: the entries out_ticks (and out_ch) hold.  Nothing is ever stored at or
 * behind index capacity, whatever the input holds by then: the events that could not be stored are added to over[0]
 * (device, 1 entry, zeroed by the caller) -- with capacity >= total and an unchanged input over stays 0, every entry
 * below total is written and nothing else.  With total == 0 nothing is written.  out_ticks[0 .. capacity) must not
 * overlap the input. */
int mhi_unbin_emit(uint32_t form, const uint8_t *in, const uint64_t *row_off, uint64_t rows, uint64_t cols,
                   uint64_t origin, uint64_t period, uint64_t phase, uint64_t *out_ticks, void *out_ch, uint32_t ch_bits,
                   uint64_t capacity, uint64_t *over, void *scratch, uint64_t scratch_bytes, void *stream);

/* ---- exact counts: what the codec's clip at S-1 drops, as a sparse side list ----------------------------------------
 * The codec stores min(x, S-1).  An element x > threshold (threshold = S-1) of channel c at sample p is ONE entry of
 * the list: pos = p (uint32, the sample index inside the channel) and val = x - threshold (uint8, 1 .. 254).  The list
 * is canonical: channel-major, ascending pos inside a channel; exc_off[0 .. channels] is its CSR index.  It is made in
 * two passes with ONE read of a number between them, as mhi_unbin_count / mhi_unbin_emit: mhi_excess_count writes
 * total[0] and exc_off, the caller sizes pos / val from total, and mhi_excess_emit stores the entries.
 * MHI_EXCESS_ROWS: rows are channels.  Row i is the bytes at in + row_off[i] (row_off: device, rows entries, bytes; a
 *   row may start at ANY byte address), and its columns [lo[i], min(hi[i], cols)) are examined (lo, hi: device, rows
 *   entries each; NULL stands for 0 and for cols).  No byte outside that window is read, and pos is the column -- not
 *   the column minus lo.  cols is the longest row: rows are cut into tiles of 16 KiB at multiples of 16384 columns.
 * MHI_EXCESS_COLS: in = one contiguous time-major [rows = T, cols = C] block, every column whole: row_off, lo and hi
 *   must be NULL.  Column c is channel c and pos is the row.  The list is, entry for entry, what the ROWS form gives on
 *   the transposed matrix; exc_off has cols + 1 entries.
 * threshold: 1 .. 254.  rows >= 1, cols >= 1, cols < 2^32, and in the COLS form rows < 2^32 (a position is 32-bit); more
 * than 2^32 - 1 pieces (ROWS: rows * ceil(cols / 16384); COLS: cols * ceil(rows / 512)) are refused.
 * scratch: device, 16-byte aligned, at least mhi_excess_scratch_bytes(form, rows, cols) bytes; it need not be zeroed,
 * and every cell of it that is read was written by the same mhi_excess_count, so that calls chain on one scratch.
 * All return MH_ERR_ARG, before any device work, for a NULL pointer that is used, an unknown form, a row_off, lo or hi
 * that does not fit the form, and any breach of the rules above.
 * count, emit and apply only enqueue on `stream`: no synchronisation, allocation or free, so they can be captured into
 * a hipGraph. */
#define MHI_EXCESS_ROWS 0u   /* rows are channels: row i = bytes in + row_off[i], columns [lo[i], hi[i]) examined */
#define MHI_EXCESS_COLS 1u   /* in = one contiguous time-major [rows = T, cols = C] block; every column whole   */

/* Bytes of scratch for (form, rows, cols).  Host arithmetic only: no device is needed or touched.  Never 0, and
 * non-decreasing in rows and in cols. */
int mhi_excess_scratch_bytes(uint32_t form, uint64_t rows, uint64_t cols, uint64_t *bytes);

/* First pass: total[0] = the number of entries (device, 1 entry) and exc_off[0 .. channels] (device; channels = rows in
 * the ROWS form, cols in the COLS form).  Leaves the 64-bit output base of every piece in the scratch. */
int mhi_excess_count(uint32_t form, const uint8_t *in, const uint64_t *row_off, const uint64_t *lo, const uint64_t *hi,
                     uint64_t rows, uint64_t cols, uint32_t threshold, uint64_t *exc_off, uint64_t *total, void *scratch,
                     uint64_t scratch_bytes, void *stream);

/* Second pass, on the SAME (form, in, row_off, lo, hi, rows, cols, threshold, scratch) as the count before it:
 * pos[0 .. total) (device, 4-byte aligned) and val[0 .. total).  capacity: the entries pos and val hold.  Nothing is ever
 * stored at or behind index capacity, whatever the input holds by then: the entries that could not be stored are added
 * to over[0] (device, 1 entry, zeroed by the caller) -- with capacity >= total and an unchanged input over stays 0,
 * every entry below total is written and nothing else.  With total == 0 nothing is written. */
int mhi_excess_emit(uint32_t form, const uint8_t *in, const uint64_t *row_off, const uint64_t *lo, const uint64_t *hi,
                    uint64_t rows, uint64_t cols, uint32_t threshold, uint32_t *pos, uint8_t *val, uint64_t capacity,
                    uint64_t *over, void *scratch, uint64_t scratch_bytes, void *stream);

/* The read side: add a list back onto decoded counts.  Output row i < n_rows takes the entries [first[i], last[i]) of
 * (pos, val) (first, last: device, n_rows entries; n_entries: the entries pos and val hold).  first[i], last[i] and every
 * index are clamped to n_entries, and first >= last is an empty row: repeated and re-ordered channels are just rows.
 * An entry with start <= pos < stop adds val to element b = (pos - start + lead) / r of the row, which lies at
 * (char *)out + i*row_stride + b*col_stride (strides in bytes: channel-major rows, a wide pitched result and a
 * time-major block are all targets).  A row has ceil((stop - start + lead) / r) elements and nothing else is stored to.
 * out_bits = 8: uint8 elements, the sum saturates at 255.  out_bits = 32: 32-bit elements, exact (out and both strides
 * multiples of 4).  start <= stop <= 2^32, 1 <= r <= 2^32, lead < 2^32.
 * The list is untrusted: an entry outside [start, stop) is dropped and no address is formed from a value that was not
 * compared first.  For r > 1 every output element has one owning thread, which searches the row's entries -- they must
 * ascend in pos for the result to be right; it is the same from run to run.  For r == 1 a thread per entry owns its
 * element: duplicate positions -- a corrupt list -- leave those elements unspecified, but every store stays in bounds.
 * The elements must not be written by anything else while the call runs; rows that alias each other are the caller's.
 * MH_ERR_ARG, before any device work: first, last or out NULL; pos or val NULL with n_entries > 0; pos not 4-byte
 * aligned; out_bits other than 8 or 32; r == 0; any breach of the ranges above.  n_rows == 0, n_entries == 0 or
 * start == stop enqueue nothing. */
int mhi_excess_apply(const uint32_t *pos, const uint8_t *val, uint64_t n_entries, const uint64_t *first, const uint64_t *last,
                     uint64_t n_rows, uint64_t start, uint64_t stop, uint64_t r, uint64_t lead, void *out, uint32_t out_bits,
                     uint64_t row_stride, uint64_t col_stride, void *stream);

/* ---- trial-aligned windows: many windows of a matrix of counts in one call, stacked or summed -------------------------
 * in: device.  Row i is the cols bytes at in + i*row_stride, at ANY byte address (a decoded range, a column slice of
 * one, a pitched matrix); no byte outside a row's cols bytes is read.  win_off: device, n_win column indices: window k
 * is the columns [win_off[k], win_off[k] + W) of every row.  It is cut into nb = ceil(W / r) bins from ITS OWN first
 * sample: bin b of window k in row i is the sum of the window's samples [b*r, min(b*r + r, W)) -- the last bin may be
 * cut, as in mh_decode_rebin.
 * MHI_WIN_STACK: element (slot, i, b) at (char *)out + slot*out_win_stride + i*out_row_stride + b*elem, where slot =
 *   win_idx ? win_idx[k] : k (win_idx: NULL, or device, n_win entries: the caller may sort the windows for reading and
 *   keep its own order in the result) and slot < n_out.  out_bits = 8: uint8 elements min(sum, 255).  out_bits = 32:
 *   32-bit elements, the sum itself (modulo 2^32, which only bins of 2^24 samples and more can reach); out and both
 *   strides multiples of 4.  sumsq must be NULL and accumulate 0.  Two windows with the same slot are the caller's
 *   business: one of them wins, every store stays in bounds.
 * MHI_WIN_SUM: out_bits must be 32.  Element (i, b) at (char *)out + i*out_row_stride + 4*b is the sum of the bin value
 *   over the valid windows, and with sumsq (NULL, or device, 8-byte aligned as is sq_row_stride) the uint64 at
 *   (char *)sumsq + i*sq_row_stride + 8*b is the sum of the SQUARES of the per-window bin values -- the square of the
 *   bin's sum, not the sum of the samples' squares.  accumulate = 0 overwrites, 1 adds to what is there (one result
 *   from several calls; the 32-bit bound below is then the caller's).  win_idx, n_out and out_win_stride are ignored.
 * The lists are untrusted: no address is formed from a value that was not compared first.  A window with win_off[k] + W
 * > cols (tested so that a sum that wraps 64 bits fails too) or with a slot >= n_out is skipped: it contributes nothing,
 * nothing is stored for it, bad[0] += 1 and bad[1] = min(bad[1], k).  The caller initialises bad (device, 2 entries)
 * to {0, UINT64_MAX}, as for mhi_seg_crc32; several calls may share it.
 * Every output element has one owner, a thread or a wave, which walks the windows itself: no atomics touch the result
 * and it is the same from run to run.  The elements must not be written by anything else while the call runs.
 * MH_ERR_ARG, before any device work: in, out or bad NULL, win_off NULL with n_win > 0; an unknown mode; out_bits that
 * does not fit the mode; sumsq or accumulate in the STACK form, accumulate above 1; a misaligned 32-bit out or 64-bit
 * sumsq, or a stride of theirs; rows, cols, W or r == 0; W, r or n_win >= 2^32; row_stride < cols with rows > 1; the
 * SUM form without accumulate when n_win * 255 * min(r, W) >= 2^32; rows so large that rows * n_win * nb reaches 2^63.
 * n_win == 0 enqueues nothing in the STACK form and, without accumulate, zero-fills out and sumsq in the SUM form.
 * Only enqueues on `stream`: no synchronisation, allocation or free, so it can be captured into a hipGraph. */
#define MHI_WIN_STACK 0u
#define MHI_WIN_SUM   1u
int mhi_windows(const uint8_t *in, uint64_t row_stride, uint64_t rows, uint64_t cols, const uint64_t *win_off,
                const uint64_t *win_idx, uint64_t n_win, uint64_t n_out, uint64_t W, uint64_t r, uint32_t mode, void *out,
                uint32_t out_bits, uint64_t out_win_stride, uint64_t out_row_stride, uint64_t *sumsq, uint64_t sq_row_stride,
                uint32_t accumulate, uint64_t *bad, void *stream);

/* ---- spike-count covariance: the channel-by-channel Gram matrix of a matrix of counts, exact ---------------------------
 * gram[i][j] (+)= sum over t < cols of a[i][t] * b[j][t]      (int64, exact)
 * sum_a[i]   (+)= sum over t of a[i][t];  sum_b[j] likewise   (int64; NULL = not wanted)
 * a, b: device.  Row i of a is the cols bytes at a + i*a_row_stride, at ANY byte address (a decoded range, a column
 * slice of one, the same matrix shifted by a lag); no byte outside a row's cols bytes is read.  b == NULL: b = a, b_rows
 * and b_row_stride are ignored, only the tiles on or above the diagonal are computed and the result is mirrored, so the
 * output is the full symmetric matrix (and sum_b, if given, receives what sum_a does).  gram[i][j] is the int64 at
 * (char *)gram + i*gram_row_stride + 8*j: a_rows rows of b_rows elements.
 * accumulate = 0 overwrites -- gram and the sums are zeroed on the stream first -- and 1 adds to what is there, so one
 * result can be built from many batches of columns.
 * The products run on the int8 matrix cores over x XOR 0x80 and are corrected exactly in int64; no int32 accumulator
 * sums more than 65536 columns.  The partial results of the runs of columns are added with 64-bit atomics: integer sums
 * do not depend on the order, the result is the same from run to run.  gram and the sums must not be written by
 * anything else while the call runs and must not overlap a or b.
 * MH_ERR_ARG, before any device work: a or gram NULL; a_rows, b_rows (b given) or cols == 0; cols >= 2^40; a_rows or
 * b_rows above 2^31, or so large that tiles x column slices reaches 2^62; a row stride below cols with more than one row;
 * gram or gram_row_stride not a multiple of 8, gram_row_stride below 8*b_rows with more than one row; sum_a or sum_b not
 * 8-byte aligned; accumulate above 1.
 * Only enqueues on `stream`: no synchronisation, allocation or free, so it can be captured into a hipGraph. */
int mhi_gram(const uint8_t *a, uint64_t a_row_stride, uint64_t a_rows, const uint8_t *b, uint64_t b_row_stride, uint64_t b_rows,
             uint64_t cols, int64_t *gram, uint64_t gram_row_stride, int64_t *sum_a, int64_t *sum_b, uint32_t accumulate,
             void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MUAHUFF_INGEST_H */
