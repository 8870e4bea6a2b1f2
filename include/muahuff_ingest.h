/*
 * muahuff_ingest.h -- C ABI of libmuahuff_ingest.so, the front-end companion of libmuahuff.so: stage L0 of the
 * reference's pipeline, spike time stamps -> binned counts, on the MI355X (gfx950).
 *
 * The reference bins per-channel spike times with histogram2 and uint8() (Data/Load_and_bin_Sabes_store_as_mat_file.m:
 * 30-54); its RTL counts detections per BIN_PERIOD clock ticks and holds at SPIKE_RATE_CLIP-1 (FPGA implementation/
 * 1_binner_final.v:19-21).  This library does the RTL's integer-tick form of it and writes either the byte-per-bin
 * channels the codec reads or, directly, the packed 2- / 4-bit chunk-blocked pieces of the stream path -- the
 * time-major block and mh_deinterleave_packed drop out of that path.
 *
 * A binner is not a codec operation, so it is not part of muahuff.h: that ABI is closed.  The conventions are the
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
 * Events before origin or at/after origin + T*period are ignored.  period >= 1, T >= 1, C >= 1, ticks < 2^63;
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

#ifdef __cplusplus
}
#endif
#endif /* MUAHUFF_INGEST_H */
