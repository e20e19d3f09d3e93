/* dega_hip.h -- C ABI of libdega_hip.so: the MI355X (gfx950) implementation of DCLib's DEGA hot path.
 *
 * This is the drop-in boundary for the path  normalize -> diff -> seg -> bac [adaptive]  (and its inverse) of
 * CenterForSecureEnergyInformatics/data-compressor.  Plain C: pointers, sizes and integer codes only; no torch types.
 * Paths below are relative to the reference's DataCompressor/ directory.
 *
 * What each entry point replaces in the reference:
 *   dega_hip_encode_*   the stage functions  EncodeDifferential (DCLib/src/diff.c:9-23)  ->  EncodeSEG (DCLib/src/seg.c:31-43)
 *                       ->  EncodeBAC (DCLib/src/bac.c:147-166)  run back to back by DCCLI's stage loop
 *                       (DCCLI/src/cli.c:430-466) -- one call codes C independent channels instead of one.
 *   dega_hip_decode_*   DecodeBAC (bac.c:244-263) -> DecodeSEG (seg.c:82-94) -> DecodeDifferential (diff.c:25-37).
 *   dega_hip_normalize_* / dega_hip_denormalize_*   Normalize / Denormalize (DCLib/src/normalize.c:9-27, :29-41).
 *   dega_hip_aggregate_* / dega_hip_*encode_agg*     Aggregate (DCLib/src/aggregate.c:9-26, table row DCLib/src/enc_dec.c:52;
 *                       encoder only, as there), alone or in front of the float-entry encoder.
 *   dega_hip_aggregate_levels_* / dega_hip_*encode_levels*   the same stage for several num_values at once, as the
 *                       granularity study runs it: K runs of `encode aggregate num_values=N_k` over the same readings,
 *                       the base series read (and uploaded) once.
 *   dega_hip_csv_write_* / dega_hip_lzmh_encode*_f32_*     WriteCSV (DCLib/src/csv.c:46-65, table row DCLib/src/enc_dec.c:55),
 *                       alone or between `aggregate` and LZMH: the chain `encode aggregate # encode csv # encode lzmh` of
 *                       the granularity study's second codec.
 *   dega_hip_csv_read_* / dega_hip_lzmh_decode_f32_*       ReadCSV (DCLib/src/csv.c:13-44, the same table row), alone or behind
 *                       LZMH: `decode csv`, the first stage of both of the study's chains, and `decode lzmh # decode csv`,
 *                       the inverse of its second.
 *   dega_hip_csv_read_split_*                              ReadCSV again (DCLib/src/csv.c:13-44) with one channel's text split over
 *                       lanes at line starts: the same results for batches of few long channels, one file per meter.
 *   dega_hip_csv_write_split_*                             WriteCSV again (DCLib/src/csv.c:46-65) with one channel's rows split over
 *                       lanes: the same text for batches of few long channels, one file per meter.
 *   dega_hip_*_var_dev (the block "ragged batches")         the same stages over channels of DIFFERENT lengths: what the
 *                       readers and decoders above deliver (a float matrix and a count per channel) goes into
 *                       aggregate, the DEGA float entry, `encode csv` and the LZMH chain as it is, every channel coded as
 *                       the reference codes a file of that channel's own length.
 *   dega_hip_to_time_major_dev / dega_hip_to_channel_major_dev / DEGA_SAMPLES_CHANNEL_MAJOR   nothing of the reference's code: its
 *                       DCCLI codes one file per meter, so its users hold C series, each contiguous (channel-major,
 *                       [C][stride]), while every kernel here reads time-major rows.  The two calls turn one image into
 *                       the other on the device, and the flag lets the host jobs take and return channel-major samples.
 *   the bit format       DCIOLib/src/bit_file_buffer.c:220-248, 297-308 (MSB-first bits, big-endian values).
 * The reference-side binding (a row in encoders_decoders[], DCLib/src/enc_dec.c:51-60, whose enc_dec_function_t
 * (DCLib/inc/enc_dec.h:11) pulls the stream out of in_bit_buf, calls these, and pushes the result into out_bit_buf)
 * is shown in INTEGRATION.md and implemented in data-compressor_amd/host/.
 *
 * Per channel the produced bytes and the exact bit length equal what the reference's chain
 *     encode diff # encode seg # encode bac [adaptive]        (valuesize 1..64)
 * produces for that channel alone; errors are per channel and use the reference's codes (common/inc/err_codes.h:8-32).
 *
 * Layouts
 *   samples  x_tc : int32 [T][ld]   time-major, channel c in column c (ld >= C elements per row; lanes = channels read
 *                                   consecutive int32 -> coalesced 256-byte rows per wavefront)
 *   streams  out  : uint8 [C][cap]  channel c's stream starts at out + c*cap; cap is a multiple of 4
 *            bits : uint64 [C]      exact stream length in bits (the last byte is zero padded)
 *            err  : int32 [C]       DEGA_OK or a negative reference error code for that channel
 *   samples  x_ct : [C][stride]     channel-major, one series after another (stride >= T elements per channel): the
 *                                   transposition calls and, with DEGA_SAMPLES_CHANNEL_MAJOR, the host jobs.  Elements are 4
 *                                   or 8 opaque bytes.  Only the logical C x T region is read or written: the padding of
 *                                   either image keeps what it held.  With a count per channel, element (c, t) with
 *                                   t >= min(count[c], T) is written as zero bits whatever its source holds.
 * "dev" entry points take DEVICE pointers and enqueue on `stream` (a hipStream_t passed as void*, NULL = default
 * stream) without synchronising.  "host" entry points take host pointers and are synchronous; inside they are a
 * pipeline over chunks of channels, and dega_hip_group_* spreads one over every GPU of the node.
 * There is no CPU fallback: without a usable GPU every call fails with DEGA_ERROR_LIBRARY_INIT.
 */
#ifndef DEGA_HIP_H
#define DEGA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Same values as the reference's common/inc/err_codes.h:8-32 */
#define DEGA_OK 0
#define DEGA_ERROR_INVALID_VALUE (-1)   /* diff/normalize range violation (diff.c:17-18, normalize.c:21-22), bad argument */
#define DEGA_ERROR_INVALID_FORMAT (-3)  /* undecodable stream (seg.c:55-56, bac.c:171-186) */
#define DEGA_ERROR_MEMORY (-6)          /* out of device memory, or a channel's stream does not fit its `cap` bytes */
#define DEGA_ERROR_LIBRARY_INIT (-10)   /* no GPU / HIP runtime failure at init */
#define DEGA_ERROR_LIBRARY_CALL (-11)   /* HIP failure during a call */

typedef struct dega_hip_ctx dega_hip_ctx;     /* one context = one device; not thread safe (like the reference's codecs) */
typedef struct dega_hip_group dega_hip_group; /* several contexts: one per GPU of the node, channels split between them */

/* What the samples of a batch are (the `samples` field of dega_hip_job). */
#define DEGA_SAMPLES_I32 0  /* int32 [T][ld], native byte order, valuesize 1..32 */
#define DEGA_SAMPLES_BE32 1 /* the same as 32-bit big-endian words: what `encode normalize` writes and `decode diff` emits
                               for valuesize 32 (DCIOLib/src/bit_file_buffer.c:297-308) -- swapped on the device, not by the caller */
#define DEGA_SAMPLES_I64 2  /* int64 [T][ld], valuesize 33..64 */
#define DEGA_SAMPLES_F32 3  /* float32 [T][ld] readings, valuesize 1..64: Normalize / Denormalize (DCLib/src/normalize.c:9-41)
                               run inside the encode / decode kernel, one launch per direction */

/* OR-ed into `samples`: the host array is channel-major, [C][ld] with ld >= T the pitch between CHANNELS in elements, instead
   of [T][ld] with ld >= C.  Everything else about the job is as without it.  Honoured by dega_hip_encode_job_host,
   dega_hip_decode_job_host, dega_hip_encode_levels_job_host (and through it dega_hip_encode_agg_job_host) and their
   dega_hip_group_* forms; every other call refuses it with DEGA_ERROR_INVALID_VALUE.  A chunk of channels goes up as it
   lies (one contiguous copy when ld == T), is transposed on the device (dega_hip_to_time_major_dev's kernel) and coded
   as ever; decode transposes behind the decoder and downloads into the caller's [C][ld], whose padding it leaves alone.
   With out_count, the tail of every decoded series (t >= out_count[c]) is zero. */
#define DEGA_SAMPLES_CHANNEL_MAJOR 0x100

/* One batch of C channels x T samples for the host-pointer entry points. */
typedef struct dega_hip_job
{
  size_t C, T, ld; /* channels, samples per channel, row pitch of `samples` in elements (>= C; channel-major: >= T) */
  int adaptive;    /* 0 = `bac`, 1 = `bac adaptive` */
  int valuesize;   /* the `valuesize` option of the stages, 1..64 */
  int samples;     /* DEGA_SAMPLES_*, optionally | DEGA_SAMPLES_CHANNEL_MAJOR */
  float factor;    /* normalization_factor (DEGA_SAMPLES_F32 only) */
} dega_hip_job;

/* ---- lifetime ---------------------------------------------------------------------------------------------------- */
int dega_hip_device_count(void);                            /* number of visible GPUs, 0 if none / no runtime */
int dega_hip_create(int device, dega_hip_ctx **ctx);        /* DEGA_OK or DEGA_ERROR_LIBRARY_INIT / _MEMORY */
void dega_hip_destroy(dega_hip_ctx *ctx);
const char *dega_hip_last_error(const dega_hip_ctx *ctx);   /* text of the last failure on this context ("" if none) */
const char *dega_hip_version(void);

/* Bytes per channel that always suffice for T samples (seg worst case 65 bits/sample, bac expansion, EOF + flush). */
size_t dega_hip_worst_case_bytes(size_t T);

/* ---- DEGA encode / decode, device pointers ----------------------------------------------------------------------- */
/* valuesize: 1..32, the `valuesize` option of the three stages (DCLib/src/enc_dec.c:72).  A sample is the low valuesize
   bits of its int32 container, read unsigned as diff.c:15 does; bits above are ignored on encode and zero on decode.
   The difference must fit valuesize bits signed, else that channel reports ERROR_INVALID_VALUE (diff.c:17-18); the
   decoder caps a codeword's zero prefix at valuesize + 1 (seg.c:55-56,74).  33..64: the *64 entry points below.  adaptive: 0 = `bac`, 1 = `bac adaptive`. */
int dega_hip_encode_dev(dega_hip_ctx *ctx, const int32_t *x_tc, size_t C, size_t T, size_t ld, int adaptive, int valuesize,
                        uint8_t *out, size_t cap, uint64_t *out_bits, int32_t *err, void *stream);
/* The same over several calls, each taking the next T_seg rows of the channels (x_tc = the first of them): a channel's
   encoder state -- bit queue, interval and model of EncodeBAC (bac.c:33-37,83-84: the statics a reference process holds
   between symbols), finished bits, the held-back word -- is saved to `state` (dega_hip_encode_state_bytes(C) bytes of
   device memory, owned by the caller, opaque) when flags has DEGA_SEGMENT_MORE and picked up when it has
   DEGA_SEGMENT_CONTINUES; out / cap / out_bits / err as above, the same in every call, final after the last one (the
   one without DEGA_SEGMENT_MORE; T_seg = 0 is allowed there).  The streams are those of one call over all the rows.
   This is how the host pipeline codes a batch of few, long channels while its rows are still arriving (one call per
   band of rows, each behind its band's copy in plain stream order), and how a caller codes series of more than 2^25
   samples. */
#define DEGA_SEGMENT_CONTINUES 1
#define DEGA_SEGMENT_MORE 2
size_t dega_hip_encode_state_bytes(size_t C);
int dega_hip_encode_segment_dev(dega_hip_ctx *ctx, const int32_t *x_tc, size_t C, size_t T_seg, size_t ld, int adaptive, int valuesize,
                                uint8_t *out, size_t cap, uint64_t *out_bits, int32_t *err, void *state, unsigned flags, void *stream);
/* in_bits[c] is the exact bit length, or 8*bytes when the stream comes from a zero-padded file.  Decodes exactly T
   samples per channel; a stream holding fewer or more yields DEGA_ERROR_INVALID_FORMAT for that channel. */
int dega_hip_decode_dev(dega_hip_ctx *ctx, const uint8_t *in, size_t cap, const uint64_t *in_bits, size_t C, size_t T, size_t ld,
                        int adaptive, int valuesize, int32_t *x_tc, int32_t *err, void *stream);

/* Like dega_hip_decode_dev, for streams whose sample count is not known (a DCLib stream has no header: the count is
   implied by the EOF symbol, bac.c:256): decodes up to max_T samples per channel and reports each channel's count in
   out_count[c]; a channel holding more than max_T samples gets DEGA_ERROR_MEMORY (call again with more room).
   What is defined: err[c] of every channel; for a channel with err[c] == 0, out_count[c] and the rows below it.  Not
   defined (here and in every other decode entry that reports counts): the rows at or beyond a channel's count, and the
   count and the whole column of a channel with err[c] != 0 -- a damaged stream is given up wherever the first check
   trips, and how much of it has been written by then depends on the waves' timing.  Nothing outside the C columns and the
   max_T rows is ever written. */
int dega_hip_decode_var_dev(dega_hip_ctx *ctx, const uint8_t *in, size_t cap, const uint64_t *in_bits, size_t C, size_t max_T, size_t ld,
                            int adaptive, int valuesize, int32_t *x_tc, uint64_t *out_count, int32_t *err, void *stream);

/* ---- valuesize 33..64: the same path with 64-bit containers -------------------------------------------------------- */
/* x_tc is int64 [T][ld]; a sample is the low valuesize bits, unsigned; for valuesize 64 the difference wraps and is not
   range checked (diff.c:17); a difference of magnitude 2^63 is coded like 0 (the reference's code number wraps, seg.c:25-28)
   -- the one lossy case, reproduced.  The decoder caps the zero prefix at min(valuesize + 1, 64) (seg.c:74).
   Slabs: dega_hip_worst_case_bytes64. */
size_t dega_hip_worst_case_bytes64(size_t T);
int dega_hip_encode64_dev(dega_hip_ctx *ctx, const int64_t *x_tc, size_t C, size_t T, size_t ld, int adaptive, int valuesize,
                          uint8_t *out, size_t cap, uint64_t *out_bits, int32_t *err, void *stream);
int dega_hip_decode64_dev(dega_hip_ctx *ctx, const uint8_t *in, size_t cap, const uint64_t *in_bits, size_t C, size_t T, size_t ld,
                          int adaptive, int valuesize, int64_t *x_tc, int32_t *err, void *stream);
int dega_hip_decode64_var_dev(dega_hip_ctx *ctx, const uint8_t *in, size_t cap, const uint64_t *in_bits, size_t C, size_t max_T, size_t ld,
                              int adaptive, int valuesize, int64_t *x_tc, uint64_t *out_count, int32_t *err, void *stream);
int dega_hip_encode64_host(dega_hip_ctx *ctx, const int64_t *x_tc, size_t C, size_t T, size_t ld, int adaptive, int valuesize,
                           uint8_t *out, size_t cap, uint64_t *out_bits, int32_t *err);
int dega_hip_decode64_var_host(dega_hip_ctx *ctx, const uint8_t *in, size_t cap, const uint64_t *in_bits, size_t C, size_t max_T, size_t ld,
                               int adaptive, int valuesize, int64_t *x_tc, uint64_t *out_count, int32_t *err);

/* ---- float entry / exit (normalize.c), device pointers ----------------------------------------------------------- */
/* v: float32 [T][ld] -> x: int32 [T][ld]; err[c] = DEGA_ERROR_INVALID_VALUE if any sample of channel c fails the range check.
   A NaN fails no comparison of that check and is a value like any other, as in the reference: the field 0 (at valuesize 64,
   through the fused entry below, 0x8000000000000000 -- what the reference's conversion gives).  Infinities are out of
   range.  Subnormal readings, products and quotients are IEEE: kept, not flushed. */
int dega_hip_normalize_dev(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, float factor, int valuesize,
                           int32_t *x_tc, int32_t *err, void *stream);
int dega_hip_denormalize_dev(dega_hip_ctx *ctx, const int32_t *x_tc, size_t C, size_t T, size_t ld, float factor, int valuesize,
                             float *v_tc, void *stream);

/* ---- stream compaction: [C][cap] slabs -> one contiguous buffer --------------------------------------------------- */
/* offsets[c] (uint64 [C+1], device) = byte offset of channel c in `packed`; a channel occupies ceil(bits/8) bytes.
   Two steps so that the caller can size `packed`: _offsets fills offsets (exclusive prefix sum, offsets[C] = total),
   _gather copies. */
int dega_hip_compact_offsets_dev(dega_hip_ctx *ctx, const uint64_t *bits, size_t C, uint64_t *offsets, void *stream);
int dega_hip_compact_gather_dev(dega_hip_ctx *ctx, const uint8_t *slabs, size_t cap, const uint64_t *offsets, size_t C,
                                uint8_t *packed, void *stream);

/* ---- synthetic load profiles: deterministic integer random walk, generated on the device ------------ */
/* x[c][0] = 10000 + h(c) mod 50000;  x[c][t] = clamp(x[c][t-1] + (h(c,t) mod (2S+1)) - S, 0, 2^31-1);  channel ids start at
   c0 (so that rank r of a multi-GPU job generates its own channel range). */
int dega_hip_synth_dev(dega_hip_ctx *ctx, int32_t *x_tc, size_t C, size_t T, size_t ld, uint64_t seed, uint64_t c0, uint32_t S, void *stream);

/* ---- LZMH, the reference's second codec (BASELINE config 4) ------------------------------------------------------- */
/* Replaces EncodeLZMH (DCLib/src/lzmh.c:130-370) and DecodeLZMH (:383-574), table row "lzmh" (DCLib/src/enc_dec.c:51-60),
   per channel and bit for bit, including the codec's quirks (an input of exactly 403 bytes encodes to nothing, :161-174;
   the decoder stops once its code register is empty after the last input bit, :571).  One GPU lane per channel.
   encode: in = uint8 [C][stride] (device, 16-byte aligned, stride a multiple of 16), in_len[c] <= stride bytes of channel c;
           out = uint8 [C][cap] slabs of 32-bit big-endian words (cap a multiple of 16, >= 48; >= dega_hip_lzmh_worst_case_bytes(n)
           never overflows), out_bits[c] = exact bit length, err[c] = 0 | ERROR_MEMORY (slab too small) | ERROR_INVALID_VALUE.
           When a slab is too small: a channel is coded whenever its stream, rounded up to whole 32-bit words, and 16 bytes
           more fit cap (dega_hip_lzmh_worst_case_bytes leaves 32); it reports ERROR_MEMORY and out_bits 0 whenever the
           rounded stream does not fit cap; in between either, and a status of 0 always comes with the whole stream.  Nothing
           is written outside a channel's slab, nor, when it is coded, behind its stream's last word; what a channel that
           reports ERROR_MEMORY leaves in its slab is unspecified.  Bytes behind in_len[c] are read but change nothing.
   decode: the inverse: in/cap/in_bits as produced by encode (cap a multiple of 4), out = uint8 [C][stride] (stride a
           multiple of 8), out_len[c] = decoded bytes; ERROR_MEMORY when a channel does not fit its row.
   render: the synthetic LZMH workload of SURVEY.md 8(d): int32 channels [T][ld] (centi-units) as ASCII "%d.%02d\n" lines. */
size_t dega_hip_lzmh_worst_case_bytes(size_t n);
int dega_hip_lzmh_encode_dev(dega_hip_ctx *ctx, const uint8_t *in, size_t stride, const uint64_t *in_len, size_t C, uint8_t *out, size_t cap,
                             uint64_t *out_bits, int32_t *err, void *stream);
int dega_hip_lzmh_decode_dev(dega_hip_ctx *ctx, const uint8_t *in, size_t cap, const uint64_t *in_bits, size_t C, uint8_t *out, size_t stride,
                             uint64_t *out_len, int32_t *err, void *stream);
int dega_hip_lzmh_render_dev(dega_hip_ctx *ctx, const int32_t *x_tc, size_t C, size_t T, size_t ld, uint8_t *out, size_t stride,
                             uint64_t *out_len, int32_t *err, void *stream);
/* The same for host memory, synchronous, chunked as dega_hip_aggregate_host is (a chunk holds its texts and its slabs).
   C = 0: DEGA_OK, ahead of everything else.  Before the device is touched both refuse, with DEGA_ERROR_INVALID_VALUE and a
   message in last_error, a null array and the stride and cap the _dev forms refuse (the alignment of the device arrays
   is the library's own concern).  encode brings home, per chunk, as many bytes of every slab as the chunk's longest stream
   has: what a slab holds beyond its stream's end is unspecified. */
int dega_hip_lzmh_encode_host(dega_hip_ctx *ctx, const uint8_t *in, size_t stride, const uint64_t *in_len, size_t C, uint8_t *out, size_t cap,
                              uint64_t *out_bits, int32_t *err);
int dega_hip_lzmh_decode_host(dega_hip_ctx *ctx, const uint8_t *in, size_t cap, const uint64_t *in_bits, size_t C, uint8_t *out, size_t stride,
                              uint64_t *out_len, int32_t *err);
/* The same for a group, through the host pipeline: chunks of channels on their own streams (upload, kernel, pack, download
   overlapped), contiguous channel ranges per device, streams packed back to back: channel c at packed[offsets[c] ..
   offsets[c+1]) (C + 1 offsets, ceil(bits / 8) bytes each).  Host memory; pinned memory is used in place.  encode returns
   ERROR_MEMORY with the size needed in offsets[C] when packed_cap is too small; stride as for the _dev forms. */
int dega_hip_group_lzmh_encode(dega_hip_group *group, const uint8_t *in, size_t stride, const uint64_t *in_len, size_t C, uint8_t *packed,
                               size_t packed_cap, uint64_t *offsets, uint64_t *out_bits, int32_t *err);
int dega_hip_group_lzmh_decode(dega_hip_group *group, const uint8_t *packed, const uint64_t *offsets, const uint64_t *in_bits, size_t C, uint8_t *out,
                               size_t stride, uint64_t *out_len, int32_t *err);

/* ---- float entry / exit fused into the coder kernels, device pointers ----------------------------------- */
/* v_tc: float32 [T][ld].  One launch: Normalize on each value as it enters the fill phase (normalize.c:16-24; a value
   failing the range check of :21 gives that channel DEGA_ERROR_INVALID_VALUE; a NaN passes it and is coded as the field 0,
   at valuesize 64 as 0x8000000000000000), then diff -> seg -> bac as above.  No int32
   intermediate exists in HBM.  valuesize 1..64.  decode: Denormalize (:36-38) in the row write; out_count NULL = exactly
   T samples per channel, else up to T and the counts are reported. */
int dega_hip_encode_f32_dev(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, float factor, int adaptive, int valuesize,
                            uint8_t *out, size_t cap, uint64_t *out_bits, int32_t *err, void *stream);
int dega_hip_decode_f32_dev(dega_hip_ctx *ctx, const uint8_t *in, size_t cap, const uint64_t *in_bits, size_t C, size_t T, size_t ld,
                            float factor, int adaptive, int valuesize, float *v_tc, uint64_t *out_count, int32_t *err, void *stream);

/* ---- aggregate: coarser granularities of the same readings (DCLib/src/aggregate.c:9-26) --------------------------------- */
/* v_tc: float32 [T][ld] -> a_tc: float32 [T_out][ld_out], T_out = dega_hip_aggregate_rows(T, num_values) = ceil(T / num_values).
   Per channel, a_tc[j] is the sum of readings j*num_values .. min((j+1)*num_values, T) - 1 exactly as aggregate.c:13-22
   forms it: a float32 accumulator that starts at +0.0f and takes the readings from left to right, one rounding per add --
   bit for bit the reference's floats (a NaN is a NaN; payloads are not promised).  The last group is short when
   num_values does not divide T (the reference stops at the end of its input, aggregate.c:21-22); num_values > T gives
   one row, the sum of all T.  num_values = 1 is not a copy: 0.0f + v turns -0.0f into +0.0f, as in the reference.
   Subnormal inputs and sums are kept.  A coarser level is always computed from the base series (sums of sums round
   differently).  One lane owns a (channel, output row) pair; nothing is reassociated.
   num_values = 0 gives DEGA_ERROR_INVALID_VALUE from every entry point below before anything is launched -- the
   reference does not terminate on it (its inner loop reads nothing, aggregate.c:16), which is not reproduced.
   T = 0 or C = 0: nothing is launched, DEGA_OK.  ld >= C, ld_out >= C; a_tc may not overlap v_tc.  There is no decoder,
   as in the reference: streams coded behind an aggregation decode with dega_hip_decode_f32_* and T_out. */
size_t dega_hip_aggregate_rows(size_t T, size_t num_values); /* ceil(T / num_values); 0 when num_values == 0 */
int dega_hip_aggregate_dev(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, size_t num_values, float *a_tc, size_t ld_out,
                           void *stream);
/* Host memory, synchronous: chunks of channels go through the context's first slot one after the other (upload, one
   launch, download) -- as many channels at a time as keep what a chunk holds on the device, here the two images, within
   1 GiB; at least 1, and whole fours from 4 on.  DEGA_HOST_CHUNK_BYTES=n (n >= 1; a measurement and test knob, read by
   every call) replaces the 1 GiB.  The other synchronous host forms -- dega_hip_csv_write_host, dega_hip_csv_read_host,
   dega_hip_lzmh_encode_host, dega_hip_lzmh_decode_host -- run the same loop. */
int dega_hip_aggregate_host(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, size_t num_values, float *a_tc, size_t ld_out);
/* `encode aggregate num_values=N # encode normalize # encode diff # encode seg # encode bac [adaptive]` per channel.  It
   IS dega_hip_encode_levels_f32_dev (below) with K = 1 and takes that call's path: two launches on `stream`, no
   synchronisation -- the aggregate kernel into a scratch of T_out x ld floats (rounded up to four) that the context
   owns, then the float-entry encoder over the T_out sums.  Calls on one context may use different streams like those of
   the other `dev` entry points: the scratch is shared, so a call on another stream than the previous one makes its
   stream wait (hipStreamWaitEvent; the host does not wait) until that call's encode launch has read it -- such calls
   run one after the other on the device.  The scratch only grows, by doubling; a block it has outgrown is never freed
   under a kernel that may still read it: it is kept until the context is destroyed (together less than the live block).  out / cap / out_bits / err as there; cap is
   judged against T_out (dega_hip_worst_case_bytes(T_out) always suffices), and so is the limit of 2^25 samples per
   channel.  num_values = 1 is coded straight from v_tc, without the aggregate launch: Normalize maps both zeros to 0,
   the streams are those of dega_hip_encode_f32_dev.  num_values = 0 is refused here, with aggregate's message. */
int dega_hip_encode_agg_f32_dev(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, size_t num_values, float factor, int adaptive,
                                int valuesize, uint8_t *out, size_t cap, uint64_t *out_bits, int32_t *err, void *stream);

/* ---- aggregate: several granularities from one pass over the base series ------------------------------------------------- */
/* K levels num_values[0 .. K) over the same readings, in the caller's order; outputs are arrays of K pointers / sizes in
   that order.  Level k's result is bit for bit what dega_hip_aggregate_dev / dega_hip_encode_agg_f32_dev gives for
   num_values[k] alone: every level is summed from the BASE series (K independent float32 accumulators per channel, each
   takes every row; a coarser level is never formed from a finer one's sums, which round differently).  What changes is
   the traffic: levels that share a pass are computed from one read of v_tc.
   Which levels share a pass is decided by dega_hip_aggregate_levels_plan (no GPU needed): a pass cuts the base rows into
   ranges of step_of[p] rows, a multiple of every N of the pass, so a level joins a pass only while the least common
   multiple still leaves enough ranges to fill the device; else it gets a pass of its own, and a pass of one level is the
   single-level launch.  The worst case is K passes: what K calls do.  Returns the number of passes (pass_of[k] in
   0 .. passes - 1, step_of[p] base rows per range; for wide != 0 and C a multiple of 4 the 16-byte form's workgroup count
   is assumed), or DEGA_ERROR_INVALID_VALUE.  The environment variable DEGA_AGG_LEVELS_MIN_WORKGROUPS=n (a measurement and
   test knob; n = 1 lets levels share a pass whatever the batch size) replaces the workgroup floor of 512, in this
   function and in every call that plans passes; results do not depend on it, only which kernel computes them.
   Refused with DEGA_ERROR_INVALID_VALUE before anything is launched: K > DEGA_AGG_MAX_LEVELS, a num_values[k] of 0, the
   same num_values twice, null or misaligned arrays, ld < C, ld_out[k] < C, an output that overlaps v_tc or another
   level's output.  K = 0, C = 0 or T = 0: nothing is launched, DEGA_OK. */
#define DEGA_AGG_MAX_LEVELS 8
int dega_hip_aggregate_levels_plan(size_t C, size_t T, const size_t *num_values, size_t K, int wide, int *pass_of, size_t *step_of);
int dega_hip_aggregate_levels_dev(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, const size_t *num_values, size_t K,
                                  float *const *a_tc, const size_t *ld_out, void *stream);
/* K x `encode aggregate num_values=N_k # encode normalize # encode diff # encode seg # encode bac [adaptive]`: the passes
   into the context's aggregate scratch (every level's sums 16-byte aligned), then K launches of the float-entry encoder
   on the same stream, level k over ceil(T / N_k) rows into out[k] / out_bits[k] / err[k] with cap[k] bytes per channel.
   The scratch and its protocol are described at dega_hip_encode_agg_f32_dev, which is this call with K = 1 (the event is
   recorded behind the last encode launch).  A level with num_values 1 is coded straight from v_tc.  cap[k] and the limit
   of 2^25 samples are judged against level k's rows. */
int dega_hip_encode_levels_f32_dev(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, const size_t *num_values, size_t K,
                                   float factor, int adaptive, int valuesize, uint8_t *const *out, const size_t *cap, uint64_t *const *out_bits,
                                   int32_t *const *err, void *stream);

/* ---- encode csv: a float32 series as text (WriteCSV, DCLib/src/csv.c:46-65) ------------------------------------------------ */
/* v_tc: float32 [T][ld] -> out: uint8 [C][stride], channel c's text at out + c * stride, out_len[c] bytes of it: for every
   reading `column - 1` copies of separator_char (csv.c:56-59), then what sprintf("%.*f\n", num_decimal_places, value)
   writes (csv.c:60), byte for byte as glibc prints it: a '-' exactly when the sign BIT is set (-0.0f gives -0.00, a NaN
   with the bit set -nan), inf / nan without decimals, else the exact value of the float rounded half-to-even to
   `decimals` = num_decimal_places = 0 .. 6 (DCLib/src/enc_dec.c:69) places, every integer digit printed (FLT_MAX has 39),
   no decimal point at 0 decimals, subnormals included.  Integer arithmetic only.  One limit of the reference is NOT
   reproduced: its line buffer has 48 bytes (csv.c:11), so it overruns on lines of 48 characters and more (negative values
   of magnitude 1e38 and above at 6 decimals); the device writes what printf would write.
   The layout is the one dega_hip_lzmh_encode_dev takes as it is: out 16-byte aligned, stride a multiple of 16 (16 ..
   0x7FFFFFF0).  A channel's text fits when text + 16 bytes <= stride (the room its last, partly filled store needs);
   one that does not fit gets err[c] = DEGA_ERROR_MEMORY and out_len[c] = 0, the others are unaffected.  Bytes of a row
   beyond out_len[c] are unspecified.  dega_hip_csv_line_max: the longest line (column - 1 + '-' + 39 digits + '.' +
   decimals + '\n'; 48 at 6 decimals in column 1); dega_hip_csv_worst_case_bytes: a stride that can never overflow,
   T x line_max + 16 rounded up to 16 -- six times what two-decimal meter readings need (about 8 bytes per value).
   Both are pure host code and return 0 for decimals > 6, column 0 or a size beyond size_t.
   Refused with DEGA_ERROR_INVALID_VALUE before anything is launched: decimals > 6, column 0 (or so many empty columns
   that no line fits stride), separator_char outside 0 .. 255, a misaligned out or stride, ld < C, null arrays, out
   overlapping v_tc.  C = 0 or T = 0: nothing is launched, DEGA_OK, lengths 0.
   The environment variable DEGA_CSV_STORE=8|64 (a measurement and test knob) picks how the kernel stores its text --
   8-byte stores straight from a register, or 64-byte blocks staged in LDS; the bytes are the same.
   `decode csv` is dega_hip_csv_read_* below. */
size_t dega_hip_csv_line_max(unsigned decimals, size_t column);
size_t dega_hip_csv_worst_case_bytes(size_t T, unsigned decimals, size_t column);
int dega_hip_csv_write_dev(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, unsigned decimals, size_t column, int separator_char,
                           uint8_t *out, size_t stride, uint64_t *out_len, int32_t *err, void *stream);
/* The same for host memory, synchronous: chunks of channels are uploaded, rendered and downloaded (as dega_hip_aggregate_host). */
int dega_hip_csv_write_host(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, unsigned decimals, size_t column, int separator_char,
                            uint8_t *out, size_t stride, uint64_t *out_len, int32_t *err);
/* `encode csv # encode lzmh` per channel on `stream`, no synchronisation: the renderer into a text scratch that the
   context owns (text_stride bytes per channel, as `stride` above), dega_hip_lzmh_encode_dev over it, and a third, tiny
   launch that hands the renderer's status on (the LZMH kernel, left as it is, would code an overflowed channel as the
   empty text): a channel whose text outgrows text_stride reports DEGA_ERROR_MEMORY with out_bits 0.  text_stride comes
   from the caller because the worst case is six times what meter readings need and would not fit the device at
   64 Ki x 86 400.  out / cap / out_bits / err as dega_hip_lzmh_encode_dev; text_len (may be NULL) receives each channel's
   text bytes, the denominator of the study's compression ratio.  The scratch follows the protocol of
   dega_hip_encode_agg_f32_dev's: grow-only by doubling, outgrown blocks kept until the context goes, and a call on
   another stream than the previous one waits on the device (hipStreamWaitEvent) until that call's last launch has read
   the text; the host never waits.  There is no `aggregate` in this chain: a -0.0f reading prints -0.00. */
int dega_hip_lzmh_encode_f32_dev(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, unsigned decimals, size_t column,
                                 int separator_char, size_t text_stride, uint8_t *out, size_t cap, uint64_t *out_bits, uint64_t *text_len, int32_t *err,
                                 void *stream);
/* K x `encode aggregate num_values=N_k # encode csv # encode lzmh`: the passes of dega_hip_aggregate_levels_plan into the
   aggregate scratch exactly as dega_hip_encode_levels_f32_dev runs them, then per level the renderer, the LZMH encoder
   and the status launch on the same stream, level k over ceil(T / N_k) sums with text_stride[k] into out[k] (cap[k]
   bytes per channel) / out_bits[k] / text_len[k] / err[k].  text_len may be NULL, and so may any text_len[k].  The text
   scratch is sized for the largest level and reused level after level (stream order makes that safe); the aggregate
   scratch's event is recorded behind the last renderer, the text scratch's behind the last launch.  This entry point
   means the chain WITH `aggregate` in it: a level with num_values 1 goes through the aggregate kernel like any other
   (+0.0f + v: a -0.0f reading prints 0.00), unlike dega_hip_encode_levels_f32_dev, where Normalize hides the difference
   and num_values 1 is coded from the base rows.  Refused before anything is launched: what the calls above refuse, K >
   DEGA_AGG_MAX_LEVELS, a num_values of 0 or twice, null arrays, two levels' outputs overlapping. */
int dega_hip_lzmh_encode_levels_f32_dev(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, const size_t *num_values, size_t K,
                                        unsigned decimals, size_t column, int separator_char, const size_t *text_stride, uint8_t *const *out,
                                        const size_t *cap, uint64_t *const *out_bits, uint64_t *const *text_len, int32_t *const *err, void *stream);

/* ---- decode csv: text as a float32 series (ReadCSV, DCLib/src/csv.c:13-44) ------------------------------------------------ */
/* text: uint8 [C][stride] with len[c] bytes of channel c at text + c * stride (the layout dega_hip_csv_write_dev and
   dega_hip_lzmh_decode_dev produce; text 16-byte aligned, stride a multiple of 16, 16 .. 0x7FFFFFF0) -> v_tc: float32
   [max_T][ld], channel c in column c, and out_count[c] values of it: the floats the reference writes for that text, in
   order, with identical bit patterns -- signs of zero, NaN signs and payloads, subnormals and infinities included.
   Splitting is csv.c:20-42 as it stands: a field ends at separator_char, at '\n' or at the last byte of the text; only
   fields of column `column` are converted and '\n' resets the column to 1; a line with fewer fields yields no value, an
   empty selected field +0.0f; and the last byte of the text is appended to a selected field whatever it is (csv.c:25-26).
   Conversion is what glibc's strtof returns for the field in the C locale (csv.c:32): leading white space, a sign, then
   the longest valid prefix of a decimal number (an exponent counts only with a digit in it), a hexadecimal one (0x, p
   exponent; glibc's handling of the bit behind the 24th in subnormal hexadecimal results included), inf / infinity, nan,
   nan(n-char-sequence) with glibc's payload (0x7fc00000 | strtoull(sequence, 0) & 0x3fffff when the whole sequence is a
   number); no conversion gives +0.0f even behind a '-'; overflow gives an infinity, underflow a correctly rounded
   subnormal or zero.  Rounding is to nearest, ties to even, on the exact decimal value of all the field's digits.
   Integer arithmetic only.  One limit of the reference is NOT reproduced: its field buffer has 48 bytes (csv.c:11,18), so
   it overruns on a selected field of 48 or more characters (the appended last byte counts, the terminator does not); such
   a channel gets err[c] = DEGA_ERROR_INVALID_FORMAT, out_count[c] = the values in front of that field, and stops there;
   its neighbours are unaffected.  So the longest line `encode csv` can write (47 characters + '\n') is readable
   everywhere except as the very last line of a text, where the newline is appended to it.
   The number of values depends on the data.  A channel with more than max_T values keeps counting without storing: it gets
   DEGA_ERROR_MEMORY and out_count[c] = the room it needs (the convention of dega_hip_decode_var_*: call again with more
   room).  max_T = 0 is legal and counts only (v_tc may be NULL then).  Rows at or beyond out_count[c] in column c are
   unspecified; columns C .. ld - 1 are not written.
   Refused with DEGA_ERROR_INVALID_VALUE before anything is launched: a null context, column 0, separator_char outside
   0 .. 255, ld < C, a misaligned text / stride / len / out_count / err / v_tc, null arrays, v_tc overlapping text, and --
   where the host can see it, in the host form -- a len[c] above stride (the device form gives such a channel
   DEGA_ERROR_INVALID_VALUE and no value).  C = 0: nothing is launched, DEGA_OK.  No synchronisation. */
int dega_hip_csv_read_dev(dega_hip_ctx *ctx, const uint8_t *text, size_t stride, const uint64_t *len, size_t C, size_t column, int separator_char,
                          float *v_tc, size_t max_T, size_t ld, uint64_t *out_count, int32_t *err, void *stream);
/* The same from and to host memory, synchronous: chunks of channels are uploaded, read and downloaded (as
   dega_hip_csv_write_host; no pipeline, no group).  Rows beyond a channel's count come back as +0.0f.  The call does not
   know the counts beforehand: it holds and downloads min(max_T, stride) rows for every channel (a text of `stride` bytes
   has no more values than that; rows of v_tc beyond them are not written), so max_T is best taken from a counting call
   (max_T = 0) or from what wrote the text. */
int dega_hip_csv_read_host(dega_hip_ctx *ctx, const uint8_t *text, size_t stride, const uint64_t *len, size_t C, size_t column, int separator_char,
                           float *v_tc, size_t max_T, size_t ld, uint64_t *out_count, int32_t *err);
/* dega_hip_csv_read_dev for few long channels: the same arguments, the same err[c], out_count[c] and rows below
   min(out_count[c], max_T) of every channel, bit for bit (the three statuses above included); rows at or beyond a channel's
   count are unspecified.  One channel's text is split over lanes, so that a single channel spreads over the whole device.
   Ownership: a channel's len[c] bytes are cut into blocks of block_bytes, block b covering bytes [b * block_bytes,
   (b + 1) * block_bytes), and a block owns exactly the lines that START inside it -- a line starts at byte 0 or at a byte
   whose predecessor is '\n', where the reader's state is always column 1 and an empty field (csv.c:27-41).  A lane whose
   block starts mid-line skips to just behind the first '\n' of its block (none, or one on the block's last byte: it owns
   nothing), then runs csv.c:22-41 byte by byte, past its block's end if need be, and stops behind the first '\n' whose
   successor lies in a later block or behind byte len[c] - 1, which is appended to a selected field and ends it whatever it
   is (csv.c:23-26).  Three launches on `stream`, no synchronisation: a count of every block's values, a scan per channel
   (each block's first row; the channel stops behind its first block with a field of 48 characters or more; out_count and
   err), and the conversion, which is not launched for max_T = 0.  The counts between them live in a scratch of the context
   with the protocol of the text scratch of dega_hip_lzmh_encode_f32_dev (grow-only, an event behind the last launch, a
   call on another stream waits for it on the device).
   block_bytes: 0 takes dega_hip_csv_read_split_block_bytes(C, stride); otherwise a multiple of 16, at least 16; a value
   above stride is one block per channel.  Anything else, and everything dega_hip_csv_read_dev refuses, is
   DEGA_ERROR_INVALID_VALUE before anything is launched; a scratch that cannot be had is DEGA_ERROR_MEMORY.  C = 0: nothing
   is launched, DEGA_OK.  dega_hip_csv_read_dev, _host and dega_hip_lzmh_decode_f32_dev do not come here. */
int dega_hip_csv_read_split_dev(dega_hip_ctx *ctx, const uint8_t *text, size_t stride, const uint64_t *len, size_t C, size_t column,
                                int separator_char, float *v_tc, size_t max_T, size_t ld, uint64_t *out_count, int32_t *err,
                                size_t block_bytes, void *stream);
/* the library's choice of block_bytes for a batch (pure host code, no GPU): a multiple of 16 in 16 .. max(16, stride) -- the
   largest block that still gives the batch enough (channel, block) pairs to fill the device, not below a floor; for a fixed
   stride it does not decrease as C grows.  0 for a stride that dega_hip_csv_read_dev refuses. */
size_t dega_hip_csv_read_split_block_bytes(size_t C, size_t stride);
/* `decode lzmh # decode csv` per channel on `stream`, no synchronisation: the inverse of dega_hip_lzmh_encode_f32_dev.
   dega_hip_lzmh_decode_dev, left as it is, writes into the context's text scratch (text_stride bytes per channel, a
   multiple of 16; its protocol and its event are those of dega_hip_lzmh_encode_f32_dev), the reader runs over that text,
   and a third, tiny launch merges the two statuses: a channel whose text outgrew text_stride reports DEGA_ERROR_MEMORY
   and out_count 0, not a parse of half a text.  in / cap / in_bits as dega_hip_lzmh_decode_dev; text_len (may be NULL)
   receives each channel's text bytes; v_tc / max_T / ld / out_count / err as dega_hip_csv_read_dev. */
int dega_hip_lzmh_decode_f32_dev(dega_hip_ctx *ctx, const uint8_t *in, size_t cap, const uint64_t *in_bits, size_t C, size_t text_stride, size_t column,
                                 int separator_char, float *v_tc, size_t max_T, size_t ld, uint64_t *out_count, uint64_t *text_len, int32_t *err,
                                 void *stream);

/* ---- ragged batches: a count per channel through aggregate, encode and csv, device pointers -------------------------------- */
/* Meter files differ in length (gaps, start dates, new meters), and dega_hip_csv_read_dev, dega_hip_lzmh_decode_f32_dev and
   the decoders' out_count report it: a matrix [max_T][ld] and a count per channel.  These entry points take exactly that.
   count: device uint64 [C], 8-byte aligned.  Channel c is rows 0 .. count[c] - 1 of column c of v_tc [T][ld]; T is the
   number of rows the matrix has (the reader's max_T).  Rows t >= count[c] of column c may be LOADED but influence no
   output and no status, whatever they hold (NaN, infinities, values outside Normalize's range: the readers leave them
   unspecified).  Every channel's result is bit for bit what the uniform twin gives for that channel alone with
   T = count[c] -- what the reference's chain gives on count[c] floats; padding a short channel instead would change the
   last sum of every level and the stream.  count[c] = 0 is the reference's result on an empty input: `aggregate` writes
   nothing, `... # encode bac adaptive` gives the 3 bits 0x20 (`... # encode bac`: what dega_hip_encode_f32_dev gives for
   T = 0), `encode csv # encode lzmh` 0 bits.  count[c] > T gives that channel DEGA_ERROR_INVALID_VALUE, no output and
   output counts / lengths / bits of 0; its neighbours are unaffected.  Host-side refusals, alignment rules, the scratch
   buffers with their event protocol and the stream semantics are the uniform twin's; in addition a null or misaligned
   count / out_count[k] and T >= 2^32 are refused, and C != 0 with T = 0 still launches (the counts decide).  A count
   goes together with a segment state through dega_hip_encode_segment_var_dev alone (integer samples, below).
   Cost: a wave walks rows up to the largest count among its 64 channels.  The aggregate's loop is the uniform kernel's
   while every lane of the wave still has rows and selects per lane behind that; the coder's filling wave takes its
   straight-line batch only while every lane still has a full batch of rows, and the general per-row writer from the
   wave's shortest channel on.  Sorting channels by length is the caller's business. */
/* K = 1 .. DEGA_AGG_MAX_LEVELS levels; one level is this call with K = 1.  Level k receives rows 0 .. out_count[k][c] - 1 of
   column c of a_tc[k], out_count[k][c] = ceil(count[c] / num_values[k]) (out_count[k]: device uint64 [C]); rows beyond
   are not promised (they are left as they were).  a_tc[k] needs the rows T allows, dega_hip_aggregate_rows(T,
   num_values[k]).  Passes are planned by dega_hip_aggregate_levels_plan on T, as for dega_hip_aggregate_levels_dev; every
   pass, single-level ones included, runs the counted kernel.  err: device int32 [C]. */
int dega_hip_aggregate_levels_var_dev(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, const uint64_t *count,
                                      const size_t *num_values, size_t K, float *const *a_tc, const size_t *ld_out, uint64_t *const *out_count,
                                      int32_t *err, void *stream);
/* dega_hip_encode_f32_dev over a ragged batch: valuesize 1 .. 64; cap and the limit of 2^25 samples are judged against T. */
int dega_hip_encode_f32_var_dev(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, const uint64_t *count, float factor, int adaptive,
                                int valuesize, uint8_t *out, size_t cap, uint64_t *out_bits, int32_t *err, void *stream);
/* dega_hip_encode_dev / dega_hip_encode64_dev over a ragged batch: one meter per channel, each stream ending where its
   input ends, which is the reference's ordinary case (one file per meter: diff.c:12-21 reads until the input is out,
   seg.c:34-41 and bac.c:152-162 end the stream there).  Channel c's status, bit length and bytes are those of the uniform
   twin on that channel alone with T = count[c]; rows at or beyond count[c] reach neither the stream, nor the range checks
   of diff.c:17-18, nor the last value.  They are the inverse of dega_hip_decode_var_dev / dega_hip_decode64_var_dev.
   samples: DEGA_SAMPLES_I32 or DEGA_SAMPLES_BE32 (byte-swapped words); valuesize 1 .. 32 (encode64: int64 samples,
   33 .. 64).  Refusals are the uniform twin's (T > 2^25 among them) and those of the counts above. */
int dega_hip_encode_var_dev(dega_hip_ctx *ctx, const int32_t *x_tc, size_t C, size_t T, size_t ld, const uint64_t *count, int adaptive, int valuesize,
                            int samples, uint8_t *out, size_t cap, uint64_t *out_bits, int32_t *err, void *stream);
int dega_hip_encode64_var_dev(dega_hip_ctx *ctx, const int64_t *x_tc, size_t C, size_t T, size_t ld, const uint64_t *count, int adaptive, int valuesize,
                              uint8_t *out, size_t cap, uint64_t *out_bits, int32_t *err, void *stream);
/* dega_hip_encode_segment_dev over a ragged batch: this launch holds rows row0 .. row0 + T_seg - 1 of series of T_total
   rows, x_tc points at row row0.  count and T_total are the same in every call of a series; a channel's own rows in a
   launch are those below its count, clamp(count[c] - row0, 0, T_seg), a channel that ended in an earlier launch adds
   nothing, and the end of every stream still comes from the last launch (the one without DEGA_SEGMENT_MORE).  count[c] >
   T_total is the verdict of every launch.  The streams are those of dega_hip_encode_var_dev over all T_total rows.
   Refused beside the twin's refusals and the counts': row0 + T_seg > T_total, T_total > 2^25. */
int dega_hip_encode_segment_var_dev(dega_hip_ctx *ctx, const int32_t *x_tc, size_t C, size_t T_seg, size_t ld, const uint64_t *count, size_t row0,
                                    size_t T_total, int adaptive, int valuesize, uint8_t *out, size_t cap, uint64_t *out_bits, int32_t *err, void *state,
                                    unsigned flags, void *stream);
/* dega_hip_encode_levels_f32_dev over a ragged batch: dega_hip_aggregate_levels_var_dev into the aggregate scratch, then the
   counted encoder per level with that level's counts.  out_count[k] is required: it is the intermediate, and what the
   caller needs to decode level k (dega_hip_decode_f32_dev with out_count).  A level with num_values 1 is coded from v_tc
   with `count` itself (out_count[k] receives it, 0 where it is above T).  cap[k] is judged against the rows T allows for level k. */
int dega_hip_encode_levels_f32_var_dev(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, const uint64_t *count,
                                       const size_t *num_values, size_t K, float factor, int adaptive, int valuesize, uint8_t *const *out,
                                       const size_t *cap, uint64_t *const *out_bits, uint64_t *const *out_count, int32_t *const *err, void *stream);
/* dega_hip_csv_write_dev over a ragged batch: channel c's text is its first count[c] readings. */
int dega_hip_csv_write_var_dev(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, const uint64_t *count, unsigned decimals,
                               size_t column, int separator_char, uint8_t *out, size_t stride, uint64_t *out_len, int32_t *err, void *stream);
/* dega_hip_csv_write_dev (count == NULL) and dega_hip_csv_write_var_dev (count: channel c is its first count[c] readings,
   count[c] > T is DEGA_ERROR_INVALID_VALUE and length 0) for few long channels: the same out_len[c], err[c] and bytes
   [0, out_len[c]) of every row, byte for byte.  The unit of work is a (channel, block of rows) pair: block b of channel c
   owns rows [b * block_rows, min((b + 1) * block_rows, n_c)), n_c being T or count[c].  Three launches on `stream`, no
   synchronisation: the lengths of every block's lines, per channel their exclusive prefix (with out_len and err; a channel
   fits iff text + 16 <= stride, else DEGA_ERROR_MEMORY and length 0), and the text, every block at its byte offset -- not
   launched for T = 0.  Stricter than the unsplit call: NO byte of `out` at or beyond out_len[c] is written, and nothing at
   all of a channel that reports an error.  The words between the launches live in a scratch of the context with the
   protocol of the text scratch of dega_hip_lzmh_encode_f32_dev (grow-only, an event behind the last launch, a call on
   another stream waits for it on the device).
   block_rows: 0 takes dega_hip_csv_write_split_block_rows(C, T); any value from 1 on is legal, one at or above T is one
   block per channel.  Everything dega_hip_csv_write_dev / _var_dev refuse, more than 2^32 - 1 blocks per channel, more
   pairs than one launch takes, and block_rows = 0 at T >= 2^32 are DEGA_ERROR_INVALID_VALUE before anything is launched; a
   scratch that cannot be had is DEGA_ERROR_MEMORY.  C = 0: nothing is launched, DEGA_OK.  T = 0: the lengths are 0 and
   nothing is launched (with a count, the two launches that report count[c] > 0).  dega_hip_csv_write_dev, _host, _var_dev
   and the dega_hip_lzmh_encode*_f32* chains do not come here. */
int dega_hip_csv_write_split_dev(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, const uint64_t *count /* may be NULL */,
                                 unsigned decimals, size_t column, int separator_char, uint8_t *out, size_t stride, uint64_t *out_len, int32_t *err,
                                 size_t block_rows, void *stream);
/* the library's choice of block_rows for a batch (pure host code, no GPU): within 1 .. max(1, T) -- the largest block that
   still gives the batch enough (channel, block) pairs to fill the device, not below a floor; for a fixed T it does not
   decrease as C grows.  0 for a T that dega_hip_csv_write_var_dev refuses (2^32 and more). */
size_t dega_hip_csv_write_split_block_rows(size_t C, size_t T);
/* dega_hip_lzmh_encode_levels_f32_dev over a ragged batch -- the chain WITH `aggregate` in it, as its twin: every level,
   num_values 1 included, through the counted aggregate kernel, then per level the counted renderer, the LZMH encoder and the
   status launches.  out_count[k] is required (level k's values per channel: what dega_hip_lzmh_decode_f32_dev reports
   back); text_len may be NULL, and so may any text_len[k]. */
int dega_hip_lzmh_encode_levels_f32_var_dev(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, const uint64_t *count,
                                            const size_t *num_values, size_t K, unsigned decimals, size_t column, int separator_char,
                                            const size_t *text_stride, uint8_t *const *out, const size_t *cap, uint64_t *const *out_bits,
                                            uint64_t *const *text_len, uint64_t *const *out_count, int32_t *const *err, void *stream);

/* ---- channel-major <-> time-major, device pointers ------------------------------------------------------------------------ */
/* x_ct [C][stride] -> x_tc [T][ld] and back: x_tc[t][c] = x_ct[c][t] for c < C, t < T, elements of elem_bytes = 4 or 8 opaque
   bytes (float32 / int32 / big-endian int32; int64).  Nothing outside the logical region of the destination is written:
   columns C .. ld - 1 of a time-major row and T .. stride - 1 of a channel-major row keep what they held.  count (device
   uint64 [C], as in the ragged entry points; NULL = uniform): element (c, t) with t >= min(count[c], T) is written as
   all-zero bits; its source element may be read but influences nothing (it may be NaN or uninitialised).  Both enqueue one
   kernel on `stream` without synchronising; pitches may be odd and the bases need only the element's alignment (16-byte
   loads and stores are used on each side whose base and pitch allow them).  DEGA_ERROR_INVALID_VALUE with nothing written:
   elem_bytes other than 4 or 8, ld < C or stride < T, a pointer not aligned to the element or a count not aligned to 8,
   source and destination ranges that overlap.  C == 0 or T == 0: DEGA_OK, nothing launched. */
int dega_hip_to_time_major_dev(dega_hip_ctx *ctx, const void *x_ct, size_t C, size_t T, size_t stride, size_t elem_bytes, const uint64_t *count,
                               void *x_tc, size_t ld, void *stream);
int dega_hip_to_channel_major_dev(dega_hip_ctx *ctx, const void *x_tc, size_t C, size_t T, size_t ld, size_t elem_bytes, const uint64_t *count,
                                  void *x_ct, size_t stride, void *stream);

/* ---- A-XDR: packed fields, the reference's third coding (`decode csv # encode normalize`) ---------------------------------- */
/* Every reading of a channel as one big-endian two's-complement field of `valuesize` bits, packed MSB first, what Normalize
   writes and Denormalize reads (DCLib/src/normalize.c:9-41), in the container of the DEGA streams: uint8 [C][cap] slabs of
   big-endian 32-bit words, the exact bit length per channel.  Rows are time-major [T][ld]; samples is DEGA_SAMPLES_F32
   (valuesize 1..64; `factor` matters for it alone), DEGA_SAMPLES_I32 (1..32) or DEGA_SAMPLES_I64 (33..64): integer rows
   hold fields in their low valuesize bits -- what lies above is ignored on the way in and zero on the way out.

   dega_hip_axdr_bytes: 4 * ceil(T * valuesize / 32), the bytes of a slab that T fields take; 0 for T = 0, a valuesize outside
   1..64, or a product that does not fit size_t.

   encode, per channel, with n = count ? count[c] : T (count: device uint64 [C], may be NULL): out_bits[c] = n * valuesize,
   the slab's first dega_hip_axdr_bytes(n, valuesize) bytes hold the stream, zero padded to the word, and no other byte of
   the slab is written.  err[c] = DEGA_ERROR_INVALID_VALUE if a reading among the first n fails the range check of
   normalize.c:21 -- the reference stops there, so bits and bytes of that channel are then not defined, but nothing outside
   its dega_hip_axdr_bytes(T, valuesize) bytes is written.  NaNs, infinities and subnormals: as dega_hip_normalize_dev.  Rows
   at or behind n may be loaded but influence nothing.  count[c] > T: DEGA_ERROR_INVALID_VALUE and 0 bits; a stream that does
   not fit cap: DEGA_ERROR_MEMORY and 0 bits; both with nothing written and the neighbours untouched.  out_bits feeds
   dega_hip_compact_offsets_dev / _gather_dev as it is.

   decode, per channel: out_count[c] = in_bits[c] / valuesize fields go to rows 0 .. of column c -- floats sign-extended and
   divided by the factor, integers with zero above the field; err[c] = 0, or DEGA_ERROR_LIBRARY_CALL (-11, what the
   reference's reader answers to a stream that ends inside a field) where in_bits[c] is no multiple of valuesize,
   DEGA_ERROR_MEMORY where the count is above max_T (out_count[c] = the room needed), DEGA_ERROR_INVALID_VALUE where
   in_bits[c] > 8 * cap.  Not defined, by the convention of dega_hip_decode_var_dev: rows at or beyond a channel's count, and
   the column of a channel with err != 0.  Nothing outside the C columns and max_T rows is written, and no bit at or beyond
   in_bits[c] influences anything.

   Refused with DEGA_ERROR_INVALID_VALUE before the device is touched, by the host forms too: a null context;
   DEGA_SAMPLES_BE32, DEGA_SAMPLES_CHANNEL_MAJOR or an unknown sample type; a valuesize that does not go with it; ld < C; a
   cap that is no multiple of 4; more than 2^32 - 1 rows; null or misaligned arrays (C != 0).  C = 0: DEGA_OK.  The _dev
   forms enqueue a memset of err and one kernel (decode: one kernel) on `stream` without synchronising.

   dega_hip_axdr_encode_levels_f32_dev: the study's third chain, `decode csv # encode aggregate # encode normalize`, for up to
   DEGA_AGG_MAX_LEVELS granularities from one upload -- dega_hip_encode_levels_f32_dev with the pack in the coder's place
   (aggregate into the context's scratch, then one pack per level; num_values 1 packs v_tc itself).  count NULL: the uniform
   form, out_count is not looked at; else the counts that dega_hip_csv_read_dev reports, and out_count[k][c] =
   ceil(count[c] / num_values[k]).

   The host forms take host pointers, are synchronous and run chunks of channels through the context's first slot (the budget
   of a chunk: DEGA_HOST_CHUNK_BYTES); of a slab only the stream's own bytes come back. */
size_t dega_hip_axdr_bytes(size_t T, int valuesize);
int dega_hip_axdr_encode_dev(dega_hip_ctx *ctx, const void *x_tc, int samples, size_t C, size_t T, size_t ld, const uint64_t *count, float factor,
                             int valuesize, uint8_t *out, size_t cap, uint64_t *out_bits, int32_t *err, void *stream);
int dega_hip_axdr_decode_dev(dega_hip_ctx *ctx, const uint8_t *in, size_t cap, const uint64_t *in_bits, size_t C, size_t max_T, size_t ld, float factor,
                             int valuesize, int samples, void *x_tc, uint64_t *out_count, int32_t *err, void *stream);
int dega_hip_axdr_encode_levels_f32_dev(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, const uint64_t *count,
                                        const size_t *num_values, size_t K, float factor, int valuesize, uint8_t *const *out, const size_t *cap,
                                        uint64_t *const *out_bits, uint64_t *const *out_count, int32_t *const *err, void *stream);
int dega_hip_axdr_encode_host(dega_hip_ctx *ctx, const void *x_tc, int samples, size_t C, size_t T, size_t ld, const uint64_t *count, float factor,
                              int valuesize, uint8_t *out, size_t cap, uint64_t *out_bits, int32_t *err);
int dega_hip_axdr_decode_host(dega_hip_ctx *ctx, const uint8_t *in, size_t cap, const uint64_t *in_bits, size_t C, size_t max_T, size_t ld, float factor,
                              int valuesize, int samples, void *x_tc, uint64_t *out_count, int32_t *err);

/* ---- host pointers: the pipelined path DCCLI's stage loop (DCCLI/src/cli.c:430-466) ends up on ---------------------------- */
/* `samples` and the outputs are HOST memory (pageable or pinned).  The batch is cut into chunks of channels, each on a
   stream of its own: upload of its columns, kernels, packing, download of its stream bytes -- copies and kernels of
   different chunks overlap, device and pinned buffers belong to the context and only grow, and only stream bytes come
   back: channel c occupies packed[offsets[c] .. offsets[c+1]) (ceil(bits / 8) bytes, channel order; offsets has C + 1
   entries).  If packed_cap is too small the call returns DEGA_ERROR_MEMORY with the size needed in offsets[C] (bits and err
   are valid then).  decode: the inverse; out_count NULL = every channel holds exactly T samples, else up to T and the
   counts are reported (a DCLib stream has no header: bac.c:256). */
int dega_hip_encode_job_host(dega_hip_ctx *ctx, const dega_hip_job *job, const void *samples, uint8_t *packed, size_t packed_cap,
                             uint64_t *offsets, uint64_t *out_bits, int32_t *err);
int dega_hip_decode_job_host(dega_hip_ctx *ctx, const dega_hip_job *job, const uint8_t *packed, const uint64_t *offsets, const uint64_t *in_bits,
                             void *samples, uint64_t *out_count, int32_t *err);
/* dega_hip_encode_job_host over a ragged batch -- series of different lengths in host memory, the reference's one file per
   meter (diff.c:12-21, seg.c:34-41, bac.c:152-162: every stream ends where its input ends).  count: HOST array of job->C
   uint64; channel c is the first count[c] samples of its column (of its row, with DEGA_SAMPLES_CHANNEL_MAJOR), and what
   lies behind them in `samples` is uploaded with the rest but influences nothing.  All four sample types, both layouts,
   and every path of the uniform job: chunks of channels (each with its share of the counts), pinned rows read in place,
   bands of rows, the worst-case pass over a chunk whose stream outgrew its slab.  Channel c's bits, err and bytes are
   those of the uniform job on that channel alone with T = count[c]; count[c] > job->T gives it DEGA_ERROR_INVALID_VALUE,
   0 bits and no bytes.  It takes what dega_hip_decode_job_host reports in out_count.  A null count with C != 0 is
   refused.  Not offered: counts with num_values != 1 or levels, series packed back to back with starts[C + 1], skipping
   the upload of rows that no count reaches, sorting channels by length. */
int dega_hip_encode_var_job_host(dega_hip_ctx *ctx, const dega_hip_job *job, const uint64_t *count, const void *samples, uint8_t *packed,
                                 size_t packed_cap, uint64_t *offsets, uint64_t *out_bits, int32_t *err);
/* dega_hip_encode_job_host with the aggregation of aggregate.c in front: job->samples must be DEGA_SAMPLES_F32 (anything
   else, and num_values = 0, give DEGA_ERROR_INVALID_VALUE with nothing written), job->T is the fine-grained length.
   num_values = 1 is dega_hip_encode_job_host itself.  Any larger num_values is dega_hip_encode_levels_job_host (below)
   with K = 1 and takes that call's path: every chunk of channels goes up whole, is summed, coded over
   ceil(T / num_values) rows, packed and downloaded.  The upload is num_values times what the coder sees, so the link sets
   the time.  `samples` must then be 4-byte aligned, as a float array is: a misaligned pointer gives
   DEGA_ERROR_INVALID_VALUE.  A packed_cap that is too small gives DEGA_ERROR_MEMORY with the size needed in offsets[C],
   bits and err valid, as above. */
int dega_hip_encode_agg_job_host(dega_hip_ctx *ctx, const dega_hip_job *job, size_t num_values, const void *samples, uint8_t *packed,
                                 size_t packed_cap, uint64_t *offsets, uint64_t *out_bits, int32_t *err);
/* dega_hip_encode_agg_job_host for K levels: job->samples must be DEGA_SAMPLES_F32, job->T is the fine length.  Every
   chunk of channels is UPLOADED ONCE, summed by the plan's passes, then coded, sized, gathered and downloaded level by
   level: level k's streams arrive in packed[k] (packed_cap[k] bytes) with offsets[k] (C + 1 entries), out_bits[k] and
   err[k] exactly as K calls of dega_hip_encode_agg_job_host would deliver them.  A packed_cap[k] that is too small
   gives DEGA_ERROR_MEMORY with the size needed in offsets[k][C]; the other levels are still delivered.  A
   DEGA_ERROR_MEMORY whose last_error names a failed call instead is an allocation that failed: no output is valid then. */
int dega_hip_encode_levels_job_host(dega_hip_ctx *ctx, const dega_hip_job *job, const size_t *num_values, size_t K, const void *samples,
                                    uint8_t *const *packed, const size_t *packed_cap, uint64_t *const *offsets, uint64_t *const *out_bits,
                                    int32_t *const *err);

/* ---- every GPU of the node: channel ranges per device, host-side concatenate, no collective ------------------------------- */
/* Channels are independent units (every stream starts from last_value = 0, DCLib/src/diff.c:11, and InitModel(),
   DCLib/src/bac.c:150), so a batch shards as contiguous channel ranges [g*C/G, (g+1)*C/G): one context, one host thread
   and one set of streams per device; every device packs its own streams and copies them to their final place in `packed`
   once the sizes of the ranges in front of it are known.  Same arguments and results as the single-context calls above --
   a group of one IS that call.  devices NULL / n <= 0: every visible device, or the comma separated list in the
   environment variable DEGA_DEVICES (DEGA_DEVICE for a single index). */
/* The partition itself (no GPU needed): cuts[g] .. cuts[g+1] is device g's channel range, cuts has G + 1 entries; ranges
   are whole 512-channel workgroup pairs where the batch is large enough. */
int dega_hip_split_channels(size_t C, int G, size_t *cuts);
int dega_hip_group_create(const int *devices, int n, dega_hip_group **group);
void dega_hip_group_destroy(dega_hip_group *group);
int dega_hip_group_size(const dega_hip_group *group);
dega_hip_ctx *dega_hip_group_context(dega_hip_group *group, int i); /* member i (for the LZMH calls, profiling, last_error) */
const char *dega_hip_group_last_error(const dega_hip_group *group);
int dega_hip_group_encode(dega_hip_group *group, const dega_hip_job *job, const void *samples, uint8_t *packed, size_t packed_cap,
                          uint64_t *offsets, uint64_t *out_bits, int32_t *err);
int dega_hip_group_decode(dega_hip_group *group, const dega_hip_job *job, const uint8_t *packed, const uint64_t *offsets, const uint64_t *in_bits,
                          void *samples, uint64_t *out_count, int32_t *err);
/* as dega_hip_encode_var_job_host: the counts are split with the channels */
int dega_hip_group_encode_var(dega_hip_group *group, const dega_hip_job *job, const uint64_t *count, const void *samples, uint8_t *packed,
                              size_t packed_cap, uint64_t *offsets, uint64_t *out_bits, int32_t *err);
int dega_hip_group_encode_agg(dega_hip_group *group, const dega_hip_job *job, size_t num_values, const void *samples, uint8_t *packed,
                              size_t packed_cap, uint64_t *offsets, uint64_t *out_bits, int32_t *err);
/* as dega_hip_encode_agg_job_host: num_values = 1 is dega_hip_group_encode, any larger one dega_hip_group_encode_levels
   with K = 1, several members included (below). */
/* as dega_hip_encode_levels_job_host.  With more than one member each of them delivers its share of each level into a
   host buffer of its own, and packed[k] is filled by host-side copies once the sizes in front are known (coarse streams
   are small).  More than one member on DISTINCT devices is unverified (tested with two members on one device). */
int dega_hip_group_encode_levels(dega_hip_group *group, const dega_hip_job *job, const size_t *num_values, size_t K, const void *samples,
                                 uint8_t *const *packed, const size_t *packed_cap, uint64_t *const *offsets, uint64_t *const *out_bits,
                                 int32_t *const *err);

/* Pinned host memory for callers that can keep their samples there: copies then run at link speed without the
   runtime's staging of pageable memory.  NULL when there is no GPU runtime. */
void *dega_hip_pinned_alloc(size_t bytes);
void dega_hip_pinned_free(void *p);

/* ---- host pointers, the earlier forms (slabs in and out; the same pipeline underneath) --------------------------------- */
int dega_hip_encode_host(dega_hip_ctx *ctx, const int32_t *x_tc, size_t C, size_t T, size_t ld, int adaptive, int valuesize,
                         uint8_t *out, size_t cap, uint64_t *out_bits, int32_t *err);
int dega_hip_decode_host(dega_hip_ctx *ctx, const uint8_t *in, size_t cap, const uint64_t *in_bits, size_t C, size_t T, size_t ld,
                         int adaptive, int valuesize, int32_t *x_tc, int32_t *err);
int dega_hip_decode_var_host(dega_hip_ctx *ctx, const uint8_t *in, size_t cap, const uint64_t *in_bits, size_t C, size_t max_T, size_t ld,
                             int adaptive, int valuesize, int32_t *x_tc, uint64_t *out_count, int32_t *err);
/* The same encode, streams returned packed: channel c occupies packed[offsets[c] .. offsets[c+1]) -- ceil(bits/8) bytes, in
   channel order, which is how DCCLI-style callers concatenate them anyway -- so only the stream bytes cross PCIe, not
   C x cap slab bytes.  offsets has C + 1 entries; if packed_cap is too small the call returns DEGA_ERROR_MEMORY with the
   size needed in offsets[C] (bits and err are valid then). */
int dega_hip_encode_packed_host(dega_hip_ctx *ctx, const int32_t *x_tc, size_t C, size_t T, size_t ld, int adaptive, int valuesize,
                                uint8_t *packed, size_t packed_cap, uint64_t *offsets, uint64_t *out_bits, int32_t *err);
/* The inverse: channel c's stream is packed[offsets[c] .. offsets[c+1]) (at least ceil(in_bits[c] / 8) bytes); out_count NULL
   = every channel holds exactly T samples, else up to T and the counts are reported (as dega_hip_decode_var_host). */
int dega_hip_decode_packed_host(dega_hip_ctx *ctx, const uint8_t *packed, const uint64_t *offsets, const uint64_t *in_bits, size_t C, size_t T,
                                size_t ld, int adaptive, int valuesize, int32_t *x_tc, uint64_t *out_count, int32_t *err);
/* float32 channels in, DEGA streams out: Normalize runs inside the encode kernel, Denormalize inside the decode kernel
   (one launch per direction, valuesize 1..64). */
int dega_hip_encode_f32_host(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, float factor, int adaptive, int valuesize,
                             uint8_t *out, size_t cap, uint64_t *out_bits, int32_t *err);
int dega_hip_decode_f32_host(dega_hip_ctx *ctx, const uint8_t *in, size_t cap, const uint64_t *in_bits, size_t C, size_t T, size_t ld,
                             float factor, int adaptive, int valuesize, float *v_tc, int32_t *err);

int dega_hip_decode_f32_var_host(dega_hip_ctx *ctx, const uint8_t *in, size_t cap, const uint64_t *in_bits, size_t C, size_t max_T, size_t ld,
                                 float factor, int adaptive, int valuesize, float *v_tc, uint64_t *out_count, int32_t *err);

/* ---- measurement hook ---------------------------------------------------------------------------------------------- */
/* Average duration in milliseconds of the DEGA encode (which=0) / DEGA decode (1) / LZMH encode (2) / LZMH decode (3) kernel launches enqueued since the last
   reset, measured with hipEvents on the stream each launch used (enabled with dega_hip_profile(ctx, 1)); returns the
   number of launches measured.  Used by bench.py for the roofline figure. */
int dega_hip_profile(dega_hip_ctx *ctx, int enable);
int dega_hip_profile_read(dega_hip_ctx *ctx, int which, double *avg_ms, int reset);

#ifdef __cplusplus
}
#endif

#endif
