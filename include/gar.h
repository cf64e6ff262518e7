/*
 * gar.h -- C ABI of the MI355X-native polyphase-FIR resampling engine.
 *
 * Drop-in boundary for tphakala/go-audio-resampler's resampling path: every
 * entry point below replaces one Go entry point (cited path:line relative to
 * the reference repo) and keeps its argument meaning, output lengths, state
 * semantics and error behaviour.  A cgo shim implementing the Go
 * `resampler.Resampler` interface over this ABI is given in INTEGRATION.md.
 *
 * Plain C types only: pointers, sizes, doubles.  Host-memory entry points
 * (the cgo path) copy through the GPU; the *_device entry points take
 * device-resident buffers and a HIP stream (hipStream_t passed as void*).
 *
 * Streams: interleaved multi-channel data uses element (t, c) at
 * base[t * frame_stride + c * channel_stride]  (interleaved: (C, 1);
 * planar with pitch P: (1, P)).
 */
#ifndef GAR_H
#define GAR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gar_resampler gar_resampler;

/* Status codes map 1:1 to the Go sentinels (resample.go:156-165). */
typedef enum gar_status {
    GAR_OK = 0,
    GAR_ERR_INVALID_CONFIG = 1,   /* ErrInvalidConfig   resample.go:158 */
    GAR_ERR_BUFFER_TOO_SMALL = 2, /* ErrBufferTooSmall  resample.go:161 -- returned before any state change */
    GAR_ERR_NOT_SUPPORTED = 3,    /* ErrNotSupported    resample.go:164 */
    GAR_ERR_CHANNEL_MISMATCH = 4, /* "expected %d channels, got %d" constant.go:205-207 */
    GAR_ERR_DEVICE = 5,           /* HIP runtime failure / no MI355X visible */
    GAR_ERR_INTERNAL = 6,         /* EstimateOutput underestimate (the Go code panics, constant.go:340-342) */
    GAR_ERR_INVALID_ARGUMENT = 7  /* NULL handle / bad channel index ("channel %d out of range" constant.go:256) */
} gar_status;

/* resampler.QualityPreset (resample.go:104-131) */
enum { GAR_QUALITY_QUICK = 0, GAR_QUALITY_LOW = 1, GAR_QUALITY_MEDIUM = 2, GAR_QUALITY_HIGH = 3,
       GAR_QUALITY_VERYHIGH = 4, GAR_QUALITY_CUSTOM = 5 };
/* resampler.QualityFlags (resample.go:133-153) */
enum { GAR_FLAG_NO_INTERPOLATION = 1, GAR_FLAG_MINIMUM_PHASE = 2, GAR_FLAG_LINEAR_PHASE = 4,
       GAR_FLAG_ALLOW_ALIASING = 8, GAR_FLAG_NO_SIMD = 16 };
/* sample / compute types.  Compute: GAR_F64 (the reference's float64), GAR_F32 (float32-class:
 * f16-split products on the f16 matrix cores, f32 accumulation, error <= exact-f32 arithmetic's
 * for full-scale material; the fixed input split scale 2^12 gives inputs an ABSOLUTE precision
 * floor of about 2^-47 (f16 subnormals), so material quieter than ~2^-26 (-156 dBFS) loses the
 * relative precision the reference's float64 New path keeps -- choose GAR_F64 or GAR_F32_EXACT
 * for such signals; |x| >= 16, Inf and NaN are recomputed exactly in f64),
 * GAR_F32_EXACT (exact f32 products on the f32 matrix cores). */
enum { GAR_F64 = 0, GAR_F32 = 1, GAR_F32_EXACT = 2 };
/* integer PCM sample types of the device entry points (in_dtype / out_dtype of gar_process_device
 * and gar_flush_device), after cmd/resample-wav/main.go:444-543: input sample i -> float64(i) *
 * (1 / maxVal) in the compute type; output y -> int(clamp(float64(y), -1, 1) * maxVal) (truncation),
 * maxVal = 32767 (PCM16, int16 storage), 8388607 (PCM24, int32 storage), 2147483647 (PCM32, int32).
 * Fused into the split-f16 kernel's loads and stores for single-stage float32 plans; staged
 * through a conversion kernel otherwise. */
enum { GAR_PCM16 = 16, GAR_PCM24 = 24, GAR_PCM32 = 32 };
/* half-precision sample types of the device entry points (in_dtype / out_dtype of gar_process_device
 * and gar_flush_device only; independent of each other and of the compute type: f16 in / f32 out,
 * PCM16 in / bf16 out, ... are all legal).  IEEE binary16 and bfloat16, 2 bytes per sample; the value
 * 3 stays unassigned.  They are not compute types: gar_config_validate, gar_new and gar_new_batch
 * answer GAR_ERR_INVALID_CONFIG for them as compute_dtype.  The host-memory entry points have no
 * half form (Go has no half type).
 *   input:  exact widening to the compute type.  f16 subnormals are values (not flushed); Inf and
 *           NaN enter the non-finite handling and |x| >= 16 the loud handling described for GAR_F32.
 *   output: ONE round-to-nearest-even from the compute type to the half type.  Values past the
 *           largest finite half become +-Inf (no clamp, unlike PCM); NaN stays NaN (payload
 *           unspecified); subnormal results are produced, not flushed.  With float64 compute the
 *           rounding is f64 -> half directly (f64 -> f32 to odd, then f32 -> half to nearest-even),
 *           never f64 -> f32 -> half with two nearest roundings.
 * Fused into the split-f16 kernel's loads and stores wherever PCM is (a stereo frame is one dword,
 * like a PCM16 frame); staged through the conversion kernel otherwise. */
enum { GAR_F16 = 4, GAR_BF16 = 5 };
/* packed 24-bit PCM, the layout of 24-bit WAV data (cmd/resample-wav/main.go:648-665 WriteSamples24:
 * byte(s), byte(s>>8), byte(s>>16)): a sample type of the device entry points only (in_dtype /
 * out_dtype of gar_process_device and gar_flush_device; input and output types stay independent:
 * packed in / f32 out, PCM16 in / packed out, f16 in / packed out are all legal).  As compute_dtype
 * gar_config_validate, gar_new and gar_new_batch answer GAR_ERR_INVALID_CONFIG.
 *   layout: 3 bytes per sample, little-endian, two's complement.  frame_stride and channel_stride
 *           count SAMPLES, i.e. units of 3 bytes: sample (t, c) occupies the bytes
 *           base + 3 * (t * frame_stride + c * channel_stride) + {0, 1, 2}.  The base pointer needs
 *           no alignment (the vector conversion kernels take a 4-byte aligned base of an interleaved
 *           contiguous buffer; any other base or layout runs the byte-wise kernel, same results).
 *   values: exactly GAR_PCM24's.  In: the 3 bytes sign-extended, then float64(i) * (1 / 8388607).
 *           Out: int(clamp(y, -1, 1) * 8388607), truncating, NaN -> 0; its low three bytes stored.
 *   bounds: no call reads or writes a byte outside the frames x channels samples the strides
 *           describe -- no vector load reaches past the last frame, no store touches the byte
 *           after a sample (or the gap bytes of a strided layout).
 * Always staged through the pack / unpack kernels around the float path (not fused into the FIR
 * kernel's loads and stores). */
enum { GAR_PCM24_PACKED = 0x100 | 24 };
/* engine.Quality (internal/engine/filter_params.go:16-41), for gar_design_engine */
enum { GAR_ENGINE_QUICK = 0, GAR_ENGINE_LOW, GAR_ENGINE_MEDIUM, GAR_ENGINE_HIGH, GAR_ENGINE_VERYHIGH,
       GAR_ENGINE_16BIT, GAR_ENGINE_20BIT, GAR_ENGINE_24BIT, GAR_ENGINE_28BIT, GAR_ENGINE_32BIT };

/* resampler.QualitySpec (resample.go:77-102) */
typedef struct gar_quality_spec {
    int32_t preset;
    int32_t precision;
    double phase_response;
    double passband_end;
    double stopband_begin;
    uint32_t flags;
} gar_quality_spec;

/* resampler.Config (resample.go:46-73) + three engine extensions. */
typedef struct gar_config {
    double input_rate;
    double output_rate;
    int32_t channels;
    gar_quality_spec quality;
    int64_t max_input_size;
    int32_t enable_simd;
    int32_t enable_parallel;
    /* extensions (zero = reference behaviour) */
    int32_t compute_dtype; /* GAR_F64 (the New path computes in float64, constant.go:121-146), GAR_F32, GAR_F32_EXACT */
    int32_t device;        /* HIP device ordinal */
    int32_t dry_run;       /* 1: host state machine only, no GPU work; process calls report lengths only */
} gar_config;

/* resampler.Info (resample.go:294-316) */
typedef struct gar_info {
    char algorithm[32];
    int32_t filter_length;
    int32_t phases;
    int32_t latency;
    int64_t memory_usage;
    int32_t simd_enabled;
    char simd_type[48];
} gar_info;

/* ---- construction -------------------------------------------------------- */
/* Config.Validate (resample.go:168-214). */
gar_status gar_config_validate(const gar_config *cfg);
/* GetPresetSpec (resample.go:217-267). */
gar_quality_spec gar_preset_spec(int32_t preset);
/* resampler.New (resample.go:272-292).  Like the Go code, a non-custom preset
 * is expanded into cfg->quality (resample.go:282-284). */
gar_status gar_new(gar_config *cfg, gar_resampler **out);
/* n_streams independent New(cfg) resamplers processed in lockstep as one GPU
 * batch (channel index = stream * cfg->channels + ch).  Each stream obeys the
 * reference's 256-channel limit (constants.go:9). */
gar_status gar_new_batch(gar_config *cfg, int32_t n_streams, gar_resampler **out);
/* resampler.NewEngine (convenience.go:125) when dtype == GAR_F64,
 * resampler.NewEngineFloat32 (convenience.go:329) when dtype == GAR_F32. */
gar_status gar_new_engine(double input_rate, double output_rate, int32_t preset, int32_t dtype,
                          gar_resampler **out);
void gar_free(gar_resampler *r);
/* engine.NewResampler[F](in, out, quality) (internal/engine/resampler.go:51-179)
 * with an engine.Quality (GAR_ENGINE_*) -- the engine seam cmd/resample-wav
 * drives directly (cmd/resample-wav/helpers.go:77-97) and the reference's
 * engine tests use.  dtype GAR_F64 = Resampler[float64]; GAR_F32 /
 * GAR_F32_EXACT = Resampler[float32] (float32 I/O). */
gar_status gar_new_engine_quality(double input_rate, double output_rate, int32_t engine_quality, int32_t dtype,
                                  gar_resampler **out);
/* Host-only NewEngine (no GPU work; process calls report exact lengths only).
 * Used to test the stream-length state machine on machines without a GPU. */
gar_status gar_new_engine_dry(double input_rate, double output_rate, int32_t preset, int32_t dtype,
                              gar_resampler **out);

/* ---- host-memory streaming (cgo path; channel 0 unless noted) ------------- */
/* EstimateOutput (constant.go:117-119, convenience.go:168-170). */
int64_t gar_estimate_output(const gar_resampler *r, int64_t input_len);
/* Exact number of samples the next process call on `channel` would return. */
int64_t gar_output_size(const gar_resampler *r, int32_t channel, int64_t input_len);
/* Exact number of samples Flush on `channel` would return now. */
int64_t gar_flush_size(const gar_resampler *r, int32_t channel);

/* Process / ProcessFloat32 (constant.go:88-146, convenience.go:138,341): fills
 * out[0:*n_out]; GAR_ERR_BUFFER_TOO_SMALL (no state change) if cap < the exact
 * output size. */
gar_status gar_process_f64(gar_resampler *r, const double *in, int64_t n, double *out, int64_t cap, int64_t *n_out);
gar_status gar_process_f32(gar_resampler *r, const float *in, int64_t n, float *out, int64_t cap, int64_t *n_out);
/* ProcessInto / ProcessFloat32Into (constant.go:103-112, :161-199,
 * convenience.go:145-160, :351-366): GAR_ERR_BUFFER_TOO_SMALL before any state
 * change when cap < EstimateOutput(n). */
gar_status gar_process_into_f64(gar_resampler *r, const double *in, int64_t n, double *out, int64_t cap,
                                int64_t *n_out);
gar_status gar_process_into_f32(gar_resampler *r, const float *in, int64_t n, float *out, int64_t cap,
                                int64_t *n_out);
/* ProcessMulti (constant.go:204-252): in[c][0:n] planar; out[c] with capacity
 * cap each; n_out[c] per channel. */
gar_status gar_process_multi_f64(gar_resampler *r, const double *const *in, int32_t n_channels, int64_t n,
                                 double *const *out, int64_t cap, int64_t *n_out);
/* Flush (constant.go:349-354, resampler.go:275-322): channel 0. */
gar_status gar_flush_f64(gar_resampler *r, double *out, int64_t cap, int64_t *n_out);
gar_status gar_flush_f32(gar_resampler *r, float *out, int64_t cap, int64_t *n_out);
/* FlushMulti (constant.go:390-404). */
gar_status gar_flush_multi_f64(gar_resampler *r, double *const *out, int32_t n_channels, int64_t cap,
                               int64_t *n_out);

/* ---- device-resident batched streaming (all channels in lockstep) -------- */
/* Process `frames` frames of all `channels` channels (must equal the handle's
 * channel count: GAR_ERR_CHANNEL_MISMATCH otherwise, like ProcessMulti,
 * constant.go:205-207) from device memory `in` (dtype in_dtype) into device
 * memory `out`; *out_frames = frames produced per channel.
 * GAR_ERR_BUFFER_TOO_SMALL (no state change) if out_cap_frames is smaller than
 * the exact output size.  Asynchronous on `stream` (NULL = the default
 * stream); returns once the work is enqueued.  Calls on one handle are
 * ordered even across streams (each waits for the handle's previous call);
 * the caller keeps `in` alive and `out` untouched until `stream` has run the
 * call.  Cost of that ordering: while a handle is used on ONE stream its calls
 * record no event (an event costs ~3.5 us of stream time per call), so the
 * first call on a different stream, gar_synchronize, gar_reset and gar_free
 * wait with hipDeviceSynchronize -- every stream of the device, including
 * other handles' work; do not call them while another thread captures a
 * stream.  After the first switch every call records an event and these wait
 * for that event only.  A device error leaves the handle refusing work (GAR_ERR_DEVICE)
 * until gar_reset.  The handle's device is made current for the call and the
 * caller's current device restored. */
gar_status gar_process_device(gar_resampler *r, const void *in, int32_t in_dtype, int64_t in_frame_stride,
                              int64_t in_channel_stride, int64_t frames, int32_t channels, void *out,
                              int32_t out_dtype, int64_t out_frame_stride, int64_t out_channel_stride,
                              int64_t out_cap_frames, int64_t *out_frames, void *stream);
/* Flush all channels into device memory (FlushMulti semantics); `channels` as above. */
gar_status gar_flush_device(gar_resampler *r, int32_t channels, void *out, int32_t out_dtype,
                            int64_t out_frame_stride, int64_t out_channel_stride, int64_t out_cap_frames,
                            int64_t *out_frames, void *stream);
/* Exact lockstep output sizes (-1 if channels are not in lockstep). */
int64_t gar_device_output_size(const gar_resampler *r, int64_t frames);
int64_t gar_device_flush_size(const gar_resampler *r);
/* Waits until every call enqueued on the handle has run and reports how it ended: GAR_OK, or
 * GAR_ERR_DEVICE when a kernel of one of them reported a broken invariant into the handle's
 * device status word (e.g. an expired progress wait of the streaming kernel: its outputs are
 * invalid) or a HIP error occurred; the handle then refuses work until gar_reset.  Every ABI call
 * also checks the status word on entry, and the host-memory calls (which synchronise) after their
 * own kernels.  No Go counterpart: the reference's calls are synchronous (constant.go:88-146); this
 * is the synchronisation point of the asynchronous *_device entry points. */
gar_status gar_synchronize(gar_resampler *r);

/* ---- dithered integer PCM output ------------------------------------------ */
/* By default every integer PCM output (GAR_PCM16 / 24 / 32 / GAR_PCM24_PACKED) is the reference CLI's
 * int(clamp(y, -1, 1) * maxVal): truncation toward zero.  GAR_DITHER_TPDF replaces it, for the integer
 * PCM out_dtypes of gar_process_device / gar_flush_device, by round-to-nearest with a +-1 LSB
 * triangular (TPDF) dither, computed inside the kernels that store the samples.  All integer
 * arithmetic is uint32, wrapping:
 *   h32(x):   x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16
 *   key(c)  = h32(lo32(seed) ^ h32(hi32(seed) ^ h32(c + 1)))    c: channel index of the handle
 *                                                               (batch: stream * channels + ch)
 *   r(c, n) = h32(h32(key(c) + hi32(n)) ^ lo32(n))              n: uint64 position in the output stream
 *   d(c, n) = ((r & 0xffff) - (r >> 16)) / 65536                in (-1, 1), exact in float32 / float64
 *   s = clamp(y, -1, 1) * maxVal   (float64, as without dither);   t = 0.5 + d(c, n)   (exact)
 *   q = floor(s + t)  (one float64 addition, then floor);  q = clamp(q, -maxVal, +maxVal);  NaN -> 0
 * and q is stored as without dither (int16 / int32 / 3 bytes).
 * Position: the first output frame of a device call has n = the lockstep group's GetStatistics
 * samplesOut at entry to the call, frame k of the call n + k.  So:
 *   - the noise of a sample depends only on (seed, channel, its index in the output stream): not on
 *     the chunking, the fused or staged conversion path, the layout, or the kernel or launch that
 *     wrote it;
 *   - gar_reset zeroes the counter, so the noise restarts;
 *   - gar_state_save / gar_state_load carry the counter (GetStatistics), so a resumed stream continues
 *     bit-identically with dither on; the blob format and version are unchanged;
 *   - outputs returned by host-memory calls advance the position like any others;
 *   - known quirk: the engine-path QualityQuick Flush is uncounted (resampler.go:276-279), so positions
 *     repeat if such a stream is processed again after a flush.
 * The setting is configuration, not stream state (like the design): it applies to the device calls
 * enqueued after gar_set_dither (the parameters travel by value in kernel arguments: no
 * synchronisation), survives gar_reset and gar_state_load, is not in the state blob, and works on
 * dry-run handles.  GAR_F16 / GAR_BF16 / float outputs and the host-memory entry points ignore it.
 * gar_set_dither: NULL handle or unknown mode -> GAR_ERR_INVALID_ARGUMENT, nothing changed.
 * gar_get_dither: each output may be NULL; *position = where the next device call would start, -1
 * when the channels are not in lockstep. */
enum { GAR_DITHER_NONE = 0, GAR_DITHER_TPDF = 1 };
gar_status gar_set_dither(gar_resampler *r, int32_t mode, uint64_t seed);
gar_status gar_get_dither(const gar_resampler *r, int32_t *mode, uint64_t *seed, int64_t *position);

/* ---- clip counter and peak meter of the integer PCM output ----------------- */
/* Every integer PCM store clamps to [-1, 1] first, and a resampled signal overshoots its input (a
 * full-scale square through 44.1k -> 48k goes past 1.0).  The meter is opt-in and per handle.  While it
 * is on, every integer PCM sample stored by gar_process_device / gar_flush_device (out_dtype
 * GAR_PCM16 / 24 / 32 / GAR_PCM24_PACKED) updates two values per channel, kept in device memory and
 * computed inside the kernels that store the sample, where the unclamped value still exists (after
 * libsoxr's soxr_num_clips).  Let y be the sample in the compute type, widened exactly to float64:
 *   - clips: uint64 count of stored samples that a clamp changed.  A sample is clipped when y > 1.0 or
 *     y < -1.0; +-Inf count; NaN does not count (it stores 0 as ever).  With GAR_DITHER_TPDF on, a
 *     sample is also clipped when q = floor(s + t) of the dither text above, taken before its clamp to
 *     +-maxVal, lies outside [-maxVal, maxVal] (a sample at exactly +-1.0 whose noise pushes it over).
 *   - peak: the maximum of |y| over the metered samples, a double.  It starts at 0, NaN is ignored,
 *     +Inf is a legal value.
 * Each stored sample is tallied exactly once, with the value that ends up in memory (an output the
 * exact fallback recomputes is tallied with the recomputed value only), and turning the meter on does
 * not change a stored byte.  Float and half outputs do not clamp and are not metered; host-memory calls
 * are not metered.  Channels are the handle's channels (batch: stream * channels + ch, as for the
 * dither keys).  The tallies accumulate across calls until read with reset or until gar_reset.
 * The on / off setting is configuration, like dither: it applies to the device calls enqueued after
 * gar_set_meter, survives gar_reset and gar_state_load and is not in the state blob (format and version
 * unchanged).  gar_reset zeroes the tallies; gar_state_load leaves them alone (they describe what this
 * handle stored, not the stream).  Dry-run handles accept both calls and read zeros.
 * gar_set_meter: on = 0 / 1; anything else, or a NULL handle: GAR_ERR_INVALID_ARGUMENT, nothing changed.
 *   The first gar_set_meter(r, 1) allocates the handle's tallies ([channels] x 16 bytes, zeroed).
 * gar_get_meter: *on = the setting.
 * gar_meter_read: waits for the handle's enqueued calls (gar_synchronize's wait; a raised device status
 *   word gives GAR_ERR_DEVICE), then clips[i], peak[i] = the tallies of channel ch0 + i, i < n_ch; either
 *   pointer may be NULL.  reset != 0 zeroes exactly those channels, ordered before any later call on the
 *   handle.  A channel range outside the handle: GAR_ERR_INVALID_ARGUMENT, nothing read or reset.  A
 *   handle whose meter was never on reads zeros.
 * Waiting: the zeroing (gar_meter_read with reset, and gar_reset on a handle whose meter has ever been on,
 *   also after it was turned off again: the tallies stay allocated) waits for the handle's enqueued calls
 *   as gar_synchronize does -- for a handle used on one stream only that is a wait for the device, see
 *   gar_process_device -- and then for a memset on the handle's own stream.  So gar_reset is no longer
 *   free of synchronisation on such a handle; do not call either during a stream capture.
 * A metered integer PCM store is served by the streaming FIR kernels or by the staged conversion kernels.
 *   Should a launch plan route a fused PCM store to any other kernel (development knobs only; the engine
 *   fuses PCM only where the streaming planner never declines), the call fails with a device error
 *   rather than store without tallying -- as a dithered store does. */
gar_status gar_set_meter(gar_resampler *r, int32_t on);
gar_status gar_get_meter(const gar_resampler *r, int32_t *on);
gar_status gar_meter_read(gar_resampler *r, int32_t ch0, int32_t n_ch, uint64_t *clips, double *peak,
                          int32_t reset);

/* ---- state snapshots (checkpoint / resume / migrate) ---------------------- */
/* The streaming state of a handle -- every channel group with its channel range, the per-stage
 * counters (history lengths, polyphase position, decimator phase, cubic phase, fused / stage-by-stage
 * mode), the history rows themselves and the GetStatistics counters -- as one self-contained blob in
 * HOST memory.  No Go counterpart: the reference's state lives in the caller's process; an engine
 * behind a C ABI has to hand it out itself.  The design (filter banks, launch plans) is not in the
 * blob: a blob is loaded into a handle constructed with the same arguments, whose own design is used.
 * A blob is little-endian and versioned (layout: DESIGN.md "State snapshots"); it serves checkpoints
 * and migration between builds of the same version, and another version is refused.  One state has
 * exactly one blob: save -> load -> save gives identical bytes.
 *
 * gar_state_size: bytes gar_state_save would write now (host bookkeeping only, no wait); -1 for NULL.
 *
 * gar_state_save: waits for every call enqueued on the handle, on any stream (the wait of
 * gar_synchronize), then writes the snapshot into buf[0:*n_written].  cap smaller than the snapshot:
 * GAR_ERR_BUFFER_TOO_SMALL, *n_written = the size needed, nothing written.  A handle that refuses
 * work after a device error, or whose device status word is raised: GAR_ERR_DEVICE.  Saving does not
 * change the handle: the next call's output is bit-identical with or without it.  n_written may be
 * NULL.  On a real handle the rows are gathered by one kernel launch and fetched by one copy.
 *
 * gar_state_load: replaces the handle's streaming state with the blob's -- groups and channel ranges
 * (a handle split by per-channel host calls comes back split), counters, histories, statistics.
 * Synchronous: it waits for the handle's enqueued calls first, buf may be freed on return, and later
 * calls on any stream are ordered after it.  The blob is treated as untrusted input and checked in
 * full before anything changes; GAR_ERR_INVALID_ARGUMENT (detail in gar_last_error, NO state change)
 * for a wrong magic or version, n different from the recorded length, a checksum mismatch, a
 * fingerprint mismatch, a dry-run blob on a real handle or the reverse, and counters, history
 * lengths, channel ranges or segment offsets that this handle's design could not have produced.
 * The fingerprint holds the input and output rate, the total channel count and the channels per
 * stream, the expanded quality spec (the engine quality for the engine constructors), New path or
 * engine path, the compute type (GAR_F32 and GAR_F32_EXACT differ) and the number of stages; the
 * device ordinal is deliberately absent -- restoring on a handle of another GPU is the migration
 * case.  A handle refusing work after a device error answers GAR_ERR_DEVICE: gar_reset first.
 * Dry-run handles take part; their blobs hold counters and no rows. */
int64_t gar_state_size(const gar_resampler *r);
gar_status gar_state_save(gar_resampler *r, void *buf, int64_t cap, int64_t *n_written);
gar_status gar_state_load(gar_resampler *r, const void *buf, int64_t n);

/* ---- state / introspection ----------------------------------------------- */
void gar_reset(gar_resampler *r);                       /* Reset (constant.go:429-444, resampler.go:325-340) */
double gar_get_ratio(const gar_resampler *r);           /* GetRatio (constant.go:447) */
int32_t gar_get_latency(const gar_resampler *r);        /* GetLatency (constant.go:407-426) */
gar_status gar_get_info(const gar_resampler *r, gar_info *info); /* GetInfo (constant.go:452-485) */
int32_t gar_channels(const gar_resampler *r);
/* GetStatistics (internal/engine/resampler.go:348-353; SimpleResampler{,Float32}.GetStatistics
 * convenience.go:184-187,393-396): samplesIn / samplesOut of channel `ch`'s engine -- input frames of
 * every non-empty Process, output frames of every Process and Flush (the QualityQuick engine's Flush
 * is uncounted, resampler.go:276-279), both zeroed by Reset.  GAR_ERR_INVALID_ARGUMENT for a bad ch. */
gar_status gar_get_statistics(const gar_resampler *r, int32_t ch, int64_t *samples_in, int64_t *samples_out);
const char *gar_status_string(gar_status s);
const char *gar_last_error(void);                       /* thread-local detail for the last failure */
/* HIP-event timing of every MFMA FIR launch (bracketed on its own stream). */
void gar_profile_enable(gar_resampler *r, int32_t on);
/* Restricts the event timing to the launch kinds whose bit is set (kind k = bit k, see
 * gar_profile_read; default all): an event pair costs a few microseconds of stream time, so a
 * timed region brackets only the kernel it measures. */
void gar_profile_kinds(gar_resampler *r, uint32_t kinds);
/* Sum of launch durations (ms) and launch count of one kernel kind (0 fused
 * DFT+polyphase FIR, 1 DFT FIR, 2 decimator FIR, 3 fused FIR launched by a
 * flush, 4 polyphase stage with live cubic coefficients, 5 QualityQuick cubic
 * stage) since its last read. */
gar_status gar_profile_read(gar_resampler *r, int32_t kind, double *ms, int64_t *launches);
/* Spread of the launches the last gar_profile_read of `kind` summed: min, median, max ms per launch
 * (zeros when there were none). */
gar_status gar_profile_launch_stats(gar_resampler *r, int32_t kind, double *min_ms, double *median_ms,
                                    double *max_ms);
/* Execution mode of pipeline stage `stage` of channel 0's group: *fused_plan = 1 when the
 * stage's DFT x2 + polyphase pair has a composite MFMA plan, *fused_now = 1 while the stream
 * still runs on it (0 after a stage-by-stage fallback: Process after Flush, the
 * polyphase_stage.go:300-307 history quirk).  Works on dry-run handles. */
gar_status gar_stage_state(const gar_resampler *r, int32_t stage, int32_t *fused_plan, int32_t *fused_now);

/* Host self-test of the staging pool the host calls convert through (no GPU): `threads` caller
 * threads each run `iters` conversion jobs of channels x frames through the pool at once (one job
 * at a time uses the workers, the others run inline) and check every element.  0 = every element
 * right; else the number of wrong elements.  For tests (CPU suite; tools/asan_tests.sh with TSan). */
int64_t gar_dev_pool_selftest(int32_t threads, int32_t iters, int32_t channels, int64_t frames);

/* The sample conversions of GAR_F16 / GAR_BF16 run on the host (no GPU; the kernels use the same
 * functions): for each in[i], from_f64[i] = the half bit pattern of ONE rounding f64 -> half (what a
 * float64-compute handle stores), from_f32[i] = the pattern of float32(in[i]) rounded to half (what a
 * float32-compute handle stores), widened[i] = from_f64[i] widened back to float32 (the input
 * conversion).  Any output may be NULL.  For tests (CPU suite). */
gar_status gar_dev_half_convert(int32_t half_type, const double *in, int64_t n, uint16_t *from_f64,
                                uint16_t *from_f32, float *widened);

/* The sample conversions of GAR_PCM24_PACKED run on the host (no GPU; the kernels use the same
 * functions): packed[3 i .. 3 i + 2] = the 3 bytes a float64-compute handle stores for in[i],
 * unpacked[i] = those bytes read back as the sign-extended integer (the input conversion before
 * its scaling).  Either output may be NULL.  For tests (CPU suite). */
gar_status gar_dev_pcm24_convert(const double *in, int64_t n, uint8_t *packed, int32_t *unpacked);

/* The dithered quantizer of gar_set_dither run on the host (no GPU; the kernels use the same
 * functions): out[i] = the integer stored for in[i] as the sample of channel `channel` at stream
 * position position0 + i, noise[i] = d(channel, position0 + i).  pcm_type is an integer PCM type
 * (GAR_PCM24_PACKED gives GAR_PCM24's integers), anything else GAR_ERR_INVALID_ARGUMENT.  out and
 * noise may each be NULL.  For tests (CPU suite). */
gar_status gar_dev_dither_quantize(int32_t pcm_type, uint64_t seed, int32_t channel, int64_t position0,
                                   const double *in, int64_t n, int32_t *out, double *noise);

/* The meter's tally of gar_set_meter run on the host (no GPU; the kernels call the same function):
 * *clips, *peak = the tallies of in[0 .. n) stored as the samples of channel `channel` at stream
 * positions position0 + i in pcm_type, with dither_mode GAR_DITHER_NONE or GAR_DITHER_TPDF (seed as
 * gar_set_dither).  Another type or mode: GAR_ERR_INVALID_ARGUMENT.  Either output may be NULL.  For
 * tests (CPU suite). */
gar_status gar_dev_meter_tally(int32_t pcm_type, int32_t dither_mode, uint64_t seed, int32_t channel,
                               int64_t position0, const double *in, int64_t n, uint64_t *clips, double *peak);

/* The launch plan of the streaming FIR kernels for one call, computed on the host (no GPU; the
 * planner of every streaming launch, csrc/gar_hxs_launch.hpp): writes the GAR_HX_TRACE line(s) such a launch
 * prints -- kernel, group size, chunking, ring, load / store layout, raw-load rows, compute waves,
 * loaders -- into buf (NUL-terminated, at most cap bytes), "not supported\n" when the planner
 * declines, nothing for an empty output range.  `r` may be a dry-run handle; `stage` picks the
 * pipeline stage, whose split-f16 plan is taken (fused, else DFT, else decimator;
 * GAR_ERR_INVALID_ARGUMENT if it has none).  Types are the ABI's sample type codes; addresses are
 * used as integers (alignment, base offsets) and never dereferenced.  Source: element (t, c) of the
 * new input at in_addr + ((t - in_base) * in_fs + c * in_cs) elements for t in [in_base, in_base +
 * in_len), zeros from valid_end, in_addr 0 for a flush; history rows of stride hist_ld at hist_addr.
 * Output: element (o, c) at out_addr + ((o - o0) * out_fs + c * out_cs) elements, o in [o_lo, o_hi).
 * hist_keep: rows of a history keep folded into the launch (0: none).  The knobs are read
 * from the environment on every call.  For tests (CPU suite). */
gar_status gar_dev_hxs_plan(const gar_resampler *r, int32_t stage, int32_t in_type, int64_t in_fs, int64_t in_cs,
                            uint64_t in_addr, int64_t in_base, int64_t in_len, int64_t valid_end, uint64_t hist_addr,
                            int64_t hist_len, int64_t hist_ld, int32_t out_type, uint64_t out_addr, int64_t o0,
                            int64_t out_fs, int64_t out_cs, int64_t o_lo, int64_t o_hi, int32_t channels,
                            int32_t cu_count, int64_t hist_keep, char *buf, int64_t cap);

/* The launch of one x == 0 FIR stage call as the engine would make it, planned on the host (no GPU;
 * csrc/gar_hx_launch.hpp firPlanLaunch): the call description of gar_dev_hxs_plan plus `which` plan of
 * the stage -- 0 fused composite, 1 DFT, 2 decimator (GAR_ERR_INVALID_ARGUMENT if the stage has none).
 * `r` may be a dry-run handle of any compute type.  Writes the line(s) the launch prints under
 * GAR_HX_TRACE / GAR_BG_TRACE -- the "hxs:" / "hxt:" / "hxq:" lines of the streaming split-f16 kernels,
 * an "hx:" line (the block kernel) or a "bg:" line (GAR_F64 / GAR_F32_EXACT compute), every field of the
 * plan -- or "not supported\n" (PCM output on the block kernel), "invalid configuration\n", nothing
 * when there is nothing to launch.  The knobs are read from the environment on every call.  For tests
 * (CPU suite). */
gar_status gar_dev_fir_plan(const gar_resampler *r, int32_t stage, int32_t which, int32_t in_type, int64_t in_fs,
                            int64_t in_cs, uint64_t in_addr, int64_t in_base, int64_t in_len, int64_t valid_end,
                            uint64_t hist_addr, int64_t hist_len, int64_t hist_ld, int32_t out_type, uint64_t out_addr,
                            int64_t o0, int64_t out_fs, int64_t out_cs, int64_t o_lo, int64_t o_hi, int32_t channels,
                            int32_t cu_count, int64_t hist_keep, char *buf, int64_t cap);

/* ---- host-only design introspection (no GPU needed) ----------------------- */
typedef struct gar_engine_geometry {
    int32_t kind; /* 0 cubic, 1 DFT-only, 2 DFT x2 + polyphase, 3 decimator, 4 pass-through */
    int32_t dft_factor, dft_taps;
    int32_t poly_phases, poly_taps;
    int64_t poly_step;
    int32_t decim_factor, decim_taps;
    int32_t fused;                 /* DFT+polyphase composed into one MFMA FIR (step has no fraction) */
    int32_t fir_period_out, fir_period_in, fir_taps_max;
    double useful_macs_per_output; /* of the MFMA FIR executed for this engine */
    double mfma_macs_per_output;
} gar_engine_geometry;
/* engine.NewResampler[float64](in, out, quality) design (resampler.go:51-179).
 * Any output buffer may be NULL: dft [factor*taps], poly_* [phases*taps] (the
 * Go layout), decim [taps]. */
gar_status gar_design_engine(double input_rate, double output_rate, int32_t engine_quality,
                             gar_engine_geometry *geom, double *dft, double *poly_a, double *poly_b,
                             double *poly_c, double *poly_d, double *decim);
/* Composite FIR of a fused DFT+polyphase engine: rows [P][taps_max] (zero padded), offsets [P]. */
gar_status gar_design_composite(double input_rate, double output_rate, int32_t engine_quality, double *rows,
                                int64_t *offsets);

/* Pipeline stages of a handle (pipeline.BuildPipeline, internal/pipeline/pipeline.go:104-183; 0 when the
 * ratio is within 0.1 % of 1) and the design geometry + engine ratio of stage `stage`
 * (engine.NewResampler[float64](48000, 48000*ratio, q), stages.go:54-70). */
int32_t gar_num_stages(const gar_resampler *r);
gar_status gar_stage_geometry(const gar_resampler *r, int32_t stage, double *stage_ratio, gar_engine_geometry *geom);

#ifdef __cplusplus
}
#endif
#endif /* GAR_H */
