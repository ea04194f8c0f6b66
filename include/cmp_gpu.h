/*
 * cmp_gpu.h -- device-pointer batch API of the MI355X build (libairscmp.so).
 *
 * No reference counterpart: the reference (lib/cmp.h) compresses one frame
 * from host memory per call.  This API runs the same frame format and the
 * same cmp_context state machine (lib/compress/cmp.c:213-393) over many
 * frames whose samples already live in GPU memory, with one launch per group
 * of frames that share pass parameters.  Frames produced here are
 * byte-identical to what cmp_compress_u16/i16/i16_in_i32 produce for the
 * same inputs, contexts and identifiers.
 *
 * Contexts come from cmp_initialise() exactly as for the host API; when a
 * context needs a work buffer (MODEL preprocessing) its work_buf must be a
 * DEVICE pointer (2-byte aligned; 16 is fastest) holding that context's model.
 *
 * Ordering / identifiers: a call is equivalent to
 *
 *     for c in [0, num_ctx): for a in [0, frames_per_ctx):
 *         sizes[c*fpc + a] = cmp_compress_<type>(&ctx[c], dst(c*fpc+a), dst_capacity,
 *                                                src(c*fpc+a), src_size)
 *
 * including the timestamp-callback sequence that feeds header identifiers.
 */
#ifndef CMP_GPU_H
#define CMP_GPU_H

#include <stdint.h>

#include "cmp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sample layout of the frames in a batch (the three cmp_compress_* entry points) */
enum cmp_gpu_sample_type {
	CMP_GPU_U16 = 0,       /* cmp_compress_u16 */
	CMP_GPU_I16 = 1,       /* cmp_compress_i16 */
	CMP_GPU_I16_IN_I32 = 2 /* cmp_compress_i16_in_i32 */
};

/* flags */
#define CMP_GPU_AUTO_RICE 0x1u /* GOLOMB_ZERO passes after NONE, DIFF or IWT preprocessing:
				* choose g = 2^k per frame (k in [0,15], fewest payload bits
				* for the pass's residuals -- the IWT coefficients for IWT --,
				* ties to smaller k) instead of the configured encoder
				* parameter; MODEL passes keep theirs; build-defined extension */
#define CMP_GPU_HOST_STEPPED 0x2u /* batches that can fall back or fail: step the context state
				   * machine on the host (one synchronisation per acquisition step)
				   * instead of on the device; same output, for comparisons */
#define CMP_GPU_STEPWISE 0x4u     /* MODEL contexts: one launch per acquisition step instead of
				   * every acquisition in one launch with the models kept on
				   * the chip; same output, for comparisons */
#define CMP_GPU_REPORT_DRAWS 0x8u /* write each frame's identifier-draw count to batch->draws
				   * (which must then be non-NULL); without it draws is never
				   * touched */

struct cmp_gpu_batch {
	enum cmp_gpu_sample_type type;
	const void *src;        /* device; frame i at src + i*src_stride (16-byte aligned frames load fastest) */
	uint64_t src_stride;    /* bytes, multiple of the sample size */
	uint32_t src_size;      /* bytes per frame, as cmp_compress_*'s src_size */
	void *dst;              /* device; frame i at dst + i*dst_stride, 8-byte aligned */
	uint64_t dst_stride;    /* bytes, multiple of 8 */
	uint32_t dst_capacity;  /* bytes available per frame */
	uint32_t *sizes;        /* device [num frames]: frame size or error value */
	uint32_t flags;
	uint8_t *draws;         /* with CMP_GPU_REPORT_DRAWS, HOST [num frames]: timestamp-callback draws each frame made
				 * (0: it carries its context's identifier; 1: a reset; 3 or 2: a
				 * primary or secondary pass that fell back, cmp.c:342-393), for
				 * assigning identifiers across processes (shard.py); valid when the
				 * call returns.  Zero-initialise the struct: fields added later
				 * default to off */
};

struct cmp_gpu_engine;

/* Create an engine bound to the current HIP device and the given hipStream_t
 * (NULL = default stream).  Returns an error value or CMP_ERR_NO_ERROR. */
uint32_t cmp_gpu_engine_create(struct cmp_gpu_engine **engine, void *hip_stream);
void cmp_gpu_engine_destroy(struct cmp_gpu_engine *engine);

/* Engine options, all 0 after cmp_gpu_engine_create.  Returns 0 or an error
 * value (CMP_ERROR(PARAMS_INVALID) for an unknown option or value).
 *   CMP_GPU_OPT_EXCLUSIVE       1: the caller promises that nothing else runs
 *                               on the device while this engine's kernels do
 *                               (one process, one stream).  The MODEL segment
 *                               walk may then order its workgroups by block
 *                               index when its whole grid fits the CUs; without
 *                               it every workgroup numbers itself with a
 *                               ticket as it starts, which stays correct beside
 *                               other kernels and processes.  CMP_GPU_AUTO_RICE
 *                               picks k inside the encode kernel for frames of
 *                               up to 32 segments (16-bit: 512 Ki samples) with
 *                               the option, up to 8 without it (a frame's
 *                               segments meet at a barrier); larger frames take
 *                               the selection kernel first.
 *   CMP_GPU_OPT_WALK_SEGMENT    MODEL segment walk: 0 automatic, or 2048 /
 *                               4096 samples per segment.
 *   CMP_GPU_OPT_NO_CONTEXT_WALK 1: MODEL batches take the segment walk where
 *                               they would take the context walk (not those
 *                               with the uncompressed fallback, which need it).
 *   CMP_GPU_OPT_IMAGE_CHUNK     (4, defined with cmp_gpu_decompress_image) bytes
 *                               of engine scratch a chunk of that call, or a run
 *                               of cmp_gpu_compress_image, may stage; 0: the
 *                               default, 256 MiB.
 *   CMP_GPU_OPT_IMAGE_RAGGED    (5, defined with cmp_gpu_compress_image) frames
 *                               of unequal sizes share one encode launch there;
 *                               0: off (the default).
 *   CMP_GPU_OPT_IMAGE_RAGGED_CHECKSUM (6, defined with cmp_gpu_compress_image)
 *                               1: checksum-enabled contexts take those launches
 *                               too; 0: they do not (the default); any other
 *                               value: CMP_ERR_PARAMS_INVALID. */
#define CMP_GPU_OPT_EXCLUSIVE 1u
#define CMP_GPU_OPT_WALK_SEGMENT 2u
#define CMP_GPU_OPT_NO_CONTEXT_WALK 3u
uint32_t cmp_gpu_engine_set_option(struct cmp_gpu_engine *engine, uint32_t option, uint32_t value);

/* Compress num_ctx * frames_per_ctx frames (see the ordering note above).
 * Returns CMP_ERR_NO_ERROR or a call-level error (batch validation: NULL or
 * misaligned pointers, bad sizes, invalid contexts).  Per-frame results,
 * including frames cmp_compress_* would reject, land in batch->sizes.
 *
 * The call is asynchronous on the engine's stream when the outcome of a
 * frame cannot change the pass of the frames after it: dst_capacity is at
 * least the worst-case frame (26 bytes + 6 per sample), no context can fall
 * back to raw storage, and -- where that worst case exceeds the 24-bit
 * compressed-size field (more than ~2.8 Mi samples, so a frame can fail with
 * CMP_ERR_HDR_CMP_SIZE_TOO_LARGE) -- no context has secondary passes with
 * frames_per_ctx > 1, and no context's coder can take a frame of this length
 * past the field at its longest codeword (16 bits UNCOMPRESSED, k + 17 bits
 * GOLOMB_ZERO with k = floor(log2 g), 48 bits otherwise), since a context
 * whose last frame fails keeps its sequence number.  Otherwise the outcome
 * of frame (c, a) decides the pass of frame (c, a+1) or the state the context
 * is left in, so the call runs one acquisition step at a time and
 * synchronises after each step (and after the step's fallbacks,
 * cmp.c:342-393).  Identifier draws are counted per frame and made at the
 * end, in the loop's order.
 *
 * Frames must not overlap: with more than one frame, src_stride >= src_size
 * and dst_stride >= min(dst_capacity, worst-case frame), else the call
 * returns CMP_ERR_GENERIC. */
uint32_t cmp_gpu_compress(struct cmp_gpu_engine *engine, struct cmp_context *ctx, uint32_t num_ctx,
			  uint32_t frames_per_ctx, const struct cmp_gpu_batch *batch);

/* Decoder (no reference counterpart: the reference has none, see
 * programs/airspacecli.c:421-423).  Decodes num_frames frames as written by
 * cmp_compress_* / cmp_gpu_compress back into their 16-bit samples (the low
 * halves, for i16-in-i32 sources).  Frames of every preprocessing mode and
 * encoder; MODEL frames need the model each was encoded against (MODEL frames
 * without one get CMP_ERR_PARAMS_INVALID).  The checksum is not verified
 * (cmp_gpu_decompress_sequences below rebuilds the models and verifies). */
struct cmp_gpu_decode_batch {
	const void *src;        /* device; frame i at src + i*src_stride, 8-byte aligned */
	uint64_t src_stride;    /* bytes, multiple of 8, >= src_capacity */
	uint32_t src_capacity;  /* bytes readable per frame, multiple of 4, >= 22 */
	uint32_t num_frames;    /* <= 65535 */
	uint16_t *dst;          /* device; frame i's samples at dst + i*dst_stride bytes */
	uint64_t dst_stride;    /* bytes, even */
	uint32_t dst_samples;   /* samples available per frame */
	uint32_t *status;       /* device [num_frames]: samples decoded, or an error value */
	const uint16_t *model;  /* device or NULL; frame i's model at model + i*model_stride bytes */
	uint64_t model_stride;  /* bytes, even */
};

/* Returns CMP_ERR_NO_ERROR or a call-level error; per-frame results land in
 * batch->status.  Synchronises with the host (the parse is sized from the
 * headers and repeated until it settles). */
uint32_t cmp_gpu_decompress(struct cmp_gpu_engine *engine, const struct cmp_gpu_decode_batch *batch);

/*
 * Whole sequences: num_ctx contexts of frames_per_ctx frames each, in the
 * order cmp_gpu_compress writes them, decoded in one call.  The model a MODEL
 * frame was encoded against is a function of the samples before it, so it is
 * rebuilt here as the reference's encoder builds it (cmp.c:120-142, 304-311),
 * per context and on the device: every frame is parsed in one batch, then one
 * kernel walks each context's frames with the model in registers.
 *
 * Per context the frames decode in order, each by what its header says:
 *   - a frame that is not MODEL (NONE, DIFF, IWT; a raw fallback frame in
 *     mid-sequence, cmp.c:380-392, is one) decodes on its own; the context's
 *     model then is its samples;
 *   - a MODEL frame: x = r + model (int16 wrap), then model[i] =
 *     (model[i]*rate + x[i]*(16-rate)) >> 4 in int32, truncated to 16 bits,
 *     rate from the frame's header (above 16: CMP_ERR_INT_HDR), x and model
 *     zero-extended for CMP_GPU_U16 and sign-extended otherwise;
 *   - a MODEL frame whose context holds no model gets CMP_ERR_PARAMS_INVALID,
 *     one whose context holds a model of another size
 *     CMP_ERR_SRC_SIZE_MISMATCH;
 *   - a frame that fails for any reason keeps its error value, and its
 *     context holds no model until its next frame that is not MODEL decodes;
 *     other contexts are unaffected.
 *
 * checksum_ok (optional) asks for verification: for every frame that decoded
 * and whose header has the checksum bit, the XXH32 of the decoded samples as
 * big-endian 16-bit words (header.c:137-163) is compared with the frame's
 * last four bytes.  A mismatch is reported there only; status is not changed.
 *
 * Returns CMP_ERR_NO_ERROR or a call-level error (CMP_ERR_GENERIC: NULL or
 * misaligned pointers, bad strides, more than 65535 frames, model without
 * model_n, CMP_GPU_SEQ_MODEL_IN without model, unknown flags), before anything
 * reaches the device.  Synchronises with the host exactly where
 * cmp_gpu_decompress does (the parse rounds), never per frame or acquisition.
 * Build-defined extension.
 */
#define CMP_GPU_SEQ_MODEL_IN 0x1u /* contexts start from the models in batch->model */

struct cmp_gpu_decode_seq_batch {
	enum cmp_gpu_sample_type type; /* U16: zero-extending model update; I16 / I16_IN_I32: sign-extending
					* (cmp.c:132-142); the output is 16-bit samples in every case */
	const void *src;        /* as cmp_gpu_decode_batch */
	uint64_t src_stride;
	uint32_t src_capacity;
	uint32_t num_ctx, frames_per_ctx; /* frame (c, a) is frame c*frames_per_ctx + a;
					   * num_ctx*frames_per_ctx <= 65535 */
	uint16_t *dst;          /* device; frame i's samples at dst + i*dst_stride bytes */
	uint64_t dst_stride;    /* bytes, even, >= 2*dst_samples (16-byte rows are fastest) */
	uint32_t dst_samples;   /* samples available per frame */
	uint32_t *status;       /* device [frames]: samples decoded, or an error value */
	uint16_t *model;        /* device or NULL: context c's model at model + c*model_stride bytes,
				 * dst_samples samples each; read with CMP_GPU_SEQ_MODEL_IN, always
				 * written with the model each context holds after its last frame */
	uint64_t model_stride;  /* bytes, even, >= 2*dst_samples */
	uint32_t *model_n;      /* device [num_ctx], required with model: samples of model held
				 * (0: none); in with CMP_GPU_SEQ_MODEL_IN, always out */
	uint8_t *checksum_ok;   /* device [frames] or NULL; non-NULL asks for verification:
				 * 0 no checksum in the frame (or the frame failed), 1 match, 2 mismatch */
	uint32_t flags;
};

uint32_t cmp_gpu_decompress_sequences(struct cmp_gpu_engine *engine, const struct cmp_gpu_decode_seq_batch *batch);

/*
 * File images: frames as they are stored -- back to back at byte granularity
 * (the sample files' .air form, any concatenation of frame files), or at the
 * 8-byte aligned offsets of cmp_gpu_pack_frames / cmp_gpu_gather -- decoded in
 * one call from ONE device buffer and a table of byte offsets, into samples
 * packed back to back, optionally big-endian as the sample files hold them.
 *
 * The frames form one context, in table order: frame f decodes exactly as
 * frame (0, f) of a one-context cmp_gpu_decompress_sequences call over the
 * same frames, with the same statuses, checksum_ok, final model and model_n
 * (MODEL and other frames mix; a frame that fails leaves the context without
 * a model).  A frame's slice is unusable when offsets[f] + 16 > src_size, its
 * compressed size (header bytes 2..4) is below 16, offsets[f] + compressed
 * size > src_size, or its original size (bytes 5..7) is odd: that frame gets
 * CMP_ERR_INT_HDR.
 *
 * dst_offsets[0] = 0 and dst_offsets[f + 1] = dst_offsets[f] + the frame's
 * header original size (0 for an unusable slice; the header's value for every
 * other frame, whether or not it decodes), so the layout follows from the
 * headers alone.  Frame f's samples are 16-bit (the low halves, as elsewhere),
 * native-endian, or byte-swapped with CMP_GPU_IMG_BIG_ENDIAN; after an error
 * the frame's own bytes are unspecified.  Nothing is written outside
 * [dst, dst + dst_offsets[num_frames]) or outside a frame's own range.
 *
 * Returns CMP_ERR_NO_ERROR or a call-level refusal, raised before any sample
 * is written: NULL engine, batch, offsets, dst_offsets or status, or
 * num_frames 0: CMP_ERR_GENERIC; NULL src CMP_ERR_SRC_NULL; src_size 0
 * CMP_ERR_SRC_SIZE_WRONG; NULL dst CMP_ERR_DST_NULL; odd dst
 * CMP_ERR_DST_UNALIGNED; an unknown type or flag, model without model_n (or
 * an odd model, model_samples 0, a status or model_n that is not 4-byte
 * aligned), MODEL_IN without model:
 * CMP_ERR_GENERIC; then, known after the header read-back,
 * dst_offsets[num_frames] > dst_capacity: CMP_ERR_DST_TOO_SMALL, and a frame
 * with more samples than model_samples while model is given: CMP_ERR_GENERIC.
 *
 * No byte outside the 16-byte aligned hull of [src, src + src_size) is read,
 * and no result depends on a byte outside the frames' own slices.  The call
 * synchronises once for the header read-back and then wherever the sequence
 * decoder does; the device outputs are valid after cmp_gpu_synchronize.  The
 * table is cut into chunks of at most 65535 frames whose staging rows fit
 * CMP_GPU_OPT_IMAGE_CHUNK bytes of engine scratch (0: 256 MiB; a chunk always
 * holds one frame at least); the model passes from chunk to chunk on the
 * device and the result does not depend on the value.  With MODEL_IN, a
 * model_n above the samples of the largest frame in the first chunk is not a
 * model of these frames and counts as none.  Build-defined extension.
 */
#define CMP_GPU_IMG_MODEL_IN   0x1u /* the context starts from batch->model / model_n */
#define CMP_GPU_IMG_BIG_ENDIAN 0x2u /* samples are written big-endian (the sample file format) */
#define CMP_GPU_OPT_IMAGE_CHUNK 4u  /* cmp_gpu_engine_set_option: bytes of staging per chunk */

struct cmp_gpu_decode_image {
	enum cmp_gpu_sample_type type; /* model update extension, as cmp_gpu_decode_seq_batch */
	const void *src;          /* device, ANY alignment */
	uint64_t src_size;        /* bytes of the image */
	const uint64_t *offsets;  /* HOST [num_frames]: byte offset of each frame in src, any alignment,
				   * any order, gaps allowed; read during the call only */
	uint32_t num_frames;      /* >= 1; no 65535 limit (the call chunks) */
	void *dst;                /* device, 2-byte aligned; frame f's samples at dst + dst_offsets[f] */
	uint64_t dst_capacity;    /* bytes */
	uint64_t *dst_offsets;    /* HOST [num_frames + 1], out: valid when the call returns */
	uint32_t *status;         /* device [num_frames]: samples decoded, or an error value */
	uint8_t *checksum_ok;     /* device [num_frames] or NULL, as cmp_gpu_decode_seq_batch */
	uint16_t *model;          /* device or NULL: the ONE context's model, model_samples samples */
	uint32_t model_samples;   /* capacity of model */
	uint32_t *model_n;        /* device, required with model: in with MODEL_IN, always out */
	uint32_t flags;
};
uint32_t cmp_gpu_decompress_image(struct cmp_gpu_engine *engine, const struct cmp_gpu_decode_image *batch);

/* Host only, no device: walk a HOST image of back-to-back frames from byte 0
 * (compressed size at header bytes 2..4) and write the offsets.  Returns the
 * number of frames found; *bad_at (optional) = the byte where the walk stopped
 * short of `size` (a frame shorter than 16 bytes, one that runs past the end,
 * fewer than 16 bytes left), or UINT64_MAX when the image ends exactly at a
 * frame's end.  offsets may be NULL (count only); at most max_frames are
 * written. */
uint64_t cmp_gpu_frame_table(const void *image, uint64_t size, uint64_t *offsets, uint64_t max_frames,
			     uint64_t *bad_at);

/*
 * Sample images: the mirror of cmp_gpu_decompress_image.  Sample frames as
 * they are stored -- at any byte offset of ONE device buffer, of unequal
 * sizes, optionally big-endian as the sample files hold them -- compressed as
 * one context in one call into a .air image on the device: the frames back to
 * back at byte granularity, with their offset table.
 *
 * Equivalence.  The frames are one context, in table order; the call is
 * equivalent to
 *
 *     for f in [0, num_frames):
 *         sizes[f] = cmp_compress_<type>(ctx, tmp_f, cmp_compress_bound(frame_bytes[f]),
 *                                        native(src + offsets[f]), frame_bytes[f])
 *
 * with all of the loop's effects: the timestamp-callback sequence, the
 * context's final sequence number, identifier and model size, and the work
 * buffer (a DEVICE pointer, as for cmp_gpu_compress).  Per-frame errors land in
 * sizes[f] with the value the loop gives: a size change in a MODEL context
 * CMP_ERR_SRC_SIZE_MISMATCH (cmp.c:246), a frame_bytes of 0 or no multiple of
 * the sample size CMP_ERR_SRC_SIZE_WRONG, a work buffer that is too small
 * CMP_ERR_WORK_BUF_TOO_SMALL, a frame_bytes whose cmp_compress_bound is an
 * error value CMP_ERR_GENERIC (cmp.c:350).  An errored frame takes no bytes.
 *
 * Layout.  out_offsets[0] = 0 and out_offsets[f + 1] = out_offsets[f] + (0 if
 * sizes[f] is an error value, else sizes[f]); frame f's bytes are at
 * out + out_offsets[f], nothing between the frames.  cmp_gpu_frame_table over
 * the first out_offsets[num_frames] bytes (read back) finds exactly the
 * stored frames.
 *
 * Capacity.  A frame whose end would pass out_capacity is not stored and gets
 * CMP_ERR_DST_TOO_SMALL, and so does EVERY frame after it, whatever its own
 * outcome was, so the image is always a prefix of the full result.  The
 * context ends as if all frames had fitted: this is the one place where the
 * call differs from a loop that ran into a small dst.  Nothing is written
 * outside [out, out + out_offsets[num_frames]).
 *
 * Reads.  No byte outside the 16-byte aligned hull of [src, src + src_size)
 * is read.
 *
 * Returns CMP_ERR_NO_ERROR or a call-level refusal, raised before anything
 * reaches the device, checked in this order: NULL engine, ctx, img, offsets,
 * frame_bytes, out_offsets or sizes, or num_frames 0: CMP_ERR_GENERIC; NULL
 * src CMP_ERR_SRC_NULL; src_size 0, or an offsets[f] + frame_bytes[f] above
 * src_size, CMP_ERR_SRC_SIZE_WRONG; NULL out CMP_ERR_DST_NULL; out_offsets not
 * 8-byte or sizes not 4-byte aligned, an unknown type, flag or batch flag,
 * CMP_GPU_REPORT_DRAWS among the batch flags, CMP_GPU_IMG_SRC_BIG_ENDIAN with
 * CMP_GPU_I16_IN_I32: CMP_ERR_GENERIC; then the context as cmp_gpu_compress
 * refuses it: CMP_ERR_CONTEXT_INVALID, or CMP_ERR_WORK_BUF_UNALIGNED for an odd
 * work buffer of a context that keeps state there.
 *
 * The table is cut into runs: maximal stretches of consecutive frames of equal
 * frame_bytes, cut further so that a run's staging rows fit
 * CMP_GPU_OPT_IMAGE_CHUNK bytes of engine scratch (0: 256 MiB; a run always
 * holds one frame at least; the result does not depend on the value).  Every
 * run is one cmp_gpu_compress batch of one context (frames that all differ in
 * size cost one launch each).  A run whose samples are native-endian, whose
 * first frame is aligned to the sample size and whose offsets step by a
 * constant that is at least frame_bytes and a multiple of the sample size is
 * read where it is; every other run is first copied into aligned native rows.
 *
 * CMP_GPU_OPT_IMAGE_RAGGED (engine option; 0, the default: off) changes only
 * how the call schedules this work; no result depends on its value.  It
 * applies when the context keeps no state in its work buffer (no MODEL pass,
 * no IWT), the checksum is disabled, or option 6 is 1, the uncompressed
 * fallback is disabled and batch_flags is 0; any other call takes the runs
 * above whatever the option says.  CMP_GPU_OPT_IMAGE_RAGGED_CHECKSUM (engine
 * option; 0, the default, or 1) is that opt-in of checksum-enabled contexts:
 * their ragged pieces take one XXH32 over all frames of the piece ahead of the
 * encode launches, which append the four bytes.  It changes the schedule only
 * as well.  The table is then cut into pieces.  A run of at least 2 frames whose
 * samples take at least the keep threshold (value 1: the built-in one, 1 MiB;
 * any other value: that many bytes) stays a run as above, and so do frames
 * that are refused.  Every other frame joins a ragged piece: consecutive
 * frames of any sizes, while their staging rows fit CMP_GPU_OPT_IMAGE_CHUNK
 * and their number 2^20, encoded by one launch per pass (two when
 * secondary_iterations is set), with one offset scan and one copy into out for
 * the whole piece.  In a ragged piece a native-endian frame whose address is
 * a multiple of the sample size is read where it is, whatever its neighbours'
 * offsets; the others are copied into aligned native rows first.
 *
 * Synchronisation.  The call is asynchronous on the engine's stream exactly
 * where cmp_gpu_compress with dst_capacity = cmp_compress_bound would be for
 * each run, synchronises where that call does and nowhere else (engine scratch
 * that has to grow waits for the stream, as there); sizes, out_offsets and out
 * are valid after cmp_gpu_synchronize.  Build-defined extension.
 */
#define CMP_GPU_OPT_IMAGE_RAGGED 5u /* cmp_gpu_engine_set_option: 0 off, 1 on, else on with that keep threshold in bytes */
#define CMP_GPU_OPT_IMAGE_RAGGED_CHECKSUM 6u /* cmp_gpu_engine_set_option: 0 off, 1 checksum-enabled contexts take ragged pieces */
#define CMP_GPU_IMG_SRC_BIG_ENDIAN 0x1u /* samples in src are big-endian 16-bit words (sample files) */

struct cmp_gpu_encode_image {
	enum cmp_gpu_sample_type type;
	const void *src;             /* device, ANY alignment */
	uint64_t src_size;           /* bytes of the sample image */
	const uint64_t *offsets;     /* HOST [num_frames]: byte offset of frame f's samples, any alignment,
				      * any order, overlaps allowed; read during the call only */
	const uint32_t *frame_bytes; /* HOST [num_frames]: frame f's src_size as cmp_compress_* takes it */
	uint32_t num_frames;         /* >= 1, no 65535 limit (the call cuts runs) */
	void *out;                   /* device, any alignment: the .air image */
	uint64_t out_capacity;       /* bytes */
	uint64_t *out_offsets;       /* DEVICE [num_frames + 1], 8-byte aligned */
	uint32_t *sizes;             /* DEVICE [num_frames], 4-byte aligned: frame size or error value */
	uint32_t batch_flags;        /* CMP_GPU_AUTO_RICE | HOST_STEPPED | STEPWISE, as cmp_gpu_batch.flags */
	uint32_t flags;              /* CMP_GPU_IMG_SRC_BIG_ENDIAN */
};
uint32_t cmp_gpu_compress_image(struct cmp_gpu_engine *engine, struct cmp_context *ctx,
				const struct cmp_gpu_encode_image *img);

/*
 * Payload-only stream: the num_samples samples at src (device) encoded as ONE
 * bit stream from bit 0 of dst (device, 8-byte aligned), exactly as the
 * reference's encoder loop writes a frame's payload -- NONE or DIFF
 * preprocessing (lib/compress/preprocess.c:268-300), cmp_encoder_encode_s16
 * (lib/compress/encoder.c:327-378), the big-endian bit writer with its
 * zero-padded flush (lib/common/bitstream_writer.h:124-158, 205-227) -- but
 * without header, checksum or the 24-bit frame size limit of a frame, and
 * without a context.  encoder_outlier is used by GOLOMB_MULTI as by
 * cmp_initialise.  Asynchronous: *size (device) receives the stream's byte
 * count, or CMP_ERR_DST_TOO_SMALL when it exceeds dst_capacity (the bytes that
 * fit are written).  num_samples <= 89478485 (bit offsets stay below 2^32 at
 * the worst case of 48 bits per sample).  Build-defined extension: no
 * reference counterpart at the public API.
 */
uint32_t cmp_gpu_encode_stream(struct cmp_gpu_engine *engine, enum cmp_gpu_sample_type type, const void *src,
			       uint32_t num_samples, enum cmp_preprocessing preprocessing,
			       enum cmp_encoder_type encoder_type, uint32_t encoder_param, uint32_t encoder_outlier,
			       void *dst, uint32_t dst_capacity, uint32_t *size);

/*
 * The inverse of cmp_gpu_encode_stream: the src_size bytes at src (device,
 * 8-byte aligned, readable up to src_size rounded up to 4) as *size reported
 * them, decoded into num_samples 16-bit samples at dst (device, 2-byte
 * aligned; 16 is fastest): the low halves for a stream encoded from
 * i16-in-i32, as with the frame decoder, so there is no type argument.
 * preprocessing, encoder_type, encoder_param and encoder_outlier mean exactly
 * what they meant to the encoder and are resolved by the same checks.  A
 * stream has no header, so nothing declares its payload size; the caller does,
 * and the decoder verifies it.  With E the bit position where the
 * num_samples-th codeword ends, a stream is valid only if num_samples valid
 * codewords exist, E <= 8 * src_size, (E + 7) / 8 == src_size, and the bits
 * [E, 8 * src_size) are zero (the bit writer's flush,
 * lib/common/bitstream_writer.h:205-227).  Anything else -- too few codewords,
 * an invalid one, E past the end, bytes left over, pad bits set: a wrong count,
 * a wrong size or wrong parameters -- is CMP_ERR_INT_BITSTREAM.  An
 * UNCOMPRESSED stream therefore needs src_size == 2 * num_samples.
 *
 * *status (device) receives num_samples or that error value; it is valid after
 * cmp_gpu_synchronize.  The result never depends on bytes past src_size, and
 * nothing is written past dst[num_samples - 1] (after an error the samples
 * before it are unspecified).
 *
 * Returns CMP_ERR_NO_ERROR or a call-level refusal, before anything reaches the
 * device, checked in this order: NULL engine or status CMP_ERR_GENERIC; NULL
 * src CMP_ERR_SRC_NULL; src not 8-byte aligned CMP_ERR_GENERIC; NULL dst
 * CMP_ERR_DST_NULL; odd dst CMP_ERR_DST_UNALIGNED; num_samples 0 or above
 * 89478485, or src_size 0 or above CMP_GPU_STREAM_DECODE_MAX,
 * CMP_ERR_SRC_SIZE_WRONG; preprocessing other than NONE / DIFF
 * CMP_ERR_PARAMS_INVALID; encoder arguments the encoder's own checks refuse:
 * the error those checks return.
 *
 * CMP_GPU_STREAM_DECODE_MAX is 2^32 - 4096 bits.  The decoder keeps bit
 * positions in 32 bits: below that size every position, every range end (a
 * multiple of 512 bits at or past the end) and every parse exit (up to 48 bits
 * past the end) stays clear of the 32-bit wrap and of the parse's sentinel
 * 0xFFFFFFFF.  Any stream of at most 89478400 samples fits (48 bits per
 * sample at most); that is 85 samples below the encoder's limit of 89478485,
 * whose worst case is 510 bytes larger.  A stream of 89478401 to 89478485
 * samples decodes as long as its size is within the limit, which all but
 * pathological inputs are.
 *
 * Synchronises with the host for the parse rounds only (the stream is cut into
 * 512-bit subsequences whose count follows from src_size; rounds repeat until
 * the parse settles); the remaining launches stay queued on the engine's
 * stream.  Engine scratch: about 16 bytes per subsequence, a quarter of
 * src_size (128 MiB at the limit).  Build-defined extension.
 */
#define CMP_GPU_STREAM_DECODE_MAX 536870400u /* bytes */
uint32_t cmp_gpu_decode_stream(struct cmp_gpu_engine *engine, const void *src, uint32_t src_size,
			       uint32_t num_samples, enum cmp_preprocessing preprocessing,
			       enum cmp_encoder_type encoder_type, uint32_t encoder_param, uint32_t encoder_outlier,
			       uint16_t *dst, uint32_t *status);

/*
 * Size the frames of a batch under many parameter sets in one call, without
 * coding them: which cmp_params should this data be compressed with?
 *
 * bits[f * num_candidates + c] (device) receives the exact number of payload
 * bits that cmp_compress_<type> writes for frame f in a pass with candidate
 * c's parameters, between the header and the flush: the sum over the frame's
 * samples of the codeword length of cmp_encoder_encode_s16
 * (lib/compress/encoder.c:327-378), the outlier resolved as for a frame
 * (encoder.c:185-224).  CMP_PREPROCESS_NONE sizes the samples, DIFF
 * x[i] - x[i-1] with x[0] as it is, IWT the frame's IWT coefficients, MODEL
 * (int16)(x[i] - model[i]) with the model the caller passes.  The model is read
 * and never updated: an estimate has no context and no sequence, and
 * model_rate does not influence a size.  CMP_ENCODER_UNCOMPRESSED gives
 * 16 * samples under every preprocessing.  For CMP_GPU_I16_IN_I32 only the low
 * halves count, as everywhere else.  The values are integers: they do not
 * depend on how the work is cut up or on run-to-run order.
 *
 * best[f] (device, optional) receives the index c that minimises
 * 8 * H(c) + bits[f][c], ties to the lowest index, with H(c) the header of a
 * frame coded with c: 16 bytes for NONE + UNCOMPRESSED and 22 otherwise.  With
 * the sixteen candidates GOLOMB_ZERO g = 2^k listed in k order this is the
 * CMP_GPU_AUTO_RICE rule.
 *
 * cmp_gpu_estimate_frame_size (host only, no device) turns a bit count into
 * the size of the frame: H(c) + (bits + 7) / 8 + (checksum_enabled ? 4 : 0), or
 * CMP_ERR_HDR_CMP_SIZE_TOO_LARGE when that exceeds CMP_HDR_MAX_COMPRESSED_SIZE;
 * CMP_ERR_GENERIC for a NULL c, and for encoder arguments the encoder's own
 * checks refuse the error those checks return.
 *
 * cmp_gpu_estimate returns CMP_ERR_NO_ERROR or a call-level refusal, before
 * anything reaches the device, checked in this order:
 *    1. NULL engine, batch, candidates or bits: CMP_ERR_GENERIC
 *    2. num_frames 0 or above CMP_GPU_ESTIMATE_MAX_FRAMES: CMP_ERR_GENERIC
 *    3. num_candidates 0 or above CMP_GPU_ESTIMATE_MAX_CANDIDATES: CMP_ERR_GENERIC
 *    4. non-zero flags, an unknown type, bits not 8-byte aligned or best not
 *       4-byte aligned: CMP_ERR_GENERIC
 *    5. NULL src: CMP_ERR_SRC_NULL
 *    6. src not aligned to the sample size: CMP_ERR_GENERIC
 *    7. src_size 0 or not a multiple of the sample size: CMP_ERR_SRC_SIZE_WRONG
 *    8. a packed size (2 bytes per sample) above CMP_HDR_MAX_ORIGINAL_SIZE:
 *       CMP_ERR_HDR_ORIGINAL_TOO_LARGE
 *    9. with more than one frame, a src_stride below src_size or not a multiple
 *       of the sample size: CMP_ERR_GENERIC
 *   10. per candidate, in index order: a preprocessing outside the four
 *       CMP_ERR_PARAMS_INVALID; the error the encoder's own checks return; a
 *       MODEL candidate with a NULL model, an odd model or model_stride, or
 *       with more than one frame a model_stride below twice the samples:
 *       CMP_ERR_PARAMS_INVALID.
 *
 * Asynchronous on the engine's stream: the call does not synchronise with the
 * host, apart from engine scratch that has to grow; bits and best are valid
 * after cmp_gpu_synchronize.  Nothing outside bits[0 .. num_frames *
 * num_candidates) and best[0 .. num_frames) is written, and no byte outside
 * the 16-byte aligned hull of the batch's samples (and models) is read.
 * Build-defined extension.
 */
struct cmp_gpu_candidate {            /* one pass's parameters, as in cmp_params */
	enum cmp_preprocessing preprocessing;   /* NONE, DIFF, IWT or MODEL */
	enum cmp_encoder_type encoder_type;
	uint32_t encoder_param;
	uint32_t encoder_outlier;
};
#define CMP_GPU_ESTIMATE_MAX_CANDIDATES 64u
#define CMP_GPU_ESTIMATE_MAX_FRAMES 1048576u

struct cmp_gpu_estimate_batch {
	enum cmp_gpu_sample_type type;
	const void *src;          /* device; frame f at src + f*src_stride, 2-/4-byte aligned (16 is fastest) */
	uint64_t src_stride;      /* bytes, multiple of the sample size, >= src_size when num_frames > 1 */
	uint32_t src_size;        /* bytes per frame, as cmp_compress_*'s src_size */
	uint32_t num_frames;
	const uint16_t *model;    /* device or NULL: frame f's model (16-bit samples, as a work buffer holds
				   * them) at model + f*model_stride bytes; needed by MODEL candidates only */
	uint64_t model_stride;    /* bytes, even; >= 2 * samples when num_frames > 1 */
	const struct cmp_gpu_candidate *candidates; /* HOST, read during the call only */
	uint32_t num_candidates;
	uint64_t *bits;           /* DEVICE [num_frames * num_candidates], 8-byte aligned:
				   * bits[f*num_candidates + c] */
	uint32_t *best;           /* DEVICE [num_frames], 4-byte aligned, or NULL */
	uint32_t flags;           /* 0 */
};
uint32_t cmp_gpu_estimate(struct cmp_gpu_engine *engine, const struct cmp_gpu_estimate_batch *batch);

/* host only, no device */
uint32_t cmp_gpu_estimate_frame_size(const struct cmp_gpu_candidate *c, uint64_t bits, int checksum_enabled);

/*
 * Pack the frames of a strided batch output (frame f at frames + f*frame_stride,
 * sizes[f] bytes, as cmp_gpu_compress leaves them) back to back into out: frame
 * f at out + offsets[f], offsets 8-byte aligned, offsets[num_frames] = the
 * total.  Frames whose size is an error value take no bytes.  Reads only the
 * compressed bytes (rounded up to 8).  All pointers are device pointers;
 * out must hold the sum of the sizes rounded up to 8 each (at most
 * num_frames * frame_capacity rounded up to 8).  Asynchronous.  This is the
 * compaction step of the multi-GPU gather (shard.py); build-defined extension.
 */
uint32_t cmp_gpu_pack_frames(struct cmp_gpu_engine *engine, const void *frames, uint64_t frame_stride,
			     uint32_t frame_capacity, const uint32_t *sizes, uint32_t num_frames, void *out,
			     uint64_t *offsets);

/*
 * Multi-GPU gather of compressed frames, one call per rank
 * of an RCCL communicator the caller owns (ncclComm_t, passed as void *; one
 * process per GPU): every rank's frames (frame j of this rank at frames +
 * j*frame_stride, sizes[j] bytes, as cmp_gpu_compress leaves them; sizes and
 * frames device pointers) end up on `root`, packed at 8-byte aligned offsets
 * in `out` (device, out_capacity bytes), with out_offsets / out_sizes (host,
 * world * frames_per_rank entries) the frame table in GLOBAL frame order:
 *   CMP_GPU_LAYOUT_ROUNDROBIN  rank r's frame j is global frame r + world*j
 *   CMP_GPU_LAYOUT_BLOCK       rank r's frame j is global frame r*F + j
 *   CMP_GPU_LAYOUT_STREAMS     streams of fpc frames, stream s on rank s mod world
 * draws (host, per local frame; NULL: one each): cmp_gpu_batch.draws with
 * CMP_GPU_REPORT_DRAWS.  With CMP_GPU_GATHER_PATCH_IDS the root rewrites each
 * frame's header identifier (bytes 8..13) to what ONE process would have drawn
 * for the node's frames in global order with the reference's default counter
 * (cmp.c:27-50): id_base + the inclusive scan of the draws; a frame before its
 * context's first draw keeps its identifier.  The frame layouts refuse the
 * patch (CMP_ERR_PARAMS_INVALID on every rank) when a frame made no draw (a
 * secondary pass depends on its rank's previous frame: use STREAMS).  Every
 * rank decides from the same all-gathered table, so all ranks return the same
 * refusal; a frame with an error value is refused the same way
 * (CMP_ERR_GENERIC), and so is a root out_capacity below the packed bytes
 * (CMP_ERR_DST_TOO_SMALL).  Local failures on any rank (NULL frames / sizes,
 * the root's NULL or misaligned out, an allocation, the packing) are shared
 * through two status exchanges before the next collective, so every rank
 * returns the same value and no rank is left waiting in RCCL.  A NULL engine
 * or communicator, or a world above 256 ranks, cannot take part and returns
 * CMP_ERR_GENERIC at once (a caller error on every rank alike).  RCCL is the
 * copy the process already holds, else loaded on first use.  When the call
 * returns, the transfers and the identifier patch are complete.  Build-defined
 * extension (the C form of airs-compression_amd/shard.py).
 */
enum cmp_gpu_layout { CMP_GPU_LAYOUT_ROUNDROBIN = 0, CMP_GPU_LAYOUT_BLOCK = 1, CMP_GPU_LAYOUT_STREAMS = 2 };
#define CMP_GPU_GATHER_PATCH_IDS 0x1u
uint32_t cmp_gpu_gather(struct cmp_gpu_engine *engine, void *nccl_comm, uint32_t root, uint32_t layout, uint32_t fpc,
			const void *frames, uint64_t frame_stride, uint32_t frame_capacity, const uint32_t *sizes,
			const uint8_t *draws, uint32_t frames_per_rank, void *out, uint64_t out_capacity,
			uint64_t *out_offsets, uint32_t *out_sizes, uint64_t id_base, uint32_t flags);

/*
 * The gather's plan on the host (no device, no RCCL): from the all-gathered
 * table (entries[r * frames_per_rank + j] = size of rank r's frame j | its
 * draws << 32), the packed bytes of each rank, and in global frame order each
 * frame's offset in the root's buffer and size; ids (optional, world * F):
 * the identifier to write, or UINT64_MAX for a frame that keeps its own.
 * Returns 0, CMP_ERR_GENERIC (a frame carries an error value) or
 * CMP_ERR_PARAMS_INVALID (layout / fpc, or a frame layout with a frame that
 * made no draw while ids are requested).
 */
uint32_t cmp_gpu_gather_plan(const uint64_t *entries, uint32_t world, uint32_t frames_per_rank, uint32_t layout,
			     uint32_t fpc, uint64_t id_base, uint64_t *rank_bytes, uint64_t *offsets, uint32_t *sizes,
			     uint64_t *ids);

/* wait for all work queued on the engine */
uint32_t cmp_gpu_synchronize(struct cmp_gpu_engine *engine);

/* Fill num_frames device frames with the counter-hash synthetic signal used by
 * the benchmark (sample_bytes 2: u16; 4: i16-in-i32 with junk upper halves). */
uint32_t cmp_gpu_synthesize(struct cmp_gpu_engine *engine, void *dst, uint32_t sample_bytes,
			    uint64_t seed, uint32_t frame0, uint32_t samples_per_frame,
			    uint32_t num_frames, uint64_t stride, uint32_t noise_w);

/* non-zero when a GPU is present and the HIP runtime initialised */
int cmp_gpu_available(void);

#ifdef __cplusplus
}
#endif

#endif /* CMP_GPU_H */
