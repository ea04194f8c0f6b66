/*
 * airs_dev.h -- internal C-ABI between the C host library (cmp_host.c) and
 * the HIP device layer (encode.hip).  Plain C types only.
 *
 * One launch encodes `num_frames` equally sized frames that share one set of
 * pass parameters (the reference's compress_engine, lib/compress/cmp.c:213-338,
 * run for many frames at once).  Per-frame variation (identifier, Golomb
 * parameter, model buffer) comes through optional device arrays.
 */
#ifndef AIRS_DEV_H
#define AIRS_DEV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum airs_model_mode {
	AIRS_MODEL_NONE = 0,   /* no model configured */
	AIRS_MODEL_STORE = 1,  /* primary pass: model[i] = sample[i]   (cmp.c:305-306) */
	AIRS_MODEL_UPDATE = 2  /* secondary pass: model[i] = blend(...) (cmp.c:307-310) */
};

struct airs_launch {
	/* input: frame f's samples at src + f*src_stride; 2 or 4 bytes per sample */
	const void *src;
	uint64_t src_stride;
	uint32_t sample_bytes;   /* 2 (u16/i16) or 4 (i16 in i32) */
	uint32_t is_unsigned;    /* u16: zero-extend in the model update (cmp.c:132-142) */
	uint32_t n;              /* samples per frame, >= 1 */
	uint32_t num_frames;
	/* launch frame j is batch frame frame_list[j] (device, optional) or
	 * frame_add + j*frame_mul; per-frame arrays below are indexed by the
	 * batch frame, identifiers and model pointers by the launch index j */
	const uint32_t *frame_list;
	uint32_t frame_add, frame_mul;

	/* output: frame f at dst + f*dst_stride (8-byte aligned), capacity cap */
	void *dst;
	uint64_t dst_stride;
	uint32_t cap;

	/* pass parameters (already validated by the host) */
	uint32_t preprocessing;  /* enum cmp_preprocessing: NONE, DIFF or MODEL */
	uint32_t encoder_type;   /* enum cmp_encoder_type */
	uint32_t encoder_param;  /* Golomb g (ignored for UNCOMPRESSED) */
	uint32_t outlier_param;  /* user outlier (GOLOMB_MULTI) */
	const uint32_t *frame_g; /* device, optional per-frame g (all powers of two) */
	/* CMP_GPU_AUTO_RICE (GOLOMB_ZERO after NONE or DIFF): g = 2^k per frame by
	 * the build-defined rule.  Frames of a few segments
	 * choose k inside the encode kernel (one read of the samples); otherwise
	 * the sliced Rice selection writes g for the launch's frames into frame_g_scratch
	 * (device, one word per batch frame) first */
	uint32_t auto_rice;
	uint32_t *frame_g_scratch;

	/* model (work buffer): batch frame f's model at model + (f / model_div)*model_stride,
	 * or model_ptrs[j] (device) */
	void *model;
	uint64_t model_stride;
	uint32_t model_div;
	const uint64_t *model_ptrs;
	uint32_t model_ptrs_al16; /* every model_ptrs[j] is 16-byte aligned (host-checked) */
	uint32_t model_mode;     /* enum airs_model_mode */
	uint32_t model_rate;
	uint64_t fail_bit;       /* samples reaching this frame bit keep their old model */

	/* header fields */
	const uint8_t *seqs;     /* device, optional: sequence number per batch frame (else seq) */
	uint64_t id_base;        /* identifier of launch frame j = id_base + j*id_step, or ids[j] */
	uint64_t id_step;
	const uint64_t *ids;     /* device, optional */
	uint32_t seq;            /* sequence number written in the header */
	uint32_t checksum_enabled;
	const uint32_t *checksums; /* device, per frame (airs_dev_checksum output) */

	/* results (device): status[f] = frame size or error value; needed[f] = size in
	 * bytes the frame needs (payload+header+checksum), even when it did not fit */
	uint32_t *status;
	uint32_t *needed;
};

struct airs_dev_engine;

/* create an engine on the current HIP device; stream = hipStream_t or NULL (default) */
struct airs_dev_engine *airs_dev_engine_create(void *stream);
/* engine options (cmp_gpu_engine_set_option): 0 or an error value */
#define AIRS_OPT_EXCLUSIVE 1u
#define AIRS_OPT_WALK_SEGMENT 2u
#define AIRS_OPT_NO_CONTEXT_WALK 3u
uint32_t airs_dev_set_option(struct airs_dev_engine *e, uint32_t option, uint32_t value);
void airs_dev_engine_destroy(struct airs_dev_engine *e);
void *airs_dev_engine_stream(struct airs_dev_engine *e);

/* enqueue one encode launch; returns 0 or a cmp error value (uint32_t)-code */
uint32_t airs_dev_encode(struct airs_dev_engine *e, const struct airs_launch *L);

/* MODEL streams in one launch (enc_walk.hip): context c's frames c*fpc + a
 * (a = 0 .. fpc-1) in acquisition order, the model of each context kept on
 * the chip between acquisitions and written to its work buffer once at the
 * end.  Only for batches whose passes cannot fail or fall back (the host's
 * asynchronous mode): frame (c, a) is a primary pass when the context's
 * sequence number before it is 0 or above `iters` (cmp.c:228-248).
 * Requirements (airs_dev_walk returns CMP_ERR_PARAMS_INVALID otherwise,
 * nothing launched): n a multiple of 4096; src, src_stride and every model
 * 16-byte aligned; primary NONE or DIFF; both encoders GOLOMB_ZERO or
 * GOLOMB_MULTI with g a power of two. */
struct airs_walk {
	const void *src;
	uint64_t src_stride;
	uint32_t sample_bytes, is_unsigned, n;
	uint32_t num_ctx, fpc;
	void *dst;
	uint64_t dst_stride;
	uint32_t cap;
	void *model;              /* context c's model at model + c*model_stride, or model_ptrs[c] */
	uint64_t model_stride;
	const uint64_t *model_ptrs;
	uint32_t pre_p, enc_p, g_p, outl_p; /* primary pass (outl: the user's outlier parameter) */
	uint32_t enc_s, g_s, outl_s;        /* secondary pass, MODEL preprocessing */
	uint32_t model_rate, iters;
	uint32_t seq0;            /* sequence number of every context before the call, or */
	const uint8_t *seq0s;     /* device [num_ctx] */
	uint64_t id_base, id_cstep, id_astep; /* identifier of frame (c, a) = base + c cstep + a astep, or */
	const uint64_t *ids;      /* device [num_ctx * fpc] */
	uint32_t checksum_enabled;
	const uint32_t *checksums; /* device [num_ctx * fpc] */
	uint32_t *status;         /* device [num_ctx * fpc] */
	/* uncompressed fallback on the chip (cmp.c:342-393; the context walk
	 * only): cap is the raw frame size; a frame whose coded size exceeds it is
	 * written raw (NONE + UNCOMPRESSED, sequence number 0), the model takes its
	 * samples and the context continues at sequence number 1.  The identifier
	 * draws of every frame (1 per reset: 0/1, 3 or 2 with a fallback) and the
	 * final sequence numbers are written for the host, which draws the
	 * identifiers in call order and patches the headers. */
	uint32_t fb, raw_size;
	uint8_t *draws;           /* device [num_ctx * fpc], with fb */
	uint8_t *seq_out;         /* device [num_ctx], with fb */
};
int airs_dev_walk_supported(const struct airs_walk *w);
uint32_t airs_dev_walk(struct airs_dev_engine *e, struct airs_walk *w);

/* payload-only stream (cmp_gpu_encode_stream): the n samples at src (device)
 * as ONE bit stream from bit 0 of dst, no header or checksum; *status
 * (device) = bytes or error value.  NONE/DIFF preprocessing. */
#define AIRS_STREAM_MAX 89478485u /* 48 bits per sample stay below 2^32 bits */
uint32_t airs_dev_encode_stream(struct airs_dev_engine *e, const void *src, uint32_t sample_bytes, uint32_t n,
				uint32_t preprocessing, uint32_t encoder_type, uint32_t encoder_param,
				uint32_t outlier_param, void *dst, uint32_t cap, uint32_t *status);

/* Batch fallback path on the device (cmp_gpu_compress): per-context state
 * machine of compress_engine / cmp_compress_generic (cmp.c:228-246, 342-393).
 * airs_dev_fb_step resolves step `prev` (>= 0) and plans step `cur` (>= 0);
 * airs_dev_fb_copy writes the raw frames of step `prev`'s fallbacks. */
struct airs_fb_step {
	uint32_t *state;          /* device [2 num_ctx]: sequence number, model size */
	uint32_t num_ctx, fpc;
	int32_t prev, cur;
	uint32_t packed;          /* 2 n */
	uint32_t iters;           /* secondary_iterations */
	uint32_t model_needed;    /* model_is_needed(params) */
	uint32_t fb_eligible;     /* fallback enabled and dst_capacity >= raw_size */
	uint32_t raw_size;        /* header + 2 n (+ checksum) */
	uint32_t err_floor;       /* values above are errors */
	uint32_t err_small, err_mismatch, err_too_large;
	uint32_t *flist_p, *flist_s; /* device [num_ctx]: launch lists of step cur (AIRS_NO_FRAME holes) */
	uint8_t *seqs, *draws, *kind, *fb; /* device [num frames] */
	uint32_t *status;         /* device [num frames]: the batch sizes */
	/* raw frame writer (fb_copy) */
	const void *src;
	uint64_t src_stride;
	uint32_t sample_bytes, n;
	void *dst;
	uint64_t dst_stride;
	const uint32_t *checksums;
	uint32_t checksum;
	void *model;              /* strided work buffers (context c at model + c model_stride), or */
	uint64_t model_stride;
	const uint64_t *model_ptrs; /* device [num_ctx] */
};
uint32_t airs_dev_fb_step(struct airs_dev_engine *e, const struct airs_fb_step *s);
uint32_t airs_dev_fb_copy(struct airs_dev_engine *e, const struct airs_fb_step *s);

/* frames f < num_frames of a strided buffer packed back to back at 8-byte
 * aligned offsets (offsets[f], offsets[num_frames] = total; frames whose size
 * is an error value take no bytes); reads only the compressed bytes */
uint32_t airs_dev_pack_frames(struct airs_dev_engine *e, const void *src, uint64_t src_stride,
			      uint32_t max_frame_bytes, const uint32_t *sizes, uint32_t num_frames,
			      uint32_t err_floor, void *out, uint64_t *offsets);

/* XXH32 (seed 419764627) over each frame's samples as big-endian 16-bit words */
uint32_t airs_dev_checksum(struct airs_dev_engine *e, const void *src, uint64_t src_stride,
			   uint32_t sample_bytes, uint32_t n, uint32_t num_frames,
			   const uint32_t *frame_list, uint32_t *out);
/* the same over frames of different sizes: frame f has frame_n[f] samples
 * (device; 0: no checksum wanted, out[f] is not written), n_max the largest */
uint32_t airs_dev_checksum_n(struct airs_dev_engine *e, const void *src, uint64_t src_stride,
			     uint32_t sample_bytes, uint32_t n_max, const uint32_t *frame_n,
			     uint32_t num_frames, uint32_t *out);

/* per-frame Rice parameter (build-defined rule): out_g[f] = 2^k
 * for the batch frames f = frame_list[j] (AIRS_NO_FRAME: none) or
 * frame_add + j*frame_mul, j < num_frames */
uint32_t airs_dev_select_rice(struct airs_dev_engine *e, const void *src, uint64_t src_stride,
			      uint32_t sample_bytes, uint32_t n, uint32_t num_frames,
			      const uint32_t *frame_list, uint32_t frame_add, uint32_t frame_mul,
			      uint32_t preprocessing, uint32_t *out_g);

/* counter-hash synthetic frames (bench/test inputs) */
uint32_t airs_dev_synth(struct airs_dev_engine *e, void *dst, uint32_t sample_bytes, uint64_t seed,
			uint32_t frame0, uint32_t n, uint32_t num_frames, uint64_t stride,
			uint32_t W);

/* engine-owned scratch, grown on demand (stream ordered) */
#define AIRS_NSLOT 27 /* scratch slots per engine; the last five are the device layer's (checksum
		       * placement, checksum products, decoder parse arrays, decoder frame info, IWT heads) */
#define AIRS_SLOT_GATHER 11 /* slots 11..13: cmp_gpu_gather (cmp_gather.c); 0..10 cmp_host.c */
#define AIRS_SLOT_IMAGE 14 /* slots 14..16: airs_dev_decode_image (tables, staging rows, model) */
#define AIRS_SLOT_ENCIMG 17 /* slots 17..19: cmp_gpu_compress_image (tables, with those of its ragged
			     * pieces behind them; sample rows; frame rows) */
#define AIRS_SLOT_ESTIMATE 20 /* slots 20..21: airs_dev_estimate (slice partials, IWT coefficients) */
void *airs_dev_scratch(struct airs_dev_engine *e, int slot, size_t bytes);
/* engine-owned device words for the gather's status exchanges (cmp_gather.c),
 * allocated with the engine so that taking part in an exchange never needs an
 * allocation that could fail on one rank only: 2 words in, then
 * 2 * AIRS_COLL_MAX_RANKS words out, then the poison record: two words,
 * {CMP_ERR_GENERIC, 0}, written when the engine is created (or the creation
 * fails) and never again.  A rank contributes it when the upload of its own
 * record failed, so that no peer reads what an earlier exchange left in the
 * first two words. */
#define AIRS_COLL_MAX_RANKS 256
#define AIRS_COLL_POISON (2 + 2 * AIRS_COLL_MAX_RANKS) /* word offset of the poison record */
#define AIRS_COLL_WORDS (AIRS_COLL_POISON + 2)
uint64_t *airs_dev_coll(struct airs_dev_engine *e);
/* engine-owned page-locked host scratch, grown on demand: asynchronous
 * read-backs and uploads; the host may rewrite it once the stream has passed
 * the copies that use it */
void *airs_dev_host_scratch(struct airs_dev_engine *e, size_t bytes);

/* rewrite header bytes 8..13 (identifier) of launch frames whose status is
 * not an error: frame j = frame_add + j*frame_mul, identifier ids[j] (device
 * memory, or engine host scratch read over the bus) */
uint32_t airs_dev_patch_ids(struct airs_dev_engine *e, void *dst, uint64_t dst_stride, uint32_t num_frames,
			    uint32_t frame_add, uint32_t frame_mul, const uint64_t *ids,
			    const uint32_t *status);

/* The commit of a speculative batch, without a stream wait: begin launches
 * one kernel that writes flags for the host (context c has a frame whose
 * status is an error) and the fault count, signals, then waits for the host's
 * release and patches identifiers if the release carries them (up to
 * AIRS_HCO_MAX_IDS frames, ids[f] for frame f).  wait polls for the signal
 * and copies the flags out (a fault count is returned as an error).
 * release MUST follow every successful begin (with ids, or NULL: no patch),
 * before any other wait on the stream and before anything else is queued on
 * it; it returns 1 when the identifiers are patched on the stream, 0 when the
 * caller must: NULL, more than the block holds, or a second release of the
 * same seq (wait released it on its time-out).  The kernel acknowledges
 * whether it patched; a release with ids queues a second small kernel right
 * behind it, which reads the acknowledgement on the device and patches the
 * headers when the first gave up waiting for the release.  So in stream order
 * the headers of the batch are whole after the release's kernel, from the
 * batch's own dst, status and ids: work the caller queues after the batch
 * (a copy of dst, the next batch into the same dst) sees them, and nothing of
 * the commit is left for a later wait, commit or the engine's destroy. */
#define AIRS_COMMIT_MAX_CTX 8192u /* contexts a commit kernel flags (AIRS_HCO_MAX_CTX) */
uint32_t airs_dev_commit_begin(struct airs_dev_engine *e, const uint32_t *status, uint32_t num_ctx, uint32_t fpc,
			       void *dst, uint64_t dst_stride, uint32_t *seq);
uint32_t airs_dev_commit_wait(struct airs_dev_engine *e, uint32_t seq, uint32_t num_ctx, uint8_t *flags);
int airs_dev_commit_release(struct airs_dev_engine *e, uint32_t seq, const uint64_t *ids, uint32_t total);

/* header bytes 8..13 of n frames at data + offsets[i] <- ids[i] (offsets and
 * ids device arrays): the multi-GPU gather's identifier patch */
uint32_t airs_dev_patch_ids_at(struct airs_dev_engine *e, void *data, const uint64_t *offsets, const uint64_t *ids,
			       uint64_t n);

/* decoder (decode.hip): frames at src + f*src_stride -> 16-bit samples at
 * dst + f*dst_stride bytes; status[f] = samples or error (see cmp_gpu.h) */
uint32_t airs_dev_decode(struct airs_dev_engine *e, const void *src, uint64_t src_stride, uint32_t src_cap,
			 uint32_t num_frames, uint16_t *dst, uint64_t dst_stride, uint32_t dst_samples,
			 uint32_t *status, const uint16_t *model, uint64_t model_stride);

/* whole sequences (cmp_gpu_decompress_sequences, see cmp_gpu.h): the same
 * pipeline over all num_ctx * fpc frames up to the residuals in dst, then one
 * walk per context with its model in registers.  model / model_n / checksum_ok
 * may be NULL; model_in: the contexts start from model / model_n. */
struct airs_decode_seq {
	const void *src;
	uint64_t src_stride;
	uint32_t src_cap;
	uint32_t num_ctx, fpc;
	uint16_t *dst;
	uint64_t dst_stride;
	uint32_t dst_samples;
	uint32_t *status;
	uint16_t *model;
	uint64_t model_stride;
	uint32_t *model_n;
	uint8_t *checksum_ok;
	uint32_t is_unsigned;    /* u16: zero-extend in the model update (cmp.c:132-142) */
	uint32_t model_in;
};
uint32_t airs_dev_decode_seq(struct airs_dev_engine *e, const struct airs_decode_seq *q);

/* file images (cmp_gpu_decompress_image, see cmp_gpu.h; decode_image.hip): the
 * frames at src + offsets[f], any alignment, as ONE context.  A header gather
 * and one read-back give the sizes; the host cuts the table into chunks
 * (cmp_image_plan.h) of at most chunk_bytes of staging; per chunk an unpack
 * kernel writes the frames into aligned rows, airs_dev_decode_seq decodes
 * them and an emit kernel packs the samples at dst + dst_offsets[f].  The
 * arguments are validated by the caller (cmp_decode_image.c); what needs the
 * headers is refused here, before anything is written: CMP_ERR_DST_TOO_SMALL,
 * and CMP_ERR_GENERIC for a frame larger than model_samples. */
struct airs_decode_image {
	const void *src;
	uint64_t src_size;
	const uint64_t *offsets;  /* host */
	uint32_t num_frames;
	void *dst;
	uint64_t dst_capacity;
	uint64_t *dst_offsets;    /* host [num_frames + 1] */
	uint32_t *status;
	uint8_t *checksum_ok;
	uint16_t *model;
	uint32_t model_samples;
	uint32_t *model_n;
	uint32_t is_unsigned, model_in, big_endian;
	uint64_t chunk_bytes;
};
uint32_t airs_dev_decode_image(struct airs_dev_engine *e, const struct airs_decode_image *q);

/* sample images (cmp_gpu_compress_image, see cmp_gpu.h; encode_image.hip): the
 * device work of one run of equal frames around the batch encoder, which the
 * caller (cmp_encode_image.c) runs between the two stages.  Everything is
 * queued on the engine's stream; nothing here synchronises.
 *   AIRS_ENCIMG_INGEST  frame j's frame_bytes bytes at src + offsets[j] (any
 *                       alignment) into the 16-byte aligned native row
 *                       rows + j*row_bytes, zero up to the next multiple of 16,
 *                       16-bit words byte-swapped with `swap`.
 *   AIRS_ENCIMG_EMIT    the offset scan, then the copy.  With B = out_offsets[0]
 *                       (0, written here, when first_run) and the sticky word
 *                       (0 when first_run): out_offsets[j + 1] = out_offsets[j] +
 *                       sizes[j], 0 for an error value; from the first frame
 *                       whose end passes out_capacity on, the sticky word is set,
 *                       every sizes[j] becomes CMP_ERR_DST_TOO_SMALL and the
 *                       offsets stand still.  With `force` (an error value) no
 *                       frame was encoded: every sizes[j] = force, no bytes.
 *                       Then frame row j (frows + j*frow_bytes, sizes[j] bytes)
 *                       goes to out + out_offsets[j]: whole 16-byte lines of out,
 *                       heads and tails byte by byte. */
enum airs_encimg_stage { AIRS_ENCIMG_INGEST = 0, AIRS_ENCIMG_EMIT = 1 };
struct airs_encode_image {
	uint32_t stage;
	uint32_t count;           /* frames of the run */
	/* ingest */
	const void *src;
	const uint64_t *offsets;  /* device [count] */
	uint32_t frame_bytes;
	uint32_t swap;
	void *rows;               /* 16-byte aligned */
	uint32_t row_bytes;       /* multiple of 16, >= frame_bytes rounded up to 16 */
	/* emit */
	const void *frows;        /* 8-byte aligned, readable up to 16 bytes past the last row */
	uint32_t frow_bytes;      /* multiple of 8 */
	uint32_t frow_cap;        /* the largest frame a row can hold */
	uint32_t *sizes;          /* device [count] */
	uint64_t *out_offsets;    /* device [count + 1] */
	uint32_t *sticky;         /* device word */
	void *out;
	uint64_t out_capacity;
	uint32_t first_run;
	uint32_t force;
	/* a ragged piece (frames of unequal sizes, all optional, device [count]):
	 * the ingest writes row_len[j] bytes of frame j to rows + row_off[j] (16-byte
	 * aligned; 0 bytes: the frame is read where it lies, nothing is copied) and
	 * frame_bytes is the largest row_len; the emit takes frame row j at
	 * frows + frow_off[j] (8-byte aligned) and frow_cap is the largest capacity.
	 * staged: the frames the ingest counts (those with row_len != 0). */
	const uint64_t *row_off;
	const uint32_t *row_len;
	const uint64_t *frow_off;
	uint32_t staged;
};
uint32_t airs_dev_encode_image(struct airs_dev_engine *e, const struct airs_encode_image *q);

/* One ragged encode launch (enc_ragged.hip; cmp_gpu_compress_image with
 * CMP_GPU_OPT_IMAGE_RAGGED, planned by cmp_image_plan.c): frames of different
 * sizes, one pass (NONE or DIFF, any coder, no model; a checksum only as the
 * four bytes of `checksums`, computed before the launch).  Block b
 * of the launch encodes segment desc[b].seg of the frame desc[b] describes;
 * the blocks of a frame stand in ascending segment order.  The frame arrays
 * are indexed by desc[b].frame.  Granule slots desc[b].slot0 + seg lie below
 * `slots`.  Everything is queued; nothing synchronises unless the engine's
 * look-back granules have to grow. */
struct airs_ragged_desc {
	uint64_t src;    /* device address of the frame's first sample (a multiple of sample_bytes) */
	uint32_t n;      /* samples of the frame, >= 1 */
	uint32_t seg;    /* this block's segment of the frame */
	uint32_t frame;  /* the frame's index in the frame arrays */
	uint32_t slot0;  /* the frame's first look-back granule slot (frame-major) */
	uint32_t rsv[2];
};
struct airs_ragged {
	uint32_t sample_bytes;   /* 2 or 4 */
	uint32_t frames;         /* frames the launch encodes (the counter) */
	uint32_t blocks;
	uint32_t slots;
	const struct airs_ragged_desc *desc; /* device [blocks], 32-byte aligned */
	void *dst;               /* frame j's row at dst + dst_off[j] */
	const uint64_t *dst_off; /* device, multiples of 8 */
	const uint32_t *caps;    /* device */
	const uint64_t *ids;     /* device */
	const uint8_t *seqs;     /* device */
	uint32_t preprocessing, encoder_type, encoder_param, outlier_param;
	uint32_t *status;        /* device: frame size or error value */
	const uint32_t *checksums; /* device, per frame, or NULL: frame j ends with checksums[j] big-endian
				    * (clipped to its capacity), 4 bytes larger, the header's checksum bit set */
};
uint32_t airs_dev_encode_ragged(struct airs_dev_engine *e, const struct airs_ragged *q);
/* samples per segment of the ragged kernel for samples of sample_bytes bytes */
uint32_t airs_dev_ragged_segment(uint32_t sample_bytes);

/* Host-side counters of the process, counted where the kernel is launched:
 * ragged encode launches, the frames they encoded, their blocks.  Copies the
 * first min(n, AIRS_RAGGED_STAT_COUNT) counters to out and returns
 * AIRS_RAGGED_STAT_COUNT.  For tests; nothing in the library reads them. */
enum airs_ragged_stat {
	AIRS_RAGGED_STAT_LAUNCHES = 0,
	AIRS_RAGGED_STAT_FRAMES = 1,
	AIRS_RAGGED_STAT_BLOCKS = 2,
	AIRS_RAGGED_STAT_COUNT = 3
};
uint32_t airs_dev_ragged_stats(uint64_t *out, uint32_t n);

/* XXH32 (seed 419764627) over frames of different sizes that lie anywhere
 * (checksum.hip): out[j] is what airs_dev_checksum gives for
 * the n[j] samples at src[j], as big-endian 16-bit words (of 4-byte samples the
 * low halves).  A product kernel writes frame j's stripes x P2 to the engine's
 * checksum-products scratch at byte off[j]; a chain kernel, four lanes per
 * frame and sixteen frames per wave, consumes them.  The host lays the
 * products out (cmp_image_ck_layout, cmp_image_plan.h): `bytes` is their sum,
 * blocks the product kernel's workgroups.  Everything is queued; nothing
 * synchronises unless the scratch has to grow. */
struct airs_ragged_ck_block {
	uint32_t frame, qb; /* round quads [256 qb, 256 qb + 256) of the frame (struct cmp_image_ck_block) */
};
struct airs_ragged_ck {
	uint32_t sample_bytes;  /* 2 or 4 */
	uint32_t frames;
	const uint64_t *src;    /* device [frames]: address of the frame's first sample, a multiple of
				 * sample_bytes at any 16-byte phase */
	const uint32_t *n;      /* device [frames]: samples, >= 1 */
	const uint64_t *off;    /* device [frames]: byte offset of the frame's products, a multiple of 16 */
	uint64_t bytes;         /* products of all frames */
	const struct airs_ragged_ck_block *blocks; /* device [num_blocks] */
	uint32_t num_blocks;    /* may be 0: no frame has 8 samples */
	uint32_t *out;          /* device [frames] */
};
uint32_t airs_dev_checksum_ragged(struct airs_dev_engine *e, const struct airs_ragged_ck *q);

/* Host-side counters of the process: ragged checksum launches (calls of
 * airs_dev_checksum_ragged) and the frames they covered.  Copies the first
 * min(n, AIRS_RAGGED_CK_STAT_COUNT) counters to out and returns
 * AIRS_RAGGED_CK_STAT_COUNT.  For tests; nothing in the library reads them. */
enum airs_ragged_ck_stat {
	AIRS_RAGGED_CK_STAT_LAUNCHES = 0,
	AIRS_RAGGED_CK_STAT_FRAMES = 1,
	AIRS_RAGGED_CK_STAT_COUNT = 2
};
uint32_t airs_dev_ragged_ck_stats(uint64_t *out, uint32_t n);

/* Host-side counters of the process, counted where the kernels are launched:
 * frames that went through the ingest copy (a run read where it lies adds
 * none), frames handed to the emit copy, frames of refused runs (the scan
 * alone).  Copies the first min(n, AIRS_ENCIMG_STAT_COUNT) counters to out and
 * returns AIRS_ENCIMG_STAT_COUNT.  For tests; nothing in the library reads
 * them. */
enum airs_encimg_stat {
	AIRS_ENCIMG_STAT_INGEST = 0,
	AIRS_ENCIMG_STAT_EMIT = 1,
	AIRS_ENCIMG_STAT_REFUSED = 2,
	AIRS_ENCIMG_STAT_COUNT = 3
};
uint32_t airs_dev_encode_image_stats(uint64_t *out, uint32_t n);

/* payload-only stream (cmp_gpu_decode_stream, see cmp_gpu.h): the frame
 * pipeline over one "frame" described by the arguments instead of a header
 * (no header kernel, no read-back; the parse rounds synchronise), then the end
 * check: the n-th codeword ends in the stream's last byte and only zero bits
 * follow.  g and outlier as cmp_coder_resolve leaves them (g = 1 for
 * UNCOMPRESSED).  src_size at most AIRS_STREAM_DECODE_MAX: every 32-bit bit
 * position, range end ((s + 1) * 512 of the last subsequence) and parse exit
 * (at most 48 bits past the end) then stays below 2^32 - 1, the parse's
 * sentinel.  Scratch: 16 bytes per 512-bit subsequence (a quarter of
 * src_size, 128 MiB at the limit), 8 per workgroup and 2 per 4096 samples. */
#define AIRS_STREAM_DECODE_MAX 536870400u /* bytes: 2^32 - 4096 bits */
uint32_t airs_dev_decode_stream(struct airs_dev_engine *e, const void *src, uint32_t src_size, uint32_t n,
				uint32_t preprocessing, uint32_t encoder_type, uint32_t g, uint32_t outlier,
				uint16_t *dst, uint32_t *status);

/* the IWT coefficients of L's frames into L->model (the model addressing of the
 * launch), as ahead of an IWT encode launch: what airs_dev_estimate sizes */
uint32_t airs_dev_iwt(struct airs_dev_engine *e, const struct airs_launch *L);

/* sizing (cmp_gpu_estimate, see cmp_gpu.h; estimate.hip): bits[f * num_cand + c]
 * = the payload bits of frame f under candidate c, best[f] (optional) = the c
 * that minimises 8 * hdr + bits, ties to the lowest c.  The candidates come
 * resolved (cmp_estimate.c): everything is validated by the caller.  Queued on
 * the engine's stream; nothing synchronises unless scratch has to grow. */
enum airs_est_kind {
	AIRS_EST_RAW = 0,     /* UNCOMPRESSED: 16 bits a sample */
	AIRS_EST_ZERO_P2 = 1, /* GOLOMB_ZERO, g = 2^k: k + 1 + min((m + 1) >> k, 16) */
	AIRS_EST_ZERO = 2,    /* GOLOMB_ZERO, any other g */
	AIRS_EST_MULTI = 3    /* GOLOMB_MULTI */
};
struct airs_est_cand {
	uint32_t kind;    /* enum airs_est_kind */
	uint32_t pre;     /* enum cmp_preprocessing */
	uint32_t k;       /* floor(log2 g) */
	uint32_t cutoff;  /* 2^(k+1) - g */
	uint32_t outlier; /* as cmp_coder_resolve leaves it */
	uint32_t g;
	uint32_t rcp;     /* airs_rcp_u32(g, 65537); not used when g is a power of two (shift) */
	uint32_t hdr;     /* header bytes of a frame of this candidate: 16 or 22 */
};
struct airs_estimate {
	const void *src;
	uint64_t src_stride;
	uint32_t sample_bytes, n, num_frames;
	const uint16_t *model;
	uint64_t model_stride;
	const struct airs_est_cand *cand; /* host */
	uint32_t num_cand;
	uint64_t *bits;
	uint32_t *best;
};
uint32_t airs_dev_estimate(struct airs_dev_engine *e, const struct airs_estimate *q);

/* Host-side counters of the process, counted where the kernels are launched:
 * sizing launches (one per group of candidates and chunk of frames), finishing
 * launches (one per chunk), IWT transforms (one per chunk with an IWT
 * candidate).  Copies the first min(n, AIRS_EST_STAT_COUNT) counters to out and
 * returns AIRS_EST_STAT_COUNT.  For tests; nothing in the library reads them. */
enum airs_est_stat {
	AIRS_EST_STAT_SIZE = 0,
	AIRS_EST_STAT_FINISH = 1,
	AIRS_EST_STAT_IWT = 2,
	AIRS_EST_STAT_COUNT = 3
};
uint32_t airs_dev_estimate_stats(uint64_t *out, uint32_t n);

/* plain memory helpers on the engine stream */
void *airs_dev_malloc(size_t bytes);
void airs_dev_free(void *p);
uint32_t airs_dev_h2d(struct airs_dev_engine *e, void *dst, const void *src, size_t bytes);
uint32_t airs_dev_d2h(struct airs_dev_engine *e, void *dst, const void *src, size_t bytes);
uint32_t airs_dev_sync(struct airs_dev_engine *e);
uint32_t airs_dev_memset(struct airs_dev_engine *e, void *dst, int v, size_t bytes);
/* rows of `width` bytes, device to device: dst + r*dpitch <- src + r*spitch */
uint32_t airs_dev_d2d_rows(struct airs_dev_engine *e, void *dst, size_t dpitch, const void *src, size_t spitch,
			   size_t width, size_t rows);

/* Host-side launch counters of the process (every engine, every thread),
 * counted where the kernel is launched: which kernel family and look-back
 * mode a call took.  Copies the first min(n, AIRS_STAT_COUNT) counters to out
 * and returns how many that is: counters are only ever added at the end, so a
 * caller that knows the first n of them gets n whatever the library has since
 * gained, and one that asks for more than the library has sees that it got
 * fewer.  For tests; nothing in the library reads them. */
enum airs_launch_stat {
	AIRS_STAT_RICE_FRAME_LB1 = 0, /* rice_kernel, frames, lbmode bit 0 set (scalar look-back from sif 16) */
	AIRS_STAT_RICE_FRAME_LB0 = 1, /* rice_kernel, frames, lbmode 0 (vector look-back) */
	AIRS_STAT_RICE_STREAM = 2,    /* rice_kernel, payload-only stream */
	AIRS_STAT_RICE_AUTO = 3,      /* rice_kernel with the candidate barrier (CMP_GPU_AUTO_RICE) */
	AIRS_STAT_ENCODE = 4,         /* encode_kernel, frames (its fused AUTO form included) */
	AIRS_STAT_ENCODE_STREAM = 5,  /* encode_kernel, payload-only stream */
	AIRS_STAT_DECODE_ROUND = 6,   /* dec_parse_kernel, a settle round (first == 0); not the speculative launch */
	AIRS_STAT_WALK_CTX = 7,       /* walk_ctx_kernel: MODEL contexts, one workgroup per context (fallback on the chip) */
	AIRS_STAT_WALK_SEG = 8,       /* walk_kernel: MODEL contexts, the segment walk */
	AIRS_STAT_FB_STEP = 9,        /* fb_step_kernel: a step of the per-acquisition device state machine */
	AIRS_STAT_COUNT = 10
};
uint32_t airs_dev_launch_stats(uint64_t *out, uint32_t n);

/* non-zero when a HIP device is usable */
int airs_dev_available(void);
const char *airs_dev_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* AIRS_DEV_H */
