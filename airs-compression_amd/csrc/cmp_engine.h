/* cmp_engine.h -- the opaque cmp_gpu_engine of include/cmp_gpu.h (private to
 * the library's host code: cmp_host.c, cmp_batch.c, cmp_gather.c, cmp_decode_seq.c,
 * cmp_decode_stream.c, cmp_decode_image.c, cmp_encode_image.c, cmp_estimate.c) */
#ifndef CMP_ENGINE_H
#define CMP_ENGINE_H

#include "cmp_gpu.h"
#include "airs_dev.h"

struct cmp_gpu_engine {
	struct airs_dev_engine *dev;
	uint32_t image_chunk; /* CMP_GPU_OPT_IMAGE_CHUNK (cmp_decode_image.c, cmp_encode_image.c); 0: the default */
	uint32_t image_ragged; /* CMP_GPU_OPT_IMAGE_RAGGED (cmp_encode_image.c): 0 off, 1 on, else the keep threshold in bytes */
	uint32_t image_ragged_ck; /* CMP_GPU_OPT_IMAGE_RAGGED_CHECKSUM (cmp_encode_image.c): 0 or 1 */
};

/* The encoder's own parameter checks (reference encoder.c:185-224), cmp_host.c:
 * 0, or the error value the encoder returns for (type, g, outlier); *resolved
 * (optional) receives the outlier the coder works with and a frame's header
 * carries. */
uint32_t cmp_coder_resolve(uint32_t type, uint32_t g, uint32_t outlier, uint32_t *resolved);

/* The batch path behind cmp_gpu_compress (cmp_batch.c), with its validation:
 * cmp_gpu_compress_image runs every run of equal frames through it
 * (cmp_encode_image.c). */
uint32_t cmp_batch_compress(struct cmp_gpu_engine *eng, struct cmp_context *ctx, uint32_t num_ctx, uint32_t fpc,
			    const struct cmp_gpu_batch *b);

/* what the batch path refuses a context for at call level, before it touches
 * the device: 0, CMP_ERR_CONTEXT_INVALID or CMP_ERR_WORK_BUF_UNALIGNED */
uint32_t cmp_context_usable(const struct cmp_context *ctx);

#endif /* CMP_ENGINE_H */
