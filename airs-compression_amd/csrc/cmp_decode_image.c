/*
 * cmp_decode_image.c -- cmp_gpu_decompress_image (include/cmp_gpu.h): frames
 * as they are stored, at any byte offsets of one device buffer, decoded as one
 * context into samples packed back to back (decode_image.hip).  The
 * call-level validation returns before anything touches the device; the
 * refusals that need the headers (the output's size, the model's capacity)
 * are the device layer's, after its read-back and before it writes a sample.
 */
#include <stdint.h>

#include "cmp_errors.h"
#include "cmp_gpu.h"
#include "airs_dev.h"
#include "cmp_engine.h"

#define ERRV(name) ((uint32_t)0u - (uint32_t)CMP_ERR_##name)

uint32_t cmp_gpu_decompress_image(struct cmp_gpu_engine *engine, const struct cmp_gpu_decode_image *b)
{
	struct airs_decode_image q;

	if (!engine || !b || !b->offsets || !b->dst_offsets || !b->status || !b->num_frames)
		return ERRV(GENERIC);
	if (!b->src)
		return ERRV(SRC_NULL);
	if (!b->src_size)
		return ERRV(SRC_SIZE_WRONG);
	if (!b->dst)
		return ERRV(DST_NULL);
	if ((uintptr_t)b->dst & 1u)
		return ERRV(DST_UNALIGNED);
	if ((unsigned)b->type > CMP_GPU_I16_IN_I32 || (b->flags & ~(CMP_GPU_IMG_MODEL_IN | CMP_GPU_IMG_BIG_ENDIAN)))
		return ERRV(GENERIC);
	if (((uintptr_t)b->status & 3u) ||
	    (b->model && (!b->model_n || !b->model_samples || ((uintptr_t)b->model & 1u) || ((uintptr_t)b->model_n & 3u))))
		return ERRV(GENERIC);
	if ((b->flags & CMP_GPU_IMG_MODEL_IN) && !b->model)
		return ERRV(GENERIC);
	q.src = b->src;
	q.src_size = b->src_size;
	q.offsets = b->offsets;
	q.num_frames = b->num_frames;
	q.dst = b->dst;
	q.dst_capacity = b->dst_capacity;
	q.dst_offsets = b->dst_offsets;
	q.status = b->status;
	q.checksum_ok = b->checksum_ok;
	q.model = b->model;
	q.model_samples = b->model_samples;
	q.model_n = b->model ? b->model_n : NULL;
	q.is_unsigned = b->type == CMP_GPU_U16;
	q.model_in = (b->flags & CMP_GPU_IMG_MODEL_IN) != 0;
	q.big_endian = (b->flags & CMP_GPU_IMG_BIG_ENDIAN) != 0;
	q.chunk_bytes = engine->image_chunk;
	return airs_dev_decode_image(engine->dev, &q);
}
