/*
 * cmp_decode_seq.c -- cmp_gpu_decompress_sequences (include/cmp_gpu.h): whole
 * sequences of frames, MODEL frames included, decoded in one call with each
 * context's model rebuilt on the device (decode.hip).  The call-level
 * validation mirrors cmp_gpu_decompress (cmp_host.c) and returns before
 * anything touches the device.
 */
#include <stdint.h>

#include "cmp_errors.h"
#include "cmp_gpu.h"
#include "airs_dev.h"
#include "cmp_engine.h"

#define ERRV(name) ((uint32_t)0u - (uint32_t)CMP_ERR_##name)
#define HDR_MAX_SIZE 22u /* base header + extension (cmp_header.h) */

uint32_t cmp_gpu_decompress_sequences(struct cmp_gpu_engine *engine, const struct cmp_gpu_decode_seq_batch *b)
{
	struct airs_decode_seq q;
	uint64_t frames;

	if (!engine || !b || !b->src || !b->dst || !b->status || !b->num_ctx || !b->frames_per_ctx)
		return ERRV(GENERIC);
	frames = (uint64_t)b->num_ctx * b->frames_per_ctx;
	if (frames > 65535u || (unsigned)b->type > CMP_GPU_I16_IN_I32 || (b->flags & ~CMP_GPU_SEQ_MODEL_IN))
		return ERRV(GENERIC);
	if (((uintptr_t)b->src & 7u) || (b->src_stride & 7u) || b->src_capacity < HDR_MAX_SIZE ||
	    (b->src_capacity & 3u) || (frames > 1 && b->src_stride < b->src_capacity))
		return ERRV(GENERIC);
	/* the chain reads the next frames' rows while it writes the current one's */
	if (((uintptr_t)b->dst & 1u) || (b->dst_stride & 1u) || (frames > 1 && b->dst_stride < 2u * (uint64_t)b->dst_samples))
		return ERRV(GENERIC);
	if (b->model && (!b->model_n || ((uintptr_t)b->model & 1u) || (b->model_stride & 1u) ||
			 ((uintptr_t)b->model_n & 3u) ||
			 (b->num_ctx > 1 && b->model_stride < 2u * (uint64_t)b->dst_samples)))
		return ERRV(GENERIC);
	if ((b->flags & CMP_GPU_SEQ_MODEL_IN) && !b->model)
		return ERRV(GENERIC);
	q.src = b->src;
	q.src_stride = b->src_stride;
	q.src_cap = b->src_capacity;
	q.num_ctx = b->num_ctx;
	q.fpc = b->frames_per_ctx;
	q.dst = b->dst;
	q.dst_stride = b->dst_stride;
	q.dst_samples = b->dst_samples;
	q.status = b->status;
	q.model = b->model;
	q.model_stride = b->model_stride;
	q.model_n = b->model ? b->model_n : NULL;
	q.checksum_ok = b->checksum_ok;
	q.is_unsigned = b->type == CMP_GPU_U16;
	q.model_in = (b->flags & CMP_GPU_SEQ_MODEL_IN) != 0;
	return airs_dev_decode_seq(engine->dev, &q);
}
