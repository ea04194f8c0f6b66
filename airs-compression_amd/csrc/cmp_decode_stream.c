/*
 * cmp_decode_stream.c -- cmp_gpu_decode_stream (include/cmp_gpu.h): the
 * inverse of cmp_gpu_encode_stream, one header-less bit stream back into its
 * 16-bit samples (decode.hip).  What a frame's header tells the frame
 * decoders comes from the caller here; the encoder arguments are resolved by
 * the encoder's own checks (cmp_coder_resolve, cmp_host.c).  The call-level
 * validation returns before anything touches the device.
 */
#include <stdint.h>

#include "cmp_errors.h"
#include "cmp_gpu.h"
#include "airs_dev.h"
#include "cmp_engine.h"

#define ERRV(name) ((uint32_t)0u - (uint32_t)CMP_ERR_##name)

uint32_t cmp_gpu_decode_stream(struct cmp_gpu_engine *engine, const void *src, uint32_t src_size,
			       uint32_t num_samples, enum cmp_preprocessing preprocessing,
			       enum cmp_encoder_type encoder_type, uint32_t encoder_param, uint32_t encoder_outlier,
			       uint16_t *dst, uint32_t *status)
{
	uint32_t e, outlier = 0;

	if (!engine || !status)
		return ERRV(GENERIC);
	if (!src)
		return ERRV(SRC_NULL);
	if ((uintptr_t)src & 7u)
		return ERRV(GENERIC);
	if (!dst)
		return ERRV(DST_NULL);
	if ((uintptr_t)dst & 1u)
		return ERRV(DST_UNALIGNED);
	if (num_samples == 0 || num_samples > AIRS_STREAM_MAX)
		return ERRV(SRC_SIZE_WRONG);
	if (src_size == 0 || src_size > CMP_GPU_STREAM_DECODE_MAX)
		return ERRV(SRC_SIZE_WRONG);
	if (preprocessing != CMP_PREPROCESS_NONE && preprocessing != CMP_PREPROCESS_DIFF)
		return ERRV(PARAMS_INVALID);
	/* the encoder's own checks (encoder.c:185-224) */
	e = cmp_coder_resolve(encoder_type, encoder_param, encoder_outlier, &outlier);
	if (e > ERRV(MAX_CODE))
		return e;
	return airs_dev_decode_stream(engine->dev, src, src_size, num_samples, preprocessing, encoder_type,
				      encoder_type == CMP_ENCODER_UNCOMPRESSED ? 1u : encoder_param, outlier, dst,
				      status);
}
