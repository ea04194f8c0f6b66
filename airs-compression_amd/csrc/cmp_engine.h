/* cmp_engine.h -- the opaque cmp_gpu_engine of include/cmp_gpu.h (private to
 * the library's host code: cmp_host.c, cmp_gather.c, cmp_decode_seq.c,
 * cmp_decode_stream.c, cmp_decode_image.c) */
#ifndef CMP_ENGINE_H
#define CMP_ENGINE_H

#include "airs_dev.h"

struct cmp_gpu_engine {
	struct airs_dev_engine *dev;
	uint32_t image_chunk; /* CMP_GPU_OPT_IMAGE_CHUNK (cmp_decode_image.c); 0: the default */
};

/* The encoder's own parameter checks (reference encoder.c:185-224), cmp_host.c:
 * 0, or the error value the encoder returns for (type, g, outlier); *resolved
 * (optional) receives the outlier the coder works with and a frame's header
 * carries. */
uint32_t cmp_coder_resolve(uint32_t type, uint32_t g, uint32_t outlier, uint32_t *resolved);

#endif /* CMP_ENGINE_H */
