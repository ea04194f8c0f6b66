/* cmp_image_plan.h -- host planning of cmp_gpu_decompress_image and
 * cmp_gpu_compress_image (cmp_image_plan.c): free of the device, so that a
 * stand-alone program can link it. */
#ifndef CMP_IMAGE_PLAN_H
#define CMP_IMAGE_PLAN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CMP_IMAGE_CHUNK_DEFAULT (256ull << 20) /* bytes of staging per chunk (CMP_GPU_OPT_IMAGE_CHUNK 0) */
#define CMP_IMAGE_CHUNK_FRAMES 65535u          /* frames per chunk at most: one decoder call */
#define CMP_IMAGE_ROW_MIN 32u                  /* a staged frame row holds the largest header, in 16-byte units */

/* one decoder call: frames [first, first + count) staged in rows of src_cap
 * bytes and decoded into rows of dst_stride bytes */
struct cmp_image_chunk {
	uint64_t first;
	uint32_t count;       /* 1 .. CMP_IMAGE_CHUNK_FRAMES */
	uint32_t src_cap;     /* multiple of 16, >= CMP_IMAGE_ROW_MIN and every frame's compressed size */
	uint32_t dst_samples; /* >= 1, every frame's samples and those of frame first - 1 (the model
			       * that comes in from the chunk before may be that large) */
	uint32_t dst_stride;  /* 2 * dst_samples rounded up to 16 */
};

/* The chunk that starts at frame `first` < num_frames.  frames[2 f] is frame
 * f's compressed size (0: an unusable slice, which still takes a row) and
 * frames[2 f + 1] its samples.  The chunk takes frames while
 * count * (src_cap + dst_stride) stays within `budget` (0: the default) and
 * count within CMP_IMAGE_CHUNK_FRAMES; it always takes one. */
void cmp_image_plan_next(const uint32_t *frames, uint64_t num_frames, uint64_t budget, uint64_t first,
			 struct cmp_image_chunk *chunk);

#define CMP_IMAGE_RUN_FRAMES 0xFFFFFFFu /* frames per run at most: what one cmp_gpu_compress call accepts */

/* one batch call of cmp_gpu_compress_image: frames [first, first + count), all
 * of frame_bytes[first] bytes */
struct cmp_image_run {
	uint64_t first;
	uint32_t count; /* 1 .. CMP_IMAGE_RUN_FRAMES */
};

/* the staging a frame of `frame_bytes` bytes of samples takes: its sample row
 * (frame_bytes rounded up to 16) and its frame row (`bound`, the frame's
 * cmp_compress_bound, rounded up to 8) */
uint64_t cmp_image_run_row(uint32_t frame_bytes, uint32_t bound);

/* The run that starts at frame `first` < num_frames: the maximal stretch of
 * consecutive frames with frame_bytes[f] == frame_bytes[first], cut so that
 * count * row_bytes (cmp_image_run_row of the run's frames) stays within
 * `budget` (0: the default) and count within max_frames (0, or anything above
 * it: CMP_IMAGE_RUN_FRAMES); it always takes one frame. */
void cmp_image_run_next(const uint32_t *frame_bytes, uint64_t num_frames, uint64_t budget, uint64_t row_bytes,
			uint32_t max_frames, uint64_t first, struct cmp_image_run *run);

#ifdef __cplusplus
}
#endif

#endif /* CMP_IMAGE_PLAN_H */
