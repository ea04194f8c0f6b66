/*
 * cmp_image_plan.c -- the host side of cmp_gpu_decompress_image that needs no
 * device: cmp_gpu_frame_table (include/cmp_gpu.h), the walk over an image of
 * back-to-back frames, and the chunk planner; and the run planner of
 * cmp_gpu_compress_image.  Nothing here includes HIP or the device layer, so
 * a stand-alone program links this file alone
 * (tests/sanitize/image_plan_fuzz.c, encode_plan_fuzz.c).
 */
#include <stddef.h>
#include <stdint.h>

#include "cmp_gpu.h"
#include "cmp_image_plan.h"

#define HDR_MIN 16u /* the base header (cmp_header.h) */

uint64_t cmp_gpu_frame_table(const void *image, uint64_t size, uint64_t *offsets, uint64_t max_frames,
			     uint64_t *bad_at)
{
	const uint8_t *p = image;
	uint64_t pos = 0, count = 0, bad = UINT64_MAX;

	while (p && pos < size) {
		uint32_t fs;

		if (size - pos < HDR_MIN) {
			bad = pos;
			break;
		}
		fs = (uint32_t)p[pos + 2] << 16 | (uint32_t)p[pos + 3] << 8 | p[pos + 4];
		if (fs < HDR_MIN || fs > size - pos) {
			bad = pos;
			break;
		}
		if (offsets && count < max_frames)
			offsets[count] = pos;
		count++;
		pos += fs;
	}
	if (!p && size)
		bad = 0;
	if (bad_at)
		*bad_at = bad;
	return count;
}

static uint32_t up16(uint32_t v)
{
	return (v + 15u) & ~15u;
}

void cmp_image_plan_next(const uint32_t *frames, uint64_t num_frames, uint64_t budget, uint64_t first,
			 struct cmp_image_chunk *chunk)
{
	/* the model a chunk receives holds as many samples as the frame before it */
	uint32_t cap = CMP_IMAGE_ROW_MIN, nmax = first ? frames[2 * (first - 1) + 1] : 1u;
	uint64_t f, count = 0;

	if (!budget)
		budget = CMP_IMAGE_CHUNK_DEFAULT;
	if (!nmax)
		nmax = 1u;
	for (f = first; f < num_frames && count < CMP_IMAGE_CHUNK_FRAMES; f++, count++) {
		const uint32_t c = up16(frames[2 * f]), n = frames[2 * f + 1];
		const uint32_t ncap = c > cap ? c : cap, nn = n > nmax ? n : nmax;

		if (count && (count + 1u) * ((uint64_t)ncap + up16(2u * nn)) > budget)
			break;
		cap = ncap;
		nmax = nn;
	}
	chunk->first = first;
	chunk->count = (uint32_t)count;
	chunk->src_cap = cap;
	chunk->dst_samples = nmax;
	chunk->dst_stride = up16(2u * nmax);
}

uint64_t cmp_image_run_row(uint32_t frame_bytes, uint32_t bound)
{
	return (((uint64_t)frame_bytes + 15u) & ~(uint64_t)15u) + (((uint64_t)bound + 7u) & ~(uint64_t)7u);
}

void cmp_image_run_next(const uint32_t *frame_bytes, uint64_t num_frames, uint64_t budget, uint64_t row_bytes,
			uint32_t max_frames, uint64_t first, struct cmp_image_run *run)
{
	const uint32_t size = frame_bytes[first];
	uint64_t count = 1, most;

	if (!budget)
		budget = CMP_IMAGE_CHUNK_DEFAULT;
	if (!max_frames || max_frames > CMP_IMAGE_RUN_FRAMES)
		max_frames = CMP_IMAGE_RUN_FRAMES;
	most = row_bytes ? budget / row_bytes : max_frames;
	if (most > max_frames)
		most = max_frames;
	while (count < most && first + count < num_frames && frame_bytes[first + count] == size)
		count++;
	run->first = first;
	run->count = (uint32_t)count;
}
