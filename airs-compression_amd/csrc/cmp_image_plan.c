/*
 * cmp_image_plan.c -- the host side of cmp_gpu_decompress_image that needs no
 * device: cmp_gpu_frame_table (include/cmp_gpu.h), the walk over an image of
 * back-to-back frames, and the chunk planner; and the run planner of
 * cmp_gpu_compress_image with the piece planner and the block table of its
 * ragged launches, and the layout of the ragged checksum's products.
 * Nothing here includes HIP or the device layer, so a stand-alone program
 * links this file alone
 * (tests/sanitize/image_plan_fuzz.c, encode_plan_fuzz.c, ragged_plan_fuzz.c,
 * ragged_ck_layout_fuzz.c).
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

/* The count of the run cmp_image_run_next cuts at frame f (max_frames 0),
 * without walking the stretch of equal frames again for every f: *eq_end is
 * the end of the stretch an earlier call walked (0 at first), and f lies in
 * that stretch while f < *eq_end. */
static uint64_t run_count(const uint32_t *frame_bytes, const uint32_t *bound, uint64_t num_frames, uint64_t budget,
			  uint64_t f, uint64_t *eq_end)
{
	const uint64_t row = cmp_image_run_row(frame_bytes[f], bound[f]);
	uint64_t most = row ? budget / row : CMP_IMAGE_RUN_FRAMES, count;

	if (*eq_end <= f) {
		uint64_t e = f + 1;

		while (e < num_frames && frame_bytes[e] == frame_bytes[f])
			e++;
		*eq_end = e;
	}
	if (most > CMP_IMAGE_RUN_FRAMES)
		most = CMP_IMAGE_RUN_FRAMES;
	count = *eq_end - f < most ? *eq_end - f : most;
	return count ? count : 1;
}

static int run_kept(uint64_t count, uint32_t frame_bytes, uint64_t keep_bytes)
{
	return count >= 2 && count * frame_bytes >= keep_bytes;
}

void cmp_image_piece_next(const uint32_t *frame_bytes, const uint32_t *bound, uint64_t num_frames, uint64_t budget,
			  uint64_t keep_bytes, uint32_t max_frames, uint64_t first, struct cmp_image_piece *piece)
{
	uint64_t eq_end = 0, count, sum, f;

	if (!budget)
		budget = CMP_IMAGE_CHUNK_DEFAULT;
	if (!max_frames || max_frames > CMP_IMAGE_RAGGED_FRAMES)
		max_frames = CMP_IMAGE_RAGGED_FRAMES;
	piece->first = first;
	count = run_count(frame_bytes, bound, num_frames, budget, first, &eq_end);
	if (!bound[first] || run_kept(count, frame_bytes[first], keep_bytes)) {
		piece->kind = bound[first] ? CMP_IMAGE_PIECE_RUN : CMP_IMAGE_PIECE_REFUSED;
		piece->count = (uint32_t)count;
		return;
	}
	sum = cmp_image_run_row(frame_bytes[first], bound[first]);
	for (f = first + 1; f < num_frames && f - first < max_frames; f++) {
		const uint64_t row = cmp_image_run_row(frame_bytes[f], bound[f]);

		if (!bound[f] || row > budget || sum > budget - row)
			break;
		if (run_kept(run_count(frame_bytes, bound, num_frames, budget, f, &eq_end), frame_bytes[f], keep_bytes))
			break;
		sum += row;
	}
	piece->kind = CMP_IMAGE_PIECE_RAGGED;
	piece->count = (uint32_t)(f - first);
}

uint64_t cmp_image_ragged_blocks(const uint32_t *segs, uint32_t count, uint32_t *active,
				 struct cmp_image_block *blocks)
{
	uint64_t total = 0;
	uint32_t j, live = 0, s;

	for (j = 0; j < count; j++) {
		total += segs[j];
		if (blocks && segs[j])
			active[live++] = j;
	}
	if (!blocks)
		return total;
	/* round s: the frames that have a segment s, in table order; those that
	 * have a segment s + 1 too stay for the next round */
	for (s = 0, total = 0; live; s++) {
		uint32_t i, keep = 0;

		for (i = 0; i < live; i++) {
			j = active[i];
			blocks[total].frame = j;
			blocks[total++].seg = s;
			if (segs[j] > s + 1u)
				active[keep++] = j;
		}
		live = keep;
	}
	return total;
}

uint64_t cmp_image_ck_region(uint32_t n)
{
	const uint64_t stripes = n / 8u;

	return (stripes + 3u) / 4u * CMP_IMAGE_CK_QUAD;
}

uint64_t cmp_image_ck_layout(const uint32_t *frame_bytes, uint32_t sample_bytes, uint32_t count, uint64_t *off,
			     struct cmp_image_ck_block *blocks, uint64_t *num_blocks)
{
	uint64_t at = 0, nb = 0;
	uint32_t j;

	for (j = 0; j < count; j++) {
		const uint64_t region = cmp_image_ck_region(frame_bytes[j] / sample_bytes);
		const uint64_t quads = region / CMP_IMAGE_CK_QUAD;
		uint64_t qb;

		if (off)
			off[j] = at;
		at += region;
		for (qb = 0; qb * CMP_IMAGE_CK_BLOCK_QUADS < quads; qb++, nb++) {
			if (blocks) {
				blocks[nb].frame = j;
				blocks[nb].qb = (uint32_t)qb;
			}
		}
	}
	if (num_blocks)
		*num_blocks = nb;
	return at;
}
