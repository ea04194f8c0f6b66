/*
 * cmp_encode_image.c -- cmp_gpu_compress_image (include/cmp_gpu.h): sample
 * frames as they are stored, at any byte offsets of one device buffer and of
 * unequal sizes, compressed as one context into a packed .air image.  The
 * call-level validation returns before anything touches the device.  The
 * table is cut into runs of equal frames (cmp_image_plan.c); every run goes
 * through the batch path of cmp_gpu_compress (cmp_batch_compress, cmp_batch.c)
 * between the copies of encode_image.hip: the ingest into aligned native rows
 * (skipped when the samples can be read where they are), then the offset scan
 * and the emit of the frame rows into the image.
 */
#include <stdint.h>
#include <string.h>

#include "cmp.h"
#include "cmp_errors.h"
#include "cmp_gpu.h"
#include "airs_dev.h"
#include "cmp_engine.h"
#include "cmp_image_plan.h"

#define ERRV(name) ((uint32_t)0u - (uint32_t)CMP_ERR_##name)
#define BATCH_FLAGS (CMP_GPU_AUTO_RICE | CMP_GPU_HOST_STEPPED | CMP_GPU_STEPWISE)

static uint32_t up16(uint32_t v)
{
	return (v + 15u) & ~15u;
}

/* what the loop's cmp_compress_* call answers for frames of fb bytes before it
 * looks at the context (0: it goes on), and the capacity the loop gives them */
static uint32_t frame_refusal(uint32_t fb, uint32_t sample_bytes, uint32_t *bound)
{
	*bound = 0;
	if (!fb || fb % sample_bytes)
		return ERRV(SRC_SIZE_WRONG);
	*bound = cmp_compress_bound(fb);
	if (cmp_is_error(*bound)) {
		*bound = 0;
		return ERRV(GENERIC); /* an error value as dst_capacity (cmp.c:350) */
	}
	return 0;
}

/* The batch path can read the run's samples where they are: native-endian, the
 * first frame aligned to the sample size, the offsets an arithmetic
 * progression whose step is at least the frame and a multiple of the sample
 * size. */
static int run_direct(const struct cmp_gpu_encode_image *img, const struct cmp_image_run *r, uint32_t sample_bytes,
		      uint64_t *stride)
{
	const uint64_t *o = img->offsets + r->first;
	const uint32_t fb = img->frame_bytes[r->first];
	uint32_t j;

	if ((img->flags & CMP_GPU_IMG_SRC_BIG_ENDIAN) || ((uintptr_t)img->src + o[0]) % sample_bytes)
		return 0;
	*stride = fb;
	if (r->count == 1)
		return 1;
	if (o[1] < o[0] || o[1] - o[0] < fb || (o[1] - o[0]) % sample_bytes)
		return 0;
	*stride = o[1] - o[0];
	for (j = 2; j < r->count; j++)
		if (o[j] < o[j - 1] || o[j] - o[j - 1] != *stride)
			return 0;
	return 1;
}

uint32_t cmp_gpu_compress_image(struct cmp_gpu_engine *engine, struct cmp_context *ctx,
				const struct cmp_gpu_encode_image *img)
{
	struct cmp_image_run r;
	struct airs_dev_engine *dev;
	uint64_t f, N, stride = 0;
	size_t rows_bytes = 0, frows_bytes = 0;
	uint32_t sample_bytes, bound, e, staged = 0, first_run = 1;
	uint8_t *tables, *rows = NULL, *frows;
	uint64_t *d_off;

	if (!engine || !ctx || !img || !img->offsets || !img->frame_bytes || !img->out_offsets || !img->sizes ||
	    !img->num_frames)
		return ERRV(GENERIC);
	if (!img->src)
		return ERRV(SRC_NULL);
	if (!img->src_size)
		return ERRV(SRC_SIZE_WRONG);
	N = img->num_frames;
	for (f = 0; f < N; f++)
		if (img->offsets[f] > img->src_size || img->frame_bytes[f] > img->src_size - img->offsets[f])
			return ERRV(SRC_SIZE_WRONG);
	if (!img->out)
		return ERRV(DST_NULL);
	if (((uintptr_t)img->out_offsets & 7u) || ((uintptr_t)img->sizes & 3u))
		return ERRV(GENERIC);
	if ((unsigned)img->type > CMP_GPU_I16_IN_I32 || (img->flags & ~CMP_GPU_IMG_SRC_BIG_ENDIAN) ||
	    (img->batch_flags & ~(BATCH_FLAGS | CMP_GPU_REPORT_DRAWS)))
		return ERRV(GENERIC);
	if (img->batch_flags & CMP_GPU_REPORT_DRAWS)
		return ERRV(GENERIC);
	if ((img->flags & CMP_GPU_IMG_SRC_BIG_ENDIAN) && img->type == CMP_GPU_I16_IN_I32)
		return ERRV(GENERIC);
	e = cmp_context_usable(ctx);
	if (e)
		return e;
	dev = engine->dev;
	sample_bytes = img->type == CMP_GPU_I16_IN_I32 ? 4u : 2u;

	/* the rows of the largest run, allocated once: growing them between runs
	 * would wait for the stream */
	for (f = 0; f < N; f += r.count) {
		const uint32_t fb = img->frame_bytes[f];
		const uint32_t refused = frame_refusal(fb, sample_bytes, &bound);
		size_t need;

		cmp_image_run_next(img->frame_bytes, N, engine->image_chunk, cmp_image_run_row(fb, bound), 0, f, &r);
		if (refused)
			continue;
		need = (size_t)r.count * ((bound + 7u) & ~7u);
		frows_bytes = need > frows_bytes ? need : frows_bytes;
		if (run_direct(img, &r, sample_bytes, &stride))
			continue;
		staged = 1;
		need = (size_t)r.count * up16(fb);
		rows_bytes = need > rows_bytes ? need : rows_bytes;
	}
	/* the sticky word, then the offsets of the frames in src */
	tables = airs_dev_scratch(dev, AIRS_SLOT_ENCIMG, 8u + (staged ? (size_t)N * 8u : 0u));
	frows = airs_dev_scratch(dev, AIRS_SLOT_ENCIMG + 2, frows_bytes + 16u);
	if (staged)
		rows = airs_dev_scratch(dev, AIRS_SLOT_ENCIMG + 1, rows_bytes);
	if (!tables || !frows || (staged && !rows))
		return ERRV(GENERIC);
	d_off = (uint64_t *)(tables + 8u);
	/* Straight from the caller's pageable table, as the batch path uploads its
	 * identifiers (cmp_batch.c): the runtime has staged a pageable source when
	 * the copy call returns.  The engine's page-locked scratch is no place for
	 * it: this call does not wait, and the next call on the engine may rewrite
	 * that scratch while the copy is still queued. */
	if (staged && airs_dev_h2d(dev, d_off, img->offsets, (size_t)N * 8u))
		return ERRV(GENERIC);

	for (f = 0; f < N; f += r.count) {
		const uint32_t fb = img->frame_bytes[f];
		const uint32_t refused = frame_refusal(fb, sample_bytes, &bound);
		struct airs_encode_image q;

		cmp_image_run_next(img->frame_bytes, N, engine->image_chunk, cmp_image_run_row(fb, bound), 0, f, &r);
		memset(&q, 0, sizeof(q));
		q.count = r.count;
		if (!refused) {
			struct cmp_gpu_batch b;

			memset(&b, 0, sizeof(b));
			b.type = img->type;
			if (run_direct(img, &r, sample_bytes, &stride)) {
				b.src = (const uint8_t *)img->src + img->offsets[f];
				b.src_stride = stride;
			} else {
				q.stage = AIRS_ENCIMG_INGEST;
				q.src = img->src;
				q.offsets = d_off + f;
				q.frame_bytes = fb;
				q.swap = (img->flags & CMP_GPU_IMG_SRC_BIG_ENDIAN) != 0;
				q.rows = rows;
				q.row_bytes = up16(fb);
				e = airs_dev_encode_image(dev, &q);
				if (e)
					return e;
				b.src = rows;
				b.src_stride = q.row_bytes;
			}
			b.src_size = fb;
			b.dst = frows;
			b.dst_stride = (bound + 7u) & ~7u;
			b.dst_capacity = bound;
			b.sizes = img->sizes + f;
			b.flags = img->batch_flags;
			e = cmp_batch_compress(engine, ctx, 1, r.count, &b);
			if (e)
				return e;
		}
		q.stage = AIRS_ENCIMG_EMIT;
		q.frows = frows;
		q.frow_bytes = (bound + 7u) & ~7u;
		q.frow_cap = bound;
		q.sizes = img->sizes + f;
		q.out_offsets = img->out_offsets + f;
		q.sticky = (uint32_t *)tables;
		q.out = img->out;
		q.out_capacity = img->out_capacity;
		q.first_run = first_run;
		q.force = refused;
		e = airs_dev_encode_image(dev, &q);
		if (e)
			return e;
		first_run = 0;
	}
	return 0;
}
